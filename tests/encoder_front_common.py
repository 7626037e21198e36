"""What tests/test_gpu_png.py and tests/test_gpu_jpeg_encode.py ask of the front end the two encoders share (hyperreel_amd/_codec.py's
Encoder): each passes its own encoders, device frames and expected bytes."""
import pytest
import torch


def two_encoders_on_two_streams(encs, frames, expect):
    """the same frame twice through one encoder, then both encoders on a stream each, three rounds: expect[i] from encs[i] every time"""
    assert encs[0].encode(frames[0]) == expect[0] and encs[0].encode(frames[0]) == expect[0]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for e, f, s in zip(encs, frames, streams):
            with torch.cuda.stream(s):
                outs.append(e.encode_device(f))
    torch.cuda.synchronize()
    for i, (buf, length) in enumerate(outs):
        assert buf[:int(length.item())].cpu().numpy().tobytes() == expect[i % 2]
    for e in encs:
        e.close()


def graph_capture_replays_over_a_changing_frame(enc, inputs):
    """one captured encode_device, three replays with the float frame refilled from `inputs` between them: the eager bytes each time"""
    frame = torch.zeros((enc.height, enc.width, enc.channels), dtype=torch.float32, device='cuda')
    out = torch.empty(enc.bound, dtype=torch.uint8, device='cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    eager = [enc.encode(x) for x in inputs]
    assert len(set(eager)) == 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode_device(frame, out=out, length=length)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc.encode_device(frame, out=out, length=length)
    for x, expect in zip(inputs, eager):
        frame.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert out[:int(length.item())].cpu().numpy().tobytes() == expect
    enc.close()


def front_end_refusals(enc):
    """a 3-channel encoder takes neither an (H, W, 4) frame nor a float64 one"""
    assert enc.channels == 3
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((enc.height, enc.width, 4), device='cuda'))
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((enc.height, enc.width, 3), dtype=torch.float64, device='cuda'))
