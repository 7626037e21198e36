"""`-m gpu`: hr_png_decode / PngDecoder / load_png against the host build of the same header (png.decode_host) and against the fixtures'
expectations (tests/png_decode_common.py): equality of bytes and of statuses, no tolerance anywhere.  The damaged files here are ones
on which the CPU suite's sanitizer-clean host build already returned a status; the decoder's loops are bounded by construction, so
those cases check error reporting and nothing else."""
import numpy as np
import pytest
import torch

import png_common as P
import png_decode_common as D
from hyperreel_amd import png

pytestmark = pytest.mark.gpu

MAX_IMAGES = 16


def _groups(cases):
    """{(w, h): [(name, data, {mode: pixels})]}: a decoder takes one size, a batch mixes the colour types of that size"""
    out = {}
    for name, data, want in cases:
        out.setdefault(D.size_of(data), []).append((name, data, want))
    return out


def _cases(kind):
    if kind == 'golden':
        return D.golden_files()
    return [(n, d, {m: D.convert(im, m) for m in D.MODES}) for n, d, im in (D.hand_files() if kind == 'hand' else D.own_files())]


@pytest.mark.parametrize('mode', list(D.MODES))
@pytest.mark.parametrize('kind', ['golden', 'hand', 'own'])
def test_exact_pixels(kind, mode):
    """batches of 1, 3 and max_images files of mixed colour types: the device's bytes equal the expectation and the host build's, and
    every status is 0"""
    checked = 0
    assert len(_cases(kind)) >= {'golden': 300, 'hand': 60, 'own': 30}[kind]
    for (w, h), group in _groups(_cases(kind)).items():
        dec = png.PngDecoder(w, h, max_images=min(len(group), MAX_IMAGES), max_file_bytes=sum(len(d) for _, d, _ in group))
        batches = [group[:1], group[:3]] + [group[i:i + dec.max_images] for i in range(0, len(group), dec.max_images)]
        for batch in batches:
            files_dev, offsets_dev = dec.upload([d for _, d, _ in batch])
            out, status = dec.decode_device(files_dev, offsets_dev, len(batch), mode)
            assert not status.cpu().numpy().any(), (w, h, status.cpu().numpy())
            got = out.cpu().numpy()
            for i, (name, data, want) in enumerate(batch):
                assert np.array_equal(got[i], want[mode]), (name, mode)
                checked += 1
        for name, data, want in group[::5]:
            host, st = png.decode_host(data, mode, with_status=True)
            assert st == D.OK and np.array_equal(host, want[mode]), name
        dec.close()
    assert checked >= len(_cases(kind))


@pytest.mark.parametrize('name', ['far_match', 'far_match_32767', 'flat_run', 'one_byte_idat', 'empty_idat', 'cuts_l9_huffman', 'cuts_l0_default'])
def test_window_edge_long_run_and_chunk_boundaries(name):
    """the distance-32768 and -32767 files (the window wraps under their matches; at 32767 a match overwrites its own source slots), the
    distance-1 length-258 file, IDAT chunks of one byte"""
    data, im = next((d, im) for n, d, im in D.hand_files() if n == name)
    h, w, c = im.shape
    dec = png.PngDecoder(w, h, max_images=2, max_file_bytes=2 * len(data))
    got = dec.decode([data, data], 'RGB').cpu().numpy()
    assert np.array_equal(got[0], D.convert(im, 'RGB')) and np.array_equal(got[1], got[0])
    dec.close()


@pytest.mark.parametrize('c', P.CHANNELS)
def test_round_trip_on_the_device_in_one_graph(c):
    """decode(encode(frame)) == to8b(frame), both calls captured in one graph and replayed three times over a refilled frame; the frame
    is wider than one strip budget, so the encoder cuts a row a strip and the decoder meets as many IDAT chunks"""
    w, h = P.shapes(c)[-1]
    mode = {1: 'L', 3: 'RGB', 4: 'RGBA'}[c]
    enc = png.PngEncoder(w, h, c)
    dec = png.PngDecoder(w, h, max_images=1, max_file_bytes=enc.bound)
    frame = torch.zeros((h, w, c), dtype=torch.float32, device='cuda')
    file = torch.zeros(enc.bound, dtype=torch.uint8, device='cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    offsets = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = torch.empty((1, h, w, c), dtype=torch.uint8, device='cuda')
    status = torch.empty(1, dtype=torch.int32, device='cuda')

    def both():
        enc.encode_device(frame, out=file, length=length)
        offsets[1:].copy_(length)
        dec.decode_device(file, offsets, 1, mode, out=out, status=status)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for content in ('disc', 'noise', 'ramp'):
        x = P.as_float(P.image(content, w, h, c))
        frame.copy_(torch.from_numpy(x).cuda())
        g.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == D.OK
        assert np.array_equal(out.cpu().numpy()[0], P.to8b_reference(x)), content
    enc.close()
    dec.close()


@pytest.mark.parametrize('mode', ['RGB', 'RGBA'])
def test_into_the_feed(mode, tmp_path):
    """load_png's tensor goes through DeviceResize as it is and equals the resize of PIL's decode of the same files"""
    import io
    from PIL import Image
    from hyperreel_amd.data import DeviceResize
    group = [c for c in D.golden_files() if D.size_of(c[1]) == (130, 70)][::4][:6]
    paths = []
    for i, (name, data, _) in enumerate(group):
        paths.append(str(tmp_path / f'{i}.png'))
        with open(paths[-1], 'wb') as f:
            f.write(data)
    images = png.load_png(paths, mode)
    pil = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert(mode)) for _, d, _ in group])
    assert images.dtype == torch.uint8 and images.is_cuda and np.array_equal(images.cpu().numpy(), pil)
    step = DeviceResize((130, 70), (65, 35), 'lanczos', max_images=len(group), mode=mode)
    got, want = step(images).cpu().numpy(), step(pil).cpu().numpy()
    step.close()
    assert np.array_equal(got, want)
    direct = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert(mode).resize((65, 35), Image.LANCZOS)) for _, d, _ in group])
    assert np.array_equal(got, direct)


DAMAGED = ['flipped_crc', 'flipped_adler', 'truncated_mid_idat', 'filter_byte_7', 'header_16_bit']


def test_damaged_files_report_their_status():
    """each damaged file between two undamaged ones: the host build's status and a zero image for it, exact pixels for its neighbours"""
    dm = D.damaged_files()
    good, im = dm['good']
    w, h = dm['size']
    files = [good]
    for name in DAMAGED:
        files += [dm['files'][name], good]
    dec = png.PngDecoder(w, h, max_images=len(files))
    files_dev, offsets_dev = dec.upload(files)
    out = torch.full((len(files), h, w, 3), 0xA5, dtype=torch.uint8, device='cuda')
    out, status = dec.decode_device(files_dev, offsets_dev, len(files), 'RGB', out=out)
    got, st = out.cpu().numpy(), status.cpu().numpy()
    for i, data in enumerate(files):
        host, host_st = png.decode_host(data, 'RGB', size=(w, h), with_status=True)
        assert st[i] == host_st and np.array_equal(got[i], host), i
        if i % 2 == 0:
            assert st[i] == D.OK and np.array_equal(got[i], im)
        else:
            assert st[i] == D.DAMAGED_STATUS[DAMAGED[i // 2]] and not got[i].any()
    with pytest.raises(png.PngDecodeError) as e:
        dec.decode(files, 'RGB')
    assert e.value.index == 1 and e.value.status_name == 'BAD_CRC'
    dec.close()


def test_empty_batch_and_refused_calls():
    """n_images = 0 launches nothing and leaves out and status alone; bad arguments are refused on the host before any launch"""
    dec = png.PngDecoder(17, 9, max_images=2)
    files_dev, offsets_dev = dec.upload([D.damaged_files()['good'][0]])
    out, status = dec.decode_device(files_dev, offsets_dev, 0, 'RGB')
    torch.cuda.synchronize()
    assert out.shape == (0, 9, 17, 3) and status.numel() == 0
    from hyperreel_amd import lib
    one = torch.zeros(2 * 9 * 17 * 3, dtype=torch.uint8, device='cuda')
    st = torch.zeros(3, dtype=torch.int32, device='cuda')
    for args in ((3, 3), (-1, 3), (1, 2)):
        with pytest.raises(RuntimeError):
            lib.call('hr_png_decode', dec._h, files_dev, offsets_dev, args[0], args[1], one, st, lib.stream(dec.device), device=dec.device)
    with pytest.raises(RuntimeError):
        lib.call('hr_png_decode', dec._h, None, offsets_dev, 1, 3, one, st, lib.stream(dec.device), device=dec.device)
    with pytest.raises(ValueError):
        dec.decode([b''] * 3)
    assert png.probe(D.damaged_files()['good'][0])[:5] == (17, 9, 8, 2, 3) and png.probe(D.damaged_files()['files']['header_16_bit']).supported is False
    dec.close()
