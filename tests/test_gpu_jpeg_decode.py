"""`-m gpu`: hr_jpeg_decode / JpegDecoder / load_jpeg / data.load_images against the fixtures' expectations (PIL's arrays,
tests/jpeg_decode_common.py) and against the host build of the same header (jpeg.decode_host): equality of bytes, of statuses and of
rounds, no tolerance anywhere.  The damaged files here are ones on which the CPU suite's sanitizer-clean host build already returned a
status; the decoder's loops are bounded by construction, so those cases check error reporting and nothing else."""
import numpy as np
import pytest
import torch

import jpeg_decode_common as D
from hyperreel_amd import jpeg

pytestmark = pytest.mark.gpu

MAX_IMAGES = 16
_host = {}


def _host_decode(data, mode, size, subseq_bits):
    """the host build's (pixels, status, rounds), computed once per case"""
    key = (data, mode, size, subseq_bits)
    if key not in _host:
        _host[key] = jpeg.decode_host(data, mode, size=size, with_status=True, subseq_bits=subseq_bits, with_rounds=True)
    return _host[key]


def _groups(cases):
    out = {}
    for name, size, data, want in cases:
        out.setdefault(size, []).append((name, data, want))
    return out


def _run(dec, files, mode):
    files_dev, offsets_dev = dec.upload(files)
    rounds = torch.full((len(files),), -1, dtype=torch.int32, device='cuda')
    out = torch.full((len(files), dec.height, dec.width, D.MODES[mode]), 0xA5, dtype=torch.uint8, device='cuda')
    out, status = dec.decode_device(files_dev, offsets_dev, len(files), mode, out=out, rounds=rounds)
    return out.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()


@pytest.mark.parametrize('subseq_bits', [0, 128])
@pytest.mark.parametrize('mode', list(D.MODES))
@pytest.mark.parametrize('kind', ['golden', 'hand'])
def test_exact_pixels(kind, mode, subseq_bits):
    """batches per size that mix subsamplings, table sets (default and optimised) and restart layouts: the device's bytes equal PIL's,
    every status is 0, and statuses and rounds equal the host build's"""
    cases = D.golden_files() if kind == 'golden' else D.hand_files()
    checked = 0
    for (w, h), group in _groups(cases).items():
        dec = jpeg.JpegDecoder(w, h, max_images=min(len(group), MAX_IMAGES), max_file_bytes=MAX_IMAGES * max(len(d) for _, d, _ in group),
                               subseq_bits=subseq_bits)
        batches = [group[:1]] + [group[i:i + dec.max_images] for i in range(0, len(group), dec.max_images)]
        for batch in batches:
            got, st, rounds = _run(dec, [d for _, d, _ in batch], mode)
            assert not st.any(), (w, h, st)
            for i, (name, data, want) in enumerate(batch):
                assert np.array_equal(got[i], want[mode]), (name, mode)
                checked += 1
            for i, (name, data, want) in list(enumerate(batch))[::3]:
                host, host_st, host_rounds = _host_decode(data, mode, (w, h), subseq_bits)
                assert host_st == st[i] and host_rounds == rounds[i] and np.array_equal(host, got[i]), (name, rounds[i], host_rounds)
        dec.close()
    assert checked >= len(cases)


@pytest.mark.parametrize('name', ['w33_h31_420_noise_q100', 'w130_h70_grey_noise_q95_rst1', 'w130_h70_420_noise_q95', 'w1_h1_420_noise_q95',
                                  'w7_h1_422_noise_q100', 'w64_h33_422_noise_q30_rstrows'])
def test_unit_boundaries(name):
    """quality-100 noise at 128 bits: many stuffed FF 00 pairs, some at a subsequence's first byte; a restart interval of one block: units
    shorter than a subsequence and the RSTn counter wrapping; 1 x 1 and 7 x 1: a whole scan inside one subsequence"""
    data, want = D.named(name)
    w, h = want['RGB'].shape[1], want['RGB'].shape[0]
    lo, eoi = D.scan_range(data)
    if name == 'w33_h31_420_noise_q100':
        scan = data[lo:eoi]
        assert any(scan[k] == 0 and scan[k - 1] == 0xFF for k in range(16, len(scan), 16)), 'no stuffing byte at a subsequence start'
    if name in ('w1_h1_420_noise_q95', 'w7_h1_422_noise_q100'):
        assert eoi - lo <= 128
    dec = jpeg.JpegDecoder(w, h, max_images=2, max_file_bytes=2 * len(data), subseq_bits=128)
    got, st, rounds = _run(dec, [data, data], 'RGB')
    host, host_st, host_rounds = _host_decode(data, 'RGB', (w, h), 128)
    assert list(st) == [D.OK, D.OK] and host_st == D.OK
    assert np.array_equal(got[0], want['RGB']) and np.array_equal(got[1], want['RGB'])
    assert list(rounds) == [host_rounds, host_rounds]
    dec.close()


DAMAGED = ['no_soi', 'overlong_segment', 'progressive', 'other_size', 'no_dht', 'sixteen_ones', 'rst_out_of_order', 'cut_in_scan', 'two_bytes_more']


def test_damaged_files_report_their_status():
    """each damaged file between two undamaged ones: the host build's status and a zero image for it, exact pixels for its neighbours"""
    dm = D.damaged_files()
    good, im = dm['good']
    w, h = dm['size']
    files = [good]
    for name in DAMAGED:
        files += [dm['files'][name], good]
    dec = jpeg.JpegDecoder(w, h, max_images=len(files), subseq_bits=128)
    got, st, rounds = _run(dec, files, 'RGB')
    for i, data in enumerate(files):
        host, host_st, host_rounds = _host_decode(data, 'RGB', (w, h), 128)
        assert st[i] == host_st and rounds[i] == host_rounds and np.array_equal(got[i], host), i
        if i % 2 == 0:
            assert st[i] == D.OK and np.array_equal(got[i], im)
        else:
            assert st[i] == D.DAMAGED_STATUS[DAMAGED[i // 2]] and not got[i].any()
    with pytest.raises(jpeg.JpegDecodeError) as e:
        dec.decode(files, 'RGB')
    assert e.value.index == 1 and e.value.status_name == 'NO_SOI'
    # offsets that do not describe the batch: that image alone is refused (image 0 now runs on into its neighbours' bytes, after its EOI)
    files_dev, offsets_dev = dec.upload([good, good, good])
    offsets_dev[1] = offsets_dev[2] + 1
    out, status = dec.decode_device(files_dev, offsets_dev, 3, 'RGB')
    st, got = status.cpu().numpy(), out.cpu().numpy()
    assert list(st) == [D.OK, D.BAD_OFFSETS, D.OK] and np.array_equal(got[0], im) and np.array_equal(got[2], im) and not got[1].any()
    dec.close()


def test_mutated_files_match_the_host_build():
    """a batch of seeded single-byte mutations: statuses, rounds and pixels are the host build's"""
    data = D.mutation_sources()[0]
    files = D.mutations(data, 32, 77)
    dec = jpeg.JpegDecoder(17, 13, max_images=len(files), subseq_bits=128)
    got, st, rounds = _run(dec, files, 'RGB')
    for i, bad in enumerate(files):
        host, host_st, host_rounds = _host_decode(bad, 'RGB', (17, 13), 128)
        assert st[i] == host_st and rounds[i] == host_rounds and np.array_equal(got[i], host), i
    dec.close()


def test_graph_capture_and_replay():
    """decode_device captured in one graph; replayed after the files are refilled it gives the second batch's pixels"""
    group = _groups(D.golden_files())[(33, 31)]
    first, second = group[:4], group[4:8]
    dec = jpeg.JpegDecoder(33, 31, max_images=4, max_file_bytes=4 * max(len(d) for _, d, _ in group))
    files_dev, offsets_dev = dec.upload([d for _, d, _ in first])
    out = torch.zeros((4, 31, 33, 3), dtype=torch.uint8, device='cuda')
    status = torch.zeros(4, dtype=torch.int32, device='cuda')
    rounds = torch.zeros(4, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.decode_device(files_dev, offsets_dev, 4, 'RGB', out=out, status=status, rounds=rounds)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dec.decode_device(files_dev, offsets_dev, 4, 'RGB', out=out, status=status, rounds=rounds)
    for batch in (second, first, second):
        again_files, again_offsets = dec.upload([d for _, d, _ in batch])
        assert again_files.data_ptr() == files_dev.data_ptr() and again_offsets.data_ptr() == offsets_dev.data_ptr()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any()
        for i, (name, data, want) in enumerate(batch):
            assert np.array_equal(out[i].cpu().numpy(), want['RGB']), name
    dec.close()


def test_into_the_feed(tmp_path):
    """load_jpeg -> reference_resize -> DeviceRaySet batch equals the same chain fed with PIL's decoded array; load_images takes a PNG
    list and a JPEG list and refuses a mixed one by name"""
    import io
    from PIL import Image
    from hyperreel_amd.data import DeviceRaySet, load_images, reference_resize
    group = [c for c in _groups(D.golden_files())[(130, 70)] if '_grey_' not in c[0]][:4]
    jpgs, pngs = [], []
    for i, (name, data, want) in enumerate(group):
        jpgs.append(str(tmp_path / f'{i}.jpg'))
        with open(jpgs[-1], 'wb') as f:
            f.write(data)
        pngs.append(str(tmp_path / f'{i}.png'))
        Image.fromarray(want['RGB']).save(pngs[-1])
    pil = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for _, d, _ in group])
    images = jpeg.load_jpeg(jpgs, 'RGB')
    assert images.dtype == torch.uint8 and images.is_cuda and np.array_equal(images.cpu().numpy(), pil)
    small, small_pil = reference_resize(images, (65, 35)), reference_resize(pil, (65, 35), device='cuda')
    assert np.array_equal(small.cpu().numpy(), small_pil.cpu().numpy())
    K = np.array([[60.0, 0, 32.5], [0, 60.0, 17.5], [0, 0, 1]], np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32)[:3], (len(group), 1, 1))
    elements = torch.arange(0, len(group) * 65 * 35, 7, dtype=torch.int64, device='cuda')
    batches = []
    for imgs in (small, small_pil):
        rays = DeviceRaySet(imgs, poses, K, None, None, (65, 35))
        b = rays.batch(0, 0, indices=elements)
        batches.append({k: b[k].cpu().numpy() for k in ('coords', 'rgb', 'weight')})
        rays.close()
    assert all(np.array_equal(batches[0][k].view(np.uint32), batches[1][k].view(np.uint32)) for k in batches[0])
    want = small_pil.cpu().numpy().reshape(-1, 3)[elements.cpu().numpy()].astype(np.float32) / np.float32(255)
    assert np.array_equal(batches[0]['rgb'], want)
    assert np.array_equal(load_images(jpgs, 'RGB').cpu().numpy(), pil) and np.array_equal(load_images(pngs, 'RGB').cpu().numpy(), pil)
    with pytest.raises(ValueError, match='1.png'):
        load_images([jpgs[0], pngs[1]])


def test_empty_batch_and_refused_calls():
    """n_images = 0 launches nothing; bad arguments are refused on the host before any launch"""
    from hyperreel_amd import lib
    good = D.damaged_files()['good'][0]
    dec = jpeg.JpegDecoder(17, 13, max_images=2)
    files_dev, offsets_dev = dec.upload([good])
    out, status = dec.decode_device(files_dev, offsets_dev, 0, 'RGB')
    torch.cuda.synchronize()
    assert out.shape == (0, 13, 17, 3) and status.numel() == 0
    one = torch.zeros(2 * 13 * 17 * 3, dtype=torch.uint8, device='cuda')
    st = torch.zeros(3, dtype=torch.int32, device='cuda')
    for n, c in ((3, 3), (-1, 3), (1, 2)):
        with pytest.raises(RuntimeError):
            lib.call('hr_jpeg_decode', dec._h, files_dev, offsets_dev, n, c, one, st, None, lib.stream(dec.device), device=dec.device)
    with pytest.raises(RuntimeError):
        lib.call('hr_jpeg_decode', dec._h, None, offsets_dev, 1, 3, one, st, None, lib.stream(dec.device), device=dec.device)
    with pytest.raises(ValueError):
        dec.decode([b''] * 3)
    for bits in (100, 96, 130, -32):
        with pytest.raises(RuntimeError):
            jpeg.JpegDecoder(17, 13, subseq_bits=bits)
    info = jpeg.probe(good)
    assert (info.width, info.height, info.components, info.h_samp, info.v_samp, info.supported) == (17, 13, 3, 2, 2, True)
    assert jpeg.probe(D.refused_files()['progressive']).supported is False and jpeg.probe(D.refused_files()['cmyk']).status == D.UNSUPPORTED
    with pytest.raises(RuntimeError):
        jpeg.probe(b'\x89PNG\r\n\x1a\n')
    dec.close()
