"""LPIPS without a GPU: hr_lpips_scores against its ctypes mirror and the entry points bound in lib.py; hyperreel_amd/csrc/hr_lpips.h,
compiled for the host, against torch -- every layer's shape on both nets over a sweep of sizes, the minimum sizes, the workspace bytes,
the weight packer's index map; the state-dict key mapping and its errors; and the oracle's own sanity (tests/lpips_oracle.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lpips_oracle as LO
from helpers import build_host_lib
from hyperreel_amd import lib
from hyperreel_amd import lpips as HL

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_math', 'hr_lpips_host.cpp')
OUT = os.path.join(HERE, 'host_math', '_build', 'libhr_lpips_host.so')
HEADERS = [os.path.join(HERE, '..', 'hyperreel_amd', 'csrc', 'hr_lpips.h'), os.path.join(HERE, '..', 'include', 'hyperreel_hip.h')]
NETS = {'alex': 0, 'vgg': 1}
CAP = 1e-5


@pytest.fixture(scope='module')
def hl():
    build_host_lib(OUT, SRC, [SRC, *HEADERS])
    m = C.CDLL(OUT)
    m.hlp_layer.argtypes = [C.c_int, C.c_int, C.c_void_p]
    m.hlp_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    m.hlp_packed_elems.argtypes = [C.c_int, C.c_int]
    m.hlp_packed_elems.restype = C.c_int64
    m.hlp_pack_src.argtypes = [C.c_int, C.c_int, C.c_void_p]
    m.hlp_pack_dst.argtypes = [C.c_int, C.c_int, C.c_void_p]
    m.hlp_pack_src.restype = m.hlp_pack_dst.restype = None
    return m


def _layers(hl, net):
    out = []
    for i in range(hl.hlp_n_layers(NETS[net])):
        v = np.zeros(7, np.int32)
        hl.hlp_layer(NETS[net], i, v.ctypes.data_as(C.c_void_p))
        out.append(dict(zip(('kind', 'cin', 'cout', 'k', 'stride', 'pad', 'tap'), (int(x) for x in v))))
    return out


def _plan(hl, net, h, w):
    n = hl.hlp_n_layers(NETS[net])
    hs, ws, slots, sizes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(10, np.int64), np.zeros(3, np.int64)
    ok = hl.hlp_plan(NETS[net], h, w, *[a.ctypes.data_as(C.c_void_p) for a in (hs, ws, slots, sizes)])
    return ok, hs, ws, slots, sizes


# ---- the ABI
def test_hr_lpips_scores_layout_matches_c(hl):
    assert hl.hlp_scores_sizeof() == C.sizeof(lib.hr_lpips_scores) == 48
    assert [n for n, _ in lib.hr_lpips_scores._fields_] == ['layer', 'total']
    assert hl.hlp_scores_offset(0) == lib.hr_lpips_scores.layer.offset == 0
    assert hl.hlp_scores_offset(1) == lib.hr_lpips_scores.total.offset == 40
    assert (hl.hlp_net_number(0), hl.hlp_net_number(1)) == (lib.HR_LPIPS_ALEX, lib.HR_LPIPS_VGG) == (0, 1)


def test_lpips_entry_points_are_bound_at_abi_27(hl):
    assert lib.ABI_VERSION == 27 == hl.hlp_abi_version()
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    p = C.POINTER(C.c_void_p)
    assert bound['hr_lpips_create'] == (C.c_int, [C.c_int32, p, p, p, p])
    assert bound['hr_lpips_destroy'] == (None, [C.c_void_p])
    assert bound['hr_lpips_workspace'] == (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32])
    assert bound['hr_lpips'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])


def test_library_sizes_the_workspace_and_refuses_before_any_launch(hl):
    """No GPU: the workspace size is host arithmetic, and these argument checks come before anything touches the device."""
    L = lib.load()
    for net in NETS:
        m = HL.MIN_SIZE[net]
        assert L.hr_lpips_workspace(NETS[net], m - 1, 64) == 0 and L.hr_lpips_workspace(NETS[net], 64, m - 1) == 0
        assert L.hr_lpips_workspace(NETS[net], m, m) > 0
        for h, w in ((m, m), (67, 93), (800, 800), (1088, 2048)):
            ok, _, _, _, sizes = _plan(hl, net, h, w)
            assert ok and L.hr_lpips_workspace(NETS[net], h, w) == sizes[2], (net, h, w)
            assert HL.workspace_doubles(net, h, w) * 8 >= sizes[2]
        assert L.hr_lpips_workspace(NETS[net], 40000, 40000) == 0                 # 2 h w passes int32
    assert L.hr_lpips_workspace(2, 64, 64) == 0 and L.hr_lpips_workspace(-1, 64, 64) == 0
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.hr_lpips(None, p, p, 64, 64, p, p, None) == -1 and b'null' in L.hr_last_error()
    h = C.c_void_p()
    arr = (C.c_void_p * 13)(*[p.value] * 13)
    assert L.hr_lpips_create(2, arr, arr, arr, C.byref(h)) == -1 and b'unknown net' in L.hr_last_error() and not h.value
    assert L.hr_lpips_create(0, None, arr, arr, C.byref(h)) == -1 and b'null' in L.hr_last_error()
    assert L.hr_lpips_create(0, arr, arr, arr, None) == -1
    holes = (C.c_void_p * 13)(*([p.value] * 3 + [None] + [p.value] * 9))
    assert L.hr_lpips_create(0, holes, arr, arr, C.byref(h)) == -1 and b'convolution 3' in L.hr_last_error() and not h.value
    L.hr_lpips_destroy(None)


def test_python_surface_refuses_the_cpu():
    sd, lin = LO.weights('alex')
    with pytest.raises(RuntimeError, match='no CPU path'):
        HL.Lpips('alex', sd, lin, device='cpu')
    with pytest.raises(ValueError, match="one of"):
        HL.workspace_doubles('squeeze', 64, 64)


# ---- hr_lpips.h against torch
def test_layer_tables_are_the_two_backbones(hl):
    for net in NETS:
        layers = _layers(hl, net)
        assert len(layers) == len(LO.LAYERS[net]) and hl.hlp_n_convs(NETS[net]) == len(HL.CONVS[net])
        convs = [l for l in layers if l['kind'] == 0]
        assert [(l['cin'], l['cout'], l['k']) for l in convs] == HL.CONVS[net]
        assert [l['cout'] for l in convs if l['tap'] >= 0] == HL.TAP_CHANNELS[net] and [l['tap'] for l in convs if l['tap'] >= 0] == [0, 1, 2, 3, 4]
        for l, o in zip(layers, LO.LAYERS[net]):
            if o[0] == 'conv':
                assert (l['kind'], l['stride'], l['pad'], l['tap']) == (0, o[2], o[3], -1 if o[4] is None else o[4])
                assert l['cout'] % 64 == 0 and (l['cin'] == 3 or l['cin'] % 32 == 0)       # what the kernel's tile and its 16-byte gather rest on
            else:
                assert (l['kind'], l['k'], l['stride'], l['pad'], l['tap']) == (1, o[1], o[2], 0, -1) and l['cin'] == l['cout'] and l['cin'] % 4 == 0


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_every_layer_shape_against_torch(hl, net):
    """Torch itself runs the layers (one channel per layer is enough for a shape) on every odd/even combination around the pools."""
    m = HL.MIN_SIZE[net]
    sizes = sorted(set([m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 7, m + 8, m + 16, m + 17, 64, 67, 93, 100, 127]))
    layers = _layers(hl, net)
    for h in sizes:
        for w in (sizes if h in (m, 67) else (m, h, 93)):
            ok, hs, ws, slots, sizes_ = _plan(hl, net, h, w)
            assert ok, (h, w)
            x = torch.zeros((1, 1, h, w))
            want = []
            for l in layers:
                x = F_conv(x, l) if l['kind'] == 0 else torch.nn.functional.max_pool2d(x, l['k'], l['stride'])
                want.append(tuple(x.shape[2:]))
            assert [(int(a), int(b)) for a, b in zip(hs, ws)] == want, (h, w)
            assert [(c, a, b) for (c, a, b) in LO.layer_shapes(net, h, w)] == [(l['cout'], *s) for l, s in zip(layers, want)]
            # the workspace: two buffers of the largest layer (both images), rounded up to 64 floats, and one double per 32 pixels of a tap
            largest = max(2 * a * b * l['cout'] for l, (a, b) in zip(layers, want))
            tap_pixels = [a * b for l, (a, b) in zip(layers, want) if l['tap'] >= 0]
            assert min(tap_pixels) >= 1
            assert list(slots[:5]) == [-(-p // 32) for p in tap_pixels] and list(slots[5:]) == list(np.cumsum([0] + list(slots[:4])))
            assert sizes_[0] == -(-largest // 64) * 64 and sizes_[1] == sum(slots[:5]) and sizes_[2] == 8 * sizes_[0] + 8 * sizes_[1]


def F_conv(x, l):
    return torch.nn.functional.conv2d(x, torch.zeros((1, 1, l['k'], l['k'])), stride=l['stride'], padding=l['pad'])


def test_minimum_sizes(hl):
    assert hl.hlp_min_size(0) == 31 == HL.MIN_SIZE['alex'] and hl.hlp_min_size(1) == 16 == HL.MIN_SIZE['vgg']
    for net, m in (('alex', 31), ('vgg', 16)):
        ok, hs, ws, _, _ = _plan(hl, net, m, m)
        assert ok and hs[-1] == 1 and ws[-1] == 1
        assert not _plan(hl, net, m - 1, m)[0] and not _plan(hl, net, m, m - 1)[0] and not _plan(hl, net, m - 1, m - 1)[0]
        # torch agrees that one pixel less leaves nothing for the last pool
        assert LO.layer_shapes(net, m - 1, m)[-1][1] == 0 and LO.layer_shapes(net, m, m)[-1][1:] == (1, 1)


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_weight_packer_index_map_round_trips(hl, net):
    for i, l in enumerate(_layers(hl, net)):
        if l['kind'] != 0:
            continue
        K = l['k'] * l['k'] * l['cin']
        Kp = -(-K // 32) * 32
        n = int(hl.hlp_packed_elems(NETS[net], i))
        assert n == l['cout'] * Kp
        src, dst = np.empty(n, np.int64), np.empty(l['cout'] * K, np.int64)
        hl.hlp_pack_src(NETS[net], i, src.ctypes.data_as(C.c_void_p))
        hl.hlp_pack_dst(NETS[net], i, dst.ctypes.data_as(C.c_void_p))
        real = src >= 0
        assert real.sum() == l['cout'] * K and (src[~real] == -1).all()
        assert np.array_equal(np.sort(src[real]), np.arange(l['cout'] * K))             # every weight exactly once
        assert np.array_equal(src[dst], np.arange(l['cout'] * K))                       # ... and where pack_dst says
        # the operand order: lane l of tile (nt, g) holds W[32 nt + (l & 31)][kk = 8 g + 4 (l >> 5) + j], kk = (ky k + kx) cin + c
        d = np.arange(n)
        j, lane, tile = d & 3, (d >> 2) & 63, d >> 8
        g, nt = tile % (Kp // 8), tile // (Kp // 8)
        kk = 8 * g + 4 * (lane >> 5) + j
        c, t = kk % l['cin'], kk // l['cin']
        want = (((32 * nt + (lane & 31)) * l['cin'] + c) * l['k'] + t // l['k']) * l['k'] + t % l['k']
        assert np.array_equal(src[real], want[real]) and (kk[~real] >= K).all()


# ---- the state dicts
def test_state_dict_keys_and_their_errors():
    assert [k[0] for k in HL.backbone_keys('alex')] == [f'features.{n}.weight' for n in (0, 3, 6, 8, 10)]
    assert [k[1] for k in HL.backbone_keys('vgg')] == [f'features.{n}.bias' for n in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)]
    assert HL.backbone_keys('alex')[0][2] == (64, 3, 11, 11) and HL.backbone_keys('vgg')[-1][2] == (512, 512, 3, 3)
    assert HL.lin_keys('alex') == [(f'lin{k}.model.1.weight', (1, c, 1, 1)) for k, c in enumerate((64, 192, 384, 256, 256))]
    assert [s[1] for _, s in HL.lin_keys('vgg')] == [64, 128, 256, 512, 512]
    for net in NETS:
        sd, lin = HL.synthetic_weights(net, 5)
        assert set(sd) == {k for wk, bk, _ in HL.backbone_keys(net) for k in (wk, bk)} and set(lin) == {k for k, _ in HL.lin_keys(net)}
        for wk, bk, shape in HL.backbone_keys(net):
            assert tuple(sd[wk].shape) == shape and tuple(sd[bk].shape) == shape[:1] and float(sd[bk].min()) >= 0.0
        assert all(float(v.min()) >= 0.0 and float(v.max()) <= 1.0 for v in lin.values())
        again = HL.synthetic_weights(net, 5)
        assert all(torch.equal(sd[k], again[0][k]) for k in sd) and not torch.equal(sd[HL.backbone_keys(net)[0][0]], HL.synthetic_weights(net, 6)[0][HL.backbone_keys(net)[0][0]])
    sd, lin = HL.synthetic_weights('alex', 5)
    # the checks run before the device is touched
    missing = {k: v for k, v in sd.items() if k != 'features.6.bias'}
    with pytest.raises(KeyError, match='features.6.bias'):
        HL.Lpips('alex', missing, lin, device='cuda:0')
    wrong = dict(sd)
    wrong['features.3.weight'] = torch.zeros((192, 64, 3, 3))
    with pytest.raises(ValueError, match=r"features.3.weight.*\(192, 64, 5, 5\)"):
        HL.Lpips('alex', wrong, lin, device='cuda:0')
    with pytest.raises(KeyError, match='lin4.model.1.weight'):
        HL.Lpips('alex', sd, {k: v for k, v in lin.items() if not k.startswith('lin4')}, device='cuda:0')
    with pytest.raises(ValueError, match='lin2.model.1.weight'):
        HL.Lpips('alex', sd, dict(lin, **{'lin2.model.1.weight': torch.zeros((1, 256, 1, 1))}), device='cuda:0')
    with pytest.raises(ValueError, match='one of'):
        HL.Lpips('squeeze', sd, lin, device='cuda:0')


def test_from_files_reads_weights_only_and_names_the_net(tmp_path, monkeypatch):
    sd, lin = HL.synthetic_weights('vgg', 2)
    torch.save(sd, tmp_path / 'backbone.pth')
    torch.save(lin, tmp_path / 'lin.pth')
    seen = {}

    def fake_init(self, net, backbone, lin_sd, device=None):
        seen.update(net=net, backbone=backbone, lin=lin_sd)

    monkeypatch.setattr(HL.Lpips, '__init__', fake_init)
    HL.Lpips.from_files(str(tmp_path / 'backbone.pth'), str(tmp_path / 'lin.pth'))
    assert seen['net'] == 'vgg' and all(torch.equal(seen['backbone'][k], sd[k]) for k in sd) and all(torch.equal(seen['lin'][k], lin[k]) for k in lin)
    HL.Lpips.from_files(str(tmp_path / 'backbone.pth'), str(tmp_path / 'lin.pth'), net='alex')
    assert seen['net'] == 'alex'
    torch.save({'lin0.model.1.weight': lin['lin0.model.1.weight']}, tmp_path / 'short.pth')
    with pytest.raises(KeyError, match='lin1.model.1.weight'):
        HL.Lpips.from_files(str(tmp_path / 'backbone.pth'), str(tmp_path / 'short.pth'))


# ---- the oracle
def test_oracle_identical_images_give_exactly_zero_and_layers_sum_to_total():
    for net, (h, w) in (('alex', (35, 47)), ('vgg', (19, 35))):
        base = LO.base_image(h, w)
        for dtype in (torch.float64, torch.float32):
            s = LO.scores(net, base, base.copy(), h, w, dtype)
            assert (s == 0.0).all()
        for label, img, s64, s32 in LO.reference(net, h, w):
            assert s64[5] == ((((s64[0] + s64[1]) + s64[2]) + s64[3]) + s64[4]) and s64[5] > 0.0, label
            assert (s64[:5] >= 0.0).all()


def test_oracle_sees_a_single_pixel_and_the_padding_rule():
    """A corner pixel changes the score, and zero padding is zero AFTER the scaling: padding with a scaled black pixel is another number."""
    h, w = 19, 35
    rows = {label: s64 for label, _, s64, _ in LO.reference('vgg', h, w)}
    assert all(rows[f'pixel {n}'][5] > 1e-7 for n in ('top-left', 'top-right', 'bottom-left', 'bottom-right', 'centre'))
    assert len({float(rows[f'pixel {n}'][0]) for n in ('top-left', 'top-right', 'bottom-left', 'bottom-right')}) == 4
    # a black 16 x 16 frame through the oracle's first convolution and the next (the first tap is after the second): were the padding a
    # scaled black pixel, the frame would be constant to the convolutions and every pixel of the tap the same; zero padding makes the border differ
    tap = LO.taps('vgg', np.zeros((16 * 16, 3), np.float32), 16, 16)[0]
    assert tap.shape == (1, 64, 16, 16)
    assert torch.allclose(tap[0, :, 5, 5], tap[0, :, 9, 7], rtol=1e-12) and not torch.allclose(tap[0, :, 0, 0], tap[0, :, 5, 5])
    assert not torch.allclose(tap[0, :, 0, 7], tap[0, :, 5, 5]) and not torch.allclose(tap[0, :, 1, 1], tap[0, :, 5, 5])


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_oracle_float32_stays_within_the_cap_on_every_pair_of_the_gpu_test(net):
    worst = (0.0, None)
    for h, w in LO.SIZES[net]:
        for label, _, s64, s32 in LO.reference(net, h, w):
            d = float(np.abs(s32 - s64).max())
            assert d <= CAP, (net, h, w, label, d)
            worst = max(worst, (d, (h, w, label)))
    print(f'{net}: the float32 oracle is at most {worst[0]:.3e} from the float64 oracle ({worst[1]})')
    assert 0.0 < worst[0] == LO.yardstick(net)
