"""`-m gpu`: LPIPS on the device (hr_lpips, hyperreel_amd.lpips, HipLightfieldModel.evaluate(lpips=...)) against the float64 torch oracle of
tests/lpips_oracle.py, on seeded synthetic weights of the real shapes (no pretrained file is on hand: agreement with the lpips package's
published numbers is unverified).

The bar is not a constant of this file: per net, the float32 oracle's largest distance from the float64 oracle over the pairs of the test
is the yardstick, computed on the CPU here; the device's `total` and every `layer[k]` may be at most 10x that from the float64 oracle (a
different summation order, tile-local K order -- the margin test_gpu_metrics.py gives SSIM), and never more than 1e-5 (published LPIPS is
read to three decimals).

Measured (MI355X): yardstick 7.0e-8 (alex, 200x176 noise 0.3) and 3.5e-8 (vgg, 19x35 noise 0.3), so the bars are 7.0e-7 and 3.5e-7; the
device's largest distance is 7.8e-8 (alex, 31x31 noise 0.3) and 2.9e-8 (vgg, 48x40 noise 0.3).  DESIGN.md 3j keeps the figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import lpips_oracle as LO
from hyperreel_amd import config as HC
from hyperreel_amd import lib as _lib
from hyperreel_amd import lpips as HL
from hyperreel_amd import metrics, scenes

pytestmark = pytest.mark.gpu

CAP = 1e-5
NETS = {'alex': 0, 'vgg': 1}
_scorers = {}


def _scorer(net):
    if net not in _scorers:
        _scorers[net] = HL.Lpips(net, *LO.weights(net))
    return _scorers[net]


def _dev(img):
    return torch.from_numpy(np.array(img)).cuda()


def _bits(t):
    return t.view(torch.int64)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _abi_scores(net, pred, gt, h, w, fill=None):
    """Through ctypes into the C ABI: the six doubles.  fill: byte the workspace and the result are set to before the call."""
    L = _lib.load()
    nbytes = int(L.hr_lpips_workspace(NETS[net], h, w))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
    out = torch.empty((48,), dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill)
        out.fill_(fill)
    rc = L.hr_lpips(_scorer(net)._h, C.c_void_p(pred.data_ptr()), C.c_void_p(gt.data_ptr()), h, w, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                    _stream())
    assert rc == 0, L.hr_last_error()
    torch.cuda.synchronize()
    return out.view(torch.float64).clone()


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_accuracy_against_the_float64_oracle(net):
    rows = []
    for h, w in LO.SIZES[net]:
        base = _dev(LO.base_image(h, w))
        for label, img, s64, s32 in LO.reference(net, h, w):
            got = _scorer(net).lpips_scores(base, _dev(img), h, w).cpu().numpy()
            rows.append(dict(size=(h, w), pair=label, total64=float(s64[5]), d32=float(np.abs(s32 - s64).max()), ddev=float(np.abs(got - s64).max()),
                             sums=got[5] == ((((got[0] + got[1]) + got[2]) + got[3]) + got[4])))
            r = rows[-1]
            print(f"{net} {h:>4}x{w:<4} {label:<20} total64 {r['total64']:.10f}  |f32-f64| {r['d32']:.2e}  |dev-f64| {r['ddev']:.2e}", flush=True)
    yard = max(r['d32'] for r in rows)
    bar = min(10.0 * yard, CAP)
    print(f'{net}: LPIPS bar min(10 x {yard:.3e}, {CAP}) = {bar:.3e}; worst device distance {max(r["ddev"] for r in rows):.3e}', flush=True)
    assert yard == LO.yardstick(net) and len(rows) == len(LO.SIZES[net]) * 8                 # no pair is left out of the comparison
    for r in rows:
        assert r['ddev'] <= bar, (r, bar)
        assert r['sums'], r


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_exactness(net):
    """identical pair, swapped pair, repeated call, poisoned buffers, another stream, a replayed graph: the same bits"""
    h, w = LO.SIZES[net][3]                                                                  # odd sizes through every pool, several workgroups
    s = _scorer(net)
    a, b = _dev(LO.base_image(h, w)), _dev(LO.pairs(h, w)[1][1])
    a0, b0 = a.clone(), b.clone()
    same = s.lpips_scores(a, a.clone(), h, w)
    assert float(same[5]) == 0.0 and (same == 0.0).all()
    ref = _abi_scores(net, a, b, h, w, fill=0x00)
    assert float(ref[5]) > 0.0
    assert torch.equal(_bits(_abi_scores(net, b, a, h, w)), _bits(ref))                      # (a, b) and (b, a)
    assert torch.equal(_bits(_abi_scores(net, a, b, h, w)), _bits(ref))                      # two calls
    assert torch.equal(_bits(_abi_scores(net, a, b, h, w, fill=0xff)), _bits(ref))           # poisoned workspace and result
    assert torch.equal(_bits(s.lpips_scores(a, b, h, w)), _bits(ref))                        # the Python surface: the same call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = s.lpips_scores(a, b, h, w)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(_bits(other), _bits(ref))
    # a captured graph over fixed buffers, result and workspace poisoned before every replay
    out = torch.empty((6,), dtype=torch.float64, device='cuda')
    ws = torch.empty((HL.workspace_doubles(net, h, w),), dtype=torch.float64, device='cuda')
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.lpips_scores(a, b, h, w, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.lpips_scores(a, b, h, w, out=out, workspace=ws)
    for _ in range(3):
        out.view(torch.uint8).fill_(0xff)
        ws.view(torch.uint8).fill_(0xff)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(b.view(torch.int32), b0.view(torch.int32))


def test_weights_from_host_pointers_give_the_same_object():
    """hr_lpips_create takes host memory too: the same bits as the device tensors the Python surface hands over."""
    net, (h, w) = 'alex', LO.SIZES['alex'][1]
    sd, lin = LO.weights(net)
    groups = [[sd[wk].contiguous() for wk, _, _ in HL.backbone_keys(net)], [sd[bk].contiguous() for _, bk, _ in HL.backbone_keys(net)],
              [lin[k].contiguous() for k, _ in HL.lin_keys(net)]]
    arrays = [(C.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in groups]
    L = _lib.load()
    handle = C.c_void_p()
    assert L.hr_lpips_create(0, *arrays, C.byref(handle)) == 0, L.hr_last_error()
    try:
        a, b = _dev(LO.base_image(h, w)), _dev(LO.pairs(h, w)[2][1])
        out = torch.zeros((6,), dtype=torch.float64, device='cuda')
        ws = torch.empty((HL.workspace_doubles(net, h, w),), dtype=torch.float64, device='cuda')
        assert L.hr_lpips(handle, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), h, w, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                          _stream()) == 0, L.hr_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(_scorer(net).lpips_scores(a, b, h, w)))
    finally:
        L.hr_lpips_destroy(handle)


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_refusals_write_nothing(net):
    L = _lib.load()
    m = HL.MIN_SIZE[net]
    img = torch.rand((64 * 64, 3), device='cuda')
    out = torch.empty((48,), dtype=torch.uint8, device='cuda').fill_(0xa5)
    ws = torch.empty((int(L.hr_lpips_workspace(NETS[net], 64, 64)),), dtype=torch.uint8, device='cuda').fill_(0xa5)
    h = _scorer(net)._h
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.hr_lpips_workspace(NETS[net], m - 1, 64) == 0 and L.hr_lpips_workspace(NETS[net], 64, m - 1) == 0
    assert L.hr_lpips(h, p(img), p(img), m - 1, 64, p(out), p(ws), _stream()) == -1 and b'at least' in L.hr_last_error()
    assert L.hr_lpips(h, p(img), p(img), 64, m - 1, p(out), p(ws), _stream()) == -1
    assert L.hr_lpips(None, p(img), p(img), 64, 64, p(out), p(ws), _stream()) == -1 and b'null' in L.hr_last_error()
    assert L.hr_lpips(h, None, p(img), 64, 64, p(out), p(ws), _stream()) == -1
    assert L.hr_lpips(h, p(img), None, 64, 64, p(out), p(ws), _stream()) == -1
    assert L.hr_lpips(h, p(img), p(img), 64, 64, None, p(ws), _stream()) == -1
    assert L.hr_lpips(h, p(img), p(img), 64, 64, p(out), None, _stream()) == -1
    assert L.hr_lpips(h, p(img), p(img), 64, 64, p(out), C.c_void_p(ws.data_ptr() + 4), _stream()) == -1 and b'aligned' in L.hr_last_error()
    torch.cuda.synchronize()
    assert (out == 0xa5).all() and (ws == 0xa5).all()
    s = _scorer(net)
    with pytest.raises(ValueError, match='at least'):
        s.lpips_scores(img[:(m - 1) * 64], img[:(m - 1) * 64], m - 1, 64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        s.lpips_scores(img.cpu(), img, 64, 64)
    with pytest.raises(ValueError, match='workspace'):
        s.lpips_scores(img, img, 64, 64, workspace=torch.empty((8,), dtype=torch.float64, device='cuda'))


def test_evaluate_with_lpips_is_render_then_score():
    from gpu_common import make_render_fn
    name, h, w = 'donerf_sphere', 60, 80
    cfg, ds = HC.model_config(name), HC.dataset_scalars(name)
    sd = scenes.make_state_dict(cfg, ds, [48, 40, 36], seed=3, density='dense', app_scale=1.0)
    model = make_render_fn(cfg, ds, sd, mlp_precision='auto').model
    rays = torch.from_numpy(scenes.benchmark_rays(name, h, w, frame=7)).cuda()
    ref = model.render(rays)['rgb'].clone()
    gt = torch.from_numpy(np.clip(ref.cpu().numpy() + np.random.default_rng(4).normal(0, 0.03, (h * w, 3)), 0, 1).astype(np.float32)).cuda()
    plain = metrics.scores_to_metrics(metrics.image_scores(ref, gt, h, w), h, w)
    rgb0, m0 = model.evaluate(rays, gt, h, w)
    assert torch.equal(rgb0.view(torch.int32), ref.view(torch.int32)) and m0 == plain and set(m0) == {'mse', 'psnr', 'ssim'}
    for net in ('alex', 'vgg'):
        rgb, m = model.evaluate(rays, gt, h, w, lpips=_scorer(net))
        assert torch.equal(rgb.view(torch.int32), ref.view(torch.int32))
        assert {k: v for k, v in m.items() if k != 'lpips'} == plain
        assert m['lpips'] == float(_scorer(net).lpips_scores(ref, gt, h, w)[5]) > 0.0
        o = LO.scores(net, ref.cpu().numpy(), gt.cpu().numpy(), h, w)
        assert abs(m['lpips'] - o[5]) <= CAP
