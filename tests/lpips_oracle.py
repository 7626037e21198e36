"""LPIPS v0.1 (eval mode) in torch on the CPU, written from the definition in hyperreel_amd/csrc/hr_lpips.h, in float64 (the oracle) and
float32 (the yardstick: what a float32 evaluation of the same formula loses), with the synthetic weights and the image pairs that
tests/test_lpips_host.py and tests/test_gpu_lpips.py share.

    x = 2 v - 1;  x = (x - shift[c]) / scale[c];  backbone with five taps after ReLUs;
    per tap: n = f / (sqrt(sum_c f^2) + 1e-10),  layer = mean_{H, W} sum_c lin[c] (n_pred - n_gt)^2;  total = sum of the layers
"""
import numpy as np
import torch
import torch.nn.functional as F

from hyperreel_amd import lpips as HL

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
SEED = 11

# ('conv', index into the net's convolutions, stride, padding, tap or None) / ('pool', kernel, stride)
LAYERS = {
    'alex': [('conv', 0, 4, 2, 0), ('pool', 3, 2), ('conv', 1, 1, 2, 1), ('pool', 3, 2), ('conv', 2, 1, 1, 2), ('conv', 3, 1, 1, 3), ('conv', 4, 1, 1, 4)],
    'vgg': [('conv', 0, 1, 1, None), ('conv', 1, 1, 1, 0), ('pool', 2, 2),
            ('conv', 2, 1, 1, None), ('conv', 3, 1, 1, 1), ('pool', 2, 2),
            ('conv', 4, 1, 1, None), ('conv', 5, 1, 1, None), ('conv', 6, 1, 1, 2), ('pool', 2, 2),
            ('conv', 7, 1, 1, None), ('conv', 8, 1, 1, None), ('conv', 9, 1, 1, 3), ('pool', 2, 2),
            ('conv', 10, 1, 1, None), ('conv', 11, 1, 1, None), ('conv', 12, 1, 1, 4)],
}
# the GPU test's frames, (h, w)
SIZES = {'alex': [(31, 31), (35, 47), (64, 64), (67, 93), (200, 176)], 'vgg': [(16, 16), (19, 35), (32, 32), (48, 40), (96, 112)]}
NOISES = (0.002, 0.05, 0.3)

_cache = {}


def weights(net):
    """(backbone state dict, lin state dict): lpips.synthetic_weights(net, SEED), made once"""
    if ('weights', net) not in _cache:
        _cache[('weights', net)] = HL.synthetic_weights(net, SEED)
    return _cache[('weights', net)]


def layer_shapes(net, h, w):
    """[(channels, height, width)] after every layer, by the floor rule"""
    out = []
    for l in LAYERS[net]:
        if l[0] == 'conv':
            cin, c, k = HL.CONVS[net][l[1]]
            stride, pad = l[2], l[3]
        else:
            k, stride, pad = l[1], l[2], 0
            c = out[-1][0]
        h, w = (h + 2 * pad - k) // stride + 1 if h + 2 * pad >= k else 0, (w + 2 * pad - k) // stride + 1 if w + 2 * pad >= k else 0
        out.append((c, h, w))
    return out


def taps(net, image, h, w, dtype=torch.float64, wts=None):
    """image: (h*w, 3) float32 numpy in [0, 1] -> the five taps (1, C_k, H_k, W_k) in `dtype`"""
    backbone, _ = wts or weights(net)
    keys = HL.backbone_keys(net)
    x = torch.from_numpy(np.array(image, np.float32)).reshape(h, w, 3).permute(2, 0, 1)[None].to(dtype)
    x = x * 2 - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    out = [None] * 5
    for l in LAYERS[net]:
        if l[0] == 'conv':
            wk, bk, _ = keys[l[1]]
            x = F.relu(F.conv2d(x, backbone[wk].to(dtype), backbone[bk].to(dtype), stride=l[2], padding=l[3]))
            if l[4] is not None:
                out[l[4]] = x
        else:
            x = F.max_pool2d(x, l[1], l[2])                      # ceil_mode=False: floor
    return out


def distance(net, taps_a, taps_b, wts=None):
    """six float64: layer[0..4], total.  The arithmetic stays in the taps' dtype until each layer's mean."""
    _, lin = wts or weights(net)
    layers = []
    for k, (fa, fb) in enumerate(zip(taps_a, taps_b)):
        na = fa / (torch.sqrt(torch.sum(fa * fa, dim=1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt(torch.sum(fb * fb, dim=1, keepdim=True)) + 1e-10)
        d = (na - nb) ** 2
        lw = lin[HL.lin_keys(net)[k][0]].to(fa.dtype)
        layers.append(float(torch.mean(torch.sum(lw * d, dim=1, keepdim=True), dim=(2, 3)).item()))
    total = 0.0
    for v in layers:
        total += v
    return np.array(layers + [total], np.float64)


def scores(net, pred, gt, h, w, dtype=torch.float64, wts=None):
    return distance(net, taps(net, pred, h, w, dtype, wts), taps(net, gt, h, w, dtype, wts), wts)


# ---- the image pairs
def base_image(h, w):
    """smooth plus noise, (h*w, 3) float32 in [0, 1]"""
    key = ('base', h, w)
    if key not in _cache:
        rng = np.random.default_rng(h * 10007 + w)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([0.5 + 0.35 * np.sin(xx / 7.0 + 0.3 * c) * np.cos(yy / 5.0 - 0.2 * c) for c in range(3)], -1)
        img = np.clip(img + rng.normal(0, 0.1, img.shape), 0, 1).astype(np.float32).reshape(-1, 3)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def pairs(h, w):
    """[(label, second image)]: the base image perturbed at NOISES, and differing from it in one pixel at the corners and the centre"""
    key = ('pairs', h, w)
    if key not in _cache:
        base = base_image(h, w)
        rng = np.random.default_rng(h * 7919 + w + 1)
        out = []
        for sigma in NOISES:
            out.append((f'noise {sigma}', np.clip(base + rng.normal(0, sigma, base.shape), 0, 1).astype(np.float32)))
        for name, (y, x) in (('top-left', (0, 0)), ('top-right', (0, w - 1)), ('bottom-left', (h - 1, 0)), ('bottom-right', (h - 1, w - 1)),
                             ('centre', (h // 2, w // 2))):
            img = base.copy()
            img[y * w + x] = 1.0 - img[y * w + x]
            out.append((f'pixel {name}', img))
        for _, img in out:
            img.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def reference(net, h, w):
    """[(label, second image, float64 scores, float32 scores)] of pairs(h, w) against base_image(h, w): computed once, the base image's
    taps shared by the pairs"""
    key = ('reference', net, h, w)
    if key not in _cache:
        base = base_image(h, w)
        t64, t32 = taps(net, base, h, w, torch.float64), taps(net, base, h, w, torch.float32)
        rows = []
        for label, img in pairs(h, w):
            s64 = distance(net, t64, taps(net, img, h, w, torch.float64))
            s32 = distance(net, t32, taps(net, img, h, w, torch.float32))
            rows.append((label, img, s64, s32))
        _cache[key] = rows
    return _cache[key]


def yardstick(net):
    """the float32 oracle's largest distance from the float64 oracle, over `total` and every layer of every pair of every size"""
    return max(float(np.abs(s32 - s64).max()) for h, w in SIZES[net] for _, _, s64, s32 in reference(net, h, w))
