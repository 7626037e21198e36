"""The bits of hyperreel_amd/csrc/hr_camera.h's camera pipeline, pinned without a GPU: SHA-256 digests of the float32 rays that the
host builds of the header (tests/host_math/hr_camera_host.cpp, hr_fisheye_host.cpp; -O1 -ffp-contract=off, IEEE operations only) give
for fixed inputs, against tests/golden/camera/pixel_ray_digests.json.

How the digests were produced: `digests()` below, run once at the commit BEFORE hr_pixel_ray and hr_pixel_ray_lens were rewritten
as one pipeline of stages (plane -> [undistort, normalise] -> world -> [NDC]), i.e. on the two separate functions that each carried
their own rotation and NDC statements.  They are this project's own recorded results and never come from the header under test: a
change of the header that moves one bit of one ray fails here, and the file is regenerated only by a change that means to move bits.

Inputs:
  hr_pixel_ray          every image of every fixture of camera_common.CASES, whole frames, with the fixture's NDC (NULL where it has
                        none), plus image 0 of the NDC fixture video_ndc with ndc == NULL
  hr_pixel_ray_fisheye  every fisheye_common.CASES entry x (a NULL hr_fisheye, every PAIRS entry -- (0, 0) among them) x ndc in (NULL, NDC)"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import camera_common as CC
import fisheye_common as FC

GOLDEN = os.path.join(CC.GOLDEN, 'pixel_ray_digests.json')


def _sha(a):
    assert a.dtype == np.float32 and a.flags['C_CONTIGUOUS']
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests():
    """{input name: SHA-256 of the (pixels, 6) float32 rays' bytes} from the current header's host builds."""
    out = {}
    hc = CC.host_lib()
    for name in CC.CASES:
        f = CC.load(name)
        nd = CC.ndc_struct(f)
        W, H = int(f['img_wh'][0]), int(f['img_wh'][1])
        cases = [(i, nd, '') for i in range(len(f['poses']))]
        if name == 'video_ndc':
            assert nd is not None
            cases.append((0, None, '/ndc_null'))
        for i, n, tag in cases:
            cam = CC.camera_of(f, i)
            rays = np.full((W * H, 6), np.nan, np.float32)
            hc.hc_pixel_rays(C.byref(cam), C.byref(n) if n is not None else None, 0, W * H, rays.ctypes.data_as(C.c_void_p))
            out[f'hr_pixel_ray/{name}/image{i}{tag}'] = _sha(rays)
    hf = FC.host_lib()
    for name in FC.CASES:
        for pair in [None] + FC.PAIRS:
            for ndc in (None, FC.NDC):
                out[f'hr_pixel_ray_fisheye/{name}/{pair}/{"ndc" if ndc else "world"}'] = _sha(FC.host_rays(hf, name, pair, ndc))
    return out


def test_the_header_gives_the_recorded_bits():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = digests()
    assert sorted(got) == sorted(want)
    assert len(got) == sum(len(CC.load(n)['poses']) for n in CC.CASES) + 1 + len(FC.CASES) * (len(FC.PAIRS) + 1) * 2
    differ = [k for k in want if got[k] != want[k]]
    print(f'{len(want)} digests, {len(differ)} differ', flush=True)
    assert not differ, differ
    # the recorded inputs tell the stages apart: NDC and the lens each move the bits, NULL and (0, 0) do not (a video fixture's frames
    # of one camera share a pose, hence a digest: the 6 columns hold no time)
    assert want['hr_pixel_ray/video_ndc/image0'] != want['hr_pixel_ray/video_ndc/image0/ndc_null']
    assert want['hr_pixel_ray_fisheye/centred/None/world'] == want['hr_pixel_ray_fisheye/centred/(0.0, 0.0)/world']
    assert want['hr_pixel_ray_fisheye/centred/None/ndc'] != want[f'hr_pixel_ray_fisheye/centred/{FC.PAIRS[1]}/ndc']
