"""Times DeviceResize (hr_image_resize) on the GPU beside PIL's Image.resize on the same machine's host, for the sizes the reference's
datasets resize at (conf/experiment/dataset/llff.yaml, technicolor.yaml, blender.yaml), the last as RGBA images (PIL resamples them
premultiplied) beside the RGB resize of the same sizes, with the ratio of the two:

    python tools/resize_ab.py [--out FILE.json] [--windows 5] [--seconds 0.4]

Per row, ms per image, each the median of `--windows` windows after a warm-up of the same shape:
  resident   the source already in device memory: device events around a window of back-to-back calls (at least `--seconds` of work)
  upload     the source a numpy array on the host, as a decoder leaves it: a host clock around DeviceResize's call, its host-to-device
             copy included, ended by a device synchronise
  pil        Image.resize on the host, one process, when PIL imports here (else the row says that it does not)
The device bytes are compared with PIL's where PIL imports: a time is reported only beside equal bytes.  A measurement needs the GPU:
without one this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hyperreel_amd.data import DeviceResize  # noqa: E402

ROWS = [((4032, 3024), (504, 378), 'lanczos', 'LLFF, Shiny', 'RGB'), ((2048, 1088), (1024, 544), 'lanczos', 'Technicolor', 'RGB'),
        ((2048, 1088), (1024, 544), 'box', 'Technicolor', 'RGB'),
        ((800, 800), (400, 400), 'lanczos', 'Blender sizes as RGB', 'RGB'), ((800, 800), (400, 400), 'lanczos', 'Blender, DoNeRF', 'RGBA')]


def host_cpu():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def time_resident(r, src, seconds, windows):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = r(src)
    torch.cuda.synchronize()
    start.record()
    for _ in range(10):
        r(src, out=out)
    stop.record()
    torch.cuda.synchronize()
    calls = max(10, int(seconds * 1e3 / max(start.elapsed_time(stop) / 10, 1e-3)))
    ms = []
    for _ in range(windows):
        start.record()
        for _ in range(calls):
            r(src, out=out)
        stop.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(stop) / calls)
    return ms, calls, out


def time_upload(r, image, windows):
    r(image)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            r(image)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return ms


def time_pil(image, dst_wh, filt, windows, mode='RGB'):
    from PIL import Image
    number = {'lanczos': Image.LANCZOS, 'box': Image.BOX}[filt]
    img = Image.fromarray(image, mode)
    ref = np.asarray(img.resize(dst_wh, number))
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        img.resize(dst_wh, number)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=0.4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resize_ab: no GPU: nothing is measured without one')
    try:
        import PIL
        pil_version = PIL.__version__
    except ImportError:
        pil_version = None
        print('PIL does not import here: no host column, and the bytes are not compared', flush=True)
    result = dict(gpu=torch.cuda.get_device_name(0), host_cpu=host_cpu(), pil=pil_version, rows=[])
    rng = np.random.default_rng(17)
    for src_wh, dst_wh, filt, what, mode in ROWS:
        image = rng.integers(0, 256, (src_wh[1], src_wh[0], len(mode)), dtype=np.uint8)
        r = DeviceResize(src_wh, dst_wh, filt, mode=mode)
        resident, calls, out = time_resident(r, torch.from_numpy(image).cuda(), a.seconds, a.windows)
        upload = time_upload(r, image, a.windows)
        row = dict(src_wh=src_wh, dst_wh=dst_wh, filter=filt, dataset=what, mode=mode, calls_per_window=calls,
                   resident_ms=statistics.median(resident), resident_ms_min_max=[min(resident), max(resident)],
                   upload_ms=statistics.median(upload), upload_ms_min_max=[min(upload), max(upload)], pil_ms=None, equal_bytes=None)
        if pil_version:
            pil, ref = time_pil(image, dst_wh, filt, a.windows, mode)
            row.update(pil_ms=statistics.median(pil), pil_ms_min_max=[min(pil), max(pil)], equal_bytes=bool(np.array_equal(out[0].cpu().numpy(), ref)))
            if not row['equal_bytes']:
                raise SystemExit(f'resize_ab: {src_wh} -> {dst_wh} {filt}: the device bytes differ from PIL\'s')
        r.close()
        result['rows'].append(row)
        pil_text = f"PIL {row['pil_ms']:.1f} ms, equal bytes" if pil_version else 'PIL does not import here'
        same = [o for o in result['rows'] if (o['src_wh'], o['dst_wh'], o['filter'], o['mode']) == (src_wh, dst_wh, filt, 'RGB')]
        if mode == 'RGBA' and same:                  # four channels move 4 / 3 of the bytes and add two conversions
            row.update(resident_over_rgb=row['resident_ms'] / same[0]['resident_ms'], upload_over_rgb=row['upload_ms'] / same[0]['upload_ms'])
            pil_text += f"  ({row['resident_over_rgb']:.2f}x the RGB row resident, {row['upload_over_rgb']:.2f}x with upload)"
        print(f"{src_wh[0]}x{src_wh[1]} -> {dst_wh[0]}x{dst_wh[1]} {filt:8s} {mode:4s} ({what}): resident {row['resident_ms']:.4f} ms  with upload "
              f"{row['upload_ms']:.3f} ms  {pil_text}", flush=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
