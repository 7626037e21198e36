"""Cost of getting PNG training images into device memory, for batches of 1, 16 and 256 files at 800 x 800 RGBA and 2048 x 1088 RGB,
content a rendered synthetic frame (a textured disc on white) and a noisy one, files written by PIL at compress_level 6: ms per batch of
  device         the upload of the files' bytes plus hr_png_decode (PngDecoder.upload + decode_device, one synchronise)
  host_1 / _16   the path it replaces: PIL's Image.open(...).convert(mode) of the same files in 1 process and in a pool of 16, plus the
                 upload of the decoded bytes.  The pool is a DataLoader's shape: every file's bytes go to a worker and every decoded
                 array comes back through a pipe, then np.stack -- host_16 holds that traffic, not PIL's decode alone (16 x host_1's
                 rate is the floor a shared-memory pool could approach)
and, with --trace, the decoder's per-kernel times from a rocprofv3 --kernel-trace run of its own (a child process).

    python tools/png_decode_ab.py [--rounds R] [--batches 1,16,256] [--out F] [--trace DIR]

The variants alternate inside a round and the best of the rounds is quoted; a window is one warmed call repeated until --seconds have
passed (at least once).  The batch is made of `--distinct` different files repeated, so that building it stays cheap.  Nothing is
asserted about time: the numbers are printed.  The decoded pixels are compared with PIL's once per case.  Measurement aid (GPU box)."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(800, 800, 'RGBA'), (2048, 1088, 'RGB')]


def make_file(w, h, mode, content, seed):
    from PIL import Image
    c = len(mode)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == 'noise':
        im = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    else:
        inside = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2) < (min(w, h) * 0.35) ** 2
        tex = (128 + 60 * np.sin(xx[..., None] * 0.031 + np.arange(c) + seed) + 50 * np.cos(yy[..., None] * 0.017)
               + rng.integers(-3, 4, (h, w, c))).clip(0, 255).astype(np.uint8)
        im = np.where(inside[..., None], tex, np.uint8(255)).astype(np.uint8)
        if c == 4:
            im[..., 3] = np.where(inside, 255, 0)
    b = io.BytesIO()
    Image.fromarray(im, mode).save(b, 'PNG', compress_level=6)
    return b.getvalue()


def pil_decode(args):
    from PIL import Image
    data, mode = args
    return np.asarray(Image.open(io.BytesIO(data)).convert(mode))


def window(step, seconds):
    step()
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='1,16,256')
    ap.add_argument('--distinct', type=int, default=4)
    ap.add_argument('--processes', type=int, default=16)
    ap.add_argument('--host1-max', type=int, default=16, help='largest batch the single-process host path is timed at (it is linear in the batch)')
    ap.add_argument('--width', type=int, default=0, help='only the case of this width (800 or 2048); default both')
    ap.add_argument('--out', default='')
    ap.add_argument('--trace', default='', help='directory for a rocprofv3 --kernel-trace --stats run of one 16-file decode per case')
    ap.add_argument('--trace-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import multiprocessing as mp
    pool = None if args.trace_child else mp.get_context('spawn').Pool(args.processes)    # fresh children, started before this process opens the device
    import torch
    from hyperreel_amd import png
    assert torch.cuda.is_available(), 'tools/png_decode_ab.py measures on the HIP device'
    batches = [int(b) for b in args.batches.split(',')]

    if args.trace_child:                                       # under the profiler: decodes only
        for w, h, mode in CASES:
            for content in ('render', 'noise'):
                files = [make_file(w, h, mode, content, s) for s in range(2)] * 8
                dec = png.PngDecoder(w, h, max_images=len(files))
                for _ in range(2):
                    dec.decode(files, mode)
                torch.cuda.synchronize()
                dec.close()
        return

    results = []
    for w, h, mode in [c for c in CASES if args.width in (0, c[0])]:
        for content in ('render', 'noise'):
            distinct = [make_file(w, h, mode, content, s) for s in range(args.distinct)]
            for n in batches:
                files = [distinct[i % len(distinct)] for i in range(n)]
                dec = png.PngDecoder(w, h, max_images=n, max_file_bytes=sum(len(f) for f in files))
                check = dec.decode(files[:min(n, len(distinct))], mode).cpu().numpy()
                exact = all(np.array_equal(check[i], pil_decode((files[i], mode))) for i in range(len(check)))

                def device():
                    files_dev, offsets_dev = dec.upload(files)
                    dec.decode_device(files_dev, offsets_dev, n, mode)
                    torch.cuda.synchronize()

                def host(p):
                    jobs = [(f, mode) for f in files]
                    arrays = pool.map(pil_decode, jobs, chunksize=max(1, n // (4 * args.processes))) if p > 1 else [pil_decode(j) for j in jobs]
                    torch.from_numpy(np.stack(arrays)).cuda()
                    torch.cuda.synchronize()

                variants = {'device': device, f'host_{args.processes}': lambda: host(args.processes)}
                if n <= args.host1_max:
                    variants['host_1'] = lambda: host(1)
                best = {k: float('inf') for k in variants}
                for _ in range(args.rounds):
                    for k, step in variants.items():
                        best[k] = min(best[k], window(step, args.seconds))
                r = {'width': w, 'height': h, 'mode': mode, 'content': content, 'files': n, 'file_bytes': len(files[0]),
                     'ms_per_batch': {'host_1': 'not measured', **{k: round(v, 3) for k, v in best.items()}}, 'pixels_equal_pil': bool(exact),
                     'device_below_host_pool': bool(best['device'] < best[f'host_{args.processes}'])}
                results.append(r)
                print(json.dumps(r), flush=True)
                dec.close()
    pool.close()
    pool.join()
    if args.trace:
        os.makedirs(args.trace, exist_ok=True)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', args.trace, '-o', 'png_decode', '--output-format', 'csv', '--', sys.executable,
               os.path.abspath(__file__), '--trace-child']
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(json.dumps({'trace': args.trace, 'returncode': r.returncode, 'tail': (r.stdout + r.stderr)[-400:]}), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
