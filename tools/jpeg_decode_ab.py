"""Cost of getting JPEG training images into device memory, for batches of 1, 8 and 32 files at 4032 x 3024 (LLFF's and Shiny's camera
files) and 1008 x 756, 4:2:0 at quality 90 as PIL writes them, without restart markers and with one a row of MCUs.  The content is
synthetic -- a smooth textured scene with mild noise, not a photograph -- so the files' sizes, not their statistics, are a camera's.
ms per batch of
  device         the upload of the files' bytes plus hr_jpeg_decode (JpegDecoder.upload + decode_device, one synchronise)
  host_1 / _16   the path it replaces: PIL's Image.open(...).convert('RGB') of the same files in 1 process and in a pool of 16, plus the
                 upload of the decoded bytes.  The pool is a DataLoader's shape: every file's bytes go to a worker and every decoded
                 array comes back through a pipe, then np.stack -- host_16 holds that traffic, not PIL's decode alone
  device_serial  (one 4032 x 3024 file only) the same decode with one subsequence over the whole scan: the serial walk of one lane, which
                 shows what the self-synchronising subsequences buy
and, with --trace, the decoder's per-kernel times from a rocprofv3 --kernel-trace run of its own (a child process).

    python tools/jpeg_decode_ab.py [--rounds R] [--batches 1,8,32] [--out F] [--trace DIR]

The variants alternate inside a round and the best of the rounds is quoted; a window is one warmed call repeated until --seconds have
passed (at least once).  The batch is made of `--distinct` different files repeated.  Nothing is asserted about time: the numbers are
printed.  The decoded pixels are compared with PIL's once per case.  Measurement aid (GPU box)."""
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

CASES = [(4032, 3024), (1008, 756)]
RESTARTS = {'none': {}, 'rows': dict(restart_marker_rows=1)}


def make_file(w, h, restart, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    scale = 4032.0 / w
    im = np.stack([128 + 70 * np.sin(xx * (0.011 * scale) + k + seed) * np.cos(yy * (0.007 * scale) - k) + 40 * np.sin((xx + yy) * (0.09 * scale) + 2 * k)
                   for k in range(3)], -1)
    im = (im + rng.normal(0, 6, im.shape)).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(im).save(b, 'JPEG', quality=90, subsampling=2, **RESTARTS[restart])
    return b.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


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
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--distinct', type=int, default=2)
    ap.add_argument('--processes', type=int, default=16)
    ap.add_argument('--host1-max', type=int, default=8, help='largest batch the single-process host path is timed at (it is linear in the batch)')
    ap.add_argument('--width', type=int, default=0, help='only the case of this width (4032 or 1008); default both')
    ap.add_argument('--out', default='')
    ap.add_argument('--trace', default='', help='directory for a rocprofv3 --kernel-trace --stats run of one 8-file decode per case')
    ap.add_argument('--trace-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import multiprocessing as mp
    pool = None if args.trace_child else mp.get_context('spawn').Pool(args.processes)    # fresh children, started before this process opens the device
    import torch
    from hyperreel_amd import jpeg
    assert torch.cuda.is_available(), 'tools/jpeg_decode_ab.py measures on the HIP device'
    batches = [int(b) for b in args.batches.split(',')]

    if args.trace_child:                                       # under the profiler: decodes only
        for w, h in CASES:
            for restart in RESTARTS:
                files = [make_file(w, h, restart, 0)] * 8
                dec = jpeg.JpegDecoder(w, h, max_images=len(files), max_file_bytes=sum(len(f) for f in files))
                for _ in range(2):
                    dec.decode(files, 'RGB')
                torch.cuda.synchronize()
                dec.close()
        return

    results = []
    for w, h in [c for c in CASES if args.width in (0, c[0])]:
        for restart in RESTARTS:
            distinct = [make_file(w, h, restart, s) for s in range(args.distinct)]
            for n in batches:
                files = [distinct[i % len(distinct)] for i in range(n)]
                total = sum(len(f) for f in files)
                dec = jpeg.JpegDecoder(w, h, max_images=n, max_file_bytes=total)
                files_dev, offsets_dev = dec.upload(files[:min(n, len(distinct))])
                rounds = torch.zeros(min(n, len(distinct)), dtype=torch.int32, device='cuda')
                check, status = dec.decode_device(files_dev, offsets_dev, len(rounds), 'RGB', rounds=rounds)
                check = check.cpu().numpy()
                exact = not status.cpu().numpy().any() and all(np.array_equal(check[i], pil_decode(files[i])) for i in range(len(check)))

                def device(d=dec):
                    files_dev, offsets_dev = d.upload(files)
                    d.decode_device(files_dev, offsets_dev, n, 'RGB')
                    torch.cuda.synchronize()

                def host(p):
                    arrays = pool.map(pil_decode, files, chunksize=1) if p > 1 else [pil_decode(f) for f in files]
                    torch.from_numpy(np.stack(arrays)).cuda()
                    torch.cuda.synchronize()

                variants = {'device': device, f'host_{args.processes}': lambda: host(args.processes)}
                if n <= args.host1_max:
                    variants['host_1'] = lambda: host(1)
                serial = None
                if n == 1 and w == 4032:
                    serial = jpeg.JpegDecoder(w, h, max_images=1, max_file_bytes=total, subseq_bits=(8 * total + 31) // 32 * 32)
                    variants['device_serial'] = lambda: device(serial)
                best = {k: float('inf') for k in variants}
                for _ in range(args.rounds):
                    for k, step in variants.items():
                        best[k] = min(best[k], window(step, args.seconds))
                        print(json.dumps({'progress': f'{w} x {h} {restart} x {n}', k: round(best[k], 3)}), file=sys.stderr, flush=True)
                r = {'width': w, 'height': h, 'restart': restart, 'files': n, 'file_bytes': len(files[0]), 'huffman_rounds': int(rounds.max().item()),
                     'ms_per_batch': {'host_1': 'not measured', **{k: round(v, 3) for k, v in best.items()}}, 'pixels_equal_pil': bool(exact),
                     'device_below_host_pool': bool(best['device'] < best[f'host_{args.processes}'])}
                results.append(r)
                print(json.dumps(r), flush=True)
                dec.close()
                if serial is not None:
                    serial.close()
    pool.close()
    pool.join()
    if args.trace:
        os.makedirs(args.trace, exist_ok=True)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', args.trace, '-o', 'jpeg_decode', '--output-format', 'csv', '--', sys.executable,
               os.path.abspath(__file__), '--trace-child']
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(json.dumps({'trace': args.trace, 'returncode': r.returncode, 'tail': (r.stdout + r.stderr)[-400:]}), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
