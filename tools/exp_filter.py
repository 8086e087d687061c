#!/usr/bin/env python3
"""tools/exp_filter.py — what the tent reconstruction filter costs on the device: chess rescaled to 4096^2, k = 2 and 4,
specialised kernels, one GPU, one process.  Per k it times, alternating:
  T  the tent call into HBM (a samples = k, filter = tent context: per band a plain launch into scratch + maray_filter_tent<k>);
  X  the box call on a samples = k context (maray_jit_pixels_ss);
  B  the plain launch of the same program over the k N x k N sample grid into one buffer;
  F  the filter kernel alone on samples already in HBM (maray_hip_time_filter),
each the median of ROUNDS x REPS between events that end in a synchronise.  F's achieved bytes per second counts what the kernel
has to move: (3 k^2 + 3) bytes per output pixel; beside it the fill rate bench.py --full reports, measured here the same way
(hipMemsetAsync of the 3-byte output raster on the stream).  T's image is checked against the numpy contract applied to B's
samples.  One JSON line per k.  --rounds N (default 5), --size N (default 4096), --out FILE: the lines, appended."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
from test_filter import tent  # noqa: E402

REPS = 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
SIZE = int(sys.argv[sys.argv.index('--size') + 1]) if '--size' in sys.argv else 4096
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(REPS):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


hip = C.CDLL('libamdhip64.so')
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
stream = torch.cuda.Stream()
N = SIZE
for k in (2, 4):
    scene = M.Scene.open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'))
    if N != 1024:
        scene.rescale(N // 1024, N // 1024)
    scene.supersample(k)
    tape = scene.lower()
    tent_ctx = M.Context(tape, backend=M.BACKEND_JIT, samples=k, filter=M.FILTER_TENT)
    box_ctx = M.Context(tape, backend=M.BACKEND_JIT, samples=k)
    plain = M.Context(tape, backend=M.BACKEND_JIT)
    out8 = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
    samples8 = torch.zeros((N * k, N * k, 3), dtype=torch.uint8, device='cuda')
    nbytes = out8.numel()
    with torch.cuda.stream(stream):
        # correctness first: T = the contract applied to B's samples, on a band of rows across the board's edge
        plain.render_rows_device(N * k, N * k, 0, N * k, d_rgb8=samples8.data_ptr(), stream=stream.cuda_stream)
        tent_ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        y0, y1 = N // 2 - 64, N // 2 + 192
        band = samples8[(y0 - 1) * k:(y1 + 1) * k].cpu().numpy()        # one output row more on both sides: those two clamp to the band, not the image
        assert np.array_equal(out8[y0:y1].cpu().numpy(), tent(band, k)[1:-1]), k

        def run_t():
            tent_ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)

        def run_x():
            box_ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)

        def run_b():
            plain.render_rows_device(N * k, N * k, 0, N * k, d_rgb8=samples8.data_ptr(), stream=stream.cuda_stream)

        def run_fill():
            hip.hipMemsetAsync(out8.data_ptr(), 0, nbytes, stream.cuda_stream)

        ms = {'T': [], 'X': [], 'B': [], 'F': [], 'fill': []}
        for fn in (run_t, run_x, run_b, run_fill):
            fn(); fn()
        stream.synchronize()
        for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
            ms['T'].append(timed(run_t, stream))
            ms['X'].append(timed(run_x, stream))
            ms['B'].append(timed(run_b, stream))
            ms['F'].append(M.time_filter(N, N, k, reps=REPS))
            ms['fill'].append(timed(run_fill, stream))
        med = {n: float(np.median(v)) for n, v in ms.items()}
        moved = (3 * k * k + 3) * N * N
        emit({'scene': 'chess' + ('' if N == 1024 else ' rescaled to %d^2' % N), 'size': N, 'k': k, 'backend': 'jit', 'kernel': tent_ctx.kernel_name,
              'rounds': ROUNDS, 'reps': REPS, 'band_rows_env': os.environ.get('MARAY_FILTER_BAND_ROWS'),
              'T_tent_ms': round(med['T'], 4), 'X_box_ms': round(med['X'], 4), 'B_plain_samples_ms': round(med['B'], 4), 'F_filter_ms': round(med['F'], 4),
              'T_minus_B_ms': round(med['T'] - med['B'], 4), 'T_over_X': round(med['T'] / med['X'], 3),
              'T_all_ms': [round(v, 4) for v in ms['T']], 'X_all_ms': [round(v, 4) for v in ms['X']], 'B_all_ms': [round(v, 4) for v in ms['B']],
              'F_all_ms': [round(v, 4) for v in ms['F']],
              'filter_bytes': moved, 'filter_GBps': round(moved / (med['F'] * 1e-3) / 1e9, 1),
              'fill_ms': round(med['fill'], 4), 'fill_GBps': round(nbytes / (med['fill'] * 1e-3) / 1e9, 1),
              'filter_over_fill': round(moved / med['F'] / (nbytes / med['fill']), 3),
              'fill_source': 'hipMemsetAsync of the 3-byte raster on the stream, as bench.py --full measures it',
              'image_checked': True})
    for c in (tent_ctx, box_ctx, plain):
        c.close()
    del out8, samples8
