#!/usr/bin/env python3
"""tools/exp_catrom.py — what the Catmull-Rom reconstruction filter costs on the device beside the tent: chess rescaled to
4096^2, k = 2 and 4, specialised kernels, one GPU, one process.  Per k it times, alternating:
  T       the Catmull-Rom call into HBM (a samples = k, filter = catrom context: per band a plain launch into scratch +
          maray_filter_catrom<k>);
  T_tent  the tent call of a samples = k, filter = tent context;
  B       the plain launch of the same program over the k N x k N sample grid into one buffer;
  F       maray_filter_catrom<k> alone on samples already in HBM (maray_hip_time_filter_ex);
  F_tent  maray_filter_tent<k> alone (maray_hip_time_filter): the yardstick,
each the median of ROUNDS x REPS between events that end in a synchronise.  Both kernels have to move (3 k^2 + 3) bytes per
output pixel; beside their rates the fill rate bench.py --full reports, measured here the same way (hipMemsetAsync of the
3-byte output raster on the stream).  Both timed pictures are checked against the numpy contracts applied to B's samples.
One JSON line per k.  --rounds N (default 5), --size N (default 4096), --ks 2,4 (default), --out FILE: the lines, appended."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
from catrom_model import catrom  # noqa: E402
from test_filter import tent  # noqa: E402

REPS = 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
SIZE = int(sys.argv[sys.argv.index('--size') + 1]) if '--size' in sys.argv else 4096
KS = [int(v) for v in sys.argv[sys.argv.index('--ks') + 1].split(',')] if '--ks' in sys.argv else [2, 4]
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
for k in KS:
    scene = M.Scene.open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'))
    if N != 1024:
        scene.rescale(N // 1024, N // 1024)
    scene.supersample(k)
    tape = scene.lower()
    cat_ctx = M.Context(tape, backend=M.BACKEND_JIT, samples=k, filter=M.FILTER_CATROM)
    tent_ctx = M.Context(tape, backend=M.BACKEND_JIT, samples=k, filter=M.FILTER_TENT)
    plain = M.Context(tape, backend=M.BACKEND_JIT)
    out8 = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
    tent8 = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
    samples8 = torch.zeros((N * k, N * k, 3), dtype=torch.uint8, device='cuda')
    nbytes = out8.numel()
    with torch.cuda.stream(stream):
        def run_t():
            cat_ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)

        def run_tent():
            tent_ctx.render_rows_device(N, N, 0, N, d_rgb8=tent8.data_ptr(), stream=stream.cuda_stream)

        def run_b():
            plain.render_rows_device(N * k, N * k, 0, N * k, d_rgb8=samples8.data_ptr(), stream=stream.cuda_stream)

        def run_fill():
            hip.hipMemsetAsync(out8.data_ptr(), 0, nbytes, stream.cuda_stream)

        def check():
            """T and T_tent = the contracts applied to B's samples, on a band of rows across the board's edge (two output rows
            more on both sides: those clamp to the band, not the image) and on the image's first and last rows."""
            stream.synchronize()
            y0, y1 = N // 2 - 64, N // 2 + 192
            band = samples8[(y0 - 2) * k:(y1 + 2) * k].cpu().numpy()
            assert np.array_equal(out8[y0:y1].cpu().numpy(), catrom(band, k)[2:-2]), k
            assert np.array_equal(tent8[y0:y1].cpu().numpy(), tent(band, k)[2:-2]), k
            assert np.array_equal(out8[:16].cpu().numpy(), catrom(samples8[:18 * k].cpu().numpy(), k)[:16]), k
            assert np.array_equal(out8[-16:].cpu().numpy(), catrom(samples8[-18 * k:].cpu().numpy(), k)[-16:]), k

        run_b(); run_t(); run_tent()
        check()
        ms = {'T': [], 'T_tent': [], 'B': [], 'F': [], 'F_tent': [], 'fill': []}
        for fn in (run_t, run_tent, run_b, run_fill):
            fn(); fn()
        stream.synchronize()
        for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
            ms['T'].append(timed(run_t, stream))
            ms['T_tent'].append(timed(run_tent, stream))
            ms['B'].append(timed(run_b, stream))
            ms['F'].append(M.time_filter(N, N, k, reps=REPS, filter=M.FILTER_CATROM))
            ms['F_tent'].append(M.time_filter(N, N, k, reps=REPS))
            ms['fill'].append(timed(run_fill, stream))
        run_b(); run_t(); run_tent()
        check()                                  # the pictures that were timed
        med = {n: float(np.median(v)) for n, v in ms.items()}
        moved = (3 * k * k + 3) * N * N
        emit({'scene': 'chess' + ('' if N == 1024 else ' rescaled to %d^2' % N), 'size': N, 'k': k, 'backend': 'jit', 'kernel': cat_ctx.kernel_name,
              'rounds': ROUNDS, 'reps': REPS, 'band_rows_env': os.environ.get('MARAY_FILTER_BAND_ROWS'),
              'T_catrom_ms': round(med['T'], 4), 'T_tent_ms': round(med['T_tent'], 4), 'B_plain_samples_ms': round(med['B'], 4),
              'F_catrom_ms': round(med['F'], 4), 'F_tent_ms': round(med['F_tent'], 4), 'F_over_F_tent': round(med['F'] / med['F_tent'], 3),
              'T_minus_B_ms': round(med['T'] - med['B'], 4), 'T_over_T_tent': round(med['T'] / med['T_tent'], 3),
              'T_all_ms': [round(v, 4) for v in ms['T']], 'T_tent_all_ms': [round(v, 4) for v in ms['T_tent']], 'B_all_ms': [round(v, 4) for v in ms['B']],
              'F_all_ms': [round(v, 4) for v in ms['F']], 'F_tent_all_ms': [round(v, 4) for v in ms['F_tent']],
              'filter_bytes': moved, 'catrom_GBps': round(moved / (med['F'] * 1e-3) / 1e9, 1), 'tent_GBps': round(moved / (med['F_tent'] * 1e-3) / 1e9, 1),
              'fill_ms': round(med['fill'], 4), 'fill_GBps': round(nbytes / (med['fill'] * 1e-3) / 1e9, 1),
              'fill_source': 'hipMemsetAsync of the 3-byte raster on the stream, as bench.py --full measures it',
              'images_checked': True})
    for c in (cat_ctx, tent_ctx, plain):
        c.close()
    del out8, tent8, samples8
