#!/usr/bin/env python3
"""tools/exp_linear.py — what the reduces in linear light cost on the device (include/maray_hip.h, "transfer"):
chess rescaled to 4096^2, k = 2 and 4, specialised kernels, one GPU, one process.  Per k it times, alternating:
  LB, LT  the box and tent calls of MARAY_TRANSFER_SRGB contexts into HBM (per band a plain launch into scratch +
          maray_filter_box_lin<k> / maray_filter_tent_lin<k>);
  T, X    today's tent call (maray_filter_tent<k>) and today's in-kernel box call;
  B       the plain launch of the same program over the k N x k N sample grid into one buffer;
  the kernels alone on samples already in HBM (maray_hip_time_filter_ex: scratch of the call's own, every byte 0x5A -- ONE value,
  so every table read of a wavefront is a broadcast: the best case of the LDS tables, which the calls above do not have):
  FLB, FLT maray_filter_box_lin<k>, maray_filter_tent_lin<k>; FT maray_filter_tent<k>;
  SL, S   maray_shutter_reduce_lin and maray_shutter_reduce over 8 frames of the N x N raster (maray_hip_time_shutter_reduce_ex);
  fill    hipMemsetAsync of the 3-byte output raster on the stream, as bench.py --full measures it,
each the median of ROUNDS x REPS between events that end in a synchronise; then the kernels alone again with
MARAY_TIME_RANDOM_BYTES=1, pseudo-random sample bytes: table reads spread over all entries, the worst case (*_random_ms).  LB's and LT's images are checked against the numpy
contracts applied to B's samples.  One JSON line per k.  --rounds N (default 5), --size N (default 4096), --out FILE: appended."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import linear_light as LL  # noqa: E402
import maray_amd as M  # noqa: E402

REPS = 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
SIZE = int(sys.argv[sys.argv.index('--size') + 1]) if '--size' in sys.argv else 4096
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SHUTTER_N = 8


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
    ctxs = {'LB': M.Context(tape, backend=M.BACKEND_JIT, samples=k, transfer=M.TRANSFER_SRGB),
            'LT': M.Context(tape, backend=M.BACKEND_JIT, samples=k, filter=M.FILTER_TENT, transfer=M.TRANSFER_SRGB),
            'T': M.Context(tape, backend=M.BACKEND_JIT, samples=k, filter=M.FILTER_TENT),
            'X': M.Context(tape, backend=M.BACKEND_JIT, samples=k)}
    plain = M.Context(tape, backend=M.BACKEND_JIT)
    out8 = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
    samples8 = torch.zeros((N * k, N * k, 3), dtype=torch.uint8, device='cuda')
    nbytes = out8.numel()
    with torch.cuda.stream(stream):
        plain.render_rows_device(N * k, N * k, 0, N * k, d_rgb8=samples8.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        y0, y1 = N // 2 - 64, N // 2 + 192
        band = samples8[(y0 - 1) * k:(y1 + 1) * k].cpu().numpy()        # one output row more on both sides: those two clamp to the band, not the image
        for name, contract in (('LB', LL.box_lin), ('LT', LL.tent_lin)):
            ctxs[name].render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(out8[y0:y1].cpu().numpy(), contract(band, k)[1:-1]), (name, k)

        def call(ctx):
            return lambda: ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)

        runs = {n: call(c) for n, c in ctxs.items()}
        runs['B'] = lambda: plain.render_rows_device(N * k, N * k, 0, N * k, d_rgb8=samples8.data_ptr(), stream=stream.cuda_stream)
        runs['fill'] = lambda: hip.hipMemsetAsync(out8.data_ptr(), 0, nbytes, stream.cuda_stream)
        alone = {'FLB': lambda: M.time_filter(N, N, k, reps=REPS, filter=M.FILTER_BOX, transfer=M.TRANSFER_SRGB),
                 'FLT': lambda: M.time_filter(N, N, k, reps=REPS, filter=M.FILTER_TENT, transfer=M.TRANSFER_SRGB),
                 'FT': lambda: M.time_filter(N, N, k, reps=REPS),
                 'SL': lambda: M.time_shutter_reduce(nbytes, SHUTTER_N, reps=REPS, transfer=M.TRANSFER_SRGB),
                 'S': lambda: M.time_shutter_reduce(nbytes, SHUTTER_N, reps=REPS)}
        ms = {n: [] for n in list(runs) + list(alone)}
        for fn in runs.values():
            fn(); fn()
        stream.synchronize()
        for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
            for n, fn in runs.items():
                ms[n].append(timed(fn, stream))
            for n, fn in alone.items():
                ms[n].append(fn())
        # the kernels alone once more on pseudo-random sample bytes (MARAY_TIME_RANDOM_BYTES: the tables' worst case), 2 x REPS each
        os.environ['MARAY_TIME_RANDOM_BYTES'] = '1'
        rnd = {n: [fn() for _ in range(2)] for n, fn in alone.items()}
        del os.environ['MARAY_TIME_RANDOM_BYTES']
        med = {n: float(np.median(v)) for n, v in ms.items()}
        moved = (3 * k * k + 3) * N * N
        d = {'scene': 'chess' + ('' if N == 1024 else ' rescaled to %d^2' % N), 'size': N, 'k': k, 'backend': 'jit', 'rounds': ROUNDS, 'reps': REPS,
             'kernels': {n: c.kernel_name for n, c in ctxs.items()}, 'shutter_frames': SHUTTER_N,
             'alone_samples': 'every byte 0x5A: table reads broadcast (best case)', 'image_checked': True}
        for n in ms:
            d[n + '_ms'] = round(med[n], 4)
            d[n + '_all_ms'] = [round(v, 4) for v in ms[n]]
        d.update({'LB_minus_B_ms': round(med['LB'] - med['B'], 4), 'LT_minus_B_ms': round(med['LT'] - med['B'], 4), 'T_minus_B_ms': round(med['T'] - med['B'], 4),
                  'LT_over_T': round(med['LT'] / med['T'], 3), 'LB_over_X': round(med['LB'] / med['X'], 3),
                  'FLT_over_FT': round(med['FLT'] / med['FT'], 3), 'FLB_over_FT': round(med['FLB'] / med['FT'], 3), 'SL_over_S': round(med['SL'] / med['S'], 3),
                  'filter_bytes': moved, 'FLB_GBps': round(moved / (med['FLB'] * 1e-3) / 1e9, 1), 'FLT_GBps': round(moved / (med['FLT'] * 1e-3) / 1e9, 1),
                  'FT_GBps': round(moved / (med['FT'] * 1e-3) / 1e9, 1),
                  'SL_GBps': round((SHUTTER_N + 1) * nbytes / (med['SL'] * 1e-3) / 1e9, 1), 'S_GBps': round((SHUTTER_N + 1) * nbytes / (med['S'] * 1e-3) / 1e9, 1),
                  'fill_GBps': round(nbytes / (med['fill'] * 1e-3) / 1e9, 1),
                  'random_bytes': 'the kernels alone on pseudo-random sample bytes, the smaller of 2 x %d' % REPS})
        for n, v in rnd.items():
            d[n + '_random_ms'] = round(min(v), 4)
        d.update({'FLT_over_FT_random': round(min(rnd['FLT']) / min(rnd['FT']), 3), 'FLB_over_FT_random': round(min(rnd['FLB']) / min(rnd['FT']), 3),
                  'SL_over_S_random': round(min(rnd['SL']) / min(rnd['S']), 3),
                  'FLB_random_over_constant': round(min(rnd['FLB']) / med['FLB'], 3), 'FLT_random_over_constant': round(min(rnd['FLT']) / med['FLT'], 3),
                  'SL_random_over_constant': round(min(rnd['SL']) / med['SL'], 3)})
        emit(d)
    for c in list(ctxs.values()) + [plain]:
        c.close()
    del out8, samples8
