#!/usr/bin/env python3
"""tools/exp_shutter.py — what motion blur costs on the device: `maray_scenes`' chess_slide_1024 (the board under translate(var t)),
as it is and rescaled to 4096^2, specialised kernels, n = 8 and 64 frames over a span of 80 pixels, one GPU, one process
(DESIGN.md 4.7).  Per (size, n) it times, alternating:
  A  the shutter call into HBM (render_rows_shutter_device: n launches with their values + the reduce passes);
  B  the same n plain launches with set_params between them and no reduce (render_rows_device into one buffer);
  R  the reduce passes alone on frames already in HBM (maray_hip_time_shutter_reduce),
each the median of ROUNDS x REPS, A and B between events that end in a synchronise.  R's achieved bytes per second counts
what the passes move: (3 n + 3) bytes per pixel for n <= 8, (3 n + 3 + accumulator bytes) above (the 16-bit partial sums: 6
bytes per pixel written by every pass but the last and read by every pass but the first); beside it the fill rate bench.py --full reports,
measured here the same way (hipMemsetAsync of the 3-byte raster on the stream).  A's image is checked against the integer
mean of B's frames.  One JSON line per (size, n).  --rounds N (default 5), --out FILE: the lines, appended."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402

REPS = 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SPAN = 80.0


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


tmp = tempfile.mkdtemp(prefix='maray_shutter_')
subprocess.check_call([os.path.join(ROOT, 'maray_amd', 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)
hip = C.CDLL('libamdhip64.so')
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
stream = torch.cuda.Stream()
for N in (1024, 4096):
    scene = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
    scene.declare_param('t', -1024.0, 1024.0)
    scene.set_param('t', 0.0)
    scene.set_param_span('t', SPAN)
    if N != 1024:
        scene.rescale(N // 1024, N // 1024)
    ctx = M.Context(scene.lower(), backend=M.BACKEND_JIT)
    out8 = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
    nbytes = out8.numel()
    with torch.cuda.stream(stream):
        for n in (8, 64):
            rows = scene.shutter_values(n)
            # correctness first: A = the integer mean of B's frames
            total = np.zeros((N, N, 3), np.uint32)
            for r in rows:
                ctx.set_params(list(r))
                ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                total += out8.cpu().numpy()
            ctx.render_rows_shutter_device(N, N, 0, N, rows, out8.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(out8.cpu().numpy(), ((total + n // 2) >> (n.bit_length() - 1)).astype(np.uint8)), (N, n)

            def run_a():
                ctx.render_rows_shutter_device(N, N, 0, N, rows, out8.data_ptr(), stream=stream.cuda_stream)

            def run_b():
                for r in rows:
                    ctx.set_params(list(r))
                    ctx.render_rows_device(N, N, 0, N, d_rgb8=out8.data_ptr(), stream=stream.cuda_stream)

            def run_fill():
                hip.hipMemsetAsync(out8.data_ptr(), 0, nbytes, stream.cuda_stream)

            ms = {'A': [], 'B': [], 'R': [], 'fill': []}
            run_a(); run_b(); run_fill()
            stream.synchronize()
            for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
                ms['A'].append(timed(run_a, stream))
                ms['B'].append(timed(run_b, stream))
                r = C.c_float()
                M.api._check(M.api.lib().maray_hip_time_shutter_reduce(0, nbytes, n, REPS, C.byref(r)))
                ms['R'].append(r.value)
                ms['fill'].append(timed(run_fill, stream))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            passes = (n + 7) // 8
            # the 16-bit partial sums: 6 B per pixel written by every pass but the last, 6 B read by every pass but the first
            acc_per_pixel = 12 * (passes - 1)
            moved = (3 * n + 3 + acc_per_pixel) * N * N
            emit({'scene': 'chess_slide_1024' + ('' if N == 1024 else ' rescaled to %d^2' % N), 'size': N, 'n': n, 'backend': 'jit', 'kernel': ctx.kernel_name,
                  'span': SPAN, 'rounds': ROUNDS, 'reps': REPS,
                  'A_shutter_ms': round(med['A'], 4), 'B_plain_launches_ms': round(med['B'], 4), 'R_reduce_ms': round(med['R'], 4),
                  'A_minus_B_ms': round(med['A'] - med['B'], 4),
                  'A_all_ms': [round(v, 4) for v in ms['A']], 'B_all_ms': [round(v, 4) for v in ms['B']], 'R_all_ms': [round(v, 4) for v in ms['R']],
                  'reduce_passes': passes, 'reduce_bytes': moved, 'reduce_GBps': round(moved / (med['R'] * 1e-3) / 1e9, 1),
                  'fill_ms': round(med['fill'], 4), 'fill_GBps': round(nbytes / (med['fill'] * 1e-3) / 1e9, 1),
                  'fill_source': 'hipMemsetAsync of the 3-byte raster on the stream, as bench.py --full measures it',
                  'frames_per_s_A': round(1e3 / med['A'], 1), 'image_checked': True})
    ctx.close()
