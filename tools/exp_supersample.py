#!/usr/bin/env python3
"""tools/exp_supersample.py — supersampled chess @4096^2 (the bench scene) on one GPU, k = 2 and 4, in one process.

For each k it times, alternating in the same call:
  A  the supersampling launch over output geometry: time_rows on a context with samples = k (RGB8 into HBM);
  B  the plain launch of the same supersampled program over the k w x k h sample grid (RGB8 into HBM),
on each back-end (specialised kernels, scalar-cache interpreter, LDS interpreter).  It checks that every A image equals
the box filter of the specialised kernels' B image, and prints one JSON line per (k, launch, back-end): us per launch,
samples per second and output pixels per second.  --rounds N: alternations (default 5)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402

import maray_amd as M  # noqa: E402
from test_gpu_supersample import box  # noqa: E402

N, REPS = 4096, 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
data = open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read()
names = {M.BACKEND_TAPE: 'tape', M.BACKEND_TAPE_SMEM: 'tape_smem', M.BACKEND_JIT: 'jit'}
for k in (2, 4):
    s = M.Scene(data)
    s.rescale(N // 1024, N // 1024)
    s.supersample(k)
    tape = s.lower()
    kinds = (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE)
    a = {x: M.Context(tape, backend=x, samples=k) for x in kinds}
    b = {x: M.Context(tape, backend=x) for x in kinds}
    # correctness first: A's image = box filter of B's, in bands of output rows
    for y0 in range(0, N, 512):
        want = box(b[M.BACKEND_JIT].render_rows(N * k, N * k, y0 * k, (y0 + 512) * k, want_f64=False)[0], k)
        for ctx in a.values():
            assert np.array_equal(ctx.render_rows(N, N, y0, y0 + 512, want_f64=False)[0], want), (k, y0, ctx.kernel_name)
    times = {}
    for _ in range(ROUNDS):                      # alternating: every launch kind sees the same clocks and neighbours
        for x, ctx in a.items():
            times.setdefault(('A', x), []).append(ctx.time_rows(N, N, 0, N, reps=REPS))
        for x, ctx in b.items():
            times.setdefault(('B', x), []).append(ctx.time_rows(N * k, N * k, 0, N * k, reps=REPS))
    for (kind, x), ms in sorted(times.items(), key=lambda t: (t[0][0], t[0][1])):
        med = float(np.median(ms))
        print(json.dumps({'k': k, 'launch': kind, 'backend': names[x], 'kernel': (a if kind == 'A' else b)[x].kernel_name,
                          'us_median': round(med * 1e3, 1), 'us_all': [round(v * 1e3, 1) for v in ms],
                          'samples_per_s': round(N * N * k * k / (med * 1e-3) / 1e9, 2) * 1e9,
                          'output_pixels_per_s': round(N * N / (med * 1e-3) / 1e9, 3) * 1e9,
                          'image_checked': True}), flush=True)
    for ctx in list(a.values()) + list(b.values()):
        ctx.close()
