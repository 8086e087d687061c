#!/usr/bin/env python3
"""tools/exp_params.py — what a new frame of an animation costs: chess under translate(var t, 0), rescaled to 4096^2, on one GPU,
in one process.  Per back-end it times, alternating:
  A  set_params + render_rows_device of the parameterised program, a new value every frame;
  B  render_rows_device of the SAME scene with the value substituted (a constant where the parameter was), lowered and built as a
     scene without parameters is: the floor, the same picture from a program that cannot move;
and once, in a fresh code-object cache directory:
  C  the first gen_to_image call on a substituted scene nothing has seen (what a new frame costs without parameters).
Median of ROUNDS x REPS launches timed with events that end in a synchronise.  A's image is checked against B's for the
value B was built with.  One JSON line per (launch, back-end).  --rounds N (default 5), --out FILE: the lines, appended."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ['MARAY_CACHE_DIR'] = tempfile.mkdtemp(prefix='maray_params_cache_')
import maray_amd as M  # noqa: E402
import params as PR  # noqa: E402
from marayb import decode, encode, sub, subst_xy_deep, var, x, y  # noqa: E402

N, REPS = 4096, 10
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
names = {M.BACKEND_TAPE: 'tape', M.BACKEND_TAPE_SMEM: 'tape_smem', M.BACKEND_JIT: 'jit', M.BACKEND_AUTO: 'auto'}


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


size, color = decode(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())
slide = [subst_xy_deep(c, [sub(x(), var('t')), y()]) for c in color]      # t in pixels of the 1024^2 scene


def substituted(v):
    s = M.Scene(encode(size, PR.substituted(slide, ['t'], (v,))))
    s.rescale(N // size[0], N // size[1])
    return s


par = M.Scene(encode(size, slide))
par.declare_param('t', -1024.0, 1024.0)
par.rescale(N // size[0], N // size[1])
t0 = time.perf_counter()
tape_a = par.lower()
lower_a = time.perf_counter() - t0
V0 = 37.5
tape_b = substituted(V0).lower()
emit({'what': 'programs', 'a_version': tape_a.program.version, 'a_params': tape_a.param_count, 'lower_a_ms': round(lower_a * 1e3, 1),
      'a_ops': [tape_a.info['n_row_ops'], tape_a.info['n_pix_ops'], tape_a.info['n_yvals']],
      'b_ops': [tape_b.info['n_row_ops'], tape_b.info['n_pix_ops'], tape_b.info['n_yvals']]})
out = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
ref = torch.zeros_like(out)
stream = torch.cuda.current_stream().cuda_stream


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(REPS):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


for backend in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE):
    a, b = M.Context(tape_a, backend=backend), M.Context(tape_b, backend=backend)
    a.set_params([V0])
    a.render_rows_device(N, N, 0, N, d_rgb8=out.data_ptr(), stream=stream)
    b.render_rows_device(N, N, 0, N, d_rgb8=ref.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), names[backend]
    frame = [0]

    def step_a(i):
        frame[0] += 1
        a.set_params([-512.0 + (frame[0] * 7.25) % 1024.0])
        a.render_rows_device(N, N, 0, N, d_rgb8=out.data_ptr(), stream=stream)

    def step_b(i):
        b.render_rows_device(N, N, 0, N, d_rgb8=ref.data_ptr(), stream=stream)
    for fn in (step_a, step_b):
        timed(fn)                                   # warm-up of each kind
    ta, tb = [], []
    for _ in range(ROUNDS):                         # alternating: both kinds see the same clocks
        ta.append(timed(step_a))
        tb.append(timed(step_b))
    for kind, ms, ctx in (('A', ta, a), ('B', tb, b)):
        emit({'launch': kind, 'backend': names[backend], 'kernel': ctx.kernel_name, 'us_median': round(float(np.median(ms)) * 1e3, 1),
              'us_all': [round(v * 1e3, 1) for v in ms], 'image_checked': True})
    a.close()
    b.close()

for k, backend in enumerate((M.BACKEND_AUTO, M.BACKEND_JIT)):        # C: a frame without parameters is another scene
    M.gen_cache_clear()
    s = substituted(100.0 + 3.0 * k)
    img = np.zeros((N, N, 3), np.uint8)
    t0 = time.perf_counter()
    M.gen_to_image(s, backend=backend, n_devices=1, out=img)
    first = time.perf_counter() - t0
    emit({'launch': 'C', 'backend': names[backend], 'kernel': M.gen_cache_info()[0].split(' kernel ')[1].split()[0], 'first_call_ms': round(first * 1e3, 1)})
M.gen_cache_clear()
