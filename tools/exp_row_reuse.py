#!/usr/bin/env python3
"""tools/exp_row_reuse.py — what keeping a geometry's ROW outputs saves where the inputs really repeat:
animations and shutters on the specialised kernels, MARAY_JIT_ROW_REUSE=0 against the default, one GPU, one process.

Scenes, at 1024^2 and rescaled to 4096^2:
  chess_fade    the committed chess with every channel multiplied by var t: a parameter only PIXEL ops read (the gain arrives);
  chess_slide   `maray_scenes`' chess_slide_1024, the board under translate(var t): ROW-read (must not get worse).
Per (scene, size, n in 8, 64), for a context of each kind, alternating:
  A  the shutter call into HBM (render_rows_shutter_device, n frames + the reduce passes);
  B  n plain launches with set_params between them (an animation), per frame;
each the median of ROUNDS x REPS between events that end in a synchronise; the two contexts' shutter images are compared and
the ROW passes / order kernels each enqueued are reported.  One JSON line per (scene, size, n).
--rounds N (default 5), --out FILE: the lines, appended; --commit ID: recorded in every line."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
from marayb import decode, encode, mul, var  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


REPS = 10
ROUNDS = int(arg('--rounds', 5))
OUT = arg('--out', None)
COMMIT = arg('--commit', None)
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


def context(tape, reuse):
    old = os.environ.get('MARAY_JIT_ROW_REUSE')
    os.environ['MARAY_JIT_ROW_REUSE'] = '1' if reuse else '0'          # read when the context is created
    try:
        return M.Context(tape, backend=M.BACKEND_JIT)
    finally:
        if old is None:
            del os.environ['MARAY_JIT_ROW_REUSE']
        else:
            os.environ['MARAY_JIT_ROW_REUSE'] = old


def scenes(tmp):
    size, color = decode(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())[:2]
    fade = M.Scene(encode(tuple(size), [mul(c, var('t')) for c in color]))
    fade.declare_param('t', 0.0, 1.0)
    fade.set_param('t', 0.5)
    fade.set_param_span('t', 1.0)
    yield 'chess_fade', fade
    subprocess.check_call([os.path.join(ROOT, 'maray_amd', 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)
    slide = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
    slide.declare_param('t', -1024.0, 1024.0)
    slide.set_param('t', 0.0)
    slide.set_param_span('t', SPAN)
    yield 'chess_slide', slide


stream = torch.cuda.Stream()
tmp_dir = tempfile.mkdtemp(prefix='maray_row_reuse_')
for name, scene in scenes(tmp_dir):
    for N in (1024, 4096):
        if N != 1024:
            scene.rescale(N // 1024, N // 1024)
        tape = scene.lower()
        ctxs = {'off': context(tape, False), 'on': context(tape, True)}
        outs = {k: torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda') for k in ctxs}
        with torch.cuda.stream(stream):
            for n in (8, 64):
                rows = scene.shutter_values(n)

                def run_a(k):
                    ctxs[k].render_rows_shutter_device(N, N, 0, N, rows, outs[k].data_ptr(), stream=stream.cuda_stream)

                def run_b(k):
                    for r in rows:
                        ctxs[k].set_params(list(r))
                        ctxs[k].render_rows_device(N, N, 0, N, d_rgb8=outs[k].data_ptr(), stream=stream.cuda_stream)

                for k in ctxs:
                    run_b(k); run_a(k)
                stream.synchronize()
                same = bool(torch.equal(outs['off'], outs['on'])) and float(outs['on'].float().std()) > 0
                before = {k: ctxs[k].launch_counts for k in ctxs}
                ms = {(f, k): [] for f in 'AB' for k in ctxs}
                for _ in range(ROUNDS):                 # alternating: every kind sees the same clocks and neighbours
                    for k in ctxs:
                        ms[('A', k)].append(timed(lambda: run_a(k), stream))
                        ms[('B', k)].append(timed(lambda: run_b(k), stream) / n)
                med = {fk: float(np.median(v)) for fk, v in ms.items()}
                launches = 2 * ROUNDS * REPS * n
                emit({'scene': name + ('' if N == 1024 else ' rescaled to %d^2' % N), 'size': N, 'n': n, 'backend': 'jit', 'kernel': ctxs['on'].kernel_name,
                      'row_params': tape.info['row_params'], 'rounds': ROUNDS, 'reps': REPS, 'commit': COMMIT, 'code_key': tape.jit_code_key,
                      'A_shutter_ms_off': round(med[('A', 'off')], 4), 'A_shutter_ms_on': round(med[('A', 'on')], 4),
                      'B_frame_us_off': round(med[('B', 'off')] * 1e3, 2), 'B_frame_us_on': round(med[('B', 'on')] * 1e3, 2),
                      'A_all_ms_off': [round(v, 4) for v in ms[('A', 'off')]], 'A_all_ms_on': [round(v, 4) for v in ms[('A', 'on')]],
                      'B_all_us_off': [round(v * 1e3, 2) for v in ms[('B', 'off')]], 'B_all_us_on': [round(v * 1e3, 2) for v in ms[('B', 'on')]],
                      'timed_launches': launches,
                      'row_passes_timed': {k: ctxs[k].launch_counts[0] - before[k][0] for k in ctxs},
                      'order_kernels_timed': {k: ctxs[k].launch_counts[1] - before[k][1] for k in ctxs},
                      'images_equal': same})
        for c in ctxs.values():
            c.close()
shutil.rmtree(tmp_dir, ignore_errors=True)
