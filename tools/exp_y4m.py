#!/usr/bin/env python3
"""tools/exp_y4m.py — what raw video costs, one GPU, one process.
  1. The conversion kernel at SIZE^2 (maray_hip_time_rgb_to_ycc, events): maray_rgb_to_ycc against a device-to-device
     hipMemcpyAsync that moves as many bytes (4.5 w h at 4:2:0, 6 w h at 4:4:4), timed in the same call.  Per sampling and matrix
     the median of ROUNDS rounds of REPS repetitions after one untimed call.
  2. Nine frames of `maray_scenes`' chess_slide_1024 (the board under translate(var t)) rescaled to SIZE^2 on one JIT context,
     alternating:
       T  nine times set_params + maray_hip_render_tiles of the whole image into a pinned host raster (what there was for getting
          nine frames to the host);
       Y  one Context.render_y4m of the nine rows of values, 4:2:0 (and once 4:4:4): the whole file assembled in host memory
          and copied into a Python bytes object;
       N  one gen_animation(container=CONTAINER_Y4M) of the same values to /dev/null: the writer's pipeline -- render, convert,
          copy, hand over -- with a sink that keeps nothing.
     Wall time per frame, the median of ROUNDS rounds after one untimed call of each; the bytes that cross to the host either
     way; and, at sizes up to 1024^2, that Y's planes are tests/ycc_model.py's of T's rasters.
One JSON line per measurement.  --rounds N (default 5), --reps N (default 10), --size N (default 4096), --out FILE: appended."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
import ycc_model as Y  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS, SIZE = arg('--rounds', 5), arg('--reps', 10), arg('--size', 4096)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
FRAMES, FROM, TO = 9, -200.0, 200.0


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
for sampling, s_name in ((M.YCC_420, '420'), (M.YCC_444, '444')):
    for matrix, m_name in ((M.YCC_BT601, '601'), (M.YCC_BT709, '709')):
        M.time_rgb_to_ycc(SIZE, SIZE, sampling, matrix, reps=2)
        rounds = [M.time_rgb_to_ycc(SIZE, SIZE, sampling, matrix, reps=REPS) for _ in range(ROUNDS)]
        k_ms, c_ms = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
        moved = 3 * SIZE * SIZE + M.ycc_frame_bytes(SIZE, SIZE, sampling)
        emit({'what': 'rgb_to_ycc kernel', 'size': SIZE, 'sampling': s_name, 'matrix': m_name, 'rounds': ROUNDS, 'reps': REPS, 'bytes_moved': moved,
              'kernel_ms': round(k_ms, 4), 'kernel_all_ms': [round(r[0], 4) for r in rounds], 'kernel_moved_GBps': round(moved / (k_ms * 1e-3) / 1e9, 1),
              'copy_ms': round(c_ms, 4), 'copy_all_ms': [round(r[1], 4) for r in rounds], 'copy_moved_GBps': round(moved / (c_ms * 1e-3) / 1e9, 1),
              'kernel_over_copy': round(k_ms / c_ms, 2),
              'copy_source': 'hipMemcpyAsync device to device of half the bytes moved, events on the same stream, same call'})

# ---- 2. nine frames to the host ---------------------------------------------------------------------------------------------
tmp = tempfile.mkdtemp(prefix='exp_y4m_')
subprocess.check_call([os.path.join(ROOT, 'maray_amd', 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)
scene = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
if SIZE != 1024:
    scene.rescale(SIZE // 1024, SIZE // 1024)
scene.declare_param('t', FROM, TO)          # (in the scene's own units: a rescaled scene samples the original)
values = np.array([[TO if i == FRAMES - 1 else FROM + i * (TO - FROM) / (FRAMES - 1)] for i in range(FRAMES)])
ctx = M.Context(scene.lower(), backend=M.BACKEND_JIT, hint_mpixels=(SIZE * SIZE >> 20) + 1)
pin = M.PinnedRaster(SIZE, SIZE)
kept = []


def tiles(keep=False):
    for v in values:
        ctx.set_params(v)
        ctx.render_rows_into(SIZE, SIZE, 0, SIZE, pin.array)
        if keep:
            kept.append(pin.array.copy())


def y4m(sampling=M.YCC_420):
    return ctx.render_y4m(SIZE, SIZE, values, fps=12, sampling=sampling)


tiles(keep=SIZE <= 1024)
data = y4m()
checked = False
if SIZE <= 1024:
    assert Y.frames_equal(Y.parse(data), kept)
    checked = True
y4m(M.YCC_444)


def to_null():
    M.gen_animation(scene, '/dev/null', values, fps=12, backend=M.BACKEND_JIT, n_devices=1, container=M.CONTAINER_Y4M)


to_null()
ms = {'T': [], 'Y': [], 'Y444': [], 'N': []}
for _ in range(ROUNDS):
    for name, fn in (('T', tiles), ('Y', y4m), ('Y444', lambda: y4m(M.YCC_444)), ('N', to_null)):
        t0 = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t0) * 1e3 / FRAMES)
med = {n: float(np.median(v)) for n, v in ms.items()}
emit({'what': 'chess_slide nine frames to the host', 'size': SIZE, 'frames': FRAMES, 'backend': 'jit', 'rounds': ROUNDS,
      'T_tiles_ms_per_frame': round(med['T'], 3), 'T_all_ms': [round(v, 3) for v in ms['T']],
      'Y_y4m_420_ms_per_frame': round(med['Y'], 3), 'Y_all_ms': [round(v, 3) for v in ms['Y']],
      'Y_y4m_444_ms_per_frame': round(med['Y444'], 3), 'Y444_all_ms': [round(v, 3) for v in ms['Y444']],
      'N_y4m_420_to_dev_null_ms_per_frame': round(med['N'], 3), 'N_all_ms': [round(v, 3) for v in ms['N']], 'N_over_T': round(med['N'] / med['T'], 3),
      'Y_over_T': round(med['Y'] / med['T'], 3), 'Y444_over_T': round(med['Y444'] / med['T'], 3),
      'T_bytes_to_host_per_frame': 3 * SIZE * SIZE, 'Y_bytes_to_host_per_frame': M.ycc_frame_bytes(SIZE, SIZE, M.YCC_420),
      'Y444_bytes_to_host_per_frame': M.ycc_frame_bytes(SIZE, SIZE, M.YCC_444), 'file_bytes_420': len(data),
      'T_host_GBps': round(3 * SIZE * SIZE / (med['T'] * 1e-3) / 1e9, 2), 'Y_host_GBps': round(M.ycc_frame_bytes(SIZE, SIZE, M.YCC_420) / (med['Y'] * 1e-3) / 1e9, 2),
      'N_host_GBps': round(M.ycc_frame_bytes(SIZE, SIZE, M.YCC_420) / (med['N'] * 1e-3) / 1e9, 2),
      'planes_checked_against_the_model': checked})
ctx.close()
