#!/usr/bin/env python3
"""tools/exp_apng.py — what the animation writer costs, one GPU.
  1. The frame-delta kernels at SIZE^2 (maray_hip_time_frame_delta_copy, events): maray_frame_delta + maray_frame_delta_box
     against a device-to-device hipMemcpyAsync of one raster's bytes timed in the same call -- the same 2 x 3 w h bytes moved.
     Median of ROUNDS rounds of REPS repetitions after one untimed call.
  2. End to end, `maray_scenes`' chess_slide_1024 (the board under translate(var t)) at 1024^2 and rescaled to SIZE^2, the CLI
     with --animate t=-200:200:9 --backend jit --gpus 1, alternating:
       S  --encoder device -o f%03d.png: nine stills, each a whole maray_gen call (what there was before --apng);
       A  --apng -o a.png: one file.
     Wall time of the process, the median of ROUNDS rounds after one untimed run of each (the first run of a scene builds its
     kernels into the code object cache); the same two ways as library calls in this process (nine gen calls with the device
     encoder against one gen_animation: no process start), alternating, median of ROUNDS after one untimed call of each; the
     sum of S's file sizes against A's file; in this process the bytes the encoders copied to the host for either way
     (maray_hip_png_bytes_to_host) and A's rectangles; and, at 1024^2, that A decodes (tests/apng_stream.py) to the stills'
     rasters.
One JSON line per measurement.  --rounds N (default 5), --reps N (default 20), --size N (default 4096), --out FILE: appended."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import apng_stream as A  # noqa: E402
import maray_amd as M  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS, SIZE = arg('--rounds', 5), arg('--reps', 20), arg('--size', 4096)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
FRAMES, FROM, TO = 9, -200.0, 200.0
EXE = os.path.join(ROOT, 'maray_amd', 'maray')


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
M.time_frame_delta(SIZE, SIZE, reps=2, with_copy=True)
rounds = [M.time_frame_delta(SIZE, SIZE, reps=REPS, with_copy=True) for _ in range(ROUNDS)]
k_ms, c_ms = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
nbytes = 3 * SIZE * SIZE
emit({'what': 'frame delta kernels', 'size': SIZE, 'rounds': ROUNDS, 'reps': REPS, 'raster_bytes': nbytes,
      'delta_ms': round(k_ms, 4), 'delta_all_ms': [round(r[0], 4) for r in rounds], 'delta_read_GBps': round(2 * nbytes / (k_ms * 1e-3) / 1e9, 1),
      'copy_ms': round(c_ms, 4), 'copy_all_ms': [round(r[1], 4) for r in rounds], 'copy_moved_GBps': round(2 * nbytes / (c_ms * 1e-3) / 1e9, 1),
      'delta_over_copy': round(k_ms / c_ms, 2),
      'copy_source': 'hipMemcpyAsync device to device of one raster, events on the same stream, same call'})

# ---- 2. end to end ----------------------------------------------------------------------------------------------------------
tmp = tempfile.mkdtemp(prefix='exp_apng_')
subprocess.check_call([os.path.join(ROOT, 'maray_amd', 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)


def wall(cmd):
    t0 = time.perf_counter()
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return (time.perf_counter() - t0) * 1e3


for n in sorted({1024, SIZE}):
    scene = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
    if n != 1024:
        scene.rescale(n // 1024, n // 1024)
    path = os.path.join(tmp, 'slide_%d.maray' % n)
    scene.save(path)
    stills, apng = os.path.join(tmp, 'f%d_%%03d.png' % n), os.path.join(tmp, 'a%d.png' % n)
    common = [EXE, '-i', path, '--animate', 't=%g:%g:%d' % (FROM, TO, FRAMES), '--backend', 'jit', '--gpus', '1']
    cmd_s, cmd_a = common + ['-o', stills, '--encoder', 'device'], common + ['-o', apng, '--apng']
    wall(cmd_s); wall(cmd_a)
    ms = {'S': [], 'A': []}
    for _ in range(ROUNDS):
        ms['S'].append(wall(cmd_s))
        ms['A'].append(wall(cmd_a))
    still_files = [stills % i for i in range(FRAMES)]
    s_bytes, a_bytes = sum(os.path.getsize(p) for p in still_files), os.path.getsize(apng)
    checked = False
    d = None
    if n == 1024:
        d = A.decode(open(apng, 'rb').read())
        assert len(d.frames) == FRAMES and all(np.array_equal(d.frames[i], M.png_read(still_files[i])) for i in range(FRAMES))
        checked = True
    # in this process: what crosses to the host either way, and the rectangles
    scene.declare_param('t', FROM, TO)
    values = [FROM if FRAMES == 1 else TO if i == FRAMES - 1 else FROM + i * (TO - FROM) / (FRAMES - 1) for i in range(FRAMES)]

    def lib_s():
        for i, v in enumerate(values):
            scene.set_param('t', v)
            M.gen(scene, os.path.join(tmp, 'p%03d.png' % i), backend=M.BACKEND_JIT, n_devices=1, encoder=M.ENCODER_DEVICE)

    def lib_a():
        M.gen_animation(scene, os.path.join(tmp, 'p.png'), {'t': values}, backend=M.BACKEND_JIT, n_devices=1)

    b0 = M.png_bytes_to_host()
    lib_s()
    b1 = M.png_bytes_to_host()
    lib_a()
    b2 = M.png_bytes_to_host()
    lib_ms = {'S': [], 'A': []}             # the same two ways as library calls in this process: no process start, no module load
    for _ in range(ROUNDS):
        for k, fn in (('S', lib_s), ('A', lib_a)):
            t0 = time.perf_counter()
            fn()
            lib_ms[k].append((time.perf_counter() - t0) * 1e3)
    assert open(os.path.join(tmp, 'p.png'), 'rb').read() == open(apng, 'rb').read()
    rects = d.rects if d else None
    if rects is None:           # the rectangles from the fcTL chunks alone (no inflate of 9 x 48 MiB)
        import struct
        import png_stream as P
        rects = [struct.unpack('>IIII', c[4:20]) for k, c in P.chunks(open(apng, 'rb').read()) if k == b'fcTL']
        rects = [(x, y, w, h) for w, h, x, y in rects]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    emit({'what': 'chess_slide end to end', 'size': n, 'frames': FRAMES, 'animate': 't=%g:%g:%d' % (FROM, TO, FRAMES), 'backend': 'jit', 'rounds': ROUNDS,
          'S_stills_wall_ms': round(med['S'], 1), 'S_all_ms': [round(v, 1) for v in ms['S']],
          'A_apng_wall_ms': round(med['A'], 1), 'A_all_ms': [round(v, 1) for v in ms['A']], 'A_over_S': round(med['A'] / med['S'], 3),
          'S_in_process_ms': round(float(np.median(lib_ms['S'])), 2), 'S_in_process_all_ms': [round(v, 2) for v in lib_ms['S']],
          'A_in_process_ms': round(float(np.median(lib_ms['A'])), 2), 'A_in_process_all_ms': [round(v, 2) for v in lib_ms['A']],
          'A_over_S_in_process': round(float(np.median(lib_ms['A']) / np.median(lib_ms['S'])), 3),
          'S_files_bytes': s_bytes, 'A_file_bytes': a_bytes, 'A_over_S_bytes': round(a_bytes / s_bytes, 3),
          'S_bytes_to_host': int(b1 - b0), 'A_bytes_to_host': int(b2 - b1), 'rects_xywh': [list(map(int, r)) for r in rects],
          'frames_checked_against_stills': checked})
    M.gen_cache_clear()
