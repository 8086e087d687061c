#!/usr/bin/env python3
"""tools/exp_png_dynamic.py — what the dynamic-Huffman codes of the device PNG encoder buy and cost, with
tools/exp_png.py's method: chess rescaled to SIZE^2 and the textured scene (config 5) at SIZE^2, specialised kernels, one GPU,
one process.  Per scene, alternating:
  Dfix  gen(scene, path, encoder=ENCODER_DEVICE): wall time per call (the parent's behaviour: the comparison);
  Ddyn  gen(scene, path, encoder=ENCODER_DEVICE | ENCODER_DYNAMIC): wall time per call;
  Kfix  the fixed coder's three kernels alone on the rendered raster in HBM as one band (events);
  Kdyn  the dynamic coder's kernels alone on it, the band's code fitted once before the timed loop (events; the host's round
        trip between the histogram and the emitter is not in K, it is in D),
each the median of ROUNDS rounds of REPS calls after one untimed call of each kind.  Also: the three files' sizes (the host
writer's too), the bytes each device coder copied to the host per call, and that all three files decode to gen_to_image's
raster.  Then `maray_scenes`' chess_slide_1024 rescaled to SIZE^2 as a nine-frame APNG (gen_animation in this process) with and
without the flag: bytes, library time, bytes to the host; the first and last frames of both files are compared.
One JSON line per scene.  --rounds N (default 5), --reps N (default 10), --size N (default 4096), --out FILE: the lines, appended."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # device buffers; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
import scenes  # noqa: E402
from marayb import encode  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS, SIZE = arg('--rounds', 5), arg('--reps', 10), arg('--size', 4096)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
N = SIZE
DYNAMIC = M.ENCODER_DEVICE | M.ENCODER_DYNAMIC
tmp = tempfile.mkdtemp(prefix='exp_png_dynamic_')


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


def wall(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def chess():
    s = M.Scene.open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'))
    if N != 1024:
        s.rescale(N // 1024, N // 1024)
    return s, None


def textured():
    return M.Scene(encode((N, N), scenes.textured(N))), scenes.textures(1)


def med(v):
    return float(np.median(v))


for name, make in (('chess', chess), ('textured (config 5)', textured)):
    scene, tex = make()
    paths = {k: os.path.join(tmp, k + '.png') for k in ('host', 'fixed', 'dynamic')}

    def run(kind):
        M.gen(scene, paths[kind], textures=tex, backend=M.BACKEND_JIT, n_devices=1,
              encoder={'host': M.ENCODER_HOST, 'fixed': M.ENCODER_DEVICE, 'dynamic': DYNAMIC}[kind])

    for kind in paths:
        run(kind)
    want = M.gen_to_image(scene, textures=tex, backend=M.BACKEND_JIT, n_devices=1)
    assert all(np.array_equal(M.png_read(p), want) for p in paths.values())
    to_host = {}
    for kind in ('fixed', 'dynamic'):
        b0 = M.png_bytes_to_host()
        run(kind)
        to_host[kind] = M.png_bytes_to_host() - b0
    raster = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    ms = {'Dfix': [], 'Ddyn': [], 'Kfix': [], 'Kdyn': []}
    stream_bytes = {}
    for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
        ms['Dfix'].append(wall(lambda: run('fixed'), REPS))
        ms['Ddyn'].append(wall(lambda: run('dynamic'), REPS))
        k, stream_bytes['fixed'] = M.time_png_encode(raster.data_ptr(), N, N, reps=REPS)
        ms['Kfix'].append(k)
        k, stream_bytes['dynamic'] = M.time_png_encode(raster.data_ptr(), N, N, reps=REPS, codes=M.CODES_DYNAMIC)
        ms['Kdyn'].append(k)
    size = {k: os.path.getsize(p) for k, p in paths.items()}
    emit({'scene': name, 'size': N, 'backend': 'jit', 'rounds': ROUNDS, 'reps': REPS, 'band_rows_env': os.environ.get('MARAY_PNG_BAND_ROWS'),
          'host_file_bytes': size['host'], 'fixed_file_bytes': size['fixed'], 'dynamic_file_bytes': size['dynamic'],
          'dynamic_over_fixed_file': round(size['dynamic'] / size['fixed'], 3), 'dynamic_over_host_file': round(size['dynamic'] / size['host'], 2),
          'fixed_bytes_to_host': int(to_host['fixed']), 'dynamic_bytes_to_host': int(to_host['dynamic']),
          'fixed_stream_bytes': int(stream_bytes['fixed']), 'dynamic_stream_bytes': int(stream_bytes['dynamic']),
          'K_fixed_ms': round(med(ms['Kfix']), 4), 'K_dynamic_ms': round(med(ms['Kdyn']), 4),
          'K_dynamic_over_fixed': round(med(ms['Kdyn']) / med(ms['Kfix']), 2),
          'K_fixed_all_ms': [round(v, 4) for v in ms['Kfix']], 'K_dynamic_all_ms': [round(v, 4) for v in ms['Kdyn']],
          'D_fixed_ms': round(med(ms['Dfix']), 3), 'D_dynamic_ms': round(med(ms['Ddyn']), 3),
          'D_dynamic_over_fixed': round(med(ms['Ddyn']) / med(ms['Dfix']), 3),
          'D_fixed_all_ms': [round(v, 3) for v in ms['Dfix']], 'D_dynamic_all_ms': [round(v, 3) for v in ms['Ddyn']],
          'raster_bytes': raster.numel(), 'images_checked': True})
    M.gen_cache_clear()
    del raster

# ---- the nine-frame chess_slide animation -----------------------------------------------------------------------------------
import apng_stream as A  # noqa: E402

FRAMES, FROM, TO = 9, -200.0, 200.0
subprocess.check_call([os.path.join(ROOT, 'maray_amd', 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)
scene = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
if N != 1024:
    scene.rescale(N // 1024, N // 1024)
scene.declare_param('t', FROM, TO)
values = [TO if i == FRAMES - 1 else FROM + i * (TO - FROM) / (FRAMES - 1) for i in range(FRAMES)]
apng = {k: os.path.join(tmp, 'slide_%s.png' % k) for k in ('fixed', 'dynamic')}


def animate(kind):
    M.gen_animation(scene, apng[kind], {'t': values}, backend=M.BACKEND_JIT, n_devices=1,
                    codes=M.CODES_DYNAMIC if kind == 'dynamic' else M.CODES_FIXED)


to_host = {}
for kind in apng:
    animate(kind)
    b0 = M.png_bytes_to_host()
    animate(kind)
    to_host[kind] = M.png_bytes_to_host() - b0
ms = {'fixed': [], 'dynamic': []}
for _ in range(ROUNDS):
    for kind in ms:
        ms[kind].append(wall(lambda: animate(kind), 1))
checked = False
if N <= 1024:                               # (inflating 2 x 9 frames of 48 MiB is left to the tests' small sizes)
    a, b = A.decode(open(apng['fixed'], 'rb').read()), A.decode(open(apng['dynamic'], 'rb').read())
    assert a.rects == b.rects and all(np.array_equal(x, y) for x, y in zip(a.frames, b.frames))
    checked = True
size = {k: os.path.getsize(p) for k, p in apng.items()}
emit({'what': 'chess_slide nine-frame APNG, gen_animation in this process', 'size': N, 'frames': FRAMES, 'backend': 'jit', 'rounds': ROUNDS,
      'fixed_file_bytes': size['fixed'], 'dynamic_file_bytes': size['dynamic'], 'dynamic_over_fixed_file': round(size['dynamic'] / size['fixed'], 3),
      'fixed_ms': round(med(ms['fixed']), 2), 'dynamic_ms': round(med(ms['dynamic']), 2), 'dynamic_over_fixed_ms': round(med(ms['dynamic']) / med(ms['fixed']), 3),
      'fixed_all_ms': [round(v, 2) for v in ms['fixed']], 'dynamic_all_ms': [round(v, 2) for v in ms['dynamic']],
      'fixed_bytes_to_host': int(to_host['fixed']), 'dynamic_bytes_to_host': int(to_host['dynamic']), 'frames_compared': checked})
