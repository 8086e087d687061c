#!/usr/bin/env python3
"""tools/exp_png_filter.py — what the device PNG encoder's row filters cost and save: chess rescaled to 4096^2
and the textured scene (config 5) at 4096^2, rendered once by the specialised kernels, one GPU, one process.  Per scene and for
png_filter in none / adaptive / up x codes in fixed / dynamic, alternating:
  E  png_encode_device of the raster in HBM: wall time per call (kernels, copies, the host's part) and the file's bytes;
  K  the encoder's kernels alone as bands of at most 2^28 filtered bytes (maray_hip_time_png_encode_opts, events).
     K(adaptive) - K(up) is what maray_png_filter_cost and maray_png_filter_pick take: `up` runs the filtered tokenisers
     without them,
each the median of ROUNDS rounds of REPS calls after one untimed call of each kind.  Every file is checked to decode to the
raster (the library's reader), and the fixed-code adaptive file is checked to be no larger than the filter-0 file.
--rounds N (default 5), --reps N (default 10), --size N (default 4096), --out FILE: the lines, appended."""
import json
import os
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
FILTERS = (('none', M.PNG_FILTER_NONE), ('adaptive', M.PNG_FILTER_ADAPTIVE), ('up', M.PNG_FILTER_UP))
CODES = (('fixed', M.CODES_FIXED), ('dynamic', M.CODES_DYNAMIC))
tmp = tempfile.mkdtemp(prefix='exp_png_filter_')


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


for name, make in (('chess', chess), ('textured (config 5)', textured)):
    scene, tex = make()
    want = M.gen_to_image(scene, textures=tex, backend=M.BACKEND_JIT, n_devices=1)
    raster = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    ptr = raster.data_ptr()
    k_rows = min(N, ((1 << 28) - 1) // (3 * N + 1))       # one band for both codes
    kinds = [(f, c) for f in FILTERS for c in CODES]
    sizes, ms_e, ms_k = {}, {}, {}
    for (fn, f), (cn, c) in kinds:                        # untimed: scratch grows, the files are checked
        png = M.png_encode_device(ptr, N, N, codes=c, png_filter=f)
        path = os.path.join(tmp, 'x.png')
        with open(path, 'wb') as fh:
            fh.write(png)
        assert np.array_equal(M.png_read(path), want), (name, fn, cn)
        sizes[fn, cn] = len(png)
        M.time_png_encode(ptr, N, k_rows, reps=1, codes=c, png_filter=f)
        ms_e[fn, cn], ms_k[fn, cn] = [], []
    assert sizes['adaptive', 'fixed'] <= sizes['none', 'fixed']
    for _ in range(ROUNDS):                               # alternating: every kind sees the same clocks and neighbours
        for (fn, f), (cn, c) in kinds:
            ms_e[fn, cn].append(wall(lambda: M.png_encode_device(ptr, N, N, codes=c, png_filter=f), REPS))
            ms_k[fn, cn].append(M.time_png_encode(ptr, N, k_rows, reps=REPS, codes=c, png_filter=f)[0])
    line = {'scene': name, 'size': N, 'rounds': ROUNDS, 'reps': REPS, 'kernel_rows': k_rows, 'raster_bytes': raster.numel()}
    for fn, cn in sizes:
        key = fn + '_' + cn
        line[key + '_file_bytes'] = sizes[fn, cn]
        line[key + '_encode_ms'] = round(float(np.median(ms_e[fn, cn])), 3)
        line[key + '_kernels_ms'] = round(float(np.median(ms_k[fn, cn])), 4)
        line[key + '_kernels_all_ms'] = [round(v, 4) for v in ms_k[fn, cn]]
    for cn, _ in CODES:
        line['adaptive_over_none_file_' + cn] = round(sizes['adaptive', cn] / sizes['none', cn], 4)
        line['cost_and_pick_ms_' + cn] = round(float(np.median(ms_k['adaptive', cn]) - np.median(ms_k['up', cn])), 4)
    line['images_checked'] = True
    emit(line)
    M.gen_cache_clear()
    del raster
