#!/usr/bin/env python3
"""tools/exp_png_indexed.py — what indexed colour buys and costs in the device PNG encoder: chess rescaled to
4096^2 and the textured scene (config 5) at 4096^2, specialised kernels, one GPU, one process.  Per scene and for the modes
truecolour with fixed codes (the default), truecolour with dynamic codes and png_color=PNG_COLOR_AUTO, alternating:
  F  the file's bytes;
  K  the encoder's kernels alone over the raster as one band (time_png_encode, events; AUTO: the colour kernels included);
  E  png_encode_device of the raster in HBM: wall time per call;
  R  Context.render_png: wall time per call, the render included,
each the median and the min .. max of ROUNDS rounds of REPS calls after one untimed call of each kind.  Every file is checked
to decode to the raster; where AUTO writes an indexed file it is checked to equal tests/png_indexed.py's model_file of the
rendered raster and to be smaller than the fixed-code truecolour file.
--rounds N (default 5), --reps N (default 5), --size N (default 4096), --out FILE: the lines, appended."""
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
import png_indexed as X  # noqa: E402
import scenes  # noqa: E402
from marayb import encode  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS, N = arg('--rounds', 5), arg('--reps', 5), arg('--size', 4096)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
MODES = (('rgb_fixed', dict()), ('rgb_dynamic', dict(codes=M.CODES_DYNAMIC)), ('auto', dict(png_color=M.PNG_COLOR_AUTO)))
tmp = tempfile.mkdtemp(prefix='exp_png_indexed_')


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


def spread(v):
    return {'median': round(float(np.median(v)), 3), 'min': round(float(min(v)), 3), 'max': round(float(max(v)), 3)}


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
    ctx = M.Context(scene.lower(), textures=tex, backend=M.BACKEND_JIT)
    n_colours, _ = M.png_palette(ptr, N, N)
    sizes, ms_k, ms_e, ms_r = {}, {}, {}, {}
    for mode, kw in MODES:                                    # untimed: kernels compiled, scratch grown, the files checked
        png = ctx.render_png(N, N, **kw)
        assert png == M.png_encode_device(ptr, N, N, **kw) or 'codes' in kw, (name, mode)
        path = os.path.join(tmp, 'x.png')
        with open(path, 'wb') as fh:
            fh.write(png)
        assert np.array_equal(M.png_read(path), want), (name, mode)
        sizes[mode] = len(png)
        M.time_png_encode(ptr, N, N, reps=1, **kw)
        ms_k[mode], ms_e[mode], ms_r[mode] = [], [], []
        if mode == 'auto' and n_colours <= 256:
            assert png == X.model_file(want), name
            assert len(png) < sizes['rgb_fixed'], name
        elif mode == 'auto':
            assert png == ctx.render_png(N, N), name
    for _ in range(ROUNDS):                                   # alternating: every mode sees the same clocks and neighbours
        for mode, kw in MODES:
            ms_k[mode].append(M.time_png_encode(ptr, N, N, reps=REPS, **kw)[0])
            ms_e[mode].append(wall(lambda: M.png_encode_device(ptr, N, N, **kw), REPS))
            ms_r[mode].append(wall(lambda: ctx.render_png(N, N, **kw), REPS))
    line = {'scene': name, 'size': N, 'rounds': ROUNDS, 'reps': REPS, 'colours': n_colours, 'indexed': n_colours <= 256,
            'raster_bytes': raster.numel(), 'files_checked': True}
    for mode, _ in MODES:
        line[mode + '_file_bytes'] = sizes[mode]
        line[mode + '_kernels_ms'] = spread(ms_k[mode])
        line[mode + '_encode_ms'] = spread(ms_e[mode])
        line[mode + '_render_png_ms'] = spread(ms_r[mode])
    emit(line)
    ctx.close()
    M.gen_cache_clear()
    del raster
