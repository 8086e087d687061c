#!/usr/bin/env python3
"""tools/exp_png.py — what writing the PNG costs with each encoder: chess rescaled to 4096^2 and the textured
scene (config 5) at 4096^2, specialised kernels, one GPU, one process.  Per scene, alternating:
  H  gen(scene, path) with the host writer (zlib level 6 on one thread): wall time per call;
  D  gen(scene, path, encoder=ENCODER_DEVICE): wall time per call;
  K  the encoder's three kernels alone on the rendered raster in HBM as one band (maray_hip_time_png_encode, events);
  F  hipMemsetAsync of the raster on a stream: the fill rate DESIGN measures kernels against,
each the median of ROUNDS rounds of REPS calls (H: HOST_REPS calls, it is seconds long), all after one untimed call of each
kind (the first gen of a scene lowers it and builds its kernels).  Also: the bytes the device encoders copied to the host per
call (maray_hip_png_bytes_to_host), the raster's bytes the host writer's path copies, both files' sizes, and that both files
decode to gen_to_image's raster.  One JSON line per scene.
--rounds N (default 5), --reps N (default 10), --host-reps N (default 2), --size N (default 4096), --out FILE: the lines, appended."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
import scenes  # noqa: E402
from marayb import encode  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS, HOST_REPS, SIZE = arg('--rounds', 5), arg('--reps', 10), arg('--host-reps', 2), arg('--size', 4096)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None


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


hip = C.CDLL('libamdhip64.so')
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
stream = torch.cuda.Stream()
N = SIZE
tmp = tempfile.mkdtemp(prefix='exp_png_')


def chess():
    s = M.Scene.open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'))
    if N != 1024:
        s.rescale(N // 1024, N // 1024)
    return s, None


def textured():
    return M.Scene(encode((N, N), scenes.textured(N))), scenes.textures(1)


for name, make in (('chess', chess), ('textured (config 5)', textured)):
    scene, tex = make()
    host_path, dev_path = os.path.join(tmp, 'host.png'), os.path.join(tmp, 'device.png')

    def run_h():
        M.gen(scene, host_path, textures=tex, backend=M.BACKEND_JIT, n_devices=1)

    def run_d():
        M.gen(scene, dev_path, textures=tex, backend=M.BACKEND_JIT, n_devices=1, encoder=M.ENCODER_DEVICE)

    run_h(); run_d()
    want = M.gen_to_image(scene, textures=tex, backend=M.BACKEND_JIT, n_devices=1)
    assert np.array_equal(M.png_read(host_path), want) and np.array_equal(M.png_read(dev_path), want)
    b0 = M.png_bytes_to_host()
    run_d()
    to_host = M.png_bytes_to_host() - b0
    raster = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    nbytes = raster.numel()

    def run_fill():
        hip.hipMemsetAsync(fill.data_ptr(), 0, nbytes, stream.cuda_stream)

    fill = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    ms = {'H': [], 'D': [], 'K': [], 'fill': []}
    stream_bytes = 0
    for _ in range(ROUNDS):                  # alternating: every kind sees the same clocks and neighbours
        ms['H'].append(wall(run_h, HOST_REPS))
        ms['D'].append(wall(run_d, REPS))
        k_ms, stream_bytes = M.time_png_encode(raster.data_ptr(), N, N, reps=REPS)
        ms['K'].append(k_ms)
        with torch.cuda.stream(stream):
            run_fill(); stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(REPS):
                run_fill()
            e1.record(stream)
            e1.synchronize()
            ms['fill'].append(e0.elapsed_time(e1) / REPS)
    med = {n: float(np.median(v)) for n, v in ms.items()}
    emit({'scene': name, 'size': N, 'backend': 'jit', 'rounds': ROUNDS, 'reps': REPS, 'host_reps': HOST_REPS,
          'band_rows_env': os.environ.get('MARAY_PNG_BAND_ROWS'),
          'H_gen_host_ms': round(med['H'], 3), 'D_gen_device_ms': round(med['D'], 3), 'H_over_D': round(med['H'] / med['D'], 2),
          'H_all_ms': [round(v, 3) for v in ms['H']], 'D_all_ms': [round(v, 3) for v in ms['D']],
          'K_kernels_ms': round(med['K'], 4), 'K_all_ms': [round(v, 4) for v in ms['K']],
          'K_raster_GBps': round(nbytes / (med['K'] * 1e-3) / 1e9, 1),
          'fill_ms': round(med['fill'], 4), 'fill_GBps': round(nbytes / (med['fill'] * 1e-3) / 1e9, 1),
          'K_over_fill': round(med['K'] / med['fill'], 2),
          'fill_source': 'hipMemsetAsync of the 3-byte raster on a stream, as bench.py --full measures it',
          'raster_bytes': nbytes, 'device_bytes_to_host': int(to_host), 'stream_bytes': int(stream_bytes),
          'host_file_bytes': os.path.getsize(host_path), 'device_file_bytes': os.path.getsize(dev_path),
          'device_over_host_file': round(os.path.getsize(dev_path) / os.path.getsize(host_path), 2),
          'images_checked': True})
    M.gen_cache_clear()
    del raster, fill
