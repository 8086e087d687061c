#!/usr/bin/env python3
"""tools/exp_census.py — what the census of guard bits (maray_jit_census) costs and saves, one GPU, one
process, MARAY_JIT_GUARD_CENSUS=0 against the default in alternation.  One JSON line each:

  frame     chess rescaled to 4096^2, per fresh context: the first launch of the geometry (ROW pass, second bounds, pixels), the
            second (census, apply, order, pixels), the mean of the 20 after that, the pixel kernel alone (time_rows), the leaf
            bits left in the device's words, those of them that are eligible (the census figure: tools/census_refine.py --exact
            counts the same on the CPU as `exact_bits`) and the set bits of any kind; `rasters_equal`: every launch's raster against the first knob-off one;
  shutter8  chess_fade (every channel times var t, a parameter only PIXEL ops read) at 4096^2, a shutter of 8 frames: the FIRST
            call of a fresh context -- one ROW pass, and with the knob on the census in front of its second frame -- the
            second call and the mean of five more.  What the census costs inside the shortest use that reuses a set at all.

--rounds N (default 3 fresh contexts of each kind), --out FILE: the lines, appended; --commit ID: recorded in every line."""
import json
import os
import sys

import numpy as np
import torch  # device buffers and events; imported before the library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
from marayb import decode, encode, mul, var  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROUNDS = int(arg('--rounds', 3))
OUT = arg('--out', None)
COMMIT = arg('--commit', None)
N = 4096


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, 'a') as f:
            f.write(line + '\n')


def context(tape, census):
    old = os.environ.get('MARAY_JIT_GUARD_CENSUS')
    os.environ['MARAY_JIT_GUARD_CENSUS'] = '1' if census else '0'       # read when the context is created
    try:
        return M.Context(tape, backend=M.BACKEND_JIT)
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_CENSUS']
        else:
            os.environ['MARAY_JIT_GUARD_CENSUS'] = old


def timed(fn, stream, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3        # us


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


stream = torch.cuda.Stream()
chess_bytes = open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read()
out = torch.zeros((N, N, 3), dtype=torch.uint8, device='cuda')
ref = None

scene = M.Scene(chess_bytes)
scene.rescale(N // 1024, N // 1024)
tape = scene.lower()
pos, n_words, gw, gh = tape.guard_layout()
leaf_mask = np.zeros(n_words, np.uint64)
for p in map(int, pos):
    if p >= 0:
        leaf_mask[p // 64] |= np.uint64(1) << np.uint64(p % 64)
with torch.cuda.stream(stream):
    for rnd in range(ROUNDS):
        for census in (False, True):
            ctx = context(tape, census)
            launch = lambda: ctx.render_rows_device(N, N, 0, N, d_rgb8=out.data_ptr(), stream=stream.cuda_stream)
            first = timed(launch, stream)
            same = True
            if ref is None:
                ref = out.clone()
            same &= bool(torch.equal(out, ref))
            second = timed(launch, stream)
            same &= bool(torch.equal(out, ref))
            later = timed(launch, stream, 20)
            same &= bool(torch.equal(out, ref))
            pix = ctx.time_rows(N, N, 0, N, d_rgb8=out.data_ptr(), reps=20) * 1e3
            words = ctx.debug_census_words()
            emit({'what': 'frame', 'scene': 'chess rescaled to %d^2' % N, 'census': census, 'round': rnd, 'commit': COMMIT, 'code_key': tape.jit_code_key,
                  'first_launch_us': round(first, 2), 'second_launch_us': round(second, 2), 'later_launch_us': round(later, 2), 'pixel_kernel_us': round(pix, 2),
                  'census_count': ctx.census_count, 'launch_counts': list(ctx.launch_counts), 'refine_count': ctx.refine_count,
                  'leaf_bits_left': popcount(words & leaf_mask[None, :]), 'eligible_leaf_bits_left': popcount(words & leaf_mask[None, :] & tape.census_eligible()[None, :]),
                  'bits_left': popcount(words), 'eligible_leaf_bits': popcount(tape.census_eligible()),
                  'rectangle': [gw, gh], 'rasters_equal': same})
            ctx.close()

size, color = decode(chess_bytes)[:2]
fade = M.Scene(encode(tuple(size), [mul(c, var('t')) for c in color]))
fade.declare_param('t', 0.0, 1.0)
fade.set_param('t', 0.5)
fade.set_param_span('t', 1.0)
fade.rescale(N // 1024, N // 1024)
ftape = fade.lower()
values = fade.shutter_values(8)
ref = None
with torch.cuda.stream(stream):
    for rnd in range(ROUNDS):
        for census in (False, True):
            ctx = context(ftape, census)
            call = lambda: ctx.render_rows_shutter_device(N, N, 0, N, values, out.data_ptr(), stream=stream.cuda_stream)
            first = timed(call, stream)
            if ref is None:
                ref = out.clone()
            same = bool(torch.equal(out, ref))
            second = timed(call, stream)
            same &= bool(torch.equal(out, ref))
            later = timed(call, stream, 5)
            emit({'what': 'shutter8', 'scene': 'chess_fade rescaled to %d^2' % N, 'census': census, 'round': rnd, 'commit': COMMIT, 'code_key': ftape.jit_code_key,
                  'row_params': ftape.info['row_params'], 'first_call_us': round(first, 2), 'second_call_us': round(second, 2), 'later_call_us': round(later, 2),
                  'eligible_leaf_bits': popcount(ftape.census_eligible()),
                  'census_count': ctx.census_count, 'launch_counts': list(ctx.launch_counts), 'images_equal': same})
            ctx.close()
