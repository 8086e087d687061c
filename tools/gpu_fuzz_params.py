#!/usr/bin/env python3
"""tools/gpu_fuzz_params.py [--cpu] [--soups] LO HI [W H] — wider sweep of the parameter fuzz of tests/test_fuzz_params.py and
tests/test_gpu_fuzz_params.py: random scenes (or, with --soups, soups: seed s is family s % 3) with parameters planted,
lowered once, every vector of values against the oracle's render of the substituted scene, f64 planes bit for bit and RGB8
byte for byte.  Default: on the GPU, one context per scene and back-end, the vectors launched in sequence (one of them twice,
the first again at the end).  --cpu: the numpy tape evaluator instead (plain, skips per wavefront, per span, per rectangle;
the guard-free lowering; lowering again with the values set) -- needs no GPU.  Prints progress; exits non-zero on a mismatch."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np
import maray_amd as M
import params as PR
import scenes
import tape_eval
from fuzz_scenes import param_scene, param_soup
from marayb import encode

args = [a for a in sys.argv[1:] if not a.startswith('--')]
cpu, soups = '--cpu' in sys.argv, '--soups' in sys.argv
lo, hi = int(args[0]), int(args[1])
W, H = (int(args[2]), int(args[3])) if len(args) > 3 else ((256, 64) if soups else (83, 9))
tex = scenes.textures(scale=64)
done = aliased = too_large = v3 = differ = guarded = no_y = bad = 0
t0 = time.time()


def on_gpu(seed, color, decl, vectors, t):
    """The number of mismatching (back-end, launch) pairs, or None for a scene the library refuses as aliased."""
    from test_gpu_fuzz_params import _launch_order, oracle
    global v3, guarded, no_y, differ
    try:
        tape = PR.declared_ids(encode((W, H), color), decl).lower()
    except M.MarayError as e:
        if e.code in (-4, -5, -7):            # aliased / self-referent / too large for the tape format
            return None
        raise
    ids = [i for i, _, _ in decl]
    v3 += tape.program.version == 3
    n_guards, reading_y = tape_eval.guards_reading_y(tape)
    guarded += n_guards > 0
    no_y += n_guards > 0 and reading_y == 0
    want, n_bad = {}, 0
    for b in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE):
        ctx = M.Context(tape, textures=t, backend=b)
        prev = None
        for k in _launch_order(len(vectors)):
            if k not in want:
                want[k] = oracle(color, ids, vectors[k], (W, H), t)
            if tape.param_count and k != prev:
                ctx.set_params(list(vectors[k]))
            prev = k
            got8, got64 = ctx.render_rows(W, H, 0, H)
            if not (PR.same_f64(got64, want[k][1]) and np.array_equal(got8, want[k][0])):
                n_bad += 1
                print('MISMATCH seed %d backend %d values %r' % (seed, b, vectors[k]), flush=True)
        ctx.close()
    differ += any(not PR.same_f64(want[0][1], f) for _, f in want.values())
    return n_bad


for seed in range(lo, hi):
    if soups:
        family = seed % 3
        color, decl, vectors = param_soup(family, seed, (24, 24, 12)[family], W, H)
        t = None
    else:
        n_tex = 2 if seed % 3 == 0 else 0
        color, decl, vectors = param_scene(seed, n_tex)
        t = tex if n_tex else None
    if cpu:
        try:
            r = PR.fuzz_check(color, decl, vectors, (W, H), t)
        except M.MarayError as e:
            if e.code != -7:                  # MARAY_E_LIMIT: a scene too large for the tape format is no finding
                raise
            too_large += 1
            continue
        n_bad = None if r is None else len(r['failures'])
        if r is not None:
            v3 += r['version'] == 3
            differ += r['differ']
            guarded += r['guards'] > 0
            no_y += r['guards'] > 0 and r['reading_y'] == 0
            for values, what in r['failures']:
                print('MISMATCH seed %d %s values %r ranges %r' % (seed, what, values, [d[1:] for d in decl]), flush=True)
    else:
        n_bad = on_gpu(seed, color, decl, vectors, t)
    done += 1
    if n_bad is None:
        aliased += 1
    else:
        bad += n_bad
    if done % 50 == 0:
        print('%d scenes, %d mismatches, %.0f s' % (done, bad, time.time() - t0), flush=True)
print('done: seeds %d..%d at %d x %d (%s, %s): %d scenes, %d refused as aliased, %d as too large, %d version 3, %d with guards%s, %d mismatches, %.0f s'
      % (lo, hi - 1, W, H, 'soups' if soups else 'random scenes', 'numpy evaluator' if cpu else 'three back-ends', done + too_large, aliased, too_large, v3, guarded,
         ' (%d with none reading y), %d with frames that differ' % (no_y, differ), bad, time.time() - t0))
sys.exit(1 if bad else 0)
