"""maray_jit_refine on the device, on the seeded scenes of tests/refine_fuzz_scenes.py: the guard words a launch
left against the numpy model (tests/refine_eval.py) bit for bit -- the device sine is glibc's, so there is no tolerance -- and every
raster against the oracle's render of the scene (values substituted: tests/params.py), RGB8 byte for byte and f64 planes bit for
bit, on a context created with MARAY_JIT_GUARD_REFINE=1 and on one created with 0.  tests/test_refine_fuzz.py holds the soundness
claim and the conditions that keep these cases from being empty.

Every test body runs in a child process with a time limit of its own; nothing follows a failure inside one.  A child prints one
line per scene, `refine-fuzz: kind seed geometry rectangles cleared`; the test prints them again."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
import refine_eval as RE
import refine_fuzz_scenes as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
%(first)s
import test_gpu_refine_fuzz as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout, torch_first=False):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call, first='import torch' if torch_first else '')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.split('\n') if ln.startswith('refine-fuzz:')]
    print('\n'.join(lines))
    return lines


def contexts(tapes, refine=True, samples=0, backend=M.BACKEND_JIT):
    """Contexts of several tapes, eight builds side by side (as tests/test_gpu_cover_fuzz.py), MARAY_JIT_GUARD_REFINE set around
    their creation (it is read when a context is created)."""
    from concurrent.futures import ThreadPoolExecutor
    old = os.environ.get('MARAY_JIT_GUARD_REFINE')
    os.environ['MARAY_JIT_GUARD_REFINE'] = '1' if refine else '0'
    try:
        with ThreadPoolExecutor(8) as pool:
            return list(pool.map(lambda t: M.Context(t, backend=backend, samples=samples), tapes))
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_REFINE']
        else:
            os.environ['MARAY_JIT_GUARD_REFINE'] = old


def oracle(made, values, want_f64=True):
    """The oracle's (rgb8, f64 planes) of the rows of the scene's geometry, the values substituted exactly."""
    from marayb import encode
    from oracle_ffi import Scene as OScene
    w, h, y0, y1 = made.geo
    color = made.color()
    if made.decl:
        color = PR.substituted_exact(color, [i for i, _, _ in made.decl], values)
    return OScene(encode((w, h), color)).render_rows(w, h, y0, y1, threads=min(16, os.cpu_count() or 1), want_f64=want_f64)


def model_words(tape, w, y0, rows, values=None, refined=True):
    pos, n_words, gw, gh = tape.guard_layout()
    geo, second, _ = RE.guard_bits(tape, w, y0, rows, gw, gh, params=values)
    return RE.pack_words(geo & second if refined else geo, pos, n_words)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def launch(ctx, geo, want, values, what):
    w, h, y0, y1 = geo
    if values is not None:
        ctx.set_params(list(values))
    got8, got64 = ctx.render_rows(w, h, y0, y1, want_f64=True)
    assert np.array_equal(got8, want[0]), (what, 'rgb8')
    assert PR.same_f64(got64, want[1]), (what, 'f64')
    return got8


def row_read(tape, values):
    """The values of the parameters a ROW op reads: what the ROW tables, and the pass behind them, are keyed by."""
    return None if values is None else tuple(v for p, v in enumerate(values) if (tape.info['row_params'] >> p) & 1)


# ---- a. words and rasters, kind by kind --------------------------------------------------------------------------------------
def plain_cases(kind):
    return [c for c in F.CASES if c[0] == kind and c[3] == 1]


BIG = ('rows', 7, F.G1100, 1)           # the blinds-like scene on 1100 x 200: 1000 rectangles of 256 x 1, four blocks of maray_jit_refine


def child_kind(kind):
    cases = plain_cases(kind)
    assert 0 < len(cases) <= 8
    made = [F.lowered(c) for c in cases]
    on = contexts([m[0] for m in made])
    off = contexts([m[0] for m in made], refine=False)
    control, = contexts([made[0][0]], backend=M.BACKEND_TAPE)
    for n, (case, (tape, md), a, b) in enumerate(zip(cases, made, on, off)):
        w, h, y0, y1 = geo = case[2]
        section = 1 if tape.jit_source_refine else 0
        assert section == (1 if tape.refine.n_outs else 0), case
        passes, before, n_cleared = 0, object(), []
        for vi, v in enumerate(md.vectors + md.vectors[:1] if md.decl else md.vectors):
            want = oracle(md, v)
            ra = launch(a, geo, want, v, (case, v, 'refine on'))
            rb = launch(b, geo, want, v, (case, v, 'refine off'))
            assert np.array_equal(ra, rb)
            if n == 0 and vi == 0:
                launch(control, geo, want, v, (case, v, 'the interpreter'))
            # the pass runs behind every ROW pass, and a ROW pass runs exactly when a ROW-read value changes
            passes += row_read(tape, v) != before
            before = row_read(tape, v)
            assert a.launch_counts[0] == b.launch_counts[0] == passes, (case, v, a.launch_counts, passes)
            assert (a.refine_count, b.refine_count) == (section * passes, 0), (case, v, a.refine_count, passes)
            got, plain = a.debug_guard_words(), b.debug_guard_words()
            assert same(plain, model_words(tape, w, y0, y1 - y0, v, refined=False)), (case, v, 'geometric words')
            assert same(got, model_words(tape, w, y0, y1 - y0, v)), (case, v, 'refined words')
            n_cleared.append(int(sum(bin(int(x)).count('1') for x in (plain & ~got).reshape(-1))))
        print('refine-fuzz: %s seed %d %dx%d rows %d-%d: %d rectangles of %d x %d, bits cleared %s, %d passes' %
              (case[:2] + geo + (got.shape[0],) + tuple(tape.guard_layout()[2:]) + (n_cleared if md.decl else n_cleared[0], a.refine_count)))
        if case == BIG:
            # one work-item per rectangle: more than two blocks of the pass, a partial one last
            assert got.shape[0] == F.refine_items(tape, case) > 2 * F.row_block() and got.shape[0] % F.row_block() and a.refine_count == 1, case
        a.close()
        b.close()
    control.close()


@pytest.mark.parametrize('kind', F.KINDS)
def test_words_and_rasters(kind):
    """The plain cases of a kind, one context with the pass and one without each, one interpreter context as a control: every
    launch's raster is the oracle's on both, the words are the model's (geo & second, and geo), refine_count is the count of ROW
    passes or 0.  A parameterised scene is launched under each of its vectors in turn and under the first again: a pass exactly
    when a ROW-read value changed.  The cases of 449 x 100 with rows 37 .. 92 are launched as that range.  `rows` holds the one
    case whose pass is more than two blocks (BIG); every other launch of this file is a single block."""
    assert (BIG in plain_cases(kind)) == (kind == 'rows')
    assert len(_run('child_kind(%r)' % kind, 600)) == len(plain_cases(kind))


# ---- b. supersampled ---------------------------------------------------------------------------------------------------------
def child_supersampled(k):
    from oracle_ffi import Scene as OScene
    from test_gpu_supersample import box
    cases = [c for c in F.CASES if c[3] == k]
    assert {c[0] for c in cases} == {'near3', 'edge', 'arith'}
    made = [F.lowered(c) for c in cases]
    on = contexts([m[0] for m in made], samples=k)
    off = contexts([m[0] for m in made], refine=False, samples=k)
    for case, (tape, md), a, b in zip(cases, made, on, off):
        w, h, y0, y1 = case[2]
        want = box(OScene(md.encoded).render_rows(k * w, k * h, k * y0, k * y1, threads=min(16, os.cpu_count() or 1), want_f64=False)[0], k)
        ra, rb = a.render_rows(w, h, y0, y1, want_f64=False)[0], b.render_rows(w, h, y0, y1, want_f64=False)[0]
        assert a.kernel_name == 'maray_jit_pixels_ss' and (a.refine_count, b.refine_count) == (1, 0), case
        assert np.array_equal(ra, rb), case
        assert np.array_equal(ra, want), case
        sw, sy0, srows = F.sample_geo(case)
        got, plain = a.debug_guard_words(), b.debug_guard_words()
        assert same(plain, model_words(tape, sw, sy0, srows, refined=False)), (case, 'geometric words')
        assert same(got, model_words(tape, sw, sy0, srows)), (case, 'refined words')
        print('refine-fuzz: %s seed %d %dx%d rows %d-%d k=%d: %d rectangles, %d bits cleared' %
              (case[:2] + case[2] + (k, got.shape[0], int(sum(bin(int(x)).count('1') for x in (plain & ~got).reshape(-1))))))
        a.close()
        b.close()


@pytest.mark.parametrize('k', [2, 4])
def test_supersampled(k):
    """near3, edge and arith at samples = k: the sections cover the k w x k h sample grid; the raster is the box filter of the
    oracle's k-times render, with the pass and without, and the words are the model's on that grid."""
    assert len(_run('child_supersampled(%d)' % k, 600)) == 3


# ---- c. blocks a stride apart ------------------------------------------------------------------------------------------------
BLOCK_ROWS, BLOCK_STRIDE, N_BLOCKS, BLOCK_Y0 = 32, 64, 2, 2
BLOCK_CASES = [('near3', 27, F.G449, 1), ('edge', 1, F.G449, 1), ('rows', 3, F.G449, 1)]


def child_blocks():
    import torch
    for case in BLOCK_CASES:
        assert case in F.CASES
        tape, md = F.lowered(case)
        w, h = case[2][:2]
        whole = oracle(md, None, want_f64=False)[0]
        pick = (BLOCK_Y0 + np.arange(N_BLOCKS)[:, None] * BLOCK_STRIDE + np.arange(BLOCK_ROWS)[None, :]).reshape(-1)
        assert pick.max() < h
        # a group of rows never straddles two blocks: the launch's words are the blocks' words one after the other
        per = lambda refined: np.concatenate([model_words(tape, w, BLOCK_Y0 + k * BLOCK_STRIDE, BLOCK_ROWS, refined=refined) for k in range(N_BLOCKS)])
        outs = []
        for refine in (True, False):
            ctx, = contexts([tape], refine=refine)
            d = torch.zeros((N_BLOCKS * BLOCK_ROWS, w, 3), dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            ctx.render_blocks_device(w, h, BLOCK_Y0, BLOCK_ROWS, BLOCK_STRIDE, N_BLOCKS, d_rgb8=d.data_ptr())
            torch.cuda.synchronize()
            outs.append(d.cpu().numpy())
            assert ctx.refine_count == (1 if refine else 0), case
            words = ctx.debug_guard_words()
            assert same(words, per(refine)), (case, refine)
            ctx.close()
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], whole[pick]), case
        print('refine-fuzz: %s seed %d %dx%d blocks of %d rows %d apart from row %d: %d rectangles, %d bits cleared' %
              (case[:2] + (w, h, BLOCK_ROWS, BLOCK_STRIDE, BLOCK_Y0, words.shape[0], int(sum(bin(int(x)).count('1') for x in (per(False) & ~per(True)).reshape(-1))))))


def test_blocks_with_a_stride():
    """render_blocks_device with two blocks of 32 rows 64 apart from row 2, a near3 and an edge scene (rectangles of 64 x 32) and the
    blinds-like scene (256 x 1): those rows of the oracle's whole frame, and the model's words block after block.  A process
    of its own with PyTorch imported first: the device buffer is PyTorch's."""
    assert len(_run('child_blocks()', 600, torch_first=True)) == len(BLOCK_CASES)
