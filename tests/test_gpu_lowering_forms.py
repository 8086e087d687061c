"""Every lowering form (lowering_forms.FORMS) and guards that read Y on the device: the three back-ends against the oracle,
RGB8 byte for byte and f64 planes bit for bit (NaN matching NaN), never with a tolerance.

When a guard's cone reads Y the specialised back-end bounds guards over rectangles of one row x 256 pixels, its launch
order ranks groups of one row, and the interpreters evaluate guards per row as y values.  The default lowering of the
suite's other scenes never takes that path; here `blinds` does under the default lowering, the polygon soup (every guard)
and the product soup (some guards: the mixed case) under y_spans=False.  tests/test_lowering_forms.py holds the condition
that makes these tests tell: the three scenes change when guards are taken from the first row of a group of 8 or 32 rows.

Images are 320 x 96: 1.25 tiles of 256 pixels (the last one ragged, five 64-pixel runs) by three 32-row groups.  Every test
body runs in a child process with a time limit of its own; nothing follows a failure inside one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lowering_forms as LF
import maray_amd as M
import tape_eval as TE
from marayb import encode
from oracle_ffi import Scene as OScene
from test_lowering import same_f64

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_JIT, M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM]
THREADS = min(16, os.cpu_count() or 1)
W, H = LF.GPU_SIZE
RANGES = [(0, H), (5, 77)]

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_lowering_forms as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout, env=None):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])


def _jit_contexts(cases):
    """The specialised contexts of several (tape, textures, samples), at most eight builds side by side (as tests/test_fuzz.py)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda c: M.Context(c[0], textures=c[1], backend=M.BACKEND_JIT, samples=c[2]), cases))


@functools.lru_cache(maxsize=None)
def oracle(data, w, h, textured=False):
    import scenes
    return OScene(data).render_rows(w, h, 0, h, scenes.textures(scale=64) if textured else None, threads=THREADS)


def compare(ctxs, w, h, ranges, want, what):
    """Every context of ctxs renders every range: equal to the rows of want = (rgb8, f64) of the whole image.  Closes them."""
    names = set()
    for ctx in ctxs:
        names.add(ctx.kernel_name)
        for y0, y1 in ranges:
            got8, got64 = ctx.render_rows(w, h, y0, y1)
            assert same_f64(got64, want[1][y0:y1]), (what, ctx.kernel_name, y0, y1)
            assert np.array_equal(got8, want[0][y0:y1]), (what, ctx.kernel_name, y0, y1)
        ctx.close()
    return names


def three_backends(tapes, textures=None, samples=0):
    """[[context per back-end] per tape]; textures: one list for all tapes or None."""
    jit = _jit_contexts([(t, textures, samples) for t in tapes])
    return [[j] + [M.Context(t, textures=textures, backend=b, samples=samples) for b in BACKENDS[1:]] for t, j in zip(tapes, jit)]


# ---- 1. every form on every back-end -----------------------------------------------------------------------------------------
def child_form(form):
    cases = []
    for name in LF.GPU_SCENES:
        data, t = LF.gpu_scene(name)
        s = M.Scene(data)
        tape = s.lower(**LF.FORMS[form])
        n_guards, n_read_y = LF.check_form(form, tape, s.lower())
        if name == 'blinds' and n_guards:
            assert n_read_y == n_guards                     # whatever the form: a band has no bound over y
        print('form', form, name, 'guards', n_guards, 'reading y', n_read_y)
        cases.append((name, data, tape, t))
    jit = _jit_contexts([(tape, t, 0) for _, _, tape, t in cases])
    names = set()
    for (name, data, tape, t), jctx in zip(cases, jit):
        ctxs = [jctx] + [M.Context(tape, textures=t, backend=b) for b in BACKENDS[1:]]
        names |= compare(ctxs, W, H, RANGES, oracle(data, W, H, t is not None), (form, name))
    print('kernels', sorted(names))


@pytest.mark.parametrize('form', list(LF.FORMS))
def test_form_on_every_back_end_equals_the_oracle(form):
    """One form of six scenes (three soups, a soup of coloured shapes, blinds, every kind of op on guarded masks with
    textures), each checked to be that form, on the three back-ends: rows 0..95 and the ragged 5..76, every pixel."""
    _run('child_form(%r)' % form, 600)


# ---- 2. the reads-Y path at launch geometries --------------------------------------------------------------------------------
_GEOMETRIES = r"""
import lowering_forms as LF
import tape_eval as TE
w, h = LF.GPU_SIZE
GEOMS = [('rows', 0, 96), ('rows', 0, 1), ('rows', 37, 38), ('rows', 95, 96), ('rows', 5, 77), ('rows', 31, 65),
         ('blocks', 3, 5, 16, 6), ('blocks', 0, 8, 32, 3), ('blocks', 10, 1, 7, 12), ('blocks', 1, 32, 33, 2)]
for name in LF.READS_Y:
    data, tape = LF.reads_y_tape(name)
    print(name, 'guards, reading y:', TE.guards_reading_y(tape))
    bare = M.Scene(data).lower(skips=False)
    assert bare.info['skip_ops'] == 0 and TE.guards_reading_y(bare)[0] == 0
    ora = Oracle(data, w, h)
    ref = M.Context(bare, backend=INTERP)
    want = {g: render(ref, w, h, g) for g in GEOMS}
    ref.close()
    for g in GEOMS:
        ora.check(want[g], g, [], f64_bands=[(0, 8), (30, 40), (60, 70), (88, 96)])
    assert T.jit_shape(tape)[1]                       # guard words, so a launch order: here of one-row groups
    for b in (JIT, M.BACKEND_TAPE, INTERP):
        ctx = M.Context(tape, backend=b)
        for g in GEOMS:
            for i in range(3):                        # the second launch computes the order, the third takes it from the cache
                assert same(render(ctx, w, h, g), want[g]), (name, ctx.kernel_name, g, i)
            assert same(render(ctx, w, h, g, f64=False), want[g]), (name, ctx.kernel_name, g, 'RGB8 only')
        for i, g in enumerate([GEOMS[0], GEOMS[4], GEOMS[0], GEOMS[4], GEOMS[6], GEOMS[0]]):      # orders evicted and computed again
            assert same(render(ctx, w, h, g), want[g]), (name, ctx.kernel_name, g, 'in turn', i)
        print('kernel', ctx.kernel_name)
        ctx.close()
print('geometries ok')
"""


def test_guards_that_read_y_at_launch_geometries():
    """The three reads-Y tapes at the whole image, single rows, ragged ranges and row blocks with block_stride > block_rows
    (block_rows = 1 too), each launched three times and then in turn, into buffers with guard bands: every byte and f64
    against the scalar-cache interpreter on the guard-free lowering (skips=False) of the same scene, that against the
    oracle on bands, the guard bands untouched."""
    from test_gpu_launches import _run as run_with_prelude
    run_with_prelude(_GEOMETRIES, 'geometries ok', 600)


_TALL = r"""
import lowering_forms as LF
import tape_eval as TE
w, h = 5, 65540
data = encode((w, h), LF.blinds(w, h))
tape = LF.blinds_tape(M.Scene(data))
print('guards, reading y:', TE.guards_reading_y(tape))
ora = Oracle(data, w, h)
g = ('rows', 0, h)
bands = [(0, 8), (65530, 65540)]
ref = M.Context(tape, backend=INTERP)
want = render(ref, w, h, g)
ref.close()
ora.check(want, g, [], f64_bands=bands)
assert float(want[0][65530:].float().std()) > 1.0            # (a picture at the far end)
for b in (JIT, M.BACKEND_TAPE):
    ctx = M.Context(tape, backend=b)
    for i in range(2):
        got = render(ctx, w, h, g)
        assert same(got, want), (ctx.kernel_name, i)
    ora.check(got, g, [], f64_bands=bands)
    print('kernel', ctx.kernel_name)
    ctx.close()
print('tall ok')
"""


def test_guards_that_read_y_on_65540_rows_in_one_launch():
    """blinds 5 pixels wide and 65,540 rows tall in one launch: with rectangles of one row the guard items of a launch
    are its rows, across the split into two grids (65,534 rows each at most).  Every byte against the interpreter; the oracle
    on the top rows and on rows 65,530..65,539, which lie on both sides of the split and of row 65,535 and end the image."""
    from test_gpu_launches import _run as run_with_prelude
    run_with_prelude(_TALL, 'tall ok', 600)


# ---- 3. supersampling -------------------------------------------------------------------------------------------------------
def child_supersampled(k):
    from test_gpu_supersample import SS_KERNELS, box
    w, h = LF.SS_SIZE
    made = [LF.ss_tape(name, k) for name in LF.READS_Y]
    names = set()
    for name, (s, tape), ctxs in zip(LF.READS_Y, made, three_backends([t for _, t in made], samples=k)):
        print(name, 'k', k, 'guards, reading y:', TE.guards_reading_y(tape))
        want8, _ = OScene(s.encode()).render_rows(w * k, h * k, 0, h * k, threads=THREADS, want_f64=False)
        want = box(want8, k)
        for ctx in ctxs:
            assert ctx.kernel_name.startswith(SS_KERNELS), ctx.kernel_name
            names.add(ctx.kernel_name)
            for y0, y1 in ((0, h), (5, 39)):
                got8, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
                assert np.array_equal(got8, want[y0:y1]), (name, k, ctx.kernel_name, y0)
            ctx.close()
    print('kernels', sorted(names))


@pytest.mark.parametrize('k', [2, 4, 8])
def test_supersampled_guards_that_read_y_equal_the_box_filter_of_the_oracle(k):
    """The three reads-Y tapes of the scenes supersampled k x k, 160 x 48 output pixels, the three back-ends with samples = k:
    the box filter of the oracle's render of the supersampled scene, every pixel."""
    _run('child_supersampled(%d)' % k, 600)


# ---- 4. deferred tiles ------------------------------------------------------------------------------------------------------
def child_deferred():
    from test_gpu_launches import tri_soup
    data = encode((W, H), tri_soup(1, [(0, W, 0, H, 16, 40)], W, H, huge_sin=True))
    s = M.Scene(data)
    default = s.lower()
    assert default.info['sin_ops'] > default.info['sin_bounded']          # Sin past the reduction range: tiles are deferred
    tapes = []
    for kw in (dict(fuse=False), dict(y_spans=False), dict(fuse=False, y_spans=False)):
        tape = s.lower(**kw)
        assert tape.info['sin_ops'] > tape.info['sin_bounded'], kw
        if 'fuse' in kw:
            LF.check_form('no_fuse', tape, default)
        if 'y_spans' in kw:
            LF.check_form('no_y_spans', tape, default)
        tapes.append(tape)
    names = set()
    for tape, ctxs in zip(tapes, three_backends(tapes)):
        names |= compare(ctxs, W, H, RANGES, oracle(data, W, H), 'deferred')
    print('kernels', sorted(names))


def test_deferred_tiles_unfused_and_with_guards_that_read_y():
    """Triangles half of which carry Step(Sin(x * 2^20 + y)): the specialised kernel defers the tiles whose Sin arguments are
    past its reduction range to the interpreter.  Unfused (a bare SIN, then STEP, must defer as STEPSIN does), with guards
    that read Y (the deferred tiles' guards come from the ROW kernel, bounded over the whole row), and both."""
    _run('child_deferred()', 600)


# ---- 5. parameters -----------------------------------------------------------------------------------------------------------
def child_params(kw_name):
    import test_gpu_fuzz_params as FP
    from fuzz_scenes import param_soup
    kw = dict(y_spans=dict(y_spans=False), shared=dict(private_regions=False))[kw_name]
    cases = []
    for family in (0, 1, 2):
        color, decl, vectors = param_soup(family, 800, (14, 12, 8)[family], W, H, n_vectors=3)
        cases.append(dict(name='soup %d' % family, color=color, decl=decl, vectors=vectors, size=(W, H), textures=None, narrow=False))

    def on_tape(c, scene, tape):
        LF.check_form('no_y_spans' if kw_name == 'y_spans' else 'shared', tape, scene.lower())
        print(c['name'], kw_name, 'guards, reading y:', TE.guards_reading_y(tape))
    FP.run_cases(cases, 3, lower_kw=kw, on_tape=on_tape)


@pytest.mark.parametrize('kw_name', ['y_spans', 'shared'])
def test_parameterised_soups_in_two_forms(kw_name):
    """One soup with parameters per family, lowered with y_spans=False (guards that read Y, bounded under parameter ranges)
    and with private_regions=False; three vectors of values launched 0, 1, 1, 2, 0 on one context per back-end, against the
    oracle's render of the scene with the values substituted."""
    _run('child_params(%r)' % kw_name, 600)


# ---- 6. knobs that must not matter -------------------------------------------------------------------------------------------
def child_knob(scene_name, form, backends):
    data, _ = LF.gpu_scene(scene_name)
    s = M.Scene(data)
    if scene_name == 'blinds':
        tape = LF.blinds_tape(s)
    else:
        tape = s.lower(**LF.FORMS[form])
        LF.check_form(form, tape, s.lower())
    ctxs = [M.Context(tape, backend=b) for b in backends]
    print('kernels', sorted(compare(ctxs, W, H, RANGES, oracle(data, W, H), (scene_name, form))))


KNOBS = [('blinds', 'default', dict(MARAY_JIT_GUARD_W='64', MARAY_JIT_GUARD_H='32'), [M.BACKEND_JIT]),
         ('blinds', 'default', dict(MARAY_JIT_MIN_REGION='0'), [M.BACKEND_JIT]),
         ('blinds', 'default', dict(MARAY_TAPE_GENERIC='1'), [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM]),
         ('polygons', 'shared', dict(MARAY_JIT_REDUCE='0'), [M.BACKEND_JIT]),
         ('polygons', 'no_rebalance', dict(MARAY_JIT_REDUCE='0'), [M.BACKEND_JIT])]


@pytest.mark.parametrize('scene_name,form,env,backends', KNOBS, ids=['guard_rectangle', 'min_region', 'tape_generic', 'reduce_shared', 'reduce_no_rebalance'])
def test_knobs_that_must_not_change_the_image(scene_name, form, env, backends):
    """With guards that read Y the guard rectangle is not the back-end's choice: MARAY_JIT_GUARD_W / _H must leave the image
    the oracle's; so must MARAY_JIT_MIN_REGION=0 and the interpreters' MARAY_TAPE_GENERIC=1 there, and MARAY_JIT_REDUCE=0 on
    the polygon soup lowered with shared regions and without rebalanced chains."""
    _run('child_knob(%r, %r, %r)' % (scene_name, form, backends), 600, env=env)


# ---- 7. the facade -----------------------------------------------------------------------------------------------------------
def child_facade():
    from test_gpu_supersample import box
    data, _ = LF.gpu_scene('blinds')
    LF.blinds_tape(M.Scene(data))
    s2 = M.Scene(data)
    s2.supersample(2)
    assert TE.guards_reading_y(LF.blinds_tape(s2))[1] > 0
    want2, _ = OScene(s2.encode()).render_rows(2 * W, 2 * H, 0, 2 * H, threads=THREADS, want_f64=False)
    wants = {1: oracle(data, W, H)[0], 2: box(want2, 2)}
    M.gen_cache_clear()
    try:
        s = M.Scene(data)
        for backend in (M.BACKEND_AUTO, M.BACKEND_JIT):      # (AUTO picks an interpreter for an image this small)
            for k in (1, 2, 1):
                assert np.array_equal(M.gen_to_image(s, backend=backend, samples=k, n_devices=2, tile_rows=16), wants[k]), (backend, k)
        print('cache', M.gen_cache_info())
        assert any(' kernel maray_jit_pixels_ss ' in line for line in M.gen_cache_info())
    finally:
        M.gen_cache_clear()


def test_gen_to_image_meets_guards_that_read_y():
    """gen_to_image lowers with the defaults: blinds is how it meets guards that read Y.  Two workers, tiles of 16 rows,
    samples 1 and 2, the back-end it picks itself and the specialised one, against the oracle and its box filter."""
    _run('child_facade()', 600, env=dict(MARAY_GEN_WRAP_DEVICES='1'))
