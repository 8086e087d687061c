"""Parameter fuzz on the device: the generators of tests/test_fuzz_params.py (random scenes and soups with parameters planted,
ranges with every kind of end, values from the ends, the zeros and the specials) through the three back-ends, ONE context
per scene and back-end, every vector of values a launch on it; then every parameter slot from 1 to 64 parameters, more
frames in flight than the values' ring has slots, and render_tiles.  Everything against the oracle's render of the scene
with the values substituted (tests/params.py), RGB8 byte for byte and f64 planes bit for bit, NaN matching NaN.

Every test body runs in a child process with a time limit of its own; nothing follows a failure inside one."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
from fuzz_scenes import PARAM_ID0

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_JIT, M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM]
SIZE = (384, 320)        # 6 runs of 64 pixels, 10 groups of 32 rows
INF, NAN = math.inf, math.nan

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
%(first)s
import test_gpu_fuzz_params as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout, torch_first=False):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call, first='import torch' if torch_first else '')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])


def _jit_contexts(cases):
    """The specialised contexts of several scenes, eight builds side by side (as tests/test_fuzz.py)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda c: M.Context(c[0], textures=c[1], backend=M.BACKEND_JIT, samples=c[2]), cases))


def _launch_order(n):
    """v0, v1, v1 again (its values unchanged: the launch that computes the cached order), v2, ..., then v0 again."""
    return [0, 1, 1] + list(range(2, n)) + [0]


def run_cases(cases, min_cases, lower_kw=None, on_tape=None):
    """cases: dicts(name, color, decl, vectors, size, textures, narrow).  Lowered once each (lower_kw: keywords of
    Scene.lower, the defaults if None; on_tape(case, scene, tape): a check of what was lowered); per back-end one context, the
    vectors launched in _launch_order; narrow: every launch once more with the f64 planes off (the four-pixels-per-lane path
    where the program is small enough)."""
    from marayb import encode
    live = []
    for c in cases:
        scene = PR.declared_ids(encode(c['size'], c['color']), c['decl'])
        try:
            live.append((c, scene.lower(**(lower_kw or {}))))
            if on_tape:
                on_tape(c, scene, live[-1][1])
        except M.MarayError as e:
            if e.code not in (-4, -5):          # aliased ids / self reference: the reference itself is ill-defined there
                raise
    assert len(live) >= min_cases, len(live)
    jit = _jit_contexts([(tape, c['textures'], 0) for c, tape in live])
    n_v3 = 0
    for (c, tape), jctx in zip(live, jit):
        (w, h), ids, vectors = c['size'], [i for i, _, _ in c['decl']], c['vectors']
        n_v3 += tape.param_count > 0
        want = {}
        for b in BACKENDS:
            ctx = jctx if b == M.BACKEND_JIT else M.Context(tape, textures=c['textures'], backend=b)
            assert ctx.param_count == tape.param_count
            prev = None
            for k in _launch_order(len(vectors)):
                if k not in want:
                    want[k] = oracle(c['color'], ids, vectors[k], c['size'], c['textures'])
                if tape.param_count and k != prev:
                    ctx.set_params(list(vectors[k]))
                prev = k
                got8, got64 = ctx.render_rows(w, h, 0, h)
                assert np.array_equal(got8, want[k][0]), (c['name'], vectors[k], ctx.kernel_name)
                assert PR.same_f64(got64, want[k][1]), (c['name'], vectors[k], ctx.kernel_name)
                if c['narrow']:
                    got8, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
                    assert np.array_equal(got8, want[k][0]), (c['name'], vectors[k], ctx.kernel_name, 'no f64 planes')
            ctx.close()
    assert n_v3 >= 0.8 * len(live), (n_v3, len(live))


def oracle(color, ids, values, size, textures=None, want_f64=True):
    from marayb import encode
    from oracle_ffi import Scene as OScene
    w, h = size
    return OScene(encode(size, PR.substituted_exact(color, ids, values))).render_rows(w, h, 0, h, textures, threads=min(16, os.cpu_count() or 1),
                                                                                       want_f64=want_f64)


# ---- 1. random scenes and soups ----------------------------------------------------------------------------------------------
def child_random_scenes():
    import scenes
    from fuzz_scenes import param_scene
    tex = scenes.textures(scale=64)
    cases = []
    for k, seed in enumerate(list(range(1000, 1028)) + list(range(6000, 6012))):
        n_tex = 2 if seed % 3 == 0 else 0
        color, decl, vectors = param_scene(seed, n_tex, n_vectors=4)
        cases.append(dict(name='scene %d' % seed, color=color, decl=decl, vectors=vectors, size=(83, 9) if seed < 6000 else (200, 70),
                          textures=tex if n_tex else None, narrow=k % 3 == 0))
    run_cases(cases, 36)


def test_random_parameterised_scenes_gpu_vs_oracle():
    """28 random scenes at 83 x 9 and 12 at 200 x 70, four vectors each, the three back-ends; a third of them with the f64
    planes off as well."""
    _run('child_random_scenes()', 1200)


def soup_cases(size, seeds=(800, 801, 802), n_vectors=3):
    from fuzz_scenes import param_soup
    w, h = size
    cases = []
    for family in (0, 1, 2):
        for seed in seeds:
            color, decl, vectors = param_soup(family, seed, (40, 30, 16)[family], w, h, n_vectors=n_vectors)
            cases.append(dict(name='soup %d %d' % (family, seed), color=color, decl=decl, vectors=vectors, size=size, textures=None,
                              narrow=seed % 3 == 0))
    return cases


def child_soups():
    run_cases(soup_cases(SIZE), 9)


def test_parameterised_soups_gpu_vs_oracle():
    """Nine soups (three of each family) at 384 x 320: shapes that parameters move and scale cross 64-pixel and 32-row
    borders, so the rectangle guards of the specialised kernels decide under parameter ranges."""
    _run('child_soups()', 1200)


def child_supersampled_soups():
    from marayb import encode
    from oracle_ffi import Scene as OScene
    from test_gpu_supersample import box
    w, h = 192, 160
    cases = [c for c in soup_cases((w, h), seeds=(810,), n_vectors=2)]
    assert len(cases) == 3
    scenes_, tapes = [], []
    for c in cases:
        s = PR.declared_ids(encode((w, h), c['color']), c['decl'])
        s.supersample(2)
        scenes_.append(s)
        tapes.append(s.lower())
    jit = _jit_contexts([(t, None, 2) for t in tapes])
    for c, tape, jctx in zip(cases, tapes, jit):
        ids = [i for i, _, _ in c['decl']]
        assert tape.param_count >= 3
        wants = []
        for values in c['vectors']:
            plain = M.Scene(encode((w, h), PR.substituted_exact(c['color'], ids, values)))
            plain.supersample(2)
            want8, _ = OScene(plain.encode()).render_rows(2 * w, 2 * h, 0, 2 * h, threads=min(16, os.cpu_count() or 1), want_f64=False)
            wants.append(box(want8, 2))
        for b in BACKENDS:
            ctx = jctx if b == M.BACKEND_JIT else M.Context(tape, backend=b, samples=2)
            for k in (0, 1, 1, 0):
                ctx.set_params(list(c['vectors'][k]))
                got8, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
                assert np.array_equal(got8, wants[k]), (c['name'], c['vectors'][k], ctx.kernel_name)
            ctx.close()


def test_supersampled_parameterised_soups_gpu_vs_oracle():
    """Three soups with samples = 2: the box filter of the oracle's 2w x 2h render of the substituted, supersampled scene."""
    _run('child_supersampled_soups()', 1200)


# ---- 2. every parameter slot -----------------------------------------------------------------------------------------------------
SLOT_COUNTS = (1, 2, 3, 4, 5, 8, 16, 17, 33, 63, 64)


def slot_scene(n):
    """r = sum_k p_k [x == k], g = sum_k p_k [y == k] (ROW work), b = p_(n-1) + x: a value read through the wrong slot moves
    a known column, row or the whole blue plane."""
    from edge_values import is_
    from marayb import add, mul, var_id, x, y
    ids = [PARAM_ID0 + k for k in range(n)]
    r = g = None
    for k, i in enumerate(ids):
        tr, tg = mul(var_id(i), is_(x(), k)), mul(var_id(i), is_(y(), k))
        r, g = (tr, tg) if r is None else (add(r, tr), add(g, tg))
    return [r, g, add(var_id(ids[-1]), x())], [(i, -INF, INF) for i in ids]




def slot_vectors(n):
    """Distinct, exact values; the second vector with -0.0, +inf, -inf and NaN in slots n - 1, 0, n // 2 and n // 3 (whichever
    of them are free, in that order)."""
    a = [1000.5 + 3.0 * k for k in range(n)]
    b = [-(0.25 + 7.0 * k) for k in range(n)]
    taken = set()
    for slot, v in ((n - 1, -0.0), (0, INF), (n // 2, -INF), (n // 3, NAN)):
        if slot not in taken:
            b[slot] = v
            taken.add(slot)
    return [tuple(a), tuple(b)]


def child_slots():
    from marayb import encode
    size = (72, 70)
    made = []
    for n in SLOT_COUNTS:
        color, decl = slot_scene(n)
        tape = PR.declared_ids(encode(size, color), decl).lower()
        assert tape.program.version == 3 and tape.param_count == n
        made.append((n, color, decl, tape))
    jit = _jit_contexts([(tape, None, 0) for _, _, _, tape in made])
    w, h = size
    for (n, color, decl, tape), jctx in zip(made, jit):
        ids = [i for i, _, _ in decl]
        vectors = slot_vectors(n)
        wants = [oracle(color, ids, v, size) for v in vectors]
        assert wants[0][1][0, n - 1, 0] == vectors[0][n - 1] and wants[0][1][n - 1, 3, 1] == vectors[0][n - 1]      # the scene is what it says
        assert wants[0][1][2, 5, 2] == vectors[0][n - 1] + 5.0
        for b in BACKENDS:
            ctx = jctx if b == M.BACKEND_JIT else M.Context(tape, backend=b)
            for k in (0, 1, 0):
                ctx.set_params(list(vectors[k]))
                got8, got64 = ctx.render_rows(w, h, 0, h)
                assert PR.same_f64(got64, wants[k][1]), (n, k, ctx.kernel_name)
                assert np.array_equal(got8, wants[k][0]), (n, k, ctx.kernel_name)
            ctx.close()


def test_every_parameter_slot_from_1_to_64_parameters():
    _run('child_slots()', 1200)


# ---- 3. more frames in flight than the ring of values has slots ----------------------------------------------------------------
FRAMES_IN_FLIGHT = 20         # ParamRing::SLOTS (jit_backend / hip_backend) is 8


def child_frames_in_flight():
    import torch
    w, h = SIZE
    spec = PR.SCENES['slide'](w, h)
    scene, names = PR.declared(spec, SIZE)
    tape = scene.lower()
    values = [(-200.0 + 21.5 * k, 100.0 - 9.25 * k) for k in range(FRAMES_IN_FLIGHT)]
    wants = [PR.oracle_frame(spec, SIZE, v) for v in values]
    assert len({w8.tobytes() for w8, _ in wants}) == FRAMES_IN_FLIGHT
    for backend in BACKENDS:
        ctx = M.Context(tape, backend=backend)
        st = torch.cuda.Stream()
        out8 = [torch.zeros((h, w, 3), dtype=torch.uint8, device='cuda') for _ in values]
        out64 = [torch.zeros((h, w, 3), dtype=torch.float64, device='cuda') for _ in values]
        torch.cuda.synchronize()
        for v, o8, o64 in zip(values, out8, out64):
            ctx.set_params(list(v))
            ctx.render_rows_device(w, h, 0, h, d_rgb8=o8.data_ptr(), d_rgb64=o64.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        for k, (o8, o64) in enumerate(zip(out8, out64)):
            assert np.array_equal(o8.cpu().numpy(), wants[k][0]), (backend, k, values[k])
            assert PR.same_f64(o64.cpu().numpy(), wants[k][1]), (backend, k, values[k])
        ctx.close()


def test_twenty_frames_in_flight_keep_their_values():
    """20 render_rows_device launches of `slide` on one stream, each with its own values and output buffers, one synchronise
    at the end: every frame is the oracle's frame of its values (device buffers from PyTorch, imported first)."""
    _run('child_frames_in_flight()', 900, torch_first=True)


# ---- 4. render_tiles -----------------------------------------------------------------------------------------------------------
def child_render_tiles():
    w, h = SIZE
    spec = PR.SCENES['slide'](w, h)
    scene, names = PR.declared(spec, SIZE)
    tape = scene.lower()
    tiles = [(100, 151), (0, 100), (151, h)]            # ragged, out of order
    for backend in BACKENDS:
        ctx = M.Context(tape, backend=backend)
        for values in ((100.0, 70.0), (-37.5, 12.75), (100.0, 70.0)):
            ctx.set_params(list(values))
            image = np.full((h, w, 3), 9, np.uint8)
            done = []
            ctx.render_tiles(w, h, tiles, image, on_tile=lambda a, b: done.append((a, b)))
            assert done == tiles
            assert np.array_equal(image, PR.oracle_frame(spec, SIZE, values, want_f64=False)[0]), (backend, values)
        ctx.close()


def test_render_tiles_with_parameters():
    """The multi-device worker's entry point on one device, two vectors of values."""
    _run('child_render_tiles()', 900)
