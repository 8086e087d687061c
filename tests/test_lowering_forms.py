"""Every form maray_lower can emit (lowering_forms.FORMS), and guards that read Y, against the oracle on the CPU: the tape
under the numpy evaluator (tests/tape_eval.py), plain and with the SKIP ops taken per wavefront, per span and -- where no guard
reads Y -- per rectangle of rows.  f64 planes bit for bit (NaN matching NaN), RGB8 byte for byte.  Then the condition that
makes the device tests of tests/test_gpu_lowering_forms.py mean something (their scenes change under stale guards), and the
offline builds of everything those tests compile."""
import ctypes as C
import os

import numpy as np
import pytest

import lowering_forms as LF
import maray_amd as M
import params as PR
import scenes
import tape_eval as TE
from fuzz_scenes import curved_soup, param_soup, polygon_soup, product_soup
from marayb import encode
from oracle_ffi import Scene as OScene
from test_lowering import same_f64

THREADS = min(16, os.cpu_count() or 1)
SMALL = (192, 48)


def check_tapes(tapes, w, h, rows, want, textures=None):
    """tapes: {form: tape or TapeV2}; want: {(y0, y1): (rgb8, f64)} from the oracle.  Returns how many renders it compared."""
    n = 0
    for form, tape in tapes.items():
        n_guards, n_read_y = TE.guards_reading_y(tape)
        geometries = [dict(tile=None), dict(tile=64), dict(tile=256)]
        if n_guards and not n_read_y:
            geometries += [dict(tile=64, yrows=8), dict(tile=64, yrows=32)]
        for y0, y1 in rows:
            want8, want64 = want[(y0, y1)]
            got = TE.render_rows(tape, w, y0, y1, textures)
            assert same_f64(got, want64), (form, 'plain', y0)
            assert np.array_equal(TE.cast_u8(got), want8), (form, 'plain', y0)
            for kw in geometries:
                got = TE.render_rows_waves(tape, w, y0, y1, textures, **kw)
                assert same_f64(got, want64), (form, kw, y0)
                assert np.array_equal(TE.cast_u8(got), want8), (form, kw, y0)
            n += 1 + len(geometries)
    return n


def _soup(name):
    w, h = SMALL
    return {'polygons': lambda: polygon_soup(2, 20, w, h, mixed=False), 'curved': lambda: curved_soup(301, 16, w, h, mixed=True),
            'products': lambda: product_soup(500, 10, w, h), 'colours': lambda: polygon_soup(3, 14, w, h, mixed='colours')}[name]()


@pytest.mark.parametrize('name', ['polygons', 'curved', 'products', 'colours'])
def test_soups_in_every_form_equal_the_oracle(name):
    w, h = SMALL
    data = encode(SMALL, _soup(name))
    tapes = LF.lowered_forms(M.Scene(data))
    n_guards, n_read_y = TE.guards_reading_y(tapes['no_y_spans'])
    assert n_guards >= 6 and n_read_y > 0
    if name == 'products':                        # the mixed case: guards that read Y next to guards that hold for a rectangle
        assert 0 < n_read_y < n_guards, (n_guards, n_read_y)
    want = {(0, h): OScene(data).render_rows(w, h, 0, h, threads=THREADS)}
    assert check_tapes(tapes, w, h, [(0, h)], want) >= 4 * len(LF.FORMS)


RANDOM_SEEDS = (100, 101, 102, 103, 104, 1145)


def test_random_scenes_in_every_form_equal_the_oracle():
    """Six random scenes whose default lowering has guards.  A scene the library refuses as aliased or self-referent (the
    reference itself is ill-defined there) is dropped; at most one may go that way."""
    from test_fuzz import lowered
    w, h = SMALL
    tex = scenes.textures(scale=64)
    done = 0
    for seed in RANDOM_SEEDS:
        n_tex = 2 if seed % 3 == 0 else 0
        data, tape = lowered(seed, n_tex, w, h)
        if tape is None:
            continue
        assert TE.guards_reading_y(tape)[0] > 0, seed
        t = tex if n_tex else None
        want = {(0, h): OScene(data).render_rows(w, h, 0, h, t, threads=THREADS)}
        check_tapes(LF.lowered_forms(M.Scene(data)), w, h, [(0, h)], want, t)
        done += 1
    assert done >= len(RANDOM_SEEDS) - 1


def test_blinds_in_every_form_equal_the_oracle():
    w, h = 320, 96
    data = encode((w, h), LF.blinds(w, h))
    s = M.Scene(data)
    assert TE.guards_reading_y(LF.blinds_tape(s)) == (9, 9)
    s2 = M.Scene(encode((700, 100), LF.blinds(700, 100)))
    assert TE.guards_reading_y(LF.blinds_tape(s2)) == (9, 9)
    want = {(0, h): OScene(data).render_rows(w, h, 0, h, threads=THREADS)}
    check_tapes(LF.lowered_forms(s), w, h, [(0, h)], want)


def test_ops_on_a_guarded_mask_in_every_form_equal_the_oracle():
    w, h = 160, 48
    tex = scenes.textures(scale=64)
    data = encode((w, h), scenes.ops_on_a_guarded_mask(w, h))
    tapes = LF.lowered_forms(M.Scene(data))
    assert TE.guards_reading_y(tapes['default'])[0] >= 3
    want = {(0, h): OScene(data).render_rows(w, h, 0, h, tex, threads=THREADS)}
    check_tapes(tapes, w, h, [(0, h)], want, tex)


@pytest.mark.parametrize('family', [0, 1, 2])
def test_parameterised_soups_in_every_form_equal_the_oracle(family):
    """One soup per family with parameters planted, two vectors of values: each form lowered once, evaluated with the values
    as constants (params.as_v2), against the oracle's render of the scene with the values substituted."""
    w, h = SMALL
    color, decl, vectors = param_soup(family, 700, (14, 12, 8)[family], w, h, n_vectors=2)
    ids = [i for i, _, _ in decl]
    tapes = LF.lowered_forms(PR.declared_ids(encode(SMALL, color), decl))
    assert tapes['default'].param_count >= 3
    frames = []
    for values in vectors:
        want = {(0, h): OScene(encode(SMALL, PR.substituted_exact(color, ids, values))).render_rows(w, h, 0, h, threads=THREADS)}
        frames.append(want[(0, h)][1])
        check_tapes({f: PR.as_v2(t, values) if t.param_count else t for f, t in tapes.items()}, w, h, [(0, h)], want)
    assert not same_f64(frames[0], frames[1])


CHESS_ROWS = [(511, 513), (600, 601), (704, 705)]


def test_chess_rows_in_every_form_equal_the_oracle(chess_bytes):
    tapes = LF.lowered_forms(M.Scene(chess_bytes))
    o = OScene(chess_bytes)
    want = {r: o.render_rows(1024, 1024, r[0], r[1], threads=THREADS) for r in CHESS_ROWS}
    check_tapes(tapes, 1024, 1024, CHESS_ROWS, want)


def test_plain_cse_is_not_ignored():
    """check_form has nothing to hold plain_cse to on one scene (on some it changes nothing): over the scenes of this file it
    must change at least one tape."""
    changed = 0
    for name in ('polygons', 'curved', 'products', 'colours'):
        s = M.Scene(encode(SMALL, _soup(name)))
        changed += [a.tobytes() for a in s.lower().arrays()] != [a.tobytes() for a in s.lower(plain_cse=True).arrays()]
    assert changed >= 1


# ---- the condition on the device tests' scenes ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', LF.READS_Y)
def test_stale_guards_change_the_scenes_the_device_tests_use(name):
    """A kernel that took one of these tapes for a rectangle-guarded one (guards of a group of 8 or 32 rows from its first
    row) would render another image: the device tests can tell.  With groups of one row it is the oracle's image."""
    w, h = LF.GPU_SIZE
    data, tape = LF.reads_y_tape(name)
    _, want64 = OScene(data).render_rows(w, h, 0, h, threads=THREADS)
    assert same_f64(LF.render_with_stale_guards(tape, w, 0, h, yrows=1, tile=64), want64)
    for yrows in (8, 32):
        got = LF.render_with_stale_guards(tape, w, 0, h, yrows=yrows, tile=64)
        assert not same_f64(got, want64), (name, yrows)


@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('name', LF.READS_Y)
def test_stale_guards_change_the_supersampled_scenes_too(name, k):
    """The same condition on the tapes of the supersampled device tests, on their sample rasters (k = 8 is the k = 4 picture
    sampled twice as finely: its raster is left to the device test)."""
    w, h = LF.SS_SIZE[0] * k, LF.SS_SIZE[1] * k
    s, tape = LF.ss_tape(name, k)
    _, want64 = OScene(s.encode()).render_rows(w, h, 0, h, threads=THREADS)
    assert same_f64(LF.render_with_stale_guards(tape, w, 0, h, yrows=1, tile=64), want64)
    for yrows in (8, 32):
        assert not same_f64(LF.render_with_stale_guards(tape, w, 0, h, yrows=yrows, tile=64), want64), (name, k, yrows)


# ---- offline builds: what the device tests compile, compiled here -----------------------------------------------------------
def _build(tape, k=0):
    L = M.lib()
    L.maray_jit_build.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.maray_jit_build_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    code, n = C.c_void_p(), C.c_size_t()
    if k:
        rc = L.maray_jit_build_samples(C.byref(tape.program), k, C.byref(code), C.byref(n))
    else:
        rc = L.maray_jit_build(C.byref(tape.program), C.byref(code), C.byref(n))
    assert rc == 0, L.maray_last_error().decode()[-2000:]
    blob = C.string_at(code, n.value)
    L.maray_free(code)
    assert blob[:4] == b'\x7fELF'


def _build_all(jobs):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:          # a build is compiler processes of its own; the threads only wait
        list(pool.map(lambda j: _build(*j), jobs))


@pytest.mark.parametrize('name', LF.GPU_SCENES)
def test_every_form_of_the_device_scenes_builds_offline(name, tmp_path, monkeypatch):
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path))
    data, _ = LF.gpu_scene(name)
    _build_all([(tape,) for tape in LF.lowered_forms(M.Scene(data)).values()])


def test_reads_y_tapes_build_offline_supersampled(tmp_path, monkeypatch):
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path))
    _build_all([(LF.ss_tape(name, k)[1], k) for name in LF.READS_Y for k in (2, 4)])


def test_deferring_scene_builds_offline_unfused_and_with_guards_that_read_y(tmp_path, monkeypatch):
    from test_gpu_launches import tri_soup
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path))
    w, h = LF.GPU_SIZE
    s = M.Scene(encode((w, h), tri_soup(1, [(0, w, 0, h, 16, 40)], w, h, huge_sin=True)))
    _build_all([(s.lower(**kw),) for kw in (dict(fuse=False), dict(y_spans=False), dict(fuse=False, y_spans=False))])
