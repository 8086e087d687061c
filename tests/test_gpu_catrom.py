"""The Catmull-Rom reconstruction filter on the device, on real scenes (include/maray_hip.h, "reconstruction filter"), compared
byte for byte, never with a tolerance.

The expected image of a context with samples = k, filter = FILTER_CATROM is `catrom` (tests/catrom_model.py: the contract in
numpy) of what a plain context of the same supersampled program renders at k w x k h.  The scenes: all_ops at 67 x 41, the
chess fixture, and the parametrised `slide` scene.  (Scene.rescale only enlarges and the top left of the chess picture is one
flat colour, so there is no small chess picture with anything in it: chess is taken at its own 1024 x 1024 at k = 2, and at
k = 4 and 8, where the vertical sums have 64 bits, on rows of its left 512 columns across the board's edges.)"""
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import params as PR
import scenes
from catrom_model import catrom
from marayb import encode
from test_filter import tent
from test_gpu_shutter import mean
from test_gpu_supersample import BACKENDS, box, chess_bytes, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 67, 41

_cache = {}


def device_samples(ss, w, h, k):
    """The scalar-cache interpreter's plain render of the supersampled scene (the whole sample raster)."""
    plain = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM)
    s8, _ = plain.render_rows(w * k, h * k, 0, h * k, want_f64=False)
    plain.close()
    return s8


def all_ops_case(k):
    """(scene bytes, samples, catrom of them): computed once, never written to."""
    if ('all_ops', k) not in _cache:
        data = encode((W, H), scenes.all_ops(W, H))
        s8 = device_samples(supersampled(data, k), W, H, k)
        want = catrom(s8, k)
        s8.setflags(write=False)
        want.setflags(write=False)
        _cache[('all_ops', k)] = (data, s8, want)
    return _cache[('all_ops', k)]


def chess_case():
    if 'chess' not in _cache:
        k = 2
        s8 = device_samples(supersampled(chess_bytes(), k), 1024, 1024, k)
        want = catrom(s8, k)
        want.setflags(write=False)
        _cache['chess'] = (k, want, box(s8, k), tent(s8, k))
    return _cache['chess']


# ---- contexts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
def test_all_ops_equals_catrom_of_the_plain_render(backend, k):
    data, s8, want = all_ops_case(k)
    ctx = M.Context(supersampled(data, k).lower(), backend=backend, samples=k, filter=M.FILTER_CATROM)
    assert '_ss' not in ctx.kernel_name                     # the inner context is the program's plain one
    assert ctx.kernel_name.endswith('+maray_filter_catrom<%d>' % k), ctx.kernel_name
    got, _ = ctx.render_rows(W, H, 0, H, want_f64=False)
    assert np.array_equal(got, want)
    part, _ = ctx.render_rows(W, H, 13, 29, want_f64=False)
    assert np.array_equal(part, want[13:29])
    assert ctx.time_rows(W, H, 0, H, reps=2) > 0.0
    ctx.close()
    assert not np.array_equal(want, box(s8, k)) and not np.array_equal(want, tent(s8, k))


def test_chess_equals_catrom_of_the_plain_render():
    k, want, want_box, want_tent = chess_case()
    ctx = M.Context(supersampled(chess_bytes(), k).lower(), backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_CATROM)
    got, _ = ctx.render_rows(1024, 1024, 0, 1024, want_f64=False)
    ctx.close()
    assert np.array_equal(got, want)
    assert not np.array_equal(want, want_box) and not np.array_equal(want, want_tent)


@pytest.mark.parametrize('k,backends', [(4, [M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]), (8, [M.BACKEND_TAPE_SMEM])])
def test_chess_rows_at_k4_and_k8(k, backends):
    """Chess, the left 512 columns of the stored 1024^2 scene, output rows across the board's edges (as test_gpu_supersample
    does for the box): each range equals catrom of the plain context's sample rows around it, two output rows more on either
    side so that no kept row clamps to the slab."""
    tape = supersampled(chess_bytes(), k).lower()
    plain = M.Context(tape, backend=M.BACKEND_TAPE_SMEM)
    ctxs = [M.Context(tape, backend=b, samples=k, filter=M.FILTER_CATROM) for b in backends]
    differs = False
    for y0, y1 in ((512, 515), (700, 701), (815, 824)):
        slab, _ = plain.render_rows(512 * k, 1024 * k, (y0 - 2) * k, (y1 + 2) * k, want_f64=False)
        want = catrom(slab, k)[2:-2]
        differs = differs or not np.array_equal(want, box(slab, k)[2:-2])
        for ctx in ctxs:
            got, _ = ctx.render_rows(512, 1024, y0, y1, want_f64=False)
            assert np.array_equal(got, want), (y0, y1, ctx.kernel_name)
    assert differs                  # else the rows show nothing about the filter
    plain.close()
    for ctx in ctxs:
        ctx.close()


# ---- composition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_parametrised_scene_and_shutter(backend):
    """set_params passes through, and frame i of a shutter call is the Catmull-Rom-filtered frame of row i."""
    k, (w, h) = 2, (96, 80)
    spec = PR.SCENES['slide'](w, h)
    scene, names = PR.declared(spec, (w, h))
    scene.supersample(k)
    tape = scene.lower()
    rows = [(-6.0, 2.0), (1.5, -1.25), (9.0, -5.0), (18.0, -10.0)]
    ctx = M.Context(tape, backend=backend, samples=k, filter=M.FILTER_CATROM)
    plain = M.Context(tape, backend=M.BACKEND_TAPE_SMEM)
    assert ctx.param_count == 2
    frames = []
    for r in rows:
        ctx.set_params(r)
        plain.set_params(r)
        frames.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
        assert np.array_equal(frames[-1], catrom(plain.render_rows(w * k, h * k, 0, h * k, want_f64=False)[0], k)), r
    plain.close()
    assert not np.array_equal(frames[0], frames[3])
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, mean(frames)), ctx.kernel_name
    part = ctx.render_rows_shutter(w, h, 11, 50, rows)
    assert np.array_equal(part, mean(frames)[11:50])
    again, _ = ctx.render_rows(w, h, 0, h, want_f64=False)           # the values set_params set are what they were
    assert np.array_equal(again, frames[3])
    ctx.close()


def test_render_png_decodes_to_the_picture(tmp_path):
    k = 4
    data, _, want = all_ops_case(k)
    ctx = M.Context(supersampled(data, k).lower(), backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_CATROM)
    png = ctx.render_png(W, H)
    ctx.close()
    path = tmp_path / 'c.png'
    path.write_bytes(bytes(png))
    assert np.array_equal(M.png_read(str(path)), want)


def test_time_filter_times_the_kernel_alone():
    for k in (2, 4, 8):
        assert M.time_filter(130, 40, k, reps=2, filter=M.FILTER_CATROM) > 0.0
    with pytest.raises(M.MarayError) as e:
        M.time_filter(130, 40, 4, reps=2, filter=M.FILTER_CATROM, transfer=M.TRANSFER_SRGB)
    assert e.value.code == -1


# ---- façade ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_gen_to_image_tiles(k):
    """tile_rows of 5 and 16: every tile and worker renders its own halo."""
    data, _, want = all_ops_case(k)
    old = os.environ.get('MARAY_GEN_WRAP_DEVICES')
    os.environ['MARAY_GEN_WRAP_DEVICES'] = '1'
    try:
        M.gen_cache_clear()
        s = M.Scene(data)
        for tile_rows, n_dev in ((5, 1), (16, 1), (5, 2)):
            assert np.array_equal(M.gen_to_image(s, samples=k, filter=M.FILTER_CATROM, n_devices=n_dev, tile_rows=tile_rows), want), (tile_rows, n_dev)
        info = M.gen_cache_info()
        assert info and all(line.endswith(' samples %d filter catrom' % k) for line in info), info
        assert all('/catrom' in line.split()[0] and '+maray_filter_catrom<%d> ' % k in line for line in info), info
    finally:
        if old is None:
            del os.environ['MARAY_GEN_WRAP_DEVICES']
        else:
            os.environ['MARAY_GEN_WRAP_DEVICES'] = old
        M.gen_cache_clear()


def test_box_and_tent_keep_their_pictures_and_the_cache_keeps_three():
    """Box and tent contexts created before and after a Catmull-Rom one render what they rendered; the façade keeps the three
    programs side by side."""
    k = 4
    data, s8, want = all_ops_case(k)
    tape = supersampled(data, k).lower()
    wants = {M.FILTER_BOX: box(s8, k), M.FILTER_TENT: tent(s8, k), M.FILTER_CATROM: want}
    for backend in (M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
        order = (M.FILTER_BOX, M.FILTER_TENT, M.FILTER_CATROM, M.FILTER_TENT, M.FILTER_BOX)
        ctxs = [M.Context(tape, backend=backend, samples=k, filter=f) for f in order]
        for _ in range(2):
            for f, c in zip(order, ctxs):
                got, _ = c.render_rows(W, H, 0, H, want_f64=False)
                assert np.array_equal(got, wants[f]), (backend, f)
        assert ctxs[1].kernel_name.endswith('+maray_filter_tent<4>') and '_ss' in ctxs[0].kernel_name
        for c in ctxs:
            c.close()
    M.gen_cache_clear()
    try:
        s = M.Scene(data)
        for f in (M.FILTER_TENT, M.FILTER_CATROM, M.FILTER_BOX, M.FILTER_CATROM, M.FILTER_TENT):
            assert np.array_equal(M.gen_to_image(s, samples=k, filter=f, n_devices=1), wants[f]), f
        info = M.gen_cache_info()
        assert len(info) == 3 and len({line.split()[0] for line in info}) == 3, info
        assert sum(line.endswith(' samples 4 filter catrom') for line in info) == 1, info
        assert sum(line.endswith(' samples 4 filter tent') for line in info) == 1, info
        assert sum(line.endswith(' samples 4') for line in info) == 1, info
    finally:
        M.gen_cache_clear()


def test_cli_writes_the_picture(tmp_path):
    k, want, want_box, _ = chess_case()
    path = os.path.join(HERE, 'golden', 'chess.maray')
    out = tmp_path / 'chess_catrom.png'
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '-s', str(k), '--filter', 'catrom', '-i', path, '-o', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(M.png_read(str(out)), want)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    data, _, _ = all_ops_case(2)
    tape = supersampled(data, 2).lower()
    ctx = M.Context(tape, backend=M.BACKEND_TAPE_SMEM, samples=2, filter=M.FILTER_CATROM)
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows(W, H, 0, H, want_f64=True)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows((1 << 19) + 1, H, 0, 1, want_f64=False)
    assert e.value.code == -7
    ctx.close()
    for kw in (dict(samples=0, filter=M.FILTER_CATROM), dict(samples=1, filter=M.FILTER_CATROM), dict(samples=2, filter=2),
               dict(samples=2, filter=M.FILTER_CATROM, transfer=M.TRANSFER_SRGB)):
        with pytest.raises(M.MarayError) as e:
            M.Context(tape, backend=M.BACKEND_TAPE_SMEM, **kw)
        assert e.value.code == -1, kw
