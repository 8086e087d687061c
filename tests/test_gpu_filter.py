"""The tent reconstruction filter on the device (include/maray_hip.h, "reconstruction filter"), compared byte for byte, never
with a tolerance.

The expected image of a context with samples = k, filter = FILTER_TENT is `tent` (tests/test_filter.py: the contract in numpy)
of the plain render of the supersampled scene at k w x k h: from the CPU oracle where the whole picture is compared, from the
device's own plain render where the question is how the picture was cut."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
import scenes
from marayb import encode
from oracle_ffi import Scene as OScene
from test_filter import tent
from test_gpu_launches import tri_soup
from test_gpu_shutter import mean
from test_gpu_supersample import BACKENDS, THREADS, box, chess_bytes, scene_case, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILE_W = 64                 # output pixels a block of maray_filter_tent computes (filter.hpp)

_oracle = {}


def oracle_samples(name, k):
    """The oracle's plain render of the supersampled scene: computed once for the three back-ends, never written to."""
    if (name, k) not in _oracle:
        data, w, h, tex = scene_case(name)
        ss = supersampled(data, k)
        want8, _ = OScene(ss.encode()).render_rows(w * k, h * k, 0, h * k, textures=tex, threads=THREADS, want_f64=False)
        want8.setflags(write=False)
        _oracle[(name, k)] = want8
    return _oracle[(name, k)]


class band_rows:
    """MARAY_FILTER_BAND_ROWS for the contexts created inside (it is read when a context is created)."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.old = os.environ.get('MARAY_FILTER_BAND_ROWS')
        if self.rows is None:
            os.environ.pop('MARAY_FILTER_BAND_ROWS', None)
        else:
            os.environ['MARAY_FILTER_BAND_ROWS'] = str(self.rows)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('MARAY_FILTER_BAND_ROWS', None)
        else:
            os.environ['MARAY_FILTER_BAND_ROWS'] = self.old


def device_samples(ss, w, h, k, tex=None):
    """The scalar-cache interpreter's plain render of the supersampled scene (the whole sample raster)."""
    plain = M.Context(ss.lower(), textures=tex, backend=M.BACKEND_TAPE_SMEM)
    s8, _ = plain.render_rows(w * k, h * k, 0, h * k, want_f64=False)
    plain.close()
    return s8


# ---- oracle parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', ['all_ops', 'edges', 'textured', 'tri_soup', 'huge_sin'])
def test_equals_tent_filter_of_the_oracle(name, backend, k):
    data, w, h, tex = scene_case(name)
    ss = supersampled(data, k)
    s8 = oracle_samples(name, k)
    ctx = M.Context(ss.lower(), textures=tex, backend=backend, samples=k, filter=M.FILTER_TENT)
    assert '_ss' not in ctx.kernel_name                     # the inner context is the program's plain one
    assert ctx.kernel_name.endswith('+maray_filter_tent<%d>' % k), ctx.kernel_name
    got8, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    want = tent(s8, k)
    assert np.array_equal(got8, want)
    if name == 'tri_soup':
        assert not np.array_equal(want, box(s8, k))        # else the comparison above shows nothing about the filter


# ---- band and halo independence --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_bands_halos_and_ragged_widths(k):
    """Every way of cutting a 37-row picture gives the slices of the one picture: one, three and all rows per band, whole
    image and row ranges at the top clamp, the bottom clamp and in the interior (single rows: the halo is larger than the
    rows); widths whose rows are misaligned (5: 15 bytes) and one below, at and one above the kernel's tile."""
    h = 37
    for w in (1, 3, 5, TILE_W - 1, TILE_W, TILE_W + 1):
        data = encode((w, h), tri_soup(3, [(0, w, 0, h, 3, max(2, w // 2))], w, h)) if w >= 3 else encode((w, h), scenes.all_ops(w, h))
        ss = supersampled(data, k)
        want = tent(device_samples(ss, w, h, k), k)
        tape = ss.lower()
        for rows in (1, 3, 1000):
            for backend in ([M.BACKEND_TAPE_SMEM, M.BACKEND_JIT] if w == TILE_W + 1 else [M.BACKEND_TAPE_SMEM]):
                with band_rows(rows):
                    ctx = M.Context(tape, backend=backend, samples=k, filter=M.FILTER_TENT)
                got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
                assert np.array_equal(got, want), (w, rows, backend)
                for y0, y1 in ((0, 1), (5, 6), (17, 30), (h - 1, h)):
                    got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
                    assert np.array_equal(got, want[y0:y1]), (w, rows, backend, y0, y1)
                ctx.close()


def test_host_tiles_have_halos_of_their_own():
    """render_tiles with tiles out of order and not on the filter's tile grid, three output rows per band."""
    k, w, h = 4, 100, 61
    data = encode((w, h), tri_soup(8, [(0, w, 0, h, 14, 20)], w, h))
    ss = supersampled(data, k)
    want = tent(device_samples(ss, w, h, k), k)
    with band_rows(3):
        ctx = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_TENT)
    img = np.full((h, w, 3), 0xA5, np.uint8)
    tiles = [(40, 61), (0, 7), (7, 8), (21, 40)]
    ctx.render_tiles(w, h, tiles, img)
    ctx.close()
    for y0, y1 in tiles:
        assert np.array_equal(img[y0:y1], want[y0:y1]), (y0, y1)
    assert (img[8:21] == 0xA5).all()


# ---- device pointers --------------------------------------------------------------------------------------------------------
_DEVICE_GEOMETRY = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from marayb import encode
from test_filter import tent
from test_gpu_launches import tri_soup
from test_gpu_supersample import supersampled
PAD, FILL = 64, 0xA5
k, w, h = 4, 201, 96
data = encode((w, h), tri_soup(6, [(0, w, 0, h, 16, 30)], w, h))
ss = supersampled(data, k)
plain = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM)
want = tent(plain.render_rows(w * k, h * k, 0, h * k, want_f64=False)[0], k)
plain.close()
for backend, band in ((M.BACKEND_TAPE, None), (M.BACKEND_TAPE_SMEM, '3'), (M.BACKEND_JIT, None), (M.BACKEND_JIT, '5')):
    os.environ.pop('MARAY_FILTER_BAND_ROWS', None)
    if band:
        os.environ['MARAY_FILTER_BAND_ROWS'] = band
    ctx = M.Context(ss.lower(), backend=backend, samples=k, filter=M.FILTER_TENT)
    for g in (('rows', 0, 96), ('rows', 33, 34), ('blocks', 3, 5, 16, 6), ('blocks', 0, 8, 32, 3), ('blocks', 10, 1, 7, 12)):
        n = g[2] - g[1] if g[0] == 'rows' else g[2] * g[4]
        rows = np.arange(g[1], g[2]) if g[0] == 'rows' else (g[1] + np.arange(g[4])[:, None] * g[3] + np.arange(g[2])[None, :]).reshape(-1)
        for off in (0, 1):                      # the destination at any alignment: w * 3 is odd, so rows alternate anyway
            b8 = torch.full(((n + 2 * PAD) * w * 3 + 8,), FILL, dtype=torch.uint8, device='cuda')
            lo = PAD * w * 3 + off
            p8 = b8.data_ptr() + lo
            if g[0] == 'rows':
                ctx.render_rows_device(w, h, g[1], g[2], d_rgb8=p8)
            else:
                ctx.render_blocks_device(w, h, *g[1:], d_rgb8=p8)
            torch.cuda.synchronize()
            assert bool((b8[:lo] == FILL).all()) and bool((b8[lo + n * w * 3:] == FILL).all()), ('guard band written', g)
            assert np.array_equal(b8[lo:lo + n * w * 3].cpu().numpy().reshape(n, w, 3), want[rows]), (backend, band, g, off)
    ctx.close()
print('ok')
"""


def test_device_buffers_blocks_and_guard_bands():
    """render_rows_device and render_blocks_device (block_stride > block_rows: every block has a halo of its own) into
    buffers with guard bands, at an even and an odd address (a process of its own: the device buffers come from PyTorch,
    imported before the library)."""
    code = _DEVICE_GEOMETRY % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_shutter_averages_tent_filtered_frames(backend):
    """Frame i of a shutter call is what the context renders after set_params(row i): here the tent-filtered frame."""
    k, (w, h) = 2, (96, 80)
    spec = PR.SCENES['slide'](w, h)
    scene, names = PR.declared(spec, (w, h))
    scene.supersample(k)
    rows = [(-6.0, 2.0), (1.5, -1.25), (9.0, -5.0), (18.0, -10.0)]
    with band_rows(24):
        ctx = M.Context(scene.lower(), backend=backend, samples=k, filter=M.FILTER_TENT)
    assert ctx.param_count == 2
    frames = []
    for r in rows:
        ctx.set_params(r)
        frames.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
    assert not np.array_equal(frames[0], frames[3])
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, mean(frames)), ctx.kernel_name
    part = ctx.render_rows_shutter(w, h, 11, 50, rows)
    assert np.array_equal(part, mean(frames)[11:50])
    # the values set_params set are what they were before the shutter call
    again, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(again, frames[3])
    ctx.close()


@pytest.mark.parametrize('backend', [M.BACKEND_JIT, M.BACKEND_TAPE_SMEM])
def test_alternating_tent_box_and_plain_launches_give_their_first_results(backend):
    w, h, k = 300, 90, 4
    data = encode((w, h), tri_soup(5, [(0, w, 0, h, 20, 25)], w, h))
    tape4 = supersampled(data, k).lower()
    plain = M.Context(M.Scene(data).lower(), backend=backend)
    aa = M.Context(tape4, backend=backend, samples=k)
    tt = M.Context(tape4, backend=backend, samples=k, filter=M.FILTER_TENT)
    first = [c.render_rows(w, h, 0, h, want_f64=False)[0] for c in (tt, aa, plain)]
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
    for _ in range(3):
        for c, f in ((tt, first[0]), (aa, first[1]), (tt, first[0]), (plain, first[2])):
            got, _ = c.render_rows(w, h, 0, h, want_f64=False)
            assert np.array_equal(got, f)
    assert tt.time_rows(w, h, 0, h, reps=2) > 0.0
    for c in (tt, aa, plain):
        c.close()
    assert M.time_filter(w, h, k, reps=2) > 0.0


# ---- façade -----------------------------------------------------------------------------------------------------------------
def facade_case():
    w, h, k = 333, 120, 4
    data = encode((w, h), tri_soup(7, [(0, w, 0, h, 25, 40)], w, h))
    ss = supersampled(data, k)
    ctx = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_TENT)
    single, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    s8 = device_samples(ss, w, h, k)
    assert np.array_equal(single, tent(s8, k))
    return data, single, box(s8, k)


def test_gen_to_image_on_two_workers_and_programs_per_filter():
    data, want_tent, want_box = facade_case()
    old = os.environ.get('MARAY_GEN_WRAP_DEVICES')
    os.environ['MARAY_GEN_WRAP_DEVICES'] = '1'
    try:
        M.gen_cache_clear()
        s = M.Scene(data)
        assert np.array_equal(M.gen_to_image(s, samples=4, filter=M.FILTER_TENT, n_devices=2, tile_rows=16), want_tent)
        M.gen_cache_clear()
        for f, want in ((M.FILTER_TENT, want_tent), (M.FILTER_BOX, want_box), (M.FILTER_TENT, want_tent)):
            assert np.array_equal(M.gen_to_image(s, samples=4, filter=f, n_devices=1), want), f
        info = M.gen_cache_info()
        assert len(info) == 2, info
        assert sum(line.endswith(' samples 4 filter tent') for line in info) == 1, info
        assert sum(line.endswith(' samples 4') for line in info) == 1, info
        assert len({line.split()[0] for line in info}) == 2, info
        assert all('+maray_filter_tent<4> ' in line for line in info if line.endswith(' filter tent')), info
        assert s.size == (333, 120)
    finally:
        if old is None:
            del os.environ['MARAY_GEN_WRAP_DEVICES']
        else:
            os.environ['MARAY_GEN_WRAP_DEVICES'] = old
        M.gen_cache_clear()


def test_cli_writes_the_pixels_of_gen_to_image(tmp_path):
    path = os.path.join(HERE, 'golden', 'chess.maray')
    out = tmp_path / 'chess_tent.png'
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '-s', '4', '--filter', 'tent', '-i', path, '-o', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = M.gen_to_image(M.Scene(chess_bytes()), samples=4, filter=M.FILTER_TENT)
    got = M.png_read(str(out))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, M.gen_to_image(M.Scene(chess_bytes()), samples=4))
    M.gen_cache_clear()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    data = encode((67, 41), scenes.all_ops(67, 41))
    tape = supersampled(data, 2).lower()
    ctx = M.Context(tape, backend=M.BACKEND_TAPE_SMEM, samples=2, filter=M.FILTER_TENT)
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows(67, 41, 0, 41, want_f64=True)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows((1 << 19) + 1, 41, 0, 1, want_f64=False)
    assert e.value.code == -7
    ctx.close()
    for kw in (dict(samples=0, filter=M.FILTER_TENT), dict(samples=1, filter=M.FILTER_TENT), dict(samples=2, filter=2)):
        with pytest.raises(M.MarayError) as e:
            M.Context(tape, backend=M.BACKEND_TAPE_SMEM, **kw)
        assert e.value.code == -1, kw
