"""maray_filter_catrom<K> on sample rasters of any bytes, compared byte for byte, never with a tolerance.

The scene is the texture-identity scene of tests/byte_rasters.py: its sample raster IS the texture S a context is created
with, so the expected picture is the numpy contract on S itself -- catrom(S, k) (tests/catrom_model.py) -- with no oracle
render.  That these rasters reach both output clamps and tell every mutant of the contract from the contract is checked
without a device in tests/test_catrom.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import catrom_model as CM
import maray_amd as M
from catrom_model import catrom

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]

_tape = []


def identity_tape():
    """One program for every k, size and raster."""
    if not _tape:
        _tape.append(BR.identity_scene().lower())
    return _tape[0]


def catrom_context(s8, k, backend=M.BACKEND_TAPE_SMEM):
    return M.Context(identity_tape(), textures=[s8], backend=backend, samples=k, filter=M.FILTER_CATROM)


def child(code, env=None):
    r = subprocess.run([sys.executable, '-c', code % {'root': ROOT, 'tests': HERE}], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
def test_random_bytes_equal_the_contract(backend, k):
    """65 x 37 pixels of uniform random bytes on the three back-ends."""
    w, h = BR.PARITY_W, BR.PARITY_H
    s8 = BR.parity_raster(k)
    ctx = catrom_context(s8, k, backend)
    assert ctx.kernel_name.endswith('+maray_filter_catrom<%d>' % k), ctx.kernel_name
    got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    assert np.array_equal(got, catrom(s8, k))


# ---- the clamps, the extremes, impulses --------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_lobe_rasters_extremes_and_impulses(k):
    """The lobe raster and its inverse (the largest and the smallest sum there is: both output clamps, and at k = 4 and 8 sums
    past 32 bits), all 0, all 255, and single samples in the corners and one before, at and after the tiles' boundaries."""
    for name, s8, w, h in CM.gpu_rasters(k)[1:]:
        ctx = catrom_context(s8, k)
        got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
        ctx.close()
        want = catrom(s8, k)
        assert np.array_equal(got, want), name
        if name.startswith('lobe'):
            assert (want == 0).any() and (want == 255).any()


# ---- geometry ----------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = (1, 2, 3, 5, 64, 65, 67, 129), (1, 2, 3, 9, 17)


@pytest.mark.parametrize('k', [2, 4, 8])
def test_widths_and_heights(k):
    """w <= 3 makes every lane an edge lane, as h <= 3 makes every row a clamped one; one below ... above the tile of 64
    pixels, two tiles and one; heights of one tile of rows and less, two (k = 2) or three tiles."""
    for w in WIDTHS:
        for h in HEIGHTS:
            s8 = BR.random_bytes(7000 + 100 * k + 10 * w + h, h * k, w * k)
            ctx = catrom_context(s8, k)
            got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
            ctx.close()
            assert np.array_equal(got, catrom(s8, k)), (w, h)


@pytest.mark.parametrize('k', [2, 4, 8])
def test_every_row_range_of_nine_rows(k):
    """render_rows over every [y0, y1) of a 9-row image is the slice of the whole picture: the halo is cut from the image."""
    w, h = 67, 9
    s8 = BR.random_bytes(7900 + k, h * k, w * k)
    want = catrom(s8, k)
    ctx = catrom_context(s8, k)
    for y0 in range(h):
        for y1 in range(y0 + 1, h + 1):
            got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
            assert np.array_equal(got, want[y0:y1]), (y0, y1)
    ctx.close()


_BANDS = r"""
import os, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import maray_amd as M
from catrom_model import catrom
assert os.environ['MARAY_FILTER_BAND_ROWS'] in ('1', '3', '8')
tape = BR.identity_scene().lower()
w, h = BR.PARITY_W, BR.PARITY_H
for k in (2, 4, 8):
    s8 = BR.parity_raster(k)
    want = catrom(s8, k)
    for backend in (M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
        ctx = M.Context(tape, textures=[s8], backend=backend, samples=k, filter=M.FILTER_CATROM)
        got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
        assert np.array_equal(got, want), (k, backend)
        for y0, y1 in ((0, 1), (1, 3), (5, 6), (7, 30), (h - 2, h), (h - 1, h)):
            got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
            assert np.array_equal(got, want[y0:y1]), (k, backend, y0, y1)
        ctx.close()
print('ok')
"""


@pytest.mark.parametrize('rows', CM.BAND_ROWS)
def test_band_rows(rows):
    """MARAY_FILTER_BAND_ROWS of 1, 3 and 8 output rows (a band's halo, 3k/2 rows, is then larger than the band or about its
    size): the picture and its row ranges are those of one band.  In a fresh child process: the variable is read when a
    context is created."""
    child(_BANDS, env={'MARAY_FILTER_BAND_ROWS': str(rows)})


# ---- destinations ------------------------------------------------------------------------------------------------------
_DESTINATIONS = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import maray_amd as M
from catrom_model import catrom
PAD, FILL = 256, 0xA5
h = BR.DESTINATION_H
tape = BR.identity_scene().lower()
for k in (2, 4, 8):
    for w in BR.DESTINATION_WS:
        s8 = BR.destination_raster(k, w)
        want = catrom(s8, k)
        ctx = M.Context(tape, textures=[s8], backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_CATROM)
        for g in (('rows', 0, h), ('rows', 7, 8), ('blocks', 2, 3, 5, 4), ('blocks', 0, 1, 11, 3), ('blocks', 1, 9, 12, 2)):
            n = g[2] - g[1] if g[0] == 'rows' else g[2] * g[4]
            rows = np.arange(g[1], g[2]) if g[0] == 'rows' else (g[1] + np.arange(g[4])[:, None] * g[3] + np.arange(g[2])[None, :]).reshape(-1)
            assert rows.max() < h
            for off in (0, 1, 2, 3):
                b8 = torch.full((n * w * 3 + 2 * PAD,), FILL, dtype=torch.uint8, device='cuda')
                lo = PAD + off
                p8 = b8.data_ptr() + lo
                assert p8 %% 4 == off
                if g[0] == 'rows':
                    ctx.render_rows_device(w, h, g[1], g[2], d_rgb8=p8)
                else:
                    ctx.render_blocks_device(w, h, *g[1:], d_rgb8=p8)
                torch.cuda.synchronize()
                assert bool((b8[:lo] == FILL).all()) and bool((b8[lo + n * w * 3:] == FILL).all()), ('guard band written', k, w, g, off)
                assert np.array_equal(b8[lo:lo + n * w * 3].cpu().numpy().reshape(n, w, 3), want[rows]), (k, w, g, off)
        ctx.close()
print('ok')
"""


def test_destinations_guard_bytes_and_blocks():
    """render_rows_device and render_blocks_device (block_stride > block_rows: every block has a halo of its own) into buffers
    with guard bytes on both sides at byte offsets 0, 1, 2, 3, for w = 1, 5, 64, 65: nothing outside the rows changes (a
    process of its own: the device buffers come from PyTorch, imported before the library)."""
    child(_DESTINATIONS)
