"""maray_filter_tent<K> (and the box kernels) on sample rasters of any bytes, compared byte for byte, never with a tolerance.

The scene is the texture-identity scene of tests/byte_rasters.py: its sample raster IS the texture S a context is created
with, so the expected picture is the numpy contract on S itself -- tent(S, k) (tests/test_filter.py), box(S, k) -- with no
oracle render, and S is random bytes, extremes or impulses where the scenes' rasters are flat or smooth.  That the scene
renders S, and that these rasters tell every mutant of the contract from the contract, is checked without a device in
tests/test_byte_rasters.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import maray_amd as M
from test_filter import tent
from test_gpu_filter import band_rows
from test_gpu_supersample import BACKENDS, SS_KERNELS, box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_tape = []


def identity_tape():
    """One program for every k, size and raster."""
    if not _tape:
        _tape.append(BR.identity_scene().lower())
    return _tape[0]


def tent_context(s8, k, backend=M.BACKEND_TAPE_SMEM):
    return M.Context(identity_tape(), textures=[s8], backend=backend, samples=k, filter=M.FILTER_TENT)


# ---- parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
def test_random_bytes_equal_the_contracts(backend, k):
    """65 x 37 pixels of uniform random bytes: a footprint one sample off shows on 0.97 of the pixels, and some sum sits on
    either side of the rounding."""
    w, h = BR.PARITY_W, BR.PARITY_H
    s8 = BR.parity_raster(k)
    ctx = tent_context(s8, k, backend)
    assert ctx.kernel_name.endswith('+maray_filter_tent<%d>' % k), ctx.kernel_name
    got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    assert np.array_equal(got, tent(s8, k))
    ctx = M.Context(identity_tape(), textures=[s8], backend=backend, samples=k)
    assert ctx.kernel_name.startswith(SS_KERNELS)
    got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    assert np.array_equal(got, box(s8, k))


# ---- extremes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_extremes(k):
    """All 0, all 255 (the largest LDS sums, 255 * 2 k^2), a checker at one-sample pitch, and single sample columns and rows
    that show every weight on its own."""
    w, h = BR.EXTREMES_W, BR.EXTREMES_H
    for name, s8 in BR.extreme_rasters(h, w, k):
        ctx = tent_context(s8, k)
        got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
        ctx.close()
        assert np.array_equal(got, tent(s8, k)), name


# ---- geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_bands_halos_and_widths_on_random_bytes(k):
    """Every way of cutting a 19-row picture gives the slices of tent(S, k): one, three and all rows per band; the whole image
    and row ranges at the top clamp, in the interior and at the bottom clamp.  w = 1 and 2 make every lane an edge lane; odd w
    at k = 2 is a row pitch of 2 modulo 4, so the rows take all four shifts of a misaligned dword between them."""
    h = BR.GEOMETRY_H
    for w in BR.GEOMETRY_WS:
        s8 = BR.geometry_raster(k, w)
        want = tent(s8, k)
        for rows in (1, 3, 1000):
            for backend in ([M.BACKEND_TAPE_SMEM, M.BACKEND_JIT] if w == 65 else [M.BACKEND_TAPE_SMEM]):
                with band_rows(rows):
                    ctx = tent_context(s8, k, backend)
                got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
                assert np.array_equal(got, want), (w, rows, backend)
                for y0, y1 in ((0, 1), (5, 6), (7, 16), (h - 1, h)):
                    got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
                    assert np.array_equal(got, want[y0:y1]), (w, rows, backend, y0, y1)
                ctx.close()


# ---- destinations ----------------------------------------------------------------------------------------------------------
_DESTINATIONS = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import maray_amd as M
from test_filter import tent
PAD, FILL = 256, 0xA5
h = BR.DESTINATION_H
tape = BR.identity_scene().lower()
for k in BR.DESTINATION_KS:
    for w in BR.DESTINATION_WS:
        s8 = BR.destination_raster(k, w)
        want = tent(s8, k)
        ctx = M.Context(tape, textures=[s8], backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_TENT)
        for g in (('rows', 0, h), ('rows', 7, 8), ('blocks', 2, 3, 5, 4), ('blocks', 0, 1, 11, 3)):
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


def test_destinations_at_every_alignment():
    """render_rows_device and render_blocks_device (block_stride > block_rows) into buffers with guard bands at byte offsets 0,
    1, 2, 3, for w = 1, 5, 64, 65 and k = 2, 8: the dword-or-bytes store at every alignment and at the row ends (a process of
    its own: the device buffers come from PyTorch, imported before the library)."""
    code = _DESTINATIONS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- streams ---------------------------------------------------------------------------------------------------------------
_STREAMS = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import maray_amd as M
from test_filter import tent
FILL = 0xA5
w, h, k = BR.STREAMS_W, BR.STREAMS_H, BR.STREAMS_K
s8 = BR.streams_raster()
want = tent(s8, k)
os.environ['MARAY_FILTER_BAND_ROWS'] = '3'
ctx = M.Context(BR.identity_scene().lower(), textures=[s8], backend=M.BACKEND_TAPE_SMEM, samples=k, filter=M.FILTER_TENT)
ranges = [(0, h), (40, 41), (7, 100), (h - 30, h)]
streams = [torch.cuda.Stream(), torch.cuda.Stream()]
bufs = [torch.full(((y1 - y0) * w * 3 + 64,), FILL, dtype=torch.uint8, device='cuda') for y0, y1 in ranges]
torch.cuda.synchronize()
for i, ((y0, y1), b) in enumerate(zip(ranges, bufs)):
    ctx.render_rows_device(w, h, y0, y1, d_rgb8=b.data_ptr() + 32, stream=streams[i %% 2].cuda_stream)
torch.cuda.synchronize()
for (y0, y1), b in zip(ranges, bufs):
    g = b.cpu().numpy()
    assert (g[:32] == FILL).all() and (g[-32:] == FILL).all(), ('guard band written', y0, y1)
    assert np.array_equal(g[32:-32].reshape(y1 - y0, w, 3), want[y0:y1]), (y0, y1)
ctx.close()
print('ok')
"""


def test_calls_in_flight_on_two_streams():
    """One tent context, 333 x 120 at k = 4 with three output rows per band; four render_rows_device calls of different row
    ranges enqueued alternately on two streams into four buffers, one synchronise at the end: each buffer holds its slice.  The
    bands of all four calls share the context's scratch, handed from stream to stream by an event.  A test cannot prove that
    ordering; it can only break where the ordering is plainly absent."""
    code = _STREAMS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]
