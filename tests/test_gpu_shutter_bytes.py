"""maray_shutter_reduce on frames of any bytes, compared byte for byte, never with a tolerance.

The scene is the atlas scene of tests/byte_rasters.py: with its one parameter set to t it renders slice t of the texture a
context is created with, so the n frames of a shutter call are whatever bytes a test lays side by side, and the expected
picture is the integer mean of those bytes (tests/test_gpu_shutter.py::mean) with no oracle render.  Random frames take every
residue modulo n to the rounding step, where the scenes' flat 0 / 255 shapes bring multiples of 255.  That the scene renders
its slices, and that these frames tell every mutant of the mean from the mean, is checked without a device in
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
from test_gpu_shutter import BACKENDS, mean
from test_gpu_supersample import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_tape = []


def atlas_tape():
    """One program for every n, size and atlas."""
    if not _tape:
        _tape.append(BR.atlas_scene().lower())
        assert _tape[0].param_count == 1
    return _tape[0]


def atlas_context(frames, backend=M.BACKEND_TAPE_SMEM, **kw):
    return M.Context(atlas_tape(), textures=[BR.atlas(frames)], backend=backend, **kw)


# ---- parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', BR.SHUTTER_NS)
@pytest.mark.parametrize('backend', BACKENDS)
def test_random_frames_equal_their_mean(backend, n):
    """n random frames of 67 x 41 (8241 bytes: a head or a tail whatever the scratch's alignment), their parameter rows passed
    in a shuffled order; the whole picture and two row ranges."""
    w, h = BR.SHUTTER_W, BR.SHUTTER_H
    frames, order = BR.shutter_case(n)
    want = mean(frames)
    rows = [(float(t),) for t in order]
    ctx = atlas_context(frames, backend)
    assert ctx.param_count == 1
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, want), ctx.kernel_name
    for y0, y1 in ((5, 6), (17, 30)):
        got = ctx.render_rows_shutter(w, h, y0, y1, rows)
        assert np.array_equal(got, want[y0:y1]), (y0, y1, ctx.kernel_name)
    ctx.close()


# ---- extremes --------------------------------------------------------------------------------------------------------------
def test_extremes():
    """Frames alternating all 0 and all 255 (every sum exactly half way: 128, and 127 were the rounding one less); all 255 in
    64 frames (16320, the most a 16-bit field holds); frames that differ from one another in one byte each, the first and the
    last byte among them."""
    w, h = BR.SHUTTER_W, BR.SHUTTER_H
    for n in (2, 8, 16, 64):
        frames = [BR.constant(255 * (i & 1), h, w) for i in range(n)]
        ctx = atlas_context(frames)
        got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in range(n)])
        ctx.close()
        assert (got == 128).all() and np.array_equal(got, mean(frames)), n
    frames = [BR.constant(255, h, w)] * 64
    ctx = atlas_context(frames)
    got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in range(64)])
    ctx.close()
    assert (got == 255).all()
    for n in (8, 64):
        frames = BR.one_byte_frames(n, h, w)
        ctx = atlas_context(frames)
        got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in range(n)])
        ctx.close()
        assert np.array_equal(got, mean(frames)), n


# ---- head, tail and alignment ----------------------------------------------------------------------------------------------
_HEAD_TAIL = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import maray_amd as M
from test_gpu_shutter import mean
PAD, FILL = 64, 0xA5
h = BR.HEAD_TAIL_ROWS[-1]
tape = BR.atlas_scene().lower()
b8 = torch.empty((2 * PAD + 16 + h * BR.HEAD_TAIL_WS[-1] * 3,), dtype=torch.uint8, device='cuda')
assert b8.data_ptr() %% 16 == 0
for n in BR.HEAD_TAIL_NS:
    frames, order = BR.head_tail_case(n)
    values = [(float(t),) for t in order]
    ctx = M.Context(tape, textures=[BR.atlas(frames)], backend=M.BACKEND_TAPE_SMEM)
    for w in BR.HEAD_TAIL_WS:
        for rows in BR.HEAD_TAIL_ROWS:
            size = rows * w * 3
            want = mean([f[:rows, :w] for f in frames]).reshape(-1)
            for mis in range(16):
                b8.fill_(FILL)
                lo = PAD + mis
                ctx.render_rows_shutter_device(w, h, 0, rows, values, b8.data_ptr() + lo)
                torch.cuda.synchronize()
                g = b8.cpu().numpy()
                assert (g[:lo] == FILL).all() and (g[lo + size:] == FILL).all(), ('guard bytes written', n, w, rows, mis)
                assert np.array_equal(g[lo:lo + size], want), (n, w, rows, mis)
    ctx.close()
print('ok')
"""


def test_head_tail_and_every_destination_misalignment():
    """Rasters of 3 .. 105 bytes (w = 1 and 5, 1 .. 7 rows: fewer bytes than one 16-byte vector, a head only, a head and a tail)
    at every destination misalignment 0 .. 15, for n = 2, 8, 16, 64, with guard bytes on both sides (a process of its own: the
    device buffers come from PyTorch, imported before the library)."""
    code = _HEAD_TAIL % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- composition -----------------------------------------------------------------------------------------------------------
COMPOSED_W, COMPOSED_H = 21, 13


def composed_case(k, n):
    """n random frames at sample scale, (k h, k w, 3) each, the shuffled order of their rows, a value of t in range."""
    frames = BR.random_frames(6000 + 10 * k + n, n, k * COMPOSED_H, k * COMPOSED_W)
    order = [int(i) for i in np.random.default_rng(7000 + n).permutation(n)]
    return frames, order, float(n // 2)


@pytest.mark.parametrize('k,n', [(2, 4), (4, 16)])
@pytest.mark.parametrize('backend', BACKENDS)
def test_shutter_averages_tent_filtered_slices(backend, k, n):
    """Frame i of a shutter call on a tent context is the tent-filtered slice; the values set before the call are restored."""
    w, h = COMPOSED_W, COMPOSED_H
    frames, order, t0 = composed_case(k, n)
    want = mean([tent(f, k) for f in frames])
    with band_rows(5):
        ctx = atlas_context(frames, backend, samples=k, filter=M.FILTER_TENT)
    ctx.set_params([t0])
    before, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(before, tent(frames[int(t0)], k))
    got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in order])
    assert np.array_equal(got, want), ctx.kernel_name
    got = ctx.render_rows_shutter(w, h, 3, 11, [(float(t),) for t in order])
    assert np.array_equal(got, want[3:11]), ctx.kernel_name
    after, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(after, before)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_shutter_averages_box_filtered_slices(backend):
    w, h, k, n = COMPOSED_W, COMPOSED_H, 2, 16
    frames, order, t0 = composed_case(k, n)
    want = mean([box(f, k) for f in frames])
    ctx = atlas_context(frames, backend, samples=k)
    ctx.set_params([t0])
    before, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(before, box(frames[int(t0)], k))
    got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in order])
    assert np.array_equal(got, want), ctx.kernel_name
    after, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(after, before)
    ctx.close()
