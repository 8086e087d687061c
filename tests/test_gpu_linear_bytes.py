"""The reduces in linear light (include/maray_hip.h, "transfer") on the device: maray_filter_box_lin<K>, maray_filter_tent_lin<K>
and maray_shutter_reduce_lin against the numpy contracts of tests/linear_light.py, byte for byte, never with a tolerance.

The scenes are the texture-identity and atlas scenes of tests/byte_rasters.py: the sample raster and the frames are whatever
bytes a test chooses.  That those bytes tell the contracts' mutants apart is checked without a device in
tests/test_linear_light.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import linear_light as LL
import maray_amd as M
import png_stream as P
from test_filter import tent
from test_gpu_filter import band_rows
from test_gpu_shutter import mean
from test_gpu_supersample import BACKENDS, box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRGB = M.TRANSFER_SRGB
FILTERS = [(M.FILTER_BOX, LL.box_lin, 'box'), (M.FILTER_TENT, LL.tent_lin, 'tent')]

_tapes = {}


def identity_tape():
    if 'identity' not in _tapes:
        _tapes['identity'] = BR.identity_scene().lower()
    return _tapes['identity']


def atlas_tape():
    if 'atlas' not in _tapes:
        _tapes['atlas'] = BR.atlas_scene().lower()
    return _tapes['atlas']


def lin_context(s8, k, filt, backend=M.BACKEND_TAPE_SMEM, transfer=SRGB):
    return M.Context(identity_tape(), textures=[s8], backend=backend, samples=k, filter=filt, transfer=transfer)


def atlas_context(frames, backend=M.BACKEND_TAPE_SMEM, **kw):
    return M.Context(atlas_tape(), textures=[BR.atlas(frames)], backend=backend, **kw)


def rendered(s8, k, filt, **kw):
    H, W, _ = s8.shape
    ctx = lin_context(s8, k, filt, **kw)
    got, _ = ctx.render_rows(W // k, H // k, 0, H // k, want_f64=False)
    ctx.close()
    return got


# ---- box and tent --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
def test_parity_raster_on_every_back_end(backend, k):
    """65 x 37 pixels of random bytes, box and tent, on all three back-ends; and the names."""
    s8 = BR.parity_raster(k)
    for filt, contract, name in FILTERS:
        ctx = lin_context(s8, k, filt, backend)
        assert ctx.kernel_name.endswith('+maray_filter_%s_lin<%d>' % (name, k)), ctx.kernel_name
        got, _ = ctx.render_rows(BR.PARITY_W, BR.PARITY_H, 0, BR.PARITY_H, want_f64=False)
        ctx.close()
        assert np.array_equal(got, contract(s8, k)), name


@pytest.mark.parametrize('k', [2, 4, 8])
def test_extremes_and_critical_sums(k):
    """All 0, all 255 (the largest sums: 24-bit horizontal ones), the checker (188 in linear light), impulses; and the raster
    whose cells sit on the rounding step's critical sums at a threshold, and the one whose footprints sit on the tent's."""
    w, h = BR.EXTREMES_W, BR.EXTREMES_H
    for filt, contract, fname in FILTERS:
        for name, s8 in BR.extreme_rasters(h, w, k) + [('critical', LL.critical_raster(k)), ('critical tent', LL.critical_tent_raster(k))]:
            got = rendered(s8, k, filt)
            assert np.array_equal(got, contract(s8, k)), (fname, name)
            if name == 'checker':
                assert (got[1:-1, 1:-1] == 188).all()


def test_threshold_rasters():
    """Every threshold of the encoder, on it and one below it (k = 2; at k = 4 the ones below that four samples cannot reach)."""
    s8 = LL.threshold_box_raster()
    assert np.array_equal(rendered(s8, 2, M.FILTER_BOX), LL.box_lin(s8, 2))
    s8 = LL.threshold_box_raster_k4()
    assert np.array_equal(rendered(s8, 4, M.FILTER_BOX), LL.box_lin(s8, 4))
    s8 = LL.threshold_tent_raster()
    assert np.array_equal(rendered(s8, 2, M.FILTER_TENT), LL.tent_lin(s8, 2))
    assert np.array_equal(rendered(s8, 2, M.FILTER_BOX), LL.box_lin(s8, 2))


@pytest.mark.parametrize('k', [2, 4, 8])
def test_widths_bands_and_row_ranges(k):
    """Widths 1 .. 129 at height 19; MARAY_FILTER_BAND_ROWS of one row, one tile and everything give equal pictures, whole and
    by row ranges (the environment is read when a context is created)."""
    h = BR.GEOMETRY_H
    for w in BR.GEOMETRY_WS:
        s8 = BR.geometry_raster(k, w)
        for filt, contract, name in FILTERS:
            want = contract(s8, k)
            for rows in ((1, 8, 1000) if w in (5, 65) else (8, 1000)):
                with band_rows(rows):
                    ctx = lin_context(s8, k, filt)
                got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
                assert np.array_equal(got, want), (name, w, rows)
                for y0, y1 in ((0, 1), (5, 6), (7, 16), (h - 1, h)):
                    got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
                    assert np.array_equal(got, want[y0:y1]), (name, w, rows, y0, y1)
                ctx.close()


_DESTINATIONS = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import linear_light as LL
import maray_amd as M
PAD, FILL = 256, 0xA5
h = BR.DESTINATION_H
tape = BR.identity_scene().lower()
for k in BR.DESTINATION_KS:
    for w in BR.DESTINATION_WS:
        s8 = BR.destination_raster(k, w)
        for filt, contract in ((M.FILTER_BOX, LL.box_lin), (M.FILTER_TENT, LL.tent_lin)):
            want = contract(s8, k)
            ctx = M.Context(tape, textures=[s8], backend=M.BACKEND_TAPE_SMEM, samples=k, filter=filt, transfer=M.TRANSFER_SRGB)
            for g in (('rows', 0, h), ('rows', 7, 8), ('blocks', 2, 3, 5, 4)):
                n = g[2] - g[1] if g[0] == 'rows' else g[2] * g[4]
                rows = np.arange(g[1], g[2]) if g[0] == 'rows' else (g[1] + np.arange(g[4])[:, None] * g[3] + np.arange(g[2])[None, :]).reshape(-1)
                for off in (0, 1):
                    b8 = torch.full((n * w * 3 + 2 * PAD,), FILL, dtype=torch.uint8, device='cuda')
                    lo = PAD + off
                    p8 = b8.data_ptr() + lo
                    assert p8 %% 2 == off
                    if g[0] == 'rows':
                        ctx.render_rows_device(w, h, g[1], g[2], d_rgb8=p8)
                    else:
                        ctx.render_blocks_device(w, h, *g[1:], d_rgb8=p8)
                    torch.cuda.synchronize()
                    assert bool((b8[:lo] == FILL).all()) and bool((b8[lo + n * w * 3:] == FILL).all()), ('guard band written', k, w, filt, g, off)
                    assert np.array_equal(b8[lo:lo + n * w * 3].cpu().numpy().reshape(n, w, 3), want[rows]), (k, w, filt, g, off)
            ctx.close()
print('ok')
"""


def test_destinations_at_an_even_and_an_odd_address():
    """Device destinations with guard bytes on both sides, rows and row blocks, w = 1, 5, 64, 65 and k = 2, 8 (a process of its
    own: the device buffers come from PyTorch, imported before the library)."""
    code = _DESTINATIONS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- shutter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', BR.SHUTTER_NS)
def test_random_frames_equal_their_linear_mean(n):
    """n random frames of 67 x 41 with their rows shuffled, whole and by row ranges; the frames on the critical sums."""
    w, h = BR.SHUTTER_W, BR.SHUTTER_H
    frames, order = BR.shutter_case(n)
    want = LL.mean_lin(frames)
    rows = [(float(t),) for t in order]
    ctx = atlas_context(frames, transfer=SRGB)
    assert ctx.kernel_name.endswith('+maray_shutter_reduce_lin'), ctx.kernel_name
    assert np.array_equal(ctx.render_rows_shutter(w, h, 0, h, rows), want)
    for y0, y1 in ((5, 6), (17, 30)):
        assert np.array_equal(ctx.render_rows_shutter(w, h, y0, y1, rows), want[y0:y1]), (y0, y1)
    ctx.close()
    crit = LL.critical_frames(n)
    ctx = atlas_context(crit, transfer=SRGB)
    cw = crit[0].shape[1]
    assert np.array_equal(ctx.render_rows_shutter(cw, 1, 0, 1, [(float(t),) for t in range(n)]), LL.mean_lin(crit))
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_shutter_extremes_and_thresholds_on_every_back_end(backend):
    """Frames alternating 0 / 255 give 188; 64 frames of 255 give 255 (the largest sum, 22 bits); the threshold frames."""
    w, h = 7, 5
    for n in (2, 16, 64):
        frames = [BR.constant(255 * (i & 1), h, w) for i in range(n)]
        ctx = atlas_context(frames, backend, transfer=SRGB)
        got = ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in range(n)])
        ctx.close()
        assert (got == 188).all(), n
    frames = [BR.constant(255, h, w)] * 64
    ctx = atlas_context(frames, backend, transfer=SRGB)
    assert (ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in range(64)]) == 255).all()
    ctx.close()
    for n in (2, 4):
        frames = LL.threshold_frames(n)
        fh, fw, _ = frames[0].shape
        ctx = atlas_context(frames, backend, transfer=SRGB)
        got = ctx.render_rows_shutter(fw, fh, 0, fh, [(float(t),) for t in range(n)])
        ctx.close()
        assert np.array_equal(got, LL.mean_lin(frames)), n


_HEAD_TAIL = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import byte_rasters as BR
import linear_light as LL
import maray_amd as M
PAD, FILL = 64, 0xA5
h = BR.HEAD_TAIL_ROWS[-1]
tape = BR.atlas_scene().lower()
b8 = torch.empty((2 * PAD + 16 + h * BR.HEAD_TAIL_WS[-1] * 3,), dtype=torch.uint8, device='cuda')
assert b8.data_ptr() %% 16 == 0
for n in BR.HEAD_TAIL_NS:
    frames, order = BR.head_tail_case(n)
    values = [(float(t),) for t in order]
    ctx = M.Context(tape, textures=[BR.atlas(frames)], backend=M.BACKEND_TAPE_SMEM, transfer=M.TRANSFER_SRGB)
    for w in BR.HEAD_TAIL_WS:
        for rows in BR.HEAD_TAIL_ROWS:
            size = rows * w * 3
            want = LL.mean_lin([f[:rows, :w] for f in frames]).reshape(-1)
            for mis in (0, 1, 7, 15):
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


def test_head_tail_sizes_and_destination_misalignments():
    """Rasters of 3 .. 105 bytes at destination misalignments 0, 1, 7, 15 for n = 2, 8, 16, 64, guard bytes on both sides."""
    code = _HEAD_TAIL % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- composition, default and identity -------------------------------------------------------------------------------------
@pytest.mark.parametrize('filt,contract,name', FILTERS)
def test_shutter_on_a_filtered_context_decodes_the_filtered_bytes(filt, contract, name):
    """Frame i is exactly the RGB8 the context renders; those bytes are decoded, averaged and encoded again."""
    w, h, k, n = 21, 13, 2, 16
    frames = BR.random_frames(6100 + n, n, k * h, k * w)
    order = [int(i) for i in np.random.default_rng(7100).permutation(n)]
    want = LL.mean_lin([contract(f, k) for f in frames])
    with band_rows(5):
        ctx = atlas_context(frames, samples=k, filter=filt, transfer=SRGB)
    ctx.set_params([3.0])
    before, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(before, contract(frames[3], k))
    assert np.array_equal(ctx.render_rows_shutter(w, h, 0, h, [(float(t),) for t in order]), want)
    assert np.array_equal(ctx.render_rows_shutter(w, h, 3, 11, [(float(t),) for t in order]), want[3:11])
    after, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert np.array_equal(after, before)
    ctx.close()


def test_nothing_to_reduce_is_the_plain_render_and_none_is_todays_reduce():
    """transfer=SRGB with samples <= 1 and no shutter: the plain bytes (and the f64 planes); transfer=NONE: today's box, tent and
    shutter, named as today."""
    s8 = BR.parity_raster(2)
    H, W, _ = s8.shape
    for samples in (0, 1):
        ctx = lin_context(s8, samples, M.FILTER_BOX)
        got8, got64 = ctx.render_rows(W, H, 0, H)
        ctx.close()
        assert np.array_equal(got8, s8) and np.array_equal(got64, s8.astype(np.float64))
    assert np.array_equal(rendered(s8, 2, M.FILTER_BOX, transfer=M.TRANSFER_NONE), box(s8, 2))
    assert np.array_equal(rendered(s8, 2, M.FILTER_TENT, transfer=M.TRANSFER_NONE), tent(s8, 2))
    ctx = lin_context(s8, 2, M.FILTER_BOX, transfer=M.TRANSFER_NONE)
    assert '+' not in ctx.kernel_name
    ctx.close()
    frames, order = BR.shutter_case(16)
    ctx = atlas_context(frames, transfer=M.TRANSFER_NONE)
    assert '+' not in ctx.kernel_name
    got = ctx.render_rows_shutter(BR.SHUTTER_W, BR.SHUTTER_H, 0, BR.SHUTTER_H, [(float(t),) for t in order])
    ctx.close()
    assert np.array_equal(got, mean(frames)) and not np.array_equal(got, LL.mean_lin(frames))
    with pytest.raises(M.MarayError) as e:
        lin_context(s8, 2, M.FILTER_BOX).render_rows(W // 2, H // 2, 0, 1, want_u8=False)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        lin_context(s8, 2, M.FILTER_BOX, transfer=2)
    assert e.value.code == -1


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _chess():
    return M.Scene(open(os.path.join(HERE, 'golden', 'chess.maray'), 'rb').read())


def test_gen_to_image_chess_is_the_contract_of_its_sample_raster():
    """chess at 256^2 with 4 x 4 samples on one device: box and tent in linear light are the numpy contracts applied to the plain
    render of the supersampled scene; the cache lines and keys say which program is which.  (The top left 256^2 of the fixture
    is sky, where linear and byte means agree: this test is about the facade -- programs, keys, contexts per (k, filter,
    transfer).  The picture that tells the two means apart is the board in test_cli_linear_... below.)"""
    n, k = 256, 4
    M.gen_cache_clear()
    ss = _chess()
    ss.supersample(k)
    samples = M.gen_to_image(ss, size=(k * n, k * n), n_devices=1)
    for filt, contract, name in FILTERS:
        got = M.gen_to_image(_chess(), size=(n, n), n_devices=1, samples=k, filter=filt, transfer=SRGB)
        assert np.array_equal(got, contract(samples, k)), name
        plain = M.gen_to_image(_chess(), size=(n, n), n_devices=1, samples=k, filter=filt)
        assert np.array_equal(plain, (box if filt == M.FILTER_BOX else tent)(samples, k))       # (kept side by side, under its own key)
    lines = M.gen_cache_info()
    srgb = [l for l in lines if l.endswith(' transfer srgb')]
    assert len(srgb) == 2 and all('/srgb ' in l and '_lin<4>' in l and ' samples 4' in l for l in srgb), lines
    assert sum(' filter tent transfer srgb' in l for l in srgb) == 1
    assert all('/srgb' not in l and '_lin' not in l for l in lines if l not in srgb)
    M.gen_cache_clear()


def test_gen_with_the_device_encoder_and_render_png_decode_to_the_same_raster(tmp_path):
    n, k = 128, 2
    M.gen_cache_clear()
    scene = _chess()
    scene.set_size(n, n)
    want = M.gen_to_image(_chess(), size=(n, n), n_devices=1, samples=k, transfer=SRGB)
    path = str(tmp_path / 'lin.png')
    M.gen(scene, path, n_devices=1, samples=k, transfer=SRGB, encoder=M.ENCODER_DEVICE)
    assert np.array_equal(M.png_read(path), want)
    ss = _chess()
    ss.supersample(k)
    ctx = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM, samples=k, transfer=SRGB)
    png = ctx.render_png(n, n)
    ctx.close()
    assert np.array_equal(P.decode(png), want)
    M.gen_cache_clear()


def test_cli_linear_writes_the_contract_of_its_sample_raster(tmp_path):
    """maray -s 8 --linear -i tests/golden/chess.maray at the fixture's own 1024^2: the file's rows 512 .. 575, the far rows of
    the board below the horizon, are box_lin of their 512 x 8192 sample rows (the box has no halo; the whole 8192^2 sample raster
    is too much for numpy in a test) and not the box mean of the bytes; sky rows 0 .. 7 are box_lin of theirs too.  --linear alone
    is the plain picture."""
    n, k = 1024, 8
    src, out = os.path.join(HERE, 'golden', 'chess.maray'), str(tmp_path / 'x.png')
    exe = os.path.join(ROOT, 'maray_amd', 'maray')
    r = subprocess.run([exe, '-s', str(k), '--linear', '--gpus', '1', '-i', src, '-o', out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = M.png_read(out)
    assert got.shape == (n, n, 3)
    ss = _chess()
    ss.supersample(k)
    ctx = M.Context(ss.lower(), backend=M.BACKEND_TAPE_SMEM)
    for y0, y1, differs in ((512, 576, True), (0, 8, False)):
        samples, _ = ctx.render_rows(k * n, k * n, k * y0, k * y1, want_f64=False)
        assert np.array_equal(got[y0:y1], LL.box_lin(samples, k)), (y0, y1)
        assert np.array_equal(got[y0:y1], box(samples, k)) != differs, (y0, y1)
    ctx.close()
    r = subprocess.run([exe, '--linear', '--gpus', '1', '-i', src, '-o', out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(M.png_read(out), M.gen_to_image(_chess(), n_devices=1))
