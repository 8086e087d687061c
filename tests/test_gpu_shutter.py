"""The shutter on the device (include/maray_hip.h, "shutter"): n frames of one context averaged in HBM by
maray_shutter_reduce, compared byte for byte with the integer mean (S + n/2) >> log2 n of the oracle's renders of the
substituted scenes (tests/params.py).  No tolerance anywhere."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
from test_gpu_supersample import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]
SIZE = (384, 320)        # 6 runs of 64 pixels, 10 groups of 32 rows
SMALL = (96, 80)

_want = {}


def times(a, b, n):
    return [a + (b - a) * ((2 * i + 1) / (2 * n)) for i in range(n)]


def mean(frames):
    """(S + n/2) >> log2 n, S the integer sum over the frames."""
    n = len(frames)
    assert n & (n - 1) == 0
    s = np.zeros(frames[0].shape, np.uint32)
    for f in frames:
        s += f
    return ((s + n // 2) >> (n.bit_length() - 1)).astype(np.uint8)


def textures_of(spec):
    return PR.scene_textures() if spec.get('textures') else None


def want_frame(name, values, size=SIZE):
    """The oracle's RGB8 frame, computed once for all back-ends and never written to."""
    key = (name, size, tuple('nan' if v != v else v for v in values))
    if key not in _want:
        spec = PR.SCENES[name](*size)
        f = PR.oracle_frame(spec, size, values, textures_of(spec), want_f64=False)[0]
        f.setflags(write=False)
        _want[key] = f
    return _want[key]


def want_mean(name, rows, size=SIZE):
    return mean([want_frame(name, r, size) for r in rows])


def context(name, backend, size=SIZE, **kw):
    spec = PR.SCENES[name](*size)
    scene, names = PR.declared(spec, size)
    tape = scene.lower()
    return M.Context(tape, textures=textures_of(spec), backend=backend, **kw), tape


def slide_rows(n, size):
    return list(zip(times(-20, 60, n), times(5, -35, n))) if size == SIZE else list(zip(times(-6, 18, n), times(2, -10, n)))


# ---- 1, 2. shapes crossing guard borders; groups and accumulators ----------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('size,n', [(SIZE, 2), (SIZE, 4), (SIZE, 8), (SMALL, 16), (SMALL, 32), (SMALL, 64)])
def test_slide_equals_the_mean_of_the_oracles_frames(size, n, backend):
    """n <= 8 at 384 x 320: one pass of the reduce, shapes crossing 64-pixel and 32-row guard borders between frames.
    n > 8 at 96 x 80: groups of 8 through 16-bit partial sums."""
    w, h = size
    rows = slide_rows(n, size)
    assert len(set(rows)) == n
    ctx, tape = context('slide', backend, size)
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, want_mean('slide', rows, size)), (n, ctx.kernel_name)
    ctx.close()


# ---- 3. the largest sum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_largest_sum(backend):
    """R is 255 in all 64 frames: S = 16320 on every pixel, the most a 16-bit field ever holds; B is 0 from a NaN parameter."""
    w, h = SMALL
    rows = list(zip(times(255, 600, 64), times(-1, 3, 64), [math.nan] * 64))
    ctx, tape = context('three', backend, SMALL)
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert (got[..., 0] == 255).all() and (got[..., 2] == 0).all()
    assert np.array_equal(got, want_mean('three', rows, SMALL)), ctx.kernel_name
    ctx.close()


# ---- 4. one case per parameter kind ------------------------------------------------------------------------------------
KINDS = [('phase', [(v,) for v in times(-3, 3, 8)]),
         ('phase_inf', [(0.0,), (2.0 ** 40,), (math.inf,), (math.nan,)]),
         ('fade', [(v,) for v in times(0, 1, 16)]),
         ('grow', [(v,) for v in times(0, 64, 8)]),
         ('texshift', [(v,) for v in times(-16, 16, 4)]),
         ('in_let', [(v,) for v in times(-8, 8, 2)])]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,rows', KINDS, ids=[k[0] for k in KINDS])
def test_parameter_kinds(name, rows, backend):
    """phase_inf on the specialised kernels defers tiles to the interpreter behind the context, which must render every
    frame with that frame's values."""
    w, h = SIZE
    ctx, tape = context(name, backend)
    assert tape.param_count == 1
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, want_mean(name, rows)), (name, ctx.kernel_name)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_program_without_parameters_renders_the_plain_picture(backend):
    w, h = SIZE
    ctx, tape = context('unused', backend)
    assert tape.param_count == 0
    got = ctx.render_rows_shutter(w, h, 0, h, 4)
    assert np.array_equal(got, want_frame('unused', (0.5,)))
    got = ctx.render_rows_shutter(w, h, 0, h, np.zeros((4, 0)))
    assert np.array_equal(got, want_frame('unused', (0.5,)))
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows_shutter(w, h, 0, h, [(0.5,)] * 4)             # a wrong column count
    assert e.value.code == -1
    ctx.close()


# ---- 5. identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_identities(backend):
    w, h = SMALL
    rows = slide_rows(16, SMALL)
    ctx, tape = context('slide', backend, SMALL)
    assert np.array_equal(ctx.render_rows_shutter(w, h, 0, h, rows[:1]), want_frame('slide', rows[0], SMALL))
    assert np.array_equal(ctx.render_rows_shutter(w, h, 0, h, [rows[3]] * 64), want_frame('slide', rows[3], SMALL))
    ctx.close()


# ---- 6. state and refusal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_state_and_refusal(backend):
    w, h = SMALL
    rows = slide_rows(16, SMALL)
    v = rows[15]
    ctx, tape = context('slide', backend, SMALL)
    ctx.set_params(list(v))
    got = ctx.render_rows_shutter(w, h, 0, h, rows[:8])
    assert np.array_equal(got, want_mean('slide', rows[:8], SMALL))
    assert np.array_equal(ctx.render_rows(w, h, 0, h, want_f64=False)[0], want_frame('slide', v, SMALL))
    # frame 5 of 8 outside the range: refused before anything is enqueued
    bad = list(rows[:8])
    bad[5] = (600.0, 0.0)
    out = np.full((h, w, 3), 0xA5, np.uint8)
    for frames in (bad, rows[:3], [rows[0]] * 128, [(1.0,)] * 4, [(1.0, 2.0, 3.0)] * 4):
        with pytest.raises(M.MarayError) as e:
            ctx.render_rows_shutter(w, h, 0, h, frames, out=out)
        assert e.value.code == -1, frames
        assert (out == 0xA5).all()
    assert np.array_equal(ctx.render_rows(w, h, 0, h, want_f64=False)[0], want_frame('slide', v, SMALL))
    with pytest.raises(M.MarayError) as e:                         # no f64 planes, no rows outside the image
        ctx.render_rows_shutter(w, h, 0, h + 1, rows[:2])
    assert e.value.code == -1
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_context_whose_values_were_never_set(backend):
    """A shutter call needs no set_params (its rows are all it needs) and does not count as one."""
    w, h = SIZE
    rows = KINDS[0][1]
    ctx, tape = context('phase', backend)
    assert np.array_equal(ctx.render_rows_shutter(w, h, 0, h, rows), want_mean('phase', rows))
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows(w, h, 0, 8)
    assert e.value.code == -1
    ctx.close()


# ---- 7. geometry -------------------------------------------------------------------------------------------------------
def device_mean(ctx, w, h, rows):
    """The numpy mean of the context's own plain renders of each row of values."""
    frames = []
    for r in rows:
        ctx.set_params(list(r))
        frames.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
    return mean(frames)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('size', [(1, 33), (3, 33), (67, 41), (257, 33)])
def test_ragged_widths_single_rows_and_y0(size, backend):
    w, h = size
    rows = list(zip(times(-5, 9, 4), times(2, -6, 4)))
    ctx, tape = context('slide', backend, size)
    want = device_mean(ctx, w, h, rows)
    for y0, y1 in ((0, h), (0, 1), (5, 6), (17, 30), (h - 1, h)):
        got = ctx.render_rows_shutter(w, h, y0, y1, rows)
        assert np.array_equal(got, want[y0:y1]), (size, y0, y1, ctx.kernel_name)
    img = np.full((h, w, 3), 0xA5, np.uint8)
    ctx.render_tiles_shutter(w, h, [(17, 30), (0, 5)], rows, img)
    assert np.array_equal(img[17:30], want[17:30]) and np.array_equal(img[:5], want[:5])
    assert (img[5:17] == 0xA5).all() and (img[30:] == 0xA5).all()
    ctx.close()


@pytest.mark.parametrize('backend', [M.BACKEND_TAPE_SMEM, M.BACKEND_JIT])
def test_a_raster_larger_than_one_pass_of_the_reduce(backend):
    """The reduce's grid is at most 2048 blocks of 256 lanes of 16 bytes: 8 MiB a pass.  2048 x 1400 x 3 bytes as ONE tile
    (8.2 MiB) makes every lane stride; n = 16 takes the partial sums through it too.  The only test above a megapixel."""
    w, h = 2048, 1400
    assert w * h * 3 > 2048 * 256 * 16
    rows = list(zip(times(-200, 500, 16), times(50, -350, 16)))
    ctx, tape = context('slide', backend, (w, h))
    frames = []
    for r in rows:
        ctx.set_params(list(r))
        frames.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
    for n, pick in ((2, [3, 12]), (16, list(range(16)))):
        img = np.zeros((h, w, 3), np.uint8)
        ctx.render_tiles_shutter(w, h, [(0, h)], [rows[i] for i in pick], img)
        assert np.array_equal(img, mean([frames[i] for i in pick])), (n, ctx.kernel_name)
    ctx.close()


# ---- 8. device pointers ------------------------------------------------------------------------------------------------
_DEVICE = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_gpu_shutter import context, device_mean, mean, times
FILL = 0xA5
w, h = 67, 41
A = list(zip(times(-5, 9, 16), times(2, -6, 16)))
B = list(zip(times(20, -12, 16), times(-9, 3, 16)))
v = (3.0, 33.0)
for backend in (M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
    ctx, tape = context('slide', backend, (w, h))
    want = {}
    for n in (2, 8, 16):
        want['A', n] = device_mean(ctx, w, h, A[:n]); want['B', n] = device_mean(ctx, w, h, B[:n])
    ctx.set_params(list(v))
    plain = ctx.render_rows(w, h, 0, h, want_f64=False)[0]
    # guard bands; PAD = 64 rows of 201 bytes is a multiple of 16, PAD = 65 leaves the destination at 9 modulo 16
    for PAD in (64, 65):
        for n in (2, 8, 16):
            for y0, y1 in ((0, h), (5, 6), (17, 30)):
                rows = y1 - y0
                b8 = torch.full((rows + 2 * PAD, w, 3), FILL, dtype=torch.uint8, device='cuda')
                p8 = b8.data_ptr() + PAD * w * 3
                assert (p8 %% 16 != 0) == (PAD == 65)
                ctx.render_rows_shutter_device(w, h, y0, y1, A[:n], p8)
                torch.cuda.synchronize()
                assert bool((b8[:PAD] == FILL).all()) and bool((b8[PAD + rows:] == FILL).all()), ('guard band written', backend, PAD, n)
                assert np.array_equal(b8[PAD:PAD + rows].cpu().numpy(), want['A', n][y0:y1]), (backend, PAD, n, y0, y1)
    # calls in flight: the scratch is the context's, so order is all that keeps them apart.  Two on one stream, a plain
    # render between them (it keeps the set_params values), one on a second stream, then a single synchronise.
    for n in (8, 16):
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        bufs = [torch.full((h + 1, w, 3), FILL, dtype=torch.uint8, device='cuda') for _ in range(4)]
        ptr = [b.data_ptr() + 3 for b in bufs]          # misaligned by 3
        torch.cuda.synchronize()
        ctx.render_rows_shutter_device(w, h, 0, h, A[:n], ptr[0], stream=s1.cuda_stream)
        ctx.render_rows_device(w, h, 0, h, d_rgb8=ptr[1], stream=s1.cuda_stream)
        ctx.render_rows_shutter_device(w, h, 0, h, B[:n], ptr[2], stream=s1.cuda_stream)
        ctx.render_rows_shutter_device(w, h, 0, h, A[:2], ptr[3], stream=s2.cuda_stream)
        torch.cuda.synchronize()
        got = [b.cpu().numpy().reshape(-1) for b in bufs]
        for g, wnt in zip(got, (want['A', n], plain, want['B', n], want['A', 2])):
            assert (g[:3] == FILL).all() and (g[3 + wnt.size:] == FILL).all(), (backend, n)
            assert np.array_equal(g[3:3 + wnt.size], wnt.reshape(-1)), (backend, n)
    ctx.close()
print('ok')
"""


def test_device_pointers_guard_bands_and_calls_in_flight():
    """render_rows_shutter_device into misaligned buffers with guard bands, and several calls enqueued before one
    synchronise (a process of its own: the device buffers come from PyTorch, imported before the library)."""
    code = _DEVICE % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- 9. with supersampling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_supersampled_frames(backend):
    """samples = 2: every frame is the box-filtered one, then the temporal mean."""
    from marayb import encode
    from oracle_ffi import Scene as OScene
    w, h = SMALL
    k = 2
    rows = slide_rows(4, SMALL)
    spec = PR.SCENES['slide'](w, h)
    key = ('slide ss', k, tuple(rows))
    if key not in _want:
        frames = []
        for values in rows:
            plain = M.Scene(encode((w, h), PR.substituted(spec['color'], ['t', 'u'], values)))
            plain.supersample(k)
            frames.append(box(OScene(plain.encode()).render_rows(k * w, k * h, 0, k * h, want_f64=False)[0], k))
        _want[key] = mean(frames)
    scene, names = PR.declared(spec, (w, h))
    scene.supersample(k)
    ctx = M.Context(scene.lower(), backend=backend, samples=k)
    got = ctx.render_rows_shutter(w, h, 0, h, rows)
    assert np.array_equal(got, _want[key]), ctx.kernel_name
    ctx.close()


# ---- 10. façade --------------------------------------------------------------------------------------------------------
def facade_case():
    spec = PR.SCENES['slide'](*SIZE)
    scene, names = PR.declared(spec, SIZE)
    scene.set_param('t', 20.0)
    scene.set_param('u', -15.0)
    scene.set_param_span('t', 80.0)
    scene.set_param_span('u', 40.0)
    rows = [tuple(r) for r in scene.shutter_values(4)]
    assert rows == [(-10.0, -30.0), (10.0, -20.0), (30.0, -10.0), (50.0, 0.0)]
    return want_mean('slide', rows), want_frame('slide', (20.0, -15.0))


@pytest.mark.parametrize('backend', [M.BACKEND_AUTO, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT])
def test_gen_to_image(backend):
    blurred, sharp = facade_case()
    M.gen_cache_clear()
    scene, names = PR.declared(PR.SCENES['slide'](*SIZE), SIZE)
    for shutter, want in ((4, blurred), (0, sharp), (4, blurred), (1, sharp)):
        img = M.gen_to_image(scene, backend=backend, n_devices=1, shutter=shutter, spans={'t': 80.0, 'u': 40.0}, params={'t': 20.0, 'u': -15.0})
        assert np.array_equal(img, want), shutter
    assert scene.size == SIZE and scene.param_info(0)[3] == 20.0 and scene.param_info(1)[3] == -15.0
    assert len(M.gen_cache_info()) == 1, M.gen_cache_info()
    img = M.gen_to_image(scene, backend=backend, n_devices=1, shutter=4, spans={'t': 0.0, 'u': 0.0})
    assert np.array_equal(img, sharp)
    assert len(M.gen_cache_info()) == 1, M.gen_cache_info()
    with pytest.raises(M.MarayError) as e:
        M.gen_to_image(scene, backend=backend, n_devices=1, shutter=3)
    assert e.value.code == -1
    M.gen_cache_clear()


def test_gen_to_image_on_two_workers():
    blurred, sharp = facade_case()
    old = os.environ.get('MARAY_GEN_WRAP_DEVICES')
    os.environ['MARAY_GEN_WRAP_DEVICES'] = '1'
    try:
        M.gen_cache_clear()
        scene, names = PR.declared(PR.SCENES['slide'](*SIZE), SIZE)
        for shutter, want in ((4, blurred), (1, sharp), (4, blurred)):
            img = M.gen_to_image(scene, n_devices=2, tile_rows=16, shutter=shutter, spans={'t': 80.0, 'u': 40.0}, params={'t': 20.0, 'u': -15.0})
            assert np.array_equal(img, want), shutter
    finally:
        if old is None:
            del os.environ['MARAY_GEN_WRAP_DEVICES']
        else:
            os.environ['MARAY_GEN_WRAP_DEVICES'] = old
        M.gen_cache_clear()


def test_cli_writes_the_pixels_of_gen_to_image(tmp_path):
    blurred, sharp = facade_case()
    scene, names = PR.declared(PR.SCENES['slide'](*SIZE), SIZE)
    path = tmp_path / 'slide.maray'
    scene.save(str(path))
    out = tmp_path / 'out.png'
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '-i', str(path), '-p', 't=20:-512:512', '-p', 'u=-15:-512:512',
                        '--shutter', 't=80', '--shutter', 'u=40', '--shutter-samples', '4', '-o', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = M.gen_to_image(scene, shutter=4, spans={'t': 80.0, 'u': 40.0}, params={'t': 20.0, 'u': -15.0})
    assert np.array_equal(want, blurred)
    assert np.array_equal(M.png_read(str(out)), want)
    M.gen_cache_clear()
