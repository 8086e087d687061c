"""Scene parameters on the device (include/maray_hip.h, "scene parameters"): every frame of a sweep rendered by ONE
context per back-end, compared with the oracle's render of the substituted scene on every pixel, bit for bit (tests/params.py).
No tolerance anywhere."""
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
SIZE = (384, 320)        # 6 runs of 64 pixels, 10 groups of 32 rows: the sweeps move shapes across both kinds of border

_want = {}


def want_frame(name, values, size=SIZE):
    key = (name, size, tuple('nan' if v != v else v for v in values))
    if key not in _want:
        spec = PR.SCENES[name](*size)
        _want[key] = PR.oracle_frame(spec, size, values, PR.scene_textures() if spec.get('textures') else None)
    return _want[key]


def setup(name, size=SIZE):
    spec = PR.SCENES[name](*size)
    scene, names = PR.declared(spec, size)
    return spec, scene, PR.scene_textures() if spec.get('textures') else None


def set_values(ctx, tape, values):
    if tape.param_count:
        ctx.set_params(list(values))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', sorted(PR.SCENES))
def test_every_frame_of_a_sweep_on_one_context(name, backend):
    """v0, v1, ..., then v0 again, on one context: every frame is the oracle's image of the substituted scene (RGB8 and the
    f64 planes), and the last equals the first.  One frame is launched twice in a row -- a geometry's second launch with
    unchanged values is what computes the specialised kernels' launch order -- so the frames after it walk a cached order
    and guard bits of other values."""
    spec, scene, tex = setup(name)
    tape = scene.lower()
    assert tape.param_count == (0 if name == 'unused' else len(spec['params']))
    w, h = SIZE
    ctx = M.Context(tape, textures=tex, backend=backend)
    assert ctx.param_count == tape.param_count
    frames = list(spec['sweep']) + [spec['sweep'][0]]
    first = None
    for k, values in enumerate(frames):
        set_values(ctx, tape, values)
        for again in range(2 if k == 1 else 1):
            got8, got64 = ctx.render_rows(w, h, 0, h)
            want8, want64 = want_frame(name, values)
            assert np.array_equal(got8, want8), (name, values, ctx.kernel_name, again)
            assert PR.same_f64(got64, want64), (name, values, ctx.kernel_name, again)
        if first is None:
            first = got8.copy()
    assert np.array_equal(got8, first)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_unused_parameters_take_no_values(backend):
    spec, scene, tex = setup('unused')
    tape = scene.lower()
    assert tape.program.version == 2 and tape.param_count == 0
    ctx = M.Context(tape, backend=backend)
    ctx.set_params([])
    with pytest.raises(M.MarayError) as e:
        ctx.set_params([0.5])
    assert e.value.code == -1
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_context_enforces_the_ranges(backend):
    """A value outside the range, NaN into a finite range, a wrong count: MARAY_E_ARG, and the old values stay."""
    spec, scene, tex = setup('phase')
    tape = scene.lower()
    w, h = SIZE
    ctx = M.Context(tape, backend=backend)
    with pytest.raises(M.MarayError) as e:      # a finite range excludes NaN, the initial value: nothing renders before a set_params
        ctx.render_rows(w, h, 0, 8)
    assert e.value.code == -1
    ctx.set_params([1.5])
    for bad in ([64.5], [math.nan], [-math.inf], [1.0, 2.0], []):
        with pytest.raises(M.MarayError) as e:
            ctx.set_params(bad)
        assert e.value.code == -1, bad
    got8, got64 = ctx.render_rows(w, h, 0, h)
    want8, want64 = want_frame('phase', (1.5,))
    assert np.array_equal(got8, want8) and PR.same_f64(got64, want64)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_time_rows_after_set_params_then_render(backend):
    """time_rows launches without a ROW pass; after a set_params its first launch must run one all the same, and a render
    after it shows the new values' picture."""
    spec, scene, tex = setup('slide')
    tape = scene.lower()
    w, h = SIZE
    ctx = M.Context(tape, backend=backend)
    ctx.set_params([0.0, 0.0])
    ctx.time_rows(w, h, 0, h, reps=3)
    ctx.set_params([100.0, 70.0])
    ctx.time_rows(w, h, 0, h, reps=3)
    got8, got64 = ctx.render_rows(w, h, 0, h)
    want8, want64 = want_frame('slide', (100.0, 70.0))
    assert np.array_equal(got8, want8) and PR.same_f64(got64, want64)
    ctx.close()


_DEVICE = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
import params as PR
from test_gpu_params import SIZE, setup, want_frame
w, h = SIZE
spec, scene, tex = setup('slide')
tape = scene.lower()
v0, v1, v2 = (0.0, 0.0), (100.0, 70.0), (0.5, 0.25)
for backend in (M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
    ctx = M.Context(tape, backend=backend)
    # two frames enqueued back to back on one stream before a single synchronise: each keeps its own values
    st = torch.cuda.Stream()
    a8 = torch.zeros((h, w, 3), dtype=torch.uint8, device='cuda'); a64 = torch.zeros((h, w, 3), dtype=torch.float64, device='cuda')
    b8 = torch.zeros_like(a8); b64 = torch.zeros_like(a64)
    torch.cuda.synchronize()
    ctx.set_params(list(v1))
    ctx.render_rows_device(w, h, 0, h, d_rgb8=a8.data_ptr(), d_rgb64=a64.data_ptr(), stream=st.cuda_stream)
    ctx.set_params(list(v2))
    ctx.render_rows_device(w, h, 0, h, d_rgb8=b8.data_ptr(), d_rgb64=b64.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    for (g8, g64), v in (((a8, a64), v1), ((b8, b64), v2)):
        want8, want64 = want_frame('slide', v)
        assert np.array_equal(g8.cpu().numpy(), want8), (backend, v)
        assert PR.same_f64(g64.cpu().numpy(), want64), (backend, v)
    # an interleaved share of the image in one launch (blocks of 32 rows, 64 apart), with another value
    ctx.set_params(list(v0))
    c8 = torch.zeros((5 * 32, w, 3), dtype=torch.uint8, device='cuda')
    ctx.render_blocks_device(w, h, 0, 32, 64, 5, d_rgb8=c8.data_ptr())
    torch.cuda.synchronize()
    rows = (np.arange(5)[:, None] * 64 + np.arange(32)[None, :]).reshape(-1)
    assert np.array_equal(c8.cpu().numpy(), want_frame('slide', v0)[0][rows]), backend
    ctx.close()
print('ok')
"""


def test_device_pointer_entry_points_keep_each_frames_values():
    """render_rows_device with two frames in flight on one stream, and render_blocks_device with an interleaved share (a
    process of its own: the device buffers come from PyTorch, imported before the library)."""
    code = _DEVICE % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


def test_deferred_tiles_see_the_same_values():
    """phase_inf on the specialised kernels: 2^40, +inf and NaN send tiles to the interpreter behind the context, which must
    render them with the same values (covered for every back-end by the sweep above; here the kernel is pinned)."""
    spec, scene, tex = setup('phase_inf')
    tape = scene.lower()
    assert tape.info['sin_bounded'] == 0
    w, h = SIZE
    ctx = M.Context(tape, backend=M.BACKEND_JIT)
    assert ctx.kernel_name == 'maray_jit_pixels'
    for values in ((2.0 ** 40,), (1.5,), (math.inf,), (math.nan,), (2.0 ** 40,)):
        ctx.set_params(list(values))
        got8, got64 = ctx.render_rows(w, h, 0, h)
        want8, want64 = want_frame('phase_inf', values)
        assert np.array_equal(got8, want8) and PR.same_f64(got64, want64), values
    ctx.close()


@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', ['slide', 'phase', 'fade'])
def test_supersampled_frames(name, backend, k):
    """samples = k with a parameter: the box filter of the oracle's k w x k h render of the substituted, supersampled scene."""
    from marayb import encode
    from oracle_ffi import Scene as OScene
    w, h = 96, 80
    spec = PR.SCENES[name](w, h)
    scene, names = PR.declared(spec, (w, h))
    scene.supersample(k)
    assert scene.param_count == len(names)
    tape = scene.lower()
    ctx = M.Context(tape, backend=backend, samples=k)
    for values in spec['sweep'][:4] + [spec['sweep'][0]]:
        plain = M.Scene(encode((w, h), PR.substituted(spec['color'], names, values)))
        plain.supersample(k)
        want8, _ = OScene(plain.encode()).render_rows(k * w, k * h, 0, k * h, want_f64=False)
        ctx.set_params(list(values))
        got8, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
        assert np.array_equal(got8, box(want8, k)), (name, values, ctx.kernel_name)
    ctx.close()


@pytest.mark.parametrize('backend', [M.BACKEND_AUTO, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT])
def test_gen_to_image_finds_its_program_again(backend):
    """Frames with other values: all right, and one program kept, not one per value."""
    M.gen_cache_clear()
    spec, scene, tex = setup('slide')
    for values in ((0.0, 0.0), (100.0, 70.0), (0.5, 0.25)):
        img = M.gen_to_image(scene, backend=backend, n_devices=1, params={'t': values[0], 'u': values[1]})
        assert np.array_equal(img, want_frame('slide', values)[0]), values
    info = M.gen_cache_info()
    assert len(info) == 1, info
    # a declared parameter nothing reads: the picture the scene always rendered, whatever value is set
    spec, scene, tex = setup('unused')
    img = M.gen_to_image(scene, backend=backend, n_devices=1, params={'t': 0.5})
    assert np.array_equal(img, want_frame('unused', (0.5,))[0])
    M.gen_cache_clear()


_ONE_BUILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_gpu_params import setup, want_frame
spec, scene, tex = setup('slide')
for values in ((0.0, 0.0), (100.0, 70.0), (0.5, 0.25)):
    img = M.gen_to_image(scene, backend=M.BACKEND_JIT, n_devices=1, params={'t': values[0], 'u': values[1]})
    assert np.array_equal(img, want_frame('slide', values)[0]), values
info = M.gen_cache_info()
assert len(info) == 1 and ' kernel maray_jit_pixels ' in info[0], info
print(' '.join(sorted(os.listdir(os.environ['MARAY_CACHE_DIR']))))
"""


def test_one_set_of_code_objects_for_every_value(tmp_path):
    """In a fresh process and a fresh MARAY_CACHE_DIR: three frames with three values leave exactly one <key> set of code
    objects (and the one remembered key of the one program)."""
    code = _ONE_BUILD % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900, env=dict(os.environ, MARAY_CACHE_DIR=str(tmp_path)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = r.stdout.strip().splitlines()[-1].split()
    assert len([f for f in files if f.endswith('.mrco')]) == 1 and len([f for f in files if f.endswith('.key')]) == 1, files


def test_gen_to_image_on_two_devices():
    if M.device_count() < 2:
        pytest.skip('needs a second GPU')
    M.gen_cache_clear()
    spec, scene, tex = setup('slide')
    for values in ((0.0, 0.0), (100.0, 70.0)):
        img = M.gen_to_image(scene, n_devices=2, tile_rows=32, params={'t': values[0], 'u': values[1]})
        assert np.array_equal(img, want_frame('slide', values)[0]), values
    assert len({line.split()[0] for line in M.gen_cache_info()}) == 1
    M.gen_cache_clear()
