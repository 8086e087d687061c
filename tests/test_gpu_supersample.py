"""Supersampled rendering on the device (include/maray_hip.h, supersampling), compared byte for byte, never with a tolerance.

The expected image of a context with samples = k is the integer box filter (rounding half up) of the plain render of the
supersampled scene at k w x k h: from the CPU oracle on small images and on bands of rows, and at full size from the
device's own plain renders (the specialised kernels, and the interpreter on a program lowered without SKIP regions)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import scenes
from marayb import encode
from oracle_ffi import Scene as OScene
from test_gpu_launches import tri_soup

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THREADS = min(16, os.cpu_count() or 1)
BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]
SS_KERNELS = ('maray_tape_pixels_ss<', 'maray_jit_pixels_ss')


def box(samples8, k):
    """(k h, k w, 3) uint8 -> (h, w, 3): per channel (S + k^2/2) >> log2(k^2), S the integer sum of a k x k block."""
    H, W, _ = samples8.shape
    s = samples8.astype(np.uint32).reshape(H // k, k, W // k, k, 3).sum(axis=(1, 3))
    return ((s + k * k // 2) >> (2 * (k.bit_length() - 1))).astype(np.uint8)


def supersampled(data, k):
    s = M.Scene(data)
    s.supersample(k)
    return s


def chess_bytes():
    with open(os.path.join(HERE, 'golden', 'chess.maray'), 'rb') as f:
        return f.read()


def scene_case(name):
    """(bytes, w, h, textures) of the scenes compared with the oracle on every pixel."""
    if name == 'all_ops':
        return encode((67, 41), scenes.all_ops(67, 41)), 67, 41, None
    if name == 'edges':
        return encode((96, 24), scenes.shapes_through_inf_and_nan()), 96, 24, None
    if name == 'textured':
        return encode((72, 30), scenes.textured(72)), 72, 30, scenes.textures(8)
    if name == 'huge_sin':          # Step(Sin) of arguments past the fast reduction: the plain JIT kernel defers those tiles
        return encode((120, 40), tri_soup(1, [(0, 120, 0, 40, 10, 25)], 120, 40, huge_sin=True)), 120, 40, None
    assert name == 'tri_soup'
    return encode((150, 70), tri_soup(2, [(0, 150, 0, 70, 12, 30)], 150, 70)), 150, 70, None


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', ['all_ops', 'edges', 'textured', 'tri_soup', 'huge_sin'])
def test_equals_box_filter_of_the_oracle(name, backend, k):
    data, w, h, tex = scene_case(name)
    ss = supersampled(data, k)
    want8, _ = OScene(ss.encode()).render_rows(w * k, h * k, 0, h * k, textures=tex, threads=THREADS, want_f64=False)
    ctx = M.Context(ss.lower(), textures=tex, backend=backend, samples=k)
    assert ctx.kernel_name.startswith(SS_KERNELS)
    got8, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    ctx.close()
    assert np.array_equal(got8, box(want8, k))


@pytest.mark.parametrize('k', [2, 4, 8])
def test_chess_512_rows_equal_box_filter_of_the_oracle(k):
    """Chess, the left 512 columns of the stored 1024^2 scene, output rows across the board's edges (the oracle is slow on
    chess: rows, not the image)."""
    ss = supersampled(chess_bytes(), k)
    o = OScene(ss.encode())
    ctxs = [M.Context(ss.lower(), backend=b, samples=k) for b in BACKENDS]
    for y0 in (512, 700, 819):
        want8, _ = o.render_rows(512 * k, 1024 * k, y0 * k, (y0 + 1) * k, threads=THREADS, want_f64=False)
        for ctx in ctxs:
            got8, _ = ctx.render_rows(512, 1024, y0, y0 + 1, want_f64=False)
            assert np.array_equal(got8, box(want8, k)), (y0, ctx.kernel_name)
    for ctx in ctxs:
        ctx.close()


def test_chess_4096_equals_box_filter_of_a_guard_free_render():
    """Full size: chess rescaled to 4096^2, k = 4 (16384^2 samples), through the specialised kernels and the scalar-cache
    interpreter.  Every byte against the box filter of the interpreter's plain render of the same supersampled scene lowered
    without SKIP regions or row guards (a guard-free answer), in bands of 512 output rows."""
    k = 4
    s = M.Scene(chess_bytes())
    s.rescale(4, 4)
    s.supersample(k)
    tape = s.lower()
    ctxs = [M.Context(tape, backend=b, samples=k) for b in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM)]
    noskip = M.Context(s.lower(skips=False, row_guards=False), backend=M.BACKEND_TAPE_SMEM)
    for y0 in range(0, 4096, 512):
        want8, _ = noskip.render_rows(4096 * k, 4096 * k, y0 * k, (y0 + 512) * k, want_f64=False)
        want = box(want8, k)
        del want8
        for ctx in ctxs:
            got8, _ = ctx.render_rows(4096, 4096, y0, y0 + 512, want_f64=False)
            assert np.array_equal(got8, want), (y0, ctx.kernel_name)
    noskip.close()
    for ctx in ctxs:
        ctx.close()


def device_reference(data, w, h, k, tex=None):
    """The box filter of the scalar-cache interpreter's plain render of the supersampled scene (the whole image)."""
    ss = supersampled(data, k)
    plain = M.Context(ss.lower(), textures=tex, backend=M.BACKEND_TAPE_SMEM)
    want8, _ = plain.render_rows(w * k, h * k, 0, h * k, want_f64=False)
    plain.close()
    return ss, box(want8, k)


@pytest.mark.parametrize('k', [2, 4, 8])
def test_ragged_widths_single_rows_and_y0(k):
    for w in sorted({1, 3, max(1, 63 // k), 64 // k + 1, 256 // k - 1, 256 // k + 1}):
        h = 37
        data = encode((w, h), tri_soup(3, [(0, w, 0, h, 3, max(2, w // 2))], w, h)) if w >= 3 else encode((w, h), scenes.all_ops(w, h))
        ss, want = device_reference(data, w, h, k)
        for backend in BACKENDS:
            ctx = M.Context(ss.lower(), backend=backend, samples=k)
            got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
            assert np.array_equal(got, want), (w, backend)
            for y0, y1 in ((0, 1), (5, 6), (17, 30), (36, 37)):
                got, _ = ctx.render_rows(w, h, y0, y1, want_f64=False)
                assert np.array_equal(got, want[y0:y1]), (w, backend, y0, y1)
            ctx.close()


def test_output_rows_around_the_grid_split():
    """Output row counts on both sides of 65,534 at k = 2 (131,068 .. 131,072 sample rows), on a narrow image."""
    k, w, h = 2, 5, 65536
    data = encode((w, h), tri_soup(4, [(0, w, 0, h, 40, 3)], w, h))
    ss, want = device_reference(data, w, h, k)
    for backend in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM):
        ctx = M.Context(ss.lower(), backend=backend, samples=k)
        for n in (65533, 65534, 65535, 65536):
            got, _ = ctx.render_rows(w, h, h - n, h, want_f64=False)
            assert np.array_equal(got, want[h - n:]), (n, backend)
        ctx.close()


@pytest.mark.parametrize('backend', [M.BACKEND_JIT, M.BACKEND_TAPE_SMEM])
def test_repeated_and_alternating_launches_give_their_first_results(backend):
    data = encode((300, 90), tri_soup(5, [(0, 300, 0, 90, 20, 25)], 300, 90))
    s4 = supersampled(data, 4)
    plain = M.Context(M.Scene(data).lower(), backend=backend)
    aa = M.Context(s4.lower(), backend=backend, samples=4)
    first1, _ = plain.render_rows(300, 90, 0, 90, want_f64=False)
    first4, _ = aa.render_rows(300, 90, 0, 90, want_f64=False)
    assert not np.array_equal(first1, first4)
    for _ in range(3):
        for ctx, first in ((aa, first4), (plain, first1), (aa, first4)):
            got, _ = ctx.render_rows(300, 90, 0, 90, want_f64=False)
            assert np.array_equal(got, first)
    aa.close()
    plain.close()


def test_f64_planes_and_limits_are_refused():
    data = encode((67, 41), scenes.all_ops(67, 41))
    ctx = M.Context(supersampled(data, 2).lower(), backend=M.BACKEND_TAPE_SMEM, samples=2)
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows(67, 41, 0, 41, want_f64=True)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        ctx.render_rows((1 << 19) + 1, 41, 0, 1, want_f64=False)
    assert e.value.code == -7
    ctx.close()


_DEVICE_GEOMETRY = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from marayb import encode
from test_gpu_launches import tri_soup
from test_gpu_supersample import device_reference
PAD, FILL = 64, 0xA5
k, w, h = 4, 200, 96
data = encode((w, h), tri_soup(6, [(0, w, 0, h, 16, 30)], w, h))
ss, want = device_reference(data, w, h, k)
for backend in (M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
    ctx = M.Context(ss.lower(), backend=backend, samples=k)
    for g in (('rows', 0, 96), ('rows', 33, 34), ('blocks', 3, 5, 16, 6), ('blocks', 0, 8, 32, 3), ('blocks', 10, 1, 7, 12)):
        n = g[2] - g[1] if g[0] == 'rows' else g[2] * g[4]
        rows = np.arange(g[1], g[2]) if g[0] == 'rows' else (g[1] + np.arange(g[4])[:, None] * g[3] + np.arange(g[2])[None, :]).reshape(-1)
        b8 = torch.full((n + 2 * PAD, w, 3), FILL, dtype=torch.uint8, device='cuda')
        p8 = b8.data_ptr() + PAD * w * 3
        if g[0] == 'rows':
            ctx.render_rows_device(w, h, g[1], g[2], d_rgb8=p8)
        else:
            ctx.render_blocks_device(w, h, *g[1:], d_rgb8=p8)
        torch.cuda.synchronize()
        assert bool((b8[:PAD] == FILL).all()) and bool((b8[PAD + n:] == FILL).all()), ('guard band written', g)
        assert np.array_equal(b8[PAD:PAD + n].cpu().numpy(), want[rows]), (backend, g)
    ctx.close()
print('ok')
"""


def test_device_buffers_blocks_and_guard_bands():
    """render_rows_device and render_blocks_device (block_stride > block_rows) into buffers with guard bands (a process of
    its own: the device buffers come from PyTorch, imported before the library)."""
    code = _DEVICE_GEOMETRY % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


def facade_case():
    data = encode((333, 120), tri_soup(7, [(0, 333, 0, 120, 25, 40)], 333, 120))
    _, want4 = device_reference(data, 333, 120, 4)
    plain = M.Context(M.Scene(data).lower(), backend=M.BACKEND_TAPE_SMEM)
    want1, _ = plain.render_rows(333, 120, 0, 120, want_f64=False)
    plain.close()
    return data, want1, want4


@pytest.mark.parametrize('backend', [M.BACKEND_AUTO, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT])
def test_gen_to_image_keeps_programs_per_sample_count(backend):
    data, want1, want4 = facade_case()
    M.gen_cache_clear()
    s = M.Scene(data)
    for k, want in ((4, want4), (1, want1), (4, want4), (0, want1)):
        img = M.gen_to_image(s, backend=backend, samples=k, n_devices=1)
        assert np.array_equal(img, want), k
    info = M.gen_cache_info()
    assert len(info) == 2, info
    assert sum(line.endswith(' samples 4') for line in info) == 1, info
    assert sum(' samples ' not in line for line in info) == 1, info
    assert all(' kernel maray_tape_pixels_ss<' in line or ' kernel maray_jit_pixels_ss ' in line for line in info if line.endswith(' samples 4'))
    assert s.size == (333, 120)                         # the caller's scene is not supersampled
    M.gen_cache_clear()


def test_gen_to_image_on_two_workers():
    """n_devices = 2 (one worker per device, or two workers on one device when only one is visible)."""
    data, want1, want4 = facade_case()
    old = os.environ.get('MARAY_GEN_WRAP_DEVICES')
    os.environ['MARAY_GEN_WRAP_DEVICES'] = '1'
    try:
        M.gen_cache_clear()
        s = M.Scene(data)
        for k, want in ((4, want4), (1, want1), (4, want4)):
            assert np.array_equal(M.gen_to_image(s, samples=k, n_devices=2, tile_rows=16), want), k
    finally:
        if old is None:
            del os.environ['MARAY_GEN_WRAP_DEVICES']
        else:
            os.environ['MARAY_GEN_WRAP_DEVICES'] = old
        M.gen_cache_clear()


def test_cli_writes_the_pixels_of_gen_to_image(tmp_path):
    path = os.path.join(HERE, 'golden', 'chess.maray')
    out = tmp_path / 'out.png'
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '-s', '4', '-i', path, '-o', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = M.gen_to_image(M.Scene(chess_bytes()), samples=4)
    assert np.array_equal(M.png_read(str(out)), want)
    M.gen_cache_clear()


def test_failed_supersample_keeps_the_cache_name():
    """A supersample that fails leaves the scene's name as it was: the next gen_to_image finds the program it kept (chess
    is a legacy file: were the name dropped, the scene would be named anew from its re-encoding, another name)."""
    M.gen_cache_clear()
    s = M.Scene(chess_bytes())
    first = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1)
    keys = {line.split()[0] for line in M.gen_cache_info()}
    assert len(keys) == 1
    with pytest.raises(M.MarayError):
        s.supersample(3)
    again = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1)
    assert np.array_equal(again, first)
    assert {line.split()[0] for line in M.gen_cache_info()} == keys
    M.gen_cache_clear()
