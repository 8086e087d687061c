"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU
oracle on the same inputs, bit-exact — f64 planes by bit pattern (all NaNs
equal), RGB8 rasters byte for byte."""
import hashlib
import json
import os

import numpy as np
import pytest

import maray_amd as M
import scenes
from conftest import GOLDEN
from marayb import encode, let_, add, mul, nat, var_id, x, y, max_, min_, step, sub, div, recip, neg, sqrt, abs_, exp
from oracle_ffi import Scene as OScene
from test_lowering import same_f64

pytestmark = pytest.mark.gpu

BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]


def gpu_vs_oracle(data, w, h, rows, textures=None, backends=BACKENDS, hoist=True):
    tape = M.Scene(data).lower(hoist_rows=hoist)
    o = OScene(data)
    want = {r: o.render_rows(w, h, r[0], r[1], textures) for r in rows}
    for b in backends:
        ctx = M.Context(tape, textures=textures, backend=b)
        for (y0, y1) in rows:
            got8, got64 = ctx.render_rows(w, h, y0, y1)
            w8, w64 = want[(y0, y1)]
            assert same_f64(got64, w64), (b, y0, y1)
            assert np.array_equal(got8, w8), (b, y0, y1)
        ctx.close()


def test_radial_gradient_1024_bit_exact():
    """Config 2: Sqrt(X*X + Y*Y) at 1024x1024; expected raster is min(255, floor(sqrt(x^2+y^2)))."""
    data = encode((1024, 1024), scenes.radial_gradient())
    tape = M.Scene(data).lower()
    yy, xx = np.mgrid[0:1024, 0:1024].astype(np.float64)
    want64 = np.sqrt(xx * xx + yy * yy)
    want8 = np.minimum(np.floor(want64), 255).astype(np.uint8)
    for b in BACKENDS:
        ctx = M.Context(tape, backend=b)
        got8, got64 = ctx.render_rows(1024, 1024, 0, 1024)
        ctx.close()
        assert np.array_equal(got64, np.repeat(want64[:, :, None], 3, axis=2))
        assert np.array_equal(got8, np.repeat(want8[:, :, None], 3, axis=2))
    gpu_vs_oracle(data, 1024, 1024, [(0, 32), (1000, 1024)])


def test_radial_gradient_8192_rgb8_whole_image():
    """Config 2 at the size its throughput is quoted on (8192^2, 192 MiB of RGB8): the whole raster against
    min(255, floor(sqrt(x^2 + y^2))) -- x^2 + y^2 < 2^27 is exact in f64 and sqrt is correctly rounded, so this holds
    unconditionally; ragged row ranges through the pipelined host path."""
    data = encode((8192, 8192), scenes.radial_gradient())
    ctx = M.Context(M.Scene(data).lower(), backend=M.BACKEND_JIT)
    got8, _ = ctx.render_rows(8192, 8192, 0, 8192, want_f64=False)
    part8, _ = ctx.render_rows(8192, 8192, 4093, 4099, want_f64=False)
    ctx.close()
    xx = np.arange(8192, dtype=np.float64)
    for y0 in range(0, 8192, 1024):                                  # in bands: the f64 reference would be 1.6 GB at once
        yy = np.arange(y0, y0 + 1024, dtype=np.float64)[:, None]
        want = np.minimum(np.floor(np.sqrt(xx * xx + yy * yy)), 255).astype(np.uint8)
        assert np.array_equal(got8[y0:y0 + 1024, :, 0], want), y0
        assert np.array_equal(got8[y0:y0 + 1024, :, 1], want) and np.array_equal(got8[y0:y0 + 1024, :, 2], want)
    assert np.array_equal(part8, got8[4093:4099])


def test_chess_1024_full_raster_matches_golden(chess_bytes):
    """Config 1 on the GPU: full 1024^2 raster equals the oracle's committed hash,
    and the PNG fixture to >= 99.98 % with mismatches only on rows 512 / 704."""
    from PIL import Image
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    png = np.asarray(Image.open(os.path.join(GOLDEN, 'chess.png')).convert('RGB'))
    tape = M.Scene(chess_bytes).lower()
    for b in BACKENDS:
        ctx = M.Context(tape, backend=b)
        got8, got64 = ctx.render_rows(1024, 1024, 0, 1024)
        ctx.close()
        assert hashlib.sha256(got8.tobytes()).hexdigest() == g['rgb8_sha256']
        assert int((got8[:, :, 0] == 255).sum()) == g['white_pixels']
        diff = np.any(got8 != png, axis=2)
        assert int(diff.sum()) == g['png_mismatch_pixels'] == 156
        assert set(np.nonzero(diff.any(axis=1))[0].tolist()) <= {512, 704}
        for xq, yq, v in g['probes_xy_rgb64']:
            assert got64[yq, xq].tolist() == v
    gpu_vs_oracle(chess_bytes, 1024, 1024, [(510, 514), (703, 706)])


@pytest.mark.parametrize('hoist', [True, False])
def test_chess_rows_hoisting_on_off(chess_bytes, hoist):
    gpu_vs_oracle(chess_bytes, 1024, 1024, [(600, 603)], hoist=hoist)


def test_chess_4096_rescaled(chess_bytes):
    """Config 3, the headline configuration, on the kernel the headline number is quoted on (maray_jit_pixels) and on
    both interpreters.  The specialised kernel's guards are evaluated per rectangle of 32 rows x 64 pixels and depend on the
    launch geometry, so 1024^2 coverage does not transfer: here the WHOLE 4096^2 raster of every back-end is compared
    byte for byte with the others', the oracle checks bands holding the knife-edge rows (2048..2051, 2816..2819: the
    rows on which images/chess.png differs from IEEE evaluation), the board's first and last rows
    (2048, 3279) and sky, and (4i,4j) == stored (i,j) ties the whole image to config 1's golden hash.
    Pixel driver: /root/reference/src/render.rs:85-97."""
    s = M.Scene(chess_bytes)
    s.rescale(4, 4)
    data = s.encode()
    bands = [(0, 2), (2046, 2052), (2815, 2820), (3278, 3282), (4094, 4096)]
    gpu_vs_oracle(data, 4096, 4096, bands, backends=[M.BACKEND_JIT, M.BACKEND_TAPE_SMEM])
    gpu_vs_oracle(data, 4096, 4096, [(2047, 2049), (2816, 2817)], backends=[M.BACKEND_TAPE])
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    tape = s.lower()
    full = {}
    for b in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE):
        ctx = M.Context(tape, backend=b)
        full[b], _ = ctx.render_rows(4096, 4096, 0, 4096, want_f64=False)
        if b == M.BACKEND_JIT:
            assert ctx.kernel_name == 'maray_jit_pixels'
            # the f64 planes of the board's busiest band, JIT against the interpreter below
            jit64 = ctx.render_rows(4096, 4096, 2800, 2832, want_u8=False)[1]
        if b == M.BACKEND_TAPE_SMEM:
            assert same_f64(jit64, ctx.render_rows(4096, 4096, 2800, 2832, want_u8=False)[1])
        ctx.close()
        sub8 = np.ascontiguousarray(full[b][::4, ::4])
        assert hashlib.sha256(sub8.tobytes()).hexdigest() == g['rgb8_sha256'], b
    assert np.array_equal(full[M.BACKEND_JIT], full[M.BACKEND_TAPE_SMEM])
    assert np.array_equal(full[M.BACKEND_JIT], full[M.BACKEND_TAPE])
    # ... and all three share one lowering and the same rectangle guards: an unsound bound (RowBounds' interval arithmetic)
    # would blank the same rectangle in all of them.  So the WHOLE frame once more from the guard-free lowering -- no SKIP
    # op, no guard, no rebalanced chain, no private region: every pixel evaluates the scene's whole DAG as
    # /root/reference/src/lib.rs:623-670 does -- on the scalar-cache interpreter, every byte against the headline kernel's.
    bare = s.lower(skips=False)
    assert bare.info['skip_ops'] == 0 and bare.info['n_yvals'] == 292 and bare.info['private_regions'] == 0
    ctx = M.Context(bare, backend=M.BACKEND_TAPE_SMEM)
    free8, _ = ctx.render_rows(4096, 4096, 0, 4096, want_f64=False)
    ctx.close()
    assert np.array_equal(free8, full[M.BACKEND_JIT])
    del free8
    # the same frame in one device-resident launch per ragged row range: geometry the bench and gen_to_image use
    ctx = M.Context(tape, backend=M.BACKEND_JIT)
    for y0, y1 in ((0, 2053), (2053, 4096)):
        got8, _ = ctx.render_rows(4096, 4096, y0, y1, want_f64=False)
        assert np.array_equal(got8, full[M.BACKEND_JIT][y0:y1]), (y0, y1)
    ctx.close()


def test_chess_16384_band(chess_bytes):
    """Config 4 (one device's share): chess rescaled x16; a band vs the oracle, and (16i,16j) == stored (i,j)."""
    s = M.Scene(chess_bytes)
    s.rescale(16, 16)
    assert s.size == (16384, 16384)
    data = s.encode()
    gpu_vs_oracle(data, 16384, 16384, [(9600, 9601)], backends=[M.BACKEND_JIT])
    ctx = M.Context(s.lower(), backend=M.BACKEND_JIT)
    got8, _ = ctx.render_rows(16384, 16384, 8192, 8192 + 2048, want_f64=False)      # rows of device 4 of 8
    ctx.close()
    small8, _ = OScene(chess_bytes).render_rows(1024, 1024, 512, 640)
    assert np.array_equal(got8[::16, ::16], small8)


def test_chess_16384_full_image_through_gen_to_image(chess_bytes):
    """Config 4 at full size: chess rescaled x16 to 16384^2 (768 MiB of RGB8) through maray_gen_to_image -- the entry
    point the CLI and a Rust `RenderMethod::Hip` arm call -- on every device present (row tiles, host-side gather:
    /root/reference/src/render.rs:54-83 is the collector it replaces).  EVERY byte of the image against the scalar-cache
    interpreter's (bands of 2,048 rows); pixel (16i,16j) == pixel (i,j) of config 1 (golden hash); the oracle on bands
    across the knife-edge rows, the board's first and last rows and every boundary of a 32-row guard group next to them."""
    s = M.Scene(chess_bytes)
    s.rescale(16, 16)
    img = M.gen_to_image(s, backend=M.BACKEND_JIT)
    assert img.shape == (16384, 16384, 3)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(img[::16, ::16]).tobytes()).hexdigest() == g['rgb8_sha256']
    assert int((img[:, :, 0] == 255).sum()) > 0 and not img[:8192 - 16].any()          # sky above the board is black
    o = OScene(s.encode())
    ctx = M.Context(s.lower(), backend=M.BACKEND_TAPE_SMEM)
    for y0 in range(0, 16384, 2048):
        got8, _ = ctx.render_rows(16384, 16384, y0, y0 + 2048, want_f64=False)
        assert np.array_equal(got8, img[y0:y0 + 2048]), y0
    # board rows 8192 .. 13119 (512 .. 819 of the stored scene); groups of 32 rows start at multiples of 32
    for y0, y1 in ((8191, 8193), (8223, 8225), (11264, 11265), (13087, 13089), (13119, 13121), (16383, 16384)):
        want8, _ = o.render_rows(16384, 16384, y0, y1, want_f64=False)
        assert np.array_equal(img[y0:y1], want8), (y0, y1)
    ctx.close()
    # R == G == B in this scene, everywhere
    assert np.array_equal(img[:, :, 0], img[:, :, 1]) and np.array_equal(img[:, :, 0], img[:, :, 2])


_CONFIG4_ONE_LAUNCH = r"""
import sys, json, hashlib, numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
s = M.Scene(open(%(scene)r, 'rb').read())
s.rescale(16, 16)
tape = s.lower()
w = h = 16384
jit = M.Context(tape, backend=M.BACKEND_JIT)
ref = M.Context(tape, backend=M.BACKEND_TAPE_SMEM)
a = torch.zeros((h, w, 3), dtype=torch.uint8, device='cuda')
b = torch.full((h, w, 3), 7, dtype=torch.uint8, device='cuda')
jit.render_rows_device(w, h, 0, h, d_rgb8=a.data_ptr())            # ONE launch of the whole frame: four tiles per wavefront
ref.render_rows_device(w, h, 0, h, d_rgb8=b.data_ptr())
torch.cuda.synchronize()
assert torch.equal(a, b), 'one-launch raster differs from the interpreter'
# the two share the lowering and its rectangle guards; the guard-free lowering (every pixel evaluates the whole DAG:
# no SKIP op, no guard, no rebalancing, no private regions) shares neither
bare = s.lower(skips=False)
assert bare.info['skip_ops'] == 0 and bare.info['private_regions'] == 0
free = M.Context(bare, backend=M.BACKEND_TAPE_SMEM)
b.fill_(5)
for y0 in range(0, h, 1024):                      # ~0.6 s a band at the bare lowering's 27 Mpx/s
    free.render_rows_device(w, h, y0, y0 + 1024, d_rgb8=b.data_ptr() + y0 * w * 3)
    torch.cuda.synchronize()
assert torch.equal(a, b), 'one-launch raster differs from the guard-free evaluation'
free.close()
g = json.load(open(%(golden)r))
assert hashlib.sha256(np.ascontiguousarray(a[::16, ::16].cpu().numpy()).tobytes()).hexdigest() == g['rgb8_sha256']
# rank 3 of 8 of `bench.py --scaling strong`: 64-row blocks 3, 11, 19, ... in one launch
br, n = 64, 8
nb = h // br // n
c = torch.zeros((nb * br, w, 3), dtype=torch.uint8, device='cuda')
jit.render_blocks_device(w, h, 3 * br, br, n * br, nb, d_rgb8=c.data_ptr())
torch.cuda.synchronize()
want = a.view(h // br, br, w, 3)[3::n].reshape(nb * br, w, 3)
assert torch.equal(c, want), 'a rank\'s interleaved share differs from the whole frame'
print('config 4 ok')
"""


def test_chess_16384_in_one_launch_equals_the_interpreter_on_every_byte(chess_bytes):
    """The launch `bench.py --scaling strong` times: the whole 16384^2 frame in ONE launch takes four tiles per wavefront
    (jit_backend.cpp: launch()), a shape the 24 MiB host tiles of the test above never take.  Every byte against the
    interpreter's, on the device (PyTorch buffers: a process of its own), and rank 3 of 8's interleaved share against the
    rows of the whole frame."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CONFIG4_ONE_LAUNCH % dict(root=os.path.dirname(here), tests=here, scene=os.path.join(GOLDEN, 'chess.maray'),
                                      golden=os.path.join(GOLDEN, 'chess_1024.json'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and 'config 4 ok' in out.stdout, out.stderr[-3000:]


_TALL_ONE_LAUNCH = r"""
import sys, numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from fuzz_scenes import polygon_soup
from marayb import encode
from oracle_ffi import Scene as OScene
w, h = 320, 70000                                   # 1.25 tiles a row; 70,000 rows: two grids (gridDim.y <= 65,535), no launch order
data = encode((w, h), polygon_soup(33, 40, w, h, mixed=False))
tape = M.Scene(data).lower()
jit = M.Context(tape, backend=M.BACKEND_JIT)
ref = M.Context(tape, backend=M.BACKEND_TAPE_SMEM)
a = torch.full((h, w, 3), 9, dtype=torch.uint8, device='cuda')
b = torch.full((h, w, 3), 7, dtype=torch.uint8, device='cuda')
jit.render_rows_device(w, h, 0, h, d_rgb8=a.data_ptr())
ref.render_rows_device(w, h, 0, h, d_rgb8=b.data_ptr())
torch.cuda.synchronize()
assert torch.equal(a, b), 'tall raster differs from the interpreter'
img = a.cpu().numpy()
assert img[::97].std() > 1.0                          # (a picture, not a constant)
o = OScene(data)
for y0, y1 in ((0, 3), (65530, 65540), (69990, 70000)):
    want8, _ = o.render_rows(w, h, y0, y1, want_f64=False)
    assert np.array_equal(img[y0:y1], want8), (y0, y1)
# a range of rows that starts past the first grid and the f64 planes of it
c8 = torch.zeros((600, w, 3), dtype=torch.uint8, device='cuda')
c64 = torch.zeros((600, w, 3), dtype=torch.float64, device='cuda')
jit.render_rows_device(w, h, 65400, 66000, d_rgb8=c8.data_ptr(), d_rgb64=c64.data_ptr())
torch.cuda.synchronize()
assert torch.equal(c8, a[65400:66000])
_, want64 = o.render_rows(w, h, 65534, 65538)
got64 = c64[134:138].cpu().numpy()
assert np.array_equal(got64.view(np.uint64), want64.view(np.uint64))
print('tall ok')
"""


def test_more_rows_than_a_grid_has_in_one_launch():
    """70,000 rows of a 320-pixel-wide scene of guarded triangles in ONE device launch: more rows than gridDim.y takes
    (65,535), so the launch is two grids and has no launch order; the ragged last tile of every row.  Every byte against
    the interpreter's on the device, the oracle on bands at the top, across row 65,535 and at the bottom, f64 planes too."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, '-c', _TALL_ONE_LAUNCH % dict(root=os.path.dirname(here), tests=here)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and 'tall ok' in out.stdout, out.stderr[-3000:]


def _maray_scenes(tmp_path, *names):
    import subprocess
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray_scenes')
    r = subprocess.run([exe, str(tmp_path)] + list(names), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return [str(tmp_path / (n + '.maray')) for n in names]


def test_authored_scenes_simplify_compress_save_render(tmp_path):
    """SURVEY 8(f) N4 end to end: examples/chess.rs as the example runs it -- builders, `.simplify(mem).compress(mem)`
    (/root/reference/examples/chess.rs:43, src/lib.rs:601-614), `save` -- written by maray_scenes at the example's size and
    NATIVELY at 4096 (what the two passes are for), then rendered by the specialised kernels.  The reference's own rules do
    not terminate on this example (maray_hip.h, MARAY_SIMPLIFY_MERGE_DIVISORS; tests/test_simplify.py); with the divisors
    merged the image is the reference's: images/chess.png except on the knife-edge rows 512 and 704, where the stored
    data/chess.maray differs from it too.  And examples/test.rs (:21) the same way, on the reference's rules as they are."""
    from PIL import Image
    p1, p4, psdf = _maray_scenes(tmp_path, 'chess_authored_1024', 'chess_authored_4096', 'sdf_512_authored')
    png = np.asarray(Image.open(os.path.join(GOLDEN, 'chess.png')).convert('RGB'))
    s1 = M.Scene.open(p1)
    assert s1.size == (1024, 1024) and not s1.legacy
    ctx = M.Context(s1.lower(), backend=M.BACKEND_JIT)
    img1, _ = ctx.render_rows(1024, 1024, 0, 1024, want_f64=False)
    ctx.close()
    diff = np.nonzero(np.any(img1 != png, axis=2))[0]
    assert 0 < len(diff) < 300 and set(diff.tolist()) <= {512, 704}
    gpu_vs_oracle(open(p1, 'rb').read(), 1024, 1024, [(0, 2), (510, 515), (702, 707), (818, 822), (1022, 1024)])
    s4 = M.Scene.open(p4)
    assert s4.size == (4096, 4096)
    full = {}
    for b in (M.BACKEND_JIT, M.BACKEND_TAPE_SMEM):
        ctx = M.Context(s4.lower(), backend=b)
        full[b], _ = ctx.render_rows(4096, 4096, 0, 4096, want_f64=False)
        ctx.close()
    assert np.array_equal(full[M.BACKEND_JIT], full[M.BACKEND_TAPE_SMEM])
    assert np.array_equal(full[M.BACKEND_JIT][::4, ::4], img1)            # x / 4096 at 4 i is x / 1024 at i: exact
    gpu_vs_oracle(open(p4, 'rb').read(), 4096, 4096, [(2046, 2052), (2815, 2820), (3278, 3282)], backends=[M.BACKEND_JIT])
    gpu_vs_oracle(open(psdf, 'rb').read(), 512, 512, [(0, 512)])


def test_transforming_builders_scene(tmp_path):
    """maray_scenes transforms_256 (rotate_at, scale_at, p2_cbez, p2_spiral, from_barycentric, var / var_offset: the rest of
    the reference's authoring functions, tests/test_builders.py) on all three back-ends against the oracle, every pixel."""
    (path,) = _maray_scenes(tmp_path, 'transforms_256')
    gpu_vs_oracle(open(path, 'rb').read(), 256, 256, [(0, 256)])


def test_example_test7_gradient(tmp_path):
    """examples/test7.rs: `nat(255) * x() / nat(128)` at 128 x 128 through maray_gen with a progress report every 10 rows
    (Report::Row(10), :9): the raster is floor(255 x / 128) in every channel and row."""
    (path,) = _maray_scenes(tmp_path, 'test7_128')
    data = open(path, 'rb').read()
    gpu_vs_oracle(data, 128, 128, [(0, 128)])
    want = np.repeat(np.repeat((255 * np.arange(128) // 128).astype(np.uint8)[None, :, None], 128, axis=0), 3, axis=2)
    out = str(tmp_path / 'test7.png')
    M.gen(M.Scene(data), out, backend=M.BACKEND_JIT, report_kind=M.api.REPORT_ROW, report_value=10)
    assert np.array_equal(M.png_read(out), want)


def test_cli_with_textures(tmp_path):
    """`maray -i scene.maray -o out.png -t a.png b.png` (/root/reference/examples/maray.rs:36-41, :58-65): textures read
    from PNG files by the binary, sampled on the device, the raster written as PNG -- against the oracle with the same
    textures, every pixel."""
    import subprocess
    from PIL import Image
    tex = scenes.textures(scale=4)
    data = encode((1024, 256), scenes.textured(1024))
    scene = str(tmp_path / 'textured.maray')
    open(scene, 'wb').write(data)
    names = []
    for i, t in enumerate(tex):
        names.append(str(tmp_path / ('t%d.png' % i)))
        M.png_write(names[-1], t)
    want8, _ = OScene(data).render_rows(1024, 256, 0, 256, tex, want_f64=False)
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    for backend in ('jit', 'tape-smem'):
        out = str(tmp_path / ('out_%s.png' % backend))
        r = subprocess.run([exe, '-i', scene, '-o', out, '--backend', backend, '-t'] + names, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.asarray(Image.open(out).convert('RGB')), want8), backend
    r = subprocess.run([exe, '-i', scene, '-o', str(tmp_path / 'x.png'), '-t', names[0]], capture_output=True, text=True)
    assert r.returncode == 1 and 'Error' in r.stderr                  # the scene calls texture 1: App id out of range


def test_gen_to_image_remembers_a_scene_between_calls(chess_bytes):
    """gen_to_image is called once per image, an animation calls it in a loop (/root/reference/src/lib.rs:1177-1213,
    examples/test*.rs).  The second call with the same scene finds its tape and its context (no lowering, no module
    loads, no streams): a few milliseconds where the first takes tens; a changed scene is another program; the cache
    can be emptied."""
    import time
    M.gen_cache_clear()
    s = M.Scene(chess_bytes)
    s.rescale(2, 2)
    with M.PinnedRaster(2048, 2048) as r:
        t0 = time.perf_counter()
        a = M.gen_to_image(s, backend=M.BACKEND_JIT, out=r.array).copy()
        t1 = time.perf_counter()
        times = []
        for _ in range(5):
            t = time.perf_counter()
            b = M.gen_to_image(s, backend=M.BACKEND_JIT, out=r.array)
            times.append(time.perf_counter() - t)
            assert np.array_equal(a, b)
        assert min(times) < 0.010 and min(times) < (t1 - t0) / 4, (t1 - t0, times)
        s.rescale(1, 2)                                               # the handle changed: its key with it
        c = M.gen_to_image(s, backend=M.BACKEND_JIT, size=(2048, 2048), out=r.array).copy()
        assert not np.array_equal(a, c)
        M.gen_cache_clear()
        d = M.gen_to_image(s, backend=M.BACKEND_JIT, size=(2048, 2048), out=r.array)
        assert np.array_equal(c, d)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(a[::2, ::2]).tobytes()).hexdigest() == g['rgb8_sha256']


def test_auto_takes_the_interpreter_when_the_compiler_dies(chess_bytes, monkeypatch, tmp_path):
    """A compiler helper that dies (MARAY_JITC_TEST_ABORT=1: the way an LLVM abort inside hiprtc ends it) makes the
    specialised back-end MARAY_E_HIP -- and MARAY_BACKEND_AUTO the interpreter: still the HIP path, same pixels."""
    monkeypatch.setenv('MARAY_JITC_TEST_ABORT', '1')
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path / 'cache'))
    monkeypatch.setenv('TMPDIR', str(tmp_path))
    monkeypatch.setenv('MARAY_AUTO', 'jit')
    s = M.Scene(chess_bytes)
    s.rescale(1, 3)                                                   # a program no other test has built
    tape = s.lower()
    with pytest.raises(M.MarayError) as e:
        M.Context(tape, backend=M.BACKEND_JIT)
    assert e.value.code == -9 and 'compiler aborted' in str(e.value)
    ctx = M.Context(tape, backend=M.BACKEND_AUTO)
    assert ctx.kernel_name != 'maray_jit_pixels'
    got8, _ = ctx.render_rows(1024, 3072, 1800, 1803, want_f64=False)
    ctx.close()
    want8, _ = OScene(s.encode()).render_rows(1024, 3072, 1800, 1803, want_f64=False)
    assert np.array_equal(got8, want8)


def test_gen_to_image_with_four_workers_on_the_devices_present(chess_bytes, monkeypatch):
    """The multi-device machinery of maray_gen_to_image on whatever is there (MARAY_GEN_WRAP_DEVICES=1: worker d drives
    device d mod visible): four host threads, four contexts, ONE build of the kernels (the first thread's; the others wait
    for it), interleaved ragged row tiles, one raster registered once and written by every context's DMA."""
    monkeypatch.setenv('MARAY_GEN_WRAP_DEVICES', '1')
    monkeypatch.setenv('MARAY_CACHE_DIR', 'off')                    # the in-process table is what the workers share
    s = M.Scene(chess_bytes)
    s.rescale(4, 2)                                                 # 4096 x 2048: a program no other test has built
    seen = []
    img = M.gen_to_image(s, backend=M.BACKEND_JIT, n_devices=4, tile_rows=104, report=lambda im, p: seen.append(p), report_kind=1,
                         report_value=256)
    monkeypatch.delenv('MARAY_GEN_WRAP_DEVICES')
    one = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1)
    assert np.array_equal(img, one)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(img[::2, ::4]).tobytes()).hexdigest() == g['rgb8_sha256']
    assert all(0 <= p < 1 for p in seen)
    with pytest.raises(M.MarayError):                               # without the knob, more devices than present is an error
        M.gen_to_image(s, n_devices=M.device_count() + 1)


def test_gen_to_image_keeps_contexts_per_device_and_rechooses_under_auto(chess_bytes, monkeypatch, tmp_path):
    """What maray_gen_to_image keeps between calls (gen.cpp).  (1) Contexts are kept per PHYSICAL device: after a call whose
    four workers shared the devices present (MARAY_GEN_WRAP_DEVICES) the idle contexts are listed under the devices they
    live on, none under a worker number past the devices.  (2) Under MARAY_BACKEND_AUTO a kept context stands for the
    choice made for the first call's size: a thumbnail takes the interpreter (nothing to build), and a later, larger call
    -- once the specialised kernels are in the code cache -- must not inherit that interpreter context."""
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path / 'cache'))
    M.gen_cache_clear()
    n_dev = M.device_count()
    s = M.Scene(chess_bytes)
    s.rescale(2, 1)                                                  # 2048 x 1024: a program of this test's own
    monkeypatch.setenv('MARAY_GEN_WRAP_DEVICES', '1')
    a = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=4, tile_rows=64)
    monkeypatch.delenv('MARAY_GEN_WRAP_DEVICES')
    info = M.gen_cache_info()
    assert len(info) == 4 and all(int(line.split(' device ')[1].split()[0]) < n_dev for line in info), info
    b = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1)  # takes a context of device 0, whichever worker left it
    assert np.array_equal(a, b)
    M.gen_cache_clear()
    # AUTO: 64 x 64 first (hint: 1 Mpixel, nothing cached -> the interpreter) ...
    small = M.gen_to_image(s, backend=M.BACKEND_AUTO, size=(64, 64), n_devices=1)
    (line,) = M.gen_cache_info()
    assert 'maray_jit' not in line and line.endswith('hint_mpixels 1'), line
    # ... the same scene's kernels get built (another caller, an earlier run: here a context made for the purpose) ...
    tape = s.lower()
    M.Context(tape, backend=M.BACKEND_JIT).close()
    assert tape.jit_code_cached
    # ... and the next, larger call re-decides instead of rendering 16 Mpixels on the thumbnail's interpreter (by AUTO's own
    # estimates cached kernels pay from ~9 Mpixels of this scene: a context of theirs costs 20 ms more than the interpreter's)
    big = M.gen_to_image(s, backend=M.BACKEND_AUTO, size=(4096, 4096), n_devices=1)
    (line,) = M.gen_cache_info()
    assert 'kernel maray_jit_pixels' in line, line
    assert np.array_equal(big[:1024, :2048], b) and np.array_equal(small, b[:64, :64])
    again = M.gen_to_image(s, backend=M.BACKEND_AUTO, size=(64, 64), n_devices=1)      # a smaller call keeps the better context
    (line,) = M.gen_cache_info()
    assert 'kernel maray_jit_pixels' in line and np.array_equal(again, small)
    M.gen_cache_clear()


_BENCH_TWO_RANKS = ['--gpus', '2', '--steps', '5', '--warmup', '2', '--full', '--long-steps', '100', '--no-cold', '--cpu-seconds', '0']


def test_bench_plain_run_dumps_the_last_step(tmp_path, chess_bytes):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` as the driver issues it: the headline alone (what
    --full measures beside it is null), K timed steps, and a fixed sample of the timed raster's rows in DIR.  Pixel
    (4i, 4j) of the 4x rescaled scene is pixel (i, j) of the stored one: sampled rows are held against the oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MARAY_BENCH_FAKE_WORLD')}
    out = str(tmp_path / 'outputs')
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j['steps'] == 3 and j['value'] > 0 and j['ms_per_step'] > 0 and j['unit'] == 'Mpixels/s'
    assert j['higher_is_better'] is True and j['dtype'] == 'f64' and j['metric'] == 'Mpixels/s on chess.maray @4096x4096'
    assert all(j[k] is None for k in ('roofline', 'long_loop', 'end_to_end', 'cold_first_render_ms', 'cpu_baseline'))
    rgb = np.load(os.path.join(out, 'rgb8.npy'))
    rows = np.load(os.path.join(out, 'rgb8_rows.npy'))
    assert rgb.dtype == np.float32 and rows.dtype == np.float64 and rgb.shape == (1024, 4096, 3) and rows.shape == (1024,)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 4096
    o = OScene(chess_bytes)
    for k in np.flatnonzero(rows % 4 == 0)[::48]:         # six rows from top to bottom
        want8, _ = o.render_rows(1024, 1024, int(rows[k]) // 4, int(rows[k]) // 4 + 1, want_f64=False)
        assert np.array_equal(rgb[k, ::4], want8[0].astype(np.float32)), int(rows[k])


def test_bench_starts_two_ranks_on_the_devices_present():
    """`python bench.py --gpus 2` as the driver issues it -- no torchrun around it: the parent starts two ranks (fresh
    processes, never an exec of a process that touched the GPU), relays rank 0's line and its exit code.  On a one-GPU box the
    two ranks share the device (a rehearsal: gloo for the barrier and the max, said so in the line); on two GPUs it is the
    real thing over RCCL.  The line must say n_gpus 2, carry config 4 beside the weak-scaling headline, and both must
    have checked their pixels against the golden hashes.  Rows are independent: /root/reference/src/render.rs:85-97."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MARAY_BENCH_FAKE_WORLD')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py')] + _BENCH_TWO_RANKS, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['scaling'] == 'weak' and j['steps'] == 5 and j['value'] > 0
    assert j['config']['pixels_per_step'] == 2 * 4096 * 4096 and j['config']['bit_exact_vs_golden'] is True
    c4 = j['config4_strong']
    assert c4 and c4['pixels_per_step'] == 16384 * 16384 and c4['rows_per_rank'] == 8192 and c4['bit_exact_vs_golden'] is True
    assert j['long_loop']['steps'] == 100 and j['long_loop']['value'] > 0
    assert (j['rehearsal'] is not None) == (M.device_count() < 2)
    assert j['roofline']['attainable_peak']['value'] > 1000         # GB/s: this box's fill rate, measured in the run


def test_gen_to_image_on_two_devices(chess_bytes):
    """Row tiles dealt to two devices, host-side gather into one raster (no collective).  Needs two
    GPUs: skips itself on a one-GPU box."""
    if M.device_count() < 2:
        pytest.skip('needs >= 2 HIP devices')
    s = M.Scene(chess_bytes)
    s.rescale(4, 4)
    one = M.gen_to_image(s, backend=M.BACKEND_JIT, n_devices=1)
    two = M.gen_to_image(s, backend=M.BACKEND_JIT, n_devices=2, tile_rows=200)          # ragged tiles, interleaved
    assert np.array_equal(one, two)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(two[::4, ::4]).tobytes()).hexdigest() == g['rgb8_sha256']


def test_textured_scene_full_size():
    """Config 5: two textures (1024^2 and 2048x512, splitmix64), 4096x4096, device-side sampling."""
    tex = scenes.textures(scale=1)
    data = encode((4096, 4096), scenes.textured(4096))
    gpu_vs_oracle(data, 4096, 4096, [(0, 3), (2047, 2050), (4093, 4096)], textures=tex)
    # whole image: every output is an integer texel value; channel c of pixel (x,y) = max of the two lookups
    ctx = M.Context(M.Scene(data).lower(), textures=tex, backend=M.BACKEND_JIT)
    got8, _ = ctx.render_rows(4096, 4096, 0, 4096, want_f64=False)
    ctx.close()
    yy, xx = np.mgrid[0:4096, 0:4096]
    a = tex[0][np.minimum(yy // 4, 1023), np.minimum(xx // 4, 1023)]
    bx = (4096 - xx) // 2
    b = np.where((bx < 2048)[..., None], tex[1][np.minimum(yy // 8, 511), np.minimum(bx, 2047)], 0)
    assert np.array_equal(got8, np.maximum(a, b))


def test_cli_renders_chess_png(tmp_path, chess_bytes):
    import subprocess
    from PIL import Image
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    out = str(tmp_path / 'chess.png')
    r = subprocess.run([exe, '-c', '8', '-i', os.path.join(GOLDEN, 'chess.maray'), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    img = np.asarray(Image.open(out).convert('RGB'))
    assert hashlib.sha256(img.tobytes()).hexdigest() == g['rgb8_sha256']
    r = subprocess.run([exe, '-i', '/nonexistent.maray', '-o', out], capture_output=True, text=True)
    assert r.returncode == 1 and 'Error' in r.stderr


def test_textured_scene(chess_bytes, monkeypatch):
    """Config 5 at reduced size vs the oracle, full size through its integer-lookup property; the specialised kernel in its
    default form (four pixels per lane: a small program without guards, texture lookups included since round 4), one pixel
    per lane, and with a call of mr_app per App op (round 3's form)."""
    tex = scenes.textures(scale=4)
    data = encode((1024, 256), scenes.textured(1024))
    gpu_vs_oracle(data, 1024, 256, [(0, 256)], textures=tex)
    for env in ({'MARAY_JIT_WIDE_APP': '0'}, {'MARAY_JIT_WIDE_APP': '0', 'MARAY_JIT_TEXEL_ONCE': '0'}, {'MARAY_JIT_TEXEL_ONCE': '0'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        gpu_vs_oracle(data, 1024, 256, [(0, 256)], textures=tex, backends=[M.BACKEND_JIT])
        for k in env:
            monkeypatch.delenv(k)


def test_ops_on_the_value_of_guarded_shapes(monkeypatch):
    """scenes.ops_on_a_guarded_mask: every kind of op, texture lookups included, fed with the value of guarded shapes -- literal
    zeros in the specialised kernel's variant for tiles without a guard bit (tests/test_jit_offline.py has the build): every
    evaluator against the oracle on every pixel, the specialised kernel also with a call of mr_app per App op."""
    tex = scenes.textures(scale=8)
    data = encode((512, 256), scenes.ops_on_a_guarded_mask(512, 256))
    gpu_vs_oracle(data, 512, 256, [(0, 256)], textures=tex)
    for env in ({'MARAY_JIT_TEXEL_ONCE': '0'},):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        gpu_vs_oracle(data, 512, 256, [(0, 256)], textures=tex, backends=[M.BACKEND_JIT])
        for k in env:
            monkeypatch.delenv(k)


def test_texel_addressing_inside_outside_and_on_a_very_tall_image():
    """`fun_color_channel` (/root/reference/src/textures.rs:27-36) around every border: coordinates below zero, exactly on the last
    texel, one past it, far past it, NaN (0/0 on one row) and +-inf (1/0), for a small image and for one that is 2^24 + 5 texels
    tall (row indices past 2^24: the address arithmetic is 64-bit) -- the specialised kernels compute a texel's address once for
    its three channels and read a valid byte on lanes outside the image (selecting 0.0): against the interpreters and the
    oracle; u8 and f64 planes.  (Round 4 also tried reading through a buffer resource, whose range check returns the 0 by
    itself: bit-exact under this test, and slower -- 63.9 against 41.4 us for config 5 -- so it is not in the library.)"""
    from marayb import app, channel, image_height, image_width
    rng = np.random.default_rng(11)
    small = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    tall_h = (1 << 24) + 5
    tall = np.zeros((tall_h, 1, 3), dtype=np.uint8)
    tall[:, 0, 0] = np.arange(tall_h) % 251
    tall[:, 0, 1] = (np.arange(tall_h) // 7) % 256
    tall[-6:, 0, 2] = [9, 8, 7, 6, 5, 4]
    w, h = 96, 8
    u = add(x(), neg(nat(20)))                                   # -20 .. 75 across the small image's 37 columns
    v = add(mul(y(), nat(4)), neg(nat(3)))                       # -3 .. 25 across its 23 rows
    pole = mul(u, recip(sub(y(), nat(2))))                       # row 2: +-inf and, at u = 0, NaN
    # rows of the tall image: the last ones, reached by x; one past the end; the first
    vt = add(nat(tall_h - 40), x())
    c = [max_(app(channel(0, 0), u, v), mul(app(channel(0, 0), pole, v), div(nat(1), nat(2)))),
         add(app(channel(1, 0), nat(0), vt), mul(app(channel(1, 1), sub(y(), nat(4)), mul(x(), nat(100000))), div(nat(1), nat(4)))),
         add(app(channel(1, 2), nat(0), vt), add(app(channel(0, 2), v, u), mul(app(image_height(1), x(), y()), div(nat(1), nat(1 << 20)))))]
    gpu_vs_oracle(encode((w, h), c), w, h, [(0, h)], textures=[small, tall])


def test_all_ops_scene_bit_exact():
    """Config 3b: every computing variant of Expr (sin, exp, ln, sqrt, abs, recip ...) - f64 planes bit-exact."""
    data = encode((640, 96), scenes.all_ops(640, 96))
    gpu_vs_oracle(data, 640, 96, [(0, 96)])
    data = encode((4096, 4096), scenes.all_ops(4096, 4096))
    gpu_vs_oracle(data, 4096, 4096, [(0, 2), (2047, 2049), (4094, 4096)], backends=[M.BACKEND_JIT, M.BACKEND_TAPE_SMEM])


def test_libm_sweep_through_the_kernels():
    """sin / exp / ln / step(sin) over 2^-40 .. 2^40 x [-300, 300] — glibc bit for bit (oracle calls the system libm)."""
    from marayb import exp, ln, sin
    v = mul(sub(x(), nat(300)), exp(mul(sub(y(), nat(40)), ln(nat(2)))))      # (x - 300) * 2^(y - 40)
    c = [sin(v), exp(mul(v, div(nat(1), nat(64)))), ln(abs_(v))]
    gpu_vs_oracle(encode((600, 81), c), 600, 81, [(0, 81)])
    c = [step(sin(v)), step(sin(add(v, nat(1)))), sin(mul(v, v))]
    gpu_vs_oracle(encode((600, 81), c), 600, 81, [(0, 81)])


def test_sin_of_huge_inf_and_nan_arguments():
    """Arguments beyond glibc's reduce_sincos range (|a| >= 105414350), inf and NaN: the specialised
    kernels defer those tiles to the interpreter kernel; results stay bit-exact."""
    from marayb import exp, ln, sin
    big = mul(x(), nat(10 ** 9))
    c = [sin(add(big, y())), step(sin(mul(big, add(y(), nat(1))))), sin(exp(x()))]                # exp(x) -> inf -> sin = NaN
    t = M.Scene(encode((1000, 4), c)).lower()
    assert t.info['sin_bounded'] == 0 and t.info['sin_ops'] == 3
    gpu_vs_oracle(encode((1000, 4), c), 1000, 4, [(0, 4)])
    # only some tiles are huge: x * 2^20 crosses 105414350 at x ~ 100
    c = [step(sin(mul(x(), nat(1 << 20)))), sin(mul(x(), nat(1 << 20))), sin(ln(sub(x(), nat(500))))]   # ln(<0) = NaN
    gpu_vs_oracle(encode((1000, 3), c), 1000, 3, [(0, 3)])


def test_corner_cases():
    nanv = var_id(99)
    c = [max_(nanv, x()), min_(mul(nanv, y()), nat(7)), step(sub(x(), y()))]
    gpu_vs_oracle(encode((300, 7), c), 300, 7, [(0, 7)])                # ragged width (not a multiple of 256)
    c = [recip(sub(x(), nat(3))), sqrt(sub(x(), y())), abs_(neg(div(x(), y())))]   # inf, NaN, -0 paths
    gpu_vs_oracle(encode((64, 5), c), 64, 5, [(0, 5)])
    # +0 / -0 through max/min feeding recip (IEEE maximumNumber/minimumNumber choice)
    z = mul(sub(x(), x()), nat(1))
    c = [recip(min_(z, neg(z))), recip(max_(z, neg(z))), recip(max_(neg(z), z))]
    gpu_vs_oracle(encode((8, 2), c), 8, 2, [(0, 2)])
    shared = let_([(0, add(x(), nat(1))), (1, mul(var_id(0), y()))], add(var_id(1), var_id(0)))
    gpu_vs_oracle(encode((8, 8), [nat(200), y(), div(shared, nat(3))]), 8, 8, [(0, 8)])
    gpu_vs_oracle(encode((1, 1), [x(), y(), nat(0)]), 1, 1, [(0, 1)])   # minimum size
    # empty row range is a no-op
    ctx = M.Context(M.Scene(encode((4, 4), [x(), x(), x()])).lower())
    a, b = ctx.render_rows(4, 4, 2, 2)
    assert a.shape == (0, 4, 3)
    with pytest.raises(M.MarayError):
        ctx.render_rows(4, 4, 3, 9)
    ctx.close()


def test_step_of_a_sum_with_a_constant_is_one_compare():
    """The specialised kernels evaluate Step(v + k), k a constant, as the compare v >= -k (and Step(-(v + k)) as v <= -k) without
    the addition (jit_emit.hpp).  Exact only because a floating-point sum is never rounded to zero and an exact zero sum is +0:
    here v runs through the values next to -k on both sides (one ulp, a subnormal's distance), through +0 and -0, huge values
    that absorb k, +-inf and NaN, for k = 0, 1, -1, tiny, huge and 2^-1074 -- all three back-ends against the oracle, f64 planes
    and bytes.  /root/reference/src/lib.rs:644-647 (Step), :651 (Add)."""
    # v(x): a table of interesting values selected by x through steps: v = sum_i t_i * [x == i]
    import struct

    def f64(bits):
        return struct.unpack('<d', struct.pack('<Q', bits))[0]
    bools, sums = [], []
    for k_num, k_den in ((0, 1), (1, 1), (3, 1), (1, 3), (1, 1 << 60), (1 << 62, 1)):
        for sign in (1, -1):
            k = div(nat(k_num), nat(k_den))
            if sign < 0:
                k = neg(k)
            # v = (x - 8) * 2^-e: exact multiples crossing zero; that minus k (crossing -k); that over (y - 1): +-inf and NaN on row 1
            for e in (0, 30, 990):
                sc = nat(1)
                for _ in range(e // 30):
                    sc = mul(sc, recip(nat(1 << 30)))
                u = mul(sub(x(), nat(8)), sc)
                for v in (u, sub(u, k), mul(u, recip(sub(y(), nat(1)))), sub(recip(sub(x(), nat(8))), recip(sub(x(), nat(8))))):
                    bools.append(step(add(v, k)))
                    bools.append(step(neg(add(k, v))))
                if e == 30:
                    sums.append(mul(step(add(u, k)), add(u, k)))      # the sum read by something else as well
    # 24 booleans a channel, as the bits of an exactly representable sum
    chans = []
    for i in range(0, len(bools), 24):
        acc = nat(0)
        for j, b_ in enumerate(bools[i:i + 24]):
            acc = add(acc, mul(b_, nat(1 << j)))
        chans.append(acc)
    chans += sums
    while len(chans) % 3:
        chans.append(nat(0))
    w, h = 17, 3
    for i in range(0, len(chans), 3):
        gpu_vs_oracle(encode((w, h), chans[i:i + 3]), w, h, [(0, h)])


def test_sqrt_of_tiny_zero_negative_and_infinite_arguments():
    """Sqrt scales arguments below 2^-767 (the Newton steps would lose bits); the device asks once per wavefront whether
    any lane needs that (device_math.h, mr_sqrt).  Subnormals, values either side of the threshold, zeros of both signs,
    negatives, inf and NaN: mixed inside a wavefront (they depend on x), uniform over it (they depend on y only, which
    also runs them in the ROW kernel), and in a 4-op scene that takes the four-pixels-per-lane form."""
    tiny = exp(neg(add(mul(x(), nat(5)), nat(400))))                  # e^-400 ... e^-1675: 1e-174 down through the subnormals to 0
    tiny_y = exp(neg(add(mul(y(), nat(90)), nat(380))))
    edge = mul(exp(neg(nat(532))), add(nat(1), mul(x(), recip(nat(64)))))       # 9.0e-232 ... 4.5e-231: crosses 2^-767 = 1.29e-231 at x = 27
    signed = mul(sub(x(), nat(100)), exp(neg(nat(700))))                       # negative, -0 / +0 at x = 100, positive: all tiny
    c = [sqrt(tiny), sqrt(edge), sqrt(signed)]
    gpu_vs_oracle(encode((256, 6), c), 256, 6, [(0, 6)])
    c = [sqrt(tiny_y), sqrt(add(tiny_y, mul(x(), nat(0)))), sqrt(recip(sub(x(), nat(7))))]      # uniform tiny; +-inf at x = 7
    gpu_vs_oracle(encode((300, 9), c), 300, 9, [(0, 9)])
    gpu_vs_oracle(encode((600, 3), [sqrt(tiny), sqrt(tiny), sqrt(tiny)]), 600, 3, [(0, 3)])      # small program: four pixels per lane
    nanv = var_id(99)
    gpu_vs_oracle(encode((128, 2), [sqrt(mul(nanv, x())), sqrt(max_(nanv, signed)), sqrt(edge)]), 128, 2, [(0, 2)])


def test_many_live_values_spill_path():
    """A scene with more simultaneously live values than fit in LDS exercises the HBM spill slots."""
    terms = [add(mul(x(), nat(k + 1)), nat(k)) for k in range(120)]
    acc = terms[0]
    for t in terms[1:]:
        acc = max_(acc, t)
    # keep every term live until the end by reusing them all again
    tail = terms[0]
    for t in terms[1:]:
        tail = add(tail, t)
    c = [add(acc, tail), acc, tail]
    data = encode((512, 3), c)
    assert M.Scene(data).lower().info['n_pix_slots'] > 80
    gpu_vs_oracle(data, 512, 3, [(0, 3)])


def test_gen_to_image_with_more_devices_than_present_fails_cleanly(chess_bytes):
    n = M.device_count()
    with pytest.raises(M.MarayError):
        M.gen_to_image(M.Scene(chess_bytes), n_devices=n + 1)
    img = M.gen_to_image(M.Scene(chess_bytes), n_devices=n, tile_rows=100)      # ragged tile height
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(img.tobytes()).hexdigest() == g['rgb8_sha256']


def test_gen_to_image_and_png_roundtrip(tmp_path, chess_bytes):
    s = M.Scene(chess_bytes)
    seen = []
    img = M.gen_to_image(s, report=lambda im, p: seen.append(p), report_kind=1, report_value=128, tile_rows=64)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(img.tobytes()).hexdigest() == g['rgb8_sha256']
    # like the reference's collector (src/render.rs:63-82: poll every 10 ms, no report once the last row is in), a
    # render that is over within one poll reports nothing; what is reported is a fraction of an unfinished image
    assert all(0 <= p < 1 for p in seen)
    p = str(tmp_path / 'out.png')
    M.gen(s, p)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(p).convert('RGB')), img)
    assert np.array_equal(M.png_read(p), img)


def test_progress_reports_arrive_while_a_long_render_runs(chess_bytes):
    """Report::Row through the LDS-tape interpreter on chess at 8192^2 (tens of milliseconds: several polls of the
    collector loop): callbacks arrive on the calling thread with the raster filled up to the row they name."""
    s = M.Scene(chess_bytes)
    s.rescale(8, 8)
    seen = []

    def report(im, p):
        seen.append((p, bool(im[int(p * 8192) - 1].any()) if p * 8192 > 4200 else None))
    img = M.gen_to_image(s, backend=M.BACKEND_TAPE, report=report, report_kind=1, report_value=256, tile_rows=64)
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(img[::8, ::8]).tobytes()).hexdigest() == g['rgb8_sha256']
    assert seen and all(0 <= p < 1 for p, _ in seen) and [p for p, _ in seen] == sorted(p for p, _ in seen)
    # a report naming a row inside the board (image rows 4096..6559) sees that row already painted
    assert all(painted for p, painted in seen if painted is not None and p * 8192 < 6500)


def test_host_rasters_pinned_and_pageable(chess_bytes):
    """The host-raster entry points (maray_hip_render_rows, maray_hip_render_tiles): tile k's device -> host copy runs
    under tile k+1's kernels.  Same bytes whether the raster is pinned (maray_host_alloc: written by DMA), registered
    (maray_host_register), or pageable (pinned staging ring + host copy); tiles ragged, out of order, disjoint."""
    import ctypes as C
    s = M.Scene(chess_bytes)
    s.rescale(4, 4)
    tape = s.lower()
    ctx = M.Context(tape, backend=M.BACKEND_JIT)
    want, _ = ctx.render_rows(4096, 4096, 0, 4096, want_f64=False)            # pageable numpy raster, cut into ~8 MiB tiles
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    assert hashlib.sha256(np.ascontiguousarray(want[::4, ::4]).tobytes()).hexdigest() == g['rgb8_sha256']
    pin = M.PinnedRaster(4096, 4096)
    pin.array[:] = 7
    ctx.render_rows_into(4096, 4096, 0, 4096, pin.array)
    assert np.array_equal(pin.array, want)
    # tiles: ragged heights, not in row order, leaving rows 1000..1999 untouched
    tiles = [(2000, 2051), (0, 1000), (2051, 4096)]
    done = []
    pin.array[:] = 7
    ctx.render_tiles(4096, 4096, tiles, pin.array, on_tile=lambda a, b: done.append((a, b)))
    assert done == tiles
    assert np.array_equal(pin.array[:1000], want[:1000]) and np.array_equal(pin.array[2000:], want[2000:])
    assert (pin.array[1000:2000] == 7).all()
    page = np.full((4096, 4096, 3), 9, np.uint8)
    ctx.render_tiles(4096, 4096, tiles, page)
    assert np.array_equal(page[:1000], want[:1000]) and np.array_equal(page[2000:], want[2000:]) and (page[1000:2000] == 9).all()
    # a raster the caller registers itself
    reg = np.zeros((4096, 4096, 3), np.uint8)
    assert M.lib().maray_host_register(reg.ctypes.data, reg.nbytes) == 0, M.lib().maray_last_error()
    ctx.render_rows_into(4096, 4096, 0, 4096, reg)
    assert M.lib().maray_host_unregister(reg.ctypes.data) == 0
    assert np.array_equal(reg, want)
    # f64 planes and RGB8 together through the pipeline, both interpreters too
    for b in (M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE):
        c2 = M.Context(tape, backend=b)
        got8, got64 = c2.render_rows(4096, 4096, 2040, 2560)
        c2.close()
        assert np.array_equal(got8, want[2040:2560])
        assert np.array_equal(np.minimum(got64, 255).astype(np.uint8), got8)
    pin.close()
    ctx.close()
    with pytest.raises(M.MarayError):
        M.Context(tape, backend=M.BACKEND_JIT).render_tiles(4096, 4096, [(0, 5000)], page)


def test_jit_in_a_process_that_imported_torch_first(chess_bytes):
    """bench.py imports PyTorch before the library, and PyTorch brings its own (older) hiprtc / comgr, which then
    compiles the specialised kernels instead of /opt/rocm's.  Same raster either way."""
    import subprocess
    import sys
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    code = ('import torch, hashlib, sys; sys.path.insert(0, %r); import maray_amd as M\n'
            'assert torch.cuda.is_available()\n'
            's = M.Scene(open(%r, "rb").read()); t = s.lower(); c = M.Context(t, backend=M.BACKEND_JIT)\n'
            'g8, _ = c.render_rows(1024, 1024, 0, 1024, want_f64=False)\n'
            'print(c.kernel_name, hashlib.sha256(g8.tobytes()).hexdigest())\n'
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(GOLDEN, 'chess.maray')))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    name, digest = out.stdout.split()[-2:]
    assert name == 'maray_jit_pixels' and digest == g['rgb8_sha256']


_BLOCKS_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_lowering import same_f64
tape = M.Scene(open(%(scene)r, 'rb').read()).lower()
w = h = 1024
y0, br, stride, nb = 64, 32, 96, 9          # rows 64..95, 160..191, ... up to 832..863
for b in (M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT):
    ctx = M.Context(tape, backend=b)
    one8 = torch.zeros((nb * br, w, 3), dtype=torch.uint8, device='cuda')
    one64 = torch.zeros((nb * br, w, 3), dtype=torch.float64, device='cuda')
    ctx.render_blocks_device(w, h, y0, br, stride, nb, d_rgb8=one8.data_ptr(), d_rgb64=one64.data_ptr())
    torch.cuda.synchronize()
    for k in range(nb):
        g8, g64 = ctx.render_rows(w, h, y0 + k * stride, y0 + k * stride + br)
        assert np.array_equal(one8[k * br:(k + 1) * br].cpu().numpy(), g8), (b, k)
        assert same_f64(one64[k * br:(k + 1) * br].cpu().numpy(), g64), (b, k)
    for bad in ((0, 32, 16, 2), (900, 32, 96, 9)):       # overlapping blocks; blocks past the image
        try:
            ctx.render_blocks_device(w, h, *bad, d_rgb8=one8.data_ptr())
        except M.MarayError:
            pass
        else:
            raise AssertionError(bad)
    ctx.close()
print('blocks ok')
"""


def test_row_blocks_in_one_launch_equal_the_blocks_one_by_one():
    """maray_hip_render_blocks_device: a rank's interleaved share (blocks of rows, a stride apart) in one launch.
    Device buffers come from PyTorch, which has to be imported before the library: a process of its own."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = _BLOCKS_SCRIPT % dict(root=os.path.dirname(here), tests=here, scene=os.path.join(GOLDEN, 'chess.maray'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and 'blocks ok' in out.stdout, out.stderr[-3000:]


def test_guards_per_group_of_rows_with_ragged_ranges(chess_bytes):
    """The specialised path evaluates chess's guards once per rectangle of 32 rows x 64 pixels; ranges that do not start
    or end on a multiple of 32 have a partial group at the end.  Against the interpreter, which evaluates them row by row."""
    tape = M.Scene(chess_bytes).lower()
    jit = M.Context(tape, backend=M.BACKEND_JIT)
    ref = M.Context(tape, backend=M.BACKEND_TAPE_SMEM)
    for y0, y1 in ((5, 1021), (509, 516), (700, 713), (481, 545), (512, 577)):
        a8, a64 = jit.render_rows(1024, 1024, y0, y1)
        b8, b64 = ref.render_rows(1024, 1024, y0, y1)
        assert np.array_equal(a8, b8) and same_f64(a64, b64), (y0, y1)
    jit.close()
    ref.close()


def test_specialised_kernel_variants_selected_by_tuning_knobs(chess_bytes, monkeypatch):
    """The eight knobs the specialised path still has, each on a path the default build of chess does
    not take: other strip lengths, other guard rectangles (256 x 8 was round 1's: the tile's words are then taken per
    tile, not per pass), every wave-level region kept or none, guards compiled away, an in-process build at -O1.  The
    layouts that lost (r2_ablations.jsonl) are gone from the library, and their knobs with them."""
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    tape = M.Scene(chess_bytes).lower()
    for env in ({'MARAY_JIT_TILES': '1'}, {'MARAY_JIT_TILES': '5'}, {'MARAY_JIT_GUARD_W': '256', 'MARAY_JIT_GUARD_H': '8'},
                {'MARAY_JIT_GUARD_W': '128', 'MARAY_JIT_GUARD_H': '16', 'MARAY_JIT_TILES': '3'}, {'MARAY_JIT_GUARD_W': '64', 'MARAY_JIT_GUARD_H': '128'},
                {'MARAY_JIT_MIN_REGION': '0'}, {'MARAY_JIT_MIN_REGION': '12'}, {'MARAY_JIT_MIN_REGION': '100000'}, {'MARAY_JIT_ROW_GUARDS': '0'},
                {'MARAY_JIT_HELPER': '0', 'MARAY_JIT_OPT': '-O1'}, {'MARAY_JIT_TEXEL_ONCE': '0'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = M.Context(tape, backend=M.BACKEND_JIT)
        got8, got64 = ctx.render_rows(1024, 1024, 0, 1024)
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        assert hashlib.sha256(got8.tobytes()).hexdigest() == g['rgb8_sha256'], env
        assert np.array_equal(np.minimum(got64, 255).astype(np.uint8), got8), env


def test_interpreter_variants_selected_by_tuning_knobs(chess_bytes, monkeypatch):
    """The interpreter's other paths: the generic loop (what a program whose slots do not fit LDS gets, spill area
    included), guards evaluated per row as y values (what a scene whose guards read Y gets), cones kept in the
    order the ROW section was scheduled in (more live slots: LDS + spill), other guard rectangles than 64 x 32."""
    g = json.load(open(os.path.join(GOLDEN, 'chess_1024.json')))
    tape = M.Scene(chess_bytes).lower()
    for env in ({'MARAY_TAPE_GENERIC': '1'}, {'MARAY_TAPE_ROW_GUARDS': '1'}, {'MARAY_TAPE_KEEP_ORDER': '1'},
                {'MARAY_TAPE_GENERIC': '1', 'MARAY_TAPE_KEEP_ORDER': '1'}, {'MARAY_TAPE_ROW_GUARDS': '1', 'MARAY_TAPE_GENERIC': '1'},
                {'MARAY_TAPE_GUARD_W': '256', 'MARAY_TAPE_GUARD_H': '8'}, {'MARAY_TAPE_GUARD_W': '128', 'MARAY_TAPE_GUARD_H': '64'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for b in (M.BACKEND_TAPE_SMEM, M.BACKEND_TAPE):
            ctx = M.Context(tape, backend=b)
            got8, _ = ctx.render_rows(1024, 1024, 0, 1024, want_f64=False)
            ctx.close()
            assert hashlib.sha256(got8.tobytes()).hexdigest() == g['rgb8_sha256'], (env, b)
        for k in env:
            monkeypatch.delenv(k)


def test_guarded_shapes_through_inf_and_nan():
    """The scene of tests/test_lowering.py's soundness test on the device, all three evaluators, ragged width."""
    gpu_vs_oracle(encode((192, 24), scenes.shapes_through_inf_and_nan()), 192, 24, [(0, 24)])
    gpu_vs_oracle(encode((700, 40), scenes.shapes_through_inf_and_nan()), 700, 40, [(0, 40), (3, 29)])


def test_a_boolean_that_is_true_on_every_lane_materialises_on_all_64():
    """Step(x) is true for every pixel: its lane mask is EXEC itself.  The select that turns a mask into an f64 must
    not be handed EXEC as its selector (the upper 32 lanes of every wavefront came out 0)."""
    c = [add(step(x()), y()), mul(add(step(x()), nat(2)), x()), sub(nat(7), step(mul(x(), y())))]
    gpu_vs_oracle(encode((200, 3), c), 200, 3, [(0, 3)])
