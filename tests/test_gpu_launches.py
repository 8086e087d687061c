"""Launches that are not the first of their geometry, and launches split into more than one grid.

From its second launch on, a geometry of the specialised back-end takes a cached launch order of its rows
(maray_jit_order, jit_backend.cpp: launch()); the timed step of bench.py is such a launch.  Every render here lands in a
buffer with guard bands of PAD rows on both sides (filled with 0xA5 / a signalling NaN no kernel writes), and every
band byte is checked afterwards.  Results are compared bit for bit: every byte against the scalar-cache interpreter
(BACKEND_TAPE_SMEM) on the device, and bands of rows against the CPU oracle.  Device buffers come from PyTorch, which
has to be imported before the library: each test runs a process of its own."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
from marayb import add, chess, div, encode, inside_triangle, max_, min_, mul, nat, sin, step, sub, to_uv, x, y
from oracle_ffi import Scene as OScene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def tri_soup(seed, regions, w, h, huge_sin=False):
    """Triangles painted over one another (a max chain of guarded shapes), placed region by region: `regions` is a list of
    (x0, x1, y0, y1, n, r), n triangles of radius r whose vertices all lie inside [x0, x1) x [y0, y1).  Each carries a
    chess pattern in its own frame, or with `huge_sin` a Step(Sin) whose argument is past glibc's reduction range for
    x >= 101 (the specialised kernel defers those tiles to the interpreter).  The gradient under the shapes reads Y in
    every pixel (max(x, y) is not a function of the row alone): a pixel given the y of another row shows."""
    from fuzz_scenes import subst_xy
    rng = random.Random(0x7A1 + seed)
    p = [x(), y()]
    tris = []
    for x0, x1, y0, y1, n, r in regions:
        while n:
            cx, cy = rng.randrange(x0, x1), rng.randrange(y0, y1)
            pts = [(min(x1 - 1, max(x0, cx + rng.randrange(-r, r + 1))), min(y1 - 1, max(y0, cy + rng.randrange(-r, r + 1)))) for _ in range(3)]
            if len(set(pts)) < 3 or (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) == (pts[2][0] - pts[0][0]) * (pts[1][1] - pts[0][1]):
                continue
            n -= 1
            tri = [(nat(a), nat(b)) for a, b in pts]
            inside = inside_triangle(tri, p)
            if huge_sin and rng.random() < 0.5:
                pattern = step(sin(add(mul(x(), nat(1 << 20)), y())))
            else:
                uv = to_uv(tri, [(nat(0), nat(0)), (nat(1), nat(0)), (nat(0), nat(1))], p)
                pattern = subst_xy(chess(rng.choice([2, 4])), uv[0], uv[1])
            tris.append(min_(inside, pattern))
    m = tris[0]
    for t in tris[1:]:
        m = max_(m, t)
    grad = mul(add(x(), mul(max_(x(), y()), nat(3))), div(nat(1), nat(w + 3 * max(w, h))))
    return [mul(m, nat(255)), mul(max_(m, mul(grad, div(nat(1), nat(2)))), nat(255)), mul(add(mul(m, div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]


def scene_bytes(name, w, h):
    """The scenes of the repeated-launch test, encoded at w x h."""
    import scenes
    from fuzz_scenes import curved_soup, polygon_soup
    if name == 'chess':
        with open(os.path.join(HERE, 'golden', 'chess.maray'), 'rb') as f:
            return f.read()
    if name == 'polygon_soup':
        return encode((w, h), polygon_soup(5, 40, w, h, mixed=False))
    if name == 'curved_soup':
        return encode((w, h), curved_soup(3, 30, w, h))
    if name == 'huge_sin':
        return encode((w, h), tri_soup(1, [(0, w, 0, h, 24, 60), (0, w, h // 3, h // 3 + 96, 6, 40)], w, h, huge_sin=True))
    assert name == 'radial'
    return encode((w, h), scenes.radial_gradient())


def jit_shape(tape):
    """(the PIXEL kernel runs four pixels per lane everywhere, the program has guard words and so a launch order) -- read
    from the generated sources, as the specialised back-end decides them (jit_wide_general, maray_jit_order)."""
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.maray_jit_source_rows.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    src, rows_src, k = C.c_void_p(), C.c_void_p(), C.c_uint32()
    assert L.maray_jit_source(C.byref(tape.program), C.byref(src)) == 0, L.maray_last_error()
    pix = C.string_at(src).decode()
    L.maray_free(src)
    assert L.maray_jit_source_rows(C.byref(tape.program), C.byref(rows_src), C.byref(k)) == 0, L.maray_last_error()
    rows = C.string_at(rows_src).decode()
    L.maray_free(rows_src)
    return 'general variant four pixels per lane' in pix.split('\n', 1)[0], 'maray_jit_order' in rows


# The part every child process shares: the one helper that backs every device render, comparisons, the oracle.
_PRELUDE = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from marayb import encode
from oracle_ffi import Scene as OScene
from test_lowering import same_f64
import test_gpu_launches as T

PAD = 64                                   # guard rows on both sides of every output
FILL8, FILL64 = 0xA5, 0x7FF4DEADBEEF0001   # RGB8 bands; f64 bands: a signalling NaN no kernel writes
THREADS = min(16, os.cpu_count() or 1)
JIT, INTERP = M.BACKEND_JIT, M.BACKEND_TAPE_SMEM


def out_rows(g):
    return g[2] - g[1] if g[0] == 'rows' else g[2] * g[4]


def image_rows(g):
    # image row of every output row: ('rows', y0, y1) or ('blocks', y0, block_rows, block_stride, n_blocks), packed
    if g[0] == 'rows':
        return np.arange(g[1], g[2])
    _, y0, br, stride, nb = g
    return (y0 + np.arange(nb)[:, None] * stride + np.arange(br)[None, :]).reshape(-1)


def render(ctx, w, h, g, f64=True):
    # one launch of geometry g into buffers of PAD + rows + PAD rows; checks the bands and returns the interior (device)
    n = out_rows(g)
    b8 = torch.full((n + 2 * PAD, w, 3), FILL8, dtype=torch.uint8, device='cuda')
    b64 = torch.full((n + 2 * PAD, w, 3), FILL64, dtype=torch.int64, device='cuda') if f64 else None
    p8 = b8.data_ptr() + PAD * w * 3
    p64 = b64.data_ptr() + PAD * w * 3 * 8 if f64 else 0
    if g[0] == 'rows':
        ctx.render_rows_device(w, h, g[1], g[2], d_rgb8=p8, d_rgb64=p64)
    else:
        ctx.render_blocks_device(w, h, *g[1:], d_rgb8=p8, d_rgb64=p64)
    torch.cuda.synchronize()
    assert bool((b8[:PAD] == FILL8).all()) and bool((b8[PAD + n:] == FILL8).all()), ('RGB8 guard band written', g)
    if b64 is None:
        return b8[PAD:PAD + n], None
    assert bool((b64[:PAD] == FILL64).all()) and bool((b64[PAD + n:] == FILL64).all()), ('f64 guard band written', g)
    in64 = b64[PAD:PAD + n]
    assert not bool((in64 == FILL64).any()), ('f64 pixel never written', g)
    return b8[PAD:PAD + n], in64.view(torch.float64)


def same(got, want):
    # bit-exact on the device: RGB8 bytes; f64 bit patterns, all NaNs equal (only where both results have f64 planes)
    if not torch.equal(got[0], want[0]):
        return False
    if got[1] is None or want[1] is None:
        return True
    a, b = got[1], want[1]
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())


class Oracle:
    # the CPU oracle on bands of image rows, each band computed once
    def __init__(self, data, w, h):
        self.o, self.w, self.h, self.memo = OScene(data), w, h, {}

    def band(self, y0, y1):
        if (y0, y1) not in self.memo:
            self.memo[(y0, y1)] = self.o.render_rows(self.w, self.h, y0, y1, threads=THREADS)
        return self.memo[(y0, y1)]

    def check(self, got, g, bands, f64_bands=()):
        # the rows of `got` (a render of g) that lie in each band [y0, y1) against the oracle; f64 planes on f64_bands
        rows = image_rows(g)
        g8 = got[0].cpu().numpy()
        g64 = got[1].cpu().numpy() if got[1] is not None else None
        for (y0, y1) in list(bands) + list(f64_bands):
            idx = np.nonzero((rows >= y0) & (rows < y1))[0]
            if not len(idx):
                continue
            w8, w64 = self.band(y0, y1)
            assert np.array_equal(g8[idx], w8[rows[idx] - y0]), ('oracle', g, y0, y1)
            if (y0, y1) in f64_bands:
                assert g64 is not None and same_f64(g64[idx], w64[rows[idx] - y0]), ('oracle f64', g, y0, y1)
"""


def _run(body, marker, timeout, **kw):
    paths = dict(root=os.path.dirname(HERE), tests=HERE)
    code = _PRELUDE % paths + body % dict(kw, **paths)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and marker in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


_REPEATED = r"""
name = %(name)r
w = h = 1024
data = T.scene_bytes(name, w, h)
tape = M.Scene(data).lower()
ora = Oracle(data, w, h)
FULL, RAGGED = ('rows', 0, 1024), ('rows', 5, 1021)
BLOCKS = ('blocks', 87, 64, 97, 10)            # rows 87..150, 184..247, ... 960..1023: no block starts on a guard group's row
TOP, SHIFTED = ('rows', 0, 992), ('rows', 32, 1024)    # the same (w, rows) at y0 = 0 and y0 = 32
ODD, ODD2 = ('rows', 0, 1001), ('rows', 11, 1012)      # two-row wavefronts meet a partial last group
GEOMS = [FULL, RAGGED, BLOCKS, TOP, SHIFTED, ODD, ODD2]
ref = M.Context(tape, backend=INTERP)
want = {g: render(ref, w, h, g) for g in GEOMS}
ref.close()
for g in GEOMS:
    ora.check(want[g], g, [(0, 2), (5, 7), (511, 513), (1022, 1024)])
if name == 'chess':                    # the whole frame against the golden raster too
    import hashlib, json
    gold = json.load(open(os.path.join(%(tests)r, 'golden', 'chess_1024.json')))
    assert hashlib.sha256(want[FULL][0].cpu().numpy().tobytes()).hexdigest() == gold['rgb8_sha256']
assert T.jit_shape(tape)[1] == (name != 'radial')          # guards (and a launch order) for all but the gradient
if name == 'huge_sin':
    assert tape.info['sin_ops'] > tape.info['sin_bounded']


def launches(ctx, seq, what, f64=True):
    for i, g in enumerate(seq):
        assert same(render(ctx, w, h, g, f64=f64), want[g]), (what, i, g, f64)


for b in (JIT, M.BACKEND_TAPE, INTERP):
    ctx = M.Context(tape, backend=b)
    for g in (FULL, RAGGED, BLOCKS):
        launches(ctx, [g] * 3, (b, 'repeated'))
        launches(ctx, [g] * 3, (b, 'repeated'), f64=False)     # without f64 planes: the specialised kernel's four-wide stores
    launches(ctx, [FULL, FULL, RAGGED, RAGGED, FULL, RAGGED, FULL, RAGGED], (b, 'A A B B A B A B'))
    launches(ctx, [FULL, RAGGED, FULL, RAGGED], (b, 'A B A B'))
    launches(ctx, [TOP, TOP, TOP, SHIFTED, SHIFTED, SHIFTED], (b, 'y0 = 0, then y0 = 32'))
    ctx.close()
ctx = M.Context(tape, backend=JIT)
launches(ctx, [ODD] * 3 + [ODD2] * 3 + [ODD], 'odd row counts')
ctx.close()
print('repeated ok', name)
"""


@pytest.mark.parametrize('name', ['chess', 'polygon_soup', 'curved_soup', 'huge_sin', 'radial'])
def test_repeated_launches_of_one_geometry_equal_the_first(name):
    """Each of three geometries -- the whole 1024^2 frame, a ragged range (rows 5..1020) and a rank's share of row blocks
    that start off the guard groups -- launched three times on one context, on all three back-ends; then two geometries in
    turn (A A B B A B A B: orders computed, then evicted), the same (w, rows) at y0 = 0 and at y0 = 32 (the first
    order must not serve the second), and odd row counts on the specialised kernels (a partial last group under the
    order).  Every launch, RGB8 and f64, equals the interpreter's first render of its geometry;
    those against the oracle on bands.  Scenes: chess, guarded triangles, curved shapes, guarded triangles with a
    Sin beyond the reduction range (deferred tiles), and the radial gradient (no guards: never an order)."""
    _run(_REPEATED, 'repeated ok', 300, name=name)


_GRID = r"""
w_list, H = (64, 320), 70000
for w in w_list:
    # all dense shapes in rows 32..63 (group 1: the dearest, the first of the launch order), a few small ones elsewhere,
    # two in the last group of 65,534 rows: a grid that took the order from its start would write rows past the end
    data = encode((w, H), T.tri_soup(2, [(0, w, 32, 64, 30, 12), (0, w, 1000, 1024, 1, 4), (0, w, 40000, 40024, 1, 4),
                                         (0, w, 65504, 65534, 2, 6), (0, w, 69000, 69030, 1, 6)], w, H))
    tape = M.Scene(data).lower()
    ora = Oracle(data, w, H)
    ref = M.Context(tape, backend=INTERP)
    TALL = ('rows', 0, H)
    want_tall = render(ref, w, H, TALL, f64=False)
    want = {}
    for n in (65534, 65535, 65536):
        g = ('rows', 0, n)
        want[n] = render(ref, w, H, g)
        ora.check(want[n], g, [(0, 4), (32, 64), (n - 40, n)], f64_bands=[(n - 4, n)])
    ref.close()
    assert float(want[65536][0][32:64].float().std()) > 1.0          # (a picture where the order puts its first rows)
    ctx = M.Context(tape, backend=JIT)
    # a launch taller than any below first: the context's y values, guard words and order then cover any stray read
    assert same(render(ctx, w, H, TALL, f64=False), want_tall), (w, 'tall')
    for n in (65534, 65535, 65536):
        g = ('rows', 0, n)
        for i in range(3):
            got = render(ctx, w, H, g)
            assert same(got, want[n]), (w, n, i)
            if i == 0:
                ora.check(got, g, [(0, 4), (32, 64), (n - 40, n)], f64_bands=[(n - 4, n)])
        assert same(render(ctx, w, H, g, f64=False), want[n]), (w, n, 'RGB8 only')
    ctx.close()
print('grid ok')
"""


def test_row_counts_at_the_grid_boundary_launched_again_and_again():
    """65,534, 65,535 and 65,536 rows (one grid holds 65,534 rows), 64 and 320 pixels wide: each three times into a guarded buffer (f64 planes too), then once more RGB8 only,
    after one 70,000-row launch on the same context.  The scene's costliest 32-row group is group 1 by construction:
    were a second grid to read the launch order from its start, it would write group 1's rows past the end of the
    raster, into the band.  Every byte against the interpreter; the oracle on rows 0-3, 32-63 and the last 40, f64
    planes of the last 4."""
    _run(_GRID, 'grid ok', 300)


_THRESHOLDS = r"""
n_cu = torch.cuda.get_device_properties(0).multi_processor_count
slots = n_cu * 28                    # jit_backend.cpp: device_slots, wavefronts the device holds at once
W = 2049                             # nine tiles a row, the last one pixel wide: room for up to eight tiles per wavefront
thr = []
for k in (1, 4, 16):                 # tiles = n_tx * rows just below / at and just above k x device_slots
    lo = k * slots // 9
    thr += [lo, lo + 1]
H = max(thr) + 1
assert 9 * thr[0] <= slots < 9 * thr[1]
progs = {
    'radial': T.scene_bytes('radial', W, H),
    'guarded': encode((W, H), T.tri_soup(3, [(0, 257, 0, 33, 12, 10), (0, W, 0, H, 40, 25), (0, W, H - 40, H, 4, 12)], W, H)),
}
for name, data in progs.items():
    tape = M.Scene(data).lower()
    ora = Oracle(data, W, H)
    ref = M.Context(tape, backend=INTERP)
    jit = M.Context(tape, backend=JIT)
    assert T.jit_shape(tape) == ((True, False) if name == 'radial' else (False, True)), name
    for n in thr:
        g = ('rows', 0, n)
        want = render(ref, W, H, g)
        ora.check(want, g, [(0, 1), (n - 1, n)], f64_bands=[(n - 1, n)])
        assert same(render(jit, W, H, g, f64=False), want), (name, n, 'RGB8 only')
        assert same(render(jit, W, H, g), want), (name, n)
    # small launches: narrow and ragged widths, one row to a guard group and one row either side of it
    for w in (1, 63, 65, 255, 256, 257):
        o = Oracle(data, w, H)
        for n in (1, 31, 32, 33):
            g = ('rows', 0, n)
            want = render(ref, w, H, g)
            o.check(want, g, [], f64_bands=[(0, 33)])
            assert same(render(jit, w, H, g, f64=False), want), (name, w, n, 'RGB8 only')
            assert same(render(jit, w, H, g), want), (name, w, n)
    jit.close()
    ref.close()
print('thresholds ok', n_cu)
"""


def test_tiles_per_wavefront_on_both_sides_of_each_threshold():
    """The specialised kernel picks tiles per wavefront by how often a launch fills the device (jit_backend.cpp: 1x, 4x and
    16x device_slots = CUs x 28): row counts of a 2049-pixel-wide launch on both sides of each, and widths 1 .. 257 by
    1, 31, 32 and 33 rows -- for a program that runs four pixels per lane everywhere (the radial gradient) and for a
    guarded one.  RGB8-only and f64 launches, every byte against the interpreter, which is checked against the oracle."""
    _run(_THRESHOLDS, 'thresholds ok', 300)


def test_a_failed_rescale_does_not_serve_the_tape_of_the_old_scene(tmp_path):
    """gen_to_image remembers a scene's tape under the scene's name.  A rescale that fails (the size overflows u32) must
    leave the scene unchanged or the name dropped: either way, the next render is the scene as `save` writes it."""
    c = [mul(step(sub(x(), nat(32))), nat(200)), mul(y(), nat(3)), add(mul(x(), nat(2)), nat(7))]
    s = M.Scene(encode((65536, 1), c))
    first = M.gen_to_image(s, size=(64, 64))                     # caches the tape under the scene's name
    with pytest.raises(M.MarayError):
        s.rescale(65537, 1)
    again = M.gen_to_image(s, size=(64, 64))
    s.save(str(tmp_path / 'after.maray'))
    want8, _ = OScene((tmp_path / 'after.maray').read_bytes()).render_rows(64, 64, 0, 64, threads=4, want_f64=False)
    assert np.array_equal(again, want8)
    assert np.array_equal(first, want8)
    assert want8[:, 31, 0].max() == 0 and want8[:, 32, 0].min() == 200           # (x visibly matters at 64 pixels)
