"""The animation writer on the device (include/maray_hip.h, "animation"): maray_frame_delta against numpy's bounding box,
apng_encode_device on arbitrary frames, Context.render_apng on the three back-ends, gen_animation and the CLI's --apng.
Every file is decoded by tests/apng_stream.py, which trusts nothing in it, and the composed frames are compared with the
inputs by np.array_equal.

Device rasters for frame_delta and apng_encode_device are torch tensors: those tests run in child processes that import torch
before the library, as tests/test_gpu_png_device.py does."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import apng_stream as A
import byte_rasters as BR
import maray_amd as M
import params as PR
import png_stream as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]
DELTA_WS, DELTA_HS = (1, 2, 5, 21, 64, 65, 257), (1, 2, 19)
ALIGN_WS, ALIGN_H = (1, 5, 65), 7


class band_rows:
    """MARAY_PNG_BAND_ROWS for the encoders created inside (it is read when an encoder is created)."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.old = os.environ.get('MARAY_PNG_BAND_ROWS')
        if self.rows is None:
            os.environ.pop('MARAY_PNG_BAND_ROWS', None)
        else:
            os.environ['MARAY_PNG_BAND_ROWS'] = str(self.rows)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('MARAY_PNG_BAND_ROWS', None)
        else:
            os.environ['MARAY_PNG_BAND_ROWS'] = self.old


def on_device(a, offset=0):
    """(tensor, pointer): a's bytes in device memory, `offset` bytes into a torch buffer.  (In a child process: torch.)"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.zeros(flat.size + offset + 16, dtype=torch.uint8, device='cuda')
    buf[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def delta(prev, cur, off_prev=0, off_cur=0):
    tp, pp = on_device(prev, off_prev)
    tc, pc = on_device(cur, off_cur)
    return M.frame_delta(pp, pc, cur.shape[1], cur.shape[0])


_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_apng as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=600):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


# ---- the launch constants, from the sources (as tests/reduce_passes.py reads the reduces') ---------------------------------
def delta_constants():
    hpp = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'apng_device.hpp')).read()
    hip = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'apng_device.hip')).read()
    m = re.findall(r'constexpr uint32_t DELTA_BLOCK = (\d+), DELTA_MAX_BLOCKS = (\d+);', hpp)
    assert len(m) == 1
    # the arithmetic restated in delta_split, line by line
    for text, line in ((hpp, 'const size_t blocks = (bytes / 16 + DELTA_BLOCK - 1) / DELTA_BLOCK;'),
                       (hpp, 'return (uint32_t)std::min<size_t>(std::max<size_t>(blocks, 1), DELTA_MAX_BLOCKS);'),
                       (hip, 'const uint32_t head = mis ? (16u - mis < a.bytes ? 16u - mis : a.bytes) : 0u;'),
                       (hip, 'const uint32_t n_vec = (a.bytes - head) / 16u;'),
                       (hip, 'const uint32_t stride = gridDim.x * DELTA_BLOCK;'),
                       (hip, 'for (uint32_t v = blockIdx.x * DELTA_BLOCK + threadIdx.x; v < n_vec; v += stride)')):
        assert line in text, 'the frame delta no longer reads %r: restate it in tests/test_gpu_apng.py' % line
    return int(m[0][0]), int(m[0][1])


def delta_split(nbytes, mis):
    """(head bytes, vectors, tail bytes, vectors one pass of the grid covers) with `cur` mis bytes past a multiple of 16."""
    block, max_blocks = delta_constants()
    head = min(16 - mis, nbytes) if mis else 0
    n_vec = (nbytes - head) // 16
    blocks = min(max((nbytes // 16 + block - 1) // block, 1), max_blocks)
    return head, n_vec, nbytes - head - 16 * n_vec, blocks * block


PASSES_W, PASSES_MIS = 1021, (0, 9)


def passes_height():
    """The smallest height of a PASSES_W-wide raster at which, at both misalignments, a lane of the capped grid takes at least
    three passes, the last of them ragged (not every lane takes it), and a tail of 1 .. 15 bytes is left."""
    h = 1
    while True:
        ok = True
        for mis in PASSES_MIS:
            head, n_vec, tail, stride = delta_split(3 * PASSES_W * h, mis)
            ok = ok and n_vec > 2 * stride + 1000 and n_vec % stride != 0 and n_vec < 3 * stride and 1 <= tail <= 15
        if ok:
            return h
        h += 1
        assert 3 * PASSES_W * h <= 64 << 20


def test_the_multi_pass_shape_is_what_it_is_for():
    """(no device) The grid IS capped (DELTA_MAX_BLOCKS): the shape is derived from the exported constants."""
    block, max_blocks = delta_constants()
    h = passes_height()
    for mis in PASSES_MIS:
        head, n_vec, tail, stride = delta_split(3 * PASSES_W * h, mis)
        assert stride == block * max_blocks and 2 * stride < n_vec < 3 * stride and tail


# ---- the delta kernel against numpy ----------------------------------------------------------------------------------------
def child_delta_content():
    for w in DELTA_WS:
        for h in DELTA_HS:
            a = P.random_bytes(1000 * w + h, h, w)
            cases = [('identical', a.copy())]
            for name, at in (('first byte', 0), ('last byte', a.size - 1)):
                b = a.copy()
                b.reshape(-1)[at] ^= 0x80
                cases.append((name, b))
            for c in range(3):
                b = a.copy()
                b[h // 2, w // 2, c] ^= 1
                cases.append(('channel %d of a middle pixel' % c, b))
            b = a.copy()
            b[0, 0, 1] ^= 4
            b[h - 1, w - 1, 2] ^= 4
            cases.append(('two far corners', b))
            b = a.copy()
            b.reshape(-1)[a.size - 1 - (a.size - 1) % 4:] ^= 0xFF
            cases.append(('the last partial dword', b))
            rng = np.random.default_rng(w * 31 + h)
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            y1, x1 = int(rng.integers(y0 + 1, h + 1)), int(rng.integers(x0 + 1, w + 1))
            b = a.copy()
            b[y0:y1, x0:x1] = P.random_bytes(7, y1 - y0, x1 - x0)
            cases.append(('a random sub-rectangle', b))
            b = a.copy()                # the four edges of a box, one pixel each, the interior equal
            b[y0, (x0 + x1 - 1) // 2, 0] ^= 1
            b[y1 - 1, (x0 + x1 - 1) // 2, 1] ^= 1
            b[(y0 + y1 - 1) // 2, x0, 2] ^= 1
            b[(y0 + y1 - 1) // 2, x1 - 1, 0] ^= 1
            cases.append(('the four edges of a box', b))
            for name, b in cases:
                want = A.bounding_box(a, b)
                assert delta(a, b) == want, (w, h, name, want)
                assert delta(b, a, 3, 9) == want, (w, h, name, 'swapped, misaligned')
            assert A.bounding_box(a, cases[0][1]) == (0, 0, 0, 0) and A.bounding_box(a, cases[6][1]) == (0, 0, w, h)


def test_delta_content_cases_at_every_size():
    """Widths at which packed rows hit every dword alignment, head and tail, heights 1, 2 and 19: identical rasters, single
    bytes, the far corners, the last partial dword, a random sub-rectangle, the four edges of a box."""
    _run('child_delta_content()')


def child_delta_alignment():
    for w in ALIGN_WS:
        a = P.random_bytes(400 + w, ALIGN_H, w)
        b = a.copy()
        b[1, w // 3] ^= 0x10
        b[ALIGN_H - 2, w - 1 - w // 4, 1] ^= 0x10
        want = A.bounding_box(a, b)
        first, last = a.copy(), a.copy()
        first.reshape(-1)[0] ^= 1
        last.reshape(-1)[-1] ^= 1
        prevs = [on_device(a, o) for o in range(16)]
        for cur, box in ((b, want), (first, (0, 0, 1, 1)), (last, (w - 1, ALIGN_H - 1, w, ALIGN_H)), (a, (0, 0, 0, 0))):
            curs = [on_device(cur, o) for o in range(16)]
            for op in range(16):
                for oc in range(16):
                    assert M.frame_delta(prevs[op][1], curs[oc][1], w, ALIGN_H) == box, (w, op, oc, box)


def test_delta_with_both_rasters_at_every_pair_of_byte_offsets():
    _run('child_delta_alignment()')


def child_delta_every_x_and_y():
    w, h = 70, 3
    a = P.random_bytes(70, h, w)
    ta, pa = on_device(a, 5)
    for x in range(w):
        b = a.copy()
        b[1, x, x % 3] ^= 0x20
        tb, pb = on_device(b, x % 16)
        assert M.frame_delta(pa, pb, w, h) == (x, 1, x + 1, 2), x
    for y in range(h):
        b = a.copy()
        b[y, 33, 1] ^= 0x20
        tb, pb = on_device(b, 2)
        assert M.frame_delta(pa, pb, w, h) == (33, y, 34, y + 1), y


def test_delta_of_a_single_pixel_at_every_x_and_every_y():
    _run('child_delta_every_x_and_y()')


def child_delta_passes():
    import torch
    w, h = PASSES_W, passes_height()
    a = P.random_bytes(5, h, w)
    for mis in PASSES_MIS:
        head, n_vec, tail, stride = delta_split(a.size, mis)
        ta, pa = on_device(a, 5)
        tb, pb = on_device(a, mis)
        assert pb % 16 == mis
        assert M.frame_delta(pa, pb, w, h) == (0, 0, 0, 0)
        # one byte in the last, ragged pass; one in the first pass; one in the second; and the tail's last byte
        for at in (head + 16 * (n_vec - 1) + 7, head + 16 * 3 + 2, head + 16 * (stride + 11) + 15, a.size - 1):
            tb[mis + at] ^= 0x40
            torch.cuda.synchronize()
            pix = at // 3
            want = (pix % w, pix // w, pix % w + 1, pix // w + 1)
            assert M.frame_delta(pa, pb, w, h) == want, (mis, at, want)
            assert M.frame_delta(pb, pa, w, h) == want, (mis, at, want, 'swapped')
            tb[mis + at] ^= 0x40
        torch.cuda.synchronize()
        assert M.frame_delta(pa, pb, w, h) == (0, 0, 0, 0)


def test_delta_where_a_lane_takes_three_passes():
    """The grid is capped at DELTA_MAX_BLOCKS blocks and lanes stride over the vectors: a raster of passes_height() rows takes
    every lane through two whole passes and some lanes through a third; a single differing byte in the last pass, in the first,
    in the second and in the tail."""
    _run('child_delta_passes()')


# ---- apng_encode_device on arbitrary frames --------------------------------------------------------------------------------
def slot_bytes(w):
    """png_slot_bytes (maray_amd/csrc/png_device.hpp), restated."""
    n = 3 * min(w, P.SEG) + 1
    return ((9 * n + 7) // 8 + 16 + 15) // 16 * 16


def row_segments(w):
    return (w + P.SEG - 1) // P.SEG


def encode_frames(frames, stream=0, **kw):
    h, w, _ = frames[0].shape
    buf, ptr = on_device(np.stack(frames), 3)
    return M.apng_encode_device(ptr, len(frames), w, h, stream=stream, **kw)


def check_file(png, frames):
    d = A.decode(png)
    h, w, _ = frames[0].shape
    assert len(d.frames) == len(frames)
    for i, (got, want) in enumerate(zip(d.frames, frames)):
        assert np.array_equal(got, want), i
    want_rects = [(0, 0, w, h)] + [A.rect_of(A.bounding_box(frames[i - 1], frames[i])) for i in range(1, len(frames))]
    assert d.rects == want_rects
    for (x, y, bw, bh), z in zip(d.rects, d.streams):          # the project's own slot bound, not a measured size
        assert len(z) <= bh * row_segments(bw) * slot_bytes(bw) + 11, (bw, bh, len(z))
    return d


def special_frames(w, h=19):
    """A random frame; one with a sub-rectangle replaced; the same again (the empty box); one column changed; one row changed;
    everything changed."""
    f = [P.random_bytes(w, h, w)]
    g = f[-1].copy()
    g[3:11, w // 4:w // 4 + max(1, w // 2)] ^= 0x55
    f.append(g)
    f.append(g.copy())
    g = g.copy()
    g[2:h - 1, w // 2, 1] ^= 0x0F
    f.append(g)
    g = g.copy()
    g[h - 1, :, 2] ^= 0xF0
    f.append(g)
    f.append(P.random_bytes(w + 1, h, w))
    return f


def child_apng_random(w):
    import torch
    for n in (1, 2, 5):
        frames = BR.random_frames(100 * w + n, n, 19, w)
        files = []
        for rows in (None, 1, 3, 1000):
            with band_rows(rows):
                files.append(encode_frames(frames, fps=(30, 1), loops=2))
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            files.append(encode_frames(frames, stream=st.cuda_stream, fps=(30, 1), loops=2))
        d = check_file(files[0], frames)
        assert d.delay == (1, 30) and d.plays == 2
        assert all(f == files[0] for f in files), (w, n)
        buf, ptr = on_device(frames[0], 7)
        assert d.streams[0] == P.idat_stream(M.png_encode_device(ptr, w, 19)), 'frame 0 is not the still of frame 0'
        assert np.array_equal(P.decode(files[0]), frames[0])            # a plain PNG reader shows frame 0


@pytest.mark.parametrize('w', [1, 65, 513])
def test_apng_encode_device_on_random_frames(w):
    """1, 2 and 5 random frames: decoded frames, rectangles (= numpy's bounding boxes), frame 0's stream (= the still's), the
    slot bound per frame, and the same file under every band height and on a non-default stream."""
    _run('child_apng_random(%d)' % w)


def child_apng_special():
    for w in (1, 65, 513):
        frames = special_frames(w)
        files = []
        for rows in (None, 1, 3):
            with band_rows(rows):
                files.append(encode_frames(frames))
        d = check_file(files[0], frames)
        assert all(f == files[0] for f in files), w
        assert d.rects[2] == (0, 0, 1, 1) and d.delay == (1, 25) and d.plays == 0
        assert d.rects[3][2] == 1 and d.rects[4][3] == 1           # one column wide; one row high
    assert sum(len(z) for z in d.streams[1:5]) < len(d.streams[0])     # four partial frames together are smaller than one whole one


def test_apng_encode_device_on_equal_frames_columns_and_rows():
    """Two identical consecutive frames (the 1 x 1 rectangle), a box one column wide, a box one row high, a sub-rectangle whose
    rows are cropped, and a frame that changes everywhere."""
    _run('child_apng_special()')


# ---- Context.render_apng ----------------------------------------------------------------------------------------------------
SMALL = (96, 80)


def slide_values(n):
    return np.array([(-6.0 + 24.0 * i / max(1, n - 1), 2.0 - 12.0 * i / max(1, n - 1)) for i in range(n)])


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_apng_equals_the_contexts_own_renders(backend):
    w, h = SMALL
    scene, names = PR.declared(PR.SCENES['slide'](w, h), SMALL)
    ctx = M.Context(scene.lower(), backend=backend)
    plain = slide_values(4)
    d = A.decode(ctx.render_apng(w, h, plain, fps=12))
    assert len(d.frames) == 4 and d.delay == (1, 12)
    for i in range(4):
        ctx.set_params(plain[i])
        assert np.array_equal(d.frames[i], ctx.render_rows(w, h, 0, h, want_f64=False)[0]), i
        if i:
            assert d.rects[i] == A.rect_of(A.bounding_box(d.frames[i - 1], d.frames[i]))
    sub = slide_values(12)
    with band_rows(16):
        ctx2 = M.Context(scene.lower(), backend=backend)
        d = A.decode(ctx2.render_apng(w, h, sub, sub=4))
        ctx2.close()
    assert len(d.frames) == 3
    for i in range(3):
        assert np.array_equal(d.frames[i], ctx.render_rows_shutter(w, h, 0, h, sub[4 * i:4 * i + 4])), i
    # a value outside its range: refused before any frame is rendered, and the context's values stay
    bad = plain.copy()
    bad[3, 1] = 1000.0
    with pytest.raises(M.MarayError) as e:
        ctx.render_apng(w, h, bad)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        ctx.render_apng(w, h, sub, sub=3)
    assert e.value.code == -1
    assert np.array_equal(ctx.render_rows(w, h, 0, h, want_f64=False)[0], A.decode(ctx.render_apng(w, h, plain[3:4])).frames[0])
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_apng_supersampled_with_tent_and_srgb(backend):
    w, h = SMALL
    scene, names = PR.declared(PR.SCENES['slide'](w, h), SMALL)
    scene.supersample(2)
    ctx = M.Context(scene.lower(), backend=backend, samples=2, filter=M.FILTER_TENT, transfer=M.TRANSFER_SRGB)
    values = slide_values(6)
    d = A.decode(ctx.render_apng(w, h, values, sub=2, loops=1))
    assert len(d.frames) == 3 and d.plays == 1
    for i in range(3):
        assert np.array_equal(d.frames[i], ctx.render_rows_shutter(w, h, 0, h, values[2 * i:2 * i + 2])), i
    ctx.close()


# ---- gen_animation and the CLI ---------------------------------------------------------------------------------------------
ATLAS_W, ATLAS_H, ATLAS_N = 50, 40, 5


def atlas_case():
    """(scene, textures, frames): slice t of the atlas is frame t; slices 1 and 2 differ in a sub-rectangle, 2 and 3 are equal."""
    frames = BR.random_frames(88, ATLAS_N, ATLAS_H, ATLAS_W)
    frames[2] = frames[1].copy()
    frames[2][5:20, 10:30] ^= 0x33
    frames[3] = frames[2].copy()
    scene = BR.atlas_scene()
    scene.set_size(ATLAS_W, ATLAS_H)
    return scene, [BR.atlas(frames)], frames


def test_gen_animation_writes_the_frames_of_gen_to_image(tmp_path):
    M.gen_cache_clear()
    scene, tex, frames = atlas_case()
    scene.set_param('t', 4.0)
    out = str(tmp_path / 'a.png')
    M.gen_animation(scene, out, {'t': range(ATLAS_N)}, fps=(10, 1), loops=3, textures=tex, backend=M.BACKEND_TAPE_SMEM)
    assert scene.param_info(0)[3] == 4.0            # the scene's value is as it was
    d = A.decode(open(out, 'rb').read())
    assert d.delay == (1, 10) and d.plays == 3 and len(d.frames) == ATLAS_N
    assert d.rects[2] == (10, 5, 20, 15) and d.rects[3] == (0, 0, 1, 1)
    for i in range(ATLAS_N):
        want = M.gen_to_image(scene, textures=tex, backend=M.BACKEND_TAPE_SMEM, n_devices=1, params={'t': float(i)})
        assert np.array_equal(want, frames[i]) and np.array_equal(d.frames[i], want), i
    # a second animation finds the program and its context: nothing is lowered, nothing is created
    info = M.gen_cache_info()
    assert len(info) == 1, info
    again = str(tmp_path / 'b.png')
    M.gen_animation(scene, again, np.arange(ATLAS_N, dtype=np.float64)[:, None], fps=(10, 1), loops=3, textures=tex, backend=M.BACKEND_TAPE_SMEM)
    assert M.gen_cache_info() == info
    assert open(again, 'rb').read() == open(out, 'rb').read()
    # a value outside the declared range: an error, no file
    with pytest.raises(M.MarayError) as e:
        M.gen_animation(scene, str(tmp_path / 'c.png'), {'t': [0.0, 100.0]}, textures=tex, backend=M.BACKEND_TAPE_SMEM)
    assert e.value.code == -1 and not os.path.exists(str(tmp_path / 'c.png'))
    with pytest.raises(M.MarayError) as e:
        M.gen_animation(scene, str(tmp_path / 'c.png'), {'t': [0.0, 1.0]}, textures=tex, backend=M.BACKEND_TAPE_SMEM, n_devices=2)
    assert e.value.code == -1
    M.gen_cache_clear()


def test_gen_animation_with_a_shutter(tmp_path):
    M.gen_cache_clear()
    scene, tex, frames = atlas_case()
    scene.set_param('t', 0.0)
    out = str(tmp_path / 'a.png')
    M.gen_animation(scene, out, {'t': [0.5, 2.5]}, textures=tex, backend=M.BACKEND_TAPE_SMEM, shutter=2, spans={'t': 2.0})
    assert scene.param_info(0)[3] == 0.0
    d = A.decode(open(out, 'rb').read())
    for i, t in enumerate((0.5, 2.5)):
        want = M.gen_to_image(scene, textures=tex, backend=M.BACKEND_TAPE_SMEM, n_devices=1, params={'t': t}, shutter=2, spans={'t': 2.0})
        assert np.array_equal(d.frames[i], want), i
        assert np.array_equal(want, BR.mean_general([frames[int(t - 0.5)], frames[int(t + 0.5)]]))
    M.gen_cache_clear()


def test_cli_apng(tmp_path):
    scene, tex, frames = atlas_case()
    path, atlas, out = str(tmp_path / 'atlas.maray'), str(tmp_path / 'atlas.png'), str(tmp_path / 'out.png')
    scene.save(path)
    M.png_write(atlas, tex[0])
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    r = subprocess.run([exe, '-i', path, '-t', atlas, '-o', out, '--backend', 'tape-smem', '--animate', 't=0:%d:%d' % (ATLAS_N - 1, ATLAS_N),
                        '--apng', '--fps', '30/2', '--loops', '4', '--gpus', '1'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = A.decode(open(out, 'rb').read())
    assert d.delay == (2, 30) and d.plays == 4 and len(d.frames) == ATLAS_N
    for i in range(ATLAS_N):
        assert np.array_equal(d.frames[i], frames[i]), i
    assert os.listdir(str(tmp_path)).count('out.png') == 1 and len(os.listdir(str(tmp_path))) == 3
