"""Raw video on the device (include/maray_hip.h, "raw video"): maray_rgb_to_ycc against tests/ycc_model.py byte for byte,
y4m_encode_device on arbitrary frames, Context.render_y4m on the three back-ends, gen_animation through both containers and
the CLI's --y4m.  Every file is taken apart by ycc_model.parse, which trusts nothing in it.

Device rasters for rgb_to_ycc and y4m_encode_device are torch tensors: those tests run in child processes that import torch
before the library, as tests/test_gpu_apng.py does.  No test sets MARAY_PNG_BAND_ROWS: this path has no PNG encoder."""
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
import ycc_model as Y

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BACKENDS = [M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM, M.BACKEND_JIT]
GUARD = 16
HEIGHTS = (1, 2, 3, 19)
EDGE_BYTES = np.array([0, 1, 127, 128, 254, 255], np.uint8)       # both sides of every shift's rounding


# ---- the launch constants, from the sources (as tests/reduce_passes.py reads the reduces') ---------------------------------
def ycc_constants():
    """(lanes of a block, pixels of a lane, the cap of the grid, pixels a wavefront spans, pixels and rows a block spans)."""
    hpp = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'yuv.hpp')).read()
    hip = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'yuv.hip')).read()
    m = re.findall(r'constexpr uint32_t YCC_BLOCK = (\d+), YCC_LANE_PIXELS = (\d+), YCC_MAX_BLOCKS = (\d+);', hpp)
    assert len(m) == 1
    block, lane_pixels, max_blocks = (int(v) for v in m[0])
    # the arithmetic restated here and in tiles(), line by line
    for text, line in ((hpp, 'constexpr uint32_t YCC_WAVE_PIXELS = 64 * YCC_LANE_PIXELS;'),
                       (hpp, 'constexpr uint32_t YCC_BLOCK_PIXELS = YCC_WAVE_PIXELS, YCC_BLOCK_ROWS = 2 * (YCC_BLOCK / 64);'),
                       (hpp, 'inline uint32_t ycc_tiles_x(uint32_t w) { return (w + YCC_BLOCK_PIXELS - 1) / YCC_BLOCK_PIXELS; }'),
                       (hpp, 'inline uint32_t ycc_tiles_y(uint32_t h) { return (h + YCC_BLOCK_ROWS - 1) / YCC_BLOCK_ROWS; }'),
                       (hpp, 'return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), YCC_MAX_BLOCKS);'),
                       (hip, 'for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)')):
        assert line in text, 'the conversion no longer reads %r: restate it in tests/test_gpu_ycc.py' % line
    wave_pixels = 64 * lane_pixels
    return block, lane_pixels, max_blocks, wave_pixels, wave_pixels, 2 * (block // 64)


def tiles(w, h):
    """(tiles, blocks of the grid) of a w x h conversion."""
    block, lane_pixels, max_blocks, wave_pixels, block_pixels, block_rows = ycc_constants()
    n = ((w + block_pixels - 1) // block_pixels) * ((h + block_rows - 1) // block_rows)
    return n, min(max(n, 1), max_blocks)


def widths():
    """1, 2, 3, 5, 63, 64, 65, and one below, at and one above a lane's, a wavefront's and a block's span of pixels."""
    block, lane_pixels, max_blocks, wave_pixels, block_pixels, block_rows = ycc_constants()
    out = {1, 2, 3, 5, 63, 64, 65}
    for span in (lane_pixels, wave_pixels, block_pixels):
        out |= {span - 1, span, span + 1}
    return sorted(v for v in out if v >= 1)


def passes_shapes():
    """(w, h) at which the grid IS capped and a block takes more than one pass: one tile column of five pixels, high enough for
    two whole passes and a ragged third whose last tile holds three rows, the last of them unpaired; and two tile columns, the
    second one pixel wide, just past the cap."""
    block, lane_pixels, max_blocks, wave_pixels, block_pixels, block_rows = ycc_constants()
    return [(5, block_rows * (2 * max_blocks + 5) + 3), (block_pixels + 1, block_rows * (max_blocks // 2) + 3)]


def test_the_multi_pass_shapes_are_what_they_are_for():
    """(no device) The shapes are derived from the exported constants: more tiles than the grid has blocks."""
    block, lane_pixels, max_blocks, wave_pixels, block_pixels, block_rows = ycc_constants()
    (w0, h0), (w1, h1) = passes_shapes()
    n, grid = tiles(w0, h0)
    assert grid == max_blocks and 2 * grid < n < 3 * grid and h0 % 2 == 1 and h0 % block_rows == 3
    n, grid = tiles(w1, h1)
    assert grid == max_blocks and grid < n < 2 * grid and w1 > block_pixels
    assert 3 * w0 * h0 < 1 << 20 and 3 * w1 * h1 < 16 << 20                # small rasters all the same
    assert set(widths()) >= {lane_pixels - 1, lane_pixels + 1, wave_pixels - 1, wave_pixels, wave_pixels + 1}


# ---- children ----------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_ycc as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=600):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


def on_device(a, offset=0):
    """(tensor, pointer): a's bytes in device memory, `offset` bytes into a torch buffer.  (In a child process: torch.)"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.zeros(flat.size + offset + 16, dtype=torch.uint8, device='cuda')
    buf[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def convert(rgb, sampling, matrix, src_off=0, dst_off=0, stream=0):
    """The device's planes of an (h, w, 3) raster, with the guard bytes around them checked."""
    import torch
    h, w, _ = rgb.shape
    n = M.ycc_frame_bytes(w, h, sampling)
    src, p_src = on_device(rgb, src_off)
    dst = torch.full((GUARD + dst_off + n + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    M.rgb_to_ycc(p_src, w, h, dst.data_ptr() + GUARD + dst_off, sampling, matrix, stream=stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.all(out[:GUARD + dst_off] == 0xA5) and np.all(out[GUARD + dst_off + n:] == 0xA5), 'a guard byte was written'
    return out[GUARD + dst_off:GUARD + dst_off + n]


def check(rgb, sampling, matrix, what, **kw):
    got = convert(rgb, sampling, matrix, **kw)
    want = np.frombuffer(Y.frame(rgb, sampling, matrix), np.uint8)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, rgb.shape, sampling, matrix, kw, 'first differing plane byte', at, int(got[at]), int(want[at])))


def rasters(seed, h, w):
    """Random bytes; bytes over EDGE_BYTES; a constant raster."""
    rng = np.random.default_rng(seed)
    return [('random', rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
            ('edges', EDGE_BYTES[rng.integers(0, 6, (h, w, 3))]),
            ('constant', np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy())]


def child_sizes(sampling):
    for w in widths():
        for h in HEIGHTS:
            for matrix in Y.MATRICES:
                for name, rgb in rasters(1000 * w + 10 * h + matrix, h, w):
                    check(rgb, sampling, matrix, name)


@pytest.mark.parametrize('sampling', Y.SAMPLINGS)
def test_rgb_to_ycc_at_every_width_and_height(sampling):
    """Widths around a lane's, a wavefront's and a block's span and the small ones, heights 1, 2, 3 and 19, both matrices, the
    three kinds of bytes: the planes are the model's and the guard bytes around them are untouched."""
    _run('child_sizes(%d)' % sampling)


def child_alignment():
    import torch
    for w in (5, 65):
        for sampling in Y.SAMPLINGS:
            rgb = rasters(w + sampling, 7, w)[0][1]
            for src_off in range(4):
                for dst_off in range(4):
                    check(rgb, sampling, Y.BT601 if (src_off + dst_off) % 2 else Y.BT709, 'offsets', src_off=src_off, dst_off=dst_off)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        check(rasters(9, 19, 65)[1][1], Y.YCC_420, Y.BT601, 'a stream of the caller', src_off=1, dst_off=3, stream=st.cuda_stream)


def test_rgb_to_ycc_at_every_pair_of_byte_offsets():
    """Source offsets 0 - 3 and destination offsets 0 - 3 at w = 5 and 65; and once on a non-default stream."""
    _run('child_alignment()')


def child_passes():
    for (w, h), sampling in zip(passes_shapes(), (Y.YCC_420, Y.YCC_444)):
        n, grid = tiles(w, h)
        assert n > grid
        rgb = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        check(rgb, sampling, Y.BT601, 'passes')
    w, h = passes_shapes()[0]
    check(EDGE_BYTES[np.random.default_rng(3).integers(0, 6, (h, w, 3))], Y.YCC_444, Y.BT709, 'passes', src_off=1, dst_off=1)


def test_rgb_to_ycc_where_a_block_takes_more_than_one_pass():
    """The grid is capped at YCC_MAX_BLOCKS and blocks stride over the tiles: rasters of passes_shapes() take some blocks through
    three passes, the last tile ragged."""
    _run('child_passes()')


# ---- y4m_encode_device --------------------------------------------------------------------------------------------------------
def child_encode():
    import torch
    for w, h in ((67, 41), (1, 1)):
        frames = BR.random_frames(100 * w + h, 3, h, w)
        buf, ptr = on_device(np.stack(frames), 3)
        for sampling in Y.SAMPLINGS:
            for matrix in Y.MATRICES:
                data = M.y4m_encode_device(ptr, 3, w, h, fps=(30000, 1001), sampling=sampling, matrix=matrix)
                head = b'YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 %s XCOLORRANGE=LIMITED\n' % (w, h, b'C444' if sampling else b'C420jpeg')
                assert data.startswith(head)
                assert len(data) == len(head) + 3 * (6 + Y.frame_bytes(w, h, sampling))
                d = Y.parse(data)
                assert (d.w, d.h, d.fps, d.sampling) == (w, h, (30000, 1001), sampling)
                assert Y.frames_equal(d, frames, matrix)
                assert data == Y.build(frames, (30000, 1001), sampling, matrix)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            assert M.y4m_encode_device(ptr, 3, w, h, stream=st.cuda_stream) == Y.build(frames)
        assert M.y4m_encode_device(ptr, 1, w, h, fps=12) == Y.build(frames[:1], (12, 1))
        assert M.y4m_encode_device(ptr, 2, w, h, fps=(0, 4))[:40].split(b' ')[3] == b'F100:4'          # delay_den = 0 means 100


def test_y4m_encode_device_on_random_frames():
    """Three random frames of 67 x 41 and of 1 x 1: the parsed planes are the model's, the header is the contract's, the length
    is exact; the same bytes on a stream of the caller's; one frame; a denominator of 0."""
    _run('child_encode()')


# ---- Context.render_y4m ---------------------------------------------------------------------------------------------------------
SMALL = (96, 80)


def slide_values(n):
    return np.array([(-6.0 + 24.0 * i / max(1, n - 1), 2.0 - 12.0 * i / max(1, n - 1)) for i in range(n)])


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_y4m_is_the_model_of_the_contexts_own_renders(backend):
    w, h = SMALL
    scene, names = PR.declared(PR.SCENES['slide'](w, h), SMALL)
    ctx = M.Context(scene.lower(), backend=backend)
    plain = slide_values(4)
    rendered = []
    for i in range(4):
        ctx.set_params(plain[i])
        rendered.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
    assert any(not np.array_equal(rendered[0], r) for r in rendered[1:])            # an animation: the frames differ
    for sampling, matrix in ((M.YCC_420, M.YCC_BT601), (M.YCC_444, M.YCC_BT709)):
        data = ctx.render_y4m(w, h, plain, fps=12, sampling=sampling, matrix=matrix)
        d = Y.parse(data)
        assert (d.w, d.h, d.fps, d.sampling) == (w, h, (12, 1), sampling)
        assert Y.frames_equal(d, rendered, matrix)
        assert data == Y.build(rendered, (12, 1), sampling, matrix)
    # n_sub = 2: every image the shutter's mean of its two rows
    sub = slide_values(6)
    d = Y.parse(ctx.render_y4m(w, h, sub, sub=2))
    assert Y.frames_equal(d, [ctx.render_rows_shutter(w, h, 0, h, sub[2 * i:2 * i + 2]) for i in range(3)])
    # a value outside its range: refused before any frame is rendered, and the context's values stay
    bad = plain.copy()
    bad[3, 1] = 1000.0
    with pytest.raises(M.MarayError) as e:
        ctx.render_y4m(w, h, bad)
    assert e.value.code == -1
    with pytest.raises(M.MarayError) as e:
        ctx.render_y4m(w, h, sub, sub=4)
    assert e.value.code == -1
    assert Y.frames_equal(Y.parse(ctx.render_y4m(w, h, plain[3:4])), [ctx.render_rows(w, h, 0, h, want_f64=False)[0]])
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_y4m_supersampled_with_tent(backend):
    w, h = SMALL
    scene, names = PR.declared(PR.SCENES['slide'](w, h), SMALL)
    scene.supersample(2)
    ctx = M.Context(scene.lower(), backend=backend, samples=2, filter=M.FILTER_TENT)
    values = slide_values(3)
    d = Y.parse(ctx.render_y4m(w, h, values))
    assert Y.frames_equal(d, [ctx.render_rows_shutter(w, h, 0, h, values[i:i + 1]) for i in range(3)])
    ctx.close()


# ---- gen_animation and the CLI -----------------------------------------------------------------------------------------------
ATLAS_W, ATLAS_H, ATLAS_N = 51, 39, 5


def atlas_case():
    """(scene, textures, frames): slice t of the atlas is frame t."""
    frames = BR.random_frames(89, ATLAS_N, ATLAS_H, ATLAS_W)
    scene = BR.atlas_scene()
    scene.set_size(ATLAS_W, ATLAS_H)
    return scene, [BR.atlas(frames)], frames


def test_gen_animation_through_both_containers(tmp_path):
    M.gen_cache_clear()
    scene, tex, frames = atlas_case()
    scene.set_param('t', 4.0)
    values = np.arange(ATLAS_N, dtype=np.float64)[:, None]
    kw = dict(fps=(10, 1), textures=tex, backend=M.BACKEND_TAPE_SMEM)
    out = str(tmp_path / 'a.y4m')
    M.gen_animation(scene, out, {'t': range(ATLAS_N)}, container=M.CONTAINER_Y4M, loops=3, codes=M.CODES_DYNAMIC, **kw)
    assert scene.param_info(0)[3] == 4.0            # the scene's value is as it was
    data = open(out, 'rb').read()
    assert Y.frames_equal(Y.parse(data), frames) and data == Y.build(frames, (10, 1))
    ctx = M.Context(scene.lower(), textures=tex, backend=M.BACKEND_TAPE_SMEM)
    assert data == ctx.render_y4m(ATLAS_W, ATLAS_H, values, fps=(10, 1))
    for sampling, matrix in ((M.YCC_444, M.YCC_BT601), (M.YCC_420, M.YCC_BT709)):
        M.gen_animation(scene, out, values, container=M.CONTAINER_Y4M, sampling=sampling, matrix=matrix, **kw)
        assert open(out, 'rb').read() == ctx.render_y4m(ATLAS_W, ATLAS_H, values, fps=(10, 1), sampling=sampling, matrix=matrix)
    ctx.close()
    # the APNG container is maray_gen_animation's file, byte for byte (fixed codes)
    a, b = str(tmp_path / 'a.png'), str(tmp_path / 'b.png')
    M.gen_animation(scene, a, values, container=M.CONTAINER_APNG, loops=3, **kw)
    arr, n, keep = M.api._textures(tex)
    go = M.GenOpts()
    go.backend = M.BACKEND_TAPE_SMEM
    import ctypes as C
    assert M.lib().maray_gen_animation(scene._h, arr, n, C.byref(go), values.ctypes.data, ATLAS_N, 1, 10, 3, os.fsencode(b)) == 0
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert all(np.array_equal(x, y) for x, y in zip(A.decode(open(a, 'rb').read()).frames, frames))
    # a value outside the declared range, and two devices: an error, no file
    bad = str(tmp_path / 'c.y4m')
    with pytest.raises(M.MarayError) as e:
        M.gen_animation(scene, bad, {'t': [0.0, 100.0]}, container=M.CONTAINER_Y4M, **kw)
    assert e.value.code == -1 and not os.path.exists(bad)
    with pytest.raises(M.MarayError) as e:
        M.gen_animation(scene, bad, {'t': [0.0, 1.0]}, container=M.CONTAINER_Y4M, n_devices=2, **kw)
    assert e.value.code == -1 and not os.path.exists(bad)
    M.gen_cache_clear()


CLI_W, CLI_H, CLI_N = 96, 832, 3


def test_cli_y4m_on_chess_slide(tmp_path):
    """`maray_scenes`' chess_slide_1024 cut to a strip of 96 x 832 over which the board's left edge slides: three frames as 4:2:0 BT.709, parsed
    and compared with the model of gen_to_image's rasters of the same values."""
    tmp = str(tmp_path)
    bin_dir = os.path.dirname(M.lib_path())
    subprocess.check_call([os.path.join(bin_dir, 'maray_scenes'), tmp, 'chess_slide_1024'], stdout=subprocess.DEVNULL)
    scene = M.Scene.open(os.path.join(tmp, 'chess_slide_1024.maray'))
    scene.set_size(CLI_W, CLI_H)
    path, out = os.path.join(tmp, 'strip.maray'), os.path.join(tmp, 'out.y4m')
    scene.save(path)
    r = subprocess.run([os.path.join(bin_dir, 'maray'), '-i', path, '-o', out, '--backend', 'tape-smem', '--animate', 't=-200:200:%d' % CLI_N, '--y4m',
                        '--y4m-matrix', '709', '--fps', '24', '--gpus', '1'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = Y.parse(open(out, 'rb').read())
    assert (d.w, d.h, d.fps, d.sampling, len(d.frames)) == (CLI_W, CLI_H, (24, 1), Y.YCC_420, CLI_N)
    scene.declare_param('t', -200.0, 200.0)
    want = [M.gen_to_image(scene, backend=M.BACKEND_TAPE_SMEM, n_devices=1, params={'t': t}) for t in (-200.0, 0.0, 200.0)]
    assert not np.array_equal(want[0], want[1]) and len(np.unique(want[0].reshape(-1, 3), axis=0)) == 2          # black and white squares
    assert Y.frames_equal(d, want, Y.BT709)
    assert sorted(os.listdir(tmp)) == ['chess_slide_1024.maray', 'out.y4m', 'strip.maray']
    M.gen_cache_clear()
