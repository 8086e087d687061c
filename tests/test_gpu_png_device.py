"""The device PNG encoder on the device (include/maray_hip.h, "device PNG encoder"): every file is decoded by
tests/png_stream.py -- signature, CRCs, IHDR, zlib.decompress with its Adler-32, length, unfilter -- and by the library's
own reader, and the decoded raster is compared with the input by np.array_equal.

Device rasters for png_encode_device are torch tensors (those tests run in child processes that import torch before the
library); for Context.render_png they come from the texture-identity scene of tests/byte_rasters.py, whose context renders
whatever bytes the test chooses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import maray_amd as M
import png_stream as P
from test_gpu_supersample import BACKENDS, scene_case, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
SEG = P.SEG

_tape = []


def identity_tape():
    if not _tape:
        _tape.append(BR.identity_scene().lower())
    return _tape[0]


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


def on_device(img, offset=0):
    """(tensor, pointer): img's bytes in device memory, `offset` bytes into a torch buffer.  (In a child process: torch.)"""
    import torch
    flat = np.ascontiguousarray(img).reshape(-1)
    buf = torch.zeros(flat.size + offset + 16, dtype=torch.uint8, device='cuda')
    buf[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def encode_tensor(img, offset=0, stream=0):
    buf, ptr = on_device(img, offset)
    return M.png_encode_device(ptr, img.shape[1], img.shape[0], stream=stream)


def render_png_of(img, backend=M.BACKEND_TAPE_SMEM):
    ctx = M.Context(identity_tape(), textures=[img], backend=backend)
    png = ctx.render_png(img.shape[1], img.shape[0])
    ctx.close()
    return png


def check(png, img, tmp_path):
    assert np.array_equal(P.decode(png), img)
    path = str(tmp_path / 'check.png')
    with open(path, 'wb') as f:
        f.write(png)
    assert np.array_equal(M.png_read(path), img)


# ---- the tests on torch tensors: each in a child process that imports torch first ----------------------------------------
# (torch brings a HIP runtime of its own: in a process that has loaded the library first it finds no device, and the whole
# suite loads the library long before this file runs; as tests/test_gpu_fuzz_params.py does)
_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_png_device as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=300):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


def _tmp():
    import pathlib
    import tempfile
    return pathlib.Path(tempfile.mkdtemp(prefix='png_device_'))


# ---- random bytes ------------------------------------------------------------------------------------------------------
def child_random_bytes():
    img = P.random_bytes(0, 37, 65)
    tmp = _tmp()
    a = encode_tensor(img)
    check(a, img, tmp)
    b = render_png_of(img)
    check(b, img, tmp)
    assert a == b


def test_random_bytes_through_both_entry_points():
    """65 x 37 random bytes: literals below and above 143 take 8 and 9 bits."""
    _run('child_random_bytes()')


# ---- geometry ----------------------------------------------------------------------------------------------------------
def child_geometry():
    tmp = _tmp()
    for w in P.GEOMETRY_WS:
        for h in P.GEOMETRY_HS:
            img = P.random_bytes(100 * w + h, h, w)
            img[h // 2, w // 3:w // 3 + 70] = 77          # (a run too, where the row is long enough)
            files = []
            for rows in P.BAND_ROWS:
                with band_rows(rows):
                    files.append(encode_tensor(img))
                    files.append(render_png_of(img))
            check(files[0], img, tmp)
            assert all(f == files[0] for f in files), (w, h)


def test_geometry_and_band_cuts():
    """Every width around the step (64) and the segment (SEG), at heights 1, 2 and 19, in bands of 1, 3 and 1000 rows, through
    both entry points: every cut decodes right and the file's bytes do not depend on the cut."""
    _run('child_geometry()')


def child_many_segments():
    tmp = _tmp()
    for h in (65537, 70001, 140000):
        img = P.random_bytes(h, h, 3)
        img[1000:1200] = 5              # rows of one run, shorter than their neighbours
        png = encode_tensor(img)
        check(png, img, tmp)
        with band_rows(60000):          # and cut into bands of single groups: the same file
            assert encode_tensor(img) == png, h


def test_more_segments_in_a_band_than_the_scan_has_single_groups_for():
    """Up to 65,536 segments a band's lengths are summed in groups of 64; past that the groups grow (128 at 70,001 segments,
    192 at 140,000).  Three pixels a row: a small raster with many segments, all in one band by the default budget."""
    _run('child_many_segments()')


# ---- source alignment --------------------------------------------------------------------------------------------------
def child_alignment():
    tmp = _tmp()
    for w in P.ALIGN_WS:
        img = P.random_bytes(300 + w, 7, w)
        files = [encode_tensor(img, offset=o) for o in range(16)]
        check(files[0], img, tmp)
        assert all(f == files[0] for f in files), w


def test_source_at_every_byte_offset():
    """The device raster starts at every offset 0 .. 15 of a torch buffer; widths 1, 5 and 65."""
    _run('child_alignment()')


# ---- runs --------------------------------------------------------------------------------------------------------------
def child_runs():
    tmp = _tmp()
    for name, img in P.run_rasters():
        try:
            check(encode_tensor(img), img, tmp)
            if img.shape[1] <= 600:
                check(render_png_of(img), img, tmp)
        except AssertionError:
            raise AssertionError(name)


def test_runs():
    """The rasters of tests/png_stream.py on which the bit packing and the run logic can go wrong."""
    _run('child_runs()')


# ---- sizes -------------------------------------------------------------------------------------------------------------
def child_sizes():
    const = np.full((64, 256, 3), 7, np.uint8)
    z = P.idat_stream(encode_tensor(const))
    print('constant 256 x 64: %d bytes of stream for %d filtered bytes' % (len(z), 64 * (3 * 256 + 1)))
    assert len(z) < 49216 // 16
    z = P.idat_stream(encode_tensor(P.random_bytes(0, 37, 65)))
    print('random 65 x 37: %d bytes of stream' % len(z))
    assert len(z) <= -(-9 * 7252 // 8) + 16 * 37 + 100


def test_a_constant_raster_shrinks_and_random_bytes_stay_within_the_bound():
    print(_run('child_sizes()'))


# ---- streams and reuse -------------------------------------------------------------------------------------------------
def child_streams():
    import torch
    tmp = _tmp()
    a, b, big = P.random_bytes(21, 30, 100), P.random_bytes(22, 30, 100), P.random_bytes(23, 90, 700)
    big[10:20, 100:600] = 3
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ta, pa = on_device(a)
        tb, pb = on_device(b)
        fa = M.png_encode_device(pa, 100, 30, stream=st.cuda_stream)
        fb = M.png_encode_device(pb, 100, 30, stream=st.cuda_stream)
    fbig = encode_tensor(big)
    check(fa, a, tmp)
    check(fb, b, tmp)
    check(fbig, big, tmp)


def test_two_streams_and_growing_scratch():
    """Two different rasters back to back on a non-default torch stream, then a larger one on the default stream."""
    _run('child_streams()')


# ---- through contexts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_of_a_scene_equals_render_rows(backend, tmp_path):
    data, w, h, tex = scene_case('all_ops')
    ctx = M.Context(M.Scene(data).lower(), textures=tex, backend=backend)
    want, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    with band_rows(16):
        ctx2 = M.Context(M.Scene(data).lower(), textures=tex, backend=backend)
        check(ctx2.render_png(w, h), want, tmp_path)
        ctx2.close()
    check(ctx.render_png(w, h), want, tmp_path)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_supersampled_with_the_tent_filter(backend, tmp_path):
    data, w, h, tex = scene_case('all_ops')
    ctx = M.Context(supersampled(data, 2).lower(), textures=tex, backend=backend, samples=2, filter=M.FILTER_TENT)
    want, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    check(ctx.render_png(w, h), want, tmp_path)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_of_a_shutter_call(backend, tmp_path):
    frames = BR.random_frames(77, 4, 23, 50)
    ctx = M.Context(BR.atlas_scene().lower(), textures=[BR.atlas(frames)], backend=backend)
    values = np.arange(4, dtype=np.float64)[:, None]
    want = ctx.render_rows_shutter(50, 23, 0, 23, values)
    assert np.array_equal(want, BR.mean_general(frames))
    check(ctx.render_png(50, 23, frames=values), want, tmp_path)
    with pytest.raises(M.MarayError) as e:          # a value outside its range: refused like the shutter entry points refuse it
        ctx.render_png(50, 23, frames=np.array([[0.0], [1.0], [2.0], [1000.0]]))
    assert e.value.code == -1
    ctx.close()


# ---- through gen -------------------------------------------------------------------------------------------------------
def chess_scene(chess_bytes):
    """The chess fixture at its own 1024 x 1024.  (Scene.rescale only enlarges, and the top left 512 x 512 of the picture is one
    flat colour, so neither a rescale nor a crop gives a 256 x 256 chess picture with anything in it.)"""
    s = M.Scene(chess_bytes)
    assert s.size == (1024, 1024)
    return s


@pytest.mark.parametrize('report', [False, True])
def test_gen_with_the_device_encoder(chess_bytes, report, tmp_path):
    s = chess_scene(chess_bytes)
    want = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM)
    out = str(tmp_path / 'gen.png')
    M.gen(s, out, backend=M.BACKEND_TAPE_SMEM, encoder=M.ENCODER_DEVICE, **(dict(report_kind=M.api.REPORT_ROW, report_value=10) if report else {}))
    check(open(out, 'rb').read(), want, tmp_path)
    host = str(tmp_path / 'host.png')
    M.gen(s, host, backend=M.BACKEND_TAPE_SMEM)
    assert np.array_equal(M.png_read(host), want)


def test_cli_with_the_device_encoder(chess_bytes, tmp_path):
    scene = str(tmp_path / 'chess.maray')
    s = chess_scene(chess_bytes)
    s.save(scene)
    want = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM)
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    out = str(tmp_path / 'cli.png')
    r = subprocess.run([exe, '-i', scene, '-o', out, '--backend', 'tape-smem', '--encoder', 'device'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    check(open(out, 'rb').read(), want, tmp_path)


def test_gen_on_two_devices_writes_the_single_device_file(chess_bytes, tmp_path):
    if M.device_count() < 2:
        pytest.skip('needs >= 2 HIP devices')
    s = chess_scene(chess_bytes)
    one, two = str(tmp_path / 'one.png'), str(tmp_path / 'two.png')
    M.gen(s, one, backend=M.BACKEND_TAPE_SMEM, n_devices=1, encoder=M.ENCODER_DEVICE)
    M.gen(s, two, backend=M.BACKEND_TAPE_SMEM, n_devices=2, encoder=M.ENCODER_DEVICE)
    assert open(one, 'rb').read() == open(two, 'rb').read()


def test_gen_with_two_workers_on_the_devices_present(chess_bytes, tmp_path, monkeypatch):
    """The multi-device assembly on any box: two workers, each with a context and an encoder, wrapped onto the devices there
    are (MARAY_GEN_WRAP_DEVICES); the file is the one-worker file."""
    monkeypatch.setenv('MARAY_GEN_WRAP_DEVICES', '1')
    s = chess_scene(chess_bytes)
    one, two = str(tmp_path / 'one.png'), str(tmp_path / 'two.png')
    M.gen(s, one, backend=M.BACKEND_TAPE_SMEM, n_devices=1, encoder=M.ENCODER_DEVICE)
    M.gen(s, two, backend=M.BACKEND_TAPE_SMEM, n_devices=2, encoder=M.ENCODER_DEVICE)
    assert open(one, 'rb').read() == open(two, 'rb').read()
    check(open(two, 'rb').read(), M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1), tmp_path)
