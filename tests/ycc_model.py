"""The raw-video contract (include/maray_hip.h, "raw video") restated for the tests of tests/test_ycc.py, test_ycc_abi.py and
test_gpu_ycc.py: the conversion twice -- `contract`, the header's sentences as a double loop over Python integers, and
`planes`, the same separably in numpy, which the tests pin against the loop -- and a YUV4MPEG2 parser that trusts nothing in
the file.  Neither conversion clamps: the contract says the values need none, and a model that clamped would hide a kernel
that does not.
"""
import re

import numpy as np

YCC_420, YCC_444 = 0, 1
BT601, BT709 = 0, 1
SAMPLINGS, MATRICES = (YCC_420, YCC_444), (BT601, BT709)
# the coefficient rows (y; cb; cr)
COEFF = {BT601: ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
         BT709: ((47, 157, 16), (-26, -86, 112), (112, -102, -10))}


def chroma_size(w, h, sampling):
    return (w, h) if sampling == YCC_444 else ((w + 1) // 2, (h + 1) // 2)


def frame_bytes(w, h, sampling):
    cw, ch = chroma_size(w, h, sampling)
    return w * h + 2 * cw * ch


def contract(rgb, sampling=YCC_420, matrix=BT601):
    """(Y', Cb, Cr) as lists of rows of Python integers: the header's sentences, pixel by pixel (>> of a Python int floors)."""
    h, w = len(rgb), len(rgb[0])
    ky, kb, kr = COEFF[matrix]

    def dot(c, p):
        return c[0] * int(p[0]) + c[1] * int(p[1]) + c[2] * int(p[2])
    y = [[((dot(ky, rgb[j][i]) + 128) >> 8) + 16 for i in range(w)] for j in range(h)]
    cw, ch = chroma_size(w, h, sampling)
    cb, cr = [[0] * cw for _ in range(ch)], [[0] * cw for _ in range(ch)]
    for j in range(ch):
        for i in range(cw):
            if sampling == YCC_444:
                cb[j][i] = ((dot(kb, rgb[j][i]) + 128) >> 8) + 128
                cr[j][i] = ((dot(kr, rgb[j][i]) + 128) >> 8) + 128
            else:
                s = [0, 0, 0]
                for b in (0, 1):
                    for a in (0, 1):
                        p = rgb[min(2 * j + b, h - 1)][min(2 * i + a, w - 1)]
                        s = [s[k] + int(p[k]) for k in range(3)]
                cb[j][i] = ((dot(kb, s) + 512) >> 10) + 128
                cr[j][i] = ((dot(kr, s) + 512) >> 10) + 128
    return y, cb, cr


def planes(rgb, sampling=YCC_420, matrix=BT601):
    """(Y', Cb, Cr) of an (h, w, 3) uint8 raster as int64 arrays, unclamped.  Separable: at 4:2:0 the columns are summed in
    pairs (the last one with itself where w is odd), then the rows."""
    a = np.asarray(rgb).astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == 3 and a.shape[0] and a.shape[1]
    h, w, _ = a.shape
    ky, kb, kr = (np.array(c, np.int64) for c in COEFF[matrix])
    y = ((a @ ky + 128) >> 8) + 16
    if sampling == YCC_444:
        return y, ((a @ kb + 128) >> 8) + 128, ((a @ kr + 128) >> 8) + 128
    xs = np.minimum(np.arange(0, w + 1, 2)[:(w + 1) // 2, None] + np.arange(2)[None, :], w - 1)           # (cw, 2)
    ys = np.minimum(np.arange(0, h + 1, 2)[:(h + 1) // 2, None] + np.arange(2)[None, :], h - 1)           # (ch, 2)
    cols = a[:, xs[:, 0]] + a[:, xs[:, 1]]                                                                  # (h, cw, 3)
    s = cols[ys[:, 0]] + cols[ys[:, 1]]                                                                     # (ch, cw, 3)
    return y, ((s @ kb + 512) >> 10) + 128, ((s @ kr + 512) >> 10) + 128


def frame(rgb, sampling=YCC_420, matrix=BT601):
    """The payload of one FRAME: the three planes as bytes, one after the other.  A value outside a byte is an error of the
    contract's, not something to clamp."""
    out = []
    for p in planes(rgb, sampling, matrix):
        assert p.min() >= 0 and p.max() <= 255
        out.append(p.astype(np.uint8).tobytes())
    return b''.join(out)


def header(w, h, fps, sampling):
    """The header line for fps = (N, D): F N:D, not reduced."""
    return b'YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=LIMITED\n' % (w, h, fps[0], fps[1], b'C444' if sampling == YCC_444 else b'C420jpeg')


def build(frames, fps=(25, 1), sampling=YCC_420, matrix=BT601):
    """The file the contract describes for a list of (h, w, 3) uint8 rasters."""
    h, w, _ = frames[0].shape
    return header(w, h, fps, sampling) + b''.join(b'FRAME\n' + frame(f, sampling, matrix) for f in frames)


class Y4m:
    pass


_HEADER = re.compile(rb'YUV4MPEG2 W([1-9][0-9]*) H([1-9][0-9]*) F([1-9][0-9]*):([1-9][0-9]*) Ip A1:1 (C420jpeg|C444) XCOLORRANGE=LIMITED')


def parse(data):
    """A Y4M file of this library's -> .w, .h, .fps (N, D), .sampling, .frames: a list of (Y', Cb, Cr) uint8 arrays.  Every
    byte is accounted for: the one header line in exactly the contract's form, then whole frames, each behind `FRAME\\n`, and
    nothing after the last."""
    assert isinstance(data, (bytes, bytearray))
    end = data.find(b'\n')
    assert end > 0, 'no header line'
    m = _HEADER.fullmatch(bytes(data[:end]))
    assert m, 'header %r' % bytes(data[:end])
    d = Y4m()
    d.w, d.h, d.fps = int(m.group(1)), int(m.group(2)), (int(m.group(3)), int(m.group(4)))
    d.sampling = YCC_444 if m.group(5) == b'C444' else YCC_420
    cw, ch = chroma_size(d.w, d.h, d.sampling)
    n = frame_bytes(d.w, d.h, d.sampling)
    d.frames = []
    at = end + 1
    assert at < len(data), 'no frame'
    while at < len(data):
        assert data[at:at + 6] == b'FRAME\n', 'frame %d does not begin with FRAME' % len(d.frames)
        at += 6
        assert at + n <= len(data), 'frame %d is cut short' % len(d.frames)
        buf = np.frombuffer(bytes(data[at:at + n]), np.uint8)
        d.frames.append((buf[:d.w * d.h].reshape(d.h, d.w), buf[d.w * d.h:d.w * d.h + cw * ch].reshape(ch, cw), buf[d.w * d.h + cw * ch:].reshape(ch, cw)))
        at += n
    assert at == len(data)
    return d


def frames_equal(parsed, rasters, matrix=BT601):
    """Every parsed frame's planes are the model's of the raster, byte for byte."""
    assert len(parsed.frames) == len(rasters)
    for i, (got, rgb) in enumerate(zip(parsed.frames, rasters)):
        want = planes(rgb, parsed.sampling, matrix)
        for name, g, w_ in zip(("Y'", 'Cb', 'Cr'), got, want):
            assert g.shape == w_.shape and np.array_equal(g.astype(np.int64), w_), (i, name)
    return True
