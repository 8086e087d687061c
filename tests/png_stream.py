"""A PNG decoder that checks everything on the way, and the rasters of the device encoder's tests (no device needed):
the helper of tests/test_png_device_abi.py and tests/test_gpu_png_device.py.

decode() takes the bytes of a file and trusts nothing in it: the signature, every chunk's CRC-32, the IHDR fields, the zlib
stream of the joined IDATs (zlib.decompress checks the Adler-32), the length h (3 w + 1) of the filtered data, and every
filter type 0 .. 4, unfiltered in numpy.
"""
import struct
import zlib

import numpy as np

SEG = 256               # pixels per segment of the device encoder's stream (include/maray_hip.h, "device PNG encoder")
SIGNATURE = b'\x89PNG\r\n\x1a\n'


def chunks(png):
    """[(type, data)] of a file; checks the signature and every CRC."""
    assert png[:8] == SIGNATURE, 'not a PNG signature'
    out, at = [], 8
    while at < len(png):
        assert at + 12 <= len(png), 'truncated chunk'
        n, = struct.unpack('>I', png[at:at + 4])
        kind, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert len(data) == n, 'truncated chunk'
        crc, = struct.unpack('>I', png[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data) & 0xFFFFFFFF, 'bad CRC in %r' % kind
        out.append((kind, data))
        at += 12 + n
    return out


def idat_stream(png):
    return b''.join(d for k, d in chunks(png) if k == b'IDAT')


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(raw, h, w):
    """h rows of 1 + 3 w filtered bytes -> (h, w, 3) uint8; filter types 0 .. 4 (bpp = 3)."""
    stride = 3 * w
    lines = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        ft, x = int(lines[y, 0]), lines[y, 1:].astype(np.int64)
        assert 0 <= ft <= 4, 'bad filter type %d' % ft
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        else:                   # 1, 3, 4 depend on the byte three to the left: pixel by pixel
            cur = np.zeros(stride, np.int64)
            for i in range(stride):
                a = int(cur[i - 3]) if i >= 3 else 0
                b = int(prev[i])
                c = int(prev[i - 3]) if i >= 3 else 0
                cur[i] = (int(x[i]) + (a if ft == 1 else (a + b) // 2 if ft == 3 else _paeth(a, b, c))) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3)


def decode(png):
    """The bytes of a PNG file -> (h, w, 3) uint8, everything checked (module docstring)."""
    cs = chunks(bytes(png))
    kinds = [k for k, _ in cs]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and kinds.count(b'IHDR') == 1 and kinds.count(b'IEND') == 1
    assert len(cs[-1][1]) == 0
    idat = [i for i, k in enumerate(kinds) if k == b'IDAT']
    assert idat and idat == list(range(idat[0], idat[-1] + 1)), 'IDAT chunks must be consecutive'
    assert all(len(cs[i][1]) <= 1 << 30 for i in idat)
    assert len(cs[0][1]) == 13
    w, h, depth, ctype, comp, filt, interlace = struct.unpack('>IIBBBBB', cs[0][1])
    assert (depth, ctype, comp, filt, interlace) == (8, 2, 0, 0, 0), 'IHDR must say 8-bit truecolour, no interlace'
    assert w > 0 and h > 0
    raw = zlib.decompress(b''.join(cs[i][1] for i in idat))            # (checks the Adler-32)
    assert len(raw) == h * (3 * w + 1), 'filtered data has %d bytes, not h (3 w + 1) = %d' % (len(raw), h * (3 * w + 1))
    return unfilter(raw, h, w)


def encode_filtered(img, filters):
    """A PNG of img whose row y uses filter type filters[y % len(filters)] (host zlib): what decode()'s unfilter is pinned by."""
    h, w, _ = img.shape
    flat = img.reshape(h, 3 * w).astype(np.int64)
    raw = bytearray()
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = flat[y]
        prev = flat[y - 1] if y else np.zeros(3 * w, np.int64)
        a = np.concatenate([np.zeros(3, np.int64), cur[:-3]])[:3 * w]
        c = np.concatenate([np.zeros(3, np.int64), prev[:-3]])[:3 * w]
        if ft == 0:
            pred = np.zeros(3 * w, np.int64)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) // 2
        else:
            pred = np.array([_paeth(int(a[i]), int(prev[i]), int(c[i])) for i in range(3 * w)], np.int64)
        raw.append(ft)
        raw += ((cur - pred) & 255).astype(np.uint8).tobytes()

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)
    return SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(bytes(raw))) + chunk(b'IEND', b'')


# ---- the rasters of the device encoder's tests ------------------------------------------------------------------------
GEOMETRY_WS = (1, 2, 3, 5, 21, 63, 64, 65, 129, SEG - 1, SEG, SEG + 1, 2 * SEG + 1)
GEOMETRY_HS = (1, 2, 19)
BAND_ROWS = (1, 3, 1000)
ALIGN_WS = (1, 5, 65)


def random_bytes(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _colour(i):
    """Colour i of a sequence in which neighbours differ in all three channels."""
    return np.array([(37 * i + 11) & 255, (91 * i + 5) & 255, (53 * i + 200) & 255], np.uint8)


def runs_row(lengths, w=None):
    """One row of runs of the given lengths in pixels, each in a colour of its own; cut or padded (random) to w."""
    px = np.concatenate([np.tile(_colour(i), (n, 1)) for i, n in enumerate(lengths)])
    if w is not None:
        if len(px) < w:
            px = np.concatenate([px, random_bytes(len(px), 1, w - len(px))[0]])
        px = px[:w]
    return px


def all_run_lengths():
    """Rows made of runs of every length 1 .. 200 pixels: row r holds the lengths r + 1, r + 11, ... in turn; 10 rows, every
    one 2,110 pixels or fewer, padded with random pixels."""
    rows = [list(range(r + 1, 201, 10)) for r in range(10)]
    w = max(sum(r) for r in rows)
    return np.stack([runs_row(r, w) for r in rows])


def match_limit_runs():
    """Runs of 85, 86, 87, 171, 172 and 173 pixels (258 bytes = 86 pixels), each after 1 .. 3 random pixels, in two rows that
    start them at different places modulo 64."""
    w = 900
    img = random_bytes(11, 2, w)
    for y, x0 in enumerate((1, 40)):
        x = x0
        for i, n in enumerate((85, 86, 87, 171, 172, 173)):
            img[y, x:x + n] = _colour(i + 7 * y)
            x += n + 1 + i % 3
        assert x <= w
    return img


def runs_modulo_64():
    """256 rows of 200 pixels with one run each: row 4 s + j starts its run at pixel s (every start 0 .. 63) and ends it before
    a pixel congruent to 4 s + j modulo 64 (every end position, four times over), one to 64 pixels long for even j and 65 to
    128 for odd j (over a step's end)."""
    rows = []
    for s in range(64):
        for j in range(4):
            end = s + 1 + (4 * s + j - s - 1) % 64 + 64 * (j & 1)
            row = random_bytes(1000 + 4 * s + j, 1, 200)[0]
            row[s:end] = _colour(s + j)
            rows.append(row)
    return np.stack(rows)


def runs_over_segment_boundary():
    """Runs that cross pixel SEG and 2 SEG of a row, from a few pixels to several steps long."""
    img = random_bytes(12, 6, 2 * SEG + 40)
    for y, (a, b) in enumerate(((SEG - 1, SEG + 1), (SEG - 3, SEG + 70), (SEG - 100, SEG + 100), (2 * SEG - 2, 2 * SEG + 2),
                               (SEG - 64, 2 * SEG + 30), (0, 2 * SEG + 40))):
        img[y, a:b] = _colour(y)
    return img


def row_wrap():
    """The last pixel of row y equals the first pixel of row y + 1 (and the first run of a row starts at its first pixel)."""
    img = random_bytes(13, 9, 70)
    for y in range(8):
        img[y + 1, 0] = img[y, -1]
        img[y + 1, 1] = img[y, -1]
    return img


def one_channel_steps(c):
    """Neighbouring pixels that differ in channel c alone: a compare that reads only the other two sees one long run."""
    img = np.zeros((3, 150, 3), np.uint8)
    img[:] = (90, 160, 230)
    img[:, :, c] = (np.arange(150)[None, :] * 7 + np.arange(3)[:, None]) & 255
    img[2, 50:100, c] = 5                                  # and a real run among them
    return img


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def run_rasters():
    """[(name, raster)] of the rasters on which the bit packing and the run logic can go wrong."""
    out = [('every run length 1..200', all_run_lengths()), ('runs around 86 and 172 pixels', match_limit_runs()),
           ('runs at every position modulo 64', runs_modulo_64()), ('runs over a segment boundary', runs_over_segment_boundary()),
           ('row wrap', row_wrap())]
    out += [('steps in channel %d alone' % c, one_channel_steps(c)) for c in range(3)]
    out += [('constant 0', np.zeros((5, 300, 3), np.uint8)), ('constant 255', np.full((5, 300, 3), 255, np.uint8)), ('checker', checker(7, 131))]
    return out
