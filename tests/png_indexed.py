"""The indexed-colour files of the device PNG encoder (include/maray_hip.h, "Indexed colour"), restated in numpy and zlib: the
model that gives the exact bytes of a file, a decoder that trusts nothing in one, and the rasters of the tests.  No device
needed: the helper of tests/test_png_indexed_abi.py and tests/test_gpu_png_indexed.py.

model_file(img) is the contract written out: the sorted palette, the bit depth, the packed rows, segments of 768 packed bytes,
steps of 64, one match of distance 1 per run of three or more repeated bytes inside a step, fixed-Huffman codes.
decode_indexed(png) checks the signature, every CRC, IHDR (colour type 3 and the depth the palette's size asks for), the chunk
order, PLTE's length, the zlib stream with its Adler-32, the stream's length, the filter bytes, the pad bits and every index.
"""
import struct
import zlib

import numpy as np

import png_stream as P

SEG = 768               # packed bytes per segment
STEP = 64               # bytes per step: a run ends with its step
COLORS_MAX = 256


# ---- palette, depth, packed rows -------------------------------------------------------------------------------------------
def _keys(img):
    a = img.astype(np.uint32)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def palette(img):
    """The distinct colours of an (h, w, 3) raster, (n, 3) uint8, ascending by R * 65536 + G * 256 + B."""
    k = np.unique(_keys(img))
    return np.stack([k >> 16, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8)


def depth(n):
    assert 1 <= n <= COLORS_MAX
    return 1 if n <= 2 else 2 if n <= 4 else 4 if n <= 16 else 8


def row_bytes(w, d):
    return (w * d + 7) // 8


def pack_rows(img):
    """(h, rb) uint8: every pixel's index into palette(img) in depth(n) bits, the leftmost pixel in the high-order bits, pad zero."""
    h, w, _ = img.shape
    keys = _keys(img)
    pal = np.unique(keys)
    d = depth(len(pal))
    idx = np.searchsorted(pal, keys).astype(np.uint8)
    per = 8 // d
    rb = row_bytes(w, d)
    padded = np.zeros((h, rb * per), np.uint8)
    padded[:, :w] = idx
    out = np.zeros((h, rb), np.uint8)
    for k in range(per):
        out |= padded[:, k::per] << (8 - d * (k + 1))
    return out


# ---- the fixed codes ------------------------------------------------------------------------------------------------------
def _rev(code, bits):
    return int('{:0{}b}'.format(code, bits)[::-1], 2)


def _literal(v):
    """(bits as they enter the LSB-first stream, their number)"""
    return (_rev(0x30 + v, 8), 8) if v < 144 else (_rev(0x190 + v - 144, 9), 9)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def _match1(length):
    """A match of `length` bytes at distance 1: the length symbol's code, its extra bits, distance code 0 (five zero bits)."""
    assert 3 <= length <= 258
    i = max(j for j in range(29) if _LEN_BASE[j] <= length)
    sym = 257 + i
    code, bits = (_rev(sym - 256, 7), 7) if sym < 280 else (_rev(0xC0 + sym - 280, 8), 8)
    code |= (length - _LEN_BASE[i]) << bits
    return code, bits + _LEN_EXTRA[i] + 5


_LIT = [_literal(v) for v in range(256)]
_MATCH = {n: _match1(n) for n in range(3, STEP + 1)}


def tokens(seg):
    """The tokens of a segment's packed bytes: [('lit', value) | ('match', length)]."""
    seg = np.asarray(seg, np.uint8)
    n = len(seg)
    rep = np.zeros(n, bool)
    rep[1:] = seg[1:] == seg[:-1]
    out = []
    for p0 in range(0, n, STEP):
        i, end = p0, min(n, p0 + STEP)
        while i < end:
            if not rep[i]:
                out.append(('lit', int(seg[i])))
                i += 1
                continue
            j = i
            while j < end and rep[j]:
                j += 1
            if j - i >= 3:
                out.append(('match', j - i))
            else:
                out += [('lit', int(seg[i]))] * (j - i)
            i = j
    return out


def segment_bytes(seg, first):
    """A segment as it stands in the stream: one fixed-Huffman block (in a row's first segment the filter byte 0 in front), the
    end-of-block, the empty stored block that ends on a byte boundary."""
    acc, nbits = 2, 3                                   # BFINAL = 0, BTYPE = 01
    toks = ([('lit', 0)] if first else []) + tokens(seg)
    for kind, v in toks:
        code, bits = _LIT[v] if kind == 'lit' else _MATCH[v]
        acc |= code << nbits
        nbits += bits
    at = (nbits + 7 + 3 + 7) // 8                       # seven zero bits, three zero bits, zeros to the byte
    return acc.to_bytes(at, 'little') + b'\x00\x00\xff\xff'


def model_stream(img):
    packed = pack_rows(img)
    z = [b'\x78\x01']
    for row in packed:
        for s in range(0, len(row), SEG):
            z.append(segment_bytes(row[s:s + SEG], s == 0))
    raw = b''.join(b'\x00' + row.tobytes() for row in packed)
    z.append(b'\x01\x00\x00\xff\xff' + struct.pack('>I', zlib.adler32(raw) & 0xFFFFFFFF))
    return b''.join(z)


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def model_file(img):
    """The exact bytes of the indexed file of an (h, w, 3) raster of at most 256 colours."""
    h, w, _ = img.shape
    pal = palette(img)
    z = model_stream(img)
    idat = b''.join(_chunk(b'IDAT', z[o:o + (1 << 30)]) for o in range(0, len(z), 1 << 30))
    return (P.SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth(len(pal)), 3, 0, 0, 0)) + _chunk(b'PLTE', pal.tobytes()) + idat +
            _chunk(b'IEND', b''))


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def decode_indexed(png):
    """The bytes of an indexed file -> ((h, w, 3) uint8, the palette (n, 3)), everything checked (module docstring)."""
    cs = P.chunks(bytes(png))                           # (the signature and every CRC)
    kinds = [k for k, _ in cs]
    assert kinds[:2] == [b'IHDR', b'PLTE'] and kinds[-1] == b'IEND' and len(kinds) >= 4, 'chunk order: %r' % kinds
    assert all(k == b'IDAT' for k in kinds[2:-1]), 'chunk order: %r' % kinds
    assert len(cs[-1][1]) == 0 and len(cs[0][1]) == 13
    assert all(len(d) <= 1 << 30 for _, d in cs[2:-1])
    w, h, d, ctype, comp, filt, interlace = struct.unpack('>IIBBBBB', cs[0][1])
    assert (ctype, comp, filt, interlace) == (3, 0, 0, 0), 'IHDR must say colour type 3, no interlace'
    assert w > 0 and h > 0
    plte = cs[1][1]
    assert len(plte) % 3 == 0 and 1 <= len(plte) // 3 <= COLORS_MAX, 'PLTE holds %d bytes' % len(plte)
    n = len(plte) // 3
    assert d == depth(n), 'depth %d for %d colours' % (d, n)
    pal = np.frombuffer(plte, np.uint8).reshape(n, 3)
    keys = _keys(pal)
    assert (keys[1:] > keys[:-1]).all(), 'the palette is not strictly ascending'
    raw = zlib.decompress(b''.join(dd for _, dd in cs[2:-1]))          # (checks the Adler-32)
    rb = row_bytes(w, d)
    assert len(raw) == h * (rb + 1), 'filtered data has %d bytes, not h (rb + 1) = %d' % (len(raw), h * (rb + 1))
    lines = np.frombuffer(raw, np.uint8).reshape(h, rb + 1)
    assert (lines[:, 0] == 0).all(), 'a filter byte is not 0'
    per = 8 // d
    idx = np.zeros((h, rb * per), np.uint8)
    for k in range(per):
        idx[:, k::per] = (lines[:, 1:] >> (8 - d * (k + 1))) & ((1 << d) - 1)
    assert (idx[:, w:] == 0).all(), 'pad bits are not 0'
    idx = idx[:, :w]
    assert int(idx.max()) < n, 'index %d with %d colours' % (int(idx.max()), n)
    return pal[idx], pal


# ---- the rasters of the tests ------------------------------------------------------------------------------------------------
def of_colours(colours, h, w, seed=0):
    """An (h, w, 3) raster whose pixels are drawn from `colours` ((n, 3) or n keys R << 16 | G << 8 | B), every one at least once
    where h w >= n."""
    c = np.asarray(colours)
    if c.ndim == 1:
        c = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=1)
    c = c.astype(np.uint8)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(c), h * w)
    if h * w >= len(c):
        pick[rng.permutation(h * w)[:len(c)]] = np.arange(len(c))
    return c[pick].reshape(h, w, 3)


def n_colours(n, seed=0):
    """n distinct keys, a seeded choice among 2^24."""
    return np.random.default_rng(1000 + seed).choice(1 << 24, n, replace=False)


def colour_sets():
    """[(name, keys)] of the sets that stress a hashed set: black with white, white alone, colours that differ in one channel
    only, greys, and multiples of 0x000400 and of 0x010000, whose low bits are all equal."""
    a = np.arange(256)
    return [('black and white', np.array([0, 0xFFFFFF])), ('white alone', np.array([0xFFFFFF])), ('black alone', np.array([0])),
            ('R only', a << 16), ('G only', a << 8), ('B only', a), ('greys', a * 0x010101), ('multiples of 0x000400', a * 0x000400),
            ('multiples of 0x010000', a * 0x010000), ('random 256 of 2^24', n_colours(256, 7))]


def grey(values):
    """A raster of greys from an (h, w) array of bytes: at depth 8 -- all 256 greys in it -- a pixel's index is its value."""
    v = np.asarray(values, np.uint8)
    return np.repeat(v[:, :, None], 3, axis=2)


def all_greys_row(w):
    return (np.arange(w) * 37 & 255).astype(np.uint8)


def byte_runs():
    """[(name, raster)] at depth 8, where pixel runs are byte runs: the first rows hold all 256 greys, so that index = value."""
    out = []
    head = np.arange(256, dtype=np.uint8)

    def with_head(rows, w):
        top = np.resize(head, (-(-256 // w), w))
        return grey(np.concatenate([top, rows]))
    # every run length 1 .. 130, each after a byte that differs, at varying starts
    w = 900
    rows = []
    for r in range(10):
        line, v = [], 0
        for n in range(r + 1, 131, 10):
            v = (v + 1 + n) & 255
            line += [v] * (n + 1)                   # n repeated bytes behind their first
            v = (v + 1) & 255
            line += [v]
        line = (line + list(all_greys_row(w)))[:w]
        rows.append(line)
    out.append(('every run length 1..130', with_head(np.array(rows, np.uint8), w)))
    # every start and end modulo 64
    rows = []
    for s in range(64):
        for j in range(4):
            end = s + 1 + (4 * s + j - s - 1) % 64 + 64 * (j & 1)
            line = all_greys_row(200).copy()
            line[s:end] = (s + j) & 255
            rows.append(line)
    out.append(('runs at every position modulo 64', with_head(np.array(rows, np.uint8), 200)))
    # over a segment boundary, and over a row end
    w = 2 * SEG + 40
    rows = []
    for a, b in ((SEG - 1, SEG + 1), (SEG - 3, SEG + 70), (SEG - 100, SEG + 100), (2 * SEG - 2, 2 * SEG + 2), (SEG - 64, 2 * SEG + 30), (0, w)):
        line = all_greys_row(w).copy()
        line[a:b] = 9
        rows.append(line)
    out.append(('runs over a segment boundary', with_head(np.array(rows, np.uint8), w)))
    rows = np.stack([all_greys_row(70) for _ in range(9)])
    for y in range(8):
        rows[y, -3:] = 200 + y
        rows[y + 1, :3] = 200 + y
    out.append(('runs over a row end', with_head(rows, 70)))
    # lengths 1 and 2 next to lengths 3: a b b c c c d d d d e e e f f g ...
    line = []
    for i, n in enumerate([1, 2, 3, 4, 3, 2, 1, 3, 3, 2, 2, 1, 1, 4, 1, 3] * 8):
        line += [(3 * i + 1) & 255] * n
    out.append(('lengths 1 and 2 next to 3', with_head(np.array([line, line[1:] + [0], line[2:] + [0, 1]], np.uint8), len(line))))
    return out


def small_rasters():
    """[(name, raster)] of at most 256 colours that need no head: constants, the checker, png_stream's run rasters that qualify."""
    out = [('constant 0', np.zeros((5, 300, 3), np.uint8)), ('constant 255', np.full((5, 300, 3), 255, np.uint8)),
           ('constant colour', np.full((3, 2000, 3), (1, 200, 77), np.uint8)), ('checker', P.checker(7, 131)),
           ('wide checker', P.checker(3, 8 * 1537 - 3))]
    out += [(name, img) for name, img in P.run_rasters() if len(np.unique(_keys(img))) <= COLORS_MAX]
    return out
