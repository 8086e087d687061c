"""An APNG decoder that trusts nothing in the file, built on tests/png_stream.py (no device needed): the helper of
tests/test_apng_abi.py and tests/test_gpu_apng.py.

decode() checks the signature and every chunk's CRC-32 (png_stream.chunks), IHDR, that acTL comes before the first IDAT and
counts exactly the fcTLs, that the sequence numbers of fcTL and fdAT are 0, 1, 2, ... without a gap, that the first fcTL is the
full canvas at (0, 0), that every rectangle is non-empty and inside the canvas, and that every frame's zlib stream is taken
completely by zlib.decompressobj with nothing left over (its Adler-32 checked, and again here), is exactly (3 bw + 1) bh bytes
long and unfilters with types 0 .. 4.  It composes the frames as a viewer does for dispose NONE / blend SOURCE: a copy of the
canvas, then canvas[y0:y1, x0:x1] = region.

build() writes such files in Python with zlib.compress: what pins the decoder, and the mutants it must reject.
"""
import struct
import zlib

import numpy as np

import png_stream as P


class Decoded:
    """frames: the composed (h, w, 3) uint8 canvases; rects: (x, y, w, h) per frame; streams: the frames' zlib streams."""

    def __init__(self, frames, rects, streams, delay, plays):
        self.frames, self.rects, self.streams, self.delay, self.plays = frames, rects, streams, delay, plays


def _inflate(z, bw, bh):
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof, 'a frame\'s stream does not end'
    assert d.unused_data == b'' and d.unconsumed_tail == b'', 'bytes left over behind a frame\'s stream'
    assert struct.unpack('>I', z[-4:])[0] == zlib.adler32(raw) & 0xFFFFFFFF, 'bad Adler-32'
    assert len(raw) == (3 * bw + 1) * bh, 'a frame\'s filtered data has %d bytes, not (3 bw + 1) bh = %d' % (len(raw), (3 * bw + 1) * bh)
    return P.unfilter(raw, bh, bw)


def decode(png):
    cs = P.chunks(bytes(png))
    kinds = [k for k, _ in cs]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and kinds.count(b'IHDR') == 1 and kinds.count(b'IEND') == 1
    assert len(cs[-1][1]) == 0 and len(cs[0][1]) == 13
    w, h, depth, ctype, comp, filt, interlace = struct.unpack('>IIBBBBB', cs[0][1])
    assert (depth, ctype, comp, filt, interlace) == (8, 2, 0, 0, 0), 'IHDR must say 8-bit truecolour, no interlace'
    assert w > 0 and h > 0
    assert kinds.count(b'acTL') == 1, 'one acTL'
    idat = [i for i, k in enumerate(kinds) if k == b'IDAT']
    assert idat and idat == list(range(idat[0], idat[-1] + 1)), 'IDAT chunks must be consecutive'
    assert kinds.index(b'acTL') < idat[0], 'acTL must come before the first IDAT'
    assert len(cs[kinds.index(b'acTL')][1]) == 8
    n_frames, plays = struct.unpack('>II', cs[kinds.index(b'acTL')][1])
    assert n_frames == kinds.count(b'fcTL') and n_frames > 0, 'acTL counts %d frames, the file has %d fcTL' % (n_frames, kinds.count(b'fcTL'))
    seq = 0
    frames = []             # [rect, delay, [stream parts]]
    for i, (kind, data) in enumerate(cs):
        assert len(data) <= 1 << 30
        if kind == b'fcTL':
            assert len(data) == 26
            s, bw, bh, x, y, dn, dd, dispose, blend = struct.unpack('>IIIIIHHBB', data)
            assert s == seq, 'sequence number %d where %d is due' % (s, seq)
            seq += 1
            assert (dispose, blend) == (0, 0), 'dispose NONE and blend SOURCE'
            assert bw > 0 and bh > 0, 'an empty frame'
            assert x + bw <= w and y + bh <= h, 'a frame past the canvas\' edge'
            if not frames:
                assert i < idat[0], 'the first fcTL must come before IDAT'
                assert (x, y, bw, bh) == (0, 0, w, h), 'the first frame must be the whole canvas'
            else:
                assert i > idat[-1] and frames[-1][2], 'a frame without data'
            frames.append([(x, y, bw, bh), (dn, dd), []])
        elif kind == b'IDAT':
            assert len(frames) == 1, 'IDAT belongs to the first frame'
            frames[0][2].append(data)
        elif kind == b'fdAT':
            assert len(frames) > 1 and len(data) >= 4, 'fdAT belongs to a later frame'
            s, = struct.unpack('>I', data[:4])
            assert s == seq, 'sequence number %d where %d is due' % (s, seq)
            seq += 1
            frames[-1][2].append(data[4:])
        else:
            assert kind in (b'IHDR', b'acTL', b'IEND'), 'unexpected chunk %r' % kind
    assert frames[-1][2], 'a frame without data'
    assert len({f[1] for f in frames}) == 1, 'one delay for all frames'
    canvas = np.zeros((h, w, 3), np.uint8)
    out, streams = [], []
    for (x, y, bw, bh), _, parts in frames:
        z = b''.join(parts)
        canvas = canvas.copy()
        canvas[y:y + bh, x:x + bw] = _inflate(z, bw, bh)
        out.append(canvas)
        streams.append(z)
    return Decoded(out, [f[0] for f in frames], streams, frames[0][1], plays)


# ---- files made in Python ------------------------------------------------------------------------------------------------
def _chunk(kind, data, bad_crc=False):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', (zlib.crc32(kind + data) ^ (1 if bad_crc else 0)) & 0xFFFFFFFF)


def _filtered(img, filters):
    """The filtered bytes of img, row y with type filters[y % len(filters)]: cut out of png_stream.encode_filtered's stream."""
    return zlib.decompress(P.idat_stream(P.encode_filtered(img, filters)))


def bounding_box(a, b):
    """(x0, y0, x1, y1) of the pixels in which two (h, w, 3) rasters differ, (0, 0, 0, 0) when equal: the contract of
    maray_frame_delta."""
    ys, xs = np.nonzero((a != b).any(2))
    if ys.size == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)


def rect_of(box):
    """The (x, y, w, h) a frame with this box is written with: 1 x 1 at (0, 0) for the empty box."""
    return (0, 0, 1, 1) if box == (0, 0, 0, 0) else (box[0], box[1], box[2] - box[0], box[3] - box[1])


def build(frames, filters=(0,), delay=(1, 25), plays=0, fdat_limit=1 << 30, seq_gap_at=None, bad_crc=None, grow_rect=None, actl_count=None,
          trailing=None):
    """An APNG of the frames (equal shapes), every later frame its bounding-box rectangle, streams by zlib.compress.
    fdat_limit: stream bytes per fdAT chunk.  The mutants: seq_gap_at = k skips a number at the k-th sequence number handed
    out; bad_crc = the name of a chunk type whose first chunk gets a wrong CRC; grow_rect = frame index whose fcTL claims one
    more column than the canvas has room for; actl_count = what acTL says; trailing = frame index whose stream gets a byte
    appended."""
    h, w, _ = frames[0].shape
    seq = [0]

    def next_seq():
        if seq_gap_at is not None and seq[0] == seq_gap_at:
            seq[0] += 1
        seq[0] += 1
        return seq[0] - 1
    spoiled = set()

    def chunk(kind, data):
        bad = kind == bad_crc and kind not in spoiled
        if bad:
            spoiled.add(kind)
        return _chunk(kind, data, bad)
    out = P.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
    out += chunk(b'acTL', struct.pack('>II', len(frames) if actl_count is None else actl_count, plays))
    for i, f in enumerate(frames):
        x, y, bw, bh = (0, 0, w, h) if i == 0 else rect_of(bounding_box(frames[i - 1], f))
        z = zlib.compress(_filtered(np.ascontiguousarray(f[y:y + bh, x:x + bw]), list(filters)))
        if trailing == i:
            z += b'\x00'
        claim_x = w - bw + 1 if grow_rect == i else x
        out += chunk(b'fcTL', struct.pack('>IIIIIHHBB', next_seq(), bw, bh, claim_x, y, delay[0], delay[1], 0, 0))
        if i == 0:
            out += chunk(b'IDAT', z)
        else:
            for at in range(0, len(z), fdat_limit):
                out += chunk(b'fdAT', struct.pack('>I', next_seq()) + z[at:at + fdat_limit])
    return out + chunk(b'IEND', b'')
