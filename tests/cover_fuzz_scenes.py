"""Random soups for the guard census and the cover of guarded ORs: the generator and the committed table of cases of
tests/test_cover_fuzz.py (the conditions on the cases, numpy alone) and tests/test_gpu_cover_fuzz.py (the device against the numpy
model's words and the oracle's rasters).  The soups of tests/fuzz_scenes.py hold no rectangle that an OR of shapes covers; these
are made for it: triangles from a few pixels across to wider than the picture, so that some hold whole 64 x 32 rectangles alone or only
together, and ORs painted as cover_scenes._paint does.  Seeded and deterministic.  No GPU in here."""
import math
import random

import numpy as np

import params as PR
from cover_scenes import _or, _paint
from fuzz_scenes import PARAM_ID0, SOUP_RANGES, subst_xy
from marayb import add, chess, div, half, inside_triangle, min_, mul, nat, neg, sd_box, sd_circle, sd_inside, sin, step, sub, to_uv, translate, var_id, x, y

KINDS = ('one', 'two', 'shared', 'colours')
RADII = (12, 25, 40, 60, 90, 140, 250)
COLOURS = (250, 170, 90, 0, -40, -200)         # a zero colour: a leaf that is 0 on every pixel; a negative one: -0.0 where the shape is 0
N_SHAPES = 16
T_ID, U_ID, C_ID = PARAM_ID0, PARAM_ID0 + 1, PARAM_ID0 + 2


def _num(v):
    return nat(v) if v >= 0 else neg(nat(-v))


class Plant:
    """The parameters of a planted soup: (t, u) translates the whole picture, which the ROW section reads; c is multiplied into the
    pattern of a few leaves, where only PIXEL ops read it: such a leaf is tainted for the cover and not eligible for the census;
    with `sin_leaf` one leaf is ANDed with Step(Sin(10^6 x) + 2), 1 on every pixel but tainted, as the Sin's argument is unbounded."""

    def __init__(self, seed):
        self.rng = random.Random(0xC07E7 + 31 * seed)
        self.c_leaves = set(self.rng.sample(range(N_SHAPES), 3))
        self.sin_leaf = self.rng.randrange(N_SHAPES) if seed % 2 else None
        self.decl = [(T_ID,) + SOUP_RANGES['t'][seed % 2],                   # (-16, 16) or (-64, 64)
                     (U_ID,) + SOUP_RANGES['u'][seed % 3],                   # (-24, -0), (-8, 8) or the degenerate (3.5, 3.5)
                     (C_ID,) + SOUP_RANGES['c'][seed % 4]]


def shapes(seed, n, w, h, plant=None):
    """n shapes: triangles (vertices on a circle of a radius from RADII round a centre in or near the picture, so some lie outside
    it), every fourth a disc or a box; about half solid, half carrying a chess pattern in the shape's own frame."""
    rng = random.Random(0xC0BE5 + seed)
    p = [x(), y()]
    c = var_id(C_ID)
    out = []
    for i in range(n):
        cx, cy = rng.randrange(-w // 8, w + w // 8), rng.randrange(-h // 4, h + h // 4)
        r = rng.choice(RADII)
        if i % 4 == 3:
            off = [_num(cx), _num(cy)]
            r = min(r, 120)
            sd = sd_circle(nat(r)) if rng.random() < 0.5 else sd_box([nat(r), nat(max(4, r // rng.choice([1, 2, 3])))])
            inside = sd_inside(translate(sd, off))
            pattern = subst_xy(chess(rng.choice([2, 4])), mul(sub(x(), off[0]), div(nat(1), nat(max(2, r // 2)))), mul(sub(y(), off[1]), div(nat(1), nat(max(2, r // 2)))))
        else:
            while True:
                a0 = rng.uniform(0.0, math.tau)
                ang = [a0 + k * math.tau / 3 + rng.uniform(-0.6, 0.6) for k in range(3)]
                ipts = [(cx + int(round(r * math.cos(a))), cy + int(round(r * math.sin(a)))) for a in ang]
                (x1, y1), (x2, y2), (x3, y3) = ipts
                if (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3) != 0:
                    break
            pts = [(_num(a), _num(b)) for a, b in ipts]
            inside = inside_triangle(pts, p)
            uv = to_uv(pts, [(nat(0), nat(0)), (nat(1), nat(0)), (nat(0), nat(1))], p)
            pattern = subst_xy(chess(rng.choice([2, 4, 6])), uv[0], uv[1])
        s = inside if rng.random() < 0.5 else min_(inside, pattern)
        if plant is not None and i in plant.c_leaves:
            s = min_(s, step(sub(mul(c, add(sin(mul(x(), div(nat(1), nat(7)))), nat(1))), half())))
        if plant is not None and i == plant.sin_leaf:
            s = min_(s, step(add(sin(mul(x(), nat(1000000))), nat(2))))
        out.append(s)
    return out


def cover_soup(seed, n, w, h, kind, plant=None):
    """Three channels.  one: one OR of all shapes on two channels; two: two ORs over disjoint halves; shared: one OR over all shapes
    and one over every second shape (leaves on shared guard bits, which must never be cleared); colours: an f64 max reduction of
    shape_i * c_i over the first shapes beside a boolean OR of the last ones, four shapes in both."""
    ss = shapes(seed, n, w, h, plant)
    if kind == 'one':
        u = _or(ss)
        color = [_paint(u), _paint(u, 50), nat(0)]
    elif kind == 'two':
        color = [_paint(_or(ss[:n // 2])), _paint(_or(ss[n // 2:]), 70), nat(0)]
    elif kind == 'shared':
        color = [_paint(_or(ss)), _paint(_or(ss[::2]), 70), nat(0)]
    elif kind == 'colours':
        rng = random.Random(0xC0105 + seed)
        first = ss[:n // 2 + 2]
        cols = [rng.choice(COLOURS) for _ in first]
        cols[:3] = [250, 0, -40]
        red = None
        for s, col in zip(first, cols):
            t = mul(s, _num(col))
            red = t if red is None else ('Max', red, t)
        color = [red, _paint(_or(ss[n // 2 - 2:])), nat(0)]
    else:
        raise ValueError(kind)
    if plant is not None:
        color = [translate(ch, [var_id(T_ID), var_id(U_ID)]) for ch in color]
    return color


def _apart(v, kept):
    """The translation of v is at least two pixels from that of every vector kept so far."""
    return all(max(abs(v[0] - k[0]), abs(v[1] - k[1])) >= 2.0 for k in kept)


def planted_soup(seed, n, w, h, kind, n_vectors=4):
    """(channels, [(id, lo, hi), ...], vectors, c'): cover_soup with Plant(seed); the vectors are the first n_vectors of
    params.value_vectors whose translations are two pixels apart from one another (so that they are different ROW keys with
    different pictures), c' another value of the PIXEL-read factor than vectors[0]'s."""
    plant = Plant(seed)
    color = cover_soup(seed, n, w, h, kind, plant)
    vectors = []
    for v in PR.value_vectors(plant.rng, plant.decl, 40 * n_vectors):
        if _apart(v, vectors):
            vectors.append(v)
        if len(vectors) == n_vectors:
            break
    assert len(vectors) == n_vectors, (seed, len(vectors))
    lo, hi = plant.decl[2][1:]
    other = [c for c in PR.candidate_values(plant.rng, lo, hi) if c != vectors[0][2]]
    return color, plant.decl, vectors, other[0]


# ---- the cases: (kind, seed, geometry) ---------------------------------------------------------------------------------------
# geometry: (w, h, y0, y1).  A: five rectangles of 64 pixels, the last tile of 256 ragged, groups of 32, 32, 32, 32 and 8 rows.
# B: a ragged fifth rectangle of 44 pixels, a window that starts and ends off the 32-row groups of the picture, a last group of 8 rows.
A = (320, 136, 0, 136)
B = (300, 200, 37, 141)

# Every case has a cover bit and a bit its census clears; tests/test_cover_fuzz.py holds the conditions the table has to meet, and
# a seed that fails one of them is replaced here, never skipped there.
PLAIN = [('one', 2, A), ('one', 1, B), ('one', 8, A),
         ('two', 2, A), ('two', 7, B), ('two', 9, B),
         ('shared', 0, A), ('shared', 3, B), ('shared', 4, A),
         ('colours', 2, A), ('colours', 5, B), ('colours', 8, A)]
PLANTED = [('one', 1, B), ('one', 2, A),
           ('two', 3, B), ('two', 4, A),
           ('shared', 0, A), ('shared', 5, B),
           ('colours', 2, A), ('colours', 3, B)]
MANY_KEYS = (('one', 1, B), 10)             # a case of PLANTED with ten vectors: more keys than a context keeps sets (RowReuse::MAX_KEPT = 8)
ENTRY_POINTS = ('one', 2, A)                # in PLAIN (a partial cover) and in PLANTED: the other entry points over the same tables


def plain(case):
    """The channels of a case of PLAIN."""
    kind, seed, (w, h, y0, y1) = case
    return cover_soup(seed, N_SHAPES, w, h, kind)


def planted(case, n_vectors=4):
    """(channels, declarations, vectors, c') of a case of PLANTED."""
    kind, seed, (w, h, y0, y1) = case
    return planted_soup(seed, N_SHAPES, w, h, kind, n_vectors)


def lowered(case, n_vectors=None):
    """(tape, channels, declarations, vectors, c'): a case lowered; n_vectors = None: a case of PLAIN, no parameters."""
    import maray_amd as M
    from marayb import encode
    w, h = case[2][:2]
    if n_vectors is None:
        color = plain(case)
        return M.Scene(encode((w, h), color)).lower(), color, [], [None], None
    color, decl, vectors, other = planted(case, n_vectors)
    return PR.declared_ids(encode((w, h), color), decl).lower(), color, decl, vectors, other


def tables(tape, geo, values=None):
    """The numpy model's three tables of guard words of one key, and which rectangles each OR covers: a dict of `refined` (what the
    ROW pass and the second bounds write), `census` (what the census leaves of them), `cover` (the third table) and `covered`."""
    import census_scenes as CS
    import cover_scenes as CV
    w, _, y0, y1 = geo
    vb, cb, cov = CV.words(tape, w, y0, y1 - y0, params=values)
    return dict(refined=CS.words(tape, w, y0, y1 - y0, params=values, census=False), census=cb, cover=vb, covered=cov)


def bit_mask(bits, n_words):
    """(n_words,) uint64 with the given bits set."""
    out = [0] * n_words
    for b in bits:
        out[b // 64] |= 1 << (b % 64)
    return np.array(out, np.uint64)
