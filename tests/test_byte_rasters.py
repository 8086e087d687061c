"""The helpers of the byte-raster tests (tests/byte_rasters.py) without a device.

Two things are checked here, so that the GPU tests need not measure them:
  - the texture-identity scene renders its texture byte for byte and the atlas scene renders slice t, on the CPU oracle and
    under the host tape evaluator for the lowered programs: the GPU tests' sample rasters and frames are the bytes they chose;
  - those bytes are sharp: every mutant of the two numpy contracts differs from its contract on them, a footprint moved by
    one sample shows on nearly every pixel, the rounding step sees its two critical sums, the mean sees every residue.
"""
import numpy as np
import pytest

import byte_rasters as BR
import maray_amd as M
import params as PR
import tape_eval as TE
from marayb import encode
from oracle_ffi import Scene as OScene
from test_filter import tent
from test_gpu_shutter import mean
from test_gpu_supersample import box

KS = [2, 4, 8]


# ---- the scenes render the bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_identity_scene_renders_its_texture_on_the_oracle(k):
    s = BR.parity_raster(k)
    H, W, _ = s.shape
    got8, got64 = OScene(encode((W, H), BR.identity_color())).render_rows(W, H, 0, H, textures=[s], threads=4)
    assert np.array_equal(got8, s)
    assert np.array_equal(got64, s.astype(np.float64))
    assert OScene(BR.identity_scene().encode()).render_rows(W, H, 5, 6, textures=[s], threads=1, want_f64=False)[0].tobytes() == s[5:6].tobytes()


@pytest.mark.parametrize('k', KS)
def test_identity_program_renders_its_texture_under_the_tape_evaluator(k):
    """One program for every k and size; with its skips ignored and with its skips taken per wavefront."""
    tape = BR.identity_scene().lower()
    assert tape.param_count == 0
    for w in (5, 65):
        s = BR.geometry_raster(k, w)
        H, W, _ = s.shape
        assert np.array_equal(TE.cast_u8(TE.render_rows(tape, W, 0, H, [s])), s)
        assert np.array_equal(TE.cast_u8(TE.render_rows_waves(tape, W, 3, H - 1, [s], tile=64)), s[3:H - 1])


def test_atlas_scene_renders_slice_t():
    """On the oracle through the substituted scene (tests/params.py), and the lowered one-parameter program under the tape
    evaluator; frames in the gaps of the atlas (a lookup one slice off) would show."""
    w, h = BR.SHUTTER_W, BR.SHUTTER_H
    tape = BR.atlas_scene().lower()
    assert tape.param_count == 1 and tape.param_range(0) == (0.0, float(BR.T_MAX))
    for n in (2, 64):
        frames, _ = BR.shutter_case(n)
        a = BR.atlas(frames)
        assert a.shape == (h, n * BR.PITCH, 3)
        for t in sorted({0, 1, 31 % n, n - 1}):
            data = encode((w, h), PR.substituted(BR.atlas_color(), ['t'], (float(t),)))
            assert np.array_equal(OScene(data).render_rows(w, h, 0, h, textures=[a], threads=4, want_f64=False)[0], frames[t]), (n, t)
            v2 = PR.as_v2(tape, (float(t),))
            assert np.array_equal(TE.cast_u8(TE.render_rows(v2, w, 0, h, [a])), frames[t]), (n, t)
            assert np.array_equal(TE.cast_u8(TE.render_rows_waves(v2, w, 0, h, [a], tile=64)), frames[t]), (n, t)


@pytest.mark.parametrize('k', [2, 4])
def test_atlas_at_sample_scale(k):
    """The composition tests' atlas (k = 2 and 4): slices of k w x k h samples, the program evaluated at sample indices."""
    w, h = 21, 13
    frames = BR.random_frames(40 + k, 4, k * h, k * w)
    a = BR.atlas(frames)
    tape = BR.atlas_scene().lower()
    for t in range(4):
        assert np.array_equal(TE.cast_u8(TE.render_rows(PR.as_v2(tape, (float(t),)), k * w, 0, k * h, [a])), frames[t])


# ---- the general forms are the contracts -------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_general_tent_is_the_contract(k):
    for s in (BR.parity_raster(k), BR.geometry_raster(k, 1), BR.geometry_raster(k, 2), BR.geometry_raster(k, 5)):
        want = tent(s, k)
        assert np.array_equal(BR.tent_general(s, k), want)
        W = 4 * k ** 4
        assert np.array_equal(((BR.tent_sums(s, k) + W // 2) // W).astype(np.uint8), want)


@pytest.mark.parametrize('n', BR.SHUTTER_NS)
def test_general_mean_is_the_contract(n):
    frames, order = BR.shutter_case(n)
    assert sorted(order) == list(range(n)) and order != list(range(n))
    assert np.array_equal(BR.mean_general(frames), mean(frames))
    assert np.array_equal(BR.mean_general([frames[i] for i in order]), mean(frames))


# ---- the tent tests' rasters are sharp ---------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_parity_raster_kills_every_tent_mutant(k):
    """Alone, every mutant; a footprint moved by one sample, sideways or by a row, on at least 0.9 of the output pixels."""
    s = BR.parity_raster(k)
    want = tent(s, k)
    assert not np.array_equal(want, box(s, k))
    mutants = BR.tent_mutants(k, BR.PARITY_W)
    assert len(mutants) == 4 * (k - 1) + 8 + 4 + 6 * k + 2 + 4
    for name, kind, f in mutants:
        got = f(s)
        differ = (got != want).any(axis=2)
        assert differ.any(), name
        if kind:
            assert differ.mean() >= 0.9, (name, differ.mean())


@pytest.mark.parametrize('k', KS)
def test_parity_raster_reaches_both_sides_of_the_rounding(k):
    """Some output byte's weighted sum is exactly W/2 modulo W (rounds up: one less would not) and some is W/2 - 1."""
    W = 4 * k ** 4
    r = BR.tent_sums(BR.parity_raster(k), k) % W
    assert (r == W // 2).any() and (r == W // 2 - 1).any()
    # the seed is the first that does it
    for seed in range(BR.PARITY_SEED[k]):
        r = BR.tent_sums(BR.random_bytes(seed, BR.PARITY_H * k, BR.PARITY_W * k), k) % W
        assert not ((r == W // 2).any() and (r == W // 2 - 1).any()), seed


def _survivors(k, w, rasters):
    """Names of the mutants of width w that equal the contract on every one of the rasters."""
    wants = [tent(s, k) for s in rasters]
    return [name for name, kind, f in BR.tent_mutants(k, w) if all(np.array_equal(f(s), want) for s, want in zip(rasters, wants))]


def _rounding_is_not_reached(k, s):
    """True where no output byte of the raster sits at the rounding constant's critical sums (a small raster at k = 8: one
    byte in 16384 does)."""
    W = 4 * k ** 4
    r = BR.tent_sums(s, k) % W
    return [name for name, hit in (('rounding constant +1', (r == W // 2 - 1).any()), ('rounding constant -1', (r == W // 2).any())) if not hit]


def _cannot_show(k, w):
    """The mutants that ARE the contract at output width w, whatever the bytes: a footprint moved for pixels px = r modulo 4
    where there is no such pixel, and two weights swapped whose positions every pixel clamps to the same sample (w = 1: the
    k/2 + 1 positions at either end of the only footprint)."""
    out = {'footprint of pixels %d modulo 4 moved %+d' % (r, d) for r in range(4) if r >= w for d in (1, -1)}
    a = k * np.arange(w)[:, None] + np.arange(2 * k)[None, :] - k // 2
    a = np.clip(a, 0, k * w - 1)
    out |= {'horizontal weights %d and %d swapped' % (i, i + 1) for i in range(2 * k - 1) if (a[:, i] == a[:, i + 1]).all()}
    return out


def _check_small_raster(k, w, s):
    left = set(_survivors(k, w, [s])) - set(_rounding_is_not_reached(k, s))
    assert left <= _cannot_show(k, w), (k, w, sorted(left - _cannot_show(k, w)))
    if w >= 4:
        assert not left and not _cannot_show(k, w), (k, w, sorted(left))


@pytest.mark.parametrize('k', KS)
def test_geometry_rasters_kill_every_tent_mutant(k):
    """Every raster of the geometry tests kills every mutant that its width can show, but a rounding constant whose critical
    sum it does not hold (at k = 8 one sum in 16384 is critical: the parity raster above is the one that holds both); from 4
    pixels up a width can show them all."""
    assert _cannot_show(k, 1) and not _cannot_show(k, 5)
    for w in BR.GEOMETRY_WS:
        _check_small_raster(k, w, BR.geometry_raster(k, w))


@pytest.mark.parametrize('k', BR.DESTINATION_KS)
def test_destination_rasters_kill_every_tent_mutant(k):
    for w in BR.DESTINATION_WS:
        _check_small_raster(k, w, BR.destination_raster(k, w))


def test_streams_raster_kills_every_tent_mutant():
    assert _survivors(BR.STREAMS_K, BR.STREAMS_W, [BR.streams_raster()]) == []


@pytest.mark.parametrize('k', KS)
def test_extreme_rasters(k):
    """What each extreme is for: the constant rasters reach the largest sums and come out unchanged; the impulses show every
    footprint position (columns: in every channel) and with the checker kill every weight, channel and footprint mutant."""
    w, h = BR.EXTREMES_W, BR.EXTREMES_H
    rasters = dict(BR.extreme_rasters(h, w, k))
    assert set(rasters) == {'zeros', 'ones', 'checker', 'columns', 'rows'}
    assert all(s.shape == (k * h, k * w, 3) and s.dtype == np.uint8 for s in rasters.values())
    assert (tent(rasters['zeros'], k) == 0).all() and (tent(rasters['ones'], k) == 255).all()
    assert BR.tent_sums(rasters['ones'], k).max() == 255 * 4 * k ** 4
    assert set(np.unique(rasters['checker'])) == {0, 255} and (rasters['checker'][:-1] != rasters['checker'][1:]).all()
    assert BR.footprint_positions_hit(k, k * w) == set(range(2 * k)) == BR.footprint_positions_hit(k, k * h)
    cols = rasters['columns']
    for c in range(3):              # every offset of a sample in its pixel, in every channel
        at = np.flatnonzero(cols[0, :, c])
        assert {int(a) % k for a in at} == set(range(k)), c
    assert (cols.sum(axis=2) <= 255).all()
    # one impulse per footprint: the horizontal sums of the column raster are single weights times 255
    sums = BR.tent_sums(cols, k)
    assert set(np.unique(sums // (255 * 2 * k * k))) == {0} | set(BR.tent_weights(k))
    left = _survivors(k, w, list(rasters.values()))
    assert all(name.startswith(('rounding', 'zero past')) for name in left), left


# ---- the shutter tests' frames are sharp -------------------------------------------------------------------------------
@pytest.mark.parametrize('n', BR.SHUTTER_NS)
def test_shutter_frames_kill_every_mean_mutant(n):
    """On the random frames in the order the GPU test passes them; and their sums take every residue modulo n, so every case of
    the rounding step occurs."""
    frames, order = BR.shutter_case(n)
    passed = [frames[i] for i in order]
    want = mean(frames)
    mutants = BR.mean_mutants(n)
    assert len(mutants) == 2 + (n - 1) + (2 if n > 8 else 0)
    for name, f in mutants:
        assert not np.array_equal(f(passed), want), name
    sums = sum(f.astype(np.int64) for f in frames)
    assert set(np.unique(sums % n)) == set(range(n))
    for rows in ((5, 6), (17, 30)):                     # the row ranges the GPU test renders
        part = [f[rows[0]:rows[1]] for f in passed]
        for name, f in mutants:
            assert not np.array_equal(f(part), want[rows[0]:rows[1]]), (name, rows)


@pytest.mark.parametrize('n', BR.HEAD_TAIL_NS)
def test_head_and_tail_frames_kill_every_mean_mutant(n):
    """The largest raster of the head-and-tail test (5 x 7 pixels, 105 bytes) kills every mutant alone; every size kills the
    two about groups; three bytes cannot show 63 frame mix-ups or hold a critical sum of the rounding, 15 bytes show the
    mix-ups."""
    frames, order = BR.head_tail_case(n)
    for w in BR.HEAD_TAIL_WS:
        for rows in BR.HEAD_TAIL_ROWS:
            part = [frames[i][:rows, :w] for i in order]
            want = mean(part)
            for name, f in BR.mean_mutants(n):
                if (w, rows) == (5, 7) or name.startswith(('the first', '8 bits')) or (name.startswith('frame') and w * rows * 3 >= 15):
                    assert not np.array_equal(f(part), want), (name, w, rows)


def test_shutter_extremes():
    """Alternating 0 / 255: every byte's sum is 255 n / 2, the mean 128 from exactly half way.  All 255 at n = 64: the largest
    sum, 16320.  Frames that differ in one byte each: the mean differs from the base in those n bytes and no other."""
    for n in (2, 8, 16, 64):
        frames = [BR.constant(255 * (i & 1), 5, 7) for i in range(n)]
        assert (mean(frames) == 128).all()
        assert (BR.mean_general(frames, half=n // 2 - 1) == 127).all()
    assert (mean([BR.constant(255, 5, 7)] * 64) == 255).all()
    assert (BR.mean_general([BR.constant(255, 5, 7)] * 64, carry_bits=8) != 255).all()
    for n in (8, 64):
        frames = BR.one_byte_frames(n, BR.SHUTTER_H, BR.SHUTTER_W)
        base = frames[0].copy()
        base.reshape(-1)[0] ^= 0xFF
        at = [int(np.flatnonzero((f != base).reshape(-1))[0]) for f in frames]
        assert all(int((f != base).sum()) == 1 for f in frames)
        assert at[0] == 0 and at[-1] == base.size - 1 and len(set(at)) == n
        moved = np.flatnonzero((mean(frames) != base).reshape(-1))
        assert set(moved) <= set(at)
        for name, f in BR.mean_mutants(n):
            if name.startswith(('the first', '8 bits')):
                assert not np.array_equal(f(frames), mean(frames)), (n, name)
