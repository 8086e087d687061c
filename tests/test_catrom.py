"""The Catmull-Rom reconstruction filter without a device (include/maray_hip.h, "reconstruction filter"): the weights and the
bounds the header states; the numpy restatement (tests/catrom_model.py) against the contract's formula written as a quadruple
loop; the crafted rasters' conditions; that the rasters the GPU tests use tell every mutant from the contract; the options
structs' layout; the CLI's usage errors; the façade's argument check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import byte_rasters as BR
import catrom_model as CM
import maray_amd as M
import scenes
from catrom_model import catrom, catrom_direct, weights
from marayb import encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG = -1


def bits_signed(lo, hi):
    """The narrowest two's-complement width that holds lo .. hi."""
    n = 1
    while not (-(1 << (n - 1)) <= lo and hi <= (1 << (n - 1)) - 1):
        n += 1
    return n


# ---- weights and bounds ------------------------------------------------------------------------------------------------
def test_k2_weights_are_the_literal_list():
    assert weights(2) == [-3, -9, 29, 111, 111, 29, -9, -3]


@pytest.mark.parametrize('k', [2, 4, 8])
def test_weights_are_the_closed_form(k):
    """e(u) = 2 D^3 CatmullRom(n / D) with the BC-spline B = 0, C = 1/2, in exact rationals."""
    from fractions import Fraction as F
    d = 2 * k
    for u, got in zip(CM.footprint(k), weights(k)):
        x = F(abs(2 * u + 1 - k), d)
        cr = F(3, 2) * x ** 3 - F(5, 2) * x ** 2 + 1 if x < 1 else -F(1, 2) * x ** 3 + F(5, 2) * x ** 2 - 4 * x + 2
        assert 0 < x < 2 and x != 1 and got == 2 * d ** 3 * cr
    assert len(weights(k)) == 4 * k and weights(k) == weights(k)[::-1]


@pytest.mark.parametrize('k', [2, 4, 8])
def test_sums_residues_and_extremes(k):
    t = weights(k)
    assert sum(t) == 16 * k ** 4 == {2: 256, 4: 4096, 8: 65536}[k]
    # the partition of unity: the weights a pixel grid gives one sample, whatever its offset in its pixel
    for r in range(k):
        assert sum(t[i] for i in range(4 * k) if i % k == r) == 16 * k ** 3 == {2: 128, 4: 1024, 8: 8192}[k]
    assert (max(t), min(t)) == {2: (111, -9), 4: (987, -75), 8: (8115, -605)}[k]
    assert CM.norm(k) == ((16 * k ** 4) ** 2, {2: 16, 4: 24, 8: 32}[k])


@pytest.mark.parametrize('k', [2, 4, 8])
def test_accumulator_bounds(k):
    t = weights(k)
    pos, neg = sum(x for x in t if x > 0), -sum(x for x in t if x < 0)
    h_max, h_min = 255 * pos, -255 * neg
    assert (h_max, h_min) == {2: (71400, -6120), 4: (1134240, -89760), 8: (18115200, -1403520)}[k]
    f_max, f_min = 255 * (pos * pos + neg * neg), -255 * 2 * pos * neg
    assert (f_max, f_min) == {2: (20138880, -3427200), 4: (5076695040, -798504960), 8: (1294628782080, -199412121600)}[k]
    # the header's widths: 25 / 33 / 41 bits of magnitude with the rounding constant added, one more for the sign
    assert (f_max + CM.norm(k)[0] // 2).bit_length() == {2: 25, 4: 33, 8: 41}[k] and -f_min < f_max
    assert bits_signed(f_min, f_max + CM.norm(k)[0] // 2) == {2: 26, 4: 34, 8: 42}[k]
    if k == 8:
        assert bits_signed(h_min, h_max) == 26
    assert max(abs(x) for x in t) < 1 << 14             # a weight times a byte is a 24-bit multiply
    if k > 2:
        assert f_max >= 1 << 32                         # 32 bits are wrong, signed or unsigned


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_a_constant_image_comes_out_unchanged(k):
    for v in (0, 1, 127, 128, 254, 255):
        s8 = np.full((5 * k, 7 * k, 3), v, np.uint8)
        assert (catrom(s8, k) == v).all(), v
    s8 = np.empty((3 * k, 4 * k, 3), np.uint8)
    s8[...] = (255, 0, 77)
    assert (catrom(s8, k) == np.array([255, 0, 77], np.uint8)).all()


@pytest.mark.parametrize('k', [2, 4, 8])
def test_random_bytes_equal_the_quadruple_loop(k):
    """7 x 5 output pixels: every pixel of the two outer columns and rows clamps its indices."""
    rng = np.random.default_rng(300 + k)
    s8 = rng.integers(0, 256, (5 * k, 7 * k, 3), dtype=np.uint8)
    s8[0, 0] = 255
    s8[-1, -1] = (0, 255, 0)
    got = catrom(s8, k)
    assert got.shape == (5, 7, 3)
    assert np.array_equal(got, catrom_direct(s8, k))


@pytest.mark.parametrize('k', [2, 4, 8])
def test_the_lobe_rasters_reach_both_clamps(k):
    """A condition on the inputs: the lobe raster and its inverse each hold an output byte whose rounded sum is below 0 and
    one whose is above 255, and at k = 4 and 8 the chosen pixel's sum does not fit 32 bits."""
    big_w, shift = CM.norm(k)
    t = weights(k)
    pos, neg = sum(x for x in t if x > 0), -sum(x for x in t if x < 0)
    for s8, at in ((CM.lobe_raster(k), 255 * (pos * pos + neg * neg)), (CM.lobe_inverse(k), -255 * 2 * pos * neg)):
        sums = CM.catrom_sums(s8, k)
        assert (sums[CM.LOBE_PY, CM.LOBE_PX] == at).all()
        m = (sums + big_w // 2) >> shift
        assert (m < 0).any() and (m > 255).any()
        out = catrom(s8, k)
        assert (out[m < 0] == 0).all() and (out[m > 255] == 255).all()
    if k > 2:
        assert CM.catrom_sums(CM.lobe_raster(k), k)[CM.LOBE_PY, CM.LOBE_PX, 0] > 1 << 32


def test_the_lobe_pixel_equals_the_quadruple_loop():
    """The crafted raster through the formula as written, on the window around the chosen pixel (k = 2, 4: the loop is slow)."""
    for k in (2, 4):
        s8 = CM.lobe_raster(k, w=7, h=5, px=3, py=2)
        assert np.array_equal(catrom(s8, k), catrom_direct(s8, k))
        assert np.array_equal(catrom(255 - s8, k), catrom_direct(255 - s8, k))


def test_random_bytes_hardly_ever_clamp():
    """Why the lobe rasters exist: of the parity raster's 7215 bytes few (k = 2) or none round outside 0 .. 255."""
    for k in (2, 4, 8):
        big_w, shift = CM.norm(k)
        m = (CM.catrom_sums(BR.parity_raster(k), k) + big_w // 2) >> shift
        assert ((m < 0) | (m > 255)).mean() < 0.02, k


# ---- mutants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 4, 8])
def test_the_gpu_rasters_tell_every_mutant_from_the_contract(k):
    """Each mutant differs from the contract on at least one of the rasters tests/test_gpu_catrom_bytes.py renders."""
    rasters = CM.gpu_rasters(k)
    want = [catrom(s8, k) for _, s8, _, _ in rasters]
    for name, f in CM.mutants(k):
        assert any(not np.array_equal(f(s8), w) for (_, s8, _, _), w in zip(rasters, want)), name
    names = [n for n, _ in CM.mutants(k)]
    assert len(names) == (6 if k == 2 else 8)


@pytest.mark.parametrize('k', [2, 4, 8])
def test_the_parity_raster_tells_the_band_mutants_at_every_band_height(k):
    """The device renders bands of 1, 3 and 8 output rows on the parity raster only (test_band_rows): on that raster alone, at
    each of those heights, the tent's halo and a clamp to the band differ from the contract."""
    s8 = BR.parity_raster(k)
    want = catrom(s8, k)
    for rows in CM.BAND_ROWS:
        for name, f in CM.band_mutants(k, rows):
            assert not np.array_equal(f(s8), want), (name, rows)


@pytest.mark.parametrize('k', [2, 4, 8])
def test_the_contract_is_its_own_banding(k):
    """catrom_banded with the contract's halo is the contract: the mutants' machinery adds nothing of its own."""
    s8 = BR.parity_raster(k)
    for rows in CM.BAND_ROWS:
        assert np.array_equal(CM.catrom_banded(s8, k, rows, 3 * k // 2), catrom(s8, k))


# ---- options, CLI, façade ----------------------------------------------------------------------------------------------
def test_options_structs_keep_their_size():
    assert C.sizeof(M.api.CtxOpts) == 32 and M.api.CtxOpts.filter.offset == 12
    assert C.sizeof(M.api.GenOpts) == 32 and M.api.GenOpts.filter.offset == 20
    assert (M.FILTER_BOX, M.FILTER_TENT, M.FILTER_CATROM) == (0, 1, 3)


def _cli(*args):
    return subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray')] + list(args), capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'))


def test_cli_filter_options(tmp_path):
    path = os.path.join(HERE, 'golden', 'chess.maray')
    out = tmp_path / 'o.png'
    for bad in (['--filter', 'catrom'], ['--filter', 'catrom', '-s', '1'], ['--filter', 'catrom', '-s', '3'], ['--filter', 'CATROM', '-s', '4'],
                ['--filter', 'catmull-rom', '-s', '4'], ['--filter', 'catrom', '-s', '4', '--linear'], ['--linear', '-s', '2', '--filter', 'catrom']):
        r = _cli('-i', path, '-o', str(out), *bad)
        assert r.returncode == 2 and 'no HIP device' not in r.stderr, (bad, r.stderr)
        assert 'Usage' in r.stderr, (bad, r.stderr)
        assert not out.exists()
    r = _cli('-i', path, '-o', str(out), '--filter', 'catrom', '-s', '4', '--linear')
    assert '--linear' in r.stderr.split('Usage')[0] and 'not built' in r.stderr.split('Usage')[0], r.stderr
    h = _cli('--help')
    assert h.returncode == 0 and 'catrom' in h.stderr
    # a well-formed command line gets as far as the device
    for good in (['-s', '4', '--filter', 'catrom'], ['--filter', 'catrom', '-s', '2'], ['-s', '8', '--filter', 'catrom']):
        ok = _cli('-i', path, '-o', str(out), *good)
        assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), (good, ok.stderr)


def test_facade_refuses_before_any_device():
    """Code -1 here means the arguments were checked first: on a machine without a device anything later is code -8."""
    s = M.Scene(encode((16, 8), scenes.all_ops(16, 8)))
    for k in (0, 1, 3):
        with pytest.raises(M.MarayError) as e:
            M.gen_to_image(s, samples=k, filter=M.FILTER_CATROM)
        assert e.value.code == E_ARG, k
    for k in (2, 4, 8):
        with pytest.raises(M.MarayError) as e:
            M.gen_to_image(s, samples=k, filter=M.FILTER_CATROM, transfer=M.TRANSFER_SRGB)
        assert e.value.code == E_ARG, k
