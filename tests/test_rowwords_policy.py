"""Row words, the parts that need no GPU: which programs get a row flag and which bit, the life of a set's `rowwords` flag and
its tables' accounting (maray_amd/csrc/row_reuse.hpp) and the apply kernel's per-rectangle function (maray_amd/csrc/rowwords.hpp)
as a stand-alone program under AddressSanitizer and UBSan, that the two kernels' text is the PIXEL kernel's, that the pinned
sources do not move with the knob, and the numpy model's own soundness."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import maray_amd as M
import census_scenes as CS
import cover_scenes as CV
import refine_scenes as RS
import rowwords_scenes as RW
from conftest import GOLDEN, ROOT
from marayb import encode
from test_census_policy import narrow_section, pixel_source
from test_cover_policy import kernel_text


def chess():
    return M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('rowwords') / 'rowwords_policy_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'maray_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'rowwords_policy_check.cpp'), '-o', exe])
    return exe


SAN = dict(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')


def test_policy_under_asan_ubsan(checker):
    out = subprocess.run([checker], capture_output=True, text=True, env=dict(os.environ, **SAN))
    assert out.returncode == 0 and 'rowwords policy ok' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def test_apply_function_against_the_model(checker):
    """The apply kernel's per-rectangle function, built for the host, on random `changed` bytes: the words are copied, the flag is
    set exactly where the count of non-zero bytes reaches the threshold."""
    rng = np.random.default_rng(20261021)
    for nw, yrows, threshold in ((1, 32, 8), (3, 32, 1), (3, 8, 2), (12, 128, 32), (2, 16, 16), (3, 32, 33)):
        n, flag = 200, 1 << int(rng.integers(0, 64))
        words = rng.integers(0, 1 << 63, size=(n, nw), dtype=np.uint64) & ~np.uint64(flag)
        density = rng.random(n)[:, None]
        changed = (rng.random((n, yrows)) < density).astype(np.uint8) * rng.integers(1, 256, size=(n, yrows), dtype=np.uint8)
        text = '%d %d %d %d %d\n' % (nw, yrows, threshold, flag, n) + '\n'.join(
            ' '.join(str(int(v)) for v in words[i]) + ' ' + ' '.join(str(int(v)) for v in changed[i]) for i in range(n))
        out = subprocess.run([checker, 'apply'], input=text, capture_output=True, text=True, env=dict(os.environ, **SAN))
        assert out.returncode == 0, out.stderr[-3000:]
        got = np.array([[int(v) for v in ln.split()] for ln in out.stdout.strip().split('\n')], dtype=object)
        take = (changed != 0).sum(axis=1) >= threshold
        want = words.copy()
        want[take, -1] |= np.uint64(flag)
        assert [int(v) for v in got[:, -1]] == [int(v) for v in take], (nw, yrows, threshold)
        assert all(int(got[i, j]) == int(want[i, j]) for i in range(n) for j in range(nw)), (nw, yrows, threshold)
        assert take.any() or threshold > yrows


def test_row_flag():
    tape = chess()
    pos, n_words, _, _ = tape.guard_layout()
    flag, cover = tape.rowwords_flag(), tape.cover_bits()
    assert flag == cover[-1] + 1 and flag not in set(int(p) for p in pos) and flag // 64 == n_words - 1
    lower = lambda color: M.Scene(encode((CV.W, CV.H), color)).lower()
    # nothing eligible, three guarded leaves, no guards: no module
    for t in (lower(RS.shared_bound()), lower(CV.three_leaves())):
        assert t.rowwords_flag() == -1 and t.jit_source_rowwords == ''
    import row_reuse_scenes as RR
    _, plain = RR.lowered(RR.sines())
    assert plain.rowwords_flag() == -1 and plain.jit_source_rowwords == ''
    # an f64 reduction alone: eligible bits, no cover bit -- the flag is the first free bit
    t = lower(CS.three_colours())
    assert t.cover_bits() == [] and t.rowwords_flag() == len([p for p in t.guard_layout()[0] if p >= 0]) and t.jit_source_rowwords
    assert lower(CV.two_ors()).rowwords_flag() == lower(CV.two_ors()).cover_bits()[-1] + 1


def _spare_bits(n_shapes):
    """A boolean OR of n_shapes guarded triangles (and census_scenes' filler)."""
    shapes = [CS._tri(3 * i, 2, 40 + 3 * i, 40) for i in range(n_shapes)]
    return CV._scene(shapes)


def test_no_spare_bit_no_module():
    """A program whose last guard word has one free bit gets a cover bit and no row flag: no module.  Found by growing an OR one
    shape at a time until the cover bit is bit 63 of its word."""
    lower = lambda color: M.Scene(encode((CV.W, CV.H), color)).lower()
    seen = False
    for n in range(50, 70):
        t = lower(_spare_bits(n))
        bits = t.cover_bits()
        if bits and bits[-1] % 64 == 63:
            assert t.rowwords_flag() == -1 and t.jit_source_rowwords == ''
            seen = True
        elif bits:
            assert t.rowwords_flag() == bits[-1] + 1
    assert seen


def test_pixels_rw_is_pixels_covs_text():
    """Line by line: apart from its name, its one more parameter and the strip's guard fetch, maray_jit_pixels_rw is
    maray_jit_pixels_cov."""
    tape = chess()
    cov, rw = kernel_text(tape.jit_source_cover, 'maray_jit_pixels_cov'), kernel_text(tape.jit_source_rowwords, 'maray_jit_pixels_rw')
    first = next(i for i, (a, b) in enumerate(zip(cov[1:], rw[1:]), 1) if a != b)
    # the head: the last parameter line
    assert cov[first].endswith('unsigned rows, unsigned rpw)') and rw[first] == cov[first][:-1] + ', const unsigned long long *__restrict__ mr_rwords)'
    assert cov[0].replace('maray_jit_pixels_cov(', 'maray_jit_pixels_rw(') == rw[0] and cov[1:first] == rw[1:first]
    a0 = next(i for i, ln in enumerate(cov) if 'const unsigned long long mr_gv = ' in ln)
    b0 = next(i for i, ln in enumerate(rw) if 'unsigned long long mr_gv = ' in ln)
    a1 = next(i for i, ln in enumerate(cov) if 'const unsigned long long mr_gnz = ' in ln)
    b1 = next(i for i, ln in enumerate(rw) if 'const unsigned long long mr_gnz = ' in ln)
    assert a0 == b0 and cov[first + 1:a0] == rw[first + 1:b0]
    assert rw[b0] == cov[a0].replace('const unsigned long long mr_gv', 'unsigned long long mr_gv')
    own = rw[b0 + 1:b1]
    assert a1 == a0 + 1 and 0 < len(own) < 12 and all('mr_rw' in ln or ln.strip() == '}' or ln.strip().startswith('{   //') for ln in own)
    assert cov[a1:] == rw[b1:] and len(cov) > 5000
    assert sum('mr_rwords' in ln for ln in rw) == 2            # the parameter and the one conditional load
    tab = lambda s: s[s.index('mr_kc_tab['):s.index('};', s.index('mr_kc_tab['))]
    assert tab(tape.jit_source_cover) == tab(tape.jit_source_rowwords)


def test_rowscan_section_is_the_pixel_kernels_text():
    """The scan's narrow section is the PIXEL kernel's: its own lines hold "mr_rw" or "mr_cv", the reduction loops do not leave
    early, and the conversion and the stores behind the section are dropped."""
    tape = chess()
    pix, scan = narrow_section(pixel_source(tape), 'maray_jit_pixels'), narrow_section(tape.jit_source_rowwords, 'maray_jit_rowscan')
    own = re.compile(r'^    (const mr_mask mr_cin = .*|if \(mr_cin == 0ull\) continue;.*|if \(\(.*\) == 0ull\) continue; .*// nothing to refine|unsigned mr_rwcv = 0u;|mr_mask mr_rwh\d+ = 0ull;)$')
    scan = [ln for ln in scan if not own.match(ln) and 'mr_cv' not in ln and 'mr_rwh' not in ln and 'mr_rwcv' not in ln]
    stop = scan.index('    (void)o0; (void)o1; (void)o2;')
    assert stop > 5000 and len(pix) > stop
    diff = 0
    for a, b in zip(pix[:stop], scan[:stop]):
        if a != b:
            assert re.sub(r' && !mr_covered\(mr_racc\w+\)', '', a) == b, (a, b)
            diff += 1
    assert diff > 0


def test_pinned_sources_do_not_move_with_the_knob():
    """tests/golden/jit_source_hashes.json with MARAY_JIT_ROW_WORDS=0 in the environment, and the census's and the cover's text and
    the code key with the knob at 0 and at 1."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_jit_source_hashes
    want = json.load(open(os.path.join(GOLDEN, 'jit_source_hashes.json')))
    tape = chess()
    old = os.environ.get('MARAY_JIT_ROW_WORDS')
    try:
        got = {}
        for v in ('0', '1'):
            os.environ['MARAY_JIT_ROW_WORDS'] = v
            got[v] = (pixel_source(tape), tape.jit_source_census, tape.jit_source_cover, tape.jit_source_rowwords, tape.jit_code_key)
        os.environ['MARAY_JIT_ROW_WORDS'] = '0'
        hashes = gen_jit_source_hashes.all_hashes()
    finally:
        if old is None:
            del os.environ['MARAY_JIT_ROW_WORDS']
        else:
            os.environ['MARAY_JIT_ROW_WORDS'] = old
    assert got['0'] == got['1'] and got['0'][4] == tape.jit_code_key
    assert hashes == want


def test_numpy_model_is_sound():
    """A cleared bit's guarded conjunctions are 0 on every pixel of the row inside the rectangle, and a set cover bit's OR is 1 on
    every such pixel -- against the oracle's raster of the scene with the OR forced to 1, as tests/test_cover_policy.py does per
    rectangle."""
    from oracle_ffi import Scene as OScene
    from marayb import nat
    one = nat(1)
    render = lambda color: OScene(encode((RW.W, RW.H), color)).render_rows(RW.W, RW.H, 0, RW.H, want_f64=False)[0]
    forced = [CV._paint(one), CV._paint(one, 50), nat(0)]
    for name in ('edge_mid_band', 'all_but_one', 'one_row', 'ragged', 'few_rows'):
        color = RW.PLAIN[name]()
        tape = M.Scene(encode((RW.W, RW.H), color)).lower()
        pos, n_words, gw, gh = tape.guard_layout()
        m = RW.row_words(tape, RW.W, 0, RW.H, threshold=1)
        assert m['flagged'].any(), name
        plan = tape.cover_plan()[0]
        cbit = plan['bit']
        got = RW._bit(m['rwords'], cbit)                                  # (rows, rectangles): the row's cover bit
        px = np.repeat(got[:, :RW.W // gw], gw, axis=1)[:, :RW.W]        # per pixel
        a, b = render(color), render(forced)
        assert np.array_equal(a[px], b[px]), name
        # cleared bits: no pixel of the row has the leaf != 0 (every pixel evaluated, not only where the model looked)
        consts, _, pix = tape.arrays()
        import refine_eval as RE
        n_ynum = RE.n_numeric(tape)
        yv_rows = RE.numeric_yvals_of_rows(tape, RW.W, 0, RW.H)
        ry, rx = np.divmod(np.arange(RW.H * RW.W), RW.W)
        for k, ends in RE.guarded_regions(tape).items():
            p = int(pos[k - n_ynum])
            if p < 0:
                continue
            cleared = RW._bit(m['band'][(np.arange(RW.H) // gh)[:, None] * m['n_rect'] + np.arange(m['n_rect'])[None, :]], p) & ~RW._bit(m['rwords'], p)
            if not cleared.any():
                continue
            covered_here = got & cleared            # cleared under a cover: the OR is 1 there whatever the leaf is
            for end in ends:
                v = RE.run(RE.cone(pix, end), consts, tape.info['n_pix_slots'], RW.H * RW.W, {0: rx.astype(np.float64), 1: ry.astype(np.float64)},
                           yvals=yv_rows[ry], params=None, want=end).reshape(RW.H, RW.W)
                zero_needed = np.repeat((cleared & ~covered_here)[:, :RW.W // gw], gw, axis=1)[:, :RW.W]
                assert not (v[zero_needed] != 0.0).any(), (name, p)
