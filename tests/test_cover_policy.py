"""The cover of guarded ORs, the parts that need no GPU: which programs get cover bits and which bits, the free-bit chooser and
the life of a set's `cover` flag (maray_amd/csrc/row_reuse.hpp) as a stand-alone program under AddressSanitizer and UBSan, that
the two kernels' sections are the PIXEL kernel's text, and the numpy side's own soundness."""
import os
import re
import subprocess

import numpy as np

import maray_amd as M
import census_scenes as CS
import cover_scenes as CV
import refine_scenes as RS
import tape_eval as TE
from conftest import GOLDEN, ROOT
from marayb import encode
from test_census_policy import narrow_section, pixel_source


def chess():
    return M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()


def test_policy_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'cover_policy_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'maray_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'cover_policy_check.cpp'), '-o', exe])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and 'cover policy ok' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def kernel_text(src, kernel):
    body = src[src.index(') ' + kernel + '(') if (') ' + kernel + '(') in src else src.index(kernel + '('):]
    end = body.find('\nextern "C"')
    return (body if end < 0 else body[:end]).split('\n')


def test_pixels_cov_is_the_pixel_kernels_text():
    """Line by line, the whole kernel: apart from its name, maray_jit_pixels_cov adds two lines per OR with a cover bit."""
    tape = chess()
    pix, cov = kernel_text(pixel_source(tape), 'maray_jit_pixels'), kernel_text(tape.jit_source_cover, 'maray_jit_pixels_cov')
    own = [ln for ln in cov if 'mr_cv' in ln]
    assert len(own) == 2 * len(tape.cover_bits()) and own[0].lstrip().startswith('if (((unsigned)') and ' = MR_ALL; else {' in own[0]
    cov = [ln for ln in cov if 'mr_cv' not in ln]
    assert len(pix) == len(cov) > 5000
    assert pix[0].replace('maray_jit_pixels(', 'maray_jit_pixels_cov(') == cov[0]
    assert pix[1:] == cov[1:]
    tab = lambda s: s[s.index('mr_kc_tab['):s.index('};', s.index('mr_kc_tab['))]
    assert tab(pixel_source(tape)) == tab(tape.jit_source_cover)


def test_cover_section_is_the_pixel_kernels_text():
    """The measurement's narrow section: its own lines hold "mr_cv" (the second accumulator, the flags), the reduction loops leave
    on the second accumulator, and the conversion and the stores behind the section are dropped."""
    tape = chess()
    pix, cov = narrow_section(pixel_source(tape), 'maray_jit_pixels'), narrow_section(tape.jit_source_cover, 'maray_jit_cover')
    loops = [ln for ln in cov if 'mr_cv' in ln and ln.lstrip().startswith('for (mr_mask mr_rm')]
    own = re.compile(r'^    (const mr_mask mr_cin = .*|// the flags of this pass.*)$')
    cov = [ln for ln in cov if not own.match(ln) and ('mr_cv' not in ln or ln in loops)]
    stop = cov.index('    (void)o0; (void)o1; (void)o2;')
    assert stop > 5000 and len(pix) > stop and loops
    diff = 0
    for a, b in zip(pix[:stop], cov[:stop]):
        if a != b:
            assert re.sub(r'mr_covered\(mr_racc', 'mr_covered(mr_cvacc', a) == b, (a, b)
            diff += 1
    assert diff == len(loops)


def test_cover_bits():
    tape = chess()
    pos, n_words, _, _ = tape.guard_layout()
    bits = tape.cover_bits()
    assert len(bits) == 1 and bits[0] not in set(int(p) for p in pos) and bits[0] // 64 == n_words - 1
    plan = tape.cover_plan()[0]
    assert len(plan['leaves']) == 128 and all(el and not tainted for _, _, tainted, el in plan['leaves'])
    lower = lambda color: M.Scene(encode((CV.W, CV.H), color)).lower()
    # an f64 colour reduction alone; a bit that gates a plain SKIP too (no eligible bit); three guarded leaves; no guards
    for t in (lower(CS.three_colours()), lower(RS.shared_bound()), lower(CV.three_leaves())):
        assert t.cover_bits() == [] and t.jit_source_cover == ''
    import row_reuse_scenes as RR
    _, plain = RR.lowered(RR.sines())
    assert plain.cover_bits() == [] and plain.jit_source_cover == ''
    # an f64 reduction beside a boolean one: one bit; two boolean ones: two
    assert len(lower(CV.with_colours()).cover_bits()) == 1 and len(lower(CV.two_ors()).cover_bits()) == 2


def test_code_key_does_not_depend_on_the_knob():
    tape = M.Scene(RS.data('zero', 0)).lower()
    old = os.environ.get('MARAY_JIT_GUARD_COVER')
    try:
        os.environ['MARAY_JIT_GUARD_COVER'] = '0'
        off = tape.jit_code_key
        os.environ['MARAY_JIT_GUARD_COVER'] = '1'
        on = tape.jit_code_key
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_COVER']
        else:
            os.environ['MARAY_JIT_GUARD_COVER'] = old
    assert on == off == tape.jit_code_key


def test_numpy_cover_is_sound():
    """The numpy side's own soundness, against the oracle: on the pixels of the rectangles it calls covered, the oracle's raster of
    the scene equals the oracle's raster of the scene with that OR replaced by the constant 1; and clearing bits under a cover
    takes no painted pixel from any reduction in a rectangle where that reduction is not covered."""
    from oracle_ffi import Scene as OScene
    from marayb import nat
    one = nat(1)
    forced = {
        'one_shape': [CV._paint(one), CV._paint(one, 50), nat(0)], 'two_together': [CV._paint(one), CV._paint(one, 50), nat(0)],
        'holes': [CV._paint(one), CV._paint(one, 50), nat(0)], 'row_out': [CV._paint(one), CV._paint(one, 50), nat(0)],
        'shared_ors': [CV.shared_ors()[0], CV._paint(one, 70), nat(0)], 'shared_with_colours': [CV.shared_with_colours()[0], CV._paint(one), nat(0)],
    }
    render = lambda color: OScene(encode((CV.W, CV.H), color)).render_rows(CV.W, CV.H, 0, CV.H, want_f64=False)[0]
    for name, with_one in forced.items():
        tape = M.Scene(encode((CV.W, CV.H), getattr(CV, name)())).lower()
        _, _, gw, gh = tape.guard_layout()
        vb, cb, cov = CV.words(tape, CV.W, 0, CV.H)
        n, ry, rx, rect_of = CV._pixels(CV.W, CV.H, gw, gh)
        assert cov.any() and not cov.all(), name
        inside = cov[rect_of, 0].reshape(CV.H, CV.W)        # (the OR that is forced is the plan's first)
        a, b = render(getattr(CV, name)()), render(with_one)
        assert np.array_equal(a[inside], b[inside]), name
        assert inside.all() or not np.array_equal(a, b), name           # (forcing the OR does change the picture elsewhere)
        before, after = CV.leaf_masks(tape, CV.W, 0, CV.H, cbits=cb), CV.leaf_masks(tape, CV.W, 0, CV.H, cbits=vb)
        for j in range(len(before)):
            free = ~cov[rect_of, j]
            assert np.array_equal(before[j][free], after[j][free]), (name, j)


def test_shared_guard_bits_are_not_cleared():
    """Leaves of two reductions on one guard bit (the lowering interns bounds): the plan clears none of those bits."""
    for name in ('shared_ors', 'shared_with_colours'):
        plan = M.Scene(encode((CV.W, CV.H), getattr(CV, name)())).lower().cover_plan()
        assert [[l[3] for l in r['leaves']].count(False) for r in plan] == [4, 4][:len(plan)], name
    for name in ('two_ors', 'with_colours'):            # shapes moved apart: every bit has one owner
        plan = M.Scene(encode((CV.W, CV.H), getattr(CV, name)())).lower().cover_plan()
        assert all(l[3] for r in plan for l in r['leaves']), name


def test_tainted_leaf_is_left_out_of_the_text():
    """A leaf with a Sin that may defer its tile is tainted: the plan says so and maray_jit_cover has no `mr_cvacc |=` for it."""
    tape = M.Scene(encode((CV.W, CV.H), CV.tainted())).lower()
    leaves = tape.cover_plan()[0]['leaves']
    assert [l[2] for l in leaves].count(True) == 1 and len(leaves) == 5
    ors = [ln for ln in tape.jit_source_cover.split('\n') if ln.strip().startswith('mr_cvacc')]
    assert len(ors) == 4
    assert not CV.covered(tape, CV.W, 0, CV.H).any()
