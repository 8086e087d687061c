"""The census of guard bits, the parts that need no GPU: when a set's census is due (maray_amd/csrc/row_reuse.hpp) as a
stand-alone program under AddressSanitizer and UBSan, which bits the library calls eligible, and that the census kernel's
section is the PIXEL kernel's text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import maray_amd as M
import census_scenes as CS
import params as PR
import refine_scenes as RS
from conftest import GOLDEN, ROOT
from marayb import encode


def test_policy_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'census_policy_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'maray_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'census_policy_check.cpp'), '-o', exe])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and 'census policy ok' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def pixel_source(tape):
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    p = C.c_void_p()
    assert L.maray_jit_source(C.byref(tape.program), C.byref(p)) == 0
    try:
        return C.string_at(p).decode()
    finally:
        L.maray_free(p)


def narrow_section(src, kernel):
    """The lines of the kernel's narrow pass: from the pass loop to the end of the kernel."""
    body = src[src.index(kernel + '('):]
    body = body[body.index('    _Pragma("unroll 1") for (unsigned e = 0; e < 4u; e++) {'):]
    end = body.find('\nextern "C"')
    return (body if end < 0 else body[:end]).split('\n')


def test_census_section_is_the_pixel_kernels_text():
    """Line by line: the census form adds its own lines (the lanes inside the picture, the rectangle's flags, a hit per
    LEAF_END), drops the conversion and the stores behind the section, and differs in the reduction loops' condition only."""
    tape = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
    pix, cen = narrow_section(pixel_source(tape), 'maray_jit_pixels'), narrow_section(tape.jit_source_census, 'maray_jit_census')
    own = re.compile(r'^    (if \(mr_any\(.* & mr_cin\) && mr_lane == 0u\) mr_chit\[\d+\] = 1;|const mr_mask mr_cin = .*|// the flags of this pass.*|unsigned char \*mr_chit = .*)$')
    cen = [ln for ln in cen if not own.match(ln)]
    stop = cen.index('    (void)o0; (void)o1; (void)o2;')
    assert stop > 5000 and len(pix) > stop
    hits = 0
    for a, b in zip(pix[:stop], cen[:stop]):
        if a != b:
            assert re.sub(r' && !mr_covered\(mr_racc\w+\)', '', a) == b, (a, b)
            hits += 1
    assert hits >= 1                                    # chess has OR reductions: their loops do not leave early here
    # the constant table is the PIXEL kernel's, entry for entry
    tab = lambda s: s[s.index('mr_kc_tab['):s.index('};', s.index('mr_kc_tab['))]
    assert tab(pixel_source(tape)) == tab(tape.jit_source_census)


def test_eligible_bits():
    tape = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
    pos, n_words, _, _ = tape.guard_layout()
    el = CS.eligible_guards(tape)
    assert len(tape.census_eligible()) == n_words and not el[pos < 0].any()
    assert el.sum() == 128 and (pos >= 0).sum() == 129          # all but the board's own bit, which gates a plain SKIP
    # refine_scenes.shared_bound: the one bit that has a leaf also gates the group's plain SKIP
    shared = M.Scene(encode((RS.W, RS.H), RS.shared_bound())).lower()
    assert not shared.census_eligible().any() and shared.jit_source_census == ''
    # a leaf that reads a parameter the ROW section does not read
    color, decl = CS.pixel_param()
    scene, _ = PR.declared(dict(color=color, params=decl), (CS.W, CS.H))
    t = scene.lower()
    p, e = t.guard_layout()[0], CS.eligible_guards(t)
    assert t.info['row_params'] == 1 and e.sum() == 3 and ((p >= 0) & ~e).sum() == 1
    # a Sin that may defer its tile: row_reuse_scenes.sines has no guarded reduction at all; a family scene has every leaf eligible
    fam = M.Scene(RS.data('mixed', 0)).lower()
    pf, ef = fam.guard_layout()[0], CS.eligible_guards(fam)
    assert ef.sum() == (pf >= 0).sum() == 12
    # a program without guards
    import row_reuse_scenes as RR
    _, plain = RR.lowered(RR.sines())
    assert plain.jit_source_census == '' and not plain.census_eligible().any()


def test_code_key_does_not_depend_on_the_knob():
    tape = M.Scene(RS.data('zero', 0)).lower()
    old = os.environ.get('MARAY_JIT_GUARD_CENSUS')
    try:
        os.environ['MARAY_JIT_GUARD_CENSUS'] = '0'
        off = tape.jit_code_key
        os.environ['MARAY_JIT_GUARD_CENSUS'] = '1'
        on = tape.jit_code_key
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_CENSUS']
        else:
            os.environ['MARAY_JIT_GUARD_CENSUS'] = old
    assert on == off == tape.jit_code_key


def test_numpy_census_keeps_every_pixel():
    """The numpy side's own soundness: clearing a bit whose leaf is zero on every pixel of the rectangle cannot change a pixel --
    checked where it is cheap to: the count of pixels on which a leaf is != 0 is 0 exactly where its census'd bit is clear."""
    tape = M.Scene(RS.data('zero', 0)).lower()
    pos, _, _, _ = tape.guard_layout()
    counts, el = CS.nonzero_counts(tape, CS.W, 0, CS.H), CS.eligible_guards(tape)
    after = CS.words(tape, CS.W, 0, CS.H)
    for g in np.nonzero(el)[0]:
        bit = (after[:, pos[g] // 64] >> np.uint64(pos[g] % 64)) & np.uint64(1)
        assert not (counts[bit == 0, g] != 0).any(), g
