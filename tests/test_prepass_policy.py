"""The wide pre-pass, the parts that need no GPU: maray_jit_pixels_pp's text is maray_jit_pixels_rw's apart from its
name and the lines that carry "mr_pp", its narrow section is the PIXEL kernel's, the pinned sources and the code key do not move
with MARAY_JIT_PREPASS, which programs get the kernel, and the numpy model's classes (tests/prepass_scenes.py) are non-trivial
for every scene tests/test_gpu_prepass.py renders."""
import json
import os
import sys

import numpy as np
import pytest

import maray_amd as M
import cover_scenes as CV
import prepass_scenes as PP
import refine_scenes as RS
import rowwords_scenes as RW
from conftest import GOLDEN, ROOT
from marayb import encode
from test_census_policy import narrow_section, pixel_source
from test_cover_policy import kernel_text


def chess():
    return M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()


def test_text_is_pixels_rws_plus_marked_lines():
    tape = chess()
    rw, pp = kernel_text(tape.jit_source_rowwords, 'maray_jit_pixels_rw'), kernel_text(tape.jit_source_prepass, 'maray_jit_pixels_pp')
    own = [ln for ln in pp if 'mr_pp' in ln]
    rest = [ln.replace('maray_jit_pixels_pp(', 'maray_jit_pixels_rw(') for ln in pp if 'mr_pp' not in ln]
    assert rest == rw and len(rw) > 5000 and 20 < len(own) < 200
    # ... and so is everything in front of the kernel: the prologue, the helpers, the constant table entry for entry
    src_rw, src_pp = tape.jit_source_rowwords, tape.jit_source_prepass
    head = lambda s, name: [ln for ln in s[:s.index('extern "C" __global__')].split('\n') if 'mr_pp' not in ln]
    assert head(src_rw, 'rw') == head(src_pp, 'pp')
    assert 'maray_jit_rowscan' not in src_pp and src_pp.count('extern "C" __global__') == 1
    # what the pre-pass adds: one ballot per strip, the skip at the head of the narrow loop, no atomics, no new barrier across wavefronts
    assert sum('mr_ballot' in ln for ln in own) >= 3 and sum('continue;' in ln for ln in own) == 2
    assert not any('atomic' in ln or '__syncthreads' in ln for ln in own)
    assert sum('mr_rwords' in ln for ln in pp) == 2            # the parameter and the one conditional load, as in maray_jit_pixels_rw


def test_narrow_section_is_the_pixel_kernels():
    tape = chess()
    pix, pp = narrow_section(pixel_source(tape), 'maray_jit_pixels'), narrow_section(tape.jit_source_prepass, 'maray_jit_pixels_pp')
    rw = narrow_section(tape.jit_source_rowwords, 'maray_jit_pixels_rw')
    pp = [ln for ln in pp if 'mr_pp' not in ln]
    assert pp == rw and len(pp) > 5000
    assert [ln for ln in pp if 'mr_cv' not in ln] == [ln for ln in pix if 'mr_cv' not in ln]


def test_pinned_sources_do_not_move_with_the_knob():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_jit_source_hashes
    want = json.load(open(os.path.join(GOLDEN, 'jit_source_hashes.json')))
    tape = chess()
    old = os.environ.get('MARAY_JIT_PREPASS')
    try:
        got = {}
        for v in ('0', '1'):
            os.environ['MARAY_JIT_PREPASS'] = v
            got[v] = (pixel_source(tape), tape.jit_source_census, tape.jit_source_cover, tape.jit_source_rowwords, tape.jit_source_prepass, tape.jit_code_key)
            assert gen_jit_source_hashes.all_hashes() == want, v
    finally:
        if old is None:
            del os.environ['MARAY_JIT_PREPASS']
        else:
            os.environ['MARAY_JIT_PREPASS'] = old
    assert got['0'] == got['1'] and got['0'][5] == tape.jit_code_key


def test_which_programs_get_the_kernel():
    lower = lambda color: M.Scene(encode((CV.W, CV.H), color)).lower()
    assert chess().jit_source_prepass
    for t in (lower(RS.shared_bound()), lower(CV.three_leaves())):          # no row words: no pre-pass
        assert t.rowwords_flag() == -1 and t.jit_source_prepass == ''
    import census_scenes as CS
    t = lower(CS.three_colours())                                           # row words without a cover bit: empty rectangles alone
    assert t.cover_bits() == [] and t.jit_source_prepass and 'mr_ppcv' not in t.jit_source_prepass
    t = lower(RW.two_ors())
    assert len(t.cover_bits()) == 2 and 'mr_ppcv1' in t.jit_source_prepass


def test_leafy_mask_literals():
    """The per-lane masks of the strip's ballot: every bit but the cover bits and the row flag."""
    tape = chess()
    _, n_words, _, _ = tape.guard_layout()
    src = tape.jit_source_prepass
    lits = [int(ln.split('mr_ppm = ')[1].split('ull')[0], 16) for ln in src.split('\n') if 'case ' in ln and 'mr_ppm = ' in ln]
    want = [(1 << 64) - 1] * n_words
    for b in tape.cover_bits() + [tape.rowwords_flag()]:
        want[b // 64] &= ~(1 << (b % 64))
    assert lits == want and 'switch (mr_lane %% %du)' % n_words in src


@pytest.mark.parametrize('scene', sorted(PP.PLAIN))
def test_model_classes_are_not_trivial(scene):
    tape = M.Scene(encode((PP.W, PP.H), PP.PLAIN[scene]())).lower()
    assert tape.jit_source_prepass
    c, m = PP.model(tape, PP.W, 0, PP.H)
    need = ('all_leafy', 'mixed') if scene == 'sin_in_leaf' else PP.CLASSES[1:]      # (a tainted leaf is never covered: its tile has no leafless-only row)
    for k in need:
        assert c['tile_rows'][k] > 0, (scene, c)
    assert sum(c['tile_rows'].values()) == PP.H * 2 and c['narrow_passes_after'] < c['narrow_passes_before']
    assert c['narrow_passes_before'] - c['narrow_passes_after'] == sum(c['leafless_passes'].values())


def test_model_classify_by_hand():
    """Two tiles, one row, one word; cover bit 5, flag bit 6."""
    w = lambda *v: np.array(v, np.uint64).reshape(1, len(v), 1)
    c = PP.classify(w(0, 0, 0, 0, 1, 32, 0, 33), [5])
    assert c['tile_rows'] == {'all_zero': 1, 'all_leafy': 0, 'mixed': 1, 'leafless_only': 0} and (c['narrow_passes_before'], c['narrow_passes_after'], c['pre_passes']) == (4, 2, 1)
    c = PP.classify(w(32, 0, 32, 0, 1, 2, 4, 8), [5])
    assert c['tile_rows'] == {'all_zero': 0, 'all_leafy': 1, 'mixed': 0, 'leafless_only': 1} and c['leafless_passes'] == {'mixed': 0, 'leafless_only': 4}
    # a flagged rectangle takes its row's words, the others the band's without the flag
    xb = np.array([[64 | 3], [64], [1], [0]], np.uint64)
    rw = np.array([[0], [32], [7], [7]], np.uint64)
    got = PP.launch_words(xb, rw, 6, 1, 32)
    assert got.reshape(-1).tolist() == [0, 32, 1, 0]
