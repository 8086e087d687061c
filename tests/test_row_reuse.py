"""Reuse of a geometry's ROW outputs, the parts that need no GPU: which parameters the ROW section reads (tape.info
'row_params', what a context keys its ROW tables on) and the policy header (maray_amd/csrc/row_reuse.hpp) as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import maray_amd as M
import row_reuse_scenes as RS
from conftest import ROOT


def row_reads(tape):
    """The mask restated from the tape's ROW ops (include/maray_tape.h: operand kind 3, index 7 + p)."""
    _, row, _ = tape.arrays()
    mask = 0
    for ins in row:
        ins = int(ins)
        op = ins & 0x7F
        if op in (0, 15):
            continue
        for ref in ((ins >> 32) & 0xFFFF, (ins >> 48) & 0xFFFF)[:2 if 10 <= op <= 14 else 1]:
            if ref >> 14 == 3 and (ref & 0x3FFF) >= 7:
                mask |= 1 << ((ref & 0x3FFF) - 7)
    return mask


def test_row_params_of_small_scenes():
    want = [(RS.plain, 0, 0),                   # a scene without parameters
            (RS.colour, 2, 0),                  # parameters that only scale a colour
            (RS.move_y, 1, 1),                  # one that moves a shape in y
            (RS.move_x, 1, 1),                  # ... in x: the guards' bounds read it
            (RS.move_and_colour, 2, 1),         # one of each: only the mover's bit
            (RS.unread, 2, 0),                  # declared, unread (next to one a PIXEL op reads)
            (RS.unread_only, 0, 0)]             # declared, unread, alone: a program without parameters
    for spec, n_params, mask in want:
        _, tape = RS.lowered(spec())
        assert tape.param_count == n_params, spec.__name__
        assert tape.info['row_params'] == mask == row_reads(tape), (spec.__name__, tape.info['row_params'])
        assert tape.info['n_row_ops'] > 0


def test_row_params_is_the_last_field_of_tape_info():
    assert M.api.TapeInfo.row_params_words.offset + 8 == C.sizeof(M.api.TapeInfo)
    _, tape = RS.lowered(RS.sines())
    assert tape.info['row_params'] == 1 and tape.info['sin_bounded'] < tape.info['sin_ops']


def test_a_program_without_parameters_has_mask_zero():
    from conftest import GOLDEN
    tape = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
    assert tape.param_count == 0 and tape.info['row_params'] == 0


def test_policy_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'row_reuse_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'maray_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'row_reuse_check.cpp'), '-o', exe])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and 'row reuse ok' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
