"""The turn prelude on the CPU through tests/emul/libterra_emul.so: the driver's order -- tables and min / max reset, the wait, the grid launches -- equal to the oracle bit
for bit.  (On a real stream, with the previous map's kernels still queued: tests/test_gpu_turn_prelude.py.)"""
import pytest

import turn_prelude_cases as tp


@pytest.mark.parametrize("turn_rows", [128, 256])
def test_two_contexts_take_turns_over_three_maps(pkg, emul_lib, orc, turn_rows):
    tp.case_two_contexts_take_turns(pkg, lambda: pkg.Terra(0, emul_lib), orc, turn_rows)


def test_two_turn_calls_back_to_back_with_scratch_growth(pkg, emul, orc):
    tp.case_back_to_back_growth(pkg, emul, orc)


@pytest.mark.parametrize("mode,nx,ny,turn_rows", tp.ONE_MAP_CASES)
def test_one_map_behind_another(pkg, emul, orc, mode, nx, ny, turn_rows):
    tp.case_one_map_behind_another(pkg, emul, orc, mode, nx, ny, turn_rows)


def test_invalid_call_returns_its_error_and_leaves_the_context_usable(pkg, emul, orc):
    tp.case_invalid_call_then_valid(pkg, emul, orc)
