"""The turn prelude on the GPU: a map's table launch (x / y sine tables, island tables, reset of the fused min / max words; fBm modes: the fill and the island launch) is
enqueued in front of the host wait for the previous map's turn event, the grid launches behind it -- the oracle's grid and its min / max, bit for bit, on the smallest
shapes where the new order can go wrong.  tests/test_turn_prelude_emul.py is the CPU twin."""
import pytest

import turn_prelude_cases as tp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("turn_rows", [128, 256])
def test_two_contexts_take_turns_over_three_maps(pkg, orc, turn_rows):
    tp.case_two_contexts_take_turns(pkg, lambda: pkg.Terra(0), orc, turn_rows)


def test_two_turn_calls_back_to_back_with_scratch_growth(pkg, gpu, orc):
    tp.case_back_to_back_growth(pkg, gpu, orc)


@pytest.mark.parametrize("mode,nx,ny,turn_rows", tp.ONE_MAP_CASES)
def test_one_map_behind_another(pkg, gpu, orc, mode, nx, ny, turn_rows):
    tp.case_one_map_behind_another(pkg, gpu, orc, mode, nx, ny, turn_rows)


def test_invalid_call_returns_its_error_and_leaves_the_context_usable(pkg, gpu, orc):
    tp.case_invalid_call_then_valid(pkg, gpu, orc)
