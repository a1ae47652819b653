"""The split noise phase on the GPU: k_sine_grid launched over a window of tile rows (all but the last T rows, the turn event, the last T rows) gives the oracle's grid
and the oracle grid's min / max, bit for bit -- on the smallest grids where the window can go wrong, and through pipeline.proc_gen_step on four contexts.
tests/test_gpu_at_size.py::test_headline_mode_four_contexts_in_flight_equal_oracle is the full-size form (the split at its default)."""
import pytest

import noise_turn_cases as nt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny,turn_rows,general", nt.SPLIT_CASES)
def test_forced_split_equals_oracle(pkg, gpu, orc, nx, ny, turn_rows, general):
    nt.case_forced_split(pkg, gpu, orc, nx, ny, turn_rows, general)


def test_four_contexts_with_split_equal_oracle(pkg, orc):
    nt.case_pipeline_small(pkg, lambda: pkg.Terra(0), orc, N=512)
