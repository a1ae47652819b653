"""The split noise phase on the CPU through tests/emul/libterra_emul.so: the driver's two be.sine_grid calls with the turn event between them, the tile-row window of
sine_grid_simple, and pipeline.proc_gen_step on four threads -- equal to the oracle bit for bit.  (The product's kernel window is tested in tests/test_gpu_noise_turn.py.)"""
import pytest

import noise_turn_cases as nt


@pytest.mark.parametrize("nx,ny,turn_rows,general", nt.SPLIT_CASES)
def test_forced_split_equals_oracle(pkg, emul, orc, nx, ny, turn_rows, general):
    nt.case_forced_split(pkg, emul, orc, nx, ny, turn_rows, general)


def test_turn_rows_option_values(pkg, emul):
    for v in ("0", "128", "100", "default"):
        emul.set_option("sg.turn_rows", v)
    for v in ("-1", "rows", ""):
        with pytest.raises(pkg.TerraError):
            emul.set_option("sg.turn_rows", v)


def test_four_thread_pipeline_with_split_equals_oracle(pkg, emul_lib, orc):
    nt.case_pipeline_small(pkg, lambda: pkg.Terra(0, emul_lib), orc, N=256)
