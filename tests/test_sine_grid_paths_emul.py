"""The host side of the sine grid's tables without a GPU: the bound on the table rows that k_sine_grid's staging reads (terra_common.hpp: sg_last_row_read), checked for
every start term and chunk length by a stand-alone program under the address and undefined-behaviour sanitizers (tests/emul/sg_table_rows_main.cpp); and the table
launches of terra_driver.hpp -- rows kstart..90 only, at the current grid's row length in scratch buffers that were grown by other grids -- through the emulator
(tests/sine_grid_path_cases.py; the emulator sums with sine_grid_simple, not with the kernel)."""
import pytest

import sine_grid_path_cases as sg
from test_host_staging_emul import run_sanitized


def test_sanitized_table_row_bound(tmp_path):
    run_sanitized(tmp_path, "sg_table_rows_main")


@pytest.mark.parametrize("nx,ny", [(132, 130), (130, 129), (4, 1)])
@pytest.mark.parametrize("mff,mss", sg.TERMS)
def test_grid_equals_oracle(pkg, emul, orc, nx, ny, mff, mss):
    sg.case_grid(pkg, emul, orc, nx, ny, mff=mff, mss=mss)


def test_row_strip_equals_oracle(pkg, emul, orc):
    sg.case_row_strip(pkg, emul, orc)


def test_scratch_reuse_equals_oracle(pkg, emul, orc):
    sg.case_scratch_reuse(pkg, emul, orc)


def test_tile_batch_equals_oracle(pkg, emul, orc):
    sg.case_tile_batch(pkg, emul, orc)
