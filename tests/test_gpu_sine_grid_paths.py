"""k_sine_grid's paths on the GPU (tests/sine_grid_path_cases.py): direct-to-LDS staging of whole row pairs from tables padded behind row 89, the straight-line epilogue of
blocks inside the grid and the guarded one of edge blocks, the per-cell instantiation for row lengths that are no multiple of 4, the tile variant -- the oracle's grid and
its min / max, bit for bit."""
import pytest

import sine_grid_path_cases as sg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny", sg.GRIDS)
def test_grid_equals_oracle(pkg, gpu, orc, nx, ny):
    sg.case_grid(pkg, gpu, orc, nx, ny)


@pytest.mark.parametrize("nx,ny,turn_rows", sg.TURN_CASES)
def test_turn_windows_equal_oracle(pkg, gpu, orc, nx, ny, turn_rows):
    sg.case_turn(pkg, gpu, orc, nx, ny, turn_rows)


def test_row_strip_equals_oracle(pkg, gpu, orc):
    sg.case_row_strip(pkg, gpu, orc)


@pytest.mark.parametrize("nx,ny", [(132, 130), (130, 129)])
@pytest.mark.parametrize("mff,mss,kc", sg.TERMS_KC)
def test_terms_and_chunks_equal_oracle(pkg, gpu, orc, mff, mss, kc, nx, ny):
    sg.case_grid(pkg, gpu, orc, nx, ny, mff=mff, kc=kc, mss=mss)


@pytest.mark.parametrize("nx,ny", [(256, 384), (132, 130)])
@pytest.mark.parametrize("minmax", [True, False])
@pytest.mark.parametrize("flag,cfg_glaciate,islands", sg.FLAG_CASES)
def test_flags_equal_oracle(pkg, gpu, orc, flag, cfg_glaciate, islands, minmax, nx, ny):
    sg.case_grid(pkg, gpu, orc, nx, ny, flag=flag, cfg_glaciate=cfg_glaciate, islands=islands, minmax=minmax)


def test_scratch_reuse_equals_oracle(pkg, gpu, orc):
    sg.case_scratch_reuse(pkg, gpu, orc)


def test_tile_batch_equals_oracle(pkg, gpu, orc):
    sg.case_tile_batch(pkg, gpu, orc)
