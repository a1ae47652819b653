"""The interior epilogue of k_sine_grid_rs on the GPU (3dworld_amd/csrc/terra_kernels.hpp): the rows of a block inside the grid leave the kernel by nontemporal 1 KB
stores, the rows of an edge block by plain ones.  Every case compares gen_grid on the device with the oracle's gen_grid bit for bit, and the min / max words
with the oracle grid's min() / max() byte for byte.  Every map has an origin of its own, so tables or rows left over from another map would show.

The shapes are one interior block (256 x 64), interior blocks in both directions (512 x 128) and an interior block with right and lower edge blocks (260 x 65); each runs
the five flag / glaciate / island combinations of the epilogue.  Two contexts taking turns with "sg.turn_rows" 64 put the head / tail split of a map on the same code."""
import numpy as np
import pytest

import sine_grid_path_cases as sg
import turn_prelude_cases as tp
from orclib import assert_bit_equal
from parity_cases import cfg_pair

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64), (512, 128), (260, 65)]
# (GEN_GLACIATE flag, config glaciate, islands): glaciate step and island term off / off, off / on, on / off, off / on by the config, on / on
EPILOGUES = [(False, 1, False), (False, 1, True), (True, 1, False), (True, 0, True), (True, 1, True)]

_origins = {}


def _origin(key):
    """an origin per case, fixed by the order in which the cases first ask for one"""
    if key not in _origins:
        i = len(_origins)
        _origins[key] = (613.0 - 157.0 * i, -1291.0 + 103.0 * i)
    return _origins[key]


@pytest.mark.parametrize("flag,cfg_glaciate,islands", EPILOGUES)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_interior_and_edge_blocks(pkg, gpu, orc, nx, ny, flag, cfg_glaciate, islands):
    key = (nx, ny, flag, cfg_glaciate, islands)
    pc_, oc = cfg_pair(pkg, mesh_gen_mode=0, mesh_freq_filter=1, glaciate=cfg_glaciate, hmap=sg.HMAP if islands else sg.HMAP_NO_ISLANDS)
    st = gpu.init_scene(pc_)
    orc.init(oc)
    x0, y0 = _origin(key)
    ref = orc.gen_grid(x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, 1 if flag else 0, 0, 0)
    buf = gpu.alloc(nx * ny * 4)
    try:
        mn, mx = gpu.gen_grid_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, pkg.GEN_GLACIATE if flag else 0, 0)
        assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), str(key))
        assert np.array([mn, mx], np.float32).tobytes() == np.array([ref.min(), ref.max()], np.float32).tobytes(), (key, mn, mx, ref.min(), ref.max())
    finally:
        buf.free()


def test_two_contexts_take_turns_over_the_split(pkg, orc):
    tp.case_two_contexts_take_turns(pkg, lambda: pkg.Terra(0), orc, 64, nx=516, ny=193)
