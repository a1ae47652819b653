"""k_sine_grid_rs on the GPU (3dworld_amd/csrc/terra_kernels.hpp): the heightmap's sine grid with the row operands in scalar registers -- blocks of 256 columns x 64 rows, a
lane's patch 4 columns x 16 rows, a wave's 16 row values by one 64-byte scalar load per term.  Every case compares gen_grid on the device with the oracle's gen_grid bit for
bit, and the min / max words with the oracle grid's min() / max() byte for byte.  Every map has an origin of its own, so tables left over from another map would show.

The shapes are the smallest at which a path can go wrong: a single 4-cell group, one cell short of a block on both axes, exactly one block, one interior block with three
edge blocks, and a grid with interior, right-edge and lower-edge blocks whose last 16-row group is partial.  The term counts cover no chunk at all, a single row, odd and
even chunk lengths and a short last chunk (chunks of at most 27 terms)."""
import numpy as np
import pytest

import sine_grid_path_cases as sg
import turn_prelude_cases as tp
from orclib import assert_bit_equal
from parity_cases import cfg_pair

pytestmark = pytest.mark.gpu

_refs = {}
_origins = {}


def _origin(key):
    """an origin per case, fixed by the order in which the cases first ask for one"""
    if key not in _origins:
        i = len(_origins)
        _origins[key] = (-977.0 + 131.0 * i, 411.0 - 89.0 * i)
    return _origins[key]


def _scene(pkg, t, mff=1, cfg_glaciate=1, islands=True):
    pc_, oc = cfg_pair(pkg, mesh_gen_mode=0, mesh_freq_filter=mff, glaciate=cfg_glaciate, hmap=sg.HMAP if islands else sg.HMAP_NO_ISLANDS)
    return t.init_scene(pc_), oc


def _ref(orc, oc, st, key, nx, ny, flag=True, mss=0):
    if key not in _refs:
        orc.init(oc)
        x0, y0 = _origin(key)
        r = orc.gen_grid(x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, 1 if flag else 0, 0, mss)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def _grid(pkg, t, orc, nx, ny, key, mff=1, flag=True, cfg_glaciate=1, islands=True, mss=0, options=()):
    st, oc = _scene(pkg, t, mff, cfg_glaciate, islands)
    ref = _ref(orc, oc, st, key, nx, ny, flag, mss)
    for k, v in options:
        t.set_option(k, v)
    x0, y0 = _origin(key)
    buf = t.alloc(nx * ny * 4)
    try:
        mn, mx = t.gen_grid_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, pkg.GEN_GLACIATE if flag else 0, mss)
        assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), str(key))
        assert np.array([mn, mx], np.float32).tobytes() == np.array([ref.min(), ref.max()], np.float32).tobytes(), (key, mn, mx, ref.min(), ref.max())
    finally:
        buf.free()


@pytest.mark.parametrize("nx,ny", [(4, 1), (252, 63), (256, 64), (260, 65), (772, 200)])
def test_block_boundaries(pkg, gpu, orc, nx, ny):
    _grid(pkg, gpu, orc, nx, ny, ("shape", nx, ny))


# mesh_freq_filter 0 starts the sum at term 0: min_start_sin m leaves 90 - m terms
@pytest.mark.parametrize("terms", [0, 1, 2, 27, 28, 53, 80, 90])
def test_term_counts(pkg, gpu, orc, terms):
    _grid(pkg, gpu, orc, 260, 65, ("terms", terms), mff=0, mss=90 - terms)


# (GEN_GLACIATE flag, config glaciate, islands): the epilogue's glaciate step and island term off / off, on / off, off / on (two ways) and on / on
@pytest.mark.parametrize("flag,cfg_glaciate,islands", [(False, 1, False), (False, 1, True), (True, 1, False), (True, 0, True), (True, 1, True)])
def test_epilogue_variants(pkg, gpu, orc, flag, cfg_glaciate, islands):
    _grid(pkg, gpu, orc, 260, 65, ("epilogue", flag, cfg_glaciate, islands), flag=flag, cfg_glaciate=cfg_glaciate, islands=islands)


@pytest.mark.parametrize("turn_rows", [0, 1, 64, 128, 1024])
def test_noise_turn_two_contexts(pkg, orc, turn_rows):
    tp.case_two_contexts_take_turns(pkg, lambda: pkg.Terra(0), orc, turn_rows, nx=772, ny=200)


@pytest.mark.parametrize("row0,nrows", [(37, 70), (64, 64)])
def test_row_strips(pkg, gpu, orc, row0, nrows):
    nx, ny, key = 260, 300, ("strips", 260, 300)
    st, oc = _scene(pkg, gpu)
    ref = _ref(orc, oc, st, key, nx, ny)[row0:row0 + nrows]
    x0, y0 = _origin(key)
    buf = gpu.alloc(nx * nrows * 4)
    try:
        mn, mx = gpu.gen_grid_rows_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, row0, nrows, pkg.GEN_GLACIATE)
        assert_bit_equal(ref, buf.download(np.float32, (nrows, nx)), f"rows {row0}..{row0 + nrows} of {nx} x {ny}")
        assert np.array([mn, mx], np.float32).tobytes() == np.array([ref.min(), ref.max()], np.float32).tobytes(), (mn, mx, ref.min(), ref.max())
    finally:
        buf.free()


def test_scratch_reuse(pkg, gpu, orc):
    for i, (nx, ny) in enumerate([(772, 200), (260, 65), (772, 200)]):
        _grid(pkg, gpu, orc, nx, ny, ("reuse", i, nx, ny))


@pytest.mark.parametrize("key,value", [("sg.kc", 20), ("sg.kc", 45), ("sg.rowgroup", 1), ("sg.rowgroup", 1024)])
def test_options_keep_the_bits(pkg, gpu, orc, key, value):
    _grid(pkg, gpu, orc, 772, 200, ("options", 772, 200), options=[(key, value)])


def test_other_row_lengths_stay_on_the_per_cell_instantiation(pkg, gpu, orc):
    _grid(pkg, gpu, orc, 387, 300, ("routing", 387, 300))
