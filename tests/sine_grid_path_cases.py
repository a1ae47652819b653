"""Cases of the paths inside k_sine_grid and of the tables it reads (3dworld_amd/csrc/terra_kernels.hpp, terra_common.hpp: sg_last_row_read), shared by the GPU tests (the
kernel) and the emulator tests (the host side: table rows kstart..90 only, padded tables in scratch buffers that grow and are reused).  Every comparison is against the
oracle's gen_grid / tile_create_zvals and the oracle grid's min() / max(), bit for bit.

The grids are the smallest at which a path can go wrong: one interior block, interior blocks only, partial blocks on both edges with rows of whole 16-byte groups (packed
epilogue, guarded form), a single group, and a row length that is no multiple of 4 (the per-cell instantiation).  mesh_freq_filter 0 / 1 / 8 start the sum at term
0 / 10 / 60 (the filter stops at 60: 90, 80 and 30 terms); min_start_sin 80 and 89 leave 10 terms and one.  Crossed with sg.kc 20 / 27 / 45 that is five, four, three, two
chunks and one, of odd and of even length, down to a single row -- an odd chunk copies one table row more than it sums, the last one the zero row behind row 89."""
import numpy as np

from orclib import assert_bit_equal
from parity_cases import cfg_pair

HMAP = [1000.0, 0, 0, 0, 1000.0, 0, 0, 0, 0, 5.0, 0.001, -4.0, 0, 0]           # islands on (sine_mag 5)
HMAP_NO_ISLANDS = [1000.0, 0, 0, 0, 1000.0, 0, 0, 0, 0, 0.0, 0.001, -4.0, 0, 0]  # sine_mag 0

# (nx, ny)
GRIDS = [(128, 128), (256, 384), (132, 130), (4, 1), (130, 129)]
TURN_CASES = [(384, 300, 128), (384, 300, 256)]  # a window with ty0 != 0: an interior head and a partial tail
TERMS = [(0, 0), (1, 0), (8, 0), (8, 80), (8, 89)]  # (mesh_freq_filter, min_start_sin)
TERMS_KC = [(mff, mss, kc) for mff, mss in TERMS for kc in (20, 27, 45)]
# (GEN_GLACIATE flag, config glaciate, islands): gl and sm of the epilogue on / on, off / on, on / off, off / off
FLAG_CASES = [(True, 1, True), (True, 0, True), (True, 1, False), (False, 1, True)]

_refs = {}


def _origin(nx, ny):
    return -nx / 2 + 33.0, -ny / 2 - 71.0


def _scene(pkg, t, orc, mff=1, cfg_glaciate=1, islands=True):
    pc_, oc = cfg_pair(pkg, mesh_gen_mode=0, mesh_freq_filter=mff, glaciate=cfg_glaciate, hmap=HMAP if islands else HMAP_NO_ISLANDS)
    st = t.init_scene(pc_)
    return st, oc


def _ref_grid(orc, oc, key, st, nx, ny, flag, mss=0):
    if key not in _refs:
        orc.init(oc)
        x0, y0 = _origin(nx, ny)
        ref = orc.gen_grid(x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, 1 if flag else 0, 0, mss)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def case_grid(pkg, t, orc, nx, ny, mff=1, kc=27, flag=True, cfg_glaciate=1, islands=True, minmax=True, mss=0):
    """one grid through the device entry point, with or without the fused min / max"""
    st, oc = _scene(pkg, t, orc, mff, cfg_glaciate, islands)
    assert st.start_eval_sin == {0: 0, 1: 10, 8: 60}[mff]
    ref = _ref_grid(orc, oc, (nx, ny, mff, flag, cfg_glaciate, islands, mss), st, nx, ny, flag, mss)
    t.set_option("sg.kc", kc)
    x0, y0 = _origin(nx, ny)
    flags = pkg.GEN_GLACIATE if flag else 0
    buf = t.alloc(nx * ny * 4)
    try:
        what = f"{nx} x {ny}, mesh_freq_filter {mff}, min_start_sin {mss}, sg.kc {kc}, GEN_GLACIATE {flag}, glaciate {cfg_glaciate}, islands {islands}"
        if minmax:
            mn, mx = t.gen_grid_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, flags, mss)
            assert (np.float32(mn), np.float32(mx)) == (ref.min(), ref.max()), (what, mn, mx, ref.min(), ref.max())
        else:
            t.gen_grid_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, flags, mss)
            t.synchronize()
        assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), what)
    finally:
        buf.free()


def case_turn(pkg, t, orc, nx, ny, turn_rows):
    """the turn entry with a forced split: two launches over windows of the grid's tile rows, one pair of min / max words"""
    st, oc = _scene(pkg, t, orc)
    ref = _ref_grid(orc, oc, (nx, ny, 1, True, 1, True, 0), st, nx, ny, True)
    t.set_option("sg.turn_rows", turn_rows)
    x0, y0 = _origin(nx, ny)
    buf, mm = t.alloc(nx * ny * 4), t.alloc(8)
    ev_prev, ev = t.event_create(), t.event_create()
    try:
        t.event_record(ev_prev)
        t.gen_grid_minmax_turn_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, mm.ptr, ev_prev, ev, pkg.GEN_GLACIATE)
        t.synchronize()
        got = mm.download(np.float32, (2,))
        assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), f"{nx} x {ny}, sg.turn_rows {turn_rows}")
        assert (got[0], got[1]) == (ref.min(), ref.max()), (got, ref.min(), ref.max())
    finally:
        t.event_destroy(ev_prev); t.event_destroy(ev)
        buf.free(); mm.free()


def case_row_strip(pkg, t, orc, nx=384, ny=300, row0=128, nrows=172):
    """rows [row0, row0 + nrows) of the grid through the row-strip entry: the strip's own tables (its first row is the grid's row row0), the strip's min / max"""
    st, oc = _scene(pkg, t, orc)
    ref = _ref_grid(orc, oc, (nx, ny, 1, True, 1, True, 0), st, nx, ny, True)[row0:row0 + nrows]
    x0, y0 = _origin(nx, ny)
    buf = t.alloc(nx * nrows * 4)
    try:
        mn, mx = t.gen_grid_rows_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, row0, nrows, pkg.GEN_GLACIATE)
        assert_bit_equal(ref, buf.download(np.float32, (nrows, nx)), f"rows {row0}..{row0 + nrows} of {nx} x {ny}")
        assert (np.float32(mn), np.float32(mx)) == (ref.min(), ref.max()), (mn, mx, ref.min(), ref.max())
    finally:
        buf.free()


def case_scratch_reuse(pkg, t, orc):
    """one context: tables that grow, are reused by a smaller and a larger grid, are released and grow again -- row k of a table lies at k * (the CURRENT padded row length)"""
    st, oc = _scene(pkg, t, orc)
    for nx, ny, release in [(384, 300, False), (128, 128, False), (512, 512, True), (132, 130, False)]:
        ref = _ref_grid(orc, oc, (nx, ny, 1, True, 1, True, 0), st, nx, ny, True)
        x0, y0 = _origin(nx, ny)
        buf = t.alloc(nx * ny * 4)
        try:
            mn, mx = t.gen_grid_minmax_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, pkg.GEN_GLACIATE)
            assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), f"{nx} x {ny} on reused scratch")
            assert (np.float32(mn), np.float32(mx)) == (ref.min(), ref.max()), (nx, ny, mn, mx)
        finally:
            buf.free()
        if release:
            t.release_scratch()


def case_tile_batch(pkg, t, orc):
    """one dense 3 x 3 batch at S = 128: the tile variant of the kernel shares the staging and the padded tables"""
    pc_, oc = cfg_pair(pkg, mesh_gen_mode=0, mesh_freq_filter=1)
    t.init_scene(pc_)
    orc.init(oc)
    tiles = [(tx, ty) for ty in (-1, 0, 1) for tx in (2, 3, 4)]
    z, _, _, _ = t.tiles_create_zvals(tiles, 0, stats=False, normals=False)
    for i, (tx, ty) in enumerate(tiles):
        zo, _ = orc.tile_create_zvals(tx, ty, 0)
        assert_bit_equal(zo, z[i], f"tile {tx}, {ty}")
