"""GPU parity tests: the product (libterra_hip.so, HIP kernels on gfx950) through the C ABI against
  (1) the golden vectors produced by the reference itself, (2) the oracle on the same seeded inputs, bit-exact,
  (3) at BASELINE.json's full sizes, size-independent properties: the LDS-tiled kernels against the independent
      one-thread-per-cell kernels, speculative erosion against the strictly serial single-lane walk, oracle rows / sub-grids.
Nothing here reads /root/reference.  Run with `pytest -m gpu` on the MI355X box."""
import os

import numpy as np
import pytest

import orclib
import parity_cases as pc
from orclib import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_scene_and_grids_golden(pkg, gpu, mode):
    pc.case_scene_and_grids(pkg, gpu, mode)


def test_shapes_golden(pkg, gpu):
    pc.case_shapes(pkg, gpu)


@pytest.mark.parametrize("mode,n,mss,force", [(0, 1030, 0, False), (0, 300, 50, False), (1, 300, 0, True), (1, 515, 0, False), (2, 515, 0, False), (3, 200, 0, False), (4, 260, 0, False)])
def test_grid_vs_oracle(pkg, gpu, orc, mode, n, mss, force):
    pc.case_grid_vs_oracle(pkg, gpu, orc, mode, n, mss, force)


def test_sine_epilogue_variants(pkg, gpu, orc):
    pc.case_sine_epilogue_variants(pkg, gpu, orc)


def test_hot_sqrt_equals_sqrtf(gpu):
    """the shortened square-root sequence of the droplet step (csrc/terra_erosion.hpp: sqrt_rn / sqrt_rn_direction) over ALL 2^32 fp32 bit patterns: bit-equal to the
    compiler's sqrtf and to the correctly rounded (float)sqrt((double)x)"""
    assert gpu.selftest_hot_sqrt(1) == 0


def test_erosion_golden(pkg, gpu):
    pc.case_erosion_golden(pkg, gpu)


@pytest.mark.parametrize("n,iters", [(96, 50), (256, 300), (512, 1000), (1024, 3000), (4096, 1000)])
def test_speculative_erosion_equals_oracle(pkg, gpu, orc, n, iters):
    pc.case_erosion_vs_oracle(pkg, gpu, orc, n, iters)


def test_erosion_serial_flags_and_overflow_fallback(pkg, gpu, orc):
    pc.case_erosion_vs_oracle(pkg, gpu, orc, 128, 120, flags=pkg.ERODE_SERIAL)
    pc.case_erosion_vs_oracle(pkg, gpu, orc, 256, 500, flags=pkg.ERODE_SERIAL_WAVE)
    gpu.set_erosion_tuning(window=64, block_list_capacity=16)
    r, _ = pc.case_erosion_vs_oracle(pkg, gpu, orc, 512, 400)
    assert r.serial_fallbacks >= 1 and r.windows >= 7


@pytest.mark.parametrize("n,iters,window,slice_steps,blk_cap,near", [(256, 3000, 64, 16, 0, 0), (256, 1200, 48, 8, 12, 0), (512, 20000, 512, 8, 0, 16), (1024, 30000, 4096, 64, 0, 512), (512, 8000, 256, 32, 0, 100000)])
def test_erosion_sliding_ring(pkg, gpu, orc, n, iters, window, slice_steps, blk_cap, near):
    r, _ = pc.case_erosion_sliding_ring(pkg, gpu, orc, n, iters, window, slice_steps, blk_cap, near=near)
    assert r.rounds > r.windows
    if blk_cap:
        assert r.serial_fallbacks >= 1


@pytest.mark.parametrize("ck,near,window,slice_steps", [("1:16", 0, 64, 16), ("4:16", 100000, 256, 32), ("7:3", 8, 128, 9)])
def test_erosion_checkpointed_retraces(pkg, gpu, orc, ck, near, window, slice_steps):
    r, _ = pc.case_erosion_sliding_ring(pkg, gpu, orc, 256, 6000, window, slice_steps, near=near, ck=ck)
    assert r.checkpoint_resumes > 0 and r.checkpoint_steps_saved > 0


def test_grid_degenerate_shapes(pkg, gpu, orc):
    pc.case_grid_degenerate_shapes(pkg, gpu, orc)


def test_tile_batch_shapes(pkg, gpu, orc):
    pc.case_tile_batch_shapes(pkg, gpu, orc)


def test_hmap_edits_and_export(pkg, gpu, orc, tmp_path):
    pc.case_hmap_edits_and_export(pkg, gpu, orc, tmp_path)


def test_tile_weights_texture(pkg, gpu, orc):
    pc.case_tile_weights(pkg, gpu, orc)


def test_tile_ao_lighting(pkg, gpu, orc):
    pc.case_tile_ao(pkg, gpu, orc)


def test_tile_mesh_shadows(pkg, gpu, orc):
    pc.case_tile_mesh_shadows(pkg, gpu, orc)


def test_tile_mesh_shadows_halo_interface(pkg, gpu, orc):
    pc.case_tile_mesh_shadows_halo(pkg, gpu, orc)


def test_tiles_post_pass_on_adversarial_zvals(pkg, gpu, orc):
    for zoff in (0, 4):  # 4: zvals not 16-byte aligned, the post pass at S = 128 runs k_tile_post_sized
        pc.case_tiles_post_adversarial(pkg, gpu, orc, zoff)


def test_tiles_from_heightmap_texture(pkg, gpu, orc):
    pc.case_tiles_from_heightmap(pkg, gpu, orc)


@pytest.mark.parametrize("n,iters,retraces,flags", [(512, 400, 100000, 0), (384, 300, 100000, 2), (256, 500, 3, 0), (128, 120, 0, 2), (1024, 300, 2, 2), (2048, 2000, 40, 2), (1024, 60, None, 0)])
def test_sparse_erosion_scheduler(pkg, gpu, orc, n, iters, retraces, flags):
    """the lean trace kernel + check / commit / re-trace rounds of the sparse scheduler, forced onto maps where droplets meet"""
    r, _ = pc.case_erosion_sparse(pkg, gpu, orc, n, iters, "1", retraces, flags)
    if retraces == 100000:
        assert r.sparse_droplets == iters and r.sparse_retraces > 0 and r.rounds == 1 + r.sparse_retraces
    elif retraces is not None:
        assert 0 < r.sparse_droplets < iters and r.sparse_retraces <= retraces


@pytest.mark.parametrize("n,iters,world,eroder,force,retraces", [
    (1024, 60, 2, 0, None, None), (2048, 300, 3, 1, None, None), (512, 400, 3, 2, "1", 100000), (256, 500, 2, 1, "1", 3), (128, 120, 2, 0, "1", 0),
    (192, 3000, 2, 1, None, None), (640, 250, 1, 0, "1", 100000), (2048, 2000, 8, 5, "1", 40), (4096, 1000, 8, 3, None, None)])
def test_sharded_sparse_erosion(pkg, gpu, orc, n, iters, world, eroder, force, retraces):
    """terra_erosion_shard_*: the ranks of the one-grid pipeline as contexts on this GPU (own streams, arenas a stride apart in one allocation): each traces the droplets
    that start in its strip, the eroding one gathers the traces and checks / commits -- the oracle's grid bit for bit (uneven and empty strips, cross-strip conflicts,
    hand-over to the general scheduler, the dense run the sparse scheduler does not take, eight strips)"""
    rep = pc.case_erosion_sharded(pkg, lambda: pkg.Terra(0), orc, n, iters, world, eroder, force, retraces)
    if retraces == 100000:
        assert rep.sparse_droplets == iters and rep.sparse_retraces > 0
    elif retraces == 3:
        assert 0 < rep.sparse_droplets < iters
    elif force is None and iters == 3000:
        assert rep.sparse_droplets == 0


def test_sparse_erosion_edge_cases_and_probe_pass(pkg, gpu, orc):
    pc.case_erosion_edge_sparse(pkg, gpu, orc)


def test_erosion_context_reuse(pkg, gpu, orc):
    pc.case_erosion_context_reuse(pkg, gpu, orc)


def test_erosion_edge_cases(pkg, gpu, orc):
    pc.case_erosion_edge(pkg, gpu, orc)


@pytest.mark.parametrize("mode,iters", [(0, 0), (0, 300), (1, 100), (4, 0)])
def test_tiles(pkg, gpu, orc, mode, iters):
    pc.case_tiles(pkg, gpu, orc, mode, iters)


def test_tile_golden(pkg, gpu):
    pc.case_tile_golden(pkg, gpu)


@pytest.mark.parametrize("bands,eroded,whole", [("1", 0, "1"), ("0", 0, "1"), ("1", 60, "1"), ("1", 0, "0"), ("0", 60, "0")])
def test_tile_ao_context_as_bands_and_as_squares(pkg, gpu, orc, bands, eroded, whole):
    """calc_mesh_ao_lighting over a dense 8 x 4 batch (a tile-column count the band form accepts): the AO context evaluated as four bands around each tile ("ao.bands" 1: its
    centre is the tile's own, here also eroded, heights) and as whole squares; the rays from one workgroup per tile with the whole context in LDS ("ao.whole" 1,
    k_tile_ao_tile) and from four band workgroups (k_tile_ao) -- the oracle's bytes every way"""
    pc_, oc = pc.cfg_pair(pkg, mesh_gen_mode=0)
    gpu.init_scene(pc_); orc.init(oc)
    tiles = [(tx, ty) for ty in range(-2, 2) for tx in range(3, 11)]
    gpu.set_option("ao.bands", bands); gpu.set_option("ao.whole", whole)
    try:
        z, _, _, _ = gpu.tiles_create_zvals(tiles, eroded)
        ao = gpu.tiles_ao_lighting(tiles, z)
    finally:
        gpu.set_option("ao.bands", "1"); gpu.set_option("ao.whole", "1")
    for i, (tx, ty) in enumerate(tiles):
        zo, _ = orc.tile_create_zvals(tx, ty, eroded)
        assert_bit_equal(z[i], zo, f"zvals {tx},{ty}")
        assert (ao[i] == orc.tile_ao_lighting(tx, ty, zo)).all(), (bands, eroded, tx, ty)


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_voxels_random_shapes(pkg, gpu, orc, seed):
    """k_voxel_sines_cols / k_voxel_sines / k_voxel_noise on random shapes, positions, generators and slabs"""
    pc.case_voxels_random(pkg, gpu, orc, seed, 24, big=True)


def test_voxels(pkg, gpu, orc):
    pc.case_voxels_golden(pkg, gpu)
    pc.case_voxels_vs_oracle(pkg, gpu, orc, 0, (96, 64, 64))
    pc.case_voxels_vs_oracle(pkg, gpu, orc, 0, (17, 9, 300))
    pc.case_voxels_vs_oracle(pkg, gpu, orc, 1, (24, 20, 33))
    pc.case_voxels_vs_oracle(pkg, gpu, orc, 2, (24, 20, 33))


def test_proc_gen_and_quantize(pkg, gpu, orc):
    pc.case_proc_gen(pkg, gpu, orc, 512, 500)
    pc.case_quantize_golden(pkg, gpu)


@pytest.mark.parametrize("mode,n", [(0, 1500), (0, 131), (1, 700), (4, 300)])
def test_gen_grid_minmax(pkg, gpu, orc, mode, n):
    pc.case_gen_grid_minmax(pkg, gpu, orc, mode, n)


@pytest.mark.parametrize("mode,nx,ny,nstrips", [(0, 1030, 777, 8), (0, 256, 300, 3), (1, 300, 200, 4), (4, 140, 90, 2), (2, 64, 5, 8)])
def test_grid_row_strips(pkg, gpu, orc, mode, nx, ny, nstrips):
    pc.case_grid_row_strips(pkg, gpu, orc, mode, nx, ny, nstrips)


@pytest.mark.parametrize("gen_mode,shape,nslabs", [(0, (96, 64, 64), 8), (0, (17, 9, 300), 2), (1, (24, 20, 33), 3), (2, (24, 20, 33), 4)])
def test_voxel_slabs(pkg, gpu, orc, gen_mode, shape, nslabs):
    pc.case_voxel_slabs(pkg, gpu, orc, gen_mode, shape, nslabs)


def test_eval_points_all_modes(pkg, gpu, orc):
    """terra_eval_points (a8: eval_mesh_sin_terms_scaled + get_exact_zval), every mode and branch, bit-exact"""
    pc.case_eval_points(pkg, gpu, orc)


def test_ground_mesh_and_point_queries(pkg, gpu, orc):
    pc.case_ground_mesh_and_point_queries(pkg, gpu, orc)


def test_mesh_text_file_read_write(pkg, gpu, orc, tmp_path):
    pc.case_mesh_text_file(pkg, gpu, orc, tmp_path)


def test_generator_protocol(pkg, gpu, orc):
    pc.case_generator_protocol(pkg, gpu, orc)


def test_inject_engine_state(pkg, gpu, orc):
    pc.case_inject_engine_state(pkg, gpu, orc)


def test_api_errors(pkg, gpu):
    pc.case_api_errors(pkg, gpu)


# ---------------------------------------------------------------- full-size properties (BASELINE.json: 4096^2 and 16384^2)

def _simple_ctx(pkg):
    os.environ["TERRA_SIMPLE_KERNELS"] = "1"
    try:
        return pkg.Terra(0)
    finally:
        del os.environ["TERRA_SIMPLE_KERNELS"]


@pytest.mark.parametrize("N,octaves", [(4096, 9), (16384, 8)])
def test_full_size_sine_grid_tiled_equals_per_cell_kernel_and_oracle_rows(pkg, gpu, orc, N, octaves):
    ff = 0 if octaves == 9 else 1
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_freq_filter=ff))
    simple = _simple_ctx(pkg)
    simple.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_freq_filter=ff))
    a, b = gpu.alloc(N * N * 4), simple.alloc(N * N * 4)
    gpu.gen_grid_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    simple.gen_grid_dev(b.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    gpu.synchronize(); simple.synchronize()
    za = a.download(np.float32, (N, N))
    zb = b.download(np.float32, (N, N))
    a.free(); b.free(); simple.close()
    assert (za.view(np.uint32) == zb.view(np.uint32)).all(), "LDS-tiled kernel differs from the per-cell kernel"
    # the first rows of the full-width grid are reproducible by the oracle as an (N x 6) grid with the same origin
    orc.init(orclib.make_config(mesh_gen_mode=0, mesh_freq_filter=ff))
    rows = orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, 6, 1)
    assert_bit_equal(rows, za[:6], "oracle rows")
    cols = orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, 6, N, 1)
    assert_bit_equal(cols, za[:, :6], "oracle columns")
    assert np.isfinite(za).all()


def test_bench_step_full_size_equals_oracle(pkg, gpu, orc):
    """BASELINE's headline configuration, the exact calls bench.py times (gen_grid_minmax_dev with the fused min + apply_erosion_dev with
    TERRA_ERODE_MINZ_IS_MIN's sparse clamp): 16384^2, 8 octaves = 80 sine terms, 1000 droplets -- the WHOLE grid and the returned min against the
    oracle's heightmap_t::proc_gen sequence (src/heightmap.cpp:130-187) on the host's cores, bit for bit."""
    N, droplets = 16384, 1000
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_freq_filter=1))
    orc.init(orclib.make_config(mesh_gen_mode=0, mesh_freq_filter=1))
    a = gpu.alloc(N * N * 4)
    mn, mx = gpu.gen_grid_minmax_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    gpu.apply_erosion_dev(a.ptr, N, N, mn, droplets, pkg.ERODE_MINZ_IS_MIN)
    rep = gpu.erosion_report().as_dict()
    z = a.download(np.float32, (N, N)); a.free()
    ref = orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, 1)   # build_arrays + enable_glaciate + eval_index loop, OpenMP over rows
    rmn, rmx = ref.min(), ref.max()
    assert np.float32(mn) == rmn and np.float32(mx) == rmx, (mn, mx, rmn, rmx)
    orc.apply_erosion(ref, float(rmn), droplets)                          # serial droplet order
    diff = z.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} cells differ, first at {np.argwhere(diff)[:4].tolist()}"
    assert rep["droplets"] == droplets
    assert 600 < rep["sparse_probe_only"] <= 849, rep  # (the oracle's step counts: 849 of this map's 1000 droplets take no step -- under water at once, or an uphill first move that deposits nothing and ends)
    assert rep["sparse_droplets"] == droplets, rep  # the timed configuration goes through the sparse scheduler alone (lean traces; its one conflicting pair is a re-trace round)
    print("erosion report", rep)


@pytest.mark.parametrize("mode", [1, 2, 4])
def test_full_size_noise_modes_whole_grid_equals_oracle(pkg, gpu, orc, mode):
    """BASELINE config 2 (4096^2, 8 octaves) in the fBm modes: every cell against the oracle, plus the fused min / max."""
    N = 4096
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=mode, mesh_freq_filter=1))
    orc.init(orclib.make_config(mesh_gen_mode=mode, mesh_freq_filter=1))
    a = gpu.alloc(N * N * 4)
    mn, mx = gpu.gen_grid_minmax_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    z = a.download(np.float32, (N, N)); a.free()
    ref = orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, 1)
    diff = z.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"mode {mode}: {int(diff.sum())} cells differ, first at {np.argwhere(diff)[:4].tolist()}"
    assert np.float32(mn) == ref.min() and np.float32(mx) == ref.max()


@pytest.mark.parametrize("N,droplets", [(4096, 100000), (4096, 1000000), (16384, 200000)])
def test_dense_erosion_config3_equals_oracle(pkg, gpu, orc, N, droplets):
    """BASELINE config 3 at its real density (config_heightmap.txt asks for 10^6 droplets: ~0.7 s of the single-threaded oracle) and a sparser large map: every cell against the
    oracle's serial droplet order -- the regime with hundreds to 1500 scheduler rounds, multi-version look-ups, re-traces that resume from checkpoints"""
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0))
    orc.init(orclib.make_config(mesh_gen_mode=0))
    a = gpu.alloc(N * N * 4)
    mn, _ = gpu.gen_grid_minmax_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    gpu.apply_erosion_dev(a.ptr, N, N, mn, droplets, pkg.ERODE_MINZ_IS_MIN)
    rep = gpu.erosion_report().as_dict()
    z = a.download(np.float32, (N, N)); a.free()
    ref = orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, 1)
    st_o = orc.apply_erosion_stats(ref, float(ref.min()), droplets)
    diff = z.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} cells differ"
    assert rep["steps"] == st_o[0].steps and rep["rounds"] > 20 and rep["traces"] > droplets and rep["checkpoint_resumes"] > 0, rep


def test_full_size_row_strips_tile_the_grid(pkg, gpu):
    """16384^2 as 8 row strips (what 8 ranks of bench.py's strips workload evaluate) == the single-call grid, bit for bit; the strips' minima fold to the grid's"""
    N, W = 16384, 8
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_freq_filter=1))
    a, b = gpu.alloc(N * N * 4), gpu.alloc(N * N * 4)
    mn, mx = gpu.gen_grid_minmax_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    mns = []
    for r in range(W):
        r0, r1 = r * N // W, (r + 1) * N // W
        m, _ = gpu.gen_grid_rows_minmax_dev(b.ptr + r0 * N * 4, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, r0, r1 - r0, pkg.GEN_GLACIATE)
        mns.append(m)
    za, zb = a.download(np.float32, (N, N)), b.download(np.float32, (N, N))
    a.free(); b.free()
    assert (za.view(np.uint32) == zb.view(np.uint32)).all() and min(mns) == mn


def test_full_size_erosion_speculative_equals_serial_walk(pkg, gpu):
    """16384^2 + 1000 droplets: the multi-version fixed point must equal the single-lane serial walk bit for bit."""
    N = 16384
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_freq_filter=1))
    a, b = gpu.alloc(N * N * 4), gpu.alloc(N * N * 4)
    gpu.gen_grid_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    gpu.gen_grid_dev(b.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
    mn, mx = gpu.minmax_dev(a.ptr, N * N)
    gpu.apply_erosion_dev(a.ptr, N, N, mn, 1000, 0)
    rep = gpu.erosion_report().as_dict()
    gpu.apply_erosion_dev(b.ptr, N, N, mn, 1000, pkg.ERODE_SERIAL)
    za, zb = a.download(np.float32, (N, N)), b.download(np.float32, (N, N))
    a.free(); b.free()
    assert (za.view(np.uint32) == zb.view(np.uint32)).all()
    assert za.min() >= mn and rep["droplets"] == 1000 and rep["rounds"] >= 1
    print("erosion report", rep)


def test_full_size_noise_modes_match_oracle_subgrid(pkg, gpu, orc):
    """fBm modes are per-cell: any sub-rectangle of the 4096^2 grid equals the oracle evaluated on that rectangle's cells.
    (cell (x,y) depends on x*mdx+mx0 only, so the oracle is run on the same origin with a narrow width / height)."""
    N = 4096
    for mode in (1, 2, 4):
        st = gpu.init_scene(pkg.make_config(mesh_gen_mode=mode))
        orc.init(orclib.make_config(mesh_gen_mode=mode))
        a = gpu.alloc(N * N * 4)
        gpu.gen_grid_dev(a.ptr, -N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, N, pkg.GEN_GLACIATE)
        z = a.download(np.float32, (N, N)); a.free()
        w = 3 if mode == 4 else 8
        assert_bit_equal(orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, N, w, 1), z[:w], f"mode {mode} rows")
        assert_bit_equal(orc.gen_grid(-N / 2, -N / 2, st.DX_VAL, st.DY_VAL, w, N, 1), z[:, :w], f"mode {mode} cols")


def test_tiles_batch_64x64_properties(pkg, gpu, orc):
    """Config 4: 64x64 tiles of 128^2.  Shared edges: tile (tx,ty) column 128 is tile (tx+1,ty) column 0 evaluated from a different
    grid origin, so values agree only approximately (reference has the same property); exact checks: a sample of tiles vs the oracle,
    integer water bboxes inside the tile, sub-block ranges consistent with zvals."""
    st = gpu.init_scene(pkg.make_config(mesh_gen_mode=0))
    orc.init(orclib.make_config(mesh_gen_mode=0))
    tiles = [(tx, ty) for ty in range(-32, 32) for tx in range(-32, 32)]
    z, stats, nm, mnz = gpu.tiles_create_zvals(tiles, 0)
    assert z.shape == (4096, 130, 130) and np.isfinite(z).all()
    for i in (0, 777, 2080, 4095):
        zo, so = orc.tile_create_zvals(*tiles[i], 0)
        assert_bit_equal(zo, z[i]); assert bytes(so) == bytes(stats[i])
    zz = z[:, :129, :129]
    sub = zz.reshape(4096, 129 * 129)
    mz = np.array([s.mzmin for s in stats]), np.array([s.mzmax for s in stats])
    assert (mz[0] == sub.min(1)).all() and (mz[1] == sub.max(1)).all()
    assert (nm[..., 3] == 0).all() and (mnz > 0).all() and (mnz <= 1).all()


@pytest.mark.parametrize("block", [0, 1])
def test_random_configs(pkg, gpu, orc, block):
    pc.case_random_configs(pkg, gpu, orc, range(block * 7, block * 7 + 7), big=True)


def test_tile_erosion_large_batch_launch_order(pkg, gpu, orc):
    """more tiles than fit the chip at once: the erosion kernel hands tiles out longest-predicted-chain first (a permutation of the launch, not of
    the results) -- every tile still equals the oracle's, land and ocean tiles alike"""
    pc_, oc = pc.cfg_pair(pkg, mesh_gen_mode=0)
    gpu.init_scene(pc_); orc.init(oc)
    tiles = [(tx, ty) for ty in range(-13, 13) for tx in range(-12, 12)]  # 624 tiles
    iters = 110
    z, st, _, _ = gpu.tiles_create_zvals(tiles, iters)
    rng = np.random.default_rng(3)
    for i in rng.choice(len(tiles), 60, replace=False):
        zo, so = orc.tile_create_zvals(tiles[i][0], tiles[i][1], iters)
        assert_bit_equal(z[i], zo, f"tile {tiles[i]}")
        assert bytes(st[i]) == bytes(so)


def test_random_heightmap_textures(pkg, gpu, orc):
    pc.case_random_heightmap_textures(pkg, gpu, orc)


@pytest.mark.parametrize("ndev,big", [(2, False), (3, True)])
def test_multi_contexts_in_one_process(pkg, orc, ndev, big):
    """terra_multi_* on the HIP library: several contexts on device 0 (the test box has one GPU; on a node every context gets its own), each driven by its own host
    thread; the shadow edges travel between the contexts' buffers with the device-to-device copy the multi-GPU path uses"""
    pc.case_multi_contexts(pkg, None, orc, ndev, big)


@pytest.mark.parametrize("env", [{"TERRA_GRAPHS": "0"}, {"TERRA_ERO_CK": "1:16", "TERRA_ERO_NEAR": "4"}, {"TERRA_ERO_CK": "40:0", "TERRA_ERO_LEAD": "0"}, {"TERRA_ERO_BATCH": "1", "TERRA_ERO_LEAD": "1"},
                                 {"TERRA_TILE_EROSION": "window"}, {"TERRA_SIMPLE_KERNELS": "1"}, {"TERRA_SG_ROWGROUP": "2"}, {"TERRA_ERO_SPARSE": "1", "TERRA_ERO_SPARSE_RETRACES": "12"}, {"TERRA_ERO_FUSE": "0"}, {"TERRA_ERO_FUSE": "7"}, {"TERRA_VOXELS_COLS": "0"}, {"TERRA_AO_BANDS": "0"}, {"TERRA_ERO_MEM_BUDGET": "200000000"}, {"TERRA_SG_KC": "45"}, {"TERRA_SG_KC": "20"}, {"TERRA_SG_KC_TILES": "45"}])
def test_experiment_knobs_never_change_a_result(pkg, orc, monkeypatch, env):
    """the environment knobs of DESIGN.md section 5 choose schedules, launch forms and cross-check kernels, never values: a whole-map erosion with re-traces, an eroded tile
    batch and its mesh shadows under each of them, bit for bit against the oracle (the knobs are read when a context is created)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = pkg.Terra(0)
    try:
        pc.case_erosion_vs_oracle(pkg, t, orc, 512, 4000)
        if "TERRA_SG_KC" in env or "TERRA_SG_ROWGROUP" in env:  # the heightmap's sine kernel: ragged grid, a late first term (odd chunk lengths), the fused min / max
            pc.case_grid_vs_oracle(pkg, t, orc, 0, 1030)
            pc.case_grid_vs_oracle(pkg, t, orc, 0, 300, 50)
            pc.case_gen_grid_minmax(pkg, t, orc, 0, 700)
        pc_, oc = pc.cfg_pair(pkg, mesh_gen_mode=0)
        t.init_scene(pc_); orc.init(oc)
        tiles = [(tx, ty) for ty in range(-28, -25) for tx in range(-29, -26)]
        z, st, nm, mnz = t.tiles_create_zvals(tiles, 150)
        zo = np.stack([orc.tile_create_zvals(tx, ty, 150)[0] for tx, ty in tiles])
        assert_bit_equal(z, zo, f"eroded tiles under {env}")
        t.release_scratch()  # every grow-only buffer back to the device: the next calls allocate afresh
        sm = t.tiles_mesh_shadows(tiles, z, (0.6, 0.5, 0.4))
        so = orc.tiles_mesh_shadows(tiles, zo, (0.6, 0.5, 0.4))
        assert np.array_equal(np.asarray(sm), np.asarray(so)), f"mesh shadows under {env}"
        pc.case_erosion_vs_oracle(pkg, t, orc, 384, 1500)
    finally:
        t.close()


def _release_then_reuse(t, what, call, small, large, check):
    """call(small), release_scratch(), call(small) again: the same bits, and the oracle's (check); then, after another release, call(large): a size that survived its
    pointer would hand out a null or too small buffer"""
    first = call(small)
    t.release_scratch()
    again = call(small)
    for a, b in zip(first, again):
        assert bytes(a) == bytes(b), f"{what}: the call after release_scratch differs from the one before"  # (the arrays' raw bytes)
    check(small, again)
    t.release_scratch()
    check(large, call(large))


def test_release_scratch_then_reuse(pkg, gpu, orc):
    """terra_release_scratch hands back every grow-only buffer of the context, the backend's six included, and each grows again on demand: per backend buffer the
    smallest call that allocates it, before and after a release, and a larger one after a release.
    h3_tab: a TERRA_GEN_FAST sine grid.  tile_map + tile_acc: a dense batch at S = 16 with stats and normals (the one-launch tile grid, k_tile_post_sized).  tile_order:
    more than 512 tiles with n*iters >= 65536 (the erosion launch order).  tile_pad: option "tile_erosion" = "window".  vox_p: a voxel sine field whose depth is no
    multiple of 4 (the P-array kernel)."""
    import tile_size_model as tsm
    t, S = gpu, 16
    # ---- h3_tab: within the tolerance of the mode (parity_cases.case_fast_mode)
    pc_, oc = pc.cfg_pair(pkg, mesh_gen_mode=0)
    st = t.init_scene(pc_); orc.init(oc)
    tol = pc.FUSED_REL_TOL*float(st.zmax_est)

    def fast_grid(dims):
        return (t.gen_grid(-0.37*dims[0], 11.0 - dims[1], st.DX_VAL, st.DY_VAL, dims[0], dims[1], pkg.GEN_GLACIATE | pkg.GEN_FAST),)

    def check_grid(dims, out):
        exact = orc.gen_grid(-0.37*dims[0], 11.0 - dims[1], st.DX_VAL, st.DY_VAL, dims[0], dims[1], 1)
        d = float(np.abs(out[0].astype(np.float64) - exact).max())
        assert d <= tol, (dims, d, tol)
    _release_then_reuse(t, "h3_tab", fast_grid, (300, 300), (520, 300), check_grid)
    # ---- vox_p: bit for bit (parity_cases.case_voxels_vs_oracle)
    vox_args = lambda dims: (*dims, pc.VOX["lo"], pc.VOX["vsz"], pc.VOX["off"], 0.8, 1.3, 7, 9, 0, -0.02, 0)  # noqa: E731
    _release_then_reuse(t, "vox_p", lambda dims: (t.voxel_fill(*vox_args(dims)),), (8, 8, 6), (16, 8, 6),
                        lambda dims, out: assert_bit_equal(orc.voxel_fill(*vox_args(dims)), out[0], f"voxels {dims}"))
    # ---- the tile passes at S = 16, against the size-general model of the reference's tile (tests/tile_size_model.py)
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=S)); orc.init(orclib.make_config(mesh_gen_mode=0, mesh_xy=S))
    assert t.tile_size == S
    block = lambda w, h: [(x, y) for y in range(-(h // 2), h - h // 2) for x in range(-(w // 2), w - w // 2)]  # noqa: E731

    def tiles_call(iters):
        def call(tiles):
            z, stt, nm, mnz = t.tiles_create_zvals(tiles, iters)
            return z, bytes(stt), nm, mnz
        return call

    def tiles_check(iters, sample):
        def check(tiles, out):
            z, stt, nm, mnz = out
            for i in sample(len(tiles)):
                tx, ty = tiles[i]
                zm = tsm.tile_zvals(orc, S, tx, ty, iters)
                assert_bit_equal(zm, z[i], f"zvals tile {tx},{ty} of {len(tiles)}, {iters} droplets")
                nb = len(stt)//len(tiles)
                assert stt[i*nb:(i + 1)*nb] == tsm.stats_bytes(tsm.tile_stats(orc, S, tx, ty, zm)), f"stats tile {tx},{ty}"
                nmm, mm = tsm.tile_normals(orc, S, zm)
                assert (nm[i] == nmm).all() and np.float32(mnz[i]).view(np.uint32) == np.float32(mm).view(np.uint32), f"normals tile {tx},{ty}"
        return check
    every = lambda n: range(n)  # noqa: E731
    some = lambda n: (0, 1, n//3, n//2 + 7, n - 2, n - 1)  # noqa: E731
    _release_then_reuse(t, "tile_map + tile_acc", tiles_call(0), block(3, 3), block(5, 5), tiles_check(0, every))
    _release_then_reuse(t, "tile_order", tiles_call(128), block(26, 20), block(30, 20), tiles_check(128, some))  # 520 and 600 tiles: n > 512, n*iters >= 65536
    t.set_option("tile_erosion", "window")
    try:
        _release_then_reuse(t, "tile_pad", tiles_call(50), block(2, 1), block(3, 2), tiles_check(50, every))
    finally:
        t.set_option("tile_erosion", "lds")


def test_overlapped_download_equals_synchronous(pkg, gpu, orc):
    pc.case_big_transfers(pkg, gpu, orc)


def test_host_wait_on_an_event_while_its_context_captures_a_graph(pkg, orc):
    """terra_event_synchronize from another thread while the recording context captures erosion rounds into hipGraphs (first use of every new grid shape / droplet count):
    the runtime refuses a host wait on an event "last recorded in a capturing stream" and poisons the capture, so terra_event_record goes through a side stream that never
    captures.  One thread records + erodes with a new graph key every time, the other waits on every event; nothing fails, every grid equals the oracle."""
    import threading
    a, b = pkg.Terra(0), pkg.Terra(0)
    try:
        pc_, oc = pc.cfg_pair(pkg, mesh_gen_mode=0)
        st = a.init_scene(pc_); b.init_scene(pc_); orc.init(oc)
        n, rounds = 384, 12
        bufs = [a.alloc(n * n * 4) for _ in range(rounds)]
        mm = a.alloc(8)
        ev = a.event_create()
        recorded = [threading.Event() for _ in range(rounds)]
        errs = []

        def producer():
            try:
                for i in range(rounds):
                    a.gen_grid_minmax_async_dev(bufs[i].ptr, -n / 2, -n / 2, st.DX_VAL, st.DY_VAL, n, n, mm.ptr, pkg.GEN_GLACIATE)
                    a.event_record(ev); recorded[i].set()
                    a.apply_erosion_devmin_dev(bufs[i].ptr, n, n, mm.ptr, 50 + 37 * i, 0)  # a droplet count never seen before: its rounds are captured now
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
            finally:
                for r in recorded:
                    r.set()

        def waiter():
            try:
                for i in range(rounds):
                    recorded[i].wait()
                    for _ in range(200):
                        b.event_synchronize(ev)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=producer), threading.Thread(target=waiter)]
        [x.start() for x in th]; [x.join() for x in th]
        assert not errs, errs
        a.synchronize()
        ref0 = orc.gen_grid(-n / 2, -n / 2, st.DX_VAL, st.DY_VAL, n, n, 1)
        for i in (0, 5, rounds - 1):
            ref = ref0.copy(); orc.apply_erosion(ref, float(ref0.min()), 50 + 37 * i)
            assert_bit_equal(ref, bufs[i].download(np.float32, (n, n)), f"grid {i}")
        a.event_destroy(ev)
    finally:
        a.close(); b.close()


def test_streamed_pipeline_device_min_and_events(pkg, orc):
    """bench.py's streamed schedule: a producer context's noise kernels back to back, {min, max} left in HBM, three consumer contexts eroding as the events fire"""
    pc.case_streamed_pipeline(pkg, lambda: pkg.Terra(0), orc, N=2048, maps=9, P=3, droplets=(1000, 0, 6000))
