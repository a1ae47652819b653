"""Cases of scenery placement (terra_tiles_place_scenery[_dev]) shared by test_scenery_place_emul.py (the host emulator) and test_gpu_scenery_place.py (HIP on
the MI355X).  Every record is compared byte for byte with tests/scenery_place_model.py, order, counts and kind counts included.

The model's result of a case is computed once per process (MODEL) together with its tally of kinds and drop reasons, which
test_scenery_place_emul.py::test_cases_are_not_vacuous checks."""
import numpy as np

import orclib
import scenery_place_model as spm
import tree_place_cases as tpc
import tree_place_model as tpm

ERR_ARG, ERR_STATE = -1, -3
TILES, SHORE, TILES9 = tpc.TILES, tpc.SHORE, tpc.TILES9
REC = 72  # bytes of a record
NK = len(spm.KINDS)


class Case:
    def __init__(self, name, S=128, mode=0, tiles=TILES, tp=None, xoff2=0, yoff2=0, capacity=256, skip=None, vegetation=1.0, water_h_off=0.0, use_voxel_rocks=2,
                 ocean_wave_height=0.0, min_objs=40):
        self.name, self.S, self.mode, self.tiles, self.xoff2, self.yoff2, self.capacity = name, S, mode, tiles, xoff2, yoff2, capacity
        self.tp = dict(tp or {})  # tree_mode 1, the reference's default
        self.skip, self.vegetation, self.water_h_off, self.use_voxel_rocks, self.ocean_wave_height = skip, vegetation, water_h_off, use_voxel_rocks, ocean_wave_height
        self.min_objs = min_objs  # what the case places at the least, all tiles together


def cases():
    return [
        Case("defaults_s128"),
        Case("shore_mode3", tp=dict(tree_mode=3), tiles=SHORE, water_h_off=0.1),  # water plants, underwater leafy plants, low stumps and mushrooms, palm and pine logs
        Case("shore_waves", tp=dict(tree_mode=3), tiles=SHORE[1:4], water_h_off=0.1, ocean_wave_height=0.3),  # get_min_water_plane_z below the water plane
        Case("dwarp_s64", S=64, mode=4, min_objs=10),
        Case("odd_s20", S=20, tiles=TILES9, min_objs=3),        # 400 cells: not a multiple of the kernel's 256
        Case("defaults_s256", S=256, capacity=700, tiles=TILES[:3]),
        Case("offsets_rgi", xoff2=37, yoff2=-21, tp=dict(rand_gen_index=5)),
        Case("rand_zone", tp=dict(tree_mode=3, tree_type_rand_zone=0.02), tiles=SHORE[:4], water_h_off=0.1),
        Case("voxel_rocks_1", use_voxel_rocks=1),
        Case("voxel_rocks_2_no_vegetation", use_voxel_rocks=2, vegetation=0.0, min_objs=20),  # voxel rocks, and no plant, log or stump
        Case("voxel_rocks_0", use_voxel_rocks=0),
        Case("skipped_tile", skip=[0, 1, 0, 0]),
        Case("capacity_small", capacity=25),
        Case("tree_scale_8_s64", S=64, tp=dict(tree_scale=8.0), capacity=450),  # smod 1511: a tenth of the cells, the ring fills more than once in a tile
        Case("tree_scale_8_s20", S=20, tp=dict(tree_scale=8.0), tiles=TILES9, capacity=320),  # smod clamped to 200: three quarters of the cells
        Case("tree_scale_16_s64", S=64, tp=dict(tree_scale=16.0), tiles=TILES[:3], capacity=800),  # smod 800: a fifth of the cells, the kernel's ring of 512 wraps
    ]


def _oracle_config(case):
    ocfg = orclib.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S)
    ocfg.water_h_off, ocfg.ocean_wave_height = case.water_h_off, case.ocean_wave_height
    return ocfg


MODEL = {}


def model(orc, case):
    """(records per tile, tally) of the case from the model, computed once"""
    if case.name not in MODEL:
        ocfg = _oracle_config(case)
        orc.init(ocfg)
        sc = tpm.Scene(orc, ocfg, tpm.TreeParams(**case.tp), vegetation=case.vegetation)
        tally = spm.new_tally()
        want = spm.place(sc, case.tiles, case.xoff2, case.yoff2, case.skip, case.use_voxel_rocks, case.ocean_wave_height, tally)
        MODEL[case.name] = (want, tally)
    return MODEL[case.name]


def configure(pkg, t, case):
    """the scene and the settings of a case on the library's side"""
    cfg = pkg.make_config(mesh_gen_mode=case.mode, mesh_xy=case.S)
    cfg.water_h_off, cfg.ocean_wave_height = case.water_h_off, case.ocean_wave_height
    t.init_scene(cfg)
    t.set_landscape(pkg.make_landscape(vegetation=case.vegetation))
    t.set_tree_params(pkg.make_tree_params(**case.tp))
    t.set_scenery_params(pkg.make_scenery_params(case.use_voxel_rocks))


def compare(what, objs, counts, kinds, want, capacity):
    """objs [n, capacity] + counts [n] + kinds [n, 9] against the model's per-tile lists"""
    assert [int(c) for c in counts] == [len(w) for w in want], f"{what}: counts {counts.tolist()} != {[len(w) for w in want]}"
    if kinds is not None:
        assert kinds.tolist() == spm.kind_counts(want).tolist(), f"{what}: kind counts {kinds.tolist()} != {spm.kind_counts(want).tolist()}"
    for t, w in enumerate(want):
        m = min(len(w), capacity)
        if m == 0:
            continue
        exp = np.array(w[:m], spm.PLACE_DTYPE)
        got = np.ascontiguousarray(objs[t, :m])
        if got.tobytes() != exp.tobytes():
            for k in range(m):
                if got[k].tobytes() != exp[k].tobytes():
                    raise AssertionError(f"{what}: tile {t} object {k} of {len(w)}: got {got[k]} != {exp[k]}")


def run_case(pkg, t, orc, case, dev=False, kind_counts=True):
    want, _ = model(orc, case)
    configure(pkg, t, case)
    n, cap = len(case.tiles), case.capacity
    if not dev:
        objs, counts, kinds = t.tiles_place_scenery(case.tiles, cap, case.xoff2, case.yoff2, case.skip, kind_counts)
    else:
        bufs = dict(ob=t.alloc(n * cap * REC), cn=t.alloc(n * 4))
        if kind_counts:
            bufs["kc"] = t.alloc(n * NK * 4)
        if case.skip is not None:
            bufs["sk"] = t.alloc(n).upload(np.asarray(case.skip, np.uint8))
        try:
            bufs["ob"].upload(np.zeros(n * cap * REC, np.uint8))
            ptr = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
            t.tiles_place_scenery_dev(case.tiles, cap, bufs["ob"].ptr, bufs["cn"].ptr, case.xoff2, case.yoff2, ptr("sk"), ptr("kc"))
            objs = bufs["ob"].download(np.uint8, (n * cap * REC,)).view(pkg.SCENERY_PLACE_DTYPE).reshape(n, cap)
            counts = bufs["cn"].download(np.uint32, (n,))
            kinds = bufs["kc"].download(np.uint32, (n, NK)) if kind_counts else None
        finally:
            for b in bufs.values():
                b.free()
    compare(case.name + (" (dev)" if dev else ""), objs, counts, kinds, want, cap)
    # records past the count are not written
    for i in range(n):
        assert not objs[i, min(int(counts[i]), cap):].tobytes().strip(b"\0"), f"{case.name}: tile {i}: records past the count were written"
    assert sum(len(w) for w in want) >= case.min_objs, (case.name, sum(len(w) for w in want))
    return want
