"""Cases of the tile clouds (terra_tiles_update_clouds[_dev], terra_tiles_cloud_view[_dev]) and what runs them against tests/cloud_model.py, on the emulator and on
the GPU alike.  An update case runs its frames one call at a time; after every call the state, the records up to count and the total are compared byte for byte.

A case's wind is given in tiles per frame: 0.01*fticks*|wind| is a tenth to a half of a tile, so that clouds migrate within a few frames.  A hook changes the
managers between two frames the way an engine may: a tile that enters the batch anew (a fresh manager), or a list that the wind has emptied."""
import ctypes as C

import numpy as np

import cloud_model as cm
import orclib
import terrain_view_cases as tc
import view_model as vw

f32 = np.float32
ERR_ARG, ERR_STATE = -1, -3
GRID3 = [(x, y) for y in range(-1, 2) for x in range(-1, 2)]
GRID5 = [(x, y) for y in range(-2, 3) for x in range(-2, 3)]
ROW2, ROW3 = [(0, 0), (1, 0)], [(0, 0), (1, 0), (2, 0)]


def _shuffled(tiles, seed, drop=()):
    t = [xy for xy in tiles if xy not in drop]
    np.random.default_rng(seed).shuffle(t)
    return [tuple(int(v) for v in xy) for xy in t]


class Case:
    def __init__(self, name, S=16, tiles=GRID3, params=None, wind=(0.3, 0.15, 0.0), fticks=1.0, animate=1, frames=3, capacity=32, hooks=None, check=None):
        self.name, self.S, self.tiles, self.params = name, S, [tuple(t) for t in tiles], dict(params or {})
        self.wind, self.fticks, self.animate, self.frames, self.capacity = wind, fticks, animate, frames, capacity
        self.hooks, self.check = dict(hooks or {}), check or (lambda t: True)


def _fresh(*which):
    """the tiles at these batch indices enter the batch anew"""
    def f(sc, tiles, mgrs):
        for k in which:
            mgrs[k] = cm.Manager()
    return f


def _emptied(*which):
    """the lists of these tiles (all of them without arguments) are empty, as after the wind has carried every cloud off"""
    def f(sc, tiles, mgrs):
        for k in (which or range(len(mgrs))):
            mgrs[k].clouds = []
            if mgrs[k].num_clouds == 0:
                mgrs[k].num_clouds = 3
    return f


def _at_edge(k, side):
    """the clouds of tile k stand close to the x edge they are about to cross (side 1: x2, -1: x1), the first and the last two closest"""
    def f(sc, tiles, mgrs):
        m = mgrs[k]
        w = f32(m.range[0][1] - m.range[0][0])
        for i, c in enumerate(m.clouds):
            near = i == 0 or i >= len(m.clouds) - 2
            off = f32(w * f32(0.02 if near else 0.6))
            c.pos[0] = f32(m.range[0][1] - off) if side > 0 else f32(m.range[0][0] + off)
    return f


def _both(*fs):
    def f(sc, tiles, mgrs):
        for g in fs:
            g(sc, tiles, mgrs)
    return f


def update_cases():
    D8 = dict(clouds_per_tile=8.0)
    return [
        Case("gen_default", frames=1, check=lambda t: t["gen"] == 9 and t["gen_clouds"] > 0 and t["early_not_generated"] == 9),
        Case("gen_single_tile", tiles=[(3, -2)], frames=2, check=lambda t: t["gen"] == 1 and t["gen_already"] == 1),
        Case("gen_s128", S=128, tiles=ROW2, frames=2, check=lambda t: t["gen"] == 2 and t["gen_clouds"] > 0),
        Case("density_zero", params=dict(clouds_per_tile=0.0), frames=2, capacity=0, check=lambda t: t["gen_no_draw"] == 9 and t["gen_clouds"] == 0 and t["empty_nothing"] == 9),
        Case("density_8", S=128, tiles=ROW2, params=D8, frames=2, check=lambda t: t["gen_clouds"] >= 8),
        Case("animate_0", animate=0, frames=3, check=lambda t: t["not_animated"] == 27 and t["steps"] == 0),
        Case("zero_wind", wind=(0.0, 0.0, 0.0), frames=3, check=lambda t: t["early_zero_wind"] == 18 and t["steps"] == 0),
        Case("wind_z_alone", wind=(0.0, 0.0, 0.3), frames=3, check=lambda t: t["steps"] == 18 and t["zero_move_steps"] == 18 and t["stay"] > 0 and t["stay"] == t["moved"]),
        Case("stay_only", params=D8, wind=(0.002, 0.001, 0.0), frames=3, check=lambda t: t["stay_only_tiles"] >= 9 and t["stay"] == t["moved"] and t["moved"] > 0),
        Case("to_later_moved_twice", tiles=ROW2, params=D8, wind=(0.4, 0.0, 0.0), frames=4, hooks={1: _at_edge(0, 1)},
             check=lambda t: t["to_later"] > 0 and t["moved_twice"] > 0 and t["to_earlier"] == 0),
        Case("to_earlier_moved_once", tiles=ROW2[::-1], params=D8, wind=(0.4, 0.0, 0.0), frames=4, hooks={1: _at_edge(1, 1)},
             check=lambda t: t["to_earlier"] > 0 and t["moved_twice"] == 0 and t["to_later"] == 0),
        Case("row_crossed_in_one_frame", tiles=ROW3, params=D8, wind=(0.5, 0.0, 0.0), frames=4, hooks={1: _at_edge(0, 1)}, check=lambda t: t["left_again"] > 0),
        Case("diagonal", params=D8, wind=(0.4, 0.4, 0.0), frames=3, check=lambda t: t["diagonal"] > 0 and t["to_later"] > 0 and t["to_earlier"] == 0),
        Case("diagonal_against_order", params=D8, wind=(-0.4, -0.35, 0.0), frames=3, check=lambda t: t["diagonal"] > 0 and t["to_earlier"] > 0),
        Case("drop_at_hole", tiles=_shuffled(GRID3, 5, drop=[(0, 0)]), params=D8, wind=(0.3, -0.2, 0.0), frames=3, check=lambda t: t["drop_hole"] > 0 and t["to_later"] + t["to_earlier"] > 0),
        Case("drop_at_ungenerated", tiles=ROW2, params=D8, wind=(0.4, 0.0, 0.0), frames=3, hooks={1: _both(_at_edge(0, 1), _fresh(1))},
             check=lambda t: t["drop_ungenerated"] > 0 and t["drop_then_generated"] > 0),
        Case("first_and_chain_leave", tiles=ROW2, params=D8, wind=(0.3, 0.0, 0.0), frames=3, hooks={1: _at_edge(0, 1)}, check=lambda t: t["first_left"] > 0 and t["swapped_in_left"] > 0),
        Case("repopulate_edge", params=D8, wind=(0.3, 0.0, 0.0), frames=3, hooks={1: _emptied()}, check=lambda t: t["repop_edge"] == 3 and t["no_repop_inner"] >= 6),
        Case("zero_wind_component", params=D8, wind=(0.0, 0.3, 0.0), frames=3, hooks={1: _emptied()}, check=lambda t: t["repop_edge_zero_component"] == 3 and t["no_repop_inner"] >= 6),
        Case("fed_before_turn", tiles=ROW3, params=D8, wind=(0.3, 0.0, 0.0), frames=3, hooks={1: _both(_at_edge(0, 1), _emptied(1))},
             check=lambda t: t["fed_before_turn"] > 0 and t["repop_edge"] == 0),
        Case("fed_after_repopulation", tiles=ROW2[::-1], params=D8, wind=(0.3, 0.1, 0.0), frames=3, hooks={1: _both(_at_edge(1, 1), _emptied(0))},
             check=lambda t: t["fed_after_repop"] > 0 and t["repop_edge"] > 0),
        Case("move_dist_redraw", params=D8, wind=(0.5, 0.0, 0.0), frames=6, check=lambda t: t["redraw"] >= 9),
        Case("overflow", tiles=ROW3, params=D8, wind=(0.4, 0.0, 0.0), frames=4, capacity=4, hooks={1: _at_edge(0, 1)},
             check=lambda t: t["overflow_gen"] > 0 and t["overflow_imm"] > 0 and t["overflow_sticky"] > 0),
        Case("holes_shuffled_s128", S=128, tiles=_shuffled(GRID5, 11, drop=[(0, 0), (1, -1), (-2, 2)]), params=dict(clouds_per_tile=3.0), wind=(-0.25, 0.3, 0.0), frames=5,
             check=lambda t: t["to_later"] > 0 and t["to_earlier"] > 0 and t["drop_hole"] > 0),
        Case("long_run", tiles=_shuffled(GRID5, 7), wind=(0.25, 0.12, 0.0), frames=200, check=lambda t: t["redraw"] > 0 and t["repop_edge"] > 0 and t["to_later"] > 0 and t["to_earlier"] > 0),
    ]


def wind_of(sc, case):
    """the wind that moves a cloud by case.wind tiles a frame at wscale 1 (z is taken as given)"""
    w = f32(sc.get_xval(sc.S) - sc.get_xval(0))
    k = f32(w / f32(0.01 * float(case.fticks)))
    return [f32(f32(case.wind[0]) * k), f32(f32(case.wind[1]) * k), f32(case.wind[2])]


MODEL = {}


def scene_of(orc, case):
    ocfg = orclib.make_config(mesh_gen_mode=0, mesh_xy=case.S)
    orc.init(ocfg)
    return cm.Scene(orc, ocfg, cm.Params(**case.params), case.capacity)


def model(orc, case):
    """(scene, step, frames, tally): frames[k] = (state_in, clouds_in or None where frame k continues from frame k - 1, state, clouds, total)"""
    if case.name not in MODEL:
        sc = scene_of(orc, case)
        step = cm.Step(wind_of(sc, case), case.fticks, case.animate)
        mgrs = [cm.Manager() for _ in case.tiles]
        tally = cm.new_tally()
        frames = []
        for k in range(case.frames):
            s_in = c_in = None
            if k in case.hooks:
                case.hooks[k](sc, case.tiles, mgrs)
                s_in, c_in = cm.pack(sc, mgrs)
            total = cm.update(sc, step, case.tiles, mgrs, tally)
            state, clouds = cm.pack(sc, mgrs)
            frames.append((s_in, c_in, state, clouds, total))
        MODEL[case.name] = (sc, step, frames, tally, mgrs)
    return MODEL[case.name][:4]


def lib_step(pkg, step):
    return pkg.make_cloud_step([float(w) for w in step.wind], float(step.fticks), step.animate)


def configure(pkg, t, case):
    t.init_scene(pkg.make_config(mesh_gen_mode=0, mesh_xy=case.S))
    p = cm.Params(**case.params)
    t.set_cloud_params(pkg.make_cloud_params(float(p.clouds_per_tile), float(p.cloud_height_offset), p.rgen_seed))


def compare_update(what, state, clouds, total, w_state, w_clouds, w_total):
    assert state.dtype.itemsize == 88 and clouds.dtype.itemsize == 32
    for t in range(len(state)):
        if state[t].tobytes() != w_state[t].tobytes():
            raise AssertionError(f"{what}: state of tile {t}: {state[t]} != {w_state[t]}")
        k = int(w_state[t]["count"])
        if clouds[t, :k].tobytes() != w_clouds[t, :k].tobytes():
            bad = next(i for i in range(k) if clouds[t, i].tobytes() != w_clouds[t, i].tobytes())
            raise AssertionError(f"{what}: record {bad} of tile {t}: {clouds[t, bad]} != {w_clouds[t, bad]}")
    assert int(total) == int(w_total), f"{what}: total {int(total)} != {int(w_total)}"


def run_update_case(pkg, t, orc, case, dev=False):
    sc, step, frames, tally = model(orc, case)
    assert case.check(tally), (case.name, {k: x for k, x in tally.items() if x})
    configure(pkg, t, case)
    n, cap = len(case.tiles), case.capacity
    ls = lib_step(pkg, step)
    state = np.zeros(n, pkg.CLOUD_TILE_DTYPE)  # (the records start as garbage: nothing behind a count is read)
    clouds = np.full(n * cap * 32, 0x77, np.uint8).view(pkg.CLOUD_DTYPE).reshape(n, cap) if cap else np.zeros((n, 0), pkg.CLOUD_DTYPE)
    bufs = {}
    if dev:
        bufs = dict(st=t.alloc(n * 88), cl=t.alloc(max(n * cap * 32, 4)), to=t.alloc(4))
        bufs["st"].upload(state.view(np.uint8))
        if cap:
            bufs["cl"].upload(clouds.view(np.uint8))
    try:
        for k, (s_in, c_in, w_state, w_clouds, w_total) in enumerate(frames):
            if s_in is not None:  # the hook's state: what an engine would hand over
                state, clouds = s_in.copy().view(pkg.CLOUD_TILE_DTYPE), c_in.copy().view(pkg.CLOUD_DTYPE).reshape(n, cap)
                if dev:
                    bufs["st"].upload(state.view(np.uint8))
                    if cap:
                        bufs["cl"].upload(clouds.view(np.uint8))
            if not dev:
                total = t.tiles_update_clouds(case.tiles, ls, state, clouds)
            else:
                bufs["to"].upload(np.full(1, 0xABCDEF01, np.uint32))
                t.tiles_update_clouds_dev(case.tiles, ls, bufs["st"].ptr, bufs["cl"].ptr if cap else None, cap, bufs["to"].ptr)
                state = bufs["st"].download(np.uint8, (n * 88,)).copy().view(pkg.CLOUD_TILE_DTYPE)
                clouds = bufs["cl"].download(np.uint8, (n * cap * 32,)).copy().view(pkg.CLOUD_DTYPE).reshape(n, cap) if cap else clouds
                total = bufs["to"].download(np.uint32, (1,))[0]
            compare_update(f"{case.name}{' (dev)' if dev else ''}, frame {k}", state, clouds, total, w_state, w_clouds, w_total)
    finally:
        for b in bufs.values():
            b.free()


# ---- the view

ALONG = dict(dir=tc._unit(1.0, 0.4, 0.15), up=(0.0, 0.0, 1.0))


class ViewCase:
    def __init__(self, name, S=16, tiles=GRID5, params=None, frames=3, wind=(0.3, 0.15, 0.0), cam=(0.0, 0.0, 0.0), cam_dz=0.0, look=ALONG, angle=0.7, aspect=1.4, far=400.0, valid=1,
                 xlate=(0.0, 0.0, 0.0), max_dist=300.0, wpz=None, written=None, check=None):
        self.name, self.S, self.tiles, self.params, self.frames, self.wind = name, S, [tuple(t) for t in tiles], dict(params or {}), frames, wind
        self.cam, self.cam_dz, self.look, self.angle, self.aspect, self.far, self.valid = cam, cam_dz, look, angle, aspect, far, valid
        self.xlate, self.max_dist, self.wpz, self.written, self.check = xlate, max_dist, wpz, written, check or (lambda t: True)
        self.fticks, self.animate, self.capacity, self.hooks = 1.0, 1, 32, {}


def _tie_records(sc, tiles, mgrs):
    """hand-written records: the same position in different tiles and slots (equal dist_sq), among others"""
    for m in mgrs:
        m.clouds = m.clouds[:2]
    z = f32(mgrs[0].range[2][0] + f32(5.0))
    for t in (4, 1, 2):
        for _ in range(2):
            mgrs[t].clouds.append(cm.Cloud(1.0, [f32(2.0), f32(1.0), z], [f32(3.0), f32(4.0), f32(2.0)]))
    mgrs[5].clouds.append(cm.Cloud(1.0, [f32(2.0), f32(-1.0), z], [f32(3.0), f32(4.0), f32(2.0)]))  # (mirrored in y about a camera at y = 0: the same sum)


def view_cases():
    D3 = dict(clouds_per_tile=3.0)
    LOW = dict(clouds_per_tile=12.0, cloud_height_offset=-0.6)  # (the high ground of the default scene lies around tile (-6, 3))
    return [
        ViewCase("offset_0_from_below", params=D3, check=lambda t: t["listed"] > 0 and t["vfc"] > 0 and t["below_zmin"] > 0 and t["alpha_one_high"] > 0 and t["alpha_one_near"] > 0 and t["ties"] == 0),
        ViewCase("offset_low", tiles=[(x - 6, y + 3) for x, y in GRID5], params=LOW, cam=(-44.0, 28.0, 0.0), cam_dz=-3.0, angle=1.2, wpz="raised",
                 check=lambda t: t["below_mesh"] > 0 and t["alpha_frac"] > 0 and t["below_water"] > 0 and t["listed"] > 0 and t["ties"] == 0),
        ViewCase("xlate", params=D3, xlate=(3.5, -2.25, 0.75), check=lambda t: t["listed"] > 0 and t["vfc"] > 0 and t["ties"] == 0),
        ViewCase("beyond_max_dist", params=D3, max_dist=15.0, angle=1.2, check=lambda t: t["too_distant"] > 0 and t["drawn"] > 0 and t["ties"] == 0),
        ViewCase("camera_among_clouds", params=D3, cam_dz="clouds", angle=1.2, check=lambda t: t["listed"] > 0 and t["vfc"] > 0 and t["ties"] == 0),
        ViewCase("view_invalid_s128", S=128, tiles=_shuffled(GRID5, 3, drop=[(1, 1)]), params=D3, valid=0, check=lambda t: t["vfc"] == 0 and t["listed"] > 0 and t["ties"] == 0),
        ViewCase("ties", tiles=GRID3, params=D3, frames=1, cam=(0.0, 0.0, 0.0), valid=0, written=_tie_records, check=lambda t: t["ties"] >= 6),
    ]


def view_model(orc, case):
    """(scene, view, args, stats, state, clouds, (stage, list), tally), computed once"""
    key = "v:" + case.name
    if key not in MODEL:
        model(orc, case)
        sc, step, frames, _, mgrs = MODEL[case.name]
        if case.written:
            case.written(sc, case.tiles, mgrs)
        if case.wpz == "raised":  # the water plane among the clouds' bottoms
            sc.water_plane_z = f32(np.percentile([float(c.pos[2] - c.size[2]) for m in mgrs for c in m.clouds], 4))
        zc = float(mgrs[0].range[2][0])
        cam_z = zc + 4.0 if case.cam_dz == "clouds" else float(sc.zmax) * 0.5 + case.cam_dz
        v = vw.make_view((case.cam[0], case.cam[1], cam_z), case.look["dir"], case.look["up"], case.angle, case.aspect, 0.05, case.far)
        v.valid = case.valid
        a = cm.ViewArgs(vw.behind_sphere_mult(case.angle, case.aspect), case.xlate, case.max_dist)
        n = len(case.tiles)
        stats = (orclib.TileStats * n)()
        for t in range(n):  # every fourth tile's mesh lies above its clouds; every other one's mzmax asks for the exact height
            stats[t].mzmin = 1000.0 if t % 4 == 3 else -100.0
            stats[t].mzmax = 1000.0 if t % 4 == 3 else (100.0 if t % 2 == 0 else -50.0)
        state, clouds = cm.pack(sc, mgrs)
        tally = cm.new_tally()
        res = cm.view(sc, v, a, case.tiles, stats, mgrs, tally)
        MODEL[key] = (sc, v, a, stats, state, clouds, res, tally)
    return MODEL[key]


def lib_view_args(pkg, a):
    return pkg.make_cloud_view_args(float(a.behind_sphere_mult), [float(x) for x in a.xlate], float(a.max_dist))


def compare_view(what, stage, lst, count, w_stage, w_list):
    assert stage.tobytes() == w_stage.tobytes(), f"{what}: stage differs at {np.argwhere(stage != w_stage)[:4].tolist()}"
    assert int(count) == len(w_list), f"{what}: list_count {int(count)} != {len(w_list)}"
    if lst[:count].tobytes() != w_list.tobytes():
        bad = next(i for i in range(len(w_list)) if lst[i].tobytes() != w_list[i].tobytes())
        raise AssertionError(f"{what}: list entry {bad}: {lst[bad]} != {w_list[bad]}")


def run_view_case(pkg, t, orc, case, dev=False):
    sc, v, a, stats, state, clouds, (w_stage, w_list), tally = view_model(orc, case)
    assert case.check(tally), (case.name, {k: x for k, x in tally.items() if x})
    configure(pkg, t, case)
    t.set_water_plane_z(float(sc.water_plane_z))
    n, cap = len(case.tiles), case.capacity
    lstats = (pkg.TileStats * n).from_buffer_copy(stats)
    lv, la = tc.lib_view(pkg, v), lib_view_args(pkg, a)
    st, cl = state.view(pkg.CLOUD_TILE_DTYPE), clouds.view(pkg.CLOUD_DTYPE).reshape(n, cap)
    if not dev:
        stage, lst = t.tiles_cloud_view(case.tiles, lstats, lv, la, st, cl)
        compare_view(case.name, stage, lst.view(cm.INST_DTYPE), len(lst), w_stage, w_list)
        return
    b = dict(ss=t.alloc(C.sizeof(lstats)).upload(np.frombuffer(lstats, np.uint8)), st=t.alloc(n * 88).upload(st.view(np.uint8)), cl=t.alloc(n * cap * 32).upload(cl.view(np.uint8)),
             sg=t.alloc(n * cap).upload(np.full(n * cap, 0x77, np.uint8)), li=t.alloc(n * cap * 24).upload(np.full(n * cap * 6, 0xABCDEF01, np.uint32)), lc=t.alloc(4).upload(np.full(1, 7, np.uint32)))
    try:
        t.tiles_cloud_view_dev(case.tiles, lv, la, b["ss"].ptr, b["st"].ptr, b["cl"].ptr, cap, b["sg"].ptr, b["li"].ptr, b["lc"].ptr)
        cnt = int(b["lc"].download(np.uint32, (1,))[0])
        words = b["li"].download(np.uint32, (n * cap * 6,)).copy()
        assert (words[cnt * 6:] == 0xABCDEF01).all(), "entries past the count were written"
        compare_view(case.name + " (dev)", b["sg"].download(np.uint8, (n, cap)).copy(), words.view(cm.INST_DTYPE), cnt, w_stage, w_list)
    finally:
        for x in b.values():
            x.free()


CHAIN_TILES = [(x, y) for y in range(1, 6) for x in range(-8, -3)]  # over the high ground of the default scene


def run_resident_chain(pkg, gpu, orc):
    """tiles_create_zvals_dev (zvals, stats) -> twenty tiles_update_clouds_dev -> tiles_cloud_view_dev on a 5 x 5 batch at S = 128 on one context, nothing read back
    until the end; against the model fed with the downloaded stats"""
    S, tiles, cap = 128, CHAIN_TILES, 32
    n, Z = len(tiles), S + 2
    case = Case("resident_chain", S=S, tiles=tiles, params=dict(clouds_per_tile=3.0, cloud_height_offset=-0.6), wind=(-0.3, 0.2, 0.0), frames=20)
    sc, step, frames, tally = model(orc, case)
    mgrs = MODEL[case.name][4]
    configure(pkg, gpu, case)
    v = vw.make_view((-75.0, -5.0, float(sc.zmax)), tc._unit(1.0, 0.6, 0.0), (0.0, 0.0, 1.0), 1.3, 1.5, 0.05, 500.0)
    a = cm.ViewArgs(vw.behind_sphere_mult(1.3, 1.5), (0.5, -0.25, 0.0), 35.0)
    b = dict(z=gpu.alloc(n * Z * Z * 4), ss=gpu.alloc(n * C.sizeof(pkg.TileStats)), st=gpu.alloc(n * 88).upload(np.zeros(n * 88, np.uint8)), cl=gpu.alloc(n * cap * 32), to=gpu.alloc(4),
             sg=gpu.alloc(n * cap), li=gpu.alloc(n * cap * 24), lc=gpu.alloc(4))
    try:
        gpu.tiles_create_zvals_dev(tiles, 0, b["z"].ptr, b["ss"].ptr)
        for _ in range(case.frames):
            gpu.tiles_update_clouds_dev(tiles, lib_step(pkg, step), b["st"].ptr, b["cl"].ptr, cap, b["to"].ptr)
        gpu.tiles_cloud_view_dev(tiles, tc.lib_view(pkg, v), lib_view_args(pkg, a), b["ss"].ptr, b["st"].ptr, b["cl"].ptr, cap, b["sg"].ptr, b["li"].ptr, b["lc"].ptr)
        stats = (orclib.TileStats * n).from_buffer_copy(b["ss"].download(np.uint8, (n * C.sizeof(pkg.TileStats),)).tobytes())
        state = b["st"].download(np.uint8, (n * 88,)).copy().view(pkg.CLOUD_TILE_DTYPE)
        clouds = b["cl"].download(np.uint8, (n * cap * 32,)).copy().view(pkg.CLOUD_DTYPE).reshape(n, cap)
        total, cnt = b["to"].download(np.uint32, (1,))[0], int(b["lc"].download(np.uint32, (1,))[0])
        stage, lst = b["sg"].download(np.uint8, (n, cap)).copy(), b["li"].download(np.uint8, (n * cap * 24,)).copy().view(cm.INST_DTYPE)
    finally:
        for x in b.values():
            x.free()
    compare_update("resident chain, frame 19", state, clouds, total, *frames[-1][2:])
    vt = cm.new_tally()
    w_stage, w_list = cm.view(sc, v, a, tiles, stats, mgrs, vt)
    compare_view("resident chain, view", stage, lst, cnt, w_stage, w_list)
    assert tally["to_later"] > 0 and tally["to_earlier"] > 0 and vt["listed"] > 0 and vt["exact_evals"] > 0 and vt["too_distant"] > 0 and vt["ties"] == 0, (tally, vt)
