"""Cases of the turn prelude (terra_engine::gen_grid_dev): a map's tables and the reset of its min / max words are enqueued in FRONT of the host wait for the previous map's
turn event, only the grid launches behind it.  Shared by the emulator tests (the driver's order, on the CPU) and the GPU tests (the same order on a real stream, with the
previous map's kernels still queued).  Every comparison is against the oracle's gen_grid and its min() / max(), bit for bit; every map has an origin of its own, so tables
left over from another map would show."""
import numpy as np
import pytest

from orclib import assert_bit_equal
from parity_cases import cfg_pair

SINE, SIMPLEX = 0, 1
# (mode, nx, ny, sg.turn_rows): 384 x 300 = three tile rows, the last one partial.  No split: sg.turn_rows 0 and a tail that covers the grid; 387 columns: not a multiple
# of 4 (the PACKED = false instantiation of the grid kernel); simplex: the hoisted fill of the min / max words and the island-table launch of the fBm modes
ONE_MAP_CASES = [(SINE, 384, 300, 0), (SINE, 384, 300, 1024), (SINE, 387, 300, 128), (SIMPLEX, 384, 300, 128)]
ORIGINS = [(-159.0, -221.0), (1033.0, 517.0), (-2750.0, 64.0)]  # (x0, y0) of the maps of a case, in call order

_refs = {}


def _cfg(pkg, mode):
    return cfg_pair(pkg, mesh_gen_mode=mode, mesh_freq_filter=1)


def _reference(orc, oc, mode, st, x0, y0, nx, ny):
    key = (mode, x0, y0, nx, ny)
    if key not in _refs:
        orc.init(oc)
        ref = orc.gen_grid(x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, 1)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _check(ref, buf, mm, nx, ny, what):
    assert_bit_equal(ref, buf.download(np.float32, (ny, nx)), what)
    want = np.array([ref.min(), ref.max()], np.float32)
    got = mm.download(np.float32, (2,))
    assert want.tobytes() == got.tobytes(), (what, got, want)


class _Maps:
    """output buffers and events of a case, freed with it"""

    def __init__(self):
        self.owned = []

    def out(self, t, nx, ny):
        buf, mm = t.alloc(nx * ny * 4), t.alloc(8)
        self.owned += [buf.free, mm.free]
        return buf, mm

    def event(self, t):
        ev = t.event_create()
        self.owned.append(lambda: t.event_destroy(ev))
        return ev

    def free(self):
        for f in reversed(self.owned):
            f()


def case_two_contexts_take_turns(pkg, make_ctx, orc, turn_rows, nx=384, ny=300):
    """A -> B -> A: every call gets the event of the map before as wait_for, nothing is synchronized between the calls"""
    a, b = make_ctx(), make_ctx()
    m = _Maps()
    try:
        pc_, oc = _cfg(pkg, SINE)
        st = [c.init_scene(pc_) for c in (a, b)][0]
        for c in (a, b):
            c.set_option("sg.turn_rows", turn_rows)
        ctxs = [a, b, a]
        outs = [m.out(c, nx, ny) for c in ctxs]
        evs = [m.event(c) for c in ctxs]
        for i, c in enumerate(ctxs):
            x0, y0 = ORIGINS[i]
            c.gen_grid_minmax_turn_dev(outs[i][0].ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, outs[i][1].ptr, evs[i - 1] if i else None, evs[i], pkg.GEN_GLACIATE)
        a.synchronize(); b.synchronize()
        for i in range(3):
            x0, y0 = ORIGINS[i]
            _check(_reference(orc, oc, SINE, st, x0, y0, nx, ny), outs[i][0], outs[i][1], nx, ny, f"map {i} of A -> B -> A, sg.turn_rows {turn_rows}")
    finally:
        m.free()
        a.close(); b.close()


def case_back_to_back_growth(pkg, t, orc, turn_rows=128):
    """one context, two turn calls without a synchronize between them; the second is larger: its scratch grows in front of its wait while the first map's kernels are queued"""
    m = _Maps()
    try:
        pc_, oc = _cfg(pkg, SINE)
        st = t.init_scene(pc_)
        t.set_option("sg.turn_rows", turn_rows)
        sizes = [(384, 300), (640, 640)]
        outs = [m.out(t, nx, ny) for nx, ny in sizes]
        evs = [m.event(t) for _ in sizes]
        for i, (nx, ny) in enumerate(sizes):
            x0, y0 = ORIGINS[i]
            t.gen_grid_minmax_turn_dev(outs[i][0].ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, outs[i][1].ptr, evs[i - 1] if i else None, evs[i], pkg.GEN_GLACIATE)
        t.synchronize()
        for i, (nx, ny) in enumerate(sizes):
            x0, y0 = ORIGINS[i]
            _check(_reference(orc, oc, SINE, st, x0, y0, nx, ny), outs[i][0], outs[i][1], nx, ny, f"map {i} of two back to back ({nx} x {ny})")
    finally:
        m.free()


def case_one_map_behind_another(pkg, t, orc, mode, nx, ny, turn_rows):
    """the map under test waits for the turn event of a map at another origin made by the same context just before: its tables are built while that map is still queued"""
    m = _Maps()
    try:
        pc_, oc = _cfg(pkg, mode)
        st = t.init_scene(pc_)
        t.set_option("sg.turn_rows", turn_rows)
        outs = [m.out(t, nx, ny) for _ in range(2)]
        evs = [m.event(t) for _ in range(2)]
        for i in range(2):
            x0, y0 = ORIGINS[i]
            t.gen_grid_minmax_turn_dev(outs[i][0].ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, outs[i][1].ptr, evs[i - 1] if i else None, evs[i], pkg.GEN_GLACIATE)
        t.synchronize()
        for i in range(2):
            x0, y0 = ORIGINS[i]
            _check(_reference(orc, oc, mode, st, x0, y0, nx, ny), outs[i][0], outs[i][1], nx, ny, f"mode {mode}, {nx} x {ny}, sg.turn_rows {turn_rows}, map {i}")
    finally:
        m.free()


def case_invalid_call_then_valid(pkg, t, orc, nx=384, ny=300, turn_rows=128):
    """ny = 0 with wait_for set: the argument error, nothing enqueued; the next call on the context equals the oracle"""
    m = _Maps()
    try:
        pc_, oc = _cfg(pkg, SINE)
        st = t.init_scene(pc_)
        t.set_option("sg.turn_rows", turn_rows)
        buf, mm = m.out(t, nx, ny)
        ev_prev, ev = m.event(t), m.event(t)
        t.event_record(ev_prev)
        x0, y0 = ORIGINS[2]
        with pytest.raises(pkg.TerraError):
            t.gen_grid_minmax_turn_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, 0, mm.ptr, ev_prev, ev, pkg.GEN_GLACIATE)
        x0, y0 = ORIGINS[1]
        t.gen_grid_minmax_turn_dev(buf.ptr, x0, y0, st.DX_VAL, st.DY_VAL, nx, ny, mm.ptr, ev_prev, ev, pkg.GEN_GLACIATE)
        t.synchronize()
        _check(_reference(orc, oc, SINE, st, x0, y0, nx, ny), buf, mm, nx, ny, "valid call behind an invalid one")
    finally:
        m.free()
