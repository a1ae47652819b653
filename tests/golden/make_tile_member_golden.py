"""Generate tests/golden/tile_member_vectors.npz: a compact recording -- inputs together with the outputs of the REFERENCE'S OWN compiled tile_t members
(oracle/_ref/tiled_mesh.o through oracle/ref_shim.cpp section 4) -- of add_tree_ao_shadow, upload_shadow_map_texture, create_texture's existing-weights branch,
line_intersect_mesh (inc_trees = 0) and add_or_remove_grass_at.  Run where the reference tree is (it is not needed to run the tests):

    python tests/golden/make_tile_member_golden.py

The inputs are tests/tile_member_cases.py's (seeded or formulas; that module's record() says what is kept and how): the line rows, the grass strokes, one splat
list per tree-map kind, the shadow texture's light-factor set on one tile, the tree weights' (tree_ao, grass) pair set.  Only the .npz is kept.

The generator asserts and prints: line hits and misses are each >= 25 % of the rows; within the +-ulp groups of each line kind the reference's answer changes inside
>= 25 % of the groups (a kind that cannot reach that is listed in CANNOT with the reason); the Python models reproduce every recorded byte; the number of rows the
models would have skipped as undefined in the reference, which is 0."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import orclib  # noqa: E402
import tile_member_cases as tmc  # noqa: E402

# line kinds whose +-ulp groups cannot reach 25 %, and why
CANNOT = {}


def main():
    orclib.build_oracle()
    assert orclib.ref_available(), "the reference tree is needed to record"
    ref = orclib.Checker("ref")
    fx, text, by_kind, reach = tmc.record(ref)
    tmc.check_grass_tallies(reach)
    hit = fx["line_hits"]["hit"] != 0
    assert 0.25 <= hit.mean() <= 0.75, f"hits {hit.mean()}"
    for k, (n, f) in sorted(by_kind.items()):
        if k in CANNOT:
            text.append(f"  {tmc.LINE_KINDS[k]}: below 25 % -- {CANNOT[k]}")
        else:
            assert f >= 0.25 * n, f"{tmc.LINE_KINDS[k]}: the reference's answer changes inside {f} of {n} groups"
    np.savez_compressed(tmc.FIXTURE, **fx)
    size = os.path.getsize(tmc.FIXTURE)
    text.append(f"{os.path.relpath(tmc.FIXTURE, ROOT)}: {size} bytes")
    assert size < 1000000
    # the models on the recording
    fx = tmc.load()
    skipped = 0
    try:
        cases, want = tmc.fixture_tree(fx)
        got, sk = tmc.model_tree(ref, cases)
        skipped += sk
        tmc.compare_tree("model", cases, got, want)
        for k in range(len(fx["shadow_lf"])):
            call, tex = tmc.fixture_shadow(fx, k)
            tmc.first_diff(f"model: shadow texture at light factor {call[0]!r}", tmc.model_shadow(call), tex)
        w, tm, out = tmc.fixture_weights(fx)
        tmc.first_diff("model: tree weights", tmc.tmm.tree_weights(w, tm), out)
        sc = tmc.fixture_line_scene(fx)
        skipped += tmc.line_rows_undefined(sc, fx["line_rows"])
        tmc.compare_lines("model", tmc.model_lines(sc, fx["line_tiles"], fx["line_z"], fx["line_mz"], fx["line_rows"], fx["line_kind"], fx["line_tile"]), fx["line_hits"], fx["line_kind"])
        gsc = tmc.grass_scene(ref)
        for k in range(len(fx["grass_strokes"])):
            s, want = tmc.fixture_stroke(fx, k)
            got = tmc.model_stroke(gsc, fx["grass_d"], s)
            tmc.compare_stroke(f"model: stroke {k}", got, want)
            assert got[3] == want[3] and tmc.calls_equal(want[4], got[4]), f"stroke {k}: flag / flower calls {want[3:]} != {got[3:]}"
    finally:
        ref.set_landscape(orclib.make_landscape())
    text.append(f"the models reproduce every recorded byte; rows skipped as undefined in the reference: {skipped}")
    assert skipped == 0
    print("\n".join(text))


if __name__ == "__main__":
    main()
