"""The primitives every pass shares -- the view tests, the libm restatements, the x86 conversions, InvSqrt, the line clip, the LOD statement -- against what the
reference's own compiled code answered for tests/golden/primitive_vectors.npz (layout and inputs: tests/primitive_cases.py, tests/golden/make_primitive_golden.py).
Everything is exact: floats bit for bit, decisions and integers value for value.  The device half is tests/test_gpu_primitives.py."""
import os
import sys

import pytest

import primitive_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "devprobe"))
import build_probe  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return pc.load()


@pytest.fixture(scope="module")
def host_probe():
    return pc.Probe(build_probe.build("host"))


def test_fixture_matches_the_live_reference(ref, fx):
    """(a) every row re-evaluated through the reference's own code (skipped where oracle/_ref is absent, like every `ref` test); the libm rows through this C library"""
    got = pc.eval_reference(ref, fx)
    got.update(pc.eval_libm(fx))
    assert set(got) == {k for keys in pc.OUTPUTS.values() for k in keys}
    for k, v in got.items():
        pc.assert_same(k, fx[k], v)


def test_fixture_keeps_its_coverage(fx):
    """the conditions the generator asserted, on the file as it is committed"""
    decisions = [fx["pt_out"], fx["sp_out"], fx["lc_ok"]] + [fx["cb_out"][:, j] for j in range(5)]
    for d in decisions:
        assert 0.1 <= d.astype(bool).mean() <= 0.9
    assert pc.num_cameras(fx) >= 12 and (fx["cam_valid"] == 0).sum() == 1
    assert sum(len(fx[pc.OUTPUTS[f][0]]) for f in pc.FAMILIES) <= 200000
    assert len(pc.constructed_cameras(fx)) == pc.num_cameras(fx) - 1


@pytest.fixture(scope="module")
def model_results(fx):
    return pc.eval_models(fx)


# Every reference function the fixture has rows for, against the one restatement the pass models share.  (One entry fewer than when the terrain and the tree model
# each had a sphere_visible_test of their own: the two became view_model's, pinned against the same rows.)
MODEL_PRIMITIVES = ["view_model.make_view", "view_model.point_visible_test", "view_model.cube_visible", "view_model.cube_completely_visible", "view_model.f2u",
                    "view_model.behind_sphere_mult", "view_model.sphere_visible_test", "terrain_view_model.lod_steep_dist", "view_model.inv_sqrt", "view_model.d2u",
                    "view_model.cube_visible_likely", "view_model.d2i", "view_model.f2i", "view_model.do_line_clip (ok)", "view_model.do_line_clip (ends)"]


@pytest.mark.parametrize("name", MODEL_PRIMITIVES)
def test_model_primitive_matches_the_reference(model_results, name):
    """(b) the Python models the passes are tested against, on the fixture's inputs"""
    exp, got = model_results[name]
    pc.assert_same(name, exp, got)


def test_every_model_primitive_is_listed(model_results):
    assert sorted(model_results) == sorted(MODEL_PRIMITIVES)


def test_no_model_keeps_a_copy():
    """whatever a model module (tests/*_model.py, the test_* files aside) calls by the name of one of view_model's public functions or classes is that very object: an
    alias at the most, never a second body that the fixture would not pin"""
    import glob
    import importlib
    import view_model
    public = {n: o for n, o in vars(view_model).items() if not n.startswith("_") and callable(o) and getattr(o, "__module__", None) == "view_model"}
    assert {"make_view", "behind_sphere_mult", "point_visible_test", "sphere_visible_test", "cube_visible", "cube_completely_visible", "cube_visible_likely", "inv_sqrt",
            "f2i", "f2u", "d2i", "d2u", "do_line_clip", "dot", "sub", "mag_sq", "cmin", "cmax"} <= set(public)
    here = os.path.dirname(os.path.abspath(__file__))
    names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(here, "*_model.py")) if not os.path.basename(p).startswith("test_"))
    assert "view_model" in names and len(names) > 15
    copies = [f"{m}.{n}" for m in names for n, o in public.items() if getattr(importlib.import_module(m), n, o) is not o]
    assert not copies, copies


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_host_probe_matches_the_reference(host_probe, fx, family):
    """(c) the TERRA_HD bodies as g++ compiles them for the host emulation"""
    assert not host_probe.is_device
    pc.check_probe(host_probe, fx, family)
    pc.check_probe(host_probe, fx, family, limit=1)


def test_host_abi_cameras_match_the_reference(emul, fx):
    """(c) terra_make_view and terra_view_behind_sphere_mult of the host emulation library"""
    pc.check_abi_cameras(emul, fx)
