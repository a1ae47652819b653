"""The gfx950 compilation of the primitives every pass shares, alone: tests/devprobe's device build evaluates each family of TERRA_HD bodies in one kernel on the
inputs of tests/golden/primitive_vectors.npz, and the results are the reference's recorded ones, exactly (tests/primitive_cases.py).  Reads the fixture only."""
import os
import sys

import pytest

import primitive_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "devprobe"))
import build_probe  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return pc.load()


@pytest.fixture(scope="module")
def device_probe():
    """libterra_devprobe_hip.so: built with the tree (oracle/Makefile: probe); compiled here only when it is missing or stale.  No library is a failure, not a skip"""
    p = pc.Probe(build_probe.build("hip"))
    assert p.is_device
    return p


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_device_probe_matches_the_reference(device_probe, fx, family):
    n = pc.check_probe(device_probe, fx, family)             # every row (the view families: a launch per camera, none a multiple of 256)
    assert n > 0
    pc.check_probe(device_probe, fx, family, limit=1)        # n = 1
    pc.check_probe(device_probe, fx, family, limit=257)      # one full block and one thread of the next


def test_device_abi_cameras_match_the_reference(gpu, fx):
    """terra_make_view and terra_view_behind_sphere_mult of libterra_hip.so"""
    pc.check_abi_cameras(gpu, fx)
