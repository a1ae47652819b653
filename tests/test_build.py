import pytest


@pytest.mark.parametrize("header", ["terra_grassview.hpp", "terra_treeview.hpp", "terra_sceneryview.hpp", "terra_decidview.hpp", "terra_lineintersect.hpp", "terra_terrainview.hpp",
                                    "terra_waterview.hpp", "terra_clouds.hpp", "terra_smapview.hpp"])
def test_pass_header_stands_alone(header, tmp_path):
    """A pass header holds the pass's records, its argument rules, constants, leaf functions and literal bodies, and the line-query header the leaf code the grass pass
    shares with the line queries: a translation unit that includes nothing else compiles as plain C++17 -- nothing in them needs the driver."""
    import os, shutil, subprocess
    cxx = shutil.which(os.environ.get("CXX") or "g++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(root, "3dworld_amd", "csrc"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_hot_kernels_do_not_spill():
    """The droplet trace kernel, the sine grid kernel and the fBm kernels must compile without scratch memory: small source changes have tipped the register
    allocator into spilling inside the droplet step loop before (1.3-1.7x slower on the GPU, same results) -- tools/check_kernel_resources.py."""
    import os, shutil, subprocess, sys
    import pytest
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_kernel_resources.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shipped_library_matches_the_sources():
    """libterra_hip.so travels with the tree (built in place, git-ignored): its recorded source hash must be the hash of csrc/ + include/terra.h + flags as they
    are now, so a stale library cannot pass for the current code (3dworld_amd/build.py)"""
    import importlib, os
    import pytest
    bmod = importlib.import_module("3dworld_amd.build")
    if not os.path.exists(bmod.LIB):
        pytest.skip("library not built yet (__graft_entry__.build() does it)")
    assert not bmod.needs_build(), "libterra_hip.so was built from other sources: run __graft_entry__.build()"
