"""The host entry points' staging (3dworld_amd/csrc/terra_stage.hpp) through tests/emul/libterra_emul.so: host form against device form with every, no and a mixed
pick of optional arrays, untouched padding, a scratch that is regrown, the empty batch (tests/host_staging_cases.py); and every converted host entry point once
under the address and undefined-behaviour sanitizers, as a stand-alone program (tests/emul/stage_san_main.cpp); and the grow-only device buffer on its own, over a
counting backend, under the same sanitizers (tests/emul/dev_buf_main.cpp)."""
import os
import subprocess

import pytest

import host_staging_cases as hsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("opt", hsc.OPTS)
@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_host_form_equals_device_form(pkg, emul, entry, opt):
    hsc.run_forms(pkg, emul, entry, opt)


@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_scratch_regrowth(pkg, emul, entry):
    hsc.run_regrowth(pkg, emul, entry)


@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_empty_batch(pkg, emul, entry):
    hsc.run_empty(pkg, emul, entry)


def run_sanitized(tmp_path, name, libs=()):
    """tests/emul/<name>.cpp built with the address and undefined-behaviour sanitizers and run as a child process: nothing is preloaded, nothing is loaded into Python"""
    src, exe = os.path.join(ROOT, "tests", "emul", name + ".cpp"), str(tmp_path / name)
    base = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", exe, src]
    errs = []
    for extra in ([], ["-static-libasan", "-static-libubsan"]):
        r = subprocess.run(base + extra + list(libs), capture_output=True, text=True)
        if r.returncode == 0:
            break
        errs.append(r.stderr[-2000:])
    else:
        if all(("asan" in e or "ubsan" in e) and ("cannot find" in e or "No such file" in e) for e in errs):
            pytest.skip("no sanitizer runtime can be linked here: " + errs[-1][-300:])
        raise AssertionError(name + ".cpp does not compile:\n" + errs[0])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_sanitized_host_entry_points(tmp_path):
    """tests/emul/stage_san_main.cpp: its own main over terra_emul.cpp, every converted host entry point once with the mixed pick of optional arrays at S = 16, n = 3,
    capacity 1."""
    run_sanitized(tmp_path, "stage_san_main", ["-lz"])


def test_sanitized_dev_buf(tmp_path):
    """tests/emul/dev_buf_main.cpp: dev_buf_t over a backend that counts alloc / free / sync and can refuse an allocation -- growing past the size frees once after one
    sync, a throwing grow leaves an empty buffer and the next one allocates afresh, two drops free once, a request within the size allocates nothing."""
    run_sanitized(tmp_path, "dev_buf_main")
