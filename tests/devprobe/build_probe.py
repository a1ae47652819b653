"""Build recipe of the primitive probe (TEST INFRASTRUCTURE ONLY): tests/devprobe/terra_devprobe.hip compiled twice,

    libterra_devprobe_hip.so    hipcc with the product's own flags (3dworld_amd.build.FLAGS) for gfx950
    libterra_devprobe_host.so   g++ -x c++ with the host emulation's flags (-O2 -ffp-contract=off)

Each build is keyed on a content hash of the probe source, every 3dworld_amd/csrc/*.hpp and the flags (as 3dworld_amd/build.py keys the product), so a library
that travelled with the tree is used as it is and one built from other sources is rebuilt.  `python build_probe.py [host|hip|all]` is what oracle/Makefile runs."""
import fcntl
import hashlib
import importlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "3dworld_amd", "csrc")
SRC = os.path.join(HERE, "terra_devprobe.hip")
HOST_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas"]  # tests/conftest.py: emul_lib


def _product_build():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("3dworld_amd.build")


def flags(kind):
    return list(_product_build().FLAGS) if kind == "hip" else HOST_FLAGS


def lib_path(kind):
    assert kind in ("hip", "host")
    return os.path.join(HERE, f"libterra_devprobe_{kind}.so")


def have_hipcc():
    try:
        _product_build().hipcc_path()
        return True
    except RuntimeError:
        return False


def source_hash(kind):
    h = hashlib.sha256()
    files = [SRC] + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")) + [os.path.join(ROOT, "include", "terra.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update((kind + " " + " ".join(flags(kind))).encode())
    return h.hexdigest()


def needs_build(kind):
    lib = lib_path(kind)
    if not os.path.exists(lib) or not os.path.exists(lib + ".srchash"):
        return True
    with open(lib + ".srchash") as f:
        return f.read().strip() != source_hash(kind)


def build(kind, force=False):
    """-> the library's path; compiles only when the library is missing or was built from other sources (RuntimeError when the compiler fails or is missing)"""
    lib = lib_path(kind)
    if not force and not needs_build(kind):
        return lib
    with open(lib + ".lock", "w") as lk:  # several test workers may find it stale at once: one builds, the others find it fresh
        fcntl.flock(lk, fcntl.LOCK_EX)
        if force or needs_build(kind):
            tmp = f"{lib}.{os.getpid()}.tmp"
            if kind == "hip":
                cmd = [_product_build().hipcc_path()] + flags(kind) + ["-I", CSRC, SRC, "-o", tmp, "-lz"]
            else:
                cmd = ["g++"] + flags(kind) + ["-I", CSRC, "-x", "c++", SRC, "-o", tmp, "-lz"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"devprobe ({kind}) build failed:\n" + r.stdout + r.stderr)
            os.replace(tmp, lib)
            with open(lib + ".srchash", "w") as f:
                f.write(source_hash(kind) + "\n")
    return lib


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("host", "all"):
        build("host")
    if which == "hip" or (which == "all" and have_hipcc()):
        build("hip")
    elif which == "all":
        print("devprobe: hipcc not found, libterra_devprobe_hip.so not built")
