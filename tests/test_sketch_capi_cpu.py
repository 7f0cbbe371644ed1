"""CPU: the Gaussian-sketch entry points are exported and bound, and include/xerus_amd.h still compiles as C."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKETCH_SYMBOLS = ["xrs_philox_words", "xrs_gaussian_matrix", "xrs_sketch_gaussian", "xrs_sketch_last_route"]


def test_sketch_symbols_are_declared_bound_and_exported():
    from xerus_amd import capi

    hdr = open(os.path.join(ROOT, "include", "xerus_amd.h")).read()
    capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (xrs_[a-z0-9_]+)", out))
    for name in SKETCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SIGNATURES, name
        assert name in exported, name
    assert capi.SKETCH_ROUTES[capi.SKETCH_FUSED] == "fused" and capi.SKETCH_ROUTES[capi.SKETCH_MATERIALISED] == "materialised"


def test_header_compiles_as_c():
    src = ('#include "xerus_amd.h"\n'
           "int use(xrs_handle_t h, double* y, const double* a) {\n"
           "    return xrs_sketch_gaussian(h, y, 2, a, 3, 4, 5u, 6u, XRS_SKETCH_FUSED) + xrs_sketch_last_route(h);\n"
           "}\n")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.c")
        with open(path, "w") as f:
            f.write(src)
        res = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), path],
                             capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_stream_and_seed_are_range_checked_before_ctypes_wraps_them():
    """uint32 / uint64 arguments: ctypes would wrap 2^32 to 0 silently; the binding raises XRS_EINVAL instead."""
    import pytest

    from xerus_amd import capi

    with pytest.raises(capi.XrsError) as info:
        capi.Handle._seed_stream("xrs_sketch_gaussian", 1, 2 ** 32)
    assert info.value.code == -1
    with pytest.raises(capi.XrsError):
        capi.Handle._seed_stream("xrs_sketch_gaussian", 2 ** 64, 0)
    assert capi.Handle._seed_stream("xrs_sketch_gaussian", 2 ** 64 - 1, 2 ** 32 - 1) == (2 ** 64 - 1, 2 ** 32 - 1)
