"""The identity element is exact in the resident launch's scans (parallel-gps_amd/csrc/pgps_resident.hip.h): filt_combine and
smth_combine of pgps_math.h with the identity on either side return the other operand bit for bit (d = 2, fp64, random
finite operands).  The workgroup scans rely on it: at the row levels every lane combines, with the identity where the DPP
shift has no source lane, instead of keeping its value by a select.  Compiled with g++ as is and, where the CPU has FMA, with
contraction on as the device compiler does it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_math", "res_identity.cpp")
INC = os.path.join(ROOT, "parallel-gps_amd", "csrc")


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


FLAGS = [["-O2"]] + ([["-O2", "-mfma", "-ffp-contract=fast"]] if _has_fma() else [])


@pytest.fixture(scope="module", params=range(len(FLAGS)), ids=lambda i: " ".join(FLAGS[i]))
def harness(request, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("res_identity") / "libresid.so")
    subprocess.run(["g++"] + FLAGS[request.param] + ["-std=c++17", "-shared", "-fPIC", "-I", INC, SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


def _elements(width, n, seed):
    """random finite operands over forty orders of magnitude, packed as the element structs lay them out"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal((n, width)) * np.exp(rng.uniform(-46, 46, (n, width))))


@pytest.mark.parametrize("kind,width", [("filt", 14), ("smth", 9)])
def test_identity_combine_is_exact(harness, kind, width):
    n = 4096
    x = _elements(width, n, seed=7 if kind == "filt" else 11)
    out = np.empty((2 * n, width))
    fn = getattr(harness, f"res_identity_{kind}_f64_d2")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    assert fn(p(x), ctypes.c_long(n), p(out)) == width
    left, right = out[0::2], out[1::2]
    assert np.array_equal(left.view(np.uint64), x.view(np.uint64)), "combine(identity, x) != x"
    assert np.array_equal(right.view(np.uint64), x.view(np.uint64)), "combine(x, identity) != x"
