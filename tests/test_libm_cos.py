"""rtw_cosf (csrc/rtw_libm.h: musl cosf in the style of rtw_sinf, for the cone sampling of sphere lights), compiled
here for the host with the device's contract-off flags as tests/test_libm.py does: within 1 ulp of the float64
cosine.  The reference calls no cosine and the oracle's zig_libm.h has none, so the float64 function is the only
yardstick."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

HARNESS = r"""
#include <stdint.h>
#include "rtw_libm.h"
void prod_cos(const float* a, float* out, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) out[i] = rtw_cosf(a[i]);
}
"""


@pytest.fixture(scope="module")
def prod_cos(tmp_path_factory):
    d = tmp_path_factory.mktemp("libm_cos")
    src = d / "h.c"
    src.write_text(HARNESS)
    so = d / "libh.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           "-I", os.path.join(REPO, "zig-raytracing-weekend_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.prod_cos.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]

    def run(a):
        a = np.ascontiguousarray(a, np.float32)
        out = np.empty_like(a)
        lib.prod_cos(a.ctypes.data, out.ctypes.data, a.size)
        return out
    return run


def ulp_err(got, exact):
    """|got - exact| in units of the float32 spacing at `exact` (float64 reference)."""
    e32 = exact.astype(np.float32)
    sp = np.spacing(np.abs(e32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - exact) / sp


def test_cos_below_one_ulp(prod_cos):
    """A dense grid of [0, 2 pi] (the azimuths the cone sampling asks for: phi = 2 pi a, a in [0, 1)), the float32
    neighbours of every range boundary of the algorithm, and random values in [-100, 100] (the medium-size
    reduction)."""
    grid = np.linspace(0.0, 2 * np.pi, 2_000_001).astype(np.float32)
    edges = np.array([0x39800000, 0x3F490FDA, 0x4016CBE3, 0x407B53D1, 0x40AFEDDF, 0x40E231D5], np.uint32)
    near = (edges[:, None] + np.arange(-4, 5, dtype=np.int64)[None, :]).astype(np.uint32).reshape(-1).view(np.float32)
    rnd = np.random.default_rng(5).uniform(-100.0, 100.0, 1_000_000).astype(np.float32)
    x = np.concatenate([grid, near, -near, rnd])
    got = prod_cos(x)
    err = ulp_err(got, np.cos(x.astype(np.float64)))
    print(f"rtw_cosf: {x.size} arguments, worst error {err.max():.4f} ulp at x = {x[err.argmax()]!r}")
    assert np.isfinite(got).all()
    assert err.max() < 1.0


def test_cos_special_values(prod_cos):
    got = prod_cos(np.array([0.0, -0.0, 1e-5, np.inf, -np.inf, np.nan], np.float32))
    assert got[:3].tolist() == [1.0, 1.0, 1.0]
    assert np.isnan(got[3:]).all()
