"""CPU: the node-table lookup of the interp model -- stanford_raytracer_amd/csrc/srt_interp_nodes.hpp's gather with clamp and
sticky flags, its unrolled coefficient rows and InterpModel::eval, the very source the device compiles -- built for the host
(tests/native/interp_nodes_host.cpp) and held against the oracle's tricubic lookup on the same grids.

Bar: the ladder's G0 bar, 1e-11 relative on N = exp(ln N), at every point: the 27 regions around the grid, exact node hits,
one ulp either side of a node, the last interior cell, 200 random interior points."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from interp_layout_cases import G0_BAR, host_grids, oracle_Ns, oracle_model, point_families, rel

SRC = os.path.join(ROOT, "tests", "native", "interp_nodes_host.cpp")
GRIDS = host_grids()


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("inh")
    so = str(d / "libinh.so")
    subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.inh_lnN.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    return L


def host_lnN(L, F, bounds, derivs, pts):
    F = np.ascontiguousarray(F, dtype=np.float64)
    nz, ny, nx, ns = F.shape
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    D = None if derivs is None else np.ascontiguousarray(np.stack(derivs), dtype=np.float64)
    x = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.zeros((len(x), 4))
    assert L.inh_lnN(ns, nx, ny, nz, b.ctypes.data, F.ctypes.data, None if D is None else D.ctypes.data, len(x), x.ctypes.data,
                     out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("case", GRIDS, ids=[g[0] for g in GRIDS])
def test_host_build_of_the_node_table_lookup_against_the_oracle(host, tmp_path, case):
    name, F, bounds, qs, ms, derivs = case
    nz, ny, nx, ns = F.shape
    om = oracle_model(tmp_path, name, F, bounds, qs, ms, derivs)
    for fam, pts in point_families(bounds, (nx, ny, nz)).items():
        want = oracle_Ns(om, pts)[:, :ns]
        assert np.all(np.isfinite(want)) and np.all(want > 0), (name, fam)  # the oracle itself answers at every point
        got = np.exp(host_lnN(host, F, bounds, derivs, pts)[:, :ns])
        err = rel(got, want)
        print("%s %s: %d points, max error %.3g, bit-equal %.1f %%" % (name, fam, len(pts), err.max(), 100 * np.mean(err == 0)))
        assert err.max() <= G0_BAR, (name, fam, int(np.argmax(err.max(axis=1))))


def test_the_program_prints_what_the_function_returns(host, tmp_path):
    name, F, bounds, qs, ms, derivs = GRIDS[1]  # 2 x 2 x 2
    exe = str(tmp_path / "interp_nodes_host")
    subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-o", exe, SRC])
    pts = point_families(bounds, (2, 2, 2))["regions27"]
    text = "%d 2 2 2 0 %d\n" % (F.shape[3], len(pts)) + " ".join("%.17g" % v for v in bounds) + "\n"
    text += " ".join("%.17g" % v for v in F.ravel()) + "\n" + " ".join("%.17g" % v for v in pts.ravel()) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[float(v) for v in ln.split()] for ln in out.splitlines()])
    assert np.array_equal(got, host_lnN(host, F, bounds, None, pts))
