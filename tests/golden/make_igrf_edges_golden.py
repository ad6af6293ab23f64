#!/usr/bin/env python3
"""Golden vectors for the edges of the use_igrf = 1 field (tests/test_igrf_edges.py), from the REAL reference through the
same mechanism as make_igrf_golden.py (oracle/_ref/ref_harness --mode=params --use_igrf=1).  Build container only.
Writes tests/golden/igrf_edges_golden.npz: inputs we authored (tests/igrf_edge_cases.py) + the reference's B.

Families (index array `fam`, names in igrf_edge_cases.FAMILY_NAMES), SM positions in metres:
  0  geographic axis, date 2010001: both hemispheres, r = 1.5, 3.3, 7 R_E, sine of the GEO colatitude 0, 3e-6 (the polar
     branch, s < 1e-5), 2e-5 and 1e-4 (just off it).  The axis comes from the ORACLE's GEO->GSW matrix for the date
     (column A13, A23, A33), rotated back to SM by the dipole tilt; every point's s is checked with the kernel's fp32 head.
  1  one point in every bin of int(r + 2) = 2 .. 31 (r = 0.9 .. 29.5 R_E), date 2010001
  2  a pair a relative 1e-5 either side of every integer r + 2 = 3 .. 31, date 2010001, each >= 8 ulp32 off the integer
  3  twenty shell points (r in [1.02, 9] R_E) at each boundary date of igrf_edge_cases.BOUNDARY_DATES
No family had to be dropped: the reference's funcPlasmaParams returns at r = 0.9 R_E (inside the Earth) and at 29.5 R_E.

    python tests/golden/make_igrf_edges_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import igrf_edge_cases as ec  # noqa: E402
from oracle import oracle, refharness  # noqa: E402
from stanford_raytracer_amd import workloads as wl  # noqa: E402


def inputs(cfg):
    """(x[n, 3] SM metres, fam[n], date_idx[n], dates[nd, 2])"""
    assert wl.R_E == ec.R_E
    dates = [ec.BASE_DATE] + list(ec.BOUNDARY_DATES)
    o = oracle.Model.ngo(cfg, *ec.BASE_DATE).set_igrf(*ec.BASE_DATE)
    _, _, _, A, cs = o.igrf_state()
    rng = np.random.default_rng(20261)
    # (a)
    ga, built = ec.axis_points_gsw(A)
    xa = ec.gsw_to_sm(ga, cs)
    ec.check_axis(ec.head(A, ec.sm_to_gsw32(xa, cs)), built)
    # (b)
    rb = ec.bin_radii()
    xb = ec.gsw_to_sm(ec.unit_vectors(rng, len(rb)) * rb[:, None], cs)
    ec.check_bins(ec.head(A, ec.sm_to_gsw32(xb, cs)))
    rp = ec.pair_radii()
    up = np.repeat(ec.unit_vectors(rng, len(rp) // 2), 2, axis=0)
    xp = ec.gsw_to_sm(up * rp[:, None], cs)
    ec.check_pairs(ec.head(A, ec.sm_to_gsw32(xp, cs)))
    # (c)
    xs, ds = [], []
    for i in range(len(ec.BOUNDARY_DATES)):
        xs.append(ec.unit_vectors(rng, 20) * wl.R_E * rng.uniform(1.02, 9.0, size=(20, 1)))
        ds.append(np.full(20, i + 1))
    x = np.concatenate([xa, xb, xp] + xs)
    fam = np.concatenate([np.full(len(xa), ec.FAM_AXIS), np.full(len(xb), ec.FAM_BIN), np.full(len(xp), ec.FAM_PAIR),
                          np.full(20 * len(ec.BOUNDARY_DATES), ec.FAM_DATE)])
    date_idx = np.concatenate([np.zeros(len(xa) + len(xb) + len(xp), dtype=np.int64)] + ds)
    return x, fam, date_idx, np.array(dates)


def reference(cfg, x, date_idx, dates):
    B = np.zeros((len(x), 3))
    for i, (yd, ms) in enumerate(dates):
        sel = date_idx == i
        ref = refharness.run_mode("params", x[sel], {"kind": 1, "file": cfg, "use_igrf": 1, "yearday": int(yd), "msec": int(ms)})
        B[sel] = ref[:, 16:19]
    return B


def make(cfg):
    x, fam, date_idx, dates = inputs(cfg)
    return {"x": x, "fam": fam, "date_idx": date_idx, "dates": dates, "B": reference(cfg, x, date_idx, dates)}


def main():
    assert refharness.available()
    td = tempfile.mkdtemp()
    cfg = os.path.join(td, "newray.in")
    open(cfg, "w").write(wl.NEWRAY_PLASMAPAUSE)
    store, again = make(cfg), make(cfg)
    for k in store:
        assert store[k].dtype == again[k].dtype and store[k].tobytes() == again[k].tobytes(), "two runs differ in " + k
    assert np.all(np.isfinite(store["B"])) and np.all(np.linalg.norm(store["B"], axis=1) > 0)
    store["provenance"] = np.array("oracle/_ref/ref_harness (flang -O3, x86-64 baseline), geopack2008.for + geopack0508_adapter.for")
    np.savez_compressed(os.path.join(HERE, "igrf_edges_golden.npz"), **store)
    print("wrote igrf_edges_golden.npz", {k: getattr(v, "shape", None) for k, v in store.items()},
          {ec.FAMILY_NAMES[f]: int(np.sum(store["fam"] == f)) for f in ec.FAMILY_NAMES})


if __name__ == "__main__":
    main()
