#!/usr/bin/env python3
"""What the REAL reference (oracle/_ref/ref_harness, see make_golden.py) returns for the calls of tests/test_oracle_vs_ref.py,
so that those tests run where oracle/_ref is absent: the test module is run once under pytest with its `reference` helper
recording every array it asks the harness for, keyed as the tests read them back.

    python tests/golden/make_oracle_vs_ref_golden.py        (where oracle/_ref is built)
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refharness  # noqa: E402


class Record:
    def __init__(self):
        self.store = {}

    def pytest_collection_finish(self, session):
        mod = sys.modules["test_oracle_vs_ref"]
        mod.reference = lambda key, run: self.store.setdefault(key, np.asarray(run(), dtype=np.float64))


def main():
    if not refharness.available():
        raise SystemExit("oracle/_ref/ref_harness missing: run python oracle/build_ref.py first")
    rec = Record()
    rc = pytest.main([os.path.join(ROOT, "tests", "test_oracle_vs_ref.py"), "-q", "-p", "no:cacheprovider"], plugins=[rec])
    if rc != 0:
        raise SystemExit("tests/test_oracle_vs_ref.py failed against the live reference (rc %d): nothing written" % rc)
    # (compiler and flags; not where the reference's sources lay)
    info = "".join(ln for ln in open(os.path.join(ROOT, "oracle", "_ref", "BUILD_INFO.txt")) if not ln.startswith("reference:"))
    out = os.path.join(HERE, "oracle_vs_ref_golden.npz")
    np.savez_compressed(out, build_info=np.array(info), **rec.store)
    print("wrote %s: %s" % (out, ", ".join("%s %s" % (k, v.shape) for k, v in sorted(rec.store.items()))))


if __name__ == "__main__":
    main()
