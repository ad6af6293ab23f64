#!/usr/bin/env python3
"""Records tests/golden/tail_stash_golden.json on an MI355X: the digests of the launches of tests/tail_stash_cases.py (rows as
bytes, nrows, stop codes, counters[1] accepted steps, counters[2] attempts) plus, for the record, the stop codes and row counts
they cover.  Run it with the library of the commit BEFORE the tail stash (check that commit out, or point SRT_LIB_OVERRIDE at a
build of it): the test then holds the stash against a library that has none.

    python tests/golden/make_tail_stash_golden.py [OUT.json]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402  (before the library's first call)

import tail_stash_cases as tc  # noqa: E402
from stanford_raytracer_amd import api  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tail_stash_golden.json")
    torch.cuda.init()
    api.init(0)
    pos, d, w = tc.rays()
    models, gold = {}, {}
    for name, (kind, extra, env) in tc.CASES.items():
        if kind not in models:
            models[kind] = tc.make_model(kind)
        r = tc.launch(models[kind], api.make_params(**dict(tc.TRACE, **extra)), pos, d, w)
        g = tc.digests(*r)
        codes, counts = np.unique(r[2], return_counts=True)
        g["stop_codes"] = {int(c): int(n) for c, n in zip(codes, counts)}
        g["rays_reaching_mark"] = [int(np.sum(r[1] > m)) for m in tc.MARKS]
        g["rays_stopping_at_mark"] = [int(np.sum(r[1] == m)) for m in tc.MARKS]
        gold[name] = g
        print(name, g)
    with open(out, "w") as f:
        json.dump({"has_tail_stash": hasattr(api.lib(), "srt_launch_stash_stats"), "cases": gold}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
