#!/usr/bin/env python3
"""Generates tests/golden/hybrid_recipe_yardstick.json: for every mixed KKT recipe of the suite (wide, few-entry and
single-entry constraints in one system: tests/dense_ref.py HYBRID_CASES and the hybrid cases of tests/route_ledger.py), the
error of the CPU oracle against the dense definitions of tests/dense_ref.py (kkt_H, kkt_x per clique, kkt_y), keyed by
dense_ref.recipe_key(pattern, recipe).

What it is for: the device bound of a hybrid case is 100 x the larger of the global yardstick value
(tests/golden/dense_ref_yardstick.json) and the value recorded here, capped at dense_ref.BOUND_CAP (dense_ref.hybrid_bound);
tests/test_hybrid_recipes.py asserts on a CPU that the oracle stays within 10 x of these values.

Run from the repo root:  python tests/golden/make_hybrid_recipe_yardstick.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from oracle import oracle
    from smcp_amd import build as b
    b.build(verbose=False)
    oracle.build()
    from tests import test_hybrid_recipes as thr
    out = {}
    for key, hc in sorted(thr.all_hybrid_cases().items()):
        out[key] = {op: float(e) for op, e in thr.oracle_kkt_errors(hc).items()}
        print(key[:60], " ".join("%s=%.1e" % kv for kv in sorted(out[key].items())), flush=True)
    from tests import dense_ref
    with open(dense_ref.MIX_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
