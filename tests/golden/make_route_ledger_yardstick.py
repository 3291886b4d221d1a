#!/usr/bin/env python3
"""Generates tests/golden/route_ledger_yardstick.json: for every pattern of tests/route_ledger.py that is not in
tests.helpers.GPU_PATTERNS, per operation the worst error of the CPU oracle against the dense definitions of
tests/dense_ref.py (dense_ref.measure(case, dense_ref.oracle_ops(case)) on the product's symbolic arrays), over the KKT
inputs the ledger uses on that pattern.

What it is for: tests/test_gpu_route_ledger.py asserts on a CPU that the oracle stays within 10 x of these values and that each
of them is at most 1 / 100 of the bound the ledger applies to the device on that pattern (route_ledger.bound_of).

Run from the repo root:  python tests/golden/make_route_ledger_yardstick.py
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
    from tests import route_ledger
    out = {}
    for name in sorted(route_ledger.NEW_PATTERNS):
        out[name] = route_ledger.oracle_errors(name)
        print(name, " ".join("%s=%.1e" % kv for kv in sorted(out[name].items())), flush=True)
    with open(route_ledger.YARDSTICK_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
