#!/usr/bin/env python3
"""Generates tests/golden/dense_ref_yardstick.json: per operation, the worst error of the CPU oracle against the dense
definitions of tests/dense_ref.py over every pattern of tests.helpers.GPU_PATTERNS, on the product's symbolic arrays and on
oracle.symbolic_ref, with the pattern, symbolic source and seed of the worst case.

What it is for: tests/test_dense_ref.py asserts that the oracle stays within 10 x of these values, and the device checks of
tests/test_gpu_dense_ref.py / tests/test_gpu_contract.py take their bounds from them (100 x, capped at 1e-12).

Run from the repo root:  python tests/golden/make_dense_ref_yardstick.py
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
    from tests import dense_ref
    from tests.helpers import GPU_PATTERNS
    worst = {}
    for name in sorted(GPU_PATTERNS):
        for which in ("product", "ref"):
            errs = dense_ref.oracle_yardstick(name, which)
            print(name, which, " ".join("%s=%.1e" % kv for kv in sorted(errs.items())), flush=True)
            for op, e in errs.items():
                if op not in worst or e > worst[op]["value"]:
                    worst[op] = dict(value=float(e), pattern=name, symbolic=which, seed=dense_ref.YARDSTICK_SEED)
    with open(dense_ref.YARDSTICK_FILE, "w") as f:
        json.dump(dict(sorted(worst.items())), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
