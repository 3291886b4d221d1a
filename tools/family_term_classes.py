"""Class counts of the (family, constraint) term lists of a workload: dense terms Td and unit terms Tu (one vector a unit
vector of the family parent's separator part: constraints.cpp, family_term_lists), and the matrix-pipe steps per list of the
fused extend-add with and without the unit terms (front_famt.hip, lf_add_family) -- and what leaving the dead ordered
pairs out of k_fam_terms<NAT, false> would make of its steps (not done: DESIGN section 7).  Counted on the host from the
positions of the constraint entries; needs the device only for the family roles.

    python tools/family_term_classes.py [--workload synth50k] > classes.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synth50k")
    args = ap.parse_args()
    import bench
    from smcp_amd import problems
    from smcp_amd.symbolic import Symbolic
    pat, m, density, label = bench.build_workload(args.workload)
    symb = Symbolic(pat)
    symb.device_init(0, 4)
    cptr, cidx, cval = problems.random_constraints(symb, m, density=density, seed=1)
    roles = symb.family_roles()
    nn, na = symb.clique_sizes()
    blkptr, chptr, chidx, sepptr, relidx = symb.blkptr, symb.chptr, symb.chidx, symb.sepptr, symb.relidx
    parents = np.nonzero(roles == 2)[0]
    fam_of = np.full(symb.Nsn, -1, dtype=np.int64)          # clique -> family number
    for f, k in enumerate(parents):
        fam_of[k] = f
        fam_of[chidx[chptr[k]:chptr[k + 1]]] = f
    k_of = np.searchsorted(blkptr, cidx, side="right") - 1  # clique of every entry
    f_of = fam_of[k_of]
    inside = f_of >= 0
    off = cidx - blkptr[k_of]
    nf = (nn + na)[k_of]
    row = off % nf
    # unit term: a separator-row entry of the parent, or of a child when the row lands in the parent's separator part
    is_parent = roles[k_of] == 2
    par = np.where(is_parent, k_of, symb.snpar[k_of])
    seprow = row >= nn[k_of]
    rel = relidx[np.minimum(sepptr[k_of] + np.maximum(row - nn[k_of], 0), len(relidx) - 1)]
    unit = inside & seprow & (is_parent | (rel >= nn[par]))
    j_of = np.searchsorted(cptr, np.arange(len(cidx)), side="right") - 1
    nfam = len(parents)
    T = np.zeros((nfam, m), dtype=np.int64)
    Tu = np.zeros((nfam, m), dtype=np.int64)
    np.add.at(T, (f_of[inside], j_of[inside]), 1)
    np.add.at(Tu, (f_of[unit], j_of[unit]), 1)
    Td = T - Tu
    ceil4 = lambda x: (x + 3) // 4
    out = {
        "workload": label, "families": int(nfam), "constraints": int(m), "lists": int(nfam * m),
        "mean_T": float(T.mean()), "mean_Td": float(Td.mean()), "mean_Tu": float(Tu.mean()),
        "max_T": int(T.max()), "unit_share": float(Tu.sum() / max(1, T.sum())),
        "lists_without_dense_terms": float(((Td == 0) & (T > 0)).mean()), "empty_lists": float((T == 0).mean()),
        # (lists of more than 64 terms / 48 entries go in chunks; none on this workload when max_T <= 48)
        "extend_add_steps_per_list": {"before": float(ceil4(2 * T).mean()), "after": float(ceil4(2 * Td).mean())},
        "fam_terms_steps_per_list": {"now": float(ceil4(2 * T).mean()), "live_pairs_only": float(ceil4(2 * Td + Tu).mean())},
        "extend_add_mfma_per_list": {"before": float(10 * ceil4(2 * T).mean()), "after": float(10 * ceil4(2 * Td).mean())},
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
