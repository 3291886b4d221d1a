"""CPU: the mixed KKT recipes of the hybrid Schur cases (tests/dense_ref.py HYBRID_CASES, the hybrid cases of tests/route_ledger.py).

A hybrid case means something only if the device takes its wide constraints through the Hessian and its narrow ones through
the SCMcolumn2 columns.  The device asserts its own classification where the case runs (dense_ref.device_kkt); here, without a
device, the rule of constraints.cpp classify_columns is applied to the same inputs: a constraint is column-sparse when its
entries touch at most min(int(n * tnzcols), trsm_cap) distinct rows / columns.  And the oracle-vs-dense error of every recipe
is held against its record (tests/golden/hybrid_recipe_yardstick.json), from which the device bounds follow.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests import route_ledger as rl

KKT_OPS = ("kkt_H", "kkt_x", "kkt_y")
_CASES = {}


def all_hybrid_cases():
    """recipe key -> hybrid case, over the GPU module's table and the ledger's scenarios"""
    out = {dense_ref.recipe_key(hc["pattern"], hc["recipe"]): hc for hc in dense_ref.HYBRID_CASES.values()}
    for key, hc in rl.hybrid_cases().items():
        out.setdefault(key, hc)
    return out


def dense_case(pattern):
    if pattern not in _CASES:
        pat = rl.LEDGER_PATTERNS[pattern]()
        _CASES[pattern] = dense_ref.DenseCase(pat, orc.Sym(Symbolic(pat)), dense_ref.YARDSTICK_SEED)
    return _CASES[pattern]


def oracle_kkt_errors(hc):
    case = dense_case(hc["pattern"])
    case.kkt_recipe, case._kkt = hc["recipe"], None
    return dense_ref.kkt_errors(case, dense_ref.oracle_ops(case).kkt)


def trsm_cap(S, max_rhs):
    """constraints.cpp classify_columns: max_rhs * tmplen / (sum of the separator sizes), tmplen = 2 blklen + 256 nsn (setup.hip)"""
    sepsum = max(1, sum(len(rows) - nn for _, nn, rows in S._iter()))
    return max(1, (max_rhs * (2 * S.blklen + 256 * S.nsn)) // sepsum)


def host_classes(hc):
    """(wide constraints the rule sweeps, narrow ones it takes as column-sparse, the others, columns of the sparse ones, trsm_cap)"""
    case = dense_case(hc["pattern"])
    case.kkt_recipe, case._kkt = hc["recipe"], None
    mix = hc["recipe"][3]
    cap = trsm_cap(case.S, hc["max_rhs"])
    tnz = min(int(case.S.n * hc["tnzcols"]), cap)
    t = dense_ref.touched(case.S, case.kkt().con)
    swept = sum(1 for k, kind in zip(t, mix) if kind == "w" and k > tnz)
    sparse = sum(1 for k, kind in zip(t, mix) if kind != "w" and 0 < k <= tnz)
    return swept, sparse, len(mix) - swept - sparse, sum(k for k, kind in zip(t, mix) if kind != "w"), cap


def test_interleave_and_the_mixed_generator():
    assert dense_ref.interleave(5, 4, 3) == "fwsfwsfwsfww" and dense_ref.interleave(1, 3, 2) == "fwsfsf" and dense_ref.interleave(2, 0, 3) == "wswss"
    case = dense_case("nested")
    mix = dense_ref.interleave(5, 4, 3)
    cptr, cidx, cval = dense_ref.mixed_constraints(case.lay, 5, 0.05, 9, mix)
    wptr, widx, wval = dense_ref.problems.random_constraints(case.lay, 5, density=0.05, seed=9)
    sizes = np.diff(cptr)
    w = 0
    for j, kind in enumerate(mix):
        if kind == "w":                                          # the wide ones are the plain recipe's, in its order
            assert np.array_equal(cidx[cptr[j]:cptr[j + 1]], widx[wptr[w]:wptr[w + 1]]) and np.array_equal(cval[cptr[j]:cptr[j + 1]], wval[wptr[w]:wptr[w + 1]])
            w += 1
        else:
            assert sizes[j] == (dense_ref.FEW_ENTRIES if kind == "f" else dense_ref.SINGLE_ENTRIES)
        assert np.all(np.diff(cidx[cptr[j]:cptr[j + 1]]) > 0) and case.low[cidx[cptr[j]:cptr[j + 1]]].all()
    narrow = np.concatenate([cidx[cptr[j]:cptr[j + 1]] for j, kind in enumerate(mix) if kind != "w"])
    assert len(set(narrow.tolist())) == len(narrow)              # no slot twice: no two narrow constraints are dependent
    # neither class is a contiguous range, and the swept list is not the identity prefix
    dl = [j for j, kind in enumerate(mix) if kind == "w"]
    sl = [j for j, kind in enumerate(mix) if kind != "w"]
    assert dl != list(range(len(dl))) and np.any(np.diff(dl) > 1) and np.any(np.diff(sl) > 1)


@pytest.mark.parametrize("key", sorted(all_hybrid_cases()))
def test_recipe_separates_and_stays_at_its_record(key):
    """the classification rule splits the case as its mix says, and the oracle stays within 10 x of its recorded error; the
    record is at most 1 / 100 of the bound the device is held to (the rule of test_new_patterns_against_the_yardstick)"""
    hc = all_hybrid_cases()[key]
    mix = hc["recipe"][3]
    swept, sparse, other, cols, cap = host_classes(hc)
    assert (swept, sparse, other) == (mix.count("w"), len(mix) - mix.count("w"), 0), (swept, sparse, other)
    yard, own = dense_ref.load_yardstick(), dense_ref.load_mix_yardstick()
    assert set(own) == set(all_hybrid_cases())
    errs = oracle_kkt_errors(hc)
    print(key[:70], "columns %d trsm_cap %d" % (cols, cap), " ".join("%s=%.1e" % kv for kv in sorted(errs.items())))
    assert set(errs) == set(KKT_OPS) == set(own[key])
    for op, e in errs.items():
        rec = own[key][op]
        assert e <= 10.0 * rec or e <= yard[op]["value"], (op, e, rec)
        assert 100.0 * rec <= dense_ref.hybrid_bound(key, op, yard, own) <= dense_ref.BOUND_CAP, (op, rec)


def test_chunks_case_passes_the_column_cap():
    """the case that must give two chunks of sparse constraints: the columns of S^-1 its narrow constraints need are more than
    vcols = trsm_cap (classify_columns), and fewer than twice that -- two chunks, the smallest count that has a chunk border"""
    swept, sparse, other, cols, cap = host_classes(dense_ref.HYBRID_CASES["chunks"])
    assert cap < cols <= 2 * cap, (cols, cap)
