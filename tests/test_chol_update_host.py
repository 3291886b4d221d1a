"""The numpy restatement of chol_update (tests/chol_update_ref.py) against numpy.linalg.cholesky of the dense matrix, on the
structures of oracle/symbolic_ref.py, and chordal.clique_support against a search over the row lists.  No device.

Bounds.  eta = |P_V(L' L'^T - M)|_F / |M|_F is held against the same eta of numpy.linalg.cholesky(M), floored at n eps, times
GATE = 16: a rank-one step is backward stable with a constant of a few units per touched entry, and an entry of L is touched
by at most k + 1 <= 18 steps here against the n / 3 of a Cholesky factorisation, so a factor of 16 over the floor is ample.
The factor itself is held against numpy's by Sun's first-order bound for the Cholesky factor,
|dL|_F / |L|_2 <= cond(M) |dM|_F / |M|_2 / sqrt 2, with |dM| the sum of the two backward errors."""
import numpy as np
import pytest

from oracle.symbolic_ref import symbolic_ref
from smcp_amd import chordal
from smcp_amd.symbolic import Symbolic
from tests import chol_update_ref as R
from tests.helpers import EXTRA, GPU_PATTERNS, edges_of, symb_of

NAMES = ("band", "arrow", "nested", "rand1", "rand2", "dense", "diag", "two_components")
GATE = 16.0
REF = {}


def pattern(name):
    return (GPU_PATTERNS.get(name) or EXTRA[name])()


def ref_case(name):
    """(structures of symbolic_ref, blkval, dense Ld, mask): built once per pattern, left unchanged"""
    if name not in REF:
        pat = pattern(name)
        S = symbolic_ref(pat[0], edges_of(pat))
        blk, Ld = R.random_factor(S, seed=5)
        REF[name] = (S, blk, Ld, R.pattern_mask(S))
    return REF[name]


@pytest.mark.parametrize("name", NAMES)
def test_walk_against_dense_cholesky(name):
    S, blk, Ld, mask = ref_case(name)
    n = Ld.shape[0]
    assert np.array_equal(np.tril(Ld) != 0, np.tril(mask))           # the factor fills its pattern: nothing is hidden
    for k, signs in ((1, "plus"), (1, "minus"), (7, "mixed"), (17, "mixed"), (17, "minus"), (64, "mixed")):
        V = R.unit_columns(Ld, R.support_columns(S, k, 100 + k, leaves_first=True))
        a = R.coefficients(k, 200 + k, signs)
        M = R.dense_M(Ld, V, a)
        before = blk.copy()
        new = R.walk(S, blk, V, a)
        assert np.array_equal(before, blk, equal_nan=True)           # the input is not written
        Ln = R.dense_factor(S, new)
        Lc = np.linalg.cholesky(M)
        yard = R.yardstick(mask, M)
        e = R.eta(mask, Ln, M)
        fwd = np.linalg.norm(Ln - Lc) / np.linalg.norm(Lc, 2)
        bound = np.linalg.cond(M) * (e + yard) * np.sqrt(n) / np.sqrt(2.0)     # (eta is a Frobenius ratio: |M|_F <= sqrt n |M|_2)
        print("%s k=%d %s: eta %.2e, numpy %.2e, ratio %.2f; |L' - chol M| / |chol M| %.2e (bound %.2e)" % (name, k, signs, e, yard, e / yard, fwd, bound))
        assert e <= GATE * yard, (name, k, signs, e, yard)
        assert fwd <= bound, (name, k, signs, fwd, bound)
        # nothing outside the union of the paths, and nothing above the diagonals, is written
        touched = R.path_union(S, V, a)
        blkptr = R.arr(S, "blkptr")
        for s in range(len(blkptr) - 1):
            if s not in touched:
                assert np.array_equal(new[blkptr[s]:blkptr[s + 1]], blk[blkptr[s]:blkptr[s + 1]], equal_nan=True), (name, s)
        assert np.array_equal(np.isnan(new), np.isnan(blk))


@pytest.mark.parametrize("name", NAMES)
def test_equals_successive_rank_one_walks_bit_for_bit(name):
    S, blk, Ld, _ = ref_case(name)
    for k, signs in ((7, "mixed"), (17, "mixed"), (33, "plus")):
        V = R.unit_columns(Ld, R.support_columns(S, k, 300 + k))
        a = R.coefficients(k, 400 + k, signs)
        a[2::5] = 0.0                                                # left out
        one = R.walk(S, blk, V, a)
        many = R.rank_one_walks(S, blk, V, a)
        assert np.array_equal(one, many, equal_nan=True), (name, k, signs)
        keep = np.flatnonzero(a)
        assert np.array_equal(one, R.walk(S, blk, V[:, keep], a[keep]), equal_nan=True)


def test_round_trip_and_errors_of_the_restatement():
    S, blk, Ld, mask = ref_case("nested")
    V = R.unit_columns(Ld, R.support_columns(S, 7, 1))
    a = R.coefficients(7, 2, "plus")
    back = R.walk(S, R.walk(S, blk, V, a), V, -a)
    M = Ld @ Ld.T
    assert R.eta(mask, R.dense_factor(S, back), M) <= GATE * R.yardstick(mask, M)
    bad = np.zeros(7)
    bad[3] = -2.0                                                    # 1 + a |L^-1 v|^2 = -1
    with pytest.raises(R.NotPositiveDefinite) as err:
        R.walk(S, blk, V, bad)
    assert err.value.column == 3
    out = V.copy()
    s = R.support_clique(S, V[:, 2])
    outside = sorted(set(range(Ld.shape[0])) - set(R.clique_rows(S, s).tolist()) - set(range(int(np.flatnonzero(V[:, 2])[0]))))
    out[outside[0], 2] = 1.0
    with pytest.raises(ValueError):
        R.walk(S, blk, out, a)


@pytest.mark.parametrize("name", NAMES + ("arrow_thin", "fam_odd"))
def test_clique_support_against_the_search(name):
    symb = symb_of(name) if name in GPU_PATTERNS else Symbolic(pattern(name))
    rng = np.random.default_rng(17)
    n, nsn = symb.n, symb.Nsn
    snptr = symb.snptr
    seen = {"hit": 0, "sep_only": 0, "none": 0}
    sets = []
    for s in range(nsn):
        rows = R.clique_rows(symb, s)
        nn = int(snptr[s + 1] - snptr[s])
        for _ in range(4):
            t0 = int(rng.integers(nn))
            extra = rows[t0 + 1:][rng.random(len(rows) - t0 - 1) < 0.5]
            sets.append(("hit", s, np.concatenate([[rows[t0]], extra])))
        if len(rows) > nn:                                           # inside the rows of clique s, but the minimum is not in N_s
            sets.append(("sep_only", s, rows[nn:]))
            sets.append(("sep_only", s, rows[nn:nn + 1]))
    for _ in range(50):                                              # random sets: mostly inside no clique
        sets.append(("none", -1, rng.choice(n, size=min(n, int(rng.integers(1, 5))), replace=False)))
    for kind, s, idx in sets:
        got = chordal.clique_support(symb, idx)
        want = R.clique_support_brute(symb, idx)
        assert got == want, (name, kind, s, idx, got, want)
        if kind == "hit":
            assert got == s
        if kind == "sep_only":
            assert got != s                                          # another clique (an ancestor) or none
        seen[kind] += 1
        assert got == chordal.clique_support(symb, idx[::-1])        # the order of the indices does not matter
    assert seen["hit"] and seen["none"]
    assert chordal.clique_support(symb, []) == -1
    assert chordal.clique_support(symb, [n]) == -1 and chordal.clique_support(symb, [-1]) == -1
    assert chordal.clique_support(symb, [0]) == 0                    # column 0 belongs to clique 0


def test_a_set_inside_no_clique():
    symb = symb_of("band")                                           # bandwidth 3: rows 0 and 10 share no clique
    assert chordal.clique_support(symb, [0, 10]) == -1 == R.clique_support_brute(symb, [0, 10])
    assert chordal.clique_support(symb, [0, 3]) == 0
    symb = symb_of("arrow")                                          # two leaves of the arrow meet only through the separator
    a, b = R.clique_rows(symb, 0), R.clique_rows(symb, 1)
    assert chordal.clique_support(symb, [a[0], b[0]]) == -1
