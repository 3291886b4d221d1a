"""GPU: the hybrid Schur route against the DENSE definitions (tests/dense_ref.py), at the dense bound, kkt_x per clique.

The hybrid route is schur_gram (kkt.hip) with swept AND column-sparse constraints in one system: the swept SUBSET goes through
the Hessian (hess_up_fast with ids = D.dlist: every sparse-input kernel reads its right-hand side r as constraint kc_ids[kc_j0 + r],
k_leaf_pairs takes D.lg_remap, gram_accumulate writes D.hd with leading dimension md, k_scatter_hd places it in H) and the others
take the SCMcolumn2 columns (k_unit_columns, two triangular solves, k_scm_columns).  The inputs are the mixed recipes of
dense_ref.HYBRID_CASES: wide, few-entry and single-entry constraints dealt in turn, so neither class is a contiguous range and the
swept list is not the identity prefix; an index slip (r for ids[r], md for m) moves a column of H and fails kkt_H.

Every case sets tnzcols itself and ASSERTS the device's classification (dense_ref.device_kkt: swept = the wide ones, sparse = the
others), and states the launch census beside its errors: k_scatter_hd, k_scm_columns and k_unit_columns ran.

Bound per operation (dense_ref.hybrid_bound): 100 x the larger of the global yardstick value and the oracle-vs-dense error
recorded for that (pattern, recipe) in tests/golden/hybrid_recipe_yardstick.json, never looser than 1e-12.  No other tolerance.

Chunks of sparse constraints.  A factor runs more than one k_scm_columns launch when the columns of S^-1 its sparse constraints
need, sum |K_s|, exceed vcols = trsm_cap = max_rhs * (2 blklen + 256 nsn) / sum(separator sizes) (constraints.cpp
classify_columns; tmplen from setup.hip).  Per right-hand side of max_rhs that is 69 columns on nested, 118 on rand2, 82 on arrow,
29 on fam_odd, 57 on nested_mid, 246 on arrow_big, 68 on arrow_thin: fam_odd is the smallest, and with max_rhs = 4 (the smallest
context the suite makes) its cap is 117 columns.  A single-entry constraint needs two columns (one on the diagonal), so 70 of
them need about 135 > 117: two chunks, which tests/test_hybrid_recipes.py holds on a CPU from the same formula.

Measured device-vs-dense worst cases (MI355X, every case of this file), against the bound in force for that recipe:

    operation   device worst   bound      worst case
    kkt_H       6.6e-16        2.3e-13    arrow_big (the parts summed on the host: 2.6e-16, nparts = 2)
    kkt_x       3.1e-15        2.4e-13    gram130 (130 swept + 3 sparse on nested; the seven patterns: 1.2e-15, nested_mid)
    kkt_y       1.6e-15        4.9e-13    gram130 (the seven patterns: 1.3e-15, nested_mid)

The hybrid route is as close to the dense definitions as the CPU oracle is on the same inputs (record: kkt_H 1.7e-15, kkt_x
2.4e-15, kkt_y 2.5e-15 over all mixed recipes).  No bound was exceeded and none was raised; the one bound above the global
yardstick's is kkt_x on gram130, by that recipe's own record.  Census: k_scatter_hd, k_unit_columns and k_scm_columns once per
factor (twice each of the latter two in the chunks case); k_leaf_pairs in every case but arrow_big, arrow_thin and gram130, with
or without TUNE_LEAFGRAM = 2.  The 18 cases take 4 s together.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from smcp_amd import chordal
from smcp_amd.symbolic import Symbolic
from tests import dense_ref
from tests.helpers import GPU_PATTERNS, kernel_census

pytestmark = pytest.mark.gpu
SEVEN = ["nested", "rand2", "arrow", "fam_odd", "nested_mid", "arrow_big", "arrow_thin"]
FAMILY = ["nested", "fam_odd", "nested_mid"]                 # of the seven: trees with small parents of childless children
EDGES = ["md1", "ns1", "two_blocks", "gram130", "ends"]
ROUTE_KERNELS = ("k_scatter_hd", "k_scm_columns", "k_unit_columns")


@pytest.fixture(scope="module")
def yards():
    return dense_ref.load_yardstick(), dense_ref.load_mix_yardstick()


@pytest.fixture(scope="module")
def contexts():
    """(pattern, max_rhs) -> (Symbolic with a device context, DenseCase), made once per module; the dense reference of a recipe
    is formed once and kept while the cases that follow use the same recipe"""
    cache = {}

    def get(hc):
        key = (hc["pattern"], hc["max_rhs"])
        if key not in cache:
            pat = GPU_PATTERNS[hc["pattern"]]()
            symb = Symbolic(pat)
            symb.device_init(0, hc["max_rhs"])
            cache[key] = (symb, dense_ref.DenseCase(pat, orc.Sym(symb), dense_ref.YARDSTICK_SEED))
        symb, case = cache[key]
        if case.kkt_recipe != hc["recipe"]:
            case.kkt_recipe, case._kkt = hc["recipe"], None
        return symb, case

    return get


def classes_of(hc):
    mix = hc["recipe"][3]
    return mix.count("w"), len(mix) - mix.count("w")


def launched(census, name):
    """launches of a kernel function over its instantiations"""
    return sum(v for k, v in census.items() if k.split("<")[0] == name)


def check(tag, hc, errs, census, yards, route=True):
    key = dense_ref.recipe_key(hc["pattern"], hc["recipe"])
    print("HYBRID", tag, " ".join("%s=%.2e" % kv for kv in sorted(errs.items())),
          " ".join("%s=%d" % (k, launched(census, k)) for k in ROUTE_KERNELS + ("k_leaf_pairs", "k_fam_terms", "k_gram_partial")))
    bad = {op: (e, dense_ref.hybrid_bound(key, op, *yards)) for op, e in errs.items() if not e <= dense_ref.hybrid_bound(key, op, *yards)}
    assert not bad, (tag, bad)
    if route:
        missing = [k for k in ROUTE_KERNELS if not launched(census, k)]
        assert not missing, (tag, "did not run", missing)


def run(name, contexts, tnzcols=None, classes=None):
    """(case table entry, errors against the dense definitions, census of the factorisation and the two solves)"""
    hc = dense_ref.HYBRID_CASES[name]
    symb, case = contexts(hc)
    kkt = dense_ref.device_kkt(symb, tnzcols=hc["tnzcols"] if tnzcols is None else tnzcols, max_rhs=hc["max_rhs"],
                               classes=classes or classes_of(hc))
    box = {}
    census = kernel_census(symb, lambda: box.update(errs=dense_ref.kkt_errors(case, kkt)))
    return hc, box["errs"], census


@pytest.mark.parametrize("name", SEVEN)
def test_seven_patterns_against_dense(name, contexts, yards):
    """4 few + 3 single constraints dealt among the wide ones of the pattern's recipe; all wide ones in one block of right-hand sides"""
    hc, errs, census = run(name, contexts)
    check(name, hc, errs, census, yards)


@pytest.mark.parametrize("name", FAMILY)
def test_family_patterns_closed_form_gram(name, contexts, yards):
    """TUNE_LEAFGRAM = 2: the children's Gram blocks in closed form, for the swept subset through D.lg_remap (k_leaf_pairs)"""
    symb, _ = contexts(dense_ref.HYBRID_CASES[name])
    chordal.tune(symb, chordal.TUNE_LEAFGRAM, 2)
    try:
        hc, errs, census = run(name, contexts)
    finally:
        chordal.tune(symb, chordal.TUNE_LEAFGRAM, 1)
    check(name + " leafgram", hc, errs, census, yards)
    assert launched(census, "k_leaf_pairs") >= 1, sorted(census)


@pytest.mark.parametrize("name", EDGES)
def test_class_size_edges(name, contexts, yards):
    """md = 1; ns = 1; five swept on max_rhs = 4 (two blocks of the sweep into one D.hd); md = 130 > GRAM_BLK (the blocked Gram
    kernels writing with leading dimension md); a swept constraint at index 0 and one at index m - 1"""
    hc, errs, census = run(name, contexts)
    check(name, hc, errs, census, yards)
    if name == "gram130":
        assert launched(census, "k_gram_partial") >= 1, sorted(census)


def test_several_chunks_of_sparse_constraints(contexts, yards):
    """70 single-entry constraints on fam_odd with max_rhs = 4: more columns of S^-1 than vcols (module docstring), so ONE factor
    launches k_unit_columns and k_scm_columns at least twice; the chunk offsets (voff, slist + q0) are then not zero"""
    hc, errs, census = run("chunks", contexts)
    check("chunks", hc, errs, census, yards)
    assert launched(census, "k_scm_columns") >= 2 and launched(census, "k_unit_columns") >= 2, census


def test_parts_on_one_context(contexts, yards):
    """kkt_schur_gram_part(part, nparts) for every part on ONE context, summed on the host: the dense H in both triangles; part 0
    alone holds the swept block; with nparts = ns + 2 some parts have an empty share.  Two sparse constraints of different parts
    share a column (asserted), so an entry of H is owed to two owners: written by both it would be twice the dense value."""
    from smcp_amd.kkt import KKTSystem
    hc = dense_ref.HYBRID_CASES["nested"]
    symb, case = contexts(hc)
    k = case.kkt()
    mix = hc["recipe"][3]
    dl = [j for j, kind in enumerate(mix) if kind == "w"]
    sl = [j for j, kind in enumerate(mix) if kind != "w"]
    ns = len(sl)
    cptr, cidx, _ = k.con
    cols = []
    for j in sl:                                                 # rows / columns a sparse constraint touches
        u = np.zeros(case.S.blklen)
        u[cidx[cptr[j]:cptr[j + 1]]] = 1.0
        cols.append(set(np.flatnonzero(case.S.dense(u).any(axis=0)).tolist()))
    sysk = KKTSystem(symb, *k.con, max_rhs=hc["max_rhs"], tnzcols=hc["tnzcols"])
    assert dense_ref.constraint_classes(sysk) == (len(dl), ns)
    L, Y = dense_ref.to_dev(symb, case.cholesky()), dense_ref.to_dev(symb, case.Yblk)
    key = dense_ref.recipe_key(hc["pattern"], hc["recipe"])
    bound = dense_ref.hybrid_bound(key, "kkt_H", *yards)
    for nparts in (2, 3, ns + 2):
        owner = {}
        for p in range(nparts):
            for q in range(ns * p // nparts, ns * (p + 1) // nparts):
                owner[q] = p
        shared = [(a, b) for a in range(ns) for b in range(a + 1, ns) if owner[a] != owner[b] and cols[a] & cols[b]]
        assert shared, "no two sparse constraints of different parts share a column (nparts = %d)" % nparts
        total, empty = np.zeros_like(k.H), 0
        box = {}

        def parts():
            for part in range(nparts):
                sysk.H.zero_()
                sysk._scm_part(L, Y, part, nparts)
                box[part] = sysk.H.cpu().numpy().T.copy()        # device H is column-major m x m

        census = kernel_census(symb, parts)
        for part in range(nparts):
            Hp = box[part]
            total += Hp
            share = ns * (part + 1) // nparts - ns * part // nparts
            if part == 0:
                assert dense_ref.relvec(Hp[np.ix_(dl, dl)], k.H[np.ix_(dl, dl)]) <= bound
            else:
                assert not Hp[np.ix_(dl, dl)].any(), "part %d of %d wrote the swept block" % (part, nparts)
            if share == 0:
                empty += 1
                assert part == 0 or not Hp.any(), "part %d of %d has no share and wrote H" % (part, nparts)
        errs = {"kkt_H": max(dense_ref.relvec(np.tril(total), np.tril(k.H)), dense_ref.relvec(np.triu(total), np.triu(k.H)))}
        worst = np.abs(total - k.H).max() / np.abs(k.H).max()
        print("HYBRID parts nparts=%d kkt_H=%.2e worst entry %.2e shared pairs %d empty shares %d" % (nparts, errs["kkt_H"], worst, len(shared), empty),
              " ".join("%s=%d" % (kk, launched(census, kk)) for kk in ROUTE_KERNELS))
        assert errs["kkt_H"] <= bound, (nparts, errs, bound)
        assert (empty >= 2) == (nparts == ns + 2)
        # the swept block once (part 0), one chunk of columns per part with a share
        assert launched(census, "k_scatter_hd") == 1 and launched(census, "k_scm_columns") == nparts - empty, census


def test_result_does_not_depend_on_the_class(contexts, yards):
    """the same mixed input with every constraint swept (tnzcols = 0) and with all but one sparse (tnzcols just below what the
    widest constraint touches), each against the same dense H, x and y"""
    hc = dense_ref.HYBRID_CASES["nested"]
    symb, case = contexts(hc)
    m = len(hc["recipe"][3])
    _, errs, census = run("nested", contexts, tnzcols=0.0, classes=(m, 0))
    check("all swept", hc, errs, census, yards, route=False)
    assert not launched(census, "k_scatter_hd") and not launched(census, "k_scm_columns")
    t = sorted(dense_ref.touched(case.S, case.kkt().con))
    assert t[-1] > t[-2]                                         # one widest constraint
    tnz = (t[-2] + 0.5) / case.S.n
    assert int(case.S.n * tnz) == t[-2]
    _, errs, census = run("nested", contexts, tnzcols=tnz, classes=(1, m - 1))
    check("all but one sparse", hc, errs, census, yards)
