"""Unit terms of the fused extend-add (front_famt.hip, lf_add_family).  A constraint entry whose term has a unit vector of
the parent's separator part, s (a_d e_u^T + e_u a_d^T), goes to the update by one ds_add_f64 per lane, without a product;
the host orders every static term list dense terms first (constraints.cpp).  k_fam_terms reads the entry lists, not these
term lists, and is unchanged.  The constraints here are built by hand from the positions of the families, one list shape
per constraint:

  0  parent separator-row entries only: every list has unit terms only (no accumulator tile, no scatter)
  1  dense terms only: parent block, child blocks (diagonals included), child separator rows that land in the parent's block
  2  entries in every other family only: empty lists beside mixed ones
  3  one dense term and 20 unit terms: the load batches of the unit phase wrap
  4  more than 64 terms, the 64th among the dense terms (a band of the pattern plus separator-row entries)
  5  more than 64 terms, the 64th among the unit terms
  6  unit terms on a -K column (parent separator row) and on a child column (child separator row outside the parent's block)
  7  several unit terms of one list with the same unit vector u (LDS adds into one row and column)

Every unit term also hits the doubled (u, u) element of the update -- lane u adds 2 s a_d[u] -- which is the likeliest
error of the unit phase; shapes 0, 3 and 7 check nothing else as hard.  Lanes beyond na: fam_top and fam_odd have parents
of (7, 33) -- na is no multiple of 16 and below 64; nested_mid has (15, 64) parents, and nested_mid16 is nested_mid with
(16, 64) parents: nn = 16.

fam_odd cannot take the fused extend-add whatever its constraints are: its families hang under top fronts of (20, 30), which
are no large fronts, and the static term lists exist only under large fronts (constraints.cpp, number_families; the long-list
test of test_gpu_parity.py expects the same of it).  There the family sweep forms the update tiles itself
(k_fam_terms<NAT, true>) and the case checks that the reordered lists leave that route alone; the (7, 33) parents of
fam_top go through the fused route.

H, x, y against the oracle at 1e-9 with the helpers and tolerances of test_family_updates_formed_by_the_extend_add, the
launch counters say which kernels ran, and the factor of H of the same problem with the closed-form leaf route off
(TUNE_LEAFGRAM 0: the unfused reference, packed updates through HBM) agrees at 1e-12."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import chordal, problems
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic
from tests.helpers import GPU_PATTERNS
from tests.test_gpu_parity import _band_constraint, _launch_counts, dev, host, lowmask, rel

pytestmark = pytest.mark.gpu


def _families(symb):
    """per family parent: (k, nn, na, children [(c, nnc, nac, rel)])"""
    roles = symb.family_roles()
    nn, na = symb.clique_sizes()
    out = []
    for k in np.nonzero(roles == 2)[0]:
        ch = []
        for c in symb.chidx[symb.chptr[k]:symb.chptr[k + 1]]:
            ch.append((int(c), int(nn[c]), int(na[c]), symb.relidx[symb.sepptr[c]:symb.sepptr[c] + na[c]].astype(np.int64)))
        out.append((int(k), int(nn[k]), int(na[k]), ch))
    return out


def _classes(symb, fam):
    """blkval positions of a family by the class of their term: dense (parent block, child blocks, child separator rows inside
    the parent's block), unit on a -K column (parent separator rows), unit on a child column (with the unit index u)"""
    k, nn, na, ch = fam
    nf = nn + na
    b = int(symb.blkptr[k])
    dense = [b + j * nf + i for j in range(nn) for i in range(j, nn)]
    unit_own = [(b + j * nf + nn + a, a) for a in range(na) for j in range(nn)]
    unit_child = []
    for c, nnc, nac, relc in ch:
        nfc = nnc + nac
        bc = int(symb.blkptr[c])
        dense += [bc + j * nfc + i for j in range(nnc) for i in range(j, nnc)]
        for a in range(nac):
            for j in range(nnc):
                p = bc + j * nfc + nnc + a
                if relc[a] < nn:
                    dense.append(p)
                else:
                    unit_child.append((p, int(relc[a]) - nn))
    return dense, unit_own, unit_child


def _hand_constraints(symb, m, rng):
    fams = _families(symb)
    assert fams
    shapes = [dict() for _ in range(8)]
    stats = dict(dense_boundary=0, unit_boundary=0, child_unit=0, same_u=0)
    band = dict(zip(*[x.tolist() for x in _band_constraint(symb, 1, rng)]))
    for f, fam in enumerate(fams):
        dense, uown, uchild = _classes(symb, fam)
        k, nn, na, ch = fam
        pick = lambda seq, n: [seq[i] for i in sorted(rng.choice(len(seq), size=min(n, len(seq)), replace=False))] if seq else []
        shapes[0].update((p, 1) for p, _ in pick(uown, 5))
        shapes[1].update((p, 1) for p in pick(dense, 12))
        shapes[1][dense[0]] = 1                                          # a diagonal entry of the parent (v / 2)
        if f % 2 == 0:
            shapes[2].update((p, 1) for p in pick(dense, 3) + [p for p, _ in pick(uown, 4) + pick(uchild, 3)])
        shapes[3].update((p, 1) for p in pick(dense, 1) + [p for p, _ in pick(uown, 20)])
        # (the band's entries inside the family are dense terms: block entries next to the diagonal)
        mine = set(dense)
        long_dense = [p for p in band if p in mine] + pick(dense, 40)
        long_dense = sorted(set(long_dense))[:80]
        shapes[4].update((p, 1) for p in long_dense + [p for p, _ in pick(uown, 6) + pick(uchild, 4)])
        stats["dense_boundary"] += len(long_dense) > 64
        nd5 = len(pick(dense, 10))
        u5 = pick(uown, 70) + pick(uchild, 10)
        shapes[5].update((p, 1) for p in pick(dense, 10) + [p for p, _ in u5])
        stats["unit_boundary"] += nd5 < 64 < nd5 + len(u5)
        shapes[6].update((p, 1) for p, _ in pick(uown, 2) + pick(uchild, 2))
        stats["child_unit"] += len(uchild) > 0
        # the same u: a whole separator row of the parent (nn entries) and, where there is one, a child row with that u
        a0 = int(rng.integers(na))
        same = [p for p, u in uown if u == a0] + [p for p, u in uchild if u == a0][:3]
        shapes[7].update((p, 1) for p in same)
        stats["same_u"] += len(same) >= 2
    rc = problems.random_constraints(symb, m, density=0.002, seed=7)
    cols = [(rc[1][rc[0][j]:rc[0][j + 1]], rc[2][rc[0][j]:rc[0][j + 1]]) for j in range(m)]
    # the shapes sit among the sparse constraints, the two long ones apart from each other
    for s, j in enumerate([1, 4, 6, 9, 3, 17, 12, 14]):
        pos = np.array(sorted(shapes[s]), dtype=np.int64)
        cols[j] = (pos, rng.standard_normal(len(pos)))
    cptr = np.concatenate([[0], np.cumsum([len(p) for p, _ in cols])]).astype(np.int64)
    cidx = np.concatenate([p for p, _ in cols]).astype(np.int64)
    cval = np.concatenate([v for _, v in cols])
    return cptr, cidx, cval, stats


_PATTERNS = dict(GPU_PATTERNS)
_PATTERNS["nested_mid16"] = lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=6, nleaf_per_mid=8, mid=(16, 64), seed=3)


# name, whether the families hang under fronts the fused extend-add takes (see above)
@pytest.mark.parametrize("name,fused", [("nested_mid", True), ("fam_top", True), ("fam_odd", False), ("nested_mid16", True)])
def test_unit_terms_of_the_family_sweep(name, fused):
    symb = Symbolic(_PATTERNS[name]())
    symb.device_init(0, 4)
    S = orc.Sym(symb)
    A = problems.random_factor_blkval(symb, 71)
    orc.llt(S, A)
    msk = lowmask(symb)
    rng = np.random.default_rng(72)
    m = 24                                             # two top fronts x 24: the fused route wants 32 (front, right-hand side) pairs
    L = A.copy()
    orc.cholesky(S, L)
    Yh = L.copy()
    orc.projected_inverse(S, Yh)
    cptr, cidx, cval, stats = _hand_constraints(symb, m, rng)
    print(name, "families", len(_families(symb)), stats, "entries", len(cidx), "cliques", symb.Nsn)
    assert stats["unit_boundary"] > 0 and stats["child_unit"] > 0 and stats["same_u"] > 0
    if name.startswith("nested_mid"):
        assert stats["dense_boundary"] > 0
    K = orc.KKT(S, cptr, cidx, cval)
    Href = K.schur_factor(L, Yh)
    bx = rng.standard_normal(symb.blklen) * msk
    by = rng.standard_normal(m)
    xr, yr = K.solve(L, Yh, Href, bx, by, 0.5)
    sys_ = KKTSystem(symb, cptr, cidx, cval, max_rhs=m, tnzcols=0.0)
    Hs, routes = {}, {}
    try:
        for leafgram in (2, 0):
            chordal.tune(symb, chordal.TUNE_LEAFGRAM, leafgram)
            Ld, Yd = dev(symb, L), dev(symb, Yh)
            box = {}
            counts = _launch_counts(symb, lambda: box.setdefault("solve", sys_.factor(Ld, Yd)))
            print(name, "leafgram", leafgram, {k: v for k, v in counts.items() if k in ("k_lf_assemble_fz", "k_fam_terms", "k_fam_terms_grp", "k_fam_sparse", "k_lf_assemble_lds")})
            routes[leafgram] = counts
            Hs[leafgram] = np.tril(sys_.H.cpu().numpy().T)
            eh = rel(Hs[leafgram], np.tril(Href))
            bxd, byd = dev(symb, bx), torch.from_numpy(by.copy()).cuda()
            box["solve"](bxd, byd, 0.5)
            ex, ey = rel(host(bxd)[msk], xr[msk]), rel(byd.cpu().numpy(), yr)
            print(name, "leafgram", leafgram, "rel err H %.2e x %.2e y %.2e" % (eh, ex, ey))
            assert eh < 1e-9 and ex < 1e-9 and ey < 1e-9
    finally:
        chordal.tune(symb, chordal.TUNE_LEAFGRAM, 1)
    assert routes[2].get("k_fam_terms", 0) >= 1, routes[2]
    assert (routes[2].get("k_lf_assemble_fz", 0) >= 1) == fused, routes[2]
    assert routes[0].get("k_lf_assemble_fz", 0) == 0, routes[0]
    e2 = rel(Hs[2], Hs[0])
    print(name, "fused against unfused: rel err H %.2e" % e2)
    assert e2 < 1e-12
