"""More than one launch group of wide cliques (ceigw_pass, cone_route / cone_wide_pass; csrc/completions.hip): the split that
happens when the workspace of the wide cliques of a call exceeds tune(symb, TUNE_SLOT_DOUBLES, value) doubles -- 2**25 by
default, which no pattern of the suite reaches.  fam_top under tune(symb, TUNE_CEIG_WIDE, 65) has three wide cliques (130,
130 and 110 rows) whose group workspaces (ceigw_layout) are 46 560 and 32 768 doubles with eigenvectors, 29 664 and 20 672
without, so that the limits 0 / 80 000 (56 000 for clique_eigvalsh) / 1 give 1 / 2 / 3 groups; every count is asserted through
clique_eig_groups.  Every output of every operation under 2 and 3 groups is, bit for bit, that of the one-group run on the
same context, and the one-group run meets the bounds of tests/test_gpu_clique_wide.py / tests/test_gpu_cone_wide.py.  In
cone_project the cliques below 65 rows run k_cone_split from LDS in the same iteration as the groups.

Groups reached: clique_eigvalsh, cone_margin 1 / 2 / 3; clique_eigh, clique_project 1 / 2 / 3; cone_project 1 / 2 / 3 with
the lists remade at every change of the limit.  Wall time on an MI355X: 1.0 s per case of the spectra, 1.6 s per case of cone_project."""
import numpy as np
import pytest
import torch

from helpers import launch_counts
from smcp_amd import chordal
from test_gpu_clique_eig import on_device
from test_gpu_clique_wide import ORTH, PRJ, RES, WIDE, case, check_against_lapack, n_wide
from test_gpu_cone_project import run_steps, start
from test_gpu_cone_wide import against_the_restatement, cone_input, device_symb as cone_symb, same_bits, three_steps
from test_cone_project_host import CONE_UNITS, GPU_FACTOR, PARAMS
from test_gpu_slot_share import LDS, beyond_lds, bits, ceig_slot2
from test_mrcompletion_host import clique_rows

pytestmark = pytest.mark.gpu

WS_VEC = {130: 46560, 110: 32768}                        # ceigw_layout with V (csrc/front_ceigw.hip), doubles
WS_VAL = {130: 29664, 110: 20672}                        # and without
VEC_LIMITS = [(0, 1), (80000, 2), (1, 3)]                # (limit, groups)
VAL_LIMITS = [(0, 1), (56000, 2), (1, 3)]
CW_B, MAX_SWEEPS = 32, 30                                # CW_B, CEIG_MAX_SWEEPS


def wide_orders(symb):
    return [int(nf) for nf in np.diff(np.asarray(symb.rowptr)) if nf >= WIDE]


def groups_of(symb, ws, limit):
    """ceigw_pass / cone_route restated: the wide cliques, ascending, in groups whose workspace stays within the limit"""
    out, doubles = [], 0
    for nf in wide_orders(symb):
        if not out or doubles + ws[nf] > (limit or 2 ** 25):
            out.append([])
            doubles = 0
        out[-1].append(nf)
        doubles += ws[nf]
    return out


def under_limits(symb, run, limits, ws, what):
    """run() under every limit: the restated number of groups, and the bits of the one-group run.  Returns that run."""
    out = []
    try:
        for limit, groups in limits:
            chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
            out.append(run())
            got = chordal.clique_eig_groups(symb)
            assert got == groups == len(groups_of(symb, ws, limit)), "%s at limit %d: %d groups, wanted %d" % (what, limit, got, groups)
            assert chordal.clique_eig_wide(symb) == n_wide(symb) == 3
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    for (limit, groups), o in zip(limits[1:], out[1:]):
        for i, (p, q) in enumerate(zip(out[0], o)):
            assert bits(p) == bits(q), "%s: output %d under %d groups differs from the one-group run" % (what, i, groups)
    return out[0]


@pytest.mark.parametrize("kind", ["definite", "rank3", "indefinite"])
def test_spectra_under_two_and_three_groups(kind):
    symb, blkA, As, eigs = case("fam_top", kind)
    assert sorted(wide_orders(symb)) == [110, 130, 130]
    X = on_device(symb, blkA)
    chordal.tune(symb, chordal.TUNE_CEIG_WIDE, WIDE)
    try:
        w, ext, sweeps = under_limits(symb, lambda: (chordal.clique_eigvalsh(X), chordal.clique_extremes(X), chordal.clique_eig_sweeps(symb)),
                                      VAL_LIMITS, WS_VAL, "clique_eigvalsh " + kind)
        m, k = under_limits(symb, lambda: chordal.cone_margin(X), VAL_LIMITS, WS_VAL, "cone_margin " + kind)
        we, Q, sw = under_limits(symb, lambda: chordal.clique_eigh(X) + (chordal.clique_eig_sweeps(symb),), VEC_LIMITS, WS_VEC, "clique_eigh " + kind)
        Z, wp, info, sp = under_limits(symb, lambda: chordal.clique_project(X, -0.5, 0.5, return_info=True) + (chordal.clique_eig_sweeps(symb),),
                                       VEC_LIMITS, WS_VEC, "clique_project " + kind)
    finally:
        chordal.tune(symb, chordal.TUNE_CEIG_WIDE, 0)
    assert torch.equal(X.blkval.cpu(), torch.from_numpy(blkA))               # the input is not written
    assert torch.equal(w, we) and torch.equal(w, wp) and sweeps == sw == sp <= 30
    assert m == float(ext[0]) and k == int(ext[1])
    worst = check_against_lapack(symb, As, eigs, w, Q, [(-0.5, 0.5, Z, info)])
    for got, bd, name in zip(worst, (16.0, ORTH, RES, PRJ), ("eigenvalues", "orthogonality", "residual", "projection")):
        assert got <= bd, "%s %s: %.2f units, bound %.2f" % (name, kind, got, bd)


@pytest.mark.parametrize("kind", ["noisy", "indef"])
@pytest.mark.parametrize("rho,relax", PARAMS)
def test_cone_project_under_two_and_three_groups(kind, rho, relax):
    symb = cone_symb("fam_top")
    blk = cone_input(symb, kind)
    worst, _ = against_the_restatement("fam_top", kind, rho, relax)            # the one-group run against its bound
    assert worst <= GPU_FACTOR * CONE_UNITS, "cone_project %s: %.2f units, bound %.2f" % (kind, worst, GPU_FACTOR * CONE_UNITS)

    def run(limit, groups, split=False):
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
        out = three_steps(symb, blk, rho, relax, split=split)
        got = chordal.clique_eig_groups(symb)
        assert got == groups == len(groups_of(symb, WS_VEC, limit)), "limit %d: %d groups, wanted %d" % (limit, got, groups)
        assert chordal.clique_eig_wide(symb) == 3
        return out

    try:
        one = run(0, 1)
        assert same_bits(one, run(80000, 2)), "two groups differ from one"
        three = run(1, 3)
        assert same_bits(one, three), "three groups differ from one"
        assert same_bits(one, run(1, 3, split=True)), "1 + 2 steps under three groups are not the 3 of one call"
        assert same_bits(one, run(0, 1)), "0 -> 1 -> 0: the lists were not made again"
        assert same_bits(one, run(80000, 2, split=True))
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
    assert torch.equal(one[0].blkval.cpu(), torch.from_numpy(np.array(blk)))


def chain(symb, limit):
    """launches of one iteration under KID_ceig_reduce and KID_ceig: per group the chain of section 23 of DESIGN.md -- a check
    before each of 30 block sweeps and one behind; form, begin, (pivot, apply) per step of every sweep, sort, split, finish --
    plus k_cone_resid, plus one k_cone_split per LDS class that holds a clique"""
    reduce_, ceig = 1, 0
    for g in groups_of(symb, WS_VEC, limit):
        nb = max(-(-nf // CW_B) for nf in g)
        steps = nb + (nb & 1) - 1
        reduce_ += MAX_SWEEPS + 1
        ceig += 2 + MAX_SWEEPS * 2 * steps + 3
    narrow = [ceig_slot2(int(nf)) for nf in np.diff(np.asarray(symb.rowptr)) if nf < WIDE]
    assert narrow and not any(beyond_lds(s) for s in narrow)               # k_cone_split runs, and from LDS only
    classes = [8192, 16384, 32768, 65536, LDS]
    split = len({min(c for c in classes if s * 8 <= c) for s in narrow})
    assert split >= 1
    ceig += split
    return reduce_, ceig


def test_launch_chain_is_the_sum_over_the_groups_and_does_not_depend_on_the_data():
    symb = cone_symb("fam_top")
    try:
        for limit, groups in VEC_LIMITS:
            chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, limit)
            counts = {}
            for kind in ("incone", "indef"):
                a, x, U, W = start(symb, cone_input(symb, kind))
                hist = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
                run_steps(symb, a, x, U, W, 1.0, 1.7, 0, 1, hist)                 # warm: the lists of this limit
                counts[kind] = launch_counts(symb, lambda: run_steps(symb, a, x, U, W, 1.0, 1.7, 1, 1, hist))
            assert chordal.clique_eig_groups(symb) == groups
            assert counts["incone"] == counts["indef"]
            want = chain(symb, limit)
            got = (counts["indef"]["k_ceig_reduce"], counts["indef"]["k_ceig"])
            assert got == want, "limit %d: (k_ceig_reduce, k_ceig) launches %s, chain formula %s" % (limit, got, want)
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)


def test_non_finite_entry_in_one_wide_clique_under_three_groups():
    symb = cone_symb("fam_top")
    blk = cone_input(symb, "noisy")
    nf = np.diff(np.asarray(symb.rowptr))
    kw = [k for k in range(symb.Nsn) if nf[k] == 130][1]                      # the second group of three
    bad = np.array(blk)
    at = symb.blkptr[kw] + 5                                                  # row 5, column 0 of that clique's own block
    bad[at] = np.nan
    r, c = clique_rows(symb, kw)[5], clique_rows(symb, kw)[0]
    holders = [k for k in range(symb.Nsn) if r in clique_rows(symb, k) and c in clique_rows(symb, k)]
    try:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
        clean = three_steps(symb, blk, 1.0, 1.7)
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 1)
        with pytest.raises(RuntimeError, match="did not converge") as e:
            chordal.cone_project(on_device(symb, bad))
        assert chordal.clique_eig_groups(symb) == 3
        named = int(str(e.value).split("clique ")[1].split()[0])
        assert named in holders and "at iteration 1 " in str(e.value), (named, holders, str(e.value))
        assert same_bits(clean, three_steps(symb, blk, 1.0, 1.7)), "the call after the NaN is not the clean run"
        assert chordal.clique_eig_groups(symb) == 3
    finally:
        chordal.tune(symb, chordal.TUNE_SLOT_DOUBLES, 0)
