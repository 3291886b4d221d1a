"""KKTSystem.residual_many / residual / refine_many (kkt_residual_many, kkt_update_many): the kkt_res of the reference
(solvers.py:401-411) and its refinement rounds (358-367) for a block -- the rows against the oracle and against the composition
the drivers use, the residuals of block solutions, what refinement gains on a perturbed factor, determinism and isolation of the
rows, launch counts, the ledger, refusals and the deferred status regime."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from smcp_amd import _lib, chordal, problems, shard
from smcp_amd.cspmatrix import cspmatrix
from smcp_amd.kkt import KKTSystem
from smcp_amd.symbolic import Symbolic
from tests.helpers import GPU_PATTERNS, launch_counts
from tests.test_gpu_parity import dev, rel, setup
from tests.test_gpu_solve_many import SENT, _padded
from tests.test_gpu_solve_many_qr import _device_case as _qr_device_case
from tests.test_gpu_solve_many_qr import _same_bits

pytestmark = pytest.mark.gpu

RES_KERNELS = ("k_res_combine", "k_res_y", "k_res_norms")
NEW_KERNELS = RES_KERNELS + ("k_kkt_many_sub",)          # (k_res_inv_table runs once per constraint set)


def _normalised(norms):
    """the two residual columns, each over max(1, the matching ||b|| column): the normalisation of test_kkt_factor_and_solve"""
    n = norms.cpu().numpy().reshape(-1, 4)
    return np.stack([n[:, 0] / np.maximum(1.0, n[:, 2]), n[:, 1] / np.maximum(1.0, n[:, 3])], axis=1).reshape(norms.shape[:-1] + (2,))


# ---- 1. rows against the oracle ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    """the factors of test_kkt_factor_and_solve, nine random rows and the oracle's residuals of them for both kk: computed once
    per pattern, shared by the two max_rhs, never written to"""
    m = 7
    symb, S, A, msk = setup(name, 7)
    L = A.copy()
    orc.cholesky(S, L)
    Yh = L.copy()
    orc.projected_inverse(S, Yh)
    cons = problems.random_constraints(symb, m, density=0.05, seed=9)
    K = orc.KKT(S, *cons)
    rng = np.random.default_rng(8)
    bl = symb.blklen
    XSh = rng.standard_normal((9, bl)) * msk
    YSh = rng.standard_normal((9, m))
    BXh = rng.standard_normal((9, bl))               # (unmasked: what the slots above the diagonal hold must not reach a norm)
    BYh = rng.standard_normal((9, m))
    refs = {kk: [K.residual(L, Yh, XSh[r], YSh[r], BXh[r], BYh[r], kk) for r in range(9)] for kk in (1.0, 0.25)}
    return dict(m=m, S=S, msk=msk, L=L, Yh=Yh, cons=cons, XSh=XSh, YSh=YSh, BXh=BXh, BYh=BYh, refs=refs)


@pytest.mark.parametrize("max_rhs", [3, 12])
@pytest.mark.parametrize("name", ["arrow", "rand2", "nested_mid", "diag", "fam_max", "fam_odd", "nested"])
def test_rows_against_the_oracle(name, max_rhs):
    """RX on the pattern and RY against K.residual to 1e-9 relative in the 2-norm: the bound test_hessian holds
    hessian(adj=None, inv=True) to on these patterns (tests/test_gpu_parity.py:118; the inputs are O(1) random, so is the
    residual).  The four norms against the host's sums over the device's own RX / BX / RY / BY to 1e-12: fewer than 1e4 terms at
    2^-53 each.  1, 2, 5 and 9 padded rows; max_rhs = 3 leaves the context setup() made (four rows): five and nine rows go in
    chunks.  The inputs, L and Y come back bit for bit and the padding of the outputs is intact."""
    c = _oracle_case(name)
    m, S, msk, L, Yh = (c[k] for k in ("m", "S", "msk", "L", "Yh"))
    symb = Symbolic(GPU_PATTERNS[name]())
    symb.device_init(0, 4)
    sys = KKTSystem(symb, *c["cons"], max_rhs=max_rhs)
    bl = symb.blklen
    assert symb._max_rhs == (4 if max_rhs == 3 else 12)
    Ld, Yd = dev(symb, L), dev(symb, Yh)
    keep = [Ld.blkval.clone(), Yd.blkval.clone()]
    states = (Ld.state(), Yd.state())
    for kk in (1.0, 0.25):
        refs = c["refs"][kk]
        for k in (1, 2, 5, 9):
            ins = [_padded(c["XSh"][:k], bl, 3), _padded(c["YSh"][:k], m, 2), _padded(c["BXh"][:k], bl, 1), _padded(c["BYh"][:k], m, 5)]
            ins0 = [t.clone() for t in ins]
            RX = torch.full((k, bl + 3), SENT, dtype=torch.float64, device="cuda")
            RY = torch.full((k, m + 1), SENT, dtype=torch.float64, device="cuda")
            out = sys.residual_many(Ld, Yd, *ins, kk, RX=RX, RY=RY)
            assert out[0] is RX and out[1] is RY and out[2].shape == (k, 4)
            assert bool((RX[:, bl:] == SENT).all()) and bool((RY[:, m:] == SENT).all())
            for a, b in zip(ins, ins0):
                assert _same_bits(a, b)
            gx, gy, gn = RX[:, :bl].cpu().numpy(), RY[:, :m].cpu().numpy(), out[2].cpu().numpy()
            for r in range(k):
                rx, ry = refs[r]
                ex, ey = rel(gx[r][msk], rx[msk]), rel(gy[r], ry)
                want = [np.sqrt(orc.dot(S, gx[r], gx[r])), np.linalg.norm(gy[r]),
                        np.sqrt(orc.dot(S, c["BXh"][r], c["BXh"][r])), np.linalg.norm(c["BYh"][r])]
                en = [abs(gn[r][q] - want[q]) / want[q] for q in range(4)]
                print("%s max_rhs %d kk %g k %d row %d: RX %.2e RY %.2e norms %s" % (name, max_rhs, kk, k, r, ex, ey, ["%.1e" % e for e in en]))
                assert ex < 1e-9 and ey < 1e-9, (kk, k, r, ex, ey)
                assert max(en) < 1e-12, (kk, k, r, en)
    assert _same_bits(Ld.blkval, keep[0]) and _same_bits(Yd.blkval, keep[1])
    assert (Ld.state(), Yd.state()) == states
    # the single form: one row, new outputs, no norms
    x, y = dev(symb, c["XSh"][4]), torch.from_numpy(c["YSh"][4].copy()).cuda()
    bx, by = dev(symb, c["BXh"][4]), torch.from_numpy(c["BYh"][4].copy()).cuda()
    r, rr = sys.residual(Ld, Yd, x, y, bx, by, 0.25)
    assert isinstance(r, cspmatrix) and rr.shape == (m,)
    assert rel(r.blkval.cpu().numpy()[msk], c["refs"][0.25][4][0][msk]) < 1e-9
    assert rel(rr.cpu().numpy(), c["refs"][0.25][4][1]) < 1e-9


# ---- 2. against the composition on the device ---------------------------------------------------------------------------
def _device_case(name, m, max_rhs, density, seed=7):
    """as in test_gpu_solve_many_qr (every constraint swept, so that factor and factor_qr both apply)"""
    return _qr_device_case(name, m, max_rhs, density, seed)


def _composition(symb, sys, L, Y, x, y, bx, by, kk):
    """kkt_res as the drivers put it together (smcp_amd/solvers.py: kkt_res), one right-hand side"""
    r = cspmatrix(symb, x.clone())
    chordal.hessian(L, Y, r, adj=None, inv=True)
    r.blkval.mul_(-kk)
    r.blkval.add_(sys.aadj(y).blkval)
    r.blkval.sub_(bx)
    rr = sys.amap(cspmatrix(symb, x.clone())) - by
    return r.blkval, rr


@pytest.mark.parametrize("m", [70, 130])
def test_against_the_composition(m):
    """arrow_big (blklen 172 032: 84 workgroups per row of the combine pass, large fronts), m = 70 and 130, 3 / 9 / 17 rows: every
    row of RX (on the pattern) and RY within 1e-13, relative in the 2-norm, of the Python composition -- the Hessian kernels are
    the same, only the order of three additions differs."""
    kk = 0.25
    symb, msk, L, Y, sys = _device_case("arrow_big", m, 20, 0.002)
    bl = symb.blklen
    assert bl == 172032
    mskd = torch.from_numpy(msk).cuda()
    rng = np.random.default_rng(8)
    XS = torch.from_numpy(rng.standard_normal((17, bl)) * msk).cuda()
    YS = torch.from_numpy(rng.standard_normal((17, m))).cuda()
    BX = torch.from_numpy(rng.standard_normal((17, bl)) * msk).cuda()
    BY = torch.from_numpy(rng.standard_normal((17, m))).cuda()
    comp = [_composition(symb, sys, L, Y, XS[r], YS[r], BX[r], BY[r], kk) for r in range(17)]
    for k in (3, 9, 17):
        RX, RY, norms = sys.residual_many(L, Y, XS[:k], YS[:k], BX[:k], BY[:k], kk)
        for r in range(k):
            ex = float(torch.linalg.norm((RX[r] - comp[r][0])[mskd]) / torch.linalg.norm(comp[r][0][mskd]))
            ey = float(torch.linalg.norm(RY[r] - comp[r][1]) / torch.linalg.norm(comp[r][1]))
            nx = np.sqrt(max(chordal.dot(cspmatrix(symb, RX[r].clone()), cspmatrix(symb, RX[r].clone())), 0.0))
            en = abs(float(norms[r, 0]) - nx) / nx
            print("m %d k %d row %d: RX %.2e RY %.2e ||RX|| against csp_dot %.1e" % (m, k, r, ex, ey, en))
            assert ex < 1e-13 and ey < 1e-13, (k, r, ex, ey)
            assert en < 1e-12, (k, r, en)


# ---- 3. solutions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,density", [("nested_mid", 7, 0.05), ("arrow", 7, 0.05)])
def test_residuals_of_block_solutions(name, m, density):
    """After factor + solve_many the two normalised residuals of every row are below 1e-10, the residual bound of
    test_kkt_factor_and_solve; the same after factor_qr + solve_many_qr, and Q is still valid then: solve_many_qr and the closure
    run without factoring again, and under TUNE_DETERMINISTIC the closure gives the bits it gave before."""
    kk = 0.25
    symb, msk, L, Y, sys = _device_case(name, m, 12, density)
    bl = symb.blklen
    rng = np.random.default_rng(8)
    BX0 = torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda()
    BY0 = torch.from_numpy(rng.standard_normal((5, m))).cuda()
    sys.factor(L, Y)
    X, Yv = sys.solve_many(L, Y, BX0.clone(), BY0.clone(), kk)
    _, _, norms = sys.residual_many(L, Y, X, Yv, BX0, BY0, kk)
    res = _normalised(norms)
    print("%s m %d factor + solve_many: normalised residuals up to %.2e %.2e" % (name, m, res[:, 0].max(), res[:, 1].max()))
    assert res.max() < 1e-10, res
    solve = sys.factor_qr(L, Y)

    def single():
        bx, by = cspmatrix(symb, BX0[1].clone()), BY0[1].clone()
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)
        try:
            solve(bx, by, kk)
        finally:
            chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)
        return bx.blkval.clone(), by.clone()

    s0 = single()
    X, Yv = sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), kk)
    _, _, norms = sys.residual_many(L, Y, X, Yv, BX0, BY0, kk)
    res = _normalised(norms)
    print("%s m %d factor_qr + solve_many_qr: normalised residuals up to %.2e %.2e" % (name, m, res[:, 0].max(), res[:, 1].max()))
    assert res.max() < 1e-10, res
    X2, Y2 = sys.solve_many_qr(L, Y, BX0.clone(), BY0.clone(), kk)          # Q is still there
    for r in range(5):
        assert rel(X2[r].cpu().numpy()[msk], X[r].cpu().numpy()[msk]) < 1e-9 and rel(Y2[r].cpu().numpy(), Yv[r].cpu().numpy()) < 1e-9
    s1 = single()
    assert _same_bits(s1[0], s0[0]) and _same_bits(s1[1], s0[1])


# ---- 4. refinement does its work ----------------------------------------------------------------------------------------
# The worst contraction of the normalised residuals that the ORACLE's refinement loop shows on nested_mid with the Cholesky factor
# of the Schur complement multiplied elementwise by 1 + 1e-6 N (N symmetric standard normal, seed 1), five rows, two rounds,
# kk = 0.7, computed on the CPU (K.solve / K.residual): 7.53e-06, counted where the later residual is above 1e-12.  The device is
# held to ten times that.
ORACLE_CONTRACTION = 7.53e-6
RHO = 10 * ORACLE_CONTRACTION


def _oracle_refine(K, L, Yh, H, bx, by, kk, rounds):
    x, y = K.solve(L, Yh, H, bx, by, kk)
    S = K.S
    nb = (max(1.0, np.sqrt(orc.dot(S, bx, bx))), max(1.0, np.linalg.norm(by)))
    hist = []
    for j in range(rounds + 1):
        rx, ry = K.residual(L, Yh, x, y, bx, by, kk)
        hist.append((np.sqrt(orc.dot(S, rx, rx)) / nb[0], np.linalg.norm(ry) / nb[1]))
        if j == rounds:
            break
        dx, dy = K.solve(L, Yh, H, rx, ry, kk)
        x, y = x - dx, y - dy
    return x, y, np.array(hist)


def test_refinement_does_its_work():
    name, m, kk = "nested_mid", 7, 0.7
    symb, S, A, msk = setup(name, 7)
    L = A.copy()
    orc.cholesky(S, L)
    Yh = L.copy()
    orc.projected_inverse(S, Yh)
    cons = problems.random_constraints(symb, m, density=0.05, seed=9)
    K = orc.KKT(S, *cons)
    Href = K.schur_factor(L, Yh)
    sys = KKTSystem(symb, *cons, max_rhs=12, tnzcols=0.0)
    bl = symb.blklen
    Ld, Yd = dev(symb, L), dev(symb, Yh)
    rng = np.random.default_rng(8)
    BXh = rng.standard_normal((5, bl)) * msk
    BYh = rng.standard_normal((5, m))
    exact = [K.solve(L, Yh, Href, BXh[r], BYh[r], kk) for r in range(5)]

    def block(pad=3):
        return _padded(BXh, bl, pad), _padded(BYh, m, 2)

    def agree(BX, BY, want, what):
        assert bool((BX[:, bl:] == SENT).all()) and bool((BY[:, m:] == SENT).all())
        gx, gy = BX[:, :bl].cpu().numpy(), BY[:, :m].cpu().numpy()
        for r in range(5):
            ex, ey = rel(gx[r][msk], want[r][0][msk]), rel(gy[r], want[r][1])
            print("%s row %d: x %.2e y %.2e" % (what, r, ex, ey))
            assert ex < 1e-9 and ey < 1e-9, (what, r, ex, ey)

    # (a) unperturbed factor: the whole of refine_many(rounds=1, final=False) against the oracle's loop
    sys.factor(Ld, Yd)
    BX, BY = block()
    out = sys.refine_many(Ld, Yd, BX, BY, kk, rounds=1, final=False)
    assert out[0] is BX and out[1] is BY and out[2].shape == (1, 5, 4)
    agree(BX, BY, [_oracle_refine(K, L, Yh, Href, BXh[r], BYh[r], kk, 1)[:2] for r in range(5)], "one round, unperturbed H")
    want0 = np.array([[np.sqrt(orc.dot(S, BXh[r], BXh[r])), np.linalg.norm(BYh[r])] for r in range(5)])
    assert np.abs(out[2][0].cpu().numpy()[:, 2:] / want0 - 1.0).max() < 1e-12          # ||bx||, ||by|| of the kept right-hand sides
    # (b) the factor of H perturbed in place, the oracle's likewise
    N = np.random.default_rng(1).standard_normal((m, m))
    N = (N + N.T) / np.sqrt(2.0)
    scale = 1.0 + 1e-6 * N
    sys.H.mul_(torch.from_numpy(scale).cuda())             # (N symmetric: the same factor whichever way H is stored)
    Hp = np.asfortranarray(Href * scale)
    worst = 0.0
    for r in range(5):
        h = _oracle_refine(K, L, Yh, Hp, BXh[r], BYh[r], kk, 2)[2]
        for j in range(2):
            for q in range(2):
                if h[j + 1, q] > 1e-12:
                    worst = max(worst, h[j + 1, q] / h[j, q])
    print("oracle on the perturbed factor: worst contraction %.3e (recorded %.3e)" % (worst, ORACLE_CONTRACTION))
    assert worst / 10 < 1e-2
    BX, BY = block()
    _, _, hist = sys.refine_many(Ld, Yd, BX, BY, kk, rounds=2)
    assert hist.shape == (3, 5, 4)
    h = _normalised(hist)
    for r in range(5):
        print("perturbed H row %d: normalised residuals by round %s" % (r, ["%.2e / %.2e" % tuple(h[j, r]) for j in range(3)]))
    assert h[0].max() > 1e-6                                # the perturbation shows before the first round
    for j in range(2):
        assert bool((h[j + 1] <= np.maximum(RHO * h[j], 1e-10)).all()), (j, h[j], h[j + 1])
    agree(BX, BY, exact, "two rounds, perturbed H")
    # (c) kkt_qr on unperturbed factors
    sys.factor_qr(Ld, Yd)
    BX, BY = block(pad=4)
    _, _, hist = sys.refine_many(Ld, Yd, BX, BY, kk, rounds=2, qr=True)
    h = _normalised(hist)
    for r in range(5):
        print("kkt_qr row %d: normalised residuals by round %s" % (r, ["%.2e / %.2e" % tuple(h[j, r]) for j in range(3)]))
    for j in range(2):
        assert bool((h[j + 1] <= np.maximum(h[j], 1e-10)).all()), (j, h[j], h[j + 1])
    agree(BX, BY, exact, "two rounds, kkt_qr")
    X2, Y2 = block()
    sys.solve_many_qr(Ld, Yd, X2, Y2, kk)                   # refinement has left Q alone
    agree(X2, Y2, exact, "solve_many_qr afterwards")


# ---- 5. properties --------------------------------------------------------------------------------------------------------
def _residual_block(sys, L, Y, bl, m, kk):
    def block(XS, YS, BX, BY, pad=0):
        RX = torch.full((5, bl + pad), SENT, dtype=torch.float64, device="cuda")
        RY = torch.full((5, m + 2 * pad), SENT, dtype=torch.float64, device="cuda")
        ins = []
        for T, w in ((XS, bl), (YS, m), (BX, bl), (BY, m)):
            P = torch.full((5, w + 3 * pad), SENT, dtype=torch.float64, device="cuda")
            P[:, :w] = T
            ins.append(P)
        _, _, norms = sys.residual_many(L, Y, *ins, kk, RX=RX, RY=RY)
        assert bool((RX[:, bl:] == SENT).all()) and bool((RY[:, m:] == SENT).all())
        return RX[:, :bl].clone(), RY[:, :m].clone(), norms.clone()
    return block


def _refine_block(sys, L, Y, bl, m, kk):
    def block(XS, YS, BX, BY, pad=0):
        PX = torch.full((5, bl + pad), SENT, dtype=torch.float64, device="cuda")
        PY = torch.full((5, m + 2 * pad), SENT, dtype=torch.float64, device="cuda")
        PX[:, :bl] = BX
        PY[:, :m] = BY
        _, _, hist = sys.refine_many(L, Y, PX, PY, kk, rounds=1)
        assert bool((PX[:, bl:] == SENT).all()) and bool((PY[:, m:] == SENT).all())
        return PX[:, :bl].clone(), PY[:, :m].clone(), hist.transpose(0, 1).contiguous()       # (row first, as the other two)
    return block


def _isolation(block, mskd, ins):
    a = block(*ins)
    b = block(*ins)
    on = lambda t: t[0][:, mskd]                           # (the slots above the diagonal are not part of the contract)
    assert bool(torch.isfinite(on(a)).all()) and bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(a[2]).all())
    assert _same_bits(on(a), on(b)) and _same_bits(a[1], b[1]) and _same_bits(a[2], b[2])      # the same call twice: the same bits
    for pad in (1, 5):
        p = block(*ins, pad=pad)
        assert _same_bits(on(p), on(a)) and _same_bits(p[1], a[1]) and _same_bits(p[2], a[2]), pad      # the padding width does not matter
    for bad in (0, 3):
        poisoned = [t.clone() for t in ins]
        for t in poisoned:
            t[bad] = float("nan")
        c = block(*poisoned)                                # one row poisoned
        for r in range(5):
            if r != bad:
                assert _same_bits(on(c)[r], on(a)[r]) and _same_bits(c[1][r], a[1][r]) and _same_bits(c[2][r], a[2][r]), (bad, r)
    # a row computed alone
    alone = [t[2:3].expand(5, -1).clone() for t in ins]
    d = block(*alone)
    assert _same_bits(on(d)[0], on(a)[2]) and _same_bits(d[1][0], a[1][2]) and _same_bits(d[2][0], a[2][2])


@pytest.mark.parametrize("name,m", [("nested_mid", 7), ("arrow_big", 130)])
def test_determinism_and_isolation(name, m):
    """Under TUNE_DETERMINISTIC (and on arrow_big, whose large fronts add nothing with atomics, on the default route as well): two
    identical calls give identical bits, norms included; a row among NaN rows equals the row computed without them; the padding
    widths -- which move the rows between 16-byte aligned and unaligned addresses -- do not change a bit."""
    kk = 0.7
    symb, msk, L, Y, sys = _device_case(name, m, 12, 0.05 if m == 7 else 0.002)
    bl = symb.blklen
    mskd = torch.from_numpy(msk).cuda()
    rng = np.random.default_rng(11)
    ins = [torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda(), torch.from_numpy(rng.standard_normal((5, m))).cuda(),
           torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda(), torch.from_numpy(rng.standard_normal((5, m))).cuda()]
    routes = [1, 0] if name == "arrow_big" else [1]
    for det in routes:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, det)
        try:
            sys.factor(L, Y)
            _isolation(_residual_block(sys, L, Y, bl, m, kk), mskd, ins)
            _isolation(_refine_block(sys, L, Y, bl, m, kk), mskd, ins)
        finally:
            chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)


@pytest.mark.parametrize("name,m,density", [("nested_mid", 7, 0.05), ("arrow_big", 130, 0.002)])
def test_launches_and_ledger(name, m, density):
    """The launches of residual_many and of refine_many are the same for 2 and 9 rows of one chunk, hold every new kernel once per
    residual (and the update once per round) and no k_reduce_final of csp_dot; the ledger grows at the first call and not again."""
    symb, msk, L, Y, sys = _device_case(name, m, 16, density)
    bl = symb.blklen
    sys.factor(L, Y)
    rng = np.random.default_rng(12)
    XS = torch.from_numpy(rng.standard_normal((17, bl)) * msk).cuda()
    YS = torch.from_numpy(rng.standard_normal((17, m))).cuda()
    BX = torch.from_numpy(rng.standard_normal((17, bl)) * msk).cuda()
    BY = torch.from_numpy(rng.standard_normal((17, m))).cuda()
    chordal.hessian(L, Y, XS[:2].clone(), adj=None, inv=True)       # (whatever the inverse Hessian itself allocates at its first call)
    before = symb.device_bytes()
    sys.residual_many(L, Y, XS[:2], YS[:2], BX[:2], BY[:2], 1.0)
    first = symb.device_bytes()
    stated = 4 * bl + 8 * 16 * 1026                          # include/smcp_amd.h: the position table and the partial sums of max_rhs rows
    print("%s m %d: ledger %d -> %d bytes, stated workspace %d" % (name, m, before, first, stated))
    assert 0 < first - before <= stated
    res, ref, sol = {}, {}, {}
    for k in (2, 9):
        res[k] = launch_counts(symb, lambda: sys.residual_many(L, Y, XS[:k], YS[:k], BX[:k], BY[:k], 1.0))
        sys.refine_many(L, Y, BX[:k].clone(), BY[:k].clone(), 1.0, rounds=2)                  # warm: scratch of the solves
        X, Yv = BX[:k].clone(), BY[:k].clone()
        sol[k] = launch_counts(symb, lambda: sys.solve_many(L, Y, X, Yv, 1.0))
        X, Yv = BX[:k].clone(), BY[:k].clone()
        ref[k] = launch_counts(symb, lambda: sys.refine_many(L, Y, X, Yv, 1.0, rounds=2))
        print("%s m %d k %d: residual_many %s\n   refine_many %s" % (name, m, k, res[k], ref[k]))
    assert res[2] == res[9], (res[2], res[9])
    for k in (2, 9):
        # refine_many(rounds=2) is three solves, three residuals and two updates and nothing else (the sweeps of solve_many choose
        # their kernels by the number of rows -- its own test compares its new kernels only -- so the sum is taken per k)
        want = {"k_kkt_many_sub": 2}
        for part in (res[k], sol[k]):
            for n, cnt in part.items():
                want[n] = want.get(n, 0) + 3 * cnt
        assert ref[k] == want, (k, ref[k], want)
    assert {n: ref[2].get(n, 0) for n in NEW_KERNELS} == {n: ref[9].get(n, 0) for n in NEW_KERNELS}
    assert sum(ref[2].values()) == sum(ref[9].values()), (ref[2], ref[9])      # the number of launches does not depend on k
    for n in RES_KERNELS:
        assert res[2].get(n, 0) == 1 and ref[2].get(n, 0) == 3, (n, res[2], ref[2])
    assert "k_kkt_many_sub" not in res[2] and ref[2].get("k_kkt_many_sub", 0) == 2
    assert res[2].get("k_amap", 0) == 1
    for n in ("k_reduce_final", "k_reduce_cliques", "k_res_inv_table", "k_aadj", "k_vec_axpby"):
        assert n not in res[2] and n not in ref[2], (n, res[2], ref[2])
    nonorm = launch_counts(symb, lambda: sys.residual(L, Y, cspmatrix(symb, XS[0].clone()), YS[0].clone(), cspmatrix(symb, BX[0].clone()), BY[0].clone(), 1.0))
    assert "k_res_norms" not in nonorm and nonorm.get("k_res_combine", 0) == 1 and nonorm.get("k_res_y", 0) == 1
    two = launch_counts(symb, lambda: sys.residual_many(L, Y, XS, YS, BX, BY, 1.0))          # 17 rows on 16: two chunks
    for n in RES_KERNELS:
        assert two.get(n, 0) == 2, (n, two)
    # (refine_many ran solve_many on nine rows in between, whose dense solve keeps a scratch of its own beyond m = 128: the
    # residual calls since the first one have added nothing to that)
    steady = symb.device_bytes()
    assert res[2].get("k_res_combine", 0) == 1 and steady >= first
    for k in (1, 9, 17):
        sys.residual_many(L, Y, XS[:k], YS[:k], BX[:k], BY[:k], 0.5)
        assert symb.device_bytes() == steady, k
    chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 1)       # the other weight source: the same buffers
    try:
        sys.residual_many(L, Y, XS[:9], YS[:9], BX[:9], BY[:9], 0.5)
    finally:
        chordal.tune(symb, chordal.TUNE_DETERMINISTIC, 0)
    assert symb.device_bytes() == steady


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.lib()
    m = 7
    symb, msk, L, Y, sys = _device_case("arrow", m, 12, 0.05)
    bl, h = symb.blklen, symb.handle
    rng = np.random.default_rng(5)
    buf = torch.from_numpy(rng.standard_normal(6 * bl + 64)).cuda()        # [0, 2 bl): RX; [2 bl, 4 bl): BX; [4 bl, 6 bl): XS; then norms
    buf0 = buf.clone()
    RX, BX, XS = (buf[i * 2 * bl:(i + 1) * 2 * bl].view(2, bl) for i in range(3))
    norms = buf[6 * bl:6 * bl + 8]
    ybuf = torch.from_numpy(rng.standard_normal(6 * m)).cuda()
    ybuf0 = ybuf.clone()
    RY, BY, YS = (ybuf[i * 2 * m:(i + 1) * 2 * m].view(2, m) for i in range(3))
    Lp, Yp = L.blkval.data_ptr(), Y.blkval.data_ptr()

    def call(ctx=h, xs=XS.data_ptr(), ys=YS.data_ptr(), bx=BX.data_ptr(), by=BY.data_ptr(), rx=RX.data_ptr(), ldrx=bl, ry=RY.data_ptr(),
             ldry=m, nm=norms.data_ptr(), nrhs=2):
        return lib.kkt_residual_many(ctx, Lp, Yp, 1.0, xs, bl, ys, m, bx, bl, by, m, rx, ldrx, ry, ldry, nm, nrhs, None)

    def untouched():
        torch.cuda.synchronize()
        return _same_bits(buf, buf0) and _same_bits(ybuf, ybuf0)

    assert call(rx=buf[bl:].data_ptr()) == -1                       # RX reaching into BX
    assert call(rx=BX.data_ptr()) == -1                             # RX is BX
    assert call(rx=buf[4 * bl + 64 - 1:].data_ptr()) == -1          # RX over XS and norms
    assert call(nm=buf[2 * bl - 1:].data_ptr()) == -1               # norms starting at the last entry of RX
    assert call(nm=RY.data_ptr()) == -1                             # norms over RY
    assert call(ry=BY.data_ptr()) == -1                             # RY is BY
    assert call(ry=buf[:2 * m].data_ptr()) == -1                    # RY inside RX
    assert call(rx=Lp) == -1 and call(rx=Yp, nrhs=1) == -1          # RX over a factor
    assert call(ldrx=bl - 1) == -1 and call(ldry=m - 1) == -1       # short leading dimensions with two rows
    assert call(nrhs=0) == -1
    assert call(xs=None) == -1 and call(rx=None) == -1 and call(by=None) == -1
    assert untouched()
    with pytest.raises(ValueError):
        sys.residual_many(L, Y, XS, YS, BX, BY[:1], 1.0)
    with pytest.raises(ValueError):
        sys.residual_many(L, Y, XS[:1], YS[:1], BX, BY, 1.0)
    with pytest.raises(ValueError):
        sys.residual_many(L, Y, XS, YS, BX, BY, 1.0, RX=RX[:, :bl - 1])
    with pytest.raises(ValueError):
        sys.residual_many(L, Y, XS, YS, BX, BY, 1.0, norms=torch.zeros(2, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        sys.refine_many(L, Y, BX, BY, 1.0, qr=True)                 # no factor_qr yet: the refusal of solve_many_qr
    with pytest.raises(ValueError):
        sys.refine_many(L, Y, BX, BY, 1.0, rounds=-1)
    assert untouched()
    # the update of a round: X and D must not share memory
    assert lib.kkt_update_many(h, BX.data_ptr(), bl, BY.data_ptr(), m, buf[3 * bl:].data_ptr(), bl, YS.data_ptr(), m, 2, None) == -1
    assert lib.kkt_update_many(h, BX.data_ptr(), bl, BY.data_ptr(), m, XS.data_ptr(), bl, YS.data_ptr(), m, 0, None) == -1
    assert untouched()
    assert call() == 0                                              # side by side is fine
    torch.cuda.synchronize()
    assert _same_bits(buf[2 * bl:6 * bl], buf0[2 * bl:6 * bl]) and _same_bits(ybuf[2 * m:], ybuf0[2 * m:])      # inputs only read
    buf.copy_(buf0)
    ybuf.copy_(ybuf0)
    # the Python methods on a sharded pair
    sys.__dict__["_spair"] = (L, Y, (L.state(), Y.state()))
    try:
        with pytest.raises(NotImplementedError):
            sys.residual_many(L, Y, XS, YS, BX, BY, 1.0)
        with pytest.raises(NotImplementedError):
            sys.refine_many(L, Y, BX, BY, 1.0)
    finally:
        sys.__dict__.pop("_spair", None)
    # a multi-rank partition on the context
    P = shard.subtree_partition(symb, 2)
    owner = np.ascontiguousarray(P.owner, dtype=np.int32)
    assert owner.max() == 1
    assert lib.csp_set_partition(h, owner.ctypes.data, 0) == 0
    assert call() == -1
    assert untouched()
    # a context without constraints
    bare = Symbolic(GPU_PATTERNS["arrow"]())
    bare.device_init(0, 4)
    assert call(ctx=bare.handle) == -1
    assert untouched()


# ---- 7. deferred status -----------------------------------------------------------------------------------------------------
def test_deferred_status():
    """chordal.lazy_status: a Y changed in place to something outside the cone (the cached factors are formed again) is latched by
    residual_many, which returns without waiting, and raises from check_status; a clean call leaves nothing behind."""
    m = 7
    symb, msk, L, Y, sys = _device_case("nested_mid", m, 12, 0.05)
    bl = symb.blklen
    rng = np.random.default_rng(4)
    ins = [torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda(), torch.from_numpy(rng.standard_normal((5, m))).cuda(),
           torch.from_numpy(rng.standard_normal((5, bl)) * msk).cuda(), torch.from_numpy(rng.standard_normal((5, m))).cuda()]
    r1 = sys.residual_many(L, Y, *ins, 0.7)
    chordal.lazy_status(symb, True)
    try:
        r2 = sys.residual_many(L, Y, *ins, 0.7)
        chordal.check_status(symb)                        # nothing failed, nothing latched
        assert rel(r2[2].cpu().numpy(), r1[2].cpu().numpy()) < 1e-12
        Y.blkval.neg_()                                   # negative definite separator blocks: every chol(Y_AA) fails
        sys.residual_many(L, Y, *ins, 0.7)                # no hang, no fault; the verdict waits
        with pytest.raises(ArithmeticError):
            chordal.check_status(symb)
        Y.blkval.neg_()
        r3 = sys.residual_many(L, Y, *ins, 0.7)           # the context recovers
        chordal.check_status(symb)
        assert rel(r3[2].cpu().numpy(), r1[2].cpu().numpy()) < 1e-12
        for r in range(5):
            assert rel(r3[0][r].cpu().numpy()[msk], r1[0][r].cpu().numpy()[msk]) < 1e-9
    finally:
        chordal.lazy_status(symb, False)
    with pytest.raises(ArithmeticError):                  # eager again: the same Y is reported by the call itself
        Y.blkval.neg_()
        sys.residual_many(L, Y, *ins, 0.7)


# ---- 8. straight after a Schur complement whose sweep used the fused extend-add ---------------------------------------------
def test_residual_straight_after_a_fused_schur_sweep():
    """The case of test_family_updates_formed_by_the_extend_add (nested_mid, m = 40, closed-form leaf blocks on: the family
    parents' updates are formed by the extend-add of the front above, k_lf_assemble_fz).  That route is a property of ONE Schur
    sweep; the inverse Hessian of a residual taken right after factor() -- no solve in between -- has extend-adds of its own on
    the same fronts and must take its own route.  Rows against K.residual to the bound of test 1."""
    name, m, kk = "nested_mid", 40, 0.5
    symb, S, A, msk = setup(name, 31)
    L = A.copy()
    orc.cholesky(S, L)
    Yh = L.copy()
    orc.projected_inverse(S, Yh)
    cons = problems.random_constraints(symb, m, density=0.002, seed=33)
    K = orc.KKT(S, *cons)
    sys = KKTSystem(symb, *cons, max_rhs=m, tnzcols=0.0)
    bl = symb.blklen
    rng = np.random.default_rng(32)
    XSh, YSh = rng.standard_normal((3, bl)) * msk, rng.standard_normal((3, m))
    BXh, BYh = rng.standard_normal((3, bl)) * msk, rng.standard_normal((3, m))
    ins = [torch.from_numpy(t).cuda() for t in (XSh, YSh, BXh, BYh)]
    chordal.tune(symb, chordal.TUNE_LEAFGRAM, 2)
    try:
        Ld, Yd = dev(symb, L), dev(symb, Yh)
        counts = launch_counts(symb, lambda: sys.factor(Ld, Yd))
        assert counts.get("k_lf_assemble_fz", 0) >= 1, counts
        RX, RY, norms = sys.residual_many(Ld, Yd, *ins, kk)
        torch.cuda.synchronize()
    finally:
        chordal.tune(symb, chordal.TUNE_LEAFGRAM, 1)
    gx, gy = RX.cpu().numpy(), RY.cpu().numpy()
    for r in range(3):
        rx, ry = K.residual(L, Yh, XSh[r], YSh[r], BXh[r], BYh[r], kk)
        ex, ey = rel(gx[r][msk], rx[msk]), rel(gy[r], ry)
        print("row %d after the fused sweep: RX %.2e RY %.2e" % (r, ex, ey))
        assert ex < 1e-9 and ey < 1e-9, (r, ex, ey)
