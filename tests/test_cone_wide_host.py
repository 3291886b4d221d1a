"""The clique step of cone_project on the wide route (tune(symb, TUNE_CEIG_WIDE, 65); csrc/front_ceigw.hip: k_ceigw_cone_form,
k_ceigw_cone_split, k_ceigw_cone_finish) restated in numpy: the negative part of T_k from the block Jacobi of
tests/test_clique_wide_host.py for blocks of at least 65 rows and from the kernel form of tests/test_cone_project_host.py
below that, plugged into cone_project_restatement and measured against its LAPACK form (no GPU needed;
tests/test_gpu_cone_wide.py imports this file).

Measured (the printed lines), three iterations, in units nf_max eps max(1, |A|): at most 0.030 on
wide_root(70) (indef) and 0.018 on wide_root(97), 0.006 on fam_top (wide cliques 130, 130, 110; noisy); the most sweeps of
a clique, Jacobi or block, 7 and 8; asserted: CONE_UNITS = 1."""
import numpy as np
import pytest

import test_cone_project_host as tch
from helpers import GPU_PATTERNS
from smcp_amd import problems
from smcp_amd.symbolic import Symbolic
from test_clique_eig_host import MAX_SWEEPS
from test_clique_wide_host import block_jacobi_restatement
from test_clique_eigh_host import lower_slots
from test_cone_project_host import CONE_UNITS, KINDS, PARAMS, cone_project_restatement, unit_of
from test_mrcompletion_host import pd_on_V

WIDE = 65
_SYMB, _REF, _INPUT = {}, {}, {}
_kernel_or_lapack = tch.negative_part


def wide_root(R):
    """two 10-column leaf cliques whose separators are rows 0 .. 5 and 20 .. 27 of a dense root clique of R rows"""
    root = np.arange(20, 20 + R)
    cl = [(np.arange(0, 10), np.concatenate([np.arange(0, 10), root[0:6]])),
          (np.arange(10, 20), np.concatenate([np.arange(10, 20), root[20:28]])),
          (root, root)]
    return problems._from_cliques(20 + R, cl)


HOST_PATS = {"wide_root70": lambda: wide_root(70), "wide_root97": lambda: wide_root(97), "fam_top": GPU_PATTERNS["fam_top"]}


def host_symb(name):
    if name not in _SYMB:
        _SYMB[name] = Symbolic(HOST_PATS[name]())
    return _SYMB[name]


def wide_input(name, symb, kind, seed=3):
    """the blkval that tch.cone_input makes for (symb, kind), kept per pattern NAME: made once, never changed.  tch.cone_input
    keeps its inputs per id(symb), and a Symbolic made after another one was freed can get its id and with it the input of
    another pattern (tests/test_gpu_cone_project.py frees Symbolics it called cone_input on); the Symbolics of one name in
    these files have the same pattern, so the name is a safe key"""
    key = (name, kind, seed)
    if key not in _INPUT:
        blk = {"noisy": tch.noisy_on_V, "indef": tch.indef_on_V, "incone": lambda s, sd: np.where(lower_slots(s), pd_on_V(s, sd), 0.0)}[kind](symb, seed)
        blk.setflags(write=False)
        _INPUT[key] = blk
    assert len(_INPUT[key]) == symb.blklen
    return _INPUT[key]


def cone_input(symb, kind):
    """wide_input for a Symbolic of host_symb"""
    return wide_input(next(n for n, s in _SYMB.items() if s is symb), symb, kind)


def negative_part(T, form):
    """tch.negative_part with one more form, "wide": a block of at least WIDE rows through block_jacobi_restatement and the
    sum of k_ceigw_cone_split (over the negative eigenvalues, ascending, per entry of the lower triangle, mirrored), a
    narrower one through the kernel form"""
    if form != "wide":
        return _kernel_or_lapack(T, form)
    if T.shape[0] < WIDE:
        return _kernel_or_lapack(T, "kernel")
    w, Q, sweeps, ok = block_jacobi_restatement(T)
    assert ok
    U = np.zeros_like(T)
    for j in range(len(w)):
        if w[j] < 0:
            U += w[j] * (Q[:, j][:, None] * Q[:, j][None, :])
    U = np.tril(U)
    return U + np.tril(U, -1).T, int((w < 0).sum()), sweeps, w


def wide_restatement(symb, blk, **kw):
    """cone_project_restatement with the clique step of the wide route"""
    tch.negative_part = negative_part
    try:
        return cone_project_restatement(symb, blk, form="wide", **kw)
    finally:
        tch.negative_part = _kernel_or_lapack


def lapack_reference(name, kind, rho, relax):
    """three iterations in the LAPACK form: made once per case, never changed"""
    key = (name, kind, rho, relax)
    if key not in _REF:
        symb = host_symb(name)
        _REF[key] = cone_project_restatement(symb, cone_input(symb, kind), rho=rho, relax=relax, steps=3)
    return _REF[key]


def compare(name, kind, rho, relax, capsys):
    symb = host_symb(name)
    ref = lapack_reference(name, kind, rho, relax)
    got = wide_restatement(symb, cone_input(symb, kind), rho=rho, relax=relax, steps=3)
    worst = max(np.abs(got[key] - ref[key]).max() for key in ("x", "U", "W")) / unit_of(symb, ref["scale"])
    with capsys.disabled():
        print("\n%s %s rho %g relax %g: wide form against LAPACK form after 3 iterations: %.3f units, %d sweeps at most"
              % (name, kind, rho, relax, worst, got["sweeps"]))
    assert worst <= CONE_UNITS
    assert got["sweeps"] <= MAX_SWEEPS
    if kind == "incone":
        assert not got["U"].any() and (got["hist"][:, 2] == 0).all()      # U exactly 0, no negative eigenvalue
    return got


@pytest.mark.parametrize("R", [70, 97])
def test_pattern_has_one_wide_clique(R):
    symb = host_symb("wide_root%d" % R)
    assert sorted(np.diff(symb.rowptr).tolist()) == [16, 18, R]


@pytest.mark.parametrize("R", [70, 97])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rho,relax", PARAMS)
def test_wide_form_against_lapack_form(R, kind, rho, relax, capsys):
    compare("wide_root%d" % R, kind, rho, relax, capsys)


def test_wide_form_against_lapack_form_on_fam_top(capsys):
    """three wide cliques (130, 130, 110) between narrow ones; one kind: a case takes several seconds on the host"""
    symb = host_symb("fam_top")
    assert sorted(np.diff(symb.rowptr)[np.diff(symb.rowptr) >= WIDE].tolist()) == [110, 130, 130]
    compare("fam_top", "noisy", PARAMS[0][0], PARAMS[0][1], capsys)


def test_plugged_form_leaves_the_host_file_as_it_was():
    wide_restatement(host_symb("wide_root70"), cone_input(host_symb("wide_root70"), "incone"), steps=1)
    assert tch.negative_part is _kernel_or_lapack
