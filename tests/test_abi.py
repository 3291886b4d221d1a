"""The C-ABI library loads without a GPU and exports every symbol include/smcp_amd.h declares;
compute entry points refuse to run without a device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import torch

from smcp_amd import _lib, problems
from smcp_amd.symbolic import Symbolic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "smcp_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b((?:csp|kkt|dense)_[a-z_0-9]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, "no ctypes signature for " + n


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        return
    symb = Symbolic(problems.band_pattern(10, 2))
    x = np.ones(symb.blklen)
    rc = _lib.lib().csp_cholesky(symb.handle, x.ctypes.data, None)
    assert rc == -2                                   # SMCP_ENODEV: context has no device
    assert _lib.lib().csp_device_init(symb.handle, 0, 1) == -2


def test_slot_doubles_tune_and_its_two_counters():
    """CSP_TUNE_SLOT_DOUBLES needs no device and refuses a negative value; CSP_Q_SLOT_SHARE and CSP_Q_CEIG_GROUPS answer 0 on
    a context that made no such call; header and Python layer carry the same numbers and document them"""
    from smcp_amd import chordal
    src = open(os.path.join(ROOT, "include", "smcp_amd.h")).read()
    assert re.search(r"#define\s+CSP_TUNE_SLOT_DOUBLES\s+8\b", src) and chordal.TUNE_SLOT_DOUBLES == 8
    assert re.search(r"\bCSP_Q_SLOT_SHARE\s*=\s*22\b", src) and re.search(r"\bCSP_Q_CEIG_GROUPS\s*=\s*23\b", src)
    assert "TUNE_SLOT_DOUBLES" in chordal.tune.__doc__ and chordal.slot_share.__doc__ and chordal.clique_eig_groups.__doc__
    symb = Symbolic(problems.band_pattern(10, 2))
    L = _lib.lib()
    assert L.csp_tune(symb.handle, 8, -1) == -1       # SMCP_EINVAL
    for value in (1, 2 ** 40, 0):
        assert L.csp_tune(symb.handle, 8, value) == 0
    for what in (22, 23):
        out = ctypes.c_int64(-1)
        assert L.csp_symbolic_query(symb.handle, what, ctypes.byref(out)) == 1 and out.value == 0
    assert L.csp_symbolic_query(symb.handle, 24, None) == -1
