"""Host side of the block KKT solve (KKTSystem.solve_many): the chunk rule and the two C entry points' declarations.
No device is needed."""
import os
import re

import pytest

from smcp_amd import _lib
from smcp_amd.kkt import solve_many_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fits(c, m, blklen, max_rhs):
    return c + -(-c * m // blklen) <= max_rhs


@pytest.mark.parametrize("m,blklen,max_rhs", [(7, 15, 4), (7, 15, 2), (7, 10 ** 6, 4), (100, 3000, 12), (1000, 1000, 9),
                                              (1, 1, 2), (400, 401, 64), (130, 129, 7)])
def test_chunks_fit_sum_and_are_maximal(m, blklen, max_rhs):
    for nrhs in (1, 2, 3, 5, 9, 17, 64):
        ch = solve_many_chunks(nrhs, m, blklen, max_rhs)
        assert sum(ch) == nrhs and all(c >= 1 for c in ch)
        assert all(fits(c, m, blklen, max_rhs) for c in ch)
        # all but the last are maximal, and no two chunks differ except the last
        for c in ch[:-1]:
            assert not fits(c + 1, m, blklen, max_rhs)
            assert c == ch[0]
        assert ch[-1] <= ch[0]


def test_chunks_of_the_stated_cases():
    # the `diag` pattern: the y temporaries of two right-hand sides cost a whole row of the stack
    assert solve_many_chunks(5, 7, 15, 4) == [2, 2, 1]
    assert solve_many_chunks(9, 7, 10 ** 9, 4) == [3, 3, 3]
    assert solve_many_chunks(1, 7, 15, 4) == [1]


def test_chunks_refuse_a_workspace_that_is_too_small():
    for max_rhs in (1, 0, -3):
        with pytest.raises(Exception):
            solve_many_chunks(3, 7, 15, max_rhs)
    with pytest.raises(Exception):
        solve_many_chunks(3, 40, 15, 3)          # one right-hand side needs 1 + 3 rows
    with pytest.raises(Exception):
        solve_many_chunks(0, 7, 15, 4)


def header_arguments(name):
    src = open(os.path.join(ROOT, "include", "smcp_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    mt = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert mt, name + " is not declared in include/smcp_amd.h"
    return [" ".join(a.split()) for a in mt.group(1).split(",")]


@pytest.mark.parametrize("name,nargs", [("kkt_solve_many", 12), ("dense_potrs_many", 8), ("kkt_solve_many_chunk", 3)])
def test_entry_points_are_declared_and_bound(name, nargs):
    args = header_arguments(name)
    assert len(args) == nargs, args
    assert name in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args)
    # pointers are bound as pointers, 64-bit integers as 64-bit integers, kk as a double
    for a, t in zip(args, argtypes):
        if "*" in a:
            assert t is _lib.c_vp, (a, t)
        elif a.startswith("int64_t"):
            assert t is _lib.c_i64, (a, t)
        elif a.startswith("double"):
            assert t.__name__ == "c_double", (a, t)
    assert hasattr(_lib.lib(), name)


def test_layouts_in_the_header():
    """the argument order the Python method relies on"""
    a = header_arguments("kkt_solve_many")
    assert [x.split()[-1].lstrip("*") for x in a] == ["ctx", "L", "Y", "H", "ldh", "kk", "BX", "ldbx", "BY", "ldby", "nrhs", "stream"]
    a = header_arguments("dense_potrs_many")
    assert [x.split()[-1].lstrip("*") for x in a] == ["ctx", "A", "n", "lda", "B", "nrhs", "ldb", "stream"]
