"""Host side of the block kkt_qr solve (KKTSystem.solve_many_qr): the chunk rule and the two C entry points' declarations.
No device is needed."""
import pytest

from smcp_amd import _lib
from smcp_amd.kkt import solve_many_qr_chunks
from tests.test_solve_many_host import header_arguments


@pytest.mark.parametrize("max_rhs", [1, 2, 3, 4, 12, 16, 17, 20, 64, 1000])
def test_chunks_sum_and_all_but_the_last_are_the_cap(max_rhs):
    cap = int(_lib.lib().kkt_qr_solve_many_chunk(max_rhs))
    assert 1 <= cap <= max_rhs                     # a chunk is never more than the Hessian sweeps take
    for nrhs in (1, 2, 3, 5, 9, 16, 17, 33, 64):
        ch = solve_many_qr_chunks(nrhs, max_rhs)
        assert sum(ch) == nrhs and all(c >= 1 for c in ch)
        assert all(c == cap for c in ch[:-1])
        assert ch[-1] <= cap


def test_chunk_grows_with_the_workspace_until_the_cap():
    lib = _lib.lib()
    caps = [int(lib.kkt_qr_solve_many_chunk(r)) for r in range(1, 200)]
    assert caps == sorted(caps)
    assert caps[0] == 1


def test_chunks_refuse_nothing_to_do_and_no_workspace():
    for nrhs, max_rhs in ((0, 4), (-1, 4), (3, 0), (3, -2)):
        with pytest.raises(Exception):
            solve_many_qr_chunks(nrhs, max_rhs)
    assert int(_lib.lib().kkt_qr_solve_many_chunk(0)) == 0


@pytest.mark.parametrize("name,nargs", [("kkt_qr_solve_many", 10), ("kkt_qr_solve_many_chunk", 1)])
def test_entry_points_are_declared_and_bound(name, nargs):
    args = header_arguments(name)
    assert len(args) == nargs, args
    assert name in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        if "*" in a:
            assert t is _lib.c_vp, (a, t)
        elif a.startswith("int64_t"):
            assert t is _lib.c_i64, (a, t)
        elif a.startswith("double"):
            assert t.__name__ == "c_double", (a, t)
    assert res is (_lib.c_i64 if name.endswith("_chunk") else __import__("ctypes").c_int)
    assert hasattr(_lib.lib(), name)


def test_layout_in_the_header():
    """the argument order the Python method relies on"""
    a = header_arguments("kkt_qr_solve_many")
    assert [x.split()[-1].lstrip("*") for x in a] == ["ctx", "L", "Y", "kk", "BX", "ldbx", "BY", "ldby", "nrhs", "stream"]
    a = header_arguments("kkt_qr_solve_many_chunk")
    assert [x.split()[-1] for x in a] == ["max_rhs"]
