"""Host side of the block KKT residual and refinement (KKTSystem.residual_many / refine_many): the declarations of the two C entry
points and their bindings.  No device is needed."""
import ctypes

import pytest

from smcp_amd import _lib
from smcp_amd.kkt import KKTSystem
from tests.test_solve_many_host import header_arguments


@pytest.mark.parametrize("name,nargs", [("kkt_residual_many", 19), ("kkt_update_many", 11)])
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
            assert t is ctypes.c_double, (a, t)
        else:
            raise AssertionError("unexpected argument " + a)
    assert res is ctypes.c_int
    assert hasattr(_lib.lib(), name)


def test_layout_in_the_header():
    """the argument order the Python methods rely on"""
    a = header_arguments("kkt_residual_many")
    assert [x.split()[-1].lstrip("*") for x in a] == ["ctx", "L", "Y", "kk", "XS", "ldxs", "YS", "ldys", "BX", "ldbx", "BY", "ldby",
                                                      "RX", "ldrx", "RY", "ldry", "norms", "nrhs", "stream"]
    # the inputs are declared read-only, the three outputs are not
    for x in a[1:3] + a[4:12:2]:
        assert x.startswith("const double*"), x
    for x in a[12:17:2]:
        assert x.startswith("double*"), x
    a = header_arguments("kkt_update_many")
    assert [x.split()[-1].lstrip("*") for x in a] == ["ctx", "XS", "ldxs", "YS", "ldys", "DX", "lddx", "DY", "lddy", "nrhs", "stream"]


def test_the_entry_point_refuses_to_run_without_a_context():
    """no CPU route: a null context is SMCP_EINVAL before anything else is looked at"""
    assert _lib.lib().kkt_residual_many(None, None, None, 1.0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 1, None) == -1
    assert _lib.lib().kkt_update_many(None, None, 0, None, 0, None, 0, None, 0, 1, None) == -1


def test_python_methods_exist():
    for name in ("residual_many", "residual", "refine_many"):
        assert callable(getattr(KKTSystem, name))
