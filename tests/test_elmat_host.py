"""The argument validation of sem_elem_matrices (include/sem_hip.h, "Element
matrices") on the CPU: every refusal is returned with NULL device pointers,
or with pointers that are never dereferenced, so the check happens before any
device call.  The kernel itself is tested in tests/test_gpu_elmat.py."""
import ctypes as C

import numpy as np
import pytest

from spectralelementmethod_amd import _lib

POISSON, STOKES, NS, JVP = (_lib.OP_POISSON, _lib.OP_AXISYM_STOKES, _lib.OP_AXISYM_NS,
                            _lib.OP_AXISYM_NS_JVP)
INVALID, NOTIMPL = _lib.SEM_E_INVALID, _lib.SEM_E_NOTIMPL


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, kind=POISSON, ndim=2, p=4, n_elem=6, x=64, D=True, w=True, re=0.0, e2n=64,
         state=None, order=None, begin=0, count=6, mat=64, rhs=None):
    """sem_elem_matrices with dummy device addresses (never dereferenced:
    validation comes first); None is a NULL pointer."""
    n = max(p, 1) + 1
    hD = np.zeros((n, n))
    hw = np.zeros(n)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    vp = lambda a: None if a is None else C.c_void_p(a)  # noqa: E731
    return lib.sem_elem_matrices(
        kind, ndim, p, n_elem, vp(x), _lib.dptr(hD) if D else None, _lib.dptr(hw) if w else None,
        re, vp(e2n), vp(state), None if o is None else o.ctypes.data_as(C.POINTER(C.c_int32)),
        begin, count, vp(mat), vp(rhs), None)


def test_symbol_is_exported_and_declared(lib):
    assert "sem_elem_matrices" in _lib.SIGNATURES
    assert hasattr(lib, "sem_elem_matrices")
    assert len(_lib.SIGNATURES["sem_elem_matrices"][1]) == 16


def test_null_device_pointers_everywhere(lib):
    """All device pointers NULL: each scalar refusal still comes back as
    itself, a plain call as SEM_E_INVALID (NULL array)."""
    null = dict(x=None, e2n=None, mat=None)
    assert call(lib, **null) == INVALID and "NULL" in _lib.last_error()
    assert call(lib, p=17, **null) == NOTIMPL
    assert call(lib, ndim=3, **null) == NOTIMPL
    assert call(lib, kind=JVP, **null) == NOTIMPL
    assert call(lib, p=0, **null) == INVALID and "p must be >= 1" in _lib.last_error()
    assert call(lib, begin=1, count=6, **null) == INVALID and "range" in _lib.last_error()
    assert call(lib, order=[0] * 25, **null) == INVALID and "permutation" in _lib.last_error()


@pytest.mark.parametrize("missing", ["x", "e2n", "mat", "D", "w"])
def test_each_null_array(lib, missing):
    kw = {missing: None if missing in ("x", "e2n", "mat") else False}
    assert call(lib, **kw) == INVALID and "NULL" in _lib.last_error()


@pytest.mark.parametrize("p", [0, -1, -7])
def test_order_below_one(lib, p):
    assert call(lib, p=p) == INVALID and "p must be >= 1" in _lib.last_error()


@pytest.mark.parametrize("p", [17, 18, 64])
def test_order_above_sixteen(lib, p):
    assert call(lib, p=p) == NOTIMPL and "p must be <= 16" in _lib.last_error()


@pytest.mark.parametrize("ndim", [1, 3, 0])
def test_only_quadrilaterals(lib, ndim):
    assert call(lib, ndim=ndim) == NOTIMPL and "ndim" in _lib.last_error()


def test_kinds(lib):
    assert call(lib, kind=JVP, state=64) == NOTIMPL
    assert call(lib, kind=7) == INVALID and "op_kind" in _lib.last_error()
    assert call(lib, kind=-1) == INVALID
    assert call(lib, kind=NS) == INVALID and "needs d_state" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(lib, kind=JVP))
    with pytest.raises(ValueError):
        _lib.check(call(lib, kind=NS))


@pytest.mark.parametrize("begin,count,n_elem", [(-1, 2, 6), (0, 7, 6), (6, 1, 6), (7, 0, 6),
                                                (3, -1, 6), (2, 5, 6), (0, 1, -1),
                                                (2 ** 62, 2 ** 62, 2 ** 62)])
def test_ranges_outside_the_mesh(lib, begin, count, n_elem):
    assert call(lib, begin=begin, count=count, n_elem=n_elem) == INVALID
    assert "range" in _lib.last_error()


@pytest.mark.parametrize("kind,nl", [(POISSON, 25), (STOKES, 50)])
def test_orders_that_are_no_permutation(lib, kind, nl):
    ident = np.arange(nl)
    for bad in (np.where(ident == 3, 4, ident),           # a repeat
                np.where(ident == nl - 1, nl, ident),     # past the end
                np.where(ident == 0, -1, ident)):         # negative
        assert call(lib, kind=kind, order=bad) == INVALID
        assert "permutation" in _lib.last_error()


def test_rhs_needs_a_state(lib):
    for kind in (POISSON, STOKES, NS):
        assert call(lib, kind=kind, rhs=64) == INVALID and "d_state" in _lib.last_error()


def test_empty_range_is_valid_and_launches_nothing(lib):
    """count == 0 passes every check and returns before the launch (no device
    is touched: this runs on a host without one)."""
    assert call(lib, count=0) == _lib.SEM_OK
    assert call(lib, begin=6, count=0) == _lib.SEM_OK
    assert call(lib, kind=NS, state=64, rhs=64, count=0, order=np.arange(50)[::-1]) == _lib.SEM_OK
