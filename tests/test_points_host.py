"""CPU checks of the point-location feature: ``Mapping.inv`` (NumPy, one
point in one element) against the reference's xi on golden x_phys, the
argument validation of the sem_points_* C ABI (no device is touched), and the
fixture's own recorded quality.  tests/golden/points.npz comes from
tests/golden/make_points_golden.py (the reference's
find_elem_containing_point / interpolate)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

CASES = ("sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm")


@pytest.fixture(scope="module")
def pts():
    return load_golden("points.npz")


def _mapping(pts, case, e):
    from spectralelementmethod_amd.basis_functions import LagrangeGaussLobatto, TensorProductQS
    from spectralelementmethod_amd.mapping import Mapping
    b = LagrangeGaussLobatto(int(pts[case + "_p"]))
    return Mapping(TensorProductQS(b, b), {"x_phys": pts[case + "_x_phys"]}, e, {"x_phys": True})


def test_fixture_lists_its_cases(pts):
    assert tuple(pts["cases"]) == CASES
    assert float(pts["ref_seconds_per_point"]) > 0
    for case in CASES:
        assert pts[case + "_xq"].shape == (2, 64)
        assert pts[case + "_interior"].sum() >= 32


@pytest.mark.parametrize("case", CASES)
def test_reference_round_trip_recorded(pts, case):
    assert float(pts[case + "_roundtrip"]) <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_mapping_inv_matches_reference(pts, case):
    xq, elem, xi_ref = pts[case + "_xq"], pts[case + "_elem"], pts[case + "_xi"]
    maps = {}
    err = 0.0
    for k in range(xq.shape[1]):
        m = maps.setdefault(int(elem[k]), _mapping(pts, case, int(elem[k])))
        xi = m.inv(xq[:, k])
        assert xi.shape == (2,)
        err = max(err, float(np.abs(xi - xi_ref[:, k]).max()))
    print("%s: max |xi - xi_ref| = %.3e" % (case, err))
    assert err <= 1e-12


@pytest.mark.parametrize("case,nb", (("sq_p4", 2), ("ann_p6", 3)))
def test_mapping_inv_outside_domain(pts, case, nb):
    """A point of the neighbour across element 0's xi0 = +1 face (element
    ``nb`` of the structured mesh) converges outside [-1, 1]^2 in element 0:
    OutsideDomain, the mapping module's class."""
    from spectralelementmethod_amd import discrete, mapping
    assert discrete.OutsideDomain is not mapping.OutsideDomain
    xi_nb = np.array([-0.7, 0.1])
    x = np.asarray(_mapping(pts, case, nb)(xi_nb)).reshape(2)
    m = _mapping(pts, case, 0)
    with pytest.raises(mapping.OutsideDomain):
        m.inv(x)
    # in its own element the point is found, also from a guess
    assert np.abs(_mapping(pts, case, nb).inv(x) - xi_nb).max() <= 1e-12
    xi = _mapping(pts, case, nb).inv(x, x_param_guess=np.array([0.1, -0.1]))
    assert np.abs(xi - xi_nb).max() <= 1e-12


def test_rootfind_solver_failure():
    from spectralelementmethod_amd import rootfind
    with pytest.raises(rootfind.SolverFailure):
        # x^2 + 1 has no real root: Newton cannot meet the tolerance
        rootfind.newton(lambda x: x * x + 1.0, np.array([0.7]),
                        lambda x: np.array([[2.0 * x[0]]]), it_max=8, tol=1e-8)
    x = rootfind.newton(lambda x: x * x - 2.0, np.array([1.0]),
                        lambda x: np.array([[2.0 * x[0]]]), it_max=8, tol=1e-8)
    assert abs(x[0] - np.sqrt(2.0)) < 1e-14


def test_points_abi_validation():
    """Bad arguments are refused before any device call."""
    from spectralelementmethod_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    dummy = C.c_void_p(64)  # never dereferenced: validation comes first
    assert lib.sem_points_create(C.byref(h), 4, 4, 6, dummy, 0, None) == _lib.SEM_E_INVALID
    assert "ndim" in _lib.last_error()
    assert lib.sem_points_create(C.byref(h), 1, 4, 6, dummy, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(C.byref(h), 2, 17, 6, dummy, 0, None) == _lib.SEM_E_NOTIMPL
    assert lib.sem_points_create(C.byref(h), 2, 0, 6, dummy, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(C.byref(h), 2, 4, 0, dummy, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(C.byref(h), 2, 4, -3, dummy, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(C.byref(h), 3, 4, 6, None, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(None, 2, 4, 6, dummy, 0, None) == _lib.SEM_E_INVALID
    assert lib.sem_points_create(C.byref(h), 2, 4, 6, dummy, -1, None) == _lib.SEM_E_INVALID
    assert not h.value
    n_out = C.c_int64(7)
    assert lib.sem_points_locate(None, 4, dummy, dummy, dummy, C.byref(n_out), None) \
        == _lib.SEM_E_INVALID
    assert lib.sem_points_invert(None, 4, dummy, dummy, None, dummy, None, None) \
        == _lib.SEM_E_INVALID
    assert lib.sem_points_map(None, 4, dummy, dummy, dummy, None) == _lib.SEM_E_INVALID
    plan = C.c_void_p()
    assert lib.sem_points_plan(None, 4, dummy, C.byref(plan), None) == _lib.SEM_E_INVALID
    assert lib.sem_points_plan(None, -1, dummy, C.byref(plan), None) == _lib.SEM_E_INVALID
    assert not plan.value
    # a negative or too large count is refused as such, ahead of every other check
    for n_bad in (-1, -2 ** 40, 2 ** 31):
        assert lib.sem_points_locate(None, n_bad, dummy, dummy, dummy, None, None) \
            == _lib.SEM_E_INVALID and "n_pts" in _lib.last_error()
        assert lib.sem_points_invert(None, n_bad, dummy, dummy, None, dummy, None, None) \
            == _lib.SEM_E_INVALID and "n_pts" in _lib.last_error()
        assert lib.sem_points_map(None, n_bad, dummy, dummy, dummy, None) \
            == _lib.SEM_E_INVALID and "n_pts" in _lib.last_error()
        assert lib.sem_points_plan(None, n_bad, dummy, C.byref(plan), None) \
            == _lib.SEM_E_INVALID and "n_pts" in _lib.last_error()
    assert lib.sem_points_eval(None, dummy, dummy, 1, 1, 1, dummy, dummy, None) \
        == _lib.SEM_E_INVALID
    info = (C.c_int64 * 4)()
    assert lib.sem_points_info(None, info, 4) == _lib.SEM_E_INVALID
    assert lib.sem_points_plan_info(None, info, 4) == _lib.SEM_E_INVALID
    lib.sem_points_destroy(None)
    lib.sem_points_plan_destroy(None)
    with pytest.raises(ValueError):
        _lib.check(lib.sem_points_create(C.byref(h), 4, 4, 6, dummy, 0, None))
    with pytest.raises(NotImplementedError):
        _lib.check(lib.sem_points_create(C.byref(h), 2, 17, 6, dummy, 0, None))
