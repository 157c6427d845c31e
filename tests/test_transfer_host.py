"""The host side of the order transfer on the CPU (csrc/sem_transfer_plan.cpp,
DESIGN.md §4.13) and its NumPy twin.

tools/transfer_check.cpp links the planner with the host basis tables and no
kernel: the owner mask of the "to" map, the CSR of the "from" nodes, the
validation of the two maps and the 1-D matrix J of all 256 order pairs.  The
np.longdouble twin (tests/transfer_twin.py), the yardstick of the GPU tests,
is checked here first: polynomial exactness, adjointness and the conservation
of the load (the transpose's scaling)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import transfer_twin as tw
from spectralelementmethod_amd import _build
from transfer_twin import mesh_pair

SEM_E_INVALID, SEM_E_NOTIMPL = -1, -2
PAIRS = [(1, 2), (2, 1), (4, 8), (16, 15)]


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    """tools/transfer_check.cpp + the planner + the basis tables, built once
    with the library's compiler"""
    exe = str(tmp_path_factory.mktemp("transfer_check") / "transfer_check")
    subprocess.run([_build.hipcc(), "-std=c++17", "-O1", "-Wall", "-I" + _build.CSRC,
                    os.path.join(ROOT, "tools", "transfer_check.cpp"),
                    os.path.join(_build.CSRC, "sem_transfer_plan.cpp"),
                    os.path.join(_build.CSRC, "sem_basis.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True)
    return json.loads(res.stdout)


def plan(exe, tmp_path, ndim, p_from, p_to, ef, nnf, et, nnt, n_elem=None):
    a, b = str(tmp_path / "from.bin"), str(tmp_path / "to.bin")
    np.asarray(ef, dtype="<u4").tofile(a)
    np.asarray(et, dtype="<u4").tofile(b)
    return run(exe, "plan", ndim, p_from, p_to, len(ef) if n_elem is None else n_elem, a, nnf, b,
               nnt)


# --------------------------------------------------------------------------- planner
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("p_from,p_to", PAIRS)
def test_owner_is_the_lowest_pair_and_the_csr_is_ascending(checker, tmp_path, ndim, p_from, p_to):
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to)
    nnf, nnt = nf.shape[1], nt.shape[1]
    out = plan(checker, tmp_path, ndim, p_from, p_to, ef, nnf, et, nnt)
    assert out["rc"] == 0
    own = np.array(out["owner"], dtype=bool)
    flat_to = et.astype(np.int64).ravel()
    # every "to" node has exactly one owner ...
    assert np.array_equal(np.bincount(flat_to[own], minlength=nnt), np.ones(nnt, dtype=np.int64))
    assert out["n_owned"] == nnt == own.sum()
    # ... and it is the lowest (element, local) entry that names the node
    first = np.full(nnt, flat_to.size, dtype=np.int64)
    np.minimum.at(first, flat_to, np.arange(flat_to.size))
    assert np.array_equal(np.flatnonzero(own), np.sort(first))
    assert np.array_equal(own.reshape(et.shape), tw.owner_mask(et))
    # the CSR: every (element, local) entry of the "from" map once, rows ascending
    flat_from = ef.astype(np.int64).ravel()
    ptr, ent = np.array(out["ptr"]), np.array(out["entry"])
    assert ptr.size == nnf + 1 and ptr[0] == 0 and ptr[-1] == flat_from.size
    assert np.array_equal(np.sort(ent), np.arange(flat_from.size))
    assert np.array_equal(np.diff(ptr), np.bincount(flat_from, minlength=nnf))
    assert np.array_equal(flat_from[ent], np.repeat(np.arange(nnf), np.diff(ptr)))
    same_row = np.repeat(np.arange(nnf), np.diff(ptr))
    assert np.all(np.diff(ent)[np.diff(same_row) == 0] > 0)
    assert out["max_row"] == np.diff(ptr).max() == 2 ** ndim


def test_unreferenced_nodes_and_no_elements(checker, tmp_path):
    (nf, ef), (nt, et) = mesh_pair(2, 2, 3)
    out = plan(checker, tmp_path, 2, 2, 3, ef, nf.shape[1] + 2, et, nt.shape[1] + 5)
    assert out["rc"] == 0 and out["n_owned"] == nt.shape[1]
    assert out["ptr"][-3:] == [ef.size] * 3            # two empty rows at the end
    out = plan(checker, tmp_path, 2, 2, 3, ef[:0], 4, et[:0], 9)
    assert out["rc"] == 0 and out["ptr"] == [0] * 5 and out["owner"] == [] and out["max_row"] == 0


def test_invalid_ids_and_sizes_are_refused(checker, tmp_path):
    (nf, ef), (nt, et) = mesh_pair(2, 2, 3)
    nnf, nnt = nf.shape[1], nt.shape[1]

    def call(ndim=2, p_from=2, p_to=3, ef=ef, nnf=nnf, et=et, nnt=nnt, n_elem=None):
        return plan(checker, tmp_path, ndim, p_from, p_to, ef, nnf, et, nnt, n_elem)
    assert call()["rc"] == 0
    bad_from, bad_to = ef.copy(), et.copy()
    bad_from[1, 0, 1] = nnf
    bad_to[-1, -1, -1] = nnt
    for bad in (call(ef=bad_from), call(et=bad_to), call(nnf=nnf - 1), call(nnt=nnt - 1),
                call(ndim=4), call(ndim=1), call(p_from=0), call(p_to=0), call(n_elem=-1),
                call(nnf=-1), call(nnt=2 ** 32 + 1),
                call(p_to=1, n_elem=2 ** 31 // 9 + 1), call(p_from=1, n_elem=2 ** 31 // 16)):
        assert bad["rc"] == SEM_E_INVALID and bad["error"], bad
    assert "from" in call(ef=bad_from)["error"] and "to" in call(et=bad_to)["error"]
    assert call(p_from=17)["rc"] == SEM_E_NOTIMPL
    assert call(p_to=17)["rc"] == SEM_E_NOTIMPL


# --------------------------------------------------------------------------- J
def test_interpolation_matrix_of_all_256_pairs(checker):
    pairs = run(checker, "matrices")["pairs"]
    assert len(pairs) == 256
    for rec in pairs:
        pf, pt = rec["p_from"], rec["p_to"]
        J = np.array(rec["J"]).reshape(pt + 1, pf + 1)
        assert np.abs(J.sum(axis=1) - 1.0).max() <= 1e-14, (pf, pt)
        # the end nodes coincide: exact unit rows
        assert J[0].tolist() == [1.0] + [0.0] * pf and J[-1].tolist() == [0.0] * pf + [1.0]
        if pf == pt:
            assert np.array_equal(J, np.eye(pf + 1))
        # float64 barycentric evaluation against the extended-precision twin
        assert np.abs(J - tw.interp_matrix(pf, pt)).max() <= 1e-13, (pf, pt)
    one = run(checker, "matrix", 4, 8)
    assert np.array_equal(np.array(one["Jt"]).reshape(5, 9), np.array(one["J"]).reshape(9, 5).T)
    assert run(checker, "matrix", 17, 2)["rc"] == SEM_E_NOTIMPL
    assert run(checker, "matrix", 0, 2)["rc"] == SEM_E_INVALID


# --------------------------------------------------------------------------- twin
def rel_l2_ext(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("p_from,p_to", PAIRS)
def test_twin_prolongs_polynomials_exactly(ndim, p_from, p_to):
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to)
    xf, xt = tw.gll_points(nf, ef), tw.gll_points(nt, et)
    deg = min(p_from, p_to)
    t = tw.Twin(ef, nf.shape[1], et, nt.shape[1])
    got = t.prolong(tw.product_polynomial(xf, deg))
    err = rel_l2_ext(got, tw.product_polynomial(xt, deg))
    print("ndim %d p %d -> %d: polynomial of degree %d prolonged to %.2e" % (ndim, p_from, p_to,
                                                                            deg, err))
    assert err <= 1e-12


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("p_from,p_to", PAIRS)
def test_twin_restrict_is_the_adjoint(ndim, p_from, p_to):
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to)
    rng = np.random.default_rng(5)
    u, r = rng.standard_normal(nf.shape[1]), rng.standard_normal(nt.shape[1])
    t = tw.Twin(ef, nf.shape[1], et, nt.shape[1])
    Pu, Ptr = t.prolong(u), t.restrict(r)
    lhs, rhs = np.dot(Pu, r.astype(np.longdouble)), np.dot(u.astype(np.longdouble), Ptr)
    bound = 1e-13 * float(np.linalg.norm(Pu.astype(np.float64))) * float(np.linalg.norm(r))
    assert abs(float(lhs - rhs)) <= bound, (float(lhs - rhs), bound)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("p_from,p_to", [(1, 2), (4, 8)])
def test_twin_restrict_conserves_the_load(ndim, p_from, p_to):
    (nf, ef), (nt, et) = mesh_pair(ndim, p_from, p_to)
    t = tw.Twin(ef, nf.shape[1], et, nt.shape[1])
    got = t.restrict(tw.assembled_detJxW(nt, et))
    ref = tw.assembled_detJxW(nf, ef)
    assert abs(float(ref.sum()) - 2.0 ** ndim) <= 1e-13
    err = rel_l2_ext(got, ref)
    print("ndim %d p %d -> %d: load restricted to %.2e" % (ndim, p_from, p_to, err))
    assert err <= 1e-12
