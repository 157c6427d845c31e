"""The host side of the volume fields on the CPU (csrc/sem_volume_plan.cpp,
DESIGN.md §4.14) and their NumPy twin.

tools/volume_check.cpp links the planner alone, with no kernel: the CSR of
the (element, local) entries of every node and the validation of the sizes
and of the map.  The twin (tests/volume_twin.py), the yardstick of the GPU
tests, is checked here first, against the reference golden and against
identities that need no reference: the gradient of a coordinate is a unit
vector, the recovery conserves integrals, and the H1 seminorm is the energy
of the stiffness matrix."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_l2

import sem_oracle
import volume_twin as vt
from spectralelementmethod_amd import _build, meshgen

SEM_E_INVALID, SEM_E_NOTIMPL = -1, -2
CASES = ("sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm")
ORDERS = (1, 2, 8, 12, 16)


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    """tools/volume_check.cpp + the planner, built once with the library's
    compiler"""
    exe = str(tmp_path_factory.mktemp("volume_check") / "volume_check")
    subprocess.run([_build.hipcc(), "-std=c++17", "-O1", "-Wall", "-I" + _build.CSRC,
                    os.path.join(ROOT, "tools", "volume_check.cpp"),
                    os.path.join(_build.CSRC, "sem_volume_plan.cpp"), "-o", exe], check=True)
    return exe


def plan(exe, tmp_path, ndim, p, e2n, n_node, n_elem=None):
    path = str(tmp_path / "e2n.bin")
    np.asarray(e2n, dtype="<u4").tofile(path)
    res = subprocess.run([exe, "plan"] + [str(a) for a in (
        ndim, p, len(e2n) if n_elem is None else n_elem, path, n_node)],
        check=True, capture_output=True, text=True)
    return json.loads(res.stdout)


# --------------------------------------------------------------------------- planner
MESHES = {"square": (2, 3, lambda: meshgen.structured_square(3, 2, 3), 4),
          "cube": (3, 2, lambda: meshgen.structured_cube(2, 2, 2, 2), 8),
          "valence": (2, 4, lambda: meshgen.quads_from_triangles(3, 3, 4), None),
          "shuffled": (2, 3, lambda: meshgen.shuffle_nodes(*meshgen.structured_square(3, 2, 3)), 4)}


@pytest.mark.parametrize("kind", sorted(MESHES))
def test_csr_is_complete_and_ascending(checker, tmp_path, kind):
    ndim, p, make, max_row = MESHES[kind]
    nodes, e2n = make()
    nn = nodes.shape[1]
    out = plan(checker, tmp_path, ndim, p, e2n, nn)
    assert out["rc"] == 0
    flat = np.asarray(e2n).astype(np.int64).ravel()
    ptr, ent = np.array(out["ptr"]), np.array(out["entry"])
    assert ptr.size == nn + 1 and ptr[0] == 0 and ptr[-1] == flat.size
    assert np.array_equal(np.sort(ent), np.arange(flat.size))          # every entry once
    assert np.array_equal(np.diff(ptr), np.bincount(flat, minlength=nn))
    row = np.repeat(np.arange(nn), np.diff(ptr))
    assert np.array_equal(flat[ent], row)                               # in its node's row
    assert np.all(np.diff(ent)[np.diff(row) == 0] > 0)                  # rows ascending
    assert out["n_referenced"] == nn
    assert out["max_row"] == np.diff(ptr).max()
    if max_row is not None:
        assert out["max_row"] == max_row
    else:
        assert len(set(np.diff(ptr).tolist())) > 3                      # valences other than 4


def test_unreferenced_nodes_and_no_elements(checker, tmp_path):
    nodes, e2n = meshgen.structured_square(3, 2, 2)
    nn = nodes.shape[1]
    out = plan(checker, tmp_path, 2, 2, e2n, nn + 3)
    assert out["rc"] == 0 and out["n_referenced"] == nn
    assert out["ptr"][-4:] == [e2n.size] * 4                            # three empty rows
    out = plan(checker, tmp_path, 2, 2, e2n[:0], 4)
    assert out["rc"] == 0 and out["ptr"] == [0] * 5 and out["entry"] == []
    assert out["max_row"] == 0 and out["n_referenced"] == 0
    assert plan(checker, tmp_path, 3, 16, e2n[:0], 0)["ptr"] == [0]


def test_invalid_ids_and_sizes_are_refused(checker, tmp_path):
    nodes, e2n = meshgen.structured_square(3, 2, 2)
    nn = nodes.shape[1]

    def call(ndim=2, p=2, e2n=e2n, nn=nn, n_elem=None):
        return plan(checker, tmp_path, ndim, p, e2n, nn, n_elem)
    assert call()["rc"] == 0
    bad = e2n.copy()
    bad[1, 0, 1] = nn
    for res in (call(e2n=bad), call(nn=nn - 1), call(ndim=4), call(ndim=1), call(p=0),
                call(n_elem=-1), call(nn=-1), call(nn=2 ** 32 + 1),
                call(p=1, n_elem=2 ** 31 // 4), call(ndim=3, p=16, n_elem=2 ** 31 // 4913 + 1)):
        assert res["rc"] == SEM_E_INVALID and res["error"], res
    assert "node id %d" % nn in call(e2n=bad)["error"]
    assert call(p=17)["rc"] == SEM_E_NOTIMPL


# --------------------------------------------------------------------------- twin
def basis_arrays(p, ndim=2):
    from spectralelementmethod_amd.operators import _basis_arrays
    basis, D, w, _ = _basis_arrays(p, None, ndim)
    return basis, D, w


@pytest.mark.parametrize("name", CASES)
def test_twin_meets_the_reference(name):
    g = load_golden("volume.npz")
    p = int(g[name + "_p"])
    _, D, w = basis_arrays(p)
    x_phys, e2n, u = g[name + "_x_phys"], g[name + "_e2n"], g[name + "_u"]
    for dtype in (np.float64, np.longdouble):
        tw = vt.Twin(x_phys, e2n, u.size, D, w, dtype)
        assert rel_l2(tw.gradient(u), g[name + "_gradient"]) <= 1e-12
        assert rel_l2(tw.detJxW, g[name + "_detJxW"]) <= 1e-12
        assert rel_l2(tw.integrate(u)[0], g[name + "_integrate"]) <= 1e-12
        assert rel_l2(tw.integrate_local(np.ones_like(tw.detJxW))[0],
                      g[name + "_integrate_one"]) <= 1e-12
    assert float(g["ref_seconds_per_element"]) > 0


def warped_square(p):
    """The warped 3 x 2 square with the reference's host x_phys."""
    from spectralelementmethod_amd.operators import reference_x_phys
    basis, D, w = basis_arrays(p)
    nodes, e2n = meshgen.structured_square(3, 2, p, warp=0.05)
    x_phys = reference_x_phys(nodes, e2n, basis)
    return x_phys, e2n, nodes.shape[1], D, w


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_twin_identities(p, dtype):
    """The bound is the one the issue states for float64, 5e-16, and the
    extended twin meets it as well.  The isoparametric interpolant of a
    coordinate is the coordinate, so its gradient is invJ . J, the unit
    vector up to the rounding of a cofactor inverse times its own matrix; the
    two sides of the conservation identity are the same products summed in
    another order (relative to the sum of their magnitudes)."""
    x_phys, e2n, nn, D, w = warped_square(p)
    tw = vt.Twin(x_phys, e2n, nn, D, w, dtype)
    xn = vt.node_coordinates(x_phys, e2n, nn)
    for c in range(2):
        g = tw.gradient(xn[c])                                   # [E, 2, n, n]
        unit = np.zeros_like(g)
        unit[:, c] = 1.0
        assert float(np.abs(g - unit).max()) <= 5e-16, (p, c)
    u = vt.smooth(xn)
    rec, grad = tw.recover(u), tw.gradient(u)
    for j in range(2):
        lhs = (tw.mass * rec[j]).sum()
        rhs = tw.integrate_local(grad[:, j])[1]
        scale = np.abs(tw.detJxW * grad[:, j]).sum()
        assert abs(float((lhs - rhs) / scale)) <= 5e-16, (p, j)
    assert abs(float(tw.mass.sum() - tw.detJxW.sum())) <= 5e-16 * float(tw.detJxW.sum())
    per, tot = tw.norms(u, u)
    assert not per.any() and not tot.any()


@pytest.mark.parametrize("p", ORDERS)
def test_twin_h1_is_the_stiffness_energy(p):
    """h1^2 == u . K u with K the oracle's Poisson action on the twin's own
    factors, in float64: the same products summed in another order, with a
    cancellation of only 1.5 inside K u on this mesh.  The bound is the
    issue's 5e-16 relative."""
    x_phys, e2n, nn, D, w = warped_square(p)
    tw = vt.Twin(x_phys, e2n, nn, D, w)
    u = vt.smooth(vt.node_coordinates(x_phys, e2n, nn))
    invJ = np.moveaxis(tw.invJ, 2, 0)                            # [E, i, j, n, n]
    G = sem_oracle.poisson_factors(invJ, tw.detJxW)
    Ku = sem_oracle.poisson_apply(G, D, e2n.astype(np.int64), u, nn)
    h1_sq = tw.norms(u)[1][1]
    gap = abs(float(u @ Ku) - h1_sq) / h1_sq
    print("p = %d: |u.Ku - h1^2| / h1^2 = %.2e" % (p, gap))
    assert gap <= 5e-16
