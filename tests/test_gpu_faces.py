"""GPU tests of the boundary faces (faces.FaceSet, sem_faces_* in
include/sem_hip.h) against

* the reference's own SubFiniteElement results (tests/golden/faces.npz);
* the NumPy twin of the stated formulas (tests/faces_twin.py) in float64 and
  in np.longdouble, fed the same float64 x_phys as the device;
* identities: closed surfaces, neighbours' normals, polynomial exactness.

``parity`` is the project's assert_parity rule (tests/test_gpu_axisym_orders.py):
<= 1e-12 relative L2 against the reference or the extended-precision twin,
else at least as accurate as the float64 twin, and <= 1e-10 in any case."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden, rel_l2

import faces_twin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = ("sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm")
TOL_PARITY = 1e-12
TOL_NORTH_STAR = 1e-10
GEOM_KEYS = ("x_phys", "n_dS", "dS", "dSxW", "unit_normal")


@pytest.fixture(scope="module")
def sem():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import operators
    return operators


@pytest.fixture(scope="module")
def fmod(sem):
    from spectralelementmethod_amd import faces
    return faces


@pytest.fixture(scope="module")
def golden():
    return load_golden("faces.npz")


def parity(y, ext, f64, what, golden=None):
    y = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    ext = np.asarray(ext, dtype=np.float64)
    e_self, e_64x = rel_l2(y, ext), rel_l2(np.asarray(f64, dtype=np.float64), ext)
    e_gold = rel_l2(y, golden) if golden is not None else np.inf
    print("%s: device to extended %.2e, to reference %.2e, float64 twin to extended %.2e"
          % (what, e_self, e_gold, e_64x))
    assert e_self <= TOL_NORTH_STAR, (what, e_self)
    if e_self <= TOL_PARITY or e_gold <= TOL_PARITY:
        return e_self
    assert e_self <= max(1.5 * e_64x, TOL_PARITY), (what, e_self, e_64x)
    return e_self


def basis_arrays(p, ndim):
    from spectralelementmethod_amd.operators import _basis_arrays
    _, D, w, _ = _basis_arrays(p, None, ndim)
    return D, w


def all_faces(E, ndim):
    return np.repeat(np.arange(E), 2 * ndim), np.tile(np.arange(2 * ndim), E)


def smooth(nodes):
    s = np.sin(nodes[0]) + np.cos(2.0 * nodes[1]) + 0.25 * nodes[0] * nodes[1]
    return s + np.sin(0.7 * nodes[2]) * nodes[0] if nodes.shape[0] == 3 else s


class Case(object):
    """Operator, all faces of all elements, and both twins on the device's
    own float64 x_phys; built once per (ndim, p, warp) and shared."""

    def __init__(self, sem, ndim, p, warp=0.05, ne=2):
        from spectralelementmethod_amd import meshgen
        if ndim == 2:
            self.nodes, self.e2n = meshgen.structured_square(ne, ne, p, warp=warp)
        else:
            self.nodes, self.e2n = meshgen.structured_cube(ne, ne, ne, p, warp=warp)
        self.ndim, self.p = ndim, p
        self.op = sem.SEMOperator(p, self.e2n, self.nodes)
        self.xp = self.op.geometry_fields()["x_phys"].cpu().numpy()
        self.elem, self.face = all_faces(self.e2n.shape[0], ndim)
        self.fs = self.op.face_set(self.elem, self.face)
        self.D, self.w = self.op.D, self.op.w
        self.u = smooth(self.nodes)
        self.t64 = faces_twin.Twin(self.xp, self.D, self.w, self.elem, self.face)
        self.tld = faces_twin.Twin(self.xp, self.D, self.w, self.elem, self.face, np.longdouble)


_CASES = {}


def case(sem, ndim, p, warp=0.05):
    key = (ndim, p, warp)
    if key not in _CASES:
        _CASES[key] = Case(sem, ndim, p, warp)
    return _CASES[key]


# ---------------------------------------------------------------- reference parity
@pytest.mark.parametrize("name", CASES)
def test_reference_parity(sem, fmod, golden, name):
    p = int(golden[name + "_p"])
    xp, e2n, u = golden[name + "_x_phys"], golden[name + "_e2n"], golden[name + "_u"]
    E = xp.shape[0]
    elem, face = all_faces(E, 2)
    fs = fmod.FaceSet(x_phys=xp, e2n=e2n, elem=elem, face=face, n_node=u.size)
    assert fs.info() == dict(ndim=2, p=p, faces=4 * E, nodes_per_face=p + 1,
                             distinct_nodes=np.unique(golden[name + "_face_node_ind"]).size,
                             max_contributions=fs.info()["max_contributions"],
                             max_node=int(golden[name + "_face_node_ind"].max()))
    assert np.array_equal(fs.node_ind.cpu().numpy(), golden[name + "_face_node_ind"])
    for key in GEOM_KEYS:
        e = rel_l2(getattr(fs, key).cpu().numpy(), golden[name + "_face_" + key])
        print("%s %s: device to reference %.2e" % (name, key, e))
        assert e <= TOL_PARITY, (key, e)
    D, w = basis_arrays(p, 2)
    t64 = faces_twin.Twin(xp, D, w, elem, face)
    tld = faces_twin.Twin(xp, D, w, elem, face, np.longdouble)
    parity(fs.gradient(u), tld.gradient(u, e2n)[0], t64.gradient(u, e2n)[0],
           name + " gradient", golden[name + "_face_gradient"])
    one = np.ones((4 * E, p + 1))
    per, tot = fs.integrate(one, return_per_face=True)
    parity(per, tld.integrate(one)[0], t64.integrate(one)[0], name + " integrate",
           golden[name + "_face_integrate"])
    assert abs(tot - golden[name + "_face_integrate"].sum()) <= 1e-12 * abs(tot)


def _dofmanager(golden, case):
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManager, Mesh
    p = int(golden[case + "_p"])
    if case.endswith("_rcm"):
        base = case[:-4]
        dm = DOFManager(Mesh.from_arrays(golden[base + "_nodes"], golden[base + "_e2n"]), 1,
                        gll_basis_2d(p), rcm_order=True)
        assert np.array_equal(dm.mesh.element_map(), golden[case + "_e2n"])
        return dm
    return DOFManager(Mesh.from_arrays(golden[case + "_nodes"], golden[case + "_e2n"]), 1,
                      gll_basis_2d(p), rcm_order=False)


@pytest.mark.parametrize("name", CASES)
def test_sub_fe_reference_parity(sem, golden, name):
    """The reference's fe.sub_fe(face) on every face of every element, served
    from the DOFManager's one batched FaceSet (geometry from the mesh nodes)."""
    dm = _dofmanager(golden, name)
    u = golden[name + "_u"]
    got = {k: [] for k in GEOM_KEYS + ("node_ind", "gradient", "integrate")}
    n = int(golden[name + "_p"]) + 1
    for fe in dm.finite_elements(x_phys=True, Jacobian=True):
        for face in range(4):
            sub = fe.sub_fe(face)
            assert sub.parent_fe is fe and sub.ndim == 1 and sub.n_nodes == n
            for k in GEOM_KEYS + ("node_ind",):
                got[k].append(getattr(sub, k))
            got["gradient"].append(sub.gradient(u[fe.node_ind]))
            got["integrate"].append(sub.integrate(np.ones(n)))
            assert np.array_equal(sub.slice_from_parent(fe.node_ind), sub.node_ind)
            assert np.array_equal(fe.node_ind.ravel()[sub.parent_dofs()], sub.node_ind)
            assert np.allclose(sub.n_dSxW, sub.n_dS * fe.quadrature.weights[0], rtol=1e-14)
            sm = fe.mapping.get_submapping(face)
            assert np.array_equal(sm.n_dS, sub.n_dS) and sm.J.shape == (2, 2, n)
            assert rel_l2(sm.detJ, sub.slice_from_parent(fe.mapping.detJ)) <= 1e-13
            assert rel_l2(sm.invJ, sub.slice_from_parent(fe.invJ)) <= 1e-13
            with pytest.raises(NotImplementedError):
                sm.inv(np.zeros(2))
    assert dm._all_faces() is dm._all_faces()  # one batched set, built once
    assert np.array_equal(np.stack(got["node_ind"]), golden[name + "_face_node_ind"])
    for k in GEOM_KEYS + ("gradient", "integrate"):
        e = rel_l2(np.stack(got[k]), golden[name + "_face_" + k])
        print("%s sub_fe %s: to reference %.2e" % (name, k, e))
        assert e <= TOL_PARITY, (k, e)


def test_boundary_elements_on_a_tagged_msh(sem):
    """DOFManager.boundary_elements / FiniteElement.boundary_elements /
    boundary_face_set on the tagged sides of a Gmsh fixture against the twin."""
    from spectralelementmethod_amd import grid_importers
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManager
    mesh = grid_importers.load_msh(os.path.join(GOLDEN, "mesh_sq_p4.msh"), 2)
    dm = DOFManager(mesh, 1, gll_basis_2d(4))
    xp = dm.geometry_fields()["x_phys"]
    e2n = mesh.element_map()
    D, w = basis_arrays(4, 2)
    u = smooth(mesh.nodes)
    for name in ("ebc", "nbc"):
        elem, face = mesh.boundary_faces(name)
        assert elem.size == 5                                  # 3 x 2 cells: 3 + 2 sides
        t64 = faces_twin.Twin(xp, D, w, elem, face)
        tld = faces_twin.Twin(xp, D, w, elem, face, np.longdouble)
        pairs = list(dm.boundary_elements(name, x_phys=True, Jacobian=True))
        assert [(fe._index, sub.face) for fe, sub in pairs] == \
            list(zip(elem.tolist(), face.tolist()))
        assert np.array_equal(np.stack([s.node_ind for _, s in pairs]), t64.node_ind(e2n))
        for key in GEOM_KEYS:
            parity(np.stack([getattr(s, key) for _, s in pairs]), getattr(tld, key),
                   getattr(t64, key), "%s %s" % (name, key))
        parity(np.stack([s.gradient(u[fe.node_ind]) for fe, s in pairs]),
               tld.gradient(u, e2n)[0], t64.gradient(u, e2n)[0], name + " gradient")
        parity(np.stack([s.integrate(s.x_phys[0] ** 2) for _, s in pairs]),
               tld.integrate(tld.x_phys[:, 0] ** 2)[0], t64.integrate(t64.x_phys[:, 0] ** 2)[0],
               name + " integrate")
        # the element's own iterator gives the same sub-elements
        fe0 = pairs[0][0]
        own = list(fe0.boundary_elements(name))
        mine = [s for fe, s in pairs if fe._index == fe0._index]
        assert len(own) == len(mine) >= 1
        for a, b in zip(own, mine):
            assert rel_l2(a.n_dS, b.n_dS) <= 1e-15 and np.array_equal(a.node_ind, b.node_ind)
        fs = dm.boundary_face_set(name)
        assert fs is dm.boundary_face_set(name) and len(fs) == 5
        assert abs(float(fs.integrate(torch.ones_like(fs.dS))) - 4.0) <= 1e-12  # two sides of 2
    with pytest.raises(KeyError):
        dm.boundary_face_set("nowhere")


# ---------------------------------------------------------------- every order
@pytest.mark.parametrize("p", list(range(1, 17)))
@pytest.mark.parametrize("ndim", [2, 3])
def test_all_orders(sem, ndim, p):
    """All faces of all elements of a 2 x 2 (x 2) warped mesh.  The flux
    total is a sum of per-face fluxes of both signs, so it is held to 1e-12 of
    the sum of their magnitudes (each is within the parity bar of its own)."""
    c = case(sem, ndim, p)
    fs, t64, tld = c.fs, c.t64, c.tld
    assert np.array_equal(fs.node_ind.cpu().numpy(), t64.node_ind(c.e2n))
    for key in GEOM_KEYS:
        parity(getattr(fs, key), getattr(tld, key), getattr(t64, key), "p=%d %s" % (p, key))
    g64, dn64 = t64.gradient(c.u, c.e2n)
    gld, dnld = tld.gradient(c.u, c.e2n)
    u = torch.from_numpy(c.u).cuda()
    parity(fs.gradient(u), gld, g64, "p=%d gradient" % p)
    parity(fs.normal_derivative(u), dnld, dn64, "p=%d normal derivative" % p)
    per, tot = fs.flux(u, return_per_face=True)
    pld, totld = tld.integrate(dnld)
    parity(per, pld, t64.integrate(dn64)[0], "p=%d flux per face" % p)
    assert abs(float(tot) - float(totld)) <= 1e-12 * float(np.abs(pld).sum())
    per2, tot2 = fs.integrate(fs.normal_derivative(u), return_per_face=True)
    assert rel_l2(per2.cpu().numpy(), per.cpu().numpy()) <= 1e-14


# ---------------------------------------------------------------- orientation
def test_extruded_lateral_normals(sem, fmod, golden):
    """On an extruded 2-D mesh the lateral faces' n_dS is the reference's 2-D
    n_dS times half the layer height, with no z component."""
    from spectralelementmethod_amd import meshgen
    name, nez, h = "sq_p4", 2, 0.3
    p = int(golden[name + "_p"])
    n = p + 1
    nodes3, e2n3 = meshgen.extrude(golden[name + "_nodes"], golden[name + "_e2n"], nez, p,
                                   z0=0.0, z1=nez * h)
    op = sem.SEMOperator(p, e2n3, nodes3)
    E2 = golden[name + "_e2n"].shape[0]
    elem = np.repeat(np.arange(E2 * nez), 4)
    face = np.tile(np.arange(4), E2 * nez)
    nd3 = op.face_set(elem, face).n_dS.cpu().numpy().reshape(E2, nez, 4, 3, n * n)
    ref = golden[name + "_face_n_dS"].reshape(E2, 4, 2, n)
    t3, t2 = fmod.face_index_table(3, n), fmod.face_index_table(2, n)
    for f in range(4):
        # the 2-D face node under each 3-D face node: equal 2-D parent dof
        q2 = np.array([np.flatnonzero(t2[f] == l // n)[0] for l in t3[f]])
        want = ref[:, None, f][:, :, :, q2] * (0.5 * h)            # [E2, 1, 2, n * n]
        assert rel_l2(nd3[:, :, f, :2], np.broadcast_to(want, nd3[:, :, f, :2].shape)) <= 1e-12
        assert np.abs(nd3[:, :, f, 2]).max() <= 1e-13 * np.abs(nd3[:, :, f, :2]).max()


@pytest.mark.parametrize("p", [3, 8])
def test_warped_cube_orientation(sem, p):
    from spectralelementmethod_amd.discrete import Mesh
    c = case(sem, 3, p)
    n = p + 1
    W = torch.from_numpy(np.multiply.outer(c.w, c.w)).cuda()
    ndsw = (c.fs.n_dS * W).cpu().numpy()                  # [F, 3, n, n]
    area = float(c.fs.dSxW.sum())
    # a. the closed exterior: sum n dS = 0 (integrand of degree 2p - 1 per variable)
    ee, ef = Mesh.from_arrays(c.nodes, c.e2n).exterior_faces()
    rows = ee.astype(np.int64) * 6 + ef
    assert rows.size == 24
    closed = np.abs(ndsw[rows].sum(axis=(0, 2, 3))).max()
    ext_area = float(c.fs.dSxW.cpu().numpy()[rows].sum())
    print("p=%d closed surface: |sum n dS| %.2e of area %.3f" % (p, closed, ext_area))
    assert closed <= 1e-12 * ext_area
    # b. interior faces: n_dSxW = -neighbour's at the shared nodes
    node = c.fs.node_ind.cpu().numpy().reshape(-1, n * n)
    interior = np.setdiff1d(np.arange(node.shape[0]), rows)
    keys = {}
    for r in interior:
        keys.setdefault(tuple(np.sort(node[r])), []).append(r)
    assert len(keys) == 12 and all(len(v) == 2 for v in keys.values())
    worst = 0.0
    for a, b in keys.values():
        perm = np.argsort(node[b])[np.argsort(np.argsort(node[a]))]   # node[b][perm] == node[a]
        assert np.array_equal(node[b][perm], node[a])
        va, vb = ndsw[a].reshape(3, -1), ndsw[b].reshape(3, -1)[:, perm]
        worst = max(worst, np.abs(va + vb).max())
    print("p=%d neighbours: |n_dSxW + n_dSxW'| %.2e" % (p, worst))
    assert worst <= 1e-12 * area
    # c. outward: unit_normal . (face centroid - element centroid) > 0
    xf = c.fs.x_phys.cpu().numpy()                         # [F, 3, n, n]
    cen_e = c.xp.reshape(c.xp.shape[0], 3, -1).mean(axis=2)
    d = xf.reshape(xf.shape[0], 3, -1).mean(axis=2) - cen_e[c.elem]
    dots = np.einsum("fcq,fc->fq", c.fs.unit_normal.cpu().numpy().reshape(-1, 3, n * n), d)
    assert dots.min() > 0.0
    assert abs(np.linalg.norm(c.fs.unit_normal.cpu().numpy(), axis=1) - 1.0).max() <= 1e-14


# ---------------------------------------------------------------- polynomial exactness
@pytest.mark.parametrize("ndim,p", [(2, 5), (3, 3)])
def test_polynomial_exactness_on_affine_mesh(sem, ndim, p):
    """u of degree <= p on an affine mesh: the face gradient is exact and the
    flux through the closed exterior equals the integral of lap u (GLL
    quadrature of degree 2p - 1 integrates it exactly)."""
    from spectralelementmethod_amd.discrete import Mesh
    c = case(sem, ndim, p, warp=0.0)
    x = np.empty_like(c.nodes)
    x[:, c.e2n.astype(np.int64)] = np.moveaxis(c.xp, 1, 0)     # the GLL points of the nodes
    X = [x[k] for k in range(ndim)]
    if ndim == 2:
        u = X[0] ** p - 2.0 * X[0] ** 2 * X[1] ** (p - 2) + X[1] ** 3 + 0.5 * X[0] * X[1] \
            + 0.7 * X[0] ** 2
        grad = lambda a, b: [p * a ** (p - 1) - 4.0 * a * b ** (p - 2) + 0.5 * b + 1.4 * a,
                             -2.0 * a ** 2 * (p - 2) * b ** (p - 3) + 3.0 * b ** 2 + 0.5 * a]
        lap = p * (p - 1) * X[0] ** (p - 2) - 4.0 * X[1] ** (p - 2) \
            - 2.0 * X[0] ** 2 * (p - 2) * (p - 3) * X[1] ** (p - 4) + 6.0 * X[1] + 1.4
    else:
        u = X[0] ** 3 + X[0] * X[1] ** 2 - 2.0 * X[2] ** 3 + X[0] * X[1] * X[2] \
            + 0.7 * X[1] ** 2
        grad = lambda a, b, z: [3.0 * a ** 2 + b ** 2 + b * z, 2.0 * a * b + a * z + 1.4 * b,
                                -6.0 * z ** 2 + a * b]
        lap = 6.0 * X[0] + 2.0 * X[0] - 12.0 * X[2] + 1.4
    xf = c.tld.x_phys
    exact = np.stack(grad(*[xf[:, k] for k in range(ndim)]), axis=1)
    parity(c.fs.gradient(u), exact, c.t64.gradient(u, c.e2n)[0], "affine gradient")
    ee, ef = Mesh.from_arrays(c.nodes, c.e2n).exterior_faces()
    ext = c.op.face_set(ee, ef)
    t64 = faces_twin.Twin(c.xp, c.D, c.w, ee, ef)
    per, tot = ext.flux(torch.from_numpy(u).cuda(), return_per_face=True)
    detJxW = c.op.geometry_fields()["detJxW"].cpu().numpy()
    want = float((lap[c.e2n.astype(np.int64)] * detJxW).sum())
    scale = float(np.abs(per.cpu().numpy()).sum())
    print("affine flux %.15g, int lap u %.15g, scale %.3g" % (float(tot), want, scale))
    assert abs(float(tot) - want) <= 1e-12 * scale
    parity(per, faces_twin.Twin(c.xp, c.D, c.w, ee, ef, np.longdouble).flux(u, c.e2n)[0],
           t64.flux(u, c.e2n)[0], "affine flux per face")


# ---------------------------------------------------------------- assembly
@pytest.mark.parametrize("ndim,p", [(2, 4), (3, 3)])
def test_assemble(sem, ndim, p):
    c = case(sem, ndim, p)
    rng = np.random.default_rng(ndim)
    vals = rng.standard_normal(tuple(c.fs.dS.shape))
    nn = c.op.n_node
    want = c.t64.assemble(vals, c.e2n, nn)
    v = torch.from_numpy(vals).cuda()
    out = c.fs.assemble(v)
    e = rel_l2(out.cpu().numpy(), want)
    print("assemble: to np.add.at %.2e" % e)
    assert e <= 1e-13
    assert torch.equal(c.fs.assemble(v), out)                      # bitwise over two calls
    info = c.fs.info()
    # every face of every element: a corner of the mesh's centre gets all of
    # its 4 (2-D) or 8 (3-D) elements, each through ndim faces
    assert info["max_contributions"] == ndim * 2 ** ndim
    assert info["distinct_nodes"] == np.unique(c.t64.node_ind(c.e2n)).size
    # a corner element with its exterior faces: the corner node gets ndim contributions
    corner = c.op.face_set([0] * ndim, [2 * a for a in range(ndim)])
    assert corner.info()["max_contributions"] == ndim
    tw = faces_twin.Twin(c.xp, c.D, c.w, [0] * ndim, [2 * a for a in range(ndim)])
    cv = rng.standard_normal(tuple(corner.dS.shape))
    on = np.zeros(nn, dtype=bool)
    on[tw.node_ind(c.e2n).ravel()] = True
    assert on.sum() == corner.info()["distinct_nodes"] < nn
    base = rng.standard_normal(nn)
    for accumulate in (False, True):
        y = torch.from_numpy(base).cuda()
        corner.assemble(torch.from_numpy(cv).cuda(), out=y, accumulate=accumulate)
        y = y.cpu().numpy()
        assert np.array_equal(y[~on], base[~on])                   # off the faces: untouched
        ref = tw.assemble(cv, c.e2n, nn) + (base if accumulate else 0.0)
        assert np.abs(y[on] - ref[on]).max() <= 1e-13 * np.abs(ref[on]).max()
    # totals: bitwise repeatable
    u = torch.from_numpy(c.u).cuda()
    assert torch.equal(c.fs.flux(u), c.fs.flux(u))
    assert torch.equal(c.fs.integrate(v), c.fs.integrate(v))
    a, b = c.fs.flux(u, return_per_face=True), c.fs.flux(u, return_per_face=True)
    assert torch.equal(a[0], b[0])


# ---------------------------------------------------------------- launch tails
@pytest.mark.parametrize("ndim,p", [(2, 6), (3, 2)])
@pytest.mark.parametrize("count", [1, 5, 67, 0])
def test_face_counts_and_strides(sem, ndim, p, count):
    c = case(sem, ndim, p)
    rng = np.random.default_rng(count)
    E = c.e2n.shape[0]
    elem, face = rng.integers(0, E, count), rng.integers(0, 2 * ndim, count)
    fs = c.op.face_set(elem, face)
    tw = faces_twin.Twin(c.xp, c.D, c.w, elem, face)
    nn = c.op.n_node
    u2 = np.stack([c.u, np.cos(c.nodes[0] * c.nodes[1])])           # [2, n_node]
    inter = np.ascontiguousarray(u2.T).ravel()                      # DOF = 2 * node + comp
    g_cm = fs.gradient(torch.from_numpy(u2).cuda())
    g_il = fs.gradient(torch.from_numpy(inter).cuda(), dofs_per_node=2)
    assert tuple(g_cm.shape) == (2, count, ndim) + fs.fshape
    assert torch.equal(g_cm, g_il)
    per, tot = fs.flux(torch.from_numpy(inter).cuda(), return_per_face=True, dofs_per_node=2)
    assert tuple(per.shape) == (2, count) and tuple(tot.shape) == (2,)
    assert torch.equal(tot, fs.flux(torch.from_numpy(u2).cuda()))
    vals = torch.ones((2, count) + fs.fshape, dtype=torch.float64, device="cuda")
    ip, it = fs.integrate(vals, return_per_face=True)
    if count == 0:
        assert fs.info()["distinct_nodes"] == 0 and fs.info()["max_node"] == -1
        assert tot.tolist() == [0.0, 0.0] and it.tolist() == [0.0, 0.0]
        y = torch.full((nn,), 3.0, dtype=torch.float64, device="cuda")
        fs.assemble(torch.empty((0,) + fs.fshape, dtype=torch.float64), out=y)
        assert bool((y == 3.0).all())
        return
    for k in range(2):
        gk, dnk = tw.gradient(u2[k], c.e2n)
        assert rel_l2(g_cm[k].cpu().numpy(), gk) <= 1e-12
        want_pf, want_tot = tw.integrate(dnk)
        assert np.abs(per[k].cpu().numpy() - want_pf).max() <= 1e-12 * np.abs(want_pf).max()
        assert abs(float(tot[k]) - want_tot) <= 1e-12 * np.abs(want_pf).sum()
    assert rel_l2(ip[0].cpu().numpy(), tw.integrate(np.ones_like(tw.dS))[0]) <= 1e-13
    assert torch.equal(ip[0], ip[1]) and torch.equal(it[0], it[1])


# ---------------------------------------------------------------- refusals
def test_refusals(sem, fmod):
    c = case(sem, 2, 4)
    E = c.e2n.shape[0]
    live = c.fs  # a live handle throughout
    for elem, face in (([E], [0]), ([-1], [0]), ([0], [4]), ([0, 1], [0, 255]), ([0], [-1])):
        with pytest.raises(ValueError):
            c.op.face_set(elem, face)
    with pytest.raises(ValueError):
        c.op.face_set([0, 1], [0])
    # the C ABI itself refuses what the facade lets through
    import ctypes as C
    from spectralelementmethod_amd import _lib
    lib = _lib.load()
    xp = torch.from_numpy(c.xp).cuda()
    h = C.c_void_p()

    def create(p, elem, face, n_elem=E):
        e, f = np.asarray(elem, dtype=np.int32), np.asarray(face, dtype=np.uint8)
        return lib.sem_faces_create(C.byref(h), 2, p, n_elem, _lib.tptr(xp), _lib.tptr(c.op.e2n),
                                    e.size, e.ctypes.data_as(C.c_void_p),
                                    f.ctypes.data_as(C.c_void_p), _lib.dptr(c.D), _lib.dptr(c.w),
                                    0, None)
    assert create(4, [E], [0]) == _lib.SEM_E_INVALID and not h.value
    assert create(4, [0], [4]) == _lib.SEM_E_INVALID and not h.value
    assert create(17, [0], [0]) == _lib.SEM_E_NOTIMPL and not h.value
    with pytest.raises(NotImplementedError):
        _lib.check(create(17, [0], [0]))
    with pytest.raises(NotImplementedError):
        fmod.FaceSet(x_phys=np.zeros((1, 2, 18, 18)), e2n=np.zeros((1, 18, 18), np.uint32),
                     elem=[0], face=[0])
    # a field of another size never reaches a kernel
    nn = c.op.n_node
    for bad in (np.zeros(nn - 1), np.zeros(nn + 1), np.zeros((2, nn - 1)), np.zeros(2 * nn)):
        for call in (live.gradient, live.normal_derivative, live.flux):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        live.gradient(np.zeros(2 * nn + 1), dofs_per_node=2)
    with pytest.raises(ValueError):
        live.integrate(np.zeros((len(live) - 1, 5)))
    with pytest.raises(ValueError):
        live.assemble(np.zeros((len(live), 4)))
    with pytest.raises(TypeError):
        live.assemble(np.zeros((len(live), 5)), out=torch.zeros(nn - 1, dtype=torch.float64,
                                                                device="cuda"))
    # an output vector shorter than the faces' nodes is refused by the library
    v = torch.zeros(len(live), 5, dtype=torch.float64, device="cuda")
    small = torch.zeros(4, dtype=torch.float64, device="cuda")
    assert lib.sem_faces_assemble(live._h, _lib.tptr(v), _lib.tptr(small), 4, 0, None) == \
        _lib.SEM_E_INVALID
    assert rel_l2(live.dS.cpu().numpy(), c.t64.dS) <= 1e-12      # and the handle still works
    closed = c.op.face_set([0], [1])
    closed.close()
    with pytest.raises(RuntimeError):
        closed.flux(c.u)


# ---------------------------------------------------------------- graph capture
def test_flux_and_gradient_graph_capture(sem):
    c = case(sem, 3, 3)
    fs = c.fs
    rng = np.random.default_rng(5)
    u = torch.from_numpy(rng.standard_normal((2, c.op.n_node))).cuda()
    F = len(fs)
    grad = torch.empty((2, F, 3) + fs.fshape, dtype=torch.float64, device="cuda")
    per = torch.empty(2, F, dtype=torch.float64, device="cuda")
    tot = torch.empty(2, dtype=torch.float64, device="cuda")
    eager_g = fs.gradient(u).clone()
    eager_t = fs.flux(u).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fs.gradient(u, out=grad, stream=s)
        fs.flux(u, out=tot, per_face=per, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fs.gradient(u, out=grad)
        fs.flux(u, out=tot, per_face=per)
    grad.zero_()
    tot.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad, eager_g) and torch.equal(tot, eager_t)
    u2 = torch.from_numpy(rng.standard_normal((2, c.op.n_node))).cuda()
    want_g, want_t = fs.gradient(u2).clone(), fs.flux(u2).clone()
    u.copy_(u2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad, want_g) and torch.equal(tot, want_t)


# ---------------------------------------------------------------- the example
def test_neumann_example(sem):
    """examples/neumann.py at p = 8 on 4 x 4 elements.  The CPU oracle's
    direct solve (oracle/sem_oracle.py assemble_poisson_matrix /
    poisson_solve_direct) of the same system with the twin's float64 Neumann
    load is 8.28e-10 from the exact solution (max error over max |u*|,
    measured on the host); ten times that allows for the PCG's tolerance."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import neumann
    plate = neumann.NeumannPlate(8, 4, 4, 0.05)
    assert len(plate.nbc) == 8 and len(plate.ebc) == 8
    u_dev = plate.solve()
    elem, face = plate.mesh.boundary_faces("nbc")
    xp = plate.op.geometry_fields()["x_phys"].cpu().numpy()
    tw = faces_twin.Twin(xp, plate.op.D, plate.op.w, elem, face)
    _, (gx, gy), _ = neumann.exact(tw.x_phys[:, 0], tw.x_phys[:, 1])
    g = gx * tw.unit_normal[:, 0] + gy * tw.unit_normal[:, 1]
    load = tw.assemble(g, plate.mesh.element_map(), plate.dm.ndof)
    e_load = rel_l2(plate.neumann_load().cpu().numpy(), load)
    u_twin = plate.solve(neumann_load=load)
    e_solve = rel_l2(u_dev, u_twin)
    err = plate.error(u_dev)
    a, b, c, bal = plate.flux_balance(u_dev)
    print("neumann: load %.2e, solve %.2e, error %.3e, balance %.3e (%.6f %.6f %.6f)"
          % (e_load, e_solve, err, bal, a, b, c))
    assert e_load <= 1e-13
    assert e_solve <= 1e-10
    assert err <= 8.3e-9
    # int_nbc g + int_ebc du_h/dn + int f: 4.5e-7 for the oracle's solution
    # (the boundary flux of u_h converges slower than u_h)
    assert abs(bal) <= 4.5e-6
