"""GPU tests of point location and field evaluation (points.PointLocator,
sem_points_* in include/sem_hip.h) against

* the reference's own find_elem_containing_point / interpolate results
  (tests/golden/points.npz, p <= 10: above it the reference's x_phys is the
  inaccurate side) at the project's parity bar 1e-10;
* the package's host basis (sem_lagrange_eval through
  LagrangeGaussLobatto.__call__ / TensorProductQS.interpolate) fed the device
  x_phys and the located xi, on hexahedra and above p = 10;
* exact polynomial reproduction on affine meshes.
Tolerances on values are relative to the largest reference value of the
case (the fields are O(1))."""
import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = ("sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm")


@pytest.fixture(scope="module")
def sem():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import operators
    return operators


@pytest.fixture(scope="module")
def pts():
    return load_golden("points.npz")


def _basis1(p):
    from spectralelementmethod_amd.basis_functions import LagrangeGaussLobatto
    return LagrangeGaussLobatto(p)


def host_eval(p, e2n, u, elem, xi):
    """sum_jk.. u[e2n[elem]] l_j(xi0) l_k(xi1) .. with the host basis."""
    b = _basis1(p)
    nd = xi.shape[0]
    B = [b(np.ascontiguousarray(xi[d])) for d in range(nd)]
    loc = np.asarray(u)[np.asarray(e2n).astype(np.int64)[elem]]
    if nd == 2:
        return np.einsum("mi,mj,mij->m", B[0], B[1], loc)
    return np.einsum("mi,mj,mk,mijk->m", B[0], B[1], B[2], loc)


def _dofmanager(pts, case):
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManager, Mesh
    p = int(pts[case + "_p"])
    if case.endswith("_rcm"):
        # the default RCM numbering, rebuilt here from the unpermuted mesh
        base = case[:-4]
        dm = DOFManager(Mesh.from_arrays(pts[base + "_nodes"], pts[base + "_e2n"]), 1,
                        gll_basis_2d(p), rcm_order=True)
        assert np.array_equal(dm.mesh.nodes, pts[case + "_nodes"])
        assert np.array_equal(dm.mesh.element_map(), pts[case + "_e2n"])
        return dm
    return DOFManager(Mesh.from_arrays(pts[case + "_nodes"], pts[case + "_e2n"]), 1,
                      gll_basis_2d(p), rcm_order=False)


# ---------------------------------------------------------------- reference parity
@pytest.mark.parametrize("case", CASES)
def test_reference_parity(sem, pts, case):
    p = int(pts[case + "_p"])
    op = sem.SEMOperator(p, pts[case + "_e2n"], pts[case + "_nodes"])
    loc = op.point_locator()
    assert op.point_locator() is loc
    xq = pts[case + "_xq"]
    ps = loc.locate(xq)
    assert ps.n_outside == 0 and bool(ps.found.all())
    elem = ps.elem.cpu().numpy()
    inter = pts[case + "_interior"]
    assert np.array_equal(elem[inter], pts[case + "_elem"][inter])
    same = elem == pts[case + "_elem"]
    dxi = np.abs(ps.xi.cpu().numpy() - pts[case + "_xi"])[:, same].max()
    vref = pts[case + "_vals"]
    vals = ps.evaluate(pts[case + "_u"])
    assert isinstance(vals, np.ndarray) and vals.shape == (xq.shape[1],)
    dv = np.abs(vals - vref).max() / np.abs(vref).max()
    drt = np.abs(ps.physical().cpu().numpy() - xq).max()
    print("%s: |dxi| %.2e, values rel %.2e, round trip %.2e" % (case, dxi, dv, drt))
    assert dxi <= 1e-10
    assert dv <= 1e-10
    assert drt <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_reference_parity_dofmanager(sem, pts, case):
    dm = _dofmanager(pts, case)
    xq, u, vref = pts[case + "_xq"], pts[case + "_u"], pts[case + "_vals"]
    assert dm.point_locator() is dm.point_locator()
    vals = dm.interpolate(u, xq)
    assert vals.shape == (xq.shape[1],)
    assert np.abs(vals - vref).max() <= 1e-10 * np.abs(vref).max()
    both = dm.interpolate(np.stack([u, 2.0 * u]), xq)
    assert both.shape == (2, xq.shape[1])
    assert np.abs(both[1] - 2.0 * vref).max() <= 2e-10 * np.abs(vref).max()
    inter = pts[case + "_interior"]
    e2n = pts[case + "_e2n"]
    for k in range(8):
        v = dm.interpolate(u, xq[:, k])
        assert np.ndim(v) == 0 and abs(v - vref[k]) <= 1e-10 * np.abs(vref).max()
        fe, x_param = dm.find_elem_containing_point(xq[:, k])
        if inter[k]:
            assert np.array_equal(fe.node_ind, e2n[pts[case + "_elem"][k]])
            assert np.abs(x_param - pts[case + "_xi"][:, k]).max() <= 1e-10
            assert abs(fe.interpolate(u[fe.node_ind], x_param).reshape(()) - vref[k]) \
                <= 1e-10 * np.abs(vref).max()


# ---------------------------------------------------------------- every node is found
@pytest.mark.parametrize("ndim,p", [(2, 2), (2, 4), (2, 8), (3, 2), (3, 4)])
def test_every_node_is_found(sem, ndim, p):
    from spectralelementmethod_amd import meshgen
    if ndim == 2:
        nodes, e2n = meshgen.structured_square(3, 2, p, warp=0.06)
    else:
        nodes, e2n = meshgen.structured_cube(2, 2, 2, p, warp=0.05)
    op = sem.SEMOperator(p, e2n, nodes)
    xp = op.geometry_fields()["x_phys"]
    E = xp.shape[0]
    xq = xp.reshape(E, ndim, -1).permute(1, 0, 2).reshape(ndim, -1).contiguous()
    ps = op.point_locator().locate(xq)
    assert ps.n_outside == 0 and bool(ps.found.all())
    xi = ps.xi.cpu().numpy()
    assert np.abs(xi).max() <= 1.0
    u = np.random.default_rng(p).standard_normal(op.n_node)
    vals = ps.evaluate(torch.from_numpy(u).to(op.device)).cpu().numpy()
    assert np.isfinite(vals).all()
    want = u[e2n.astype(np.int64)].reshape(-1)
    assert np.abs(vals - want).max() <= 1e-12
    # exactly at the GLL nodes of a hand-made set the basis is the delta
    b = _basis1(p)
    g = np.stack(np.meshgrid(*([b.nodes] * ndim), indexing="ij")).reshape(ndim, -1)
    hand = op.point_locator().point_set(np.zeros(g.shape[1], dtype=np.int32), g)
    v0 = hand.evaluate(u)
    assert np.array_equal(v0, u[e2n[0].astype(np.int64)].reshape(-1))


# ---------------------------------------------------------------- exactness
def _poly(ndim, p, seed):
    """Random polynomial of degree <= p per direction: standard normal
    coefficients of the monomials x^i y^j (z^k)."""
    from numpy.polynomial import polynomial as P
    c = np.random.default_rng(seed).standard_normal((p + 1,) * ndim)
    return (lambda x, y: P.polyval2d(x, y, c)) if ndim == 2 else \
        (lambda x, y, z: P.polyval3d(x, y, z, c))


def _affine_x_phys(nodes, e2n, p):
    """x_phys of an axis-aligned affine mesh, exactly: every element's box
    scaled onto the GLL nodes [E, ndim] + [n] * ndim."""
    ndim = nodes.shape[0]
    g = _basis1(p).nodes
    m = e2n.reshape(e2n.shape[0], -1).astype(np.int64)
    xp = np.empty((e2n.shape[0], ndim) + (p + 1,) * ndim)
    for d in range(ndim):
        c = nodes[d][m]
        lo, hi = c.min(axis=1), c.max(axis=1)
        shp = [1] * ndim
        shp[d] = p + 1
        line = lo[:, None] + (g[None, :] + 1.0) * 0.5 * (hi - lo)[:, None]
        xp[:, d] = line.reshape([-1] + shp)
    return xp


@pytest.mark.parametrize("ndim,p,shape", [(2, 1, (3, 2)), (2, 3, (3, 2)), (2, 8, (3, 2)),
                                          (2, 12, (3, 2)), (2, 16, (3, 2)),
                                          (3, 1, (2, 2, 2)), (3, 4, (2, 2, 2)),
                                          (3, 8, (2, 2, 2)), (3, 12, (2, 1, 1)),
                                          (3, 16, (2, 1, 1))])
def test_polynomial_exactness_affine(sem, ndim, p, shape):
    """The affine geometry is handed to the locator exactly (raw x_phys
    arrays): the x_phys the operator derives from the mesh nodes carries the
    rounding of the equispaced -> GLL transform (measured 2.6e-12 / 5.0e-12 at
    p = 16 in 2-D / 3-D), so the located xi would be off
    by as much and f(x(xi)) would no longer be a polynomial of degree p in xi:
    the premise of exactness.  The operator's own locator (geometry_fields ->
    PointLocator) is held to the same bound where that rounding times the
    field's relative gradient (about p for these polynomials, p^2 at most)
    stays below it: up to p = 8 (x_phys to 1e-14) and in 2-D at p = 12
    (4.9e-14 * 12 = 5.9e-13; measured 2.1e-13).  On hexahedra at p = 12 it
    does not (9.8e-14 * 12 = 1.2e-12; measured 1.22e-12), nor at p = 16.  What is
    left is the float64 rounding of the GLL table itself: 3.5e-13 for these
    polynomials at p = 16 in 3-D with the host basis."""
    from spectralelementmethod_amd import meshgen
    from spectralelementmethod_amd.points import PointLocator
    nodes, e2n = (meshgen.structured_square if ndim == 2 else meshgen.structured_cube)(*shape, p)
    xp = _affine_x_phys(nodes, e2n, p)
    f = _poly(ndim, p, 100 * ndim + p)
    u = np.zeros(nodes.shape[1])
    u[e2n.astype(np.int64)] = f(*[xp[:, d] for d in range(ndim)])
    xq = np.random.default_rng(p).uniform(-1.0, 1.0, size=(ndim, 200))
    want = f(*xq)
    locators = [PointLocator(x_phys=xp, e2n=e2n)]
    if p <= 8 or (ndim == 2 and p <= 12):
        locators.append(sem.SEMOperator(p, e2n, nodes).point_locator())
    for loc in locators:
        ps = loc.locate(xq)
        assert ps.n_outside == 0
        vals = ps.evaluate(u)
        err = np.abs(vals - want).max() / np.abs(want).max()
        print("ndim %d p %d %s: rel err %.2e" % (ndim, p, "exact x_phys" if loc is locators[0]
                                                 else "operator x_phys", err))
        assert err <= 1e-12


# ---------------------------------------------------------------- hexahedra, p > 10, warped
@pytest.mark.parametrize("ndim,p,shape", [(3, 3, (2, 2, 2)), (3, 8, (2, 2, 2)),
                                          (3, 12, (2, 1, 1)), (2, 12, (3, 2)), (2, 16, (3, 2))])
def test_warped_against_host_basis(sem, ndim, p, shape):
    from spectralelementmethod_amd import meshgen
    from spectralelementmethod_amd.basis_functions import TensorProductQS
    gen = meshgen.structured_square if ndim == 2 else meshgen.structured_cube
    nodes, e2n = gen(*shape, p, warp=0.05)
    op = sem.SEMOperator(p, e2n, nodes)
    rng = np.random.default_rng(7 * p + ndim)
    xq = rng.uniform(-0.95, 0.95, size=(ndim, 48))
    ps = op.point_locator().locate(xq)
    assert ps.n_outside == 0
    elem, xi = ps.elem.cpu().numpy(), ps.xi.cpu().numpy()
    u = rng.standard_normal(op.n_node)
    vals = ps.evaluate(u)
    tb = TensorProductQS(*([_basis1(p)] * ndim))
    xp = op.geometry_fields()["x_phys"].cpu().numpy()
    want = np.empty(xq.shape[1])
    back = np.empty_like(xq)
    for k in range(xq.shape[1]):
        want[k] = np.asarray(tb.interpolate(u[e2n[elem[k]].astype(np.int64)], xi[:, k])).reshape(())
        back[:, k] = np.asarray(tb.interpolate(xp[elem[k]], xi[:, k])).reshape(ndim)
    assert np.abs(vals - host_eval(p, e2n, u, elem, xi)).max() <= 1e-12 * np.abs(want).max()
    ev = np.abs(vals - want).max() / np.abs(want).max()
    rt = np.abs(ps.physical().cpu().numpy() - xq).max()
    print("ndim %d p %d: values rel %.2e, round trip %.2e, host map %.2e"
          % (ndim, p, ev, rt, np.abs(back - xq).max()))
    assert ev <= 1e-12
    assert rt <= 1e-11
    assert np.abs(back - xq).max() <= 1e-11


# ---------------------------------------------------------------- outside and bad input
def test_outside_points(sem, pts):
    from spectralelementmethod_amd import discrete
    case = "sq_p4"
    dm = _dofmanager(pts, case)
    loc = dm.point_locator()
    u = pts[case + "_u"]
    xq = np.concatenate([pts[case + "_xq"][:, :5],
                         np.array([[1.5, -3.0, 0.2, np.nan], [0.0, 2.0, -1.0001, 0.3]])], axis=1)
    ps = loc.locate(xq)
    elem = ps.elem.cpu().numpy()
    assert ps.n_outside == 4 and np.array_equal(elem[5:], [-1] * 4) and (elem[:5] >= 0).all()
    assert np.array_equal(ps.found.cpu().numpy(), [True] * 5 + [False] * 4)
    assert np.isnan(ps.xi.cpu().numpy()[:, 5:]).all()
    vals = ps.evaluate(u)
    assert np.isnan(vals[5:]).all()
    assert np.abs(vals[:5] - pts[case + "_vals"][:5]).max() <= 1e-10
    assert np.isnan(ps.physical().cpu().numpy()[:, 5:]).all()
    batch = dm.interpolate(u, xq)
    assert np.isnan(batch[5:]).all() and np.array_equal(batch[:5], vals[:5])
    with pytest.raises(discrete.OutsideDomain):
        dm.interpolate(u, [1.5, 0.0])
    with pytest.raises(discrete.OutsideDomain):
        dm.find_elem_containing_point([-3.0, 2.0])


def test_bad_element_ids_evaluate_to_nan(sem, pts):
    """Ids -1, E and 2^31 - 1 belong to no run: NaN, and no memory indexed."""
    case = "sq_p8"
    p = int(pts[case + "_p"])
    e2n = pts[case + "_e2n"]
    op = sem.SEMOperator(p, e2n, pts[case + "_nodes"])
    loc = op.point_locator()
    E = e2n.shape[0]
    rng = np.random.default_rng(3)
    m = 40
    elem = rng.integers(0, E, size=m).astype(np.int32)
    bad = {3: -1, 17: E, 29: 2 ** 31 - 1, 30: -(2 ** 31)}
    for k, v in bad.items():
        elem[k] = v
    xi = rng.uniform(-1, 1, size=(2, m))
    ps = loc.point_set(elem, xi)
    assert ps.n_outside == len(bad)
    u = pts[case + "_u"]
    vals = ps.evaluate(np.stack([u, -u]))
    good = np.array([k not in bad for k in range(m)])
    assert np.isnan(vals[:, ~good]).all()
    want = host_eval(p, e2n, u, elem[good], xi[:, good])
    assert np.abs(vals[0, good] - want).max() <= 1e-12
    assert np.array_equal(vals[1, good], -vals[0, good])
    x = ps.physical().cpu().numpy()
    assert np.isnan(x[:, ~good]).all() and np.isfinite(x[:, good]).all()
    info = ps.plan_info()
    assert info["points"] == m and info["in_runs"] == m - len(bad)
    xi2, status = loc.invert(x, elem)
    status = status.cpu().numpy()
    assert (status[~good] == 2).all() and (status[good] == 0).all()
    assert np.abs(xi2.cpu().numpy()[:, good] - xi[:, good]).max() <= 1e-10


# ---------------------------------------------------------------- layouts and order
def test_layouts_order_and_determinism(sem, pts):
    case = "ann_p6"
    p = int(pts[case + "_p"])
    op = sem.SEMOperator(p, pts[case + "_e2n"], pts[case + "_nodes"])
    loc = op.point_locator()
    xq = pts[case + "_xq"]
    ps = loc.locate(xq)
    rng = np.random.default_rng(11)
    U = torch.from_numpy(rng.standard_normal((3, op.n_node))).to(op.device)
    one = [ps.evaluate(U[c].contiguous()) for c in range(3)]
    allc = ps.evaluate(U)
    assert allc.shape == (3, xq.shape[1])
    for c in range(3):
        assert torch.equal(allc[c], one[c])
    inter = U[:2].t().contiguous().reshape(-1)  # DOF = 2 * node + comp
    il = ps.evaluate(inter, dofs_per_node=2)
    assert il.shape == (2, xq.shape[1]) and torch.equal(il, allc[:2])
    nested = ps.evaluate(U.reshape(3, 1, op.n_node))
    assert nested.shape == (3, 1, xq.shape[1]) and torch.equal(nested[:, 0], allc)
    assert torch.equal(ps.evaluate(U), allc)  # bitwise repeatable
    perm = rng.permutation(xq.shape[1])
    ps2 = loc.locate(xq[:, perm])
    assert torch.equal(ps2.evaluate(U), allc[:, torch.from_numpy(perm).to(op.device)])
    out = torch.full_like(allc, -1.0)
    assert ps.evaluate(U, out=out) is out and torch.equal(out, allc)
    with pytest.raises(TypeError):
        ps.evaluate(U, out=out[:2])


# ---------------------------------------------------------------- run lengths
@pytest.mark.parametrize("n_long,width", [(300, 64), (40, 16)])
def test_long_and_short_runs(sem, pts, n_long, width):
    """One element with a run longer than an item (cut into several) and one
    point in each other element (idle lanes)."""
    case = "sq_p8"
    p = int(pts[case + "_p"])
    e2n = pts[case + "_e2n"]
    op = sem.SEMOperator(p, e2n, pts[case + "_nodes"])
    E = e2n.shape[0]
    rng = np.random.default_rng(n_long)
    elem = np.concatenate([np.full(n_long, 2), np.delete(np.arange(E), 2)]).astype(np.int32)
    order = rng.permutation(elem.size)
    elem = elem[order]
    xi = rng.uniform(-1, 1, size=(2, elem.size))
    ps = op.point_locator().point_set(elem, xi)
    info = ps.plan_info()
    assert info["width"] == width and info["touched_elements"] == E
    assert info["items"] == -(-n_long // width) + E - 1
    u = pts[case + "_u"]
    vals = ps.evaluate(u)
    assert np.abs(vals - host_eval(p, e2n, u, elem, xi)).max() <= 1e-12


# ---------------------------------------------------------------- graph capture
def test_evaluate_graph_capture(sem, pts):
    case = "sq_p4"
    p = int(pts[case + "_p"])
    op = sem.SEMOperator(p, pts[case + "_e2n"], pts[case + "_nodes"])
    ps = op.point_locator().locate(np.concatenate([pts[case + "_xq"], [[2.0], [2.0]]], axis=1))
    assert ps.n_outside == 1
    rng = np.random.default_rng(5)
    u = torch.from_numpy(rng.standard_normal((2, op.n_node))).to(op.device)
    out = torch.empty(2, len(ps), dtype=torch.float64, device=op.device)
    eager = ps.evaluate(u).clone()  # also builds the plan
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ps.evaluate(u, out=out, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ps.evaluate(u, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:, :-1], eager[:, :-1]) and bool(torch.isnan(out[:, -1]).all())
    u2 = torch.from_numpy(rng.standard_normal((2, op.n_node))).to(op.device)
    want = ps.evaluate(u2).clone()
    u.copy_(u2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:, :-1], want[:, :-1]) and bool(torch.isnan(out[:, -1]).all())


# ---------------------------------------------------------------- sizes of u, counts
def test_mis_sized_u_is_refused(sem, pts):
    """The kernel indexes u with the mesh's map, so a field of another mesh,
    order or layout must be refused before the launch."""
    from spectralelementmethod_amd.points import PointLocator
    case = "sq_p4"
    p = int(pts[case + "_p"])
    e2n = pts[case + "_e2n"]
    op = sem.SEMOperator(p, e2n, pts[case + "_nodes"])
    loc = op.point_locator()
    nn = op.n_node
    assert loc.n_node == nn
    ps = loc.locate(pts[case + "_xq"][:, :8])
    u = pts[case + "_u"]
    good = ps.evaluate(u)
    dev = torch.from_numpy(u).to(op.device)
    for bad in (u[:-1], u[:1], np.zeros(0), np.zeros(nn + 1), np.zeros((2, nn - 1)),
                np.zeros((nn, 2)), np.zeros(2 * nn), np.float64(1.0), dev[:-1],
                torch.zeros(2 * nn, dtype=torch.float64, device=op.device)):
        with pytest.raises(ValueError):
            ps.evaluate(bad)
    for bad, dpn in ((np.zeros(2 * nn - 2), 2), (np.zeros(2 * nn), 1), (np.zeros(nn), 2),
                     (np.zeros(2 * nn), 4), (np.zeros((2, nn)), 2), (np.zeros(2 * nn), 0)):
        with pytest.raises(ValueError):
            ps.evaluate(bad, dofs_per_node=dpn)
    assert np.array_equal(ps.evaluate(u), good)
    assert np.array_equal(ps.evaluate(np.repeat(u, 2), dofs_per_node=2)[1], good)
    # raw arrays: n_node is the map's largest entry + 1
    raw = PointLocator(x_phys=op.geometry_fields()["x_phys"], e2n=e2n)
    assert raw.n_node == int(e2n.max()) + 1 == nn
    ps2 = raw.locate(pts[case + "_xq"][:, :8])
    with pytest.raises(ValueError):
        ps2.evaluate(u[:-1])
    assert np.array_equal(ps2.evaluate(u), good)
    # through the reference API
    dm = _dofmanager(pts, case)
    with pytest.raises(ValueError):
        dm.interpolate(u[:-1], pts[case + "_xq"][:, 0])
    with pytest.raises(ValueError):
        dm.interpolate(np.zeros((nn, 2)), pts[case + "_xq"])


def test_bad_counts_with_a_live_handle(sem, pts):
    """n_pts outside [0, 2^31) is SEM_E_INVALID with a valid sem_points too;
    nothing is launched and the arrays are not touched."""
    import ctypes as C
    from spectralelementmethod_amd import _lib
    case = "sq_p2"
    op = sem.SEMOperator(int(pts[case + "_p"]), pts[case + "_e2n"], pts[case + "_nodes"])
    loc = op.point_locator()
    lib = _lib.load()
    xq = torch.zeros(2, 4, dtype=torch.float64, device=op.device)
    xi = torch.full((2, 4), 7.0, dtype=torch.float64, device=op.device)
    elem = torch.full((4,), 7, dtype=torch.int32, device=op.device)
    n_out = C.c_int64(0)
    plan = C.c_void_p()
    for n_bad in (-1, -4, 2 ** 31):
        assert lib.sem_points_locate(loc._pts, n_bad, _lib.tptr(xq), _lib.tptr(elem),
                                     _lib.tptr(xi), C.byref(n_out), None) == _lib.SEM_E_INVALID
        assert "n_pts" in _lib.last_error()
        assert lib.sem_points_invert(loc._pts, n_bad, _lib.tptr(xq), _lib.tptr(elem), None,
                                     _lib.tptr(xi), None, None) == _lib.SEM_E_INVALID
        assert lib.sem_points_map(loc._pts, n_bad, _lib.tptr(elem), _lib.tptr(xi),
                                  _lib.tptr(xq), None) == _lib.SEM_E_INVALID
        assert lib.sem_points_plan(loc._pts, n_bad, _lib.tptr(elem), C.byref(plan),
                                   None) == _lib.SEM_E_INVALID
        assert not plan.value
    torch.cuda.synchronize()
    assert bool((xi == 7.0).all()) and bool((elem == 7).all()) and bool((xq == 0.0).all())
    # an empty point set is fine
    ps = loc.locate(np.zeros((2, 0)))
    assert len(ps) == 0 and ps.n_outside == 0
    assert ps.evaluate(pts[case + "_u"]).shape == (0,)


# ---------------------------------------------------------------- the example
def test_resample_example(sem, tmp_path, capsys):
    """examples/resample.py end to end on a tiny mesh: every pixel is inside,
    the image holds the solved field (its boundary values bound it below)."""
    import os
    import runpy
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = runpy.run_path(os.path.join(here, "examples", "resample.py"))["main"]
    out = tmp_path / "u.npy"
    image = main(["--p", "4", "--nex", "4", "--ney", "4", "--pixels", "16", "--out", str(out)])
    assert tuple(image.shape) == (16, 16)
    img = np.load(str(out))
    assert np.array_equal(img, image.cpu().numpy()) and np.isfinite(img).all()
    assert "0 outside the mesh" in capsys.readouterr().out
    # -lap u = 1 with u >= 0 on the essential boundary: u > 0 inside
    assert img.min() > 0.0
