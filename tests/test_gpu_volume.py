"""GPU tests of the volume fields (volume.VolumeSet, sem_volume_* in
include/sem_hip.h): the reference golden
(tests/golden/volume.npz), the float64 and np.longdouble twins of the stated
formulas on the device's own x_phys (tests/volume_twin.py, itself checked on
the CPU in tests/test_volume_host.py), the existing Poisson action, analytic
gradients, repeatability and the DOFManager facade.

Bars: the project's parity rule (``parity`` of tests/test_gpu_faces.py:
<= 1e-12 relative L2 to the golden or the extended twin, else as accurate as
the float64 twin, <= 1e-10 in any case); H1^2 against u . K u to 1e-10, the
project's bar for the action; L2^2 against sum(mass u^2) to 1e-13 (the same
non-negative terms summed in another order)."""
import functools

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import volume_twin as vt
from test_gpu_faces import parity

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN_CASES = ("sq_p2", "sq_p4", "sq_p8", "ann_p6", "sq_p4_rcm")


@pytest.fixture(scope="module")
def vmod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import volume
    return volume


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def mesh_of(kind, *args, **kw):
    from spectralelementmethod_amd import meshgen
    if kind == "shuffled":
        return meshgen.shuffle_nodes(*meshgen.structured_square(*args, **kw))
    if kind == "rcm":
        return meshgen.rcm_renumber(*meshgen.shuffle_nodes(*meshgen.structured_square(*args, **kw)))
    return getattr(meshgen, kind)(*args, **kw)


class Case(object):
    """A mesh on the device with its VolumeSet, both twins on the device's own
    x_phys, a smooth field u and v = u (1 + 1e-9 sin)."""

    def __init__(self, kind, args, p, warp=None, pad=0):
        from spectralelementmethod_amd.operators import SEMOperator
        from spectralelementmethod_amd.volume import VolumeSet
        kw = {} if warp is None else dict(warp=warp)
        nodes, e2n = mesh_of(kind, *args, **kw)
        self.p, self.e2n = p, np.asarray(e2n)
        self.op = SEMOperator(p, e2n, nodes, device="cuda:0")
        self.ndim = self.op.ndim
        x_phys = self.op.geometry_fields()["x_phys"]
        self.nn = nodes.shape[1] + pad
        self.vol = VolumeSet(x_phys=x_phys, e2n=e2n, n_node=self.nn, device="cuda:0") if pad \
            else self.op.volume_set()
        xh = x_phys.cpu().numpy()
        self.f64 = vt.Twin(xh, e2n, self.nn, self.op.D, self.op.w)
        self.ext = vt.Twin(xh, e2n, self.nn, self.op.D, self.op.w, np.longdouble)
        self.xn = np.nan_to_num(vt.node_coordinates(xh, e2n, self.nn))
        self.u = vt.smooth(self.xn)
        self.v = self.u * (1.0 + 1e-9 * np.sin(3.0 * self.xn[0] + self.xn[1]))

    def check(self, what="", fields=True, norms=True):
        """gradient, recover and the norms of u and of u - v against both
        twins by the parity rule."""
        vol, u, v = self.vol, self.u, self.v
        tag = "%s p %d %s" % (what, self.p, "hex" if self.ndim == 3 else "quad")
        if fields:
            parity(vol.gradient(u), self.ext.gradient(u), self.f64.gradient(u), tag + " gradient")
            parity(vol.recover(u), self.ext.recover(u), self.f64.recover(u), tag + " recover")
        if norms:
            for name, args in (("norms(u)", (u,)), ("norms(u - v)", (u, v))):
                per, res = vol.norms(*args, return_per_element=True)
                pe, te = self.ext.norms(*args)
                p6, t6 = self.f64.norms(*args)
                parity(per, pe, p6, "%s %s per element" % (tag, name))
                parity(np.stack([res.l2_sq, res.h1_sq]), te, t6, "%s %s totals" % (tag, name))
                assert np.allclose(res.l2 ** 2, res.l2_sq, rtol=1e-14, atol=0)


@functools.lru_cache(maxsize=None)
def case(kind, args, p, warp=None, pad=0):
    return Case(kind, args, p, warp, pad)


# --------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reference_parity(vmod, name):
    g = load_golden("volume.npz")
    from spectralelementmethod_amd.operators import _basis_arrays
    p = int(g[name + "_p"])
    _, D, w, _ = _basis_arrays(p, None, 2)
    x_phys, e2n, u = g[name + "_x_phys"], g[name + "_e2n"], g[name + "_u"]
    vol = vmod.VolumeSet(x_phys=x_phys, e2n=e2n, n_node=u.size, device="cuda:0")
    ext, f64 = (vt.Twin(x_phys, e2n, u.size, D, w, dt) for dt in (np.longdouble, np.float64))
    parity(vol.gradient(u), ext.gradient(u), f64.gradient(u), name + " gradient",
           golden=g[name + "_gradient"])
    per, tot = vol.integrate(u, return_per_element=True)
    parity(per, ext.integrate(u)[0], f64.integrate(u)[0], name + " integrate",
           golden=g[name + "_integrate"])
    assert abs(tot - g[name + "_integrate"].sum()) <= 1e-12 * np.abs(g[name + "_integrate"]).sum()
    ones = np.ones((len(vol),) + vol.eshape)
    per1, _ = vol.integrate_local(ones, return_per_element=True)
    parity(per1, ext.integrate_local(ones)[0], f64.integrate_local(ones)[0],
           name + " integrate(1)", golden=g[name + "_integrate_one"])
    parity(vol.mass, ext.mass, f64.mass, name + " mass",
           golden=f64.assemble(g[name + "_detJxW"]))
    assert vol.info() == dict(ndim=2, p=p, elements=len(e2n), nodes=u.size,
                              referenced_nodes=u.size, max_contributions=4,
                              scratch_bytes=8 * 2 * e2n.size)


# --------------------------------------------------------------------------- every order
@pytest.mark.parametrize("p", range(1, 17))
def test_every_order_2d(vmod, p):
    case("structured_square", (2, 2, p), p, 0.05).check()


@pytest.mark.parametrize("p,args", [(1, (2, 2, 2)), (2, (2, 2, 2)), (4, (2, 2, 2)),
                                    (8, (2, 2, 2)), (12, (2, 1, 1)), (16, (2, 1, 1))])
def test_hexahedra(vmod, p, args):
    case("structured_cube", args + (p,), p, 0.05 if args == (2, 2, 2) else None).check()


# --------------------------------------------------------------------------- packing tails
@pytest.mark.parametrize("kind,args,p", [
    ("structured_square", (1, 1, 3), 3), ("structured_cube", (1, 1, 1, 2), 2),
    ("structured_square", (7, 1, 1), 1), ("structured_square", (7, 1, 2), 2),
    ("structured_square", (3, 2, 15), 15), ("structured_square", (3, 2, 16), 16)])
def test_packing_tails(vmod, kind, args, p):
    c = case(kind, args, p, 0.05)
    c.check("tail")
    per, tot = c.vol.integrate(c.u, return_per_element=True)
    pe, te = c.ext.integrate(c.u)
    parity(per, pe, c.f64.integrate(c.u)[0], "tail p %d integrate" % p)
    assert abs(float(tot) - float(te)) <= 1e-12 * float(np.abs(pe).sum())


# --------------------------------------------------------------------------- irregular sharing
@pytest.mark.parametrize("kind,args,p", [
    ("annulus", (4, 3, 6), 6), ("quads_from_triangles", (3, 3, 4), 4),
    ("shuffled", (3, 2, 5), 5), ("rcm", (3, 2, 5), 5)])
def test_irregular_sharing(vmod, kind, args, p):
    c = case(kind, args, p, 0.05 if kind in ("shuffled", "rcm") else None)
    c.check(kind)
    parity(c.vol.mass, c.ext.mass, c.f64.mass, kind + " mass")
    rows = np.bincount(c.e2n.astype(np.int64).ravel(), minlength=c.nn)
    assert c.vol.info()["max_contributions"] == rows.max()
    if kind == "quads_from_triangles":
        assert len(set(rows.tolist())) > 3                      # valences other than 4


def test_unreferenced_nodes_get_zero_and_nothing_is_written_outside(vmod):
    c = case("structured_square", (3, 2, 4), 4, 0.05, 3)
    assert c.vol.info()["referenced_nodes"] == c.nn - 3 and c.vol.n_node == c.nn
    assert torch.equal(c.vol.mass[-3:], torch.zeros(3, dtype=torch.float64, device="cuda"))
    big = torch.full((2 * c.nn + 16,), 7.0, dtype=torch.float64, device="cuda")
    out = big[8:8 + 2 * c.nn].view(2, c.nn)
    assert c.vol.recover(dev(c.u), out=out) is out
    assert torch.equal(out[:, -3:], torch.zeros_like(out[:, -3:]))
    assert torch.equal(big[:8], torch.full_like(big[:8], 7.0))
    assert torch.equal(big[-8:], torch.full_like(big[-8:], 7.0))
    c.check("padded")


# --------------------------------------------------------------------------- components
@pytest.mark.parametrize("kind,args,p", [("structured_square", (3, 2, 4), 4),
                                         ("structured_cube", (2, 2, 2, 2), 2)])
def test_components_and_layouts(vmod, kind, args, p):
    c = case(kind, args, p, 0.05)
    vol, nn = c.vol, c.nn
    rng = np.random.default_rng(3)
    calls = (vol.gradient, vol.recover, vol.integrate,
             lambda *a, **k: torch.stack(vol.norms(*a, **k)[2:], dim=-1))
    for ncomp in (1, 2, 3):
        u = dev(rng.standard_normal((ncomp, nn)))
        for call in calls:
            single = torch.stack([call(u[k]) for k in range(ncomp)])
            assert torch.equal(call(u), single)                          # component-major
    u = dev(rng.standard_normal((2, nn)))
    inter = u.T.contiguous().reshape(-1)
    for call in calls:
        assert torch.equal(call(inter, dofs_per_node=2), call(u))        # interleaved
    g = vol.gradient(u)
    assert tuple(g.shape) == (2, len(vol), c.ndim) + vol.eshape
    assert torch.equal(vol.integrate_local(g[:, :, 0]),
                       torch.stack([vol.integrate_local(g[k, :, 0]) for k in range(2)]))
    hg = vol.gradient(host(u))                                           # host in, host out
    assert isinstance(hg, np.ndarray) and np.array_equal(hg, host(g))
    n = vol.norms(host(u[0]), host(u[1]))
    assert isinstance(n.l2, np.floating) and n.l2 == float(vol.norms(u[0], u[1]).l2)


# --------------------------------------------------------------------------- the hot path
@pytest.mark.parametrize("ndim,p", [(2, p) for p in range(1, 17)]
                         + [(3, p) for p in (1, 2, 3, 4, 5, 6, 7, 8, 16)])
def test_norms_agree_with_the_poisson_action(vmod, ndim, p):
    if ndim == 2:
        c = case("structured_square", (2, 2, p), p, 0.05)
    elif p <= 8:
        c = case("structured_cube", (2, 2, 2, p) if p in (1, 2, 4, 8) else (2, 1, 1, p), p,
                 0.05 if p in (1, 2, 4, 8) else None)
    else:
        c = case("structured_cube", (2, 1, 1, p), p)
    u = dev(c.u)
    res = c.vol.norms(u)
    energy = float(torch.dot(u, c.op.apply(u)))
    gap_h1 = abs(float(res.h1_sq) - energy) / energy
    mass_u2 = float((c.vol.mass * u * u).sum())
    gap_l2 = abs(float(res.l2_sq) - mass_u2) / mass_u2
    print("ndim %d p %d: |h1^2 - u.Ku| / u.Ku = %.2e, |l2^2 - sum m u^2| / . = %.2e"
          % (ndim, p, gap_h1, gap_l2))
    assert gap_h1 <= 1e-10 and gap_l2 <= 1e-13


# --------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("kind,args,p", [("structured_square", (3, 2, p), p)
                                         for p in (1, 2, 5, 8, 16)]
                         + [("structured_cube", (2, 1, 1, p), p) for p in (2, 4)])
def test_polynomials_are_differentiated_exactly(vmod, kind, args, p):
    c = case(kind, args, p, 0.0)                                 # affine elements
    x = c.xn.astype(np.longdouble)
    a, b = p, max(p - 1, 1)
    # on hexahedra times z^p, so that every row of invJ and every local
    # derivative meets an analytic value
    z, dz = (x[2] ** p, p * x[2] ** (p - 1)) if c.ndim == 3 else (1.0, None)
    u = (x[0] ** a * x[1] ** b * z).astype(np.float64)
    exact = np.zeros((c.ndim, c.nn), np.longdouble)
    exact[0] = a * x[0] ** (a - 1) * x[1] ** b * z
    exact[1] = b * x[0] ** a * x[1] ** (b - 1) * z
    if c.ndim == 3:
        exact[2] = x[0] ** a * x[1] ** b * dz
    exact_e = np.moveaxis(exact[:, c.e2n.astype(np.int64)], 0, 1)        # [E, ndim, n, ..]
    parity(c.vol.gradient(u), exact_e, c.f64.gradient(u), "p %d x^%d y^%d gradient" % (p, a, b))
    parity(c.vol.recover(u), exact, c.f64.recover(u), "p %d x^%d y^%d recover" % (p, a, b))
    per, res = c.vol.norms(u, u, return_per_element=True)
    assert not host(per).any() and float(res.l2) == 0.0 and float(res.h1) == 0.0


# --------------------------------------------------------------------------- errors
def test_errors(vmod):
    c = case("structured_square", (3, 2, 4), 4, 0.05)
    x_phys = c.vol.x_phys.cpu().numpy().copy()
    e2n = c.e2n.copy()
    x_phys[1] = x_phys[1][:, ::-1]                               # element 1 inverted
    e2n[1] = e2n[1][::-1]
    with pytest.raises(AssertionError) as err:
        vmod.VolumeSet(x_phys=x_phys, e2n=e2n, n_node=c.nn, device="cuda:0")
    assert "detJ <= 0 at 25 element nodes" in str(err.value)
    with pytest.raises(ValueError):
        vmod.VolumeSet(x_phys=c.vol.x_phys, e2n=c.e2n, n_node=c.nn - 1, device="cuda:0")
    for call in (c.vol.gradient, c.vol.recover, c.vol.integrate, c.vol.norms):
        with pytest.raises(ValueError):
            call(np.zeros(c.nn + 1))
        with pytest.raises(ValueError):
            call(np.zeros(2 * c.nn + 1), dofs_per_node=2)
    with pytest.raises(ValueError):
        c.vol.norms(np.zeros(c.nn), np.zeros((2, c.nn)))
    with pytest.raises(ValueError):
        c.vol.integrate_local(np.zeros((len(c.vol), 5, 4)))
    with pytest.raises(ValueError):
        c.vol.gradient(np.zeros(c.nn), out=torch.zeros(3, dtype=torch.float64, device="cuda"))
    empty = vmod.VolumeSet(x_phys=c.vol.x_phys[:0], e2n=c.e2n[:0], n_node=4, device="cuda:0")
    assert float(empty.integrate(np.ones(4))) == 0.0 and not host(empty.recover(np.ones(4))).any()
    assert not host(empty.mass).any() and empty.gradient(np.ones(4)).shape == (0, 2, 5, 5)


# --------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kind,args,p", [("structured_square", (3, 2, 8), 8),
                                         ("structured_cube", (2, 2, 2, 4), 4)])
def test_repeatability_and_graph_capture(vmod, kind, args, p):
    c = case(kind, args, p, 0.05)
    vol = c.vol
    u, v = dev(np.stack([c.u, c.v])), dev(np.stack([c.v, c.u]))
    for call in (lambda: vol.recover(u), lambda: vol.integrate(u),
                 lambda: torch.stack(vol.norms(u, v)[2:])):
        assert torch.equal(call(), call())
    eager = vol.gradient(u).clone(), vol.recover(u).clone(), \
        torch.stack(vol.norms(u, v)[2:], dim=-1).clone()
    outs = [torch.zeros_like(t) for t in eager]

    def step(stream=None):
        vol.gradient(u, out=outs[0], stream=stream)
        vol.recover(u, out=outs[1], stream=stream)
        vol.norms(u, v, out=outs[2], stream=stream)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e)


# --------------------------------------------------------------------------- facade
def test_dof_manager_facade(vmod):
    from spectralelementmethod_amd import meshgen
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManager, Mesh
    p = 5
    dm = DOFManager(Mesh.from_arrays(*meshgen.structured_square(3, 2, p, warp=0.05)), 1,
                    gll_basis_2d(p), device="cuda:0")                    # RCM numbering
    xn = dm.mesh.nodes
    u = vt.smooth(xn)
    v = u * (1.0 + 1e-3 * np.cos(xn[0]))
    fes = list(dm.finite_elements(x_phys=True, Jacobian=True))
    grad = np.stack([fe.gradient(u[fe.node_ind]) for fe in fes])
    got = dm.gradient(u)
    assert isinstance(got, np.ndarray) and rel_l2(got, grad) <= 1e-12
    total = sum(fe.integrate(u[fe.node_ind]) for fe in fes)
    assert abs(dm.integrate(u) - total) <= 1e-12 * abs(total)
    d = u - v
    l2 = np.sqrt(sum(fe.integrate(d[fe.node_ind] ** 2) for fe in fes))
    h1 = np.sqrt(sum(fe.integrate((fe.gradient(d[fe.node_ind]) ** 2).sum(axis=0)) for fe in fes))
    assert abs(dm.norm(u, v) - l2) <= 1e-12 * l2
    assert abs(dm.norm(u, v, kind="h1") - h1) <= 1e-12 * h1
    assert dm.norm(u) == dm.volume_set().norms(u).l2 and dm.volume_set() is dm.volume_set()
    with pytest.raises(ValueError):
        dm.norm(u, kind="h2")
    with pytest.raises(ValueError):
        dm.gradient(u[:-1])
