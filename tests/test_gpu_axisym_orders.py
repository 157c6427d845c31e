"""The axisymmetric kernels (Stokes block stored / nodal, Navier-Stokes
residual, Jacobian-vector product; two DOFs per node) at every order
p = 1..16 against the extended-precision oracle (oracle/sem_oracle.py
axisym_*_extended), and the quadrilateral Poisson diag() against an
independent value.

Two yardsticks (measured per order: tools/axisym_accuracy.py):

* factors installed (set_geometry with the float64 oracle's factors, the same
  factors cast up on the oracle's side): only the operator arithmetic
  differs.  Bar 1e-13: the float64 NumPy evaluation of the same formulas is
  <= 2.6e-16 from that reference at every order, a kernel summing n <= 17
  terms in four contractions and up to four element contributions per node
  in another order stays within a few n eps ~ 1e-14; ten times that.
* geometry from the mesh on both sides: the rule of test_gpu_parity.py
  assert_parity (1e-12 against the float64 oracle or the extended one, else
  at least as accurate as the float64 oracle) and the north-star 1e-10
  against the extended evaluation.  The nodal Stokes kernel derives its
  factors from the mesh only (installed factors switch it off), so it is
  always judged this way.

Meshes: annulus(5, 2 * (64 // n) + 1, p), n = p + 1: five element lines (a
one-line tail after a block of four), lines of 2 EPW + 1 elements (more than
two wavefront groups, a partly filled last group).  Its lines are no whole
number of chains, so the planner takes the element-coloured plan there; the
plan variants (seams, colour launches, pattern table, 16- / 32-bit map) run
on annulus(8, 16 * (64 // n), p) as well, the smallest mesh on which the
pattern table is built in both seam modes (128 groups)."""
import functools

import numpy as np
import pytest

from conftest import load_golden, rel_l2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RE = 5.0
TOL_FACTORS = 1e-13   # installed factors: operator arithmetic only
TOL_PARITY = 1e-12    # geometry from the mesh (assert_parity rule)
TOL_NORTH_STAR = 1e-10
KNOBS = ("SEM_PLAN", "SEM_SEAM", "SEM_MAP_PATTERNS", "SEM_MAP16")


@pytest.fixture(scope="module")
def sem():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import operators
    return operators


def _mesh(p, kind):
    from spectralelementmethod_amd import meshgen
    n = p + 1
    if kind == "tail":
        return meshgen.annulus(5, 2 * (64 // n) + 1, p)
    if kind == "chain":
        return meshgen.annulus(8, 16 * (64 // n), p)
    if kind == "tail-shuffled":
        return meshgen.shuffle_nodes(*_mesh(p, "tail"))
    if kind == "chain-shuffled":
        return meshgen.shuffle_nodes(*_mesh(p, "chain"))
    nodes, e2n = meshgen.quads_from_triangles(4, 3, p)
    nodes[0] += 3.0  # rho > 0
    if kind == "tri-shuffled":
        e2n = meshgen.shuffle_elements(e2n)
    else:
        assert kind == "tri"
    return nodes, e2n


class Case(object):
    """Mesh, inputs, float64 factors and the references of one (p, mesh);
    built once and shared (references are computed on first use)."""

    def __init__(self, p, kind):
        import sem_oracle
        self.so = sem_oracle
        self.p = p
        self.nodes, self.e2n = _mesh(p, kind)
        self.half = load_golden("gll.npz")["half_%d" % p]
        self.prob = sem_oracle.PoissonProblem(self.nodes, self.e2n, self.half)
        self.F = sem_oracle.axisym_ns_factors(self.prob.x_phys, self.prob.invJ, self.prob.detJxW)
        rng = np.random.default_rng(p)
        self.nn = self.nodes.shape[1]
        self.s = rng.standard_normal(2 * self.nn)
        self.d = rng.standard_normal(2 * self.nn)
        self.s2 = rng.standard_normal(2 * self.nn)
        self._cache = {}

    def _get(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def ext_factors(self):
        """(Stokes, NS, JVP) in extended precision from the installed factors."""
        so, h, e = self.so, self.half, self.e2n
        return self._get("ext_f", lambda: (
            so.axisym_apply_extended(h, e, self.s, F=self.F),
            so.axisym_ns_apply_extended(h, e, self.s, RE, F=self.F),
            so.axisym_ns_jvp_extended(h, e, self.s, self.d, RE, F=self.F)))

    def ext_mesh(self):
        so, h, e = self.so, self.half, self.e2n
        return self._get("ext_m", lambda: (
            so.axisym_apply_extended(h, e, self.s, nodes=self.nodes),
            so.axisym_ns_apply_extended(h, e, self.s, RE, nodes=self.nodes),
            so.axisym_ns_jvp_extended(h, e, self.s, self.d, RE, nodes=self.nodes)))

    def f64_mesh(self):
        so, pr = self.so, self.prob
        return self._get("f64", lambda: (
            so.axisym_apply(self.F[:, :7], pr.D, pr.e2n, self.s, self.nn),
            so.axisym_ns_apply(self.F, pr.D, pr.quad, pr.e2n, self.s, self.nn, RE),
            so.axisym_ns_jvp(self.F, pr.D, pr.quad, pr.e2n, self.s, self.d, self.nn, RE)))


@functools.lru_cache(maxsize=None)
def case(p, kind="tail"):
    return Case(p, kind)


def components(y, ref):
    """Relative L2 per component: y[0::2] (omega row), y[1::2] (psi row)."""
    return rel_l2(y[0::2], ref[0::2]), rel_l2(y[1::2], ref[1::2])


def assert_factors(y, ext, what):
    e = components(y, ext)
    print("%s: device to extended (installed factors) %.2e %.2e" % ((what,) + e))
    assert max(e) <= TOL_FACTORS, (what, e)


def assert_mesh(y, ref, ext, what):
    """assert_parity of test_gpu_parity.py per component, and the north star."""
    for k in (0, 1):
        yk, rk, xk = y[k::2], ref[k::2], ext[k::2]
        e_ref, e_self, e_refx = rel_l2(yk, rk), rel_l2(yk, xk), rel_l2(rk, xk)
        print("%s[%d]: device to oracle %.2e, device to extended %.2e, oracle to extended %.2e"
              % (what, k, e_ref, e_self, e_refx))
        assert e_self <= TOL_NORTH_STAR, (what, k, e_self)
        if e_ref < TOL_PARITY or e_self < TOL_PARITY:
            continue
        assert e_self <= max(1.5 * e_refx, TOL_PARITY), (what, k, e_self, e_refx)
        assert e_ref <= 2.0 * e_refx + TOL_PARITY, (what, k, e_ref, e_refx)


def installed(sem, c, **kw):
    """Operator with the float64 oracle's factors installed (stored kernels)."""
    op = sem.SEMOperator(c.p, c.e2n, c.nodes, dofs_per_node=2, **kw)
    op.set_geometry(c.F[:, :7], kind="axisym_stokes")
    op.set_geometry(c.F, kind="axisym_ns")
    op.set_reynolds(RE)
    return op


def run3(op, c):
    """Stokes, NS (recording the linearisation), JVP -> numpy."""
    s, d = torch.from_numpy(c.s).cuda(), torch.from_numpy(c.d).cuda()
    return [op.apply(s, kind="axisym_stokes").cpu().numpy(),
            op.apply(s, kind="axisym_ns", linearize=True).cpu().numpy(),
            op.apply(d, kind="axisym_ns_jvp").cpu().numpy()]


def nodal_stokes(sem, c):
    op = sem.SEMOperator(c.p, c.e2n, c.nodes, dofs_per_node=2, geometry="nodal")
    y = op.apply(torch.from_numpy(c.s).cuda(), kind="axisym_stokes").cpu().numpy()
    assert op.plan_info()["geometry_axisym"] == "nodal"
    return op, y


# ---------------------------------------------------------------------------
# a. operator arithmetic, factors installed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", list(range(1, 17)))
def test_axisym_installed_factors_all_orders(sem, p):
    c = case(p)
    op = installed(sem, c)
    assert op.plan_info()["geometry_axisym"] == "stored"
    for y, ext, what in zip(run3(op, c), c.ext_factors(), ("stokes", "ns", "jvp")):
        assert_factors(y, ext, "p=%d %s" % (p, what))


# ---------------------------------------------------------------------------
# b. production path, geometry from the mesh
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["stored", "nodal", "auto"])
@pytest.mark.parametrize("p", list(range(1, 17)))
def test_axisym_mesh_geometry_all_orders(sem, p, geometry):
    c = case(p)
    n = p + 1
    op = sem.SEMOperator(p, c.e2n, c.nodes, dofs_per_node=2, geometry=geometry)
    op.set_reynolds(RE)
    s = torch.from_numpy(c.s).cuda()
    y = op.apply(s, kind="axisym_stokes").cpu().numpy()
    expect = geometry if geometry != "auto" else ("nodal" if (n <= 7 or n == 17) else "stored")
    assert op.plan_info()["geometry_axisym"] == expect
    assert_mesh(y, c.f64_mesh()[0], c.ext_mesh()[0], "p=%d stokes %s" % (p, expect))
    if geometry == "stored":  # NS and JVP take stored factors in every mode: once per order
        yn = op.apply(s, kind="axisym_ns", linearize=True).cpu().numpy()
        yj = op.apply(torch.from_numpy(c.d).cuda(), kind="axisym_ns_jvp").cpu().numpy()
        assert_mesh(yn, c.f64_mesh()[1], c.ext_mesh()[1], "p=%d ns" % p)
        assert_mesh(yj, c.f64_mesh()[2], c.ext_mesh()[2], "p=%d jvp" % p)


# ---------------------------------------------------------------------------
# c. plan and map variants
# ---------------------------------------------------------------------------
VARIANT_ORDERS = (1, 2, 3, 7, 8, 10, 12, 14, 15, 16)


def _variant(sem, monkeypatch, c, env, expect):
    """Both operators of one variant (stored with installed factors, nodal
    from the mesh) with the plan_info it must report; -> four outputs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    op = installed(sem, c)
    opn, yn = nodal_stokes(sem, c)
    for o in (op, opn):
        info = o.plan_info()
        for k, v in expect.items():
            if k == "map_patterns":  # True: a table was built
                assert (info[k] > 0) == v, (env, k, info)
            elif k == "atomic":
                assert (info["atomic_groups"] > 0) == v, (env, info)
            else:
                assert info[k] == v, (env, k, info)
    return run3(op, c) + [yn], op.plan_info()


def _check_variant(c, ys, tag):
    for y, ext, what in zip(ys[:3], c.ext_factors(), ("stokes", "ns", "jvp")):
        assert_factors(y, ext, "%s %s" % (tag, what))
    assert_mesh(ys[3], c.f64_mesh()[0], c.ext_mesh()[0], "%s stokes nodal" % tag)


def _check_agree(outs):
    names = list(outs)
    for name in names[1:]:
        for a, b, what in zip(outs[names[0]], outs[name], ("stokes", "ns", "jvp", "nodal")):
            e = rel_l2(a, b)
            print("%s vs %s %s: %.2e" % (name, names[0], what, e))
            assert e <= 1e-15, (name, names[0], what, e)


@pytest.mark.parametrize("p", VARIANT_ORDERS)
def test_axisym_variants_chain_mesh(sem, monkeypatch, p):
    """Seam plan / colour launches x pattern table / 16-bit map / 32-bit map:
    the six forms of k_axisym_nodal (two-plane from p = 8) and both forms of
    k_axisym_apply, each asserted through plan_info."""
    c = case(p, "chain")
    pat = p >= 2  # PatternMap<N>: n >= 3
    outs = {}
    for seam in ("1", "0"):
        plan = "chains-seams" if seam == "1" else "chains"
        for name, env, expect in (
                ("pat", {}, dict(map_entry_bytes=2, map_patterns=pat)),
                ("m16", {"SEM_MAP_PATTERNS": "0"}, dict(map_entry_bytes=2, map_patterns=False)),
                ("m32", {"SEM_MAP16": "0"}, dict(map_entry_bytes=4, map_patterns=False))):
            env = dict(env, SEM_SEAM=seam)
            tag = "p=%d chain seam=%s %s" % (p, seam, name)
            ys, info = _variant(sem, monkeypatch, c, env, dict(expect, plan=plan, atomic=False))
            assert (info["seam_nodes"] > 0) == (seam == "1"), info
            assert info["colours"] == (1 if seam == "1" else 4), info
            _check_variant(c, ys, tag)
            outs[tag] = ys
    _check_agree(outs)


@pytest.mark.parametrize("p", VARIANT_ORDERS)
def test_axisym_variants_tail_mesh(sem, monkeypatch, p):
    """Lines of 2 EPW + 1 elements: element-coloured chains by default,
    chains whose groups all emit with atomics when element colouring is
    forbidden (SEM_PLAN=0), and the 32-bit map."""
    c = case(p)
    outs = {}
    for name, env, expect in (
            ("default", {}, dict(plan="element-coloured", atomic=False)),
            ("m32", {"SEM_MAP16": "0"}, dict(plan="element-coloured", map_entry_bytes=4,
                                             atomic=False)),
            ("atomic", {"SEM_PLAN": "0"}, dict(plan="chains", atomic=True))):
        tag = "p=%d tail %s" % (p, name)
        ys, info = _variant(sem, monkeypatch, c, env, expect)
        assert info["colours"] > 1, info
        _check_variant(c, ys, tag)
        outs[tag] = ys
    _check_agree(outs)


@pytest.mark.parametrize("kind", ["tail-shuffled", "chain-shuffled"])
@pytest.mark.parametrize("p", VARIANT_ORDERS)
def test_axisym_variants_shuffled_nodes(sem, monkeypatch, p, kind):
    """Randomly renumbered nodes: a group row's ids leave the 16-bit window
    and the plan falls back to the 32-bit map on its own."""
    c = case(p, kind)
    plan = "element-coloured" if kind == "tail-shuffled" else "chains-seams"
    expect = dict(plan=plan, map_patterns=False)
    # up to 4096 nodes (p = 1, 2, 3 on the tail mesh) every row fits the 12-bit window
    if not (kind == "tail-shuffled" and c.nn <= 4096):
        expect["map_entry_bytes"] = 4
    ys, _ = _variant(sem, monkeypatch, c, {}, expect)
    _check_variant(c, ys, "p=%d %s" % (p, kind))


# ---------------------------------------------------------------------------
# d. accumulate and linearisation state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 8, 11, 16])
def test_axisym_accumulate_and_linearisation_state(sem, p):
    c = case(p)
    op = installed(sem, c)
    opn = sem.SEMOperator(p, c.e2n, c.nodes, dofs_per_node=2, geometry="nodal")
    s1, s2 = torch.from_numpy(c.s).cuda(), torch.from_numpy(c.s2).cuda()
    d = torch.from_numpy(c.d).cuda()
    y0 = torch.from_numpy(np.random.default_rng(100 + p).standard_normal(2 * c.nn)).cuda()
    for o, kind in ((op, "axisym_stokes"), (opn, "axisym_stokes"), (op, "axisym_ns")):
        ref = o.apply(s1, kind=kind)
        y = y0.clone()
        o.apply(s1, out=y, kind=kind, accumulate=True)
        e = ((y - (y0 + ref)).norm() / ref.norm()).item()
        print("p=%d %s accumulate: %.2e" % (p, kind, e))
        assert e <= 1e-13, (kind, e)
        # overwrite mode does not depend on the previous contents of out
        y.fill_(123.0)
        o.apply(s1, out=y, kind=kind)
        e = ((y - ref).norm() / ref.norm()).item()
        assert e <= 1e-13, (kind, e)
    assert opn.plan_info()["geometry_axisym"] == "nodal"
    # the recorded linearisation survives applies that do not record
    op.apply(s1, kind="axisym_ns", linearize=True)
    j1 = op.apply(d, kind="axisym_ns_jvp")
    op.apply(s2, kind="axisym_stokes")
    op.apply(s2, kind="axisym_ns")
    assert torch.equal(op.apply(d, kind="axisym_ns_jvp"), j1)
    assert_factors(j1.cpu().numpy(), c.ext_factors()[2], "p=%d jvp at s1" % p)
    # and is replaced by the next recording one
    op.apply(s2, kind="axisym_ns", linearize=True)
    j2 = op.apply(d, kind="axisym_ns_jvp").cpu().numpy()
    ext2 = c.so.axisym_ns_jvp_extended(c.half, c.e2n, c.s2, c.d, RE, F=c.F)
    assert_factors(j2, ext2, "p=%d jvp at s2" % p)
    # only the omega row (y[0::2]) carries the state; two independent N(0, 1)
    # states give advection terms that differ by O(1) of the row
    apart = rel_l2(j2[0::2], c.ext_factors()[2][0::2])
    print("p=%d jvp at s2 against the reference at s1: %.2e" % (p, apart))
    assert apart > 1e-3, apart


# ---------------------------------------------------------------------------
# e. unstructured map, two DOFs per node
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tri", "tri-shuffled"])
@pytest.mark.parametrize("p", [2, 7, 11])
def test_axisym_unstructured(sem, p, kind):
    """Split-triangle quadrilaterals (three elements around interior nodes),
    as generated and in a random element order."""
    c = case(p, kind)
    op = installed(sem, c)
    info = op.plan_info()
    tag = "p=%d %s plan=%s atomic_groups=%d of %d map=%dB" % (
        p, kind, info["plan"], info["atomic_groups"], info["groups"], info["map_entry_bytes"])
    print(tag)
    for y, ext, what in zip(run3(op, c), c.ext_factors(), ("stokes", "ns", "jvp")):
        assert_factors(y, ext, "%s %s" % (tag, what))
    opn, yn = nodal_stokes(sem, c)
    assert opn.plan_info()["plan"] == info["plan"]
    assert_mesh(yn, c.f64_mesh()[0], c.ext_mesh()[0], "%s stokes nodal" % tag)


# ---------------------------------------------------------------------------
# Quadrilateral diag() against an independent value
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def diag_case(p, shuffled=False):
    import sem_oracle
    from spectralelementmethod_amd import meshgen
    nodes, e2n = meshgen.structured_square(5, 4, p, warp=0.05)
    if shuffled:
        nodes, e2n = meshgen.shuffle_nodes(nodes, e2n)
    half = load_golden("gll.npz")["half_%d" % p]
    prob = sem_oracle.PoissonProblem(nodes, e2n, half)
    n2 = (p + 1) ** 2
    # float64 side: the diagonal of the reference's dense element matrices, assembled
    dL = np.stack([np.diagonal(prob.element_matrices([e])[0].reshape(n2, n2))
                   for e in range(e2n.shape[0])])
    d64 = np.bincount(prob.e2n.ravel(), weights=dL.ravel(), minlength=prob.ndof)
    return dict(nodes=nodes, e2n=e2n, prob=prob, d64=d64,
                ext_G=sem_oracle.poisson_diag_extended(half, e2n, G=prob.G, ndof=prob.ndof),
                ext_mesh=sem_oracle.poisson_diag_extended(half, e2n, nodes=nodes))


def _check_diag(sem, p, shuffled):
    c = diag_case(p, shuffled)
    op = sem.SEMOperator(p, c["e2n"], c["nodes"])
    op.set_geometry(c["prob"].G)
    e = rel_l2(op.diag().cpu().numpy(), c["ext_G"])
    print("p=%d diag, installed factors: %.2e" % (p, e))
    assert e <= TOL_FACTORS, e
    for geometry in ("stored", "nodal"):
        op = sem.SEMOperator(p, c["e2n"], c["nodes"], geometry=geometry)
        d = op.diag().cpu().numpy()
        e_ref, e_self = rel_l2(d, c["d64"]), rel_l2(d, c["ext_mesh"])
        e_refx = rel_l2(c["d64"], c["ext_mesh"])
        print("p=%d diag %s: device to oracle %.2e, to extended %.2e, oracle to extended %.2e"
              % (p, geometry, e_ref, e_self, e_refx))
        if e_ref < TOL_PARITY:
            continue
        assert e_self <= max(1.5 * e_refx, TOL_PARITY), (geometry, e_self, e_refx)
        assert e_ref <= 2.0 * e_refx + TOL_PARITY, (geometry, e_ref, e_refx)


@pytest.mark.parametrize("p", list(range(1, 17)))
def test_poisson_diag_all_orders(sem, p):
    _check_diag(sem, p, False)


def test_poisson_diag_shuffled_nodes(sem):
    _check_diag(sem, 8, True)
