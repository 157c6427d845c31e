"""Hexahedral Poisson action on the fp64 matrix cores (k_hex_mfma,
kernel="mfma" on 3-D meshes, p = 11..16).

The standard mesh, structured_cube(3, 2, 2, p, warp=0.05), is the smallest
on which the kernel can still go wrong: four xi0 chains of three elements
(the register carry and both chain-end faces) and faces, edges and corners
shared across workgroups (column slots, the seam sum).  Yardsticks:

* the extended-precision evaluation of the action (as test_hex_orders_vs_oracle
  above p = 10): within 1e-11 of it and no further from it than the float64
  oracle (or 1e-12);
* the column form on identical device factors: only the summation order of
  the contractions differs.  Two float64 summation orders of this action
  differ by 2.1e-16 .. 2.4e-16 on this mesh at p = 11..16; 1e-13 leaves a
  factor of ~400 for FMA contraction in the matrix pipe, and any indexing
  fault shows at 1e-6 or above."""
import numpy as np
import pytest

from conftest import rel_l2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-12      # floor of the float64-oracle comparison
TOL_HI = 1e-11   # p = 11..16 vs the extended-precision oracle / float64 oracle at p = 12
TOL_FORM = 1e-13  # matrix-core form vs column form, identical factors
ORDERS = range(11, 17)


@pytest.fixture(scope="module")
def sem():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from spectralelementmethod_amd import operators
    return operators


def _oracle(gll, nodes, e2n, p):
    import sem_oracle
    return sem_oracle.HexPoissonProblem(nodes, e2n, gll["half_%d" % p])


@pytest.fixture(scope="module")
def standard(sem, gll):
    """Per order, computed once and left unchanged: the standard mesh, u, and
    the column form's action of u."""
    from spectralelementmethod_amd import meshgen
    cache = {}

    def get(p):
        if p not in cache:
            nodes, e2n = meshgen.structured_cube(3, 2, 2, p, warp=0.05)
            u = np.random.default_rng(p).standard_normal(nodes.shape[1])
            col = sem.SEMOperator(p, e2n, nodes, kernel="column")
            y_col = col.apply(torch.from_numpy(u).cuda()).cpu().numpy()
            assert col.plan_info()["kernel"] == "column"
            col.close()
            cache[p] = dict(nodes=nodes, e2n=e2n, u=u, y_col=y_col)
        return cache[p]
    return get


def _mfma_action(sem, p, e2n, nodes, u):
    op = sem.SEMOperator(p, e2n, nodes, kernel="mfma")
    y = op.apply(torch.from_numpy(u).cuda()).cpu().numpy()
    return op, y


@pytest.mark.parametrize("p", ORDERS)
def test_hex_mfma_orders_vs_oracle(sem, gll, standard, p):
    import sem_oracle
    S = standard(p)
    nodes, e2n, u = S["nodes"], S["e2n"], S["u"]
    op, y = _mfma_action(sem, p, e2n, nodes, u)
    info = op.plan_info()
    assert info["kernel"] == "mfma" and info["hex_kernel"] == "mfma"
    assert info["ndim"] == 3 and info["chains"] == 4
    P = _oracle(gll, nodes, e2n, p)
    ext = np.asarray(sem_oracle.hex_poisson_apply_extended(nodes, e2n, gll["half_%d" % p], u),
                     dtype=np.float64)
    err, err_f64 = rel_l2(y, ext), rel_l2(P.apply(u), ext)
    print("p=%d mfma vs extended %.2e, float64 oracle vs extended %.2e" % (p, err, err_f64))
    assert err < TOL_HI and err <= max(err_f64, TOL)


@pytest.mark.parametrize("p", ORDERS)
def test_hex_mfma_vs_column_same_factors(sem, standard, p):
    S = standard(p)
    op, y = _mfma_action(sem, p, S["e2n"], S["nodes"], S["u"])
    assert op.plan_info()["template_map"]  # the structured numbering: template-map instantiation
    err = rel_l2(y, S["y_col"])
    print("p=%d mfma vs column %.2e" % (p, err))
    assert err < TOL_FORM


@pytest.mark.parametrize("p", [12, 16])
def test_hex_mfma_accumulate(sem, standard, p):
    S = standard(p)
    op = sem.SEMOperator(p, S["e2n"], S["nodes"], kernel="mfma")
    u = torch.from_numpy(S["u"]).cuda()
    y0 = torch.from_numpy(np.random.default_rng(100 + p).standard_normal(S["u"].size)).cuda()
    y = op.apply(u, out=y0.clone(), accumulate=True)
    err = rel_l2(y.cpu().numpy(), y0.cpu().numpy() + S["y_col"])
    print("p=%d accumulate %.2e" % (p, err))
    assert err < TOL_FORM


def _permute_local(e2n, rng, frac=0.5):
    """Re-orient a fraction of the elements (swap / reverse local axes): the
    mesh is the same, the xi0 chains break wherever orientations differ."""
    e2n = e2n.copy()
    for e in np.flatnonzero(rng.random(e2n.shape[0]) < frac):
        perm = rng.permutation(3)
        flips = rng.random(3) < 0.5
        # orientation-preserving only (a reflection would make detJ < 0)
        sign = np.linalg.det(np.eye(3)[perm]) * (-1) ** int(flips.sum())
        if sign < 0:
            flips[0] = not flips[0]
        t = np.transpose(e2n[e], perm)
        for ax in range(3):
            if flips[ax]:
                t = np.flip(t, axis=ax)
        e2n[e] = t
    return e2n


@pytest.mark.parametrize("warp", [0.0, 0.05])
@pytest.mark.parametrize("case", ["shuffle_nodes", "shuffle_elements", "reoriented"])
def test_hex_mfma_numberings_that_defeat_the_plan(sem, gll, case, warp):
    """p = 12 on structured_cube(3, 2, 2): shuffled node ids (no template
    map: the per-element map instantiation), shuffled elements (the chains
    break) and re-oriented elements, each against the column form on the same
    numbering (1e-13) and, on the plain cube, against the float64 oracle
    (1e-11).

    The float64 oracle is compared on the unwarped cube only: its own
    distance from the extended-precision action at p = 12 is 4.5e-13 ..
    7.3e-13 there, but 8.2e-12 / 9.8e-12 / 1.07e-11 (re-oriented / shuffled
    elements / shuffled nodes) on the warp = 0.05 mesh, and 0.86e-11 ..
    1.34e-11 at warp = 0.01 .. 0.03 (host arithmetic only, no device code
    involved): at 1e-11 a comparison with it on a warped mesh measures the
    oracle's rounding of the equispaced -> GLL transform, not
    the kernel.  The warped mesh, where the cross factors G01 / G02 / G12 are
    non-zero, is covered by the column-form comparison on identical factors."""
    from spectralelementmethod_amd import meshgen
    p = 12
    nodes, e2n = meshgen.structured_cube(3, 2, 2, p, warp=warp)
    rng = np.random.default_rng(5)
    if case == "shuffle_nodes":
        nodes, e2n = meshgen.shuffle_nodes(nodes, e2n, seed=4)
    elif case == "shuffle_elements":
        e2n = meshgen.shuffle_elements(e2n, seed=3)
    else:
        e2n = _permute_local(e2n, rng)
    u = rng.standard_normal(nodes.shape[1])
    op, y = _mfma_action(sem, p, e2n, nodes, u)
    info = op.plan_info()
    assert info["hex_kernel"] == "mfma"
    if case == "shuffle_nodes":
        assert not info["template_map"]  # the per-element map instantiation
    col = sem.SEMOperator(p, e2n, nodes, kernel="column")
    y_col = col.apply(torch.from_numpy(u).cuda()).cpu().numpy()
    err_col = rel_l2(y, y_col)
    print("%s warp %g: mfma vs column %.2e" % (case, warp, err_col))
    assert err_col < TOL_FORM
    if warp == 0.0:
        err = rel_l2(y, _oracle(gll, nodes, e2n, p).apply(u))
        print("%s warp %g: mfma vs float64 oracle %.2e" % (case, warp, err))
        assert err < TOL_HI


def test_hex_mfma_is_deterministic(sem):
    from spectralelementmethod_amd import meshgen
    p = 15
    nodes, e2n = meshgen.structured_cube(4, 3, 2, p, warp=0.05)
    op = sem.SEMOperator(p, e2n, nodes, kernel="mfma")
    assert op.plan_info()["hex_kernel"] == "mfma"
    u = torch.from_numpy(np.random.default_rng(1).standard_normal(nodes.shape[1])).cuda()
    y1 = op.apply(u).clone()
    for _ in range(3):
        assert torch.equal(op.apply(u), y1)


def test_hex_mfma_solver_path(sem):
    """sem_pcg_solve and sem_apply_dot reach the matrix-core form through the
    same dispatch point as sem_apply."""
    from spectralelementmethod_amd import meshgen
    p = 11
    nodes, e2n = meshgen.structured_cube(2, 2, 2, p, warp=0.05)
    ebc = np.abs(nodes[0] + 1) < 1e-12
    sol = {}
    for kernel in ("mfma", "column"):
        op = sem.SEMOperator(p, e2n, nodes, kernel=kernel)
        F = op.assemble(op.geometry_fields()["detJxW"])
        x = torch.zeros(nodes.shape[1], dtype=torch.float64, device="cuda")
        x, its, rel = op.pcg_solve(F, x, ebc, rtol=1e-14, max_iter=5000)
        assert op.plan_info()["kernel"] == kernel
        sol[kernel] = x.cpu().numpy()
        if kernel == "mfma":
            u = torch.from_numpy(np.random.default_rng(2).standard_normal(nodes.shape[1])).cuda()
            y = op.apply(u).clone()
            yd, dot = op.apply_dot(u)
            assert torch.equal(yd, y)
            ref = torch.dot(u, y).item()
            assert abs(dot.item() - ref) <= 1e-12 * abs(ref)
    err = rel_l2(sol["mfma"], sol["column"])
    print("pcg mfma vs column %.2e" % err)
    assert err < 1e-10


def test_hex_mfma_limits(sem, gll, monkeypatch):
    from spectralelementmethod_amd import meshgen
    nodes8, e2n8 = meshgen.structured_cube(2, 2, 2, 8, warp=0.05)
    with pytest.raises(NotImplementedError):
        sem.SEMOperator(8, e2n8, nodes8, kernel="mfma")
    nodes12, e2n12 = meshgen.structured_cube(2, 1, 1, 12)
    with pytest.raises(NotImplementedError):
        sem.SEMOperator(12, e2n12, nodes12, kernel="mfma", geometry="nodal")
    # the defaults keep the column forms
    monkeypatch.delenv("SEM_KERNEL", raising=False)
    for p, form in ((12, "three_block"), (16, "rows")):
        nodes, e2n = meshgen.structured_cube(2, 1, 1, p)
        info = sem.SEMOperator(p, e2n, nodes).plan_info()
        assert info["kernel"] == "column" and info["hex_kernel"] == form
    # SEM_KERNEL=1 in the environment: the matrix-core form where it is built,
    # silently the column form elsewhere
    monkeypatch.setenv("SEM_KERNEL", "1")
    nodes, e2n = meshgen.structured_cube(2, 1, 1, 15)
    assert sem.SEMOperator(15, e2n, nodes).plan_info()["hex_kernel"] == "mfma"
    op = sem.SEMOperator(8, e2n8, nodes8)
    assert op.plan_info()["hex_kernel"] == "three_block"
    u = np.random.default_rng(8).standard_normal(nodes8.shape[1])
    y = op.apply(torch.from_numpy(u).cuda()).cpu().numpy()
    assert rel_l2(y, _oracle(gll, nodes8, e2n8, 8).apply(u)) < TOL
