"""GPU tests of the p-multigrid preconditioner (multigrid.PMultigrid,
sem_mg_* in include/sem_hip.h) against the float64 twin of
the stated cycle (tests/mg_twin.py, itself checked on the CPU in
tests/test_mg_host.py): the V-cycle entry by entry, its symmetry and
definiteness, the PCG solve against the oracle's direct solve and against
the Jacobi solve, the launch counts, repeatability, graph capture and the
refusals.

The shapes are 4 x 4 quadrilaterals at p = 4, 3 x 3 at p = 6, 2 x 2 at p = 7,
3 x 3 at p = 1 (a single level) and 2 x 2 x 2 hexahedra at p = 4, warp 0.05,
Dirichlet on two sides and on all sides.  The twin is fed the lambda_max the
device reports.  The bar against the twin and between solves is the
project's oracle bar, 1e-10 relative L2.  Lines that start with "ACC" are the
records of profiles/multigrid/accuracy.txt."""
import functools

import numpy as np
import pytest

from conftest import rel_l2

import mg_twin as mt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = [(name, sides) for name, _, _, _ in mt.SHAPES for sides in mt.SIDES]


@pytest.fixture(scope="module")
def sem():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import spectralelementmethod_amd
    return spectralelementmethod_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def setup(name, sides):
    """(operator, PMultigrid, twin with the device's lambda_max, mask) of a
    case: built once, shared among the tests, left unchanged."""
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask = mt.problem(name, sides)
    op = SEMOperator(e2n.shape[1] - 1, e2n, nodes, device="cuda:0")
    mg = op.multigrid(mask)
    twin = mt.Twin(nodes, e2n, mask, lambda_max=mg.lambda_max)
    return op, mg, twin, mask


# --------------------------------------------------------------------------- the cycle
@pytest.mark.parametrize("name,sides", CASES)
def test_vcycle_matches_the_twin(sem, name, sides):
    op, mg, twin, mask = setup(name, sides)
    assert mg.ladder == twin.ladder == mt.default_ladder(op.p)
    for lv, o, m in zip(twin.levels, mg.levels, mg.masks):
        assert np.array_equal(o.e2n.cpu().numpy().view(np.uint32), lv.e2n)
        assert np.array_equal(o.nodes.cpu().numpy(), lv.nodes)
        assert np.array_equal(m.cpu().numpy(), lv.mask)
    # the device's estimator is the twin's: same start vector, same count
    own = [mt.estimate_lambda_max(lv.K, lv.mask) for lv in twin.levels]
    assert np.allclose(mg.lambda_max, own, rtol=1e-9, atol=0), (mg.lambda_max, own)
    r = np.random.default_rng(3).standard_normal(op.ndof)       # non-zero on fixed DOFs too
    z = mg.vcycle(r)
    err = rel_l2(z, twin.M(r))
    print("ACC %s %s ladder %s: vcycle to twin %.2e" % (name, sides, mg.ladder, err))
    assert err <= TOL, err
    assert not z[mask].any()


@pytest.mark.parametrize("name,sides", CASES)
def test_cycle_is_symmetric_positive_definite_on_the_device(sem, name, sides):
    op, mg, _, mask = setup(name, sides)
    rng = np.random.default_rng(7)
    for _ in range(3):
        a, b = rng.standard_normal(op.ndof) * ~mask, rng.standard_normal(op.ndof) * ~mask
        Ma, Mb = mg.vcycle(a), mg.vcycle(b)
        gap = abs(a @ Mb - b @ Ma) / abs(a @ Mb)
        print("ACC %s %s: |<a, M b> - <b, M a>| / |<a, M b>| = %.2e" % (name, sides, gap))
        assert gap <= 1e-12, gap
        assert a @ Ma > 0 and b @ Mb > 0


# --------------------------------------------------------------------------- the solve
@pytest.mark.parametrize("name,sides", CASES)
def test_pcg_solve_with_pmg(sem, name, sides):
    op, mg, twin, mask = setup(name, sides)
    K = twin.levels[0].K
    rhs, x0 = mt.solve_data(mask)
    ref = mt.sem_oracle.poisson_solve_direct(K, rhs, mask, x0)
    x, its, rel = op.pcg_solve(dev(rhs), dev(x0), mask, rtol=1e-12, precond="pmg")
    xj, its_j, _ = op.pcg_solve(dev(rhs), dev(x0), mask, rtol=1e-12)
    _, its_twin = mt.pcg(K, twin.M, rhs, x0, mask, 1e-12)
    e_ref, e_jac = rel_l2(x.cpu().numpy(), ref), rel_l2(x.cpu().numpy(), xj.cpu().numpy())
    print("ACC %s %s: pMG-PCG %d iterations (twin %d, Jacobi %d), to the direct solve %.2e, "
          "to Jacobi-PCG %.2e, relres %.1e" % (name, sides, its, its_twin, its_j, e_ref, e_jac, rel))
    assert e_ref <= TOL and e_jac <= TOL, (e_ref, e_jac)
    assert np.array_equal(x.cpu().numpy()[mask], x0[mask])
    assert abs(its - its_twin) <= 1 and its < its_j, (its, its_twin, its_j)
    assert rel <= 1e-12
    # a PMultigrid of this operator and mask is accepted as well (another
    # hierarchy: its diagonals are atomic sums, so not the same bits)
    x2, its2, _ = op.pcg_solve(dev(rhs), dev(x0), mask, rtol=1e-12, precond=mg)
    assert abs(its2 - its) <= 1 and rel_l2(x2.cpu().numpy(), x.cpu().numpy()) <= TOL


def test_dofmanager_solve_poisson_passes_the_preconditioner_through(sem):
    from spectralelementmethod_amd.basis_functions import gll_basis_2d
    from spectralelementmethod_amd.discrete import DOFManagerSC, Mesh
    nodes, e2n, _ = mt.problem("quad4x4_p4", "two")
    # the manager renumbers the nodes (exterior first, RCM)
    dm = DOFManagerSC(Mesh.from_arrays(nodes, e2n.astype(np.uint32)), 1, gll_basis_2d(4))
    nodes, e2n = dm.mesh.nodes, dm.mesh.element_map()
    mask = mt.dirichlet_mask(nodes, "two")
    rhs, x0 = mt.solve_data(mask)
    ref = mt.sem_oracle.poisson_solve_direct(mt.assemble(nodes, e2n), rhs, mask, x0)
    u, its, _ = dm.solve_poisson(rhs, x0.copy(), mask, rtol=1e-12, precond="pmg")
    uj, its_j, _ = dm.solve_poisson(rhs, x0.copy(), mask, rtol=1e-12)
    print("ACC DOFManagerSC quad4x4_p4 two (its own numbering): pMG %d, Jacobi %d iterations, to the "
          "direct solve %.2e" % (its, its_j, rel_l2(u, ref)))
    assert rel_l2(u, ref) <= TOL and rel_l2(u, uj) <= TOL and its < its_j


# --------------------------------------------------------------------------- structure
@pytest.mark.parametrize("k,kc", [(2, 8), (1, 1), (3, 5)])
def test_info_reports_the_actions_per_level(sem, k, kc):
    op, _, _, mask = setup("quad4x4_p4", "two")
    mg = op.multigrid(mask, smooth_degree=k, coarse_degree=kc)
    mg.vcycle(torch.ones(op.ndof, dtype=torch.float64, device="cuda"))
    info = mg.info()
    assert [lv["p"] for lv in info["levels"]] == [4, 2, 1]
    assert [lv["ndof"] for lv in info["levels"]] == [o.ndof for o in mg.levels]
    for lv in info["levels"][:-1]:
        assert lv["actions"] == lv["actions_run"] == 2 * k
        assert lv["passes"] == lv["passes_run"] == 2 * k + 2
    last = info["levels"][-1]
    assert last["actions"] == last["actions_run"] == kc - 1
    assert last["passes"] == last["passes_run"] == kc
    mg.close()


def test_two_solves_are_bitwise_equal(sem):
    op, mg, _, mask = setup("quad3x3_p6", "two")
    rhs, x0 = mt.solve_data(mask)
    a = mg.solve(dev(rhs), dev(x0), rtol=1e-12)
    b = mg.solve(dev(rhs), dev(x0), rtol=1e-12)
    assert a[1] == b[1] and a[2] == b[2] and torch.equal(a[0], b[0])


@pytest.mark.parametrize("name", ["quad3x3_p6", "hex2x2x2_p4"])
def test_captured_vcycle_replays_bitwise(sem, name):
    op, mg, _, mask = setup(name, "all")
    rng = np.random.default_rng(5)
    r = dev(rng.standard_normal(op.ndof))
    eager = mg.vcycle(r).clone()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mg.vcycle(r, out=out, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mg.vcycle(r, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    r2 = dev(rng.standard_normal(op.ndof))
    want = mg.vcycle(r2).clone()
    r.copy_(r2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_rtol_zero_runs_exactly_max_iter_iterations(sem):
    op, mg, _, mask = setup("quad4x4_p4", "all")
    rhs, x0 = mt.solve_data(mask)
    for n_it, check in ((3, 1), (5, 4), (0, 1)):
        _, its, rel = mg.solve(dev(rhs), dev(x0), rtol=0.0, max_iter=n_it, check_every=check)
        assert its == n_it and (rel < 1.0 or n_it == 0)
    with pytest.raises(ValueError, match="did not converge"):
        mg.solve(dev(rhs), dev(x0), rtol=1e-12, max_iter=2)


@pytest.mark.parametrize("sides", mt.SIDES)
def test_single_level_p1(sem, sides):
    op, mg, twin, mask = setup("quad3x3_p1", sides)
    assert mg.ladder == [1] and len(mg.levels) == 1 and mg.transfers == []
    assert mg.levels[0] is op
    info = mg.info()["levels"]
    assert len(info) == 1 and info[0]["actions"] == 7
    r = np.random.default_rng(4).standard_normal(op.ndof)
    assert rel_l2(mg.vcycle(r), twin.M(r)) <= TOL
    rhs, x0 = mt.solve_data(mask)
    x, its, _ = mg.solve(dev(rhs), dev(x0), rtol=1e-12)
    ref = mt.sem_oracle.poisson_solve_direct(twin.levels[0].K, rhs, mask, x0)
    assert rel_l2(x.cpu().numpy(), ref) <= TOL


def test_a_callers_ladder(sem):
    op, _, _, mask = setup("quad3x3_p6", "two")
    nodes, e2n, _ = mt.problem("quad3x3_p6", "two")
    mg = op.multigrid(mask, ladder=[6, 2, 1])
    twin = mt.Twin(nodes, e2n, mask, ladder=[6, 2, 1], lambda_max=mg.lambda_max)
    r = np.random.default_rng(6).standard_normal(op.ndof)
    err = rel_l2(mg.vcycle(r), twin.M(r))
    print("ACC quad3x3_p6 two ladder [6, 2, 1]: vcycle to twin %.2e" % err)
    assert err <= TOL
    mg.close()


# --------------------------------------------------------------------------- refusals
def test_other_kinds_are_not_implemented(sem):
    op, mg, _, mask = setup("quad4x4_p4", "two")
    from spectralelementmethod_amd.multigrid import PMultigrid
    x = torch.zeros(op.ndof, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError):
        op.pcg_solve(x, x.clone(), mask, kind="axisym_stokes", precond="pmg")
    with pytest.raises(NotImplementedError):
        PMultigrid(op, mask, kind="axisym_ns")


def test_two_dofs_per_node_are_not_implemented(sem):
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask = mt.problem("quad4x4_p4", "two")
    op = SEMOperator(4, e2n, nodes, dofs_per_node=2, device="cuda:0")
    with pytest.raises(NotImplementedError, match="dofs_per_node"):
        op.multigrid(np.repeat(mask, 2))


def test_node_states_are_not_implemented(sem):
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask = mt.problem("quad4x4_p4", "two")
    op = SEMOperator(4, e2n, nodes, device="cuda:0",
                     node_state=np.zeros(nodes.shape[1], dtype=np.uint8))
    with pytest.raises(NotImplementedError, match="node states"):
        op.multigrid(mask)


def test_user_geometry_is_not_implemented(sem):
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask = mt.problem("quad4x4_p4", "two")
    op = SEMOperator(4, e2n, nodes, device="cuda:0", geometry="stored")
    op.set_geometry(torch.ones(op.n_elem, 3, 5, 5, dtype=torch.float64))
    x = torch.zeros(op.ndof, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="set_geometry"):
        op.pcg_solve(x, x.clone(), mask, precond="pmg")


def test_reference_geometry_is_not_implemented(sem):
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask = mt.problem("quad4x4_p4", "two")
    op = SEMOperator(4, e2n, nodes, device="cuda:0", geometry="reference")
    with pytest.raises(NotImplementedError, match="geometry"):
        op.multigrid(mask)


def test_forced_renumbering_is_not_implemented(sem):
    op, mg, _, mask = setup("quad4x4_p4", "two")
    x = torch.zeros(op.ndof, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="renumber"):
        op.pcg_solve(x, x.clone(), mask, precond="pmg", renumber=True)
    with pytest.raises(ValueError, match="precond"):
        op.pcg_solve(x, x.clone(), mask, precond="ilu")


def test_a_closed_hierarchy_raises(sem):
    op, _, _, mask = setup("quad4x4_p4", "all")
    mg = op.multigrid(mask)
    mg.close()
    x = torch.zeros(op.ndof, dtype=torch.float64, device="cuda")
    for call in (lambda: mg.vcycle(x), lambda: mg.solve(x, x.clone()), mg.info,
                 lambda: op.pcg_solve(x, x.clone(), mask, precond=mg)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    mg.close()                                   # twice is fine
    assert op.apply(x) is not None               # level 0 is the caller's and lives on


def test_a_non_divisor_ladder_and_a_wrong_mask_raise_value_error(sem):
    op, mg, _, mask = setup("quad3x3_p6", "two")
    for ladder in ([6, 4, 1], [6, 3, 2], [3, 1], [6, 6], []):
        with pytest.raises(ValueError):
            op.multigrid(mask, ladder=ladder)
    with pytest.raises(ValueError, match="mask"):
        op.multigrid(mask[:-1])
    x = torch.zeros(op.ndof, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="mask"):
        op.pcg_solve(x, x.clone(), mask[:-1], precond="pmg")
    other = mask.copy()
    other[-1] = ~other[-1]
    with pytest.raises(ValueError, match="another operator or mask"):
        op.pcg_solve(x, x.clone(), other, precond=mg)
    for bad in (dict(smooth_degree=0), dict(coarse_degree=0), dict(smooth_ratio=1.0),
                dict(coarse_ratio=0.5)):
        with pytest.raises(ValueError):
            op.multigrid(mask, **bad)
