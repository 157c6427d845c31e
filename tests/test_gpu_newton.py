"""The Newton driver of examples/axisym_newton.py on ``annulus(3, 2, 4)`` at
Re = 5 with psi = rho^2 (0.5 + 0.1 z), omega = rho (0.3 cos(0.5 z) + 0.05 rho)
on the mesh boundary, and examples/poisson.py restated on local_systems.

The case was checked on the CPU with the NumPy oracle and a dense Newton
before the bars were set: 6 iterations, free-DOF residual 338 -> 7e-14 (154
free DOFs of 234), Jacobian condition number 1.6e2.  A condensed solve loses
a few digits against a dense one: that is the margin between 2e-16 and the
1e-10 bar.  p = 4 keeps the interior blocks small (18 interior DOFs per
element): static condensation at large element sizes is not this file's
subject."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def example(name):
    spec = importlib.util.spec_from_file_location(name + "_example",
                                                  os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ex():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return example("axisym_newton")


@pytest.fixture(scope="module")
def newton(ex):
    """The Re = 5 case solved once: (flow, iterations, residual before, after)."""
    flow = ex.AxisymFlow(ex.annulus_mesh(4, 3, 2), 4, 5.0)
    r0 = flow.residual_norm()
    its = flow.solve(it_max=8, tol=1e-9, verbose=False)
    return flow, its, r0, flow.residual_norm()


def test_newton_converges(newton):
    flow, its, _, _ = newton
    print("||d omega|| per iteration: " + " ".join("%.3e" % d for d in flow.du_norms))
    assert int((~flow.on_ebc).sum()) == 154 and flow.dm.ndof == 234
    assert its <= 8
    assert flow.du_norms[-1] <= 1e-9
    assert np.all(np.isfinite(flow.soln_vec))


def test_matrix_free_residual_vanishes(newton):
    """The residual kernel shares no code with the matrix kernel."""
    _, _, r0, r1 = newton
    print("matrix-free residual on the free DOFs: %.6e -> %.6e (%.2e of the start)"
          % (r0, r1, r1 / r0))
    assert r0 > 1.0
    assert r1 <= 1e-10 * r0


def test_reynolds_zero_is_the_stokes_solve(ex):
    """With Re set to 0 the driver meets the AXISYM_STOKES system solved in
    one step.  Both are condensed solves of the same linear system (condition
    number 1.6e2): they agree to the 1e-10 the residual bar allows."""
    ns = ex.AxisymFlow(ex.annulus_mesh(4, 3, 2), 4, 0.0)
    its = ns.solve(it_max=8, tol=1e-9, verbose=False)
    st = ex.AxisymFlow(ex.annulus_mesh(4, 3, 2), 4, 0.0)
    u = st.solve_stokes()
    err = np.linalg.norm(ns.soln_vec - u) / np.linalg.norm(u)
    print("Re = 0: %d iterations (||d omega|| %s); to the one-step Stokes solve %.2e"
          % (its, " ".join("%.2e" % d for d in ns.du_norms), err))
    assert its <= 2          # a linear problem: the second update is rounding
    assert err <= 1e-10
    assert ns.residual_norm() <= 1e-10 * ns.residual_norm(np.where(ns.on_ebc, u, 0.0))


def test_diverging_iteration_raises(ex):
    """max_n_diverge increases of ||d omega|| end the iteration."""
    flow = ex.AxisymFlow(ex.annulus_mesh(4, 3, 2), 4, 5.0)
    norms = iter([1.0, 2.0, 3.0, 4.0, 5.0])
    flow.newton_step = lambda: np.full(flow.dm.ndof, next(norms) / np.sqrt(flow.dm.ndof // 2))
    with pytest.raises(ex.SolverFailure):
        flow.solve(it_max=10, max_n_diverge=3, verbose=False)
    assert len(flow.du_norms) == 4    # 2, 3, 4 grew
    flow.newton_step = lambda: np.ones(flow.dm.ndof)
    with pytest.raises(ex.SolverFailure):
        flow.solve(it_max=3, verbose=False)  # never below the tolerance


def test_poisson_example_on_local_systems():
    """examples/poisson.py: the method on device-built local systems gives
    the solution of the einsum method on the p = 4, 8 x 8 default."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    px = example("poisson")
    plate = px.PoissonPlate(px.square_mesh(4, 8, 8), 4)
    u = plate.run().copy()
    u_dev = plate.solve_device_systems()
    err = np.linalg.norm(u_dev - u) / np.linalg.norm(u)
    print("device-built local systems to the einsum method: %.2e" % err)
    assert err <= 1e-12
    assert np.array_equal(plate.soln_vec, u)
