"""Root finding (mirror of sem/rootfind.py): the Newton-Raphson iteration
``Mapping.inv`` runs on the host for one point in one element.  The batched
device form is ``sem_points_locate`` / ``sem_points_invert``
(csrc/sem_points_launch.hip)."""
import numpy as np


class SolverFailure(Exception):
    """A non-linear solver did not find a 'good' solution
    (sem/rootfind.py:15-19)."""


def newton(f, x0, jac, it_max, tol):
    """Newton-Raphson for a vector-valued function (sem/rootfind.py:22-53):
    at most ``it_max`` steps x += solve(jac(x), -f(x)), returning x once
    ||dx||_2 <= tol; SolverFailure when the cap is reached."""
    x = np.array(x0, dtype=np.float64)
    for _ in range(it_max):
        dx = np.linalg.solve(jac(x), -f(x))
        x += dx
        if np.isclose(np.linalg.norm(dx), 0.0, atol=tol):
            return x
    raise SolverFailure("Maximum number of iterations exceeded before tolerence could be met.")
