"""Element mappings (mirror of sem/mapping.py: ``Mapping`` :79-181).

In the reference each ``Mapping`` computes x_phys, J, J^-1 and detJ for one
cell on the host when it is constructed (sem/mapping.py:86-119).  Here the
fields of ALL cells come from one device launch (``sem_geom_fields``,
k_geometry in csrc/sem_kernels.h) and a ``Mapping`` is a view of cell i.

``Mapping.inv`` is the reference's one-element, one-point Newton inverse
(sem/mapping.py:146-178) in NumPy on the x_phys view the Mapping holds: no
device is needed.  Locating many points over the whole mesh is the device
path of ``points.PointLocator``.

Out of scope: face ``SubMapping``s (boundary-condition
surface terms); they raise NotImplementedError.
"""
import numpy as np

from . import rootfind


class OutsideDomain(Exception):
    """Physical point outside an element (sem/mapping.py:12-16)."""


class Mapping(object):
    def __init__(self, basis, fields, index, compute_flags):
        self._basis = basis
        self._fields = fields
        self._i = index
        self._cmpflags = dict(compute_flags)

    @property
    def ndim(self):
        return self._basis.ndim

    def _get(self, key, flag):
        if not self._cmpflags.get(flag, False):
            raise AttributeError("'%s' was not requested (compute flag %r)" % (key, flag))
        return self._fields[key][self._i]

    @property
    def x_phys(self):
        return self._get("x_phys", "x_phys")

    @property
    def J(self):
        return self._get("J", "Jacobian")

    @property
    def invJ(self):
        return self._get("invJ", "Jacobian")

    @property
    def detJ(self):
        return self._get("detJ", "Jacobian")

    def __call__(self, x_param):
        """Parametric -> physical coordinates (sem/mapping.py:138-141)."""
        return np.moveaxis(self._basis.interpolate(self.x_phys, x_param), -1, 0)

    def _nodal_jacobian(self):
        """J[c][d] = d x_c / d xi_d at the nodes, [ndim, ndim] + coeff_shape:
        the 1-D differentiation matrices applied to x_phys on the host (the
        reference's ``J`` field, sem/mapping.py:113)."""
        x = np.asarray(self.x_phys, dtype=np.float64)
        nd = self.ndim
        mats = self._basis.get_D1_matrices()
        J = np.empty((nd, nd) + x.shape[1:])
        for d in range(nd):
            J[:, d] = np.moveaxis(np.tensordot(x, mats[d], axes=([1 + d], [1])), -1, 1 + d)
        return J

    def inv(self, x_phys, x_param_guess=None):
        """Physical -> parametric coordinates of one point in this element
        (sem/mapping.py:146-178): Newton from ``x_param_guess`` (default 0),
        at most 8 iterations, tolerance 1e-8 on ||dx||_2, the Jacobian
        interpolated from its nodal values.  Raises ``OutsideDomain`` when the
        converged point is not in [-1, 1]^d (strict, as the reference) and
        ``rootfind.SolverFailure`` when Newton does not converge."""
        x_phys = np.array(x_phys, dtype=np.float64).reshape(self.ndim)
        if x_param_guess is None:
            x_param_guess = np.zeros_like(x_phys)
        J = self._nodal_jacobian()

        def delta_x_phys(x_param):
            return np.asarray(self(x_param)).reshape(self.ndim) - x_phys

        def eval_jacobian(x_param):
            return np.asarray(self._basis.interpolate(J, x_param)).reshape(self.ndim, self.ndim)

        x_param = rootfind.newton(delta_x_phys, x_param_guess, eval_jacobian, it_max=8, tol=1e-8)
        if (x_param >= -1.).all() and (x_param <= 1.).all():
            return x_param
        raise OutsideDomain("Given physical point is not in the parametric domain of the "
                            "finite element.")

    def get_submapping(self, face):
        raise NotImplementedError("face sub-mappings (sem/mapping.py:184-272) are out of scope")
