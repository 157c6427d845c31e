"""Element mappings (mirror of sem/mapping.py: ``Mapping`` :79-181).

In the reference each ``Mapping`` computes x_phys, J, J^-1 and detJ for one
cell on the host when it is constructed (sem/mapping.py:86-119).  Here the
fields of ALL cells come from one device launch (``sem_geom_fields``,
k_geometry in csrc/sem_kernels.h) and a ``Mapping`` is a view of cell i.

``Mapping.inv`` is the reference's one-element, one-point Newton inverse
(sem/mapping.py:146-178) in NumPy on the x_phys view the Mapping holds: no
device is needed.  Locating many points over the whole mesh is the device
path of ``points.PointLocator``.

``Mapping.get_submapping(face)`` returns a ``SubMapping`` (sem/mapping.py:
184-272): a view of one face of the batched ``faces.FaceSet`` the DOFManager
keeps for all faces of all cells.
"""
import numpy as np

from . import rootfind


class OutsideDomain(Exception):
    """Physical point outside an element (sem/mapping.py:12-16)."""


class Mapping(object):
    def __init__(self, basis, fields, index, compute_flags, face_source=None):
        self._basis = basis
        self._fields = fields
        self._i = index
        self._cmpflags = dict(compute_flags)
        # face -> (host arrays of a FaceSet, row) of this cell's face
        self._face_source = face_source

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
        """The mapping of one face (sem/mapping.py:180-181), a view of the
        DOFManager's batched face geometry."""
        if self._face_source is None:
            raise ValueError("this Mapping belongs to no DOFManager: no face geometry")
        face = int(face)
        if not 0 <= face < 2 * self.ndim:
            raise ValueError("face must be in [0, %d)" % (2 * self.ndim))
        fields, row = self._face_source(face)
        return SubMapping(self, face, fields, row)


class SubMapping(object):
    """One face of an element (sem/mapping.py:184-272): ``x_phys``, ``J``,
    ``invJ``, ``detJ`` of the parent at the face nodes and the scaled normal
    ``n_dS`` with ``dS`` and ``unit_normal``, in the face order of
    include/sem_hip.h "Faces".  Views of row ``row`` of a ``faces.FaceSet``'s
    host arrays; 3-D faces have the normal the reference leaves unfinished."""

    def __init__(self, parent_mapping, face, fields, row):
        self._parent_mapping = parent_mapping
        self._face = face
        self._fields = fields
        self._row = row

    @property
    def ndim(self):
        return self._parent_mapping.ndim - 1

    def _get(self, key):
        return self._fields[key][self._row]

    x_phys = property(lambda self: self._get("x_phys"))
    J = property(lambda self: self._get("J"))
    invJ = property(lambda self: self._get("invJ"))
    detJ = property(lambda self: self._get("detJ"))
    n_dS = property(lambda self: self._get("n_dS"))
    dS = property(lambda self: self._get("dS"))
    unit_normal = property(lambda self: self._get("unit_normal"))

    def inv(self, x_phys):
        raise NotImplementedError("Cannot compute the parametric coordinates of a SubMapping "
                                  "from physical coordinates.")
