"""Point location and field evaluation at arbitrary physical points on the GPU.

The reference reads a field back one point at a time:
``DOFManager.find_elem_containing_point`` sorts every cell centroid per query
and runs ``Mapping.inv`` (a Newton iteration of Python barycentric
evaluations) in each cell until one accepts the point
(sem/discrete.py:263-280, sem/mapping.py:146-178), and
``DOFManager.interpolate`` evaluates the element's interpolant there
(sem/discrete.py:221-233).  Here all points go through batched kernels of
libsem_hip.so (include/sem_hip.h "Points", csrc/sem_points*.hip):

* ``PointLocator(op)`` owns a ``sem_points`` built from the operator's
  x_phys (uniform grid of element boxes; nothing but the boxes leaves the
  device);
* ``PointLocator.locate(x)`` returns a ``PointSet``: element id and
  parametric coordinates of every point (``elem == -1`` / NaN outside);
* ``PointSet.evaluate(u)`` interpolates global coefficient vectors at the
  points, ``PointSet.physical()`` maps them back to physical space.

Deviations from the reference: a Newton failure in one
candidate element skips that element instead of raising; a point is accepted
within ``|xi| <= 1 + 1e-10`` and clamped; points outside the mesh are
reported, not raised, by the batched calls.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _as_points(x, ndim, device):
    """float64 device tensor [ndim, M] from host or device points; also
    whether the caller passed host data."""
    is_np = not isinstance(x, torch.Tensor)
    t = torch.as_tensor(np.asarray(x, dtype=np.float64)) if is_np else x
    if t.dtype != torch.float64:
        raise TypeError("points must be float64")
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2 or t.shape[0] != ndim:
        raise ValueError("points must have shape [%d, M]" % ndim)
    return t.to(device).contiguous(), is_np


class PointLocator(object):
    """Locates physical points in the elements of one mesh on one GPU.

    Parameters
    ----------
    op : SEMOperator, optional
        x_phys comes from its ``geometry_fields()``, the element map from
        ``op.e2n``.
    x_phys, e2n : optional
        Raw arrays instead of an operator: x_phys float64 [E, ndim, n, n(, n)]
        (the layout ``sem_geom_fields`` writes) and the uint32 element map
        [E, n, n(, n)]; quadrilaterals and hexahedra, 1 <= p <= 16.
    device : optional
        Device of the raw arrays (default: the operator's / current device).
    """

    def __init__(self, op=None, x_phys=None, e2n=None, device=None):
        self._lib = _lib.load()
        self._pts = None
        if op is not None:
            device = op.device
            x_phys = op.geometry_fields()["x_phys"]
            e2n = op.e2n
        elif x_phys is None or e2n is None:
            raise ValueError("PointLocator needs an operator or x_phys and e2n")
        from .operators import SEMOperator, _device_index
        self.device = torch.device("cuda", _device_index(device))
        x_phys = torch.as_tensor(x_phys, dtype=torch.float64).to(self.device).contiguous()
        e2n = SEMOperator._to_map(e2n).to(self.device).contiguous()
        self.ndim = x_phys.dim() - 2
        if self.ndim not in (2, 3) or x_phys.shape[1] != self.ndim:
            raise ValueError("x_phys must have shape [E, ndim, n, n] or [E, ndim, n, n, n]")
        self.n = int(x_phys.shape[2])
        self.p = self.n - 1
        self.n_elem = int(x_phys.shape[0])
        if tuple(x_phys.shape[2:]) != (self.n,) * self.ndim or \
                tuple(e2n.shape) != (self.n_elem,) + (self.n,) * self.ndim:
            raise ValueError("x_phys [E, ndim] + [n] * ndim and e2n [E] + [n] * ndim expected")
        self.x_phys = x_phys  # borrowed by the library: kept alive here
        self.e2n = e2n
        # the node count every evaluated field must have: the kernel indexes
        # u with this map and checks nothing
        # (e2n holds uint32 entries viewed as int32)
        self.n_node = int(op.n_node) if op is not None else \
            int((e2n.to(torch.int64) & 0xFFFFFFFF).max().item()) + 1
        pts = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_points_create(C.byref(pts), self.ndim, self.p, self.n_elem,
                                                   _lib.tptr(x_phys), self.device.index,
                                                   _lib.stream_ptr()))
        self._pts = pts

    def close(self):
        if getattr(self, "_pts", None):
            self._lib.sem_points_destroy(self._pts)
            self._pts = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """Setup of the candidate grid (include/sem_hip.h sem_points_info)."""
        v = (C.c_int64 * 12)()
        _lib.check(self._lib.sem_points_info(self._pts, v, 12))
        v = list(v)
        return dict(ndim=v[0], p=v[1], n_elem=v[2], grid=tuple(v[3:3 + v[0]]), cells=v[6],
                    entries=v[7], max_candidates=v[8], last_found=v[9], last_outside=v[10],
                    newton_itmax=v[11])

    def locate(self, x, stream=None):
        """Element and parametric coordinates of the points x [ndim, M] (host
        or device) as a ``PointSet``."""
        xq, _ = _as_points(x, self.ndim, self.device)
        m = int(xq.shape[1])
        elem = torch.empty(m, dtype=torch.int32, device=self.device)
        xi = torch.empty(self.ndim, m, dtype=torch.float64, device=self.device)
        n_out = C.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_points_locate(self._pts, m, _lib.tptr(xq), _lib.tptr(elem),
                                                   _lib.tptr(xi), C.byref(n_out),
                                                   _lib.stream_ptr(stream)))
        return PointSet(self, elem, xi, n_outside=int(n_out.value))

    def invert(self, x, elem, guess=None, stream=None):
        """``Mapping.inv`` for many points in caller-given elements: returns
        (xi [ndim, M], status uint8 [M]: 0 inside, 1 converged outside the
        element, 2 failed or bad element id)."""
        xq, _ = _as_points(x, self.ndim, self.device)
        m = int(xq.shape[1])
        elem = torch.as_tensor(elem).to(self.device).to(torch.int32).contiguous()
        if elem.shape != (m,):
            raise ValueError("one element id per point expected")
        g = None if guess is None else _as_points(guess, self.ndim, self.device)[0]
        if g is not None and g.shape != xq.shape:
            raise ValueError("guess must have the shape of the points")
        xi = torch.empty_like(xq)
        status = torch.empty(m, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_points_invert(self._pts, m, _lib.tptr(xq), _lib.tptr(elem),
                                                   _lib.tptr(g), _lib.tptr(xi), _lib.tptr(status),
                                                   _lib.stream_ptr(stream)))
        return xi, status

    def point_set(self, elem, xi):
        """A ``PointSet`` from caller-given element ids [M] and parametric
        coordinates [ndim, M]; ids outside [0, n_elem) evaluate to NaN."""
        elem = torch.as_tensor(elem).to(self.device).to(torch.int32).contiguous()
        xi, _ = _as_points(xi, self.ndim, self.device)
        if elem.shape != (xi.shape[1],):
            raise ValueError("one element id per point expected")
        bad = (elem < 0) | (elem >= self.n_elem)
        return PointSet(self, elem, xi, n_outside=int(bad.sum().item()))


class PointSet(object):
    """Located points: ``elem`` int32 [M] (-1 outside the mesh), ``xi``
    float64 [ndim, M] (NaN outside), ``found`` bool [M], ``n_outside``."""

    def __init__(self, locator, elem, xi, n_outside):
        self.locator = locator
        self.elem = elem
        self.xi = xi
        self.n_outside = n_outside
        self._plan = None

    def __len__(self):
        return int(self.elem.shape[0])

    @property
    def found(self):
        return (self.elem >= 0) & (self.elem < self.locator.n_elem)

    def _get_plan(self, stream=None):
        if self.locator._pts is None:
            raise RuntimeError("the PointLocator of this PointSet was closed")
        if self._plan is None:
            loc = self.locator
            plan = C.c_void_p()
            with torch.cuda.device(loc.device):
                _lib.check(loc._lib.sem_points_plan(loc._pts, len(self), _lib.tptr(self.elem),
                                                    C.byref(plan), _lib.stream_ptr(stream)))
            self._plan = plan
        return self._plan

    def plan_info(self):
        """Evaluation plan (include/sem_hip.h sem_points_plan_info)."""
        v = (C.c_int64 * 6)()
        _lib.check(self.locator._lib.sem_points_plan_info(self._get_plan(), v, 6))
        return dict(points=v[0], in_runs=v[1], items=v[2], touched_elements=v[3], width=v[4],
                    items_per_workgroup=v[5])

    def close(self):
        if getattr(self, "_plan", None):
            self.locator._lib.sem_points_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, u, out=None, stream=None, dofs_per_node=None):
        """Interpolate global coefficients at the points.

        u : [n_node] -> [M]; [..., n_node] (component-major) -> [..., M];
        with ``dofs_per_node=dpn`` the interleaved [dpn * n_node] DOF vector
        (DOF = dpn * node + comp) -> [dpn, M].  n_node is the locator's
        (``PointLocator.n_node``); a u of any other size raises ValueError,
        since the kernel indexes it with the mesh's map.  Host arrays come back as host
        arrays.  Points outside the mesh evaluate to NaN.  ``out`` (device,
        contiguous, the result's shape) and ``stream`` make the call
        allocation-free: it can be captured in a graph once the plan exists
        (first call, or ``plan_info()``)."""
        loc = self.locator
        is_np = not isinstance(u, torch.Tensor)
        ut = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64)) if is_np else u
        if ut.dtype != torch.float64:
            raise TypeError("u must be float64")
        ut = ut.to(loc.device)
        if not ut.is_contiguous():
            ut = ut.contiguous()
        m = len(self)
        if dofs_per_node is not None:
            dpn = int(dofs_per_node)
            if ut.dim() != 1 or dpn < 1 or ut.numel() != dpn * loc.n_node:
                raise ValueError("interleaved u must be 1-D with dofs_per_node * n_node = "
                                 "%d * %d entries, got shape %s"
                                 % (dpn, loc.n_node, list(ut.shape)))
            ncomp, cs, ns, shape = dpn, 1, dpn, (dpn, m)
        else:
            # the kernel indexes u with the mesh's own map: a field of another
            # mesh, order or layout must not reach it
            if ut.dim() < 1 or int(ut.shape[-1]) != loc.n_node:
                raise ValueError("u must have shape [..., n_node = %d], got %s (an interleaved "
                                 "DOF vector needs dofs_per_node=)"
                                 % (loc.n_node, list(ut.shape)))
            nn = loc.n_node
            ncomp = int(ut.numel() // nn)
            if ncomp < 1:
                raise ValueError("u has an empty component axis: %s" % list(ut.shape))
            cs, ns, shape = nn, 1, tuple(ut.shape[:-1]) + (m,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=loc.device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float64
                  and out.device == loc.device and out.is_contiguous()
                  and tuple(out.shape) == shape):
            raise TypeError("out must be a contiguous float64 tensor of shape %s on %s"
                            % (list(shape), loc.device))
        plan = self._get_plan(stream)
        with torch.cuda.device(loc.device):
            _lib.check(loc._lib.sem_points_eval(plan, _lib.tptr(loc.e2n), _lib.tptr(self.xi),
                                                ncomp, cs, ns, _lib.tptr(ut), _lib.tptr(out),
                                                _lib.stream_ptr(stream)))
        return out.cpu().numpy() if is_np else out

    def physical(self, stream=None):
        """x(xi) of the points in their elements [ndim, M] (NaN outside): the
        round trip of ``locate``."""
        loc = self.locator
        if loc._pts is None:
            raise RuntimeError("the PointLocator of this PointSet was closed")
        x = torch.empty_like(self.xi)
        with torch.cuda.device(loc.device):
            _lib.check(loc._lib.sem_points_map(loc._pts, len(self), _lib.tptr(self.elem),
                                               _lib.tptr(self.xi), _lib.tptr(x),
                                               _lib.stream_ptr(stream)))
        return x
