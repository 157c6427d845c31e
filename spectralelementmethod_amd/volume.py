"""Volume fields on the GPU: gradients, recovery, integrals, norms.

The reference post-processes a solution one element at a time in NumPy:
``FiniteElement.gradient`` / ``deriv`` / ``integrate``
(sem/discrete.py:674-689).  ``VolumeSet`` does it for all elements of a mesh
with the kernels of libsem_hip.so (include/sem_hip.h "Volume",
csrc/sem_volume.hip), on quadrilaterals and hexahedra at p = 1..16:

* ``gradient(u)``: the physical gradient of global coefficient vectors on
  every element, [..., E, ndim, n, n(, n)];
* ``recover(u)``: the continuous nodal gradient [..., ndim, n_node], the
  lumped-mass L2 projection of the element gradients;
* ``integrate(u)`` / ``integrate_local(vals)``: volume integrals of nodal
  fields and of element-local values;
* ``norms(u, v=None)``: the GLL-quadrature L2 norm and H1 seminorm of u - v;
* ``mass``: the lumped mass, the assembled detJxW.

No per-node J / invJ is stored: the kernels recompute the geometry from
x_phys.  Every sum is taken in a fixed order without atomics: two calls give
the same bits.  Axisymmetric weights, divergence / curl, the ranks of a
decomposition and non-isoparametric mappings are out of scope.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

Norms = collections.namedtuple("Norms", "l2 h1 l2_sq h1_sq")


class VolumeSet(object):
    """All elements of one mesh on one GPU.

    Parameters
    ----------
    op : SEMOperator, optional
        x_phys comes from its ``geometry_fields()``, the map from ``op.e2n``,
        D and the quadrature weights from its basis.
    x_phys, e2n, n_node : optional
        Raw arrays instead of an operator: x_phys float64 [E, ndim] + [n] *
        ndim as ``sem_geom_fields`` writes it, the uint32 element map and the
        node count (default: the largest id + 1).  An id >= n_node raises
        ValueError, a node with detJ <= 0 AssertionError, before any field
        is touched.
    """

    def __init__(self, op=None, x_phys=None, e2n=None, n_node=None, device=None):
        self._lib = _lib.load()
        self._h = None
        from .operators import SEMOperator, _basis_arrays, _device_index
        D = w = None
        if op is not None:
            device = op.device
            if x_phys is None:
                x_phys = op.geometry_fields()["x_phys"]
            e2n = op.e2n
            n_node = op.n_node
            D, w = op.D, op.w
        elif x_phys is None or e2n is None:
            raise ValueError("VolumeSet needs an operator or x_phys and e2n")
        self.device = torch.device("cuda", _device_index(device))
        # the library borrows both until destroy: they live here
        self.x_phys = torch.as_tensor(x_phys, dtype=torch.float64).to(self.device).contiguous()
        self.e2n = SEMOperator._to_map(e2n).to(self.device).contiguous()
        self.ndim = self.x_phys.dim() - 2
        if self.ndim not in (2, 3) or self.x_phys.shape[1] != self.ndim:
            raise ValueError("x_phys must have shape [E, ndim, n, n] or [E, ndim, n, n, n]")
        self.n = int(self.x_phys.shape[2])
        self.p = self.n - 1
        self.n_elem = int(self.x_phys.shape[0])
        self.eshape = (self.n,) * self.ndim
        if tuple(self.x_phys.shape[2:]) != self.eshape or \
                tuple(self.e2n.shape) != (self.n_elem,) + self.eshape:
            raise ValueError("x_phys [E, ndim] + [n] * ndim and e2n [E] + [n] * ndim expected")
        if self.p > 16:
            raise NotImplementedError("volume: p <= 16")
        if D is None:
            _, D, w, _ = _basis_arrays(self.p, None, self.ndim)
        if n_node is None:
            n_node = int((self.e2n.to(torch.int64) & 0xFFFFFFFF).max().item()) + 1 \
                if self.n_elem else 0
        self.n_node = int(n_node)
        D = np.ascontiguousarray(D, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_volume_create(
                C.byref(h), self.ndim, self.p, self.n_elem, _lib.tptr(self.x_phys),
                _lib.tptr(self.e2n), self.n_node, _lib.dptr(D), _lib.dptr(w), self.device.index,
                _lib.stream_ptr()))
        self._h = h
        self._mass = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sem_volume_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n_elem

    def _handle(self):
        if self._h is None:
            raise RuntimeError("this VolumeSet was closed")
        return self._h

    def info(self):
        """include/sem_hip.h sem_volume_info."""
        v = (C.c_int64 * 7)()
        _lib.check(self._lib.sem_volume_info(self._handle(), v, 7))
        return dict(ndim=v[0], p=v[1], elements=v[2], nodes=v[3], referenced_nodes=v[4],
                    max_contributions=v[5], scratch_bytes=v[6])

    @property
    def mass(self):
        """The lumped mass [n_node]: detJxW summed into the nodes, 0 at nodes
        no element references.  A new tensor at every read: the caller may
        change it."""
        if self._mass is None:
            m = torch.zeros(self.n_node, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self._lib.sem_volume_mass(self._handle(), _lib.tptr(m),
                                                     _lib.stream_ptr()))
            self._mass = m
        return self._mass.clone()

    # ------------------------------------------------------------------ fields
    def _field(self, u, dofs_per_node, name="u"):
        """(device tensor, ncomp, comp_stride, node_stride, leading shape,
        host input?) of a global coefficient array (the conventions of
        ``FaceSet.gradient``); the kernels index it with the mesh's own map,
        so any other size is refused here."""
        is_np = not isinstance(u, torch.Tensor)
        ut = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64)) if is_np else u
        if ut.dtype != torch.float64:
            raise TypeError("%s must be float64" % name)
        ut = ut.to(self.device)
        if not ut.is_contiguous():
            ut = ut.contiguous()
        nn = self.n_node
        if dofs_per_node is not None:
            dpn = int(dofs_per_node)
            if ut.dim() != 1 or dpn < 1 or ut.numel() != dpn * nn:
                raise ValueError("interleaved %s must be 1-D with dofs_per_node * n_node = %d * %d "
                                 "entries, got shape %s" % (name, dpn, nn, list(ut.shape)))
            return ut, dpn, 1, dpn, (dpn,), is_np
        if ut.dim() < 1 or int(ut.shape[-1]) != nn:
            raise ValueError("%s must have shape [..., n_node = %d], got %s (an interleaved DOF "
                             "vector needs dofs_per_node=)" % (name, nn, list(ut.shape)))
        lead = tuple(ut.shape[:-1])
        ncomp = int(np.prod(lead, dtype=np.int64))
        if ncomp < 1:
            raise ValueError("%s has an empty component axis: %s" % (name, list(ut.shape)))
        return ut, ncomp, nn, 1, lead, is_np

    def _out(self, out, shape, name="out"):
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=self.device)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64
                and out.device == self.device and out.is_contiguous()
                and tuple(out.shape) == tuple(shape)):
            raise ValueError("%s must be a contiguous float64 tensor of shape %s on %s"
                             % (name, list(shape), self.device))
        return out

    def gradient(self, u, out=None, stream=None, dofs_per_node=None):
        """``FiniteElement.gradient`` of every element: u [..., n_node] ->
        [..., E, ndim, n, n(, n)]; with ``dofs_per_node=dpn`` the interleaved
        [dpn * n_node] vector -> [dpn, E, ndim, ...].  Host arrays come back
        as host arrays."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        g = self._out(out, lead + (self.n_elem, self.ndim) + self.eshape)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_volume_gradient(self._handle(), ncomp, cs, ns, _lib.tptr(ut),
                                                     _lib.tptr(g), _lib.stream_ptr(stream)))
        return g.cpu().numpy() if is_np else g

    def recover(self, u, out=None, stream=None, dofs_per_node=None):
        """The continuous nodal gradient [..., ndim, n_node] of u [...,
        n_node] ([dpn, ndim, n_node] of an interleaved vector): at every node
        the detJxW-weighted mean of the element gradients there, 0 at nodes
        no element references."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        nn = self.n_node
        g = self._out(out, lead + (self.ndim, nn))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_volume_recover(self._handle(), ncomp, cs, ns, _lib.tptr(ut),
                                                    self.ndim * nn, nn, 1, _lib.tptr(g),
                                                    _lib.stream_ptr(stream)))
        return g.cpu().numpy() if is_np else g

    def _sums(self, lead, tail, per_element, out, stream, is_np, want_per, call):
        pe = self._out(per_element, lead + (self.n_elem,) + tail, "per_element") \
            if want_per or per_element is not None else None
        tot = self._out(out, lead + tail)
        with torch.cuda.device(self.device):
            _lib.check(call(_lib.tptr(pe), _lib.tptr(tot), _lib.stream_ptr(stream)))
        if is_np:
            pe, tot = (pe.cpu().numpy() if pe is not None else None), tot.cpu().numpy()
        return pe, tot

    def integrate(self, u, return_per_element=False, out=None, per_element=None, stream=None,
                  dofs_per_node=None):
        """The volume integral of nodal fields: u [..., n_node] -> [...], and
        with ``return_per_element`` (per element [..., E], total)."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        pe, tot = self._sums(lead, (), per_element, out, stream, is_np, return_per_element,
                             lambda a, b, s: self._lib.sem_volume_integrate(
                                 self._handle(), ncomp, cs, ns, _lib.tptr(ut), a, b, s))
        return (pe, tot) if return_per_element else tot

    def integrate_local(self, vals, return_per_element=False, out=None, per_element=None,
                        stream=None):
        """``FiniteElement.integrate`` of every element, summed: vals [..., E,
        n, n(, n)] -> [...], and with ``return_per_element`` (per element
        [..., E], total)."""
        is_np = not isinstance(vals, torch.Tensor)
        v = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float64)) if is_np else vals
        if v.dtype != torch.float64:
            raise TypeError("vals must be float64")
        v = v.to(self.device).contiguous()
        tail = (self.n_elem,) + self.eshape
        k = v.dim() - len(tail)
        if k < 0 or tuple(v.shape[k:]) != tail:
            raise ValueError("vals must have shape [..., %s], got %s"
                             % (", ".join(map(str, tail)), list(v.shape)))
        lead = tuple(v.shape[:k])
        ncomp = int(np.prod(lead, dtype=np.int64))
        if ncomp < 1:
            raise ValueError("vals has an empty component axis")
        pe, tot = self._sums(lead, (), per_element, out, stream, is_np, return_per_element,
                             lambda a, b, s: self._lib.sem_volume_integrate_local(
                                 self._handle(), ncomp, _lib.tptr(v), a, b, s))
        return (pe, tot) if return_per_element else tot

    def norms(self, u, v=None, return_per_element=False, out=None, per_element=None, stream=None,
              dofs_per_node=None):
        """The discrete norms of u - v (v None: of u) with the GLL quadrature
        of the stiffness matrix: ``Norms(l2, h1, l2_sq, h1_sq)``, each [...],
        h1 the seminorm |grad (u - v)|.  The difference is formed at the
        nodes before it is differentiated.  ``out`` [..., 2] receives the
        squares; with ``return_per_element`` also the squares per element
        [..., E, 2]."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        vt = None
        if v is not None:
            vt, ncomp_v, _, _, lead_v, _ = self._field(v, dofs_per_node, "v")
            if lead_v != lead:
                raise ValueError("u and v must have the same shape")
        pe, tot = self._sums(lead, (2,), per_element, out, stream, is_np, return_per_element,
                             lambda a, b, s: self._lib.sem_volume_norms(
                                 self._handle(), ncomp, cs, ns, _lib.tptr(ut), _lib.tptr(vt), a,
                                 b, s))
        sq = np.sqrt if is_np else torch.sqrt
        res = Norms(sq(tot[..., 0]), sq(tot[..., 1]), tot[..., 0], tot[..., 1])
        return (pe, res) if return_per_element else res
