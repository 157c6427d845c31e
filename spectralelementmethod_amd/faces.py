"""Boundary faces on the GPU: normals, surface integrals, Neumann loads.

The reference builds one Python object per face: ``SubMapping`` takes the
face's tangents from the parent's Jacobian and turns them into the scaled
normal ``n_dS`` (sem/mapping.py:184-272), ``SubFiniteElement`` adds the
surface quadrature ``dSxW``, ``integrate`` and the parent's gradient sliced
to the face (sem/discrete.py:708-775).  Its 3-D normal is unfinished
(``_compute_normal_vec`` drops the cross product).  Here a whole list of
(element, face) pairs goes through batched kernels of libsem_hip.so
(include/sem_hip.h "Faces", csrc/sem_faces.hip), on quadrilaterals and
hexahedra at p = 1..16:

* ``FaceSet(op, elem, face)`` (``op.face_set(elem, face)``) owns a
  ``sem_faces``: per face node the position, ``n_dS``, ``dS``, ``dSxW``,
  ``unit_normal`` and the global node id, in the reference's face order;
* ``gradient(u)`` / ``normal_derivative(u)`` of global coefficient vectors at
  the face nodes, ``integrate(vals)`` and the fused ``flux(u)`` (the integral
  of grad u . n over the faces, bitwise repeatable);
* ``assemble(vals)``: the Neumann load vector, ``out[node] += vals dSxW``,
  without atomics.

Face ids and orders are stated in include/sem_hip.h; ``face_index_table``
gives them as index arrays.  The faces of a decomposition's ranks and
non-isoparametric mappings are out of scope.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def face_index_table(ndim, n):
    """int64 [2 * ndim, nf]: element-local lexicographic index (xi0 slowest)
    of face node q of each face, nf = n^(ndim-1).  Face = 2 * axis + side.
    2-D: counter-clockwise round the element (faces 0 and 3 reversed).  3-D:
    q = q0 * n + q1 with (q0, q1) along the axes (axis+1, axis+2) mod 3 on a
    side-1 face and (axis+2, axis+1) mod 3 on a side-0 face."""
    lin = np.arange(n ** ndim, dtype=np.int64).reshape((n,) * ndim)
    rows = []
    for face in range(2 * ndim):
        ax, side = divmod(face, 2)
        fixed = n - 1 if side else 0
        if ndim == 2:
            line = np.take(lin, fixed, axis=ax)
            rows.append(line[::-1] if face in (0, 3) else line)
        else:
            sl = np.take(np.moveaxis(lin, (ax, (ax + 1) % 3, (ax + 2) % 3), (0, 1, 2)), fixed,
                         axis=0)                       # [a_(ax+1), a_(ax+2)]
            rows.append((sl if side else sl.T).ravel())
    return np.stack(rows)


def subface_slice(face, arr, ndim):
    """The trailing ``ndim`` axes of ``arr`` (an element array) restricted
    to ``face`` in face order: [..., n] in 2-D, [..., n, n] in 3-D (the
    reference's ``_subface_slice``, sem/mapping.py:19-76)."""
    arr = np.asarray(arr)
    n = arr.shape[-1]
    lead = arr.shape[:arr.ndim - ndim]
    idx = face_index_table(ndim, n)[face]
    return arr.reshape(lead + (-1,))[..., idx].reshape(lead + (n,) * (ndim - 1))


class FaceSet(object):
    """Faces of the elements of one mesh on one GPU.

    Parameters
    ----------
    op : SEMOperator, optional
        x_phys comes from its ``geometry_fields()``, the map from ``op.e2n``,
        D and the quadrature weights from its basis.
    elem, face : array-like [F]
        Element id and face id (2 * axis + side) of every face; a pair may
        repeat, F may be 0.  A bad id raises ValueError before any kernel.
    x_phys, e2n, n_node : optional
        Raw arrays instead of an operator: x_phys float64 [E, ndim] + [n] *
        ndim as ``sem_geom_fields`` writes it and the uint32 element map.
    """

    def __init__(self, op=None, elem=(), face=(), x_phys=None, e2n=None, n_node=None, device=None):
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
            raise ValueError("FaceSet needs an operator or x_phys and e2n")
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
        if self.p > 16:
            raise NotImplementedError("faces: p <= 16")
        if D is None:
            _, D, w, _ = _basis_arrays(self.p, None, self.ndim)
        self.e2n = e2n
        # the node count every field must have: the kernels index u with the
        # mesh's own map and check nothing
        self.n_node = int(n_node) if n_node is not None else \
            int((e2n.to(torch.int64) & 0xFFFFFFFF).max().item()) + 1
        elem = np.ascontiguousarray(np.asarray(elem).ravel())
        face = np.ascontiguousarray(np.asarray(face).ravel())
        if elem.shape != face.shape:
            raise ValueError("one face id per element id expected")
        if elem.size and (not np.issubdtype(elem.dtype, np.integer)
                          or not np.issubdtype(face.dtype, np.integer)):
            raise TypeError("element and face ids must be integers")
        # ids that do not fit the C types are out of range anyway
        if elem.size and (elem.min() < 0 or elem.max() >= self.n_elem):
            raise ValueError("faces: element id outside [0, %d)" % self.n_elem)
        if face.size and (face.min() < 0 or face.max() >= 2 * self.ndim):
            raise ValueError("faces: face id outside [0, %d)" % (2 * self.ndim))
        self.elem = elem.astype(np.int32)
        self.face = face.astype(np.uint8)
        self.n_faces = int(self.elem.size)
        self.fshape = (self.n,) * (self.ndim - 1)
        self.nf = self.n ** (self.ndim - 1)
        h = C.c_void_p()
        D = np.ascontiguousarray(D, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_faces_create(
                C.byref(h), self.ndim, self.p, self.n_elem, _lib.tptr(x_phys), _lib.tptr(e2n),
                self.n_faces, self.elem.ctypes.data_as(C.c_void_p),
                self.face.ctypes.data_as(C.c_void_p), _lib.dptr(D), _lib.dptr(w),
                self.device.index, _lib.stream_ptr()))
        self._h = h
        self._geom = None
        self._host = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sem_faces_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n_faces

    def _handle(self):
        if self._h is None:
            raise RuntimeError("this FaceSet was closed")
        return self._h

    def info(self):
        """include/sem_hip.h sem_faces_info."""
        v = (C.c_int64 * 7)()
        _lib.check(self._lib.sem_faces_info(self._handle(), v, 7))
        return dict(ndim=v[0], p=v[1], faces=v[2], nodes_per_face=v[3], distinct_nodes=v[4],
                    max_contributions=v[5], max_node=v[6])

    # ------------------------------------------------------------------ geometry
    def _fields(self):
        if self._geom is None:
            F, d, fs = self.n_faces, self.ndim, self.fshape
            kw = dict(dtype=torch.float64, device=self.device)
            g = dict(x_phys=torch.empty(F, d, *fs, **kw), n_dS=torch.empty(F, d, *fs, **kw),
                     dS=torch.empty(F, *fs, **kw), dSxW=torch.empty(F, *fs, **kw),
                     unit_normal=torch.empty(F, d, *fs, **kw),
                     node_ind=torch.empty(F, *fs, dtype=torch.int32, device=self.device),
                     J=torch.empty(F, d, d, *fs, **kw), invJ=torch.empty(F, d, d, *fs, **kw),
                     detJ=torch.empty(F, *fs, **kw))
            with torch.cuda.device(self.device):
                _lib.check(self._lib.sem_faces_geometry(
                    self._handle(), *[_lib.tptr(g[k]) for k in (
                        "x_phys", "n_dS", "dS", "dSxW", "unit_normal", "node_ind", "J", "invJ",
                        "detJ")], _lib.stream_ptr()))
            # uint32 ids as int64, the index type of torch
            g["node_ind"] = g["node_ind"].to(torch.int64) & 0xFFFFFFFF
            self._geom = g
        return self._geom

    x_phys = property(lambda self: self._fields()["x_phys"], doc="[F, ndim, *fshape]")
    n_dS = property(lambda self: self._fields()["n_dS"], doc="scaled normal [F, ndim, *fshape]")
    dS = property(lambda self: self._fields()["dS"], doc="|n_dS| [F, *fshape]")
    dSxW = property(lambda self: self._fields()["dSxW"], doc="dS x quadrature weights")
    unit_normal = property(lambda self: self._fields()["unit_normal"])
    node_ind = property(lambda self: self._fields()["node_ind"], doc="int64 [F, *fshape]")
    J = property(lambda self: self._fields()["J"], doc="J[c][i] = dx_c/dxi_i [F, d, d, *fshape]")
    invJ = property(lambda self: self._fields()["invJ"])
    detJ = property(lambda self: self._fields()["detJ"])

    def host(self):
        """The geometry tensors as host arrays (copied once)."""
        if self._host is None:
            self._host = {k: v.cpu().numpy() for k, v in self._fields().items()}
        return self._host

    # ------------------------------------------------------------------ fields
    def _field(self, u, dofs_per_node):
        """(device tensor, ncomp, comp_stride, node_stride, leading shape,
        host input?) of a global coefficient array; the kernels index it
        with the mesh's own map, so any other size is refused here."""
        is_np = not isinstance(u, torch.Tensor)
        ut = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64)) if is_np else u
        if ut.dtype != torch.float64:
            raise TypeError("u must be float64")
        ut = ut.to(self.device)
        if not ut.is_contiguous():
            ut = ut.contiguous()
        nn = self.n_node
        if dofs_per_node is not None:
            dpn = int(dofs_per_node)
            if ut.dim() != 1 or dpn < 1 or ut.numel() != dpn * nn:
                raise ValueError("interleaved u must be 1-D with dofs_per_node * n_node = %d * %d "
                                 "entries, got shape %s" % (dpn, nn, list(ut.shape)))
            return ut, dpn, 1, dpn, (dpn,), is_np
        if ut.dim() < 1 or int(ut.shape[-1]) != nn:
            raise ValueError("u must have shape [..., n_node = %d], got %s (an interleaved DOF "
                             "vector needs dofs_per_node=)" % (nn, list(ut.shape)))
        ncomp = int(ut.numel() // nn)
        if ncomp < 1:
            raise ValueError("u has an empty component axis: %s" % list(ut.shape))
        return ut, ncomp, nn, 1, tuple(ut.shape[:-1]), is_np

    def _out(self, out, shape, name):
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=self.device)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64
                and out.device == self.device and out.is_contiguous()
                and tuple(out.shape) == tuple(shape)):
            raise TypeError("%s must be a contiguous float64 tensor of shape %s on %s"
                            % (name, list(shape), self.device))
        return out

    def _grad(self, u, dofs_per_node, want_grad, want_dn, out, stream):
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        F, fs = self.n_faces, self.fshape
        g = self._out(out if want_grad else None, lead + (F, self.ndim) + fs, "out") \
            if want_grad else None
        dn = self._out(out if not want_grad else None, lead + (F,) + fs, "out") \
            if want_dn else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_faces_gradient(self._handle(), _lib.tptr(self.e2n), ncomp, cs,
                                                    ns, _lib.tptr(ut), _lib.tptr(g), _lib.tptr(dn),
                                                    _lib.stream_ptr(stream)))
        res = g if want_grad else dn
        return res.cpu().numpy() if is_np else res

    def gradient(self, u, out=None, stream=None, dofs_per_node=None):
        """Physical gradient of the parent elements' interpolant of u at the
        face nodes: u [..., n_node] -> [..., F, ndim, *fshape]; with
        ``dofs_per_node=dpn`` the interleaved [dpn * n_node] vector ->
        [dpn, F, ndim, *fshape].  Host arrays come back as host arrays."""
        return self._grad(u, dofs_per_node, True, False, out, stream)

    def normal_derivative(self, u, out=None, stream=None, dofs_per_node=None):
        """grad u . unit_normal at the face nodes, [..., F, *fshape]."""
        return self._grad(u, dofs_per_node, False, True, out, stream)

    def _sums(self, lead, per_face, out, stream, call):
        F = self.n_faces
        pf = self._out(per_face, lead + (F,), "per_face")
        tot = self._out(out, lead, "out")
        with torch.cuda.device(self.device):
            _lib.check(call(_lib.tptr(pf), _lib.tptr(tot), _lib.stream_ptr(stream)))
        return pf, tot

    def integrate(self, vals, return_per_face=False, out=None, per_face=None, stream=None):
        """sum vals dSxW over the faces (``SubFiniteElement.integrate`` of
        every face, summed): vals [..., F, *fshape] -> [...], and with
        ``return_per_face`` (per face [..., F], total).  The sums are taken
        in a fixed order: two calls give the same bits."""
        is_np = not isinstance(vals, torch.Tensor)
        v = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float64)) if is_np else vals
        if v.dtype != torch.float64:
            raise TypeError("vals must be float64")
        v = v.to(self.device).contiguous()
        tail = (self.n_faces,) + self.fshape
        k = v.dim() - len(tail)
        if k < 0 or tuple(v.shape[k:]) != tail:
            raise ValueError("vals must have shape [..., %s], got %s"
                             % (", ".join(map(str, tail)), list(v.shape)))
        lead = tuple(v.shape[:k])
        ncomp = int(np.prod(lead, dtype=np.int64))
        if ncomp < 1:
            raise ValueError("vals has an empty component axis")
        pf, tot = self._sums(lead, per_face, out, stream,
                             lambda a, b, s: self._lib.sem_faces_integrate(
                                 self._handle(), ncomp, _lib.tptr(v), a, b, s))
        if is_np:
            pf, tot = pf.cpu().numpy(), tot.cpu().numpy()
        return (pf, tot) if return_per_face else tot

    def flux(self, u, return_per_face=False, out=None, per_face=None, stream=None,
             dofs_per_node=None):
        """The integral of grad u . n over the faces, without writing the
        gradient out; shapes and repeatability as ``integrate``."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, dofs_per_node)
        pf, tot = self._sums(lead, per_face, out, stream,
                             lambda a, b, s: self._lib.sem_faces_flux(
                                 self._handle(), _lib.tptr(self.e2n), ncomp, cs, ns,
                                 _lib.tptr(ut), a, b, s))
        if is_np:
            pf, tot = pf.cpu().numpy(), tot.cpu().numpy()
        return (pf, tot) if return_per_face else tot

    def assemble(self, vals, out=None, accumulate=False, stream=None):
        """The Neumann load vector: out[node] (+)= sum vals dSxW over the
        face nodes of each boundary node (vals [F, *fshape], out [n_node];
        a new zero vector when ``out`` is None).  Nodes on no listed face
        keep their value in both modes; no atomics, two calls give the same
        bits."""
        v = torch.as_tensor(vals, dtype=torch.float64).to(self.device).contiguous()
        if tuple(v.shape) != (self.n_faces,) + self.fshape:
            raise ValueError("vals must have shape %s" % [self.n_faces, *self.fshape])
        if out is None:
            out = torch.zeros(self.n_node, dtype=torch.float64, device=self.device)
            accumulate = False
        else:
            out = self._out(out, (self.n_node,), "out")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_faces_assemble(self._handle(), _lib.tptr(v), _lib.tptr(out),
                                                    self.n_node, 1 if accumulate else 0,
                                                    _lib.stream_ptr(stream)))
        return out
