"""Fields between two polynomial orders of one mesh on the GPU.

The reference has no such operation: carrying a solution from the order-p_a
discretisation of a mesh to the order-p_b discretisation of the same mesh
(p-refinement, nested iteration, error indication by comparing orders, or a
change of node numbering at p_a == p_b) is a host loop over elements there.
``Transfer`` does it with the kernels of libsem_hip.so (include/sem_hip.h
"Transfer", csrc/sem_transfer.hip), on quadrilaterals and hexahedra for any
pair of orders in 1..16:

* ``prolong(u)``: the "from" interpolant of every element evaluated at the
  element's "to" GLL nodes; a node several elements share takes the value of
  its owner, the lowest (element, local index) pair, so two calls give the
  same bits;
* ``restrict(r)``: the exact transpose of that matrix, summed in a fixed
  order without atomics.

``SEMOperator.transfer_to(other)`` builds one from two operators on the same
elements; ``multigrid.PMultigrid`` builds its V-cycle on them (DESIGN.md
§4.15).  Transfers across the ranks of a decomposition are out of scope
(DESIGN.md §9).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _corners(nodes, e2n, ndim):
    """Corner coordinates [E, 2^ndim, ndim] of every element, in the order of
    the element's own local axes."""
    e2n = np.asarray(e2n).astype(np.int64) & 0xFFFFFFFF
    ends = np.ix_(*([[0, -1]] * ndim))
    ids = e2n[(slice(None),) + ends].reshape(e2n.shape[0], -1)
    return np.moveaxis(np.asarray(nodes)[:, ids], 0, -1)


class Transfer(object):
    """Prolongation and its transpose between two discretisations of the
    same elements on one GPU.

    Parameters
    ----------
    e2n_from, e2n_to : uint32 [E, n_from, n_from(, n_from)], [E, n_to, ...]
        The two element maps: same elements in the same order, same local
        axis orientation per element.  An id >= its node count raises
        ValueError before any kernel.
    n_node_from, n_node_to : int
        Node counts: the sizes every vector must have.
    device : optional
    keep : optional
        Anything to keep alive with the transfer (the two operators).
    """

    def __init__(self, e2n_from, n_node_from, e2n_to, n_node_to, device=None, keep=None):
        self._lib = _lib.load()
        self._h = None
        from .operators import SEMOperator, _device_index
        self.device = torch.device("cuda", _device_index(device))
        # the library borrows the two maps until destroy: they live here
        self.e2n_from = SEMOperator._to_map(e2n_from).to(self.device).contiguous()
        self.e2n_to = SEMOperator._to_map(e2n_to).to(self.device).contiguous()
        self._keep = keep
        self.ndim = self.e2n_from.dim() - 1
        if self.ndim not in (2, 3) or self.e2n_to.dim() != self.e2n_from.dim():
            raise ValueError("element maps must both have shape [E, n, n] or [E, n, n, n]")
        self.n_from, self.n_to = int(self.e2n_from.shape[1]), int(self.e2n_to.shape[1])
        self.p_from, self.p_to = self.n_from - 1, self.n_to - 1
        if tuple(self.e2n_from.shape[1:]) != (self.n_from,) * self.ndim or \
                tuple(self.e2n_to.shape[1:]) != (self.n_to,) * self.ndim:
            raise ValueError("element maps must have shape [E] + [n] * ndim")
        if self.e2n_from.shape[0] != self.e2n_to.shape[0]:
            raise ValueError("the two discretisations have %d and %d elements"
                             % (self.e2n_from.shape[0], self.e2n_to.shape[0]))
        self.n_elem = int(self.e2n_from.shape[0])
        self.n_node_from, self.n_node_to = int(n_node_from), int(n_node_to)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_transfer_create(
                C.byref(h), self.ndim, self.p_from, self.p_to, self.n_elem,
                _lib.tptr(self.e2n_from), self.n_node_from, _lib.tptr(self.e2n_to),
                self.n_node_to, self.device.index, _lib.stream_ptr()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sem_transfer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise RuntimeError("this Transfer was closed")
        return self._h

    def info(self):
        """include/sem_hip.h sem_transfer_info."""
        v = (C.c_int64 * 9)()
        _lib.check(self._lib.sem_transfer_info(self._handle(), v, 9))
        return dict(ndim=v[0], p_from=v[1], p_to=v[2], elements=v[3], nodes_from=v[4],
                    nodes_to=v[5], owned_entries=v[6], max_contributions=v[7],
                    scratch_bytes=v[8])

    # ------------------------------------------------------------------ fields
    def _field(self, u, nn, dofs_per_node, name):
        """(device tensor, ncomp, comp_stride, node_stride, leading shape,
        host input?) of a coefficient array of nn nodes (the conventions of
        ``PointSet.evaluate``); any other size is refused here, the kernels
        check nothing."""
        is_np = not isinstance(u, torch.Tensor)
        ut = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64)) if is_np else u
        if ut.dtype != torch.float64:
            raise TypeError("%s must be float64" % name)
        ut = ut.to(self.device)
        if not ut.is_contiguous():
            ut = ut.contiguous()
        if dofs_per_node is not None:
            dpn = int(dofs_per_node)
            if ut.dim() != 1 or dpn < 1 or ut.numel() != dpn * nn:
                raise ValueError("interleaved %s must be 1-D with dofs_per_node * n_node = %d * %d "
                                 "entries, got shape %s" % (name, dpn, nn, list(ut.shape)))
            return ut, dpn, 1, dpn, None, is_np
        if ut.dim() < 1 or int(ut.shape[-1]) != nn:
            raise ValueError("%s must have shape [..., n_node = %d], got %s (an interleaved DOF "
                             "vector needs dofs_per_node=)" % (name, nn, list(ut.shape)))
        ncomp = int(ut.numel() // nn) if nn else int(np.prod(ut.shape[:-1], dtype=np.int64))
        if ncomp < 1:
            raise ValueError("%s has an empty component axis: %s" % (name, list(ut.shape)))
        return ut, ncomp, nn, 1, tuple(ut.shape[:-1]), is_np

    def _out(self, out, lead, ncomp, nn, zero):
        """The output of ncomp components of nn nodes, laid out as the input
        (lead None: interleaved), with its strides."""
        shape = (ncomp * nn,) if lead is None else lead + (nn,)
        cs, ns = (1, ncomp) if lead is None else (nn, 1)
        if out is None:
            make = torch.zeros if zero else torch.empty
            return make(shape, dtype=torch.float64, device=self.device), cs, ns
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64
                and out.device == self.device and out.is_contiguous()
                and tuple(out.shape) == tuple(shape)):
            raise ValueError("out must be a contiguous float64 tensor of shape %s on %s"
                             % (list(shape), self.device))
        return out, cs, ns

    def prolong(self, u, out=None, stream=None, dofs_per_node=None):
        """u [..., n_node_from] -> [..., n_node_to]; with ``dofs_per_node=dpn``
        the interleaved [dpn * n_node_from] vector -> [dpn * n_node_to].  "To"
        nodes no element references keep what ``out`` holds (0 in a new
        output).  Host arrays come back as host arrays."""
        ut, ncomp, cs, ns, lead, is_np = self._field(u, self.n_node_from, dofs_per_node, "u")
        res, cs_o, ns_o = self._out(out, lead, ncomp, self.n_node_to, True)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_transfer_prolong(
                self._handle(), ncomp, cs, ns, _lib.tptr(ut), cs_o, ns_o, _lib.tptr(res),
                _lib.stream_ptr(stream)))
        return res.cpu().numpy() if is_np else res

    def restrict(self, r, out=None, accumulate=False, stream=None, dofs_per_node=None):
        """The transpose of ``prolong``: r [..., n_node_to] -> [...,
        n_node_from] (interleaved with ``dofs_per_node``).  Every "from" node
        is written (0 where no element references it); ``accumulate=True``
        adds to ``out`` instead."""
        rt, ncomp, cs, ns, lead, is_np = self._field(r, self.n_node_to, dofs_per_node, "r")
        if out is None:
            accumulate = False
        res, cs_o, ns_o = self._out(out, lead, ncomp, self.n_node_from, False)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_transfer_restrict(
                self._handle(), ncomp, cs, ns, _lib.tptr(rt), cs_o, ns_o, _lib.tptr(res),
                1 if accumulate else 0, _lib.stream_ptr(stream)))
        return res.cpu().numpy() if is_np else res


def between(op_from, op_to, check=True):
    """The ``Transfer`` from one ``SEMOperator`` to another on the same
    elements (``SEMOperator.transfer_to``)."""
    if op_from.device != op_to.device:
        raise ValueError("the two operators live on %s and %s" % (op_from.device, op_to.device))
    if op_from.ndim != op_to.ndim:
        raise ValueError("the two operators have %d and %d dimensions"
                         % (op_from.ndim, op_to.ndim))
    if op_from.n_elem != op_to.n_elem:
        raise ValueError("the two discretisations have %d and %d elements"
                         % (op_from.n_elem, op_to.n_elem))
    if check:
        ca, cb = (_corners(op.nodes.cpu().numpy(), op.e2n.cpu().numpy().view(np.uint32), op.ndim)
                  for op in (op_from, op_to))
        size = float(np.abs(ca).max()) if ca.size else 1.0
        bad = np.flatnonzero(np.abs(ca - cb).max(axis=(1, 2)) > 1e-9 * max(size, 1e-300))
        if bad.size:
            raise ValueError("element %d (and %d more) of the two meshes differ in their corner "
                             "coordinates: the elements or their local axes do not correspond"
                             % (bad[0], bad.size - 1))
    return Transfer(op_from.e2n, op_from.n_node, op_to.e2n, op_to.n_node, device=op_from.device,
                    keep=(op_from, op_to))
