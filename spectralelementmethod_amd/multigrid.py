"""p-multigrid preconditioner of the assembled Poisson solve on the GPU.

The reference solves its Poisson systems directly (static condensation,
sem/discrete.py:502-528); the device solve is a conjugate-gradient iteration
whose count grows with the order and the mesh under the diagonal
preconditioner.  ``PMultigrid`` is a V-cycle over the orders p_0 > p_1 > ...
on the same elements (include/sem_hip.h "p-multigrid", csrc/sem_mg.hip,
DESIGN.md §4.15):

* the default ladder divides by the smallest prime factor down to 1, so every
  level's mesh nodes are a subset of the finer level's and the coarse element
  maps are subsampled fine maps (any conforming mesh, any numbering);
* every level is an ordinary ``SEMOperator`` with library geometry, adjacent
  levels are joined by a ``transfer.Transfer`` (prolong and its exact
  transpose);
* smoothing is a Chebyshev-Jacobi iteration over [lambda_max / ratio,
  lambda_max] with lambda_max(D^-1 A) estimated at setup by a fixed number of
  power iterations from a fixed start vector; the coarsest level is a longer
  Chebyshev iteration from zero.  Nothing in the cycle depends on the data,
  so M is a fixed symmetric positive definite matrix and plain PCG applies.

``SEMOperator.multigrid(dirichlet)`` builds one; ``SEMOperator.pcg_solve(...,
precond="pmg")`` solves with it.  Decompositions across ranks are out of
scope.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

# lambda_max(D^-1 A_ff) is taken as SAFETY times the Rayleigh quotient after
# POWER_ITERATIONS power iterations from start_vector().  The quotient is a
# lower bound; tests/test_mg_host.py checks on every test shape against a
# dense eigensolve that the product lies in [lambda_max, 1.5 lambda_max]
# (below, the smoother amplifies the top modes; far above, the smoothing
# interval is wasted).
POWER_ITERATIONS = 30
SAFETY = 1.15


def start_vector(n):
    """The fixed start vector of the power iteration: a multiplicative hash of
    the index mapped to [-0.5, 0.5) (exact integer arithmetic, the same on
    every machine)."""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32 - 0.5


def default_ladder(p):
    """p, then the quotient by the smallest prime factor, down to 1
    (sem_mg_ladder)."""
    lib = _lib.load()
    out, n = (C.c_int * 8)(), C.c_int(0)
    _lib.check(lib.sem_mg_ladder(int(p), out, 8, C.byref(n)))
    return [int(out[i]) for i in range(n.value)]


def check_ladder(ladder):
    """ValueError unless ``ladder`` is a descending divisor chain of orders."""
    lib = _lib.load()
    lad = [int(q) for q in ladder]
    _lib.check(lib.sem_mg_check_ladder((C.c_int * max(len(lad), 1))(*lad), len(lad)))
    return lad


def coarsen(e2n_fine, n_node_fine, p_coarse):
    """(e2n_coarse uint32, keep uint32): the subsampled element map of order
    p_coarse with compacted ids and the fine id of every coarse node
    (sem_mg_coarsen; host arrays)."""
    lib = _lib.load()
    ef = np.ascontiguousarray(e2n_fine, dtype=np.uint32)
    ndim, p_fine = ef.ndim - 1, ef.shape[1] - 1
    ec = np.zeros((ef.shape[0],) + (int(p_coarse) + 1,) * ndim, dtype=np.uint32)
    keep = np.zeros(max(int(n_node_fine), 1), dtype=np.uint32)
    nc = C.c_int64(0)
    _lib.check(lib.sem_mg_coarsen(ndim, p_fine, int(p_coarse), ef.shape[0], ef.ctypes.data,
                                  int(n_node_fine), ec.ctypes.data, keep.ctypes.data,
                                  C.byref(nc)))
    return ec, keep[:nc.value].copy()


def coarse_mask(e2n_fine, mask_fine, e2n_coarse, n_node_coarse):
    """The Dirichlet mask of the coarse level (sem_mg_coarse_mask): a coarse
    node is fixed iff every fine node of its entity (vertex, open edge, open
    face, open interior) in some element that contains it is fixed."""
    lib = _lib.load()
    ef = np.ascontiguousarray(e2n_fine, dtype=np.uint32)
    ec = np.ascontiguousarray(e2n_coarse, dtype=np.uint32)
    mf = np.ascontiguousarray(mask_fine, dtype=np.uint8)
    mc = np.zeros(max(int(n_node_coarse), 1), dtype=np.uint8)
    _lib.check(lib.sem_mg_coarse_mask(ef.ndim - 1, ef.shape[1] - 1, ec.shape[1] - 1, ef.shape[0],
                                      ef.ctypes.data, mf.size, mf.ctypes.data, ec.ctypes.data,
                                      int(n_node_coarse), mc.ctypes.data))
    return mc[:int(n_node_coarse)].astype(bool)


def estimate_lambda_max(op, mask, iterations=POWER_ITERATIONS, safety=SAFETY):
    """safety * (v . A v) / (v . D v) after ``iterations`` power iterations of
    D^-1 A on the free DOFs of ``op`` from start_vector() (setup only: torch
    operations around the operator's action)."""
    d = op.diag()
    free = ~mask
    dinv = torch.where(free, 1.0 / d, torch.zeros_like(d))
    v = torch.from_numpy(start_vector(op.ndof)).to(op.device) * free
    lam = 0.0
    for _ in range(int(iterations)):
        av = op.apply(v)
        lam = float(torch.dot(v, av) / torch.dot(v, d * v))
        w = dinv * av
        v = w / torch.linalg.vector_norm(w)
    return float(safety) * lam


class PMultigrid(object):
    """The V-cycle preconditioner M of one Poisson ``SEMOperator`` and one
    Dirichlet mask, and the PCG that runs with it.

    Parameters
    ----------
    op : SEMOperator
        The fine level: Poisson, one DOF per node, library geometry, no node
        states (NotImplementedError otherwise).  It is level 0 as it stands,
        in the caller's numbering.
    dirichlet : bool [ndof]
        True where x is fixed (ValueError for another size).
    ladder : list of int, optional
        The orders of the levels, ``op.p`` first, a descending divisor chain
        (ValueError otherwise).  Default: ``default_ladder(op.p)``.
    smooth_degree, smooth_ratio : int, float
        Chebyshev degree and lambda_max / lambda_min of the pre- and
        post-smoother of every level but the coarsest.
    coarse_degree, coarse_ratio : int, float
        The same for the coarsest level's iteration from zero.

    Members: ``levels`` (the operators, fine first), ``transfers`` (level
    l + 1 -> l), ``masks`` (device bool), ``lambda_max`` (per level).  The
    object keeps its operators alive; ``close()`` frees the coarse ones.
    """

    def __init__(self, op, dirichlet, ladder=None, smooth_degree=2, coarse_degree=8,
                 smooth_ratio=4.0, coarse_ratio=30.0, kind=0):
        from .operators import SEMOperator, op_kind, POISSON
        self._lib = _lib.load()
        self._h = None
        self.levels, self.transfers = [], []
        if op_kind(kind) != POISSON:
            raise NotImplementedError("p-multigrid: the Poisson operator")
        if op.dpn != 1:
            raise NotImplementedError("p-multigrid: dofs_per_node == 1")
        if op._shared:
            raise NotImplementedError("p-multigrid: operators without node states")
        if op._user_geom:
            raise NotImplementedError("p-multigrid: library geometry (set_geometry was called)")
        if op.geometry == "reference":
            raise NotImplementedError("p-multigrid: geometry 'auto', 'nodal' or 'stored'")
        mask = np.asarray(dirichlet.cpu() if isinstance(dirichlet, torch.Tensor) else dirichlet)
        mask = mask.astype(bool).ravel()
        if mask.size != op.ndof:
            raise ValueError("dirichlet mask has %d entries, expected ndof = %d"
                             % (mask.size, op.ndof))
        self.ladder = default_ladder(op.p) if ladder is None else check_ladder(ladder)
        if self.ladder[0] != op.p:
            raise ValueError("the ladder starts at order %d, the operator has order %d"
                             % (self.ladder[0], op.p))
        self.op, self.device = op, op.device
        self.smooth_degree, self.coarse_degree = int(smooth_degree), int(coarse_degree)
        self.smooth_ratio, self.coarse_ratio = float(smooth_ratio), float(coarse_ratio)
        # the levels: subsampled maps, kept nodes, coarse masks (host)
        e2n = op.e2n.cpu().numpy().view(np.uint32)
        nodes = op.nodes.cpu().numpy()
        self.levels, masks = [op], [mask]
        for q in self.ladder[1:]:
            ec, keep = coarsen(e2n, nodes.shape[1], q)
            mc = coarse_mask(e2n, masks[-1], ec, keep.size)
            nodes = np.ascontiguousarray(nodes[:, keep.astype(np.int64)])
            self.levels.append(SEMOperator(q, ec, nodes, device=self.device,
                                           geometry=op.geometry))
            masks.append(mc)
            e2n = ec
        with torch.cuda.device(self.device):
            self.masks = [torch.from_numpy(m).to(self.device) for m in masks]
            self.transfers = [c.transfer_to(f, check=False)
                              for f, c in zip(self.levels[:-1], self.levels[1:])]
            self.lambda_max = [estimate_lambda_max(o, m) for o, m in zip(self.levels, self.masks)]
            L = len(self.levels)
            self._masks8 = [m.to(torch.uint8).contiguous() for m in self.masks]
            ctxs = (C.c_void_p * L)(*[o._ctx for o in self.levels])
            trs = (C.c_void_p * max(L - 1, 1))(*[t._handle() for t in self.transfers])
            mks = (C.c_void_p * L)(*[m.data_ptr() for m in self._masks8])
            lam = (C.c_double * L)(*self.lambda_max)
            h = C.c_void_p()
            _lib.check(self._lib.sem_mg_create(
                C.byref(h), L, ctxs, trs, mks, lam, self.smooth_degree, self.coarse_degree,
                self.smooth_ratio, self.coarse_ratio, self.device.index, _lib.stream_ptr()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sem_mg_destroy(self._h)
            self._h = None
        for t in getattr(self, "transfers", []):
            t.close()
        for o in getattr(self, "levels", [])[1:]:  # level 0 is the caller's
            o.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise RuntimeError("this PMultigrid was closed")
        return self._h

    def matches(self, op, dirichlet):
        """Was this hierarchy built for ``op`` and this mask?"""
        m = torch.as_tensor(dirichlet, dtype=torch.bool).to(self.device).ravel()
        return op is self.op and m.numel() == op.ndof and bool(torch.equal(m, self.masks[0]))

    def info(self):
        """include/sem_hip.h sem_mg_info: per level the DOFs, the operator
        actions and vector passes of one cycle as planned, and as the last
        cycle enqueued them."""
        L = len(self.levels)
        v = (C.c_int64 * (4 + 5 * L))()
        _lib.check(self._lib.sem_mg_info(self._handle(), v, 4 + 5 * L))
        lv = [dict(p=self.ladder[l], ndof=v[4 + 5 * l], actions=v[5 + 5 * l],
                   passes=v[6 + 5 * l], actions_run=v[7 + 5 * l], passes_run=v[8 + 5 * l],
                   lambda_max=self.lambda_max[l]) for l in range(L)]
        return dict(levels=lv, smooth_degree=v[1], coarse_degree=v[2], vector_bytes=v[3])

    def _vec(self, v, name):
        if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64
                and v.device == self.device and v.is_contiguous()
                and v.numel() == self.op.ndof):
            raise ValueError("%s must be a contiguous float64 tensor of %d entries on %s"
                             % (name, self.op.ndof, self.device))
        return v

    def vcycle(self, r, out=None, stream=None):
        """z = M r (entries of r on fixed DOFs are ignored, z is 0 there).
        Device tensors; a host array comes back as a host array.  Allocates
        nothing when ``out`` is given and does not synchronise."""
        is_np = not isinstance(r, torch.Tensor)
        if is_np:
            r = torch.as_tensor(np.ascontiguousarray(r, dtype=np.float64)).to(self.device)
        r = self._vec(r, "r")
        out = torch.empty_like(r) if out is None else self._vec(out, "out")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_mg_vcycle(self._handle(), _lib.tptr(r), _lib.tptr(out),
                                               _lib.stream_ptr(stream)))
        return out.cpu().numpy() if is_np else out

    def profile(self, r, stream=None):
        """Milliseconds per level of one cycle (sem_mg_profile; diagnostic,
        synchronises)."""
        r = self._vec(r, "r")
        out = torch.empty_like(r)
        ms = (C.c_double * len(self.levels))()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_mg_profile(self._handle(), _lib.tptr(r), _lib.tptr(out), ms,
                                                _lib.stream_ptr(stream)))
        return list(ms)

    def solve(self, rhs, x, rtol=1e-13, max_iter=20000, check_every=1, stream=None):
        """PCG with M on the free DOFs (sem_mg_pcg_solve, the semantics of
        ``SEMOperator.pcg_solve``): ``x`` (device tensor) holds the Dirichlet
        values on entry and is updated in place.  Returns (x, iterations,
        relative residual); ValueError when not converged."""
        h = self._handle()
        rhs = self.op._vec(rhs, "rhs")
        if not isinstance(x, torch.Tensor) or x.device != self.device:
            raise TypeError("x must be a device tensor on %s" % self.device)
        x = self.op._vec(x, "x")
        its, rel = C.c_int(0), C.c_double(0.0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sem_mg_pcg_solve(h, _lib.tptr(rhs), _lib.tptr(x), float(rtol),
                                                  int(max_iter), int(check_every), C.byref(its),
                                                  C.byref(rel), _lib.stream_ptr(stream)))
        return x, its.value, rel.value
