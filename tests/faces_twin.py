"""NumPy twin of the boundary-face formulas (include/sem_hip.h "Faces"),
written from the stated conventions, evaluated in float64 or np.longdouble
from the same float64 x_phys.  The yardstick of tests/test_faces_host.py and
tests/test_gpu_faces.py.

Conventions: face = 2 * axis + side (side 0: xi = -1).  2-D faces run
counter-clockwise (faces 0 and 3 reversed).  3-D side-1 faces carry the axes
(axis+1, axis+2) mod 3, side-0 faces (axis+2, axis+1) mod 3.  Tangents are the
matching columns of J[c][i] = dx_c/dxi_i (negated on 2-D faces 0 and 3);
n_dS = (t_y, -t_x) or t0 x t1; dS = |n_dS|; dSxW = dS times the tensor of the
1-D weights; grad_j = sum_i invJ[i][j] du/dxi_i."""
import numpy as np


def face_slice(face, arr, ndim):
    """The trailing ndim element axes of arr restricted to the face, in face
    order, by explicit slicing and transposes."""
    ax, side = divmod(face, 2)
    k = -1 if side else 0
    lead = arr.ndim - ndim
    if ndim == 2:
        line = arr[..., k, :] if ax == 0 else arr[..., :, k]
        return line[..., ::-1] if face in (0, 3) else line
    # move the element axes to (ax, ax+1, ax+2) cyclically, cut the first
    cyc = [lead + (ax + j) % 3 for j in range(3)]
    a = np.transpose(arr, list(range(lead)) + cyc)[..., k, :, :]
    return a if side else np.swapaxes(a, -1, -2)


def index_table(ndim, n):
    lin = np.arange(n ** ndim).reshape((n,) * ndim)
    return np.stack([face_slice(f, lin, ndim).ravel() for f in range(2 * ndim)])


def element_derivs(a, D, ndim):
    """d a / d xi_i of element arrays a [..., n, .., n]: [ndim, ..., n, .., n]."""
    out = []
    for i in range(ndim):
        axis = a.ndim - ndim + i
        out.append(np.moveaxis(np.tensordot(a, D, axes=([axis], [1])), -1, axis))
    return np.stack(out)


def _inverse(J):
    """Inverse and determinant of J [d, d, ...] by cofactors (any dtype)."""
    d = J.shape[0]
    if d == 2:
        det = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
        inv = np.stack([np.stack([J[1, 1], -J[0, 1]]), np.stack([-J[1, 0], J[0, 0]])]) / det
        return inv, det
    C = np.empty_like(J)
    for r in range(3):
        for k in range(3):
            r1, r2, k1, k2 = (r + 1) % 3, (r + 2) % 3, (k + 1) % 3, (k + 2) % 3
            C[r, k] = J[r1, k1] * J[r2, k2] - J[r1, k2] * J[r2, k1]
    det = J[0, 0] * C[0, 0] + J[0, 1] * C[0, 1] + J[0, 2] * C[0, 2]
    return np.swapaxes(C, 0, 1) / det, det


class Twin(object):
    """Face geometry of the (elem, face) pairs from x_phys [E, ndim, n, ..]."""

    def __init__(self, x_phys, D, w, elem, face, dtype=np.float64):
        self.dtype = dtype
        x = np.asarray(x_phys).astype(dtype)
        self.D = np.asarray(D).astype(dtype)
        self.w = np.asarray(w).astype(dtype)
        self.ndim = nd = x.shape[1]
        self.n = n = x.shape[2]
        self.elem = np.asarray(elem, dtype=np.int64)
        self.face = np.asarray(face, dtype=np.int64)
        self.fshape = (n,) * (nd - 1)
        used = np.unique(self.elem)
        geo = {}
        for e in used:
            # J[c][i]: derivative i of component c
            J = np.swapaxes(element_derivs(x[e], self.D, nd), 0, 1)
            inv, det = _inverse(J)
            geo[e] = (x[e], J, inv, det)
        F = self.elem.size
        fs = self.fshape
        self.x_phys = np.empty((F, nd) + fs, dtype)
        self.J = np.empty((F, nd, nd) + fs, dtype)
        self.invJ = np.empty((F, nd, nd) + fs, dtype)
        self.detJ = np.empty((F,) + fs, dtype)
        self.n_dS = np.empty((F, nd) + fs, dtype)
        self.W = self.w if nd == 2 else self.w[:, None] * self.w[None, :]
        for k in range(F):
            e, f = self.elem[k], self.face[k]
            xe, J, inv, det = geo[e]
            self.x_phys[k] = face_slice(f, xe, nd)
            self.J[k] = Jf = face_slice(f, J, nd)
            self.invJ[k] = face_slice(f, inv, nd)
            self.detJ[k] = face_slice(f, det, nd)
            ax, side = divmod(f, 2)
            if nd == 2:
                t = Jf[:, 1 - ax] * (-1 if f in (0, 3) else 1)
                self.n_dS[k, 0], self.n_dS[k, 1] = t[1], -t[0]
            else:
                b, c = (ax + 1) % 3, (ax + 2) % 3
                t0, t1 = (Jf[:, b], Jf[:, c]) if side else (Jf[:, c], Jf[:, b])
                self.n_dS[k] = np.stack([t0[1] * t1[2] - t0[2] * t1[1],
                                         t0[2] * t1[0] - t0[0] * t1[2],
                                         t0[0] * t1[1] - t0[1] * t1[0]])
        self.dS = np.sqrt((self.n_dS ** 2).sum(axis=1))
        self.unit_normal = self.n_dS / self.dS[:, None]
        self.dSxW = self.dS * self.W
        self.n_dSxW = self.n_dS * self.W

    def node_ind(self, e2n):
        e2n = np.asarray(e2n).astype(np.int64)
        return np.stack([face_slice(f, e2n[e], self.ndim) for e, f in zip(self.elem, self.face)]) \
            if self.elem.size else np.empty((0,) + self.fshape, np.int64)

    def gradient(self, u, e2n):
        """grad [F, ndim, *fshape] and its product with the unit normal of the
        global coefficient vector u [n_node]."""
        e2n = np.asarray(e2n).astype(np.int64)
        u = np.asarray(u).astype(self.dtype)
        nd = self.ndim
        g = np.empty((self.elem.size, nd) + self.fshape, self.dtype)
        cache = {}
        for k, (e, f) in enumerate(zip(self.elem, self.face)):
            if e not in cache:
                cache[e] = element_derivs(u[e2n[e]], self.D, nd)
            du = face_slice(f, cache[e], nd)                       # [i, *fshape]
            g[k] = (self.invJ[k] * du[:, None]).sum(axis=0)        # sum_i invJ[i][j] du_i
        return g, (g * self.unit_normal).sum(axis=1)

    def integrate(self, vals):
        """per face and total of sum vals dSxW (vals [F, *fshape])."""
        per = (np.asarray(vals).astype(self.dtype) * self.dSxW).reshape(self.elem.size, -1).sum(1)
        return per, per.sum()

    def flux(self, u, e2n):
        return self.integrate(self.gradient(u, e2n)[1])

    def assemble(self, vals, e2n, n_node):
        out = np.zeros(n_node, self.dtype)
        np.add.at(out, self.node_ind(e2n).ravel(),
                  (np.asarray(vals).astype(self.dtype) * self.dSxW).ravel())
        return out
