"""NumPy twin of the volume formulas (include/sem_hip.h "Volume"), written
from the stated definitions, evaluated in float64 or np.longdouble from the
same float64 x_phys.  The yardstick of tests/test_volume_host.py and
tests/test_gpu_volume.py.

J[c][i] = dx_c/dxi_i from x_phys and D; invJ by cofactors; detJxW = det J
times the tensor of the 1-D weights; grad_j = sum_i invJ[i][j] du/dxi_i;
mass = detJxW summed into the nodes; recover = (detJxW grad summed into the
nodes) / mass; norms of d = u - v formed at the nodes first."""
import numpy as np

from faces_twin import _inverse, element_derivs


class Twin(object):
    """Volume fields of the mesh x_phys [E, ndim, n, ..], e2n [E, n, ..]."""

    def __init__(self, x_phys, e2n, n_node, D, w, dtype=np.float64):
        self.dtype = dtype
        x = np.asarray(x_phys).astype(dtype)
        self.D = np.asarray(D).astype(dtype)
        w = np.asarray(w).astype(dtype)
        self.ndim = nd = x.shape[1]
        self.n = x.shape[2]
        self.E = x.shape[0]
        self.e2n = np.asarray(e2n).astype(np.int64)
        self.n_node = int(n_node)
        d = element_derivs(x, self.D, nd)                    # [i, E, c, n, ..]
        self.J = np.moveaxis(d, (2, 0), (0, 1))              # [c, i, E, n, ..]
        self.invJ, self.detJ = _inverse(self.J)              # [i, j, E, ..], [E, ..]
        W = w
        for _ in range(nd - 1):
            W = np.multiply.outer(W, w)
        self.detJxW = self.detJ * W
        self.mass = self.assemble(self.detJxW)

    def assemble(self, elem_vals):
        """Element values [E, n, ..] summed into the nodes [n_node]."""
        out = np.zeros(self.n_node, self.dtype)
        np.add.at(out, self.e2n.ravel(), np.asarray(elem_vals).astype(self.dtype).ravel())
        return out

    def gradient_local(self, ul):
        """[E, ndim, n, ..] of element-local coefficients [E, n, ..]."""
        du = element_derivs(np.asarray(ul).astype(self.dtype), self.D, self.ndim)  # [i, E, ..]
        g = (self.invJ * du[:, None]).sum(axis=0)            # sum_i invJ[i][j] du_i: [j, E, ..]
        return np.moveaxis(g, 0, 1)

    def gradient(self, u):
        return self.gradient_local(np.asarray(u).astype(self.dtype)[self.e2n])

    def recover(self, u):
        """[ndim, n_node]; 0 where no element references a node."""
        g = self.gradient(u)
        out = np.zeros((self.ndim, self.n_node), self.dtype)
        has = self.mass != 0
        for j in range(self.ndim):
            s = self.assemble(self.detJxW * g[:, j])
            out[j, has] = s[has] / self.mass[has]
        return out

    def integrate_local(self, vals):
        """(per element [E], total) of sum vals detJxW."""
        per = (np.asarray(vals).astype(self.dtype) * self.detJxW).reshape(self.E, -1).sum(axis=1)
        return per, per.sum()

    def integrate(self, u):
        return self.integrate_local(np.asarray(u).astype(self.dtype)[self.e2n])

    def norms(self, u, v=None):
        """(per element [E, 2], total [2]) of the squares: sum detJxW d^2 and
        sum detJxW |grad d|^2, d = u - v."""
        d = np.asarray(u).astype(self.dtype)
        if v is not None:
            d = d - np.asarray(v).astype(self.dtype)
        dl = d[self.e2n]
        g = self.gradient_local(dl)
        per = np.stack([self.integrate_local(dl * dl)[0],
                        self.integrate_local((g * g).sum(axis=1))[0]], axis=1)
        return per, per.sum(axis=0)


def node_coordinates(x_phys, e2n, n_node):
    """[ndim, n_node] physical coordinates of the GLL nodes from x_phys (NaN
    at nodes no element references)."""
    x = np.asarray(x_phys)
    out = np.full((x.shape[1], int(n_node)), np.nan)
    out[:, np.asarray(e2n).astype(np.int64)] = np.moveaxis(x, 1, 0)
    return out


def smooth(xn):
    """A smooth field of node coordinates [ndim, N]."""
    s = np.sin(1.3 * xn[0]) + np.cos(2.0 * xn[1]) + 0.25 * xn[0] * xn[1]
    if xn.shape[0] == 3:
        s = s + np.sin(0.7 * xn[2] + 0.3) * (1.0 + 0.5 * xn[0])
    return s
