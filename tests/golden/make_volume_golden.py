#!/usr/bin/env python
"""Generate tests/golden/volume.npz by running the REFERENCE's element
post-processing (FiniteElement.gradient / integrate / detJxW,
sem/discrete.py:594-597, 680-688) on every element of the five cases of
make_points_golden.py.

Test infrastructure like make_goldens.py, whose helpers (reference import
shims, synthetic meshes) it reuses; only its output is committed.

Per case: nodes and element map as the reference's DOFManager leaves them,
the reference's x_phys, the smooth nodal field of make_points_golden.py, and
per element gradient(u_local) [E, 2, n, n], integrate(u_local) [E],
integrate(1) [E] and detJxW [E, n, n].  ``ref_seconds_per_element`` is the
reference's measured time per element for the gradient and the two integrals
on the generating host.

The generator also checks, on the CPU, that the float64 twin
(tests/volume_twin.py) meets what it stores to 1e-12 relative.

Usage:  python tests/golden/make_volume_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402
from make_points_golden import smooth_field  # noqa: E402
import volume_twin  # noqa: E402

KEYS = ("gradient", "integrate", "integrate_one", "detJxW")


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


def main():
    mg._TABLES.update(mg.decode_basis_hdf5())
    mg.install_runtime_shims()
    from sem.discrete import DOFManager
    cases = [("sq_p2", "square", 2, False), ("sq_p4", "square", 4, False),
             ("sq_p8", "square", 8, False), ("ann_p6", "annulus", 6, False),
             ("sq_p4_rcm", "square", 4, True)]
    out = {"cases": np.array([c[0] for c in cases])}
    t_total, n_total = 0.0, 0
    for name, kind, p, rcm in cases:
        if kind == "square":
            nodes, e2n = mg.structured_square(3, 2, p, warp=0.06)
        else:
            nodes, e2n = mg.annulus(4, 3, p)
        mesh = mg.ref_mesh(nodes, e2n)
        _, tb = mg.ref_basis(p)
        dm = DOFManager(mesh, 1, tb, rcm_order=rcm)
        u = smooth_field(mesh.nodes)
        rows = {k: [] for k in KEYS}
        x_phys = []
        for fe in dm.finite_elements(x_phys=True, Jacobian=True):
            x_phys.append(fe.x_phys.copy())
            ul = u[fe.node_ind]
            t0 = time.perf_counter()
            vals = dict(gradient=fe.gradient(ul), integrate=fe.integrate(ul),
                        integrate_one=fe.integrate(1))
            t_total += time.perf_counter() - t0
            n_total += 1
            vals["detJxW"] = fe.detJxW
            for k in KEYS:
                rows[k].append(np.array(vals[k], dtype=np.float64))
        x_phys = np.stack(x_phys)
        e2n_ref = mg.mesh_map(mesh)
        out[name + "_p"] = np.array(p)
        out[name + "_nodes"] = mesh.nodes.copy()
        out[name + "_e2n"] = e2n_ref
        out[name + "_x_phys"] = x_phys
        out[name + "_u"] = u
        for k in KEYS:
            out[name + "_" + k] = np.stack(rows[k])
        # the float64 twin on the same x_phys
        D = np.asarray(tb.get_D1_matrices()[0], dtype=np.float64)
        w = np.asarray(tb.quad_rule.weights[0], dtype=np.float64)
        tw = volume_twin.Twin(x_phys, e2n_ref, mesh.nodes.shape[1], D, w)
        errs = dict(gradient=rel(tw.gradient(u), out[name + "_gradient"]),
                    integrate=rel(tw.integrate(u)[0], out[name + "_integrate"]),
                    integrate_one=rel(tw.integrate_local(np.ones_like(tw.detJxW))[0],
                                      out[name + "_integrate_one"]),
                    detJxW=rel(tw.detJxW, out[name + "_detJxW"]))
        print("  %s: %d elements, twin to reference %s" % (
            name, x_phys.shape[0], " ".join("%s %.1e" % kv for kv in errs.items())))
        assert max(errs.values()) <= 1e-12, errs
    out["ref_seconds_per_element"] = np.array(t_total / n_total)
    print("  reference: %.3e s per element" % (t_total / n_total))
    path = os.path.join(mg.OUT, "volume.npz")
    np.savez_compressed(path, **out)
    print("volume.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
