#!/usr/bin/env python
"""Generate tests/golden/faces.npz by running the REFERENCE's boundary
sub-elements (FiniteElement.sub_fe -> SubFiniteElement / SubMapping,
sem/discrete.py:699-775, sem/mapping.py:184-272) on all four faces of every
element of the five cases of make_points_golden.py.

Test infrastructure like make_goldens.py, whose helpers (reference import
shims, synthetic meshes) it reuses; only its output is committed.

Per case: nodes and element map as the reference's DOFManager leaves them,
the reference's x_phys, the smooth nodal field of make_points_golden.py, and
for the faces in (element, face) order, face = 0..3 fastest: x_phys, n_dS,
dS, dSxW, unit_normal, node_ind, gradient(u_local) and integrate(1).
``ref_seconds_per_face`` is the reference's measured time per sub-element
built and evaluated on the generating host.

The generator also checks, on the CPU, that the float64 twin
(tests/faces_twin.py) meets what it stores to 1e-12 relative.

Usage:  python tests/golden/make_faces_golden.py
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
import faces_twin  # noqa: E402

KEYS = ("x_phys", "n_dS", "dS", "dSxW", "unit_normal", "node_ind", "gradient", "integrate")


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
            for face in range(4):
                t0 = time.perf_counter()
                sub = fe.sub_fe(face)
                vals = dict(x_phys=sub.x_phys, n_dS=sub.n_dS, dS=sub.dS, dSxW=sub.dSxW,
                            unit_normal=sub.unit_normal, node_ind=sub.node_ind,
                            gradient=sub.gradient(ul), integrate=sub.integrate(np.ones(p + 1)))
                t_total += time.perf_counter() - t0
                n_total += 1
                for k in KEYS:
                    rows[k].append(np.array(vals[k]))
        x_phys = np.stack(x_phys)
        e2n_ref = mg.mesh_map(mesh)
        out[name + "_p"] = np.array(p)
        out[name + "_nodes"] = mesh.nodes.copy()
        out[name + "_e2n"] = e2n_ref
        out[name + "_x_phys"] = x_phys
        out[name + "_u"] = u
        for k in KEYS:
            out[name + "_face_" + k] = np.stack(rows[k])
        # the float64 twin on the same x_phys
        D = np.asarray(tb.get_D1_matrices()[0], dtype=np.float64)
        w = np.asarray(tb.quad_rule.weights[0], dtype=np.float64)
        E = x_phys.shape[0]
        tw = faces_twin.Twin(x_phys, D, w, np.repeat(np.arange(E), 4), np.tile(np.arange(4), E))
        assert np.array_equal(tw.node_ind(e2n_ref), out[name + "_face_node_ind"])
        errs = {k: rel(getattr(tw, k), out[name + "_face_" + k])
                for k in ("x_phys", "n_dS", "dS", "dSxW", "unit_normal")}
        errs["gradient"] = rel(tw.gradient(u, e2n_ref)[0], out[name + "_face_gradient"])
        errs["integrate"] = rel(tw.integrate(np.ones_like(tw.dS))[0],
                                out[name + "_face_integrate"])
        print("  %s: %d faces, twin to reference %s" % (
            name, 4 * E, " ".join("%s %.1e" % kv for kv in errs.items())))
        assert max(errs.values()) <= 1e-12, errs
    out["ref_seconds_per_face"] = np.array(t_total / n_total)
    print("  reference: %.3e s per face" % (t_total / n_total))
    path = os.path.join(mg.OUT, "faces.npz")
    np.savez_compressed(path, **out)
    print("faces.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
