#!/usr/bin/env python
"""Generate tests/golden/points.npz by running the REFERENCE's point location
and interpolation (DOFManager.find_elem_containing_point / interpolate,
sem/discrete.py:221-233, 263-280; Mapping.inv, sem/mapping.py:146-178).

Test infrastructure like make_goldens.py, whose helpers (reference import
shims, synthetic meshes) it reuses; only its output is committed.

Per case: nodes and element map as the reference's DOFManager leaves them
(rcm_order False, plus one case with the default RCM numbering), the
reference's x_phys, 64 seeded interior query points, the reference's element
id and xi of each, its own round-trip error |x(xi) - x|, the value of
DOFManager.interpolate for a smooth nodal field, and the mask of points with
min(1 - |xi|) >= 1e-6 (a point on a face may belong to either neighbour, so
only those are compared on the element id).  The generator asserts that the
reference locates every point.  ``ref_seconds_per_point`` is the reference's
measured time per located and interpolated point on the generating host.

Usage:  python tests/golden/make_points_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402

N_POINTS = 64
INTERIOR_MARGIN = 1e-6


def smooth_field(nodes):
    x, y = nodes
    return np.sin(x) + np.cos(2.0 * y) + 0.25 * x * y


def query_points(kind, rng):
    if kind == "square":
        return rng.uniform(-0.95, 0.95, size=(2, N_POINTS))
    r = rng.uniform(1.05, 3.95, size=N_POINTS)
    th = rng.uniform(0.1, np.pi - 0.1, size=N_POINTS)
    return np.stack([r * np.sin(th), r * np.cos(th)])


def main():
    mg._TABLES.update(mg.decode_basis_hdf5())
    mg.install_runtime_shims()
    from sem.discrete import DOFManager
    cases = [("sq_p2", "square", 2, False), ("sq_p4", "square", 4, False),
             ("sq_p8", "square", 8, False), ("ann_p6", "annulus", 6, False),
             ("sq_p4_rcm", "square", 4, True)]
    rng = np.random.default_rng(20240607)
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
        xq = query_points(kind, rng)
        elem = np.empty(N_POINTS, dtype=np.int32)
        xi = np.empty((2, N_POINTS))
        vals = np.empty(N_POINTS)
        rt = 0.0
        cell_ids = {id_key(mesh.get_cell(i)): i for i in range(mesh.n_cells)}
        for k in range(N_POINTS):
            t0 = time.perf_counter()
            fe, x_param = dm.find_elem_containing_point(xq[:, k])  # raises if dropped
            vals[k] = dm.interpolate(u, xq[:, k])
            t_total += time.perf_counter() - t0
            n_total += 1
            elem[k] = cell_ids[id_key(fe._cell)]
            xi[:, k] = x_param
            rt = max(rt, float(np.abs(np.asarray(fe.mapping(x_param)).reshape(2)
                                      - xq[:, k]).max()))
        assert np.isfinite(xi).all() and np.isfinite(vals).all()
        x_phys = np.stack([fe.x_phys for fe in dm.finite_elements(x_phys=True)])
        out[name + "_p"] = np.array(p)
        out[name + "_nodes"] = mesh.nodes.copy()
        out[name + "_e2n"] = mg.mesh_map(mesh)
        out[name + "_x_phys"] = x_phys
        out[name + "_u"] = u
        out[name + "_xq"] = xq
        out[name + "_elem"] = elem
        out[name + "_xi"] = xi
        out[name + "_vals"] = vals
        out[name + "_roundtrip"] = np.array(rt)
        out[name + "_interior"] = (1.0 - np.abs(xi)).min(axis=0) >= INTERIOR_MARGIN
        print("  %s: %d/%d located, round trip %.2e, interior %d" %
              (name, N_POINTS, N_POINTS, rt, int(out[name + "_interior"].sum())))
    out["ref_seconds_per_point"] = np.array(t_total / n_total)
    print("  reference: %.3e s per point" % (t_total / n_total))
    path = os.path.join(mg.OUT, "points.npz")
    np.savez_compressed(path, **out)
    print("points.npz %d bytes" % os.path.getsize(path))


def id_key(cell):
    return tuple(np.asarray(cell.node_ind_lexicographic).ravel()[:4].tolist())


if __name__ == "__main__":
    main()
