#!/usr/bin/env python
"""Generate tests/golden/elem_matrices.npz by running the REFERENCE's element
operators on the first and last element of the ``p4_3x2`` annulus case.

Test infrastructure like make_goldens.py, whose helpers (reference import
shims, ``annulus``, ``ref_mesh``, ``axisym_ops``, ``axisym_Ae``,
``poisson_Lse``) it reuses; only its output is committed.

Stored per element e in ``elems`` (lexicographic local DOFs, DOF = 2 node +
comp for the two-component systems):
  jac_l   [2 n^2, 2 n^2]  the Newton Jacobian of compute_local_system
                          (examples/squirmer-axisymmetric.py:272-291)
  rhs_l   [2 n^2]         -res_l of the same call (:292-296)
  Lse     [n^2, n^2]      the element Laplacian (examples/poisson.py:166-193)
at the state and Reynolds number of tests/golden/axisym_ns.npz (``p4_3x2``),
whose nodes and element map are the mesh.

Usage:  python tests/golden/make_elem_matrices_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

CASE, P, NTH, NR = "p4_3x2", 4, 3, 2


def main():
    mg._TABLES.update(mg.decode_basis_hdf5())
    mg.install_runtime_shims()
    from sem.discrete import DOFManager
    from sem.sp_array import KroneckerArray
    np.float = float  # sem/sp_array.py:39 (NumPy >= 1.24 removed np.float)
    ns = np.load(os.path.join(HERE, "axisym_ns.npz"))
    nodes, e2n = mg.annulus(NTH, NR, P)
    mesh = mg.ref_mesh(nodes, e2n)
    assert np.array_equal(mg.mesh_map(mesh), ns[CASE + "_e2n"])
    assert np.array_equal(mesh.nodes, ns[CASE + "_nodes"])
    _, tb = mg.ref_basis(P)
    dm = DOFManager(mesh, 2, tb, rcm_order=False)
    n_rey = float(ns[CASE + "_re"])
    sol = ns[CASE + "_soln"]
    sfn, vort = sol[0::2], sol[1::2]
    elems = [0, mesh.n_cells - 1]
    out = {"case": np.array(CASE), "elems": np.array(elems), "re": np.array(n_rey)}
    for e, fe in enumerate(dm.finite_elements(x_phys=True, Jacobian=True)):
        if e not in elems:
            continue
        E2e, Lve, Me_d = mg.axisym_ops(fe)
        Ae = mg.axisym_Ae(fe, n_rey)
        Me = KroneckerArray(shape=fe.basis.coeff_shape * 2)
        Me.add_diag(Me_d, [0, 1, 0, 1])
        loc = fe.node_ind
        s_l, w_l = sfn[loc], vort[loc]
        nn = loc.size
        Ae_w = Ae.dot_dense(w_l, [4, 5])
        jac = np.zeros((2 * nn, 2 * nn))
        jac[0::2, 0::2] = Ae_w.to_array().reshape(nn, nn)
        jac[0::2, 1::2] = (Ae.dot_dense(s_l, [2, 3]).to_array() + Lve).reshape(nn, nn)
        jac[1::2, 0::2] = E2e.reshape(nn, nn)
        jac[1::2, 1::2] = -Me.to_array().reshape(nn, nn)
        res = np.zeros(2 * nn)
        res[0::2] = (Ae_w.dot_dense(s_l, [2, 3]).to_array()
                     + np.einsum("pqrs,rs", Lve, w_l)).ravel()
        res[1::2] = (np.einsum("pqrs,rs", E2e, s_l)
                     - Me.dot_dense(w_l, [2, 3]).to_array()).ravel()
        Lse, _ = mg.poisson_Lse(fe)
        out["jac_l_%d" % e] = jac
        out["rhs_l_%d" % e] = -res
        out["Lse_%d" % e] = Lse.reshape(nn, nn)
        print("  element %d: |jac_l| = %.6e  |rhs_l| = %.6e  |Lse| = %.6e"
              % (e, np.linalg.norm(jac), np.linalg.norm(res), np.linalg.norm(Lse)))
    path = os.path.join(HERE, "elem_matrices.npz")
    np.savez_compressed(path, **out)
    print("elem_matrices.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
