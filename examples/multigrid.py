#!/usr/bin/env python
r"""One Poisson problem solved with both preconditioners of the device PCG.

    -lap u = 1  on the warped square, u = 0.2((x+1) + (y+1)) on all four sides

The matrix-free operator (SEMOperator), the right-hand side assembled from
detJxW, then ``pcg_solve`` twice: with the diagonal (Jacobi) preconditioner,
the default, and with the p-multigrid V-cycle over the orders p, p / 2, ...
(``precond="pmg"``, multigrid.PMultigrid).  Prints iterations, times and the
difference of the two solutions.  The reference has no iterative solve
(sem/discrete.py:502-528 is a direct one).

    python examples/multigrid.py [--p 8 --nex 64 --ney 64 --warp 0.05 --rtol 1e-10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectralelementmethod_amd import meshgen  # noqa: E402


def main(argv=None):
    import torch
    from spectralelementmethod_amd.operators import SEMOperator
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--nex", type=int, default=64)
    ap.add_argument("--ney", type=int, default=64)
    ap.add_argument("--warp", type=float, default=0.05)
    ap.add_argument("--rtol", type=float, default=1e-10)
    args = ap.parse_args(argv)
    nodes, e2n = meshgen.structured_square(args.nex, args.ney, args.p, warp=args.warp)
    x, y = nodes
    fixed = (np.abs(np.abs(nodes) - 1.0) < 1e-12).any(axis=0)
    op = SEMOperator(args.p, e2n, nodes)
    rhs = op.assemble(op.geometry_fields()["detJxW"])
    u0 = torch.from_numpy(np.where(fixed, 0.2 * ((x + 1) + (y + 1)), 0.0)).to(op.device)

    def solve(**kw):
        u = u0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u, its, rel = op.pcg_solve(rhs, u, fixed, rtol=args.rtol, **kw)
        torch.cuda.synchronize()
        return u, its, rel, time.perf_counter() - t0

    t0 = time.perf_counter()
    mg = op.multigrid(fixed)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    print("%d x %d elements, p = %d, %d DOF; levels %s, lambda_max %s, set-up %.3f s"
          % (args.nex, args.ney, args.p, op.ndof, mg.ladder,
             ["%.3f" % v for v in mg.lambda_max], t_setup))
    solve(), solve(precond=mg)                       # warm-up
    uj, its_j, rel_j, t_j = solve()
    um, its_m, rel_m, t_m = solve(precond=mg)
    diff = float(torch.linalg.vector_norm(um - uj) / torch.linalg.vector_norm(uj))
    print("Jacobi-PCG: %5d iterations, %.4f s, relative residual %.1e" % (its_j, t_j, rel_j))
    print("pMG-PCG:    %5d iterations, %.4f s, relative residual %.1e" % (its_m, t_m, rel_m))
    print("the two solutions differ by %.2e (relative L2); time ratio %.2f" % (diff, t_j / t_m))
    return um.cpu().numpy()


if __name__ == "__main__":
    main()
