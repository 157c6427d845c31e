"""Resample a solved Poisson field onto a uniform image grid on the GPU.

Solves -lap u = 1 on a (warped) square with the essential boundary values of
examples/poisson.py on the left and bottom edges, matrix-free on the device,
then reads the solution back on an M x M pixel grid: ``locate`` finds element
and parametric coordinates of every pixel centre once, ``evaluate``
interpolates the field there (and would do so again for every further field
or time step).  The reference does this one point at a time with
``DOFManager.interpolate`` (sem/discrete.py:221-233).

  python examples/resample.py --p 8 --nex 64 --ney 64 --pixels 512 --out u.npy
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectralelementmethod_amd import meshgen  # noqa: E402
from spectralelementmethod_amd.operators import SEMOperator  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--nex", type=int, default=32)
    ap.add_argument("--ney", type=int, default=32)
    ap.add_argument("--warp", type=float, default=0.05)
    ap.add_argument("--pixels", type=int, default=256, help="image is pixels x pixels")
    ap.add_argument("--out", default=None, help="write the image as .npy")
    args = ap.parse_args(argv)

    nodes, e2n = meshgen.structured_square(args.nex, args.ney, args.p, args.warp)
    op = SEMOperator(args.p, e2n, nodes)
    on, vals = meshgen.square_dirichlet_left_bottom(nodes)      # u = 0.2 ((x+1) + (y+1)) there
    fixed = torch.from_numpy(on).to(op.device)
    rhs = op.assemble(op.geometry_fields()["detJxW"])          # f = 1
    u = torch.from_numpy(vals).to(op.device)
    u, its, rel = op.pcg_solve(rhs, u, fixed, rtol=1e-12)

    m = args.pixels
    c = (torch.arange(m, dtype=torch.float64, device=op.device) + 0.5) * (2.0 / m) - 1.0
    gx, gy = torch.meshgrid(c, c, indexing="ij")
    pixels = torch.stack([gx.reshape(-1), gy.reshape(-1)])      # [2, m * m]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ps = op.point_locator().locate(pixels)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    image = ps.evaluate(u).reshape(m, m)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    back = (ps.physical() - pixels).abs().max().item()
    print("ndof %d, PCG %d iterations (rel. residual %.1e)" % (op.ndof, its, rel))
    print("%d x %d pixels: %d outside the mesh, locate %.2f ms, evaluate (with its plan) "
          "%.2f ms, round trip %.1e" % (m, m, ps.n_outside, 1e3 * (t1 - t0), 1e3 * (t2 - t1),
                                       back))
    print("u: max %.6f at pixel %s, mean %.6f" % (
        image.max().item(), tuple(int(v) for v in np.unravel_index(
            int(image.argmax().item()), (m, m))), image.mean().item()))
    if args.out:
        np.save(args.out, image.cpu().numpy())
    return image


if __name__ == "__main__":
    main()
