"""Throughput of point location and field evaluation (points.PointLocator).

Shapes:
  resample  the 1024^2, p = 8 Poisson mesh onto a 4096^2 pixel grid
            (1.68e7 points, ~16 per element);
  hex       27^3 hexahedra, p = 8, onto 256^3 points (~850 per element);
  sparse    1e5 random points in the 1024^2 mesh (~1 per touched element:
            the gather dominates).
``locate`` (and the plan) is timed once; ``evaluate`` in steady state:
warm-up, then device events around a window of about ``--window`` seconds.
Each result line is JSON: points/s, the algorithmic bytes from the shapes
(map + u per touched element, xi, the permutation, the items, the output),
the multiply-adds, and the share of the HBM and fp64 vector peaks.  The
reference's seconds per point (tests/golden/points.npz, its only baseline)
is printed beside them.

  python tools/bench_points.py [--shapes resample,hex,sparse] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spectralelementmethod_amd import meshgen  # noqa: E402
from spectralelementmethod_amd.operators import SEMOperator  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X specification
FP64_VECTOR_PEAK = 78.6e12  # FLOP/s, MI355X specification (vector fp64)


def pixel_grid(ndim, m, device):
    """Pixel centres of an m^ndim grid over [-1, 1]^ndim, [ndim, m^ndim]."""
    c = (torch.arange(m, dtype=torch.float64, device=device) + 0.5) * (2.0 / m) - 1.0
    g = torch.meshgrid(*([c] * ndim), indexing="ij")
    return torch.stack([a.reshape(-1) for a in g]).contiguous()


def shape(name, small):
    if name == "resample":
        ne, m = (128, 512) if small else (1024, 4096)
        nodes, e2n = meshgen.structured_square(ne, ne, 8, warp=0.05)
        return 8, nodes, e2n, lambda dev: pixel_grid(2, m, dev)
    if name == "hex":
        ne, m = (9, 64) if small else (27, 256)
        nodes, e2n = meshgen.structured_cube(ne, ne, ne, 8, warp=0.05)
        return 8, nodes, e2n, lambda dev: pixel_grid(3, m, dev)
    if name == "sparse":
        ne, m = (128, 2000) if small else (1024, 100000)
        nodes, e2n = meshgen.structured_square(ne, ne, 8, warp=0.05)
        g = torch.Generator().manual_seed(1)
        x = torch.rand(2, m, dtype=torch.float64, generator=g) * 1.98 - 0.99
        return 8, nodes, e2n, lambda dev: x.to(dev)
    raise ValueError("unknown shape %r" % name)


def run(name, small, window):
    p, nodes, e2n, points = shape(name, small)
    t0 = time.perf_counter()
    op = SEMOperator(p, e2n, nodes)
    del nodes
    loc = op.point_locator()
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    xq = points(op.device)
    m = int(xq.shape[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ps = loc.locate(xq)
    torch.cuda.synchronize()
    t_locate = time.perf_counter() - t0
    t0 = time.perf_counter()
    plan = ps.plan_info()
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t0
    u = torch.randn(op.n_node, dtype=torch.float64, device=op.device)
    out = torch.empty(m, dtype=torch.float64, device=op.device)
    for _ in range(3):
        ps.evaluate(u, out=out)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    ps.evaluate(u, out=out)
    ev[1].record()
    torch.cuda.synchronize()
    k = max(3, int(window * 1e3 / max(ev[0].elapsed_time(ev[1]), 1e-3)))
    ev[0].record()
    for _ in range(k):
        ps.evaluate(u, out=out)
    ev[1].record()
    torch.cuda.synchronize()
    sec = ev[0].elapsed_time(ev[1]) * 1e-3 / k
    nd, n = op.ndim, op.n
    nloc = n ** nd
    valid = plan["in_runs"]
    bytes_model = (plan["touched_elements"] * nloc * (4 + 8) + valid * (nd * 8 + 4 + 8)
                   + plan["items"] * 12)
    fma = valid * sum(n ** k for k in range(1, nd + 1))
    bw, fl = bytes_model / sec, 2.0 * fma / sec
    rec = dict(shape=name, small=bool(small), ndim=nd, p=p, n_elem=op.n_elem, points=m,
               outside=ps.n_outside, points_per_element=valid / max(plan["touched_elements"], 1),
               item_width=plan["width"], items=plan["items"], grid=loc.info()["grid"],
               max_candidates=loc.info()["max_candidates"], setup_s=t_setup,
               locate_s=t_locate, locate_points_per_s=m / t_locate, plan_s=t_plan,
               evaluate_s=sec, evaluate_repeats=k, evaluate_points_per_s=m / sec,
               bytes=bytes_model, fma=fma, bytes_per_s=bw, flop_per_s=fl,
               hbm_peak_share=bw / HBM_PEAK, fp64_vector_peak_share=fl / FP64_VECTOR_PEAK,
               bound=("memory" if bw / HBM_PEAK > fl / FP64_VECTOR_PEAK else "compute"))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="resample,hex,sparse")
    ap.add_argument("--small", action="store_true", help="reduced shapes (a quick check)")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of steady-state evaluate")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    a = ap.parse_args()
    recs = [run(s, a.small, a.window) for s in a.shapes.split(",") if s]
    ref = float(np.load(os.path.join(ROOT, "tests", "golden", "points.npz"))["ref_seconds_per_point"])
    print(json.dumps(dict(reference_seconds_per_point=ref)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(results=recs, reference_seconds_per_point=ref), f, indent=1)


if __name__ == "__main__":
    main()
