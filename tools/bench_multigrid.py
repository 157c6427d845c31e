#!/usr/bin/env python3
"""Time the assembled Poisson solve to 1e-10 with Jacobi-PCG and with
pMG-PCG (multigrid.PMultigrid) on one GPU.

Both solvers run from the same build on the same operator, right-hand side
and mask (all sides Dirichlet, warp 0.05, random right-hand side), after one
warm-up solve each (code objects, clocks), alternating Jacobi / pMG for
``--reps`` rounds; the Jacobi solve is `SEMOperator.pcg_solve`'s default
path.  Per solver: iterations, wall time of every round (host clock around a
device synchronise), time per iteration; for pMG also the set-up time and the
per-level split of one cycle (sem_mg_profile: device events between the
levels' segments, median of 5).

    python tools/bench_multigrid.py                 # 128^2, 256^2, hex 27^3 at p = 8
    python tools/bench_multigrid.py --cases quad128

writes profiles/multigrid/bench_multigrid.json (--out).  Two more modes
measure the fused smoother pass alone, on a single-level hierarchy so that
every kernel name has one size:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python tools/bench_multigrid.py --smoother-cycles 1024
    python tools/bench_multigrid.py --trace-csv DIR/run_kernel_trace.csv --trace-n 1024

the second turns the trace into bytes / time per pass (bytes counted from the
arrays each pass reads and writes) and merges it into the JSON.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quad128": (2, 128, 8), "quad256": (2, 256, 8), "hex27": (3, 27, 8)}
# doubles per DOF each vector pass of csrc/sem_mg.hip reads + writes
PASS_DOUBLES = {"k_mg_first<2, false>": 4, "k_mg_first<2, true>": 7,
                "k_mg_step<2, true>": 8, "k_mg_step<2, false>": 7}


def problem(ndim, ne, p):
    import numpy as np
    from spectralelementmethod_amd import meshgen
    if ndim == 2:
        nodes, e2n = meshgen.structured_square(ne, ne, p, warp=0.05)
    else:
        nodes, e2n = meshgen.structured_cube(ne, ne, ne, p, warp=0.05)
    mask = (np.abs(np.abs(nodes) - 1.0) < 1e-12).any(axis=0)
    rhs = np.random.default_rng(0).standard_normal(nodes.shape[1])
    return nodes, e2n, mask, rhs


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run_case(name, reps, rtol):
    import torch
    from spectralelementmethod_amd.operators import SEMOperator
    ndim, ne, p = CASES[name]
    nodes, e2n, mask, rhs = problem(ndim, ne, p)
    op = SEMOperator(p, e2n, nodes, device="cuda:0")
    b = torch.from_numpy(rhs).cuda()
    m = torch.from_numpy(mask).cuda()
    t_setup, mg = timed(lambda: op.multigrid(mask))

    def jacobi():
        return op.pcg_solve(b, torch.zeros_like(b), m, rtol=rtol, max_iter=200000)

    def pmg():
        return op.pcg_solve(b, torch.zeros_like(b), m, rtol=rtol, max_iter=2000, precond=mg)
    jacobi(), pmg()                                   # warm-up: code objects, clocks
    rec = {"jacobi": [], "pmg": []}
    for _ in range(reps):                             # alternating
        for key, fn in (("jacobi", jacobi), ("pmg", pmg)):
            t, (x, its, rel) = timed(fn)
            rec[key].append((t, its, rel, x))
    diff = float(torch.linalg.vector_norm(rec["pmg"][-1][3] - rec["jacobi"][-1][3]) /
                 torch.linalg.vector_norm(rec["jacobi"][-1][3]))
    out = dict(case=name, ndim=ndim, elements_per_side=ne, p=p, ndof=op.ndof, rtol=rtol,
               ladder=mg.ladder, lambda_max=mg.lambda_max, setup_s=t_setup,
               solutions_rel_l2=diff)
    for key, runs in rec.items():
        ts = [r[0] for r in runs]
        out[key] = dict(iterations=runs[-1][1], relres=runs[-1][2], wall_s=ts, wall_s_min=min(ts),
                        ms_per_iteration=1e3 * min(ts) / max(runs[-1][1], 1))
    out["speedup_wall_min"] = out["jacobi"]["wall_s_min"] / out["pmg"]["wall_s_min"]
    r = torch.randn(op.ndof, dtype=torch.float64, device="cuda")
    prof = [mg.profile(r) for _ in range(6)][1:]
    out["cycle_ms_per_level"] = [statistics.median(c[l] for c in prof)
                                 for l in range(len(mg.levels))]
    out["levels"] = mg.info()["levels"]
    mg.close()
    op.close()
    return out


def smoother_cycles(ne, cycles=10):
    """Cycles of a single-level hierarchy (Chebyshev of degree 3 from zero:
    k_mg_first<2, false>, then k_mg_step<2, true> and k_mg_step<2, false>)
    at ne x ne, p = 8, for a kernel trace."""
    import torch
    from spectralelementmethod_amd.operators import SEMOperator
    nodes, e2n, mask, rhs = problem(2, ne, 8)
    op = SEMOperator(8, e2n, nodes, device="cuda:0")
    mg = op.multigrid(mask, ladder=[8], coarse_degree=3)
    r = torch.from_numpy(rhs).cuda()
    z = torch.empty_like(r)
    for _ in range(cycles):
        mg.vcycle(r, out=z)
    torch.cuda.synchronize()
    print("smoother cycles: %d at %d DOF" % (cycles, op.ndof))


def trace_summary(path, ne):
    """{kernel: median microseconds, bytes per DOF, TB/s} of the vector
    passes in a rocprofv3 kernel trace of smoother_cycles(ne)."""
    ndof = (8 * ne + 1) ** 2
    dur = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "").replace(" ", "")
            for key in PASS_DOUBLES:
                if key.replace(" ", "") in name:
                    dur.setdefault(key, []).append(int(row["End_Timestamp"]) -
                                                   int(row["Start_Timestamp"]))
    out = {"ndof": ndof}
    for key, d in sorted(dur.items()):
        d = d[len(d) // 3:]                             # past the clock ramp
        us = statistics.median(d) / 1e3
        nbytes = 8 * PASS_DOUBLES[key] * ndof
        out[key] = dict(calls=len(d), median_us=us, bytes_per_dof=8 * PASS_DOUBLES[key],
                        tb_per_s=nbytes / (us * 1e-6) / 1e12)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multigrid",
                                                  "bench_multigrid.json"))
    ap.add_argument("--smoother-cycles", type=int, metavar="NE")
    ap.add_argument("--trace-csv")
    ap.add_argument("--trace-n", type=int, default=1024)
    args = ap.parse_args()
    if args.smoother_cycles:
        return smoother_cycles(args.smoother_cycles)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    if args.trace_csv:
        doc["smoother_pass"] = trace_summary(args.trace_csv, args.trace_n)
        print(json.dumps(doc["smoother_pass"]))
    else:
        import torch
        doc["device"] = torch.cuda.get_device_name(0)
        doc.setdefault("cases", {})
        for name in args.cases:
            doc["cases"][name] = run_case(name, args.reps, args.rtol)
            c = doc["cases"][name]
            print("%s (%d DOF): Jacobi %d its %.4f s, pMG %d its %.4f s (x %.2f), set-up %.2f s, "
                  "cycle per level %s ms" % (name, c["ndof"], c["jacobi"]["iterations"],
                                             c["jacobi"]["wall_s_min"], c["pmg"]["iterations"],
                                             c["pmg"]["wall_s_min"], c["speedup_wall_min"],
                                             c["setup_s"],
                                             ["%.3f" % v for v in c["cycle_ms_per_level"]]),
                  flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
