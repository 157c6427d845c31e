"""Time of the volume kernels (volume.VolumeSet) at the benchmark sizes, p = 8:

  quad  1024^2 quadrilaterals (67.1 M nodes);
  hex   27^3 hexahedra (10.2 M nodes).

``gradient``, ``recover``, ``norms`` (of u - v) and ``integrate`` are timed in
steady state: warm-up, then device events around a window of about
``--window`` seconds.  Each against two baselines:

  (a) the torch composition a user would write from ``geometry_fields()``:
      an index gather, one ``matmul`` with D per direction, an elementwise
      multiply-sum with the stored invJ, products with the stored detJxW,
      ``index_add_`` for the recovery, timed the same way.  (a) and the new
      path alternate in the same process for ``--rounds`` rounds; an
      operation passes when its slowest round is faster than the fastest
      round of (a), i.e. it wins by more than the spread seen in this run.
      Repeat the command to see the spread between runs.
  (b) a device-to-device copy that moves the bytes the call must move (read +
      written, computed from the shapes below), i.e. a buffer of half those
      bytes copied once.  The ratio is recorded, not gated.

The geometry is a smooth warp of the structured mesh evaluated at the GLL
nodes on the device (the times do not depend on it); the stored invJ / detJxW
of (a) are computed from the same x_phys.  ``reference_s_per_element`` is the
reference's own time per element from tests/golden/volume.npz.  Exit status 1
when an operation does not pass against (a).

  python tools/bench_volume.py [--shapes quad,hex] [--small] [--out FILE]
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
from spectralelementmethod_amd.operators import _basis_arrays  # noqa: E402
from spectralelementmethod_amd.volume import VolumeSet  # noqa: E402

OPS = ("gradient", "recover", "norms", "integrate")


def steady(fn, window):
    """Seconds per call of fn() in steady state (device events)."""
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    k = max(5, int(window * 1e3 / max(ev[0].elapsed_time(ev[1]), 1e-3)))
    ev[0].record()
    for _ in range(k):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3 / k


def mesh(name, small, p, dev):
    """(x_phys [E, nd, n, ..] on the device, e2n, n_node) of the warped
    structured benchmark mesh."""
    basis, D, w, _ = _basis_arrays(p, None, 2 if name == "quad" else 3)
    xi = torch.from_numpy(np.asarray(basis._subbases[0].nodes, dtype=np.float64)).to(dev)
    n = p + 1
    if name == "quad":
        ne, nd = (128 if small else 1024), 2
        e2n, nn = meshgen._element_map(ne, ne, p, ne * p + 1), (ne * p + 1) ** 2
    elif name == "hex":
        ne, nd = (9 if small else 27), 3
        N = ne * p + 1
        e2n, nn = meshgen._element_map3(ne, ne, ne, p, N, N), N ** 3
    else:
        raise ValueError("unknown shape %r" % name)
    # straight coordinates in [-1, 1] per axis: element index slowest first
    line = (torch.arange(ne, dtype=torch.float64, device=dev)[:, None] * 2.0
            + (xi[None, :] + 1.0)) / ne - 1.0                       # [ne, n]
    ax = []
    for a in range(nd):
        shape = [1] * (2 * nd)
        shape[a], shape[nd + a] = ne, n
        ax.append(line.reshape(shape).expand(*([ne] * nd + [n] * nd)))
    warp = 0.05 / nd
    bump = sum(torch.sin(np.pi * (c + 0.3 * k)) for k, c in enumerate(ax))
    x = torch.stack([c + warp * bump * torch.cos(0.5 * np.pi * c) for c in ax], dim=nd)
    x_phys = x.reshape((ne ** nd, nd) + (n,) * nd).contiguous()
    return x_phys, e2n, nn, D, w


def stored_geometry(x_phys, D, w):
    """invJ [E, i, j, n, ..] and detJxW [E, n, ..] with torch, as
    ``geometry_fields()`` stores them."""
    nd = x_phys.shape[1]
    letters = "ijk"[:nd]
    J = torch.stack([torch.einsum("%sm,ec%s->ec%s" % (letters[i], letters.replace(letters[i], "m"),
                                                      letters), D, x_phys)
                     for i in range(nd)], dim=2)                     # [E, c, i, ...]
    # cofactors: inv[i][j] = C[j][i] / det
    if nd == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        rows = [[J[:, 1, 1], -J[:, 0, 1]], [-J[:, 1, 0], J[:, 0, 0]]]
    else:
        def cof(r, k):
            r1, r2, k1, k2 = (r + 1) % 3, (r + 2) % 3, (k + 1) % 3, (k + 2) % 3
            return J[:, r1, k1] * J[:, r2, k2] - J[:, r1, k2] * J[:, r2, k1]
        det = sum(J[:, 0, k] * cof(0, k) for k in range(3))
        rows = [[cof(j, i) for j in range(3)] for i in range(3)]
    inv = torch.stack([torch.stack(r, dim=1) for r in rows], dim=1) / det[:, None, None]
    W = w
    for _ in range(nd - 1):
        W = W[..., None] * w
    return inv, det * W


def run(name, small, window, rounds, p=8):
    dev = torch.device("cuda", torch.cuda.current_device())
    x_phys, e2n, nn, D, w = mesh(name, small, p, dev)
    nd, n = x_phys.shape[1], p + 1
    E, nloc = x_phys.shape[0], n ** x_phys.shape[1]
    ent = E * nloc
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = VolumeSet(x_phys=x_phys, e2n=e2n, n_node=nn, device=dev)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    kw = dict(dtype=torch.float64, device=dev)
    u = torch.randn(nn, **kw)
    v = u * (1.0 + 1e-3 * torch.randn(nn, **kw))
    eshape = (E,) + (n,) * nd
    o_grad = torch.empty((E, nd) + (n,) * nd, **kw)
    o_rec, o_int, o_nrm = torch.empty(nd, nn, **kw), torch.empty((), **kw), torch.empty(2, **kw)
    new = dict(gradient=lambda: vol.gradient(u, out=o_grad),
               recover=lambda: vol.recover(u, out=o_rec),
               norms=lambda: vol.norms(u, v, out=o_nrm),
               integrate=lambda: vol.integrate(u, out=o_int))

    # (a) the same operations composed from torch calls on stored geometry
    Dt, wt = torch.from_numpy(D).to(dev), torch.from_numpy(w).to(dev)
    invJ, detJxW = stored_geometry(x_phys, Dt, wt)
    idx = torch.from_numpy(e2n.reshape(-1).astype(np.int64)).to(dev)
    mass = vol.mass
    DtT = Dt.T.contiguous()
    res = {}

    def t_grad(f):
        # one matmul with D^T per direction (that axis moved last), then an
        # elementwise multiply-sum with the stored invJ (torch.einsum for
        # either step picks a far slower path at these shapes: 140 ms at
        # 1024^2, measured, against the figures this form gives)
        ul = f[idx].reshape(eshape)
        du = torch.stack([torch.matmul(ul.movedim(1 + i, -1), DtT).movedim(-1, 1 + i)
                          for i in range(nd)], dim=1)                          # [E, i, ...]
        return (invJ * du[:, :, None]).sum(dim=1)                              # [E, j, ...]

    def torch_gradient():
        res["gradient"] = t_grad(u)

    def torch_recover():
        g = t_grad(u) * detJxW[:, None]
        num = torch.zeros(nd, nn, **kw)
        num.index_add_(1, idx, g.movedim(1, 0).reshape(nd, -1))
        res["recover"] = num / mass

    def torch_norms():
        d = u - v
        dl = d[idx].reshape(eshape)
        g = t_grad(d)
        res["norms"] = torch.stack([(detJxW * dl * dl).sum(), (detJxW * (g * g).sum(dim=1)).sum()])

    def torch_integrate():
        res["integrate"] = (detJxW * u[idx].reshape(eshape)).sum()
    old = dict(gradient=torch_gradient, recover=torch_recover, norms=torch_norms,
               integrate=torch_integrate)
    times = {k: dict(new=[], torch=[]) for k in OPS}
    for _ in range(rounds):
        for k in OPS:
            times[k]["torch"].append(steady(old[k], window))
            times[k]["new"].append(steady(new[k], window))
    outs = dict(gradient=o_grad, recover=o_rec, norms=o_nrm, integrate=o_int)
    diff = {k: float((outs[k] - res[k]).norm() / res[k].norm()) for k in OPS}
    del invJ, detJxW, idx, res

    # (b) a copy of the bytes each call must move
    common = nn * 8 + ent * 4 + ent * nd * 8               # u, the map, x_phys
    nbytes = dict(gradient=common + ent * nd * 8,
                  recover=common + 2 * ent * nd * 8 + (nn + 1) * 4 + ent * 4 + nn * 8 + nd * nn * 8,
                  norms=common + nn * 8 + 2 * E * 8,
                  integrate=nn * 8 + ent * 4 + ent * 8 + E * 8)    # u, the map, the stored detJxW
    copy = {}
    for k in OPS:
        src = torch.empty(nbytes[k] // 16, **kw)
        dst = torch.empty_like(src)
        copy[k] = steady(lambda: dst.copy_(src), window)
        del src, dst
    golden = np.load(os.path.join(ROOT, "tests", "golden", "volume.npz"))
    rec = dict(shape=name, small=bool(small), ndim=nd, p=p, n_elem=E, n_node=nn,
               create_s=t_create, rounds=rounds, info=vol.info(),
               reference_s_per_element=float(golden["ref_seconds_per_element"]))
    ok = True
    for k in OPS:
        t_new, t_old = times[k]["new"], times[k]["torch"]
        beats = max(t_new) < min(t_old)
        ok = ok and beats
        rec[k] = dict(new_s=t_new, torch_s=t_old, new_median_s=float(np.median(t_new)),
                      torch_median_s=float(np.median(t_old)),
                      speedup_over_torch=float(np.median(t_old) / np.median(t_new)),
                      beats_torch_beyond_spread=bool(beats), bytes=nbytes[k], copy_s=copy[k],
                      time_over_copy=float(np.median(t_new) / copy[k]),
                      bytes_per_s=float(nbytes[k] / np.median(t_new)), torch_rel_diff=diff[k],
                      s_per_element=float(np.median(t_new) / E))
    print(json.dumps(rec), flush=True)
    vol.close()
    return rec, ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="quad,hex")
    ap.add_argument("--small", action="store_true", help="reduced shapes (a quick check)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of steady state per call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of (a) and the new path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume", "bench_volume.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume needs a HIP device")
    done = [run(s, a.small, a.window, a.rounds) for s in a.shapes.split(",") if s]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(results=[r for r, _ in done]), f, indent=1)
    return 0 if all(ok for _, ok in done) else 1


if __name__ == "__main__":
    sys.exit(main())
