"""Time of the order-transfer kernels (transfer.Transfer) at the benchmark
sizes, p = 4 -> 8:

  quad  1024^2 quadrilaterals (16.8 M "from" nodes, 67.1 M "to" nodes);
  hex   27^3 hexahedra (1.3 M and 10.2 M nodes).

``prolong`` and ``restrict`` are timed in steady state: warm-up, then device
events around a window of about ``--window`` seconds.  Beside each:

  (a) a torch composition of the same operation from ready index tensors
      (index gather, ``einsum`` with J per direction, ``index_copy_`` of the
      owned entries / ``index_add_``), timed the same way;
  (b) a device-to-device copy that moves the same number of bytes as the call
      must (read + written: maps, owner mask, CSR, both vectors, and for
      restrict the scratch written and read back), i.e. a buffer of half
      those bytes copied once.

No threshold is set: the ratios to (a) and (b) are reported as measured.
``create`` (maps to the host, plan, tables back) is timed once with a host
clock around a synchronise.

  python tools/bench_transfer.py [--shapes quad,hex] [--small] [--out FILE]
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
from spectralelementmethod_amd import _lib, meshgen  # noqa: E402
from spectralelementmethod_amd.transfer import Transfer  # noqa: E402


def steady(fn, window):
    """Seconds per call of fn() in steady state (device events)."""
    for _ in range(5):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    k = max(10, int(window * 1e3 / max(ev[0].elapsed_time(ev[1]), 1e-3)))
    ev[0].record()
    for _ in range(k):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3 / k, k


def maps(name, small, p):
    """(e2n, n_node) of the structured benchmark mesh at order p."""
    if name == "quad":
        ne = 128 if small else 1024
        N = ne * p + 1
        return meshgen._element_map(ne, ne, p, N), N * N
    if name == "hex":
        ne = 9 if small else 27
        N = ne * p + 1
        return meshgen._element_map3(ne, ne, ne, p, N, N), N ** 3
    raise ValueError("unknown shape %r" % name)


def interp_matrix(p_from, p_to):
    """J [n_to, n_from] from the library's own tables."""
    lib = _lib.load()
    tab = []
    for p in (p_from, p_to):
        x, b, w = (np.zeros(p + 1) for _ in range(3))
        _lib.check(lib.sem_gll_table(p, _lib.dptr(x), _lib.dptr(b), _lib.dptr(w)))
        tab.append((x, b))
    J = np.zeros((p_to + 1, p_from + 1))
    _lib.check(lib.sem_lagrange_eval(p_from + 1, _lib.dptr(tab[0][0]), _lib.dptr(tab[0][1]),
                                     p_to + 1, _lib.dptr(tab[1][0]), _lib.dptr(J)))
    return J


def run(name, small, window, p_from=4, p_to=8):
    ef, nnf = maps(name, small, p_from)
    et, nnt = maps(name, small, p_to)
    nd = ef.ndim - 1
    E, lf, lt = ef.shape[0], (p_from + 1) ** nd, (p_to + 1) ** nd
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = Transfer(ef, nnf, et, nnt, device=dev)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    info = tr.info()
    kw = dict(dtype=torch.float64, device=dev)
    u, r = torch.randn(nnf, **kw), torch.randn(nnt, **kw)
    u_to, r_from = torch.zeros(nnt, **kw), torch.zeros(nnf, **kw)
    t_pro, k_pro = steady(lambda: tr.prolong(u, out=u_to), window)
    t_res, k_res = steady(lambda: tr.restrict(r, out=r_from), window)

    # (a) the same operation composed from torch calls
    J = torch.from_numpy(interp_matrix(p_from, p_to)).to(dev)
    idx_f = torch.from_numpy(ef.reshape(-1).astype(np.int64)).to(dev)
    idx_t = torch.from_numpy(et.reshape(-1).astype(np.int64)).to(dev)
    _, first = np.unique(et.reshape(-1), return_index=True)
    own_pos = torch.from_numpy(np.sort(first)).to(dev)
    own_node = idx_t[own_pos]
    own_f = torch.zeros(E * lt, **kw)
    own_f[own_pos] = 1.0
    eq_p = "ai,bj,eij->eab" if nd == 2 else "ai,bj,ck,eijk->eabc"
    eq_r = "ai,bj,eab->eij" if nd == 2 else "ai,bj,ck,eabc->eijk"
    mats = [J] * nd
    shape_f, shape_t = (E,) + (p_from + 1,) * nd, (E,) + (p_to + 1,) * nd
    a_to, a_from = torch.zeros(nnt, **kw), torch.zeros(nnf, **kw)

    def torch_prolong():
        loc = torch.einsum(eq_p, *mats, u[idx_f].reshape(shape_f)).reshape(-1)
        a_to.index_copy_(0, own_node, loc[own_pos])

    def torch_restrict():
        loc = (r[idx_t] * own_f).reshape(shape_t)
        a_from.zero_()
        a_from.index_add_(0, idx_f, torch.einsum(eq_r, *mats, loc).reshape(-1))
    t_tpro, _ = steady(torch_prolong, window)
    t_tres, _ = steady(torch_restrict, window)
    err_p = float((a_to - u_to).norm() / u_to.norm())
    err_r = float((a_from - r_from).norm() / r_from.norm())
    del idx_f, idx_t, own_pos, own_node, own_f, a_to, a_from

    # (b) a copy of the bytes each call must move
    b_pro = E * lf * 4 + nnf * 8 + E * lt * (4 + 1) + nnt * 8
    b_res = E * lt * (4 + 1) + nnt * 8 + 2 * E * lf * 8 + (nnf + 1) * 4 + E * lf * 4 + nnf * 8
    copies = {}
    for key, b in (("prolong", b_pro), ("restrict", b_res)):
        src = torch.empty(b // 16, **kw)
        dst = torch.empty_like(src)
        copies[key], _ = steady(lambda: dst.copy_(src), window)
        del src, dst
    rec = dict(shape=name, small=bool(small), ndim=nd, p_from=p_from, p_to=p_to, n_elem=E,
               nodes_from=nnf, nodes_to=nnt, create_s=t_create,
               scratch_bytes=info["scratch_bytes"], max_contributions=info["max_contributions"],
               prolong_s=t_pro, prolong_repeats=k_pro, prolong_bytes=b_pro,
               prolong_bytes_per_s=b_pro / t_pro, prolong_torch_s=t_tpro,
               prolong_copy_s=copies["prolong"], prolong_speedup_over_torch=t_tpro / t_pro,
               prolong_time_over_copy=t_pro / copies["prolong"],
               prolong_torch_rel_diff=err_p,
               restrict_s=t_res, restrict_repeats=k_res, restrict_bytes=b_res,
               restrict_bytes_per_s=b_res / t_res, restrict_torch_s=t_tres,
               restrict_copy_s=copies["restrict"], restrict_speedup_over_torch=t_tres / t_res,
               restrict_time_over_copy=t_res / copies["restrict"],
               restrict_torch_rel_diff=err_r)
    print(json.dumps(rec), flush=True)
    tr.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="quad,hex")
    ap.add_argument("--small", action="store_true", help="reduced shapes (a quick check)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of steady state per call")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transfer needs a HIP device")
    recs = [run(s, a.small, a.window) for s in a.shapes.split(",") if s]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(results=recs), f, indent=1)


if __name__ == "__main__":
    main()
