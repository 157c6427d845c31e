// Host-side planning of the order-transfer kernels: see sem_transfer_plan.h.
// No HIP header is included here (as sem_faces_plan.cpp).
#include "sem_transfer_plan.h"

#include <algorithm>
#include <limits>
#include <string>

#include "sem_error.h"

namespace semtransfer {

using sem::fail;

namespace {

int64_t ipow(int n, int d) {
  int64_t r = 1;
  for (int i = 0; i < d; ++i) r *= n;
  return r;
}

}  // namespace

int check_sizes(int ndim, int p_from, int p_to, int64_t n_elem, int64_t n_node_from,
                int64_t n_node_to) {
  if (ndim != 2 && ndim != 3) return fail(SEM_E_INVALID, "transfer: ndim must be 2 or 3");
  if (p_from < 1 || p_to < 1) return fail(SEM_E_INVALID, "transfer: orders must be >= 1");
  if (p_from > 16 || p_to > 16) return fail(SEM_E_NOTIMPL, "transfer: orders <= 16");
  if (n_elem < 0) return fail(SEM_E_INVALID, "transfer: n_elem must be >= 0");
  const int64_t id_max = (int64_t)1 << 32;
  if (n_node_from < 0 || n_node_from > id_max || n_node_to < 0 || n_node_to > id_max)
    return fail(SEM_E_INVALID, "transfer: node counts must be in [0, 2^32]");
  const int64_t lim = std::numeric_limits<int32_t>::max();
  if (n_elem > lim / ipow(p_from + 1, ndim) || n_elem > lim / ipow(p_to + 1, ndim))
    return fail(SEM_E_INVALID, "transfer: n_elem * n^ndim must be < 2^31 on both sides");
  return SEM_OK;
}

int check_map(const char* side, const uint32_t* map, int64_t n_entries, int64_t n_node) {
  if (n_entries > 0 && !map)
    return fail(SEM_E_INVALID, std::string("transfer: NULL \"") + side + "\" map");
  for (int64_t k = 0; k < n_entries; ++k)
    if ((int64_t)map[k] >= n_node)
      return fail(SEM_E_INVALID, std::string("transfer: \"") + side + "\" map entry " +
                                     std::to_string(k) + ": node id " + std::to_string(map[k]) +
                                     " >= n_node = " + std::to_string(n_node));
  return SEM_OK;
}

int interp_matrix(int p_from, int p_to, std::vector<double>& J, std::vector<double>& Jt) {
  const int nf = p_from + 1, nt = p_to + 1;
  std::vector<double> xf(nf), bf(nf), wf(nf), xt(nt), bt(nt), wt(nt);
  int rc = sem_gll_table(p_from, xf.data(), bf.data(), wf.data());
  if (rc != SEM_OK) return rc;
  rc = sem_gll_table(p_to, xt.data(), bt.data(), wt.data());
  if (rc != SEM_OK) return rc;
  J.assign((size_t)nt * nf, 0.0);
  rc = sem_lagrange_eval(nf, xf.data(), bf.data(), nt, xt.data(), J.data());
  if (rc != SEM_OK) return rc;
  Jt.assign((size_t)nf * nt, 0.0);
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nf; ++j) Jt[(size_t)j * nt + i] = J[(size_t)i * nf + j];
  return SEM_OK;
}

void plan(int64_t n_entries_from, const uint32_t* e2n_from, int64_t n_node_from,
          int64_t n_entries_to, const uint32_t* e2n_to, int64_t n_node_to, Plan& out) {
  // owner: the first entry in ascending (element, local) order to name a node
  std::vector<bool> seen((size_t)n_node_to, false);
  out.owner.assign((size_t)n_entries_to, 0);
  out.n_owned = 0;
  for (int64_t k = 0; k < n_entries_to; ++k) {
    const uint32_t g = e2n_to[k];
    if (!seen[g]) {
      seen[g] = true;
      out.owner[(size_t)k] = 1;
      ++out.n_owned;
    }
  }
  // counting sort of the "from" entries by node: each row stays ascending
  out.ptr.assign((size_t)n_node_from + 1, 0);
  for (int64_t k = 0; k < n_entries_from; ++k) ++out.ptr[(size_t)e2n_from[k] + 1];
  out.max_row = 0;
  for (int64_t g = 0; g < n_node_from; ++g) {
    out.max_row = std::max<int64_t>(out.max_row, out.ptr[(size_t)g + 1]);
    out.ptr[(size_t)g + 1] += out.ptr[(size_t)g];
  }
  out.entry.assign((size_t)n_entries_from, 0);
  std::vector<int32_t> fill(out.ptr.begin(), out.ptr.end() - 1);
  for (int64_t k = 0; k < n_entries_from; ++k) out.entry[(size_t)fill[e2n_from[k]]++] = (int32_t)k;
}

}  // namespace semtransfer
