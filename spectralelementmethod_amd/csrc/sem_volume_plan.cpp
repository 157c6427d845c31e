// Host-side planning of the volume kernels: see sem_volume_plan.h.
// No HIP header is included here (as sem_transfer_plan.cpp).
#include "sem_volume_plan.h"

#include <algorithm>
#include <limits>
#include <string>

#include "sem_error.h"

namespace semvolume {

using sem::fail;

int check_sizes(int ndim, int p, int64_t n_elem, int64_t n_node) {
  if (ndim != 2 && ndim != 3) return fail(SEM_E_INVALID, "volume: ndim must be 2 or 3");
  if (p < 1) return fail(SEM_E_INVALID, "volume: p must be >= 1");
  if (p > 16) return fail(SEM_E_NOTIMPL, "volume: p <= 16");
  if (n_elem < 0) return fail(SEM_E_INVALID, "volume: n_elem must be >= 0");
  if (n_node < 0 || n_node > ((int64_t)1 << 32))
    return fail(SEM_E_INVALID, "volume: n_node must be in [0, 2^32]");
  int64_t nloc = 1;
  for (int i = 0; i < ndim; ++i) nloc *= p + 1;
  if (n_elem > std::numeric_limits<int32_t>::max() / nloc)
    return fail(SEM_E_INVALID, "volume: n_elem * n^ndim must be < 2^31");
  return SEM_OK;
}

int check_map(const uint32_t* map, int64_t n_entries, int64_t n_node) {
  if (n_entries > 0 && !map) return fail(SEM_E_INVALID, "volume: NULL element map");
  for (int64_t k = 0; k < n_entries; ++k)
    if ((int64_t)map[k] >= n_node)
      return fail(SEM_E_INVALID, "volume: map entry " + std::to_string(k) + ": node id " +
                                     std::to_string(map[k]) +
                                     " >= n_node = " + std::to_string(n_node));
  return SEM_OK;
}

void plan(int64_t n_entries, const uint32_t* e2n, int64_t n_node, Plan& out) {
  // counting sort of the entries by node: each row stays ascending
  out.ptr.assign((size_t)n_node + 1, 0);
  for (int64_t k = 0; k < n_entries; ++k) ++out.ptr[(size_t)e2n[k] + 1];
  out.max_row = 0;
  out.n_referenced = 0;
  for (int64_t g = 0; g < n_node; ++g) {
    const int32_t len = out.ptr[(size_t)g + 1];
    out.max_row = std::max<int64_t>(out.max_row, len);
    out.n_referenced += len > 0;
    out.ptr[(size_t)g + 1] += out.ptr[(size_t)g];
  }
  out.entry.assign((size_t)n_entries, 0);
  std::vector<int32_t> fill(out.ptr.begin(), out.ptr.end() - 1);
  for (int64_t k = 0; k < n_entries; ++k) out.entry[(size_t)fill[e2n[k]]++] = (int32_t)k;
}

}  // namespace semvolume
