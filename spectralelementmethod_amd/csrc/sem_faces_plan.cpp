// Host-side planning of the boundary-face kernels: see sem_faces_plan.h.
// No HIP header is included here (as sem_plan.cpp).
#include "sem_faces_plan.h"

#include <algorithm>
#include <limits>
#include <numeric>
#include <string>

#include "sem_error.h"

namespace semfaces {

using sem::fail;

int check(int ndim, int p, int64_t n_elem, int64_t n_faces, const int32_t* elem,
          const uint8_t* face) {
  if (ndim != 2 && ndim != 3) return fail(SEM_E_INVALID, "faces: ndim must be 2 or 3");
  if (p < 1) return fail(SEM_E_INVALID, "faces: p must be >= 1");
  if (p > 16) return fail(SEM_E_NOTIMPL, "faces: p <= 16");
  if (n_elem < 1 || n_elem > (int64_t)std::numeric_limits<int32_t>::max())
    return fail(SEM_E_INVALID, "faces: n_elem must be in [1, 2^31)");
  if (n_faces < 0) return fail(SEM_E_INVALID, "faces: n_faces must be >= 0");
  const int64_t nf = ndim == 2 ? p + 1 : (int64_t)(p + 1) * (p + 1);
  if (n_faces > (int64_t)std::numeric_limits<int32_t>::max() / nf)
    return fail(SEM_E_INVALID, "faces: n_faces * nodes per face must be < 2^31");
  if (n_faces > 0 && (!elem || !face)) return fail(SEM_E_INVALID, "faces: NULL element/face list");
  for (int64_t f = 0; f < n_faces; ++f) {
    if (elem[f] < 0 || (int64_t)elem[f] >= n_elem)
      return fail(SEM_E_INVALID, "faces: entry " + std::to_string(f) + ": element id " +
                                     std::to_string(elem[f]) + " outside [0, n_elem)");
    if (face[f] >= 2 * ndim)
      return fail(SEM_E_INVALID, "faces: entry " + std::to_string(f) + ": face " +
                                     std::to_string((int)face[f]) + " >= 2 * ndim");
  }
  return SEM_OK;
}

void index_tables(int ndim, int n, std::vector<int32_t>& table) {
  const int nf = ndim == 2 ? n : n * n;
  table.assign((size_t)2 * ndim * nf, 0);
  for (int fc = 0; fc < 2 * ndim; ++fc) {
    const int ax = fc / 2, side = fc % 2;
    const int fixed = side ? n - 1 : 0;
    for (int q = 0; q < nf; ++q) {
      int a[3] = {0, 0, 0};
      a[ax] = fixed;
      if (ndim == 2) {
        // counter-clockwise round the element: faces 0 and 3 run backwards
        a[1 - ax] = (fc == 0 || fc == 3) ? n - 1 - q : q;
        table[(size_t)fc * nf + q] = a[0] * n + a[1];
      } else {
        const int q0 = q / n, q1 = q % n;
        const int b = (ax + 1) % 3, c = (ax + 2) % 3;
        // side 1: face axes (ax+1, ax+2); side 0: the reverse order
        a[side ? b : c] = q0;
        a[side ? c : b] = q1;
        table[(size_t)fc * nf + q] = (a[0] * n + a[1]) * n + a[2];
      }
    }
  }
}

void node_csr(const uint32_t* node_of_entry, int64_t n_entries, NodeCsr& csr) {
  csr.node.clear();
  csr.ptr.assign(1, 0);
  csr.entry.resize((size_t)n_entries);
  csr.max_row = 0;
  std::iota(csr.entry.begin(), csr.entry.end(), 0);
  // stable: entries of one node keep their ascending (face, q) order
  std::stable_sort(csr.entry.begin(), csr.entry.end(), [&](int32_t a, int32_t b) {
    return node_of_entry[a] < node_of_entry[b];
  });
  for (int64_t k = 0; k < n_entries; ++k) {
    const uint32_t nd = node_of_entry[csr.entry[k]];
    if (csr.node.empty() || csr.node.back() != nd) {
      if (!csr.node.empty()) csr.ptr.push_back((int32_t)k);
      csr.node.push_back(nd);
    }
  }
  if (!csr.node.empty()) csr.ptr.push_back((int32_t)n_entries);
  for (size_t r = 0; r + 1 < csr.ptr.size(); ++r)
    csr.max_row = std::max<int64_t>(csr.max_row, csr.ptr[r + 1] - csr.ptr[r]);
}

}  // namespace semfaces
