// Host-side planning of the p-multigrid preconditioner: see sem_mg_plan.h.
// No HIP header is included here (as sem_transfer_plan.cpp).
#include "sem_mg_plan.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "sem_error.h"

namespace semmg {

using sem::fail;

namespace {

int64_t ipow(int n, int d) {
  int64_t r = 1;
  for (int i = 0; i < d; ++i) r *= n;
  return r;
}

}  // namespace

int default_ladder(int p, std::vector<int>& out) {
  out.clear();
  if (p < 1) return fail(SEM_E_INVALID, "multigrid: the order must be >= 1");
  if (p > 16) return fail(SEM_E_NOTIMPL, "multigrid: orders <= 16");
  out.push_back(p);
  while (p > 1) {
    int f = 2;
    while (p % f) ++f;
    p /= f;
    out.push_back(p);
  }
  return SEM_OK;
}

int check_ladder(const int* ladder, int n) {
  if (!ladder || n < 1) return fail(SEM_E_INVALID, "multigrid: the ladder needs at least one order");
  for (int l = 0; l < n; ++l) {
    if (ladder[l] < 1 || ladder[l] > 16)
      return fail(SEM_E_INVALID, "multigrid: ladder order " + std::to_string(ladder[l]) +
                                     " is outside 1..16");
    if (l && (ladder[l] >= ladder[l - 1] || ladder[l - 1] % ladder[l]))
      return fail(SEM_E_INVALID, "multigrid: the ladder must be a descending divisor chain, " +
                                     std::to_string(ladder[l]) + " does not divide " +
                                     std::to_string(ladder[l - 1]));
  }
  return SEM_OK;
}

int check_coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, int64_t n_node_fine) {
  if (ndim != 2 && ndim != 3) return fail(SEM_E_INVALID, "multigrid: ndim must be 2 or 3");
  const int pair[2] = {p_fine, p_coarse};
  int rc = check_ladder(pair, 2);
  if (rc != SEM_OK) return rc;
  if (n_elem < 0) return fail(SEM_E_INVALID, "multigrid: n_elem must be >= 0");
  if (n_node_fine < 0 || n_node_fine > ((int64_t)1 << 32))
    return fail(SEM_E_INVALID, "multigrid: node counts must be in [0, 2^32]");
  if (n_elem > std::numeric_limits<int32_t>::max() / ipow(p_fine + 1, ndim))
    return fail(SEM_E_INVALID, "multigrid: n_elem * n^ndim must be < 2^31");
  return SEM_OK;
}

int coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* e2n_fine,
            int64_t n_node_fine, std::vector<uint32_t>& e2n_coarse, std::vector<uint32_t>& keep) {
  int rc = check_coarsen(ndim, p_fine, p_coarse, n_elem, n_node_fine);
  if (rc != SEM_OK) return rc;
  if (n_elem > 0 && !e2n_fine) return fail(SEM_E_INVALID, "multigrid: NULL fine map");
  const int nf = p_fine + 1, nc = p_coarse + 1, s = p_fine / p_coarse;
  const int64_t lf = ipow(nf, ndim), lc = ipow(nc, ndim);
  for (int64_t k = 0; k < n_elem * lf; ++k)
    if ((int64_t)e2n_fine[k] >= n_node_fine)
      return fail(SEM_E_INVALID, "multigrid: fine map entry " + std::to_string(k) + ": node id " +
                                     std::to_string(e2n_fine[k]) + " >= n_node = " +
                                     std::to_string(n_node_fine));
  e2n_coarse.assign((size_t)(n_elem * lc), 0);
  std::vector<uint8_t> kept((size_t)n_node_fine, 0);
  const int nk = ndim == 3 ? nc : 1;
  for (int64_t e = 0; e < n_elem; ++e)
    for (int i = 0; i < nc; ++i)
      for (int j = 0; j < nc; ++j)
        for (int k = 0; k < nk; ++k) {
          const int64_t fine = ndim == 3 ? ((int64_t)s * i * nf + s * j) * nf + s * k
                                         : (int64_t)s * i * nf + s * j;
          const int64_t coarse = ndim == 3 ? ((int64_t)i * nc + j) * nc + k : (int64_t)i * nc + j;
          const uint32_t g = e2n_fine[e * lf + fine];
          e2n_coarse[(size_t)(e * lc + coarse)] = g;  // the fine id for now
          kept[g] = 1;
        }
  // compact in ascending order of the fine id
  std::vector<uint32_t> new_id((size_t)n_node_fine, 0);
  keep.clear();
  for (int64_t g = 0; g < n_node_fine; ++g)
    if (kept[(size_t)g]) {
      new_id[(size_t)g] = (uint32_t)keep.size();
      keep.push_back((uint32_t)g);
    }
  for (auto& g : e2n_coarse) g = new_id[g];
  return SEM_OK;
}

int coarse_mask(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* e2n_fine,
                int64_t n_node_fine, const uint8_t* mask_fine, const uint32_t* e2n_coarse,
                int64_t n_node_coarse, std::vector<uint8_t>& mask_coarse) {
  int rc = check_coarsen(ndim, p_fine, p_coarse, n_elem, n_node_fine);
  if (rc != SEM_OK) return rc;
  if (n_node_coarse < 0 || n_node_coarse > n_node_fine)
    return fail(SEM_E_INVALID, "multigrid: the coarse level has more nodes than the fine one");
  if ((n_elem > 0 && (!e2n_fine || !e2n_coarse)) || (n_node_fine > 0 && !mask_fine))
    return fail(SEM_E_INVALID, "multigrid: NULL map or mask");
  const int nf = p_fine + 1, nc = p_coarse + 1;
  const int64_t lf = ipow(nf, ndim), lc = ipow(nc, ndim);
  for (int64_t k = 0; k < n_elem * lf; ++k)
    if ((int64_t)e2n_fine[k] >= n_node_fine)
      return fail(SEM_E_INVALID, "multigrid: fine map entry " + std::to_string(k) +
                                     " >= n_node = " + std::to_string(n_node_fine));
  for (int64_t k = 0; k < n_elem * lc; ++k)
    if ((int64_t)e2n_coarse[k] >= n_node_coarse)
      return fail(SEM_E_INVALID, "multigrid: coarse map entry " + std::to_string(k) +
                                     " >= n_node = " + std::to_string(n_node_coarse));
  mask_coarse.assign((size_t)n_node_coarse, 0);
  // class of a local index along one axis: 0 the low end, 1 open, 2 the high end
  auto cls = [](int i, int p) { return i == 0 ? 0 : i == p ? 2 : 1; };
  const int nkf = ndim == 3 ? nf : 1, nkc = ndim == 3 ? nc : 1;
  for (int64_t e = 0; e < n_elem; ++e) {
    // all_fixed[class triple]: every fine node of that entity of e is fixed;
    // an empty entity (p_fine = 1 has no open range; not reached: p_fine >= 2)
    bool all_fixed[27];
    std::fill(all_fixed, all_fixed + 27, true);
    for (int i = 0; i < nf; ++i)
      for (int j = 0; j < nf; ++j)
        for (int k = 0; k < nkf; ++k) {
          const int64_t loc = ndim == 3 ? ((int64_t)i * nf + j) * nf + k : (int64_t)i * nf + j;
          const int c = (cls(i, p_fine) * 3 + cls(j, p_fine)) * 3 + (ndim == 3 ? cls(k, p_fine) : 0);
          if (!mask_fine[e2n_fine[e * lf + loc]]) all_fixed[c] = false;
        }
    for (int i = 0; i < nc; ++i)
      for (int j = 0; j < nc; ++j)
        for (int k = 0; k < nkc; ++k) {
          const int64_t loc = ndim == 3 ? ((int64_t)i * nc + j) * nc + k : (int64_t)i * nc + j;
          const int c =
              (cls(i, p_coarse) * 3 + cls(j, p_coarse)) * 3 + (ndim == 3 ? cls(k, p_coarse) : 0);
          if (all_fixed[c]) mask_coarse[e2n_coarse[e * lc + loc]] = 1;
        }
  }
  return SEM_OK;
}

int chebyshev(int degree, double lambda_max, double ratio, Cheb& out) {
  if (degree < 1) return fail(SEM_E_INVALID, "multigrid: a Chebyshev degree must be >= 1");
  if (!std::isfinite(lambda_max) || lambda_max <= 0.0)
    return fail(SEM_E_INVALID, "multigrid: lambda_max must be finite and > 0");
  if (!std::isfinite(ratio) || ratio <= 1.0)
    return fail(SEM_E_INVALID, "multigrid: a smoothing ratio must be finite and > 1");
  const double a = lambda_max / ratio, b = lambda_max;
  const double theta = 0.5 * (b + a), delta = 0.5 * (b - a), sigma = theta / delta;
  out.inv_theta = 1.0 / theta;
  out.c1.assign((size_t)degree, 0.0);
  out.c2.assign((size_t)degree, 0.0);
  out.c2[0] = out.inv_theta;
  double rho = 1.0 / sigma;
  for (int j = 1; j < degree; ++j) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    out.c1[(size_t)j] = rho_new * rho;
    out.c2[(size_t)j] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
  return SEM_OK;
}

void cycle_counts(int n_levels, int smooth_degree, int coarse_degree, std::vector<int>& actions,
                  std::vector<int>& passes) {
  actions.assign((size_t)std::max(n_levels, 0), 0);
  passes.assign((size_t)std::max(n_levels, 0), 0);
  for (int l = 0; l < n_levels; ++l) {
    if (l == n_levels - 1) {  // Chebyshev from zero: the first step needs no action
      actions[(size_t)l] = coarse_degree - 1;
      passes[(size_t)l] = coarse_degree;
    } else {
      // pre-smoothing k - 1, residual 1, post-smoothing 1 + (k - 1)
      actions[(size_t)l] = 2 * smooth_degree;
      // k pre, the residual, the prolong-add, k post
      passes[(size_t)l] = 2 * smooth_degree + 2;
    }
  }
}

int check_create(int n_levels, const void* const* ctxs, const void* const* transfers,
                 const void* const* masks, const double* lambda_max, int smooth_degree,
                 int coarse_degree, double smooth_ratio, double coarse_ratio) {
  if (n_levels < 1 || n_levels > 16)
    return fail(SEM_E_INVALID, "sem_mg_create: n_levels must be in 1..16");
  if (!ctxs || !masks || !lambda_max || (n_levels > 1 && !transfers))
    return fail(SEM_E_INVALID, "sem_mg_create: NULL array");
  for (int l = 0; l < n_levels; ++l) {
    if (!ctxs[l] || !masks[l])
      return fail(SEM_E_INVALID, "sem_mg_create: NULL context or mask of level " +
                                     std::to_string(l));
    if (l + 1 < n_levels && !transfers[l])
      return fail(SEM_E_INVALID, "sem_mg_create: NULL transfer of level " + std::to_string(l));
    Cheb c;
    const bool last = l == n_levels - 1;
    int rc = chebyshev(last ? coarse_degree : smooth_degree, lambda_max[l],
                       last ? coarse_ratio : smooth_ratio, c);
    if (rc != SEM_OK) return rc;
  }
  return SEM_OK;
}

int check_level_sizes(int level, int64_t ndof_fine, int64_t ndof_coarse, int64_t transfer_from,
                      int64_t transfer_to) {
  if (ndof_fine != transfer_to || ndof_coarse != transfer_from)
    return fail(SEM_E_INVALID, "sem_mg_create: transfer " + std::to_string(level) + " maps " +
                                   std::to_string(transfer_from) + " -> " +
                                   std::to_string(transfer_to) + " nodes, levels " +
                                   std::to_string(level + 1) + " and " + std::to_string(level) +
                                   " have " + std::to_string(ndof_coarse) + " and " +
                                   std::to_string(ndof_fine));
  return SEM_OK;
}

}  // namespace semmg

extern "C" {

int sem_mg_ladder(int p, int* ladder, int capacity, int* n_levels) {
  if (!ladder || !n_levels || capacity < 0)
    return sem::fail(SEM_E_INVALID, "sem_mg_ladder: NULL argument");
  std::vector<int> v;
  int rc = semmg::default_ladder(p, v);
  if (rc != SEM_OK) return rc;
  if ((int)v.size() > capacity)
    return sem::fail(SEM_E_INVALID, "sem_mg_ladder: the ladder has " + std::to_string(v.size()) +
                                        " levels");
  std::copy(v.begin(), v.end(), ladder);
  *n_levels = (int)v.size();
  return SEM_OK;
}

int sem_mg_check_ladder(const int* ladder, int n_levels) {
  return semmg::check_ladder(ladder, n_levels);
}

int sem_mg_coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* h_e2n_fine,
                   int64_t n_node_fine, uint32_t* h_e2n_coarse, uint32_t* h_keep,
                   int64_t* n_node_coarse) {
  if (!h_e2n_coarse || !h_keep || !n_node_coarse)
    return sem::fail(SEM_E_INVALID, "sem_mg_coarsen: NULL output");
  std::vector<uint32_t> ec, keep;
  int rc = semmg::coarsen(ndim, p_fine, p_coarse, n_elem, h_e2n_fine, n_node_fine, ec, keep);
  if (rc != SEM_OK) return rc;
  std::copy(ec.begin(), ec.end(), h_e2n_coarse);
  std::copy(keep.begin(), keep.end(), h_keep);
  *n_node_coarse = (int64_t)keep.size();
  return SEM_OK;
}

int sem_mg_coarse_mask(int ndim, int p_fine, int p_coarse, int64_t n_elem,
                       const uint32_t* h_e2n_fine, int64_t n_node_fine, const uint8_t* h_mask_fine,
                       const uint32_t* h_e2n_coarse, int64_t n_node_coarse,
                       uint8_t* h_mask_coarse) {
  if (!h_mask_coarse && n_node_coarse > 0)
    return sem::fail(SEM_E_INVALID, "sem_mg_coarse_mask: NULL output");
  std::vector<uint8_t> m;
  int rc = semmg::coarse_mask(ndim, p_fine, p_coarse, n_elem, h_e2n_fine, n_node_fine,
                              h_mask_fine, h_e2n_coarse, n_node_coarse, m);
  if (rc != SEM_OK) return rc;
  std::copy(m.begin(), m.end(), h_mask_coarse);
  return SEM_OK;
}

}  // extern "C"
