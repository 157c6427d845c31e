// Host-side planning of the p-multigrid preconditioner (include/sem_hip.h,
// "p-multigrid"): the ladder of orders, the subsampled element map of a
// coarser level with its compacted node ids, the coarse Dirichlet mask, the
// Chebyshev coefficients of a smoother, the launch counts of the cycle and
// the validation of sem_mg_create's arguments.  Pure C++, no HIP:
// csrc/sem_mg_plan.cpp links with csrc/sem_basis.cpp (the error message) into
// tools/mg_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sem_hip.h"

namespace semmg {

// The default ladder of order p: p, then the quotient by the smallest prime
// factor, down to 1 (16 8 4 2 1; 12 6 3 1; 9 3 1; 7 1; 1).  SEM_E_INVALID for
// p < 1, SEM_E_NOTIMPL for p > 16.
int default_ladder(int p, std::vector<int>& out);

// SEM_OK when ladder[0..n) is a divisor chain: 1 <= n, every order in 1..16,
// strictly descending, each order a divisor of its predecessor.
int check_ladder(const int* ladder, int n);

// SEM_OK, or SEM_E_INVALID for ndim not 2 or 3, orders that are no divisor
// pair (1 <= p_coarse < p_fine <= 16, p_fine % p_coarse == 0), n_elem < 0, a
// node count outside [0, 2^32], n_elem * (p_fine + 1)^ndim >= 2^31.
int check_coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, int64_t n_node_fine);

// The coarse level of a fine map [n_elem][(p_fine + 1)^ndim]:
// e2n_coarse[e][i, j(, k)] = id of e2n_fine[e][s i, s j(, s k)], s = p_fine /
// p_coarse, the kept fine ids compacted in ascending order; keep[c] is the
// fine id of coarse node c.  SEM_E_INVALID for a fine id >= n_node_fine.
int coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* e2n_fine,
            int64_t n_node_fine, std::vector<uint32_t>& e2n_coarse, std::vector<uint32_t>& keep);

// mask_coarse [keep.size()]: a coarse node is fixed iff in some element that
// contains it every fine node of its entity is fixed; the entity is, per
// local axis, the same end of the element where the coarse index is an end
// (0 or p_coarse) and the open range 1 .. p_fine - 1 where it is not (a
// vertex, an open edge, an open face or the open interior).
int coarse_mask(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* e2n_fine,
                int64_t n_node_fine, const uint8_t* mask_fine, const uint32_t* e2n_coarse,
                int64_t n_node_coarse, std::vector<uint8_t>& mask_coarse);

// Chebyshev iteration of the given degree for D^-1 A on [lambda_max / ratio,
// lambda_max]: d_0 = inv_theta D^-1 r; step j = 1 .. degree - 1:
// d_j = c1[j] d_{j-1} + c2[j] D^-1 r_j (c1[0] = 0, c2[0] = inv_theta).
// SEM_E_INVALID for degree < 1, lambda_max not finite or <= 0, ratio not
// finite or <= 1.
struct Cheb {
  double inv_theta = 0.0;
  std::vector<double> c1, c2;  // [degree]
};
int chebyshev(int degree, double lambda_max, double ratio, Cheb& out);

// Operator actions and vector-pass launches of this unit per level and
// V-cycle: 2 k on a smoothed level, coarse_degree - 1 on the coarsest.
void cycle_counts(int n_levels, int smooth_degree, int coarse_degree, std::vector<int>& actions,
                  std::vector<int>& passes);

// The arguments of sem_mg_create that need no device: level count, degrees,
// ratios, the lambda_max of every level, NULL arrays, the sizes of adjacent
// levels against their transfer (ndof[l] = the "to" node count of transfer
// l, ndof[l + 1] its "from" node count).
int check_create(int n_levels, const void* const* ctxs, const void* const* transfers,
                 const void* const* masks, const double* lambda_max, int smooth_degree,
                 int coarse_degree, double smooth_ratio, double coarse_ratio);
int check_level_sizes(int level, int64_t ndof_fine, int64_t ndof_coarse, int64_t transfer_from,
                      int64_t transfer_to);

}  // namespace semmg
