// Host-side planning of the order-transfer kernels (include/sem_hip.h,
// "Transfer"): validation of the two element maps, the 1-D interpolation
// matrix J and its transpose, the owner mask of the "to" map and the CSR of
// the (element, local) contributions of every "from" node.  Pure C++, no HIP:
// csrc/sem_transfer_plan.cpp links with the host basis tables
// (csrc/sem_basis.cpp) into tools/transfer_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sem_hip.h"

namespace semtransfer {

// SEM_OK, or SEM_E_INVALID for ndim not 2 or 3, an order < 1, n_elem < 0, a
// node count outside [0, 2^32], n_elem * n^ndim >= 2^31 on either side;
// SEM_E_NOTIMPL for an order > 16.
int check_sizes(int ndim, int p_from, int p_to, int64_t n_elem, int64_t n_node_from,
                int64_t n_node_to);

// SEM_OK, or SEM_E_INVALID naming the first entry of map [n_entries] that is
// >= n_node (`side` is "from" or "to" in the message).
int check_map(const char* side, const uint32_t* map, int64_t n_entries, int64_t n_node);

// J [n_to][n_from], J[i][j] = l_j^from(x_i^to), from sem_gll_table and
// sem_lagrange_eval (a coincident node gives exactly 0 or 1), and Jt
// [n_from][n_to] its transpose.
int interp_matrix(int p_from, int p_to, std::vector<double>& J, std::vector<double>& Jt);

struct Plan {
  // [n_elem * nloc_to]: 1 where the entry is the lowest (element, local) pair
  // that references its "to" node
  std::vector<uint8_t> owner;
  int64_t n_owned = 0;
  // rows of the "from" nodes: entry[ptr[g] .. ptr[g + 1]) are the entries
  // (element * nloc_from + local) of e2n_from equal to g, ascending
  std::vector<int32_t> ptr;    // [n_node_from + 1]
  std::vector<int32_t> entry;  // [n_elem * nloc_from]
  int64_t max_row = 0;
};
// The maps must have passed check_sizes and check_map.
void plan(int64_t n_entries_from, const uint32_t* e2n_from, int64_t n_node_from,
          int64_t n_entries_to, const uint32_t* e2n_to, int64_t n_node_to, Plan& out);

}  // namespace semtransfer
