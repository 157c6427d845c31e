// Host-side planning of the volume kernels (include/sem_hip.h, "Volume"):
// validation of the sizes and of the element map, and the CSR of the
// (element, local) entries of every node, rows ascending.  Pure C++, no HIP:
// csrc/sem_volume_plan.cpp links alone into tools/volume_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sem_hip.h"

namespace semvolume {

// SEM_OK, or SEM_E_INVALID for ndim not 2 or 3, p < 1, n_elem < 0, n_node
// outside [0, 2^32], n_elem * n^ndim >= 2^31; SEM_E_NOTIMPL for p > 16.
int check_sizes(int ndim, int p, int64_t n_elem, int64_t n_node);

// SEM_OK, or SEM_E_INVALID naming the first entry of map [n_entries] that is
// >= n_node (or a NULL map with entries).
int check_map(const uint32_t* map, int64_t n_entries, int64_t n_node);

struct Plan {
  // entry[ptr[g] .. ptr[g + 1]) are the entries (element * nloc + local) of
  // e2n equal to g, ascending; a node no element references has an empty row
  std::vector<int32_t> ptr;    // [n_node + 1]
  std::vector<int32_t> entry;  // [n_entries]
  int64_t n_referenced = 0;    // nodes with a row
  int64_t max_row = 0;
};
// The map must have passed check_sizes and check_map.
void plan(int64_t n_entries, const uint32_t* e2n, int64_t n_node, Plan& out);

}  // namespace semvolume
