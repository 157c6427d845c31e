// Host-side planning of the boundary-face kernels (include/sem_hip.h,
// "Faces"): validation of the (element, face) list, the face-order index
// tables and the node -> (face, q) CSR of the Neumann assembly.  Pure C++, no
// HIP: csrc/sem_faces_plan.cpp links alone into tools/faces_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sem_hip.h"

namespace semfaces {

// SEM_OK, or SEM_E_INVALID naming the first pair with an element id outside
// [0, n_elem) or a face >= 2 * ndim (also: ndim not 2 or 3, p < 1, negative
// counts, n_faces * n^(ndim-1) >= 2^31); SEM_E_NOTIMPL for p > 16.
int check(int ndim, int p, int64_t n_elem, int64_t n_faces, const int32_t* elem,
          const uint8_t* face);

// table[face * nf + q]: element-local lexicographic index (xi0 slowest) of
// face node q, in the face order of include/sem_hip.h; [2 * ndim][nf].
void index_tables(int ndim, int n, std::vector<int32_t>& table);

// From the global node id of every (face, q) entry ([n_entries], entry =
// face * nf + q): the sorted distinct nodes, and per node its entries in
// ascending order (CSR).  Returns the longest row.
struct NodeCsr {
  std::vector<uint32_t> node;  // [n_distinct], ascending
  std::vector<int32_t> ptr;    // [n_distinct + 1]
  std::vector<int32_t> entry;  // [n_entries]
  int64_t max_row = 0;
};
void node_csr(const uint32_t* node_of_entry, int64_t n_entries, NodeCsr& csr);

}  // namespace semfaces
