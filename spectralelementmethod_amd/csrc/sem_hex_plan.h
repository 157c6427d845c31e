// Scatter plan of the hexahedral action: what the
// planner (host, once per map) and the element kernels (sem_hex.h,
// sem_hex_mfma.h) share, and the planner's interface.  Pure C++, no HIP:
// csrc/sem_hex_plan.cpp links alone into tools/hex_plan_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

namespace semh {

constexpr int HEX_MIN_N = 2;
constexpr int HEX_MAX_N = 17;  // p <= 16

// element slots per workgroup: as many n x n thread tiles as fit in 256 threads
constexpr int hex_slots(int n) { return 256 / (n * n) > 0 ? 256 / (n * n) : 1; }
constexpr int hex_threads(int n) { return (hex_slots(n) * n * n + 63) / 64 * 64; }
// boundary columns of an element: b or c on the element boundary
constexpr int hex_nbc(int n) { return 4 * (n - 1); }

// y-merge (three-block kernel, with the z-merge): the S slots of a
// workgroup form a Y x Z grid (Z = hex_grid_z(n) slots along xi2 per row, Y
// rows along xi1; Y = 1 when S is prime), and slot s hands its xi1 = 0 face
// to slot s - Z when that face IS slot s - Z's xi1 = n-1 face at every chain
// step (HEX_CF_YGIVE, checked by the planner), through the w2 block.  Columns
// a slot already handed over in the z-merge (c = 0) stay out of the y-merge
// on both sides.  p = 1 / 2 / 3 / 4 / 7: 8 x 8, 4 x 7, 4 x 4, 2 x 5, 2 x 2
// slots; on by default at p <= 3 (sem_hex.hip ctx_init), SEM_HEX_YMERGE=1 / 0
// in the environment forces it.
constexpr int hex_grid_z(int n) {
  int z = hex_slots(n);
  for (int y = 2; y * y <= hex_slots(n); ++y)
    if (hex_slots(n) % y == 0) z = hex_slots(n) / y;
  return z;
}

// boundary-column index of (b, c) in [0, 4(n-1)), -1 for an interior column
constexpr int hex_bcol(int n, int b, int c) {
  if (b == 0) return c;
  if (b == n - 1) return 3 * n - 4 + c;
  if (c == 0) return n + 2 * (b - 1);
  if (c == n - 1) return n + 2 * (b - 1) + 1;
  return -1;
}

// cflag[w * S + s], the flags of the sub-chain in slot s of workgroup w
enum : uint8_t {
  HEX_CF_HEAD = 1,   // the chain head face (row a = 0 of step 0) goes to its face slots
  HEX_CF_TAIL = 2,   // the tail face (row a = n-1 of the last step) likewise
  HEX_CF_ZGIVE = 4,  // z-merge: the xi2 = 0 face is slot s-1's xi2 = n-1 face at every
                     // step; column c = 0 is handed to it in LDS
  HEX_CF_YGIVE = 8,  // y-merge: the xi1 = 0 face is slot s-Z's xi1 = n-1 face likewise
};

// Slot space (HexLaunch::slot): column slots [pos][n][NBC], then from
// face_base on the face slots [n_wg * S][2][n^2] (side 0: head, 1: tail).
constexpr int64_t hex_col_slot(int n, int pos, int a, int bcol) {
  return ((int64_t)pos * n + a) * hex_nbc(n) + bcol;
}
constexpr int64_t hex_face_base(int n, int64_t n_pos) { return n_pos * n * hex_nbc(n); }
constexpr int64_t hex_face_slot(int n, int64_t face_base, int wg, int slot, int side, int bc) {
  return face_base + (int64_t)(wg * hex_slots(n) + slot) * 2 * (n * n) + side * (n * n) + bc;
}
constexpr int64_t hex_n_slot(int n, int64_t n_pos, int64_t n_wg) {
  return hex_face_base(n, n_pos) + n_wg * hex_slots(n) * 2 * (n * n);
}

}  // namespace semh

namespace semhexplan {

struct HexPlanOptions {
  bool zmerge = true, ymerge = false;  // HexState::zmerge / ymerge (sem_hex.hip ctx_init)
  int64_t resident = 0;                // workgroups of the element kernel resident on the device
  int chain_cap = 0;                   // > 0: the sub-chain length cap, whatever the rule says
  double chain_start = 1.0;            // a workgroup's fixed start, in element steps
};

// SEM_HEX_CHAIN -> chain_cap, SEM_HEX_CHAIN_START -> chain_start; the other
// fields as declared
HexPlanOptions hex_plan_options_from_env();

// The arrays set_map uploads (HexLaunch, k_hex_seam_sum, k_hex_zero) and the
// plan's scalars
struct HexPlan {
  std::vector<int> wg_off, wg_len, elist;
  std::vector<unsigned long long> cmask;
  std::vector<uint8_t> cflag;
  std::vector<uint32_t> seam_gid, seam_ptr, seam_idx, zero;
  int64_t n_slot = 0, face_base = 0, n_chains = 0, n_sub = 0, lc = 0, n_direct = 0;
};

// Plans the map e2n [n_elem][n][n][n] into an empty plan.  SEM_OK;
// SEM_E_INVALID for an entry >= n_node or a plan past the 32-bit index
// spaces; SEM_E_NOTIMPL for a non-conforming mesh.
int hex_plan_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
                 const HexPlanOptions& opt, HexPlan& plan);

// Template map (HexLaunch::ebase / tmpl): does every element's map equal its
// first node's id + the offsets of element 0?  Then tmpl [n^3] holds the
// offsets and ebase [n_elem] the first ids; otherwise both come back empty.
bool hex_template_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int n,
                      std::vector<int>& tmpl, std::vector<uint32_t>& ebase);

}  // namespace semhexplan
