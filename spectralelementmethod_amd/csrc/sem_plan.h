// The 2-D scatter plan: the vocabulary the host planner (sem_plan.cpp) and
// the kernels (sem_kernels.h) share, and the planner's interface.  No HIP:
// the planner is plain C++17 and is checked on the CPU (tools/plan_check.cpp,
// tests/test_plan_host.py).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/sem_hip.h"

namespace semk {

constexpr int WAVE = 64;
constexpr int epw_of(int n) { return WAVE / n; }  // elements per wavefront (column kernel)
// Groups per chain round = wavefronts per workgroup: 4.  At n = 17 the
// colour launches ran faster with 2-wave chains (p = 16 at 1e7 DOF: 0.165
// against 0.173 ms, profiles/r02/variants), but AUTO takes the seam plan
// there (one launch), on which 4-wave chains are ahead: 0.131
// against 0.136 ms (profiles/r02/final/chain_width).  SEM_CHAIN_WAVES
// (diagnostic builds) forces one value for every order.
#ifdef SEM_CHAIN_WAVES
constexpr int chain_waves_of(int) { return SEM_CHAIN_WAVES; }
#else
constexpr int chain_waves_of(int) { return 4; }
#endif

// packed map entry = gid | code << CODE_SHIFT
constexpr int CODE_SHIFT = 28;
constexpr uint32_t GID_MASK = (1u << CODE_SHIFT) - 1u;
constexpr uint32_t W_STORE = 0;   // first writer: y = v   (y += v in accumulate mode)
constexpr uint32_t W_RMW = 1;     // later writer: y += v (no concurrent writer)
constexpr uint32_t W_SKIP = 2;    // value merged into another lane / padding
constexpr uint32_t W_ATOMIC = 3;  // fallback
constexpr uint32_t W_MERGE = 4;   // add the next lane's value before writing
constexpr uint32_t W_CARRY = 8;   // add the value handed over by the previous group
// SKIP | CARRY: row n-1 entry whose value the same lane adds to row 0 of its
// next round (block layout): not written by this round
constexpr uint32_t W_ROWCARRY = W_SKIP | W_CARRY;

// 16-bit map: entries (gid - base) | code << 12, one 32-bit base per (slot, row)
constexpr uint32_t M16_OFF_MASK = 0xFFFu;
constexpr uint32_t M16_WIDE = 0xFFFFFFFFu;  // base[slot][0]: this group uses the 32-bit map
constexpr int M16_CODE_SHIFT = 12;

// orders with pattern-table (PAT) kernels (SEM_MAP_PATTERN_N, a bit per n;
// the host builds a table only for these): every order from n = 3 --
// measured faster at p = 4 / 6 / 8 / 10 / 12 / 14 / 16.  The
// pattern id sits in the top 4 bits of bases 1..map_pattern_id_rows(n): up to
// 16^id_rows patterns.
#ifndef SEM_MAP_PATTERN_N
#define SEM_MAP_PATTERN_N 0x3FFF8u
#endif
constexpr bool map_pattern_order(int n) {
  return n >= 3 && n <= 31 && ((SEM_MAP_PATTERN_N >> n) & 1u);
}
constexpr int map_pattern_id_rows(int n) { return n - 1 < 4 ? n - 1 : 4; }

constexpr int MAX_COLOURS = 8;  // + one trailing all-atomic class
// AUTO choice of the seam plan (Poisson column kernel), from the MI355X A/B
// of profiles/r02/seams2 (ms per action, colour launches -> seams; cpc =
// chains per colour): it wins where a colour launch is a few generations of
// resident workgroups or less -- p = 16 198^2 (cpc 1,633) 0.164 -> 0.134,
// p = 12 263^2 0.139 -> 0.114, p = 10 316^2 (1,296) 0.158 -> 0.128, p = 9
// 351^2 (1,297) 0.120 -> 0.113, p = 8 512^2 (2,342) 0.185 -> 0.179, 384^2
// (1,372) 0.107 -> 0.095, 128 x 1024 (1,171; one rank's strip of the
// 8-GPU split) 0.098 -> 0.089, 256^2 (585) 0.0635 -> 0.0477, p = 6 256^2
// (488) 0.040 -> 0.030, p = 4 395^2 (815) 0.045 -> 0.036 -- and loses where
// the colour launches stream many generations and the seams are a large
// share of the nodes: p = 8 1024^2 (9,365) 0.640 -> 0.668, p = 6 527^2
// (1,928) 0.118 -> 0.122, p = 4 790^2 (3,250) 0.113 -> 0.129, p = 2 1581^2
// 0.132 -> 0.161.
// Two DOFs per node (axisymmetric block, p = 6, profiles/r02/final/
// axisym_seams): 128^2 (cpc 114) 0.0441 -> 0.0236, 512^2 (cpc 1,820) 0.227
// -> 0.274 (the nodal kernel's seam instantiation runs 1 wave per SIMD
// instead of 2).
// AUTO of the block layout (sem_plan.cpp groups_blocks, 4 rounds): only
// where the mesh still has this many chains with it.  Measured on MI355X,
// ms per action, consecutive groups -> blocks (profiles/r03/sweep): the
// axisymmetric Stokes block at 512^2, p = 6 (1,920 block chains) 0.302 ->
// 0.257; Poisson p = 8 1024^2 (9,472) 0.684 -> 0.671, 395^2 (1,481) 0.106
// -> 0.107, p = 6 527^2 (1,980) 0.118 -> 0.122, p = 12 263^2 0.132 ->
// 0.151, p = 16 198^2 0.139 -> 0.188, 256^2 p = 8 0.046 -> 0.056.
inline int64_t block_min_chains(int n, int dpn) {
  (void)n;
  return dpn == 2 ? 1024 : 4096;
}
inline bool seam_auto(int n, int64_t chains_per_colour, int dpn = 1, bool blocks = false) {
  // block layout: the seams are a few % of the nodes (every R-th node row and
  // every 4*EPW-th column) -- 1024^2 p = 8: R = 4 seams 0.671, colours 0.692,
  // consecutive groups 0.684 ms (profiles/r03/blocks_ab.txt)
  if (blocks && dpn == 1) return true;
  if (dpn == 2) return chains_per_colour <= 512;
  // n = 7 (p = 6 at 527^2, 1,929 chains per colour; profiles/r04/p6/):
  // nodal seams 0.099-0.100 against nodal colours 0.106-0.111 and stored
  // colours 0.118-0.120 ms per action; stored seams 0.116-0.118
  return n >= 11 || chains_per_colour <= 1024 || ((n >= 9 || n == 7) && chains_per_colour <= 2400);
}

}  // namespace semk

namespace semplan {

// the planner's knobs (plan_options_from_env reads them from the environment)
struct PlanOptions {
  // SEM_CHAIN_ROUNDS: rounds of chain_waves_of(n) groups per chain.  Measured
  // on MI355X at p = 8, 10^6 elements: 1 round 0.79-0.81 ms, 2: 0.85, 4:
  // 0.88, 8: 0.97 (longer chains: fewer workgroups, lockstep).  Single-wave
  // chains (no workgroup barrier, register carry, next-group prefetch)
  // measured 0.90-0.95 ms (nodal) and 0.89-0.92 (stored): the prefetch
  // registers halve occupancy.  Not kept.
  int chain_rounds = 1;
  // SEM_BLOCK_ROUNDS: block layout (groups_blocks) with that many rounds
  // stacked along the lines, the node row between rounds carried in
  // registers; 0 or 1: off, -1: AUTO (build_plan, block_min_chains)
  int block_rounds = -1;
  // SEM_SEAM: seam plan (one launch + seam sums) 1 forced, 0 forbidden,
  // 2: AUTO (seam_auto, per dofs per node)
  int seam = 2;
  // SEM_PLAN: element-coloured fallback for orders that defeat the chain
  // patterns, 1 forced, 0 forbidden, -1: by the share of atomic groups
  int plan = -1;
  // SEM_MAP16 / SEM_MAP_PATTERNS = 0: keep the 32-bit map stream / the
  // per-group 16-bit entries (measured at p = 8, 10^6 elements: DESIGN.md §4.1)
  bool map16 = true;
  bool map_patterns = true;
  int64_t chain_swizzle_max = 2400;  // SEM_CHAIN_SWIZZLE_MAX (chain_swizzle)
};
PlanOptions plan_options_from_env();

// everything sem_set_map_shared uploads or records for one element map
struct Plan {
  std::vector<uint32_t> owner;  // first element referencing each node
  std::vector<uint32_t> mapP;   // [slot][r][lane] gid | code << CODE_SHIFT, launch order
  std::vector<int> epos;             // element -> packed position slot * epw + k
  std::vector<uint8_t> slot_fill;    // real elements in each slot (first lanes)
  std::vector<int64_t> colour_start;  // in chains, one launch per range
  std::vector<uint32_t> zero;         // nodes zeroed before an overwrite (sorted)
  int64_t n_atomic_groups = 0;
  int64_t n_slots = 0;
  bool conforming = true;
  int64_t n_rmw = 0;       // read-modify-write entries (a node's final value elsewhere)
  int rounds = 1;          // rounds of chain_waves_of(n) groups per chain
  bool blocks = false;     // block layout (groups_blocks)
  int64_t row_carries = 0;  // entries carried to the next round in registers
  bool round_sync = true;  // some chain read-modify-writes a node it stored in an earlier round
  bool ecol = false;       // element-coloured chains (build_plan_ecol)
  // seam plan: chains in element order, one launch; nodes written by several
  // chains go through per-colour slots summed by k_seam_sum
  bool seam = false;
  std::vector<uint8_t> chain_colour;  // [chain] in launch order
  std::vector<uint32_t> seam_gid;
  std::vector<uint16_t> seam_mask;  // colours | 0x100 prior
  int seam_ns = 0;
  bool seam_failed = false;  // inside plan_map: build_plan gave the seams up, plan again
  // 16-bit form of mapP (column kernel; build_map16, build_map_patterns)
  bool map16 = false;
  bool map_pat = false;  // m16 is a pattern table of n_map_pat blocks
  int64_t n_map_pat = 0;
  std::vector<uint16_t> m16;
  std::vector<uint32_t> mbase;  // [slot][r]
};

// Plans the scatter of one element map e2n [n_elem][n][n] for the column
// kernel (chains of groups of epw_of(n) elements) or, with mfma, the element
// kernel (one element per slot).  node_state: empty or [n_node] of
// SEM_NODE_PRIOR / SEM_NODE_OTHER.  Returns SEM_OK or an error set through
// sem::fail.
int plan_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n, int dpn,
             bool mfma, const std::vector<uint8_t>& node_state, const PlanOptions& opt, Plan& P);

}  // namespace semplan
