// Host planner of the 2-D scatter (once per element map): packs the map into
// groups and chains, colours them, and decides every entry's write code; the
// kernels (sem_kernels.h) execute the codes as they find them.  Plain C++17,
// no HIP: checked on the CPU by tools/plan_check.cpp (tests/test_plan_host.py).
#include "sem_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include "sem_error.h"

using sem::fail;
using namespace semk;

namespace semplan {
namespace {

// ---------------------------------------------------------------------------
// The chain plan (build_plan):
//   1. groups = EPW element slots (one wavefront each), chains = CH = 4 *
//      rounds consecutive groups (one workgroup each), from a group table
//      (groups_consecutive / groups_blocks below);
//   2. greedy colouring of chains: chains of one colour share no node
//      (per-node colour bitmask; chains needing > MAX_COLOURS colours, and
//      every chain of a non-conforming mesh, go to a final all-atomic class);
//   3. launch order = colour-major; epos[e] = packed position of element e;
//   4. inside a chain the 4 groups of a round run concurrently, rounds run in
//      order.  A node may be shared inside a round only by (a) the elements on
//      two neighbouring lanes of one group (row r, lanes L, L+1: MERGE on L,
//      SKIP on L+1) or (b) the last lane of group i-1 and lane 0 of group i
//      (row r: SKIP on the former, CARRY on the latter); anything else makes
//      the chain atomic.  Across rounds, (c) row n-1 of a lane's element and
//      row 0 of the same lane's element in the next round (the block layout)
//      is carried in registers: SKIP | CARRY on the former, which is then no
//      writer at all; any other node a chain touches again in a later round
//      is a read-modify-write of its own earlier store;
//   5. write codes in launch order: first writer of a node -> STORE, later
//      writers -> RMW (atomic chains -> ATOMIC);
//   6. zero list = unreferenced nodes + nodes whose first writer is atomic.
// ---------------------------------------------------------------------------

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share
// one L2).  For a seam-plan launch of at most SEM_CHAIN_SWIZZLE_MAX chains
// (default 2,400) the planner reorders the chains so that workgroup b runs
// chain q(b) = x * (nch / 8) + min(x, nch % 8) + b / 8 (x = b % 8): each XCD
// then works on one contiguous run of chains, which share node columns of u
// and x_phys and the partial lines of y at their ends.  A permutation of the
// chain blocks of the packed arrays (slots, element positions, chain
// colours); node-indexed data and the seam sums are untouched, so results
// are bitwise those of the unpermuted plan.  Measured as a kernel-side
// remap (profiles/r04/xcd/, kernel median ms per action): cfg2 256^2 (2,341
// chains) 0.042 against 0.044; on the larger launches (4,993 - 9,472 chains)
// neutral to 6 % slower, hence the bound.  (Done in the kernel, as a
// run-time choice, it cost the headline kernel a scratch spill per round.)
void chain_swizzle(Plan& P, int n, int rounds, int64_t max_chains) {
  if (P.colour_start.size() != 2) return;
  const int64_t nch = P.colour_start[1] - P.colour_start[0];
  if (nch < 16 || nch > max_chains) return;
  const int64_t spc = (int64_t)rounds * chain_waves_of(n);  // slots per chain
  if (P.n_slots != nch * spc) return;
  constexpr int64_t NX = 8;
  const int64_t q = nch / NX, r = nch % NX;
  std::vector<int64_t> perm(nch), inv(nch);  // new position b <- old chain perm[b]
  for (int64_t b = 0; b < nch; ++b) {
    const int64_t x = b % NX, k = b / NX;
    perm[b] = x * q + (x < r ? x : r) + k;
    inv[perm[b]] = b;
  }
  const size_t per_slot = P.mapP.size() / (size_t)P.n_slots;
  std::vector<uint32_t> mp(P.mapP.size());
  std::vector<uint8_t> fill(P.slot_fill.size());
  for (int64_t b = 0; b < nch; ++b) {
    std::copy(P.mapP.begin() + perm[b] * spc * per_slot,
              P.mapP.begin() + (perm[b] + 1) * spc * per_slot, mp.begin() + b * spc * per_slot);
    std::copy(P.slot_fill.begin() + perm[b] * spc, P.slot_fill.begin() + (perm[b] + 1) * spc,
              fill.begin() + b * spc);
  }
  P.mapP.swap(mp);
  P.slot_fill.swap(fill);
  const int epw = epw_of(n);
  for (int& ep : P.epos) {
    if (ep < 0) continue;
    const int64_t slot = ep / epw, k = ep % epw;
    const int64_t ch = slot / spc, within = slot % spc;
    ep = (int)((inv[ch] * spc + within) * epw + k);
  }
  if ((int64_t)P.chain_colour.size() == nch) {
    std::vector<uint8_t> cc(nch);
    for (int64_t b = 0; b < nch; ++b) cc[b] = P.chain_colour[perm[b]];
    P.chain_colour.swap(cc);
  }
}

// groups of EPW consecutive elements, chains of CH consecutive groups
void groups_consecutive(int64_t n_elem, int epw, int CH, std::vector<int64_t>& gel) {
  const int64_t n_groups = (n_elem + epw - 1) / epw;
  const int64_t n_chains = (n_groups + CH - 1) / CH;
  gel.assign((size_t)(n_chains * CH * epw), -1);
  for (int64_t e = 0; e < n_elem; ++e) gel[e] = e;
}

// Block layout for structured numberings: the elements form
// "lines" -- runs of consecutive ids in which each element's last node column
// is the next one's first -- of equal length L, and line l + 1 sits on line l
// (element e + L has e's node row n-1 as its row 0).  A chain is a block of
// R stacked lines x CW * EPW elements; round rd of the chain is line rd of the
// block, so the node row between consecutive rounds is carried from one round
// to the next in registers (same wave, same lane) instead of being written by
// two chains.  Returns false (gel untouched) when the numbering is not of
// that form; the caller then uses groups_consecutive.
bool groups_blocks(const std::vector<uint32_t>& e2n, int64_t n_elem, int n, int epw, int CW,
                   int R, std::vector<int64_t>& gel) {
  const int nn = n * n;
  auto at = [&](int64_t e, int r, int jj) { return e2n[e * nn + r * n + jj]; };
  std::vector<int64_t> ls{0};
  for (int64_t e = 0; e + 1 < n_elem; ++e) {
    bool cont = true;
    for (int r = 0; r < n && cont; ++r) cont = at(e, r, n - 1) == at(e + 1, r, 0);
    if (!cont) ls.push_back(e + 1);
  }
  ls.push_back(n_elem);
  const int64_t nl = (int64_t)ls.size() - 1;
  if (nl < 2 || R < 2) return false;
  const int64_t len = ls[1] - ls[0];
  for (int64_t l = 0; l < nl; ++l)
    if (ls[l + 1] - ls[l] != len) return false;
  std::vector<uint8_t> on(nl, 0);  // line l + 1 sits on line l
  int64_t n_on = 0;
  for (int64_t l = 0; l + 1 < nl; ++l) {
    bool ok = true;
    for (int64_t i = 0; i < len && ok; ++i)
      for (int jj = 0; jj < n && ok; ++jj) ok = at(ls[l] + i + len, 0, jj) == at(ls[l] + i, n - 1, jj);
    on[l] = ok ? 1 : 0;
    n_on += ok ? 1 : 0;
  }
  if (n_on * 2 < nl - 1) return false;
  const int64_t seg = (int64_t)CW * epw;
  const int64_t nseg = (len + seg - 1) / seg;
  std::vector<int64_t> out;
  out.reserve((size_t)((nl + R - 1) / R * nseg * R * seg));
  for (int64_t l = 0; l < nl;) {
    int r = 1;  // stacked lines of this block
    while (r < R && l + r < nl && on[l + r - 1]) ++r;
    for (int64_t sg = 0; sg < nseg; ++sg)
      for (int rd = 0; rd < R; ++rd)
        for (int w = 0; w < CW; ++w)
          for (int k = 0; k < epw; ++k) {
            const int64_t i = sg * seg + (int64_t)w * epw + k;
            out.push_back(rd < r && i < len ? ls[l + rd] + i : -1);
          }
    l += r;
  }
  gel.swap(out);
  return true;
}

inline bool is_bnd(int n, int r, int jj) { return r == 0 || r == n - 1 || jj == 0 || jj == n - 1; }

// What the three builders below share.
// References of every node (cnt), P.owner = the first element referencing it,
// P.conforming = the interior local nodes of every element are its own.
int count_refs(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n, Plan& P,
               std::vector<uint32_t>& cnt) {
  const int nn = n * n;
  cnt.assign(n_node, 0);
  P.owner.assign(n_node, 0xFFFFFFFFu);
  for (int64_t t = 0; t < n_elem * nn; ++t) {
    if (e2n[t] >= n_node) return fail(SEM_E_INVALID, "element map references node >= n_node");
    if (!cnt[e2n[t]]++) P.owner[e2n[t]] = (uint32_t)(t / nn);
  }
  P.conforming = true;
  for (int64_t e = 0; e < n_elem; ++e)
    for (int r = 1; r < n - 1; ++r)
      for (int jj = 1; jj < n - 1; ++jj)
        if (cnt[e2n[e * nn + r * n + jj]] != 1) {
          P.conforming = false;
          return SEM_OK;
        }
  return SEM_OK;
}

// written[g]: y[g] holds a value before this plan's first writer (SEM_NODE_PRIOR)
std::vector<uint8_t> prior_values(const std::vector<uint8_t>& node_state, int64_t n_node) {
  std::vector<uint8_t> written(n_node, 0);
  for (size_t i = 0; i < node_state.size(); ++i)
    written[i] = (node_state[i] & SEM_NODE_PRIOR) ? 1 : 0;
  return written;
}

// Launch order, colour-major: order[start[q] .. start[q + 1]) = the items of
// colour q (the trailing class MAX_COLOURS: atomic) in the order of seq, or
// in natural order when seq is null.
void colour_major(const std::vector<int64_t>* seq, const std::vector<int>& colour,
                  std::vector<int64_t>& start, std::vector<int64_t>& order) {
  const int64_t count = (int64_t)colour.size();
  start.assign(MAX_COLOURS + 2, 0);
  for (int64_t i = 0; i < count; ++i) start[colour[i] + 1]++;
  for (int q = 0; q <= MAX_COLOURS; ++q) start[q + 1] += start[q];
  std::vector<int64_t> fill(start.begin(), start.end() - 1);
  order.resize(count);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t id = seq ? (*seq)[i] : i;
    order[fill[colour[id]]++] = id;
  }
}

// the zero list's tail: the unreferenced nodes no other operator writes; sorted
void finish_zero_list(const std::vector<uint32_t>& cnt, const std::vector<uint8_t>& node_state,
                      Plan& P) {
  for (size_t i = 0; i < cnt.size(); ++i)
    if (cnt[i] == 0 && (node_state.empty() || !node_state[i])) P.zero.push_back((uint32_t)i);
  std::sort(P.zero.begin(), P.zero.end());
}

// Breadth-first element order (bfs) and a greedy colouring along it, used by
// the two element-coloured plans: elements of one colour < MAX_COLOURS share
// no node; colour MAX_COLOURS = no colour left, or a node referenced twice.
void colour_elements(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
                     bool conforming, std::vector<int64_t>& bfs, std::vector<int>& colour) {
  const int nn = n * n;
  auto shared_local = [&](int r, int jj) { return !conforming || is_bnd(n, r, jj); };
  // breadth-first element order over shared nodes: greedy colouring along it
  // needs far fewer colours than along a random element order (split
  // triangles, shuffled: 8 instead of 11), and packing classes in it keeps
  // neighbouring elements in neighbouring groups
  bfs.clear();
  bfs.reserve(n_elem);
  {
    std::vector<int64_t> start(n_node + 1, 0);
    for (int64_t e = 0; e < n_elem; ++e)
      for (int r = 0; r < n; ++r)
        for (int jj = 0; jj < n; ++jj)
          if (shared_local(r, jj)) start[e2n[e * nn + r * n + jj] + 1]++;
    for (int64_t i = 0; i < n_node; ++i) start[i + 1] += start[i];
    std::vector<int64_t> inc(start[n_node]), fill(start.begin(), start.end() - 1);
    for (int64_t e = 0; e < n_elem; ++e)
      for (int r = 0; r < n; ++r)
        for (int jj = 0; jj < n; ++jj)
          if (shared_local(r, jj)) inc[fill[e2n[e * nn + r * n + jj]]++] = e;
    std::vector<uint8_t> seen(n_elem, 0);
    for (int64_t s0 = 0; s0 < n_elem; ++s0) {
      if (seen[s0]) continue;
      seen[s0] = 1;
      size_t head = bfs.size();
      bfs.push_back(s0);
      while (head < bfs.size()) {
        const int64_t e = bfs[head++];
        for (int r = 0; r < n; ++r)
          for (int jj = 0; jj < n; ++jj) {
            if (!shared_local(r, jj)) continue;
            const uint32_t gid = e2n[e * nn + r * n + jj];
            for (int64_t t = start[gid]; t < start[gid + 1]; ++t)
              if (!seen[inc[t]]) {
                seen[inc[t]] = 1;
                bfs.push_back(inc[t]);
              }
          }
      }
    }
  }
  std::vector<uint8_t> cmask(n_node, 0);
  std::vector<int64_t> stamp(n_node, -1);
  colour.assign(n_elem, 0);
  std::vector<uint32_t> cn;
  for (const int64_t e : bfs) {
    cn.clear();
    uint32_t forb = 0;
    bool dup = false;
    for (int r = 0; r < n; ++r)
      for (int jj = 0; jj < n; ++jj)
        if (shared_local(r, jj)) {
          const uint32_t gid = e2n[e * nn + r * n + jj];
          if (stamp[gid] == e) {
            dup = true;
            continue;
          }
          stamp[gid] = e;
          cn.push_back(gid);
          forb |= cmask[gid];
        }
    int c = MAX_COLOURS;
    if (!dup)
      for (int q = 0; q < MAX_COLOURS; ++q)
        if (!(forb & (1u << q))) {
          c = q;
          break;
        }
    if (c < MAX_COLOURS)
      for (uint32_t gid : cn) cmask[gid] |= (uint8_t)(1u << c);
    colour[e] = c;
  }
}

// node_state (may be empty): SEM_NODE_PRIOR = y already holds a value when
// this operator runs (first touches become read-modify-write, never zeroed);
// SEM_NODE_OTHER = another operator writes it (not zeroed when unreferenced).
// block_rounds >= 2: try the block layout with that many rounds (P.blocks
// tells whether it applied; rounds is then block_rounds).
int build_plan(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
               int rounds, const std::vector<uint8_t>& node_state, Plan& P, int seam = 0,
               int seam_dpn = 1, int block_rounds = 0) {
  const int epw = epw_of(n), lw = epw * n, nn = n * n;
  const int CW = chain_waves_of(n);  // groups of a chain that run concurrently
  std::vector<int64_t> gel;          // [group][lane element] -> element or -1
  // block_rounds < 0: AUTO -- 4 rounds when the mesh then still has enough
  // chains to fill the chip many times over (block_min_chains); fewer chains
  // leave a tail of lone workgroups that costs more than the carried rows save
  const bool block_auto = block_rounds < 0;
  if (block_auto) block_rounds = 4;
  P.blocks = block_rounds >= 2 && groups_blocks(e2n, n_elem, n, epw, CW, block_rounds, gel);
  if (P.blocks && block_auto &&
      (int64_t)gel.size() / ((int64_t)epw * CW * block_rounds) < block_min_chains(n, seam_dpn)) {
    P.blocks = false;
    gel.clear();
  }
  if (P.blocks) rounds = block_rounds;
  P.rounds = rounds;
  const int CH = CW * rounds;
  if (!P.blocks) groups_consecutive(n_elem, epw, CH, gel);
  const int64_t n_groups = (int64_t)gel.size() / epw;
  const int64_t n_chains = n_groups / CH;
  std::vector<uint32_t> cnt;
  if (const int rc = count_refs(e2n, n_elem, n_node, n, P, cnt)) return rc;
  const bool conforming = P.conforming;
  auto shared_local = [&](int r, int jj) { return !conforming || is_bnd(n, r, jj); };
  // the elements of chain ch, lane order
  auto chain_elem = [&](int64_t ch, int64_t t) { return gel[(size_t)(ch * CH * epw + t)]; };
  const int64_t chain_len = (int64_t)CH * epw;
  // 2. chain colouring
  std::vector<uint8_t> cmask(n_node, 0);
  std::vector<int> colour(n_chains);
  {
    std::vector<int64_t> stamp(n_node, -1);
    std::vector<uint32_t> cn;
    for (int64_t ch = 0; ch < n_chains; ++ch) {
      int c = MAX_COLOURS;
      if (conforming) {
        cn.clear();
        uint32_t forb = 0;
        for (int64_t t = 0; t < chain_len; ++t) {
          const int64_t e = chain_elem(ch, t);
          if (e < 0) continue;
          for (int r = 0; r < n; ++r)
            for (int jj = 0; jj < n; ++jj)
              if (is_bnd(n, r, jj)) {
                const uint32_t gid = e2n[e * nn + r * n + jj];
                if (stamp[gid] != ch) {
                  stamp[gid] = ch;
                  cn.push_back(gid);
                  forb |= cmask[gid];
                }
              }
        }
        for (int q = 0; q < MAX_COLOURS; ++q)
          if (!(forb & (1u << q))) {
            c = q;
            break;
          }
        if (c < MAX_COLOURS)
          for (uint32_t gid : cn) cmask[gid] |= (uint8_t)(1u << c);
      }
      colour[ch] = c;
    }
  }
  std::vector<uint8_t>().swap(cmask);
  // 3. launch order: colour-major (one launch per colour), or for the seam
  // plan element order in one launch
  std::vector<int64_t> order(n_chains);
  if (seam == 2) {  // AUTO (seam_auto): high orders, or colour classes below ~1 generation
    std::vector<int64_t> per(MAX_COLOURS + 1, 0);
    for (int64_t ch = 0; ch < n_chains; ++ch) per[colour[ch]]++;
    seam = seam_auto(n, *std::max_element(per.begin(), per.end()), seam_dpn, P.blocks) ? 1 : 0;
  }
  P.seam = seam == 1 && conforming;
  for (int64_t ch = 0; ch < n_chains && P.seam; ++ch)
    if (colour[ch] >= MAX_COLOURS) P.seam = false;
  std::vector<uint8_t> nw;      // seam plan: chains writing each node (saturating)
  std::vector<uint16_t> smask;  // and their colours
  if (P.seam) {
    for (int64_t ch = 0; ch < n_chains; ++ch) order[ch] = ch;
    P.colour_start = {0, n_chains};
    nw.assign(n_node, 0);
    smask.assign(n_node, 0);
    std::vector<int32_t> lastc2(n_node, -1);
    int maxc = 0;
    for (int64_t ch = 0; ch < n_chains; ++ch) {
      maxc = std::max(maxc, colour[ch]);
      for (int64_t t = 0; t < chain_len; ++t) {
        const int64_t e = chain_elem(ch, t);
        if (e < 0) continue;
        for (int r = 0; r < n; ++r)
          for (int jj = 0; jj < n; ++jj)
            if (is_bnd(n, r, jj)) {
              const uint32_t gid = e2n[e * nn + r * n + jj];
              if (lastc2[gid] != (int32_t)ch) {
                lastc2[gid] = (int32_t)ch;
                if (nw[gid] < 255) nw[gid]++;
                smask[gid] |= (uint16_t)(1u << colour[ch]);
              }
            }
      }
    }
    P.seam_ns = maxc + 1;
    P.chain_colour.resize(n_chains);
    for (int64_t ch = 0; ch < n_chains; ++ch) P.chain_colour[ch] = (uint8_t)colour[ch];
  } else {
    colour_major(nullptr, colour, P.colour_start, order);
  }
  P.n_slots = n_chains * CH;
  P.epos.assign(n_elem, 0);
  P.slot_fill.assign(P.n_slots, 0);
  for (int64_t q = 0; q < n_chains; ++q)
    for (int i = 0; i < CH; ++i) {
      const int64_t g = order[q] * CH + i;
      const int64_t slot = q * CH + i;
      int fill = 0;
      for (int k = 0; k < epw; ++k) {
        const int64_t e = gel[g * epw + k];
        if (e < 0) break;  // real elements first
        P.epos[e] = (int)(slot * epw + k);
        fill = k + 1;
      }
      P.slot_fill[slot] = (uint8_t)fill;
    }
  // 4./5. validation and write codes, chain by chain in launch order
  P.mapP.assign((size_t)P.n_slots * n * lw, W_SKIP << CODE_SHIFT);
  std::vector<uint8_t> written = prior_values(node_state, n_node);
  std::vector<int64_t> lastc(n_node, -1);  // chain of the last touch
  std::vector<int> lastt(n_node, -1);      // (group in chain) * n * lw + pos of the last touch
  // per entry: 0 normal, 1 merge-skip, 2 carry-skip, 3 carry-in, 4 row carry-out
  std::vector<uint8_t> act((size_t)CH * n * lw);
  P.n_atomic_groups = 0;
  P.row_carries = 0;
  P.round_sync = false;
  bool seam_conflict = false;
  auto lane_elem = [&](int64_t g, int lane) -> int64_t {
    const int k = lane / n;
    return k < epw ? gel[g * epw + k] : -1;
  };
  for (int64_t q = 0; q < n_chains; ++q) {
    const int64_t ch = order[q];
    bool atomic_chain = colour[ch] >= MAX_COLOURS;
    std::fill(act.begin(), act.end(), (uint8_t)0);
    if (!atomic_chain) {
      // (c) row carries between consecutive rounds of a wave
      for (int i = 0; i + CW < CH; ++i) {
        const int64_t g = ch * CH + i;
        for (int lane = 0; lane < lw; ++lane) {
          const int jj = lane % n;
          const int64_t e = lane_elem(g, lane), f = lane_elem(g + CW, lane);
          if (e < 0 || f < 0) continue;
          if (e2n[f * nn + jj] == e2n[e * nn + (n - 1) * n + jj])
            act[(size_t)i * n * lw + (n - 1) * lw + lane] = 4;
        }
      }
      for (int i = 0; i < CH && !atomic_chain; ++i) {
        const int64_t g = ch * CH + i;
        for (int r = 0; r < n && !atomic_chain; ++r)
          for (int lane = 0; lane < lw; ++lane) {
            const int jj = lane % n;
            const int64_t e = lane_elem(g, lane);
            if (e < 0) continue;
            if (!shared_local(r, jj)) continue;
            const int pos = r * lw + lane;
            const int tag = i * n * lw + pos;
            if (act[tag] == 4) continue;  // carried to the next round: not a writer
            const uint32_t gid = e2n[e * nn + r * n + jj];
            if (lastc[gid] == ch) {
              const int pi = lastt[gid] / (n * lw), ppos = lastt[gid] % (n * lw);
              const bool same_round = (pi / CW) == (i / CW);
              if (pi == i && lane > 0 && ppos == pos - 1 && jj == 0 && (ppos % lw) % n == n - 1) {
                act[tag] = 1;  // merge into lane L (pos-1)
              } else if (pi == i - 1 && lane == 0 && ppos == r * lw + lw - 1) {
                act[tag] = 3;  // carry-in
                act[pi * n * lw + ppos] = 2;  // carry-out skip
              } else if (same_round) {
                atomic_chain = true;
                break;
              } else if (P.seam && nw[gid] >= 2) {
                // an earlier round of this chain stored the node into its
                // seam slot: a second plain slot store would drop it
                seam_conflict = true;
              } else {
                P.round_sync = true;  // an earlier round of this chain: sequential, RMW
              }
            }
            lastc[gid] = ch;
            lastt[gid] = tag;
          }
      }
    }
    if (atomic_chain) {
      for (int i = 0; i < CH; ++i)
        if (gel[(ch * CH + i) * epw] >= 0) P.n_atomic_groups++;
    }
    for (int i = 0; i < CH; ++i) {
      const int64_t g = ch * CH + i;
      uint32_t* out = P.mapP.data() + (q * CH + i) * (int64_t)n * lw;
      for (int r = 0; r < n; ++r)
        for (int lane = 0; lane < lw; ++lane) {
          const int pos = r * lw + lane;
          const int jj = lane % n;
          const int64_t e = lane_elem(g, lane);
          if (e < 0) continue;  // padding stays SKIP
          const uint32_t gid = e2n[e * nn + r * n + jj];
          const uint8_t a = act[i * n * lw + pos];
          uint32_t code;
          if (!shared_local(r, jj)) {
            code = written[gid] ? W_RMW : W_STORE;  // conforming interior node: sole writer
          } else if (atomic_chain) {
            code = W_ATOMIC;
            if (!written[gid]) {
              P.zero.push_back(gid);
              written[gid] = 1;
            }
          } else if (a == 4) {
            code = W_ROWCARRY;
            P.row_carries++;
          } else if (a == 1) {
            code = W_SKIP;
            out[pos - 1] |= W_MERGE << CODE_SHIFT;
          } else if (a == 2) {
            code = W_SKIP;
          } else if (P.seam && nw[gid] >= 2) {
            code = W_ATOMIC;  // seam slot of this chain's colour (k_seam_sum)
            if (a == 3) code |= W_CARRY;
          } else {
            code = written[gid] ? W_RMW : W_STORE;
            written[gid] = 1;
            if (a == 3) code |= W_CARRY;
          }
          out[pos] = gid | (code << CODE_SHIFT);
        }
    }
  }
  finish_zero_list(cnt, node_state, P);
  P.n_rmw = 0;
  for (const uint32_t e : P.mapP) P.n_rmw += ((e >> CODE_SHIFT) & 3u) == W_RMW ? 1 : 0;
  if (P.seam) {
    if (P.n_atomic_groups || seam_conflict) {  // sharing the seam slots cannot express
      P.seam = false;
      P.seam_failed = true;  // the caller plans again without seams
      return SEM_OK;
    }
    for (int64_t i = 0; i < n_node; ++i)
      if (nw[i] >= 2) {
        P.seam_gid.push_back((uint32_t)i);
        const bool prior = !node_state.empty() && (node_state[i] & SEM_NODE_PRIOR);
        P.seam_mask.push_back((uint16_t)(smask[i] | (prior ? 0x100u : 0u)));
      }
  }
  return SEM_OK;
}


// 16-bit form of a column-kernel plan's packed map: one 32-bit
// base per (slot, row) = the smallest node id of the row's real elements,
// entries (gid - base) | code << 12, for rows spanning fewer than 4096 ids
// (locality-ordered meshes; 57 consecutive ids per row at p = 8 on the
// structured mesh); padding entries keep offset 0.  A group with a wider row
// is flagged (base[slot][0] = M16_WIDE) and reads the 32-bit map; the form is
// used only when at most 1 / 16 of the groups are flagged.
bool build_map16(const Plan& P, int n, std::vector<uint16_t>& m16, std::vector<uint32_t>& base) {
  const int lw = epw_of(n) * n;
  m16.assign((size_t)P.n_slots * n * lw, (uint16_t)(W_SKIP << M16_CODE_SHIFT));
  base.assign((size_t)P.n_slots * n, 0u);
  int64_t wide = 0;
  for (int64_t sl = 0; sl < P.n_slots; ++sl) {
    if (!P.slot_fill[sl]) continue;
    const int lanes = P.slot_fill[sl] * n;
    bool fits = true;
    for (int r = 0; r < n && fits; ++r) {
      const uint32_t* row = &P.mapP[((size_t)sl * n + r) * lw];
      uint32_t lo = 0xFFFFFFFFu, hi = 0;
      for (int l = 0; l < lanes; ++l) {
        lo = std::min(lo, row[l] & GID_MASK);
        hi = std::max(hi, row[l] & GID_MASK);
      }
      base[(size_t)sl * n + r] = lo;
      fits = hi - lo <= M16_OFF_MASK;
    }
    if (!fits) {
      base[(size_t)sl * n] = M16_WIDE;
      ++wide;
      continue;
    }
    for (int r = 0; r < n; ++r) {
      const uint32_t* row = &P.mapP[((size_t)sl * n + r) * lw];
      const uint32_t lo = base[(size_t)sl * n + r];
      uint16_t* out = &m16[((size_t)sl * n + r) * lw];
      for (int l = 0; l < lanes; ++l)
        out[l] = (uint16_t)(((row[l] & GID_MASK) - lo) | ((row[l] >> CODE_SHIFT) << M16_CODE_SHIFT));
    }
  }
  int64_t filled = 0;
  for (uint8_t f : P.slot_fill) filled += f ? 1 : 0;
  return wide * 16 <= filled;
}

// Pattern table of a 16-bit map (the PAT kernels, csrc/sem_kernels.h): every
// group's block of n x lw entries (offsets and codes) deduplicated; the
// table replaces m16 and each group's pattern id goes into bits 28-31 of its
// bases 1..map_pattern_id_rows(n).  Declined when an order has no PAT
// kernels, when more than 1 / 8 of the groups are distinct, or past
// 16^id_rows patterns.  On the structured block layout a handful of layouts (which rows are carried,
// slotted or merged) cover every group.
bool build_map_patterns(std::vector<uint16_t>& m16, std::vector<uint32_t>& mb, int n,
                        int64_t n_slots, int64_t* n_pat) {
  *n_pat = 0;
  if (!map_pattern_order(n)) return false;
  const int Q = map_pattern_id_rows(n);  // bases carrying the id
  const int lw = epw_of(n) * n;
  const uint32_t max_pat = 1u << (4 * Q);
  const size_t blk = (size_t)n * lw;
  std::unordered_map<uint64_t, std::vector<uint32_t>> seen;
  std::vector<uint16_t> table;
  std::vector<uint32_t> pid((size_t)n_slots, 0);
  for (int64_t sl = 0; sl < n_slots; ++sl) {
    if (mb[(size_t)sl * n] == M16_WIDE) continue;  // reads the 32-bit map
    const uint16_t* e = &m16[(size_t)sl * blk];
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < blk; ++i) h = (h ^ e[i]) * 1099511628211ull;
    auto& cand = seen[h];
    uint32_t id = 0xFFFFFFFFu;
    for (uint32_t c : cand)
      if (std::memcmp(&table[(size_t)c * blk], e, blk * sizeof(uint16_t)) == 0) {
        id = c;
        break;
      }
    if (id == 0xFFFFFFFFu) {
      id = (uint32_t)(table.size() / blk);
      if (id >= max_pat || (int64_t)id * 8 > n_slots) return false;
      table.insert(table.end(), e, e + blk);
      cand.push_back(id);
    }
    pid[(size_t)sl] = id;
  }
  // bases 1..Q must have their top 4 bits free (node ids < 2^28: packed maps)
  for (int64_t sl = 0; sl < n_slots; ++sl) {
    if (mb[(size_t)sl * n] == M16_WIDE) continue;
    for (int q = 1; q <= Q; ++q)
      if (mb[(size_t)sl * n + q] & ~GID_MASK) return false;
  }
  for (int64_t sl = 0; sl < n_slots; ++sl) {
    if (mb[(size_t)sl * n] == M16_WIDE) continue;
    for (int q = 0; q < Q; ++q)
      mb[(size_t)sl * n + 1 + q] |= ((pid[(size_t)sl] >> (4 * q)) & 15u) << 28;
  }
  *n_pat = (int64_t)(table.size() / blk);
  m16.swap(table);
  return true;
}

// ---------------------------------------------------------------------------
// Element-level plan for the MFMA kernel (one element per wavefront, no
// chains): elements are greedily coloured so that elements of one colour
// share no node (a per-node colour bitmask over their element-boundary nodes,
// all nodes on a non-conforming map); one launch per colour, natural element
// order inside a colour; STORE for the first writer of a node in launch
// order, RMW after it.  Elements that would need more than MAX_COLOURS
// colours, or that reference one node twice, go to a final class whose
// shareable nodes are written with atomics.  Group = slot = one element, so
// the packed map and factors are compact per element ([slot][r][j]).
// ---------------------------------------------------------------------------
// seam = 1 (n = 17 kernel): one launch over all elements in breadth-first
// order instead of one per colour; a node of several elements is stored by
// each into the slot of its element's colour and summed by k_seam_sum (the
// column kernel's seam plan with one element per chain).
// seams for the n = 17 MFMA kernel under AUTO (SEM_SEAM=0 / 1 forces): off.
// p = 16, 198^2 on MI355X (profiles/r03/mfma17): one launch 0.161 ms + seam
// sums 0.052 ms (the seam slots of horizontal element edges are scattered
// 8-byte accesses) against 4 colour launches of 0.049 ms
#ifndef MFMA_SEAM_AUTO
#define MFMA_SEAM_AUTO 0
#endif
int build_plan_elem(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
                    const std::vector<uint8_t>& node_state, Plan& P, int seam = 0) {
  const int nn = n * n;
  std::vector<uint32_t> cnt;
  if (const int rc = count_refs(e2n, n_elem, n_node, n, P, cnt)) return rc;
  const bool conforming = P.conforming;
  auto shared_local = [&](int r, int jj) { return !conforming || is_bnd(n, r, jj); };
  std::vector<int64_t> bfs;
  std::vector<int> colour;
  colour_elements(e2n, n_elem, n_node, n, conforming, bfs, colour);
  std::vector<int64_t> order(n_elem);
  int maxc = 0;
  for (int64_t e = 0; e < n_elem; ++e) maxc = std::max(maxc, colour[e]);
  P.seam = seam == 1 && conforming && maxc < MAX_COLOURS;
  if (P.seam) {
    order = bfs;
    P.colour_start = {0, n_elem};
    P.seam_ns = maxc + 1;
    P.chain_colour.resize(n_elem);
    for (int64_t q = 0; q < n_elem; ++q) P.chain_colour[q] = (uint8_t)colour[order[q]];
  } else {
    colour_major(nullptr, colour, P.colour_start, order);
  }
  P.n_slots = n_elem;
  P.epos.assign(n_elem, 0);
  for (int64_t q = 0; q < n_elem; ++q) P.epos[order[q]] = (int)q;
  P.slot_fill.assign(n_elem, 1);
  P.mapP.assign((size_t)n_elem * nn, W_SKIP << CODE_SHIFT);
  std::vector<uint8_t> written = prior_values(node_state, n_node);
  P.n_atomic_groups = 0;
  for (int64_t q = 0; q < n_elem; ++q) {
    const int64_t e = order[q];
    const bool atomic = colour[e] >= MAX_COLOURS;
    if (atomic) P.n_atomic_groups++;
    uint32_t* out = P.mapP.data() + q * nn;
    for (int r = 0; r < n; ++r)
      for (int jj = 0; jj < n; ++jj) {
        const uint32_t gid = e2n[e * nn + r * n + jj];
        uint32_t code;
        if (P.seam && cnt[gid] >= 2) {
          code = W_ATOMIC;  // seam slot of this element's colour (k_seam_sum)
        } else if (atomic && shared_local(r, jj)) {
          code = W_ATOMIC;
          if (!written[gid]) P.zero.push_back(gid);
        } else {
          code = written[gid] ? W_RMW : W_STORE;
        }
        written[gid] = 1;
        out[r * n + jj] = gid | (code << CODE_SHIFT);
      }
  }
  finish_zero_list(cnt, node_state, P);
  P.n_rmw = 0;
  for (const uint32_t e : P.mapP) P.n_rmw += ((e >> CODE_SHIFT) & 3u) == W_RMW ? 1 : 0;
  if (P.seam) {
    std::vector<uint16_t> smask(n_node, 0);
    for (int64_t e = 0; e < n_elem; ++e)
      for (int t = 0; t < nn; ++t) smask[e2n[e * nn + t]] |= (uint16_t)(1u << colour[e]);
    for (int64_t i = 0; i < n_node; ++i)
      if (cnt[i] >= 2) {
        P.seam_gid.push_back((uint32_t)i);
        const bool prior = !node_state.empty() && (node_state[i] & SEM_NODE_PRIOR);
        P.seam_mask.push_back((uint16_t)(smask[i] | (prior ? 0x100u : 0u)));
      }
  }
  return SEM_OK;
}

// ---------------------------------------------------------------------------
// Element-coloured plan for the column kernel (meshes whose element order
// defeats the chain patterns: irregular valence, random element order).
// Elements are greedily coloured, in breadth-first order over shared nodes,
// so that elements of one colour share no node, then packed colour class by
// colour class, in that order inside a class, into groups of EPW elements and
// chains of chain_waves_of(n) * rounds groups (a class's last group / chain may
// be partly empty).  Nothing inside a launch shares a node, so the codes
// are plain STORE (first writer in launch order) / RMW with no merge or
// carry; elements needing more than MAX_COLOURS colours go to a final
// all-atomic class.  Chosen by plan_map when the chain plan would send
// more than half of its groups to the atomic fallback and this plan sends
// fewer.
// ---------------------------------------------------------------------------
int build_plan_ecol(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
                    int rounds, const std::vector<uint8_t>& node_state, Plan& P) {
  const int epw = epw_of(n), lw = epw * n, nn = n * n;
  const int CH = chain_waves_of(n) * rounds;
  std::vector<uint32_t> cnt;
  if (const int rc = count_refs(e2n, n_elem, n_node, n, P, cnt)) return rc;
  const bool conforming = P.conforming;
  auto shared_local = [&](int r, int jj) { return !conforming || is_bnd(n, r, jj); };
  std::vector<int64_t> bfs;
  std::vector<int> colour;
  colour_elements(e2n, n_elem, n_node, n, conforming, bfs, colour);
  // pack each class (cls[q] .. cls[q + 1] of order) into groups and chains
  std::vector<int64_t> cls, order;
  colour_major(&bfs, colour, cls, order);
  P.colour_start.assign(MAX_COLOURS + 2, 0);
  int64_t n_chains = 0;
  for (int q = 0; q <= MAX_COLOURS; ++q) {
    const int64_t groups = (cls[q + 1] - cls[q] + epw - 1) / epw;
    n_chains += (groups + CH - 1) / CH;
    P.colour_start[q + 1] = n_chains;
  }
  P.n_slots = n_chains * CH;
  P.epos.assign(n_elem, 0);
  P.slot_fill.assign(P.n_slots, 0);
  P.mapP.assign((size_t)P.n_slots * n * lw, W_SKIP << CODE_SHIFT);
  std::vector<uint8_t> written = prior_values(node_state, n_node);
  P.n_atomic_groups = 0;
  for (int q = 0; q <= MAX_COLOURS; ++q) {
    const bool atomic = q == MAX_COLOURS;
    const int64_t slot0 = P.colour_start[q] * CH;
    for (int64_t idx = 0; idx < cls[q + 1] - cls[q]; ++idx) {
      const int64_t e = order[cls[q] + idx];
      const int64_t slot = slot0 + idx / epw;
      const int k = (int)(idx % epw);
      P.epos[e] = (int)(slot * epw + k);
      P.slot_fill[slot] = (uint8_t)(k + 1);
      uint32_t* out = P.mapP.data() + slot * (int64_t)n * lw;
      for (int r = 0; r < n; ++r)
        for (int jj = 0; jj < n; ++jj) {
          const uint32_t gid = e2n[e * nn + r * n + jj];
          uint32_t code;
          if (atomic && shared_local(r, jj)) {
            code = W_ATOMIC;
            if (!written[gid]) P.zero.push_back(gid);
          } else {
            code = written[gid] ? W_RMW : W_STORE;
          }
          written[gid] = 1;
          out[r * lw + k * n + jj] = gid | (code << CODE_SHIFT);
        }
    }
    if (atomic) P.n_atomic_groups += (cls[q + 1] - cls[q] + epw - 1) / epw;
  }
  finish_zero_list(cnt, node_state, P);
  return SEM_OK;
}

}  // namespace

PlanOptions plan_options_from_env() {
  PlanOptions o;
  if (const char* s = std::getenv("SEM_CHAIN_ROUNDS")) o.chain_rounds = std::max(1, std::atoi(s));
  if (const char* s = std::getenv("SEM_BLOCK_ROUNDS")) o.block_rounds = std::atoi(s);
  if (const char* s = std::getenv("SEM_SEAM")) o.seam = std::atoi(s) == 1 ? 1 : 0;
  if (const char* s = std::getenv("SEM_PLAN")) o.plan = std::atoi(s);
  if (const char* s = std::getenv("SEM_MAP16")) o.map16 = std::atoi(s) != 0;
  if (const char* s = std::getenv("SEM_MAP_PATTERNS")) o.map_patterns = std::atoi(s) != 0;
  if (const char* s = std::getenv("SEM_CHAIN_SWIZZLE_MAX")) o.chain_swizzle_max = std::atoll(s);
  return o;
}

int plan_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n, int dpn,
             bool mfma, const std::vector<uint8_t>& node_state, const PlanOptions& opt, Plan& P) {
  P = Plan();
  int rounds = opt.chain_rounds;
  // the n = 17 MFMA kernel takes seams by default (MFMA_SEAM_AUTO); the
  // n <= 16 MFMA kernel has no seam form
  const int eseam = (mfma && n == 17) ? (opt.seam == 2 ? MFMA_SEAM_AUTO : opt.seam) : 0;
  int rc = mfma ? build_plan_elem(e2n, n_elem, n_node, n, node_state, P, eseam)
                : build_plan(e2n, n_elem, n_node, n, rounds, node_state, P, opt.seam, dpn,
                             opt.block_rounds);
  if (!rc && P.seam_failed) {
    P = Plan();
    rc = build_plan(e2n, n_elem, n_node, n, rounds, node_state, P, 0, dpn, opt.block_rounds);
  }
  if (rc) return rc;
  if (!mfma) rounds = P.rounds;
  // XCD-contiguous chain order for small seam-plan launches (chain_swizzle)
  if (!mfma && P.seam) chain_swizzle(P, n, rounds, opt.chain_swizzle_max);
  // element colouring gives up the chains' gather locality: on a structured
  // mesh whose element order breaks a quarter of the chains it measured 2.4x
  // slower than the chains with their atomics, so it is tried only when most
  // groups would be atomic
  const int64_t ng_col = (n_elem + epw_of(n) - 1) / epw_of(n);
  if (!mfma && opt.plan != 0 && (opt.plan == 1 || P.n_atomic_groups * 2 > ng_col)) {
    Plan Q;
    if ((rc = build_plan_ecol(e2n, n_elem, n_node, n, rounds, node_state, Q))) return rc;
    if (opt.plan == 1 || Q.n_atomic_groups < P.n_atomic_groups) {
      P = std::move(Q);
      P.ecol = true;
    }
  }
  P.rounds = mfma ? 1 : rounds;
  P.blocks = !mfma && !P.ecol && P.blocks;
  if (!P.blocks) P.row_carries = 0;
  // 16-bit map and its pattern table for the column kernel
  if (!mfma && opt.map16 && build_map16(P, n, P.m16, P.mbase)) {
    P.map16 = true;
    P.map_pat = opt.map_patterns && build_map_patterns(P.m16, P.mbase, n, P.n_slots, &P.n_map_pat);
  } else {
    P.m16.clear();
    P.mbase.clear();
  }
  return SEM_OK;
}

}  // namespace semplan
