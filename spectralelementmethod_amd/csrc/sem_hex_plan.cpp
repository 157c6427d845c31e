// Scatter planner of the hexahedral action (sem_hex_plan.h; host, once per
// map).  Pure C++, no HIP: checked on the CPU by tools/hex_plan_check.cpp
// (tests/test_hex_plan_host.py).  DESIGN.md §4.9 / §5.
//
// Chains follow xi0: element e' succeeds e when e's face a = n-1 is e''s
// face a = 0 node for node (same (b, c) order), so one thread holds the
// shared node row of both.  Chains are cut into sub-chains of <= Lc elements
// so that the launch has enough workgroups; a workgroup runs S sub-chains of
// equal length in lockstep (slot s of step k = launch position
// wg_off + k*S + s).
//
// Every (element, node) the kernel writes is a write EVENT, except row
// a = n-1 of a non-last chain element (carried).  A node with one event is a
// plain store.  A node with several events is a SEAM node: each of its events
// goes to a slot of its own and k_hex_seam_sum adds them.  The kernel decides
// per thread and element from two small masks: a boundary column (b or c on
// the element boundary) is slotted as a whole when any of its events is on a
// seam node (cmask bit), a chain's first / last face likewise (cflag).  The
// planner replays exactly that rule (thread_rows), checks that every plain
// store hits a one-event node (conforming mesh) and lists the slots of each
// seam node.
#include "sem_hex_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <unordered_map>

#include "../../include/sem_hip.h"
#include "sem_error.h"

using sem::fail;
using namespace semh;

namespace semhexplan {
namespace {

struct Sub {
  int64_t start, len;  // elements order[start .. start + len)
};

// the map, its sizes and what one step leaves for the next
struct Work {
  const std::vector<uint32_t>& h;
  const int64_t E, n_node;
  const int N, N2;
  const int64_t N3;
  const int S, GZ, GY;
  std::vector<int64_t> succ, pred;          // 1
  std::vector<int64_t> order, chain_start;  // 2: elements chain by chain, [n_chains + 1]
  int64_t lc = 1;                           // 3
  std::vector<Sub> sub;                     // 4
  bool grid = false;                        // 5
  std::vector<int64_t> sub_wg, sub_slot;
  std::vector<uint8_t> grid_wg;
  std::vector<uint8_t> zm, ym;  // 5b: [n_wg * S]
  std::vector<uint8_t> cnt;     // 6: events per node, saturating

  Work(const std::vector<uint32_t>& h_, int64_t E_, int64_t n_node_, int n)
      : h(h_), E(E_), n_node(n_node_), N(n), N2(n * n), N3((int64_t)n * n * n), S(hex_slots(n)),
        GZ(hex_grid_z(n)), GY(hex_slots(n) / hex_grid_z(n)) {}

  int64_t n_chains() const { return (int64_t)chain_start.size() - 1; }
  const uint32_t* elem(size_t i, int64_t k) const { return &h[order[sub[i].start + k] * N3]; }
  // a thread whose column is handed over emits no write of its own (the
  // kernel's give / ygive, sem_hex.h)
  bool merged(int64_t w, int64_t s, int b, int c) const {
    if (c == 0 && zm[w * S + s]) return true;
    return b == 0 && ym[w * S + s] && !(c == 0 && zm[w * S + s - GZ]);
  }
};

uint64_t face_hash(const uint32_t* f, int n2) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int j = 0; j < n2; ++j) {
    h ^= f[j] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
  }
  return h ^ (h >> 31);
}

// hash of an element face given as n^2 entries at f[i * stride1 + j * stride2]
uint64_t face_hash_strided(const uint32_t* f, int n, int stride1, int stride2) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      h ^= f[i * stride1 + j * stride2] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
      h *= 0xBF58476D1CE4E5B9ull;
    }
  return h ^ (h >> 31);
}

// 1. successors along xi0
void successors(Work& W) {
  const std::vector<uint32_t>& h = W.h;
  const int N = W.N, N2 = W.N2;
  const int64_t E = W.E, N3 = W.N3;
  W.succ.assign(E, -1);
  W.pred.assign(E, -1);
  std::unordered_map<uint64_t, int64_t> first;
  first.reserve((size_t)E * 2);
  for (int64_t e = 0; e < E; ++e) {
    auto it = first.emplace(face_hash(&h[e * N3], N2), e);
    if (!it.second) it.first->second = -1;  // ambiguous: never chained
  }
  for (int64_t e = 0; e < E; ++e) {
    const uint32_t* fl = &h[e * N3 + (int64_t)(N - 1) * N2];
    auto it = first.find(face_hash(fl, N2));
    if (it == first.end() || it->second < 0 || it->second == e) continue;
    const int64_t e2 = it->second;
    if (std::memcmp(fl, &h[e2 * N3], sizeof(uint32_t) * N2) != 0) continue;
    if (W.pred[e2] >= 0) continue;
    W.succ[e] = e2;
    W.pred[e2] = e;
  }
}

// 2. maximal chains (heads without predecessor; then any cycle, cut anywhere)
void maximal_chains(Work& W) {
  const int64_t E = W.E;
  W.order.reserve(E);
  std::vector<uint8_t> seen(E, 0);
  auto walk = [&](int64_t e) {
    W.chain_start.push_back((int64_t)W.order.size());
    while (e >= 0 && !seen[e]) {
      seen[e] = 1;
      W.order.push_back(e);
      e = W.succ[e];
    }
  };
  for (int64_t e = 0; e < E; ++e)
    if (W.pred[e] < 0) walk(e);
  for (int64_t e = 0; e < E; ++e)
    if (!seen[e]) walk(e);
  W.chain_start.push_back((int64_t)W.order.size());
}

// 3. sub-chains of near-equal length <= lc.  A workgroup's time grows
//    with its sub-chain length and the launch runs in generations of
//    `resident` workgroups, so lc minimises generations x sub-chain length
//    (ties: the longer sub-chains, fewer seam nodes).  27^3 at p = 8: lc = 9,
//    729 workgroups in one generation -- 0.271 against 0.278 ms per step
//    for the round's first rule (lc = 3, 2.85 generations) and 0.275 /
//    0.288 / 0.305 for lc = 5 / 4 / 7 (profiles/r05/hex/chain_length/).
//    A workgroup also pays a fixed start (D into LDS, its flags, the
//    first map rows) worth about one element step: cost = generations x
//    (sub-chain length + 1).  Without that term the rule took sub-chains
//    of one element at p = 1 / 3 / 6 / 7 (~1e7 DOF, many generations
//    either way): 1.431 / 0.418 / 0.285 / 0.268 ms per step against 1.193
//    / 0.397 / 0.277 / 0.258 with it (sub-chains of 12 / 14 / 8 / 15);
//    the other orders keep their plan (profiles/r06/hex_chain_start/).
//    HexPlanOptions::chain_start sets the term, chain_cap the length.
void choose_length(Work& W, const HexPlanOptions& opt) {
  double best = 0.0;
  for (int64_t c = 1; c <= 16; ++c) {
    int64_t nsub = 0, maxlen = 0;
    for (int64_t ch = 0; ch < W.n_chains(); ++ch) {
      const int64_t M = W.chain_start[ch + 1] - W.chain_start[ch];
      const int64_t parts = (M + c - 1) / c;
      nsub += parts;
      maxlen = std::max(maxlen, (M + parts - 1) / parts);
    }
    const int64_t nwg = (nsub + W.S - 1) / W.S;
    const int64_t gens = opt.resident > 0 ? (nwg + opt.resident - 1) / opt.resident : 1;
    const double cost = (double)gens * ((double)maxlen + opt.chain_start);
    if (c == 1 || cost <= best) {
      best = cost;
      W.lc = c;
    }
  }
  if (opt.chain_cap > 0) W.lc = opt.chain_cap;
}

// 4. the cuts; longest first, then by the smallest node id of the head
//    element (neighbouring sub-chains share faces: on a locality-ordered
//    node numbering they run in the same or adjacent workgroups, whatever
//    the element order)
void sub_chains(Work& W) {
  std::vector<Sub> sub;
  for (int64_t ch = 0; ch < W.n_chains(); ++ch) {
    const int64_t a0 = W.chain_start[ch], M = W.chain_start[ch + 1] - a0;
    const int64_t parts = (M + W.lc - 1) / W.lc;
    const int64_t q = M / parts, r = M % parts;
    int64_t off = a0;
    for (int64_t k = 0; k < parts; ++k) {
      const int64_t len = q + (k < r ? 1 : 0);
      sub.push_back({off, len});
      off += len;
    }
  }
  std::vector<uint32_t> key(sub.size());
  for (size_t i = 0; i < sub.size(); ++i) {
    const uint32_t* me = &W.h[W.order[sub[i].start] * W.N3];
    key[i] = *std::min_element(me, me + W.N3);
  }
  std::vector<size_t> idx(sub.size());
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
    if (sub[x].len != sub[y].len) return sub[x].len > sub[y].len;
    return key[x] < key[y];
  });
  W.sub.resize(sub.size());
  for (size_t i = 0; i < idx.size(); ++i) W.sub[i] = sub[idx[i]];
}

// 5. workgroups of S equal-length sub-chains.  With the y-merge the S
//    slots form a GY x GZ grid: row r of a workgroup is GZ sub-chains that
//    follow each other along xi2 (xi2 = n-1 face of one = xi2 = 0 face of
//    the next at every step), row r + 1 the xi1-neighbours of row r.  A
//    workgroup whose first row cannot be completed (mesh edge, irregular
//    numbering) takes the next free sub-chains of its length in order, as
//    without the y-merge; so does the rest of a grid that ends early.
int workgroups(Work& W, const HexPlanOptions& opt, HexPlan& P) {
  const std::vector<uint32_t>& h = W.h;
  const std::vector<Sub>& sub = W.sub;
  const std::vector<int64_t>& order = W.order;
  const int N = W.N, N2 = W.N2, S = W.S, GZ = W.GZ, GY = W.GY;
  const int64_t N3 = W.N3;
  W.grid = opt.zmerge && opt.ymerge && GY >= 2;
  const size_t nsub = sub.size();
  // same-length neighbour along xi2 (kind 0) / xi1 (kind 1): its face 0
  // equals my face n-1 at every step
  auto face_ptr = [&](int64_t e, int kind, int side, int& st1, int& st2) -> const uint32_t* {
    // kind 0: xi2 face c = side: entries (a, b) at a*N2 + b*N; kind 1: xi1
    // face b = side: entries (a, c) at a*N2 + c
    if (kind == 0) {
      st1 = N2;
      st2 = N;
      return &h[e * N3 + side];
    }
    st1 = N2;
    st2 = 1;
    return &h[e * N3 + (int64_t)side * N];
  };
  auto same_faces = [&](int64_t i, int64_t j, int kind) -> bool {
    if (sub[i].len != sub[j].len) return false;
    for (int64_t k = 0; k < sub[i].len; ++k) {
      int a1, a2, b1, b2;
      const uint32_t* f1 = face_ptr(order[sub[i].start + k], kind, N - 1, a1, a2);
      const uint32_t* f2 = face_ptr(order[sub[j].start + k], kind, 0, b1, b2);
      for (int x = 0; x < N; ++x)
        for (int y = 0; y < N; ++y)
          if (f1[x * a1 + y * a2] != f2[x * b1 + y * b2]) return false;
    }
    return true;
  };
  std::vector<int64_t> nbr[2];
  if (W.grid)
    for (int kind = 0; kind < 2; ++kind) {
      nbr[kind].assign(nsub, -1);
      std::unordered_map<uint64_t, int64_t> head;
      head.reserve(nsub * 2);
      for (size_t j = 0; j < nsub; ++j) {
        int s1, s2;
        const uint32_t* f = face_ptr(order[sub[j].start], kind, 0, s1, s2);
        auto it = head.emplace(face_hash_strided(f, N, s1, s2), (int64_t)j);
        if (!it.second) it.first->second = -1;  // ambiguous
      }
      for (size_t i = 0; i < nsub; ++i) {
        int s1, s2;
        const uint32_t* f = face_ptr(order[sub[i].start], kind, N - 1, s1, s2);
        auto it = head.find(face_hash_strided(f, N, s1, s2));
        if (it == head.end() || it->second < 0 || it->second == (int64_t)i) continue;
        if (same_faces((int64_t)i, it->second, kind)) nbr[kind][i] = it->second;
      }
    }
  W.sub_wg.assign(nsub, -1);
  W.sub_slot.assign(nsub, -1);
  int64_t pos = 0;
  size_t cur = 0;  // first sub-chain not yet placed
  std::vector<int64_t> slots(S);
  while (true) {
    while (cur < nsub && W.sub_wg[cur] >= 0) ++cur;
    if (cur >= nsub) break;
    const int64_t len = sub[cur].len;
    const int64_t w = (int64_t)P.wg_off.size();
    std::fill(slots.begin(), slots.end(), -1);
    int filled = 0;
    bool is_grid = false;
    if (W.grid) {
      int64_t rs = (int64_t)cur;
      for (int r = 0; r < GY && rs >= 0; ++r) {
        int64_t x = rs;
        int zi = 0;
        for (; zi < GZ && x >= 0; ++zi) {
          bool taken = W.sub_wg[x] >= 0 || sub[x].len != len;
          for (int t = 0; t < filled + zi && !taken; ++t) taken = slots[t] == x;
          if (taken) break;
          slots[filled + zi] = x;
          x = zi + 1 < GZ ? nbr[0][x] : x;
        }
        if (zi < GZ) {  // incomplete row: drop it
          for (int t = filled; t < filled + zi; ++t) slots[t] = -1;
          break;
        }
        filled += GZ;
        rs = nbr[1][slots[filled - GZ]];
      }
      is_grid = filled >= 2 * GZ;
      if (!is_grid) {
        std::fill(slots.begin(), slots.end(), -1);
        filled = 0;
      }
    }
    // the rest: the next free sub-chains of this length, in order
    for (size_t j = cur; j < nsub && filled < S && sub[j].len == len; ++j) {
      if (W.sub_wg[j] >= 0) continue;
      bool taken = false;
      for (int t = 0; t < filled && !taken; ++t) taken = slots[t] == (int64_t)j;
      if (!taken) slots[filled++] = (int64_t)j;
    }
    if (pos > 0x7FFFFFFFll - len * S) return fail(SEM_E_INVALID, "hex plan: too many elements");
    P.wg_off.push_back((int)pos);
    P.wg_len.push_back((int)len);
    W.grid_wg.push_back(is_grid ? 1 : 0);
    for (int64_t k = 0; k < len; ++k)
      for (int s = 0; s < S; ++s)
        P.elist.push_back(slots[s] >= 0 ? (int)order[sub[slots[s]].start + k] : -1);
    for (int s = 0; s < S; ++s)
      if (slots[s] >= 0) {
        W.sub_wg[slots[s]] = w;
        W.sub_slot[slots[s]] = s;
      }
    pos += len * S;
  }
  return SEM_OK;
}

// 5b. z-merge: slot s of a workgroup hands its xi2 = 0 face to slot s-1
//     when, at every chain step, that face IS slot s-1's xi2 = n-1 face
//     node for node (same (a, b)); the kernel sums it in LDS.  In a grid
//     workgroup only within a row.  y-merge: slot s hands its xi1 = 0 face
//     to slot s - GZ likewise (same (a, c)).
void merge_flags(Work& W, const HexPlanOptions& opt, const HexPlan& P) {
  const std::vector<uint32_t>& h = W.h;
  const int N = W.N, N2 = W.N2, S = W.S, GZ = W.GZ;
  const int64_t N3 = W.N3, n_wg = (int64_t)P.wg_off.size();
  W.zm.assign(n_wg * S, 0);
  W.ym.assign(n_wg * S, 0);
  auto elem_at = [&](int64_t w, int64_t k, int s) { return P.elist[P.wg_off[w] + k * S + s]; };
  if (opt.zmerge)
    for (int64_t w = 0; w < n_wg; ++w)
      for (int s = 1; s < S; ++s) {
        if (W.grid_wg[w] && s % GZ == 0) continue;
        bool ok = true;
        for (int64_t k = 0; k < P.wg_len[w] && ok; ++k) {
          const int e1 = elem_at(w, k, s - 1), e2 = elem_at(w, k, s);
          if (e1 < 0 || e2 < 0) {
            ok = false;
            break;
          }
          const uint32_t* m1 = &h[(int64_t)e1 * N3];
          const uint32_t* m2 = &h[(int64_t)e2 * N3];
          for (int ab = 0; ab < N2 && ok; ++ab) ok = m1[ab * N + N - 1] == m2[ab * N];
        }
        W.zm[w * S + s] = ok ? 1 : 0;
      }
  if (W.grid)
    for (int64_t w = 0; w < n_wg; ++w) {
      if (!W.grid_wg[w]) continue;
      for (int s = GZ; s < S; ++s) {
        bool ok = true;
        for (int64_t k = 0; k < P.wg_len[w] && ok; ++k) {
          const int e1 = elem_at(w, k, s - GZ), e2 = elem_at(w, k, s);
          if (e1 < 0 || e2 < 0) {
            ok = false;
            break;
          }
          const uint32_t* m1 = &h[(int64_t)e1 * N3];
          const uint32_t* m2 = &h[(int64_t)e2 * N3];
          for (int a = 0; a < N && ok; ++a)
            for (int c = 0; c < N && ok; ++c) ok = m1[a * N2 + (N - 1) * N + c] == m2[a * N2 + c];
        }
        W.ym[w * S + s] = ok ? 1 : 0;
      }
    }
}

// The write rule of the element kernels (hex_store_column, sem_hex.h) for
// thread (b, c) of sub-chain i at step k, f the sub-chain's cflag: nothing
// where the column is handed over in LDS; otherwise every row but the carried
// one (a = n-1 of a non-last step), row 0 of the first step and row n-1 of
// the last being the head / tail face where f says they are slotted.
// fn(a, row kind) returns non-zero to stop; that value is returned.
enum RowKind { ROW_HEAD, ROW_TAIL, ROW_BODY };
template <class Fn>
int thread_rows(const Work& W, size_t i, int64_t k, int b, int c, uint8_t f, Fn&& fn) {
  if (W.merged(W.sub_wg[i], W.sub_slot[i], b, c)) return 0;
  const int N = W.N;
  const int64_t len = W.sub[i].len;
  for (int a = 0; a < N; ++a) {
    if (a == N - 1 && k < len - 1) continue;
    RowKind kind = ROW_BODY;
    if (a == 0 && k == 0 && (f & HEX_CF_HEAD))
      kind = ROW_HEAD;
    else if (a == N - 1 && k == len - 1 && (f & HEX_CF_TAIL))
      kind = ROW_TAIL;
    if (int rc = fn(a, kind)) return rc;
  }
  return 0;
}

// 6. events per node
void count_events(Work& W) {
  const int N = W.N, N2 = W.N2;
  W.cnt.assign(W.n_node, 0);
  for (size_t i = 0; i < W.sub.size(); ++i)
    for (int64_t k = 0; k < W.sub[i].len; ++k) {
      const uint32_t* me = W.elem(i, k);
      for (int b = 0; b < N; ++b)
        for (int c = 0; c < N; ++c)
          thread_rows(W, i, k, b, c, 0, [&](int a, RowKind) {
            uint8_t& n = W.cnt[me[a * N2 + b * N + c]];
            if (n < 255) ++n;
            return 0;
          });
    }
}

// 7. face flags, column masks
void flags_and_masks(const Work& W, HexPlan& P) {
  const int N = W.N, N2 = W.N2, S = W.S;
  for (size_t i = 0; i < W.sub.size(); ++i) {
    const int64_t len = W.sub[i].len, ws = W.sub_wg[i] * S + W.sub_slot[i];
    const uint32_t* hd = W.elem(i, 0);
    const uint32_t* tl = W.elem(i, len - 1) + (int64_t)(N - 1) * N2;
    uint8_t f = 0;
    for (int j = 0; j < N2; ++j) {
      if (W.cnt[hd[j]] > 1) f |= HEX_CF_HEAD;
      if (W.cnt[tl[j]] > 1) f |= HEX_CF_TAIL;
    }
    if (W.zm[ws]) f |= HEX_CF_ZGIVE;
    if (W.ym[ws]) f |= HEX_CF_YGIVE;
    P.cflag[ws] = f;
    for (int64_t k = 0; k < len; ++k) {
      const uint32_t* me = W.elem(i, k);
      unsigned long long mask = 0;
      for (int b = 0; b < N; ++b)
        for (int c = 0; c < N; ++c) {
          const int bcol = hex_bcol(N, b, c);
          if (bcol < 0) continue;
          thread_rows(W, i, k, b, c, f, [&](int a, RowKind kind) {
            if (kind != ROW_BODY || W.cnt[me[a * N2 + b * N + c]] <= 1) return 0;
            mask |= 1ull << bcol;
            return 1;
          });
        }
      P.cmask[P.wg_off[W.sub_wg[i]] + k * S + W.sub_slot[i]] = mask;
    }
  }
}

// 8. replay the kernel's rule: plain stores must hit one-event nodes; the
//    slotted events of each seam node, in a fixed order (counting sort)
int replay_and_seams(const Work& W, HexPlan& P) {
  const int N = W.N, N2 = W.N2, S = W.S;
  const int64_t n_node = W.n_node;
  // fn(node, slot index or -1 for a plain store)
  auto for_events = [&](auto&& fn) -> int {
    for (size_t i = 0; i < W.sub.size(); ++i) {
      const int w = (int)W.sub_wg[i], s = (int)W.sub_slot[i];
      const uint8_t f = P.cflag[w * S + s];
      for (int64_t k = 0; k < W.sub[i].len; ++k) {
        const int pos = P.wg_off[w] + (int)k * S + s;
        const uint32_t* me = W.elem(i, k);
        const unsigned long long mask = P.cmask[pos];
        for (int b = 0; b < N; ++b)
          for (int c = 0; c < N; ++c) {
            const int bc = b * N + c, bcol = hex_bcol(N, b, c);
            const bool colslot = bcol >= 0 && ((mask >> bcol) & 1ull);
            const int rc = thread_rows(W, i, k, b, c, f, [&](int a, RowKind kind) {
              int64_t sidx = -1;
              if (kind != ROW_BODY)
                sidx = hex_face_slot(N, P.face_base, w, s, kind == ROW_TAIL, bc);
              else if (colslot)
                sidx = hex_col_slot(N, pos, a, bcol);
              return fn(me[a * N2 + bc], sidx);
            });
            if (rc) return rc;
          }
      }
    }
    return SEM_OK;
  };
  std::vector<uint32_t> scount(n_node + 1, 0);
  int64_t n_direct = 0;
  int rc = for_events([&](uint32_t g, int64_t sidx) -> int {
    if (sidx < 0) {
      if (W.cnt[g] != 1)
        return fail(SEM_E_NOTIMPL,
                    "hex plan: a node inside an element column is shared (non-conforming mesh)");
      ++n_direct;
    } else {
      ++scount[g];
    }
    return SEM_OK;
  });
  if (rc) return rc;
  std::vector<uint32_t> start(n_node + 1, 0);
  for (int64_t g = 0; g < n_node; ++g) start[g + 1] = start[g] + scount[g];
  P.seam_idx.assign(start[n_node], 0);
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  for_events([&](uint32_t g, int64_t sidx) -> int {
    if (sidx >= 0) P.seam_idx[fill[g]++] = (uint32_t)sidx;
    return SEM_OK;
  });
  P.seam_ptr.push_back(0);
  for (int64_t g = 0; g < n_node; ++g) {
    if (scount[g]) {
      P.seam_gid.push_back((uint32_t)g);
      P.seam_ptr.push_back(start[g + 1]);
    }
    if (W.cnt[g] == 0) P.zero.push_back((uint32_t)g);
  }
  P.n_direct = n_direct;
  return SEM_OK;
}

}  // namespace

HexPlanOptions hex_plan_options_from_env() {
  HexPlanOptions o;
  if (const char* e = std::getenv("SEM_HEX_CHAIN_START")) o.chain_start = std::atof(e);
  if (const char* s = std::getenv("SEM_HEX_CHAIN")) o.chain_cap = std::max(1, std::atoi(s));
  return o;
}

int hex_plan_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node, int n,
                 const HexPlanOptions& opt, HexPlan& P) {
  for (size_t i = 0; i < e2n.size(); ++i)
    if (e2n[i] >= (uint64_t)n_node) return fail(SEM_E_INVALID, "element map entry >= n_node");
  Work W(e2n, n_elem, n_node, n);
  successors(W);
  maximal_chains(W);
  choose_length(W, opt);
  sub_chains(W);
  if (int rc = workgroups(W, opt, P)) return rc;
  const int64_t n_wg = (int64_t)P.wg_off.size(), n_pos = (int64_t)P.elist.size();
  P.cmask.assign(n_pos, 0ull);
  P.cflag.assign(n_wg * W.S, 0);
  P.face_base = hex_face_base(n, n_pos);
  P.n_slot = hex_n_slot(n, n_pos, n_wg);
  merge_flags(W, opt, P);
  count_events(W);
  flags_and_masks(W, P);
  if (P.n_slot >= 0xFFFFFFFFll) return fail(SEM_E_INVALID, "hex plan: slot space exceeds 2^32");
  if (int rc = replay_and_seams(W, P)) return rc;
  P.n_chains = W.n_chains();
  P.n_sub = (int64_t)W.sub.size();
  P.lc = W.lc;
  return SEM_OK;
}

bool hex_template_map(const std::vector<uint32_t>& e2n, int64_t n_elem, int n,
                      std::vector<int>& tmpl, std::vector<uint32_t>& ebase) {
  const int64_t N3 = (int64_t)n * n * n;
  tmpl.assign((size_t)N3, 0);
  ebase.clear();
  bool ok = n_elem > 0;
  for (int64_t i = 0; i < N3 && ok; ++i) {
    const int64_t d = (int64_t)e2n[i] - (int64_t)e2n[0];
    ok = d >= INT32_MIN && d <= INT32_MAX;
    tmpl[(size_t)i] = (int)d;
  }
  if (ok) ebase.resize((size_t)n_elem);
  for (int64_t e = 0; e < n_elem && ok; ++e) {
    const uint32_t* me = &e2n[(size_t)e * N3];
    ebase[(size_t)e] = me[0];
    for (int64_t i = 1; i < N3 && ok; ++i) ok = me[i] == me[0] + (uint32_t)tmpl[(size_t)i];
  }
  if (!ok) {
    tmpl.clear();
    ebase.clear();
  }
  return ok;
}

}  // namespace semhexplan
