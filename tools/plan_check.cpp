// Stand-alone checker of the 2-D scatter planner (csrc/sem_plan.cpp), CPU only:
//
//   plan_check MAP N N_ELEM N_NODE DPN MFMA [STATE]
//
// MAP: raw little-endian uint32 element map [N_ELEM][N][N]; STATE: optional
// uint8 node states [N_NODE]; planner options from the environment, as in the
// library.  Plans the map, replays the plan in integers the way the kernels
// execute it (sem_kernels.h: k_poisson_apply, chain_emit, emit1, emit1_seam,
// load_map, k_seam_sum) and prints one JSON line: the error code, the plan's
// scalars, the violations found ("errors", empty when the plan is sound) and
// an FNV-1a digest of every array the library would upload.
//
// Build: c++ -std=c++17 -I<repo>/spectralelementmethod_amd/csrc
//        tools/plan_check.cpp spectralelementmethod_amd/csrc/sem_plan.cpp
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "sem_error.h"
#include "sem_plan.h"

using namespace semk;
using semplan::Plan;

namespace {
std::string g_error;
}
namespace sem {
void set_error(const std::string& msg) { g_error = msg; }
int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}
}  // namespace sem

namespace {

template <typename T>
bool read_file(const char* path, size_t count, std::vector<T>& out) {
  out.resize(count);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)(count * sizeof(T)));
  return (size_t)f.gcount() == count * sizeof(T);
}

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <typename T>
  void vec(const std::vector<T>& v) {
    const uint64_t n = v.size();
    bytes(&n, sizeof n);
    bytes(v.data(), v.size() * sizeof(T));
  }
  void num(int64_t v) { bytes(&v, sizeof v); }
};
template <typename T>
uint64_t digest(const std::vector<T>& v) {
  Fnv f;
  f.vec(v);
  return f.h;
}

std::vector<std::string> g_errors;
void err(const std::string& what, int64_t a = -1, int64_t b = -1) {
  if (g_errors.size() >= 8) return;
  std::string s = what;
  if (a >= 0) s += " " + std::to_string(a);
  if (b >= 0) s += " " + std::to_string(b);
  g_errors.push_back(s);
}

constexpr int64_t SENTINEL = int64_t(1) << 40;  // y of a node nothing has written
constexpr int64_t POISON = int64_t(1) << 50;    // a value no code may use
constexpr int64_t PRIOR = 1000;                 // y of a SEM_NODE_PRIOR node on entry
constexpr int64_t UNSET = INT64_MIN;

struct Replay {
  const Plan& P;
  const std::vector<uint8_t>& state;
  int64_t n_node;
  std::vector<int64_t> y, slot;
  // last STORE / RMW of each node: launch, chain, round, wave
  std::vector<int64_t> wl, wc;
  std::vector<int> wr, ww;

  Replay(const Plan& P_, const std::vector<uint8_t>& state_, int64_t n_node_)
      : P(P_), state(state_), n_node(n_node_), y(n_node_, SENTINEL), wl(n_node_, -1),
        wc(n_node_, -1), wr(n_node_, -1), ww(n_node_, -1) {
    for (int64_t i = 0; i < n_node; ++i)
      if (!state.empty() && (state[i] & SEM_NODE_PRIOR)) y[i] = PRIOR;
    for (uint32_t g : P.zero) y[g] = 0;
    if (P.seam) slot.assign((size_t)P.seam_ns * n_node, UNSET);
  }

  // one entry as emit1 / emit1_seam execute it
  void emit(uint32_t raw, int64_t v, int64_t launch, int64_t chain, int rd, int wave) {
    const uint32_t a = (raw >> CODE_SHIFT) & 3u, g = raw & GID_MASK;
    if (a == W_SKIP) return;
    if (g >= n_node) return err("entry past n_node", g);
    if (a == W_ATOMIC) {
      if (!P.seam) {
        y[g] += v;
        return;
      }
      if ((size_t)chain >= P.chain_colour.size() || P.chain_colour[chain] >= P.seam_ns)
        return err("seam chain without a colour", chain);
      int64_t& s = slot[(size_t)P.chain_colour[chain] * n_node + g];
      if (s != UNSET) err("seam slot written twice, node", g);
      s = v;
      return;
    }
    if (wl[g] == launch) {
      if (wc[g] != chain)
        err("node written by two chains of one launch", g);
      else if (wr[g] == rd && ww[g] != wave)
        err("node written by two waves of one round", g);
      else if (wr[g] != rd && !P.round_sync)
        err("node written in two rounds without round_sync", g);
    }
    wl[g] = launch, wc[g] = chain, wr[g] = rd, ww[g] = wave;
    y[g] = a == W_STORE ? v : y[g] + v;
  }

  // chains of groups (k_poisson_apply, chain_emit)
  void chains(int n) {
    const int epw = epw_of(n), lw = epw * n, CW = chain_waves_of(n), rounds = P.rounds;
    std::vector<int64_t> v((size_t)n * lw), pre, rowc((size_t)CW * lw);
    std::vector<int64_t> carry((size_t)2 * CW * n);  // [round parity][wave][row]
    for (size_t q = 0; q + 1 < P.colour_start.size(); ++q)
      for (int64_t ch = P.colour_start[q]; ch < P.colour_start[q + 1]; ++ch) {
        std::fill(rowc.begin(), rowc.end(), 0);
        std::fill(carry.begin(), carry.end(), POISON);
        for (int rd = 0; rd < rounds; ++rd)
          for (int w = 0; w < CW; ++w) {
            const int64_t g = (ch * rounds + rd) * CW + w;
            const uint32_t* raw = &P.mapP[(size_t)g * n * lw];
            const int real = P.slot_fill[g] * n;
            for (int r = 0; r < n; ++r)
              for (int l = 0; l < lw; ++l) v[r * lw + l] = l < real ? 1 : POISON;
            for (int l = 0; l < lw; ++l) {  // 1. the row carry goes to row 0 first
              const bool out = (raw[(n - 1) * lw + l] >> CODE_SHIFT) == W_ROWCARRY;
              const int64_t held = out ? v[(n - 1) * lw + l] : 0;
              v[l] += rowc[w * lw + l];
              rowc[w * lw + l] = held;
            }
            pre = v;  // 2. MERGE adds the next lane's pre-merge value
            for (int r = 0; r < n; ++r)
              for (int l = 0; l < lw; ++l)
                if ((raw[r * lw + l] >> CODE_SHIFT) & W_MERGE)
                  v[r * lw + l] += l + 1 < lw ? pre[r * lw + l + 1] : POISON;
            // 3. the last lane's column goes to lane 0 of the chain's next group
            int64_t* mine = &carry[((rd & 1) * CW + w) * n];
            for (int r = 0; r < n; ++r) mine[r] = v[r * lw + lw - 1];
            const int64_t* src = w > 0 ? mine - n : &carry[(((rd + 1) & 1) * CW + CW - 1) * n];
            for (int r = 0; r < n; ++r)
              if ((raw[r * lw] >> CODE_SHIFT) & W_CARRY) v[r * lw] += src[r];
            for (int r = 0; r < n; ++r)  // 4. / 5. the stores
              for (int l = 0; l < lw; ++l) emit(raw[r * lw + l], v[r * lw + l], (int64_t)q, ch, rd, w);
          }
      }
  }

  // one element per slot (MFMA kernel): no merge, no carry
  void elements(int n) {
    for (size_t q = 0; q + 1 < P.colour_start.size(); ++q)
      for (int64_t s = P.colour_start[q]; s < P.colour_start[q + 1]; ++s)
        for (int t = 0; t < n * n; ++t) {
          const uint32_t raw = P.mapP[(size_t)s * n * n + t];
          if ((raw >> CODE_SHIFT) & ~3u) err("merge or carry code in an element plan, slot", s);
          emit(raw, 1, (int64_t)q, s, 0, 0);
        }
  }

  // k_seam_sum, then every node against its reference count
  void finish(const std::vector<uint32_t>& cnt) {
    int64_t used = 0, written = 0;
    for (size_t i = 0; i < P.seam_gid.size(); ++i) {
      const uint32_t g = P.seam_gid[i], m = P.seam_mask[i];
      const bool prior = !state.empty() && (state[g] & SEM_NODE_PRIOR);
      if (((m & 0x100u) != 0) != prior) err("seam mask prior bit, node", g);
      int64_t s = prior ? y[g] : 0;
      for (int c = 0; c < 8; ++c)
        if (m & (1u << c)) {
          const int64_t t = c < P.seam_ns ? slot[(size_t)c * n_node + g] : UNSET;
          if (t == UNSET) err("seam mask names an unwritten slot, node", g);
          s += t;
          ++used;
        }
      y[g] = s;
    }
    for (int64_t t : slot) written += t != UNSET;
    if (written != used) err("seam slots written but never summed", written - used);
    for (int64_t g = 0; g < n_node; ++g) {
      const uint8_t st = state.empty() ? 0 : state[g];
      int64_t want = cnt[g] + ((st & SEM_NODE_PRIOR) ? PRIOR : 0);
      if (!cnt[g] && !(st & SEM_NODE_PRIOR)) want = st ? SENTINEL : 0;
      if (y[g] != want) err("node value after the replay, node", g, y[g] < 0 ? 0 : y[g]);
    }
  }
};

// (c) the 16-bit map and its pattern table decode to mapP (load_map)
void check_map16(const Plan& P, int n, int lw) {
  const size_t blk = (size_t)n * lw;
  if (P.mbase.size() != (size_t)P.n_slots * n) return err("mbase size");
  if (P.m16.size() != (P.map_pat ? (size_t)P.n_map_pat : (size_t)P.n_slots) * blk)
    return err("m16 size");
  const int Q = map_pattern_id_rows(n);
  int64_t wide = 0, filled = 0;
  std::vector<uint32_t> b(n);
  for (int64_t sl = 0; sl < P.n_slots; ++sl) {
    filled += P.slot_fill[sl] ? 1 : 0;
    for (int r = 0; r < n; ++r) b[r] = P.mbase[(size_t)sl * n + r];
    if (b[0] == M16_WIDE) {
      ++wide;
      continue;
    }
    int64_t pid = sl;
    if (P.map_pat) {
      pid = 0;
      for (int q = 1; q <= Q; ++q) {
        pid |= (int64_t)(b[q] >> 28) << (4 * (q - 1));
        b[q] &= GID_MASK;
      }
      if (pid >= P.n_map_pat) return err("pattern id past the table, slot", sl);
    }
    const uint16_t* o = &P.m16[(size_t)pid * blk];
    const uint32_t* want = &P.mapP[(size_t)sl * blk];
    const int real = P.slot_fill[sl] * n;
    for (int r = 0; r < n; ++r)
      for (int l = 0; l < lw; ++l) {
        const uint32_t e = o[r * lw + l];
        const uint32_t raw = (b[r] + (e & M16_OFF_MASK)) | ((e >> M16_CODE_SHIFT) << CODE_SHIFT);
        // padding lanes: only the code is executed (SKIP)
        if (l < real ? raw != want[r * lw + l] : (raw ^ want[r * lw + l]) >> CODE_SHIFT)
          return err("16-bit map differs from mapP, slot", sl, r * lw + l);
      }
  }
  if (wide * 16 > filled) err("more than 1/16 of the groups are wide", wide, filled);
}

// (d) bookkeeping
void check_books(const Plan& P, const std::vector<uint32_t>& e2n, int64_t n_elem, int64_t n_node,
                 int n, int epw, bool mfma, const std::vector<uint32_t>& cnt) {
  const int lw = epw * n, nn = n * n;
  const int64_t CH = mfma ? 1 : (int64_t)chain_waves_of(n) * P.rounds;
  if (P.colour_start.empty() || P.colour_start[0] != 0) return err("colour_start");
  for (size_t q = 0; q + 1 < P.colour_start.size(); ++q)
    if (P.colour_start[q + 1] < P.colour_start[q]) return err("colour_start decreases");
  if (P.n_slots != P.colour_start.back() * CH) err("n_slots is not the sum over launches");
  if ((int64_t)P.slot_fill.size() != P.n_slots || P.mapP.size() != (size_t)P.n_slots * n * lw ||
      (int64_t)P.epos.size() != n_elem || (int64_t)P.owner.size() != n_node)
    return err("array sizes");
  if (P.seam && (int64_t)P.chain_colour.size() != P.colour_start.back()) err("chain_colour size");
  if (P.seam_gid.size() != P.seam_mask.size()) err("seam_gid / seam_mask sizes");
  std::vector<uint8_t> taken((size_t)P.n_slots * epw, 0);
  int64_t fill = 0;
  for (uint8_t f : P.slot_fill) fill += f;
  if (fill != n_elem) err("slot_fill does not sum to n_elem", fill);
  for (int64_t e = 0; e < n_elem; ++e) {
    const int64_t pos = P.epos[e];
    if (pos < 0 || pos >= P.n_slots * epw) return err("epos out of range, element", e);
    const int64_t sl = pos / epw, k = pos % epw;
    if (k >= P.slot_fill[sl]) err("epos on a padding lane, element", e);
    if (taken[pos]++) err("epos not injective, element", e);
    for (int r = 0; r < n; ++r)
      for (int jj = 0; jj < n; ++jj)
        if ((P.mapP[((size_t)sl * n + r) * lw + k * n + jj] & GID_MASK) != e2n[e * nn + r * n + jj])
          return err("mapP does not hold the element's nodes, element", e);
  }
  for (size_t i = 0; i < P.zero.size(); ++i) {
    if (i && P.zero[i] <= P.zero[i - 1]) return err("zero list not sorted and duplicate-free");
    if (P.zero[i] >= n_node) return err("zero list entry past n_node");
  }
  std::vector<uint32_t> first(n_node, 0xFFFFFFFFu);
  for (int64_t t = n_elem * nn - 1; t >= 0; --t) first[e2n[t]] = (uint32_t)(t / nn);
  if (first != P.owner) err("owner is not the first element referencing each node");
  int64_t n_rmw = 0;
  for (uint32_t e : P.mapP) n_rmw += ((e >> CODE_SHIFT) & 3u) == W_RMW;
  if (!P.ecol && n_rmw != P.n_rmw) err("n_rmw", P.n_rmw, n_rmw);
  (void)cnt;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: plan_check MAP N N_ELEM N_NODE DPN MFMA [STATE]\n");
    return 2;
  }
  const int n = std::atoi(argv[2]);
  const int64_t n_elem = std::atoll(argv[3]), n_node = std::atoll(argv[4]);
  const int dpn = std::atoi(argv[5]);
  const bool mfma = std::atoi(argv[6]) != 0;
  std::vector<uint32_t> e2n;
  std::vector<uint8_t> state;
  if (n < 2 || n > 17 || n_elem < 1 || n_node < 1 ||
      !read_file(argv[1], (size_t)n_elem * n * n, e2n) ||
      (argc > 7 && !read_file(argv[7], (size_t)n_node, state))) {
    std::fprintf(stderr, "plan_check: bad sizes or short input file\n");
    return 2;
  }
  Plan P;
  const int rc = semplan::plan_map(e2n, n_elem, n_node, n, dpn, mfma, state,
                                   semplan::plan_options_from_env(), P);
  if (rc) {
    std::printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, g_error.c_str());
    return 0;
  }
  const int epw = mfma ? 1 : epw_of(n);
  std::vector<uint32_t> cnt(n_node, 0);
  for (uint32_t g : e2n) cnt[g]++;
  check_books(P, e2n, n_elem, n_node, n, epw, mfma, cnt);
  if (g_errors.empty()) {
    Replay R(P, state, n_node);
    for (uint32_t g : P.zero)
      if (!state.empty() && state[g]) err("zero list holds a marked node", g);
    if (P.seam && P.n_atomic_groups) err("seam plan with atomic chains");
    if (mfma)
      R.elements(n);
    else
      R.chains(n);
    R.finish(cnt);
    if (P.map16) check_map16(P, n, epw * n);
  }
  Fnv sc;
  for (int64_t v : {(int64_t)P.rounds, (int64_t)P.blocks, P.row_carries, (int64_t)P.round_sync,
                    (int64_t)P.ecol, (int64_t)P.seam, (int64_t)P.seam_ns, P.n_slots,
                    P.n_atomic_groups, (int64_t)P.conforming, P.n_rmw, (int64_t)P.map16,
                    (int64_t)P.map_pat, P.n_map_pat})
    sc.num(v);
  std::printf("{\"rc\": 0, \"rounds\": %d, \"blocks\": %d, \"row_carries\": %" PRId64
              ", \"round_sync\": %d, \"ecol\": %d, \"seam\": %d, \"seam_ns\": %d, \"n_seam\": %zu"
              ", \"n_slots\": %" PRId64 ", \"n_chains\": %" PRId64 ", \"n_atomic_groups\": %" PRId64
              ", \"conforming\": %d, \"n_rmw\": %" PRId64 ", \"map16\": %d, \"map_pat\": %d"
              ", \"n_map_pat\": %" PRId64 ", \"zero\": [",
              P.rounds, (int)P.blocks, P.row_carries, (int)P.round_sync, (int)P.ecol, (int)P.seam,
              P.seam_ns, P.seam_gid.size(), P.n_slots, P.colour_start.back(), P.n_atomic_groups,
              (int)P.conforming, P.n_rmw, (int)P.map16, (int)P.map_pat, P.n_map_pat);
  for (size_t i = 0; i < P.zero.size() && i < 64; ++i) std::printf("%s%u", i ? ", " : "", P.zero[i]);
  std::printf("], \"n_zero\": %zu, \"errors\": [", P.zero.size());
  for (size_t i = 0; i < g_errors.size(); ++i)
    std::printf("%s\"%s\"", i ? ", " : "", g_errors[i].c_str());
  std::printf("], \"digests\": {\"mapP\": \"%016" PRIx64 "\", \"epos\": \"%016" PRIx64
              "\", \"zero\": \"%016" PRIx64 "\", \"owner\": \"%016" PRIx64
              "\", \"colour_start\": \"%016" PRIx64 "\", \"chain_colour\": \"%016" PRIx64
              "\", \"seam_gid\": \"%016" PRIx64 "\", \"seam_mask\": \"%016" PRIx64
              "\", \"m16\": \"%016" PRIx64 "\", \"mbase\": \"%016" PRIx64
              "\", \"scalars\": \"%016" PRIx64 "\"}}\n",
              digest(P.mapP), digest(P.epos), digest(P.zero), digest(P.owner),
              digest(P.colour_start), digest(P.chain_colour), digest(P.seam_gid),
              digest(P.seam_mask), digest(P.m16), digest(P.mbase), sc.h);
  return 0;
}
