// Stand-alone checker of the hexahedral scatter planner
// (csrc/sem_hex_plan.cpp), CPU only:
//
//   hex_plan_check MAP N N_ELEM N_NODE RESIDENT ZMERGE YMERGE FORM
//
// MAP: raw little-endian uint32 element map [N_ELEM][N][N][N]; RESIDENT: the
// workgroups resident on the device (sub-chain length rule); FORM:
// three_block, rows or mfma, the kernel whose rule is replayed;
// SEM_HEX_CHAIN / SEM_HEX_CHAIN_START from the environment, as in the
// library.  Plans the map, replays the plan the way that kernel executes it
// (sem_hex.h k_hex_poisson / k_hex_rows, sem_hex_mfma.h k_hex_mfma, then
// k_hex_seam_sum): thread by thread, every value carrying the global node it
// belongs to and the number of (element, local node) pairs summed into it.
// Prints one JSON line: the error code, the plan's scalars, the violations
// found ("errors", empty when the plan is sound) and an FNV-1a digest of
// every array the library would upload.
//
// The replay follows the kernels' text, not the planner's: it shares the
// vocabulary of sem_hex_plan.h (slot counts, hex_bcol, the flag names, the
// slot addressing) and nothing else with sem_hex_plan.cpp.
//
// Build: c++ -std=c++17 -I<repo>/spectralelementmethod_amd/csrc
//        tools/hex_plan_check.cpp spectralelementmethod_amd/csrc/sem_hex_plan.cpp
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "sem_error.h"
#include "sem_hex_plan.h"

using namespace semh;
using semhexplan::HexPlan;

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

bool read_file(const char* path, size_t count, std::vector<uint32_t>& out) {
  out.resize(count);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)(count * sizeof(uint32_t)));
  return (size_t)f.gcount() == count * sizeof(uint32_t);
}

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  void num(int64_t v) { bytes(&v, sizeof v); }
};
template <typename T>
uint64_t digest(const std::vector<T>& v) {
  Fnv f;
  f.num((int64_t)v.size());
  if (!v.empty()) f.bytes(v.data(), v.size() * sizeof(T));
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

enum Form { THREE_BLOCK, ROWS, MFMA };

// a value in a register, in LDS or in a slot: the node it belongs to and how
// many (element, local node) contributions it holds
struct Val {
  int64_t node = -1, count = 0;
};

struct Replay {
  const HexPlan& P;
  const std::vector<uint32_t>& map;
  const int N, N2, N3, S, NBC, GZ;
  const Form form;
  const int64_t n_node;
  std::vector<Val> slot;           // the slot space
  std::vector<int64_t> y;          // y[g] after the plain stores: count, -1 = not written
  std::vector<uint8_t> slot_used;  // listed in a seam list

  Replay(const HexPlan& P_, const std::vector<uint32_t>& map_, int n, Form form_, int64_t n_node_)
      : P(P_), map(map_), N(n), N2(n * n), N3(n * n * n), S(hex_slots(n)), NBC(hex_nbc(n)),
        GZ(hex_grid_z(n)), form(form_), n_node(n_node_), slot((size_t)P_.n_slot),
        y((size_t)n_node_, -1), slot_used((size_t)P_.n_slot, 0) {}

  void add(Val& v, const Val& o, const char* what, int64_t w) {
    if (v.node != o.node) err(std::string(what) + ": the two sides name different nodes, workgroup", w);
    v.count += o.count;
  }
  void to_slot(int64_t idx, const Val& v) {
    if (idx < 0 || idx >= P.n_slot) return err("slot index at or past n_slot", idx);
    if (slot[idx].node >= 0) return err("slot written twice", idx);
    if (y[v.node] >= 0) err("node with a plain store and a slot", v.node);
    slot[idx] = v;
  }
  void store(const Val& v) {
    if (y[v.node] >= 0) return err("node with two plain stores", v.node);
    y[v.node] = v.count;
  }

  // one workgroup, as the element kernel of the form runs it
  void workgroup(int w) {
    const int L = P.wg_len[w], base = P.wg_off[w];
    const bool mfma = form == MFMA, rows = form == ROWS;
    // y-merge: compiled into the three-block kernel where the grid has rows
    const bool YM = form == THREE_BLOCK && GZ < S;
    const int T = S * N2;  // threads with s < S (the others are never active)
    struct Thread {
      bool active, give, take, ygive, ytake;
      int s, sl, b, c, bc, bcol;
      uint8_t cf;
      Val carry;
    };
    std::vector<Thread> th(T);
    bool wg_merge = false;
    if (!mfma)
      for (int t = 1; t < S; ++t)
        wg_merge |= (P.cflag[w * S + t] & (rows ? HEX_CF_ZGIVE : HEX_CF_ZGIVE | HEX_CF_YGIVE)) != 0;
    for (int tid = 0; tid < T; ++tid) {
      Thread& t = th[tid];
      t.s = tid / N2;
      t.bc = tid - t.s * N2;
      t.b = t.bc / N, t.c = t.bc - t.b * N;
      t.bcol = hex_bcol(N, t.b, t.c);
      t.give = t.take = t.ygive = t.ytake = false;
      if (mfma) {  // k_hex_mfma: one slot, no flag but head / tail is read
        t.active = true;
        t.sl = 0;
        t.cf = P.cflag[w];
        if (P.elist[base] < 0) err("empty slot in a matrix-core plan, workgroup", w);
        if (t.cf & (HEX_CF_ZGIVE | HEX_CF_YGIVE)) err("merge flag in a matrix-core plan, workgroup", w);
        continue;
      }
      t.active = P.elist[base + t.s] >= 0;
      t.sl = t.active ? t.s : 0;
      t.cf = t.active ? P.cflag[w * S + t.s] : 0;
      t.give = (t.cf & HEX_CF_ZGIVE) && t.c == 0;
      t.take = t.active && t.c == N - 1 && t.s + 1 < S && (P.cflag[w * S + t.s + 1] & HEX_CF_ZGIVE);
      if (YM) {
        t.ygive = (t.cf & HEX_CF_YGIVE) && t.b == 0 && t.s >= GZ &&
                  !(t.c == 0 && ((t.cf & HEX_CF_ZGIVE) || (P.cflag[w * S + t.s - GZ] & HEX_CF_ZGIVE)));
        if (t.active && t.b == N - 1 && t.s + GZ < S) {
          const uint8_t cg = P.cflag[w * S + t.s + GZ];
          t.ytake = (cg & HEX_CF_YGIVE) && !(t.c == 0 && ((cg & HEX_CF_ZGIVE) || (t.cf & HEX_CF_ZGIVE)));
        }
        if ((t.cf & HEX_CF_YGIVE) && t.s < GZ) err("y-give flag in the first grid row, workgroup", w);
      } else if (t.cf & HEX_CF_YGIVE) {
        err("y-give flag in a plan for a kernel without the y-merge, workgroup", w);
      }
      if (t.give && t.s == 0) err("z-give flag in slot 0, workgroup", w);
      if ((t.give || t.take || t.ygive || t.ytake) && !wg_merge)
        err("hand-over in a workgroup that skips the merge, workgroup", w);
    }
    // the LDS exchange: [receiving slot][a][b] (z), [receiving slot][a][c] (y)
    std::vector<Val> xz((size_t)S * N2), xy((size_t)S * N2);
    std::vector<uint8_t> zw((size_t)S * N2), yw((size_t)S * N2);
    std::vector<Val> yv((size_t)T * N);
    for (int k = 0; k < L; ++k) {
      for (int tid = 0; tid < T; ++tid) {
        const Thread& t = th[tid];
        if (!t.active) continue;
        const int e = P.elist[base + k * (mfma ? 1 : S) + t.s];
        if (e < 0) {
          err("empty slot below a real one, workgroup", w, t.s);
          return;
        }
        for (int a = 0; a < N; ++a) yv[(size_t)tid * N + a] = Val{map[(size_t)e * N3 + a * N2 + t.bc], 1};
      }
      if (wg_merge) {
        std::fill(zw.begin(), zw.end(), 0);
        std::fill(yw.begin(), yw.end(), 0);
        for (int tid = 0; tid < T; ++tid) {
          const Thread& t = th[tid];
          if (t.give && t.s > 0 && (!rows || t.active))
            for (int a = 0; a < N; ++a) {
              xz[(size_t)(t.sl - 1) * N2 + a * N + t.b] = yv[(size_t)tid * N + a];
              zw[(size_t)(t.sl - 1) * N2 + a * N + t.b] = 1;
            }
        }
        for (int tid = 0; tid < T; ++tid) {
          const Thread& t = th[tid];
          if (!t.take) continue;
          for (int a = 0; a < N; ++a) {
            uint8_t& f = zw[(size_t)t.sl * N2 + a * N + t.b];
            if (f != 1) err("z-take without its give, workgroup", w, t.s);
            else add(yv[(size_t)tid * N + a], xz[(size_t)t.sl * N2 + a * N + t.b], "z-merge", w);
            f = 2;
          }
        }
        for (uint8_t f : zw)
          if (f == 1) {
            err("z-give without its take, workgroup", w);
            break;
          }
        if (YM) {
          for (int tid = 0; tid < T; ++tid) {
            const Thread& t = th[tid];
            if (t.ygive)
              for (int a = 0; a < N; ++a) {
                xy[(size_t)(t.sl - GZ) * N2 + a * N + t.c] = yv[(size_t)tid * N + a];
                yw[(size_t)(t.sl - GZ) * N2 + a * N + t.c] = 1;
              }
          }
          for (int tid = 0; tid < T; ++tid) {
            const Thread& t = th[tid];
            if (!t.ytake) continue;
            for (int a = 0; a < N; ++a) {
              uint8_t& f = yw[(size_t)t.sl * N2 + a * N + t.c];
              if (f != 1) err("y-take without its give, workgroup", w, t.s);
              else add(yv[(size_t)tid * N + a], xy[(size_t)t.sl * N2 + a * N + t.c], "y-merge", w);
              f = 2;
            }
          }
          for (uint8_t f : yw)
            if (f == 1) {
              err("y-give without its take, workgroup", w);
              break;
            }
        }
      }
      // the stores
      for (int tid = 0; tid < T; ++tid) {
        Thread& t = th[tid];
        if (!t.active || t.give || t.ygive) continue;
        Val* v = &yv[(size_t)tid * N];
        const int pos = base + k * (mfma ? 1 : S) + t.s;
        if (k > 0) add(v[0], t.carry, "carry", w);
        const bool last = k == L - 1;
        if (!last) t.carry = v[N - 1];
        const bool colslot = t.bcol >= 0 && ((P.cmask[pos] >> t.bcol) & 1ull);
        for (int a = 0; a < N; ++a) {
          if (a == N - 1 && !last) continue;
          if (a == 0 && k == 0 && (t.cf & HEX_CF_HEAD))
            to_slot(hex_face_slot(N, P.face_base, w, t.sl, 0, t.bc), v[a]);
          else if (a == N - 1 && last && (t.cf & HEX_CF_TAIL))
            to_slot(hex_face_slot(N, P.face_base, w, t.sl, 1, t.bc), v[a]);
          else if (colslot)
            to_slot(hex_col_slot(N, pos, a, t.bcol), v[a]);
          else
            store(v[a]);
        }
      }
    }
  }

  // k_hex_seam_sum (overwrite mode), then every node against its reference count
  void finish(const std::vector<uint32_t>& cnt) {
    const size_t ns = P.seam_gid.size();
    if (P.seam_ptr.size() != ns + 1 || P.seam_ptr[0] != 0 || P.seam_ptr[ns] != P.seam_idx.size())
      return err("seam_ptr does not span seam_idx");
    for (size_t i = 0; i < ns; ++i) {
      const uint32_t g = P.seam_gid[i];
      if (g >= n_node) return err("seam node past n_node", g);
      if (P.seam_ptr[i + 1] < P.seam_ptr[i]) return err("seam_ptr decreases");
      if (y[g] >= 0) err("node with a plain store and a seam sum", g);
      int64_t sum = 0;
      for (uint32_t j = P.seam_ptr[i]; j < P.seam_ptr[i + 1]; ++j) {
        const uint32_t idx = P.seam_idx[j];
        if (idx >= P.n_slot) return err("seam_idx at or past n_slot", idx);
        if (slot[idx].node < 0) err("seam_idx names a slot never written", idx);
        else if (slot[idx].node != g) err("seam sum adds a slot of another node, node", g);
        if (slot_used[idx]++) err("slot in two seam lists", idx);
        sum += slot[idx].count;
      }
      y[g] = sum;
    }
    for (int64_t i = 0; i < P.n_slot; ++i)
      if (slot[i].node >= 0 && !slot_used[i]) {
        err("written slot in no seam list", i);
        break;
      }
    std::vector<uint32_t> unref;
    for (int64_t g = 0; g < n_node; ++g) {
      if (!cnt[g]) unref.push_back((uint32_t)g);
      if (y[g] != (cnt[g] ? (int64_t)cnt[g] : -1))
        err("node value after the replay, node", g, y[g] < 0 ? 0 : y[g]);
    }
    if (unref != P.zero) err("zero list is not the unreferenced nodes");
  }
};

// sizes and bounds of the launch tables, elist a permutation of the elements
bool check_books(const HexPlan& P, int n, int64_t n_elem, Form form) {
  const int S = hex_slots(n);
  const size_t n_wg = P.wg_off.size();
  if (form == MFMA && S != 1) return err("the matrix-core form needs one slot per workgroup"), false;
  if (P.wg_len.size() != n_wg || P.cflag.size() != n_wg * S || P.cmask.size() != P.elist.size())
    return err("array sizes"), false;
  if (P.face_base != hex_face_base(n, (int64_t)P.elist.size()) ||
      P.n_slot != hex_n_slot(n, (int64_t)P.elist.size(), (int64_t)n_wg))
    return err("face_base / n_slot"), false;
  int64_t pos = 0;
  for (size_t w = 0; w < n_wg; ++w) {
    if (P.wg_off[w] != pos || P.wg_len[w] < 1) return err("wg_off / wg_len, workgroup", w), false;
    pos += (int64_t)P.wg_len[w] * S;
  }
  if (pos != (int64_t)P.elist.size()) return err("launch positions"), false;
  std::vector<uint8_t> seen((size_t)n_elem, 0);
  for (int e : P.elist) {
    if (e < -1 || e >= n_elem) return err("elist entry out of range"), false;
    if (e >= 0 && seen[e]++) return err("element twice in elist", e), false;
  }
  for (int64_t e = 0; e < n_elem; ++e)
    if (!seen[e]) return err("element missing from elist", e), false;
  return true;
}

// the sub-chains of the plan (the columns of its workgroups) grouped into the
// chains they were cut from: the longest sub-chain, and the largest
// difference of lengths within one chain
void sub_chain_lengths(const HexPlan& P, const std::vector<uint32_t>& map, int n, int64_t& longest,
                       int64_t& spread) {
  const int S = hex_slots(n), N2 = n * n;
  const int64_t N3 = (int64_t)N2 * n;
  struct Sub {
    int head, tail, len;
  };
  std::vector<Sub> sub;
  for (size_t w = 0; w < P.wg_off.size(); ++w)
    for (int s = 0; s < S; ++s)
      if (P.elist[P.wg_off[w] + s] >= 0)
        sub.push_back({P.elist[P.wg_off[w] + s], P.elist[P.wg_off[w] + (P.wg_len[w] - 1) * S + s],
                       P.wg_len[w]});
  std::map<std::vector<uint32_t>, int> heads;  // face a = 0 -> sub-chain, -1 = ambiguous
  for (size_t i = 0; i < sub.size(); ++i) {
    const uint32_t* f = &map[sub[i].head * N3];
    auto it = heads.emplace(std::vector<uint32_t>(f, f + N2), (int)i);
    if (!it.second) it.first->second = -1;
  }
  std::vector<int> root(sub.size());
  std::iota(root.begin(), root.end(), 0);
  auto find = [&](int i) {
    while (root[i] != i) i = root[i] = root[root[i]];
    return i;
  };
  for (size_t i = 0; i < sub.size(); ++i) {
    const uint32_t* f = &map[sub[i].tail * N3 + (int64_t)(n - 1) * N2];
    auto it = heads.find(std::vector<uint32_t>(f, f + N2));
    if (it != heads.end() && it->second >= 0) root[find((int)i)] = find(it->second);
  }
  std::vector<int> lo(sub.size(), INT32_MAX), hi(sub.size(), 0);
  longest = spread = 0;
  for (size_t i = 0; i < sub.size(); ++i) {
    const int r = find((int)i);
    lo[r] = std::min(lo[r], sub[i].len);
    hi[r] = std::max(hi[r], sub[i].len);
    longest = std::max<int64_t>(longest, sub[i].len);
  }
  for (size_t i = 0; i < sub.size(); ++i)
    if (hi[i]) spread = std::max<int64_t>(spread, hi[i] - lo[i]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr,
                 "usage: hex_plan_check MAP N N_ELEM N_NODE RESIDENT ZMERGE YMERGE FORM\n");
    return 2;
  }
  const int n = std::atoi(argv[2]);
  const int64_t n_elem = std::atoll(argv[3]), n_node = std::atoll(argv[4]);
  const std::string fname = argv[8];
  const Form form = fname == "rows" ? ROWS : fname == "mfma" ? MFMA : THREE_BLOCK;
  std::vector<uint32_t> e2n;
  if (n < HEX_MIN_N || n > HEX_MAX_N || n_elem < 1 || n_node < 1 ||
      (form == THREE_BLOCK && fname != "three_block") ||
      !read_file(argv[1], (size_t)n_elem * n * n * n, e2n)) {
    std::fprintf(stderr, "hex_plan_check: bad arguments or short input file\n");
    return 2;
  }
  semhexplan::HexPlanOptions opt = semhexplan::hex_plan_options_from_env();
  opt.resident = std::atoll(argv[5]);
  opt.zmerge = std::atoi(argv[6]) != 0;
  opt.ymerge = std::atoi(argv[7]) != 0;
  if (opt.ymerge && form != THREE_BLOCK) {
    std::fprintf(stderr, "hex_plan_check: the y-merge exists only in three_block\n");
    return 2;
  }
  HexPlan P;
  const int rc = semhexplan::hex_plan_map(e2n, n_elem, n_node, n, opt, P);
  if (rc) {
    std::printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, g_error.c_str());
    return 0;
  }
  std::vector<int> tmpl;
  std::vector<uint32_t> ebase;
  const bool tmap = semhexplan::hex_template_map(e2n, n_elem, n, tmpl, ebase);
  const int S = hex_slots(n);
  int64_t longest = 0, spread = 0;
  if (check_books(P, n, n_elem, form)) {
    std::vector<uint32_t> cnt((size_t)n_node, 0);
    for (uint32_t g : e2n) cnt[g]++;
    Replay R(P, e2n, n, form, n_node);
    for (size_t w = 0; w < P.wg_off.size() && g_errors.empty(); ++w) R.workgroup((int)w);
    if (g_errors.empty()) R.finish(cnt);
    sub_chain_lengths(P, e2n, n, longest, spread);
    if (tmap) {
      const size_t N3 = (size_t)n * n * n;
      bool same = tmpl.size() == N3 && ebase.size() == (size_t)n_elem;
      for (size_t t = 0; t < e2n.size() && same; ++t)
        same = e2n[t] == ebase[t / N3] + (uint32_t)tmpl[t % N3];
      if (!same) err("tmpl and ebase do not reproduce the map");
    } else if (!tmpl.empty() || !ebase.empty()) {
      err("tmpl or ebase without a template map");
    }
  }
  int64_t grid_wgs = 0, bit63 = 0;
  for (size_t w = 0; w < P.wg_off.size(); ++w) {
    bool yg = false;
    for (int s = 0; s < S; ++s) yg |= (P.cflag[w * S + s] & HEX_CF_YGIVE) != 0;
    grid_wgs += yg;
  }
  for (unsigned long long m : P.cmask) bit63 += (m >> 63) & 1ull;
  Fnv sl;
  sl.num(P.face_base);
  sl.num(P.n_slot);
  std::printf("{\"rc\": 0, \"n_wg\": %zu, \"n_pos\": %zu, \"n_chains\": %" PRId64
              ", \"n_sub\": %" PRId64 ", \"lc\": %" PRId64 ", \"n_seam\": %zu, \"n_seam_writes\": %zu"
              ", \"n_direct\": %" PRId64 ", \"grid_wgs\": %" PRId64 ", \"template_map\": %s"
              ", \"sub_len_max\": %" PRId64 ", \"sub_len_spread\": %" PRId64
              ", \"cmask_bit63\": %" PRId64 ", \"zero\": [",
              P.wg_off.size(), P.elist.size(), P.n_chains, P.n_sub, P.lc, P.seam_gid.size(),
              P.seam_idx.size(), P.n_direct, grid_wgs, tmap ? "true" : "false", longest, spread,
              bit63);
  for (size_t i = 0; i < P.zero.size() && i < 64; ++i) std::printf("%s%u", i ? ", " : "", P.zero[i]);
  std::printf("], \"errors\": [");
  for (size_t i = 0; i < g_errors.size(); ++i)
    std::printf("%s\"%s\"", i ? ", " : "", g_errors[i].c_str());
  std::printf("], \"digests\": {\"wg_off\": \"%016" PRIx64 "\", \"wg_len\": \"%016" PRIx64
              "\", \"elist\": \"%016" PRIx64 "\", \"cmask\": \"%016" PRIx64
              "\", \"cflag\": \"%016" PRIx64 "\", \"seam_gid\": \"%016" PRIx64
              "\", \"seam_ptr\": \"%016" PRIx64 "\", \"seam_idx\": \"%016" PRIx64
              "\", \"zero\": \"%016" PRIx64 "\", \"tmpl\": \"%016" PRIx64
              "\", \"ebase\": \"%016" PRIx64 "\", \"slots\": \"%016" PRIx64 "\"}}\n",
              digest(P.wg_off), digest(P.wg_len), digest(P.elist), digest(P.cmask), digest(P.cflag),
              digest(P.seam_gid), digest(P.seam_ptr), digest(P.seam_idx), digest(P.zero),
              digest(tmpl), digest(ebase), sl.h);
  return 0;
}
