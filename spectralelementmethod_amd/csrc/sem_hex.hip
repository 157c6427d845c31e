// Hexahedral (3-D) operator path of libsem_hip.so: the per-order launches of
// sem_hex.h and the 3-D halves of the C ABI entry points (sem_device.hip
// forwards a context created with ndim = 3 here); the scatter plan comes from
// sem_hex_plan.cpp.  DESIGN.md §4.9 / §5.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "sem_ctx.h"
#include "sem_hex.h"
#include "sem_hex_mfma.h"

using sem::fail;
using semd::DeviceGuard;
using semd::grid_for;
using semd::upload;

struct HexState {
  int N = 0, slots = 0, threads = 0, nbc = 0;
  // launch tables (HexLaunch)
  int64_t n_wg = 0, n_pos = 0;
  int* d_wg_off = nullptr;
  int* d_wg_len = nullptr;
  int* d_elist = nullptr;
  unsigned long long* d_cmask = nullptr;
  uint8_t* d_cflag = nullptr;
  double* d_slot = nullptr;
  int64_t face_base = 0, n_slot = 0;
  // seam sums: seam node i = gid[i] sums slot[idx[ptr[i] .. ptr[i+1])]
  uint32_t* d_seam_gid = nullptr;
  uint32_t* d_seam_ptr = nullptr;
  uint32_t* d_seam_idx = nullptr;
  int64_t n_seam = 0, n_seam_writes = 0;
  uint32_t* d_zero = nullptr;  // unreferenced nodes (overwrite mode zeroes them)
  int64_t n_zero = 0;
  uint32_t* d_map = nullptr;   // the library's copy of the caller's map [E][n][n][n]
  double* d_vx = nullptr;      // V_eq^-1 hi, lo (extended-precision inverse, p >= 11)
  double* d_G = nullptr;       // stored factors, 6 per element node (pair layout, sem_hex.h hex_g)
  bool have_G = false;
  // the action's kernel: k_hex_poisson (three-block, default) or k_hex_rows
  // (row form, SEM_HEX_ROWS=1; the diagonal always runs k_hex_poisson)
  bool rows = true;
  // the action on the fp64 matrix cores (k_hex_mfma; n = 12..17, on request:
  // SEM_KERNEL_MFMA at the time of sem_set_map); the diagonal keeps
  // k_hex_poisson
  bool mfma = false;
  // xi2 faces between the slots of a workgroup summed in LDS (both kernels;
  // SEM_HEX_ZMERGE=0 turns it off)
  bool zmerge = false;
  // xi1 faces between the rows of a workgroup's slot grid too (three-block
  // kernel only; SEM_HEX_YMERGE=0 turns it off)
  bool ymerge = false;
  // template map (HexLaunch::ebase / tmpl; both kernel forms): every
  // element's ids = its first node's id + one offset block (SEM_HEX_TMAP=0
  // turns it off)
  bool tmap = false;
  uint32_t* d_ebase = nullptr;
  int* d_tmpl = nullptr;
  // diagnostics (sem_plan_info)
  int64_t n_chains = 0, n_subchains = 0, chain_len = 0, n_direct = 0;

  void free_plan() {
    for (void* p : {(void*)d_wg_off, (void*)d_wg_len, (void*)d_elist, (void*)d_cmask,
                    (void*)d_cflag, (void*)d_slot, (void*)d_seam_gid, (void*)d_seam_ptr,
                    (void*)d_seam_idx, (void*)d_zero, (void*)d_ebase, (void*)d_tmpl})
      (void)hipFree(p);
    d_ebase = nullptr;
    d_tmpl = nullptr;
    tmap = false;
    d_wg_off = d_wg_len = d_elist = nullptr;
    d_cmask = nullptr;
    d_cflag = nullptr;
    d_slot = nullptr;
    d_seam_gid = d_seam_ptr = d_seam_idx = d_zero = nullptr;
    n_wg = n_pos = n_slot = n_seam = n_seam_writes = n_zero = 0;
  }
};

namespace {

#define SEM_TRY_RC(expr) \
  do {                     \
    int _rc = (expr);      \
    if (_rc) return _rc;   \
  } while (0)

int hex_check_order(int n) {
  if (n < semh::HEX_MIN_N || n > semh::HEX_MAX_N)
    return fail(SEM_E_NOTIMPL, "hexahedral kernels are built for orders 1.." +
                                   std::to_string(semh::HEX_MAX_N - 1));
  return SEM_OK;
}

// ---------------------------------------------------------------------------
// One element kernel: the three-block kernel (action and diagonal), the row
// form or the matrix-core form (the action only: HEX_SET / HEX_ACC; set_map
// turns HexState::mfma on only at the orders it is built for), with or
// without the template map, in the mode asked for
enum { HEX_FORM_THREE_BLOCK, HEX_FORM_ROWS, HEX_FORM_MFMA };

template <int N, int FORM, bool TM>
void launch_hex_form(const HexState* H, const semh::HexLaunch& L, int mode, const double* u,
                     double* y, const double* d_D, const semh::HexD<N>& Dk, hipStream_t st) {
  const dim3 g((unsigned)H->n_wg), b(semh::hex_threads(N));
  auto launch = [&](auto mode_c) {
    constexpr int MODE = decltype(mode_c)::value;
    if constexpr (FORM == HEX_FORM_MFMA)
      hipLaunchKernelGGL((semh::k_hex_mfma<N, MODE, TM>), g, b, 0, st, u, y, H->d_map, H->d_G, d_D,
                         L);
    else if constexpr (FORM == HEX_FORM_ROWS)
      hipLaunchKernelGGL((semh::k_hex_rows<N, MODE, TM>), g, b, 0, st, u, y, H->d_map, H->d_G, d_D,
                         L, Dk);
    else
      hipLaunchKernelGGL((semh::k_hex_poisson<N, MODE, TM>), g, b, 0, st, u, y, H->d_map, H->d_G,
                         d_D, L, Dk);
  };
  if (mode == semh::HEX_SET)
    launch(std::integral_constant<int, semh::HEX_SET>{});
  else if (mode == semh::HEX_ACC)
    launch(std::integral_constant<int, semh::HEX_ACC>{});
  else if constexpr (FORM == HEX_FORM_THREE_BLOCK)
    launch(std::integral_constant<int, semh::HEX_DIAG>{});
}

template <int N>
int launch_hex_apply(sem_ctx* c, int mode, const double* u, double* y, hipStream_t st) {
  HexState* H = c->hex;
  const semh::HexLaunch L{H->d_wg_off, H->d_wg_len, H->d_elist,   H->d_cmask,
                          H->d_cflag,  H->d_slot,   H->face_base, H->d_ebase, H->d_tmpl};
  semh::HexD<N> Dk;
  for (int i = 0; i < N * N; ++i) Dk.d[i] = c->hD[i];
  const bool action = mode != semh::HEX_DIAG;  // the diagonal always runs k_hex_poisson
  if (H->mfma && action) {
    if constexpr (N >= semh::HEX_MFMA_MIN_N && N <= semh::HEX_MFMA_MAX_N) {
      if (H->tmap)
        launch_hex_form<N, HEX_FORM_MFMA, true>(H, L, mode, u, y, c->d_D, Dk, st);
      else
        launch_hex_form<N, HEX_FORM_MFMA, false>(H, L, mode, u, y, c->d_D, Dk, st);
    }
  } else if (H->rows && action) {
    if (H->tmap)
      launch_hex_form<N, HEX_FORM_ROWS, true>(H, L, mode, u, y, c->d_D, Dk, st);
    else
      launch_hex_form<N, HEX_FORM_ROWS, false>(H, L, mode, u, y, c->d_D, Dk, st);
  } else {
    if (H->tmap)
      launch_hex_form<N, HEX_FORM_THREE_BLOCK, true>(H, L, mode, u, y, c->d_D, Dk, st);
    else
      launch_hex_form<N, HEX_FORM_THREE_BLOCK, false>(H, L, mode, u, y, c->d_D, Dk, st);
  }
  HIP_TRY(hipGetLastError());
  if (H->n_seam) {
    const dim3 gs(grid_for(H->n_seam, 256, 8192)), bs(256);
    if (mode == semh::HEX_ACC)
      hipLaunchKernelGGL(semh::k_hex_seam_sum<true>, gs, bs, 0, st, y, H->d_seam_gid,
                         H->d_seam_ptr, H->d_seam_idx, H->n_seam, H->d_slot);
    else
      hipLaunchKernelGGL(semh::k_hex_seam_sum<false>, gs, bs, 0, st, y, H->d_seam_gid,
                         H->d_seam_ptr, H->d_seam_idx, H->n_seam, H->d_slot);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

// from this many nodes per line (p >= 11) the equispaced -> GLL transform
// runs as three compensated passes (k_hex_eq2gll_pass) before k_hex_geom:
// float64 sums lose 7e-12 (p = 12) to 1e-8 (p = 16) of the action against
// the extended-precision oracle (oracle
// hex_poisson_apply_extended); at p <= 10 the plain passes stay (4.7e-13)
constexpr int HEX_DOT2_MIN_N = 12;

// V_eq^-1 as hi + lo doubles, from V_eq built and inverted in x87 extended
// precision on the GLL nodes of the context's basis: the float64 inverse the
// caller passes is itself off by ~cond(V_eq) eps (1e-11 at p = 16), which the
// compensated passes would otherwise carry into x_phys.  Only for the standard
// GLL basis (the baked table reproduces the context's D bit for bit);
// otherwise hi = the caller's inverse, lo = 0.
int eq2gll_hilo(sem_ctx* c, double* hi, double* lo) {
  const int n = c->n;
  std::vector<double> xn(n), bw(n), qw(n), D((size_t)n * n);
  bool gll = sem::gll_table(c->p, xn.data(), bw.data(), qw.data()) == SEM_OK;
  if (gll) {
    sem::diff_matrix(n, xn.data(), bw.data(), D.data());
    gll = std::memcmp(D.data(), c->hD, sizeof(double) * n * n) == 0;
  }
  if (!gll) {
    HIP_TRY(hipMemcpy(hi, c->d_Vinv, sizeof(double) * n * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n * n; ++i) lo[i] = 0.0;
    return SEM_OK;
  }
  std::vector<long double> a((size_t)n * 2 * n, 0.0L);
  for (int i = 0; i < n; ++i) {
    const long double x = -1.0L + 2.0L * i / (long double)(n - 1);
    int hit = -1;
    long double sum = 0.0L;
    for (int j = 0; j < n && hit < 0; ++j) {
      const long double d = x - (long double)xn[j];
      if (d == 0.0L) hit = j;
      else sum += (long double)bw[j] / d;
    }
    for (int j = 0; j < n; ++j)
      a[(size_t)i * 2 * n + j] =
          hit >= 0 ? (j == hit ? 1.0L : 0.0L) : ((long double)bw[j] / (x - (long double)xn[j])) / sum;
    a[(size_t)i * 2 * n + n + i] = 1.0L;
  }
  for (int col = 0; col < n; ++col) {  // Gauss-Jordan, partial pivoting
    int piv = col;
    for (int r = col + 1; r < n; ++r)
      if (fabsl(a[(size_t)r * 2 * n + col]) > fabsl(a[(size_t)piv * 2 * n + col])) piv = r;
    if (piv != col)
      for (int j = 0; j < 2 * n; ++j) std::swap(a[(size_t)col * 2 * n + j], a[(size_t)piv * 2 * n + j]);
    const long double dg = a[(size_t)col * 2 * n + col];
    for (int j = 0; j < 2 * n; ++j) a[(size_t)col * 2 * n + j] /= dg;
    for (int r = 0; r < n; ++r) {
      if (r == col) continue;
      const long double f = a[(size_t)r * 2 * n + col];
      for (int j = 0; j < 2 * n; ++j) a[(size_t)r * 2 * n + j] -= f * a[(size_t)col * 2 * n + j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const long double v = a[(size_t)i * 2 * n + n + j];
      hi[i * n + j] = (double)v;
      lo[i * n + j] = (double)(v - (long double)hi[i * n + j]);
    }
  return SEM_OK;
}

template <int N>
int launch_hex_geom(sem_ctx* c, const double* nodes, double* GP, double* xph, double* J,
                    double* iJ, double* dJ, double* dJW, hipStream_t st) {
  HexState* H = c->hex;
  constexpr int S = semh::hex_slots(N), N3 = N * N * N;
  const int64_t nb = std::min<int64_t>((c->n_elem + S - 1) / S, 16384);
  double* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  const double* xrel = nullptr;
  if constexpr (N >= HEX_DOT2_MIN_N) {
    // relative coordinates (R, Rl), then -> (A, Al) -> (R, Rl) -> A along xi0, xi1, xi2
    const int64_t total = c->n_elem * 3 * N3;
    if (!H->d_vx) HIP_TRY(hipMalloc(&H->d_vx, 2 * N * N * sizeof(double)));
    {
      std::vector<double> vx(2 * N * N);
      SEM_TRY_RC(eq2gll_hilo(c, vx.data(), vx.data() + N * N));
      HIP_TRY(hipMemcpy(H->d_vx, vx.data(), vx.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    for (double*& b : buf) HIP_TRY(hipMallocAsync((void**)&b, total * sizeof(double), st));
    const dim3 g(grid_for(total, 256, 16384)), bl(256);
    const double *vh = H->d_vx, *vl = H->d_vx + N * N;
    hipLaunchKernelGGL(semh::k_hex_rel_coords<N>, g, bl, 0, st, nodes, c->n_node, H->d_map,
                       c->n_elem, buf[0], buf[3]);
    hipLaunchKernelGGL((semh::k_hex_eq2gll_pass<N, 0>), g, bl, 0, st, buf[0], buf[3], buf[1],
                       buf[2], vh, vl, c->n_elem * 3);
    hipLaunchKernelGGL((semh::k_hex_eq2gll_pass<N, 1>), g, bl, 0, st, buf[1], buf[2], buf[0],
                       buf[3], vh, vl, c->n_elem * 3);
    hipLaunchKernelGGL((semh::k_hex_eq2gll_pass<N, 2>), g, bl, 0, st, buf[0], buf[3], buf[1],
                       nullptr, vh, vl, c->n_elem * 3);
    HIP_TRY(hipGetLastError());
    xrel = buf[1];
  }
  hipLaunchKernelGGL(semh::k_hex_geom<N>, dim3((unsigned)nb), dim3(semh::hex_threads(N)), 0, st,
                     nodes, c->n_node, H->d_map, c->n_elem, c->d_Vinv, c->d_D, c->d_w, GP, xph, J,
                     iJ, dJ, dJW, c->d_bad, xrel);
  HIP_TRY(hipGetLastError());
  for (double* b : buf)
    if (b) HIP_TRY(hipFreeAsync(b, st));
  return SEM_OK;
}

#define HEX_DISPATCH(rc, n, FN, ...)            \
  switch (n) {                                  \
    case 2: rc = FN<2>(__VA_ARGS__); break;     \
    case 3: rc = FN<3>(__VA_ARGS__); break;     \
    case 4: rc = FN<4>(__VA_ARGS__); break;     \
    case 5: rc = FN<5>(__VA_ARGS__); break;     \
    case 6: rc = FN<6>(__VA_ARGS__); break;     \
    case 7: rc = FN<7>(__VA_ARGS__); break;     \
    case 8: rc = FN<8>(__VA_ARGS__); break;     \
    case 9: rc = FN<9>(__VA_ARGS__); break;     \
    case 10: rc = FN<10>(__VA_ARGS__); break;   \
    case 11: rc = FN<11>(__VA_ARGS__); break;   \
    case 12: rc = FN<12>(__VA_ARGS__); break;   \
    case 13: rc = FN<13>(__VA_ARGS__); break;   \
    case 14: rc = FN<14>(__VA_ARGS__); break;   \
    case 15: rc = FN<15>(__VA_ARGS__); break;   \
    case 16: rc = FN<16>(__VA_ARGS__); break;   \
    case 17: rc = FN<17>(__VA_ARGS__); break;   \
    default: rc = fail(SEM_E_NOTIMPL, "hexahedral order out of range"); break; \
  }
static_assert(semh::HEX_MAX_N == 17, "HEX_DISPATCH lists n = 2..17");

// workgroups of the element kernel resident per CU (LDS and VGPR bound)
// (the matrix-core form: of the instantiation that will run, with or without
// the template map -- their register counts straddle an occupancy step)
template <int N>
int hex_wgs_per_cu(bool rows, bool mfma, bool tmap, int* out) {
  int nb = 0;
  const void* k = rows ? reinterpret_cast<const void*>(&semh::k_hex_rows<N, semh::HEX_SET>)
                       : reinterpret_cast<const void*>(&semh::k_hex_poisson<N, semh::HEX_SET>);
  if constexpr (N >= semh::HEX_MFMA_MIN_N)
    if (mfma)
      k = tmap ? reinterpret_cast<const void*>(&semh::k_hex_mfma<N, semh::HEX_SET, true>)
               : reinterpret_cast<const void*>(&semh::k_hex_mfma<N, semh::HEX_SET>);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, semh::hex_threads(N), 0) !=
      hipSuccess) {
    (void)hipGetLastError();
    nb = 0;
  }
  *out = nb;
  return SEM_OK;
}

int need_map(const sem_ctx* c) {
  if (!c->have_basis) return fail(SEM_E_STATE, "sem_set_basis must precede this call");
  if (!c->hex->d_map) return fail(SEM_E_STATE, "sem_set_map must precede this call");
  return SEM_OK;
}

}  // namespace

namespace semh {

// the row form by default where the three-block kernel's LDS
// (3 S n^3 doubles) exceeds 64 KiB: n >= 14
static bool hex_rows_default(int n) {
  const int64_t lds = 8 * (3 * (int64_t)hex_slots(n) * n * n * n + (int64_t)n * n);
  return lds > 65536;
}

int ctx_init(sem_ctx* c) {
  int rc = hex_check_order(c->n);
  if (rc) return rc;
  if (c->dpn != 1) return fail(SEM_E_NOTIMPL, "hexahedral operators: dofs_per_node == 1 only");
  c->hex = new HexState();
  c->hex->N = c->n;
  c->hex->slots = hex_slots(c->n);
  c->hex->threads = hex_threads(c->n);
  c->hex->nbc = hex_nbc(c->n);
  // the row form only on request (SEM_HEX_ROWS=1): with the z-merge in both
  // kernels the three-block kernel is as fast or faster at every order
  // measured (p = 2 / 4 / 6, DESIGN.md §4.9, profiles/r05/hex/zmerge_w1/)
  // and above p = 12, where the three-block kernel's 3 n^3 doubles of LDS
  // would leave one workgroup (of one element slot) per CU
  const char* re = std::getenv("SEM_HEX_ROWS");
  c->hex->rows = re ? std::atoi(re) != 0 : hex_rows_default(c->n);
  const char* ze = std::getenv("SEM_HEX_ZMERGE");
  c->hex->zmerge = !(ze && std::atoi(ze) == 0);
  // y-merge by default at n <= 4 (p <= 3), where it measured faster (p = 1 /
  // 2 / 3: 1.530 -> 1.429, 0.589 -> 0.544, 0.430 -> 0.415 ms per step at
  // ~1e7 DOF); at p = 4 / 7 its extra barrier per step outweighs the seams
  // it removes (0.324 -> 0.328, 0.266 -> 0.275; profiles/r06/hex_ymerge/).
  // SEM_HEX_YMERGE=1 / 0 forces it on / off.
  const char* ye = std::getenv("SEM_HEX_YMERGE");
  const bool ywant = ye ? std::atoi(ye) != 0 : c->n <= 4;
  c->hex->ymerge = ywant && c->hex->zmerge && !c->hex->rows && hex_grid_z(c->n) < hex_slots(c->n);
  return SEM_OK;
}

void ctx_free(sem_ctx* c) {
  if (!c->hex) return;
  c->hex->free_plan();
  (void)hipFree(c->hex->d_map);
  (void)hipFree(c->hex->d_G);
  (void)hipFree(c->hex->d_vx);
  delete c->hex;
  c->hex = nullptr;
}

int set_map(sem_ctx* c, const uint32_t* d_e2n, hipStream_t st) {
  HexState* H = c->hex;
  const int N = c->n;
  const int64_t N3 = (int64_t)N * N * N;
  const size_t count = (size_t)c->n_elem * N3;
  std::vector<uint32_t> h(count);
  HIP_TRY(hipMemcpyAsync(h.data(), d_e2n, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (!c->n_cu) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) ==
            hipSuccess &&
        ncu > 0)
      c->n_cu = ncu;
  }
  // the matrix-core form on request, where it is built (other orders stay
  // on the column forms: SEM_KERNEL=1 in the environment reaches every context)
  const bool mfma = c->kernel == SEM_KERNEL_MFMA && N >= HEX_MFMA_MIN_N && N <= HEX_MFMA_MAX_N;
  // template map (HexLaunch::ebase / tmpl; SEM_HEX_TMAP=0 turns it off)
  std::vector<int> tmpl;
  std::vector<uint32_t> eb;
  const char* te = std::getenv("SEM_HEX_TMAP");
  const bool tmap_ok =
      !(te && std::atoi(te) == 0) && semhexplan::hex_template_map(h, c->n_elem, N, tmpl, eb);
  int wpc = 0, rc = SEM_OK;
  HEX_DISPATCH(rc, N, hex_wgs_per_cu, H->rows, mfma, tmap_ok, &wpc);
  if (rc) return rc;
  semhexplan::HexPlanOptions opt = semhexplan::hex_plan_options_from_env();
  opt.zmerge = H->zmerge;
  opt.ymerge = H->ymerge;
  opt.resident = (int64_t)std::max(c->n_cu, 1) * std::max(wpc, 1);
  semhexplan::HexPlan P;
  rc = semhexplan::hex_plan_map(h, c->n_elem, c->n_node, N, opt, P);
  if (rc) return rc;
  c->epoch++;
  c->map_epoch++;
  H->free_plan();
  H->mfma = mfma;
  (void)hipFree(H->d_map);
  H->d_map = nullptr;
  HIP_TRY(hipMalloc(&H->d_map, count * sizeof(uint32_t)));
  HIP_TRY(hipMemcpy(H->d_map, h.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((rc = upload(&H->d_wg_off, P.wg_off)) || (rc = upload(&H->d_wg_len, P.wg_len)) ||
      (rc = upload(&H->d_elist, P.elist)) || (rc = upload(&H->d_cmask, P.cmask)) ||
      (rc = upload(&H->d_cflag, P.cflag)) || (rc = upload(&H->d_seam_gid, P.seam_gid)) ||
      (rc = upload(&H->d_seam_ptr, P.seam_ptr)) || (rc = upload(&H->d_seam_idx, P.seam_idx)) ||
      (rc = upload(&H->d_zero, P.zero)))
    return rc;
  // template map: one offset block shared by every element (structured
  // numberings); every kernel form and the diagonal
  if (tmap_ok) {
    if ((rc = upload(&H->d_ebase, eb)) || (rc = upload(&H->d_tmpl, tmpl))) return rc;
    H->tmap = true;
  }
  H->n_wg = (int64_t)P.wg_off.size();
  H->n_pos = (int64_t)P.elist.size();
  H->face_base = P.face_base;
  H->n_slot = P.n_slot;
  H->n_seam = (int64_t)P.seam_gid.size();
  H->n_seam_writes = (int64_t)P.seam_idx.size();
  H->n_zero = (int64_t)P.zero.size();
  H->n_chains = P.n_chains;
  H->n_subchains = P.n_sub;
  H->chain_len = P.lc;
  H->n_direct = P.n_direct;
  if (H->n_seam) HIP_TRY(hipMalloc(&H->d_slot, std::max<int64_t>(H->n_slot, 1) * sizeof(double)));
  // geometry belonged to the previous map
  (void)hipFree(H->d_G);
  H->d_G = nullptr;
  H->have_G = false;
  c->d_e2n = d_e2n;
  return SEM_OK;
}

static int ensure_G(sem_ctx* c) {
  HexState* H = c->hex;
  if (!H->d_G) {
    const size_t bytes = (size_t)c->n_elem * 6 * c->n * c->n * c->n * sizeof(double);
    HIP_TRY(hipMalloc(&H->d_G, bytes));
  }
  return SEM_OK;
}

int geom_from_nodes(sem_ctx* c, const double* d_nodes, int op_kind, int64_t* n_bad,
                    hipStream_t st) {
  if (op_kind != SEM_OP_POISSON)
    return fail(SEM_E_NOTIMPL, "hexahedral operators: Poisson only");
  int rc = need_map(c);
  if (rc) return rc;
  if ((rc = ensure_G(c))) return rc;
  c->epoch++;
  HIP_TRY(hipMemsetAsync(c->d_bad, 0, sizeof(unsigned long long), st));
  HEX_DISPATCH(rc, c->n, launch_hex_geom, c, d_nodes, c->hex->d_G, nullptr, nullptr, nullptr,
               nullptr, nullptr, st);
  if (rc) return rc;
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, c->d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_bad) *n_bad = (int64_t)bad;
  if (bad) {
    c->hex->have_G = false;
    return fail(SEM_E_DETJ, "detJ <= 0 at " + std::to_string(bad) + " quadrature nodes");
  }
  c->hex->have_G = true;
  return SEM_OK;
}

int geom_fields(sem_ctx* c, const double* d_nodes, double* x_phys, double* J, double* invJ,
                double* detJ, double* detJxW, hipStream_t st) {
  int rc = need_map(c);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->d_bad, 0, sizeof(unsigned long long), st));
  HEX_DISPATCH(rc, c->n, launch_hex_geom, c, d_nodes, nullptr, x_phys, J, invJ, detJ, detJxW,
               st);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return SEM_OK;
}

int set_geom(sem_ctx* c, const double* d_G, int op_kind, hipStream_t st) {
  if (op_kind != SEM_OP_POISSON)
    return fail(SEM_E_NOTIMPL, "hexahedral operators: Poisson only");
  int rc = need_map(c);
  if (rc) return rc;
  if ((rc = ensure_G(c))) return rc;
  c->epoch++;
  const int64_t total = c->n_elem * 6 * c->n * c->n * c->n;
  hipLaunchKernelGGL(k_hex_pack_geom, dim3(grid_for(total)), dim3(256), 0, st, d_G, c->n_elem,
                     c->n, c->hex->d_G);
  HIP_TRY(hipGetLastError());
  c->hex->have_G = true;
  return SEM_OK;
}

int apply(sem_ctx* c, int op_kind, const double* u, double* y, int flags, hipStream_t st) {
  if (op_kind != SEM_OP_POISSON)
    return fail(SEM_E_NOTIMPL, "hexahedral operators: Poisson only");
  if (flags & ~(SEM_APPLY_ACCUMULATE | SEM_APPLY_SKIP_ZERO))
    return fail(SEM_E_INVALID, "sem_apply flags not supported on hexahedra");
  int rc = need_map(c);
  if (rc) return rc;
  HexState* H = c->hex;
  if (!H->have_G) return fail(SEM_E_STATE, "geometry for this operator has not been computed");
  const bool acc = flags & SEM_APPLY_ACCUMULATE;
  if (!acc && !(flags & SEM_APPLY_SKIP_ZERO) && H->n_zero)
    if ((rc = zero_shared(c, y, st))) return rc;
  HEX_DISPATCH(rc, c->n, launch_hex_apply, c, acc ? HEX_ACC : HEX_SET, u, y, st);
  return rc;
}

int diag(sem_ctx* c, int op_kind, double* d, hipStream_t st) {
  if (op_kind != SEM_OP_POISSON) return fail(SEM_E_NOTIMPL, "sem_diag: Poisson only");
  int rc = need_map(c);
  if (rc) return rc;
  if (!c->hex->have_G) return fail(SEM_E_STATE, "geometry/map not set");
  if (c->hex->n_zero && (rc = zero_shared(c, d, st))) return rc;
  HEX_DISPATCH(rc, c->n, launch_hex_apply, c, HEX_DIAG, nullptr, d, st);
  return rc;
}

int zero_shared(sem_ctx* c, double* y, hipStream_t st) {
  HexState* H = c->hex;
  if (!H->d_map) return fail(SEM_E_STATE, "map must be set");
  if (H->n_zero) {
    hipLaunchKernelGGL(semh::k_hex_zero, dim3(grid_for(H->n_zero, 256, 4096)), dim3(256), 0, st, y,
                       H->d_zero, H->n_zero);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int plan_info(const sem_ctx* c, int64_t* info, int n_info) {
  const HexState* H = c->hex;
  // [0] workgroups, [1] zero list, [2] atomic groups (0), [3] conforming (1),
  // [4] element slots per workgroup, [5] chains (maximal), [6] sub-chain
  // length cap, [7] launch positions, [8] sub-chains, [9] seam nodes,
  // [10] slotted writes, [11] plain stores, [12] threads per workgroup,
  // [13] ndim (3), [14] geometry ready, [15] action kernel (2 matrix-core
  // form, 1 row form, 0 three-block), [16] z-merge in the plan, [17] y-merge: slots per grid
  // row (0: off), [18] template map
  const int64_t v[] = {H->n_wg,        H->n_zero, 0,
                       1,              H->slots,  H->n_chains,
                       H->chain_len,   H->n_pos,  H->n_subchains,
                       H->n_seam,      H->n_seam_writes, H->n_direct,
                       H->threads,     3,         H->have_G ? 1 : 0,
                       H->mfma ? 2 : H->rows ? 1 : 0, H->zmerge ? 1 : 0, H->ymerge ? hex_grid_z(H->N) : 0,
                       H->tmap ? 1 : 0};
  const int nv = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n_info; ++i) info[i] = i < nv ? v[i] : 0;
  return SEM_OK;
}

int zero_list(const sem_ctx* c, std::vector<uint32_t>* nodes, bool* only_unreferenced) {
  const HexState* H = c->hex;
  nodes->assign((size_t)H->n_zero, 0u);
  *only_unreferenced = true;
  if (H->n_zero)
    HIP_TRY(hipMemcpy(nodes->data(), H->d_zero, H->n_zero * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
  return SEM_OK;
}

int assemble(sem_ctx* c, const double* vals, double* out, int accumulate, hipStream_t st) {
  HexState* H = c->hex;
  if (!H->d_map) return fail(SEM_E_STATE, "sem_set_map must precede sem_assemble");
  if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, c->n_node * sizeof(double), st));
  const int64_t total = c->n_elem * c->n * c->n * c->n;
  hipLaunchKernelGGL(semh::k_hex_assemble, dim3(grid_for(total)), dim3(256), 0, st, H->d_map, vals,
                     total, out);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

}  // namespace semh
