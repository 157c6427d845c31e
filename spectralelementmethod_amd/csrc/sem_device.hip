// Device half of libsem_hip.so: the small kernels and the C ABI (the setup
// planner -- map packing, group colouring, write codes -- is sem_plan.cpp).  The operator
// kernels are instantiated per order in sem_launch.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sem_ctx.h"

using sem::fail;
using namespace semk;
using namespace semd;

namespace {

// user-supplied factors [E][ncomp][n][n] -> packed (element positions epos)
__global__ void k_pack_geom(const double* __restrict__ G, int64_t n_elem, int n, int ncomp,
                            int epw, const int* __restrict__ epos, double* __restrict__ GP) {
  const int64_t nn = (int64_t)n * n;
  const int64_t total = n_elem * ncomp * nn;
  const int lw = epw * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / (ncomp * nn);
    const int64_t rem = t - e * ncomp * nn;
    const int c = (int)(rem / nn);
    const int node = (int)(rem - c * nn);
    const int r = node / n, jj = node - r * n;
    const int64_t pos = epos[e];  // packed position slot * epw + lane element
    const int64_t gg = pos / epw;
    const int kk = (int)(pos - gg * epw);
    GP[((gg * ncomp + c) * n + r) * lw + kk * n + jj] = G[t];
  }
}

// u.y over all nodes (the fallback of sem_apply_dot on plans without seams)
__global__ void __launch_bounds__(BLOCK)
    k_dot_plain(const double* __restrict__ u, const double* __restrict__ y, int64_t n,
                double* __restrict__ part) {
  double v = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
    v = fma(u[i], y[i], v);
  __shared__ double sh[BLOCK / WAVE];
  const double t = semk::block_sum_fixed<BLOCK / WAVE>(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ void k_zero_list(double* __restrict__ y, const uint32_t* __restrict__ idx, int64_t n,
                            int dpn) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t base = (int64_t)idx[t] * dpn;
    for (int c = 0; c < dpn; ++c) y[base + c] = 0.0;
  }
}

// diag of the Poisson element operator, summed through the map:
// K_e[pq,pq] = sum_m D[m][p]^2 G00[m][q] + sum_n D[n][q]^2 G11[p][n] + 2 D[p][p] D[q][q] G01[p][q]
__global__ void k_poisson_diag(const uint32_t* __restrict__ mapP, const double* __restrict__ GP,
                               const int* __restrict__ epos, const double* __restrict__ gD, int n,
                               int epw, int64_t n_elem, double* __restrict__ diag) {
  __shared__ double sD[MAXN * MAXN];
  for (int i = threadIdx.x; i < n * n; i += blockDim.x) sD[i] = gD[i];
  __syncthreads();
  const int lw = epw * n;
  const int64_t total = n_elem * n * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / (n * n);
    const int node = (int)(t - e * n * n);
    const int p = node / n, q = node - p * n;
    const int64_t pos = epos[e];  // packed position slot * epw + lane element
    const int64_t gg = pos / epw;
    const int kk = (int)(pos - gg * epw);
    const double* G = GP + gg * (int64_t)(3 * n * lw) + kk * n;
    double s = 0.0;
    for (int m = 0; m < n; ++m) s += sD[m * n + p] * sD[m * n + p] * G[(0 * n + m) * lw + q];
    for (int nn = 0; nn < n; ++nn) s += sD[nn * n + q] * sD[nn * n + q] * G[(2 * n + p) * lw + nn];
    s += 2.0 * sD[p * n + p] * sD[q * n + q] * G[(1 * n + p) * lw + q];
    const uint32_t gi = mapP[(gg * n + p) * lw + kk * n + q] & GID_MASK;
    atomic_add_f64(diag + gi, s);
  }
}

// out[map[e][i][j]] += vals[e][i][j] through the caller's map (setup-time assembly)
__global__ void k_assemble(const uint32_t* __restrict__ e2n, const double* __restrict__ vals,
                           int64_t total, double* __restrict__ out) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x)
    atomic_add_f64(out + e2n[t], vals[t]);
}

__global__ void k_gather(const double* __restrict__ src, const uint32_t* __restrict__ idx,
                         int64_t n, double* __restrict__ dst) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    dst[t] = src[idx[t]];
}

__global__ void k_vec_add(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    dst[t] += src[t];
}

__global__ void k_scatter_add(double* __restrict__ dst, const uint32_t* __restrict__ idx,
                              int64_t n, const double* __restrict__ src) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    dst[idx[t]] += src[t];
}

// out[b][m][q] = sum_{r,s} A0[m][r] A1[q][s] in[b][r][s]  (A = NULL -> identity)
// TensorProduct.deriv / gradient (D(x)I, I(x)D; sem/basis_functions.py:626-650),
// compute_coeffs_grid_eq (Vinv(x)Vinv; :599-624), interpolate_on_grid_eq (:539-569).
__global__ void k_tensor_apply(int n, int64_t batch, const double* __restrict__ gA0,
                               const double* __restrict__ gA1, const double* __restrict__ in,
                               double* __restrict__ out) {
  __shared__ double sA0[MAXN * MAXN], sA1[MAXN * MAXN];
  __shared__ double tile[MAXN * MAXN];
  const int nn = n * n;
  for (int i = threadIdx.x; i < nn; i += blockDim.x) {
    const int r = i / n, c = i - r * n;
    sA0[i] = gA0 ? gA0[i] : (r == c ? 1.0 : 0.0);
    sA1[i] = gA1 ? gA1[i] : (r == c ? 1.0 : 0.0);
  }
  for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
    __syncthreads();
    for (int i = threadIdx.x; i < nn; i += blockDim.x) tile[i] = in[b * nn + i];
    __syncthreads();
    for (int i = threadIdx.x; i < nn; i += blockDim.x) {
      const int m = i / n, q = i - m * n;
      double a = 0.0;
      for (int r = 0; r < n; ++r) {
        double t = 0.0;
        for (int s = 0; s < n; ++s) t = fma(sA1[q * n + s], tile[r * n + s], t);
        a = fma(sA0[m * n + r], t, a);
      }
      out[b * nn + i] = a;
    }
  }
}

// det_inv_2x2 (sem/linalg.py:105-115) over n points: mat [2][2][n] -> det [n], inv [2][2][n]
__global__ void k_det_inv_2x2(int64_t n, const double* __restrict__ M, double* __restrict__ det,
                              double* __restrict__ inv) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const double a = M[t], b = M[n + t], c = M[2 * n + t], d = M[3 * n + t];
    const double dt = a * d - b * c;
    const double r = 1.0 / dt;
    det[t] = dt;
    inv[t] = d * r;
    inv[n + t] = -b * r;
    inv[2 * n + t] = -c * r;
    inv[3 * n + t] = a * r;
  }
}


}  // namespace
namespace sem {
int64_t ctx_ndof(const sem_ctx* c) { return c->n_node * c->dpn; }
int ctx_device(const sem_ctx* c) { return c->device; }
uint64_t ctx_epoch(const sem_ctx* c) { return c->epoch; }
int ctx_dpn(const sem_ctx* c) { return c->dpn; }
uint64_t ctx_map_epoch(const sem_ctx* c) { return c->map_epoch; }
bool ctx_seam_fusable(const sem_ctx* c) {
  // the n = 17 MFMA seam form sums its own seams (launch_apply_n ignores
  // defer_seam_sum there), so it is never fused with the finish
  return c->seam && !c->mfma && c->n_seam > 0 && c->dpn == 1 && c->seam_ns >= 1 &&
         c->seam_ns <= 8;
}
int ctx_seam_gids(const sem_ctx* c, std::vector<uint32_t>* gids) {
  gids->assign((size_t)c->n_seam, 0u);
  if (c->n_seam)
    HIP_TRY(hipMemcpy(gids->data(), c->d_seam_gid, c->n_seam * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
  return SEM_OK;
}
void ctx_set_defer_seam_sum(sem_ctx* c, bool defer) { c->defer_seam_sum = defer; }
bool ctx_seam_has_prior(const sem_ctx* c) {
  if (!c->n_seam) return false;
  std::vector<uint16_t> m((size_t)c->n_seam);
  if (hipMemcpy(m.data(), c->d_seam_mask, c->n_seam * sizeof(uint16_t), hipMemcpyDeviceToHost) !=
      hipSuccess) {
    (void)hipGetLastError();
    return true;  // unknown: treated as not fusable
  }
  for (uint16_t v : m)
    if (v & 0x100u) return true;
  return false;
}
int ctx_zero_list(const sem_ctx* c, std::vector<uint32_t>* nodes, bool* only_unreferenced) {
  if (c->ndim == 3) return semh::zero_list(c, nodes, only_unreferenced);
  nodes->assign((size_t)c->n_zero, 0u);
  *only_unreferenced = c->n_atomic_groups == 0;
  if (c->n_zero) {
    HIP_TRY(hipMemcpy(nodes->data(), c->d_zero, c->n_zero * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
  }
  return SEM_OK;
}
}  // namespace sem

namespace semd {
// second launch of the seam plan (k_seam_sum / k_seam_sum2 over the seam
// nodes, one instantiation per colour count)
int seam_ilp_of(const sem_ctx* c) { return c->n == 17 ? SEAM_ILP_17 : SEAM_ILP; }

int64_t seam_sum_blocks(const sem_ctx* c) {
  return c->n_seam ? grid_for(c->n_seam, BLOCK * seam_ilp_of(c)) : 0;
}

int launch_seam_sum(sem_ctx* c, double* y, int acc, hipStream_t st, const double* du,
                    double* dot) {
  if (!c->n_seam) return SEM_OK;
  const dim3 g(c->dpn == 2 ? grid_for(c->n_seam) : (int)seam_sum_blocks(c)), b(BLOCK);
  const bool ilp2 = seam_ilp_of(c) == 2;
  static_assert(SEAM_ILP == 1 || SEAM_ILP == 2, "seam-sum ILP 1 or 2");
  switch (c->seam_ns) {
#define SEAM_NS(K)                                                                           \
  case K:                                                                                  \
    if (c->dpn == 2)                                                                       \
      hipLaunchKernelGGL(k_seam_sum2<K>, g, b, 0, st, y, c->d_seam_gid, c->d_seam_mask,    \
                         c->n_seam, c->d_seam_buf, c->n_node, acc);                        \
    else if (dot && ilp2)                                                                  \
      hipLaunchKernelGGL((k_seam_sum<K, true, 2>), g, b, 0, st, y, c->d_seam_gid,          \
                         c->d_seam_mask, c->n_seam, c->d_seam_buf, c->n_node, acc, du, dot);\
    else if (dot)                                                                          \
      hipLaunchKernelGGL((k_seam_sum<K, true, 1>), g, b, 0, st, y, c->d_seam_gid,          \
                         c->d_seam_mask, c->n_seam, c->d_seam_buf, c->n_node, acc, du, dot);\
    else if (ilp2)                                                                         \
      hipLaunchKernelGGL((k_seam_sum<K, false, 2>), g, b, 0, st, y, c->d_seam_gid,         \
                         c->d_seam_mask, c->n_seam, c->d_seam_buf, c->n_node, acc, nullptr, \
                         nullptr);                                                         \
    else                                                                                   \
      hipLaunchKernelGGL((k_seam_sum<K, false, 1>), g, b, 0, st, y, c->d_seam_gid,         \
                         c->d_seam_mask, c->n_seam, c->d_seam_buf, c->n_node, acc, nullptr, \
                         nullptr);                                                         \
    break;
    SEAM_NS(1) SEAM_NS(2) SEAM_NS(3) SEAM_NS(4) SEAM_NS(5) SEAM_NS(6) SEAM_NS(7) SEAM_NS(8)
#undef SEAM_NS
    default:
      return sem::fail(SEM_E_STATE, "seam plan with more than 8 colours");
  }
  return SEM_OK;
}
}  // namespace semd

namespace {

int check_op(sem_ctx* c, int op_kind) {
  if (op_kind == SEM_OP_POISSON) {
    if (c->dpn != 1) return fail(SEM_E_INVALID, "Poisson operator needs dofs_per_node == 1");
    return SEM_OK;
  }
  if (op_kind == SEM_OP_AXISYM_STOKES || op_kind == SEM_OP_AXISYM_NS ||
      op_kind == SEM_OP_AXISYM_NS_JVP) {
    if (c->dpn != 2)
      return fail(SEM_E_INVALID, "axisymmetric Stokes block needs dofs_per_node == 2");
    return SEM_OK;
  }
  return fail(SEM_E_INVALID, "unknown op_kind " + std::to_string(op_kind));
}

// factor slot of an operator kind: the two Navier-Stokes kinds share one
int gp_slot(int op_kind) {
  return op_kind == SEM_OP_POISSON ? 0 : (op_kind == SEM_OP_AXISYM_STOKES ? 1 : 2);
}

// partial-sum buffer of sem_apply_dot (grown on demand, never shrunk)
int ensure_dot(sem_ctx* c, int64_t n) {
  if (c->d_dot && c->n_dot >= n) return SEM_OK;
  (void)hipFree(c->d_dot);
  c->d_dot = nullptr;
  HIP_TRY(hipMalloc(&c->d_dot, std::max<int64_t>(n, 1) * sizeof(double)));
  c->n_dot = std::max<int64_t>(n, 1);
  return SEM_OK;
}

// The zero fill is ordered on the stream of the kernels that fill the
// buffer: a plain hipMemset of device memory may still be in flight on the
// legacy default stream when a kernel on a non-blocking stream (the
// multi-GPU side stream) writes the factors.
int ensure_gp(sem_ctx* c, int op_kind, hipStream_t st) {
  const int slot = gp_slot(op_kind);
  if (!c->d_GP[slot]) {
    const int ncomp = sem_op_ncomp(op_kind);
    // + WAVE: the column kernels address the factors per lane, and the idle
    // lanes of a wavefront (lane >= lw, orders that do not divide 64) read up
    // to WAVE - lw entries past their slot's block -- past the array in the
    // last slot (values unused)
    const size_t bytes =
        ((size_t)c->n_slots * ncomp * c->n * c->lw + WAVE) * sizeof(double);
    HIP_TRY(hipMalloc(&c->d_GP[slot], bytes));
    HIP_TRY(hipMemsetAsync(c->d_GP[slot], 0, bytes, st));
  }
  return SEM_OK;
}


}  // namespace
extern "C" {

int sem_ctx_create(sem_ctx** out, int p, int64_t n_elem, int64_t n_node, int dpn, int device) {
  return sem_ctx_create_nd(out, 2, p, n_elem, n_node, dpn, device);
}

int sem_ctx_create_nd(sem_ctx** out, int ndim, int p, int64_t n_elem, int64_t n_node, int dpn,
                      int device) {
  if (!out) return fail(SEM_E_INVALID, "null ctx pointer");
  *out = nullptr;
  if (ndim != 2 && ndim != 3)
    return fail(SEM_E_NOTIMPL, "operators on quadrilaterals (ndim 2) and hexahedra (ndim 3) only");
  if (p < 1) return fail(SEM_E_INVALID, "Must specify an order of 1 or greater.");
  if (p > SEM_MAX_ORDER)
    return fail(SEM_E_NOTIMPL, "operator kernels built for orders 1.." +
                                   std::to_string(SEM_MAX_ORDER));
  if (n_elem < 1 || n_node < 1 || dpn < 1 || dpn > 2)
    return fail(SEM_E_INVALID, "bad sizes (n_elem, n_node >= 1, dpn in {1,2})");
  if (ndim == 2 && n_node > (int64_t)GID_MASK)
    return fail(SEM_E_INVALID, "n_node exceeds the per-GPU limit of 2^28 - 1 nodes");
  if (n_node > (int64_t)0xFFFFFFFFll)
    return fail(SEM_E_INVALID, "n_node exceeds the uint32 element map");
  DeviceGuard g(device);
  sem_ctx* c = new sem_ctx();
  c->p = p;
  c->n = p + 1;
  c->dpn = dpn;
  c->device = device;
  c->n_elem = n_elem;
  c->n_node = n_node;
  c->epw = epw_of(c->n);
  c->lw = c->epw * c->n;
  c->n_groups = (n_elem + c->epw - 1) / c->epw;
  if (const char* s = std::getenv("SEM_GEOM_MODE")) c->geom_mode = std::atoi(s);
  if (const char* s = std::getenv("SEM_KERNEL")) c->kernel = std::atoi(s);
  if (c->n_groups > 0x7FFFFFFFll) {
    delete c;
    return fail(SEM_E_INVALID, "too many elements");
  }
  hipError_t e1 = hipMalloc(&c->d_D, SEM_MAXN * SEM_MAXN * sizeof(double));
  hipError_t e2 = hipMalloc(&c->d_w, SEM_MAXN * sizeof(double));
  hipError_t e3 = hipMalloc(&c->d_Vinv, SEM_MAXN * SEM_MAXN * sizeof(double));
  hipError_t e4 = hipMalloc(&c->d_bad, sizeof(unsigned long long));
  if (!e4) e4 = hipMalloc(&c->d_deo, sizeof(DEOData<SEM_MAXN>));
  if (e1 || e2 || e3 || e4) {
    sem_ctx_destroy(c);
    return fail(SEM_E_HIP, "hipMalloc failed in sem_ctx_create");
  }
  if (ndim == 3) {
    c->ndim = 3;
    if (const int rc = semh::ctx_init(c)) {
      sem_ctx_destroy(c);
      return rc;
    }
  }
  *out = c;
  return SEM_OK;
}

void sem_ctx_destroy(sem_ctx* c) {
  if (!c) return;
  DeviceGuard g(c->device);
  semh::ctx_free(c);
  (void)hipFree(c->d_D);
  (void)hipFree(c->d_w);
  (void)hipFree(c->d_Vinv);
  (void)hipFree(c->d_deo);
  (void)hipFree(c->d_mapP);
  (void)hipFree(c->d_map16);
  (void)hipFree(c->d_mbase);
  (void)hipFree(c->d_epos);
  (void)hipFree(c->d_zero);
  for (double* g : c->d_GP) (void)hipFree(g);
  (void)hipFree(c->d_lin);
  (void)hipFree(c->d_XG);
  (void)hipFree(c->d_owner);
  (void)hipFree(c->d_bad);
  (void)hipFree(c->d_ccol);
  (void)hipFree(c->d_seam_gid);
  (void)hipFree(c->d_seam_mask);
  (void)hipFree(c->d_seam_buf);
  (void)hipFree(c->d_dot);
  delete c;
}

int sem_set_basis(sem_ctx* c, const double* hD, const double* hw) {
  if (!c || !hD || !hw) return fail(SEM_E_INVALID, "null argument");
  DeviceGuard g(c->device);
  const int n = c->n;
  // the kernels use D in even-odd form and half of w: a node set symmetric
  // about 0 (GLL), D[n-1-i][n-1-j] = -D[i][j] and w[n-1-i] = w[i]
  double dmax = 0.0, wmax = 0.0, dasym = 0.0, wasym = 0.0;
  for (int i = 0; i < n; ++i) {
    wmax = std::max(wmax, std::fabs(hw[i]));
    wasym = std::max(wasym, std::fabs(hw[i] - hw[n - 1 - i]));
    for (int j = 0; j < n; ++j) {
      dmax = std::max(dmax, std::fabs(hD[i * n + j]));
      dasym = std::max(dasym, std::fabs(hD[i * n + j] + hD[(n - 1 - i) * n + (n - 1 - j)]));
    }
  }
  if (!(dasym <= 1e-12 * dmax) || !(wasym <= 1e-14 * wmax))
    return fail(SEM_E_INVALID,
                "sem_set_basis: D and w must come from a node set symmetric about 0 (GLL)");
  c->epoch++;
  std::memcpy(c->hD, hD, sizeof(double) * n * n);
  std::memcpy(c->hw, hw, sizeof(double) * n);
  {
    const double* kd = sem_deo_const_d(n);
    // SEM_CONST_D: unset = the per-order choice (const_d_order), 0 = never,
    // 1 = wherever D matches
    const char* e = std::getenv("SEM_CONST_D");
    const bool want = e ? e[0] == '1' : const_d_order(n);
    c->const_d = want && kd && std::memcmp(kd, hD, sizeof(double) * n * n) == 0;
  }
  HIP_TRY(hipMemcpy(c->d_D, hD, sizeof(double) * n * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_w, hw, sizeof(double) * n, hipMemcpyHostToDevice));
  int rc = SEM_OK;
  SEM_DISPATCH_N(rc, n, upload_deo, c);
  if (rc) return rc;
  c->have_basis = true;
  return SEM_OK;
}

int sem_set_map(sem_ctx* c, const uint32_t* d_e2n, void* stream) {
  return sem_set_map_shared(c, d_e2n, nullptr, stream);
}

int sem_set_map_shared(sem_ctx* c, const uint32_t* d_e2n, const uint8_t* d_node_state,
                       void* stream) {
  if (!c || !d_e2n) return fail(SEM_E_INVALID, "null argument");
  DeviceGuard g(c->device);
  if (c->ndim == 3) {
    if (d_node_state)
      return fail(SEM_E_NOTIMPL, "sem_set_map_shared: node states on hexahedra are not supported");
    return semh::set_map(c, d_e2n, S(stream));
  }
  c->epoch++;
  c->map_epoch++;
  hipStream_t st = S(stream);
  const int n = c->n;
  std::vector<uint32_t> h((size_t)c->n_elem * n * n);
  std::vector<uint8_t> state;
  HIP_TRY(hipMemcpyAsync(h.data(), d_e2n, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (d_node_state) {
    state.resize(c->n_node);
    HIP_TRY(hipMemcpyAsync(state.data(), d_node_state, state.size(), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  const bool mfma = want_mfma(c);
  semplan::Plan P;
  if (const int rc = semplan::plan_map(h, c->n_elem, c->n_node, n, c->dpn, mfma, state,
                                       semplan::plan_options_from_env(), P))
    return rc;
  std::vector<uint32_t>().swap(h);
  c->d_e2n = d_e2n;
  int rc;
  if ((rc = upload(&c->d_mapP, P.mapP)) || (rc = upload(&c->d_map16, P.m16)) ||
      (rc = upload(&c->d_mbase, P.mbase)) || (rc = upload(&c->d_epos, P.epos)) ||
      (rc = upload(&c->d_zero, P.zero)) || (rc = upload(&c->d_owner, P.owner)) ||
      (rc = upload(&c->d_ccol, P.chain_colour)) || (rc = upload(&c->d_seam_gid, P.seam_gid)) ||
      (rc = upload(&c->d_seam_mask, P.seam_mask)))
    return rc;
  c->mfma = mfma;
  c->ecol = P.ecol;
  c->epw = mfma ? 1 : epw_of(n);
  c->lw = c->epw * n;
  c->n_groups = (c->n_elem + c->epw - 1) / c->epw;
  c->rounds = P.rounds;
  c->blocks = P.blocks;
  c->row_carries = P.row_carries;
  c->round_sync = P.round_sync;
  c->n_slots = P.n_slots;
  c->map16 = P.map16;
  c->map_pat = P.map_pat;
  c->n_map_pat = P.n_map_pat;
  c->n_zero = (int64_t)P.zero.size();
  c->colour_start = P.colour_start;
  c->seam = P.seam;
  // sem_apply_dot's fused form: every node's final value is one STORE (or a
  // seam sum): no read-modify-write, nothing zeroed separately
  c->seam_dot = !mfma && P.seam && P.n_rmw == 0 && P.zero.empty() && state.empty();
  c->seam_ns = P.seam_ns;
  c->n_seam = (int64_t)P.seam_gid.size();
  c->n_atomic_groups = P.n_atomic_groups;
  c->conforming = P.conforming;
  (void)hipFree(c->d_seam_buf);
  c->d_seam_buf = nullptr;
  if (c->n_seam)  // slots addressed by node id (only seam nodes' slots are touched)
    HIP_TRY(hipMalloc(&c->d_seam_buf, (size_t)c->n_node * c->seam_ns * c->dpn * sizeof(double)));
  // geometry was derived for the previous map
  for (double*& g : c->d_GP) {
    (void)hipFree(g);
    g = nullptr;
  }
  (void)hipFree(c->d_lin);
  c->d_lin = nullptr;
  c->lin_valid = false;
  c->xg_valid = false;
  c->xg_axi = false;
  return SEM_OK;
}

int sem_plan_info(sem_ctx* c, int64_t* info, int n_info) {
  if (!c || !info || n_info < 1) return fail(SEM_E_INVALID, "bad arguments");
  if (c->ndim == 3) return semh::plan_info(c, info, n_info);
  const int64_t nc = c->colour_start.empty() ? 0 : (int64_t)c->colour_start.size() - 1;
  constexpr int NV = 8 + MAX_COLOURS + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1 + 1;
  int64_t vals[NV] = {c->n_groups, c->n_zero, c->n_atomic_groups, c->conforming ? 1 : 0,
                      c->epw,      nc,        c->rounds,          c->n_slots};
  for (int64_t q = 0; q < nc && q <= MAX_COLOURS; ++q)
    vals[8 + q] = c->colour_start[q + 1] - c->colour_start[q];
  vals[NV - 10] = c->mfma ? SEM_KERNEL_MFMA : SEM_KERNEL_COLUMN;
  vals[NV - 9] = c->map16 ? 2 : 4;  // bytes per packed map entry
  // the geometry the Poisson action actually uses: nodal only once x_phys
  // per node exists (sem_set_geom installs stored factors); before any
  // geometry, the mode sem_geom_from_nodes will resolve to
  const bool eff_nodal = c->xg_valid ? true : (c->d_GP[0] ? false : nodal_mode(c));
  vals[NV - 8] = eff_nodal ? SEM_GEOM_NODAL : SEM_GEOM_STORED;
  // plan: 0 chains (colour launches), 1 element-coloured chains, 2 elements
  // (MFMA kernel), 4 chains + seam sums (3 was the retired one-launch plan),
  // 5 elements + seam sums (n = 17 MFMA kernel)
  vals[NV - 7] = c->mfma ? (c->seam ? 5 : 2) : (c->ecol ? 1 : (c->seam ? 4 : 0));
  // the same for the axisymmetric Stokes block (dofs_per_node = 2)
  const bool axi_nodal =
      c->xg_axi ? true : (c->d_GP[1] ? false : nodal_mode_op(c, SEM_OP_AXISYM_STOKES));
  vals[NV - 6] = c->dpn == 2 ? (axi_nodal ? SEM_GEOM_NODAL : SEM_GEOM_STORED) : 0;
  vals[NV - 5] = c->seam ? c->n_seam : 0;  // seam nodes
  vals[NV - 4] = c->blocks ? 1 : 0;          // block layout
  vals[NV - 3] = c->row_carries;             // entries carried between rounds
  vals[NV - 2] = c->const_d && c->map16 && !c->mfma ? 1 : 0;  // Poisson: D as constants
  vals[NV - 1] = c->map_pat ? c->n_map_pat : 0;  // map pattern table: patterns (0: off)
  for (int i = 0; i < n_info && i < NV; ++i) info[i] = vals[i];
  return SEM_OK;
}

static int geom_common(sem_ctx* c, const double* d_nodes, const double* h_Vinv) {
  if (!c || !d_nodes || !h_Vinv) return fail(SEM_E_INVALID, "null argument");
  if (!c->have_basis) return fail(SEM_E_STATE, "sem_set_basis must precede geometry");
  if (!c->d_e2n) return fail(SEM_E_STATE, "sem_set_map must precede geometry");
  HIP_TRY(hipMemcpy(c->d_Vinv, h_Vinv, sizeof(double) * c->n * c->n, hipMemcpyHostToDevice));
  return SEM_OK;
}

int sem_set_geom_mode(sem_ctx* c, int mode) {
  if (!c) return fail(SEM_E_INVALID, "null ctx");
  if (mode != SEM_GEOM_STORED && mode != SEM_GEOM_NODAL && mode != SEM_GEOM_AUTO)
    return fail(SEM_E_INVALID, "unknown geometry mode " + std::to_string(mode));
  if (c->ndim == 3 && mode == SEM_GEOM_NODAL)
    return fail(SEM_E_NOTIMPL, "hexahedra: stored geometric factors only");
  c->geom_mode = mode;
  c->epoch++;
  return SEM_OK;
}

int sem_set_reynolds(sem_ctx* c, double re) {
  if (!c) return fail(SEM_E_INVALID, "null ctx");
  if (!std::isfinite(re)) return fail(SEM_E_INVALID, "Reynolds number must be finite");
  c->reynolds = re;
  c->epoch++;
  c->lin_valid = false;  // a recorded linearisation belongs to the old Re
  return SEM_OK;
}

int sem_set_kernel(sem_ctx* c, int kernel) {
  if (!c) return fail(SEM_E_INVALID, "null ctx");
  if (kernel != SEM_KERNEL_COLUMN && kernel != SEM_KERNEL_MFMA && kernel != SEM_KERNEL_AUTO)
    return fail(SEM_E_INVALID, "unknown kernel " + std::to_string(kernel));
  if (kernel == SEM_KERNEL_MFMA && c->ndim == 3 && (c->n < 12 || c->n > 17))
    return fail(SEM_E_NOTIMPL, "hexahedra: the MFMA kernel is built for p = 11..16");
  if (kernel == SEM_KERNEL_MFMA && (c->dpn != 1 || c->n > 17))
    return fail(SEM_E_NOTIMPL, "the MFMA kernel needs dofs_per_node == 1 and p <= 16");
  c->kernel = kernel;
  c->epoch++;
  return SEM_OK;
}

int sem_geom_from_nodes(sem_ctx* c, const double* d_nodes, const double* h_Vinv, int op_kind,
                        int64_t* n_bad_nodes, void* stream) {
  if (!c) return fail(SEM_E_INVALID, "null ctx");
  DeviceGuard g(c->device);
  int rc = geom_common(c, d_nodes, h_Vinv);
  if (rc) return rc;
  if ((rc = check_op(c, op_kind))) return rc;
  if (c->ndim == 3) return semh::geom_from_nodes(c, d_nodes, op_kind, n_bad_nodes, S(stream));
  const bool nodal = nodal_mode_op(c, op_kind);
  c->epoch++;
  double* GP = nullptr;
  if (nodal) {
    if (!c->d_XG) HIP_TRY(hipMalloc(&c->d_XG, c->n_node * sizeof(double2)));
    // stale stored factors would otherwise survive for sem_diag
    (void)hipFree(c->d_GP[gp_slot(op_kind)]);
    c->d_GP[gp_slot(op_kind)] = nullptr;
  } else {
    if ((rc = ensure_gp(c, op_kind, S(stream)))) return rc;
    GP = c->d_GP[gp_slot(op_kind)];
  }
  hipStream_t st = S(stream);
  HIP_TRY(hipMemsetAsync(c->d_bad, 0, sizeof(unsigned long long), st));
  if (nodal) HIP_TRY(hipMemsetAsync(c->d_XG, 0, c->n_node * sizeof(double2), st));
  SEM_DISPATCH_N(rc, c->n, launch_geom_n, c, d_nodes, op_kind, GP, nullptr, nullptr, nullptr,
                 nullptr, nullptr, nodal ? c->d_XG : nullptr, nullptr, st);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, c->d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_bad_nodes) *n_bad_nodes = (int64_t)bad;
  if (bad) return fail(SEM_E_DETJ, "detJ <= 0 at " + std::to_string(bad) + " quadrature nodes");
  // x_phys per node is one array for the mesh: recomputed here, from these
  // nodes, for every operator that reads it
  if (op_kind == SEM_OP_POISSON) c->xg_valid = nodal;
  if (op_kind == SEM_OP_AXISYM_STOKES) c->xg_axi = nodal;
  if (gp_slot(op_kind) == 2) c->lin_valid = false;  // linearisation used the old factors
  return SEM_OK;
}

int sem_geom_from_xphys(sem_ctx* c, const double* d_xphys, int op_kind, int64_t* n_bad_nodes,
                        void* stream) {
  if (!c || !d_xphys) return fail(SEM_E_INVALID, "null argument");
  if (c->ndim == 3) return fail(SEM_E_NOTIMPL, "sem_geom_from_xphys: quadrilaterals only");
  if (!c->have_basis) return fail(SEM_E_STATE, "sem_set_basis must precede geometry");
  if (!c->d_e2n) return fail(SEM_E_STATE, "sem_set_map must precede geometry");
  DeviceGuard g(c->device);
  int rc;
  if ((rc = check_op(c, op_kind))) return rc;
  hipStream_t st = S(stream);
  c->epoch++;
  if ((rc = ensure_gp(c, op_kind, st))) return rc;
  HIP_TRY(hipMemsetAsync(c->d_bad, 0, sizeof(unsigned long long), st));
  SEM_DISPATCH_N(rc, c->n, launch_geom_n, c, nullptr, op_kind, c->d_GP[gp_slot(op_kind)], nullptr,
                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st, d_xphys);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, c->d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_bad_nodes) *n_bad_nodes = (int64_t)bad;
  if (bad) return fail(SEM_E_DETJ, "detJ <= 0 at " + std::to_string(bad) + " quadrature nodes");
  // the stored factors take over from any x_phys per node
  if (op_kind == SEM_OP_POISSON) c->xg_valid = false;
  if (op_kind == SEM_OP_AXISYM_STOKES) c->xg_axi = false;
  if (gp_slot(op_kind) == 2) c->lin_valid = false;
  return SEM_OK;
}

int sem_geom_fields(sem_ctx* c, const double* d_nodes, const double* h_Vinv, double* x_phys,
                    double* J, double* invJ, double* detJ, double* detJxW, void* stream) {
  if (!c) return fail(SEM_E_INVALID, "null ctx");
  DeviceGuard g(c->device);
  int rc = geom_common(c, d_nodes, h_Vinv);
  if (rc) return rc;
  hipStream_t st = S(stream);
  if (c->ndim == 3) return semh::geom_fields(c, d_nodes, x_phys, J, invJ, detJ, detJxW, st);
  HIP_TRY(hipMemsetAsync(c->d_bad, 0, sizeof(unsigned long long), st));
  SEM_DISPATCH_N(rc, c->n, launch_geom_n, c, d_nodes, SEM_OP_POISSON, nullptr, x_phys, J, invJ,
                 detJ, detJxW, nullptr, nullptr, st);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return SEM_OK;
}

int sem_set_geom(sem_ctx* c, const double* d_G, int op_kind, void* stream) {
  if (!c || !d_G) return fail(SEM_E_INVALID, "null argument");
  if (c->ndim == 3) {
    DeviceGuard g(c->device);
    return semh::set_geom(c, d_G, op_kind, S(stream));
  }
  if (!c->d_epos) return fail(SEM_E_STATE, "sem_set_map must precede sem_set_geom");
  DeviceGuard g(c->device);
  int rc;
  if ((rc = check_op(c, op_kind))) return rc;
  if ((rc = ensure_gp(c, op_kind, S(stream)))) return rc;
  const int ncomp = sem_op_ncomp(op_kind);
  c->epoch++;
  if (op_kind == SEM_OP_POISSON) c->xg_valid = false;  // caller's factors take over
  if (op_kind == SEM_OP_AXISYM_STOKES) c->xg_axi = false;
  hipLaunchKernelGGL(k_pack_geom, dim3(grid_for(c->n_elem * ncomp * c->n * c->n)), dim3(BLOCK), 0,
                     S(stream), d_G, c->n_elem, c->n, ncomp, c->epw, c->d_epos,
                     c->d_GP[gp_slot(op_kind)]);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_zero_shared(sem_ctx* c, double* y, void* stream) {
  if (!c || !y) return fail(SEM_E_INVALID, "null argument");
  if (c->ndim == 3) {
    DeviceGuard g(c->device);
    return semh::zero_shared(c, y, S(stream));
  }
  if (!c->d_mapP) return fail(SEM_E_STATE, "map must be set");
  DeviceGuard g(c->device);
  if (c->n_zero)
    hipLaunchKernelGGL(k_zero_list, dim3(grid_for(c->n_zero, BLOCK, 4096)), dim3(BLOCK), 0,
                       S(stream), y, c->d_zero, c->n_zero, c->dpn);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_apply(sem_ctx* c, int op_kind, const double* u, double* y, int flags, void* stream) {
  if (!c || !u || !y) return fail(SEM_E_INVALID, "null argument");
  {  // the kernels read u while other workgroups write y (both __restrict__)
    const size_t nb = (size_t)c->n_node * c->dpn * sizeof(double);
    const char *a = reinterpret_cast<const char*>(u), *b = reinterpret_cast<const char*>(y);
    if (a < b + nb && b < a + nb) return fail(SEM_E_INVALID, "sem_apply: u and y overlap");
  }
  if (flags & ~(SEM_APPLY_ACCUMULATE | SEM_APPLY_SKIP_ZERO | SEM_APPLY_LINEARIZE))
    return fail(SEM_E_INVALID, "unknown sem_apply flags");
  int rc;
  if ((rc = check_op(c, op_kind))) return rc;
  if (c->ndim == 3) {
    DeviceGuard g(c->device);
    return semh::apply(c, op_kind, u, y, flags, S(stream));
  }
  if (!c->have_basis || !c->d_mapP) return fail(SEM_E_STATE, "basis and map must be set");
  if (!use_nodal(c, op_kind) && !c->d_GP[gp_slot(op_kind)])
    return fail(SEM_E_STATE, "geometry for this operator has not been computed");
  const bool lin = flags & SEM_APPLY_LINEARIZE;
  if (lin && op_kind != SEM_OP_AXISYM_NS)
    return fail(SEM_E_INVALID, "SEM_APPLY_LINEARIZE applies to SEM_OP_AXISYM_NS only");
  if (op_kind == SEM_OP_AXISYM_NS_JVP && !c->lin_valid)
    return fail(SEM_E_STATE, "no linearisation: apply SEM_OP_AXISYM_NS with SEM_APPLY_LINEARIZE first");
  if (lin && !c->d_lin) {
    // + WAVE: idle lanes of the last slot, as in ensure_gp
    HIP_TRY(hipMalloc(&c->d_lin,
                      ((size_t)c->n_slots * 5 * c->n * c->lw + WAVE) * sizeof(double)));
    c->epoch++;
  }
  DeviceGuard g(c->device);
  hipStream_t st = S(stream);
  const int accumulate = flags & SEM_APPLY_ACCUMULATE;
  if (!accumulate && !(flags & SEM_APPLY_SKIP_ZERO) && c->n_zero)
    hipLaunchKernelGGL(k_zero_list, dim3(grid_for(c->n_zero, BLOCK, 4096)), dim3(BLOCK), 0, st, y,
                       c->d_zero, c->n_zero, c->dpn);
  SEM_DISPATCH_N(rc, c->n, launch_apply_n, c, op_kind, u, y, accumulate, lin, st, nullptr);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  if (lin) c->lin_valid = true;
  return SEM_OK;
}

int sem_apply_dot(sem_ctx* c, int op_kind, const double* u, double* y, double* d_dot,
                  void* stream) {
  if (!c || !d_dot) return fail(SEM_E_INVALID, "null argument");
  if (!(c->seam_dot && op_kind == SEM_OP_POISSON && c->dpn == 1)) {
    // no fused form on this plan: the action, then a separate u.y pass
    int rc = sem_apply(c, op_kind, u, y, 0, stream);
    if (rc) return rc;
    DeviceGuard g(c->device);
    hipStream_t st = S(stream);
    const int64_t n = c->n_node * c->dpn;
    const int nb = grid_for(n, BLOCK, 2048);
    if ((rc = ensure_dot(c, nb))) return rc;
    hipLaunchKernelGGL(k_dot_plain, dim3(nb), dim3(BLOCK), 0, st, u, y, n, c->d_dot);
    hipLaunchKernelGGL(k_dot_finish, dim3(1), dim3(DOT_FIN_THREADS), 0, st, c->d_dot, (int64_t)nb,
                       c->d_dot, (int64_t)0, d_dot);
    HIP_TRY(hipGetLastError());
    return SEM_OK;
  }
  int rc;
  if ((rc = check_op(c, op_kind))) return rc;
  if (!c->have_basis || !c->d_mapP) return fail(SEM_E_STATE, "basis and map must be set");
  if (!use_nodal(c, op_kind) && !c->d_GP[gp_slot(op_kind)])
    return fail(SEM_E_STATE, "geometry for this operator has not been computed");
  {
    const size_t nb = (size_t)c->n_node * sizeof(double);
    const char *a = reinterpret_cast<const char*>(u), *b = reinterpret_cast<const char*>(y);
    if (a < b + nb && b < a + nb) return fail(SEM_E_INVALID, "sem_apply_dot: u and y overlap");
  }
  DeviceGuard g(c->device);
  const int64_t nch = c->colour_start.back() - c->colour_start.front();
  if ((rc = ensure_dot(c, nch + seam_sum_blocks(c)))) return rc;
  SEM_DISPATCH_N(rc, c->n, launch_apply_n, c, op_kind, u, y, 0, false, S(stream), d_dot);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_vec_add(double* dst, const double* src, int64_t n, void* stream) {
  if (n < 0 || (n && (!dst || !src))) return fail(SEM_E_INVALID, "bad arguments");
  if (!n) return SEM_OK;
  hipLaunchKernelGGL(k_vec_add, dim3(grid_for(n)), dim3(BLOCK), 0, S(stream), dst, src, n);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_diag(sem_ctx* c, int op_kind, double* d_diag, void* stream) {
  if (!c || !d_diag) return fail(SEM_E_INVALID, "null argument");
  if (op_kind != SEM_OP_POISSON) return fail(SEM_E_NOTIMPL, "sem_diag: Poisson only");
  int rc;
  if ((rc = check_op(c, op_kind))) return rc;
  if (c->ndim == 3) {
    DeviceGuard g(c->device);
    return semh::diag(c, op_kind, d_diag, S(stream));
  }
  if (!c->d_mapP || !(c->d_GP[0] || use_nodal(c, op_kind)))
    return fail(SEM_E_STATE, "geometry/map not set");
  DeviceGuard g(c->device);
  hipStream_t st = S(stream);
  if (!c->d_GP[0]) {  // NODAL mode: derive the stored factors once from x_phys per node
    if ((rc = ensure_gp(c, op_kind, st))) return rc;
    SEM_DISPATCH_N(rc, c->n, launch_geom_n, c, nullptr, SEM_OP_POISSON, c->d_GP[0], nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr, c->d_XG, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemsetAsync(d_diag, 0, c->n_node * sizeof(double), st));
  hipLaunchKernelGGL(k_poisson_diag, dim3(grid_for(c->n_elem * c->n * c->n)), dim3(BLOCK), 0, st,
                     c->d_mapP, c->d_GP[0], c->d_epos, c->d_D, c->n, c->epw, c->n_elem, d_diag);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_assemble(sem_ctx* c, const double* vals, double* out, int accumulate, void* stream) {
  if (!c || !vals || !out) return fail(SEM_E_INVALID, "null argument");
  if (c->ndim == 3) {
    DeviceGuard g(c->device);
    return semh::assemble(c, vals, out, accumulate, S(stream));
  }
  if (!c->d_e2n) return fail(SEM_E_STATE, "sem_set_map must precede sem_assemble");
  if (c->dpn != 1) return fail(SEM_E_INVALID, "sem_assemble: dofs_per_node == 1 only");
  DeviceGuard g(c->device);
  hipStream_t st = S(stream);
  if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, c->n_node * sizeof(double), st));
  const int64_t total = c->n_elem * c->n * c->n;
  hipLaunchKernelGGL(k_assemble, dim3(grid_for(total)), dim3(BLOCK), 0, st, c->d_e2n, vals, total,
                     out);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_gather(const double* src, const uint32_t* idx, int64_t n, double* dst, void* stream) {
  if (n < 0 || (n && (!src || !idx || !dst))) return fail(SEM_E_INVALID, "bad arguments");
  if (!n) return SEM_OK;
  hipLaunchKernelGGL(k_gather, dim3(grid_for(n)), dim3(BLOCK), 0, S(stream), src, idx, n, dst);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_scatter_add(double* dst, const uint32_t* idx, int64_t n, const double* src, void* stream) {
  if (n < 0 || (n && (!src || !idx || !dst))) return fail(SEM_E_INVALID, "bad arguments");
  if (!n) return SEM_OK;
  hipLaunchKernelGGL(k_scatter_add, dim3(grid_for(n)), dim3(BLOCK), 0, S(stream), dst, idx, n, src);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_tensor_apply(int n, int64_t batch, const double* h_A0, const double* h_A1,
                     const double* d_in, double* d_out, void* stream) {
  if (n < 1 || n > SEM_MAXN || batch < 0 || (batch && (!d_in || !d_out)))
    return fail(SEM_E_INVALID, "sem_tensor_apply: bad arguments");
  if (!batch) return SEM_OK;
  hipStream_t st = S(stream);
  double* dA = nullptr;
  HIP_TRY(hipMallocAsync((void**)&dA, 2 * n * n * sizeof(double), st));
  if (h_A0) HIP_TRY(hipMemcpyAsync(dA, h_A0, n * n * sizeof(double), hipMemcpyHostToDevice, st));
  if (h_A1)
    HIP_TRY(hipMemcpyAsync(dA + n * n, h_A1, n * n * sizeof(double), hipMemcpyHostToDevice, st));
  const int grid = (int)std::min<int64_t>(batch, 4096);
  hipLaunchKernelGGL(k_tensor_apply, dim3(grid), dim3(BLOCK), 0, st, n, batch,
                     h_A0 ? dA : nullptr, h_A1 ? dA + n * n : nullptr, d_in, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipFreeAsync(dA, st));
  return SEM_OK;
}

int sem_det_inv_2x2(int64_t n, const double* d_mat, double* d_det, double* d_inv, void* stream) {
  if (n < 0 || (n && (!d_mat || !d_det || !d_inv))) return fail(SEM_E_INVALID, "bad arguments");
  if (!n) return SEM_OK;
  hipLaunchKernelGGL(k_det_inv_2x2, dim3(grid_for(n)), dim3(BLOCK), 0, S(stream), n, d_mat, d_det,
                     d_inv);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

}  // extern "C"

namespace sem {
int ctx_seam_pack(sem_ctx* c, double* y, double* send, const uint32_t* sidx, const int32_t* sj,
                  int64_t ne, hipStream_t st) {
  const int64_t tot = c->n_seam + ne;
  if (!tot) return SEM_OK;
  const dim3 g(semd::grid_for(tot)), b(BLOCK);
  switch (c->seam_ns) {
#define SEAM_PACK(K)                                                                        \
  case K:                                                                                 \
    hipLaunchKernelGGL(k_seam_pack<K>, g, b, 0, st, y, c->d_seam_gid, c->d_seam_mask,      \
                       c->n_seam, c->d_seam_buf, c->n_node, send, sidx, sj, ne);          \
    break;
    SEAM_PACK(1) SEAM_PACK(2) SEAM_PACK(3) SEAM_PACK(4) SEAM_PACK(5) SEAM_PACK(6) SEAM_PACK(7)
    SEAM_PACK(8)
#undef SEAM_PACK
    default:
      return fail(SEM_E_STATE, "seam plan with more than 8 colours");
  }
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int ctx_seam_finish(sem_ctx* c, double* y, const DDFinish& f, hipStream_t st) {
  const int64_t tot = (f.sel ? f.n_sel : c->n_seam) + (f.skip_rest ? 0 : f.n_rest) +
                      (f.skip_zero ? 0 : f.nz);
  if (!tot) return SEM_OK;
  const dim3 g(semd::grid_for(tot)), b(BLOCK);
  switch (c->seam_ns) {
#define SEAM_FIN(K)                                                                         \
  case K:                                                                                 \
    hipLaunchKernelGGL(k_seam_dd_finish<K>, g, b, 0, st, y, c->d_seam_gid, c->d_seam_mask, \
                       c->n_seam, c->d_seam_buf, c->n_node, f);                           \
    break;
    SEAM_FIN(1) SEAM_FIN(2) SEAM_FIN(3) SEAM_FIN(4) SEAM_FIN(5) SEAM_FIN(6) SEAM_FIN(7)
    SEAM_FIN(8)
#undef SEAM_FIN
    default:
      return fail(SEM_E_STATE, "seam plan with more than 8 colours");
  }
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}
}  // namespace sem
