// p-multigrid preconditioner of the assembled Poisson solve and the PCG that
// runs with it (include/sem_hip.h "p-multigrid").
//
// Levels p_0 > p_1 > ... > p_L live on the same elements; level l is an
// operator context (borrowed), its Dirichlet mask and 1 / diag (0 on fixed
// DOFs), and transfer l carries level l + 1 to level l (sem_transfer.hip).
// One V-cycle z = M r is a single chain of launches on the caller's stream:
//
//   level l < L:  x = Chebyshev_k(b) from zero          k passes, k - 1 actions
//                 r = (b - A x) * free                   1 action, 1 pass
//                 b_{l+1} = restrict(r)
//                 ... level l + 1 ...
//                 x += prolong(x_{l+1}) on free DOFs     1 pass
//                 x = Chebyshev_k(b) from x              k passes, k actions
//   level L:      x = Chebyshev_kc(b) from zero          kc passes, kc - 1 actions
//
// The Chebyshev iteration for D^-1 A on [lambda_max / ratio, lambda_max] is
// d_0 = D^-1 r / theta, then per step x += d, r -= A d, d = c1 d + c2 D^-1 r
// (csrc/sem_mg_plan.cpp chebyshev).  Each step after the action q = A d is
// one pass over q, r, d, x and D^-1 that writes r, d and x (k_mg_step); x
// takes the new d in the same pass, so no trailing x += d remains and the
// last step leaves r unwritten.  The post-smoother's residual and first step
// are one pass as well (k_mg_first<ADD>).  No inner dot product or Krylov
// solve: M is a fixed symmetric positive definite matrix, plain PCG is valid.
//
// The vector passes follow the measured conventions of the Jacobi PCG
// (sem_dd.hip): at most 512 workgroups of 256 threads in a
// grid-stride walk, 16-byte nontemporal accesses, every load of a round
// issued before the first use, level vectors padded to 32 doubles, dot
// products as fixed-order two-stage sums (bitwise repeatable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sem_internal.h"
#include "sem_mg_plan.h"

using sem::fail;

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

#define SEM_TRY(expr)    \
  do {                   \
    int _rc = (expr);    \
    if (_rc) return _rc; \
  } while (0)

namespace {

constexpr int BLK = 256;
constexpr int WV = 64;
constexpr int RED_BLOCKS = 512;  // workgroups of a pass = partial sums per dot (fixed order)
constexpr int UNR = 4;           // doubles per thread and round

struct Level {
  sem_ctx* ctx = nullptr;        // borrowed
  sem_transfer* down = nullptr;  // borrowed: level l + 1 ("from") -> level l ("to")
  int64_t n = 0, nn = 0;         // DOFs, padded to 32
  double* base = nullptr;        // dinv, b, x, r, d, q, e: 7 rows of nn
  double *dinv = nullptr, *b = nullptr, *x = nullptr, *r = nullptr, *d = nullptr, *q = nullptr,
         *e = nullptr;
  semmg::Cheb cheb;
  int degree = 0;
  int actions = 0, passes = 0;          // planned per cycle
  int run_actions = 0, run_passes = 0;  // enqueued by the last cycle
};

}  // namespace

struct sem_mg {
  int device = 0, n_levels = 0, smooth_degree = 0, coarse_degree = 0;
  std::vector<Level> lv;
  double* p = nullptr;    // PCG search direction [nn of level 0]
  double* red = nullptr;  // partials [2][RED_BLOCKS], then scalars rz[2], pq, (unused, rr)
  size_t vector_bytes = 0;
};

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int grid_for(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + BLK - 1) / BLK, RED_BLOCKS));
}

struct Guard {
  int prev = -1;
  explicit Guard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~Guard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// ------------------------------------------------------------------ kernels
template <int V>
__device__ __forceinline__ void ldv(const double* __restrict__ a, int64_t i, double (&o)[V]) {
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = __builtin_nontemporal_load(a + i * V + e);
}
template <int V>
__device__ __forceinline__ void stv(double* __restrict__ a, int64_t i, const double (&o)[V]) {
#pragma unroll
  for (int e = 0; e < V; ++e) __builtin_nontemporal_store(o[e], a + i * V + e);
}

__device__ double block_sum(double v) {
  __shared__ double sh[BLK / WV];
  for (int o = WV / 2; o > 0; o >>= 1) v += __shfl_down(v, o, WV);
  if ((threadIdx.x & (WV - 1)) == 0) sh[threadIdx.x / WV] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < BLK / WV; ++w) s += sh[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ void write_partials(double s0, double s1, double* partial) {
  s0 = block_sum(s0);
  s1 = block_sum(s1);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s0;
    partial[RED_BLOCKS + blockIdx.x] = s1;
  }
}

// fixed-order sum of the partials: out[0] (and out[1] with nd = 2);
// hist (may be null) also takes the second sum, the r.r history
__global__ void __launch_bounds__(BLK)
    k_mg_finish(const double* __restrict__ partial, int nb, int nd, double* __restrict__ out,
                double* __restrict__ hist) {
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < nb; i += BLK) {
    s0 += partial[i];
    s1 += partial[RED_BLOCKS + i];
  }
  s0 = block_sum(s0);
  s1 = block_sum(s1);
  if (threadIdx.x == 0) {
    out[0] = s0;
    if (nd > 1) out[1] = s1;
    if (hist) *hist = s1;
  }
}

// diag -> 1 / diag, 0 on fixed DOFs (the flag every pass reads with it)
__global__ void k_mg_invert(double* __restrict__ d, const uint8_t* __restrict__ fixed, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)BLK + threadIdx.x; t < n; t += (int64_t)gridDim.x * BLK)
    d[t] = fixed[t] ? 0.0 : 1.0 / d[t];
}

// The passes walk n / V items of V DOFs in a grid-stride sequence, UNR / V
// items at a time; the n % V last DOFs go to thread 0 of block 0.
//
// First Chebyshev step.  ADD = false (from zero): d = D^-1 b / theta, x = d;
// b, D^-1 read, d, x written.  ADD = true (from x, q = A x): r = (b - q) on
// free DOFs and 0 elsewhere, d = D^-1 r / theta, x += d.
template <int V, bool ADD>
__global__ void __launch_bounds__(BLK)
    k_mg_first(const double* __restrict__ b, const double* __restrict__ q,
               const double* __restrict__ dinv, double inv_theta, double* __restrict__ r,
               double* __restrict__ d, double* __restrict__ x, int64_t n) {
  constexpr int U = UNR / V;
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double bv[U][V], qv[U][V], iv[U][V], xv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(b, i, bv[u]);
      ldv<V>(dinv, i, iv[u]);
      if (ADD) {
        ldv<V>(q, i, qv[u]);
        ldv<V>(x, i, xv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * st >= nv) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (ADD) bv[u][e] = iv[u][e] != 0.0 ? bv[u][e] - qv[u][e] : 0.0;
        const double dt = iv[u][e] * bv[u][e] * inv_theta;
        xv[u][e] = ADD ? xv[u][e] + dt : dt;
        iv[u][e] = dt;
      }
      if (ADD) stv<V>(r, i0 + u * st, bv[u]);
      stv<V>(d, i0 + u * st, iv[u]);
      stv<V>(x, i0 + u * st, xv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) {
      double rt = b[t];
      if (ADD) r[t] = rt = dinv[t] != 0.0 ? rt - q[t] : 0.0;
      const double dt = dinv[t] * rt * inv_theta;
      x[t] = ADD ? x[t] + dt : dt;
      d[t] = dt;
    }
}

// A later Chebyshev step, after q = A d: r = r_in - q, d = c1 d + c2 D^-1 r,
// x += d (r_in is b in the first step after a start from zero).  WRITE_R =
// false in the smoother's last step, whose r nothing reads.
template <int V, bool WRITE_R>
__global__ void __launch_bounds__(BLK)
    k_mg_step(const double* __restrict__ q, const double* r_in, double* r_out,
              double* __restrict__ d, double* __restrict__ x, const double* __restrict__ dinv,
              double c1, double c2, int64_t n) {
  constexpr int U = UNR / V;
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double qv[U][V], rv[U][V], dv[U][V], xv[U][V], iv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(q, i, qv[u]);
      ldv<V>(r_in, i, rv[u]);
      ldv<V>(d, i, dv[u]);
      ldv<V>(x, i, xv[u]);
      ldv<V>(dinv, i, iv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * st >= nv) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        rv[u][e] -= qv[u][e];
        dv[u][e] = fma(c1, dv[u][e], c2 * (iv[u][e] * rv[u][e]));
        xv[u][e] += dv[u][e];
      }
      if (WRITE_R) stv<V>(r_out, i0 + u * st, rv[u]);
      stv<V>(d, i0 + u * st, dv[u]);
      stv<V>(x, i0 + u * st, xv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) {
      const double rt = r_in[t] - q[t];
      const double dt = fma(c1, d[t], c2 * (dinv[t] * rt));
      if (WRITE_R) r_out[t] = rt;
      d[t] = dt;
      x[t] += dt;
    }
}

// MODE 0, residual and mask: out = (a - c) on free DOFs, 0 elsewhere (a = b,
// c = A x: what restrict reads).  MODE 1, prolong-add: out = a + c on free
// DOFs, a elsewhere (a = out = x, c = the prolonged correction).
template <int V, int MODE>
__global__ void __launch_bounds__(BLK)
    k_mg_combine(const double* a, const double* __restrict__ c, const double* __restrict__ dinv,
                 double* out, int64_t n) {
  constexpr int U = UNR / V;
  auto one = [](double at, double ct, double it) {
    return MODE == 0 ? (it != 0.0 ? at - ct : 0.0) : (it != 0.0 ? at + ct : at);
  };
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double av[U][V], cv[U][V], iv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(a, i, av[u]);
      ldv<V>(c, i, cv[u]);
      ldv<V>(dinv, i, iv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * st >= nv) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) av[u][e] = one(av[u][e], cv[u][e], iv[u][e]);
      stv<V>(out, i0 + u * st, av[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) out[t] = one(a[t], c[t], dinv[t]);
}

// ---- PCG with a general z (the shape of k_cg_residual / k_cg_step)
// r = (b - q) on free DOFs (q = A x), partial sums of r.r
template <int V>
__global__ void __launch_bounds__(BLK)
    k_mg_cg_start(const double* __restrict__ b, const double* __restrict__ q,
                  const double* __restrict__ dinv, double* __restrict__ r, int64_t n,
                  double* __restrict__ partial) {
  double s1 = 0.0;
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i = blockIdx.x * (int64_t)BLK + threadIdx.x; i < nv; i += st) {
    double bv[V], qv[V], iv[V];
    ldv<V>(b, i, bv);
    ldv<V>(q, i, qv);
    ldv<V>(dinv, i, iv);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      bv[e] = iv[e] != 0.0 ? bv[e] - qv[e] : 0.0;
      s1 = fma(bv[e], bv[e], s1);
    }
    stv<V>(r, i, bv);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) {
      const double rt = dinv[t] != 0.0 ? b[t] - q[t] : 0.0;
      r[t] = rt;
      s1 = fma(rt, rt, s1);
    }
  write_partials(0.0, s1, partial);
}

// partial sums of r.z (z = 0 on fixed DOFs)
__global__ void __launch_bounds__(BLK)
    k_mg_cg_rz(const double* __restrict__ r, const double* __restrict__ z, int64_t n,
               double* __restrict__ partial) {
  constexpr int V = 2, U = UNR / V;
  double s0 = 0.0;
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double rv[U][V], zv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(r, i, rv[u]);
      ldv<V>(z, i, zv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * st < nv)
#pragma unroll
        for (int e = 0; e < V; ++e) s0 = fma(rv[u][e], zv[u][e], s0);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) s0 = fma(r[t], z[t], s0);
  write_partials(s0, 0.0, partial);
}

// p = z + beta p, beta = rz_new / rz_old on the device (FIRST: p = z)
template <bool FIRST>
__global__ void __launch_bounds__(BLK)
    k_mg_cg_dir(const double* __restrict__ z, double* __restrict__ p,
                const double* __restrict__ rz_new, const double* __restrict__ rz_old, int64_t n) {
  constexpr int V = 2, U = UNR / V;
  double beta = 0.0;
  if (!FIRST) {
    const double den = *rz_old;
    beta = den != 0.0 ? *rz_new / den : 0.0;
  }
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double zv[U][V], pv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(z, i, zv[u]);
      if (!FIRST) ldv<V>(p, i, pv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * st >= nv) continue;
      if (!FIRST)
#pragma unroll
        for (int e = 0; e < V; ++e) zv[u][e] = fma(beta, pv[u][e], zv[u][e]);
      stv<V>(p, i0 + u * st, zv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) p[t] = FIRST ? z[t] : fma(beta, p[t], z[t]);
}

// alpha = rz / pq on the device; x += alpha p; r -= alpha q on free DOFs;
// partial sums of r.r
template <int V>
__global__ void __launch_bounds__(BLK)
    k_mg_cg_update(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                   const double* __restrict__ q, const double* __restrict__ dinv,
                   const double* __restrict__ rz, const double* __restrict__ pq, int64_t n,
                   double* __restrict__ partial) {
  constexpr int U = UNR / V;
  const double den = *pq;
  const double alpha = den != 0.0 ? *rz / den : 0.0;
  double s1 = 0.0;
  const int64_t nv = n / V, st = (int64_t)gridDim.x * BLK;
  for (int64_t i0 = blockIdx.x * (int64_t)BLK + threadIdx.x; i0 < nv; i0 += U * st) {
    double xv[U][V], rv[U][V], pv[U][V], qv[U][V], iv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * st < nv ? i0 + u * st : 0;
      ldv<V>(x, i, xv[u]);
      ldv<V>(r, i, rv[u]);
      ldv<V>(p, i, pv[u]);
      ldv<V>(q, i, qv[u]);
      ldv<V>(dinv, i, iv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * st >= nv) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        xv[u][e] = fma(alpha, pv[u][e], xv[u][e]);
        rv[u][e] = iv[u][e] != 0.0 ? fma(-alpha, qv[u][e], rv[u][e]) : 0.0;
        s1 = fma(rv[u][e], rv[u][e], s1);
      }
      stv<V>(x, i0 + u * st, xv[u]);
      stv<V>(r, i0 + u * st, rv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * V; t < n; ++t) {
      x[t] = fma(alpha, p[t], x[t]);
      const double rt = dinv[t] != 0.0 ? fma(-alpha, q[t], r[t]) : 0.0;
      r[t] = rt;
      s1 = fma(rt, rt, s1);
    }
  write_partials(0.0, s1, partial);
}

// ------------------------------------------------------------------ the cycle
inline bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

int action(Level& v, const double* u, double* y, hipStream_t st) {
  ++v.run_actions;
  return sem_apply(v.ctx, SEM_OP_POISSON, u, y, 0, st);
}

// x = Chebyshev(b) of the level's degree, from zero (ADD = false) or from x
// (ADD = true: the residual b - A x is formed in the first pass); v2: b and x
// allow 16-byte accesses
template <int V>
int smooth(Level& v, const double* b, double* x, bool add, hipStream_t st) {
  const dim3 grid(grid_for(v.n)), blk(BLK);
  const semmg::Cheb& c = v.cheb;
  if (add) {
    SEM_TRY(action(v, x, v.q, st));
    hipLaunchKernelGGL((k_mg_first<V, true>), grid, blk, 0, st, b, v.q, v.dinv, c.inv_theta, v.r,
                       v.d, x, v.n);
  } else {
    hipLaunchKernelGGL((k_mg_first<V, false>), grid, blk, 0, st, b, nullptr, v.dinv, c.inv_theta,
                       v.r, v.d, x, v.n);
  }
  ++v.run_passes;
  for (int j = 1; j < v.degree; ++j) {
    SEM_TRY(action(v, v.d, v.q, st));
    const double* r_in = (!add && j == 1) ? b : v.r;
    if (j + 1 < v.degree)
      hipLaunchKernelGGL((k_mg_step<V, true>), grid, blk, 0, st, v.q, r_in, v.r, v.d, x, v.dinv,
                         c.c1[(size_t)j], c.c2[(size_t)j], v.n);
    else
      hipLaunchKernelGGL((k_mg_step<V, false>), grid, blk, 0, st, v.q, r_in, v.r, v.d, x, v.dinv,
                         c.c1[(size_t)j], c.c2[(size_t)j], v.n);
    ++v.run_passes;
  }
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int smooth(Level& v, const double* b, double* x, bool add, bool v2, hipStream_t st) {
  return v2 ? smooth<2>(v, b, x, add, st) : smooth<1>(v, b, x, add, st);
}

// z = M r.  marks (may be null): 2 * n_levels events recorded at the
// boundaries of the levels' segments (sem_mg_profile).
int cycle(sem_mg* mg, const double* d_r, double* d_z, hipStream_t st, hipEvent_t* marks) {
  const int L = mg->n_levels;
  const bool v2 = aligned16(d_r) && aligned16(d_z);
  for (auto& v : mg->lv) v.run_actions = v.run_passes = 0;
  int mark = 0;
  if (marks) HIP_TRY(hipEventRecord(marks[mark++], st));
  for (int l = 0; l + 1 < L; ++l) {
    Level& v = mg->lv[(size_t)l];
    Level& c = mg->lv[(size_t)l + 1];
    const double* b = l ? v.b : d_r;
    double* x = l ? v.x : d_z;
    const bool vv = l ? true : v2;
    const dim3 grid(grid_for(v.n)), blk(BLK);
    SEM_TRY(smooth(v, b, x, false, vv, st));
    SEM_TRY(action(v, x, v.q, st));
    if (vv)
      hipLaunchKernelGGL((k_mg_combine<2, 0>), grid, blk, 0, st, b, v.q, v.dinv, v.r, v.n);
    else
      hipLaunchKernelGGL((k_mg_combine<1, 0>), grid, blk, 0, st, b, v.q, v.dinv, v.r, v.n);
    ++v.run_passes;
    HIP_TRY(hipGetLastError());
    SEM_TRY(sem_transfer_restrict(v.down, 1, v.n, 1, v.r, c.n, 1, c.b, 0, st));
    if (marks) HIP_TRY(hipEventRecord(marks[mark++], st));
  }
  {
    Level& v = mg->lv[(size_t)L - 1];
    SEM_TRY(smooth(v, L > 1 ? v.b : d_r, L > 1 ? v.x : d_z, false, L > 1 ? true : v2, st));
    if (marks) HIP_TRY(hipEventRecord(marks[mark++], st));
  }
  for (int l = L - 2; l >= 0; --l) {
    Level& v = mg->lv[(size_t)l];
    Level& c = mg->lv[(size_t)l + 1];
    const double* b = l ? v.b : d_r;
    double* x = l ? v.x : d_z;
    const bool vv = l ? true : v2;
    const dim3 grid(grid_for(v.n)), blk(BLK);
    SEM_TRY(sem_transfer_prolong(v.down, 1, c.n, 1, c.x, v.n, 1, v.e, st));
    if (vv)
      hipLaunchKernelGGL((k_mg_combine<2, 1>), grid, blk, 0, st, x, v.e, v.dinv, x, v.n);
    else
      hipLaunchKernelGGL((k_mg_combine<1, 1>), grid, blk, 0, st, x, v.e, v.dinv, x, v.n);
    ++v.run_passes;
    HIP_TRY(hipGetLastError());
    SEM_TRY(smooth(v, b, x, true, vv, st));
    if (marks) HIP_TRY(hipEventRecord(marks[mark++], st));
  }
  return SEM_OK;
}

struct SolveScratch {
  double* hist = nullptr;
  double* h_hist = nullptr;  // pinned
  ~SolveScratch() {
    (void)hipFree(hist);
    (void)hipHostFree(h_hist);
  }
};

}  // namespace

extern "C" {

int sem_mg_create(sem_mg** out, int n_levels, sem_ctx* const* ctxs, sem_transfer* const* transfers,
                  const uint8_t* const* d_dirichlet, const double* h_lambda_max,
                  int smooth_degree, int coarse_degree, double smooth_ratio, double coarse_ratio,
                  int device, void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_mg_create: out is NULL");
  *out = nullptr;
  SEM_TRY(semmg::check_create(n_levels, reinterpret_cast<const void* const*>(ctxs),
                              reinterpret_cast<const void* const*>(transfers),
                              reinterpret_cast<const void* const*>(d_dirichlet), h_lambda_max,
                              smooth_degree, coarse_degree, smooth_ratio, coarse_ratio));
  if (device < 0) return fail(SEM_E_INVALID, "sem_mg_create: device must be >= 0");
  for (int l = 0; l < n_levels; ++l) {
    if (sem::ctx_dpn(ctxs[l]) != 1)
      return fail(SEM_E_NOTIMPL, "sem_mg_create: Poisson contexts with one DOF per node");
    if (sem::ctx_device(ctxs[l]) != device)
      return fail(SEM_E_INVALID, "sem_mg_create: level " + std::to_string(l) +
                                     " lives on another device");
    if (l + 1 < n_levels) {
      int64_t ti[6];
      SEM_TRY(sem_transfer_info(transfers[l], ti, 6));
      SEM_TRY(semmg::check_level_sizes(l, sem::ctx_ndof(ctxs[l]), sem::ctx_ndof(ctxs[l + 1]),
                                       ti[4], ti[5]));
    }
  }
  Guard guard(device);
  hipStream_t st = S(stream);
  sem_mg* mg = new sem_mg();
  mg->device = device;
  mg->n_levels = n_levels;
  mg->smooth_degree = smooth_degree;
  mg->coarse_degree = coarse_degree;
  mg->lv.resize((size_t)n_levels);
  std::vector<int> actions, passes;
  semmg::cycle_counts(n_levels, smooth_degree, coarse_degree, actions, passes);
#define MG_TRY_HIP(expr)                                                             \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      sem_mg_destroy(mg);                                                            \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
#define MG_TRY(expr)       \
  do {                     \
    int _rc = (expr);      \
    if (_rc) {             \
      sem_mg_destroy(mg);  \
      return _rc;          \
    }                      \
  } while (0)
  for (int l = 0; l < n_levels; ++l) {
    Level& v = mg->lv[(size_t)l];
    const bool last = l == n_levels - 1;
    v.ctx = ctxs[l];
    v.down = last ? nullptr : transfers[l];
    v.n = sem::ctx_ndof(ctxs[l]);
    v.nn = (std::max<int64_t>(v.n, 1) + 31) / 32 * 32;
    v.degree = last ? coarse_degree : smooth_degree;
    v.actions = actions[(size_t)l];
    v.passes = passes[(size_t)l];
    MG_TRY(semmg::chebyshev(v.degree, h_lambda_max[l], last ? coarse_ratio : smooth_ratio,
                            v.cheb));
    const size_t bytes = 7 * (size_t)v.nn * sizeof(double);
    MG_TRY_HIP(hipMalloc(&v.base, bytes));
    // the prolong scratch keeps 0 on nodes no element references
    MG_TRY_HIP(hipMemsetAsync(v.base, 0, bytes, st));
    mg->vector_bytes += bytes;
    v.dinv = v.base;
    v.b = v.dinv + v.nn;
    v.x = v.b + v.nn;
    v.r = v.x + v.nn;
    v.d = v.r + v.nn;
    v.q = v.d + v.nn;
    v.e = v.q + v.nn;
    MG_TRY(sem_diag(v.ctx, SEM_OP_POISSON, v.dinv, st));
    hipLaunchKernelGGL(k_mg_invert, dim3(grid_for(v.n)), dim3(BLK), 0, st, v.dinv, d_dirichlet[l],
                       v.n);
    MG_TRY_HIP(hipGetLastError());
  }
  MG_TRY_HIP(hipMalloc(&mg->p, (size_t)mg->lv[0].nn * sizeof(double)));
  MG_TRY_HIP(hipMalloc(&mg->red, (2 * RED_BLOCKS + 8) * sizeof(double)));
  mg->vector_bytes += (size_t)mg->lv[0].nn * sizeof(double);
  MG_TRY_HIP(hipStreamSynchronize(st));  // the masks are free again
#undef MG_TRY_HIP
#undef MG_TRY
  *out = mg;
  return SEM_OK;
}

void sem_mg_destroy(sem_mg* mg) {
  if (!mg) return;
  {
    Guard guard(mg->device);
    for (auto& v : mg->lv) (void)hipFree(v.base);
    (void)hipFree(mg->p);
    (void)hipFree(mg->red);
  }
  delete mg;
}

int sem_mg_vcycle(sem_mg* mg, const double* d_r, double* d_z, void* stream) {
  if (!mg || !d_r || !d_z) return fail(SEM_E_INVALID, "sem_mg_vcycle: NULL argument");
  if (d_r == d_z) return fail(SEM_E_INVALID, "sem_mg_vcycle: d_z must not alias d_r");
  Guard guard(mg->device);
  return cycle(mg, d_r, d_z, S(stream), nullptr);
}

int sem_mg_profile(sem_mg* mg, const double* d_r, double* d_z, double* h_ms, void* stream) {
  if (!mg || !d_r || !d_z || !h_ms) return fail(SEM_E_INVALID, "sem_mg_profile: NULL argument");
  if (d_r == d_z) return fail(SEM_E_INVALID, "sem_mg_profile: d_z must not alias d_r");
  Guard guard(mg->device);
  const int L = mg->n_levels;
  std::vector<hipEvent_t> marks((size_t)(2 * L), nullptr);
  int rc = SEM_OK;
  for (auto& m : marks)
    if (hipEventCreate(&m) != hipSuccess) rc = fail(SEM_E_HIP, "sem_mg_profile: hipEventCreate");
  if (rc == SEM_OK) rc = cycle(mg, d_r, d_z, S(stream), marks.data());
  if (rc == SEM_OK && hipStreamSynchronize(S(stream)) != hipSuccess)
    rc = fail(SEM_E_HIP, "sem_mg_profile: hipStreamSynchronize");
  if (rc == SEM_OK) {
    // segments in stream order: down 0 .. L-2, the coarsest, up L-2 .. 0
    for (int l = 0; l < L; ++l) h_ms[l] = 0.0;
    for (int s = 0; s + 1 < 2 * L; ++s) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, marks[(size_t)s], marks[(size_t)s + 1]) != hipSuccess) {
        rc = fail(SEM_E_HIP, "sem_mg_profile: hipEventElapsedTime");
        break;
      }
      const int l = s < L ? s : 2 * L - 2 - s;
      h_ms[l] += (double)ms;
    }
  }
  for (auto& m : marks)
    if (m) (void)hipEventDestroy(m);
  return rc;
}

int sem_mg_pcg_solve(sem_mg* mg, const double* d_b, double* d_x, double rtol, int max_iter,
                     int check_every, int* iters, double* relres, void* stream) {
  if (!mg || !d_b || !d_x) return fail(SEM_E_INVALID, "sem_mg_pcg_solve: NULL argument");
  if (max_iter < 0 || !(rtol >= 0.0))
    return fail(SEM_E_INVALID, "sem_mg_pcg_solve: need rtol >= 0, max_iter >= 0");
  const int check = std::max(check_every, 1);
  Guard guard(mg->device);
  hipStream_t st = S(stream);
  Level& f = mg->lv[0];
  const int64_t n = f.n;
  SolveScratch s;
  HIP_TRY(hipMalloc(&s.hist, ((size_t)max_iter + 1) * sizeof(double)));
  HIP_TRY(hipHostMalloc(&s.h_hist, ((size_t)check + 1) * sizeof(double)));
  // the residual lives in the fine level's b row and z in its x row (the
  // cycle of a multi-level hierarchy takes them as its arguments and leaves
  // those two rows alone), q in its q row, which the cycle overwrites only
  // after the update pass has read it
  double *r = f.b, *z = f.x, *q = f.q, *p = mg->p;
  double* partial = mg->red;
  double* RZ[2] = {mg->red + 2 * RED_BLOCKS, mg->red + 2 * RED_BLOCKS + 1};
  double* pq = mg->red + 2 * RED_BLOCKS + 2;
  double* rr = mg->red + 2 * RED_BLOCKS + 4;  // (unused sum, r.r)
  const bool v2 = aligned16(d_b) && aligned16(d_x);
  const dim3 grid(grid_for(n)), blk(BLK);
  const int gb = grid_for(n);
  SEM_TRY(sem_apply(f.ctx, SEM_OP_POISSON, d_x, q, 0, st));
  if (v2)
    hipLaunchKernelGGL(k_mg_cg_start<2>, grid, blk, 0, st, d_b, q, f.dinv, r, n, partial);
  else
    hipLaunchKernelGGL(k_mg_cg_start<1>, grid, blk, 0, st, d_b, q, f.dinv, r, n, partial);
  hipLaunchKernelGGL(k_mg_finish, dim3(1), blk, 0, st, partial, gb, 2, rr, s.hist);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s.h_hist, s.hist, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double rr0 = s.h_hist[0];
  if (!std::isfinite(rr0)) return fail(SEM_E_INVALID, "PCG: non-finite initial residual");
  const double tol2 = rtol * rtol * rr0;
  double rr_last = rr0;
  int it = 0;
  bool done = rr0 == 0.0;
  while (!done && it < max_iter) {
    const int blkn = std::min(check, max_iter - it);
    for (int k = 0; k < blkn; ++k) {
      const int o = it & 1, nw = o ^ 1;
      SEM_TRY(cycle(mg, r, z, st, nullptr));
      hipLaunchKernelGGL(k_mg_cg_rz, grid, blk, 0, st, r, z, n, partial);
      hipLaunchKernelGGL(k_mg_finish, dim3(1), blk, 0, st, partial, gb, 1, RZ[nw], nullptr);
      if (it == 0)
        hipLaunchKernelGGL(k_mg_cg_dir<true>, grid, blk, 0, st, z, p, RZ[nw], RZ[o], n);
      else
        hipLaunchKernelGGL(k_mg_cg_dir<false>, grid, blk, 0, st, z, p, RZ[nw], RZ[o], n);
      HIP_TRY(hipGetLastError());
      // p.q summed inside the action where the plan allows (p = 0 on fixed DOFs)
      SEM_TRY(sem_apply_dot(f.ctx, SEM_OP_POISSON, p, q, pq, st));
      if (v2)
        hipLaunchKernelGGL(k_mg_cg_update<2>, grid, blk, 0, st, d_x, r, p, q, f.dinv, RZ[nw], pq,
                           n, partial);
      else
        hipLaunchKernelGGL(k_mg_cg_update<1>, grid, blk, 0, st, d_x, r, p, q, f.dinv, RZ[nw], pq,
                           n, partial);
      hipLaunchKernelGGL(k_mg_finish, dim3(1), blk, 0, st, partial, gb, 2, rr, s.hist + it + 1);
      HIP_TRY(hipGetLastError());
      ++it;
    }
    HIP_TRY(hipMemcpyAsync(s.h_hist, s.hist + it - blkn + 1, blkn * sizeof(double),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < blkn; ++k) {
      rr_last = s.h_hist[k];
      if (!std::isfinite(rr_last)) return fail(SEM_E_INVALID, "PCG: non-finite residual");
      if (rr_last <= tol2) done = true;
    }
  }
  if (iters) *iters = it;
  if (relres) *relres = rr0 > 0.0 ? std::sqrt(rr_last / rr0) : 0.0;
  if (!done && rtol > 0.0)
    return fail(SEM_E_INVALID, "PCG did not converge in " + std::to_string(max_iter) +
                                   " iterations");
  return SEM_OK;
}

int sem_mg_info(sem_mg* mg, int64_t* info, int n_info) {
  if (!mg || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_mg_info: NULL argument");
  std::vector<int64_t> v = {mg->n_levels, mg->smooth_degree, mg->coarse_degree,
                            (int64_t)mg->vector_bytes};
  for (const auto& l : mg->lv) {
    const int64_t row[5] = {l.n, l.actions, l.passes, l.run_actions, l.run_passes};
    v.insert(v.end(), row, row + 5);
  }
  for (int i = 0; i < std::min<int>(n_info, (int)v.size()); ++i) info[i] = v[(size_t)i];
  return SEM_OK;
}

}  // extern "C"
