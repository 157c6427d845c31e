// Volume fields (include/sem_hip.h, "Volume"): the physical gradient of a
// global field on every element, the continuous nodal gradient recovered from
// it, volume integrals, the discrete L2 / H1 norms and the lumped mass.  The
// batched device form of FiniteElement.gradient / integrate
// (sem/discrete.py:674-689), which the reference runs per element in NumPy.
// Quadrilaterals and hexahedra, p = 1..16.
//
// One element kernel, templated on (ndim, n, mode).  A workgroup of 256 lanes
// holds one element, or 256 / n^ndim small ones side by side (64 at p = 1 in
// 2-D); the last workgroup may be partial.  One field at a time is staged in
// LDS (n^ndim doubles per element, 38.4 KB for a hexahedron at n = 17): first
// u (gathered through the element map, u - v for the error norms), then each
// component of x_phys.  After every staging a lane differentiates the field
// along every axis at its own nodes with rows of D (also in LDS) and keeps the
// results in registers: du/dxi, then J.  A lane owns at most 4 nodes at a
// time; an element with more than 1024 nodes (hexahedra from p = 10) goes
// through the staging again for the next 256 * NPT nodes.  From J the lane
// forms the cofactor inverse and detJ and ends in the mode's epilogue:
//   GRAD     stores grad_j = sum_i invJ[i][j] du/dxi_i;
//   RECOVER  stores detJxW * grad to the handle's scratch; a second kernel,
//            one lane per node, sums the node's CSR row in ascending (element,
//            local) order and divides by the lumped mass;
//   NORMS    reduces detJxW d^2 and detJxW |grad d|^2 over the element;
//   DETJ     (create) stores detJxW and counts detJ <= 0 per element.
// No per-node J / invJ is stored anywhere: geometry is recomputed from x_phys
// (the choice of the NODAL Poisson kernel).  The handle keeps detJxW, one
// double per element node: the integrals are a plain weighted sum over it
// (k_vol_integrate, a power-of-two share of a workgroup's lanes per element),
// which recomputing the geometry lost to a torch composition that reads a
// stored detJxW.  Sums are fixed-order: a lane adds
// its own nodes in ascending order, the lanes of an element are combined by a
// binary tree in LDS, the elements by a second single-workgroup launch per
// value (as sem_faces.hip).  No atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sem_internal.h"
#include "sem_volume_plan.h"

using sem::fail;

#define VOL_BLOCK 256
#define VOL_MAX_NPT 4

struct sem_volume {
  int ndim = 0, p = 0, n = 0, nloc = 0, device = 0;
  int64_t n_elem = 0, n_node = 0, n_referenced = 0, max_row = 0;
  size_t scratch_doubles = 0;
  const double* d_x_phys = nullptr;  // borrowed
  const uint32_t* d_e2n = nullptr;   // borrowed
  int32_t *d_ptr = nullptr, *d_entry = nullptr;
  double *d_D = nullptr, *d_w = nullptr, *d_m = nullptr, *d_wdet = nullptr, *d_scratch = nullptr;
};

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

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

enum { M_GRAD = 0, M_RECOVER = 1, M_NORMS = 2, M_DETJ = 3 };
#define VOL_TOTAL_BLOCK 1024

constexpr int ipow(int n, int d) { return d == 0 ? 1 : n * ipow(n, d - 1); }
constexpr int floor_pow2(int v) { return v < 2 ? 1 : 2 * floor_pow2(v / 2); }

// how a workgroup is shared out
template <int ND, int N>
struct Shape {
  static constexpr int NLOC = ipow(N, ND);
  static constexpr int EPW = NLOC <= VOL_BLOCK / 2 ? VOL_BLOCK / NLOC : 1;  // elements per workgroup
  static constexpr int SLOTS = EPW * NLOC;
  static constexpr int PER = (SLOTS + VOL_BLOCK - 1) / VOL_BLOCK;  // nodes per lane in all
  // hexahedra at n = 16: a lane's nodes (256 apart) share their lines along
  // two axes, the compiler keeps all of them live and four nodes spill
  static constexpr int MAX_NPT = ND == 3 && N == 16 ? 2 : VOL_MAX_NPT;
  static constexpr int PASSES = (PER + MAX_NPT - 1) / MAX_NPT;
  static constexpr int NPT = (PER + PASSES - 1) / PASSES;  // nodes per lane per pass
  static constexpr int SEG = NLOC < VOL_BLOCK ? NLOC : VOL_BLOCK;  // lanes of one element
  static constexpr int P2 = floor_pow2(SEG);
};

// what every launch of the element kernel reads
struct VolArgs {
  int64_t n_elem;
  const double* x_phys;
  const uint32_t* e2n;
  const double *D, *w;
};

// d f / d xi_i (i < ND) at the local node l of the staged element f
template <int ND, int N>
__device__ inline void local_derivs(const double* f, const double* sD, int l, double* d) {
  int st = 1;
#pragma unroll
  for (int i = ND - 1; i >= 0; --i) {
    const int ai = (l / st) % N;
    const double* line = f + (l - ai * st);
    const double* row = sD + ai * N;
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < N; ++m) acc += row[m] * line[m * st];
    d[i] = acc;
    st *= N;
  }
}

// inv[i][j] = d xi_i / d x_j and det of J[c][i] = d x_c / d xi_i, by cofactors
template <int ND>
__device__ inline double inverse(const double (*J)[ND], double (*inv)[ND]) {
  if constexpr (ND == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double r = 1.0 / det;
    inv[0][0] = J[1][1] * r;
    inv[0][1] = -J[0][1] * r;
    inv[1][0] = -J[1][0] * r;
    inv[1][1] = J[0][0] * r;
    return det;
  } else {
    double C[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        C[r][k] = J[r1][k1] * J[r2][k2] - J[r1][k2] * J[r2][k1];
      }
    const double det = J[0][0] * C[0][0] + J[0][1] * C[0][1] + J[0][2] * C[0][2];
    const double rd = 1.0 / det;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) inv[i][j] = C[j][i] * rd;
    return det;
  }
}

template <int ND, int N>
__device__ inline double quad_weight(const double* sW, int l) {
  if constexpr (ND == 2)
    return sW[l / N] * sW[l % N];
  else
    return sW[l / (N * N)] * sW[(l / N) % N] * sW[l % N];
}

// grid (ceil(n_elem / EPW), components).  u is read as u[c * cs + node * ns];
// v (NORMS) may be NULL.  out: GRAD / RECOVER [c][n_elem][ND][NLOC], DETJ
// [n_elem][NLOC].  red: NORMS [c][n_elem][2], DETJ [n_elem].
template <int ND, int N, int MODE>
__global__ void __launch_bounds__(VOL_BLOCK)
    k_vol_elem(VolArgs A, int64_t cs, int64_t ns, const double* __restrict__ u,
               const double* __restrict__ v, double* __restrict__ out,
               double* __restrict__ red) {
  using Sh = Shape<ND, N>;
  constexpr int NLOC = Sh::NLOC, EPW = Sh::EPW, SLOTS = Sh::SLOTS, NPT = Sh::NPT;
  constexpr bool GRADIENT = MODE == M_GRAD || MODE == M_RECOVER || MODE == M_NORMS;
  constexpr bool REDUCE = MODE == M_NORMS || MODE == M_DETJ;
  __shared__ double sD[N * N];
  __shared__ double sW[N];
  __shared__ double sF[SLOTS];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.y;
  const int64_t e0 = blockIdx.x * (int64_t)EPW;
  for (int k = t; k < N * N; k += VOL_BLOCK) sD[k] = A.D[k];
  if (t < N) sW[t] = A.w[t];
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 1
  for (int ps = 0; ps < Sh::PASSES; ++ps) {
    double du[NPT][ND], d0[NPT], J[NPT][ND][ND];
    if constexpr (GRADIENT) {
      __syncthreads();  // the readers of the pass before are done
      for (int s = t; s < SLOTS; s += VOL_BLOCK) {
        const int64_t e = e0 + s / NLOC;
        double val = 0.0;
        if (e < A.n_elem) {
          const int64_t off = c * cs + (int64_t)A.e2n[e * NLOC + s % NLOC] * ns;
          val = u[off];
          if (MODE == M_NORMS && v) val -= v[off];
        }
        sF[s] = val;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const int s = (ps * NPT + k) * VOL_BLOCK + t;
        d0[k] = 0.0;
#pragma unroll
        for (int i = 0; i < ND; ++i) du[k][i] = 0.0;
        if (s < SLOTS) {
          local_derivs<ND, N>(sF + s / NLOC * NLOC, sD, s % NLOC, du[k]);
          d0[k] = sF[s];
        }
      }
    }
#pragma unroll
    for (int cx = 0; cx < ND; ++cx) {
      __syncthreads();
      for (int s = t; s < SLOTS; s += VOL_BLOCK) {
        const int64_t e = e0 + s / NLOC;
        sF[s] = e < A.n_elem ? A.x_phys[(e * ND + cx) * NLOC + s % NLOC] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const int s = (ps * NPT + k) * VOL_BLOCK + t;
#pragma unroll
        for (int i = 0; i < ND; ++i) J[k][cx][i] = 0.0;
        if (s < SLOTS) local_derivs<ND, N>(sF + s / NLOC * NLOC, sD, s % NLOC, J[k][cx]);
      }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int s = (ps * NPT + k) * VOL_BLOCK + t;
      const int64_t e = e0 + s / NLOC;
      if (s >= SLOTS || e >= A.n_elem) continue;
      const int l = s % NLOC;
      double inv[ND][ND];
      const double det = inverse<ND>(J[k], inv);
      const double wdet = det * quad_weight<ND, N>(sW, l);
      double g[ND];
      if constexpr (GRADIENT) {
#pragma unroll
        for (int j = 0; j < ND; ++j) {
          double a = 0.0;
#pragma unroll
          for (int i = 0; i < ND; ++i) a += inv[i][j] * du[k][i];
          g[j] = a;
        }
      }
      if constexpr (MODE == M_GRAD || MODE == M_RECOVER) {
        const double sc = MODE == M_RECOVER ? wdet : 1.0;
#pragma unroll
        for (int j = 0; j < ND; ++j) out[((c * A.n_elem + e) * ND + j) * NLOC + l] = sc * g[j];
      } else if constexpr (MODE == M_NORMS) {
        double g2 = 0.0;
#pragma unroll
        for (int j = 0; j < ND; ++j) g2 += g[j] * g[j];
        acc0 += wdet * (d0[k] * d0[k]);
        acc1 += wdet * g2;
      } else {
        out[e * NLOC + l] = wdet;
        acc0 += det > 0.0 ? 0.0 : 1.0;
      }
    }
  }
  if constexpr (REDUCE) {
    // the lanes of one element, combined in a fixed order
    constexpr int SEG = Sh::SEG, P2 = Sh::P2;
    __shared__ double r0[VOL_BLOCK];
    __shared__ double r1[MODE == M_NORMS ? VOL_BLOCK : 1];
    r0[t] = acc0;
    if constexpr (MODE == M_NORMS) r1[t] = acc1;
    __syncthreads();
    const int sub = t / SEG, q = t % SEG;
    const bool mine = sub < EPW;
    if constexpr (P2 < SEG) {
      if (mine && q < SEG - P2) {
        r0[t] += r0[t + P2];
        if constexpr (MODE == M_NORMS) r1[t] += r1[t + P2];
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int h = P2 / 2; h > 0; h >>= 1) {
      if (mine && q < h) {
        r0[t] += r0[t + h];
        if constexpr (MODE == M_NORMS) r1[t] += r1[t + h];
      }
      __syncthreads();
    }
    const int64_t e = e0 + sub;
    if (mine && q == 0 && e < A.n_elem) {
      if constexpr (MODE == M_NORMS) {
        red[(c * A.n_elem + e) * 2] = r0[t];
        red[(c * A.n_elem + e) * 2 + 1] = r1[t];
      } else {
        red[c * A.n_elem + e] = r0[t];
      }
    }
  }
}

// per_elem[c][e] = sum_l wdet[e][l] * value: lpe lanes (a power of two, 4 ..
// 64) per element, 256 / lpe elements per workgroup; grid (ceil(n_elem /
// (256 / lpe)), components).  value = u[c * cs + e2n[e][l] * ns], or with
// local != 0 u[(c * n_elem + e) * nloc + l].
__global__ void __launch_bounds__(VOL_BLOCK)
    k_vol_integrate(int64_t n_elem, int nloc, int lpe, const double* __restrict__ wdet,
                    const uint32_t* __restrict__ e2n, int64_t cs, int64_t ns,
                    const double* __restrict__ u, int local, double* __restrict__ per_elem) {
  __shared__ double r[VOL_BLOCK];
  const int t = threadIdx.x, lane = t % lpe;
  const int64_t c = blockIdx.y;
  const int64_t e = blockIdx.x * (int64_t)(VOL_BLOCK / lpe) + t / lpe;
  double acc = 0.0;
  if (e < n_elem) {
    const double* wd = wdet + e * nloc;
    if (local) {
      const double* ue = u + (c * n_elem + e) * nloc;
      for (int l = lane; l < nloc; l += lpe) acc += wd[l] * ue[l];
    } else {
      const uint32_t* map = e2n + e * nloc;
      const double* uc = u + c * cs;
      for (int l = lane; l < nloc; l += lpe) acc += wd[l] * uc[(int64_t)map[l] * ns];
    }
  }
  r[t] = acc;
  __syncthreads();
  for (int h = lpe / 2; h > 0; h >>= 1) {
    if (lane < h) r[t] += r[t + h];
    __syncthreads();
  }
  if (lane == 0 && e < n_elem) per_elem[c * n_elem + e] = r[t];
}

// total[k] = sum_e per_elem[(k / nq * n_elem + e) * nq + k % nq]: one
// workgroup per value, fixed order (four running sums per lane keep four
// loads in flight)
__global__ void __launch_bounds__(VOL_TOTAL_BLOCK)
    k_vol_total(int64_t n_elem, int nq, const double* __restrict__ per_elem,
                double* __restrict__ total) {
  constexpr int B = VOL_TOTAL_BLOCK;
  __shared__ double r[B];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x / nq;
  const int q = blockIdx.x % nq;
  const double* p = per_elem + c * n_elem * nq + q;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t e = t; e < n_elem; e += 4 * B) {
    a0 += p[e * nq];
    if (e + B < n_elem) a1 += p[(e + B) * nq];
    if (e + 2 * B < n_elem) a2 += p[(e + 2 * B) * nq];
    if (e + 3 * B < n_elem) a3 += p[(e + 3 * B) * nq];
  }
  r[t] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  for (int h = B / 2; h > 0; h >>= 1) {
    if (t < h) r[t] += r[t + h];
    __syncthreads();
  }
  if (t == 0) total[blockIdx.x] = r[0];
}

// m[g] = sum of detJxW over node g's CSR row, in the row's order
__global__ void __launch_bounds__(VOL_BLOCK)
    k_vol_mass(int64_t n_node, const int32_t* __restrict__ ptr, const int32_t* __restrict__ entry,
               const double* __restrict__ wdet, double* __restrict__ m) {
  const int64_t g = blockIdx.x * (int64_t)VOL_BLOCK + threadIdx.x;
  if (g >= n_node) return;
  double acc = 0.0;
  for (int32_t k = ptr[g]; k < ptr[g + 1]; ++k) acc += wdet[entry[k]];
  m[g] = acc;
}

// out[j][g] = (sum over node g's CSR row of scratch[e][j][l]) / m[g], 0 for a
// node without a row; grid (ceil(n_node / 256), ndim)
__global__ void __launch_bounds__(VOL_BLOCK)
    k_vol_nodes(int64_t n_node, int ndim, int nloc, const int32_t* __restrict__ ptr,
                const int32_t* __restrict__ entry, const double* __restrict__ scratch,
                const double* __restrict__ m, int64_t ds, int64_t ns, double* __restrict__ out) {
  const int64_t g = blockIdx.x * (int64_t)VOL_BLOCK + threadIdx.x;
  if (g >= n_node) return;
  const int j = blockIdx.y;
  const int32_t b = ptr[g], e = ptr[g + 1];
  double acc = 0.0;
  for (int32_t k = b; k < e; ++k) {
    const int64_t en = entry[k];
    const int64_t el = en / nloc;
    acc += scratch[(el * ndim + j) * nloc + (en - el * nloc)];
  }
  out[j * ds + g * ns] = b == e ? 0.0 : acc / m[g];
}

template <int MODE, int ND, int N>
void launch_one(const sem_volume* V, int ncomp, int64_t cs, int64_t ns, const double* u,
                const double* v, double* out, double* red, hipStream_t st) {
  const VolArgs A = {V->n_elem, V->d_x_phys, V->d_e2n, V->d_D, V->d_w};
  const dim3 grid(blocks_for(V->n_elem, Shape<ND, N>::EPW), (unsigned)ncomp);
  k_vol_elem<ND, N, MODE><<<grid, VOL_BLOCK, 0, st>>>(A, cs, ns, u, v, out, red);
}

template <int MODE, int ND>
void launch_nd(const sem_volume* V, int ncomp, int64_t cs, int64_t ns, const double* u,
               const double* v, double* out, double* red, hipStream_t st) {
  switch (V->n) {
#define VOL_CASE(N)                                                        \
  case N:                                                                  \
    launch_one<MODE, ND, N>(V, ncomp, cs, ns, u, v, out, red, st);        \
    break;
    VOL_CASE(2) VOL_CASE(3) VOL_CASE(4) VOL_CASE(5) VOL_CASE(6) VOL_CASE(7) VOL_CASE(8) VOL_CASE(9)
    VOL_CASE(10) VOL_CASE(11) VOL_CASE(12) VOL_CASE(13) VOL_CASE(14) VOL_CASE(15) VOL_CASE(16)
    VOL_CASE(17)
#undef VOL_CASE
  }
}

// the element kernel of the handle's (ndim, n); n_elem > 0
template <int MODE>
void launch_elem(const sem_volume* V, int ncomp, int64_t cs, int64_t ns, const double* u,
                 const double* v, double* out, double* red, hipStream_t st) {
  if (V->ndim == 2)
    launch_nd<MODE, 2>(V, ncomp, cs, ns, u, v, out, red, st);
  else
    launch_nd<MODE, 3>(V, ncomp, cs, ns, u, v, out, red, st);
}

int check_fields(const sem_volume* V, const char* what, int ncomp, int64_t comp_stride,
                 int64_t node_stride) {
  if (!V) return fail(SEM_E_INVALID, std::string(what) + ": volume is NULL");
  if (ncomp < 1 || ncomp > 65535)
    return fail(SEM_E_INVALID, std::string(what) + ": ncomp must be in [1, 65535]");
  if (comp_stride < 0 || node_stride < 1)
    return fail(SEM_E_INVALID, std::string(what) + ": comp_stride >= 0 and node_stride >= 1");
  return SEM_OK;
}

}  // namespace

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

namespace {

// nq values per (component, element) -- nq = 2: the norms' element kernel,
// nq = 1: the weighted sum over the stored detJxW -- then summed over the
// elements: into the caller's d_per_elem, or through the handle's scratch a
// few components at a time
int reduce_fields(sem_volume* V, int nq, int ncomp, int64_t cs, int64_t ns, const double* d_u,
                  const double* d_v, int local, double* d_per_elem, double* d_total, void* stream) {
  const int64_t E = V->n_elem;
  if (!d_per_elem && !d_total) return SEM_OK;
  Guard guard(V->device);
  // components the scratch holds (n_elem * nq values each)
  const int64_t cap = E > 0 ? (int64_t)(V->scratch_doubles / (size_t)(E * nq)) : ncomp;
  const int chunk = d_per_elem ? ncomp : (int)std::min<int64_t>(ncomp, cap);
  for (int c0 = 0; c0 < ncomp; c0 += chunk) {
    const int nc = std::min(chunk, ncomp - c0);
    double* buf = d_per_elem ? d_per_elem : V->d_scratch;
    if (E > 0) {
      const double* uc = local ? d_u + (int64_t)c0 * E * V->nloc : d_u + c0 * cs;
      const double* vc = d_v ? d_v + c0 * cs : nullptr;
      if (nq == 2) {
        launch_elem<M_NORMS>(V, nc, cs, ns, uc, vc, nullptr, buf, S(stream));
      } else {
        // lanes per element: the power of two that covers a small element,
        // else the one of 16 / 32 / 64 that leaves the fewest lanes idle in
        // the last round (32 at n^ndim = 81: 81 of 96 against 81 of 128)
        int lpe = 4;
        while (lpe < V->nloc && lpe < 64) lpe *= 2;
        if (V->nloc > 64)
          for (int cand = 32; cand >= 16; cand /= 2) {
            const int rounds_c = (V->nloc + cand - 1) / cand, rounds_l = (V->nloc + lpe - 1) / lpe;
            if (rounds_c * cand < rounds_l * lpe) lpe = cand;
          }
        k_vol_integrate<<<dim3(blocks_for(E, VOL_BLOCK / lpe), (unsigned)nc), VOL_BLOCK, 0,
                          S(stream)>>>(E, V->nloc, lpe, V->d_wdet, V->d_e2n, cs, ns, uc, local,
                                       buf);
      }
      HIP_TRY(hipGetLastError());
    }
    if (d_total) {
      k_vol_total<<<(unsigned)(nc * nq), VOL_TOTAL_BLOCK, 0, S(stream)>>>(
          E, nq, buf, d_total + (int64_t)c0 * nq);
      HIP_TRY(hipGetLastError());
    }
  }
  return SEM_OK;
}

}  // namespace

extern "C" {

int sem_volume_create(sem_volume** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                      const uint32_t* d_e2n, int64_t n_node, const double* h_D, const double* h_w,
                      int device, void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_volume_create: out is NULL");
  *out = nullptr;
  int rc = semvolume::check_sizes(ndim, p, n_elem, n_node);
  if (rc != SEM_OK) return rc;
  if (!h_D || !h_w || (n_elem > 0 && (!d_x_phys || !d_e2n)))
    return fail(SEM_E_INVALID, "sem_volume_create: NULL array");
  if (device < 0) return fail(SEM_E_INVALID, "sem_volume_create: device must be >= 0");
  Guard guard(device);
  hipStream_t st = S(stream);
  sem_volume* V = new sem_volume();
  V->ndim = ndim;
  V->p = p;
  const int n = V->n = p + 1;
  V->nloc = ndim == 2 ? n * n : n * n * n;
  V->device = device;
  V->n_elem = n_elem;
  V->n_node = n_node;
  V->d_x_phys = d_x_phys;
  V->d_e2n = d_e2n;
#define VOLUME_TRY(expr)                                                             \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      sem_volume_destroy(V);                                                         \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
  // the map comes to the host: every id is checked before any launch
  const size_t ent = (size_t)n_elem * V->nloc;
  std::vector<uint32_t> h_map(ent);
  if (n_elem > 0)
    VOLUME_TRY(hipMemcpyAsync(h_map.data(), d_e2n, ent * sizeof(uint32_t), hipMemcpyDeviceToHost,
                              st));
  VOLUME_TRY(hipStreamSynchronize(st));
  rc = semvolume::check_map(h_map.data(), (int64_t)ent, n_node);
  if (rc != SEM_OK) {
    sem_volume_destroy(V);
    return rc;
  }
  semvolume::Plan pl;
  semvolume::plan((int64_t)ent, h_map.data(), n_node, pl);
  V->n_referenced = pl.n_referenced;
  V->max_row = pl.max_row;
  // the recovery's scratch, one component: [n_elem][ndim][nloc].  At create it
  // holds the per-element counts [n_elem] and their sum
  V->scratch_doubles = std::max<size_t>(ent * ndim, 4);
  VOLUME_TRY(hipMalloc(&V->d_ptr, pl.ptr.size() * sizeof(int32_t)));
  VOLUME_TRY(hipMalloc(&V->d_entry, std::max<size_t>(ent, 1) * sizeof(int32_t)));
  VOLUME_TRY(hipMalloc(&V->d_D, (size_t)n * n * sizeof(double)));
  VOLUME_TRY(hipMalloc(&V->d_w, (size_t)n * sizeof(double)));
  VOLUME_TRY(hipMalloc(&V->d_m, std::max<size_t>((size_t)n_node, 1) * sizeof(double)));
  VOLUME_TRY(hipMalloc(&V->d_wdet, std::max<size_t>(ent, 1) * sizeof(double)));
  VOLUME_TRY(hipMalloc(&V->d_scratch, V->scratch_doubles * sizeof(double)));
  VOLUME_TRY(hipMemcpyAsync(V->d_ptr, pl.ptr.data(), pl.ptr.size() * sizeof(int32_t),
                            hipMemcpyHostToDevice, st));
  VOLUME_TRY(hipMemcpyAsync(V->d_entry, pl.entry.data(), ent * sizeof(int32_t),
                            hipMemcpyHostToDevice, st));
  VOLUME_TRY(hipMemcpyAsync(V->d_D, h_D, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice,
                            st));
  VOLUME_TRY(hipMemcpyAsync(V->d_w, h_w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  double bad = 0.0;
  if (n_elem > 0) {
    // the scratch has at least 8 * n_elem doubles: the counts and their sum fit
    double* counts = V->d_scratch;
    double* total = counts + n_elem;
    launch_elem<M_DETJ>(V, 1, 0, 1, nullptr, nullptr, V->d_wdet, counts, st);
    VOLUME_TRY(hipGetLastError());
    k_vol_total<<<1, VOL_TOTAL_BLOCK, 0, st>>>(n_elem, 1, counts, total);
    VOLUME_TRY(hipGetLastError());
    VOLUME_TRY(hipMemcpyAsync(&bad, total, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (n_node > 0) {
    k_vol_mass<<<blocks_for(n_node, VOL_BLOCK), VOL_BLOCK, 0, st>>>(n_node, V->d_ptr, V->d_entry,
                                                                    V->d_wdet, V->d_m);
    VOLUME_TRY(hipGetLastError());
  }
  VOLUME_TRY(hipStreamSynchronize(st));  // the host tables and h_D / h_w are free again
#undef VOLUME_TRY
  if (bad > 0.0) {
    sem_volume_destroy(V);
    return fail(SEM_E_DETJ, "sem_volume_create: detJ <= 0 at " + std::to_string((int64_t)bad) +
                                " element nodes");
  }
  *out = V;
  return SEM_OK;
}

void sem_volume_destroy(sem_volume* V) {
  if (!V) return;
  {
    Guard guard(V->device);
    (void)hipFree(V->d_ptr);
    (void)hipFree(V->d_entry);
    (void)hipFree(V->d_D);
    (void)hipFree(V->d_w);
    (void)hipFree(V->d_m);
    (void)hipFree(V->d_wdet);
    (void)hipFree(V->d_scratch);
  }
  delete V;
}

int sem_volume_mass(sem_volume* V, double* d_m, void* stream) {
  if (!V || !d_m) return fail(SEM_E_INVALID, "sem_volume_mass: NULL argument");
  if (V->n_node == 0) return SEM_OK;
  Guard guard(V->device);
  HIP_TRY(hipMemcpyAsync(d_m, V->d_m, (size_t)V->n_node * sizeof(double),
                         hipMemcpyDeviceToDevice, S(stream)));
  return SEM_OK;
}

int sem_volume_gradient(sem_volume* V, int ncomp, int64_t comp_stride, int64_t node_stride,
                        const double* d_u, double* d_grad, void* stream) {
  int rc = check_fields(V, "sem_volume_gradient", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (V->n_elem == 0) return SEM_OK;
  if (!d_u || !d_grad) return fail(SEM_E_INVALID, "sem_volume_gradient: NULL array");
  Guard guard(V->device);
  launch_elem<M_GRAD>(V, ncomp, comp_stride, node_stride, d_u, nullptr, d_grad, nullptr,
                      S(stream));
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_volume_recover(sem_volume* V, int ncomp, int64_t comp_stride, int64_t node_stride,
                       const double* d_u, int64_t out_comp_stride, int64_t out_dim_stride,
                       int64_t out_node_stride, double* d_g, void* stream) {
  int rc = check_fields(V, "sem_volume_recover", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (out_comp_stride < 0 || out_dim_stride < 0 || out_node_stride < 1)
    return fail(SEM_E_INVALID, "sem_volume_recover: output strides >= 0, node stride >= 1");
  if (V->n_node == 0) return SEM_OK;
  if (!d_g || (V->n_elem > 0 && !d_u)) return fail(SEM_E_INVALID, "sem_volume_recover: NULL array");
  Guard guard(V->device);
  // the scratch holds one component
  for (int c = 0; c < ncomp; ++c) {
    if (V->n_elem > 0) {
      launch_elem<M_RECOVER>(V, 1, comp_stride, node_stride, d_u + c * comp_stride, nullptr,
                             V->d_scratch, nullptr, S(stream));
      HIP_TRY(hipGetLastError());
    }
    k_vol_nodes<<<dim3(blocks_for(V->n_node, VOL_BLOCK), (unsigned)V->ndim), VOL_BLOCK, 0,
                  S(stream)>>>(V->n_node, V->ndim, V->nloc, V->d_ptr, V->d_entry, V->d_scratch,
                               V->d_m, out_dim_stride, out_node_stride, d_g + c * out_comp_stride);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int sem_volume_integrate(sem_volume* V, int ncomp, int64_t comp_stride, int64_t node_stride,
                         const double* d_u, double* d_per_elem, double* d_total, void* stream) {
  int rc = check_fields(V, "sem_volume_integrate", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (V->n_elem > 0 && !d_u) return fail(SEM_E_INVALID, "sem_volume_integrate: d_u is NULL");
  return reduce_fields(V, 1, ncomp, comp_stride, node_stride, d_u, nullptr, 0, d_per_elem,
                       d_total, stream);
}

int sem_volume_integrate_local(sem_volume* V, int ncomp, const double* d_vals, double* d_per_elem,
                               double* d_total, void* stream) {
  int rc = check_fields(V, "sem_volume_integrate_local", ncomp, 0, 1);
  if (rc != SEM_OK) return rc;
  if (V->n_elem > 0 && !d_vals)
    return fail(SEM_E_INVALID, "sem_volume_integrate_local: d_vals is NULL");
  return reduce_fields(V, 1, ncomp, 0, 1, d_vals, nullptr, 1, d_per_elem, d_total, stream);
}

int sem_volume_norms(sem_volume* V, int ncomp, int64_t comp_stride, int64_t node_stride,
                     const double* d_u, const double* d_v, double* d_per_elem, double* d_total,
                     void* stream) {
  int rc = check_fields(V, "sem_volume_norms", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (V->n_elem > 0 && !d_u) return fail(SEM_E_INVALID, "sem_volume_norms: d_u is NULL");
  return reduce_fields(V, 2, ncomp, comp_stride, node_stride, d_u, d_v, 0, d_per_elem, d_total,
                       stream);
}

int sem_volume_info(sem_volume* V, int64_t* info, int n_info) {
  if (!V || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_volume_info: NULL argument");
  const int64_t v[7] = {V->ndim,         V->p,       V->n_elem, V->n_node,
                        V->n_referenced, V->max_row, (int64_t)(V->scratch_doubles * sizeof(double))};
  for (int i = 0; i < std::min(n_info, 7); ++i) info[i] = v[i];
  return SEM_OK;
}

}  // extern "C"
