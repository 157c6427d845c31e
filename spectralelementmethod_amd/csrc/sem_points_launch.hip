// Per-order launch unit of the point kernels: the instantiations of
// k_pts_locate / k_pts_invert / k_pts_map / k_pts_eval for the orders n in
// [SEM_N_LO, SEM_N_HI], both dimensions (the build compiles this file once
// per range, in parallel; spectralelementmethod_amd/_build.py).  The design
// is described at the top of sem_points.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>

#include "sem_points.h"

#ifndef SEM_N_LO
#define SEM_N_LO 2
#endif
#ifndef SEM_N_HI
#define SEM_N_HI 17
#endif

namespace semp {
namespace {

// ---------------------------------------------------------------- basis
// l_j(x) and l_j'(x), j < N, of the GLL Lagrange basis in barycentric form,
// written to a strided column (stride in doubles).  At x exactly on a node
// the values are the Kronecker delta and the derivatives that row of the
// differentiation matrix: no 0/0 is formed.
template <int N>
__device__ inline void pts_basis_col(const double* __restrict__ gx, const double* __restrict__ gw,
                                     double x, double* l, double* dl, int stride) {
  int hit = -1;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double d = x - gx[j];
    if (d == 0.0) hit = j;
    const double t = gw[j] / (d == 0.0 ? 1.0 : d);
    l[j * stride] = t;
    s += t;
  }
  if (hit < 0) {
    const double inv = 1.0 / s;
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double lj = l[j * stride] * inv;
      l[j * stride] = lj;
      a += lj / (x - gx[j]);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) dl[j * stride] = l[j * stride] * (a - 1.0 / (x - gx[j]));
  } else {
    const double xh = gx[hit], wh = gw[hit];
    double diag = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double d = (j == hit) ? 0.0 : (gw[j] / wh) / (xh - gx[j]);
      l[j * stride] = (j == hit) ? 1.0 : 0.0;
      dl[j * stride] = d;
      diag -= d;
    }
    dl[hit * stride] = diag;
  }
}

// values only, into registers
template <int N>
__device__ inline void pts_basis_reg(const double* __restrict__ gx, const double* __restrict__ gw,
                                     double x, double (&l)[N]) {
  int hit = -1;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double d = x - gx[j];
    if (d == 0.0) hit = j;
    const double t = gw[j] / (d == 0.0 ? 1.0 : d);
    l[j] = t;
    s += t;
  }
  const double inv = 1.0 / s;
#pragma unroll
  for (int j = 0; j < N; ++j) l[j] = hit < 0 ? l[j] * inv : (j == hit ? 1.0 : 0.0);
}

// x(xi) and J[c][d] = d x_c / d xi_d in one element; sb = this lane's LDS
// columns [2 * ND][N] (values of dimension d at 2 d, derivatives at 2 d + 1)
template <int ND, int N>
__device__ inline void pts_map(const double* __restrict__ xe, const double* sb, double (&xo)[ND],
                               double (&J)[ND][ND]) {
  constexpr int NLOC = ipow(N, ND);
  constexpr int L = PTS_LANES;
  const double* lz = sb + (2 * (ND - 1)) * N * L;
  const double* dz = sb + (2 * (ND - 1) + 1) * N * L;
  double z[N], zd[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    z[k] = lz[k * L];
    zd[k] = dz[k * L];
  }
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    const double* xc = xe + c * NLOC;
    double v = 0.0, g[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) g[d] = 0.0;
    if constexpr (ND == 2) {
#pragma unroll 1
      for (int i = 0; i < N; ++i) {
        double s = 0.0, sd = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double cv = xc[i * N + k];
          s += cv * z[k];
          sd += cv * zd[k];
        }
        const double li = sb[(0 * N + i) * L], di = sb[(1 * N + i) * L];
        v += li * s;
        g[0] += di * s;
        g[1] += li * sd;
      }
    } else {
#pragma unroll 1
      for (int i = 0; i < N; ++i) {
        const double li = sb[(0 * N + i) * L], di = sb[(1 * N + i) * L];
        double t = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll 1
        for (int j = 0; j < N; ++j) {
          double s = 0.0, sd = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double cv = xc[(i * N + j) * N + k];
            s += cv * z[k];
            sd += cv * zd[k];
          }
          const double lj = sb[(2 * N + j) * L], dj = sb[(3 * N + j) * L];
          t += lj * s;
          t1 += dj * s;
          t2 += lj * sd;
        }
        v += li * t;
        g[0] += di * t;
        g[1] += li * t1;
        g[2] += li * t2;
      }
    }
    xo[c] = v;
#pragma unroll
    for (int d = 0; d < ND; ++d) J[c][d] = g[d];
  }
}

template <int ND, int N>
__device__ inline void pts_set_basis(const double* __restrict__ gb, const double (&xi)[ND],
                                     double* sb) {
#pragma unroll
  for (int d = 0; d < ND; ++d)
    pts_basis_col<N>(gb, gb + N, xi[d], sb + (2 * d) * N * PTS_LANES,
                     sb + (2 * d + 1) * N * PTS_LANES, PTS_LANES);
}

// dx = J^-1 r, closed form; false when J is singular or dx is not finite
template <int ND>
__device__ inline bool pts_solve(const double (&J)[ND][ND], const double (&r)[ND],
                                 double (&dx)[ND]) {
  if constexpr (ND == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    dx[0] = (J[1][1] * r[0] - J[0][1] * r[1]) * inv;
    dx[1] = (J[0][0] * r[1] - J[1][0] * r[0]) * inv;
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
    const double c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
    const double c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    const double c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    const double c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    dx[0] = (c00 * r[0] + c10 * r[1] + c20 * r[2]) * inv;
    dx[1] = (c01 * r[0] + c11 * r[1] + c21 * r[2]) * inv;
    dx[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) * inv;
  }
  bool ok = true;
#pragma unroll
  for (int d = 0; d < ND; ++d) ok = ok && isfinite(dx[d]);
  return ok;
}

// the reference's Newton (sem/rootfind.py:22-53 as called at
// sem/mapping.py:171) in one element: true when |dx|_2 <= tol was met within
// the iteration cap; a singular Jacobian or a non-finite iterate ends it
template <int ND, int N>
__device__ inline bool pts_newton(const double* __restrict__ xe, const double* __restrict__ gb,
                                  const double (&xq)[ND], double (&xi)[ND], double* sb) {
#pragma unroll 1
  for (int it = 0; it < PTS_NEWTON_ITMAX; ++it) {
    pts_set_basis<ND, N>(gb, xi, sb);
    double x[ND], J[ND][ND], r[ND], dx[ND];
    pts_map<ND, N>(xe, sb, x, J);
    double nrm = 0.0;
#pragma unroll
    for (int d = 0; d < ND; ++d) r[d] = xq[d] - x[d];
    if (!pts_solve<ND>(J, r, dx)) return false;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      xi[d] += dx[d];
      nrm += dx[d] * dx[d];
    }
    if (sqrt(nrm) <= PTS_NEWTON_TOL) return true;
  }
  return false;
}

template <int ND>
__device__ inline bool pts_inside(double (&xi)[ND]) {
  bool in = true;
#pragma unroll
  for (int d = 0; d < ND; ++d) in = in && fabs(xi[d]) <= 1.0 + SEM_POINTS_XI_SLACK;
  if (in) {
#pragma unroll
    for (int d = 0; d < ND; ++d) xi[d] = fmin(1.0, fmax(-1.0, xi[d]));
  }
  return in;
}


template <int ND, int N>
__global__ void __launch_bounds__(PTS_LANES)
    k_pts_locate(int64_t n_pts, int64_t n_elem, const double* __restrict__ xphys,
                 const double* __restrict__ gb, const double* __restrict__ box,
                 const double* __restrict__ cen, const int32_t* __restrict__ cell_ptr,
                 const int32_t* __restrict__ cell_elem, PtsGrid grid,
                 const double* __restrict__ xq_in, int32_t* __restrict__ elem_out,
                 double* __restrict__ xi_out, unsigned long long* __restrict__ n_outside) {
  constexpr int NLOC = ipow(N, ND);
  __shared__ double s_basis[2 * ND * N * PTS_LANES];
  double* sb = s_basis + threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)PTS_LANES + threadIdx.x;
  if (i >= n_pts) return;
  double xq[ND];
  bool in_grid = true;
  int64_t cell = 0;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    xq[d] = xq_in[d * n_pts + i];
    const double f = (xq[d] - grid.lo[d]) * grid.inv_h[d];
    // a point on the upper face of the grid belongs to the last cell; a NaN
    // or a point off the grid has no cell
    const double gd = (double)grid.g[d];
    if (!(f >= 0.0 && f <= gd)) in_grid = false;
    const int k = min((int)floor(in_grid ? f : 0.0), grid.g[d] - 1);
    cell = cell * grid.g[d] + k;
  }
  int32_t found = -1;
  double xi[ND];
  if (in_grid) {
    const int32_t c0 = cell_ptr[cell], c1 = cell_ptr[cell + 1];
    // candidates in ascending (centroid distance, element id): select the
    // next one after (d_prev, e_prev) each round -- at most c1 - c0 rounds
    double d_prev = -1.0;
    int32_t e_prev = -1;
#pragma unroll 1
    for (int32_t round = c0; round < c1 && found < 0; ++round) {
      double d_best = std::numeric_limits<double>::infinity();
      int32_t e_best = -1;
#pragma unroll 1
      for (int32_t k = c0; k < c1; ++k) {
        const int32_t e = cell_elem[k];
        bool inb = true;
        double dist = 0.0;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          inb = inb && xq[d] >= box[(int64_t)e * 2 * ND + d] &&
                xq[d] <= box[(int64_t)e * 2 * ND + ND + d];
          const double t = xq[d] - cen[(int64_t)e * ND + d];
          dist += t * t;
        }
        if (!inb) continue;
        const bool after = dist > d_prev || (dist == d_prev && e > e_prev);
        const bool better = dist < d_best || (dist == d_best && e < e_best);
        if (after && better) {
          d_best = dist;
          e_best = e;
        }
      }
      if (e_best < 0) break;
      d_prev = d_best;
      e_prev = e_best;
#pragma unroll
      for (int d = 0; d < ND; ++d) xi[d] = 0.0;
      if (pts_newton<ND, N>(xphys + (int64_t)e_best * ND * NLOC, gb, xq, xi, sb) &&
          pts_inside<ND>(xi))
        found = e_best;
    }
  }
  elem_out[i] = found;
#pragma unroll
  for (int d = 0; d < ND; ++d)
    xi_out[d * n_pts + i] = found >= 0 ? xi[d] : std::numeric_limits<double>::quiet_NaN();
  if (found < 0) atomicAdd(n_outside, 1ull);
}

template <int ND, int N>
__global__ void __launch_bounds__(PTS_LANES)
    k_pts_invert(int64_t n_pts, int64_t n_elem, const double* __restrict__ xphys,
                 const double* __restrict__ gb, const double* __restrict__ xq_in,
                 const int32_t* __restrict__ elem_in, const double* __restrict__ guess,
                 double* __restrict__ xi_out, uint8_t* __restrict__ status) {
  constexpr int NLOC = ipow(N, ND);
  __shared__ double s_basis[2 * ND * N * PTS_LANES];
  double* sb = s_basis + threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)PTS_LANES + threadIdx.x;
  if (i >= n_pts) return;
  const int32_t e = elem_in[i];
  double xq[ND], xi[ND];
  uint8_t st = 2;
  bool ok = e >= 0 && (int64_t)e < n_elem;
  if (ok) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      xq[d] = xq_in[d * n_pts + i];
      xi[d] = guess ? guess[d * n_pts + i] : 0.0;
    }
    ok = pts_newton<ND, N>(xphys + (int64_t)e * ND * NLOC, gb, xq, xi, sb);
    if (ok) st = pts_inside<ND>(xi) ? 0 : 1;
  }
#pragma unroll
  for (int d = 0; d < ND; ++d)
    xi_out[d * n_pts + i] = ok ? xi[d] : std::numeric_limits<double>::quiet_NaN();
  if (status) status[i] = st;
}

template <int ND, int N>
__global__ void __launch_bounds__(PTS_LANES)
    k_pts_map(int64_t n_pts, int64_t n_elem, const double* __restrict__ xphys,
              const double* __restrict__ gb, const int32_t* __restrict__ elem_in,
              const double* __restrict__ xi_in, double* __restrict__ x_out) {
  constexpr int NLOC = ipow(N, ND);
  __shared__ double s_basis[2 * ND * N * PTS_LANES];
  double* sb = s_basis + threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)PTS_LANES + threadIdx.x;
  if (i >= n_pts) return;
  const int32_t e = elem_in[i];
  double x[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) x[d] = std::numeric_limits<double>::quiet_NaN();
  if (e >= 0 && (int64_t)e < n_elem) {
    double xi[ND], J[ND][ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) xi[d] = xi_in[d * n_pts + i];
    pts_set_basis<ND, N>(gb, xi, sb);
    pts_map<ND, N>(xphys + (int64_t)e * ND * NLOC, sb, x, J);
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) x_out[d * n_pts + i] = x[d];
}

// ---------------------------------------------------------------- evaluation
template <int ND, int N, int W>
__global__ void __launch_bounds__(PTS_BLOCK)
    k_pts_eval(const PtsItem* __restrict__ items, int64_t n_items,
               const int32_t* __restrict__ perm, const uint32_t* __restrict__ e2n,
               const double* __restrict__ xi, int64_t n_pts, int ncomp, int64_t comp_stride,
               int64_t node_stride, const double* __restrict__ u, double* __restrict__ out,
               const double* __restrict__ gb) {
  constexpr int G = PTS_BLOCK / W;      // items per workgroup
  constexpr int SLAB = N * N;           // coefficients staged at a time
  constexpr int NSLAB = ND == 3 ? N : 1;
  constexpr int NLOC = SLAB * NSLAB;
  constexpr int STRIDE = SLAB | 1;      // odd: the items' slabs start on different banks
  __shared__ double s_c[G * STRIDE];
  const int g = threadIdx.x / W, s = threadIdx.x % W;
  const int64_t it = blockIdx.x * (int64_t)G + g;
  const bool have = it < n_items;
  PtsItem item = {0, 0, 0};
  if (have) item = items[it];
  const int64_t pt = (have && s < item.count) ? perm[item.start + s] : -1;
  // lanes without a point run the same arithmetic at xi = 0 (uniform control
  // flow around the barriers); only the final store is guarded
  double la[N], lb[N];
  pts_basis_reg<N>(gb, gb + N, pt >= 0 ? xi[(ND - 2) * n_pts + pt] : 0.0, la);
  pts_basis_reg<N>(gb, gb + N, pt >= 0 ? xi[(ND - 1) * n_pts + pt] : 0.0, lb);
  double x0 = 0.0, inv0 = 0.0;
  int hit0 = -1;
  if constexpr (ND == 3) {
    // l_i(xi0) is rebuilt per plane from (x0, hit0, inv0): no register array
    // is indexed by the rolled plane loop
    x0 = pt >= 0 ? xi[pt] : 0.0;
    double sum = 0.0;
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      const double d = x0 - gb[j];
      if (d == 0.0) hit0 = j;
      sum += gb[N + j] / (d == 0.0 ? 1.0 : d);
    }
    inv0 = 1.0 / sum;
  }
  double* sc = s_c + g * STRIDE;
  const uint32_t* map = e2n + (int64_t)item.elem * NLOC;
#pragma unroll 1
  for (int c = 0; c < ncomp; ++c) {
    const double* uc = u + c * comp_stride;
    double acc = 0.0;
#pragma unroll 1
    for (int sl = 0; sl < NSLAB; ++sl) {
      __syncthreads();
      if (have)
        for (int k = s; k < SLAB; k += W) sc[k] = uc[(int64_t)map[sl * SLAB + k] * node_stride];
      __syncthreads();
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) r += lb[k] * sc[j * N + k];
        t += la[j] * r;
        // finish a row before the next row's LDS reads issue: the scheduler
        // otherwise clusters all n^2 reads first, two registers each
        asm volatile("" : "+v"(t) : : "memory");
      }
      if constexpr (ND == 3) {
        const double d0 = x0 - gb[sl];
        const double l0 = hit0 >= 0 ? (sl == hit0 ? 1.0 : 0.0)
                                    : gb[N + sl] / (d0 == 0.0 ? 1.0 : d0) * inv0;
        acc += l0 * t;
      } else {
        acc = t;
      }
    }
    if (pt >= 0) out[c * n_pts + pt] = acc;
  }
}

}  // namespace

template <int ND, int N>
int pts_launch(const PtsCall& c) {
  const sem_points* P = c.P;
  const dim3 b(PTS_LANES), g(blocks_for(c.n_pts, PTS_LANES));
  switch (c.op) {
    case PTS_LOCATE:
      hipLaunchKernelGGL((k_pts_locate<ND, N>), g, b, 0, c.st, c.n_pts, P->n_elem, P->d_x,
                         P->d_basis, P->d_box, P->d_cen, P->d_cell_ptr, P->d_cell_elem, c.grid,
                         c.xq, c.elem_out, c.xi_out, P->d_count);
      break;
    case PTS_INVERT:
      hipLaunchKernelGGL((k_pts_invert<ND, N>), g, b, 0, c.st, c.n_pts, P->n_elem, P->d_x,
                         P->d_basis, c.xq, c.elem_in, c.xi_in, c.xi_out, c.status);
      break;
    case PTS_MAP:
      hipLaunchKernelGGL((k_pts_map<ND, N>), g, b, 0, c.st, c.n_pts, P->n_elem, P->d_x,
                         P->d_basis, c.elem_in, c.xi_in, c.x_out);
      break;
    case PTS_EVAL: {
      const sem_pplan* L = c.L;
      if (L->width == 16)
        hipLaunchKernelGGL((k_pts_eval<ND, N, 16>), dim3(blocks_for(L->n_items, PTS_BLOCK / 16)),
                           dim3(PTS_BLOCK), 0, c.st, L->d_items, L->n_items, L->d_perm, c.e2n,
                           c.xi_in, L->n_pts, c.ncomp, c.comp_stride, c.node_stride, c.u, c.out,
                           P->d_basis);
      else
        hipLaunchKernelGGL((k_pts_eval<ND, N, 64>), dim3(blocks_for(L->n_items, PTS_BLOCK / 64)),
                           dim3(PTS_BLOCK), 0, c.st, L->d_items, L->n_items, L->d_perm, c.e2n,
                           c.xi_in, L->n_pts, c.ncomp, c.comp_stride, c.node_stride, c.u, c.out,
                           P->d_basis);
      break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return sem::fail(SEM_E_HIP, std::string("points launch: ") + hipGetErrorString(e));
  return SEM_OK;
}

#define SEM_PTS_INSTANTIATE(N)                      \
  template int pts_launch<2, N>(const PtsCall&);    \
  template int pts_launch<3, N>(const PtsCall&);

#if SEM_N_LO <= 2 && 2 <= SEM_N_HI
SEM_PTS_INSTANTIATE(2)
#endif
#if SEM_N_LO <= 3 && 3 <= SEM_N_HI
SEM_PTS_INSTANTIATE(3)
#endif
#if SEM_N_LO <= 4 && 4 <= SEM_N_HI
SEM_PTS_INSTANTIATE(4)
#endif
#if SEM_N_LO <= 5 && 5 <= SEM_N_HI
SEM_PTS_INSTANTIATE(5)
#endif
#if SEM_N_LO <= 6 && 6 <= SEM_N_HI
SEM_PTS_INSTANTIATE(6)
#endif
#if SEM_N_LO <= 7 && 7 <= SEM_N_HI
SEM_PTS_INSTANTIATE(7)
#endif
#if SEM_N_LO <= 8 && 8 <= SEM_N_HI
SEM_PTS_INSTANTIATE(8)
#endif
#if SEM_N_LO <= 9 && 9 <= SEM_N_HI
SEM_PTS_INSTANTIATE(9)
#endif
#if SEM_N_LO <= 10 && 10 <= SEM_N_HI
SEM_PTS_INSTANTIATE(10)
#endif
#if SEM_N_LO <= 11 && 11 <= SEM_N_HI
SEM_PTS_INSTANTIATE(11)
#endif
#if SEM_N_LO <= 12 && 12 <= SEM_N_HI
SEM_PTS_INSTANTIATE(12)
#endif
#if SEM_N_LO <= 13 && 13 <= SEM_N_HI
SEM_PTS_INSTANTIATE(13)
#endif
#if SEM_N_LO <= 14 && 14 <= SEM_N_HI
SEM_PTS_INSTANTIATE(14)
#endif
#if SEM_N_LO <= 15 && 15 <= SEM_N_HI
SEM_PTS_INSTANTIATE(15)
#endif
#if SEM_N_LO <= 16 && 16 <= SEM_N_HI
SEM_PTS_INSTANTIATE(16)
#endif
#if SEM_N_LO <= 17 && 17 <= SEM_N_HI
SEM_PTS_INSTANTIATE(17)
#endif

}  // namespace semp
