// Dense element matrices (include/sem_hip.h, "Element matrices"): the local
// systems the reference builds per element in Python (examples/poisson.py:
// 166-193, examples/squirmer-axisymmetric.py:259-297) written by one launch
// for a range of elements, in any local DOF order.
//
// Self-contained like the points and faces units: x_phys is borrowed in the
// layout sem_geom_fields writes, the per-node factors are derived here the
// way k_geom derives the stored ones (sem_kernels.h: J from coordinates
// relative to the element's node (0, 0), det_inv_2x2, W = det w_m w_n,
// rho = x), so W / rho at rho = 0 is formed and propagates exactly as there.
//
// The output is the traffic: n^4 dpn^2 doubles per element, of which only the
// ~2 n^3 entries with q == s or p == r carry an O(n) sum.  One workgroup of
// 256 lanes takes one element at a time (grid-stride):
//   - D, w and the local order arrive as kernel arguments (no device copy, no
//     allocation: the call is graph-capturable) and are staged in LDS once;
//   - per element, x_phys and the gathered state are staged, each lane derives
//     the factors and the pointwise coefficients of its nodes into LDS, and
//     (where they fit in 64 KB) the two O(n) sums of every (q, p, r) / (p, q, s)
//     are tabulated: T1[q][p][r] = sum_m G00[m,q] D[m,p] D[m,r],
//     T4[p][q][s] = sum_k G11[p,k] D[k,q] D[k,s];
//   - the element's nl x nl block is contiguous, so the lanes walk its linear
//     index: a wavefront stores 64 consecutive doubles (consecutive columns of
//     a row, running on into the next row), the lexicographic (p, q, comp) of
//     row and column read from the order table in LDS.  Plain vector stores,
//     non-temporal.
//
// Entry (row (p, q, ca), column (r, s, cb)), K_G the stiffness block of the
// factors G (the four terms of sem_hip.h):
//   S K_G + [q == s] c0 D[p][r] + [p == r] c1 D[q][s] + [p == r, q == s] c2
// with (S; c0, c1, c2) at the row node:
//   Poisson          1; 0, 0, 0
//   (omega, psi)     0; a0, a1, 0            (Navier-Stokes only)
//   (omega, omega)   1; a2, a3, W/rho + a4   Lve (+ d(Ae omega psi)/d omega)
//   (psi, psi)       1; 2W iJ00, 2W iJ10, 0  E2e
//   (psi, omega)     0; 0, 0, -rho^2 W       -Me
// a0..a4: the linearisation coefficients of sem_kernels.h (axisym_group).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "sem_internal.h"

using sem::fail;

namespace {

constexpr int ELMAT_BLOCK = 256;
constexpr int ELMAT_MAX_GRID = 2048;  // 8 workgroups on each of 256 CUs
constexpr size_t ELMAT_LDS_LIMIT = 64 * 1024;

// D, w and the local order travel in the kernel argument segment
struct ElmatBasis {
  double D[SEM_MAXN * SEM_MAXN];
  double w[SEM_MAXN];
  uint16_t ord[2 * SEM_MAXN * SEM_MAXN];
};
static_assert(sizeof(ElmatBasis) <= 3700, "kernel arguments stay well below 4 KB");

struct ElmatArgs {
  int n, kind, tab;
  double re;
  const double* x_phys;
  const uint32_t* e2n;
  const double* state;
  int64_t elem_begin, elem_count;
  double* mat;
  double* rhs;
};

// per-node arrays of n^2 doubles in LDS, in this order
enum { A_D = 0, A_G00, A_G01, A_G11, A_POISSON_END };
enum { A_A0 = A_POISSON_END, A_A1, A_B0, A_B1, A_B2, A_E0, A_E1, A_M, A_AXI_END };
// scratch arrays (overlaid by the tables once the factors are known)
enum { S_X0 = 0, S_X1, S_U0, S_U1, S_D0A, S_D1A, S_D0B, S_D1B, S_W0A, S_W1A, S_W0B, S_W1B, S_END };

__host__ __device__ inline size_t elmat_doubles(int dpn, int n, bool tab) {
  const size_t n2 = (size_t)n * n;
  const size_t fixed = (dpn == 1 ? A_POISSON_END : A_AXI_END) * n2;
  const size_t scratch = (size_t)S_END * n2, tables = tab ? 2 * n2 * n : 0;
  return fixed + (scratch > tables ? scratch : tables);
}

inline size_t elmat_lds(int dpn, int n, bool tab) {
  // doubles, then the packed order table (uint32 per local DOF)
  return elmat_doubles(dpn, n, tab) * sizeof(double) + (size_t)dpn * n * n * sizeof(uint32_t);
}

template <int DPN>
__global__ void __launch_bounds__(ELMAT_BLOCK)
    k_elem_matrices(const ElmatBasis B, const ElmatArgs P) {
  extern __shared__ double lds[];
  const int n = P.n, n2 = n * n, nl = DPN * n2;
  const int tid = threadIdx.x;
  constexpr int NFIX = DPN == 1 ? A_POISSON_END : A_AXI_END;
  double* sD = lds + A_D * n2;
  double* sG00 = lds + A_G00 * n2;
  double* sG01 = lds + A_G01 * n2;
  double* sG11 = lds + A_G11 * n2;
  double* sc = lds + NFIX * n2;  // scratch / tables
  double* sT1 = sc;
  double* sT4 = sc + n2 * n;
  uint32_t* sOrd = reinterpret_cast<uint32_t*>(lds + elmat_doubles(DPN, n, P.tab != 0));
  const bool has_state = P.state != nullptr;
  const bool ns = P.kind == SEM_OP_AXISYM_NS;

  for (int i = tid; i < n2; i += ELMAT_BLOCK) sD[i] = B.D[i];
  // row / column a of the output is local DOF ord[a]: node | p << 10 | q << 15 | comp << 20
  for (int a = tid; a < nl; a += ELMAT_BLOCK) {
    const int l = B.ord[a];
    const int node = l / DPN, c = l - node * DPN;
    const int p = node / n, q = node - p * n;
    sOrd[a] = (uint32_t)node | (uint32_t)p << 10 | (uint32_t)q << 15 | (uint32_t)c << 20;
  }

  for (int64_t eo = blockIdx.x; eo < P.elem_count; eo += gridDim.x) {
    const int64_t e = P.elem_begin + eo;
    __syncthreads();  // the previous element's tables are no longer read
    for (int i = tid; i < n2; i += ELMAT_BLOCK) {
      sc[S_X0 * n2 + i] = P.x_phys[(e * 2 + 0) * n2 + i];
      sc[S_X1 * n2 + i] = P.x_phys[(e * 2 + 1) * n2 + i];
      if (has_state) {
        const int64_t g = P.e2n[e * n2 + i];
        if (DPN == 1) {
          sc[S_U0 * n2 + i] = P.state[g];
        } else {
          sc[S_U0 * n2 + i] = P.state[2 * g];      // psi
          sc[S_U1 * n2 + i] = P.state[2 * g + 1];  // omega
        }
      }
    }
    __syncthreads();
    const double x00 = sc[S_X0 * n2], x10 = sc[S_X1 * n2];
    for (int i = tid; i < n2; i += ELMAT_BLOCK) {
      const int m = i / n, k = i - m * n;
      // J[c][d] = d x_c / d xi_d on coordinates relative to node (0, 0)
      double J00 = 0.0, J01 = 0.0, J10 = 0.0, J11 = 0.0;
      double d0a = 0.0, d1a = 0.0, d0b = 0.0, d1b = 0.0;
      for (int r = 0; r < n; ++r) {
        const double dm = sD[m * n + r], dk = sD[k * n + r];
        J00 = fma(dm, sc[S_X0 * n2 + r * n + k] - x00, J00);
        J01 = fma(dk, sc[S_X0 * n2 + m * n + r] - x00, J01);
        J10 = fma(dm, sc[S_X1 * n2 + r * n + k] - x10, J10);
        J11 = fma(dk, sc[S_X1 * n2 + m * n + r] - x10, J11);
        if (has_state) {
          d0a = fma(dm, sc[S_U0 * n2 + r * n + k], d0a);
          d1a = fma(dk, sc[S_U0 * n2 + m * n + r], d1a);
          if (DPN == 2) {
            d0b = fma(dm, sc[S_U1 * n2 + r * n + k], d0b);
            d1b = fma(dk, sc[S_U1 * n2 + m * n + r], d1b);
          }
        }
      }
      const double det = J00 * J11 - J01 * J10;
      const double rdet = 1.0 / det;
      const double iJ00 = J11 * rdet, iJ01 = -J01 * rdet;
      const double iJ10 = -J10 * rdet, iJ11 = J00 * rdet;
      const double ww = B.w[m] * B.w[k];
      const double W = det * B.w[m] * B.w[k];
      const double A00 = iJ00 * iJ00 + iJ01 * iJ01;
      const double A01 = iJ00 * iJ10 + iJ01 * iJ11;
      const double A11 = iJ10 * iJ10 + iJ11 * iJ11;
      double g00, g01, g11;
      if (DPN == 1) {
        g00 = W * A00;
        g01 = W * A01;
        g11 = W * A11;
      } else {
        const double rho = (sc[S_X0 * n2 + i] - x00) + x00;
        const double rW = rho * W;
        g00 = rW * A00;
        g01 = rW * A01;
        g11 = rW * A11;
        const double f5 = W / rho;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
        if (ns) {
          const double f7 = f5 * iJ01, f8 = f5 * iJ11;
          const double om = sc[S_U1 * n2 + i];
          const double rw = P.re * ww;
          a0 = fma(rw, d1b, P.re * f7 * om);
          a1 = fma(-rw, d0b, P.re * f8 * om);
          a2 = -rw * d1a;
          a3 = rw * d0a;
          a4 = P.re * fma(f7, d0a, f8 * d1a);
        }
        lds[A_A0 * n2 + i] = a0;
        lds[A_A1 * n2 + i] = a1;
        lds[A_B0 * n2 + i] = a2;
        lds[A_B1 * n2 + i] = a3;
        lds[A_B2 * n2 + i] = f5 + a4;
        lds[A_E0 * n2 + i] = 2.0 * W * iJ00;
        lds[A_E1 * n2 + i] = 2.0 * W * iJ10;
        lds[A_M * n2 + i] = -(rW * rho);
      }
      sG00[i] = g00;
      sG01[i] = g01;
      sG11[i] = g11;
      if (P.rhs) {
        sc[S_D0A * n2 + i] = d0a;
        sc[S_D1A * n2 + i] = d1a;
        sc[S_W0A * n2 + i] = fma(g00, d0a, g01 * d1a);
        sc[S_W1A * n2 + i] = fma(g01, d0a, g11 * d1a);
        if (DPN == 2) {
          sc[S_D0B * n2 + i] = d0b;
          sc[S_D1B * n2 + i] = d1b;
          sc[S_W0B * n2 + i] = fma(g00, d0b, g01 * d1b);
          sc[S_W1B * n2 + i] = fma(g01, d0b, g11 * d1b);
        }
      }
    }
    __syncthreads();
    if (P.rhs) {
      // the element-local residual at the state; a lane reads its own node's
      // state slots and overwrites them with the residual
      for (int i = tid; i < n2; i += ELMAT_BLOCK) {
        const int p = i / n, q = i - p * n;
        double sa = 0.0, sb = 0.0;
        for (int m = 0; m < n; ++m) {
          const double dp = sD[m * n + p], dq = sD[m * n + q];
          sa = fma(dp, sc[S_W0A * n2 + m * n + q], fma(dq, sc[S_W1A * n2 + p * n + m], sa));
          if (DPN == 2)
            sb = fma(dp, sc[S_W0B * n2 + m * n + q], fma(dq, sc[S_W1B * n2 + p * n + m], sb));
        }
        if (DPN == 1) {
          sc[S_U0 * n2 + i] = sa;
        } else {
          const double om = sc[S_U1 * n2 + i];
          const double d0p = sc[S_D0A * n2 + i], d1p = sc[S_D1A * n2 + i];
          const double d0o = sc[S_D0B * n2 + i], d1o = sc[S_D1B * n2 + i];
          // omega row: Lve omega + Ae omega psi; psi row: E2e psi - Me omega
          const double y_om = sb + fma(lds[A_B2 * n2 + i], om,
                                       fma(lds[A_B1 * n2 + i], d1o, lds[A_B0 * n2 + i] * d0o));
          const double y_ps = sa + fma(lds[A_E0 * n2 + i], d0p,
                                       fma(lds[A_E1 * n2 + i], d1p, lds[A_M * n2 + i] * om));
          sc[S_U0 * n2 + i] = y_om;  // local DOF 2 node + 0
          sc[S_U1 * n2 + i] = y_ps;  // local DOF 2 node + 1
        }
      }
      __syncthreads();
      double* out = P.rhs + eo * nl;
      for (int a = tid; a < nl; a += ELMAT_BLOCK) {
        const uint32_t o = sOrd[a];
        const int node = o & 1023, c = (o >> 20) & 1;
        __builtin_nontemporal_store(-sc[(c ? S_U1 : S_U0) * n2 + node], out + a);
      }
      __syncthreads();
    }
    if (P.tab) {
      const int n3 = n2 * n;
      for (int i = tid; i < n3; i += ELMAT_BLOCK) {
        const int a = i / n2, rem = i - a * n2;
        const int b = rem / n, c = rem - b * n;
        double t1 = 0.0, t4 = 0.0;
        for (int m = 0; m < n; ++m) {
          t1 = fma(sG00[m * n + a] * sD[m * n + b], sD[m * n + c], t1);
          t4 = fma(sG11[a * n + m] * sD[m * n + b], sD[m * n + c], t4);
        }
        sT1[i] = t1;  // [q][p][r]
        sT4[i] = t4;  // [p][q][s]
      }
      __syncthreads();
    }
    double* out = P.mat + eo * (int64_t)nl * nl;
    const int total = nl * nl;
    int a = tid / nl, b = tid - a * nl;
    const int da = ELMAT_BLOCK / nl, db = ELMAT_BLOCK - da * nl;
    for (int idx = tid; idx < total; idx += ELMAT_BLOCK) {
      const uint32_t oa = sOrd[a], ob = sOrd[b];
      const int na = oa & 1023, p = (oa >> 10) & 31, q = (oa >> 15) & 31;
      const int nb = ob & 1023, r = (ob >> 10) & 31, s = (ob >> 15) & 31;
      const double dpr = sD[p * n + r], dqs = sD[q * n + s];
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
      bool stiff = true;
      if (DPN == 2) {
        const int combo = (int)((oa >> 20) & 1) * 2 + (int)((ob >> 20) & 1);
        if (combo == 0) {  // omega row, psi column
          stiff = false;
          c0 = lds[A_A0 * n2 + na];
          c1 = lds[A_A1 * n2 + na];
        } else if (combo == 1) {  // omega row, omega column
          c0 = lds[A_B0 * n2 + na];
          c1 = lds[A_B1 * n2 + na];
          c2 = lds[A_B2 * n2 + na];
        } else if (combo == 2) {  // psi row, psi column
          c0 = lds[A_E0 * n2 + na];
          c1 = lds[A_E1 * n2 + na];
        } else {  // psi row, omega column
          stiff = false;
          c2 = lds[A_M * n2 + na];
        }
      }
      double v = 0.0;
      if (stiff)
        v = sG01[r * n + q] * sD[r * n + p] * dqs + sG01[p * n + s] * sD[s * n + q] * dpr;
      if (q == s) {
        if (stiff) {
          if (P.tab) {
            v += sT1[(q * n + p) * n + r];
          } else {
            double t = 0.0;
            for (int m = 0; m < n; ++m) t = fma(sG00[m * n + q] * sD[m * n + p], sD[m * n + r], t);
            v += t;
          }
        }
        if (DPN == 2) v = fma(c0, dpr, v);
      }
      if (p == r) {
        if (stiff) {
          if (P.tab) {
            v += sT4[(p * n + q) * n + s];
          } else {
            double t = 0.0;
            for (int m = 0; m < n; ++m) t = fma(sG11[p * n + m] * sD[m * n + q], sD[m * n + s], t);
            v += t;
          }
        }
        if (DPN == 2) {
          v = fma(c1, dqs, v);
          if (na == nb) v += c2;
        }
      }
      __builtin_nontemporal_store(v, out + idx);
      a += da;
      b += db;
      if (b >= nl) {
        b -= nl;
        ++a;
      }
    }
  }
}

}  // namespace

extern "C" int sem_elem_matrices(int op_kind, int ndim, int p, int64_t n_elem,
                                 const double* d_x_phys, const double* h_D, const double* h_w,
                                 double re, const uint32_t* d_e2n, const double* d_state,
                                 const int32_t* h_local_order, int64_t elem_begin,
                                 int64_t elem_count, double* d_mat, double* d_rhs, void* stream) {
  // every argument is checked before any device call
  if (op_kind == SEM_OP_AXISYM_NS_JVP)
    return fail(SEM_E_NOTIMPL, "sem_elem_matrices: the Jacobian is the matrix of SEM_OP_AXISYM_NS");
  if (op_kind != SEM_OP_POISSON && op_kind != SEM_OP_AXISYM_STOKES && op_kind != SEM_OP_AXISYM_NS)
    return fail(SEM_E_INVALID, "sem_elem_matrices: unknown op_kind");
  if (ndim != 2) return fail(SEM_E_NOTIMPL, "sem_elem_matrices: ndim must be 2");
  if (p < 1) return fail(SEM_E_INVALID, "sem_elem_matrices: p must be >= 1");
  if (p > SEM_MAX_ORDER) return fail(SEM_E_NOTIMPL, "sem_elem_matrices: p must be <= 16");
  if (n_elem < 0 || elem_begin < 0 || elem_count < 0 || elem_begin > n_elem ||
      elem_count > n_elem - elem_begin)
    return fail(SEM_E_INVALID, "sem_elem_matrices: element range outside [0, n_elem]");
  const int n = p + 1, dpn = op_kind == SEM_OP_POISSON ? 1 : 2, nl = dpn * n * n;
  if (h_local_order) {
    std::vector<char> seen((size_t)nl, 0);
    for (int a = 0; a < nl; ++a) {
      const int32_t l = h_local_order[a];
      if (l < 0 || l >= nl || seen[l])
        return fail(SEM_E_INVALID,
                    "sem_elem_matrices: h_local_order is not a permutation of 0..nl-1");
      seen[l] = 1;
    }
  }
  if (!d_x_phys || !h_D || !h_w || !d_e2n || !d_mat)
    return fail(SEM_E_INVALID, "sem_elem_matrices: NULL array");
  if (d_rhs && !d_state) return fail(SEM_E_INVALID, "sem_elem_matrices: d_rhs needs d_state");
  if (op_kind == SEM_OP_AXISYM_NS && !d_state)
    return fail(SEM_E_INVALID, "sem_elem_matrices: SEM_OP_AXISYM_NS needs d_state");
  if (elem_count == 0) return SEM_OK;

  ElmatBasis B;
  for (int i = 0; i < n * n; ++i) B.D[i] = h_D[i];
  for (int i = 0; i < n; ++i) B.w[i] = h_w[i];
  for (int a = 0; a < nl; ++a) B.ord[a] = (uint16_t)(h_local_order ? h_local_order[a] : a);
  ElmatArgs P;
  P.n = n;
  P.kind = op_kind;
  P.tab = elmat_lds(dpn, n, true) <= ELMAT_LDS_LIMIT ? 1 : 0;
  P.re = re;
  P.x_phys = d_x_phys;
  P.e2n = d_e2n;
  // the linear kinds read the state for the right-hand side only
  P.state = (op_kind == SEM_OP_AXISYM_NS || d_rhs) ? d_state : nullptr;
  P.elem_begin = elem_begin;
  P.elem_count = elem_count;
  P.mat = d_mat;
  P.rhs = d_rhs;
  const size_t lds = elmat_lds(dpn, n, P.tab != 0);
  const unsigned grid = (unsigned)(elem_count < ELMAT_MAX_GRID ? elem_count : ELMAT_MAX_GRID);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dpn == 1)
    k_elem_matrices<1><<<grid, ELMAT_BLOCK, lds, st>>>(B, P);
  else
    k_elem_matrices<2><<<grid, ELMAT_BLOCK, lds, st>>>(B, P);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    return fail(SEM_E_HIP, std::string("sem_elem_matrices: ") + hipGetErrorString(err));
  return SEM_OK;
}
