// Boundary faces (include/sem_hip.h, "Faces"): normals, surface quadrature,
// face gradients, surface integrals and the Neumann load vector for a list
// of (element, face) pairs.  The device form of the reference's SubMapping /
// SubFiniteElement (sem/mapping.py:184-272, sem/discrete.py:708-775), which
// builds one Python object per face and leaves the 3-D normal unfinished.
//
// One workgroup per face: one wavefront (64 lanes) on quadrilaterals, 256
// lanes looping over the n^2 <= 289 face nodes on hexahedra.  The parent
// element's coefficients (x_phys one component at a time at create, u
// gathered through the element map afterwards) are staged whole in LDS
// (n^ndim doubles, 39 KB at most) with coalesced reads, so a face whose
// normal axis is not the fastest index still reads whole lines; each lane
// then differentiates along every axis at its face node with rows of D (the
// first or last row along the normal axis).  The order n is a run-time
// argument: the work is a few thousand faces, nothing is unrolled.
//
// Sums are fixed-order: a lane adds its own face nodes in ascending q, the
// lanes are combined by a binary tree in LDS, the per-face values by a second
// single-workgroup launch per component in the same way.  The assembly runs
// one lane per distinct boundary node over that node's CSR row (built on the
// host, csrc/sem_faces_plan.cpp): no atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "sem_faces_plan.h"
#include "sem_internal.h"

using sem::fail;

#define FACES_SCRATCH_COMP 8

struct sem_faces {
  int ndim = 0, p = 0, n = 0, nf = 0, nloc = 0, device = 0;
  int64_t n_elem = 0, F = 0, n_distinct = 0, max_row = 0, max_node = -1;
  int32_t* d_elem = nullptr;
  uint8_t* d_face = nullptr;
  int32_t* d_fidx = nullptr;
  double *d_D = nullptr, *d_w = nullptr;
  double *d_x = nullptr, *d_J = nullptr, *d_invJ = nullptr, *d_detJ = nullptr, *d_ndS = nullptr,
         *d_dSxW = nullptr, *d_scratch = nullptr;
  uint32_t* d_node = nullptr;
  uint32_t* d_bnode = nullptr;
  int32_t *d_ptr = nullptr, *d_entry = nullptr;
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

// what the kernels read of a sem_faces
struct FacesDev {
  int n, nf, nloc;
  int64_t F;
  const int32_t* elem;
  const uint8_t* face;
  const int32_t* fidx;
  const double *D, *w;
  double *x, *J, *invJ, *detJ, *ndS, *dSxW;
  uint32_t* node;
};

FacesDev dev_view(const sem_faces* P) {
  return {P->n,   P->nf,  P->nloc, P->F,    P->d_elem, P->d_face, P->d_fidx, P->d_D,
          P->d_w, P->d_x, P->d_J,  P->d_invJ, P->d_detJ, P->d_ndS,  P->d_dSxW, P->d_node};
}

template <int ND>
constexpr int faces_block() {
  return ND == 2 ? 64 : 256;
}

// d s / d xi_i (i < ND) at the element-local node l of the staged element s
template <int ND>
__device__ inline void local_derivs(const double* s, const double* __restrict__ D, int n, int l,
                                    double* du) {
  int st = 1;
  for (int i = ND - 1; i >= 0; --i) {
    const int ai = (l / st) % n;
    const double* line = s + (l - ai * st);
    const double* row = D + ai * n;
    double acc = 0.0;
    for (int m = 0; m < n; ++m) acc += row[m] * line[m * st];
    du[i] = acc;
    st *= n;
  }
}

// sum of v over the workgroup in a fixed order (every lane calls it);
// the result is valid in lane 0
template <int BLOCK>
__device__ inline double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int h = BLOCK / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  return red[0];
}

// ---------------------------------------------------------------- create
template <int ND>
__global__ void __launch_bounds__(faces_block<ND>())
    k_faces_geom(FacesDev P, const double* __restrict__ x_phys, const uint32_t* __restrict__ e2n) {
  extern __shared__ double s[];
  const int64_t f = blockIdx.x;
  const int n = P.n, nf = P.nf, nloc = P.nloc;
  const int64_t e = P.elem[f];
  const int fc = P.face[f];
  const int32_t* fidx = P.fidx + fc * nf;
  for (int c = 0; c < ND; ++c) {
    const double* xc = x_phys + (e * ND + c) * nloc;
    for (int k = threadIdx.x; k < nloc; k += blockDim.x) s[k] = xc[k];
    __syncthreads();
    for (int q = threadIdx.x; q < nf; q += blockDim.x) {
      const int l = fidx[q];
      P.x[(f * ND + c) * nf + q] = s[l];
      double d[ND];
      local_derivs<ND>(s, P.D, n, l, d);
      for (int i = 0; i < ND; ++i) P.J[((f * ND + c) * ND + i) * nf + q] = d[i];
    }
    __syncthreads();
  }
  const int ax = fc >> 1, side = fc & 1;
  // every lane reads back the J entries it wrote itself
  for (int q = threadIdx.x; q < nf; q += blockDim.x) {
    const int l = fidx[q];
    double J[ND][ND];
    for (int c = 0; c < ND; ++c)
      for (int i = 0; i < ND; ++i) J[c][i] = P.J[((f * ND + c) * ND + i) * nf + q];
    double nd[ND], wq, det;
    double* inv = P.invJ + f * ND * ND * nf + q;  // [i][j] at stride nf
    if constexpr (ND == 2) {
      const int col = 1 - ax;
      const double sg = (fc == 0 || fc == 3) ? -1.0 : 1.0;
      const double tx = sg * J[0][col], ty = sg * J[1][col];
      nd[0] = ty;
      nd[1] = -tx;
      const int a_other = ax == 0 ? l % n : l / n;
      wq = P.w[a_other];
      det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      const double r = 1.0 / det;
      inv[0 * nf] = J[1][1] * r;
      inv[1 * nf] = -J[0][1] * r;
      inv[2 * nf] = -J[1][0] * r;
      inv[3 * nf] = J[0][0] * r;
    } else {
      const int b = (ax + 1) % 3, c2 = (ax + 2) % 3;
      const int c0 = side ? b : c2, c1 = side ? c2 : b;
      const double t0[3] = {J[0][c0], J[1][c0], J[2][c0]};
      const double t1[3] = {J[0][c1], J[1][c1], J[2][c1]};
      nd[0] = t0[1] * t1[2] - t0[2] * t1[1];
      nd[1] = t0[2] * t1[0] - t0[0] * t1[2];
      nd[2] = t0[0] * t1[1] - t0[1] * t1[0];
      int a[3];
      a[0] = l / (n * n);
      a[1] = (l / n) % n;
      a[2] = l % n;
      wq = P.w[a[b]] * P.w[a[c2]];
      // cofactors: inv[i][j] = C[j][i] / det
      double C[3][3];
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
          const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
          C[r][k] = J[r1][k1] * J[r2][k2] - J[r1][k2] * J[r2][k1];
        }
      det = J[0][0] * C[0][0] + J[0][1] * C[0][1] + J[0][2] * C[0][2];
      const double r = 1.0 / det;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) inv[(i * 3 + j) * nf] = C[j][i] * r;
    }
    double dS2 = 0.0;
    for (int c = 0; c < ND; ++c) {
      P.ndS[(f * ND + c) * nf + q] = nd[c];
      dS2 += nd[c] * nd[c];
    }
    P.detJ[f * nf + q] = det;
    P.dSxW[f * nf + q] = sqrt(dS2) * wq;
    P.node[f * nf + q] = e2n[e * nloc + l];
  }
}

// ---------------------------------------------------------------- geometry out
template <int ND>
__global__ void k_faces_export(FacesDev P, double* __restrict__ x, double* __restrict__ ndS,
                               double* __restrict__ dS, double* __restrict__ dSxW,
                               double* __restrict__ unit, uint32_t* __restrict__ node,
                               double* __restrict__ J, double* __restrict__ invJ,
                               double* __restrict__ detJ) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int nf = P.nf;
  if (k >= P.F * nf) return;
  const int64_t f = k / nf;
  const int q = (int)(k - f * nf);
  double nd[ND], s2 = 0.0;
  for (int c = 0; c < ND; ++c) {
    nd[c] = P.ndS[(f * ND + c) * nf + q];
    s2 += nd[c] * nd[c];
  }
  const double s = sqrt(s2);
  for (int c = 0; c < ND; ++c) {
    const int64_t o = (f * ND + c) * nf + q;
    if (x) x[o] = P.x[o];
    if (ndS) ndS[o] = nd[c];
    if (unit) unit[o] = nd[c] / s;
  }
  if (dS) dS[k] = s;
  if (dSxW) dSxW[k] = P.dSxW[k];
  if (node) node[k] = P.node[k];
  if (detJ) detJ[k] = P.detJ[k];
  for (int m = 0; m < ND * ND; ++m) {
    const int64_t o = (f * ND * ND + m) * nf + q;
    if (J) J[o] = P.J[o];
    if (invJ) invJ[o] = P.invJ[o];
  }
}

// ---------------------------------------------------------------- gradient / flux
// grid (F, ncomp).  FLUX: per_face[c][f] = sum_q grad . unit dSxW; otherwise
// grad [c][F][ND][nf] and dudn [c][F][nf] (either may be NULL).
template <int ND, bool FLUX>
__global__ void __launch_bounds__(faces_block<ND>())
    k_faces_grad(FacesDev P, const uint32_t* __restrict__ e2n, int64_t comp_stride,
                 int64_t node_stride, const double* __restrict__ u, double* __restrict__ grad,
                 double* __restrict__ dudn, double* __restrict__ per_face) {
  extern __shared__ double s[];
  __shared__ double red[faces_block<ND>()];
  const int64_t f = blockIdx.x;
  const int64_t c = blockIdx.y;
  const int n = P.n, nf = P.nf, nloc = P.nloc;
  const int64_t e = P.elem[f];
  const int32_t* fidx = P.fidx + (int)P.face[f] * nf;
  const uint32_t* map = e2n + e * nloc;
  const double* uc = u + c * comp_stride;
  for (int k = threadIdx.x; k < nloc; k += blockDim.x) s[k] = uc[(int64_t)map[k] * node_stride];
  __syncthreads();
  double acc = 0.0;
  for (int q = threadIdx.x; q < nf; q += blockDim.x) {
    double du[ND];
    local_derivs<ND>(s, P.D, n, fidx[q], du);
    const double* inv = P.invJ + f * ND * ND * nf + q;
    double dn = 0.0, s2 = 0.0;
    for (int j = 0; j < ND; ++j) {
      double g = 0.0;
      for (int i = 0; i < ND; ++i) g += inv[(i * ND + j) * nf] * du[i];
      const double nd = P.ndS[(f * ND + j) * nf + q];
      dn += g * nd;
      s2 += nd * nd;
      if (!FLUX && grad) grad[((c * P.F + f) * ND + j) * nf + q] = g;
    }
    dn /= sqrt(s2);
    if (FLUX)
      acc += dn * P.dSxW[f * nf + q];
    else if (dudn)
      dudn[(c * P.F + f) * nf + q] = dn;
  }
  if (FLUX) {
    const double tot = block_sum<faces_block<ND>()>(acc, red);
    if (threadIdx.x == 0) per_face[c * P.F + f] = tot;
  }
}

// per_face[c][f] = sum_q vals[c][f][q] dSxW[f][q]; grid (F, ncomp)
template <int ND>
__global__ void __launch_bounds__(faces_block<ND>())
    k_faces_integrate(FacesDev P, const double* __restrict__ vals, double* __restrict__ per_face) {
  __shared__ double red[faces_block<ND>()];
  const int64_t f = blockIdx.x, c = blockIdx.y;
  const int nf = P.nf;
  double acc = 0.0;
  for (int q = threadIdx.x; q < nf; q += blockDim.x)
    acc += vals[(c * P.F + f) * nf + q] * P.dSxW[f * nf + q];
  const double tot = block_sum<faces_block<ND>()>(acc, red);
  if (threadIdx.x == 0) per_face[c * P.F + f] = tot;
}

// total[c] = sum_f per_face[c][f]: one workgroup per component, fixed order
__global__ void __launch_bounds__(256)
    k_faces_total(int64_t F, const double* __restrict__ per_face, double* __restrict__ total) {
  __shared__ double red[256];
  const int64_t c = blockIdx.x;
  double acc = 0.0;
  for (int64_t f = threadIdx.x; f < F; f += 256) acc += per_face[c * F + f];
  const double tot = block_sum<256>(acc, red);
  if (threadIdx.x == 0) total[c] = tot;
}

// out[node] (+)= sum over the node's CSR row of vals dSxW
__global__ void k_faces_assemble(int64_t n_rows, const uint32_t* __restrict__ bnode,
                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ entry,
                                 const double* __restrict__ vals, const double* __restrict__ dSxW,
                                 double* __restrict__ out, int accumulate) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  double acc = 0.0;
  for (int32_t k = ptr[r]; k < ptr[r + 1]; ++k) {
    const int32_t en = entry[k];
    acc += vals[en] * dSxW[en];
  }
  const uint32_t nd = bnode[r];
  out[nd] = accumulate ? out[nd] + acc : acc;
}

int check_fields(const sem_faces* P, const char* what, int ncomp, int64_t comp_stride,
                 int64_t node_stride) {
  if (!P) return fail(SEM_E_INVALID, std::string(what) + ": faces is NULL");
  if (ncomp < 1 || ncomp > 65535)
    return fail(SEM_E_INVALID, std::string(what) + ": ncomp must be in [1, 65535]");
  if (comp_stride < 0 || node_stride < 1)
    return fail(SEM_E_INVALID, std::string(what) + ": comp_stride >= 0 and node_stride >= 1");
  return SEM_OK;
}

// the per-face buffer of a sum: the caller's, or the handle's scratch
int sum_buffer(sem_faces* P, const char* what, int ncomp, double* d_per_face, double** buf) {
  *buf = d_per_face;
  if (!d_per_face) {
    if (ncomp > FACES_SCRATCH_COMP)
      return fail(SEM_E_INVALID, std::string(what) + ": d_per_face may be NULL up to ncomp = 8");
    *buf = P->d_scratch;
  }
  return SEM_OK;
}

}  // namespace

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

extern "C" {

int sem_faces_create(sem_faces** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                     const uint32_t* d_e2n, int64_t n_faces, const int32_t* h_elem,
                     const uint8_t* h_face, const double* h_D, const double* h_w, int device,
                     void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_faces_create: out is NULL");
  *out = nullptr;
  // every (element, face) pair is checked before any device call
  int rc = semfaces::check(ndim, p, n_elem, n_faces, h_elem, h_face);
  if (rc != SEM_OK) return rc;
  if (!d_x_phys || !d_e2n || !h_D || !h_w)
    return fail(SEM_E_INVALID, "sem_faces_create: NULL array");
  if (device < 0) return fail(SEM_E_INVALID, "sem_faces_create: device must be >= 0");
  Guard guard(device);
  hipStream_t st = S(stream);
  sem_faces* P = new sem_faces();
  P->ndim = ndim;
  P->p = p;
  const int n = P->n = p + 1;
  const int nf = P->nf = ndim == 2 ? n : n * n;
  P->nloc = nf * n;
  P->device = device;
  P->n_elem = n_elem;
  const int64_t F = P->F = n_faces;
  std::vector<int32_t> fidx;
  semfaces::index_tables(ndim, n, fidx);
#define FACES_TRY(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      sem_faces_destroy(P);                                                          \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
  const size_t Fa = (size_t)std::max<int64_t>(F, 1), ent = Fa * nf, d2 = (size_t)ndim * ndim;
  FACES_TRY(hipMalloc(&P->d_elem, Fa * sizeof(int32_t)));
  FACES_TRY(hipMalloc(&P->d_face, Fa));
  FACES_TRY(hipMalloc(&P->d_fidx, fidx.size() * sizeof(int32_t)));
  FACES_TRY(hipMalloc(&P->d_D, (size_t)n * n * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_w, (size_t)n * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_x, ent * ndim * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_J, ent * d2 * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_invJ, ent * d2 * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_detJ, ent * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_ndS, ent * ndim * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_dSxW, ent * sizeof(double)));
  FACES_TRY(hipMalloc(&P->d_node, ent * sizeof(uint32_t)));
  FACES_TRY(hipMalloc(&P->d_scratch, Fa * FACES_SCRATCH_COMP * sizeof(double)));
  FACES_TRY(hipMemcpyAsync(P->d_fidx, fidx.data(), fidx.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
  FACES_TRY(hipMemcpyAsync(P->d_D, h_D, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, st));
  FACES_TRY(hipMemcpyAsync(P->d_w, h_w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  std::vector<uint32_t> node((size_t)F * nf);
  if (F > 0) {
    FACES_TRY(hipMemcpyAsync(P->d_elem, h_elem, F * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FACES_TRY(hipMemcpyAsync(P->d_face, h_face, F, hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)P->nloc * sizeof(double);
    if (ndim == 2)
      k_faces_geom<2><<<(unsigned)F, faces_block<2>(), lds, st>>>(dev_view(P), d_x_phys, d_e2n);
    else
      k_faces_geom<3><<<(unsigned)F, faces_block<3>(), lds, st>>>(dev_view(P), d_x_phys, d_e2n);
    FACES_TRY(hipGetLastError());
    FACES_TRY(hipMemcpyAsync(node.data(), P->d_node, node.size() * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, st));
  }
  FACES_TRY(hipStreamSynchronize(st));  // the host lists and h_D / h_w are free again
  semfaces::NodeCsr csr;
  semfaces::node_csr(node.data(), (int64_t)node.size(), csr);
  P->n_distinct = (int64_t)csr.node.size();
  P->max_row = csr.max_row;
  P->max_node = csr.node.empty() ? -1 : (int64_t)csr.node.back();
  FACES_TRY(hipMalloc(&P->d_bnode, std::max<size_t>(csr.node.size(), 1) * sizeof(uint32_t)));
  FACES_TRY(hipMalloc(&P->d_ptr, csr.ptr.size() * sizeof(int32_t)));
  FACES_TRY(hipMalloc(&P->d_entry, std::max<size_t>(csr.entry.size(), 1) * sizeof(int32_t)));
  FACES_TRY(hipMemcpyAsync(P->d_bnode, csr.node.data(), csr.node.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, st));
  FACES_TRY(hipMemcpyAsync(P->d_ptr, csr.ptr.data(), csr.ptr.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
  FACES_TRY(hipMemcpyAsync(P->d_entry, csr.entry.data(), csr.entry.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
  FACES_TRY(hipStreamSynchronize(st));
#undef FACES_TRY
  *out = P;
  return SEM_OK;
}

void sem_faces_destroy(sem_faces* P) {
  if (!P) return;
  {
    Guard guard(P->device);
    (void)hipFree(P->d_elem);
    (void)hipFree(P->d_face);
    (void)hipFree(P->d_fidx);
    (void)hipFree(P->d_D);
    (void)hipFree(P->d_w);
    (void)hipFree(P->d_x);
    (void)hipFree(P->d_J);
    (void)hipFree(P->d_invJ);
    (void)hipFree(P->d_detJ);
    (void)hipFree(P->d_ndS);
    (void)hipFree(P->d_dSxW);
    (void)hipFree(P->d_node);
    (void)hipFree(P->d_scratch);
    (void)hipFree(P->d_bnode);
    (void)hipFree(P->d_ptr);
    (void)hipFree(P->d_entry);
  }
  delete P;
}

int sem_faces_geometry(sem_faces* P, double* d_x, double* d_n_dS, double* d_dS, double* d_dSxW,
                       double* d_unit, uint32_t* d_node_ind, double* d_J, double* d_invJ,
                       double* d_detJ, void* stream) {
  if (!P) return fail(SEM_E_INVALID, "sem_faces_geometry: faces is NULL");
  if (P->F == 0) return SEM_OK;
  Guard guard(P->device);
  const unsigned grid = blocks_for(P->F * P->nf, 256);
  if (P->ndim == 2)
    k_faces_export<2><<<grid, 256, 0, S(stream)>>>(dev_view(P), d_x, d_n_dS, d_dS, d_dSxW, d_unit,
                                                   d_node_ind, d_J, d_invJ, d_detJ);
  else
    k_faces_export<3><<<grid, 256, 0, S(stream)>>>(dev_view(P), d_x, d_n_dS, d_dS, d_dSxW, d_unit,
                                                   d_node_ind, d_J, d_invJ, d_detJ);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_faces_gradient(sem_faces* P, const uint32_t* d_e2n, int ncomp, int64_t comp_stride,
                       int64_t node_stride, const double* d_u, double* d_grad, double* d_dudn,
                       void* stream) {
  int rc = check_fields(P, "sem_faces_gradient", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (P->F == 0 || (!d_grad && !d_dudn)) return SEM_OK;
  if (!d_e2n || !d_u) return fail(SEM_E_INVALID, "sem_faces_gradient: NULL array");
  Guard guard(P->device);
  const dim3 grid((unsigned)P->F, (unsigned)ncomp);
  const size_t lds = (size_t)P->nloc * sizeof(double);
  if (P->ndim == 2)
    k_faces_grad<2, false><<<grid, faces_block<2>(), lds, S(stream)>>>(
        dev_view(P), d_e2n, comp_stride, node_stride, d_u, d_grad, d_dudn, nullptr);
  else
    k_faces_grad<3, false><<<grid, faces_block<3>(), lds, S(stream)>>>(
        dev_view(P), d_e2n, comp_stride, node_stride, d_u, d_grad, d_dudn, nullptr);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_faces_integrate(sem_faces* P, int ncomp, const double* d_vals, double* d_per_face,
                        double* d_total, void* stream) {
  int rc = check_fields(P, "sem_faces_integrate", ncomp, 0, 1);
  if (rc != SEM_OK) return rc;
  if (!d_per_face && !d_total) return SEM_OK;
  double* buf = nullptr;
  rc = sum_buffer(P, "sem_faces_integrate", ncomp, d_per_face, &buf);
  if (rc != SEM_OK) return rc;
  Guard guard(P->device);
  if (P->F > 0) {
    if (!d_vals) return fail(SEM_E_INVALID, "sem_faces_integrate: d_vals is NULL");
    const dim3 grid((unsigned)P->F, (unsigned)ncomp);
    if (P->ndim == 2)
      k_faces_integrate<2><<<grid, faces_block<2>(), 0, S(stream)>>>(dev_view(P), d_vals, buf);
    else
      k_faces_integrate<3><<<grid, faces_block<3>(), 0, S(stream)>>>(dev_view(P), d_vals, buf);
    HIP_TRY(hipGetLastError());
  }
  if (d_total) {
    k_faces_total<<<(unsigned)ncomp, 256, 0, S(stream)>>>(P->F, buf, d_total);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int sem_faces_flux(sem_faces* P, const uint32_t* d_e2n, int ncomp, int64_t comp_stride,
                   int64_t node_stride, const double* d_u, double* d_per_face, double* d_total,
                   void* stream) {
  int rc = check_fields(P, "sem_faces_flux", ncomp, comp_stride, node_stride);
  if (rc != SEM_OK) return rc;
  if (!d_per_face && !d_total) return SEM_OK;
  double* buf = nullptr;
  rc = sum_buffer(P, "sem_faces_flux", ncomp, d_per_face, &buf);
  if (rc != SEM_OK) return rc;
  Guard guard(P->device);
  if (P->F > 0) {
    if (!d_e2n || !d_u) return fail(SEM_E_INVALID, "sem_faces_flux: NULL array");
    const dim3 grid((unsigned)P->F, (unsigned)ncomp);
    const size_t lds = (size_t)P->nloc * sizeof(double);
    if (P->ndim == 2)
      k_faces_grad<2, true><<<grid, faces_block<2>(), lds, S(stream)>>>(
          dev_view(P), d_e2n, comp_stride, node_stride, d_u, nullptr, nullptr, buf);
    else
      k_faces_grad<3, true><<<grid, faces_block<3>(), lds, S(stream)>>>(
          dev_view(P), d_e2n, comp_stride, node_stride, d_u, nullptr, nullptr, buf);
    HIP_TRY(hipGetLastError());
  }
  if (d_total) {
    k_faces_total<<<(unsigned)ncomp, 256, 0, S(stream)>>>(P->F, buf, d_total);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int sem_faces_assemble(sem_faces* P, const double* d_vals, double* d_out, int64_t n_node,
                       int accumulate, void* stream) {
  if (!P) return fail(SEM_E_INVALID, "sem_faces_assemble: faces is NULL");
  // the node ids were read back at create: none may lie past the output
  if (n_node <= P->max_node)
    return fail(SEM_E_INVALID, "sem_faces_assemble: a face node id is >= n_node");
  if (P->n_distinct == 0) return SEM_OK;
  if (!d_vals || !d_out) return fail(SEM_E_INVALID, "sem_faces_assemble: NULL array");
  Guard guard(P->device);
  k_faces_assemble<<<blocks_for(P->n_distinct, 256), 256, 0, S(stream)>>>(
      P->n_distinct, P->d_bnode, P->d_ptr, P->d_entry, d_vals, P->d_dSxW, d_out, accumulate);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_faces_info(sem_faces* P, int64_t* info, int n_info) {
  if (!P || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_faces_info: NULL argument");
  const int64_t v[7] = {P->ndim, P->p, P->F, P->nf, P->n_distinct, P->max_row, P->max_node};
  for (int i = 0; i < std::min(n_info, 7); ++i) info[i] = v[i];
  return SEM_OK;
}

}  // extern "C"
