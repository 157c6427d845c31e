// Transfer between polynomial orders (include/sem_hip.h, "Transfer"): the
// coefficient vector of the order-p_from discretisation of a mesh carried to
// the order-p_to discretisation of the same elements (prolong), and the exact
// transpose of that matrix (restrict).  Quadrilaterals and hexahedra, any
// pair of orders in 1..16.
//
// One kernel serves both directions.  A workgroup of 256 lanes holds one
// element, or a few small ones side by side (a power-of-two share of the
// lanes each).  It stages the element's input through the element map into
// LDS, contracts one direction after the other with the 1-D matrix (J, or Jt
// for restrict), which also sits in LDS, one lane per output entry, between
// two LDS buffers used in turn; the last direction goes straight to memory:
//   prolong  reads u_from through e2n_from, stores through e2n_to where the
//            entry owns its node (the lowest (element, local) pair);
//   restrict reads r_to through e2n_to at owned entries (0 elsewhere) and
//            stores the element-local result to the handle's scratch; a
//            second kernel then walks the CSR of every "from" node, one lane
//            per node, in ascending (element, local) order: no atomics.
// The orders are run-time arguments (the work is bound by memory).  On
// hexahedra J and the two buffers pass 64 KB for 14 of the 256 order pairs
// (one order 16 and the other >= 10, and 15 with 15; a handle sizes both
// directions): there create asks for the larger LDS of gfx950 explicitly
// (80,920 B at 16 -> 16).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sem_internal.h"
#include "sem_transfer_plan.h"

using sem::fail;

// components the restrict scratch holds: more go through it in turns
#define TRANSFER_SCRATCH_COMP 2
#define TRANSFER_BLOCK 256

struct sem_transfer {
  int ndim = 0, p_from = 0, p_to = 0, nf = 0, nt = 0, nloc_from = 0, nloc_to = 0, device = 0;
  int tpe = 0, epw = 0;  // lanes per element, elements per workgroup
  int64_t n_elem = 0, n_node_from = 0, n_node_to = 0, n_owned = 0, max_row = 0;
  size_t scratch_bytes = 0;
  const uint32_t *d_e2n_from = nullptr, *d_e2n_to = nullptr;  // borrowed
  uint8_t* d_owner = nullptr;
  int32_t *d_ptr = nullptr, *d_entry = nullptr;
  double *d_J = nullptr, *d_Jt = nullptr, *d_scratch = nullptr;
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

// what one launch of the element kernel reads
struct ElemArgs {
  int n_in, n_out, nloc_in, nloc_out;
  int tpe, epw;
  int buf0, buf1;  // doubles per element of the two LDS buffers
  int64_t n_elem;
  const double* M;  // [n_out][n_in]
  const uint32_t *map_in, *map_out;
  const uint8_t* owner;  // of the "to" map: the input side of restrict, the output side of prolong
};

// LDS doubles per element: buffer 0 holds the input and, on hexahedra, the
// result of the second direction; buffer 1 the result of the first
template <int ND>
void lds_buffers(int n_in, int n_out, int* buf0, int* buf1) {
  if (ND == 2) {
    *buf0 = n_in * n_in;
    *buf1 = n_out * n_in;
  } else {
    *buf0 = std::max(n_in * n_in * n_in, n_out * n_out * n_in);
    *buf1 = n_out * n_in * n_in;
  }
}

// Entry o of the contraction of axis a: axes before a already have n_out
// entries, a and those after it n_in; the result has n_out along a.
// sum_j M[i_a][j] src[.., j, ..] in ascending j.
template <int ND>
__device__ inline double contract(const double* __restrict__ M, const double* __restrict__ src,
                                  int a, int n_in, int n_out, int o) {
  int idx[ND];
  for (int i = ND - 1; i >= 0; --i) {
    const int sz = i <= a ? n_out : n_in;
    idx[i] = o % sz;
    o /= sz;
  }
  int st = 1, base = 0, sta = 1;
  for (int i = ND - 1; i >= 0; --i) {
    if (i == a)
      sta = st;
    else
      base += idx[i] * st;
    st *= i < a ? n_out : n_in;
  }
  const double* row = M + idx[a] * n_in;
  double acc = 0.0;
  for (int j = 0; j < n_in; ++j) acc += row[j] * src[base + j * sta];
  return acc;
}

// grid (ceil(n_elem / epw), components).  RESTRICT: out is the scratch
// [component][n_elem][nloc_out]; otherwise the "to" vector.
template <int ND, bool RESTRICT>
__global__ void __launch_bounds__(TRANSFER_BLOCK)
    k_transfer_elem(ElemArgs A, int64_t cs_in, int64_t ns_in, const double* __restrict__ in,
                    int64_t cs_out, int64_t ns_out, double* __restrict__ out) {
  extern __shared__ double lds[];
  const int msz = A.n_out * A.n_in;
  const int sub = threadIdx.x / A.tpe, lane = threadIdx.x % A.tpe;
  double* b0 = lds + msz + sub * (A.buf0 + A.buf1);
  double* b1 = b0 + A.buf0;
  for (int k = threadIdx.x; k < msz; k += TRANSFER_BLOCK) lds[k] = A.M[k];
  const int64_t e = blockIdx.x * (int64_t)A.epw + sub;
  const bool live = e < A.n_elem;
  if (live) {
    const uint32_t* map = A.map_in + e * A.nloc_in;
    const double* src = in + blockIdx.y * cs_in;
    for (int k = lane; k < A.nloc_in; k += A.tpe) {
      const bool take = !RESTRICT || A.owner[e * A.nloc_in + k];
      b0[k] = take ? src[(int64_t)map[k] * ns_in] : 0.0;
    }
  }
  __syncthreads();
  const double* s = b0;
  double* d = b1;
  int cnt = A.nloc_in;
  for (int a = 0; a < ND - 1; ++a) {
    cnt = cnt / A.n_in * A.n_out;
    if (live)
      for (int o = lane; o < cnt; o += A.tpe) d[o] = contract<ND>(lds, s, a, A.n_in, A.n_out, o);
    __syncthreads();
    double* t = const_cast<double*>(s);
    s = d;
    d = t;
  }
  if (!live) return;
  for (int o = lane; o < A.nloc_out; o += A.tpe) {
    const double v = contract<ND>(lds, s, ND - 1, A.n_in, A.n_out, o);
    if (RESTRICT) {
      out[(blockIdx.y * A.n_elem + e) * A.nloc_out + o] = v;
    } else if (A.owner[e * A.nloc_out + o]) {
      out[blockIdx.y * cs_out + (int64_t)A.map_out[e * A.nloc_out + o] * ns_out] = v;
    }
  }
}

// out[c][g] (+)= sum of the scratch entries of node g's CSR row, in the row's
// order; grid (ceil(n_node / 256), components).  A node without a row gets 0
// in overwrite mode and is left alone when accumulating.
__global__ void __launch_bounds__(TRANSFER_BLOCK)
    k_transfer_nodes(int64_t n_node, const int32_t* __restrict__ ptr,
                     const int32_t* __restrict__ entry, int64_t comp_entries,
                     const double* __restrict__ scratch, int64_t cs, int64_t ns,
                     double* __restrict__ out, int accumulate) {
  const int64_t g = blockIdx.x * (int64_t)TRANSFER_BLOCK + threadIdx.x;
  if (g >= n_node) return;
  const int32_t b = ptr[g], e = ptr[g + 1];
  if (accumulate && b == e) return;
  const double* sc = scratch + blockIdx.y * comp_entries;
  double acc = 0.0;
  for (int32_t k = b; k < e; ++k) acc += sc[entry[k]];
  double* o = out + blockIdx.y * cs + g * ns;
  *o = accumulate ? *o + acc : acc;
}

ElemArgs elem_args(const sem_transfer* T, bool restrict_) {
  ElemArgs A;
  A.n_in = restrict_ ? T->nt : T->nf;
  A.n_out = restrict_ ? T->nf : T->nt;
  A.nloc_in = restrict_ ? T->nloc_to : T->nloc_from;
  A.nloc_out = restrict_ ? T->nloc_from : T->nloc_to;
  A.tpe = T->tpe;
  A.epw = T->epw;
  if (T->ndim == 2)
    lds_buffers<2>(A.n_in, A.n_out, &A.buf0, &A.buf1);
  else
    lds_buffers<3>(A.n_in, A.n_out, &A.buf0, &A.buf1);
  A.n_elem = T->n_elem;
  A.M = restrict_ ? T->d_Jt : T->d_J;
  A.map_in = restrict_ ? T->d_e2n_to : T->d_e2n_from;
  A.map_out = restrict_ ? nullptr : T->d_e2n_to;
  A.owner = T->d_owner;
  return A;
}

size_t lds_bytes(const ElemArgs& A) {
  return ((size_t)A.n_out * A.n_in + (size_t)A.epw * (A.buf0 + A.buf1)) * sizeof(double);
}

int check_vectors(const sem_transfer* T, const char* what, int ncomp, int64_t cs_a, int64_t ns_a,
                  const void* a, int64_t cs_b, int64_t ns_b, const void* b) {
  if (!T) return fail(SEM_E_INVALID, std::string(what) + ": transfer is NULL");
  if (ncomp < 1 || ncomp > 65535)
    return fail(SEM_E_INVALID, std::string(what) + ": ncomp must be in [1, 65535]");
  if (cs_a < 0 || ns_a < 1 || cs_b < 0 || ns_b < 1)
    return fail(SEM_E_INVALID, std::string(what) + ": comp_stride >= 0 and node_stride >= 1");
  if (!a || !b) return fail(SEM_E_INVALID, std::string(what) + ": NULL array");
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

int sem_transfer_create(sem_transfer** out, int ndim, int p_from, int p_to, int64_t n_elem,
                        const uint32_t* d_e2n_from, int64_t n_node_from,
                        const uint32_t* d_e2n_to, int64_t n_node_to, int device, void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_transfer_create: out is NULL");
  *out = nullptr;
  int rc = semtransfer::check_sizes(ndim, p_from, p_to, n_elem, n_node_from, n_node_to);
  if (rc != SEM_OK) return rc;
  if (n_elem > 0 && (!d_e2n_from || !d_e2n_to))
    return fail(SEM_E_INVALID, "sem_transfer_create: NULL element map");
  if (device < 0) return fail(SEM_E_INVALID, "sem_transfer_create: device must be >= 0");
  std::vector<double> J, Jt;
  rc = semtransfer::interp_matrix(p_from, p_to, J, Jt);
  if (rc != SEM_OK) return rc;
  Guard guard(device);
  hipStream_t st = S(stream);
  sem_transfer* T = new sem_transfer();
  T->ndim = ndim;
  T->p_from = p_from;
  T->p_to = p_to;
  const int nf = T->nf = p_from + 1, nt = T->nt = p_to + 1;
  T->nloc_from = ndim == 2 ? nf * nf : nf * nf * nf;
  T->nloc_to = ndim == 2 ? nt * nt : nt * nt * nt;
  T->device = device;
  T->n_elem = n_elem;
  T->n_node_from = n_node_from;
  T->n_node_to = n_node_to;
  T->d_e2n_from = d_e2n_from;
  T->d_e2n_to = d_e2n_to;
  // lanes per element: a power of two near half the larger element, so that
  // a lane has about two entries of the last direction
  const int half = (std::max(T->nloc_from, T->nloc_to) + 1) / 2;
  int tpe = 16;
  while (tpe < half && tpe < TRANSFER_BLOCK) tpe *= 2;
  T->tpe = tpe;
  T->epw = TRANSFER_BLOCK / tpe;
#define TRANSFER_TRY(expr)                                                           \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      sem_transfer_destroy(T);                                                       \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
  // two LDS buffers of a large hexahedron pass the 64 KB every launch may
  // have: ask for what gfx950 holds per workgroup
  const size_t lds = std::max(lds_bytes(elem_args(T, false)), lds_bytes(elem_args(T, true)));
  if (lds > 64 * 1024) {
    int lds_max = 0;
    TRANSFER_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (lds > (size_t)lds_max) {
      sem_transfer_destroy(T);
      return fail(SEM_E_NOTIMPL, "sem_transfer_create: this order pair needs " +
                                     std::to_string(lds) + " bytes of LDS per workgroup, the "
                                     "device has " + std::to_string(lds_max));
    }
    TRANSFER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transfer_elem<3, false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TRANSFER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transfer_elem<3, true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  // the maps come to the host: every id is checked before any launch
  const size_t ent_from = (size_t)n_elem * T->nloc_from, ent_to = (size_t)n_elem * T->nloc_to;
  std::vector<uint32_t> h_from(ent_from), h_to(ent_to);
  if (n_elem > 0) {
    TRANSFER_TRY(hipMemcpyAsync(h_from.data(), d_e2n_from, ent_from * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, st));
    TRANSFER_TRY(hipMemcpyAsync(h_to.data(), d_e2n_to, ent_to * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, st));
  }
  TRANSFER_TRY(hipStreamSynchronize(st));
  rc = semtransfer::check_map("from", h_from.data(), (int64_t)ent_from, n_node_from);
  if (rc == SEM_OK) rc = semtransfer::check_map("to", h_to.data(), (int64_t)ent_to, n_node_to);
  if (rc != SEM_OK) {
    sem_transfer_destroy(T);
    return rc;
  }
  semtransfer::Plan pl;
  semtransfer::plan((int64_t)ent_from, h_from.data(), n_node_from, (int64_t)ent_to, h_to.data(),
                    n_node_to, pl);
  T->n_owned = pl.n_owned;
  T->max_row = pl.max_row;
  T->scratch_bytes = std::max<size_t>(ent_from, 1) * TRANSFER_SCRATCH_COMP * sizeof(double);
  TRANSFER_TRY(hipMalloc(&T->d_owner, std::max<size_t>(ent_to, 1)));
  TRANSFER_TRY(hipMalloc(&T->d_ptr, pl.ptr.size() * sizeof(int32_t)));
  TRANSFER_TRY(hipMalloc(&T->d_entry, std::max<size_t>(ent_from, 1) * sizeof(int32_t)));
  TRANSFER_TRY(hipMalloc(&T->d_J, J.size() * sizeof(double)));
  TRANSFER_TRY(hipMalloc(&T->d_Jt, Jt.size() * sizeof(double)));
  TRANSFER_TRY(hipMalloc(&T->d_scratch, T->scratch_bytes));
  TRANSFER_TRY(hipMemcpyAsync(T->d_owner, pl.owner.data(), ent_to, hipMemcpyHostToDevice, st));
  TRANSFER_TRY(hipMemcpyAsync(T->d_ptr, pl.ptr.data(), pl.ptr.size() * sizeof(int32_t),
                              hipMemcpyHostToDevice, st));
  TRANSFER_TRY(hipMemcpyAsync(T->d_entry, pl.entry.data(), ent_from * sizeof(int32_t),
                              hipMemcpyHostToDevice, st));
  TRANSFER_TRY(hipMemcpyAsync(T->d_J, J.data(), J.size() * sizeof(double), hipMemcpyHostToDevice,
                              st));
  TRANSFER_TRY(hipMemcpyAsync(T->d_Jt, Jt.data(), Jt.size() * sizeof(double),
                              hipMemcpyHostToDevice, st));
  TRANSFER_TRY(hipStreamSynchronize(st));  // the host tables are free again
#undef TRANSFER_TRY
  *out = T;
  return SEM_OK;
}

void sem_transfer_destroy(sem_transfer* T) {
  if (!T) return;
  {
    Guard guard(T->device);
    (void)hipFree(T->d_owner);
    (void)hipFree(T->d_ptr);
    (void)hipFree(T->d_entry);
    (void)hipFree(T->d_J);
    (void)hipFree(T->d_Jt);
    (void)hipFree(T->d_scratch);
  }
  delete T;
}

int sem_transfer_prolong(sem_transfer* T, int ncomp, int64_t cs_from, int64_t ns_from,
                         const double* d_u_from, int64_t cs_to, int64_t ns_to, double* d_u_to,
                         void* stream) {
  int rc = check_vectors(T, "sem_transfer_prolong", ncomp, cs_from, ns_from, d_u_from, cs_to,
                         ns_to, d_u_to);
  if (rc != SEM_OK) return rc;
  if (T->n_elem == 0) return SEM_OK;
  Guard guard(T->device);
  const ElemArgs A = elem_args(T, false);
  const dim3 grid(blocks_for(T->n_elem, T->epw), (unsigned)ncomp);
  if (T->ndim == 2)
    k_transfer_elem<2, false><<<grid, TRANSFER_BLOCK, lds_bytes(A), S(stream)>>>(
        A, cs_from, ns_from, d_u_from, cs_to, ns_to, d_u_to);
  else
    k_transfer_elem<3, false><<<grid, TRANSFER_BLOCK, lds_bytes(A), S(stream)>>>(
        A, cs_from, ns_from, d_u_from, cs_to, ns_to, d_u_to);
  HIP_TRY(hipGetLastError());
  return SEM_OK;
}

int sem_transfer_restrict(sem_transfer* T, int ncomp, int64_t cs_to, int64_t ns_to,
                          const double* d_r_to, int64_t cs_from, int64_t ns_from,
                          double* d_r_from, int accumulate, void* stream) {
  int rc = check_vectors(T, "sem_transfer_restrict", ncomp, cs_to, ns_to, d_r_to, cs_from,
                         ns_from, d_r_from);
  if (rc != SEM_OK) return rc;
  if (T->n_node_from == 0) return SEM_OK;
  Guard guard(T->device);
  const ElemArgs A = elem_args(T, true);
  const int64_t comp_entries = T->n_elem * T->nloc_from;
  for (int c0 = 0; c0 < ncomp; c0 += TRANSFER_SCRATCH_COMP) {
    const unsigned nc = (unsigned)std::min(TRANSFER_SCRATCH_COMP, ncomp - c0);
    if (T->n_elem > 0) {
      const dim3 grid(blocks_for(T->n_elem, T->epw), nc);
      if (T->ndim == 2)
        k_transfer_elem<2, true><<<grid, TRANSFER_BLOCK, lds_bytes(A), S(stream)>>>(
            A, cs_to, ns_to, d_r_to + c0 * cs_to, 0, 1, T->d_scratch);
      else
        k_transfer_elem<3, true><<<grid, TRANSFER_BLOCK, lds_bytes(A), S(stream)>>>(
            A, cs_to, ns_to, d_r_to + c0 * cs_to, 0, 1, T->d_scratch);
      HIP_TRY(hipGetLastError());
    }
    k_transfer_nodes<<<dim3(blocks_for(T->n_node_from, TRANSFER_BLOCK), nc), TRANSFER_BLOCK, 0,
                       S(stream)>>>(T->n_node_from, T->d_ptr, T->d_entry, comp_entries,
                                    T->d_scratch, cs_from, ns_from, d_r_from + c0 * cs_from,
                                    accumulate);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int sem_transfer_info(sem_transfer* T, int64_t* info, int n_info) {
  if (!T || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_transfer_info: NULL argument");
  const int64_t v[9] = {T->ndim,      T->p_from, T->p_to,   T->n_elem,
                        T->n_node_from, T->n_node_to, T->n_owned, T->max_row,
                        (int64_t)T->scratch_bytes};
  for (int i = 0; i < std::min(n_info, 9); ++i) info[i] = v[i];
  return SEM_OK;
}

}  // extern "C"
