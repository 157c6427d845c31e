// Point location and field evaluation at arbitrary physical points
// (include/sem_hip.h, "Points"): the device form of the reference's
// DOFManager.find_elem_containing_point / interpolate (sem/discrete.py:
// 221-233, 263-280) and Mapping.inv (sem/mapping.py:146-178).
//
// Setup (sem_points_create).  Per element, from x_phys [E][ndim][n^ndim]:
// an axis-aligned box over its GLL coefficients inflated by
// SEM_POINTS_BOX_MARGIN of its extent, and the centroid of its 2^d corner
// coefficients (k_pts_boxes).  The boxes (not x_phys) go to the host, which
// lays a uniform grid of about E cells over the mesh box and lists, per
// cell, the elements whose box meets it (CSR).
//
// Location (k_pts_locate): one lane per point.  The lane walks the
// candidates of its cell whose box holds the point, in ascending centroid
// distance (ties: element id), and runs the reference's Newton in each:
// xi = 0, at most 8 steps, stop at |dx|_2 <= 1e-8, analytic Jacobian
// sum c l' (x) l, closed-form 2x2 / 3x3 solve.  The 1-D basis values and
// derivatives of a lane live in an LDS column [array][k][lane] (no barrier:
// a lane reads only its own column), so the loops over xi0 (and xi1 on
// hexahedra) stay rolled at every order and the innermost one unrolls.
//
// Evaluation (k_pts_eval, the hot path).  sem_points_plan buckets the points
// by element (count, host scan, fill) and cuts every element's run into items
// of at most W points (W = 16 or 64, from the mean run length).  A 256-thread
// workgroup holds 256 / W items; the W lanes of an item gather a slab of
// their element's coefficients (all n^2 on quadrilaterals, one xi0 plane of
// n^2 on hexahedra) through the element map into LDS with coalesced map
// reads, then every lane contracts the slab with its own basis values held
// in registers: all lanes of an item read the same LDS address at each step
// (a broadcast).  Points in no run are written as NaN by a second small
// launch over the tail of the permutation and index no memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "sem_points.h"

using sem::fail;

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

using namespace semp;

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

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

// ---------------------------------------------------------------- setup
// box over the coefficients of element e, inflated, and the corner centroid
__global__ void k_pts_boxes(int64_t n_elem, int ndim, int n, int64_t nloc,
                            const double* __restrict__ x, double margin,
                            double* __restrict__ box, double* __restrict__ cen) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n_elem) return;
  for (int c = 0; c < ndim; ++c) {
    const double* xc = x + (e * ndim + c) * nloc;
    double lo = xc[0], hi = xc[0];
    for (int64_t k = 1; k < nloc; ++k) {
      const double v = xc[k];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    const double pad = margin * (hi - lo) + 1e-14 * fmax(fabs(lo), fabs(hi));
    box[e * 2 * ndim + c] = lo - pad;
    box[e * 2 * ndim + ndim + c] = hi + pad;
    // corners: every index 0 or n - 1 (reference Mesh._compute_cell_centroids)
    double s = 0.0;
    for (int v = 0; v < (1 << ndim); ++v) {
      int64_t idx = 0;
      for (int d = 0; d < ndim; ++d) idx = idx * n + (((v >> d) & 1) ? n - 1 : 0);
      s += xc[idx];
    }
    cen[e * ndim + c] = s / (double)(1 << ndim);
  }
}

// ---------------------------------------------------------------- plan
__global__ void k_pts_count(int64_t n_pts, int64_t n_elem, const int32_t* __restrict__ elem,
                            int32_t* __restrict__ count) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_pts) return;
  const int32_t e = elem[i];
  if (e >= 0 && (int64_t)e < n_elem) atomicAdd(&count[e], 1);
}

// perm[start[e] + k] = i for the points of element e; points in no run fill
// perm downwards from n_pts - 1.  fill[E] counts them.
__global__ void k_pts_fill(int64_t n_pts, int64_t n_elem, const int32_t* __restrict__ elem,
                           const int32_t* __restrict__ start, int32_t* __restrict__ fill,
                           int32_t* __restrict__ perm) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_pts) return;
  const int32_t e = elem[i];
  if (e >= 0 && (int64_t)e < n_elem)
    perm[start[e] + atomicAdd(&fill[e], 1)] = (int32_t)i;
  else
    perm[n_pts - 1 - atomicAdd(&fill[n_elem], 1)] = (int32_t)i;
}

// NaN for the points in no run: the tail perm[n_valid .. n_pts)
__global__ void k_pts_nan(const int32_t* __restrict__ perm, int64_t n_valid, int64_t n_pts,
                          int ncomp, double* __restrict__ out) {
  const int64_t k = n_valid + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= n_pts) return;
  const int64_t pt = perm[k];
  for (int c = 0; c < ncomp; ++c) out[c * n_pts + pt] = std::numeric_limits<double>::quiet_NaN();
}

template <int ND>
int pts_dispatch(int n, const PtsCall& c) {
  int rc = SEM_OK;
  switch (n) {
    case 2: rc = pts_launch<ND, 2>(c); break;
    case 3: rc = pts_launch<ND, 3>(c); break;
    case 4: rc = pts_launch<ND, 4>(c); break;
    case 5: rc = pts_launch<ND, 5>(c); break;
    case 6: rc = pts_launch<ND, 6>(c); break;
    case 7: rc = pts_launch<ND, 7>(c); break;
    case 8: rc = pts_launch<ND, 8>(c); break;
    case 9: rc = pts_launch<ND, 9>(c); break;
    case 10: rc = pts_launch<ND, 10>(c); break;
    case 11: rc = pts_launch<ND, 11>(c); break;
    case 12: rc = pts_launch<ND, 12>(c); break;
    case 13: rc = pts_launch<ND, 13>(c); break;
    case 14: rc = pts_launch<ND, 14>(c); break;
    case 15: rc = pts_launch<ND, 15>(c); break;
    case 16: rc = pts_launch<ND, 16>(c); break;
    case 17: rc = pts_launch<ND, 17>(c); break;
    default: rc = fail(SEM_E_NOTIMPL, "points: order out of range"); break;
  }
  return rc;
}

int pts_run(const PtsCall& c) {
  return c.P->ndim == 2 ? pts_dispatch<2>(c.P->n, c) : pts_dispatch<3>(c.P->n, c);
}

int check_count(int64_t n_pts, const char* what) {
  if (n_pts < 0 || n_pts > (int64_t)std::numeric_limits<int32_t>::max())
    return fail(SEM_E_INVALID, std::string(what) + ": n_pts must be in [0, 2^31)");
  return SEM_OK;
}

}  // namespace

extern "C" {

int sem_points_create(sem_points** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                      int device, void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_points_create: out is NULL");
  *out = nullptr;
  if (ndim != 2 && ndim != 3) return fail(SEM_E_INVALID, "sem_points_create: ndim must be 2 or 3");
  if (p < 1) return fail(SEM_E_INVALID, "sem_points_create: p must be >= 1");
  if (p > SEM_MAX_ORDER) return fail(SEM_E_NOTIMPL, "sem_points_create: p <= 16");
  if (n_elem <= 0 || n_elem > (int64_t)std::numeric_limits<int32_t>::max())
    return fail(SEM_E_INVALID, "sem_points_create: n_elem must be in [1, 2^31)");
  if (!d_x_phys) return fail(SEM_E_INVALID, "sem_points_create: d_x_phys is NULL");
  if (device < 0) return fail(SEM_E_INVALID, "sem_points_create: device must be >= 0");
  Guard guard(device);
  sem_points* P = new sem_points();
  P->ndim = ndim;
  P->p = p;
  P->n = p + 1;
  P->device = device;
  P->n_elem = n_elem;
  P->nloc = ipow(P->n, ndim);
  P->d_x = d_x_phys;
  hipStream_t st = S(stream);
  const int n = P->n;
  std::vector<double> basis(2 * n), quad(n);
  int rc = sem::gll_table(p, basis.data(), basis.data() + n, quad.data());
  if (rc != SEM_OK) {
    delete P;
    return rc;
  }
#define PTS_TRY(expr)                                                                \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      sem_points_destroy(P);                                                         \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
  PTS_TRY(hipMalloc(&P->d_basis, 2 * n * sizeof(double)));
  PTS_TRY(hipMalloc(&P->d_box, n_elem * 2 * ndim * sizeof(double)));
  PTS_TRY(hipMalloc(&P->d_cen, n_elem * ndim * sizeof(double)));
  PTS_TRY(hipMalloc(&P->d_count, sizeof(unsigned long long)));
  PTS_TRY(hipMemcpyAsync(P->d_basis, basis.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice,
                         st));
  k_pts_boxes<<<blocks_for(n_elem, 256), 256, 0, st>>>(n_elem, ndim, n, P->nloc, d_x_phys,
                                                       SEM_POINTS_BOX_MARGIN, P->d_box, P->d_cen);
  PTS_TRY(hipGetLastError());
  std::vector<double> box((size_t)n_elem * 2 * ndim);
  PTS_TRY(hipMemcpyAsync(box.data(), P->d_box, box.size() * sizeof(double), hipMemcpyDeviceToHost,
                         st));
  PTS_TRY(hipStreamSynchronize(st));

  // uniform grid of about E cells over the mesh box
  double lo[3], hi[3];
  for (int d = 0; d < ndim; ++d) {
    lo[d] = std::numeric_limits<double>::infinity();
    hi[d] = -lo[d];
  }
  for (int64_t e = 0; e < n_elem; ++e)
    for (int d = 0; d < ndim; ++d) {
      const double a = box[e * 2 * ndim + d], b = box[e * 2 * ndim + ndim + d];
      if (!std::isfinite(a) || !std::isfinite(b)) {
        sem_points_destroy(P);
        return fail(SEM_E_INVALID, "sem_points_create: x_phys holds a non-finite value");
      }
      lo[d] = std::min(lo[d], a);
      hi[d] = std::max(hi[d], b);
    }
  double vol = 1.0;
  for (int d = 0; d < ndim; ++d) {
    if (!(hi[d] > lo[d])) hi[d] = lo[d] + 1.0;  // a degenerate extent: one cell
    vol *= hi[d] - lo[d];
  }
  const double h = std::pow(vol / (double)n_elem, 1.0 / ndim);
  int64_t n_cells = 1;
  for (int d = 0; d < ndim; ++d) {
    const double want = std::ceil((hi[d] - lo[d]) / h);
    P->g[d] = (int)std::min(std::max(want, 1.0), 32768.0);
    n_cells *= P->g[d];
  }
  while (n_cells > 4 * n_elem + 64) {  // extreme aspect ratios: coarsen the longest axis
    int m = 0;
    for (int d = 1; d < ndim; ++d)
      if (P->g[d] > P->g[m]) m = d;
    n_cells /= P->g[m];
    P->g[m] = (P->g[m] + 1) / 2;
    n_cells *= P->g[m];
  }
  for (int d = 0; d < ndim; ++d) {
    P->lo[d] = lo[d];
    P->inv_h[d] = P->g[d] / (hi[d] - lo[d]);
  }
  P->n_cells = n_cells;
  // CSR: elements whose box meets each cell (two passes: count, fill)
  auto range = [&](int64_t e, int d, int* k0, int* k1) {
    const double a = (box[e * 2 * ndim + d] - P->lo[d]) * P->inv_h[d];
    const double b = (box[e * 2 * ndim + ndim + d] - P->lo[d]) * P->inv_h[d];
    *k0 = std::min(std::max((int)std::floor(a), 0), P->g[d] - 1);
    *k1 = std::min(std::max((int)std::floor(b), 0), P->g[d] - 1);
  };
  std::vector<int32_t> ptr((size_t)n_cells + 1, 0);
  int64_t total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> elems;
    std::vector<int32_t> cur;
    if (pass == 1) {
      if (total > (int64_t)std::numeric_limits<int32_t>::max()) {
        sem_points_destroy(P);
        return fail(SEM_E_INVALID, "sem_points_create: candidate list exceeds 2^31 entries");
      }
      int64_t run = 0;
      for (int64_t c = 0; c < n_cells; ++c) {
        const int32_t k = ptr[c + 1];
        ptr[c] = (int32_t)run;
        run += k;
        P->max_cand = std::max<int64_t>(P->max_cand, k);
      }
      ptr[n_cells] = (int32_t)run;
      elems.resize((size_t)total);
      cur.assign(ptr.begin(), ptr.end() - 1);
    }
    for (int64_t e = 0; e < n_elem; ++e) {
      int k0[3] = {0, 0, 0}, k1[3] = {0, 0, 0};
      for (int d = 0; d < ndim; ++d) range(e, d, &k0[d], &k1[d]);
      for (int a = k0[0]; a <= k1[0]; ++a)
        for (int b = k0[1]; b <= k1[1]; ++b)
          for (int c = k0[2]; c <= k1[2]; ++c) {
            const int64_t cell = ndim == 2 ? (int64_t)a * P->g[1] + b
                                           : ((int64_t)a * P->g[1] + b) * P->g[2] + c;
            if (pass == 0) {
              ++ptr[cell + 1];
              ++total;
            } else {
              elems[cur[cell]++] = (int32_t)e;
            }
          }
    }
    if (pass == 1) {
      P->n_entries = total;
      PTS_TRY(hipMalloc(&P->d_cell_ptr, ptr.size() * sizeof(int32_t)));
      PTS_TRY(hipMalloc(&P->d_cell_elem, std::max<size_t>(elems.size(), 1) * sizeof(int32_t)));
      PTS_TRY(hipMemcpyAsync(P->d_cell_ptr, ptr.data(), ptr.size() * sizeof(int32_t),
                             hipMemcpyHostToDevice, st));
      PTS_TRY(hipMemcpyAsync(P->d_cell_elem, elems.data(), elems.size() * sizeof(int32_t),
                             hipMemcpyHostToDevice, st));
      PTS_TRY(hipStreamSynchronize(st));
    }
  }
#undef PTS_TRY
  *out = P;
  return SEM_OK;
}

void sem_points_destroy(sem_points* P) {
  if (!P) return;
  Guard guard(P->device);
  (void)hipFree(P->d_basis);
  (void)hipFree(P->d_box);
  (void)hipFree(P->d_cen);
  (void)hipFree(P->d_cell_ptr);
  (void)hipFree(P->d_cell_elem);
  (void)hipFree(P->d_count);
  delete P;
}

int sem_points_locate(sem_points* P, int64_t n_pts, const double* d_xq, int32_t* d_elem,
                      double* d_xi, int64_t* n_outside, void* stream) {
  // the count first: a negative n_pts is refused whatever else is passed
  int rc = check_count(n_pts, "sem_points_locate");
  if (rc != SEM_OK) return rc;
  if (!P) return fail(SEM_E_INVALID, "sem_points_locate: pts is NULL");
  if (n_outside) *n_outside = 0;
  if (n_pts == 0) return SEM_OK;
  if (!d_xq || !d_elem || !d_xi) return fail(SEM_E_INVALID, "sem_points_locate: NULL array");
  Guard guard(P->device);
  hipStream_t st = S(stream);
  HIP_TRY(hipMemsetAsync(P->d_count, 0, sizeof(unsigned long long), st));
  PtsGrid grid;
  for (int d = 0; d < 3; ++d) {
    grid.g[d] = P->g[d];
    grid.lo[d] = P->lo[d];
    grid.inv_h[d] = P->inv_h[d];
  }
  PtsCall call = {};
  call.op = PTS_LOCATE;
  call.P = P;
  call.st = st;
  call.n_pts = n_pts;
  call.grid = grid;
  call.xq = d_xq;
  call.elem_out = d_elem;
  call.xi_out = d_xi;
  rc = pts_run(call);
  if (rc != SEM_OK) return rc;
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, P->d_count, sizeof(cnt), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  P->last_outside = (int64_t)cnt;
  P->last_located = n_pts - (int64_t)cnt;
  if (n_outside) *n_outside = (int64_t)cnt;
  return SEM_OK;
}

int sem_points_invert(sem_points* P, int64_t n_pts, const double* d_xq, const int32_t* d_elem_in,
                      const double* d_xi_guess, double* d_xi, uint8_t* d_status, void* stream) {
  // the count first: a negative n_pts is refused whatever else is passed
  int rc = check_count(n_pts, "sem_points_invert");
  if (rc != SEM_OK) return rc;
  if (!P) return fail(SEM_E_INVALID, "sem_points_invert: pts is NULL");
  if (n_pts == 0) return SEM_OK;
  if (!d_xq || !d_elem_in || !d_xi) return fail(SEM_E_INVALID, "sem_points_invert: NULL array");
  Guard guard(P->device);
  hipStream_t st = S(stream);
  PtsCall call = {};
  call.op = PTS_INVERT;
  call.P = P;
  call.st = st;
  call.n_pts = n_pts;
  call.xq = d_xq;
  call.elem_in = d_elem_in;
  call.xi_in = d_xi_guess;
  call.xi_out = d_xi;
  call.status = d_status;
  return pts_run(call);
}

int sem_points_map(sem_points* P, int64_t n_pts, const int32_t* d_elem, const double* d_xi,
                   double* d_x_out, void* stream) {
  // the count first: a negative n_pts is refused whatever else is passed
  int rc = check_count(n_pts, "sem_points_map");
  if (rc != SEM_OK) return rc;
  if (!P) return fail(SEM_E_INVALID, "sem_points_map: pts is NULL");
  if (n_pts == 0) return SEM_OK;
  if (!d_elem || !d_xi || !d_x_out) return fail(SEM_E_INVALID, "sem_points_map: NULL array");
  Guard guard(P->device);
  hipStream_t st = S(stream);
  PtsCall call = {};
  call.op = PTS_MAP;
  call.P = P;
  call.st = st;
  call.n_pts = n_pts;
  call.elem_in = d_elem;
  call.xi_in = d_xi;
  call.x_out = d_x_out;
  return pts_run(call);
}

int sem_points_plan(sem_points* P, int64_t n_pts, const int32_t* d_elem, sem_pplan** out,
                    void* stream) {
  if (!out) return fail(SEM_E_INVALID, "sem_points_plan: out is NULL");
  *out = nullptr;
  // the count first: a negative n_pts is refused whatever else is passed
  int rc = check_count(n_pts, "sem_points_plan");
  if (rc != SEM_OK) return rc;
  if (!P) return fail(SEM_E_INVALID, "sem_points_plan: pts is NULL");
  if (n_pts > 0 && !d_elem) return fail(SEM_E_INVALID, "sem_points_plan: d_elem is NULL");
  Guard guard(P->device);
  hipStream_t st = S(stream);
  sem_pplan* L = new sem_pplan();
  L->pts = P;
  L->device = P->device;
  L->n_pts = n_pts;
  if (n_pts == 0) {
    *out = L;
    return SEM_OK;
  }
  const int64_t E = P->n_elem;
  int32_t *d_cnt = nullptr, *d_start = nullptr;
#define PLAN_TRY(expr)                                                               \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      (void)hipFree(d_cnt);                                                          \
      (void)hipFree(d_start);                                                        \
      sem_points_plan_destroy(L);                                                    \
      return fail(SEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    }                                                                                \
  } while (0)
  PLAN_TRY(hipMalloc(&d_cnt, (E + 1) * sizeof(int32_t)));
  PLAN_TRY(hipMalloc(&d_start, E * sizeof(int32_t)));
  PLAN_TRY(hipMalloc(&L->d_perm, n_pts * sizeof(int32_t)));
  PLAN_TRY(hipMemsetAsync(d_cnt, 0, (E + 1) * sizeof(int32_t), st));
  k_pts_count<<<blocks_for(n_pts, 256), 256, 0, st>>>(n_pts, E, d_elem, d_cnt);
  PLAN_TRY(hipGetLastError());
  std::vector<int32_t> cnt((size_t)E), start((size_t)E);
  PLAN_TRY(hipMemcpyAsync(cnt.data(), d_cnt, E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PLAN_TRY(hipStreamSynchronize(st));
  int64_t run = 0, touched = 0;
  for (int64_t e = 0; e < E; ++e) {
    start[e] = (int32_t)run;
    run += cnt[e];
    touched += cnt[e] > 0;
  }
  L->n_valid = run;
  L->n_touched = touched;
  // lanes per item: short runs (the resampling case, ~16 points per element)
  // share a wavefront four at a time
  L->width = (touched > 0 && run <= 24 * touched) ? 16 : 64;
  std::vector<PtsItem> items;
  items.reserve((size_t)(run / L->width + touched));
  for (int64_t e = 0; e < E; ++e)
    for (int32_t o = 0; o < cnt[e]; o += L->width)
      items.push_back({(int32_t)e, start[e] + o, std::min<int32_t>(L->width, cnt[e] - o)});
  L->n_items = (int64_t)items.size();
  PLAN_TRY(hipMalloc(&L->d_items, std::max<size_t>(items.size(), 1) * sizeof(PtsItem)));
  PLAN_TRY(hipMemcpyAsync(L->d_items, items.data(), items.size() * sizeof(PtsItem),
                          hipMemcpyHostToDevice, st));
  PLAN_TRY(hipMemcpyAsync(d_start, start.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PLAN_TRY(hipMemsetAsync(d_cnt, 0, (E + 1) * sizeof(int32_t), st));
  k_pts_fill<<<blocks_for(n_pts, 256), 256, 0, st>>>(n_pts, E, d_elem, d_start, d_cnt, L->d_perm);
  PLAN_TRY(hipGetLastError());
  PLAN_TRY(hipStreamSynchronize(st));
#undef PLAN_TRY
  (void)hipFree(d_cnt);
  (void)hipFree(d_start);
  *out = L;
  return SEM_OK;
}

void sem_points_plan_destroy(sem_pplan* L) {
  if (!L) return;
  {
    Guard guard(L->device);
    (void)hipFree(L->d_perm);
    (void)hipFree(L->d_items);
  }
  delete L;
}

int sem_points_eval(sem_pplan* L, const uint32_t* d_e2n, const double* d_xi, int ncomp,
                    int64_t comp_stride, int64_t node_stride, const double* d_u, double* d_out,
                    void* stream) {
  if (!L || !L->pts) return fail(SEM_E_INVALID, "sem_points_eval: plan is NULL");
  if (ncomp < 1) return fail(SEM_E_INVALID, "sem_points_eval: ncomp must be >= 1");
  if (comp_stride < 0 || node_stride < 1)
    return fail(SEM_E_INVALID, "sem_points_eval: comp_stride >= 0 and node_stride >= 1");
  if (L->n_pts == 0) return SEM_OK;
  if (!d_e2n || !d_xi || !d_u || !d_out) return fail(SEM_E_INVALID, "sem_points_eval: NULL array");
  sem_points* P = L->pts;
  Guard guard(P->device);
  hipStream_t st = S(stream);
  if (L->n_items > 0) {
    PtsCall call = {};
    call.op = PTS_EVAL;
    call.P = P;
    call.st = st;
    call.n_pts = L->n_pts;
    call.L = L;
    call.e2n = d_e2n;
    call.xi_in = d_xi;
    call.ncomp = ncomp;
    call.comp_stride = comp_stride;
    call.node_stride = node_stride;
    call.u = d_u;
    call.out = d_out;
    const int rc = pts_run(call);
    if (rc != SEM_OK) return rc;
  }
  if (L->n_valid < L->n_pts) {
    k_pts_nan<<<blocks_for(L->n_pts - L->n_valid, 256), 256, 0, st>>>(L->d_perm, L->n_valid,
                                                                      L->n_pts, ncomp, d_out);
    HIP_TRY(hipGetLastError());
  }
  return SEM_OK;
}

int sem_points_info(sem_points* P, int64_t* info, int n_info) {
  if (!P || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_points_info: NULL argument");
  const int64_t v[12] = {P->ndim,    P->p,        P->n_elem,   P->g[0],
                         P->g[1],    P->ndim == 3 ? P->g[2] : 1, P->n_cells, P->n_entries,
                         P->max_cand, P->last_located, P->last_outside, PTS_NEWTON_ITMAX};
  for (int i = 0; i < std::min(n_info, 12); ++i) info[i] = v[i];
  return SEM_OK;
}

int sem_points_plan_info(sem_pplan* L, int64_t* info, int n_info) {
  if (!L || !info || n_info < 0) return fail(SEM_E_INVALID, "sem_points_plan_info: NULL argument");
  const int64_t v[6] = {L->n_pts, L->n_valid, L->n_items, L->n_touched, L->width,
                        PTS_BLOCK / L->width};
  for (int i = 0; i < std::min(n_info, 6); ++i) info[i] = v[i];
  return SEM_OK;
}

}  // extern "C"
