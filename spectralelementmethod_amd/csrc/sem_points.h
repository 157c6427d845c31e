// Shared declarations of the point location / evaluation unit
// (sem_points.hip: C ABI and setup; sem_points_launch.hip: the per-order
// kernels, compiled once per range of orders like sem_launch.hip).
#pragma once
#include "sem_internal.h"

struct sem_points {
  int ndim = 0, p = 0, n = 0, device = 0;
  int64_t n_elem = 0, nloc = 0;
  const double* d_x = nullptr;  // borrowed x_phys [E][ndim][nloc]
  double* d_basis = nullptr;    // [2][n]: GLL nodes, barycentric weights
  double* d_box = nullptr;      // [E][2 * ndim]: lo[ndim], hi[ndim] (inflated)
  double* d_cen = nullptr;      // [E][ndim]
  int32_t* d_cell_ptr = nullptr;  // [n_cells + 1]
  int32_t* d_cell_elem = nullptr;
  unsigned long long* d_count = nullptr;  // n_outside
  int g[3] = {1, 1, 1};
  double lo[3] = {0, 0, 0}, inv_h[3] = {0, 0, 0};
  int64_t n_cells = 0, n_entries = 0, max_cand = 0;
  // last calls (sem_points_info)
  int64_t last_located = 0, last_outside = 0;
};

struct PtsItem {
  int32_t elem, start, count;
};

struct sem_pplan {
  sem_points* pts = nullptr;
  int64_t n_pts = 0, n_valid = 0, n_items = 0, n_touched = 0;
  int width = 64;
  int device = 0;          // of pts (the plan's own copy: destroy does not touch pts)
  int32_t* d_perm = nullptr;  // [n_pts]: runs first, points in no run last
  PtsItem* d_items = nullptr;
};

namespace semp {

constexpr int PTS_NEWTON_ITMAX = 8;
constexpr double PTS_NEWTON_TOL = 1e-8;
constexpr int PTS_BLOCK = 256;  // evaluation workgroup
constexpr int PTS_LANES = 64;   // location workgroup: one wavefront

__host__ __device__ constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

struct PtsGrid {
  int g[3];
  double lo[3], inv_h[3];
};

enum PtsOp { PTS_LOCATE = 0, PTS_INVERT = 1, PTS_MAP = 2, PTS_EVAL = 3 };

// one launch of a per-order kernel (pts_launch<ND, N>)
struct PtsCall {
  PtsOp op;
  const sem_points* P;
  hipStream_t st;
  int64_t n_pts;
  PtsGrid grid;                // locate
  const double* xq;            // locate, invert
  const int32_t* elem_in;      // invert, map
  const double* xi_in;         // invert (guess, may be null), map, eval
  int32_t* elem_out;           // locate
  double* xi_out;              // locate, invert
  uint8_t* status;             // invert
  double* x_out;               // map
  const sem_pplan* L;          // eval
  const uint32_t* e2n;
  int ncomp;
  int64_t comp_stride, node_stride;
  const double* u;
  double* out;
};

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <int ND, int N>
int pts_launch(const PtsCall& c);

}  // namespace semp
