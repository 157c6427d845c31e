// Hexahedral Poisson action on the fp64 matrix cores, n = 12..17 (p = 11..16;
// included by sem_hex.hip only).  DESIGN.md §4.9.
//
// Same inputs, plan (HexLaunch) and write rule as k_hex_rows; at these orders
// a workgroup holds one element slot (hex_slots(n) = 1) and walks its
// sub-chain along xi0.  The six contractions of an element run as 16 x 16
// tiles of v_mfma_f64_16x16x4_f64 (accumulator layout: lane l, register i
// holds row (l >> 4) + 4 i, column l & 15; A operand lane l = A[l & 15][l >> 4],
// B operand lane l = B[l >> 4][l & 15] of a k-step); the pointwise w = G d
// runs on the VALU in that accumulator layout.
//
// A tile has two indices, the block three: the element's u block sits in LDS
// ([a][b][c], row stride n, plane stride SA padded) and a wavefront takes
// whole index planes ("units"), one at a time:
//
//   gather   thread (b, c) of the column layout: u[map] -> sU           barrier
//   phase A  unit a:  d1[a, :, :] = D U[a, :, :]            -> sX        barrier
//   phase B  unit b:  d0 = D U[:, b, :],  d2 = U[:, b, :] D^T  (registers)
//                     w = G (d0, d1, d2) at (a = h + 4 i, b, c): w0 stays in
//                     registers (it is the B operand of D^T w0 as it lies),
//                     w1 -> sX in place of d1, w2 -> sU in place of U[:, b, :]
//                     (dead: only this unit read it after phase A)
//                     y02 = D^T w0 + w2 D  -> sU[:, b, :]               barrier
//   phase C  unit a:  sU[a, :, :] += D^T w1[a, :, :]                    barrier
//   store    thread (b, c): its column of sU, the write rule of k_hex_rows
//
// so the xi1 contractions are the ones taken in the other orientation, and
// their operands (d1 in, w1 out) are what crosses between orientations
// through LDS.  Inside phase B a plane belongs to one wavefront: its steps
// are ordered by wavefront fences, not workgroup barriers.  The D fragments
// (FA[t][s] = D[16 t + (l & 15)][4 s + (l >> 4)] and its transpose FT) stay
// in registers for the whole sub-chain; they serve as A or B operand of all
// six contractions.
//
// n < 16 is one zero-padded tile with ceil(n / 4) k-steps; n = 17 runs
// zero-padded 2 x 2 tiles with five k-steps (the second tile row / column
// holds index 16 alone).  A lane whose row, column or summation index is
// >= n supplies zero without issuing the load, and drops its results.
//
// The plane stride SA = n^2 rounded up to 4 mod 8 doubles: the A-operand
// reads (lanes 0..15 at stride SA, + l >> 4) then touch all 32 eight-byte
// bank pairs twice, the minimum for 64 lanes.
#pragma once
#include "sem_hex.h"

namespace semh {

typedef double hdbl4 __attribute__((ext_vector_type(4)));

constexpr int HEX_MFMA_MIN_N = 12;
constexpr int HEX_MFMA_MAX_N = 17;
constexpr int hex_mfma_sa(int n) {
  int s = n * n;
  while (s % 8 != 4) ++s;
  return s;
}
// LDS (two n^3 blocks: 28 / 35 / 44 / 54 / 66 / 79 KB at n = 12..17) leaves
// 5 / 4 / 3 / 2 / 2 / 2 workgroups per CU.  Two waves per SIMD requested where
// the tiles are single (the allocator takes 108-145 VGPRs there, three to
// four waves); the 2 x 2 tiles of n = 17 need 224-240 VGPRs, and a bound of
// three waves per SIMD (168) spills
constexpr int hex_mfma_min_waves(int n) { return n <= 16 ? 2 : 1; }

__device__ __forceinline__ hdbl4 hex_mfma(double a, double b, hdbl4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// orders the LDS accesses of one wavefront (a plane of phase B is private to it)
__device__ __forceinline__ void hex_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int N, int MODE, bool TM = false>
__global__ void __launch_bounds__(hex_threads(N), hex_mfma_min_waves(N))
    k_hex_mfma(const double* __restrict__ u, double* __restrict__ y,
               const uint32_t* __restrict__ map, const double* __restrict__ G,
               const double* __restrict__ gD, HexLaunch P) {
  static_assert(MODE == HEX_SET || MODE == HEX_ACC, "matrix-core form: the action only");
  static_assert(N >= HEX_MFMA_MIN_N && N <= HEX_MFMA_MAX_N && hex_slots(N) == 1,
                "one element slot per workgroup");
  constexpr int N2 = N * N, N3 = N2 * N, T = hex_threads(N), NBC = hex_nbc(N);
  constexpr int NW = T / 64;         // wavefronts
  constexpr int NT = (N + 15) / 16;  // tiles per index
  constexpr int KS = (N + 3) / 4;    // k-steps
  constexpr int SA = hex_mfma_sa(N);
  constexpr int GROW = 3 * N2, GPAIR = N2;  // factor layout (hex_g)
  __shared__ double sU[N * SA];  // u, then w2, then y: [a][b][c] at a * SA + b * N + c
  __shared__ double sX[N3];      // d1, then w1:        [a][b][c] at a * N2 + b * N + c
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 4, cl = lane & 15;
  // D fragments
  double FA[NT][KS], FT[NT][KS];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int r = 16 * t + cl, k = 4 * s + h;
      FA[t][s] = 0.0;
      FT[t][s] = 0.0;
      if (r < N && k < N) {
        FA[t][s] = gD[r * N + k];
        FT[t][s] = gD[k * N + r];
      }
    }
  // the column layout of the gather and the stores: thread (b, c)
  const int w = blockIdx.x;
  const int L = P.wg_len[w];
  const int base = P.wg_off[w];
  const bool active = tid < N2;
  const int bc = active ? tid : 0;
  const int b_ = bc / N, c_ = bc - b_ * N;
  static_assert(hex_bcol_agrees<N>(), "hex_bcol_n differs from hex_bcol");
  const int bcol = hex_bcol_n<N>(b_, c_);
  const uint8_t cf = P.cflag[w];
  // hex_face_slot(N, P.face_base, w, 0, 0, bc); the tail face N2 further
  double* const face = P.slot + P.face_base + (int64_t)w * 2 * N2 + bc;
  double carry = 0.0;
  int en = P.elist[base];
  [[maybe_unused]] int toff[TM ? N : 1];  // template map (HexLaunch::tmpl)
  if constexpr (TM)
#pragma unroll
    for (int a = 0; a < N; ++a) toff[a] = P.tmpl[a * N2 + bc];
  // this thread's column of element el's map
  auto load_map = [&](int el, uint32_t (&dst)[N]) {
    if constexpr (TM) {
      const uint32_t eb = P.ebase[el];
#pragma unroll
      for (int a = 0; a < N; ++a) dst[a] = eb + (uint32_t)toff[a];
    } else {
#pragma unroll
      for (int a = 0; a < N; ++a) dst[a] = map[(int64_t)el * N3 + a * N2 + bc];
    }
  };
  // The map entries are read twice per element step, for the gather and
  // again for the stores, instead of staying in registers across the
  // products with the next element's loaded one step ahead, as k_hex_rows
  // does: 17-34 registers that decide between two and three, or three and
  // four, waves per SIMD.  Reading twice measured 13 % faster at p = 12 and
  // p = 16, 3 % slower at p = 15.
  const hdbl4 z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int k = 0; k < L; ++k) {
    const int pos = base + k;
    const int e = en;
    uint32_t m[N];
    if (active) load_map(e, m);
    if (active) {
      double uc[N];
#pragma unroll
      for (int a = 0; a < N; ++a) uc[a] = u[m[a]];
#pragma unroll
      for (int a = 0; a < N; ++a) sU[a * SA + bc] = uc[a];
    }
    __syncthreads();  // u complete; the previous element's sX reads are done
    if (k + 1 < L) en = P.elist[pos + 1];
    // phase A: d1[a, b, c] = sum_r D[b][r] U[a, r, c], tiles (b, c) at fixed a
#pragma unroll 1
    for (int a = wave; a < N; a += NW) {
      const double* const ua = sU + a * SA;
      double* const xa = sX + a * N2;
#pragma unroll
      for (int tc = 0; tc < NT; ++tc) {
        const int c = 16 * tc + cl;
        double Bu[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int r = 4 * s + h;
          Bu[s] = 0.0;
          if (r < N && c < N) Bu[s] = ua[r * N + c];
        }
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) {
          hdbl4 acc = z;
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = hex_mfma(FA[tb][s], Bu[s], acc);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = 16 * tb + h + 4 * i;
            if (b < N && c < N) xa[b * N + c] = acc[i];
          }
        }
      }
    }
    __syncthreads();  // d1 complete
    // phase B: tiles (a, c) at fixed b
#pragma unroll 1
    for (int b = wave; b < N; b += NW) {
      double* const ub = sU + b * N;
      double* const xb = sX + b * N;
      // the factors of this plane's nodes (a = 16 ta + h + 4 i, b, c): per
      // tile row 16 lanes read 16 consecutive pairs, a 256-byte run.  Loaded
      // ahead of the products where a plane is one tile; the 2 x 2 tiles of
      // n = 17 would not fit the register file, they are read where used
      constexpr bool GPRE = NT == 1;
      [[maybe_unused]] double2 q[GPRE ? 4 : 1][3];
      if constexpr (GPRE) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int a = h + 4 * i;
#pragma unroll
          for (int j = 0; j < 3; ++j) q[i][j] = make_double2(0.0, 0.0);
          if (a < N && cl < N) {
            const double2* ga = hex_g<N>(G, e, b * N + cl) + a * GROW;
#pragma unroll
            for (int j = 0; j < 3; ++j) q[i][j] = ga[j * GPAIR];
          }
        }
      }
      double Bu[NT][KS], Au[NT][KS];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int x = 16 * t + cl, r = 4 * s + h;
          Bu[t][s] = 0.0;
          Au[t][s] = 0.0;
          if (x < N && r < N) {
            Bu[t][s] = ub[r * SA + x];  // U[r, b, c = x]
            Au[t][s] = ub[x * SA + r];  // U[a = x, b, r]
          }
        }
      hdbl4 d0[NT][NT], d2[NT][NT];
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tc = 0; tc < NT; ++tc) {
          hdbl4 a0 = z, a2 = z;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            a0 = hex_mfma(FA[ta][s], Bu[tc][s], a0);  // D U
            a2 = hex_mfma(Au[ta][s], FA[tc][s], a2);  // U D^T
          }
          d0[ta][tc] = a0;
          d2[ta][tc] = a2;
        }
      hex_wave_sync();  // every read of U[:, b, :] precedes the w2 stores
      double w0[NT][NT][4];
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tc = 0; tc < NT; ++tc)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int a = 16 * ta + h + 4 * i, c = 16 * tc + cl;
            w0[ta][tc][i] = 0.0;
            if (a < N && c < N) {
              double2 q0, q1, q2;
              if constexpr (GPRE) {
                q0 = q[i][0], q1 = q[i][1], q2 = q[i][2];
              } else {
                const double2* ga = hex_g<N>(G, e, b * N + c) + a * GROW;
                q0 = ga[0], q1 = ga[GPAIR], q2 = ga[2 * GPAIR];
              }
              const double g00 = q0.x, g01 = q0.y, g02 = q1.x, g11 = q1.y, g12 = q2.x, g22 = q2.y;
              const double e0 = d0[ta][tc][i], e1 = xb[a * N2 + c], e2 = d2[ta][tc][i];
              w0[ta][tc][i] = g00 * e0 + g01 * e1 + g02 * e2;
              xb[a * N2 + c] = g01 * e0 + g11 * e1 + g12 * e2;
              ub[a * SA + c] = g02 * e0 + g12 * e1 + g22 * e2;
            }
          }
      hex_wave_sync();  // w2 complete
      double Aw[NT][KS];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int a = 16 * t + cl, r = 4 * s + h;
          Aw[t][s] = 0.0;
          if (a < N && r < N) Aw[t][s] = ub[a * SA + r];  // w2[a, b, r]
        }
      hdbl4 yt[NT][NT];
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tc = 0; tc < NT; ++tc) {
          hdbl4 acc = z;
          // D^T w0: register i of w0's tile row tr is k-step 4 tr + i as it lies
#pragma unroll
          for (int tr = 0; tr < NT; ++tr)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (4 * tr + i < KS) acc = hex_mfma(FT[ta][4 * tr + i], w0[tr][tc][i], acc);
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = hex_mfma(Aw[ta][s], FT[tc][s], acc);  // w2 D
          yt[ta][tc] = acc;
        }
      hex_wave_sync();  // every read of w2 precedes the y stores
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tc = 0; tc < NT; ++tc)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int a = 16 * ta + h + 4 * i, c = 16 * tc + cl;
            if (a < N && c < N) ub[a * SA + c] = yt[ta][tc][i];
          }
    }
    __syncthreads();  // w1 and y02 complete
    // phase C: y[a, b, c] += sum_q D[q][b] w1[a, q, c], tiles (b, c) at fixed a
#pragma unroll 1
    for (int a = wave; a < N; a += NW) {
      double* const ya = sU + a * SA;
      const double* const xa = sX + a * N2;
#pragma unroll
      for (int tc = 0; tc < NT; ++tc) {
        const int c = 16 * tc + cl;
        double Bw[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int r = 4 * s + h;
          Bw[s] = 0.0;
          if (r < N && c < N) Bw[s] = xa[r * N + c];
        }
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) {
          hdbl4 acc = z;
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = hex_mfma(FT[tb][s], Bw[s], acc);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = 16 * tb + h + 4 * i;
            if (b < N && c < N) ya[b * N + c] += acc[i];
          }
        }
      }
    }
    __syncthreads();  // y complete
    // the write rule of k_hex_rows (sem_hex_plan.cpp thread_rows), thread (b, c):
    // its column of y
    if (active) {
      load_map(e, m);
      double yv[N];
#pragma unroll
      for (int a = 0; a < N; ++a) yv[a] = sU[a * SA + bc];  // rewritten by this thread only
      if (k > 0) yv[0] += carry;
      const bool last = k == L - 1;
      if (!last) carry = yv[N - 1];
      const bool colslot = bcol >= 0 && ((P.cmask[pos] >> bcol) & 1ull);
      double* const cs = P.slot + ((int64_t)pos * N) * NBC + bcol;
#pragma unroll
      for (int a = 0; a < N; ++a) {
        if (a == N - 1 && !last) continue;  // carried into the next element's row 0
        const double v = yv[a];
        if (a == 0 && k == 0 && (cf & HEX_CF_HEAD)) {
          face[0] = v;
        } else if (a == N - 1 && last && (cf & HEX_CF_TAIL)) {
          face[N2] = v;
        } else if (colslot) {
          cs[a * NBC] = v;
        } else {
          if constexpr (MODE == HEX_ACC)
            y[m[a]] += v;
          else
            y[m[a]] = v;
        }
      }
    }
  }
}

}  // namespace semh
