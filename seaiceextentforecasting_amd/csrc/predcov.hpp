// Joint predictive covariance of m test points (sigp_predict_cov):  C = sigma_f (K** + [noise] sn~ I - Z Z^T)  with the solved rows
// Z = k~(Xs, X) L~^-T  [m_pad][n_pad].  Z Z^T is short and wide (m x m outputs, K = n_pad): one workgroup per 128 x 128 output tile would
// leave the chip idle at small m, so K is split over the grid (predcov_partial_kernel) and the slices are summed in a fixed order by the
// pass that also forms the prior and mirrors the lower triangle (predcov_finish_kernel).  No atomics: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"
#include "syrk128.hpp"

namespace sigp {

// Where the partial product of (slice s, tile pair p = (bi, bj), bi >= bj) lives.  Workspace form: part [S][P][128][128]
// (tile_stride = 128 * 128, ldp = 128, slice_stride = P * tile_stride).  In-place form (S == 1): the tile goes straight to its place in the
// [m_pad][m_pad] staging matrix of the finish step (ldp = m_pad).
struct PredcovTiles {
  double* part;
  long tile_stride, ldp, slice_stride;
  int inplace;
  __host__ __device__ long tile_off(int p, int bi, int bj) const {
    return inplace ? ((long)bi * SY_T * ldp + (long)bj * SY_T) : (long)p * tile_stride;
  }
};

// tile pair p of the lower tile space, row by row: row bi holds the pairs (bi, 0) .. (bi, bi)
__device__ __forceinline__ void predcov_pair(int p, int& bi, int& bj) {
  bi = 0;
  while (p > bi) { p -= bi + 1; ++bi; }
  bj = p;
}

// grid = (P tile pairs, S slices).  Slice s covers the block columns [s nkb / S, (s + 1) nkb / S) of Z (nkb = n_pad / 128 >= S: never
// empty, together all of [0, n_pad), lengths differing by at most one block).  The tile loop is syrk128_tile's SET form: LDS-DMA staging,
// two-buffer pipeline, v_mfma_f64_16x16x4_f64; 64 KiB of LDS, two workgroups per CU, as syrk128_kernel.  Diagonal pairs are whole tiles.
__global__ __launch_bounds__(256, 2) void predcov_partial_kernel(const double* __restrict__ Z, long ldz, int nkb, PredcovTiles t) {
  constexpr int KTe = Num<double>::KT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* As = (double*)smem_raw;        // [2][128][KT]
  double* Bs = As + 2 * SY_T * KTe;      // [2][128][KT]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int bi, bj;
  predcov_pair((int)blockIdx.x, bi, bj);
  const int S = (int)gridDim.y, s = (int)blockIdx.y;
  const long kb0 = (long)s * nkb / S, kb1 = (long)(s + 1) * nkb / S;
  const double* Ag = Z + (long)bi * SY_T * ldz + kb0 * SY_T;
  const double* Bg = Z + (long)bj * SY_T * ldz + kb0 * SY_T;
  double* Cw = t.part + (long)s * t.slice_stride + t.tile_off((int)blockIdx.x, bi, bj) + (long)(wm * 64) * t.ldp + wn * 64;
  unsigned long long ph0 = 0, ph1 = 0;
  syrk128_tile<double, true>(Ag, ldz, Bg, ldz, Cw, t.ldp, (int)(kb1 - kb0) * SY_T, 0, As, Bs, false, ph0, ph1);
}

struct PredcovFinish {
  PredcovTiles t; int S;
  double* C; long ldc;             // [m_pad][m_pad] staging matrix of the result (the in-place partials live here too)
  const double* Xs; int dp, d;     // padded test rows [m_pad][dp]
  const double* Kss; long ldk;     // reference kernel: T_s Xs^T [m_pad][m_pad] (every tile), else nullptr
  KParams kp;
  double sigma_f;
  int noise;
};

// grid = (P tile pairs, 16 sub-tiles of 32 x 32), 256 threads, four entries each.  Entry (i, j), i >= j:
//   v = sigma_f (k**_ij + [i == j and noise] sn~ - sum_{s = 0 .. S-1} partial_s(i, j))
// goes to (i, j) and, through LDS, to (j, i): bitwise symmetric.  The prior is the unit covariance of the test rows by the device function of
// the builds (its diagonal is exactly 1), or the symmetric part of T_s Xs^T for the reference kernel (both orders of the product are there,
// so the entry does not depend on which of the two points comes first).  In place (S == 1) an entry is read by the thread that overwrites
// it, and the mirrored entries lie where nothing is read.
__global__ __launch_bounds__(256) void predcov_finish_kernel(PredcovFinish g) {
  __shared__ double sh[32][33];
  int bi, bj;
  predcov_pair((int)blockIdx.x, bi, bj);
  const int sr = (int)blockIdx.y >> 2, sc = (int)blockIdx.y & 3;
  if (bi == bj && sr < sc) return;
  const bool dsub = bi == bj && sr == sc;
  const int b = threadIdx.x & 31, a0 = threadIdx.x >> 5;
  const long toff = g.t.tile_off((int)blockIdx.x, bi, bj);
  const int i0 = bi * SY_T + sr * 32, j0 = bj * SY_T + sc * 32;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int a = a0 + 8 * q;
    if (dsub && a < b) continue;
    const int i = i0 + a, j = j0 + b;
    double sum = 0.0;
    const double* pp = g.t.part + toff + (long)(sr * 32 + a) * g.t.ldp + sc * 32 + b;
    for (int s = 0; s < g.S; ++s) sum += pp[(long)s * g.t.slice_stride];
    double prior;
    if (g.Kss != nullptr) {
      prior = 0.5 * (g.Kss[(long)i * g.ldk + j] + g.Kss[(long)j * g.ldk + i]);
    } else {
      const double* xi = g.Xs + (long)i * g.dp;
      const double* xj = g.Xs + (long)j * g.dp;
      double sq = 0.0;
      for (int p = 0; p < g.d; ++p) { const double u = xi[p] - xj[p]; sq += u * u; }
      prior = cov_from_sq(g.kp, sq);
    }
    sh[a][b] = g.sigma_f * (prior + ((i == j && g.noise) ? g.kp.sn : 0.0) - sum);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int a = a0 + 8 * q;
    if (dsub) {
      g.C[(long)(i0 + a) * g.ldc + j0 + b] = a >= b ? sh[a][b] : sh[b][a];
    } else {
      g.C[(long)(i0 + a) * g.ldc + j0 + b] = sh[a][b];
      g.C[(long)(j0 + a) * g.ldc + i0 + b] = sh[b][a];
    }
  }
}

}  // namespace sigp
