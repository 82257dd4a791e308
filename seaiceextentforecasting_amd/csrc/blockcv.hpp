// Leave-block-out cross-validation (sigp_cv, sigp_cv_batch): K-fold / h-block / hv-block folds of CONSECUTIVE rows from ONE factorisation.
// With P = K~^-1, a = P y and S the index window a fold removes (its scored rows plus a gap on each side):
//     r_S = P_SS^-1 a_S = y_S - mean_S        Cov_S = s_S P_SS^-1        s_S = (y^T a - a_S^T r_S) / (n - |S|)  or  y^T a / n
// -- what a real refit without the rows of S predicts for them (leave-one-out is |S| = 1).  U = L~^-T is what trtri_levels leaves for
// sigp_loo; P_SS = U_S U_S^T is the short-and-wide product of the row strip U[S, min(S) .. n):
//   cv_strip_partial_kernel   (fold, K slice, member): the strip product on the fp64 matrix pipe, and a_S = U_S z beside it
//   cv_strip_finish_kernel    (fold, member): slices added in a fixed order, mirrored, identity padded to 128 x 128
//   potrf_diag_kernel         the blocked Cholesky's own diagonal-block kernel over the fold blocks: P_SS = M M^T, X = M^-1, info
//   cv_close_kernel           (fold, member): t = X a_S, r = X^T t, a_S^T r = t.t, [P_SS^-1]_ii = sum_k X_ki^2; the scored rows' outputs
// and loo_sum_kernel adds the n score terms.  No atomics anywhere: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_mfma.hpp"
#include "kernels_misc.hpp"

namespace sigp {

constexpr int CV_MAXW = 128;    // widest window (block + 2 gap): one diagonal block of potrf_diag_kernel
constexpr int CV_KC = 32;       // columns of U per LDS stage
constexpr int CV_LP = CV_KC + 2;   // pitch of the [row][k] image: the 8-byte fragment reads (row = lane & 15, k = lane >> 4) of a 32-lane group fall in 32 distinct bank pairs
constexpr int CV_SLOTS = 9;     // 16 x 16 accumulators per wave: the 36 lower subtiles of a 128-row window over four waves

// fold f scores the rows [c0, c1) and removes the window [r0, r1)
__host__ __device__ inline void cv_window(int n, int block, int gap, int f, int& r0, int& r1, int& c0, int& c1) {
  const long a = (long)f * block, b = a + block;
  c0 = (int)a;
  c1 = (int)(b < n ? b : n);
  r0 = c0 - gap > 0 ? c0 - gap : 0;
  r1 = (long)c1 + gap < n ? c1 + gap : n;
}

// threads of a strip workgroup for windows of up to wp = 16 nt rows: one wave per lower subtile, four at most
inline int cv_strip_threads(int wp) {
  const int nt = wp / 16, nsub = nt * (nt + 1) / 2;
  return 64 * (nsub < 4 ? nsub : 4);
}

// grid = (folds of this pass, S slices, members); blockDim = cv_strip_threads(wp).  The window's rows of U, from column kb = r0 rounded
// down to the stage width to the end, are cut into stages of CV_KC columns; slice s takes the stages [s nch / S, (s + 1) nch / S) (possibly
// none: its partial is zero).  What must never reach the product is removed by SELECT on the way to LDS (it may be NaN): entries left of
// the diagonal (k < i: unwritten blocks below the block diagonal, and the unspecified part of a diagonal block), columns >= n (padding),
// rows beyond the window (never loaded: a window is not 128-aligned and row r0 + 127 may lie beyond the allocation).  Every load is
// a 16-byte pair of row i < r1 <= n at columns < n_pad: inside the matrix.
// Subtile (ti, tj), tj <= ti, of the w_pad x w_pad product belongs to wave (index mod waves): D = A B^T with A = rows 16 ti .., B = rows
// 16 tj .. of the image; a lane's accumulator register r is row lq + 4 r, column lr of the subtile (Num<double>::drow).
// part  [member][fold][slice][wp][wp]   (lower subtiles written)        apart [member][fold][slice][wp]:  sum_k U[i, k] z[k] over the slice
__global__ __launch_bounds__(256) void cv_strip_partial_kernel(const double* __restrict__ U, long ld, long sU, const double* __restrict__ z,
                                                               long sZ, int n, int block, int gap, int f0, int wp,
                                                               double* __restrict__ part, double* __restrict__ apart) {
  __shared__ __attribute__((aligned(16))) double T[CV_MAXW * CV_LP];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nthr >> 6;
  const int S = (int)gridDim.y, s = (int)blockIdx.y;
  const long slot_idx = ((long)blockIdx.z * gridDim.x + blockIdx.x) * S + s;
  U += (long)blockIdx.z * sU;
  z += (long)blockIdx.z * sZ;
  part += slot_idx * wp * wp;
  apart += slot_idx * wp;
  int r0, r1, c0, c1;
  cv_window(n, block, gap, f0 + (int)blockIdx.x, r0, r1, c0, c1);
  const int w = r1 - r0, nt = (w + 15) >> 4, nsub = nt * (nt + 1) / 2;
  const int kb = r0 & ~(CV_KC - 1), nch = (((n + CV_KC - 1) & ~(CV_KC - 1)) - kb) / CV_KC;
  const int ch0 = (int)((long)s * nch / S), ch1 = (int)((long)(s + 1) * nch / S);

  int sti[CV_SLOTS], stj[CV_SLOTS];
  d4 acc[CV_SLOTS];
#pragma unroll
  for (int q = 0; q < CV_SLOTS; ++q) {
    int p = wave + q * nw, bi = 0;
    if (p >= nsub) p = 0;
    while (p > bi) { p -= bi + 1; ++bi; }
    sti[q] = bi; stj[q] = p;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[q][r] = 0.0;
  }
  const int nslot = (nsub - wave + nw - 1) / nw;      // subtiles of this wave (uniform per wave; 0 when the window is narrower than the launch's widest)

  // staging: thread -> column pair cp of the stage, rows rrow + rpp q
  const int cp = tid & 15, rrow = tid >> 4, rpp = nthr >> 4;
  d2 pre[8];
  double areg[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) areg[q] = 0.0;
  auto fetch = [&](int c) {
    const int k = kb + c * CV_KC + 2 * cp;
    const d2 zz = *(const d2*)(z + k);
    const double z0 = k < n ? zz[0] : 0.0, z1 = k + 1 < n ? zz[1] : 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = rrow + rpp * q, i = r0 + row;
      d2 v = {0.0, 0.0};
      if (row < w && k + 2 > i) v = *(const d2*)(U + (long)i * ld + k);
      const bool in0 = row < w && k >= i && k < n, in1 = row < w && k + 1 >= i && k + 1 < n;
      v[0] = in0 ? v[0] : 0.0;
      v[1] = in1 ? v[1] : 0.0;
      pre[q] = v;
      areg[q] = fma(v[0], z0, fma(v[1], z1, areg[q]));
    }
  };
  if (ch0 < ch1) fetch(ch0);
  for (int c = ch0; c < ch1; ++c) {
    __syncthreads();                      // every wave is done with the previous stage's image
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = rrow + rpp * q;
      if (row < 16 * nt) *(d2*)(T + row * CV_LP + 2 * cp) = pre[q];
    }
    __syncthreads();
    if (c + 1 < ch1) fetch(c + 1);        // in flight beside the products
#pragma unroll
    for (int kk = 0; kk < CV_KC; kk += 4) {
#pragma unroll
      for (int q = 0; q < CV_SLOTS; ++q) {
        if (q < nslot) {
          const double a = T[(16 * sti[q] + lr) * CV_LP + kk + lq];
          const double b = T[(16 * stj[q] + lr) * CV_LP + kk + lq];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < CV_SLOTS; ++q) {
    if (q < nslot) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(long)(16 * sti[q] + Num<double>::drow(lq, r)) * wp + 16 * stj[q] + lr] = acc[q][r];
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    double v = areg[q];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    const int row = rrow + rpp * q;
    if (cp == 0 && row < w) apart[row] = v;
  }
}

// grid = (folds of this pass, members), 256 threads.  Pb [member][fold][128][128] = P_SS (slices added in the order 0 .. S-1, entry (i, j) taken
// from the computed lower triangle at (max, min): exactly symmetric) inside an identity;  av [member][fold][128] = a_S, zero beyond the window;
// info [member][fold] = 0 for the factorisation that follows.
__global__ __launch_bounds__(256) void cv_strip_finish_kernel(const double* __restrict__ part, const double* __restrict__ apart, int S, int wp,
                                                              int n, int block, int gap, int f0, double* __restrict__ Pb,
                                                              double* __restrict__ av, int* __restrict__ info) {
  const long idx = (long)blockIdx.y * gridDim.x + blockIdx.x;
  int r0, r1, c0, c1;
  cv_window(n, block, gap, f0 + (int)blockIdx.x, r0, r1, c0, c1);
  const int w = r1 - r0;
  const long tile = (long)wp * wp;
  part += idx * S * tile;
  apart += idx * S * wp;
  Pb += idx * CV_MAXW * CV_MAXW;
  for (int e = threadIdx.x; e < CV_MAXW * CV_MAXW; e += 256) {
    const int i = e >> 7, j = e & 127, hi = i > j ? i : j, lo = i > j ? j : i;
    double v = i == j ? 1.0 : 0.0;
    if (hi < w) {
      v = 0.0;
      for (int s = 0; s < S; ++s) v += part[s * tile + (long)hi * wp + lo];
    }
    Pb[e] = v;
  }
  if (threadIdx.x < CV_MAXW) {
    double v = 0.0;
    if ((int)threadIdx.x < w)
      for (int s = 0; s < S; ++s) v += apart[(long)s * wp + threadIdx.x];
    av[idx * CV_MAXW + threadIdx.x] = v;
  }
  if (threadIdx.x == 0) info[idx] = 0;
}

// grid = (folds of this pass, members), 256 threads.  X [member][fold][128][128] = M^-1 (lower, as potrf_diag_kernel leaves it; only the
// window's w x w corner is read), av = a_S.  t = X a_S (a wave per row), then thread (i, half) walks column i of X over every second
// row: r_i = sum_{k >= i} X_ki t_k and h_i = sum_{k >= i} X_ki^2 = [P_SS^-1]_ii, the two halves added in a fixed order.
// s = (q - t.t) / (n - w) (mode 0, "refit") or q / n (mode 1, "fixed"), q = y^T A~ read from *q.  out [member][4][ldo] as loo_rows_kernel's:
// mean, var, the nlpd term and the squared error of the SCORED rows [c0, c1) (every row belongs to exactly one fold).  A fold whose
// P_SS failed its pivot test (info != 0) leaves NaN rows and +inf terms.
__global__ __launch_bounds__(256) void cv_close_kernel(const double* __restrict__ X, const double* __restrict__ av, const int* __restrict__ info,
                                                       const double* __restrict__ y, long sY, const KParams* __restrict__ kps,
                                                       const double* __restrict__ q, long sQ, int mode, int n, int block, int gap, int f0,
                                                       double* __restrict__ out, long ldo, long sO) {
  __shared__ double sa[CV_MAXW], st[CV_MAXW], sr[2][CV_MAXW], sg[2][CV_MAXW], sh[4], s_tt;
  const long idx = (long)blockIdx.y * gridDim.x + blockIdx.x;
  X += idx * CV_MAXW * CV_MAXW;
  y += (long)(kps ? kps[blockIdx.y].ds : (int)blockIdx.y) * sY;
  out += (long)blockIdx.y * sO;
  const double qq = q[(long)blockIdx.y * sQ];
  int r0, r1, c0, c1;
  cv_window(n, block, gap, f0 + (int)blockIdx.x, r0, r1, c0, c1);
  const int w = r1 - r0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < CV_MAXW) sa[tid] = av[idx * CV_MAXW + tid];
  __syncthreads();
  for (int k = wave; k < w; k += 4) {
    double a = 0.0;
    for (int i = lane; i <= k; i += 64) a = fma(X[k * CV_MAXW + i], sa[i], a);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) st[k] = a;
  }
  __syncthreads();
  {
    const int i = tid & (CV_MAXW - 1), half = tid >> 7;
    double r = 0.0, g = 0.0;
    if (i < w)
      for (int k = i + half; k < w; k += 2) {
        const double x = X[k * CV_MAXW + i];
        r = fma(x, st[k], r);
        g = fma(x, x, g);
      }
    sr[half][i] = r; sg[half][i] = g;
  }
  const double tt = block_reduce_sum(tid < w ? st[tid] * st[tid] : 0.0, sh);
  if (tid == 0) s_tt = tt;
  __syncthreads();
  const int i = tid + c0 - r0;
  if (tid < c1 - c0) {
    const double r = sr[0][i] + sr[1][i], g = sg[0][i] + sg[1][i];
    const double s = mode == 0 ? (qq - s_tt) / (double)(n - w) : qq / (double)n;
    const double v = s * g;
    const bool bad = info[idx] != 0;
    const int gi = c0 + tid;
    out[gi] = bad ? __builtin_nan("") : y[gi] - r;
    out[ldo + gi] = bad ? __builtin_nan("") : v;
    out[2 * ldo + gi] = bad ? __builtin_huge_val() : 0.5 * log(2.0 * M_PI * v) + r * r / (2.0 * v);
    out[3 * ldo + gi] = bad ? __builtin_huge_val() : r * r;
  }
}

}  // namespace sigp
