// Kernels of the inducing-point (sparse) fit (sigp_sparse.inc; include/sigp.h: sigp_sparse_fit / sigp_sparse_predict).  fp64 throughout.
//   sparse_cross_kernel      k(Z, X_c) [m_pad][chunk]: rectangular covariance tiles from two row sources, distances in GEMM form
//   sparse_stats_kernel      b += V_c y_c, yy += y_c . y_c                                 (one wave per row, fixed order, no atomics)
//   sparse_trace_kernel      n - |V|_F^2 as the sum of the column deficits 1 - |V_c[:, j]|^2
//   sparse_assemble_kernel   B = sn~ I - N in place, identity on the padding
//   sparse_pred_kernel       q . w, q . q, p . p per test row
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"

namespace sigp {

// kb_gram_tile (kernels_misc.hpp) with separate sources for the tile's 64 rows (Xr, row tile bi) and its 128 columns (Xc, column tile bj):
// both are staged relative to the local origin x0 = row 64 bi of Xr, so the Gram form's error scales with the spread of the points, not
// with their offset, and the tile is translation-invariant.  Same LDS images ([64][DC + 2], [128][DC + 2], 16-byte aligned), the same
// column order sigma, the same accumulator layout: the squared distance of (row 16 wave + lr, column 16 t + 4 lq + c) is
// kb_gram_sq(acc[t][c], nI[16 wave + lr], nJ[16 t + 4 lq + c]).  Xr needs 64 (bi + 1) rows, Xc 128 (bj + 1) rows, dp >= (d + 3) & ~3.
template <int DC>
__device__ __forceinline__ void sparse_gram_tile(const double* Xr, const double* Xc, int dp, int d, int bi, int bj, double* Xi, double* Xj,
                                                 double* nI, double* nJ, d4 (&acc)[8]) {
  constexpr int LP = DC + 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int dq = (d + 3) & ~3;
  const double* x0 = Xr + (long)bi * KB_TM * dp;
  double sacc = 0.0;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
  const int sig = 4 * (lr & 3) + (lr >> 2);
  for (int p0 = 0; p0 < dq; p0 += DC) {
    const int pc = min(DC, dq - p0);
    const int h = pc >> 1, q = (tid % h) * 2, rstep = 256 / h;
    const d2 o = *(const d2*)(x0 + p0 + q);
    __syncthreads();
    if (tid < rstep * h) {
      for (int row = tid / h; row < KB_TM + KB_TN; row += rstep) {
        const double* src = row < KB_TM ? Xr + (long)(bi * KB_TM + row) * dp : Xc + (long)(bj * KB_TN + row - KB_TM) * dp;
        const d2 v = *(const d2*)(src + p0 + q);
        double* dst = row < KB_TM ? Xi + row * LP + q : Xj + (row - KB_TM) * LP + q;
        *(d2*)dst = v - o;
      }
    }
    __syncthreads();
    const double* bI = Xi + (16 * wave + lr) * LP + lq;
    const double* aJ = Xj + sig * LP + lq;
    for (int kk = 0; kk < pc; kk += 4) {
      const double b = bI[kk];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aJ[16 * t * LP + kk], b, acc[t], 0, 0, 0);
    }
    if (tid < KB_TM + KB_TN) {
      const double* xr = tid < KB_TM ? Xi + tid * LP : Xj + (tid - KB_TM) * LP;
      for (int p = 0; p < pc; p += 2) { const d2 u = *(const d2*)(xr + p); sacc = fma(u.x, u.x, sacc); sacc = fma(u.y, u.y, sacc); }
    }
  }
  if (tid < KB_TM) nI[tid] = sacc; else if (tid < KB_TM + KB_TN) nJ[tid - KB_TM] = sacc;
  __syncthreads();
}

// Kc [m_pad][ld] = k(Z, X_c): row i = inducing point i (Zs [m_pad][dp], zero padded), column j = row j of the staged chunk (Xc [ld][dp],
// zero padded); rows >= m and columns >= ncols are zero.  grid (ld / 128, m_pad / 64), 256 threads, one 64 x 128 tile per workgroup.
template <int DC>
__global__ __launch_bounds__(256) void sparse_cross_kernel(const double* __restrict__ Zs, const double* __restrict__ Xc, int dp, int d, int m,
                                                           int ncols, double* __restrict__ Kc, long ld, const KParams* __restrict__ kps) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  const KParams kp = kps[0];
  constexpr int LP = DC + 2;
  __shared__ __attribute__((aligned(16))) double Xi[KB_TM * LP];
  __shared__ __attribute__((aligned(16))) double Xj[KB_TN * LP];
  __shared__ __attribute__((aligned(16))) double nI[KB_TM], nJ[KB_TN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  d4 acc[8];
  sparse_gram_tile<DC>(Zs, Xc, dp, d, bi, bj, Xi, Xj, nI, nJ, acc);
  const int gi = bi * KB_TM + 16 * wave + lr;
  const double ni = nI[16 * wave + lr];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int gj = bj * KB_TN + 16 * t + 4 * lq;
    const d2 nj01 = *(const d2*)(nJ + 16 * t + 4 * lq), nj23 = *(const d2*)(nJ + 16 * t + 4 * lq + 2);
    const double njv[4] = {nj01.x, nj01.y, nj23.x, nj23.y};
    KbOut4<double> o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o.v[c] = (gi < m && gj + c < ncols) ? cov_from_sq(kp, kb_gram_sq(acc[t][c], ni, njv[c])) : 0.0;
    *(KbOut4<double>*)(Kc + (long)gi * ld + gj) = o;
  }
}

// One wave per row r of V_c [rows][ld] (rows a multiple of 4; columns 0 .. ncols_pad - 1, zero past the chunk's data):
//   bvec[r] += V_c[r] . y_c
// and one more workgroup whose first wave adds y_c . y_c to *yy.  Every entry has ONE writer and the chunks arrive in stream order: one
// chain of additions per entry, the same bits on every run.  grid = rows / 4 + 1 workgroups of 256 threads.
__global__ __launch_bounds__(256) void sparse_stats_kernel(const double* __restrict__ V, long ld, int rows, int ncols_pad, const double* __restrict__ y,
                                                           double* __restrict__ bvec, double* __restrict__ yy) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  double a = 0.0;
  if (r < rows) {
    const double* v = V + (long)r * ld;
    for (int j = lane; j < ncols_pad; j += 64) a = fma(v[j], y[j], a);
  } else if (r == rows) {
    for (int j = lane; j < ncols_pad; j += 64) { const double x = y[j]; a = fma(x, x, a); }
  } else {
    return;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if (lane != 0) return;
  if (r < rows) bvec[r] += a; else *yy += a;
}

// The trace term n - |V|_F^2 of the collapsed bound, accumulated as what it is -- the sum over the data points of k(x_j, x_j) - q_jj =
// 1 - |V_c[:, j]|^2 -- instead of as the difference of two numbers of size n: where the inducing points explain the data, every deficit is
// small and carries the absolute error of ONE column norm near 1 (about u), while n - t would carry ulp(n) per addition.  A workgroup owns
// 64 columns; wave w sums the squares of rows w, w + 4, ... (ascending), the four partial norms are added in wave order, and the 64
// deficits by a shuffle tree: dpart[blockIdx.x] += their sum (one writer per entry, chunks in stream order).  Columns >= ncols (padding)
// contribute nothing.  grid = ceil(ncols / 64) workgroups of 256 threads.
__global__ __launch_bounds__(256) void sparse_trace_kernel(const double* __restrict__ V, long ld, int rows, int ncols, double* __restrict__ dpart) {
  __shared__ double sh[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (j < ncols)
    for (int r = wave; r < rows; r += 4) { const double v = V[(long)r * ld + j]; s = fma(v, v, s); }
  sh[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  double dfc = j < ncols ? fmax(1.0 - (((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane]), 0.0) : 0.0;   // (a deficit is >= 0: clamped like the squared distances)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dfc += __shfl_down(dfc, off, 64);
  if (lane == 0) dpart[blockIdx.x] += dfc;
}

// Bm [m_pad][ld] holds N = -sum_c V_c V_c^T on its lower 128-tiles: B = sn~ I - N in place, the identity on the padding rows / columns.
// (Entries above the diagonal inside the diagonal tiles are never read by the factorisation.)
__global__ void sparse_assemble_kernel(double* __restrict__ Bm, long ld, int m, int m_pad, double sn) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)m_pad * m_pad) return;
  const int i = (int)(idx / m_pad), j = (int)(idx % m_pad);
  if (j > i) return;
  double* p = Bm + (long)i * ld + j;
  if (i < m) *p = (i == j ? sn : 0.0) - *p;
  else *p = (i == j) ? 1.0 : 0.0;
}

// Per test row r of chunk blockIdx.y (P, Q [chunks][128][ld]: p = L^-1 k(Z, x*), q = L_B^-1 p as rows; w [ncol]):
//   res[r] = q . w    res[128 + r] = q . q    res[256 + r] = p . p        (res += 512 blockIdx.y)
__global__ __launch_bounds__(256) void sparse_pred_kernel(const double* __restrict__ P, const double* __restrict__ Q, long ld, int ncol,
                                                          const double* __restrict__ w, double* __restrict__ res) {
  __shared__ double sh[4];
  const int r = blockIdx.x;
  const double* p = P + ((long)blockIdx.y * 128 + r) * ld;
  const double* q = Q + ((long)blockIdx.y * 128 + r) * ld;
  res += blockIdx.y * 512;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < ncol; i += 256) {
    const double qi = q[i], pi = p[i];
    a = fma(qi, w[i], a); b = fma(qi, qi, b); c = fma(pi, pi, c);
  }
  a = block_reduce_sum(a, sh);
  b = block_reduce_sum(b, sh);
  c = block_reduce_sum(c, sh);
  if (threadIdx.x == 0) { res[r] = a; res[128 + r] = b; res[256 + r] = c; }
}

}  // namespace sigp
