// Exact gradients of the leave-block-out scores with respect to d per-feature (ARD) length scales (sigp_cv_grad_ard, driver:
// sigp_cvard.inc): the adjoint form of looard.hpp with a BLOCK in place of the diagonal.  Notation of blockcv.hpp: P = K~^-1, a = P y,
// q = y^T a; fold f removes the window S (w rows) and scores C within it; Q = P_SS, H = Q^-1, r = H a_S, s = (q - a_S^T r)/(n - w) ("refit")
// or q/n ("fixed"), var_i = s H_ii (i in C).  The score depends on the direction D = dK~/dtheta only through b = P D a, e = a^T D a and
// the blocks (P D P)_SS, linearly, so the chain rule transposes into one symmetric adjoint that does not depend on the direction:
//     d score = sum_ij G_ij D_ij,     G = 1/2 (v a^T + a v^T) + P B P + eps a a^T,     v = P beta,
//     beta = sum_f E_f beta_f,   B = sum_f E_f B_f E_f^T,   eps = sum_f eps_f         (E_f places the window's rows in 0 .. n)
// With rbar_i = r_i/var_i, kappa_i = 1/(2 var_i) - r_i^2/(2 var_i^2) (nlpd) or rbar_i = 2 r_i, kappa_i = 0 (sse) on C and zero outside,
// t = H rbar and sbar = sum_{i in C} kappa_i H_ii:
//     beta_f = -t                                    [+ refit: 2 sbar r / (n - w)]
//     B_f    = 1/2 (t r^T + r t^T) + s H diag(kappa) H   [- refit: sbar r r^T / (n - w)]
//     eps_f  = -sbar / (n - w)  [refit]   or   -sbar / n  [fixed]
// B is symmetric, block diagonal for gap = 0 and banded with |i - j| < 128 otherwise; block = 1, gap = 0 gives diag(gamma), beta and eps of
// looard.hpp.  The derivatives are then looard.hpp's contraction, by the same kernels (ard_grad_partial_kernel<., ARD_W_LOO>,
// loo_ard_finish_kernel) over M = P B P, v, a, eps.  What is new on the device:
//   cv_adj_fold_kernel       (fold): beta_f, B_f (at the window's own size), eps_f from X = M^-1 (Q = M M^T, H = X^T X), a_S and q --
//                            inside cv_launch's pass loop, right after cv_close_kernel; the two products on the fp64 matrix pipe
//   cv_adj_gather_kernel     (row of the band store): every entry of beta and B adds its folds' terms in ascending fold order
//   cv_adj_eps_kernel        eps = the fold terms in ascending order
//   cv_adj_v_kernel          v = P beta, one wave per row of P; rows and columns n .. n_pad of P are zeroed on the way
//   cv_band_product_kernel   P B into a full n_pad x n_pad matrix: the trailing update's 128-tile loop over the K window of the three block
//                            columns in which B's block row is not zero (6 x 128 n_pad^2 flops)
// B lives in a band store: row i holds the three 128-column blocks around its own, [n_pad][384].  Rows and columns n .. n_pad of every
// operand are masked.  No atomics anywhere: the same bits on every run.
// Lockstep members (sigp_cv_grad_ard_batch): every kernel below takes the member from a grid dimension and adds the member's offsets -- P and
// P B n_pad^2 apart, the band stores n_pad x 384 apart, the vectors LooArdGroupVecs::mstride() apart, eps_f F apart, q in the slot's result
// rows -- to its pointers before anything is read: uniform values, no vector register, and a member executes the instructions a single fit
// does.  B_f and beta_f lie at the (member, fold) pair index of cv_strip_finish_kernel and cv_close_kernel.  The single fit launches one
// member with zero strides.
#pragma once
#include <hip/hip_runtime.h>

#include "blockcv.hpp"
#include "score_layout.hpp"
#include "syrk128.hpp"

namespace sigp {

constexpr int CVA_BAND = 3 * SY_T;     // columns of a row of the band store
static_assert(CVA_BAND == SL_BAND && CV_MAXW == SL_BLK, "score_layout.hpp lays the band store and the fold blocks out for these");

// What cv_launch does for the gradient when it is given a CvAdjoint (sigp_cv_grad_ard; score_layout.hpp): the fold adjoints of each pass and
// their assembly.

// the first and the last fold whose window holds row x
__device__ __forceinline__ int cva_first_fold(int x, int block, int gap) { return x >= gap ? (x - gap) / block : 0; }
__device__ __forceinline__ int cva_last_fold(int x, int block, int gap, int F) { const int f = (x + gap) / block; return f < F ? f : F - 1; }

// grid = (folds of this pass, members), 256 threads, dynamic LDS = wp * mp doubles (wp / mp: the widest window / scored block of the launch rounded up
// to 16).  X [pair][128][128] = M^-1 (lower; only the window's w x w corner is read, by SELECT), av [pair][128] = a_S, q = y^T A~ from
// q[member * sQ]; B_f and beta_f at the pair index, eps_f at [member * sE][fold].
//   t0 = X a_S, r = X^T t0, g_i = H_ii = sum_k X_ki^2, s, var, kappa, rbar, sbar        as cv_close_kernel forms them
//   Hc = X^T X[:, C]          [w][m] into LDS: subtile (ti, tj) by one wave, D = A B^T with A = columns 16 ti .. of X, B = columns
//                             c0 - r0 + 16 tj .. of X, K = the window's rows from 16 ti on
//   t = Hc rbar_C;  beta_f;  eps_f
//   B_f = 1/2 (t r^T + r t^T) + Hc diag(s kappa_C) Hc^T - [refit] sbar r r^T / (n - w)    lower subtiles, K = the scored rows
// A lane's accumulator register e is row lq + 4 e, column lr of the subtile (Num<double>::drow).  Rows beyond the window give zeros.
__global__ __launch_bounds__(256) void cv_adj_fold_kernel(const double* __restrict__ X, const double* __restrict__ av, const double* __restrict__ q,
                                                          int mode, int crit, int n, int block, int gap, int f0, int wp, int mp,
                                                          double* __restrict__ Bf, double* __restrict__ betaf, double* __restrict__ epsf, long sQ = 0,
                                                          long sE = 0) {
  extern __shared__ __attribute__((aligned(16))) double Hc[];       // [wp][mp]
  __shared__ double sa[CV_MAXW], st[CV_MAXW], sr[CV_MAXW], sg[CV_MAXW], srb[CV_MAXW], ssk[CV_MAXW], stt[CV_MAXW], sh[4], s_sc[2];
  const long idx = (long)blockIdx.y * gridDim.x + blockIdx.x;
  X += idx * CV_MAXW * CV_MAXW;
  av += idx * CV_MAXW;
  Bf += idx * (long)wp * wp;
  betaf += idx * wp;
  epsf += (long)blockIdx.y * sE;
  const double qq = q[(long)blockIdx.y * sQ];
  int r0, r1, c0, c1;
  cv_window(n, block, gap, f0 + (int)blockIdx.x, r0, r1, c0, c1);
  const int w = r1 - r0, m = c1 - c0, cl = c0 - r0;
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = (w + 15) >> 4, mt = (m + 15) >> 4;
  if (tid < CV_MAXW) {
    sa[tid] = av[tid];
    st[tid] = 0.0; srb[tid] = 0.0; ssk[tid] = 0.0;
  }
  __syncthreads();
  for (int k = wave; k < w; k += 4) {
    double a = 0.0;
    for (int i = lane; i <= k; i += 64) a = fma(X[k * CV_MAXW + i], sa[i], a);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) st[k] = a;
  }
  __syncthreads();
  if (tid < CV_MAXW) {
    double r = 0.0, g = 0.0;
    if (tid < w)
      for (int k = tid; k < w; ++k) {
        const double x = X[k * CV_MAXW + tid];
        r = fma(x, st[k], r);
        g = fma(x, x, g);
      }
    sr[tid] = r; sg[tid] = g;
  }
  const double tt = block_reduce_sum(tid < w ? st[tid] * st[tid] : 0.0, sh);
  if (tid == 0) s_sc[0] = mode == 0 ? (qq - tt) / (double)(n - w) : qq / (double)n;
  __syncthreads();
  const double s = s_sc[0];
  double kg = 0.0;
  if (tid < m) {
    const double r = sr[cl + tid], g = sg[cl + tid];
    if (crit == 0) {
      const double var = s * g;
      const double kappa = 1.0 / (2.0 * var) - r * r / (2.0 * var * var);
      srb[tid] = r / var;
      ssk[tid] = s * kappa;
      kg = kappa * g;
    } else {
      srb[tid] = 2.0 * r;
    }
  }
  const double sb = block_reduce_sum(kg, sh);
  if (tid == 0) s_sc[1] = sb;

  // Hc = X^T X[:, C]
  for (int p = wave; p < nt * mt; p += 4) {
    const int ti = p / mt, tj = p - ti * mt;
    const int i = 16 * ti + lr, cj = 16 * tj + lr, c = cl + cj;
    const bool iin = i < w, cin = cj < m;
    const int ci = cin ? c : 0;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kk = 16 * ti; kk < 16 * nt; kk += 4) {
      const int k = kk + lq;
      const double a = (iin && k < w && k >= i) ? X[k * CV_MAXW + i] : 0.0;
      const double b = (cin && k < w && k >= c) ? X[k * CV_MAXW + ci] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) Hc[(16 * ti + Num<double>::drow(lq, e)) * mp + 16 * tj + lr] = acc[e];
  }
  __syncthreads();
  const double sbar = s_sc[1];
  const double rf = mode == 0 ? 1.0 / (double)(n - w) : 0.0;
  if (tid < CV_MAXW) {
    double t = 0.0;
    if (tid < w)
      for (int c = 0; c < m; ++c) t = fma(Hc[tid * mp + c], srb[c], t);
    stt[tid] = t;
    if (tid < wp) betaf[tid] = tid < w ? -t + 2.0 * sbar * rf * sr[tid] : 0.0;
  }
  if (tid == 0) epsf[f0 + (int)blockIdx.x] = crit == 0 ? -sbar / (mode == 0 ? (double)(n - w) : (double)n) : 0.0;
  __syncthreads();

  // B_f, lower subtiles
  for (int p = wave; p < nt * (nt + 1) / 2; p += 4) {
    int ti = 0, tj = p;
    while (tj > ti) { tj -= ti + 1; ++ti; }
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (crit == 0)
      for (int kk = 0; kk < 16 * mt; kk += 4) {
        const int c = kk + lq;
        const double a = Hc[(16 * ti + lr) * mp + c] * ssk[c];
        const double b = Hc[(16 * tj + lr) * mp + c];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 16 * ti + Num<double>::drow(lq, e), j = 16 * tj + lr;
      Bf[(long)i * wp + j] = acc[e] + 0.5 * (stt[i] * sr[j] + sr[i] * stt[j]) - sbar * rf * sr[i] * sr[j];
    }
  }
}

// grid = (the rows [row0, row0 + gridDim.x) that the folds [f0, f0 + nf) of this pass touch, members), 128 threads; the member's B_f and
// beta_f of the pass begin at pair member * nf, its band store and beta at member * sBand and member * sBeta.  Entry (i, j) of B (band column
// jj = j - 128 (i / 128 - 1)) adds B_f[i - r0_f][j - r0_f], read from the computed lower triangle at (max, min), of every fold of the pass whose
// window holds both rows, in ascending fold order, to what the earlier passes left there; beta_i likewise: one chain of additions from
// zero in ascending fold order however the folds are split into passes, so the split does not show in the bits.  Rows and columns from n
// on stay zero.
__global__ __launch_bounds__(128) void cv_adj_gather_kernel(const double* __restrict__ Bf, const double* __restrict__ betaf, int wp, int n, int block,
                                                            int gap, int F, int f0, int nf, int row0, double* __restrict__ band,
                                                            double* __restrict__ beta, long sBand = 0, long sBeta = 0) {
  {
    const long mb = blockIdx.y;
    Bf += mb * nf * wp * wp; betaf += mb * nf * wp; band += mb * sBand; beta += mb * sBeta;
  }
  const int i = row0 + (int)blockIdx.x;
  if (i >= n) return;
  const int jb = (i / SY_T - 1) * SY_T;
  const int fl_i = cva_first_fold(i, block, gap), fh_i = cva_last_fold(i, block, gap, F);
  const int flast = f0 + nf - 1;
  for (int jj = threadIdx.x; jj < CVA_BAND; jj += 128) {
    const int j = jb + jj;
    if (j < 0 || j >= n) continue;
    int fa = j > i ? cva_first_fold(j, block, gap) : fl_i, fb = j < i ? cva_last_fold(j, block, gap, F) : fh_i;
    fa = fa > f0 ? fa : f0;
    fb = fb < flast ? fb : flast;
    if (fa > fb) continue;
    double acc = band[(long)i * CVA_BAND + jj];
    for (int f = fa; f <= fb; ++f) {
      int r0, r1, c0, c1;
      cv_window(n, block, gap, f, r0, r1, c0, c1);
      if (i < r0 || i >= r1 || j < r0 || j >= r1) continue;
      const int li = i - r0, lj = j - r0, hi = li > lj ? li : lj, lo = li > lj ? lj : li;
      acc += Bf[(long)(f - f0) * wp * wp + (long)hi * wp + lo];
    }
    band[(long)i * CVA_BAND + jj] = acc;
  }
  if (threadIdx.x == 0) {
    const int fa = fl_i > f0 ? fl_i : f0, fb = fh_i < flast ? fh_i : flast;
    double acc = beta[i];
    for (int f = fa; f <= fb; ++f) {
      int r0, r1, c0, c1;
      cv_window(n, block, gap, f, r0, r1, c0, c1);
      if (i >= r0 && i < r1) acc += betaf[(long)(f - f0) * wp + (i - r0)];
    }
    beta[i] = acc;
  }
}

// one block per member: eps = epsf[0] + epsf[1] + ..  in that order (chunks of 256 through LDS, added by thread 0)
__global__ __launch_bounds__(256) void cv_adj_eps_kernel(const double* __restrict__ epsf, int F, double* __restrict__ eps, long sE = 0, long sW = 0) {
  __shared__ double sh[256];
  epsf += (long)blockIdx.x * sE;
  eps += (long)blockIdx.x * sW;
  double acc = 0.0;
  for (int f0 = 0; f0 < F; f0 += 256) {
    __syncthreads();
    sh[threadIdx.x] = f0 + (int)threadIdx.x < F ? epsf[f0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = F - f0 < 256 ? F - f0 : 256;
      for (int k = 0; k < m; ++k) acc += sh[k];
    }
  }
  if (threadIdx.x == 0) eps[0] = acc;
}

// One WAVE per row i < n_pad of the full P:  v_i = sum_{k < n} P_ik beta_k (zero for i >= n), and the entries of P in rows or columns
// n .. n_pad are set to zero, so that the two products that follow see masked operands.  blockIdx.y = lockstep member.
__global__ __launch_bounds__(256) void cv_adj_v_kernel(double* __restrict__ P, long ld, int n, int n_pad, const double* __restrict__ beta, double* __restrict__ v,
                                                       long sP = 0, long sW = 0) {
  {
    const long mb = blockIdx.y;
    P += mb * sP; beta += mb * sW; v += mb * sW;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n_pad) return;
  double* row = P + (long)i * ld;
  double acc = 0.0;
  for (int k0 = 0; k0 < n_pad; k0 += 128) {
    const int k = k0 + lane * 2;
    const d2 p = *(const d2*)(row + k);
    const d2 bv = *(const d2*)(beta + k);
    d2 o;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool in = i < n && k + e < n;
      o[e] = in ? p[e] : 0.0;
      acc = fma(o[e], in ? bv[e] : 0.0, acc);
    }
    if (i >= n || k + 2 > n) *(d2*)(row + k) = o;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) v[i] = acc;
}

// grid = (T, T) tiles (bj, bi) of C = P B, every one written whole.  Tile (bi, bj) = rows bi of P against rows bj of the band store (B is
// symmetric: its rows are its columns) over the block columns k0 = max(bj - 1, 0) .. min(bj + 2, T) of P, which are the band columns from
// 128 (k0 - bj + 1) on.  The tile loop is syrk128_tile's SET form: LDS-DMA staging, two-buffer pipeline, v_mfma_f64_16x16x4_f64; 64 KiB of
// LDS, two workgroups per CU, as syrk128_kernel.  blockIdx.z = lockstep member.
__global__ __launch_bounds__(256, 2) void cv_band_product_kernel(const double* __restrict__ P, long ldp, const double* __restrict__ band, double* __restrict__ C,
                                                                 long ldc, int T, long sP = 0, long sBand = 0) {
  constexpr int KTe = Num<double>::KT;
  {
    const long mb = blockIdx.z;
    P += mb * sP; band += mb * sBand; C += mb * sP;
  }
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* As = (double*)smem_raw;        // [2][128][KT]
  double* Bs = As + 2 * SY_T * KTe;      // [2][128][KT]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int bj = (int)blockIdx.x, bi = (int)blockIdx.y;
  const int k0 = bj > 0 ? bj - 1 : 0, k1 = bj + 2 < T ? bj + 2 : T;
  const double* Ag = P + (long)bi * SY_T * ldp + (long)k0 * SY_T;
  const double* Bg = band + (long)bj * SY_T * CVA_BAND + (long)(k0 - bj + 1) * SY_T;
  double* Cw = C + ((long)bi * SY_T + wm * 64) * ldc + (long)bj * SY_T + wn * 64;
  unsigned long long ph0 = 0, ph1 = 0;
  syrk128_tile<double, true>(Ag, ldp, Bg, (long)CVA_BAND, Cw, ldc, (k1 - k0) * SY_T, 0, As, Bs, false, ph0, ph1);
}

}  // namespace sigp
