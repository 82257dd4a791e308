// Exact gradients of the leave-one-out scores (sigp_loo_grad / sigp_loo_grad_batch; Rasmussen & Williams 5.4.2).  With P = K~^-1 (full,
// symmetric), a = P y, g_i = P_ii, r_i = a_i / g_i, var_i = s_i / g_i and, for a hyper-parameter with D = dK~/dtheta (symmetric),
//     t = D a,  b = P t,  e = a^T t,  c_i = [P D P]_ii
// the per-point chain rule is
//     dr_i = -b_i / g_i + a_i c_i / g_i^2
//     ds_i = -e / n  (fixed)   or   (-e + 2 a_i b_i / g_i - a_i^2 c_i / g_i^2) / (n - 1)  (refit)
//     dvar_i = ds_i / g_i + s_i c_i / g_i^2
//     d nlpd = sum_i dvar_i / (2 var_i) + r_i dr_i / var_i - r_i^2 dvar_i / (2 var_i^2)          d sse = sum_i 2 r_i dr_i
// The one cubic quantity is c.  With D' = D above its diagonal, half of D on it and zero below (so D = D' + D'^T), c_i = 2 sum_b W'_bi P_bi
// for W' = D' P: rows of D' are zero left of their diagonal, so the 128-tile product skips the K blocks left of the row block
// (GemmArgsT::ktri = 1 on the full tile space of syrk128_kernel's SET form): n^3 flops instead of the 2 n^3 of D P.
// The noise parameter has D = sn~ I, nothing cubic: the kernels below work with D = I (t = a, b = P a, e = a^T a, c_i = sum_k P_ik^2) and the
// host multiplies by sn~.  Everything is linear in D, so a constant factor of D (the reference kernel's l) is applied on the host as well.
// Rows and columns n .. n_pad of every operand are masked: the padding contributes nothing.  No atomics anywhere: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"
#include "score_layout.hpp"

namespace sigp {

// The per-member vector workspace of the gradient pass, LooGradVecs: score_layout.hpp.

// P (the lower 128-tiles of U U^T) -> full symmetric: every element above the diagonal is its mirror image.  Grid (n_pad / 32, n_pad / 32,
// member), 32 x 32 tiles through LDS so that both sides are coalesced; tile (bi, bj) with bi <= bj is written from tile (bj, bi).
__global__ __launch_bounds__(256) void loo_grad_mirror_kernel(double* __restrict__ P, long ld, long sP) {
  __shared__ double tile[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  P += (long)blockIdx.z * sP;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) tile[r][tx] = P[(long)(bj * 32 + r) * ld + bi * 32 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (bi < bj || tx > r) P[(long)(bi * 32 + r) * ld + bj * 32 + tx] = tile[tx][r];
}

// One WAVE per row i of D (full symmetric as the builds leave it): t_i = sum_{k < n} D_ik a_k from the whole row, then the row is rewritten
// as row i of D': zero left of the diagonal, half the diagonal entry, zero from column n on; rows n .. n_pad are zeroed.  A wave touches its
// own row only.  blockIdx.y = member.
// tri = 0 (A/B timing of the full product): only the padding is zeroed, the row stays whole.
__global__ __launch_bounds__(256) void loo_grad_prep_kernel(double* __restrict__ D, long ld, long sD, int n, int n_pad, int tri, LooGradVecs v) {
  const int m = blockIdx.y;
  D += (long)m * sD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n_pad) return;
  const double* a = v.a(m);
  double* row = D + (long)i * ld;
  double acc = 0.0;
  for (int k0 = 0; k0 < n_pad; k0 += 128) {
    const int k = k0 + lane * 2;
    d2 dv = *(const d2*)(row + k);
    const d2 av = *(const d2*)(a + k);
    d2 o;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool in = i < n && k + e < n;
      acc = fma(in ? dv[e] : 0.0, in ? av[e] : 0.0, acc);
      o[e] = !in ? 0.0 : !tri ? dv[e] : k + e > i ? dv[e] : k + e == i ? 0.5 * dv[e] : 0.0;
    }
    *(d2*)(row + k) = o;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) v.t(m)[i] = acc;
}

// One WAVE per training point i over row i of the full P, columns < n:  b_i = sum_k P_ik t_k,  (P a)_i,  sum_k P_ik^2.
__global__ __launch_bounds__(256) void loo_grad_rows_kernel(const double* __restrict__ P, long ld, long sP, int n, LooGradVecs v) {
  const int m = blockIdx.y;
  P += (long)m * sP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;
  const double* a = v.a(m);
  const double* t = v.t(m);
  const double* row = P + (long)i * ld;
  double sb = 0.0, sa = 0.0, sp = 0.0;
  for (int k0 = 0; k0 < n; k0 += 128) {
    const int k = k0 + lane * 2;
    if (k >= n) continue;
    const d2 p = *(const d2*)(row + k);
    const d2 tv = *(const d2*)(t + k);
    const d2 av = *(const d2*)(a + k);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool in = k + e < n;
      const double pe = in ? p[e] : 0.0;
      sb = fma(pe, in ? tv[e] : 0.0, sb);
      sa = fma(pe, in ? av[e] : 0.0, sa);
      sp = fma(pe, pe, sp);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sb += __shfl_down(sb, off, 64); sa += __shfl_down(sa, off, 64); sp += __shfl_down(sp, off, 64); }
  if (lane == 0) { v.b(m)[i] = sb; v.pa(m)[i] = sa; v.pp(m)[i] = sp; }
}

// Column sums of W' o P by row chunks: grid (n_pad / 128 column blocks, n_pad / 128 row chunks, member); wave w adds rows w, w + 4, .. of the
// chunk (rows < n) for the block's 128 columns, two per lane, and the four waves' sums meet in LDS in a fixed order:
//     cpart[chunk][i] = sum_{b in chunk, b < n} W'_bi P_bi
__global__ __launch_bounds__(256) void loo_grad_cols_kernel(const double* __restrict__ W, const double* __restrict__ P, long ld, long sM, int n, LooGradVecs v) {
  __shared__ double sh[4][128];
  const int m = blockIdx.z;
  W += (long)m * sM; P += (long)m * sM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 128 + lane * 2;
  const int r0 = blockIdx.y * 128;
  double acc0 = 0.0, acc1 = 0.0;
  for (int r = r0 + wave; r < min(n, r0 + 128); r += 4) {
    const d2 w = *(const d2*)(W + (long)r * ld + col);
    const d2 p = *(const d2*)(P + (long)r * ld + col);
    acc0 = fma(w[0], p[0], acc0);
    acc1 = fma(w[1], p[1], acc1);
  }
  sh[wave][lane * 2] = acc0; sh[wave][lane * 2 + 1] = acc1;
  __syncthreads();
  if (threadIdx.x < 128)
    v.cpart(m)[(long)blockIdx.y * v.n_pad + blockIdx.x * 128 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// The chain rule per point and the fixed-order sums, one block per member.  out [4] = d nlpd / d(theta_1, theta_2), d sse / d(theta_1, theta_2)
// for D_1 = the matrix the prep pass saw and D_2 = I.  g_i is the diagonal of P; s_i and var_i are formed as loo_rows_kernel forms them
// (mode 0 "refit", 1 "fixed"; q = y^T A~ from *q).  cfac = 2 for the triangular product (c = 2 colsum(W' o P)), 1 for the full one.
__global__ __launch_bounds__(256) void loo_grad_point_kernel(const double* __restrict__ P, long ld, long sP, int n, const double* __restrict__ q, long sQ, int mode,
                                                             double cfac, LooGradVecs v) {
  __shared__ double sh[4];
  __shared__ double ee[2];
  const int m = blockIdx.x;
  P += (long)m * sP;
  const double* a = v.a(m);
  const double* t = v.t(m);
  const double* b1 = v.b(m);
  const double* pa = v.pa(m);
  const double* pp = v.pp(m);
  const double* cp = v.cpart(m);
  double e1 = 0.0, e2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { e1 = fma(a[i], t[i], e1); e2 = fma(a[i], a[i], e2); }
  e1 = block_reduce_sum(e1, sh);
  e2 = block_reduce_sum(e2, sh);
  if (threadIdx.x == 0) { ee[0] = e1; ee[1] = e2; }
  __syncthreads();
  const double qq = q[(long)m * sQ];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const double g = P[(long)i * ld + i], ai = a[i];
    const double r = ai / g;
    const double s = mode == 0 ? (qq - ai * r) / (double)(n - 1) : qq / (double)n;
    const double var = s / g;
    double c1 = 0.0;
    for (int k = 0; k < v.T; ++k) c1 += cp[(long)k * v.n_pad + i];
    const double c[2] = {cfac * c1, pp[i]}, b[2] = {b1[i], pa[i]};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const double dr = -b[p] / g + ai * c[p] / (g * g);
      const double ds = mode == 0 ? (-ee[p] + 2.0 * ai * b[p] / g - ai * ai * c[p] / (g * g)) / (double)(n - 1) : -ee[p] / (double)n;
      const double dvar = ds / g + s * c[p] / (g * g);
      acc[p] += dvar / (2.0 * var) + r * dr / var - r * r * dvar / (2.0 * var * var);
      acc[2 + p] += 2.0 * r * dr;
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double s = block_reduce_sum(acc[p], sh);
    if (threadIdx.x == 0) v.out(m)[p] = s;
  }
}

}  // namespace sigp
