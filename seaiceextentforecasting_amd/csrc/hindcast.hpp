// Expanding-window (rolling-origin) hindcast validation from ONE fit (sigp_hindcast, sigp_hindcast_batch, sigp_hindcast_grad_ard and, for
// lockstep groups, sigp_hindcast_grad_ard_batch; drivers: sigp_hindcast.inc, sigp_hindcastbatch.inc).  Rows are in time order, 0-based.
// Row t is scored when s = t - lead + 1 >= min_train; its training set is rows [0, s).
// The Cholesky factor of the first s rows is the leading s x s block of L = L~, and z = L^-1 y restricted to its first s entries is that
// prefix's solved vector, so with the hyper-parameters held every origin's forecast is read out of the factor and the solved ride row:
//     r_t = y_t - mean_t = sum_{j=s..t} L_tj z_j        w_t = sum_{j=s..t} L_tj^2        var_t = sigma_t w_t  (with the noise, like fvar)
//     sigma_t = (sum_{j<s} z_j^2) / s  (mode 0, "refit": sigma_f profiled on the training rows alone)   or   q / n  (mode 1, "fixed")
//     nlpd = sum_t log(2 pi var_t)/2 + r_t^2/(2 var_t),   sse = sum_t r_t^2    over the scored rows
// No L~^-T is needed for the values.  The gradient is one symmetric adjoint G = d score / d K~ (reverse-mode Cholesky):
//     kappa_t = 1/(2 var_t) - r_t^2/(2 var_t^2), rho_t = r_t/var_t  (nlpd);   kappa_t = 0, rho_t = 2 r_t  (sse)
//     B_tj = rho_t z_j + 2 kappa_t sigma_t L_tj   for s_t <= j <= t  (a band of width lead; zero in unscored rows)
//     zbar_j = sum_{t: s_t <= j <= t} rho_t L_tj + 2 z_j sum_{t: s_t > j} kappa_t w_t / s_t     (fixed: 2 z_j (sum_t kappa_t w_t) / n)
//     A = L^T B - zbar z^T on its lower triangle;  C_ij = C_ji = A_ij / 2 (i >= j);  G = U C U^T,  U = L^-T
//     d score / d log l_k = sum_ij G_ij h_ij (u_ik - u_jk)^2  (ard_grad_partial_kernel<., ARD_W_LOO> with M = G, v = 0, eps = 0),  d / d log sn~ = sn~ tr G
// The lower triangle of L^T B is banded: (L^T B)_ij = sum_{k=i..j+lead-1} L_ki B_kj for 0 <= i - j < lead, and B is never stored: an entry of
// C forms the terms of B it needs from rho, kappa sigma, z and L.  W = U C needs no cubic product: the banded part of C is a banded product
// and its rank-one part two scans along each row of U (hindcast_w_kernel; lockstep groups: hindcast_w_lds_kernel).  The one cubic step
// beyond U is G = U W^T on syrk128_kernel's SET form (sigp_hindcast.inc).  Rows and columns n .. n_pad of Cb and W are zero.  No atomics anywhere: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"
#include "score_layout.hpp"

namespace sigp {

// member strides of the kernels below (doubles): L and its ride row z alike; q: the slot's result rows (512 apart); v: HindcastVecs; C: U, Cb and W alike
struct HindcastStrides { long L, q, v, C; };

// Exclusive scan of f(p), p = 0 .. n - 1, by one block of 256 threads in a fixed order: thread t owns the chunk [t c, (t + 1) c), c = ceil(n / 256);
// it adds its chunk, then the totals of the threads before it in ascending order, and calls put(p, sum of f before p, f(p)) along its chunk.
template <typename F, typename P>
__device__ __forceinline__ void hc_block_scan(int n, double* tot /* [256] LDS */, F f, P put) {
  const int c = (n + 255) / 256, p0 = (int)threadIdx.x * c, p1 = min(n, p0 + c);
  double s = 0.0;
  for (int p = p0; p < p1; ++p) s += f(p);
  tot[threadIdx.x] = s;
  __syncthreads();
  double run = 0.0;
  for (int u = 0; u < (int)threadIdx.x; ++u) run += tot[u];
  for (int p = p0; p < p1; ++p) { const double v = f(p); put(p, run, v); run += v; }
}

// cum[j] = sum_{i < j} z_i^2, j < n.  blockIdx.x = lockstep member.
__global__ __launch_bounds__(256) void hindcast_scan_kernel(const double* __restrict__ z, int n, HindcastVecs hv, HindcastStrides ms) {
  __shared__ double tot[256];
  z += (long)blockIdx.x * ms.L; hv.base += (long)blockIdx.x * ms.v;
  double* cum = hv.cum();
  hc_block_scan(n, tot, [&](int p) { return z[p] * z[p]; }, [&](int p, double before, double) { cum[p] = before; });
}

// One WAVE per row t < n: the contiguous segments L[t, s..t] and z[s..t] (at most 128 entries: two per lane), added across the lanes in a fixed
// order; lane 0 closes the row.  out [member][4][ldo] as loo_rows_kernel's: mean, var, the row's nlpd term, its squared error (loo_sum_kernel
// adds the terms); an unscored row gets NaN, NaN and two zeros.  rw = 1: r_t and w_t (zero when unscored) into hv for the gradient.
// blockIdx.y = lockstep member (its y is data set kps[member].ds of stride sY).
__global__ __launch_bounds__(256) void hindcast_rows_kernel(const double* __restrict__ L, long ld, int n, const double* __restrict__ z, const double* __restrict__ y,
                                                            const double* __restrict__ q, int lead, int min_train, int mode, double* __restrict__ out, long ldo,
                                                            HindcastVecs hv, int rw, HindcastStrides ms, long sY, long sO, const KParams* __restrict__ kps) {
  {
    const long mb = blockIdx.y;
    L += mb * ms.L; z += mb * ms.L; q += mb * ms.q; hv.base += mb * ms.v; out += mb * sO;
    y += (long)(kps ? kps[mb].ds : (int)mb) * sY;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  if (t >= n) return;
  const int s = t - lead + 1;
  const bool scored = s >= min_train;
  double r = 0.0, w = 0.0;
  if (scored) {
    const double* row = L + (long)t * ld;
    for (int j = s + lane; j <= t; j += 64) {
      const double l = row[j];
      r = fma(l, z[j], r);
      w = fma(l, l, w);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { r += __shfl_down(r, off, 64); w += __shfl_down(w, off, 64); }
  if (lane != 0) return;
  if (rw) { hv.r()[t] = r; hv.w()[t] = w; }
  if (!scored) {
    const double qnan = __builtin_nan("");
    out[t] = qnan; out[ldo + t] = qnan; out[2 * ldo + t] = 0.0; out[3 * ldo + t] = 0.0;
    return;
  }
  const double sig = mode == 0 ? hv.cum()[s] / (double)s : *q / (double)n;
  const double v = sig * w;
  out[t] = y[t] - r;
  out[ldo + t] = v;
  out[2 * ldo + t] = 0.5 * log(2.0 * M_PI * v) + r * r / (2.0 * v);
  out[3 * ldo + t] = r * r;
}

// The coefficients of the score `crit` (0 nlpd, 1 sse) in sigma mode `mode`, one block per member: rho_t, ks_t = kappa_t sigma_t (zero in
// unscored rows) and suf[t0] = sum_{t >= t0} g_t with g_t = kappa_t w_t / s_t (refit) or kappa_t w_t / n (fixed), by a fixed-order scan from
// the last row down.  sigma_t and var_t are formed as hindcast_rows_kernel forms them.  One block per member and O(n) on purpose: the
// coefficients are evaluated twice (for the chunk sums and again when they are stored, instead of a store and a reload) and every thread adds
// the totals of the threads before it serially, so that each suffix sum is one chain of additions in a fixed order whatever n is.
__global__ __launch_bounds__(256) void hindcast_coef_kernel(int n, const double* __restrict__ q, int lead, int min_train, int mode, int crit, HindcastVecs hv,
                                                            HindcastStrides ms) {
  __shared__ double tot[256];
  q += (long)blockIdx.x * ms.q; hv.base += (long)blockIdx.x * ms.v;
  const double* cum = hv.cum();
  const double* rr = hv.r();
  const double* ww = hv.w();
  double* rho = hv.rho();
  double* ks = hv.ks();
  double* suf = hv.suf();
  const double qn = *q / (double)n;
  auto coef = [&](int t, double& rh, double& k_s) -> double {
    const int s = t - lead + 1;
    rh = 0.0; k_s = 0.0;
    if (s < min_train) return 0.0;
    const double r = rr[t], w = ww[t];
    if (crit != 0) { rh = 2.0 * r; return 0.0; }
    const double sig = mode == 0 ? cum[s] / (double)s : qn;
    const double var = sig * w;
    const double kappa = 1.0 / (2.0 * var) - r * r / (2.0 * var * var);
    rh = r / var;
    k_s = kappa * sig;
    return mode == 0 ? kappa * w / (double)s : kappa * w / (double)n;
  };
  hc_block_scan(n, tot,
                [&](int p) { double a, b; return coef(n - 1 - p, a, b); },
                [&](int p, double before, double g) {
                  const int t = n - 1 - p;
                  double a, b;
                  (void)coef(t, a, b);
                  rho[t] = a; ks[t] = b; suf[t] = before + g;
                });
}

// zbar_j, one thread per column j of L (its entries L_tj, t = j .. j + lead - 1, are read along the rows: coalesced across the threads);
// zero from n on.  blockIdx.y = lockstep member.
__global__ __launch_bounds__(256) void hindcast_zbar_kernel(const double* __restrict__ L, long ld, int n, int n_pad, const double* __restrict__ z, int lead, int mode,
                                                            HindcastVecs hv, HindcastStrides ms) {
  {
    const long mb = blockIdx.y;
    L += mb * ms.L; z += mb * ms.L; hv.base += mb * ms.v;
  }
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_pad) return;
  double acc = 0.0;
  if (j < n) {
    const double* rho = hv.rho();
    const int t1 = min(n - 1, j + lead - 1);
    for (int t = j; t <= t1; ++t) acc = fma(rho[t], L[(long)t * ld + j], acc);
    const double sf = mode == 0 ? (j + lead < n ? hv.suf()[j + lead] : 0.0) : hv.suf()[0];
    acc = fma(2.0 * z[j], sf, acc);
  }
  hv.zbar()[j] = acc;
}

// The banded part of C, Cb [n_pad][n_pad] symmetric: Cb_ij = Cb_ji = (L^T B)_ij / 2 for 0 <= i - j < lead, summed in ascending k; zero
// elsewhere and from n on.  (The rank-one part of C, -zbar_i z_j / 2, is never stored: hindcast_w_kernel.)  Entry (row, col) is computed from
// (i, j) = (max, min), so both halves carry the same bits and every store is coalesced.  grid (n_pad / 256, n_pad, members).
__global__ __launch_bounds__(256) void hindcast_band_kernel(const double* __restrict__ L, long ld, int n, int n_pad, const double* __restrict__ z, int lead,
                                                            HindcastVecs hv, double* __restrict__ Cb, HindcastStrides ms) {
  {
    const long mb = blockIdx.z;
    L += mb * ms.L; z += mb * ms.L; hv.base += mb * ms.v; Cb += mb * ms.C;
  }
  const int row = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n_pad) return;
  const int i = max(row, col), j = min(row, col);
  double a = 0.0;
  if (i < n && i - j < lead) {
    const double zj = z[j];
    const double* rho = hv.rho();
    const double* ks = hv.ks();
    const int k1 = min(n - 1, j + lead - 1);
    for (int k = i; k <= k1; ++k) {
      const double lki = L[(long)k * ld + i], lkj = L[(long)k * ld + j];
      a = fma(lki, fma(2.0 * ks[k], lkj, rho[k] * zj), a);
    }
    a *= 0.5;
  }
  Cb[(long)row * ld + col] = a;
}

// W = U C, one block per row i of the upper-triangular U = L~^-T (this kernel never reads entries left of the diagonal; the product G = U W^T
// behind it does, inside the diagonal 128-blocks: sigp_hindcast.inc states what it relies on), without a cubic product:
//     W_ik = sum_{j >= i, |j - k| < lead} U_ij Cb_jk  -  ( zbar_k sum_{i <= j < k} U_ij z_j  +  z_k sum_{j >= max(i, k)} U_ij zbar_j ) / 2.
// The two sums of the rank-one part are one prefix scan and one suffix scan along the row (hc_block_scan: a fixed order); the banded part is
// at most 2 lead - 1 terms per entry, Cb read along its rows (Cb is symmetric): coalesced across the threads.  Rows and columns n .. n_pad
// of W are zero.  blockIdx.y = lockstep member.
//
// The row of W both kernels below form, written once so that every entry is one chain of floating-point operations whichever kernel forms
// it: urow[j] and wrow[j] (j = i .. n - 1: the row piece of U and the rank-one part on its way) live where the caller says -- global memory
// (hindcast_w_kernel: wrow is the row of W itself) or LDS (hindcast_w_lds_kernel) -- and `out` is the row of W.
template <typename UR, typename WR>
__device__ __forceinline__ void hc_w_row(int i, int n, int n_pad, int lead, UR urow, WR wrow, const double* __restrict__ z, const double* __restrict__ zbar,
                                         const double* __restrict__ Cb, long ld, double* out, double* tot /* [256] LDS */, double* whole /* LDS */) {
  const int len = n - i;
  // prefix: wrow[j] = -zbar_j / 2 sum_{i <= j' < j} U_ij' z_j'
  hc_block_scan(len, tot, [&](int p) { return urow[i + p] * z[i + p]; }, [&](int p, double before, double) { wrow[i + p] = -0.5 * zbar[i + p] * before; });
  __syncthreads();
  // suffix, from the last column down: wrow[j] -= z_j / 2 sum_{j' >= j} U_ij' zbar_j'; the whole sum serves the columns left of the diagonal
  hc_block_scan(len, tot, [&](int p) { return urow[n - 1 - p] * zbar[n - 1 - p]; },
                [&](int p, double before, double v) {
                  const int j = n - 1 - p;
                  const double sfx = before + v;
                  wrow[j] = fma(-0.5 * z[j], sfx, wrow[j]);
                  if (j == i) *whole = sfx;
                });
  __syncthreads();
  const double wh = *whole;
  for (int k = threadIdx.x; k < n_pad; k += 256) {
    if (k >= n) { out[k] = 0.0; continue; }
    double a = k < i ? -0.5 * z[k] * wh : wrow[k];
    const int j0 = max(i, k - lead + 1), j1 = min(n - 1, k + lead - 1);
    for (int j = j0; j <= j1; ++j) a = fma(urow[j], Cb[(long)j * ld + k], a);
    out[k] = a;
  }
}

__global__ __launch_bounds__(256) void hindcast_w_kernel(const double* __restrict__ U, const double* __restrict__ Cb, long ld, int n, int n_pad,
                                                         const double* __restrict__ z, int lead, HindcastVecs hv, double* __restrict__ W, HindcastStrides ms) {
  __shared__ double tot[256];
  __shared__ double whole;
  {
    const long mb = blockIdx.y;
    U += mb * ms.C; Cb += mb * ms.C; W += mb * ms.C; z += mb * ms.L; hv.base += mb * ms.v;
  }
  const int i = blockIdx.x;
  double* wrow = W + (long)i * ld;
  if (i >= n) {
    for (int k = threadIdx.x; k < n_pad; k += 256) wrow[k] = 0.0;
    return;
  }
  hc_w_row(i, n, n_pad, lead, U + (long)i * ld, wrow, z, hv.zbar(), Cb, ld, wrow, tot, &whole);
}

// The same row with the row piece U[i, i..n) and the rank-one part kept in dynamic LDS (hindcast_w_lds_bytes(n_pad), score_layout.hpp), for
// lockstep groups: hindcast_w_kernel's chunked scans make the lanes of a wave read the row of U -- and read and write the row of W -- at a
// stride of the chunk length c = ceil(len / 256), one cache line per lane from c = 16 on.  Here global memory is touched three times, each
// 256 consecutive doubles wide: the row piece of U comes in once, Cb is read along its rows, the row of W goes out once.  hc_w_row forms
// every entry, so a row carries hindcast_w_kernel's bits.  Column j of the row sits at LDS index q + (q >> 5), q = j - i: the scans' lanes
// are c doubles apart, which at c = 8, 16, 32 (n = 2048 .. 8192) would put 8, 16, 32 lanes of a 32-lane ds_read_b64 group on one pair of
// banks; with the skew of one double per 32 the group's 32 addresses fall on 32 bank pairs at all three.  z and zbar stay in global
// memory: 16 n bytes shared by every row, they live in the caches.
// grid (n_pad, members), n_pad <= HINDCAST_W_LDS_MAX_NPAD.
struct HcLdsRow {
  double* p; int i;
  __device__ __forceinline__ double& operator[](int j) const { const int q = j - i; return p[q + (q >> 5)]; }
};

__global__ __launch_bounds__(256) void hindcast_w_lds_kernel(const double* __restrict__ U, const double* __restrict__ Cb, long ld, int n, int n_pad,
                                                             const double* __restrict__ z, int lead, HindcastVecs hv, double* __restrict__ W, HindcastStrides ms) {
  extern __shared__ double hc_w_lds[];   // the row piece of U, then the rank-one part: hindcast_w_lds_row(n_pad) doubles each
  __shared__ double tot[256];
  __shared__ double whole;
  {
    const long mb = blockIdx.y;
    U += mb * ms.C; Cb += mb * ms.C; W += mb * ms.C; z += mb * ms.L; hv.base += mb * ms.v;
  }
  const int i = blockIdx.x;
  double* out = W + (long)i * ld;
  if (i >= n) {
    for (int k = threadIdx.x; k < n_pad; k += 256) out[k] = 0.0;
    return;
  }
  const HcLdsRow urow{hc_w_lds, i}, wrow{hc_w_lds + hindcast_w_lds_row(n_pad), i};
  const double* ug = U + (long)i * ld;
  for (int j = i + (int)threadIdx.x; j < n; j += 256) urow[j] = ug[j];
  __syncthreads();
  hc_w_row(i, n, n_pad, lead, urow, wrow, z, hv.zbar(), Cb, ld, out, tot, &whole);
}

}  // namespace sigp
