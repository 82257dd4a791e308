// Exact gradients of the leave-one-out scores with respect to d per-feature (ARD) length scales (sigp_loo_grad_ard, driver:
// sigp_looard.inc).  The per-point chain rule of loograd.hpp is LINEAR in the three quantities that depend on the direction D = dK~/dtheta,
//     b = P D a,   c = diag(P D P),   e = a^T D a,
// so it transposes into one symmetric adjoint matrix that does not depend on the direction:
//     d score = beta^T b + gamma^T c + eps e = sum_ij G_ij D_ij,     G = 1/2 (v a^T + a v^T) + P diag(gamma) P + eps a a^T,   v = P beta.
// With kappa_i = 1/(2 var_i) - r_i^2/(2 var_i^2), rho_i = r_i/var_i (notation of loograd.hpp: g_i = P_ii, r_i = a_i/g_i, var_i = s_i/g_i):
//     nlpd   beta_i  = -rho_i/g_i                               + [refit]  2 kappa_i a_i / (g_i^2 (n - 1))
//            gamma_i = kappa_i s_i/g_i^2 + rho_i a_i/g_i^2      - [refit]  kappa_i a_i^2 / (g_i^3 (n - 1))
//            eps     = -sum_i kappa_i/g_i / (n - 1)  [refit]    or  / n  [fixed]
//     sse    beta_i  = -2 r_i/g_i,   gamma_i = 2 r_i a_i/g_i^2,   eps = 0
// Every derivative is then the contraction ardgrad.hpp performs for the nlML, for all d features in one pass:
//     d score / d log l_k = sum_ij G_ij h_ij (u_ik - u_jk)^2     (a pair i > j visited once carries 2 G_ij h_ij; the diagonal contributes 0)
//     d score / d log sn~ = sn~ tr G
// The one cubic quantity is M = P diag(gamma) P = (P Gamma) P^T: its lower 128-tiles by syrk128_kernel's SET form (n^3 flops), whatever d.
// Rows and columns n .. n_pad of every operand are masked.  No atomics anywhere: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"
#include "score_layout.hpp"

namespace sigp {

// The vector workspace of the pass (in the gradient workspace of sigp_loo_grad), LooArdVecs: score_layout.hpp.
// Lockstep members (sigp_loo_grad_ard_batch): every kernel below takes the member from a grid dimension and adds the member's offsets -- P, PG
// and M n_pad^2 apart, the vectors LooArdGroupVecs::mstride() apart, q in the slot's result rows -- to its pointers before anything is
// read: uniform values, no vector register, and a member executes the instructions a single fit does.  The single fits launch one member
// with zero strides.
struct LooArdStrides { long P, q, w, partial, grad; };   // P: P, PG and M alike;  w: the vector workspace;  q: 512 doubles in a slot

// beta, gamma [n_pad] (zero from n on) and eps of the score `crit` (0 nlpd, 1 sse) in sigma mode `mode` (0 "refit", 1 "fixed"), one block:
// g_i is the diagonal of P, q = y^T A~ comes from *q; s_i and var_i are formed as loo_rows_kernel / loo_grad_point_kernel form them.
// Every thread adds its points in ascending order and block_reduce_sum adds the threads in a fixed order.  blockIdx.x = lockstep member.
__global__ __launch_bounds__(256) void loo_ard_coef_kernel(const double* __restrict__ P, long ld, int n, int n_pad, const double* __restrict__ q, int mode, int crit,
                                                           LooArdVecs w, LooArdStrides ms = LooArdStrides{0, 0, 0, 0, 0}) {
  __shared__ double sh[4];
  {
    const long mb = blockIdx.x;
    P += mb * ms.P; q += mb * ms.q; w.base += mb * ms.w;
  }
  const double* a = w.a();
  double* beta = w.beta();
  double* gamma = w.gamma();
  const double qq = q[0];
  const double n1 = (double)(n - 1);
  double esum = 0.0;
  for (int i = threadIdx.x; i < n_pad; i += 256) {
    double be = 0.0, ga = 0.0;
    if (i < n) {
      const double g = P[(long)i * ld + i], ai = a[i];
      const double r = ai / g;
      if (crit == 0) {
        const double s = mode == 0 ? (qq - ai * r) / n1 : qq / (double)n;
        const double var = s / g;
        const double kappa = 1.0 / (2.0 * var) - r * r / (2.0 * var * var), rho = r / var;
        be = -rho / g;
        ga = kappa * s / (g * g) + rho * ai / (g * g);
        if (mode == 0) {
          be += 2.0 * kappa * ai / (g * g * n1);
          ga -= kappa * ai * ai / (g * g * g * n1);
        }
        esum += kappa / g;
      } else {
        be = -2.0 * r / g;
        ga = 2.0 * r * ai / (g * g);
      }
    }
    beta[i] = be;
    gamma[i] = ga;
  }
  esum = block_reduce_sum(esum, sh);
  if (threadIdx.x == 0) w.eps()[0] = crit == 0 ? -esum / (mode == 0 ? n1 : (double)n) : 0.0;
}

// One WAVE per row i < n_pad of the full P:  v_i = sum_{k < n} P_ik beta_k  and row i of P Gamma, PG_ik = P_ik gamma_k, written whole
// (zero from column n on; rows n .. n_pad are zero and v is zero there).  blockIdx.y = lockstep member.
__global__ __launch_bounds__(256) void loo_ard_scale_kernel(const double* __restrict__ P, double* __restrict__ PG, long ld, int n, int n_pad, LooArdVecs w,
                                                            LooArdStrides ms = LooArdStrides{0, 0, 0, 0, 0}) {
  {
    const long mb = blockIdx.y;
    P += mb * ms.P; PG += mb * ms.P; w.base += mb * ms.w;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n_pad) return;
  const double* beta = w.beta();
  const double* gamma = w.gamma();
  const double* row = P + (long)i * ld;
  double* orow = PG + (long)i * ld;
  double acc = 0.0;
  for (int k0 = 0; k0 < n_pad; k0 += 128) {
    const int k = k0 + lane * 2;
    const d2 p = *(const d2*)(row + k);
    const d2 bv = *(const d2*)(beta + k);
    const d2 gv = *(const d2*)(gamma + k);
    d2 o;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool in = i < n && k + e < n;
      const double pe = in ? p[e] : 0.0;
      acc = fma(pe, in ? bv[e] : 0.0, acc);
      o[e] = in ? pe * gv[e] : 0.0;
    }
    *(d2*)(orow + k) = o;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) w.v()[i] = acc;
}

// grad[k] = sum over the tiles, in tile order, of partial[tile][k] (k < d: block k), and grad[d] = sn~ tr G = sn~ sum_i (M_ii + v_i a_i + eps a_i^2)
// (block d): ard_grad_finish_kernel with the adjoint of a leave-one-out score in the noise component.  blockIdx.y = lockstep member: grad
// [member][ms.grad], and the member's sn~ from sn_m (device memory; NULL: the argument sn, a single fit).
__global__ __launch_bounds__(256) void loo_ard_finish_kernel(const double* __restrict__ partial, long ntiles, int dp, int d, int n, const double* __restrict__ M, long ld,
                                                             LooArdVecs w, double sn, double* __restrict__ grad, LooArdStrides ms = LooArdStrides{0, 0, 0, 0, 0},
                                                             const double* __restrict__ sn_m = nullptr) {
  __shared__ double sh[4];
  const int k = blockIdx.x;
  {
    const long mb = blockIdx.y;
    partial += mb * ms.partial; M += mb * ms.P; w.base += mb * ms.w; grad += mb * ms.grad;
    if (sn_m != nullptr) sn = sn_m[mb];
  }
  double t = 0.0;
  if (k < d) {
    for (long i = threadIdx.x; i < ntiles; i += 256) t += partial[i * dp + k];
  } else {
    const double* a = w.a();
    const double* v = w.v();
    const double eps = w.eps()[0];
    for (int i = threadIdx.x; i < n; i += 256) t += M[(long)i * ld + i] + a[i] * fma(eps, a[i], v[i]);
  }
  t = block_reduce_sum(t, sh);
  if (threadIdx.x == 0) grad[k] = k < d ? t : sn * t;
}

}  // namespace sigp
