// Exact gradient of the profiled nlML with respect to d per-feature (ARD) length scales, all d components in ONE pass over K~^-1
// (sigp_nlml_grad_ard, driver: sigp_ardgrad.inc).  With u_i = x_i / l (the features as sigp_set_length_scales stages them), P = K~^-1,
// a = P y, sf = y^T a / n:
//     d nlML / d log l_k = sum_ij W_ij (u_ik - u_jk)^2,     W_ij = 1/2 (P_ij - a_i a_j / sf) h_ij,
//     h = k (RBF),  h = (5/3)(1 + s) e^-s, s = sqrt(5) r (Matern-5/2);  the diagonal contributes 0.
// Forming d derivative matrices and reducing each against K~^-1 costs ~24 d n^2 bytes; here K~^-1 is read once (4 n^2 bytes).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_misc.hpp"

namespace sigp {

// h_ij of the formula above from the squared distance of the scaled features (length scale 1; the clamps of cov_from_sq)
__device__ __forceinline__ double ard_h_from_sq(int kernel_id, double sq) {
  if (kernel_id == KID_RBF) return exp_cov(-0.5 * sq);
  const double s = fmin(sqrt(5.0 * sq), KS_MAX);
  return (5.0 / 3.0) * (1.0 + s) * exp_cov(-s);
}

// Column means of the first n rows of U [n_pad][dp] (one block per feature, fixed-order sum) and the centred copy Uc = U - mean on those
// rows; Uc's padding (rows >= n, columns >= d) is zeroed by the caller.  Differences of rows are unchanged; the expanded square of
// ard_grad_partial_kernel then cancels at the scale of the data's spread, not of its offset (SST in kelvin, years).
// blockIdx.y = lockstep member: its U and Uc lie sU doubles behind the previous member's (a single fit: one member, stride 0).
__global__ __launch_bounds__(256) void ard_center_kernel(const double* __restrict__ U, int dp, int n, double* __restrict__ Uc, long sU = 0) {
  __shared__ double sh[4];
  __shared__ double mean;
  const int k = blockIdx.x;
  U += (long)blockIdx.y * sU; Uc += (long)blockIdx.y * sU;
  double t = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) t += U[(long)i * dp + k];
  t = block_reduce_sum(t, sh);
  if (threadIdx.x == 0) mean = t / (double)n;
  __syncthreads();
  const double mu = mean;
  for (int i = threadIdx.x; i < n; i += 256) Uc[(long)i * dp + k] = U[(long)i * dp + k] - mu;
}

// One workgroup per 64 x 128 tile of the lower triangle of K~^-1 (the covariance build's tiles and tile walk: kbuild_tiles(n_pad) of
// them); every pair i > j is visited once and stands for (j, i) as well (the factor 2 cancels W's 1/2), a tile on the diagonal uses its
// strictly lower part.  Per tile:
//   - squared distances of the scaled features by the covariance build's own GEMM-form code (kb_gram_tile), on U itself;
//   - W = (P - a a^T / sf) o h, masked, in the accumulator layout the distances arrive in: lane (lr, lq) of wave w holds row 16 w + lr,
//     columns 16 t + 4 lq + c.  That IS the A operand of v_mfma_f64_16x16x4_f64 when the four columns of a K step are taken as
//     16 t + 4 q + c, q = 0 .. 3 (the sum over j may run in any order), so W never goes through LDS; only its row sums do;
//   - with the centred features, in chunks of 16:  sum_j W_ij (u_ik - u_jk)^2 = u_ik^2 rowsum(W)_i + [W (U_J o U_J)]_ik - 2 u_ik [W U_J]_ik,
//     the two products on the matrix pipe (B operand: rows 16 t + 4 lq + c of U_J, 16 consecutive features per quarter wave);
//   - the 16 x (4 waves x 4 quarter waves) partial sums of a chunk are added in a fixed order: partial[tile][k], no atomics.
// The expanded square cancels at the scale of the CENTRED data's spread: a component's error is about u (spread / difference)^2 of its sum with
// |.| inside (S).  Measured one launch at a time against long double (tests/test_hip_ard_pass.py, docs/EXPERIMENTS.md): error / S = 3e-16 for
// N(0,1) features, 5e-16 behind an offset of 1e4 (the centring removes it), and 3.2e-9 -- ABOVE 1e-9, a factor of 3 inside the end-to-end
// tolerance of 1e-8 -- for a feature in two clusters at +-3000 with unit scatter; an fp64 emulation of the formula gives the same 3.4e-9.
// sf = q[0] / n is read from device memory (the fit's epilogue left y^T a there): no host round trip before the pass.
// WSEL picks the weight: ARD_W_NLML, the adjoint of the nlML above; ARD_W_LOO, the adjoint of a leave-one-out score (looard.hpp) --
// W = (2 M_ij + v_i a_j + a_i v_j + 2 eps a_i a_j) o h with M = P diag(gamma) P read where P is read (its lower 128-tiles), v = P beta and
// eps[0] from device memory (q is not read).  Everything after the weight is shared.
// blockIdx.y = lockstep member (sigp_nlml_grad_ard_batch, sigp_loo_grad_ard_batch): member b reads U, Uc, P, a, q (ARD_W_NLML) or v, eps
// (ARD_W_LOO) and writes partial at b times the strides of ms (in doubles); the offsets are added to the pointers before anything is read,
// so a member executes the instructions a single fit does.  Single fits launch one member with zero strides.
// What each operand must hold where the formula does not reach (tests/test_hip_ard_pass.py fills the second kind with NaN):
//   ZERO (read and used):        U in columns >= d up to dp (the staged rows and their norms take whole chunks of 4 features) and, as the
//                                engine's staging leaves it, in rows >= n (they reach masked entries alone);  Uc in both, which the pass's
//                                memset and ard_center_kernel see to: its padding rows are B operands of the products (0 x anything must be 0).
//   ANYTHING (loaded at most, never used: the mask gi < n && gj + c < gi selects 0.0, it does not multiply):
//                                P / M on and above the diagonal inside the lower 128-tiles, every 128-tile above the diagonal (not even
//                                loaded), rows and columns >= n;  a and v from n on;  q under ARD_W_LOO, v and eps under ARD_W_NLML (null
//                                pointers in the engine);  whatever lies between the members' strided buffers.
//   The finish kernels read, besides the partials, the diagonal of P / M and a (v, eps) on rows < n alone.
enum { ARD_W_NLML = 0, ARD_W_LOO = 1 };
struct ArdMemberStrides { long U, P, a, q, partial, v, eps; };   // U and Uc alike; q: the slot's result rows (512 doubles apart); v, eps: ARD_W_LOO alone
template <int DC, int WSEL = ARD_W_NLML>
__global__ __launch_bounds__(256) void ard_grad_partial_kernel(const double* __restrict__ U, const double* __restrict__ Uc, int dp, int d, int n,
                                                               int kernel_id, const double* __restrict__ P, long ld,
                                                               const double* __restrict__ a, const double* __restrict__ q,
                                                               double* __restrict__ partial, const double* __restrict__ v = nullptr,
                                                               const double* __restrict__ eps = nullptr, ArdMemberStrides ms = ArdMemberStrides{0, 0, 0, 0, 0, 0, 0}) {
  {
    const long mb = blockIdx.y;
    U += mb * ms.U; Uc += mb * ms.U; P += mb * ms.P; a += mb * ms.a; partial += mb * ms.partial;
    if constexpr (WSEL == ARD_W_NLML) q += mb * ms.q;
    else { v += mb * ms.v; eps += mb * ms.eps; }
  }
  const int u = blockIdx.x >> 1;                       // (the lower-triangle tile walk of kbuild_mfma_kernel)
  int k = (int)((sqrt(8.0 * u + 1.0) - 1.0) * 0.5);
  while ((k + 1) * (k + 2) / 2 <= u) ++k;
  while (k * (k + 1) / 2 > u) --k;
  const int bj = u - k * (k + 1) / 2, bi = 2 * k + (blockIdx.x & 1);
  constexpr int LP = DC + 2;
  __shared__ __attribute__((aligned(16))) double Xi[KB_TM * LP];
  __shared__ __attribute__((aligned(16))) double Xj[KB_TN * LP];
  __shared__ __attribute__((aligned(16))) double nI[KB_TM], nJ[KB_TN];
  __shared__ double rs[KB_TM];
  __shared__ double red[16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  d4 acc[8];
  kb_gram_tile<DC>(U, dp, d, bi, bj, Xi, Xj, nI, nJ, acc);
  const int gi = bi * KB_TM + 16 * wave + lr;
  const double ni = nI[16 * wave + lr];
  double ai_sf = 0.0, ai = 0.0, vi = 0.0, eps2 = 0.0;
  if constexpr (WSEL == ARD_W_NLML) {
    const double sf = q[0] / (double)n;
    ai_sf = a[gi] / sf;
  } else {
    ai = a[gi]; vi = v[gi]; eps2 = 2.0 * eps[0];
  }
  double rowsum = 0.0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int gj = bj * KB_TN + 16 * t + 4 * lq;
    const d2 nj01 = *(const d2*)(nJ + 16 * t + 4 * lq), nj23 = *(const d2*)(nJ + 16 * t + 4 * lq + 2);
    const double njv[4] = {nj01.x, nj01.y, nj23.x, nj23.y};
    const d2 p01 = *(const d2*)(P + (long)gi * ld + gj), p23 = *(const d2*)(P + (long)gi * ld + gj + 2);
    const double pv[4] = {p01.x, p01.y, p23.x, p23.y};
    const d2 a01 = *(const d2*)(a + gj), a23 = *(const d2*)(a + gj + 2);
    const double av[4] = {a01.x, a01.y, a23.x, a23.y};
    double vv[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (WSEL == ARD_W_LOO) {
      const d2 v01 = *(const d2*)(v + gj), v23 = *(const d2*)(v + gj + 2);
      vv[0] = v01.x; vv[1] = v01.y; vv[2] = v23.x; vv[3] = v23.y;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double w = 0.0;
      if (gi < n && gj + c < gi) {
        const double h = ard_h_from_sq(kernel_id, kb_gram_sq(acc[t][c], ni, njv[c]));
        if constexpr (WSEL == ARD_W_NLML) w = fma(-ai_sf, av[c], pv[c]) * h;
        else w = fma(2.0, pv[c], fma(vi, av[c], ai * fma(eps2, av[c], vv[c]))) * h;
      }
      acc[t][c] = w;
      rowsum += w;
    }
  }
  rowsum += __shfl_xor(rowsum, 16, 64);
  rowsum += __shfl_xor(rowsum, 32, 64);
  if (lq == 0) rs[16 * wave + lr] = rowsum;
  __syncthreads();
  double rsv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rsv[r] = rs[16 * wave + lq + 4 * r];
  const int dq = (d + 15) & ~15;                       // (<= dp; U and Uc are zero there)
  const double* uJ = Uc + (long)(bj * KB_TN + 4 * lq) * dp + lr;
  const double* uI = Uc + (long)(bi * KB_TM + 16 * wave + lq) * dp + lr;
  for (int f0 = 0; f0 < dq; f0 += 16) {
    d4 D1, D2;
#pragma unroll
    for (int r = 0; r < 4; ++r) { D1[r] = 0.0; D2[r] = 0.0; }
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double b = uJ[(long)(16 * t + c) * dp + f0];
        D1 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[t][c], b, D1, 0, 0, 0);
        D2 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[t][c], b * b, D2, 0, 0, 0);
      }
    double s = 0.0;                                    // feature f0 + lr, rows 16 wave + lq + 4 r of the tile
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double ui = uI[(long)(4 * r) * dp + f0];
      s += fma(ui * ui, rsv[r], fma(-2.0 * ui, D1[r], D2[r]));
    }
    red[4 * wave + lq][lr] = s;
    __syncthreads();
    if (tid < 16) {
      double tsum = 0.0;
#pragma unroll
      for (int w = 0; w < 16; ++w) tsum += red[w][tid];
      partial[(long)blockIdx.x * dp + f0 + tid] = tsum;
    }
    __syncthreads();
  }
}

// grad[k] = sum over the tiles, in tile order, of partial[tile][k] (k < d: block k), and grad[d] = sn~ sum_i (P_ii / 2 - a_i^2 / (2 sf))
// (block d).  Every thread adds its tiles / rows in ascending order and block_reduce_sum adds the threads in a fixed order: the same
// bits on every run.  blockIdx.y = lockstep member: the strides of ms as above, grad [member][sGrad], and the member's sn~ from sn_m
// (device memory; NULL: the argument sn, a single fit).
__global__ __launch_bounds__(256) void ard_grad_finish_kernel(const double* __restrict__ partial, long ntiles, int dp, int d, int n,
                                                              const double* __restrict__ P, long ld, const double* __restrict__ a,
                                                              const double* __restrict__ q, double sn, double* __restrict__ grad,
                                                              ArdMemberStrides ms = ArdMemberStrides{0, 0, 0, 0, 0, 0, 0}, long sGrad = 0,
                                                              const double* __restrict__ sn_m = nullptr) {
  __shared__ double sh[4];
  const int k = blockIdx.x;
  {
    const long mb = blockIdx.y;
    partial += mb * ms.partial; P += mb * ms.P; a += mb * ms.a; q += mb * ms.q; grad += mb * sGrad;
    if (sn_m != nullptr) sn = sn_m[mb];
  }
  double t = 0.0;
  if (k < d) {
    for (long i = threadIdx.x; i < ntiles; i += 256) t += partial[i * dp + k];
  } else {
    const double sf = q[0] / (double)n;
    for (int i = threadIdx.x; i < n; i += 256) t += 0.5 * P[(long)i * ld + i] - a[i] * a[i] / (2.0 * sf);
  }
  t = block_reduce_sum(t, sh);
  if (threadIdx.x == 0) grad[k] = k < d ? t : sn * t;
}

// Per-member scaled staging of a lockstep group (sigp_batch_run_ard, sigp_nlml_grad_ard_batch): member b = blockIdx.y has data set
// (first_ds + b) % batch of the resident batch data (bX [batch][n_pad][dp], bXs [batch][ride][dp], by [batch][n_pad], zero padded) and the
// divisors div [b][dp].  One launch fills the member's scaled training features, scaled ride rows and its y, laid out as the resident data are
// so that the member is "data set b" of the staging area to every kernel that takes a data-set index.  u = x / l_k is the IEEE division
// (pad_copy_kernel's, the same bits); the padding (rows >= n, features >= d) is zero in the source and stays zero.
__global__ __launch_bounds__(256) void ard_stage_kernel(const double* __restrict__ bX, const double* __restrict__ bXs, const double* __restrict__ by,
                                                        long first_ds, long batch, int n_pad, int ride, int dp, int d, const double* __restrict__ div,
                                                        double* __restrict__ X, double* __restrict__ Xs, double* __restrict__ y) {
  const long b = blockIdx.y, ds = (first_ds + b) % batch;
  const long nx = (long)n_pad * dp, nr = (long)ride * dp;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < nx + nr) {
    const bool train = idx < nx;
    if (!train) idx -= nx;
    const int p = (int)(idx % dp);
    double v = train ? bX[ds * nx + idx] : bXs[ds * nr + idx];
    if (p < d) v = v / div[b * dp + p];
    (train ? X + b * nx : Xs + b * nr)[idx] = v;
  } else if (idx < nx + nr + n_pad) {
    idx -= nx + nr;
    y[b * n_pad + idx] = by[ds * n_pad + idx];
  }
}

}  // namespace sigp
