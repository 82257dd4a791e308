// Refined block solve for gfx950 (fp64): a row tile against ONE 128 x 128 diagonal block of the factor, as a product with the stored inverse
// block plus ONE residual-correction step, in one launch and in place.  The plain product  X = A W^T  (W = inv(L) as the diagonal-block
// kernel left it) carries an error proportional to cond(L); substitution is backward stable.  One step of
//     X1 = A W^T,    R = A - X1 L^T,    X = X1 + R W^T          (forward:  X L^T = A)
//     X1 = A W,      R = A - X1 L,      X = X1 + R W            (TRANS:    X L   = A)
// brings the row residual |X L^T - A| down to substitution's while u cond(L) < 1 (option accurate_solve, include/sigp.h at sigp_potrf).
//
// Design (CDNA4): one workgroup of 256 threads = 4 waves owns RS_TM = 32 rows from load to store (rows are independent: C == A is safe).  Wave w
// owns the 32 x 32 column block w as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64, the layout of the plain column solve (gemm_mfma_kernel<32, 128, 1, 4>).
// The three products run back to back as one stream of 3 x 8 k-slices of 16 of the triangular operand (W, L, W), staged global -> VGPR ->
// LDS double-buffered with one barrier per slice and four slices in flight in registers, as gemm_tile_body stages the operands of its small tiles.  The LEFT operand of each product is a whole
// 32 x 128 image in LDS (pitch 130: the 8-byte fragment reads row = lane & 15, k = lane >> 4 of a 32-lane pass hit 32 distinct bank slots):
//     P1 = A  (read from HBM once)  ->  product 1  ->  X1 in the accumulators; kept in registers, and -X1 written to P2
//     accumulators <- A from P1     ->  product 2 on P2  ->  R = A - X1 L^T in the accumulators, written to P1 (A is no longer needed)
//     accumulators <- X1            ->  product 3 on P1  ->  X, stored
// so neither A nor X1 nor R travels through HBM.  L is read in its lower triangle only (what stands above the diagonal of a diagonal block of
// the matrix is undefined): 16-byte chunks that lie wholly above the diagonal are not loaded, the one straddling element is replaced by zero.
// W gets the same treatment (its strict upper triangle is zero by construction).  Zero k-slices are skipped per 16-column accumulator
// block (forward: slices beyond the block's columns, TRANS: slices before them), as strip_tri does; every entry sums its k in ascending
// order, no atomics: the same bits on every run, for any grid.  Rows beyond `rows` are staged as zeros and not stored.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_mfma.hpp"

namespace sigp {

constexpr int RS_TM = 32;                 // rows per workgroup
constexpr int RS_N = 128;                 // the diagonal block
constexpr int RS_PP = RS_N + 2;           // pitch of the 32 x 128 left-operand images
constexpr int RS_QN = 18;                 // pitch of a [n][16 k] slice image (forward form), as Num<double>::LDP
constexpr int RS_QT = RS_N + 16;          // pitch of a [16 k][n] slice image (TRANS), as gemm_tile_body's BT image
constexpr int RS_PD = 4;                  // k-slices of W / L in flight in registers
constexpr int RS_QBUF = RS_N * RS_QN;     // doubles per slice buffer (= 16 * RS_QT)
static_assert(RS_N * RS_QN == 16 * RS_QT, "both slice images have the same size");
constexpr int refined_lds_bytes() { return (2 * RS_TM * RS_PP + 2 * RS_QBUF) * (int)sizeof(double); }

struct RefinedArgs {
  double* A; long lda, sA;                // rows x 128 row tile(s), solved in place; member stride sA
  const double* W; long ldw, sW;          // the inverse diagonal block (lower triangular)
  const double* L; long ldl, sL;          // the diagonal block of the factor (lower triangle read)
  int rows;                               // rows of A (any count >= 1; grid.x = ceil(rows / 32), grid.y = members)
};

template <bool TRANS>
__global__ __launch_bounds__(256) void refined_solve_kernel(RefinedArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* P1 = (double*)smem_raw;         // [32][RS_PP]  A, later R
  double* P2 = P1 + RS_TM * RS_PP;        // [32][RS_PP]  -X1
  double* Qs = P2 + RS_TM * RS_PP;        // [2][RS_QBUF] k-slices of W / L

  const int tid = (int)threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const long bz = (long)blockIdx.y;
  const int row0 = (int)blockIdx.x * RS_TM;
  double* Ag = a.A + bz * a.sA + (long)row0 * a.lda;
  const double* Wg = a.W + bz * a.sW;
  const double* Lg = a.L + bz * a.sL;
  const int nrow = min(RS_TM, a.rows - row0);     // rows of this tile that exist

  // A -> P1: thread t carries 16-byte chunks (t & 7) + 8 p of row t >> 3
  {
    const int r = tid >> 3, c2 = (tid & 7) * 2;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      d2 v = {0.0, 0.0};
      if (r < nrow) v = *(const d2*)(Ag + (long)r * a.lda + c2 + 16 * p);
      *(d2*)(P1 + r * RS_PP + c2 + 16 * p) = v;
    }
  }

  // slice gs of the stream W, L, W: 128 x 16 (forward: rows n, k contiguous) or 16 x 128 (TRANS: rows k, n contiguous) of the lower triangle
  const int arow = tid >> 3, acp = (tid & 7) * 2;     // forward staging coordinates: 8 lanes x 16 B per 128-byte row slice, rows arow + 32 p
  const int bkr = tid >> 6, bcp = (tid & 63) * 2;     // TRANS: 64 lanes x 16 B per k-row, k-rows bkr + 4 p
  d2 vq[RS_PD][4];
  auto gload = [&](int gs, int q) {
    const double* Q = (gs >= 8 && gs < 16) ? Lg : Wg;
    const long ldq = (gs >= 8 && gs < 16) ? a.ldl : a.ldw;
    const int k0 = (gs & 7) * 16;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // element (i, j) of the block is stored, and non-zero, only for j <= i
      const int i = TRANS ? k0 + bkr + 4 * p : arow + 32 * p;
      const int j = TRANS ? bcp : k0 + acp;
      d2 v = {0.0, 0.0};
      if (j <= i) {
        v = *(const d2*)(Q + (long)i * ldq + j);
        if (j + 1 > i) v[1] = 0.0;
      }
      vq[q][p] = v;
    }
  };
  auto sstore = [&](int buf, int q) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (TRANS) *(d2*)(Qs + buf * RS_QBUF + (bkr + 4 * p) * RS_QT + bcp) = vq[q][p];
      else *(d2*)(Qs + buf * RS_QBUF + (arow + 32 * p) * RS_QN + acp) = vq[q][p];
    }
  };

  d4 acc[2][2], x1[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  // register prefetch, RS_PD slices deep as in gemm_tile_body's small tiles: a slice costs max(MFMA time, global latency / RS_PD).  Invariant at
  // slice gs: LDS buffer gs & 1 holds slice gs, register set (gs + j) % RS_PD holds slice gs + j for 1 <= j < RS_PD, set gs % RS_PD is free
#pragma unroll
  for (int q = 0; q < RS_PD; ++q) gload(q, q);
  sstore(0, 0);
  __syncthreads();
#pragma unroll 1
  for (int ph = 0; ph < 3; ++ph) {
    const double* Pop = ph == 1 ? P2 : P1;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int gs = ph * 8 + s, buf = gs & 1, q = s % RS_PD;      // (8 slices per product, RS_PD divides 8: gs % RS_PD == s % RS_PD)
      if (gs + RS_PD < 24) gload(gs + RS_PD, q);
      const double* Ab = Pop + lr * RS_PP + s * 16 + lq;
      const double* Bb = TRANS ? Qs + buf * RS_QBUF + lq * RS_QT + wn * 32 + lr : Qs + buf * RS_QBUF + (wn * 32 + lr) * RS_QN + lq;
      // 16-column block cb = 2 wn + j of the output meets non-zero k only in slices s <= cb (forward) / s >= cb (TRANS)
      const bool on0 = TRANS ? s >= 2 * wn : s <= 2 * wn;
      const bool on1 = TRANS ? s >= 2 * wn + 1 : s <= 2 * wn + 1;
      if (on0 || on1) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double a0 = Ab[kk * 4], a1 = Ab[16 * RS_PP + kk * 4];
          if (on0) {
            const double b0 = TRANS ? Bb[kk * 4 * RS_QT] : Bb[kk * 4];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
          }
          if (on1) {
            const double b1 = TRANS ? Bb[kk * 4 * RS_QT + 16] : Bb[16 * RS_QN + kk * 4];
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
          }
        }
      }
      if (gs + 1 < 24) sstore(buf ^ 1, (q + 1) % RS_PD);
      __syncthreads();
    }
    if (ph == 2) break;
    // hand-over between two products, in the accumulator layout (row = i 16 + lq + 4 r, column = wn 32 + j 16 + lr).  The barrier that
    // closed slice 7 has every wave's operand reads of this product behind it.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = (i * 16 + lq + 4 * r) * RS_PP + wn * 32 + j * 16 + lr;
          if (ph == 0) {               // X1: keep, -X1 -> P2, start product 2 from A
            x1[i][j][r] = acc[i][j][r];
            P2[o] = -acc[i][j][r];
            acc[i][j][r] = P1[o];
          } else {                     // R -> P1 (each entry of A was read by the thread that now overwrites it), start product 3 from X1
            P1[o] = acc[i][j][r];
            acc[i][j][r] = x1[i][j][r];
          }
        }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = i * 16 + lq + 4 * r;
        if (rr < nrow) Ag[(long)rr * a.lda + wn * 32 + j * 16 + lr] = acc[i][j][r];
      }
}

}  // namespace sigp
