/*
 * sigp_debug.h -- micro-benchmark / diagnostic entry points of libsigp.so (NOT part of the drop-in ABI of sigp.h).
 * They exist so that single kernels can be timed and ablated on the GPU box from tools/*.py; nothing in
 * seaiceextentforecasting_amd/ binds them.
 */
#ifndef SIGP_DEBUG_H
#define SIGP_DEBUG_H
#include "sigp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* wall-clock phase stamps of one potrf_diag_kernel launch (tools/diag_phases.py) */
int sigp_debug_diag_stamps(sigp_handle* h, const double* A128, double* out_us, int nout);
/* time potrf_diag_kernel on one 128x128 SPD block; `skip` bit mask switches phases off (tools/diag_bench.py) */
int sigp_debug_time_diag(sigp_handle* h, const double* A128, int skip, int reps, double* ms_avg, double* L_out, double* Linv_out);
/* time the covariance build for nb lockstep members of order n; flags: 2 no covariance function, 4 no store (tools/kbuild_bench.py) */
int sigp_debug_time_kbuild(sigp_handle* h, int n, int d, int nb, int kernel_id, int flags, int reps, double* ms_avg);
/* sustained v_mfma_f64_16x16x4_f64 rate; seed < 0: pseudo-random operands (tools/mfma_peak.py) */
int sigp_debug_mfma_peak(sigp_handle* h, int blocks, int iters, double* tflops, double seed);
/* time the lower-tile update on a synthetic panel: rt row tiles, depth K; small = 0 generic 128-tile kernel,
 * 1 generic 64-tile kernel, 2 syrk128_kernel; dbg = ablation bits; clock_ghz = in-kernel clock (tools/syrk_bench.py).
 * Measurement bits of syrk128_kernel: 256 phase stamps (prologue / K loop / epilogue cycles, turnaround, on stderr); 1024 one workgroup
 * per CU (extra dynamic LDS, same code); 2048 persistent walk of the product instantiation, one workgroup per slot; 4096 (with 256) per-CU
 * timeline of the last launch; 8192 / 16384 wave priority 3 outside / inside the K loop */
int sigp_debug_time_syrk(sigp_handle* h, int rt, int K, int patch, int small, int reps, double* ms_avg, double* tflops, int dbg,
                         double* clock_ghz);
/* do small kernels on different streams overlap? (tools/stream_conc.py) */
int sigp_debug_stream_concurrency(sigp_handle* h, int nstreams, int reps, int blocks, int iters, int use_slot_streams, double* ms_out);
/* which CUs does a hipExtStreamCreateWithCUMask mask enable? out2[2*b] = XCC_ID, out2[2*b+1] = HW_ID of block b (tools/cumask_probe.py) */
int sigp_debug_cumask_probe(sigp_handle* h, const unsigned* mask8, int blocks, unsigned* out2);

/*
 * Run-and-return entries (tests/test_hip_tile_primitives.py): the caller's HOST operands go to the device, exactly ONE launch is issued
 * through the launcher the engine uses (no ablation bits, no stamps, plain tile walk), and the output buffer comes back WHOLE, so that
 * gaps and tiles the descriptor does not own can be inspected.  dtype = SIGP_F64 / SIGP_F32 (the element type of every buffer).
 * Every entry checks its descriptor against the buffer sizes given in elements and returns SIGP_BAD_ARG, launching nothing, for a
 * descriptor that would read or write outside them, for a row or member stride that is not a multiple of 16 bytes, for K that is not a
 * positive multiple of the K-slice (16 doubles / 32 floats), and for what the kernels do not implement: ktri = 2 outside the plain walk
 * of gemm_mfma_kernel, ktri with `auto`, zshift without a lower walk or with ktri = 1, a tile whose triangular k span is empty, a ride
 * row with more than 16 rows in use, members that share output tiles.
 *
 * sigp_debug_run_gemm: C (-)= A B^T over the tile window (r0, r1, c0, c1) of GemmArgsT, in units of cfg's tile.  cfg:
 *   0  32x128 SET          1  32x128 SET, B transposed      2  32x128 SETNEG, B transposed
 *   3  64x64 SET           4  64x64 SUB                     5  64x64 SUB, B transposed
 *   6  128x128 SUB         7  128x128 SETNEG, B transposed  8  32x32 SUB
 *   9  syrk128 SUB (launch_syrk128_t: option diag_tiles picks the diagonal-skip instantiation as in a fit)   10  syrk128 SET
 *   11 auto (gemm_sub_auto with the handle's small_tile_threshold / tiny_tile_threshold; window in 128-units)
 * B = NULL or B == A: ONE operand of a_elems elements (the launch sees the same device pointer on both sides; ldb, sB, zB as given).
 * zshift shifts the trapezoid of member y of the `batch` axis (blockIdx.y) down by zshift * y tile rows.
 */
int sigp_debug_run_gemm(sigp_handle* h, int dtype, int cfg, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int K, int r0, int r1,
                        int c0, int c1, int lower, int ktri, int batch, int64_t sA, int64_t sB, int64_t sC, int zcount, int64_t zA, int64_t zB, int64_t zC,
                        int zshift, int ride_bi1, int ride_rows, int64_t a_elems, int64_t b_elems, int64_t c_elems);
/* panel_strip_kernel: strips rb0 .. rb0 + nstrips - 1 (128-row blocks of M) of the panel of block columns [J, J + Wp), Mt = [Wp * 128][ldm] per member;
 * option strip_tri picks the instantiation.  M comes back whole. */
int sigp_debug_run_strip(sigp_handle* h, int dtype, void* M, int64_t ld, const void* Mt, int64_t ldm, int rb0, int nstrips, int J, int Wp, int members, int64_t sM,
                         int64_t sMt, int64_t m_elems, int64_t mt_elems);
/* chain_link_kernel on block column c of M: block (c+1, c) is solved into `scratch` and applied to block (c+1, c+1), the rows_ride 128-row blocks
 * below it are solved in place.  M and scratch come back whole. */
int sigp_debug_run_link(sigp_handle* h, int dtype, void* M, int64_t ld, int c, const void* Linv, void* scratch, int rows_ride, int members, int64_t sM, int64_t sL,
                        int64_t sS, int64_t m_elems, int64_t linv_elems, int64_t scratch_elems);
/* refined_solve_kernel (option accurate_solve; fp64 only): A [rows][lda >= 128] per member is replaced, in ONE launch through launch_refined_solve, by
 * X = A W^T + (A - (A W^T) L^T) W^T (trans = 0: X L^T = A) or X = A W + (A - (A W) L) W (trans = 1: X L = A); W [128][ldw] the inverse block, L [128][ldl]
 * the diagonal block, of which only the lower triangle is read; members sA / sW / sL elements apart (sW, sL may be 0: one block for all).  Any
 * rows >= 1.  SIGP_BAD_ARG, nothing launched: a descriptor that leaves the buffers, a stride that is not a multiple of 16 bytes, members that
 * share rows.  A comes back whole. */
int sigp_debug_run_refined_solve(sigp_handle* h, int trans, void* A, int64_t lda, int rows, const void* W, int64_t ldw, const void* L, int64_t ldl, int members,
                                 int64_t sA, int64_t sW, int64_t sL, int64_t a_elems, int64_t w_elems, int64_t l_elems);
/* (the diagonal block: sigp_debug_time_diag with reps = 1, skip = 0 returns L and Linv of one block) */

/*
 * Run-and-return entries of the quadratic solve kernels (tests/test_hip_solve_kernels.py), same convention: host operands in, ONE launch with
 * the grid rule the engine uses, every buffer back whole; SIGP_BAD_ARG, nothing launched, for a descriptor that would read or write outside
 * the buffer sizes given in elements, for a row or member stride that is not a multiple of 16 bytes, and for a K (rowdot) or a column count
 * (coldot) that is not a multiple of the 16-byte vector width (2 doubles / 4 floats): the kernels load whole vectors.
 *
 * rowdot_kernel:  Zout[r][j] (-)= sum_k (Zin + Zadd)[r][k] Mx[j ld + k],  j < nrows, r < nrhs (1 .. 4);  kmode 0: k in [0, K), 1: [0, j],
 * 2: [j, K) (nrows <= K for 1 and 2);  sub = 1 subtracts from the prior content;  Zadd may be NULL (same shape as Zin; one member only: the
 * kernel has no member stride for it);  pm_pw > 0: Zout is panel-major [panel][4][pm_pw], entry of row g = j_off + j of right-hand side r at
 * ((g / pm_pw) 4 + r) pm_pw + g % pm_pw, otherwise row-major with ldzout;  `members` lockstep members sM / sZi / sZo elements apart.
 */
int sigp_debug_run_rowdot(sigp_handle* h, int dtype, const void* Mx, int64_t ld, int nrows, int K, int kmode, const void* Zin, int64_t ldzin, void* Zout, int64_t ldzout,
                          int nrhs, int sub, const void* Zadd, int pm_pw, int j_off, int members, int64_t sM, int64_t sZi, int64_t sZo, int64_t m_elems,
                          int64_t zin_elems, int64_t zout_elems);
/* coldot_kernel:  Zout[r][j] -= sum_{k < K} Zin[r][k] Mx[k ld + j],  j < ncols, r < nrhs (1 .. 4) */
int sigp_debug_run_coldot(sigp_handle* h, int dtype, const void* Mx, int64_t ld, int ncols, int K, const void* Zin, int64_t ldzin, void* Zout, int64_t ldzout, int nrhs,
                          int64_t m_elems, int64_t zin_elems, int64_t zout_elems);
/* The fp32 engine's block solves on the factor and inverse blocks the last single fp32 fit left on the handle.  rhs [nrhs][n] doubles (rounded to
 * fp32, pad rows zeroed, as a refinement step hands its residuals over) is replaced by  which = 0: L~^-1 rhs (f32_block_forward),
 * 1: L~^-T rhs (f32_block_backward),  2: L~^-T L~^-1 rhs (both). */
int sigp_debug_f32_solve(sigp_handle* h, int which, double* rhs, int64_t n, int nrhs);
/* which = 0: fU, the row-major inverse-transposes of the factor's 2048-column diagonal blocks;  1: fV, their transposes.  out [n_pad][n_pad] floats. */
int sigp_debug_f32_get_inverse(sigp_handle* h, int which, float* out);
/* The adjoint G = d score / d K~ of a hindcast score (include/sigp.h: sigp_hindcast_grad_ard) on the single fp64 fit the handle holds, by
 * sigp_hindcast_grad_ard's own launches up to its ARD pass: the lower 128-tiles into out [n][ldo] as the product wrote them (the
 * diagonal tiles whole: their two halves agree to rounding, not bit for bit), zeros in the tiles above.  criterion SIGP_LOO_NLPD /
 * SIGP_LOO_SSE; lead, min_train, sigma_mode as sigp_hindcast. */
int sigp_debug_run_hindcast_adjoint(sigp_handle* h, int64_t lead, int64_t min_train, int sigma_mode, int criterion, double* out, int64_t ldo);
/* ONE launch of W = U C (hindcast.hpp) on host operands, every buffer back whole: which = 0 hindcast_w_kernel, 1 hindcast_w_lds_kernel
 * (n_pad <= 8192).  U, Cb, W hold c_elems doubles each: member m's n_pad x n_pad matrix at m sC, rows ld >= n_pad apart (of U only the
 * entries i <= j < n are read, of Cb rows and columns below n; W comes in with the caller's sentinels and goes back whole: rows and columns
 * 0 .. n_pad of every member are written).  z, zbar hold z_elems doubles each, member m's [n] at m sZ.  1 <= n <= n_pad, n_pad a multiple
 * of 128, 1 <= lead <= 128, 1 <= members <= 8.  SIGP_BAD_ARG, nothing launched: a descriptor that leaves the buffers, members whose
 * matrices overlap, which = 1 beyond the LDS limit. */
int sigp_debug_run_hindcast_w(sigp_handle* h, int which, const double* U, const double* Cb, const double* z, const double* zbar, double* W, int n, int n_pad,
                              int64_t ld, int lead, int members, int64_t sC, int64_t sZ, int64_t c_elems, int64_t z_elems);

/*
 * Run-and-return entries of the score-gradient kernels (tests/test_hip_ard_pass.py, tests/test_hip_score_products.py), same convention: host
 * operands in, the engine's launches through the engine's launchers, every buffer back whole; SIGP_BAD_ARG, nothing launched, for a
 * descriptor that leaves the buffer sizes given in elements, a row or member stride that is not a multiple of 16 bytes, members whose
 * outputs overlap, and what the kernels do not implement.  fp64 handles only.
 *
 * sigp_debug_run_ard_pass: ONE call of ard_tile_pass_members<wsel> -- the memset of the centred copy, ard_center_kernel and
 * ard_grad_partial_kernel<8 | 32, wsel> (d <= 8 | d > 8, as the engine chooses) -- then the matching finish kernel (wsel = 0, ARD_W_NLML:
 * ard_grad_finish_kernel;  1, ARD_W_LOO: loo_ard_finish_kernel).  Per member m < members (<= 8):
 *   U        [n_pad][dp] at m sU: the scaled features, ZERO in rows >= n and columns >= d (the kernels read them); dp >= d rounded up to 16
 *   M        [n_pad][ld] at m sP: K~^-1 (wsel 0) or the adjoint matrix (1); only the lower 128-tiles' entries (i, j), j < i < n, and the
 *            diagonal i < n (finish kernel) enter the results
 *   vec      wsel 0: a [n_pad] at m sVec;  wsel 1: a LooArdVecs arena at m sVec -- a at 0, v at 3 n_pad, eps at 4 n_pad (4 n_pad + 1 doubles;
 *            beta and gamma between them are not read).  Entries >= n of a and v do not enter the results
 *   q        wsel 0: q[m sQ] = y^T a (sf = q / n);  wsel 1: not read, may be NULL
 *   sn, sn_m the noise factor of the last gradient component: sn_m [members] if not NULL, else sn for every member
 *   Uc       OUT [(members - 1) sU + n_pad dp]: the centred copy as the pass left it (the entry sizes the handle's workspace itself)
 *   partial  IN/OUT [tiles = T (T + 1), T = n_pad / 128][dp] at m sPartial: columns < d rounded up to 16 are written, the rest keeps the
 *            caller's sentinels
 *   grad     IN/OUT [d + 1] at m sGrad
 * kernel_id = SIGP_KERNEL_RBF / SIGP_KERNEL_MATERN52.  n_pad a multiple of 128, <= 4096; d <= 1024.
 */
int sigp_debug_run_ard_pass(sigp_handle* h, int wsel, int kernel_id, int n, int n_pad, int d, int dp, int members, const double* U, int64_t sU, int64_t u_elems,
                            const double* M, int64_t ld, int64_t sP, int64_t m_elems, const double* vec, int64_t sVec, int64_t vec_elems, const double* q, int64_t sQ,
                            int64_t q_elems, double sn, const double* sn_m, double* Uc, double* partial, int64_t sPartial, int64_t partial_elems, double* grad,
                            int64_t sGrad, int64_t grad_elems);
/* ONE launch of cv_band_product_kernel through the launcher sigp_cv_grad_ard uses: C = P B on T x T 128-tiles, every tile written whole.
 * P and C [128 T][ld] per member, both sP apart (the kernel has one member stride for the two); band [128 T][384] per member, sBand apart:
 * row i holds the three 128-column blocks of B around its own.  Tile (bi, bj) reads block columns max(bj - 1, 0) .. min(bj + 2, T) of P's
 * block row bi and the matching band columns of block row bj -- nothing else.  T <= 32, members <= 8.  C comes back whole. */
int sigp_debug_run_cv_band(sigp_handle* h, const double* P, const double* band, double* C, int T, int64_t ld, int members, int64_t sP, int64_t sBand, int64_t p_elems,
                           int64_t band_elems, int64_t c_elems);
/* predcov_partial_kernel through the launcher sigp_predict_cov uses, then -- finish != 0 -- predcov_finish_kernel, with sigp_predict_cov's
 * tile descriptor.  Z [m_pad][ldz >= 128 nkb]; slice s of S covers block columns [s nkb / S, (s + 1) nkb / S).  S = 1: the in-place form (the
 * lower tiles' products go to C, part is not touched);  1 < S <= nkb: the workspace form, part [S][P][128][128], P = c (c + 1) / 2,
 * c = m_pad / 128.  The finish step writes C = sigma_f (prior + [i == j and noise] sn - sum_s partial_s), mirrored.  Prior: the symmetric part
 * of Kss [m_pad][ldk] if not NULL, else the unit covariance kernel_id (RBF / MATERN52, length scale ell) of Xs [m_pad][dp >= d].
 * part [part_elems] and C [m_pad][m_pad] come in with the caller's sentinels and go back whole.  m_pad a multiple of 128, <= 2048. */
int sigp_debug_run_predcov(sigp_handle* h, const double* Z, int64_t ldz, int m_pad, int nkb, int S, int finish, const double* Xs, int dp, int d, const double* Kss, int64_t ldk,
                           int kernel_id, double ell, double sn, double sigma_f, int noise, double* part, double* C, int64_t z_elems, int64_t xs_elems, int64_t kss_elems,
                           int64_t part_elems, int64_t c_elems);
#ifdef __cplusplus
}
#endif
#endif
