/*
 * sigp.h -- C ABI of the MI355X-native Gaussian-process engine (libsigp.so).
 *
 * Drop-in boundary for the GPR hot path of William-gregory/SeaIceExtentForecasting.  The reference has
 * no function boundary there: the path is the inline statement block
 *     north/June1st.py:231-277   (M ... fvar)          and the closure
 *     north/June1st.py:235-257   MLII(hyperparameters) -> (nlML, grad[2])
 * repeated byte-identically in all 14 forecast scripts.  Each entry point below cites
 * the statements it replaces.  Binding on the reference side is ctypes.
 *
 * Conventions
 *   - plain C, no C++ exceptions cross the ABI; every call returns SIGP_OK / SIGP_NOT_SPD /
 *     SIGP_BAD_ARG / SIGP_HIP_ERROR; message via sigp_last_error().
 *   - host arrays are row-major float64 (NumPy C order) owned by the caller; the library owns all
 *     device memory and frees it in sigp_destroy().
 *   - one handle = one GPU + its streams and workspaces.  Calls on a handle are serialised on its
 *     streams and are synchronous on return; a handle is NOT thread-safe, distinct handles are
 *     independent.
 *   - there is no CPU fallback: without a usable HIP device sigp_create() fails with SIGP_HIP_ERROR.
 */
#ifndef SIGP_H
#define SIGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sigp_handle sigp_handle;

enum { SIGP_OK = 0, SIGP_NOT_SPD = 1, SIGP_BAD_ARG = 2, SIGP_HIP_ERROR = 3 };
enum { SIGP_F64 = 0, SIGP_F32 = 1 };
/* covariance functions: 0 is the reference's own (north/June1st.py:264-265); 1,2 are the kernels
 * BASELINE.json's configs add on the same fit/solve/predict skeleton. */
enum { SIGP_KERNEL_NETDIFFUSION = 0, SIGP_KERNEL_RBF = 1, SIGP_KERNEL_MATERN52 = 2 };
/* sigp_get_matrix selectors */
enum { SIGP_MAT_K = 0, SIGP_MAT_L = 1 };
/* kernel classes for sigp_profile_get (one per device kernel, so totals line up with rocprofv3 --stats):
 * kbuild_kernel(+ride_build), potrf_diag_kernel, gemm_mfma_kernel<32,128> (panel solve),
 * gemm_mfma_kernel<64,64> (updates with few tiles), syrk128_kernel (inner + trailing updates), epilogue_kernel */
enum { SIGP_KC_KBUILD = 0, SIGP_KC_DIAG = 1, SIGP_KC_TRSM = 2, SIGP_KC_UPDATE_SMALL = 3,
       SIGP_KC_SYRK128 = 4, SIGP_KC_EPILOGUE = 5, SIGP_KC_SMALL = 6 /* smallgp_kernel */,
       SIGP_KC_MLII = 7 /* triangular inversion + U U^T of sigp_nlml_grad; triangular inversion + row pass of sigp_loo; triangular inversion + the fold steps of sigp_cv; + U U^T, the triangular product and the n^2 passes of sigp_loo_grad; triangular inversion + U U^T + the tile pass of sigp_nlml_grad_ard; sigp_loo's two + U U^T, the n^2 passes, the product P diag(gamma) P and the tile pass of sigp_loo_grad_ard; sigp_cv's entries + per pass the fold adjoints and their assembly, then U U^T, the n^2 passes, the banded product P B, the product (P B) P and the tile pass of sigp_cv_grad_ard; the scan and the row pass of sigp_hindcast; + the adjoint's n^2 passes, triangular inversion, W = U C, the product U W^T and the tile pass of sigp_hindcast_grad_ard */, SIGP_KC_COUNT = 8 };

#define SIGP_MAX_RIDE 127 /* test points that can ride along one factorisation */

int sigp_version(void);
/* "HIP runtime <version> (<status>) from <path of the libamdhip64 that serves this process>" -- for error reports: a process that
 * also loads PyTorch-ROCm has two HIP runtimes on disk, and whichever is mapped first serves everyone. */
int sigp_runtime_info(char* buf, int64_t len);

/* lifetime ------------------------------------------------------------------------------------ */
int sigp_create(sigp_handle** h, int device_id, int dtype);
int sigp_destroy(sigp_handle* h);
const char* sigp_last_error(const sigp_handle* h);

/* data staging: the enclosing-scope variables the reference block reads ------------------------- */
/* X [n,d] (row stride ldx), y [n]:  north/June1st.py:214, 226-229 (y, X).  Copies host -> HBM. */
int sigp_set_train(sigp_handle* h, const double* X, int64_t n, int64_t d, int64_t ldx, const double* y);
/* Xs [m,d], m <= SIGP_MAX_RIDE: the test row(s) north/June1st.py:228 (Xs).  These "ride along" the
 * factorisation as extra right-hand-side rows, so fit+predict needs no separate triangular solve.
 * m = 0 clears them. */
int sigp_set_test(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs);

/* K5: kernel-matrix build  K~ = k(X,X) + sn_tilde*I  into HBM (lower triangle), plus the ride-along
 * rows [y ; k~(Xs,X)].  Replaces north/June1st.py:265 (the multi_dot + eye term).
 * RBF / Matern-5/2: ell is the length scale.  */
int sigp_kernel_build(sigp_handle* h, int kernel_id, double ell, double sn_tilde);
/* Reference kernel: host passes Sigma~ = expm(ell*M) [N,N] (north/June1st.py:264; N = d of set_train);
 * device forms X Sigma~ X^T + sn_tilde*I (north/June1st.py:265). */
int sigp_kernel_build_from_sigma(sigp_handle* h, const double* Sigma, int64_t ldsigma, double sn_tilde);

/* K6: blocked Cholesky  K~ = L~ L~^T  in place (north/June1st.py:265 np.linalg.cholesky).
 * info: 0, or LAPACK-style 1-based index of the first non-positive pivot (-> SIGP_NOT_SPD).
 *
 * Accuracy (fp64 engine; measured, tests/test_hip_conditioning.py, docs/EXPERIMENTS.md "Conditioning").  The 128 x 128 diagonal blocks are
 * factored to LAPACK's residual whatever their conditioning.  The rows below a diagonal block are NOT solved by substitution but multiplied
 * by the explicitly inverted block, and the later solves (alpha~, predictions, U = L~^-T behind loo / cv / the gradients) are products with
 * inverses as well: such a product carries an error proportional to cond of the inverted block, where substitution is backward stable.
 * The factor's residual rho = ||L~ L~^T - K~||_F / ||K~||_F therefore depends on cond(K11) of the diagonal blocks, not on cond(K~):
 *     cond(K11) <= 1e8  (any cond(K~) up to 1e14 tested)   rho = 3e-16 .. 1e-15     LAPACK on the same matrices: 2e-16 .. 6e-16
 *     cond(K11) ~ 1e6                                       rho ~ 1e-15
 *     cond(K11) ~ 1e10                                      rho ~ 5e-14              (about 100 to 200 times LAPACK's)
 *     cond(K11) ~ 1e13                                      rho = 1e-12 .. 8e-12, or SIGP_NOT_SPD at a pivot of the block AFTER the ill-conditioned
 *                                                           one, on matrices that LAPACK factors with minimum pivot ~ sn~
 * and alpha~, sigma_f, nlML, the predictions, loo / cv and the gradients lose the same factor against an fp64 LAPACK fit of the same matrix.
 * A smooth kernel on ordered, densely sampled inputs (RBF / Matern, long length scale) puts cond(K11) within a factor 3 of cond(K~) ~ n / sn~
 * (the three rows above: sn~ = 1e-4, 1e-8, 1e-11 at l = 3 on 257 .. 640 sorted points of [0, 10]).  A matrix of the same cond(K~) whose
 * diagonal blocks are benign is not affected.
 *
 * Option "accurate_solve" = 1 (sigp_set_option; off by default, fp64 engine, single-GPU fits and lockstep groups) puts ONE residual-correction step
 * behind every such product with an inverted 128 x 128 diagonal block:  X1 = A W^T, R = A - X1 L^T, X = X1 + R W^T  (W the stored inverse, L the
 * diagonal block itself, of which only the lower triangle is read), all three products in one launch per block column with A, X1 and R held on
 * chip (csrc/refined_solve.hpp).  Covered: the column solves of the factorisation -- the ride-along rows with them, so z = L~^-1 y and
 * v = L~^-1 k* --, the forward block solves of sigp_predict / sigp_predict_cov and the backward block solves of sigp_get_alpha.  With it, on the
 * same matrices (measured, tests/test_hip_accurate_solve.py, docs/EXPERIMENTS.md "Accurate solves"):
 *     cond(K11) ~ 1e6, 1e10, 1e13 (sn~ = 1e-4, 1e-8, 1e-11)      rho <= 1.3 times LAPACK's; every matrix factors (sn~ = 1e-13 included)
 *     alpha~, sigma_f, nlML, predictions (ride-along and general)    within 5.1 times LAPACK's error against a long-double fit
 *     loo, cv, the exact MLII gradient                               within 5.3 times LAPACK's (their U = L~^-T and fold solves stay explicit inverses,
 *                                                                    by nature; they start from an accurate factor)
 * What the option overrides while it is on: "panel_mode" (every panel as panel_mode 0: a strip solve is a product with the inverse of a panel's
 * whole top triangle) and bit 2 of "panel_chain" (no fused link: its column solve is a plain product); the other bits of panel_chain, "schedule"
 * and "outer_blocks" keep their meaning, and the first two their "same bits" guarantee.  With the option at 0 the library issues exactly the
 * launches it issues without this paragraph.  Cost: the column solves triple their flops (they are about 384 / n of a fit's) and single fits lose
 * the fused link; measured in docs/EXPERIMENTS.md.  Out of scope: the fp32 engine (sigp_set_option answers SIGP_BAD_ARG on an fp32 handle; it
 * refines against K~ itself), sharded fits (sigp_dist_fit with the option set: SIGP_BAD_ARG), sigp_small_*, and U = L~^-T by recursive doubling
 * with the fold solves of sigp_cv (see above). */
int sigp_potrf(sigp_handle* h, int64_t* info);

/* K7,K8,K12: A~ = K~^-1 y, sigma_f = y^T A~/n (north/June1st.py:266-268), nlML (north/June1st.py:246).
 * Requires sigp_potrf. */
int sigp_fit(sigp_handle* h, double* sigma_f, double* nlml);

/* K9-K11 for the ride-along test rows: mean[m], var[m] (var includes sigma_n: north/June1st.py:272-277). */
int sigp_predict_ride(sigp_handle* h, double* mean, double* var);
/* K9-K11 for arbitrary new test points after a fit (any m): cross-kernel build + forward solve. */
int sigp_predict(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, double* mean, double* var);

/* The JOINT posterior of m new test points after a fit: the mean and the full m x m covariance (what every GP library returns for
 * return_cov=True; the variances of north/June1st.py:273, :277 are its diagonal).  With Z = k~(Xs, X) L~^-T (the solved rows sigp_predict
 * reduces to their squared norms) and z = L~^-1 y:
 *     mean_j = Z_j . z        (the same launches as sigp_predict: the same bits)
 *     cov_ij = sigma_f (k~**(xs_i, xs_j) + [i == j and noise] sn~ - Z_i . Z_j)
 * noise != 0: the covariance of the observations y* (sigma_n = sn~ sigma_f on the diagonal, so diag(cov) is sigp_predict's var); noise == 0:
 * of the latent f*.  mean [m], cov [m][ldc >= m] row-major, the full matrix, bitwise symmetric.  k~** is the unit prior of the fit's
 * kernel (RBF / Matern: diagonal exactly 1; reference kernel: Xs Sigma~ Xs^T formed on the device).  Cost: the forward solve of
 * sigp_predict, n^2 m flops (m triangular solves), + the product Z Z^T, n m^2 flops (lower tile pairs of 128 x 128, K split over "cov_slices" slices whose
 * partial tiles are added in a fixed order: the same bits on every run for a given slice count) + m^2 prior entries.  Device memory:
 * 8 m_pad (n_pad + m_pad) bytes (+ 128 KiB per partial tile), m_pad = m rounded up to 128.  Device work is accounted under SIGP_KC_KBUILD
 * (rows), SIGP_KC_TRSM (one entry per lockstep solve group) and SIGP_KC_EPILOGUE (the product and the finishing pass, one entry each).
 * 1 <= m <= SIGP_MAX_COV.  fp64 engine, any of the three kernels, after sigp_fit / sigp_fit_predict; on an fp32 handle or after a sharded
 * fit (sigp_dist_fit): SIGP_BAD_ARG.  The factor and the fit's state are only read: sigp_predict / sigp_get_alpha / sigp_loo afterwards
 * return what they returned before. */
#define SIGP_MAX_COV 8192
int sigp_predict_cov(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, int noise, double* mean, double* cov, int64_t ldc);

/* Inducing-point (sparse) GP regression for n past the dense limit: the DTC predictive with Titsias' collapsed variational bound ("SGPR").
 * K = sigma_f (k + sn~ I) with k the unit-variance RBF or Matern-5/2 covariance, data X [n][ldx] and y [n], m inducing points Z [m][ldz],
 * jitter eps >= 0, sn~ > 0; sigma_f is profiled as in the dense fit.  Whitened form (never the normal equations sn~ K_mm + K_mn K_nm, which
 * square the conditioning):
 *     L  = chol(k(Z,Z) + eps I)                     m x m
 *     V  = L^-1 k(Z,X)                              m x n, never held whole: chunks of "sparse_chunk" columns, ascending
 *     B  = sn~ I + V V^T,  L_B = chol(B)            m x m
 *     b  = V y,  w = L_B^-1 b,  t = |V|_F^2,  yy = y^T y
 *     sigma_f = (yy - w^T w) / (sn~ n)
 *     1/2 log|Q~ + sn~ I| = 1/2 (n - m) log sn~ + sum log diag(L_B)
 *     nlml  = n/2 + 1/2 log|Q~ + sn~ I| + n/2 log sigma_f + n/2 log 2 pi        (the dense fit's expression with the DTC determinant)
 *     bound = nlml + (n - t) / (2 sn~)                                            (the collapsed bound: >= nlml, equal when Z = X, eps = 0;
 *                                                                                  n - t is summed as the column deficits 1 - |V[:, j]|^2)
 * and at a new point x*, with p = L^-1 k(Z,x*), q = L_B^-1 p:
 *     mean = q^T w,   var = sigma_f (1 + sn~ - p^T p + sn~ q^T q)                (the noise included, as in sigp_predict)
 * X, y, Z, Xs are HOST pointers; X and y are streamed chunk by chunk.  sigp_set_train and the handle's dense state are not involved: a sparse
 * fit clears built / factored / fitted, so sigp_predict, sigp_loo, ... refuse as before any fit, and a later dense fit returns what a fresh
 * handle returns (sigp_sparse_predict then refuses).  nell = 1: isotropic length scale ell[0]; nell = d: per-feature scales -- the chunks, Z
 * and Xs are divided by them while they are staged and the kernel runs at unit length scale (the bits of the isotropic fit at ell = 1 on
 * pre-divided inputs).  kernel_id: SIGP_KERNEL_RBF or SIGP_KERNEL_MATERN52.  n < m is legal.  out [4] = { sigma_f, nlml, bound, info }.
 * SIGP_BAD_ARG (the limit is named in sigp_last_error): an fp32 handle, the reference kernel, nell not 1 or d, a length scale or sn~ <= 0,
 * jitter < 0, m outside 1 .. SIGP_SPARSE_MAX_INDUCING, n < 1.  SIGP_NOT_SPD: k(Z,Z) + eps I (duplicate inducing points without jitter) or B
 * is not positive definite; out = { inf, inf, inf, pivot }; the handle stays usable.
 * Every sum has one chain of additions in ascending chunk order (no atomics): the same bits on every run; another sparse_chunk is another
 * summation order (agreement to rounding).  Cost about 2 n m^2 flops on the matrix pipe + n m covariances; device memory
 * 8 (2 (m_pad + 128) m_pad + m_pad chunk + chunk (dp + ldx + 1)) bytes.  Device work is accounted under SIGP_KC_KBUILD (k(Z,Z), k(Z,X_c)),
 * SIGP_KC_TRSM (the whitening), SIGP_KC_SYRK128 (V_c V_c^T) and the factorisations' own classes.
 * Not covered: gradients, optimising Z, FITC, fp32, lockstep batches, sharded fits, the reference kernel, predict_cov / loo / cv / hindcast. */
#define SIGP_SPARSE_MAX_INDUCING 8192
int sigp_sparse_fit(sigp_handle* h, int kernel_id, const double* ell, int64_t nell, double sn_tilde, double jitter,
                    const double* X, int64_t n, int64_t d, int64_t ldx, const double* y,
                    const double* Z, int64_t m, int64_t ldz, double* out /* [4]: sigma_f, nlml, bound, info */);
/* mean [ms], var [ms] at the rows of Xs [ms][ldxs >= d] (host) from the last sigp_sparse_fit: lockstep groups of up to 16 chunks of 128 points. */
int sigp_sparse_predict(sigp_handle* h, const double* Xs, int64_t ms, int64_t ldxs, double* mean, double* var);

/* Fused hot path: build -> potrf -> fit -> predict_ride with one host synchronisation.
 * Sigma may be NULL unless kernel_id == SIGP_KERNEL_NETDIFFUSION.
 * out[4] = { sigma_f, nlml, (double)info, sigma_n };  mean/var [m_ride] may be NULL when m_ride == 0. */
int sigp_fit_predict(sigp_handle* h, int kernel_id, double ell, double sn_tilde, const double* Sigma,
                     int64_t ldsigma, double* out, double* mean, double* var);

/* Batch of independent fits that share (n, d, m): the retrospective loop over years
 * (north/retrospective_forecasts/September1st_retro.py:176-248) and the hyper-parameter grid
 * (north/June1st.py:210-211).  Problem b uses X + b*strideX, y + b*stridey, Xs + b*strideXs
 * (a stride of 0 shares the array between problems, e.g. one data set x many grid points).
 * RBF / Matern only.  out [batch,4], mean/var [batch,m].  Fits are pipelined over `concurrency`
 * stream sets (1..16) so one fit's panel factorisations overlap another's trailing updates. */
int sigp_fit_batch(sigp_handle* h, int64_t batch, int kernel_id, const double* X, int64_t strideX,
                   const double* y, int64_t stridey, const double* Xs, int64_t strideXs, int64_t n,
                   int64_t d, int64_t m, const double* ell, const double* sn_tilde, int concurrency,
                   double* out, double* mean, double* var);
/* The same batch in two steps: sigp_batch_upload copies the data sets (host pointers, same layout/strides as
 * sigp_fit_batch) into HBM once, where they stay resident; sigp_batch_run then runs fits [first, first+count) on the
 * resident data (fit i uses data set i % batch) -- the timed region of bench.py is one sigp_batch_run call. */
int sigp_batch_upload(sigp_handle* h, int64_t batch, const double* X, int64_t strideX, const double* y,
                      int64_t stridey, const double* Xs, int64_t strideXs, int64_t n, int64_t d, int64_t m);
/* allocate the lockstep slots for (group, concurrency) ahead of time, so no allocation falls inside a timed batch_run */
int sigp_batch_reserve(sigp_handle* h, int64_t group, int concurrency);
int sigp_batch_run(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell,
                   const double* sn_tilde, int concurrency, double* out, double* mean, double* var);

/* The reference's OWN kernel at the reference's OWN size, batched: the retro loop
 * (north/retrospective_forecasts/September1st_retro.py:176-248: 3 regions x ~40 years of independent fits, n = year - 1979 <= 45)
 * times the 20 x 20 (l, sn~) grid of north/June1st.py:210-211 -- ONE WORKGROUP PER FIT, everything in LDS, one launch for the lot.
 * Each fit is north/June1st.py:264-277 + :246: K~ = X expm(l M) X^T + sn~ I, Cholesky, A~, sigma_f, k*, k**, fmean, fvar, nlML.
 * Data sets are ragged (n, N, m per set, 1 <= n <= 128, 0 <= m <= 8) and staged once in factored form (one
 * eigendecomposition per data set serves every l of the grid):
 *   A   [(n+m)][N] = [X ; Xs] Q      lam [N] = eigenvalues of M = Q diag(lam) Q^T        (lam_mode 0: weights exp(l lam_k))
 *   A   [(n+m)][N] = [X ; Xs] U      lam [N] = eigenvalues of a host-side Sigma~ = U diag(lam) U^T   (lam_mode 1: weights lam_k;
 *                                    this is how scipy's Pade expm(l M) -- the reference's own numbers at l = 3.1e10 -- goes through)
 * so that K~ = A_train diag(w) A_train^T + sn~ I.  Pools are flat double arrays; *_off give each set's start (in doubles).
 * sigp_small_run: fit i uses data set set_index[i] with (ell[i], sn_tilde[i]); out [nprob][4] = sigma_f, nlML, info, sigma_n
 * (info > 0: LAPACK pivot index, other entries +inf, mean/var NaN -- north/June1st.py:254-256); mean / var [nprob][mstride]. */
int sigp_small_upload(sigp_handle* h, int64_t nsets, const int64_t* n, const int64_t* N, const int64_t* m, const int32_t* lam_mode,
                      const double* A_pool, const int64_t* A_off, const double* y_pool, const int64_t* y_off,
                      const double* lam_pool, const int64_t* lam_off);
int sigp_small_run(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde,
                   double* out, double* mean, double* var, int64_t mstride);
/* The same launch with the MLII closure's second return value (north/June1st.py:235-257, the call the reference left commented out at
 * :259-262 `minimize(MLII, x0, method='CG', jac=True)`), for every (data set, theta) of the list at once: out8 [nprob][8] =
 * sigma_f, nlML, info, sigma_n, then the reference's own 2-vector "gradient" (:248-252: tr(K^-1 dK)/2 - alpha^T dK alpha/2 with
 * dKdl = X (M Sigma) X^T + sigma_n I, dKds = X Sigma X^T + sigma_f I -- NOT the derivative of nlML), then the exact
 * derivative of the profiled nlML w.r.t. (log l, log sn~).  A non-SPD K~ gives +inf in all of them (:254-256).  The inverse factor
 * L~^-1 is formed in LDS over L~; M Sigma~ = Q diag(lam exp(l lam)) Q^T needs no second matrix (lam_mode 0).  Sets staged with
 * lam_mode 1 (weights of a host-side Pade expm) need the derivative weights dlam_k = u_k^T M u_k * lam_k, given once per upload by
 * sigp_small_set_dweights (dlam_pool mirrors lam_pool: same offsets, `count` = its total length); without them their gradient is NaN. */
int sigp_small_set_dweights(sigp_handle* h, const double* dlam_pool, int64_t count);
int sigp_small_run_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde,
                        double* out8, double* mean, double* var, int64_t mstride);

/* The caller that produces the GP's features: ComplexNetworks.Network.tau (ComplexNetworks.py:31-47) on the device.
 * series [N][T] (row stride lds): the anomaly series of the N active grid cells.  Forms the N x N cell-to-cell correlation matrix
 * (np.corrcoef: one fp64 MFMA product of the standardised rows, clipped to [-1, 1], NaN on the diagonal) into R [N][N] (row stride
 * ldr; may be NULL) and returns the sum and the count of its entries with r >= 0 and r > r_crit -- the entries whose one-sided
 * t-test p-value (dof = T - 2) is below the significance level, r_crit = t_c / sqrt(dof + t_c^2), t_c = t.isf(significance, dof).
 * tau = sum / count. */
int sigp_corr_tau(sigp_handle* h, const double* series, int64_t N, int64_t T, int64_t lds, double r_crit, double* R, int64_t ldr,
                  double* sum_out, double* count_out);

/* ComplexNetworks.Network.intra_links (ComplexNetworks.py:298-309): the per-area anomaly series that become the GP's features.
 * data [P][T] pixel-major, weight [P] (sqrt(cell area) or sqrt(cos lat)), label [P] = area index 0..A-1 of the pixel or -1;
 * out [A][T] = sum over the area's pixels of data * weight (NaN products as 0), pixels added in ascending order. */
int sigp_area_sums(sigp_handle* h, const double* data, int64_t P, int64_t T, const double* weight, const int32_t* label, int64_t A, double* out);

/* ComplexNetworks.Network.area_level (ComplexNetworks.py:49-281) on the HOST (sequential greedy region growing + merging; no
 * handle, no GPU): the same decisions as the reference, in the same order, on means formed in np.nanmean's summation order, so the
 * areas are identical (csrc/area_level.cpp).  R [N][N]: the cell-to-cell correlations (NaN on the diagonal) of the N active cells;
 * node_of_cell [dimX*dimY]: row of R of a grid cell (row-major), -1 for an inactive one; cell_nan: flat index of the first NaN
 * cell of the data (the reference's out-of-bounds sentinel); tau: the threshold of sigp_corr_tau; latlon != 0: left / right
 * neighbours wrap.  Outputs (caller-allocated, N entries each, area_offsets N + 1): the areas in the reference's dict order --
 * area_ids[a] = its key, cells_out[area_offsets[a] .. area_offsets[a+1]) = its cells (flat indices) in list order -- and the
 * cells set aside by the merging step, in order (Network.unavail): at most unavail_cap of them are written, *n_unavail_out is the
 * full length (it can exceed N on a lat-lon grid; call again with a larger buffer then). */
int sigp_area_level(const double* R, int64_t N, const int32_t* node_of_cell, int64_t dimX, int64_t dimY, int32_t cell_nan, double tau,
                    int latlon, int32_t* cells_out, int64_t* area_offsets, int32_t* area_ids, int64_t* n_areas_out, int32_t* unavail_out,
                    int64_t unavail_cap, int64_t* n_unavail_out);
/* np.nanmean of a contiguous array in NumPy's own summation order (what sigp_area_level decides on; exported for its test) */
double sigp_host_nanmean(const double* a, int64_t n);

/* The step before the feature pipeline: detrend() of north/June1st.py:179-194 (one cut: cut_len = {T}) and of the retro
 * scripts (north/retrospective_forecasts/June1st_retro.py:178-195: one detrended cube per cut-off year) in ONE launch.
 * data [P][T] pixel-major anomaly series; cut c removes the least-squares line (scipy.stats.linregress semantics, NaN propagating)
 * fitted to the first cut_len[c] steps.  dt_out: the cuts' [P][cut_len[c]] blocks back to back; trend_out [ncuts][P][2] = slope, intercept. */
int sigp_detrend(sigp_handle* h, const double* data, int64_t P, int64_t T, int64_t ncuts, const int64_t* cut_len, double* dt_out, double* trend_out);

/* named scalars of the last operation: "refine_residual" (fp32 engine: max|y - K~ alpha~| / max|y| after the last refinement
 * step), "matrix_bytes" (device bytes held by this handle's matrix / factor buffers), "cov_slices" (the K slices the last sigp_predict_cov
 * ran its covariance product with: what "cov_slices" = 0 chose), "sparse_factor_a_ms" / "sparse_chunks_ms" / "sparse_factor_b_ms" (host clock of
 * the three phases of the last sigp_sparse_fit, each closed by a synchronisation: staging Z and factoring k(Z,Z) + eps I; the chunk loop;
 * assembling and factoring B), "dist_*" (see sigp_dist_fit). */
int sigp_get_stat(sigp_handle* h, const char* name, double* value);

/* K7 (explicit): alpha~ = K~^-1 y  [n]  (north/June1st.py:266; alpha of :271 is alpha~/sigma_f). */
int sigp_get_alpha(sigp_handle* h, double* alpha_tilde);
/* copy the lower triangle of K~ (before potrf) or L~ (after) to host, [n,n] row-major, upper = 0 */
int sigp_get_matrix(sigp_handle* h, int which, double* out, int64_t ldo);

/* K13/K14: MLII(theta) (north/June1st.py:235-257): theta = (log ell, log sn_tilde).
 * grad_mode 0 = none, 1 = reference formulae (:248-252), 2 = exact derivative of the profiled nlML.
 * Non-SPD -> returns SIGP_NOT_SPD and nlml = grad = +inf (the reference's except branch :254-256).
 * For the reference kernel the caller passes Sigma~ and dSigma = M @ Sigma~ (host, [N,N]). */
int sigp_nlml_grad(sigp_handle* h, int kernel_id, const double theta[2], const double* Sigma,
                   const double* MSigma, int64_t ldsigma, int grad_mode, double* nlml, double grad[2]);

/* MLII for a lockstep group of fits on the data sets resident after sigp_batch_upload (RBF / Matern, fp64): value and EXACT gradient
 * of the profiled nlML (north/June1st.py:235-257 with the true derivative = sigp_nlml_grad's grad_mode 2) for `count` (data set,
 * theta) pairs; fit i uses data set (first + i) % batch and theta[2i .. 2i+1] = (log ell, log sn~).  Groups of `group` members
 * (sigp_set_option) advance through every launch together: build, blocked Cholesky, L~^-T by recursive triangular inversion,
 * K~^-1 = U U^T, A~ = U z, reductions with dK~/dlog ell recomputed on the fly.  One call per optimiser iteration serves every
 * retrospective year (the call the reference left commented out, north/June1st.py:259-262, batched over the retro loop of
 * north/retrospective_forecasts/September1st_retro.py:176-248).  grad_mode 0 (value only; grad may be NULL) or 2.
 * Any feature count d >= 1 that sigp_batch_upload accepts is supported (the gradient's reduction holds the first 64 features of its rows in
 * LDS and reads the rest from global memory: no limit on d).
 * nlml [count], grad [count][2]; a non-SPD member gets +inf in both (the reference's except branch :254-256). */
int sigp_nlml_grad_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int grad_mode, double* nlml, double* grad);

/* Per-feature (ARD) length scales for the RBF / Matern-5/2 kernels: "which features matter, and how much".  With u_i = x_i / l
 * (element-wise, l in R^d) the ARD kernel is the isotropic one at ell = 1 on the scaled features: r^2_ij = sum_k (u_ik - u_jk)^2,
 * k = exp(-r^2/2) (RBF), k = (1 + s + s^2/3) e^-s with s = sqrt(5) r (Matern-5/2).  So the scales live in the STAGING and nothing else changes:
 * sigp_set_length_scales: ell [d] with finite ell[k] > 0 and d = the d of sigp_set_train (anything else: SIGP_BAD_ARG); ell = NULL returns the
 * handle to isotropic (the raw features again, bit for bit).  From then on the training features, the ride-along rows (those staged
 * already and those of later sigp_set_test calls) and the test points of sigp_predict / sigp_predict_cov are divided by ell[k] as they are
 * staged -- the IEEE division x / ell[k], not a product with a reciprocal: a caller who stages X / l and Xs / l with ell = 1 gets the
 * same bits from every call.  The ell argument of the build and fit calls stays a common multiplier (1 in ARD use).  The handle keeps
 * the raw features and ride rows beside the scaled ones (8 (n_pad + 128) dp bytes, allocated by the first call), so new scales need no new
 * sigp_set_train.  The call voids the fit, as sigp_set_test does; sigp_set_train clears the scales.  A handle that never sets scales
 * runs exactly the launches it ran before.
 * With scales set: SIGP_BAD_ARG for the reference kernel (SIGP_KERNEL_NETDIFFUSION in sigp_fit_predict, sigp_kernel_build_from_sigma)
 * and for sigp_dist_fit / sigp_dist_predict; on an fp32 handle the call itself is SIGP_BAD_ARG.  sigp_loo, sigp_cv, sigp_predict_cov and
 * sigp_get_alpha work on an ARD fit as on any other (they stage no features, or divide them as above).  The lockstep-batch entries
 * (sigp_batch_upload and everything on its resident data) stage their own data and neither read nor change these scales: sigp_batch_run,
 * sigp_nlml_grad_batch, sigp_loo_batch, sigp_loo_grad_batch and sigp_cv_batch are isotropic; per-feature scales PER FIT of a lockstep group
 * are sigp_batch_run_ard's and sigp_nlml_grad_ard_batch's (below). */
int sigp_set_length_scales(sigp_handle* h, const double* ell, int64_t d);
/* MLII with per-feature length scales: theta = (log l_1 .. log l_d, log sn~), ntheta = d + 1 (else SIGP_BAD_ARG) -> the profiled nlML
 * (north/June1st.py:235-257) and, with grad_mode 2, its exact gradient grad [d + 1] (grad_mode 0: value only, grad may be NULL).  A grid
 * over d + 1 parameters is out of reach; this is what an optimiser is given instead.  The call sets the scales to exp(theta[k]), fits with
 * ell = 1 through sigp_fit_predict's own launches (nlml carries that fit's bits) and, with P = K~^-1, a = P y, sf = y^T a / n, returns
 *     d nlML / d log l_k = sum_ij W_ij (u_ik - u_jk)^2,     W_ij = 1/2 (P_ij - a_i a_j / sf) h_ij,
 *     d nlML / d log sn~ = sn~ (tr P / 2 - a^T a / (2 sf))                                  (as sigp_nlml_grad)
 * with h_ij = k_ij (RBF), h_ij = (5/3)(1 + s_ij) e^-s_ij (Matern-5/2); the diagonal contributes 0, and at equal scales the d components
 * add up to sigp_nlml_grad's d nlML / d log ell.  ALL d components come from ONE pass over K~^-1 (4 n^2 bytes; d derivative matrices
 * through sigp_nlml_grad's reduction would move ~24 d n^2): one workgroup per 64 x 128 tile of its lower triangle forms the tile's
 * squared distances with the covariance build's own GEMM-form code, W in the accumulator layout they arrive in, and -- on the column-
 * centred scaled features -- the expanded square u_ik^2 rowsum(W)_i + [W (U_J o U_J)]_ik - 2 u_ik [W U_J]_ik with both products on
 * v_mfma_f64_16x16x4_f64; per-tile partial sums, added in a fixed order (no atomics: the same bits on every run).  Any d that
 * sigp_set_train accepts.  Cost on top of the fit: L~^-T and K~^-1 = U U^T as sigp_nlml_grad (2 n^3/3 flops), then the pass.
 * A non-SPD K~ or an exp(theta[k]) that overflows (or underflows to 0) gives +inf in nlml and every grad entry and returns SIGP_NOT_SPD, as
 * sigp_nlml_grad does.  fp64 engine, RBF / Matern-5/2 only; before sigp_set_train: SIGP_BAD_ARG.  Afterwards the handle is fitted at
 * those hyper-parameters with the scales set: sigp_predict, sigp_predict_ride, sigp_loo, sigp_cv, sigp_predict_cov work on it.  Device
 * work is accounted under SIGP_KC_MLII (the triangular inversion, U U^T, the pass: one entry each).
 * Lockstep groups of such fits: sigp_nlml_grad_ard_batch (the ARD gradients of the leave-one-out scores are sigp_loo_grad_ard's and, in
 * lockstep groups, sigp_loo_grad_ard_batch's; those of the leave-block-out scores sigp_cv_grad_ard's and sigp_cv_grad_ard_batch's).  Not covered: the one-workgroup kernel (sigp_small_*), the fp32 engine,
 * sharded fits. */
int sigp_nlml_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int grad_mode, double* nlml, double* grad);

/* Per-feature (ARD) length scales in lockstep groups on the data sets resident after sigp_batch_upload (RBF / Matern-5/2, fp64).  Scales
 * belong to a FIT, not to a data set: fit i uses data set (first + i) % batch with its own l_i in R^d, and two members of one group may share
 * a data set and differ in scales (several starts per data set: the ARD likelihood is multimodal).  Per group (sigp_set_option "group") ONE
 * staging launch fills, for every member, its scaled training features, scaled ride rows and its y -- u = x / l_k, the IEEE division, as
 * sigp_set_length_scales stages them (a caller who uploads X / l and Xs / l as data sets of their own and runs the isotropic entries at
 * ell = 1 gets the same bits) -- after ONE copy of the group's divisors; the staging area (8 group ((n_pad + 128) dp + n_pad) bytes) is
 * allocated before the call's first launch.  From there on the group runs the isotropic entries' own launches at ell = 1: build, blocked
 * Cholesky, epilogue.  The groups run one after another (no `concurrency`), as the score entries' do.
 * sigp_batch_run_ard: ell [count][ldell >= d], sn_tilde [count] -> out [count][4], mean / var [count][m] as sigp_batch_run gives them (the
 * ride points divided by the member's scales).  A non-finite or non-positive ell: SIGP_BAD_ARG.
 * sigp_nlml_grad_ard_batch: what sigp_nlml_grad_batch does, with theta_i = theta[i ldtheta .. + ntheta) = (log l_1 .. log l_d, log sn~),
 * ntheta = d + 1: nlml [count] and, with grad_mode 2, grad [count][ldgrad >= d + 1] (grad_mode 0: value only, grad may be NULL), the exact
 * gradient of sigp_nlml_grad_ard.  Per group: staging, fit, L~^-T, K~^-1 = U U^T and A~ = U z for every member at once, then
 * sigp_nlml_grad_ard's tile pass and its fixed-order sums with the member on a grid axis, one launch each (partials per member and tile,
 * no atomics: the same bits on every run; the tile pass executes a single fit's instructions, so a member carries the bits
 * sigp_nlml_grad_ard returns for that fit wherever the lockstep factorisation has the single fit's bits -- the small orders the tests pin;
 * at large orders the blocked Cholesky's schedule depends on the number of members, as for every batch entry).  A member whose
 * exp(theta) overflows, one of whose scales underflows to 0, or whose K~ is not SPD gets +inf in nlml and in all d + 1 gradient entries;
 * its group mates are unaffected and the call returns SIGP_OK, as sigp_nlml_grad_batch does.
 * SIGP_BAD_ARG: before sigp_batch_upload, an fp32 handle, the reference kernel, ntheta != d + 1, a leading dimension below its width.
 * Device work is accounted under SIGP_KC_MLII, the staging under SIGP_KC_KBUILD.  Both calls leave the handle unfitted, as the other batch
 * entries do, and neither read nor change the single-fit scales of sigp_set_length_scales.
 * The leave-one-out and leave-block-out scores and their ARD gradients for lockstep groups: sigp_loo_grad_ard_batch,
 * sigp_cv_grad_ard_batch.  Not covered: sigp_small_*, the fp32 engine, sharded fits. */
int sigp_batch_run_ard(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, int64_t ldell, const double* sn_tilde,
                       double* out, double* mean, double* var);
int sigp_nlml_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta,
                             int grad_mode, double* nlml, double* grad, int64_t ldgrad);

/* Leave-one-out cross-validation with the hyper-parameters held (Rasmussen & Williams 5.4.2): what the block north/June1st.py:264-277
 * returns for training point i when it is fitted on the other n - 1 points and asked to predict point i, for every i, from ONE
 * factorisation:  g_i = [K~^-1]_ii,  mean_i = y_i - A~_i / g_i,  var_i = s_i / g_i (includes the noise, like fvar
 * :273, :277) with s_i = (y^T A~ - A~_i^2 / g_i) / (n - 1) (SIGP_LOO_REFIT: sigma_f re-profiled without point i, :267-268 on n - 1 points)
 * or s_i = sigma_f (SIGP_LOO_FIXED: R&W eq. 5.12);  score [2] = nlpd = sum_i log(2 pi var_i)/2 + (y_i - mean_i)^2 / (2 var_i)  and
 * sse = sum_i (y_i - mean_i)^2, each added in a fixed order (the same bits on every run).  Cost on top of a fit: L~^-T (n^3/3 flops) and one
 * pass over its triangle (4 n^2 bytes); no K~^-1.  Device work is accounted under SIGP_KC_MLII (two entries per call or lockstep group:
 * the triangular inversion and the row pass).  n = 1 has no leave-one-out: SIGP_BAD_ARG.  fp64 engine only; after a sharded fit
 * (sigp_dist_fit) or on an fp32 handle: SIGP_BAD_ARG.
 * sigp_loo: after sigp_fit / sigp_fit_predict on this handle; mean [n], var [n], score [2].  The factor and the fit's state are only
 * read: sigp_predict / sigp_get_alpha afterwards return what they returned before. */
enum { SIGP_LOO_REFIT = 0, SIGP_LOO_FIXED = 1 };
int sigp_loo(sigp_handle* h, int sigma_mode, double* mean, double* var, double* score);
/* Lockstep groups (sigp_set_option "group") on the data sets resident after sigp_batch_upload, like sigp_nlml_grad_batch (RBF / Matern;
 * any other kernel_id: SIGP_BAD_ARG -- the reference kernel's batch is sigp_small_run_loo): fit i uses data set (first + i) % batch with
 * (ell[i], sn_tilde[i]); mean / var [count][nstride >= n] (both may be NULL: scores only), score [count][2].  A non-SPD member gets
 * +inf scores and NaN rows (north/June1st.py:254-256); the other members are not affected. */
int sigp_loo_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde,
                   int sigma_mode, double* mean, double* var, int64_t nstride, double* score);
/* The leave-one-out scores AND their exact derivatives with respect to (log ell, log sn~) (Rasmussen & Williams 5.4.2), so that an optimiser
 * can minimise them instead of searching a grid.  With P = K~^-1, a = P y, g_i = P_ii and D = dK~/dtheta:  t = D a, b = P t, e = a^T t,
 * c_i = [P D P]_ii;  dr_i = -b_i/g_i + a_i c_i/g_i^2;  ds_i = -e/n (FIXED) or (-e + 2 a_i b_i/g_i - a_i^2 c_i/g_i^2)/(n - 1) (REFIT);
 * dvar_i = ds_i/g_i + s_i c_i/g_i^2;  d nlpd = sum_i dvar_i/(2 var_i) + r_i dr_i/var_i - r_i^2 dvar_i/(2 var_i^2);  d sse = sum_i 2 r_i dr_i.
 * On top of sigp_loo's work (the same launches: mean, var and score carry the same bits): K~^-1 = U U^T (n^3/3), dK~/dlog ell from the
 * covariance build, and the one new cubic step c = diag(K~^-1 dK~ K~^-1) as a triangular 128-tile product of n^3 flops (half of the full
 * product); everything else is n^2 passes and fixed-order sums (no atomics: the same bits on every run).  log sn~ needs no cubic work.
 * Device work is accounted under SIGP_KC_MLII.  Memory: 8 n_pad^2 bytes each for the factor, L~^-T, K~^-1 and dK~ PER MEMBER (the lockstep
 * entry holds dK~ per member, which sigp_nlml_grad_batch avoids).
 * sigp_loo_grad: after sigp_fit / sigp_fit_predict; mean / var [n] may both be NULL; score [2] as sigp_loo;
 * grad [4] = d nlpd/d(log ell, log sn~), d sse/d(log ell, log sn~).  MSigma = M @ Sigma~ [N][ldsigma]: reference kernel only (required there,
 * and the fit must have come from sigp_fit_predict, which is told ell: d/dlog ell = ell d/dell), else NULL.  Errors as sigp_loo (fp32 handle,
 * sharded fit, n < 2, not fitted: SIGP_BAD_ARG).  The fit is only read: sigp_predict / sigp_get_alpha / sigp_loo afterwards return the bits
 * they returned before.
 * The one-workgroup kernel has its own: sigp_small_run_loo_grad.  Not covered: sharded fits, the fp32 engine.  With per-feature length scales
 * set (sigp_set_length_scales) the derivative is that of the common multiplier ell; the per-feature derivatives are sigp_loo_grad_ard's. */
int sigp_loo_grad(sigp_handle* h, int sigma_mode, const double* MSigma, int64_t ldsigma, double* mean, double* var, double* score, double* grad);
/* Lockstep groups on the resident batch data, arguments as sigp_loo_batch (RBF / Matern only); grad [count][4].  A non-SPD member gets +inf
 * scores and gradients and NaN rows; the other members are not affected. */
int sigp_loo_grad_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde,
                        int sigma_mode, double* mean, double* var, int64_t nstride, double* score, double* grad);
/* The leave-one-out scores and the exact derivatives of ONE of them with respect to per-feature length scales: theta = (log l_1 .. log l_d,
 * log sn~), ntheta = d + 1, as sigp_nlml_grad_ard; criterion names the score that grad [d + 1] differentiates.  The call sets the scales
 * to exp(theta[k]), fits with ell = 1 through sigp_fit_predict's own launches and runs sigp_loo's launches: score [2] and mean / var [n]
 * (both may be NULL, not one alone) carry the bits sigp_loo returns on that fit.  grad = NULL: scores only, no cubic work beyond sigp_loo's.
 * The chain rule of sigp_loo_grad is linear in the three quantities that depend on the direction D = dK~/dtheta (b = P D a, c = diag(P D P),
 * e = a^T D a), so it is transposed into one symmetric adjoint that does not:  d score = beta^T b + gamma^T c + eps e = sum_ij G_ij D_ij,
 *     G = 1/2 (v a^T + a v^T) + P diag(gamma) P + eps a a^T,   v = P beta,
 *     nlpd: beta_i = -rho_i/g_i [+ 2 kappa_i a_i/(g_i^2 (n - 1))],  gamma_i = kappa_i s_i/g_i^2 + rho_i a_i/g_i^2 [- kappa_i a_i^2/(g_i^3 (n - 1))],
 *           eps = -sum_i kappa_i/g_i / (n - 1) [REFIT; the bracketed terms too] or / n [FIXED],  kappa_i = 1/(2 var_i) - r_i^2/(2 var_i^2), rho_i = r_i/var_i;
 *     sse:  beta_i = -2 r_i/g_i,  gamma_i = 2 r_i a_i/g_i^2,  eps = 0;
 *     d score / d log l_k = sum_ij G_ij h_ij (u_ik - u_jk)^2  (h as sigp_nlml_grad_ard),     d score / d log sn~ = sn~ tr G.
 * Cost on top of sigp_loo: K~^-1 = U U^T (n^3/3), ONE cubic product M = (P Gamma) P^T on the lower 128-tiles (n^3 flops, the price of
 * sigp_loo_grad's one product -- d runs of that route would need d) and sigp_nlml_grad_ard's tile pass with 2 G o h as its weight, all d
 * components at once; everything else is n^2 passes and fixed-order sums (no atomics: the same bits on every run).  Memory: sigp_loo_grad's
 * single-fit buffers and the centred features of sigp_nlml_grad_ard.  Device work is accounted under SIGP_KC_MLII (sigp_loo's two entries,
 * then U U^T, the n^2 passes, the product, the tile pass: one entry each).
 * SIGP_BAD_ARG: the reference kernel, an fp32 handle, before sigp_set_train, n < 2, ntheta != d + 1, a bad sigma_mode or criterion.
 * SIGP_NOT_SPD: a non-SPD K~ or an exp(theta[k]) that is not finite and positive (sn~ = 0 is allowed): +inf in score and every grad entry,
 * NaN in mean / var.  Afterwards the handle is fitted at those hyper-parameters with the scales set, as after sigp_nlml_grad_ard.
 * Lockstep groups of such fits: sigp_loo_grad_ard_batch (below).  Not covered: sigp_small_*, the fp32 engine, sharded fits.  The
 * leave-block-out scores: sigp_cv_grad_ard. */
enum { SIGP_LOO_NLPD = 0, SIGP_LOO_SSE = 1 };
int sigp_loo_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int sigma_mode, int criterion,
                      double* mean, double* var, double* score, double* grad);
/* ... for lockstep groups on the data sets resident after sigp_batch_upload (RBF / Matern-5/2, fp64): what sigp_loo_grad_batch does, with
 * scales per FIT as in sigp_nlml_grad_ard_batch -- fit i uses data set (first + i) % batch and theta_i = theta[i ldtheta .. + ntheta) =
 * (log l_1 .. log l_d, log sn~), ntheta = d + 1; two members of one group may share a data set and differ in scales.  score [count][2] =
 * nlpd, sse; mean / var [count][nstride >= n] (both or neither); grad [count][ldgrad >= d + 1], the derivatives of the score `criterion`
 * names, or NULL: scores and predictions only, no cubic work beyond sigp_loo_batch's.  Groups of `group` members (sigp_set_option) run one
 * after another.  Per group: sigp_batch_run_ard's staging launch, the isotropic entries' fit at ell = 1 on the staged features and
 * sigp_loo_batch's launches on it -- the scores and predictions carry the bits sigp_loo_batch returns on data sets X / l uploaded as they
 * are, at ell = 1 --, then for every member at once K~^-1 = U U^T, a = U z, the coefficients beta, gamma, eps, v = P beta and P Gamma, ONE
 * cubic product M = (P Gamma) P^T per member (n^3 flops, whatever d) and sigp_loo_grad_ard's tile pass and fixed-order sums with the
 * member on a grid axis (no atomics: the same bits on every run, whatever the group size; a member executes a single fit's instructions
 * and carries the bits sigp_loo_grad_ard returns for it wherever the lockstep factorisation has the single fit's bits).  One copy brings a
 * group's gradients back.  A member whose exp(theta) overflows, one of whose scales underflows to 0, or whose K~ is not SPD gets +inf in
 * both scores and all d + 1 gradient entries and NaN rows in mean / var; its group mates are unaffected and the call returns SIGP_OK.
 * Memory beside the slot: three matrices of 8 group n_pad^2 bytes (L~^-T / M, K~^-1, P Gamma), as sigp_loo_grad_batch, and the staging area.
 * SIGP_BAD_ARG: before sigp_batch_upload, count < 1, an fp32 handle, the reference kernel, n < 2, ntheta != d + 1, a leading dimension
 * below its width, a bad sigma_mode or criterion, mean without var.  Device work is accounted under SIGP_KC_MLII, the staging under
 * SIGP_KC_KBUILD.  The handle is left unfitted, as after the other batch entries.
 * The leave-block-out scores in lockstep groups: sigp_cv_grad_ard_batch.  Not covered: sigp_small_*, the fp32 engine, sharded fits. */
int sigp_loo_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta,
                            int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad);
/* sigp_small_run with the leave-one-out cross-validation of every fit in the SAME single launch (L~^-1 formed in LDS over L~ as in
 * sigp_small_run_grad): out6 [nprob][6] = sigma_f, nlML, info, sigma_n, nlpd, sse; mean / var as in sigp_small_run;
 * loo_mean / loo_var [nprob][nstride >= largest n of the upload], entries beyond a set's n = NaN.  info > 0: nlpd = sse = +inf and NaN rows.
 * A fit that names a data set of one point: SIGP_BAD_ARG. */
int sigp_small_run_loo(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int sigma_mode,
                       double* out6, double* mean, double* var, int64_t mstride, double* loo_mean, double* loo_var, int64_t nstride);

/* Leave-block-out cross-validation with the hyper-parameters held: K-fold / h-block / hv-block folds of CONSECUTIVE rows (the rows are
 * consecutive years; leaving one year out keeps its serially correlated neighbours in the training set), from ONE factorisation.
 * block >= 1, gap >= 0: fold f SCORES the rows [c0, c1) = [f block, min(n, (f + 1) block)) and REMOVES the window
 * S_f = [max(0, c0 - gap), min(n, c1 + gap)) from training (the gap rows are removed but not scored); every row is scored by exactly one
 * fold, windows overlap when gap > 0, and their sizes differ at the two ends and in the last fold.  With P = K~^-1 and A~ = P y
 * (DESIGN.md section 2):  y_S - mean_S = P_SS^-1 A~_S,  Cov_S = s_S P_SS^-1 (includes the noise, like fvar),
 * s_S = (y^T A~ - A~_S^T P_SS^-1 A~_S) / (n - |S|) (SIGP_LOO_REFIT: sigma_f re-profiled without S -- what a real refit without the rows of S
 * returns) or y^T A~ / n (SIGP_LOO_FIXED).  mean [n], var [n] (var_i = s_S [P_SS^-1]_ii, the marginal variance; no joint block density is
 * defined), score [2] = nlpd, sse as sigp_loo's, added in a fixed order.  block = 1, gap = 0 is leave-one-out.  A shuffled K-fold is the
 * same call after the caller permutes the rows before the fit.
 * Limits: block + 2 gap <= SIGP_CV_MAX_WINDOW (one diagonal block; SIGP_CV_SMALL_MAX_WINDOW in sigp_small_run_cv), and every fold must leave
 * a training row (n - |S_f| >= 1): otherwise SIGP_BAD_ARG, as for an fp32 handle, a sharded fit, no fit, or n < 2.
 * Cost on top of sigp_loo's L~^-T: the strip products P_SS = U_S U_S^T of the rows U[S, min S .. n) (2 |S|^2 (n - min S) flops per fold on
 * the fp64 matrix pipe, split over "cv_slices" K slices and added in a fixed order: no atomics, the same bits on every run), a |S| x |S|
 * Cholesky per fold by the factorisation's own diagonal-block kernel, and two short solves.  Device work is accounted under SIGP_KC_MLII
 * (the triangular inversion, then four entries per pass of at most 1024 (member, fold) pairs).  Memory on top of sigp_loo: per pair of a
 * pass the partials (slices x (window rounded up to 16)^2 doubles) and 2 x 8 x 128^2 bytes.
 * sigp_cv: after sigp_fit / sigp_fit_predict, every kernel.  The fit is only read: sigp_predict / sigp_get_alpha / sigp_loo afterwards return
 * the bits they returned before.  A fold whose P_SS fails its pivot test leaves NaN in its rows and +inf in both scores. */
enum { SIGP_CV_MAX_WINDOW = 128, SIGP_CV_SMALL_MAX_WINDOW = 32 };
int sigp_cv(sigp_handle* h, int64_t block, int64_t gap, int sigma_mode, double* mean, double* var, double* score);
/* Lockstep groups on the resident batch data, argument conventions of sigp_loo_batch (RBF / Matern only; mean / var [count][nstride >= n]
 * may both be NULL; score [count][2]).  A member with a non-SPD K~, or one of whose P_SS fails its pivot test, gets +inf scores and NaN
 * rows; the other members are not affected. */
int sigp_cv_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde, int64_t block,
                  int64_t gap, int sigma_mode, double* mean, double* var, int64_t nstride, double* score);
/* sigp_small_run with the leave-block-out cross-validation of every fit in the SAME single launch (the reference kernel's batch; L~^-1 in
 * LDS as in sigp_small_run_loo, then per fold P_SS from its columns, a |S| x |S| Cholesky and the solves in LDS): out6 [nprob][6] =
 * sigma_f, nlML, info, sigma_n, nlpd, sse; cv_mean / cv_var [nprob][nstride >= largest n of the upload], NaN beyond a set's n.
 * block + 2 gap <= SIGP_CV_SMALL_MAX_WINDOW; every fold of every named data set must leave a training row.  info > 0 or a failed pivot of
 * a P_SS: nlpd = sse = +inf and NaN rows.
 * LDS: the folds need 17 152 bytes behind the plain image, so this launch picks its OWN feature chunk -- the largest of {the upload's, 16, 8}
 * that leaves them.  Largest order of the upload by its largest m: 128 (m <= 2), 127 (m = 3 .. 5), 126 (m = 6), 125 (m = 7, 8); beyond it
 * SIGP_BAD_ARG (the handle stays usable for the other launches).  Where that chunk is smaller than the upload's (largest order from 119 at
 * m = 0, 118 at m = 1, 2, 114 at m = 8) and a set has more features than it, K~ is summed in shorter pieces: sigma_f, nlML, sigma_n, mean
 * and var of this launch agree with sigp_small_run's to rounding, not bit for bit. */
int sigp_small_run_cv(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t block,
                      int64_t gap, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* cv_mean, double* cv_var,
                      int64_t nstride);
/* The leave-block-out scores and the exact derivatives of ONE of them with respect to per-feature length scales: theta, ntheta = d + 1,
 * criterion (SIGP_LOO_NLPD / SIGP_LOO_SSE) and mean / var [n] (both or neither) as sigp_loo_grad_ard; block, gap and the fold limits as
 * sigp_cv.  The call sets the scales to exp(theta[k]), fits with ell = 1 through sigp_fit_predict's own launches and runs sigp_cv's
 * launches: score [2], mean and var carry the bits sigp_cv returns on that fit (at the same "cv_slices").  grad = NULL: scores only.
 * The adjoint of sigp_loo_grad_ard with a block in place of the diagonal.  Per fold f with window S (w rows), scored
 * rows C, H = P_SS^-1, r = H A~_S, s as sigp_cv, var_i = s H_ii:  rbar_i = r_i/var_i, kappa_i = 1/(2 var_i) - r_i^2/(2 var_i^2) (nlpd) or
 * rbar_i = 2 r_i, kappa_i = 0 (sse) on C and zero outside;  t = H rbar,  sbar = sum_C kappa_i H_ii;
 *     beta_f = -t [+ 2 sbar r/(n - w)],  B_f = 1/2 (t r^T + r t^T) + s H diag(kappa) H [- sbar r r^T/(n - w)],  eps += -sbar/(n - w) [REFIT; the
 *     bracketed terms too] or -sbar/n [FIXED];   beta = sum_f E_f beta_f,  B = sum_f E_f B_f E_f^T (symmetric, |i - j| < 128),
 *     d score = sum_ij G_ij D_ij,   G = 1/2 (v a^T + a v^T) + P B P + eps a a^T,   v = P beta,
 *     d score / d log l_k = sum_ij G_ij h_ij (u_ik - u_jk)^2,     d score / d log sn~ = sn~ tr G.
 * block = 1, gap = 0 is sigp_loo_grad_ard's adjoint.  Cost on top of sigp_cv: per fold two products of the window's size on the fp64 matrix
 * pipe; K~^-1 = U U^T (n^3/3); P B over B's band (6 x 128 n_pad^2 flops); ONE cubic product M = (P B) P^T on the lower 128-tiles (n^3 flops for
 * any d and any fold layout) and sigp_nlml_grad_ard's tile pass.  Every sum has a fixed order (no atomics: the same bits on every run).
 * Memory: sigp_loo_grad's single-fit buffers, sigp_cv's workspaces, the centred features, B in a band store (8 x 384 n_pad bytes) and
 * B_f / beta_f of one pass of at most 1024 folds (8 (window rounded up to 16)^2 bytes per fold).  Device work is accounted under SIGP_KC_MLII
 * (sigp_cv's entries and two more per pass -- the fold adjoints, their assembly -- then U U^T, the n^2 passes, the banded product, the
 * product M, the tile pass: one entry each).
 * SIGP_BAD_ARG: as sigp_loo_grad_ard, and sigp_cv's fold checks (block + 2 gap <= SIGP_CV_MAX_WINDOW, every fold leaves a training row).
 * SIGP_NOT_SPD: a non-SPD K~, an exp(theta[k]) that is not finite and positive, or a fold whose P_SS fails its pivot test: +inf in score and
 * every grad entry, NaN in mean / var.  Afterwards the handle is fitted at those hyper-parameters with the scales set, as after
 * sigp_loo_grad_ard.
 * Lockstep groups of such fits: sigp_cv_grad_ard_batch (below).  Not covered: sigp_small_*, the reference kernel, the fp32 engine, sharded
 * fits. */
int sigp_cv_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int64_t block, int64_t gap, int sigma_mode,
                     int criterion, double* mean, double* var, double* score, double* grad);
/* ... for lockstep groups on the data sets resident after sigp_batch_upload (RBF / Matern-5/2, fp64): what sigp_cv_batch does, with scales
 * per FIT and every other convention as in sigp_loo_grad_ard_batch -- fit i uses data set (first + i) % batch and theta_i =
 * theta[i ldtheta .. + ntheta) = (log l_1 .. log l_d, log sn~), ntheta = d + 1; two members of one group may share a data set and differ in
 * scales.  block, gap and the fold limits as sigp_cv, on the batch's n.  score [count][2] = nlpd, sse; mean / var [count][nstride >= n]
 * (both or neither); grad [count][ldgrad >= d + 1], the derivatives of the score `criterion` names, or NULL: scores and predictions only,
 * no cubic work beyond sigp_cv_batch's.  Groups of `group` members (sigp_set_option) run one after another.  Per group:
 * sigp_batch_run_ard's staging launch, the isotropic entries' fit at ell = 1 on the staged features and sigp_cv_batch's launches on it --
 * the scores and predictions carry the bits sigp_cv_batch returns on data sets X / l uploaded as they are, at ell = 1 --, with, per pass of
 * 1024 / members folds of every member, the fold adjoints beta_f, B_f, eps_f of all (member, fold) pairs in one launch and their assembly
 * into every member's beta and band store in another; then for every member at once K~^-1 = U U^T, a = U z, eps, v = P beta, P B over
 * B's band, ONE cubic product M = (P B) P^T per member (n^3 flops, whatever d and the folds) and sigp_loo_grad_ard's tile pass and
 * fixed-order sums with the member on a grid axis.  Every entry of beta and B adds its folds' terms in ascending fold order in one chain
 * from zero, however the folds are split into passes (no atomics): the same bits on every run, whatever the group size, and a member
 * executes a single fit's instructions and carries the bits sigp_cv_grad_ard returns for it wherever the lockstep factorisation has the
 * single fit's bits.  One copy brings a group's gradients back.  A member whose exp(theta) overflows, one of whose scales underflows to 0,
 * whose K~ is not SPD or one of whose folds' P_SS fails its pivot test gets +inf in both scores and all d + 1 gradient entries and NaN rows
 * in mean / var; its group mates are unaffected and the call returns SIGP_OK.
 * Memory beside the slot: three matrices of 8 group n_pad^2 bytes (L~^-T / M, K~^-1, P B), the staging area, sigp_cv_batch's work buffers,
 * per member a band store (8 x 384 n_pad bytes) and eps_f, and B_f / beta_f of one pass of at most 1024 (member, fold) pairs.
 * SIGP_BAD_ARG: everything sigp_loo_grad_ard_batch refuses, and sigp_cv's fold checks (block + 2 gap <= SIGP_CV_MAX_WINDOW, every fold
 * leaves a training row).  Device work is accounted under SIGP_KC_MLII (sigp_cv_grad_ard's entries, their figures times the members), the
 * staging under SIGP_KC_KBUILD.  The handle is left unfitted, as after the other batch entries.
 * Not covered: sigp_small_*, the reference kernel, the fp32 engine, sharded fits. */
int sigp_cv_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta,
                           int64_t block, int64_t gap, int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score,
                           double* grad, int64_t ldgrad);

/* Expanding-window (rolling-origin) hindcast validation: the score the reference's retrospective loop reports -- train on the years before
 * t, forecast year t, for every t (September1st_retro.py:176-248) -- with the hyper-parameters (and, for the reference kernel, M and the
 * feature columns) held, from ONE fit.  Rows are in time order, 0-based.  Row t is scored when s = t - lead + 1 >= min_train; its training
 * set is rows [0, s): lead = 1 is one step ahead, and lead - 1 rows between the training set and the target are withheld.  The Cholesky
 * factor of the first s rows is the leading block of L~ and the first s entries of z = L~^-1 y are that prefix's solved vector, so
 *     y_t - mean_t = sum_{j=s..t} L~_tj z_j,    var_t = sigma_t sum_{j=s..t} L~_tj^2    (with the noise, like fvar),
 *     sigma_t = (sum_{j<s} z_j^2) / s  (SIGP_LOO_REFIT: sigma_f profiled on the training rows alone, what a fit on rows [0, s) returns)
 *            or q / n                  (SIGP_LOO_FIXED: the full fit's sigma_f, its own bits),
 *     score[0] = sum_t log(2 pi var_t)/2 + (y_t - mean_t)^2 / (2 var_t),   score[1] = sum_t (y_t - mean_t)^2   over the scored rows,
 * added in a fixed order (no atomics: the same bits on every run).  Rows that are not scored get NaN in mean / var.  No L~^-T is formed:
 * one scan of z^2 and one pass over n segments of at most lead entries.
 * sigp_hindcast: after sigp_fit / sigp_fit_predict, any kernel; mean [n], var [n], score [2].  The factor, z and q are only read:
 * sigp_predict / sigp_get_alpha / sigp_loo / sigp_cv afterwards return the bits they returned before.  SIGP_BAD_ARG: an fp32 handle, a
 * sharded fit, not fitted, lead < 1, lead > SIGP_HINDCAST_MAX_LEAD, min_train < 1, no scored row (min_train + lead - 1 > n - 1), a bad
 * sigma_mode.  Device work is accounted under SIGP_KC_MLII (the scan and the row pass: one entry each).
 * Gradients for lockstep groups: sigp_hindcast_grad_ard_batch (below); the reference kernel's, in the one-workgroup kernel:
 * sigp_small_run_hindcast_grad.  Out of scope: the fp32 engine, sharded fits. */
enum { SIGP_HINDCAST_MAX_LEAD = 128, SIGP_HINDCAST_SMALL_MAX_LEAD = 32 };
int sigp_hindcast(sigp_handle* h, int64_t lead, int64_t min_train, int sigma_mode, double* mean, double* var, double* score);
/* ... for lockstep groups on the data sets resident after sigp_batch_upload (RBF / Matern-5/2; the retro loop's refits per grid point,
 * September1st_retro.py:176-248, for many grid points at once): arguments and errors as sigp_loo_batch, and sigp_hindcast's checks on
 * lead, min_train and sigma_mode.  A non-SPD member gets +inf scores and NaN rows; its group mates keep their bits.  The handle is left
 * unfitted, as after the other batch entries. */
int sigp_hindcast_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde, int64_t lead,
                        int64_t min_train, int sigma_mode, double* mean, double* var, int64_t nstride, double* score);
/* One more flavour of the one-workgroup kernel (sigp_small_upload / sigp_small_run: the reference's own kernel at the reference's own size,
 * one workgroup per fit): the retro loop's rolling-origin refits (September1st_retro.py:176-248) for every queued (data set, l, sn~) in the
 * same single launch as the fits.  Arguments, outputs and conventions as sigp_small_run_loo: out6 [nprob][6] = sigma_f, nlML, info, sigma_n,
 * hindcast nlpd, hindcast sse; hc_mean / hc_var [nprob][nstride >= the largest n] (NaN where a row is not scored and beyond a set's n).
 * L~ and z are read where the factorisation left them in LDS; no inverse is formed.  A non-SPD K~ gives +inf in both scores.
 * SIGP_BAD_ARG: what sigp_small_run_loo refuses, lead < 1, lead > SIGP_HINDCAST_SMALL_MAX_LEAD, min_train < 1, a bad sigma_mode, and a named
 * data set without a scored row (min_train + lead - 1 > n - 1).  The other four instantiations of the kernel keep their instructions. */
int sigp_small_run_hindcast(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t lead,
                            int64_t min_train, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* hc_mean,
                            double* hc_var, int64_t nstride);
/* Gradients of the leave-one-out and hindcast scores in the one-workgroup kernel (the reference's own kernel): sigp_small_run_loo /
 * sigp_small_run_hindcast with `criterion` (SIGP_LOO_NLPD / SIGP_LOO_SSE) added, in the same single launch, one workgroup per fit.
 * out8 [nprob][8] = the six outputs of the score entry, then d S / d log l and d S / d log sn~ of the score S the criterion names, with
 * (l, sn~) held and sigma_f re-profiled as sigma_mode says.  out8[0..5], mean / var and the row predictions carry the bytes the score entry
 * returns for the same arguments.  A score is a function of K~ = A diag(w) A^T + sn~ I and y alone; with its symmetric adjoint G = dS/dK~
 * (sigp_loo_grad_ard's for leave-one-out, sigp_hindcast_grad_ard's for the hindcast)
 *     dS/dlog l = l <G, A diag(dw) A^T>,  dw_k = lam_k exp(l lam_k)  (lam_mode 1 sets: sigp_small_set_dweights' pool; without it NaN),     dS/dlog sn~ = sn~ tr G.
 * G is never stored: with X = L~^-1 formed in LDS over L~, G = X^T C X and both contractions are sums of b^T C b over b = X a_c and over the
 * columns of X; the hindcast flavour saves the band L~(t, s_t..t) before the inverse overwrites it.  No atomics, every sum in a fixed order:
 * the same bits on every run, whatever a fit's place in the queue.  A non-SPD K~: +inf in out8[4..7], rows as the caller left them.
 * Limits (SmallLayout, smallgp_layout.hpp): every n <= 96 with every m <= 8 and every lead <= SIGP_HINDCAST_SMALL_MAX_LEAD; beyond that what
 * fits in LDS at feature chunk 8 -- leave-one-out: n <= 128 up to m = 6, n <= 127 at m = 7, 8; hindcast at lead = 1: n <= 128 up to m = 5,
 * n <= 127 above, and at n = 128, m = 0 up to lead = 6 -- for the LARGEST n and m uploaded.  SIGP_BAD_ARG: what the score entry refuses, a
 * bad criterion, and a launch beyond these limits.  To fit, the launch may build K~ from shorter feature chunks than the score entry does
 * (as sigp_small_run_cv); the bytes then agree where no set has more features than the chunk.  The leave-block-out scores: sigp_small_run_cv_grad (below). */
int sigp_small_run_loo_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int sigma_mode,
                            int criterion, double* out8, double* mean, double* var, int64_t mstride, double* loo_mean, double* loo_var,
                            int64_t nstride);
int sigp_small_run_hindcast_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t lead,
                                 int64_t min_train, int sigma_mode, int criterion, double* out8, double* mean, double* var, int64_t mstride,
                                 double* hc_mean, double* hc_var, int64_t nstride);
/* Gradients of the leave-block-out scores in the one-workgroup kernel: sigp_small_run_cv with `criterion` (SIGP_LOO_NLPD / SIGP_LOO_SSE) added, in
 * the same single launch, one workgroup per fit.  out8 [nprob][8] = the six outputs of sigp_small_run_cv, then d S / d log l and d S / d log sn~
 * of the score the criterion names, (l, sn~) held and sigma_f re-profiled per fold as sigma_mode says; out8[0..5], mean / var and cv_mean /
 * cv_var carry the bytes sigp_small_run_cv returns for the same arguments.  The adjoint is sigp_cv_grad_ard's (G = 1/2 (v a^T + a v^T) + P B P +
 * eps a a^T), contracted as sigp_small_run_loo_grad contracts its own: with X = L~^-1, G = X^T C X, C = 1/2 (u z^T + z u^T) + X B X^T + eps z z^T,
 * u = X beta, and b^T C b = (b.u)(b.z) + p^T B p + eps (b.z)^2 with p = X^T b, summed over b = X a_c (weights l dw_c) and over the columns of X
 * (weight sn~).  Per fold H = P_SS^-1, t = H rbar, beta_f, B_f and eps_f are formed in LDS behind the fold's scores; B, symmetric with
 * |i - j| < block + 2 gap, is kept as its lower band [n][block + 2 gap].  Folds run one after the other and every entry is added by one thread:
 * overlapping windows add in ascending fold order, no atomics, the same bits on every run and whatever a fit's place in the queue.
 * lam_mode 1 sets without sigp_small_set_dweights: NaN in d S / d log l alone.  A non-SPD K~ or a failed pivot of a fold's P_SS: +inf in
 * out8[4..7] (the latter with NaN rows, as sigp_small_run_cv).
 * Limits (SmallLayout, smallgp_layout.hpp) for the LARGEST n and m uploaded: every n <= 96 with every m <= 8 at every window block + 2 gap <=
 * SIGP_CV_SMALL_MAX_WINDOW; beyond that what fits in LDS at feature chunk 8 -- at m = 0 n <= 123 / 121 / 119 / 116 / 109 for windows
 * 1 / 5 / 8 / 16 / 32, at m = 8 n <= 119 / 117 / 115 / 113 / 106.  SIGP_BAD_ARG: what sigp_small_run_cv refuses, a bad criterion, and a launch
 * beyond these limits (the message names n, m, the window and the bytes).  To fit, the launch may build K~ from shorter feature chunks than
 * sigp_small_run_cv does; the bytes then agree where both use the same chunk or no set has more features than this launch's chunk.  The seven
 * other instantiations of the kernel keep their instructions. */
int sigp_small_run_cv_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t block,
                           int64_t gap, int sigma_mode, int criterion, double* out8, double* mean, double* var, int64_t mstride, double* cv_mean,
                           double* cv_var, int64_t nstride);
/* The one-workgroup kernel with an RBF / Matern-5/2 covariance, one length scale per fit or one per feature (ARD): sigp_small_run with
 * K~ = k(X, X) + sn~ I in place of X Sigma~ X^T, one workgroup per fit, one launch for the list, n <= 128.  The data sets come from
 * sigp_small_upload as before with A = [X ; Xs], the RAW rows, lam_mode 0 and any lam (it is not read).  kernel_id: SIGP_KERNEL_RBF or
 * SIGP_KERNEL_MATERN52, one per call.  ell [nprob][ldell]: ard = 0, fit p has the scale ell[p ldell] for every feature; ard = 1, fit p has
 * ell[p ldell + k] for feature k < N of its set (ldell >= the largest N named).  The workgroup stages u = x / l_k (the IEEE division, as
 * sigp_set_length_scales does), sums the squared distances by direct differences in ascending k (exact zeros on the diagonal and for duplicate
 * rows; the same bits whatever the feature chunk) and maps them through the library's covariance functions at unit length scale; k** = 1.
 * out4, mean, var and mstride as sigp_small_run; a non-SPD K~ as there (+inf, info = the pivot, NaN predictions).
 * SIGP_BAD_ARG, the message naming the offender: a kernel id other than the two, ard not 0 / 1, a scale that is not finite and > 0 or whose
 * reciprocal is not finite, ldell too small, and everything sigp_small_run refuses. */
int sigp_small_run_k(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard,
                     const double* sn_tilde, double* out4, double* mean, double* var, int64_t mstride);
/* sigp_small_run_k, then value + EXACT gradient of the profiled nlML in every length scale and sn~ in the same single launch; out4, mean and
 * var carry the bytes sigp_small_run_k returns.  grad [nprob][ldg]: ard = 0 (d/d log l, d/d log sn~), ldg >= 2; ard = 1
 * d/d log l_0 .. d/d log l_{N-1}, d/d log sn~, ldg >= N + 1 of every set named, NaN behind a fit's N + 1 entries.  With W = K~^-1 - a~ a~^T /
 * sigma_f and h as in sigp_nlml_grad_ard:  d/d log l_k = sum_{i>j} W_ij h_ij (u_ik - u_jk)^2,  d/d log sn~ = sn~ (tr K~^-1 - a~.a~ / sigma_f) / 2;
 * one common scale: the sum over k in ascending k.  In LDS: X = L~^-1 over L~, the squared distances again into the strict upper triangle of the
 * bordered matrix, each replaced by W_ij h_ij (n^3/3 multiply-adds, no second n x n buffer), then one pass per feature over the pairs; fixed
 * summation order, no atomics: the same bits on every run.  A non-SPD K~: +inf in every gradient entry of the fit.  LDS: the image of
 * sigp_small_run_grad.  SIGP_BAD_ARG: as sigp_small_run_k, grad = NULL and ldg too small. */
int sigp_small_run_k_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard,
                          const double* sn_tilde, double* out4, double* mean, double* var, int64_t mstride, double* grad, int64_t ldg);
/* sigp_small_run_loo with that covariance: the leave-one-out tail reads K~, L~^-1, z and y alone and runs its own statements.  Arguments behind
 * sn_tilde, outputs, limits and refusals as sigp_small_run_loo; out6[0..3], mean and var carry sigp_small_run_k's bytes. */
int sigp_small_run_k_loo(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard,
                         const double* sn_tilde, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* loo_mean,
                         double* loo_var, int64_t nstride);
/* sigp_small_run_cv with that covariance: folds, windows, LDS limits and refusals as there (the layouts are the same).  The launch may pick a
 * shorter feature chunk than sigp_small_run_k; the squared distances are one running sum in ascending k per entry, so out6[0..3], mean and var
 * still carry sigp_small_run_k's bytes. */
int sigp_small_run_k_cv(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard,
                        const double* sn_tilde, int64_t block, int64_t gap, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride,
                        double* cv_mean, double* cv_var, int64_t nstride);
/* sigp_small_run_hindcast with that covariance: rows, lead, min_train, limits and refusals as there; L~ and z are read where the factorisation
 * left them.  The score gradients (sigp_small_run_*_grad) are not built for the stationary covariances. */
int sigp_small_run_k_hindcast(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard,
                              const double* sn_tilde, int64_t lead, int64_t min_train, int sigma_mode, double* out6, double* mean, double* var,
                              int64_t mstride, double* hc_mean, double* hc_var, int64_t nstride);
/* The hindcast scores AND the exact derivatives of one of them with respect to theta = (log l_1 .. log l_d, log sn~) (RBF / Matern-5/2,
 * fp64), so that the length scales can be chosen by the score the retro loop reports (September1st_retro.py:176-248) instead of a grid.
 * theta, ntheta = d + 1, criterion (SIGP_LOO_NLPD / SIGP_LOO_SSE) and mean / var [n] (both or neither) as sigp_loo_grad_ard.  Sets the
 * scales, fits with ell = 1 through sigp_fit_predict's own launches and runs sigp_hindcast's launches: score [2] and mean / var carry the
 * bits sigp_hindcast returns on that fit.  grad = NULL: scores only, no L~^-T and no cubic work.
 * The gradient is one symmetric adjoint G = d score / d K~, the reverse-mode derivative of the Cholesky factorisation: with
 * kappa_t = 1/(2 var_t) - r_t^2/(2 var_t^2), rho_t = r_t/var_t (nlpd) or kappa_t = 0, rho_t = 2 r_t (sse), r_t = y_t - mean_t,
 *     B_tj = rho_t z_j + 2 kappa_t sigma_t L~_tj  (s_t <= j <= t),   zbar_j = sum_{t: s_t <= j <= t} rho_t L~_tj + 2 z_j sum_{t: s_t > j} kappa_t w_t / s_t
 *     (FIXED: 2 z_j (sum_t kappa_t w_t) / n),   A = L~^T B - zbar z^T on its lower triangle,   C_ij = C_ji = A_ij / 2 (i >= j),   G = U C U^T, U = L~^-T,
 *     grad[k] = sum_ij G_ij h_ij (u_ik - u_jk)^2 (h as in sigp_nlml_grad_ard),   grad[d] = sn~ tr G.
 * Cost on top of the values: U = L~^-T (n^3/3) and G = U W^T on the lower 128-tiles (n^3/3) are the cubic steps -- 2 n^3 / 3 against the
 * 5 n^3 / 3 of sigp_loo_grad_ard; W = U C needs no cubic product (the banded part of C is a banded product of 2 n^2 lead flops, its
 * rank-one part two fixed-order scans along each row of U); then sigp_loo_grad_ard's tile pass with G as its matrix, all d components at
 * once.  Memory: sigp_loo_grad's single-fit buffers and the centred features.  SIGP_KC_MLII, one entry per step.
 * SIGP_BAD_ARG: as sigp_loo_grad_ard, and sigp_hindcast's checks.  SIGP_NOT_SPD (K~ not SPD or exp(theta) overflowed): score and grad
 * +inf, mean / var NaN.  Afterwards the handle is fitted at exp(theta) with the scales set, as after sigp_loo_grad_ard. */
int sigp_hindcast_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int64_t lead, int64_t min_train, int sigma_mode,
                           int criterion, double* mean, double* var, double* score, double* grad);
/* ... for lockstep groups on the data sets resident after sigp_batch_upload (RBF / Matern-5/2, fp64): what sigp_hindcast_batch does, with
 * scales per FIT and every other convention as in sigp_cv_grad_ard_batch, lead / min_train in place of block / gap -- fit i uses data set
 * (first + i) % batch and theta_i = theta[i ldtheta .. + ntheta) = (log l_1 .. log l_d, log sn~), ntheta = d + 1; two members of one group
 * may share a data set and differ in scales.  score [count][2] = nlpd, sse; mean / var [count][nstride >= n] (both or neither; NaN where a
 * row is not scored); grad [count][ldgrad >= d + 1], the derivatives of the score `criterion` names, or NULL: scores and predictions only,
 * no L~^-T and no cubic work.  Groups of `group` members (sigp_set_option) run one after another.  Per group: sigp_batch_run_ard's staging
 * launch, the isotropic entries' fit at ell = 1 on the staged features and sigp_hindcast_batch's launches on it -- the scores and
 * predictions carry the bits sigp_hindcast_batch returns on data sets X / l uploaded as they are, at ell = 1 --, then for every member at
 * once sigp_hindcast_grad_ard's steps with the member on a grid axis: the coefficients, zbar, the banded part of C, U = L~^-T, W = U C,
 * ONE cubic product G = U W^T per member and sigp_loo_grad_ard's tile pass and fixed-order sums.  W = U C runs on a kernel of its own here
 * (hindcast_w_lds_kernel): it keeps the row piece of U and the row of W in LDS (16.5 n_pad bytes) and touches global memory only in runs
 * of 256 consecutive doubles, where the single fit's kernel reads and writes at a stride of up to 32 doubles; both form every entry by the
 * same chain of operations, so W has the same bits.  It serves n_pad <= 8192 (132 KB of the 160 KB of LDS a workgroup may have); larger
 * groups take the single fit's kernel.  No atomics:
 * the same bits on every run, whatever the group size, and a member executes a single fit's floating-point operations and carries the bits
 * sigp_hindcast_grad_ard returns for it wherever the lockstep factorisation has the single fit's bits.  One copy brings a group's gradients
 * back.  A member whose exp(theta) overflows, one of whose scales underflows to 0 or whose K~ is not SPD gets +inf in both scores and all
 * d + 1 gradient entries and NaN rows in mean / var; its group mates are unaffected and the call returns SIGP_OK.
 * Memory beside the slot: the staging area and the vectors; a gradient adds three matrices of 8 group n_pad^2 bytes (L~^-T, W, Cb / G).
 * SIGP_BAD_ARG: everything sigp_loo_grad_ard_batch refuses, and sigp_hindcast's checks on the batch's n (lead <= SIGP_HINDCAST_MAX_LEAD).
 * Device work is accounted under SIGP_KC_MLII (sigp_hindcast_grad_ard's entries, their figures times the members), the staging under
 * SIGP_KC_KBUILD.  The handle is left unfitted, as after the other batch entries.
 * Not covered: sigp_small_*, the reference kernel's gradient, the fp32 engine, sharded fits. */
int sigp_hindcast_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta,
                                 int64_t lead, int64_t min_train, int sigma_mode, int criterion, double* mean, double* var, int64_t nstride,
                                 double* score, double* grad, int64_t ldgrad);

/* One large fit sharded over the GPUs of a node (BASELINE configs[3] fp64, configs[4] fp32 + fp64 refinement): 1-D block-cyclic
 * ownership of outer panels (W column blocks of 128; panel q belongs to rank q % nranks), OWNER-ONLY storage -- a rank allocates,
 * builds and updates only the block columns of its own panels (per-rank matrix bytes ~ 1/nranks) -- and the block-row panel
 * broadcast inside the library: per panel the owner factors it on its panel stream, packs [rows below its top block, ride rows
 * included] x [its columns] (what the later panels read; the last panel does not travel) in SEGMENTS of `dist_segment` column blocks:
 * a segment is broadcast on a communication stream (RCCL over xGMI) as soon as its last column is solved, while the owner's chain
 * goes on with the next columns and every rank is still applying the previous panel (look-ahead); the next panel's owner applies
 * each segment to its columns as it arrives, every other rank assembles the segments and updates its later panels in one launch.
 * Streams are ordered with events only: no host synchronisation and no device-to-host read per panel; the pivot info is MIN-reduced once at the end together with the 512 partial ride-row reductions (the only other fp64 exchange).
 * Replaces north/June1st.py:265 (np.linalg.cholesky) and :266-277, :246 for one large K~, as sigp_fit_predict does on one GPU.
 * fp32 handles (SIGP_F32): the fp32 factor is sharded the same way; x = K~^-1 [y k*] then comes from triangular solves on the
 * DISTRIBUTED factor (per panel: one skinny product with the explicit inverse of the owner's diagonal block + one skinny update
 * of the owner's column panel, and one 16 KB collective) and the fp64 residual of the iterative refinement is sharded by rows
 * (each rank recomputes the covariance of its rows only; one all-reduce assembles it).
 *
 *   sigp_dist_unique_id(id)            rank 0: a fresh 128-byte ncclUniqueId, to be handed to the other ranks by any channel
 *   sigp_dist_init(h, nranks, rank, id)  open THIS handle's communicator on its device (collective: every rank calls it).
 *                                      librccl is bound at run time (dlopen): a process that already has an RCCL mapped -- PyTorch-ROCm
 *                                      ships its own -- gets that one; nranks == 1 needs no RCCL at all (id NULL; with an id a one-rank
 *                                      communicator is opened and every collective of the fit still goes through it)
 *   sigp_dist_init_transport(...)      instead of the library's communicator, the caller's: callbacks that move a buffer.  device_buffers
 *                                      = 1: they receive DEVICE pointers and the hipStream_t to enqueue on (a communicator the caller
 *                                      already owns); 0: HOST pointers (the library stages through pinned memory and synchronises per
 *                                      collective -- rehearsal on a box with fewer GPUs than ranks, fabrics without device collectives).
 *                                      Same panel loop, same arithmetic, same order.
 *   sigp_dist_fit(...)                 after sigp_set_train / sigp_set_test with the SAME data on every rank (n d 8 bytes): the whole
 *                                      sharded fit; out / mean / var as sigp_fit_predict, identical on every rank.  Sigma as there
 *                                      (reference kernel: fp64 only).  SIGP_NOT_SPD + LAPACK pivot in out[2] on every rank otherwise.
 *                                      The factor stays spread over the ranks; other test points: sigp_dist_predict.
 *   set_option("owner_only", 1) before sigp_set_train keeps an fp64 handle from allocating the n x n single-GPU matrix;
 *   set_option("dist_stats", 1) times the broadcasts with HIP events: sigp_get_stat "dist_fit_ms", "dist_factor_ms" (device time of the
 *   panel loop), "dist_bcast_bytes", "dist_comm_ms" (per panel: first segment ready -> last segment arrived, summed), "dist_stall_ms" (time
 *   the update stream sat idle waiting for a panel: what look-ahead did NOT hide), "dist_solve_ms", "dist_collectives", "dist_comm_ranks"
 *   (what the communicator itself reports: ncclCommCount), "dist_host_comm_ms", "dist_enqueue_ms" (host time inside the collectives'
 *   enqueue calls / for the whole panel loop). */
typedef struct sigp_transport {
  void* ctx;
  int device_buffers;
  /* broadcast `bytes` from rank `root` in place; stream: hipStream_t to order on (device_buffers) or NULL (host pointers: blocking) */
  int (*bcast)(void* ctx, void* buf, uint64_t bytes, int root, void* stream);
  /* all-reduce `count` elements in place; is_f32: float, else double; op 0 = sum, 1 = min.  Non-zero return = failure. */
  int (*allreduce)(void* ctx, void* buf, uint64_t count, int is_f32, int op, void* stream);
  /* Only for set_option("dist_panel_split", 1) (may be NULL otherwise), both in place on a buffer of nranks chunks of `chunk_bytes`:
   * scatter: the root's chunk r goes to rank r at buf + r chunk_bytes (the root keeps its own);
   * allgather: rank r contributes the chunk at buf + r chunk_bytes, every rank ends with all of them. */
  int (*scatter)(void* ctx, void* buf, uint64_t chunk_bytes, int root, void* stream);
  int (*allgather)(void* ctx, void* buf, uint64_t chunk_bytes, void* stream);
} sigp_transport;
int sigp_dist_unique_id(void* id128);
int sigp_dist_init(sigp_handle* h, int nranks, int rank, const void* nccl_id);
int sigp_dist_init_transport(sigp_handle* h, int nranks, int rank, const sigp_transport* transport);
/* The same for a caller compiled against ANOTHER version of this header: struct_bytes = sizeof(sigp_transport) as the caller knows it; members
 * beyond it read as NULL (the struct grew from four to six members in 4.0: a 3.x caller passes its shorter struct here, or sets scatter /
 * allgather to NULL).  sigp_version() >= 500 has this entry point. */
int sigp_dist_init_transport2(sigp_handle* h, int nranks, int rank, const sigp_transport* tr, int64_t struct_bytes);
int sigp_dist_fit(sigp_handle* h, int kernel_id, double ell, double sn_tilde, const double* Sigma, int64_t ldsigma, int64_t W, int lookahead,
                  double* out, double* mean, double* var);
/* Predictions at NEW test points after a sharded fit (north/June1st.py:272-277): collective -- every rank calls it with the same Xs [m,d]
 * and gets the same mean / var (var includes sigma_n).  mean = k~*^T alpha~ with alpha~ = K~^-1 y replicated once per fit (fp64: one backward
 * solve on the distributed factor; fp32: the refined solution); var from forward solves on the distributed factor, 4 points per pass, the
 * squares summed per rank and all-reduced once.  RBF / Matern fits; fp32 handles: the variance carries the fp32 factor's accuracy
 * (as sigp_predict on an fp32 handle). */
int sigp_dist_predict(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, double* mean, double* var);
int sigp_dist_shutdown(sigp_handle* h);                                /* destroy the communicator, free the sharded storage */
int64_t sigp_num_blocks(sigp_handle* h);                               /* T = n_pad / 128                        */

/* measurement ---------------------------------------------------------------------------------- */
/* enable=1: bracket every kernel launch with HIP events on the stream it is launched on and
 * accumulate per kernel class; enable = bit mask with bit (8+k) set: only kernel class k (less perturbation);
 * enable=0: off (default).  sigp_profile_get drains finished events. */
int sigp_profile(sigp_handle* h, int enable);
int sigp_profile_get(sigp_handle* h, int kclass, double* total_ms, int64_t* launches, double* flops,
                     double* bytes);
int sigp_profile_reset(sigp_handle* h);
/* Wait for everything the handle's device has been given (hipDeviceSynchronize on the handle's device).  Every entry point above is
 * synchronous on return already; a caller that brackets a timed region (bench.py) uses this for the bracket itself, so that the
 * measurement runs on the HIP runtime the library links and needs no second one (PyTorch's) in the process. */
int sigp_synchronize(sigp_handle* h);
/* tuning knobs; returns SIGP_BAD_ARG for an unknown name or an invalid value.  Defaults in brackets.
 *   outer_blocks [8]      outer panel width in 128-column blocks (K of the trailing update = 128 x this); left unset, single fits of at most
 *                         24 block columns (n <= 3072) are one panel
 *   lookahead [1]         factor the next panel on the panel stream while the trailing update runs
 *   schedule [0]          0 right-looking outer panels, 1 left-looking (same factor bit for bit)
 *   panel_mode [2]        rows below a panel's top block: 0 recursion, 1 strip solve, 2 strips when strips x members >= strip_min [512]
 *   accurate_solve [0]    1: one residual-correction step behind every product with an inverted diagonal block in the factorisation's column solves
 *                         and in the block solves of sigp_predict / sigp_predict_cov / sigp_get_alpha (see sigp_potrf: LAPACK-grade accuracy on
 *                         ill-conditioned diagonal blocks; overrides panel_mode and bit 2 of panel_chain while on; 0 / 1, fp64 handles only)
 *   diag_tiles [1]        symmetric trailing updates: a diagonal 128 x 128 tile loads, multiplies and stores only the 36 of its 64 16 x 16 pairs on or below
 *                         the diagonal (nothing reads the rest; same lower halves bit for bit; 0 = whole tiles, for A/B timing)
 *   ride_tiles [1]        trailing updates: while at most 16 rows of the ride-along block are in use (y and up to 15 test points), its tiles stage and
 *                         multiply those 16 rows only (the other rows are zero rows; same results bit for bit; 0 = whole tiles, for A/B timing)
 *   strip_tri [1]         strip solves skip the zero 16-column x 16-k tile-slices of the inverse diagonal blocks (same bits; 0 = the full products, for A/B timing)
 *   group [8]             fits factorised in lockstep per launch (batch path, fp64 and fp32; 1..256)
 *   loo_grad_tri [1]      sigp_loo_grad: the cubic step multiplies the upper triangle of dK~ only (n^3 flops; 0 = the full product, 2 n^3, for A/B timing:
 *                         another summation order, the same result to rounding)
 *   cov_slices [0]        sigp_predict_cov: K slices of the covariance product Z Z^T (one workgroup per 128 x 128 tile pair and slice): 0 = auto, the
 *                         smallest count that gives every CU two workgroups (capped by the n_pad / 128 block columns and by 1 GiB of partial
 *                         tiles); 1 .. n_pad / 128 = fixed (1: no partials, one workgroup walks the whole K of its tile)
 *   sparse_chunk [4096]   sigp_sparse_fit: rows of X per chunk (a multiple of 128 in 128 .. 65536; the last chunk may be shorter): the K of the
 *                         accumulation V_c V_c^T and the width of the whitening's products; V_c takes 8 m_pad sparse_chunk bytes
 *   cv_slices [0]         sigp_cv / sigp_cv_batch: K slices of the strip product U_S U_S^T (one workgroup per fold, slice and member): 0 = auto, the
 *                         smallest count that gives every CU two workgroups from one member's folds (at most 32; the same for a fit and for a lockstep group); otherwise the count, clipped to the 32-column stages
 *                         of the fit (1: one workgroup walks the whole strip); sigp_get_stat "cv_slices" = what the last call ran with
 *   small_tile_threshold [320], tiny_tile_threshold [256], trsm128_threshold [256]   tile-shape switches by tile count
 *   refine_iters [3]      fp32 engine: fp64 refinement steps at most; refine_tol_e [12]: stop once every residual is <= 1e-12 (0 = never early)
 *   refine_stored [1]     fp32 engine: the covariance build also writes K~ in fp64 (8 n^2 bytes per lockstep member, skipped above 40 GB) and the
 *                         refinement's residuals read it (HBM-bound) instead of recomputing n^2 covariances each; 0 = recompute (no extra memory)
 *   refine_sym [1]        ... reading the stored lower triangle ONCE per residual (4 n^2 bytes; row and column sums of every tile from LDS), 0 = in two passes
 *   owner_only [0]        sigp_set_train does not allocate the n x n single-GPU matrix (sigp_dist_fit); dist_stats [0] see sigp_dist_fit;
 *   dist_segment [2]      column blocks per streamed broadcast segment of the sharded fit (>= the panel width: panels travel whole)
 *   dist_panel_split [-1] (-1 = by the number of ranks: on from four; 0 / 1)  sharded fit, panel exchange by ROW PIECES ("all-gather of block-row pieces"): the owner factors only the panel's W x W top
 *                         block and broadcasts it (8 MB at W = 8); the rows below it are scattered in `world` pieces, every rank solves its piece, and
 *                         an in-place all-gather assembles the panel on every rank -- the owner's throughput work leaves the chain and each link carries
 *                         1/world of the panel instead of all of it.  Rows are independent: bit-identical to dist_panel_split = 0 wherever both run the same
 *                         tile kernels (every order up to ~ 10 000 at W = 8); beyond, a whole panel's in-panel updates go to the 128-tile kernel and a
 *                         row piece's do not (another k order inside a 16-slice): last-bit differences.
 *   dist_lookahead2d [1]  with the row-split exchange: the NEXT panel's first update is divided by rows as well -- every rank applies it to its own piece
 *                         before solving it; the next owner keeps the update of its top block (from the rows right below the panel's top block, which the
 *                         owner solves itself behind its chain and broadcasts ahead of the pieces) and starts its chain beside the piece solves and the
 *                         all-gather.  A schedule: bit-identical to 0 at every tested shape.
 *   ride_reps [0]         tile pairs per riding workgroup of the diagonal-block launch (0 = one; -1 = by the launch, about four riders per CU; n = fixed):
 *                         shortens that launch in lockstep batches and lengthens the trailing update beside it by as much (docs/EXPERIMENTS.md)
 *   dist_timeout_ms [120000] deadline (time WITHOUT progress of the update stream's panel counter) of every host-side wait of the sharded path; RCCL's asynchronous error state is polled meanwhile.  On an
 *                         error / when it passes: ncclCommAbort, SIGP_HIP_ERROR (the panel reached is in sigp_last_error), the handle's sharded
 *                         state is dead until sigp_dist_shutdown + a fresh sigp_dist_init* -- a dead peer is an error, not a hang; 0 = wait for ever
 *   strips_after_update [1] (look-ahead: the next panel's strip solve -- MFMA work for the whole chip -- waits for the rest of the trailing update; 0 = beside
 *   it: same throughput, a batch is bound by the sum of its MFMA work, but the update's launches then last as long as both kernels' work: bench.py's
 *   roofline.strips_beside_update)
 *   schedules of the latency chain -- bit-identical results, DESIGN.md section 7:  panel_chain [15] (bit 0: panels that are not strip-solved,
 *   bit 1: top blocks of strip-solved panels, are factored column by column with update work riding in the diagonal-block launches;
 *   bit 2: ONE launch between two diagonal blocks (chain_link_kernel: what the next block needs, the column solve riding, every other update
 *   riding in the next diagonal-block launch), bit 3: the binary recursion's two-column leaves take that form too; 0 = binary recursion), chain_rows [80] (bit 0 applies while rows-below x members <= this),
 *   first_on_panel [1] (the update of the next panel's columns on the panel stream: 0 never, 1 for chain-form panels, 2 always)
 *   pan_priority, diag_prio, host_timing   measurement switches
 * The rejected experiments of DESIGN.md section 7 (xcd_chunks, update_wgs / update_late, pipeline_head / head_gate, wide_tiles, n64_tiles,
 * patch, small_nt64, reserve_cus, panel_ll, c_dma, syrk_v2) are compiled into libsigp_debug.so only (make debug; include/sigp_debug.h):
 * the product library answers SIGP_BAD_ARG to their names and carries none of their kernels. */
int sigp_set_option(sigp_handle* h, const char* name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SIGP_H */
