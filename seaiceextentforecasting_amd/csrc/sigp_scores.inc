// The steps the score and gradient entry points share: sigp_nlml_grad(_batch / _ard), sigp_loo(_batch), sigp_loo_grad(_batch / _ard), sigp_cv(_batch)
// and sigp_cv_grad_ard.  Included inside extern "C" of sigp.hip, before sigp_nlml_grad.  Host code only: each launch sequence is written
// once here and the entry points call the steps in order.  Every step takes the number of lockstep members nb; a single fit is nb = 1.
//
// Workspaces: gU [n_pad][n_pad] holds U = L~^-T, gK [n_pad][n_pad] parks the inversion's products and then holds P = K~^-1, both with member
// stride n_pad^2.  Every other arena's layout: score_layout.hpp.

// ---- workspaces ------------------------------------------------------------------------------------------------------------------------------
// An entry point grows every buffer it will touch here, before its first launch, and builds its views afterwards: growing a buffer later
// would drop what the earlier launches left in it, and the launch helpers below take views and grow nothing.
// gU and gK for G lockstep members, and gPart for the view the entry lays over it (`parts` = that view's size)
static int scores_ensure(sigp_handle* h, int G, long n_pad, long parts) {
  int rc;
  if ((rc = ensure(h, &h->gU, &h->cap_gU, (long)G * n_pad * n_pad))) return rc;
  if ((rc = ensure(h, &h->gK, &h->cap_gK, (long)G * n_pad * n_pad))) return rc;
  return ensure(h, &h->gPart, &h->cap_gPart, parts);
}

// ... and what a gradient pass adds: the second matrix operand gD and gvec doubles of vectors per member (0: none)
static int scores_grad_ensure(sigp_handle* h, int G, long n_pad, long gvec) {
  int rc;
  if ((rc = ensure(h, &h->gD, &h->cap_gD, (long)G * n_pad * n_pad))) return rc;
  return ensure(h, &h->gV, &h->cap_gV, (long)G * gvec);
}

// ... the MLII entries: a = U z in scratchZ (zlen doubles), and for a per-feature gradient the centred features [G][n_pad][dp] in ardXc (dp = 0: none)
static int scores_mlii_ensure(sigp_handle* h, long zlen, int G, long n_pad, long dp) {
  int rc;
  if ((rc = ensure(h, &h->scratchZ, &h->cap_Z, zlen))) return rc;
  return ensure(h, &h->ardXc, &h->cap_ardXc, (long)G * n_pad * dp);
}

// ---- the cubic steps -------------------------------------------------------------------------------------------------------------------------
// U = L~^-T (upper triangular, row-major) into gU by trtri_levels, its products parked in gK: n^3/3 flops per member
static int inv_factor(sigp_handle* h, hipStream_t st, int nb, const double* Lm, long sL, const double* dinvp, long sD, long n_pad) {
  const int T = (int)(n_pad / NB);
  ProfScope ps(h, st, SIGP_KC_MLII, nb * (double)n_pad * n_pad * n_pad / 3, 0.0);
  return trtri_levels<double>(h, st, Lm, n_pad, dinvp, h->gU, h->gK, n_pad, T, T, nb, sL, sD, n_pad * n_pad);
}

// C = A B^T on 128-tiles of n_pad x n_pad operands (member stride n_pad^2) by syrk128_kernel's SET form: the lower tile space or the full
// one; ktri = 1: K runs from the row block on (rows of A -- and of B, on the lower space -- are zero left of their diagonal block).
// No profile entry of its own: the callers' flop figures differ.
static int syrk_set(sigp_handle* h, hipStream_t st, int nb, const double* A, const double* B, double* C, long n_pad, int lower, int ktri) {
  const int T = (int)(n_pad / NB);
  GemmArgs g{};
  g.A = A; g.lda = n_pad; g.B = B; g.ldb = n_pad; g.C = C; g.ldc = n_pad; g.K = (int)n_pad;
  g.batch = nb; g.sA = g.sB = g.sC = n_pad * n_pad;
  g.r0 = 0; g.r1 = T; g.c0 = 0; g.c1 = T; g.lower = lower; g.ktri = ktri;
  return launch_syrk128_t<double, true>(h, st, g);
}

// P = K~^-1 = U U^T on the lower 128-tiles of gK (rows of U are zero left of their diagonal block, so tile (i, j) sums k from 128 i: n^3/3)
static int kinv_lower(sigp_handle* h, hipStream_t st, int nb, long n_pad) {
  ProfScope ps(h, st, SIGP_KC_MLII, nb * (double)n_pad * n_pad * n_pad / 3, 0.0);
  return syrk_set(h, st, nb, h->gU, h->gU, h->gK, n_pad, 1, 1);
}

// ---- the n^2 steps (no profile entries of their own: the callers book them with their other n^2 passes) -----------------------------------------
// a = U z: one skinny product with the upper-triangular U (one wave per row, k from the diagonal) instead of a backward block solve of two
// launches per 128 columns.  z = the members' solved ride row 0 (stride sZ), out with stride sOut.
static int alpha_from_U(sigp_handle* h, hipStream_t st, int nb, const double* z, long sZ, double* out, long sOut, long n_pad) {
  hipLaunchKernelGGL(rowdot_kernel<double>, dim3((unsigned)((n_pad + 3) / 4), (unsigned)nb), dim3(256), 0, st, (const double*)h->gU, n_pad, (int)n_pad, (int)n_pad, 2,
                     z, n_pad, out, n_pad, 1, 0, (const double*)nullptr, 0, 0, n_pad * n_pad, sZ, sOut);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// the lower 128-tiles of P in gK -> the full symmetric matrix
static int mirror_P(sigp_handle* h, hipStream_t st, int nb, long n_pad) {
  hipLaunchKernelGGL(loo_grad_mirror_kernel, dim3((unsigned)(n_pad / 32), (unsigned)(n_pad / 32), (unsigned)nb), dim3(256), 0, st, h->gK, n_pad, n_pad * n_pad);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// ---- per-feature (ARD) gradients ---------------------------------------------------------------------------------------------------------------
// The tile pass over scaled features U [n_pad][dp] (nb lockstep members, strides ms): their centred copy into ardXc, then every tile's share
// of all d components into partial [tiles][dp].  W = ARD_W_NLML: M = K~^-1 (lower tiles), a, q = y^T a;  W = ARD_W_LOO: M, a, v, eps of
// looard.hpp (q is not read; v and eps at the strides ms.v, ms.eps).  The callers launch their own finish kernel, and book the pass and the finish under one profile
// entry of their own.  ard_tile_pass: the single fit -- the handle's own features, one member, zero strides.
extern "C++" {
template <int W>
static int ard_tile_pass_members(sigp_handle* h, hipStream_t st, int nb, const double* U, long n, long d, long dp, long n_pad, ArdMemberStrides ms, int kernel_id,
                                 const double* M, long ldm, const double* a, const double* q, const double* v, const double* eps, double* partial) {
  const long ntiles = kbuild_tiles(n_pad);
  const int kid = kernel_id == SIGP_KERNEL_RBF ? KID_RBF : KID_MATERN52;
  HIPCHK(h, hipMemsetAsync(h->ardXc, 0, (size_t)(ms.U * (nb - 1) + n_pad * dp) * sizeof(double), st));
  hipLaunchKernelGGL(ard_center_kernel, dim3((unsigned)d, (unsigned)nb), dim3(256), 0, st, U, (int)dp, (int)n, h->ardXc, ms.U);
  if (d <= 8)
    hipLaunchKernelGGL((ard_grad_partial_kernel<8, W>), dim3((unsigned)ntiles, (unsigned)nb), dim3(256), 0, st, U, (const double*)h->ardXc, (int)dp, (int)d, (int)n, kid, M, ldm,
                       a, q, partial, v, eps, ms);
  else
    hipLaunchKernelGGL((ard_grad_partial_kernel<32, W>), dim3((unsigned)ntiles, (unsigned)nb), dim3(256), 0, st, U, (const double*)h->ardXc, (int)dp, (int)d, (int)n, kid, M, ldm,
                       a, q, partial, v, eps, ms);
  return SIGP_OK;
}
template <int W>
static int ard_tile_pass(sigp_handle* h, hipStream_t st, int kernel_id, const double* M, long ldm, const double* a, const double* q, const double* v,
                         const double* eps, double* partial) {
  return ard_tile_pass_members<W>(h, st, 1, h->X, h->n, h->d, h->dp, h->n_pad, ArdMemberStrides{0, 0, 0, 0, 0, 0, 0}, kernel_id, M, ldm, a, q, v, eps, partial);
}
}  // extern "C++"

// The checks the three ARD entries have in common (`what` = the message prefix), in two parts: each entry has checks of its own between
// them, and the order of the refusals stays what it was
static int ard_check_engine(sigp_handle* h, const char* what, int kernel_id) {
  if (h->n == 0) return fail(h, SIGP_BAD_ARG, "%s: call set_train first", what);
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "%s: fp64 engine only", what);
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "%s: RBF / MATERN52 only", what);
  return SIGP_OK;
}
static int ard_check_theta(sigp_handle* h, const char* what, int64_t ntheta) {
  if (ntheta != h->d + 1) return fail(h, SIGP_BAD_ARG, "%s: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", what, h->d + 1, (long long)ntheta);
  return SIGP_OK;
}

// The head the three ARD entries share, after their checks: l = exp(theta[0 .. d)), sn~ = exp(theta[d]), the scales staged and the fit made at ell = 1 on the
// scaled features (sigp_fit_predict's own launches).  SIGP_OK (snt and out4 = sigma_f, nlML, info, sigma_n set), SIGP_NOT_SPD (exp
// overflowed or K~ is not SPD: the caller fills its outputs with inf) or an error.
static int ard_theta_fit(sigp_handle* h, int kernel_id, const double* theta, double* snt, double out4[4]) {
  const long d = h->d;
  std::vector<double> ell((size_t)d);
  for (long k = 0; k < d; ++k) ell[(size_t)k] = std::exp(theta[k]);
  *snt = std::exp(theta[d]);
  for (long k = 0; k < d; ++k)
    if (!std::isfinite(ell[(size_t)k]) || !(ell[(size_t)k] > 0)) return SIGP_NOT_SPD;
  if (!std::isfinite(*snt)) return SIGP_NOT_SPD;
  int rc;
  if ((rc = sigp_set_length_scales(h, ell.data(), d))) return rc;
  return sigp_fit_predict(h, kernel_id, 1.0, *snt, nullptr, 0, out4, nullptr, nullptr);
}

// ... and what sigp_loo_grad_ard / sigp_cv_grad_ard hand back on SIGP_NOT_SPD (grad, mean / var may be NULL)
static int ard_all_inf(sigp_handle* h, double* score, double* grad, double* mean, double* var) {
  const double inf = std::numeric_limits<double>::infinity(), qnan = std::nan("");
  score[0] = score[1] = inf;
  if (grad) for (long k = 0; k <= h->d; ++k) grad[k] = inf;
  if (mean) for (long i = 0; i < h->n; ++i) mean[i] = var[i] = qnan;
  return SIGP_NOT_SPD;
}

// sigp_loo_grad_ard / sigp_cv_grad_ard: the single fit's score buffers (without a gradient: ScoreParts of one member; ScoreArdParts begins with
// them) and, for a gradient, gD, the vectors and the centred features
static int ard_scores_ensure(sigp_handle* h, bool grad) {
  const long n_pad = h->n_pad, dp = h->dp;
  int rc;
  if ((rc = scores_ensure(h, 1, n_pad, grad ? ScoreArdParts::size(n_pad, kbuild_tiles(n_pad), dp) : ScoreParts::size(1, n_pad)))) return rc;
  if (!grad) return SIGP_OK;
  if ((rc = scores_grad_ensure(h, 1, n_pad, LooArdVecs::size(n_pad)))) return rc;
  return ensure(h, &h->ardXc, &h->cap_ardXc, n_pad * dp);
}

// ---- single fits: q and the read-back ------------------------------------------------------------------------------------------------------
// q = y^T A~ behind the one member's scores -- the host copy of the fit's epilogue (s.res may have moved on)
static int scores_stage_q(sigp_handle* h, hipStream_t st, ScoreParts sp) {
  HIPCHK(h, hipMemcpyAsync(sp.q(), h->fit_res.data(), sizeof(double), hipMemcpyHostToDevice, st));
  return SIGP_OK;
}

// mean, var [n] (may be NULL together) and score [2] on their way to the caller; complete after sync_slot
static int scores_to_host(sigp_handle* h, hipStream_t st, long n, ScoreParts sp, double* mean, double* var, double* score) {
  if (mean) {
    HIPCHK(h, hipMemcpyAsync(mean, sp.mean(0), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(var, sp.var(0), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipMemcpyAsync(score, sp.sums(), 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  return SIGP_OK;
}

// ---- lockstep groups on the resident batch data (sigp_batch_upload) ---------------------------------------------------------------------------
static int batch_check_params(sigp_handle* h, const char* what, int64_t count, const double* ell, const double* sn_tilde) {
  for (int64_t i = 0; i < count; ++i)
    if (!(ell[i] > 0) || !std::isfinite(ell[i]) || !(sn_tilde[i] >= 0) || !std::isfinite(sn_tilde[i])) return fail(h, SIGP_BAD_ARG, "%s: finite ell > 0 and sn_tilde >= 0 required", what);
  return SIGP_OK;
}

// One group of nb members through the fit on data sets laid out as the resident ones (X [.][n_pad][dp], y [.][n_pad], Xs [.][RIDE][dp]): member b
// has (ell[b], snt[b]) and data set ds[b], m ride points.  Covariance build, blocked Cholesky, epilogue: q stays on the device in the slot's
// result rows, and the parameters uploaded here stay put until the next group's (y of member b is data set s.kps[b].ds).
static int batch_group_fit_on(sigp_handle* h, Slot& s, int nb, int kernel_id, const double* ell, const double* snt, const int* ds, const double* X, const double* y,
                              const double* Xs, long m) {
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, n_pad = h->b_npad;
  int rc;
  for (int b = 0; b < nb; ++b) s.kps_host[b] = make_kparams(kernel_id, ell[b], snt[b], ds[b]);
  if ((rc = upload_kparams(h, s, nb))) return rc;
  if ((rc = build_cov(h, s, nb, X, n_pad * dp, y, n_pad, Xs, (long)RIDE * dp, n, d, dp, n_pad, m))) return rc;
  if ((rc = potrf_slot(h, s, nb, n_pad, false, 1 + (int)m))) return rc;
  return epilogue_slot(h, s, nb, n, n_pad, m);
}

// ... on the resident batch data: member b has data set (first_ds + b) % batch, no ride points.  sigp_batch_run has its own loop: concurrency
// and slots, which the score entries do without.
static int batch_group_fit(sigp_handle* h, Slot& s, int nb, int kernel_id, const double* ell, const double* snt, long first_ds) {
  std::vector<int> ds((size_t)nb);
  for (int b = 0; b < nb; ++b) ds[(size_t)b] = (int)((first_ds + b) % h->b_count);
  return batch_group_fit_on(h, s, nb, kernel_id, ell, snt, ds.data(), h->bX, h->by, h->bXs, 0);
}

// a group's rows (mv [nb][2][n_pad] <- mean, var; NULL: none) and sums (sc [nb][2]) on their way to the host, nb <= sp.G
static int batch_scores_fetch(sigp_handle* h, hipStream_t st, int nb, ScoreParts sp, double* mv, double* sc) {
  const long n_pad = sp.n_pad;
  if (mv) HIPCHK(h, hipMemcpy2DAsync(mv, (size_t)2 * n_pad * sizeof(double), sp.mean(0), (size_t)sp.mstride() * sizeof(double), (size_t)2 * n_pad * sizeof(double), (size_t)nb, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(sc, sp.sums(), (size_t)nb * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  return SIGP_OK;
}

// fit i of the call <- one member's sums sc [2] and rows mv [2][n_pad] (NULL with mean / var): +inf scores and NaN rows unless ok
static void batch_scores_scatter(long i, bool ok, const double* sc, const double* mv, long n, long n_pad, double* mean, double* var, int64_t nstride, double* score) {
  const double inf = std::numeric_limits<double>::infinity(), qnan = std::nan("");
  score[2 * i] = ok ? sc[0] : inf;
  score[2 * i + 1] = ok ? sc[1] : inf;
  if (!mean) return;
  for (long j = 0; j < n; ++j) {
    mean[i * nstride + j] = ok ? mv[j] : qnan;
    var[i * nstride + j] = ok ? mv[n_pad + j] : qnan;
  }
}

// The parameters of the derivative covariance dK~/dlog l of nb RBF / Matern members into gKps: member b has length scale ell[b] and data set
// ds[b].  gKps is sized for the slot's whole lockstep capacity, so a later, larger group of the same call never reallocates it.  From
// pageable memory: the copy call returns once the host buffer has been staged, so the vector may go out of scope.
static int upload_dlogl_kparams(sigp_handle* h, hipStream_t st, int nb, int kernel_id, const double* ell, const int* ds) {
  std::vector<KParams> dkp((size_t)nb);
  for (int b = 0; b < nb; ++b) dkp[(size_t)b] = make_kparams(kernel_id == SIGP_KERNEL_RBF ? KID_RBF_DLOGL : KID_MATERN52_DLOGL, ell[b], 0.0, ds[b]);
  if (h->cap_gKps < nb) {
    const int cap = std::max(nb, h->slots[0].capB);
    HIPCHK(h, hipDeviceSynchronize());
    if (h->gKps) HIPCHK(h, hipFree(h->gKps));
    h->gKps = nullptr; h->cap_gKps = 0;
    HIPCHK(h, hipMalloc((void**)&h->gKps, (size_t)cap * sizeof(KParams)));
    h->cap_gKps = cap;
  }
  HIPCHK(h, hipMemcpyAsync(h->gKps, dkp.data(), (size_t)nb * sizeof(KParams), hipMemcpyHostToDevice, st));
  return SIGP_OK;
}
