// sigp_cv_grad_ard: the leave-block-out scores AND the exact derivatives of one of them with respect to (log l_1 .. log l_d, log sn~)
// (cvard.hpp has the formulae and the kernels).  Included inside extern "C" of sigp.hip, after sigp_scores.inc (the shared steps),
// sigp_blockcv.inc and sigp_looard.inc.
//
// The scales are set and the fit is made as sigp_loo_grad_ard makes it (ard_theta_fit: ell = 1, sigp_fit_predict's own launches); then cv_launch (U = L~^-T
// in gU, the scores: the same launches as sigp_cv, so the same bits) with, per pass of at most 1024 folds:
//   beta_f, B_f, eps_f   cv_adj_fold_kernel, right after the closing solves (the fold blocks are overwritten by the next pass)
//   beta, B              cv_adj_gather_kernel: the folds' terms added in ascending fold order into beta [n_pad] and the band store [n_pad][384]
// and on top of it:
//   P = U U^T            kinv_lower: lower 128-tiles into gK (n^3/3);  a = U z (alpha_from_U);  mirror_P         (sigp_loo_grad_ard's launches)
//   eps, v = P beta      cv_adj_eps_kernel, cv_adj_v_kernel (one pass over the rows of P, which also zeroes its padding)
//   P B into gD          cv_band_product_kernel: the 128-tile loop over the three block columns of B's band (6 x 128 n_pad^2 flops)
//   M = (P B) P^T        lower 128-tiles into gU, which is dead by then: syrk_set (n^3 flops for any d)
//   the ARD pass         loo_ard_pass, as sigp_loo_grad_ard
// Memory: sigp_loo_grad's single-fit buffers (gU, gK, gD, gV, gPart), ardXc, sigp_cv's workspaces and cvAdj: the band store, B_f / beta_f of one
// pass and eps_f.  Profile class: SIGP_KC_MLII (on top of cv_launch's entries: two per pass, then U U^T, the n^2 passes, the banded
// product, the product M, the ARD pass: one entry each).
// Out of scope: sigp_small_*, the reference kernel, the fp32 engine, sharded fits.  Lockstep groups: sigp_cv_grad_ard_batch
// (sigp_cvardbatch.inc), which runs the steps below -- cv_adj_zero, cv_launch with the adjoint, cv_ard_products -- with a member axis.

// The adjoint's accumulators of nb members before cv_launch's first pass: the band stores (contiguous) and every member's beta
static int cv_adj_zero(sigp_handle* h, hipStream_t st, int nb, long n_pad, const CvAdjoint& adj) {
  HIPCHK(h, hipMemsetAsync(adj.band, 0, (size_t)((nb - 1) * adj.sBand + n_pad * CVA_BAND) * sizeof(double), st));
  for (int b = 0; b < nb; ++b) HIPCHK(h, hipMemsetAsync(adj.beta + b * adj.sBeta, 0, (size_t)n_pad * sizeof(double), st));
  return SIGP_OK;
}

// ONE launch of cv_band_product_kernel for nb members: C = P B, T x T tiles each, P and C [n_pad][ld] sP apart, the band stores sBand apart.
// cv_ard_products and the debug library's run-and-return entry (sigp_debug_run_cv_band) both launch through here.  The refusal guards the
// tile's 32-bit DMA offsets (syrk128.hpp); it needs a row of 32 MiB, a matrix no test can allocate: it is not reached by any test.
static int launch_cv_band_product(sigp_handle* h, hipStream_t st, int nb, const double* P, long ld, const double* band, double* Cm, int T, long sP, long sBand) {
  if (!sy_row_stride_ok(ld, sizeof(double))) return fail(h, SIGP_BAD_ARG, "cv band product: row stride beyond the tile's 32-bit DMA offsets");
  static AttrOnce b_attr;
  HIPCHK(h, b_attr.set(h->device, (const void*)cv_band_product_kernel, SY_LDS_BYTES));
  hipLaunchKernelGGL(cv_band_product_kernel, dim3((unsigned)T, (unsigned)T, (unsigned)nb), dim3(256), SY_LDS_BYTES, st, P, ld, band, Cm, ld, T, sP, sBand);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// The gradient's steps between cv_launch (with adj) and the ARD pass, for nb lockstep members: P into gK, a, eps and v into the members'
// vectors (w = member 0's, the others sW apart; z = the members' solved ride row 0, sZ apart), P B into gD, M = (P B) P^T into gU.  One
// member with zero strides is the single fit.  Four profile entries, their figures times nb.
static int cv_ard_products(sigp_handle* h, hipStream_t st, int nb, long n, long n_pad, long F, const double* z, long sZ, const CvAdjoint& adj, LooArdVecs w, long sW) {
  const long ld = n_pad, sP = n_pad * n_pad;
  const int T = (int)(n_pad / NB);
  int rc;
  if ((rc = kinv_lower(h, st, nb, n_pad))) return rc;
  {   // a = U z;  P -> full;  eps;  v = P beta (and the padding of P zeroed)
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 4.0 * n_pad * n_pad, nb * 28.0 * n_pad * n_pad);
    if ((rc = alpha_from_U(h, st, nb, z, sZ, w.a(), sW, n_pad))) return rc;
    if ((rc = mirror_P(h, st, nb, n_pad))) return rc;
    hipLaunchKernelGGL(cv_adj_eps_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)adj.epsf, (int)F, w.eps(), adj.sEps, sW);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(cv_adj_v_kernel, dim3((unsigned)(n_pad / 4), (unsigned)nb), dim3(256), 0, st, h->gK, ld, (int)n, (int)n_pad, (const double*)w.beta(), w.v(), sP, sW);
    HIPCHK(h, hipGetLastError());
  }
  {   // P B: tile (bi, bj) = rows bi of P against rows bj of the band store, the K window of B's three block columns
    ProfScope ps(h, st, SIGP_KC_MLII, nb * (2.0 * n_pad * n_pad * CVA_BAND), nb * (8.0 * n_pad * n_pad));
    if ((rc = launch_cv_band_product(h, st, nb, h->gK, ld, adj.band, h->gD, T, sP, adj.sBand))) return rc;
  }
  {   // M = (P B) P^T: tile (bi, bj), bi >= bj, = rows bi of P B against rows bj of P (= its columns), the whole K span
    ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n_pad * n_pad * (n_pad + NB)), 0.0);
    if ((rc = syrk_set(h, st, nb, h->gD, h->gK, h->gU, n_pad, 1, 0))) return rc;
  }
  return SIGP_OK;
}

int sigp_cv_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int64_t block, int64_t gap, int sigma_mode, int criterion, double* mean,
                     double* var, double* score, double* grad) {
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "cv_grad_ard: bad argument (theta [d + 1], score [2] required)");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "cv_grad_ard: mean and var come together (both NULL: scores and gradient only)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "cv_grad_ard: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "cv_grad_ard: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  int rc;
  if ((rc = ard_check_engine(h, "cv_grad_ard", kernel_id))) return rc;
  if (h->n < 2) return fail(h, SIGP_BAD_ARG, "cv_grad_ard: cross-validation needs n >= 2 training points");
  if ((rc = ard_check_theta(h, "cv_grad_ard", ntheta))) return rc;
  if (const char* why = cv_check_folds(h->n, block, gap, SIGP_CV_MAX_WINDOW))
    return fail(h, SIGP_BAD_ARG, "cv_grad_ard: %s (block = %lld, gap = %lld, n = %ld, SIGP_CV_MAX_WINDOW = %d)", why, (long long)block, (long long)gap, h->n, SIGP_CV_MAX_WINDOW);
  double snt, out[4];
  rc = ard_theta_fit(h, kernel_id, theta, &snt, out);
  if (rc == SIGP_NOT_SPD) return ard_all_inf(h, score, grad, mean, var);
  if (rc) return rc;

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, ld = n_pad;
  const long F = (n + block - 1) / block, FP = std::min<long>(F, CV_PASS_BLOCKS);
  const long wp = round_up(std::min<long>(n, block + 2 * gap), 16);
  if ((rc = ard_scores_ensure(h, grad != nullptr))) return rc;
  if ((rc = cv_work_ensure(h, n, block, gap, 1, 0))) return rc;
  if (grad && (rc = ensure(h, &h->cvAdj, &h->cap_cvAdj, CvAdjStore::size(n_pad, FP, wp, F)))) return rc;
  const ScoreArdParts ap{h->gPart, n_pad, kbuild_tiles(n_pad), h->dp};   // the scores as sigp_cv has them; then the tile pass's partials and the gradient
  const ScoreParts sp = ap.scores();
  const LooArdVecs w{h->gV, n_pad};
  CvAdjoint adj{};
  if (grad) {
    adj = CvAdjStore{h->cvAdj, n_pad, FP, wp, F}.adjoint(criterion, w.beta());
    if ((rc = cv_adj_zero(h, st, 1, n_pad, adj))) return rc;
  }
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = cv_launch(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, h->y, 0, nullptr, sp.q(), 0, sigma_mode, sp, cv_work(h, 1, n, block, gap), (int)block, (int)gap,
                      grad ? &adj : nullptr))) return rc;
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  // a fold whose P_SS failed its pivot test left +inf in both sums
  auto finish = [&]() -> int {
    if ((rc = sync_slot(h, s))) return rc;
    return std::isfinite(score[0]) && std::isfinite(score[1]) ? SIGP_OK : ard_all_inf(h, score, grad, mean, var);
  };
  if (!grad) return finish();

  if ((rc = cv_ard_products(h, st, 1, n, n_pad, F, s.mat + n_pad * ld, 0, adj, w, 0))) return rc;
  if ((rc = loo_ard_pass(h, st, kernel_id, w, ap, snt, grad))) return rc;
  return finish();
}
