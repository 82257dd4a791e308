// sigp_loo_grad_ard: the leave-one-out scores AND the exact derivatives of one of them with respect to (log l_1 .. log l_d, log sn~)
// (looard.hpp has the formulae and the kernels).  Included inside extern "C" of sigp.hip, after sigp_scores.inc (the shared steps),
// sigp_loograd.inc and sigp_ardgrad.inc.
//
// The scales are set and the fit is made as sigp_nlml_grad_ard makes it (ard_theta_fit: ell = 1, sigp_fit_predict's own launches); then, on
// top of loo_launch (U = L~^-T in gU, the scores: the same launches as sigp_loo, so the same bits):
//   P = U U^T        kinv_lower: lower 128-tiles into gK (n^3/3);  a = U z (alpha_from_U);  mirror_P: P to the full symmetric matrix
//   beta, gamma, eps the coefficients of the chosen score and sigma mode (loo_ard_coef_kernel: a, diag P and q from device memory)
//   v = P beta, P Gamma into gD, one pass over the rows of P (loo_ard_scale_kernel)
//   M = (P Gamma) P^T lower 128-tiles into gU, which is dead by then: syrk_set on the lower tile space, whole diagonal tiles
//                    (the DG form of a diagonal tile belongs to the product form !SET alone, and A != B here anyway): n^3 flops for any d
//   the ARD pass     loo_ard_pass (one member of loo_ard_pass_members): the tile pass with ARD_W_LOO over M, v, a, eps, then loo_ard_finish_kernel
// Memory: sigp_loo_grad's single-fit buffers (gU, gK, gD, gV, gPart; gPart also holds the pass's per-tile partials) plus ardXc.
// Profile class: SIGP_KC_MLII (on top of loo_launch's two entries: U U^T, the n^2 passes, the product M, the ARD pass: one entry each).
// Out of scope: sigp_small_*, the fp32 engine, sharded fits.  Lockstep groups: sigp_loo_grad_ard_batch (sigp_looardbatch.inc), which runs
// these launches with a member axis.  The leave-block-out scores: sigp_cvard.inc.

// The ARD pass of a leave-one-out / leave-block-out score (sigp_cv_grad_ard shares it) over M in gU with the vectors w: every tile's share of
// all d components, then the fixed-order sums; the gradient [d + 1] on its way to the caller.  The partials and the gradient lie in ap.
// The member form (sigp_loo_grad_ard_batch): nb lockstep members on scaled features U [nb][n_pad][dp] (member stride sU), member b's M at
// M + b ls.P (gU here and for the leave-block-out scores, gD for the hindcast scores), vectors, partials and gradient at b times the
// strides of ls behind w, partial and gdev (ls.grad = d + 1: the group's gradients go to the
// host in one copy), its sn~ in sn_m[b] (NULL: snt).  One member with zero strides is the single fit.
static int loo_ard_pass_members(sigp_handle* h, hipStream_t st, int nb, int kernel_id, const double* U, long sU, long n, long d, long dp, long n_pad, LooArdVecs w,
                                LooArdStrides ls, const double* M, double* partial, double* gdev, double snt, const double* sn_m, double* grad) {
  const long ntiles = kbuild_tiles(n_pad);
  const ArdMemberStrides ms{sU, ls.P, ls.w, 0, ls.partial, ls.w, ls.w};
  int rc;
  {
    ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 36)), nb * (4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp)));
    if ((rc = ard_tile_pass_members<ARD_W_LOO>(h, st, nb, U, n, d, dp, n_pad, ms, kernel_id, M, n_pad, w.a(), nullptr, w.v(), w.eps(), partial))) return rc;
    hipLaunchKernelGGL(loo_ard_finish_kernel, dim3((unsigned)(d + 1), (unsigned)nb), dim3(256), 0, st, (const double*)partial, ntiles, (int)dp, (int)d, (int)n,
                       M, n_pad, w, snt, gdev, ls, sn_m);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(grad, gdev, (size_t)nb * (d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  return SIGP_OK;
}

static int loo_ard_pass(sigp_handle* h, hipStream_t st, int kernel_id, LooArdVecs w, ScoreArdParts ap, double snt, double* grad) {
  return loo_ard_pass_members(h, st, 1, kernel_id, h->X, 0, h->n, h->d, h->dp, h->n_pad, w, LooArdStrides{0, 0, 0, 0, 0}, h->gU, ap.partial(), ap.grad(), snt, nullptr, grad);
}

int sigp_loo_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int sigma_mode, int criterion, double* mean, double* var, double* score,
                      double* grad) {
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: bad argument (theta [d + 1], score [2] required)");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: mean and var come together (both NULL: scores and gradient only)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  int rc;
  if ((rc = ard_check_engine(h, "loo_grad_ard", kernel_id))) return rc;
  if (h->n < 2) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: leave-one-out needs n >= 2 training points");
  if ((rc = ard_check_theta(h, "loo_grad_ard", ntheta))) return rc;
  double snt, out[4];
  rc = ard_theta_fit(h, kernel_id, theta, &snt, out);
  if (rc == SIGP_NOT_SPD) return ard_all_inf(h, score, grad, mean, var);
  if (rc) return rc;

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, ld = n_pad;
  if ((rc = ard_scores_ensure(h, grad != nullptr))) return rc;
  const ScoreArdParts ap{h->gPart, n_pad, kbuild_tiles(n_pad), h->dp};   // the scores as sigp_loo has them; then the tile pass's partials and the gradient
  const ScoreParts sp = ap.scores();
  const LooArdVecs w{h->gV, n_pad};
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = loo_launch(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, h->y, 0, nullptr, sp.q(), 0, sigma_mode, sp))) return rc;
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  if (!grad) return sync_slot(h, s);

  if ((rc = kinv_lower(h, st, 1, n_pad))) return rc;
  {   // a = U z;  P -> full;  beta, gamma, eps;  v = P beta and P Gamma
    ProfScope ps(h, st, SIGP_KC_MLII, 4.0 * n_pad * n_pad, 36.0 * n_pad * n_pad);
    if ((rc = alpha_from_U(h, st, 1, s.mat + n_pad * ld, 0, w.a(), 0, n_pad))) return rc;
    if ((rc = mirror_P(h, st, 1, n_pad))) return rc;
    hipLaunchKernelGGL(loo_ard_coef_kernel, dim3(1), dim3(256), 0, st, (const double*)h->gK, ld, (int)n, (int)n_pad, (const double*)sp.q(), sigma_mode, criterion, w);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_ard_scale_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, st, (const double*)h->gK, h->gD, ld, (int)n, (int)n_pad, w);
    HIPCHK(h, hipGetLastError());
  }
  {   // M = (P Gamma) P^T: tile (bi, bj), bi >= bj, = rows bi of P Gamma against rows bj of P (= its columns), the whole K span
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * n_pad * (n_pad + NB), 0.0);
    if ((rc = syrk_set(h, st, 1, h->gD, h->gK, h->gU, n_pad, 1, 0))) return rc;
  }
  if ((rc = loo_ard_pass(h, st, kernel_id, w, ap, snt, grad))) return rc;
  return sync_slot(h, s);
}
