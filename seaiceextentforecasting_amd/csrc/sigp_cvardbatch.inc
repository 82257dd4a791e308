// sigp_cv_grad_ard_batch: the leave-block-out scores AND the exact derivatives of one of them with respect to (log l_1 .. log l_d, log sn~) for
// lockstep groups of fits on the data sets resident after sigp_batch_upload (include/sigp.h) -- and the driver it shares with
// sigp_loo_grad_ard_batch (sigp_looardbatch.inc), ard_score_batch: the two entries differ in the score's launches and in the adjoint's
// coefficients, and in nothing else.  Included inside extern "C" of sigp.hip, after sigp_looardbatch.inc and sigp_cvard.inc.
//
// Per group of nb members, on slot 0:
//   staging              ard_stage_group: every member's scaled features, ride rows and y ("data set b" of the staging area), sn~ in ArdStage::sn
//   fit                  batch_group_fit_on at ell = 1 on the staging pointers, no ride points
//   scores               leave-one-out: loo_launch with nb members, as sigp_loo_grad_batch calls it
//                        leave-block-out: cv_launch with nb members, as sigp_cv_batch calls it (nb x 1024 / nb folds per pass), and for a
//                        gradient with the adjoint: every member's band store and beta zeroed (cv_adj_zero), then per pass the fold adjoints
//                        at the (member, fold) pair index and their assembly (cvard.hpp)
// and for a gradient, every step for all members at once:
//   leave-one-out        P = U U^T (kinv_lower);  a = U z, mirror_P, beta, gamma, eps (loo_ard_coef_kernel), v = P beta and P Gamma into gD
//                        (loo_ard_scale_kernel);  M = (P Gamma) P^T (syrk_set) into gU
//   leave-block-out      cv_ard_products (sigp_cvard.inc): P = U U^T;  a = U z, mirror_P, eps, v = P beta;  P B into gD;  M = (P B) P^T into gU
//   the ARD pass         loo_ard_pass_members: the tile pass on the staged features, the fixed-order sums, ONE copy of the group's gradients
// then batch_scores_fetch, sync_slot, batch_scores_scatter.  A member whose exp(theta) is not finite and positive rides along at harmless
// parameters (the ok[] of sigp_nlml_grad_ard_batch); it, a member whose K~ is not SPD and -- leave-block-out -- a member one of whose folds
// failed its pivot test (+inf in its sums, sigp_cv_batch's test) get +inf in both scores and every gradient entry and what
// batch_scores_scatter leaves a failed member in mean / var.  Members share no memory: their group mates keep their bits.
// Memory beside the slot: gU, gK, gD [G][n_pad][n_pad], the staging area, the centred features, LooArdGroupVecs and LooArdGroupParts; the
// leave-block-out scores add sigp_cv_batch's work buffers and CvAdjGroupStore (score_layout.hpp), grown for the groups of G and the tail.
// Profile classes: the staging SIGP_KC_KBUILD, the rest SIGP_KC_MLII (sigp_loo_grad_ard's / sigp_cv_grad_ard's entries, their figures times nb).
// Out of scope: sigp_small_*, the reference kernel, the fp32 engine, sharded fits.

// A member's parameters from its theta = (log l_1 .. log l_d, log sn~): ell [d] and sn~.  false: an exp(theta) is not finite and positive; the
// member then rides along at harmless parameters (ell = 1, sn~ = 1) and the driver drops its results.
static bool ard_member_params(const double* th, long d, double* ell, double* snt) {
  bool good = true;
  for (long k = 0; k < d; ++k) {
    ell[k] = std::exp(th[k]);
    if (!std::isfinite(ell[k]) || !(ell[k] > 0)) good = false;
  }
  *snt = std::exp(th[d]);
  if (!std::isfinite(*snt)) good = false;
  if (!good) {
    std::fill(ell, ell + d, 1.0);
    *snt = 1.0;
  }
  return good;
}

static int ard_score_batch(sigp_handle* h, const char* what, const CvFolds* cv, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta,
                           int64_t ldtheta, int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad) {
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "%s: bad argument (theta [count][ldtheta], score [count][2] required)", what);
  int rc;
  if ((rc = ard_batch_check(h, what, first, count, kernel_id))) return rc;
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "%s: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED", what);
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "%s: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE", what);
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "%s: mean and var come together (both NULL: scores and gradients only)", what);
  if (mean && nstride < h->b_n) return fail(h, SIGP_BAD_ARG, "%s: mean / var [count][nstride >= %ld] required", what, h->b_n);
  if (h->b_n < 2) return fail(h, SIGP_BAD_ARG, "%s: %s needs n >= 2 training points", what, cv ? "cross-validation" : "leave-one-out");
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, n_pad = h->b_npad, ld = n_pad;
  if (ntheta != d + 1) return fail(h, SIGP_BAD_ARG, "%s: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", what, d + 1, (long long)ntheta);
  if (ldtheta < ntheta) return fail(h, SIGP_BAD_ARG, "%s: ldtheta = %lld below ntheta = %lld", what, (long long)ldtheta, (long long)ntheta);
  if (grad && ldgrad < d + 1) return fail(h, SIGP_BAD_ARG, "%s: ldgrad = %lld below d + 1 = %ld", what, (long long)ldgrad, d + 1);
  if (cv)
    if (const char* why = cv_check_folds(n, cv->block, cv->gap, SIGP_CV_MAX_WINDOW))
      return fail(h, SIGP_BAD_ARG, "%s: %s (block = %lld, gap = %lld, n = %ld, SIGP_CV_MAX_WINDOW = %d)", what, why, (long long)cv->block, (long long)cv->gap, n, SIGP_CV_MAX_WINDOW);
  HIPCHK(h, hipSetDevice(h->device));
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  const long ntiles = kbuild_tiles(n_pad);
  const long block = cv ? (long)cv->block : 1, gap = cv ? (long)cv->gap : 0, F = (n + block - 1) / block;
  const double inf = std::numeric_limits<double>::infinity();
  Slot& s = h->slots[0];
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  hipStream_t st = s.s_upd;
  h->nslots = std::max(h->nslots, 1);
  ArdStage a;
  if ((rc = ard_stage_ensure(h, s, &a))) return rc;
  if ((rc = scores_ensure(h, G, n_pad, grad ? LooArdGroupParts::size(G, n_pad, ntiles, dp, d + 1) : ScoreParts::size(G, n_pad)))) return rc;
  if (grad) {
    if ((rc = scores_grad_ensure(h, G, n_pad, LooArdGroupVecs::size(1, n_pad)))) return rc;
    if ((rc = scores_mlii_ensure(h, 0, G, n_pad, dp))) return rc;
  }
  if (cv) {
    const int tail = (int)(count % G);
    if ((rc = cv_work_ensure(h, n, block, gap, G, tail))) return rc;
    if (grad)
      for (int nb : {G, tail}) {
        if (nb < 1) continue;
        const CvWork cw = cv_work(h, nb, n, block, gap);
        if ((rc = ensure(h, &h->cvAdj, &h->cap_cvAdj, CvAdjGroupStore::size(nb, n_pad, cw.blocks / nb, cw.wp, F)))) return rc;
      }
  }
  const LooArdGroupParts gp{h->gPart, G, n_pad, ntiles, dp, d + 1};   // (without a gradient only its ScoreParts are there, and only they are used)
  const ScoreParts sp = gp.scores();
  const ArdParts ap = gp.ard();
  const LooArdGroupVecs gw{h->gV, n_pad, G};
  const LooArdVecs w = gw.member(0);
  const LooArdStrides ls{n_pad * n_pad, 512, gw.mstride(), ap.mstride(), d + 1};
  std::vector<double> hdiv((size_t)(a.cap * (dp + 1))), one((size_t)G, 1.0), ell((size_t)G * d), snt((size_t)G), gh(grad ? (size_t)G * (d + 1) : 0);
  std::vector<double> mv(mean ? (size_t)G * 2 * n_pad : 0), sc((size_t)G * 2);
  std::vector<int> ds((size_t)G);
  std::vector<char> ok((size_t)G);
  for (int b = 0; b < G; ++b) ds[(size_t)b] = b;             // member b is "data set b" of the staging area
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    for (int b = 0; b < nb; ++b) ok[(size_t)b] = ard_member_params(theta + (g0 + b) * ldtheta, d, &ell[(size_t)(b * d)], &snt[(size_t)b]);
    if ((rc = ard_stage_group(h, st, a, nb, ell.data(), d, snt.data(), first + g0, hdiv))) return rc;
    if ((rc = batch_group_fit_on(h, s, nb, kernel_id, one.data(), snt.data(), ds.data(), a.X, a.y, a.Xs, 0))) return rc;
    CvAdjoint adj{};
    if (cv) {
      const CvWork cw = cv_work(h, nb, n, block, gap);        // this group's views: their layout depends on nb
      if (grad) {
        adj = CvAdjGroupStore{h->cvAdj, nb, n_pad, cw.blocks / nb, cw.wp, F}.adjoint(criterion, w.beta(), gw.mstride());
        if ((rc = cv_adj_zero(h, st, nb, n_pad, adj))) return rc;
      }
      if ((rc = cv_launch(h, st, nb, n, n_pad, s.mat, s.matStride, s.dinv, s.dinvStride, a.y, n_pad, s.kps, s.res, 512, sigma_mode, sp, cw, (int)block, (int)gap,
                          grad ? &adj : nullptr))) return rc;
    } else {
      if ((rc = loo_launch(h, st, nb, n, n_pad, s.mat, s.matStride, s.dinv, s.dinvStride, a.y, n_pad, s.kps, s.res, 512, sigma_mode, sp))) return rc;
    }
    if (grad) {
      if (cv) {
        if ((rc = cv_ard_products(h, st, nb, n, n_pad, F, s.mat + n_pad * ld, s.matStride, adj, w, gw.mstride()))) return rc;
      } else {
        if ((rc = kinv_lower(h, st, nb, n_pad))) return rc;
        {   // a = U z;  P -> full;  beta, gamma, eps;  v = P beta and P Gamma
          ProfScope ps(h, st, SIGP_KC_MLII, nb * 4.0 * n_pad * n_pad, nb * 36.0 * n_pad * n_pad);
          if ((rc = alpha_from_U(h, st, nb, s.mat + n_pad * ld, s.matStride, w.a(), gw.mstride(), n_pad))) return rc;
          if ((rc = mirror_P(h, st, nb, n_pad))) return rc;
          hipLaunchKernelGGL(loo_ard_coef_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)h->gK, ld, (int)n, (int)n_pad, (const double*)s.res, sigma_mode, criterion, w, ls);
          HIPCHK(h, hipGetLastError());
          hipLaunchKernelGGL(loo_ard_scale_kernel, dim3((unsigned)(n_pad / 4), (unsigned)nb), dim3(256), 0, st, (const double*)h->gK, h->gD, ld, (int)n, (int)n_pad, w, ls);
          HIPCHK(h, hipGetLastError());
        }
        {   // M = (P Gamma) P^T, every member's lower tiles in one launch
          ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n_pad * n_pad * (n_pad + NB)), 0.0);
          if ((rc = syrk_set(h, st, nb, h->gD, h->gK, h->gU, n_pad, 1, 0))) return rc;
        }
      }
      if ((rc = loo_ard_pass_members(h, st, nb, kernel_id, a.X, n_pad * dp, n, d, dp, n_pad, w, ls, h->gU, ap.partial(), ap.grad(), 0.0, a.sn, gh.data()))) return rc;
    }
    if ((rc = batch_scores_fetch(h, st, nb, sp, mean ? mv.data() : nullptr, sc.data()))) return rc;
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const long i = g0 + b;
      bool good = ok[(size_t)b] && s.info_host[b] == 0;
      // leave-block-out: a fold whose P_SS failed its pivot test left +inf terms in the member's sums (sigp_cv_batch's test)
      if (cv) good = good && std::isfinite(sc[(size_t)2 * b]) && std::isfinite(sc[(size_t)2 * b + 1]);
      batch_scores_scatter(i, good, &sc[(size_t)2 * b], mean ? &mv[(size_t)b * 2 * n_pad] : nullptr, n, n_pad, mean, var, nstride, score);
      if (!grad) continue;
      for (long k = 0; k <= d; ++k) grad[i * ldgrad + k] = good ? gh[(size_t)(b * (d + 1) + k)] : inf;
    }
  }
  h->built = h->factored = h->fitted = false;               // slot 0 no longer holds the single-fit state
  return SIGP_OK;
}

int sigp_cv_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta, int64_t block, int64_t gap,
                           int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad) {
  const CvFolds cv{block, gap};
  return ard_score_batch(h, "cv_grad_ard_batch", &cv, first, count, kernel_id, theta, ntheta, ldtheta, sigma_mode, criterion, mean, var, nstride, score, grad, ldgrad);
}
