// sigp_hindcast_grad_ard_batch: the expanding-window hindcast scores AND the exact derivatives of one of them with respect to
// (log l_1 .. log l_d, log sn~) for lockstep groups of fits on the data sets resident after sigp_batch_upload (include/sigp.h):
// sigp_nlml_grad_ard_batch's staging and group fit, sigp_hindcast_batch's scores, and sigp_hindcast_grad_ard's gradient with the member on a
// grid axis (hindcast.hpp).  Included inside extern "C" of sigp.hip, after sigp_cvardbatch.inc (ard_member_params) and sigp_hindcast.inc.
//
// Per group of nb members, on slot 0:
//   staging              ard_stage_group: every member's scaled features, ride rows and y ("data set b" of the staging area), sn~ in ArdStage::sn
//   fit                  batch_group_fit_on at ell = 1 on the staging pointers, no ride points
//   scores               hindcast_launch with nb members (q = y^T A~ in the slot's result rows); r and w stay in the vectors for a gradient
// and for a gradient, every step for all members at once (hindcast_adjoint):
//   rho, ks, suf, zbar   hindcast_coef_kernel (one block per member), hindcast_zbar_kernel
//   Cb into gD           hindcast_band_kernel;  U = L~^-T into gU: inv_factor
//   W = U C into gK      hindcast_w_lds_kernel: the row piece of U in LDS, every global access 256 doubles wide -- hindcast_w_kernel's strided
//                        scans cost the single fit as much as the cubic product behind them, and a group would pay that nb times beside
//                        full-chip launches.  Beyond HINDCAST_W_LDS_MAX_NPAD (score_layout.hpp): hindcast_w_kernel (the debug library
//                        also takes it with the option hindcast_w_lds = 0).  One row body serves both kernels: the same bits either way.
//   G = U W^T            syrk_set on the lower tile space into gD, which is dead by then (n^3/3 per member)
//   the ARD pass         loo_ard_pass_members over M = G with every member's a = v = 0 and eps = 0, ONE copy of the group's gradients
// then batch_scores_fetch, sync_slot, batch_scores_scatter.  A member whose exp(theta) is not finite and positive rides along at harmless
// parameters (ard_member_params); it and a member whose K~ is not SPD get +inf in both scores and every gradient entry and what
// batch_scores_scatter leaves a failed member in mean / var.  Members share no memory: their group mates keep their bits.
// Memory beside the slot: the staging area, HindcastArdGroupVecs and ScoreParts; a gradient adds gU, gK, gD [G][n_pad][n_pad], the centred
// features and LooArdGroupParts (score_layout.hpp).  Profile classes: the staging SIGP_KC_KBUILD, the rest SIGP_KC_MLII
// (sigp_hindcast_grad_ard's entries, their figures times nb).
// Out of scope: sigp_small_*, the reference kernel's gradient, the fp32 engine, sharded fits.

int sigp_hindcast_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta, int64_t lead,
                                 int64_t min_train, int sigma_mode, int criterion, double* mean, double* var, int64_t nstride, double* score, double* grad, int64_t ldgrad) {
  const char* what = "hindcast_grad_ard_batch";
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "%s: bad argument (theta [count][ldtheta], score [count][2] required)", what);
  int rc;
  if ((rc = ard_batch_check(h, what, first, count, kernel_id))) return rc;
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "%s: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE", what);
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "%s: mean and var come together (both NULL: scores and gradients only)", what);
  if (mean && nstride < h->b_n) return fail(h, SIGP_BAD_ARG, "%s: mean / var [count][nstride >= %ld] required", what, h->b_n);
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, n_pad = h->b_npad;
  if ((rc = hindcast_check(h, what, n, lead, min_train, sigma_mode, SIGP_HINDCAST_MAX_LEAD))) return rc;
  if (ntheta != d + 1) return fail(h, SIGP_BAD_ARG, "%s: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", what, d + 1, (long long)ntheta);
  if (ldtheta < ntheta) return fail(h, SIGP_BAD_ARG, "%s: ldtheta = %lld below ntheta = %lld", what, (long long)ldtheta, (long long)ntheta);
  if (grad && ldgrad < d + 1) return fail(h, SIGP_BAD_ARG, "%s: ldgrad = %lld below d + 1 = %ld", what, (long long)ldgrad, d + 1);
  HIPCHK(h, hipSetDevice(h->device));
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  const long ntiles = kbuild_tiles(n_pad);
  const double inf = std::numeric_limits<double>::infinity();
  Slot& s = h->slots[0];
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  hipStream_t st = s.s_upd;
  h->nslots = std::max(h->nslots, 1);
  ArdStage a;
  if ((rc = ard_stage_ensure(h, s, &a))) return rc;
  if ((rc = ensure(h, &h->gV, &h->cap_gV, HindcastArdGroupVecs::size(G, n_pad)))) return rc;
  if (grad) {
    if ((rc = scores_ensure(h, G, n_pad, LooArdGroupParts::size(G, n_pad, ntiles, dp, d + 1)))) return rc;
    if ((rc = scores_grad_ensure(h, G, n_pad, 0))) return rc;
    if ((rc = scores_mlii_ensure(h, 0, G, n_pad, dp))) return rc;
  } else if ((rc = ensure(h, &h->gPart, &h->cap_gPart, ScoreParts::size(G, n_pad)))) return rc;
  const LooArdGroupParts gp{h->gPart, G, n_pad, ntiles, dp, d + 1};   // (without a gradient only its ScoreParts are there, and only they are used)
  const ScoreParts sp = gp.scores();
  const ArdParts ap = gp.ard();
  const HindcastArdGroupVecs gv{h->gV, n_pad, G};
  const HindcastVecs hv = gv.member(0).hc();
  const LooArdVecs w = gv.member(0).ard();
  const LooArdStrides ls{n_pad * n_pad, 512, gv.mstride(), ap.mstride(), d + 1};
  // (the option is a measurement switch the product library refuses: there the choice is by n_pad alone)
  const bool w_lds = hindcast_w_use_lds(n_pad) && h->opt_hindcast_w_lds != 0;
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
    if ((rc = hindcast_launch(h, st, nb, n, n_pad, s.mat, s.matStride, a.y, n_pad, s.kps, s.res, 512, lead, min_train, sigma_mode, sp, hv, gv.mstride(), grad ? 1 : 0))) return rc;
    if (grad) {
      if ((rc = hindcast_adjoint(h, st, nb, n, n_pad, s.mat, s.matStride, s.dinv, s.dinvStride, lead, min_train, sigma_mode, criterion, s.res, 512, hv, gv.mstride(), w_lds)))
        return rc;
      // every member's a = v = 0, eps = 0: the adjoint is G alone
      HIPCHK(h, hipMemset2DAsync(w.base, (size_t)gv.mstride() * sizeof(double), 0, (size_t)LooArdVecs::size(n_pad) * sizeof(double), (size_t)nb, st));
      if ((rc = loo_ard_pass_members(h, st, nb, kernel_id, a.X, n_pad * dp, n, d, dp, n_pad, w, ls, h->gD, ap.partial(), ap.grad(), 0.0, a.sn, gh.data()))) return rc;
    }
    if ((rc = batch_scores_fetch(h, st, nb, sp, mean ? mv.data() : nullptr, sc.data()))) return rc;
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const long i = g0 + b;
      const bool good = ok[(size_t)b] && s.info_host[b] == 0;
      batch_scores_scatter(i, good, &sc[(size_t)2 * b], mean ? &mv[(size_t)b * 2 * n_pad] : nullptr, n, n_pad, mean, var, nstride, score);
      if (!grad) continue;
      for (long k = 0; k <= d; ++k) grad[i * ldgrad + k] = good ? gh[(size_t)(b * (d + 1) + k)] : inf;
    }
  }
  h->built = h->factored = h->fitted = false;               // slot 0 no longer holds the single-fit state
  return SIGP_OK;
}
