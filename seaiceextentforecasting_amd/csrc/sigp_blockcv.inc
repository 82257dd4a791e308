// sigp_cv, sigp_cv_batch: leave-block-out cross-validation (K-fold / h-block / hv-block folds of consecutive rows) from one factorisation.
// Included inside extern "C" of sigp.hip, after sigp_scores.inc (the shared steps) and sigp_loograd.inc.  Kernels and the closed form: blockcv.hpp.
//
//   U = L~^-T                      inv_factor, as sigp_loo (n^3/3)
//   per fold f, window S_f:        P_SS = U_S U_S^T  (2 |S|^2 (n - min S) flops, split over K slices), a_S = U_S z;
//                                  P_SS = M M^T and X = M^-1 by the factorisation's own diagonal-block kernel; the closing solves
//   score                          loo_sum_kernel over the n terms
//
// Only reads the factor, the ride rows and the fit's state.  Folds are worked off in passes of at most CV_PASS_BLOCKS (member, fold) pairs,
// which bounds the workspaces whatever n / block is (CvWork, score_layout.hpp).

constexpr long CV_PASS_BLOCKS = 1024;

static const char* cv_check_folds(long n, int64_t block, int64_t gap, int64_t maxw) {
  if (block < 1 || gap < 0) return "block >= 1 and gap >= 0 required";
  if (block > maxw || gap > maxw || block + 2 * gap > maxw) return "the window block + 2 gap exceeds the widest one supported";
  const long F = (n + block - 1) / block;
  for (long f = 0; f < F; ++f) {
    int r0, r1, c0, c1;
    cv_window((int)n, (int)block, (int)gap, (int)f, r0, r1, c0, c1);
    if (n - (r1 - r0) < 1) return "a fold leaves no training row (its window covers the whole data set)";
  }
  return nullptr;
}

// K slices of the strip product: 0 (auto) = enough to give every CU two workgroups from ONE member's folds (at most 32), at most one per
// stage of the longest strip.  The count does not depend on the lockstep group, so a member of a group adds its slices in the order its
// single fit does: the same bits from sigp_cv and sigp_cv_batch.
static int cv_slices(const sigp_handle* h, long folds, long n) {
  const long nch = (n + CV_KC - 1) / CV_KC;
  long S = h->opt_cv_slices > 0 ? h->opt_cv_slices : std::min<long>(32, (2L * h->ncu + folds - 1) / folds);
  return (int)std::max(1L, std::min(S, nch));
}

// The work buffers of a pass over a group of nb members: FP = blocks / nb folds of each.  The layout depends on nb, so every group lays its own
// view over the arenas ...
static CvWork cv_work(const sigp_handle* h, int nb, long n, long block, long gap) {
  const long F = (n + block - 1) / block;
  const long FP = std::max<long>(1, std::min<long>(F, CV_PASS_BLOCKS / nb));
  return CvWork{h->cvPart, h->cvBlk, h->cvVec, FP * nb, cv_slices(h, std::min<long>(F, CV_PASS_BLOCKS), n), round_up(std::min<long>(n, block + 2 * gap), 16)};
}

// ... which the entry grows for the groups it will run: of G members and, with tail > 0, a last one of `tail`
static int cv_work_ensure(sigp_handle* h, long n, long block, long gap, int G, int tail) {
  int rc;
  for (int nb : {G, tail}) {
    if (nb < 1) continue;
    const CvWork w = cv_work(h, nb, n, block, gap);
    if ((rc = ensure(h, &h->cvPart, &h->cap_cvPart, CvWork::part_size(w.blocks, w.S, w.wp)))) return rc;
    if ((rc = ensure(h, &h->cvBlk, &h->cap_cvBlk, CvWork::blk_size(w.blocks)))) return rc;
    if ((rc = ensure(h, &h->cvVec, &h->cap_cvVec, CvWork::vec_size(w.blocks)))) return rc;
  }
  return SIGP_OK;
}

// the launcher the single and the lockstep entry points share (arguments as loo_launch; cw = cv_work of this nb); results in sp as loo_launch leaves them.
// adj (sigp_cv_grad_ard, sigp_cv_grad_ard_batch; cvard.hpp): after every pass's closing solves, the fold adjoints of that pass and their
// assembly into every member's adj->band / adj->beta -- Xb and av are overwritten by the next pass.  With adj = nullptr the launches are
// those of sigp_cv.
static int cv_launch(sigp_handle* h, hipStream_t st, int nb, long n, long n_pad, const double* Lm, long sL, const double* dinvp, long sD,
                     const double* y, long sY, const KParams* kps, const double* q, long sQ, int mode, ScoreParts sp, CvWork cw, int block, int gap,
                     const CvAdjoint* adj = nullptr) {
  const long ld = n_pad;
  const long F = (n + block - 1) / block;
  const int wmax = (int)std::min<long>(n, (long)block + 2L * gap), wp = (int)cw.wp;
  const long FP = cw.blocks / nb;
  const int S = (int)cw.S;
  h->cv_slices_used = S;
  int rc;
  double *part = cw.part(), *apart = cw.apart(), *Pb = cw.Pb(), *Xb = cw.Xb(), *av = cw.av();
  int* info = cw.info();
  if ((rc = inv_factor(h, st, nb, Lm, sL, dinvp, sD, n_pad))) return rc;
  static AttrOnce d_attr;
  HIPCHK(h, d_attr.set(h->device, (const void*)potrf_diag_kernel<double>, DIAG_LDS_BYTES));
  const double* z = Lm + n_pad * ld;
  for (long f0 = 0; f0 < F; f0 += FP) {
    const unsigned nf = (unsigned)std::min<long>(FP, F - f0);
    const double wf = (double)nb * nf;
    {
      ProfScope ps(h, st, SIGP_KC_MLII, wf * 2.0 * wmax * wmax * (n - 0.5 * (2 * f0 + nf) * block), wf * 8.0 * wmax * n);
      hipLaunchKernelGGL(cv_strip_partial_kernel, dim3(nf, (unsigned)S, (unsigned)nb), dim3((unsigned)cv_strip_threads(wp)), 0, st, (const double*)h->gU, ld,
                         n_pad * n_pad, z, sL, (int)n, block, gap, (int)f0, wp, part, apart);
      HIPCHK(h, hipGetLastError());
    }
    {
      ProfScope ps(h, st, SIGP_KC_MLII, wf * S * wmax * wmax, wf * 8.0 * (CV_MAXW * CV_MAXW + (double)S * wmax * wmax));
      hipLaunchKernelGGL(cv_strip_finish_kernel, dim3(nf, (unsigned)nb), dim3(256), 0, st, (const double*)part, (const double*)apart, S, wp, (int)n, block, gap,
                         (int)f0, Pb, av, info);
      HIPCHK(h, hipGetLastError());
    }
    {
      ProfScope ps(h, st, SIGP_KC_MLII, wf * 2.0 * NB * NB * NB / 3, wf * 3.0 * NB * NB * 8);
      hipLaunchKernelGGL(potrf_diag_kernel<double>, dim3(nf * (unsigned)nb), dim3(DIAG_THREADS), DIAG_LDS_BYTES, st, Pb, (long)CV_MAXW, Xb, info, 0,
                         h->opt_diag_prio ? 0 : 32, (long)CV_MAXW * CV_MAXW, (long)CV_MAXW * CV_MAXW);
      HIPCHK(h, hipGetLastError());
    }
    {
      ProfScope ps(h, st, SIGP_KC_MLII, wf * 2.0 * wmax * wmax, wf * 8.0 * wmax * wmax);
      hipLaunchKernelGGL(cv_close_kernel, dim3(nf, (unsigned)nb), dim3(256), 0, st, (const double*)Xb, (const double*)av, (const int*)info, y, sY, kps, q, sQ, mode,
                         (int)n, block, gap, (int)f0, sp.base, n_pad, sp.mstride());
      HIPCHK(h, hipGetLastError());
    }
    if (adj) {
      const int mp = (int)round_up(std::min<long>(n, block), 16);
      const int lds = wp * mp * (int)sizeof(double);
      {
        ProfScope ps(h, st, SIGP_KC_MLII, wf * (2.0 * wmax * wmax * mp + (adj->crit == 0 ? 1.0 * wmax * wmax * mp : 0.0) + 4.0 * wmax * wmax), wf * 8.0 * (1.5 * wmax * wmax + wmax));
        static AttrOnce a_attr;
        HIPCHK(h, a_attr.set(h->device, (const void*)cv_adj_fold_kernel, CV_MAXW * CV_MAXW * (int)sizeof(double)));
        hipLaunchKernelGGL(cv_adj_fold_kernel, dim3(nf, (unsigned)nb), dim3(256), (size_t)lds, st, (const double*)Xb, (const double*)av, q, mode, adj->crit, (int)n, block, gap,
                           (int)f0, wp, mp, adj->Bf, adj->betaf, adj->epsf, sQ, adj->sEps);
        HIPCHK(h, hipGetLastError());
      }
      {
        int r0, r1, c0, c1, rl0, rl1;
        cv_window((int)n, block, gap, (int)f0, r0, r1, c0, c1);
        cv_window((int)n, block, gap, (int)(f0 + nf - 1), rl0, rl1, c0, c1);
        // 2 gap / block + 1 terms per entry; the division last, so that the figures of nb members are nb times one member's where it is exact
        const double ent = (double)nb * (rl1 - r0) * CVA_BAND;
        ProfScope ps(h, st, SIGP_KC_MLII, ent * (2.0 * gap + block) / block, ent * 8.0 * (2.0 * gap + 3.0 * block) / block);
        hipLaunchKernelGGL(cv_adj_gather_kernel, dim3((unsigned)(rl1 - r0), (unsigned)nb), dim3(128), 0, st, (const double*)adj->Bf, (const double*)adj->betaf, wp, (int)n, block, gap,
                           (int)F, (int)f0, (int)nf, r0, adj->band, adj->beta, adj->sBand, adj->sBeta);
        HIPCHK(h, hipGetLastError());
      }
    }
  }
  hipLaunchKernelGGL(loo_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)sp.base, n_pad, sp.mstride(), (int)n, sp.sums());
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

int sigp_cv(sigp_handle* h, int64_t block, int64_t gap, int sigma_mode, double* mean, double* var, double* score) {
  if (!h || !mean || !var || !score) return fail(h, SIGP_BAD_ARG, "cv: bad argument (mean [n], var [n], score [2] required)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "cv: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "cv: fp64 engine only (the fp32 engine keeps the inverses of its 2048-column diagonal blocks, not L~^-T)");
  if (!h->fitted) return fail(h, SIGP_BAD_ARG, "cv: call sigp_fit / sigp_fit_predict first (a sharded fit leaves no single-GPU factor: sigp_cv does not apply)");
  if (h->n < 2) return fail(h, SIGP_BAD_ARG, "cv: cross-validation needs n >= 2 training points");
  if (const char* why = cv_check_folds(h->n, block, gap, SIGP_CV_MAX_WINDOW))
    return fail(h, SIGP_BAD_ARG, "cv: %s (block = %lld, gap = %lld, n = %ld, SIGP_CV_MAX_WINDOW = %d)", why, (long long)block, (long long)gap, h->n, SIGP_CV_MAX_WINDOW);
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad;
  int rc;
  if ((rc = scores_ensure(h, 1, n_pad, ScoreParts::size(1, n_pad)))) return rc;
  if ((rc = cv_work_ensure(h, n, block, gap, 1, 0))) return rc;
  const ScoreParts sp{h->gPart, 1, n_pad};
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = cv_launch(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, h->y, 0, nullptr, sp.q(), 0, sigma_mode, sp, cv_work(h, 1, n, block, gap), (int)block, (int)gap))) return rc;
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  return sync_slot(h, s);
}

int sigp_cv_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde, int64_t block, int64_t gap,
                  int sigma_mode, double* mean, double* var, int64_t nstride, double* score) {
  if (!h || h->b_count == 0 || first < 0 || count < 1 || !ell || !sn_tilde || !score) return fail(h, SIGP_BAD_ARG, "cv_batch: bad argument (sigp_batch_upload first)");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "cv_batch: fp64 engine only");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "cv_batch: RBF / MATERN52 only (the reference kernel's batch is sigp_small_run_cv)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "cv_batch: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "cv_batch: mean and var come together (both NULL: scores only)");
  if (mean && nstride < h->b_n) return fail(h, SIGP_BAD_ARG, "cv_batch: mean / var [count][nstride >= %ld] required", h->b_n);
  if (h->b_n < 2) return fail(h, SIGP_BAD_ARG, "cv_batch: cross-validation needs n >= 2 training points");
  if (const char* why = cv_check_folds(h->b_n, block, gap, SIGP_CV_MAX_WINDOW))
    return fail(h, SIGP_BAD_ARG, "cv_batch: %s (block = %lld, gap = %lld, n = %ld, SIGP_CV_MAX_WINDOW = %d)", why, (long long)block, (long long)gap, h->b_n, SIGP_CV_MAX_WINDOW);
  int rc;
  if ((rc = batch_check_params(h, "cv_batch", count, ell, sn_tilde))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const long n = h->b_n, n_pad = h->b_npad;
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  if ((rc = scores_ensure(h, G, n_pad, ScoreParts::size(G, n_pad)))) return rc;
  if ((rc = cv_work_ensure(h, n, block, gap, G, (int)(count % G)))) return rc;
  const ScoreParts sp{h->gPart, G, n_pad};
  std::vector<double> mv(mean ? (size_t)G * 2 * n_pad : 0), sc((size_t)G * 2);
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    if ((rc = batch_group_fit(h, s, nb, kernel_id, ell + g0, sn_tilde + g0, first + g0))) return rc;
    if ((rc = cv_launch(h, st, nb, n, n_pad, s.mat, s.matStride, s.dinv, s.dinvStride, h->by, n_pad, s.kps, s.res, 512, sigma_mode, sp, cv_work(h, nb, n, block, gap), (int)block, (int)gap))) return rc;
    if ((rc = batch_scores_fetch(h, st, nb, sp, mean ? mv.data() : nullptr, sc.data()))) return rc;
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      // a member whose K~ is not SPD, or one of whose P_SS failed its pivot test (+inf terms in its sums): +inf scores, NaN rows
      const bool ok = s.info_host[b] == 0 && std::isfinite(sc[(size_t)2 * b]) && std::isfinite(sc[(size_t)2 * b + 1]);
      batch_scores_scatter(g0 + b, ok, &sc[(size_t)2 * b], mean ? &mv[(size_t)b * 2 * n_pad] : nullptr, n, n_pad, mean, var, nstride, score);
    }
  }
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}
