// sigp_hindcast, sigp_hindcast_batch, sigp_hindcast_grad_ard: expanding-window hindcast validation from one fit, and the exact per-feature
// gradient of its scores (hindcast.hpp has the formulae and the kernels; sigp_hindcastbatch.inc the gradient for lockstep groups).  Included inside extern "C" of sigp.hip, after sigp_scores.inc
// and sigp_looard.inc.
//
// The values read the factor, the solved ride row z and q = z.z alone: a scan of z^2, the row pass, loo_sum_kernel.  No L~^-T.
// The gradient, on top of them:
//   rho, kappa sigma, suf     hindcast_coef_kernel (one block, fixed-order scan);  zbar: hindcast_zbar_kernel
//   Cb                        the banded part of the adjoint C with respect to L^-1 K~ L^-T into gD (hindcast_band_kernel: n^2 stores, n lead^2 flops)
//   U = L~^-T                 inv_factor into gU (n^3/3; its products park in gK)
//   W = U C                   into gK, a sibling of cv_band_product_kernel written for this operand (hindcast_w_kernel: one block per row of U,
//                             a prefix and a suffix scan for the rank-one part of C, at most 2 lead - 1 terms per entry for the banded part:
//                             cv_band_product_kernel takes a full left operand and a 384-column band store, neither of which fits U and lead <= 128)
//   G = U W^T                 lower 128-tiles into gD, which is dead by then: syrk_set on the lower tile space, K from the row block on
//                             (U is upper triangular; G is symmetric, so U W^T stands for W U^T): n^3/3 -- the one cubic step beyond U
//   the ARD pass              the tile pass with ARD_W_LOO over M = G with a = v = 0, eps = 0, then loo_ard_finish_kernel
// Memory: sigp_loo_grad's single-fit buffers (gU, gK, gD, gV, gPart) plus ardXc.  Profile class: SIGP_KC_MLII, one entry per step.
// Lockstep groups: sigp_hindcast_grad_ard_batch (sigp_hindcastbatch.inc), which runs these launches with a member axis and W = U C on
// hindcast_w_lds_kernel.  Out of scope: sigp_small_*, the reference kernel's gradient, the fp32 engine, sharded fits.

// the value pass for nb lockstep members: cum, the rows, the sums.  rw = 1: r and w stay in hv for the gradient.
static int hindcast_launch(sigp_handle* h, hipStream_t st, int nb, long n, long n_pad, const double* Lm, long sL, const double* y, long sY, const KParams* kps,
                           const double* q, long sQ, long lead, long min_train, int mode, ScoreParts sp, HindcastVecs hv, long sV, int rw) {
  const long ld = n_pad;
  const HindcastStrides ms{sL, sQ, sV, 0};
  {
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 2.0 * n, nb * 16.0 * n);
    hipLaunchKernelGGL(hindcast_scan_kernel, dim3((unsigned)nb), dim3(256), 0, st, Lm + n_pad * ld, (int)n, hv, ms);
    HIPCHK(h, hipGetLastError());
  }
  {
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 4.0 * n * lead, nb * 16.0 * n * lead);
    hipLaunchKernelGGL(hindcast_rows_kernel, dim3((unsigned)((n + 3) / 4), (unsigned)nb), dim3(256), 0, st, Lm, ld, (int)n, Lm + n_pad * ld, y, q, (int)lead, (int)min_train,
                       mode, sp.base, n_pad, hv, rw, ms, sY, sp.mstride(), kps);
    HIPCHK(h, hipGetLastError());
  }
  hipLaunchKernelGGL(loo_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)sp.base, n_pad, sp.mstride(), (int)n, sp.sums());
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// the checks on (lead, min_train, sigma_mode) the entries share; n = the number of training rows
static int hindcast_check(sigp_handle* h, const char* what, long n, int64_t lead, int64_t min_train, int sigma_mode, int64_t max_lead) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "%s: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED", what);
  if (lead < 1 || lead > max_lead) return fail(h, SIGP_BAD_ARG, "%s: 1 <= lead <= %lld required (got %lld)", what, (long long)max_lead, (long long)lead);
  if (min_train < 1) return fail(h, SIGP_BAD_ARG, "%s: min_train >= 1 required (got %lld)", what, (long long)min_train);
  if (min_train > n || min_train + lead - 1 > n - 1) return fail(h, SIGP_BAD_ARG, "%s: no row is scored (min_train + lead - 1 = %lld > n - 1 = %ld)", what, (long long)(min_train + lead - 1), n - 1);
  return SIGP_OK;
}

int sigp_hindcast(sigp_handle* h, int64_t lead, int64_t min_train, int sigma_mode, double* mean, double* var, double* score) {
  if (!h || !mean || !var || !score) return fail(h, SIGP_BAD_ARG, "hindcast: bad argument (mean [n], var [n], score [2] required)");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "hindcast: fp64 engine only");
  if (!h->fitted) return fail(h, SIGP_BAD_ARG, "hindcast: call sigp_fit / sigp_fit_predict first (a sharded fit leaves no single-GPU factor: sigp_hindcast does not apply)");
  int rc;
  if ((rc = hindcast_check(h, "hindcast", h->n, lead, min_train, sigma_mode, SIGP_HINDCAST_MAX_LEAD))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad;
  if ((rc = ensure(h, &h->gPart, &h->cap_gPart, ScoreParts::size(1, n_pad)))) return rc;
  if ((rc = ensure(h, &h->gV, &h->cap_gV, HindcastVecs::size(n_pad)))) return rc;
  const ScoreParts sp{h->gPart, 1, n_pad};
  const HindcastVecs hv{h->gV, n_pad};
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = hindcast_launch(h, st, 1, n, n_pad, s.mat, 0, h->y, 0, nullptr, sp.q(), 0, lead, min_train, sigma_mode, sp, hv, 0, 0))) return rc;
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  return sync_slot(h, s);
}

// The same for lockstep groups of RBF / Matern fits on the resident batch data, as sigp_loo_batch: build, blocked Cholesky, epilogue (q stays
// on the device in the slot's result rows), then the value pass with the member on a grid dimension.
int sigp_hindcast_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde, int64_t lead, int64_t min_train,
                        int sigma_mode, double* mean, double* var, int64_t nstride, double* score) {
  if (!h || h->b_count == 0 || first < 0 || count < 1 || !ell || !sn_tilde || !score) return fail(h, SIGP_BAD_ARG, "hindcast_batch: bad argument (sigp_batch_upload first)");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "hindcast_batch: fp64 engine only");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "hindcast_batch: RBF / MATERN52 only");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "hindcast_batch: mean and var come together (both NULL: scores only)");
  if (mean && nstride < h->b_n) return fail(h, SIGP_BAD_ARG, "hindcast_batch: mean / var [count][nstride >= %ld] required", h->b_n);
  int rc;
  if ((rc = hindcast_check(h, "hindcast_batch", h->b_n, lead, min_train, sigma_mode, SIGP_HINDCAST_MAX_LEAD))) return rc;
  if ((rc = batch_check_params(h, "hindcast_batch", count, ell, sn_tilde))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const long n = h->b_n, n_pad = h->b_npad;
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  if ((rc = ensure(h, &h->gPart, &h->cap_gPart, ScoreParts::size(G, n_pad)))) return rc;
  if ((rc = ensure(h, &h->gV, &h->cap_gV, G * HindcastVecs::size(n_pad)))) return rc;
  const ScoreParts sp{h->gPart, G, n_pad};
  const HindcastVecs hv{h->gV, n_pad};
  std::vector<double> mv(mean ? (size_t)G * 2 * n_pad : 0), sc((size_t)G * 2);
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    if ((rc = batch_group_fit(h, s, nb, kernel_id, ell + g0, sn_tilde + g0, first + g0))) return rc;
    if ((rc = hindcast_launch(h, st, nb, n, n_pad, s.mat, s.matStride, h->by, n_pad, s.kps, s.res, 512, lead, min_train, sigma_mode, sp, hv, HindcastVecs::size(n_pad), 0))) return rc;
    if ((rc = batch_scores_fetch(h, st, nb, sp, mean ? mv.data() : nullptr, sc.data()))) return rc;
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b)
      batch_scores_scatter(g0 + b, s.info_host[b] == 0, &sc[(size_t)2 * b], mean ? &mv[(size_t)b * 2 * n_pad] : nullptr, n, n_pad, mean, var, nstride, score);
  }
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}

// The adjoint of the score `criterion` for nb lockstep members, after hindcast_launch with rw = 1 on the same stream: G = d score / d K~,
// lower 128-tiles (whole diagonal tiles), into gD.  gU holds U = L~^-T afterwards, gK W = U C, all three n_pad^2 apart.  Member b's factor
// (and its ride row z) at Lm + b sL, its inverse diagonal blocks at dinvp + b sD, q at q + b sQ, its vectors at b sV behind hv; the single
// fit is one member with zero strides.  w_lds: W = U C by hindcast_w_lds_kernel (lockstep groups with n_pad <= HINDCAST_W_LDS_MAX_NPAD;
// the same bits, hindcast.hpp) instead of hindcast_w_kernel.
// Precondition on inv_factor, shared with kinv_lower: the product G = U W^T starts K at the row block and reads the WHOLE diagonal 128-block
// of U, so trtri_levels must leave zeros left of the diagonal inside the diagonal blocks (blocks below the block diagonal are never read).
// Inside a diagonal tile G_ij = sum_k U_ik W_jk and G_ji = sum_k U_jk W_ik are different sums: the two halves agree to rounding, not bit for
// bit.  The ARD pass reads the strictly lower half and the diagonal only.
static int hindcast_adjoint(sigp_handle* h, hipStream_t st, int nb, long n, long n_pad, const double* Lm, long sL, const double* dinvp, long sD, long lead, long min_train,
                            int mode, int criterion, const double* q, long sQ, HindcastVecs hv, long sV, bool w_lds) {
  const long ld = n_pad;
  const HindcastStrides ms{sL, sQ, sV, n_pad * n_pad};
  const double* z = Lm + n_pad * ld;
  int rc;
  {   // rho, kappa sigma and the suffix sums: one block per member, a fixed-order scan
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 12.0 * n, nb * 48.0 * n);
    hipLaunchKernelGGL(hindcast_coef_kernel, dim3((unsigned)nb), dim3(256), 0, st, (int)n, q, (int)lead, (int)min_train, mode, criterion, hv, ms);
    HIPCHK(h, hipGetLastError());
  }
  {   // zbar
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 2.0 * n * lead, nb * 8.0 * n * lead);
    hipLaunchKernelGGL(hindcast_zbar_kernel, dim3((unsigned)(n_pad / 256 + 1), (unsigned)nb), dim3(256), 0, st, Lm, ld, (int)n, (int)n_pad, z, (int)lead, mode, hv, ms);
    HIPCHK(h, hipGetLastError());
  }
  {   // the banded part of C
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 4.0 * n * lead * lead, nb * (8.0 * n_pad * n_pad + 16.0 * n * lead * lead));
    hipLaunchKernelGGL(hindcast_band_kernel, dim3((unsigned)((n_pad + 255) / 256), (unsigned)n_pad, (unsigned)nb), dim3(256), 0, st, Lm, ld, (int)n, (int)n_pad, z, (int)lead,
                       hv, h->gD, ms);
    HIPCHK(h, hipGetLastError());
  }
  if ((rc = inv_factor(h, st, nb, Lm, sL, dinvp, sD, n_pad))) return rc;
  {   // W = U C: the two scans and the banded product
    ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n * n * (2.0 * lead + 3.0)), nb * (8.0 * n * n * (lead + 2.0)));
    if (w_lds) {
      static AttrOnce attr;
      HIPCHK(h, attr.set(h->device, (const void*)hindcast_w_lds_kernel, (int)hindcast_w_lds_bytes(HINDCAST_W_LDS_MAX_NPAD)));
      hipLaunchKernelGGL(hindcast_w_lds_kernel, dim3((unsigned)n_pad, (unsigned)nb), dim3(256), (size_t)hindcast_w_lds_bytes(n_pad), st, (const double*)h->gU,
                         (const double*)h->gD, ld, (int)n, (int)n_pad, z, (int)lead, hv, h->gK, ms);
    } else {
      hipLaunchKernelGGL(hindcast_w_kernel, dim3((unsigned)n_pad, (unsigned)nb), dim3(256), 0, st, (const double*)h->gU, (const double*)h->gD, ld, (int)n, (int)n_pad, z,
                         (int)lead, hv, h->gK, ms);
    }
    HIPCHK(h, hipGetLastError());
  }
  {   // G = U W^T
    ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n_pad * n_pad * n_pad / 3), 0.0);
    if ((rc = syrk_set(h, st, nb, h->gU, h->gK, h->gD, n_pad, 1, 1))) return rc;
  }
  return SIGP_OK;
}

int sigp_hindcast_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int64_t lead, int64_t min_train, int sigma_mode, int criterion,
                           double* mean, double* var, double* score, double* grad) {
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "hindcast_grad_ard: bad argument (theta [d + 1], score [2] required)");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "hindcast_grad_ard: mean and var come together (both NULL: scores and gradient only)");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "hindcast_grad_ard: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  int rc;
  if ((rc = ard_check_engine(h, "hindcast_grad_ard", kernel_id))) return rc;
  if ((rc = hindcast_check(h, "hindcast_grad_ard", h->n, lead, min_train, sigma_mode, SIGP_HINDCAST_MAX_LEAD))) return rc;
  if ((rc = ard_check_theta(h, "hindcast_grad_ard", ntheta))) return rc;
  double snt, out[4];
  rc = ard_theta_fit(h, kernel_id, theta, &snt, out);
  if (rc == SIGP_NOT_SPD) return ard_all_inf(h, score, grad, mean, var);
  if (rc) return rc;

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad;
  // the vectors first: ard_scores_ensure asks gV for less and must find it grown
  if ((rc = ensure(h, &h->gV, &h->cap_gV, grad ? HindcastArdVecs::size(n_pad) : HindcastVecs::size(n_pad)))) return rc;
  if (grad) {
    if ((rc = ard_scores_ensure(h, true))) return rc;
  } else if ((rc = ensure(h, &h->gPart, &h->cap_gPart, ScoreParts::size(1, n_pad)))) return rc;
  const ScoreArdParts ap{h->gPart, n_pad, kbuild_tiles(n_pad), h->dp};   // the scores as sigp_hindcast has them; then the tile pass's partials and the gradient
  const ScoreParts sp = ap.scores();
  const HindcastArdVecs av{h->gV, n_pad};
  const HindcastVecs hv = av.hc();
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = hindcast_launch(h, st, 1, n, n_pad, s.mat, 0, h->y, 0, nullptr, sp.q(), 0, lead, min_train, sigma_mode, sp, hv, 0, grad ? 1 : 0))) return rc;
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  if (!grad) return sync_slot(h, s);

  if ((rc = hindcast_adjoint(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, lead, min_train, sigma_mode, criterion, sp.q(), 0, hv, 0, false))) return rc;
  const LooArdVecs w = av.ard();
  HIPCHK(h, hipMemsetAsync(w.base, 0, (size_t)LooArdVecs::size(n_pad) * sizeof(double), st));   // a = v = 0, eps = 0: the adjoint is G alone
  {
    const long d = h->d, dp = h->dp, ntiles = kbuild_tiles(n_pad);
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 36), 4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp));
    if ((rc = ard_tile_pass<ARD_W_LOO>(h, st, kernel_id, h->gD, n_pad, w.a(), nullptr, w.v(), w.eps(), ap.partial()))) return rc;
    hipLaunchKernelGGL(loo_ard_finish_kernel, dim3((unsigned)(d + 1), 1), dim3(256), 0, st, (const double*)ap.partial(), ntiles, (int)dp, (int)d, (int)n, (const double*)h->gD, n_pad,
                       w, snt, ap.grad(), LooArdStrides{0, 0, 0, 0, 0}, (const double*)nullptr);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(grad, ap.grad(), (size_t)(h->d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  return sync_slot(h, s);
}
