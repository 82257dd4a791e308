// sigp_batch_run_ard, sigp_nlml_grad_ard_batch: per-feature (ARD) length scales in lockstep groups on the data sets resident after
// sigp_batch_upload (include/sigp.h).  Scales belong to a FIT, not to a data set -- fit i uses data set (first + i) % batch, and two members
// of one group may share a data set and differ in scales (several starts per data set) -- so every group stages its members' scaled
// features: ard_stage_kernel (ardgrad.hpp) fills, in one launch, a staging area that is laid out as the resident data are, member b being
// its "data set b": scaled training features [n_pad][dp], scaled ride rows [RIDE][dp] and the member's y [n_pad] (KParams::ds addresses X,
// y and Xs alike).  From there on the group runs batch_group_fit_on's launches at ell = 1 on the staging pointers: no covariance function
// and no existing kernel's arithmetic changes, and the isotropic batch entries issue the launches they issued before.
// The gradient: inv_factor, kinv_lower, alpha_from_U for all members at once (as sigp_nlml_grad_batch), then sigp_nlml_grad_ard's tile pass
// and finish kernel with the member on grid.y -- partials per (member, tile), fixed-order sums, no atomics.
// Both entries run their groups one after another on slot 0, as the score entries do.  Profile classes: the staging SIGP_KC_KBUILD, the
// gradient's work SIGP_KC_MLII.  The leave-one-out scores and their ARD gradients for groups: sigp_looardbatch.inc, on this file's staging.
// The leave-block-out scores and their ARD gradients for groups: sigp_cvardbatch.inc.  Out of scope: sigp_small_*, the fp32 engine, sharded fits.  Included inside
// extern "C" of sigp.hip, after sigp_ardgrad.inc.

// the staging area of slot s (ArdStage, score_layout.hpp), sized for the slot's capacity
static int ard_stage_ensure(sigp_handle* h, const Slot& s, ArdStage* a) {
  const long cap = s.capB, n_pad = h->b_npad, dp = h->b_dp;
  int rc;
  if ((rc = ensure(h, &h->bStage, &h->cap_bStage, ArdStage::size(cap, n_pad, dp)))) return rc;
  *a = ArdStage::at(h->bStage, cap, n_pad, dp);
  return SIGP_OK;
}

// divisors [nb][d] (row stride ldell) and sn~ [nb] of a group up in ONE copy, then the one staging launch; hdiv [cap][dp] + [cap] is the
// caller's host buffer (it outlives the group: the caller synchronises before the next one)
static int ard_stage_group(sigp_handle* h, hipStream_t st, const ArdStage& a, int nb, const double* ell, long ldell, const double* snt, long first_ds,
                           std::vector<double>& hdiv) {
  const long d = h->b_d, dp = h->b_dp, n_pad = h->b_npad;
  std::fill(hdiv.begin(), hdiv.end(), 1.0);
  for (int b = 0; b < nb; ++b) {
    std::copy(ell + b * ldell, ell + b * ldell + d, hdiv.begin() + b * dp);
    hdiv[(size_t)(a.cap * dp + b)] = snt[b];
  }
  HIPCHK(h, hipMemcpyAsync(a.div, hdiv.data(), hdiv.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const long tot = (n_pad + RIDE) * dp + n_pad;
  ProfScope ps(h, st, SIGP_KC_KBUILD, (double)nb * (n_pad + RIDE) * d, 16.0 * nb * tot);
  hipLaunchKernelGGL(ard_stage_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)nb), dim3(256), 0, st, (const double*)h->bX, (const double*)h->bXs, (const double*)h->by,
                     first_ds, h->b_count, (int)n_pad, RIDE, (int)dp, (int)d, (const double*)a.div, a.X, a.Xs, a.y);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

static int ard_batch_check(sigp_handle* h, const char* what, int64_t first, int64_t count, int kernel_id) {
  if (h->b_count == 0) return fail(h, SIGP_BAD_ARG, "%s: call sigp_batch_upload first", what);
  if (first < 0 || count < 1) return fail(h, SIGP_BAD_ARG, "%s: first >= 0 and count >= 1 required", what);
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "%s: fp64 engine only", what);
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "%s: RBF / MATERN52 only", what);
  return SIGP_OK;
}

int sigp_batch_run_ard(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, int64_t ldell, const double* sn_tilde, double* out,
                       double* mean, double* var) {
  if (!h || !ell || !sn_tilde || !out) return fail(h, SIGP_BAD_ARG, "batch_run_ard: bad argument");
  int rc;
  if ((rc = ard_batch_check(h, "batch_run_ard", first, count, kernel_id))) return rc;
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, m = h->b_m, n_pad = h->b_npad;
  if (ldell < d) return fail(h, SIGP_BAD_ARG, "batch_run_ard: ldell = %lld below the %ld features", (long long)ldell, d);
  for (int64_t i = 0; i < count; ++i) {
    for (long k = 0; k < d; ++k)
      if (!(ell[i * ldell + k] > 0) || !std::isfinite(ell[i * ldell + k])) return fail(h, SIGP_BAD_ARG, "batch_run_ard: finite ell > 0 required (fit %lld, feature %ld)", (long long)i, k);
    if (!(sn_tilde[i] >= 0) || !std::isfinite(sn_tilde[i])) return fail(h, SIGP_BAD_ARG, "batch_run_ard: finite sn_tilde >= 0 required");
  }
  HIPCHK(h, hipSetDevice(h->device));
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  Slot& s = h->slots[0];
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  hipStream_t st = s.s_upd;
  h->nslots = std::max(h->nslots, 1);
  ArdStage a;
  if ((rc = ard_stage_ensure(h, s, &a))) return rc;
  std::vector<double> hdiv((size_t)(a.cap * (dp + 1))), one((size_t)G, 1.0), kss((size_t)std::max<long>(m, 1), 1.0);
  std::vector<int> ds((size_t)G);
  for (int b = 0; b < G; ++b) ds[(size_t)b] = b;           // member b is "data set b" of the staging area
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    if ((rc = ard_stage_group(h, st, a, nb, ell + g0 * ldell, ldell, sn_tilde + g0, first + g0, hdiv))) return rc;
    if ((rc = batch_group_fit_on(h, s, nb, kernel_id, one.data(), sn_tilde + g0, ds.data(), a.X, a.y, a.Xs, m))) return rc;
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const long i = g0 + b;
      finish_results(s.res_host + 512 * b, s.info_host[b], n, m, sn_tilde[i], kss.data(), out + 4 * i, mean ? mean + i * m : nullptr, var ? var + i * m : nullptr);
    }
  }
  h->built = h->factored = h->fitted = false;               // slot 0 no longer holds the single-fit state
  return SIGP_OK;
}

int sigp_nlml_grad_ard_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* theta, int64_t ntheta, int64_t ldtheta, int grad_mode,
                             double* nlml, double* grad, int64_t ldgrad) {
  if (!h || !theta || !nlml) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: bad argument");
  int rc;
  if ((rc = ard_batch_check(h, "nlml_grad_ard_batch", first, count, kernel_id))) return rc;
  if (grad_mode != 0 && grad_mode != 2) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: grad_mode 0 (value) or 2 (exact gradient)");
  if (grad_mode != 0 && !grad) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: grad buffer required");
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, n_pad = h->b_npad, ld = n_pad;
  if (ntheta != d + 1) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", d + 1, (long long)ntheta);
  if (ldtheta < ntheta) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: ldtheta = %lld below ntheta = %lld", (long long)ldtheta, (long long)ntheta);
  if (grad_mode != 0 && ldgrad < d + 1) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard_batch: ldgrad = %lld below d + 1 = %ld", (long long)ldgrad, d + 1);
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
  if (grad_mode != 0) {
    if ((rc = scores_ensure(h, G, n_pad, ArdParts::size(G, ntiles, dp, d + 1)))) return rc;
    if ((rc = scores_mlii_ensure(h, (long)G * n_pad, G, n_pad, dp))) return rc;
  }
  const ArdParts ap{h->gPart, G, ntiles, dp, d + 1};
  const ArdMemberStrides ms{n_pad * dp, n_pad * n_pad, n_pad, 512, ap.mstride()};
  std::vector<double> hdiv((size_t)(a.cap * (dp + 1))), one((size_t)G, 1.0), ell((size_t)G * d), snt((size_t)G), gh((size_t)G * (d + 1));
  std::vector<int> ds((size_t)G);
  std::vector<char> ok((size_t)G);
  for (int b = 0; b < G; ++b) ds[(size_t)b] = b;
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    for (int b = 0; b < nb; ++b) {
      const double* th = theta + (g0 + b) * ldtheta;
      bool good = true;
      for (long k = 0; k < d; ++k) {
        const double l = std::exp(th[k]);
        ell[(size_t)(b * d + k)] = l;
        if (!std::isfinite(l) || !(l > 0)) good = false;
      }
      snt[(size_t)b] = std::exp(th[d]);
      if (!std::isfinite(snt[(size_t)b])) good = false;
      if (!good) {                                           // the member rides along at harmless parameters; its results are dropped
        std::fill(ell.begin() + b * d, ell.begin() + (b + 1) * d, 1.0);
        snt[(size_t)b] = 1.0;
      }
      ok[(size_t)b] = good;
    }
    if ((rc = ard_stage_group(h, st, a, nb, ell.data(), d, snt.data(), first + g0, hdiv))) return rc;
    if ((rc = batch_group_fit_on(h, s, nb, kernel_id, one.data(), snt.data(), ds.data(), a.X, a.y, a.Xs, 0))) return rc;
    if (grad_mode != 0) {
      // for every member at once: U = L~^-T, K~^-1 = U U^T (lower 128-tiles in gK), A~ = U z: the route of sigp_nlml_grad_batch
      if ((rc = inv_factor(h, st, nb, s.mat, s.matStride, s.dinv, s.dinvStride, n_pad))) return rc;
      if ((rc = kinv_lower(h, st, nb, n_pad))) return rc;
      if ((rc = alpha_from_U(h, st, nb, s.mat + n_pad * ld, s.matStride, h->scratchZ, n_pad, n_pad))) return rc;
      // the one pass over every member's K~^-1 and the fixed-order sums, one launch each (q = y^T A~ in the slot's result rows)
      double* partial = ap.partial();
      double* gdev = ap.grad();
      {
        ProfScope ps(h, st, SIGP_KC_MLII, nb * ((double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 30)), nb * (4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp)));
        if ((rc = ard_tile_pass_members<ARD_W_NLML>(h, st, nb, a.X, n, d, dp, n_pad, ms, kernel_id, h->gK, ld, h->scratchZ, s.res, nullptr, nullptr, partial))) return rc;
        hipLaunchKernelGGL(ard_grad_finish_kernel, dim3((unsigned)(d + 1), (unsigned)nb), dim3(256), 0, st, (const double*)partial, ntiles, (int)dp, (int)d, (int)n,
                           (const double*)h->gK, ld, (const double*)h->scratchZ, (const double*)s.res, 0.0, gdev, ms, ap.gw, (const double*)a.sn);
        HIPCHK(h, hipGetLastError());
      }
      HIPCHK(h, hipMemcpyAsync(gh.data(), gdev, (size_t)nb * (d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const long i = g0 + b;
      const bool good = ok[(size_t)b] && s.info_host[b] == 0;
      double out[4];
      finish_results(s.res_host + 512 * b, good ? 0 : 1, n, 0, snt[(size_t)b], nullptr, out, nullptr, nullptr);
      nlml[i] = out[1];
      if (grad_mode == 0) continue;
      for (long k = 0; k <= d; ++k) grad[i * ldgrad + k] = good ? gh[(size_t)(b * (d + 1) + k)] : inf;
    }
  }
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}
