// sigp_set_length_scales, sigp_nlml_grad_ard: per-feature (ARD) length scales for the RBF / Matern-5/2 kernels (include/sigp.h).
// The ARD kernel is the isotropic one at ell = 1 on u = x / l, so the scales live in the STAGING: the handle keeps the raw features and
// ride rows beside the scaled ones the builds read (pad_copy_kernel's divisor), and every later staging of test points divides alike.
// No covariance function and no existing kernel changes; a handle that never sets scales runs the launches it ran before.
// Out of scope: the one-workgroup kernel (sigp_small_*), the fp32 engine, sharded fits.  Per-feature scales per fit of a lockstep group on the
// resident batch data: sigp_ardbatch.inc.  ARD gradients of the leave-one-out / leave-block-out scores: sigp_looard.inc, sigp_cvard.inc.
// Included inside extern "C" of sigp.hip, after sigp_scores.inc (the shared steps: sigp_nlml_grad_ard is ard_check_engine, ard_theta_fit,
// inv_factor, kinv_lower, alpha_from_U, ard_tile_pass<ARD_W_NLML> and its own finish kernel) and sigp_blockcv.inc.

// X, Xs <- raw / l (or the raw values back); the fit is void afterwards
static int ard_restage(sigp_handle* h, bool scaled) {
  hipStream_t st = h->slots[0].s_upd;
  const long n_pad = h->n_pad, dp = h->dp;
  if (scaled) {
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((n_pad * dp + 255) / 256)), dim3(256), 0, st, (const double*)h->Xraw, dp, (int)n_pad, (int)h->d, h->X, (int)n_pad,
                       (int)dp, (const double*)h->ardDiv);
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((RIDE * dp + 255) / 256)), dim3(256), 0, st, (const double*)h->XsRaw, dp, RIDE, (int)h->d, h->Xs, RIDE, (int)dp,
                       (const double*)h->ardDiv);
    HIPCHK(h, hipGetLastError());
  } else {
    HIPCHK(h, hipMemcpyAsync(h->X, h->Xraw, (size_t)n_pad * dp * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->Xs, h->XsRaw, (size_t)RIDE * dp * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}

int sigp_set_length_scales(sigp_handle* h, const double* ell, int64_t d) {
  if (!h) return SIGP_BAD_ARG;
  if (!ell) {                                     // back to isotropic: the raw features again, bit for bit
    if (!h->ard_on) return SIGP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    h->ard_on = false;
    return ard_restage(h, false);
  }
  if (h->n == 0) return fail(h, SIGP_BAD_ARG, "set_length_scales: call set_train first");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "set_length_scales: fp64 engine only");
  if (d != h->d) return fail(h, SIGP_BAD_ARG, "set_length_scales: %lld scales for %ld features", (long long)d, h->d);
  for (int64_t k = 0; k < d; ++k)
    if (!(ell[k] > 0) || !std::isfinite(ell[k])) return fail(h, SIGP_BAD_ARG, "set_length_scales: finite ell[k] > 0 required (k = %lld)", (long long)k);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->slots[0].s_upd;
  const long n_pad = h->n_pad, dp = h->dp;
  int rc;
  if (!h->ard_on) {                               // X and Xs hold the raw values: keep them
    if ((rc = ensure(h, &h->Xraw, &h->cap_Xraw, n_pad * dp))) return rc;
    if ((rc = ensure(h, &h->XsRaw, &h->cap_XsRaw, (long)RIDE * dp))) return rc;
    if ((rc = ensure(h, &h->ardDiv, &h->cap_ardDiv, dp))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->Xraw, h->X, (size_t)n_pad * dp * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->XsRaw, h->Xs, (size_t)RIDE * dp * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  h->ard_ell.assign((size_t)dp, 1.0);
  std::copy(ell, ell + d, h->ard_ell.begin());
  HIPCHK(h, hipMemcpyAsync(h->ardDiv, h->ard_ell.data(), (size_t)dp * sizeof(double), hipMemcpyHostToDevice, st));
  h->ard_on = true;
  return ard_restage(h, true);
}

int sigp_nlml_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int grad_mode, double* nlml, double* grad) {
  if (!h || !theta || !nlml) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: bad argument");
  int rc;
  if ((rc = ard_check_engine(h, "nlml_grad_ard", kernel_id))) return rc;
  if (grad_mode != 0 && grad_mode != 2) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: grad_mode 0 (value) or 2 (exact gradient)");
  if (grad_mode != 0 && !grad) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: grad buffer required");
  if ((rc = ard_check_theta(h, "nlml_grad_ard", ntheta))) return rc;
  double snt, out[4];
  rc = ard_theta_fit(h, kernel_id, theta, &snt, out);
  if (rc == SIGP_NOT_SPD) {
    *nlml = std::numeric_limits<double>::infinity();
    if (grad) for (long k = 0; k <= h->d; ++k) grad[k] = *nlml;
  }
  if (rc) return rc;
  *nlml = out[1];
  if (grad_mode == 0) return SIGP_OK;

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, d = h->d, dp = h->dp, n_pad = h->n_pad, ld = n_pad;
  const long ntiles = kbuild_tiles(n_pad);
  if ((rc = scores_ensure(h, 1, n_pad, ArdParts::size(1, ntiles, dp, dp + 1)))) return rc;
  if ((rc = scores_mlii_ensure(h, (long)RIDE * n_pad, 1, n_pad, dp))) return rc;
  const ArdParts ap{h->gPart, 1, ntiles, dp, dp + 1};
  // U = L~^-T, K~^-1 = U U^T (lower 128-tiles in gK), A~ = U z: the route of sigp_nlml_grad
  if ((rc = inv_factor(h, st, 1, s.mat, 0, s.dinv, 0, n_pad))) return rc;
  if ((rc = kinv_lower(h, st, 1, n_pad))) return rc;
  if ((rc = alpha_from_U(h, st, 1, s.mat + n_pad * ld, 0, h->scratchZ, 0, n_pad))) return rc;
  // the one pass: every tile's share of all d components, then the fixed-order sums (s.res[0] = y^T A~ of the fit just made)
  double* partial = ap.partial();
  double* gdev = ap.grad();
  {
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 30), 4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp));
    if ((rc = ard_tile_pass<ARD_W_NLML>(h, st, kernel_id, h->gK, ld, h->scratchZ, s.res, nullptr, nullptr, partial))) return rc;
    hipLaunchKernelGGL(ard_grad_finish_kernel, dim3((unsigned)(d + 1)), dim3(256), 0, st, (const double*)partial, ntiles, (int)dp, (int)d, (int)n, (const double*)h->gK, ld,
                       (const double*)h->scratchZ, (const double*)s.res, snt, gdev);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(grad, gdev, (size_t)(d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  return sync_slot(h, s);
}
