// sigp_set_length_scales, sigp_nlml_grad_ard: per-feature (ARD) length scales for the RBF / Matern-5/2 kernels (include/sigp.h).
// The ARD kernel is the isotropic one at ell = 1 on u = x / l, so the scales live in the STAGING: the handle keeps the raw features and
// ride rows beside the scaled ones the builds read (pad_copy_kernel's divisor), and every later staging of test points divides alike.
// No covariance function and no existing kernel changes; a handle that never sets scales runs the launches it ran before.
// Out of scope: the lockstep-batch entries (their resident data is staged by sigp_batch_upload and stays isotropic), the one-workgroup
// kernel (sigp_small_*), the fp32 engine, sharded fits.  ARD gradients of the leave-one-out / leave-block-out scores: sigp_looard.inc, sigp_cvard.inc.

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
  if (h->n == 0) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: call set_train first");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: fp64 engine only");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: RBF / MATERN52 only");
  if (grad_mode != 0 && grad_mode != 2) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: grad_mode 0 (value) or 2 (exact gradient)");
  if (grad_mode != 0 && !grad) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: grad buffer required");
  if (ntheta != h->d + 1) return fail(h, SIGP_BAD_ARG, "nlml_grad_ard: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", h->d + 1, (long long)ntheta);
  const long n = h->n, d = h->d, dp = h->dp, n_pad = h->n_pad, ld = n_pad;
  const double inf = std::numeric_limits<double>::infinity();
  auto all_inf = [&]() -> int { *nlml = inf; if (grad) for (long k = 0; k <= d; ++k) grad[k] = inf; return SIGP_NOT_SPD; };
  std::vector<double> ell((size_t)d);
  for (long k = 0; k < d; ++k) ell[(size_t)k] = std::exp(theta[k]);
  const double snt = std::exp(theta[d]);
  for (long k = 0; k < d; ++k)
    if (!std::isfinite(ell[(size_t)k]) || !(ell[(size_t)k] > 0)) return all_inf();
  if (!std::isfinite(snt)) return all_inf();
  int rc;
  if ((rc = sigp_set_length_scales(h, ell.data(), d))) return rc;
  double out[4];
  rc = sigp_fit_predict(h, kernel_id, 1.0, snt, nullptr, 0, out, nullptr, nullptr);
  if (rc == SIGP_NOT_SPD) return all_inf();
  if (rc) return rc;
  *nlml = out[1];
  if (grad_mode == 0) return SIGP_OK;

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const int T = (int)(n_pad / NB);
  const long ntiles = kbuild_tiles(n_pad);
  if ((rc = ensure(h, &h->gU, &h->cap_gU, n_pad * n_pad))) return rc;
  if ((rc = ensure(h, &h->gK, &h->cap_gK, n_pad * n_pad))) return rc;
  if ((rc = ensure(h, &h->gPart, &h->cap_gPart, ntiles * dp + dp + 1))) return rc;
  if ((rc = ensure(h, &h->scratchZ, &h->cap_Z, (long)RIDE * n_pad))) return rc;
  if ((rc = ensure(h, &h->ardXc, &h->cap_ardXc, n_pad * dp))) return rc;
  // U = L~^-T, K~^-1 = U U^T (lower 128-tiles in gK), A~ = U z: the route of sigp_nlml_grad
  {
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * n_pad * n_pad / 3, 0.0);
    if ((rc = trtri_levels<double>(h, st, s.mat, ld, s.dinv, h->gU, h->gK, ld, T, T))) return rc;
  }
  {
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * n_pad * n_pad / 3, 0.0);
    GemmArgs g{};
    g.A = h->gU; g.lda = ld; g.B = h->gU; g.ldb = ld; g.C = h->gK; g.ldc = ld; g.K = (int)n_pad;
    g.r0 = 0; g.r1 = T; g.c0 = 0; g.c1 = T; g.lower = 1; g.ktri = 1;
    if ((rc = launch_syrk128_t<double, true>(h, st, g))) return rc;
  }
  hipLaunchKernelGGL(rowdot_kernel<double>, dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, st, (const double*)h->gU, ld, (int)n_pad, (int)n_pad, 2,
                     (const double*)(s.mat + n_pad * ld), ld, h->scratchZ, ld, 1, 0);
  HIPCHK(h, hipGetLastError());
  // the one pass: every tile's share of all d components, then the fixed-order sums (s.res[0] = y^T A~ of the fit just made)
  double* partial = h->gPart;
  double* gdev = h->gPart + ntiles * dp;
  {
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 30), 4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp));
    HIPCHK(h, hipMemsetAsync(h->ardXc, 0, (size_t)n_pad * dp * sizeof(double), st));
    hipLaunchKernelGGL(ard_center_kernel, dim3((unsigned)d), dim3(256), 0, st, (const double*)h->X, (int)dp, (int)n, h->ardXc);
    if (d <= 8)
      hipLaunchKernelGGL(ard_grad_partial_kernel<8>, dim3((unsigned)ntiles), dim3(256), 0, st, (const double*)h->X, (const double*)h->ardXc, (int)dp, (int)d, (int)n,
                         kernel_id == SIGP_KERNEL_RBF ? KID_RBF : KID_MATERN52, (const double*)h->gK, ld, (const double*)h->scratchZ, (const double*)s.res, partial);
    else
      hipLaunchKernelGGL(ard_grad_partial_kernel<32>, dim3((unsigned)ntiles), dim3(256), 0, st, (const double*)h->X, (const double*)h->ardXc, (int)dp, (int)d, (int)n,
                         kernel_id == SIGP_KERNEL_RBF ? KID_RBF : KID_MATERN52, (const double*)h->gK, ld, (const double*)h->scratchZ, (const double*)s.res, partial);
    hipLaunchKernelGGL(ard_grad_finish_kernel, dim3((unsigned)(d + 1)), dim3(256), 0, st, (const double*)partial, ntiles, (int)dp, (int)d, (int)n, (const double*)h->gK, ld,
                       (const double*)h->scratchZ, (const double*)s.res, snt, gdev);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(grad, gdev, (size_t)(d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  return sync_slot(h, s);
}
