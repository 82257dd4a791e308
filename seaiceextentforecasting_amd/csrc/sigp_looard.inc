// sigp_loo_grad_ard: the leave-one-out scores AND the exact derivatives of one of them with respect to (log l_1 .. log l_d, log sn~)
// (looard.hpp has the formulae and the kernels).  Included inside extern "C" of sigp.hip, after sigp_loograd.inc and sigp_ardgrad.inc.
//
// The scales are set and the fit is made as sigp_nlml_grad_ard makes it (ell = 1, sigp_fit_predict's own launches); then, on top of
// loo_launch (U = L~^-T in gU, the scores: the same launches as sigp_loo, so the same bits):
//   P = U U^T        lower 128-tiles into gK (n^3/3), mirrored to the full symmetric matrix (loo_grad_mirror_kernel);  a = U z
//   beta, gamma, eps the coefficients of the chosen score and sigma mode (loo_ard_coef_kernel: a, diag P and q from device memory)
//   v = P beta, P Gamma into gD, one pass over the rows of P (loo_ard_scale_kernel)
//   M = (P Gamma) P^T lower 128-tiles into gU, which is dead by then: syrk128_kernel's SET form on the lower tile space, whole diagonal tiles
//                    (the DG form of a diagonal tile belongs to the product form !SET alone, and A != B here anyway): n^3 flops for any d
//   the ARD pass     ard_grad_partial_kernel<., ARD_W_LOO> over M, v, a, eps, then loo_ard_finish_kernel
// Memory: sigp_loo_grad's single-fit buffers (gU, gK, gD, gV, gPart; gPart also holds the pass's per-tile partials) plus ardXc.
// Profile class: SIGP_KC_MLII (on top of loo_launch's two entries: U U^T, the n^2 passes, the product M, the ARD pass: one entry each).
// Out of scope: the lockstep-batch entries, sigp_small_*, the fp32 engine, sharded fits.  The leave-block-out scores: sigp_cvard.inc.

int sigp_loo_grad_ard(sigp_handle* h, int kernel_id, const double* theta, int64_t ntheta, int sigma_mode, int criterion, double* mean, double* var, double* score,
                      double* grad) {
  if (!h || !theta || !score) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: bad argument (theta [d + 1], score [2] required)");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: mean and var come together (both NULL: scores and gradient only)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  if (h->n == 0) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: call set_train first");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: fp64 engine only");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: RBF / MATERN52 only");
  if (h->n < 2) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: leave-one-out needs n >= 2 training points");
  if (ntheta != h->d + 1) return fail(h, SIGP_BAD_ARG, "loo_grad_ard: theta = (log l_1 .. log l_d, log sn~): %ld entries required (got %lld)", h->d + 1, (long long)ntheta);
  const long n = h->n, d = h->d, dp = h->dp, n_pad = h->n_pad, ld = n_pad;
  const double inf = std::numeric_limits<double>::infinity(), qnan = std::nan("");
  auto all_inf = [&]() -> int {
    score[0] = score[1] = inf;
    if (grad) for (long k = 0; k <= d; ++k) grad[k] = inf;
    if (mean) for (long i = 0; i < n; ++i) mean[i] = var[i] = qnan;
    return SIGP_NOT_SPD;
  };
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

  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const int T = (int)(n_pad / NB);
  const long ntiles = kbuild_tiles(n_pad), sM = n_pad * n_pad;
  // every buffer before the first launch: growing one of them later would drop what the earlier launches left in it
  if ((rc = ensure(h, &h->gU, &h->cap_gU, sM))) return rc;
  if ((rc = ensure(h, &h->gK, &h->cap_gK, sM))) return rc;
  if ((rc = ensure(h, &h->gPart, &h->cap_gPart, 4 * n_pad + 4 + (grad ? ntiles * dp + dp + 1 : 0)))) return rc;
  if (grad) {
    if ((rc = ensure(h, &h->gD, &h->cap_gD, sM))) return rc;
    if ((rc = ensure(h, &h->gV, &h->cap_gV, LooArdVecs::size(n_pad)))) return rc;
    if ((rc = ensure(h, &h->ardXc, &h->cap_ardXc, n_pad * dp))) return rc;
  }
  double* tail = h->gPart + 4 * n_pad;              // score [2], then q = y^T A~, as sigp_loo
  HIPCHK(h, hipMemcpyAsync(tail + 2, h->fit_res.data(), sizeof(double), hipMemcpyHostToDevice, st));
  if ((rc = loo_launch(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, h->y, 0, nullptr, tail + 2, 0, sigma_mode, 1))) return rc;
  if (mean) {
    HIPCHK(h, hipMemcpyAsync(mean, h->gPart, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(var, h->gPart + n_pad, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipMemcpyAsync(score, tail, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!grad) return sync_slot(h, s);

  LooArdVecs w{h->gV, n_pad};
  {   // P = U U^T, lower tiles
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * n_pad * n_pad / 3, 0.0);
    GemmArgs g{};
    g.A = h->gU; g.lda = ld; g.B = h->gU; g.ldb = ld; g.C = h->gK; g.ldc = ld; g.K = (int)n_pad;
    g.r0 = 0; g.r1 = T; g.c0 = 0; g.c1 = T; g.lower = 1; g.ktri = 1;
    if ((rc = launch_syrk128_t<double, true>(h, st, g))) return rc;
  }
  {   // a = U z;  P -> full;  beta, gamma, eps;  v = P beta and P Gamma
    ProfScope ps(h, st, SIGP_KC_MLII, 4.0 * n_pad * n_pad, 36.0 * n_pad * n_pad);
    hipLaunchKernelGGL(rowdot_kernel<double>, dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, st, (const double*)h->gU, ld, (int)n_pad, (int)n_pad, 2,
                       (const double*)(s.mat + n_pad * ld), ld, w.a(), ld, 1, 0);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_grad_mirror_kernel, dim3((unsigned)(n_pad / 32), (unsigned)(n_pad / 32), 1u), dim3(256), 0, st, h->gK, ld, sM);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_ard_coef_kernel, dim3(1), dim3(256), 0, st, (const double*)h->gK, ld, (int)n, (int)n_pad, (const double*)(tail + 2), sigma_mode, criterion, w);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_ard_scale_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, st, (const double*)h->gK, h->gD, ld, (int)n, (int)n_pad, w);
    HIPCHK(h, hipGetLastError());
  }
  {   // M = (P Gamma) P^T: tile (bi, bj), bi >= bj, = rows bi of P Gamma against rows bj of P (= its columns), the whole K span
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * n_pad * (n_pad + NB), 0.0);
    GemmArgs g{};
    g.A = h->gD; g.lda = ld; g.B = h->gK; g.ldb = ld; g.C = h->gU; g.ldc = ld; g.K = (int)n_pad;
    g.r0 = 0; g.r1 = T; g.c0 = 0; g.c1 = T; g.lower = 1; g.ktri = 0;
    if ((rc = launch_syrk128_t<double, true>(h, st, g))) return rc;
  }
  double* partial = tail + 4;
  double* gdev = partial + ntiles * dp;
  {   // the one pass: every tile's share of all d components, then the fixed-order sums
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n * n * (3.0 * d + 4.0 * ((d + 15) / 16 * 16) + 36), 4.0 * n * n + 8.0 * ntiles * (192.0 * d + dp));
    const int kid = kernel_id == SIGP_KERNEL_RBF ? KID_RBF : KID_MATERN52;
    HIPCHK(h, hipMemsetAsync(h->ardXc, 0, (size_t)n_pad * dp * sizeof(double), st));
    hipLaunchKernelGGL(ard_center_kernel, dim3((unsigned)d), dim3(256), 0, st, (const double*)h->X, (int)dp, (int)n, h->ardXc);
    if (d <= 8)
      hipLaunchKernelGGL((ard_grad_partial_kernel<8, ARD_W_LOO>), dim3((unsigned)ntiles), dim3(256), 0, st, (const double*)h->X, (const double*)h->ardXc, (int)dp, (int)d, (int)n,
                         kid, (const double*)h->gU, ld, (const double*)w.a(), (const double*)nullptr, partial, (const double*)w.v(), (const double*)w.eps());
    else
      hipLaunchKernelGGL((ard_grad_partial_kernel<32, ARD_W_LOO>), dim3((unsigned)ntiles), dim3(256), 0, st, (const double*)h->X, (const double*)h->ardXc, (int)dp, (int)d, (int)n,
                         kid, (const double*)h->gU, ld, (const double*)w.a(), (const double*)nullptr, partial, (const double*)w.v(), (const double*)w.eps());
    hipLaunchKernelGGL(loo_ard_finish_kernel, dim3((unsigned)(d + 1)), dim3(256), 0, st, (const double*)partial, ntiles, (int)dp, (int)d, (int)n, (const double*)h->gU, ld, w, snt, gdev);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(grad, gdev, (size_t)(d + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  return sync_slot(h, s);
}
