// sigp_sparse_fit / sigp_sparse_predict: inducing-point (sparse) GP regression -- DTC predictive, Titsias' collapsed bound -- for n past the
// dense limit.  Included inside extern "C" of sigp.hip.  K = sigma_f (k + sn~ I), m inducing points Z, jitter eps:
//
//   L   = chol(k(Z,Z) + eps I)                 the covariance build with eps in the noise slot, potrf_slot           (slot spA)
//   V_c = L^-1 k(Z, X_c)        [m_pad][chunk] per chunk of rows of X: sparse_cross_kernel (GEMM-form distances; below 16 features the
//                                              direct differences of ride_build_kernel, the covariance build's own choice), then a block
//                                              forward substitution FROM THE LEFT with the factor's inverse diagonal blocks -- the
//                                              whitened form; no explicit L^-1, no normal equations (docs/EXPERIMENTS.md, "Sparse fit")
//   N  -= V_c V_c^T             lower tiles    launch_syrk128_t, K = chunk, into the matrix of slot spB
//   b  += V_c y_c, yy += |y_c|^2                     sparse_stats_kernel; b lives in ride row 0 of slot spB
//   n - t += sum_j (1 - |V_c[:, j]|^2)               sparse_trace_kernel: the trace term as column deficits, not as n minus a sum of size n
//   B   = sn~ I - N, L_B = chol(B), w = L_B^-1 b     sparse_assemble_kernel, potrf_slot (w = the solved ride row), epilogue_kernel
//
// Everything of one call runs in stream order, chunks ascending, no atomics: the same bits on every run.  The dense state of the handle
// (sigp_set_train, slot 0) is not touched; the two factors live in slots of their own.  Workspaces (doubles): 2 (m_pad + 128) m_pad for the
// slots, m_pad chunk for V_c, chunk (dp + ldx + 1) for the staged chunk.

static int sparse_cross(sigp_handle* h, hipStream_t st, const double* Xc, long nc, long ncp, double* Kc) {
  const long m = h->sp_m, m_pad = h->sp_mpad, d = h->sp_d, dp = h->sp_dp;
  ProfScope ps(h, st, SIGP_KC_KBUILD, (double)m * nc * (3.0 * d + 20), 8.0 * (m_pad * ncp + (double)(nc + m) * d));
  if (h->opt_kbuild_mfma == 1 || (h->opt_kbuild_mfma == 2 && d >= 16)) {
    dim3 grid((unsigned)(ncp / KB_TN), (unsigned)(m_pad / KB_TM));
    if (d <= 8) hipLaunchKernelGGL(sparse_cross_kernel<8>, grid, dim3(256), 0, st, (const double*)h->spZ, Xc, (int)dp, (int)d, (int)m, (int)nc, Kc, ncp, (const KParams*)h->spKps);
    else hipLaunchKernelGGL(sparse_cross_kernel<32>, grid, dim3(256), 0, st, (const double*)h->spZ, Xc, (int)dp, (int)d, (int)m, (int)nc, Kc, ncp, (const KParams*)h->spKps);
  } else {
    hipLaunchKernelGGL(ride_build_kernel<double>, dim3((unsigned)((ncp + 255) / 256), (unsigned)m_pad, 1), dim3(256), 0, st, Xc, 0L, (const double*)h->spZ, 0L,
                       (const double*)nullptr, 0L, (int)dp, (int)d, (int)nc, (int)ncp, (int)m, 0, Kc, 0L, ncp, (const KParams*)h->spKps, 1);
  }
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// V [m_pad][ncp] <- L^-1 V by block rows: V[kb] = inv(L_kk) V[kb] (in place: a 128 x 128 tile reads only the columns it writes),
// V[kb+1:] -= L[kb+1:, kb] V[kb]
static int sparse_whiten(sigp_handle* h, hipStream_t st, const Slot& s, double* V, long m_pad, long ncp) {
  const int T = (int)(m_pad / NB);
  ProfScope ps(h, st, SIGP_KC_TRSM, (double)m_pad * m_pad * ncp, 4.0 * m_pad * m_pad + 16.0 * m_pad * ncp);
  for (int kb = 0; kb < T; ++kb) {
    int rc;
    GemmArgs g{};
    g.A = s.dinv + (long)kb * NB * NB; g.lda = NB; g.B = V + (long)kb * NB * ncp; g.ldb = ncp; g.C = V + (long)kb * NB * ncp; g.ldc = ncp;
    g.K = NB; g.r0 = 0; g.r1 = 1; g.c0 = 0; g.c1 = (int)(ncp / NB); g.lower = 0;
    if ((rc = launch_gemm_cfg<128, 128, 2, 2, GEMM_SET, true>(h, st, g))) return rc;
    if (kb + 1 < T) {
      GemmArgs u{};
      u.A = s.mat + (long)(kb + 1) * NB * m_pad + (long)kb * NB; u.lda = m_pad; u.B = V + (long)kb * NB * ncp; u.ldb = ncp;
      u.C = V + (long)(kb + 1) * NB * ncp; u.ldc = ncp;
      u.K = NB; u.r0 = 0; u.r1 = T - kb - 1; u.c0 = 0; u.c1 = (int)(ncp / NB); u.lower = 0;
      if ((rc = launch_gemm_cfg<128, 128, 2, 2, GEMM_SUB, true>(h, st, u))) return rc;
    }
  }
  return SIGP_OK;
}

static int sparse_not_spd(sigp_handle* h, double* out, int info, const char* what) {
  const double inf = std::numeric_limits<double>::infinity();
  out[0] = out[1] = out[2] = inf; out[3] = (double)info;
  return fail(h, SIGP_NOT_SPD, "sparse_fit: %s is not positive definite (pivot %d)", what, info);
}

int sigp_sparse_fit(sigp_handle* h, int kernel_id, const double* ell, int64_t nell, double sn_tilde, double jitter, const double* X, int64_t n,
                    int64_t d, int64_t ldx, const double* y, const double* Z, int64_t m, int64_t ldz, double* out) {
  if (!h) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "sparse_fit: fp64 handles only (SIGP_F64)");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "sparse_fit: kernel_id must be SIGP_KERNEL_RBF (1) or SIGP_KERNEL_MATERN52 (2), got %d (the reference kernel is not covered)", kernel_id);
  if (!ell || !X || !y || !Z || !out) return fail(h, SIGP_BAD_ARG, "sparse_fit: ell, X, y, Z and out [4] required");
  if (n < 1 || n > (1LL << 31) - 1 - 65536) return fail(h, SIGP_BAD_ARG, "sparse_fit: 1 <= n < 2^31 - 65536 required (n = %lld)", (long long)n);
  if (d < 1 || d > 4096 || ldx < d || ldz < d) return fail(h, SIGP_BAD_ARG, "sparse_fit: 1 <= d <= 4096 features and ldx, ldz >= d required (d = %lld, ldx = %lld, ldz = %lld)", (long long)d, (long long)ldx, (long long)ldz);
  if (m < 1 || m > SIGP_SPARSE_MAX_INDUCING) return fail(h, SIGP_BAD_ARG, "sparse_fit: 1 <= m <= %d inducing points required (m = %lld)", SIGP_SPARSE_MAX_INDUCING, (long long)m);
  if (nell != 1 && nell != d) return fail(h, SIGP_BAD_ARG, "sparse_fit: nell must be 1 or d = %lld (nell = %lld)", (long long)d, (long long)nell);
  for (int64_t p = 0; p < nell; ++p)
    if (!(ell[p] > 0) || !std::isfinite(ell[p])) return fail(h, SIGP_BAD_ARG, "sparse_fit: every length scale must be finite and > 0 (ell[%lld] = %g)", (long long)p, ell[p]);
  if (!(sn_tilde > 0) || !std::isfinite(sn_tilde)) return fail(h, SIGP_BAD_ARG, "sparse_fit: sn_tilde > 0 required (got %g)", sn_tilde);
  if (!(jitter >= 0) || !std::isfinite(jitter)) return fail(h, SIGP_BAD_ARG, "sparse_fit: jitter >= 0 required (got %g)", jitter);
  HIPCHK(h, hipSetDevice(h->device));
  h->sp_fitted = false;
  h->built = h->factored = h->fitted = false;           // the dense entries refuse as before any fit
  const bool ard = nell == d && d > 1;
  const long m_pad = round_up(m, NB), dp = round_up(d, 64);
  const long chunk = std::min<long>(h->opt_sparse_chunk, round_up(n, NB));
  int rc;
  Slot& sa = h->spA; Slot& sb = h->spB;
  if ((rc = slot_reserve(h, sa, m_pad, 1))) return rc;
  if ((rc = slot_reserve(h, sb, m_pad, 1))) return rc;
  if ((rc = ensure(h, &h->spZ, &h->cap_spZ, m_pad * dp))) return rc;
  if ((rc = ensure(h, &h->spXc, &h->cap_spXc, chunk * dp))) return rc;
  if ((rc = ensure(h, &h->spY, &h->cap_spY, chunk))) return rc;
  if ((rc = ensure(h, &h->spK, &h->cap_spK, m_pad * chunk))) return rc;
  if ((rc = ensure(h, &h->spT, &h->cap_spT, chunk / 64 + 8))) return rc;
  if ((rc = ensure(h, &h->spDiv, &h->cap_spDiv, dp))) return rc;
  if ((rc = ensure(h, &h->stage, &h->cap_stage, std::max<long>(m * ldz, chunk * ldx)))) return rc;
  constexpr int PRED_CHUNKS = 16;
  if (!h->spKps) HIPCHK(h, hipMalloc((void**)&h->spKps, PRED_CHUNKS * sizeof(KParams)));
  hipStream_t st = sa.s_upd;
  h->sp_m = m; h->sp_mpad = m_pad; h->sp_d = d; h->sp_dp = dp; h->sp_n = n; h->sp_ard = ard; h->sp_sn = sn_tilde;
  h->sp_kp = make_kparams(kernel_id, ard ? 1.0 : ell[0], jitter, 0);
  {
    KParams kpc[PRED_CHUNKS];
    for (int k = 0; k < PRED_CHUNKS; ++k) { kpc[k] = h->sp_kp; kpc[k].ds = k; }       // "data set" k = chunk k of a prediction group
    HIPCHK(h, hipMemcpyAsync(h->spKps, kpc, sizeof kpc, hipMemcpyHostToDevice, st));
    if (ard) HIPCHK(h, hipMemcpyAsync(h->spDiv, ell, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));                                                // kpc lives on this frame
  }
  const double* div = ard ? (const double*)h->spDiv : nullptr;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](int k) { const auto t1 = std::chrono::steady_clock::now(); h->sp_ms[k] = std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1; };
  // 1. L = chol(k(Z,Z) + eps I): the jitter rides in the covariance build's noise slot
  HIPCHK(h, hipMemcpyAsync(h->stage, Z, (size_t)((m - 1) * ldz + d) * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((m_pad * dp + 255) / 256)), dim3(256), 0, st, (const double*)h->stage, (long)ldz, (int)m, (int)d, h->spZ, (int)m_pad,
                     (int)dp, div);
  HIPCHK(h, hipGetLastError());
  {
    ProfScope ps(h, st, SIGP_KC_KBUILD, (double)m * m / 2 * (3.0 * d + 20), 8.0 * m * d + 4.0 * m * (m + 1));
    launch_kbuild<double>(h, dim3((unsigned)kbuild_tiles(m_pad), 1, 1), st, h->spZ, 0L, (int)dp, (int)d, (int)m, sa.mat, sa.matStride, m_pad, h->spKps, 0);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemsetAsync(sa.mat + m_pad * m_pad, 0, (size_t)RIDE * m_pad * sizeof(double), st));   // no ride rows
  if ((rc = potrf_slot(h, sa, 1, m_pad, false, 1))) return rc;
  HIPCHK(h, hipMemcpyAsync(sa.info_host, sa.info, sizeof(int), hipMemcpyDeviceToHost, st));
  if ((rc = sync_slot(h, sa))) return rc;
  lap(0);
  if (*sa.info_host != 0) return sparse_not_spd(h, out, *sa.info_host, "k(Z,Z) + jitter I");
  // 2. the chunks, ascending
  HIPCHK(h, hipMemsetAsync(sb.mat, 0, (size_t)(m_pad + RIDE) * m_pad * sizeof(double), st));
  HIPCHK(h, hipMemsetAsync(h->spT, 0, (size_t)(chunk / 64 + 8) * sizeof(double), st));   // [chunk / 64] deficit partials, then yy
  double* bvec = sb.mat + m_pad * m_pad;                  // ride row 0 of slot spB
  const int T = (int)(m_pad / NB);
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const long nc = (long)std::min<int64_t>(chunk, n - c0), ncp = round_up(nc, NB);
    HIPCHK(h, hipMemcpyAsync(h->stage, X + c0 * ldx, (size_t)((nc - 1) * ldx + d) * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((ncp * dp + 255) / 256)), dim3(256), 0, st, (const double*)h->stage, (long)ldx, (int)nc, (int)d, h->spXc, (int)ncp,
                       (int)dp, div);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemsetAsync(h->spY, 0, (size_t)ncp * sizeof(double), st));
    HIPCHK(h, hipMemcpyAsync(h->spY, y + c0, (size_t)nc * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = sparse_cross(h, st, h->spXc, nc, ncp, h->spK))) return rc;
    if ((rc = sparse_whiten(h, st, sa, h->spK, m_pad, ncp))) return rc;
    {
      GemmArgs g{};
      g.A = h->spK; g.lda = ncp; g.B = h->spK; g.ldb = ncp; g.C = sb.mat; g.ldc = m_pad; g.K = (int)ncp;
      g.r0 = 0; g.r1 = T; g.c0 = 0; g.c1 = T; g.lower = 1;
      ProfScope ps(h, st, SIGP_KC_SYRK128, (double)m_pad * m_pad * ncp, 8.0 * (m_pad * ncp + (double)m_pad * m_pad), (int)ncp);
      if ((rc = launch_syrk128_t<double, false>(h, st, g))) return rc;
    }
    hipLaunchKernelGGL(sparse_stats_kernel, dim3((unsigned)(m_pad / 4 + 1)), dim3(256), 0, st, (const double*)h->spK, ncp, (int)m_pad, (int)ncp, (const double*)h->spY, bvec,
                       h->spT + chunk / 64);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(sparse_trace_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(256), 0, st, (const double*)h->spK, ncp, (int)m, (int)nc, h->spT);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(st));
  lap(1);
  // 3. B = sn~ I - N, L_B = chol(B), w = L_B^-1 b (the ride row)
  hipStream_t sq = sb.s_upd;
  hipLaunchKernelGGL(sparse_assemble_kernel, dim3((unsigned)((m_pad * m_pad + 255) / 256)), dim3(256), 0, sq, sb.mat, m_pad, (int)m, (int)m_pad, sn_tilde);
  HIPCHK(h, hipGetLastError());
  if ((rc = potrf_slot(h, sb, 1, m_pad, false, 1))) return rc;
  {
    ProfScope ps(h, sq, SIGP_KC_EPILOGUE, 4.0 * m, 16.0 * m);
    hipLaunchKernelGGL(epilogue_kernel<double>, dim3(2, 1), dim3(256), 0, sq, (const double*)bvec, m_pad, (const double*)bvec, (const double*)sb.mat, m_pad, (int)m, (int)m_pad, 1,
                       sb.res, 0L, 0L, 0L);
    HIPCHK(h, hipGetLastError());
  }
  std::vector<double> tv((size_t)chunk / 64 + 8);
  HIPCHK(h, hipMemcpyAsync(sb.res_host, sb.res, 512 * sizeof(double), hipMemcpyDeviceToHost, sq));
  HIPCHK(h, hipMemcpyAsync(sb.info_host, sb.info, sizeof(int), hipMemcpyDeviceToHost, sq));
  HIPCHK(h, hipMemcpyAsync(tv.data(), h->spT, tv.size() * sizeof(double), hipMemcpyDeviceToHost, sq));
  if ((rc = sync_slot(h, sb))) return rc;
  lap(2);
  if (*sb.info_host != 0) return sparse_not_spd(h, out, *sb.info_host, "sn~ I + V V^T");
  double deficit = 0.0;                                   // n - |V|_F^2
  for (long b = 0; b < chunk / 64; ++b) deficit += tv[(size_t)b];
  const double yy = tv[(size_t)(chunk / 64)], ww = sb.res_host[0], logdiag = sb.res_host[256];
  const double sf = (yy - ww) / (sn_tilde * (double)n);
  const double hlogdet = 0.5 * ((double)n - (double)m) * std::log(sn_tilde) + logdiag;
  const double nlml = 0.5 * n + hlogdet + 0.5 * n * std::log(sf) + 0.5 * n * std::log(2.0 * M_PI);
  out[0] = sf; out[1] = nlml; out[2] = nlml + deficit / (2.0 * sn_tilde); out[3] = 0.0;
  h->sp_sigma_f = sf;
  h->sp_fitted = true;
  return SIGP_OK;
}

int sigp_sparse_predict(sigp_handle* h, const double* Xs, int64_t ms, int64_t ldxs, double* mean, double* var) {
  if (!h) return SIGP_BAD_ARG;
  if (!h->sp_fitted || h->built || h->factored || h->fitted)
    return fail(h, SIGP_BAD_ARG, "sparse_predict: call sigp_sparse_fit first (a dense build or fit since then has replaced the sparse fit)");
  if (!Xs || !mean || !var || ms < 1 || ldxs < h->sp_d)
    return fail(h, SIGP_BAD_ARG, "sparse_predict: Xs [ms >= 1][ldxs >= d = %ld], mean [ms] and var [ms] required (ms = %lld, ldxs = %lld)", h->sp_d, (long long)ms, (long long)ldxs);
  HIPCHK(h, hipSetDevice(h->device));
  Slot& sa = h->spA; Slot& sb = h->spB;
  hipStream_t st = sa.s_upd;
  const long m = h->sp_m, m_pad = h->sp_mpad, d = h->sp_d, dp = h->sp_dp;
  constexpr int PRED_CHUNKS = 16;   // lockstep group of the forward solves, as sigp_predict
  const long gmax = std::min<long>(PRED_CHUNKS, (ms + RIDE - 1) / RIDE);
  int rc;
  if ((rc = ensure(h, &h->spP, &h->cap_spP, gmax * RIDE * m_pad))) return rc;
  if ((rc = ensure(h, &h->spQ, &h->cap_spQ, gmax * RIDE * m_pad))) return rc;
  const long raw = gmax * RIDE * std::max<long>(ldxs, dp);           // stage = [raw group | padded group [gmax*128][dp] | results [gmax][512]]
  if ((rc = ensure(h, &h->stage, &h->cap_stage, raw + gmax * RIDE * dp + gmax * 512))) return rc;
  double* xs_grp = h->stage + raw;
  double* res_grp = xs_grp + gmax * RIDE * dp;
  const double* w = sb.mat + m_pad * m_pad;                           // the solved ride row of slot spB
  std::vector<double> res_host((size_t)gmax * 512);
  for (int64_t c0 = 0; c0 < ms; c0 += gmax * RIDE) {
    const long mg = (long)std::min<int64_t>(gmax * RIDE, ms - c0);
    const int nch = (int)((mg + RIDE - 1) / RIDE);
    HIPCHK(h, hipMemcpyAsync(h->stage, Xs + c0 * ldxs, (size_t)((mg - 1) * ldxs + d) * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)(((long)nch * RIDE * dp + 255) / 256)), dim3(256), 0, st, (const double*)h->stage, (long)ldxs, (int)mg, (int)d, xs_grp,
                       nch * RIDE, (int)dp, h->sp_ard ? (const double*)h->spDiv : nullptr);
    HIPCHK(h, hipGetLastError());
    {
      ProfScope ps(h, st, SIGP_KC_KBUILD, (double)nch * RIDE * m * (3.0 * d + 20), 8.0 * nch * RIDE * m_pad);
      hipLaunchKernelGGL(ride_build_kernel<double>, dim3((unsigned)((m_pad + 255) / 256), RIDE, (unsigned)nch), dim3(256), 0, st, (const double*)h->spZ, 0L, (const double*)xs_grp,
                         (long)RIDE * dp, (const double*)nullptr, 0L, (int)dp, (int)d, (int)m, (int)m_pad, (int)RIDE, 0, h->spP, (long)RIDE * m_pad, m_pad,
                         (const KParams*)h->spKps, 1);
      HIPCHK(h, hipGetLastError());
    }
    {
      ProfScope ps(h, st, SIGP_KC_TRSM, 2.0 * nch * RIDE * m_pad * m_pad, 8.0 * m_pad * m_pad + 32.0 * nch * RIDE * m_pad);
      if ((rc = solve_rows_forward_t<double>(h, st, sa.mat, sa.dinv, h->spP, m_pad, nch))) return rc;      // rows p = L^-1 k(Z, x*)
      HIPCHK(h, hipMemcpyAsync(h->spQ, h->spP, (size_t)nch * RIDE * m_pad * sizeof(double), hipMemcpyDeviceToDevice, st));
      if ((rc = solve_rows_forward_t<double>(h, st, sb.mat, sb.dinv, h->spQ, m_pad, nch))) return rc;      // rows q = L_B^-1 p
    }
    hipLaunchKernelGGL(sparse_pred_kernel, dim3(RIDE, (unsigned)nch), dim3(256), 0, st, (const double*)h->spP, (const double*)h->spQ, m_pad, (int)m_pad, w, res_grp);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(res_host.data(), res_grp, (size_t)nch * 512 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (long j = 0; j < mg; ++j) {
      const double* rj = res_host.data() + (j / RIDE) * 512;
      mean[c0 + j] = rj[j % RIDE];
      var[c0 + j] = h->sp_sigma_f * (1.0 + h->sp_sn - rj[256 + j % RIDE] + h->sp_sn * rj[128 + j % RIDE]);
    }
  }
  return SIGP_OK;
}
