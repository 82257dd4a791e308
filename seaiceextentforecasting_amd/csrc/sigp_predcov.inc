// sigp_predict_cov: the joint posterior of m new test points (mean + the full m x m covariance).  Included inside extern "C" of sigp.hip.
//
//   Z   = k~(Xs, X) L~^-T           [m_pad][n_pad], ALL of it resident (sigp_predict reuses one group's worth): built like sigp_predict's
//                                   rows, solved by the same lockstep groups of at most 16 chunks of 128 rows (solve_rows_forward)
//   mean_j = Z_j . z                epilogue_kernel against z = L~^-1 y -- the launch and the row arithmetic of sigp_predict: the same bits
//   cov = sigma_f (K** + [noise] sn~ I - Z Z^T)      predcov_partial_kernel (split-K over S slices) + predcov_finish_kernel (predcov.hpp)
//
// Only reads the factor, the ride rows and the fit's state.  Workspaces (doubles): covZ m_pad n_pad, covXs m_pad dp, covC m_pad^2,
// covPart S P 128^2 when S > 1 (P = c (c + 1) / 2 tile pairs, c = m_pad / 128), covRes 512 c; reference kernel: covTs m_pad dp, covK m_pad^2.

// slices of the covariance product: 0 (auto) = the smallest S that gives every CU two workgroups, within the partials' workspace bound
static int predcov_slices(const sigp_handle* h, long P, long nkb) {
  if (h->opt_cov_slices > 0) return h->opt_cov_slices;
  constexpr long MAX_PARTIAL_TILES = 8192;                 // 1 GiB of partials at most (auto only: a fixed S is the caller's choice)
  long S = (2L * h->ncu + P - 1) / P;
  S = std::min(S, std::max(1L, MAX_PARTIAL_TILES / P));
  return (int)std::max(1L, std::min(S, nkb));
}

// ONE launch of predcov_partial_kernel: P tile pairs x S slices of Z Z^T, Z [m_pad][ldz] with nkb block columns, into the tiles of t.
// sigp_predict_cov and the debug library's run-and-return entry (sigp_debug_run_predcov) both launch through here.  The refusal guards the
// tile's 32-bit DMA offsets (syrk128.hpp); it needs a row of 32 MiB, a matrix no test can allocate: it is not reached by any test.
static int launch_predcov_partial(sigp_handle* h, hipStream_t st, const double* Z, long ldz, int nkb, long P, int S, const PredcovTiles& t) {
  if (!sy_row_stride_ok(ldz, sizeof(double))) return fail(h, SIGP_BAD_ARG, "predictive covariance: row stride beyond the tile's 32-bit DMA offsets");
  static AttrOnce attr;
  HIPCHK(h, attr.set(h->device, (const void*)predcov_partial_kernel, SY_LDS_BYTES));
  hipLaunchKernelGGL(predcov_partial_kernel, dim3((unsigned)P, (unsigned)S), dim3(256), SY_LDS_BYTES, st, Z, ldz, nkb, t);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

int sigp_predict_cov(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, int noise, double* mean, double* cov, int64_t ldc) {
  if (!h) return SIGP_BAD_ARG;
  if (!Xs || !mean || !cov) return fail(h, SIGP_BAD_ARG, "predict_cov: bad argument (Xs [m][ldxs], mean [m], cov [m][ldc] required)");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "predict_cov: fp64 engine only (the fp32 engine's variances carry the fp32 factor's accuracy: no joint covariance from it)");
  if (!h->fitted) return fail(h, SIGP_BAD_ARG, "predict_cov: call sigp_fit / sigp_fit_predict first (a sharded fit leaves no single-GPU factor: sigp_predict_cov does not apply)");
  if (m < 1 || m > SIGP_MAX_COV) return fail(h, SIGP_BAD_ARG, "predict_cov: 1 <= m <= %d test points required (m = %lld)", SIGP_MAX_COV, (long long)m);
  if (ldxs < h->d) return fail(h, SIGP_BAD_ARG, "predict_cov: Xs needs %ld columns (ldxs = %lld)", h->d, (long long)ldxs);
  if (ldc < m) return fail(h, SIGP_BAD_ARG, "predict_cov: cov [m][ldc >= m] required (ldc = %lld)", (long long)ldc);
  const bool refk = h->kernel_id == SIGP_KERNEL_NETDIFFUSION;
  if (refk && (!h->T || !h->Sig)) return fail(h, SIGP_BAD_ARG, "predict_cov: no Sigma state");
  const long n = h->n, n_pad = h->n_pad, ld = n_pad, dp = h->dp, d = h->d;
  const long m_pad = round_up(m, RIDE), c = m_pad / RIDE, P = c * (c + 1) / 2, nkb = n_pad / NB;
  if (h->opt_cov_slices > nkb) return fail(h, SIGP_BAD_ARG, "predict_cov: cov_slices = %d exceeds the %ld block columns of this fit", h->opt_cov_slices, nkb);
  const int S = predcov_slices(h, P, nkb);
  h->cov_slices_used = S;
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  int rc;
  if ((rc = ensure(h, &h->covZ, &h->cap_covZ, m_pad * n_pad))) return rc;
  if ((rc = ensure(h, &h->covXs, &h->cap_covXs, m_pad * dp))) return rc;
  if ((rc = ensure(h, &h->covC, &h->cap_covC, m_pad * m_pad))) return rc;
  if ((rc = ensure(h, &h->covRes, &h->cap_covRes, c * 512))) return rc;
  if (S > 1 && (rc = ensure(h, &h->covPart, &h->cap_covPart, (long)S * P * NB * NB))) return rc;
  if (refk) {
    if ((rc = ensure(h, &h->covTs, &h->cap_covTs, m_pad * dp))) return rc;
    if ((rc = ensure(h, &h->covK, &h->cap_covK, m_pad * m_pad))) return rc;
  }
  if ((rc = ensure(h, &h->stage, &h->cap_stage, m * ldxs))) return rc;
  // test rows, zero padded to [m_pad][dp] (padding rows are ordinary points at the origin: finite everywhere, never copied out)
  HIPCHK(h, hipMemcpyAsync(h->stage, Xs, (size_t)((m - 1) * ldxs + d) * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((m_pad * dp + 255) / 256)), dim3(256), 0, st, h->stage, (long)ldxs, (int)m, (int)d, h->covXs, (int)m_pad, (int)dp,
                     h->ard_on ? (const double*)h->ardDiv : nullptr);
  HIPCHK(h, hipGetLastError());
  constexpr int PRED_CHUNKS = 16;   // lockstep group of the forward solve, as sigp_predict
  if (refk) {
    ProfScope ps(h, st, SIGP_KC_KBUILD, 2.0 * m * d * (n + d + m), 8.0 * (m_pad * n_pad + 2.0 * m_pad * m_pad));
    GemmArgs g{};                   // rows k~(xs, X) = xs T^T, T = X Sigma~ of the fit
    g.A = h->covXs; g.lda = dp; g.B = h->T; g.ldb = dp; g.C = h->covZ; g.ldc = ld; g.K = (int)dp;
    g.r0 = 0; g.r1 = (int)(m_pad / 64); g.c0 = 0; g.c1 = (int)(n_pad / 64); g.lower = 0;
    if ((rc = launch_gemm_cfg<64, 64, 2, 2, GEMM_SET, false>(h, st, g))) return rc;
    GemmArgs g2{};                  // T_s = Xs Sigma~
    g2.A = h->covXs; g2.lda = dp; g2.B = h->Sig; g2.ldb = dp; g2.C = h->covTs; g2.ldc = dp; g2.K = (int)dp;
    g2.r0 = 0; g2.r1 = (int)(m_pad / 64); g2.c0 = 0; g2.c1 = (int)(dp / 64); g2.lower = 0;
    if ((rc = launch_gemm_cfg<64, 64, 2, 2, GEMM_SET, false>(h, st, g2))) return rc;
    GemmArgs g3{};                  // K** = T_s Xs^T, every tile: the finish step takes its symmetric part
    g3.A = h->covTs; g3.lda = dp; g3.B = h->covXs; g3.ldb = dp; g3.C = h->covK; g3.ldc = m_pad; g3.K = (int)dp;
    g3.r0 = 0; g3.r1 = (int)(m_pad / 64); g3.c0 = 0; g3.c1 = (int)(m_pad / 64); g3.lower = 0;
    if ((rc = launch_gemm_cfg<64, 64, 2, 2, GEMM_SET, false>(h, st, g3))) return rc;
  } else {
    if (!h->pred_kps) HIPCHK(h, hipMalloc((void**)&h->pred_kps, PRED_CHUNKS * sizeof(KParams)));
    KParams kpc[PRED_CHUNKS];
    for (int k = 0; k < PRED_CHUNKS; ++k) { kpc[k] = h->kp; kpc[k].ds = k; }   // "data set" k = chunk k of a group (strideXs below)
    HIPCHK(h, hipMemcpyAsync(h->pred_kps, kpc, sizeof kpc, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));                                         // kpc lives on this frame
    ProfScope ps(h, st, SIGP_KC_KBUILD, (double)m_pad * n * (3.0 * d + 20), 8.0 * (m_pad * n_pad + (double)n * d));
    for (long c0 = 0; c0 < c; c0 += PRED_CHUNKS) {
      const int nch = (int)std::min<long>(PRED_CHUNKS, c - c0);
      hipLaunchKernelGGL(ride_build_kernel<double>, dim3((unsigned)((n_pad + 255) / 256), RIDE, (unsigned)nch), dim3(256), 0, st, h->X, 0L,
                         h->covXs + c0 * RIDE * dp, (long)RIDE * dp, (const double*)nullptr, 0L, (int)dp, (int)d, (int)n, (int)n_pad, (int)RIDE, 0,
                         h->covZ + c0 * RIDE * ld, (long)RIDE * ld, ld, h->pred_kps, 1);
      HIPCHK(h, hipGetLastError());
    }
  }
  const double* z = s.mat + n_pad * ld;   // solved row 0 of the ride block: z = L~^-1 y
  for (long c0 = 0; c0 < c; c0 += PRED_CHUNKS) {
    const int nch = (int)std::min<long>(PRED_CHUNKS, c - c0);
    double* Zg = h->covZ + c0 * RIDE * ld;
    {
      ProfScope ps(h, st, SIGP_KC_TRSM, (double)nch * RIDE * n_pad * n_pad, 4.0 * n_pad * n_pad + 16.0 * nch * RIDE * n_pad);
      if ((rc = solve_rows_forward(h, s, Zg, n_pad, nch))) return rc;
    }
    hipLaunchKernelGGL(epilogue_kernel<double>, dim3((unsigned)RIDE, (unsigned)nch), dim3(256), 0, st, (const double*)Zg, ld, z, (const double*)nullptr, ld, (int)n,
                       (int)n_pad, (int)RIDE, h->covRes + c0 * 512, (long)RIDE * ld, 0L, 0L);
    HIPCHK(h, hipGetLastError());
  }
  PredcovTiles t{};
  t.inplace = S == 1;
  if (t.inplace) { t.part = h->covC; t.tile_stride = 0; t.ldp = m_pad; t.slice_stride = 0; }
  else { t.part = h->covPart; t.tile_stride = (long)NB * NB; t.ldp = NB; t.slice_stride = P * NB * NB; }
  {
    ProfScope ps(h, st, SIGP_KC_EPILOGUE, (double)P * 2.0 * NB * NB * n_pad, 8.0 * P * (2.0 * NB * n_pad + (double)S * NB * NB), (int)(n_pad / S));
    if ((rc = launch_predcov_partial(h, st, h->covZ, ld, (int)nkb, P, S, t))) return rc;
  }
  {
    PredcovFinish f{};
    f.t = t; f.S = S; f.C = h->covC; f.ldc = m_pad; f.Xs = h->covXs; f.dp = (int)dp; f.d = (int)d;
    f.Kss = refk ? h->covK : nullptr; f.ldk = m_pad; f.kp = h->kp; f.sigma_f = h->sigma_f; f.noise = noise != 0;
    ProfScope ps(h, st, SIGP_KC_EPILOGUE, (double)P * NB * NB * (S + (refk ? 4.0 : 3.0 * d + 20)), 8.0 * P * NB * NB * (S + 2.0 + (refk ? 2.0 : 0.0)));
    hipLaunchKernelGGL(predcov_finish_kernel, dim3((unsigned)P, 16), dim3(256), 0, st, f);
    HIPCHK(h, hipGetLastError());
  }
  std::vector<double> res((size_t)c * 512);
  HIPCHK(h, hipMemcpyAsync(res.data(), h->covRes, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpy2DAsync(cov, (size_t)ldc * sizeof(double), h->covC, (size_t)m_pad * sizeof(double), (size_t)m * sizeof(double), (size_t)m, hipMemcpyDeviceToHost, st));
  if ((rc = sync_slot(h, s))) return rc;
  for (long j = 0; j < m; ++j) mean[j] = res[(size_t)(j / RIDE) * 512 + j % RIDE];
  return SIGP_OK;
}
