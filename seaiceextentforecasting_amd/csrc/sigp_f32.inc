// fp32 engine of libsigp.so (BASELINE configs[4]): fp32 covariance build + blocked Cholesky (potrf_core<float>, sigp_factor.inc), block
// triangular solves and the fp64 iterative refinement.  Included by sigp.hip inside its anonymous namespace (one translation unit).

// ---- fp32 engine: fp32 kernel matrix + Cholesky, fp64 iterative refinement of alpha~ and w_j -----------------
// (BASELINE configs[4]; no reference counterpart -- the reference is fp64 NumPy.  Same outputs as the fp64 path:
//  sigma_f, nlML, mean, var of north/June1st.py:267-277, 246.)
constexpr int REFINE_CHUNKS = 64;
// partial-sum slots of a residual: REFINE_CHUNKS column chunks (+ one per 256 rows for kres_sym_kernel's column sums)
inline size_t refine_part_bytes(long n_pad) { return (size_t)(REFINE_CHUNKS + n_pad / 256 + 1) * 4 * n_pad * sizeof(double); }
// host wait for a stream by polling: the refinement's stopping test sits between two short kernels, and a blocking
// hipStreamSynchronize wakes the host 0.3 ms after the stream is done (kernel trace, n = 32768)
// Hot for the first 2 ms, then with short sleeps, and with a deadline (5 minutes: a refinement step is milliseconds) -- a wedged stream is an
// error, not a host core spinning for ever.
int spin_sync(sigp_handle* h, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  for (long it = 0;; ++it) {
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess) return SIGP_OK;
    if (e != hipErrorNotReady) HIPCHK(h, e);
    if ((it & 255) == 255) {
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (ms > 300e3) return fail(h, SIGP_HIP_ERROR, "fp32 refinement: the stream did not finish within 300 s");
      if (ms > 2.0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
}
int f32_reserve(sigp_handle* h, long n_pad, int G = 1) {
  if (h->cap_f_npad >= n_pad && h->cap_f_G >= G) return SIGP_OK;
  n_pad = std::max(n_pad, h->cap_f_npad); G = std::max(G, h->cap_f_G);
  HIPCHK(h, hipDeviceSynchronize());
  for (float** p : {&h->fmat, &h->fdinv, &h->fZ, &h->fU, &h->fV, &h->fXw}) if (*p) { HIPCHK(h, hipFree(*p)); *p = nullptr; }
  for (double** p : {&h->xq, &h->rq, &h->rpart, &h->fpart}) if (*p) { HIPCHK(h, hipFree(*p)); *p = nullptr; }
  h->cap_f_npad = 0; h->cap_f_G = 0;
  // G lockstep members of the factor (batch path); the solve / refinement workspaces below serve one member at a time
  HIPCHK(h, hipMalloc((void**)&h->fmat, (size_t)G * (n_pad + RIDE) * n_pad * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->fdinv, (size_t)G * (n_pad / NB) * NB * NB * sizeof(float)));
  HIPCHK(h, hipMemset(h->fdinv, 0, (size_t)G * (n_pad / NB) * NB * NB * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->fZ, (size_t)RIDE * n_pad * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->fU, (size_t)n_pad * n_pad * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->fV, (size_t)n_pad * n_pad * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->fXw, (size_t)TS_RHS * n_pad * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->xq, (size_t)4 * n_pad * sizeof(double)));
  HIPCHK(h, hipMalloc((void**)&h->rq, (size_t)4 * n_pad * sizeof(double)));
  HIPCHK(h, hipMalloc((void**)&h->rpart, refine_part_bytes(n_pad)));
  HIPCHK(h, hipMalloc((void**)&h->fpart, (size_t)(n_pad / 256 + 1) * 8 * sizeof(double)));
  HIPCHK(h, hipDeviceSynchronize());
  h->cap_f_npad = n_pad; h->cap_f_G = G;
  h->dc.cap_ref_npad = n_pad;      // (the sharded fp32 fit shares xq / rq / rpart / fpart: they now have this size)
  return SIGP_OK;
}

#define SIGP_DREG_DISPATCH(d, CALL)            \
  do {                                         \
    if ((d) <= 8) { CALL(8); }                 \
    else if ((d) <= 16) { CALL(16); }          \
    else if ((d) <= 32) { CALL(32); }          \
    else { CALL(64); }                         \
  } while (0)

// fp64 copy of K~ for the refinement's residuals (kbuild_kernel's second output): G members of n_pad^2 doubles, if that is at most 40 GB
int f32_kq_reserve(sigp_handle* h, long n_pad, int G) {
  h->kq_members = 0;
  const size_t need = (size_t)G * n_pad * n_pad * sizeof(double);
  if (!h->opt_refine_stored || need > ((size_t)40 << 30)) return SIGP_OK;
  if (h->cap_kq < need) {
    HIPCHK(h, hipDeviceSynchronize());
    if (h->kq) HIPCHK(h, hipFree(h->kq));
    h->kq = nullptr; h->cap_kq = 0;
    if (hipMalloc((void**)&h->kq, need) != hipSuccess) {     // no room for the copy: the residuals recompute the covariance instead (same engine, same results)
      (void)hipGetLastError();
      h->kq = nullptr;
      return SIGP_OK;
    }
    h->cap_kq = need;
  }
  h->kq_members = G;
  return SIGP_OK;
}

// one fp32 fit on slot 0's streams from device-resident X [n_pad][dp], y [n_pad], Xs [128][dp] (m <= 3 ride points)
// fp32 engine in three steps so that the multi-GPU driver can put its own panel loop in the middle:
//   f32_build  fp32 kernel matrix + ride rows into fmat;   factor (potrf_core<float> or the sigp_dist_* panel loop);
//   f32_finish reductions, x0, fp64 iterative refinement, results
int f32_build(sigp_handle* h, int kernel_id, double ell, double sn, const double* X, const double* y, const double* Xs, long n, long d,
              long dp, long n_pad, long m) {
  if (m > 3) return fail(h, SIGP_BAD_ARG, "fp32 engine: at most 3 ride-along test points (refinement solves 1+m systems)");
  if (d > 64) return fail(h, SIGP_BAD_ARG, "fp32 engine: d <= 64 required");
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long ld = n_pad;
  int rc;
  if ((rc = f32_reserve(h, n_pad))) return rc;
  if ((rc = slot_reserve(h, s, NB, 1))) return rc;     // res / info / kps buffers only
  const KParams kp = make_kparams(kernel_id, ell, sn, 0);
  s.kps_host[0] = kp;
  if ((rc = upload_kparams(h, s, 1))) return rc;
  if ((rc = f32_kq_reserve(h, n_pad, 1))) return rc;
  {
    ProfScope ps(h, st, SIGP_KC_KBUILD, (double)n * n / 2 * (3.0 * d + 20), 8.0 * n * d + 2.0 * n * (n + 1));
    dim3 grid((unsigned)kbuild_tiles(n_pad), 1, 1);
    launch_kbuild<float>(h, grid, st, X, 0L, (int)dp, (int)d, (int)n, h->fmat, 0L, ld, s.kps, 0, 0, h->kq_members ? h->kq : (double*)nullptr, 0L);
    HIPCHK(h, hipGetLastError());
    dim3 g2((unsigned)((n_pad + 255) / 256), RIDE, 1);
    hipLaunchKernelGGL(ride_build_kernel<float>, g2, dim3(256), 0, st, X, 0L, Xs, 0L, y, 0L, (int)dp, (int)d, (int)n, (int)n_pad, (int)m, 1,
                       h->fmat + n_pad * ld, 0L, ld, s.kps, 1);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

// ---- block triangular solves of the fp32 refinement (kernels_misc.hpp: rowdot / coldot) ------------------------------
// forward:  X = Z L^-T  (rows = right-hand sides; Z is consumed), backward:  Z = X L^-1 (X is consumed).  Right-looking over
// the 2048-column big blocks: product with the explicit inverse of the diagonal block, then one update of everything left.
int f32_block_forward(sigp_handle* h, hipStream_t st, long n_pad, int nrhs, float* Zw, float* Xout) {
  const long ld = n_pad;
  for (long c0 = 0; c0 < n_pad; c0 += TS_BS) {
    const int kb = (int)std::min<long>(TS_BS, n_pad - c0);
    const long rem = n_pad - (c0 + kb);
    ProfScope ps(h, st, SIGP_KC_TRSM, 2.0 * nrhs * ((double)kb * kb / 2 + (double)rem * kb), 4.0 * ((double)kb * kb / 2 + (double)rem * kb));
    hipLaunchKernelGGL(rowdot_kernel<float>, dim3((unsigned)((kb + 3) / 4)), dim3(256), 0, st, (const float*)(h->fV + c0 * (ld + 1)), ld, kb, kb, 1,
                       (const float*)(Zw + c0), ld, Xout + c0, ld, nrhs, 0);
    if (rem > 0)
      hipLaunchKernelGGL(rowdot_kernel<float>, dim3((unsigned)((rem + 3) / 4)), dim3(256), 0, st, (const float*)(h->fmat + (c0 + kb) * ld + c0), ld, (int)rem, kb, 0,
                         (const float*)(Xout + c0), ld, Zw + c0 + kb, ld, nrhs, 1);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

int f32_block_backward(sigp_handle* h, hipStream_t st, long n_pad, int nrhs, float* Xw, float* Zout) {
  const long ld = n_pad;
  const long nbig = (n_pad + TS_BS - 1) / TS_BS;
  for (long b = nbig - 1; b >= 0; --b) {
    const long c0 = b * TS_BS;
    const int kb = (int)std::min<long>(TS_BS, n_pad - c0);
    ProfScope ps(h, st, SIGP_KC_TRSM, 2.0 * nrhs * ((double)kb * kb / 2 + (double)c0 * kb), 4.0 * ((double)kb * kb / 2 + (double)c0 * kb));
    hipLaunchKernelGGL(rowdot_kernel<float>, dim3((unsigned)((kb + 3) / 4)), dim3(256), 0, st, (const float*)(h->fU + c0 * (ld + 1)), ld, kb, kb, 2,
                       (const float*)(Xw + c0), ld, Zout + c0, ld, nrhs, 0);
    if (c0 > 0)
      hipLaunchKernelGGL(coldot_kernel<float>, dim3((unsigned)(c0 / 64)), dim3(256), 0, st, (const float*)(h->fmat + c0 * ld), ld, (int)c0, kb,
                         (const float*)(Zout + c0), ld, Xw, ld, nrhs);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

// `member`: which lockstep member's reductions / info to use (h->fmat / h->fdinv already point at that member's factor)
int f32_finish(sigp_handle* h, int kernel_id, double ell, double sn, const double* X, const double* y, const double* Xs, long n, long d,
               long dp, long n_pad, long m, double* out, double* mean, double* var, int member = 0) {
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long ld = n_pad;
  const int nrhs = (int)(1 + m);
  const KParams kp = make_kparams(kernel_id, ell, sn, 0);
  int rc;
  {
    const float* Z = h->fmat + n_pad * ld;
    hipLaunchKernelGGL(epilogue_kernel<float>, dim3((unsigned)(m + 2), 1), dim3(256), 0, st, Z, ld, Z, (const float*)h->fmat, ld, (int)n,
                       (int)n_pad, (int)(m + 1), s.res + 512 * member, 0L, 0L, 0L);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(s.res_host + 512 * member, s.res + 512 * member, 512 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(s.info_host + member, s.info + member, sizeof(int), hipMemcpyDeviceToHost, st));
  // inverse-transposes of the factor's 2048-column diagonal blocks (fU) and their transposes (fV; it is the scratch of the
  // inversion first), for the block triangular solves below
  {
    const int T = (int)(n_pad / NB);
    ProfScope ps(h, st, SIGP_KC_MLII, (double)n_pad * TS_BS * TS_BS / 3, 0.0);
    if ((rc = trtri_levels<float>(h, st, h->fmat, ld, h->fdinv, h->fU, h->fV, ld, T, TS_BS / NB))) return rc;
    const int nbig = (int)((n_pad + TS_BS - 1) / TS_BS);
    hipLaunchKernelGGL(transpose_diag_blocks_kernel<float>, dim3(TS_BS / 32, TS_BS / 32, (unsigned)nbig), dim3(256), 0, st, (const float*)h->fU, h->fV, ld, (int)n_pad, TS_BS);
    HIPCHK(h, hipGetLastError());
  }
  // x0 = L^-T (L^-1 b): the ride rows already hold L^-1 [y k*]; one backward block solve finishes them
  HIPCHK(h, hipMemcpyAsync(h->fXw, h->fmat + n_pad * ld, (size_t)nrhs * n_pad * sizeof(float), hipMemcpyDeviceToDevice, st));
  if ((rc = f32_block_backward(h, st, n_pad, nrhs, h->fXw, h->fZ))) return rc;
  {
    const long tot = (long)nrhs * n_pad;
    hipLaunchKernelGGL((convert_rows_kernel<float, double>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)h->fZ, ld, h->xq, ld,
                       nrhs, (int)n_pad, (int)n);
    HIPCHK(h, hipGetLastError());
  }
  const unsigned nblk = (unsigned)((n + 255) / 256);
  // the columns of a residual in chunks, so that the launch fills the chip (~8 workgroups per CU): chunk length a multiple of 64
  const bool stored = member < h->kq_members;            // residuals from the fp64 K~ the build wrote (one more partial: the row pass)
  const double* Kq = stored ? h->kq + (size_t)member * n_pad * n_pad : nullptr;
  const int want = (int)std::min<long>(REFINE_CHUNKS - (stored ? 1 : 0), std::max<long>(1, 2048 / nblk));
  const int jlen = (int)(((n + want - 1) / want + 63) / 64 * 64);
  const unsigned nchunk = (unsigned)((n + jlen - 1) / jlen);
  // kres_sym_kernel's cut of the triangle: 256-row bands x column chunks of symlen (a multiple of 64, at most 32 chunks)
  const bool sym = stored && h->opt_refine_sym;
  const int symS = (int)((n_pad + 255) / 256);
  const int symlen = (int)std::max<long>(256, ((n_pad + 31) / 32 + 63) / 64 * 64);
  const int symJ = (int)((n_pad + symlen - 1) / symlen);
  double* norms_dev = s.res + 512 * member + 496;             // 16 doubles: norms, then the final dots (the epilogue's results end well below; res_host is pinned)
  double* norms_host = s.res_host + 512 * member + 496;
  for (int it = 0; it <= h->opt_refine_iters; ++it) {
    // r = b - K~ x in fp64: from the stored fp64 K~ (two coalesced passes over its lower triangle), or with the covariance recomputed on the fly
    if (stored && h->opt_refine_sym) {   // one pass over the stored triangle
#define CALL_SYM(NR) hipLaunchKernelGGL(kres_sym_kernel<NR>, dim3((unsigned)symS, (unsigned)symJ), dim3(256), 0, st, Kq, ld, (int)n_pad, nrhs, (const double*)h->xq, ld, h->rpart, ld, symlen, symJ)
      if (nrhs == 1) CALL_SYM(1); else if (nrhs == 2) CALL_SYM(2); else CALL_SYM(4);
#undef CALL_SYM
    } else if (stored) {
      hipLaunchKernelGGL(kres_lower_cols_kernel, dim3(nblk, nchunk), dim3(256), 0, st, Kq, ld, (int)n, nrhs, (const double*)h->xq, ld, h->rpart, ld, jlen);
      hipLaunchKernelGGL(kres_lower_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, Kq, ld, (int)n, nrhs, (const double*)h->xq, ld, h->rpart, ld, (int)nchunk);
    } else {
#define CALL_RES(D) hipLaunchKernelGGL(krefine_residual_kernel<D>, dim3(nblk, nchunk), dim3(256), 0, st, X, (int)dp, (int)n, nrhs, (const double*)h->xq, ld, h->rpart, ld, jlen, kp)
      SIGP_DREG_DISPATCH(d, CALL_RES);
#undef CALL_RES
    }
    HIPCHK(h, hipGetLastError());
#define CALL_FIN(D) hipLaunchKernelGGL(krefine_finish_kernel<D>, dim3(nblk, (unsigned)nrhs), dim3(256), 0, st, X, Xs, y, (int)dp, (int)n, nrhs, (const double*)h->rpart, ld, \
                                       sym ? symJ : (int)nchunk + (stored ? 1 : 0), h->rq, ld, kp, 0, -1, sym ? symlen : 0, sym ? symS : 0)
    SIGP_DREG_DISPATCH(d, CALL_FIN);
#undef CALL_FIN
    HIPCHK(h, hipGetLastError());
    // max |r| per right-hand side and max |y| (device; the host reads these 5 numbers, never the residual rows)
    hipLaunchKernelGGL(refine_norms_kernel, dim3((unsigned)nrhs + 1), dim3(1024), 0, st, (const double*)h->rq, ld, (int)n, nrhs, y, norms_dev);
    HIPCHK(h, hipGetLastError());
    if (it == h->opt_refine_iters) break;    // the last pass only measures the residual
    if (h->opt_refine_tol_e > 0 && it > 0) {
      // converged already?  (every right-hand side: y against max|y|, the unit-variance cross-covariances against 1)  Then this
      // residual is the final measurement: one residual + one solve pair saved on every well-conditioned fit
      HIPCHK(h, hipMemcpyAsync(norms_host, norms_dev, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
      if ((rc = spin_sync(h, st))) return rc;
      double worst = 0;
      for (int r = 0; r < nrhs; ++r) worst = std::max(worst, r == 0 ? (norms_host[nrhs] > 0 ? norms_host[0] / norms_host[nrhs] : 0.0) : norms_host[r]);
      if (worst <= std::pow(10.0, -(double)h->opt_refine_tol_e)) break;
    }
    const long tot = (long)nrhs * n_pad;
    hipLaunchKernelGGL((convert_rows_kernel<double, float>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double*)h->rq, ld, h->fZ, ld,
                       nrhs, (int)n_pad, (int)n);
    HIPCHK(h, hipGetLastError());
    if ((rc = f32_block_forward(h, st, n_pad, nrhs, h->fZ, h->fXw))) return rc;
    if ((rc = f32_block_backward(h, st, n_pad, nrhs, h->fXw, h->fZ))) return rc;
    hipLaunchKernelGGL(accumulate_rows_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)h->fZ, ld, h->xq, ld, nrhs,
                       (int)n_pad);
    HIPCHK(h, hipGetLastError());
  }
#define CALL_DOT(D) hipLaunchKernelGGL(krefine_dots_kernel<D>, dim3(nblk), dim3(256), 0, st, X, Xs, y, (int)dp, (int)n, nrhs, (const double*)h->xq, ld, h->fpart, kp)
  SIGP_DREG_DISPATCH(d, CALL_DOT);
#undef CALL_DOT
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(sum_parts8_kernel, dim3(1), dim3(64), 0, st, (const double*)h->fpart, (int)nblk, norms_dev + 8);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(norms_host, norms_dev, 16 * sizeof(double), hipMemcpyDeviceToHost, st));    // norms + the eight dots: pinned, one copy
  if ((rc = spin_sync(h, st))) return rc;
  const int info = s.info_host[member];
  const double inf = std::numeric_limits<double>::infinity();
  if (info != 0) {
    out[0] = inf; out[1] = inf; out[2] = (double)info; out[3] = inf;
    for (long j = 0; j < m; ++j) { if (mean) mean[j] = std::nan(""); if (var) var[j] = std::nan(""); }
    return SIGP_OK;
  }
  double dots0[4] = {0, 0, 0, 0}, dots1[4] = {0, 0, 0, 0};
  for (int r = 0; r < nrhs; ++r) { dots0[r] = norms_host[8 + r]; dots1[r] = norms_host[8 + 4 + r]; }
  const double rmax = norms_host[0], ymax = norms_host[nrhs];
  h->refine_resid = ymax > 0 ? rmax / ymax : 0.0;
  const double sf = dots0[0] / (double)n;                                   // y^T alpha~ / n
  out[0] = sf;
  out[1] = 0.5 * n + s.res_host[512 * member + 256] + 0.5 * n * std::log(sf) + 0.5 * n * std::log(2.0 * M_PI);   // log-det from the fp32 factor
  out[2] = 0.0; out[3] = sf * sn;
  for (long j = 0; j < m; ++j) {
    if (mean) mean[j] = dots0[1 + j];                                       // k*^T alpha~
    if (var) var[j] = sf * (1.0 + sn - dots1[1 + j]);                       // k** + sn~ - k*^T K~^-1 k*
  }
  return SIGP_OK;
}

int f32_fit(sigp_handle* h, int kernel_id, double ell, double sn, const double* X, const double* y, const double* Xs, long n, long d,
            long dp, long n_pad, long m, double* out, double* mean, double* var) {
  int rc = f32_build(h, kernel_id, ell, sn, X, y, Xs, n, d, dp, n_pad, m);
  if (rc) return rc;
  if ((rc = potrf_core<float>(h, h->slots[0], h->fmat, 0, h->fdinv, 0, 1, n_pad, false, 1 + (int)m))) return rc;
  return f32_finish(h, kernel_id, ell, sn, X, y, Xs, n, d, dp, n_pad, m, out, mean, var);
}

// nb fp32 fits of equal order in lockstep (batch path): one covariance build and one blocked Cholesky over all members
// (grid.y / grid.z = member, as the fp64 lockstep batches), then the solves + fp64 refinement member by member (they are
// HBM-bound streams of one factor each and share the workspaces).  kps_host[b] holds member b's hyper-parameters / data set.
int f32_fit_lockstep(sigp_handle* h, int nb, int kernel_id, const double* ell, const double* sn, const long* ds, const double* bX, const double* by,
                     const double* bXs, long n, long d, long dp, long n_pad, long m, double* out, double* mean, double* var) {
  if (m > 3) return fail(h, SIGP_BAD_ARG, "fp32 engine: at most 3 ride-along test points (refinement solves 1+m systems)");
  if (d > 64) return fail(h, SIGP_BAD_ARG, "fp32 engine: d <= 64 required");
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long ld = n_pad, fStride = (n_pad + RIDE) * n_pad, dStride = (n_pad / NB) * NB * NB;
  int rc;
  if ((rc = f32_reserve(h, n_pad, nb))) return rc;
  if ((rc = slot_reserve(h, s, NB, nb))) return rc;     // res / info / kps buffers for nb members
  for (int b = 0; b < nb; ++b) s.kps_host[b] = make_kparams(kernel_id, ell[b], sn[b], (int)ds[b]);
  if ((rc = upload_kparams(h, s, nb))) return rc;
  if ((rc = f32_kq_reserve(h, n_pad, nb))) return rc;
  {
    ProfScope ps(h, st, SIGP_KC_KBUILD, nb * ((double)n * n / 2 * (3.0 * d + 20)), nb * (8.0 * n * d + 2.0 * n * (n + 1)));
    launch_kbuild<float>(h, dim3((unsigned)kbuild_tiles(n_pad), 1, (unsigned)nb), st, bX, n_pad * dp, (int)dp, (int)d, (int)n, h->fmat, fStride, ld, s.kps, 0, 0,
                         h->kq_members ? h->kq : (double*)nullptr, n_pad * n_pad);
    hipLaunchKernelGGL(ride_build_kernel<float>, dim3((unsigned)((n_pad + 255) / 256), RIDE, (unsigned)nb), dim3(256), 0, st, bX, n_pad * dp, bXs, (long)RIDE * dp, by, n_pad,
                       (int)dp, (int)d, (int)n, (int)n_pad, (int)m, 1, h->fmat + n_pad * ld, fStride, ld, s.kps, 1);
    HIPCHK(h, hipGetLastError());
  }
  if ((rc = potrf_core<float>(h, s, h->fmat, fStride, h->fdinv, dStride, nb, n_pad, false, 1 + (int)m))) return rc;
  float* const fm0 = h->fmat; float* const fd0 = h->fdinv;
  for (int b = 0; b < nb && !rc; ++b) {
    h->fmat = fm0 + b * fStride; h->fdinv = fd0 + b * dStride;        // view of member b for the solve / refinement code
    rc = f32_finish(h, kernel_id, ell[b], sn[b], bX + ds[b] * n_pad * dp, by + ds[b] * n_pad, bXs + ds[b] * (long)RIDE * dp, n, d, dp, n_pad, m, out + 4 * b,
                    mean ? mean + b * m : nullptr, var ? var + b * m : nullptr, b);
  }
  h->fmat = fm0; h->fdinv = fd0;
  return rc;
}

int sync_slot(sigp_handle* h, Slot& s) {
  HIPCHK(h, hipStreamSynchronize(s.s_upd));
  return SIGP_OK;
}

