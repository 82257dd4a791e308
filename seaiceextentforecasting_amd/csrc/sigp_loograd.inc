// sigp_loo_grad / sigp_loo_grad_batch: the leave-one-out scores AND their exact derivatives with respect to (log l, log sn~) (loograd.hpp has
// the formulae and the kernels).  Included inside extern "C" of sigp.hip, after sigp_scores.inc (the shared steps) and loo_launch.
//
// On top of loo_launch (U = L~^-T in gU, the scores: the same launches as sigp_loo, so the same bits), per lockstep member:
//   P = U U^T        kinv_lower: lower 128-tiles into gK (as sigp_nlml_grad, n^3/3);  mirror_P: to the full symmetric matrix
//   a = U z          alpha_from_U, as sigp_nlml_grad
//   t = D a, D -> D' one pass over gD (loo_grad_prep_kernel)
//   W' = D' P        into gU, which is dead by then: syrk_set on the full tile space with ktri = 1 (n^3 flops; the walk
//                    issues the row blocks with the longest K spans first)
//   b, P a, sum P^2  one pass over the rows of P (loo_grad_rows_kernel);  c = 2 colsum(W' o P) by row chunks (loo_grad_cols_kernel)
//   the chain rule per point and four fixed-order sums (loo_grad_point_kernel)
// Memory per member: 8 n_pad^2 bytes each for the slot matrix, gU, gK and gD -- the lockstep path holds gD per member, which
// sigp_nlml_grad_batch avoids by recomputing dK~ on the fly -- plus (5 + n_pad / 128) n_pad doubles of vectors.
// Profile class: SIGP_KC_MLII (on top of loo_launch's two entries: U U^T, the product W' with n_pad^3 flops, and one entry for the n^2 passes).
// Out of scope: gradients in sigp_small_run_loo (the one-workgroup LDS kernel), sharded fits, the fp32 engine.  Gradients with respect to
// per-feature length scales: sigp_loo_grad_ard (sigp_looard.inc).

static int loo_grad_ensure(sigp_handle* h, int G, long n_pad) {
  int rc;
  if ((rc = scores_ensure(h, G, n_pad, ScoreParts::size(G, n_pad)))) return rc;
  return scores_grad_ensure(h, G, n_pad, LooGradVecs::size(n_pad));
}

// dK~/dlog l of RBF / Matern members into gD (full symmetric, zero on the padding): member b has data set ds[b] of X (stride strideX) and
// length scale ell[b]
static int loo_grad_build_dlogl(sigp_handle* h, hipStream_t st, int nb, int kernel_id, const double* ell, const int* ds, const double* X, long strideX,
                                long n, long d, long dp, long n_pad) {
  int rc;
  if ((rc = upload_dlogl_kparams(h, st, nb, kernel_id, ell, ds))) return rc;
  ProfScope ps(h, st, SIGP_KC_KBUILD, nb * ((double)n * n * (3.0 * d + 20)), nb * 8.0 * n_pad * n_pad);
  dim3 grid((unsigned)(n_pad / KB_TN), (unsigned)(n_pad / KB_TM), (unsigned)nb);
  launch_kbuild<double>(h, grid, st, X, strideX, (int)dp, (int)d, (int)n, h->gD, n_pad * n_pad, n_pad, h->gKps, 1);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// The gradient pass for nb lockstep members after loo_launch (gU = U) with dK~ in gD: the single fit (nb = 1) and the lockstep groups share it.
// z = the members' solved ride row 0 (stride sZ), q = y^T A~ per member (stride sQ).  Leaves out [4] per member in the vector workspace.
static int loo_grad_launch(sigp_handle* h, hipStream_t st, int nb, long n, long n_pad, const double* z, long sZ, const double* q, long sQ, int mode, LooGradVecs v) {
  const long ld = n_pad, sM = n_pad * n_pad;
  const int T = (int)(n_pad / NB), tri = h->opt_loo_grad_tri;
  int rc;
  if ((rc = kinv_lower(h, st, nb, n_pad))) return rc;
  {   // a = U z;  P -> full;  t = D a and D -> D'
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 3.0 * n_pad * n_pad, nb * 36.0 * n_pad * n_pad);
    if ((rc = alpha_from_U(h, st, nb, z, sZ, v.base, v.stride, n_pad))) return rc;
    if ((rc = mirror_P(h, st, nb, n_pad))) return rc;
    hipLaunchKernelGGL(loo_grad_prep_kernel, dim3((unsigned)(n_pad / 4), (unsigned)nb), dim3(256), 0, st, h->gD, ld, sM, (int)n, (int)n_pad, tri, v);
    HIPCHK(h, hipGetLastError());
  }
  {   // W' = D' P: tile (bi, bj) = rows bi of D' against rows bj of P (= its columns), K from the row block on
    ProfScope ps(h, st, SIGP_KC_MLII, nb * (tri ? 1.0 : 2.0) * n_pad * n_pad * n_pad, 0.0);
    if ((rc = syrk_set(h, st, nb, h->gD, h->gK, h->gU, n_pad, 0, tri ? 1 : 0))) return rc;
  }
  {
    ProfScope ps(h, st, SIGP_KC_MLII, nb * 8.0 * n * n, nb * 24.0 * n * n);
    hipLaunchKernelGGL(loo_grad_rows_kernel, dim3((unsigned)((n + 3) / 4), (unsigned)nb), dim3(256), 0, st, (const double*)h->gK, ld, sM, (int)n, v);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_grad_cols_kernel, dim3((unsigned)T, (unsigned)T, (unsigned)nb), dim3(256), 0, st, (const double*)h->gU, (const double*)h->gK, ld, sM, (int)n, v);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(loo_grad_point_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const double*)h->gK, ld, sM, (int)n, q, sQ, mode, tri ? 2.0 : 1.0, v);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

int sigp_loo_grad(sigp_handle* h, int sigma_mode, const double* MSigma, int64_t ldsigma, double* mean, double* var, double* score, double* grad) {
  if (!h || !score || !grad) return fail(h, SIGP_BAD_ARG, "loo_grad: bad argument (score [2], grad [4] required)");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "loo_grad: mean and var come together (both NULL: scores and gradients only)");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "loo_grad: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "loo_grad: fp64 engine only (the fp32 engine keeps the inverses of its 2048-column diagonal blocks, not L~^-T)");
  if (!h->fitted) return fail(h, SIGP_BAD_ARG, "loo_grad: call sigp_fit / sigp_fit_predict first (a sharded fit leaves no single-GPU factor: sigp_loo_grad does not apply)");
  if (h->n < 2) return fail(h, SIGP_BAD_ARG, "loo_grad: leave-one-out needs n >= 2 training points");
  const bool refk = h->kernel_id == SIGP_KERNEL_NETDIFFUSION;
  if (refk && !MSigma) return fail(h, SIGP_BAD_ARG, "loo_grad: M @ Sigma~ required for the reference kernel");
  if (refk && ldsigma < h->d) return fail(h, SIGP_BAD_ARG, "loo_grad: MSigma [N][ldsigma >= %ld] required", h->d);
  if (refk && !(h->ell > 0)) return fail(h, SIGP_BAD_ARG, "loo_grad: the reference kernel's length scale is known after sigp_fit_predict only (d/dlog l = l d/dl)");
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, ld = n_pad;
  int rc;
  if ((rc = loo_grad_ensure(h, 1, n_pad))) return rc;
  const ScoreParts sp{h->gPart, 1, n_pad};
  const LooGradVecs v{h->gV, LooGradVecs::size(n_pad), n_pad, (int)(n_pad / NB)};
  const double* q = sp.q();
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = loo_launch(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, h->y, 0, nullptr, q, 0, sigma_mode, sp))) return rc;
  if (refk) {
    if ((rc = build_xsxt(h, MSigma, ldsigma, h->gD))) return rc;     // X (M Sigma~) X^T = dK~/dl
  } else {
    const int ds0 = 0;
    if ((rc = loo_grad_build_dlogl(h, st, 1, h->kernel_id, &h->ell, &ds0, h->X, 0L, n, h->d, h->dp, n_pad))) return rc;
  }
  if ((rc = loo_grad_launch(h, st, 1, n, n_pad, s.mat + n_pad * ld, 0, q, 0, sigma_mode, v))) return rc;
  double g4[4];
  if ((rc = scores_to_host(h, st, n, sp, mean, var, score))) return rc;
  HIPCHK(h, hipMemcpyAsync(g4, v.out(0), sizeof g4, hipMemcpyDeviceToHost, st));
  if ((rc = sync_slot(h, s))) return rc;
  const double scale1 = refk ? h->ell : 1.0;        // dK~/dlog l = l X (M Sigma~) X^T
  grad[0] = scale1 * g4[0]; grad[1] = h->sn_tilde * g4[1];
  grad[2] = scale1 * g4[2]; grad[3] = h->sn_tilde * g4[3];
  return SIGP_OK;
}

int sigp_loo_grad_batch(sigp_handle* h, int64_t first, int64_t count, int kernel_id, const double* ell, const double* sn_tilde, int sigma_mode,
                        double* mean, double* var, int64_t nstride, double* score, double* grad) {
  if (!h || h->b_count == 0 || first < 0 || count < 1 || !ell || !sn_tilde || !score || !grad) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: bad argument (sigp_batch_upload first)");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: fp64 engine only");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: RBF / MATERN52 only");
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if ((mean == nullptr) != (var == nullptr)) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: mean and var come together (both NULL: scores and gradients only)");
  if (mean && nstride < h->b_n) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: mean / var [count][nstride >= %ld] required", h->b_n);
  if (h->b_n < 2) return fail(h, SIGP_BAD_ARG, "loo_grad_batch: leave-one-out needs n >= 2 training points");
  int rc;
  if ((rc = batch_check_params(h, "loo_grad_batch", count, ell, sn_tilde))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const long n = h->b_n, d = h->b_d, dp = h->b_dp, n_pad = h->b_npad, ld = n_pad;
  const int G = (int)std::max<long>(1, std::min<long>(h->opt_group, count));
  const double inf = std::numeric_limits<double>::infinity();
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  if ((rc = slot_reserve(h, s, n_pad, G))) return rc;
  if ((rc = loo_grad_ensure(h, G, n_pad))) return rc;
  const ScoreParts sp{h->gPart, G, n_pad};
  const LooGradVecs v{h->gV, LooGradVecs::size(n_pad), n_pad, (int)(n_pad / NB)};
  std::vector<double> mv(mean ? (size_t)G * 2 * n_pad : 0), sc((size_t)G * 2), g4((size_t)G * 4);
  std::vector<int> ds((size_t)G);
  for (long g0 = 0; g0 < count; g0 += G) {
    const int nb = (int)std::min<long>(G, count - g0);
    for (int b = 0; b < nb; ++b) ds[(size_t)b] = (int)((first + g0 + b) % h->b_count);
    if ((rc = batch_group_fit(h, s, nb, kernel_id, ell + g0, sn_tilde + g0, first + g0))) return rc;
    if ((rc = loo_launch(h, st, nb, n, n_pad, s.mat, s.matStride, s.dinv, s.dinvStride, h->by, n_pad, s.kps, s.res, 512, sigma_mode, sp))) return rc;
    if ((rc = loo_grad_build_dlogl(h, st, nb, kernel_id, ell + g0, ds.data(), h->bX, n_pad * dp, n, d, dp, n_pad))) return rc;
    if ((rc = loo_grad_launch(h, st, nb, n, n_pad, s.mat + n_pad * ld, s.matStride, s.res, 512, sigma_mode, v))) return rc;
    if ((rc = batch_scores_fetch(h, st, nb, sp, mean ? mv.data() : nullptr, sc.data()))) return rc;
    HIPCHK(h, hipMemcpy2DAsync(g4.data(), 4 * sizeof(double), v.out(0), (size_t)v.stride * sizeof(double), 4 * sizeof(double), (size_t)nb, hipMemcpyDeviceToHost, st));
    if ((rc = sync_slot(h, s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const long i = g0 + b;
      const bool ok = s.info_host[b] == 0;
      batch_scores_scatter(i, ok, &sc[(size_t)2 * b], mean ? &mv[(size_t)b * 2 * n_pad] : nullptr, n, n_pad, mean, var, nstride, score);
      grad[4 * i] = ok ? g4[(size_t)4 * b] : inf;
      grad[4 * i + 1] = ok ? sn_tilde[i] * g4[(size_t)4 * b + 1] : inf;
      grad[4 * i + 2] = ok ? g4[(size_t)4 * b + 2] : inf;
      grad[4 * i + 3] = ok ? sn_tilde[i] * g4[(size_t)4 * b + 3] : inf;
    }
  }
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}
