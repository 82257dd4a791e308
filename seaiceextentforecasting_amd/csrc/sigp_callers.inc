// Entry points around the GP block (included by sigp.hip inside extern "C"): the reference kernel at reference size
// (sigp_small_*), ComplexNetworks tau() and intra_links() sums, detrend() -- SURVEY 8f rows 2 and 4, a10 / a11.

// ---- the reference's own kernel at the reference's own size: one workgroup per fit (smallgp.hpp) ---------------------
int sigp_small_upload(sigp_handle* h, int64_t nsets, const int64_t* n, const int64_t* N, const int64_t* m, const int32_t* lam_mode,
                      const double* A_pool, const int64_t* A_off, const double* y_pool, const int64_t* y_off, const double* lam_pool,
                      const int64_t* lam_off) {
  if (!h || nsets < 1 || !n || !N || !m || !lam_mode || !A_pool || !A_off || !y_pool || !y_off || !lam_pool || !lam_off)
    return fail(h, SIGP_BAD_ARG, "small_upload: bad argument");
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "small_upload: fp64 engine only");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<SmallSet> sets((size_t)nsets);
  long totA = 0, toty = 0, totl = 0;
  int nmax = 0, mmax = 0;
  for (int64_t i = 0; i < nsets; ++i) {
    if (n[i] < 1 || n[i] > SM_NMAX) return fail(h, SIGP_BAD_ARG, "small_upload: data set %ld has n = %ld; this path takes 1 <= n <= %d (larger fits go through sigp_fit_predict)", (long)i, (long)n[i], SM_NMAX);
    if (N[i] < 1 || m[i] < 0 || m[i] > SM_MMAX) return fail(h, SIGP_BAD_ARG, "small_upload: data set %ld: N >= 1 and 0 <= m <= %d required", (long)i, SM_MMAX);
    if (lam_mode[i] != 0 && lam_mode[i] != 1) return fail(h, SIGP_BAD_ARG, "small_upload: lam_mode must be 0 (exp(l lam)) or 1 (weights)");
    if (A_off[i] < 0 || y_off[i] < 0 || lam_off[i] < 0) return fail(h, SIGP_BAD_ARG, "small_upload: negative offset");
    SmallSet& s = sets[(size_t)i];
    s.a_off = A_off[i]; s.y_off = y_off[i]; s.lam_off = lam_off[i];
    s.n = (int)n[i]; s.N = (int)N[i]; s.m = (int)m[i]; s.lam_mode = lam_mode[i];
    totA = std::max<long>(totA, A_off[i] + (n[i] + m[i]) * N[i]);
    toty = std::max<long>(toty, y_off[i] + n[i]);
    totl = std::max<long>(totl, lam_off[i] + N[i]);
    nmax = std::max(nmax, s.n); mmax = std::max(mmax, s.m);
  }
  // feature chunk: the largest of 32 / 16 / 8 whose LDS image fits beside the bordered matrix of the largest data set
  const int ch = small_pick_chunk(nmax, mmax, SmallFlavour::Plain, 32);
  if (!ch) return fail(h, SIGP_BAD_ARG, "small_upload: n = %d with m = %d does not fit in LDS", nmax, mmax);
  int rc;
  if ((rc = ensure(h, &h->sm_A, &h->cap_sm_A, totA))) return rc;
  if ((rc = ensure(h, &h->sm_y, &h->cap_sm_y, toty))) return rc;
  if ((rc = ensure(h, &h->sm_lam, &h->cap_sm_lam, totl))) return rc;
  if (h->sm_sets_dev) { HIPCHK(h, hipFree(h->sm_sets_dev)); h->sm_sets_dev = nullptr; }
  HIPCHK(h, hipMalloc((void**)&h->sm_sets_dev, sets.size() * sizeof(SmallSet)));
  HIPCHK(h, hipMemcpy(h->sm_sets_dev, sets.data(), sets.size() * sizeof(SmallSet), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->sm_A, A_pool, (size_t)totA * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->sm_y, y_pool, (size_t)toty * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->sm_lam, lam_pool, (size_t)totl * sizeof(double), hipMemcpyHostToDevice));
  h->sm_sets.swap(sets);
  h->sm_ch = ch; h->sm_mmax = mmax; h->sm_nmax = nmax; h->sm_lds = SmallLayout{nmax, mmax, ch, SmallFlavour::Plain}.bytes();
  h->sm_lam_len = totl; h->sm_has_dlam = false;
  return SIGP_OK;
}

int sigp_small_set_dweights(sigp_handle* h, const double* dlam_pool, int64_t count) {
  if (!h || h->sm_sets.empty()) return fail(h, SIGP_BAD_ARG, "small_set_dweights: call sigp_small_upload first");
  if (!dlam_pool || count != h->sm_lam_len) return fail(h, SIGP_BAD_ARG, "small_set_dweights: the pool must mirror lam_pool (%ld doubles)", h->sm_lam_len);
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = ensure(h, &h->sm_dlam, &h->cap_sm_dlam, count))) return rc;
  HIPCHK(h, hipMemcpy(h->sm_dlam, dlam_pool, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
  h->sm_has_dlam = true;
  return SIGP_OK;
}

// what a launch forms besides the fits, and where it goes
struct SmallRequest {
  SmallFlavour flavour = SmallFlavour::Plain;
  int sigma_mode = 0;                                  // Loo, Cv, Hindcast: SIGP_LOO_REFIT / SIGP_LOO_FIXED
  int64_t block = 0, gap = 0;                          // Cv, CvGrad
  int64_t lead = 0, min_train = 0;                     // Hindcast, HindcastGrad
  int criterion = 0;                                   // LooGrad, HindcastGrad, CvGrad: SIGP_LOO_NLPD / SIGP_LOO_SSE
  double *row_mean = nullptr, *row_var = nullptr;      // Loo, Cv, Hindcast: the caller's [nprob][pitch]
  int64_t pitch = 0;
  // sigp_small_run_k*: a stationary covariance (SmallCov::Stationary) of the sets' raw rows; `ell` is then [nprob][ldell]
  SmallCov cov = SmallCov::Factored;
  int kernel_id = 0;                                   // SIGP_KERNEL_RBF / SIGP_KERNEL_MATERN52
  int ard = 0;                                         // 1: fit p has the scales ell[p ldell + k], k < N of its set; 0: ell[p ldell] for every feature
  int64_t ldell = 1;
  double* grad = nullptr;                              // Grad: the caller's [nprob][ldg]
  int64_t ldg = 0;
  const char* name = "small_run";                      // the entry's name in the messages of the stationary checks
};

extern "C++" {
// one launch of smallgp_kernel<NT, F, C> over nprob fits; the kernel's dynamic-LDS limit is lifted once per device
template <int NT, SmallFlavour F, SmallCov C = SmallCov::Factored>
static hipError_t small_launch(sigp_handle* h, hipStream_t st, int64_t nprob, long lds, int ch, double* d_out, double* d_mean, double* d_var, int ms, const SmallExtras& x) {
  static AttrOnce attr;
  const hipError_t e = attr.set(h->device, (const void*)smallgp_kernel<NT, F, C>, (int)SM_LDS_MAX);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smallgp_kernel<NT, F, C>), dim3((unsigned)nprob), dim3(NT), (size_t)lds, st, h->sm_sets_dev, h->sm_probs, h->sm_A, h->sm_y, h->sm_lam, ch, d_out, d_mean, d_var, ms,
                     h->sm_has_dlam ? h->sm_dlam : nullptr, x);
  return hipGetLastError();
}
}  // extern "C++"

// adds the flops of one fit of the set s in the flavour of rq
static void small_count_flops(double& fl, const SmallSet& s, const SmallRequest& rq) {
  const double n = s.n, inverse = n * n * n / 3;      // X = L~^-1
  const bool stationary = rq.cov == SmallCov::Stationary;
  // the build: a multiply-add per (pair, feature), or a difference and a multiply-add and the covariance function (~40 flops) per pair
  fl += (stationary ? 1.5 * n * (n + 2.0 * s.m) * s.N + 20.0 * n * (n + 2.0 * s.m) : n * n * s.N) + n * n * n / 3 + 2.0 * n * n * (1 + s.m);
  switch (rq.flavour) {
    case SmallFlavour::Plain: break;
    case SmallFlavour::Grad:
      if (stationary) fl += inverse + 1.5 * n * n * s.N + inverse + 20.0 * n * n + 2.0 * n * n * s.N;     // X, sq again, E = W o h, E against every feature's differences
      else fl += n * n * s.N + inverse + 2.0 * n * s.N;                                // X A, A^T a~
      break;
    case SmallFlavour::Loo: fl += inverse + 2.0 * n * n; break;                       // X's column norms and X^T z
    case SmallFlavour::Cv: fl += inverse + 2.0 * n * n; fl += n * n * (rq.block + 2.0 * rq.gap); break;   // ... and the folds' P_SS from X's columns
    case SmallFlavour::Hindcast: fl += 4.0 * n * rq.lead + 2.0 * n * n; break;        // the row segments and the prefix sums of z^2
    // ... then X, b_c = X a_c and x_c^T C x_c: Loo X^T b_c and the lower triangle of P; Hindcast the band and the scan against every column
    case SmallFlavour::LooGrad: fl += 2.0 * inverse + 2.0 * n * n + 2.0 * n * n * s.N + 4.0 * n * (s.N + n); break;
    case SmallFlavour::HindcastGrad: fl += 4.0 * n * rq.lead + 2.0 * n * n + inverse + n * n * s.N + (8.0 * rq.lead + 5.0) * n * (s.N + n); break;
    // Cv's, then per fold H and B_f, b_c = X a_c, p_c = X^T b_c for the features and for X's own columns (P) and the band against every p_c
    case SmallFlavour::CvGrad: {
      const double wd = rq.block + 2.0 * rq.gap;
      fl += inverse + 2.0 * n * n + n * n * wd + (n / rq.block) * (wd * wd * wd / 3 + wd * wd * rq.block) + 2.0 * n * n * s.N + inverse + (2.0 * wd + 4.0) * n * (s.N + n);
      break;
    }
  }
}

static int small_run_impl(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, double* out,
                          double* mean, double* var, int64_t mstride, const SmallRequest& rq) {
  if (!h || h->sm_sets.empty()) return fail(h, SIGP_BAD_ARG, "small_run: call sigp_small_upload first");
  const SmallFlavour F = rq.flavour;
  const bool cv = F == SmallFlavour::Cv || F == SmallFlavour::CvGrad, hc = F == SmallFlavour::Hindcast || F == SmallFlavour::HindcastGrad, rows = small_has_rows(F);
  const char* cvloo = cv ? "cv" : "loo";
  if (nprob < 1 || !set_index || !ell || !sn_tilde || !out) return fail(h, SIGP_BAD_ARG, "small_run: bad argument");
  const bool stationary = rq.cov == SmallCov::Stationary, sgrad = stationary && F == SmallFlavour::Grad;
  if (stationary) {
    if (rq.kernel_id != SIGP_KERNEL_RBF && rq.kernel_id != SIGP_KERNEL_MATERN52)
      return fail(h, SIGP_BAD_ARG, "%s: kernel_id = %d; the stationary covariances are SIGP_KERNEL_RBF and SIGP_KERNEL_MATERN52", rq.name, rq.kernel_id);
    if (rq.ard != 0 && rq.ard != 1) return fail(h, SIGP_BAD_ARG, "%s: ard must be 0 (one length scale per fit) or 1 (one per feature), got %d", rq.name, rq.ard);
    if (rq.ldell < 1) return fail(h, SIGP_BAD_ARG, "%s: ldell = %lld; ell is [nprob][ldell >= 1]", rq.name, (long long)rq.ldell);
    if (sgrad && !rq.grad) return fail(h, SIGP_BAD_ARG, "%s: grad [nprob][ldg] required", rq.name);
    if (sgrad && rq.ldg < 2) return fail(h, SIGP_BAD_ARG, "%s: ldg = %lld; grad holds (d/d log l, d/d log sn~) per fit: ldg >= 2", rq.name, (long long)rq.ldg);
  }
  if (rows && (!rq.row_mean || !rq.row_var || rq.pitch < h->sm_nmax)) {
    if (hc) return fail(h, SIGP_BAD_ARG, "small_run_hindcast: hc_mean / hc_var [nprob][nstride >= %d] required", h->sm_nmax);
    return fail(h, SIGP_BAD_ARG, "small_run_%s: %s_mean / %s_var [nprob][nstride >= %d] required", cvloo, cvloo, cvloo, h->sm_nmax);
  }
  // the leave-block-out launch picks its own feature chunk: the largest of {the upload's, 16, 8} whose image leaves room for the folds
  int ch = h->sm_ch; long lds = h->sm_lds;
  if (F == SmallFlavour::Cv) {
    ch = small_pick_chunk(h->sm_nmax, h->sm_mmax, F, h->sm_ch);
    lds = SmallLayout{h->sm_nmax, h->sm_mmax, ch ? ch : 8, F}.bytes();
    if (!ch)
      return fail(h, SIGP_BAD_ARG, "small_run_cv: n = %d with m = %d leaves no LDS for the folds' %ld bytes (feature chunk 8: %ld of %ld bytes)", h->sm_nmax, h->sm_mmax,
                  lds - SmallLayout{h->sm_nmax, h->sm_mmax, 8, SmallFlavour::Plain}.bytes(), lds, SM_LDS_MAX);
  }
  // so do the score gradients, whose image adds Bc, gv and (hindcast) the saved band
  // ... and the leave-block-out gradient, whose image has the folds' scratch as well and the band of the adjoint, block + 2 gap wide
  if (F == SmallFlavour::CvGrad) {
    const int64_t window = rq.block > SIGP_CV_SMALL_MAX_WINDOW || rq.gap > SIGP_CV_SMALL_MAX_WINDOW ? SIGP_CV_SMALL_MAX_WINDOW + 1 : rq.block + 2 * rq.gap;
    if (window > SIGP_CV_SMALL_MAX_WINDOW)
      return fail(h, SIGP_BAD_ARG, "small_run_cv_grad: block = %lld, gap = %lld: the window block + 2 gap is at most SIGP_CV_SMALL_MAX_WINDOW = %d", (long long)rq.block, (long long)rq.gap,
                  SIGP_CV_SMALL_MAX_WINDOW);
    ch = small_pick_chunk(h->sm_nmax, h->sm_mmax, F, h->sm_ch, (int)window);
    lds = SmallLayout{h->sm_nmax, h->sm_mmax, ch ? ch : 8, F, (int)window}.bytes();
    if (!ch)
      return fail(h, SIGP_BAD_ARG, "small_run_cv_grad: n = %d with m = %d and window = %d needs %ld bytes of LDS at feature chunk 8; the limit is %ld (every n <= 96 with m <= %d and window <= %d fits)",
                  h->sm_nmax, h->sm_mmax, (int)window, lds, SM_LDS_MAX, SM_MMAX, SIGP_CV_SMALL_MAX_WINDOW);
  } else if (small_is_score_grad(F)) {
    const int lead = hc ? (int)rq.lead : 0;
    ch = small_pick_chunk(h->sm_nmax, h->sm_mmax, F, h->sm_ch, lead);
    lds = SmallLayout{h->sm_nmax, h->sm_mmax, ch ? ch : 8, F, lead}.bytes();
    if (!ch)
      return fail(h, SIGP_BAD_ARG, "small_run_%s_grad: n = %d with m = %d and lead = %d needs %ld bytes of LDS at feature chunk 8; the limit is %ld (every n <= 96 with m <= %d and lead <= %d fits)",
                  hc ? "hindcast" : "loo", h->sm_nmax, h->sm_mmax, lead, lds, SM_LDS_MAX, SM_MMAX, (int)SIGP_HINDCAST_SMALL_MAX_LEAD);
  }
  std::vector<char> cv_checked(cv ? h->sm_sets.size() : 0, 0);
  if (h->sm_mmax > 0 && (!mean || !var || mstride < h->sm_mmax)) return fail(h, SIGP_BAD_ARG, "small_run: mean / var [nprob][mstride >= %d] required", h->sm_mmax);
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<SmallProb> probs((size_t)nprob);
  for (int64_t i = 0; i < nprob; ++i) {
    if (set_index[i] < 0 || set_index[i] >= (int64_t)h->sm_sets.size()) return fail(h, SIGP_BAD_ARG, "small_run: fit %ld names data set %ld of %zu", (long)i, (long)set_index[i], h->sm_sets.size());
    if (!(sn_tilde[i] >= 0) || (!stationary && !std::isfinite(ell[i]))) return fail(h, SIGP_BAD_ARG, "small_run: finite ell and sn_tilde >= 0 required");
    const int n = h->sm_sets[(size_t)set_index[i]].n;
    if (stationary) {
      const int N = h->sm_sets[(size_t)set_index[i]].N, nl = rq.ard ? N : 1;
      if (nl > rq.ldell) return fail(h, SIGP_BAD_ARG, "%s: fit %ld names a data set of N = %d features; ldell = %lld holds fewer scales", rq.name, (long)i, N, (long long)rq.ldell);
      if (sgrad && nl + 1 > rq.ldg)
        return fail(h, SIGP_BAD_ARG, "%s: fit %ld has %d derivatives (%d length scale%s and sn~); ldg = %lld holds fewer", rq.name, (long)i, nl + 1, nl, nl > 1 ? "s" : "", (long long)rq.ldg);
      for (int k = 0; k < nl; ++k) {
        const double l = ell[i * rq.ldell + k];
        if (!(l > 0) || !std::isfinite(l) || !std::isfinite(1.0 / l))
          return fail(h, SIGP_BAD_ARG, "%s: fit %ld: length scale %d is %g; every scale must be finite and > 0 with a finite reciprocal", rq.name, (long)i, k, l);
      }
    }
    if (hc && rq.min_train + rq.lead - 1 > n - 1)
      return fail(h, SIGP_BAD_ARG, "small_run_hindcast: fit %ld names a data set without a scored row (min_train + lead - 1 = %lld > n - 1 = %d)", (long)i,
                  (long long)(rq.min_train + rq.lead - 1), n - 1);
    if (rows && !hc && n < 2) return fail(h, SIGP_BAD_ARG, "small_run_%s: fit %ld names a data set of one point; cross-validation needs n >= 2", cvloo, (long)i);
    if (cv && !cv_checked[(size_t)set_index[i]]) {
      if (const char* why = cv_check_folds(n, rq.block, rq.gap, SIGP_CV_SMALL_MAX_WINDOW))
        return fail(h, SIGP_BAD_ARG, "small_run_cv: fit %ld: %s (block = %lld, gap = %lld, n = %d, SIGP_CV_SMALL_MAX_WINDOW = %d)", (long)i, why, (long long)rq.block, (long long)rq.gap,
                    n, SIGP_CV_SMALL_MAX_WINDOW);
      cv_checked[(size_t)set_index[i]] = 1;
    }
    probs[(size_t)i] = SmallProb{(int)set_index[i], 0, ell[i * rq.ldell], sn_tilde[i]};
  }
  const long ms = std::max<int64_t>(mstride, 1);
  const long ns = rows ? (long)rq.pitch : 0;
  const long ow = small_out_width(F, rq.cov);
  const long ng = sgrad ? (long)rq.ldg : 0;
  const long per = ow + 2 * ms + 2 * ns + ng;
  if (h->cap_sm_probs < nprob) {
    if (h->sm_probs) HIPCHK(h, hipFree(h->sm_probs));
    h->sm_probs = nullptr; h->cap_sm_probs = 0;
    HIPCHK(h, hipMalloc((void**)&h->sm_probs, (size_t)nprob * sizeof(SmallProb)));
    h->cap_sm_probs = nprob;
  }
  int rc;
  if ((rc = ensure(h, &h->sm_out, &h->cap_sm_out, nprob * per))) return rc;
  hipStream_t st = h->slots[0].s_upd;
  HIPCHK(h, hipMemcpyAsync(h->sm_probs, probs.data(), probs.size() * sizeof(SmallProb), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(h->sm_out, 0xff, (size_t)(nprob * per) * sizeof(double), st));   // NaN wherever a set has fewer test points than mstride
  if (stationary && rq.ard) {
    if ((rc = ensure(h, &h->sm_ell, &h->cap_sm_ell, nprob * rq.ldell))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->sm_ell, ell, (size_t)(nprob * rq.ldell) * sizeof(double), hipMemcpyHostToDevice, st));
  }
  double* d_out = h->sm_out;
  double* d_mean = h->sm_out + nprob * ow;
  double* d_var = d_mean + nprob * ms;
  double* d_lmean = d_var + nprob * ms;        // [nprob][ns] each; NaN beyond a set's n (the memset above)
  double* d_lvar = d_lmean + nprob * ns;
  double* d_grad = d_lvar + nprob * ns;        // [nprob][ng]; NaN behind a fit's derivatives
  {
    double fl = 0;
    for (const auto& pb : probs) small_count_flops(fl, h->sm_sets[(size_t)pb.set], rq);
    ProfScope ps(h, st, SIGP_KC_SMALL, fl, 0.0);
    const SmallExtras x{d_lmean, d_lvar, (int)ns, rq.sigma_mode, (int)rq.block, (int)rq.gap, (int)rq.lead, (int)rq.min_train, rq.criterion,
                        make_kparams(stationary ? rq.kernel_id : 0, 1.0, 0.0, 0), stationary && rq.ard ? h->sm_ell : nullptr, (int)rq.ldell, (int)ng, d_grad};
    decltype(&small_launch<256, SmallFlavour::Plain>) launch = nullptr;
    if (stationary) switch (F) {
      case SmallFlavour::Plain: launch = small_launch<256, SmallFlavour::Plain, SmallCov::Stationary>; break;
      case SmallFlavour::Grad: launch = small_launch<256, SmallFlavour::Grad, SmallCov::Stationary>; break;
      case SmallFlavour::Loo: launch = small_launch<256, SmallFlavour::Loo, SmallCov::Stationary>; break;
      case SmallFlavour::Cv: launch = small_launch<256, SmallFlavour::Cv, SmallCov::Stationary>; break;
      case SmallFlavour::Hindcast: launch = small_launch<256, SmallFlavour::Hindcast, SmallCov::Stationary>; break;
      default: return fail(h, SIGP_BAD_ARG, "%s: the score gradients are not built for the stationary covariances", rq.name);
    }
    else switch (F) {
      // four wavefronts per fit at every order; one per fit (orders up to 64) is a measurement switch: on the reference-size grid
      // (48 000 fits, n = 6 .. 45) four wavefronts per fit take 1.02 ms, one wavefront per fit 1.71 ms
      case SmallFlavour::Plain: launch = h->sm_nmax <= 64 && h->opt_small_nt64 ? small_launch<64, SmallFlavour::Plain> : small_launch<256, SmallFlavour::Plain>; break;
      case SmallFlavour::Grad: launch = small_launch<256, SmallFlavour::Grad>; break;
      case SmallFlavour::Loo: launch = small_launch<256, SmallFlavour::Loo>; break;
      case SmallFlavour::Cv: launch = small_launch<256, SmallFlavour::Cv>; break;
      case SmallFlavour::Hindcast: launch = small_launch<256, SmallFlavour::Hindcast>; break;
      case SmallFlavour::LooGrad: launch = small_launch<256, SmallFlavour::LooGrad>; break;
      case SmallFlavour::HindcastGrad: launch = small_launch<256, SmallFlavour::HindcastGrad>; break;
      case SmallFlavour::CvGrad: launch = small_launch<256, SmallFlavour::CvGrad>; break;
    }
    HIPCHK(h, launch(h, st, nprob, lds, ch, d_out, d_mean, d_var, (int)ms, x));
  }
  HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)nprob * ow * sizeof(double), hipMemcpyDeviceToHost, st));
  if (h->sm_mmax > 0) {
    // device rows have pitch ms; the caller's have pitch mstride (== ms whenever mstride >= 1)
    HIPCHK(h, hipMemcpyAsync(mean, d_mean, (size_t)nprob * ms * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(var, d_var, (size_t)nprob * ms * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (rows) {
    // tens of MB for a retro grid: through pinned memory of the handle's own (a pageable destination of that size makes the
    // runtime pin and unpin the caller's pages: 25 ms around a 1 ms launch), then one host copy into the caller's arrays
    const long tot = 2 * nprob * ns;
    if (h->cap_sm_loo_host < tot) {
      if (h->sm_loo_host) HIPCHK(h, hipHostFree(h->sm_loo_host));
      h->sm_loo_host = nullptr; h->cap_sm_loo_host = 0;
      HIPCHK(h, hipHostMalloc((void**)&h->sm_loo_host, (size_t)tot * sizeof(double)));
      h->cap_sm_loo_host = tot;
    }
    HIPCHK(h, hipMemcpyAsync(h->sm_loo_host, d_lmean, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (sgrad) HIPCHK(h, hipMemcpyAsync(rq.grad, d_grad, (size_t)nprob * ng * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (rows) {
    memcpy(rq.row_mean, h->sm_loo_host, (size_t)nprob * ns * sizeof(double));
    memcpy(rq.row_var, h->sm_loo_host + nprob * ns, (size_t)nprob * ns * sizeof(double));
  }
  return SIGP_OK;
}

int sigp_small_run(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, double* out,
                   double* mean, double* var, int64_t mstride) {
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out, mean, var, mstride, SmallRequest{});
}

int sigp_small_run_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, double* out8,
                        double* mean, double* var, int64_t mstride) {
  SmallRequest rq;
  rq.flavour = SmallFlavour::Grad;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out8, mean, var, mstride, rq);
}

// sigp_small_run with the leave-one-out cross-validation of every fit in the same single launch (SmallFlavour::Loo)
int sigp_small_run_loo(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int sigma_mode,
                       double* out6, double* mean, double* var, int64_t mstride, double* loo_mean, double* loo_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_loo: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  SmallRequest rq;
  rq.flavour = SmallFlavour::Loo; rq.sigma_mode = sigma_mode;
  rq.row_mean = loo_mean; rq.row_var = loo_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

// sigp_small_run with the leave-block-out cross-validation of every fit in the same single launch (SmallFlavour::Cv)
int sigp_small_run_cv(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t block, int64_t gap, int sigma_mode,
                      double* out6, double* mean, double* var, int64_t mstride, double* cv_mean, double* cv_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_cv: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (block < 1 || gap < 0) return fail(h, SIGP_BAD_ARG, "small_run_cv: block >= 1 and gap >= 0 required");
  SmallRequest rq;
  rq.flavour = SmallFlavour::Cv; rq.sigma_mode = sigma_mode; rq.block = block; rq.gap = gap;
  rq.row_mean = cv_mean; rq.row_var = cv_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

// sigp_small_run with the expanding-window hindcast validation of every fit in the same single launch (SmallFlavour::Hindcast:
// L~ and z are read where the factorisation left them in LDS; no inverse is formed)
int sigp_small_run_hindcast(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t lead, int64_t min_train,
                            int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* hc_mean, double* hc_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_hindcast: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (lead < 1 || lead > SIGP_HINDCAST_SMALL_MAX_LEAD) return fail(h, SIGP_BAD_ARG, "small_run_hindcast: 1 <= lead <= %d required (got %lld)", (int)SIGP_HINDCAST_SMALL_MAX_LEAD, (long long)lead);
  if (min_train < 1) return fail(h, SIGP_BAD_ARG, "small_run_hindcast: min_train >= 1 required (got %lld)", (long long)min_train);
  SmallRequest rq;
  rq.flavour = SmallFlavour::Hindcast; rq.sigma_mode = sigma_mode; rq.lead = lead; rq.min_train = min_train;
  rq.row_mean = hc_mean; rq.row_var = hc_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

// sigp_small_run_loo, then the derivatives of one of its two scores w.r.t. (log l, log sn~) in the same single launch (SmallFlavour::LooGrad)
int sigp_small_run_loo_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int sigma_mode, int criterion,
                            double* out8, double* mean, double* var, int64_t mstride, double* loo_mean, double* loo_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_loo_grad: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "small_run_loo_grad: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  SmallRequest rq;
  rq.flavour = SmallFlavour::LooGrad; rq.sigma_mode = sigma_mode; rq.criterion = criterion;
  rq.row_mean = loo_mean; rq.row_var = loo_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out8, mean, var, mstride, rq);
}

// sigp_small_run_hindcast, then the derivatives of one of its two scores in the same single launch (SmallFlavour::HindcastGrad: the band of L~ the
// adjoint reads is saved in LDS, then L~^-1 is formed over L~)
int sigp_small_run_hindcast_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t lead, int64_t min_train,
                                 int sigma_mode, int criterion, double* out8, double* mean, double* var, int64_t mstride, double* hc_mean, double* hc_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_hindcast_grad: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "small_run_hindcast_grad: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  if (lead < 1 || lead > SIGP_HINDCAST_SMALL_MAX_LEAD) return fail(h, SIGP_BAD_ARG, "small_run_hindcast_grad: 1 <= lead <= %d required (got %lld)", (int)SIGP_HINDCAST_SMALL_MAX_LEAD, (long long)lead);
  if (min_train < 1) return fail(h, SIGP_BAD_ARG, "small_run_hindcast_grad: min_train >= 1 required (got %lld)", (long long)min_train);
  SmallRequest rq;
  rq.flavour = SmallFlavour::HindcastGrad; rq.sigma_mode = sigma_mode; rq.criterion = criterion; rq.lead = lead; rq.min_train = min_train;
  rq.row_mean = hc_mean; rq.row_var = hc_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out8, mean, var, mstride, rq);
}

// sigp_small_run_cv, then the derivatives of one of its two scores in the same single launch (SmallFlavour::CvGrad: the adjoint of cvard.hpp fold by fold,
// its B kept as a band in LDS)
int sigp_small_run_cv_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, const double* ell, const double* sn_tilde, int64_t block, int64_t gap, int sigma_mode,
                           int criterion, double* out8, double* mean, double* var, int64_t mstride, double* cv_mean, double* cv_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_cv_grad: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "small_run_cv_grad: criterion must be SIGP_LOO_NLPD or SIGP_LOO_SSE");
  if (block < 1 || gap < 0) return fail(h, SIGP_BAD_ARG, "small_run_cv_grad: block >= 1 and gap >= 0 required");
  SmallRequest rq;
  rq.flavour = SmallFlavour::CvGrad; rq.sigma_mode = sigma_mode; rq.criterion = criterion; rq.block = block; rq.gap = gap;
  rq.row_mean = cv_mean; rq.row_var = cv_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out8, mean, var, mstride, rq);
}

// ---- the same kernel with an RBF / Matern-5/2 covariance of the sets' raw rows, one length scale per fit or one per feature (SmallCov::Stationary) --------
static SmallRequest small_k_request(const char* name, SmallFlavour f, int kernel_id, int64_t ldell, int ard) {
  SmallRequest rq;
  rq.name = name; rq.flavour = f; rq.cov = SmallCov::Stationary; rq.kernel_id = kernel_id; rq.ldell = ldell; rq.ard = ard;
  return rq;
}

int sigp_small_run_k(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard, const double* sn_tilde,
                     double* out4, double* mean, double* var, int64_t mstride) {
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out4, mean, var, mstride, small_k_request("small_run_k", SmallFlavour::Plain, kernel_id, ldell, ard));
}

// sigp_small_run_k, then the exact gradient of the profiled nlML in every length scale and sn~ in the same single launch
int sigp_small_run_k_grad(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard, const double* sn_tilde,
                          double* out4, double* mean, double* var, int64_t mstride, double* grad, int64_t ldg) {
  SmallRequest rq = small_k_request("small_run_k_grad", SmallFlavour::Grad, kernel_id, ldell, ard);
  rq.grad = grad; rq.ldg = ldg;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out4, mean, var, mstride, rq);
}

int sigp_small_run_k_loo(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard, const double* sn_tilde,
                         int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* loo_mean, double* loo_var, int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_k_loo: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  SmallRequest rq = small_k_request("small_run_k_loo", SmallFlavour::Loo, kernel_id, ldell, ard);
  rq.sigma_mode = sigma_mode;
  rq.row_mean = loo_mean; rq.row_var = loo_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

int sigp_small_run_k_cv(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard, const double* sn_tilde,
                        int64_t block, int64_t gap, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* cv_mean, double* cv_var,
                        int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_k_cv: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (block < 1 || gap < 0) return fail(h, SIGP_BAD_ARG, "small_run_k_cv: block >= 1 and gap >= 0 required");
  SmallRequest rq = small_k_request("small_run_k_cv", SmallFlavour::Cv, kernel_id, ldell, ard);
  rq.sigma_mode = sigma_mode; rq.block = block; rq.gap = gap;
  rq.row_mean = cv_mean; rq.row_var = cv_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

int sigp_small_run_k_hindcast(sigp_handle* h, int64_t nprob, const int64_t* set_index, int kernel_id, const double* ell, int64_t ldell, int ard, const double* sn_tilde,
                              int64_t lead, int64_t min_train, int sigma_mode, double* out6, double* mean, double* var, int64_t mstride, double* hc_mean, double* hc_var,
                              int64_t nstride) {
  if (sigma_mode != SIGP_LOO_REFIT && sigma_mode != SIGP_LOO_FIXED) return fail(h, SIGP_BAD_ARG, "small_run_k_hindcast: sigma_mode must be SIGP_LOO_REFIT or SIGP_LOO_FIXED");
  if (lead < 1 || lead > SIGP_HINDCAST_SMALL_MAX_LEAD) return fail(h, SIGP_BAD_ARG, "small_run_k_hindcast: 1 <= lead <= %d required (got %lld)", (int)SIGP_HINDCAST_SMALL_MAX_LEAD, (long long)lead);
  if (min_train < 1) return fail(h, SIGP_BAD_ARG, "small_run_k_hindcast: min_train >= 1 required (got %lld)", (long long)min_train);
  SmallRequest rq = small_k_request("small_run_k_hindcast", SmallFlavour::Hindcast, kernel_id, ldell, ard);
  rq.sigma_mode = sigma_mode; rq.lead = lead; rq.min_train = min_train;
  rq.row_mean = hc_mean; rq.row_var = hc_var; rq.pitch = nstride;
  return small_run_impl(h, nprob, set_index, ell, sn_tilde, out6, mean, var, mstride, rq);
}

// ---- ComplexNetworks tau(): cell-to-cell correlation matrix + thresholded mean (ComplexNetworks.py:31-47) ------------
int sigp_corr_tau(sigp_handle* h, const double* series, int64_t N, int64_t T, int64_t lds, double r_crit, double* R, int64_t ldr,
                  double* sum_out, double* count_out) {
  if (!h || !series || N < 2 || T < 3 || lds < T || !sum_out || !count_out || (R && ldr < N)) return fail(h, SIGP_BAD_ARG, "corr_tau: bad argument");
  if (N > 46000) return fail(h, SIGP_BAD_ARG, "corr_tau: more than 46000 cells not supported (tile index range)");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->slots[0].s_upd;
  const long n_pad = round_up(N, 64), k_pad = round_up(T, 16);
  int rc;
  // workspaces: raw series | Z | R | partial sums, carved out of the gradient buffers (n x n class)
  if ((rc = ensure(h, &h->stage, &h->cap_stage, N * lds))) return rc;
  if ((rc = ensure(h, &h->gD, &h->cap_gD, n_pad * k_pad))) return rc;
  if ((rc = ensure(h, &h->gK, &h->cap_gK, n_pad * n_pad))) return rc;
  if ((rc = ensure(h, &h->gPart, &h->cap_gPart, 2 * n_pad))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->stage, series, (size_t)((N - 1) * lds + T) * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(corr_standardise_kernel, dim3((unsigned)((n_pad + 127) / 128)), dim3(128), 0, st, (const double*)h->stage, (long)lds, (int)N, (int)T, h->gD, (int)n_pad,
                     (int)k_pad);
  HIPCHK(h, hipGetLastError());
  {
    GemmArgs g{};                                         // R = Z Z^T, all 64x64 tiles (area_level reads the full symmetric matrix)
    g.A = h->gD; g.lda = k_pad; g.B = h->gD; g.ldb = k_pad; g.C = h->gK; g.ldc = n_pad; g.K = (int)k_pad;
    g.r0 = 0; g.r1 = (int)(n_pad / 64); g.c0 = 0; g.c1 = (int)(n_pad / 64); g.lower = 0;
    ProfScope ps(h, st, SIGP_KC_KBUILD, 2.0 * N * N * T, 8.0 * N * N);
    if ((rc = launch_gemm_cfg<64, 64, 2, 2, GEMM_SET, false>(h, st, g))) return rc;
  }
  hipLaunchKernelGGL(corr_threshold_kernel, dim3((unsigned)N), dim3(256), 0, st, h->gK, n_pad, (int)N, r_crit, h->gPart);
  HIPCHK(h, hipGetLastError());
  std::vector<double> part((size_t)2 * N);
  HIPCHK(h, hipMemcpyAsync(part.data(), h->gPart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (R) HIPCHK(h, hipMemcpy2DAsync(R, (size_t)ldr * sizeof(double), h->gK, (size_t)n_pad * sizeof(double), (size_t)N * sizeof(double), (size_t)N, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  double s = 0, c = 0;
  for (int64_t i = 0; i < N; ++i) { s += part[2 * i]; c += part[2 * i + 1]; }
  *sum_out = s; *count_out = c;
  return SIGP_OK;
}

// ---- intra_links(): the per-area anomaly series that become the GP's features ----------------------------------------------
int sigp_area_sums(sigp_handle* h, const double* data, int64_t P, int64_t T, const double* weight, const int32_t* label, int64_t A, double* out) {
  if (!h || !data || !weight || !label || !out || P < 1 || T < 1 || A < 1) return fail(h, SIGP_BAD_ARG, "area_sums: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->slots[0].s_upd;
  int rc;
  const long lab_dbl = (P + 1) / 2;                                  // int32 labels, in doubles
  if ((rc = ensure(h, &h->stage, &h->cap_stage, P * T + P + lab_dbl + A * T))) return rc;
  double* d_data = h->stage; double* d_w = d_data + P * T; int* d_lab = (int*)(d_w + P); double* d_out = d_w + P + lab_dbl;
  HIPCHK(h, hipMemcpyAsync(d_data, data, (size_t)(P * T) * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_w, weight, (size_t)P * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_lab, label, (size_t)P * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(area_sums_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)A), dim3(64), 0, st, (const double*)d_data, (const double*)d_w, (const int*)d_lab, (int)P,
                     (int)T, (int)A, d_out);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)(A * T) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return SIGP_OK;
}

// ---- detrend(): per-pixel least-squares line removal for every cut-off year in one launch --------------------------------
int sigp_detrend(sigp_handle* h, const double* data, int64_t P, int64_t T, int64_t ncuts, const int64_t* cut_len, double* dt_out, double* trend_out) {
  if (!h || !data || P < 1 || T < 2 || ncuts < 1 || !cut_len || !dt_out || !trend_out) return fail(h, SIGP_BAD_ARG, "detrend: bad argument");
  std::vector<int> nc((size_t)ncuts);
  std::vector<long> off((size_t)ncuts);
  long tot = 0;
  for (int64_t c = 0; c < ncuts; ++c) {
    if (cut_len[c] < 2 || cut_len[c] > T) return fail(h, SIGP_BAD_ARG, "detrend: cut %ld uses %ld of %ld time steps", (long)c, (long)cut_len[c], (long)T);
    nc[(size_t)c] = (int)cut_len[c]; off[(size_t)c] = tot; tot += P * cut_len[c];
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->slots[0].s_upd;
  int rc;
  const long hdr = round_up(ncuts * 2, 8);                       // cut lengths (int) + offsets (long), in doubles
  if ((rc = ensure(h, &h->stage, &h->cap_stage, P * T + hdr + 8))) return rc;
  if ((rc = ensure(h, &h->gD, &h->cap_gD, tot + ncuts * P * 2))) return rc;
  double* d_data = h->stage;
  long* d_off = (long*)(h->stage + P * T);
  int* d_nc = (int*)(d_off + ncuts);
  double* d_dt = h->gD;
  double* d_tr = h->gD + tot;
  HIPCHK(h, hipMemcpyAsync(d_data, data, (size_t)(P * T) * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_off, off.data(), (size_t)ncuts * sizeof(long), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_nc, nc.data(), (size_t)ncuts * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(detrend_kernel, dim3((unsigned)((P + 127) / 128), (unsigned)ncuts), dim3(128), 0, st, (const double*)d_data, (int)P, (int)T, (const int*)d_nc,
                     (const long*)d_off, (int)ncuts, d_dt, d_tr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(dt_out, d_dt, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(trend_out, d_tr, (size_t)(ncuts * P * 2) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return SIGP_OK;
}

