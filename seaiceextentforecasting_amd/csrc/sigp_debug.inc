// Micro-benchmark / diagnostic entry points (include/sigp_debug.h).  Compiled ONLY into libsigp_debug.so
// (make debug: -DSIGP_DEBUG_TOOLS); the product library libsigp.so contains none of this.
// Included from sigp.hip inside its extern "C" block.
// fp64 MFMA issue-rate probe: nothing but v_mfma_f64_16x16x4_f64 on 16 independent accumulators per wave
__global__ __launch_bounds__(256, 2) void mfma_peak_kernel(double* out, int iters, double seed) {
  sigp::d4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = sigp::d4{0.0, 0.0, 0.0, 0.0};
  double a[8], b[8];
  unsigned long long x = 88172645463325252ull + threadIdx.x * 2654435761ull + blockIdx.x * 97ull;
#pragma unroll
  for (int i = 0; i < 8; ++i) {   // seed < 0: full-range pseudo-random operands (data toggling); else constants
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    a[i] = seed < 0 ? (double)(long long)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5 : seed + threadIdx.x * 1e-3;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    b[i] = seed < 0 ? (double)(long long)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5 : seed - threadIdx.x * 1e-3;
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i & 7], b[(i + (i >> 3)) & 7], acc[i], 0, 0, 0);
  }
  double s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

__global__ void whereami_kernel(unsigned* out) {
  // hold the CU for a while so that blocks spread over every CU the mask allows
  long long t0 = clock64();
  while (clock64() - t0 < 200000) {}
  if (threadIdx.x == 0) {
    unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));   // HW_REG_XCC_ID, 32 bits
    unsigned hwid = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
    out[2 * blockIdx.x] = xcc;
    out[2 * blockIdx.x + 1] = hwid;
  }
}

// ---- debug / micro-benchmark entry points (not part of the product ABI; see tools/) -------------------
int sigp_debug_time_diag(sigp_handle* h, const double* A128, int skip, int reps, double* ms_avg, double* L_out, double* Linv_out) {
  if (!h || !A128 || reps < 1 || reps > 4096) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  // `reps` copies of the block are factored by `reps` back-to-back launches between two events (a lone 60 us launch on
  // an idle GPU is timed at whatever clock the chip idles at); 20 untimed launches first
  double *a0, *a1, *li; int* info;
  HIPCHK(h, hipMalloc((void**)&a0, NB * NB * 8)); HIPCHK(h, hipMalloc((void**)&a1, (size_t)reps * NB * NB * 8));
  HIPCHK(h, hipMalloc((void**)&li, NB * NB * 8)); HIPCHK(h, hipMalloc((void**)&info, 4));
  HIPCHK(h, hipMemset(li, 0, NB * NB * 8));
  HIPCHK(h, hipMemcpy(a0, A128, NB * NB * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemset(info, 0, 4));
  HIPCHK(h, hipFuncSetAttribute((const void*)potrf_diag_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, DIAG_LDS_BYTES));
  hipStream_t st = h->slots[0].s_upd;
  hipEvent_t e0, e1; HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
  float ms = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int r = 0; r < reps; ++r) HIPCHK(h, hipMemcpyAsync(a1 + (size_t)r * NB * NB, a0, NB * NB * 8, hipMemcpyDeviceToDevice, st));
    const int n = pass == 0 ? std::min(reps, 20) : reps;
    HIPCHK(h, hipEventRecord(e0, st));
    for (int r = 0; r < n; ++r)
      hipLaunchKernelGGL(potrf_diag_kernel<double>, dim3(1), dim3(DIAG_THREADS), DIAG_LDS_BYTES, st, a1 + (size_t)r * NB * NB, (long)NB, li, info, 0, skip, 0L, 0L);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
  }
  if (ms_avg) *ms_avg = ms / reps;
  if (L_out) HIPCHK(h, hipMemcpy(L_out, a1, NB * NB * 8, hipMemcpyDeviceToHost));
  if (Linv_out) HIPCHK(h, hipMemcpy(Linv_out, li, NB * NB * 8, hipMemcpyDeviceToHost));
  (void)hipFree(a0); (void)hipFree(a1); (void)hipFree(li); (void)hipFree(info);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return SIGP_OK;
}

// phase stamps of ONE potrf_diag_kernel launch (flags bit 64): out_us[k] = microseconds since the kernel's first instruction, k as DIAG_STAMP's
int sigp_debug_diag_stamps(sigp_handle* h, const double* A128, double* out_us, int nout) {
  if (!h || !A128 || !out_us || nout < 1 || nout > 64 + 192) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  double *a0, *li; int* info;
  HIPCHK(h, hipMalloc((void**)&a0, NB * NB * 8)); HIPCHK(h, hipMalloc((void**)&li, NB * NB * 8)); HIPCHK(h, hipMalloc((void**)&info, 4));
  HIPCHK(h, hipMemset(li, 0, NB * NB * 8)); HIPCHK(h, hipMemset(info, 0, 4));
  HIPCHK(h, hipFuncSetAttribute((const void*)potrf_diag_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, DIAG_LDS_BYTES));
  hipStream_t st = h->slots[0].s_upd;
  unsigned long long z[64] = {0}, zr[192] = {0};
  const int nl = nout > 56 ? 400 : 5;  // nout > 50: the last of 400 back-to-back launches (the chip's clock under a chain of such kernels)
  for (int r = 0; r < nl; ++r) {       // the last launch is the one read (warm instruction cache)
    HIPCHK(h, hipMemcpyAsync(a0, A128, NB * NB * 8, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_diag_stamp), z, sizeof z, 0, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_diag_stamp_role), zr, sizeof zr, 0, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(potrf_diag_kernel<double>, dim3(1), dim3(DIAG_THREADS), DIAG_LDS_BYTES, st, a0, (long)NB, li, info, 0, 64, 0L, 0L);
    HIPCHK(h, hipGetLastError());
    if (nl == 5) HIPCHK(h, hipStreamSynchronize(st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpyFromSymbol(z, HIP_SYMBOL(g_diag_stamp), sizeof z));
  HIPCHK(h, hipMemcpyFromSymbol(zr, HIP_SYMBOL(g_diag_stamp_role), sizeof zr));
  for (int k = 64; k < nout; ++k) out_us[k] = zr[k - 64] ? (double)(zr[k - 64] - z[0]) * 0.01 : -1.0;
  for (int k = 0; k < std::min(nout, 48); ++k) out_us[k] = z[k] ? (double)(z[k] - z[0]) * 0.01 : -1.0;     // s_memrealtime: 100 MHz
  for (int k = 50; k < std::min(nout, 54); ++k) out_us[k] = z[k] ? (double)(z[k] - z[0]) * 0.01 : -1.0;
  if (nout > 48) out_us[48] = (double)(z[49] - z[48]) / ((double)(z[44] - z[0]) * 0.01) * 1e-3;            // shader clock in GHz over the kernel body (s_memtime cycles / us)
  (void)hipFree(a0); (void)hipFree(li); (void)hipFree(info);
  return SIGP_OK;
}

// time kbuild_kernel for nb lockstep members of order n (flags: 2 no covariance function, 4 no store)
int sigp_debug_time_kbuild(sigp_handle* h, int n, int d, int nb, int kernel_id, int flags, int reps, double* ms_avg) {
  if (!h || n < 128 || n % 128 || d < 1 || d > 64 || nb < 1 || reps < 1) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const long dp = round_up(d, 8), ld = n;
  double *X, *Mat; KParams* kps;
  HIPCHK(h, hipMalloc((void**)&X, (size_t)n * dp * 8)); HIPCHK(h, hipMalloc((void**)&Mat, (size_t)nb * n * n * 8));
  HIPCHK(h, hipMalloc((void**)&kps, (size_t)nb * sizeof(KParams)));
  std::vector<double> hx((size_t)n * dp, 0.0);
  for (long i = 0; i < n; ++i) for (int p = 0; p < d; ++p) hx[i * dp + p] = 1e-3 * (double)(((i * dp + p) * 2654435761u) % 4000) - 2.0;
  HIPCHK(h, hipMemcpy(X, hx.data(), hx.size() * 8, hipMemcpyHostToDevice));
  std::vector<KParams> hk((size_t)nb, make_kparams(kernel_id, std::sqrt((double)d), 1e-2, 0));
  HIPCHK(h, hipMemcpy(kps, hk.data(), hk.size() * sizeof(KParams), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_upd;
  hipEvent_t e0, e1; HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
  double tot = 0;
  for (int r = 0; r < reps + 2; ++r) {
    HIPCHK(h, hipEventRecord(e0, st));
    launch_kbuild<double>(h, dim3((unsigned)kbuild_tiles(n), 1, (unsigned)nb), st, X, 0L, (int)dp, d, n, Mat, (long)n * n, ld, kps, flags & ~1);   // (option kbuild_mfma picks the kernel)
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    float ms; HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) tot += ms;
  }
  if (ms_avg) *ms_avg = tot / reps;
  (void)hipFree(X); (void)hipFree(Mat); (void)hipFree(kps); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return SIGP_OK;
}

int sigp_debug_mfma_peak(sigp_handle* h, int blocks, int iters, double* tflops, double seed) {
  if (!h || blocks < 1 || iters < 1) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  double* out; HIPCHK(h, hipMalloc((void**)&out, (size_t)blocks * 256 * 8));
  hipStream_t st = h->slots[0].s_pan;
  hipEvent_t e0, e1; HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
  float best = 1e30f;
  for (int r = 0; r < 5; ++r) {
    HIPCHK(h, hipEventRecord(e0, st));
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, st, out, iters, seed);
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    float ms; HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    if (r > 0 && ms < best) best = ms;
  }
  if (tflops) *tflops = (double)blocks * 4 * iters * 16 * 2048.0 / (best * 1e-3) / 1e12;
  (void)hipFree(out); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return SIGP_OK;
}

// time the lower-tile update C -= P P^T (128x128 tiles) on a synthetic (rt*128) x K panel, tile walk `patch`
}  // extern "C" (templates need C++ linkage)

template <typename Real>
static int debug_time_syrk_t(sigp_handle* h, int rt, int K, int patch, int small, int reps, double* ms_avg, double* tflops, int dbg, double* clock_ghz) {
  if (!h || rt < 1 || K < 16 || reps < 1) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  // SIGP_DEBUG_LDPAD = elements added to both row strides (0: the panel is compact, row stride K -- a power of two, like n_pad in a fit)
  const long pad = getenv("SIGP_DEBUG_LDPAD") ? atol(getenv("SIGP_DEBUG_LDPAD")) : 0;
  const long n = (long)rt * NB, ldp = K + pad, ldc = n + pad;
  Real *P, *Cm;
  HIPCHK(h, hipMalloc((void**)&P, (size_t)n * ldp * sizeof(Real))); HIPCHK(h, hipMalloc((void**)&Cm, (size_t)n * ldc * sizeof(Real)));
  HIPCHK(h, hipMemset(Cm, 0, (size_t)n * ldc * sizeof(Real)));
  std::vector<Real> hp((size_t)n * ldp);
  for (size_t i = 0; i < hp.size(); ++i) hp[i] = (Real)(1e-3 * (double)((i * 2654435761u) % 1000) - 0.5);
  HIPCHK(h, hipMemcpy(P, hp.data(), hp.size() * sizeof(Real), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_pan;
  hipEvent_t e0, e1; HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
  GemmArgsT<Real> g{};
  g.A = P; g.lda = ldp; g.B = P; g.ldb = ldp; g.C = Cm; g.ldc = ldc; g.K = K; g.r0 = 0; g.r1 = rt; g.c0 = 0; g.c1 = rt; g.lower = 1; g.patch = patch; g.dbg = dbg;
  unsigned long long* stamp = nullptr;
  const int ngrid = gemm_grid_size(0, rt, 0, rt, 1, patch);
  if (clock_ghz && small == 2) { HIPCHK(h, hipMalloc((void**)&stamp, (size_t)ngrid * 104)); HIPCHK(h, hipMemset(stamp, 0, (size_t)ngrid * 104)); g.stamp = stamp; }   // 5 + 8 (timeline) words per tile
  if (small == 1) { g.r1 *= 2; g.c1 *= 2; }
  double tot = 0;
  for (int r = 0; r < reps + 2; ++r) {
    HIPCHK(h, hipEventRecord(e0, st));
    int rc = small == 1 ? launch_gemm_cfg<Real, 64, 64, 2, 2, GEMM_SUB, false>(h, st, g) : small == 2 ? launch_syrk128_t<Real, false>(h, st, g) : launch_gemm_cfg<Real, 128, 128, 2, 2, GEMM_SUB, false>(h, st, g);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    float ms; HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) tot += ms;
  }
  if (stamp) {
    std::vector<unsigned long long> hs((size_t)ngrid * 5);
    HIPCHK(h, hipMemcpy(hs.data(), stamp, hs.size() * 8, hipMemcpyDeviceToHost));
    if (dbg & 256) {
      // full tiles only: in the plain lower walk every column of the tile space starts with its diagonal tile (the shorter DG form)
      std::vector<char> is_diag((size_t)ngrid, 0);
      if (patch == 0) { size_t i = 0; for (int bj = 0; bj < rt; ++bj) { is_diag[i] = 1; i += (size_t)(rt - bj); } }
      double p0 = 0, p1 = 0, p2 = 0; int nfull = 0;
      for (int i = 0; i < ngrid; ++i) {
        if (is_diag[i] && ngrid > rt) continue;
        p0 += (double)hs[2 * (size_t)ngrid + 3 * i]; p1 += (double)hs[2 * (size_t)ngrid + 3 * i + 1]; p2 += (double)hs[2 * (size_t)ngrid + 3 * i + 2]; ++nfull;
      }
      fprintf(stderr, "[syrk phases] cycles per tile (wave 0): prologue %.0f  K loop %.0f  epilogue %.0f  (per K-slice %.0f)\n", p0 / nfull, p1 / nfull, p2 / nfull,
              p1 / nfull / (K / Num<Real>::KT));
    }
    double sc = 0, sr = 0;
    for (int i = 0; i < ngrid; ++i) { sc += (double)hs[2 * i]; sr += (double)(hs[2 * i + 1] >> 8); }
    if (dbg & 32) { fprintf(stderr, "[xcc by block]"); for (int i = 0; i < std::min(ngrid, 96); ++i) fprintf(stderr, " %d", (int)(hs[2 * i + 1] & 0xf)); fprintf(stderr, "\n"); }
    *clock_ghz = sr > 0 ? sc / (sr * 10.0) : 0.0;   // s_memrealtime ticks at 100 MHz
    if (dbg & 256) {
      // turnaround: what a slot spends per tile OUTSIDE the stamped body (dispatch or walk step, kernarg loads, retirement) =
      // launch time x clock / tiles per slot - stamped cycles per tile (which, under dbg 256, include the wait for the C stores)
      const double slots = (double)h->ncu * ((dbg & 1024) ? 1 : 2), per_slot = tot / reps * 1e-3 * *clock_ghz * 1e9 * slots / ngrid;
      fprintf(stderr, "[syrk turnaround] %s%s launch cycles per tile and slot %.0f  stamped body %.0f  turnaround %.0f\n", (dbg & 1024) ? "1 wg/CU " : "2 wg/CU ",
              (dbg & 2048) ? "persistent" : "one tile per wg", per_slot, sc / ngrid, per_slot - sc / ngrid);
    }
    if ((dbg & 4096) && (dbg & 256) && *clock_ghz > 0) {
      // timeline of the last launch (dbg 4096): per CU, how much of the steady state -- from the moment every slot has been filled once to the
      // last tile's start -- has 2 / 1 / 0 workgroups inside their stamped body, and inside their K loop; what is left is ramp and tail
      std::vector<unsigned long long> tl((size_t)ngrid * 8);
      HIPCHK(h, hipMemcpy(tl.data(), stamp + 5 * (size_t)ngrid, tl.size() * 8, hipMemcpyDeviceToHost));
      const int slots_cu = (dbg & 1024) ? 1 : 2, slots = h->ncu * slots_cu;
      std::vector<double> starts((size_t)ngrid);
      double t_first = 1e300, t_end = 0, lag = 0;
      for (int i = 0; i < ngrid; ++i) {
        starts[i] = (double)tl[8 * (size_t)i + 1];
        double em = 0; for (int w = 0; w < 4; ++w) em = std::max(em, (double)tl[8 * (size_t)i + 2 + w]);
        t_first = std::min(t_first, starts[i]); t_end = std::max(t_end, em); lag += em - (double)tl[8 * (size_t)i + 2];
      }
      std::vector<double> ss = starts; std::sort(ss.begin(), ss.end());
      if (ngrid > 2 * slots) {
        const double w0 = ss[slots - 1], w1 = ss[ngrid - 1];
        struct Ev { double t; int dres, dloop; };
        std::map<unsigned, std::vector<Ev>> per_cu;
        int started = 0;
        for (int i = 0; i < ngrid; ++i) {
          const double s0 = starts[i], e0 = (double)tl[8 * (size_t)i + 2], cyc = (double)hs[2 * (size_t)i];
          double em = 0; for (int w = 0; w < 4; ++w) em = std::max(em, (double)tl[8 * (size_t)i + 2 + w]);
          const double tpc = cyc > 0 ? (e0 - s0) / cyc : 0.0;      // ticks per cycle of this body
          const double l0 = s0 + (double)hs[2 * (size_t)ngrid + 3 * i] * tpc, l1 = l0 + (double)hs[2 * (size_t)ngrid + 3 * i + 1] * tpc;
          auto& v = per_cu[(unsigned)tl[8 * (size_t)i]];
          v.push_back({s0, 1, 0}); v.push_back({em, -1, 0}); v.push_back({l0, 0, 1}); v.push_back({l1, 0, -1});
          started += s0 > w0 && s0 <= w1;
        }
        double R[4] = {0, 0, 0, 0}, Lp[4] = {0, 0, 0, 0};
        for (auto& kv : per_cu) {
          auto& v = kv.second;
          std::sort(v.begin(), v.end(), [](const Ev& a, const Ev& b) { return a.t < b.t; });
          int res = 0, lp = 0; double tprev = w0;
          for (const Ev& e : v) {
            const double tc = std::min(std::max(e.t, w0), w1);
            R[std::min(std::max(res, 0), 3)] += tc - tprev; Lp[std::min(std::max(lp, 0), 3)] += tc - tprev; tprev = tc;
            res += e.dres; lp += e.dloop;
          }
          R[std::min(std::max(res, 0), 3)] += w1 - tprev; Lp[std::min(std::max(lp, 0), 3)] += w1 - tprev;
        }
        const double all = (w1 - w0) * (double)per_cu.size(), tick_cyc = *clock_ghz * 10.0;
        const double mean_res = (R[1] + 2 * R[2] + 3 * R[3]) / all;
        fprintf(stderr, "[syrk timeline] %d CUs seen; launch %.1f us = ramp %.1f + steady %.1f + tail %.1f (stamped), event-timed %.1f us\n", (int)per_cu.size(),
                (t_end - t_first) * 0.01, (w0 - t_first) * 0.01, (w1 - w0) * 0.01, (t_end - w1) * 0.01, tot / reps * 1e3);
        fprintf(stderr, "[syrk timeline] steady state, share of CU time with k workgroups in their body: k=0 %.4f  k=1 %.4f  k=2 %.4f  k>2 %.4f; in their K loop: k=0 %.4f  k=1 %.4f  k=2 %.4f\n",
                R[0] / all, R[1] / all, R[2] / all, R[3] / all, Lp[0] / all, Lp[1] / all, (Lp[2] + Lp[3]) / all);
        fprintf(stderr, "[syrk timeline] slot time outside a body per tile started: %.0f cycles; last wave ends %.0f cycles after wave 0\n",
                started > 0 ? (slots_cu - mean_res) * all / started * tick_cyc : 0.0, lag / ngrid * tick_cyc);
      }
    }
    (void)hipFree(stamp);
  }
  const double nt = (double)rt * (rt + 1) / 2;
  if (ms_avg) *ms_avg = tot / reps;
  if (tflops) *tflops = nt * 2.0 * NB * NB * K / (tot / reps * 1e-3) / 1e12;
  (void)hipFree(P); (void)hipFree(Cm); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return SIGP_OK;
}

extern "C" {

// small: 0 generic 128-tile kernel, 1 generic 64-tile kernel, 2 syrk128_kernel; +16: the fp32 instantiation
int sigp_debug_time_syrk(sigp_handle* h, int rt, int K, int patch, int small, int reps, double* ms_avg, double* tflops, int dbg, double* clock_ghz) {
  if (small & 16) return debug_time_syrk_t<float>(h, rt, K, patch, small & 15, reps, ms_avg, tflops, dbg, clock_ghz);
  return debug_time_syrk_t<double>(h, rt, K, patch, small, reps, ms_avg, tflops, dbg, clock_ghz);
}

// do independent small kernels on different streams of this handle overlap?  returns wall ms for nstreams x reps launches
int sigp_debug_stream_concurrency(sigp_handle* h, int nstreams, int reps, int blocks, int iters, int use_slot_streams, double* ms_out) {
  if (!h || nstreams < 1 || nstreams > 16) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<hipStream_t> st((size_t)nstreams);
  for (int i = 0; i < nstreams; ++i) {
    if (use_slot_streams) {
      int rc = slot_init(h, h->slots[i / 2]);
      if (rc) return rc;
      st[i] = (i & 1) ? h->slots[i / 2].s_pan : h->slots[i / 2].s_upd;
    } else {
      HIPCHK(h, hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    }
  }
  double* out; HIPCHK(h, hipMalloc((void**)&out, (size_t)nstreams * blocks * 256 * 8));
  HIPCHK(h, hipDeviceSynchronize());
  auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < reps; ++r)
    for (int i = 0; i < nstreams; ++i)
      hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, st[i], out + (size_t)i * blocks * 256, iters, 0.25);
  HIPCHK(h, hipDeviceSynchronize());
  if (ms_out) *ms_out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!use_slot_streams) for (auto q : st) (void)hipStreamDestroy(q);
  (void)hipFree(out);
  return SIGP_OK;
}

// which XCC / CU does CU-mask bit `bit` select?  out[0] = XCC_ID reg, out[1] = HW_ID reg of a 1-block kernel
int sigp_debug_cumask_probe(sigp_handle* h, const unsigned* mask8, int blocks, unsigned* out2) {
  if (!h || !mask8 || blocks < 1 || !out2) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st;
  HIPCHK(h, hipExtStreamCreateWithCUMask(&st, 8, mask8));
  unsigned* d; HIPCHK(h, hipMalloc((void**)&d, (size_t)blocks * 8));
  HIPCHK(h, hipMemset(d, 0xff, (size_t)blocks * 8));
  HIPCHK(h, hipDeviceSynchronize());
  hipLaunchKernelGGL(whereami_kernel, dim3(blocks), dim3(64), 0, st, d);
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(out2, d, (size_t)blocks * 8, hipMemcpyDeviceToHost));
  (void)hipFree(d); (void)hipStreamDestroy(st);
  return SIGP_OK;
}

// ---- run-and-return entries: ONE launch of a tile primitive on the caller's operands, through the launcher the engine uses ----------------
// (tests/test_hip_tile_primitives.py).  Every entry works out the largest element each operand can touch from the descriptor and refuses
// (SIGP_BAD_ARG, nothing launched) what would leave the buffers, what is misaligned for the 16-byte staging accesses, and the descriptors
// the kernels do not implement.
}  // extern "C" (templates need C++ linkage)

// the tiles member y owns in a plain-walk launch: what gemm_tile_coords hands out over blockIdx.x < gemm_grid_size (patch = 0)
template <typename F>
static void debug_for_owned_tiles(int r0, int r1, int c0, int c1, int lower, int zshift, int y, F&& f) {
  for (int bj = c0; bj < c1; ++bj) {
    const int lo = lower ? std::max(r0, bj + zshift * y) : r0;
    for (int bi = lo; bi < r1; ++bi) f(bi, bj);
  }
}

struct DebugDeviceBuf {   // freed on every return path
  void* p = nullptr;
  ~DebugDeviceBuf() { if (p) (void)hipFree(p); }
};

enum { DBG_CFG_32x128_SET = 0, DBG_CFG_32x128_SET_BT, DBG_CFG_32x128_SETNEG_BT, DBG_CFG_64x64_SET, DBG_CFG_64x64_SUB, DBG_CFG_64x64_SUB_BT,
       DBG_CFG_128x128_SUB, DBG_CFG_128x128_SETNEG_BT, DBG_CFG_32x32_SUB, DBG_CFG_SYRK128_SUB, DBG_CFG_SYRK128_SET, DBG_CFG_AUTO, DBG_CFG_COUNT };

template <typename Real>
static int debug_run_gemm_t(sigp_handle* h, int cfg, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int K, int r0, int r1, int c0,
                            int c1, int lower, int ktri, int batch, long sA, long sB, long sC, int zcount, long zA, long zB, long zC, int zshift,
                            int ride_bi1, int ride_rows, long a_elems, long b_elems, long c_elems) {
  constexpr int KTe = Num<Real>::KT, NE = Num<Real>::NE;
  constexpr long LIM = 1L << 20;
  static const int tm_of[DBG_CFG_COUNT] = {32, 32, 32, 64, 64, 64, 128, 128, 32, 128, 128, 128};
  static const int tn_of[DBG_CFG_COUNT] = {128, 128, 128, 64, 64, 64, 128, 128, 32, 128, 128, 128};
  if (!h || !A || !C || cfg < 0 || cfg >= DBG_CFG_COUNT) return SIGP_BAD_ARG;
  const bool alias = B == nullptr || B == A;          // one operand: the launch sees the SAME device pointer on both sides
  const bool bt = cfg == DBG_CFG_32x128_SET_BT || cfg == DBG_CFG_32x128_SETNEG_BT || cfg == DBG_CFG_64x64_SUB_BT || cfg == DBG_CFG_128x128_SETNEG_BT;
  const bool syrk = cfg == DBG_CFG_SYRK128_SUB || cfg == DBG_CFG_SYRK128_SET;
  const int TM = tm_of[cfg], TN = tn_of[cfg];
  if (K < KTe || K % KTe || K > LIM) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: K = %d is not a positive multiple of the K-slice %d", K, KTe);
  if (r0 < 0 || c0 < 0 || r1 > 4096 || c1 > 4096 || (lower != 0 && lower != 1)) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: tile window");
  if (batch < 0 || batch > 64 || zcount < 0 || zcount > 64) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: member counts");
  const int nby = std::max(1, batch), nbz = std::max(1, zcount);
  if (lda < 1 || ldb < 1 || ldc < 1 || sA < 0 || sB < 0 || sC < 0 || zA < 0 || zB < 0 || zC < 0 || lda > LIM || ldb > LIM || ldc > LIM ||
      a_elems < 1 || b_elems < (alias ? 0 : 1) || c_elems < 1 || std::max({sA, sB, sC, zA, zB, zC}) > (1L << 40))
    return fail(h, SIGP_BAD_ARG, "debug_run_gemm: strides");
  if (lda % NE || ldb % NE || ldc % NE || sA % NE || sB % NE || sC % NE || zA % NE || zB % NE || zC % NE)
    return fail(h, SIGP_BAD_ARG, "debug_run_gemm: a row or member stride is not a multiple of 16 bytes");
  if ((nby > 1 && sC == 0) || (nbz > 1 && zC == 0)) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: members would write the same tiles");
  if (ktri < 0 || ktri > 2 || (ktri == 2 && (syrk || cfg == DBG_CFG_AUTO || lower)) || (ktri == 1 && cfg == DBG_CFG_AUTO))
    return fail(h, SIGP_BAD_ARG, "debug_run_gemm: ktri = %d is not implemented by this kernel / walk", ktri);
  // zshift moves member blockIdx.y's trapezoid: only the plain lower walk knows it, and only downwards (the grid is sized for member 0)
  if (zshift < 0 || zshift > 4096 || (zshift && (!lower || ktri == 1))) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: zshift needs a lower walk without ktri = 1");
  if (ride_bi1 < 0 || ride_rows < 0 || (ride_bi1 > 0 && (ride_rows < 1 || ride_rows > 16 || ride_bi1 > r1)))
    return fail(h, SIGP_BAD_ARG, "debug_run_gemm: ride row (the RD form multiplies at most 16 rows)");
  bool ok = true;
  const long b_cap = alias ? a_elems : b_elems;
  for (int y = 0; y < nby && ok; ++y)
    for (int z = 0; z < nbz && ok; ++z)
      debug_for_owned_tiles(r0, r1, c0, c1, lower, zshift, y, [&](int bi, int bj) {
        const long ks = ktri == 1 ? (long)bi * TM : 0;
        long span = K - ks;
        if (ktri == 2) span = std::min<long>(span, (long)(bj + 1) * TN);
        if (span < KTe || span % KTe) { ok = false; return; }       // (an empty span still stages one slice in syrk128_kernel)
        const long a_hi = y * sA + z * zA + ((long)bi * TM + TM - 1) * lda + ks + span - 1;
        const long b_hi = y * sB + z * zB + (bt ? (ks + span - 1) * ldb + (long)bj * TN + TN - 1 : ((long)bj * TN + TN - 1) * ldb + ks + span - 1);
        const long c_hi = y * sC + z * zC + ((long)bi * TM + TM - 1) * ldc + (long)bj * TN + TN - 1;
        if (a_hi >= a_elems || b_hi >= b_cap || c_hi >= c_elems) ok = false;
      });
  if (!ok) return fail(h, SIGP_BAD_ARG, "debug_run_gemm: the descriptor reaches outside the operand buffers (or a tile's k span is empty)");

  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dA, dB, dC;
  HIPCHK(h, hipMalloc(&dA.p, (size_t)a_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dA.p, A, (size_t)a_elems * sizeof(Real), hipMemcpyHostToDevice));
  if (!alias) {
    HIPCHK(h, hipMalloc(&dB.p, (size_t)b_elems * sizeof(Real)));
    HIPCHK(h, hipMemcpy(dB.p, B, (size_t)b_elems * sizeof(Real), hipMemcpyHostToDevice));
  }
  HIPCHK(h, hipMalloc(&dC.p, (size_t)c_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dC.p, C, (size_t)c_elems * sizeof(Real), hipMemcpyHostToDevice));
  GemmArgsT<Real> g{};
  g.A = (const Real*)dA.p; g.lda = lda; g.B = alias ? g.A : (const Real*)dB.p; g.ldb = ldb; g.C = (Real*)dC.p; g.ldc = ldc;
  g.K = K; g.batch = batch; g.sA = sA; g.sB = sB; g.sC = sC; g.r0 = r0; g.r1 = r1; g.c0 = c0; g.c1 = c1; g.lower = lower;
  g.stamp = nullptr; g.dbg = 0; g.patch = 0; g.ntile = 0; g.ktri = ktri;
  g.zcount = zcount; g.zA = zA; g.zB = zB; g.zC = zC; g.zshift = zshift; g.ride_bi1 = ride_bi1; g.ride_rows = ride_rows;
  hipStream_t st = h->slots[0].s_upd;
  int rc = SIGP_BAD_ARG;
  switch (cfg) {
    case DBG_CFG_32x128_SET: rc = launch_gemm_cfg<Real, 32, 128, 1, 4, GEMM_SET, false>(h, st, g); break;
    case DBG_CFG_32x128_SET_BT: rc = launch_gemm_cfg<Real, 32, 128, 1, 4, GEMM_SET, true>(h, st, g); break;
    case DBG_CFG_32x128_SETNEG_BT: rc = launch_gemm_cfg<Real, 32, 128, 1, 4, GEMM_SETNEG, true>(h, st, g); break;
    case DBG_CFG_64x64_SET: rc = launch_gemm_cfg<Real, 64, 64, 2, 2, GEMM_SET, false>(h, st, g); break;
    case DBG_CFG_64x64_SUB: rc = launch_gemm_cfg<Real, 64, 64, 2, 2, GEMM_SUB, false>(h, st, g); break;
    case DBG_CFG_64x64_SUB_BT: rc = launch_gemm_cfg<Real, 64, 64, 2, 2, GEMM_SUB, true>(h, st, g); break;
    case DBG_CFG_128x128_SUB: rc = launch_gemm_cfg<Real, 128, 128, 2, 2, GEMM_SUB, false>(h, st, g); break;
    case DBG_CFG_128x128_SETNEG_BT: rc = launch_gemm_cfg<Real, 128, 128, 2, 2, GEMM_SETNEG, true>(h, st, g); break;
    case DBG_CFG_32x32_SUB: rc = launch_gemm_cfg<Real, 32, 32, 2, 2, GEMM_SUB, false>(h, st, g); break;
    case DBG_CFG_SYRK128_SUB: rc = launch_syrk128_t<Real, false>(h, st, g); break;
    case DBG_CFG_SYRK128_SET: rc = launch_syrk128_t<Real, true>(h, st, g); break;
    case DBG_CFG_AUTO: rc = gemm_sub_auto<Real>(h, st, g); break;
  }
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(C, dC.p, (size_t)c_elems * sizeof(Real), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

template <typename Real>
static int debug_run_strip_t(sigp_handle* h, void* M, long ld, const void* Mt, long ldm, int rb0, int nstrips, int J, int Wp, int members, long sM, long sMt,
                             long m_elems, long mt_elems) {
  constexpr int NE = Num<Real>::NE;
  constexpr long LIM = 1L << 20;
  if (!h || !M || !Mt) return SIGP_BAD_ARG;
  if (rb0 < 0 || nstrips < 0 || J < 0 || Wp < 1 || Wp > MT_W || members < 1 || members > 64 || rb0 > 4096 || nstrips > 4096 || J > 4096)
    return fail(h, SIGP_BAD_ARG, "debug_run_strip: strips / panel");
  if (ld < (long)(J + Wp) * NB || ldm < (long)Wp * NB || ld > LIM || ldm > LIM || sM < 0 || sMt < 0 || m_elems < 1 || mt_elems < 1 || std::max(sM, sMt) > (1L << 40) ||
      (members > 1 && sM == 0))
    return fail(h, SIGP_BAD_ARG, "debug_run_strip: strides");
  if (ld % NE || ldm % NE || sM % NE || sMt % NE) return fail(h, SIGP_BAD_ARG, "debug_run_strip: a row or member stride is not a multiple of 16 bytes");
  if (nstrips > 0 && ((members - 1) * sM + ((long)(rb0 + nstrips) * NB - 1) * ld + (long)(J + Wp) * NB - 1 >= m_elems ||
                      (members - 1) * sMt + ((long)Wp * NB - 1) * ldm + (long)Wp * NB - 1 >= mt_elems))
    return fail(h, SIGP_BAD_ARG, "debug_run_strip: the descriptor reaches outside the operand buffers");
  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dM, dT;
  HIPCHK(h, hipMalloc(&dM.p, (size_t)m_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dM.p, M, (size_t)m_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dT.p, (size_t)mt_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dT.p, Mt, (size_t)mt_elems * sizeof(Real), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_upd;
  if (nstrips > 0) {
    StripArgsT<Real> a{(Real*)dM.p, ld, sM, (const Real*)dT.p, ldm, sMt, rb0, J, Wp};
    const int rc = launch_panel_strip<Real>(h, st, a, nstrips, members);
    if (rc) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(M, dM.p, (size_t)m_elems * sizeof(Real), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

template <typename Real>
static int debug_run_link_t(sigp_handle* h, void* M, long ld, int c, const void* Linv, void* scratch, int rows_ride, int members, long sM, long sL, long sS,
                            long m_elems, long linv_elems, long scratch_elems) {
  constexpr int NE = Num<Real>::NE;
  constexpr long LIM = 1L << 20;
  if (!h || !M || !Linv || !scratch) return SIGP_BAD_ARG;
  if (c < 0 || c > 4096 || rows_ride < 0 || rows_ride > 4096 || members < 1 || members > 64) return fail(h, SIGP_BAD_ARG, "debug_run_link: column / rows / members");
  if (ld < (long)(c + 2) * NB || ld > LIM || sM < 0 || sL < 0 || sS < 0 || m_elems < 1 || linv_elems < 1 || scratch_elems < 1 || std::max({sM, sL, sS}) > (1L << 40) ||
      (members > 1 && (sM == 0 || sS == 0)))
    return fail(h, SIGP_BAD_ARG, "debug_run_link: strides");
  if (ld % NE || sM % NE || sL % NE || sS % NE) return fail(h, SIGP_BAD_ARG, "debug_run_link: a row or member stride is not a multiple of 16 bytes");
  if ((members - 1) * sM + ((long)(c + 2 + rows_ride) * NB - 1) * ld + (long)(c + 2) * NB - 1 >= m_elems || (members - 1) * sL + (long)NB * NB > linv_elems ||
      (members - 1) * sS + (long)NB * NB > scratch_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_link: the descriptor reaches outside the operand buffers");
  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dM, dL, dS;
  HIPCHK(h, hipMalloc(&dM.p, (size_t)m_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dM.p, M, (size_t)m_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dL.p, (size_t)linv_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dL.p, Linv, (size_t)linv_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dS.p, (size_t)scratch_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dS.p, scratch, (size_t)scratch_elems * sizeof(Real), hipMemcpyHostToDevice));
  LinkArgsT<Real> a{};
  a.Acol = (Real*)dM.p + (long)(c + 1) * NB * ld + (long)c * NB; a.ld = ld;
  a.Linv = (const Real*)dL.p;
  a.Cdiag = (Real*)dM.p + (long)(c + 1) * NB * (ld + 1);
  a.scratch = (Real*)dS.p;
  a.sM = sM; a.sL = sL; a.sS = sS; a.rows_ride = rows_ride;
  hipStream_t st = h->slots[0].s_upd;
  const int rc = launch_chain_link<Real>(h, st, a, members);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(M, dM.p, (size_t)m_elems * sizeof(Real), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(scratch, dS.p, (size_t)scratch_elems * sizeof(Real), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

extern "C" {

int sigp_debug_run_gemm(sigp_handle* h, int dtype, int cfg, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int K, int r0, int r1,
                        int c0, int c1, int lower, int ktri, int batch, int64_t sA, int64_t sB, int64_t sC, int zcount, int64_t zA, int64_t zB, int64_t zC,
                        int zshift, int ride_bi1, int ride_rows, int64_t a_elems, int64_t b_elems, int64_t c_elems) {
  if (dtype == SIGP_F32)
    return debug_run_gemm_t<float>(h, cfg, A, lda, B, ldb, C, ldc, K, r0, r1, c0, c1, lower, ktri, batch, sA, sB, sC, zcount, zA, zB, zC, zshift, ride_bi1, ride_rows,
                                   a_elems, b_elems, c_elems);
  if (dtype != SIGP_F64) return SIGP_BAD_ARG;
  return debug_run_gemm_t<double>(h, cfg, A, lda, B, ldb, C, ldc, K, r0, r1, c0, c1, lower, ktri, batch, sA, sB, sC, zcount, zA, zB, zC, zshift, ride_bi1, ride_rows,
                                  a_elems, b_elems, c_elems);
}

int sigp_debug_run_strip(sigp_handle* h, int dtype, void* M, int64_t ld, const void* Mt, int64_t ldm, int rb0, int nstrips, int J, int Wp, int members, int64_t sM,
                         int64_t sMt, int64_t m_elems, int64_t mt_elems) {
  if (dtype == SIGP_F32) return debug_run_strip_t<float>(h, M, ld, Mt, ldm, rb0, nstrips, J, Wp, members, sM, sMt, m_elems, mt_elems);
  if (dtype != SIGP_F64) return SIGP_BAD_ARG;
  return debug_run_strip_t<double>(h, M, ld, Mt, ldm, rb0, nstrips, J, Wp, members, sM, sMt, m_elems, mt_elems);
}

int sigp_debug_run_link(sigp_handle* h, int dtype, void* M, int64_t ld, int c, const void* Linv, void* scratch, int rows_ride, int members, int64_t sM, int64_t sL,
                        int64_t sS, int64_t m_elems, int64_t linv_elems, int64_t scratch_elems) {
  if (dtype == SIGP_F32) return debug_run_link_t<float>(h, M, ld, c, Linv, scratch, rows_ride, members, sM, sL, sS, m_elems, linv_elems, scratch_elems);
  if (dtype != SIGP_F64) return SIGP_BAD_ARG;
  return debug_run_link_t<double>(h, M, ld, c, Linv, scratch, rows_ride, members, sM, sL, sS, m_elems, linv_elems, scratch_elems);
}

int sigp_debug_run_refined_solve(sigp_handle* h, int trans, void* A, int64_t lda, int rows, const void* W, int64_t ldw, const void* L, int64_t ldl, int members,
                                 int64_t sA, int64_t sW, int64_t sL, int64_t a_elems, int64_t w_elems, int64_t l_elems) {
  constexpr long LIM = 1L << 20;
  if (!h || !A || !W || !L) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: fp64 only");
  if ((trans != 0 && trans != 1) || rows < 1 || rows > LIM || members < 1 || members > 64) return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: trans / rows / members");
  if (lda < NB || ldw < NB || ldl < NB || lda > LIM || ldw > LIM || ldl > LIM || sA < 0 || sW < 0 || sL < 0 || std::max({sA, sW, sL}) > (1L << 40) || a_elems < 1 ||
      w_elems < 1 || l_elems < 1)
    return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: strides");
  if (lda % 2 || ldw % 2 || ldl % 2 || sA % 2 || sW % 2 || sL % 2) return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: a row or member stride is not a multiple of 16 bytes");
  const long a_hi = (long)(rows - 1) * lda + NB - 1;
  if ((members - 1) * sA + a_hi >= a_elems || (members - 1) * sW + (long)(NB - 1) * ldw + NB - 1 >= w_elems || (members - 1) * sL + (long)(NB - 1) * ldl + NB - 1 >= l_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: the descriptor reaches outside the operand buffers");
  if (members > 1 && sA <= a_hi) return fail(h, SIGP_BAD_ARG, "debug_run_refined_solve: members would write the same entries");
  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dA, dW, dL;
  HIPCHK(h, hipMalloc(&dA.p, (size_t)a_elems * sizeof(double)));
  HIPCHK(h, hipMemcpy(dA.p, A, (size_t)a_elems * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dW.p, (size_t)w_elems * sizeof(double)));
  HIPCHK(h, hipMemcpy(dW.p, W, (size_t)w_elems * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dL.p, (size_t)l_elems * sizeof(double)));
  HIPCHK(h, hipMemcpy(dL.p, L, (size_t)l_elems * sizeof(double), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_upd;
  const RefinedArgs a{(double*)dA.p, lda, sA, (const double*)dW.p, ldw, sW, (const double*)dL.p, ldl, sL, rows};
  const int rc = trans ? launch_refined_solve<true>(h, st, a, members) : launch_refined_solve<false>(h, st, a, members);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(A, dA.p, (size_t)a_elems * sizeof(double), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

// ---- run-and-return entries of the quadratic solve kernels (tests/test_hip_solve_kernels.py) ------------------------------------------------
// rowdot_kernel / coldot_kernel: ONE launch with the grid rule the engine uses (one wave per matrix row, four per workgroup; one workgroup per
// 16 vectors of columns) on the caller's operands, every buffer back whole.  The kernels load whole 16-byte vectors of Mx and of the
// right-hand sides, so K (rowdot) and the column count (coldot) must be multiples of the vector width, like every row and member stride.
}  // extern "C" (templates need C++ linkage)

template <typename Real>
static int debug_run_rowdot_t(sigp_handle* h, const void* Mx, long ld, int nrows, int K, int kmode, const void* Zin, long ldzin, void* Zout, long ldzout, int nrhs,
                              int sub, const void* Zadd, int pm_pw, int j_off, int members, long sM, long sZi, long sZo, long m_elems, long zin_elems,
                              long zout_elems) {
  constexpr int NE = Num<Real>::NE;
  constexpr long LIM = 1L << 20;
  if (!h || !Mx || !Zin || !Zout) return SIGP_BAD_ARG;
  if (nrows < 1 || nrows > LIM || K < 1 || K > LIM || K % NE) return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: K = %d is not a positive multiple of the vector width %d", K, NE);
  if (kmode < 0 || kmode > 2 || nrhs < 1 || nrhs > TS_RHS || (sub != 0 && sub != 1) || members < 1 || members > 64)
    return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: kmode / nrhs / sub / members");
  if (kmode != 0 && nrows > K) return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: a triangular k range needs nrows <= K");
  if (ld < K || ldzin < K || ld > LIM || ldzin > LIM || sM < 0 || sZi < 0 || sZo < 0 || std::max({sM, sZi, sZo}) > (1L << 40) || m_elems < 1 || zin_elems < 1 || zout_elems < 1)
    return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: strides");
  if (ld % NE || ldzin % NE || sM % NE || sZi % NE || sZo % NE) return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: a row or member stride is not a multiple of 16 bytes");
  if (pm_pw < 0 || pm_pw > LIM || pm_pw % NE || j_off < 0 || j_off > LIM || (pm_pw == 0 && (j_off != 0 || ldzout < nrows || ldzout > LIM || ldzout % NE)))
    return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: output layout");
  if (Zadd && members > 1) return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: Zadd has no member stride (the kernel reads ONE Zadd for every member)");
  const long g_hi = (long)j_off + nrows - 1;
  const long out_hi = pm_pw > 0 ? ((g_hi / pm_pw) * TS_RHS + nrhs - 1) * pm_pw + g_hi % pm_pw : (long)(nrhs - 1) * ldzout + nrows - 1;
  if ((members - 1) * sM + (long)(nrows - 1) * ld + K - 1 >= m_elems || (members - 1) * sZi + (long)(nrhs - 1) * ldzin + K - 1 >= zin_elems ||
      (members - 1) * sZo + out_hi >= zout_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: the descriptor reaches outside the operand buffers");
  if (members > 1 && sZo <= out_hi) return fail(h, SIGP_BAD_ARG, "debug_run_rowdot: members would write the same entries");
  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dM, dI, dA, dO;
  HIPCHK(h, hipMalloc(&dM.p, (size_t)m_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dM.p, Mx, (size_t)m_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dI.p, (size_t)zin_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dI.p, Zin, (size_t)zin_elems * sizeof(Real), hipMemcpyHostToDevice));
  if (Zadd) {
    HIPCHK(h, hipMalloc(&dA.p, (size_t)zin_elems * sizeof(Real)));
    HIPCHK(h, hipMemcpy(dA.p, Zadd, (size_t)zin_elems * sizeof(Real), hipMemcpyHostToDevice));
  }
  HIPCHK(h, hipMalloc(&dO.p, (size_t)zout_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dO.p, Zout, (size_t)zout_elems * sizeof(Real), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_upd;
  hipLaunchKernelGGL(rowdot_kernel<Real>, dim3((unsigned)((nrows + 3) / 4), (unsigned)members), dim3(256), 0, st, (const Real*)dM.p, ld, nrows, K, kmode, (const Real*)dI.p,
                     ldzin, (Real*)dO.p, ldzout, nrhs, sub, (const Real*)dA.p, pm_pw, j_off, sM, sZi, sZo);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(Zout, dO.p, (size_t)zout_elems * sizeof(Real), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

template <typename Real>
static int debug_run_coldot_t(sigp_handle* h, const void* Mx, long ld, int ncols, int K, const void* Zin, long ldzin, void* Zout, long ldzout, int nrhs, long m_elems,
                              long zin_elems, long zout_elems) {
  constexpr int NE = Num<Real>::NE, CW = 16 * NE;
  constexpr long LIM = 1L << 20;
  if (!h || !Mx || !Zin || !Zout) return SIGP_BAD_ARG;
  if (ncols < 1 || ncols > LIM || ncols % NE) return fail(h, SIGP_BAD_ARG, "debug_run_coldot: the column count %d is not a positive multiple of the vector width %d", ncols, NE);
  if (K < 1 || K > LIM || nrhs < 1 || nrhs > TS_RHS) return fail(h, SIGP_BAD_ARG, "debug_run_coldot: K / nrhs");
  if (ld < ncols || ldzin < K || ldzout < ncols || ld > LIM || ldzin > LIM || ldzout > LIM || m_elems < 1 || zin_elems < 1 || zout_elems < 1)
    return fail(h, SIGP_BAD_ARG, "debug_run_coldot: strides");
  if (ld % NE || ldzin % NE || ldzout % NE) return fail(h, SIGP_BAD_ARG, "debug_run_coldot: a row stride is not a multiple of 16 bytes");
  if ((long)(K - 1) * ld + ncols - 1 >= m_elems || (long)(nrhs - 1) * ldzin + K - 1 >= zin_elems || (long)(nrhs - 1) * ldzout + ncols - 1 >= zout_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_coldot: the descriptor reaches outside the operand buffers");
  HIPCHK(h, hipSetDevice(h->device));
  DebugDeviceBuf dM, dI, dO;
  HIPCHK(h, hipMalloc(&dM.p, (size_t)m_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dM.p, Mx, (size_t)m_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dI.p, (size_t)zin_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dI.p, Zin, (size_t)zin_elems * sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dO.p, (size_t)zout_elems * sizeof(Real)));
  HIPCHK(h, hipMemcpy(dO.p, Zout, (size_t)zout_elems * sizeof(Real), hipMemcpyHostToDevice));
  hipStream_t st = h->slots[0].s_upd;
  hipLaunchKernelGGL(coldot_kernel<Real>, dim3((unsigned)((ncols + CW - 1) / CW)), dim3(256), 0, st, (const Real*)dM.p, ld, ncols, K, (const Real*)dI.p, ldzin, (Real*)dO.p,
                     ldzout, nrhs);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(Zout, dO.p, (size_t)zout_elems * sizeof(Real), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

extern "C" {

int sigp_debug_run_rowdot(sigp_handle* h, int dtype, const void* Mx, int64_t ld, int nrows, int K, int kmode, const void* Zin, int64_t ldzin, void* Zout, int64_t ldzout,
                          int nrhs, int sub, const void* Zadd, int pm_pw, int j_off, int members, int64_t sM, int64_t sZi, int64_t sZo, int64_t m_elems,
                          int64_t zin_elems, int64_t zout_elems) {
  if (dtype == SIGP_F32)
    return debug_run_rowdot_t<float>(h, Mx, ld, nrows, K, kmode, Zin, ldzin, Zout, ldzout, nrhs, sub, Zadd, pm_pw, j_off, members, sM, sZi, sZo, m_elems, zin_elems, zout_elems);
  if (dtype != SIGP_F64) return SIGP_BAD_ARG;
  return debug_run_rowdot_t<double>(h, Mx, ld, nrows, K, kmode, Zin, ldzin, Zout, ldzout, nrhs, sub, Zadd, pm_pw, j_off, members, sM, sZi, sZo, m_elems, zin_elems, zout_elems);
}

int sigp_debug_run_coldot(sigp_handle* h, int dtype, const void* Mx, int64_t ld, int ncols, int K, const void* Zin, int64_t ldzin, void* Zout, int64_t ldzout, int nrhs,
                          int64_t m_elems, int64_t zin_elems, int64_t zout_elems) {
  if (dtype == SIGP_F32) return debug_run_coldot_t<float>(h, Mx, ld, ncols, K, Zin, ldzin, Zout, ldzout, nrhs, m_elems, zin_elems, zout_elems);
  if (dtype != SIGP_F64) return SIGP_BAD_ARG;
  return debug_run_coldot_t<double>(h, Mx, ld, ncols, K, Zin, ldzin, Zout, ldzout, nrhs, m_elems, zin_elems, zout_elems);
}

// The fp32 engine's block solves on the factor and the inverse blocks the last fp32 fit left on the handle: rhs [nrhs][n] (doubles; rounded to
// fp32 and the pad rows zeroed by convert_rows_kernel, as a refinement step hands its residuals over) is replaced by
// which = 0: L~^-1 rhs (f32_block_forward), 1: L~^-T rhs (f32_block_backward), 2: L~^-T L~^-1 rhs (both, as a refinement step runs them).
int sigp_debug_f32_solve(sigp_handle* h, int which, double* rhs, int64_t n, int nrhs) {
  if (!h || !rhs || which < 0 || which > 2 || nrhs < 1 || nrhs > TS_RHS) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F32 || !h->fitted || n != h->n || !h->fU || h->cap_f_npad < h->n_pad) return fail(h, SIGP_BAD_ARG, "debug_f32_solve: the handle holds no fp32 fit of order %ld", (long)n);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->slots[0].s_upd;
  const long n_pad = h->n_pad, ld = n_pad, tot = (long)nrhs * n_pad;
  int rc;
  HIPCHK(h, hipMemcpy2DAsync(h->rq, (size_t)ld * sizeof(double), rhs, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)nrhs, hipMemcpyHostToDevice, st));
  float* in = which == 1 ? h->fXw : h->fZ;
  hipLaunchKernelGGL((convert_rows_kernel<double, float>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double*)h->rq, ld, in, ld, nrhs, (int)n_pad, (int)n);
  HIPCHK(h, hipGetLastError());
  if (which != 1 && (rc = f32_block_forward(h, st, n_pad, nrhs, h->fZ, h->fXw))) return rc;
  if (which != 0 && (rc = f32_block_backward(h, st, n_pad, nrhs, h->fXw, h->fZ))) return rc;
  const float* res = which == 0 ? h->fXw : h->fZ;
  hipLaunchKernelGGL((convert_rows_kernel<float, double>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, res, ld, h->rq, ld, nrhs, (int)n_pad, (int)n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpy2DAsync(rhs, (size_t)n * sizeof(double), h->rq, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), (size_t)nrhs, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return SIGP_OK;
}

// the inverse blocks of the last fp32 fit: which = 0 fU (row-major upper triangular inverse-transposes of the 2048-column diagonal blocks),
// 1 fV (their transposes); out [n_pad][n_pad] floats (n_pad = 128 sigp_num_blocks)
int sigp_debug_f32_get_inverse(sigp_handle* h, int which, float* out) {
  if (!h || !out || which < 0 || which > 1) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F32 || !h->fitted || !h->fU || h->cap_f_npad < h->n_pad) return fail(h, SIGP_BAD_ARG, "debug_f32_get_inverse: the handle holds no fp32 fit");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->slots[0].s_upd));
  HIPCHK(h, hipMemcpy(out, which == 0 ? h->fU : h->fV, (size_t)h->n_pad * h->n_pad * sizeof(float), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

// G = d score / d K~ of a hindcast score on the single fp64 fit (hindcast.hpp; sigp_hindcast_grad_ard's launches up to the ARD pass): its lower
// 128-tiles into out [n][ldo] as the product wrote them -- the diagonal tiles whole, both halves -- and zeros in the tiles above.
int sigp_debug_run_hindcast_adjoint(sigp_handle* h, int64_t lead, int64_t min_train, int sigma_mode, int criterion, double* out, int64_t ldo) {
  if (!h || !out || ldo < h->n) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64 || !h->fitted) return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_adjoint: the handle holds no fp64 fit");
  if (criterion != SIGP_LOO_NLPD && criterion != SIGP_LOO_SSE) return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_adjoint: bad criterion");
  int rc;
  if ((rc = hindcast_check(h, "debug_run_hindcast_adjoint", h->n, lead, min_train, sigma_mode, SIGP_HINDCAST_MAX_LEAD))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad;
  if ((rc = ensure(h, &h->gV, &h->cap_gV, HindcastArdVecs::size(n_pad)))) return rc;
  if ((rc = scores_ensure(h, 1, n_pad, ScoreParts::size(1, n_pad)))) return rc;
  if ((rc = scores_grad_ensure(h, 1, n_pad, 0))) return rc;
  const ScoreParts sp{h->gPart, 1, n_pad};
  const HindcastVecs hv{h->gV, n_pad};
  if ((rc = scores_stage_q(h, st, sp))) return rc;
  if ((rc = hindcast_launch(h, st, 1, n, n_pad, s.mat, 0, h->y, 0, nullptr, sp.q(), 0, lead, min_train, sigma_mode, sp, hv, 0, 1))) return rc;
  if ((rc = hindcast_adjoint(h, st, 1, n, n_pad, s.mat, 0, s.dinv, 0, lead, min_train, sigma_mode, criterion, sp.q(), 0, hv, 0, false))) return rc;
  HIPCHK(h, hipMemcpy2DAsync(out, (size_t)ldo * sizeof(double), h->gD, (size_t)n_pad * sizeof(double), (size_t)n * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, st));
  if ((rc = sync_slot(h, s))) return rc;
  for (long i = 0; i < n; ++i)
    for (long j = (i / NB + 1) * NB; j < n; ++j) out[i * ldo + j] = 0.0;
  return SIGP_OK;
}

// ONE launch of hindcast_w_kernel (which = 0) or hindcast_w_lds_kernel (1) on host operands (include/sigp_debug.h).  zbar travels inside a
// HindcastVecs arena whose other six vectors are NaN: the kernels read zbar alone.
int sigp_debug_run_hindcast_w(sigp_handle* h, int which, const double* U, const double* Cb, const double* z, const double* zbar, double* W, int n, int n_pad,
                              int64_t ld, int lead, int members, int64_t sC, int64_t sZ, int64_t c_elems, int64_t z_elems) {
  constexpr long LIM = 1L << 28;
  if (!h || !U || !Cb || !z || !zbar || !W || which < 0 || which > 1) return SIGP_BAD_ARG;
  if (n < 1 || n_pad < n || n_pad % 128 || n_pad > 16384 || ld < n_pad || ld > LIM || lead < 1 || lead > SIGP_HINDCAST_MAX_LEAD || members < 1 || members > 8)
    return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_w: n / n_pad / ld / lead / members");
  if (sC < 0 || sZ < 0 || sC > LIM || sZ > LIM || c_elems < 1 || c_elems > LIM || z_elems < 1 || z_elems > LIM) return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_w: strides");
  const long mat_hi = (long)(n_pad - 1) * ld + n_pad - 1;
  if ((long)(members - 1) * sC + mat_hi >= c_elems || (long)(members - 1) * sZ + n - 1 >= z_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_w: the descriptor reaches outside the operand buffers");
  if (members > 1 && sC <= mat_hi) return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_w: members would write the same entries");
  if (which == 1 && !hindcast_w_use_lds(n_pad)) return fail(h, SIGP_BAD_ARG, "debug_run_hindcast_w: n_pad = %d is beyond hindcast_w_lds_kernel's LDS limit", n_pad);
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cb = (size_t)c_elems * sizeof(double), zb = (size_t)z_elems * sizeof(double), head = (size_t)6 * n_pad * sizeof(double);
  DebugDeviceBuf dU, dC, dW, dZ, dV;
  HIPCHK(h, hipMalloc(&dU.p, cb)); HIPCHK(h, hipMemcpy(dU.p, U, cb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dC.p, cb)); HIPCHK(h, hipMemcpy(dC.p, Cb, cb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dW.p, cb)); HIPCHK(h, hipMemcpy(dW.p, W, cb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dZ.p, zb)); HIPCHK(h, hipMemcpy(dZ.p, z, zb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMalloc(&dV.p, head + zb));
  HIPCHK(h, hipMemset(dV.p, 0xFF, head));                    // cum .. suf: NaN
  HIPCHK(h, hipMemcpy((char*)dV.p + head, zbar, zb, hipMemcpyHostToDevice));
  const HindcastVecs hv{(double*)dV.p, n_pad};               // hv.zbar() = the copy of zbar; member m's sZ behind it
  const HindcastStrides ms{sZ, 0, sZ, sC};
  hipStream_t st = h->slots[0].s_upd;
  if (which == 1) {
    static AttrOnce attr;
    HIPCHK(h, attr.set(h->device, (const void*)hindcast_w_lds_kernel, (int)hindcast_w_lds_bytes(HINDCAST_W_LDS_MAX_NPAD)));
    hipLaunchKernelGGL(hindcast_w_lds_kernel, dim3((unsigned)n_pad, (unsigned)members), dim3(256), (size_t)hindcast_w_lds_bytes(n_pad), st, (const double*)dU.p,
                       (const double*)dC.p, (long)ld, n, n_pad, (const double*)dZ.p, lead, hv, (double*)dW.p, ms);
  } else {
    hipLaunchKernelGGL(hindcast_w_kernel, dim3((unsigned)n_pad, (unsigned)members), dim3(256), 0, st, (const double*)dU.p, (const double*)dC.p, (long)ld, n, n_pad,
                       (const double*)dZ.p, lead, hv, (double*)dW.p, ms);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(W, dW.p, cb, hipMemcpyDeviceToHost));
  return SIGP_OK;
}

// ---- run-and-return entries of the score-gradient kernels (tests/test_hip_ard_pass.py, tests/test_hip_score_products.py) -------------------
// Same convention: host operands in, the launches the engine issues through the launchers the engine uses, every buffer back whole;
// SIGP_BAD_ARG, nothing launched, for a descriptor that leaves the buffer sizes given in elements, a stride that is not a multiple of
// 16 bytes, members whose outputs overlap and what the kernels do not implement.
static int debug_upload(sigp_handle* h, DebugDeviceBuf& b, const double* src, long elems) {
  HIPCHK(h, hipMalloc(&b.p, (size_t)elems * sizeof(double)));
  HIPCHK(h, hipMemcpy(b.p, src, (size_t)elems * sizeof(double), hipMemcpyHostToDevice));
  return SIGP_OK;
}

// One call of ard_tile_pass_members<W> (its memset of ardXc, ard_center_kernel, ard_grad_partial_kernel<8 | 32, W> by d) and the matching finish
// kernel.  wsel = ARD_W_NLML: vec = a [members][sVec], q [members][sQ] (q[0] = y^T a);  ARD_W_LOO: vec = a LooArdVecs arena per member (a at 0,
// v at 3 n_pad, eps at 4 n_pad), q is not used.  The member strides are the engine's: ArdMemberStrides{sU, sP, sVec, sQ, sPartial, sVec, sVec}
// and LooArdStrides{sP, 0, sVec, sPartial, sGrad}.
int sigp_debug_run_ard_pass(sigp_handle* h, int wsel, int kernel_id, int n, int n_pad, int d, int dp, int members, const double* U, int64_t sU, int64_t u_elems,
                            const double* M, int64_t ld, int64_t sP, int64_t m_elems, const double* vec, int64_t sVec, int64_t vec_elems, const double* q, int64_t sQ,
                            int64_t q_elems, double sn, const double* sn_m, double* Uc, double* partial, int64_t sPartial, int64_t partial_elems, double* grad,
                            int64_t sGrad, int64_t grad_elems) {
  constexpr long LIM = 1L << 28;
  if (!h || !U || !M || !vec || !Uc || !partial || !grad) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: fp64 only");
  if (wsel != ARD_W_NLML && wsel != ARD_W_LOO) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: wsel");
  if (wsel == ARD_W_NLML && !q) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: ARD_W_NLML reads q");
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: RBF / MATERN52 only");
  if (n < 1 || n_pad < n || n_pad % 128 || n_pad > 4096 || d < 1 || d > 1024 || dp < ((d + 15) & ~15) || dp > 4096 || members < 1 || members > 8)
    return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: n / n_pad / d / dp / members (dp must hold d rounded up to 16 features)");
  if (ld < n_pad || ld > LIM || sU < 0 || sP < 0 || sVec < 0 || sQ < 0 || sPartial < 0 || sGrad < 0 || std::max({sU, sP, sVec, sQ, sPartial, sGrad}) > LIM ||
      std::max({u_elems, m_elems, vec_elems, q_elems, partial_elems, grad_elems}) > LIM || std::min({u_elems, m_elems, vec_elems, partial_elems, grad_elems}) < 1 || q_elems < 0)
    return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: strides");
  // 16-byte accesses: rows of U, Uc and P, the vectors a and v
  if (dp % 2 || ld % 2 || sU % 2 || sP % 2 || sVec % 2) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: a row or member stride is not a multiple of 16 bytes");
  const long ntiles = kbuild_tiles(n_pad), mb1 = members - 1;
  const long u_hi = (long)n_pad * dp - 1, m_hi = (long)(n_pad - 1) * ld + n_pad - 1, v_hi = wsel == ARD_W_LOO ? LooArdVecs::size(n_pad) - 1 : (long)n_pad - 1;
  const long p_hi = ntiles * dp - 1;
  if (mb1 * sU + u_hi >= u_elems || mb1 * sP + m_hi >= m_elems || mb1 * sVec + v_hi >= vec_elems || (wsel == ARD_W_NLML && mb1 * sQ >= q_elems) ||
      mb1 * sPartial + p_hi >= partial_elems || mb1 * sGrad + d >= grad_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: the descriptor reaches outside the operand buffers");
  if (members > 1 && (sU <= u_hi || sPartial <= p_hi || sGrad <= d)) return fail(h, SIGP_BAD_ARG, "debug_run_ard_pass: members would write the same entries");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  const long uc_elems = mb1 * sU + (long)n_pad * dp;
  if ((rc = ensure(h, &h->ardXc, &h->cap_ardXc, uc_elems))) return rc;
  DebugDeviceBuf dU, dM, dV, dQ, dP, dG, dS;
  if ((rc = debug_upload(h, dU, U, u_elems)) || (rc = debug_upload(h, dM, M, m_elems)) || (rc = debug_upload(h, dV, vec, vec_elems)) ||
      (rc = debug_upload(h, dP, partial, partial_elems)) || (rc = debug_upload(h, dG, grad, grad_elems)))
    return rc;
  if (q && q_elems > 0 && (rc = debug_upload(h, dQ, q, q_elems))) return rc;
  if (sn_m && (rc = debug_upload(h, dS, sn_m, members))) return rc;
  hipStream_t st = h->slots[0].s_upd;
  const double* dv = (const double*)dV.p;
  const ArdMemberStrides ms{sU, sP, sVec, sQ, sPartial, sVec, sVec};
  if (wsel == ARD_W_NLML) {
    if ((rc = ard_tile_pass_members<ARD_W_NLML>(h, st, members, (const double*)dU.p, n, d, dp, n_pad, ms, kernel_id, (const double*)dM.p, ld, dv, (const double*)dQ.p, nullptr,
                                                nullptr, (double*)dP.p)))
      return rc;
    hipLaunchKernelGGL(ard_grad_finish_kernel, dim3((unsigned)(d + 1), (unsigned)members), dim3(256), 0, st, (const double*)dP.p, ntiles, dp, d, n, (const double*)dM.p, (long)ld,
                       dv, (const double*)dQ.p, sn, (double*)dG.p, ms, (long)sGrad, (const double*)dS.p);
  } else {
    const LooArdVecs w{(double*)dV.p, n_pad};
    if ((rc = ard_tile_pass_members<ARD_W_LOO>(h, st, members, (const double*)dU.p, n, d, dp, n_pad, ms, kernel_id, (const double*)dM.p, ld, w.a(), nullptr, w.v(), w.eps(),
                                               (double*)dP.p)))
      return rc;
    hipLaunchKernelGGL(loo_ard_finish_kernel, dim3((unsigned)(d + 1), (unsigned)members), dim3(256), 0, st, (const double*)dP.p, ntiles, dp, d, n, (const double*)dM.p, (long)ld, w,
                       sn, (double*)dG.p, LooArdStrides{sP, 0, sVec, sPartial, sGrad}, (const double*)dS.p);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(Uc, h->ardXc, (size_t)uc_elems * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(partial, dP.p, (size_t)partial_elems * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(grad, dG.p, (size_t)grad_elems * sizeof(double), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

// ONE launch of cv_band_product_kernel through launch_cv_band_product: C = P B on T x T tiles per member.  P and C [128 T][ld] per member, sP
// apart (the kernel has ONE member stride for both); band [128 T][384] per member, sBand apart.
int sigp_debug_run_cv_band(sigp_handle* h, const double* P, const double* band, double* Cm, int T, int64_t ld, int members, int64_t sP, int64_t sBand, int64_t p_elems,
                           int64_t band_elems, int64_t c_elems) {
  constexpr long LIM = 1L << 28;
  if (!h || !P || !band || !Cm) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: fp64 only");
  if (T < 1 || T > 32 || members < 1 || members > 8) return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: T / members");
  const long n_pad = (long)T * NB;
  if (ld < n_pad || ld > LIM || sP < 0 || sBand < 0 || sP > LIM || sBand > LIM || p_elems < 1 || band_elems < 1 || c_elems < 1 || std::max({p_elems, band_elems, c_elems}) > LIM)
    return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: strides");
  if (ld % 2 || sP % 2 || sBand % 2) return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: a row or member stride is not a multiple of 16 bytes");
  const long mb1 = members - 1, m_hi = (n_pad - 1) * ld + n_pad - 1, b_hi = n_pad * CVA_BAND - 1;
  if (mb1 * sP + m_hi >= p_elems || mb1 * sP + m_hi >= c_elems || mb1 * sBand + b_hi >= band_elems)
    return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: the descriptor reaches outside the operand buffers");
  if (members > 1 && sP <= m_hi) return fail(h, SIGP_BAD_ARG, "debug_run_cv_band: members would write the same entries");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  DebugDeviceBuf dP, dB, dC;
  if ((rc = debug_upload(h, dP, P, p_elems)) || (rc = debug_upload(h, dB, band, band_elems)) || (rc = debug_upload(h, dC, Cm, c_elems))) return rc;
  hipStream_t st = h->slots[0].s_upd;
  if ((rc = launch_cv_band_product(h, st, members, (const double*)dP.p, ld, (const double*)dB.p, (double*)dC.p, T, sP, sBand))) return rc;
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(Cm, dC.p, (size_t)c_elems * sizeof(double), hipMemcpyDeviceToHost));
  return SIGP_OK;
}

// predcov_partial_kernel through launch_predcov_partial, then (finish != 0) predcov_finish_kernel, with sigp_predict_cov's tile descriptor:
// S = 1 the in-place form (the partials go to C, `part` is not touched), S > 1 the workspace form part [S][P][128][128].  Cm [m_pad][m_pad] and
// part come in with the caller's sentinels and go back whole.  Kss [m_pad][ldk] or NULL (the prior of Xs [m_pad][dp] by kernel_id, ell).
int sigp_debug_run_predcov(sigp_handle* h, const double* Z, int64_t ldz, int m_pad, int nkb, int S, int finish, const double* Xs, int dp, int d, const double* Kss, int64_t ldk,
                           int kernel_id, double ell, double sn, double sigma_f, int noise, double* part, double* Cm, int64_t z_elems, int64_t xs_elems, int64_t kss_elems,
                           int64_t part_elems, int64_t c_elems) {
  constexpr long LIM = 1L << 28;
  if (!h || !Z || !part || !Cm || (!Xs && !Kss)) return SIGP_BAD_ARG;
  if (h->dtype != SIGP_F64) return fail(h, SIGP_BAD_ARG, "debug_run_predcov: fp64 only");
  if (m_pad < NB || m_pad % NB || m_pad > 2048 || nkb < 1 || nkb > 256) return fail(h, SIGP_BAD_ARG, "debug_run_predcov: m_pad / nkb");
  if (S < 1 || S > nkb) return fail(h, SIGP_BAD_ARG, "debug_run_predcov: 1 <= S <= nkb slices (a slice is never empty)");
  if (!Kss && ((kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) || !(ell > 0) || d < 1 || dp < d || dp > 4096))
    return fail(h, SIGP_BAD_ARG, "debug_run_predcov: without Kss the prior needs RBF / MATERN52, ell > 0 and Xs [m_pad][dp >= d]");
  const long c = m_pad / NB, P = c * (c + 1) / 2;
  if (ldz < (long)nkb * NB || ldz > LIM || (Kss && (ldk < m_pad || ldk > LIM)) || std::max({z_elems, xs_elems, kss_elems, part_elems, c_elems}) > LIM || z_elems < 1 ||
      part_elems < 1 || c_elems < 1)
    return fail(h, SIGP_BAD_ARG, "debug_run_predcov: strides");
  if (ldz % 2) return fail(h, SIGP_BAD_ARG, "debug_run_predcov: a row stride is not a multiple of 16 bytes");
  if ((long)(m_pad - 1) * ldz + (long)nkb * NB > z_elems || (long)m_pad * m_pad > c_elems || (S > 1 && (long)S * P * NB * NB > part_elems) ||
      (Kss && (long)(m_pad - 1) * ldk + m_pad > kss_elems) || (!Kss && (long)m_pad * dp > xs_elems))
    return fail(h, SIGP_BAD_ARG, "debug_run_predcov: the descriptor reaches outside the operand buffers");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  DebugDeviceBuf dZ, dX, dK, dW, dC;
  if ((rc = debug_upload(h, dZ, Z, z_elems)) || (rc = debug_upload(h, dW, part, part_elems)) || (rc = debug_upload(h, dC, Cm, c_elems))) return rc;
  if (Kss && (rc = debug_upload(h, dK, Kss, kss_elems))) return rc;
  if (!Kss && (rc = debug_upload(h, dX, Xs, xs_elems))) return rc;
  hipStream_t st = h->slots[0].s_upd;
  PredcovTiles t{};
  t.inplace = S == 1;
  if (t.inplace) { t.part = (double*)dC.p; t.tile_stride = 0; t.ldp = m_pad; t.slice_stride = 0; }
  else { t.part = (double*)dW.p; t.tile_stride = (long)NB * NB; t.ldp = NB; t.slice_stride = P * NB * NB; }
  if ((rc = launch_predcov_partial(h, st, (const double*)dZ.p, ldz, nkb, P, S, t))) return rc;
  if (finish) {
    PredcovFinish f{};
    f.t = t; f.S = S; f.C = (double*)dC.p; f.ldc = m_pad; f.Xs = (const double*)dX.p; f.dp = dp; f.d = d;
    f.Kss = (const double*)dK.p; f.ldk = ldk; f.kp = make_kparams(Kss ? SIGP_KERNEL_RBF : kernel_id, Kss ? 1.0 : ell, sn, 0); f.sigma_f = sigma_f; f.noise = noise != 0;
    hipLaunchKernelGGL(predcov_finish_kernel, dim3((unsigned)P, 16), dim3(256), 0, st, f);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(st));
  HIPCHK(h, hipMemcpy(part, dW.p, (size_t)part_elems * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(Cm, dC.p, (size_t)c_elems * sizeof(double), hipMemcpyDeviceToHost));
  return SIGP_OK;
}
