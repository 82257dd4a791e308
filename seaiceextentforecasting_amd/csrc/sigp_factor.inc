// Blocked Cholesky drivers of libsigp.so (host side; included by sigp.hip inside its anonymous namespace): the three panel primitives --
// diagonal block, column solve, lower-trapezoid update -- each written ONCE, the two panel forms built from them (latency chain,
// binary recursion) and the drivers on top: potrf_core (a slot's lockstep members, the fp32 engine) and the sharded fit's panel
// selectors (dist_panel, dist_panel_top).  A change of schedule is made here and nowhere else.

// Where a factorisation lives.  M = (virtual) origin of the storage, row stride ld, member stride matStride: a slot's square matrices,
// the fp32 engine's matrix, or one rank's block columns of a sharded factor (origin shifted so that GLOBAL block indices land in it).
template <typename Real>
struct FactorView {
  Real* M; long ld, matStride;
  Real* dinv; long dinvStride;       // inverse diagonal blocks, NB x NB each, block column c at dinv + c NB^2
  int nb;                            // lockstep members (one launch covers the same step of all of them)
  int* info;                         // the slot's pivot-failure flags, one per member
  Real* lk;                          // the slot's scratch block of the fused chain link
  Real* at(long rblk, long cblk) const { return M + rblk * NB * ld + cblk * NB; }
  Real* dinv_at(long cblk) const { return dinv + cblk * NB * NB; }
};
template <typename Real>
FactorView<Real> member_view(Slot& s, Real* Mm, long ld, Real* dinvp) {   // one member (the sharded fit)
  return FactorView<Real>{Mm, ld, 0L, dinvp, 0L, 1, s.info, (Real*)s.lk};
}

// What the panel forms take from their caller beyond the view (the sharded fit: all defaults).
struct PanelOpts {
  int ll = 0;                        // panel_rec: left-looking (sub)panels up to this width (option panel_ll)
  bool leaf_pairs = false;           // panel_rec: two-column leaves through the fused link (panel_chain bit 3)
  int patch = 0;                     // tile walk of the recursion's and the outer updates (option patch)
  int ride_R = 0, ride_rows = 0;     // ride16: an update down to row block ride_R multiplies only ride_rows rows of its last block row
};

// ---- primitive 1: diagonal block of column c (factor + inverse) ---------------------------------------------------------------
// riding (64-tile units, may be null) = an update whose tiles ride in the launch; linked: the launch follows a fused link of column
// c - 1 (B operand of block column c from the scratch block, which is also copied into the matrix)
template <typename Real>
int diag_block(sigp_handle* h, const FactorView<Real>& v, hipStream_t st, int c, const GemmArgsT<Real>* riding = nullptr, bool linked = false) {
  constexpr int diag_lds = diag_lds_bytes<Real>();
  constexpr int du_lds = std::max(diag_lds, 2 * gemm_lds_bytes<Real, 64, 64, false>());   // (fp32: the two update engines need more than the block)
  static AttrOnce du_attr, d_attr;
  const int nb = v.nb, flags = h->opt_diag_prio ? 0 : 32;
  const int ntile = riding ? gemm_grid_size(riding->r0, riding->r1, riding->c0, riding->c1, riding->lower, 0) : 0;
  const double uflops = riding ? nb * (double)ntile * 2.0 * 64 * 64 * riding->K : 0.0;
  ProfScope ps(h, st, SIGP_KC_DIAG, nb * 2.0 * NB * NB * NB / 3 + uflops, nb * 3.0 * NB * NB * 8 + nb * (double)ntile * 2.0 * 64 * 64 * sizeof(Real));
  Real* Ac = v.at(c, c);
  if (ntile > 0 || linked) {
    HIPCHK(h, du_attr.set(h->device, (const void*)diag_update_kernel<Real>, du_lds));
    // tile pairs per riding workgroup: in lockstep batches so many that about four riders per CU are left (see diag_update_kernel)
    const int pairs = (ntile + 1) / 2;
    const long want = h->opt_ride_reps > 0 ? h->opt_ride_reps : (h->opt_ride_reps < 0 ? ((long)nb * pairs + 4L * h->ncu - 1) / (4L * h->ncu) : 1);
    const int reps = (int)std::max<long>(1, std::min<long>(want, 32));
    const int wgs = (pairs + reps - 1) / reps;
    hipLaunchKernelGGL(diag_update_kernel<Real>, dim3(nb + nb * wgs + (linked ? nb : 0)), dim3(DIAG_THREADS), du_lds, st, Ac, v.ld, v.dinv_at(c), v.info, c * NB,
                       flags, v.matStride, v.dinvStride, nb, riding ? *riding : GemmArgsT<Real>{}, ntile, wgs, linked ? (const Real*)v.lk : (const Real*)nullptr,
                       (long)NB * NB, linked ? Ac - NB : (Real*)nullptr, reps);
  } else {
    HIPCHK(h, d_attr.set(h->device, (const void*)potrf_diag_kernel<Real>, diag_lds));
    hipLaunchKernelGGL(potrf_diag_kernel<Real>, dim3(nb), dim3(DIAG_THREADS), diag_lds, st, Ac, v.ld, v.dinv_at(c), v.info, c * NB, flags, v.matStride, v.dinvStride);
  }
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// ---- primitive 2: column solve  X = A inv(L_cc)^T ---------------------------------------------------------------------------------
// g carries the operands (A, B = the inverse diagonal block, C and their strides); `rows` 128-row blocks of nb members.  The tile
// choice (option trsm128_threshold) of every column solve of the library: the factorisation's and the sharded fit's row pieces.
template <typename Real>
int launch_column_solve(sigp_handle* h, hipStream_t st, GemmArgsT<Real> g, long rows, int nb) {
  if (rows <= 0) return SIGP_OK;
  g.batch = nb; g.K = NB; g.r0 = 0; g.c0 = 0; g.c1 = 1; g.lower = 0;
  ProfScope ps(h, st, SIGP_KC_TRSM, nb * 2.0 * rows * NB * NB * NB, nb * 2.0 * rows * NB * NB * 8);
  if (rows * nb >= h->opt_trsm128) {   // enough 128-row tiles to fill the chip: the LDS-DMA kernel
    g.r1 = (int)rows;
    return launch_syrk128_t<Real, true>(h, st, g);
  }
  g.r1 = (int)rows * 4;                // few rows: 32-row tiles for parallelism
  return launch_gemm_cfg<Real, 32, 128, 1, 4, GEMM_SET, false>(h, st, g);
}
// ---- primitive 2, refined (option accurate_solve, fp64): X = A inv(L)^T (TRANS: A inv(L)) with ONE residual-correction step against the
// diagonal block L itself, in place, one launch (refined_solve.hpp).  The launcher of every refined solve of the library: the
// factorisation's columns, the block solves of sigp_predict / sigp_predict_cov / sigp_get_alpha, and the debug library's run-and-return entry.
template <bool TRANS>
int launch_refined_solve(sigp_handle* h, hipStream_t st, const RefinedArgs& a, int nb) {
  if (a.rows <= 0 || nb <= 0) return SIGP_OK;
  static AttrOnce r_attr;
  ProfScope ps(h, st, SIGP_KC_TRSM, nb * 3.0 * 2.0 * a.rows * NB * NB, nb * (2.0 * a.rows * NB + 2.0 * NB * NB) * 8);
  HIPCHK(h, r_attr.set(h->device, (const void*)refined_solve_kernel<TRANS>, refined_lds_bytes()));
  hipLaunchKernelGGL(refined_solve_kernel<TRANS>, dim3((unsigned)((a.rows + RS_TM - 1) / RS_TM), (unsigned)nb), dim3(256), refined_lds_bytes(), st, a);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}
// rows_below 128-row blocks under the diagonal block of column c (the ride block is one of them when the rows reach it):
// L[c+1.., c] = A[c+1.., c] inv(L_cc)^T
template <typename Real>
int solve_column(sigp_handle* h, const FactorView<Real>& v, hipStream_t st, int c, int rows_below) {
  if constexpr (std::is_same<Real, double>::value) {
    if (h->opt_accurate) {             // option accurate_solve: the product and one residual correction against L_cc, one launch
      if (rows_below <= 0) return SIGP_OK;
      RefinedArgs a{v.at(c + 1, c), v.ld, v.matStride, v.dinv_at(c), (long)NB, v.dinvStride, v.at(c, c), v.ld, v.matStride, rows_below * NB};
      return launch_refined_solve<false>(h, st, a, v.nb);
    }
  }
  GemmArgsT<Real> g{};
  g.A = v.at(c + 1, c); g.lda = v.ld; g.sA = v.matStride;
  g.B = v.dinv_at(c); g.ldb = NB; g.sB = v.dinvStride;
  g.C = v.at(c + 1, c); g.ldc = v.ld; g.sC = v.matStride;
  return launch_column_solve<Real>(h, st, g, rows_below, v.nb);
}

// ---- primitive 3: lower-trapezoid update ---------------------------------------------------------------------------------------------
// columns ccol0 + [c0, c1), rows from each column's diagonal block to rlim,  -= P P^T  with  P = L[:, kcol0 .. kcol0 + kw)
template <typename Real>
GemmArgsT<Real> update_args(const FactorView<Real>& v, int kcol0, int kw, int ccol0, int c0, int c1, int rlim) {
  GemmArgsT<Real> g{};
  g.A = v.at(ccol0, kcol0); g.lda = v.ld;
  g.B = g.A; g.ldb = v.ld;
  g.C = v.at(ccol0, ccol0); g.ldc = v.ld;
  g.batch = v.nb; g.sA = g.sB = g.sC = v.matStride;
  g.K = kw * NB; g.r0 = 0; g.r1 = rlim - ccol0; g.c0 = c0; g.c1 = c1; g.lower = 1; g.patch = 0;
  return g;
}
// ... as a launch of its own, with the caller's tile walk and ride-block form
template <typename Real>
int trapezoid_update(sigp_handle* h, const FactorView<Real>& v, hipStream_t st, const PanelOpts& o, int kcol0, int kw, int ccol0, int c0, int c1, int rlim) {
  GemmArgsT<Real> g = update_args(v, kcol0, kw, ccol0, c0, c1, rlim);
  g.patch = o.patch;
  if (o.ride_rows > 0 && rlim == o.ride_R) { g.ride_bi1 = rlim - ccol0; g.ride_rows = o.ride_rows; }   // (block row R - 1 of the matrix = row R - 1 - ccol0 of this tile space)
  return gemm_sub_auto(h, st, g);
}

// ---- the launches of the two fused panel kernels (the engine's only ones; the debug library's run-and-return entries go through them too) ----
// chain_link_kernel: the 36 chain workgroups + 8 ride workgroups per 128-row block below block row c+1, of nb lockstep members
template <typename Real>
int launch_chain_link(sigp_handle* h, hipStream_t st, const LinkArgsT<Real>& a, int nb) {
  static AttrOnce l_attr;
  HIPCHK(h, l_attr.set(h->device, (const void*)chain_link_kernel<Real>, link_lds_bytes<Real>()));
  hipLaunchKernelGGL(chain_link_kernel<Real>, dim3((unsigned)(LINK_CHAIN_WGS + 8 * a.rows_ride), (unsigned)nb), dim3(256), link_lds_bytes<Real>(), st, a);
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}
// panel_strip_kernel: nstrips 128-row strips from row block a.rb0 down, of nb lockstep members (option strip_tri picks the instantiation)
template <typename Real>
int launch_panel_strip(sigp_handle* h, hipStream_t st, const StripArgsT<Real>& a, int nstrips, int nb) {
  if (!sy_row_stride_ok(a.ld, sizeof(Real)) || !sy_row_stride_ok(a.ldm, sizeof(Real))) return fail(h, SIGP_BAD_ARG, "panel_strip: row stride beyond the tile's 32-bit DMA offsets");
  static AttrOnce strip_attr, strip_attr_full;
  if (h->opt_strip_tri) {
    HIPCHK(h, strip_attr.set(h->device, (const void*)panel_strip_kernel<Real>, SY_LDS_BYTES));
    hipLaunchKernelGGL(panel_strip_kernel<Real>, dim3(nstrips, nb), dim3(256), SY_LDS_BYTES, st, a);
  } else {
    HIPCHK(h, strip_attr_full.set(h->device, (const void*)panel_strip_kernel<Real, false>, SY_LDS_BYTES));
    hipLaunchKernelGGL((panel_strip_kernel<Real, false>), dim3(nstrips, nb), dim3(256), SY_LDS_BYTES, st, a);
  }
  HIPCHK(h, hipGetLastError());
  return SIGP_OK;
}

// ---- a panel as a latency chain ---------------------------------------------------------------------------------------------
// Block columns [J0, J0 + Wp) of the view's lockstep members (already up to date), right-looking and column by column, arranged
// around the chain  diagonal block c -> what diagonal block c+1 needs -> diagonal block c+1:
//   fused link (panel_chain bit 2, chain_link.hpp): ONE launch between two diagonal blocks -- its first 36 workgroups form
//     L[c+1, c] and apply it to block (c+1, c+1); the column solve of the rows below rides in the same launch, the update of every
//     other block (column c+1 below its diagonal block, the panel's columns c+2..) rides in the launch of diagonal block c+1;
//   otherwise (and for columns with so many rows below that their solve is chip-filling work for the LDS-DMA kernel): column solve
//     (all rows), update of column c+1 (all rows), diagonal block c+1 with the update of the columns c+2.. riding.
// Same k order per tile as the binary recursion either way: bit-identical factors.
// rlim = one past the last row block touched (R for a whole panel, J0 + Wp for the top block of a strip-solved panel).
// on_col (may be null): called once block column c is final in the matrix (the sharded fit streams it to the other ranks).
template <typename Real>
int chain_panel(sigp_handle* h, const FactorView<Real>& v, hipStream_t sp, int J0, int Wp, int rlim, const std::function<int(int)>* on_col = nullptr) {
  const int nb = v.nb;
  int rc = diag_block(h, v, sp, J0);
  if (rc) return rc;
  for (int i = 0; i < Wp; ++i) {
    const int c = J0 + i;
    const int rows_below = rlim - (c + 1);
    const bool last = i + 1 >= Wp;
    // (the link's ride solves any number of rows, 16 per workgroup; beyond link_rows 128-row blocks x members the stand-alone LDS-DMA solve is the better kernel)
    // (option accurate_solve: no fused link -- its column solve is a plain product with the inverse block)
    const bool fused = !last && !h->opt_accurate && (h->opt_panel_chain & 4) != 0 && rows_below >= 1 && (long)rows_below * nb < h->opt_link_rows;
    if (!fused) {
      if ((rc = solve_column(h, v, sp, c, rows_below))) return rc;
      if (on_col && (rc = (*on_col)(c))) return rc;
      if (last) break;
      if ((rc = gemm_sub_auto(h, sp, update_args(v, c, 1, c + 1, 0, 1, rlim)))) return rc;
      const int rest = Wp - i - 2;                             // columns c+2 .. J0+Wp-1
      if (rest > 0) {
        GemmArgsT<Real> gu = update_args(v, c, 1, c + 1, 1, 1 + rest, rlim);
        gu.r0 *= 2; gu.r1 *= 2; gu.c0 *= 2; gu.c1 *= 2;
        rc = diag_block(h, v, sp, c + 1, &gu);
      } else {
        rc = diag_block(h, v, sp, c + 1);
      }
      if (rc) return rc;
      continue;
    }
    {
      LinkArgsT<Real> a{};
      a.Acol = v.at(c + 1, c); a.ld = v.ld;
      a.Linv = v.dinv_at(c);
      a.Cdiag = v.at(c + 1, c + 1);
      a.scratch = v.lk;
      a.sM = v.matStride; a.sL = v.dinvStride; a.sS = (long)NB * NB;
      a.rows_ride = rows_below - 1;
      ProfScope ps(h, sp, SIGP_KC_TRSM, nb * (2.0 * rows_below * NB * NB * NB + (double)NB * NB * NB), nb * 2.0 * rows_below * NB * NB * 8);
      if ((rc = launch_chain_link<Real>(h, sp, a, nb))) return rc;
    }
    GemmArgsT<Real> gu = update_args(v, c, 1, c + 1, 0, Wp - i - 1, rlim);   // columns c+1 .. J0+Wp-1 from row block c+2 down (block (c+1, c+1) is done)
    gu.r0 = 2; gu.r1 *= 2; gu.c0 *= 2; gu.c1 *= 2;
    if ((rc = diag_block(h, v, sp, c + 1, &gu, true))) return rc;
    if (on_col && (rc = (*on_col)(c))) return rc;              // (block row c+1 of column c reached the matrix in that launch)
  }
  return SIGP_OK;
}

// ---- a panel by binary recursion ----------------------------------------------------------------------------------------------------
// Block columns [J0, J0 + Wp) (already up to date): the left half, a rank-(half) update of the right half's columns, then the
// right half.  rlim and on_col as for chain_panel (on_col: right after the column solve of block column c has been enqueued).
template <typename Real>
int panel_rec(sigp_handle* h, const FactorView<Real>& v, hipStream_t sp, int J0, int Wp, int rlim, const PanelOpts& o, const std::function<int(int)>* on_col = nullptr) {
  int rc;
  if (Wp == 1) {
    if ((rc = diag_block(h, v, sp, J0))) return rc;
    if ((rc = solve_column(h, v, sp, J0, rlim - (J0 + 1)))) return rc;
    return on_col ? (*on_col)(J0) : SIGP_OK;
  }
  if (o.ll && Wp <= o.ll) {
    // left-looking inside a (sub)panel: column block c is updated once with all earlier columns of the panel
    // (K = 128 (c-J0)), then factored: each panel column is read/written once and the average K doubles
    for (int i = 0; i < Wp; ++i) {
      if (i > 0 && (rc = trapezoid_update(h, v, sp, o, J0, i, J0 + i, 0, 1, rlim))) return rc;
      if ((rc = panel_rec(h, v, sp, J0 + i, 1, rlim, o, on_col))) return rc;
    }
    return SIGP_OK;
  }
  if (Wp == 2 && o.leaf_pairs && rlim - J0 >= 2)   // the recursion's leaf pairs through the fused link: D, link, D + riding update of the second column, solve
    return chain_panel(h, v, sp, J0, 2, rlim, on_col);
  const int hw = Wp / 2;
  if ((rc = panel_rec(h, v, sp, J0, hw, rlim, o, on_col))) return rc;
  if ((rc = trapezoid_update(h, v, sp, o, J0, hw, J0 + hw, 0, Wp - hw, rlim))) return rc;
  return panel_rec(h, v, sp, J0 + hw, Wp - hw, rlim, o, on_col);
}

// block columns per outer panel
// (a single fit of at most 24 block columns, unless the caller chose: ONE panel -- no panel boundary (each is a trailing update in series with the
//  chain), and the right-looking rides of such a panel still fit beside its diagonal blocks: n = 2048 0.670 ms (16) vs 0.715 (8), n = 3072 1.082
//  (24) vs 1.126 (16) / 1.122 (8).  From there on the rides of the first columns outlast the diagonal block: n = 4096 1.653 (8) / 1.675 (16) / 1.755 (32);
//  tools/single_sweep.py)
// (fp32 fits from 192 block columns on: the fp32 update runs its K = 1024 tile in half the time of the fp64 one, so the tile's C read +
//  write weighs twice as much -- K = 2048 instead: n = 32768 102.95 vs 104.4 ms (12: 103.3, 24: 104.1, 32: 106.3); n = 16384 19.2 vs 19.05: not there)
inline int outer_width(const sigp_handle* h, int nb, int T, bool f32 = false) {
  if (!h->outer_set && f32 && T >= 192) return 16;             // (a lockstep group of 4 at n = 32768: 97.7 vs 98.6-99.0 ms per fit)
  return (!h->outer_set && nb == 1 && T <= 24 && (h->opt_panel_chain & 4)) ? std::max(1, T) : std::max(1, h->opt_outer);
}

// ---- blocked Cholesky of the nb lockstep members of slot s (each augmented with its ride rows) --------
// Every launch covers the same step of all nb factorisations (grid.y / grid.x = member), so launches stay
// GPU-filling as the trailing matrices shrink and the per-step latency chain is paid once per nb fits.
// PotrfRun = one call of potrf_core: what its pieces (panel top and strips, the two outer schedules) share
template <typename Real>
struct PotrfRun {
  sigp_handle* h; Slot& s; FactorView<Real> v; PanelOpts po;
  int T, R, W;                       // column blocks, row blocks including the ride block, block columns per outer panel
  bool la; hipStream_t sp, su;       // lookahead: panels on their own stream sp beside the update stream su

  // top = the top block of a strip-solved panel.  A whole panel takes the chain form only while its riding updates (K = 128, 64x64
  // tiles: 4 flop per operand byte) stay shorter than the diagonal block they ride beside: up to chain_rows (80) 128-row blocks x
  // members below the panel's first column (n = 32768 in fp32 is 4 % faster with the recursion's K = 256 / 512 updates)
  int panel_any(int J0, int Wp, int rlim, bool top) const {
    const bool chain = Wp > 2 && (top ? (h->opt_panel_chain & 2) != 0 : ((h->opt_panel_chain & 1) != 0 && (long)(rlim - J0) * v.nb <= h->opt_chain_rows));
    return chain ? chain_panel(h, v, sp, J0, Wp, rlim) : panel_rec(h, v, sp, J0, Wp, rlim, po);
  }
  // factor block columns [J0, J0+Wp): panel_top = everything on the panel stream up to the strip solve (the whole panel when it
  // is not strip-solved); panel_strips = the Mt products + strip kernel for the rows below the top block (no-op otherwise)
  bool use_strips(int J0, int Wp) const {
    const int below = R - (J0 + Wp);             // row blocks under the panel's top block (the ride block is one of them)
    // (option accurate_solve: no strip solves -- a strip is a product with the inverse of the panel's whole top triangle)
    return std::is_same<Real, double>::value && !h->opt_accurate && Wp > 1 && Wp <= MT_W && below > 0 &&
           (h->opt_panel_mode == 1 || (h->opt_panel_mode == 2 && (long)below * v.nb >= h->opt_strip_min));
  }
  int panel_top(int J0, int Wp) const {
    // panel_mode 1: recursion on the top Wp x Wp block only, then every 128-row strip below it is solved by one
    // workgroup walking the panel's columns (panel_strip_kernel): the lower rows are read and written once
    return use_strips(J0, Wp) ? panel_any(J0, Wp, J0 + Wp, true) : panel_any(J0, Wp, R, false);
  }
  int panel_strips(int J0, int Wp) const {
    if (!use_strips(J0, Wp)) return SIGP_OK;
    const int below = R - (J0 + Wp), nb = v.nb;
    int rc;
    Real* mt = (Real*)s.mt;
    const long mtStride = MT_LD * MT_LD;
    {
      ProfScope ps(h, sp, SIGP_KC_UPDATE_SMALL, nb * 2.0 * NB * NB * NB * (Wp * (Wp - 1) / 2), nb * 3.0 * NB * NB * 8 * (Wp * (Wp + 1) / 2));
      hipLaunchKernelGGL(mt_diag_kernel<Real>, dim3(Wp, nb), dim3(256), 0, sp, v.dinv_at(J0), v.dinvStride, mt, MT_LD, mtStride);
      HIPCHK(h, hipGetLastError());
      for (int j = 1; j < Wp; ++j) {             // Mt[j, 0:j] = -inv(L_jj) L[j, 0:j]
        GemmArgsT<Real> g{};
        g.A = v.dinv_at(J0 + j); g.lda = NB; g.sA = v.dinvStride;
        g.B = v.at(J0 + j, J0); g.ldb = v.ld; g.sB = v.matStride;     // K x N row-major (BT)
        g.C = mt + (long)j * NB * MT_LD; g.ldc = MT_LD; g.sC = mtStride;
        g.batch = nb; g.K = NB; g.r0 = 0; g.r1 = 4; g.c0 = 0; g.c1 = j; g.lower = 0;
        if ((rc = launch_gemm_cfg<Real, 32, 128, 1, 4, GEMM_SETNEG, true>(h, sp, g))) return rc;
      }
    }
    {
      ProfScope ps(h, sp, SIGP_KC_TRSM, nb * (double)below * 2.0 * NB * NB * NB * (Wp * (Wp + 1) / 2), nb * (double)below * 2.0 * Wp * NB * NB * 8);
      StripArgsT<Real> a{v.M, v.ld, v.matStride, mt, MT_LD, mtStride, J0 + Wp, J0, Wp};
      if ((rc = launch_panel_strip<Real>(h, sp, a, below, nb))) return rc;
    }
    return SIGP_OK;
  }
  int panel(int J0, int Wp) const {
    int rc = panel_top(J0, Wp);
    return rc ? rc : panel_strips(J0, Wp);
  }
  // trailing update of columns J+Wc + [c0, c1) with panel [J, J+Wc), all rows
  int outer(hipStream_t st, int J, int Wc, int c0, int c1) const {
    // persistent form (update_wgs): only for outer trailing updates, and with update_late only for the last panels, where the
    // updates are small and the panel chain they share the chip with is what the step waits for
    const int panels_left = (T - (J + Wc) + W - 1) / W;
    h->persist_now = h->opt_update_wgs > 0 && (h->opt_update_late == 0 || panels_left <= h->opt_update_late);
    const int rc_ = trapezoid_update(h, v, st, po, J, Wc, J + Wc, c0, c1, R);
    h->persist_now = false;
    return rc_;
  }

  // Left-looking outer schedule (panel 0 is factored): panel q (columns J..J+Wq) is brought up to date in two launches,
  //   A(q): C_q -= L[:, 0 : J-W] L[q rows, 0 : J-W]^T   (all panels but the last one: K = 128 (J-W), up to n - 2*128 W)
  //   B(q): C_q -= P_{q-1} P_{q-1}^T                    (the panel factored last: K = 128 W)
  // and then factored, F(q).  A(q+1) only needs panels 0..q-1, so it runs on the update stream while the panel
  // stream does B(q), F(q).  Each C tile is read and written twice per panel instead of once per EARLIER panel,
  // and almost all flops run at K >= 1024.  The k order of every tile's sum is the same as in the right-looking
  // schedule (panels in order, k ascending), so the factor is bit-identical.
  int left_looking() const {
    int rc;
    hipEvent_t evF[2] = {s.ev_pan, s.ev_done};
    if (la) HIPCHK(h, hipEventRecord(evF[0], sp));                 // F(0)
    int q = 1;
    for (int J = W; J < T; J += W, ++q) {
      const int Wq = std::min(W, T - J);
      if (la) {
        if (q >= 2) {
          HIPCHK(h, hipStreamWaitEvent(su, evF[q & 1], 0));          // F(q-2) done (same parity as q)
          if ((rc = trapezoid_update(h, v, su, po, 0, J - W, J, 0, Wq, R))) return rc;    // A(q)
          HIPCHK(h, hipEventRecord(s.ev_la, su));
          HIPCHK(h, hipStreamWaitEvent(sp, s.ev_la, 0));
        }
        if ((rc = trapezoid_update(h, v, sp, po, J - W, W, J, 0, Wq, R))) return rc;      // B(q), after F(q-1) in stream order
        if ((rc = panel(J, Wq))) return rc;                                      // F(q)
        HIPCHK(h, hipEventRecord(evF[q & 1], sp));
      } else {
        if ((rc = trapezoid_update(h, v, su, po, 0, J, J, 0, Wq, R))) return rc;          // A(q)+B(q) in one launch
        if ((rc = panel(J, Wq))) return rc;
      }
    }
    if (la) {
      HIPCHK(h, hipEventRecord(s.ev_pan, sp));
      HIPCHK(h, hipStreamWaitEvent(su, s.ev_pan, 0));
    }
    return SIGP_OK;
  }

  // Right-looking outer schedule (panel 0 is factored): each panel updates the whole trailing matrix, the next panel's columns first
  int right_looking() const {
    int rc;
    bool have_rest = false;                      // first_on_panel: an update of the rest of the trailing matrix is in flight on su
    bool tail_marked = false;                    // ev_tail recorded (pipeline_head = 3)
    for (int J = 0; J < T; J += W) {
      const int Wc = std::min(W, T - J);
      const int ncols = T - (J + Wc);            // trailing column blocks
      if (ncols <= 0) break;
      const int Wn = std::min(W, ncols);         // width of the next panel
      if (la && !tail_marked && ncols <= h->opt_head_gate) {   // panel J is the last one before the tail: the next group's head may start behind it
        HIPCHK(h, hipEventRecord(s.ev_tail, sp));
        tail_marked = true;
      }
      if (la && (h->opt_first_on_panel == 2 || (h->opt_first_on_panel == 1 && !use_strips(J + Wc, Wn)))) {
        // The update of the NEXT panel's columns stays on the panel stream (stream order, no inter-queue hand-off in the chain
        // panel -> first update -> next panel: each hand-off is a barrier packet pair, 11-13 us measured); the update stream gets
        // the rest of the trailing matrix, which the panel stream only has to see finished one panel later.
        if (have_rest) HIPCHK(h, hipStreamWaitEvent(sp, s.ev_done, 0));   // rest(J - W) wrote these columns too
        if ((rc = outer(sp, J, Wc, 0, Wn))) return rc;
        HIPCHK(h, hipEventRecord(s.ev_pan, sp));            // panel J and the first update done: the rest starts behind them, so the
        HIPCHK(h, hipStreamWaitEvent(su, s.ev_pan, 0));     // update the chain waits for has the chip to itself
        have_rest = ncols > Wn;
        if (have_rest) {
          if ((rc = outer(su, J, Wc, Wn, ncols))) return rc;
          HIPCHK(h, hipEventRecord(s.ev_done, su));
        }
        if (h->opt_strips_after_update && use_strips(J + Wc, Wn)) {
          if ((rc = panel_top(J + Wc, Wn))) return rc;
          if (have_rest) HIPCHK(h, hipStreamWaitEvent(sp, s.ev_done, 0));
          if ((rc = panel_strips(J + Wc, Wn))) return rc;
        } else if ((rc = panel(J + Wc, Wn))) return rc;
      } else if (la) {
        HIPCHK(h, hipEventRecord(s.ev_pan, sp));            // panel J done
        HIPCHK(h, hipStreamWaitEvent(su, s.ev_pan, 0));
        if ((rc = outer(su, J, Wc, 0, Wn))) return rc;      // next panel's columns first
        HIPCHK(h, hipEventRecord(s.ev_la, su));
        HIPCHK(h, hipStreamWaitEvent(sp, s.ev_la, 0));
        if (h->opt_strips_after_update && use_strips(J + Wc, Wn)) {
          // only the next panel's top block (a latency chain of small launches) overlaps the rest of the update; its strip solve --
          // MFMA work for the whole chip -- starts when that update is done instead of sharing the chip with it
          if ((rc = panel_top(J + Wc, Wn))) return rc;
          if ((rc = outer(su, J, Wc, Wn, ncols))) return rc;
          HIPCHK(h, hipEventRecord(s.ev_done, su));
          HIPCHK(h, hipStreamWaitEvent(sp, s.ev_done, 0));
          if ((rc = panel_strips(J + Wc, Wn))) return rc;
        } else {
          if ((rc = panel(J + Wc, Wn))) return rc;          // next panel overlaps the rest of the update
          if ((rc = outer(su, J, Wc, Wn, ncols))) return rc;
          HIPCHK(h, hipEventRecord(s.ev_done, su));         // (a later panel may take the first_on_panel form and wait for this)
        }
        have_rest = ncols > Wn;
      } else {
        if ((rc = outer(su, J, Wc, 0, ncols))) return rc;
        if ((rc = panel(J + Wc, Wn))) return rc;
      }
    }
    if (la) {   // join: the update stream is the slot's completion stream
      if (!tail_marked) HIPCHK(h, hipEventRecord(s.ev_tail, sp));
      HIPCHK(h, hipEventRecord(s.ev_pan, sp));
      HIPCHK(h, hipStreamWaitEvent(su, s.ev_pan, 0));
    }
    return SIGP_OK;
  }
};

template <typename Real>
int potrf_core(sigp_handle* h, Slot& s, Real* M, long matStride, Real* dinvp, long dinvStride, int nb, long n_pad, bool head_on_panel = false,
               int ride_rows = RIDE) {
  const int T = (int)(n_pad / NB);   // column blocks
  const int R = T + 1;               // row blocks including the ride block
  const bool la = h->opt_lookahead != 0;
  PotrfRun<Real> run{h, s, FactorView<Real>{M, n_pad, matStride, dinvp, dinvStride, nb, s.info, (Real*)s.lk}, PanelOpts{}, T, R,
                     outer_width(h, nb, T, std::is_same<Real, float>::value), la, la ? s.s_pan : s.s_upd, s.s_upd};
  run.po.ll = h->opt_panel_ll; run.po.leaf_pairs = (h->opt_panel_chain & 8) != 0; run.po.patch = h->opt_patch;
  // ride_rows: rows of the ride-along block in use (y + the test points; the rest are zero rows).  Up to 16: the block row's tiles in the
  // trailing updates multiply their first 16-row sub-tile only (syrk128_tile's RD form)
  if (h->opt_ride_tiles && h->opt_diag_tiles && ride_rows <= 16) { run.po.ride_R = R; run.po.ride_rows = ride_rows; }   // (the RD form lives in the kernel instantiation that has the DG form)
  if (std::is_same<Real, double>::value && (h->opt_panel_mode == 1 || (h->opt_panel_mode == 2 && (long)R * nb >= h->opt_strip_min))) {
    int rcm = slot_ensure_mt(h, s, nb);
    if (rcm) return rcm;
  }
  // head_on_panel (lockstep batches, head pipelining): the covariance build of this group was enqueued on the PANEL stream and
  // the update stream starts with a wait for the previous group, so the build and the first panel run while the previous
  // group is still updating; nothing of this group's head may then be ordered behind the update stream
  const bool head = head_on_panel && la;
  HIPCHK(h, hipMemsetAsync(s.info, 0, (size_t)nb * sizeof(int), head ? run.sp : run.su));
  if (la && !head) {   // panel stream starts after the build on the update stream
    HIPCHK(h, hipEventRecord(s.ev_la, run.su));
    HIPCHK(h, hipStreamWaitEvent(run.sp, s.ev_la, 0));
  }
  int rc = run.panel(0, std::min(run.W, T));
  if (rc) return rc;
  return h->opt_schedule == 1 ? run.left_looking() : run.right_looking();
}

int potrf_slot(sigp_handle* h, Slot& s, int nb, long n_pad, bool head_on_panel = false, int ride_rows = RIDE) {
  return potrf_core<double>(h, s, s.mat, s.matStride, s.dinv, s.dinvStride, nb, n_pad, head_on_panel, ride_rows);
}

// ---- the sharded fit's panels (one member; sigp_shard.inc) -----------------------------------------------------------------------------------------------
// Mm = (virtual) origin of one rank's block columns (ld = its column count, origin shifted so that GLOBAL column indices land in it);
// on_col as above (the sharded fit streams a final column to the other ranks while the chain goes on).  Whole panels: the latency
// chain under the conditions of potrf_core's whole panels, else the plain recursion (no left-looking sub-panels, no leaf pairs).
template <typename Real>
int dist_panel(sigp_handle* h, Slot& s, Real* Mm, long ld, Real* dinvp, hipStream_t sp, long n_pad, int J0, int Wp, const std::function<int(int)>* on_col = nullptr) {
  const int R = (int)(n_pad / NB) + 1;
  const FactorView<Real> v = member_view(s, Mm, ld, dinvp);
  if (!(h->opt_panel_chain & 1) || Wp <= 2 || (long)(R - J0) > h->opt_chain_rows) return panel_rec(h, v, sp, J0, Wp, R, PanelOpts{}, on_col);
  return chain_panel(h, v, sp, J0, Wp, R, on_col);
}
// the top W x W block of panel [J0, J0 + Wp) only (rows below it are somebody else's work): always the chain
template <typename Real>
int dist_panel_top(sigp_handle* h, Slot& s, Real* Mm, long ld, Real* dinvp, hipStream_t sp, int J0, int Wp) {
  return chain_panel(h, member_view(s, Mm, ld, dinvp), sp, J0, Wp, J0 + Wp);
}
