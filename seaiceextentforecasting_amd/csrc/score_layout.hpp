// The layouts of the workspaces the score and gradient entry points share (sigp_nlml_grad*, sigp_loo*, sigp_cv*): one small view per
// layout, its size and its accessors derived from the same fields, so that what an entry asks ensure() for and what its launches and
// read-backs address cannot part ways.  The host builds a view after it has grown the arena (sigp_scores.inc: the *_ensure helpers) and
// hands it to the launch helpers; kernels take LooGradVecs and LooArdVecs by value.  A view owns nothing.
// Plain C++ (no HIP include), so that a host compiler can check the arithmetic: tests/test_score_layout_host.py.
//
// Arena (sigp_handle)   view                 who
//   gPart               ScoreParts           sigp_loo, sigp_cv, sigp_loo_grad and their batch forms
//                       ScoreArdParts        sigp_loo_grad_ard, sigp_cv_grad_ard: ScoreParts of one member, then the tile pass's partials
//                       MliiParts            sigp_nlml_grad
//                       MliiGroupParts       sigp_nlml_grad_batch
//                       ArdParts             sigp_nlml_grad_ard, sigp_nlml_grad_ard_batch
//                       LooArdGroupParts     sigp_loo_grad_ard_batch, sigp_cv_grad_ard_batch, sigp_hindcast_grad_ard_batch: ScoreParts of G members, then
//                                            ArdParts of G members
//   gV                  LooGradVecs          sigp_loo_grad(_batch)
//                       LooArdVecs           sigp_loo_grad_ard, sigp_cv_grad_ard
//                       LooArdGroupVecs      sigp_loo_grad_ard_batch, sigp_cv_grad_ard_batch: G LooArdVecs at an even member stride
//                       HindcastVecs         sigp_hindcast, sigp_hindcast_batch (G of them, size() apart)
//                       HindcastArdVecs      sigp_hindcast_grad_ard: HindcastVecs, then LooArdVecs
//                       HindcastArdGroupVecs sigp_hindcast_grad_ard_batch: G HindcastArdVecs at an even member stride
//   cvPart cvBlk cvVec  CvWork               cv_launch
//   cvAdj               CvAdjStore           sigp_cv_grad_ard; it fills the CvAdjoint that cv_launch and the kernels take
//                       CvAdjGroupStore      sigp_cv_grad_ard_batch: the same pieces for the nb members of a lockstep group
//   bStage              ArdStage             sigp_batch_run_ard, sigp_nlml_grad_ard_batch, sigp_loo_grad_ard_batch, sigp_cv_grad_ard_batch,
//                                            sigp_hindcast_grad_ard_batch
// gU, gK, gD [G][n_pad][n_pad], scratchZ and ardXc are used whole: they have no layout beyond their size.
// Everything is in doubles.  n_pad is a multiple of 128, dp of 64, wp of 16.
#pragma once

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace sigp {

constexpr long SL_BLK = 128;            // the 128-block: NB, RIDE, CV_MAXW and SY_T of the kernels (sigp.hip asserts that they agree)
constexpr long SL_BAND = 3 * SL_BLK;    // columns of a row of the band store (CVA_BAND)

// hands out consecutive pieces of an arena: take(len) is the offset of the next piece, at the total once all are taken
struct Carve {
  long at = 0;
  __host__ __device__ long take(long len) { const long o = at; at += len; return o; }
};

// ---- gPart -----------------------------------------------------------------------------------------------------------------------------------
// The score entries: per member [4][n_pad] (mean, var and the two rows of score terms), then 4 doubles per member of sums: [G][2] scores;
// a single fit (G = 1): score [2], q = y^T A~, one spare.  The sums lie behind the rows of the G members the arena is laid out for, NOT of
// the nb <= G members a group has: a partial last group leaves rows unused and finds its sums where a full group does.
struct ScoreParts {
  double* base; long G, n_pad;
  __host__ __device__ static long size(long G, long n_pad) { return G * (4 * n_pad + 4); }
  __host__ __device__ long mstride() const { return 4 * n_pad; }                 // member m's rows at base + m * mstride()
  __host__ __device__ double* mean(long m) const { return base + m * mstride(); }
  __host__ __device__ double* var(long m) const { return mean(m) + n_pad; }
  __host__ __device__ double* sums() const { return base + G * mstride(); }      // member m's two scores at sums() + 2 m
  __host__ __device__ double* q() const { return sums() + 2; }                   // G = 1 only: with G > 1 it is member 1's scores
};

// ... of one member, then the ARD pass's tile partials [tiles][dp] and the gradient (d + 1 of the dp + 1 doubles kept for it)
struct ScoreArdParts {
  double* base; long n_pad, tiles, dp;
  __host__ __device__ static long size(long n_pad, long tiles, long dp) { return ScoreParts::size(1, n_pad) + tiles * dp + dp + 1; }
  __host__ __device__ ScoreParts scores() const { return ScoreParts{base, 1, n_pad}; }
  __host__ __device__ double* partial() const { return base + ScoreParts::size(1, n_pad); }
  __host__ __device__ double* grad() const { return partial() + tiles * dp; }
};

// sigp_nlml_grad: [n][4] terms (T(D), Q(D), tr K~^-1, A~^T A~ per row), summed on the host
struct MliiParts {
  double* base;
  __host__ __device__ static long size(long n_pad) { return 4 * n_pad; }
  __host__ __device__ double* rows() const { return base; }
};

// sigp_nlml_grad_batch: per member [n_pad][4] terms, then -- behind the G members the arena is laid out for, as ScoreParts' -- [G][4] sums
struct MliiGroupParts {
  double* base; long G, n_pad;
  __host__ __device__ static long size(long G, long n_pad) { return G * (4 * n_pad + 4); }
  __host__ __device__ long mstride() const { return 4 * n_pad; }
  __host__ __device__ double* rows() const { return base; }
  __host__ __device__ double* sums() const { return base + G * mstride(); }      // member m's four sums at sums() + 4 m
};

// The per-feature MLII gradient: per member the tile partials [tiles][dp], then -- behind all G members' -- the gradients, gw doubles kept
// per member: the lockstep groups keep and use d + 1 (member m's at grad() + m (d + 1)), the single fit keeps dp + 1 and uses d + 1.
struct ArdParts {
  double* base; long G, tiles, dp, gw;
  __host__ __device__ static long size(long G, long tiles, long dp, long gw) { return G * (tiles * dp + gw); }
  __host__ __device__ long mstride() const { return tiles * dp; }
  __host__ __device__ double* partial() const { return base; }
  __host__ __device__ double* grad() const { return base + G * mstride(); }
};

// The per-feature gradient of a leave-one-out score for a lockstep group: ScoreParts of G members (the sums behind all G members' rows, as
// ever), then ArdParts of G members keeping gw = d + 1 gradient entries each.
struct LooArdGroupParts {
  double* base; long G, n_pad, tiles, dp, gw;
  __host__ __device__ static long size(long G, long n_pad, long tiles, long dp, long gw) { return ScoreParts::size(G, n_pad) + ArdParts::size(G, tiles, dp, gw); }
  __host__ __device__ ScoreParts scores() const { return ScoreParts{base, G, n_pad}; }
  __host__ __device__ ArdParts ard() const { return ArdParts{base + ScoreParts::size(G, n_pad), G, tiles, dp, gw}; }
};

// ---- gV --------------------------------------------------------------------------------------------------------------------------------------
// Per-member vector workspace of sigp_loo_grad's gradient pass: a, t, b (= P t), P a, sum_k P_ik^2 [n_pad each], the column pass's partial
// sums [n_pad / 128][n_pad], the four gradient components.  a and t are read in 16-byte pairs: every row starts at an even offset, and
// the member stride size(n_pad) is even.
struct LooGradVecs {
  double* base; long stride;        // member m at base + m * stride
  long n_pad; int T;                // T = n_pad / 128 row chunks of the column pass
  __host__ __device__ static long size(long n_pad) { return (5 + n_pad / 128) * n_pad + 4; }
  __host__ __device__ double* a(int m) const { return base + m * stride; }
  __host__ __device__ double* t(int m) const { return a(m) + n_pad; }
  __host__ __device__ double* b(int m) const { return a(m) + 2 * n_pad; }
  __host__ __device__ double* pa(int m) const { return a(m) + 3 * n_pad; }
  __host__ __device__ double* pp(int m) const { return a(m) + 4 * n_pad; }
  __host__ __device__ double* cpart(int m) const { return a(m) + 5 * n_pad; }
  __host__ __device__ double* out(int m) const { return a(m) + (5 + T) * n_pad; }
};

// Vector workspace of the ARD pass of a leave-one-out / leave-block-out score: a, beta, gamma, v [n_pad each], then eps.  The four vectors
// are read in 16-byte pairs: even offsets.
struct LooArdVecs {
  double* base; long n_pad;
  __host__ __device__ static long size(long n_pad) { return 4 * n_pad + 1; }
  __host__ __device__ double* a() const { return base; }
  __host__ __device__ double* beta() const { return base + n_pad; }
  __host__ __device__ double* gamma() const { return base + 2 * n_pad; }
  __host__ __device__ double* v() const { return base + 3 * n_pad; }
  __host__ __device__ double* eps() const { return base + 4 * n_pad; }
};

// ... of the G members of a lockstep group.  LooArdVecs::size is odd and the vectors are read in 16-byte pairs, so the members lie
// mstride() = 4 n_pad + 2 apart (even; one double spare behind eps): member b is the LooArdVecs at base + b mstride().
struct LooArdGroupVecs {
  double* base; long n_pad, G;
  __host__ __device__ static long size(long G, long n_pad) { return G * (4 * n_pad + 2); }
  __host__ __device__ long mstride() const { return 4 * n_pad + 2; }
  __host__ __device__ LooArdVecs member(long b) const { return LooArdVecs{base + b * mstride(), n_pad}; }
};

// Per-member vector workspace of the hindcast entries (hindcast.hpp): cum (prefix sums of z^2), then -- the gradient alone -- r, w, rho,
// ks (= kappa sigma), suf, zbar [n_pad each].  Read one double at a time.
struct HindcastVecs {
  double* base; long n_pad;
  __host__ __device__ static long size(long n_pad) { return 7 * n_pad; }
  __host__ __device__ double* cum() const { return base; }
  __host__ __device__ double* r() const { return base + n_pad; }
  __host__ __device__ double* w() const { return base + 2 * n_pad; }
  __host__ __device__ double* rho() const { return base + 3 * n_pad; }
  __host__ __device__ double* ks() const { return base + 4 * n_pad; }
  __host__ __device__ double* suf() const { return base + 5 * n_pad; }
  __host__ __device__ double* zbar() const { return base + 6 * n_pad; }
};

// sigp_hindcast_grad_ard: HindcastVecs of the one member, then the LooArdVecs the ARD pass takes (a, v and eps are zero here: the adjoint is
// the matrix G alone).  7 n_pad is even, so the LooArdVecs' 16-byte reads stay aligned.
struct HindcastArdVecs {
  double* base; long n_pad;
  __host__ __device__ static long size(long n_pad) { return HindcastVecs::size(n_pad) + LooArdVecs::size(n_pad); }
  __host__ __device__ HindcastVecs hc() const { return HindcastVecs{base, n_pad}; }
  __host__ __device__ LooArdVecs ard() const { return LooArdVecs{base + HindcastVecs::size(n_pad), n_pad}; }
};

// sigp_hindcast_grad_ard_batch: G members of HindcastArdVecs -- HindcastVecs, then the LooArdVecs the ARD pass takes -- mstride() = 11 n_pad + 2
// apart: HindcastArdVecs::size is odd and the LooArdVecs are read in 16-byte pairs, so one double is spare behind every member's eps, as in
// LooArdGroupVecs.  hc(0) and ard(0) are member 0's views; the launches reach member b at b mstride() behind them.
struct HindcastArdGroupVecs {
  double* base; long n_pad, G;
  __host__ __device__ static long size(long G, long n_pad) { return G * (HindcastArdVecs::size(n_pad) + 1); }
  __host__ __device__ long mstride() const { return HindcastArdVecs::size(n_pad) + 1; }
  __host__ __device__ HindcastArdVecs member(long b) const { return HindcastArdVecs{base + b * mstride(), n_pad}; }
};

// The dynamic LDS of hindcast_w_lds_kernel (hindcast.hpp): the row piece of U and the rank-one part of the row of W, n_pad doubles each and
// one double of skew per 32; the kernel's scan totals (2 KB, static) come on top.  A group takes that kernel while n_pad is at most
// HINDCAST_W_LDS_MAX_NPAD -- 132 KB of the 160 KB a workgroup may have -- and hindcast_w_kernel beyond it.
constexpr long HINDCAST_W_LDS_MAX_NPAD = 8192;
__host__ __device__ constexpr long hindcast_w_lds_row(long n_pad) { return n_pad + n_pad / 32; }
__host__ __device__ constexpr long hindcast_w_lds_bytes(long n_pad) { return 2 * hindcast_w_lds_row(n_pad) * 8; }
__host__ __device__ constexpr bool hindcast_w_use_lds(long n_pad) { return n_pad <= HINDCAST_W_LDS_MAX_NPAD; }

// ---- cvPart, cvBlk, cvVec ----------------------------------------------------------------------------------------------------------------------
// The work buffers of one pass of cv_launch over `blocks` (member, fold) pairs with S K-slices and windows of at most wp rows:
//   cvPart  part [blocks][S][wp][wp], apart [blocks][S][wp]      the slices' shares of P_SS and a_S
//   cvBlk   Pb, Xb [blocks][128][128]                            P_SS, then its factor's inverse
//   cvVec   av [blocks][128], then info [blocks]                 a_S; the pivot tests' results: `int` inside a buffer of doubles, one double
//                                                                kept per block
struct CvWork {
  double *cvPart, *cvBlk, *cvVec; long blocks, S, wp;
  __host__ __device__ static long part_size(long blocks, long S, long wp) { return blocks * S * (wp * wp + wp); }
  __host__ __device__ static long blk_size(long blocks) { return 2 * blocks * SL_BLK * SL_BLK; }
  __host__ __device__ static long vec_size(long blocks) { return blocks * (SL_BLK + 1); }
  __host__ __device__ double* part() const { return cvPart; }
  __host__ __device__ double* apart() const { return cvPart + blocks * S * wp * wp; }
  __host__ __device__ double* Pb() const { return cvBlk; }
  __host__ __device__ double* Xb() const { return cvBlk + blocks * SL_BLK * SL_BLK; }
  __host__ __device__ double* av() const { return cvVec; }
  __host__ __device__ int* info() const { return (int*)(cvVec + blocks * SL_BLK); }
};

// ---- cvAdj -----------------------------------------------------------------------------------------------------------------------------------
// What cv_launch does for the gradient when it is given one of these (sigp_cv_grad_ard, sigp_cv_grad_ard_batch): the fold adjoints of each
// pass and their assembly.  Of a lockstep group: member m's band store, beta and eps_f at m times the strides; a single fit has zero strides.
struct CvAdjoint {
  int crit;          // 0 nlpd, 1 sse
  double* Bf;        // [(member, fold) pairs of a pass][wp][wp]  (lower 16 x 16 subtiles written)
  double* betaf;     // [pairs of a pass][wp]
  double* epsf;      // [members][F]
  double* band;      // [members][n_pad][CVA_BAND], zero before the first pass
  double* beta;      // [n_pad] per member, zero before the first pass
  long sBand = 0, sBeta = 0, sEps = 0;
};

// The adjoint store of F folds worked off in passes of FP: the band store [n_pad][384], B_f [FP][wp][wp] and beta_f [FP][wp] of one pass, eps_f [F]
struct CvAdjStore {
  double* base; long n_pad, FP, wp, F;
  __host__ __device__ static long size(long n_pad, long FP, long wp, long F) { return n_pad * SL_BAND + FP * (wp * wp + wp) + F; }
  __host__ __device__ double* band() const { return base; }
  __host__ __device__ double* Bf() const { return band() + n_pad * SL_BAND; }
  __host__ __device__ double* betaf() const { return Bf() + FP * wp * wp; }
  __host__ __device__ double* epsf() const { return betaf() + FP * wp; }
  // ... as cv_launch takes it; beta [n_pad] lives with the pass's other vectors (LooArdVecs::beta)
  __host__ __device__ CvAdjoint adjoint(int crit, double* beta) const { return CvAdjoint{crit, Bf(), betaf(), epsf(), band(), beta, 0, 0, 0}; }
};

// ... of the nb members of a lockstep group, each worked off in passes of FP folds (cv_launch: FP = CvWork::blocks / nb): the band stores
// [nb][n_pad][384], B_f [nb FP][wp][wp] and beta_f [nb FP][wp] of one pass at the (member, fold) pair index, eps_f [nb][F].  The layout
// depends on nb, as CvWork's: every group lays its own view over the arena, which the entry grows for the groups it will run (of G members
// and the tail).  One member is CvAdjStore, piece for piece.  The band stores are read in 16-byte pairs: their stride n_pad x 384 is even;
// eps_f is read one double at a time.  beta lives with the pass's other vectors, at LooArdGroupVecs' even stride.
struct CvAdjGroupStore {
  double* base; long nb, n_pad, FP, wp, F;
  __host__ __device__ static long size(long nb, long n_pad, long FP, long wp, long F) { return nb * (n_pad * SL_BAND + FP * (wp * wp + wp) + F); }
  __host__ __device__ long band_stride() const { return n_pad * SL_BAND; }
  __host__ __device__ long eps_stride() const { return F; }
  __host__ __device__ double* band() const { return base; }
  __host__ __device__ double* Bf() const { return band() + nb * band_stride(); }
  __host__ __device__ double* betaf() const { return Bf() + nb * FP * wp * wp; }
  __host__ __device__ double* epsf() const { return betaf() + nb * FP * wp; }
  // ... as cv_launch takes it; beta = member 0's (LooArdGroupVecs::member(0).beta()), the others sBeta = LooArdGroupVecs::mstride() apart
  __host__ __device__ CvAdjoint adjoint(int crit, double* beta, long sBeta) const {
    return CvAdjoint{crit, Bf(), betaf(), epsf(), band(), beta, band_stride(), sBeta, eps_stride()};
  }
};

// ---- bStage ----------------------------------------------------------------------------------------------------------------------------------
// The staging area of a slot's lockstep ARD groups, sized for the slot's capacity (so a later, larger group of the same call never
// reallocates it) and laid out as the resident data are, member b being its "data set b".  div and sn are uploaded in ONE copy: sn follows
// div without a gap.
struct ArdStage {
  double *X, *Xs, *y, *div, *sn;      // [cap][n_pad][dp], [cap][RIDE][dp], [cap][n_pad], divisors [cap][dp], sn~ [cap]
  long cap;
  __host__ __device__ static long size(long cap, long n_pad, long dp) { return cap * ((n_pad + SL_BLK) * dp + n_pad + dp + 1); }
  __host__ __device__ static ArdStage at(double* base, long cap, long n_pad, long dp) {
    Carve c;
    ArdStage a;
    a.cap = cap;
    a.X = base + c.take(cap * n_pad * dp);
    a.Xs = base + c.take(cap * SL_BLK * dp);
    a.y = base + c.take(cap * n_pad);
    a.div = base + c.take(cap * dp);
    a.sn = base + c.take(cap);
    return a;
  }
};

}  // namespace sigp
