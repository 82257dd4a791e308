// The one-workgroup kernel (smallgp.hpp) in numbers: its limits, its flavours and where each piece of a fit lies in LDS.  The kernel takes
// its pointers from SmallLayout, the host (sigp_callers.inc) its launch sizes and feature chunks, so that what a launch asks for and what
// the kernel addresses cannot part ways.
// Plain C++ (no HIP include), so that a host compiler can check the arithmetic: tests/test_small_cases_host.py.
#pragma once

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace sigp {

constexpr int SM_NMAX = 128;                   // largest order one workgroup handles
constexpr int SM_MMAX = 8;                     // test points per fit
constexpr int SM_CVW = 32;                     // widest window (block + 2 gap) of the leave-block-out flavour
constexpr int SM_CVP = SM_CVW + 1;             // odd pitch of its w x w scratch matrices
constexpr int SM_GV = 4;                       // vectors of order n the score gradients keep (gv)
constexpr int SM_RED = 16;                     // doubles of reduction scratch (one per wavefront is used)
constexpr int SM_SLACK = 24;                   // unused doubles behind a~: part of every launch's size since the first
constexpr long SM_LDS_MAX = 160 * 1024 - 64;   // bytes of dynamic LDS one workgroup may ask for

// What one launch forms besides the fit itself (sigma_f, nlML, info, sigma_n, the test points' means and variances):
//   Plain     nothing
//   Grad      the MLII gradients
//   Loo       the leave-one-out predictions and scores
//   Cv        the leave-block-out predictions and scores
//   Hindcast  the expanding-window hindcast predictions and scores
//   LooGrad / HindcastGrad / CvGrad   what Loo / Hindcast / Cv form, then the derivatives of one of the two scores w.r.t. (log l, log sn~)
enum class SmallFlavour { Plain, Grad, Loo, Cv, Hindcast, LooGrad, HindcastGrad, CvGrad };

// Where K~ comes from: Factored, the reference's own X Sigma~ X^T as A diag(w) A^T (smallgp.hpp's header), or Stationary, the RBF / Matern-5/2
// kernel of the raw rows with one length scale or one per feature.  Stationary has Plain, Grad, Loo, Cv and Hindcast, in the factored flavours'
// own layout: SmallLayout does not ask which.
enum class SmallCov { Factored, Stationary };

// does the flavour differentiate a row score?
__host__ __device__ constexpr bool small_is_score_grad(SmallFlavour f) {
  return f == SmallFlavour::LooGrad || f == SmallFlavour::HindcastGrad || f == SmallFlavour::CvGrad;
}
// doubles per fit of `out`
__host__ __device__ constexpr int small_out_width(SmallFlavour f) { return f == SmallFlavour::Plain ? 4 : f == SmallFlavour::Grad || small_is_score_grad(f) ? 8 : 6; }
// ... of the covariance kind c: the stationary Grad flavour writes its N + 1 derivatives into an array of their own
__host__ __device__ constexpr int small_out_width(SmallFlavour f, SmallCov c) { return c == SmallCov::Stationary && f == SmallFlavour::Grad ? 4 : small_out_width(f); }
// does the flavour write a prediction per training row (mean / var [nprob][pitch]) and the scores out[4], out[5]?
__host__ __device__ constexpr bool small_has_rows(SmallFlavour f) {
  return f == SmallFlavour::Loo || f == SmallFlavour::Cv || f == SmallFlavour::Hindcast || small_is_score_grad(f);
}

// The LDS image of a fit of n training rows and m test points built ch features at a time; every offset in doubles from the start of the
// dynamic LDS.  A launch is sized for its largest n and m; each workgroup lays out its own fit.
//   Kp  [n + 1 + m][ldk]     the bordered matrix: K~ (lower), the y row, the k~* rows; ldk odd: column walks spread over the banks
//   Ac  [n + m][lda]         feature chunk, pre-scaled by sqrt(w_k)
//   wk  [ch]                 the chunk's weights
//   kss [SM_MMAX]            k~**_j
//   red [SM_RED]             reduction scratch
//   at  [n]                  a~ = L~^-T z, then SM_SLACK doubles
//   Cv and CvGrad, behind all of that:
//   Pw  [SM_CVW][SM_CVP]     a fold's P_SS, then its factor M (lower)
//   Ww  [SM_CVW][SM_CVP]     W = M^-1 (lower)
//   tv  [SM_CVW]             t = W a~_S
//   LooGrad and HindcastGrad alone, behind at and its slack:
//   Bc  [n][lda]             b_c = X a_c for the chunk's columns (X = L~^-1): what the Grad tail forms and does not keep
//   gv  [SM_GV][n]           the adjoint's vectors: Loo g, beta, gamma, u = X beta;  Hindcast rho, 2 kappa sigma, kappa w / s, zbar
//   hb  [n][lead]            HindcastGrad alone: the band L~(t, s_t .. t), saved before the inverse overwrites L~
//   CvGrad: Pw, Ww and tv at Cv's own offsets, and behind tv
//   Bc  [n][lda]             as above; once it is staged Ac is free and holds p_c = X^T b_c of the chunk's columns
//   gv  [SM_GV][n]           beta, then per fold r, rbar, kappa (a window has fewer than n rows); u = X beta after the folds
//   hb  [n][lead]            the lower band of the adjoint's B, bb(i, i - j), lead = block + 2 gap <= SM_CVW
// Limits of the two (every order the upload takes is laid out; what does not fit in SM_LDS_MAX at feature chunk 8 is refused):
//   every order n <= 96 with every m <= SM_MMAX fits, HindcastGrad at every lead <= SIGP_HINDCAST_SMALL_MAX_LEAD = 32 (chunk 32 throughout);
//   beyond that whatever bytes() <= SM_LDS_MAX admits: LooGrad n <= 128 up to m = 6 and n <= 127 at m = 7, 8;  HindcastGrad at lead = 1
//   n <= 128 up to m = 5 and n <= 127 at m = 6 .. 8, and at n = 128, m = 0 up to lead = 6.
// CvGrad: every order n <= 96 with every m <= SM_MMAX fits at every window <= SM_CVW (at n = 96, m = 8: chunk 32 up to window 10, chunk 16 beyond);
//   above that what fits at chunk 8: at m = 0 n <= 123 / 121 / 119 / 116 / 109 for windows 1 / 5 / 8 / 16 / 32, at m = 8 n <= 119 / 117 / 115 / 113 / 106.
struct SmallLayout {
  int n, m, ch;
  SmallFlavour flavour;
  int lead = 0;                                // the pitch of hb: HindcastGrad the lead, CvGrad the window block + 2 gap
  __host__ __device__ constexpr int rows() const { return n + 1 + m; }
  __host__ __device__ constexpr int ldk() const { return n | 1; }
  __host__ __device__ constexpr int lda() const { return ch + 1; }
  __host__ __device__ constexpr long Kp() const { return 0; }
  __host__ __device__ constexpr long Ac() const { return Kp() + (long)rows() * ldk(); }
  __host__ __device__ constexpr long wk() const { return Ac() + (long)(n + m) * lda(); }
  __host__ __device__ constexpr long kss() const { return wk() + ch; }
  __host__ __device__ constexpr long red() const { return kss() + SM_MMAX; }
  __host__ __device__ constexpr long at() const { return red() + SM_RED; }
  __host__ __device__ constexpr long Pw() const { return at() + n + SM_SLACK; }
  __host__ __device__ constexpr long Ww() const { return Pw() + SM_CVW * SM_CVP; }
  __host__ __device__ constexpr long tv() const { return Ww() + SM_CVW * SM_CVP; }
  __host__ __device__ constexpr long Bc() const { return flavour == SmallFlavour::CvGrad ? tv() + SM_CVW : Pw(); }
  __host__ __device__ constexpr long gv() const { return Bc() + (long)n * lda(); }
  __host__ __device__ constexpr long hb() const { return gv() + (long)SM_GV * n; }
  __host__ __device__ constexpr long end() const {
    return flavour == SmallFlavour::Cv ? tv() + SM_CVW : flavour == SmallFlavour::LooGrad ? hb() : flavour == SmallFlavour::HindcastGrad || flavour == SmallFlavour::CvGrad ? hb() + (long)n * lead : Pw();
  }
  __host__ __device__ constexpr long bytes() const { return end() * (long)sizeof(double); }
};

// The feature chunk of a launch whose largest fit has nmax rows and mmax test points: the largest of start, start / 2, ... down to 8
// whose image fits (sigp_small_upload: start = 32, the Plain image; the Cv and score-gradient launches: start = the upload's chunk); 0 if none does.
__host__ __device__ constexpr int small_pick_chunk(int nmax, int mmax, SmallFlavour f, int start, int lead = 0) {
  for (int ch = start; ch >= 8; ch /= 2)
    if (SmallLayout{nmax, mmax, ch, f, lead}.bytes() <= SM_LDS_MAX) return ch;
  return 0;
}

}  // namespace sigp
