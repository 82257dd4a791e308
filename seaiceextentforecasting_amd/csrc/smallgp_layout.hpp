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
constexpr int SM_RED = 16;                     // doubles of reduction scratch (one per wavefront is used)
constexpr int SM_SLACK = 24;                   // unused doubles behind a~: part of every launch's size since the first
constexpr long SM_LDS_MAX = 160 * 1024 - 64;   // bytes of dynamic LDS one workgroup may ask for

// What one launch forms besides the fit itself (sigma_f, nlML, info, sigma_n, the test points' means and variances):
//   Plain     nothing
//   Grad      the MLII gradients
//   Loo       the leave-one-out predictions and scores
//   Cv        the leave-block-out predictions and scores
//   Hindcast  the expanding-window hindcast predictions and scores
enum class SmallFlavour { Plain, Grad, Loo, Cv, Hindcast };

// doubles per fit of `out`
__host__ __device__ constexpr int small_out_width(SmallFlavour f) { return f == SmallFlavour::Plain ? 4 : f == SmallFlavour::Grad ? 8 : 6; }
// does the flavour write a prediction per training row (mean / var [nprob][pitch]) and the scores out[4], out[5]?
__host__ __device__ constexpr bool small_has_rows(SmallFlavour f) { return f == SmallFlavour::Loo || f == SmallFlavour::Cv || f == SmallFlavour::Hindcast; }

// The LDS image of a fit of n training rows and m test points built ch features at a time; every offset in doubles from the start of the
// dynamic LDS.  A launch is sized for its largest n and m; each workgroup lays out its own fit.
//   Kp  [n + 1 + m][ldk]     the bordered matrix: K~ (lower), the y row, the k~* rows; ldk odd: column walks spread over the banks
//   Ac  [n + m][lda]         feature chunk, pre-scaled by sqrt(w_k)
//   wk  [ch]                 the chunk's weights
//   kss [SM_MMAX]            k~**_j
//   red [SM_RED]             reduction scratch
//   at  [n]                  a~ = L~^-T z, then SM_SLACK doubles
//   Cv alone, behind all of that:
//   Pw  [SM_CVW][SM_CVP]     a fold's P_SS, then its factor M (lower)
//   Ww  [SM_CVW][SM_CVP]     W = M^-1 (lower)
//   tv  [SM_CVW]             t = W a~_S
struct SmallLayout {
  int n, m, ch;
  SmallFlavour flavour;
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
  __host__ __device__ constexpr long bytes() const { return (flavour == SmallFlavour::Cv ? tv() + SM_CVW : Pw()) * (long)sizeof(double); }
};

// The feature chunk of a launch whose largest fit has nmax rows and mmax test points: the largest of start, start / 2, ... down to 8
// whose image fits (sigp_small_upload: start = 32, the Plain image; the Cv launch: start = the upload's chunk); 0 if none does.
__host__ __device__ constexpr int small_pick_chunk(int nmax, int mmax, SmallFlavour f, int start) {
  for (int ch = start; ch >= 8; ch /= 2)
    if (SmallLayout{nmax, mmax, ch, f}.bytes() <= SM_LDS_MAX) return ch;
  return 0;
}

}  // namespace sigp
