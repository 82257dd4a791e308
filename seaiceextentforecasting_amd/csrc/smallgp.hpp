// The reference's OWN kernel at the reference's OWN size (n <= 128 training years, any number of features), batched:
// one workgroup per fit, everything in LDS.  Replaces, per (region, year, grid point),
//     north/June1st.py:264-277   (expm -> X Sigma~ X^T + sn~ I -> cholesky -> A~ -> sigma_f -> k*, k** -> v -> fmean, fvar)
//     north/June1st.py:246       (nlML)
// for the retro loop (north/retrospective_forecasts/September1st_retro.py:176-248) times the 20 x 20 hyper-parameter
// grid of north/June1st.py:210-211 -- ~5e4 fits of order <= 45 that are launch-latency bound one at a time.
//
// Covariance in factored form.  M is symmetric negative semi-definite, M = Q diag(lam) Q^T, so
//     Sigma~(l) = expm(l M) = Q diag(exp(l lam)) Q^T,        K~ = (X Q) diag(exp(l lam)) (X Q)^T + sn~ I :
// a data set is staged ONCE as A = [X ; Xs] Q (rows 0..n-1 training, rows n.. test points) with lam, and every grid point
// of that data set rebuilds K~ from A with its own weights (one eigendecomposition per data set).
// lam_mode 1: the weights are given directly (w_k = lam_k >= 0): A = [X ; Xs] U, lam = eigenvalues of a host-side
// Sigma~ = U diag(lam) U^T -- this is how a Pade expm(l M) from the host (the reference's own numbers at extreme l,
// SURVEY App. C-11) goes through the same kernel.
//
// Layout in LDS (smallgp_layout.hpp: SmallLayout): augmented lower-trapezoid  Kp[(n + 1 + m)][ldk]: rows 0..n-1 = K~ (lower), row n = y,
// rows n+1.. = k~*_j.  A right-looking column Cholesky of the bordered matrix leaves  z = L~^-1 y  in row n and  v_j = L~^-1 k~*_j  below it
// (the same ride-along trick as the blocked path), so sigma_f = z.z/n, fmean_j = v_j.z, fvar_j = sigma_f (k~** + sn~ - v_j.v_j).
//
// smallgp_kernel<NT, F>: every flavour F (SmallFlavour) runs the fit -- covariance build, bordered Cholesky, fit epilogue -- and writes
// out [nprob][small_out_width(F)]: sigma_f, nlML, info (LAPACK pivot index, 0 = ok), sigma_n;  mean / var [nprob][mstride].  Then its tail:
//
// Plain: nothing more.
//
// Grad (8 outputs): the same four, then the reference's MLII "gradient" (north/June1st.py:248-252) and the exact derivative of
// the profiled nlML w.r.t. (log l, log sn~).  In factored form every matrix of :248-252 is a reweighting of the same A:
//     dKdl = X (M Sigma) X^T + sigma_n I = sigma_f (D1 + sn~ I),  D1 = A diag(dw) A^T,  dw_k = lam_k exp(l lam_k)   (M Sigma~ = Q diag(lam w) Q^T)
//     dKds = X Sigma X^T + sigma_f I     = sigma_f (K~ - sn~ I + I),      K^-1 = K~^-1 / sigma_f,  alpha = a~ / sigma_f,
// so with T0 = tr(K~^-1), T1 = tr(K~^-1 D1), q0 = a~.a~, q1 = a~^T D1 a~ :
//     ref   g1 = (T1 + sn~ T0)/2 - (q1 + sn~ q0)/(2 sigma_f)        g2 = (1 - sn~)(T0 - q0/sigma_f)/2      (a~^T y = n sigma_f)
//     exact g1 = l (T1 - q1/sigma_f)/2                              g2 = sn~ (T0 - q0/sigma_f)/2
// T0, T1 come from the explicit inverse factor X = L~^-1 (formed in place over L~, row by row): T0 = |X|_F^2,
// T1 = sum_c dw_c |X a_c|^2 (a_c = column c of A; X a_c is never stored), a~ = X^T z, q1 = sum_c dw_c (a_c.a~)^2.
// lam_mode 1 sets (weights from a host-side Pade expm) take dw from the `dlam` pool (sigp_small_set_dweights); without it their
// gradient entries are NaN.
//
// Loo (6 outputs): leave-one-out cross-validation of the fit (Rasmussen & Williams 5.4.2) from the same
// in-LDS X = L~^-1 and a~:  g_i = [K~^-1]_ii = sum_{k >= i} X(k,i)^2,  loo_mean_i = y_i - a~_i / g_i,  loo_var_i = s_i / g_i with
// s_i = (zz - a~_i^2 / g_i) / (n - 1) (sigma_fixed = 0: sigma_f re-profiled without point i, what a refit on the other n - 1 points
// returns) or sigma_f (sigma_fixed = 1);  out[4] = nlpd = sum_i log(2 pi var_i)/2 + (y_i - mean_i)^2 / (2 var_i),  out[5] = sse;
// row_mean / row_var [nprob][pitch].  A non-SPD K~ gives +inf in both scores (the rows stay as the caller initialised them).
//
// Cv (6 outputs): leave-block-out cross-validation (blockcv.hpp: folds of `block` consecutive rows, `gap`
// rows removed on each side, windows of at most SM_CVW rows) from the same in-LDS X and a~, fold after fold in the Pw, Ww and tv of its
// layout:  P_SS(i, j) = sum_{k >= max} X(k, r0 + i) X(k, r0 + j),  P_SS = M M^T column by column,  W = M^-1 (one thread per
// column),  t = W a~_S,  r = W^T t,  h_i = sum_k W(k, i)^2;  mean = y - r,  var = s h with s = (zz - t.t) / (n - w) (sigma_fixed = 0) or sigma_f;
// outputs as Loo's, written for the scored rows of each fold.  A failed pivot of a P_SS: +inf in both scores and NaN rows.
//
// Hindcast (6 outputs): expanding-window hindcast validation (hindcast.hpp) from L~ and z as they lie in LDS
// after the factorisation -- no inverse is formed.  Row t is scored when s = t - lead + 1 >=
// min_train;  r_t = sum_{j=s..t} L~(t,j) z_j,  w_t = sum_{j=s..t} L~(t,j)^2,  mean_t = y_t - r_t,  var_t = sigma_t w_t with sigma_t =
// (sum_{j<s} z_j^2) / s (sigma_fixed = 0: sigma_f profiled on the training rows alone) or sigma_f (sigma_fixed = 1); one thread per row, every
// sum in ascending j.  Outputs as Loo's; rows that are not scored get NaN.  A non-SPD K~ gives +inf in both scores.
//
// NT = threads per workgroup: 256 (four wavefronts per fit) is the default at every order; NT = 64 (one wavefront per fit, every
// barrier of the column loop a wave-local no-op) is kept as a measurement switch ("small_nt64") -- on the reference-size grid it
// is SLOWER (1.71 vs 1.02 ms for 48 000 fits of n = 6 .. 45): the rank-1 updates have ~n^2/2 elements, enough for four waves,
// and one resident wave per fit leaves the LDS pipeline idle between dependent steps.
#pragma once
#include <hip/hip_runtime.h>

#include "blockcv.hpp"
#include "smallgp_layout.hpp"

namespace sigp {

struct SmallSet {
  long a_off;      // doubles into the A pool: A [(n + m)][N] row-major
  long y_off;      // doubles into the y pool: y [n]
  long lam_off;    // doubles into the lam pool: lam [N]
  int n, N, m;
  int lam_mode;    // 0: w_k = exp(ell * lam_k);  1: w_k = max(lam_k, 0)
};
struct SmallProb {
  int set;         // data set of this fit
  int pad;
  double ell;      // length scale (lam_mode 0)
  double sn;       // sigma_n tilde
};
// what the flavours take beyond the fit's own arguments
struct SmallExtras {
  double* row_mean;        // Loo, Cv, Hindcast: the prediction for every training row, [nprob][pitch]
  double* row_var;
  int pitch;
  int sigma_fixed;         // Loo, Cv, Hindcast: 0 = sigma_f re-profiled without the rows left out, 1 = the full fit's sigma_f
  int block, gap;          // Cv
  int lead, min_train;     // Hindcast
};

// one workgroup's fit: its sizes, its pieces in LDS and this thread's place in the 16-wide element mapping
struct SmallFit {
  int n, N, m, R;          // R = n + 1 + m rows of the bordered matrix
  int ldk, lda, ch;
  double *Kp, *Ac, *wk, *kss, *red, *at;
  const double* z;         // row n of Kp: y, then z = L~^-1 y
  int tid, tx, ty;
};

// sum over the NT threads of the workgroup; result valid on every thread
template <int NT>
__device__ inline double smallgp_allsum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) t += sh[w];
  return t;
}

// K~ (lower), k~*, k~** from the factored covariance, ch features at a time; then sn~ on the diagonal and y in row n
template <int NT>
__device__ __forceinline__ void smallgp_build(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const double* __restrict__ A,
                                              const double* __restrict__ lam, const double* __restrict__ y) {
  constexpr int TY = NT / 16;       // thread rows of the 16-wide element mapping
  const int n = w.n, N = w.N, m = w.m, ldk = w.ldk, lda = w.lda, ch = w.ch, tid = w.tid, tx = w.tx, ty = w.ty;
  double *Kp = w.Kp, *Ac = w.Ac, *wk = w.wk, *kss = w.kss;
  for (int e = tid; e < w.R * ldk; e += NT) Kp[e] = 0.0;
  if (tid < SM_MMAX) kss[tid] = 0.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    __syncthreads();
    if (tid < kc) {
      const double l = lam[k0 + tid];
      wk[tid] = sqrt(st.lam_mode ? fmax(l, 0.0) : exp(pb.ell * l));
    }
    __syncthreads();
    for (int e = tid; e < (n + m) * kc; e += NT) {
      const int r = e / kc, k = e - r * kc;
      Ac[r * lda + k] = A[(long)r * N + k0 + k] * wk[k];
    }
    __syncthreads();
    for (int i = ty; i < n + m; i += TY) {
      const int krow = i < n ? i : i + 1;               // test rows sit below the y row
      const double* ai = Ac + i * lda;
      const int jmax = i < n ? i : n - 1;
      for (int j = tx; j <= jmax; j += 16) {
        const double* aj = Ac + j * lda;
        double acc = 0.0;
        for (int k = 0; k < kc; ++k) acc = fma(ai[k], aj[k], acc);
        Kp[krow * ldk + j] += acc;
      }
    }
    if (tid < m) {
      const double* as = Ac + (n + tid) * lda;
      double acc = 0.0;
      for (int k = 0; k < kc; ++k) acc = fma(as[k], as[k], acc);
      kss[tid] += acc;
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) {
    Kp[i * ldk + i] += pb.sn;
    Kp[n * ldk + i] = y[i];
  }
  __syncthreads();
}

// Right-looking column Cholesky, one column per step, of the leading ncol columns of P [nrow][ld] (lower): rows ncol.. ride along and
// come out as L^-1 times themselves.  A non-positive or NaN pivot is replaced by 1 and the first one's 1-based index (LAPACK's info)
// recorded in *bad, which the caller has zeroed.
template <int NT>
__device__ __forceinline__ void smallgp_col_cholesky(double* P, int ld, int ncol, int nrow, int* bad, int tid, int tx, int ty) {
  constexpr int TY = NT / 16;
  for (int j = 0; j < ncol; ++j) {
    double d = P[j * ld + j];
    if (__builtin_expect(!(d > 0.0), 0)) {      // the same on every thread, and rare: a branch around the record, not a select on d
      if (tid == 0 && *bad == 0) *bad = j + 1;
      d = 1.0;
    }
    const double s = sqrt(d), inv = 1.0 / s;
    __syncthreads();                // everyone has read the pivot
    for (int i = j + tid; i < nrow; i += NT) P[i * ld + j] = (i == j) ? s : P[i * ld + j] * inv;
    __syncthreads();
    for (int i = j + 1 + ty; i < nrow; i += TY) {
      const double lij = P[i * ld + j];
      const int cmax = i < ncol ? i : ncol - 1;
      for (int c = j + 1 + tx; c <= cmax; c += 16) P[i * ld + c] = fma(-lij, P[c * ld + j], P[i * ld + c]);
    }
    __syncthreads();
  }
}

// sigma_f, nlML, the test points' means and variances (north/June1st.py:267-268, 246, 276-277); o = this fit's row of `out`, mean / var
// its rows.  Returns info; zz = z.z and sf = sigma_f on every thread.
template <int NT, SmallFlavour F>
__device__ __forceinline__ int smallgp_fit_epilogue(const SmallFit& w, const SmallProb& pb, const int* s_info, double* o, double* mean, double* var,
                                                    double& zz, double& sf) {
  const int n = w.n, ldk = w.ldk, tid = w.tid;
  const double* z = w.z;
  double zq = 0.0, ld_ = 0.0;
  for (int i = tid; i < n; i += NT) { zq = fma(z[i], z[i], zq); ld_ += log(w.Kp[i * ldk + i]); }
  zz = smallgp_allsum<NT>(zq, w.red);
  const double logdet = smallgp_allsum<NT>(ld_, w.red);
  const int info = *s_info;
  const double inf = __builtin_huge_val(), qnan = __builtin_nan("");
  sf = zz / (double)n;
  if (tid == 0) {
    if (info == 0) {
      o[0] = sf;
      o[1] = 0.5 * n + logdet + 0.5 * n * log(sf) + 0.5 * n * log(2.0 * M_PI);
      o[2] = 0.0;
      o[3] = sf * pb.sn;
    } else {
      o[0] = inf; o[1] = inf; o[2] = (double)info; o[3] = inf;
      for (int k = 4; k < small_out_width(F); ++k) o[k] = inf;          // north/June1st.py:254-256
    }
  }
  for (int j = 0; j < w.m; ++j) {
    const double* v = w.Kp + (n + 1 + j) * ldk;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < n; i += NT) { a = fma(v[i], z[i], a); b = fma(v[i], v[i], b); }
    const double vz = smallgp_allsum<NT>(a, w.red);
    const double vv = smallgp_allsum<NT>(b, w.red);
    if (tid == 0) {
      mean[j] = info == 0 ? vz : qnan;
      var[j] = info == 0 ? sf * (w.kss[j] + pb.sn - vv) : qnan;
    }
  }
  return info;
}

// X = L~^-1 in place, row by row: X(i,j) = -X(i,i) sum_{k=j}^{i-1} L(i,k) X(k,j); rows above i are complete, row i of L~ is
// read by everyone before anyone overwrites it.  Element j of the row belongs to a 16-lane group (k split over its lanes).
template <int NT>
__device__ __forceinline__ void smallgp_invert(const SmallFit& w) {
  constexpr int TY = NT / 16;
  const int n = w.n, ldk = w.ldk, tid = w.tid, tx = w.tx, ty = w.ty;
  double* Kp = w.Kp;
  for (int i = 0; i < n; ++i) {
    const double xii = 1.0 / Kp[i * ldk + i];
    constexpr int MC = (SM_NMAX + TY - 1) / TY;
    double mine[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      const int j = ty + c * TY;
      if (j < i) {
        double acc = 0.0;
        for (int k = j + tx; k < i; k += 16) acc = fma(Kp[i * ldk + k], Kp[k * ldk + j], acc);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
        mine[c] = -xii * acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      const int j = ty + c * TY;
      if (j < i && tx == 0) Kp[i * ldk + j] = mine[c];
    }
    if (tid == 0) Kp[i * ldk + i] = xii;
    __syncthreads();
  }
}

// a~ = X^T z into `at`, one thread per entry (odd pitch: the lanes' columns fall in different banks); no barrier behind it
template <int NT>
__device__ __forceinline__ void smallgp_atilde(const SmallFit& w) {
  for (int i = w.tid; i < w.n; i += NT) {
    double a = 0.0;
    for (int k = i; k < w.n; ++k) a = fma(w.Kp[k * w.ldk + i], w.z[k], a);
    w.at[i] = a;
  }
}

// the threads' shares (tn, ts) of a row flavour's scores, summed into o[4] = nlpd and o[5] = sse; with `bad`, +inf in both where *bad != 0.
// Returns whether it was.
template <int NT>
__device__ __forceinline__ bool smallgp_write_scores(const SmallFit& w, double tn, double ts, double* o, const int* bad = nullptr) {
  const double inf = __builtin_huge_val();
  const double nlpd = smallgp_allsum<NT>(tn, w.red);
  const double sse = smallgp_allsum<NT>(ts, w.red);
  const bool failed = bad && *bad != 0;
  if (w.tid == 0) { o[4] = failed ? inf : nlpd; o[5] = failed ? inf : sse; }
  return failed;
}

// ---- the tails: y, o, rmean, rvar = this fit's y, its row of `out` and its rows of the flavour's predictions -------------------------------
template <int NT>
__device__ __forceinline__ void smallgp_tail_hindcast(const SmallFit& w, const SmallExtras& x, const double* __restrict__ y, double sf, double* o,
                                                      double* __restrict__ rmean, double* __restrict__ rvar) {
  const double qnan = __builtin_nan("");
  const double* z = w.z;
  double tn = 0.0, ts = 0.0;
  for (int t = w.tid; t < w.n; t += NT) {
    const int s = t - x.lead + 1;
    double mu = qnan, v = qnan;
    if (s >= x.min_train) {
      const double* row = w.Kp + t * w.ldk;
      double r = 0.0, wt = 0.0;
      for (int j = s; j <= t; ++j) { r = fma(row[j], z[j], r); wt = fma(row[j], row[j], wt); }
      double sig = sf;
      if (!x.sigma_fixed) {
        double c = 0.0;
        for (int j = 0; j < s; ++j) c = fma(z[j], z[j], c);
        sig = c / (double)s;
      }
      v = sig * wt;
      mu = y[t] - r;
      tn += 0.5 * log(2.0 * M_PI * v) + r * r / (2.0 * v);
      ts = fma(r, r, ts);
    }
    rmean[t] = mu;
    rvar[t] = v;
  }
  smallgp_write_scores<NT>(w, tn, ts, o);
}

template <int NT>
__device__ __forceinline__ void smallgp_tail_loo(const SmallFit& w, const SmallExtras& x, const double* __restrict__ y, double zz, double sf, double* o,
                                                 double* __restrict__ rmean, double* __restrict__ rvar) {
  const int n = w.n;
  // column i of X: a~_i and g_i in one walk (odd pitch: the lanes' columns fall in different banks)
  double tn = 0.0, ts = 0.0;
  for (int i = w.tid; i < n; i += NT) {
    double a = 0.0, g = 0.0;
    for (int k = i; k < n; ++k) { const double xk = w.Kp[k * w.ldk + i]; a = fma(xk, w.z[k], a); g = fma(xk, xk, g); }
    const double r = a / g;                                    // y_i - loo_mean_i
    const double v = (x.sigma_fixed ? sf : (zz - a * r) / (double)(n - 1)) / g;
    rmean[i] = y[i] - r;
    rvar[i] = v;
    tn += 0.5 * log(2.0 * M_PI * v) + r * r / (2.0 * v);
    ts = fma(r, r, ts);
  }
  smallgp_write_scores<NT>(w, tn, ts, o);
}

// Pw, Ww, tv: the folds' scratch behind the plain layout (SmallLayout)
template <int NT>
__device__ __forceinline__ void smallgp_tail_cv(const SmallFit& w, const SmallExtras& x, double* Pw, double* Ww, double* tv, const double* __restrict__ y,
                                                double zz, double sf, double* o, double* __restrict__ rmean, double* __restrict__ rvar) {
  const int n = w.n, ldk = w.ldk, tid = w.tid;
  const double qnan = __builtin_nan("");
  const double* Kp = w.Kp;
  const double* at = w.at;
  __shared__ int s_cvbad;
  if (tid == 0) s_cvbad = 0;
  smallgp_atilde<NT>(w);
  __syncthreads();
  double tn = 0.0, ts = 0.0;
  const int F = (n + x.block - 1) / x.block;
  for (int f = 0; f < F; ++f) {
    int r0, r1, c0, c1;
    cv_window(n, x.block, x.gap, f, r0, r1, c0, c1);
    const int wd = r1 - r0;
    for (int e = tid; e < wd * wd; e += NT) {
      const int i = e / wd, j = e - i * wd;
      if (j <= i) {
        double p = 0.0;
        for (int k = r0 + i; k < n; ++k) p = fma(Kp[k * ldk + r0 + i], Kp[k * ldk + r0 + j], p);
        Pw[i * SM_CVP + j] = p;
      }
    }
    __syncthreads();
    smallgp_col_cholesky<NT>(Pw, SM_CVP, wd, wd, &s_cvbad, tid, w.tx, w.ty);
    if (tid < wd) {                     // column tid of W: M W = I by forward substitution
      for (int k = tid; k < wd; ++k) {
        double acc = k == tid ? 1.0 : 0.0;
        for (int j = tid; j < k; ++j) acc = fma(-Pw[k * SM_CVP + j], Ww[j * SM_CVP + tid], acc);
        Ww[k * SM_CVP + tid] = acc / Pw[k * SM_CVP + k];
      }
    }
    __syncthreads();
    if (tid < wd) {
      double t = 0.0;
      for (int i = 0; i <= tid; ++i) t = fma(Ww[tid * SM_CVP + i], at[r0 + i], t);
      tv[tid] = t;
    }
    __syncthreads();
    if (tid < wd) {
      double tt = 0.0, r = 0.0, hh = 0.0;
      for (int k = 0; k < wd; ++k) tt = fma(tv[k], tv[k], tt);
      for (int k = tid; k < wd; ++k) { const double xk = Ww[k * SM_CVP + tid]; r = fma(xk, tv[k], r); hh = fma(xk, xk, hh); }
      const int gi = r0 + tid;
      if (gi >= c0 && gi < c1) {
        const double v = (x.sigma_fixed ? sf : (zz - tt) / (double)(n - wd)) * hh;
        rmean[gi] = y[gi] - r;
        rvar[gi] = v;
        tn += 0.5 * log(2.0 * M_PI * v) + r * r / (2.0 * v);
        ts = fma(r, r, ts);
      }
    }
    __syncthreads();
  }
  if (smallgp_write_scores<NT>(w, tn, ts, o, &s_cvbad))
    for (int i = tid; i < n; i += NT) { rmean[i] = qnan; rvar[i] = qnan; }
}

template <int NT>
__device__ __forceinline__ void smallgp_tail_grad(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const double* __restrict__ A,
                                                  const double* __restrict__ lam, const double* __restrict__ dlam, double sf, double* o) {
  const int n = w.n, N = w.N, ldk = w.ldk, lda = w.lda, ch = w.ch, tid = w.tid;
  const double qnan = __builtin_nan("");
  double *Kp = w.Kp, *Ac = w.Ac, *wk = w.wk, *at = w.at;
  smallgp_atilde<NT>(w);
  double t0 = 0.0, t1 = 0.0, q0 = 0.0, q1 = 0.0;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (j <= i) { const double xe = Kp[i * ldk + j]; t0 = fma(xe, xe, t0); }
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) q0 = fma(at[i], at[i], q0);
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    __syncthreads();
    if (tid < kc) {
      const double l = lam[k0 + tid];
      wk[tid] = st.lam_mode ? (dlam ? dlam[k0 + tid] : qnan) : l * exp(pb.ell * l);
    }
    for (int e = tid; e < n * kc; e += NT) {
      const int r = e / kc, k = e - r * kc;
      Ac[r * lda + k] = A[(long)r * N + k0 + k];
    }
    __syncthreads();
    for (int e = tid; e < n * kc; e += NT) {
      const int i = e / kc, c = e - i * kc;
      const double* xi = Kp + i * ldk;
      double v = 0.0;
      for (int k = 0; k <= i; ++k) v = fma(xi[k], Ac[k * lda + c], v);
      t1 = fma(wk[c] * v, v, t1);
    }
    if (tid < kc) {
      double b = 0.0;
      for (int i = 0; i < n; ++i) b = fma(Ac[i * lda + tid], at[i], b);
      q1 = fma(wk[tid] * b, b, q1);
    }
  }
  const double T0 = smallgp_allsum<NT>(t0, w.red);
  const double T1 = smallgp_allsum<NT>(t1, w.red);
  const double Q0 = smallgp_allsum<NT>(q0, w.red);
  const double Q1 = smallgp_allsum<NT>(q1, w.red);
  if (tid == 0) {
    const double sn = pb.sn;
    o[4] = 0.5 * (T1 + sn * T0) - 0.5 * (Q1 + sn * Q0) / sf;
    o[5] = 0.5 * (1.0 - sn) * (T0 - Q0 / sf);
    o[6] = 0.5 * pb.ell * (T1 - Q1 / sf);
    o[7] = 0.5 * sn * (T0 - Q0 / sf);
  }
}

template <int NT, SmallFlavour F>
__global__ __launch_bounds__(NT) void smallgp_kernel(const SmallSet* __restrict__ sets, const SmallProb* __restrict__ probs,
                                                      const double* __restrict__ Apool, const double* __restrict__ ypool,
                                                      const double* __restrict__ lampool, int ch, double* __restrict__ out,
                                                      double* __restrict__ mean, double* __restrict__ var, int mstride,
                                                      const double* __restrict__ dlampool, SmallExtras x) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ int s_info;
  const SmallProb pb = probs[blockIdx.x];
  const SmallSet st = sets[pb.set];
  const SmallLayout lay{st.n, st.m, ch, F};
  double* lds = (double*)smem_raw;
  SmallFit w;
  w.n = st.n; w.N = st.N; w.m = st.m; w.R = lay.rows();
  w.ldk = lay.ldk(); w.lda = lay.lda(); w.ch = ch;
  w.Kp = lds + lay.Kp(); w.Ac = lds + lay.Ac(); w.wk = lds + lay.wk(); w.kss = lds + lay.kss(); w.red = lds + lay.red(); w.at = lds + lay.at();
  w.z = w.Kp + w.n * w.ldk;
  w.tid = threadIdx.x; w.tx = w.tid & 15; w.ty = w.tid >> 4;
  const double* A = Apool + st.a_off;
  const double* lam = lampool + st.lam_off;
  const double* y = ypool + st.y_off;
  double* o = out + (long)blockIdx.x * small_out_width(F);

  if (w.tid == 0) s_info = 0;
  smallgp_build<NT>(w, st, pb, A, lam, y);
  smallgp_col_cholesky<NT>(w.Kp, w.ldk, w.n, w.R, &s_info, w.tid, w.tx, w.ty);
  double zz, sf;
  const int info = smallgp_fit_epilogue<NT, F>(w, pb, &s_info, o, mean + (long)blockIdx.x * mstride, var + (long)blockIdx.x * mstride, zz, sf);
  if constexpr (F != SmallFlavour::Plain) {
    if (info != 0) return;           // uniform
    double* rmean = x.row_mean + (long)blockIdx.x * x.pitch;
    double* rvar = x.row_var + (long)blockIdx.x * x.pitch;
    if constexpr (F == SmallFlavour::Hindcast) {
      smallgp_tail_hindcast<NT>(w, x, y, sf, o, rmean, rvar);
    } else {
      smallgp_invert<NT>(w);
      if constexpr (F == SmallFlavour::Cv) smallgp_tail_cv<NT>(w, x, lds + lay.Pw(), lds + lay.Ww(), lds + lay.tv(), y, zz, sf, o, rmean, rvar);
      if constexpr (F == SmallFlavour::Loo) smallgp_tail_loo<NT>(w, x, y, zz, sf, o, rmean, rvar);
      if constexpr (F == SmallFlavour::Grad) smallgp_tail_grad<NT>(w, st, pb, A, lam, dlampool ? dlampool + st.lam_off : nullptr, sf, o);
    }
  }
}

}  // namespace sigp
