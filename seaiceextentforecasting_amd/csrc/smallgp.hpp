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
// LooGrad, HindcastGrad (8 outputs): Loo's / Hindcast's six -- the same statements in the same order, so the same bits --, then the
// derivative of the score x.crit (nlpd or sse) w.r.t. (log l, log sn~) with theta held and sigma_f re-profiled as x.sigma_fixed says.  The score
// is a function of K~ and y alone; with its symmetric adjoint G = dS/dK~ = X^T C X (X = L~^-1)
//     dS/dlog l = l <G, D1> = l sum_c dw_c b_c^T C b_c,  b_c = X a_c  (the chunk's b_c kept in Bc),     dS/dlog sn~ = sn~ tr G = sn~ sum_c x_c^T C x_c,
// x_c = column c of X (the upper triangle of Kp is zero from the build on).  G and C are never formed; b^T C b is
//   Loo (looard.hpp)        (u.b)(z.b) + sum_j gamma_j (X^T b)_j^2 + eps (z.b)^2,   u = X beta       [C = (u z^T + z u^T)/2 + X Gamma X^T + eps z z^T]
//   Hindcast (hindcast.hpp) sum_t sum_{i=s_t..t} L_ti b_i (sum_{j=s_t..i-1} B_tj b_j + B_ti b_i / 2) - sum_i zbar_i b_i (sum_{j<i} z_j b_j + z_i b_i / 2)
//                           with B_tj = rho_t z_j + 2 kappa_t sigma_t L_tj: the lower triangle of L^T B - zbar z^T, its diagonal halved.
// The band L~(t, s_t..t) is saved in hb before the inverse overwrites L~.  Every thread adds its terms in a fixed order and smallgp_allsum adds
// the threads: the same bits on every run.  lam_mode 1 sets without dweights: NaN in dS/dlog l alone.
//
// CvGrad (8 outputs): Cv's six -- the same statements in the same order --, then the derivative of the score x.crit with the adjoint of cvard.hpp:
// per fold H = P_SS^-1 = W^T W (over M in Pw), rbar, kappa on the scored rows, t = H rbar, sbar = sum kappa_i H_ii,
//     beta_f = -t [+ refit: 2 sbar r / (n - w)],   B_f = (t r^T + r t^T)/2 + s H diag(kappa) H [- refit: sbar r r^T / (n - w)],   eps_f = -sbar / (n - w) or -sbar / n,
// beta into gv[0], the lower band of B = sum_f E_f B_f E_f^T into hb [n][block + 2 gap], fold after fold, every entry added by one thread: overlapping
// windows add in ascending fold order.  C = (u z^T + z u^T)/2 + X B X^T + eps z z^T, u = X beta, so
//     b^T C b = (u.b)(z.b) + p^T B p + eps (z.b)^2,   p = X^T b  (a vector in Ac, free once Bc is staged, before the band is summed)
// over b_c = X a_c and over the columns of X, ch at a time.  A failed pivot of a P_SS: +inf in out[4..7] and NaN rows.
//
// Stationary covariances (SmallCov::Stationary; Plain, Grad, Loo, Cv, Hindcast): K~ = k(X, X) + sn~ I for the RBF / Matern-5/2 kernel with one length
// scale or one per feature (ARD).  A set's A holds the raw rows [X ; Xs], its lam is ignored.  smallgp_build_stationary stages u = x / l_k (the IEEE
// division, as ard_stage_kernel) ch features at a time and adds (u_ik - u_jk)^2 onto the running squared distance in ascending k -- exact zeros on the
// diagonal and for duplicate rows, and the same bits whatever the chunk --, then one pass maps sq -> k~ with cov_from_sq at unit length scale.  From
// there on the fit, the epilogue and the Loo / Cv / Hindcast tails are the factored flavours' own statements: they read K~, L~, X, z and y alone.
// Grad (4 outputs, and grad [nprob][ldg]): value + exact gradient of the profiled nlML in all N + 1 directions (ardgrad.hpp's formula),
//     d nlML / d log l_k = sum_{i>j} W_ij h_ij (u_ik - u_jk)^2,   W = K~^-1 - a~ a~^T / sigma_f,   d nlML / d log sn~ = sn~ (tr K~^-1 - a~.a~ / sigma_f) / 2 :
// sq is formed again into the strict UPPER triangle of Kp (zero from the build on: neither the column Cholesky nor the in-place inverse writes there),
// every entry is replaced by E_ij = (sum_{k >= i} X(k,i) X(k,j) - a~_i a~_j / sigma_f) h_ij, and one more pass over the re-staged chunks sums
// g_k = sum_{i>j} E_ij (u_ik - u_jk)^2, every thread over its own pairs in a fixed order, then smallgp_allsum.  One common scale: the sum of the g_k in
// ascending k.  The score gradients are not built for this covariance: their b_c = X a_c contraction rests on the factored form.
//
// NT = threads per workgroup: 256 (four wavefronts per fit) is the default at every order; NT = 64 (one wavefront per fit, every
// barrier of the column loop a wave-local no-op) is kept as a measurement switch ("small_nt64") -- on the reference-size grid it
// is SLOWER (1.71 vs 1.02 ms for 48 000 fits of n = 6 .. 45): the rank-1 updates have ~n^2/2 elements, enough for four waves,
// and one resident wave per fit leaves the LDS pipeline idle between dependent steps.
#pragma once
#include <hip/hip_runtime.h>

#include "ardgrad.hpp"
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
  int block, gap;          // Cv, CvGrad
  int lead, min_train;     // Hindcast
  int crit;                // LooGrad, HindcastGrad, CvGrad: the score that is differentiated, 0 = nlpd, 1 = sse (SIGP_LOO_NLPD / SIGP_LOO_SSE)
  // SmallCov::Stationary alone
  KParams kp;              // make_kparams(kernel id, 1.0, ...): the covariance function at unit length scale
  const double* scales;    // per-feature length scales [nprob][ldell]; nullptr: one scale per fit, SmallProb::ell
  int ldell;
  int ldg;                 // Grad: the pitch of grad
  double* grad;            // Grad: [nprob][ldg], d/d log l_0 .. l_{N-1} (one scale: d/d log l), then d/d log sn~
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

// the chunk's scales into wk and u = x / l_k of the first `rows` rows of A into Ac (the IEEE division, as ard_stage_kernel); a barrier ahead and one behind
template <int NT>
__device__ __forceinline__ void smallgp_stage_u(const SmallFit& w, const SmallProb& pb, const double* __restrict__ A, const double* __restrict__ ls, int k0, int kc,
                                                int rows) {
  __syncthreads();
  if (w.tid < kc) w.wk[w.tid] = ls ? ls[k0 + w.tid] : pb.ell;
  __syncthreads();
  for (int e = w.tid; e < rows * kc; e += NT) {
    const int r = e / kc, k = e - r * kc;
    w.Ac[r * w.lda + k] = A[(long)r * w.N + k0 + k] / w.wk[k];
  }
  __syncthreads();
}

// K~ (lower), k~*, k~** = 1 of a stationary covariance (kp: the kernel at unit length scale; ls: this fit's per-feature scales, nullptr: pb.ell for
// every feature): the squared distances of the scaled rows by direct differences, every entry one running sum in ascending k across the chunks, then
// cov_from_sq; sn~ on the diagonal and y in row n as smallgp_build
template <int NT>
__device__ __forceinline__ void smallgp_build_stationary(const SmallFit& w, const SmallProb& pb, const KParams& kp, const double* __restrict__ A,
                                                         const double* __restrict__ ls, const double* __restrict__ y) {
  constexpr int TY = NT / 16;
  const int n = w.n, N = w.N, m = w.m, ldk = w.ldk, lda = w.lda, ch = w.ch, tid = w.tid, tx = w.tx, ty = w.ty;
  double *Kp = w.Kp, *Ac = w.Ac;
  for (int e = tid; e < w.R * ldk; e += NT) Kp[e] = 0.0;
  if (tid < SM_MMAX) w.kss[tid] = 1.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_u<NT>(w, pb, A, ls, k0, kc, n + m);       // its first barrier publishes the zeros
    for (int i = ty; i < n + m; i += TY) {
      const int krow = i < n ? i : i + 1;               // test rows sit below the y row
      const double* ai = Ac + i * lda;
      const int jmax = i < n ? i : n - 1;
      for (int j = tx; j <= jmax; j += 16) {
        const double* aj = Ac + j * lda;
        double acc = Kp[krow * ldk + j];
        for (int k = 0; k < kc; ++k) { const double d = ai[k] - aj[k]; acc = fma(d, d, acc); }
        Kp[krow * ldk + j] = acc;
      }
    }
  }
  __syncthreads();
  for (int i = ty; i < n + m; i += TY) {
    const int krow = i < n ? i : i + 1;
    const int jmax = i < n ? i : n - 1;
    for (int j = tx; j <= jmax; j += 16) Kp[krow * ldk + j] = cov_from_sq(kp, Kp[krow * ldk + j]) + (i == j ? pb.sn : 0.0);
  }
  for (int i = tid; i < n; i += NT) Kp[n * ldk + i] = y[i];
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

// sigma_f, nlML, the test points' means and variances (north/June1st.py:267-268, 246, 276-277); o = this fit's row of `out` (OW doubles), mean / var
// its rows.  Returns info; zz = z.z and sf = sigma_f on every thread.
template <int NT, int OW>
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
      for (int k = 4; k < OW; ++k) o[k] = inf;          // north/June1st.py:254-256
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
// KEEP: r_t, w_t and sigma_t of every row (w_t = 0: not scored) into gv[0], gv[1], gv[2] for the gradient
template <int NT, bool KEEP = false>
__device__ __forceinline__ void smallgp_tail_hindcast(const SmallFit& w, const SmallExtras& x, const double* __restrict__ y, double sf, double* o,
                                                      double* __restrict__ rmean, double* __restrict__ rvar, double* gv = nullptr) {
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
      if constexpr (KEEP) { gv[t] = r; gv[w.n + t] = wt; gv[2 * w.n + t] = sig; }
    } else if constexpr (KEEP) {
      gv[t] = 0.0; gv[w.n + t] = 0.0; gv[2 * w.n + t] = 0.0;
    }
    rmean[t] = mu;
    rvar[t] = v;
  }
  smallgp_write_scores<NT>(w, tn, ts, o);
}

// KEEP: a~_i into at and g_i into gv[0] for the gradient
template <int NT, bool KEEP = false>
__device__ __forceinline__ void smallgp_tail_loo(const SmallFit& w, const SmallExtras& x, const double* __restrict__ y, double zz, double sf, double* o,
                                                 double* __restrict__ rmean, double* __restrict__ rvar, double* gv = nullptr) {
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
    if constexpr (KEEP) { w.at[i] = a; gv[i] = g; }
  }
  smallgp_write_scores<NT>(w, tn, ts, o);
}

// kappa = d nlpd / d var, rho = d nlpd / d r of a scored row with residual r and variance v; for the sse 0 and 2 r
__device__ __forceinline__ void small_kappa_rho(int crit, double r, double v, double& kappa, double& rho) {
  if (crit == 0) { kappa = 1.0 / (2.0 * v) - r * r / (2.0 * v * v); rho = r / v; }
  else { kappa = 0.0; rho = 2.0 * r; }
}

// Pw, Ww, tv: the folds' scratch behind the plain layout (SmallLayout)
// KEEP: the adjoint of cvard.hpp fold by fold for the gradient -- beta into gv[0], the lower band of B into bb [n][wb] (bb(i, i - j), wb = block + 2 gap),
// eps returned; gv[1], gv[2], gv[3] hold a fold's r, rbar and kappa, Pw its H = W^T W once M is dead, tv its t = H rbar once t0 = W a~_S is.  Folds
// run one after the other and within a fold every entry belongs to one thread: overlapping windows add in ascending fold order.  Returns
// whether a fold's P_SS failed its pivot test.
template <int NT, bool KEEP = false>
__device__ __forceinline__ bool smallgp_tail_cv(const SmallFit& w, const SmallExtras& x, double* Pw, double* Ww, double* tv, const double* __restrict__ y,
                                                double zz, double sf, double* o, double* __restrict__ rmean, double* __restrict__ rvar, double* gv = nullptr,
                                                double* bb = nullptr, double* eps_out = nullptr) {
  const int n = w.n, ldk = w.ldk, tid = w.tid;
  const double qnan = __builtin_nan("");
  const double* Kp = w.Kp;
  const double* at = w.at;
  __shared__ int s_cvbad;
  if (tid == 0) s_cvbad = 0;
  smallgp_atilde<NT>(w);
  const int wb = x.block + 2 * x.gap;
  double eps = 0.0;
  if constexpr (KEEP) {
    for (int i = tid; i < n; i += NT) gv[i] = 0.0;
    for (int e = tid; e < n * wb; e += NT) bb[e] = 0.0;
  }
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
        if constexpr (KEEP) small_kappa_rho(x.crit, r, v, gv[3 * n + tid], gv[2 * n + tid]);
      } else if constexpr (KEEP) {
        gv[2 * n + tid] = 0.0; gv[3 * n + tid] = 0.0;
      }
      if constexpr (KEEP) gv[n + tid] = r;
    }
    __syncthreads();
    if constexpr (KEEP) {
      const double *fr = gv + n, *frb = gv + 2 * n, *fk = gv + 3 * n;
      const int cl = c0 - r0, ch = c1 - r0;             // the scored rows within the window
      const double nw = (double)(n - wd);
      double tt = 0.0;                                  // as the scoring thread summed it
      for (int k = 0; k < wd; ++k) tt = fma(tv[k], tv[k], tt);
      const double s = x.sigma_fixed ? sf : (zz - tt) / nw;
      for (int e = tid; e < wd * wd; e += NT) {         // H = W^T W over M, both triangles
        const int i = e / wd, j = e - i * wd;
        if (j <= i) {
          double hij = 0.0;
          for (int k = i; k < wd; ++k) hij = fma(Ww[k * SM_CVP + i], Ww[k * SM_CVP + j], hij);
          Pw[i * SM_CVP + j] = hij;
          Pw[j * SM_CVP + i] = hij;
        }
      }
      __syncthreads();
      double sbar = 0.0;
      for (int k = cl; k < ch; ++k) sbar = fma(fk[k], Pw[k * SM_CVP + k], sbar);
      if (tid < wd) {
        double t = 0.0;
        for (int k = cl; k < ch; ++k) t = fma(Pw[tid * SM_CVP + k], frb[k], t);
        tv[tid] = t;
      }
      __syncthreads();
      const double sr = x.sigma_fixed ? 0.0 : sbar / nw;
      if (tid < wd) gv[r0 + tid] += fma(2.0 * sr, fr[tid], -tv[tid]);
      for (int e = tid; e < wd * wd; e += NT) {
        const int i = e / wd, j = e - i * wd;
        if (j <= i) {
          double hk = 0.0;
          for (int k = cl; k < ch; ++k) hk = fma(Pw[i * SM_CVP + k] * fk[k], Pw[k * SM_CVP + j], hk);
          bb[(r0 + i) * wb + i - j] += 0.5 * (tv[i] * fr[j] + fr[i] * tv[j]) + s * hk - sr * fr[i] * fr[j];
        }
      }
      eps -= x.sigma_fixed ? sbar / (double)n : sr;
      __syncthreads();
    }
  }
  const bool failed = smallgp_write_scores<NT>(w, tn, ts, o, &s_cvbad);
  if (failed)
    for (int i = tid; i < n; i += NT) { rmean[i] = qnan; rvar[i] = qnan; }
  if constexpr (KEEP) *eps_out = eps;
  return failed;
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

// after smallgp_invert: the exact gradient of the profiled nlML of a stationary covariance in all N + 1 directions into g (ls: per-feature scales,
// g[0 .. N-1] = d/d log l_k, g[N] = d/d log sn~; ls = nullptr: g[0] = d/d log l, g[1] = d/d log sn~).  The strict upper triangle of Kp holds sq, then E.
template <int NT>
__device__ __forceinline__ void smallgp_tail_grad_stationary(const SmallFit& w, const SmallProb& pb, const KParams& kp, const double* __restrict__ A,
                                                             const double* __restrict__ ls, double sf, double* __restrict__ g) {
  constexpr int TY = NT / 16;
  const int n = w.n, N = w.N, ldk = w.ldk, lda = w.lda, ch = w.ch, tid = w.tid, tx = w.tx, ty = w.ty;
  double *Kp = w.Kp, *Ac = w.Ac, *at = w.at;
  smallgp_atilde<NT>(w);
  double t0 = 0.0, q0 = 0.0;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (j <= i) { const double xe = Kp[i * ldk + j]; t0 = fma(xe, xe, t0); }
  }
  // sq again, as the build summed it, into Kp(j, i), j < i
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_u<NT>(w, pb, A, ls, k0, kc, n);           // its first barrier publishes a~
    for (int i = ty; i < n; i += TY) {
      const double* ai = Ac + i * lda;
      for (int j = tx; j < i; j += 16) {
        const double* aj = Ac + j * lda;
        double acc = Kp[j * ldk + i];
        for (int k = 0; k < kc; ++k) { const double d = ai[k] - aj[k]; acc = fma(d, d, acc); }
        Kp[j * ldk + i] = acc;
      }
    }
  }
  for (int i = tid; i < n; i += NT) q0 = fma(at[i], at[i], q0);
  __syncthreads();                                          // sq is complete: the next pass maps the entries to other threads
  // E_ij = ([K~^-1]_ij - a~_i a~_j / sigma_f) h_ij over its own sq: the entry's thread reads the lower triangle (X) and a~ alone
  const double isf = 1.0 / sf;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (j < i) {
      double p = 0.0;
      for (int k = i; k < n; ++k) p = fma(Kp[k * ldk + i], Kp[k * ldk + j], p);
      Kp[j * ldk + i] = fma(-at[i] * at[j], isf, p) * ard_h_from_sq(kp.kernel_id, Kp[j * ldk + i]);
    }
  }
  const double T0 = smallgp_allsum<NT>(t0, w.red);
  const double Q0 = smallgp_allsum<NT>(q0, w.red);
  double common = 0.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_u<NT>(w, pb, A, ls, k0, kc, n);           // its first barrier: E is complete, the last chunk's readers are done
    for (int c = 0; c < kc; ++c) {
      double acc = 0.0;
      for (int e = tid; e < n * n; e += NT) {
        const int i = e / n, j = e - i * n;
        if (j < i) { const double d = Ac[i * lda + c] - Ac[j * lda + c]; acc = fma(Kp[j * ldk + i] * d, d, acc); }
      }
      const double gk = smallgp_allsum<NT>(acc, w.red);
      if (ls) { if (tid == 0) g[k0 + c] = gk; }
      else common += gk;
    }
  }
  if (tid == 0) {
    if (!ls) g[0] = common;
    g[ls ? N : 1] = 0.5 * pb.sn * (T0 - Q0 * isf);
  }
}

// ---- the score gradients (LooGrad, HindcastGrad, CvGrad) ----------------------------------------------------------------------------------------

// dw of the chunk's features into wk and the chunk's raw columns into Ac (as the Grad tail stages them), then Bc(i, c) = sum_{k <= i} X(i, k) Ac(k, c);
// a barrier ahead of the staging and one behind Bc
template <int NT>
__device__ __forceinline__ void smallgp_stage_b(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const double* __restrict__ A, const double* __restrict__ lam,
                                                const double* __restrict__ dlam, int k0, int kc, double* Bc) {
  const int n = w.n, N = w.N, ldk = w.ldk, lda = w.lda, tid = w.tid;
  const double qnan = __builtin_nan("");
  __syncthreads();
  if (tid < kc) {
    const double l = lam[k0 + tid];
    w.wk[tid] = st.lam_mode ? (dlam ? dlam[k0 + tid] : qnan) : l * exp(pb.ell * l);
  }
  for (int e = tid; e < n * kc; e += NT) {
    const int r = e / kc, k = e - r * kc;
    w.Ac[r * lda + k] = A[(long)r * N + k0 + k];
  }
  __syncthreads();
  for (int e = tid; e < n * kc; e += NT) {
    const int i = e / kc, c = e - i * kc;
    const double* xi = w.Kp + i * ldk;
    double v = 0.0;
    for (int k = 0; k <= i; ++k) v = fma(xi[k], w.Ac[k * lda + c], v);
    Bc[i * lda + c] = v;
  }
  __syncthreads();
}

// this thread's share of sum_c wc_c b_c^T C b_c over the ncol columns of b [n][ldb] for the leave-one-out C (wc = nullptr: weights 1):
// gam, u, eps as in the header; `tri`: b is X itself, whose column c is zero above row c
template <int NT>
__device__ __forceinline__ double smallgp_quad_loo(const SmallFit& w, const double* b, int ldb, int ncol, const double* wc, bool tri, const double* gam, const double* u,
                                                   double eps) {
  const int n = w.n, ldk = w.ldk, tid = w.tid;
  const double* z = w.z;
  double acc = 0.0;
  for (int e = tid; e < n * ncol; e += NT) {              // gamma_j (X^T b_c)_j^2; with b = X the pair (j, c), j < c, stands for (c, j) as well
    const int j = e / ncol, c = e - j * ncol;
    if (tri && j > c) continue;
    double p = 0.0;
    for (int k = tri ? c : j; k < n; ++k) p = fma(w.Kp[k * ldk + j], b[k * ldb + c], p);
    const double g = tri && j < c ? gam[j] + gam[c] : gam[j];
    acc = fma((wc ? wc[c] : 1.0) * g * p, p, acc);
  }
  for (int c = tid; c < ncol; c += NT) {
    double ub = 0.0, zb = 0.0;
    for (int i = tri ? c : 0; i < n; ++i) { const double bi = b[i * ldb + c]; ub = fma(u[i], bi, ub); zb = fma(z[i], bi, zb); }
    acc = fma(wc ? wc[c] : 1.0, ub * zb + eps * zb * zb, acc);
  }
  return acc;
}

// the same for the hindcast C: rho, ks = 2 kappa sigma (both zero in rows that are not scored), zbar and the band hb [n][lead]
template <int NT>
__device__ __forceinline__ double smallgp_quad_hindcast(const SmallFit& w, const double* b, int ldb, int ncol, const double* wc, const double* rho, const double* ks,
                                                        const double* zbar, const double* hb, int lead, int min_train) {
  const int n = w.n, tid = w.tid;
  const double* z = w.z;
  double acc = 0.0;
  for (int e = tid; e < n * ncol; e += NT) {              // row t of B against column c
    const int t = e / ncol, c = e - t * ncol;
    const int s = t - lead + 1;
    if (s < min_train) continue;
    const double* lt = hb + t * lead - s;
    const double rt = rho[t], kt = ks[t];
    double pre = 0.0, q = 0.0;
    for (int j = s; j <= t; ++j) {
      const double bj = b[j * ldb + c], lj = lt[j];
      const double Bb = (rt * z[j] + kt * lj) * bj;
      q = fma(lj * bj, pre + 0.5 * Bb, q);
      pre += Bb;
    }
    acc = fma(wc ? wc[c] : 1.0, q, acc);
  }
  for (int c = tid; c < ncol; c += NT) {                  // the rank-one part: a scan of z_j b_j down the column
    double pre = 0.0, q = 0.0;
    for (int i = 0; i < n; ++i) {
      const double bi = b[i * ldb + c], zb = z[i] * bi;
      q = fma(zbar[i] * bi, pre + 0.5 * zb, q);
      pre += zb;
    }
    acc = fma(wc ? -wc[c] : -1.0, q, acc);
  }
  return acc;
}

// after smallgp_invert and smallgp_tail_loo<NT, true>: o[6], o[7]
template <int NT>
__device__ __forceinline__ void smallgp_tail_loo_grad(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const SmallExtras& x, const double* __restrict__ A,
                                                      const double* __restrict__ lam, const double* __restrict__ dlam, double* Bc, double* gv, double zz, double sf,
                                                      double* o) {
  const int n = w.n, N = w.N, ldk = w.ldk, ch = w.ch, tid = w.tid;
  double *gg = gv, *beta = gv + n, *gam = gv + 2 * n, *u = gv + 3 * n;
  const double n1 = (double)(n - 1);
  double ke = 0.0;
  for (int i = tid; i < n; i += NT) {                     // the thread that wrote at[i] and g_i
    const double a = w.at[i], g = gg[i], r = a / g;
    const double s = x.sigma_fixed ? sf : (zz - a * r) / n1;
    const double v = s / g;
    double kappa, rho;
    small_kappa_rho(x.crit, r, v, kappa, rho);
    double be = -rho / g, ga = kappa * s / (g * g) + rho * a / (g * g);
    if (!x.sigma_fixed) { be += 2.0 * kappa * a / (g * g * n1); ga -= kappa * a * a / (g * g * g * n1); }
    beta[i] = be; gam[i] = ga;
    ke += kappa / g;
  }
  const double eps = -smallgp_allsum<NT>(ke, w.red) / (x.sigma_fixed ? (double)n : n1);     // its barriers publish beta
  for (int i = tid; i < n; i += NT) {
    double a = 0.0;
    for (int k = 0; k <= i; ++k) a = fma(w.Kp[i * ldk + k], beta[k], a);
    u[i] = a;
  }
  double g1 = 0.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_b<NT>(w, st, pb, A, lam, dlam, k0, kc, Bc);
    g1 += smallgp_quad_loo<NT>(w, Bc, w.lda, kc, w.wk, false, gam, u, eps);
  }
  __syncthreads();                                        // u, where there was no chunk
  const double g0 = smallgp_quad_loo<NT>(w, w.Kp, ldk, n, nullptr, true, gam, u, eps);
  const double G1 = smallgp_allsum<NT>(g1, w.red);
  const double G0 = smallgp_allsum<NT>(g0, w.red);
  if (tid == 0) { o[6] = pb.ell * G1; o[7] = pb.sn * G0; }
}

// after smallgp_tail_hindcast<NT, true>, L~ still in place: saves the band, inverts, o[6], o[7]
template <int NT>
__device__ __forceinline__ void smallgp_tail_hindcast_grad(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const SmallExtras& x, const double* __restrict__ A,
                                                           const double* __restrict__ lam, const double* __restrict__ dlam, double* Bc, double* gv, double* hb,
                                                           double* o) {
  const int n = w.n, N = w.N, ldk = w.ldk, ch = w.ch, tid = w.tid, lead = x.lead;
  double *rho = gv, *ks = gv + n, *kw = gv + 2 * n, *zbar = gv + 3 * n;
  const double* z = w.z;
  for (int t = tid; t < n; t += NT) {                     // the thread that wrote r_t, w_t, sigma_t there
    const int s = t - lead + 1;
    const double r = rho[t], wt = ks[t], sig = kw[t];
    double rh = 0.0, k2 = 0.0, kq = 0.0;
    if (s >= x.min_train) {
      double kappa;
      small_kappa_rho(x.crit, r, sig * wt, kappa, rh);
      k2 = 2.0 * kappa * sig;
      kq = kappa * wt / (double)(x.sigma_fixed ? n : s);
      for (int j = s; j <= t; ++j) hb[t * lead + j - s] = w.Kp[t * ldk + j];
    }
    rho[t] = rh; ks[t] = k2; kw[t] = kq;
  }
  __syncthreads();
  for (int j = tid; j < n; j += NT) {
    // zbar_j = sum_{t scored, s_t <= j <= t} rho_t L_tj + 2 z_j sum_{t scored, s_t > j} kappa_t w_t / s_t   (fixed: every scored t, / n)
    double a = 0.0, c = 0.0;
    const int t1 = min(n - 1, j + lead - 1);
    for (int t = j; t <= t1; ++t)
      if (t - lead + 1 >= x.min_train) a = fma(rho[t], hb[t * lead + j - (t - lead + 1)], a);
    for (int t = x.sigma_fixed ? 0 : t1 + 1; t < n; ++t) c += kw[t];
    zbar[j] = fma(2.0 * z[j], c, a);
  }
  smallgp_invert<NT>(w);                                  // its first barrier comes before its first write: the band is out
  double g1 = 0.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_b<NT>(w, st, pb, A, lam, dlam, k0, kc, Bc);
    g1 += smallgp_quad_hindcast<NT>(w, Bc, w.lda, kc, w.wk, rho, ks, zbar, hb, lead, x.min_train);
  }
  const double g0 = smallgp_quad_hindcast<NT>(w, w.Kp, ldk, n, nullptr, rho, ks, zbar, hb, lead, x.min_train);
  const double G1 = smallgp_allsum<NT>(g1, w.red);
  const double G0 = smallgp_allsum<NT>(g0, w.red);
  if (tid == 0) { o[6] = pb.ell * G1; o[7] = pb.sn * G0; }
}

// this thread's share of sum_c wc_c b_c^T C b_c over the ncol <= ch columns of b [n][ldb] for the leave-block-out C (wc = nullptr: weights 1):
// (u.b)(z.b) + p^T B p + eps (z.b)^2 with p = X^T b, which goes through Ac one column per thread element first (B is a band: p has to exist as a
// vector).  first: column c of b is zero above row first + c (b = columns first .. of X itself; 0 and b dense otherwise).  A barrier ahead of p
// (the last slab's readers) and one behind it.
template <int NT>
__device__ __forceinline__ double smallgp_quad_cv(const SmallFit& w, const double* b, int ldb, int ncol, const double* wc, int first, bool tri, const double* bb, int wb,
                                                  const double* u, double eps) {
  const int n = w.n, ldk = w.ldk, lda = w.lda, tid = w.tid;
  const double* z = w.z;
  double* p = w.Ac;
  __syncthreads();
  for (int e = tid; e < n * ncol; e += NT) {
    const int j = e / ncol, c = e - j * ncol;
    const int k0 = tri ? max(j, first + c) : j;
    double a = 0.0;
    for (int k = k0; k < n; ++k) a = fma(w.Kp[k * ldk + j], b[k * ldb + c], a);
    p[j * lda + c] = a;
  }
  __syncthreads();
  double acc = 0.0;
  for (int e = tid; e < n * ncol; e += NT) {              // row i of B against p_c: the diagonal once, the band below it for both triangles
    const int i = e / ncol, c = e - i * ncol;
    const double* bi = bb + i * wb;
    const int dmax = min(i, wb - 1);
    double q = 0.0;
    for (int d = 1; d <= dmax; ++d) q = fma(bi[d], p[(i - d) * lda + c], q);
    const double pi = p[i * lda + c];
    acc = fma((wc ? wc[c] : 1.0) * pi, fma(bi[0], pi, 2.0 * q), acc);
  }
  for (int c = tid; c < ncol; c += NT) {
    double ub = 0.0, zb = 0.0;
    for (int i = tri ? first + c : 0; i < n; ++i) { const double bi = b[i * ldb + c]; ub = fma(u[i], bi, ub); zb = fma(z[i], bi, zb); }
    acc = fma(wc ? wc[c] : 1.0, ub * zb + eps * zb * zb, acc);
  }
  return acc;
}

// after smallgp_invert and smallgp_tail_cv<NT, true> (beta in gv[0], the band in bb, eps): o[6], o[7]
template <int NT>
__device__ __forceinline__ void smallgp_tail_cv_grad(const SmallFit& w, const SmallSet& st, const SmallProb& pb, const SmallExtras& x, const double* __restrict__ A,
                                                     const double* __restrict__ lam, const double* __restrict__ dlam, double* Bc, double* gv, const double* bb, double eps,
                                                     double* o) {
  const int n = w.n, N = w.N, ldk = w.ldk, ch = w.ch, tid = w.tid, wb = x.block + 2 * x.gap;
  const double* beta = gv;
  double* u = gv + n;
  for (int i = tid; i < n; i += NT) {                     // the fold loop ended on a barrier: beta is complete, a fold's r is dead
    double a = 0.0;
    for (int k = 0; k <= i; ++k) a = fma(w.Kp[i * ldk + k], beta[k], a);
    u[i] = a;
  }
  double g1 = 0.0;
  for (int k0 = 0; k0 < N; k0 += ch) {
    const int kc = min(ch, N - k0);
    smallgp_stage_b<NT>(w, st, pb, A, lam, dlam, k0, kc, Bc);
    g1 += smallgp_quad_cv<NT>(w, Bc, w.lda, kc, w.wk, 0, false, bb, wb, u, eps);
  }
  double g0 = 0.0;
  for (int c0 = 0; c0 < n; c0 += ch) g0 += smallgp_quad_cv<NT>(w, w.Kp + c0, ldk, min(ch, n - c0), nullptr, c0, true, bb, wb, u, eps);
  const double G1 = smallgp_allsum<NT>(g1, w.red);
  const double G0 = smallgp_allsum<NT>(g0, w.red);
  if (tid == 0) { o[6] = pb.ell * G1; o[7] = pb.sn * G0; }
}

template <int NT, SmallFlavour F, SmallCov C = SmallCov::Factored>
__global__ __launch_bounds__(NT) void smallgp_kernel(const SmallSet* __restrict__ sets, const SmallProb* __restrict__ probs,
                                                      const double* __restrict__ Apool, const double* __restrict__ ypool,
                                                      const double* __restrict__ lampool, int ch, double* __restrict__ out,
                                                      double* __restrict__ mean, double* __restrict__ var, int mstride,
                                                      const double* __restrict__ dlampool, SmallExtras x) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ int s_info;
  const SmallProb pb = probs[blockIdx.x];
  const SmallSet st = sets[pb.set];
  const SmallLayout lay{st.n, st.m, ch, F, F == SmallFlavour::HindcastGrad ? x.lead : F == SmallFlavour::CvGrad ? x.block + 2 * x.gap : 0};
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
  constexpr int OW = small_out_width(F, C);
  double* o = out + (long)blockIdx.x * OW;
  const double* ls = nullptr;        // Stationary: this fit's per-feature scales
  if constexpr (C == SmallCov::Stationary) ls = x.scales ? x.scales + (long)blockIdx.x * x.ldell : nullptr;

  if (w.tid == 0) s_info = 0;
  if constexpr (C == SmallCov::Stationary) smallgp_build_stationary<NT>(w, pb, x.kp, A, ls, y);
  else smallgp_build<NT>(w, st, pb, A, lam, y);
  smallgp_col_cholesky<NT>(w.Kp, w.ldk, w.n, w.R, &s_info, w.tid, w.tx, w.ty);
  double zz, sf;
  const int info = smallgp_fit_epilogue<NT, OW>(w, pb, &s_info, o, mean + (long)blockIdx.x * mstride, var + (long)blockIdx.x * mstride, zz, sf);
  if constexpr (C == SmallCov::Stationary && F == SmallFlavour::Grad) {
    static_assert(NT == 256, "the stationary flavours are built at four wavefronts per fit");
    double* g = x.grad + (long)blockIdx.x * x.ldg;
    if (info != 0) {                 // uniform
      for (int k = w.tid; k <= (ls ? w.N : 1); k += NT) g[k] = __builtin_huge_val();
      return;
    }
    smallgp_invert<NT>(w);
    smallgp_tail_grad_stationary<NT>(w, pb, x.kp, A, ls, sf, g);
  } else if constexpr (F != SmallFlavour::Plain) {
    static_assert(C == SmallCov::Factored || !small_is_score_grad(F), "the score gradients rest on the factored form");
    if (info != 0) return;           // uniform
    double* rmean = x.row_mean + (long)blockIdx.x * x.pitch;
    double* rvar = x.row_var + (long)blockIdx.x * x.pitch;
    const double* dlam = dlampool ? dlampool + st.lam_off : nullptr;
    if constexpr (F == SmallFlavour::Hindcast) {
      smallgp_tail_hindcast<NT>(w, x, y, sf, o, rmean, rvar);
    } else if constexpr (F == SmallFlavour::HindcastGrad) {
      smallgp_tail_hindcast<NT, true>(w, x, y, sf, o, rmean, rvar, lds + lay.gv());
      smallgp_tail_hindcast_grad<NT>(w, st, pb, x, A, lam, dlam, lds + lay.Bc(), lds + lay.gv(), lds + lay.hb(), o);
    } else if constexpr (F == SmallFlavour::LooGrad) {
      smallgp_invert<NT>(w);
      smallgp_tail_loo<NT, true>(w, x, y, zz, sf, o, rmean, rvar, lds + lay.gv());
      smallgp_tail_loo_grad<NT>(w, st, pb, x, A, lam, dlam, lds + lay.Bc(), lds + lay.gv(), zz, sf, o);
    } else if constexpr (F == SmallFlavour::CvGrad) {
      smallgp_invert<NT>(w);
      double eps;
      if (smallgp_tail_cv<NT, true>(w, x, lds + lay.Pw(), lds + lay.Ww(), lds + lay.tv(), y, zz, sf, o, rmean, rvar, lds + lay.gv(), lds + lay.hb(), &eps)) {
        if (w.tid == 0) { o[6] = __builtin_huge_val(); o[7] = __builtin_huge_val(); }
        return;                        // uniform
      }
      smallgp_tail_cv_grad<NT>(w, st, pb, x, A, lam, dlam, lds + lay.Bc(), lds + lay.gv(), lds + lay.hb(), eps, o);
    } else {
      smallgp_invert<NT>(w);
      if constexpr (F == SmallFlavour::Cv) smallgp_tail_cv<NT>(w, x, lds + lay.Pw(), lds + lay.Ww(), lds + lay.tv(), y, zz, sf, o, rmean, rvar);
      if constexpr (F == SmallFlavour::Loo) smallgp_tail_loo<NT>(w, x, y, zz, sf, o, rmean, rvar);
      if constexpr (F == SmallFlavour::Grad) smallgp_tail_grad<NT>(w, st, pb, A, lam, dlam, sf, o);
    }
  }
}

}  // namespace sigp
