"""A high-precision yardstick for fits on ill-conditioned covariance matrices, and the inputs of the conditioning tests
(tests/test_conditioning_host.py, tests/test_hip_conditioning.py).

Everything here is plain NumPy in ``np.longdouble`` (x87 extended: 64-bit mantissa, eps = 1.08e-19; NumPy has no BLAS for that type, so
no blocked kernel and no FMA contraction is involved): Cholesky by columns, forward and back substitution, and the oracle's formulae on
top of them.  Every function takes the fp64 matrix K~ (and the cross-covariance rows) AS THE DEVICE WAS GIVEN IT: the answer is "the exact
result for this matrix", not "for the ideal kernel" -- on a matrix of condition 1e13 the two differ by far more than any solver's error.
With eps_ld / eps_fp64 = 2^-11 the reference's own forward error is 2048 times below what an fp64 LAPACK fit of the same matrix
carries, which is the unit the tests measure in.

``lapack_fit`` is that fp64 LAPACK fit (np.linalg.cholesky + triangular solves, the oracle's non-idiom route) with the same outputs.
"""
import functools
import math

import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

LD = np.longdouble
U = 2.0 ** -53                                  # fp64 unit roundoff
AVAILABLE = bool(np.finfo(LD).eps < 1e-18)      # False where long double is fp64 (the tests skip)


class NotSPD(np.linalg.LinAlgError):
    def __init__(self, info, pivots):
        super().__init__("hp cholesky: pivot %d is not positive" % info)
        self.info, self.pivots = info, pivots


# ---- the solver ---------------------------------------------------------------------------------------------------------------------
def cholesky(K):
    """(L, squared pivots) of the fp64 matrix K, by columns in long double; NotSPD (info = 1-based index, the pivots so far) otherwise."""
    A = np.asarray(K, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    piv = np.zeros(n, dtype=LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j] = c[0]
        if not c[0] > 0:
            raise NotSPD(j + 1, piv[:j + 1].copy())
        L[j:, j] = c / np.sqrt(c[0])
    return L, piv


def forward(L, B):
    """L^-1 B by substitution (B [n] or [n, k])"""
    X = np.array(B, dtype=LD)
    for j in range(L.shape[0]):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    return X


def backward(L, B):
    """L^-T B by substitution"""
    X = np.array(B, dtype=LD)
    for j in range(L.shape[0] - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def inverse(L):
    """K^-1 = L^-T L^-1"""
    W = forward(L, np.eye(L.shape[0], dtype=LD))
    return backward(L, W)


# ---- metrics (long double arithmetic on fp64 results) ---------------------------------------------------------------------------------
def rho(L, K):
    """||L L^T - K||_F / ||K||_F"""
    L = np.tril(np.asarray(L, dtype=LD))
    K = np.asarray(K, dtype=LD)
    R = L @ L.T - K
    return float(np.sqrt(np.sum(R * R)) / np.sqrt(np.sum(K * K)))


def eta(K, x, b):
    """normwise backward error of x as a solution of K x = b: ||b - K x||_inf / (||K||_inf ||x||_inf + ||b||_inf)"""
    K, x, b = np.asarray(K, dtype=LD), np.asarray(x, dtype=LD).reshape(-1), np.asarray(b, dtype=LD).reshape(-1)
    r = b - K @ x
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(K), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))))


def refine_residual(K, x, b):
    """max|b - K x| / max|b|, the figure the fp32 engine reports"""
    K, x, b = np.asarray(K, dtype=LD), np.asarray(x, dtype=LD).reshape(-1), np.asarray(b, dtype=LD).reshape(-1)
    return float(np.max(np.abs(b - K @ x)) / np.max(np.abs(b)))


# ---- the oracle's formulae, once per arithmetic ---------------------------------------------------------------------------------------
def cv_folds(n, block, gap=0):
    c0 = np.arange(0, n, block)
    c1 = np.minimum(c0 + block, n)
    return np.stack([np.maximum(c0 - gap, 0), np.minimum(c1 + gap, n), c0, c1], axis=1)


def _scores(P, a, y, q, n, block, small_inverse):
    """leave-block-out closed form (tests/test_cv_host.py; block = 1: tests/test_loo_host.py), sigma_f re-profiled without the window"""
    mean, var = np.zeros(n, dtype=P.dtype), np.zeros(n, dtype=P.dtype)
    for r0, r1, c0, c1 in cv_folds(n, block):
        Ci = small_inverse(P[r0:r1, r0:r1])
        r = Ci @ a[r0:r1]
        s = (q - a[r0:r1] @ r) / (n - (r1 - r0))
        mean[c0:c1] = y[c0:c1] - r
        var[c0:c1] = s * np.diag(Ci)
    return mean, var


def _fit(K, y, sn, dK, ks, kss, block, chol, fwd, bwd, inv, small_inverse, dtype):
    K = np.asarray(K, dtype=dtype)
    y = np.asarray(y, dtype=dtype).reshape(-1)
    n = len(y)
    L = chol(K)
    alpha = bwd(L, fwd(L, y))
    q = y @ alpha
    sf = q / n
    two_pi = 2 * np.arccos(dtype(-1))
    out = dict(L=L, alpha=alpha, sigma_f=sf,
               nlml=dtype(n) / 2 + np.sum(np.log(np.diag(L))) + dtype(n) / 2 * np.log(sf) + dtype(n) / 2 * np.log(two_pi))
    if ks is not None:
        ks = np.asarray(ks, dtype=dtype)                      # [m, n] rows k~(x*, X), unit signal variance, no noise
        v = fwd(L, ks.T)
        out["v"] = v
        out["mean"] = ks @ alpha
        out["var"] = sf * (np.asarray(kss, dtype=dtype) + dtype(sn) - np.sum(v * v, axis=0))
    if dK is not None or block:
        P = inv(L)
        out["Kinv"] = P
    if block:
        out["loo_mean"], out["loo_var"] = _scores(P, alpha, y, q, n, 1, small_inverse)
        out["cv_mean"], out["cv_var"] = _scores(P, alpha, y, q, n, block, small_inverse)
    if dK is not None:
        dK = np.asarray(dK, dtype=dtype)
        g1 = np.sum(P * dK) / 2 - (alpha @ (dK @ alpha)) / (2 * sf)
        g2 = dtype(sn) * np.trace(P) / 2 - dtype(sn) * (alpha @ alpha) / (2 * sf)
        out["grad"] = np.array([g1, g2], dtype=dtype)
    return out


def hp_fit(K, y, sn, dK=None, ks=None, kss=None, block=5):
    """dict(L, alpha, sigma_f, nlml[, v, mean, var][, Kinv, loo_mean, loo_var, cv_mean, cv_var][, grad]) in long double: alpha~ = K~^-1 y,
    the profiled sigma_f = y^T alpha~ / n, nlML = n/2 + sum log diag L~ + n/2 log sigma_f + n/2 log 2 pi, predictions
    sigma_f (k** + sn~ - ||L~^-1 k*||^2), the leave-one-out and leave-block-out closed forms (sigma_f re-profiled without the window) and
    the exact gradient of the profiled nlML in (log l, log sn~), given dK = dK~/dlog l.  Raises NotSPD."""
    return _fit(K, y, sn, dK, ks, kss, block, lambda A: cholesky(A)[0], forward, backward, inverse,
                lambda B: inverse(cholesky(B)[0]), LD)


def lapack_fit(K, y, sn, dK=None, ks=None, kss=None, block=5):
    """the same in fp64 through LAPACK (potrf, trtrs), as the oracle's ``ref_idiom=False`` route does it"""
    def inv(L):
        return solve_triangular(L.T, solve_triangular(L, np.eye(L.shape[0]), lower=True), lower=False)
    return _fit(K, y, sn, dK, ks, kss, block, np.linalg.cholesky, lambda L, B: solve_triangular(L, B, lower=True),
                lambda L, B: solve_triangular(L.T, B, lower=False), inv, np.linalg.inv, np.float64)


def hp_refit_without(K, y, sn, r0, r1, c0, c1):
    """a REAL long-double refit without the rows [r0, r1), predicting the rows [c0, c1): (mean, var) -- what the closed form must equal"""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    keep = np.ones(len(y), dtype=bool)
    keep[r0:r1] = False
    ks = K[c0:c1][:, keep]
    kss = np.diag(K)[c0:c1] - sn
    r = hp_fit(K[np.ix_(keep, keep)], y[keep], sn, ks=ks, kss=kss, block=0)
    return r["mean"], r["var"]


def err(a, b):
    """max |a - b| with the difference taken in long double"""
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def hp_matmul(A, B, block=64):
    """A @ B in long double (A [m, k], B [k, n] of any real type, widened first), by row blocks of A: every entry is one plain
    dot product over k ascending in extended precision (NumPy has no BLAS for long double)."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    out = np.empty((A.shape[0], B.shape[1]), dtype=LD)
    for i in range(0, A.shape[0], block):
        out[i:i + block] = A[i:i + block] @ B
    return out


def cond2(K):
    w = np.linalg.eigvalsh(np.asarray(K, dtype=np.float64))
    return float(w[-1] / abs(w[0])) if w[0] != 0 else np.inf


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
def roundtrip(v):
    """exp(log v) by the C library: the value an ``nlml`` call at theta = log v hands to the covariance build, so that ``fit`` and ``nlml``
    factor the SAME fp64 matrix (a last-bit change of l moves a K~ of condition 1e13 by more than any solver's error)"""
    return math.exp(math.log(v)) if v > 0 else 0.0


ELL_A = roundtrip(3.0)
A_SIZES = (257, 384, 640)                      # three ragged 128-blocks, exactly three, five
A_LEVELS = (1e-4, 1e-8, 1e-11)                 # sn~: the control, then the harder levels
A_EDGE = 1e-13
A_DECADE = {1e-4: (1e6, 1e7), 1e-8: (1e10, 1e11), 1e-11: (1e13, 1e14)}      # cond(K~) ~ 0.6 n / sn~
B_SIZES = (257, 640)
B_LEVELS = (4, 8, 12, 14)                      # p: spectrum logspace(0, -p, n); the control, then the harder levels
B_EDGE = (1e-13, 1e-15, 3e-16, -1e-15)         # lambda_min of the edge members (spectrum logspace(0, -8) above it), n = 257


@functools.lru_cache(maxsize=None)
def family_a(n):
    """"ordered years": x = sort(U(0, 10)), d = 1, y = sin x + 0.1 N(0, 1); test points: 3 ride rows inside the data, and a general set of
    200 (training rows, points between them, points far outside the data)"""
    rng = np.random.default_rng(7100 + n)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    y = np.sin(x) + 0.1 * rng.standard_normal(n)
    ride = np.array([[0.5 * (x[0] + x[1])], [5.0], [x[n // 2]]])                       # between two rows, mid-range, a training row
    gen = np.concatenate([x[[0, n // 3, n - 1]], rng.uniform(0.0, 10.0, 190), [-40.0, 55.0, 1e3], x[[1, 2, 3, 4]]])[:, None]
    return x[:, None].copy(), y, ride, gen


def cross_a(kind, X, Xs):
    """(k~(x*, X) [m, n], k~(x*, x*) [m]) by the oracle's covariance function"""
    return O.cov_unit(kind, Xs, X, ELL_A), np.ones(Xs.shape[0])


def dk_a(kind, X):
    """dK~/dlog l by the oracle's formulae (oracle.gp_oracle.mlii, grad='exact')"""
    D2 = O.sqdist(X, X)
    if kind == "rbf":
        return O.cov_unit(kind, X, X, ELL_A) * D2 / (ELL_A * ELL_A)
    s = np.sqrt(5.0 * D2) / ELL_A
    return (s * s / 3.0) * (1.0 + s) * np.exp(-s)


def _spectral(n, lam, seed, dtype=np.float64):
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0].astype(dtype)
    K = (Q * np.asarray(lam, dtype=dtype)) @ Q.T
    return ((K + K.T) / 2).astype(np.float64)


@functools.lru_cache(maxsize=None)
def family_b(n, p=None, lam_min=None):
    """"prescribed spectrum": K = Q diag(logspace(0, -p, n)) Q^T, symmetrised (benign diagonal blocks: it separates an ill-conditioned
    matrix from an ill-conditioned block).  ``lam_min``: the edge members, p = 8 with the smallest eigenvalue replaced, formed in long
    double and rounded to fp64 (forming them in fp64 would move an eigenvalue of 1e-15 by its own size).  Also dK, a second symmetric
    matrix with the same eigenvectors (the "derivative" the gradient test hands over), y, and test points as rows of R^n: 3 ride rows and
    200 general ones, of which the first 5 are the short general set (unit vectors = training rows, a large vector among them)."""
    lam = np.logspace(0.0, -(8.0 if p is None else float(p)), n)
    if lam_min is not None:
        lam[-1] = lam_min
    K = _spectral(n, lam, 7200 + n, np.float64 if lam_min is None else LD)
    dK = _spectral(n, -lam * np.linspace(0.0, 1.0, n), 7200 + n)
    rng = np.random.default_rng(7300 + n)
    y = rng.standard_normal(n)
    E = np.eye(n)
    ride = np.stack([E[5], rng.standard_normal(n) / np.sqrt(n), 0.5 * (E[0] + E[n - 1])])
    gen = np.stack([E[0], E[n - 1], rng.standard_normal(n) / np.sqrt(n), 30.0 * rng.standard_normal(n), E[128]])
    gen = np.vstack([gen, rng.standard_normal((195, n)) / np.sqrt(n)])
    return K, dK, y, ride, gen


def cross_b(K, Xs):
    """X = I, Sigma = K: k~(x*, X) = x* K, k~(x*, x*) = x* K x*^T, in long double rounded to fp64"""
    ks = np.asarray(Xs, dtype=LD) @ np.asarray(K, dtype=LD)
    return ks.astype(np.float64), np.sum(ks * np.asarray(Xs, dtype=LD), axis=1).astype(np.float64)
