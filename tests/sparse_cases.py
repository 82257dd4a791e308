"""Cases and yardsticks of the inducing-point (sparse) fit (include/sigp.h: sigp_sparse_fit / sigp_sparse_predict), shared by
tests/test_sparse_host.py (CPU tier) and tests/test_hip_sparse.py (GPU).  No tests here.

Two evaluations of the same closed form (the header's formulae, whitened form):
  ``closed_form``     fp64: SciPy ``cholesky`` / ``solve_triangular`` on ``oracle.cov_unit``
  ``closed_form_hp``  long double, through tests/hp_reference.py (``cholesky`` / ``forward`` / ``hp_matmul``) on the SAME fp64 covariance
                      matrices: "the exact result for these matrices"
Data: ``oracle.synthetic_problem`` with fixed seeds, l = sqrt(d); Z a seeded random subset of the rows of X (where m > n: all of X and
seeded N(0,1) rows beside it)."""
import functools
from collections import namedtuple

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import hp_reference as H
from oracle import gp_oracle as O

LD = H.LD
U = H.U
AVAILABLE = H.AVAILABLE

Case = namedtuple("Case", "kind n m d sn eps chunk seed")

# (n, m, d, sparse_chunk): m inside one 128 tile | m across a tile edge, three chunks, the last ragged (188 columns) | many chunks, three tile
# rows | features past one 64-column pad | n < m | m = 1
SHAPES = ((300, 100, 3, 128), (700, 130, 3, 256), (700, 300, 8, 128), (515, 129, 66, 256), (50, 64, 3, 128), (40, 1, 2, 128))
PAIRS = ((1e-2, 1e-8), (1e-2, 1e-6), (1e-4, 1e-8))       # (sn~, jitter)
MS_TEST = 9                                               # test points of a case
COND_CAP = 1e8                                            # cond(K_mm + eps I) of every case
SHARP_COND = 1e6                                          # ... and of the cases the sharper bound applies to
GATE = 1e-8                                               # the suite's prediction tolerance
FP64_GATE = 1e-11                                         # the fp64 closed form against long double on these inputs


def _table():
    out = []
    for kind in ("rbf", "matern52"):
        for si, (n, m, d, chunk) in enumerate(SHAPES):
            seed = 20270000 + si                          # one data set per shape, shared by the kernels and the (sn~, jitter) pairs
            for (sn, eps) in PAIRS:
                if kind == "rbf" and d == 3 and (sn, eps) != (1e-2, 1e-6):
                    continue                              # RBF at d = 3 stays under the condition cap with the larger jitter only
                out.append(Case(kind, n, m, d, sn, eps, chunk, seed))
    return tuple(out)


TABLE = _table()


def case_id(c):
    return "%s-n%d-m%d-d%d-sn%g-eps%g" % (c.kind, c.n, c.m, c.d, c.sn, c.eps)


def is_sharp(c):
    """the cases of condition <= 1e6: every Matern-5/2 case, RBF at d = 8 and d = 66 (and the one-point case)"""
    return c.kind == "matern52" or c.d >= 8 or c.m == 1


def inducing_subset(X, m, seed):
    """m rows: a seeded random subset of X, in X's order; for m > n all of X and seeded N(0,1) rows beside it"""
    rng = np.random.default_rng(seed)
    n, d = X.shape
    if m <= n:
        return X[np.sort(rng.choice(n, size=m, replace=False))].copy()
    return np.vstack([X, rng.standard_normal((m - n, d))])


@functools.lru_cache(maxsize=None)
def data(c):
    """(X, y, Xs, Z, ell) of a case; read-only"""
    X, y, Xs = O.synthetic_problem(c.n, c.d, c.seed, m=MS_TEST)
    Z = inducing_subset(X, c.m, c.seed + 500000)
    for a in (X, y, Xs, Z):
        a.setflags(write=False)
    return X, y, Xs, Z, float(np.sqrt(c.d))


def _scaled(X, Z, Xs, ell):
    """per-feature scales: the inputs divided by them and unit length scale (the library's idiom); a scalar stays"""
    if np.ndim(ell) == 0:
        return X, Z, Xs, float(ell)
    ell = np.asarray(ell, dtype=np.float64)
    return X / ell, Z / ell, (None if Xs is None else Xs / ell), 1.0


def covariances(kind, X, Z, Xs, ell, eps):
    """the fp64 matrices both closed forms start from: K_mm + eps I, K_mn, K_m*"""
    X, Z, Xs, ell = _scaled(np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64), None if Xs is None else np.atleast_2d(Xs), ell)
    Kmm = O.cov_unit(kind, Z, Z, ell) + eps * np.eye(Z.shape[0])
    Kmn = O.cov_unit(kind, Z, X, ell)
    Kms = None if Xs is None else O.cov_unit(kind, Z, Xs, ell)
    return Kmm, Kmn, Kms


def _finish(n, m, sn, yy, ww, t, logdiag, log, pi):
    sf = (yy - ww) / (sn * n)
    nlml = 0.5 * n + (0.5 * (n - m) * log(sn) + logdiag) + 0.5 * n * log(sf) + 0.5 * n * log(2 * pi)
    return sf, nlml, nlml + (n - t) / (2 * sn)


def closed_form(kind, X, y, Z, Xs, ell, sn, eps, mats=None):
    """fp64: dict(sigma_f, nlml, bound, mean, var, cond)"""
    Kmm, Kmn, Kms = mats or covariances(kind, X, Z, Xs, ell, eps)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, m = len(y), Kmm.shape[0]
    Lm = cholesky(Kmm, lower=True)
    V = solve_triangular(Lm, Kmn, lower=True)
    LB = cholesky(sn * np.eye(m) + V @ V.T, lower=True)
    w = solve_triangular(LB, V @ y, lower=True)
    sf, nlml, bound = _finish(n, m, sn, float(y @ y), float(w @ w), float(np.sum(V * V)), float(np.sum(np.log(np.diag(LB)))), np.log, np.pi)
    out = dict(sigma_f=sf, nlml=nlml, bound=bound, cond=H.cond2(Kmm))
    if Kms is not None:
        p = solve_triangular(Lm, Kms, lower=True)
        q = solve_triangular(LB, p, lower=True)
        out.update(mean=q.T @ w, var=sf * (1.0 + sn - np.sum(p * p, axis=0) + sn * np.sum(q * q, axis=0)))
    return out


def closed_form_hp(kind, X, y, Z, Xs, ell, sn, eps, mats=None):
    """long double on the same fp64 covariance matrices: dict(sigma_f, nlml, bound, mean, var) of long doubles"""
    Kmm, Kmn, Kms = mats or covariances(kind, X, Z, Xs, ell, eps)
    y = np.asarray(y, dtype=LD).reshape(-1)
    n, m = len(y), Kmm.shape[0]
    sn = LD(sn)
    Lm = H.cholesky(Kmm)[0]
    V = H.forward(Lm, Kmn)
    Bm = H.hp_matmul(V, V.T)
    Bm[np.diag_indices(m)] += sn
    LB = H.cholesky(Bm)[0]
    w = H.forward(LB, H.hp_matmul(V, y[:, None])[:, 0])
    sf, nlml, bound = _finish(LD(n), LD(m), sn, y @ y, w @ w, np.sum(V * V), np.sum(np.log(np.diag(LB))), np.log, np.arctan(LD(1)) * 4)
    out = dict(sigma_f=sf, nlml=nlml, bound=bound)
    if Kms is not None:
        p = H.forward(Lm, Kms)
        q = H.forward(LB, p)
        out.update(mean=q.T @ w, var=sf * (LD(1) + sn - np.sum(p * p, axis=0) + sn * np.sum(q * q, axis=0)))
    return out


def error(got, ref, ymax):
    """the largest of: sigma_f, nlml, bound relative; mean relative to max |y|; var relative to sigma_f -- differences taken in long double"""
    def rel(a, b):
        return float(abs(LD(a) - LD(b)) / abs(LD(b)))
    e = [rel(got[k], ref[k]) for k in ("sigma_f", "nlml", "bound")]
    if "mean" in ref and ref.get("mean") is not None:
        e.append(H.err(got["mean"], ref["mean"]) / float(ymax))
        e.append(H.err(got["var"], ref["var"]) / float(ref["sigma_f"]))
    return max(e)


@functools.lru_cache(maxsize=None)
def references(c):
    """(fp64 closed form, long-double closed form or None, e_fp64 or None) of a case -- computed once, shared, left unchanged"""
    X, y, Xs, Z, ell = data(c)
    mats = covariances(c.kind, X, Z, Xs, ell, c.eps)
    f64 = closed_form(c.kind, X, y, Z, Xs, ell, c.sn, c.eps, mats)
    if not AVAILABLE:
        return f64, None, None
    hp = closed_form_hp(c.kind, X, y, Z, Xs, ell, c.sn, c.eps, mats)
    return f64, hp, error(f64, hp, np.max(np.abs(y)))


def sharp_bound(c, e_f64, margin=16.0):
    """margin * max(the fp64 closed form's own error, (n + m) u): the bound of tests/small_cases.py"""
    return margin * max(e_f64, (c.n + c.m) * U)
