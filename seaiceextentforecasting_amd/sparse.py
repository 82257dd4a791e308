"""Inducing-point (sparse) GP regression for n past the dense limit (include/sigp.h: sigp_sparse_fit / sigp_sparse_predict): the host
side of ``GPR.sparse_fit`` / ``GPR.sparse_predict`` and the choice of inducing points.  The fit itself runs on the device; only
``select_inducing`` is host arithmetic (NumPy, O(n m d))."""
import numpy as np

from . import _lib as L
from .gpr import LinAlgError


def select_inducing(X, m, method="random", seed=0):
    """``m`` rows of ``X`` [n, d] to serve as inducing points, as an array [m, d].

    ``random``: a seeded draw without replacement.  ``farthest``: greedy farthest-point selection from a seeded first row -- every next
    point is the row farthest from the ones chosen so far (O(n m d)), which spreads the points over the data instead of following its
    density.  Either way the result consists of distinct rows of ``X`` (no row index twice), so distinct rows of ``X`` give inducing
    points without duplicates of each other."""
    X = L.f64(X, 2)
    n = X.shape[0]
    m = int(m)
    if m < 1 or m > n:
        raise ValueError("select_inducing: 1 <= m <= n = %d required (m = %d)" % (n, m))
    if method not in ("random", "farthest"):
        raise ValueError("select_inducing: method must be 'random' or 'farthest'")
    rng = np.random.default_rng(seed)
    if method == "random":
        return X[np.sort(rng.choice(n, size=m, replace=False))].copy()
    idx = np.empty(m, dtype=np.int64)
    idx[0] = int(rng.integers(n))
    diff = X - X[idx[0]]
    dist = np.einsum("ij,ij->i", diff, diff)
    dist[idx[0]] = -1.0                                   # chosen rows are never chosen again, even among coincident points
    for k in range(1, m):
        idx[k] = int(np.argmax(dist))
        diff = X - X[idx[k]]
        dist = np.minimum(dist, np.einsum("ij,ij->i", diff, diff))
        dist[idx[:k + 1]] = -1.0
    return X[idx].copy()


def _ell_vector(ell, d):
    """(ell as the library takes it [1] or [d], the value kept as ``sparse_ell_``)"""
    if np.ndim(ell) == 0:
        vec = np.array([float(ell)])
    else:
        vec = L.f64(np.asarray(ell, dtype=np.float64), 1).copy()
        if vec.shape[0] != d:
            raise ValueError("sparse_fit: ell must be a scalar or hold one length scale per feature (%d), got %d" % (d, vec.shape[0]))
    if not np.all(np.isfinite(vec)) or not np.all(vec > 0):
        raise ValueError("sparse_fit: every length scale must be finite and > 0")
    return vec


def sparse_fit(gp, X, y, Z, ell, sn_tilde, jitter=1e-8, kind=None):
    """``GPR.sparse_fit``: see there."""
    kind = gp.kernel if kind is None else kind
    if kind not in ("rbf", "matern52"):
        raise ValueError("sparse_fit: kind must be 'rbf' or 'matern52' (the reference kernel is not covered), got %r" % (kind,))
    if gp.dtype != "f64":
        raise ValueError("sparse_fit: fp64 engine only")
    X = L.f64(X, 2)
    y = L.f64(np.asarray(y).reshape(-1), 1)
    Z = L.f64(np.atleast_2d(Z), 2)
    n, d = X.shape
    if y.shape[0] != n:
        raise ValueError("sparse_fit: X has %d rows but y has %d" % (n, y.shape[0]))
    if Z.shape[1] != d:
        raise ValueError("sparse_fit: Z must have %d columns" % d)
    m = Z.shape[0]
    if m < 1 or m > L.SPARSE_MAX_INDUCING:
        raise ValueError("sparse_fit: 1 <= m <= %d inducing points required (m = %d)" % (L.SPARSE_MAX_INDUCING, m))
    if not float(sn_tilde) > 0:
        raise ValueError("sparse_fit: sn_tilde > 0 required")
    if not float(jitter) >= 0:
        raise ValueError("sparse_fit: jitter >= 0 required")
    vec = _ell_vector(ell, d)
    out = np.zeros(4)
    gp._fitted = False                 # the dense entries refuse as before any fit
    gp._sparse_d = None
    rc = gp._lib.sigp_sparse_fit(gp._h, L.KERNEL_IDS[kind], L.ptr(vec), vec.shape[0], float(sn_tilde), float(jitter), L.ptr(X), n, d, d, L.ptr(y),
                                 L.ptr(Z), m, d, L.ptr(out))
    if rc == L.NOT_SPD:
        msg = gp._lib.sigp_last_error(gp._h)
        raise LinAlgError("sparse_fit: %s" % (msg.decode() if msg else "Matrix is not positive definite"), int(out[3]))
    gp._check(rc, "sparse_fit")
    gp._sparse_d = d
    gp.sparse_ell_ = float(vec[0]) if np.ndim(ell) == 0 else vec
    gp.sparse_sigma_f_, gp.sparse_nlml_, gp.sparse_bound_ = float(out[0]), float(out[1]), float(out[2])
    return dict(sigma_f=float(out[0]), nlml=float(out[1]), bound=float(out[2]), n=int(n), m=int(m))


def sparse_predict(gp, Xs):
    """``GPR.sparse_predict``: see there."""
    d = getattr(gp, "_sparse_d", None)
    if d is None:
        raise RuntimeError("sparse_predict: call sparse_fit() first")
    Xs = L.f64(np.atleast_2d(Xs), 2)
    if Xs.shape[1] != d:
        raise ValueError("sparse_predict: Xs must have %d columns" % d)
    ms = Xs.shape[0]
    if ms < 1:
        raise ValueError("sparse_predict: at least one test point required")
    mean, var = np.zeros(ms), np.zeros(ms)
    gp._check(gp._lib.sigp_sparse_predict(gp._h, L.ptr(Xs), ms, Xs.shape[1], L.ptr(mean), L.ptr(var)), "sparse_predict")
    return mean, var
