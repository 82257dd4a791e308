"""The case table of the one-workgroup kernel (csrc/smallgp.hpp: plain, MLII gradient, leave-one-out, leave-block-out, hindcast) and its
long-double references (tests/test_small_cases_host.py, tests/test_hip_small_flavours.py).  No GPU code here.

The references take the inputs AS THE DEVICE GETS THEM -- the staged factor A, lam, lam_mode and dlam of ``SmallBatch._sets`` plus
(l, sn~) -- and build K~ = (A sqrt w)(A sqrt w)^T + sn~ I, k*, k** and dK~/dlog l = l A diag(dw) A^T themselves.  Every formula is written
ONCE and parameterised on its arithmetic (``Arith``): ``HP`` is tests/hp_reference.py's long double (the reference), ``F64`` the same
formulas in fp64 through LAPACK (the comparator whose own error against long double is the unit the GPU tier measures in).

Orders, feature counts and test points are the smallest at which the kernel's mappings change: the 16-wide element mapping and its
TY = 16 thread rows (15, 16, 17; the inverse's second, third and fourth register slot from 17, 33, 49), the parity of the LDS pitch
n | 1, one feature chunk, the chunk's edge and three chunks at both ch = 16 and ch = 32 with N > n and N < n, and m = 8 bordered rows."""
import collections
import functools
import types

import numpy as np
from scipy.linalg import solve_triangular

import hp_reference as H
from test_hindcast_host import scored_rows

LD = H.LD
U = H.U
AVAILABLE = H.AVAILABLE

ORDERS = (2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128)
FEATURES = (1, 15, 16, 17, 33, 65)
MS = (0, 1, 8)
POINTS = ((1e-3, 1e-1), (0.05, 1.0), (0.7, 10.0), (0.7, 1e-6))
COND_CAP = 1e10
CV_LAYOUTS = ((1, 0), (5, 1), (8, 0), (7, 3), (32, 0), (30, 1), (2, 15))
HC_SETTINGS = ((1, 1), (1, 2), (2, 3), (32, 1))
MODES = ("refit", "fixed")
LDS_MAX = 160 * 1024 - 64                       # bytes of LDS one workgroup may ask for
CV_W = 32                                       # SM_CVW
CV_EXTRA = (2 * CV_W * (CV_W + 1) + CV_W) * 8   # Pw, Ww and tv of SmallLayout: what the leave-block-out image adds


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
Arith = collections.namedtuple("Arith", "name dtype chol fwd bwd inv small_inverse")


def _f64_inv(L):
    return solve_triangular(L.T, solve_triangular(L, np.eye(L.shape[0]), lower=True), lower=False)


HP = Arith("long double", LD, lambda A: H.cholesky(A)[0], H.forward, H.backward, H.inverse, lambda B: H.inverse(H.cholesky(B)[0]))
F64 = Arith("fp64 LAPACK", np.float64, np.linalg.cholesky, lambda L, B: solve_triangular(L, B, lower=True),
            lambda L, B: solve_triangular(L.T, B, lower=False), _f64_inv, np.linalg.inv)


# ---- LDS of a launch (csrc/smallgp_layout.hpp: SmallLayout::bytes, small_pick_chunk; test_small_cases_host.py holds them to it) ---------------
def lds_bytes(n, m, ch):
    return ((n + 1 + m) * (n | 1) + (n + m) * (ch + 1) + ch + 4 * 8 + 16 + n) * 8


def upload_chunk(nmax, mmax):
    """the feature chunk sigp_small_upload picks: the largest of 32 / 16 / 8 whose plain image fits"""
    for ch in (32, 16, 8):
        if lds_bytes(nmax, mmax, ch) <= LDS_MAX:
            return ch
    return None


def cv_chunk(nmax, mmax, before_fix=False):
    """the feature chunk of the leave-block-out launch (None: refused): the largest of {upload's, 16, 8} not above the upload's that leaves
    CV_EXTRA; ``before_fix``: the upload's chunk or nothing, as the parent did"""
    up = upload_chunk(nmax, mmax)
    if up is None:
        return None
    for ch in ((up,) if before_fix else (32, 16, 8)):
        if ch <= up and lds_bytes(nmax, mmax, ch) + CV_EXTRA <= LDS_MAX:
            return ch
    return None


def cv_order_limit(m, before_fix=False):
    """the largest order the leave-block-out launch accepts at mmax = m"""
    return max(n for n in range(2, 129) if cv_chunk(n, m, before_fix) is not None)


# ---- admissibility (include/sigp.h: sigp_small_run_cv, sigp_small_run_hindcast) --------------------------------------------------------------
def cv_admissible(n, block, gap):
    if block < 1 or gap < 0 or block + 2 * gap > CV_W or n < 2:
        return False
    f = H.cv_folds(n, block, gap)
    return bool(np.all(n - (f[:, 1] - f[:, 0]) >= 1))


def hc_admissible(n, lead, min_train):
    return 1 <= lead <= 32 and min_train >= 1 and min_train + lead - 1 <= n - 1


# ---- the formulae, once per arithmetic --------------------------------------------------------------------------------------------------------
def _score(res, var, dt):
    two_pi = 2 * np.arccos(dt(-1))
    return np.sum(np.log(two_pi * var) / 2 + res * res / (2 * var)), np.sum(res * res)


def _rows(mean, var, y, rows, dt):
    res = y[rows] - mean[rows]
    nlpd, sse = _score(res, var[rows], dt)
    return dict(mean=mean, var=var, nlpd=nlpd, sse=sse)


def loo_rows(c, mode):
    """Rasmussen & Williams 5.4.2 with the profiled signal variance: g_i = [K~^-1]_ii, residual a~_i / g_i"""
    dt, n, g = c["dtype"], c["n"], np.diag(c["P"])
    r = c["alpha"] / g
    s = (c["q"] - c["alpha"] * r) / (n - 1) if mode == "refit" else c["sigma_f"]
    return _rows(c["y"] - r, s / g, c["y"], np.arange(n), dt)


def cv_rows(c, block, gap, mode):
    """leave-block-out from P = K~^-1: residual_S = P_SS^-1 a~_S, Cov_S = s_S P_SS^-1, s_S = (y^T a~ - a~_S^T P_SS^-1 a~_S) / (n - |S|)"""
    dt, n, P, a, ar = c["dtype"], c["n"], c["P"], c["alpha"], c["arith"]
    mean, var = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    for r0, r1, c0, c1 in H.cv_folds(n, block, gap):
        Ci = ar.small_inverse(P[r0:r1, r0:r1])
        r = Ci @ a[r0:r1]
        s = (c["q"] - a[r0:r1] @ r) / (n - (r1 - r0)) if mode == "refit" else c["sigma_f"]
        mean[c0:c1] = c["y"][c0:c1] - r[c0 - r0:c1 - r0]
        var[c0:c1] = s * np.diag(Ci)[c0 - r0:c1 - r0]
    return _rows(mean, var, c["y"], np.arange(n), dt)


def hc_rows(c, lead, min_train, mode):
    """expanding-window hindcast from L~ and z = L~^-1 y (csrc/smallgp.hpp): row t is scored when s = t - lead + 1 >= min_train;
    r_t = sum_{j=s..t} L~(t,j) z_j, w_t = sum_{j=s..t} L~(t,j)^2, var_t = sigma_t w_t, sigma_t = sum_{j<s} z_j^2 / s or sigma_f.
    Also ``w`` itself (NaN where a row is not scored)."""
    dt, n, L, z = c["dtype"], c["n"], c["L"], c["z"]
    mean, var, wt = np.full(n, np.nan, dtype=dt), np.full(n, np.nan, dtype=dt), np.full(n, np.nan, dtype=dt)
    rows = scored_rows(n, lead, min_train)
    for t in rows:
        s = t - lead + 1
        r = L[t, s:t + 1] @ z[s:t + 1]
        wt[t] = L[t, s:t + 1] @ L[t, s:t + 1]
        sig = (z[:s] @ z[:s]) / s if mode == "refit" else c["sigma_f"]
        mean[t], var[t] = c["y"][t] - r, sig * wt[t]
    out = _rows(mean, var, c["y"], rows, dt)
    out["w"] = wt
    return out


def core_from_matrix(K, y, sn, ar, ks=None, kss=None, dK=None, need_inverse=True):
    """the fit of the matrix K~ in the arithmetic ``ar``: sigma_f, sigma_n, nlml[, mean, var][, grad] and what the validation rows need"""
    dt = ar.dtype
    K = np.asarray(K, dtype=dt)
    y = np.asarray(y, dtype=dt).reshape(-1)
    n = len(y)
    L = ar.chol(K)
    z = ar.fwd(L, y)
    alpha = ar.bwd(L, z)
    q = y @ alpha
    sf = q / n
    two_pi = 2 * np.arccos(dt(-1))
    c = dict(arith=ar, dtype=dt, n=n, y=y, L=L, z=z, alpha=alpha, q=q, sigma_f=sf, sigma_n=sf * dt(sn),
             nlml=dt(n) / 2 + np.sum(np.log(np.diag(L))) + dt(n) / 2 * np.log(sf) + dt(n) / 2 * np.log(two_pi))
    if ks is not None and len(ks):
        ks = np.asarray(ks, dtype=dt)
        v = ar.fwd(L, ks.T)
        c["mean"] = ks @ alpha
        c["var"] = sf * (np.asarray(kss, dtype=dt) + dt(sn) - np.sum(v * v, axis=0))
    else:
        c["mean"], c["var"] = np.zeros(0, dtype=dt), np.zeros(0, dtype=dt)
    if need_inverse:
        c["P"] = ar.inv(L)
    if dK is not None:
        dK = np.asarray(dK, dtype=dt)
        P = c["P"]
        c["grad"] = np.array([np.sum(P * dK) / 2 - (alpha @ (dK @ alpha)) / (2 * sf),
                              dt(sn) * np.trace(P) / 2 - dt(sn) * (alpha @ alpha) / (2 * sf)], dtype=dt)
    return c


def build(staged, ell, sn, ar):
    """(K~, k* [m, n], k** [m], dK~/dlog l) of a staged set (A [(n + m), N], y, lam, lam_mode, dlam) at (l, sn~) in the arithmetic ``ar``"""
    A, y, lam, mode, dlam = staged
    dt = ar.dtype
    n = len(y)
    A = np.asarray(A, dtype=dt)
    lam = np.asarray(lam, dtype=dt)
    if mode == 0:
        w = np.exp(dt(ell) * lam)
        dw = lam * w
    else:
        w = np.maximum(lam, dt(0))
        dw = np.asarray(dlam, dtype=dt)
    As = A * np.sqrt(w)
    G = As @ As.T
    K = G[:n, :n] + dt(sn) * np.eye(n, dtype=dt)
    dK = dt(ell) * ((A[:n] * dw) @ A[:n].T)
    return K, G[n:, :n], np.diag(G)[n:].copy(), dK


def core(staged, ell, sn, ar):
    K, ks, kss, dK = build(staged, ell, sn, ar)
    c = core_from_matrix(K, staged[1], sn, ar, ks, kss, dK)
    c["K"] = K
    return c


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "n N m ell sn expm seed")


def _table():
    cases = []
    for i, n in enumerate(ORDERS):
        for k, N in enumerate(FEATURES):
            m = MS[(i + k) % 3]
            for ell, sn in POINTS:                         # every (order, N) data set at all four (l, sn~): 408 "eigh" fits
                cases.append(Case(n, N, m, ell, sn, "eigh", 20261000 + 1000 * n + N))
        k = i % len(FEATURES)                              # "pade" (lam_mode 1): one data set per order
        cases.append(Case(n, FEATURES[k], MS[(i + k) % 3], POINTS[(i + 1) % 3][0], POINTS[(i + 1) % 3][1], "pade", 20261000 + 1000 * n + FEATURES[k]))
    return tuple(cases)


def _extra():
    """orders 113 .. 128 with m <= 2 for the leave-block-out launch's own chunk (16 up to n = 124, 8 above), three chunks of 8 each"""
    return tuple(Case(n, 17, (0, 1, 2)[i % 3], POINTS[i % 3][0], POINTS[i % 3][1], "eigh" if i % 4 else "pade", 20262000 + n)
                 for i, n in enumerate(range(113, 129)))


TABLE = _table()
EXTRA = _extra()


@functools.lru_cache(maxsize=None)
def dataset(n, N, m, seed):
    """X ~ N(0, 1), y = X w / sqrt(N) + 0.3 eps, Xs ~ N(0, 1), M = the graph Laplacian of the package"""
    from seaiceextentforecasting_amd.features import laplacian_M
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, N))
    y = X @ rng.standard_normal(N) / np.sqrt(N) + 0.3 * rng.standard_normal(n)
    Xs = rng.standard_normal((m, N))
    return X, y, Xs, laplacian_M(X)


def queue(sb, cases):
    """add the cases' data sets (one per distinct (n, N, m, seed)) and fits to a SmallBatch; returns the data-set id of every case"""
    ids, ds_of = {}, []
    for c in cases:
        key = (c.n, c.N, c.m, c.seed)
        if key not in ids:
            X, y, Xs, M = dataset(*key)
            ids[key] = sb.add_dataset(X, y, Xs if c.m else None, M)
        sb.add_fit(ids[key], c.ell, c.sn, expm=c.expm)
        ds_of.append(ids[key])
    return ds_of


def host_batch(cases):
    """the real SmallBatch staging without a device: a SmallBatch whose ``_sets`` / ``_fits`` hold what ``upload`` and ``run`` would send"""
    from seaiceextentforecasting_amd.smallbatch import SmallBatch
    sb = SmallBatch(types.SimpleNamespace(kernel="netdiffusion", dtype="f64"))
    queue(sb, cases)
    return sb


@functools.lru_cache(maxsize=None)
def staged(case):
    """(A, y, lam, lam_mode, dlam) of one case, through the real staging"""
    sb = host_batch((case,))
    return sb._sets[sb._fits[0][0]]


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "name cases chunk cv_chunk cv hc one_row")


def _batch(name, cases):
    cases = tuple(cases)
    ns = sorted({c.n for c in cases})
    nmax, mmax = ns[-1], max(c.m for c in cases)
    cvc = cv_chunk(nmax, mmax)
    layouts = list(CV_LAYOUTS) + ([(ns[0] - 1, 0)] if ns[-1] < 33 else [])
    cv = tuple(dict.fromkeys(bg for bg in layouts if cvc is not None and all(cv_admissible(n, *bg) for n in ns)))
    one_row = (2, ns[0] - 2) if ns[0] >= 3 else (1, 1)            # (lead, n - lead): exactly one scored row in the smallest sets
    hc = tuple(dict.fromkeys(lm for lm in HC_SETTINGS + (one_row,) if all(hc_admissible(n, *lm) for n in ns)))
    return Batch(name, cases, upload_chunk(nmax, mmax), cvc, cv, hc, one_row)


@functools.lru_cache(maxsize=None)
def batches():
    """a   every order <= 96, m up to 8: upload chunk 32, kept by the leave-block-out launch (only the layouts n = 2 admits)
    b   every order, (128, m = 8) among them: upload chunk 16; beyond the leave-block-out launch's LDS at any chunk
    mid / big   a and b from order 33: every layout and setting is admissible (big: hindcast only, for the same LDS reason)
    s2 / s15    orders {2, 3} and {15 .. 32} on their own: the small-window layouts and settings, (n_min - 1, 0) among them
    c16 / c8    orders 113 .. 124 and 125 .. 128 with m <= 2: the leave-block-out launch at its own chunk 16 and 8"""
    t = TABLE
    out = [_batch("a", [c for c in t if c.n <= 96]), _batch("b", t),
           _batch("mid", [c for c in t if 33 <= c.n <= 96]), _batch("big", [c for c in t if c.n >= 33]),
           _batch("s2", [c for c in t if c.n <= 3]), _batch("s15", [c for c in t if 15 <= c.n <= 32]),
           _batch("c16", [c for c in EXTRA if c.n <= 124]),
           _batch("c8", [c for c in EXTRA if c.n >= 125] + [c for c in t if c.n >= 127 and c.m <= 1 and c.expm == "eigh"][::5])]
    return {b.name: b for b in out}


# ---- references, computed once per (case, arithmetic) and per layout ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _core_of(case, name):
    return core(staged(case), case.ell, case.sn, HP if name == HP.name else F64)


@functools.lru_cache(maxsize=None)
def rows_of(case, name, flavour, a=0, b=0):
    """{mode: dict(mean, var, nlpd, sse[, w])} of one case: flavour 'loo', 'cv' (a, b = block, gap) or 'hc' (a, b = lead, min_train)"""
    c = _core_of(case, name)
    if flavour == "loo":
        return {mode: loo_rows(c, mode) for mode in MODES}
    if flavour == "cv":
        return {mode: cv_rows(c, a, b, mode) for mode in MODES}
    return {mode: hc_rows(c, a, b, mode) for mode in MODES}


def reference(case, ar=HP):
    return _core_of(case, ar.name)


# ---- the error of a fit in a flavour -----------------------------------------------------------------------------------------------------------
def _abs1(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref) / np.maximum(1, np.abs(ref)))) if ref.size else 0.0


def _rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref) / np.abs(ref))) if ref.size else 0.0


def _mean(got, ref, ymax):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref))) / max(1.0, ymax) if ref.size else 0.0


def plain_error(got, ref):
    """got / ref: dicts with sigma_f, sigma_n, nlml, mean [m], var [m]: |d| / max(1, |ref|) for nlML, relative for sigma_f, sigma_n and
    the variances, max|d| / max(1, max|y|) for the means"""
    ymax = float(np.max(np.abs(ref["y"])))
    return max(_abs1(got["nlml"], ref["nlml"]), _rel(got["sigma_f"], ref["sigma_f"]), _rel(got["sigma_n"], ref["sigma_n"]),
               _rel(got["var"], ref["var"]), _mean(got["mean"], ref["mean"], ymax))


def grad_error(got, ref):
    return _abs1(got, ref["grad"])


def rows_error(got, ref, y):
    """got / ref: dicts with mean [n], var [n] (NaN where a row is not scored, in both), nlpd, sse"""
    ok = ~np.isnan(np.asarray(ref["var"], dtype=np.float64))
    assert np.array_equal(ok, ~np.isnan(np.asarray(got["var"], dtype=np.float64))) and np.array_equal(ok, ~np.isnan(np.asarray(got["mean"], dtype=np.float64)))
    ymax = float(np.max(np.abs(np.asarray(y, dtype=np.float64))))
    return max(_abs1(got["nlpd"], ref["nlpd"]), _abs1(got["sse"], ref["sse"]), _rel(np.asarray(got["var"])[ok], np.asarray(ref["var"])[ok]),
               _mean(np.asarray(got["mean"])[ok], np.asarray(ref["mean"])[ok], ymax))


def bound(case, e_f64, margin=16.0):
    """margin * max(the fp64 LAPACK comparator's own error, (n + N) u): the a-priori size of the n- and N-term sums both sides form"""
    return margin * max(e_f64, (case.n + case.N) * U)
