"""The case table of the one-workgroup kernel's stationary flavours (csrc/smallgp.hpp: SmallCov::Stationary -- RBF / Matern-5/2 with one
length scale or one per feature; plain, MLII gradient, leave-one-out, leave-block-out, hindcast) and its long-double references
(tests/test_small_stationary_host.py, tests/test_hip_small_stationary.py).  No GPU code here.

The references take the inputs AS THE DEVICE FORMS THEM: the scaled features u = x / l_k, the IEEE fp64 division the workgroup itself
performs, are the input; the squared distances (direct differences, ascending k), the covariance function, h and the per-feature derivative
matrices h o D_k^2 are then built in the arithmetic asked for (``small_cases.HP``: long double, the reference; ``small_cases.F64``: the same
formulas in fp64 through NumPy and LAPACK, the comparator whose own error is the unit the GPU tier measures in).  The fit, the validation
rows, the error measures and the bound are ``small_cases``'s own (``core_from_matrix``, ``loo_rows`` / ``cv_rows`` / ``hc_rows``, ``bound``).

The exact gradient of the profiled nlML (the closed form of csrc/ardgrad.hpp), with W = K~^-1 - a~ a~^T / sigma_f:
    d nlML / d log l_k = sum_{i>j} W_ij h_ij (u_ik - u_jk)^2,   h = k~ (RBF),  h = (5/3)(1 + s) e^-s, s = sqrt(5 sq) (Matern-5/2)
    d nlML / d log sn~ = sn~ (tr K~^-1 - a~.a~ / sigma_f) / 2
and for one common scale the sum of the components over k.

Shapes: orders 2, 15, 16, 17 (the 16-wide thread mapping's edges), 33, 64, 96, 127, 128 (the LDS limit); features 1, 8, 9 (one chunk, the
edge of chunk 8), 32, 33 (the edge of chunk 32), 65 (three chunks); m = 0, 1, 8; both kernels.  Scales: one common scale; per-feature scales
spread over two decades; one feature at l = 1e6 (irrelevant: its derivative is ~ 0); one duplicated training row (sq = 0 off the diagonal)
with sn~ > 0.  cond(K~) <= (n + sn~) / sn~ <= 1.3e8 by construction (sn~ >= 1e-6): no case is ever left out for its conditioning."""
import collections
import functools

import numpy as np

import hp_reference as H
import small_cases as SC

LD = SC.LD
ORDERS = (2, 15, 16, 17, 33, 64, 96, 127, 128)
FEATURES = (1, 8, 9, 32, 33, 65)
MS = (0, 1, 8)
KERNELS = ("rbf", "matern52")
KINDS = ("iso", "ard", "irrelevant", "dup")
SNS = (1e-1, 1e-3, 1e-6)
CV_LAYOUTS = ((1, 0), (5, 1), (30, 1))
HC_SETTINGS = ((1, 2), (32, 1))

Case = collections.namedtuple("Case", "n N m kernel kind sn seed")


def _table():
    cases = []
    for i, n in enumerate(ORDERS):
        for k, N in enumerate(FEATURES):
            kind = KINDS[(i + k + k // 2) % 4]
            if N == 1 and kind in ("ard", "irrelevant"):       # one feature: nothing to spread, nothing to switch off
                kind = ("iso", "dup")[i % 2]
            cases.append(Case(n, N, MS[(i + k) % 3], KERNELS[(i + k) % 2], kind, SNS[(i + k // 2) % 3], 20271000 + 1000 * n + N))
    # ... and per order the other kernel with per-feature scales at N = 9 (two chunks of 8 where the launch's chunk is 8)
    for i, n in enumerate(ORDERS):
        cases.append(Case(n, 9, MS[i % 3], KERNELS[i % 2], "ard", SNS[i % 3], 20272000 + n))
    return tuple(cases)


TABLE = _table()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(X [n, N], y [n], Xs [m, N], scales: a float (one common scale) or an array [N])"""
    X, y, Xs, _ = SC.dataset(case.n, case.N, case.m, case.seed)
    X = X.copy()
    base = H.roundtrip(1.5 * np.sqrt(case.N))
    if case.kind == "dup":
        X[1] = X[0]
    if case.kind in ("iso", "dup"):
        return X, y, Xs, base
    if case.kind == "ard":
        ell = np.sqrt(case.N) * np.logspace(-0.5, 1.5, case.N)
        ell = ell[np.random.default_rng(case.seed).permutation(case.N)]
    else:
        ell = np.full(case.N, base)
        ell[case.N // 2] = 1e6
    return X, y, Xs, np.array([H.roundtrip(v) for v in ell])


def queue(sb, cases):
    """add the cases' data sets and fits to a SmallStationaryBatch of their kernel"""
    for c in cases:
        X, y, Xs, ell = inputs(c)
        sb.add_fit(sb.add_dataset(X, y, Xs if c.m else None), ell, c.sn)


# ---- the covariance, once per arithmetic --------------------------------------------------------------------------------------------------------
def scaled(X, Xs, ell):
    """u = [X ; Xs] / l_k: the fp64 division the workgroup performs"""
    return np.vstack([X, Xs]) / np.broadcast_to(np.asarray(ell, dtype=np.float64), (X.shape[1],))


def sq_parts(U, dt):
    """D [N][R, R], D_k(i, j) = (u_ik - u_jk)^2 in the arithmetic dt, and their sum in ascending k"""
    U = np.asarray(U, dtype=dt)
    D = np.stack([(U[:, k][:, None] - U[:, k][None, :]) ** 2 for k in range(U.shape[1])])
    sq = np.zeros(D.shape[1:], dtype=dt)
    for k in range(D.shape[0]):
        sq = sq + D[k]
    return D, sq


def cov_h(kernel, sq):
    """(k~, h) of the squared distances of the scaled features (unit length scale)"""
    dt = sq.dtype.type
    if kernel == "rbf":
        k = np.exp(-sq / dt(2))
        return k, k
    s = np.sqrt(dt(5) * sq)
    e = np.exp(-s)
    return (dt(1) + s + s * s / dt(3)) * e, dt(5) / dt(3) * (dt(1) + s) * e


def build(case, ar):
    """(K~ [n, n], k* [m, n], k** [m], dK [N][n, n] with dK_k = h o D_k^2 = dK~/dlog l_k) in the arithmetic ``ar``"""
    X, y, Xs, ell = inputs(case)
    n, dt = case.n, ar.dtype
    D, sq = sq_parts(scaled(X, Xs, ell), dt)
    k, h = cov_h(case.kernel, sq)
    K = k[:n, :n] + dt(case.sn) * np.eye(n, dtype=dt)
    return K, k[n:, :n], np.ones(case.m, dtype=dt), h[:n, :n] * D[:, :n, :n]


def gradient(c, dK, sn, common):
    """the closed form above from a ``core_from_matrix`` fit: [N + 1] (``common``: [2]) in the fit's arithmetic"""
    dt = c["dtype"]
    W = c["P"] - np.outer(c["alpha"], c["alpha"]) / c["sigma_f"]
    low = np.tril(np.ones(W.shape, dtype=bool), -1)
    gk = np.array([np.sum((W * d)[low]) for d in dK], dtype=dt)
    gs = dt(sn) * (np.trace(c["P"]) - (c["alpha"] @ c["alpha"]) / c["sigma_f"]) / 2
    if common:
        tot = dt(0)
        for v in gk:
            tot = tot + v
        gk = np.array([tot], dtype=dt)
    return np.concatenate([gk, [gs]]).astype(dt)


@functools.lru_cache(maxsize=None)
def _core_of(case, name):
    ar = SC.HP if name == SC.HP.name else SC.F64
    K, ks, kss, dK = build(case, ar)
    c = SC.core_from_matrix(K, inputs(case)[1], case.sn, ar, ks, kss)
    c["K"] = K
    c["grad"] = gradient(c, dK, case.sn, common=np.ndim(inputs(case)[3]) == 0)
    c["grad_ard"] = gradient(c, dK, case.sn, common=False)       # all N + 1 components also where the case has one scale
    return c


def reference(case, ar=SC.HP):
    return _core_of(case, ar.name)


@functools.lru_cache(maxsize=None)
def rows_of(case, name, flavour, a=0, b=0):
    """{mode: dict(mean, var, nlpd, sse)} of one case: flavour 'loo', 'cv' (a, b = block, gap) or 'hc' (a, b = lead, min_train)"""
    c = _core_of(case, name)
    if flavour == "loo":
        return {mode: SC.loo_rows(c, mode) for mode in SC.MODES}
    if flavour == "cv":
        return {mode: SC.cv_rows(c, a, b, mode) for mode in SC.MODES}
    return {mode: SC.hc_rows(c, a, b, mode) for mode in SC.MODES}


def cond_bound(case):
    """||K~||_F ||K~^-1||_F in long double: an upper bound of the 2-norm condition number"""
    c = reference(case)
    return float(np.sqrt(np.sum(c["K"] * c["K"])) * np.sqrt(np.sum(c["P"] * c["P"])))


# ---- batches: one upload each ----------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "name kernel cases cv hc")


@functools.lru_cache(maxsize=None)
def batches():
    """per kernel: s2 (order 2), lo (15 .. 17), mid (33 .. 96), big (127, 128 with m <= 1: inside the leave-block-out launch's LDS at feature
    chunk 8) and big8 (127, 128 with m = 8: upload chunk 16, beyond the leave-block-out launch); with the layouts and settings every set of
    the batch admits"""
    groups = (("s2", lambda c: c.n == 2), ("lo", lambda c: 15 <= c.n <= 17), ("mid", lambda c: 33 <= c.n <= 96),
              ("big", lambda c: c.n >= 127 and c.m <= 1), ("big8", lambda c: c.n >= 127 and c.m == 8))
    out = {}
    for kernel in KERNELS:
        for name, pick in groups:
            cases = tuple(c for c in TABLE if c.kernel == kernel and pick(c))
            if not cases:
                continue
            ns = sorted({c.n for c in cases})
            cvc = SC.cv_chunk(ns[-1], max(c.m for c in cases))
            cv = tuple(bg for bg in CV_LAYOUTS if cvc is not None and all(SC.cv_admissible(n, *bg) for n in ns))
            hc = tuple(lm for lm in HC_SETTINGS if all(SC.hc_admissible(n, *lm) for n in ns))
            out[(kernel, name)] = Batch(name, kernel, cases, cv, hc)
    return out
