"""The gradient of the leave-block-out scores of the one-workgroup kernel (csrc/smallgp.hpp: CvGrad) in closed form, on the arithmetic of
tests/small_cases.py (``Arith``: long double = the reference, fp64 LAPACK = the comparator), built like ``loo_adjoint`` of
tests/small_grad_cases.py, whose ``contract``, ``grad_error`` and median-of-``DRAWS`` comparator protocol it reuses.  No GPU code here.

The adjoint G = dS/dK~ is that of tests/test_cv_ard_host.py (``cv_adjoint``, fp64 NumPy; csrc/cvard.hpp), restated on ``Arith`` and held to the
original in tests/test_small_cv_grad_host.py."""
import contextlib
import functools

import numpy as np

import small_cases as SC
import small_grad_cases as GC

CRITERIA = GC.CRITERIA
LDS_MAX = SC.LDS_MAX
MAX_WINDOW = SC.CV_W        # SIGP_CV_SMALL_MAX_WINDOW
FLOOR = (96, 8, 32)         # every n <= 96 with every m <= 8 and every window <= 32 must run


# ---- LDS of the launch (csrc/smallgp_layout.hpp; test_small_cv_grad_host.py holds these to a host program's sweep) -------------------------
def cv_grad_lds_bytes(n, m, ch, window):
    """SmallLayout::bytes() of CvGrad: the leave-block-out image (plain, Pw, Ww, tv), Bc [n][ch + 1], gv [4][n], the band [n][window]"""
    return SC.lds_bytes(n, m, ch) + SC.CV_EXTRA + (n * (ch + 1) + 4 * n + n * window) * 8


def cv_grad_chunk(nmax, mmax, window):
    """the feature chunk of the launch (None: refused): the largest of {the upload's, 16, 8} not above the upload's whose image fits"""
    up = SC.upload_chunk(nmax, mmax)
    if up is None:
        return None
    for ch in (32, 16, 8):
        if ch <= up and cv_grad_lds_bytes(nmax, mmax, ch, window) <= LDS_MAX:
            return ch
    return None


def order_limit(m, window):
    return max(n for n in range(1, 129) if cv_grad_chunk(n, m, window) is not None)


# ---- the adjoint ----------------------------------------------------------------------------------------------------------------------------
def cv_adjoint(c, block, gap, mode, crit):
    """G of the leave-block-out score: 1/2 (v a^T + a v^T) + P B P + eps a a^T, beta, B, eps assembled fold by fold (csrc/cvard.hpp)"""
    dt, n, P, a, q, ar = c["dtype"], c["n"], c["P"], c["alpha"], c["q"], c["arith"]
    beta, B, eps = np.zeros(n, dtype=dt), np.zeros((n, n), dtype=dt), dt(0)
    for r0, r1, c0, c1 in SC.H.cv_folds(n, block, gap):
        w = r1 - r0
        Hm = ar.small_inverse(P[r0:r1, r0:r1])
        r = Hm @ a[r0:r1]
        s = (q - a[r0:r1] @ r) / (n - w) if mode == "refit" else c["sigma_f"]
        sl = slice(c0 - r0, c1 - r0)
        hd = np.diag(Hm)
        rbar, kappa = np.zeros(w, dtype=dt), np.zeros(w, dtype=dt)
        kappa[sl], rbar[sl] = GC._kappa_rho(crit, r[sl], s * hd[sl])
        t = Hm @ rbar
        sbar = np.sum(kappa * hd)
        bf = -t
        Bf = (np.outer(t, r) + np.outer(r, t)) / 2 + s * ((Hm * kappa) @ Hm)
        if mode == "refit":
            bf = bf + 2 * sbar * r / (n - w)
            Bf = Bf - sbar * np.outer(r, r) / (n - w)
            eps = eps - sbar / (n - w)
        else:
            eps = eps - sbar / n
        beta[r0:r1] += bf
        B[r0:r1, r0:r1] += Bf
    v = P @ beta
    return (np.outer(v, a) + np.outer(a, v)) / 2 + P @ B @ P + eps * np.outer(a, a)


def score_grad(staged, ell, sn, ar, block, gap, mode, crit):
    """dict(score, grad [2], S [2], G) of one staged set at (l, sn~) in the arithmetic ``ar``"""
    A, y, lam, lmode, dlam = staged
    K, ks, kss, dK = SC.build((A, y, lam, lmode, np.full(len(lam), np.nan) if dlam is None else dlam), ell, sn, ar)
    c = SC.core_from_matrix(K, y, sn, ar)
    G = cv_adjoint(c, block, gap, mode, crit)
    grad, S = GC.contract(G, dK, sn)
    return dict(score=SC.cv_rows(c, block, gap, mode)[crit], grad=grad, S=S, G=G)


def score(staged, ell, sn, ar, block, gap, mode, crit):
    K, ks, kss, dK = SC.build(staged, ell, sn, ar)
    return SC.cv_rows(SC.core_from_matrix(K, staged[1], sn, ar), block, gap, mode)[crit]


def central_difference(staged, ell, sn, block, gap, mode, crit, h=1e-5):
    """[dS/dlog l, dS/dlog sn~] by central differences of ``score`` in long double, step h in log theta (lam_mode 0 sets)"""
    assert staged[3] == 0
    LD = SC.LD
    e = np.exp(LD(h))
    f = lambda l, s: score(staged, l, s, SC.HP, block, gap, mode, crit)
    return np.array([(f(LD(ell) * e, LD(sn)) - f(LD(ell) / e, LD(sn))) / (2 * LD(h)), (f(LD(ell), LD(sn) * e) - f(LD(ell), LD(sn) / e)) / (2 * LD(h))], dtype=LD)


@functools.lru_cache(maxsize=None)
def reference(case, arith_name, block, gap, mode, crit, dweights=True):
    """dict(score, grad [2], S [2]) of a table case from its (cached) ``small_cases.reference``; ``dweights=False``: a lam_mode 1 set whose
    dweights were not uploaded -- NaN in grad[0] and S[0]"""
    ar = SC.HP if arith_name == SC.HP.name else SC.F64
    c = SC.reference(case, ar)
    dK = SC.build(SC.staged(case), case.ell, case.sn, ar)[3]
    grad, S = GC.contract(cv_adjoint(c, block, gap, mode, crit), dK, case.sn)
    if not dweights:
        grad[0] = S[0] = np.nan
    return dict(score=SC.rows_of(case, ar.name, "cv", block, gap)[mode][crit], grad=grad, S=S)


@functools.lru_cache(maxsize=None)
def comparator_error(case, block, gap, mode, crit, dweights=True):
    """the median over ``small_grad_cases.DRAWS`` fp64 evaluations (the same admissible roundings of K~) of ``grad_error`` against the
    long-double reference"""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = contextlib.nullcontext
    ref = reference(case, SC.HP.name, block, gap, mode, crit, dweights)
    errs = []
    with threadpool_limits(1):
        for draw in range(GC.DRAWS):
            c, dK = GC._comparator_core(case, draw)
            grad, _ = GC.contract(cv_adjoint(c, block, gap, mode, crit), dK, case.sn)
            if not dweights:
                grad[0] = np.nan
            errs.append(GC.grad_error(np.asarray(grad, dtype=np.float64), ref))
    return float(np.median(errs))


# ---- the GPU tier's cases -------------------------------------------------------------------------------------------------------------------
BIG_LAYOUT = (5, 0)


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """name -> cases.  small, mid and wide are those of ``small_grad_cases.gpu_batches`` (orders 2, 3; 16 .. 96 with a 'pade' member, N cycling
    1 / 17 / 65 and m 0 / 8; mid's members from order 33), so the fits' long-double references are shared with that tier.
    big0 / big8   the largest order the layout admits for the window of BIG_LAYOUT at m = 0 / m = 8, at its own feature chunk 8: N = 1 and N = 17"""
    g = GC.gpu_batches()
    w = BIG_LAYOUT[0] + 2 * BIG_LAYOUT[1]
    n0, n8 = order_limit(0, w), order_limit(8, w)
    big0 = tuple(GC._point(n0, N, 0, "eigh", 20269300 + N) for N in (1, 17))
    big8 = tuple(GC._point(n8, N, 8, "eigh", 20269400 + N) for N in (1, 17))
    return dict(small=g["small"], mid=g["mid"], wide=g["wide"], big0=big0, big8=big8)


_LAYOUTS = dict(small=((1, 0),), mid=((1, 0), (5, 1), (8, 0), (7, 3), (2, 15)), wide=((32, 0), (30, 1), (2, 15)), big0=(BIG_LAYOUT,), big8=(BIG_LAYOUT,))


def layouts(name):
    """the (block, gap) a batch runs: of those the issue lists for it, the ones every member admits"""
    return tuple(bg for bg in _LAYOUTS[name] if all(SC.cv_admissible(c.n, *bg) for c in gpu_batches()[name]))
