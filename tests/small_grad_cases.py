"""The gradients of the leave-one-out and hindcast scores of the one-workgroup kernel (csrc/smallgp.hpp: LooGrad, HindcastGrad) in closed
form, written ONCE and parameterised on the arithmetic of tests/small_cases.py (``Arith``: long double = the reference, fp64 LAPACK = the
comparator).  No GPU code here.

With theta held a score S is a function of K~ = A diag(w) A^T + sn~ I and y alone; with its symmetric adjoint G = dS/dK~
    dS/dlog l = <G, dK~/dlog l> = l <G, A diag(dw) A^T>        dS/dlog sn~ = sn~ tr G.
The adjoints are those of tests/test_loo_ard_host.py (``loo_adjoint``) and tests/test_hindcast_host.py (``hindcast_adjoint``), which are fp64
NumPy; they are restated here on ``Arith`` and held to the originals in tests/test_small_score_grad_host.py.  The scale of a derivative is
the sum of the absolute values of its contraction's terms: sum_ij |G_ij D_ij|, and sn~ sum_i |G_ii|."""
import contextlib
import functools

import numpy as np

import small_cases as SC
from test_hindcast_host import scored_rows

CRITERIA = ("nlpd", "sse")
LDS_MAX = SC.LDS_MAX
HC_MAX_LEAD = 32            # SIGP_HINDCAST_SMALL_MAX_LEAD
FLOOR = (96, 8, 8)          # every n <= 96 with every m <= 8 and every lead <= 8 must run


# ---- LDS of the two launches (csrc/smallgp_layout.hpp; test_small_score_grad_host.py holds these to a host program's sweep) ---------------
def grad_lds_bytes(n, m, ch, lead=0):
    """SmallLayout::bytes() of LooGrad (lead = 0) / HindcastGrad: the plain image, Bc [n][ch + 1], gv [4][n], hb [n][lead]"""
    return SC.lds_bytes(n, m, ch) + (n * (ch + 1) + 4 * n + n * lead) * 8


def grad_chunk(nmax, mmax, lead=0):
    """the feature chunk of the launch (None: refused): the largest of {the upload's, 16, 8} not above the upload's whose image fits"""
    up = SC.upload_chunk(nmax, mmax)
    if up is None:
        return None
    for ch in (32, 16, 8):
        if ch <= up and grad_lds_bytes(nmax, mmax, ch, lead) <= LDS_MAX:
            return ch
    return None


def order_limit(m, lead=0):
    return max(n for n in range(1, 129) if grad_chunk(n, m, lead) is not None)


def lead_limit(n, m):
    ok = [lead for lead in range(1, HC_MAX_LEAD + 1) if grad_chunk(n, m, lead) is not None]
    return max(ok) if ok else 0


# ---- the adjoints -------------------------------------------------------------------------------------------------------------------------------
def _kappa_rho(crit, r, var):
    if crit == "sse":
        return 0 * r, 2 * r
    return 1 / (2 * var) - r * r / (2 * var * var), r / var


def loo_adjoint(c, mode, crit):
    """G of the leave-one-out score: 1/2 (v a^T + a v^T) + P diag(gamma) P + eps a a^T (csrc/looard.hpp)"""
    n, P, a, q = c["n"], c["P"], c["alpha"], c["q"]
    g = np.diag(P).copy()
    r = a / g
    s = (q - a * r) / (n - 1) if mode == "refit" else np.full(n, c["sigma_f"], dtype=c["dtype"])
    kappa, rho = _kappa_rho(crit, r, s / g)
    beta = -rho / g
    gamma = kappa * s / g ** 2 + rho * a / g ** 2
    eps = -np.sum(kappa / g) / ((n - 1) if mode == "refit" else n)
    if mode == "refit":
        beta = beta + 2 * kappa * a / (g ** 2 * (n - 1))
        gamma = gamma - kappa * a * a / (g ** 3 * (n - 1))
    v = P @ beta
    return (np.outer(v, a) + np.outer(a, v)) / 2 + (P * gamma) @ P + eps * np.outer(a, a)


def hindcast_adjoint(c, lead, min_train, mode, crit):
    """G = U C U^T of the hindcast score, U = L~^-T, C from A = L~^T B - zbar z^T on its lower triangle (csrc/hindcast.hpp)"""
    dt, n, L, z, ar = c["dtype"], c["n"], c["L"], c["z"], c["arith"]
    B = np.zeros((n, n), dtype=dt)
    zbar = np.zeros(n, dtype=dt)
    for t in scored_rows(n, lead, min_train):
        s = t - lead + 1
        r = L[t, s:t + 1] @ z[s:t + 1]
        w = L[t, s:t + 1] @ L[t, s:t + 1]
        sig = (z[:s] @ z[:s]) / s if mode == "refit" else c["sigma_f"]
        kappa, rho = _kappa_rho(crit, r, sig * w)
        B[t, s:t + 1] = rho * z[s:t + 1] + 2 * kappa * sig * L[t, s:t + 1]
        zbar[s:t + 1] += rho * L[t, s:t + 1]
        if mode == "refit":
            zbar[:s] += 2 * z[:s] * kappa * w / s
        else:
            zbar += 2 * z * kappa * w / n
    T = np.tril(L.T @ B - np.outer(zbar, z))
    T[np.diag_indices(n)] /= 2
    U = ar.fwd(L, np.eye(n, dtype=dt)).T
    return U @ ((T + T.T) / 2) @ U.T


def contract(G, dK, sn):
    """(grad [2], S [2]) of an adjoint: <G, dK~/dlog l> and sn~ tr G with the sums of the absolute values of their terms"""
    dt = G.dtype.type
    return (np.array([np.sum(G * dK), dt(sn) * np.trace(G)], dtype=G.dtype),
            np.array([np.sum(np.abs(G * dK)), dt(sn) * np.sum(np.abs(np.diag(G)))], dtype=G.dtype))


def score_grad(staged, ell, sn, ar, flavour, mode, crit, lead=0, min_train=0):
    """dict(score, grad [2], S [2]) of one staged set at (l, sn~) in the arithmetic ``ar``; flavour 'loo' or 'hc'.  A lam_mode 1 set without
    dweights (dlam None) has NaN in grad[0] and S[0]."""
    A, y, lam, lmode, dlam = staged
    K, ks, kss, dK = SC.build((A, y, lam, lmode, np.full(len(lam), np.nan) if dlam is None else dlam), ell, sn, ar)
    c = SC.core_from_matrix(K, y, sn, ar)
    if flavour == "loo":
        rows, G = SC.loo_rows(c, mode), loo_adjoint(c, mode, crit)
    else:
        rows, G = SC.hc_rows(c, lead, min_train, mode), hindcast_adjoint(c, lead, min_train, mode, crit)
    grad, S = contract(G, dK, sn)
    return dict(score=rows[crit], grad=grad, S=S, G=G)


def score(staged, ell, sn, ar, flavour, mode, crit, lead=0, min_train=0):
    """the score alone, from the rows ``small_cases`` defines"""
    K, ks, kss, dK = SC.build(staged, ell, sn, ar)
    c = SC.core_from_matrix(K, staged[1], sn, ar, need_inverse=flavour == "loo")
    return (SC.loo_rows(c, mode) if flavour == "loo" else SC.hc_rows(c, lead, min_train, mode))[crit]


def central_difference(staged, ell, sn, flavour, mode, crit, lead=0, min_train=0, h=1e-5):
    """[dS/dlog l, dS/dlog sn~] by central differences of ``score`` in long double, step h in log theta (lam_mode 0 sets)"""
    assert staged[3] == 0
    LD = SC.LD
    e = np.exp(LD(h))
    f = lambda l, s: score(staged, l, s, SC.HP, flavour, mode, crit, lead, min_train)
    return np.array([(f(LD(ell) * e, LD(sn)) - f(LD(ell) / e, LD(sn))) / (2 * LD(h)), (f(LD(ell), LD(sn) * e) - f(LD(ell), LD(sn) / e)) / (2 * LD(h))], dtype=LD)


@functools.lru_cache(maxsize=None)
def reference(case, arith_name, flavour, mode, crit, lead=0, min_train=0, dweights=True):
    """dict(score, grad [2], S [2]) of a table case from its (cached) ``small_cases.reference``; ``dweights=False``: a lam_mode 1 set whose
    dweights were not uploaded -- NaN in grad[0] and S[0]"""
    ar = SC.HP if arith_name == SC.HP.name else SC.F64
    c = SC.reference(case, ar)
    dK = SC.build(SC.staged(case), case.ell, case.sn, ar)[3]
    if flavour == "loo":
        rows, G = SC.rows_of(case, ar.name, "loo")[mode], loo_adjoint(c, mode, crit)
    else:
        rows, G = SC.rows_of(case, ar.name, "hc", lead, min_train)[mode], hindcast_adjoint(c, lead, min_train, mode, crit)
    grad, S = contract(G, dK, case.sn)
    if not dweights:
        grad[0] = S[0] = np.nan
    return dict(score=rows[crit], grad=grad, S=S)


def grad_error(got, ref):
    """max over the two entries of |got - ref| / S; an entry whose reference is NaN must be NaN, one whose terms are all zero (a single
    feature: lam = 0, dw = 0) must be zero"""
    e = 0.0
    for k in range(2):
        if np.isnan(np.float64(ref["grad"][k])):
            assert np.isnan(got[k]), (got, ref["grad"])
        elif ref["S"][k] == 0:
            assert got[k] == 0, (got, ref["grad"])
        else:
            e = max(e, float(abs(SC.LD(got[k]) - ref["grad"][k]) / ref["S"][k]))
    return e


# ---- the comparator's error ------------------------------------------------------------------------------------------------------------------------
# The unit the GPU tier measures in is the error of an fp64 NumPy evaluation of the same formulas.  A gradient entry is ONE number, and on an
# ill-conditioned fit one evaluation's error in one number is a draw: K~ itself is known only to its rounding (every entry an N-term fp64 sum),
# and moving its entries by relative amounts within one unit roundoff -- another admissible rounding of the same K~ -- moves the comparator's
# error in d/dlog sn~ of a fit of condition 1.3e8 between 8e-12 and 8e-9.  So the unit is the MEDIAN of the comparator's error over DRAWS
# evaluations: K~ as NumPy rounds it, and DRAWS - 1 copies with every entry moved by a seeded relative amount uniform in [-u, u] (symmetric).
# The median, not the maximum: it is the typical error of an fp64 evaluation, and a single unlucky draw does not widen the bound.  Nothing of
# the device enters it.
DRAWS = 8


@functools.lru_cache(maxsize=None)
def _comparator_core(case, draw):
    st = SC.staged(case)
    K, ks, kss, dK = SC.build(st, case.ell, case.sn, SC.F64)
    if draw:
        n = K.shape[0]
        E = np.tril(np.random.default_rng(1000 * case.seed + draw).uniform(-1.0, 1.0, (n, n))) * SC.U
        K = K * (1.0 + E + np.tril(E, -1).T)
    return SC.core_from_matrix(K, st[1], case.sn, SC.F64), dK


@functools.lru_cache(maxsize=None)
def comparator_error(case, flavour, mode, crit, lead=0, min_train=0, dweights=True):
    """the median over DRAWS fp64 evaluations of ``grad_error`` against the long-double reference"""
    try:                                            # orders <= 128: a BLAS thread pool only gets in the way
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = contextlib.nullcontext
    ref = reference(case, SC.HP.name, flavour, mode, crit, lead, min_train, dweights)
    errs = []
    with threadpool_limits(1):
        for draw in range(DRAWS):
            c, dK = _comparator_core(case, draw)
            G = loo_adjoint(c, mode, crit) if flavour == "loo" else hindcast_adjoint(c, lead, min_train, mode, crit)
            grad, _ = contract(G, dK, case.sn)
            if not dweights:
                grad[0] = np.nan
            errs.append(grad_error(np.asarray(grad, dtype=np.float64), ref))
    return float(np.median(errs))


# ---- the GPU tier's cases: the smallest shapes at which each piece of the two tails can go wrong -----------------------------------------------
ACC_ORDERS = (2, 3, 16, 17, 33, 49, 64, 65, 96)


def _point(n, N, m, expm, seed):
    """the first of small_cases.POINTS (from a start that rotates with the order) whose K~ stays under the condition cap"""
    for k in range(len(SC.POINTS)):
        ell, sn = SC.POINTS[(n + k) % len(SC.POINTS)]
        c = SC.Case(n, N, m, ell, sn, expm, seed)
        if SC.H.cond2(np.asarray(SC.build(SC.staged(c), ell, sn, SC.F64)[0], dtype=np.float64)) < SC.COND_CAP:
            return c
    raise AssertionError("no admissible point for n = %d, N = %d" % (n, N))


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """name -> cases.  N cycles through 1, 17, 65 (one chunk, its edge region, three chunks of 32) and m through 0, 8 along the orders.
    small   orders 2, 3                 leave-one-out at n - 1 = 1; the hindcast settings (1, 1) and, at n = 3, (1, 2): one scored row
    mid     orders 16 .. 96, a 'pade' set (lam_mode 1) among them: every setting with lead <= 8
    wide    the members of mid from order 33: lead = 32, the largest the entry takes (at n = 33 exactly one scored row)
    big0 / big8   the largest orders the two launches admit at m = 0 (128) and m = 8 (127), at their own feature chunk 8: N = 1 (one chunk
            whatever its size: the score entry's bytes) and N = 17 (three chunks)"""
    Ns, ms = (1, 17, 65), (0, 8)
    small = [_point(n, Ns[(i + 1) % 3], ms[i % 2], "eigh", 20266000 + n) for i, n in enumerate(ACC_ORDERS[:2])]
    mid = [_point(n, Ns[i % 3], ms[i % 2], "eigh", 20266000 + n) for i, n in enumerate(ACC_ORDERS[2:])]
    mid += [_point(17, 65, 8, "eigh", 20266117), _point(64, 1, 0, "eigh", 20266164), _point(33, 17, 8, "pade", 20266233)]
    big0 = [_point(128, N, 0, "eigh", 20266300 + N) for N in (1, 17)]
    big8 = [_point(127, N, 8, "eigh", 20266400 + N) for N in (1, 17)]
    return dict(small=tuple(small), mid=tuple(mid), wide=tuple(c for c in mid if c.n >= 33), big0=tuple(big0), big8=tuple(big8))


# per batch the hindcast settings (lead, min_train); leave-one-out runs on every batch but wide
GPU_HC = dict(small=((1, 1),), mid=((1, 1), (1, 2), (2, 3), (8, 1)), wide=((32, 1),), big0=((1, 2), (6, 1)), big8=((1, 2),))
