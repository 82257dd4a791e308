"""GPU tier of the per-feature (ARD) gradients of the expanding-window hindcast scores in lockstep groups: ``GPR.hindcast_ard_batch``,
``GPR.hindcast_objective_batch``, ``GPR.optimize_hindcast_batch`` and the C entry point sigp_hindcast_grad_ard_batch.

Reference and error convention are those of tests/test_hip_hindcast_ard.py: the forward-mode NumPy closed form of
tests/test_hindcast_host.py and, as its second route, the NumPy adjoint; every gradient error measured against the per-component scale S,
the device within max(1e-8, 10 x spread) where spread is the disagreement of the two routes; a case counts only when spread <= 1e-8
(``_check`` asserts it: none may be dropped; on the problems below the worst spread is 5.6e-14, at n = 2).  Problems are those of
tests/test_hip_loo_ard_batch.py: B = 2 data sets, F = 7 members with scales of their own, sn~ alternating 1e-2 / 3e-2, first = 1; scales
belong to a fit, not to a data set."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_hindcast_host import hindcast_ard_closed_form, hindcast_closed_form
from test_hip_hindcast_ard import CRITERIA, KINDS, MODES, _check
from test_hip_loo_ard_batch import SNS, _problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def L():
    from seaiceextentforecasting_amd import _lib
    return _lib


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


@functools.lru_cache(maxsize=None)
def _references(kind, n, d, lead, mt, mode):
    """per member (the closed form with its two routes, the predictions' closed form): computed once, shared by the tests below"""
    Xb, yb, ells, sn, _, ds = _problem(n, d)
    out = []
    for i in range(len(ds)):
        X, y = Xb[ds[i]], yb[ds[i]]
        U = X / ells[i]
        out.append((hindcast_ard_closed_form(kind, X, y, ells[i], sn[i], lead, mt, mode),
                    hindcast_closed_form(O.cov_unit(kind, U, U, 1.0) + sn[i] * np.eye(n), y, lead, mt, mode)))
    return out


def _windows(n):
    w = [(1, 1)] + ([(5, 3)] if n > 7 else [])
    return w + ([(128, 2)] if n == 300 else [])


# ---- 1. every member against the closed form ---------------------------------------------------------------------------------------------------
# (n, d): the minimum; odd sizes below one block; one row past a block; three blocks with a lead that straddles two of them (128, 2)
SHAPES = [(2, 1), (37, 3), (129, 8), (300, 8)]
CASES = [(kind, n, d, w) for kind in KINDS for n, d in SHAPES for w in _windows(n)] + [("rbf", 200, 65, (5, 3))]      # ... and d past one 64-column pad


@pytest.mark.parametrize("kind,n,d,window", CASES)
def test_members_equal_the_closed_form(S, kind, n, d, window):
    """B = 2 data sets, F = 7 members in groups of 3, 3, 1 (a partial last group), first = 1; both criteria, both sigma modes"""
    lead, mt = window
    Xb, yb, ells, sn, theta, ds = _problem(n, d)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            refs = _references(kind, n, d, lead, mt, mode)
            for crit in CRITERIA:
                key = crit[9:]
                r = gp.hindcast_ard_batch(theta, lead=lead, min_train=mt, first=1, criterion=crit, sigma_f=mode, group=3, predictions=True)
                assert set(r) == {"value", "grad", "mean", "var", "nlpd", "sse"}
                assert r["value"].shape == (7,) and r["grad"].shape == (7, d + 1) and r["mean"].shape == (7, n) and r["var"].shape == (7, n)
                assert r["nlpd"].shape == (7,) and r["sse"].shape == (7,)
                assert _same_bits(r["value"], r[key])
                for i in range(7):
                    a, cf = refs[i]
                    spread = np.abs(a[key + "_grad"] - a[key + "_adj"]) / a[key + "_S"]
                    _check("%s n=%d d=%d lead=%d min_train=%d %s %s member %d" % (kind, n, d, lead, mt, mode, crit, i), r["grad"][i], a[key + "_grad"], a[key + "_S"], spread)
                    for k in ("nlpd", "sse"):
                        assert abs(float(r[k][i]) - a[k]) <= 1e-8 * abs(a[k]), (mode, crit, i, k, r[k][i], a[k])
                    if crit == CRITERIA[0]:           # (the predictions do not depend on the criterion)
                        sc, y = cf["scored"], yb[ds[i]]
                        assert np.all(np.isnan(np.delete(r["mean"][i], sc))) and np.all(np.isnan(np.delete(r["var"][i], sc))), (mode, i)
                        assert np.max(np.abs(r["mean"][i][sc] - cf["mean"][sc])) <= 1e-8 * np.max(np.abs(y)), (mode, i)     # (the scales of test_hip_hindcast.py)
                        assert np.all(np.abs(r["var"][i][sc] - cf["var"][sc]) <= 1e-8 * cf["var"][sc]), (mode, i)
        v0, g0 = gp.hindcast_ard_batch(theta, lead=lead, min_train=mt, first=1, group=3, grad=None)
        assert g0 is None and v0.shape == (7,)


# ---- 2. the bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", [(129, 8), (300, 8)])
def test_members_have_the_bits_of_the_single_fit_whatever_the_group(S, kind, n, d):
    lead, mt = 3, 5
    Xb, yb, _, sn, theta, ds = _problem(n, d)
    F = len(ds)
    ells = np.stack([S.GPR._exp(t[:d]) for t in theta])        # the library's own exp(theta): the scales the staging divides by
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                kw = dict(lead=lead, min_train=mt, first=1, criterion=crit, sigma_f=mode)
                r3 = gp.hindcast_ard_batch(theta, group=3, predictions=True, **kw)
                v3, g3 = r3["value"], r3["grad"]
                v3b, g3b = gp.hindcast_ard_batch(theta, group=3, **kw)
                v1, g1 = gp.hindcast_ard_batch(theta, group=1, **kw)
                v8, g8 = gp.hindcast_ard_batch(theta, group=8, **kw)
                v0, g0 = gp.hindcast_ard_batch(theta, group=3, grad=None, **kw)
                assert _same_bits(v3, v3b) and _same_bits(g3, g3b), "two calls differ"
                assert _same_bits(v3, v1) and _same_bits(g3, g1) and _same_bits(v3, v8) and _same_bits(g3, g8), "a member's bits depend on its group"
                assert g0 is None and _same_bits(v0, v3), "grad=None changes the value"
                for i in range(F):
                    gp.set_data(Xb[ds[i]], yb[ds[i]])
                    s = gp.hindcast_ard(theta[i], lead=lead, min_train=mt, criterion=crit, sigma_f=mode, predictions=True)
                    assert _same_bits(v3[i], s["value"]), ("value of member", mode, crit, i, v3[i], s["value"])
                    assert _same_bits(g3[i], s["grad"]), ("gradient of member", mode, crit, i, g3[i], s["grad"])
                    assert _same_bits(r3["mean"][i], s["mean"]) and _same_bits(r3["var"][i], s["var"]), ("predictions of member", mode, crit, i)
            r = gp.hindcast_ard_batch(theta, lead=lead, min_train=mt, first=1, sigma_f=mode, group=3, predictions=True, grad=None)
            assert r["grad"] is None
            # staging is exactly a division: hindcast_batch on the pre-divided data at ell = 1
            with S.GPR(kernel=kind) as pre:
                pre.upload_batch(np.stack([Xb[ds[i]] / ells[i] for i in range(F)]), np.stack([yb[ds[i]] for i in range(F)]), None, group=3)
                want = pre.hindcast_batch(np.ones(F), S.GPR._exp(theta[:, d]), lead=lead, min_train=mt, sigma_f=mode, group=3, predictions=True)
            for k in ("nlpd", "sse", "mean", "var"):
                assert _same_bits(r[k], want[k]), ("predictions=True against hindcast_batch on pre-divided data", mode, k)


def test_the_w_kernel_does_not_show_in_the_bits(S, L):
    """The group driver chooses the W kernel by n_pad alone; the debug library's measurement switch ``hindcast_w_lds`` = 0 keeps a group on
    the single fit's kernel, the path groups beyond the LDS limit take: the same values and gradients bit for bit.  The product library
    refuses the switch."""
    n, d = 300, 8
    Xb, yb, _, _, theta, _ = _problem(n, d)
    Xc, yc, tc = L.f64(Xb, 3), L.f64(yb, 2), L.f64(theta, 2)
    F = len(theta)
    with S.GPR(kernel="rbf") as gp:
        with pytest.raises(ValueError, match="libsigp_debug"):
            gp.set_option("hindcast_w_lds", 0)
        gp.upload_batch(Xb, yb, None, group=3)
        v, g = gp.hindcast_ard_batch(theta, lead=5, min_train=3, first=1, group=3)
    dbg = L.load(debug=True)
    h = C.c_void_p()
    assert dbg.sigp_create(C.byref(h), 0, 0) == L.OK
    try:
        assert dbg.sigp_batch_upload(h, 2, L.ptr(Xc), n * d, L.ptr(yc), n, None, 0, n, d, 0) == L.OK
        assert dbg.sigp_set_option(h, b"group", 3) == L.OK
        for w_lds in (-1, 0):
            assert dbg.sigp_set_option(h, b"hindcast_w_lds", w_lds) == L.OK
            sc, gr = np.zeros((F, 2)), np.zeros((F, d + 1))
            assert dbg.sigp_hindcast_grad_ard_batch(h, 1, F, L.KERNEL_IDS["rbf"], L.ptr(tc), d + 1, d + 1, 5, 3, 0, 0, None, None, 0, L.ptr(sc), L.ptr(gr), d + 1) == L.OK
            assert np.all(np.isfinite(gr)) and _same_bits(sc[:, 0], v) and _same_bits(gr, g), w_lds
    finally:
        dbg.sigp_destroy(h)


# ---- 3. failing members leave their group mates alone ----------------------------------------------------------------------------------------------
def test_failing_members_get_inf_and_their_mate_keeps_its_bits(S):
    """the construction of tests/test_hip_loo_ard_batch.py: duplicate rows with sn~ = 0; an overflowing exp"""
    n, d, B = 200, 8, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20260900 + b)
    Xb[1, 1] = Xb[1, 0]                                      # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    theta = np.stack([np.concatenate([np.log(ard_scales(d, 20260910 + i)), [np.log(1e-2)]]) for i in range(B)])
    theta[1, d] = -np.inf                                    # sn~ = 0 on the singular data set
    theta[2, 3] = 800.0                                      # exp overflows
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for crit in CRITERIA:
            r = gp.hindcast_ard_batch(theta, lead=2, min_train=4, criterion=crit, group=3, predictions=True)
            alone = gp.hindcast_ard_batch(theta[:1], lead=2, min_train=4, criterion=crit, group=3, predictions=True)
            v0, g0 = gp.hindcast_ard_batch(theta, lead=2, min_train=4, criterion=crit, group=3, grad=None)
            for k in ("value", "nlpd", "sse"):
                assert np.all(np.isposinf(r[k][1:])), (crit, k, r[k])
                assert np.isfinite(r[k][0]) and _same_bits(r[k][0], alone[k][0]), (crit, k)
            assert np.all(np.isposinf(r["grad"][1:])) and np.all(np.isfinite(r["grad"][0])), r["grad"]
            assert np.all(np.isnan(r["mean"][1:])) and np.all(np.isnan(r["var"][1:]))
            assert _same_bits(r["grad"][0], alone["grad"][0]) and _same_bits(r["mean"][0], alone["mean"][0]) and _same_bits(r["var"][0], alone["var"][0])
            assert g0 is None and _same_bits(v0, r["value"])
        f, g = gp.hindcast_objective_batch(np.array([[np.log(3.0), np.log(1e-2)], [0.0, 0.0], [800.0, np.log(1e-2)]]), lead=2, min_train=4, group=3)
        assert np.isfinite(f[0]) and np.isfinite(f[1]) and np.isposinf(f[2]) and np.all(np.isposinf(g[2])) and np.all(np.isfinite(g[:2]))


# ---- 4. the C ABI: leading dimensions and refusals -------------------------------------------------------------------------------------------------
def _abi_problem():
    n, d, B, F = 129, 5, 2, 5
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20261000 + b)
    ells = np.stack([ard_scales(d, 20261010 + i) for i in range(F)])
    sn = np.array([SNS[i % 2] for i in range(F)])
    return n, d, B, F, Xb, yb, np.concatenate([np.log(ells), np.log(sn)[:, None]], axis=1)


def test_abi_leading_dimensions(S, L):
    n, d, B, F, Xb, yb, theta = _abi_problem()
    pad, SENT, lead, mt = 3, -12345.678, 5, 3

    def wide(A, fill):
        out = np.full((A.shape[0], A.shape[1] + pad), fill)
        out[:, :A.shape[1]] = A
        return out

    with S.GPR(kernel="matern52") as gp:
        lib, h, kid = gp._lib, gp._h, gp._kid
        gp.upload_batch(Xb, yb, None, group=3)
        gp.set_option("group", 3)
        for mode in (0, 1):
            for crit in (0, 1):
                sc, grad, mean, var = np.zeros((F, 2)), np.zeros((F, d + 1)), np.zeros((F, n)), np.zeros((F, n))
                assert lib.sigp_hindcast_grad_ard_batch(h, 1, F, kid, L.ptr(theta), d + 1, d + 1, lead, mt, mode, crit, L.ptr(mean), L.ptr(var), n, L.ptr(sc), L.ptr(grad),
                                                        d + 1) == L.OK
                t0 = mt + lead - 1
                assert np.all(np.isfinite(sc)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(mean[:, t0:])) and np.all(var[:, t0:] > 0)
                assert np.all(np.isnan(mean[:, :t0])) and np.all(np.isnan(var[:, :t0]))
                # wide rows: NaN in the gaps of theta, a sentinel in the gaps of the outputs
                thw = wide(theta, np.nan)
                scw, gradw, meanw, varw = np.zeros((F, 2)), np.full((F, d + 1 + pad), SENT), np.full((F, n + pad), SENT), np.full((F, n + pad), SENT)
                assert lib.sigp_hindcast_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, lead, mt, mode, crit, L.ptr(meanw), L.ptr(varw), n + pad, L.ptr(scw),
                                                        L.ptr(gradw), d + 1 + pad) == L.OK
                assert _same_bits(scw, sc) and _same_bits(gradw[:, :d + 1], grad) and np.all(gradw[:, d + 1:] == SENT)
                assert _same_bits(meanw[:, :n], mean) and _same_bits(varw[:, :n], var) and np.all(meanw[:, n:] == SENT) and np.all(varw[:, n:] == SENT)
                # no gradient, no predictions: the same scores, nothing else written
                gradw[:] = SENT
                sc0 = np.zeros((F, 2))
                assert lib.sigp_hindcast_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, lead, mt, mode, crit, None, None, 0, L.ptr(sc0), None, 0) == L.OK
                assert _same_bits(sc0, sc) and np.all(gradw == SENT)


def test_what_the_c_entry_refuses(S, L):
    n, d, B, F, Xb, yb, theta = _abi_problem()
    sc, grad, mean, var = np.zeros((F, 2)), np.zeros((F, d + 1)), np.zeros((F, n)), np.zeros((F, n))

    def call(gp, first=0, count=F, kid=None, th=theta, ntheta=d + 1, ldtheta=d + 1, lead=5, mt=3, mode=0, crit=0, mean_=None, var_=None, nstride=n, score=sc, grad_=grad,
             ldgrad=d + 1):
        return gp._lib.sigp_hindcast_grad_ard_batch(gp._h, first, count, gp._kid if kid is None else kid, L.ptr(th), ntheta, ldtheta, lead, mt, mode, crit, L.ptr(mean_),
                                                    L.ptr(var_), nstride, L.ptr(score), L.ptr(grad_), ldgrad)

    with S.GPR(kernel="rbf") as gp:
        assert call(gp) == L.BAD_ARG                                                        # before sigp_batch_upload
        with pytest.raises(RuntimeError):
            gp.hindcast_ard_batch(theta)
        gp.upload_batch(Xb, yb, None, group=3)
        assert call(gp, mean_=mean, var_=var) == L.OK
        good = [sc.copy(), grad.copy(), mean.copy(), var.copy()]
        assert call(gp, count=0) == L.BAD_ARG and call(gp, count=-1) == L.BAD_ARG and call(gp, first=-1) == L.BAD_ARG
        assert call(gp, ntheta=d) == L.BAD_ARG and call(gp, ntheta=d + 2, ldtheta=d + 2) == L.BAD_ARG
        assert call(gp, ldtheta=d) == L.BAD_ARG                                             # ldtheta < ntheta
        assert call(gp, ldgrad=d) == L.BAD_ARG                                              # ldgrad < d + 1 with a gradient asked for
        assert call(gp, grad_=None, ldgrad=0) == L.OK                                       # ... and of no concern without one
        assert call(gp, mode=2) == L.BAD_ARG and call(gp, mode=-1) == L.BAD_ARG
        assert call(gp, crit=2) == L.BAD_ARG and call(gp, crit=-1) == L.BAD_ARG
        assert call(gp, mean_=mean) == L.BAD_ARG and call(gp, var_=var) == L.BAD_ARG         # one of mean / var alone
        assert call(gp, mean_=mean, var_=var, nstride=n - 1) == L.BAD_ARG
        assert call(gp, kid=0) == L.BAD_ARG                                                 # the reference kernel
        assert call(gp, score=None) == L.BAD_ARG
        assert call(gp, lead=0) == L.BAD_ARG and call(gp, lead=129, mt=1) == L.BAD_ARG       # sigp_hindcast's checks
        assert call(gp, mt=0) == L.BAD_ARG
        assert call(gp, lead=128, mt=1) == L.OK                                             # one scored row
        assert call(gp, lead=128, mt=2) == L.BAD_ARG and call(gp, lead=1, mt=n) == L.BAD_ARG     # no scored row
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta[:, :d])
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta, lead=129)
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta, lead=1, min_train=n)
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta, criterion="cv_nlpd")
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta, sigma_f="profiled")
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta, grad="ref")
        assert call(gp, mean_=mean, var_=var) == L.OK                                        # the handle goes on: the same bits as before the refusals
        for a, b in zip(good, [sc, grad, mean, var]):
            assert _same_bits(a, b)
    with S.GPR(kernel="netdiffusion") as gp:
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta)
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        assert call(gp, kid=1) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.hindcast_ard_batch(theta)


# ---- 5. the lockstep optimiser ---------------------------------------------------------------------------------------------------------------------
def _years(B=2):
    """B small years (n = 60, d = 3) whose y bends along x_1 and x_2 and ignores x_3 (tests/test_hindcast_batch_host.py runs the same
    lockstep optimiser on the closed form of these years: there the irrelevant scale ends as the largest in both)"""
    n, d = 60, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        rng = np.random.default_rng(20264100 + b)
        Xb[b] = rng.standard_normal((n, d))
        yb[b] = np.sin(1.5 * Xb[b, :, 0]) + np.cos(1.2 * Xb[b, :, 1]) + 0.1 * rng.standard_normal(n)
    return Xb, yb, d, np.log([np.sqrt(3.0)] * d + [1e-2])


def test_optimize_hindcast_batch_lowers_every_start_and_finds_the_irrelevant_feature(S):
    Xb, yb, d, th0 = _years()
    B, lead, mt = len(Xb), 1, 8
    th2 = np.log([np.sqrt(3.0), 1e-2])
    starts = np.concatenate([np.tile(th0, (B, 1)), np.tile(np.log([1.0, 2.0, 1.5, 1e-1]), (B, 1))])      # two starts per data set
    with S.GPR(kernel="rbf") as gp:
        res = gp.optimize_hindcast_batch(Xb, yb, th0, lead=lead, min_train=mt, criterion="hindcast_nlpd", group=4)
        again = gp.hindcast_ard_batch(res["x"], lead=lead, min_train=mt, group=4)
        at_start = gp.hindcast_ard_batch(starts, lead=lead, min_train=mt, group=4, grad=None)[0]
        res2 = gp.optimize_hindcast_batch(Xb, yb, th2, lead=lead, min_train=mt, group=4)                 # log l repeated; hindcast_nlpd by default
        multi = gp.optimize_hindcast_batch(Xb, yb, starts, lead=lead, min_train=mt, group=4)
        iso = gp.optimize_hindcast_batch(Xb, yb, th2, lead=lead, min_train=mt, ard=False, group=4)
        iso_start = gp.hindcast_objective_batch(np.tile(th2, (B, 1)), lead=lead, min_train=mt, group=4)[0]
        # one common length scale: the sum rule against hindcast_ard_batch at equal scales
        th_eq = np.concatenate([np.repeat(iso["x"][:, :1], d, axis=1), iso["x"][:, 1:]], axis=1)
        va, ga = gp.hindcast_ard_batch(th_eq, lead=lead, min_train=mt, group=4)
        cv_like = gp.optimize_cv_batch(Xb, yb, th0, 5, group=4, maxiter=2)                              # the shapes to match
        with pytest.raises(ValueError, match="optimize_ard"):
            gp.optimize_batch(Xb, yb, th0, group=4, ard=True, criterion="hindcast_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_ard_batch(Xb, yb, th0, criterion="hindcast_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_cv_batch(Xb, yb, th0, 5, criterion="hindcast_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_hindcast_batch(Xb, yb, th0, criterion="cv_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_hindcast_batch(Xb, yb, th0[:3], group=4)
        with pytest.raises(ValueError):
            gp.optimize_hindcast_batch(Xb, yb, th0, lead=60)
    assert set(res) == set(cv_like)
    for k in cv_like:
        assert np.shape(res[k]) == np.shape(cv_like[k]), k
    assert res["x"].shape == (B, d + 1) and multi["x"].shape == (2 * B, d + 1) and res["fun"].shape == (B,) and res["jac"].shape == (B, d + 1)
    assert iso["x"].shape == (B, 2) and iso["jac"].shape == (B, 2)
    assert _same_bits(again[0], res["fun"]) and _same_bits(again[1], res["jac"])                        # fun and jac are hindcast_ard_batch's at x
    print("starts %s -> %s in %s steps (converged %s); x %s" % (at_start, multi["fun"], multi["nit"], multi["converged"], multi["x"]))
    assert np.all(multi["fun"] < at_start), (multi["fun"], at_start)                                   # every start descends
    assert np.all(iso["fun"] < iso_start), (iso["fun"], iso_start)
    assert np.all(res["x"][:, 2] > res["x"][:, 0]) and np.all(res["x"][:, 2] > res["x"][:, 1])          # the irrelevant feature's scale above the relevant ones'
    assert _same_bits(res2["x"], res["x"]) and _same_bits(res2["fun"], res["fun"])
    assert _same_bits(multi["x"][:B], res["x"]) and _same_bits(multi["fun"][:B], res["fun"])
    assert _same_bits(va, iso["fun"]) and _same_bits(np.array([[np.sum(gi[:-1]), gi[-1]] for gi in ga]), iso["jac"])
