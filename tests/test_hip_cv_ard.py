"""GPU tier of the per-feature (ARD) gradients of the leave-block-out scores: ``GPR.cv_ard``, ``GPR.cv_objective``, the 'cv_nlpd' /
'cv_sse' criteria of ``GPR.optimize_ard`` / ``GPR.optimize`` and the C entry point sigp_cv_grad_ard against the per-direction NumPy closed
form that tests/test_cv_ard_host.py pins to central differences.

Scale of every gradient error: S (test_cv_ard_host.cv_ard_closed_form: S_k = sum_ij |G_ij D_ij|).  The reference is computed by two routes
to K~^-1 (explicit inverse; Cholesky + U U^T, the device's own route); their difference / S -- the *spread* -- is the reference's own
error, and the device must stay within max(1e-8, 10 x spread): the convention of tests/test_hip_loo_ard.py.  A case counts only if its
spread is <= 1e-8; on these inputs it is <= 1e-13, so none is dropped (``_check`` asserts it)."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_cv_ard_host import cv_ard_closed_form, cv_ard_problem

pytestmark = pytest.mark.gpu

SN = 1e-2
KINDS = ("rbf", "matern52")
MODES = ("refit", "fixed")
CRITERIA = ("cv_nlpd", "cv_sse")


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


def _theta(ells, sn=SN):
    return np.concatenate([np.log(ells), [np.log(sn)]])


def _reference_of(kind, X, y, ells, block, gap, sn=SN):
    """{mode: (closed form by the explicit inverse, {criterion: spread [d + 1]}, closed form by the other route)}: computed once per problem"""
    out = {}
    for mode in MODES:
        a = cv_ard_closed_form(kind, X, y, ells, sn, block, gap, mode, "inv")
        b = cv_ard_closed_form(kind, X, y, ells, sn, block, gap, mode, "chol")
        out[mode] = (a, {c: np.abs(a[c[3:] + "_grad"] - b[c[3:] + "_grad"]) / a[c[3:] + "_S"] for c in CRITERIA}, b)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, n, d, block, gap):
    X, y, ells = cv_ard_problem(n, d)
    return (X, y, ells), _reference_of(kind, X, y, ells, block, gap)


def _check(tag, got, ref, S_, spread, factor=1.0):
    """device error / S <= factor max(1e-8, 10 spread) for every component; the case counts only if spread <= 1e-8"""
    err = np.abs(np.asarray(got) - ref) / S_
    print("%s: error / S max %.3g   spread max %.3g" % (tag, float(np.max(err)), float(np.max(spread))))
    assert np.all(S_ > 0), (tag, S_)
    assert np.all(spread <= 1e-8), (tag, spread)
    assert np.all(err <= factor * np.maximum(1e-8, 10.0 * spread)), (tag, err, spread)


# ---- 1. the gradient and the values against the closed form -----------------------------------------------------------------------------
# (n, d, block, gap): the minimum; clipped windows; windows across row 128; a full 128 window with clipped ends; w = 128 exactly with a
# ragged last fold; every B entry summed from up to 7 folds; block-diagonal B of full blocks; d past one pad of 64, and two;
# 1100 folds: two passes of the pair limit
SHAPES = [(2, 1, 1, 0), (37, 3, 5, 2), (129, 8, 16, 8), (130, 8, 64, 32), (300, 8, 100, 14), (300, 8, 1, 3), (300, 8, 128, 0), (200, 65, 7, 3),
          (200, 130, 7, 3)]
CASES = [(kind,) + sh for kind in KINDS for sh in SHAPES] + [("rbf", 1100, 8, 1, 2)]


@pytest.mark.parametrize("kind,n,d,block,gap", CASES)
def test_cv_ard_gradient_and_values_equal_the_closed_form(S, kind, n, d, block, gap):
    (X, y, ells), ref = _reference(kind, n, d, block, gap)
    theta = _theta(ells)
    tag = "%s n=%d d=%d block=%d gap=%d" % (kind, n, d, block, gap)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        for mode in MODES:
            a, spread, _ = ref[mode]
            for crit in CRITERIA:
                key = crit[3:]
                v, g = gp.cv_ard(theta, block, gap=gap, criterion=crit, sigma_f=mode)
                assert g.shape == (d + 1,)
                _check("%s %s %s" % (tag, mode, crit), g, a[key + "_grad"], a[key + "_S"], spread[crit])
                assert abs(float(v) - a[key]) <= 1e-8 * abs(a[key]), (tag, mode, crit, v, a[key])
        v0, g0 = gp.cv_ard(theta, block, gap=gap, grad=None)
    assert g0 is None and abs(float(v0) - ref["refit"][0]["nlpd"]) <= 1e-8 * abs(ref["refit"][0]["nlpd"])


# ---- 2. block = 1 without a gap is leave-one-out -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d", [("rbf", 129, 8), ("matern52", 300, 8)])
def test_cv_ard_with_block_one_equals_loo_ard(S, kind, n, d):
    """two device results meet: twice the bound"""
    (X, y, ells), ref = _reference(kind, n, d, 1, 0)
    th = _theta(ells)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        for mode in MODES:
            a, spread, _ = ref[mode]
            for crit in CRITERIA:
                key = crit[3:]
                v, g = gp.cv_ard(th, 1, criterion=crit, sigma_f=mode)
                v1, g1 = gp.loo_ard(th, criterion="loo_" + key, sigma_f=mode)
                assert abs(float(v) - float(v1)) <= 1e-10 * abs(float(v1))
                _check("%s n=%d d=%d %s %s (cv_ard(1) against loo_ard)" % (kind, n, d, mode, crit), g, g1, a[key + "_S"], spread[crit], factor=2.0)


# ---- 3. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,block,gap,slices", [("rbf", 5, 0, 0), ("matern52", 16, 8, 0), ("rbf", 16, 8, 3)])
def test_cv_ard_carries_the_bits_of_refit_and_cv(S, kind, block, gap, slices):
    n, d = 300, 8
    X, y, Xs = O.synthetic_problem(n, d, 20262300, m=3)
    Xn = O.synthetic_problem(4, d, 20262301, m=140)[2]
    th = _theta(ard_scales(d, 20262302))

    def state(gp):
        lo, cv = gp.loo("refit"), gp.cv(block, gap)
        return ([np.array([gp.sigma_f_, gp.nlml_, gp.sigma_n_, gp.sn_tilde_])] + list(gp.predict(Xs)) + list(gp.predict(Xn))
                + [lo["mean"], lo["var"], np.array([lo["nlpd"], lo["sse"]]), cv["mean"], cv["var"], np.array([cv["nlpd"], cv["sse"]])])

    with S.GPR(kernel=kind) as gp:
        gp.set_option("cv_slices", slices)
        gp.set_data(X, y, Xs=Xs)
        gp.refit(S.GPR._exp(th[:-1]), float(S.GPR._exp(th[-1:])[0]))
        before = {mode: gp.cv(block, gap, mode) for mode in MODES}           # a plain cv() before the feature's code path has run
        fit = state(gp)
        for mode in MODES:
            r = {c: gp.cv_ard(th, block, gap=gap, criterion=c, sigma_f=mode, predictions=True) for c in CRITERIA}
            used = int(gp._stat("cv_slices"))
            r2 = {c: gp.cv_ard(th, block, gap=gap, criterion=c, sigma_f=mode) for c in CRITERIA}
            after_grad = state(gp)
            v0, g0 = gp.cv_ard(th, block, gap=gap, criterion="cv_sse", sigma_f=mode, grad=None)
            assert g0 is None and gp._fitted and gp.ell_.shape == (d,) and np.allclose(gp.ell_, np.exp(th[:d]), rtol=1e-14, atol=0)
            after_value = state(gp)
            gp.refit(S.GPR._exp(th[:-1]), float(S.GPR._exp(th[-1:])[0]))
            plain = gp.cv(block, gap, mode)                                   # ... and after it
            assert int(gp._stat("cv_slices")) == used and (slices == 0 or used == slices)
            for k in ("mean", "var", "nlpd", "sse"):
                assert _same_bits(plain[k], before[mode][k]), (mode, k)
            for c in CRITERIA:
                assert set(r[c]) == {"value", "grad", "mean", "var", "nlpd", "sse"}
                assert _same_bits(r[c]["nlpd"], plain["nlpd"]) and _same_bits(r[c]["sse"], plain["sse"]), (mode, c)
                assert _same_bits(r[c]["mean"], plain["mean"]) and _same_bits(r[c]["var"], plain["var"]), (mode, c)
                assert _same_bits(r[c]["value"], plain[c[3:]]) and _same_bits(r2[c][0], plain[c[3:]]), (mode, c)
                assert _same_bits(r[c]["grad"], r2[c][1]), (mode, c)                   # two calls: identical bits
            assert _same_bits(v0, plain["sse"])
            for i, (a, b, c) in enumerate(zip(fit, after_grad, after_value)):
                assert _same_bits(a, b) and _same_bits(a, c), (mode, i)
        assert not _same_bits(r["cv_nlpd"]["grad"], r["cv_sse"]["grad"])


# ---- 4. what is refused, the non-SPD branch, overflow ---------------------------------------------------------------------------------------
def test_what_cv_ard_refuses(S, L):
    n, d = 60, 4
    X, y, Xs = O.synthetic_problem(n, d, 20262400, m=2)
    ells = ard_scales(d, 20262401)
    th = _theta(ells)
    g, sc, mu, var = np.zeros(d + 1), np.zeros(2), np.zeros(n), np.zeros(n)

    def call(gp, kid=1, theta=th, ntheta=d + 1, block=5, gap=0, mode=0, crit=0, mean=None, var_=None, score=sc, grad=g):
        return gp._lib.sigp_cv_grad_ard(gp._h, kid, L.ptr(theta), ntheta, block, gap, mode, crit, L.ptr(mean), L.ptr(var_), L.ptr(score), L.ptr(grad))

    with S.GPR(kernel="rbf") as gp:
        assert call(gp) == L.BAD_ARG                           # before set_train
        gp.fit(X, y, ells, SN, Xs=Xs)
        good = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs))
        assert call(gp, ntheta=d) == L.BAD_ARG and call(gp, ntheta=d + 2) == L.BAD_ARG
        assert call(gp, kid=0) == L.BAD_ARG                    # the reference kernel
        assert call(gp, mode=2) == L.BAD_ARG and call(gp, mode=-1) == L.BAD_ARG
        assert call(gp, crit=2) == L.BAD_ARG and call(gp, crit=-1) == L.BAD_ARG
        assert call(gp, mean=mu) == L.BAD_ARG and call(gp, var_=var) == L.BAD_ARG       # one of mean / var alone
        assert call(gp, score=None) == L.BAD_ARG
        assert call(gp, block=0) == L.BAD_ARG and call(gp, gap=-1) == L.BAD_ARG
        assert call(gp, block=129) == L.BAD_ARG and call(gp, block=5, gap=62) == L.BAD_ARG     # window > 128
        assert call(gp, block=60) == L.BAD_ARG and call(gp, block=20, gap=20) == L.BAD_ARG      # a fold that leaves no training row
        assert call(gp, mean=mu, var_=var) == L.OK and np.all(np.isfinite(g)) and np.all(var > 0)
        g[:] = 7.0
        assert call(gp, grad=None) == L.OK and np.all(g == 7.0) and np.all(np.isfinite(sc))     # grad = NULL: scores only
        for bad in (dict(criterion="loo_nlpd"), dict(sigma_f="both"), dict(grad="ref"), dict(gap=62)):
            with pytest.raises(ValueError):
                gp.cv_ard(th, 5, **bad)
        for bad in (129, 60, 0):
            with pytest.raises(ValueError):
                gp.cv_ard(th, bad)
            with pytest.raises(ValueError):
                gp.optimize_ard(th, criterion="cv_nlpd", block=bad)
            with pytest.raises(ValueError):
                gp.optimize(th[-2:], criterion="cv_nlpd", block=bad)
        with pytest.raises(ValueError):
            gp.cv_ard(th[:-1], 5)
        with pytest.raises(ValueError):
            gp.optimize(th, ard=True, criterion="cv_nlpd")     # stays refused: optimize_ard is the entry
        gp.refit(ells, SN)                                     # the handle is still usable
        again = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs))
        for a, b in zip(good, again):
            assert _same_bits(a, b)
    with S.GPR(kernel="netdiffusion") as gp:
        gp.fit(X, y, 0.05, SN)
        with pytest.raises(ValueError):
            gp.cv_ard(th, 5)
        with pytest.raises(ValueError):
            gp.cv_objective(th[-2:], 5)
        with pytest.raises(ValueError):
            gp.optimize_ard(th, criterion="cv_nlpd")
        with pytest.raises(ValueError):
            gp.optimize(th[-2:], criterion="cv_sse")
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, 2.0, SN)
        assert call(gp) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.cv_ard(th, 5)
        gp.refit(2.0, SN)
        assert np.isfinite(gp.nlml_)


def test_cv_ard_non_spd_and_overflow_give_inf(S, L):
    n, d = 40, 3
    X, y, _ = O.synthetic_problem(n, d, 20262500)
    X[1] = X[0]                                                # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    th = np.concatenate([np.log(ard_scales(d, 20262501)), [-np.inf]])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for crit in CRITERIA:
            v, g = gp.cv_ard(th, 5, gap=1, criterion=crit)
            assert np.isposinf(v) and g.shape == (d + 1,) and np.all(np.isposinf(g))
        r = gp.cv_ard(th, 5, predictions=True)
        assert np.isposinf(r["value"]) and np.isposinf(r["nlpd"]) and np.isposinf(r["sse"]) and np.all(np.isnan(r["mean"])) and np.all(np.isnan(r["var"]))
        v, g = gp.cv_ard(th, 5, grad=None)
        assert np.isposinf(v) and g is None
        over = np.array([800.0, 0.0, 0.0, np.log(SN)])         # exp overflows
        v, g = gp.cv_ard(over, 5)
        assert np.isposinf(v) and g.shape == (d + 1,) and np.all(np.isposinf(g))
        v2, g2 = gp.cv_objective(np.array([800.0, np.log(SN)]), 5)
        assert np.isposinf(v2) and g2.shape == (2,) and np.all(np.isposinf(g2))
        sc, gg, mu, var = np.zeros(2), np.zeros(d + 1), np.zeros(n), np.zeros(n)
        assert gp._lib.sigp_cv_grad_ard(gp._h, 1, L.ptr(over), d + 1, 5, 0, 0, 0, L.ptr(mu), L.ptr(var), L.ptr(sc), L.ptr(gg)) == L.NOT_SPD
        assert np.all(np.isposinf(sc)) and np.all(np.isposinf(gg)) and np.all(np.isnan(mu)) and np.all(np.isnan(var))
        th[-1] = np.log(SN)
        v, g = gp.cv_ard(th, 5, gap=1)                         # ... and the handle goes on
        assert np.isfinite(v) and np.all(np.isfinite(g))


# ---- 5. the profile entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,block,gap,passes", [(300, 5, 1, 1), (1100, 1, 2, 2)])
def test_cv_ard_profile_entries(S, n, block, gap, passes):
    """SIGP_KC_MLII: sigp_cv's entries (the triangular inversion, four per pass); the gradient adds two per pass (the fold adjoints, their
    assembly) and five more: U U^T, the n^2 passes, the banded product, the product M, the tile pass"""
    d = 8
    X, y, ells = cv_ard_problem(n, d)
    th = _theta(ells)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        gp.refit(ells, SN)
        gp.profile_reset()
        gp.cv(block, gap)
        c0 = gp.profile_get()["mlii"]["launches"]
        assert c0 == 1 + 4 * passes
        gp.profile_reset()
        gp.cv_ard(th, block, gap=gap, grad=None)
        assert gp.profile_get()["mlii"]["launches"] == c0
        gp.profile_reset()
        gp.cv_ard(th, block, gap=gap)
        assert gp.profile_get()["mlii"]["launches"] == c0 + 2 * passes + 5


# ---- 6. the optimisers ---------------------------------------------------------------------------------------------------------------------
def _relevance_problem():
    n, d = 200, 4
    rng = np.random.default_rng(20262600)
    X = rng.standard_normal((n, d))
    y = np.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)       # x_3 and x_4 do not enter
    bounds = [(-3.0, 5.0)] * d + [(-12.0, 3.0)]
    th0 = np.log([np.sqrt(d)] * d + [1e-2])
    return X, y, d, bounds, th0


def test_optimize_ard_by_the_leave_block_out_density(S):
    """L-BFGS-B with ftol = 0 goes on until the largest entry of the projected gradient it is GIVEN (the device's) is <= gtol = 1e-5, or until
    its line search finds no lower value any more (the rounding floor of the score, below that gradient); the closed form differs from the
    device's by at most 1e-8 S.  So at the end every component that is not at a bound has |closed-form gradient| <= 1e-5 + 1e-8 S_k, and a
    component at a bound pushes outwards."""
    X, y, d, bounds, th0 = _relevance_problem()
    block = 5
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        res = gp.optimize_ard(th0, criterion="cv_nlpd", block=block, method="L-BFGS-B", bounds=bounds, options=dict(ftol=0.0, gtol=1e-5, maxiter=500))
        assert gp._fitted and np.allclose(gp.ell_, np.exp(res.x[:d]), rtol=1e-14, atol=0) and np.isclose(gp.sn_tilde_, np.exp(res.x[d]), rtol=1e-14, atol=0)
        assert gp.cv(block)["nlpd"] == res.fun
    at = cv_ard_closed_form("rbf", X, y, np.exp(res.x[:d]), np.exp(res.x[d]), block, 0, "refit")
    start = cv_ard_closed_form("rbf", X, y, np.exp(th0[:d]), np.exp(th0[d]), block, 0, "refit")
    lo, hi = np.array(bounds).T
    at_lo, at_hi = res.x <= lo + 1e-12, res.x >= hi - 1e-12
    free = ~(at_lo | at_hi)
    gr, S_ = at["nlpd_grad"], at["nlpd_S"]
    print("CV-ARD: device %.9g at %s in %d evaluations (%s); closed form there %.9g, start %.9g; |grad| / S %s; free %s"
          % (res.fun, res.x, res.nfev, res.message, at["nlpd"], start["nlpd"], np.abs(gr) / S_, free))
    assert abs(at["nlpd"] - res.fun) <= 1e-8 * abs(at["nlpd"])
    assert at["nlpd"] < start["nlpd"]
    assert np.all(np.abs(gr[free]) <= 1e-5 + 1e-8 * S_[free]), (gr, S_, free)
    assert np.all(gr[at_lo] >= -1e-8 * S_[at_lo]) and np.all(gr[at_hi] <= 1e-8 * S_[at_hi])
    assert min(res.x[2], res.x[3]) > res.x[0] + 1.0           # the irrelevant features get far longer scales than the one y bends along


def test_optimize_by_the_leave_block_out_error_over_one_length_scale(S):
    """``optimize(criterion='cv_sse', block=5, gap=1)``: at the point it lands on, the two-parameter gradient (the sum of the components,
    and the noise's) equals the closed form's at equal scales -- the bound of the components, on sum_k S_k and S_noise."""
    X, y, d, _, _ = _relevance_problem()
    block, gap = 5, 1
    th0 = np.log([2.0, 1e-2])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        start = float(gp.cv_objective(th0, block, gap=gap, criterion="cv_sse")[0])
        res = gp.optimize(th0, criterion="cv_sse", block=block, gap=gap, method="L-BFGS-B", bounds=[(-3.0, 5.0), (-12.0, 3.0)])
        assert np.all(np.isfinite(res.x)) and np.isfinite(res.fun) and res.fun < start
        assert gp._fitted and np.isclose(gp.ell_, np.exp(res.x[0]), rtol=1e-14, atol=0)
        v, g2 = gp.cv_objective(res.x, block, gap=gap, criterion="cv_sse")
        vn, gn = gp.cv_objective(res.x, block, gap=gap, criterion="cv_nlpd", sigma_f="fixed")
    assert float(v) == res.fun and g2.shape == (2,)
    ells = np.full(d, np.exp(res.x[0]))
    a = cv_ard_closed_form("rbf", X, y, ells, np.exp(res.x[1]), block, gap, "refit", "inv")
    b = cv_ard_closed_form("rbf", X, y, ells, np.exp(res.x[1]), block, gap, "refit", "chol")
    af = cv_ard_closed_form("rbf", X, y, ells, np.exp(res.x[1]), block, gap, "fixed", "inv")
    bf = cv_ard_closed_form("rbf", X, y, ells, np.exp(res.x[1]), block, gap, "fixed", "chol")
    for tag, got, p, q_, key in (("cv_sse refit", g2, a, b, "sse"), ("cv_nlpd fixed", gn, af, bf, "nlpd")):
        two = lambda r: np.array([np.sum(r[key + "_grad"][:d]), r[key + "_grad"][d]])
        S2 = np.array([np.sum(p[key + "_S"][:d]), p[key + "_S"][d]])
        _check("optimize landing point, %s" % tag, got, two(p), S2, np.abs(two(p) - two(q_)) / S2)
    assert abs(float(v) - a["sse"]) <= 1e-8 * abs(a["sse"]) and abs(float(vn) - af["nlpd"]) <= 1e-8 * abs(af["nlpd"])
