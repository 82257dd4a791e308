"""GPU tier of the per-feature (ARD) gradients of the leave-one-out scores: ``GPR.loo_ard``, ``GPR.optimize_ard`` and the C entry point
sigp_loo_grad_ard against the per-point NumPy closed form that tests/test_loo_ard_host.py pins to central differences.

Scale of every gradient error: S (test_loo_ard_host.loo_ard_closed_form: S_k = sum_ij |G_ij h_ij (u_ik - u_jk)^2| for a feature, sn~
sum_i |G_ii| for the noise).  The reference is computed by two routes to K~^-1 (explicit inverse; Cholesky + U U^T, the device's own
route); their difference / S -- the *spread* -- is the reference's own error, and the device must stay within max(1e-8, 10 x spread), the
convention of tests/test_hip_ard.py and tests/test_hip_loo_grad.py."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_hip_covariance_inputs import dyadic, offsets
from test_loo_ard_host import loo_ard_closed_form

pytestmark = pytest.mark.gpu

SN = 1e-2
KINDS = ("rbf", "matern52")
MODES = ("refit", "fixed")
CRITERIA = ("loo_nlpd", "loo_sse")


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


def _reference_of(kind, X, y, ells, sn=SN):
    """{mode: (closed form by the explicit inverse, {criterion: spread [d + 1]}, closed form by the other route)}: computed once per problem"""
    out = {}
    for mode in MODES:
        a, b = loo_ard_closed_form(kind, X, y, ells, sn, mode, "inv"), loo_ard_closed_form(kind, X, y, ells, sn, mode, "chol")
        out[mode] = (a, {c: np.abs(a[c[4:] + "_grad"] - b[c[4:] + "_grad"]) / a[c[4:] + "_S"] for c in CRITERIA}, b)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, n, d):
    X, y, _ = O.synthetic_problem(n, d, 20251700 + 7 * n + d)
    ells = ard_scales(d, 20251800 + 7 * n + d)
    return (X, y, ells), _reference_of(kind, X, y, ells)


def _check(tag, got, ref, S_, spread, factor=1.0):
    """device error / S <= factor max(1e-8, 10 spread) for every component; the case counts only if spread <= 1e-8"""
    err = np.abs(np.asarray(got) - ref) / S_
    print("%s: error / S max %.3g   spread max %.3g" % (tag, float(np.max(err)), float(np.max(spread))))
    assert np.all(S_ > 0), (tag, S_)
    assert np.all(spread <= 1e-8), (tag, spread)
    assert np.all(err <= factor * np.maximum(1e-8, 10.0 * spread)), (tag, err, spread)


def _check_all(tag, gp, theta, ref):
    """every (sigma mode, criterion) of one problem on one handle"""
    d = len(theta) - 1
    for mode in MODES:
        a, spread, _ = ref[mode]
        for crit in CRITERIA:
            key = crit[4:]
            v, g = gp.loo_ard(theta, criterion=crit, sigma_f=mode)
            assert g.shape == (d + 1,)
            _check("%s %s %s" % (tag, mode, crit), g, a[key + "_grad"], a[key + "_S"], spread[crit])
            assert abs(float(v) - a[key]) <= 1e-8 * abs(a[key]), (tag, mode, crit, v, a[key])


# ---- 1. the gradient against the closed form -------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (37, 3), (128, 8), (129, 8), (300, 8), (200, 65), (200, 130)]
CASES = [(kind, n, d) for kind in KINDS for (n, d) in SHAPES] + [("rbf", 1000, 8)]


@pytest.mark.parametrize("kind,n,d", CASES)
def test_loo_ard_gradient_equals_the_closed_form(S, kind, n, d):
    (X, y, ells), ref = _reference(kind, n, d)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        _check_all("%s n=%d d=%d" % (kind, n, d), gp, _theta(ells), ref)
        v0, g0 = gp.loo_ard(_theta(ells), grad=None)
    assert g0 is None and abs(float(v0) - ref["refit"][0]["nlpd"]) <= 1e-8 * abs(ref["refit"][0]["nlpd"])


# ---- 2. the two device routes agree --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d", [("rbf", 129, 8), ("matern52", 300, 8), ("rbf", 200, 65)])
def test_loo_ard_components_add_up_to_the_per_point_route(S, kind, n, d):
    """``loo(grad=True)`` on the fit ``loo_ard`` left differentiates with respect to the common multiplier of the scales: d/dlog ell =
    sum_k d/dlog l_k, and d/dlog sn~ is the same number.  Two device results meet: twice the bound, on sum_k S_k and on S_noise."""
    (X, y, ells), ref = _reference(kind, n, d)
    th = _theta(ells)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        for mode in MODES:
            a, spread, b = ref[mode]
            for crit in CRITERIA:
                key = crit[4:]
                v, g = gp.loo_ard(th, criterion=crit, sigma_f=mode)
                old = gp.loo(mode, grad=True)
                assert old[key] == float(v)
                got = np.array([np.sum(g[:d]), g[d]])
                S2 = np.array([np.sum(a[key + "_S"][:d]), a[key + "_S"][d]])
                sp2 = np.array([abs(np.sum(a[key + "_grad"][:d]) - np.sum(b[key + "_grad"][:d])) / S2[0], spread[crit][d]])   # the reference's own error on the sum
                _check("%s n=%d d=%d %s %s (two routes)" % (kind, n, d, mode, crit), got, old[key + "_grad"], S2, sp2, factor=2.0)


# ---- 3. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_loo_ard_carries_the_bits_of_refit_and_loo(S, kind):
    n, d = 300, 8
    X, y, Xs = O.synthetic_problem(n, d, 20252300, m=3)
    Xn = O.synthetic_problem(4, d, 20252301, m=140)[2]
    th = _theta(ard_scales(d, 20252302))
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y, Xs=Xs)
        n0 = gp.nlml_ard(th)
        for mode in MODES:
            r = {c: gp.loo_ard(th, criterion=c, sigma_f=mode, predictions=True) for c in CRITERIA}
            r2 = {c: gp.loo_ard(th, criterion=c, sigma_f=mode) for c in CRITERIA}
            v0, g0 = gp.loo_ard(th, criterion="loo_sse", sigma_f=mode, grad=None)
            assert gp._fitted and gp.ell_.shape == (d,) and np.allclose(gp.ell_, np.exp(th[:d]), rtol=1e-14, atol=0)
            state = [np.array([gp.sigma_f_, gp.nlml_, gp.sigma_n_, gp.sn_tilde_])] + list(gp.predict(Xs)) + list(gp.predict(Xn))
            gp.refit(S.GPR._exp(th[:-1]), float(S.GPR._exp(th[-1:])[0]))
            plain = gp.loo(mode)
            fit = [np.array([gp.sigma_f_, gp.nlml_, gp.sigma_n_, gp.sn_tilde_])] + list(gp.predict(Xs)) + list(gp.predict(Xn))
            for c in CRITERIA:
                assert set(r[c]) == {"value", "grad", "mean", "var", "nlpd", "sse"}
                assert _same_bits(r[c]["nlpd"], plain["nlpd"]) and _same_bits(r[c]["sse"], plain["sse"]), (mode, c)
                assert _same_bits(r[c]["mean"], plain["mean"]) and _same_bits(r[c]["var"], plain["var"]), (mode, c)
                assert _same_bits(r[c]["value"], plain[c[4:]]) and _same_bits(r2[c][0], plain[c[4:]]), (mode, c)
                assert _same_bits(r[c]["grad"], r2[c][1]), (mode, c)                   # two calls: identical bits
            assert g0 is None and _same_bits(v0, plain["sse"])
            for i, (a, b) in enumerate(zip(state, fit)):
                assert _same_bits(a, b), (mode, i)
        assert not _same_bits(r["loo_nlpd"]["grad"], r["loo_sse"]["grad"])
        n1 = gp.nlml_ard(th)                                   # its instantiation of the tile pass is untouched
        assert _same_bits(n0[0], n1[0]) and _same_bits(n0[1], n1[1])


# ---- 4. uncentred features -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_loo_ard_gradient_with_offset_features(S, kind):
    """Dyadic inputs, integer offsets and power-of-two scales: (X + o) / l is exact, so the reference computed WITHOUT the offset is the
    reference of every offset, and the device must meet the same bound there."""
    n, d = 200, 8
    rng = np.random.default_rng(20251600)
    X = dyadic(rng, (n, d))
    y = np.sin(X @ (rng.standard_normal(d) / np.sqrt(d))) + 0.1 * rng.standard_normal(n)
    ells = 2.0 ** rng.integers(0, 3, d)
    ref = _reference_of(kind, X, y, ells)
    for off in ("zero", "mixed", "1e4"):
        o = offsets(off, d)
        assert np.array_equal((X + o) - o, X)
        with S.GPR(kernel=kind) as gp:
            gp.set_data(X + o, y)
            _check_all("%s offset %s" % (kind, off), gp, _theta(ells), ref)


# ---- 5. what is refused, and the non-SPD branch -------------------------------------------------------------------------------------------
def test_what_loo_ard_refuses(S, L):
    n, d = 60, 4
    X, y, Xs = O.synthetic_problem(n, d, 20252400, m=2)
    ells = ard_scales(d, 20252401)
    th = _theta(ells)
    g, sc, mu, var = np.zeros(d + 1), np.zeros(2), np.zeros(n), np.zeros(n)

    def call(gp, kid=1, theta=th, ntheta=d + 1, mode=0, crit=0, mean=None, var_=None, score=sc, grad=g):
        return gp._lib.sigp_loo_grad_ard(gp._h, kid, L.ptr(theta), ntheta, mode, crit, L.ptr(mean), L.ptr(var_), L.ptr(score), L.ptr(grad))

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
        assert call(gp, mean=mu, var_=var) == L.OK and np.all(np.isfinite(g)) and np.all(var > 0)
        g[:] = 7.0
        assert call(gp, grad=None) == L.OK and np.all(g == 7.0) and np.all(np.isfinite(sc))     # grad = NULL: scores only
        for bad in (dict(criterion="nlml"), dict(sigma_f="both"), dict(grad="ref")):
            with pytest.raises(ValueError):
                gp.loo_ard(th, **bad)
        with pytest.raises(ValueError):
            gp.loo_ard(th[:-1])
        with pytest.raises(ValueError):
            gp.optimize_ard(th, criterion="loo")
        with pytest.raises(ValueError):
            gp.optimize_ard(th[:3])
        with pytest.raises(ValueError):
            gp.optimize(th, ard=True, criterion="loo_nlpd")    # stays refused: optimize_ard is the entry
        gp.refit(ells, SN)                                     # the handle is still usable
        again = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs))
        for a, b in zip(good, again):
            assert _same_bits(a, b)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X[:1], y[:1])
        assert call(gp) == L.BAD_ARG                           # n < 2: no leave-one-out
    with S.GPR(kernel="netdiffusion") as gp:
        gp.fit(X, y, 0.05, SN)
        with pytest.raises(ValueError):
            gp.loo_ard(th)
        with pytest.raises(ValueError):
            gp.optimize_ard(th, criterion="loo_nlpd")
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, 2.0, SN)
        assert call(gp) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.loo_ard(th)
        gp.refit(2.0, SN)
        assert np.isfinite(gp.nlml_)


def test_loo_ard_non_spd_gives_inf(S, L):
    n, d = 40, 3
    X, y, _ = O.synthetic_problem(n, d, 20252500)
    X[1] = X[0]                                                # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    th = np.concatenate([np.log(ard_scales(d, 20252501)), [-np.inf]])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for crit in CRITERIA:
            v, g = gp.loo_ard(th, criterion=crit)
            assert np.isposinf(v) and g.shape == (d + 1,) and np.all(np.isposinf(g))
        r = gp.loo_ard(th, predictions=True)
        assert np.isposinf(r["value"]) and np.isposinf(r["nlpd"]) and np.isposinf(r["sse"]) and np.all(np.isnan(r["mean"])) and np.all(np.isnan(r["var"]))
        v, g = gp.loo_ard(th, grad=None)
        assert np.isposinf(v) and g is None
        over = np.array([800.0, 0.0, 0.0, np.log(SN)])         # exp overflows
        v, g = gp.loo_ard(over)
        assert np.isposinf(v) and np.all(np.isposinf(g))
        sc, gg, mu, var = np.zeros(2), np.zeros(d + 1), np.zeros(n), np.zeros(n)
        assert gp._lib.sigp_loo_grad_ard(gp._h, 1, L.ptr(over), d + 1, 0, 0, L.ptr(mu), L.ptr(var), L.ptr(sc), L.ptr(gg)) == L.NOT_SPD
        assert np.all(np.isposinf(sc)) and np.all(np.isposinf(gg)) and np.all(np.isnan(mu)) and np.all(np.isnan(var))
        th[-1] = np.log(SN)
        v, g = gp.loo_ard(th)                                  # ... and the handle goes on
        assert np.isfinite(v) and np.all(np.isfinite(g))


# ---- 6. the optimiser ----------------------------------------------------------------------------------------------------------------------
def _relevance_problem():
    """the data set of test_hip_ard.test_optimize_ard_finds_the_irrelevant_feature"""
    n, d = 96, 3
    rng = np.random.default_rng(20251900)
    X = rng.standard_normal((n, d))
    y = np.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)       # x_3 does not enter
    bounds = [(-3.0, 5.0)] * d + [(-12.0, 3.0)]
    th0 = np.log([np.sqrt(3.0)] * d + [1e-2])
    return X, y, d, bounds, th0


def test_optimize_ard_by_the_leave_one_out_density_finds_the_irrelevant_feature(S):
    X, y, d, bounds, th0 = _relevance_problem()

    def f(th):
        try:
            r = loo_ard_closed_form("rbf", X, y, np.exp(th[:d]), np.exp(th[d]), "refit")
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        return r["nlpd"], r["nlpd_grad"]

    ref = minimize(f, th0, jac=True, method="L-BFGS-B", bounds=bounds)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        res = gp.optimize_ard(th0, criterion="loo_nlpd", sigma_f="refit", method="L-BFGS-B", bounds=bounds)
        assert gp._fitted and np.allclose(gp.ell_, np.exp(res.x[:d]), rtol=1e-14, atol=0) and np.isclose(gp.sn_tilde_, np.exp(res.x[d]), rtol=1e-14, atol=0)
        assert gp.loo("refit")["nlpd"] == res.fun
    at, start = f(res.x)[0], f(th0)[0]
    print("LOO-ARD: reference %.9g at %s in %d evaluations; device %.9g at %s in %d (closed form there: %.9g); start %.9g"
          % (ref.fun, ref.x, ref.nfev, res.fun, res.x, res.nfev, at, start))
    assert at <= ref.fun + 1e-6 * abs(ref.fun)
    assert at < start
    assert res.x[2] > res.x[0] + 1.0                           # the irrelevant feature gets a far longer scale than the one y bends along


def test_optimize_ard_other_criteria(S):
    """loo_sse: its valley on this data is flat and the optimum is not stable under 1e-9 of gradient noise, so only finiteness and descent
    are asserted.  nlml: the same iterates as ``optimize(ard=True)``."""
    X, y, d, bounds, th0 = _relevance_problem()
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        start = float(gp.loo_ard(th0, criterion="loo_sse", grad=None)[0])
        res = gp.optimize_ard(th0, criterion="loo_sse", method="L-BFGS-B", bounds=bounds)
        assert np.all(np.isfinite(res.x)) and np.isfinite(res.fun) and res.fun < start
        assert gp._fitted and gp.loo("refit")["sse"] == res.fun
        a = gp.optimize_ard(th0, criterion="nlml", method="L-BFGS-B", bounds=bounds)
        b = gp.optimize(th0, ard=True, method="L-BFGS-B", bounds=bounds)
        c = gp.optimize_ard(np.log([np.sqrt(3.0), 1e-2]), method="L-BFGS-B", bounds=bounds)       # log l broadcast, criterion 'nlml' by default
    assert np.array_equal(a.x, b.x) and a.fun == b.fun and np.array_equal(c.x, a.x)


# ---- 7. the profile entries of the calls ------------------------------------------------------------------------------------------------
# (launches, flops, bytes) of SIGP_KC_MLII at n = 300 (three 128-tiles, padded rows in the last), d = 8, RBF: what the library books for
# the triangular inversion, U U^T, the n^2 passes, the product M and the tile pass.  The figures are sums of products of small integers,
# all exactly representable in a double, read off the library before the host drivers of these entry points were single-sourced.
MLII_PINS = {
    "nlml_ard": (3, 48368736.0, 513600.0),                    # triangular inversion, U U^T, the tile pass
    "loo_ard_value_only": (2, 19054368.0, 360000.0),          # loo's own two entries
    "loo_ard": (6, 125176032.0, 6182016.0),                   # ... + U U^T, the n^2 passes, the product M, the tile pass
}


def test_nlml_ard_and_loo_ard_profile_entries(S):
    n, d = 300, 8
    X, y, _ = O.synthetic_problem(n, d, 20252300)
    th = _theta(ard_scales(d, 20252302))
    calls = {"nlml_ard": lambda gp: gp.nlml_ard(th), "loo_ard_value_only": lambda gp: gp.loo_ard(th, grad=None), "loo_ard": lambda gp: gp.loo_ard(th)}
    got = {}
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for name, fn in calls.items():
            gp.profile_reset()
            fn(gp)
            p = gp.profile_get()["mlii"]
            got[name] = (p["launches"], p["flops"], p["bytes"])
            print("%s: %r" % (name, got[name]))
    assert got == MLII_PINS, got
