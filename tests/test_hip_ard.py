"""GPU tier of the per-feature (ARD) length scales: ``GPR.fit(ell=<sequence>)``, ``GPR.nlml_ard``, ``GPR.optimize(ard=True)`` and the two C
entry points (sigp_set_length_scales, sigp_nlml_grad_ard) against the NumPy closed form that tests/test_ard_host.py pins to central
differences.

Scale of every gradient error: S (test_ard_host.ard_closed_form: the component's sum with |.| inside).  The reference is computed by two
routes to K~^-1 (explicit inverse; Cholesky + U U^T, the device's own route); their difference / S -- the *spread* -- is the reference's own
error, and the device must stay within max(1e-8, 10 x spread), the convention of tests/test_hip_loo_grad.py.  A component whose S is exactly
0 (one training point: no pair of points) must be exactly 0 on the device."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_ard_host import ard_closed_form, ard_scales, oracle_value
from test_hip_covariance_inputs import dyadic, offsets

pytestmark = pytest.mark.gpu

SN = 1e-2
KINDS = ("rbf", "matern52")


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
    """(gradient by the explicit inverse, S, spread [d + 1], value): computed once per problem"""
    a, S_, val = ard_closed_form(kind, X, y, ells, sn, "inv")
    b, _, _ = ard_closed_form(kind, X, y, ells, sn, "chol")
    with np.errstate(invalid="ignore", divide="ignore"):
        spread = np.where(S_ > 0, np.abs(a - b) / S_, 0.0)
    return a, S_, spread, val


@functools.lru_cache(maxsize=None)
def _reference(kind, n, d):
    X, y, _ = O.synthetic_problem(n, d, 20251400 + 7 * n + d)
    ells = ard_scales(d, 20251500 + 7 * n + d)
    return (X, y, ells), _reference_of(kind, X, y, ells)


def _check(tag, got, ref, S_, spread):
    """device error / S <= max(1e-8, 10 spread) for every component; the case counts only if spread <= 1e-8"""
    got = np.asarray(got)
    pos = S_ > 0
    err = np.abs(got[pos] - ref[pos]) / S_[pos]
    print("%s: error / S max %.3g   spread max %.3g" % (tag, float(np.max(err)) if err.size else 0.0, float(np.max(spread))))
    assert np.all(spread <= 1e-8), (tag, spread)
    assert np.all(got[~pos] == 0.0), (tag, got[~pos])
    assert np.all(err <= np.maximum(1e-8, 10.0 * spread[pos])), (tag, err, spread)


# ---- 1. the gradient against the closed form -------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 1), (37, 3), (128, 8), (129, 8), (300, 8), (200, 65), (200, 130)]
CASES = [(kind, n, d) for kind in KINDS for (n, d) in SHAPES] + [("rbf", 1000, 8)]


@pytest.mark.parametrize("kind,n,d", CASES)
def test_ard_gradient_equals_the_closed_form(S, kind, n, d):
    (X, y, ells), (ref, S_, spread, val) = _reference(kind, n, d)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        v, g = gp.nlml_ard(_theta(ells))
        v0, g0 = gp.nlml_ard(_theta(ells), grad=None)
    assert g.shape == (d + 1,) and g0 is None and v0 == v
    if n == 1:
        # One point: no pair, the length scale does not enter (exactly 0).  The noise component vanishes identically too -- K~ = 1 + sn~,
        # P = 1 / K~, a = P y, sf = y a, so P / 2 - a^2 / (2 sf) = P / 2 - P / 2 -- and its S is the rounding residue of that difference
        # (~1e-19, different by each route: spread 1), no scale.  The bound is the rounding itself: a few ulps of the two halves sn~ P / 2.
        assert g[0] == 0.0 and S_[0] == 0.0
        assert abs(g[1]) <= 16 * np.finfo(np.float64).eps * SN / (1.0 + SN), g
        assert abs(ref[1]) <= 16 * np.finfo(np.float64).eps * SN / (1.0 + SN), ref
    else:
        _check("%s n=%d d=%d" % (kind, n, d), g, ref, S_, spread)
    want = oracle_value(kind, X, y, ells, SN)
    assert abs(float(v) - want) <= 1e-8 * abs(want), (v, want)
    assert abs(val - want) <= 1e-8 * abs(want)


# ---- 2. uncentred features -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_ard_gradient_with_offset_features(S, kind):
    """Dyadic inputs, integer offsets and power-of-two scales: (X + o) / l is exact, so the reference computed WITHOUT the offset is the
    reference of every offset, and the device must meet the same bound there."""
    n, d = 200, 8
    rng = np.random.default_rng(20251600)
    X = dyadic(rng, (n, d))
    y = np.sin(X @ (rng.standard_normal(d) / np.sqrt(d))) + 0.1 * rng.standard_normal(n)
    ells = 2.0 ** rng.integers(0, 3, d)
    ref, S_, spread, val = _reference_of(kind, X, y, ells)
    for off in ("zero", "mixed", "1e4"):
        o = offsets(off, d)
        assert np.array_equal((X + o) - o, X)
        with S.GPR(kernel=kind) as gp:
            gp.set_data(X + o, y)
            v, g = gp.nlml_ard(_theta(ells))
        _check("%s offset %s" % (kind, off), g, ref, S_, spread)
        assert abs(float(v) - val) <= 1e-8 * abs(val), (off, v, val)


# ---- 3. the scaling is exactly a division ---------------------------------------------------------------------------------------------------
def _everything(gp, Xs, Xs_many, Xs_cov):
    out = [np.array([gp.sigma_f_, gp.nlml_, gp.sigma_n_])]
    out += list(gp.predict(Xs)) + list(gp.predict(Xs_many)) + list(gp.predict_cov(Xs_cov))
    lo, cv = gp.loo(), gp.cv(block=5, gap=1)
    out += [lo["mean"], lo["var"], np.array([lo["nlpd"], lo["sse"]]), cv["mean"], cv["var"], np.array([cv["nlpd"], cv["sse"]])]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_ard_fit_equals_a_fit_on_divided_features_bit_for_bit(S, kind):
    n, d = 129, 8
    X, y, Xs = O.synthetic_problem(n, d, 20251700, m=5)
    Xs_many = O.synthetic_problem(4, d, 20251701, m=200)[2]
    Xs_cov = Xs_many[:150]
    l1, l2 = ard_scales(d, 20251702), ard_scales(d, 20251703)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, l1, SN, Xs=Xs)
        assert np.array_equal(gp.ell_, l1)
        ard1 = _everything(gp, Xs, Xs_many, Xs_cov)
        gp.refit(l2, SN)                                   # new scales, no new set_data
        ard2 = _everything(gp, Xs, Xs_many, Xs_cov)
        gp.refit(np.sqrt(d), SN)                           # a scalar afterwards: isotropic again
        assert gp.ell_ == float(np.sqrt(d))
        iso_after = _everything(gp, Xs, Xs_many, Xs_cov)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X / l1, y, 1.0, SN, Xs=Xs / l1)
        pre1 = _everything(gp, Xs / l1, Xs_many / l1, Xs_cov / l1)
        gp.fit(X / l2, y, 1.0, SN, Xs=Xs / l2)
        pre2 = _everything(gp, Xs / l2, Xs_many / l2, Xs_cov / l2)
    with S.GPR(kernel=kind) as gp:                         # a handle that never saw per-feature scales
        gp.fit(X, y, np.sqrt(d), SN, Xs=Xs)
        iso = _everything(gp, Xs, Xs_many, Xs_cov)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, l2, SN, Xs=Xs)
        fresh2 = _everything(gp, Xs, Xs_many, Xs_cov)
    for i, (a, b) in enumerate(zip(ard1, pre1)):
        assert _same_bits(a, b), ("scales 1 against pre-divided features", i)
    for i, (a, b, c) in enumerate(zip(ard2, pre2, fresh2)):
        assert _same_bits(a, b) and _same_bits(a, c), ("scales 2 (refit) against pre-divided features / a fresh fit", i)
    for i, (a, b) in enumerate(zip(iso_after, iso)):
        assert _same_bits(a, b), ("scalar ell after ARD", i)
    assert not _same_bits(ard1[0], ard2[0]) and not _same_bits(ard1[0], iso[0])


# ---- 4. determinism and state ----------------------------------------------------------------------------------------------------------------
def test_nlml_ard_is_deterministic_and_leaves_the_fit(S):
    n, d = 300, 8
    X, y, Xs = O.synthetic_problem(n, d, 20251800, m=3)
    Xn = O.synthetic_problem(4, d, 20251801, m=140)[2]
    ells = ard_scales(d, 20251802)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y, Xs=Xs)
        v1, g1 = gp.nlml_ard(_theta(ells))
        v2, g2 = gp.nlml_ard(_theta(ells))
        assert _same_bits(v1, v2) and _same_bits(g1, g2)
        assert gp._fitted and gp.ell_.shape == (d,) and np.allclose(gp.ell_, ells, rtol=1e-14, atol=0) and gp.nlml_ == float(v1)
        after = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs)) + list(gp.predict(Xn)) + [gp.loo()["var"]]
        gp.fit(X, y, gp.ell_.copy(), gp.sn_tilde_, Xs=Xs)      # ell_ / sn_tilde_: the library's own exp(theta)
        assert _same_bits(gp.nlml_, v1)                    # the value is the fit's, bit for bit
        fit = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs)) + list(gp.predict(Xn)) + [gp.loo()["var"]]
    for i, (a, b) in enumerate(zip(after, fit)):
        assert _same_bits(a, b), i


# ---- 5. the optimiser finds relevance ---------------------------------------------------------------------------------------------------------
def test_optimize_ard_finds_the_irrelevant_feature(S):
    n, d = 96, 3
    rng = np.random.default_rng(20251900)
    X = rng.standard_normal((n, d))
    y = np.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)       # x_3 does not enter
    bounds = [(-3.0, 5.0)] * d + [(-12.0, 3.0)]
    th0 = np.log([np.sqrt(3.0)] * d + [1e-2])

    def f(th):
        try:
            g, _, v = ard_closed_form("rbf", X, y, np.exp(th[:d]), np.exp(th[d]))
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        return float(v), g

    ref = minimize(f, th0, jac=True, method="L-BFGS-B", bounds=bounds)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        res = gp.optimize(th0, ard=True, method="L-BFGS-B", bounds=bounds)
        assert gp._fitted and np.allclose(gp.ell_, np.exp(res.x[:d]), rtol=1e-14, atol=0) and gp.nlml_ == res.fun
        res2 = gp.optimize(np.log([np.sqrt(3.0), 1e-2]), ard=True, method="L-BFGS-B", bounds=bounds)      # log l broadcast
        iso = gp.optimize(np.log([np.sqrt(3.0), 1e-2]), method="L-BFGS-B", bounds=[bounds[0], bounds[-1]])
        with pytest.raises(ValueError):
            gp.optimize(th0, ard=True, criterion="loo_nlpd")
        with pytest.raises(ValueError):
            gp.optimize(th0[:3], ard=True)
    at = f(res.x)[0]
    print("ARD: reference %.9g at %s in %d evaluations; device %.9g at %s in %d (closed form there: %.9g); isotropic %.9g"
          % (ref.fun, ref.x, ref.nfev, res.fun, res.x, res.nfev, at, iso.fun))
    assert at <= ref.fun + 1e-6 * abs(ref.fun)
    assert res.fun < iso.fun
    assert np.array_equal(res2.x, res.x)
    assert res.x[2] > res.x[0] + 1.0                           # the irrelevant feature gets a far longer scale than the one y bends along


# ---- 6. what is refused ----------------------------------------------------------------------------------------------------------------------
def test_what_per_feature_scales_refuse(S, L):
    n, d = 60, 4
    X, y, Xs = O.synthetic_problem(n, d, 20252000, m=2)
    ells = ard_scales(d, 20252001)
    val, g, out = C.c_double(), np.zeros(d + 1), np.zeros(4)
    th = _theta(ells)
    with S.GPR(kernel="rbf") as gp:
        lib, h = gp._lib, gp._h
        assert lib.sigp_nlml_grad_ard(h, 1, L.ptr(th), d + 1, 2, C.byref(val), L.ptr(g)) == L.BAD_ARG          # before set_train
        assert lib.sigp_set_length_scales(h, L.ptr(ells), d) == L.BAD_ARG
        gp.fit(X, y, ells, SN, Xs=Xs)
        good = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs))
        for bad in (ells[:3], np.append(ells, 1.0)):
            with pytest.raises(ValueError):
                gp.refit(bad, SN)
        assert lib.sigp_set_length_scales(h, L.ptr(ells), d - 1) == L.BAD_ARG
        for v in (0.0, -1.0, np.nan, np.inf):
            e = ells.copy(); e[1] = v
            assert lib.sigp_set_length_scales(h, L.ptr(e), d) == L.BAD_ARG, v
            with pytest.raises(ValueError):
                gp.refit(e, SN)
        assert lib.sigp_nlml_grad_ard(h, 1, L.ptr(th), d, 2, C.byref(val), L.ptr(g)) == L.BAD_ARG              # ntheta != d + 1
        assert lib.sigp_nlml_grad_ard(h, 1, L.ptr(th), d + 2, 2, C.byref(val), L.ptr(g)) == L.BAD_ARG
        assert lib.sigp_nlml_grad_ard(h, 0, L.ptr(th), d + 1, 2, C.byref(val), L.ptr(g)) == L.BAD_ARG          # the reference kernel
        assert lib.sigp_nlml_grad_ard(h, 1, L.ptr(th), d + 1, 1, C.byref(val), L.ptr(g)) == L.BAD_ARG          # no reference formulae here
        with pytest.raises(ValueError):
            gp.nlml_ard(th[:-1])
        # scales set: the reference kernel and the sharded fit are refused
        Sig = np.eye(d)
        assert lib.sigp_kernel_build_from_sigma(h, L.ptr(Sig), d, SN) == L.BAD_ARG
        assert lib.sigp_fit_predict(h, 0, 0.05, SN, L.ptr(Sig), d, L.ptr(out), None, None) == L.BAD_ARG
        assert lib.sigp_dist_fit(h, 1, 1.0, SN, None, 0, 2, 1, L.ptr(out), L.ptr(np.zeros(2)), L.ptr(np.zeros(2))) == L.BAD_ARG
        gp.refit(ells, SN)                                     # the handle is still usable, and nothing above changed its scales
        again = [np.array([gp.sigma_f_, gp.nlml_])] + list(gp.predict(Xs))
        for a, b in zip(good, again):
            assert _same_bits(a, b)
    with S.GPR(kernel="netdiffusion") as gp:
        with pytest.raises(ValueError):
            gp.fit(X, y, ells, SN)
        gp.fit(X, y, 0.05, SN)
        assert np.isfinite(gp.nlml_)
        with pytest.raises(ValueError):
            gp.nlml_ard(th)
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        with pytest.raises(ValueError):
            gp.fit(X, y, ells, SN)
        gp.fit(X, y, 2.0, SN)
        assert gp._lib.sigp_set_length_scales(gp._h, L.ptr(ells), d) == L.BAD_ARG
        assert gp._lib.sigp_nlml_grad_ard(gp._h, 1, L.ptr(th), d + 1, 2, C.byref(val), L.ptr(g)) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.nlml_ard(th)
        gp.refit(2.0, SN)
        assert np.isfinite(gp.nlml_)


def test_non_spd_gives_inf(S):
    n, d = 40, 3
    X, y, _ = O.synthetic_problem(n, d, 20252100)
    X[1] = X[0]                                                # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    th = np.concatenate([np.log(ard_scales(d, 20252101)), [-np.inf]])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        v, g = gp.nlml_ard(th)
        assert np.isposinf(v) and g.shape == (d + 1,) and np.all(np.isposinf(g))
        v, g = gp.nlml_ard(np.array([800.0, 0.0, 0.0, np.log(SN)]))       # exp overflows
        assert np.isposinf(v) and np.all(np.isposinf(g))
        th[-1] = np.log(SN)
        v, g = gp.nlml_ard(th)                                 # ... and the handle goes on
        assert np.isfinite(v) and np.all(np.isfinite(g))


# ---- 7. the C ABI with a non-tight ldx ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_abi_length_scales_with_wide_rows(S, L, kind):
    n, d, pad = 200, 5, 3
    X, y, Xs = O.synthetic_problem(n, d, 20252200, m=3)
    Xn = O.synthetic_problem(4, d, 20252201, m=130)[2]
    ells = ard_scales(d, 20252202)

    def wide(A):
        out = np.full((A.shape[0], A.shape[1] + pad), np.nan)
        out[:, :A.shape[1]] = A
        return out

    def state(gp, mean, var):
        return [np.array([gp.sigma_f_, gp.nlml_]), gp.alpha_, gp.L_tilde_, mean, var]

    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ells, SN, Xs=Xs)
        mu, var = gp.predict(Xn)
        tight = state(gp, mu, var) + [gp._ride_mean, gp._ride_var]
        lib, h = gp._lib, gp._h
        Xw, Xsw, Xnw = wide(X), wide(Xs), wide(Xn)
        assert lib.sigp_set_train(h, L.ptr(Xw), n, d, d + pad, L.ptr(y)) == L.OK             # clears the scales
        assert lib.sigp_set_length_scales(h, L.ptr(ells), d) == L.OK
        assert lib.sigp_set_test(h, L.ptr(Xsw), 3, d + pad) == L.OK                           # staged while the scales are set
        out, rm, rv = np.zeros(4), np.zeros(3), np.zeros(3)
        assert lib.sigp_fit_predict(h, gp._kid, 1.0, SN, None, 0, L.ptr(out), L.ptr(rm), L.ptr(rv)) == L.OK
        gp.sigma_f_, gp.nlml_ = float(out[0]), float(out[1])
        mu_w, var_w = np.zeros(130), np.zeros(130)
        assert lib.sigp_predict(h, L.ptr(Xnw), 130, d + pad, L.ptr(mu_w), L.ptr(var_w)) == L.OK
        wide_ = state(gp, mu_w, var_w) + [rm, rv]
    for i, (a, b) in enumerate(zip(tight, wide_)):
        assert np.all(np.isfinite(a)) and _same_bits(a, b), i
