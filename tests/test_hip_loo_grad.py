"""GPU tier of the leave-one-out gradients (``GPR.loo(grad=True)`` / ``loo_batch(grad=True)`` / ``loo_objective`` /
``optimize(criterion=...)`` / ``optimize_batch(criterion=...)``) against the NumPy closed form that tests/test_loo_grad_host.py pins
to central differences.

Scale of every error: S = sum_i |per-point term| of the component (the gradients themselves vanish at an optimum).  The reference is
computed by two routes to K~^-1 (explicit inverse; Cholesky + U U^T, the device's own route); their difference / S -- the *spread* -- is
the reference's own error, and the device must stay within max(1e-8, 10 x spread): 1e-8 is the suite's scalar tolerance, the factor
10 allows for a third summation order."""
import functools

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_loo_grad_host import dk_tilde, k_tilde, loo_grad_closed_form, problem
from test_loo_host import loo_closed_form

pytestmark = pytest.mark.gpu

KEYS = ("nlpd_grad", "sse_grad")
BOUNDS = [(-3.0, 5.0), (-12.0, 3.0)]
THETA0 = np.log([np.sqrt(8.0), 1e-2])


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _reference_of(kind, X, y, ell, sn, M):
    """{mode: (closed form by the explicit inverse, spread [2 keys][2])}: computed once per problem"""
    Kt, dK = k_tilde(kind, X, ell, sn, M), dk_tilde(kind, X, ell, sn, M)
    out = {}
    for mode in ("refit", "fixed"):
        a, b = loo_grad_closed_form(Kt, dK, y, mode, "inv"), loo_grad_closed_form(Kt, dK, y, mode, "chol")
        out[mode] = (a, {k: np.abs(a[k] - b[k]) / a[k[:-4] + "S"] for k in KEYS})
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, n):
    X, y, ell, sn, M = problem(kind, n, 20250300 + n)
    return (X, y, ell, sn, M), _reference_of(kind, X, y, ell, sn, M)


def _check(tag, got, ref, spread):
    """device error / S <= max(1e-8, 10 spread) for both scores and both parameters; the case counts only if spread <= 1e-8"""
    worst = 0.0
    for k in KEYS:
        err = np.abs(np.asarray(got[k]) - ref[k]) / ref[k[:-4] + "S"]
        print("%s %s: error / S %s   spread %s" % (tag, k, err, spread[k]))
        assert np.all(spread[k] <= 1e-8), (tag, k, spread[k])
        assert np.all(err <= np.maximum(1e-8, 10.0 * spread[k])), (tag, k, err, spread[k])
        worst = max(worst, float(np.max(err)))
    return worst


# ---- 1. the device against the NumPy reference -------------------------------------------------------------------------------------
CASES = [(kind, n) for kind in ("rbf", "matern52", "netdiffusion") for n in (2, 37, 128, 129, 300)] + [("rbf", 1000)]


@pytest.mark.parametrize("kind,n", CASES)
def test_loo_gradients_equal_the_closed_form(S, kind, n):
    (X, y, ell, sn, M), ref = _reference(kind, n)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        got = {mode: gp.loo(mode, grad=True) for mode in ("refit", "fixed")}
    for mode in ("refit", "fixed"):
        assert got[mode]["nlpd_grad"].shape == (2,) and got[mode]["sse_grad"].shape == (2,)
        _check("%s n=%d %s" % (kind, n, mode), got[mode], *ref[mode])


# ---- 2. invariants ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
def test_gradient_call_leaves_scores_fit_and_bits_alone(S, kind):
    n = 300
    X, y, ell, sn, M = problem(kind, n, 20250401)
    Xs = O.synthetic_problem(5, X.shape[1], 77)[0]
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        mu0, var0 = gp.predict(Xs)
        nl0, a0 = gp.nlml_, gp.alpha_.copy()
        plain = {mode: gp.loo(mode) for mode in ("refit", "fixed")}
        g1 = {mode: gp.loo(mode, grad=True) for mode in ("refit", "fixed")}
        g2 = {mode: gp.loo(mode, grad=True) for mode in ("refit", "fixed")}
        mu1, var1 = gp.predict(Xs)
        again = gp.loo()
        assert gp.nlml_ == nl0 and np.array_equal(gp.alpha_, a0)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    for mode in ("refit", "fixed"):
        assert set(g1[mode]) == set(plain[mode]) | set(KEYS)
        for k in ("mean", "var"):
            assert np.array_equal(g1[mode][k], plain[mode][k]), (mode, k)
        for k in ("nlpd", "sse", "mse", "skill"):
            assert g1[mode][k] == plain[mode][k], (mode, k)
        for k in KEYS:
            assert np.array_equal(g1[mode][k], g2[mode][k]), (mode, k)           # two calls: identical bits
    assert np.array_equal(g1["refit"]["sse_grad"], g1["fixed"]["sse_grad"])      # the squared errors do not depend on the mode
    assert not np.array_equal(g1["refit"]["nlpd_grad"], g1["fixed"]["nlpd_grad"])
    assert again["nlpd"] == plain["refit"]["nlpd"] and np.array_equal(again["var"], plain["refit"]["var"])


# ---- 3. lockstep batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_loo_grad_batch_members_equal_the_closed_form_and_single_fits(S, group):
    B, n, d = 5, 200, 8
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20250500 + b)
    Xb[2, 1] = Xb[2, 0]                                  # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    ell = np.array([np.sqrt(8.0)] * B + [2.0] * B)
    sn = np.array([1e-2] * B + [3e-2] * B)
    sn[2] = 0.0                                          # fit 2 = data set 2 without noise: not positive definite
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=group)
        plain = gp.loo_batch(ell, sn, group=group)
        r = gp.loo_batch(ell, sn, group=group, grad=True)
        assert r["nlpd_grad"].shape == (2 * B, 2) and r["sse_grad"].shape == (2 * B, 2)
        for k in ("nlpd", "sse", "mean", "var"):
            assert np.array_equal(r[k], plain[k], equal_nan=True), k
        assert np.isposinf(r["nlpd"][2]) and np.all(np.isposinf(r["nlpd_grad"][2])) and np.all(np.isposinf(r["sse_grad"][2]))
        worst_ref = worst_one = 0.0
        for i in range(2 * B):
            if i == 2:
                continue
            ref = _reference_of("rbf", Xb[i % B], yb[i % B], ell[i], sn[i], None)["refit"]
            member = {k: r[k][i] for k in KEYS}
            worst_ref = max(worst_ref, _check("group %d member %d" % (group, i), member, *ref))
            gp.fit(Xb[i % B], yb[i % B], ell[i], sn[i])
            one = gp.loo(grad=True)
            for k in KEYS:
                e = float(np.max(np.abs(member[k] - one[k]) / ref[0][k[:-4] + "S"]))
                worst_one = max(worst_one, e)
                assert e <= 1e-10, (group, i, k, e)
        print("group %d: worst member against the closed form %.3g, against its single fit %.3g (error / S)" % (group, worst_ref, worst_one))


# ---- 4. the optimiser -------------------------------------------------------------------------------------------------------------------
def _numpy_objective(X, y, key):
    def f(th):
        ell, sn = np.exp(th)
        Kt = k_tilde("rbf", X, ell, sn)
        try:
            np.linalg.cholesky(Kt)
        except np.linalg.LinAlgError:
            return np.inf, np.asarray([np.inf, np.inf])
        return float(loo_closed_form(Kt, y, "refit")[key]), loo_grad_closed_form(Kt, dk_tilde("rbf", X, ell, sn), y, "refit")[key + "_grad"]
    return f


@pytest.mark.parametrize("criterion", ["loo_nlpd", "loo_sse"])
def test_optimize_reaches_the_reference_optimum(S, criterion):
    X, y, _ = O.synthetic_problem(200, 8, 20250700)
    f = _numpy_objective(X, y, criterion[4:])
    ref = minimize(f, THETA0, jac=True, method="L-BFGS-B", bounds=BOUNDS)
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        res = gp.optimize(THETA0, method="L-BFGS-B", criterion=criterion, bounds=BOUNDS)
        assert gp._fitted and gp.ell_ == float(np.exp(res.x[0]))
    at = f(res.x)[0]
    print("%s: reference %.9g at %s in %d evaluations; device %.9g at %s in %d (oracle there: %.9g)" % (criterion, ref.fun, ref.x, ref.nfev, res.fun, res.x, res.nfev, at))
    assert at <= ref.fun + 1e-6 * abs(ref.fun)
    assert res.nfev <= 3 * ref.nfev


def test_optimize_batch_reaches_every_members_reference_optimum(S):
    """Data sets: the first three seeds from 20250700 on whose reference optimum lies inside the reference's bounds (the lockstep BFGS has
    none: a data set whose score keeps falling towards l -> inf has no optimum to compare)."""
    sets, refs, seed = [], [], 20250700
    while len(sets) < 3:
        X, y, _ = O.synthetic_problem(200, 8, seed)
        ref = minimize(_numpy_objective(X, y, "nlpd"), THETA0, jac=True, method="L-BFGS-B", bounds=BOUNDS)
        if all(lo + 1e-3 < x < hi - 1e-3 for x, (lo, hi) in zip(ref.x, BOUNDS)):
            sets.append((X, y)); refs.append(ref)
        seed += 1
    with S.GPR(kernel="rbf") as gp:
        res = gp.optimize_batch(np.stack([s_[0] for s_ in sets]), np.stack([s_[1] for s_ in sets]), THETA0, group=3, criterion="loo_nlpd")
    for b, ((X, y), ref) in enumerate(zip(sets, refs)):
        at = _numpy_objective(X, y, "nlpd")(res["x"][b])[0]
        print("member %d: reference %.9g in %d evaluations; device %.9g at %s, %d rounds (oracle there: %.9g)" % (b, ref.fun, ref.nfev, res["fun"][b], res["x"][b], res["nfev"], at))
        assert at <= ref.fun + 1e-6 * abs(ref.fun)
        assert res["nfev"] <= 3 * ref.nfev


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_what_has_no_leave_one_out_gradient(S):
    from seaiceextentforecasting_amd import _lib as L
    X, y, ell, sn, _ = problem("rbf", 40, 20250801)
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, ell, sn)
        with pytest.raises(ValueError, match="fp64"):
            gp.loo(grad=True)
    with S.GPR(kernel="rbf") as gp:
        with pytest.raises(RuntimeError):
            gp.loo_objective(THETA0)                         # no data staged
        gp.set_data(X, y)
        with pytest.raises(RuntimeError):
            gp.loo(grad=True)                                # not fitted
        out = np.zeros(4)
        assert gp._lib.sigp_loo_grad(gp._h, 0, None, 0, None, None, L.ptr(out), L.ptr(out)) == L.BAD_ARG      # ... and the library says so too
        gp.fit(X[:1], y[:1], ell, sn)
        with pytest.raises(ValueError):
            gp.loo(grad=True)                                # one point
        with pytest.raises(ValueError):
            gp.optimize(THETA0, criterion="bogus")
        with pytest.raises(ValueError):
            gp.loo_objective(THETA0, criterion="nlml")
    Xn, yn, elln, snn, M = problem("netdiffusion", 30, 20250802)
    with S.GPR(kernel="netdiffusion") as gp:
        with pytest.raises(ValueError, match="reference kernel"):
            gp.optimize_batch([Xn], [yn], np.log([elln, snn]), M=[M], criterion="loo_nlpd")
        gp.fit(Xn, yn, elln, snn, M=M)
        out = np.zeros(4)
        assert gp._lib.sigp_loo_grad(gp._h, 0, None, 0, None, None, L.ptr(out), L.ptr(out)) == L.BAD_ARG      # the reference kernel without M @ Sigma~
        assert np.all(np.isfinite(gp.loo(grad=True)["nlpd_grad"]))


# ---- 6. the profile entries of the calls ------------------------------------------------------------------------------------------------
# (launches, flops, bytes) of SIGP_KC_MLII at n = 300 (three 128-tiles, padded rows in the last), d = 8, RBF; the lockstep entries: one
# group of two members.  The figures are sums of products of small integers, all exactly representable in a double, read off the library
# before the host drivers of these entry points were single-sourced.
MLII_PINS = {
    "loo": (2, 19054368.0, 360000.0),                         # triangular inversion, the row pass
    "loo_grad": (6, 95714208.0, 7828416.0),                   # ... + U U^T, the n^2 passes, the product W', the row / column / point passes
    "nlml_exact": (2, 37748736.0, 0.0),                       # triangular inversion, U U^T
    "loo_batch": (2, 38108736.0, 720000.0),
    "loo_grad_batch": (6, 191428416.0, 15656832.0),
    "cv_batch": (5, 207349576.0, 65400960.0),                 # triangular inversion, four entries for the one pass of 60 folds (block 5, gap 1)
    "nlml_batch": (2, 75497472.0, 0.0),
}


def test_loo_nlml_and_lockstep_profile_entries(S):
    n, d = 300, 8
    Xb = np.zeros((2, n, d)); yb = np.zeros((2, n))
    for b in range(2):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20250900 + b)
    ell, sn = np.array([np.sqrt(8.0), 2.0]), np.array([1e-2, 3e-2])
    th = np.log(np.stack([ell, sn], axis=1))
    single = {"loo": lambda gp: gp.loo(), "loo_grad": lambda gp: gp.loo(grad=True), "nlml_exact": lambda gp: gp.nlml(th[0], grad="exact")}
    batch = {"loo_batch": lambda gp: gp.loo_batch(ell, sn, group=2), "loo_grad_batch": lambda gp: gp.loo_batch(ell, sn, group=2, grad=True),
             "cv_batch": lambda gp: gp.cv_batch(ell, sn, 5, gap=1, group=2), "nlml_batch": lambda gp: gp.nlml_batch(th, group=2)}
    got = {}
    with S.GPR(kernel="rbf") as gp:
        gp.fit(Xb[0], yb[0], ell[0], sn[0])
        for name, fn in single.items():                      # (nlml comes last: it refits)
            gp.profile_reset()
            fn(gp)
            p = gp.profile_get()["mlii"]
            got[name] = (p["launches"], p["flops"], p["bytes"])
            print("%s: %r" % (name, got[name]))
        gp.upload_batch(Xb, yb, None, group=2)
        for name, fn in batch.items():
            gp.profile_reset()
            fn(gp)
            p = gp.profile_get()["mlii"]
            got[name] = (p["launches"], p["flops"], p["bytes"])
            print("%s: %r" % (name, got[name]))
    assert got == MLII_PINS, got


# ---- 7. a partial last lockstep group -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _partial_group_problem():
    """three fits in groups of two at n = 130 (two 128-tiles, 126 padded rows): the second group has one member in a workspace laid out for
    two, the one place where offsets indexed by the group size and by the members present part ways"""
    B, n, d = 3, 130, 8
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20251000 + b)
    ell, sn = np.array([np.sqrt(8.0), 2.0, 3.5]), np.array([1e-2, 3e-2, 1e-1])
    return Xb, yb, ell, sn, np.log(np.stack([ell, sn], axis=1))


def _differing(pairs):
    bad = []
    for tag, a, b in pairs:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        same = np.array_equal(a, b)
        print("%s: %s (max |difference| %.3g)" % (tag, "same bits" if same else "DIFFERS", float(np.max(np.abs(a - b)))))
        if not same:
            bad.append(tag)
    return bad


def test_partial_last_lockstep_group_equals_single_fits(S):
    """``loo_batch``, ``loo_batch(grad=True)`` and ``cv_batch`` against the single-fit calls at the same (l, sn~): the same bits.
    ``nlml_batch`` already runs ragged last groups against ``nlml(grad="exact")`` in
    test_hip_argument_ranges.py::test_lockstep_mlii_gradient_at_feature_counts_around_and_past_one_pad (five fits in groups of three, and a
    member's bits equal whatever its group) and in test_hip_round2.py::test_lockstep_mlii_gradients_match_the_oracle_for_every_member, at the
    tolerance two different reductions allow: ``sigp_nlml_grad`` reduces a stored dK~ row by row, ``sigp_nlml_grad_batch`` recomputes it over
    the lower triangle, so the sums run in another order (2.8e-13 on gradients of order 10 here).  What has the same bits is pinned here too:
    its values against the single fit, and its gradient against the one-member call of the same entry, where the group size and the members
    present coincide."""
    Xb, yb, ell, sn, th = _partial_group_problem()
    block, gap = 5, 1
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=2)
        loo = gp.loo_batch(ell, sn, group=2)
        loog = gp.loo_batch(ell, sn, group=2, grad=True)
        cv = gp.cv_batch(ell, sn, block, gap=gap, group=2)
        nl, nlg = gp.nlml_batch(th, group=2, grad="exact")
        alone = [gp.nlml_batch(th[i:i + 1], first=i, group=2, grad="exact") for i in range(len(ell))]
        pairs = []
        for i in range(len(ell)):
            gp.fit(Xb[i], yb[i], ell[i], sn[i])
            one, oneg, onecv = gp.loo(), gp.loo(grad=True), gp.cv(block, gap)
            v, _ = gp.nlml(th[i], grad=None)
            pairs += [("member %d loo_batch %s" % (i, k), loo[k][i], one[k]) for k in ("nlpd", "sse", "mean", "var")]
            pairs += [("member %d loo_batch(grad) %s" % (i, k), loog[k][i], oneg[k]) for k in ("nlpd", "sse", "mean", "var") + KEYS]
            pairs += [("member %d cv_batch %s" % (i, k), cv[k][i], onecv[k]) for k in ("nlpd", "sse", "mean", "var")]
            pairs += [("member %d nlml_batch value" % i, nl[i], v), ("member %d nlml_batch value (alone)" % i, nl[i], alone[i][0][0]),
                      ("member %d nlml_batch gradient (alone)" % i, nlg[i], alone[i][1][0])]
    bad = _differing(pairs)
    assert not bad, bad
