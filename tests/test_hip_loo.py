"""GPU tier of the leave-one-out cross-validation (``GPR.loo`` / ``loo_batch`` / ``loo_grid``, ``SmallBatch.run(loo=...)``,
``retro_grid_search(criterion=...)``): against REAL refits on n - 1 points by the oracle and by the engine itself, and -- for the
sizes where n refits are out of reach -- against the closed forms that tests/test_loo_host.py pins to such refits.
Tolerances are the suite's own (tests/test_hip_parity.py): predictions 1e-8, scalars 1e-9 / 1e-8 relative as stated per test."""
import numpy as np
import pytest

from conftest import GOLDEN_NAMES, load_golden
from oracle import gp_oracle as O
from test_loo_host import loo_closed_form, oracle_refits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _problem(kind, n, seed):
    """the smoke test's settings: (X, y, ell, sn~, M)"""
    if kind == "netdiffusion":
        X, y, _ = O.synthetic_problem(n, 12, seed)
        return X, y, 0.05, 1e-2, O.laplacian_M(X)
    X, y, _ = O.synthetic_problem(n, 8, seed)
    return X, y, np.sqrt(8.0), 1e-2, None


def _cond(Kt):
    w = np.linalg.eigvalsh(Kt)          # K~ is symmetric positive definite: cond_2 = lambda_max / lambda_min
    return float(w[-1] / w[0])


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1.0)))


def _check_loo(tag, r, y, mean, var, nlpd, sse, tol=1e-8):
    e_mean = float(np.max(np.abs(r["mean"] - mean)) / np.max(np.abs(y)))
    e_var, e_nlpd, e_sse = _relmax(r["var"], var), abs(r["nlpd"] - nlpd) / abs(nlpd), abs(r["sse"] - sse) / abs(sse)
    print("%s: mean %.3g  var %.3g  nlpd %.3g  sse %.3g" % (tag, e_mean, e_var, e_nlpd, e_sse))
    assert e_mean <= tol, (tag, e_mean)
    assert e_var <= tol, (tag, e_var)
    assert e_nlpd <= tol and e_sse <= tol, (tag, e_nlpd, e_sse)


# ---- 1. GPR.loo against real refits (oracle) and, for large n, the pinned closed form -------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n", [2, 37, 128, 129, 300])
def test_loo_refit_equals_real_oracle_refits_at_every_point(S, kind, n):
    X, y, ell, sn, M = _problem(kind, n, 20240100 + n)
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    assert _cond(Kt) <= 1e6
    mean, var, _ = oracle_refits(X, y, ell, sn, kind, M)
    res = y - mean
    nlpd, sse = float(np.sum(0.5 * np.log(2 * np.pi * var) + res * res / (2 * var))), float(np.sum(res * res))
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        r = gp.loo("refit")
    assert r["mean"].shape == (n,) and r["var"].shape == (n,)
    _check_loo("%s n=%d" % (kind, n), r, y, mean, var, nlpd, sse)
    assert abs(r["mse"] - sse / n) <= 1e-8 * sse / n
    assert abs(r["skill"] - (1.0 - sse / np.sum((y - y.mean()) ** 2))) <= 1e-8 * max(1.0, abs(r["skill"]))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n", [1000, 2500])
def test_loo_large_n_equals_the_closed_form(S, kind, n):
    """n = 2500 crosses the 2048 panel boundary of the blocked factor and of the triangular inversion."""
    X, y, ell, sn, M = _problem(kind, n, 20240200 + n)
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    c = _cond(Kt)
    print("cond(K~) = %.3g" % c)
    assert c <= 1e6
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        got = {mode: gp.loo(mode) for mode in ("refit", "fixed")}
    for mode in ("refit", "fixed"):
        cf = loo_closed_form(Kt, y, mode)
        _check_loo("%s n=%d %s" % (kind, n, mode), got[mode], y, cf["mean"], cf["var"], cf["nlpd"], cf["sse"])


# ---- 2. the engine against itself ----------------------------------------------------------------------------------------------
def test_loo_equals_the_engines_own_refits_and_fixed_mode_differs_by_sigma_f_alone(S):
    n = 64
    X, y, ell, sn, _ = _problem("rbf", n, 20240301)
    mean, var = np.zeros(n), np.zeros(n)
    with S.GPR(kernel="rbf") as gp:
        for i in range(n):
            k = np.arange(n) != i
            gp.fit(X[k], y[k], ell, sn, Xs=X[i:i + 1])
            mu, v = gp.predict(X[i:i + 1])
            mean[i], var[i] = mu[0], v[0]
        gp.fit(X, y, ell, sn)
        rf, fx = gp.loo("refit"), gp.loo("fixed")
        sf = gp.sigma_f_
        A = gp.alpha_.reshape(-1) * sf
    e_mean, e_var = float(np.max(np.abs(rf["mean"] - mean)) / np.max(np.abs(y))), _relmax(rf["var"], var)
    print("engine refits: mean %.3g var %.3g" % (e_mean, e_var))
    assert e_mean <= 1e-8 and e_var <= 1e-8
    assert np.array_equal(rf["mean"], fx["mean"])                      # the means do not depend on the mode: identical bits
    sf_loo = (n * sf - A * (y - rf["mean"])) / (n - 1)
    e_ratio = _relmax(fx["var"] / rf["var"], sf / sf_loo)
    print("var fixed / refit against sigma_f / sigma_f(-i): %.3g" % e_ratio)
    assert e_ratio <= 1e-12


# ---- 3. loo leaves the fit alone and is deterministic ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
def test_predict_after_loo_same_bits_and_loo_twice_same_bits(S, kind):
    n = 300
    X, y, ell, sn, M = _problem(kind, n, 20240401)
    Xs = O.synthetic_problem(5, X.shape[1], 77)[0]
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        mu0, var0 = gp.predict(Xs)
        nl0, a0 = gp.nlml_, gp.alpha_.copy()
        r1 = gp.loo()
        mu1, var1 = gp.predict(Xs)
        r2 = gp.loo()
        r3 = gp.loo("fixed")
        mu2, var2 = gp.predict(Xs)
        assert gp.nlml_ == nl0 and np.array_equal(gp.alpha_, a0)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1) and np.array_equal(mu0, mu2) and np.array_equal(var0, var2)
    for k in ("mean", "var"):
        assert np.array_equal(r1[k], r2[k])
    assert r1["nlpd"] == r2["nlpd"] and r1["sse"] == r2["sse"] and r3["sse"] == r1["sse"]


# ---- 4. lockstep batch and grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4, 8])
def test_loo_batch_members_equal_single_fits_and_a_non_spd_member_stays_alone(S, group):
    B, n, d = 5, 200, 8
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240500 + b)
    Xb[2, 1] = Xb[2, 0]                                  # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    ell = np.array([np.sqrt(8.0)] * B + [2.0] * B)
    sn = np.array([1e-2] * B + [3e-2] * B)
    sn[2] = 0.0                                          # fit 2 = data set 2 without noise: not positive definite
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=group)
        r = gp.loo_batch(ell, sn, group=group)
        sc = gp.loo_batch(ell, sn, group=group, predictions=False)
        assert set(sc) == {"nlpd", "sse"}
        assert np.array_equal(sc["nlpd"], r["nlpd"]) and np.array_equal(sc["sse"], r["sse"])
        assert r["mean"].shape == (2 * B, n) and r["var"].shape == (2 * B, n)
        assert np.isposinf(r["nlpd"][2]) and np.isposinf(r["sse"][2]) and np.all(np.isnan(r["mean"][2])) and np.all(np.isnan(r["var"][2]))
        worst = 0.0
        for i in range(2 * B):
            if i == 2:
                continue
            gp.fit(Xb[i % B], yb[i % B], ell[i], sn[i])
            one = gp.loo()
            e = max(float(np.max(np.abs(r["mean"][i] - one["mean"])) / np.max(np.abs(yb[i % B]))), _relmax(r["var"][i], one["var"]),
                    abs(r["nlpd"][i] / one["nlpd"] - 1), abs(r["sse"][i] / one["sse"] - 1))
            worst = max(worst, e)
            assert e <= 1e-12, (group, i, e)
        print("group %d: worst member against its single fit %.3g" % (group, worst))


@pytest.mark.parametrize("kind,tol", [("rbf", 1e-12), ("netdiffusion", 1e-8)])
def test_loo_grid_equals_a_loop_of_loo(S, kind, tol):
    """RBF: lockstep groups against single fits of the same blocked engine (1e-12).  Reference kernel: the one-workgroup-per-fit
    kernel against the blocked engine, two different factorisations of the same K~ (the suite's 1e-8)."""
    n = 100
    X, y, ell, sn, M = _problem(kind, n, 20240601)
    ells, sns = np.array([0.5, 1.0, 2.0]) * ell, np.array([1e-2, 1e-1])
    with S.GPR(kernel=kind) as gp:
        g = gp.loo_grid(X, y, ells, sns, M=M)
        assert g["nlpd"].shape == (3, 2) and g["sse"].shape == (3, 2)
        for a, e in enumerate(ells):
            for b, s_ in enumerate(sns):
                gp.fit(X, y, e, s_, M=M)
                one = gp.loo()
                print(kind, a, b, abs(g["nlpd"][a, b] / one["nlpd"] - 1), abs(g["sse"][a, b] / one["sse"] - 1))
                assert abs(g["nlpd"][a, b] - one["nlpd"]) <= tol * abs(one["nlpd"]) and abs(g["sse"][a, b] - one["sse"]) <= tol * abs(one["sse"])


# ---- 5. the reference's own kernel at the reference's own size: every golden record x its stored theta, ONE launch ------------------
def test_small_batch_loo_all_golden_records_in_one_launch(S):
    """Against the closed form on the oracle's K~; tolerance max(1e-8, 1e3 * 2.3e-16 * cond(K~)) as tests/test_hip_round5.py uses
    for quantities that go through the in-LDS inverse (both sides carry cond(K~) eps), relative for var, against max(1, |.|) for
    the scores and max(1, max|y|) for the means."""
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    assert len(recs) == 63
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        want = []
        for r in recs:
            ds = sb.add_dataset(r["X"], r["y"], r["Xs"], r["M"])
            for th, nl in zip(r["mlii_theta"], r["mlii_nlml"]):
                ell, sn = float(np.exp(th[0])), float(np.exp(th[1]))
                if ell > 1e6:
                    continue          # l = 3.1e10: the eigen route and scipy's Pade expm differ there
                sb.add_fit(ds, ell, sn, expm="eigh")
                want.append((r, ell, sn, nl))
        assert len(want) >= 63 * 5
        plain0 = sb.run()
        gp.profile(True, ["small"])
        launches0 = gp.profile_get()["small"]["launches"]
        res = sb.run(loo="refit")
        assert gp.profile_get()["small"]["launches"] - launches0 == 1          # ONE launch for the lot
        fixed = sb.run(loo="fixed")
        plain1 = sb.run()
    assert set(plain0) == {"sigma_f", "nlml", "info", "sigma_n", "mean", "var"} and set(plain1) == set(plain0)
    for k in plain0:
        assert np.array_equal(plain0[k], plain1[k], equal_nan=True), k
    nmax = max(len(np.asarray(r["y"]).reshape(-1)) for r in recs)
    assert res["loo_mean"].shape == (len(want), nmax) and res["loo_var"].shape == (len(want), nmax)
    ninf, worst = 0, 0.0
    for i, (r, ell, sn, nl) in enumerate(want):
        y = np.asarray(r["y"], dtype=np.float64).reshape(-1)
        n = len(y)
        assert np.all(np.isnan(res["loo_mean"][i, n:])) and np.all(np.isnan(res["loo_var"][i, n:]))
        if np.isinf(nl):              # the reference's except branch
            ninf += 1
            assert res["info"][i] > 0 and np.isposinf(res["loo_nlpd"][i]) and np.isposinf(res["loo_sse"][i])
            assert np.all(np.isnan(res["loo_mean"][i])) and np.all(np.isnan(res["loo_var"][i]))
            continue
        assert res["info"][i] == 0
        Kt = O.fit_predict(r["X"], r["y"], r["Xs"], ell, sn, M=r["M"], ref_idiom=False)["K_tilde"]
        tol = max(1e-8, 1e3 * 2.3e-16 * np.linalg.cond(Kt))
        for mode, got in (("refit", res), ("fixed", fixed)):
            cf = loo_closed_form(Kt, y, mode)
            e = max(float(np.max(np.abs(got["loo_mean"][i, :n] - cf["mean"])) / max(1.0, np.max(np.abs(y)))), _relmax(got["loo_var"][i, :n], cf["var"]),
                    abs(got["loo_nlpd"][i] - cf["nlpd"]) / max(1.0, abs(cf["nlpd"])), abs(got["loo_sse"][i] - cf["sse"]) / max(1.0, abs(cf["sse"])))
            worst = max(worst, e / tol)
            assert e <= tol, (i, mode, ell, sn, e, tol)
        assert np.array_equal(res["loo_mean"][i, :n], fixed["loo_mean"][i, :n])
    print("worst error / tolerance over %d fits: %.3g" % (len(want), worst))
    assert ninf == 63


# ---- 6. the retro grid search with a cross-validated criterion -----------------------------------------------------------------------
def test_retro_grid_search_criteria(S):
    from seaiceextentforecasting_amd.retro import _problem as retro_problem, _retro_inputs
    script = "north_September"
    g = load_golden(script + "_retro")
    fmin, fmax = g["args"]
    ells, sns = np.array([1e-3, 0.05, 1.0]), np.array([1e-2, 1.0, 1e2, 1e4])
    tab = S.SCRIPT_TABLE[script]
    ny = fmax - fmin + 1
    with S.GPR(kernel="netdiffusion") as gp:
        default = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp)
        nlml = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="nlml")
        nlpd = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="loo_nlpd")
        sse = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="loo_sse")
        sb = S.SmallBatch(gp)
        for k, region in enumerate(tab["regions"]):
            for year in range(fmin, fmax + 1):
                _, y, sic, sst = _retro_inputs(tab, g["SIC"], g["SIEs_dt"], g["SST"], region, year, fmin)
                X, Xs, M = retro_problem(tab, k, y, sic, sst)
                ds = sb.add_dataset(X, y, None, M)
                for e in ells:
                    for s_ in sns:
                        sb.add_fit(ds, e, s_, expm="eigh")
        r = sb.run(loo="refit")
    assert set(default) == set(tab["regions"]) == set(nlml) == set(nlpd) == set(sse)
    for k, region in enumerate(tab["regions"]):
        assert default[region].tobytes() == nlml[region].tobytes()
        assert nlpd[region].shape == (ny, len(ells), len(sns)) and sse[region].shape == (ny, len(ells), len(sns))
        assert np.array_equal(nlpd[region], r["loo_nlpd"].reshape(len(tab["regions"]), ny, len(ells), len(sns))[k])
        assert np.array_equal(sse[region], r["loo_sse"].reshape(len(tab["regions"]), ny, len(ells), len(sns))[k])


# ---- 7. what has no leave-one-out ------------------------------------------------------------------------------------------------------
def test_loo_of_one_point_and_of_the_fp32_engine_are_value_errors(S):
    X, y, ell, sn, _ = _problem("rbf", 40, 20240701)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X[:1], y[:1], ell, sn)
        with pytest.raises(ValueError):
            gp.loo()
        with pytest.raises(ValueError):
            gp.loo("bogus")
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        X12 = O.synthetic_problem(1, 12, 3)[0]
        sb.add_fit(sb.add_dataset(X12, y[:1], None, np.zeros((12, 12))), 0.05, 1e-2)
        with pytest.raises(ValueError):
            sb.run(loo="refit")
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, ell, sn)
        with pytest.raises(ValueError, match="fp64"):
            gp.loo()
