"""GPU tier of the leave-block-out cross-validation (``GPR.cv`` / ``cv_batch`` / ``cv_grid``, ``SmallBatch.run(cv=...)``,
``retro_grid_search(criterion="cv_*")``): against REAL refits without each fold's window by the oracle, and -- where that many refits are
out of reach -- against the block closed form that tests/test_cv_host.py pins to such refits.
Tolerances are the suite's own (tests/test_hip_loo.py): predictions and scores 1e-8, engine against engine 1e-12."""
import numpy as np
import pytest

from conftest import GOLDEN_NAMES, load_golden
from oracle import gp_oracle as O
from test_cv_host import cv_closed_form, cv_folds, cv_problem, oracle_block_refits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _cond(Kt):
    w = np.linalg.eigvalsh(Kt)          # K~ is symmetric positive definite: cond_2 = lambda_max / lambda_min
    return float(w[-1] / w[0])


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1.0)))


def _scores(y, mean, var):
    res = y - mean
    return float(np.sum(0.5 * np.log(2 * np.pi * var) + res * res / (2 * var))), float(np.sum(res * res))


def _errors(r, y, mean, var, nlpd, sse):
    return (float(np.max(np.abs(r["mean"] - mean)) / np.max(np.abs(y))), _relmax(r["var"], var), abs(r["nlpd"] - nlpd) / abs(nlpd), abs(r["sse"] - sse) / abs(sse))


def _check_cv(tag, r, y, mean, var, nlpd, sse, tol=1e-8):
    e = _errors(r, y, mean, var, nlpd, sse)
    print("%s: mean %.3g  var %.3g  nlpd %.3g  sse %.3g" % ((tag,) + e))
    assert max(e) <= tol, (tag, e)


def _against(a, b, y):
    """engine against engine: worst relative difference of two results of cv / loo"""
    return max(float(np.max(np.abs(a["mean"] - b["mean"])) / np.max(np.abs(y))), _relmax(a["var"], b["var"]), abs(a["nlpd"] / b["nlpd"] - 1), abs(a["sse"] / b["sse"] - 1))


# ---- 1. GPR.cv against real oracle refits ----------------------------------------------------------------------------------------------
# the minimum; a ragged last fold with clipped edge windows; windows across row 128 with n_pad = 256; aligned full tiles; an unaligned
# window of exactly 128 rows; many small windows, one of them straddling column 128
@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n,block,gap", [(2, 1, 0), (37, 5, 2), (130, 64, 32), (300, 128, 0), (300, 100, 14), (300, 7, 3)])
def test_cv_equals_real_oracle_refits_without_each_window(S, kind, n, block, gap):
    X, y, ell, sn, M = cv_problem(kind, n, 20250100 + n)
    y = np.asarray(y).reshape(-1)
    full = O.fit_predict(X, y.reshape(-1, 1), X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)
    assert _cond(full["K_tilde"]) <= 1e6
    mean, var, sf = oracle_block_refits(X, y, ell, sn, kind, M, block, gap)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        got = {mode: gp.cv(block, gap, mode) for mode in ("refit", "fixed")}
    want = {"refit": var, "fixed": var / sf * float(full["sigma_f"])}       # "fixed" keeps the full fit's signal variance
    for mode in ("refit", "fixed"):
        r = got[mode]
        assert r["mean"].shape == (n,) and r["var"].shape == (n,) and np.array_equal(r["folds"], cv_folds(n, block, gap))
        nlpd, sse = _scores(y, mean, want[mode])
        _check_cv("%s n=%d block=%d gap=%d %s" % (kind, n, block, gap, mode), r, y, mean, want[mode], nlpd, sse)
        assert abs(r["mse"] - sse / n) <= 1e-8 * sse / n
        assert abs(r["skill"] - (1.0 - sse / np.sum((y - y.mean()) ** 2))) <= 1e-8 * max(1.0, abs(r["skill"]))
    assert np.array_equal(got["refit"]["mean"], got["fixed"]["mean"])      # the means do not depend on the mode: identical bits


# ---- 2. large n against the pinned closed form: across the 2048 panel boundary, several K slices ---------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n,block,gap", [(2500, 100, 14), (1000, 128, 0)])
def test_cv_large_n_equals_the_closed_form(S, kind, n, block, gap):
    X, y, ell, sn, M = cv_problem(kind, n, 20240200 + n)
    y = np.asarray(y).reshape(-1)
    Kt = O.fit_predict(X, y.reshape(-1, 1), X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    c = _cond(Kt)
    print("cond(K~) = %.3g" % c)
    assert c <= 1e6
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        got = {mode: gp.cv(block, gap, mode) for mode in ("refit", "fixed")}
        print("cv_slices (auto) = %d" % int(gp._stat("cv_slices")))
    for mode in ("refit", "fixed"):
        cf = cv_closed_form(Kt, y, block, gap, mode)
        _check_cv("%s n=%d %s" % (kind, n, mode), got[mode], y, cf["mean"], cf["var"], cf["nlpd"], cf["sse"])


# ---- 3. block = 1 is leave-one-out ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
@pytest.mark.parametrize("n", [129, 300])
def test_cv_of_block_one_equals_loo(S, kind, n):
    X, y, ell, sn, M = cv_problem(kind, n, 20250100 + n)
    y = np.asarray(y).reshape(-1)
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        for mode in ("refit", "fixed"):
            e = _against(gp.cv(1, 0, mode), gp.loo(mode), y)
            print("%s n=%d %s: cv(1) against loo %.3g" % (kind, n, mode, e))
            assert e <= 1e-12


# ---- 4. K slices: any count gives the same result to rounding, the same count the same bits ------------------------------------------------
def test_cv_slices_agree_and_runs_repeat_bit_for_bit(S):
    n, block, gap = 300, 100, 14
    X, y, ell, sn, M = cv_problem("rbf", n, 20250100 + n)
    y = np.asarray(y).reshape(-1)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X, y, ell, sn)
        got, used = {}, {}
        for s_ in (1, 3, 0):
            gp.set_option("cv_slices", s_)
            got[s_] = [gp.cv(block, gap), gp.cv(block, gap)]
            used[s_] = int(gp._stat("cv_slices"))
        with pytest.raises(ValueError):
            gp.set_option("cv_slices", -1)
    assert used[1] == 1 and used[3] == 3 and used[0] >= 1
    for s_, (a, b) in got.items():
        assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["var"], b["var"]) and a["nlpd"] == b["nlpd"] and a["sse"] == b["sse"], s_
    for s_ in (3, 0):
        e = _against(got[s_][0], got[1][0], y)
        print("cv_slices %d (ran with %d) against 1: %.3g" % (s_, used[s_], e))
        assert e <= 1e-12


# ---- 5. the fit is left alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
def test_predict_alpha_nlml_and_loo_carry_the_same_bits_after_cv(S, kind):
    n = 300
    X, y, ell, sn, M = cv_problem(kind, n, 20240401)
    Xs = O.synthetic_problem(5, X.shape[1], 77)[0]
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        mu0, var0 = gp.predict(Xs)
        nl0, a0, l0 = gp.nlml_, gp.alpha_.copy(), gp.loo()
        gp.cv(7, 3)
        gp.cv(100, 14, "fixed")
        mu1, var1 = gp.predict(Xs)
        l1 = gp.loo()
        assert gp.nlml_ == nl0 and np.array_equal(gp.alpha_, a0)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    assert np.array_equal(l0["mean"], l1["mean"]) and np.array_equal(l0["var"], l1["var"]) and l0["nlpd"] == l1["nlpd"] and l0["sse"] == l1["sse"]


# ---- 6. lockstep batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 8])
def test_cv_batch_members_equal_single_fits_and_a_non_spd_member_stays_alone(S, group):
    B, n, d = 5, 200, 8
    block, gap = 48, 8                                   # windows of 56 and 64 rows; fold 2 removes [88, 152): across row 128
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240500 + b)
    Xb[2, 1] = Xb[2, 0]                                  # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    ell = np.array([np.sqrt(8.0)] * B + [2.0] * B)
    sn = np.array([1e-2] * B + [3e-2] * B)
    sn[2] = 0.0                                          # fit 2 = data set 2 without noise: not positive definite
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=group)
        r = gp.cv_batch(ell, sn, block, gap=gap, group=group)
        sc = gp.cv_batch(ell, sn, block, gap=gap, group=group, predictions=False)
        assert set(sc) == {"nlpd", "sse"}
        assert np.array_equal(sc["nlpd"], r["nlpd"]) and np.array_equal(sc["sse"], r["sse"])
        assert r["mean"].shape == (2 * B, n) and r["var"].shape == (2 * B, n)
        assert np.isposinf(r["nlpd"][2]) and np.isposinf(r["sse"][2]) and np.all(np.isnan(r["mean"][2])) and np.all(np.isnan(r["var"][2]))
        worst = 0.0
        for i in range(2 * B):
            if i == 2:
                continue
            gp.fit(Xb[i % B], yb[i % B], ell[i], sn[i])
            one = gp.cv(block, gap)
            e = _against(dict(mean=r["mean"][i], var=r["var"][i], nlpd=r["nlpd"][i], sse=r["sse"][i]), one, yb[i % B])
            worst = max(worst, e)
            assert e <= 1e-12, (group, i, e)
        print("group %d: worst member against its single fit %.3g" % (group, worst))


# ---- 7. grid -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tol", [("rbf", 1e-12), ("netdiffusion", 1e-8)])
def test_cv_grid_equals_a_loop_of_cv(S, kind, tol):
    """RBF: lockstep groups against single fits of the same blocked engine (1e-12).  Reference kernel: the one-workgroup-per-fit
    kernel against the blocked engine, two different factorisations of the same K~ (the suite's 1e-8)."""
    n, block, gap = 100, 10, 2
    X, y, ell, sn, M = cv_problem(kind, n, 20240601)
    ells, sns = np.array([0.5, 1.0, 2.0]) * ell, np.array([1e-2, 1e-1])
    with S.GPR(kernel=kind) as gp:
        g = gp.cv_grid(X, y, ells, sns, block, gap=gap, M=M)
        assert g["nlpd"].shape == (3, 2) and g["sse"].shape == (3, 2)
        for a, e in enumerate(ells):
            for b, s_ in enumerate(sns):
                gp.fit(X, y, e, s_, M=M)
                one = gp.cv(block, gap)
                print(kind, a, b, abs(g["nlpd"][a, b] / one["nlpd"] - 1), abs(g["sse"][a, b] / one["sse"] - 1))
                assert abs(g["nlpd"][a, b] - one["nlpd"]) <= tol * abs(one["nlpd"]) and abs(g["sse"][a, b] - one["sse"]) <= tol * abs(one["sse"])


# ---- 8. the reference's own kernel at the reference's own size: every golden record x its stored theta, ONE launch ------------------------------
def test_small_batch_cv_all_golden_records_in_one_launch(S):
    """Against the block closed form on the oracle's K~; tolerance max(1e-8, 1e3 * 2.3e-16 * cond(K~)) as tests/test_hip_loo.py uses for
    quantities that go through the in-LDS inverse, relative for var, against max(1, |.|) for the scores and max(1, max|y|) for the means.
    (The closed form and real refits -- the two CPU routes -- agree to 4e-4 of that tolerance on these fits.)"""
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    assert len(recs) == 63
    shapes = [(5, 1), (8, 0)]
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
        res = {(shapes[0], "refit"): sb.run(cv=dict(block=shapes[0][0], gap=shapes[0][1], sigma_f="refit"))}
        assert gp.profile_get()["small"]["launches"] - launches0 == 1          # ONE launch for the lot
        for bg in shapes:
            for mode in ("refit", "fixed"):
                if (bg, mode) not in res:
                    res[(bg, mode)] = sb.run(cv=dict(block=bg[0], gap=bg[1], sigma_f=mode))
        plain1 = sb.run()
    assert set(plain0) == {"sigma_f", "nlml", "info", "sigma_n", "mean", "var"} and set(plain1) == set(plain0)
    for k in plain0:
        assert np.array_equal(plain0[k], plain1[k], equal_nan=True), k
    nmax = max(len(np.asarray(r["y"]).reshape(-1)) for r in recs)
    for got in res.values():
        assert got["cv_mean"].shape == (len(want), nmax) and got["cv_var"].shape == (len(want), nmax)
        assert set(got) == {"sigma_f", "nlml", "info", "sigma_n", "mean", "var", "cv_mean", "cv_var", "cv_nlpd", "cv_sse"}
    ninf, worst = 0, 0.0
    for i, (r, ell, sn, nl) in enumerate(want):
        y = np.asarray(r["y"], dtype=np.float64).reshape(-1)
        n = len(y)
        for got in res.values():
            assert np.all(np.isnan(got["cv_mean"][i, n:])) and np.all(np.isnan(got["cv_var"][i, n:]))
        if np.isinf(nl):              # the reference's except branch
            ninf += 1
            for got in res.values():
                assert got["info"][i] > 0 and np.isposinf(got["cv_nlpd"][i]) and np.isposinf(got["cv_sse"][i])
                assert np.all(np.isnan(got["cv_mean"][i])) and np.all(np.isnan(got["cv_var"][i]))
            continue
        Kt = O.fit_predict(r["X"], r["y"], r["Xs"], ell, sn, M=r["M"], ref_idiom=False)["K_tilde"]
        tol = max(1e-8, 1e3 * 2.3e-16 * np.linalg.cond(Kt))
        for (bg, mode), got in res.items():
            assert got["info"][i] == 0
            cf = cv_closed_form(Kt, y, bg[0], bg[1], mode)
            e = max(float(np.max(np.abs(got["cv_mean"][i, :n] - cf["mean"])) / max(1.0, np.max(np.abs(y)))), _relmax(got["cv_var"][i, :n], cf["var"]),
                    abs(got["cv_nlpd"][i] - cf["nlpd"]) / max(1.0, abs(cf["nlpd"])), abs(got["cv_sse"][i] - cf["sse"]) / max(1.0, abs(cf["sse"])))
            worst = max(worst, e / tol)
            assert e <= tol, (i, bg, mode, ell, sn, e, tol)
        for bg in shapes:
            assert np.array_equal(res[(bg, "refit")]["cv_mean"][i, :n], res[(bg, "fixed")]["cv_mean"][i, :n])
    print("worst error / tolerance over %d fits x %d settings: %.3g" % (len(want), len(res), worst))
    assert ninf == 63


# ---- 9. the retro grid search with a block cross-validated criterion ----------------------------------------------------------------------------
def test_retro_grid_search_block_criteria(S):
    from seaiceextentforecasting_amd.retro import _problem as retro_problem, _retro_inputs
    script = "north_September"
    g = load_golden(script + "_retro")
    fmin, fmax = g["args"]
    ells, sns = np.array([1e-3, 0.05, 1.0]), np.array([1e-2, 1.0, 1e2, 1e4])
    tab = S.SCRIPT_TABLE[script]
    ny = fmax - fmin + 1
    block, gap = 4, 1
    with S.GPR(kernel="netdiffusion") as gp:
        default = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp)
        nlml = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="nlml", block=block, gap=gap)
        nlpd = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="cv_nlpd", block=block, gap=gap)
        sse = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="cv_sse", block=block, gap=gap)
        sse5 = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="cv_sse")
        sb = S.SmallBatch(gp)
        for k, region in enumerate(tab["regions"]):
            for year in range(fmin, fmax + 1):
                _, y, sic, sst = _retro_inputs(tab, g["SIC"], g["SIEs_dt"], g["SST"], region, year, fmin)
                X, Xs, M = retro_problem(tab, k, y, sic, sst)
                ds = sb.add_dataset(X, y, None, M)
                for e in ells:
                    for s_ in sns:
                        sb.add_fit(ds, e, s_, expm="eigh")
        r = sb.run(cv=dict(block=block, gap=gap))
        r5 = sb.run(cv=dict(block=5, gap=0))
    assert set(default) == set(tab["regions"]) == set(nlml) == set(nlpd) == set(sse)
    shape = (len(tab["regions"]), ny, len(ells), len(sns))
    for k, region in enumerate(tab["regions"]):
        assert default[region].tobytes() == nlml[region].tobytes()
        assert nlpd[region].shape == shape[1:] and sse[region].shape == shape[1:]
        assert nlpd[region].tobytes() == np.ascontiguousarray(r["cv_nlpd"].reshape(shape)[k]).tobytes()
        assert sse[region].tobytes() == np.ascontiguousarray(r["cv_sse"].reshape(shape)[k]).tobytes()
        assert sse5[region].tobytes() == np.ascontiguousarray(r5["cv_sse"].reshape(shape)[k]).tobytes()      # the defaults: block = 5, gap = 0


# ---- 10. what has no block cross-validation -------------------------------------------------------------------------------------------------------
def test_cv_value_errors(S):
    X, y, ell, sn, _ = cv_problem("rbf", 40, 20240701)
    y = np.asarray(y).reshape(-1)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X[:1], y[:1], ell, sn)
        with pytest.raises(ValueError):
            gp.cv(1)                                     # n = 1
        gp.fit(X, y, ell, sn)
        for kw in (dict(block=100, gap=15), dict(block=129), dict(block=20, gap=20), dict(block=40)):      # window > 128; a fold that leaves no training row
            with pytest.raises(ValueError):
                gp.cv(**kw)
        # the library's own checks, behind the Python ones
        m, v, s2 = np.zeros(40), np.zeros(40), np.zeros(2)
        from seaiceextentforecasting_amd import _lib as L
        for block, gap in ((0, 0), (5, -1), (100, 15), (40, 0), (20, 20)):
            assert gp._lib.sigp_cv(gp._h, block, gap, 0, L.ptr(m), L.ptr(v), L.ptr(s2)) == L.BAD_ARG, (block, gap)
        assert gp._lib.sigp_cv(gp._h, 5, 0, 7, L.ptr(m), L.ptr(v), L.ptr(s2)) == L.BAD_ARG
        r = gp.cv(39)                                    # the widest block that still leaves a training row in every fold
        assert np.all(np.isfinite(r["mean"])) and np.all(r["var"] > 0)
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        X12, y12, _ = O.synthetic_problem(40, 12, 3)
        sb.add_fit(sb.add_dataset(X12, y12, None), 0.05, 1e-2)
        with pytest.raises(ValueError):
            sb.run(cv=dict(block=30, gap=2))            # window > 32 on the one-workgroup kernel
        sb.add_fit(sb.add_dataset(X12[:20], y12[:20], None), 0.05, 1e-2)
        with pytest.raises(ValueError):
            sb.run(cv=dict(block=20))                   # the second data set has 20 rows: its only fold leaves nothing to train on
        ok = sb.run(cv=dict(block=10, gap=5))
        assert np.all(ok["info"] == 0) and np.all(np.isfinite(ok["cv_nlpd"]))
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, ell, sn)
        with pytest.raises(ValueError, match="fp64"):
            gp.cv(5)
