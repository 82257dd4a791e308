"""GPU tier of the expanding-window hindcast validation (``GPR.hindcast`` / ``hindcast_batch`` / ``hindcast_grid``): against the closed form
that tests/test_hindcast_host.py pins to brute-force refits on every prefix, and against the engine's own ``GPR.fit`` refits on prefixes.
Errors are measured as tests/test_hip_loo.py measures them, at the suite's 1e-8, on matrices with cond(K~) <= 1e6."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from test_hindcast_host import _kt, hindcast_closed_form, scored_rows
from test_hip_loo import _check_loo, _cond, _problem

pytestmark = pytest.mark.gpu

MODES = ("refit", "fixed")


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
def _case(kind, n):
    X, y, ell, sn, M = _problem(kind, n, 20261600 + n)
    Kt = _kt(kind, X, ell, sn, M)
    return X, y, ell, sn, M, Kt


def _check(tag, r, y, cf):
    sc = cf["scored"]
    assert np.all(np.isnan(np.delete(r["mean"], sc))) and np.all(np.isnan(np.delete(r["var"], sc))), tag
    assert np.array_equal(np.arange(len(y))[r["scored"]], sc), tag
    sub = dict(mean=r["mean"][sc], var=r["var"][sc], nlpd=r["nlpd"], sse=r["sse"])
    _check_loo(tag, sub, y, cf["mean"][sc], cf["var"][sc], cf["nlpd"], cf["sse"])
    assert abs(r["mse"] - cf["sse"] / len(sc)) <= 1e-8 * cf["sse"] / len(sc)


def _settings(n):
    """(lead, min_train): lead in {1, 3, 128}, min_train in {1, 5, n - lead (a single scored row)}, where a row is scored"""
    out = []
    for lead in (1, 3, 128):
        for mt in (1, 5, n - lead):
            if mt >= 1 and mt + lead - 1 <= n - 1 and (lead, mt) not in out:
                out.append((lead, mt))
    return out


# ---- 1. values against the closed form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n", [2, 37, 128, 129, 300])
def test_hindcast_equals_the_closed_form(S, kind, n):
    X, y, ell, sn, M, Kt = _case(kind, n)
    assert _cond(Kt) <= 1e6
    settings = _settings(n)
    assert settings
    if n in (129, 300):
        assert (128, 1) in settings          # a lead that straddles the 128 boundary
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn)
        for lead, mt in settings:
            for mode in MODES:
                r = gp.hindcast(lead=lead, min_train=mt, sigma_f=mode)
                _check("%s n=%d lead=%d min_train=%d %s" % (kind, n, lead, mt, mode), r, y, hindcast_closed_form(Kt, y, lead, mt, mode))


def test_hindcast_reference_kernel(S):
    n = 37
    X, y, ell, sn, M, Kt = _case("netdiffusion", n)
    assert _cond(Kt) <= 1e6
    with S.GPR(kernel="netdiffusion") as gp:
        gp.fit(X, y, ell, sn, M=M)
        for lead, mt in ((1, 1), (3, 5)):
            for mode in MODES:
                _check("netdiffusion lead=%d %s" % (lead, mode), gp.hindcast(lead=lead, min_train=mt, sigma_f=mode), y, hindcast_closed_form(Kt, y, lead, mt, mode))
        r = gp.hindcast()                      # min_train=None: max(2, d + 1)
        assert r["scored"] == slice(max(2, X.shape[1] + 1), n)


def test_hindcast_equals_the_engines_own_refits_on_prefixes(S):
    n, lead, mt = 40, 3, 4
    X, y, ell, sn, _ = _problem("rbf", n, 20261701)
    sc = scored_rows(n, lead, mt)
    mean, var = np.zeros(n), np.zeros(n)
    with S.GPR(kernel="rbf") as gp:
        for t in sc:
            s = t - lead + 1
            gp.fit(X[:s], y[:s], ell, sn, Xs=X[t:t + 1])
            mu, v = gp.predict(X[t:t + 1])
            mean[t], var[t] = mu[0], v[0]
        gp.fit(X, y, ell, sn)
        rf, fx = gp.hindcast(lead=lead, min_train=mt), gp.hindcast(lead=lead, min_train=mt, sigma_f="fixed")
        sf = gp.sigma_f_
        Lt = gp.L_tilde_
    e_mean = float(np.max(np.abs(rf["mean"][sc] - mean[sc])) / np.max(np.abs(y)))
    e_var = float(np.max(np.abs(rf["var"][sc] / var[sc] - 1.0)))
    print("engine refits: mean %.3g var %.3g" % (e_mean, e_var))
    assert e_mean <= 1e-8 and e_var <= 1e-8
    assert _same_bits(rf["mean"], fx["mean"])                          # the means do not depend on the mode
    # FIXED: var_t = sigma_f w_t
    w = np.array([float(Lt[t, t - lead + 1:t + 1] @ Lt[t, t - lead + 1:t + 1]) for t in sc])
    assert float(np.max(np.abs(fx["var"][sc] / (sf * w) - 1.0))) <= 1e-13


def test_fixed_mode_variances_carry_the_fits_own_sigma_f_bits(S):
    """At lead = 1 the row segment is the one entry L~_tt, so w_t = L~_tt^2 is a single rounded product whatever the order of the sums, and
    var_t = sigma_f w_t must be the product of the fit's own sigma_f (``gp.sigma_f_``: the bits of the fit's epilogue) with it, bit for bit --
    a sigma_f recomputed on the device from another sum of z^2 would differ in the last bits on some row."""
    n = 300
    X, y, ell, sn, _ = _problem("rbf", n, 20261702)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X, y, ell, sn)
        fx = gp.hindcast(lead=1, min_train=1, sigma_f="fixed")
        sf, dg = gp.sigma_f_, np.diag(gp.L_tilde_).copy()
    assert _same_bits(fx["var"][1:], sf * (dg[1:] * dg[1:]))


# ---- 2. the fit is left alone; the same bits twice; accurate solves ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
def test_fit_is_only_read_and_hindcast_twice_gives_the_same_bits(S, kind):
    n = 300
    X, y, ell, sn, M = _problem(kind, n, 20261801)
    Xs = O.synthetic_problem(5, X.shape[1], 78)[0]
    with S.GPR(kernel=kind) as gp:
        gp.fit(X, y, ell, sn, M=M)
        mu0, var0 = gp.predict(Xs)
        a0, loo0, cv0 = gp.alpha_.copy(), gp.loo(), gp.cv(5, 1)
        r1 = gp.hindcast(lead=3, min_train=5)
        r2 = gp.hindcast(lead=3, min_train=5)
        mu1, var1 = gp.predict(Xs)
        a1, loo1, cv1 = gp.alpha_.copy(), gp.loo(), gp.cv(5, 1)
        r3 = gp.hindcast(lead=3, min_train=5)
    for k in ("mean", "var"):
        assert _same_bits(r1[k], r2[k]) and _same_bits(r1[k], r3[k])
        assert _same_bits(loo0[k], loo1[k]) and _same_bits(cv0[k], cv1[k])
    assert r1["nlpd"] == r2["nlpd"] == r3["nlpd"] and r1["sse"] == r2["sse"] == r3["sse"]
    assert _same_bits(mu0, mu1) and _same_bits(var0, var1) and _same_bits(a0, a1)
    assert loo0["nlpd"] == loo1["nlpd"] and cv0["nlpd"] == cv1["nlpd"]


def test_hindcast_with_accurate_solves(S):
    n = 300
    X, y, ell, sn, M, Kt = _case("rbf", n)
    with S.GPR(kernel="rbf", accurate=True) as gp:
        gp.fit(X, y, ell, sn)
        r = gp.hindcast(lead=3, min_train=5)
    _check("accurate", r, y, hindcast_closed_form(Kt, y, 3, 5, "refit"))


# ---- 3. lockstep groups ------------------------------------------------------------------------------------------------------------------
def test_hindcast_batch_equals_the_single_fits(S):
    n, d, lead, mt = 200, 8, 3, 5
    X, y, _ = O.synthetic_problem(n, d, 20261901)
    ells = np.sqrt(8.0) * np.array([0.7, 1.0, 1.3, 1.6, 2.0])
    sns = np.array([1e-2, 2e-2, 1e-2, 5e-2, 1e-1])
    with S.GPR(kernel="rbf") as gp:
        single = []
        for e, s_ in zip(ells, sns):
            gp.fit(X, y, e, s_)
            single.append({m: gp.hindcast(lead=lead, min_train=mt, sigma_f=m) for m in MODES})
        gp.upload_batch(X, y, None, group=8)
        first = None
        for group in (1, 2, 8):
            for m in MODES:
                r = gp.hindcast_batch(ells, sns, lead=lead, min_train=mt, sigma_f=m, group=group)
                sc = scored_rows(n, lead, mt)
                for i in range(5):
                    assert np.all(np.isnan(np.delete(r["mean"][i], sc)))
                    assert np.max(np.abs(r["mean"][i][sc] - single[i][m]["mean"][sc])) <= 1e-12 * np.max(np.abs(y))
                    assert np.max(np.abs(r["var"][i][sc] / single[i][m]["var"][sc] - 1.0)) <= 1e-12
                    assert abs(r["nlpd"][i] - single[i][m]["nlpd"]) <= 1e-12 * max(1.0, abs(single[i][m]["nlpd"]), len(sc))
                    assert abs(r["sse"][i] - single[i][m]["sse"]) <= 1e-12 * single[i][m]["sse"]
            if first is None:
                first = r
        g = gp.hindcast_grid(X, y, ells[:2], sns[:3], lead=lead, min_train=mt)
        assert g["nlpd"].shape == (2, 3) and np.all(np.isfinite(g["nlpd"]))
        assert abs(g["nlpd"][1, 0] - gp.hindcast_batch(ells[1:2], sns[:1], lead=lead, min_train=mt, predictions=False)["nlpd"][0]) == 0.0


def test_hindcast_batch_non_spd_member_gets_inf_and_its_mates_keep_their_bits(S):
    n, d = 150, 4
    X, y, _ = O.synthetic_problem(n, d, 20261902)
    X[1] = X[0]                                     # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    ells, good, bad = np.full(3, 2.0), np.array([1e-2, 1e-2, 2e-2]), np.array([1e-2, 0.0, 2e-2])
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(X, y, None, group=8)
        a = gp.hindcast_batch(ells, good, lead=2, min_train=3, group=8)
        b = gp.hindcast_batch(ells, bad, lead=2, min_train=3, group=8)
    assert np.isposinf(b["nlpd"][1]) and np.isposinf(b["sse"][1]) and np.all(np.isnan(b["mean"][1])) and np.all(np.isnan(b["var"][1]))
    for i in (0, 2):
        assert a["nlpd"][i] == b["nlpd"][i] and a["sse"][i] == b["sse"][i]
        assert _same_bits(a["mean"][i], b["mean"][i]) and _same_bits(a["var"][i], b["var"][i])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_handle_usable(S, L):
    n = 37
    X, y, ell, sn, M, Kt = _case("rbf", n)
    lib = L.load()
    mean, var, score = np.zeros(n), np.zeros(n), np.zeros(2)
    p = L.ptr
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        assert lib.sigp_hindcast(gp._h, 1, 1, 0, p(mean), p(var), p(score)) == L.BAD_ARG          # not fitted
        gp.fit(X, y, ell, sn)
        ok = gp.hindcast(lead=1, min_train=1)
        for lead, mt, mode in ((0, 1, 0), (129, 1, 0), (1, 0, 0), (1, n, 0), (30, 8, 0), (1, 1, 2), (1, 1, -1)):
            assert lib.sigp_hindcast(gp._h, lead, mt, mode, p(mean), p(var), p(score)) == L.BAD_ARG, (lead, mt, mode)
            again = gp.hindcast(lead=1, min_train=1)
            assert _same_bits(ok["mean"], again["mean"]) and ok["nlpd"] == again["nlpd"]
        assert lib.sigp_hindcast(gp._h, 1, 1, 0, None, p(var), p(score)) == L.BAD_ARG
        for kw in (dict(lead=0), dict(lead=129), dict(min_train=0), dict(min_train=n), dict(sigma_f="loo")):
            with pytest.raises(ValueError):
                gp.hindcast(**kw)
        assert gp.hindcast(lead=n - 1, min_train=1)["scored"] == slice(n - 1, n)     # a single scored row
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(X, y, ell, sn)
        assert lib.sigp_hindcast(gp._h, 1, 1, 0, p(mean), p(var), p(score)) == L.BAD_ARG           # fp32 handle
        mu, _ = gp.predict(X[:2])
        assert np.all(np.isfinite(mu))
    with S.DistributedGPR("rbf", 0, 1, None, device=0, outer_blocks=8) as dg:                       # a sharded fit (one rank) leaves no single-GPU factor
        dg.fit(X, y, ell, sn)
        mu0, _ = dg.predict(X[:2])
        assert lib.sigp_hindcast(dg.gp._h, 1, 1, 0, p(mean), p(var), p(score)) == L.BAD_ARG
        mu1, _ = dg.predict(X[:2])
        assert _same_bits(mu0, mu1)


# ---- 5. the one-workgroup kernel ----------------------------------------------------------------------------------------------------------
def _retro_records(S, script, picks):
    from seaiceextentforecasting_amd.retro import _problem as retro_problem, _retro_inputs
    g = load_golden(script + "_retro")
    fmin, fmax = g["args"]
    tab = S.SCRIPT_TABLE[script]
    out = []
    for k, year in picks(len(tab["regions"]), fmin, fmax):
        _, y, sic, sst = _retro_inputs(tab, g["SIC"], g["SIEs_dt"], g["SST"], tab["regions"][k], year, fmin)
        X, Xs, M = retro_problem(tab, k, y, sic, sst)
        out.append((np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), M))
    return g, tab, fmin, fmax, out


def test_small_hindcast_equals_the_blocked_engine_on_golden_retro_records(S):
    """Two (region, year) records of the golden retro loop x 3 x 2 grid points, both sigma modes: the one-workgroup flavour against
    ``GPR.fit`` + ``GPR.hindcast`` on the same data at the suite's 1e-8; NaN where a row is not scored and beyond a record's n."""
    _, _, _, _, recs = _retro_records(S, "north_September", lambda R, fmin, fmax: [(0, fmin), (R - 1, fmax)])
    ells, sns, lead, mt = (1e-3, 0.05, 1.0), (1.0, 1e2), 2, 3
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        want = []
        for X, y, M in recs:
            ds = sb.add_dataset(X, y, None, M)
            for e in ells:
                for s_ in sns:
                    sb.add_fit(ds, e, s_, expm="pade")
                    want.append((X, y, M, e, s_))
        plain0 = sb.run()
        gp.profile(True, ["small"])
        l0 = gp.profile_get()["small"]["launches"]
        got = {m: sb.run(hindcast=dict(lead=lead, min_train=mt, sigma_f=m)) for m in MODES}
        assert gp.profile_get()["small"]["launches"] - l0 == 2                # ONE launch per call for the lot
        gp.profile(False)
        plain1 = sb.run()
        for k in plain0:
            assert np.array_equal(plain0[k], plain1[k], equal_nan=True), k
        for kw in (dict(grad=True), dict(loo="refit"), dict(cv=dict(block=2))):
            with pytest.raises(ValueError, match="separately"):
                sb.run(hindcast=dict(lead=1), **kw)
        for bad in (dict(lead=0), dict(lead=33), dict(min_train=0), dict(min_train=10 ** 6), dict(sigma_f="loo"), dict(block=2), "refit"):
            with pytest.raises(ValueError):
                sb.run(hindcast=bad)
        nmax = max(len(y) for _, y, _ in recs)
        worst = 0.0
        for i, (X, y, M, e, s_) in enumerate(want):
            n = len(y)
            gp.fit(X, y, e, s_, M=M)
            for m in MODES:
                ref = gp.hindcast(lead=lead, min_train=mt, sigma_f=m)
                r = got[m]
                assert r["hindcast_mean"].shape == (len(want), nmax) and r["info"][i] == 0
                assert np.all(np.isnan(r["hindcast_mean"][i, n:])) and np.all(np.isnan(r["hindcast_var"][i, n:]))
                sc = np.arange(n)[ref["scored"]]
                assert np.all(np.isnan(np.delete(r["hindcast_mean"][i, :n], sc))) and np.all(np.isnan(np.delete(r["hindcast_var"][i, :n], sc)))
                sub = dict(mean=r["hindcast_mean"][i, sc], var=r["hindcast_var"][i, sc], nlpd=r["hindcast_nlpd"][i], sse=r["hindcast_sse"][i])
                _check_loo("small record %d l=%g sn=%g %s" % (i // 6, e, s_, m), sub, y, ref["mean"][sc], ref["var"][sc], ref["nlpd"], ref["sse"])
            assert abs(got["refit"]["nlml"][i] - gp.nlml_) <= 1e-8 * abs(gp.nlml_)
        g = gp.hindcast_grid(recs[0][0], recs[0][1], ells, sns, lead=lead, min_train=mt, M=recs[0][2])
        assert g["nlpd"].shape == (3, 2)


def test_retro_grid_search_hindcast_entry_equals_a_host_loop_of_refits(S):
    """One table entry of ``retro_grid_search(criterion="hindcast_nlpd")`` against the loop it replaces: for every origin a real fit on the
    years before it and a forecast of the target year, features, standardisation and M held."""
    script, lead, mt = "north_September", 1, 2
    ells, sns = np.array([0.05, 1.0]), np.array([1.0, 1e2])
    g, tab, fmin, fmax, recs = _retro_records(S, script, lambda R, fmin, fmax: [(0, fmax)])
    X, y, M = recs[0]
    n = len(y)
    with S.GPR(kernel="netdiffusion", expm="eigh") as gp:
        nlpd = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="hindcast_nlpd", lead=lead, min_train=mt)
        sse = S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion="hindcast_sse", lead=lead, min_train=mt)
        ny = fmax - fmin + 1
        assert set(nlpd) == set(tab["regions"]) and nlpd[tab["regions"][0]].shape == (ny, 2, 2)
        tn = ts = 0.0
        for t in scored_rows(n, lead, mt):
            s = t - lead + 1
            gp.fit(X[:s], y[:s], ells[0], sns[1], M=M, Xs=X[t:t + 1])
            mu, v = gp.predict(X[t:t + 1])
            r = y[t] - mu[0]
            tn += 0.5 * np.log(2 * np.pi * v[0]) + r * r / (2 * v[0])
            ts += r * r
    a, b = nlpd[tab["regions"][0]][ny - 1, 0, 1], sse[tab["regions"][0]][ny - 1, 0, 1]
    print("retro entry: nlpd %.12g (host loop %.12g), sse %.12g (host loop %.12g)" % (a, tn, b, ts))
    assert abs(a - tn) <= 1e-8 * max(1.0, abs(tn)) and abs(b - ts) <= 1e-8 * ts
    with pytest.raises(ValueError):
        S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], criterion="hindcast")
