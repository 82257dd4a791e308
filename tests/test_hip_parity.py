"""GPU tier: the HIP engine (through the C ABI, libsigp.so) against the oracle on identical inputs.

Tolerances (fp64):
  kernel matrix K~            <= 1e-13 relative (max-norm)         SURVEY.md 7 step 3
  Cholesky factor L~          <= 1e-11 relative, ||LL^T-K||/||K|| <= 1e-13*sqrt(n) here (easy matrices); the tight form,
                              ||LL^T-K||_F/||K||_F <= 16 max(LAPACK's own, 2^-53) with the product in long double (LAPACK: 2-6e-16),
                              at cond(K~) up to 1e14, is asserted in tests/test_hip_conditioning.py
  predictions (mean, var)     <= 1e-8 relative                      BASELINE.json north_star
  sigma_f, nlML               <= 1e-9 relative
"""
import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

TOL_PRED = 1e-8


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n", [1, 7, 64, 128, 129, 257, 1024])
def test_build_factor_fit_predict(S, kind, n):
    """Every stage of one fit against the oracle, including non-multiple-of-tile sizes and n=1."""
    if kind == "netdiffusion" and n < 7:
        pytest.skip("cov() of a single row is undefined")
    d = 4 if n < 64 else 8
    X, y, Xs = O.synthetic_problem(n, d, 1000 + n, m=3)
    ell, sn = (np.sqrt(d), 1e-2) if kind != "netdiffusion" else (0.05, 1e-2)
    ref = O.fit_predict(X, y, Xs, ell, sn, kind=kind, ref_idiom=False)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y, Xs=Xs)
        K = gp.kernel_matrix(ell, sn)
        assert rel(K, np.tril(ref["K_tilde"])) <= 1e-13
        gp.refit(ell, sn)
        L = gp.L_tilde_
        assert rel(L, ref["L_tilde"]) <= 1e-11
        assert np.linalg.norm(L @ L.T - ref["K_tilde"]) / np.linalg.norm(ref["K_tilde"]) <= 1e-13 * np.sqrt(max(n, 4))
        assert rel(gp.sigma_f_, ref["sigma_f"]) <= 1e-9
        assert rel(gp.nlml_, ref["nlml"]) <= 1e-9
        mu, var = gp.predict(Xs)                     # ride-along rows
        assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED
        Xs2 = np.random.default_rng(n).standard_normal((5, d))
        ref2 = O.fit_predict(X, y, Xs2, ell, sn, kind=kind, M=ref["M"], ref_idiom=False)
        mu2, var2 = gp.predict(Xs2)                  # general path: cross-kernel build + forward block solve
        assert rel(mu2, ref2["fmean"]) <= TOL_PRED and rel(var2, ref2["fvar"]) <= TOL_PRED
        assert rel(gp.alpha_, ref["alpha"]) <= 1e-8
        assert rel(gp.L_, ref["L"]) <= 1e-11


def test_reference_idiom_agreement_config1(S):
    """BASELINE configs[0] (n=64, d=4 RBF) against the reference's call sequence (two Cholesky, gesv solves)."""
    X, y, Xs = O.synthetic_problem(64, 4, 20240000, m=1)
    ref = O.fit_predict(X, y, Xs, 2.0, 1e-2, kind="rbf", ref_idiom=True)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X, y, 2.0, 1e-2, Xs=Xs)
        mu, var = gp.predict(Xs)
    assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED
    assert rel(gp.sigma_n_, ref["sigma_n"]) <= 1e-9


def test_many_test_points_general_path(S):
    """m > 127 cannot ride along: predict() chunks through the forward block solve."""
    X, y, Xs = O.synthetic_problem(300, 8, 5, m=200)
    ref = O.fit_predict(X, y, Xs, np.sqrt(8.0), 1e-2, kind="matern52", ref_idiom=False)
    with S.GPR(kernel="matern52") as gp:
        gp.fit(X, y, np.sqrt(8.0), 1e-2, Xs=Xs)
        mu, var = gp.predict(Xs)
    assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED


def test_golden_scripts_through_the_engine(S, golden):
    """The reference's 14 forecast scripts: host loop of retro.py + HIP engine vs captures of the reference."""
    g = golden
    script = g["script"].replace("_retro", "")
    with S.GPR(kernel="netdiffusion") as gp:
        if g["kind"] == "retro":
            out = S.retro_forecast(script, g["SIC"], g["SIEs_dt"], g["SIEs_trend"], g["args"][0], g["args"][1], SST=g["SST"], gp=gp)
            for key, val in g["GPR"].items():
                # values are rounded to 3 decimals by the reference; allow one unit in the last place for
                # results that sit within 1e-8 of a rounding boundary
                assert np.max(np.abs(out[key] - val)) <= 1.0000001e-3, key
                assert np.mean(out[key] == val) >= 0.9, key
        else:
            SIC = {"anoms": g["SIC"]["anoms"]}
            SST = {"anoms": g["SST"]["anoms"]} if g["SST"] else None
            out = S.operational_forecast(script, SIC, g["SIEs_dt"], g["SIEs_trend"], g["args"][0], SST=SST, gp=gp)
            regs = S.SCRIPT_TABLE[script]["regions"]
            for r in g["records"]:
                o = out[regs[int(r["k"])]]
                kss = float(r["KXsXs"][0][0])
                assert abs(o["fmean"] - r["fmean"]) <= TOL_PRED * max(abs(float(r["fmean"])), np.abs(r["KXXs"]).max() * np.abs(r["alpha"]).max())
                assert abs(o["fvar"] - r["fvar"]) <= TOL_PRED * kss
                assert abs(o["fmean_rt"] - r["fmean_rt"]) <= TOL_PRED * abs(float(r["fmean_rt"]))


def test_golden_intermediates(S, golden):
    """L, alpha, sigma_f of the engine against the reference's captured locals (every region/year record)."""
    for r in golden["records"]:
        X, y, Xs, M = r["X"], r["y"], r["Xs"], r["M"]
        with S.GPR(kernel="netdiffusion") as gp:
            gp.fit(X, y, float(r["ell"]), float(r["sn_tilde"]), M=M, Xs=Xs)
            cond = np.linalg.cond(r["L_tilde"]) ** 2
            tol = max(1e-10, 100 * cond * 2.3e-16)
            assert rel(gp.sigma_f_, r["sigma_f"]) <= tol
            assert rel(gp.L_, r["L"]) <= max(1e-10, tol)
            assert rel(gp.alpha_, r["alpha"]) <= tol
            # nlML (north/June1st.py:246) evaluated on the reference's own captured L and alpha at the script's l
            # (mlii_nlml[0] is at exp(log l): for l = 3.1e10 that 1-ulp change moves expm(l M) by ~1e-6)
            n = r["y"].shape[0]
            nl_ref = float((r["y"].T @ r["alpha"])[0, 0]) / 2 + np.log(np.diag(r["L"])).sum() + n * np.log(2 * np.pi) / 2
            assert abs(gp.nlml_ - nl_ref) <= 1e-9 * abs(nl_ref)


def test_mlii_contract_against_reference_closure(S, golden):
    """gp.nlml(theta, grad='ref') == the reference's live MLII closure: value, its 2-vector "gradient"
    (north/June1st.py:248-252) and the except-branch -> (inf, [inf, inf])."""
    for r in golden["records"]:                     # every captured (region, year): the fits are of order <= 45
        with S.GPR(kernel="netdiffusion") as gp:
            gp.set_data(r["X"], r["y"], M=r["M"])
            cond = np.linalg.cond(r["L_tilde"]) ** 2
            for th, nl, gr in zip(r["mlii_theta"], r["mlii_nlml"], r["mlii_grad"]):
                val, grad = gp.nlml(th, grad="ref")
                if np.isinf(nl):
                    assert np.isinf(val) and np.all(np.isinf(grad))
                    continue
                if np.exp(th[0]) > 1e6:
                    continue      # l = 3.1e10: expm(l M) moves by ~1e-6 under 1-ulp changes of l
                assert abs(val - nl) <= 1e-9 * abs(nl)
                # the reference sums tr(solve(L.T, solve(L, dK))) in LU arithmetic: both sides carry cond(K)*eps
                tol = max(1e-7, 1e3 * 2.3e-16 * np.linalg.cond(O.fit_predict(r["X"], r["y"], r["Xs"], float(np.exp(th[0])), float(np.exp(th[1])), M=r["M"], ref_idiom=False)["K_tilde"]))
                assert np.max(np.abs(grad - gr)) <= tol * max(1.0, np.max(np.abs(gr))), (th, grad, gr)
            del cond


@pytest.mark.parametrize("kind", ["netdiffusion", "rbf", "matern52"])
def test_exact_gradient_matches_oracle_and_finite_differences(S, kind):
    rng = np.random.default_rng(5)
    n, N = 150, 6
    X = rng.standard_normal((n, N))
    y = X @ rng.standard_normal(N) + 0.3 * rng.standard_normal(n)
    th = {"netdiffusion": np.array([np.log(0.14), np.log(6.1)]), "rbf": np.array([0.5, -1.0]), "matern52": np.array([0.8, -0.5])}[kind]
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        f0, g0 = gp.nlml(th, grad="exact")
        fo, go = O.mlii(th, X, y, kind=kind, grad="exact")
        assert abs(f0 - fo) <= 1e-9 * abs(fo)
        assert np.allclose(g0, go, rtol=1e-7, atol=1e-9), (g0, go)
        h = 1e-5
        fd = np.array([(gp.nlml(th + h * e, grad=None)[0] - gp.nlml(th - h * e, grad=None)[0]) / (2 * h) for e in np.eye(2)])
        assert np.allclose(g0, fd, rtol=1e-5, atol=1e-6), (g0, fd)
        if kind != "netdiffusion":
            with pytest.raises(ValueError):
                gp.nlml(th, grad="ref")


def test_exact_gradient_n1024(S):
    """K13/K14 at a multi-block size: lockstep forward solve of the identity (8 chunks) + SYRK."""
    X, y, _ = O.synthetic_problem(1024, 8, 42, m=1)
    th = np.array([np.log(np.sqrt(8.0)), np.log(1e-2)])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        f0, g0 = gp.nlml(th, grad="exact")
    fo, go = O.mlii(th, X, y, kind="rbf", grad="exact")
    assert abs(f0 - fo) <= 1e-9 * abs(fo) and np.allclose(g0, go, rtol=1e-7, atol=1e-8), (g0, go)


def test_not_spd_raises_linalgerror_with_pivot(S):
    """Non-SPD K~: fit raises np.linalg.LinAlgError (as north/June1st.py:265 does) carrying LAPACK's info."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 3))
    X[150:190] = X[20:60]                 # duplicate points, sn = 0 -> exactly singular (40 pivots that round to ~ +-1e-16)
    y = rng.standard_normal(200)
    with S.GPR(kernel="rbf") as gp:
        with pytest.raises(np.linalg.LinAlgError) as ei:
            gp.fit(X, y, 1.0, 0.0)
        assert 1 <= ei.value.info <= 200
        gp.fit(X, y, 1.0, 1e-3)           # the handle stays usable
        assert np.isfinite(gp.nlml_)
    with pytest.raises(ValueError):
        S.GPR(kernel="rbf").fit(X, y, -1.0, 1e-2)


def test_batch_equals_sequential_and_oracle(S):
    """fit_batch (lockstep groups, several groups in flight) == one-at-a-time fits == oracle."""
    n, d, B, F = 520, 8, 5, 13
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n)); Xsb = np.zeros((B, 2, d))
    for b in range(B):
        Xb[b], yb[b], Xsb[b] = O.synthetic_problem(n, d, 300 + b, m=2)
    ell = np.sqrt(d) * np.logspace(-0.3, 0.3, F)
    sn = np.logspace(-2.5, -1, F)
    with S.GPR(kernel="rbf") as gp:
        for group, conc in ((4, 2), (1, 3), (16, 1)):
            r = gp.fit_batch(Xb, yb, Xsb, ell, sn, concurrency=conc, group=group)
            assert np.all(r["info"] == 0)
            for i in range(F):
                b = i % B
                ref = O.fit_predict(Xb[b], yb[b], Xsb[b], ell[i], sn[i], kind="rbf", ref_idiom=False)
                assert rel(r["mean"][i], ref["fmean"]) <= TOL_PRED and rel(r["var"][i], ref["fvar"]) <= TOL_PRED
                assert rel(r["nlml"][i], ref["nlml"]) <= 1e-9 and rel(r["sigma_f"][i], ref["sigma_f"]) <= 1e-9
        gp.fit(Xb[1], yb[1], ell[1], sn[1], Xs=Xsb[1])
        mu, var = gp.predict(Xsb[1])
        assert rel(mu, r["mean"][1]) <= 1e-12 and rel(var, r["var"][1]) <= 1e-12   # lockstep == single, bit for bit up to rounding


def test_batch_isolates_a_failing_member(S):
    """One non-SPD member of a lockstep group reports its own info; the others are unaffected."""
    n, d = 260, 4
    X, y, Xs = O.synthetic_problem(n, d, 9, m=1)
    Xbad = X.copy(); Xbad[200:250] = Xbad[10:60]      # 50 exactly singular directions with sn = 0: some pivot rounds <= 0
    Xb = np.stack([X, Xbad, X]); yb = np.stack([y, y, y]); Xsb = np.stack([Xs, Xs, Xs])
    with S.GPR(kernel="rbf") as gp:
        r = gp.fit_batch(Xb, yb, Xsb, [2.0, 2.0, 2.0], [1e-2, 0.0, 1e-2], concurrency=1, group=4)
    assert r["info"][0] == 0 and r["info"][2] == 0 and r["info"][1] > 0
    assert np.isinf(r["nlml"][1]) and np.isnan(r["mean"][1]).all()
    ref = O.fit_predict(X, y, Xs, 2.0, 1e-2, kind="rbf", ref_idiom=False)
    assert rel(r["mean"][0], ref["fmean"]) <= TOL_PRED and rel(r["mean"][2], ref["fmean"]) <= TOL_PRED


def test_nlml_grid_matches_oracle(S):
    X, y, _ = O.synthetic_problem(300, 4, 77, m=1)
    ells = 2.0 * np.logspace(-0.5, 0.5, 3)
    sns = np.logspace(-2, 0, 4)
    with S.GPR(kernel="rbf") as gp:
        G = gp.nlml_grid(X, y, ells, sns, concurrency=2, group=4)
    for i, e in enumerate(ells):
        for j, s_ in enumerate(sns):
            nl, _ = O.mlii(np.log([e, s_]), X, y, kind="rbf", grad="exact")
            assert abs(G[i, j] - float(nl)) <= 1e-9 * abs(float(nl))


@pytest.mark.parametrize("opts", [dict(outer_blocks=1, lookahead=0), dict(outer_blocks=2, lookahead=1),
                                  dict(outer_blocks=5, lookahead=1), dict(outer_blocks=16, lookahead=1),
                                  dict(outer_blocks=2, lookahead=1, schedule="left"), dict(outer_blocks=2, lookahead=0, schedule="left"),
                                  dict(outer_blocks=1, lookahead=1, schedule="left"), dict(outer_blocks=3, lookahead=1, schedule="left")])
def test_blocking_options_do_not_change_results(S, opts):
    """Panel width / look-ahead only reorder launches: the factor is bitwise the same (fp64 sums in the same k order)."""
    X, y, Xs = O.synthetic_problem(1100, 8, 123, m=2)
    with S.GPR(kernel="rbf") as g0, S.GPR(kernel="rbf", **opts) as g1:
        g0.fit(X, y, np.sqrt(8.0), 1e-2, Xs=Xs)
        g1.fit(X, y, np.sqrt(8.0), 1e-2, Xs=Xs)
        assert np.array_equal(g0.L_tilde_, g1.L_tilde_)
        assert g0.nlml_ == g1.nlml_


@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
@pytest.mark.parametrize("n,W", [(257, 2), (1100, 2), (1100, 4), (2100, 8), (1300, 16), (900, 3)])
def test_strip_panel_mode_matches_oracle(S, kind, n, W):
    """panel_mode='strips' (top block by recursion, the rows below by panel_strip_kernel with pre-multiplied inverse
    blocks) is a different association of the same block forward substitution: same tolerances as the default path,
    and bit-identical with itself across look-ahead on/off."""
    d = 8
    X, y, Xs = O.synthetic_problem(n, d, 900 + n + W, m=3)
    ell, sn = (np.sqrt(d), 1e-2) if kind == "rbf" else (0.05, 1e-2)
    ref = O.fit_predict(X, y, Xs, ell, sn, kind=kind, ref_idiom=False)
    Ls = []
    for la in (1, 0):
        with S.GPR(kernel=kind, outer_blocks=W, lookahead=la, panel_mode="strips") as gp:
            gp.fit(X, y, ell, sn, M=ref["M"], Xs=Xs)
            mu, var = gp.predict(Xs)
            L = gp.L_tilde_
            assert rel(L, ref["L_tilde"]) <= 1e-11 and rel(gp.nlml_, ref["nlml"]) <= 1e-9
            assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED
            assert rel(gp.alpha_, ref["alpha"]) <= 1e-8
            Ls.append(L)
    assert np.array_equal(Ls[0], Ls[1])


@pytest.mark.parametrize("seed", range(8))
def test_strip_vs_recursive_random_shapes(S, seed):
    """Random (n, d, m, W, group) -- strips forced -- against the recursive path on the same lockstep batch."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(130, 2600)); d = int(rng.integers(1, 20)); m = int(rng.integers(0, 6))
    W = int(rng.choice([2, 3, 4, 6, 8, 16])); B = int(rng.integers(1, 5))
    kind = ["rbf", "matern52"][seed % 2]
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n)); Xsb = np.zeros((B, max(m, 1), d))
    for b in range(B):
        Xb[b], yb[b], Xsb[b] = O.synthetic_problem(n, d, 100 * seed + b, m=max(m, 1))
    Xs_arg = Xsb[:, :m] if m > 0 else None
    ell = np.sqrt(d) * rng.uniform(0.5, 2.0, B); sn = 10.0 ** rng.uniform(-3, 0, B)
    res = {}
    for mode in ("recursive", "strips"):
        with S.GPR(kernel=kind, outer_blocks=W, panel_mode=mode) as gp:
            res[mode] = gp.fit_batch(Xb, yb, Xs_arg, ell, sn, concurrency=1, group=B)
    a, b_ = res["recursive"], res["strips"]
    assert np.all(a["info"] == 0) and np.all(b_["info"] == 0)
    assert rel(b_["nlml"], a["nlml"]) <= 1e-10 and rel(b_["sigma_f"], a["sigma_f"]) <= 1e-10
    if m > 0:
        assert rel(b_["mean"], a["mean"]) <= TOL_PRED and rel(b_["var"], a["var"]) <= TOL_PRED


def test_strip_panel_mode_batch_and_failure(S):
    """Lockstep batch in strips mode == sequential default-mode fits to parity tolerance; a non-SPD member reports its pivot."""
    n, d, B = 700, 6, 5
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n)); Xsb = np.zeros((B, 2, d))
    for b in range(B):
        Xb[b], yb[b], Xsb[b] = O.synthetic_problem(n, d, 31 + b, m=2)
    Xb[3, 300:350] = Xb[3, 100:150]
    ell = np.full(B, 2.0); sn = np.array([1e-2, 1e-1, 1e-3, 0.0, 1e-2])
    with S.GPR(kernel="rbf", outer_blocks=2, panel_mode="strips") as gp:
        r = gp.fit_batch(Xb, yb, Xsb, ell, sn, concurrency=1, group=5)
    assert r["info"][3] > 300 and np.all(np.delete(r["info"], 3) == 0)
    for b in (0, 1, 2, 4):
        ref = O.fit_predict(Xb[b], yb[b], Xsb[b], ell[b], sn[b], kind="rbf", ref_idiom=False)
        assert rel(r["mean"][b], ref["fmean"]) <= TOL_PRED and rel(r["var"][b], ref["fvar"]) <= TOL_PRED
        assert rel(r["nlml"][b], ref["nlml"]) <= 1e-9


def test_shared_eigendecomposition_for_the_reference_kernel(S):
    """GPR(expm='eigh') (one eigh of M per data set) gives the same nlML / gradients / predictions as the
    per-call Pade expm path over an l grid."""
    X, y, Xs = O.synthetic_problem(300, 10, 5150, m=2)
    with S.GPR(kernel="netdiffusion") as g0, S.GPR(kernel="netdiffusion", expm="eigh") as g1:
        g0.set_data(X, y, Xs=Xs); g1.set_data(X, y, Xs=Xs)
        for ell in (1e-3, 0.05, 1.0, 20.0):
            for grad in ("ref", "exact"):
                th = np.log([ell, 1e-2])
                v0, d0 = g0.nlml(th, grad=grad)
                v1, d1 = g1.nlml(th, grad=grad)
                assert abs(v0 - v1) <= 1e-9 * abs(v0) and np.max(np.abs(d0 - d1)) <= 1e-7 * max(np.max(np.abs(d0)), 1e-12)
            g0.refit(ell, 1e-2); g1.refit(ell, 1e-2)
            (m0, s0), (m1, s1) = g0.predict(Xs), g1.predict(Xs)
            assert rel(m1, m0) <= TOL_PRED and rel(s1, s0) <= TOL_PRED


def test_full_size_properties_n4096(S):
    """BASELINE configs[1] (n=4096, d=8 RBF): oracle comparison + size-independent identities."""
    n, d = 4096, 8
    X, y, Xs = O.synthetic_problem(n, d, 20240001, m=4)
    ell, sn = np.sqrt(d), 1e-2
    ref = O.fit_predict(X, y, Xs, ell, sn, kind="rbf", ref_idiom=False)
    with S.GPR(kernel="rbf") as gp:
        gp.fit(X, y, ell, sn, Xs=Xs)
        mu, var = gp.predict(Xs)
        assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED
        assert rel(gp.nlml_, ref["nlml"]) <= 1e-9
        a = gp.alpha_
        assert abs(float(y @ a[:, 0]) - n) <= 1e-8 * n                    # y^T alpha = n  
        L = gp.L_tilde_
        K = ref["K_tilde"]
        assert np.linalg.norm(L @ L.T - K) / np.linalg.norm(K) <= 1e-13 * np.sqrt(n)
        assert np.all(var > 0)


def test_full_size_properties_n8192_batch(S):
    """BASELINE configs[2] shape (n=8192, d=8, batch of years x grid points) through size-independent
    properties: y^T alpha~ = n sigma_f, K~ alpha~ = y (residual), lockstep == single fit, var > 0."""
    n, d, B = 8192, 8, 2
    Xb = np.zeros((B, n, d)); yb = np.zeros((B, n)); Xsb = np.zeros((B, 1, d))
    for b in range(B):
        Xb[b], yb[b], Xsb[b] = O.synthetic_problem(n, d, 20240002 + b, m=1)
    ell = np.array([np.sqrt(d), 1.5 * np.sqrt(d), np.sqrt(d)])
    sn = np.array([1e-2, 1e-1, 1e-2])
    with S.GPR(kernel="rbf") as gp:
        r = gp.fit_batch(Xb, yb, Xsb, ell, sn, concurrency=1, group=4)
        assert np.all(r["info"] == 0) and np.all(r["var"] > 0) and np.all(np.isfinite(r["nlml"]))
        gp.fit(Xb[0], yb[0], ell[0], sn[0], Xs=Xsb[0])
        mu, var = gp.predict(Xsb[0])
        assert rel(mu, r["mean"][0]) <= 1e-12 and rel(gp.nlml_, r["nlml"][0]) <= 1e-13
        at = gp.alpha_[:, 0] * gp.sigma_f_                                # alpha~ = K~^-1 y
        assert abs(float(yb[0] @ at) - n * gp.sigma_f_) <= 1e-9 * n * gp.sigma_f_
        rows = np.random.default_rng(0).choice(n, 64, replace=False)      # residual of K~ alpha~ = y on sampled rows
        Krows = O.cov_unit("rbf", Xb[0][rows], Xb[0], ell[0])
        Krows[np.arange(64), rows] += sn[0]
        assert np.max(np.abs(Krows @ at - yb[0][rows])) <= 1e-8 * np.max(np.abs(yb[0]))
        mu2, var2 = gp.predict(Xb[0][:3])                                 # predicting at training points ~ interpolation
        assert np.all(var2 > 0) and np.all(np.abs(mu2 - yb[0][:3]) < 1.0)
    # the bench configuration's panel path (strip solve below each panel's top block, lockstep group of 12 here) agrees
    # with the recursive path of the fits above to the parity tolerance
    ell12, sn12 = np.tile(ell, 4), np.tile(sn, 4)
    with S.GPR(kernel="rbf", outer_blocks=8, panel_mode="strips") as gp:
        r2 = gp.fit_batch(Xb, yb, Xsb, ell12, sn12, concurrency=1, group=12)
    assert np.all(r2["info"] == 0)
    for i in range(3):
        assert rel(r2["mean"][i], r["mean"][i]) <= TOL_PRED and rel(r2["var"][i], r["var"][i]) <= TOL_PRED
        assert rel(r2["nlml"][i], r["nlml"][i]) <= 1e-10 and rel(r2["sigma_f"][i], r["sigma_f"][i]) <= 1e-10
    assert np.array_equal(r2["mean"][:3], r2["mean"][6:9])                # same (data set, hyper-parameters) -> same bits


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d", [(300, 4), (1024, 8), (2049, 32)])
def test_fp32_engine_with_fp64_refinement(S, kind, n, d):
    """BASELINE configs[4] path (fp32 kernel matrix + Cholesky, fp64 iterative refinement with the covariance
    recomputed on the fly) against the fp64 oracle.  Stated tolerances: mean, sigma_f, alpha <= 1e-6 relative
    (SURVEY 8d), variance of the ride-along points <= 1e-5 (refined), nlML <= 1e-5 (its log-det comes from the fp32
    factor), general-path variance <= 1e-3 (fp32 factor)."""
    X, y, Xs = O.synthetic_problem(n, d, 77 + n, m=2)
    ell, sn = np.sqrt(d), 1e-1
    ref = O.fit_predict(X, y, Xs, ell, sn, kind=kind, ref_idiom=False)
    with S.GPR(kernel=kind, dtype="f32") as gp:
        gp.fit(X, y, ell, sn, Xs=Xs)
        mu, var = gp.predict(Xs)
        assert rel(mu, ref["fmean"]) <= 1e-6 and rel(var, ref["fvar"]) <= 1e-5, (rel(mu, ref["fmean"]), rel(var, ref["fvar"]))
        assert rel(gp.sigma_f_, ref["sigma_f"]) <= 1e-6 and rel(gp.nlml_, ref["nlml"]) <= 1e-5
        assert rel(gp.alpha_, ref["alpha"]) <= 1e-6
        assert rel(gp.L_tilde_, ref["L_tilde"]) <= 1e-3            # the factor itself is fp32
        Xs2 = np.random.default_rng(1).standard_normal((140, d))     # > 128 points: chunked general path
        ref2 = O.fit_predict(X, y, Xs2, ell, sn, kind=kind, ref_idiom=False)
        mu2, var2 = gp.predict(Xs2)
        assert rel(mu2, ref2["fmean"]) <= 1e-6 and rel(var2, ref2["fvar"]) <= 1e-3
    with pytest.raises(ValueError):
        S.GPR(kernel="netdiffusion", dtype="f32")


def test_fp32_batch_and_not_spd(S):
    n, d = 700, 8
    X, y, Xs = O.synthetic_problem(n, d, 31, m=1)
    with S.GPR(kernel="matern52", dtype="f32") as gp:
        r = gp.fit_batch(X, y, Xs, [2.0, 3.0, 2.5], [1e-1, 1e-1, 2e-1], concurrency=1, group=4)
        for i, (e, s_) in enumerate(zip([2.0, 3.0, 2.5], [1e-1, 1e-1, 2e-1])):
            ref = O.fit_predict(X, y, Xs, e, s_, kind="matern52", ref_idiom=False)
            assert rel(r["mean"][i], ref["fmean"]) <= 1e-6 and rel(r["nlml"][i], ref["nlml"]) <= 1e-5
        Xbad = X.copy(); Xbad[300:360] = Xbad[0:60]
        with pytest.raises(np.linalg.LinAlgError):
            gp.fit(Xbad, y, 2.0, 0.0)


def test_optimiser_loop_on_the_device_engine(S):
    """The reference's commented-out minimize(MLII, ...) call (north/June1st.py:259-262) re-enabled against the
    engine with the exact gradient: the optimum has a (numerically) zero gradient and a lower nlML than the start."""
    X, y, _ = O.synthetic_problem(400, 4, 5, m=1)
    th0 = np.array([np.log(1.0), np.log(0.5)])
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        f0, _ = gp.nlml(th0, grad=None)
        res = gp.optimize(th0, method="L-BFGS-B")
        f1, g1 = gp.nlml(res.x, grad="exact")
        assert res.fun < f0 - 1.0 and abs(f1 - res.fun) <= 1e-9 * abs(f1)
        assert np.max(np.abs(g1)) <= 1e-3 * max(1.0, abs(f1))
        fo, go = O.mlii(res.x, X, y, kind="rbf", grad="exact")
        assert abs(f1 - fo) <= 1e-9 * abs(fo)


def test_one_handle_through_changing_sizes_kernels_and_paths(S):
    """State hygiene: one handle reused across sizes (buffers grow and shrink logically), ride / no-ride fits,
    batch runs in between, general predict and alpha after each -- every result against the oracle."""
    rng = np.random.default_rng(2024)
    with S.GPR(kernel="matern52") as gp:
        for step, n in enumerate([300, 1100, 64, 515, 129, 1100]):
            d = 5
            X, y, Xs = O.synthetic_problem(n, d, 900 + step, m=2)
            ell, sn = float(1.5 + rng.random()), float(10 ** rng.uniform(-2.5, -1))
            ref = O.fit_predict(X, y, Xs, ell, sn, kind="matern52", ref_idiom=False)
            if step % 2 == 0:
                gp.fit(X, y, ell, sn, Xs=Xs)
            else:
                gp.fit(X, y, ell, sn)                      # no ride rows: predict takes the general path
            mu, var = gp.predict(Xs)
            assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED, (step, n)
            assert rel(gp.alpha_, ref["alpha"]) <= 1e-8 and rel(gp.nlml_, ref["nlml"]) <= 1e-9
            if step in (1, 3):                              # a batch run clobbers the single-fit slot
                r = gp.fit_batch(X, y, Xs, [ell, 2 * ell], [sn, sn], concurrency=2, group=2)
                assert rel(r["mean"][0], ref["fmean"]) <= TOL_PRED
                with pytest.raises(RuntimeError):
                    gp.predict(Xs)                          # no fitted state after a batch
                gp.refit(ell, sn)
                mu2, _ = gp.predict(Xs)
                assert rel(mu2, ref["fmean"]) <= TOL_PRED
            f, g = gp.nlml(np.log([ell, sn]), grad="exact")
            fo, go = O.mlii(np.log([ell, sn]), X, y, kind="matern52", grad="exact")
            assert abs(f - fo) <= 1e-9 * abs(fo) and np.allclose(g, go, rtol=1e-6, atol=1e-8), (step, g, go)
