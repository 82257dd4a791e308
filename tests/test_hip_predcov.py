"""GPU tier of the joint predictive covariance (``GPR.predict_cov`` / ``predict(return_cov=True)`` / ``sample``; sigp_predict_cov):
against the NumPy closed form that tests/test_predcov_host.py pins to the oracle, against what the engine already returns
(``predict``), and the split-K driver against itself.

Tolerances.  A covariance matrix is compared on ITS OWN scale, e = max|cov - cov_ref| / max(diag(cov_ref)) <= 1e-8 -- the suite's
prediction tolerance (tests/test_hip_parity.py); off-diagonal entries are not compared elementwise, they can be arbitrarily close
to zero.  Means: 1e-8 of max|y|.  Every problem has cond(K~) <= 1e6 (asserted), so both sides carry at most ~1e6 x 2.2e-16."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from test_predcov_host import predcov_closed_form, predcov_factor

pytestmark = pytest.mark.gpu

TOL = 1e-8
KINDS = ["rbf", "matern52", "netdiffusion"]


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _problem(kind, n, seed):
    """the settings of tests/test_hip_loo.py: (X, y, ell, sn~, M)"""
    if kind == "netdiffusion":
        X, y, _ = O.synthetic_problem(n, 12, seed)
        return X, y, 0.05, 1e-2, O.laplacian_M(X)
    X, y, _ = O.synthetic_problem(n, 8, seed)
    return X, y, np.sqrt(8.0), 1e-2, None


def _test_points(m, d, seed):
    """m test points with two identical rows (the first and the last: in different 128-row chunks when m > 128)"""
    Xs = O.synthetic_problem(m, d, seed)[0].copy()
    if m >= 2:
        Xs[m - 1] = Xs[0]
    return Xs


@functools.lru_cache(maxsize=None)
def _fit(kind, n):
    """one problem per (kind, n), factorised on the host once and shared (read-only) by every test that needs it"""
    X, y, ell, sn, M = _problem(kind, n, 20240500 + n)
    f = predcov_factor(X, y, ell, sn, kind, M)
    w = np.linalg.eigvalsh(f["K_tilde"])
    cond = float(w[-1] / w[0])
    print("%s n=%d: cond(K~) = %.3g" % (kind, n, cond))
    for a in (X, y, f["K_tilde"], f["L_tilde"], f["z"]):
        a.setflags(write=False)
    return dict(X=X, y=y, ell=ell, sn=sn, M=M, factor=f, cond=cond)


def _reference(p, kind, Xs, noise):
    return predcov_closed_form(p["X"], p["y"], Xs, p["ell"], p["sn"], kind, p["M"], noise, factor=p["factor"])


def _cov_err(cov, ref):
    return float(np.max(np.abs(cov - ref)) / np.max(np.diag(ref)))


def _check(tag, p, kind, Xs, mean, cov, noise):
    ref = _reference(p, kind, Xs, noise)
    e_cov, e_mean = _cov_err(cov, ref["cov"]), float(np.max(np.abs(mean - ref["mean"])) / np.max(np.abs(p["y"])))
    print("%s noise=%d: cov %.3g  mean %.3g" % (tag, noise, e_cov, e_mean))
    assert e_cov <= TOL, (tag, noise, e_cov)
    assert e_mean <= TOL, (tag, noise, e_mean)


# ---- 1. parity with the closed form -------------------------------------------------------------------------------------------------
# a single chunk (m = 1, 2), the chunk boundary (127, 128, 129), several tile pairs (300), several K blocks (n = 300, 1000), and n = 2500:
# past the 2048 panel boundary of the factor, with 20 block columns that the automatic slice count does not divide evenly
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m", [(37, 1), (37, 2), (300, 127), (300, 128), (300, 129), (300, 300), (1000, 300), (2500, 129)])
def test_predict_cov_equals_the_closed_form(S, kind, n, m):
    p = _fit(kind, n)
    assert p["cond"] <= 1e6
    Xs = _test_points(m, p["X"].shape[1], 20240600 + m)
    with S.GPR(kernel=kind) as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"], M=p["M"])
        mean, cov = gp.predict_cov(Xs, noise=True)
        mean_l, cov_l = gp.predict_cov(Xs, noise=False)
        sigma_n = gp.sigma_n_
    assert mean.shape == (m,) and cov.shape == (m, m)
    tag = "%s n=%d m=%d" % (kind, n, m)
    _check(tag, p, kind, Xs, mean, cov, True)
    _check(tag, p, kind, Xs, mean_l, cov_l, False)
    assert np.array_equal(mean, mean_l)
    # the noise is sigma_n on the diagonal and nothing anywhere else
    dlt = cov - cov_l
    e_noise = float(np.max(np.abs(np.diag(dlt) / sigma_n - 1.0)))
    print("%s: diag(noise - latent) / sigma_n - 1 = %.3g" % (tag, e_noise))
    assert e_noise <= 1e-12
    assert np.array_equal(dlt - np.diag(np.diag(dlt)), np.zeros((m, m)))


# ---- 2. consistency with what exists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [5, 129])          # predict's single-chunk path and (RBF / Matern) its lockstep groups
def test_predict_cov_is_consistent_with_predict_and_leaves_the_fit_alone(S, kind, m):
    p = _fit(kind, 300)
    assert p["cond"] <= 1e6
    Xs = _test_points(m, p["X"].shape[1], 20240700 + m)
    with S.GPR(kernel=kind) as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"], M=p["M"])
        mu0, var0 = gp.predict(Xs)
        loo0, nlml0 = gp.loo("refit"), gp.nlml_
        mean, cov = gp.predict_cov(Xs, noise=True)
        mean_rc, cov_rc = gp.predict(Xs, return_cov=True)
        _, lat = gp.predict_cov(Xs, noise=False)
        mu1, var1 = gp.predict(Xs)
        loo1, nlml1 = gp.loo("refit"), gp.nlml_
    e_diag = float(np.max(np.abs(np.diag(cov) / var0 - 1.0)))
    print("%s m=%d: diag(cov) / predict's var - 1 = %.3g" % (kind, m, e_diag))
    assert e_diag <= 1e-8
    assert np.array_equal(mean, mu0)                                   # the same launches, the same bits
    assert np.array_equal(mean_rc, mean) and np.array_equal(cov_rc, cov)
    assert np.array_equal(cov, cov.T) and np.array_equal(lat, lat.T)
    np.linalg.cholesky(cov)                                            # raises LinAlgError unless positive definite
    # the identical test rows (first and last): identical rows and columns of the latent covariance
    assert np.array_equal(lat[0], lat[m - 1]) and np.array_equal(lat[:, 0], lat[:, m - 1])
    # the fit is only read
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0) and nlml1 == nlml0
    for k in ("mean", "var"):
        assert np.array_equal(loo1[k], loo0[k]), k
    assert loo1["nlpd"] == loo0["nlpd"] and loo1["sse"] == loo0["sse"]


# ---- 3. split-K ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,slices", [(1000, 129, (1, 3, 0, 8)), (2500, 300, (1, 3, 0))])      # 8 = every block column of n = 1000 its own slice
def test_slice_counts_agree_and_each_is_deterministic(S, n, m, slices):
    kind = "rbf"
    p = _fit(kind, n)
    assert p["cond"] <= 1e6
    Xs = _test_points(m, p["X"].shape[1], 20240800 + m)
    nkb = (n + 127) // 128
    got = {}
    with S.GPR(kernel=kind) as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"], M=p["M"])
        for s_ in slices:
            gp.set_option("cov_slices", s_)
            mean, cov = gp.predict_cov(Xs)
            mean2, cov2 = gp.predict_cov(Xs)
            assert np.array_equal(cov, cov2) and np.array_equal(mean, mean2), s_      # fixed summation order: the same bits on every run
            assert np.array_equal(cov, cov.T)
            got[s_] = (mean, cov)
        for bad in (-1, nkb + 1):
            with pytest.raises(ValueError) as ei:
                gp.set_option("cov_slices", bad)
            assert "cov_slices" in str(ei.value)
        mean, cov = gp.predict_cov(Xs)                                               # a rejected value leaves the last valid one in force
        assert np.array_equal(cov, got[slices[-1]][1])
    _check("rbf n=%d m=%d cov_slices=1" % (n, m), p, kind, Xs, got[1][0], got[1][1], True)
    scale = float(np.max(np.diag(got[1][1])))
    for s_ in slices[1:]:
        e = float(np.max(np.abs(got[s_][1] - got[1][1]))) / scale
        print("n=%d m=%d: cov_slices %d against 1: %.3g" % (n, m, s_, e))
        assert e <= 1e-12, (s_, e)                                                    # another summation order: not bit for bit
        assert np.array_equal(got[s_][0], got[1][0])                                  # the mean does not go through the product


# ---- 4. more than one lockstep group of the forward solve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "netdiffusion"])
def test_more_test_points_than_one_solve_group(S, kind):
    n, m = 300, 2100                                 # 17 chunks of 128 rows: a full group of 16 and a second one
    p = _fit(kind, n)
    assert p["cond"] <= 1e6
    Xs = _test_points(m, p["X"].shape[1], 20240900)
    with S.GPR(kernel=kind) as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"], M=p["M"])
        mean, cov = gp.predict_cov(Xs, noise=True)
        mu, _ = gp.predict(Xs)
    _check("%s n=%d m=%d" % (kind, n, m), p, kind, Xs, mean, cov, True)
    assert np.array_equal(cov, cov.T) and np.array_equal(mean, mu)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_are_value_errors_and_leave_the_handle_usable(S):
    from seaiceextentforecasting_amd import _lib as L
    p = _fit("rbf", 300)
    d = p["X"].shape[1]
    Xs = _test_points(3, d, 20241000)

    def raises(fn):
        with pytest.raises(ValueError) as ei:
            fn()
        assert len(str(ei.value)) > len("predict_cov: "), str(ei.value)

    with S.GPR(kernel="rbf") as gp:
        raises(lambda: gp.predict_cov(Xs))                                          # before fit
        gp.fit(p["X"], p["y"], p["ell"], p["sn"])
        raises(lambda: gp.predict_cov(np.zeros((0, d))))                            # m = 0
        raises(lambda: gp.predict_cov(np.zeros((L.MAX_COV + 1, d))))                # m = SIGP_MAX_COV + 1
        raises(lambda: gp.predict_cov(np.zeros((3, d + 1))))                        # the wrong number of columns
        raises(lambda: gp.predict_cov(np.zeros((3, d - 1))))
        raises(lambda: gp.sample(np.zeros((3, d)), z=np.zeros((2, 4))))             # z of the wrong shape
        # the C entry point's own checks
        mean, cov = np.zeros(3), np.zeros((3, 3))
        big = np.zeros((1, d))
        for args in ((L.ptr(Xs), 0, d, 1, L.ptr(mean), L.ptr(cov), 3), (L.ptr(big), L.MAX_COV + 1, d, 1, L.ptr(mean), L.ptr(cov), L.MAX_COV + 1),
                     (L.ptr(Xs), 3, d - 1, 1, L.ptr(mean), L.ptr(cov), 3), (L.ptr(Xs), 3, d, 1, L.ptr(mean), L.ptr(cov), 2),
                     (None, 3, d, 1, L.ptr(mean), L.ptr(cov), 3), (L.ptr(Xs), 3, d, 1, None, L.ptr(cov), 3), (L.ptr(Xs), 3, d, 1, L.ptr(mean), None, 3)):
            assert gp._lib.sigp_predict_cov(gp._h, *args) == L.BAD_ARG, args[1:]
            assert gp._lib.sigp_last_error(gp._h).decode().startswith("predict_cov:")
        mean, cov = gp.predict_cov(Xs)                                              # the handle is still good
        _check("after errors", p, "rbf", Xs, mean, cov, True)
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"])
        mu0, var0 = gp.predict(Xs)
        raises(lambda: gp.predict_cov(Xs))                                          # the fp32 engine has no joint covariance
        mu1, var1 = gp.predict(Xs)
        assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)


# ---- 6. sample --------------------------------------------------------------------------------------------------------------------------
def test_sample_is_mean_plus_cholesky_factor_times_z(S):
    kind, n, m, size = "rbf", 300, 40, 6
    p = _fit(kind, n)
    Xs = _test_points(m, p["X"].shape[1], 20241100)
    z = np.random.default_rng(7).standard_normal((size, m))
    with S.GPR(kernel=kind) as gp:
        gp.fit(p["X"], p["y"], p["ell"], p["sn"])
        for noise in (False, True):
            mean, cov = gp.predict_cov(Xs, noise=noise)
            draws = gp.sample(Xs, size=size, noise=noise, z=z)
            jitter = gp.sample_jitter_
            scale = float(np.max(np.diag(cov)))
            assert draws.shape == (size, m)
            assert jitter == 0.0 if noise else (jitter == 0.0 or 1e-12 <= jitter <= 1e-6)
            want = mean + (np.linalg.cholesky(cov + jitter * scale * np.eye(m)) @ z.T).T
            e = float(np.max(np.abs(draws - want)))
            print("sample noise=%d: jitter %.3g  |draws - (mean + chol z)| %.3g" % (noise, jitter, e))
            assert e <= 1e-10
            if not noise:
                # Rows 0 and m-1 of the latent covariance are identical, so with C' = cov + jitter scale I = L L^T the two columns of the
                # draws differ by (L_0 - L_{m-1}) . z_k, and |L_0 - L_{m-1}|^2 = (e_0 - e_{m-1})^T C' (e_0 - e_{m-1}) = 2 jitter scale exactly,
                # plus the factorisation's backward error (e_0 - e_{m-1})^T dC (e_0 - e_{m-1}) <= 4 (m + 2) eps scale (Higham, Thm 10.3).
                bound = np.sqrt(2.0 * jitter * scale + 4.0 * (m + 2) * np.finfo(float).eps * scale) * np.linalg.norm(z, axis=1)
                gap = np.abs(draws[:, 0] - draws[:, m - 1])
                print("duplicated point: max gap %.3g  (bound %.3g)" % (gap.max(), bound.max()))
                assert np.all(gap <= bound)
        a = gp.sample(Xs, size=3, seed=123)
        b = gp.sample(Xs, size=3, seed=123)
        c = gp.sample(Xs, size=3, seed=124)
        assert a.shape == (3, m) and np.array_equal(a, b) and not np.array_equal(a, c)
        assert gp.sample(Xs[:5]).shape == (1, 5)


# ---- 7. the reference kernel at the reference's own size ------------------------------------------------------------------------------
def test_golden_retro_record_joint_covariance(S):
    r = load_golden("north_June_retro")["records"][-1]
    X, y, M, ell, sn = r["X"], r["y"].reshape(-1), r["M"], float(r["ell"]), float(r["sn_tilde"])
    Xs = np.vstack([r["Xs"], X[:3]])                 # the record's test row and three training rows
    with S.GPR(kernel="netdiffusion") as gp:
        gp.fit(X, y, ell, sn, M=M, Xs=r["Xs"])       # fitted as tests/test_hip_parity.py does
        got = {noise: gp.predict_cov(Xs, noise=noise) for noise in (True, False)}
        mu, var = gp.predict(r["Xs"])
    for noise in (True, False):
        ref = predcov_closed_form(X, y, Xs, ell, sn, "netdiffusion", M, noise)
        e_cov = _cov_err(got[noise][1], ref["cov"])
        e_mean = float(np.max(np.abs(got[noise][0] - ref["mean"])) / np.max(np.abs(y)))
        print("golden n=%d noise=%d: cov %.3g  mean %.3g" % (len(y), noise, e_cov, e_mean))
        assert e_cov <= TOL and e_mean <= TOL
    assert abs(got[True][1][0, 0] / var[0] - 1.0) <= 1e-8 and abs(got[True][0][0] - mu[0]) <= 1e-8 * np.max(np.abs(y))
    fvar_ref = float(r["KXsXs"][0, 0] - np.sum(r["v"] ** 2))              # north/June1st.py:277 on the reference's own captured locals
    assert abs(got[True][1][0, 0] / fvar_ref - 1.0) <= 1e-8
