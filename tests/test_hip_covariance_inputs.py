"""GPU tier: the stationary covariance builds (RBF, Matern-5/2) on inputs the synthetic N(0, 1) problems never reach -- features
far from the origin (SST in kelvin, years, areas in 10^3 km^2), every build path (option kbuild_mfma: VALU distances with the
table-driven exp, GEMM-form distances with the polynomial exp, and the default switch between them at 16 features), the whole
argument range of the covariance functions, and length scales from 1e-160 to 1e160.

Inputs are dyadic (N(0, 1) rounded to 2^-20) with integer offsets, so X + o is exact: the oracle's direct differences see the same
squared distances for every offset, and the engine's K~(X + o) must equal its K~(X).  References: the oracle (direct differences)
where it is defined, mpmath at 50 digits where it is not (the functions' ulp accuracy, the extreme length scales).

Tolerances are the suite's (tests/test_hip_parity.py): K~ 1e-13 relative, predictions / alpha 1e-8, sigma_f / nlML 1e-9; the fp32
engine's from tests/test_hip_round2.py."""
import math

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

TOL_K, TOL_PRED, TOL_SF = 1e-13, 1e-8, 1e-9
MIXED = np.array([273.0, 2000.0, 0.0, -50.0, 1e4, 1.0, -1e4, 12.0])       # per feature, cycled
KINDS = ("rbf", "matern52")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def dyadic(rng, shape, bits=20):
    return np.round(rng.standard_normal(shape) * 2.0 ** bits) / 2.0 ** bits


def offsets(name, d):
    return {"zero": np.zeros(d), "mixed": np.resize(MIXED, d), "1e4": np.full(d, 1e4)}[name]


def problem(n, d, seed, m=5, train_rows=3):
    """Dyadic X, y = sin(X w) + noise, test points = `train_rows` training points + m random ones."""
    rng = np.random.default_rng(seed)
    X = dyadic(rng, (n, d))
    y = np.sin(X @ (rng.standard_normal(d) / np.sqrt(d))) + 0.1 * rng.standard_normal(n)
    Xs = np.vstack([X[[0, n // 2, n - 1][:train_rows]], dyadic(rng, (m, d))])
    return X, y, Xs


def kref(kind, X, ell, sn):
    K = O.cov_unit(kind, X, X, ell)
    K[np.diag_indices_from(K)] += sn
    return np.tril(K)


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


# ---- (a) K~ through every build path ----------------------------------------------------------------------------------------------
# d: the DC = 8 / 32 instantiations, the (d + 3) & ~3 zero padding, a second feature chunk, dp past 64;
# n: inside one 64-row tile, across the 128-column tile, ragged.
A_DIMS = (1, 3, 5, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [7, 129, 300])
def test_kernel_matrix_every_build_path_and_offset(S, kind, n):
    sn = 1e-2
    bad = []
    with S.GPR(kernel=kind) as gp:
        for d in A_DIMS:
            X, y, _ = problem(n, d, 100 * n + d)
            ell = float(np.sqrt(d))
            ref = kref(kind, X, ell, sn)                 # direct differences: the same for every offset (X + o is exact)
            got = {}
            for off in ("zero", "mixed", "1e4"):
                gp.set_data(X + offsets(off, d), y)
                for mf in (0, 1, 2):
                    gp.set_option("kbuild_mfma", mf)
                    K = np.tril(gp.kernel_matrix(ell, sn))
                    got[off, mf] = K
                    e = rel(K, ref)
                    if not (e <= TOL_K):
                        bad.append(("oracle", d, off, mf, e))
            for off in ("zero", "mixed", "1e4"):
                e = rel(got[off, 1], got[off, 0])        # the two builds against each other
                if not (e <= TOL_K):
                    bad.append(("mfma 1 vs 0", d, off, e))
                for mf in (0, 1, 2):                     # translation invariance, engine to engine
                    e = rel(got[off, mf], got["zero", mf])
                    if not (e <= TOL_K):
                        bad.append(("X+o vs X", d, off, mf, e))
    assert not bad, bad


# ---- (b) fits through every entry point that builds K~ with GEMM-form distances ---------------------------------------------------
@pytest.mark.parametrize("kind,d,n", [("rbf", 16, 1100), ("matern52", 32, 1300)])
@pytest.mark.parametrize("off", ["zero", "mixed", "1e4"])
def test_fit_and_predict_at_offsets(S, kind, d, n, off):
    """GPR.fit (K~ + ride rows), ride-along and general predict, with test points that include training points."""
    X, y, Xs = problem(n, d, 7 * d + n)
    ell = float(np.sqrt(d))
    o = offsets(off, d)
    Xs2 = np.vstack([Xs, Xs[:2] + 0.25])                 # different shape: the general path (cross-covariances + forward solve)
    with S.GPR(kernel=kind) as gp:
        for sn in (1e-2, 1e-4):
            ref = O.fit_predict(X, y, Xs, ell, sn, kind=kind, ref_idiom=False)
            ref2 = O.fit_predict(X, y, Xs2, ell, sn, kind=kind, M=ref["M"], ref_idiom=False)
            gp.fit(X + o, y, ell, sn, Xs=Xs + o)
            mu, var = gp.predict(Xs + o)
            mu2, var2 = gp.predict(Xs2 + o)
            assert rel(mu, ref["fmean"]) <= TOL_PRED and rel(var, ref["fvar"]) <= TOL_PRED, (sn, rel(mu, ref["fmean"]), rel(var, ref["fvar"]))
            assert rel(mu2, ref2["fmean"]) <= TOL_PRED and rel(var2, ref2["fvar"]) <= TOL_PRED, (sn, rel(mu2, ref2["fmean"]), rel(var2, ref2["fvar"]))
            assert rel(gp.sigma_f_, ref["sigma_f"]) <= TOL_SF and rel(gp.nlml_, ref["nlml"]) <= TOL_SF, (sn, rel(gp.nlml_, ref["nlml"]))
            assert rel(gp.alpha_, ref["alpha"]) <= TOL_PRED, (sn, rel(gp.alpha_, ref["alpha"]))


@pytest.mark.parametrize("panel_mode", [None, "strips"])
def test_lockstep_batch_members_with_different_offsets(S, panel_mode):
    """fit_batch as one lockstep group whose members carry different offsets (per-member data set kps.ds); once with strip panels."""
    n, d, B = 1100, 32, 3
    kind = "matern52"
    Xb, yb, Xsb = np.zeros((B, n, d)), np.zeros((B, n)), np.zeros((B, 5, d))
    base = []
    for b, off in enumerate(("1e4", "zero", "mixed")):
        X, y, Xs = problem(n, d, 900 + b, m=2)
        base.append((X, y, Xs))
        o = offsets(off, d)
        Xb[b], yb[b], Xsb[b] = X + o, y, Xs + o
    ell = np.array([np.sqrt(d), 1.2 * np.sqrt(d), 0.9 * np.sqrt(d)])
    sn = np.array([1e-2, 1e-3, 1e-2])
    with S.GPR(kernel=kind, outer_blocks=2, panel_mode=panel_mode) as gp:
        if panel_mode == "strips":
            gp.set_option("strip_min", 1)
        r = gp.fit_batch(Xb, yb, Xsb, ell, sn, concurrency=1, group=B)
    assert np.all(r["info"] == 0)
    for b, (X, y, Xs) in enumerate(base):
        ref = O.fit_predict(X, y, Xs, ell[b], sn[b], kind=kind, ref_idiom=False)
        assert rel(r["mean"][b], ref["fmean"]) <= TOL_PRED and rel(r["var"][b], ref["fvar"]) <= TOL_PRED, (b, rel(r["mean"][b], ref["fmean"]))
        assert rel(r["nlml"][b], ref["nlml"]) <= TOL_SF and rel(r["sigma_f"][b], ref["sigma_f"]) <= TOL_SF, (b, rel(r["nlml"][b], ref["nlml"]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("off", ["mixed", "1e4"])
def test_exact_gradient_at_offsets(S, kind, off):
    """nlml(theta, grad='exact') -- K~ and the derivative matrix (full build) -- with the tolerances of
    test_exact_gradient_matches_oracle_and_finite_differences."""
    n, d = 1000, 16
    X, y, _ = problem(n, d, 31)
    th = np.array([np.log(np.sqrt(d)) + 0.2, np.log(1e-2)])
    fo, go = O.mlii(th, X, y, kind=kind, grad="exact")
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X + offsets(off, d), y)
        f0, g0 = gp.nlml(th, grad="exact")
    assert abs(f0 - fo) <= 1e-9 * abs(fo), (f0, fo)
    assert np.allclose(g0, go, rtol=1e-7, atol=1e-9), (g0, go)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("off", ["zero", "1e4"])
def test_fp32_engine_refinement_at_offsets(S, kind, off):
    """fp32 factor + fp64 refinement at d = 32: refined against the stored fp64 K~ (GEMM form) and against recomputed covariances
    (direct differences) -- the two agree as in test_fp32_refinement_from_the_stored_fp64_matrix_equals_the_recomputed_one, and each
    matches the oracle at that test's tolerances."""
    n, d, sn = 1300, 32, 0.1
    X, y, Xs = problem(n, d, 4242, m=1, train_rows=2)
    ell = float(np.sqrt(d))
    o = offsets(off, d)
    got = []
    with S.GPR(kernel=kind, dtype="f32") as gp:
        for stored in (1, 0):
            gp.set_option("refine_stored", stored)
            gp.fit(X + o, y, ell, sn, Xs=Xs + o)
            mu, var = gp.predict(Xs + o)
            got.append((gp.alpha_.copy(), gp.nlml_, gp.sigma_f_, mu, var, gp.refine_residual_))
    a1, a0 = got
    assert rel(a1[0], a0[0]) <= 1e-11 and rel(a1[1], a0[1]) <= 1e-12 and rel(a1[2], a0[2]) <= 1e-12, (rel(a1[0], a0[0]), rel(a1[1], a0[1]))
    assert rel(a1[3], a0[3]) <= 1e-11 and rel(a1[4], a0[4]) <= 1e-10, (rel(a1[3], a0[3]), rel(a1[4], a0[4]))
    ref = O.fit_predict(X, y, Xs, ell, sn, kind=kind, ref_idiom=False)
    for a in (a1, a0):
        assert 0 <= a[5] <= 1e-10
        assert rel(a[0], ref["alpha"]) <= 1e-6 and rel(a[1], ref["nlml"]) <= 5e-5, (rel(a[0], ref["alpha"]), rel(a[1], ref["nlml"]))
        assert rel(a[3], ref["fmean"]) <= 1e-6 and rel(a[4], ref["fvar"]) <= 1e-5, (rel(a[3], ref["fmean"]), rel(a[4], ref["fvar"]))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sharded_fit_one_rank_at_offsets(S, dtype):
    """DistributedGPR on one rank: the build of the own block columns (cyclic tile selection) with offset features."""
    n, d, sn = 2100, 32, 1e-1
    X, y, Xs = problem(n, d, 515, m=1, train_rows=2)
    ell = float(np.sqrt(d))
    o = offsets("mixed", d)
    ref = O.fit_predict(X, y, Xs, ell, sn, kind="rbf", ref_idiom=False)
    with S.DistributedGPR("rbf", 0, 1, None, device=0, outer_blocks=8, dtype=dtype) as dg:
        dg.fit(X + o, y, ell, sn, Xs=Xs + o)
        mu, var = dg.predict(Xs + o)
        nl = dg.nlml_
    tp, tv, tn = (TOL_PRED, TOL_PRED, TOL_SF) if dtype == "f64" else (1e-6, 1e-5, 5e-5)
    assert rel(mu, ref["fmean"]) <= tp and rel(var, ref["fvar"]) <= tv, (rel(mu, ref["fmean"]), rel(var, ref["fvar"]))
    assert rel(nl, ref["nlml"]) <= tn, (nl, ref["nlml"])


# ---- (c) the covariance functions over their whole argument range, in ulps ------------------------------------------------------------
# Stated bounds (kernels_misc.hpp): exp_cov <= 2 ulp, exp_cov_tab <= 4 ulp, where the result is normal; <= 2 units of 2^-1074 where it
# is subnormal (measured on MI355X: 1.97 / 0.82 ulp, 0.94 / 0.78 units).  Matern-5/2 (1 + s + s^2/3) exp(-s), from the same fp64 s:
# MATERN_ULP ulp while exp(-s) is normal (measured 3.73 with exp_cov_tab, 2.70 with exp_cov), plus (1 + s + s^2/3) units of 2^-1074
# beyond (the subnormal exp's own rounding, magnified by the polynomial).
EXP_ULP = {0: 4, 1: 2}          # kbuild_mfma -> bound of the exp it uses (0: exp_cov_tab, 1: exp_cov)
MATERN_ULP = {0: 4, 1: 3}
TINY = 2.0 ** -1074


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def ulp_errors(got, exact_mp, mpmath):
    """|got - exact| in ulps of the exact value (normal results) and in units of 2^-1074 (subnormal results)."""
    out_n, out_s = np.zeros(len(got)), np.zeros(len(got))
    for i, (g, e) in enumerate(zip(got, exact_mp)):
        err = abs(mpmath.mpf(float(g)) - e)
        ef = float(e)
        if ef >= 2.2250738585072014e-308:
            out_n[i] = float(err / mpmath.ldexp(1, math.frexp(ef)[1] - 53))
        else:
            out_s[i] = float(err / mpmath.mpf(TINY))
    return out_n, out_s


def dyadic_line(n, seed):
    """d = 1 points on a 2^-10 grid in [-20, 20]: squared distances, norms, dot products and row shifts are all exact."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.uniform(-20.0, 20.0, n) * 1024.0) / 1024.0
    x[:4] = [-20.0, 20.0, -19.0, 19.0]
    return x.reshape(-1, 1)


def test_exp_accuracy_over_the_whole_argument_range(S):
    """RBF with l = 1, sn~ = 0: every entry of K~ is exp(x), x = fl(-0.5 |d|^2) exact, x in [-800, 0]."""
    mpmath = _mp()
    n = 640
    X = dyadic_line(n, 77)
    sq = (X - X.T) ** 2
    il = np.tril_indices(n, -1)
    xv = -0.5 * sq[il]                                   # what the kernel forms (c_rbf = -0.5 exactly)
    ux, inv = np.unique(xv, return_inverse=True)
    # coverage: every residue of the table index k mod 64 on both sides of each rounding boundary, the subnormal tail
    t = ux * (64.0 * 1.44269504088896338700)
    k = np.rint(t)
    side = t - k                                        # (-0.5, 0.5]: which side of the boundary the argument rounded from
    for r in range(64):
        sel = (k.astype(np.int64) & 63) == r
        assert np.any(sel & (side > 0.45)) and np.any(sel & (side < -0.45)), r
    assert np.sum((ux > -745.0) & (ux < -708.0)) >= 100 and ux.min() < -746.0
    ex = [mpmath.exp(mpmath.mpf(float(v))) for v in ux]
    with S.GPR(kernel="rbf") as gp:
        gp.set_data(X, np.zeros(n))
        for mf in (0, 1):
            gp.set_option("kbuild_mfma", mf)
            K = gp.kernel_matrix(1.0, 0.0)
            assert np.all(np.diag(K) == 1.0)
            got = np.zeros(len(ux))
            got[inv] = K[il]
            assert np.all(got[inv] == K[il])                # one value per argument
            en, es = ulp_errors(got, ex, mpmath)
            assert en.max() <= EXP_ULP[mf] and es.max() <= 2.0, (mf, en.max(), float(ux[np.argmax(en)]), es.max())


def test_matern_accuracy_over_the_whole_argument_range(S):
    """Matern-5/2 with l = 1/16 (inv_ell = 16 exact), sn~ = 0: s = fl(sqrt(5 |d|^2)) 16 in [0, 1431]; reference from the same fp64 s."""
    mpmath = _mp()
    n = 640
    X = dyadic_line(n, 78)
    sq = (X - X.T) ** 2
    il = np.tril_indices(n, -1)
    sv = np.sqrt(5.0 * sq[il]) * 16.0
    us, inv = np.unique(sv, return_inverse=True)
    assert np.sum((us > 708.0) & (us < 745.0)) >= 100 and us.max() > 758.0
    ex, poly = [], np.zeros(len(us))
    for i, v in enumerate(us):
        s = mpmath.mpf(float(v))
        p = 1 + s + s * s / 3
        ex.append(p * mpmath.exp(-s))
        poly[i] = float(p)
    with S.GPR(kernel="matern52") as gp:
        gp.set_data(X, np.zeros(n))
        for mf in (0, 1):
            gp.set_option("kbuild_mfma", mf)
            K = gp.kernel_matrix(0.0625, 0.0)
            assert np.all(np.diag(K) == 1.0)
            got = np.zeros(len(us))
            got[inv] = K[il]
            assert np.all(got[inv] == K[il])
            err = np.array([float(abs(mpmath.mpf(float(g)) - e)) for g, e in zip(got, ex)])
            exf = np.array([float(e) for e in ex])
            ulp = np.array([math.ldexp(1.0, math.frexp(v)[1] - 53) if v > 0 else TINY for v in exf])
            normal_exp = us < 708.0                     # exp(-s) normal
            en = err[normal_exp] / ulp[normal_exp]
            assert en.max() <= MATERN_ULP[mf], (mf, en.max(), float(us[normal_exp][np.argmax(en)]))
            beyond = ~normal_exp
            lim = MATERN_ULP[mf] * ulp[beyond] + (poly[beyond] + 1.0) * TINY
            assert np.all(err[beyond] <= lim), (mf, float(np.max(err[beyond] / lim)))


# ---- (d) length-scale extremes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matrix_at_extreme_length_scales(S, kind):
    """l from 1e-160 to 1e160: K~ finite, in [0, 1 + sn~], diagonal exactly 1 + sn~, off-diagonal entries within the functions' ulp
    bounds of mpmath at the kernel's own fp64 argument (x = fl(c_rbf |d|^2), c_rbf = -0.5 / l^2 clamped to -DBL_MAX; s = fl(sqrt(5 |d|^2)
    / l), bounded by 1e3) and exactly 0 where that value underflows.  d = 3 dyadic points: |d|^2 is exact in both builds."""
    mpmath = _mp()
    n, d, sn = 129, 3, 1e-2
    X, y, _ = problem(n, d, 606)
    il = np.tril_indices(n, -1)
    sq = O.sqdist(X, X)[il]
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        for ell in (1e-160, 1e-10, 1e-3, 1e3, 1e10, 1e160):
            with np.errstate(over="ignore", divide="ignore"):
                c_rbf = max(-0.5 / (ell * ell), -np.finfo(np.float64).max)
                inv_ell = min(1.0 / ell, np.finfo(np.float64).max)
                arg = c_rbf * sq if kind == "rbf" else np.minimum(np.sqrt(5.0 * sq) * inv_ell, 1e3)
            ex, extra = [], []                           # exact value, allowance beyond the ulp bound (the (c) tests' subnormal terms)
            for v in arg:
                fv = float(v)
                v = mpmath.mpf(fv)
                if kind == "rbf":
                    ex.append(mpmath.exp(v)); extra.append(2 * TINY)
                else:
                    p = 1 + v + v * v / 3
                    ex.append(p * mpmath.exp(-v)); extra.append(float(p + 1) * TINY if fv >= 708.0 else 2 * TINY)
            for mf in (0, 1):
                gp.set_option("kbuild_mfma", mf)
                K = gp.kernel_matrix(ell, sn)
                assert np.all(np.isfinite(K)), (ell, mf)
                assert np.all(np.diag(K) == 1.0 + sn), (ell, mf, np.diag(K)[:4])
                off = K[il]
                assert np.all((off >= 0.0) & (off <= 1.0 + sn)), (ell, mf)
                bound = EXP_ULP[mf] if kind == "rbf" else MATERN_ULP[mf]
                for g, e, x in zip(off, ex, extra):
                    ef = float(e)
                    if e < mpmath.ldexp(1, -1076):             # underflows (clear of the rounding boundary at 2^-1075)
                        assert g == 0.0, (ell, mf, g, e)
                    else:
                        u = math.ldexp(1.0, math.frexp(ef)[1] - 53) if ef >= 2.2250738585072014e-308 else TINY
                        assert float(abs(mpmath.mpf(float(g)) - e)) <= bound * u + x, (ell, mf, g, e)


@pytest.mark.parametrize("kind", KINDS)
def test_nlml_at_a_vanishing_length_scale(S, kind):
    """l = 1e-160: K~ = (1 + sn~) I, so the profiled nlML is n/2 (1 + log(y^T y / n) + log 2 pi) and both gradients vanish."""
    n, d, snt = 300, 4, 1e-2
    X, y, _ = problem(n, d, 707)
    closed = 0.5 * n * (1.0 + np.log(float(y @ y) / n) + np.log(2.0 * np.pi))
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        f0, _ = gp.nlml((np.log(1e-160), np.log(snt)), grad=None)
        f1, g1 = gp.nlml((np.log(1e-160), np.log(snt)), grad="exact")
    assert abs(f0 - closed) <= 1e-12 * abs(closed) and abs(f1 - closed) <= 1e-12 * abs(closed), (f0, f1, closed)
    assert np.all(np.isfinite(g1)) and np.max(np.abs(g1)) <= 1e-10 * n, g1
