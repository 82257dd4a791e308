"""GPU tier of the per-feature (ARD) gradients of the leave-one-out scores in lockstep groups: ``GPR.loo_ard_batch``,
``GPR.optimize_ard_batch`` and the C entry point sigp_loo_grad_ard_batch.

Reference and conventions are those of tests/test_hip_loo_ard.py and tests/test_hip_ard_batch.py: the per-point NumPy closed form of
tests/test_loo_ard_host.py, every gradient error measured against the per-component scale S, the device within max(1e-8, 10 x spread) where
spread is the disagreement of the reference's two routes to K~^-1; a case counts only when spread <= 1e-8 (a condition every shape below
meets: checked with the closed form alone).  Scales belong to a fit, not to a data set: fit i uses data set (first + i) % B."""
import functools

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_hip_loo_ard import CRITERIA, KINDS, MODES, _check, _reference_of
from test_loo_ard_batch_host import loo_objective
from test_loo_host import loo_closed_form

pytestmark = pytest.mark.gpu

SNS = (1e-2, 3e-2)


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
def _problem(n, d, B=2, F=7, first=1):
    """B data sets and F members with scales and noise of their own: (Xb, yb, ells [F, d], sn [F], theta [F, d + 1], data set of member i)"""
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20260700 + 11 * n + d + 1000 * b)
    ells = np.stack([ard_scales(d, 20260800 + 11 * n + d + 1000 * i) for i in range(F)])
    sn = np.array([SNS[i % 2] for i in range(F)])
    theta = np.concatenate([np.log(ells), np.log(sn)[:, None]], axis=1)
    return Xb, yb, ells, sn, theta, [(first + i) % B for i in range(F)]


@functools.lru_cache(maxsize=None)
def _references(kind, n, d):
    """per member {mode: (closed form, {criterion: spread}, other route)}: computed once, shared by the tests below"""
    Xb, yb, ells, sn, _, ds = _problem(n, d)
    return [_reference_of(kind, Xb[ds[i]], yb[ds[i]], ells[i], sn[i]) for i in range(len(ds))]


# ---- 1. every member against the closed form ---------------------------------------------------------------------------------------------------
# minimal n, one tile exactly, one row past a tile, d past 8 (the <32> instantiation), several tiles, d past one 64-column pad
SHAPES = [(2, 1), (37, 3), (128, 8), (129, 9), (300, 8), (200, 65)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_members_equal_the_closed_form(S, kind, n, d):
    """B = 2 data sets, F = 7 members in groups of 3, 3, 1 (a partial last group), first = 1; both criteria, both sigma modes"""
    Xb, yb, ells, sn, theta, ds = _problem(n, d)
    refs = _references(kind, n, d)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                key = crit[4:]
                r = gp.loo_ard_batch(theta, first=1, criterion=crit, sigma_f=mode, group=3, predictions=True)
                assert set(r) == {"value", "grad", "mean", "var", "nlpd", "sse"}
                assert r["value"].shape == (7,) and r["grad"].shape == (7, d + 1) and r["mean"].shape == (7, n) and r["var"].shape == (7, n)
                assert _same_bits(r["value"], r[key])
                for i in range(7):
                    a, spread, _ = refs[i][mode]
                    _check("%s n=%d d=%d %s %s member %d" % (kind, n, d, mode, crit, i), r["grad"][i], a[key + "_grad"], a[key + "_S"], spread[crit])
                    for k in ("nlpd", "sse"):
                        assert abs(float(r[k][i]) - a[k]) <= 1e-8 * abs(a[k]), (mode, crit, i, k, r[k][i], a[k])
                    if crit == CRITERIA[0]:           # (the predictions do not depend on the criterion)
                        want = loo_closed_form(O.cov_unit(kind, Xb[ds[i]] / ells[i], Xb[ds[i]] / ells[i], 1.0) + sn[i] * np.eye(n), yb[ds[i]], mode)
                        assert np.max(np.abs(r["mean"][i] - want["mean"])) <= 1e-8 * np.max(np.abs(yb[ds[i]])), (mode, i)     # (the scale of test_hip_loo.py)
                        assert np.all(np.abs(r["var"][i] - want["var"]) <= 1e-8 * want["var"]), (mode, i)


# ---- 2. the bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", [(129, 8), (300, 8)])
def test_members_have_the_bits_of_the_single_fit_whatever_the_group(S, kind, n, d):
    Xb, yb, _, sn, theta, ds = _problem(n, d)
    F = len(ds)
    ells = np.stack([S.GPR._exp(t[:d]) for t in theta])        # the library's own exp(theta): the scales the staging divides by
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                v3, g3 = gp.loo_ard_batch(theta, first=1, criterion=crit, sigma_f=mode, group=3)
                v3b, g3b = gp.loo_ard_batch(theta, first=1, criterion=crit, sigma_f=mode, group=3)
                v1, g1 = gp.loo_ard_batch(theta, first=1, criterion=crit, sigma_f=mode, group=1)
                v0, g0 = gp.loo_ard_batch(theta, first=1, criterion=crit, sigma_f=mode, group=3, grad=None)
                assert _same_bits(v3, v3b) and _same_bits(g3, g3b), "two calls differ"
                assert _same_bits(v3, v1) and _same_bits(g3, g1), "a member's bits depend on its group"
                assert g0 is None and _same_bits(v0, v3), "grad=None changes the value"
                for i in range(F):
                    gp.set_data(Xb[ds[i]], yb[ds[i]])
                    v, g = gp.loo_ard(theta[i], criterion=crit, sigma_f=mode)
                    assert _same_bits(v3[i], v), ("value of member", mode, crit, i, v3[i], v)
                    assert _same_bits(g3[i], g), ("gradient of member", mode, crit, i, g3[i], g)
            r = gp.loo_ard_batch(theta, first=1, sigma_f=mode, group=3, predictions=True, grad=None)
            # staging is exactly a division: loo_batch on the pre-divided data at ell = 1
            with S.GPR(kernel=kind) as pre:
                pre.upload_batch(np.stack([Xb[ds[i]] / ells[i] for i in range(F)]), np.stack([yb[ds[i]] for i in range(F)]), None, group=3)
                want = pre.loo_batch(np.ones(F), S.GPR._exp(theta[:, d]), sigma_f=mode, group=3, predictions=True)
            for k in ("nlpd", "sse", "mean", "var"):
                assert _same_bits(r[k], want[k]), ("predictions=True against loo_batch on pre-divided data", mode, k)


# ---- 3. two members of one group on the same data set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_members_of_one_group_share_a_data_set_and_differ_in_scales(S, kind):
    """F = 5 members on B = 2 data sets in groups of 3: members 0 and 2 share data set 0 within one group"""
    n, d, B, F = 129, 8, 2, 5
    Xb, yb, _, _, theta7, _ = _problem(n, d)
    theta = theta7[:F]
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        v, g = gp.loo_ard_batch(theta, group=3)
        for i in range(F):
            gp.set_data(Xb[i % B], yb[i % B])
            v1, g1 = gp.loo_ard(theta[i])
            assert _same_bits(v[i], v1) and _same_bits(g[i], g1), (i, v[i], v1)
    assert not _same_bits(v[0], v[2]) and not _same_bits(g[0], g[2])      # the same data set at other scales is another fit


# ---- 4. equal scales: the components add up to the isotropic derivatives ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_equal_scales_add_up_to_the_isotropic_batch_gradient(S, kind):
    n, d, B, F = 129, 8, 2, 5
    Xb, yb, _, _, _, _ = _problem(n, d)
    ell = np.sqrt(d) * np.array([1.0, 0.6, 1.5, 0.8, 1.2])
    sn = np.array([SNS[i % 2] for i in range(F)])
    th_ard = np.concatenate([np.repeat(np.log(ell)[:, None], d, axis=1), np.log(sn)[:, None]], axis=1)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        got = {(mode, crit): gp.loo_ard_batch(th_ard, criterion=crit, sigma_f=mode, group=3) for mode in MODES for crit in CRITERIA}
        iso = {mode: gp.loo_batch(ell, sn, sigma_f=mode, group=3, predictions=False, grad=True) for mode in MODES}
    for i in range(F):
        X, y = Xb[i % B], yb[i % B]
        for mode in MODES:
            ra = _reference_of(kind, X, y, np.full(d, ell[i]), sn[i])[mode]
            for crit in CRITERIA:
                key = crit[4:]
                v, g = got[(mode, crit)]
                S_ = ra[0][key + "_S"]
                scale = np.array([np.sum(S_[:d]), S_[d]])
                ga, gb = ra[0][key + "_grad"], ra[2][key + "_grad"]
                spread = np.abs(np.array([np.sum(ga[:d]) - np.sum(gb[:d]), ga[d] - gb[d]])) / scale     # the reference's own error on the sums
                _check("%s %s %s member %d (sum_k d/dlog l_k, d/dlog sn~)" % (kind, mode, crit, i), np.array([np.sum(g[i, :d]), g[i, d]]),
                       iso[mode][key + "_grad"][i], scale, spread)
                assert abs(v[i] - iso[mode][key][i]) <= 1e-10 * abs(iso[mode][key][i]), (mode, crit, i)


# ---- 5. failing members leave their group mates alone ----------------------------------------------------------------------------------------------
def test_failing_members_get_inf_and_their_mate_keeps_its_bits(S):
    n, d, B = 200, 8, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20260900 + b)
    Xb[1, 1] = Xb[1, 0]                                      # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    theta = np.stack([np.concatenate([np.log(ard_scales(d, 20260910 + i)), [np.log(1e-2)]]) for i in range(B)])
    theta[1, d] = -np.inf                                    # sn~ = 0 on the singular data set, as test_loo_ard_non_spd_gives_inf builds it
    theta[2, 3] = 800.0                                      # exp overflows
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for crit in CRITERIA:
            r = gp.loo_ard_batch(theta, criterion=crit, group=3, predictions=True)
            alone = gp.loo_ard_batch(theta[:1], criterion=crit, group=3, predictions=True)
            v0, g0 = gp.loo_ard_batch(theta, criterion=crit, group=3, grad=None)
            for k in ("value", "nlpd", "sse"):
                assert np.all(np.isposinf(r[k][1:])), (crit, k, r[k])
                assert np.isfinite(r[k][0]) and _same_bits(r[k][0], alone[k][0]), (crit, k)
            assert np.all(np.isposinf(r["grad"][1:])) and np.all(np.isfinite(r["grad"][0])), r["grad"]
            assert np.all(np.isnan(r["mean"][1:])) and np.all(np.isnan(r["var"][1:]))
            assert _same_bits(r["grad"][0], alone["grad"][0]) and _same_bits(r["mean"][0], alone["mean"][0]) and _same_bits(r["var"][0], alone["var"][0])
            assert g0 is None and _same_bits(v0, r["value"])


# ---- 6, 7. the C ABI: leading dimensions and refusals -------------------------------------------------------------------------------------------------
def _abi_problem():
    n, d, B, F = 129, 5, 2, 5
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20261000 + b)
    ells = np.stack([ard_scales(d, 20261010 + i) for i in range(F)])
    sn = np.array([SNS[i % 2] for i in range(F)])
    return n, d, B, F, Xb, yb, np.concatenate([np.log(ells), np.log(sn)[:, None]], axis=1)


def test_abi_leading_dimensions(S, L):
    n, d, B, F, Xb, yb, theta = _abi_problem()
    pad, SENT = 3, -12345.678

    def wide(A, fill):
        out = np.full((A.shape[0], A.shape[1] + pad), fill)
        out[:, :A.shape[1]] = A
        return out

    with S.GPR(kernel="matern52") as gp:
        lib, h, kid = gp._lib, gp._h, gp._kid
        gp.upload_batch(Xb, yb, None, group=3)
        gp.set_option("group", 3)
        for mode in (0, 1):
            for crit in (0, 1):
                sc, grad, mean, var = np.zeros((F, 2)), np.zeros((F, d + 1)), np.zeros((F, n)), np.zeros((F, n))
                assert lib.sigp_loo_grad_ard_batch(h, 1, F, kid, L.ptr(theta), d + 1, d + 1, mode, crit, L.ptr(mean), L.ptr(var), n, L.ptr(sc), L.ptr(grad), d + 1) == L.OK
                assert np.all(np.isfinite(sc)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(mean)) and np.all(var > 0)
                # wide rows: NaN in the gaps of theta, a sentinel in the gaps of the outputs
                thw = wide(theta, np.nan)
                scw, gradw, meanw, varw = np.zeros((F, 2)), np.full((F, d + 1 + pad), SENT), np.full((F, n + pad), SENT), np.full((F, n + pad), SENT)
                assert lib.sigp_loo_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, mode, crit, L.ptr(meanw), L.ptr(varw), n + pad, L.ptr(scw), L.ptr(gradw),
                                                   d + 1 + pad) == L.OK
                assert _same_bits(scw, sc) and _same_bits(gradw[:, :d + 1], grad) and np.all(gradw[:, d + 1:] == SENT)
                assert _same_bits(meanw[:, :n], mean) and _same_bits(varw[:, :n], var) and np.all(meanw[:, n:] == SENT) and np.all(varw[:, n:] == SENT)
                # no gradient, no predictions: the same scores, nothing else written
                gradw[:] = SENT
                sc0 = np.zeros((F, 2))
                assert lib.sigp_loo_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, mode, crit, None, None, 0, L.ptr(sc0), None, 0) == L.OK
                assert _same_bits(sc0, sc) and np.all(gradw == SENT)


def test_what_the_c_entry_refuses(S, L):
    n, d, B, F, Xb, yb, theta = _abi_problem()
    sc, grad, mean, var = np.zeros((F, 2)), np.zeros((F, d + 1)), np.zeros((F, n)), np.zeros((F, n))

    def call(gp, first=0, count=F, kid=None, th=theta, ntheta=d + 1, ldtheta=d + 1, mode=0, crit=0, mean_=None, var_=None, nstride=n, score=sc, grad_=grad, ldgrad=d + 1):
        return gp._lib.sigp_loo_grad_ard_batch(gp._h, first, count, gp._kid if kid is None else kid, L.ptr(th), ntheta, ldtheta, mode, crit, L.ptr(mean_), L.ptr(var_), nstride,
                                               L.ptr(score), L.ptr(grad_), ldgrad)

    with S.GPR(kernel="rbf") as gp:
        assert call(gp) == L.BAD_ARG                                                        # before sigp_batch_upload
        gp.upload_batch(Xb, yb, None, group=3)
        assert call(gp, mean_=mean, var_=var) == L.OK
        good = [sc.copy(), grad.copy(), mean.copy(), var.copy()]
        assert call(gp, count=0) == L.BAD_ARG and call(gp, count=-1) == L.BAD_ARG and call(gp, first=-1) == L.BAD_ARG
        assert call(gp, ntheta=d) == L.BAD_ARG and call(gp, ntheta=d + 2, ldtheta=d + 2) == L.BAD_ARG
        assert call(gp, ldtheta=d) == L.BAD_ARG                                             # ldtheta < ntheta
        assert call(gp, ldgrad=d) == L.BAD_ARG                                              # ldgrad < d + 1 with a gradient asked for
        assert call(gp, grad_=None, ldgrad=0) == L.OK                                       # ... and of no concern without one
        assert call(gp, mode=2) == L.BAD_ARG and call(gp, mode=-1) == L.BAD_ARG
        assert call(gp, crit=2) == L.BAD_ARG and call(gp, crit=-1) == L.BAD_ARG
        assert call(gp, mean_=mean) == L.BAD_ARG and call(gp, var_=var) == L.BAD_ARG         # one of mean / var alone
        assert call(gp, mean_=mean, var_=var, nstride=n - 1) == L.BAD_ARG
        assert call(gp, kid=0) == L.BAD_ARG                                                 # the reference kernel
        assert call(gp, score=None) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.loo_ard_batch(theta[:, :d])
        assert call(gp, mean_=mean, var_=var) == L.OK                                        # the handle goes on: the same bits as before the refusals
        for a, b in zip(good, [sc, grad, mean, var]):
            assert _same_bits(a, b)
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb[:, :1], yb[:, :1], None, group=3)
        assert call(gp) == L.BAD_ARG                                                        # n < 2: no leave-one-out
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        assert call(gp, kid=1) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.loo_ard_batch(theta)


# ---- 8. the single fits are what they were -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_single_fits_keep_their_bits_after_a_batch_call(S, kind):
    """``loo_ard`` and ``cv_ard`` on a handle that ran ``loo_ard_batch`` in between (shared workspaces, grown for a group) against a fresh
    handle: the zero-stride launches of the member kernels return the single fit's bits"""
    n, d = 129, 8
    Xb, yb, _, _, theta, ds = _problem(n, d)
    X, y, th = Xb[0], yb[0], theta[0]

    def singles(gp):
        out = []
        for mode in MODES:
            for crit in CRITERIA:
                r = gp.loo_ard(th, criterion=crit, sigma_f=mode, predictions=True)
                c = gp.cv_ard(th, 5, criterion="cv_" + crit[4:], sigma_f=mode, predictions=True)
                out += [r[k] for k in ("value", "grad", "mean", "var")] + [c[k] for k in ("value", "grad", "mean", "var")]
        return out

    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        fresh = singles(gp)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        before = singles(gp)
        gp.upload_batch(Xb, yb, None, group=3)
        v, g = gp.loo_ard_batch(theta, first=1, group=3)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
        gp.set_data(X, y)
        after = singles(gp)
    for i, (a, b, c) in enumerate(zip(fresh, before, after)):
        assert np.all(np.isfinite(a)) and _same_bits(a, b) and _same_bits(a, c), i


# ---- 9. the lockstep optimiser ---------------------------------------------------------------------------------------------------------------------
def _relevance_years(B=3):
    """the relevance problem of tests/test_hip_loo_ard.py (y bends along x_1, leans on x_2, ignores x_3), B years of it"""
    n, d = 96, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        rng = np.random.default_rng(20251900 + b)
        Xb[b] = rng.standard_normal((n, d))
        yb[b] = np.sin(1.5 * Xb[b, :, 0]) + 0.5 * Xb[b, :, 1] + 0.1 * rng.standard_normal(n)
    return Xb, yb, d, np.log([np.sqrt(3.0)] * d + [1e-2])


def test_optimize_ard_batch_finds_the_irrelevant_feature(S):
    Xb, yb, d, th0 = _relevance_years()
    B = len(Xb)
    with S.GPR(kernel="rbf") as gp:
        res = gp.optimize_ard_batch(Xb, yb, th0, criterion="loo_nlpd", group=4)
        res2 = gp.optimize_ard_batch(Xb, yb, np.log([np.sqrt(3.0), 1e-2]), group=4)                       # log l repeated; loo_nlpd by default
        multi = gp.optimize_ard_batch(Xb, yb, np.tile(th0, (2 * B, 1)), group=4)                          # two starts per data set
        ml = gp.optimize_ard_batch(Xb, yb, th0, criterion="nlml", group=4)
        ml0 = gp.optimize_batch(Xb, yb, th0, group=4, ard=True)
        with pytest.raises(ValueError, match="optimize_ard"):
            gp.optimize_batch(Xb, yb, th0, group=4, ard=True, criterion="loo_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_ard_batch(Xb, yb, th0[:3], group=4)
        with pytest.raises(ValueError):
            gp.optimize_ard_batch(Xb, yb, th0, criterion="cv_nlpd")
        # the single-handle optimiser from the same start, without a box as the lockstep driver has none
        single = []
        for b in range(B):
            gp.set_data(Xb[b], yb[b])
            single.append(gp.optimize_ard(th0, criterion="loo_nlpd", method="L-BFGS-B"))
    assert res["x"].shape == (B, d + 1) and multi["x"].shape == (2 * B, d + 1) and res["fun"].shape == (B,)
    assert np.all(res["converged"]) and np.all(multi["converged"]), (res["converged"], res["jac"])
    # The leave-one-out density of such a year may have several basins, and two local optimisers from one start need not end in the same
    # one.  Which years can be compared is decided by the reference alone: those where SciPy's L-BFGS-B on the closed form ends at the same
    # value with and without the box of test_hip_loo_ard's relevance problem (1e-6 relative) -- an interior optimum the start leads to
    # whatever the step rule.  On these the lockstep value, evaluated on the host, is within the nlML twin's bound of optimize_ard's.
    bounds = [(-3.0, 5.0)] * d + [(-12.0, 3.0)]
    sample = []
    for b in range(B):
        fb = loo_objective("rbf", Xb[b], yb[b])
        boxed, free = minimize(fb, th0, jac=True, method="L-BFGS-B", bounds=bounds), minimize(fb, th0, jac=True, method="L-BFGS-B")
        if abs(boxed.fun - free.fun) <= 1e-6 * abs(free.fun):
            sample.append(b)
        at, at_single = fb(res["x"][b])[0], fb(single[b].x)[0]
        print("year %d%s: lockstep %.12g at %s in %d steps (closed form there: %.12g); optimize_ard %.12g at %s (closed form there: %.12g); reference boxed %.12g, free %.12g"
              % (b, " (sample)" if b in sample else "", res["fun"][b], res["x"][b], res["nit"][b], at, single[b].fun, single[b].x, at_single, boxed.fun, free.fun))
        if b in sample:
            assert abs(at - res["fun"][b]) <= 1e-8 * abs(at), (b, at, res["fun"][b])
            assert at <= at_single + 1e-6 * abs(at_single), (b, at, at_single)
    assert sample, "no year with an interior optimum: change the seeds"
    for b in range(B):
        assert res["fun"][b] < loo_objective("rbf", Xb[b], yb[b])(th0)[0]
    assert np.all(res["x"][:, 2] > res["x"][:, 0]) and np.all(res["x"][:, 2] > res["x"][:, 1])      # the irrelevant feature's scale above the relevant ones'
    assert _same_bits(res2["x"], res["x"]) and _same_bits(res2["fun"], res["fun"])
    assert _same_bits(multi["x"][:B], res["x"]) and _same_bits(multi["x"][B:], res["x"]) and _same_bits(multi["fun"][B:], multi["fun"][:B])
    assert _same_bits(ml["x"], ml0["x"]) and _same_bits(ml["fun"], ml0["fun"])


# ---- 10. the profile entries of one call -------------------------------------------------------------------------------------------------------------
def test_loo_ard_batch_profile_entries(S):
    """One call, one group of nb = 3 members at n = 300 (n_pad = 384, T = 3), d = 8, RBF.  Counts derived from the driver's sequence:
    the KBUILD class holds the staging launch and the group's covariance build; the MLII class holds, per group, inv_factor (1 entry),
    the row pass (1), and for a gradient kinv_lower (1), the n^2 passes (1), the product M (1), the tile pass with its finish (1): the
    entries of ``loo_ard`` (tests/test_hip_loo_ard.py: 2 without a gradient, 6 with), whatever the number of members.  Flops and bytes
    are the single entry's x nb: from the single call on the same handle."""
    n, d, nb = 300, 8, 3
    Xb, yb, _, _, theta, _ = _problem(n, d)
    got = {}
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=nb)
        gp.loo_ard_batch(theta[:nb], group=nb)                 # (allocations out of the way)
        for name, kw in (("value_only", dict(grad=None)), ("gradient", dict())):
            gp.profile_reset()
            gp.loo_ard_batch(theta[:nb], group=nb, **kw)
            p = gp.profile_get()
            got[name] = {k: (p[k]["launches"], p[k]["flops"], p[k]["bytes"]) for k in ("kbuild", "mlii")}
            print("%s: %r" % (name, got[name]))
        gp.set_data(Xb[0], yb[0])
        single = {}
        for name, kw in (("value_only", dict(grad=None)), ("gradient", dict())):
            gp.profile_reset()
            gp.loo_ard(theta[0], **kw)
            p = gp.profile_get()["mlii"]
            single[name] = (p["launches"], p["flops"], p["bytes"])
    assert got["value_only"]["mlii"][0] == 2 and got["gradient"]["mlii"][0] == 6, got
    assert got["value_only"]["kbuild"][0] == 2 and got["gradient"]["kbuild"][0] == 2, got       # the staging and the covariance build
    for name in ("value_only", "gradient"):
        assert single[name][0] == got[name]["mlii"][0]
        assert got[name]["mlii"][1] == nb * single[name][1] and got[name]["mlii"][2] == nb * single[name][2], (name, got[name], single[name])
    n_pad, dp, ride = 384, 64, 128
    stage = (float(nb * (n_pad + ride) * d), 16.0 * nb * ((n_pad + ride) * dp + n_pad))                 # ard_stage_group's entry
    build = (nb * (n * n / 2 * (3.0 * d + 20)), nb * (8.0 * n * d + 4.0 * n * (n + 1)))                   # build_cov's entry for nb members
    for name in ("value_only", "gradient"):
        assert got[name]["kbuild"][1:] == (stage[0] + build[0], stage[1] + build[1]), (name, got[name]["kbuild"], stage, build)
