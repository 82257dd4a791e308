"""GPU tier of the per-feature (ARD) gradients of the leave-block-out scores in lockstep groups: ``GPR.cv_ard_batch``,
``GPR.cv_objective_batch``, ``GPR.optimize_cv_batch`` and the C entry point sigp_cv_grad_ard_batch.

Reference and error convention are those of tests/test_hip_cv_ard.py: the per-direction NumPy closed form of tests/test_cv_ard_host.py by
two routes to K~^-1, every gradient error measured against the per-component scale S, the device within max(1e-8, 10 x spread) where
spread is the disagreement of the two routes; a case counts only when spread <= 1e-8 (``_check`` asserts it: none may be dropped; on the
shapes below the worst spread is 2.1e-13).  Problems are those of tests/test_hip_loo_ard_batch.py: B = 2 data sets, F = 7 members with
scales of their own, sn~ alternating 1e-2 / 3e-2, first = 1; scales belong to a fit, not to a data set."""
import functools

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_cv_ard_host import cv_ard_closed_form
from test_cv_host import cv_closed_form
from test_hip_cv_ard import CRITERIA, KINDS, MODES, _check, _reference_of
from test_hip_loo_ard_batch import SNS, _problem

pytestmark = pytest.mark.gpu


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
def _references(kind, n, d, block, gap):
    """per member {mode: (closed form, {criterion: spread}, other route)}: computed once, shared by the tests below"""
    Xb, yb, ells, sn, _, ds = _problem(n, d)
    return [_reference_of(kind, Xb[ds[i]], yb[ds[i]], ells[i], block, gap, sn[i]) for i in range(len(ds))]


# ---- 1. every member against the closed form ---------------------------------------------------------------------------------------------------
# (n, d, block, gap): the minimum; clipped windows; windows across row 128; full 128-row windows with clipped ends; w = 128 exactly with a
# ragged last fold; block-diagonal B of full blocks; d past one 64-column pad; 400 folds > 1024 / 3: the groups of 3 take two passes, the
# tail group of one member takes one
SHAPES = [(2, 1, 1, 0), (37, 3, 5, 2), (129, 8, 16, 8), (130, 8, 64, 32), (300, 8, 100, 14), (300, 8, 128, 0), (200, 65, 7, 3), (400, 4, 1, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,block,gap", SHAPES)
def test_members_equal_the_closed_form(S, kind, n, d, block, gap):
    """B = 2 data sets, F = 7 members in groups of 3, 3, 1 (a partial last group), first = 1; both criteria, both sigma modes"""
    Xb, yb, ells, sn, theta, ds = _problem(n, d)
    refs = _references(kind, n, d, block, gap)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                key = crit[3:]
                r = gp.cv_ard_batch(theta, block, gap=gap, first=1, criterion=crit, sigma_f=mode, group=3, predictions=True)
                assert set(r) == {"value", "grad", "mean", "var", "nlpd", "sse"}
                assert r["value"].shape == (7,) and r["grad"].shape == (7, d + 1) and r["mean"].shape == (7, n) and r["var"].shape == (7, n)
                assert r["nlpd"].shape == (7,) and r["sse"].shape == (7,)
                assert _same_bits(r["value"], r[key])
                for i in range(7):
                    a, spread, _ = refs[i][mode]
                    _check("%s n=%d d=%d block=%d gap=%d %s %s member %d" % (kind, n, d, block, gap, mode, crit, i), r["grad"][i], a[key + "_grad"], a[key + "_S"],
                           spread[crit])
                    for k in ("nlpd", "sse"):
                        assert abs(float(r[k][i]) - a[k]) <= 1e-8 * abs(a[k]), (mode, crit, i, k, r[k][i], a[k])
                    if crit == CRITERIA[0]:           # (the predictions do not depend on the criterion)
                        U = Xb[ds[i]] / ells[i]
                        want = cv_closed_form(O.cov_unit(kind, U, U, 1.0) + sn[i] * np.eye(n), yb[ds[i]], block, gap, mode)
                        assert np.max(np.abs(r["mean"][i] - want["mean"])) <= 1e-8 * np.max(np.abs(yb[ds[i]])), (mode, i)     # (the scales of test_hip_cv.py)
                        assert np.all(np.abs(r["var"][i] - want["var"]) <= 1e-8 * want["var"]), (mode, i)
        v0, g0 = gp.cv_ard_batch(theta, block, gap=gap, first=1, group=3, grad=None)
        assert g0 is None and v0.shape == (7,)


# ---- 2. the bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,block,gap", [(129, 8, 16, 8), (300, 8, 5, 0)])
def test_members_have_the_bits_of_the_single_fit_whatever_the_group(S, kind, n, d, block, gap):
    Xb, yb, _, sn, theta, ds = _problem(n, d)
    F = len(ds)
    ells = np.stack([S.GPR._exp(t[:d]) for t in theta])        # the library's own exp(theta): the scales the staging divides by
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                kw = dict(gap=gap, first=1, criterion=crit, sigma_f=mode)
                r3 = gp.cv_ard_batch(theta, block, group=3, predictions=True, **kw)
                v3, g3 = r3["value"], r3["grad"]
                v3b, g3b = gp.cv_ard_batch(theta, block, group=3, **kw)
                v1, g1 = gp.cv_ard_batch(theta, block, group=1, **kw)
                v0, g0 = gp.cv_ard_batch(theta, block, group=3, grad=None, **kw)
                assert _same_bits(v3, v3b) and _same_bits(g3, g3b), "two calls differ"
                assert _same_bits(v3, v1) and _same_bits(g3, g1), "a member's bits depend on its group"
                assert g0 is None and _same_bits(v0, v3), "grad=None changes the value"
                for i in range(F):
                    gp.set_data(Xb[ds[i]], yb[ds[i]])
                    s = gp.cv_ard(theta[i], block, gap=gap, criterion=crit, sigma_f=mode, predictions=True)
                    assert _same_bits(v3[i], s["value"]), ("value of member", mode, crit, i, v3[i], s["value"])
                    assert _same_bits(g3[i], s["grad"]), ("gradient of member", mode, crit, i, g3[i], s["grad"])
                    assert _same_bits(r3["mean"][i], s["mean"]) and _same_bits(r3["var"][i], s["var"]), ("predictions of member", mode, crit, i)
            r = gp.cv_ard_batch(theta, block, gap=gap, first=1, sigma_f=mode, group=3, predictions=True, grad=None)
            assert r["grad"] is None
            # staging is exactly a division: cv_batch on the pre-divided data at ell = 1
            with S.GPR(kernel=kind) as pre:
                pre.upload_batch(np.stack([Xb[ds[i]] / ells[i] for i in range(F)]), np.stack([yb[ds[i]] for i in range(F)]), None, group=3)
                want = pre.cv_batch(np.ones(F), S.GPR._exp(theta[:, d]), block, gap=gap, sigma_f=mode, group=3, predictions=True)
            for k in ("nlpd", "sse", "mean", "var"):
                assert _same_bits(r[k], want[k]), ("predictions=True against cv_batch on pre-divided data", mode, k)


# ---- 3. the split into passes does not show in the bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_pass_split_does_not_change_the_bits(S, kind):
    """(300, 8, 1, 3) with group = 8: ONE group of 7 members, 1024 / 7 = 146 folds of each per pass, three passes -- every entry of B adds
    terms of up to 7 folds, some of them from two passes; the single fit works its 300 folds off in one pass"""
    n, d, block, gap = 300, 8, 1, 3
    Xb, yb, _, _, theta, ds = _problem(n, d)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=8)
        got = {crit: gp.cv_ard_batch(theta, block, gap=gap, first=1, criterion=crit, group=8, predictions=True) for crit in CRITERIA}
        for i in range(len(ds)):
            gp.set_data(Xb[ds[i]], yb[ds[i]])
            for crit in CRITERIA:
                s = gp.cv_ard(theta[i], block, gap=gap, criterion=crit, predictions=True)
                for k in ("value", "grad", "mean", "var"):
                    assert _same_bits(got[crit][k][i], s[k]), (crit, i, k)


# ---- 4. two members of one group on the same data set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_members_of_one_group_share_a_data_set_and_differ_in_scales(S, kind):
    """F = 5 members on B = 2 data sets in groups of 3: members 0 and 2 share data set 0 within one group"""
    n, d, B, F = 129, 8, 2, 5
    Xb, yb, _, _, theta7, _ = _problem(n, d)
    theta = theta7[:F]
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        v, g = gp.cv_ard_batch(theta, 5, gap=1, group=3)
        for i in range(F):
            gp.set_data(Xb[i % B], yb[i % B])
            v1, g1 = gp.cv_ard(theta[i], 5, gap=1)
            assert _same_bits(v[i], v1) and _same_bits(g[i], g1), (i, v[i], v1)
    assert not _same_bits(v[0], v[2]) and not _same_bits(g[0], g[2])      # the same data set at other scales is another fit


# ---- 5. block = 1 without a gap is leave-one-out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_block_one_without_a_gap_equals_loo_ard_batch(S, kind):
    """two device results meet: twice the bound"""
    n, d = 129, 8
    Xb, yb, _, _, theta, ds = _problem(n, d)
    refs = _references(kind, n, d, 1, 0)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for mode in MODES:
            for crit in CRITERIA:
                key = crit[3:]
                v, g = gp.cv_ard_batch(theta, 1, first=1, criterion=crit, sigma_f=mode, group=3)
                v1, g1 = gp.loo_ard_batch(theta, first=1, criterion="loo_" + key, sigma_f=mode, group=3)
                assert np.all(np.abs(v - v1) <= 1e-10 * np.abs(v1)), (mode, crit, v, v1)
                for i in range(len(ds)):
                    a, spread, _ = refs[i][mode]
                    _check("%s %s %s member %d (cv_ard_batch(1) against loo_ard_batch)" % (kind, mode, crit, i), g[i], g1[i], a[key + "_S"], spread[crit], factor=2.0)


# ---- 6. one common length scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_cv_objective_batch_has_the_bits_of_cv_objective(S, kind):
    n, d, block, gap = 129, 8, 5, 1
    Xb, yb, _, sn, _, ds = _problem(n, d)
    F = len(ds)
    theta = np.stack([np.log(np.sqrt(d) * np.array([1.0, 0.6, 1.5, 0.8, 1.2, 0.7, 1.1])), np.log(sn)], axis=1)
    with S.GPR(kernel=kind) as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        got = {(mode, crit): gp.cv_objective_batch(theta, block, gap=gap, first=1, criterion=crit, sigma_f=mode, group=3) for mode in MODES for crit in CRITERIA}
        for i in range(F):
            gp.set_data(Xb[ds[i]], yb[ds[i]])
            for mode in MODES:
                for crit in CRITERIA:
                    v, g = got[(mode, crit)]
                    assert v.shape == (F,) and g.shape == (F, 2)
                    v1, g1 = gp.cv_objective(theta[i], block, gap=gap, criterion=crit, sigma_f=mode)
                    assert _same_bits(v[i], v1) and _same_bits(g[i], g1), (mode, crit, i, v[i], v1, g[i], g1)


# ---- 7. failing members leave their group mates alone ----------------------------------------------------------------------------------------------
def test_failing_members_get_inf_and_their_mate_keeps_its_bits(S):
    """the construction of tests/test_hip_loo_ard_batch.py: duplicate rows with sn~ = 0; an overflowing exp"""
    n, d, B = 200, 8, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20260900 + b)
    Xb[1, 1] = Xb[1, 0]                                      # duplicate rows: K~ is singular at sn~ = 0 (second pivot exactly 0)
    theta = np.stack([np.concatenate([np.log(ard_scales(d, 20260910 + i)), [np.log(1e-2)]]) for i in range(B)])
    theta[1, d] = -np.inf                                    # sn~ = 0 on the singular data set
    theta[2, 3] = 800.0                                      # exp overflows
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        for crit in CRITERIA:
            r = gp.cv_ard_batch(theta, 5, gap=1, criterion=crit, group=3, predictions=True)
            alone = gp.cv_ard_batch(theta[:1], 5, gap=1, criterion=crit, group=3, predictions=True)
            v0, g0 = gp.cv_ard_batch(theta, 5, gap=1, criterion=crit, group=3, grad=None)
            for k in ("value", "nlpd", "sse"):
                assert np.all(np.isposinf(r[k][1:])), (crit, k, r[k])
                assert np.isfinite(r[k][0]) and _same_bits(r[k][0], alone[k][0]), (crit, k)
            assert np.all(np.isposinf(r["grad"][1:])) and np.all(np.isfinite(r["grad"][0])), r["grad"]
            assert np.all(np.isnan(r["mean"][1:])) and np.all(np.isnan(r["var"][1:]))
            assert _same_bits(r["grad"][0], alone["grad"][0]) and _same_bits(r["mean"][0], alone["mean"][0]) and _same_bits(r["var"][0], alone["var"][0])
            assert g0 is None and _same_bits(v0, r["value"])
        f, g = gp.cv_objective_batch(np.array([[np.log(3.0), np.log(1e-2)], [0.0, 0.0], [800.0, np.log(1e-2)]]), 5, gap=1, group=3)
        assert np.isfinite(f[0]) and np.isfinite(f[1]) and np.isposinf(f[2]) and np.all(np.isposinf(g[2])) and np.all(np.isfinite(g[:2]))


# ---- 8. the C ABI: leading dimensions and refusals -------------------------------------------------------------------------------------------------
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
    pad, SENT, block, gap = 3, -12345.678, 16, 8

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
                assert lib.sigp_cv_grad_ard_batch(h, 1, F, kid, L.ptr(theta), d + 1, d + 1, block, gap, mode, crit, L.ptr(mean), L.ptr(var), n, L.ptr(sc), L.ptr(grad),
                                                  d + 1) == L.OK
                assert np.all(np.isfinite(sc)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(mean)) and np.all(var > 0)
                # wide rows: NaN in the gaps of theta, a sentinel in the gaps of the outputs
                thw = wide(theta, np.nan)
                scw, gradw, meanw, varw = np.zeros((F, 2)), np.full((F, d + 1 + pad), SENT), np.full((F, n + pad), SENT), np.full((F, n + pad), SENT)
                assert lib.sigp_cv_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, block, gap, mode, crit, L.ptr(meanw), L.ptr(varw), n + pad, L.ptr(scw),
                                                  L.ptr(gradw), d + 1 + pad) == L.OK
                assert _same_bits(scw, sc) and _same_bits(gradw[:, :d + 1], grad) and np.all(gradw[:, d + 1:] == SENT)
                assert _same_bits(meanw[:, :n], mean) and _same_bits(varw[:, :n], var) and np.all(meanw[:, n:] == SENT) and np.all(varw[:, n:] == SENT)
                # no gradient, no predictions: the same scores, nothing else written
                gradw[:] = SENT
                sc0 = np.zeros((F, 2))
                assert lib.sigp_cv_grad_ard_batch(h, 1, F, kid, L.ptr(thw), d + 1, d + 1 + pad, block, gap, mode, crit, None, None, 0, L.ptr(sc0), None, 0) == L.OK
                assert _same_bits(sc0, sc) and np.all(gradw == SENT)


def test_what_the_c_entry_refuses(S, L):
    n, d, B, F, Xb, yb, theta = _abi_problem()
    sc, grad, mean, var = np.zeros((F, 2)), np.zeros((F, d + 1)), np.zeros((F, n)), np.zeros((F, n))

    def call(gp, first=0, count=F, kid=None, th=theta, ntheta=d + 1, ldtheta=d + 1, block=5, gap=1, mode=0, crit=0, mean_=None, var_=None, nstride=n, score=sc, grad_=grad,
             ldgrad=d + 1):
        return gp._lib.sigp_cv_grad_ard_batch(gp._h, first, count, gp._kid if kid is None else kid, L.ptr(th), ntheta, ldtheta, block, gap, mode, crit, L.ptr(mean_),
                                              L.ptr(var_), nstride, L.ptr(score), L.ptr(grad_), ldgrad)

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
        assert call(gp, block=0) == L.BAD_ARG and call(gp, gap=-1) == L.BAD_ARG              # the fold checks of sigp_cv
        assert call(gp, block=129, gap=0) == L.BAD_ARG and call(gp, block=5, gap=62) == L.BAD_ARG and call(gp, block=1, gap=129) == L.BAD_ARG     # block + 2 gap > 128
        with pytest.raises(ValueError):
            gp.cv_ard_batch(theta[:, :d], 5)
        with pytest.raises(ValueError):
            gp.cv_ard_batch(theta, 5, gap=62)
        assert call(gp, mean_=mean, var_=var) == L.OK                                        # the handle goes on: the same bits as before the refusals
        for a, b in zip(good, [sc, grad, mean, var]):
            assert _same_bits(a, b)
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb[:, :60], yb[:, :60], None, group=3)
        assert call(gp, nstride=60) == L.OK
        assert call(gp, block=60, gap=0) == L.BAD_ARG and call(gp, block=20, gap=20) == L.BAD_ARG      # a fold that leaves no training row
        with pytest.raises(ValueError):
            gp.cv_ard_batch(theta, 60)
        first_part = sc.copy()
        assert call(gp, nstride=60) == L.OK and _same_bits(first_part, sc)
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb[:, :1], yb[:, :1], None, group=3)
        assert call(gp, block=1, gap=0) == L.BAD_ARG                                        # n < 2: no cross-validation
    with S.GPR(kernel="rbf", dtype="f32") as gp:
        gp.upload_batch(Xb, yb, None, group=3)
        assert call(gp, kid=1) == L.BAD_ARG
        with pytest.raises(ValueError):
            gp.cv_ard_batch(theta, 5)


# ---- 9. the single fits are what they were -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_single_fits_keep_their_bits_after_a_batch_call(S, kind):
    """``loo_ard``, ``cv_ard``, ``cv`` and ``loo`` on a handle that ran ``cv_ard_batch`` in between (shared workspaces, grown and laid out for a
    group) against a fresh handle: the zero-stride launches of the member kernels return the single fit's bits"""
    n, d = 129, 8
    Xb, yb, _, _, theta, ds = _problem(n, d)
    X, y, th = Xb[0], yb[0], theta[0]

    def singles(gp):
        out = []
        for mode in MODES:
            for crit in CRITERIA:
                r = gp.loo_ard(th, criterion="loo_" + crit[3:], sigma_f=mode, predictions=True)
                c = gp.cv_ard(th, 16, gap=8, criterion=crit, sigma_f=mode, predictions=True)
                out += [r[k] for k in ("value", "grad", "mean", "var")] + [c[k] for k in ("value", "grad", "mean", "var")]
            cv, lo = gp.cv(16, 8, mode), gp.loo(mode)            # on the fit cv_ard left
            out += [cv["mean"], cv["var"], np.array([cv["nlpd"], cv["sse"]]), lo["mean"], lo["var"], np.array([lo["nlpd"], lo["sse"]])]
        return out

    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        fresh = singles(gp)
    with S.GPR(kernel=kind) as gp:
        gp.set_data(X, y)
        before = singles(gp)
        gp.upload_batch(Xb, yb, None, group=3)
        v, g = gp.cv_ard_batch(theta, 16, gap=8, first=1, group=3)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
        gp.set_data(X, y)
        after = singles(gp)
    for i, (a, b, c) in enumerate(zip(fresh, before, after)):
        assert np.all(np.isfinite(a)) and _same_bits(a, b) and _same_bits(a, c), i


# ---- 10. the profile entries of one call -------------------------------------------------------------------------------------------------------------
def test_cv_ard_batch_profile_entries(S):
    """One call, one group of nb = 3 members at n = 300, block 5, gap 1 (60 folds of each member: one pass), d = 8, RBF.  The KBUILD class
    holds the staging launch and the group's covariance build; the MLII class holds the entries of ``cv_ard`` (tests/test_hip_cv_ard.py:
    the triangular inversion and four per pass; a gradient adds two per pass and five more), whatever the number of members.  Flops and
    bytes are the single call's x nb: from the single call on the same handle."""
    n, d, nb, block, gap = 300, 8, 3, 5, 1
    Xb, yb, _, _, theta, _ = _problem(n, d)
    got = {}
    with S.GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=nb)
        gp.cv_ard_batch(theta[:nb], block, gap=gap, group=nb)                 # (allocations out of the way)
        for name, kw in (("value_only", dict(grad=None)), ("gradient", dict())):
            gp.profile_reset()
            gp.cv_ard_batch(theta[:nb], block, gap=gap, group=nb, **kw)
            p = gp.profile_get()
            got[name] = {k: (p[k]["launches"], p[k]["flops"], p[k]["bytes"]) for k in ("kbuild", "mlii")}
            print("%s: %r" % (name, got[name]))
        gp.set_data(Xb[0], yb[0])
        single = {}
        for name, kw in (("value_only", dict(grad=None)), ("gradient", dict())):
            gp.profile_reset()
            gp.cv_ard(theta[0], block, gap=gap, **kw)
            p = gp.profile_get()["mlii"]
            single[name] = (p["launches"], p["flops"], p["bytes"])
            print("single %s: %r" % (name, single[name]))
    assert got["value_only"]["mlii"][0] == 1 + 4 and got["gradient"]["mlii"][0] == 1 + 4 + 2 + 5, got
    assert got["value_only"]["kbuild"][0] == 2 and got["gradient"]["kbuild"][0] == 2, got       # the staging and the covariance build
    for name in ("value_only", "gradient"):
        assert single[name][0] == got[name]["mlii"][0]
        assert got[name]["mlii"][1] == nb * single[name][1] and got[name]["mlii"][2] == nb * single[name][2], (name, got[name], single[name])


# ---- 11. the lockstep optimiser ---------------------------------------------------------------------------------------------------------------------
def _cv_objective(kind, X, y, block, gap=0, crit="nlpd", mode="refit"):
    """theta -> (value, grad [d + 1]) of a leave-block-out score by the closed form; (inf, inf) where K~ is not SPD or the result is not finite"""
    d = X.shape[1]

    def f(th):
        try:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                r = cv_ard_closed_form(kind, X, y, np.exp(th[:d]), np.exp(th[d]), block, gap, mode)
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        v, g = r[crit], r[crit + "_grad"]
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, np.full(d + 1, np.inf)
        return float(v), g
    return f


def _bending_years(B=3):
    """B years in the style of tests/test_hip_loo_ard_batch.py's relevance problem (n = 96, d = 3), with y bending along x_1 AND x_2 and
    ignoring x_3.  In that problem y leans on x_2 linearly, and a linear dependence wants a long scale of its own: the closed form alone
    (SciPy's L-BFGS-B and ``bfgs_lockstep`` on it) puts l_2 above l_3 in two of its three years under the leave-block-out density.  Here
    both relevant features bend y, and the closed form alone puts l_3 above both in every year."""
    n, d = 96, 3
    Xb, yb = np.zeros((B, n, d)), np.zeros((B, n))
    for b in range(B):
        rng = np.random.default_rng(20263100 + b)
        Xb[b] = rng.standard_normal((n, d))
        yb[b] = np.sin(1.5 * Xb[b, :, 0]) + np.cos(1.2 * Xb[b, :, 1]) + 0.1 * rng.standard_normal(n)
    return Xb, yb, d, np.log([np.sqrt(3.0)] * d + [1e-2])


def test_optimize_cv_batch_finds_the_irrelevant_feature(S):
    Xb, yb, d, th0 = _bending_years()
    B, block = len(Xb), 5
    th2 = np.log([np.sqrt(3.0), 1e-2])
    with S.GPR(kernel="rbf") as gp:
        res = gp.optimize_cv_batch(Xb, yb, th0, block, criterion="cv_nlpd", group=4)
        again = gp.cv_ard_batch(res["x"], block, group=4)
        res2 = gp.optimize_cv_batch(Xb, yb, th2, block, group=4)                                         # log l repeated; cv_nlpd by default
        multi = gp.optimize_cv_batch(Xb, yb, np.tile(th0, (2 * B, 1)), block, group=4)                   # two starts per data set
        iso = gp.optimize_cv_batch(Xb, yb, th2, block, ard=False, group=4)
        with pytest.raises(ValueError, match="optimize_ard"):
            gp.optimize_batch(Xb, yb, th0, group=4, ard=True, criterion="cv_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_ard_batch(Xb, yb, th0, criterion="cv_nlpd")
        with pytest.raises(ValueError):
            gp.optimize_cv_batch(Xb, yb, th0[:3], block, group=4)
        # the single-handle optimiser from the same start, without a box as the lockstep driver has none
        single = []
        for b in range(B):
            gp.set_data(Xb[b], yb[b])
            single.append(gp.optimize_ard(th0, criterion="cv_nlpd", block=block, method="L-BFGS-B"))
    assert res["x"].shape == (B, d + 1) and multi["x"].shape == (2 * B, d + 1) and res["fun"].shape == (B,) and res["jac"].shape == (B, d + 1)
    assert iso["x"].shape == (B, 2) and iso["jac"].shape == (B, 2)
    assert np.all(res["converged"]) and np.all(multi["converged"]) and np.all(iso["converged"]), (res["converged"], res["jac"], iso["converged"])
    assert _same_bits(again[0], res["fun"]) and _same_bits(again[1], res["jac"])                      # fun and jac are cv_ard_batch's at x
    # Which years can be compared with the single-handle optimiser is decided by the reference alone, as in tests/test_hip_loo_ard_batch.py:
    # those where SciPy's L-BFGS-B on the closed form ends at the same value with and without the box (1e-6 relative).
    bounds = [(-3.0, 5.0)] * d + [(-12.0, 3.0)]
    sample = []
    for b in range(B):
        fb = _cv_objective("rbf", Xb[b], yb[b], block)
        boxed, free = minimize(fb, th0, jac=True, method="L-BFGS-B", bounds=bounds), minimize(fb, th0, jac=True, method="L-BFGS-B")
        if abs(boxed.fun - free.fun) <= 1e-6 * abs(free.fun):
            sample.append(b)
        x = res["x"][b]
        ra = cv_ard_closed_form("rbf", Xb[b], yb[b], np.exp(x[:d]), np.exp(x[d]), block, 0, "refit", "inv")
        rb = cv_ard_closed_form("rbf", Xb[b], yb[b], np.exp(x[:d]), np.exp(x[d]), block, 0, "refit", "chol")
        at, at_single = ra["nlpd"], fb(single[b].x)[0]
        print("year %d%s: lockstep %.12g at %s in %d steps (closed form there: %.12g); optimize_ard %.12g at %s (closed form there: %.12g); reference boxed %.12g, free %.12g"
              % (b, " (sample)" if b in sample else "", res["fun"][b], x, res["nit"][b], at, single[b].fun, single[b].x, at_single, boxed.fun, free.fun))
        assert abs(at - res["fun"][b]) <= 1e-8 * abs(at), (b, at, res["fun"][b])
        _check("year %d: jac at the returned x" % b, res["jac"][b], ra["nlpd_grad"], ra["nlpd_S"], np.abs(ra["nlpd_grad"] - rb["nlpd_grad"]) / ra["nlpd_S"])
        assert res["fun"][b] < fb(th0)[0]
        if b in sample:
            assert at <= at_single + 1e-6 * abs(at_single), (b, at, at_single)
        # one common length scale: the summed closed-form gradient at equal scales, on sum_k S_k and S_noise
        xi = iso["x"][b]
        pa = cv_ard_closed_form("rbf", Xb[b], yb[b], np.full(d, np.exp(xi[0])), np.exp(xi[1]), block, 0, "refit", "inv")
        pb = cv_ard_closed_form("rbf", Xb[b], yb[b], np.full(d, np.exp(xi[0])), np.exp(xi[1]), block, 0, "refit", "chol")
        two = lambda r: np.array([np.sum(r["nlpd_grad"][:d]), r["nlpd_grad"][d]])
        S2 = np.array([np.sum(pa["nlpd_S"][:d]), pa["nlpd_S"][d]])
        _check("year %d: ard=False, jac at the returned x" % b, iso["jac"][b], two(pa), S2, np.abs(two(pa) - two(pb)) / S2)
        assert abs(pa["nlpd"] - iso["fun"][b]) <= 1e-8 * abs(pa["nlpd"])
    assert sample, "no year with an interior optimum: change the seeds"
    assert np.all(res["x"][:, 2] > res["x"][:, 0]) and np.all(res["x"][:, 2] > res["x"][:, 1])      # the irrelevant feature's scale above the relevant ones'
    assert _same_bits(res2["x"], res["x"]) and _same_bits(res2["fun"], res["fun"])
    assert _same_bits(multi["x"][:B], res["x"]) and _same_bits(multi["x"][B:], res["x"]) and _same_bits(multi["fun"][B:], multi["fun"][:B])
