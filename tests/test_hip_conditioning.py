"""GPU tier: factorisation and solves on ILL-CONDITIONED covariance matrices, cond(K~) = 1e6 .. 1e14 -- the range between the easy matrices of
the parity tests and the exactly singular ones of the NOT_SPD tests, and the one the optimisers walk into (long length scale, small noise).

Every triangular solve on the device is a product with an explicitly inverted block (the 128 x 128 ``dinv`` blocks, U = L~^-T by recursive
doubling, 2048-column inverses in the fp32 engine).  Substitution is backward stable whatever the conditioning; a product with an inverse carries
an error proportional to cond of the inverted block, and on a smooth kernel over ordered inputs the leading 128-block is nearly as
ill-conditioned as the whole matrix.  The flat 1e-8 / 1e3 eps cond tolerances of the other files cannot see such a loss; these tests can.

Yardstick.  Every device quantity is compared with the SAME quantity computed by LAPACK in fp64 on the SAME fp64 matrix (read back from
the device), both measured against a long-double reference of that matrix (tests/hp_reference.py):

  independent of conditioning   rho = ||L L^T - K||_F / ||K||_F,  eta = ||y - K a||_inf / (||K||_inf ||a||_inf + ||y||_inf):
                                q_dev <= 16 max(q_lapack, u),  u = 2^-53
  proportional to cond          |q_dev - q_hp| <= 16 max(|q_lapack - q_hp|, u scale)   (max-norm over a vector quantity; scale = its size,
                                for mean_* and grad_l the size of the summed terms: input_sizes)
  growth                        ratio = q_dev / max(q_lapack, floor) at the hardest level <= 8 x the ratio at the control level
                                (a scalar's control ratio counts as at least 1: check_growth says why)

The margin 16: two correct blocked Choleskys differ by their summation order (LAPACK's own figures move 2-4 x between blockings and sizes);
a loss through an inverse shows as 1e2 .. 1e7.  It is stated, not tuned.  ``-s`` prints every figure; docs/EXPERIMENTS.md keeps the table.

The solved rows v = L~^-1 k* behind ``predict`` are not exposed by the Python surface, so their backward error cannot be formed; their
effect is measured through the predictive variance.  fp32 engine: ``predict`` off the ride-along path takes its variance from the fp32 factor
(include/sigp.h) and that variance is not held to fp64 bounds; its mean and the ride-along predictions come from the refined solution and are.
"""
import math

import numpy as np
import pytest

import hp_reference as H

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")]

MARGIN, GROWTH = 16.0, 8.0
# include/sigp.h, sigp_set_option: schedules / equivalent routes of the same factorisation
PATHS = {"default": {}, "panel_mode=0": {"panel_mode": 0}, "panel_mode=1,strip_min=1": {"panel_mode": 1, "strip_min": 1},
         "outer_blocks=1": {"outer_blocks": 1}, "outer_blocks=2": {"outer_blocks": 2}, "panel_chain=0": {"panel_chain": 0},
         "small/tiny_tile_threshold=1": {"small_tile_threshold": 1, "tiny_tile_threshold": 1}, "schedule=1": {"schedule": 1}}
SAME_BITS = ("panel_chain=0", "schedule=1")          # the header: "same factor bit for bit", "bit-identical results"
GEN5 = [0, 3, 193, 194, 196]                         # of family A's 200 general points: a training row, an interior point, -40, 55, a training row

A_GROUPS = [("A", kind, n) for kind in ("rbf", "matern52") for n in H.A_SIZES]
B_GROUPS = [("B", "spectrum", n) for n in H.B_SIZES]
LEVELS = {"A": H.A_LEVELS, "B": H.B_LEVELS}
CASES = [g + (lv,) for g in A_GROUPS + B_GROUPS for lv in LEVELS[g[0]]]
PATH_GROUPS = [g for g in A_GROUPS + B_GROUPS if g[2] >= 384]
PATH_CASES = [g + (lv,) for g in PATH_GROUPS for lv in LEVELS[g[0]]]
OTHER_PATHS = [p for p in PATHS if p != "default"]

_DEV, _REF, _MEASURED, _NEGATIVE = {}, {}, {}, {}

# THE FINDING (measured on an MI355X, docs/EXPERIMENTS.md "Conditioning"): on family A the factor's residual grows with cond of the
# diagonal block.  The diagonal-block kernel itself stays at LAPACK's level; the rows below it are solved by a product with the explicitly
# inverted block, and the residual sits in exactly those tiles.  rho_device / max(rho_lapack, u) of the default fit per (kernel, n, sn~);
# None: the trailing update inherits so much error that a pivot of the NEXT block goes negative and the device reports NOT_SPD on a
# matrix LAPACK factors with minimum pivot ~ sn~.  Every path below gives the same factor at these sizes.  Curing it is a change to the
# factorisation's hot path (to be measured at n = 8192), so the cases are strict xfails here, and family B -- the same cond(K~) with
# benign blocks -- holds every bound.
RHO_RATIO = {("rbf", 257, 1e-8): 162.3, ("rbf", 257, 1e-11): None, ("rbf", 384, 1e-8): 114.2, ("rbf", 384, 1e-11): None,
             ("rbf", 640, 1e-8): 88.0, ("rbf", 640, 1e-11): None, ("matern52", 257, 1e-8): 213.8, ("matern52", 257, 1e-11): 35605.6,
             ("matern52", 384, 1e-8): 169.8, ("matern52", 384, 1e-11): 3557.5, ("matern52", 640, 1e-8): 135.2, ("matern52", 640, 1e-11): None}


def known(*values, case=None, group=None):
    """the parameter set, as a strict xfail where the finding above applies (an AssertionError -- a bound, or the device's NOT_SPD on a matrix
    LAPACK factors -- is the expected failure; any other exception fails the test)"""
    keys = [case[1:]] if case else [group[1:] + (lv,) for lv in H.A_LEVELS[1:]]
    if (case or group)[0] != "A" or keys[0] not in RHO_RATIO:
        return pytest.param(*values)
    what = ", ".join("sn~ = %g: %s" % (k[2], "NOT_SPD on a matrix LAPACK factors" if RHO_RATIO[k] is None else "rho ratio %.1f" % RHO_RATIO[k])
                     for k in keys)
    return pytest.param(*values, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason="panel solves by an inverted diagonal block lose cond(K11): " + what))


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def inputs(case):
    """what one fit is given: dict(X, y, ell, sn, theta, M, ride, gen, sets {name: rows of vstack(ride, gen)}, cross, dK)"""
    family, kind, n, level = case
    if family == "A":
        X, y, ride, gen = H.family_a(n)
        sn = H.roundtrip(level)
        sets = dict(ride=np.arange(3), gen5=3 + np.asarray(GEN5), gen200=3 + np.arange(200))
        return dict(X=X, y=y, ell=H.ELL_A, sn=sn, theta=[math.log(3.0), math.log(level)], M=None, ride=ride, gen=gen, sets=sets,
                    cross=lambda K: H.cross_a(kind, X, np.vstack([ride, gen])), dK=lambda: H.dk_a(kind, X))
    K0, dK, y, ride, gen = H.family_b(n, **({"lam_min": level[1]} if isinstance(level, tuple) else {"p": level}))
    sets = dict(ride=np.arange(3), gen5=3 + np.arange(5), gen200=3 + np.arange(200))
    return dict(X=np.eye(n), y=y, ell=1.0, sn=0.0, theta=[0.0, -np.inf], M=np.zeros((n, n)), ride=ride, gen=gen, sets=sets, K0=K0, dK0=dK,
                cross=lambda K: H.cross_b(K, np.vstack([ride, gen])), dK=lambda: dK)


def make_gp(S, case, inp, dtype="f64"):
    """family A: the ordinary covariance build.  Family B: the reference kernel with X = I and "Sigma" = K (so that K~ = X Sigma X^T + 0 I is
    the prescribed matrix, as tests/test_hip_round2.py::test_diagonal_block_kernel_reports_the_first_bad_pivot hands its matrix over), through
    a test-local subclass whose ``_sigma`` returns (K, dK): every call of the Python host then runs on that matrix."""
    if case[0] == "A":
        return S.GPR(kernel=case[1], dtype=dtype)

    class SpectrumGPR(S.GPR):
        def _sigma(self, ell, with_derivative=False):
            return (inp["K0"], inp["dK0"]) if with_derivative else inp["K0"]

    return SpectrumGPR(kernel="netdiffusion")


def raw_alpha(gp):
    from seaiceextentforecasting_amd import _lib as L
    a = np.zeros(gp.n)
    gp._check(gp._lib.sigp_get_alpha(gp._h, L.ptr(a)), "get_alpha")        # alpha~ itself (``alpha_`` divides it by sigma_f)
    return a


def device_run(S, case, path="default", full=True):
    """one fit on the device and everything the host surface computes from it (``full=False``: the factor only); dict(K, spd, info) if the
    device says NOT_SPD"""
    if (case, path) in _DEV:
        return _DEV[(case, path)]
    inp = inputs(case)
    with make_gp(S, case, inp) as gp:
        for name, value in PATHS[path].items():
            gp.set_option(name, value)
        gp.set_data(inp["X"], inp["y"], M=inp["M"], Xs=inp["ride"])
        Kl = gp.kernel_matrix(inp["ell"], inp["sn"])
        out = dict(K=Kl + np.tril(Kl, -1).T, spd=True)
        if "K0" in inp:         # the matrix the ``_sigma`` override hands over IS what the device factors (X = I: every product is exact up to the sum's order)
            assert np.max(np.abs(out["K"] - (inp["K0"] + inp["sn"] * np.eye(len(inp["y"]))))) <= 4 * H.U * np.max(np.abs(inp["K0"]))
        try:
            gp.refit(inp["ell"], inp["sn"])
        except S.LinAlgError as e:
            out.update(spd=False, info=e.info)
            _DEV[(case, path)] = out
            return out
        out.update(L=gp.L_tilde_, alpha=raw_alpha(gp), sigma_f=gp.sigma_f_, nlml=gp.nlml_)
        if not full:
            _DEV[(case, path)] = out
            return out
        out["ride"] = gp.predict(inp["ride"])                                  # the rows that rode along the factorisation
        out["gen5"] = gp.predict(inp["gen"][GEN5] if case[0] == "A" else inp["gen"][:5])   # the general path, one chunk
        if "gen200" in inp["sets"] and path == "default":
            out["gen200"] = gp.predict(inp["gen"])                             # ... past the ride-along limit
        loo, cv = gp.loo(), gp.cv(5)
        out.update(loo_mean=loo["mean"], loo_var=loo["var"], cv_mean=cv["mean"], cv_var=cv["var"])
        out["nlml_call"], out["grad"] = gp.nlml(inp["theta"], grad="exact")
    _DEV[(case, path)] = out
    return out


def reference(S, case, K=None, block=5, grad=True):
    """the long-double and the LAPACK results for the matrix the device built (default path), once per case"""
    if case in _REF:
        return _REF[case]
    inp = inputs(case)
    K = device_run(S, case)["K"] if K is None else K
    ks, kss = inp["cross"](K)
    dK = inp["dK"]() if grad else None
    hp = H.hp_fit(K, inp["y"], inp["sn"], dK=dK, ks=ks, kss=kss, block=block)
    la = H.lapack_fit(K, inp["y"], inp["sn"], dK=dK, ks=ks, kss=kss, block=block)
    la["rho"], la["eta"] = H.rho(la["L"], K), H.eta(K, la["alpha"], inp["y"])
    _REF[case] = dict(K=K, hp=hp, la=la, kss=kss, **input_sizes(hp, ks, kss, inp["sn"], dK))
    return _REF[case]


def input_sizes(hp, ks, kss, sn, dK):
    """The size of the two quantities whose INPUTS the device forms for itself and does not hand out: the cross-covariance rows k* and
    dK~/dlog l (the reference is given the host's fp64 values of both; K~ itself is read back from the device, so it is exact).  The device's
    covariance function agrees with the host's to a few u per entry -- exp(-t) moves by t u when t is rounded --, so an exact solver given
    the device's own rows still differs from the reference by about u sum_i |k*_i alpha~_i| in a mean and u (1/2 sum_ij |P_ij dK_ij| +
    sum_ij |alpha~_i dK_ij alpha~_j| / (2 sigma_f)) in the gradient: the natural size of a sum is the size of its terms, not of what is
    left after they cancel.  A variance sigma_f (k** + sn~ - k*^T K~^-1 k*) moves by 2 sigma_f dk*^T w with w = K~^-1 k* = L~^-T v, so beside
    its own size sigma_f (k** + sn~) it carries 2 sigma_f u sum_i |k*_i w_i| (3.6 to 5 times sigma_f u (k** + sn~) in all on family A's control level).
    These are the ``scale`` of mean_*, var_* and grad_l; where LAPACK's own error is larger, it decides."""
    a = np.abs(hp["alpha"])
    absk = np.abs(np.asarray(ks, dtype=H.LD))
    w = H.backward(hp["L"], hp["v"])
    out = dict(mean_size=np.asarray(absk @ a, dtype=np.float64),
               var_size=np.asarray(hp["sigma_f"] * (np.asarray(kss, dtype=H.LD) + sn + 2 * np.sum(absk.T * np.abs(w), axis=0)), dtype=np.float64))
    if dK is not None:
        D = np.abs(np.asarray(dK, dtype=H.LD))
        out["grad_l_size"] = float(np.sum(np.abs(hp["Kinv"]) * D) / 2 + a @ (D @ a) / (2 * hp["sigma_f"]))
    return out


def ratio(dev, lap, floor):
    den = max(lap, floor)
    return dev / den if den > 0 else (0.0 if dev == 0 else np.inf)


def forward_rows(inp, ref, dev, names=None):
    """[(name, |q_dev - q_hp|, |q_lapack - q_hp|, u scale)] of the quantities whose error is proportional to cond"""
    hp, la, n = ref["hp"], ref["la"], len(inp["y"])
    sf = float(hp["sigma_f"])
    rows = []

    def add(name, q_dev, q_la, q_hp, scale):
        if q_dev is not None and (names is None or name in names):
            rows.append((name, H.err(q_dev, q_hp), H.err(q_la, q_hp), H.U * float(scale)))

    add("alpha", dev.get("alpha"), la["alpha"], hp["alpha"], np.max(np.abs(hp["alpha"])))
    add("sigma_f", dev.get("sigma_f"), la["sigma_f"], hp["sigma_f"], abs(sf))
    add("nlml", dev.get("nlml"), la["nlml"], hp["nlml"], max(abs(float(hp["nlml"])), n / 2))
    for tag, idx in inp["sets"].items():
        if tag in dev:
            add("mean_" + tag, dev[tag][0], la["mean"][idx], hp["mean"][idx], np.max(ref["mean_size"][idx]))
            add("var_" + tag, dev[tag][1], la["var"][idx], hp["var"][idx], np.max(ref["var_size"][idx]))
    if "loo_mean" in dev:
        for k in ("loo", "cv"):
            add(k + "_mean", dev[k + "_mean"], la[k + "_mean"], hp[k + "_mean"], np.max(np.abs(inp["y"])))
            add(k + "_var", dev[k + "_var"], la[k + "_var"], hp[k + "_var"], np.max(np.abs(hp[k + "_var"])))
    if "grad" in dev:
        add("nlml_call", dev["nlml_call"], la["nlml"], hp["nlml"], max(abs(float(hp["nlml"])), n / 2))
        add("grad_l", dev["grad"][0], la["grad"][0], hp["grad"][0], ref["grad_l_size"])
        add("grad_sn", dev["grad"][1], la["grad"][1], hp["grad"][1], abs(float(hp["grad"][1])))
    return rows


def measure(S, case, path="default"):
    """{quantity: (device figure, LAPACK figure, floor, ratio)} of one fit, printed once"""
    if (case, path) in _MEASURED:
        return _MEASURED[(case, path)]
    inp, dev, ref = inputs(case), device_run(S, case, path), reference(S, case)
    assert dev["spd"], "the device reports NOT_SPD (pivot %s) on a matrix LAPACK factors" % dev.get("info")
    assert np.array_equal(dev["K"], ref["K"])                  # every path is given the same matrix
    if path != "default" and np.array_equal(dev["L"], device_run(S, case)["L"]):
        rho_dev = measure(S, case)["rho"][0]                   # the same factor: the same residual (a long-double n^3 product saved)
    else:
        rho_dev = H.rho(dev["L"], ref["K"])
    rows = [("rho", rho_dev, ref["la"]["rho"], H.U), ("eta", H.eta(ref["K"], dev["alpha"], inp["y"]), ref["la"]["eta"], H.U)]
    rows += forward_rows(inp, ref, dev)
    m = {name: (d, l, f, ratio(d, l, f)) for name, d, l, f in rows}
    print("\n%s %s n=%d level=%g path=%s cond(K~)=%.2e cond(K11)=%.2e" % (case + (path, H.cond2(ref["K"]), H.cond2(ref["K"][:128, :128]))))
    for name, (d, l, f, r) in m.items():
        print("    %-12s device %.3e  lapack %.3e  floor %.1e  ratio %8.3f" % (name, d, l, f, r))
    # a variance must not go negative on an input where LAPACK's own fp64 variances do not.  (Family B is left out: with X = I and sn~ = 0
    # every test point lies in the span of the training rows and its exact variance is 0 -- the sign is rounding noise in any arithmetic.)
    _NEGATIVE[(case, path)] = ["var_%s: %.3e < 0 on an input where every LAPACK variance is >= 0" % (tag, dev[tag][1].min())
                               for tag, idx in inp["sets"].items()
                               if tag in dev and case[0] == "A" and np.all(ref["la"]["var"][idx] >= 0) and not np.all(dev[tag][1] >= 0)]
    _MEASURED[(case, path)] = m
    return m


def check_bounds(m, what, negative=()):
    bad = list(negative) + ["%s: device %.3e > %g * max(lapack %.3e, floor %.1e)  (ratio %.1f)" % (k, d, MARGIN, l, f, r) for k, (d, l, f, r) in m.items()
           if not d <= MARGIN * max(l, f)]
    assert not bad, "%s\n  " % (what,) + "\n  ".join(bad)


SCALARS = ("sigma_f", "nlml", "nlml_call", "grad_l", "grad_sn")


def check_growth(S, group, path):
    """rho, eta and every vector quantity (max-norm over its entries): hardest <= 8 x control.  The scalars: hardest <= 8 x max(control, 1).
    The error of ONE number is as close to zero as chance has it, in either arithmetic, so a control ratio below 1 is no yardstick (a device
    sigma_f that happens to be 60 times better than LAPACK's on the easy matrix would make "2.5 times worse on the hard one" a failure);
    "as good as LAPACK" is the least a control level can be held to."""
    lv = LEVELS[group[0]]
    ctrl, hard = measure(S, group + (lv[0],), path), measure(S, group + (lv[-1],), path)
    bad = ["%s: ratio %.3f at the hardest level > %g * %.3f at the control" % (k, hard[k][3], GROWTH, ctrl[k][3]) for k in hard
           if not hard[k][3] <= GROWTH * (max(ctrl[k][3], 1.0) if k in SCALARS else ctrl[k][3])]
    assert not bad, "%s path=%s\n  " % (group, path) + "\n  ".join(bad)


# ---- one fit per (family, n, level) on defaults ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,kind,n,level", [known(*c, case=c) for c in CASES])
def test_default_fit_is_as_accurate_as_lapack(S, family, kind, n, level):
    """factor, alpha~, sigma_f, nlML, predictions (ride-along rows; the general path with 5 and 200 points, training rows and far points among
    them: k** - ||v||^2 ~ sn~ cancels catastrophically there), LOO, cv(block=5) and the exact MLII gradient against the bounds above"""
    case = (family, kind, n, level)
    m = measure(S, case)
    dev = device_run(S, case)
    assert dev["nlml_call"] == dev["nlml"]                 # ``nlml`` at theta = log of the fit's parameters factors the same matrix
    check_bounds(m, str(case), _NEGATIVE[(case, "default")])


@pytest.mark.parametrize("family,kind,n", [known(*g, group=g) for g in A_GROUPS + B_GROUPS])
def test_error_ratio_does_not_grow_with_conditioning(S, family, kind, n):
    """the assertion that is independent of any absolute margin: device error over LAPACK error at cond ~ 1e13 / 1e14 against cond ~ 1e6 / 1e4"""
    check_growth(S, (family, kind, n), "default")


# ---- the documented schedules and equivalent routes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,kind,n,level,path", [known(*c, p, case=c) for c in PATH_CASES for p in OTHER_PATHS])
def test_option_paths_are_as_accurate_as_lapack(S, family, kind, n, level, path):
    case = (family, kind, n, level)
    m = measure(S, case, path)
    check_bounds(m, "%s path=%s" % (case, path), _NEGATIVE[(case, path)])


@pytest.mark.parametrize("family,kind,n,level,path", [c + (p,) for c in PATH_CASES for p in SAME_BITS])
def test_schedules_the_header_calls_bit_identical_are(S, family, kind, n, level, path):
    """``schedule`` ("same factor bit for bit") and ``panel_chain`` ("bit-identical results") against the default run, on every matrix of the path
    tests, the ill-conditioned ones included -- this does not depend on how accurate the factor is, so no case is an expected failure: where
    both runs factor the matrix every result carries the same bits, where both refuse it they refuse it at the same pivot"""
    case = (family, kind, n, level)
    base, dev = device_run(S, case), device_run(S, case, path)
    assert np.array_equal(base["K"], dev["K"])
    assert base["spd"] == dev["spd"], (base.get("info"), dev.get("info"))
    if not base["spd"]:
        assert base["info"] == dev["info"]
        return
    for k in ("L", "alpha", "sigma_f", "nlml", "loo_mean", "loo_var", "cv_mean", "cv_var", "nlml_call", "grad"):
        assert np.array_equal(base[k], dev[k]), (path, k)
    for k in ("ride", "gen5"):
        assert np.array_equal(base[k][0], dev[k][0]) and np.array_equal(base[k][1], dev[k][1]), (path, k)


@pytest.mark.parametrize("n", [257, 384])
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_gradient_on_ordered_inputs_with_dK_handed_over_exactly(S, kind, n):
    """d nlML / d log l on family A is bounded loosely above (the device forms dK~/dlog l itself: input_sizes).  Here family A's control-level
    matrix goes through family B's route -- X = I, "Sigma" = k~(X, X) and dK from the host --, so that K~ (read back) and dK are the
    device's inputs exactly and the floor is u |g|: the gradient pipeline (U = L~^-T, K~^-1 = U U^T, the reduction) on a matrix whose
    diagonal blocks are as ill-conditioned as it is, held to 16 x LAPACK.  (The harder levels show the factor's loss and are covered above.)"""
    from oracle import gp_oracle as O
    X, y, _, _ = H.family_a(n)
    level = H.A_LEVELS[0]
    sn = H.roundtrip(level)
    inp = dict(K0=O.cov_unit(kind, X, X, H.ELL_A), dK0=H.dk_a(kind, X), y=y, sn=sn)
    with make_gp(S, ("B",), inp) as gp:
        gp.set_data(np.eye(n), y, M=np.zeros((n, n)))
        Kl = gp.kernel_matrix(1.0, sn)
        K = Kl + np.tril(Kl, -1).T
        assert np.max(np.abs(K - (inp["K0"] + sn * np.eye(n)))) <= 4 * H.U
        val, g = gp.nlml([0.0, math.log(level)], grad="exact")
    hp = H.hp_fit(K, y, sn, dK=inp["dK0"], block=0)
    la = H.lapack_fit(K, y, sn, dK=inp["dK0"], block=0)
    rows = [("nlml", H.err(val, hp["nlml"]), H.err(la["nlml"], hp["nlml"]), H.U * max(abs(float(hp["nlml"])), n / 2))]
    rows += [(name, H.err(g[i], hp["grad"][i]), H.err(la["grad"][i], hp["grad"][i]), H.U * abs(float(hp["grad"][i]))) for i, name in enumerate(("grad_l", "grad_sn"))]
    m = {name: (d, l, f, ratio(d, l, f)) for name, d, l, f in rows}
    print("\nexact dK: %s n=%d sn~=%g cond(K~)=%.2e" % (kind, n, level, H.cond2(K)))
    for name, (d, l, f, r) in m.items():
        print("    %-12s device %.3e  lapack %.3e  floor %.1e  ratio %8.3f" % (name, d, l, f, r))
    check_bounds(m, "exact dK %s n=%d" % (kind, n))


@pytest.mark.parametrize("family,kind,n,path", [known(*g, p, group=g) for g in PATH_GROUPS for p in OTHER_PATHS])
def test_option_paths_do_not_grow_with_conditioning(S, family, kind, n, path):
    check_growth(S, (family, kind, n), path)


# ---- near the edge of definiteness ----------------------------------------------------------------------------------------------------------
EDGE_CASES = [("B", "spectrum", 257, ("lambda_min", lam)) for lam in H.B_EDGE] + [("A", kind, 257, H.A_EDGE) for kind in ("rbf", "matern52")]


@pytest.mark.parametrize("family,kind,n,level", EDGE_CASES, ids=lambda v: "%s=%g" % v if isinstance(v, tuple) else None)
def test_edge_of_definiteness_is_never_silently_wrong(S, family, kind, n, level):
    """the device may answer either way, but: OK -> its factor obeys the residual bound; NOT_SPD -> the long-double Cholesky of the same matrix
    has a squared pivot <= 64 n u ||K~||_2 (or fails itself); a matrix built with a negative eigenvalue must be refused"""
    case = (family, kind, n, level)
    dev = device_run(S, case, full=False)
    K = dev["K"]
    try:
        minpiv = float(np.min(H.cholesky(K)[1]))
    except H.NotSPD as e:
        minpiv = float(np.min(e.pivots))
    try:
        rho_la = H.rho(np.linalg.cholesky(K), K)
    except np.linalg.LinAlgError:
        rho_la = 0.0
    norm2 = float(np.max(np.abs(np.linalg.eigvalsh(K))))
    print("\n%s %s n=%d level=%s: device %s, hp min squared pivot %.3e (64 n u ||K|| = %.3e), LAPACK rho %s" % (
        case + ("OK" if dev["spd"] else "NOT_SPD (pivot %d)" % dev["info"], minpiv, 64 * n * H.U * norm2, rho_la or "LinAlgError")))
    if dev["spd"]:
        assert not (isinstance(level, tuple) and level[1] < 0), "an indefinite matrix was factored"
        r = H.rho(dev["L"], K)
        print("    rho device %.3e  ratio %.3f" % (r, r / max(rho_la, H.U)))
        assert r <= MARGIN * max(rho_la, H.U)
    else:
        assert minpiv <= 64 * n * H.U * norm2


# ---- lockstep batch -------------------------------------------------------------------------------------------------------------------------
BATCH_LEVELS = [1e-8, 1e-11, 1e-4, 1e-2]          # one group of 4 at n = 384: two hard members, the control level, an easy member
_BATCH = {}


def batch_run(S, kind):
    if kind in _BATCH:
        return _BATCH[kind]
    X, y, ride, _ = H.family_a(384)
    easy = [1e-1, 3e-2, 2e-2, 1e-2]
    with S.GPR(kernel=kind) as gp:
        fit = gp.fit_batch(X, y, ride, [H.ELL_A] * 4, [H.roundtrip(v) for v in BATCH_LEVELS], group=4)
        val, grad = gp.nlml_batch(np.array([[math.log(3.0), math.log(v)] for v in BATCH_LEVELS]), grad="exact", group=4)
        fit_e = gp.fit_batch(X, y, ride, [H.ELL_A] * 4, [H.roundtrip(v) for v in easy], group=4)
        val_e, grad_e = gp.nlml_batch(np.array([[math.log(3.0), math.log(v)] for v in easy]), grad="exact", group=4)
    _BATCH[kind] = (fit, val, grad, fit_e, val_e, grad_e)
    return _BATCH[kind]


def check_batch_member(S, kind, i):
    """member i of the group against the single-fit bounds (its matrix: the single fit's build of the same parameters)"""
    fit, val, grad = batch_run(S, kind)[:3]
    level = BATCH_LEVELS[i]
    case = ("A", kind, 384, level)
    inp = inputs(case)
    assert fit["info"][i] == 0, "member %d (sn~ = %g): NOT_SPD (pivot %d) on a matrix LAPACK factors" % (i, level, fit["info"][i])
    if level == 1e-2:                       # not a level of the single-fit tests
        with S.GPR(kernel=kind) as gp1:
            gp1.set_data(inp["X"], inp["y"])
            Kl = gp1.kernel_matrix(H.ELL_A, inp["sn"])
        ref = reference(S, case, K=Kl + np.tril(Kl, -1).T)
    else:
        ref = reference(S, case)
    dev = dict(sigma_f=fit["sigma_f"][i], nlml=fit["nlml"][i], ride=(fit["mean"][i], fit["var"][i]), nlml_call=val[i], grad=grad[i])
    rows = forward_rows(inp, ref, dev, names=("sigma_f", "nlml", "mean_ride", "var_ride", "nlml_call", "grad_l", "grad_sn"))
    m = {name: (d, l, f, ratio(d, l, f)) for name, d, l, f in rows}
    print("\nbatch member %d: %s sn~=%g" % (i, kind, level))
    for name, (d, l, f, r) in m.items():
        print("    %-12s device %.3e  lapack %.3e  floor %.1e  ratio %8.3f" % (name, d, l, f, r))
    check_bounds(m, "batch member %d (sn~ = %g)" % (i, level))


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_lockstep_group_easy_members_are_untouched_by_hard_ones(S, kind):
    """``fit_batch`` and ``nlml_batch(grad='exact')`` on a group with sn~ = 1e-8, 1e-11, 1e-4 and 1e-2: the easy member carries the bits it has in
    a group of four easy fits, and it and the control-level member obey the single-fit bounds"""
    fit, val, grad, fit_e, val_e, grad_e = batch_run(S, kind)
    for k in ("sigma_f", "nlml", "mean", "var", "info"):
        assert np.array_equal(fit[k][3], fit_e[k][3]), k
    assert val[3] == val_e[3] and np.array_equal(grad[3], grad_e[3])
    check_batch_member(S, kind, 2)
    check_batch_member(S, kind, 3)


@pytest.mark.parametrize("kind,member", [known(kind, i, case=("A", kind, 384, BATCH_LEVELS[i])) for kind in ("rbf", "matern52") for i in (0, 1)])
def test_lockstep_group_hard_members_obey_the_single_fit_bounds(S, kind, member):
    check_batch_member(S, kind, member)


# ---- fp32 engine ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1e-2, 1e-4, 1e-6, 1e-8])
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_fp32_engine_reports_its_residual_truthfully(S, kind, level):
    """fp32 factor + fp64 refinement at default ``refine_iters``; the last level is past what an fp32 factor can precondition.  The reported
    ``refine_residual_`` must be the residual of the returned alpha~ (recomputed in long double, within a factor 2 plus 1e-15); where it is
    <= 1e-12, alpha~, sigma_f, the ride-along predictions and the general path's mean obey the fp64 forward bounds; where it is larger, or the fit raises LinAlgError,
    the call announced itself and nothing more is asserted"""
    n = 384
    X, y, ride, gen = H.family_a(n)
    sn = H.roundtrip(level)
    with S.GPR(kernel=kind) as gp64:
        gp64.set_data(X, y)
        Kl = gp64.kernel_matrix(H.ELL_A, sn)
    K = Kl + np.tril(Kl, -1).T
    with S.GPR(kernel=kind, dtype="f32") as gp:
        try:
            gp.fit(X, y, H.ELL_A, sn, Xs=ride)
        except S.LinAlgError as e:
            print("\nfp32 %s sn~=%g: LinAlgError (pivot %d)" % (kind, level, e.info))
            return
        reported = gp.refine_residual_
        dev = dict(alpha=raw_alpha(gp), sigma_f=gp.sigma_f_, ride=gp.predict(ride), gen5=gp.predict(gen[GEN5]))
    true = H.refine_residual(K, dev["alpha"], y)
    print("\nfp32 %s sn~=%g cond=%.2e: refine_residual_ reported %.3e, recomputed %.3e" % (kind, level, H.cond2(K), reported, true))
    assert true <= 2 * reported + 1e-15 and reported <= 2 * true + 1e-15
    if reported <= 1e-12:
        inp = dict(y=y, sn=sn, sets=dict(ride=np.arange(3), gen5=3 + np.arange(5)))
        ks, kss = H.cross_a(kind, X, np.vstack([ride, gen[GEN5]]))
        hp = H.hp_fit(K, y, sn, ks=ks, kss=kss, block=0)
        ref = dict(hp=hp, la=H.lapack_fit(K, y, sn, ks=ks, kss=kss, block=0), kss=kss, **input_sizes(hp, ks, kss, sn, None))
        # (the general path's mean is k* against the refined alpha~; its VARIANCE comes from the fp32 factor, as the header says, and is not held to fp64)
        rows = forward_rows(inp, ref, dev, names=("alpha", "sigma_f", "mean_ride", "var_ride", "mean_gen5"))
        m = {name: (d, l, f, ratio(d, l, f)) for name, d, l, f in rows}
        for name, (d, l, f, r) in m.items():
            print("    %-12s device %.3e  lapack %.3e  floor %.1e  ratio %8.3f" % (name, d, l, f, r))
        check_bounds(m, "fp32 %s sn~ = %g" % (kind, level))
