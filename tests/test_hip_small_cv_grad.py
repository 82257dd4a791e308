"""GPU tier of the leave-block-out score gradient of the one-workgroup kernel (csrc/smallgp.hpp: CvGrad; ``SmallBatch.run(cv_grad=)``,
``GPR.small_cv_score_batch``, ``GPR.optimize_small_cv_batch``, ``retro_optimise(criterion="cv_*")``) against the long-double closed form of
tests/small_cv_grad_cases.py (pinned by tests/test_small_cv_grad_host.py).

The yardstick is that of tests/test_hip_small_score_grad.py, unchanged:  |g_device - g_ref| / S <= 16 max(e_fp64, (n + N) u) for each of the
two gradient entries, S = the sum of the absolute values of the contraction's terms, e_fp64 = the median over ``small_grad_cases.DRAWS``
admissible roundings of K~ of the error of an fp64 NumPy evaluation of the same formulas.  The other outputs of a launch are byte-equal to
``run(cv=)``'s wherever both launches sum the features in the same chunks, and elsewhere held to that launch's own yardstick
(tests/test_hip_small_flavours.py).  Every test prints its largest ratio (``RATIO`` lines; docs/EXPERIMENTS.md records them).

Measured on an MI355X (bound 16): 6.03 (the 'pade' member n = 33 at block 32), 3.31 at n = 2, below 1.3 on every other batch; block 1 without a gap
against the leave-one-out reference 1.41."""
import numpy as np
import pytest

import small_cases as SC
import small_cv_grad_cases as CG
import small_grad_cases as GC
from conftest import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")]
MARGIN = 16.0


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _launch(S, cases, layouts, order=None):
    """{(block, gap, mode): (score launch, {crit: gradient launch}, the nlpd gradient launch again)} of one upload"""
    cases = list(cases) if order is None else [cases[i] for i in order]
    out = {}
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        SC.queue(sb, cases)
        for block, gap in layouts:
            for mode in SC.MODES:
                kw = dict(block=block, gap=gap, sigma_f=mode)
                out[(block, gap, mode)] = (sb.run(cv=kw), {crit: sb.run(cv_grad=dict(score=crit, **kw)) for crit in CG.CRITERIA}, sb.run(cv_grad=dict(score="nlpd", **kw)))
    return out


_RESULTS = {}


def _results(S, name):
    if name not in _RESULTS:
        _RESULTS[name] = _launch(S, CG.gpu_batches()[name], CG.layouts(name))
    return _RESULTS[name]


def _judge(tag, items):
    worst, bad = (-1.0, None, 0.0, 0.0), []
    for c, ed, ef in items:
        assert np.isfinite(ed) and np.isfinite(ef), (tag, c, ed, ef)
        ratio = ed / max(ef, (c.n + c.N) * SC.U)
        if ratio > worst[0]:
            worst = (ratio, c, ed, ef)
        if ed > SC.bound(c, ef, MARGIN):
            bad.append((ratio, ed, ef, c))
    print("RATIO %-40s %8.3g   (e_device %.3g, e_fp64 %.3g, (n + N) u %.3g: %s)" % (tag, worst[0], worst[2], worst[3], (worst[1].n + worst[1].N) * SC.U, (worst[1],)))
    assert not bad, (tag, len(bad), sorted(bad, key=lambda t: -t[0])[:5])
    return worst[0]


def _fit_bytes(r, i, c, grad):
    parts = [r[k][i].tobytes() for k in ("sigma_f", "nlml", "info", "sigma_n")] + [r["mean"][i, :c.m].tobytes(), r["var"][i, :c.m].tobytes()]
    parts += [r["cv_mean"][i, :c.n].tobytes(), r["cv_var"][i, :c.n].tobytes(), r["cv_nlpd"][i].tobytes(), r["cv_sse"][i].tobytes()]
    return parts + ([r["cv_grad"][i].tobytes()] if grad else [])


# ---- 1. accuracy, the score entry's bytes, repeatability ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mid", "wide", "big0", "big8"])
def test_gradients_within_the_bound_and_the_rest_has_the_score_launch_bytes(S, name):
    cases, dev, layouts = CG.gpu_batches()[name], _results(S, name), CG.layouts(name)
    nmax, mmax = max(c.n for c in cases), max(c.m for c in cases)
    assert layouts, name
    if name == "mid":
        assert layouts == ((1, 0), (5, 1), (8, 0), (7, 3))            # overlapping windows, a short last fold, clipped windows; (2, 15) needs 33 rows: wide
    if name == "wide":
        assert layouts == ((32, 0), (30, 1), (2, 15)) and min(c.n for c in cases) == 33     # n = 33, block 32: a last fold of exactly one scored row
    if name.startswith("big"):
        w = CG.BIG_LAYOUT[0] + 2 * CG.BIG_LAYOUT[1]
        assert nmax == CG.order_limit(mmax, w) and CG.cv_grad_chunk(nmax + 1, mmax, w) is None and CG.cv_grad_chunk(nmax, mmax, w) == 8
    for block, gap in layouts:
        chunk = CG.cv_grad_chunk(nmax, mmax, block + 2 * gap)
        same_chunk = chunk == SC.cv_chunk(nmax, mmax)
        for mode in SC.MODES:
            score, grads, again = dev[(block, gap, mode)]
            items = []
            for crit in CG.CRITERIA:
                r = grads[crit]
                assert np.all(r["info"] == 0) and r["cv_grad"].shape == (len(cases), 2)
                for i, c in enumerate(cases):
                    ref = CG.reference(c, SC.HP.name, block, gap, mode, crit)
                    items.append((c, GC.grad_error(r["cv_grad"][i], ref), CG.comparator_error(c, block, gap, mode, crit)))
                    # outputs 0 .. 5, mean / var and the rows: run(cv=)'s bytes wherever both launches sum the features in the same chunks
                    if same_chunk or c.N <= chunk:
                        assert _fit_bytes(r, i, c, False) == _fit_bytes(score, i, c, False), (block, gap, mode, crit, c)
                    else:       # ... and elsewhere the error of the fit in the score flavour, as test_hip_small_flavours.py judges that launch
                        fit, f64fit = SC.reference(c), SC.reference(c, SC.F64)
                        rr, fr = SC.rows_of(c, SC.HP.name, "cv", block, gap)[mode], SC.rows_of(c, SC.F64.name, "cv", block, gap)[mode]
                        got = dict(mean=r["cv_mean"][i, :c.n], var=r["cv_var"][i, :c.n], nlpd=r["cv_nlpd"][i], sse=r["cv_sse"][i])
                        plain = dict(sigma_f=r["sigma_f"][i], sigma_n=r["sigma_n"][i], nlml=r["nlml"][i], mean=r["mean"][i, :c.m], var=r["var"][i, :c.m])
                        assert max(SC.rows_error(got, rr, fit["y"]), SC.plain_error(plain, fit)) <= SC.bound(
                            c, max(SC.rows_error(fr, rr, fit["y"]), SC.plain_error(f64fit, fit)), MARGIN), (block, gap, mode, crit, c)
            _judge("%s cv block=%d gap=%d %s" % (name, block, gap, mode), items)
            for k in again:         # a second call: the same bytes
                assert again[k].tobytes() == grads["nlpd"][k].tobytes(), (block, gap, mode, k)


def test_block_one_without_a_gap_is_the_leave_one_out_gradient(S):
    """different sums, so to rounding and not byte for byte: the (1, 0) gradient is held to the LEAVE-ONE-OUT long-double reference at the
    leave-one-out bound, and so the two launches differ by at most the two bounds together"""
    cases, dev = CG.gpu_batches()["mid"], _results(S, "mid")
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        SC.queue(sb, cases)
        loo = {(mode, crit): sb.run(loo=mode, score_grad=crit) for mode in SC.MODES for crit in CG.CRITERIA}
    for mode in SC.MODES:
        items = []
        for crit in CG.CRITERIA:
            r = dev[(1, 0, mode)][1][crit]
            for i, c in enumerate(cases):
                ref = GC.reference(c, SC.HP.name, "loo", mode, crit)
                ef = GC.comparator_error(c, "loo", mode, crit)
                items.append((c, GC.grad_error(r["cv_grad"][i], ref), ef))
                diff = np.abs(SC.LD(1) * r["cv_grad"][i] - loo[(mode, crit)]["loo_grad"][i])
                ok = ~np.isnan(np.asarray(ref["S"], dtype=np.float64)) & (ref["S"] > 0)
                assert np.all(diff[ok] <= 2 * SC.bound(c, ef, MARGIN) * ref["S"][ok]), (mode, crit, c)
        _judge("mid cv (1, 0) against leave-one-out %s" % mode, items)


def test_a_lam_mode_1_set_without_dweights_has_nan_in_dlogl_alone(S):
    """the 'pade' member of mid, uploaded with and without ``sigp_small_set_dweights``"""
    c = next(c for c in CG.gpu_batches()["mid"] if c.expm == "pade")
    res = {}
    for dweights in (True, False):
        with S.GPR(kernel="netdiffusion") as gp:
            sb = S.SmallBatch(gp)
            SC.queue(sb, [c])
            sb.upload(dweights=dweights)
            res[dweights] = {crit: sb.run(cv_grad=dict(block=5, gap=1, score=crit)) for crit in CG.CRITERIA}
    for crit, r in res[False].items():
        full = res[True][crit]
        assert np.isnan(r["cv_grad"][0, 0]) and np.isfinite(full["cv_grad"][0, 0]), crit
        assert r["cv_grad"][0, 1].tobytes() == full["cv_grad"][0, 1].tobytes()
        assert _fit_bytes(r, 0, c, False) == _fit_bytes(full, 0, c, False), "everything else is unchanged"
        ref = CG.reference(c, SC.HP.name, 5, 1, "refit", crit, dweights=False)
        assert np.isnan(np.float64(ref["grad"][0]))
        assert GC.grad_error(r["cv_grad"][0], ref) <= SC.bound(c, CG.comparator_error(c, 5, 1, "refit", crit, dweights=False), MARGIN)


# ---- 2. a fit's bytes do not depend on its place in the queue or on its neighbours ------------------------------------------------------------------
def test_results_do_not_depend_on_the_order_of_the_queue(S):
    cases, dev = CG.gpu_batches()["mid"], _results(S, "mid")
    F = len(cases)
    layouts = [(5, 1), (7, 3)]
    rev = _launch(S, cases, layouts, order=list(range(F - 1, -1, -1)))
    twice = _launch(S, cases, layouts, order=[i // 2 for i in range(2 * F)])
    for block, gap in layouts:
        for mode in SC.MODES:
            key = (block, gap, mode)
            for crit in CG.CRITERIA:
                for i, c in enumerate(cases):
                    mine = _fit_bytes(dev[key][1][crit], i, c, True)
                    assert mine == _fit_bytes(rev[key][1][crit], F - 1 - i, c, True), (key, crit, c)
                    assert mine == _fit_bytes(twice[key][1][crit], 2 * i, c, True) == _fit_bytes(twice[key][1][crit], 2 * i + 1, c, True), (key, crit, c)


def test_a_non_spd_member_at_the_largest_order_leaves_its_neighbours_alone(S):
    """the largest order BIG_LAYOUT admits at m = 0, duplicate rows, sn~ = 0, N = 17 < n"""
    block, gap = CG.BIG_LAYOUT
    n, m, N = CG.order_limit(0, block + 2 * gap), 0, 17
    X, y, Xs, M = SC.dataset(n, N, m, 20269000 + n)
    Xb = X.copy()
    Xb[n // 2:] = X[:n - n // 2]
    kw = dict(cv_grad=dict(block=block, gap=gap, score="nlpd"))
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        good, bad = sb.add_dataset(X, y, None, M), sb.add_dataset(Xb, y, None, M)
        for ds, sn in ((good, 0.1), (bad, 0.0), (good, 1.0)):
            sb.add_fit(ds, 0.05, sn)
        with3 = sb.run(**kw)
        sb.clear_fits()
        sb.add_fit(good, 0.05, 0.1)
        sb.add_fit(good, 0.05, 1.0)
        with2 = sb.run(**kw)
    assert 1 <= with3["info"][1] <= n and with3["info"][0] == 0 and with3["info"][2] == 0 and np.all(with2["info"] == 0)
    assert with3["cv_nlpd"][1] == np.inf and with3["cv_sse"][1] == np.inf and np.all(with3["cv_grad"][1] == np.inf)
    assert np.all(np.isnan(with3["cv_mean"][1])) and np.all(np.isnan(with3["cv_var"][1]))
    assert np.all(np.isfinite(with3["cv_grad"][[0, 2]])) and np.all(np.isfinite(with3["cv_nlpd"][[0, 2]]))
    for k in with3:
        assert with3[k][[0, 2]].tobytes() == with2[k].tobytes(), k


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_limit_and_leave_the_handle_usable(S):
    from seaiceextentforecasting_amd import _lib as L
    block, gap = CG.BIG_LAYOUT
    w = block + 2 * gap
    n0 = CG.order_limit(0, w)
    wide = next(x for x in range(w + 1, CG.MAX_WINDOW + 1) if CG.cv_grad_chunk(n0, 0, x) is None)         # the first window beyond the layout at that order
    assert CG.cv_grad_chunk(n0, 0, wide - 1) == 8 and CG.cv_grad_chunk(n0 + 1, 0, w) is None and SC.cv_chunk(n0 + 1, 0) is not None

    def direct(gp, sb, extra):
        """the entry itself, past the Python checks: its return code"""
        si, ell, sn = (np.zeros(1, dtype=np.int64), np.array([0.05]), np.array([1.0]))
        nmax = max(s[1].shape[0] for s in sb._sets)
        out, mean, var = np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8))
        rm, rv = np.zeros((1, nmax)), np.zeros((1, nmax))
        return gp._lib.sigp_small_run_cv_grad(gp._h, 1, L.iptr(si), L.ptr(ell), L.ptr(sn), *extra, L.ptr(out), L.ptr(mean), L.ptr(var), 8, L.ptr(rm), L.ptr(rv), nmax)

    with S.GPR(kernel="netdiffusion") as gp:        # an order beyond the layout
        sb = S.SmallBatch(gp)
        SC.queue(sb, [SC.Case(n0 + 1, 17, 0, 0.05, 1.0, "eigh", 20269501)])
        before = sb.run(cv=dict(block=block, gap=gap))
        with pytest.raises(ValueError, match=r"n = %d with m = 0 and window = %d needs \d+ bytes of LDS.*limit is %d" % (n0 + 1, w, CG.LDS_MAX)):
            sb.run(cv_grad=dict(block=block, gap=gap))
        assert direct(gp, sb, (block, gap, 0, 0)) == L.BAD_ARG
        after = sb.run(cv=dict(block=block, gap=gap))
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
    with S.GPR(kernel="netdiffusion") as gp:        # a window beyond it
        sb = S.SmallBatch(gp)
        SC.queue(sb, [SC.Case(n0, 17, 0, 0.05, 1.0, "eigh", 20269502)])
        before = sb.run(cv=dict(block=wide, gap=0))
        ok = sb.run(cv_grad=dict(block=wide - 1, gap=0))
        assert np.all(np.isfinite(ok["cv_grad"]))
        with pytest.raises(ValueError, match=r"n = %d with m = 0 and window = %d needs \d+ bytes of LDS.*limit is %d" % (n0, wide, CG.LDS_MAX)):
            sb.run(cv_grad=dict(block=wide, gap=0))
        assert direct(gp, sb, (wide, 0, 0, 0)) == L.BAD_ARG
        assert direct(gp, sb, (33, 0, 0, 0)) == L.BAD_ARG and direct(gp, sb, (1, 16, 0, 0)) == L.BAD_ARG     # beyond SIGP_CV_SMALL_MAX_WINDOW
        assert direct(gp, sb, (0, 0, 0, 0)) == L.BAD_ARG and direct(gp, sb, (5, -1, 0, 0)) == L.BAD_ARG
        for bad in (-1, 2):                                                                                    # a bad criterion, a bad sigma mode
            assert direct(gp, sb, (block, gap, 0, bad)) == L.BAD_ARG and direct(gp, sb, (block, gap, bad, 0)) == L.BAD_ARG
        assert direct(gp, sb, (block, gap, 1, 1)) == 0
        after = sb.run(cv=dict(block=wide, gap=0))
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k


# ---- 4. end to end: the retro loop's hyper-parameters by the leave-block-out score ------------------------------------------------------------------
def test_retro_optimise_by_the_leave_block_out_score(S):
    script, criterion, block = "north_September", "cv_nlpd", 5
    g = load_golden(script + "_retro")
    fmin, fmax = g["args"]
    tab = S.SCRIPT_TABLE[script]
    gtol = 1e-5
    with S.GPR(kernel="netdiffusion") as gp:
        out = S.retro_optimise(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], gp=gp, criterion=criterion, block=block, gtol=gtol)
        ny = fmax - fmin + 1
        x0 = np.asarray([[np.log(tab["ell"][k]), np.log(tab["sn"][k])] for k in range(len(tab["regions"])) for _ in range(ny)])      # as retro_optimise forms it
        x = np.concatenate([out[r]["x"] for r in tab["regions"]])
        fun = np.concatenate([out[r]["fun"] for r in tab["regions"]])
        jac = np.concatenate([out[r]["jac"] for r in tab["regions"]])
        conv = np.concatenate([out[r]["converged"] for r in tab["regions"]])
        sb = gp._small

        def scores(theta):
            sb.clear_fits()
            ell, sn = np.exp(theta[:, 0]), np.exp(theta[:, 1])
            for i, ds in enumerate(gp._small_ids):
                sb.add_fit(ds, ell[i], sn[i])
            return sb.run(cv=dict(block=block, gap=0, sigma_f="refit"))

        at0, atx = scores(x0)[criterion], scores(x)
        fx, gx = gp.small_cv_score_batch(x, block, criterion=criterion)
    assert len(fun) == 3 * ny and np.all(np.isfinite(fun))
    assert np.all(fun <= at0), "never above the score at the script's table entries"
    assert np.all(np.abs(fun - atx[criterion]) <= 1e-12 * np.abs(fun)), "fun is the score launch's value at x"
    assert gx.tobytes() == jac.tobytes() and fx.tobytes() == fun.tobytes(), "the value and gradient returned are those at x"
    assert np.all(np.max(np.abs(jac[conv]), axis=1) <= gtol), "a fit marked converged has its gradient within the optimiser's gtol"
    print("RETRO %s: %d of %d converged, %d launches, median decrease %.3g, %d at |g| <= gtol" % (criterion, int(conv.sum()), len(conv), out["nfev"], float(np.median(at0 - fun)),
                                                                                         int(np.sum(np.max(np.abs(jac), axis=1) <= gtol))))
