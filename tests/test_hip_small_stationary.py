"""GPU tier of the one-workgroup kernel's stationary flavours (csrc/smallgp.hpp: SmallCov::Stationary; ``sigp_small_run_k*``,
``SmallStationaryBatch``, ``GPR.small_nlml_ard_batch``, ``GPR.optimize_small_ard_batch``) against the long-double references of
tests/small_stationary_cases.py (pinned by tests/test_small_stationary_host.py).

The yardstick is ``small_cases.bound``, unchanged: every output of every flavour lies within 16 max(e_fp64, (n + N) u) of the long-double
reference, e_fp64 = the error of the fp64 NumPy / LAPACK evaluation of the same formulas on the same inputs, measured per flavour with
``small_cases``'s own error measures (the gradient: |d| / max(1, |ref|) over all N + 1 components, or both of a common scale).  Every test
prints its largest ratio error / max(e_fp64, (n + N) u) per flavour (``RATIO`` lines; docs/EXPERIMENTS.md records them).

Measured on an MI355X, largest ratio over both kernels and all batches (bound 16): plain 2.19, gradient 4.30, leave-one-out 5.44 (n = 2, a
duplicated row), leave-block-out 5.13 ((30, 1) at n = 127, sn~ = 1e-6), hindcast 2.21."""
import numpy as np
import pytest

import hp_reference as H
import small_cases as SC
import small_stationary_cases as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")]
MARGIN = 16.0
PARITY = 1e-8
BATCHES = sorted(T.batches())


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


def _run_all(sb, batch):
    out = dict(plain=sb.run(), grad=sb.run(grad=True), again=sb.run(grad=True), loo={mode: sb.run(loo=mode) for mode in SC.MODES})
    out["cv"] = {(b, g, mode): sb.run(cv=dict(block=b, gap=g, sigma_f=mode)) for b, g in batch.cv for mode in SC.MODES}
    out["hc"] = {(l, mt, mode): sb.run(hindcast=dict(lead=l, min_train=mt, sigma_f=mode)) for l, mt in batch.hc for mode in SC.MODES}
    return out


_RESULTS = {}


def _results(S, key):
    """every launch of one batch, once: all its cases in one upload (per-feature scales as soon as one case has them), and the cases with
    one common scale alone in a second upload (the ard = 0 launches)"""
    if key not in _RESULTS:
        batch = T.batches()[key]
        common = tuple(c for c in batch.cases if c.kind in ("iso", "dup"))
        with S.GPR(kernel=batch.kernel) as gp:
            sb = S.SmallStationaryBatch(gp)
            T.queue(sb, batch.cases)
            mixed = _run_all(sb, batch)
            sb = S.SmallStationaryBatch(gp)
            T.queue(sb, common)
            alone = _run_all(sb, batch) if common else None
        _RESULTS[key] = (mixed, alone, common)
    return _RESULTS[key]


def _judge(tag, items):
    worst, bad = (-1.0, None, 0.0, 0.0), []
    for c, ed, ef in items:
        assert np.isfinite(ed) and np.isfinite(ef), (tag, c, ed, ef)
        ratio = ed / max(ef, (c.n + c.N) * SC.U)
        if ratio > worst[0]:
            worst = (ratio, c, ed, ef)
        if ed > SC.bound(c, ef, MARGIN):
            bad.append((ratio, ed, ef, c))
    print("RATIO %-44s %8.3g   (e_device %.3g, e_fp64 %.3g, (n + N) u %.3g: %s)" % (tag, worst[0], worst[2], worst[3], (worst[1].n + worst[1].N) * SC.U, (worst[1],)))
    assert not bad, (tag, len(bad), sorted(bad, key=lambda t: -t[0])[:5])


def _plain(r, i, c):
    return dict(sigma_f=r["sigma_f"][i], sigma_n=r["sigma_n"][i], nlml=r["nlml"][i], mean=r["mean"][i, :c.m], var=r["var"][i, :c.m])


def _plain_bytes(r, i, c):
    return [r[k][i].tobytes() for k in ("sigma_f", "nlml", "info", "sigma_n")] + [r["mean"][i, :c.m].tobytes(), r["var"][i, :c.m].tobytes()]


def _rows(r, prefix, i, c):
    return dict(mean=r[prefix + "_mean"][i, :c.n], var=r[prefix + "_var"][i, :c.n], nlpd=r[prefix + "_nlpd"][i], sse=r[prefix + "_sse"][i])


def _device_grad(r, i, c, common):
    k = 1 if common else c.N
    assert np.all(np.isnan(r["grad_ell"][i, k:])), "NaN behind a fit's derivatives"
    return np.concatenate([r["grad_ell"][i, :k], [r["grad_sn"][i]]])


def _check_launches(tag, dev, cases, batch):
    """every flavour of one upload against the references; the flavours' fits carry the plain launch's bytes; a second call the same bytes"""
    hp, f64 = [T.reference(c) for c in cases], [T.reference(c, SC.F64) for c in cases]
    assert np.all(dev["plain"]["info"] == 0)
    _judge(tag + " plain", [(c, SC.plain_error(_plain(dev["plain"], i, c), hp[i]), SC.plain_error(f64[i], hp[i])) for i, c in enumerate(cases)])
    items = []
    for i, c in enumerate(cases):
        common = c.kind in ("iso", "dup")
        key = "grad" if common else "grad_ard"
        items.append((c, SC._abs1(_device_grad(dev["grad"], i, c, common), hp[i][key]), SC._abs1(f64[i][key], hp[i][key])))
        if c.kind == "irrelevant":
            # every term of its sum is (l / 1e6)^2 <= 2e-10 of a relevant feature's; 1e-6 leaves four decades for the cancellation among those
            g = dev["grad"]["grad_ell"][i]
            assert abs(g[c.N // 2]) <= 1e-6 * max(1.0, np.max(np.abs(g[:c.N]))), "a feature at l = 1e6 has a derivative of ~ 0"
    _judge(tag + " grad", items)
    for k in dev["grad"]:
        assert dev["grad"][k].tobytes() == dev["again"][k].tobytes(), (tag, k, "a second call returns the same bytes")
    flavours = [("loo", "loo", (0, 0), dev["loo"])] + [("cv", "cv", bg, {m: dev["cv"][bg + (m,)] for m in SC.MODES}) for bg in batch.cv]
    flavours += [("hc", "hindcast", lm, {m: dev["hc"][lm + (m,)] for m in SC.MODES}) for lm in batch.hc]
    for fl, prefix, (a, b), by_mode in flavours:
        for mode in SC.MODES:
            r = by_mode[mode]
            items = []
            for i, c in enumerate(cases):
                ref, cmp_ = T.rows_of(c, SC.HP.name, fl, a, b)[mode], T.rows_of(c, SC.F64.name, fl, a, b)[mode]
                y = hp[i]["y"]
                items.append((c, SC.rows_error(_rows(r, prefix, i, c), ref, y), SC.rows_error(cmp_, ref, y)))
                assert np.all(np.isnan(r[prefix + "_mean"][i, c.n:])) and np.all(np.isnan(r[prefix + "_var"][i, c.n:]))
            _judge("%s %s(%d, %d) %s" % (tag, prefix, a, b, mode), items)
    for name, r in [("grad", dev["grad"])] + [(p + str(ab) + m, bm[m]) for _, p, ab, bm in flavours for m in SC.MODES]:
        for i, c in enumerate(cases):
            assert _plain_bytes(r, i, c) == _plain_bytes(dev["plain"], i, c), (tag, name, c, "the plain launch's bytes")


# ---- 1. accuracy, the plain launch's bytes, repeatability, one scale against N equal ones -----------------------------------------------------------
@pytest.mark.parametrize("key", BATCHES, ids=lambda k: "%s-%s" % k)
def test_every_output_of_every_flavour_within_the_bound(S, key):
    batch = T.batches()[key]
    mixed, alone, common = _results(S, key)
    tag = "%s %s" % (batch.kernel, batch.name)
    _check_launches(tag, mixed, batch.cases, batch)
    if not common:
        return
    _check_launches(tag + " ard=0", alone, common, batch)
    # a case with one scale: the launch with N equal scales forms the same fit, and the sum of its N components is the common derivative
    where = {c: i for i, c in enumerate(batch.cases)}
    for j, c in enumerate(common):
        i = where[c]
        assert _plain_bytes(mixed["plain"], i, c) == _plain_bytes(alone["plain"], j, c), (c, "N equal scales: the same division, the same bits")
        ga, gm = _device_grad(alone["grad"], j, c, True), _device_grad(mixed["grad"], i, c, True)
        ref, f64 = T.reference(c), T.reference(c, SC.F64)
        assert SC._abs1(gm, ref["grad"]) <= SC.bound(c, SC._abs1(f64["grad"], ref["grad"]), MARGIN), c
        assert np.max(np.abs(ga - gm)) <= 2 * SC.bound(c, SC._abs1(f64["grad"], ref["grad"]), MARGIN) * max(1.0, float(np.max(np.abs(ref["grad"])))), c


def test_a_batch_of_per_feature_fits_returns_all_components_of_one_scale_fits_too(S):
    """the raw entry with ard = 1 at equal scales: all N + 1 components against the reference's, and their sum against the common derivative"""
    from seaiceextentforecasting_amd import _lib as L
    c = next(c for c in T.TABLE if c.kind == "iso" and c.n == 33 and c.N > 1)
    X, y, Xs, ell = T.inputs(c)
    with S.GPR(kernel=c.kernel) as gp:
        sb = S.SmallStationaryBatch(gp)
        sb.add_dataset(X, y, Xs if c.m else None)
        sb.upload()
        si, sn = np.zeros(1, dtype=np.int64), np.array([c.sn])
        out, mean, var = np.zeros((1, 4)), np.zeros((1, 8)), np.zeros((1, 8))
        g = np.zeros((1, c.N + 3))
        ells = np.full((1, c.N), ell)
        gp._check(gp._lib.sigp_small_run_k_grad(gp._h, 1, L.iptr(si), gp._kid, L.ptr(ells), c.N, 1, L.ptr(sn), L.ptr(out), L.ptr(mean), L.ptr(var), 8, L.ptr(g), c.N + 3), "k_grad")
    ref, f64 = T.reference(c), T.reference(c, SC.F64)
    assert np.all(np.isnan(g[0, c.N + 1:]))
    b = SC.bound(c, SC._abs1(f64["grad_ard"], ref["grad_ard"]), MARGIN)
    assert SC._abs1(g[0, :c.N + 1], ref["grad_ard"]) <= b
    assert SC._abs1(np.array([np.cumsum(g[0, :c.N])[-1], g[0, c.N]]), ref["grad"]) <= SC.bound(c, SC._abs1(f64["grad"], ref["grad"]), MARGIN)


# ---- 2. against the blocked engine ----------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(b)
    assert np.array_equal(ok, ~np.isnan(a))
    return float(np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(b[ok])))


@pytest.mark.parametrize("kernel", T.KERNELS)
@pytest.mark.parametrize("n,N,m", [(45, 5, 3), (128, 9, 2)])
def test_agrees_with_the_blocked_engine(S, kernel, n, N, m):
    X, y, Xs, _ = SC.dataset(n, N, m, 20279000 + n)
    ell = np.array([H.roundtrip(v) for v in np.sqrt(N) * np.logspace(-0.3, 0.7, N)])
    sn = H.roundtrip(0.05)
    theta = np.log(np.concatenate([ell, [sn]]))
    cvs, hcs = ((1, 0), (5, 1), (30, 1)), ((1, 2), (32, 1))
    with S.GPR(kernel=kernel) as gp:
        gp.fit(X, y, ell, sn, Xs=Xs)
        big = dict(sigma_f=gp.sigma_f_, nlml=gp.nlml_, sigma_n=gp.sigma_n_, pred=gp.predict(Xs))
        big["loo"] = {mode: gp.loo(mode) for mode in SC.MODES}
        big["cv"] = {(b, g, mode): gp.cv(b, g, mode) for b, g in cvs for mode in SC.MODES}
        big["hc"] = {(l, mt, mode): gp.hindcast(l, mt, mode) for l, mt in hcs for mode in SC.MODES}
        big["grad"] = gp.nlml_ard(theta)
        big["iso"] = gp.fit(X, y, float(ell[0]), sn, Xs=Xs).nlml_
    with S.GPR(kernel=kernel) as gp:
        sb = S.SmallStationaryBatch(gp)
        ds = sb.add_dataset(X, y, Xs)
        sb.add_fit(ds, ell, sn)
        sb.add_fit(ds, float(ell[0]), sn)
        r, rg = sb.run(), sb.run(grad=True)
        for k in ("sigma_f", "nlml", "sigma_n"):
            assert _rel(r[k][0], big[k]) <= PARITY, k
        assert _rel(r["mean"][0], big["pred"][0]) <= PARITY and _rel(r["var"][0], big["pred"][1]) <= PARITY
        assert _rel(r["nlml"][1], big["iso"]) <= PARITY, "one common scale"
        assert _rel(rg["nlml"][0], big["grad"][0]) <= PARITY
        assert _rel(np.concatenate([rg["grad_ell"][0], [rg["grad_sn"][0]]]), big["grad"][1]) <= PARITY
        for mode in SC.MODES:
            q = sb.run(loo=mode)
            for a, b in (("loo_mean", "mean"), ("loo_var", "var"), ("loo_nlpd", "nlpd"), ("loo_sse", "sse")):
                assert _rel(q[a][0], big["loo"][mode][b]) <= PARITY, (mode, a)
            for bl, g in cvs:
                q = sb.run(cv=dict(block=bl, gap=g, sigma_f=mode))
                for a, b in (("cv_mean", "mean"), ("cv_var", "var"), ("cv_nlpd", "nlpd"), ("cv_sse", "sse")):
                    assert _rel(q[a][0], big["cv"][(bl, g, mode)][b]) <= PARITY, (mode, bl, g, a)
            for l, mt in hcs:
                q = sb.run(hindcast=dict(lead=l, min_train=mt, sigma_f=mode))
                for a, b in (("hindcast_mean", "mean"), ("hindcast_var", "var"), ("hindcast_nlpd", "nlpd"), ("hindcast_sse", "sse")):
                    assert _rel(q[a][0], big["hc"][(l, mt, mode)][b]) <= PARITY, (mode, l, mt, a)


# ---- 3. a non-SPD member ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", T.KERNELS)
def test_a_non_spd_member_at_the_largest_order_leaves_its_neighbours_alone(S, kernel):
    """rows 0 and 1 identical with sn~ = 0: K~(1, 0) = 1 exactly, an exact zero for the second pivot"""
    n, N = 128, 9
    X, y, _, _ = SC.dataset(n, N, 0, 20279500)
    Xb = X.copy()
    Xb[1] = Xb[0]
    ell = np.sqrt(N) * np.logspace(-0.3, 0.7, N)
    flavours = (dict(), dict(grad=True), dict(loo="refit"), dict(cv=dict(block=5, gap=1)), dict(hindcast=dict(lead=1, min_train=2)))
    with S.GPR(kernel=kernel) as gp:
        sb = S.SmallStationaryBatch(gp)
        good, bad = sb.add_dataset(X, y), sb.add_dataset(Xb, y)
        for ds, sn in ((good, 0.1), (bad, 0.0), (good, 1.0)):
            sb.add_fit(ds, ell, sn)
        with3 = [sb.run(**kw) for kw in flavours]
        sb.clear_fits()
        sb.add_fit(good, ell, 0.1)
        sb.add_fit(good, ell, 1.0)
        with2 = [sb.run(**kw) for kw in flavours]
    for kw, a, b in zip(flavours, with3, with2):
        assert list(a["info"]) == [0, 2, 0] and np.all(b["info"] == 0), kw
        assert a["sigma_f"][1] == np.inf and a["nlml"][1] == np.inf and a["sigma_n"][1] == np.inf
        for k in a:
            assert a[k][[0, 2]].tobytes() == b[k].tobytes(), (kw, k)
            assert np.all(np.isfinite(a[k][[0, 2]]) | (k.endswith(("_mean", "_var")) and "hindcast" in k)), (kw, k)
    assert np.all(with3[1]["grad_ell"][1] == np.inf) and with3[1]["grad_sn"][1] == np.inf, "+inf in every gradient entry"
    for r, p in zip(with3[2:], ("loo", "cv", "hindcast")):
        assert r[p + "_nlpd"][1] == np.inf and r[p + "_sse"][1] == np.inf
        assert np.all(np.isnan(r[p + "_mean"][1])) and np.all(np.isnan(r[p + "_var"][1]))


# ---- 4. the optimiser ---------------------------------------------------------------------------------------------------------------------------------
def test_optimize_small_ard_batch_finds_the_irrelevant_features(S):
    """6 data sets, n = 40, N = 5; y depends on features 0, 1, 2 alone"""
    B, n, N = 6, 40, 5
    rng = np.random.default_rng(20279600)
    X = rng.standard_normal((B, n, N))
    y = np.sin(1.5 * X[:, :, 0]) + 0.8 * X[:, :, 1] - 0.6 * X[:, :, 2] ** 2 + 0.3 * rng.standard_normal((B, n))
    y = y - y.mean(axis=1, keepdims=True)
    theta0 = np.array([np.log(2.0), np.log(0.1)])
    with S.GPR(kernel="rbf") as gp:
        small = gp.optimize_small_ard_batch(X, y, theta0, maxiter=100)
        at_x, g_x = gp.small_nlml_ard_batch(small["x"])
        blocked = gp.optimize_batch(X, y, theta0, ard=True, maxiter=100)
    print("OPTIMISE nfev %d / %d, nit %s / %s, fun %s / %s" % (small["nfev"], blocked["nfev"], small["nit"], blocked["nit"], small["fun"], blocked["fun"]))
    assert small["x"].shape == (B, N + 1) and np.all(small["converged"]), small
    assert at_x.tobytes() == small["fun"].tobytes() and g_x.tobytes() == small["jac"].tobytes(), "the value and gradient returned are those at x"
    assert np.all(small["fun"] <= blocked["fun"] + 1e-6), (small["fun"], blocked["fun"])
    for b in range(B):
        assert np.min(small["x"][b, 3:5]) > np.max(small["x"][b, :3]), (b, small["x"][b])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_offender_and_are_those_of_the_factored_entries(S):
    from seaiceextentforecasting_amd import _lib as L
    rng = np.random.default_rng(3)

    def entries(gp, nmax, ms=8):
        """the five entries past the Python checks: call(name, kid, ell [F, ldell], ldell, ard, extra..., ldg=) -> (code, message)"""
        def call(name, kid, ell, ldell, ard, *extra, ldg=None, sets=None):
            F = ell.shape[0]
            si = np.zeros(F, dtype=np.int64) if sets is None else np.asarray(sets, dtype=np.int64)
            sn = np.full(F, 0.1)
            out, mean, var = np.zeros((F, 8)), np.zeros((F, ms)), np.zeros((F, ms))
            tail = ()
            if name in ("loo", "cv", "hindcast"):
                tail = (L.ptr(np.zeros((F, nmax))), L.ptr(np.zeros((F, nmax))), nmax)
            if name == "grad":
                g = np.zeros((F, max(ldg, 1)))
                tail = (L.ptr(g), ldg)
            fn = getattr(gp._lib, "sigp_small_run_k" + ("_" + name if name else ""))
            rc = fn(gp._h, F, L.iptr(si), kid, L.ptr(np.ascontiguousarray(ell)), ldell, ard, L.ptr(sn), *extra, L.ptr(out), L.ptr(mean), L.ptr(var), ms, *tail)
            return rc, (gp._lib.sigp_last_error(gp._h) or b"").decode()
        return call

    def factored(gp, name, nmax, *extra, ds=0):
        si, ell, sn = np.full(1, ds, dtype=np.int64), np.array([0.05]), np.array([0.1])
        out, mean, var = np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 8))
        rc = getattr(gp._lib, "sigp_small_run_" + name)(gp._h, 1, L.iptr(si), L.ptr(ell), L.ptr(sn), *extra, L.ptr(out), L.ptr(mean), L.ptr(var), 8,
                                                         L.ptr(np.zeros((1, nmax))), L.ptr(np.zeros((1, nmax))), nmax)
        return rc, (gp._lib.sigp_last_error(gp._h) or b"").decode()

    with S.GPR(kernel="rbf") as gp:
        sb = S.SmallStationaryBatch(gp)
        sb.add_dataset(rng.standard_normal((40, 5)), rng.standard_normal(40), rng.standard_normal((2, 5)))
        sb.add_dataset(rng.standard_normal((20, 7)), rng.standard_normal(20))
        sb.add_fit(0, 1.0, 0.1)
        before = sb.run(grad=True)
        call = entries(gp, 40)
        one, five = np.ones((1, 1)), np.ones((1, 5))
        for kid in (0, 3, -1):
            rc, msg = call("", kid, one, 1, 0)
            assert rc == L.BAD_ARG and "kernel_id = %d" % kid in msg, msg
        for name, extra in (("", ()), ("grad", ()), ("loo", (0,)), ("cv", (5, 1, 0)), ("hindcast", (1, 2, 0))):
            kw = dict(ldg=6) if name == "grad" else {}
            for v in (0.0, -1.0, np.nan, np.inf, 1e-320):
                bad = five.copy(); bad[0, 3] = v
                rc, msg = call(name, 1, bad, 5, 1, *extra, **kw)
                assert rc == L.BAD_ARG and "fit 0" in msg and "length scale 3" in msg, (name, v, msg)
                rc, msg = call(name, 2, np.full((1, 1), v), 1, 0, *extra, **kw)
                assert rc == L.BAD_ARG and "length scale 0" in msg, (name, v, msg)
            rc, msg = call(name, 1, five[:, :4], 4, 1, *extra, **kw)
            assert rc == L.BAD_ARG and "ldell = 4" in msg and "N = 5" in msg, (name, msg)
            rc, msg = call(name, 1, one, 0, 0, *extra, **kw)
            assert rc == L.BAD_ARG and "ldell = 0" in msg, (name, msg)
            rc, msg = call(name, 1, one, 1, 2, *extra, **kw)
            assert rc == L.BAD_ARG and "ard" in msg, (name, msg)
            assert call(name, 1, five, 5, 1, *extra, **kw)[0] == L.OK and call(name, 2, one, 1, 0, *extra, **kw)[0] == L.OK
        rc, msg = call("grad", 1, five, 5, 1, ldg=5)
        assert rc == L.BAD_ARG and "ldg = 5" in msg and "6 derivatives" in msg, msg
        rc, msg = call("grad", 1, one, 1, 0, ldg=1)
        assert rc == L.BAD_ARG and "ldg = 1" in msg, msg
        rc, msg = call("grad", 1, np.ones((1, 7)), 7, 1, ldg=7, sets=[1])
        assert rc == L.BAD_ARG and "fit 0" in msg and "8 derivatives" in msg, msg
        # the folds', the lead's and the modes' limits: the factored entries' codes, and past the entry's name their messages
        for name, extras in (("cv", ((33, 0, 0), (1, 16, 0), (0, 0, 0), (5, -1, 0), (5, 1, 2), (20, 0, 0), (18, 7, 0))),
                             ("hindcast", ((33, 1, 0), (0, 2, 0), (1, 0, 0), (1, 2, 7), (32, 9, 0), (19, 2, 0))), ("loo", ((2,), (-1,)))):
            for extra in extras:
                rc, msg = call(name, 1, np.ones((1, 7)), 7, 1, *extra, sets=[1])
                frc, fmsg = factored(gp, name, 40, *extra, ds=1)
                assert rc == L.BAD_ARG and frc == L.BAD_ARG and msg.replace("small_run_k_", "small_run_") == fmsg, (name, extra, msg, fmsg)
        after = sb.run(grad=True)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), (k, "the handle stays usable")
    with S.GPR(kernel="matern52") as gp:            # the LDS limit of the leave-block-out launch: order 128 with m = 8
        sb = S.SmallStationaryBatch(gp)
        sb.add_dataset(rng.standard_normal((128, 3)), rng.standard_normal(128), rng.standard_normal((8, 3)))
        sb.add_fit(0, 1.0, 0.1)
        assert np.all(np.isfinite(sb.run(loo="refit")["loo_nlpd"]))
        with pytest.raises(ValueError, match=r"n = 128 with m = 8 leaves no LDS for the folds"):
            sb.run(cv=dict(block=5))
        rc, msg = entries(gp, 128)("cv", 2, np.ones((1, 1)), 1, 0, 5, 0, 0)
        frc, fmsg = factored(gp, "cv", 128, 5, 0, 0)
        assert rc == L.BAD_ARG and frc == L.BAD_ARG and msg == fmsg
        assert np.all(np.isfinite(sb.run(grad=True)["grad_ell"][:, 0]))
