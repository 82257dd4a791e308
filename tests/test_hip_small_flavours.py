"""GPU tier of the one-workgroup kernel (csrc/smallgp.hpp) in its five flavours -- plain, MLII gradient, leave-one-out, leave-block-out,
expanding-window hindcast -- at every order up to 128, feature counts past the chunk, m = 8 bordered rows, full and clipped windows,
lead = 32 and lam_mode 1 sets, against the long-double references of tests/small_cases.py (pinned by tests/test_small_cases_host.py).

The yardstick:  e_device <= 16 max(e_fp64, (n + N) u),  u = 2^-53.  e_fp64 is the error of an fp64 LAPACK evaluation of the same
formulas on the same staged inputs (never the code under test), (n + N) u the a-priori size of the n- and N-term sums both sides
form, 16 the project's margin over LAPACK (tests/test_hip_conditioning.py).  Every test prints its largest ratio e_device / max(...)
(``RATIO`` lines; docs/EXPERIMENTS.md records them).

Measured on an MI355X (largest ratio per flavour over all batches; bound 16): plain 7.85, gradient 6.55, leave-one-out 5.09,
leave-block-out 11.9, hindcast 7.85; per batch in docs/EXPERIMENTS.md, "One-workgroup kernel: five flavours at every order"."""
import os
import subprocess
import sys

import numpy as np
import pytest

import small_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")]
MARGIN = 16.0
PLAIN_KEYS = ("sigma_f", "nlml", "info", "sigma_n", "mean", "var")
ROW_KEYS = {"loo": "loo", "cv": "cv", "hc": "hindcast"}


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


# ---- launches, once per batch ------------------------------------------------------------------------------------------------------------------
def _launch_all(S, cases, cv=(), hc=(), order=None):
    """every flavour of one upload: dict(plain, grad, loo{mode}, cv{(block, gap)}{mode}, hc{(lead, min_train)}{mode})"""
    cases = list(cases) if order is None else [cases[i] for i in order]
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        SC.queue(sb, cases)
        out = dict(plain=sb.run(), grad=sb.run(grad=True), loo={mode: sb.run(loo=mode) for mode in SC.MODES}, cv={}, hc={})
        for block, gap in cv:
            out["cv"][(block, gap)] = {mode: sb.run(cv=dict(block=block, gap=gap, sigma_f=mode)) for mode in SC.MODES}
        for lead, mt in hc:
            out["hc"][(lead, mt)] = {mode: sb.run(hindcast=dict(lead=lead, min_train=mt, sigma_f=mode)) for mode in SC.MODES}
        out["plain_again"] = sb.run()
    return out


_RESULTS = {}


def _results(S, name):
    if name not in _RESULTS:
        b = SC.batches()[name]
        _RESULTS[name] = _launch_all(S, b.cases, b.cv, b.hc)
    return _RESULTS[name]


def _plain(r, i, c):
    assert np.all(np.isnan(r["mean"][i, c.m:])) and np.all(np.isnan(r["var"][i, c.m:])), "NaN beyond a set's m"
    return dict(sigma_f=r["sigma_f"][i], sigma_n=r["sigma_n"][i], nlml=r["nlml"][i], mean=r["mean"][i, :c.m], var=r["var"][i, :c.m])


def _rows(r, i, c, flavour):
    k = ROW_KEYS[flavour]
    assert np.all(np.isnan(r[k + "_mean"][i, c.n:])) and np.all(np.isnan(r[k + "_var"][i, c.n:])), "NaN beyond a set's n"
    return dict(mean=r[k + "_mean"][i, :c.n], var=r[k + "_var"][i, :c.n], nlpd=r[k + "_nlpd"][i], sse=r[k + "_sse"][i])


def _judge(tag, items):
    """items: (case, e_device, e_fp64).  Prints the largest ratio to max(e_fp64, (n + N) u) and holds every one to the margin."""
    worst, bad = (-1.0, None, 0.0, 0.0), []
    for c, ed, ef in items:
        assert np.isfinite(ed) and np.isfinite(ef), (tag, c, ed, ef)
        ratio = ed / max(ef, (c.n + c.N) * SC.U)
        if ratio > worst[0]:
            worst = (ratio, c, ed, ef)
        if ed > SC.bound(c, ef, MARGIN):
            bad.append((ratio, ed, ef, c))
    print("RATIO %-34s %8.3g   (e_device %.3g, e_fp64 %.3g, (n + N) u %.3g: %s)" % (tag, worst[0], worst[2], worst[3], (worst[1].n + worst[1].N) * SC.U, (worst[1],)))
    assert not bad, (tag, len(bad), sorted(bad, key=lambda t: -t[0])[:5])
    return worst[0]


def _rows_items(flavour, cases, dev, a=0, b=0):
    """(case, e_device, e_fp64) of a rows flavour over a batch, both sigma modes; the plain outputs of the launch count in"""
    items = []
    for mode in SC.MODES:
        r = dev[mode]
        assert np.all(r["info"] == 0)
        for i, c in enumerate(cases):
            ref, f64 = SC.reference(c), SC.reference(c, SC.F64)
            rr, fr = SC.rows_of(c, SC.HP.name, flavour, a, b)[mode], SC.rows_of(c, SC.F64.name, flavour, a, b)[mode]
            got = _rows(r, i, c, flavour)
            if flavour == "cv":         # scores finite and no row NaN, or both scores +inf and every row NaN: no mixture
                assert np.isfinite(got["nlpd"]) and np.isfinite(got["sse"]) and not np.any(np.isnan(got["mean"])) and not np.any(np.isnan(got["var"])), (c, mode)
            items.append((c, max(SC.rows_error(got, rr, ref["y"]), SC.plain_error(_plain(r, i, c), ref)),
                          max(SC.rows_error(fr, rr, ref["y"]), SC.plain_error(f64, ref))))
    return items


# ---- 1. the five flavours against the bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_plain_and_gradient_within_the_bound(S, name):
    b, dev = SC.batches()[name], _results(S, name)
    assert np.all(dev["plain"]["info"] == 0) and np.all(dev["grad"]["info"] == 0)
    plain, grad = [], []
    for i, c in enumerate(b.cases):
        ref, f64 = SC.reference(c), SC.reference(c, SC.F64)
        plain.append((c, SC.plain_error(_plain(dev["plain"], i, c), ref), SC.plain_error(f64, ref)))
        grad.append((c, max(SC.grad_error(dev["grad"]["grad_exact"][i], ref), SC.plain_error(_plain(dev["grad"], i, c), ref)),
                     max(SC.grad_error(f64["grad"], ref), SC.plain_error(f64, ref))))
    _judge("plain %s" % name, plain)
    _judge("grad %s" % name, grad)
    for k in PLAIN_KEYS:      # the same launch twice, and the gradient launch's plain outputs: the same bits
        assert dev["plain"][k].tobytes() == dev["plain_again"][k].tobytes() == dev["grad"][k].tobytes(), k


@pytest.mark.parametrize("name", ["a", "b"])
def test_leave_one_out_within_the_bound(S, name):
    b, dev = SC.batches()[name], _results(S, name)
    _judge("loo %s" % name, _rows_items("loo", b.cases, dev["loo"]))


@pytest.mark.parametrize("name", ["a", "mid", "s2", "s15", "c16", "c8"])
def test_leave_block_out_within_the_bound(S, name):
    """mid: every layout at the upload's chunk 32; s2 / s15: the small windows, (n_min - 1, 0) among them; c16 / c8: orders 113 .. 128 at the
    launch's own chunk 16 and 8.  (Batch b cannot run this flavour: n = 128 with m = 8 is beyond its LDS at any chunk.)"""
    b, dev = SC.batches()[name], _results(S, name)
    assert b.cv and set(dev["cv"]) == set(b.cv)
    for bg in b.cv:
        _judge("cv %s block=%d gap=%d" % ((name,) + bg), _rows_items("cv", b.cases, dev["cv"][bg], *bg))


@pytest.mark.parametrize("name", ["a", "b", "mid", "big", "s2", "s15"])
def test_hindcast_within_the_bound(S, name):
    b, dev = SC.batches()[name], _results(S, name)
    assert b.hc and set(dev["hc"]) == set(b.hc)
    for lm in b.hc:
        items = _rows_items("hc", b.cases, dev["hc"][lm], *lm)         # rows_error: NaN exactly on the rows that are not scored
        _judge("hc %s lead=%d min_train=%d" % ((name,) + lm), items)
    one = [c for c in b.cases if c.n - b.one_row[0] == b.one_row[1]]
    assert one
    i = b.cases.index(one[0])
    assert np.count_nonzero(~np.isnan(dev["hc"][b.one_row]["refit"]["hindcast_var"][i])) == 1


# ---- 2. flavour launches carry the plain launch's bits (the leave-block-out launch keeps the upload's chunk here) --------------------------------
@pytest.mark.parametrize("name", ["a", "mid", "s15"])
def test_flavour_launches_carry_the_plain_launch_bits(S, name):
    b, dev = SC.batches()[name], _results(S, name)
    assert b.cv_chunk == b.chunk
    launches = [("loo", dev["loo"])] + [("cv", dev["cv"][bg]) for bg in b.cv] + [("hc", dev["hc"][lm]) for lm in b.hc]
    for flavour, byMode in launches:
        for mode in SC.MODES:
            for k in PLAIN_KEYS:
                assert byMode[mode][k].tobytes() == dev["plain"][k].tobytes(), (flavour, mode, k)
        k = ROW_KEYS[flavour] + "_mean"
        assert byMode["refit"][k].tobytes() == byMode["fixed"][k].tobytes(), (flavour, "the means do not depend on the mode")
        assert byMode["refit"][ROW_KEYS[flavour] + "_sse"].tobytes() == byMode["fixed"][ROW_KEYS[flavour] + "_sse"].tobytes()


# ---- 3. cross-flavour identities, at the bound --------------------------------------------------------------------------------------------------
def _row_norms(L, lead, min_train):
    """sum_{j = t - lead + 1 .. t} L(t, j)^2 for the rows t >= min_train + lead - 1, NaN elsewhere, in L's own arithmetic"""
    n = L.shape[0]
    t, j = np.arange(n)[:, None], np.arange(n)[None, :]
    w = np.sum(np.where((j > t - lead) & (j <= t), L * L, 0), axis=1)
    return np.where(np.arange(n) >= min_train + lead - 1, w, np.nan)


@pytest.mark.parametrize("name", ["mid", "s15", "c8"])
def test_block_one_is_leave_one_out_and_fixed_hindcast_variances_are_row_norms(S, name):
    """The leave-block-out launch at (1, 0) measured against the reference's LEAVE-ONE-OUT rows, and the hindcast launch's "fixed" rows
    against sigma_f sum_{j=s..t} L~(t,j)^2 formed HERE from the reference's L~ (``_row_norms``: a masked row sum, not the row loop of
    ``small_cases.hc_rows``).  Both are held to the error of the fit in the flavour -- every output of the launch, as everywhere in this
    file -- against the comparator's.  The ratio of the variances alone is printed, not asserted: one output of an ill-conditioned fit is
    one draw of the comparator's error (docs/EXPERIMENTS.md, "One ratio above 16, run down")."""
    b, dev = SC.batches()[name], _results(S, name)
    items = []
    for mode in SC.MODES:
        r = dev["cv"][(1, 0)][mode]
        for i, c in enumerate(b.cases):
            ref, f64 = SC.reference(c), SC.reference(c, SC.F64)
            rr, fr = SC.rows_of(c, SC.HP.name, "loo")[mode], SC.rows_of(c, SC.F64.name, "loo")[mode]
            items.append((c, max(SC.rows_error(_rows(r, i, c, "cv"), rr, ref["y"]), SC.plain_error(_plain(r, i, c), ref)),
                          max(SC.rows_error(fr, rr, ref["y"]), SC.plain_error(f64, ref))))
    _judge("cv(1, 0) against loo %s" % name, items)
    items, alone = [], []
    for lm in b.hc:
        r = dev["hc"][lm]["fixed"]
        for i, c in enumerate(b.cases):
            ref, f64 = SC.reference(c), SC.reference(c, SC.F64)
            rr, fr = SC.rows_of(c, SC.HP.name, "hc", *lm)["fixed"], SC.rows_of(c, SC.F64.name, "hc", *lm)["fixed"]
            want = dict(rr, var=ref["sigma_f"] * _row_norms(ref["L"], *lm))
            items.append((c, max(SC.rows_error(_rows(r, i, c, "hc"), want, ref["y"]), SC.plain_error(_plain(r, i, c), ref)),
                          max(SC.rows_error(fr, want, ref["y"]), SC.plain_error(f64, ref))))
            ok = ~np.isnan(want["var"].astype(np.float64))
            alone.append(SC._rel(r["hindcast_var"][i, :c.n][ok], want["var"][ok]) / max(SC._rel(fr["var"][ok], want["var"][ok]), (c.n + c.N) * SC.U))
    print("variances alone, largest ratio (not asserted) %s: %.3g" % (name, max(alone)))
    _judge("hc fixed var = sigma_f |L~ row|^2 %s" % name, items)


# ---- 4. a fit's bits do not depend on its place in the launch, on its neighbours or on the upload -----------------------------------------------
def _fit_bytes(dev, i, c, cv, hc):
    """every output of fit i (case c), trimmed to its own m and n: the paddings' widths belong to the upload"""
    def plain(r):
        return [r[k][i].tobytes() for k in ("sigma_f", "nlml", "info", "sigma_n")] + [r["mean"][i, :c.m].tobytes(), r["var"][i, :c.m].tobytes()]
    parts = plain(dev["plain"]) + plain(dev["grad"]) + [dev["grad"]["grad_exact"][i].tobytes(), dev["grad"]["grad_ref"][i].tobytes()]
    for flavour, byMode in [("loo", dev["loo"])] + [("cv", dev["cv"][bg]) for bg in cv] + [("hc", dev["hc"][lm]) for lm in hc]:
        for mode in SC.MODES:
            r, k = byMode[mode], ROW_KEYS[flavour]
            parts += plain(r) + [r[k + "_mean"][i, :c.n].tobytes(), r[k + "_var"][i, :c.n].tobytes(), r[k + "_nlpd"][i].tobytes(), r[k + "_sse"][i].tobytes()]
    return parts


def test_results_do_not_depend_on_the_order_of_the_queue(S):
    b, dev = SC.batches()["mid"], _results(S, "mid")
    F = len(b.cases)
    cv, hc = ((7, 3), (32, 0)), ((2, 3), (32, 1))
    rev = _launch_all(S, b.cases, cv, hc, order=list(range(F - 1, -1, -1)))
    twice = _launch_all(S, b.cases, cv, hc, order=[i // 2 for i in range(2 * F)])
    for i in range(F):
        c = b.cases[i]
        mine = _fit_bytes(dev, i, c, cv, hc)
        assert mine == _fit_bytes(rev, F - 1 - i, c, cv, hc), c
        assert mine == _fit_bytes(twice, 2 * i, c, cv, hc) == _fit_bytes(twice, 2 * i + 1, c, cv, hc), c


def test_a_single_chunk_fit_alone_has_the_bits_it_has_in_the_batch(S):
    """N <= 8: one feature chunk at any ch, summed in the same order -- alone (its own nmax, mmax, ch) as in batch b (chunk 16)"""
    b, dev = SC.batches()["b"], _results(S, "b")
    picked = [min(i for i, c in enumerate(b.cases) if c.N <= 8 and c.n == n) for n in (17, 49, 96, 128)]
    for i in picked:
        alone = _launch_all(S, [b.cases[i]], (), b.hc)
        assert _fit_bytes(alone, 0, b.cases[i], (), b.hc) == _fit_bytes(dev, i, b.cases[i], (), b.hc), b.cases[i]


# ---- 5. a non-SPD member at size, between two good fits of the same order -----------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "grad", "loo", "cv", "hc"])
def test_a_non_spd_member_at_size_leaves_its_neighbours_alone(S, flavour):
    """n = 128, m = 8, duplicate rows, sn~ = 0, N = 17 < n (n = 125 for the leave-block-out launch: the largest order it takes at m = 8)"""
    n, m, N = (125 if flavour == "cv" else 128), 8, 17
    X, y, Xs, M = SC.dataset(n, N, m, 20263000 + n)
    Xb = X.copy()
    Xb[n // 2:] = X[:n - n // 2]
    kw = dict(plain={}, grad=dict(grad=True), loo=dict(loo="refit"), cv=dict(cv=dict(block=30, gap=1)), hc=dict(hindcast=dict(lead=32, min_train=1)))[flavour]
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        good, bad = sb.add_dataset(X, y, Xs, M), sb.add_dataset(Xb, y, Xs, M)
        for ds, sn in ((good, 0.1), (bad, 0.0), (good, 1.0)):
            sb.add_fit(ds, 0.05, sn)
        with3 = sb.run(**kw)
        sb.clear_fits()                     # the bad set stays staged: nmax, mmax and the chunk are unchanged
        sb.add_fit(good, 0.05, 0.1)
        sb.add_fit(good, 0.05, 1.0)
        with2 = sb.run(**kw)
    assert 1 <= with3["info"][1] <= n and with3["info"][0] == 0 and with3["info"][2] == 0 and np.all(with2["info"] == 0)
    assert np.all(np.isnan(with3["mean"][1])) and np.all(np.isnan(with3["var"][1])) and with3["sigma_f"][1] == np.inf and with3["nlml"][1] == np.inf
    if flavour == "grad":
        assert np.all(with3["grad_exact"][1] == np.inf) and np.all(with3["grad_ref"][1] == np.inf)
    if flavour in ROW_KEYS:
        k = ROW_KEYS[flavour]
        assert with3[k + "_nlpd"][1] == np.inf and with3[k + "_sse"][1] == np.inf
        assert np.all(np.isnan(with3[k + "_mean"][1])) and np.all(np.isnan(with3[k + "_var"][1]))
        assert np.all(np.isfinite(with3[k + "_nlpd"][[0, 2]])) and np.all(np.isfinite(with3[k + "_sse"][[0, 2]]))
    for k in with3:
        assert with3[k][[0, 2]].tobytes() == with2[k].tobytes(), k


# ---- 6. the leave-block-out launch and LDS --------------------------------------------------------------------------------------------------------
def _anchor(S, n, m):
    """one data set (n, m), N = 17 (three chunks of 8), one fit: (plain, loo, cv or the refusal's message, plain and loo after it)"""
    c = SC.Case(n, 17, m, 0.05, 1.0, "eigh", 20264000 + 10 * n + m)
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        SC.queue(sb, [c])
        before = (sb.run(), sb.run(loo="refit"))
        try:
            cv = {mode: sb.run(cv=dict(block=30, gap=1, sigma_f=mode)) for mode in SC.MODES}
        except ValueError as e:
            cv = str(e)
        after = (sb.run(), sb.run(loo="refit"))
    for x, y in zip(before, after):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), ("the handle's other launches changed", n, m, k)
    return c, cv


@pytest.mark.parametrize("n,m", [(128, 0), (128, 2), (127, 3), (125, 8)])
def test_leave_block_out_is_accepted_up_to_its_lds_limit(S, n, m):
    assert SC.cv_chunk(n, m) == 8 and SC.cv_chunk(n, m, before_fix=True) is None and (n == 128 or SC.cv_chunk(n + 1, m) is None)
    c, cv = _anchor(S, n, m)
    assert isinstance(cv, dict), cv
    _judge("cv anchor n=%d m=%d block=30 gap=1" % (n, m), _rows_items("cv", [c], cv, 30, 1))


@pytest.mark.parametrize("n,m", [(128, 3), (126, 8)])
def test_leave_block_out_is_refused_beyond_its_lds_limit_and_the_handle_stays_usable(S, n, m):
    assert SC.cv_chunk(n, m) is None and SC.upload_chunk(n, m) == 16
    c, cv = _anchor(S, n, m)            # ValueError is SIGP_BAD_ARG (GPR._check); _anchor compares the launches around it
    assert isinstance(cv, str) and "LDS" in cv and "n = %d with m = %d" % (n, m) in cv, cv


# ---- 7. small_nt64: one wavefront per fit (debug library only, plain flavour, nmax <= 64) ----------------------------------------------------
def _nt64_cases():
    return [c for c in SC.TABLE if c.n <= 64]


def run_nt64(path):
    """in a process that loaded libsigp_debug.so: the orders <= 64 of the table with the option off and on"""
    import seaiceextentforecasting_amd as S
    res = {}
    with S.GPR(kernel="netdiffusion") as gp:
        sb = S.SmallBatch(gp)
        SC.queue(sb, _nt64_cases())
        for on in (0, 1):
            gp.set_option("small_nt64", on)
            r = sb.run()
            res.update({"%s_%d" % (k, on): r[k] for k in PLAIN_KEYS})
    np.savez(path, **res)


def test_small_nt64_within_the_bound_on_the_debug_library(tmp_path):
    out = str(tmp_path / "nt64.npz")
    env = dict(os.environ, SIGP_USE_DEBUG_LIB="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_hip_small_flavours as T; T.run_nt64(%r)" % (os.path.join(ROOT, "tests"), ROOT, out)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    cases = _nt64_cases()
    for on in (0, 1):
        r = {k: z["%s_%d" % (k, on)] for k in PLAIN_KEYS}
        assert np.all(r["info"] == 0)
        items = [(c, SC.plain_error(_plain(r, i, c), SC.reference(c)), SC.plain_error(SC.reference(c, SC.F64), SC.reference(c))) for i, c in enumerate(cases)]
        _judge("plain small_nt64=%d (orders <= 64)" % on, items)
