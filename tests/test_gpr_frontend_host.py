"""CPU tier of the Python front end of the validation-score families (``GPR.loo* / cv* / hindcast* / *_objective* / optimize*``): what every
public method hands to the library -- the entries in order, with their scalar arguments --, what it returns (keys, shapes, dtypes), the handle's
state afterwards, the ``theta`` an optimiser's objective receives and the ``refit`` it ends with, and which refusal fires first when two
arguments are bad at once.  Everything goes through the public API on a handle whose library is a recording stand-in: no device."""
import inspect

import numpy as np
import pytest

from seaiceextentforecasting_amd import _lib as L
from test_cv_ard_batch_host import _handle

D, N, F, BLOCK, GAP, LEAD, MT, GROUP = 3, 40, 3, 5, 1, 2, 4, 4
TH = np.array([[0.25, -0.5, 0.75, -2.0], [0.5, 0.0, -0.25, -1.0], [-0.5, 0.25, 0.0, -3.0]])       # [F, d + 1]
TH2 = np.array([[0.25, -2.0], [0.5, -1.0], [-0.5, -3.0]])                                           # [F, 2]
ELL, SN = np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3])
GRID = dict(ells=[1.0, 2.0], sns=[0.1, 0.2, 0.3])


class Recording:
    """stands for the library: every entry appends (its name, its int / float / bytes arguments) to ``calls`` and returns 0 (SIGP_OK); nothing
    is written through a pointer, so every output buffer keeps its zeros"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(a.item() if isinstance(a, np.generic) else a for a in args if isinstance(a, (int, float, bytes, np.integer, np.floating)))))
            return 0
        return entry


def _batch(kernel="rbf", dtype="f64", staged=True):
    """a handle with F-independent data sets staged (``_batch_d`` / ``_batch_n``), no single fit"""
    gp = _handle(kernel, dtype, *((D, N) if staged else ()))
    gp._lib, gp._kid, gp._fitted, gp._has_data, gp._ard, gp._ride = Recording(), L.KERNEL_IDS[kernel], False, False, False, None
    return gp


def _single(kernel="rbf", dtype="f64", fitted=True, data=True):
    """a handle with one data set staged and (``fitted``) a fit on the device"""
    gp = _batch(kernel, dtype, staged=False)
    if data:
        gp.n, gp.d, gp._X, gp._y, gp._M, gp._has_data, gp._fitted = N, D, np.zeros((N, D)), np.linspace(-1.0, 1.0, N), None, True, fitted
    return gp


def _xy(B=None):
    rng = np.random.default_rng(7)
    return (rng.standard_normal((N, D)), rng.standard_normal(N)) if B is None else (rng.standard_normal((B, N, D)), rng.standard_normal((B, N)))


def _shapes(r):
    """the shape of a result: dict -> {key: (shape, dtype)}, tuple -> a tuple of (shape, dtype); None stays None"""
    if isinstance(r, dict):
        return {k: _shapes(v) for k, v in r.items()}
    if isinstance(r, tuple):
        return tuple(_shapes(v) for v in r)
    if r is None or isinstance(r, slice):
        return r
    return (np.shape(r), np.asarray(r).dtype.str)


def _bound(name, a, kw):
    """how ``GPR.<name>`` reads the arguments behind its first one: {parameter: value} with the defaults filled in (a call may name an
    argument or pass it by position: the same call)"""
    from seaiceextentforecasting_amd import GPR
    b = inspect.signature(getattr(GPR, name)).bind(None, None, *a, **kw)
    b.apply_defaults()
    return dict(list(b.arguments.items())[2:])


SET, UP, RES = ("sigp_set_option", (b"group", GROUP)), ("sigp_batch_upload", (1, N * D, N, 0, N, D, 0)), ("sigp_batch_reserve", (GROUP, 1))
S0, V, M, FN, F2, FD = ((), "<f8"), ((N,), "<f8"), ((F, N), "<f8"), ((F,), "<f8"), ((F, 2), "<f8"), ((F, D + 1), "<f8")
G6 = ((2, 3), "<f8")
SINGLE = dict(mean=V, var=V, nlpd=S0, sse=S0, mse=S0, skill=S0)
ARD1 = dict(value=S0, grad=((D + 1,), "<f8"), mean=V, var=V, nlpd=S0, sse=S0)
ARDF = dict(value=FN, grad=FD, mean=M, var=M, nlpd=FN, sse=FN)
AFTER = [("sigp_fit", ())]          # _after_ard_call without ride points

# name -> (handle, call, the library entries in order with their scalar arguments, the result's shape, (_fitted, _ard) afterwards)
HAPPY = {
    "loo": (_single, lambda gp: gp.loo(), [("sigp_loo", (0,))], SINGLE, (True, False)),
    "loo fixed grad": (_single, lambda gp: gp.loo("fixed", grad=True), [("sigp_loo_grad", (1, 0))], dict(SINGLE, nlpd_grad=((2,), "<f8"), sse_grad=((2,), "<f8")), (True, False)),
    "cv": (_single, lambda gp: gp.cv(BLOCK, gap=GAP), [("sigp_cv", (BLOCK, GAP, 0))], dict(SINGLE, folds=((8, 4), "<i8")), (True, False)),
    "hindcast": (_single, lambda gp: gp.hindcast(LEAD, MT, "fixed"), [("sigp_hindcast", (LEAD, MT, 1))], dict(SINGLE, scored=slice(MT + LEAD - 1, N)), (True, False)),
    "hindcast default min_train": (_single, lambda gp: gp.hindcast(), [("sigp_hindcast", (1, D + 1, 0))], dict(SINGLE, scored=slice(D + 1, N)), (True, False)),
    "loo_batch": (_batch, lambda gp: gp.loo_batch(ELL, SN, first=1, group=GROUP), [SET, ("sigp_loo_batch", (1, F, 1, 0, N))], dict(nlpd=FN, sse=FN, mean=M, var=M), (False, False)),
    "loo_batch grad": (_batch, lambda gp: gp.loo_batch(ELL, SN, sigma_f="fixed", group=GROUP, predictions=False, grad=True),
                       [SET, ("sigp_loo_grad_batch", (0, F, 1, 1, N))], dict(nlpd=FN, sse=FN, nlpd_grad=F2, sse_grad=F2), (False, False)),
    "cv_batch": (_batch, lambda gp: gp.cv_batch(ELL, SN, BLOCK, gap=GAP, group=GROUP), [SET, ("sigp_cv_batch", (0, F, 1, BLOCK, GAP, 0, N))],
                 dict(nlpd=FN, sse=FN, mean=M, var=M), (False, False)),
    "cv_batch scores": (_batch, lambda gp: gp.cv_batch(ELL, SN, BLOCK, group=GROUP, predictions=False), [SET, ("sigp_cv_batch", (0, F, 1, BLOCK, 0, 0, N))],
                        dict(nlpd=FN, sse=FN), (False, False)),
    "hindcast_batch": (_batch, lambda gp: gp.hindcast_batch(ELL, SN, lead=LEAD, group=GROUP), [SET, ("sigp_hindcast_batch", (0, F, 1, LEAD, D + 1, 0, N))],
                       dict(nlpd=FN, sse=FN, mean=M, var=M), (False, False)),
    "hindcast_batch scores": (_batch, lambda gp: gp.hindcast_batch(ELL, SN, LEAD, MT, sigma_f="fixed", group=GROUP, predictions=False),
                              [SET, ("sigp_hindcast_batch", (0, F, 1, LEAD, MT, 1, N))], dict(nlpd=FN, sse=FN), (False, False)),
    "loo_grid": (_batch, lambda gp: gp.loo_grid(*_xy(), group=GROUP, **GRID), [UP, RES, SET, ("sigp_loo_batch", (0, 6, 1, 0, N))], dict(nlpd=G6, sse=G6), (False, False)),
    "cv_grid": (_batch, lambda gp: gp.cv_grid(*_xy(), block=BLOCK, gap=GAP, group=GROUP, **GRID), [UP, RES, SET, ("sigp_cv_batch", (0, 6, 1, BLOCK, GAP, 0, N))],
                dict(nlpd=G6, sse=G6), (False, False)),
    "hindcast_grid": (_batch, lambda gp: gp.hindcast_grid(*_xy(), lead=LEAD, group=GROUP, **GRID), [UP, RES, SET, ("sigp_hindcast_batch", (0, 6, 1, LEAD, D + 1, 0, N))],
                      dict(nlpd=G6, sse=G6), (False, False)),
    "nlml_ard": (_single, lambda gp: gp.nlml_ard(TH[0]), [("sigp_nlml_grad_ard", (1, D + 1, 2))] + AFTER, (S0, ((D + 1,), "<f8")), (True, True)),
    "nlml_ard value": (_single, lambda gp: gp.nlml_ard(TH[0], grad=None), [("sigp_nlml_grad_ard", (1, D + 1, 0))] + AFTER, (S0, None), (True, True)),
    "loo_ard": (_single, lambda gp: gp.loo_ard(TH[0], "loo_sse", "fixed"), [("sigp_loo_grad_ard", (1, D + 1, 1, 1))] + AFTER, (S0, ((D + 1,), "<f8")), (True, True)),
    "loo_ard value": (_single, lambda gp: gp.loo_ard(TH[0], grad=None), [("sigp_loo_grad_ard", (1, D + 1, 0, 0))] + AFTER, (S0, None), (True, True)),
    "loo_ard predictions": (_single, lambda gp: gp.loo_ard(TH[0], predictions=True), [("sigp_loo_grad_ard", (1, D + 1, 0, 0))] + AFTER, ARD1, (True, True)),
    "cv_ard": (_single, lambda gp: gp.cv_ard(TH[0], BLOCK, GAP, "cv_sse", "fixed"), [("sigp_cv_grad_ard", (1, D + 1, BLOCK, GAP, 1, 1))] + AFTER,
               (S0, ((D + 1,), "<f8")), (True, True)),
    "cv_ard value": (_single, lambda gp: gp.cv_ard(TH[0], BLOCK, grad=None), [("sigp_cv_grad_ard", (1, D + 1, BLOCK, 0, 0, 0))] + AFTER, (S0, None), (True, True)),
    "cv_ard predictions": (_single, lambda gp: gp.cv_ard(TH[0], BLOCK, predictions=True), [("sigp_cv_grad_ard", (1, D + 1, BLOCK, 0, 0, 0))] + AFTER, ARD1, (True, True)),
    "hindcast_ard": (_single, lambda gp: gp.hindcast_ard(TH[0], LEAD, MT, "hindcast_sse", "fixed"), [("sigp_hindcast_grad_ard", (1, D + 1, LEAD, MT, 1, 1))] + AFTER,
                     (S0, ((D + 1,), "<f8")), (True, True)),
    "hindcast_ard value": (_single, lambda gp: gp.hindcast_ard(TH[0], grad=None), [("sigp_hindcast_grad_ard", (1, D + 1, 1, D + 1, 0, 0))] + AFTER, (S0, None), (True, True)),
    "hindcast_ard predictions": (_single, lambda gp: gp.hindcast_ard(TH[0], predictions=True), [("sigp_hindcast_grad_ard", (1, D + 1, 1, D + 1, 0, 0))] + AFTER, ARD1,
                                 (True, True)),
    "cv_objective": (_single, lambda gp: gp.cv_objective(TH2[0], BLOCK, GAP), [("sigp_cv_grad_ard", (1, D + 1, BLOCK, GAP, 0, 0))] + AFTER, (S0, ((2,), "<f8")), (True, True)),
    "hindcast_objective": (_single, lambda gp: gp.hindcast_objective(TH2[0], LEAD), [("sigp_hindcast_grad_ard", (1, D + 1, LEAD, D + 1, 0, 0))] + AFTER,
                           (S0, ((2,), "<f8")), (True, True)),
    "loo_objective": (_single, lambda gp: gp.loo_objective(np.zeros(2), "loo_sse", "fixed"), [("sigp_fit_predict", (1, 1.0, 1.0, 0)), ("sigp_loo_grad", (1, 0))],
                      (S0, ((2,), "<f8")), (True, False)),
    "nlml_ard_batch": (_batch, lambda gp: gp.nlml_ard_batch(TH, first=1, group=GROUP), [SET, ("sigp_nlml_grad_ard_batch", (1, F, 1, D + 1, D + 1, 2, D + 1))], (FN, FD),
                       (False, False)),
    "nlml_ard_batch value": (_batch, lambda gp: gp.nlml_ard_batch(TH, grad=None, group=GROUP), [SET, ("sigp_nlml_grad_ard_batch", (0, F, 1, D + 1, D + 1, 0, D + 1))], (FN, None),
                             (False, False)),
    "loo_ard_batch": (_batch, lambda gp: gp.loo_ard_batch(TH, 1, "loo_sse", "fixed", group=GROUP), [SET, ("sigp_loo_grad_ard_batch", (1, F, 1, D + 1, D + 1, 1, 1, N, D + 1))],
                      (FN, FD), (False, False)),
    "loo_ard_batch value": (_batch, lambda gp: gp.loo_ard_batch(TH, grad=None, group=GROUP), [SET, ("sigp_loo_grad_ard_batch", (0, F, 1, D + 1, D + 1, 0, 0, N, D + 1))],
                            (FN, None), (False, False)),
    "loo_ard_batch predictions": (_batch, lambda gp: gp.loo_ard_batch(TH, group=GROUP, predictions=True),
                                  [SET, ("sigp_loo_grad_ard_batch", (0, F, 1, D + 1, D + 1, 0, 0, N, D + 1))], ARDF, (False, False)),
    "cv_ard_batch": (_batch, lambda gp: gp.cv_ard_batch(TH, BLOCK, GAP, 1, "cv_sse", "fixed", group=GROUP),
                     [SET, ("sigp_cv_grad_ard_batch", (1, F, 1, D + 1, D + 1, BLOCK, GAP, 1, 1, N, D + 1))], (FN, FD), (False, False)),
    "cv_ard_batch value": (_batch, lambda gp: gp.cv_ard_batch(TH, BLOCK, grad=None, group=GROUP),
                           [SET, ("sigp_cv_grad_ard_batch", (0, F, 1, D + 1, D + 1, BLOCK, 0, 0, 0, N, D + 1))], (FN, None), (False, False)),
    "cv_ard_batch predictions": (_batch, lambda gp: gp.cv_ard_batch(TH, BLOCK, group=GROUP, predictions=True),
                                 [SET, ("sigp_cv_grad_ard_batch", (0, F, 1, D + 1, D + 1, BLOCK, 0, 0, 0, N, D + 1))], ARDF, (False, False)),
    "hindcast_ard_batch": (_batch, lambda gp: gp.hindcast_ard_batch(TH, LEAD, MT, 1, "hindcast_sse", "fixed", group=GROUP),
                           [SET, ("sigp_hindcast_grad_ard_batch", (1, F, 1, D + 1, D + 1, LEAD, MT, 1, 1, N, D + 1))], (FN, FD), (False, False)),
    "hindcast_ard_batch value": (_batch, lambda gp: gp.hindcast_ard_batch(TH, grad=None, group=GROUP),
                                 [SET, ("sigp_hindcast_grad_ard_batch", (0, F, 1, D + 1, D + 1, 1, D + 1, 0, 0, N, D + 1))], (FN, None), (False, False)),
    "hindcast_ard_batch predictions": (_batch, lambda gp: gp.hindcast_ard_batch(TH, group=GROUP, predictions=True),
                                       [SET, ("sigp_hindcast_grad_ard_batch", (0, F, 1, D + 1, D + 1, 1, D + 1, 0, 0, N, D + 1))], ARDF, (False, False)),
    "cv_objective_batch": (_batch, lambda gp: gp.cv_objective_batch(TH2, BLOCK, GAP, 1, "cv_sse", "fixed", GROUP),
                           [SET, ("sigp_cv_grad_ard_batch", (1, F, 1, D + 1, D + 1, BLOCK, GAP, 1, 1, N, D + 1))], (FN, F2), (False, False)),
    "hindcast_objective_batch": (_batch, lambda gp: gp.hindcast_objective_batch(TH2, LEAD, None, 1, "hindcast_sse", "fixed", GROUP),
                                 [SET, ("sigp_hindcast_grad_ard_batch", (1, F, 1, D + 1, D + 1, LEAD, D + 1, 1, 1, N, D + 1))], (FN, F2), (False, False)),
}


@pytest.mark.parametrize("name", sorted(HAPPY))
def test_entries_called_results_and_state(name):
    make, call, entries, shapes, state = HAPPY[name]
    gp = make()
    r = call(gp)
    assert gp._lib.calls == entries
    assert _shapes(r) == shapes
    assert (gp._fitted, gp._ard) == state


def test_ard_calls_leave_the_fit_at_exp_theta_and_read_the_ride_predictions():
    """after ``*_ard`` the handle is fitted at exp(theta) by the C library's exp, scales set; ride points are read back"""
    from seaiceextentforecasting_amd import GPR
    for call in (lambda gp: gp.nlml_ard(TH[0]), lambda gp: gp.loo_ard(TH[0]), lambda gp: gp.cv_ard(TH[0], BLOCK), lambda gp: gp.hindcast_ard(TH[0]),
                 lambda gp: gp.cv_objective(TH2[0], BLOCK), lambda gp: gp.hindcast_objective(TH2[0])):
        gp = _single(fitted=False)
        gp._ride = np.zeros((2, D))
        call(gp)
        assert [c[0] for c in gp._lib.calls[1:]] == ["sigp_fit", "sigp_predict_ride"]
        assert gp.ell_.shape == (D,) and gp._ride_mean.shape == (2,) and gp._ride_var.shape == (2,) and gp._fitted and gp._ard
    gp = _single()
    gp.loo_ard(TH[0])
    assert np.array_equal(gp.ell_, GPR._exp(TH[0, :-1])) and gp.sn_tilde_ == GPR._exp(TH[0, -1:])[0] and gp.nlml_ == 0.0
    gp = _single()
    gp.cv_objective(TH2[0], BLOCK)
    assert np.array_equal(gp.ell_, GPR._exp(np.full(D, TH2[0, 0]))) and gp.sn_tilde_ == GPR._exp(TH2[0, 1:])[0]


def test_common_scale_objectives_sum_the_length_scale_components():
    """``cv_objective`` / ``hindcast_objective``: the ARD sibling at (log l x d, log sn~), d/dlog l = sum_k d/dlog l_k in NumPy's order"""
    g = np.array([0.1, 0.7, -0.3, 2.5])
    seen = []

    def stub(theta, *a, **kw):
        seen.append((np.array(theta), a, kw))
        return 1.5, g

    gp = _single()
    gp.cv_ard = gp.hindcast_ard = stub
    v, g2 = gp.cv_objective(TH2[0], BLOCK, gap=GAP, criterion="cv_sse", sigma_f="fixed")
    assert v == 1.5 and np.array_equal(g2, [np.sum(g[:-1]), g[-1]]) and g2.dtype == np.float64
    assert np.array_equal(seen[0][0], [0.25, 0.25, 0.25, -2.0]) and _bound("cv_ard", *seen[0][1:]) == _bound("cv_ard", (BLOCK,), dict(gap=GAP, criterion="cv_sse", sigma_f="fixed"))
    v, g2 = gp.hindcast_objective(TH2[0], LEAD, MT, "hindcast_sse", "fixed")
    assert v == 1.5 and np.array_equal(g2, [np.sum(g[:-1]), g[-1]])
    assert np.array_equal(seen[1][0], [0.25, 0.25, 0.25, -2.0]) and _bound("hindcast_ard", *seen[1][1:]) == _bound("hindcast_ard", (), dict(lead=LEAD, min_train=MT, criterion="hindcast_sse", sigma_f="fixed"))


def test_batch_objectives_mask_overflow_and_fill_inf():
    """theta [F, 2] with an overflowing row: that member rides at harmless parameters and comes back inf, for all three families"""
    th = np.array([[0.5, -2.0], [800.0, -1.0], [-0.25, -3.0], [0.0, np.inf]])
    gp = _batch()
    v, g = gp.cv_objective_batch(th, BLOCK, group=GROUP)
    assert np.array_equal(v, [0.0, np.inf, 0.0, np.inf]) and np.array_equal(g, [[0.0, 0.0], [np.inf] * 2, [0.0, 0.0], [np.inf] * 2])
    gp = _batch()
    v, g = gp.hindcast_objective_batch(th, group=GROUP)
    assert np.array_equal(v, [0.0, np.inf, 0.0, np.inf]) and np.array_equal(g, [[0.0, 0.0], [np.inf] * 2, [0.0, 0.0], [np.inf] * 2])
    # the leave-one-out one is reached through optimize_batch(criterion='loo_*'): loo_batch sees exp(theta), 1.0 where it overflows
    seen = {}

    def loo_batch(ell, sn, **kw):
        seen.update(ell=np.array(ell), sn=np.array(sn), kw=kw)
        return dict(nlpd=np.array([1.0, 2.0, np.nan, 4.0]), sse=np.zeros(4), nlpd_grad=np.arange(8.0).reshape(4, 2), sse_grad=np.zeros((4, 2)))

    gp = _batch()
    gp.upload_batch, gp.loo_batch = (lambda *a, **kw: None), loo_batch
    r = gp.optimize_batch(np.zeros((2, N, D)), np.zeros((2, N)), th, criterion="loo_nlpd", sigma_f="fixed", group=GROUP, maxiter=0)
    assert np.array_equal(seen["ell"], [np.exp(0.5), 1.0, np.exp(-0.25), 1.0]) and np.array_equal(seen["sn"], [np.exp(-2.0), 1.0, np.exp(-3.0), 1.0])
    assert seen["kw"] == dict(sigma_f="fixed", group=GROUP, predictions=False, grad=True)
    assert np.array_equal(r["fun"], [1.0, np.inf, np.inf, np.inf]) and np.array_equal(r["jac"], [[0.0, 1.0], [np.inf] * 2, [np.inf] * 2, [np.inf] * 2])


class Stop(Exception):
    pass


def _first_theta(method, theta0, B=2, stub=None, **kw):
    """the starts as they reach the objective named ``stub`` (replaced on the instance) in the first round of a lockstep optimiser"""
    seen = {}

    def objective(theta, *a, **k):
        seen.update(theta=np.array(theta), a=a, kw=k)
        raise Stop()

    gp = _batch(staged=False)
    gp.upload_batch = lambda *a, **k: seen.update(upload=k)
    setattr(gp, stub, objective)
    with pytest.raises(Stop):
        getattr(gp, method)(np.zeros((B, N, D)), np.zeros((B, N)), theta0, **kw)
    assert seen["upload"] == dict(group=kw.get("group", 8), concurrency=1)
    return seen


T2, TD = np.array([0.5, -2.0]), np.array([0.1, 0.2, 0.3, -2.0])
T62 = np.arange(12.0).reshape(6, 2)
T6D = np.arange(24.0).reshape(6, 4)
WIDE = lambda t: np.concatenate([np.repeat(t[:, :1], D, axis=1), t[:, 1:]], axis=1)


@pytest.mark.parametrize("method, stub, kw, passed", [
    ("optimize_batch", "nlml_ard_batch", dict(ard=True, group=GROUP), ((), dict(grad="exact", group=GROUP))),
    ("optimize_ard_batch", "loo_ard_batch", dict(criterion="loo_sse", sigma_f="fixed", group=GROUP), ((), dict(criterion="loo_sse", sigma_f="fixed", grad="exact", group=GROUP))),
    ("optimize_cv_batch", "cv_ard_batch", dict(block=BLOCK, gap=GAP, group=GROUP),
     ((BLOCK,), dict(gap=GAP, criterion="cv_nlpd", sigma_f="refit", grad="exact", group=GROUP))),
    ("optimize_hindcast_batch", "hindcast_ard_batch", dict(lead=LEAD, group=GROUP),
     ((), dict(lead=LEAD, min_train=D + 1, criterion="hindcast_nlpd", sigma_f="refit", group=GROUP))),
])
def test_ard_starts_of_the_lockstep_optimisers(method, stub, kw, passed):
    """theta0 [2], [d + 1], [B, 2], [S B, 2], [S B, d + 1], [1, d + 1] -> the starts [F, d + 1], and the arguments the objective is called with"""
    for theta0, want in ((T2, np.tile(WIDE(T2[None]), (2, 1))), (TD, np.tile(TD, (2, 1))), (T62[:2], WIDE(T62[:2])), (T62, WIDE(T62)), (T6D, T6D), (TD[None], np.tile(TD, (2, 1)))):
        seen = _first_theta(method, theta0, stub=stub, **kw)
        assert np.array_equal(seen["theta"], want), (theta0, seen["theta"])
        assert _bound(stub, seen["a"], seen["kw"]) == _bound(stub, *passed)
    for bad0 in (np.zeros(3), np.zeros((2, 5))):
        with pytest.raises(ValueError, match="theta0 must hold d \\+ 1 = 4 entries per start"):
            _first_theta(method, bad0, stub=stub, **kw)


@pytest.mark.parametrize("method, stub, kw, passed", [
    ("optimize_batch", "nlml_batch", dict(group=GROUP), ((), dict(grad="exact", group=GROUP))),
    ("optimize_cv_batch", "cv_objective_batch", dict(block=BLOCK, gap=GAP, ard=False, group=GROUP), ((BLOCK,), dict(gap=GAP, criterion="cv_nlpd", sigma_f="refit", group=GROUP))),
    ("optimize_hindcast_batch", "hindcast_objective_batch", dict(lead=LEAD, ard=False, group=GROUP),
     ((), dict(lead=LEAD, min_train=D + 1, criterion="hindcast_nlpd", sigma_f="refit", group=GROUP))),
])
def test_common_scale_starts_of_the_lockstep_optimisers(method, stub, kw, passed):
    """theta0 [2], [B, 2], [S B, 2] -> the starts [F, 2]; what is neither is refused by each site in its own way"""
    for theta0, want in ((T2, np.tile(T2, (2, 1))), (T62[:2], T62[:2]), (T62, T62)):
        seen = _first_theta(method, theta0, stub=stub, **kw)
        assert np.array_equal(seen["theta"], want), (theta0, seen["theta"])
        assert _bound(stub, seen["a"], seen["kw"]) == _bound(stub, *passed)
    for bad0 in (np.zeros(4), np.zeros((2, 3))):
        with pytest.raises(ValueError, match="broadcast" if method == "optimize_batch" else "theta0 must hold 2 entries per start"):
            _first_theta(method, bad0, stub=stub, **kw)


def _quadratic(p, centre):
    """(objective stub, the thetas it saw): a convex quadratic with its minimum at ``centre``"""
    seen = []

    def f(theta, *a, **kw):
        theta = np.asarray(theta, dtype=np.float64)
        seen.append((theta.copy(), a, kw))
        assert theta.shape == (p,)
        return np.float64(0.5 * np.sum((theta - centre) ** 2)), theta - centre
    return f, seen


def _optimised(stubs, p, run, **handle):
    """run a single-fit optimiser on a handle whose objective methods ``stubs`` are one quadratic; returns (result, thetas seen, refit's arguments)"""
    gp = _single(**handle)
    centre = np.linspace(-0.5, 0.5, p)
    f, seen = _quadratic(p, centre)
    refits = []
    for s in stubs:
        setattr(gp, s, f)
    gp.refit = lambda ell, sn: refits.append((ell, sn))
    res = run(gp)
    assert np.allclose(res.x, centre, atol=1e-5) and len(refits) == 1
    return res, seen, refits[0]


@pytest.mark.parametrize("grad", ["exact", None])
def test_optimize_ard_minimises_each_family_and_refits_by_the_c_exp(grad):
    from seaiceextentforecasting_amd import GPR
    cases = [("nlml", "nlml_ard", (), dict(grad=grad)), ("loo_sse", "loo_ard", (), dict(criterion="loo_sse", sigma_f="fixed", grad=grad)),
             ("cv_sse", "cv_ard", (BLOCK,), dict(gap=GAP, criterion="cv_sse", sigma_f="fixed", grad=grad)),
             ("hindcast_sse", "hindcast_ard", (), dict(lead=LEAD, min_train=D + 1, criterion="hindcast_sse", sigma_f="fixed", grad=grad))]
    for criterion, stub, a, kw in cases:
        for theta0 in (T2, TD):
            res, seen, (ell, sn) = _optimised([stub], D + 1, lambda gp: gp.optimize_ard(theta0, criterion=criterion, sigma_f="fixed", grad=grad, block=BLOCK, gap=GAP, lead=LEAD))
            assert np.array_equal(seen[0][0], WIDE(theta0[None])[0] if len(theta0) == 2 else theta0) and _bound(stub, *seen[0][1:]) == _bound(stub, a, kw)
            assert np.array_equal(ell, GPR._exp(res.x[:-1])) and isinstance(sn, float) and sn == GPR._exp(res.x[-1:])[0]
    for theta0 in (T2, TD):       # optimize(ard=True) is optimize_ard(criterion='nlml')
        res, seen, (ell, sn) = _optimised(["nlml_ard"], D + 1, lambda gp: gp.optimize(theta0, grad=grad, ard=True))
        assert np.array_equal(seen[0][0], WIDE(theta0[None])[0] if len(theta0) == 2 else theta0) and _bound("nlml_ard", *seen[0][1:]) == _bound("nlml_ard", (), dict(grad=grad))
        assert np.array_equal(ell, GPR._exp(res.x[:-1])) and isinstance(sn, float) and sn == GPR._exp(res.x[-1:])[0]
    for run in (lambda gp: gp.optimize_ard(np.zeros(3)), lambda gp: gp.optimize(np.zeros(3), ard=True)):
        with pytest.raises(ValueError, match="theta0 must hold d \\+ 1 = 4 entries, or 2"):
            run(_single())


@pytest.mark.parametrize("grad", ["exact", None])
def test_optimize_minimises_each_family_over_two_parameters_and_refits_by_numpys_exp(grad):
    # criterion -> the objective reached with grad='exact' / with grad=None, and how it is called
    both = dict(criterion="cv_sse", sigma_f="fixed")
    cases = [("nlml", "nlml", 2, (), dict(grad=grad)), ("loo_sse", "loo_objective", 2, ("loo_sse", "fixed"), {}),
             ("cv_sse", "cv_objective" if grad else "cv_ard", 2 if grad else D + 1, (BLOCK,), dict(both, gap=GAP, **({} if grad else dict(grad=None)))),
             ("hindcast_sse", "hindcast_objective" if grad else "hindcast_ard", 2 if grad else D + 1, (),
              dict(lead=LEAD, min_train=D + 1, criterion="hindcast_sse", sigma_f="fixed", **({} if grad else dict(grad=None))))]
    for criterion, stub, p, a, kw in cases:
        gp = _single()
        seen, refits = [], []

        def f(theta, *a_, **kw_):
            theta = np.asarray(theta, dtype=np.float64)
            seen.append((theta.copy(), a_, kw_))
            assert theta.shape == (p,)
            c = np.array([0.3, -0.4])
            t2 = theta[[0, -1]]
            return np.float64(0.5 * np.sum((t2 - c) ** 2)), (t2 - c if p == 2 else np.concatenate([np.full(D, (t2[0] - c[0]) / D), t2[1:] - c[1:]]))

        setattr(gp, stub, f)
        gp.refit = lambda ell, sn: refits.append((ell, sn))
        res = gp.optimize(T2, grad=grad, criterion=criterion, sigma_f="fixed", block=BLOCK, gap=GAP, lead=LEAD)
        assert np.allclose(res.x, [0.3, -0.4], atol=1e-5) and res.x.shape == (2,)
        assert np.array_equal(seen[0][0], T2 if p == 2 else WIDE(T2[None])[0]) and _bound(stub, *seen[0][1:]) == _bound(stub, a, kw)
        assert refits == [(float(np.exp(res.x[0])), float(np.exp(res.x[1])))] and all(isinstance(v, float) for v in refits[0])


class FakeSmall:
    """stands for ``SmallBatch`` behind ``gp._small``: records what is queued; fits at l = 3 overflow, as scipy's expm may"""
    def __init__(self):
        self.log = []
        self.fits = []

    def clear_fits(self):
        self.log.append("clear")
        self.fits = []

    def add_fit(self, ds, ell, sn, expm="eigh"):
        if 2.5 < ell < 3.5:
            raise FloatingPointError("expm(l M) overflowed")
        self.fits.append((ds, float(ell), float(sn), expm))
        return len(self.fits) - 1

    def run(self, **kw):
        self.log.append(("run", kw))
        k = len(self.fits)
        r = dict(nlml=10.0 + np.arange(k), grad_ref=np.full((k, 2), 1.0), grad_exact=np.full((k, 2), 2.0))
        for fam in ("loo", "hindcast"):
            r.update({fam + "_nlpd": 20.0 + np.arange(k), fam + "_sse": np.where(np.arange(k) == 1, np.inf, 30.0), fam + "_grad": np.full((k, 2), 3.0)})
        return r


def _small_handle():
    gp = _single("netdiffusion", data=False)
    gp._small, gp._small_ids = FakeSmall(), [7, 8, 9]
    return gp


SMALL_TH = np.log([[1.0, 0.1], [3.0, 0.2], [2.0, 0.3], [4.0, 0.4]])
SMALL_TH[3, 0] = 800.0          # exp overflows: never queued


def test_one_workgroup_batches_stage_only_what_can_be_evaluated():
    """``nlml_batch`` (reference kernel) and ``small_score_batch``: an overflowing exp(theta) is never queued, a fit whose expm overflows is
    dropped, the rest run in one launch and their results are scattered into inf-filled arrays"""
    ell, sn = np.exp(SMALL_TH[:3, 0]), np.exp(SMALL_TH[:3, 1])
    for grad, key, fill in (("exact", "grad_exact", 2.0), ("ref", "grad_ref", 1.0), (None, None, None)):
        gp = _small_handle()
        v, g = gp.nlml_batch(SMALL_TH, first=1, grad=grad, expm="pade")
        assert gp._small.log == ["clear", ("run", dict(grad=grad is not None))]
        assert gp._small.fits == [(8, ell[0], sn[0], "pade"), (7, ell[2], sn[2], "pade")]          # data set (first + i) % B
        assert np.array_equal(v, [10.0, np.inf, 11.0, np.inf])
        assert g is None if grad is None else np.array_equal(g, [[fill] * 2, [np.inf] * 2, [fill] * 2, [np.inf] * 2])
    gp = _small_handle()
    gp.nlml_batch(SMALL_TH, sets=[2, 1, 0, 1])
    assert gp._small.fits == [(9, ell[0], sn[0], "eigh"), (7, ell[2], sn[2], "eigh")]
    gp = _small_handle()
    v, g = gp.nlml_batch(np.array([[800.0, 0.0]]))
    assert gp._small.log == ["clear"] and np.array_equal(v, [np.inf]) and np.array_equal(g, [[np.inf, np.inf]])      # nothing to run: no launch
    for criterion, run_kw in (("loo_nlpd", dict(loo="fixed", score_grad="nlpd")), ("hindcast_sse", dict(hindcast=dict(lead=LEAD, min_train=MT, sigma_f="fixed"), score_grad="sse"))):
        gp = _small_handle()
        v, g = gp.small_score_batch(SMALL_TH, criterion=criterion, lead=LEAD, min_train=MT, sigma_f="fixed", first=1, expm="pade")
        assert gp._small.log == ["clear", ("run", run_kw)]
        assert gp._small.fits == [(8, ell[0], sn[0], "pade"), (7, ell[2], sn[2], "pade")]
        if criterion == "loo_nlpd":
            assert np.array_equal(v, [20.0, np.inf, 21.0, np.inf]) and np.array_equal(g, [[3.0] * 2, [np.inf] * 2, [3.0] * 2, [np.inf] * 2])
        else:               # the second fit that ran came back inf: its gradient is inf too
            assert np.array_equal(v, [30.0, np.inf, np.inf, np.inf]) and np.array_equal(g, [[3.0] * 2, [np.inf] * 2, [np.inf] * 2, [np.inf] * 2])
    assert not gp._fitted


def test_small_batch_run_checks_the_hindcast_window_with_its_own_lead_cap():
    from seaiceextentforecasting_amd import SmallBatch
    gp = _single("netdiffusion", data=False)
    sb = SmallBatch(gp)
    sb.add_dataset(np.zeros((6, 2)), np.zeros(6), None, np.zeros((2, 2)))
    for hc, frag in ((dict(lead=0), "1 <= lead <= 32"), (dict(lead=33), "1 <= lead <= 32"), (dict(min_train=0), "min_train >= 1"), (dict(sigma_f="both"), "sigma_f must be"),
                     (dict(sigma_f="both", lead=0), "sigma_f must be"), (dict(lead=0, min_train=0), "1 <= lead <= 32"), (dict(lead=3, min_train=4), "a data set of 6 rows has no scored row"),
                     (dict(lead=2, horizon=1), "hindcast must be dict"), (dict(lead=33, min_train=9), "1 <= lead <= 32")):
        with pytest.raises(ValueError, match=frag):
            sb.run(hindcast=hc)
    assert gp._lib.calls == []


# ---- refusals: the type, a fragment of the message, and which one wins when two arguments are bad --------------------------------------
ENGINE = "per-feature length scales: RBF / Matern kernels on the fp64 engine only"
SIGMA = "sigma_f must be 'refit' or 'fixed'"
GRAD = "grad must be None or 'exact'"
NODATA = "no data staged; call fit\\(\\) or set_data\\(\\) first"
STAGE = "stage the data sets with upload_batch\\(\\) first"
X2, Y2 = np.zeros((2, N, D)), np.zeros((2, N))
nodata = lambda **kw: _single(data=False, **kw)
unstaged = lambda **kw: _batch(staged=False, **kw)
nd = lambda make: (lambda: make(kernel="netdiffusion"))
f32 = lambda make: (lambda: make(dtype="f32"))

REFUSALS = [
    # (handle, call, exception type, fragment)
    # -- single fits on the factor
    (_single, lambda gp: gp.loo("both"), ValueError, SIGMA),
    (lambda: _single(fitted=False), lambda gp: gp.loo(), RuntimeError, "loo: call fit\\(\\) first"),
    (lambda: _single(fitted=False), lambda gp: gp.loo("both"), ValueError, SIGMA),
    (lambda: _single(fitted=False), lambda gp: gp.hindcast(), RuntimeError, "hindcast: call fit\\(\\) first"),
    (lambda: _single(fitted=False), lambda gp: gp.hindcast(sigma_f="both"), ValueError, SIGMA),
    (lambda: _single(fitted=False), lambda gp: gp.hindcast(lead=0), RuntimeError, "hindcast: call fit\\(\\) first"),
    (_single, lambda gp: gp.hindcast(lead=0), ValueError, "hindcast: 1 <= lead <= 128 required"),
    (_single, lambda gp: gp.hindcast(lead=129, sigma_f="both"), ValueError, SIGMA),
    (_single, lambda gp: gp.hindcast(min_train=0), ValueError, "hindcast: min_train >= 1 required"),
    (_single, lambda gp: gp.hindcast(lead=36, min_train=5), ValueError, "hindcast: no row is scored \\(min_train \\+ lead - 1 = 40 > n - 1 = 39\\)"),
    (_single, lambda gp: gp.cv(BLOCK, sigma_f="both"), ValueError, SIGMA),
    (_single, lambda gp: gp.cv(0, sigma_f="both"), ValueError, SIGMA),
    (_single, lambda gp: gp.cv(2.5), ValueError, "block >= 1 and gap >= 0 \\(integers\\) required"),
    (_single, lambda gp: gp.cv(100, 20), ValueError, "the window block \\+ 2 gap = 140 exceeds 128 rows"),
    (_single, lambda gp: gp.cv(40), ValueError, "every fold must leave a training row \\(n = 40, block = 40, gap = 0\\)"),
    (f32(_single), lambda gp: gp.cv(BLOCK), ValueError, "cv: fp64 engine only"),
    (f32(_single), lambda gp: gp.cv(129), ValueError, "exceeds 128 rows"),                                  # the folds before the engine
    (lambda: _single(fitted=False), lambda gp: gp.cv(BLOCK), RuntimeError, "cv: call fit\\(\\) first"),
    (lambda: _single(fitted=False, dtype="f32"), lambda gp: gp.cv(BLOCK), ValueError, "cv: fp64 engine only"),
    # -- lockstep scores
    (_batch, lambda gp: gp.loo_batch(ELL, SN, sigma_f="both"), ValueError, SIGMA),
    (nd(_batch), lambda gp: gp.loo_batch(ELL, SN, sigma_f="both"), ValueError, SIGMA),
    (nd(_batch), lambda gp: gp.loo_batch(ELL, SN), ValueError, "loo_batch covers the RBF / Matern kernels; the reference kernel's batch is SmallBatch.run\\(loo=...\\)"),
    (_batch, lambda gp: gp.loo_batch(ELL, SN[:2]), ValueError, "ell and sn_tilde must have the same length"),
    (unstaged, lambda gp: gp.loo_batch(ELL, SN), RuntimeError, "loo_batch: " + STAGE),
    (unstaged, lambda gp: gp.loo_batch(ELL, SN[:2]), ValueError, "same length"),
    (nd(_batch), lambda gp: gp.cv_batch(ELL, SN, BLOCK), ValueError, "cv_batch covers the RBF / Matern kernels; the reference kernel's batch is SmallBatch.run\\(cv=...\\)"),
    (nd(_batch), lambda gp: gp.cv_batch(ELL, SN, 129), ValueError, "exceeds 128 rows"),
    (unstaged, lambda gp: gp.cv_batch(ELL, SN, BLOCK), RuntimeError, "cv_batch: " + STAGE),
    (_batch, lambda gp: gp.cv_batch(ELL, SN, 40), ValueError, "every fold must leave a training row"),
    (nd(_batch), lambda gp: gp.hindcast_batch(ELL, SN, lead=0), ValueError, "hindcast_batch covers the RBF / Matern kernels"),      # here the kernel comes first
    (_batch, lambda gp: gp.hindcast_batch(ELL, SN, lead=0, sigma_f="both"), ValueError, SIGMA),
    (_batch, lambda gp: gp.hindcast_batch(ELL, SN, lead=37), ValueError, "no row is scored"),
    (unstaged, lambda gp: gp.hindcast_batch(ELL, SN), RuntimeError, "hindcast_batch: " + STAGE),
    # -- grids
    (_batch, lambda gp: gp.loo_grid(*_xy(), sigma_f="both", **GRID), ValueError, SIGMA),
    (_batch, lambda gp: gp.cv_grid(*_xy(), block=40, **GRID), ValueError, "every fold must leave a training row"),
    (nd(_batch), lambda gp: gp.cv_grid(*_xy(), block=33, **GRID), ValueError, "exceeds 32 rows"),           # the one-workgroup kernel's window
    (_batch, lambda gp: gp.hindcast_grid(*_xy(), lead=37, **GRID), ValueError, "no row is scored"),
    (_batch, lambda gp: gp.hindcast_grid(*_xy(), lead=129, sigma_f="both", **GRID), ValueError, SIGMA),
    # -- per-feature objectives of one fit
    (_single, lambda gp: gp.nlml_ard(TH[0], grad="ref"), ValueError, GRAD),
    (nodata, lambda gp: gp.nlml_ard(TH[0], grad="ref"), RuntimeError, "nlml_ard: " + NODATA),            # here missing data comes first
    (nd(_single), lambda gp: gp.nlml_ard(TH[0]), ValueError, ENGINE),
    (_single, lambda gp: gp.nlml_ard(TH[0, :3]), ValueError, "theta must hold d \\+ 1 = 4 entries \\(log l_1 .. log l_d, log sn~\\), got 3"),
    (f32(_single), lambda gp: gp.nlml_ard(TH[0, :3]), ValueError, ENGINE),
    (_single, lambda gp: gp.loo_ard(TH[0], criterion="cv_nlpd", sigma_f="both"), ValueError, "criterion must be 'loo_nlpd' or 'loo_sse'"),
    (_single, lambda gp: gp.loo_ard(TH[0], sigma_f="both", grad="ref"), ValueError, SIGMA),
    (nodata, lambda gp: gp.loo_ard(TH[0], grad="ref"), ValueError, GRAD),                                  # grad before missing data
    (nodata, lambda gp: gp.loo_ard(TH[0]), RuntimeError, "loo_ard: " + NODATA),
    (nd(nodata), lambda gp: gp.loo_ard(TH[0]), RuntimeError, "loo_ard: " + NODATA),
    (f32(_single), lambda gp: gp.loo_ard(TH[0]), ValueError, ENGINE),
    (_single, lambda gp: gp.loo_ard(TH[0, :3]), ValueError, "theta must hold d \\+ 1 = 4"),
    (_single, lambda gp: gp.cv_ard(TH[0], BLOCK, criterion="loo_nlpd", sigma_f="both"), ValueError, "criterion must be 'cv_nlpd' or 'cv_sse'"),
    (_single, lambda gp: gp.cv_ard(TH[0], BLOCK, sigma_f="both", grad="ref"), ValueError, GRAD),
    (nodata, lambda gp: gp.cv_ard(TH[0], BLOCK, grad="ref"), ValueError, GRAD),
    (nodata, lambda gp: gp.cv_ard(TH[0], 129), ValueError, "exceeds 128 rows"),
    (nodata, lambda gp: gp.cv_ard(TH[0], BLOCK), RuntimeError, "cv_ard: " + NODATA),
    (nd(_single), lambda gp: gp.cv_ard(TH[0], 40), ValueError, "every fold must leave a training row"),    # the folds before the engine
    (nd(_single), lambda gp: gp.cv_ard(TH[0], BLOCK), ValueError, ENGINE),
    (_single, lambda gp: gp.hindcast_ard(TH[0], criterion="cv_nlpd", sigma_f="both"), ValueError, "criterion must be 'hindcast_nlpd' or 'hindcast_sse'"),
    (_single, lambda gp: gp.hindcast_ard(TH[0], lead=0, grad="ref"), ValueError, GRAD),
    (nodata, lambda gp: gp.hindcast_ard(TH[0], lead=0), ValueError, "1 <= lead <= 128"),
    (nodata, lambda gp: gp.hindcast_ard(TH[0]), RuntimeError, "hindcast_ard: " + NODATA),
    (nd(_single), lambda gp: gp.hindcast_ard(TH[0], lead=37), ValueError, "no row is scored"),            # the window before the engine
    (f32(_single), lambda gp: gp.hindcast_ard(TH[0]), ValueError, ENGINE),
    (_single, lambda gp: gp.hindcast_ard(TH[0, :3]), ValueError, "theta must hold d \\+ 1 = 4"),
    # -- common-scale objectives of one fit
    (nd(_single), lambda gp: gp.cv_objective(TH2[0], 129), ValueError, "cv_objective covers the RBF / Matern kernels \\(the reference kernel's leave-block-out scores have no gradient: cv_grid\\)"),
    (_single, lambda gp: gp.cv_objective(TH2[0], 129, criterion="nlml"), ValueError, "criterion must be 'cv_nlpd' or 'cv_sse'"),
    (nodata, lambda gp: gp.cv_objective(TH2[0], BLOCK), RuntimeError, "cv_ard: " + NODATA),
    (f32(_single), lambda gp: gp.cv_objective(TH2[0], BLOCK), ValueError, ENGINE),
    (nd(_single), lambda gp: gp.hindcast_objective(TH2[0], lead=0), ValueError, "hindcast_objective covers the RBF / Matern kernels \\(the reference kernel's hindcast scores have no gradient\\)"),
    (_single, lambda gp: gp.hindcast_objective(TH2[0], lead=0, criterion="nlml"), ValueError, "criterion must be 'hindcast_nlpd' or 'hindcast_sse'"),
    (nodata, lambda gp: gp.hindcast_objective(TH2[0]), RuntimeError, "hindcast_ard: " + NODATA),
    (_single, lambda gp: gp.loo_objective(TH2[0], "cv_nlpd", "both"), ValueError, "criterion must be 'loo_nlpd' or 'loo_sse'"),
    (nodata, lambda gp: gp.loo_objective(TH2[0], sigma_f="both"), ValueError, SIGMA),
    (nodata, lambda gp: gp.loo_objective(TH2[0]), RuntimeError, "loo_objective: " + NODATA),
    # -- per-feature objectives of lockstep groups
    (unstaged, lambda gp: gp.nlml_ard_batch(TH, grad="ref"), ValueError, GRAD),
    (nd(unstaged), lambda gp: gp.nlml_ard_batch(TH), ValueError, ENGINE),
    (unstaged, lambda gp: gp.nlml_ard_batch(TH), RuntimeError, "nlml_ard_batch: " + STAGE),
    (_batch, lambda gp: gp.nlml_ard_batch(TH[:, :3]), ValueError, "theta must be \\[F, d \\+ 1\\] = \\[F, 4\\] \\(log l_1 .. log l_d, log sn~\\), got \\(3, 3\\)"),
    (_batch, lambda gp: gp.loo_ard_batch(TH, criterion="cv_nlpd", sigma_f="both"), ValueError, "criterion must be 'loo_nlpd' or 'loo_sse' \\(the leave-block-out scores 'cv_nlpd' / 'cv_sse': cv_ard_batch\\)"),
    (_batch, lambda gp: gp.loo_ard_batch(TH, sigma_f="both", grad="ref"), ValueError, SIGMA),
    (nd(unstaged), lambda gp: gp.loo_ard_batch(TH, grad="ref"), ValueError, GRAD),
    (nd(unstaged), lambda gp: gp.loo_ard_batch(TH), ValueError, ENGINE),                                   # the engine before the staged data
    (unstaged, lambda gp: gp.loo_ard_batch(TH), RuntimeError, "loo_ard_batch: " + STAGE),
    (_batch, lambda gp: gp.loo_ard_batch(TH[:, :3]), ValueError, "theta must be \\[F, d \\+ 1\\] = \\[F, 4\\]"),
    (_batch, lambda gp: gp.cv_ard_batch(TH, BLOCK, criterion="loo_nlpd", sigma_f="both"), ValueError, "criterion must be 'cv_nlpd' or 'cv_sse' \\(the leave-one-out scores: loo_ard_batch\\)"),
    (_batch, lambda gp: gp.cv_ard_batch(TH, 129, sigma_f="both", grad="ref"), ValueError, SIGMA),
    (_batch, lambda gp: gp.cv_ard_batch(TH, 129, grad="ref"), ValueError, GRAD),
    (nd(_batch), lambda gp: gp.cv_ard_batch(TH, 40), ValueError, "every fold must leave a training row"),  # the folds before the engine
    (nd(unstaged), lambda gp: gp.cv_ard_batch(TH, BLOCK), ValueError, ENGINE),
    (unstaged, lambda gp: gp.cv_ard_batch(TH, BLOCK), RuntimeError, "cv_ard_batch: " + STAGE),
    (_batch, lambda gp: gp.hindcast_ard_batch(TH, criterion="cv_nlpd", grad="ref"),
     ValueError, "criterion must be 'hindcast_nlpd' or 'hindcast_sse' \\(the leave-one-out scores: loo_ard_batch, the leave-block-out scores: cv_ard_batch\\)"),
    (_batch, lambda gp: gp.hindcast_ard_batch(TH, sigma_f="both", grad="ref"), ValueError, GRAD),        # here grad comes before sigma_f
    (_batch, lambda gp: gp.hindcast_ard_batch(TH, lead=0, sigma_f="both"), ValueError, SIGMA),
    (f32(_batch), lambda gp: gp.hindcast_ard_batch(TH, lead=37), ValueError, "no row is scored"),          # the window before the engine
    (f32(unstaged), lambda gp: gp.hindcast_ard_batch(TH), ValueError, ENGINE),
    (unstaged, lambda gp: gp.hindcast_ard_batch(TH), RuntimeError, "hindcast_ard_batch: " + STAGE),
    (_batch, lambda gp: gp.hindcast_ard_batch(TH[:, :3]), ValueError, "theta must be \\[F, d \\+ 1\\] = \\[F, 4\\]"),
    # -- common-scale objectives of lockstep groups
    (_batch, lambda gp: gp.cv_objective_batch(TH2, 129, criterion="loo_nlpd"), ValueError, "criterion must be 'cv_nlpd' or 'cv_sse'"),
    (nd(_batch), lambda gp: gp.cv_objective_batch(TH2, 129, sigma_f="both"), ValueError, SIGMA),
    (nd(_batch), lambda gp: gp.cv_objective_batch(TH2, 129), ValueError, "exceeds 128 rows"),
    (nd(unstaged), lambda gp: gp.cv_objective_batch(TH2, BLOCK), ValueError, ENGINE),
    (unstaged, lambda gp: gp.cv_objective_batch(TH, BLOCK), RuntimeError, "cv_objective_batch: " + STAGE),
    (_batch, lambda gp: gp.cv_objective_batch(TH, BLOCK), ValueError, "theta must be \\[F, 2\\] = \\(log l, log sn~\\) per fit, got \\(3, 4\\)"),
    (_batch, lambda gp: gp.hindcast_objective_batch(TH2, lead=0, criterion="loo_nlpd"), ValueError, "criterion must be 'hindcast_nlpd' or 'hindcast_sse'"),
    (nd(_batch), lambda gp: gp.hindcast_objective_batch(TH2, lead=0), ValueError, "1 <= lead <= 128"),
    (nd(unstaged), lambda gp: gp.hindcast_objective_batch(TH2), ValueError, ENGINE),
    (unstaged, lambda gp: gp.hindcast_objective_batch(TH), RuntimeError, "hindcast_objective_batch: " + STAGE),
    (_batch, lambda gp: gp.hindcast_objective_batch(TH), ValueError, "theta must be \\[F, 2\\] = \\(log l, log sn~\\) per fit, got \\(3, 4\\)"),
    # -- optimisers of one fit
    (nodata, lambda gp: gp.optimize_ard(TD, criterion="mse", sigma_f="both"), ValueError, "criterion must be 'nlml', 'loo_nlpd', 'loo_sse', 'cv_nlpd', 'cv_sse', 'hindcast_nlpd' or 'hindcast_sse'"),
    (nodata, lambda gp: gp.optimize_ard(TD, sigma_f="both", grad="ref"), ValueError, SIGMA),
    (nodata, lambda gp: gp.optimize_ard(TD, grad="ref"), ValueError, "optimize_ard takes grad='exact' or None"),
    (nodata, lambda gp: gp.optimize_ard(TD), RuntimeError, "optimize_ard: " + NODATA),
    (nd(nodata), lambda gp: gp.optimize_ard(TD), RuntimeError, "optimize_ard: " + NODATA),
    (nd(nodata), lambda gp: gp.optimize_ard(TD, criterion="cv_nlpd"), ValueError, ENGINE),                 # a fold or window criterion: the engine before the data
    (nd(nodata), lambda gp: gp.optimize_ard(TD, criterion="cv_nlpd", block=129), ValueError, "exceeds 128 rows"),
    (nd(nodata), lambda gp: gp.optimize_ard(TD, criterion="hindcast_nlpd"), ValueError, ENGINE),
    (nd(nodata), lambda gp: gp.optimize_ard(TD, criterion="hindcast_nlpd", lead=0), ValueError, "1 <= lead <= 128"),
    (nd(_single), lambda gp: gp.optimize_ard(TD, criterion="hindcast_nlpd", lead=37), ValueError, "no row is scored"),
    (nodata, lambda gp: gp.optimize(T2, ard=True, criterion="loo_nlpd", grad="ref"), ValueError, "ard=True: criterion must be 'nlml' \\(optimize_ard minimises"),
    (nodata, lambda gp: gp.optimize(T2, ard=True, grad="ref"), ValueError, "ard=True takes grad='exact' or None"),
    (nodata, lambda gp: gp.optimize(T2, ard=True), RuntimeError, "optimize: " + NODATA),
    (nd(nodata), lambda gp: gp.optimize(T2, criterion="cv_nlpd", grad="ref"), ValueError, "a leave-block-out criterion takes grad='exact' or None"),
    (nd(nodata), lambda gp: gp.optimize(T2, criterion="cv_nlpd", block=129), ValueError, "criterion 'cv_nlpd' / 'cv_sse' covers the RBF / Matern kernels \\(the reference kernel: cv_grid\\)"),
    (f32(nodata), lambda gp: gp.optimize(T2, criterion="cv_nlpd", block=129), ValueError, "criterion 'cv_nlpd' / 'cv_sse': fp64 engine only"),
    (nodata, lambda gp: gp.optimize(T2, criterion="cv_nlpd", block=129), ValueError, "exceeds 128 rows"),
    (nodata, lambda gp: gp.optimize(T2, criterion="cv_nlpd"), RuntimeError, "optimize: " + NODATA),
    (nd(nodata), lambda gp: gp.optimize(T2, criterion="hindcast_nlpd", grad="ref"), ValueError, "a hindcast criterion takes grad='exact' or None"),
    (nd(nodata), lambda gp: gp.optimize(T2, criterion="hindcast_nlpd", lead=0), ValueError, "criterion 'hindcast_nlpd' / 'hindcast_sse' covers the RBF / Matern kernels \\(the reference kernel: hindcast after fit\\)"),
    (f32(nodata), lambda gp: gp.optimize(T2, criterion="hindcast_nlpd", lead=0), ValueError, "criterion 'hindcast_nlpd' / 'hindcast_sse': fp64 engine only"),
    (nodata, lambda gp: gp.optimize(T2, criterion="hindcast_nlpd", lead=0), ValueError, "1 <= lead <= 128"),
    (nodata, lambda gp: gp.optimize(T2, criterion="hindcast_nlpd"), RuntimeError, "optimize: " + NODATA),
    (nodata, lambda gp: gp.optimize(T2, criterion="mse", grad="ref"), ValueError, "criterion must be 'nlml', 'loo_nlpd', 'loo_sse', 'cv_nlpd', 'cv_sse', 'hindcast_nlpd' or 'hindcast_sse'"),
    (nodata, lambda gp: gp.optimize(T2, criterion="loo_nlpd", grad="ref"), ValueError, "a leave-one-out criterion takes grad='exact' or None"),
    # -- lockstep optimisers
    (nd(unstaged), lambda gp: gp.optimize_ard_batch(X2, Y2, TD, criterion="cv_nlpd", sigma_f="both"),
     ValueError, "criterion must be 'nlml', 'loo_nlpd' or 'loo_sse' \\(the leave-block-out scores 'cv_nlpd' / 'cv_sse': optimize_cv_batch\\)"),
    (nd(unstaged), lambda gp: gp.optimize_ard_batch(X2, Y2, TD, sigma_f="both"), ValueError, SIGMA),
    (nd(unstaged), lambda gp: gp.optimize_ard_batch(X2, Y2, np.zeros(3)), ValueError, ENGINE),
    (unstaged, lambda gp: gp.optimize_ard_batch(X2, Y2, np.zeros(3)), ValueError, "theta0 must hold d \\+ 1 = 4 entries per start"),
    (nd(unstaged), lambda gp: gp.optimize_cv_batch(X2, Y2, TD, 129, criterion="loo_nlpd", sigma_f="both"),
     ValueError, "criterion must be 'cv_nlpd' or 'cv_sse' \\(the leave-one-out scores and 'nlml': optimize_ard_batch\\)"),
    (nd(unstaged), lambda gp: gp.optimize_cv_batch(X2, Y2, TD, 129, sigma_f="both"), ValueError, SIGMA),
    (nd(unstaged), lambda gp: gp.optimize_cv_batch(X2, Y2, TD, 129), ValueError, ENGINE),                  # here the engine comes before the folds
    (unstaged, lambda gp: gp.optimize_cv_batch(X2, Y2, np.zeros(3), 129), ValueError, "exceeds 128 rows"),
    (nd(unstaged), lambda gp: gp.optimize_hindcast_batch(X2, Y2, TD, lead=0, criterion="loo_nlpd", sigma_f="both"),
     ValueError, "criterion must be 'hindcast_nlpd' or 'hindcast_sse' \\(the leave-block-out scores: optimize_cv_batch; the leave-one-out scores and 'nlml': optimize_ard_batch\\)"),
    (nd(unstaged), lambda gp: gp.optimize_hindcast_batch(X2, Y2, TD, lead=0, sigma_f="both"), ValueError, SIGMA),
    (nd(unstaged), lambda gp: gp.optimize_hindcast_batch(X2, Y2, TD, lead=0), ValueError, ENGINE),
    (unstaged, lambda gp: gp.optimize_hindcast_batch(X2, Y2, np.zeros(3), lead=0), ValueError, "1 <= lead <= 128"),
    (nd(unstaged), lambda gp: gp.optimize_batch(X2, Y2, T2, ard=True, criterion="loo_nlpd"), ValueError, "optimize_batch\\(ard=True\\): criterion must be 'nlml'"),
    (nd(unstaged), lambda gp: gp.optimize_batch(X2, Y2, T2, ard=True), ValueError, "optimize_batch\\(ard=True\\): per-feature length scales cover the RBF / Matern kernels"),
    (nd(unstaged), lambda gp: gp.optimize_batch(X2, Y2, T2, criterion="cv_nlpd"), ValueError, "criterion must be 'nlml', 'loo_nlpd' or 'loo_sse'"),
    (nd(unstaged), lambda gp: gp.optimize_batch(X2, Y2, T2, criterion="loo_nlpd"), ValueError, "optimize_batch: the leave-one-out criteria cover the RBF / Matern kernels"),
    (unstaged, lambda gp: gp.optimize_batch(X2, Y2, T2, method="newton"), ValueError, "method='newton' needs the one-workgroup-per-point kernel"),
    # -- the one-workgroup batches
    (nd(unstaged), lambda gp: gp.nlml_batch(TH), ValueError, "theta must be \\[F, 2\\]"),
    (nd(unstaged), lambda gp: gp.nlml_batch(TH2, grad="both"), ValueError, "grad must be None, 'ref' or 'exact'"),
    (nd(unstaged), lambda gp: gp.nlml_batch(TH2), RuntimeError, "nlml_batch: stage the data sets with upload_batch\\(X_list, y_list, Xs_list, M=M_list\\) first"),
    (unstaged, lambda gp: gp.nlml_batch(TH2, grad="ref", sets=[0, 0, 0]), ValueError, GRAD),
    (unstaged, lambda gp: gp.nlml_batch(TH2, sets=[0, 0, 0]), ValueError, "sets= is for the reference kernel's ragged data sets"),
    (unstaged, lambda gp: gp.small_score_batch(TH2, criterion="cv_nlpd"), ValueError, "small_score_batch runs the reference kernel \\(RBF / Matern: loo_ard_batch, hindcast_ard_batch\\)"),
    (nd(unstaged), lambda gp: gp.small_score_batch(TH2, criterion="cv_nlpd", sigma_f="both"),
     ValueError, "criterion must be 'loo_nlpd', 'loo_sse', 'hindcast_nlpd' or 'hindcast_sse' \\(block-CV gradients are not built for the reference kernel\\)"),
    (nd(unstaged), lambda gp: gp.small_score_batch(TH2, sigma_f="both"), ValueError, SIGMA),
    (nd(unstaged), lambda gp: gp.small_score_batch(TH), RuntimeError, "small_score_batch: stage the data sets with upload_batch\\(X_list, y_list, Xs_list, M=M_list\\) first"),
    (_small_handle, lambda gp: gp.small_score_batch(TH), ValueError, "theta must be \\[F, 2\\]"),
    (unstaged, lambda gp: gp.optimize_small_batch([X2[0]], [Y2[0]], T2, criterion="cv_nlpd"),
     ValueError, "optimize_small_batch runs the reference kernel \\(RBF / Matern: optimize_batch, optimize_ard_batch, optimize_hindcast_batch\\)"),
    (nd(unstaged), lambda gp: gp.optimize_small_batch([X2[0]], [Y2[0]], T2, criterion="cv_nlpd"), ValueError, "block-CV gradients are not built for the reference kernel"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_and_their_order(i):
    make, call, exc, fragment = REFUSALS[i]
    gp = make()
    with pytest.raises(exc, match=fragment) as e:
        call(gp)
    assert type(e.value) is exc
    assert gp._lib.calls == []          # refused before any device call
