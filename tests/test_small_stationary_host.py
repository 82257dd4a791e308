"""Host tier of the one-workgroup kernel's stationary flavours (tests/small_stationary_cases.py): the long-double references the GPU tier
(tests/test_hip_small_stationary.py) measures against are pinned here -- the closed-form gradient against central differences of the
long-double nlML, the covariance against the oracle's, the table's conditioning, the LDS layouts -- and the argument refusals of
``SmallStationaryBatch`` that need no device."""
import os
import subprocess
import types

import numpy as np
import pytest

import small_cases as SC
import small_stationary_cases as T
from oracle import gp_oracle as O

needs_ld = pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nlml_ld(case, log_ell, log_sn):
    """the profiled nlML in long double at scales exp(log_ell) [N] and sn~ = exp(log_sn), from the RAW rows (the division in long double: the
    function whose derivative the closed form is)"""
    X, y, _, _ = T.inputs(case)
    U = np.asarray(X, dtype=SC.LD) / np.exp(np.asarray(log_ell, dtype=SC.LD))
    _, sq = T.sq_parts(U, SC.LD)
    K = T.cov_h(case.kernel, sq)[0] + np.exp(SC.LD(log_sn)) * np.eye(case.n, dtype=SC.LD)
    return SC.core_from_matrix(K, y, 0.0, SC.HP, need_inverse=False)["nlml"]


FD_CASES = [c for c in T.TABLE if c.n in (15, 16, 17, 33) and c.N in (8, 9, 32, 33) and c.sn >= 1e-3]
FD_STEP, FD_TOL = 1e-6, 1e-7


def test_the_finite_difference_cases_cover_both_kernels_and_every_kind_of_scales():
    assert {c.kernel for c in FD_CASES} == set(T.KERNELS) and {c.kind for c in FD_CASES} == set(T.KINDS)


@needs_ld
@pytest.mark.parametrize("case", FD_CASES, ids=lambda c: "%s-%s-n%d-N%d" % (c.kernel, c.kind, c.n, c.N))
def test_the_closed_form_gradient_is_the_derivative_of_the_long_double_nlml(case):
    """central differences with step h = 1e-6 in long double, every direction.  FD_TOL: the differences carry the rounding of two nlML values,
    at most n cond(K~) eps_ld / (2 h) with cond <= (n + sn~) / sn~ <= 3.3e4 (sn~ >= 1e-3, n <= 33): 6e-8; the truncation h^2 |f'''| / 6 ~ 1e-11"""
    X, y, Xs, ell = T.inputs(case)
    lell = np.log(np.broadcast_to(np.asarray(ell, dtype=SC.LD), (case.N,)).astype(SC.LD))
    lsn = np.log(SC.LD(case.sn))
    # the closed form at the same long-double scaled features
    U = np.asarray(X, dtype=SC.LD) / np.exp(lell)
    D, sq = T.sq_parts(U, SC.LD)
    k, h = T.cov_h(case.kernel, sq)
    c = SC.core_from_matrix(k + np.exp(lsn) * np.eye(case.n, dtype=SC.LD), y, np.exp(lsn), SC.HP)
    g = T.gradient(c, h * D, np.exp(lsn), common=False)
    step = SC.LD(FD_STEP)
    fd = np.zeros(case.N + 1, dtype=SC.LD)
    for k_ in range(case.N):
        e = np.zeros(case.N, dtype=SC.LD); e[k_] = step
        fd[k_] = (_nlml_ld(case, lell + e, lsn) - _nlml_ld(case, lell - e, lsn)) / (2 * step)
    fd[case.N] = (_nlml_ld(case, lell, lsn + step) - _nlml_ld(case, lell, lsn - step)) / (2 * step)
    err = np.max(np.abs(g - fd) / np.maximum(1, np.abs(fd)))
    assert err < FD_TOL, (case, float(err))
    # one common scale: the sum of the components
    both = (_nlml_ld(case, lell + step, lsn) - _nlml_ld(case, lell - step, lsn)) / (2 * step)
    assert abs(T.gradient(c, h * D, np.exp(lsn), common=True)[0] - both) < FD_TOL * max(1, abs(both))
    if case.kind == "irrelevant":
        assert abs(g[case.N // 2]) < 1e-9 and np.max(np.abs(g[:case.N])) > 1e-3, "a feature at l = 1e6 has no say"


@pytest.mark.parametrize("kernel", T.KERNELS)
def test_the_covariance_is_the_oracles_on_pre_divided_features(kernel):
    for case in [c for c in T.TABLE if c.kernel == kernel and c.n in (2, 17, 33)]:
        X, y, Xs, ell = T.inputs(case)
        U = T.scaled(X, Xs, ell)
        K, ks, kss, _ = T.build(case, SC.F64)
        n = case.n
        ref = O.cov_unit(kernel, U[:n], U[:n], 1.0)
        assert np.max(np.abs(K - case.sn * np.eye(n) - ref)) <= 8 * SC.U, case
        assert np.all(np.diag(K) == 1.0 + case.sn)
        if case.m:
            assert np.max(np.abs(ks - O.cov_unit(kernel, U[n:], U[:n], 1.0))) <= 8 * SC.U, case
        if case.kind == "dup":
            assert K[1, 0] == 1.0 and np.array_equal(K[2:, 0], K[2:, 1]), "a duplicated row: sq = 0 exactly"
        if SC.AVAILABLE:
            Kl = T.build(case, SC.HP)[0]
            assert np.max(np.abs(Kl - K)) <= 8 * SC.U


@needs_ld
def test_every_case_is_admissible():
    """cond(K~) <= COND_CAP for EVERY case, by the long-double bound ||K~||_F ||K~^-1||_F >= cond_2: no GPU case is ever skipped for
    its conditioning; and the table has every shape the GPU tier names"""
    worst = max(T.cond_bound(c) for c in T.TABLE)
    print("cond(K~) <= %.3g over %d cases" % (worst, len(T.TABLE)))
    for c in T.TABLE:
        assert T.cond_bound(c) <= SC.COND_CAP, (c, T.cond_bound(c))
    for kernel in T.KERNELS:
        mine = [c for c in T.TABLE if c.kernel == kernel]
        assert {c.n for c in mine} == set(T.ORDERS) and {c.N for c in mine} == set(T.FEATURES) and {c.m for c in mine} == set(T.MS)
        assert {c.kind for c in mine} == set(T.KINDS)
    assert {(c.n, c.N) for c in T.TABLE} == {(n, N) for n in T.ORDERS for N in T.FEATURES}
    for c in T.TABLE:
        ell = T.inputs(c)[3]
        if c.kind == "ard":
            assert ell.shape == (c.N,) and ell.max() / ell.min() >= 99.9 * (c.N > 1), "two decades"
        if c.kind == "irrelevant":
            assert ell[c.N // 2] > 9e5 and np.all(np.delete(ell, c.N // 2) < 20)
        if c.kind == "dup":
            assert c.sn > 0 and np.array_equal(T.inputs(c)[0][0], T.inputs(c)[0][1])
    seen_cv, seen_hc = set(), set()
    for b in T.batches().values():
        for c in b.cases:
            assert all(SC.cv_admissible(c.n, *bg) for bg in b.cv) and all(SC.hc_admissible(c.n, *lm) for lm in b.hc)
        seen_cv |= set(b.cv); seen_hc |= set(b.hc)
    assert seen_cv == set(T.CV_LAYOUTS) and seen_hc == set(T.HC_SETTINGS)
    assert sorted(c for b in T.batches().values() for c in b.cases) == sorted(T.TABLE), "every case is in exactly one batch"


_LAYOUT_PROBE = r"""
#include <cstdio>
#include <initializer_list>
#include "smallgp_layout.hpp"
using namespace sigp;
int main() {
  const SmallFlavour fl[] = {SmallFlavour::Plain, SmallFlavour::Grad, SmallFlavour::Loo, SmallFlavour::Cv, SmallFlavour::Hindcast};
  for (int n : {2, 17, 96, 127, 128})
    for (int m : {0, 1, 8})
      for (int ch : {8, 16, 32})
        for (int f = 0; f < 5; ++f)
          std::printf("%d %d %d %d %ld %d %d\n", n, m, ch, f, SmallLayout{n, m, ch, fl[f]}.bytes(), small_out_width(fl[f], SmallCov::Factored),
                      small_out_width(fl[f], SmallCov::Stationary));
  static_assert(small_out_width(SmallFlavour::Grad, SmallCov::Stationary) == 4 && small_out_width(SmallFlavour::Grad, SmallCov::Factored) == 8, "");
  return 0;
}
"""


def test_the_stationary_flavours_have_the_factored_layouts(tmp_path):
    """SmallLayout does not ask for the covariance kind: the five flavours' images are the factored ones', whose sizes small_cases.lds_bytes
    states; only the width of ``out`` differs, for Grad (its N + 1 derivatives go to an array of their own)"""
    src = tmp_path / "probe.cpp"
    src.write_text(_LAYOUT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(rows) == 5 * 3 * 3 * 5
    for n, m, ch, f, nbytes, wf, ws in rows:
        assert nbytes == SC.lds_bytes(n, m, ch) + (SC.CV_EXTRA if f == 3 else 0), (n, m, ch, f)
        assert wf == (4, 8, 6, 6, 6)[f] and ws == (4, 4, 6, 6, 6)[f]


def test_the_library_declares_and_binds_the_five_entries():
    from seaiceextentforecasting_amd import _lib as L
    names = ["sigp_small_run_k" + s for s in ("", "_grad", "_loo", "_cv", "_hindcast")]
    header = open(os.path.join(ROOT, "include", "sigp.h")).read()
    for name in names:
        assert "int %s(sigp_handle* h" % name in header and name in L.SIGNATURES
    assert len(L.SIGNATURES["sigp_small_run_k_grad"][1]) == len(L.SIGNATURES["sigp_small_run_k"][1]) + 2
    assert L.load().sigp_version() >= 630


def _fake(kernel="rbf", dtype="f64"):
    return types.SimpleNamespace(kernel=kernel, dtype=dtype)


def test_small_stationary_batch_refusals():
    from seaiceextentforecasting_amd import SmallStationaryBatch, SmallBatch
    with pytest.raises(ValueError, match="RBF / Matern"):
        SmallStationaryBatch(_fake("netdiffusion"))
    with pytest.raises(ValueError, match="fp64"):
        SmallStationaryBatch(_fake("rbf", "f32"))
    with pytest.raises(ValueError, match="reference kernel"):
        SmallBatch(_fake("rbf"))                                   # SmallBatch keeps refusing the other kernels
    sb = SmallStationaryBatch(_fake("matern52"))
    rng = np.random.default_rng(1)
    X, y = rng.standard_normal((40, 5)), rng.standard_normal(40)
    with pytest.raises(ValueError, match="128"):
        sb.add_dataset(rng.standard_normal((129, 5)), rng.standard_normal(129))
    with pytest.raises(ValueError, match="rows"):
        sb.add_dataset(X, y[:-1])
    with pytest.raises(ValueError, match="Xs"):
        sb.add_dataset(X, y, rng.standard_normal((9, 5)))
    with pytest.raises(ValueError, match="Xs"):
        sb.add_dataset(X, y, rng.standard_normal((2, 4)))
    ds = sb.add_dataset(X, y, rng.standard_normal((2, 5)))
    for bad in ([1.0, 2.0], np.ones(6)):
        with pytest.raises(ValueError, match="N = 5"):
            sb.add_fit(ds, bad, 0.1)
    for bad in (0.0, -1.0, np.inf, np.nan, 1e-320, [1.0, 1.0, 0.0, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="length scale"):
            sb.add_fit(ds, bad, 0.1)
    with pytest.raises(ValueError, match="sn_tilde"):
        sb.add_fit(ds, 1.0, -0.1)
    with pytest.raises(ValueError, match="data set"):
        sb.add_fit(3, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="no fits"):
        sb.run()
    assert sb.add_fit(ds, 1.0, 0.1) == 0 and sb.add_fit(ds, np.ones(5), 0.0) == 1
    for kw in (dict(grad=True, loo="refit"), dict(grad=True, cv=dict(block=5)), dict(grad=True, hindcast=dict()), dict(loo="refit", cv=dict(block=5)),
               dict(loo="fixed", hindcast=dict()), dict(cv=dict(block=5), hindcast=dict(lead=1))):
        with pytest.raises(ValueError, match="separately"):
            sb.run(**kw)
    with pytest.raises(ValueError, match="loo must be"):
        sb.run(loo="both")
    for bad in (5, dict(gap=1), dict(block=5, window=3)):
        with pytest.raises(ValueError, match="cv must be"):
            sb.run(cv=bad)
    with pytest.raises(ValueError, match="exceeds 32"):
        sb.run(cv=dict(block=31, gap=1))
    sb.add_dataset(X[:10], y[:10])
    with pytest.raises(ValueError, match="training row"):
        sb.run(cv=dict(block=10))                                  # the set of 10 rows: one window of all of them
    with pytest.raises(ValueError, match="sigma_f"):
        sb.run(cv=dict(block=5, sigma_f="both"))
    with pytest.raises(ValueError, match="hindcast must be"):
        sb.run(hindcast=dict(block=1))
    with pytest.raises(ValueError, match="lead <= 32"):
        sb.run(hindcast=dict(lead=33))
    with pytest.raises(ValueError, match="no scored row"):
        sb.run(hindcast=dict(lead=32, min_train=9))
    sb.clear_fits()
    with pytest.raises(RuntimeError, match="no fits"):
        sb.run(grad=True)


def test_the_optimiser_refuses_other_criteria_by_name():
    from seaiceextentforecasting_amd import GPR
    gp = GPR.__new__(GPR)            # no device: the refusal comes first
    gp.kernel, gp.dtype = "rbf", "f64"
    with pytest.raises(ValueError, match="optimize_ard_batch.*optimize_cv_batch.*optimize_hindcast_batch"):
        gp.optimize_small_ard_batch([np.zeros((4, 2))], [np.zeros(4)], [0.0, 0.0], criterion="loo_nlpd")
    gp.kernel = "netdiffusion"
    with pytest.raises(ValueError, match="RBF / Matern"):
        gp.optimize_small_ard_batch([np.zeros((4, 2))], [np.zeros(4)], [0.0, 0.0])
    gp.kernel = "rbf"
    with pytest.raises(ValueError, match="share the number of features"):
        gp.optimize_small_ard_batch([np.zeros((4, 2)), np.zeros((4, 3))], [np.zeros(4)] * 2, [0.0, 0.0])
    with pytest.raises(RuntimeError, match="upload_small_ard"):
        gp.small_nlml_ard_batch(np.zeros((1, 3)))
    gp._h = None                     # __del__ has nothing to release
