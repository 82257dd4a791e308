"""CPU tier of the per-feature (ARD) gradients of the hindcast scores in lockstep groups (include/sigp.h: sigp_hindcast_grad_ard_batch): the
ABI is declared, exported and bound, the Python checks of ``GPR.hindcast_ard_batch`` / ``GPR.hindcast_objective_batch`` /
``GPR.optimize_hindcast_batch`` refuse without a device, ``HindcastArdGroupVecs`` and the LDS rule of ``hindcast_w_lds_kernel`` in
csrc/score_layout.hpp are checked by a host compiler, ``hindcast_objective_batch``'s reduction is checked on a stub, and the lockstep
optimiser is run on the NumPy closed form of tests/test_hindcast_host.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import gp_oracle as O
from test_cv_ard_batch_host import _handle
from test_hindcast_host import hindcast_ard_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc")


def test_entry_point_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    name, nargs = "sigp_hindcast_grad_ard_batch", 17
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, "%s is not declared in include/sigp.h" % name
    assert len(m.group(1).split(",")) == nargs, m.group(1)
    assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
    assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
    assert L.load().sigp_version() >= 620
    a = np.ones(8)
    assert L.load().sigp_hindcast_grad_ard_batch(None, 0, 1, 1, L.ptr(a), 4, 4, 1, 2, 0, 0, None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    dbg_hdr = open(os.path.join(ROOT, "include", "sigp_debug.h")).read()
    assert re.search(r"\bint\s+sigp_debug_run_hindcast_w\s*\(", dbg_hdr) and hasattr(C.CDLL(L.DEBUG_LIB_PATH), "sigp_debug_run_hindcast_w")
    assert not hasattr(lib, "sigp_debug_run_hindcast_w")            # the product library has none of the debug entries


def test_signatures_of_the_new_methods():
    import seaiceextentforecasting_amd as S
    p = inspect.signature(S.GPR.hindcast_ard_batch).parameters
    assert list(p)[1:] == ["theta", "lead", "min_train", "first", "criterion", "sigma_f", "grad", "group", "predictions"]
    assert [p[k].default for k in list(p)[2:]] == [1, None, 0, "hindcast_nlpd", "refit", "exact", 8, False]
    p = inspect.signature(S.GPR.hindcast_objective_batch).parameters
    assert list(p)[1:] == ["theta", "lead", "min_train", "first", "criterion", "sigma_f", "group"]
    assert [p[k].default for k in list(p)[2:]] == [1, None, 0, "hindcast_nlpd", "refit", 8]
    p = inspect.signature(S.GPR.optimize_hindcast_batch).parameters
    assert list(p)[1:] == ["X", "y", "theta0", "lead", "min_train", "criterion", "sigma_f", "ard", "group", "maxiter", "gtol", "ftol", "max_step"]
    assert all(p[k].default is inspect.Parameter.empty for k in ("X", "y", "theta0"))
    assert [p[k].default for k in list(p)[4:]] == [1, None, "hindcast_nlpd", "refit", True, 8, 50, 1e-5, 1e-10, 2.0]


def test_the_python_checks_come_before_any_device_call():
    th = np.zeros((3, 4))
    th2 = np.zeros((3, 2))
    X, y = np.zeros((2, 40, 3)), np.zeros((2, 40))
    for bad in (dict(criterion="nlml"), dict(criterion="loo_nlpd"), dict(criterion="cv_nlpd")):
        with pytest.raises(ValueError, match="hindcast_nlpd"):
            _handle(d=3, n=40).hindcast_ard_batch(th, **bad)
        with pytest.raises(ValueError, match="hindcast_nlpd"):
            _handle(d=3, n=40).hindcast_objective_batch(th2, **bad)
        with pytest.raises(ValueError, match="hindcast_nlpd"):
            _handle().optimize_hindcast_batch(X, y, th[0], **bad)
    for call in (lambda **kw: _handle(d=3, n=40).hindcast_ard_batch(th, **kw), lambda **kw: _handle(d=3, n=40).hindcast_objective_batch(th2, **kw),
                 lambda **kw: _handle().optimize_hindcast_batch(X, y, th[0], **kw)):
        with pytest.raises(ValueError, match="sigma_f must be 'refit' or 'fixed'"):
            call(sigma_f="both")
        # the window, on the batch's n: no lead, a lead past 128, no training row, no scored row
        for lead, mt in ((0, 2), (129, 1), (1, 0), (1, 40), (36, 5)):
            with pytest.raises(ValueError, match="hindcast"):
                call(lead=lead, min_train=mt)
    for bad in (dict(grad="ref"), dict(grad=True)):
        with pytest.raises(ValueError, match="grad"):
            _handle(d=3, n=40).hindcast_ard_batch(th, **bad)
    with pytest.raises(ValueError, match="d \\+ 1"):
        _handle(d=3, n=40).hindcast_ard_batch(th[:, :3])            # theta width
    with pytest.raises(RuntimeError, match="upload_batch"):
        _handle().hindcast_ard_batch(th)                            # no upload_batch
    with pytest.raises(RuntimeError, match="upload_batch"):
        _handle().hindcast_objective_batch(th2)
    for kw in (dict(kernel="netdiffusion"), dict(dtype="f32")):
        with pytest.raises(ValueError, match="fp64 engine only"):
            _handle(d=3, n=40, **kw).hindcast_ard_batch(th)
        with pytest.raises(ValueError, match="fp64 engine only"):
            _handle(d=3, n=40, **kw).hindcast_objective_batch(th2)
        with pytest.raises(ValueError, match="fp64 engine only"):
            _handle(**kw).optimize_hindcast_batch(X, y, th[0])
    with pytest.raises(ValueError):
        _handle(d=3, n=40).hindcast_objective_batch(th)             # [F, 2] required
    # theta0 through _ard_starts, before the upload
    for bad0 in (np.zeros(3), np.zeros((2, 5))):
        with pytest.raises(ValueError, match="theta0"):
            _handle().optimize_hindcast_batch(X, y, bad0)
    for bad0 in (np.zeros(4), np.zeros((2, 3))):
        with pytest.raises(ValueError, match="theta0"):
            _handle().optimize_hindcast_batch(X, y, bad0, ard=False)
    with pytest.raises(ValueError, match="hindcast"):
        _handle().optimize_hindcast_batch(X, y, th[0], min_train=None, lead=37)      # min_train=None is max(2, d + 1) = 4: 4 + 36 > 39
    # the siblings still refuse the hindcast criteria
    with pytest.raises(ValueError):
        _handle(d=3, n=40).loo_ard_batch(th, criterion="hindcast_nlpd")
    with pytest.raises(ValueError):
        _handle(d=3, n=40).cv_ard_batch(th, 5, criterion="hindcast_nlpd")
    with pytest.raises(ValueError):
        _handle().optimize_ard_batch(X, y, th[0], criterion="hindcast_nlpd")
    with pytest.raises(ValueError):
        _handle().optimize_cv_batch(X, y, th[0], 5, criterion="hindcast_nlpd")
    with pytest.raises(ValueError, match="optimize_ard"):
        _handle().optimize_batch(X, y, th[0], ard=True, criterion="hindcast_nlpd")


def test_starts_are_those_of_the_siblings():
    """theta0 [2], [d + 1], [S B, 2], [B, d + 1] -> the starts ``_ard_starts`` makes of them, as they reach the objective"""
    class Stop(Exception):
        pass

    seen = {}

    def stub(theta, **kw):
        seen.update(shape=np.shape(theta), kw=kw)
        raise Stop()

    for theta0, want in ((np.array([0.5, -2.0]), (2, 4)), (np.zeros(4), (2, 4)), (np.zeros((6, 2)), (6, 4)), (np.zeros((2, 4)), (2, 4))):
        gp = _handle()
        gp.upload_batch = lambda *a, **kw: None
        gp.hindcast_ard_batch = stub
        with pytest.raises(Stop):
            gp.optimize_hindcast_batch(np.zeros((2, 40, 3)), np.zeros((2, 40)), theta0, lead=2, group=3)
        assert seen["shape"] == want
        assert seen["kw"] == dict(lead=2, min_train=4, criterion="hindcast_nlpd", sigma_f="refit", group=3)      # min_train=None became max(2, d + 1)


def test_hindcast_objective_batch_sums_the_components_of_a_stub():
    """``hindcast_objective_batch`` is ``hindcast_ard_batch`` at equal scales with d/dlog l = sum_k d/dlog l_k; a non-finite exp gives inf"""
    d, n = 3, 40
    seen = {}

    def stub(theta, lead=1, min_train=None, first=0, criterion="hindcast_nlpd", sigma_f="refit", grad="exact", group=8, predictions=False):
        seen.update(theta=np.array(theta), args=(lead, min_train, first, criterion, sigma_f, grad, group, predictions))
        F = theta.shape[0]
        return np.arange(1.0, F + 1), np.arange(F * (d + 1), dtype=np.float64).reshape(F, d + 1) + 0.25

    gp = _handle(d=d, n=n)
    gp.hindcast_ard_batch = stub
    th = np.array([[0.5, -2.0], [800.0, -1.0], [-0.25, -3.0], [0.0, np.inf]])
    v, g = gp.hindcast_objective_batch(th, lead=2, first=1, criterion="hindcast_sse", sigma_f="fixed", group=3)
    assert seen["args"] == (2, 4, 1, "hindcast_sse", "fixed", "exact", 3, False)             # min_train=None became max(2, d + 1)
    assert seen["theta"].shape == (4, d + 1) and np.all(np.isfinite(seen["theta"]))         # a member that cannot be evaluated rides at harmless parameters
    for i in (0, 2):
        assert np.all(seen["theta"][i, :d] == th[i, 0]) and seen["theta"][i, d] == th[i, 1]
    assert v.shape == (4,) and g.shape == (4, 2)
    full = np.arange(4 * (d + 1), dtype=np.float64).reshape(4, d + 1) + 0.25
    for i in (0, 2):
        assert v[i] == i + 1.0 and g[i, 0] == np.sum(full[i, :d]) and g[i, 1] == full[i, d]
    for i in (1, 3):
        assert np.isposinf(v[i]) and np.all(np.isposinf(g[i]))


LAYOUT_PROGRAM = r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "score_layout.hpp"
using namespace sigp;

static long checks = 0, bad = 0;
static void expect(bool ok, const char* what, long a = 0, long b = 0) {
  ++checks;
  if (!ok && ++bad <= 20) std::fprintf(stderr, "FAILED %s (%ld, %ld)\n", what, a, b);
}
struct Piece { const void* p; long bytes; };
static void check_pieces(const char* view, const double* base, long size, const std::vector<Piece>& ps) {
  const char* lo = (const char*)base;
  const char* hi = lo + size * 8;
  for (const Piece& x : ps) expect((const char*)x.p >= lo && (const char*)x.p + x.bytes <= hi && x.bytes > 0, view, (const char*)x.p - lo, x.bytes);
  for (size_t i = 0; i < ps.size(); ++i)
    for (size_t j = i + 1; j < ps.size(); ++j) {
      const char *a = (const char*)ps[i].p, *b = (const char*)ps[j].p;
      expect(a + ps[i].bytes <= b || b + ps[j].bytes <= a, view, (long)i, (long)j);
    }
}
static double* const V0 = (double*)(uintptr_t)0x40000000;   // 16-byte aligned, never dereferenced
static bool even(const double* p) { return ((p - V0) & 1) == 0; }

int main() {
  const long npads[] = {128, 256, 384, 1152, 4096, 8192, 16384}, Gs[] = {1, 2, 3, 8};
  for (long n_pad : npads)
    for (long G : Gs) {
      const HindcastArdGroupVecs gv{V0, n_pad, G};
      const long size = HindcastArdGroupVecs::size(G, n_pad);
      expect((gv.mstride() & 1) == 0, "HindcastArdGroupVecs: an even member stride", gv.mstride());
      expect(gv.mstride() >= HindcastArdVecs::size(n_pad) && size == G * gv.mstride(), "HindcastArdGroupVecs: size and stride");
      for (long nb = 1; nb <= G; ++nb) {       // a group of nb <= G members on a workspace laid out for G
        std::vector<Piece> ps;
        for (long m = 0; m < nb; ++m) {
          const HindcastVecs hv = gv.member(m).hc();
          const LooArdVecs w = gv.member(m).ard();
          // the launches reach member m at m mstride() behind member 0's views
          expect(hv.base == gv.member(0).hc().base + m * gv.mstride() && w.base == gv.member(0).ard().base + m * gv.mstride(), "HindcastArdGroupVecs: member m behind member 0", m);
          for (double* v : {hv.cum(), hv.r(), hv.w(), hv.rho(), hv.ks(), hv.suf(), hv.zbar(), w.a(), w.beta(), w.gamma(), w.v()}) ps.push_back({v, n_pad * 8});
          ps.push_back({w.eps(), 8});
          expect(even(w.a()) && even(w.beta()) && even(w.gamma()) && even(w.v()), "HindcastArdGroupVecs: the ARD pass's vectors at even offsets", m);
          expect(w.eps() + 1 <= V0 + (m + 1) * gv.mstride(), "HindcastArdGroupVecs: eps inside the member", m);
        }
        check_pieces("HindcastArdGroupVecs", V0, size, ps);
      }
      if (G == 1) expect(gv.member(0).hc().base == HindcastArdVecs{V0, n_pad}.hc().base && gv.member(0).ard().base == HindcastArdVecs{V0, n_pad}.ard().base, "one member: HindcastArdVecs");
    }
  // the LDS rule of hindcast_w_lds_kernel: monotone, inside what a workgroup may have at the limit (its 2 KB + 8 of static LDS on top), the
  // other kernel beyond it; the row of n_pad doubles and its skew of one per 32 fit the row's share
  const long LDS_MAX = 160 * 1024, STATIC = 256 * 8 + 8;
  long prev = 0;
  for (long n_pad = 128; n_pad <= 32768; n_pad += 128) {
    const long b = hindcast_w_lds_bytes(n_pad);
    expect(b > prev, "hindcast_w_lds_bytes: monotone", n_pad, b);
    prev = b;
    expect(b >= 16 * n_pad && b <= 17 * n_pad, "hindcast_w_lds_bytes: 16 n_pad and the skew", n_pad, b);
    expect((n_pad - 1) + ((n_pad - 1) >> 5) < hindcast_w_lds_row(n_pad), "the last skewed index inside the row", n_pad);
    expect(b == 2 * 8 * hindcast_w_lds_row(n_pad), "two rows", n_pad);
    expect(hindcast_w_use_lds(n_pad) == (n_pad <= HINDCAST_W_LDS_MAX_NPAD), "the rule is the limit", n_pad);
    if (hindcast_w_use_lds(n_pad)) expect(b + STATIC <= LDS_MAX, "inside 160 KiB wherever the LDS kernel is chosen", n_pad, b);
  }
  expect(HINDCAST_W_LDS_MAX_NPAD % 128 == 0 && hindcast_w_lds_bytes(HINDCAST_W_LDS_MAX_NPAD) + STATIC <= LDS_MAX, "the limit itself");
  expect(!hindcast_w_use_lds(HINDCAST_W_LDS_MAX_NPAD + 128), "one block beyond the limit falls back");
  expect(hindcast_w_lds_bytes(8192) == 135168 && HindcastArdGroupVecs::size(3, 256) == 3 * 2818, "numbers");
  std::printf("%ld %ld\n", checks, bad);
  return 0;
}
'''


def test_group_vectors_and_the_lds_rule(tmp_path):
    """``HindcastArdGroupVecs`` over n_pad in {128 .. 16384}, G in {1, 2, 3, 8} and every nb <= G: the pieces inside the arena, disjoint, the
    member stride even, a partial group on a workspace laid out for G; ``hindcast_w_lds_bytes`` over every n_pad up to 32768: monotone, at
    most 160 KiB with the kernel's static LDS wherever ``hindcast_w_use_lds`` says yes, no beyond the stated limit"""
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    checks, bad = (int(x) for x in p.stdout.split())
    assert bad == 0, p.stderr
    assert checks > 5000, checks      # the sweep ran
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    assert "n_pad <= 8192" in hdr     # the limit is stated where callers read


def _closed_form_objective(kind, X, y, lead, mt, crit="nlpd", mode="refit"):
    """theta -> (value, grad [d + 1]) of a hindcast score by the closed form; (inf, inf) where K~ is not SPD or the result is not finite"""
    d = X.shape[1]

    def f(th):
        try:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                r = hindcast_ard_closed_form(kind, X, y, np.exp(th[:d]), np.exp(th[d]), lead, mt, mode)
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        v, g = r[crit], r[crit + "_grad"]
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, np.full(d + 1, np.inf)
        return float(v), g
    return f


def test_lockstep_optimiser_on_the_closed_form_ends_where_scipy_ends():
    """Two tiny data sets (n = 12, d = 2), hindcast nlpd at lead 1, min_train 3, two starts each, through ``optim.bfgs_lockstep`` as
    ``optimize_hindcast_batch`` drives it (start i on data set i % B).  SciPy's BFGS from the same start ends at the same minimum: the
    values agree to 1e-8 (both stop at a gradient of at most 1e-6, and the value's error is quadratic in it), the points to 1e-3 (one
    scale runs along a flat direction)."""
    from seaiceextentforecasting_amd.optim import bfgs_lockstep
    B, n, d, lead, mt = 2, 12, 2, 1, 3
    fs = []
    for b in range(B):
        X, y, _ = O.synthetic_problem(n, d, 20264200 + b)
        fs.append(_closed_form_objective("rbf", X, y, lead, mt))
    th0 = np.log([np.sqrt(2.0), np.sqrt(2.0), 1e-1])
    starts = np.concatenate([np.tile(th0, (B, 1)), np.tile(th0 + [0.3, -0.2, 0.5], (B, 1))])

    def evaluate(T):
        out = [fs[i % B](T[i]) for i in range(len(T))]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    res = bfgs_lockstep(evaluate, starts, maxiter=200, gtol=1e-6)
    assert np.all(res["converged"]), res
    for i in range(len(starts)):
        ref = minimize(fs[i % B], starts[i], jac=True, method="BFGS", options=dict(gtol=1e-6))
        print("start %d: lockstep %.12g at %s in %d steps; scipy %.12g at %s" % (i, res["fun"][i], res["x"][i], res["nit"][i], ref.fun, ref.x))
        assert res["fun"][i] < evaluate(starts)[0][i]
        assert abs(res["fun"][i] - ref.fun) <= 1e-8 * max(1.0, abs(ref.fun)), (i, res["fun"][i], ref.fun)
        assert np.max(np.abs(res["x"][i] - ref.x)) <= 1e-3, (i, res["x"][i], ref.x)


def test_the_years_of_the_gpu_optimiser_test_have_an_irrelevant_third_feature():
    """the closed form alone, through the same lockstep optimiser, puts l_3 above l_1 and l_2 in both years of
    tests/test_hip_hindcast_ard_batch.py's optimiser test, from both of its starts: what that test then asks of the device"""
    from seaiceextentforecasting_amd.optim import bfgs_lockstep
    from test_hip_hindcast_ard_batch import _years
    Xb, yb, d, th0 = _years()
    B = len(Xb)
    fs = [_closed_form_objective("rbf", Xb[b], yb[b], 1, 8) for b in range(B)]
    starts = np.concatenate([np.tile(th0, (B, 1)), np.tile(np.log([1.0, 2.0, 1.5, 1e-1]), (B, 1))])

    def evaluate(T):
        out = [fs[i % B](T[i]) for i in range(len(T))]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    res = bfgs_lockstep(evaluate, starts)
    assert np.all(res["converged"]) and np.all(res["fun"] < evaluate(starts)[0])
    assert np.all(res["x"][:, 2] > res["x"][:, 0] + 1.0) and np.all(res["x"][:, 2] > res["x"][:, 1] + 1.0), res["x"]
