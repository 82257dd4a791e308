"""CPU tier of the per-feature (ARD) gradients of the leave-one-out scores in lockstep groups (include/sigp.h: sigp_loo_grad_ard_batch): the
ABI is declared, exported and bound, the Python checks of ``GPR.loo_ard_batch`` / ``GPR.optimize_ard_batch`` refuse without a device, the
group layouts of csrc/score_layout.hpp are checked by a host compiler, and the lockstep BFGS of ``optim.py`` -- which
``optimize_ard_batch`` runs on ``loo_ard_batch`` -- minimises the leave-one-out density over d + 1 parameters per start, pinned on the
NumPy closed form of tests/test_loo_ard_host.py against SciPy's L-BFGS-B from the same start."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.optimize import minimize

from test_ard_batch_host import relevance_problem
from test_loo_ard_host import loo_ard_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc")
LOO_ARD_BATCH_SYMBOLS = {"sigp_loo_grad_ard_batch": 15}
SEEDS = (20260100, 20260101)            # B = 2 of the data sets of tests/test_ard_batch_host.py


def loo_objective(kind, X, y, crit="nlpd", mode="refit"):
    """theta -> (value, grad [d + 1]) of a leave-one-out score by the closed form; (inf, inf) where K~ is not SPD or the result is not finite"""
    d = X.shape[1]

    def f(th):
        try:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                r = loo_ard_closed_form(kind, X, y, np.exp(th[:d]), np.exp(th[d]), mode)
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        v, g = r[crit], r[crit + "_grad"]
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, np.full(d + 1, np.inf)
        return float(v), g
    return f


def test_loo_ard_batch_entry_point_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in LOO_ARD_BATCH_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert L.load().sigp_version() >= 590


def test_loo_ard_batch_null_handle_is_rejected_and_the_python_checks_come_first():
    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.ones(8)
    assert lib.sigp_loo_grad_ard_batch(None, 0, 1, 1, L.ptr(a), 4, 4, 0, 0, None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    p = inspect.signature(S.GPR.loo_ard_batch).parameters
    assert list(p)[1:] == ["theta", "first", "criterion", "sigma_f", "grad", "group", "predictions"]
    assert [p[k].default for k in list(p)[2:]] == [0, "loo_nlpd", "refit", "exact", 8, False]
    p = inspect.signature(S.GPR.optimize_ard_batch).parameters
    assert list(p)[1:] == ["X", "y", "theta0", "criterion", "sigma_f", "group", "maxiter", "gtol", "ftol", "max_step"]
    assert [p[k].default for k in list(p)[4:]] == ["loo_nlpd", "refit", 8, 50, 1e-5, 1e-10, 2.0]

    class Refusing:
        """stands for the library: every call on it is a device call the Python checks should have prevented"""
        def __getattr__(self, name):
            raise AssertionError("device call %s before the Python checks" % name)

    def handle(kernel="rbf", dtype="f64", d=None, n=None):
        gp = object.__new__(S.GPR)              # no handle: nothing below may reach the library
        gp.kernel, gp.dtype, gp._lib, gp._h = kernel, dtype, Refusing(), None
        if d is not None:
            gp._batch_d, gp._batch_n = d, n
        return gp

    th = np.zeros((3, 4))
    X, y = np.zeros((2, 5, 3)), np.zeros((2, 5))
    for bad in (dict(criterion="nlml"), dict(criterion="cv_nlpd"), dict(sigma_f="both"), dict(grad="ref"), dict(grad=True)):
        with pytest.raises(ValueError):
            handle(d=3, n=5).loo_ard_batch(th, **bad)
    with pytest.raises(ValueError, match="d \\+ 1"):
        handle(d=3, n=5).loo_ard_batch(th[:, :3])                # theta width
    with pytest.raises(RuntimeError, match="upload_batch"):
        handle().loo_ard_batch(th)                              # no upload_batch
    for kw in (dict(kernel="netdiffusion"), dict(dtype="f32")):
        with pytest.raises(ValueError, match="fp64 engine only"):
            handle(d=3, n=5, **kw).loo_ard_batch(th)
        with pytest.raises(ValueError, match="fp64 engine only"):
            handle(**kw).optimize_ard_batch(X, y, th[0])
    for bad in (dict(criterion="cv_nlpd"), dict(criterion="loo"), dict(sigma_f="both")):
        with pytest.raises(ValueError):
            handle().optimize_ard_batch(X, y, th[0], **bad)
    for bad0 in (np.zeros(3), np.zeros((2, 5))):
        with pytest.raises(ValueError, match="theta0"):
            handle().optimize_ard_batch(X, y, bad0)              # theta0 width, before the upload


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
// the pieces lie inside the arena, are disjoint, and add up to `size` doubles exactly (no gap the view does not know of) when `exact`
static void check_pieces(const char* view, const double* base, long size, const std::vector<Piece>& ps, bool exact) {
  const char* lo = (const char*)base;
  const char* hi = lo + size * 8;
  long total = 0;
  for (const Piece& x : ps) { expect((const char*)x.p >= lo && (const char*)x.p + x.bytes <= hi && x.bytes > 0, view, (const char*)x.p - lo, x.bytes); total += x.bytes; }
  for (size_t i = 0; i < ps.size(); ++i)
    for (size_t j = i + 1; j < ps.size(); ++j) {
      const char *a = (const char*)ps[i].p, *b = (const char*)ps[j].p;
      expect(a + ps[i].bytes <= b || b + ps[j].bytes <= a, view, (long)i, (long)j);
    }
  if (exact) expect(total == size * 8, view, total, size * 8);
}
static bool even(const double* base, const double* p) { return ((p - base) & 1) == 0; }
static double* const B0 = (double*)(uintptr_t)0x10000000;   // 16-byte aligned, never dereferenced

int main() {
  const long npads[] = {128, 256, 384, 4096}, Gs[] = {1, 2, 3, 8}, ds[] = {1, 8, 64, 65, 130};
  for (long n_pad : npads) for (long G : Gs) for (long d : ds) {
    const long dp = (d + 63) / 64 * 64, T = n_pad / 128, tiles = T * (T + 1);
    // ---- gV: the vectors of G members at an even stride
    LooArdGroupVecs gw{B0, n_pad, G};
    expect((gw.mstride() & 1) == 0, "LooArdGroupVecs: even member stride");
    expect(gw.mstride() >= LooArdVecs::size(n_pad), "LooArdGroupVecs: a member holds a LooArdVecs");
    expect(LooArdGroupVecs::size(G, n_pad) == G * gw.mstride(), "LooArdGroupVecs: size");
    expect(LooArdGroupVecs::size(1, n_pad) == gw.mstride(), "LooArdGroupVecs: what scores_grad_ensure is asked for per member");
    std::vector<Piece> ps;
    for (long b = 0; b < G; ++b) {
      const LooArdVecs w = gw.member(b), at{B0 + b * gw.mstride(), n_pad};
      expect(w.base == at.base && w.n_pad == at.n_pad && w.a() == at.a() && w.beta() == at.beta() && w.gamma() == at.gamma() && w.v() == at.v() && w.eps() == at.eps(),
             "LooArdGroupVecs: member(b) is the LooArdVecs at base + b mstride");
      expect(even(B0, w.a()) && even(B0, w.beta()) && even(B0, w.gamma()) && even(B0, w.v()), "LooArdGroupVecs: the four vectors at even offsets", b);
      ps.push_back({w.a(), n_pad * 8}); ps.push_back({w.beta(), n_pad * 8}); ps.push_back({w.gamma(), n_pad * 8}); ps.push_back({w.v(), n_pad * 8});
      ps.push_back({w.eps(), 8}); ps.push_back({w.eps() + 1, 8});      // eps and the spare double that makes the stride even
    }
    check_pieces("LooArdGroupVecs", B0, LooArdGroupVecs::size(G, n_pad), ps, true);
    // ---- gPart: ScoreParts of G members, the tile partials [G][tiles][dp], [G][d + 1] gradients; a group of nb <= G members
    for (long nb = 1; nb <= G; ++nb) {
      LooArdGroupParts gp{B0, G, n_pad, tiles, dp, d + 1};
      const ScoreParts sp = gp.scores();
      const ArdParts ap = gp.ard();
      expect(sp.base == B0 && sp.G == G && sp.n_pad == n_pad, "LooArdGroupParts begins with the ScoreParts of G members");
      expect(sp.sums() - B0 == G * 4 * n_pad, "LooArdGroupParts: the sums behind the rows of G members, not nb");
      expect(ap.base - B0 == ScoreParts::size(G, n_pad) && ap.G == G && ap.tiles == tiles && ap.dp == dp && ap.gw == d + 1, "LooArdGroupParts: ArdParts behind the ScoreParts");
      expect(ap.mstride() == tiles * dp && ap.grad() - ap.partial() == G * tiles * dp, "LooArdGroupParts: the gradients behind all G members' partials");
      ps.clear();
      for (long m = 0; m < nb; ++m) {
        ps.push_back({sp.mean(m), n_pad * 8}); ps.push_back({sp.var(m), n_pad * 8}); ps.push_back({sp.var(m) + n_pad, 2 * n_pad * 8});
        ps.push_back({ap.partial() + m * ap.mstride(), tiles * dp * 8}); ps.push_back({ap.grad() + m * ap.gw, (d + 1) * 8});
      }
      ps.push_back({sp.sums(), nb * 2 * 8});
      if (nb == G) ps.push_back({sp.sums() + 2 * G, 2 * G * 8});        // the spare half of ScoreParts' 4 doubles per member
      check_pieces("LooArdGroupParts", B0, LooArdGroupParts::size(G, n_pad, tiles, dp, d + 1), ps, nb == G);
    }
    expect(LooArdGroupParts::size(G, n_pad, tiles, dp, d + 1) == G * (4 * n_pad + 4) + G * tiles * dp + G * (d + 1), "LooArdGroupParts: size");
  }
  {  // numbers: n_pad = 256, G = 3, d = 8 (dp = 64, 6 tiles)
    LooArdGroupVecs gw{B0, 256, 3};
    LooArdGroupParts gp{B0, 3, 256, 6, 64, 9};
    expect(gw.mstride() == 1026 && gw.member(2).v() - B0 == 2820 && gw.member(2).eps() - B0 == 3076 && LooArdGroupVecs::size(3, 256) == 3078, "numbers: LooArdGroupVecs");
    expect(gp.scores().sums() - B0 == 3072 && gp.ard().partial() - B0 == 3084 && gp.ard().grad() - B0 == 4236 && LooArdGroupParts::size(3, 256, 6, 64, 9) == 4263,
           "numbers: LooArdGroupParts");
    expect(LooArdVecs::size(256) == 1025, "LooArdVecs stays what it was");
  }
  std::printf("%ld %ld\n", checks, bad);
  return 0;
}
'''


def test_group_layouts_of_the_loo_ard_batch(tmp_path):
    """LooArdGroupVecs and LooArdGroupParts over n_pad in {128, 256, 384, 4096}, G in {1, 2, 3, 8} (and every nb <= G), d in {1, 8, 64, 65,
    130}: the member stride is even, every vector at an even offset, member(b) the LooArdVecs at base + b mstride, the pieces of both views
    disjoint and adding up to their size, the sums behind G members, not nb"""
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    checks, bad = (int(x) for x in p.stdout.split())
    assert bad == 0, p.stderr
    assert checks > 10000, checks       # the sweep ran


def test_bfgs_lockstep_minimises_the_leave_one_out_density_from_four_starts():
    """``bfgs_lockstep`` on the closed form of the leave-one-out density: F = 4 starts on B = 2 data sets (start i on data set i % B, the
    batch's own pairing), p = d + 1 = 4.  For every start the value at the returned x is <= the value SciPy's L-BFGS-B reaches from the
    same start + 1e-6 |that value| (the bound of the nlML twin in tests/test_ard_batch_host.py).
    The reference runs WITHOUT a box: the lockstep driver has none, and unlike the nlML of these data sets their leave-one-out density has
    several basins (l_3 -> inf in all of them) -- a box at l <= e^5 turns the reference of seed 20260100 into another one, with l_2 and
    l_3 on the wall, so a boxed reference would compare the minima of two different problems."""
    from seaiceextentforecasting_amd.optim import bfgs_lockstep
    d, B = 3, len(SEEDS)
    data = [relevance_problem(s) for s in SEEDS]
    fs = [loo_objective("rbf", X, y) for X, y in data]
    starts = np.array([np.log([np.sqrt(3.0)] * d + [1e-2])] * B + [np.log([1.0, 2.0, 3.0, 3e-2])] * B)
    F = len(starts)

    def evaluate(theta):
        assert theta.shape == (F, d + 1)
        out = [fs[i % B](t) for i, t in enumerate(theta)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    res = bfgs_lockstep(evaluate, starts, maxiter=50)
    assert res["x"].shape == (F, d + 1) and res["jac"].shape == (F, d + 1)
    for i in range(F):
        ref = minimize(fs[i % B], starts[i], jac=True, method="L-BFGS-B")
        at = fs[i % B](res["x"][i])[0]
        print("start %d (seed %d): reference %.12g, lockstep %.12g (reported %.12g) in %d steps, x = %s" % (i, SEEDS[i % B], ref.fun, at, res["fun"][i], res["nit"][i], res["x"][i]))
        assert at == res["fun"][i]
        assert at <= ref.fun + 1e-6 * abs(ref.fun), (i, at, ref.fun)
    assert np.all(res["converged"])
