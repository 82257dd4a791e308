"""CPU tier of the leave-block-out score gradient of the one-workgroup kernel (csrc/smallgp.hpp: CvGrad; helpers: tests/small_cv_grad_cases.py):
the closed form the GPU tier (tests/test_hip_small_cv_grad.py) measures the device against equals central differences of the score
``small_cases`` defines, its adjoint equals the fp64 NumPy statement of tests/test_cv_ard_host.py and, at block 1 without a gap, the
leave-one-out adjoint; the LDS image of the flavour (``SmallLayout``, csrc/smallgp_layout.hpp) is swept by a stand-alone host program; and
the Python surface checks its arguments without a device."""
import os
import subprocess

import numpy as np
import pytest

import small_cases as SC
import small_cv_grad_cases as CG
import small_grad_cases as GC
from test_cv_ard_host import cv_adjoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")
FD_TOL = 1e-7            # of S: catches a wrong formula, not rounding (step 1e-5 in log theta: truncation ~1e-10, rounding ~1e-14)


def _case(n):
    """the first 'eigh' table case of order n with N = 17 whose condition stays under the cap"""
    return next(c for c in SC.TABLE if c.n == n and c.N == 17 and c.expm == "eigh" and SC.H.cond2(np.asarray(SC.reference(c, SC.F64)["K"], dtype=np.float64)) < SC.COND_CAP)


@needs_ld
@pytest.mark.parametrize("n", [3, 17, 33])
def test_cv_closed_form_equals_central_differences(n):
    """every layout of small_cases.CV_LAYOUTS the order admits: n = 3 (1, 0) alone, n = 17 those with a window <= 16, n = 33 all seven"""
    c = _case(n)
    st = SC.staged(c)
    lay = [bg for bg in SC.CV_LAYOUTS if SC.cv_admissible(n, *bg)]
    assert len(lay) == {3: 1, 17: 4, 33: 7}[n]
    for block, gap in lay:
        for mode in SC.MODES:
            for crit in CG.CRITERIA:
                r = CG.score_grad(st, c.ell, c.sn, SC.HP, block, gap, mode, crit)
                fd = CG.central_difference(st, c.ell, c.sn, block, gap, mode, crit)
                err = np.abs(r["grad"] - fd) / r["S"]
                print("cv n = %d block = %d gap = %d %s %s: grad %s, |closed - fd| / S %s" % (n, block, gap, mode, crit, r["grad"].astype(np.float64), err.astype(np.float64)))
                assert np.all(r["S"] > 0) and np.all(err <= FD_TOL), (c, block, gap, mode, crit, err)


def test_the_adjoint_restates_the_numpy_statement_of_the_blocked_engine():
    """fp64 against fp64: the same formulas, so agreement to a few ulps of the adjoint's largest entry times the condition of the solve"""
    for n in (3, 17, 33):
        c = _case(n)
        core = SC.reference(c, SC.F64)
        y, P = (np.asarray(core[k], dtype=np.float64) for k in ("y", "P"))
        for block, gap in [bg for bg in SC.CV_LAYOUTS if SC.cv_admissible(n, *bg)]:
            for mode in SC.MODES:
                for crit in CG.CRITERIA:
                    G, G0 = CG.cv_adjoint(core, block, gap, mode, crit), cv_adjoint(P, y, block, gap, mode, crit)
                    assert np.max(np.abs(G - G0)) <= 1e-9 * np.max(np.abs(G0)), (c, block, gap, mode, crit)


@needs_ld
def test_block_one_without_a_gap_is_the_leave_one_out_adjoint():
    for n in (3, 17):
        c = _case(n)
        for ar in (SC.HP, SC.F64):
            core = SC.reference(c, ar)
            for mode in SC.MODES:
                for crit in CG.CRITERIA:
                    G, G0 = CG.cv_adjoint(core, 1, 0, mode, crit), GC.loo_adjoint(core, mode, crit)
                    assert np.max(np.abs(G - G0)) <= 1e-9 * np.max(np.abs(G0)), (c, ar.name, mode, crit)


# ---- the LDS image of the flavour -----------------------------------------------------------------------------------------------------------------
LAYOUT_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "smallgp_layout.hpp"
using namespace sigp;

int main() {
  std::printf("K %d %d %d %d %ld %d %d %d %d %d %d %d %d\n", SM_NMAX, SM_MMAX, SM_GV, SM_CVW, SM_LDS_MAX, (int)SmallFlavour::Plain, (int)SmallFlavour::Grad, (int)SmallFlavour::Loo,
              (int)SmallFlavour::Cv, (int)SmallFlavour::Hindcast, (int)SmallFlavour::LooGrad, (int)SmallFlavour::HindcastGrad, (int)SmallFlavour::CvGrad);
  const SmallFlavour g = SmallFlavour::CvGrad;
  std::printf("F %d %d %d\n", small_out_width(g), (int)small_has_rows(g), (int)small_is_score_grad(g));
  for (int n = 1; n <= SM_NMAX; ++n)
    for (int m = 0; m <= SM_MMAX; ++m) {
      const int up = small_pick_chunk(n, m, SmallFlavour::Plain, 32);
      for (int ch : {8, 16, 32}) {
        const SmallLayout c{n, m, ch, SmallFlavour::Cv};
        std::printf("V %d %d %d %ld %ld %ld %ld\n", n, m, ch, c.bytes(), c.Pw(), c.Ww(), c.tv());
      }
      for (int win = 1; win <= SM_CVW; ++win) {
        for (int ch : {8, 16, 32}) {
          const SmallLayout l{n, m, ch, g, win};
          std::printf("L %d %d %d %d %ld %d %d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", n, m, ch, win, l.bytes(), l.ldk(), l.lda(), l.Kp(), l.Ac(), l.wk(), l.kss(), l.red(),
                      l.at(), l.Pw(), l.Ww(), l.tv(), l.Bc(), l.gv(), l.hb());
        }
        std::printf("C %d %d %d %d %d\n", n, m, win, up, up ? small_pick_chunk(n, m, g, up, win) : 0);
      }
    }
  return 0;
}
'''


@pytest.mark.parametrize("sanitize", [False, True])
def test_layout_of_the_leave_block_out_gradient(tmp_path, sanitize):
    """every size, offset and chunk of CvGrad at n = 1 .. 128, m = 0 .. 8, window 1 .. 32, ch in {8, 16, 32}: the pieces lie inside bytes() and do
    not overlap, Pw / Ww / tv are where Cv has them, the launch is accepted exactly where an image fits in SM_LDS_MAX, at the largest chunk
    that does, the promised floor holds and the earlier enumerators keep their values.  Once more under the host sanitizers (a stand-alone
    program with its own main)."""
    src = tmp_path / "cv_grad_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "cv_grad_layout"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc"), "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = {k: [] for k in "KFVLC"}
    for line in p.stdout.split("\n"):
        if line:
            rows[line[0]].append([int(x) for x in line.split()[1:]])
    assert rows["K"] == [[128, 8, 4, CG.MAX_WINDOW, CG.LDS_MAX, 0, 1, 2, 3, 4, 5, 6, 7]]       # appended: enumerators 0 .. 6 keep their values
    assert rows["F"] == [[8, 1, 1]]
    assert len(rows["L"]) == 128 * 9 * 32 * 3 and len(rows["C"]) == 128 * 9 * 32 and len(rows["V"]) == 128 * 9 * 3
    cv = {(n, m, ch): (size, Pw, Ww, tv) for n, m, ch, size, Pw, Ww, tv in rows["V"]}
    W, WP = SC.CV_W, SC.CV_W + 1
    for n, m, ch, win, size, ldk, lda, Kp, Ac, wk, kss, red, at, Pw, Ww, tv, Bc, gv, hb in rows["L"]:
        assert size == CG.cv_grad_lds_bytes(n, m, ch, win), (n, m, ch, win)
        assert (ldk, lda) == (n | 1, ch + 1)
        assert (Kp, Ac, wk, kss, red, at) == (0, (n + 1 + m) * ldk, (n + 1 + m) * ldk + (n + m) * lda, wk + ch, kss + 8, red + 16), (n, m, ch, win)
        assert (Pw, Ww, tv) == cv[(n, m, ch)][1:] and Pw * 8 == SC.lds_bytes(n, m, ch), "the folds' scratch lies where Cv has it"
        assert Bc * 8 == cv[(n, m, ch)][0] == SC.lds_bytes(n, m, ch) + SC.CV_EXTRA, "the new pieces lie behind the leave-block-out image"
        pieces = sorted([(Kp, (n + 1 + m) * ldk), (Ac, (n + m) * lda), (wk, ch), (kss, 8), (red, 16), (at, n), (Pw, W * WP), (Ww, W * WP), (tv, W), (Bc, n * lda), (gv, 4 * n),
                         (hb, n * win)])
        assert pieces[0][0] >= 0 and 8 * (pieces[-1][0] + pieces[-1][1]) <= size, (n, m, ch, win)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(pieces, pieces[1:])), (n, m, ch, win)
    for n, m, win, up, ch in rows["C"]:
        assert (up or None, ch or None) == (SC.upload_chunk(n, m), CG.cv_grad_chunk(n, m, win)), (n, m, win)
        fits = [c for c in (8, 16, 32) if up and c <= up and CG.cv_grad_lds_bytes(n, m, c, win) <= CG.LDS_MAX]
        assert ch == (max(fits) if fits else 0), "accepted exactly where an image fits, at the largest chunk that does"
        if n <= CG.FLOOR[0] and m <= CG.FLOOR[1] and win <= CG.FLOOR[2]:
            assert ch >= 8, ("the floor", n, m, win)
    # the limits include/sigp.h, smallgp_layout.hpp and SmallBatch.run state
    assert [CG.order_limit(0, w) for w in (1, 5, 8, 16, 32)] == [123, 121, 119, 116, 109]
    assert [CG.order_limit(8, w) for w in (1, 5, 8, 16, 32)] == [119, 117, 115, 113, 106]
    assert [CG.cv_grad_chunk(96, 8, w) for w in (1, 10, 11, 32)] == [32, 32, 16, 16]


# ---- the Python surface, without a device --------------------------------------------------------------------------------------------------------
def test_cv_grad_argument_checks_need_no_device():
    sb = SC.host_batch([SC.Case(17, 17, 1, 0.05, 1.0, "eigh", 20265017)])
    with pytest.raises(ValueError, match="score must be 'nlpd' or 'sse'"):
        sb.run(cv_grad=dict(block=5, score="nlml"))
    with pytest.raises(ValueError, match="exceeds 32 rows"):
        sb.run(cv_grad=dict(block=31, gap=1))
    with pytest.raises(ValueError, match="must leave a training row"):
        sb.run(cv_grad=dict(block=17))
    with pytest.raises(ValueError, match=r"cv_grad must be dict\(block="):
        sb.run(cv_grad=dict(gap=1))
    with pytest.raises(ValueError, match=r"cv_grad must be dict\(block="):
        sb.run(cv_grad=dict(block=5, lead=1))
    for other in (dict(grad=True), dict(loo="refit"), dict(cv=dict(block=5)), dict(hindcast=dict(lead=1)), dict(loo="refit", score_grad="nlpd")):
        with pytest.raises(ValueError, match="run them separately"):
            sb.run(cv_grad=dict(block=5), **other)
    # the three refusals the earlier tiers pin stay as they are
    with pytest.raises(ValueError, match="block-CV gradients are not built"):
        sb.run(cv=dict(block=5), score_grad="nlpd")
    import seaiceextentforecasting_amd as S
    gp = S.GPR.__new__(S.GPR)
    gp.kernel = "netdiffusion"
    with pytest.raises(ValueError, match="block-CV gradients are not built"):
        gp.small_score_batch(np.zeros((1, 2)), criterion="cv_nlpd")
    with pytest.raises(ValueError, match="block-CV gradients are not built"):
        gp.optimize_small_batch([np.zeros((3, 2))], [np.zeros(3)], np.zeros(2), criterion="cv_sse")
    # ... and the new names check theirs before they touch the device
    with pytest.raises(ValueError, match="'cv_nlpd' or 'cv_sse'"):
        gp.small_cv_score_batch(np.zeros((1, 2)), 5, criterion="loo_nlpd")
    with pytest.raises(ValueError, match="exceeds 32 rows"):
        gp.optimize_small_cv_batch([np.zeros((3, 2))], [np.zeros(3)], np.zeros(2), 33)
    gp.kernel = "rbf"
    with pytest.raises(ValueError, match="optimize_cv_batch"):
        gp.optimize_small_cv_batch([np.zeros((3, 2))], [np.zeros(3)], np.zeros(2), 5)
