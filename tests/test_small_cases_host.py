"""CPU tier of the one-workgroup kernel's case table (tests/small_cases.py): the long-double closed forms that the GPU tier
(tests/test_hip_small_flavours.py) measures the device against are pinned to REAL long-double refits, the table meets its condition cap
through the real ``SmallBatch`` staging, every layout listed for a batch is admissible for every set of it, the fp64 comparator's own
error is a usable unit, and the LDS anchors of the leave-block-out launch follow from ``SmallLayout`` (csrc/smallgp_layout.hpp)."""
import os
import subprocess

import numpy as np
import pytest

import hp_reference as H
import small_cases as SC
from test_hindcast_host import scored_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not SC.AVAILABLE, reason="long double is fp64 on this platform")
LD = SC.LD
TOL = 1e3 * float(np.finfo(LD).eps)       # the precision of the reference itself on matrices of condition <= 1e4


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _refit_without(K, y, sn, r0, r1, c0, c1):
    """``hp_reference.hp_refit_without`` -- a REAL long-double refit without the rows [r0, r1), predicting [c0, c1) -- with k** = K_ii - sn~
    taken in long double: the helper's fp64 subtraction rounds at u |K_ii|, which is 1e3 eps_ld of a variance well below K_ii.  The means
    are the helper's own.  Also the refit's sigma_f."""
    keep = np.ones(len(y), dtype=bool)
    keep[r0:r1] = False
    r = H.hp_fit(K[np.ix_(keep, keep)], y[keep], sn, ks=K[c0:c1][:, keep], kss=np.diag(K)[c0:c1].astype(LD) - LD(sn), block=0)
    mean, _ = H.hp_refit_without(K, y, sn, r0, r1, c0, c1)
    assert np.array_equal(mean, r["mean"])
    return r["mean"], r["var"], r["sigma_f"]


@pytest.fixture(scope="module")
def refit_cases():
    """a few table cases with n <= 33, as fp64 matrices (closed form and refits must see the SAME matrix).  cond(K~) <= 1e3 = TOL / eps_ld,
    inside the 1e4 the tolerance was stated for: the closed forms subtract (y^T a~ - a~_S^T P_SS^-1 a~_S with one training row left), and
    what that loses grows with the condition"""
    out = []
    for c in SC.TABLE:
        if c.n in (3, 16, 17, 33) and c.N in (15, 17, 65) and c.expm == "eigh":
            K, ks, kss, dK = SC.build(SC.staged(c), c.ell, c.sn, SC.HP)
            K = np.asarray(K, dtype=np.float64)
            if H.cond2(K) <= 1e3:
                out.append((c, K, np.asarray(SC.staged(c)[1], dtype=np.float64)))
    assert len(out) >= 4 and {c.n for c, _, _ in out} >= {3, 17, 33}
    return out


@needs_ld
def test_loo_and_cv_closed_forms_equal_real_long_double_refits(refit_cases):
    worst = 0.0
    for c, K, y in refit_cases:
        core = SC.core_from_matrix(K, y, c.sn, SC.HP)
        # windows of at most half the rows: s_S = (y^T a~ - a~_S^T P_SS^-1 a~_S) / (n - |S|) is a difference, and with ONE training row left
        # (block = n - 1) it keeps 1e-15 of a long-double fit of condition 700 -- the closed form's own limit, not a disagreement
        layouts = [(1, 0)] + [bg for bg in SC.CV_LAYOUTS + ((c.n // 2, 0),) if SC.cv_admissible(c.n, *bg) and bg[0] + 2 * bg[1] <= c.n // 2]
        # ... and block = n - 1 all the same (the GPU tier's batch s15 runs (14, 0)): means and "fixed" variances at TOL; the "refit" variance
        # at 2 TOL q / (q - t), t = a~_S^T P_SS^-1 a~_S -- q and t are each good to TOL, their difference to TOL (q + t) / (q - t)
        for block, gap in dict.fromkeys(layouts + [(c.n - 1, 0)]):
            wide = block + 2 * gap > c.n // 2
            got = SC.cv_rows(core, block, gap, "refit")
            fixed = SC.cv_rows(core, block, gap, "fixed")
            loo = SC.loo_rows(core, "refit") if (block, gap) == (1, 0) else None
            for r0, r1, c0, c1 in H.cv_folds(c.n, block, gap):
                mean, var, sf_fold = _refit_without(K, y, c.sn, r0, r1, c0, c1)
                e = max(float(np.max(np.abs(got["mean"][c0:c1] - mean))) / max(1.0, float(np.max(np.abs(y)))),
                        _rel(fixed["var"][c0:c1], var * core["sigma_f"] / sf_fold))
                if wide:      # q / (q - t) = n sigma_f / ((n - |S|) s_S), from the two modes' variances of one row
                    amp = float(c.n * fixed["var"][c0] / ((c.n - (r1 - r0)) * got["var"][c0]))
                    e_refit = _rel(got["var"][c0:c1], var)
                    print("n = %d block = %d fold at %d: refit variance %.3g, q / (q - t) = %.3g" % (c.n, block, r0, e_refit, amp))
                    assert amp >= 1 and e_refit <= 2 * amp * TOL, (c, block, r0, e_refit, amp)
                else:
                    e = max(e, _rel(got["var"][c0:c1], var))
                if loo is not None:
                    e = max(e, _rel(loo["var"][c0:c1], var), float(np.max(np.abs(loo["mean"][c0:c1] - mean))))
                worst = max(worst, e)
                assert e <= TOL, (c, block, gap, r0, e)
            assert np.array_equal(got["mean"], fixed["mean"])
    print("closed forms against refits: worst %.3g (tolerance %.3g)" % (worst, TOL))


@needs_ld
def test_hindcast_closed_form_equals_real_long_double_prefix_refits(refit_cases):
    for c, K, y in refit_cases:
        core = SC.core_from_matrix(K, y, c.sn, SC.HP, need_inverse=False)
        settings = [lm for lm in SC.HC_SETTINGS + ((2, c.n - 2),) if SC.hc_admissible(c.n, *lm)]
        assert settings
        for lead, mt in settings:
            got = {mode: SC.hc_rows(core, lead, mt, mode) for mode in SC.MODES}
            rows = scored_rows(c.n, lead, mt)
            assert np.array_equal(np.flatnonzero(~np.isnan(got["refit"]["var"].astype(np.float64))), rows)
            assert np.array_equal(np.flatnonzero(~np.isnan(got["fixed"]["mean"].astype(np.float64))), rows)
            for t in rows:
                s = t - lead + 1
                f = H.hp_fit(K[:s, :s], y[:s], c.sn, ks=K[t:t + 1, :s], kss=np.array([K[t, t]], dtype=LD) - LD(c.sn), block=0)
                e = max(float(abs(got["refit"]["mean"][t] - f["mean"][0])) / max(1.0, float(np.max(np.abs(y)))), _rel(got["refit"]["var"][t], f["var"][0]),
                        _rel(got["fixed"]["var"][t], f["var"][0] * core["sigma_f"] / f["sigma_f"]),
                        _rel(got["refit"]["w"][t] * core["sigma_f"], got["fixed"]["var"][t]))
                assert e <= TOL, (c, lead, mt, t, e)
    # exactly one scored row
    assert len(scored_rows(17, 2, 15)) == 1 and len(scored_rows(33, 32, 1)) == 1


@needs_ld
def test_cv_of_block_one_is_loo_in_the_reference():
    for c in SC.TABLE:
        if c.n in (2, 17, 49) and c.N == 17:
            core = SC.reference(c)
            for mode in SC.MODES:
                a, b = SC.cv_rows(core, 1, 0, mode), SC.loo_rows(core, mode)
                # the same arithmetic at block = 1 (Ci = 1 / P_ii by a 1 x 1 factor and its inverse): a few roundings per row, which the
                # "refit" variance's subtraction q - a~_i^2 / P_ii enlarges (21 eps_ld at sn~ = 1e-6) -- TOL, with no condition factor
                e = max(_rel(a["var"], b["var"]), float(np.max(np.abs(a["mean"] - b["mean"]) / np.maximum(1, np.abs(b["mean"])))))
                es = max(abs(float(a[k] - b[k])) / max(1.0, abs(float(b[k]))) for k in ("nlpd", "sse"))
                assert e <= TOL and es <= TOL, (c, mode, e, es)


def test_the_case_table_covers_its_shapes_and_meets_the_condition_cap():
    t = SC.TABLE
    assert {c.n for c in t} == set(SC.ORDERS) and {c.N for c in t} == set(SC.FEATURES)
    for n in SC.ORDERS:
        mine = [c for c in t if c.n == n]
        assert {c.N for c in mine} == set(SC.FEATURES) and {c.m for c in mine} == set(SC.MS)
        assert any(c.expm == "pade" for c in mine)
        for N in SC.FEATURES:       # every (order, N) data set at all four (l, sn~)
            assert sorted((c.ell, c.sn) for c in mine if c.N == N and c.expm == "eigh") == sorted(SC.POINTS)
    assert sum(c.expm == "eigh" for c in t) == 408 and sum(c.expm == "pade" for c in t) == len(SC.ORDERS)
    worst = 0.0
    # the whole grid the table is drawn from -- every (order, N) at all four (l, sn~), eigh and pade -- through the real staging
    seen = {(c.n, c.N): c for c in t}
    count = 0
    for c0 in seen.values():
        for ell, sn in SC.POINTS:
            for expm in ("eigh", "pade"):
                c = c0._replace(ell=ell, sn=sn, expm=expm)
                cd = H.cond2(SC.build(SC.staged(c), ell, sn, SC.F64)[0])
                worst = max(worst, cd)
                count += 1
                assert cd <= SC.COND_CAP, (c, cd)
    for c in SC.EXTRA:
        cd = H.cond2(SC.build(SC.staged(c), c.ell, c.sn, SC.F64)[0])
        assert cd <= SC.COND_CAP, (c, cd)
    print("cond(K~): worst of %d cases %.3g" % (count, worst))
    assert count == 816


def test_every_layout_of_a_batch_is_admissible_for_every_set_of_it():
    B = SC.batches()
    for b in B.values():
        for c in b.cases:
            assert all(SC.cv_admissible(c.n, *bg) for bg in b.cv) and all(SC.hc_admissible(c.n, *lm) for lm in b.hc), (b.name, c)
        assert b.hc and b.one_row in b.hc and any(len(scored_rows(c.n, *b.one_row)) == 1 for c in b.cases)
    full, small = set(SC.CV_LAYOUTS), {(1, 0), (5, 1), (8, 0), (7, 3), (14, 0)}
    assert set(B["mid"].cv) == full and set(B["c16"].cv) == full and set(B["c8"].cv) == full and set(B["s15"].cv) == small
    assert set(B["s2"].cv) == {(1, 0)} and B["b"].cv == () and B["big"].cv == ()
    assert set(B["mid"].hc) >= set(SC.HC_SETTINGS) and set(B["big"].hc) >= set(SC.HC_SETTINGS)
    # each feature chunk actually runs: 32 (kept by the leave-block-out launch), 16, and the launch's own 16 and 8
    assert (B["a"].chunk, B["a"].cv_chunk, B["mid"].chunk, B["mid"].cv_chunk) == (32, 32, 32, 32)
    assert (B["b"].chunk, B["big"].chunk, B["b"].cv_chunk) == (16, 16, None)
    assert (B["c16"].chunk, B["c16"].cv_chunk, B["c8"].chunk, B["c8"].cv_chunk) == (32, 16, 16, 8)
    for b in B.values():
        assert any(c.N > (b.cv_chunk or b.chunk) for c in b.cases) and any(c.expm == "pade" for c in b.cases), b.name


LAYOUT_PROGRAM = r'''
#include <cstdio>
#include <initializer_list>
#include "smallgp_layout.hpp"
using namespace sigp;

int main() {
  const SmallFlavour fl[] = {SmallFlavour::Plain, SmallFlavour::Grad, SmallFlavour::Loo, SmallFlavour::Cv, SmallFlavour::Hindcast};
  std::printf("K %d %d %d %d %ld\n", SM_NMAX, SM_MMAX, SM_CVW, SM_CVP, SM_LDS_MAX);
  for (int f = 0; f < 5; ++f) std::printf("F %d %d %d\n", f, small_out_width(fl[f]), (int)small_has_rows(fl[f]));
  for (int n = 1; n <= SM_NMAX; ++n)
    for (int m = 0; m <= SM_MMAX; ++m) {
      for (int ch : {8, 16, 32})
        for (int f = 0; f < 5; ++f) {
          const SmallLayout l{n, m, ch, fl[f]};
          std::printf("L %d %d %d %d %ld %d %d %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", n, m, ch, f, l.bytes(), l.ldk(), l.lda(), l.Kp(), l.Ac(), l.wk(), l.kss(), l.red(), l.at(),
                      l.Pw(), l.Ww(), l.tv());
        }
      const int up = small_pick_chunk(n, m, SmallFlavour::Plain, 32);
      std::printf("C %d %d %d %d\n", n, m, up, up ? small_pick_chunk(n, m, SmallFlavour::Cv, up) : 0);
    }
  return 0;
}
'''


def test_lds_anchors_of_the_leave_block_out_launch(tmp_path):
    """from SmallLayout::bytes() against 160 KiB - 64: the parent refused n >= 119 (m = 0), 118 (m = 1, 2), 114 (m = 8);
    with the launch's own chunk the limits are 128 (m <= 2), 127 (m = 3 .. 5), 126 (m = 6), 125 (m = 7, 8)"""
    # ``small_cases.lds_bytes`` / ``upload_chunk`` / ``cv_chunk`` restate csrc/smallgp_layout.hpp, which a stand-alone host program sweeps:
    # n = 1 .. 128, m = 0 .. 8, ch in {8, 16, 32}, all five flavours.  The behaviour itself -- accepted, refused, the handle usable
    # afterwards -- is tested through the library on the GPU.
    src = tmp_path / "small_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "small_layout"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc"), "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = {k: [] for k in "KFLC"}
    for line in p.stdout.split("\n"):
        if line:
            rows[line[0]].append([int(x) for x in line.split()[1:]])
    assert rows["K"] == [[128, 8, SC.CV_W, SC.CV_W + 1, SC.LDS_MAX]]
    assert rows["F"] == [[0, 4, 0], [1, 8, 0], [2, 6, 1], [3, 6, 1], [4, 6, 1]]       # plain, gradient, leave-one-out, leave-block-out, hindcast
    assert len(rows["L"]) == 128 * 9 * 3 * 5 and len(rows["C"]) == 128 * 9
    CV = 3
    for n, m, ch, f, size, ldk, lda, Kp, Ac, wk, kss, red, at, Pw, Ww, tv in rows["L"]:
        assert size == SC.lds_bytes(n, m, ch) + (SC.CV_EXTRA if f == CV else 0), (n, m, ch, f)
        assert (ldk, lda) == (n | 1, ch + 1)
        # the offsets the kernel had as literals: red = kss + SM_MMAX, at = red + 16, Pw = at + n + 24 (24 doubles of slack)
        assert (Kp, Ac, wk, kss, red, at, Pw) == (0, (n + 1 + m) * ldk, (n + 1 + m) * ldk + (n + m) * lda, wk + ch, kss + 8, red + 16, at + n + 24), (n, m, ch, f)
        assert (Ww, tv) == (Pw + 32 * 33, Pw + 2 * 32 * 33) and Pw * 8 == SC.lds_bytes(n, m, ch)
        pieces = [(Kp, (n + 1 + m) * ldk), (Ac, (n + m) * lda), (wk, ch), (kss, 8), (red, 16), (at, n)]
        if f == CV:
            pieces += [(Pw, 32 * 33), (Ww, 32 * 33), (tv, 32)]
        pieces.sort()
        assert pieces[0][0] >= 0 and 8 * (pieces[-1][0] + pieces[-1][1]) <= size, (n, m, ch, f)                 # inside bytes() ...
        assert all(a[0] + a[1] <= b[0] for a, b in zip(pieces, pieces[1:])), (n, m, ch, f)                        # ... and disjoint
    for n, m, up, cvc in rows["C"]:
        assert (up or None, cvc or None) == (SC.upload_chunk(n, m), SC.cv_chunk(n, m)), (n, m)
    assert [SC.cv_order_limit(m, before_fix=True) for m in (0, 1, 2, 8)] == [118, 117, 117, 113]
    assert [SC.cv_order_limit(m) for m in range(9)] == [128, 128, 128, 127, 127, 127, 126, 125, 125]
    for n, m in ((128, 0), (128, 2), (127, 3), (125, 8)):
        assert SC.cv_chunk(n, m) == 8 and SC.cv_chunk(n, m, before_fix=True) is None
    for n, m in ((128, 3), (126, 8)):
        assert SC.cv_chunk(n, m) is None and SC.upload_chunk(n, m) == 16


@needs_ld
def test_the_fp64_comparator_error_is_finite_and_non_zero_on_every_case():
    lo, hi = np.inf, 0.0
    for c in SC.TABLE + SC.EXTRA:
        r, f = SC.reference(c), SC.reference(c, SC.F64)
        e = [SC.plain_error(f, r), SC.grad_error(f["grad"], r),
             max(SC.rows_error(SC.loo_rows(f, mode), SC.loo_rows(r, mode), r["y"]) for mode in SC.MODES),
             max(SC.rows_error(SC.hc_rows(f, 1, 1, mode), SC.hc_rows(r, 1, 1, mode), r["y"]) for mode in SC.MODES)]
        assert all(np.isfinite(x) and x > 0 for x in e), (c, e)
        lo, hi = min(lo, min(e)), max(hi, max(e))
    print("fp64 LAPACK against long double: %.3g .. %.3g" % (lo, hi))
