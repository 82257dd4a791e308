"""Host tier of the fp32 solve tests: the helpers of tests/solve_cases.py against plain loops, and the condition on the cases of
tests/test_hip_f32_refinement.py -- the reference refinement (fp32 LAPACK factor, fp32 substitution, long-double residual) must itself
contract by at least a factor 10 per step until it reaches the rounding floor of an fp64 residual, so that "the device contracts as the
reference does" is never asserted on a case where the reference has stalled.  No GPU."""
import numpy as np
import pytest

import hp_reference as H
import solve_cases as SC
import tile_cases as TC

LD = H.LD
needs_ld = pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")


# ---- the block solves, restated ---------------------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("n", [300, 2400, 4100])
def test_block_solve_restatement_equals_substitution(n):
    """per big block a product with the ``strtri`` inverse, then one update, on a random well-conditioned triangle (unit-scale diagonal,
    off-diagonal entries N(0, 1/n)): both routes in fp32 arithmetic, both measured against long-double substitution as the GPU tier
    measures the device -- the restatement's error is within the project's margin of substitution's, and both are fp32 rounding"""
    rng = np.random.default_rng(8800 + n)
    L = np.tril(rng.standard_normal((n, n)) / np.sqrt(n), -1)
    L[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    L = L.astype(np.float32)
    inv = SC.block_inverses(L)
    assert sorted(inv) == [c0 for c0, _ in SC.big_blocks(n)]
    B = rng.standard_normal((n, 4)).astype(np.float32)
    hp = {0: SC.hp_substitution(L, B, 0), 1: SC.hp_substitution(L, B, 1)}
    hp[2] = SC.hp_substitution(L, hp[0], 1)
    for which in (0, 1, 2):
        a, b = SC.restatement(L, inv, B, which), SC.substitution(L, B, which)
        assert a.dtype == np.float32 and b.dtype == np.float32
        scale = float(np.max(np.abs(hp[which])))
        e_rest, e_sub = H.err(a, hp[which]) / scale, H.err(b, hp[which]) / scale
        print("n=%d which=%d: restatement %.3e  substitution %.3e" % (n, which, e_rest, e_sub))
        assert e_rest <= SC.BOUND * max(e_sub, 2.0 ** -24) and e_sub <= SC.BOUND * max(e_rest, 2.0 ** -24), (which, e_rest, e_sub)
        assert max(e_rest, e_sub) <= 1e-4                         # 2^-24 sqrt(n) cond_2(L) <= 6e-8 * 64 * 20 here; a wrong or missing block gives O(1)


@needs_ld
def test_blocked_long_double_substitution_is_substitution():
    rng = np.random.default_rng(8801)
    n = 300
    L = (np.tril(rng.standard_normal((n, n)) / np.sqrt(n), -1) + np.diag(rng.uniform(1.0, 2.0, n))).astype(np.float32)
    B = rng.standard_normal((n, 3)).astype(np.float32)
    Ll = L.astype(LD)
    plain = {0: H.forward(Ll, B), 1: H.backward(Ll, B)}
    plain[2] = H.backward(Ll, plain[0])
    for which in (0, 1, 2):
        got = SC.hp_substitution(L, B, which, block=64)
        assert float(np.max(np.abs(got - plain[which]))) <= 1e-16 * float(np.max(np.abs(plain[which])))


# ---- the reference refinement -------------------------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("kind,n,level", SC.REFINE_CASES)
def test_reference_refinement_contracts_on_every_gpu_case(kind, n, level):
    K = SC.host_matrix(kind, n, level)
    y = SC.problem(n)[1]
    xs, rhos = SC.reference_sequence(K, y)
    floor = SC.residual_floor(K, xs[-1], y)
    print("\nreference %s n=%d sn~=%g: rho_k = %s  floor %.2e" % (kind, n, level, " ".join("%.2e" % r for r in rhos), floor))
    assert len(rhos) == SC.STEPS + 1 and rhos[0] <= 1e-1
    assert SC.contracts(rhos, floor), rhos
    # the yardstick of the forward error: LAPACK's fp64 solution refined in long double solves the system to the floor
    x = SC.exact_solution(K, y)
    assert SC.residual(np.asarray(K, dtype=LD), x, y)[1] <= floor


# ---- ownership and addresses of single launches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [d for d in SC.rowdot_cases() + SC.coldot_cases() if d.n * d.K <= 300 * 300], ids=SC.launch_id)
def test_launch_masks_agree_with_an_element_loop(d):
    """(the launches with K = 2048 go through the same vectorised code; the element loop keeps to the small ones)"""
    L, m = SC.launch_layout(d), SC.launch_masks(d)
    ne = TC.NE[d.dtype]
    for s in (L.ld, L.ldzin, L.sM, L.sZi, L.sZo) + (() if d.pm_pw else (L.ldzout,)):
        assert s % ne == 0
    own, readM, readZ = np.zeros(L.zout_elems, bool), np.zeros(L.m_elems, bool), np.zeros(L.zin_elems, bool)
    for b in range(d.members):
        for j in range(d.n):
            klo, khi = SC.k_range(d, j)
            assert 0 <= klo < khi <= d.K
            for r in range(d.nrhs):
                i = b * L.sZo + SC.out_index(d, L, r, j)
                assert 0 <= i < L.zout_elems - SC.GAP and not own[i]               # inside the member's block; no entry written twice
                assert i == m["own_index"][b, r, j]
                own[i] = True
                for k in range(klo, khi):
                    readZ[b * L.sZi + r * L.ldzin + k] = True
            for k in range(klo, khi):
                readM[b * L.sM + (j * L.ld + k if d.kernel == "rowdot" else k * L.ld + j)] = True
    assert np.array_equal(own, m["own"]) and np.array_equal(readM, m["readM"]) and np.array_equal(readZ, m["readZ"])
    if d.pm_pw:
        g = d.j_off + np.arange(d.n)
        assert L.panels == g.max() // d.pm_pw + 1
        for r in range(d.nrhs):                                                    # panel p holds [4][pm_pw]: row r of panel p starts at (4 p + r) pm_pw
            assert np.array_equal(m["own_index"][0, r], (4 * (g // d.pm_pw) + r) * d.pm_pw + g % d.pm_pw)


def test_launch_case_lists_cover_what_they_claim():
    rows, cols = SC.rowdot_cases(), SC.coldot_cases()
    for dt in ("f32", "f64"):
        step, ne, cw = 64 * TC.NE[dt], TC.NE[dt], 16 * TC.NE[dt]
        r = [d for d in rows if d.dtype == dt]
        assert {step, step + ne, 2048} <= {d.K for d in r}
        assert {(k, n) for k in (1, 2) for n in (4, 5, 129)} <= {(d.kmode, d.n) for d in r}
        assert {1, 2, 3, 4} <= {d.nrhs for d in r} and {0, 1} <= {d.sub for d in r} and any(d.zadd for d in r)
        assert any(d.pm_pw == 256 and d.j_off < 256 < d.j_off + d.n for d in r) and any(d.members == 2 for d in r) and any(d.pad for d in r)
        assert any(d.family == "cancel" for d in r)
        c = [d for d in cols if d.dtype == dt]
        assert {cw, cw + ne, 2048} <= {d.n for d in c} and {16, 128, 200, 2048} <= {d.K for d in c}
        assert {1, 2, 3, 4} <= {d.nrhs for d in c} and any(d.pad for d in c) and any(d.family == "cancel" for d in c)


@needs_ld
def test_launch_reference_and_judge_on_a_numpy_launch():
    """the reference, the bound and ``launch_judge`` on launches computed by NumPy in the working type: inside the bound, nothing moved; a
    dropped k-slice, a write outside the owned entries and a NaN are each caught"""
    for d in (SC.launch(kernel="rowdot", n=9, K=260, kmode=2, nrhs=3, sub=1, zadd=True, family="cancel"),
              SC.launch(kernel="rowdot", n=12, K=256, nrhs=2, pm_pw=256, j_off=250),
              SC.launch(kernel="coldot", dtype="f64", n=34, K=200, nrhs=2, family="cancel", pad=2)):
        ops, m, L, t = SC.launch_operands(d), SC.launch_masks(d), SC.launch_layout(d), TC.NPT[d.dtype]
        ref, bound = SC.launch_reference(d, ops)
        assert np.all(np.isfinite(ref.astype(np.float64))) and np.all(bound > 0)
        P = SC.launch_products(d, ops)[0].astype(t)
        reads_out = d.kernel == "coldot" or d.sub
        val = (ops["out0"].astype(t) - P if reads_out else P).astype(t)
        dev = ops["Zout"].copy()
        dev[m["own_index"].reshape(-1)] = val.reshape(-1)
        ratio, moved = SC.launch_judge(d, ops, dev, ref, bound, m)
        assert ratio <= 1.0 and moved == 0, (d, ratio, moved)
        bad = dev.copy()
        bad[np.flatnonzero(~m["own"])[0]] = 1.0
        assert SC.launch_judge(d, ops, bad, ref, bound, m)[1] == 1
        bad = dev.copy()
        bad[m["own_index"][0, 0, d.n - 1]] = np.nan
        assert SC.launch_judge(d, ops, bad, ref, bound, m)[0] == np.inf
        # drop the first vector of every k range: the cancelling family's results move by far more than the bound
        ne = TC.NE[d.dtype]
        ops2 = dict(ops, M=ops["M"].copy())
        Mm = TC.view(ops2["M"], 0, L.m_rows, L.ld)
        for j in range(d.n):
            klo = SC.k_range(d, j)[0]
            if d.kernel == "rowdot":
                Mm[j, klo:klo + ne] = 0
            else:
                Mm[:ne, j] = 0
        P2 = SC.launch_products(d, ops2)[0].astype(t)
        bad = ops["Zout"].copy()
        bad[m["own_index"].reshape(-1)] = (ops["out0"].astype(t) - P2 if reads_out else P2).astype(t).reshape(-1)
        assert SC.launch_judge(d, ops, bad, ref, bound, m)[0] > 1.0
