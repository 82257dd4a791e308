"""GPU tier: the MFMA tile primitives, ONE launch at a time, against long double.

Every cubic flop of the library runs through ``gemm_mfma_kernel`` (nine instantiations per element type), ``syrk128_kernel`` (plain, SET,
and the diagonal-skip instantiation with its DG and RD tile forms), ``panel_strip_kernel`` and ``chain_link_kernel``; whole fits reach them
only with the descriptors today's schedules emit and judge them by end-to-end tolerances or by bit-identity of the code with itself.  Here
each launch goes through the debug library's run-and-return entries (include/sigp_debug.h: host operands in, one launch through the
engine's own launcher, the whole output buffer back) and three properties are asserted (tests/tile_cases.py builds the operands, the
footprints and the references; tests/test_tile_walk_host.py checks those helpers and the tile walk on the host):

  value       for every entry the descriptor owns   |C_dev - C_ref| <= (K_eff + 2) u (|A| |B|^T + |C0|)
              u = 2^-53 / 2^-24, K_eff the tile's k span, C_ref the long-double value from the operands as the device got them (fp32
              operands widened).  The forward bound of a length-K inner product in any summation order: no factor, nothing measured.
              Two operand families: standard normal, and a cancelling one (results 1e-6 of the summed magnitudes, one K-slice 1e-8 of
              the rest) under which a dropped or doubled slice is far outside the bound.
  footprint   C starts as a sentinel bit pattern everywhere the descriptor owns nothing (tiles outside the window, above the diagonal of
              a lower walk, above a member's shifted trapezoid, row gaps, member gaps -- and for the SET forms the owned tiles too);
              every such element comes back with the sentinel's bits.  A and B carry NaN wherever no owned tile reads: gaps, and the k
              range a triangular span (ktri) must SKIP rather than multiply.  Exceptions, as documented in syrk128.hpp: the strictly
              upper part of a diagonal tile under the DG form is unspecified (its lower half is checked, and the whole tile with
              diag_tiles = 0); the RD form wants zero rows beyond ride_rows in A, and those rows of C keep their bits.
  same bits   a second identical call returns identical bits; diag_tiles 1 / 0 give the same lower halves and a ride row in the RD
              form / as an ordinary tile the same results, bit for bit (include/sigp.h).

Strip solve, chain link and diagonal block: see their tests.  The last test ties the debug build (ablation branches live) to the product
library: the same fits on both, equal bits.  ``-s`` prints the largest |error| / bound of every case; docs/EXPERIMENTS.md "Tile
primitives" keeps the table.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hp_reference as H
import tile_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = H.LD
NB = 128
BAD_ARG = 2
DTYPE_ID = {"f64": 0, "f32": 1}
DEFAULT_OPTS = (("small_tile_threshold", 320), ("tiny_tile_threshold", 256), ("diag_tiles", 1), ("strip_tri", 1))
_i, _l, _p = C.c_int, C.c_int64, C.c_void_p
_RATIOS = {}


def note(primitive, dtype, what, ratio):
    print("ratio %-18s %s %-70s %.4f" % (primitive, dtype, what, ratio))
    key = (primitive, dtype)
    if ratio > _RATIOS.get(key, (-1.0, ""))[0]:
        _RATIOS[key] = (ratio, what)


class Dbg:
    def __init__(self):
        from seaiceextentforecasting_amd import _lib as L
        self.lib = lib = L.load(debug=True)
        lib.sigp_debug_run_gemm.restype = _i
        lib.sigp_debug_run_gemm.argtypes = [_p, _i, _i, _p, _l, _p, _l, _p, _l, _i, _i, _i, _i, _i, _i, _i, _i, _l, _l, _l, _i, _l, _l, _l, _i, _i, _i, _l, _l, _l]
        lib.sigp_debug_run_strip.restype = _i
        lib.sigp_debug_run_strip.argtypes = [_p, _i, _p, _l, _p, _l, _i, _i, _i, _i, _i, _l, _l, _l, _l]
        lib.sigp_debug_run_link.restype = _i
        lib.sigp_debug_run_link.argtypes = [_p, _i, _p, _l, _i, _p, _p, _i, _i, _l, _l, _l, _l, _l, _l]
        lib.sigp_debug_time_diag.restype = _i
        lib.sigp_debug_time_diag.argtypes = [_p, _p, _i, _i, _p, _p, _p]
        h = _p()
        rc = lib.sigp_create(C.byref(h), 0, 0)
        assert rc == 0, "sigp_create failed (rc = %d)" % rc
        self.h = h

    def option(self, name, value):
        assert self.lib.sigp_set_option(self.h, name.encode(), int(value)) == 0, name

    def error(self):
        m = self.lib.sigp_last_error(self.h)
        return m.decode() if m else ""

    def close(self):
        self.lib.sigp_destroy(self.h)


@pytest.fixture(scope="module")
def dbg():
    d = Dbg()
    yield d
    d.close()
    if _RATIOS:
        print("\nlargest |C_dev - C_ref| / bound per primitive and element type:")
        for (prim, dt), (r, what) in sorted(_RATIOS.items()):
            print("  %-18s %s  %.4f  (%s)" % (prim, dt, r, what))


@pytest.fixture
def options(dbg):
    """set handle options for one test; the defaults come back afterwards"""
    def set_all(pairs):
        for k, v in pairs:
            dbg.option(k, v)
    yield set_all
    set_all(DEFAULT_OPTS)


def ptr(a):
    return None if a is None else a.ctypes.data_as(_p)


def bits(a):
    return a.view(TC.BITS["f64" if a.dtype == np.float64 else "f32"])


def gemm_args(d, **over):
    L, r = TC.layout(d), dict(zip(("r0", "r1", "c0", "c1"), d.win))
    a = dict(cfg=TC.CFGS[d.cfg].id, lda=L.lda, ldb=L.ldb, ldc=L.ldc, K=d.K, lower=d.lower, ktri=d.ktri, batch=d.batch, sA=L.sA, sB=L.sB, sC=L.sC,
             zcount=d.zcount, zA=L.zA, zB=L.zB, zC=L.zC, zshift=d.zshift, ride_bi1=d.ride[0], ride_rows=d.ride[1], a_elems=L.a_elems,
             b_elems=L.b_elems, c_elems=L.c_elems, **r)
    for k, v in over.items():
        a[k] = a[k] + v if k.endswith("_elems") else v
    return a


def run_gemm(dbg, d, ops, **over):
    """one launch: (rc, the whole C buffer afterwards)"""
    a = gemm_args(d, **over)
    out = ops["C"].copy()
    rc = dbg.lib.sigp_debug_run_gemm(dbg.h, DTYPE_ID[d.dtype], a["cfg"], ptr(ops["A"]), a["lda"], ptr(ops["B"]), a["ldb"], ptr(out), a["ldc"], a["K"],
                                     a["r0"], a["r1"], a["c0"], a["c1"], a["lower"], a["ktri"], a["batch"], a["sA"], a["sB"], a["sC"], a["zcount"],
                                     a["zA"], a["zB"], a["zC"], a["zshift"], a["ride_bi1"], a["ride_rows"], a["a_elems"], a["b_elems"], a["c_elems"])
    return rc, out


def primitive_of(d):
    return {"gemm": "gemm_mfma " + d.cfg, "syrk": d.cfg, "auto": "gemm_sub_auto"}[TC.CFGS[d.cfg].kind]


# ---- gemm_mfma_kernel, syrk128_kernel, gemm_sub_auto -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", TC.gemm_cases() + TC.auto_cases(), ids=TC.case_id)
def test_one_launch_value_footprint_same_bits(dbg, options, d):
    options((("diag_tiles", d.diag_tiles),) + tuple(d.opts))
    ops, m = TC.operands(d), TC.masks(d)
    ref, bound = TC.reference(d, ops)
    rc, dev = run_gemm(dbg, d, ops)
    assert rc == 0, dbg.error()
    ratio, moved = TC.judge(d, ops, dev, ref, bound, m)
    note(primitive_of(d), d.dtype, TC.case_id(d), ratio)
    rc, again = run_gemm(dbg, d, ops)
    assert rc == 0, dbg.error()
    assert moved == 0, "%d elements the descriptor does not own changed" % moved
    assert ratio <= 1.0, "largest |C_dev - C_ref| / bound = %.3f" % ratio
    assert np.array_equal(bits(dev), bits(again)), "a second identical launch gave other bits"
    spec = ~m["unspec"]
    if TC.diag_skip_launch(d):
        # the whole diagonal tile with diag_tiles = 0, and the same lower halves bit for bit (include/sigp.h, option diag_tiles)
        d0 = d._replace(diag_tiles=0)
        options((("diag_tiles", 0),))
        rc, full = run_gemm(dbg, d0, ops)
        assert rc == 0, dbg.error()
        m0 = TC.masks(d0)
        if not d.ride[0]:
            assert m0["check"].sum() > m["check"].sum() and not m0["unspec"].any()
        ratio0, moved0 = TC.judge(d0, ops, full, ref, bound, m0)      # (the reference covers whole tiles: only the masks differ)
        note(primitive_of(d), d.dtype, TC.case_id(d0) + " (whole diagonal tiles)", ratio0)
        assert moved0 == 0 and ratio0 <= 1.0, (moved0, ratio0)
        assert np.array_equal(bits(dev)[spec], bits(full)[spec]), "diag_tiles 1 and 0 differ in the lower halves"
        options((("diag_tiles", d.diag_tiles),))
    if d.ride[0]:
        # the ride row as an ordinary block row (what ride_tiles = 0 launches): the same results bit for bit
        rc, plain = run_gemm(dbg, d, ops, ride_bi1=0, ride_rows=0)
        assert rc == 0, dbg.error()
        assert np.array_equal(bits(dev)[spec], bits(plain)[spec]), "the RD form and the ordinary tile differ"
        if TC.diag_skip_launch(d):
            # the RD form neither reads nor writes rows 16 .. of its tiles (syrk128.hpp): the sentinel there stays, and nothing else changes
            rest = TC.ride_rest(d)
            poisoned = dict(ops, C=ops["C"].copy())
            bits(poisoned["C"])[rest] = TC.SENTINEL[d.dtype]
            rc, out = run_gemm(dbg, d, poisoned)
            assert rc == 0, dbg.error()
            assert np.all(bits(out)[rest] == TC.SENTINEL[d.dtype]), "rows 16 .. of a ride-row tile were read or written: the RD form did not run"
            assert np.array_equal(bits(out)[~rest & spec], bits(dev)[~rest & spec])


@pytest.mark.parametrize("what,d,over", TC.refused_cases(), ids=[c[0].replace(" ", "_") for c in TC.refused_cases()])
def test_descriptors_that_leave_the_buffers_are_refused(dbg, what, d, over):
    L = TC.layout(d)
    t = TC.NPT[d.dtype]
    ops = dict(A=np.ones(L.a_elems, t), B=None if d.alias else np.ones(max(L.b_elems, 1), t), C=np.full(L.c_elems, 7.0, t))
    rc, out = run_gemm(dbg, d, ops, **over)
    assert rc == BAD_ARG, (what, rc)
    assert np.all(out == 7.0)
    rc, out = run_gemm(dbg, d, ops)                       # the unchanged descriptor is accepted where it is a valid one
    if not over:
        assert rc == BAD_ARG
    else:
        assert rc == 0, (what, dbg.error())


# ---- panel_strip_kernel ----------------------------------------------------------------------------------------------------------------------
_CHOL = {}


def panel_factor(member):
    """(L [512, 512] long double) of a well-conditioned SPD panel top, cond ~ 34 (a Wishart matrix with twice as many columns as rows); its
    leading blocks are the factors of the narrower panels.  Member 1: rows scaled by powers of two (D L is the exact factor of D T D)."""
    if "L" not in _CHOL:
        rng = np.random.default_rng(4100)
        G = rng.standard_normal((4 * NB, 8 * NB))
        T = G @ G.T / (8 * NB)
        assert H.cond2(T) <= 1e3
        _CHOL["L"] = H.cholesky((T + T.T) / 2)[0]
        _CHOL["D"] = 2.0 ** np.random.default_rng(4101).integers(-2, 3, 4 * NB)
    return _CHOL["L"] if member == 0 else _CHOL["L"] * _CHOL["D"].astype(LD)[:, None]


def inv_block(Ljj):
    return H.forward(Ljj, np.eye(NB, dtype=LD))


def make_mt(member, Wp, t):
    """Mt [Wp 128][Wp 128] rounded to the working type: block row j = [-inv(L_jj) L_j0 .. -inv(L_jj) L_j,j-1 | inv(L_jj) | 0]"""
    Lp = panel_factor(member)[:Wp * NB, :Wp * NB]
    Mt = np.zeros((Wp * NB, Wp * NB), dtype=LD)
    for j in range(Wp):
        r = slice(j * NB, (j + 1) * NB)
        Ij = np.tril(inv_block(Lp[r, r]))
        Mt[r, :j * NB] = -H.hp_matmul(Ij, Lp[r, :j * NB])
        Mt[r, r] = Ij
    return Mt.astype(t)


STRIPS = [("f64", 1, 1, 0, 1, 0), ("f64", 2, 3, 1, 1, 2), ("f64", 4, 1, 2, 2, 0), ("f64", 4, 3, 0, 1, 2), ("f64", 2, 1, 0, 2, 2),
          ("f32", 2, 1, 1, 2, 4), ("f32", 4, 3, 0, 1, 0)]


@pytest.mark.parametrize("dtype,Wp,nstrips,J,members,pad", STRIPS, ids=["%s-Wp%d-strips%d-J%d-members%d-pad%d" % s for s in STRIPS])
def test_strip_solve(dbg, options, dtype, Wp, nstrips, J, members, pad):
    """One workgroup per 128-row strip walks the panel's column blocks: X_j = [X_0 .. X_{j-1} | A_j] Mt_j^T, K_j = 128 (j + 1), the
    earlier X_k read back from memory in the working type.  Reference: the same recurrence in long double with the SAME rounded Mt
    (this tests the kernel, not the conditioning of the panel).  Bound, per column block and propagated through |Mt|:

        b_j = (K_j + 2) u |[X_0 .. X_{j-1} | A_j]| |Mt_j|^T  +  sum_{k < j} b_k |Mt_jk|^T

    (first term: the rounding of block j's own inner products; second: the error already in the operands X_k, carried by the
    product).  Footprint: everything outside the strips' panel columns keeps its sentinel bits; Mt carries NaN right of each block
    row's diagonal block (beyond K_j) and in its gaps, zeros above the diagonal of the diagonal blocks (the full-block instantiation
    multiplies them; strip_tri = 1 skips them: the same bits, include/sigp.h)."""
    t, u = TC.NPT[dtype], LD(TC.UNIT[dtype])
    rb0 = J + Wp
    rows, ld = (rb0 + nstrips) * NB, (J + Wp) * NB + pad
    sM = rows * ld + TC.GAP
    m_elems = (members - 1) * sM + rows * ld + TC.GAP
    ldm = Wp * NB + pad
    sMt = Wp * NB * ldm + TC.GAP
    mt_elems = (members - 1) * sMt + Wp * NB * ldm + TC.GAP
    rng = np.random.default_rng([77, Wp, nstrips, J, members])
    M = np.full(m_elems, TC.SENTINEL[dtype], dtype=TC.BITS[dtype]).view(t)
    Mt = np.full(mt_elems, np.nan, dtype=t)
    own = np.zeros(m_elems, bool)
    ref, bound = np.full(m_elems, np.nan, dtype=LD), np.full(m_elems, np.nan, dtype=LD)
    for b in range(members):
        Mm, Om = TC.view(M, b * sM, rows, ld), TC.view(own, b * sM, rows, ld)
        Rm, Bm = TC.view(ref, b * sM, rows, ld), TC.view(bound, b * sM, rows, ld)
        Tm = TC.view(Mt, b * sMt, Wp * NB, ldm)
        mt = make_mt(b, Wp, t)
        for j in range(Wp):
            Tm[j * NB:(j + 1) * NB, :(j + 1) * NB] = mt[j * NB:(j + 1) * NB, :(j + 1) * NB]
        rs, cs = slice(rb0 * NB, rows), slice(J * NB, (J + Wp) * NB)
        Mm[rs, cs] = rng.standard_normal((nstrips * NB, Wp * NB)).astype(t)
        Om[rs, cs] = True
        S, Sb = Mm[rs, cs].astype(LD), np.zeros((nstrips * NB, Wp * NB), dtype=LD)
        for j in range(Wp):
            k = (j + 1) * NB
            mj = mt[j * NB:(j + 1) * NB, :k].astype(LD)
            X = H.hp_matmul(S[:, :k], mj.T)
            Sb[:, j * NB:k] = (k + 2) * u * H.hp_matmul(np.abs(S[:, :k]), np.abs(mj).T) + H.hp_matmul(Sb[:, :j * NB], np.abs(mj[:, :j * NB]).T)
            S[:, j * NB:k] = X
        Rm[rs, cs], Bm[rs, cs] = S, Sb
    results = {}
    for tri in (1, 0, 1):
        options((("strip_tri", tri),))
        out = M.copy()
        rc = dbg.lib.sigp_debug_run_strip(dbg.h, DTYPE_ID[dtype], ptr(out), ld, ptr(Mt), ldm, rb0, nstrips, J, Wp, members, sM, sMt, m_elems, mt_elems)
        assert rc == 0, dbg.error()
        moved = int(np.count_nonzero(bits(out)[~own] != bits(M)[~own]))
        e = np.abs(out[own].astype(LD) - ref[own])
        ratio = float(np.max(np.where(np.isfinite(e), e / bound[own], np.inf)))
        note("panel_strip" + ("" if tri else " full"), dtype, "Wp %d strips %d J %d members %d pad %d" % (Wp, nstrips, J, members, pad), ratio)
        assert moved == 0, "%d elements outside the strips' panel columns changed" % moved
        assert ratio <= 1.0, "strip_tri = %d: largest |X_dev - X_ref| / bound = %.3f" % (tri, ratio)
        if tri in results:
            assert np.array_equal(bits(out), bits(results[tri])), "a second identical launch gave other bits"
        results[tri] = out
    assert np.array_equal(bits(results[0]), bits(results[1])), "strip_tri 1 and 0 differ"
    # refusals: one element short, a leading dimension narrower than the panel, more strips than rows
    bad = lambda *a: dbg.lib.sigp_debug_run_strip(dbg.h, DTYPE_ID[dtype], ptr(M.copy()), *a)   # noqa: E731
    assert bad(ld, ptr(Mt), ldm, rb0, nstrips, J, Wp, members, sM, sMt, (members - 1) * sM + rows * ld - pad - 1, mt_elems) == BAD_ARG
    assert bad((J + Wp) * NB - TC.NE[dtype], ptr(Mt), ldm, rb0, nstrips, J, Wp, members, sM, sMt, m_elems, mt_elems) == BAD_ARG
    assert bad(ld, ptr(Mt), ldm, rb0, nstrips + 1, J, Wp, members, sM, sMt, m_elems, mt_elems) == BAD_ARG
    assert bad(ld, ptr(Mt), ldm, rb0, nstrips, J, Wp, members, sM, sMt, m_elems, (members - 1) * sMt + Wp * NB * ldm - pad - 1) == BAD_ARG


# ---- chain_link_kernel -------------------------------------------------------------------------------------------------------------------------
LINKS = [("f64", 0, 0, 1, 0), ("f64", 1, 1, 2, 2), ("f64", 0, 3, 1, 2), ("f64", 1, 3, 2, 0), ("f32", 0, 1, 2, 4), ("f32", 1, 3, 1, 0)]


@pytest.mark.parametrize("dtype,c,rows_ride,members,pad", LINKS, ids=["%s-c%d-ride%d-members%d-pad%d" % s for s in LINKS])
def test_chain_link(dbg, dtype, c, rows_ride, members, pad):
    """The fused link against the two operations it replaces (chain_link.hpp), K = 128 both:
    the column solve  L[c+1.., c] = A inv(L_cc)^T  -- block row c+1 into the scratch block (the matrix keeps the unsolved block: other
    workgroups of the launch still read it), the rows_ride blocks below it in place -- with bound (K + 2) u |A| |Linv|^T; and the update
    of block (c+1, c+1), C -= S S^T over the 36 16 x 16 tiles of its lower triangle with S the solved block AS THE DEVICE FORMED IT
    (its scratch output, widened), bound (K + 2) u (|S| |S|^T + |C0|).  The 28 tiles above the diagonal carry the sentinel and keep it,
    as does everything else in the matrix.  The scratch block and the ride rows equal the stand-alone column solve (32x128 SET tiles,
    launch_column_solve) bit for bit."""
    t, u = TC.NPT[dtype], LD(TC.UNIT[dtype])
    rows, ld = (c + 2 + rows_ride) * NB, (c + 2) * NB + pad
    sM = rows * ld + TC.GAP
    m_elems = (members - 1) * sM + rows * ld + TC.GAP
    sL = sS = NB * NB + TC.GAP
    l_elems = (members - 1) * sL + NB * NB
    rng = np.random.default_rng([91, c, rows_ride, members])
    M = np.full(m_elems, TC.SENTINEL[dtype], dtype=TC.BITS[dtype]).view(t)
    Linv = np.full(l_elems, np.nan, dtype=t)
    scratch0 = np.full(l_elems, TC.SENTINEL[dtype], dtype=TC.BITS[dtype]).view(t)
    tiles16 = np.kron(np.tril(np.ones((8, 8), bool)), np.ones((16, 16), bool))          # the 36 tiles of the lower triangle
    for b in range(members):
        Mm = TC.view(M, b * sM, rows, ld)
        Mm[(c + 1) * NB:, c * NB:(c + 1) * NB] = rng.standard_normal((rows - (c + 1) * NB, NB)).astype(t)
        Cd = Mm[(c + 1) * NB:(c + 2) * NB, (c + 1) * NB:(c + 2) * NB]
        Cd[tiles16] = rng.standard_normal(int(tiles16.sum())).astype(t)
        Linv[b * sL:b * sL + NB * NB] = np.tril(inv_block(panel_factor(b)[:NB, :NB])).astype(t).reshape(-1)
    out, scr = M.copy(), scratch0.copy()
    call = lambda o, s: dbg.lib.sigp_debug_run_link(dbg.h, DTYPE_ID[dtype], ptr(o), ld, c, ptr(Linv), ptr(s), rows_ride, members, sM, sL, sS, m_elems,   # noqa: E731
                                                    l_elems, l_elems)
    assert call(out, scr) == 0, dbg.error()
    out2, scr2 = M.copy(), scratch0.copy()
    assert call(out2, scr2) == 0, dbg.error()
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(scr), bits(scr2)), "a second identical launch gave other bits"
    touched = np.zeros(m_elems, bool)
    worst_solve = worst_upd = 0.0
    for b in range(members):
        Mm, Om, Tm = TC.view(M, b * sM, rows, ld), TC.view(out, b * sM, rows, ld), TC.view(touched, b * sM, rows, ld)
        Li = Linv[b * sL:b * sL + NB * NB].reshape(NB, NB)
        A = Mm[(c + 1) * NB:, c * NB:(c + 1) * NB]
        Xref = H.hp_matmul(A, Li.T)
        Xb = (NB + 2) * u * H.hp_matmul(np.abs(A), np.abs(Li).T)
        S = scr[b * sS:b * sS + NB * NB].reshape(NB, NB)
        Xdev = np.vstack([S, Om[(c + 2) * NB:, c * NB:(c + 1) * NB]])
        e = np.abs(Xdev.astype(LD) - Xref)
        worst_solve = max(worst_solve, float(np.max(np.where(np.isfinite(e), e / Xb, np.inf))))
        Tm[(c + 2) * NB:, c * NB:(c + 1) * NB] = True
        C0 = Mm[(c + 1) * NB:(c + 2) * NB, (c + 1) * NB:(c + 2) * NB]
        Cref = C0.astype(LD)[tiles16] - H.hp_matmul(S, S.T)[tiles16]
        Cb = (NB + 2) * u * (H.hp_matmul(np.abs(S), np.abs(S).T)[tiles16] + np.abs(C0[tiles16]))
        e = np.abs(Om[(c + 1) * NB:(c + 2) * NB, (c + 1) * NB:(c + 2) * NB][tiles16].astype(LD) - Cref)
        worst_upd = max(worst_upd, float(np.max(np.where(np.isfinite(e), e / Cb, np.inf))))
        Tm[(c + 1) * NB:(c + 2) * NB, (c + 1) * NB:(c + 2) * NB] = tiles16
        # the stand-alone column solve of the same rows: one launch of 32-row tiles
        nrow = A.shape[0]
        Cs = np.zeros(nrow * NB, t)
        rc = dbg.lib.sigp_debug_run_gemm(dbg.h, DTYPE_ID[dtype], TC.CFGS["32x128_set"].id, ptr(np.ascontiguousarray(A)), NB, ptr(np.ascontiguousarray(Li)), NB, ptr(Cs), NB,
                                         NB, 0, nrow // 32, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, nrow * NB, NB * NB, nrow * NB)
        assert rc == 0, dbg.error()
        assert np.array_equal(bits(Cs), bits(np.ascontiguousarray(Xdev).reshape(-1))), "the fused link and the stand-alone column solve differ"
    note("chain_link solve", dtype, "c %d ride %d members %d pad %d" % (c, rows_ride, members, pad), worst_solve)
    note("chain_link update", dtype, "c %d ride %d members %d pad %d" % (c, rows_ride, members, pad), worst_upd)
    moved = int(np.count_nonzero(bits(out)[~touched] != bits(M)[~touched]))
    sgap = np.ones(l_elems, bool)
    for b in range(members):
        sgap[b * sS:b * sS + NB * NB] = False
    moved += int(np.count_nonzero(bits(scr)[sgap] != bits(scratch0)[sgap]))
    assert moved == 0, "%d elements outside the link's outputs changed" % moved
    assert worst_solve <= 1.0 and worst_upd <= 1.0, (worst_solve, worst_upd)
    assert dbg.lib.sigp_debug_run_link(dbg.h, DTYPE_ID[dtype], ptr(M.copy()), ld, c, ptr(Linv), ptr(scratch0.copy()), rows_ride + 1, members, sM, sL, sS,
                                       m_elems, l_elems, l_elems) == BAD_ARG
    assert dbg.lib.sigp_debug_run_link(dbg.h, DTYPE_ID[dtype], ptr(M.copy()), ld, c, ptr(Linv), ptr(scratch0.copy()), rows_ride, members, sM, sL, sS,
                                       m_elems, l_elems - 1, l_elems) == BAD_ARG


# ---- potrf_diag_kernel -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 6, 10], ids=["cond1e2", "cond1e6", "cond1e10"])
def test_diagonal_block(dbg, p):
    """One 128 x 128 block through sigp_debug_time_diag (reps = 1, no phase switched off): L and inv(L) of a random SPD matrix with
    spectrum logspace(0, -p).  ||L L^T - A||_F / ||A||_F and ||Linv L - I||_F as ratios to LAPACK's on the same matrix
    (np.linalg.cholesky, scipy solve_triangular), the form and the margin (16) of tests/test_hip_conditioning.py:
    q_dev <= 16 max(q_lapack, u).  The strictly upper part of Linv is exactly zero."""
    from scipy.linalg import solve_triangular
    A = H._spectral(NB, np.logspace(0.0, -float(p), NB), 9000 + p)
    Ld, Li, ms = np.zeros((NB, NB)), np.full((NB, NB), np.nan), C.c_double(0)
    rc = dbg.lib.sigp_debug_time_diag(dbg.h, ptr(A), 0, 1, C.byref(ms), ptr(Ld), ptr(Li))
    assert rc == 0, dbg.error()
    Ld = np.tril(Ld)
    Ll = np.linalg.cholesky(A)
    Lil = solve_triangular(Ll, np.eye(NB), lower=True)

    def inv_res(Linv, Lf):
        R = H.hp_matmul(Linv, Lf) - np.eye(NB, dtype=LD)
        return float(np.sqrt(np.sum(R * R)))

    rho_d, rho_l = H.rho(Ld, A), H.rho(Ll, A)
    inv_d, inv_l = inv_res(Li, Ld), inv_res(Lil, Ll)
    print("diag block cond 1e%d: rho dev %.3e lapack %.3e (ratio %.2f)   ||Linv L - I||_F dev %.3e lapack %.3e (ratio %.2f)"
          % (p, rho_d, rho_l, rho_d / max(rho_l, H.U), inv_d, inv_l, inv_d / max(inv_l, H.U)))
    assert np.all(np.triu(Li, 1) == 0.0), "the strictly upper part of Linv is not exactly zero"
    assert rho_d <= 16.0 * max(rho_l, H.U), (rho_d, rho_l)
    assert inv_d <= 16.0 * max(inv_l, H.U), (inv_d, inv_l)


# ---- the debug build against the product build ---------------------------------------------------------------------------------------------------
def run_fits(path):
    """three fits through the ordinary Python surface, results to an .npz (the child process runs this on libsigp_debug.so)"""
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    res = {}

    def single(tag, n, seed, dtype, **kw):
        X, y, Xs = O.synthetic_problem(n, 8, seed, m=2)
        with GPR(kernel="rbf", dtype=dtype, **kw) as gp:
            gp.fit(X, y, np.sqrt(8.0), 1e-2, Xs=Xs)
            mu, var = gp.predict(Xs)
            res.update({tag + "_L": gp.L_tilde_, tag + "_nlml": np.float64(gp.nlml_), tag + "_mean": np.asarray(mu), tag + "_var": np.asarray(var)})

    single("n300_f64", 300, 31, "f64")
    single("n300_f32", 300, 31, "f32")
    single("n1100_strips", 1100, 32, "f64", outer_blocks=4, panel_mode="strips")
    P = [O.synthetic_problem(700, 8, 33 + i, m=2) for i in range(3)]                    # a lockstep group of 3, two ride rows each
    with GPR(kernel="rbf") as gp:
        r = gp.fit_batch(np.stack([q[0] for q in P]), np.stack([q[1] for q in P]), np.stack([q[2] for q in P]), np.sqrt(8.0) * np.array([1.0, 1.1, 0.9]),
                         np.array([1e-2, 2e-2, 5e-3]), group=3)
    assert np.all(r["info"] == 0)
    res.update({"batch_nlml": r["nlml"], "batch_sigma_f": r["sigma_f"], "batch_mean": r["mean"], "batch_var": r["var"]})
    np.savez(path, **res)


def test_debug_library_computes_what_the_product_library_computes(tmp_path):
    """libsigp_debug.so compiles the same kernels with the ablation branches live (-DSIGP_DEBUG_TOOLS); everything above was measured on
    it.  The same fits -- n = 300 (fp64 and fp32), n = 1100 with four-block outer panels and strip-solved panels, a lockstep group of 3
    at n = 700 -- in a fresh process on the debug library and here on libsigp.so: factor, nlML, means, variances, equal bits."""
    out_dbg, out_prod = str(tmp_path / "debug.npz"), str(tmp_path / "product.npz")
    env = dict(os.environ, SIGP_USE_DEBUG_LIB="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_hip_tile_primitives as T; T.run_fits(%r)" % (os.path.join(ROOT, "tests"), ROOT, out_dbg)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    assert os.environ.get("SIGP_USE_DEBUG_LIB") != "1", "this process must run the product library"
    run_fits(out_prod)
    a, b = np.load(out_dbg), np.load(out_prod)
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 16
    for k in a.files:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s differs between libsigp_debug.so and libsigp.so" % k
