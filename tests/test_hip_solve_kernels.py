"""GPU tier: the quadratic solve kernels ONE launch at a time, and the fp32 engine's block solves ONE call at a time, against long double.

``rowdot_kernel`` and ``coldot_kernel`` (csrc/kernels_misc.hpp) carry every triangular solve of the fp32 engine's refinement and of the
sharded drivers; whole fits reach them only through a refinement that forgives its preconditioner (tests/test_hip_f32_refinement.py), and
``rowdot_kernel<double>``, ``Zadd``, the panel-major output and an arbitrary column count of ``coldot`` only through the sharded drivers.
Here each launch goes through the debug library's run-and-return entries (include/sigp_debug.h) on operands built by
tests/solve_cases.py (the host tier checks those helpers):

  value        every owned entry within (K_eff + 3) u (|Zin + Zadd| |M| + |out0|) of the long-double value -- K_eff the number of terms of the
               entry's k range, out0 the prior content where the launch reads it (sub = 1; always for coldot).  The forward bound of an inner
               product in ANY summation order, fused or not (+ 1 for the rounding of Zin + Zadd, + 1 for the subtraction): no measured factor.
               Standard-normal operands, and a cancelling family (prior content = the product to 1e-6, one k-slice 1e-8 of the rest).
  reads        NaN in every element of Mx, Zin and Zadd outside the k range of the row being formed -- the elements that share a 16-byte
               vector with the first or last one in range among them --, beyond K, in right-hand sides >= nrhs and between members: the
               kernels SELECT, they do not multiply, so no NaN may reach an output.
  writes       everything the descriptor does not own keeps its sentinel bits: right-hand sides >= nrhs, columns outside [0, n), the gaps
               of a padded leading dimension, the other rows and panels of a panel-major output, the space between members.
  same bits    a second identical call returns identical bits.

Then the block solves on real factors (``sigp_debug_f32_solve``: f32_block_forward, f32_block_backward, both) against long-double substitution
on the device's own factor, with two fp32 references on that factor (LAPACK substitution; a NumPy restatement of the engine's algorithm), and
the explicit inverses of the 2048-column diagonal blocks (``sigp_debug_f32_get_inverse``) against LAPACK's ``strtri`` -- this separates the
quality of the solves from the quality of the factor, which the refinement tests cannot.  ``-s`` prints every figure;
docs/EXPERIMENTS.md "fp32 solves" keeps the table.
"""
import ctypes as C

import numpy as np
import pytest

import hp_reference as H
import solve_cases as SC
import tile_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")]

LD = H.LD
NB = SC.NB
BAD_ARG = 2
DTYPE_ID = {"f64": 0, "f32": 1}
KERNEL_ID = {"rbf": 1, "matern52": 2}
_i, _l, _p = C.c_int, C.c_int64, C.c_void_p
_RATIOS = {}


def note(what, dtype, case, ratio):
    print("ratio %-8s %s %-70s %.4f" % (what, dtype, case, ratio))
    if ratio > _RATIOS.get((what, dtype), (-1.0, ""))[0]:
        _RATIOS[(what, dtype)] = (ratio, case)


def ptr(a):
    return None if a is None else a.ctypes.data_as(_p)


def bits(a):
    return a.view(TC.BITS["f64" if a.dtype == np.float64 else "f32"])


class Dbg:
    """libsigp_debug.so: the run-and-return entries, and the plain C ABI for fp32 fits on handles those entries can look into"""

    def __init__(self):
        from seaiceextentforecasting_amd import _lib as L
        self.lib = lib = L.load(debug=True)
        lib.sigp_debug_run_rowdot.restype = _i
        lib.sigp_debug_run_rowdot.argtypes = [_p, _i, _p, _l, _i, _i, _i, _p, _l, _p, _l, _i, _i, _p, _i, _i, _i, _l, _l, _l, _l, _l, _l]
        lib.sigp_debug_run_coldot.restype = _i
        lib.sigp_debug_run_coldot.argtypes = [_p, _i, _p, _l, _i, _i, _p, _l, _p, _l, _i, _l, _l, _l]
        lib.sigp_debug_f32_solve.restype = _i
        lib.sigp_debug_f32_solve.argtypes = [_p, _i, _p, _l, _i]
        lib.sigp_debug_f32_get_inverse.restype = _i
        lib.sigp_debug_f32_get_inverse.argtypes = [_p, _i, _p]
        self.h = self.create(0)
        self.fits = {}

    def create(self, dtype):
        h = _p()
        rc = self.lib.sigp_create(C.byref(h), 0, dtype)
        assert rc == 0, "sigp_create failed (rc = %d)" % rc
        return h

    def error(self, h=None):
        m = self.lib.sigp_last_error(h or self.h)
        return m.decode() if m else ""

    def f32_fit(self, kind, n, level=1e-1):
        """an fp32 fit of solve_cases.problem(n) on a handle of its own (kept): dict(h, L32 -- the device's factor, whose values are fp32)"""
        key = (kind, n, level)
        if key not in self.fits:
            from seaiceextentforecasting_amd import _lib as L
            X, y, _ = SC.problem(n)
            X, y = L.f64(X, 2), L.f64(y, 1)
            h = self.create(1)
            out, mean, var = np.zeros(4), np.zeros(1), np.zeros(1)
            assert self.lib.sigp_set_train(h, L.ptr(X), n, X.shape[1], X.shape[1], L.ptr(y)) == 0, self.error(h)
            assert self.lib.sigp_fit_predict(h, KERNEL_ID[kind], SC.ELL, level, None, 0, L.ptr(out), L.ptr(mean), L.ptr(var)) == 0, self.error(h)
            Lf = np.zeros((n, n))
            assert self.lib.sigp_get_matrix(h, 1, L.ptr(Lf), n) == 0, self.error(h)
            L32 = np.tril(Lf).astype(np.float32)
            assert np.array_equal(L32.astype(np.float64), np.tril(Lf))              # the fp32 engine's factor: its values ARE fp32 numbers
            self.fits[key] = dict(h=h, L32=L32)
        return self.fits[key]

    def close(self):
        for f in self.fits.values():
            self.lib.sigp_destroy(f["h"])
        self.lib.sigp_destroy(self.h)


@pytest.fixture(scope="module")
def dbg():
    d = Dbg()
    yield d
    d.close()
    if _RATIOS:
        print("\nlargest figure per kernel and element type:")
        for (what, dt), (r, case) in sorted(_RATIOS.items()):
            print("  %-8s %s  %.4f  (%s)" % (what, dt, r, case))


def launch_args(d, **over):
    L = SC.launch_layout(d)
    a = dict(n=d.n, K=d.K, kmode=d.kmode, nrhs=d.nrhs, sub=d.sub, pm_pw=d.pm_pw, j_off=d.j_off, members=d.members, ld=L.ld, ldzin=L.ldzin, ldzout=L.ldzout,
             sM=L.sM, sZi=L.sZi, sZo=L.sZo, m_elems=L.m_elems, zin_elems=L.zin_elems, zout_elems=L.zout_elems)
    for k, v in over.items():
        a[k] = a[k] + v if k.endswith("_elems") else v
    return a


def run_launch(dbg, d, ops, **over):
    """one launch: (rc, the whole Zout buffer afterwards)"""
    a = launch_args(d, **over)
    out = ops["Zout"].copy()
    if d.kernel == "rowdot":
        rc = dbg.lib.sigp_debug_run_rowdot(dbg.h, DTYPE_ID[d.dtype], ptr(ops["M"]), a["ld"], a["n"], a["K"], a["kmode"], ptr(ops["Zin"]), a["ldzin"], ptr(out), a["ldzout"],
                                           a["nrhs"], a["sub"], ptr(ops["Zadd"]), a["pm_pw"], a["j_off"], a["members"], a["sM"], a["sZi"], a["sZo"], a["m_elems"],
                                           a["zin_elems"], a["zout_elems"])
    else:
        rc = dbg.lib.sigp_debug_run_coldot(dbg.h, DTYPE_ID[d.dtype], ptr(ops["M"]), a["ld"], a["n"], a["K"], ptr(ops["Zin"]), a["ldzin"], ptr(out), a["ldzout"], a["nrhs"],
                                           a["m_elems"], a["zin_elems"], a["zout_elems"])
    return rc, out


# ---- rowdot_kernel, coldot_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", SC.rowdot_cases() + SC.coldot_cases(), ids=SC.launch_id)
def test_one_launch_value_reads_writes_same_bits(dbg, d):
    ops, m = SC.launch_operands(d), SC.launch_masks(d)
    assert np.isnan(ops["M"]).any() and np.isnan(ops["Zin"]).any()                      # (every case has gaps the launch must not use)
    ref, bound = SC.launch_reference(d, ops)
    rc, dev = run_launch(dbg, d, ops)
    assert rc == 0, dbg.error()
    ratio, moved = SC.launch_judge(d, ops, dev, ref, bound, m)
    note(d.kernel, d.dtype, SC.launch_id(d), ratio)
    rc, again = run_launch(dbg, d, ops)
    assert rc == 0, dbg.error()
    assert moved == 0, "%d elements the descriptor does not own changed" % moved
    assert ratio <= 1.0, "largest |Z_dev - Z_ref| / bound = %.3f (inf: a NaN reached an output)" % ratio
    assert np.array_equal(bits(dev), bits(again)), "a second identical launch gave other bits"


@pytest.mark.parametrize("what,d,over", SC.refused_launches(), ids=[c[0].replace(" ", "_") for c in SC.refused_launches()])
def test_launches_that_leave_the_buffers_are_refused(dbg, what, d, over):
    L, t = SC.launch_layout(d), TC.NPT[d.dtype]
    ops = dict(M=np.ones(L.m_elems, t), Zin=np.ones(L.zin_elems, t), Zadd=None, Zout=np.full(L.zout_elems, 7.0, t))
    rc, out = run_launch(dbg, d, ops, **over)
    assert rc == BAD_ARG, (what, rc)
    assert np.all(out == 7.0)
    rc, out = run_launch(dbg, d, ops)                     # the unchanged descriptor is a valid one
    assert rc == 0, (what, dbg.error())


def test_zadd_with_members_is_refused(dbg):
    """rowdot_kernel offsets Mx, Zin and Zout by the member, not Zadd: the entry refuses what the kernel does not implement"""
    d = SC.launch(kernel="rowdot", n=5, K=256, nrhs=2, members=2)
    L = SC.launch_layout(d)
    ops = dict(M=np.ones(L.m_elems, np.float32), Zin=np.ones(L.zin_elems, np.float32), Zadd=np.ones(L.zin_elems, np.float32), Zout=np.full(L.zout_elems, 7.0, np.float32))
    rc, out = run_launch(dbg, d, ops)
    assert rc == BAD_ARG and np.all(out == 7.0)


# ---- the block solves on real factors ------------------------------------------------------------------------------------------------------------
SOLVE_SIZES = (2400, 4100)
_SOLVE_REF = {}


def solve_reference(dbg, kind, n):
    """right-hand sides [n, 4] (standard normal, fp32) and, per ``which``, the long-double solution on the device's factor with the errors of the
    two fp32 references, for all four columns and for the first alone"""
    key = (kind, n)
    if key not in _SOLVE_REF:
        L32 = dbg.f32_fit(kind, n)["L32"]
        B = np.random.default_rng([9100, n]).standard_normal((n, SC.TS_RHS)).astype(np.float32)
        inv = SC.block_inverses(L32)
        hp = {0: SC.hp_substitution(L32, B, 0), 1: SC.hp_substitution(L32, B, 1)}
        hp[2] = SC.hp_substitution(L32, hp[0], 1)
        _SOLVE_REF[key] = dict(B=B, hp=hp, sub={w: SC.substitution(L32, B, w) for w in (0, 1, 2)}, rest={w: SC.restatement(L32, inv, B, w) for w in (0, 1, 2)})
    return _SOLVE_REF[key]


def rel_err(x, hp):
    return float(np.max(np.abs(np.asarray(x, dtype=LD) - hp)) / np.max(np.abs(hp)))


@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["forward", "backward", "both"])
@pytest.mark.parametrize("n", SOLVE_SIZES)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_block_solves_are_as_accurate_as_substitution(dbg, kind, n, which, nrhs):
    """err = max|x - x_hp| / max|x_hp| over the nrhs columns:  err(device) <= 16 max(err(fp32 substitution), err(restatement), 2^-24)"""
    fit, ref = dbg.f32_fit(kind, n), solve_reference(dbg, kind, n)
    rhs = np.ascontiguousarray(ref["B"][:, :nrhs].T, dtype=np.float64)
    rc = dbg.lib.sigp_debug_f32_solve(fit["h"], which, ptr(rhs), n, nrhs)
    assert rc == 0, dbg.error(fit["h"])
    dev = rhs.T
    assert np.array_equal(dev.astype(np.float32).astype(np.float64), dev)              # fp32 results
    hp = ref["hp"][which][:, :nrhs]
    e_dev, e_sub, e_rest = rel_err(dev, hp), rel_err(ref["sub"][which][:, :nrhs], hp), rel_err(ref["rest"][which][:, :nrhs], hp)
    ratio = e_dev / max(e_sub, e_rest, 2.0 ** -24)
    print("block solve %-8s n=%d which=%d nrhs=%d: device %.3e  substitution %.3e  restatement %.3e  ratio %.3f" % (kind, n, which, nrhs, e_dev, e_sub, e_rest, ratio))
    note("solve%d" % which, "f32", "%s n=%d nrhs=%d" % (kind, n, nrhs), ratio)
    again = np.ascontiguousarray(ref["B"][:, :nrhs].T, dtype=np.float64)
    assert dbg.lib.sigp_debug_f32_solve(fit["h"], which, ptr(again), n, nrhs) == 0
    assert np.array_equal(bits(again), bits(rhs)), "a second identical call gave other bits"
    assert e_dev <= SC.BOUND * max(e_sub, e_rest, 2.0 ** -24), (e_dev, e_sub, e_rest)


def test_block_solve_entry_refuses_what_it_cannot_run(dbg):
    fit = dbg.f32_fit("rbf", 2400)
    rhs = np.ones((1, 2400))
    assert dbg.lib.sigp_debug_f32_solve(dbg.h, 2, ptr(rhs), 2400, 1) == BAD_ARG           # an fp64 handle without a fit
    assert dbg.lib.sigp_debug_f32_solve(fit["h"], 3, ptr(rhs), 2400, 1) == BAD_ARG
    assert dbg.lib.sigp_debug_f32_solve(fit["h"], 2, ptr(rhs), 2399, 1) == BAD_ARG
    assert dbg.lib.sigp_debug_f32_solve(fit["h"], 2, ptr(rhs), 2400, 5) == BAD_ARG
    assert np.all(rhs == 1.0)
    assert dbg.lib.sigp_debug_f32_get_inverse(dbg.h, 0, ptr(np.zeros(4, np.float32))) == BAD_ARG


# ---- the explicit inverses of the big diagonal blocks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2400, 2600, 4100])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_inverse_blocks_against_strtri(dbg, kind, n):
    """fU holds, per aligned 2048 diagonal block b, U_bb = L_bb^-T (upper triangular, row-major) by recursive doubling over 128-tiles with a
    ragged last pair (T = 19: level 2; T = 21: level 4; T = 33: a last block of one tile); fV its transpose.  R = U_bb^T L_bb - I in fp64 (the
    operands are fp32 values: fp64 forms every product exactly and sums 2048 of them to 1e-13), the last block restricted to the rows below n:
    max|R| <= 16 max|R_ref| with R_ref from LAPACK's strtri of the same block -- per 128-tile, so that a skipped tile pair is named.  fV is the
    transpose of fU bit for bit on and above the tile diagonal of every big block; below it fU is never written nor read."""
    fit = dbg.f32_fit(kind, n)
    L32, npad = fit["L32"], SC.n_pad(n)
    fU, fV = np.zeros((npad, npad), np.float32), np.zeros((npad, npad), np.float32)
    assert dbg.lib.sigp_debug_f32_get_inverse(fit["h"], 0, ptr(fU)) == 0, dbg.error(fit["h"])
    assert dbg.lib.sigp_debug_f32_get_inverse(fit["h"], 1, ptr(fV)) == 0, dbg.error(fit["h"])
    inv = SC.block_inverses(L32)
    for c0, kb in SC.big_blocks(npad):
        kv = min(kb, n - c0)                                                     # rows of the block below n
        Lb = L32[c0:c0 + kv, c0:c0 + kv].astype(np.float64)
        Ub = fU[c0:c0 + kb, c0:c0 + kb]
        nt = kb // NB
        upper = np.kron(np.triu(np.ones((nt, nt), bool)), np.ones((NB, NB), bool))          # tiles on and above the tile diagonal
        assert np.all(np.isfinite(Ub[upper]))
        assert np.array_equal(bits(np.ascontiguousarray(fV[c0:c0 + kb, c0:c0 + kb].T))[upper], bits(np.ascontiguousarray(Ub))[upper]), "fV is not fU transposed (block at %d)" % c0
        Ut = np.where(upper, Ub, np.float32(0))[:kv, :kv].astype(np.float64)
        assert np.all(np.tril(Ut, -1) == 0.0), "an inverse block is not upper triangular"
        R = Ut.T @ Lb - np.eye(kv)
        R_ref = inv[c0].astype(np.float64) @ Lb - np.eye(kv)
        worst_ref = float(np.max(np.abs(R_ref)))
        tiles = [(float(np.max(np.abs(R[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]))), i, j) for i in range((kv + NB - 1) // NB) for j in range(i + 1)]
        worst, wi, wj = max(tiles)
        print("inverse block %-8s n=%d c0=%d (%d tiles): max|U^T L - I| device %.3e (tile %d,%d)  strtri %.3e  ratio %.3f" % (kind, n, c0, nt, worst, wi, wj, worst_ref, worst / worst_ref))
        note("inverse", "f32", "%s n=%d c0=%d" % (kind, n, c0), worst / worst_ref)
        bad = ["tile (%d, %d): %.3e" % (i, j, v) for v, i, j in tiles if not v <= SC.BOUND * worst_ref]
        assert not bad, "block at %d: max|U^T L - I| per tile above %g * strtri's %.3e:\n  " % (c0, SC.BOUND, worst_ref) + "\n  ".join(bad)
