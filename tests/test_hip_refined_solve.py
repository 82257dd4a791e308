"""GPU tier: refined_solve_kernel (csrc/refined_solve.hpp, option ``accurate_solve``) one launch at a time through
``sigp_debug_run_refined_solve`` of libsigp_debug.so, which issues it through the engine's own launcher.

Operands.  L = the fp64 factor of the leading 128-block of family A (tests/hp_reference.py; n = 384, both kernels) at sn~ = 1e-4, 1e-8, 1e-11
and 1e-13; W = inv(L) by long-double substitution rounded to fp64, and also the pair (L, W) the device's own diagonal-block kernel returns for
that block.  Right-hand sides, two kinds:
  "normal"      A standard normal, as the issue of this feature sets it;
  "consistent"  A = X0 L^T with X0 standard normal (transposed form: X0 L): rows as the factorisation meets them, whose solution is of
                moderate size.
Bound, per row i:  max_j |X L^T - A|_ij <= 16 max(the same figure of fp64 substitution (scipy.linalg.solve_triangular) on the same operands,
u max_j (|X| |L^T|)_ij), every figure formed in long double.
Control.  The plain product A W^T (what the engine runs without the option), formed on the host from the same operands at sn~ = 1e-11, must
EXCEED that bound, or the test could not tell the two kernels apart.  Measured on the host: on "consistent" rows it does so on every row (60 to
25 000 times the bound's right-hand side); on "normal" rows it does NOT (0.3 to 3): a random right-hand side makes |X| ~ cond(L) |A|, the floor
u |X| |L^T| then is as large as the plain product's error, and nothing distinguishes a backward-stable solve from the product.  The control is
therefore asserted on the consistent rows and printed for the normal ones; the bound is asserted on both.

Also: NaN in the strict upper triangle of the L operand (it must not be read: what stands above the diagonal of a diagonal block of the matrix is
undefined), sentinels in every entry the launch does not own (columns beyond 128 of a wider row stride, rows beyond ``rows``, the gap between
members), the same bits from a second call, row counts of one tile, three tiles and a count off the tile boundary, 1 and 2 members (the second
member with another level's blocks, so that a dropped member offset shows), and the descriptors the entry must refuse.
"""
import ctypes as C

import numpy as np
import pytest

import hp_reference as H
import refined_cases as RC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")]

NB, MARGIN, BAD_ARG = RC.NB, 16.0, 2
SENTINEL = -7.0e300
ROWS = (RC.TILE, 3 * RC.TILE, RC.TILE + 13)          # one tile, three tiles, two tiles of which the second holds 13 rows
_i, _l, _p = C.c_int, C.c_int64, C.c_void_p


def ptr(a):
    return a.ctypes.data_as(_p)


class Dbg:
    def __init__(self):
        from seaiceextentforecasting_amd import _lib as L
        self.lib = lib = L.load(debug=True)
        lib.sigp_debug_run_refined_solve.restype = _i
        lib.sigp_debug_run_refined_solve.argtypes = [_p, _i, _p, _l, _i, _p, _l, _p, _l, _i, _l, _l, _l, _l, _l, _l]
        lib.sigp_debug_time_diag.restype = _i
        lib.sigp_debug_time_diag.argtypes = [_p, _p, _i, _i, _p, _p, _p]
        self.h = _p()
        rc = lib.sigp_create(C.byref(self.h), 0, 0)
        assert rc == 0, "sigp_create failed (rc = %d)" % rc

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


_BLOCKS = {}


def blocks(dbg, kind, level, source):
    """(L, W) of the leading block: source "host" = LAPACK's factor and its long-double inverse, "device" = what potrf_diag_kernel returns"""
    key = (kind, level, source)
    if key not in _BLOCKS:
        K11, L, W = RC.leading_block(kind, level)
        if source == "device":
            ms, L, W = C.c_double(0), np.zeros((NB, NB)), np.zeros((NB, NB))
            assert dbg.lib.sigp_debug_time_diag(dbg.h, ptr(K11), 0, 1, C.byref(ms), ptr(L), ptr(W)) == 0, dbg.error()
            L, W = np.tril(L), np.tril(W)
        _BLOCKS[key] = (L, W)
    return _BLOCKS[key]


def rhs(rows, Ls, trans, kind_of_rhs, seed):
    rng = np.random.default_rng(seed)
    out = []
    for L in Ls:
        A = rng.standard_normal((rows, NB))
        out.append(A @ (np.tril(L) if trans else np.tril(L).T) if kind_of_rhs == "consistent" else A)
    return out


def run(dbg, trans, As, Ls, Ws, lda=NB + 6, ldl=NB + 2, gap=64, extra_rows=3):
    """one launch on `len(As)` members; returns the solved rows per member after checking that nothing else was written"""
    members, rows = len(As), As[0].shape[0]
    sA = (rows + extra_rows) * lda + gap
    buf = np.full((members - 1) * sA + (rows + extra_rows) * lda, SENTINEL)
    Lbuf, Wbuf = np.full((members, NB, ldl), np.nan), np.full((members, NB, NB), SENTINEL)
    owned = np.zeros(buf.shape, dtype=bool)
    for m in range(members):
        view = buf[m * sA: m * sA + rows * lda].reshape(rows, lda)
        view[:, :NB] = As[m]
        owned[m * sA: m * sA + rows * lda].reshape(rows, lda)[:, :NB] = True
        iu = np.triu_indices(NB, 1)
        Lbuf[m, :, :NB] = np.tril(Ls[m])
        Lbuf[m, iu[0], iu[1]] = np.nan                         # the strict upper triangle of the L operand: never to be read
        Wbuf[m] = np.tril(Ws[m])
    before = buf.copy()
    rc = dbg.lib.sigp_debug_run_refined_solve(dbg.h, int(trans), ptr(buf), lda, rows, ptr(Wbuf), NB, ptr(Lbuf), ldl, members, sA, NB * NB, NB * ldl,
                                              buf.size, Wbuf.size, Lbuf.size)
    assert rc == 0, dbg.error()
    assert np.array_equal(buf[~owned], before[~owned]), "the launch wrote outside the rows it owns"
    out = [buf[m * sA: m * sA + rows * lda].reshape(rows, lda)[:, :NB].copy() for m in range(members)]
    assert all(np.all(np.isfinite(X)) for X in out), "NaN from above the diagonal of L (or a sentinel) reached the result"
    return out, buf


def check_rows(X, L, A, trans, what):
    res, floor = RC.row_residual(X, L, A, trans)
    Xs = RC.substitution(A, L, trans)
    res_s, _ = RC.row_residual(Xs, L, A, trans)
    bound = MARGIN * np.maximum(res_s, floor)
    worst = float(np.max(res / np.maximum(res_s, floor)))
    print("%-64s max row residual / max(substitution's, floor) = %.3f" % (what, worst))
    assert np.all(res <= bound), "%s: row %d: %.3e > 16 max(%.3e, %.3e)" % (what, int(np.argmax(res / bound)), res.max(), res_s.max(), floor.max())
    return bound


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("level", RC.LEVELS)
@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("trans", [False, True], ids=["forward", "transposed"])
def test_one_launch_solves_to_substitution_accuracy(dbg, trans, kind, level, source):
    """every row count and both kinds of right-hand side, one member; then two members (the second with the next level's blocks) on the row
    count off the tile boundary; and a second call returns the same bits"""
    L, W = blocks(dbg, kind, level, source)
    print()
    for rows in ROWS:
        for which in ("normal", "consistent"):
            (A,) = rhs(rows, [L], trans, which, 100 + rows)
            (X,), raw = run(dbg, trans, [A], [L], [W])
            check_rows(X, L, A, trans, "%s %s sn~=%g W:%s rows=%d %s" % ("T" if trans else "F", kind, level, source, rows, which))
            if rows == ROWS[-1]:
                (X2,), raw2 = run(dbg, trans, [A], [L], [W])
                assert np.array_equal(raw.view(np.uint64), raw2.view(np.uint64)), "a second call returned other bits"
    other = RC.LEVELS[(RC.LEVELS.index(level) + 1) % len(RC.LEVELS)]
    L2, W2 = blocks(dbg, kind, other, source)
    As = rhs(ROWS[-1], [L, L2], trans, "consistent", 7)
    Xs, _ = run(dbg, trans, As, [L, L2], [W, W2])
    for m, (X, Lm, A) in enumerate(zip(Xs, (L, L2), As)):
        check_rows(X, Lm, A, trans, "%s %s sn~=%g W:%s two members, member %d" % ("T" if trans else "F", kind, (level, other)[m], source, m))
    (X1,), _ = run(dbg, trans, As[1:], [L2], [W2])
    assert np.array_equal(Xs[1], X1), "a member of a group carries other bits than the same rows alone"


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("trans", [False, True], ids=["forward", "transposed"])
def test_the_plain_product_fails_the_same_bound(dbg, trans, kind):
    """the control at sn~ = 1e-11: A W^T on the host, same operands (module docstring: asserted on the consistent rows, printed for the normal ones)"""
    L, W = blocks(dbg, kind, 1e-11, "host")
    print()
    for which in ("normal", "consistent"):
        (A,) = rhs(ROWS[-1], [L], trans, which, 100 + ROWS[-1])
        P = RC.refined(A, W, L, steps=0, trans=trans)
        res, floor = RC.row_residual(P, L, A, trans)
        res_s, _ = RC.row_residual(RC.substitution(A, L, trans), L, A, trans)
        r = res / np.maximum(res_s, floor)
        print("plain product, %s %s rows: residual / max(substitution's, floor) = %.2f .. %.2f" % (kind, which, r.min(), r.max()))
        if which == "consistent":
            assert np.all(r > MARGIN), "the bound does not separate the plain product from the refined solve"
            (X,), _ = run(dbg, trans, [A], [L], [W])
            res_d, floor_d = RC.row_residual(X, L, A, trans)
            assert np.all(res_d <= MARGIN * np.maximum(res_s, floor_d))


def test_bad_descriptors_are_refused(dbg):
    L, W = blocks(dbg, "rbf", 1e-4, "host")
    A = np.zeros((40, NB))
    call = dbg.lib.sigp_debug_run_refined_solve

    def rc(trans=0, lda=NB, rows=40, ldw=NB, ldl=NB, members=1, sA=0, sW=0, sL=0, a_elems=A.size, w_elems=W.size, l_elems=L.size):
        return call(dbg.h, trans, ptr(A), lda, rows, ptr(W), ldw, ptr(L), ldl, members, sA, sW, sL, a_elems, w_elems, l_elems)

    assert rc() == 0 and rc(members=2, sA=20 * NB, rows=20) == 0, dbg.error()
    for bad in (dict(trans=2), dict(rows=0), dict(rows=41), dict(lda=NB - 2), dict(lda=NB + 1), dict(ldw=NB + 2), dict(ldl=NB + 2), dict(members=0),
                dict(members=2, sA=0), dict(members=2, sA=20 * NB - 2, rows=20), dict(members=2, sA=20 * NB + 1, rows=20), dict(a_elems=A.size - 1),
                dict(w_elems=W.size - 1), dict(l_elems=L.size - 1), dict(members=2, sA=20 * NB, rows=20, sW=2), dict(sA=-2)):
        assert rc(**bad) == BAD_ARG, bad
    assert np.all(A == 0)
    h32 = _p()
    assert dbg.lib.sigp_create(C.byref(h32), 0, 1) == 0
    try:
        assert call(h32, 0, ptr(A), NB, 40, ptr(W), NB, ptr(L), NB, 1, 0, 0, 0, A.size, W.size, L.size) == BAD_ARG      # fp64 only
    finally:
        dbg.lib.sigp_destroy(h32)
