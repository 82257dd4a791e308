"""GPU tier of the two kernels that form W = U C for the hindcast gradient (csrc/hindcast.hpp), one launch at a time through the debug
library's run-and-return entry ``sigp_debug_run_hindcast_w``: ``hindcast_w_kernel`` (which = 0: the single fit's, whose member path only
the lockstep groups beyond the LDS limit take) and ``hindcast_w_lds_kernel`` (which = 1: the groups').

    W_ik = sum_{j >= i, |j - k| < lead} U_ij Cb_jk  -  ( zbar_k sum_{i <= j < k} U_ij z_j  +  z_k sum_{j >= max(i, k)} U_ij zbar_j ) / 2      (i, k < n)

Reference: the formula in long double.  Bound: an entry is one chain of at most len + 2 lead + 2 roundings over its terms (len = n - i: a
scan of at most len - 1 additions, the closing product or fma, 2 lead - 1 fmas of the banded part), so its error is at most
(len + 2 lead + 2) u (|U| |C|)_ik with u = 2^-53 and |C| assembled from the absolute values of Cb and of the two rank-one terms.
Everything the kernels must not read is NaN: U left of its diagonal and from n on, Cb outside its band and from n on, z and zbar from n on."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -12345.678
U_RND = 2.0 ** -53


def _bits(a, b):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)))


@pytest.fixture(scope="module")
def dbg():
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load(debug=True)
    _p, _l, _i, _d = C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_double)
    lib.sigp_debug_run_hindcast_w.restype = _i
    lib.sigp_debug_run_hindcast_w.argtypes = [_p, _i, _d, _d, _d, _d, _d, _i, _i, _l, _i, _i, _l, _l, _l, _l]
    h = C.c_void_p()
    assert lib.sigp_create(C.byref(h), 0, 0) == L.OK
    yield lib, h, L
    lib.sigp_destroy(h)


@functools.lru_cache(maxsize=None)
def _case(n, lead, members, wide):
    """operands with padded strides when ``wide``, and per member the long-double W [n][n] and the scale |U| |C| [n][n]"""
    rng = np.random.default_rng(20265000 + 1000 * n + 10 * lead + members + (5 if wide else 0))
    n_pad = (n + 127) // 128 * 128
    ld = n_pad + (2 if wide else 0)
    sC = n_pad * ld + (6 if wide else 0)
    sZ = n + (3 if wide else 0)
    c_elems, z_elems = members * sC + (4 if wide else 0), members * sZ + (2 if wide else 0)
    U, Cb = np.full(c_elems, np.nan), np.full(c_elems, np.nan)
    z, zbar = np.full(z_elems, np.nan), np.full(z_elems, np.nan)
    refs = []
    ii, kk = np.arange(n)[:, None], np.arange(n)[None, :]
    for m in range(members):
        Um = np.triu(rng.standard_normal((n, n)))
        Cm = rng.standard_normal((n, n))
        Cm = np.where(np.abs(ii - kk) < lead, 0.5 * (Cm + Cm.T), 0.0)
        zm, zb = rng.standard_normal(n), rng.standard_normal(n)
        Uv = U[m * sC:m * sC + n_pad * ld].reshape(n_pad, ld)
        Cv = Cb[m * sC:m * sC + n_pad * ld].reshape(n_pad, ld)
        Uv[:n, :n] = np.where(kk >= ii, Um, np.nan)
        Cv[:n, :n] = np.where(np.abs(ii - kk) < lead, Cm, np.nan)
        z[m * sZ:m * sZ + n], zbar[m * sZ:m * sZ + n] = zm, zb
        refs.append((_w_formula(Um.astype(np.longdouble), Cm.astype(np.longdouble), zm.astype(np.longdouble), zb.astype(np.longdouble), lead),
                     _w_formula(np.abs(Um), np.abs(Cm), np.abs(zm), np.abs(zb), lead, scale=True)))
    return dict(n=n, n_pad=n_pad, ld=ld, lead=lead, members=members, sC=sC, sZ=sZ, c_elems=c_elems, z_elems=z_elems, U=U, Cb=Cb, z=z, zbar=zbar, refs=refs)


def _w_formula(U, Cb, z, zbar, lead, scale=False):
    """the formula above on an upper-triangular U [n][n] in U's precision; ``scale``: the operands are absolute values and the rank-one terms
    are added instead of subtracted -- the sum of the absolute values of an entry's terms, |U| |C|"""
    n = U.shape[0]
    W = np.zeros_like(U)
    for o in range(-(lead - 1), lead):                       # the banded part: column k takes U[:, k + o] Cb[k + o, k]
        k = np.arange(max(0, -o), min(n, n - o))
        W[:, k] += U[:, k + o] * Cb[k + o, k][None, :]
    P, Q = U * z[None, :], U * zbar[None, :]
    pre = np.cumsum(P, axis=1) - P                           # sum_{j < k} U_ij z_j   (U is zero left of the diagonal: j runs from i)
    suf = np.cumsum(Q[:, ::-1], axis=1)[:, ::-1]             # sum_{j >= k} U_ij zbar_j: the whole row sum for k <= i
    half = np.asarray(0.5, dtype=U.dtype)
    rank = half * (zbar[None, :] * pre + z[None, :] * suf)
    return W + rank if scale else W - rank


def _run(dbg, c, which):
    lib, h, L = dbg
    W = np.full(c["c_elems"], SENT)
    rc = lib.sigp_debug_run_hindcast_w(h, which, L.ptr(c["U"]), L.ptr(c["Cb"]), L.ptr(c["z"]), L.ptr(c["zbar"]), L.ptr(W), c["n"], c["n_pad"], c["ld"], c["lead"],
                                       c["members"], c["sC"], c["sZ"], c["c_elems"], c["z_elems"])
    assert rc == L.OK, lib.sigp_last_error(h)
    return W


# n: one row; one row past a block; chunk lengths c = ceil(len / 256) = 1 and 2 with both edges (256, 257); c = 3 (600)
@pytest.mark.parametrize("members,wide", [(1, False), (2, True)])
@pytest.mark.parametrize("lead", [1, 5, 128])
@pytest.mark.parametrize("n", [2, 129, 257, 600])
def test_one_launch_value_zeros_sentinels_and_bits(dbg, n, lead, members, wide):
    c = _case(n, lead, members, wide)
    n_pad, ld, sC = c["n_pad"], c["ld"], c["sC"]
    got = {}
    for which in (0, 1):
        W = _run(dbg, c, which)
        assert _bits(W, _run(dbg, c, which)), ("a second launch differs", which)
        owned = np.zeros(c["c_elems"], dtype=bool)
        for m in range(members):
            Wm = W[m * sC:m * sC + n_pad * ld].reshape(n_pad, ld)
            owned[m * sC:m * sC + n_pad * ld].reshape(n_pad, ld)[:, :n_pad] = True
            assert np.all(Wm[n:, :n_pad] == 0.0) and np.all(Wm[:n, n:n_pad] == 0.0), ("rows and columns n .. n_pad", which, m)
            ref, scale = c["refs"][m]
            bound = (n - np.arange(n)[:, None] + 2 * lead + 2) * U_RND * scale
            err = np.abs(Wm[:n, :n].astype(np.longdouble) - ref).astype(np.float64)
            assert np.all(np.isfinite(Wm[:n, :n])), ("something that must not be read was read", which, m)
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
            print("n=%d lead=%d members=%d which=%d member %d: error / bound max %.3g" % (n, lead, members, which, m, worst))
            assert np.all(err <= bound), (which, m, worst)
        assert np.all(W[~owned] == SENT), ("a sentinel outside the owned rows was overwritten", which)
        got[which] = W
    assert _bits(got[0], got[1]), "hindcast_w_lds_kernel and hindcast_w_kernel differ"


def test_descriptors_that_leave_the_buffers_are_refused(dbg):
    lib, h, L = dbg
    c = _case(129, 5, 2, True)

    def rc(which=1, **over):
        a = dict(c, **over)
        W = np.full(c["c_elems"], SENT)
        r = lib.sigp_debug_run_hindcast_w(h, which, L.ptr(c["U"]), L.ptr(c["Cb"]), L.ptr(c["z"]), L.ptr(c["zbar"]), L.ptr(W), a["n"], a["n_pad"], a["ld"], a["lead"],
                                          a["members"], a["sC"], a["sZ"], a["c_elems"], a["z_elems"])
        assert r != L.OK and np.all(W == SENT)
        return r

    for which in (0, 1):
        assert rc(which, members=3) == L.BAD_ARG                       # a third member leaves both buffers
        assert rc(which, c_elems=c["c_elems"] - 14) == L.BAD_ARG and rc(which, z_elems=c["z_elems"] - 6) == L.BAD_ARG      # the last member's last entry
        assert rc(which, ld=c["n_pad"] - 1) == L.BAD_ARG and rc(which, n_pad=384) == L.BAD_ARG and rc(which, n_pad=200) == L.BAD_ARG
        assert rc(which, sC=c["n_pad"] * c["ld"] - 3) == L.BAD_ARG      # members would share entries
        assert rc(which, n=0) == L.BAD_ARG and rc(which, n=c["n_pad"] + 1) == L.BAD_ARG
        assert rc(which, lead=0) == L.BAD_ARG and rc(which, lead=129) == L.BAD_ARG
        assert rc(which, members=0) == L.BAD_ARG and rc(which, members=9) == L.BAD_ARG
    assert rc(2) == L.BAD_ARG
