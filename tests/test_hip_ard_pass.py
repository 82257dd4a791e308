"""GPU tier of the ARD tile pass (csrc/ardgrad.hpp, csrc/looard.hpp), one call of ard_tile_pass_members and its finish kernel at a time through
the debug library's run-and-return entry ``sigp_debug_run_ard_pass``: host operands in, every buffer back whole.  Reference, bound (derived
term by term from the kernel's arithmetic, no fitted factor) and the cases: tests/score_kernel_cases.py, whose host tier shows that every
listed mutation of the kernel's formula leaves the bound by a factor of 10 at least.

Per case: every partial of every tile and feature and every gradient component within its bound; Uc within its bound and exactly zero in its
padding; partials exactly zero at n = 1; sentinels kept from column d rounded up to 16 on and in every gap; NaN everywhere the contract says
nothing is used (P / M outside j < i < n and the diagonal, a and v from n on, the member gaps, q under ARD_W_LOO, v and eps under
ARD_W_NLML) without a trace in the results; the same bits on a second call; a member of a group of 3 bit for bit the member run alone.
``-s`` prints error / bound per case and, last, the largest per kernel and family with the gradient's error / S beside it."""
import ctypes as C

import numpy as np
import pytest

import hp_reference as H
import score_kernel_cases as K

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.AVAILABLE, reason="long double is not an extended type here")]
WORST = {}


@pytest.fixture(scope="module")
def dbg():
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load(debug=True)
    _p, _l, _i, _d, _f = C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_double), C.c_double
    lib.sigp_debug_run_ard_pass.restype = _i
    lib.sigp_debug_run_ard_pass.argtypes = [_p, _i, _i, _i, _i, _i, _i, _i, _d, _l, _l, _d, _l, _l, _l, _d, _l, _l, _d, _l, _l, _f, _d, _d, _d, _l, _l, _d, _l, _l]
    h = C.c_void_p()
    assert lib.sigp_create(C.byref(h), 0, 0) == L.OK
    yield lib, h, L
    lib.sigp_destroy(h)


def _args(c, ops):
    Ly = K.ard_layout(c)
    return dict(wsel=K.WSEL[c.wsel], kernel_id=K.KERNEL_ID[c.kern], n=c.n, n_pad=c.n_pad, d=c.d, dp=Ly.dp, members=c.members, sU=Ly.sU, u_elems=Ly.u_elems, ld=Ly.ld,
                sP=Ly.sP, m_elems=Ly.m_elems, sVec=Ly.sVec, vec_elems=Ly.vec_elems, sQ=Ly.sQ, q_elems=Ly.q_elems, sPartial=Ly.sPartial,
                partial_elems=Ly.partial_elems, sGrad=Ly.sGrad, grad_elems=Ly.grad_elems)


def _run(dbg, c, ops, **over):
    """(return code, dict(Uc, partial, grad)); a single fit hands its sn~ over as the argument, a group as sn_m"""
    lib, h, L = dbg
    a = dict(_args(c, ops), **over)
    out = dict(Uc=K.sentinels(K.ard_layout(c).uc_elems), partial=np.array(ops["partial"]), grad=np.array(ops["grad"]))
    single = c.members == 1
    sn_m = None if single else np.array(ops["sn_m"])
    rc = lib.sigp_debug_run_ard_pass(h, a["wsel"], a["kernel_id"], a["n"], a["n_pad"], a["d"], a["dp"], a["members"], L.ptr(ops["U"]), a["sU"], a["u_elems"],
                                     L.ptr(ops["M"]), a["ld"], a["sP"], a["m_elems"], L.ptr(ops["vec"]), a["sVec"], a["vec_elems"], L.ptr(ops["q"]), a["sQ"],
                                     a["q_elems"], float(ops["sn_m"][0]) if single else float("nan"), L.ptr(sn_m), L.ptr(out["Uc"]), L.ptr(out["partial"]),
                                     a["sPartial"], a["partial_elems"], L.ptr(out["grad"]), a["sGrad"], a["grad_elems"])
    return rc, out


@pytest.mark.parametrize("c", K.ard_cases(), ids=K.ard_id)
def test_one_pass_values_footprint_and_bits(dbg, c):
    lib, h, L = dbg
    ops = K.ard_operands(c)
    rc, out = _run(dbg, c, ops)
    assert rc == L.OK, lib.sigp_last_error(h)
    r = K.ard_judge(c, ops, out)
    print("%s: error / bound  Uc %.3g  partial %.3g  grad %.3g  noise %.3g;  error / S %.3g" % (K.ard_id(c), r["uc"], r["partial"], r["grad"], r["noise"], r["err_over_S"]))
    for part in ("uc", "partial", "grad", "noise", "err_over_S"):
        key = (part, c.kern, c.wsel, c.family)
        WORST[key] = max(WORST.get(key, 0.0), r[part])
    assert r["uc"] <= 1.0 and r["uc_padding_zero"], ("Uc", r)
    assert r["partial"] <= 1.0, ("a partial is outside its bound (or something that must not be used was used)", r)
    assert r["zero_columns"] and r["n1_zero"], ("columns d .. of a written chunk, or the partials of n = 1, are not exactly zero", r)
    assert r["grad"] <= 1.0 and r["noise"] <= 1.0, ("finish kernel", r)
    assert r["moved"] == 0, "a sentinel outside the written columns was overwritten"
    rc2, again = _run(dbg, c, ops)
    assert rc2 == L.OK and all(K.same_bits(out[k], again[k]) for k in out), "a second call differs"
    if c.members > 1:
        Ly = K.ard_layout(c)
        c1, ops1 = K.ard_member(c, ops, 1)
        rc1, alone = _run(dbg, c1, ops1)
        assert rc1 == L.OK, lib.sigp_last_error(h)
        assert K.same_bits(alone["partial"], out["partial"][Ly.sPartial:2 * Ly.sPartial]), "a group member's partials differ from the member run alone"
        assert K.same_bits(alone["grad"], out["grad"][Ly.sGrad:2 * Ly.sGrad]), "a group member's gradient differs from the member run alone"
        assert K.same_bits(alone["Uc"], out["Uc"][Ly.sU:Ly.sU + c.n_pad * Ly.dp])


def test_refused_descriptors_launch_nothing(dbg):
    lib, h, L = dbg
    for c in (next(x for x in K.ard_cases() if x.members == 3 and x.wsel == "nlml" and x.d == 17),
              next(x for x in K.ard_cases() if x.members == 3 and x.wsel == "loo" and x.n_pad == 256)):
        ops, Ly = K.ard_operands(c), K.ard_layout(c)

        def refused(**over):
            rc, out = _run(dbg, c, ops, **over)
            assert K.same_bits(out["partial"], ops["partial"]) and K.same_bits(out["grad"], ops["grad"]) and K.kept(out["Uc"], slice(None)), over
            return rc == L.BAD_ARG

        # the last member's last element of every buffer (behind it: the trailing gap, and for M the row padding)
        assert refused(u_elems=Ly.u_elems - 7) and refused(m_elems=Ly.m_elems - 13) and refused(vec_elems=Ly.vec_elems - 6 - (0 if c.wsel == "loo" else 3 * c.n_pad + 1))
        assert refused(partial_elems=Ly.partial_elems - 6) and refused(grad_elems=Ly.grad_elems - 4) and refused(members=4)
        if c.wsel == "nlml":
            assert refused(q_elems=Ly.q_elems - 3)
        # strides that are not multiples of 16 bytes
        assert refused(sU=Ly.sU - 1) and refused(sP=Ly.sP - 1) and refused(sVec=Ly.sVec - 1) and refused(ld=Ly.ld - 1) and refused(dp=Ly.dp - 1)
        # members whose outputs overlap
        assert refused(sPartial=Ly.tiles * Ly.dp - 2) and refused(sGrad=c.d) and refused(sU=c.n_pad * Ly.dp - 2) and refused(sPartial=0)
        # what the kernels do not implement
        assert refused(wsel=2) and refused(kernel_id=0) and refused(n=0) and refused(n=c.n_pad + 1) and refused(n_pad=c.n_pad - 56) and refused(d=0)
        assert refused(dp=Ly.dq - 2) and refused(members=0) and refused(members=9) and refused(ld=c.n_pad - 2)


def test_zz_summary_of_the_largest_ratios():
    """(prints; with -s) the largest error / bound per kernel, weight and family, and the gradient's error / S per family"""
    print("\n%-9s %-5s %-8s  %9s %9s %9s %9s  %10s" % ("kernel", "W", "family", "Uc", "partial", "grad", "noise", "error / S"))
    for kern in K.KERNEL_ID:
        for wsel in K.WSEL:
            for fam in K.ARD_FAMILIES:
                if ("partial", kern, wsel, fam) in WORST:
                    print("%-9s %-5s %-8s  %9.3g %9.3g %9.3g %9.3g  %10.3g" % ((kern, wsel, fam) + tuple(WORST[(p, kern, wsel, fam)] for p in ("uc", "partial", "grad", "noise", "err_over_S"))))
    for fam in K.ARD_FAMILIES:
        print("error / S, family %-8s %.3g" % (fam, max([v for k, v in WORST.items() if k[0] == "err_over_S" and k[3] == fam] or [0.0])))
    assert all(v <= 1.0 for k, v in WORST.items() if k[0] != "err_over_S")
