"""CPU tier of the per-feature (ARD) gradients of the leave-block-out scores (include/sigp.h: sigp_cv_grad_ard): the ABI is declared,
exported and bound, the Python argument checks need no device, and the NumPy closed form that the GPU tests use as their yardstick is
pinned against central differences of ``test_cv_host.cv_closed_form``, against ``test_loo_ard_host.loo_ard_closed_form`` at block = 1,
gap = 0, and against the adjoint form the device uses.

``cv_ard_closed_form`` is written the per-direction way: one explicit derivative matrix D_k per parameter and, per fold with window S,
    b = P D a,  C = P D P,  e = a^T D a;   dr = -H b_S + H C_SS r,   dH = H C_SS H,   ds = (-e + 2 b_S^T r - r^T C_SS r)/(n - w)  or  -e/n,
which is independent of the adjoint form
    d score = sum_ij G_ij D_ij,   G = 1/2 (v a^T + a v^T) + P B P + eps a a^T,   v = P beta.
The adjoint enters the reference only as the error SCALE S_k = sum_ij |G_ij D_ij| -- the gradient vanishes at an optimum and is no scale
for itself -- and as ``*_adj``, which one test compares with the per-direction numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_cv_host import cv_closed_form, cv_folds
from test_loo_ard_host import ard_k_tilde, loo_adjoint, loo_ard_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_ARD_SYMBOLS = {"sigp_cv_grad_ard": 12}
CRITERIA = ("nlpd", "sse")
# (n, d, block, gap): the shapes the issue pins to central differences
FD_SHAPES = [(37, 3, 5, 0), (37, 3, 5, 2), (60, 4, 1, 3), (130, 8, 64, 32), (129, 8, 16, 8)]


def cv_adjoint(P, y, block, gap, mode, crit):
    """G = d score / d K~ (symmetric) of the leave-block-out score ``crit`` ('nlpd' | 'sse') in sigma mode ``mode`` ('refit' | 'fixed'):
    per fold beta_f, B_f, eps_f assembled into beta, B, eps (include/sigp.h: sigp_cv_grad_ard)"""
    n = len(y)
    a = P @ y
    q = float(y @ a)
    beta, B, eps = np.zeros(n), np.zeros((n, n)), 0.0
    for r0, r1, c0, c1 in cv_folds(n, block, gap):
        w = r1 - r0
        H = np.linalg.inv(P[r0:r1, r0:r1])
        r = H @ a[r0:r1]
        s = (q - float(a[r0:r1] @ r)) / (n - w) if mode == "refit" else q / n
        sl = slice(c0 - r0, c1 - r0)
        hd = np.diag(H)
        rbar, kappa = np.zeros(w), np.zeros(w)
        if crit == "sse":
            rbar[sl] = 2 * r[sl]
        else:
            var = s * hd[sl]
            rbar[sl] = r[sl] / var
            kappa[sl] = 1 / (2 * var) - r[sl] ** 2 / (2 * var ** 2)
        t = H @ rbar
        sbar = float(np.sum(kappa * hd))
        bf = -t
        Bf = 0.5 * (np.outer(t, r) + np.outer(r, t)) + s * (H * kappa) @ H
        if mode == "refit":
            bf = bf + 2 * sbar * r / (n - w)
            Bf = Bf - sbar * np.outer(r, r) / (n - w)
            eps -= sbar / (n - w)
        else:
            eps -= sbar / n
        beta[r0:r1] += bf
        B[r0:r1, r0:r1] += Bf
    v = P @ beta
    return 0.5 * (np.outer(v, a) + np.outer(a, v)) + P @ B @ P + eps * np.outer(a, a)


def cv_ard_closed_form(kind, X, y, ells, sn, block, gap, mode="refit", route="inv"):
    """dict(nlpd, sse, nlpd_grad [d + 1], sse_grad [d + 1], nlpd_S, sse_S, nlpd_adj, sse_adj) at per-feature length scales ``ells`` and noise
    ``sn``: the leave-block-out scores, their derivatives with respect to (log l_1 .. log l_d, log sn~) the per-direction way, the error
    scales, and (``*_adj``) the same derivatives through the adjoint.  P = K~^-1 comes from the explicit inverse (route 'inv') or from the
    Cholesky factor as U U^T with U = L~^-T (route 'chol': the device's own route)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = X.shape
    U = X / np.asarray(ells, dtype=np.float64)
    D2 = O.sqdist(U, U)
    Kt = O.cov_unit(kind, U, U, 1.0) + sn * np.eye(n)
    if route == "inv":
        P = np.linalg.inv(Kt)
    else:
        Ui = solve_triangular(np.linalg.cholesky(Kt), np.eye(n), lower=True).T
        P = Ui @ Ui.T
    if kind == "rbf":
        h = np.exp(-0.5 * D2)
    else:
        s5 = np.sqrt(5.0 * D2)
        h = (5.0 / 3.0) * (1.0 + s5) * np.exp(-s5)
    a = P @ y
    q = float(y @ a)
    folds = []
    nlpd = sse = 0.0
    for r0, r1, c0, c1 in cv_folds(n, block, gap):
        H = np.linalg.inv(P[r0:r1, r0:r1])
        r = H @ a[r0:r1]
        s = (q - float(a[r0:r1] @ r)) / (n - (r1 - r0)) if mode == "refit" else q / n
        sl = slice(c0 - r0, c1 - r0)
        var = s * np.diag(H)[sl]
        nlpd += float(np.sum(0.5 * np.log(2 * np.pi * var) + r[sl] ** 2 / (2 * var)))
        sse += float(np.sum(r[sl] ** 2))
        folds.append((r0, r1, sl, H, r, s, var))
    out = dict(nlpd=nlpd, sse=sse)
    G = {c: cv_adjoint(P, y, block, gap, mode, c) for c in CRITERIA}
    for c in CRITERIA:
        for key in ("grad", "S", "adj"):
            out["%s_%s" % (c, key)] = np.zeros(d + 1)
    for k in range(d + 1):
        D = h * (U[:, k][:, None] - U[:, k][None, :]) ** 2 if k < d else sn * np.eye(n)
        tD = D @ a
        b = P @ tD
        e = float(a @ tD)
        PDP = P @ D @ P
        for r0, r1, sl, H, r, s, var in folds:
            Cs, bS = PDP[r0:r1, r0:r1], b[r0:r1]
            dr = (-H @ bS + H @ (Cs @ r))[sl]
            dH = np.einsum("ij,jk,ki->i", H, Cs, H)[sl]
            ds = (-e + 2 * float(bS @ r) - float(r @ Cs @ r)) / (n - (r1 - r0)) if mode == "refit" else -e / n
            dvar = ds * np.diag(H)[sl] + s * dH
            rr = r[sl]
            out["nlpd_grad"][k] += np.sum(dvar / (2 * var) + rr * dr / var - rr * rr * dvar / (2 * var ** 2))
            out["sse_grad"][k] += np.sum(2 * rr * dr)
        for crit in CRITERIA:
            out[crit + "_S"][k] = np.sum(np.abs(G[crit] * D))
            out[crit + "_adj"][k] = np.sum(G[crit] * D)
    return out


def cv_ard_problem(n, d):
    """(X, y, ells) of a shape: the data and scales the CPU and the GPU tier share"""
    X, y, _ = O.synthetic_problem(n, d, 20261200 + 7 * n + d)
    return X, y, ard_scales(d, 20261300 + 7 * n + d)


def test_cv_ard_entry_point_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in CV_ARD_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert L.CV_CRITERION_IDS == {"cv_nlpd": 0, "cv_sse": 1}
    assert L.load().sigp_version() >= 570


def test_cv_ard_null_handle_is_rejected_and_the_python_checks_need_no_device():
    import inspect

    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.zeros(4)
    assert lib.sigp_cv_grad_ard(None, 1, L.ptr(a), 4, 5, 0, 0, 0, None, None, L.ptr(a), L.ptr(a)) == L.BAD_ARG
    p = inspect.signature(S.GPR.cv_ard).parameters
    assert (p["gap"].default, p["criterion"].default, p["sigma_f"].default, p["grad"].default, p["predictions"].default) == (0, "cv_nlpd", "refit", "exact", False)
    p = inspect.signature(S.GPR.optimize_ard).parameters
    assert (p["criterion"].default, p["sigma_f"].default, p["method"].default, p["grad"].default, p["block"].default, p["gap"].default) == ("nlml", "refit", "L-BFGS-B", "exact", 5, 0)
    p = inspect.signature(S.GPR.optimize).parameters
    assert (p["block"].default, p["gap"].default) == (5, 0)
    assert callable(getattr(S.GPR, "cv_objective", None))

    gp = object.__new__(S.GPR)          # no handle, no device: every check below comes before the first library call
    gp._h, gp._fitted, gp._has_data, gp.kernel, gp.dtype = None, False, False, "rbf", "f64"
    th = np.zeros(4)
    for bad in (dict(criterion="loo_nlpd"), dict(criterion="nlml"), dict(sigma_f="both"), dict(grad="ref"), dict(gap=-1), dict(gap=62)):
        with pytest.raises(ValueError):
            gp.cv_ard(th, 5, **bad)
    for block in (0, 129, 2.5):
        with pytest.raises(ValueError):
            gp.cv_ard(th, block)
        with pytest.raises(ValueError):
            gp.cv_objective(th[:2], block)
        with pytest.raises(ValueError):
            gp.optimize_ard(th, criterion="cv_nlpd", block=block)
        with pytest.raises(ValueError):
            gp.optimize(th[:2], criterion="cv_sse", block=block)
    with pytest.raises(ValueError):
        gp.optimize_ard(th, criterion="cv")
    with pytest.raises(ValueError):
        gp.optimize(th[:2], criterion="cv")
    with pytest.raises(ValueError):
        gp.optimize(th, ard=True, criterion="cv_nlpd")        # stays refused: optimize_ard is the entry
    with pytest.raises(ValueError):
        gp.optimize(th[:2], criterion="cv_nlpd", grad="ref")
    with pytest.raises(RuntimeError):
        gp.cv_ard(th, 5)                                         # no data staged
    with pytest.raises(RuntimeError):
        gp.optimize(th[:2], criterion="cv_nlpd")
    gp._has_data, gp.n, gp.d = True, 10, 3
    for call in (lambda: gp.cv_ard(th, 10), lambda: gp.cv_ard(th, 4, gap=5), lambda: gp.cv_objective(th[:2], 10),
                 lambda: gp.optimize_ard(th, criterion="cv_sse", block=10), lambda: gp.optimize(th[:2], criterion="cv_sse", block=10)):
        with pytest.raises(ValueError):
            call()                                               # a fold that leaves no training row
    with pytest.raises(ValueError):
        gp.cv_ard(th[:3], 5)                                     # d + 1 entries
    for kernel, dtype in (("netdiffusion", "f64"), ("rbf", "f32")):
        gp.kernel, gp.dtype = kernel, dtype
        with pytest.raises(ValueError):
            gp.cv_ard(th, 5)
        with pytest.raises(ValueError):
            gp.cv_objective(th[:2], 5)
        with pytest.raises(ValueError):
            gp.optimize_ard(th, criterion="cv_nlpd", block=5)
        with pytest.raises(ValueError):
            gp.optimize(th[:2], criterion="cv_nlpd", block=5)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d,block,gap", FD_SHAPES)
def test_closed_form_equals_central_differences(kind, n, d, block, gap):
    X, y, ells = cv_ard_problem(n, d)
    sn, h = 1e-2, 1e-5
    th = np.concatenate([np.log(ells), [np.log(sn)]])
    for mode in ("refit", "fixed"):
        ref = cv_ard_closed_form(kind, X, y, ells, sn, block, gap, mode)
        at = cv_closed_form(ard_k_tilde(kind, X, ells, sn), y, block, gap, mode)
        for crit in CRITERIA:
            assert abs(ref[crit] - at[crit]) <= 1e-10 * abs(at[crit]), (mode, crit)
        num = {c: np.zeros(d + 1) for c in CRITERIA}
        for p in range(d + 1):
            v = []
            for sgn in (1.0, -1.0):
                t = th.copy(); t[p] += sgn * h
                v.append(cv_closed_form(ard_k_tilde(kind, X, np.exp(t[:d]), np.exp(t[d])), y, block, gap, mode))
            for crit in CRITERIA:
                num[crit][p] = (v[0][crit] - v[1][crit]) / (2 * h)
        for crit in CRITERIA:
            err = np.abs(ref[crit + "_grad"] - num[crit]) / ref[crit + "_S"]
            print("%s n=%d d=%d block=%d gap=%d %s %s: error / S %s" % (kind, n, d, block, gap, mode, crit, err))
            assert np.all(err <= 1e-7), (kind, n, d, block, gap, mode, crit, err)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("mode", ["refit", "fixed"])
def test_block_one_without_a_gap_is_the_leave_one_out_gradient(kind, mode):
    """the same sums in another order: rounding only (1e-10 S); the adjoint is loo_adjoint's to 1e-13 of its largest entry"""
    n, d = 60, 4
    X, y, ells = cv_ard_problem(n, d)
    cv = cv_ard_closed_form(kind, X, y, ells, 1e-2, 1, 0, mode)
    loo = loo_ard_closed_form(kind, X, y, ells, 1e-2, mode)
    P = np.linalg.inv(ard_k_tilde(kind, X, ells, 1e-2))
    for crit in CRITERIA:
        assert abs(cv[crit] - loo[crit]) <= 1e-12 * abs(loo[crit]), crit
        assert np.all(np.abs(cv[crit + "_grad"] - loo[crit + "_grad"]) <= 1e-10 * loo[crit + "_S"]), crit
        assert np.all(np.abs(cv[crit + "_S"] - loo[crit + "_S"]) <= 1e-10 * loo[crit + "_S"]), crit
        Ga, Gb = cv_adjoint(P, y, 1, 0, mode, crit), loo_adjoint(P, y, mode, crit)
        assert np.max(np.abs(Ga - Gb)) <= 1e-13 * np.max(np.abs(Gb)), crit


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d,block,gap", [(129, 8, 16, 8), (60, 4, 1, 3), (130, 8, 64, 32)])
def test_adjoint_form_equals_the_per_direction_form_and_both_routes_agree(kind, n, d, block, gap):
    """What the device computes (the contraction with G) against the per-direction chain rule, and the two routes to P = K~^-1 whose
    difference / S is the GPU tests' measure of the reference's own error.  Rounding only: 1e-10 S."""
    X, y, ells = cv_ard_problem(n, d)
    for mode in ("refit", "fixed"):
        a = cv_ard_closed_form(kind, X, y, ells, 1e-2, block, gap, mode, "inv")
        b = cv_ard_closed_form(kind, X, y, ells, 1e-2, block, gap, mode, "chol")
        for crit in CRITERIA:
            S = a[crit + "_S"]
            assert np.all(np.abs(a[crit + "_adj"] - a[crit + "_grad"]) <= 1e-10 * S), (mode, crit)
            assert np.all(np.abs(a[crit + "_grad"] - b[crit + "_grad"]) <= 1e-10 * S), (mode, crit)
