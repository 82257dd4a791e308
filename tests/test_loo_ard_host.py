"""CPU tier of the per-feature (ARD) gradients of the leave-one-out scores (include/sigp.h: sigp_loo_grad_ard): the ABI is declared,
exported and bound, and the NumPy closed form that the GPU tests use as their yardstick is pinned against central differences of the
leave-one-out scores of NumPy refits and, at equal scales, against the isotropic closed form of tests/test_loo_grad_host.py.

``loo_ard_closed_form`` is written the per-point way (Rasmussen & Williams 5.4.2 differentiated, one explicit derivative matrix D_k per
feature: the formulae of ``test_loo_grad_host.loo_grad_closed_form``), which is independent of the adjoint form the device uses
    d score = sum_ij G_ij D_ij,   G = 1/2 (v a^T + a v^T) + P diag(gamma) P + eps a a^T.
The adjoint enters the reference only as the error SCALE: S_k = sum_ij |G_ij h_ij (u_ik - u_jk)^2| for a feature, sn~ sum_i |G_ii| for the
noise -- the gradient vanishes at an optimum and is no scale for itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O
from test_ard_host import ard_scales
from test_loo_grad_host import dk_tilde, k_tilde, loo_grad_closed_form
from test_loo_host import loo_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOO_ARD_SYMBOLS = {"sigp_loo_grad_ard": 10}
CRITERIA = ("nlpd", "sse")


def ard_k_tilde(kind, X, ells, sn):
    U = np.asarray(X, dtype=np.float64) / np.asarray(ells, dtype=np.float64)
    return O.cov_unit(kind, U, U, 1.0) + sn * np.eye(U.shape[0])


def loo_adjoint(P, y, mode, crit):
    """G = d score / d K~ (symmetric) of the leave-one-out score ``crit`` ('nlpd' | 'sse') in sigma mode ``mode`` ('refit' | 'fixed')"""
    n = len(y)
    a = P @ y
    g = np.diag(P).copy()
    q = float(y @ a)
    r = a / g
    if crit == "sse":
        beta, gamma, eps = -2 * r / g, 2 * r * a / g ** 2, 0.0
    else:
        s = (q - a * r) / (n - 1) if mode == "refit" else np.full(n, q / n)
        var = s / g
        kappa, rho = 1 / (2 * var) - r * r / (2 * var ** 2), r / var
        beta = -rho / g
        gamma = kappa * s / g ** 2 + rho * a / g ** 2
        eps = -np.sum(kappa / g) / ((n - 1) if mode == "refit" else n)
        if mode == "refit":
            beta = beta + 2 * kappa * a / (g ** 2 * (n - 1))
            gamma = gamma - kappa * a * a / (g ** 3 * (n - 1))
    v = P @ beta
    return 0.5 * (np.outer(v, a) + np.outer(a, v)) + (P * gamma) @ P + eps * np.outer(a, a)


def loo_ard_closed_form(kind, X, y, ells, sn, mode="refit", route="inv"):
    """dict(nlpd, sse, nlpd_grad [d + 1], sse_grad [d + 1], nlpd_S [d + 1], sse_S [d + 1], nlpd_adj [d + 1], sse_adj [d + 1]) at per-feature
    length scales ``ells`` and noise ``sn``: the scores, their derivatives with respect to (log l_1 .. log l_d, log sn~) the per-point way,
    the error scales, and (``*_adj``) the same derivatives through the adjoint.  P = K~^-1 comes from the explicit inverse (route 'inv') or
    from the Cholesky factor as U U^T with U = L~^-T (route 'chol': the device's own route)."""
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
    g = np.diag(P).copy()
    q = float(y @ a)
    r = a / g
    s = (q - a * a / g) / (n - 1) if mode == "refit" else np.full(n, q / n)
    var = s / g
    out = dict(nlpd=float(np.sum(0.5 * np.log(2 * np.pi * var) + r * r / (2 * var))), sse=float(np.sum(r * r)))
    G = {c: loo_adjoint(P, y, mode, c) for c in CRITERIA}
    for c in CRITERIA:
        for key in ("grad", "S", "adj"):
            out["%s_%s" % (c, key)] = np.zeros(d + 1)
    for k in range(d + 1):
        D = h * (U[:, k][:, None] - U[:, k][None, :]) ** 2 if k < d else sn * np.eye(n)
        t = D @ a
        b = P @ t
        e = float(a @ t)
        c = np.einsum("ij,ij->i", P @ D, P)
        dr = -b / g + a * c / g ** 2
        ds = (-e + 2 * a * b / g - a * a * c / g ** 2) / (n - 1) if mode == "refit" else np.full(n, -e / n)
        dvar = ds / g + s * c / g ** 2
        out["nlpd_grad"][k] = np.sum(dvar / (2 * var) + r * dr / var - r * r * dvar / (2 * var ** 2))
        out["sse_grad"][k] = np.sum(2 * r * dr)
        for crit in CRITERIA:
            out[crit + "_S"][k] = np.sum(np.abs(G[crit] * D))
            out[crit + "_adj"][k] = np.sum(G[crit] * D)
    return out


def test_loo_ard_entry_point_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in LOO_ARD_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"SIGP_LOO_NLPD\s*=\s*0\s*,\s*SIGP_LOO_SSE\s*=\s*1", hdr)
    assert L.LOO_CRITERION_IDS == {"loo_nlpd": 0, "loo_sse": 1}
    assert L.load().sigp_version() >= 560


def test_loo_ard_null_handle_is_rejected_and_the_python_surface_exists():
    import inspect

    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.zeros(4)
    assert lib.sigp_loo_grad_ard(None, 1, L.ptr(a), 4, 0, 0, None, None, L.ptr(a), L.ptr(a)) == L.BAD_ARG
    assert callable(getattr(S.GPR, "loo_ard", None)) and callable(getattr(S.GPR, "optimize_ard", None))
    p = inspect.signature(S.GPR.loo_ard).parameters
    assert (p["criterion"].default, p["sigma_f"].default, p["grad"].default, p["predictions"].default) == ("loo_nlpd", "refit", "exact", False)
    p = inspect.signature(S.GPR.optimize_ard).parameters
    assert (p["criterion"].default, p["sigma_f"].default, p["method"].default, p["grad"].default) == ("nlml", "refit", "L-BFGS-B", "exact")


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d", [(37, 3), (129, 8)])
def test_closed_form_equals_central_differences(kind, n, d):
    X, y, _ = O.synthetic_problem(n, d, 20251700 + 7 * n + d)
    ells, sn, h = ard_scales(d, 20251800 + 7 * n + d), 1e-2, 1e-5
    th = np.concatenate([np.log(ells), [np.log(sn)]])
    for mode in ("refit", "fixed"):
        ref = loo_ard_closed_form(kind, X, y, ells, sn, mode)
        at = loo_closed_form(ard_k_tilde(kind, X, ells, sn), y, mode)
        for crit in CRITERIA:
            assert abs(ref[crit] - at[crit]) <= 1e-10 * abs(at[crit]), (mode, crit)
        num = {c: np.zeros(d + 1) for c in CRITERIA}
        for p in range(d + 1):
            v = []
            for sgn in (1.0, -1.0):
                t = th.copy(); t[p] += sgn * h
                v.append(loo_closed_form(ard_k_tilde(kind, X, np.exp(t[:d]), np.exp(t[d])), y, mode))
            for crit in CRITERIA:
                num[crit][p] = (v[0][crit] - v[1][crit]) / (2 * h)
        for crit in CRITERIA:
            err = np.abs(ref[crit + "_grad"] - num[crit]) / ref[crit + "_S"]
            print("%s n=%d d=%d %s %s: error / S %s" % (kind, n, d, mode, crit, err))
            assert np.all(err <= 1e-7), (kind, n, d, mode, crit, err)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("mode", ["refit", "fixed"])
def test_equal_scales_give_the_isotropic_gradient(kind, mode):
    """sum_k d/dlog l_k = d/dlog l at l_1 = .. = l_d = l; both sides are the same sums in another order, so they agree to rounding
    (1e-10 of the isotropic form's own scale S = sum_i |per-point term| leaves three digits for the order of the sums)"""
    n, d = 129, 8
    X, y, _ = O.synthetic_problem(n, d, 20251200)
    ell, sn = np.sqrt(8.0), 1e-2
    ard = loo_ard_closed_form(kind, X, y, np.full(d, ell), sn, mode)
    iso = loo_grad_closed_form(k_tilde(kind, X, ell, sn), dk_tilde(kind, X, ell, sn), y, mode)
    for crit in CRITERIA:
        assert abs(np.sum(ard[crit + "_grad"][:d]) - iso[crit + "_grad"][0]) <= 1e-10 * iso[crit + "_S"][0], (crit, "length scale")
        assert abs(ard[crit + "_grad"][d] - iso[crit + "_grad"][1]) <= 1e-10 * iso[crit + "_S"][1], (crit, "noise")


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_adjoint_form_equals_the_per_point_form_and_both_routes_agree(kind):
    """What the device computes (the contraction with G) against the per-point chain rule, and the two routes to P = K~^-1 whose difference
    / S is the GPU tests' measure of the reference's own error.  Rounding only: 1e-10 S."""
    n, d = 129, 8
    X, y, _ = O.synthetic_problem(n, d, 20251301)
    ells = ard_scales(d, 20251302)
    for mode in ("refit", "fixed"):
        a = loo_ard_closed_form(kind, X, y, ells, 1e-2, mode, "inv")
        b = loo_ard_closed_form(kind, X, y, ells, 1e-2, mode, "chol")
        for crit in CRITERIA:
            S = a[crit + "_S"]
            assert np.all(np.abs(a[crit + "_adj"] - a[crit + "_grad"]) <= 1e-10 * S), (mode, crit)
            assert np.all(np.abs(a[crit + "_grad"] - b[crit + "_grad"]) <= 1e-10 * S), (mode, crit)
