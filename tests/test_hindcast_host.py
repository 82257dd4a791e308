"""CPU tier of the expanding-window hindcast validation (include/sigp.h: sigp_hindcast, sigp_hindcast_batch, sigp_hindcast_grad_ard): the
ABI is declared, exported and bound, and the NumPy closed forms that the GPU tests use as their yardsticks are pinned --
``hindcast_closed_form`` (the prefix identity: every origin's forecast from the one factor L~ and z = L~^-1 y) against brute-force refits on
every prefix through ``oracle.gp_oracle``, and ``hindcast_ard_closed_form`` (a FORWARD-mode derivative, dL = L Phi(L^-1 D L^-T),
dz = -L^-1 dL z, differentiated row by row, one explicit derivative matrix per feature) against central differences of the brute-force
score and, at equal scales, against the sum rule.

The device computes the gradient through the reverse-mode adjoint G = d score / d K~ (``hindcast_adjoint``).  The adjoint enters the
reference only as ``*_adj`` and as the error SCALE S_k = sum_ij |G_ij h_ij (u_ik - u_jk)^2| for a feature, sn~ sum_i |G_ii| for the noise:
the gradient vanishes at an optimum and is no scale for itself."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O
from test_ard_host import ard_scales

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINDCAST_SYMBOLS = {"sigp_hindcast": 7, "sigp_hindcast_batch": 13, "sigp_small_run_hindcast": 15, "sigp_hindcast_grad_ard": 12}
CRITERIA = ("nlpd", "sse")


def scored_rows(n, lead, min_train):
    """the rows t with s = t - lead + 1 >= min_train"""
    return np.arange(min_train + lead - 1, n)


def hindcast_closed_form(Kt, y, lead=1, min_train=1, mode="refit"):
    """dict(mean [n], var [n] (NaN where a row is not scored), nlpd, sse, scored) from L~ = chol(K~) and z = L~^-1 y alone"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = len(y)
    Lt = np.linalg.cholesky(Kt)
    z = solve_triangular(Lt, y, lower=True)
    mean, var = np.full(n, np.nan), np.full(n, np.nan)
    for t in scored_rows(n, lead, min_train):
        s = t - lead + 1
        r = float(Lt[t, s:t + 1] @ z[s:t + 1])
        w = float(Lt[t, s:t + 1] @ Lt[t, s:t + 1])
        sig = float(z[:s] @ z[:s]) / s if mode == "refit" else float(z @ z) / n
        mean[t], var[t] = y[t] - r, sig * w
    sc = scored_rows(n, lead, min_train)
    r = y[sc] - mean[sc]
    return dict(mean=mean, var=var, nlpd=float(np.sum(0.5 * np.log(2 * np.pi * var[sc]) + r * r / (2 * var[sc]))), sse=float(np.sum(r * r)), scored=sc)


def hindcast_brute_force(kind, X, y, ell, sn, lead=1, min_train=1, mode="refit", M=None):
    """the same by a real ``oracle.fit_predict`` on every prefix (M held for the reference kernel); mode 'fixed' rescales the refit's
    variance to the full fit's sigma_f"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = len(y)
    if kind == "netdiffusion" and M is None:
        M = O.laplacian_M(X)
    sf_full = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["sigma_f"]
    mean, var = np.full(n, np.nan), np.full(n, np.nan)
    for t in scored_rows(n, lead, min_train):
        s = t - lead + 1
        f = O.fit_predict(X[:s], y[:s], X[t:t + 1], ell, sn, kind=kind, M=M, ref_idiom=False)
        mean[t] = f["fmean"][0]
        var[t] = f["fvar"][0] if mode == "refit" else f["fvar"][0] * sf_full / f["sigma_f"]
    sc = scored_rows(n, lead, min_train)
    r = y[sc] - mean[sc]
    return dict(mean=mean, var=var, nlpd=float(np.sum(0.5 * np.log(2 * np.pi * var[sc]) + r * r / (2 * var[sc]))), sse=float(np.sum(r * r)), scored=sc)


def _rows(Lt, z, lead, min_train, mode):
    n = len(z)
    q = float(z @ z)
    out = []
    for t in scored_rows(n, lead, min_train):
        s = t - lead + 1
        r = float(Lt[t, s:t + 1] @ z[s:t + 1])
        w = float(Lt[t, s:t + 1] @ Lt[t, s:t + 1])
        sig = float(z[:s] @ z[:s]) / s if mode == "refit" else q / n
        out.append((t, s, r, w, sig))
    return out


def hindcast_adjoint(Lt, z, lead, min_train, mode, crit, parts=False):
    """G = d score / d K~ (symmetric) of the hindcast score ``crit`` ('nlpd' | 'sse') by the reverse-mode derivative of the Cholesky
    factorisation: the formulae of include/sigp.h, dense.  ``parts``: (G, U, C, |C|) with G = U C U^T and |C| the
    same assembly of the absolute values of the terms of A = L^T B - zbar z^T (its diagonal cancels: no scale for itself)."""
    n = len(z)
    B = np.zeros((n, n))
    zbar = np.zeros(n)
    for t, s, r, w, sig in _rows(Lt, z, lead, min_train, mode):
        var = sig * w
        kappa, rho = (1 / (2 * var) - r * r / (2 * var * var), r / var) if crit == "nlpd" else (0.0, 2 * r)
        B[t, s:t + 1] = rho * z[s:t + 1] + 2 * kappa * sig * Lt[t, s:t + 1]
        zbar[s:t + 1] += rho * Lt[t, s:t + 1]
        if mode == "refit":
            zbar[:s] += 2 * z[:s] * kappa * w / s
        else:
            zbar += 2 * z * kappa * w / n
    A = Lt.T @ B - np.outer(zbar, z)
    T = np.tril(A)
    T[np.diag_indices(n)] *= 0.5
    Cm = 0.5 * (T + T.T)
    U = solve_triangular(Lt, np.eye(n), lower=True).T
    G = U @ Cm @ U.T
    if not parts:
        return G
    Ta = np.tril(np.abs(Lt.T) @ np.abs(B) + np.outer(np.abs(zbar), np.abs(z)))
    Ta[np.diag_indices(n)] *= 0.5
    return G, U, Cm, 0.5 * (Ta + Ta.T)


def hindcast_ard_closed_form(kind, X, y, ells, sn, lead=1, min_train=1, mode="refit"):
    """dict(nlpd, sse, {nlpd,sse}_grad [d + 1], _S [d + 1], _adj [d + 1], {nlpd,sse}_G) at per-feature length scales ``ells`` and noise
    ``sn``: the scores, their derivatives with respect to (log l_1 .. log l_d, log sn~) in FORWARD mode, the error scales, the same
    derivatives through the adjoint, and the adjoint itself"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = X.shape
    U = X / np.asarray(ells, dtype=np.float64)
    D2 = O.sqdist(U, U)
    Kt = O.cov_unit(kind, U, U, 1.0) + sn * np.eye(n)
    if kind == "rbf":
        h = np.exp(-0.5 * D2)
    else:
        s5 = np.sqrt(5.0 * D2)
        h = (5.0 / 3.0) * (1.0 + s5) * np.exp(-s5)
    Lt = np.linalg.cholesky(Kt)
    z = solve_triangular(Lt, y, lower=True)
    rows = _rows(Lt, z, lead, min_train, mode)
    val = hindcast_closed_form(Kt, y, lead, min_train, mode)
    out = dict(nlpd=val["nlpd"], sse=val["sse"])
    G = {c: hindcast_adjoint(Lt, z, lead, min_train, mode, c) for c in CRITERIA}
    for c in CRITERIA:
        out[c + "_G"] = G[c]
        for key in ("grad", "S", "adj"):
            out["%s_%s" % (c, key)] = np.zeros(d + 1)
    for k in range(d + 1):
        D = h * (U[:, k][:, None] - U[:, k][None, :]) ** 2 if k < d else sn * np.eye(n)
        Y = solve_triangular(Lt, solve_triangular(Lt, D, lower=True).T, lower=True)       # L^-1 D L^-T
        Phi = np.tril(Y)
        Phi[np.diag_indices(n)] *= 0.5
        dL = Lt @ Phi
        dz = -solve_triangular(Lt, dL @ z, lower=True)
        dn = ds = 0.0
        for t, s, r, w, sig in rows:
            dr = float(dL[t, s:t + 1] @ z[s:t + 1] + Lt[t, s:t + 1] @ dz[s:t + 1])
            dw = 2 * float(Lt[t, s:t + 1] @ dL[t, s:t + 1])
            dsig = 2 * float(z[:s] @ dz[:s]) / s if mode == "refit" else 2 * float(z @ dz) / n
            var, dvar = sig * w, dsig * w + sig * dw
            dn += dvar / (2 * var) + r * dr / var - r * r * dvar / (2 * var * var)
            ds += 2 * r * dr
        out["nlpd_grad"][k], out["sse_grad"][k] = dn, ds
        for c in CRITERIA:
            out[c + "_S"][k] = np.sum(np.abs(G[c] * D))
            out[c + "_adj"][k] = np.sum(G[c] * D)
    return out


def _kt(kind, X, ell, sn, M=None):
    X = np.asarray(X, dtype=np.float64)
    St = O.sigma_tilde(O.laplacian_M(X) if M is None else M, ell) if kind == "netdiffusion" else None
    return O.cov_unit(kind, X, X, ell, St) + sn * np.eye(X.shape[0])


def test_hindcast_entry_points_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in HINDCAST_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"SIGP_HINDCAST_MAX_LEAD\s*=\s*128\s*,\s*SIGP_HINDCAST_SMALL_MAX_LEAD\s*=\s*32", hdr)
    assert (L.HINDCAST_MAX_LEAD, L.HINDCAST_SMALL_MAX_LEAD) == (128, 32)
    assert L.HINDCAST_CRITERION_IDS == {"hindcast_nlpd": 0, "hindcast_sse": 1}
    assert L.load().sigp_version() >= 610


def test_hindcast_null_handle_is_rejected_and_the_python_surface_exists():
    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.zeros(4)
    assert lib.sigp_hindcast(None, 1, 1, 0, L.ptr(a), L.ptr(a), L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_hindcast_batch(None, 0, 1, 1, L.ptr(a), L.ptr(a), 1, 1, 0, None, None, 0, L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_hindcast_grad_ard(None, 1, L.ptr(a), 4, 1, 1, 0, 0, None, None, L.ptr(a), L.ptr(a)) == L.BAD_ARG
    i1 = np.zeros(1, dtype=np.int64)
    assert lib.sigp_small_run_hindcast(None, 1, L.iptr(i1), L.ptr(a), L.ptr(a), 1, 2, 0, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    p = inspect.signature(S.SmallBatch.run).parameters
    assert p["hindcast"].default is None and "hindcast=dict(lead=1, min_train=2, sigma_f=" in S.SmallBatch.run.__doc__
    from seaiceextentforecasting_amd import retro
    p = inspect.signature(retro.retro_grid_search).parameters
    assert (p["criterion"].default, p["lead"].default, p["min_train"].default) == ("nlml", 1, 2)
    assert {"hindcast_nlpd", "hindcast_sse"} <= set(retro._CRITERIA) and "held fixed" in retro.retro_grid_search.__doc__
    with pytest.raises(ValueError, match="hindcast_nlpd"):
        retro.retro_grid_search("north_September", None, None, 0, 0, criterion="hindcast")      # refused before anything is touched
    p = inspect.signature(S.GPR.hindcast).parameters
    assert (p["lead"].default, p["min_train"].default, p["sigma_f"].default) == (1, None, "refit")
    p = inspect.signature(S.GPR.hindcast_batch).parameters
    assert (p["lead"].default, p["min_train"].default, p["first"].default, p["sigma_f"].default, p["group"].default, p["predictions"].default) == \
        (1, None, 0, "refit", 8, True)
    p = inspect.signature(S.GPR.hindcast_ard).parameters
    assert (p["lead"].default, p["min_train"].default, p["criterion"].default, p["sigma_f"].default, p["grad"].default, p["predictions"].default) == \
        (1, None, "hindcast_nlpd", "refit", "exact", False)
    p = inspect.signature(S.GPR.optimize_ard).parameters
    assert (p["criterion"].default, p["lead"].default, p["min_train"].default) == ("nlml", 1, None)
    assert "hindcast_nlpd" in S.GPR.optimize_ard.__doc__ and "max(2, d + 1)" in S.GPR.hindcast.__doc__


def _cases(n):
    return [c for c in {(1, 1), (1, 5), (3, 4), (n - 1, 1)} if c[1] + c[0] - 1 <= n - 1]


@pytest.mark.parametrize("kind", ["netdiffusion", "rbf", "matern52"])
@pytest.mark.parametrize("n", [2, 12, 37])
def test_closed_form_equals_refits_on_every_prefix(kind, n):
    """The prefix identity against real refits: 1e-10 of the scale of the data (|y| = O(1), variances O(sigma_f)); measured 7e-14."""
    d = 3 if n > 2 else 1
    X, y, _ = O.synthetic_problem(n, d, 20261000 + n)
    ell, sn = (0.05, 1.0) if kind == "netdiffusion" else (np.sqrt(float(d)), 1e-2)
    cases = _cases(n)
    assert cases
    for lead, mt in cases:
        for mode in ("refit", "fixed"):
            a = hindcast_closed_form(_kt(kind, X, ell, sn), y, lead, mt, mode)
            b = hindcast_brute_force(kind, X, y, ell, sn, lead, mt, mode)
            sc = a["scored"]
            assert np.array_equal(sc, b["scored"]) and len(sc) == n - (mt + lead - 1)
            assert np.all(np.isnan(np.delete(a["mean"], sc))) and np.all(np.isnan(np.delete(a["var"], sc)))
            ys = max(1.0, float(np.max(np.abs(y))))
            em = np.max(np.abs(a["mean"][sc] - b["mean"][sc])) / ys
            ev = np.max(np.abs(a["var"][sc] - b["var"][sc]) / b["var"][sc])
            print("%s n=%d lead=%d min_train=%d %s: mean %.2e var %.2e" % (kind, n, lead, mt, mode, em, ev))
            assert em <= 1e-10 and ev <= 1e-10, (kind, n, lead, mt, mode, em, ev)
            for c in CRITERIA:
                assert abs(a[c] - b[c]) <= 1e-10 * max(1.0, abs(b[c]), len(sc)), (kind, n, lead, mt, mode, c)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d", [(12, 2), (37, 3)])
def test_forward_mode_equals_central_differences_of_the_brute_force_score(kind, n, d):
    X, y, _ = O.synthetic_problem(n, d, 20261100 + 7 * n + d)
    ells, sn, h = ard_scales(d, 20261200 + 7 * n + d), 1e-2, 1e-5
    th = np.concatenate([np.log(ells), [np.log(sn)]])
    for lead, mt in ((1, 1), (5, 3)):
        for mode in ("refit", "fixed"):
            ref = hindcast_ard_closed_form(kind, X, y, ells, sn, lead, mt, mode)
            num = {c: np.zeros(d + 1) for c in CRITERIA}
            for p in range(d + 1):
                v = []
                for sgn in (1.0, -1.0):
                    t = th.copy(); t[p] += sgn * h
                    v.append(hindcast_brute_force(kind, X / np.exp(t[:d]), y, 1.0, np.exp(t[d]), lead, mt, mode))
                for c in CRITERIA:
                    num[c][p] = (v[0][c] - v[1][c]) / (2 * h)
            for c in CRITERIA:
                err = np.abs(ref[c + "_grad"] - num[c]) / ref[c + "_S"]
                print("%s n=%d d=%d lead=%d %s %s: error / S %s" % (kind, n, d, lead, mode, c, err))
                assert np.all(err <= 1e-7), (kind, n, d, lead, mt, mode, c, err)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("n,d", [(37, 3), (129, 8)])
def test_adjoint_equals_forward_mode(kind, n, d):
    """What the device computes (the contraction with G) against the independent forward-mode derivative: rounding only, 1e-10 S (measured
    2e-14); G is symmetric"""
    X, y, _ = O.synthetic_problem(n, d, 20261300 + 7 * n + d)
    ells = ard_scales(d, 20261400 + 7 * n + d)
    for lead, mt in ((1, 1), (5, 3)):
        for mode in ("refit", "fixed"):
            a = hindcast_ard_closed_form(kind, X, y, ells, 1e-2, lead, mt, mode)
            for c in CRITERIA:
                spread = np.abs(a[c + "_adj"] - a[c + "_grad"]) / a[c + "_S"]
                print("%s n=%d d=%d lead=%d %s %s: spread %s" % (kind, n, d, lead, mode, c, spread))
                assert np.all(spread <= 1e-10), (kind, n, d, lead, mt, mode, c, spread)
                assert np.allclose(a[c + "_G"], a[c + "_G"].T, rtol=0, atol=1e-12 * np.max(np.abs(a[c + "_G"])))


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("mode", ["refit", "fixed"])
def test_equal_scales_obey_the_sum_rule(kind, mode):
    """sum_k d/dlog l_k = d/dlog l at l_1 = .. = l_d = l: the forward-mode derivative along the common direction, and central differences of
    the closed-form score in log l"""
    n, d, lead, mt = 37, 3, 3, 4
    X, y, _ = O.synthetic_problem(n, d, 20261500)
    ell, sn, h = np.sqrt(3.0), 1e-2, 1e-5
    a = hindcast_ard_closed_form(kind, X, y, np.full(d, ell), sn, lead, mt, mode)
    for c in CRITERIA:
        v = [hindcast_closed_form(_kt(kind, X, ell * np.exp(sg * h), sn), y, lead, mt, mode)[c] for sg in (1.0, -1.0)]
        num = (v[0] - v[1]) / (2 * h)
        assert abs(np.sum(a[c + "_grad"][:d]) - num) <= 1e-7 * np.sum(a[c + "_S"][:d]), (c, np.sum(a[c + "_grad"][:d]), num)
