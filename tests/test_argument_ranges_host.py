"""CPU tier of tests/test_hip_argument_ranges.py: the yardsticks that file leans on where they are new -- the oracle's exact MLII
gradient at feature counts past one 64-column pad, the block closed form at an order whose folds need a second pass, and the pass
arithmetic of ``cv_launch`` (csrc/sigp_blockcv.inc) restated as a pure function of (folds, members) -- and the leave-one-out gradients'
closed form in extended precision, for problems whose cond(K~) leaves the fp64 closed form less accurate than the bound it serves."""
import os
import re

import numpy as np
import pytest

from oracle import gp_oracle as O
from scipy.linalg import solve_triangular

from test_cv_host import cv_closed_form, cv_folds, cv_problem
from test_loo_grad_host import dk_tilde, k_tilde, loo_grad_closed_form, problem
from test_loo_host import loo_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stationary_problem(n, d, m=3):
    """(X, y, Xs, ell, sn~) of the feature-count tests: ``O.synthetic_problem(n, d, 20250900 + d)``, l = sqrt(d), sn~ = 1e-2"""
    X, y, Xs = O.synthetic_problem(n, d, 20250900 + d, m=m)
    return X, y, Xs, float(np.sqrt(d)), 1e-2


def reference_problem(n, N, m=3):
    """(X, y, Xs, ell, sn~, M) of the reference-kernel tests: ``O.synthetic_problem(n, N, 20251000 + N + n, m=3)``, l = 0.05, sn~ = 1e-2"""
    X, y, Xs = O.synthetic_problem(n, N, 20251000 + N + n, m=m)
    return X, y, Xs, 0.05, 1e-2, O.laplacian_M(X)


def cv_pass_blocks():
    """CV_PASS_BLOCKS as csrc/sigp_blockcv.inc states it"""
    src = open(os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc", "sigp_blockcv.inc")).read()
    m = re.search(r"constexpr\s+long\s+CV_PASS_BLOCKS\s*=\s*(\d+)\s*;", src)
    assert m, "CV_PASS_BLOCKS is not defined in sigp_blockcv.inc"
    return int(m.group(1))


def cv_passes(F, nb, pass_blocks=1024):
    """[(f0, nf)]: the passes ``cv_launch`` works F folds of nb lockstep members off in -- FP = max(1, min(F, pass_blocks // nb)) folds
    per pass, the last one ragged"""
    FP = max(1, min(F, pass_blocks // nb))
    return [(f0, min(FP, F - f0)) for f0 in range(0, F, FP)]


def _refined_inverse(Kt, route):
    """K~^-1 in ``np.longdouble``: the fp64 inverse by ``route`` ('inv': explicit inverse; 'chol': U U^T with U = L~^-T, as
    ``loo_grad_closed_form`` takes them) and one Newton step P <- P + P (I - K~ P) in extended precision, which squares its error"""
    n = Kt.shape[0]
    if route == "inv":
        P = np.linalg.inv(Kt)
    else:
        U = solve_triangular(np.linalg.cholesky(Kt), np.eye(n), lower=True).T
        P = U @ U.T
    P, K = P.astype(np.longdouble), Kt.astype(np.longdouble)
    return P + P @ (np.eye(n, dtype=np.longdouble) - K @ P)


def _loo_grad_terms(P, dK_list, y):
    """what ``loo_grad_closed_form`` derives from P, y and each derivative matrix, in the precision of P: shared by the two modes"""
    a = P @ y
    g = np.diag(P).copy()
    per_d = []
    for D in dK_list:
        t = D @ a
        per_d.append((P @ t, a @ t, np.einsum("ij,ij->i", P @ D, P)))
    return a, g, y @ a, per_d


def _loo_grad_of_terms(terms, n, mode):
    """``test_loo_grad_host.loo_grad_closed_form`` from ``_loo_grad_terms``, formula for formula"""
    a, g, q, per_d = terms
    r = a / g
    s = (q - a * a / g) / (n - 1) if mode == "refit" else np.full(n, q / n)
    var = s / g
    out = dict(nlpd_grad=[], sse_grad=[], nlpd_S=[], sse_S=[])
    for b, e, c in per_d:
        dr = -b / g + a * c / g ** 2
        ds = (-e + 2 * a * b / g - a * a * c / g ** 2) / (n - 1) if mode == "refit" else np.full(n, -e / n)
        dvar = ds / g + s * c / g ** 2
        tn = dvar / (2 * var) + r * dr / var - r * r * dvar / (2 * var ** 2)
        ts = 2 * r * dr
        out["nlpd_grad"].append(np.sum(tn)); out["nlpd_S"].append(np.sum(np.abs(tn)))
        out["sse_grad"].append(np.sum(ts)); out["sse_S"].append(np.sum(np.abs(ts)))
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def loo_grad_reference(kind, X, y, ell, sn, M):
    """{mode: (closed form, spread [2 keys][2])} in the shape of ``test_hip_loo_grad._reference_of``, for ``test_hip_loo_grad._check``, with
    both routes to K~^-1 refined and everything after them evaluated in ``np.longdouble``.  The fp64 closed form's two routes differ by
    about cond(K~) x 1e-13 of S (1.3e-8 at N = 64, n = 300, cond 6e4: more than the 1e-8 that ``_check`` lets a reference have); these
    differ by about 1e-12."""
    Kt, dK = k_tilde(kind, X, ell, sn, M), dk_tilde(kind, X, ell, sn, M)
    yl, dKl = np.asarray(y, dtype=np.longdouble).reshape(-1), [D.astype(np.longdouble) for D in dK]
    terms = {route: _loo_grad_terms(_refined_inverse(Kt, route), dKl, yl) for route in ("inv", "chol")}
    out = {}
    for mode in ("refit", "fixed"):
        a, b = (_loo_grad_of_terms(terms[route], len(yl), mode) for route in ("inv", "chol"))
        out[mode] = (a, {k: np.abs(a[k] - b[k]) / a[k[:-4] + "S"] for k in ("nlpd_grad", "sse_grad")})
    return out


# ---- 1. the oracle's exact gradient past one pad ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [70, 130])
def test_oracle_exact_gradient_equals_central_differences_past_one_pad(kind, d):
    """Step and tolerance of tests/test_hip_parity.py::test_exact_gradient_matches_oracle_and_finite_differences (h = 1e-5, rtol 1e-5,
    atol 1e-6), at the theta the GPU tier evaluates."""
    X, y, _, ell, sn = stationary_problem(300, d)
    th = np.array([np.log(ell) + 0.2, np.log(sn)])
    f0, g0 = O.mlii(th, X, y, kind=kind, grad="exact")
    h = 1e-5
    fd = np.array([(O.mlii(th + h * e, X, y, kind=kind, grad="exact")[0] - O.mlii(th - h * e, X, y, kind=kind, grad="exact")[0]) / (2 * h) for e in np.eye(2)])
    print("%s d=%d: nlml %.9g  grad %s  central differences %s" % (kind, d, f0, g0, fd))
    assert np.isfinite(f0) and np.allclose(g0, fd, rtol=1e-5, atol=1e-6), (g0, fd)
    assert abs(g0[0]) >= 1.0            # a wrong d/dlog l cannot hide under an absolute tolerance of 1e-9


# ---- 2. the two closed forms at an order whose leave-one-out folds need a second pass -------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
def test_block_one_closed_form_is_the_leave_one_out_closed_form_at_n_1100(kind):
    """tolerance of tests/test_cv_host.py::test_block_one_is_leave_one_out"""
    n = 1100
    X, y, ell, sn, M = cv_problem(kind, n, 20250300 + n)
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    c = np.linalg.cond(Kt)
    assert c <= 1e6
    yv = np.asarray(y).reshape(-1)
    for mode in ("refit", "fixed"):
        cv, loo = cv_closed_form(Kt, yv, 1, 0, mode), loo_closed_form(Kt, yv, mode)
        e = max(np.max(np.abs(cv["mean"] - loo["mean"])) / np.max(np.abs(yv)), np.max(np.abs(cv["var"] / loo["var"] - 1)),
                abs(cv["nlpd"] - loo["nlpd"]) / abs(loo["nlpd"]), abs(cv["sse"] / loo["sse"] - 1))
        print("%s %s: cond(K~) %.3g  cv(1) against loo %.3g" % (kind, mode, c, e))
        assert e <= 1e-13


# ---- 3. the passes ---------------------------------------------------------------------------------------------------------------------
# (n, block, gap, members, the passes the GPU tier means to reach)
PASS_SHAPES = [(1100, 1, 0, 1, [(0, 1024), (1024, 76)]),
               (1300, 1, 3, 1, [(0, 1024), (1024, 276)]),
               (700, 2, 1, 3, [(0, 341), (341, 9)]),
               (300, 1, 0, 8, [(0, 128), (128, 128), (256, 44)])]


@pytest.mark.parametrize("n,block,gap,nb,want", PASS_SHAPES)
def test_passes_produce_every_fold_exactly_once(n, block, gap, nb, want):
    P = cv_pass_blocks()
    assert P == 1024
    folds = cv_folds(n, block, gap)
    F = len(folds)
    assert F == (n + block - 1) // block
    passes = cv_passes(F, nb, P)
    assert passes == want
    assert len(passes) >= 2 and all(1 <= nf and nf * nb <= P for _, nf in passes)
    seen = np.zeros(F, dtype=np.int64)
    scored = np.zeros(n, dtype=np.int64)
    for f0, nf in passes:
        for local in range(nf):                 # blockIdx.x of the pass: the window comes from f0 + blockIdx.x
            r0, r1, c0, c1 = folds[f0 + local]
            seen[f0 + local] += 1
            scored[c0:c1] += 1
            assert 0 <= r0 <= c0 < c1 <= r1 <= n and r1 - r0 <= block + 2 * gap
    assert np.all(seen == 1) and np.all(scored == 1)


def test_passes_of_a_single_pass_and_of_more_members_than_blocks():
    assert cv_passes(300, 1) == [(0, 300)]                      # the largest case of tests/test_hip_cv.py: one pass
    assert cv_passes(5, 8) == [(0, 5)]
    assert cv_passes(3, 2048) == [(0, 1), (1, 1), (2, 1)]       # 1024 // nb = 0: one fold per pass


# ---- 4. the leave-one-out gradients' closed form in extended precision ---------------------------------------------------------------------
def _fp64_closed_forms(kind, X, y, ell, sn, M, mode):
    Kt, dK = k_tilde(kind, X, ell, sn, M), dk_tilde(kind, X, ell, sn, M)
    return loo_grad_closed_form(Kt, dK, y, mode, "inv"), loo_grad_closed_form(Kt, dK, y, mode, "chol")


def test_refined_loo_gradient_reference_is_the_closed_form_where_that_is_accurate():
    """rbf, n = 129 (cond(K~) ~ 1e3): the fp64 closed form's routes agree to 1e-10 of S
    (tests/test_loo_grad_host.py::test_both_routes_to_the_inverse_agree), and the refined reference agrees with both as closely"""
    X, y, ell, sn, M = problem("rbf", 129, 20250229)
    ref = loo_grad_reference("rbf", X, y, ell, sn, M)
    for mode in ("refit", "fixed"):
        new, spread = ref[mode]
        for old in _fp64_closed_forms("rbf", X, y, ell, sn, M, mode):
            for k in ("nlpd_grad", "sse_grad"):
                S = k[:-4] + "S"
                e = np.abs(new[k] - old[k]) / old[S]
                print("rbf n=129 %s %s: refined against fp64 %s  spread %s" % (mode, k, e, spread[k]))
                assert np.all(e <= 1e-10) and np.all(spread[k] <= 1e-10)
                assert np.all(np.abs(new[S] / old[S] - 1.0) <= 1e-10)


def test_refined_loo_gradient_reference_where_the_fp64_closed_form_is_not_accurate_enough():
    """The reference kernel at N = 64, n = 300 (cond(K~) ~ 6e4): the refined routes agree to 1e-10 of S, well inside the 1e-8 that
    ``test_hip_loo_grad._check`` lets a reference's spread be, and the refined value lies as near each fp64 route as those lie to each
    other (twice their difference, plus the 1e-10)."""
    X, y, _, ell, sn, M = reference_problem(300, 64)
    ref = loo_grad_reference("netdiffusion", X, y, ell, sn, M)
    for mode in ("refit", "fixed"):
        new, spread = ref[mode]
        a, b = _fp64_closed_forms("netdiffusion", X, y, ell, sn, M, mode)
        for k in ("nlpd_grad", "sse_grad"):
            S = new[k[:-4] + "S"]
            old_spread = np.abs(a[k] - b[k]) / S
            e = np.maximum(np.abs(new[k] - a[k]), np.abs(new[k] - b[k])) / S
            print("netdiffusion N=64 n=300 %s %s: refined spread %s  fp64 spread %s  refined against fp64 %s" % (mode, k, spread[k], old_spread, e))
            assert np.all(spread[k] <= 1e-10)
            assert np.all(e <= 2.0 * old_spread + 1e-10)
