"""CPU tier of the conditioning tests: the long-double reference (tests/hp_reference.py) is pinned against LAPACK, and the inputs of
tests/test_hip_conditioning.py are checked to be what that file says they are -- cond(K~) in its decade, factorable by LAPACK, every
LAPACK quantity finite.  These are conditions on the INPUTS: if one fails the input is to be replaced, not the bound.  ``-s`` prints the
table of cond(K~), cond of the leading 128-block and LAPACK's own rho / eta / forward errors per input (docs/EXPERIMENTS.md keeps a copy).
"""
import numpy as np
import pytest

import hp_reference as H
from oracle import gp_oracle as O

pytestmark = pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")

A_CASES = [("A", kind, n, sn) for kind in ("rbf", "matern52") for n in H.A_SIZES for sn in H.A_LEVELS]
B_CASES = [("B", "spectrum", n, p) for n in H.B_SIZES for p in H.B_LEVELS]


def host_input(family, kind, n, level):
    """(K~, y, sn~, dK, k* rows, k**, decade of cond) with K~ from the oracle's covariance function (the device builds its own)"""
    if family == "A":
        X, y, ride, gen = H.family_a(n)
        Xs = np.vstack([ride, gen])
        ks, kss = H.cross_a(kind, X, Xs)
        sn = H.roundtrip(level)
        return O.cov_unit(kind, X, X, H.ELL_A) + sn * np.eye(n), y, sn, H.dk_a(kind, X), ks, kss, H.A_DECADE[level]
    K, dK, y, ride, gen = H.family_b(n, p=level)
    ks, kss = H.cross_b(K, np.vstack([ride, gen]))
    return K, y, 0.0, dK, ks, kss, (10.0 ** (level - 0.5), 10.0 ** (level + 0.5))


def test_hp_solver_on_a_matrix_with_a_known_factor():
    """integers: L L^T is exact in fp64, so the hp factor, solve, inverse and log det must be exact to long-double rounding"""
    rng = np.random.default_rng(1)
    n = 40
    L0 = np.tril(rng.integers(-3, 4, (n, n))).astype(np.float64)
    L0[np.arange(n), np.arange(n)] = rng.integers(1, 5, n)
    K = L0 @ L0.T
    x0 = rng.integers(-5, 6, n).astype(np.float64)
    L, piv = H.cholesky(K)
    assert H.err(L, L0) <= 1e-15 and H.err(piv, np.diag(L0) ** 2) <= 1e-14
    P = H.inverse(L)                       # (small integer triangles are badly conditioned: the bounds scale with |K^-1| |K|)
    growth = n * float(np.finfo(H.LD).eps) * float(np.max(np.abs(P))) * float(np.max(np.abs(K)))
    assert H.err(H.backward(L, H.forward(L, K @ x0)), x0) <= 64 * growth * float(np.max(np.abs(x0)))
    assert H.err(P @ K.astype(H.LD), np.eye(n)) <= 64 * growth
    assert H.rho(L0, K) == 0.0 and H.eta(K, x0, K @ x0) == 0.0
    with pytest.raises(H.NotSPD) as e:
        K[6, 6] -= 2 * L0[6, 6] ** 2
        H.cholesky(K)
    assert e.value.info == 7 and len(e.value.pivots) == 7


@pytest.mark.parametrize("family,kind,n,level", A_CASES + B_CASES)
def test_inputs_are_in_their_decade_and_the_reference_agrees_with_lapack(family, kind, n, level):
    K, y, sn, dK, ks, kss, (lo, hi) = host_input(family, kind, n, level)
    assert np.array_equal(K, K.T)
    c = H.cond2(K)
    c11 = H.cond2(K[:128, :128])
    assert lo <= c < hi, (c, lo, hi)
    la = H.lapack_fit(K, y, sn, dK=dK, ks=ks, kss=kss)            # np.linalg.cholesky succeeds, or this raises
    hp = H.hp_fit(K, y, sn, dK=dK, ks=ks, kss=kss)
    assert float(np.min(np.diag(hp["L"]) ** 2)) > 0
    for k, v in la.items():
        assert np.all(np.isfinite(v)), k
    amax = float(np.max(np.abs(hp["alpha"])))
    fwd = H.err(la["alpha"], hp["alpha"]) / amax
    assert fwd <= 64 * c * H.U, (fwd, c)
    # the reference itself: backward stable in ITS arithmetic (2048 times below fp64's unit)
    assert H.rho(hp["L"], K) <= 64 * float(np.finfo(H.LD).eps) and H.eta(K, hp["alpha"], y) <= 64 * float(np.finfo(H.LD).eps)
    r, e = H.rho(la["L"], K), H.eta(K, la["alpha"], y)
    assert r <= 1e-15 * np.sqrt(n) and e <= 64 * H.U
    print("\n%s %-8s n=%3d level=%-6g cond=%.2e cond11=%.2e minpiv=%.1e | LAPACK rho=%.1e eta=%.1e fwd(alpha)=%.1e sf=%.1e nlml=%.1e mean=%.1e "
          "var=%.1e loo=%.1e/%.1e cv=%.1e/%.1e grad=%.1e/%.1e" % (
              family, kind, n, level, c, c11, float(np.min(np.diag(hp["L"]) ** 2)), r, e, fwd, H.err(la["sigma_f"], hp["sigma_f"]),
              H.err(la["nlml"], hp["nlml"]), H.err(la["mean"], hp["mean"]), H.err(la["var"], hp["var"]), H.err(la["loo_mean"], hp["loo_mean"]),
              H.err(la["loo_var"], hp["loo_var"]), H.err(la["cv_mean"], hp["cv_mean"]), H.err(la["cv_var"], hp["cv_var"]),
              abs(float(la["grad"][0] - hp["grad"][0])), abs(float(la["grad"][1] - hp["grad"][1]))))


@pytest.mark.parametrize("family,kind,n,level", [("A", "rbf", 257, 1e-4), ("A", "matern52", 257, 1e-11), ("A", "rbf", 640, 1e-11), ("B", "spectrum", 257, 14)])
def test_hp_closed_forms_equal_real_hp_refits_without_the_window(family, kind, n, level):
    """the leave-one-out and leave-block-out closed forms of the reference against REAL long-double refits without the window (a few folds:
    first, one across row 128, last -- a refit is 0.25 s at n = 640), to the reference's own forward error 64 cond eps_ld"""
    K, y, sn, dK, ks, kss, _ = host_input(family, kind, n, level)
    hp = H.hp_fit(K, y, sn)
    tol = 64 * H.cond2(K) * float(np.finfo(H.LD).eps)
    folds = H.cv_folds(n, 5)
    for f in (0, 25, len(folds) - 1):
        r0, r1, c0, c1 = folds[f]
        mean, var = H.hp_refit_without(K, y, sn, r0, r1, c0, c1)
        assert H.err(mean, hp["cv_mean"][c0:c1]) <= tol * max(1.0, float(np.max(np.abs(y))))
        assert H.err(var, hp["cv_var"][c0:c1]) <= tol * float(np.max(np.abs(hp["cv_var"])))
    for i in (0, 128, n - 1):
        mean, var = H.hp_refit_without(K, y, sn, i, i + 1, i, i + 1)
        assert H.err(mean, hp["loo_mean"][i:i + 1]) <= tol * max(1.0, float(np.max(np.abs(y))))
        assert H.err(var, hp["loo_var"][i:i + 1]) <= tol * float(np.max(np.abs(hp["loo_var"])))


def test_edge_inputs_are_what_they_claim():
    """near the edge of definiteness: the hp Cholesky decides what the fp64 matrix IS (LAPACK may answer either way there); the member built
    with a negative eigenvalue must be indefinite as an fp64 matrix, the ones with lambda_min >= 1e-15 definite"""
    n = 257
    for lam in H.B_EDGE:
        K = H.family_b(n, lam_min=lam)[0]
        try:
            minpiv = float(np.min(H.cholesky(K)[1]))
        except H.NotSPD as e:
            minpiv = float(e.pivots[-1])
        try:
            np.linalg.cholesky(K)
            lapack = "factors"
        except np.linalg.LinAlgError:
            lapack = "LinAlgError"
        print("\nB edge n=%d lambda_min=%-8g hp min squared pivot=%.2e  LAPACK %s" % (n, lam, minpiv, lapack))
        assert (minpiv <= 0) if lam < 0 else (minpiv > 0 or lam < 1e-15)
    X, y, _, _ = H.family_a(n)
    for kind in ("rbf", "matern52"):
        K = O.cov_unit(kind, X, X, H.ELL_A) + H.A_EDGE * np.eye(n)
        print("\nA edge %s n=%d sn~=%g cond=%.2e hp min squared pivot=%.2e" % (kind, n, H.A_EDGE, H.cond2(K), float(np.min(H.cholesky(K)[1]))))
