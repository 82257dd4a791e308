"""CPU tier: the blocked algorithm of the engine restated in NumPy (tests/refined_cases.py) on family A of tests/hp_reference.py, with 0
and 1 residual-correction steps behind every product with an inverted diagonal block.

  0 steps   reproduces the device's finding (docs/EXPERIMENTS.md "Conditioning"): the factor residual rho is more than 16 times LAPACK's at
            sn~ = 1e-8 on every kernel and size (measured here: 88 to 189), and at sn~ = 1e-13 a pivot of the second block goes negative
  1 step    every matrix factors, sn~ = 1e-13 included, and rho and the backward error eta of alpha~ are within 2 x LAPACK's on the same
            fp64 matrix (measured: rho 0.7 to 1.0, eta 0.7 to 1.3) -- so one step is enough, and the option has no second one

Both figures are formed in long double (hp_reference.rho / eta).  No device is involved: this pins the yardstick and the claim.
"""
import numpy as np
import pytest

import hp_reference as H
import refined_cases as RC

pytestmark = pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")

_LAPACK = {}


def lapack(kind, n, level):
    key = (kind, n, level)
    if key not in _LAPACK:
        K, y = RC.matrix_a(kind, n, level)
        L, alpha = RC.lapack_fit(K, y)
        _LAPACK[key] = (K, y, H.rho(L, K), H.eta(K, alpha, y))
    return _LAPACK[key]


@pytest.mark.parametrize("kind,n", [(k, n) for k in RC.KINDS for n in H.A_SIZES])
def test_without_a_correction_step_the_emulation_shows_the_loss(kind, n):
    K, y, rho_la, _ = lapack(kind, n, 1e-8)
    L, _ = RC.blocked_fit(K, y, steps=0)
    r = H.rho(L, K) / rho_la
    print("\n%s n=%d sn~=1e-8, 0 steps: rho ratio %.1f" % (kind, n, r))
    assert r > 16


@pytest.mark.parametrize("kind", RC.KINDS)
def test_without_a_correction_step_the_edge_level_is_refused(kind):
    """the emulated engine, like the device, meets a negative pivot in the block after the ill-conditioned one at sn~ = 1e-13"""
    K, y, _, _ = lapack(kind, 384, H.A_EDGE)
    with pytest.raises(np.linalg.LinAlgError):
        RC.blocked_fit(K, y, steps=0)


@pytest.mark.parametrize("kind,n,level", RC.CASES)
def test_one_correction_step_is_as_accurate_as_lapack(kind, n, level):
    K, y, rho_la, eta_la = lapack(kind, n, level)
    L, alpha = RC.blocked_fit(K, y, steps=1)                       # (raises where a block is not positive definite: every matrix must factor)
    rho, eta = H.rho(L, K), H.eta(K, alpha, y)
    print("\n%s n=%d sn~=%g, 1 step: rho %.3e (%.2f x LAPACK)  eta %.3e (%.2f x LAPACK)" % (kind, n, level, rho, rho / rho_la, eta, eta / eta_la))
    assert rho <= 2 * rho_la and eta <= 2 * eta_la


@pytest.mark.parametrize("trans", [False, True])
def test_the_correction_is_exact_algebra(trans):
    """with W = inv(L) exactly, R vanishes and the step changes nothing: in long double on a benign block X L^T = A to 1e-17"""
    rng = np.random.default_rng(5)
    L = np.tril(rng.standard_normal((RC.NB, RC.NB))) / 16 + 2 * np.eye(RC.NB)
    W = np.asarray(H.forward(np.asarray(L, dtype=H.LD), np.eye(RC.NB, dtype=H.LD)))
    A = np.asarray(rng.standard_normal((7, RC.NB)), dtype=H.LD)
    X = RC.refined(A, W, np.asarray(L, dtype=H.LD), 1, trans)
    Lm = np.asarray(np.tril(L) if trans else np.tril(L).T, dtype=H.LD)
    assert float(np.max(np.abs(X @ Lm - A))) <= 1e-16
