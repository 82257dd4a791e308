"""The refined block solve (option ``accurate_solve``, csrc/refined_solve.hpp) restated in NumPy, and the operands of its tests
(tests/test_refined_solve_host.py, tests/test_hip_refined_solve.py, tests/test_hip_accurate_solve.py).

The engine never substitutes: every triangular solve is a product with an explicitly inverted 128 x 128 diagonal block W = inv(L).  The
emulation below runs the same blocked algorithm in fp64 -- a right-looking Cholesky on 128-blocks whose rows below a diagonal block are
``A21 @ W.T``, then z = L~^-1 y and alpha~ = L~^-T z block by block through the same inverses -- with ``steps`` residual-correction steps

    X1 = A W^T,   R = A - X1 L^T,   X = X1 + R W^T          (forward;  the backward direction: X1 = A W, R = A - X1 L, X = X1 + R W)

behind every such product.  steps = 0 is the engine as it stands, steps = 1 what the option switches on.  The diagonal blocks are LAPACK's
(the device's diagonal-block kernel is at LAPACK's residual whatever the conditioning: tests/test_hip_conditioning.py), W comes from
fp64 substitution on the identity.  It pins the yardstick and the claim "one step suffices" independently of any device.
"""
import numpy as np
from scipy.linalg import solve_triangular

import hp_reference as H
from oracle import gp_oracle as O

NB = 128
TILE = 32                                         # rows per workgroup of refined_solve_kernel (RS_TM)
LEVELS = H.A_LEVELS + (H.A_EDGE,)                 # sn~ = 1e-4, 1e-8, 1e-11 and the edge 1e-13
KINDS = ("rbf", "matern52")
CASES = [(kind, n, lv) for kind in KINDS for n in H.A_SIZES for lv in LEVELS]


def matrix_a(kind, n, level):
    """(K~, y) of family A on the host: k(X, X) + sn~ I"""
    X, y, _, _ = H.family_a(n)
    return O.cov_unit(kind, X, X, H.ELL_A) + H.roundtrip(level) * np.eye(n), y


def refined(A, W, L, steps=1, trans=False):
    """A inv(L)^T (trans: A inv(L)) as a product with W = inv(L) and ``steps`` correction steps against the lower triangle of L, in the
    arithmetic of ``A`` (fp64 for the emulation; long double where a test wants the exact product of the given operands)"""
    Lt = np.tril(L)
    Wm, Lm = (W, Lt) if trans else (W.T, Lt.T)
    X = A @ Wm
    for _ in range(steps):
        X = X + (A - X @ Lm) @ Wm
    return X


def block_inverse(L):
    return solve_triangular(L, np.eye(L.shape[0]), lower=True)


def blocked_fit(K, y, steps):
    """(L~, alpha~) of the emulated engine; np.linalg.LinAlgError where a diagonal block is not positive definite (the device's NOT_SPD)"""
    n = K.shape[0]
    M = np.tril(K).astype(np.float64)
    edges = list(range(0, n, NB)) + [n]
    Ws = []
    for b0, b1 in zip(edges[:-1], edges[1:]):
        M[b0:b1, b0:b1] = np.linalg.cholesky(M[b0:b1, b0:b1] + np.tril(M[b0:b1, b0:b1], -1).T)
        Ws.append(block_inverse(M[b0:b1, b0:b1]))
        if b1 < n:
            M[b1:, b0:b1] = refined(M[b1:, b0:b1], Ws[-1], M[b0:b1, b0:b1], steps)
            M[b1:, b1:] -= np.tril(M[b1:, b0:b1] @ M[b1:, b0:b1].T)
    z = np.array(y, dtype=np.float64)[None, :]                       # a row, as the ride block carries it
    blocks = list(zip(edges[:-1], edges[1:]))
    for k, (b0, b1) in enumerate(blocks):                            # z <- z L~^-T
        z[:, b0:b1] = refined(z[:, b0:b1], Ws[k], M[b0:b1, b0:b1], steps)
        if b1 < n:
            z[:, b1:] -= z[:, b0:b1] @ M[b1:, b0:b1].T
    for k, (b0, b1) in reversed(list(enumerate(blocks))):           # alpha~ <- z L~^-1
        z[:, b0:b1] = refined(z[:, b0:b1], Ws[k], M[b0:b1, b0:b1], steps, trans=True)
        if b0 > 0:
            z[:, :b0] -= z[:, b0:b1] @ M[b0:b1, :b0]
    return M, z[0]


def lapack_fit(K, y):
    L = np.linalg.cholesky(K)
    return L, solve_triangular(L.T, solve_triangular(L, y, lower=True), lower=False)


# ---- operands of the single-launch tests ----------------------------------------------------------------------------------------------
def leading_block(kind, level, n=384):
    """(K11, L, W): the leading 128-block of family A, its fp64 LAPACK factor, and inv(L) by long-double substitution rounded to fp64"""
    K, _ = matrix_a(kind, n, level)
    K11 = np.ascontiguousarray(K[:NB, :NB])
    L = np.linalg.cholesky(K11)
    W = np.tril(np.asarray(H.forward(np.asarray(L, dtype=H.LD), np.eye(NB, dtype=H.LD)), dtype=np.float64))
    return K11, L, W


def row_residual(X, L, A, trans=False):
    """(max_j |X L^T - A|_ij, u max_j (|X| |L^T|)_ij) per row i, in long double (trans: X L)"""
    Lt = np.tril(np.asarray(L, dtype=np.float64))
    Lm = Lt if trans else Lt.T
    R = H.hp_matmul(X, Lm) - np.asarray(A, dtype=H.LD)
    floor = H.U * (np.abs(X) @ np.abs(Lm))
    return np.max(np.abs(R), axis=1).astype(np.float64), np.max(floor, axis=1)


def substitution(A, L, trans=False):
    """X with X L^T = A (trans: X L = A) by fp64 substitution (LAPACK trtrs)"""
    Lt = np.tril(L)
    return solve_triangular(Lt.T, A.T, lower=False).T if trans else solve_triangular(Lt, A.T, lower=True).T
