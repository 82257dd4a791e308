#!/usr/bin/env python3
"""How far do the hindcast variances of ONE ill-conditioned fit of tests/small_cases.py move under fp64 rounding alone?  (Host only, no GPU.)

For a case of the table and every hindcast setting of its batch, the relative error against long double of sigma_f sum_{j=s..t} L~(t,j)^2
  * from LAPACK's Cholesky (the comparator of tests/test_hip_small_flavours.py),
  * from a plain fp64 right-looking Cholesky by columns (the order of csrc/smallgp.hpp, without FMA),
  * from LAPACK on K~ with every entry perturbed by a random relative amount within one unit roundoff (median and maximum of --draws).
docs/EXPERIMENTS.md, "One-workgroup kernel: five flavours at every order", quotes the figures for the default case.

  python tools/small_hc_variance_spread.py [--n 49 --N 17 --sn 1e-6 --ell 0.7 --draws 20 --batch mid]"""
import argparse
import os
import sys

import numpy as np
from scipy.linalg import solve_triangular

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]

import hp_reference as H      # noqa: E402
import small_cases as SC      # noqa: E402


def row_variances(L, y, lead, min_train):
    z = solve_triangular(L, y, lower=True)
    n = len(y)
    sf = (z @ z) / n
    out = np.full(n, np.nan)
    for t in range(min_train + lead - 1, n):
        s = t - lead + 1
        out[t] = sf * (L[t, s:t + 1] @ L[t, s:t + 1])
    return out


def cholesky_right_looking(K):
    A = K.copy()
    for j in range(len(A)):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] *= 1.0 / A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=49)
    ap.add_argument("--N", type=int, default=17)
    ap.add_argument("--ell", type=float, default=0.7)
    ap.add_argument("--sn", type=float, default=1e-6)
    ap.add_argument("--draws", type=int, default=20)
    ap.add_argument("--batch", default="mid")
    a = ap.parse_args()
    c = [c for c in SC.TABLE if (c.n, c.N, c.ell, c.sn, c.expm) == (a.n, a.N, a.ell, a.sn, "eigh")][0]
    st = SC.staged(c)
    K = SC.build(st, c.ell, c.sn, SC.F64)[0]
    y = np.asarray(st[1])
    cond = H.cond2(K)
    print("%s: cond(K~) = %.3g, cond u = %.3g" % (c, cond, cond * SC.U))
    ref = SC.reference(c)
    rng = np.random.default_rng(0)
    for lead, mt in SC.batches()[a.batch].hc:
        want = ref["sigma_f"] * SC.hc_rows(ref, lead, mt, "fixed")["w"]
        ok = ~np.isnan(want.astype(np.float64))
        e = [SC._rel(row_variances(L, y, lead, mt)[ok], want[ok]) for L in (np.linalg.cholesky(K), cholesky_right_looking(K))]
        pert = []
        for _ in range(a.draws):
            Kp = np.tril(K * (1 + SC.U * rng.uniform(-1, 1, K.shape)))
            Kp = Kp + np.tril(Kp, -1).T
            pert.append(SC._rel(row_variances(np.linalg.cholesky(Kp), y, lead, mt)[ok], want[ok]))
        print("lead = %2d min_train = %2d:  LAPACK %.3g   right-looking %.3g   one-ulp perturbations of K~: median %.3g, max %.3g"
              % (lead, mt, e[0], e[1], np.median(pert), np.max(pert)))


if __name__ == "__main__":
    main()
