"""The leave-one-out gradient beside the calls it competes with, on one GPU through the product library (no torch), modelled on
tools/loo_bench.py:

  single fits (RBF, d = 8, fp64; default n = 4096 8192): `refit`, `loo()` after a fit, `nlml(grad="exact")` (which refits), `loo(grad=True)`
      after a fit, and the latter with the FULL product dK~ K~^-1 instead of the triangular one (set_option("loo_grad_tri", 0): the A/B of
      the cubic step) -- host clock around calls that are synchronous on return, bracketed by sigp_synchronize; every shape warmed up,
      then `--reps` repeats with the calls ALTERNATING inside each repeat; median and best reported, and the SIGP_KC_MLII share of one
      `loo(grad=True)` from sigp_profile (HIP events, a pass of its own);
  a lockstep group of 8 (`--group-n`, default 2048): `loo_batch`, `nlml_batch(grad="exact")`, `loo_batch(grad=True)`.

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "reps": len(v)} for k, v in ms.items()}


def single(n, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th = np.log([ell, sn])

    def full(gp):
        gp.set_option("loo_grad_tri", 0)
        try:
            gp.loo(grad=True)
        finally:
            gp.set_option("loo_grad_tri", 1)

    calls = {"fit": lambda gp: gp.refit(ell, sn), "loo_after_fit": lambda gp: gp.loo(), "nlml_exact": lambda gp: gp.nlml(th, grad="exact"),
             "loo_grad_after_fit": lambda gp: gp.loo(grad=True), "loo_grad_full_product_after_fit": full}
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, fn in calls.items():
                if k.endswith("after_fit"):
                    gp.refit(ell, sn)
                t = timed(gp, lambda: fn(gp))
                if r >= 2:
                    ms[k].append(t)
        gp.refit(ell, sn)
        gp.profile_reset(); gp.profile(True, ["mlii"])
        gp.loo(grad=True)
        p = gp.profile_get()["mlii"]
        gp.profile(False)
    out = summary(ms)
    out["mlii_class_of_one_loo_grad"] = {"ms": p["ms"], "launches": p["launches"], "flops": p["flops"], "tflops": p["flops"] / (p["ms"] * 1e-3) * 1e-12 if p["ms"] > 0 else None}
    f, g = out["fit"]["median_ms"], out["nlml_exact"]["median_ms"]
    out["model"] = {"nlml_exact_minus_fit_ms": g - f, "expected_loo_grad_after_fit_ms": 2.5 * (g - f),
                    "note": "flop model: trtri n^3/3 + U U^T n^3/3 (what nlml(grad='exact') adds to a fit) against those two plus the n^3 product"}
    return out


def group(n, G, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    Xb = np.zeros((G, n, d)); yb = np.zeros((G, n))
    for b in range(G):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240100 + b)
    ell, sn = np.full(G, np.sqrt(d)), np.full(G, 1e-2)
    th = np.log(np.stack([ell, sn], axis=1))
    ms = {"loo_batch": [], "nlml_batch_exact": [], "loo_grad_batch": []}
    with GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=G)
        calls = {"loo_batch": lambda: gp.loo_batch(ell, sn, group=G, predictions=False), "nlml_batch_exact": lambda: gp.nlml_batch(th, grad="exact", group=G),
                 "loo_grad_batch": lambda: gp.loo_batch(ell, sn, group=G, predictions=False, grad=True)}
        for r in range(2 + reps):
            for k, fn in calls.items():
                t = timed(gp, fn)
                if r >= 2:
                    ms[k].append(t)
    out = summary(ms)
    out.update(n=n, members=G)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--group-n", type=int, default=2048)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "loo_grad_bench", "kernel": "rbf", "d": 8, "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["single"] = {str(n): single(n, a.reps) for n in a.n}
    if a.group > 0:
        rec["lockstep_group"] = group(a.group_n, a.group, a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
