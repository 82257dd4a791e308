"""The per-feature (ARD) gradient beside the call it competes with, on one GPU through the product library (no torch), modelled on
tools/loo_grad_bench.py:

  single fits (RBF, fp64; default n = 4096 8192, d = 8 64): `refit`, `nlml(grad="exact")` (two hyper-parameters: the yardstick, code this
      gradient does not touch) and `nlml_ard` (d + 1 hyper-parameters, all from one pass over K~^-1) at equal length scales, so that both
      factor the same matrix -- host clock around calls that are synchronous on return, bracketed by sigp_synchronize; every shape warmed
      up, then `--reps` repeats with the calls ALTERNATING inside each repeat; median and best reported, their ratio, and the SIGP_KC_MLII
      share of one call of each from sigp_profile (HIP events, a pass of its own).

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r10_ard_bench.json)."""
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


def mlii_class(gp, fn):
    gp.profile_reset(); gp.profile(True, ["mlii"])
    fn()
    p = gp.profile_get()["mlii"]
    gp.profile(False)
    return {"ms": p["ms"], "launches": p["launches"], "flops": p["flops"]}


def single(n, d, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th = np.log([ell, sn])
    th_ard = np.log([ell] * d + [sn])
    calls = {"fit": lambda gp: gp.refit(ell, sn), "nlml_exact": lambda gp: gp.nlml(th, grad="exact"), "nlml_ard": lambda gp: gp.nlml_ard(th_ard)}
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, fn in calls.items():
                t = timed(gp, lambda: fn(gp))
                if r >= 2:
                    ms[k].append(t)
        v_iso, g_iso = gp.nlml(th, grad="exact")
        p_iso = mlii_class(gp, lambda: gp.nlml(th, grad="exact"))
        v_ard, g_ard = gp.nlml_ard(th_ard)
        p_ard = mlii_class(gp, lambda: gp.nlml_ard(th_ard))
    out = summary(ms)
    out["mlii_class_of_one_nlml_exact"], out["mlii_class_of_one_nlml_ard"] = p_iso, p_ard
    out["ratio_nlml_ard_over_nlml_exact"] = out["nlml_ard"]["median_ms"] / out["nlml_exact"]["median_ms"]
    # the same matrix either way: the d length-scale components add up to the isotropic one (a check of the run, not a tolerance)
    out["check"] = {"nlml_exact": float(v_iso), "nlml_ard": float(v_ard), "dlogl_exact": float(g_iso[0]), "sum_dlogl_ard": float(np.sum(g_ard[:d])),
                    "dlogsn_exact": float(g_iso[1]), "dlogsn_ard": float(g_ard[d])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "ard_bench", "kernel": "rbf", "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["single"] = {"n=%d d=%d" % (n, d): single(n, d, a.reps) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
