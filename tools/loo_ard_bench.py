"""The per-feature (ARD) gradient of a leave-one-out score beside the calls it competes with, on one GPU through the product library (no
torch), modelled on tools/ard_bench.py and tools/loo_grad_bench.py:

  single fits (RBF, fp64; default n = 4096 8192, d = 8 64) at equal length scales, so that every call factors the same matrix: `refit`,
      `loo()` and `loo(grad=True)` on that fit (two hyper-parameters: the yardstick, code this gradient does not touch), `nlml_ard` and
      `loo_ard` (d + 1 hyper-parameters; both fit first) -- host clock around calls that are synchronous on return, bracketed by
      sigp_synchronize; every shape warmed up, then `--reps` repeats with the calls ALTERNATING inside each repeat; median and best reported.
  the SIGP_KC_MLII device time of one call of each (HIP events from sigp_profile, a pass of its own) and the covariance-build class of one
      `loo(grad=True)` (its dK~ build).  sigp_profile gives class totals, so the steps are split by differences:
          ARD tile pass        = mlii(nlml_ard) - mlii(nlml(grad="exact"))         (both: triangular inversion + U U^T, then the pass)
          gradient work        = mlii(loo_ard) - mlii(loo_ard(grad=None))          (U U^T, the n^2 passes, the product M, the tile pass)
      By flop count mlii(loo_ard) = mlii(loo(grad=True)) + the ARD tile pass (the dK~ build is in another class): `model` holds that sum
      and the measured ratio to it; `ratio_loo_ard_over_fit_plus_loo_grad` is the wall-clock ratio against the same work done the old way
      for ONE direction (refit + loo(grad=True)), `ratio_loo_ard_over_loo_grad` the plain quotient of the two calls.

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r11_loo_ard_bench.json)."""
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


def classes(gp, fn, names=("mlii",)):
    gp.profile_reset(); gp.profile(True, list(names))
    fn()
    p = gp.profile_get()
    gp.profile(False)
    return {c: {"ms": p[c]["ms"], "launches": p[c]["launches"], "flops": p[c]["flops"]} for c in names}


def single(n, d, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th = np.log([ell, sn])
    th_ard = np.log([ell] * d + [sn])
    calls = {"fit": lambda gp: gp.refit(ell, sn), "loo_after_fit": lambda gp: gp.loo(), "loo_grad_after_fit": lambda gp: gp.loo(grad=True),
             "nlml_ard": lambda gp: gp.nlml_ard(th_ard), "loo_ard": lambda gp: gp.loo_ard(th_ard), "loo_ard_value_only": lambda gp: gp.loo_ard(th_ard, grad=None)}
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, fn in calls.items():            # (`fit` comes first: the two calls after it run on an isotropic fit of the same matrix)
                t = timed(gp, lambda: fn(gp))
                if r >= 2:
                    ms[k].append(t)
        gp.refit(ell, sn)
        iso = gp.loo(grad=True)
        p_loo = classes(gp, lambda: gp.loo())
        p_loo_grad = classes(gp, lambda: gp.loo(grad=True), ("mlii", "kbuild"))
        p_nlml = classes(gp, lambda: gp.nlml(th, grad="exact"))
        p_nlml_ard = classes(gp, lambda: gp.nlml_ard(th_ard))
        v_ard, g_ard = gp.loo_ard(th_ard)
        p_loo_ard = classes(gp, lambda: gp.loo_ard(th_ard))
        p_loo_ard_value = classes(gp, lambda: gp.loo_ard(th_ard, grad=None))
    out = summary(ms)
    out["mlii_class"] = {"loo": p_loo["mlii"], "loo_grad": p_loo_grad["mlii"], "nlml_exact": p_nlml["mlii"], "nlml_ard": p_nlml_ard["mlii"],
                         "loo_ard": p_loo_ard["mlii"], "loo_ard_value_only": p_loo_ard_value["mlii"]}
    out["kbuild_class_of_one_loo_grad"] = p_loo_grad["kbuild"]
    pass_ms = p_nlml_ard["mlii"]["ms"] - p_nlml["mlii"]["ms"]
    want = p_loo_grad["mlii"]["ms"] + pass_ms
    out["model"] = {"ard_tile_pass_ms": pass_ms, "gradient_work_ms": p_loo_ard["mlii"]["ms"] - p_loo_ard_value["mlii"]["ms"],
                    "expected_mlii_of_loo_ard_ms": want, "measured_over_expected": p_loo_ard["mlii"]["ms"] / want,
                    "note": "flop model: mlii(loo_ard) = mlii(loo(grad=True)) + the ARD tile pass; the pass = mlii(nlml_ard) - mlii(nlml exact)"}
    out["ratio_loo_ard_over_loo_grad"] = out["loo_ard"]["median_ms"] / out["loo_grad_after_fit"]["median_ms"]
    out["ratio_loo_ard_over_fit_plus_loo_grad"] = out["loo_ard"]["median_ms"] / (out["fit"]["median_ms"] + out["loo_grad_after_fit"]["median_ms"])
    # the same matrix either way: the d length-scale components add up to the isotropic one (a check of the run, not a tolerance)
    out["check"] = {"nlpd_iso": float(iso["nlpd"]), "nlpd_ard": float(v_ard), "dlogl_iso": float(iso["nlpd_grad"][0]), "sum_dlogl_ard": float(np.sum(g_ard[:d])),
                    "dlogsn_iso": float(iso["nlpd_grad"][1]), "dlogsn_ard": float(g_ard[d])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "loo_ard_bench", "kernel": "rbf", "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["single"] = {"n=%d d=%d" % (n, d): single(n, d, a.reps) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
