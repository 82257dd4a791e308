"""The expanding-window hindcast validation and its per-feature (ARD) gradient beside the calls they compete with, on one GPU through the
product library (no torch), modelled on tools/loo_ard_bench.py:

  single fits (RBF, fp64, d = 8; default n = 4096 8192) at equal length scales, so that every call factors the same matrix: `refit`, `loo()`
      and `hindcast()` at lead 1 and 5 on that fit, `loo_ard`, `hindcast_ard` at lead 1 and 5 and its value-only form (these fit first) --
      host clock around calls that are synchronous on return, bracketed by sigp_synchronize; every shape warmed up, then `--reps` repeats
      with the calls ALTERNATING inside each repeat; median, best and worst reported.  The yardsticks (`refit`, `loo`, `loo_ard`) are code
      this feature does not touch, timed in the same run.
  a lockstep group of 8 at n = 2048: `hindcast_batch` against `loo_batch`, scores only.
  the SIGP_KC_MLII device time (HIP events from sigp_profile, a pass of its own) of one call of `loo`, `loo_ard`, `hindcast`, `hindcast_ard`
      and `hindcast_ard(grad=None)`, and the per-step split of one `hindcast_ard` at lead 1 and 5 (one HIP-event bracket per step: the
      library prints every bracketed entry at set_option("host_timing", 2), and the tool reads them back from a redirected stderr, as
      tools/cv_ard_bench.py does): the scan, the row pass, the coefficients, zbar, the band, the triangular inversion, W = U C, G = U W^T,
      the ARD tile pass.
  the golden retro grid (north_September: 3 regions x years x a 4 x 4 grid, the reference kernel, one launch): `retro_grid_search` with
      criterion "hindcast_nlpd" against "loo_nlpd".

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r17_hindcast_bench.json)."""
import argparse
import json
import os
import re
import sys
import tempfile
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
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "worst_ms": float(np.max(v)), "reps": len(v)} for k, v in ms.items()}


def mlii(gp, fn):
    gp.profile_reset(); gp.profile(True, ["mlii"])
    fn()
    p = gp.profile_get()["mlii"]
    gp.profile(False)
    return {"ms": p["ms"], "launches": p["launches"], "flops": p["flops"]}


LAUNCH = re.compile(r"\[sigp-launch\] class (\d+) K (\d+) gflop ([0-9.eE+-]+) ms ([0-9.eE+-]+)")
STEPS = ("scan", "row_pass", "coefficients", "zbar", "band", "triangular_inversion", "w_scans_and_band_product", "product_g", "ard_tile_pass")


def steps(gp, fn):
    """the SIGP_KC_MLII entries of one hindcast_ard call, in launch order, by name"""
    gp.profile_reset(); gp.profile(True, ["mlii"]); gp.set_option("host_timing", 2)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
            gp.profile_get()                       # drains the events: the library prints them here
        finally:
            os.dup2(saved, 2); os.close(saved)
            gp.set_option("host_timing", 0); gp.profile(False)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    ent = [float(m.group(4)) for m in LAUNCH.finditer(text) if int(m.group(1)) == 7]
    if len(ent) != len(STEPS):
        return {"error": "expected %d entries, got %d" % (len(STEPS), len(ent))}
    return {nm + "_ms": ms for nm, ms in zip(STEPS, ent)}


def run_calls(gp, calls, reps):
    ms = {k: [] for k in calls}
    for r in range(2 + reps):                      # two warm-up rounds: every shape, every workspace allocated
        for k, fn in calls.items():
            t = timed(gp, fn)
            if r >= 2:
                ms[k].append(t)
    return summary(ms)


def single(n, d, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th = np.log([ell] * d + [sn])
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        calls = {"fit": lambda: gp.refit(ell, sn), "loo_after_fit": lambda: gp.loo(), "hindcast_lead1_after_fit": lambda: gp.hindcast(lead=1),
                 "hindcast_lead5_after_fit": lambda: gp.hindcast(lead=5), "loo_ard": lambda: gp.loo_ard(th), "hindcast_ard_lead1": lambda: gp.hindcast_ard(th, lead=1),
                 "hindcast_ard_lead5": lambda: gp.hindcast_ard(th, lead=5), "hindcast_ard_value_only": lambda: gp.hindcast_ard(th, lead=1, grad=None)}
        out = run_calls(gp, calls, reps)           # (`fit` comes first: the calls after it run on an isotropic fit of the same matrix)
        gp.refit(ell, sn)
        cls = {"loo": mlii(gp, lambda: gp.loo()), "hindcast_lead1": mlii(gp, lambda: gp.hindcast(lead=1)), "loo_ard": mlii(gp, lambda: gp.loo_ard(th)),
               "hindcast_ard_lead1": mlii(gp, lambda: gp.hindcast_ard(th, lead=1)), "hindcast_ard_lead5": mlii(gp, lambda: gp.hindcast_ard(th, lead=5)),
               "hindcast_ard_value_only": mlii(gp, lambda: gp.hindcast_ard(th, lead=1, grad=None))}
        out["steps_hindcast_ard_lead1"] = steps(gp, lambda: gp.hindcast_ard(th, lead=1))
        out["steps_hindcast_ard_lead5"] = steps(gp, lambda: gp.hindcast_ard(th, lead=5))
    out["mlii_class"] = cls
    out["gradient_work_ms"] = cls["hindcast_ard_lead1"]["ms"] - cls["hindcast_ard_value_only"]["ms"]
    out["ratio_hindcast_over_loo"] = out["hindcast_lead1_after_fit"]["median_ms"] / out["loo_after_fit"]["median_ms"]
    out["ratio_hindcast_ard_over_loo_ard"] = {"lead1": out["hindcast_ard_lead1"]["median_ms"] / out["loo_ard"]["median_ms"],
                                              "lead5": out["hindcast_ard_lead5"]["median_ms"] / out["loo_ard"]["median_ms"]}
    return out


def group(n, d, G, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    X, y, _ = O.synthetic_problem(n, d, 20240001)
    ells, sns = np.sqrt(d) * np.linspace(0.8, 1.5, G), np.full(G, 1e-2)
    with GPR(kernel="rbf") as gp:
        gp.upload_batch(X, y, None, group=G)
        calls = {"loo_batch": lambda: gp.loo_batch(ells, sns, group=G, predictions=False),
                 "hindcast_batch_lead1": lambda: gp.hindcast_batch(ells, sns, lead=1, group=G, predictions=False),
                 "hindcast_batch_lead5": lambda: gp.hindcast_batch(ells, sns, lead=5, group=G, predictions=False)}
        out = run_calls(gp, calls, reps)
    out["ratio_hindcast_batch_over_loo_batch"] = out["hindcast_batch_lead1"]["median_ms"] / out["loo_batch"]["median_ms"]
    return out


def golden_grid(reps):
    import seaiceextentforecasting_amd as S
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_golden
    script = "north_September"
    g = load_golden(script + "_retro")
    fmin, fmax = g["args"]
    ells, sns = np.logspace(-3, 0, 4), np.logspace(-2, 4, 4)
    with S.GPR(kernel="netdiffusion") as gp:
        call = lambda c: S.retro_grid_search(script, g["SIC"], g["SIEs_dt"], fmin, fmax, SST=g["SST"], ells=ells, sns=sns, gp=gp, criterion=c)
        out = run_calls(gp, {"retro_grid_loo_nlpd": lambda: call("loo_nlpd"), "retro_grid_hindcast_nlpd": lambda: call("hindcast_nlpd")}, reps)
        kern = {}
        for c in ("loo_nlpd", "hindcast_nlpd"):
            gp.profile_reset(); gp.profile(True, ["small"])
            call(c)
            p = gp.profile_get()["small"]
            gp.profile(False)
            kern[c] = {"ms": p["ms"], "launches": p["launches"]}
    out["small_class"] = kern
    out["fits"] = int(3 * (fmax - fmin + 1) * 16)
    out["note"] = "the host clock includes the feature selection and eigendecompositions of retro_grid_search; small_class is the one launch (HIP events)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "hindcast_bench", "kernel": "rbf", "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["single"] = {"n=%d d=%d" % (n, a.d): single(n, a.d, a.reps) for n in a.n}
    rec["group_of_8_n=2048"] = group(2048, a.d, 8, a.reps)
    rec["golden_retro_grid"] = golden_grid(a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
