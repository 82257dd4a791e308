"""What option ``accurate_solve`` costs, on one GPU through the product library (no torch).

Per shape -- a single fit at n = 4096 and 8192 (RBF, d = 8, fp64): ``refit``, ``predict`` at m = 1024 new points, ``alpha_``; a lockstep
group of 8 at n = 2048: ``fit_batch`` -- the option ALTERNATES between 0 and 1 inside every repeat on ONE handle (clock drift favours
neither), host clock around calls that are synchronous on return, bracketed by sigp_synchronize; every call is warmed up in both settings
first.  Reported per call: the median of ``--reps`` (5) repeats with the spread (min, max) for either setting, and the ratio of the medians
option 1 / option 0.

The column solves alone come from a second pass with the SIGP_KC_TRSM class bracketed by events (sigp_profile): per setting the class's
time, launches and flop count over one ``refit`` -- option 1: every launch is refined_solve_kernel, counted at 3 x 2 r 128^2 flops per row
tile of r rows; option 0: the plain column solves and the fused-link / strip forms, each at its own count -- and the rates they give.
Prints one JSON line; ``--out FILE`` also writes it."""
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


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "reps": len(v)}


def alternate(gp, calls, reps, before=None):
    """{call: {"0": stats, "1": stats, "ratio": median 1 / median 0}}"""
    ms = {k: {0: [], 1: []} for k in calls}
    for rep in range(-2, reps):                  # two warm-up rounds: every workspace of either setting allocated
        for opt in (0, 1):
            gp.set_option("accurate_solve", opt)
            if before:
                before(gp)
            for k, fn in calls.items():
                t = timed(gp, lambda: fn(gp))
                if rep >= 0:
                    ms[k][opt].append(t)
    gp.set_option("accurate_solve", 0)
    return {k: {"0": stats(v[0]), "1": stats(v[1]), "ratio": float(np.median(v[1]) / np.median(v[0]))} for k, v in ms.items()}


def trsm_class(gp, fit):
    out = {}
    for opt in (0, 1):
        gp.set_option("accurate_solve", opt)
        fit(gp)
        gp.profile(True, classes=["trsm"])
        gp.profile_reset()
        fit(gp)
        gp.synchronize()
        p = gp.profile_get()["trsm"]
        gp.profile(False)
        out[str(opt)] = {"ms": p["ms"], "launches": int(p["launches"]), "gflop": p["flops"] * 1e-9,
                         "tflops": p["flops"] / (p["ms"] * 1e-3) * 1e-12 if p["ms"] > 0 else None}
    gp.set_option("accurate_solve", 0)
    return out


def single(n, m, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, Xs = O.synthetic_problem(n, d, 20240000, m=m)
    ell, sn = np.sqrt(d), 1e-2
    calls = {"refit": lambda gp: gp.refit(ell, sn), "predict_m%d" % m: lambda gp: gp.predict(Xs), "alpha_": lambda gp: gp.alpha_}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        rec = alternate(gp, calls, reps)
        rec["trsm_class_of_one_refit"] = trsm_class(gp, lambda g: g.refit(ell, sn))
    return rec


def group(n, members, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, Xs = O.synthetic_problem(n, d, 20240001, m=2)
    ell = np.full(members, np.sqrt(d))
    sn = np.logspace(-2, -1, members)
    with GPR(kernel="rbf") as gp:
        fit = lambda g: g.fit_batch(X, y, Xs, ell, sn, concurrency=1, group=members)
        rec = alternate(gp, {"fit_batch": fit}, reps)
        rec["trsm_class_of_one_fit_batch"] = trsm_class(gp, fit)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--group-n", type=int, default=2048)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rec = {"tool": "accurate_bench", "reps": a.reps, "single": {str(n): single(n, a.m, a.reps) for n in a.n},
           "group": {"n": a.group_n, "members": a.members, **group(a.group_n, a.members, a.reps)}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
