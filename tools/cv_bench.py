"""Leave-block-out cross-validation beside the call it competes with, leave-one-out, IN THE SAME RUN, on one GPU through the product
library (no torch):

  large fits (RBF, d = 8, fp64; default n = 4096 8192): `fit`, `loo()`, `cv(block=128)`, `cv(block=16, gap=8)`, `cv(block=1)` after a fit -- host
      clock around calls that are synchronous on return, bracketed by sigp_synchronize; every shape warmed up, then `--reps` repeats with
      the calls ALTERNATING inside each repeat (clock drift favours none); min and median reported, and cv / loo from the medians;
      the device time of one call from sigp_profile (class mlii: the triangular inversion both share, then strip product / finish /
      fold Cholesky / closing solves per pass; cv - loo is what the fold steps cost beyond the row pass), in a pass of its own; `cv_slices` auto against 1 for every shape;
  lockstep: `cv_batch(block=16, gap=8)` against `loo_batch` for a group of 8 at n = 2048;
  the reference-size grid: the 63 golden records x the 20 x 20 (l, sn~) grid in one launch: `run(loo="refit")` against
      `run(cv=dict(block=5, gap=1))`, call and kernel (sigp_profile class small).

Prints one JSON line; `--out FILE` also writes it (profiles/r09_cv_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SHAPES = {"cv_b128": (128, 0), "cv_b16_g8": (16, 8), "cv_b1": (1, 0)}


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "reps": len(v)}


def large(n, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    calls = {"fit": lambda gp: gp.refit(ell, sn), "loo": lambda gp: gp.loo()}
    for k, (b, g) in SHAPES.items():
        calls[k] = lambda gp, b=b, g=g: gp.cv(b, g)
        calls[k + "_slices1"] = lambda gp, b=b, g=g: gp.cv(b, g)
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        gp.refit(ell, sn)
        for rep in range(2 + reps):              # two warm-up rounds (every shape, every workspace allocated), then the repeats
            for k, fn in calls.items():
                gp.set_option("cv_slices", 1 if k.endswith("_slices1") else 0)
                t = timed(gp, lambda: fn(gp))
                if rep >= 2:
                    ms[k].append(t)
        out = {k: stats(v) for k, v in ms.items()}
        for k in SHAPES:
            out[k]["over_loo"] = out[k]["median_ms"] / out["loo"]["median_ms"]
            gp.set_option("cv_slices", 0)
            calls[k](gp)
            out[k]["cv_slices_auto"] = int(gp._stat("cv_slices"))
        # device time of one call by class (HIP events around every launch group), in a pass of its own
        for k in ["loo"] + list(SHAPES):
            dev = []
            for _ in range(max(3, reps // 2)):
                gp.profile_reset(); gp.profile(True, ["mlii"])
                calls[k](gp)
                p = gp.profile_get()["mlii"]
                dev.append(p["ms"])
                gp.profile(False)
            out[k]["device_ms_mlii"] = float(np.median(dev))
            out[k]["entries_mlii"] = int(p["launches"])
        inv = out["loo"]["device_ms_mlii"]
        for k in SHAPES:
            out[k]["device_ms_over_loo_device"] = out[k]["device_ms_mlii"] / inv
    return out


def lockstep(n, group, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    Xb = np.zeros((group, n, d)); yb = np.zeros((group, n))
    for b in range(group):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240000 + b)
    ell, sn = np.full(group, np.sqrt(d)), np.full(group, 1e-2)
    calls = {"loo_batch": lambda gp: gp.loo_batch(ell, sn, group=group, predictions=False),
             "cv_batch_b16_g8": lambda gp: gp.cv_batch(ell, sn, 16, gap=8, group=group, predictions=False)}
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.upload_batch(Xb, yb, None, group=group)
        for _ in range(2):
            for fn in calls.values():
                fn(gp)
        for _ in range(reps):
            for k, fn in calls.items():
                ms[k].append(timed(gp, lambda: fn(gp)))
    out = {k: stats(v) for k, v in ms.items()}
    out["n"], out["group"] = n, group
    out["cv_over_loo"] = out["cv_batch_b16_g8"]["median_ms"] / out["loo_batch"]["median_ms"]
    return out


def small(reps):
    from conftest import GOLDEN_NAMES, load_golden
    from seaiceextentforecasting_amd import GPR, SmallBatch
    from seaiceextentforecasting_amd.features import LGRID, SGRID
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    modes = {"loo": dict(loo="refit"), "cv_b5_g1": dict(cv=dict(block=5, gap=1))}
    ms = {k: [] for k in modes}
    with GPR(kernel="netdiffusion") as gp:
        sb = SmallBatch(gp)
        for r in recs:
            ds = sb.add_dataset(r["X"], r["y"], None, r["M"])
            for e in LGRID:
                for s_ in SGRID:
                    sb.add_fit(ds, e, s_, expm="eigh")
        F = len(recs) * len(LGRID) * len(SGRID)
        for kw in modes.values():
            sb.run(**kw); sb.run(**kw)
        for _ in range(reps):
            for k, kw in modes.items():
                ms[k].append(timed(gp, lambda: sb.run(**kw)))
        kern = {k: [] for k in modes}
        for _ in range(reps):                    # the launch alone: HIP events around it (sigp_profile), in a pass of its own
            for k, kw in modes.items():
                gp.profile_reset(); gp.profile(True, ["small"])
                sb.run(**kw)
                kern[k].append(gp.profile_get()["small"]["ms"])
                gp.profile(False)
    out = {"fits": F, "records": len(recs)}
    for k in modes:
        out[k] = {"call": stats(ms[k]), "kernel": stats(kern[k]), "evals_per_s_kernel": F / (float(np.median(kern[k])) * 1e-3)}
    out["cv_over_loo_kernel"] = out["cv_b5_g1"]["kernel"]["median_ms"] / out["loo"]["kernel"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--no-lockstep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "cv_bench", "kernel": "rbf", "d": 8, "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["large"] = {str(n): large(n, a.reps) for n in a.n}
    if not a.no_lockstep:
        rec["lockstep"] = lockstep(2048, 8, a.reps)
    if not a.no_small:
        rec["small_grid"] = small(a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
