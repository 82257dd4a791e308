"""Leave-one-out cross-validation beside the calls it competes with, on one GPU through the product library (no torch):

  large fits (RBF, d = 8, fp64; default n = 4096 8192): `refit`, `refit + loo`, `nlml(grad="exact")` -- host clock around calls that
      are synchronous on return, bracketed by sigp_synchronize; every shape warmed up, then `--reps` repeats with the three calls
      ALTERNATING inside each repeat (clock drift favours none); median and best reported;
  the reference-size grid: the 63 golden records x the 20 x 20 (l, sn~) grid in one launch: `run()`, `run(grad=True)`, `run(loo="refit")`
      as evaluations / s.

The kernels alone come from a rocprofv3 pass of this same script (`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o loo
-- python tools/loo_bench.py --n 8192 --reps 3 --no-small`, ONE size so that a kernel's average is that size's): give its
`*_kernel_stats.csv` as `--kernel-stats` to a later run (or to `--stats-only --n 8192`) and the record gains `loo_rows_kernel` and
`rowdot_kernel` (launched by nlml(grad="exact") on the same U and by nothing else here): average time, bytes / s over the 4 n^2 bytes of U's upper
triangle both read, and their ratio.  `--skip-loo` times only what an older library has (the parent's numbers on the same box).
Prints one JSON line; `--out FILE` also writes it."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def large(n, reps, skip_loo):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th = np.log([ell, sn])
    calls = {"fit": lambda gp: gp.refit(ell, sn), "nlml_exact": lambda gp: gp.nlml(th, grad="exact")}
    if not skip_loo:
        calls["fit_loo"] = lambda gp: (gp.refit(ell, sn), gp.loo())
        calls["loo_after_fit"] = lambda gp: gp.loo()
    ms = {k: [] for k in calls}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        for _ in range(2):                       # warm-up: every shape, every workspace allocated
            for k, fn in calls.items():
                if k == "loo_after_fit":
                    gp.refit(ell, sn)
                fn(gp)
        for _ in range(reps):
            for k, fn in calls.items():
                if k == "loo_after_fit":
                    gp.refit(ell, sn)
                ms[k].append(timed(gp, lambda: fn(gp)))
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "reps": len(v)} for k, v in ms.items()}


def small(reps, skip_loo):
    from conftest import GOLDEN_NAMES, load_golden
    from seaiceextentforecasting_amd import GPR, SmallBatch
    from seaiceextentforecasting_amd.features import LGRID, SGRID
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    modes = {"plain": dict(), "grad": dict(grad=True)}
    if not skip_loo:
        modes["loo"] = dict(loo="refit")
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
        for _ in range(reps):                    # the calls as a user makes them (host packing, launch, copies back), no brackets
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
        call, kms = float(np.median(ms[k])), float(np.median(kern[k]))
        out[k] = {"call_ms": call, "call_ms_all": [round(v, 3) for v in ms[k]], "kernel_ms": kms, "evals_per_s_call": F / (call * 1e-3), "evals_per_s_kernel": F / (kms * 1e-3)}
    return out


def kernel_stats(path, n):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key in ("loo_rows_kernel", "rowdot_kernel<double>"):
                if key in r["Name"]:
                    rows[key.split("<")[0]] = r
    out = {"n": n, "bytes": 4.0 * n * n, "source": "rocprofv3 --kernel-trace --stats, AverageNs"}
    for k, r in rows.items():
        t = float(r["AverageNs"]) * 1e-9
        out[k] = {"calls": int(r["Calls"]), "average_ms": t * 1e3, "min_ms": float(r["MinNs"]) * 1e-6, "bytes_per_s": out["bytes"] / t}
    if len(rows) == 2:
        out["loo_rows_over_rowdot_rate"] = out["loo_rows_kernel"]["bytes_per_s"] / out["rowdot_kernel"]["bytes_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--skip-loo", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--stats-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"tool": "loo_bench", "kernel": "rbf", "d": 8, "dtype": "f64"}
    if not a.stats_only:
        from seaiceextentforecasting_amd import _lib as L
        rec["sigp_version"] = L.load().sigp_version()
        rec["large"] = {str(n): large(n, a.reps, a.skip_loo) for n in a.n}
        if not a.no_small:
            rec["small_grid"] = small(a.reps, a.skip_loo)
    if a.kernel_stats:
        rec["kernels_alone"] = kernel_stats(a.kernel_stats, max(a.n))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
