"""What the stationary flavours of the one-workgroup kernel cost (csrc/smallgp.hpp: SmallCov::Stationary) beside the factored flavours on
the same data sets, and one gradient round of per-feature fits beside the lockstep route that existed before them.

1. The reference-size grid: the shapes of the 63 golden retro records x a 20 x 20 grid = 25 200 fits in ONE launch per flavour.  The
   factored flavours run the records as the retro loop does ((l, sn~) = LGRID x SGRID); the stationary flavours run the records' raw rows
   with the RBF kernel, one common scale from d0 logspace(-0.5, 1, 20) (d0 = the record's root-mean-square distance) x SGRID.  Timed: the
   launch alone, by HIP events around it (sigp_profile, class SIGP_KC_SMALL), the five stationary and the five factored flavours ALTERNATING
   inside each repeat; medians of `--reps` (5) repeats, best and worst beside them, after two warm-up launches each.
2. One round of an MLII optimisation over per-feature scales: F = 63 S fits (S = `--starts` starts per data set) through
   ``SmallStationaryBatch.run(grad=True)`` -- one launch -- beside ``GPR.nlml_ard_batch`` on the same F fits, the lockstep groups of the
   blocked engine.  That engine takes data sets of one shape, so for this part every record is cut to the last 23 rows and the first 8
   features (the smallest n and N among the records).  Timed: the whole call, host to host (there is no single launch to time in the
   lockstep route), alternating, `--reps` repeats after two warm-up calls each.  Reported: both medians, the slowest repeat of the
   single launch beside the fastest repeat of the lockstep call, and their ratio.

    python tools/small_stationary_bench.py --out profiles/r21_small_stationary_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stats(v):
    return {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "worst_ms": float(np.max(v)), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--starts", type=int, default=8)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from conftest import GOLDEN_NAMES, load_golden
    from seaiceextentforecasting_amd import GPR, SmallBatch, SmallStationaryBatch
    from seaiceextentforecasting_amd import _lib as L
    from seaiceextentforecasting_amd.features import LGRID, SGRID
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    hc = dict(lead=1, min_train=2, sigma_f="refit")
    cv = dict(block=5, gap=1, sigma_f="refit")
    modes = {"plain": dict(), "grad": dict(grad=True), "loo": dict(loo="refit"), "cv": dict(cv=cv), "hindcast": dict(hindcast=hc)}
    kern = {(kind, k): [] for kind in ("stationary", "factored") for k in modes}
    with GPR(kernel="netdiffusion") as gf, GPR(kernel="rbf") as gs:
        sf, ss = SmallBatch(gf), SmallStationaryBatch(gs)
        for r in recs:
            X = np.asarray(r["X"], dtype=np.float64)
            ds = sf.add_dataset(X, r["y"], None, r["M"])
            dk = ss.add_dataset(X, r["y"])
            d0 = float(np.sqrt(np.mean(np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2))))
            for e, ek in zip(LGRID, d0 * np.logspace(-0.5, 1.0, len(LGRID))):
                for s_ in SGRID:
                    sf.add_fit(ds, e, s_, expm="eigh")
                    ss.add_fit(dk, float(ek), s_)
        F = len(recs) * len(LGRID) * len(SGRID)
        runs = {"stationary": (gs, ss), "factored": (gf, sf)}
        for gp, sb in runs.values():
            for kw in modes.values():
                sb.run(**kw); sb.run(**kw)
        for _ in range(a.reps):
            for k, kw in modes.items():
                for kind, (gp, sb) in runs.items():
                    gp.profile_reset(); gp.profile(True, ["small"])
                    sb.run(**kw)
                    kern[(kind, k)].append(gp.profile_get()["small"]["ms"])
                    gp.profile(False)
    # ---- one gradient round of per-feature fits: one launch beside the lockstep groups ----
    n0, N0 = min(r["X"].shape[0] for r in recs), min(r["X"].shape[1] for r in recs)
    Xb = np.stack([np.asarray(r["X"], dtype=np.float64)[-n0:, :N0] for r in recs])
    yb = np.stack([np.asarray(r["y"], dtype=np.float64).reshape(-1)[-n0:] for r in recs])
    B = len(recs)
    rng = np.random.default_rng(21)
    theta = np.concatenate([np.log(np.sqrt(N0)) + rng.uniform(-0.5, 1.0, (a.starts * B, N0)), np.log(rng.uniform(0.05, 0.5, (a.starts * B, 1)))], axis=1)
    one, lock = [], []
    with GPR(kernel="rbf") as gp:
        gp.upload_small_ard(Xb, yb)
        gp.upload_batch(Xb, yb, None, group=a.group, concurrency=1)
        for _ in range(2):
            v1, g1 = gp.small_nlml_ard_batch(theta)
            v2, g2 = gp.nlml_ard_batch(theta, group=a.group)
        agree = float(max(np.max(np.abs(v1 - v2) / np.maximum(1, np.abs(v2))), np.max(np.abs(g1 - g2)) / np.max(np.abs(g2))))
        for _ in range(a.reps):
            for fn, acc in ((lambda: gp.small_nlml_ard_batch(theta), one), (lambda: gp.nlml_ard_batch(theta, group=a.group), lock)):
                gp.synchronize()
                t0 = time.perf_counter()
                fn()
                gp.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "small_stationary_bench", "sigp_version": L.load().sigp_version(), "fits": F, "records": len(recs),
           "largest_n": int(max(r["X"].shape[0] for r in recs)), "kernel_id": "rbf", "cv": cv, "hindcast": hc,
           "timing": "HIP events around the launch (SIGP_KC_SMALL), alternating, median of reps",
           "kernel": {kind: {k: stats(kern[(kind, k)]) for k in modes} for kind in ("stationary", "factored")},
           "gradient_round": {"fits": int(theta.shape[0]), "data_sets": B, "n": int(n0), "N": int(N0), "starts": a.starts, "group": a.group,
                              "timing": "whole call, host to host, alternating", "largest_difference": agree,
                              "one_launch": stats(one), "lockstep": stats(lock)}}
    out["stationary_over_factored"] = {k: out["kernel"]["stationary"][k]["median_ms"] / out["kernel"]["factored"][k]["median_ms"] for k in modes}
    gr = out["gradient_round"]
    gr["lockstep_best_over_one_launch_worst"] = gr["lockstep"]["best_ms"] / gr["one_launch"]["worst_ms"]
    gr["expectation_met"] = bool(gr["one_launch"]["worst_ms"] < gr["lockstep"]["best_ms"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
