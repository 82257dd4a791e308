"""What the score gradients of the one-workgroup kernel cost (csrc/smallgp.hpp: LooGrad, HindcastGrad) beside the launches they combine.

The reference-size grid: the 63 golden records x the 20 x 20 (l, sn~) grid = 25 200 fits in ONE launch per flavour.  Timed: the launch
alone, by HIP events around it (sigp_profile, class SIGP_KC_SMALL), for `HindcastGrad`, `LooGrad`, `Grad`, `Loo` and `Hindcast` ALTERNATING
inside each repeat (clock drift favours none); medians of `--reps` (9) repeats, best and worst beside them, after two warm-up launches each.
Reported: each new flavour beside `Grad + its score flavour` of the same run (both new flavours contain ONE inverse, as `Grad` does; the
sum contains two for leave-one-out), and the whole call (host packing, launch, copies back) for the same five.

    python tools/small_score_grad_bench.py --out profiles/r19_small_score_grad_bench.json
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lead", type=int, default=1)
    ap.add_argument("--min-train", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from conftest import GOLDEN_NAMES, load_golden
    from seaiceextentforecasting_amd import GPR, SmallBatch
    from seaiceextentforecasting_amd import _lib as L
    from seaiceextentforecasting_amd.features import LGRID, SGRID
    recs = [r for name in GOLDEN_NAMES for r in load_golden(name)["records"]]
    hc = dict(lead=a.lead, min_train=a.min_train, sigma_f="refit")
    modes = {"hindcast_grad": dict(hindcast=hc, score_grad="nlpd"), "loo_grad": dict(loo="refit", score_grad="nlpd"), "grad": dict(grad=True),
             "loo": dict(loo="refit"), "hindcast": dict(hindcast=hc)}
    kern, call = {k: [] for k in modes}, {k: [] for k in modes}
    with GPR(kernel="netdiffusion") as gp:
        sb = SmallBatch(gp)
        for r in recs:
            ds = sb.add_dataset(r["X"], r["y"], None, r["M"])
            for e in LGRID:
                for s_ in SGRID:
                    sb.add_fit(ds, e, s_, expm="eigh")
        F = len(recs) * len(LGRID) * len(SGRID)
        nmax = max(r["X"].shape[0] for r in recs)
        for kw in modes.values():
            sb.run(**kw); sb.run(**kw)
        for _ in range(a.reps):
            for k, kw in modes.items():
                gp.profile_reset(); gp.profile(True, ["small"])
                sb.run(**kw)
                kern[k].append(gp.profile_get()["small"]["ms"])
                gp.profile(False)
        for _ in range(a.reps):
            for k, kw in modes.items():
                gp.synchronize()
                t0 = time.perf_counter()
                sb.run(**kw)
                gp.synchronize()
                call[k].append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "small_score_grad_bench", "sigp_version": L.load().sigp_version(), "fits": F, "records": len(recs), "largest_n": int(nmax), "lead": a.lead,
           "min_train": a.min_train, "criterion": "nlpd", "sigma_f": "refit", "timing": "HIP events around the launch (SIGP_KC_SMALL), alternating, median of reps",
           "kernel": {k: stats(v) for k, v in kern.items()}, "call": {k: stats(v) for k, v in call.items()}}
    med = lambda k: out["kernel"][k]["median_ms"]
    out["hindcast_grad_over_grad_plus_hindcast"] = med("hindcast_grad") / (med("grad") + med("hindcast"))
    out["loo_grad_over_grad_plus_loo"] = med("loo_grad") / (med("grad") + med("loo"))
    out["evals_per_s_kernel"] = {k: F / (med(k) * 1e-3) for k in modes}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
