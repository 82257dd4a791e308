"""Per-feature (ARD) gradients of the hindcast density in lockstep groups beside the calls they compete with, on one GPU through the product
library (no torch), modelled on tools/cv_ard_batch_bench.py:

  one lockstep group of 8 fits (RBF, fp64; default n = 2048 4096, d = 8 64; 8 data sets, equal length scales so that every call factors the
  same matrices) and, for every lead of --leads (default 1 5): `hindcast_ard_batch` with its gradient (d + 1 hyper-parameters per fit),
  8 sequential single-fit `hindcast_ard` calls (what a user had to run before; the data of one fit stay staged on the handle, so no upload
  is timed), `hindcast_batch` on the same data (scores at one common scale), `hindcast_ard_batch(grad=None)` (scores only) and, once per
  shape, `loo_ard_batch` (the leave-one-out sibling) -- host clock around calls that are synchronous on return, bracketed by
  sigp_synchronize; every shape warmed up, then `--reps` repeats with the calls ALTERNATING inside each repeat; median, best and worst
  reported and the ratios.  Expectation 1: the lockstep call beats 8 sequential `hindcast_ard` calls (ratio below 1;
  `lockstep_beats_8_sequential_beyond_spread`: its slowest repeat against the fastest repeat of the 8 calls).
  Where the time goes: the SIGP_KC_MLII entries of one `hindcast_ard_batch` call step by step (one HIP-event bracket per step; the
  library prints them with host_timing = 2), `--reps` times ALTERNATING between the two kernels that can form W = U C: the group's
  `hindcast_w_lds_kernel` (what the driver takes by n_pad) and the single fit's `hindcast_w_kernel` on the same operands (the measurement
  switch hindcast_w_lds = 0 of the debug library, on a third handle that loads it; the timed calls above run on the product library).
  Expectation 2: the LDS kernel is not slower (`w_lds_over_w_strided`, medians; best and worst of each beside it).

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r18_hindcast_batch_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from cv_ard_bench import mlii_entries
from hindcast_bench import STEPS
from loo_ard_batch_bench import classes, summary, timed

GROUP = 8


def steps_of(gp, fn, w_lds):
    """the SIGP_KC_MLII entries (ms) of one hindcast_ard_batch call by name, W = U C on the kernel ``w_lds`` selects"""
    gp.set_option("hindcast_w_lds", w_lds)
    try:
        ent, total = mlii_entries(gp, fn)
    finally:
        gp.set_option("hindcast_w_lds", -1)
    if len(ent) != len(STEPS):
        return {"error": "expected %d entries, got %d" % (len(STEPS), len(ent))}
    out = {nm + "_ms": ms for nm, (_, ms) in zip(STEPS, ent)}
    out["mlii_ms"] = total["ms"]
    return out


def group(n, d, reps, leads):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    Xb, yb = np.zeros((GROUP, n, d)), np.zeros((GROUP, n))
    for b in range(GROUP):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240000 + b)
    ell, sn = np.sqrt(d), 1e-2
    ells, sns = np.full(GROUP, ell), np.full(GROUP, sn)
    th_ard = np.tile(np.log([ell] * d + [sn]), (GROUP, 1))
    os.environ["SIGP_USE_DEBUG_LIB"] = "1"         # the handle of the per-step brackets: the debug library has the W kernels' A/B switch
    gd = GPR(kernel="rbf")
    del os.environ["SIGP_USE_DEBUG_LIB"]
    with GPR(kernel="rbf") as gb, GPR(kernel="rbf") as gs, gd:
        gb.upload_batch(Xb, yb, None, group=GROUP)
        gd.upload_batch(Xb, yb, None, group=GROUP)
        gs.set_data(Xb[0], yb[0])
        calls = {"loo_ard_batch": (gb, lambda: gb.loo_ard_batch(th_ard, group=GROUP))}
        for lead in leads:
            tag = " lead=%d" % lead
            calls["hindcast_ard_batch" + tag] = (gb, lambda lead=lead: gb.hindcast_ard_batch(th_ard, lead=lead, group=GROUP))
            calls["hindcast_ard_x8" + tag] = (gs, lambda lead=lead: [gs.hindcast_ard(th_ard[0], lead=lead) for _ in range(GROUP)])
            calls["hindcast_batch" + tag] = (gb, lambda lead=lead: gb.hindcast_batch(ells, sns, lead=lead, group=GROUP, predictions=False))
            calls["hindcast_ard_batch_value" + tag] = (gb, lambda lead=lead: gb.hindcast_ard_batch(th_ard, lead=lead, grad=None, group=GROUP))
        ms = {k: [] for k in calls}
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, (gp, fn) in calls.items():
                t = timed(gp, fn)
                if r >= 2:
                    ms[k].append(t)
        out = summary(ms)
        out["leads"] = {}
        for lead in leads:
            tag = "lead=%d" % lead
            lock, seq = out["hindcast_ard_batch " + tag], out["hindcast_ard_x8 " + tag]
            fn = calls["hindcast_ard_batch " + tag][1]
            v_ard, g_ard = fn()
            v_one, g_one = gs.hindcast_ard(th_ard[0], lead=lead)
            per = {"lds": [], "strided": []}
            fd = lambda lead=lead: gd.hindcast_ard_batch(th_ard, lead=lead, group=GROUP)
            fd()                                   # (allocations out of the way)
            for _ in range(reps):                  # the two W kernels alternating, every other step beside them
                per["lds"].append(steps_of(gd, fd, -1))
                per["strided"].append(steps_of(gd, fd, 0))
            rec = {"ratio_hindcast_ard_batch_over_8_hindcast_ard": lock["median_ms"] / seq["median_ms"],
                   "ratio_hindcast_ard_batch_over_loo_ard_batch": lock["median_ms"] / out["loo_ard_batch"]["median_ms"],
                   "ratio_hindcast_ard_batch_over_hindcast_batch": lock["median_ms"] / out["hindcast_batch " + tag]["median_ms"],
                   "ratio_hindcast_ard_batch_over_its_values": lock["median_ms"] / out["hindcast_ard_batch_value " + tag]["median_ms"],
                   "lockstep_beats_8_sequential_beyond_spread": bool(lock["worst_ms"] < seq["best_ms"]),
                   "classes_of_one_hindcast_ard_batch": classes(gb, fn),
                   "classes_of_8_hindcast_ard": classes(gs, calls["hindcast_ard_x8 " + tag][1]),
                   # the same matrices either way (a check of the run, not a tolerance): member 0 against its single fit
                   "check": {"hindcast_ard_batch_0": float(v_ard[0]), "hindcast_ard_0": float(v_one),
                             "member_0_has_the_bits_of_the_single_fit": bool(v_ard[0] == v_one and np.array_equal(g_ard[0], g_one))}}
            bad = [s["error"] for k in per for s in per[k] if "error" in s]
            if bad:
                rec["steps"] = {"error": bad[0]}
            else:
                med = lambda k, nm: float(np.median([s[nm] for s in per[k]]))
                rec["steps"] = {nm + "_ms": med("lds", nm + "_ms") for nm in STEPS}
                w = {k: [s["w_scans_and_band_product_ms"] for s in per[k]] for k in per}
                rec["w_step"] = {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "worst_ms": float(np.max(v)), "reps": len(v)} for k, v in w.items()}
                rec["w_lds_over_w_strided"] = rec["w_step"]["lds"]["median_ms"] / rec["w_step"]["strided"]["median_ms"]
                rec["w_lds_not_slower_beyond_spread"] = bool(rec["w_step"]["lds"]["worst_ms"] <= rec["w_step"]["strided"]["best_ms"])
                rec["w_step_over_product_g"] = {k: rec["w_step"][k]["median_ms"] / med(k, "product_g_ms") for k in per}
                rec["mlii_ms"] = {k: med(k, "mlii_ms") for k in per}
            out["leads"][tag] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--leads", type=int, nargs="*", default=[1, 5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "hindcast_batch_bench", "kernel": "rbf", "dtype": "f64", "group": GROUP, "criterion": "hindcast_nlpd", "sigma_f": "refit",
           "sigp_version": L.load().sigp_version()}
    rec["group_of_8"] = {"n=%d d=%d" % (n, d): group(n, d, a.reps, a.leads) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
