"""Per-feature (ARD) gradients of the leave-one-out density in lockstep groups beside the calls they compete with, on one GPU through the
product library (no torch), modelled on tools/ard_batch_bench.py:

  one lockstep group of 8 fits (RBF, fp64; default n = 2048 4096, d = 8 64; 8 data sets, equal length scales so that every call factors the
  same matrices): `loo_ard_batch` with its gradient (d + 1 hyper-parameters per fit), 8 sequential single-fit `loo_ard` calls (what a user
  had to run before; the data of one fit stay staged on the handle, so no upload is timed), `loo_batch(grad=True)` on the same data (two
  hyper-parameters per fit), `nlml_ard_batch` (the marginal-likelihood sibling) and `loo_ard_batch(grad=None)` (scores only) -- host clock
  around calls that are synchronous on return, bracketed by sigp_synchronize; every shape warmed up, then `--reps` repeats with the calls
  ALTERNATING inside each repeat; median, best and worst reported and the ratios.
  The criterion: the lockstep call beats 8 sequential `loo_ard` calls by more than the run-to-run spread -- the slowest repeat of
  `loo_ard_batch` against the fastest repeat of the 8 calls (`lockstep_beats_8_sequential_beyond_spread`).
  Where the time goes: the SIGP_KC_* classes (HIP events through sigp_profile, a pass of its own) of one `loo_ard_batch` call and of 8
  `loo_ard` calls.

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r14_loo_ard_batch_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

GROUP = 8


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "worst_ms": float(np.max(v)), "reps": len(v)} for k, v in ms.items()}


def classes(gp, fn):
    """ms and entries of every kernel class that one run of fn books"""
    gp.profile_reset(); gp.profile(True)
    fn()
    p = gp.profile_get()
    gp.profile(False)
    return {k: {"ms": v["ms"], "launches": v["launches"]} for k, v in p.items() if v["launches"]}


def group(n, d, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    Xb, yb = np.zeros((GROUP, n, d)), np.zeros((GROUP, n))
    for b in range(GROUP):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240000 + b)
    ell, sn = np.sqrt(d), 1e-2
    ells, sns = np.full(GROUP, ell), np.full(GROUP, sn)
    th_ard = np.tile(np.log([ell] * d + [sn]), (GROUP, 1))
    with GPR(kernel="rbf") as gb, GPR(kernel="rbf") as gs:
        gb.upload_batch(Xb, yb, None, group=GROUP)
        gs.set_data(Xb[0], yb[0])
        calls = {"loo_ard_batch": (gb, lambda: gb.loo_ard_batch(th_ard, group=GROUP)),
                 "loo_ard_x8": (gs, lambda: [gs.loo_ard(th_ard[0]) for _ in range(GROUP)]),
                 "loo_batch_grad": (gb, lambda: gb.loo_batch(ells, sns, group=GROUP, predictions=False, grad=True)),
                 "nlml_ard_batch": (gb, lambda: gb.nlml_ard_batch(th_ard, group=GROUP)),
                 "loo_ard_batch_value": (gb, lambda: gb.loo_ard_batch(th_ard, grad=None, group=GROUP))}
        ms = {k: [] for k in calls}
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, (gp, fn) in calls.items():
                t = timed(gp, fn)
                if r >= 2:
                    ms[k].append(t)
        v_ard, g_ard = gb.loo_ard_batch(th_ard, group=GROUP)
        iso = gb.loo_batch(ells, sns, group=GROUP, predictions=False, grad=True)
        v_one, g_one = gs.loo_ard(th_ard[0])
        cl_batch = classes(gb, calls["loo_ard_batch"][1])
        cl_x8 = classes(gs, calls["loo_ard_x8"][1])
    out = summary(ms)
    out["ratio_loo_ard_batch_over_8_loo_ard"] = out["loo_ard_batch"]["median_ms"] / out["loo_ard_x8"]["median_ms"]
    out["ratio_loo_ard_batch_over_loo_batch_grad"] = out["loo_ard_batch"]["median_ms"] / out["loo_batch_grad"]["median_ms"]
    out["ratio_loo_ard_batch_over_nlml_ard_batch"] = out["loo_ard_batch"]["median_ms"] / out["nlml_ard_batch"]["median_ms"]
    out["lockstep_beats_8_sequential_beyond_spread"] = bool(out["loo_ard_batch"]["worst_ms"] < out["loo_ard_x8"]["best_ms"])
    out["classes_of_one_loo_ard_batch"], out["classes_of_8_loo_ard"] = cl_batch, cl_x8
    # the same matrices either way (a check of the run, not a tolerance): member 0 against its single fit and the isotropic batch
    out["check"] = {"loo_ard_batch_0": float(v_ard[0]), "loo_ard_0": float(v_one), "loo_batch_0": float(iso["nlpd"][0]),
                    "member_0_has_the_bits_of_the_single_fit": bool(v_ard[0] == v_one and np.array_equal(g_ard[0], g_one)),
                    "sum_dlogl_loo_ard_batch_0": float(np.sum(g_ard[0, :d])), "dlogl_loo_batch_0": float(iso["nlpd_grad"][0, 0]),
                    "dlogsn_loo_ard_batch_0": float(g_ard[0, d]), "dlogsn_loo_batch_0": float(iso["nlpd_grad"][0, 1])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "loo_ard_batch_bench", "kernel": "rbf", "dtype": "f64", "group": GROUP, "criterion": "loo_nlpd", "sigma_f": "refit",
           "sigp_version": L.load().sigp_version()}
    rec["group_of_8"] = {"n=%d d=%d" % (n, d): group(n, d, a.reps) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
