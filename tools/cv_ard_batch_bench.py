"""Per-feature (ARD) gradients of the leave-block-out density in lockstep groups beside the calls they compete with, on one GPU through the
product library (no torch), modelled on tools/loo_ard_batch_bench.py:

  one lockstep group of 8 fits (RBF, fp64; default n = 2048 4096, d = 8 64; 8 data sets, equal length scales so that every call factors the
  same matrices) and, for every (block, gap) of --folds (default 5,0 16,8): `cv_ard_batch` with its gradient (d + 1 hyper-parameters per
  fit), 8 sequential single-fit `cv_ard` calls (what a user had to run before; the data of one fit stay staged on the handle, so no upload
  is timed), `cv_batch` on the same data (scores at one common scale), `cv_ard_batch(grad=None)` (scores only) and, once per shape,
  `loo_ard_batch` (the leave-one-out sibling) -- host clock around calls that are synchronous on return, bracketed by sigp_synchronize;
  every shape warmed up, then `--reps` repeats with the calls ALTERNATING inside each repeat; median, best and worst reported and the ratios.
  The criterion: the lockstep call beats 8 sequential `cv_ard` calls by more than the run-to-run spread -- the slowest repeat of
  `cv_ard_batch` against the fastest repeat of the 8 calls (`lockstep_beats_8_sequential_beyond_spread`).
  Where the time goes: the SIGP_KC_* classes (HIP events through sigp_profile, a pass of its own) of one `cv_ard_batch` call and of 8
  `cv_ard` calls, and the SIGP_KC_MLII entries of one `cv_ard_batch` call step by step (tools/cv_ard_bench.py reads them back): the fold
  adjoints, their assembly and the banded product -- the steps that are new with a member axis -- against the product M.

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r15_cv_ard_batch_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from cv_ard_bench import mlii_entries, steps_of
from loo_ard_batch_bench import classes, summary, timed

GROUP = 8
PASS_PAIRS = 1024          # (member, fold) pairs of one pass of cv_launch


def group(n, d, reps, folds):
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
        calls = {"loo_ard_batch": (gb, lambda: gb.loo_ard_batch(th_ard, group=GROUP))}
        for b, g in folds:
            tag = " block=%d gap=%d" % (b, g)
            calls["cv_ard_batch" + tag] = (gb, lambda b=b, g=g: gb.cv_ard_batch(th_ard, b, gap=g, group=GROUP))
            calls["cv_ard_x8" + tag] = (gs, lambda b=b, g=g: [gs.cv_ard(th_ard[0], b, gap=g) for _ in range(GROUP)])
            calls["cv_batch" + tag] = (gb, lambda b=b, g=g: gb.cv_batch(ells, sns, b, gap=g, group=GROUP, predictions=False))
            calls["cv_ard_batch_value" + tag] = (gb, lambda b=b, g=g: gb.cv_ard_batch(th_ard, b, gap=g, grad=None, group=GROUP))
        ms = {k: [] for k in calls}
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, (gp, fn) in calls.items():
                t = timed(gp, fn)
                if r >= 2:
                    ms[k].append(t)
        out = summary(ms)
        out["folds"] = {}
        for b, g in folds:
            tag = "block=%d gap=%d" % (b, g)
            F = -(-n // b)
            fp = max(1, min(F, PASS_PAIRS // GROUP))
            passes = -(-F // fp)
            lock, seq = out["cv_ard_batch " + tag], out["cv_ard_x8 " + tag]
            v_ard, g_ard = gb.cv_ard_batch(th_ard, b, gap=g, group=GROUP)
            v_one, g_one = gs.cv_ard(th_ard[0], b, gap=g)
            ent, total = mlii_entries(gb, calls["cv_ard_batch " + tag][1])
            steps = steps_of(ent, passes)
            rec = {"passes": passes,
                   "ratio_cv_ard_batch_over_8_cv_ard": lock["median_ms"] / seq["median_ms"],
                   "ratio_cv_ard_batch_over_loo_ard_batch": lock["median_ms"] / out["loo_ard_batch"]["median_ms"],
                   "ratio_cv_ard_batch_over_cv_batch": lock["median_ms"] / out["cv_batch " + tag]["median_ms"],
                   "ratio_cv_ard_batch_over_its_values": lock["median_ms"] / out["cv_ard_batch_value " + tag]["median_ms"],
                   "lockstep_beats_8_sequential_beyond_spread": bool(lock["worst_ms"] < seq["best_ms"]),
                   "classes_of_one_cv_ard_batch": classes(gb, calls["cv_ard_batch " + tag][1]),
                   "classes_of_8_cv_ard": classes(gs, calls["cv_ard_x8 " + tag][1]),
                   "mlii_class": {"ms": total["ms"], "launches": total["launches"], "flops": total["flops"]},
                   "steps": steps,
                   # the same matrices either way (a check of the run, not a tolerance): member 0 against its single fit
                   "check": {"cv_ard_batch_0": float(v_ard[0]), "cv_ard_0": float(v_one),
                             "member_0_has_the_bits_of_the_single_fit": bool(v_ard[0] == v_one and np.array_equal(g_ard[0], g_one))}}
            if "error" not in steps:
                new = steps["fold_adjoints_ms"] + steps["assembly_ms"] + steps["band_product_ms"]
                rec["new_steps_ms"] = new
                rec["new_steps_over_product_m"] = new / steps["product_m_ms"]
                rec["new_steps_share_of_mlii"] = new / total["ms"]
            out["folds"][tag] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--folds", nargs="*", default=["5,0", "16,8"], help="block,gap pairs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    folds = [tuple(int(v) for v in f.split(",")) for f in a.folds]
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "cv_ard_batch_bench", "kernel": "rbf", "dtype": "f64", "group": GROUP, "criterion": "cv_nlpd", "sigma_f": "refit",
           "sigp_version": L.load().sigp_version()}
    rec["group_of_8"] = {"n=%d d=%d" % (n, d): group(n, d, a.reps, folds) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
