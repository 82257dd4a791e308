"""Per-feature (ARD) length scales in lockstep groups beside the calls they compete with, on one GPU through the product library (no torch),
modelled on tools/ard_bench.py:

  one lockstep group of 8 fits (RBF, fp64; default n = 2048 4096, d = 8 64; 8 data sets, equal length scales so that every call factors the
  same matrices): `nlml_ard_batch` (d + 1 hyper-parameters per fit), `nlml_batch(grad="exact")` on the same data (two hyper-parameters per
  fit: code this change does not touch) and 8 sequential single-fit `nlml_ard` calls (what a user had to run before; the data of one fit
  stay staged on the handle, so no upload is timed) -- host clock around calls that are synchronous on return, bracketed by
  sigp_synchronize; every shape warmed up, then `--reps` repeats with the calls ALTERNATING inside each repeat; median and best reported
  and the two ratios.  The staging launch on its own: the SIGP_KC_KBUILD class (HIP events through sigp_profile, a pass of its own) of one
  `nlml_ard_batch(grad=None)` call minus that of one `nlml_batch(grad=None)` call -- the two issue the same covariance builds, the staging
  launch is the difference.

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r13_ard_batch_bench.json)."""
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
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "reps": len(v)} for k, v in ms.items()}


def kclass(gp, name, fn):
    gp.profile_reset(); gp.profile(True, [name])
    fn()
    p = gp.profile_get()[name]
    gp.profile(False)
    return {"ms": p["ms"], "launches": p["launches"]}


def group(n, d, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    Xb, yb = np.zeros((GROUP, n, d)), np.zeros((GROUP, n))
    for b in range(GROUP):
        Xb[b], yb[b], _ = O.synthetic_problem(n, d, 20240000 + b)
    ell, sn = np.sqrt(d), 1e-2
    th = np.tile(np.log([ell, sn]), (GROUP, 1))
    th_ard = np.tile(np.log([ell] * d + [sn]), (GROUP, 1))
    ms = {"nlml_ard_batch": [], "nlml_batch_exact": [], "nlml_ard_x8": []}
    with GPR(kernel="rbf") as gb, GPR(kernel="rbf") as gs:
        gb.upload_batch(Xb, yb, None, group=GROUP)
        gs.set_data(Xb[0], yb[0])
        calls = {"nlml_ard_batch": (gb, lambda: gb.nlml_ard_batch(th_ard, group=GROUP)),
                 "nlml_batch_exact": (gb, lambda: gb.nlml_batch(th, grad="exact", group=GROUP)),
                 "nlml_ard_x8": (gs, lambda: [gs.nlml_ard(th_ard[0]) for _ in range(GROUP)])}
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            for k, (gp, fn) in calls.items():
                t = timed(gp, fn)
                if r >= 2:
                    ms[k].append(t)
        v_ard, g_ard = gb.nlml_ard_batch(th_ard, group=GROUP)
        v_iso, g_iso = gb.nlml_batch(th, grad="exact", group=GROUP)
        v_one, g_one = gs.nlml_ard(th_ard[0])
        kb_ard = kclass(gb, "kbuild", lambda: gb.nlml_ard_batch(th_ard, grad=None, group=GROUP))
        kb_iso = kclass(gb, "kbuild", lambda: gb.nlml_batch(th, grad=None, group=GROUP))
        ml_ard = kclass(gb, "mlii", lambda: gb.nlml_ard_batch(th_ard, group=GROUP))
        ml_iso = kclass(gb, "mlii", lambda: gb.nlml_batch(th, grad="exact", group=GROUP))
    out = summary(ms)
    out["ratio_nlml_ard_batch_over_8_nlml_ard"] = out["nlml_ard_batch"]["median_ms"] / out["nlml_ard_x8"]["median_ms"]
    out["ratio_nlml_ard_batch_over_nlml_batch_exact"] = out["nlml_ard_batch"]["median_ms"] / out["nlml_batch_exact"]["median_ms"]
    out["kbuild_class_of_one_nlml_ard_batch_value"], out["kbuild_class_of_one_nlml_batch_value"] = kb_ard, kb_iso
    out["staging_launch_ms"] = kb_ard["ms"] - kb_iso["ms"]
    out["mlii_class_of_one_nlml_ard_batch"], out["mlii_class_of_one_nlml_batch_exact"] = ml_ard, ml_iso
    # the same matrices either way (a check of the run, not a tolerance): member 0 against its single fit and the isotropic batch
    out["check"] = {"nlml_ard_batch_0": float(v_ard[0]), "nlml_ard_0": float(v_one), "nlml_batch_0": float(v_iso[0]),
                    "member_0_has_the_bits_of_the_single_fit": bool(v_ard[0] == v_one and np.array_equal(g_ard[0], g_one)),
                    "sum_dlogl_ard_batch_0": float(np.sum(g_ard[0, :d])), "dlogl_batch_0": float(g_iso[0, 0]),
                    "dlogsn_ard_batch_0": float(g_ard[0, d]), "dlogsn_batch_0": float(g_iso[0, 1])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "ard_batch_bench", "kernel": "rbf", "dtype": "f64", "group": GROUP, "sigp_version": L.load().sigp_version()}
    rec["group_of_8"] = {"n=%d d=%d" % (n, d): group(n, d, a.reps) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
