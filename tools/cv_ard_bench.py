"""The per-feature (ARD) gradient of a leave-block-out score beside the calls it competes with, on one GPU through the product library (no
torch), modelled on tools/loo_ard_bench.py:

  single fits (RBF, fp64; default n = 4096 8192, d = 8 64) at equal length scales, so that every call factors the same matrix.  All calls
      ALTERNATE inside each repeat of one run: `refit`, `loo()`, `loo_ard`, and for every (block, gap) of --folds (default 5,0 128,0 16,8 1,0)
      `cv(block, gap)` on that fit and `cv_ard(block, gap)` (which fits first) -- host clock around calls that are synchronous on return,
      bracketed by sigp_synchronize; every shape warmed up twice, then `--reps` repeats; median and best reported.
  the SIGP_KC_MLII entries of ONE `cv_ard` call per (block, gap), step by step (HIP events from sigp_profile; the library prints every
      bracketed entry at set_option("host_timing", 2), and the tool reads them back from a redirected stderr): the triangular inversion, per
      pass of 1024 folds the four steps of `cv` and the two new ones (fold adjoints, assembly), then U U^T, the n^2 passes, the banded
      product P B, the product M = (P B) P^T and the ARD tile pass.
  ratios, per (block, gap):
      cv_ard_over_parts        = cv_ard / (refit + cv + (loo_ard - refit - loo))        the same work from calls that exist already: a fit, the
                                 scores, and loo_ard's gradient part (U U^T, the n^2 passes, one cubic product, the tile pass)
      cv_ard_over_loo_ard      the plain quotient (loo_ard re-measured in this run; its record is profiles/r11_loo_ard_bench.json)
      band_product_over_model  the banded product's time / (its flop count / the rate the product M reached in the same call): both are
                                 syrk128_tile's SET form, M with K = n_pad, the banded product with K = 384 (256 in the two edge block columns)

Prints one JSON line; `--out FILE` also writes it (the committed record: profiles/r12_cv_ard_bench.json)."""
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

LAUNCH = re.compile(r"\[sigp-launch\] class (\d+) K (\d+) gflop ([0-9.eE+-]+) ms ([0-9.eE+-]+)")


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {k: {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "reps": len(v)} for k, v in ms.items()}


def mlii_entries(gp, fn):
    """[(gflop, ms)] of the SIGP_KC_MLII entries of fn(), in launch order"""
    gp.profile_reset(); gp.profile(True, ["mlii"]); gp.set_option("host_timing", 2)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
            total = gp.profile_get()["mlii"]           # drains the events: the library prints them here
        finally:
            os.dup2(saved, 2); os.close(saved)
            gp.set_option("host_timing", 0); gp.profile(False)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    ent = [(float(m.group(3)), float(m.group(4))) for m in LAUNCH.finditer(text) if int(m.group(1)) == 7]
    return ent, total


def steps_of(ent, passes):
    """name the entries of one cv_ard call: 1 + 6 passes + 5"""
    if len(ent) != 1 + 6 * passes + 5:
        return {"error": "expected %d entries, got %d" % (1 + 6 * passes + 5, len(ent))}
    per = ("strip_products", "strip_finish", "fold_cholesky", "closing_solves", "fold_adjoints", "assembly")
    out = {"triangular_inversion_ms": ent[0][1]}
    for i, nm in enumerate(per):
        out[nm + "_ms"] = float(sum(ent[1 + 6 * p + i][1] for p in range(passes)))
    tail = ent[1 + 6 * passes:]
    for nm, (gf, ms) in zip(("u_ut", "n2_passes", "band_product", "product_m", "ard_tile_pass"), tail):
        out[nm + "_ms"] = ms
        out[nm + "_gflop"] = gf
    rate = out["product_m_gflop"] / out["product_m_ms"]                 # GFLOP per ms
    out["product_m_tflops"] = rate
    out["band_product_tflops"] = out["band_product_gflop"] / out["band_product_ms"]
    out["band_product_model_ms"] = out["band_product_gflop"] / rate
    out["band_product_over_model"] = out["band_product_ms"] / out["band_product_model_ms"]
    return out


def single(n, d, reps, folds):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    th_ard = np.log([ell] * d + [sn])
    ms = {}
    with GPR(kernel="rbf") as gp:
        gp.set_data(X, y)
        names = ["fit", "loo_after_fit", "loo_ard"]
        for r in range(2 + reps):                  # two warm-up rounds: every shape, every workspace allocated
            seq = [("fit", lambda: gp.refit(ell, sn)), ("loo_after_fit", lambda: gp.loo()), ("loo_ard", lambda: gp.loo_ard(th_ard))]
            for b, g in folds:
                seq.append(("fit", lambda: gp.refit(ell, sn)))                     # cv runs on an isotropic fit of the same matrix
                seq.append(("cv_after_fit block=%d gap=%d" % (b, g), lambda b=b, g=g: gp.cv(b, g)))
                seq.append(("cv_ard block=%d gap=%d" % (b, g), lambda b=b, g=g: gp.cv_ard(th_ard, b, gap=g)))
                seq.append(("cv_ard_value_only block=%d gap=%d" % (b, g), lambda b=b, g=g: gp.cv_ard(th_ard, b, gap=g, grad=None)))
            for k, fn in seq:
                t = timed(gp, fn)
                if r >= 2:
                    ms.setdefault(k, []).append(t)
        out = summary(ms)
        fit, loo, loo_ard = (out[k]["median_ms"] for k in names)
        out["folds"] = {}
        for b, g in folds:
            tag = "block=%d gap=%d" % (b, g)
            passes = (-(-n // b) + 1023) // 1024
            ent, total = mlii_entries(gp, lambda: gp.cv_ard(th_ard, b, gap=g))
            v, gr = gp.cv_ard(th_ard, b, gap=g)
            cv, cv_ard = out["cv_after_fit " + tag]["median_ms"], out["cv_ard " + tag]["median_ms"]
            out["folds"][tag] = {"passes": passes, "mlii_class": {"ms": total["ms"], "launches": total["launches"], "flops": total["flops"]},
                                 "steps": steps_of(ent, passes),
                                 "cv_ard_over_parts": cv_ard / (fit + cv + (loo_ard - fit - loo)),
                                 "cv_ard_over_loo_ard": cv_ard / loo_ard,
                                 "value": float(v), "grad_sum_dlogl": float(np.sum(gr[:d])), "grad_dlogsn": float(gr[d])}
        lv, lg = gp.loo_ard(th_ard)
        c1 = gp.cv_ard(th_ard, 1)
        # block = 1 without a gap is leave-one-out (a check of the run, not a tolerance)
        out["check"] = {"loo_ard_nlpd": float(lv), "cv_ard_block1_nlpd": float(c1[0]), "loo_ard_sum_dlogl": float(np.sum(lg[:d])),
                        "cv_ard_block1_sum_dlogl": float(np.sum(c1[1][:d])), "loo_ard_dlogsn": float(lg[d]), "cv_ard_block1_dlogsn": float(c1[1][d])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--d", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--folds", nargs="*", default=["5,0", "128,0", "16,8", "1,0"], help="block,gap pairs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    folds = [tuple(int(v) for v in f.split(",")) for f in a.folds]
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "cv_ard_bench", "kernel": "rbf", "dtype": "f64", "sigp_version": L.load().sigp_version()}
    rec["single"] = {"n=%d d=%d" % (n, d): single(n, d, a.reps, folds) for n in a.n for d in a.d}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
