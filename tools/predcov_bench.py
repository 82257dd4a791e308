"""The joint predictive covariance (GPR.predict_cov, sigp_predict_cov) beside the call it extends (GPR.predict), on one GPU through the
product library (no torch): RBF, d = 8, fp64, n = 8192 training points, m = 128 / 1024 / 2048 test points.

  calls     host clock around `predict` and `predict_cov` (synchronous on return, bracketed by sigp_synchronize): every shape warmed up,
            then `--reps` repeats with the calls ALTERNATING inside each repeat; median and best;
  kernels   the per-class split of ONE predict_cov call from sigp_profile (HIP events around the launches, in passes of their own):
            `kbuild` = the rows k~(Xs, X), `trsm` = the lockstep forward solve, `epilogue` = the covariance product (predcov_partial_kernel)
            + the finishing pass (predcov_finish_kernel); the product as a fraction of the solve of the same call and -- its n m_pad^2
            algorithmic flops (lower tile pairs) over the class's time -- of the fp64 MFMA peak;
  slices    all of it with `cov_slices` = 0 (auto split-K) and = 1 (one workgroup walks the whole K of its tile pair).

Prints one JSON line; `--out FILE` also writes it (profiles/r07_predcov_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_F64_MFMA_TFLOPS = 78.6    # MI355X dense fp64 matrix peak (bench.py)


def timed(gp, fn):
    gp.synchronize()
    t = time.perf_counter()
    fn()
    gp.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return {"median_ms": float(np.median(v)), "best_ms": float(np.min(v)), "reps": len(v)}


def run(n, ms_, reps):
    from oracle import gp_oracle as O
    from seaiceextentforecasting_amd import GPR
    d = 8
    X, y, _ = O.synthetic_problem(n, d, 20240000)
    ell, sn = np.sqrt(d), 1e-2
    out = {}
    with GPR(kernel="rbf") as gp:
        gp.fit(X, y, ell, sn)
        for m in ms_:
            Xs = O.synthetic_problem(m, d, 20240001 + m)[0]
            rec = {}
            for _ in range(2):                       # warm-up: every workspace allocated, both slice settings
                gp.predict(Xs)
                for s_ in (0, 1):
                    gp.set_option("cov_slices", s_)
                    gp.predict_cov(Xs)
            t = {"predict": [], "predict_cov_auto": [], "predict_cov_slices1": []}
            for _ in range(reps):
                t["predict"].append(timed(gp, lambda: gp.predict(Xs)))
                for s_, key in ((0, "predict_cov_auto"), (1, "predict_cov_slices1")):
                    gp.set_option("cov_slices", s_)
                    t[key].append(timed(gp, lambda: gp.predict_cov(Xs)))
            rec["calls"] = {k: stats(v) for k, v in t.items()}
            m_pad = (m + 127) // 128 * 128
            for s_, key in ((0, "auto"), (1, "slices1")):
                gp.set_option("cov_slices", s_)
                kern = {"kbuild": [], "trsm": [], "epilogue": []}
                for _ in range(reps):                # the launches alone: HIP events around them, in passes of their own
                    gp.profile_reset(); gp.profile(True, list(kern))
                    gp.predict_cov(Xs)
                    pg = gp.profile_get()
                    gp.profile(False)
                    for k in kern:
                        kern[k].append(pg[k]["ms"])
                prod, solve = float(np.median(kern["epilogue"])), float(np.median(kern["trsm"]))
                flops = pg["epilogue"]["flops"]
                rec["kernels_" + key] = {
                    "cov_slices": int(gp._stat("cov_slices")), "rows_ms": float(np.median(kern["kbuild"])), "solve_ms": solve, "product_ms": prod,
                    "product_ms_best": float(np.min(kern["epilogue"])), "product_over_solve": prod / solve,
                    "product_flops_accounted": flops, "product_tflops": float(n) * m_pad * m_pad * (1 + 128.0 / m_pad) / (prod * 1e-3) * 1e-12,
                }
                rec["kernels_" + key]["product_frac_of_fp64_mfma_peak"] = rec["kernels_" + key]["product_tflops"] / PEAK_F64_MFMA_TFLOPS
            rec["product_slices1_over_auto"] = rec["kernels_slices1"]["product_ms"] / rec["kernels_auto"]["product_ms"]
            gp.set_option("cov_slices", 0)
            out[str(m)] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, nargs="*", default=[128, 1024, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import _lib as L
    rec = {"tool": "predcov_bench", "kernel": "rbf", "d": 8, "dtype": "f64", "n": a.n, "sigp_version": L.load().sigp_version(),
           "peak_fp64_mfma_tflops": PEAK_F64_MFMA_TFLOPS,
           "note": "product = predcov_partial_kernel + predcov_finish_kernel (class epilogue); product_tflops counts the 2 x 128^2 x n_pad flops of every lower tile pair"}
    rec["m"] = run(a.n, a.m, a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
