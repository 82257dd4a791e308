"""The inducing-point (sparse) fit (GPR.sparse_fit, sigp_sparse_fit) on one GPU through the product library (no torch): RBF, d = 8, fp64,
BASELINE.md's synthetic generator (oracle.synthetic_problem), l = sqrt(d), sn~ = 1e-2, jitter 1e-6, inducing points a seeded random subset.

  fits      n = 65536 / 262144 / 1048576 x m = 1024 / 2048 at the default sparse_chunk: host clock around `sparse_fit` (synchronous on
            return), one warm-up, then `--reps` repeats; the three phases of the call from sigp_get_stat (host clock, each closed by a
            synchronisation: Z + factor of k(Z,Z), the chunk loop, B + its factor) and, from a profiled pass of its own (HIP events around
            the launches), the chunk loop's split: `kbuild` = k(Z, X_c) (+ the one build of k(Z,Z)), `trsm` = the whitening (+ the panel
            solves of the two factorisations), `syrk128` = V_c V_c^T (+ the factorisations' trailing updates); the rate of the two cubic
            steps (n m_pad^2 flops each as accounted) beside
  dense     the trailing update's rate in a dense n = 8192 fit of the same run (class syrk128 of sigp_profile);
  chunks    the same fit at sparse_chunk = 2048 / 4096 / 8192 / 16384 (n = 262144, m = 2048);
  quality   n = 16384: `sparse_fit` with m = 512 .. 4096 `farthest` inducing points beside the dense `fit`: time, and the RMSE of the
            predictive mean against the dense one on 1024 held-out points.

Prints one JSON line; `--out FILE` also writes it (profiles/r22_sparse_bench.json).  `--quick` runs a reduced set (smoke of the tool)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_F64_MFMA_TFLOPS = 78.6    # MI355X dense fp64 matrix peak (bench.py)
D, SN, JITTER = 8, 1e-2, 1e-6


def clock(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def problem(n, seed=20240000):
    from oracle import gp_oracle as O
    X, y, _ = O.synthetic_problem(n, D, seed)
    return X, y


def sparse_record(gp, X, y, Z, reps, chunk=None):
    if chunk is not None:
        gp.set_option("sparse_chunk", chunk)
    ell = np.sqrt(D)
    n, m = X.shape[0], Z.shape[0]
    m_pad = (m + 127) // 128 * 128
    gp.sparse_fit(X, y, Z, ell, SN, jitter=JITTER)                     # warm-up: every workspace allocated
    t, phases = [], []
    for _ in range(reps):
        ms, r = clock(lambda: gp.sparse_fit(X, y, Z, ell, SN, jitter=JITTER))
        t.append(ms)
        phases.append([gp._stat("sparse_factor_a_ms"), gp._stat("sparse_chunks_ms"), gp._stat("sparse_factor_b_ms")])
    gp.profile_reset(); gp.profile(True)
    gp.sparse_fit(X, y, Z, ell, SN, jitter=JITTER)
    pg = gp.profile_get()
    gp.profile(False); gp.profile_reset()
    ph = np.median(np.asarray(phases), axis=0)
    cubic = float(n) * m_pad * m_pad                                   # flops of the whitening, and of V V^T
    rec = {"n": n, "m": m, "sparse_chunk": chunk, "fit_ms_median": float(np.median(t)), "fit_ms_best": float(np.min(t)), "reps": reps,
           "sigma_f": r["sigma_f"], "nlml": r["nlml"], "bound": r["bound"],
           "phase_ms": {"factor_kmm": float(ph[0]), "chunks": float(ph[1]), "factor_b": float(ph[2])},
           "class_ms": {k: pg[k]["ms"] for k in ("kbuild", "trsm", "syrk128", "diag", "update_small", "epilogue")},
           "whitening_tflops": cubic / (pg["trsm"]["ms"] * 1e-3) * 1e-12 if pg["trsm"]["ms"] > 0 else None,
           "accumulation_tflops": cubic / (pg["syrk128"]["ms"] * 1e-3) * 1e-12 if pg["syrk128"]["ms"] > 0 else None,
           "fit_tflops": 2.0 * cubic / (float(np.median(t)) * 1e-3) * 1e-12}
    return rec


def dense_update_rate(gp, n=8192):
    X, y = problem(n, 20240008)
    gp.fit(X, y, np.sqrt(D), SN)
    gp.profile_reset(); gp.profile(True, ["syrk128"])
    ms, _ = clock(lambda: gp.refit(np.sqrt(D), SN))
    pg = gp.profile_get()
    gp.profile(False); gp.profile_reset()
    s = pg["syrk128"]
    return {"n": n, "fit_ms_profiled": ms, "syrk128_ms": s["ms"], "syrk128_flops": s["flops"],
            "syrk128_tflops": s["flops"] / (s["ms"] * 1e-3) * 1e-12 if s["ms"] > 0 else None}


def quality(gp, ms_, n=16384, held=1024):
    from seaiceextentforecasting_amd import select_inducing
    Xa, ya = problem(n + held, 20240016)
    X, y, Xs = Xa[:n], ya[:n], Xa[n:]
    ell = np.sqrt(D)
    gp.fit(X, y, ell, SN)
    t_dense, _ = clock(lambda: gp.refit(ell, SN))
    dmean, _ = gp.predict(Xs)
    out = {"n": n, "held_out": held, "dense_fit_ms": t_dense, "dense_rmse_to_targets": float(np.sqrt(np.mean((dmean - ya[n:]) ** 2))), "m": {}}
    for m in ms_:
        t_sel, Z = clock(lambda: select_inducing(X, m, "farthest", 0))
        gp.sparse_fit(X, y, Z, ell, SN, jitter=JITTER)
        t_fit, r = clock(lambda: gp.sparse_fit(X, y, Z, ell, SN, jitter=JITTER))
        t_pred, (mean, _) = clock(lambda: gp.sparse_predict(Xs))
        out["m"][str(m)] = {"select_ms_host": t_sel, "fit_ms": t_fit, "predict_ms": t_pred, "bound": r["bound"], "nlml": r["nlml"],
                            "rmse_mean_vs_dense": float(np.sqrt(np.mean((mean - dmean) ** 2))),
                            "rmse_to_targets": float(np.sqrt(np.mean((mean - ya[n:]) ** 2)))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from seaiceextentforecasting_amd import GPR, _lib as L
    ns, ms_ = ((65536,), (1024,)) if a.quick else ((65536, 262144, 1048576), (1024, 2048))
    chunks = (2048, 8192) if a.quick else (2048, 4096, 8192, 16384)
    rec = {"tool": "sparse_bench", "kernel": "rbf", "d": D, "dtype": "f64", "sn_tilde": SN, "jitter": JITTER, "sigp_version": L.load().sigp_version(),
           "peak_fp64_mfma_tflops": PEAK_F64_MFMA_TFLOPS,
           "note": "whitening / accumulation_tflops: n m_pad^2 flops over the class's time of ONE profiled fit (the class also holds the two factorisations' share)"}
    rng = np.random.default_rng(1)
    with GPR(kernel="rbf") as gp:
        rec["dense_update"] = dense_update_rate(gp)
        rec["fits"] = []
        for n in ns:
            X, y = problem(n)
            for m in ms_:
                Z = X[np.sort(rng.choice(n, size=m, replace=False))]
                gp.set_option("sparse_chunk", 4096)
                rec["fits"].append(sparse_record(gp, X, y, Z, a.reps))
        n, m = (65536, 1024) if a.quick else (262144, 2048)
        X, y = problem(n)
        Z = X[np.sort(rng.choice(n, size=m, replace=False))]
        rec["chunks"] = [sparse_record(gp, X, y, Z, a.reps, chunk) for chunk in chunks]
        gp.set_option("sparse_chunk", 4096)
        rec["quality"] = quality(gp, (512,) if a.quick else (512, 1024, 2048, 4096), n=4096 if a.quick else 16384)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
