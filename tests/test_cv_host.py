"""CPU tier of the leave-block-out cross-validation (include/sigp.h: sigp_cv, sigp_cv_batch, sigp_small_run_cv): the ABI is declared,
exported and bound; the argument checks that need no device; and the block closed form the GPU tests use as their yardstick
(DESIGN.md section 2), pinned here against REAL oracle refits without the removed window."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_loo_host import loo_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_SYMBOLS = {"sigp_cv": 7, "sigp_cv_batch": 13, "sigp_small_run_cv": 15}
# (n, block, gap): the minimum; a ragged last fold; clipped edge windows; a window of exactly 128; many small windows; leave-one-out;
# windows across row 128
CV_SHAPES = [(2, 1, 0), (37, 5, 0), (37, 5, 2), (300, 100, 14), (300, 7, 3), (300, 1, 0), (130, 64, 32)]


def cv_folds(n, block, gap):
    """[F, 4] = (r0, r1, c0, c1): fold f scores the rows [c0, c1) = [f block, min(n, (f + 1) block)) and removes [r0, r1) = [max(0, c0 - gap), min(n, c1 + gap))"""
    assert block >= 1 and gap >= 0
    out = []
    for c0 in range(0, n, block):
        c1 = min(n, c0 + block)
        out.append((max(0, c0 - gap), min(n, c1 + gap), c0, c1))
    return np.asarray(out, dtype=np.int64)


def cv_closed_form(Kt, y, block, gap, mode="refit"):
    """With P = K~^-1, a = P y and S a fold's window:  y_S - mean_S = P_SS^-1 a_S,  Cov_S = s_S P_SS^-1,
    s_S = (y^T a - a_S^T P_SS^-1 a_S) / (n - |S|) ("refit") or y^T a / n ("fixed"); the scored rows of every fold."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = len(y)
    P = np.linalg.inv(Kt)
    a = P @ y
    q = float(y @ a)
    mean, var, sf = np.zeros(n), np.zeros(n), np.zeros(n)
    for r0, r1, c0, c1 in cv_folds(n, block, gap):
        Ci = np.linalg.inv(P[r0:r1, r0:r1])
        r = Ci @ a[r0:r1]
        s = (q - float(a[r0:r1] @ r)) / (n - (r1 - r0)) if mode == "refit" else q / n
        sl = slice(c0 - r0, c1 - r0)
        mean[c0:c1] = y[c0:c1] - r[sl]
        var[c0:c1] = s * np.diag(Ci)[sl]
        sf[c0:c1] = s
    res = y - mean
    return dict(mean=mean, var=var, sigma_f=sf, nlpd=float(np.sum(0.5 * np.log(2 * np.pi * var) + res * res / (2 * var))), sse=float(np.sum(res * res)))


def oracle_block_refits(X, y, ell, sn, kind, M, block, gap):
    """fit without the rows of the fold's window, predict the scored rows -- for every fold (M, like the feature columns, stays the full set's)"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = len(y)
    mean, var, sf = np.zeros(n), np.zeros(n), np.zeros(n)
    for r0, r1, c0, c1 in cv_folds(n, block, gap):
        k = np.ones(n, dtype=bool)
        k[r0:r1] = False
        r = O.fit_predict(X[k], y[k].reshape(-1, 1), X[c0:c1], ell, sn, kind=kind, M=M, ref_idiom=False)
        mean[c0:c1], var[c0:c1], sf[c0:c1] = np.asarray(r["fmean"]).reshape(-1), np.asarray(r["fvar"]).reshape(-1), float(r["sigma_f"])
    return mean, var, sf


def cv_problem(kind, n, seed):
    """the smoke test's settings, as tests/test_hip_loo.py: (X, y, ell, sn~, M)"""
    if kind == "netdiffusion":
        X, y, _ = O.synthetic_problem(n, 12, seed)
        return X, y, 0.05, 1e-2, O.laplacian_M(X)
    X, y, _ = O.synthetic_problem(n, 8, seed)
    return X, y, np.sqrt(8.0), 1e-2, None


def test_cv_entry_points_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in CV_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"SIGP_CV_MAX_WINDOW\s*=\s*128\s*,\s*SIGP_CV_SMALL_MAX_WINDOW\s*=\s*32", hdr)
    assert "cv_slices" in hdr
    assert L.load().sigp_version() >= 540
    assert (L.CV_MAX_WINDOW, L.CV_SMALL_MAX_WINDOW) == (128, 32)


def test_cv_null_handle_and_null_buffers_are_rejected_before_any_device_work():
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.zeros(4)
    i64 = np.zeros(1, dtype=np.int64)
    assert lib.sigp_cv(None, 5, 0, 0, L.ptr(a), L.ptr(a), L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_cv(None, 5, 0, 0, None, None, None) == L.BAD_ARG
    assert lib.sigp_cv_batch(None, 0, 1, 1, L.ptr(a), L.ptr(a), 5, 0, 0, None, None, 0, L.ptr(a)) == L.BAD_ARG
    assert lib.sigp_small_run_cv(None, 1, L.iptr(i64), L.ptr(a), L.ptr(a), 5, 0, 0, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    assert lib.sigp_small_run_cv(None, 1, L.iptr(i64), L.ptr(a), L.ptr(a), 5, 0, 7, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    assert lib.sigp_small_run_cv(None, 1, L.iptr(i64), L.ptr(a), L.ptr(a), 0, 0, 0, L.ptr(a), None, None, 0, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG


def test_python_argument_checks_need_no_device():
    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd.retro import retro_grid_search
    for name in ("cv", "cv_batch", "cv_grid"):
        assert callable(getattr(S.GPR, name, None)), name
    gp = object.__new__(S.GPR)          # no handle, no device: every check below comes before the first library call
    gp._h, gp._fitted, gp.kernel, gp.dtype = None, False, "rbf", "f64"
    for kw in (dict(block=0), dict(block=-3), dict(block=5, gap=-1), dict(block=100, gap=15), dict(block=129), dict(block=5, sigma_f="bogus"), dict(block=2.5)):
        with pytest.raises(ValueError):
            gp.cv(**kw)
        with pytest.raises(ValueError):
            gp.cv_batch([1.0], [1e-2], **kw)
        with pytest.raises(ValueError):
            gp.cv_grid(np.zeros((40, 3)), np.zeros(40), [1.0], [1e-2], **kw)
    with pytest.raises(ValueError):
        gp.cv_grid(np.zeros((40, 3)), np.zeros(40), [1.0], [1e-2], block=20, gap=20)        # the first fold removes all 40 rows
    f = S.GPR.cv_folds(37, 5, 2)
    assert np.array_equal(f, cv_folds(37, 5, 2)) and f.shape == (8, 4)
    with pytest.raises(ValueError):
        retro_grid_search("September1st", {}, {}, 2000, 2001, criterion="bogus")
    with pytest.raises(ValueError):
        retro_grid_search("north_September", {}, {}, 2000, 2001, criterion="cv_nlpd", block=0)
    with pytest.raises(ValueError):
        retro_grid_search("north_September", {}, {}, 2000, 2001, criterion="cv_sse", block=30, gap=2)
    sb = S.SmallBatch(types.SimpleNamespace(kernel="netdiffusion", dtype="f64"))
    with pytest.raises(ValueError):
        sb.run(cv=dict(block=5), loo="refit")
    with pytest.raises(ValueError):
        sb.run(cv=dict(block=5), grad=True)
    for bad in (dict(block=0), dict(block=5, gap=-1), dict(block=30, gap=2), dict(block=5, sigma_f="bogus"), dict(gap=1), dict(block=5, extra=1), "refit"):
        with pytest.raises(ValueError):
            sb.run(cv=bad)


def test_folds_cover_every_row_once_and_windows_are_clipped():
    for n, block, gap in CV_SHAPES + [(129, 128, 0)]:
        f = cv_folds(n, block, gap)
        assert f[0, 2] == 0 and f[-1, 3] == n and np.array_equal(f[1:, 2], f[:-1, 3])
        assert np.all(f[:, 0] == np.maximum(f[:, 2] - gap, 0)) and np.all(f[:, 1] == np.minimum(f[:, 3] + gap, n))
        assert np.all(f[:, 1] - f[:, 0] <= block + 2 * gap) and np.all(n - (f[:, 1] - f[:, 0]) >= 1)


@pytest.mark.parametrize("kind", ["rbf", "matern52", "netdiffusion"])
@pytest.mark.parametrize("n,block,gap", CV_SHAPES)
def test_block_closed_form_equals_real_oracle_refits(kind, n, block, gap):
    """The yardstick of the GPU tests: the block closed form from inv(K~) == real fits without each fold's window, to 1e-10 (mean relative
    to max|y|, var and sigma_f relative)."""
    X, y, ell, sn, M = cv_problem(kind, n, 20250100 + n)
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    c = np.linalg.cond(Kt)
    assert c <= 1e6
    yv = np.asarray(y).reshape(-1)
    cf = cv_closed_form(Kt, yv, block, gap, "refit")
    mean, var, sf = oracle_block_refits(X, yv, ell, sn, kind, M, block, gap)
    e = (np.max(np.abs(cf["mean"] - mean)) / np.max(np.abs(yv)), np.max(np.abs(cf["var"] / var - 1)), np.max(np.abs(cf["sigma_f"] / sf - 1)))
    print("cond(K~) %.3g  mean %.3g  var %.3g  sigma_f %.3g" % ((c,) + e))
    assert max(e) <= 1e-10, e
    fx = cv_closed_form(Kt, yv, block, gap, "fixed")      # "fixed" differs from "refit" by the signal variance alone
    assert np.array_equal(fx["mean"], cf["mean"]) and np.allclose(fx["var"] / cf["var"], fx["sigma_f"] / cf["sigma_f"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("kind,n", [("rbf", 300), ("matern52", 37), ("netdiffusion", 40)])
def test_block_one_is_leave_one_out(kind, n):
    X, y, ell, sn, M = cv_problem(kind, n, 20250100 + n)
    Kt = O.fit_predict(X, y, X[:1], ell, sn, kind=kind, M=M, ref_idiom=False)["K_tilde"]
    yv = np.asarray(y).reshape(-1)
    for mode in ("refit", "fixed"):
        cv, loo = cv_closed_form(Kt, yv, 1, 0, mode), loo_closed_form(Kt, yv, mode)
        e = max(np.max(np.abs(cv["mean"] - loo["mean"])) / np.max(np.abs(yv)), np.max(np.abs(cv["var"] / loo["var"] - 1)),
                abs(cv["nlpd"] - loo["nlpd"]) / abs(loo["nlpd"]), abs(cv["sse"] / loo["sse"] - 1))
        print(kind, n, mode, e)
        assert e <= 1e-13
