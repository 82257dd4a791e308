"""Batches of small RBF / Matern-5/2 fits (n <= 128 rows, any number of features) with one length scale per fit or one per feature (ARD),
through ``sigp_small_upload`` / ``sigp_small_run_k*``: one workgroup per fit, everything in LDS, one launch for the whole list
(include/sigp.h).  The counterpart of ``SmallBatch`` for the stationary covariances: a retrospective study's (region, year) data sets
times a grid, or every start of an MLII optimisation over per-feature scales, at the size the application has -- where the blocked engine
pads each fit to a 128-tile and issues a dozen dependent launches per lockstep group.

A data set is staged once as its raw rows [X ; Xs]; every fit brings its own scales, the workgroup divides the features by them and builds
K~ = k(X, X) + sn~ I from squared distances summed by direct differences.  The leave-one-out, leave-block-out and hindcast flavours run the
reference kernel's own tails on that K~.  Not built: the score gradients (``SmallBatch.run(score_grad= / cv_grad=)``) -- the blocked
engine has them (``GPR.loo_ard_batch`` and its siblings).
"""
import numpy as np

from . import _lib as L
from .smallbatch import NMAX, MMAX


class SmallStationaryBatch:
    def __init__(self, gp):
        if gp.kernel not in ("rbf", "matern52") or gp.dtype != "f64":
            raise ValueError("SmallStationaryBatch runs the RBF / Matern-5/2 kernels on the fp64 engine (the reference kernel: SmallBatch)")
        self.gp = gp
        self._data = []          # (X, y, Xs): a data set is its own device set
        self._fits = []          # (data set, scales [1] or [N], sn)
        self._uploaded = 0

    # ---- building the list ---------------------------------------------------------------------------------------
    def add_dataset(self, X, y, Xs=None):
        """One data set: X [n, N] (n <= 128), y [n] or [n, 1], Xs [m, N] (m <= 8) or None.  Returns the data-set id."""
        X = L.f64(X, 2)
        y = L.f64(np.asarray(y).reshape(-1), 1)
        n, N = X.shape
        if y.shape[0] != n:
            raise ValueError("X has %d rows but y has %d" % (n, y.shape[0]))
        if not (1 <= n <= NMAX) or N < 1:
            raise ValueError("this path takes 1 <= n <= %d training rows of N >= 1 features (got %d x %d); larger fits go through GPR.fit" % (NMAX, n, N))
        if Xs is None:
            Xs = np.zeros((0, N))
        Xs = L.f64(np.atleast_2d(Xs), 2)
        if Xs.shape[1] != N or Xs.shape[0] > MMAX:
            raise ValueError("Xs must be [m <= %d, %d]" % (MMAX, N))
        self._data.append((X, y, Xs))
        return len(self._data) - 1

    def add_fit(self, ds, ell, sn_tilde):
        """Queue one fit of data set ``ds``: ``ell`` a scalar (one length scale) or a sequence of N (one per feature), sn~ >= 0.  Returns its
        index in the result arrays."""
        if not (0 <= int(ds) < len(self._data)):
            raise ValueError("data set %r of %d" % (ds, len(self._data)))
        N = self._data[ds][0].shape[1]
        ell = np.array(ell, dtype=np.float64).reshape(-1)
        if ell.shape[0] not in (1, N):
            raise ValueError("ell must be a scalar or a sequence of N = %d length scales (got %d)" % (N, ell.shape[0]))
        with np.errstate(divide="ignore", over="ignore"):
            if not np.all(np.isfinite(ell) & (ell > 0) & np.isfinite(1.0 / ell)):
                raise ValueError("every length scale must be finite and > 0 with a finite reciprocal")
        if not (float(sn_tilde) >= 0):
            raise ValueError("sn_tilde >= 0 required")
        self._fits.append((int(ds), ell, float(sn_tilde)))
        return len(self._fits) - 1

    # ---- device ---------------------------------------------------------------------------------------------------
    def upload(self):
        """Stage every data set queued so far in HBM (flat pools + offsets; the raw rows, ``lam`` unused)."""
        sets = self._data
        if not sets:
            raise RuntimeError("no data sets queued")
        n = np.array([s[0].shape[0] for s in sets], dtype=np.int64)
        N = np.array([s[0].shape[1] for s in sets], dtype=np.int64)
        m = np.array([s[2].shape[0] for s in sets], dtype=np.int64)
        mode = np.zeros(len(sets), dtype=np.int32)
        a_off = np.concatenate([[0], np.cumsum((n + m) * N)[:-1]]).astype(np.int64)
        y_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        l_off = np.concatenate([[0], np.cumsum(N)[:-1]]).astype(np.int64)
        A = np.concatenate([np.vstack([s[0], s[2]]).reshape(-1) for s in sets])
        y = np.concatenate([s[1] for s in sets])
        lam = np.zeros(int(N.sum()))
        gp = self.gp
        gp._check(gp._lib.sigp_small_upload(gp._h, len(sets), L.iptr(n), L.iptr(N), L.iptr(m), L.iptr(mode), L.ptr(A), L.iptr(a_off),
                                            L.ptr(y), L.iptr(y_off), L.ptr(lam), L.iptr(l_off)), "small_upload")
        self._uploaded = len(sets)
        self._mmax = int(m.max())

    def clear_fits(self):
        """Forget the queued fits; the data sets (and what is staged in HBM) stay."""
        self._fits = []

    def run(self, grad=False, loo=None, cv=None, hindcast=None):
        """All queued fits in one launch -> dict(sigma_f, nlml, info, sigma_n, mean [F, mmax], var [F, mmax]), +inf / NaN predictions where
        K~ is not positive definite, as ``SmallBatch.run``.

        ``grad=True`` (``sigp_small_run_k_grad``): also the exact gradient of the profiled nlML, grad_ell [F, Nmax] -- d/d log l_k of a fit
        with per-feature scales, NaN beyond its set's N; for a fit with one scale column 0 holds the derivative in the common log l and the
        rest is NaN -- and grad_sn [F] = d/d log sn~; +inf where K~ is not positive definite.  Every other key carries the bytes of the
        launch without it.

        ``loo="refit" | "fixed"``, ``cv=dict(block=, gap=0, sigma_f="refit")``, ``hindcast=dict(lead=1, min_train=2, sigma_f="refit")``: the
        same single launch validates every fit instead (``sigp_small_run_k_loo`` / ``_cv`` / ``_hindcast``), with the arguments, the result
        keys (loo_mean, loo_var [F, nmax], loo_nlpd, loo_sse [F]; cv_*; hindcast_*), the limits and the refusals of ``SmallBatch.run``; the
        keys of the plain launch carry its bytes.  One launch forms the gradient or one kind of validation: any two of the four raise
        ValueError.

        Fits with one scale and fits with per-feature scales may share a batch.  A batch of one-scale fits alone runs with one scale per
        fit (``ard = 0``); as soon as one fit has per-feature scales the launch takes N scales for every fit, the one-scale fits' repeated
        -- the workgroup divides by the same numbers, so the fit has the same bits -- and their common derivative is the sum of the N
        components in ascending k, which is what the ``ard = 0`` launch adds up itself."""
        if sum((bool(grad), loo is not None, cv is not None, hindcast is not None)) > 1:
            raise ValueError("one launch forms the gradients, the leave-one-out, the leave-block-out or the hindcast predictions: run them separately")
        if not self._fits:
            raise RuntimeError("no fits queued")
        from .gpr import GPR
        gp = self.gp
        if hindcast is not None:
            if not isinstance(hindcast, dict) or set(hindcast) - {"lead", "min_train", "sigma_f"}:
                raise ValueError("hindcast must be dict(lead=1, min_train=2, sigma_f='refit')")
            mode = hindcast.get("sigma_f", "refit")
            lead, mt = GPR._hindcast_args(gp, hindcast.get("lead", 1), hindcast.get("min_train", 2), mode, max_lead=L.HINDCAST_SMALL_MAX_LEAD)
            for X, _, _ in self._data:
                if mt + lead - 1 > X.shape[0] - 1:
                    raise ValueError("hindcast: a data set of %d rows has no scored row (min_train + lead - 1 = %d)" % (X.shape[0], mt + lead - 1))
            prefix, fn, extra = "hindcast", "sigp_small_run_k_hindcast", (lead, mt, L.LOO_MODES[mode])
        elif cv is not None:
            if not isinstance(cv, dict) or "block" not in cv or set(cv) - {"block", "gap", "sigma_f"}:
                raise ValueError("cv must be dict(block=, gap=0, sigma_f='refit')")
            mode = cv.get("sigma_f", "refit")
            block, gap = GPR._cv_args(cv["block"], cv.get("gap", 0), mode, max_window=L.CV_SMALL_MAX_WINDOW)
            for X, _, _ in self._data:
                GPR._cv_args(block, gap, mode, max_window=L.CV_SMALL_MAX_WINDOW, n=X.shape[0])
            prefix, fn, extra = "cv", "sigp_small_run_k_cv", (block, gap, L.LOO_MODES[mode])
        elif loo is not None:
            if loo not in L.LOO_MODES:
                raise ValueError("loo must be None, 'refit' or 'fixed'")
            prefix, fn, extra = "loo", "sigp_small_run_k_loo", (L.LOO_MODES[loo],)
        else:
            prefix, fn, extra = None, "sigp_small_run_k_grad" if grad else "sigp_small_run_k", ()
        if self._uploaded != len(self._data):
            self.upload()
        F = len(self._fits)
        si = np.array([f[0] for f in self._fits], dtype=np.int64)
        sn = np.array([f[2] for f in self._fits], dtype=np.float64)
        Nof = np.array([self._data[f[0]][0].shape[1] for f in self._fits])
        one = np.array([f[1].shape[0] == 1 and self._data[f[0]][0].shape[1] != 1 for f in self._fits])     # one scale for several features
        ard = int(not np.all([f[1].shape[0] == 1 for f in self._fits]))
        ldell = int(Nof.max()) if ard else 1
        ell = np.ones((F, ldell))
        for i, (_, l, _) in enumerate(self._fits):
            ell[i, :Nof[i] if ard else 1] = l
        ms = max(self._mmax, 1)
        width = 6 if prefix else 4
        out = np.zeros((F, width)); mean = np.full((F, ms), np.nan); var = np.full((F, ms), np.nan)
        args = extra + (L.ptr(out), L.ptr(mean), L.ptr(var), ms)
        if prefix:       # a prediction per training row
            nmax = max(s[0].shape[0] for s in self._data)
            rmean = np.full((F, nmax), np.nan); rvar = np.full((F, nmax), np.nan)
            args += (L.ptr(rmean), L.ptr(rvar), nmax)
        if grad:
            ldg = ldell + 1
            g = np.full((F, ldg), np.nan)
            args += (L.ptr(g), ldg)
        gp._check(getattr(gp._lib, fn)(gp._h, F, L.iptr(si), gp._kid, L.ptr(ell), ldell, ard, L.ptr(sn), *args), fn[5:])
        gp._fitted = False
        res = dict(sigma_f=out[:, 0], nlml=out[:, 1], info=out[:, 2].astype(np.int64), sigma_n=out[:, 3],
                   mean=mean[:, :self._mmax], var=var[:, :self._mmax])
        if prefix:
            res.update({prefix + "_mean": rmean, prefix + "_var": rvar, prefix + "_nlpd": out[:, 4].copy(), prefix + "_sse": out[:, 5].copy()})
        if grad:
            Nmax = int(Nof.max())
            ge = np.full((F, Nmax), np.nan)
            nl = Nof if ard else np.ones(F, dtype=np.int64)
            for i in range(F):
                ge[i, :nl[i]] = g[i, :nl[i]]
                if ard and one[i]:      # the common derivative: the components added in ascending k
                    ge[i, 0] = np.cumsum(g[i, :nl[i]])[-1]
                    ge[i, 1:] = np.nan
            res["grad_ell"], res["grad_sn"] = ge, g[np.arange(F), nl].copy()
        return res
