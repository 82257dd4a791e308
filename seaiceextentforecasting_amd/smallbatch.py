"""Batches of the reference's own GP at the reference's own size -- the retro loop
(north/retrospective_forecasts/September1st_retro.py:176-248: 3 regions x ~40 years, n = year - 1979 <= 45) times the
20 x 20 (l, sn~) grid of north/June1st.py:210-211 -- through ``sigp_small_upload`` / ``sigp_small_run``: one workgroup per
fit, one launch for the whole list (include/sigp.h).

Host side: data sets are staged in factored form so that the device never needs ``expm``:

  expm="eigh"  M = Q diag(lam) Q^T once per data set;  A = [X ; Xs] Q, weights exp(l lam) formed on the device
               for every l of a grid.
  expm="pade"  Sigma~ = scipy.linalg.expm(l M) per (data set, l) as the reference does (north/June1st.py:264), then
               Sigma~ = U diag(s) U^T;  A = [X ; Xs] U, weights s.  Reproduces the reference's numbers also for its
               extreme table entry l = 3.1e10, at one host eigendecomposition per (data set, l).

``run(grad=True)`` is the MLII closure (north/June1st.py:235-257) for the whole list in the same single launch: the value, the
reference's own "gradient" formulae (:248-252) and the exact derivative (``sigp_small_run_grad``).  M Sigma~ needs no second
matrix: in the eigenbasis it is the reweighting lam_k exp(l lam_k); "pade" sets carry u_k^T M u_k * s_k instead.
"""
import numpy as np

from . import _lib as L
from .features import laplacian_M, sigma_tilde

NMAX, MMAX = 128, 8


class SmallBatch:
    def __init__(self, gp):
        if gp.kernel != "netdiffusion" or gp.dtype != "f64":
            raise ValueError("SmallBatch runs the reference kernel on the fp64 engine")
        self.gp = gp
        self._data = []          # (X, y, Xs, M)
        self._eig = {}           # ds -> (lam, Q)
        self._sets = []          # device sets: (A, y, lam, mode, dlam)
        self._set_of = {}        # (ds, None) or (ds, ell) -> device set index
        self._fits = []          # (device set, ell, sn)
        self._packed = None      # the fit list as arrays (rebuilt after add_fit)
        self._uploaded = 0

    # ---- building the list ---------------------------------------------------------------------------------------
    def add_dataset(self, X, y, Xs=None, M=None):
        """One (region, year): X [n, N], y [n] or [n, 1], Xs [m, N] (m <= 8) or None, M = the graph Laplacian
        (north/June1st.py:231-233; computed from X when omitted).  Returns the data-set id."""
        X = L.f64(X, 2)
        y = L.f64(np.asarray(y).reshape(-1), 1)
        n, N = X.shape
        if y.shape[0] != n:
            raise ValueError("X has %d rows but y has %d" % (n, y.shape[0]))
        if not (1 <= n <= NMAX):
            raise ValueError("this path takes 1 <= n <= %d training rows (got %d); larger fits go through GPR.fit" % (NMAX, n))
        if Xs is None:
            Xs = np.zeros((0, N))
        Xs = L.f64(np.atleast_2d(Xs), 2)
        if Xs.shape[1] != N or Xs.shape[0] > MMAX:
            raise ValueError("Xs must be [m <= %d, %d]" % (MMAX, N))
        M = laplacian_M(X) if M is None else L.f64(M, 2)
        if M.shape != (N, N):
            raise ValueError("M must be %dx%d" % (N, N))
        self._data.append((X, y, Xs, M))
        return len(self._data) - 1

    def _device_set(self, ds, ell, expm):
        key = (ds, None) if expm == "eigh" else (ds, float(ell))
        idx = self._set_of.get(key)
        if idx is not None:
            return idx
        X, y, Xs, M = self._data[ds]
        XX = np.vstack([X, Xs])
        if expm == "eigh":
            if ds not in self._eig:
                lam, Q = np.linalg.eigh(0.5 * (M + M.T))
                self._eig[ds] = (np.minimum(lam, 0.0), Q)      # the exact spectrum is <= 0
            lam, Q = self._eig[ds]
            dev = (np.ascontiguousarray(XX @ Q), y, np.ascontiguousarray(lam), 0, np.zeros_like(lam))
        else:
            Sig = sigma_tilde(M, float(ell))
            if not np.all(np.isfinite(Sig)):
                raise FloatingPointError("expm(l M) overflowed")
            s, U = np.linalg.eigh(0.5 * (Sig + Sig.T))
            # M and Sigma~ = expm(l M) share eigenvectors: M Sigma~ = U diag(mu s) U^T with mu_k = u_k^T M u_k (the MLII gradient's
            # d Sigma/dl, north/June1st.py:248); inside a degenerate cluster of s the choice of U does not matter where s ~ 0
            mu = np.einsum("ik,ij,jk->k", U, M, U)
            dev = (np.ascontiguousarray(XX @ U), y, np.ascontiguousarray(s), 1, np.ascontiguousarray(mu * np.maximum(s, 0.0)))
        self._sets.append(dev)
        self._set_of[key] = len(self._sets) - 1
        return self._set_of[key]

    def add_fit(self, ds, ell, sn_tilde, expm="eigh"):
        """Queue one fit of data set ``ds`` at (l, sn~).  Returns its index in the result arrays."""
        if expm not in ("eigh", "pade"):
            raise ValueError("expm must be 'eigh' or 'pade'")
        if not (float(ell) > 0) or not (float(sn_tilde) >= 0):
            raise ValueError("ell > 0 and sn_tilde >= 0 required")
        self._fits.append((self._device_set(ds, ell, expm), float(ell), float(sn_tilde)))
        self._packed = None
        return len(self._fits) - 1

    # ---- device ---------------------------------------------------------------------------------------------------
    def upload(self, dweights=True):
        """Stage every data set queued so far in HBM (flat pools + offsets).  ``dweights=False`` leaves out the M Sigma~ weights of the "pade"
        sets (``sigp_small_set_dweights``): their d/d log l entries are then NaN."""
        sets = self._sets
        if not sets:
            raise RuntimeError("no fits queued")
        n = np.array([s[1].shape[0] for s in sets], dtype=np.int64)
        N = np.array([s[0].shape[1] for s in sets], dtype=np.int64)
        m = np.array([s[0].shape[0] - s[1].shape[0] for s in sets], dtype=np.int64)
        mode = np.array([s[3] for s in sets], dtype=np.int32)
        a_off = np.concatenate([[0], np.cumsum((n + m) * N)[:-1]]).astype(np.int64)
        y_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        l_off = np.concatenate([[0], np.cumsum(N)[:-1]]).astype(np.int64)
        A = np.concatenate([s[0].reshape(-1) for s in sets])
        y = np.concatenate([s[1] for s in sets])
        lam = np.concatenate([s[2] for s in sets])
        gp = self.gp
        gp._check(gp._lib.sigp_small_upload(gp._h, len(sets), L.iptr(n), L.iptr(N), L.iptr(m), L.iptr(mode), L.ptr(A), L.iptr(a_off),
                                            L.ptr(y), L.iptr(y_off), L.ptr(lam), L.iptr(l_off)), "small_upload")
        if mode.any() and dweights:
            dlam = np.concatenate([s[4] for s in sets])
            gp._check(gp._lib.sigp_small_set_dweights(gp._h, L.ptr(dlam), len(dlam)), "small_set_dweights")
        self._uploaded = len(sets)
        self._mmax = int(m.max())

    def clear_fits(self):
        """Forget the queued fits; the data sets (and what is staged in HBM) stay."""
        self._fits = []
        self._packed = None

    def run(self, grad=False, loo=None, cv=None, hindcast=None, score_grad=None, cv_grad=None):
        """All queued fits in one launch -> dict(sigma_f, nlml, info, sigma_n, mean [F, mmax], var [F, mmax]); with ``grad=True``
        also grad_ref [F, 2] (the reference's MLII formulae, north/June1st.py:248-252) and grad_exact [F, 2] (the derivative of the
        profiled nlML w.r.t. (log l, log sn~)); +inf where K~ is not positive definite (:254-256).

        ``loo="refit"`` / ``"fixed"``: the same single launch also cross-validates every fit leave-one-out with (l, sn~) held
        (``sigp_small_run_loo``; "refit" re-profiles sigma_f without the left-out point -- what a fit on the other n - 1 points
        returns --, "fixed" keeps the full fit's sigma_f): loo_mean, loo_var [F, nmax] (NaN beyond a data set's n), loo_nlpd,
        loo_sse [F] (+inf / NaN rows where K~ is not positive definite).  One launch forms the gradients or the leave-one-out
        predictions: ``grad=True`` together with ``loo`` raises ValueError.

        ``cv=dict(block=, gap=0, sigma_f="refit")``: the same single launch cross-validates every fit leave-block-out instead
        (``sigp_small_run_cv``; folds and modes as ``GPR.cv``, block + 2 gap <= 32, every fold of every data set must leave a training row):
        cv_mean, cv_var [F, nmax] (NaN beyond a data set's n), cv_nlpd, cv_sse [F] (+inf / NaN rows where K~ or a fold's block of K~^-1 is
        not positive definite).  Mutually exclusive with ``loo`` and ``grad``.  The folds' LDS limits the largest order of the batch by its
        largest m: 128 (m <= 2), 127 (m = 3 .. 5), 126 (m = 6), 125 (m = 7, 8); beyond it ValueError, and the batch still runs every other
        launch.  To fit, the launch may build K~ from shorter feature chunks than ``run()`` does (largest order from 119 at m = 0, 118 at
        m = 1, 2, 114 at m = 8): where a set then has more features than the chunk, sigma_f, nlml, sigma_n, mean and var of this launch agree
        with ``run()``'s to rounding, not bit for bit.

        ``hindcast=dict(lead=1, min_train=2, sigma_f="refit")``: the same single launch validates every fit by the expanding-window hindcast
        instead (``sigp_small_run_hindcast``; rows and modes as ``GPR.hindcast``, lead <= 32, every data set must have a scored row:
        min_train + lead - 1 <= n - 1): hindcast_mean, hindcast_var [F, nmax] (NaN where a row is not scored and beyond a data set's n),
        hindcast_nlpd, hindcast_sse [F] (+inf / NaN rows where K~ is not positive definite).  L~ and z are read where the factorisation left
        them; no inverse is formed.  Mutually exclusive with ``grad``, ``loo`` and ``cv``.

        ``score_grad="nlpd"`` / ``"sse"`` with ``loo=`` or ``hindcast=``: the same single launch also differentiates that score of every fit
        with respect to (log l, log sn~), (l, sn~) held and sigma_f re-profiled as the mode says (``sigp_small_run_loo_grad`` /
        ``sigp_small_run_hindcast_grad``): loo_grad / hindcast_grad [F, 2]; every other key carries the bytes of the launch without it (where no
        data set has more features than the launch's feature chunk, as for ``cv``).  "pade" fits take d/d log l through the staged M Sigma~
        weights, as ``grad=True`` does.  +inf where K~ is not positive definite.  The launch keeps more in LDS: every batch whose largest order
        is <= 96 runs (any m <= 8, any lead <= 32); beyond that leave-one-out takes n <= 128 up to m = 6 and n <= 127 at m = 7, 8, the hindcast
        at lead = 1 n <= 128 up to m = 5 and n <= 127 above, and at n = 128, m = 0 lead <= 6; what does not fit raises ValueError (the
        library's SIGP_BAD_ARG, whose message names the bytes needed and the limit) and the batch still runs every other launch.  From order 97
        on the launch may build K~ from shorter feature chunks than the score launch does: sets with more features than the chunk then agree
        with it to rounding, not byte for byte.  ``cv=`` with ``score_grad`` raises: the leave-block-out gradients come through ``cv_grad=``.

        ``cv_grad=dict(block=, gap=0, sigma_f="refit", score="nlpd" | "sse")``: what ``cv=dict(block=, gap=, sigma_f=)`` returns -- the same bytes,
        where no data set has more features than the launch's feature chunk -- and cv_grad [F, 2], the derivatives of that leave-block-out score
        with respect to (log l, log sn~), in the same single launch (``sigp_small_run_cv_grad``; the adjoint of ``GPR.cv_ard``, its banded B kept
        in LDS).  A flavour of its own: mutually exclusive with ``grad``, ``loo``, ``cv``, ``hindcast`` and ``score_grad``.  +inf in the scores and
        the gradient where K~ or a fold's block of K~^-1 is not positive definite; "pade" fits as above.  Every batch whose largest order is
        <= 96 runs (any m <= 8, any window block + 2 gap <= 32); beyond that the largest order is 123 / 121 / 119 / 116 / 109 at m = 0 and
        119 / 117 / 115 / 113 / 106 at m = 8 for windows 1 / 5 / 8 / 16 / 32; what does not fit raises ValueError (the library's message names
        n, m, the window, the bytes needed and the limit) and the batch still runs every other launch."""
        if cv_grad is not None:
            if grad or loo is not None or cv is not None or hindcast is not None or score_grad is not None:
                raise ValueError("one launch forms the gradients, the leave-one-out, the leave-block-out or the hindcast predictions: run them separately "
                                 "(cv_grad is a flavour of its own: the leave-block-out predictions and the gradient of one of their scores)")
            if not isinstance(cv_grad, dict) or "block" not in cv_grad or set(cv_grad) - {"block", "gap", "sigma_f", "score"}:
                raise ValueError("cv_grad must be dict(block=, gap=0, sigma_f='refit', score='nlpd' | 'sse')")
            if cv_grad.get("score", "nlpd") not in self._SCORE_IDS:
                raise ValueError("cv_grad: score must be 'nlpd' or 'sse'")
            cv = {k: v for k, v in cv_grad.items() if k != "score"}
        if score_grad is not None:
            if cv is not None:
                raise ValueError("score_grad: block-CV gradients are not built in the one-workgroup kernel (loo= and hindcast= have them)")
            if score_grad not in ("nlpd", "sse"):
                raise ValueError("score_grad must be None, 'nlpd' or 'sse'")
            if loo is None and hindcast is None:
                raise ValueError("score_grad differentiates a row score: pass loo= or hindcast= with it (grad=True is the nlML's gradient)")
        if hindcast is not None:
            if loo is not None or grad or cv is not None:
                raise ValueError("one launch forms the gradients, the leave-one-out, the leave-block-out or the hindcast predictions: run them separately")
            if not isinstance(hindcast, dict) or set(hindcast) - {"lead", "min_train", "sigma_f"}:
                raise ValueError("hindcast must be dict(lead=1, min_train=2, sigma_f='refit')")
            hc_mode = hindcast.get("sigma_f", "refit")
            hc_lead, hc_mt = self.gp._hindcast_args(hindcast.get("lead", 1), hindcast.get("min_train", 2), hc_mode, max_lead=L.HINDCAST_SMALL_MAX_LEAD)
            for X, _, _, _ in self._data:
                if hc_mt + hc_lead - 1 > X.shape[0] - 1:
                    raise ValueError("hindcast: a data set of %d rows has no scored row (min_train + lead - 1 = %d)" % (X.shape[0], hc_mt + hc_lead - 1))
        if loo is not None and loo not in L.LOO_MODES:
            raise ValueError("loo must be None, 'refit' or 'fixed'")
        if loo is not None and grad:
            raise ValueError("one launch forms the MLII gradients or the leave-one-out predictions: run(grad=True) and run(loo=...) separately")
        if cv is not None:
            if loo is not None or grad:
                raise ValueError("one launch forms the gradients, the leave-one-out or the leave-block-out predictions: run them separately")
            if not isinstance(cv, dict) or "block" not in cv or set(cv) - {"block", "gap", "sigma_f"}:
                raise ValueError("cv must be dict(block=, gap=0, sigma_f='refit')")
            from .gpr import GPR
            cv_mode = cv.get("sigma_f", "refit")
            cv_block, cv_gap = GPR._cv_args(cv["block"], cv.get("gap", 0), cv_mode, max_window=L.CV_SMALL_MAX_WINDOW)
            for X, _, _, _ in self._data:
                GPR._cv_args(cv_block, cv_gap, cv_mode, max_window=L.CV_SMALL_MAX_WINDOW, n=X.shape[0])
        if self._uploaded != len(self._sets):
            self.upload()
        F = len(self._fits)
        if self._packed is None:
            arr = np.asarray(self._fits, dtype=np.float64)
            self._packed = (np.ascontiguousarray(arr[:, 0], dtype=np.int64), np.ascontiguousarray(arr[:, 1]), np.ascontiguousarray(arr[:, 2]))
        si, ell, sn = self._packed
        if hindcast is not None:
            flavour, extra = "hindcast", (hc_lead, hc_mt, L.LOO_MODES[hc_mode])
            if score_grad is not None:
                flavour, extra = "hindcast_grad", extra + (self._SCORE_IDS[score_grad],)
        elif cv is not None:
            flavour, extra = "cv", (cv_block, cv_gap, L.LOO_MODES[cv_mode])
            if cv_grad is not None:
                flavour, extra = "cv_grad", extra + (self._SCORE_IDS[cv_grad.get("score", "nlpd")],)
        elif loo is not None:
            flavour, extra = "loo", (L.LOO_MODES[loo],)
            if score_grad is not None:
                flavour, extra = "loo_grad", extra + (self._SCORE_IDS[score_grad],)
        else:
            flavour, extra = ("grad" if grad else "plain"), ()
        prefix, fn, what, width = self._FLAVOURS[flavour]
        ms = max(self._mmax, 1)
        out = np.zeros((F, width)); mean = np.full((F, ms), np.nan); var = np.full((F, ms), np.nan)
        args = extra + (L.ptr(out), L.ptr(mean), L.ptr(var), ms)
        if prefix:       # a prediction per training row
            nmax = max(s[1].shape[0] for s in self._sets)
            rmean = np.full((F, nmax), np.nan); rvar = np.full((F, nmax), np.nan)
            args += (L.ptr(rmean), L.ptr(rvar), nmax)
        gp = self.gp
        gp._check(getattr(gp._lib, fn)(gp._h, F, L.iptr(si), L.ptr(ell), L.ptr(sn), *args), what)
        gp._fitted = False
        res = dict(sigma_f=out[:, 0], nlml=out[:, 1], info=out[:, 2].astype(np.int64), sigma_n=out[:, 3],
                   mean=mean[:, :self._mmax], var=var[:, :self._mmax])
        if prefix:
            res.update({prefix + "_mean": rmean, prefix + "_var": rvar, prefix + "_nlpd": out[:, 4].copy(), prefix + "_sse": out[:, 5].copy()})
        if grad:
            res["grad_ref"], res["grad_exact"] = out[:, 4:6].copy(), out[:, 6:8].copy()
        if score_grad is not None or cv_grad is not None:
            res[prefix + "_grad"] = out[:, 6:8].copy()
        return res

    _SCORE_IDS = {"nlpd": 0, "sse": 1}       # SIGP_LOO_NLPD / SIGP_LOO_SSE

    # flavour -> (prefix of its result keys, entry point (its arguments beyond the common ones go ahead of ``out``), the name errors carry,
    # doubles per fit of ``out``)
    _FLAVOURS = {"plain": (None, "sigp_small_run", "small_run", 4),
                 "grad": (None, "sigp_small_run_grad", "small_run", 8),
                 "loo": ("loo", "sigp_small_run_loo", "small_run_loo", 6),
                 "cv": ("cv", "sigp_small_run_cv", "small_run_cv", 6),
                 "hindcast": ("hindcast", "sigp_small_run_hindcast", "small_run_hindcast", 6),
                 "loo_grad": ("loo", "sigp_small_run_loo_grad", "small_run_loo_grad", 8),
                 "hindcast_grad": ("hindcast", "sigp_small_run_hindcast_grad", "small_run_hindcast_grad", 8),
                 "cv_grad": ("cv", "sigp_small_run_cv_grad", "small_run_cv_grad", 8)}
