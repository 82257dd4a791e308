"""``GPR``: the fit / predict / nlml call sites that replace the reference's inline GP block
(north/June1st.py:231-277 and its 13 byte-identical siblings).

A script's block becomes::

    gp = GPR(kernel="netdiffusion")
    gp.fit(X, y, l_init[k], sigma_init[k], M=M, Xs=Xs)      # :264-271
    fmean, fvar = gp.predict(Xs)                            # :272-277  (fvar includes sigma_n)

All numerics run in HIP kernels behind libsigp.so (include/sigp.h).  There is no CPU fallback: without
the library or a GPU the constructor raises.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .features import SigmaEigh, laplacian_M, sigma_tilde


class LinAlgError(np.linalg.LinAlgError):
    """Raised where the reference's live block raises ``np.linalg.LinAlgError`` (non-SPD K~ at
    north/June1st.py:265); carries the LAPACK-style pivot index in ``.info``."""

    def __init__(self, msg, info=0):
        super().__init__(msg)
        self.info = info


# The validation-score families, one row each: the criteria and their ids, the normaliser of the family's own arguments (called as
# ``args(gp, values, sigma_f, n, d)`` with n, d of the staged data or None; it refuses a bad ``sigma_f``, fold or window and returns the
# values as the library takes them), the keywords those arguments go by, the library entries of the per-feature (ARD) call of one fit and
# of a lockstep group, and the wording of the refusals: ``criteria`` for a criterion of another family, ``elsewhere`` what the group entry
# adds to it, ``objective`` why ``<family>_objective`` refuses the reference kernel, ``optimize`` what ``optimize`` calls the family and
# the reference kernel's way to its scores.  A fourth family is a row here, its ``<family>_ard`` / ``_ard_batch`` / ``_objective`` /
# ``_objective_batch`` / ``optimize_<family>_batch`` methods (signature and docstring; the body is one call of ``_family_ard`` /
# ``_common_scale`` / ``_family_objective_batch`` / ``_optimize_family_batch``) and its own arguments in ``optimize`` / ``optimize_ard``.
_FAMILIES = {
    "loo": dict(ids=L.LOO_CRITERION_IDS, args=None, params=(), ard="sigp_loo_grad_ard", ard_batch="sigp_loo_grad_ard_batch",
                criteria="criterion must be 'loo_nlpd' or 'loo_sse'", elsewhere=" (the leave-block-out scores 'cv_nlpd' / 'cv_sse': cv_ard_batch)"),
    "cv": dict(ids=L.CV_CRITERION_IDS, args=lambda gp, a, sigma_f, n, d: gp._cv_args(*a, sigma_f, n=n), params=("block", "gap"),
               ard="sigp_cv_grad_ard", ard_batch="sigp_cv_grad_ard_batch",
               criteria="criterion must be 'cv_nlpd' or 'cv_sse'", elsewhere=" (the leave-one-out scores: loo_ard_batch)",
               objective="the reference kernel's leave-block-out scores have no gradient: cv_grid", optimize=("leave-block-out", "cv_grid")),
    "hindcast": dict(ids=L.HINDCAST_CRITERION_IDS, args=lambda gp, a, sigma_f, n, d: gp._hindcast_args(*a, sigma_f, n, d), params=("lead", "min_train"),
                     ard="sigp_hindcast_grad_ard", ard_batch="sigp_hindcast_grad_ard_batch",
                     criteria="criterion must be 'hindcast_nlpd' or 'hindcast_sse'",
                     elsewhere=" (the leave-one-out scores: loo_ard_batch, the leave-block-out scores: cv_ard_batch)",
                     objective="the reference kernel's hindcast scores have no gradient", optimize=("hindcast", "hindcast after fit")),
}
_ALL_CRITERIA = "criterion must be 'nlml', 'loo_nlpd', 'loo_sse', 'cv_nlpd', 'cv_sse', 'hindcast_nlpd' or 'hindcast_sse'"


def _family_of(criterion):
    """the name of the family ``criterion`` belongs to, None for 'nlml' and anything else"""
    return next((name for name, fam in _FAMILIES.items() if criterion in fam["ids"]), None)


def _check_sigma_f(sigma_f):
    if sigma_f not in L.LOO_MODES:
        raise ValueError("sigma_f must be 'refit' or 'fixed'")


def _check_grad(grad, allowed=(None, "exact"), message=None):
    if grad not in allowed:
        raise ValueError(message or "grad must be None%s or 'exact'" % (", 'ref'" if "ref" in allowed else ""))


def _finite_exp(theta):
    """theta [F, 2] = (log l, log sn~) -> (l [F], sn~ [F], which rows can be evaluated: both finite and l > 0)"""
    with np.errstate(over="ignore"):
        ell, sn = np.exp(theta[:, 0]), np.exp(theta[:, 1])
    return ell, sn, np.isfinite(ell) & np.isfinite(sn) & (ell > 0)


class GPR:
    def __init__(self, kernel="netdiffusion", dtype="f64", device=0, outer_blocks=None, lookahead=None, schedule=None,
                 panel_mode=None, expm="pade", accurate=None):
        if kernel not in L.KERNEL_IDS:
            raise ValueError("kernel must be one of %s" % sorted(L.KERNEL_IDS))
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        if dtype == "f32" and kernel == "netdiffusion":
            raise ValueError("the fp32 engine (fp32 factor + fp64 iterative refinement) covers the RBF / Matern kernels only")
        if expm not in ("pade", "eigh"):
            raise ValueError("expm must be 'pade' (scipy.linalg.expm per call, the reference's numbers) or 'eigh' (one eigendecomposition per data set)")
        self._expm = expm              # reference kernel only: how Sigma~ = expm(l M) is formed
        self._eig = None
        self.dtype = dtype
        self.kernel = kernel
        self._kid = L.KERNEL_IDS[kernel]
        self._lib = L.load()
        h = C.c_void_p()
        rc = self._lib.sigp_create(C.byref(h), int(device), 0 if dtype == "f64" else 1)
        if rc != L.OK:
            raise L.SigpError("sigp_create(device=%d) failed (rc=%d): no usable MI355X / HIP runtime [%s]; there is no CPU fallback"
                              % (device, rc, L.runtime_info()))
        self._h = h
        self.device = device
        self._has_data = False
        self._fitted = False
        self._ride = None
        self._ard = False              # per-feature length scales are set on the handle (sigp_set_length_scales)
        if outer_blocks is not None:
            self.set_option("outer_blocks", outer_blocks)
        if lookahead is not None:
            self.set_option("lookahead", int(bool(lookahead)))
        if schedule is not None:      # "right" | "left": outer schedule of the blocked Cholesky (same factor, bit for bit)
            self.set_option("schedule", {"right": 0, "left": 1}[schedule])
        if panel_mode is not None:    # "recursive" | "strips" | "auto": how the rows below a panel's top block are solved
            self.set_option("panel_mode", {"recursive": 0, "strips": 1, "auto": 2}[panel_mode])
        if accurate is not None:      # True: one residual-correction step behind every product with an inverted diagonal block (option accurate_solve)
            self.set_option("accurate_solve", int(bool(accurate)))

    # ---- plumbing ------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc == L.OK:
            return
        msg = self._lib.sigp_last_error(self._h)
        msg = msg.decode() if msg else ""
        if rc == L.NOT_SPD:
            raise LinAlgError("%s: %s" % (what, msg or "Matrix is not positive definite"))
        if rc == L.BAD_ARG:
            raise ValueError("%s: %s" % (what, msg))
        raise L.SigpError("%s: %s" % (what, msg))

    def _require_data(self, what):
        if not self._has_data:
            raise RuntimeError("%s: no data staged; call fit() or set_data() first" % what)

    def _require_ard_engine(self):
        if self.kernel == "netdiffusion" or self.dtype != "f64":
            raise ValueError("per-feature length scales: RBF / Matern kernels on the fp64 engine only")

    def _require_staged(self, what):
        """d of the data sets of the lockstep batch"""
        d = getattr(self, "_batch_d", None)
        if d is None:
            raise RuntimeError("%s: stage the data sets with upload_batch() first" % what)
        return d

    def _shape(self, batch=False):
        """(n, d) of the staged data set (``batch``: of the lockstep batch's data sets), (None, None) before any is staged"""
        if batch:
            return getattr(self, "_batch_n", None), getattr(self, "_batch_d", None)
        return (self.n, self.d) if getattr(self, "_has_data", False) else (None, None)

    def set_option(self, name, value):
        self._check(self._lib.sigp_set_option(self._h, name.encode(), int(value)), "set_option")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sigp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- data ----------------------------------------------------------------------------------
    def set_data(self, X, y, M=None, Xs=None):
        """Stage the enclosing-scope variables of the reference block (X, y, M, Xs) in HBM."""
        X = L.f64(X, 2)
        y = L.f64(np.asarray(y).reshape(-1), 1)
        if y.shape[0] != X.shape[0]:
            raise ValueError("X has %d rows but y has %d" % (X.shape[0], y.shape[0]))
        self._check(self._lib.sigp_set_train(self._h, L.ptr(X), X.shape[0], X.shape[1], X.shape[1], L.ptr(y)), "set_train")
        self.n, self.d = X.shape
        self._X, self._y = X, y
        self._ard = False              # sigp_set_train clears the scales
        self._M = None
        if self.kernel == "netdiffusion":
            self._M = laplacian_M(X) if M is None else L.f64(M, 2)
            if self._M.shape != (self.d, self.d):
                raise ValueError("M must be %dx%d" % (self.d, self.d))
            self._eig = SigmaEigh(self._M) if self._expm == "eigh" else None     # one eigh per data set
        self._set_ride(Xs)
        self._has_data = True
        self._fitted = False

    def _sigma(self, ell, with_derivative=False):
        """Sigma~ = expm(l M) (north/June1st.py:264) and, for the MLII gradient, M Sigma~ (:243-244 d Sigma/dl)."""
        if self._eig is not None:
            Sig = self._eig.sigma(ell)
            return (Sig, self._eig.msigma(ell)) if with_derivative else Sig
        Sig = sigma_tilde(self._M, ell)
        return (Sig, self._M @ Sig) if with_derivative else Sig

    def _set_ride(self, Xs):
        if Xs is None:
            self._ride = None
            self._check(self._lib.sigp_set_test(self._h, None, 0, 0), "set_test")
            return
        Xs = L.f64(np.atleast_2d(Xs), 2)
        if Xs.shape[1] != self.d:
            raise ValueError("Xs must have %d columns" % self.d)
        if Xs.shape[0] > (L.MAX_RIDE if self.dtype == "f64" else 3):
            self._ride = None      # too many to ride along: predict() takes the general path
            self._check(self._lib.sigp_set_test(self._h, None, 0, 0), "set_test")
            return
        self._check(self._lib.sigp_set_test(self._h, L.ptr(Xs), Xs.shape[0], Xs.shape[1]), "set_test")
        self._ride = Xs

    def _set_scales(self, ell):
        """``ell`` a sequence: per-feature length scales onto the handle, returns them as an array [d].  A scalar: clears any scales that
        are set (no library call otherwise: scalar fits issue the calls they always did), returns None."""
        if np.ndim(ell) == 0:
            if self._ard:
                self._check(self._lib.sigp_set_length_scales(self._h, None, 0), "set_length_scales")
                self._ard = False
            return None
        self._require_ard_engine()
        vec = L.f64(np.asarray(ell, dtype=np.float64), 1).copy()
        if vec.shape[0] != self.d:
            raise ValueError("ell must be a scalar or hold one length scale per feature (%d), got %d" % (self.d, vec.shape[0]))
        self._check(self._lib.sigp_set_length_scales(self._h, L.ptr(vec), vec.shape[0]), "set_length_scales")
        self._ard = True
        return vec

    # ---- fit (north/June1st.py:264-271) --------------------------------------------------------
    def fit(self, X, y, ell, sn_tilde, M=None, Xs=None):
        """Kernel build -> Cholesky -> A~ -> profiled sigma_f.  ``Xs`` (optional, <= 127 rows) rides along
        the factorisation so the following ``predict(Xs)`` costs nothing extra.  Raises LinAlgError
        if K~ is not positive definite, as the reference's live block does.

        ``ell``: a scalar, or a sequence of ``d`` per-feature (ARD) length scales (RBF / Matern, fp64): the library then divides
        feature k by ``ell[k]`` wherever it stages features (training rows, ``Xs``, the points of later ``predict`` / ``predict_cov`` /
        ``sample`` calls), so ``loo`` / ``cv`` and the predictions need no scaling by the caller; ``ell_`` becomes that array.  A scalar
        afterwards returns the handle to the isotropic kernel."""
        self.set_data(X, y, M=M, Xs=Xs)
        return self.refit(ell, sn_tilde)

    def refit(self, ell, sn_tilde):
        """Fit again on the staged data with new hyper-parameters (grid search / optimiser loop)."""
        self._require_data("refit")
        out = np.zeros(4)
        m = 0 if self._ride is None else self._ride.shape[0]
        mean = np.zeros(max(m, 1))
        var = np.zeros(max(m, 1))
        Sig = None
        ell_vec = self._set_scales(ell)
        if ell_vec is not None:
            ell = 1.0                  # the common multiplier
        if self.kernel == "netdiffusion":
            Sig = L.f64(self._sigma(float(ell)), 2)
            self._Sigma_tilde = Sig
        self._fitted = False
        rc = self._lib.sigp_fit_predict(self._h, self._kid, float(ell), float(sn_tilde), L.ptr(Sig),
                                        0 if Sig is None else Sig.shape[1], L.ptr(out), L.ptr(mean), L.ptr(var))
        self.info_ = int(out[2]) if rc in (L.OK, L.NOT_SPD) else -1
        if rc == L.NOT_SPD:
            raise LinAlgError("Matrix is not positive definite (pivot %d)" % self.info_, self.info_)
        self._check(rc, "fit")
        self.ell_, self.sn_tilde_ = (float(ell) if ell_vec is None else ell_vec), float(sn_tilde)
        self.sigma_f_, self.nlml_, self.sigma_n_ = float(out[0]), float(out[1]), float(out[3])
        self._ride_mean, self._ride_var = mean[:m].copy(), var[:m].copy()
        self._fitted = True
        return self

    # ---- predict (north/June1st.py:272-277) ----------------------------------------------------
    def predict(self, Xs, return_cov=False):
        """(fmean [m], fvar [m]); fvar is the variance of y*, i.e. includes sigma_n (:273, :277).
        ``return_cov=True``: (fmean [m], cov [m, m]) -- the joint covariance of y* at all test points (``predict_cov``), whose diagonal is fvar."""
        if return_cov:
            return self.predict_cov(Xs, noise=True)
        if not self._fitted:
            raise RuntimeError("predict: call fit() first")
        Xs = L.f64(np.atleast_2d(Xs), 2)
        if Xs.shape[1] != self.d:
            raise ValueError("Xs must have %d columns" % self.d)
        if self._ride is not None and Xs.shape == self._ride.shape and np.array_equal(Xs, self._ride):
            return self._ride_mean.copy(), self._ride_var.copy()
        m = Xs.shape[0]
        mean, var = np.zeros(m), np.zeros(m)
        self._check(self._lib.sigp_predict(self._h, L.ptr(Xs), m, Xs.shape[1], L.ptr(mean), L.ptr(var)), "predict")
        return mean, var

    # ---- inducing-point (sparse) regression for n past the dense limit ---------------------------------
    def sparse_fit(self, X, y, Z, ell, sn_tilde, jitter=1e-8, kind=None):
        """Inducing-point fit (DTC predictive, Titsias' collapsed bound; ``sigp_sparse_fit``) of ``y`` on ``X`` [n, d] with the inducing
        points ``Z`` [m, d] (``select_inducing``), m <= 8192 and n as large as host memory holds: X and y are streamed to the device in
        chunks (option ``sparse_chunk``), about 2 n m^2 flops.  ``ell``: a scalar or a sequence of d per-feature length scales;
        ``jitter`` is added to the diagonal of k(Z,Z); ``kind``: 'rbf' / 'matern52' (default: the engine's kernel).  Returns
        ``dict(sigma_f, nlml, bound, n, m)``: the profiled signal variance, the DTC negative log marginal likelihood and the collapsed
        variational bound (>= nlml).  Raises LinAlgError when k(Z,Z) + jitter I or sn~ I + V V^T is not positive definite.  Nothing of
        ``fit`` / ``set_data`` is involved: afterwards ``predict`` / ``loo`` / ... refuse as before any fit; ``sparse_predict`` predicts."""
        from .sparse import sparse_fit
        return sparse_fit(self, X, y, Z, ell, sn_tilde, jitter=jitter, kind=kind)

    def sparse_predict(self, Xs):
        """(mean [ms], var [ms]) at the rows of ``Xs`` from the last ``sparse_fit``; var includes the noise, as ``predict``'s."""
        from .sparse import sparse_predict
        return sparse_predict(self, Xs)

    # ---- joint posterior at new points -------------------------------------------------------------
    def predict_cov(self, Xs, noise=True):
        """(mean [m], cov [m, m]): the joint Gaussian posterior at the rows of ``Xs`` (``sigp_predict_cov``; 1 <= m <= 8192) from the factor on
        the device: cov = sigma_f (k~** + [noise] sn~ I - k~* K~^-1 k~*^T).  ``noise=True``: of the observations y* (diag(cov) is ``predict``'s
        fvar); ``noise=False``: of the latent function f*.  The mean is ``predict``'s, bit for bit; cov is exactly symmetric.  An error bar for
        any linear function w of the forecasts is w^T cov w.  fp64 engine only.  The fit stays as it is."""
        Xs = L.f64(np.atleast_2d(Xs), 2)
        d = getattr(self, "d", None)
        if d is not None and Xs.shape[1] != d:
            raise ValueError("Xs must have %d columns" % d)
        m = Xs.shape[0]
        if m < 1 or m > L.MAX_COV:
            raise ValueError("predict_cov: 1 <= m <= %d test points required (m = %d)" % (L.MAX_COV, m))
        mean, cov = np.zeros(m), np.zeros((m, m))
        self._check(self._lib.sigp_predict_cov(self._h, L.ptr(Xs), m, Xs.shape[1], int(bool(noise)), L.ptr(mean), L.ptr(cov), m), "predict_cov")
        return mean, cov

    def sample(self, Xs, size=1, noise=False, seed=None, z=None):
        """``size`` coherent draws [size, m] from the joint posterior at ``Xs``: mean + chol(cov) z with z [size, m] standard normals
        (``np.random.default_rng(seed)`` unless given).  The m x m factorisation runs on the host (``np.linalg.cholesky``).  A latent covariance
        (``noise=False``) can be singular to rounding (repeated or nearly repeated test points): jitter * max(diag) is then added to its
        diagonal, jitter = 1e-12, 1e-11, ... up to 1e-6, before LinAlgError is raised; the value used is left in ``sample_jitter_`` (0.0: none)."""
        mean, cov = self.predict_cov(Xs, noise=noise)
        m = mean.shape[0]
        if z is None:
            z = np.random.default_rng(seed).standard_normal((int(size), m))
        else:
            z = np.asarray(z, dtype=np.float64)
            if z.ndim != 2 or z.shape[1] != m:
                raise ValueError("z must be [size, %d]" % m)
        scale = float(np.max(np.diag(cov)))
        Lc = None
        for jitter in (0.0,) + (() if noise else tuple(10.0 ** e for e in range(-12, -5))):
            try:
                Lc = np.linalg.cholesky(cov + (jitter * scale) * np.eye(m) if jitter else cov)
                break
            except np.linalg.LinAlgError:
                pass
        if Lc is None:
            raise LinAlgError("sample: the %s covariance of the test points is not positive definite%s"
                              % ("predictive" if noise else "latent", "" if noise else " even with a relative jitter of 1e-6"))
        self.sample_jitter_ = jitter
        return mean + z @ Lc.T

    # ---- leave-one-out cross-validation ----------------------------------------------------------
    def loo(self, sigma_f="refit", grad=False):
        """Leave-one-out cross-validation of the current fit with (l, sn~) (and, for the reference kernel, M and the feature
        columns) held: what ``fit`` on the other n - 1 points followed by ``predict`` of the left-out point returns, for every
        point, from the factor already on the device (``sigp_loo``: L~^-T and one pass over it; about the price of a second fit).

        sigma_f='refit'  the signal variance is re-profiled without the left-out point (north/June1st.py:267-268 on n - 1 points):
                         identical to n real refits;
        sigma_f='fixed'  the full fit's sigma_f is kept (Rasmussen & Williams eq. 5.12).  The means do not depend on the mode.

        Returns dict(mean [n], var [n] (includes the noise, like fvar), nlpd, sse, mse, skill) with
        skill = 1 - sse / sum((y - mean(y))^2).  The fit stays as it is: ``predict`` afterwards works unchanged.

        ``grad=True`` (``sigp_loo_grad``) adds nlpd_grad [2] and sse_grad [2], the exact derivatives of the two scores with respect to
        (log l, log sn~); every other entry carries the same bits as without."""
        _check_sigma_f(sigma_f)
        if not self._fitted:
            raise RuntimeError("loo: call fit() first")
        mean, var, score = np.zeros(self.n), np.zeros(self.n), np.zeros(2)
        g4 = None
        if grad:
            MSig = None
            if self.kernel == "netdiffusion":
                MSig = L.f64(self._sigma(self.ell_, with_derivative=True)[1], 2)
            g4 = np.zeros(4)
            self._check(self._lib.sigp_loo_grad(self._h, L.LOO_MODES[sigma_f], L.ptr(MSig), 0 if MSig is None else MSig.shape[1], L.ptr(mean), L.ptr(var),
                                                L.ptr(score), L.ptr(g4)), "loo")
        else:
            self._check(self._lib.sigp_loo(self._h, L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), L.ptr(score)), "loo")
        nlpd, sse = float(score[0]), float(score[1])
        res = dict(mean=mean, var=var, nlpd=nlpd, sse=sse, mse=sse / self.n, skill=1.0 - sse / float(np.sum((self._y - self._y.mean()) ** 2)))
        if grad:
            res["nlpd_grad"], res["sse_grad"] = g4[:2].copy(), g4[2:].copy()
        return res

    def loo_batch(self, ell, sn_tilde, first=0, sigma_f="refit", group=8, predictions=True, grad=False):
        """``loo`` for many (data set, l, sn~) on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern), in
        lockstep groups of ``group`` fits (``sigp_loo_batch``): fit i uses data set (first + i) % B.  Returns dict(nlpd [F], sse [F])
        and, with ``predictions``, mean [F, n], var [F, n]; a non-SPD member gets +inf / NaN (north/June1st.py:254-256).
        ``grad=True`` (``sigp_loo_grad_batch``) adds nlpd_grad [F, 2] and sse_grad [F, 2] with respect to (log l, log sn~)."""
        _check_sigma_f(sigma_f)
        ell, sn, F, n, score, mean, var = self._batch_score_args("loo_batch", ell, sn_tilde, group, predictions)
        g4 = np.zeros((F, 4)) if grad else None
        if grad:
            self._check(self._lib.sigp_loo_grad_batch(self._h, int(first), F, self._kid, L.ptr(ell), L.ptr(sn), L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), n,
                                                      L.ptr(score), L.ptr(g4)), "loo_batch")
        else:
            self._check(self._lib.sigp_loo_batch(self._h, int(first), F, self._kid, L.ptr(ell), L.ptr(sn), L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), n,
                                                 L.ptr(score)), "loo_batch")
        return self._batch_score_result(score, mean, var, g4)

    def _batch_score_args(self, what, ell, sn_tilde, group, predictions):
        """what ``loo_batch`` and ``cv_batch`` do between their own checks and the library call: (ell [F], sn [F], F, n, score [F, 2], mean, var
        [F, n] or None), the lockstep group set"""
        if self.kernel == "netdiffusion":
            raise ValueError("%s covers the RBF / Matern kernels; the reference kernel's batch is SmallBatch.run(%s=...)" % (what, what[:-6]))
        ell = L.f64(np.atleast_1d(ell), 1)
        sn = L.f64(np.atleast_1d(sn_tilde), 1)
        F = len(ell)
        if len(sn) != F:
            raise ValueError("ell and sn_tilde must have the same length")
        self._require_staged(what)
        n = self._batch_n
        self.set_option("group", group)
        return ell, sn, F, n, np.zeros((F, 2)), (np.zeros((F, n)) if predictions else None), (np.zeros((F, n)) if predictions else None)

    def _batch_score_result(self, score, mean, var, g4=None):
        """... and after it: the result dict (the single fit, if any, is gone)"""
        self._fitted = False
        res = dict(nlpd=score[:, 0].copy(), sse=score[:, 1].copy())
        if g4 is not None:
            res["nlpd_grad"], res["sse_grad"] = g4[:, :2].copy(), g4[:, 2:].copy()
        if mean is not None:
            res["mean"], res["var"] = mean, var
        return res

    def loo_grid(self, X, y, ells, sns, sigma_f="refit", group=8, M=None):
        """The leave-one-out scores on the (l, sn~) grid for one data set, shaped like ``nlml_grid``: dict(nlpd, sse), each
        [len(ells), len(sns)], +inf where K~ is not SPD.  Reference kernel (n <= 128): one launch, one workgroup per grid point."""
        _check_sigma_f(sigma_f)
        return self._score_grid(X, y, ells, sns, group, M, "loo", sigma_f, lambda E, S: self.loo_batch(E, S, sigma_f=sigma_f, group=group, predictions=False))

    def _score_grid(self, X, y, ells, sns, group, M, prefix, small_arg, batch):
        """what ``loo_grid``, ``cv_grid`` and ``hindcast_grid`` do behind their own checks: the (l, sn~) mesh for one data set through
        ``SmallBatch.run(prefix=small_arg)`` (reference kernel) or ``upload_batch`` and ``batch(E, S)``; dict(nlpd, sse), each [len(ells), len(sns)]"""
        ells = np.asarray(ells, dtype=np.float64).reshape(-1)
        sns = np.asarray(sns, dtype=np.float64).reshape(-1)
        E, S = np.meshgrid(ells, sns, indexing="ij")
        if self.kernel == "netdiffusion":
            from .smallbatch import SmallBatch
            sb = SmallBatch(self)
            ds = sb.add_dataset(X, y, None, M)
            for e, s_ in zip(E.reshape(-1), S.reshape(-1)):
                sb.add_fit(ds, e, s_, expm=self._expm)
            r = sb.run(**{prefix: small_arg})
            nlpd, sse = r[prefix + "_nlpd"], r[prefix + "_sse"]
        else:
            self.upload_batch(L.f64(X, 2), y, None, group=group)
            r = batch(E.reshape(-1), S.reshape(-1))
            nlpd, sse = r["nlpd"], r["sse"]
        return dict(nlpd=nlpd.reshape(len(ells), len(sns)), sse=sse.reshape(len(ells), len(sns)))

    # ---- expanding-window hindcast validation ----------------------------------------------------
    def _hindcast_args(self, lead, min_train, sigma_f, n=None, d=None, max_lead=L.HINDCAST_MAX_LEAD):
        """the checks ``hindcast`` and its relatives share; ``min_train=None`` means max(2, d + 1).  Returns (lead, min_train)."""
        _check_sigma_f(sigma_f)
        lead = int(lead)
        if lead < 1 or lead > max_lead:
            raise ValueError("hindcast: 1 <= lead <= %d required" % max_lead)
        if min_train is None:
            min_train = 2 if d is None else max(2, d + 1)
        min_train = int(min_train)
        if min_train < 1:
            raise ValueError("hindcast: min_train >= 1 required")
        if n is not None and min_train + lead - 1 > n - 1:
            raise ValueError("hindcast: no row is scored (min_train + lead - 1 = %d > n - 1 = %d)" % (min_train + lead - 1, n - 1))
        return lead, min_train

    def hindcast(self, lead=1, min_train=None, sigma_f="refit"):
        """Expanding-window (rolling-origin) hindcast validation of the current fit with (l, sn~) (and, for the reference kernel, M and the
        feature columns) held: what the retrospective loop reports -- ``fit`` on rows [0, s) followed by ``predict`` of row t = s + lead - 1,
        for every t with s >= ``min_train`` -- read out of the factor already on the device (``sigp_hindcast``: the factor of a prefix is
        the leading block of L~; one pass over n row segments, no inverse).  Rows are taken in time order; ``lead`` - 1 rows between the
        training set and the target are withheld.  ``min_train=None`` means max(2, d + 1).

        sigma_f='refit'  the signal variance is profiled on the training rows [0, s) alone: identical to real refits on the prefixes;
        sigma_f='fixed'  the full fit's sigma_f is kept.  The means do not depend on the mode.

        Returns dict(mean [n], var [n] (with the noise, like fvar; NaN where a row is not scored), nlpd, sse, mse, skill over the scored
        rows, scored = slice(min_train + lead - 1, n)) with skill = 1 - sse / sum((y - mean(y))^2) over the scored rows.  The fit stays as
        it is: ``predict`` / ``loo`` / ``cv`` afterwards work unchanged."""
        if not self._fitted:
            _check_sigma_f(sigma_f)
            raise RuntimeError("hindcast: call fit() first")
        lead, min_train = self._hindcast_args(lead, min_train, sigma_f, self.n, self.d)
        mean, var, score = np.zeros(self.n), np.zeros(self.n), np.zeros(2)
        self._check(self._lib.sigp_hindcast(self._h, lead, min_train, L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), L.ptr(score)), "hindcast")
        return self._hindcast_result(mean, var, score, lead, min_train)

    def _hindcast_result(self, mean, var, score, lead, min_train):
        scored = slice(min_train + lead - 1, self.n)
        ys = self._y[scored]
        nlpd, sse = float(score[0]), float(score[1])
        return dict(mean=mean, var=var, nlpd=nlpd, sse=sse, mse=sse / len(ys), skill=1.0 - sse / float(np.sum((ys - ys.mean()) ** 2)) if len(ys) > 1 else np.nan,
                    scored=scored)

    def hindcast_batch(self, ell, sn_tilde, lead=1, min_train=None, first=0, sigma_f="refit", group=8, predictions=True):
        """``hindcast`` for many (data set, l, sn~) on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern), in lockstep
        groups of ``group`` fits (``sigp_hindcast_batch``): fit i uses data set (first + i) % B.  Returns dict(nlpd [F], sse [F]) and, with
        ``predictions``, mean [F, n], var [F, n] (NaN where a row is not scored); a non-SPD member gets +inf / NaN.  ``min_train=None``
        means max(2, d + 1) with d of the staged data sets, as in ``hindcast``."""
        if self.kernel == "netdiffusion":
            raise ValueError("hindcast_batch covers the RBF / Matern kernels; the reference kernel's batch is SmallBatch.run(hindcast=...)")
        lead, min_train = self._hindcast_args(lead, min_train, sigma_f, *self._shape(batch=True))
        ell, sn, F, n, score, mean, var = self._batch_score_args("hindcast_batch", ell, sn_tilde, group, predictions)
        self._check(self._lib.sigp_hindcast_batch(self._h, int(first), F, self._kid, L.ptr(ell), L.ptr(sn), lead, min_train, L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), n,
                                                  L.ptr(score)), "hindcast_batch")
        return self._batch_score_result(score, mean, var)

    def hindcast_grid(self, X, y, ells, sns, lead=1, min_train=None, sigma_f="refit", group=8, M=None):
        """The hindcast scores on the (l, sn~) grid for one data set, shaped like ``loo_grid``: dict(nlpd, sse), each [len(ells), len(sns)],
        +inf where K~ is not SPD.  Reference kernel (n <= 128, lead <= 32): one launch, one workgroup per grid point
        (``SmallBatch.run(hindcast=...)``).  ``min_train=None`` means max(2, d + 1), as in ``hindcast``."""
        Xa = np.asarray(X)
        lead, min_train = self._hindcast_args(lead, min_train, sigma_f, Xa.shape[0], Xa.shape[1])
        return self._score_grid(X, y, ells, sns, group, M, "hindcast", dict(lead=lead, min_train=min_train, sigma_f=sigma_f),
                                lambda E, S: self.hindcast_batch(E, S, lead=lead, min_train=min_train, sigma_f=sigma_f, group=group, predictions=False))

    # ---- leave-block-out cross-validation --------------------------------------------------------
    @staticmethod
    def cv_folds(n, block, gap=0):
        """The folds of ``cv``: an [F, 4] int array of (r0, r1, c0, c1) -- fold f scores the rows [c0, c1) = [f block, min(n, (f + 1) block))
        and removes the window [r0, r1) = [max(0, c0 - gap), min(n, c1 + gap)) from training."""
        c0 = np.arange(0, int(n), int(block), dtype=np.int64)
        c1 = np.minimum(c0 + int(block), int(n))
        return np.stack([np.maximum(c0 - int(gap), 0), np.minimum(c1 + int(gap), int(n)), c0, c1], axis=1)

    @staticmethod
    def _cv_args(block, gap, sigma_f, max_window=L.CV_MAX_WINDOW, n=None):
        _check_sigma_f(sigma_f)
        if int(block) != block or int(gap) != gap or block < 1 or gap < 0:
            raise ValueError("block >= 1 and gap >= 0 (integers) required")
        if block + 2 * gap > max_window:
            raise ValueError("the window block + 2 gap = %d exceeds %d rows" % (block + 2 * gap, max_window))
        if n is not None:
            f = GPR.cv_folds(n, block, gap)
            if n < 2 or np.any(n - (f[:, 1] - f[:, 0]) < 1):
                raise ValueError("every fold must leave a training row (n = %d, block = %d, gap = %d)" % (n, block, gap))
        return int(block), int(gap)

    def cv(self, block, gap=0, sigma_f="refit"):
        """Leave-block-out (K-fold, h-block, hv-block) cross-validation of the current fit with (l, sn~) (and, for the reference kernel, M and
        the feature columns) held -- for ordered rows such as consecutive years, where leaving ONE row out keeps its serially correlated
        neighbours in the training set and makes ``loo`` optimistic.  Fold f scores the rows [f block, (f + 1) block) and removes them, plus
        ``gap`` rows on each side (removed but not scored), from training: what ``fit`` on the remaining rows followed by ``predict`` of the scored
        rows returns, for every fold, from the factor already on the device (``sigp_cv``: L~^-T as ``loo``, then per fold the |S| x |S| block
        of K~^-1, its Cholesky factor and two short solves).  block + 2 gap <= 128, and every fold must leave a training row.  ``cv(1)`` is
        ``loo()``.  An arbitrary (shuffled) K-fold is the same call after the rows are permuted before ``fit``.

        sigma_f='refit'  the signal variance is re-profiled without the removed window (divisor n - |S_f| per fold): identical to real refits;
        sigma_f='fixed'  the full fit's sigma_f is kept.  The means do not depend on the mode.

        Returns dict(mean [n], var [n] (marginal, includes the noise, like fvar), nlpd, sse, mse, skill, folds [F, 4] = (r0, r1, c0, c1) as
        ``cv_folds``).  The fit stays as it is."""
        n = getattr(self, "n", None) if self._fitted else None
        block, gap = self._cv_args(block, gap, sigma_f, n=n)
        if self.dtype != "f64":
            raise ValueError("cv: fp64 engine only")
        if not self._fitted:
            raise RuntimeError("cv: call fit() first")
        mean, var, score = np.zeros(self.n), np.zeros(self.n), np.zeros(2)
        self._check(self._lib.sigp_cv(self._h, block, gap, L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), L.ptr(score)), "cv")
        nlpd, sse = float(score[0]), float(score[1])
        return dict(mean=mean, var=var, nlpd=nlpd, sse=sse, mse=sse / self.n, skill=1.0 - sse / float(np.sum((self._y - self._y.mean()) ** 2)),
                    folds=self.cv_folds(self.n, block, gap))

    def cv_batch(self, ell, sn_tilde, block, gap=0, first=0, sigma_f="refit", group=8, predictions=True):
        """``cv`` for many (data set, l, sn~) on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern), in lockstep groups
        of ``group`` fits (``sigp_cv_batch``): fit i uses data set (first + i) % B.  Returns dict(nlpd [F], sse [F]) and, with
        ``predictions``, mean [F, n], var [F, n]; a member whose K~ (or one of whose blocks of K~^-1) is not SPD gets +inf / NaN."""
        block, gap = self._cv_args(block, gap, sigma_f, n=self._shape(batch=True)[0])
        ell, sn, F, n, score, mean, var = self._batch_score_args("cv_batch", ell, sn_tilde, group, predictions)
        self._check(self._lib.sigp_cv_batch(self._h, int(first), F, self._kid, L.ptr(ell), L.ptr(sn), block, gap, L.LOO_MODES[sigma_f], L.ptr(mean), L.ptr(var), n,
                                            L.ptr(score)), "cv_batch")
        return self._batch_score_result(score, mean, var)

    def cv_grid(self, X, y, ells, sns, block, gap=0, sigma_f="refit", group=8, M=None):
        """The leave-block-out scores on the (l, sn~) grid for one data set, shaped like ``loo_grid``: dict(nlpd, sse), each
        [len(ells), len(sns)], +inf where K~ is not SPD.  Reference kernel (n <= 128, block + 2 gap <= 32): one launch, one workgroup per
        grid point (``SmallBatch.run(cv=...)``); the other kernels go through ``cv_batch``."""
        small = self.kernel == "netdiffusion"
        block, gap = self._cv_args(block, gap, sigma_f, max_window=L.CV_SMALL_MAX_WINDOW if small else L.CV_MAX_WINDOW, n=np.shape(X)[0])
        return self._score_grid(X, y, ells, sns, group, M, "cv", dict(block=block, gap=gap, sigma_f=sigma_f),
                                lambda E, S: self.cv_batch(E, S, block, gap=gap, sigma_f=sigma_f, group=group, predictions=False))

    # ---- MLII (north/June1st.py:235-257) -------------------------------------------------------
    def nlml(self, theta, grad="ref"):
        """``MLII(hyperparameters)``: theta = (log l, log sn~) -> (nlML, grad[2]).

        grad='ref'   the reference's own formulae (:248-252; NOT the derivative of nlML, SURVEY App. C-7;
                     defined for the reference kernel only),
        grad='exact' the analytic derivative of the profiled nlML (what an optimiser should be given),
        grad=None    value only (second entry None).
        A non-SPD K~ or an overflowing exp(theta) gives ``(inf, [inf, inf])`` like the reference's except
        branch (:254-256).  Everything O(n^3) runs on the device (K13/K14: tr(K~^-1 dK~) from a lockstep
        forward block solve of the identity + one SYRK)."""
        self._require_data("nlml")
        _check_grad(grad, (None, "ref", "exact"))
        if grad == "ref" and self.kernel != "netdiffusion":
            raise ValueError("grad='ref' is defined for the reference kernel only")
        theta = L.f64(np.asarray(theta, dtype=np.float64).reshape(2), 1)
        inf2 = (np.inf, np.asarray([np.inf, np.inf]))
        with np.errstate(over="ignore"):
            ell = float(np.exp(theta[0]))
        if not np.isfinite(ell) or not np.isfinite(np.exp(theta[1])):
            return inf2
        self._set_scales(ell)          # a scalar length scale: clears per-feature scales if any are set (no library call otherwise)
        Sig = MSig = None
        if self.kernel == "netdiffusion":
            try:
                with np.errstate(over="raise", invalid="raise"):
                    Sig, MSig = self._sigma(ell, with_derivative=True)
                    Sig, MSig = L.f64(Sig, 2), L.f64(MSig, 2)
            except (ValueError, OverflowError, FloatingPointError):
                return inf2
            if not (np.all(np.isfinite(Sig)) and np.all(np.isfinite(MSig))):
                return inf2
        mode = {None: 0, "ref": 1, "exact": 2}[grad]
        val = C.c_double()
        g = np.zeros(2)
        self._fitted = False
        rc = self._lib.sigp_nlml_grad(self._h, self._kid, L.ptr(theta), L.ptr(Sig), L.ptr(MSig),
                                      0 if Sig is None else Sig.shape[1], mode, C.byref(val), L.ptr(g))
        if rc == L.NOT_SPD:
            return inf2
        self._check(rc, "nlml")
        return np.float64(val.value), (None if grad is None else g)

    @staticmethod
    def _exp(theta):
        """exp of each entry by the C library's exp, which is what ``sigp_nlml_grad_ard`` applies to theta (NumPy's vectorised exp may differ
        in the last bit): a ``refit`` at these values repeats the fit the library made, bit for bit"""
        return np.array([math.exp(t) for t in np.asarray(theta, dtype=np.float64).reshape(-1)])

    def nlml_ard(self, theta, grad="exact"):
        """MLII with per-feature (ARD) length scales: theta = (log l_1 .. log l_d, log sn~) -> (nlML, grad [d + 1]) (``sigp_nlml_grad_ard``:
        every component of the exact gradient from one pass over K~^-1); ``grad=None``: value only (second entry None).  A non-SPD K~ or an
        overflowing exp(theta) gives ``(inf, [inf] * (d + 1))``, like ``nlml``.  Afterwards the handle is fitted at exp(theta) with the scales
        set: ``predict`` / ``predict_cov`` / ``loo`` / ``cv`` work on it, and ``nlml_`` is the value returned.  RBF / Matern, fp64."""
        r = self._ard_call("nlml_ard", theta, grad, None, False, lambda th, mean, var, score, g: self._lib.sigp_nlml_grad_ard(
            self._h, self._kid, L.ptr(th), th.shape[0], 0 if grad is None else 2, L.ptr(score), L.ptr(g)))
        return r["value"], (r["grad"] if r["spd"] else np.full(self.d + 1, np.inf))      # (the inf gradient even with grad=None)

    def _ard_call(self, what, theta, grad, which, predictions, call):
        """what ``nlml_ard``, ``loo_ard`` and ``cv_ard`` share, after the checks of their own: the checks they have in common, the buffers, the
        library call -- ``call(theta, mean, var, score, g)`` returns its code and leaves the two scores (``nlml_ard``: the nlML) in ``score``,
        of which ``which`` is the value (None: ``nlml_ard``) --, the non-SPD branch and the handle's state afterwards.  Returns dict(value, grad,
        mean, var, nlpd, sse, spd)."""
        self._require_data(what)
        _check_grad(grad)
        self._require_ard_engine()
        theta = L.f64(np.asarray(theta, dtype=np.float64).reshape(-1), 1)
        if theta.shape[0] != self.d + 1:
            raise ValueError("theta must hold d + 1 = %d entries (log l_1 .. log l_d, log sn~), got %d" % (self.d + 1, theta.shape[0]))
        score = np.zeros(2)
        g = np.zeros(self.d + 1) if grad is not None else None
        mean = np.zeros(self.n) if predictions else None
        var = np.zeros(self.n) if predictions else None
        self._fitted = False
        rc = call(theta, mean, var, score, g)
        spd = rc != L.NOT_SPD
        if spd:
            self._check(rc, what)
            self._after_ard_call(theta, float(score[0]) if which is None else None, what)
            value = np.float64(score[0 if which is None else which])
        else:
            self._ard = True           # (set unless exp(theta) itself was refused; a scalar refit then clears them, which is harmless)
            value, g = np.inf, (None if grad is None else np.full(self.d + 1, np.inf))
        return dict(value=value, grad=g, mean=mean, var=var, nlpd=float(score[0]), sse=float(score[1]), spd=spd)

    def _after_ard_call(self, theta, nlml, what):
        """the handle's state after a library call that fitted at exp(theta) with per-feature scales: the fit's scalars (its epilogue: the
        same bits) and the ride predictions"""
        self._ard = True
        sf, nl = C.c_double(), C.c_double()
        self._check(self._lib.sigp_fit(self._h, C.byref(sf), C.byref(nl)), what)
        self.ell_, self.sn_tilde_ = self._exp(theta[:-1]), float(self._exp(theta[-1:])[0])
        self.sigma_f_, self.nlml_, self.sigma_n_ = float(sf.value), float(nl.value if nlml is None else nlml), float(sf.value) * self.sn_tilde_
        m = 0 if self._ride is None else self._ride.shape[0]
        mean, var = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        if m:
            self._check(self._lib.sigp_predict_ride(self._h, L.ptr(mean), L.ptr(var)), what)
        self._ride_mean, self._ride_var = mean[:m].copy(), var[:m].copy()
        self._fitted = True

    def loo_ard(self, theta, criterion="loo_nlpd", sigma_f="refit", grad="exact", predictions=False):
        """A leave-one-out score with per-feature (ARD) length scales as an optimiser's objective: theta = (log l_1 .. log l_d, log sn~) ->
        (value, grad [d + 1]) with value = the leave-one-out negative log predictive density (``criterion='loo_nlpd'``) or sum of squared
        errors (``'loo_sse'``) of the fit at exp(theta) and its exact gradient (``sigp_loo_grad_ard``: one cubic product and one pass for all
        d components); ``grad=None``: value only (second entry None, no cubic work beyond ``loo``'s).  A non-SPD K~ or an overflowing
        exp(theta) gives ``(inf, [inf] * (d + 1))``, like ``nlml_ard``.  ``predictions=True`` returns dict(value, grad, mean [n], var [n], nlpd,
        sse) instead: the bits ``loo(sigma_f)`` returns on that fit.  Afterwards the handle is fitted at exp(theta) with the scales set, as
        after ``nlml_ard``.  RBF / Matern, fp64."""
        return self._family_ard("loo", theta, (), criterion, sigma_f, grad, predictions, sigma_f_first=True)

    def _family_ard(self, family, theta, args, criterion, sigma_f, grad, predictions, sigma_f_first=False, first=None, group=None):
        """``<family>_ard`` and, with ``first`` and ``group``, ``<family>_ard_batch`` behind their signatures: the refusals in the order each
        entry has them -- the criterion, ``sigma_f`` (ahead of ``grad`` only with ``sigma_f_first``; otherwise with the family's arguments),
        ``grad`` (here, not only in ``_ard_call``: a wrong ``grad`` is refused before missing data), the family's arguments ``args`` on the
        staged data -- and then the family's library entry through ``_ard_call`` / ``_ard_score_batch``."""
        fam, batch = _FAMILIES[family], first is not None
        if criterion not in fam["ids"]:
            raise ValueError(fam["criteria"] + (fam["elsewhere"] if batch else ""))
        if sigma_f_first:
            _check_sigma_f(sigma_f)
        _check_grad(grad)
        args = self._family_kw(family, args, sigma_f, *self._shape(batch)).values()
        cid, mode = fam["ids"][criterion], L.LOO_MODES[sigma_f]
        if batch:
            return self._ard_score_batch(family + "_ard_batch", theta, grad, group, predictions, cid, lambda th, F, d, n, mean, var, score, g: getattr(self._lib, fam["ard_batch"])(
                self._h, int(first), F, self._kid, L.ptr(th), d + 1, d + 1, *args, mode, cid, L.ptr(mean), L.ptr(var), n, L.ptr(score), L.ptr(g), d + 1))
        r = self._ard_call(family + "_ard", theta, grad, cid, predictions, lambda th, mean, var, score, g: getattr(self._lib, fam["ard"])(
            self._h, self._kid, L.ptr(th), th.shape[0], *args, mode, cid, L.ptr(mean), L.ptr(var), L.ptr(score), L.ptr(g)))
        del r["spd"]
        return r if predictions else (r["value"], r["grad"])

    def cv_ard(self, theta, block, gap=0, criterion="cv_nlpd", sigma_f="refit", grad="exact", predictions=False):
        """A leave-block-out score with per-feature (ARD) length scales as an optimiser's objective: theta = (log l_1 .. log l_d, log sn~) ->
        (value, grad [d + 1]) with value = the negative log predictive density (``criterion='cv_nlpd'``) or sum of squared errors
        (``'cv_sse'``) of ``cv(block, gap, sigma_f)`` on the fit at exp(theta), and its exact gradient (``sigp_cv_grad_ard``: the adjoint of
        ``loo_ard`` with a block in place of the diagonal -- one cubic product and one pass for all d components, whatever the folds);
        ``grad=None``: value only (second entry None, no work beyond ``cv``'s).  A non-SPD K~, an overflowing exp(theta) or a fold whose block
        of K~^-1 is not SPD gives ``(inf, [inf] * (d + 1))``.  ``predictions=True`` returns dict(value, grad, mean [n], var [n], nlpd, sse)
        instead: the bits ``cv(block, gap, sigma_f)`` returns on that fit.  Afterwards the handle is fitted at exp(theta) with the scales set,
        as after ``loo_ard``.  RBF / Matern, fp64; block + 2 gap <= 128 and every fold must leave a training row."""
        return self._family_ard("cv", theta, (block, gap), criterion, sigma_f, grad, predictions)

    def hindcast_ard(self, theta, lead=1, min_train=None, criterion="hindcast_nlpd", sigma_f="refit", grad="exact", predictions=False):
        """An expanding-window hindcast score with per-feature (ARD) length scales as an optimiser's objective: theta = (log l_1 .. log l_d,
        log sn~) -> (value, grad [d + 1]) with value = the negative log predictive density (``criterion='hindcast_nlpd'``) or sum of
        squared errors (``'hindcast_sse'``) of ``hindcast(lead, min_train, sigma_f)`` on the fit at exp(theta), and its exact gradient
        (``sigp_hindcast_grad_ard``: the reverse-mode adjoint of the Cholesky factorisation and one pass for all d components);
        ``grad=None``: value only (second entry None, no inverse and no cubic work).  A non-SPD K~ or an overflowing exp(theta) gives
        ``(inf, [inf] * (d + 1))``.  ``predictions=True`` returns dict(value, grad, mean [n], var [n], nlpd, sse) instead: the bits
        ``hindcast`` returns on that fit.  ``min_train=None`` means max(2, d + 1).  Afterwards the handle is fitted at exp(theta) with the
        scales set, as after ``loo_ard``.  RBF / Matern, fp64."""
        return self._family_ard("hindcast", theta, (lead, min_train), criterion, sigma_f, grad, predictions)

    def _family_kw(self, family, args, sigma_f, n, d):
        """the family's own arguments as the keywords its methods take them by, refused or normalised for data of shape (n, d) (None, None:
        nothing staged yet) by the family's normaliser -- which refuses a wrong ``sigma_f`` first"""
        fam = _FAMILIES[family]
        return dict(zip(fam["params"], fam["args"](self, args, sigma_f, n, d))) if fam["args"] else {}

    def _common_scale(self, family, theta, args, criterion, sigma_f, grad="exact"):
        """``<family>_ard`` over ONE common length scale: theta = (log l, log sn~) goes in as (log l x d, log sn~) and the gradient comes
        back as d/dlog l = sum_k d/dlog l_k (None with ``grad=None``).  Before any data is staged theta goes in as it is, for
        ``<family>_ard`` to refuse the call.  The reference kernel is refused first, in the words of ``<family>_objective``."""
        fam = _FAMILIES[family]
        if self.kernel == "netdiffusion":
            raise ValueError("%s_objective covers the RBF / Matern kernels (%s)" % (family, fam["objective"]))
        theta = np.asarray(theta, dtype=np.float64).reshape(2)
        if getattr(self, "_has_data", False):
            theta = np.concatenate([np.full(self.d, theta[0]), theta[1:]])
        v, g = getattr(self, family + "_ard")(theta, criterion=criterion, sigma_f=sigma_f, grad=grad, **dict(zip(fam["params"], args)))
        return v, (None if g is None else np.array([np.sum(g[:-1]), g[-1]]))

    def hindcast_objective(self, theta, lead=1, min_train=None, criterion="hindcast_nlpd", sigma_f="refit"):
        """A hindcast score as an optimiser's objective over ONE common length scale: theta = (log l, log sn~) -> (value, grad [2]).  It is
        ``hindcast_ard`` at equal scales with d/dlog l = sum_k d/dlog l_k, as ``cv_objective``.  RBF / Matern, fp64."""
        return self._common_scale("hindcast", theta, (lead, min_train), criterion, sigma_f)

    def cv_objective(self, theta, block, gap=0, criterion="cv_nlpd", sigma_f="refit"):
        """A leave-block-out score as an optimiser's objective over ONE common length scale: theta = (log l, log sn~) -> (value, grad [2])
        with value = the ``criterion`` ('cv_nlpd' | 'cv_sse') of ``cv(block, gap, sigma_f)`` on the fit at exp(theta).  It is ``cv_ard`` at equal
        scales with d/dlog l = sum_k d/dlog l_k.  A non-SPD K~ or an overflowing exp(theta) gives ``(inf, [inf, inf])``.  Afterwards the
        handle is fitted at exp(theta), the scales set to the common l.  RBF / Matern, fp64."""
        return self._common_scale("cv", theta, (block, gap), criterion, sigma_f)

    def optimize_ard(self, theta0, criterion="nlml", sigma_f="refit", method="L-BFGS-B", grad="exact", block=5, gap=0, lead=1, min_train=None, **kw):
        """Minimise ``criterion`` over one length scale per feature and the noise: 'nlml' (``nlml_ard``; what ``optimize(ard=True)`` does),
        'loo_nlpd' or 'loo_sse' (``loo_ard`` with ``sigma_f``), 'cv_nlpd' or 'cv_sse' (``cv_ard`` with ``block``, ``gap`` and ``sigma_f``),
        'hindcast_nlpd' or 'hindcast_sse' (``hindcast_ard`` with ``lead``, ``min_train`` and ``sigma_f``: the score the retrospective loop
        reports) -- with
        d + 1 hyper-parameters and few data the marginal likelihood overfits the relevance of features, and the predictive score is the honest
        objective; for ordered rows (consecutive years) the leave-block-out one, since ``loo`` keeps a row's correlated neighbours in the
        training set.  ``theta0`` = (log l_1 .. log l_d, log sn~), or (log l, log sn~)
        with log l broadcast to every feature; ``grad`` 'exact' or None (SciPy then differences the value).  ``bounds`` and the other keywords
        go to SciPy as they are.  Returns the scipy ``OptimizeResult``; afterwards the handle is fitted at ``exp(result.x)``."""
        family = _family_of(criterion)
        if criterion != "nlml" and family is None:
            raise ValueError(_ALL_CRITERIA)
        _check_sigma_f(sigma_f)
        _check_grad(grad, message="optimize_ard takes grad='exact' or None")
        if family is None:
            return self._minimize_ard("optimize_ard", lambda th: self.nlml_ard(th, grad=grad), theta0, method, grad, kw)
        own = self._family_kw(family, dict(loo=(), cv=(block, gap), hindcast=(lead, min_train))[family], sigma_f, *self._shape())
        if own:                        # (the leave-one-out scores leave the engine to ``loo_ard``, behind the staged data)
            self._require_ard_engine()
        return self._minimize_ard("optimize_ard", lambda th: getattr(self, family + "_ard")(th, criterion=criterion, sigma_f=sigma_f, grad=grad, **own), theta0, method, grad, kw)

    def _minimize_ard(self, what, objective, theta0, method, grad, kw):
        """``optimize_ard`` and ``optimize(ard=True)`` behind their own refusals: the staged data, ``theta0`` as d + 1 entries, the minimiser"""
        self._require_data(what)
        th0 = np.asarray(theta0, dtype=np.float64).reshape(-1)
        if th0.shape[0] == 2 and self.d != 1:
            th0 = np.concatenate([np.full(self.d, th0[0]), th0[1:]])
        if th0.shape[0] != self.d + 1:
            raise ValueError("theta0 must hold d + 1 = %d entries, or 2 (log l is broadcast)" % (self.d + 1))
        return self._minimize(objective, th0, method, grad, kw, ard=True)

    def _minimize(self, objective, th0, method, grad, kw, ard=False):
        """The tail of ``optimize`` and ``optimize_ard``: SciPy's ``minimize`` on ``objective(theta) -> (value, grad)`` (``grad=None``: on the
        value alone, SciPy differences it) and the refit at exp(result.x) -- by ``_exp`` for per-feature results, whose fits the library
        made at the C library's exp, by NumPy's for (log l, log sn~), as ``nlml`` and ``loo_objective`` form it: the two can differ in the
        last bit."""
        from scipy.optimize import minimize

        if grad is None:
            res = minimize(lambda th: float(objective(th)[0]), th0, method=method, jac=False, **kw)
        else:
            def fun(th):
                v, g = objective(th)
                return float(v), np.asarray(g, dtype=np.float64)

            res = minimize(fun, th0, method=method, jac=True, **kw)
        if np.all(np.isfinite(res.x)):
            try:
                if ard:
                    self.refit(self._exp(res.x[:-1]), float(self._exp(res.x[-1:])[0]))
                else:
                    self.refit(float(np.exp(res.x[0])), float(np.exp(res.x[1])))
            except LinAlgError:
                pass
        return res

    def loo_objective(self, theta, criterion="loo_nlpd", sigma_f="refit"):
        """A leave-one-out score as an optimiser's objective: theta = (log l, log sn~) -> (value, grad[2]) with value = the
        leave-one-out negative log predictive density (``criterion='loo_nlpd'``) or sum of squared errors (``'loo_sse'``) of the fit at
        exp(theta), and its exact gradient (``loo(grad=True)``).  A non-SPD K~ or an overflowing exp(theta) gives ``(inf, [inf, inf])``,
        like ``nlml``.  Afterwards the handle is fitted at exp(theta)."""
        if criterion not in L.LOO_CRITERIA:
            raise ValueError(_FAMILIES["loo"]["criteria"])
        _check_sigma_f(sigma_f)
        self._require_data("loo_objective")
        theta = np.asarray(theta, dtype=np.float64).reshape(2)
        inf2 = (np.inf, np.asarray([np.inf, np.inf]))
        with np.errstate(over="ignore"):
            ell, sn = float(np.exp(theta[0])), float(np.exp(theta[1]))
        if not (np.isfinite(ell) and np.isfinite(sn) and ell > 0):
            return inf2
        try:
            with np.errstate(over="raise", invalid="raise"):
                self.refit(ell, sn)
                r = self.loo(sigma_f, grad=True)
        except (LinAlgError, OverflowError, FloatingPointError):
            return inf2
        key = L.LOO_CRITERIA[criterion]
        if not (np.isfinite(r[key]) and np.all(np.isfinite(r[key + "_grad"]))):
            return inf2
        return np.float64(r[key]), r[key + "_grad"]

    def optimize(self, theta0, method="L-BFGS-B", grad="exact", criterion="nlml", sigma_f="refit", ard=False, block=5, gap=0, lead=1, min_train=None, **kw):
        """The reference's commented-out optimiser call (north/June1st.py:259-262:
        ``minimize(MLII, x0=[log l0, log sn0], method='CG', jac=True)``) against the device engine.
        ``grad='exact'`` (default) feeds the true derivative of the profiled nlML; ``grad='ref'`` reproduces the
        reference's MLII contract verbatim (its "gradient" is not the derivative, so CG stalls as in SURVEY App. C-7).
        ``criterion='loo_nlpd'`` / ``'loo_sse'`` minimises that leave-one-out score instead (``loo_objective`` with ``sigma_f``; grad
        'exact' or None); ``criterion='cv_nlpd'`` / ``'cv_sse'`` the leave-block-out score of ``cv(block, gap, sigma_f)`` (``cv_objective``;
        RBF / Matern); ``criterion='hindcast_nlpd'`` / ``'hindcast_sse'`` the expanding-window hindcast score of ``hindcast(lead, min_train,
        sigma_f)`` (``hindcast_objective``; RBF / Matern).  Returns the scipy ``OptimizeResult``; afterwards the handle is fitted at ``exp(result.x)``.
        ``ard=True``: one length scale per feature, by ``nlml_ard``'s exact gradient -- ``theta0`` = (log l_1 .. log l_d, log sn~), or
        (log l, log sn~) with log l broadcast to every feature; ``criterion`` must be 'nlml' here (``optimize_ard`` takes the others); the relevance of feature k is read from
        ``result.x[k]`` (a large log l_k: the feature does not matter).  ``bounds`` and the other keywords go to SciPy as they are."""
        if ard:
            if criterion != "nlml":
                raise ValueError("ard=True: criterion must be 'nlml' (optimize_ard minimises the leave-one-out, leave-block-out and hindcast scores -- loo_ard, cv_ard, hindcast_ard -- over per-feature scales)")
            _check_grad(grad, message="ard=True takes grad='exact' or None")
            return self._minimize_ard("optimize", lambda th: self.nlml_ard(th, grad=grad), theta0, method, grad, kw)
        family = _family_of(criterion)
        if family in ("cv", "hindcast"):
            fam, names = _FAMILIES[family], "criterion '%s_nlpd' / '%s_sse'" % (family, family)
            _check_grad(grad, message="a %s criterion takes grad='exact' or None" % fam["optimize"][0])
            if self.kernel == "netdiffusion":
                raise ValueError("%s covers the RBF / Matern kernels (the reference kernel: %s)" % (names, fam["optimize"][1]))
            if self.dtype != "f64":
                raise ValueError("%s: fp64 engine only" % names)
            own = self._family_kw(family, dict(cv=(block, gap), hindcast=(lead, min_train))[family], sigma_f, *self._shape())
            self._require_data("optimize")
            th0 = np.asarray(theta0, dtype=np.float64).reshape(2)
            if grad is None:
                objective = lambda th: self._common_scale(family, th, own.values(), criterion, sigma_f, grad=None)
            else:
                objective = lambda th: getattr(self, family + "_objective")(th, criterion=criterion, sigma_f=sigma_f, **own)
        elif criterion != "nlml":
            if family is None:
                raise ValueError(_ALL_CRITERIA)
            _check_grad(grad, message="a leave-one-out criterion takes grad='exact' or None")
            th0 = np.asarray(theta0, dtype=np.float64)
            objective = lambda th: self.loo_objective(th, criterion, sigma_f)
        else:
            th0 = np.asarray(theta0, dtype=np.float64)
            objective = lambda th: self.nlml(th, grad=grad)             # grad=None: value only, SciPy differences it numerically
        return self._minimize(objective, th0, method, grad, kw)

    # ---- state accessors -----------------------------------------------------------------------
    def _stat(self, name):
        v = C.c_double()
        self._check(self._lib.sigp_get_stat(self._h, name.encode(), C.byref(v)), "get_stat")
        return v.value

    @property
    def refine_residual_(self):
        """fp32 engine: max|y - K~ alpha~| / max|y| after the last fp64 refinement step of the last fit."""
        return self._stat("refine_residual")

    @property
    def matrix_bytes_(self):
        """Device bytes this handle holds in matrix / factor buffers."""
        return self._stat("matrix_bytes")

    @property
    def alpha_(self):
        """alpha = K^-1 y = A~/sigma_f (north/June1st.py:271), shape (n, 1)."""
        a = np.zeros(self.n)
        self._check(self._lib.sigp_get_alpha(self._h, L.ptr(a)), "get_alpha")
        return (a / self.sigma_f_).reshape(-1, 1)

    @property
    def L_tilde_(self):
        out = np.zeros((self.n, self.n))
        self._check(self._lib.sigp_get_matrix(self._h, 1, L.ptr(out), self.n), "get_matrix")
        return out

    @property
    def L_(self):
        """L = chol(K) = sqrt(sigma_f) L~ (north/June1st.py:270)."""
        return np.sqrt(self.sigma_f_) * self.L_tilde_

    def build(self, ell, sn_tilde):
        """K5 only: K~ (+ ride rows) into HBM; the factorisation is driven separately (potrf / DistributedGPR)."""
        if not self._has_data:
            raise RuntimeError("build: no data staged")
        if self.kernel == "netdiffusion":
            Sig = L.f64(self._sigma(float(ell)), 2)
            self._check(self._lib.sigp_kernel_build_from_sigma(self._h, L.ptr(Sig), Sig.shape[1], float(sn_tilde)), "kernel_build")
        else:
            ell_vec = self._set_scales(ell)        # a sequence: per-feature length scales (the build's own ell is then 1)
            self._check(self._lib.sigp_kernel_build(self._h, self._kid, 1.0 if ell_vec is not None else float(ell), float(sn_tilde)), "kernel_build")
            if ell_vec is not None:
                ell = ell_vec
        self.ell_, self.sn_tilde_ = (ell if np.ndim(ell) else float(ell)), float(sn_tilde)
        self._fitted = False

    def kernel_matrix(self, ell, sn_tilde):
        """K~ (lower triangle) as built on the device -- test/diagnostic accessor."""
        self.build(ell, sn_tilde)
        out = np.zeros((self.n, self.n))
        self._check(self._lib.sigp_get_matrix(self._h, 0, L.ptr(out), self.n), "get_matrix")
        self._fitted = False
        return out

    # ---- batches (retro loop :176-248, grid :210-211) ------------------------------------------
    def fit_batch(self, X, y, Xs, ell, sn_tilde, concurrency=2, group=8, M=None):
        """Independent fits.  X [B,n,d] (or [n,d] shared), y [B,n] (or [n]), Xs [B,m,d] (or [m,d] / None), ell [F],
        sn_tilde [F]; F fits, fit i uses data set i % B.
        Returns dict(sigma_f, nlml, info, sigma_n, mean [F,m], var [F,m]).

        RBF / Matern: lockstep groups on the blocked engine (data sets share (n, d, m)).  A 2-D ``ell`` [F, d] gives every FIT its own
        per-feature (ARD) length scales (``sigp_batch_run_ard``: the library divides the member's features and test points by them; the
        groups then run one after another, ``concurrency`` does not apply).
        Reference kernel: X / y / Xs may also be LISTS of arrays of different shapes (the retro years: n grows with the
        year); fits of order n <= 128 run one workgroup per fit in a single launch (``smallbatch.SmallBatch``), with
        Sigma~ = expm(l M) formed as this engine's ``expm`` option says; larger ones go one at a time through ``fit``."""
        if self.kernel == "netdiffusion":
            return self._fit_batch_netdiffusion(X, y, Xs, ell, sn_tilde, M)
        X = L.f64(X)
        shared = X.ndim == 2
        Xb = X[None] if shared else X
        B, n, d = Xb.shape
        yb = L.f64(np.asarray(y).reshape(B, n))
        m = 0
        Xsb = None
        if Xs is not None:
            Xsb = L.f64(Xs)
            Xsb = Xsb[None] if Xsb.ndim == 2 else Xsb
            if Xsb.shape[0] != B or Xsb.shape[2] != d:
                raise ValueError("Xs must be [B,m,d]")
            m = Xsb.shape[1]
        ell = self._batch_ell(ell, d)
        sn = L.f64(np.atleast_1d(sn_tilde), 1)
        F = len(ell)
        if len(sn) != F:
            raise ValueError("ell and sn_tilde must have the same length")
        self._check(self._lib.sigp_batch_upload(self._h, B, L.ptr(Xb), n * d, L.ptr(yb), n, L.ptr(Xsb), m * d, n, d, m), "batch_upload")
        self._batch_m, self._batch_n, self._batch_d, self._batch_B = m, n, d, B
        return self.run_batch(0, F, ell, sn, concurrency, group)

    @staticmethod
    def _batch_ell(ell, d):
        """ell [F] (one common length scale per fit) or [F, d] (per-feature scales per fit) as a contiguous array"""
        ell = L.f64(np.atleast_1d(ell))
        if ell.ndim == 2:
            if d is None:
                raise RuntimeError("run_batch: stage the data sets with fit_batch() / upload_batch() first")
            if ell.shape[1] != d:
                raise ValueError("a 2-D ell must be [F, d] = [F, %d] (one length scale per fit and feature), got %s" % (d, ell.shape))
        elif ell.ndim != 1:
            raise ValueError("ell must be [F] or [F, d]")
        return ell

    def predict_batch(self, X, y, Xs, ell, sn_tilde, **kw):
        """(mean [F, m], var [F, m]) of a batch of independent fits at their test points -- the per-(region, year) outputs
        ``fmean`` / ``fvar`` of the retro loop (September1st_retro.py:236-242).  The test points ride along each factorisation,
        so this IS ``fit_batch``; it exists for callers that only want the predictions."""
        r = self.fit_batch(X, y, Xs, ell, sn_tilde, **kw)
        if np.any(r["info"] != 0):
            bad = int(np.flatnonzero(r["info"])[0])
            raise LinAlgError("Matrix is not positive definite (fit %d, pivot %d)" % (bad, r["info"][bad]), int(r["info"][bad]))
        return r["mean"], r["var"]

    def _fit_batch_netdiffusion(self, X, y, Xs, ell, sn_tilde, M=None):
        from .smallbatch import SmallBatch, NMAX, MMAX
        if isinstance(X, np.ndarray) and X.ndim == 2:
            X, y, Xs, M = [X], [y], [Xs], [M]
        B = len(X)
        Xs = [None] * B if Xs is None else list(Xs)
        if M is not None and isinstance(M, np.ndarray) and M.ndim == 2 and B > 1:
            raise ValueError("M must be None or a sequence of %d Laplacians (one per data set), not a single array" % B)
        M = [None] * B if M is None else list(M)
        if len(M) != B or len(Xs) != B:
            raise ValueError("X, Xs and M must have one entry per data set (%d)" % B)
        ell = np.atleast_1d(np.asarray(ell, dtype=np.float64)); sn = np.atleast_1d(np.asarray(sn_tilde, dtype=np.float64))
        F = len(ell)
        if len(sn) != F:
            raise ValueError("ell and sn_tilde must have the same length")
        mmax = max([0] + [np.atleast_2d(x).shape[0] for x in Xs if x is not None])
        res = dict(sigma_f=np.zeros(F), nlml=np.zeros(F), info=np.zeros(F, np.int64), sigma_n=np.zeros(F),
                   mean=np.full((F, mmax), np.nan), var=np.full((F, mmax), np.nan))
        small = [i for i in range(F) if np.asarray(X[i % B]).shape[0] <= NMAX and (Xs[i % B] is None or np.atleast_2d(Xs[i % B]).shape[0] <= MMAX)]
        if small:
            sb = SmallBatch(self)
            ids = {}
            for i in small:
                b = i % B
                if b not in ids:
                    ids[b] = sb.add_dataset(X[b], y[b], Xs[b], M[b])
                sb.add_fit(ids[b], ell[i], sn[i], expm=self._expm)
            r = sb.run()
            for k in ("sigma_f", "nlml", "info", "sigma_n"):
                res[k][small] = r[k]
            res["mean"][small, :r["mean"].shape[1]] = r["mean"]
            res["var"][small, :r["var"].shape[1]] = r["var"]
        small_set = set(small)
        for i in range(F):                                                # orders beyond one workgroup: the blocked engine, one fit at a time
            if i in small_set:
                continue
            b = i % B
            try:
                self.fit(X[b], y[b], ell[i], sn[i], M=M[b], Xs=Xs[b])
                res["sigma_f"][i], res["nlml"][i], res["sigma_n"][i] = self.sigma_f_, self.nlml_, self.sigma_n_
                if Xs[b] is not None:
                    mu, var = self.predict(Xs[b])
                    res["mean"][i, :len(mu)], res["var"][i, :len(var)] = mu, var
            except LinAlgError as e:
                res["sigma_f"][i] = res["nlml"][i] = res["sigma_n"][i] = np.inf
                res["info"][i] = e.info
        self._fitted = False
        return res

    def upload_batch(self, X, y, Xs, group=8, concurrency=1, M=None):
        """Stage data sets in HBM and allocate the lockstep slots without running any fit (bench warm-up).
        Reference kernel: X / y / Xs / M are sequences of ragged data sets (n <= 128 rows each: the retro years), kept as a
        ``SmallBatch`` whose data stay resident for ``nlml_batch`` / ``optimize_batch``."""
        if self.kernel == "netdiffusion":
            from .smallbatch import SmallBatch
            if isinstance(X, np.ndarray) and X.ndim == 2:
                X, y, Xs, M = [X], [y], [Xs], [M]
            B = len(X)
            Xs = [None] * B if Xs is None else list(Xs)
            M = [None] * B if M is None else list(M)
            if len(y) != B or len(Xs) != B or len(M) != B:
                raise ValueError("X, y, Xs and M must have one entry per data set (%d)" % B)
            sb = SmallBatch(self)
            self._small_ids = [sb.add_dataset(X[b], y[b], Xs[b], M[b]) for b in range(B)]
            self._small = sb
            return
        X = L.f64(X)
        Xb = X[None] if X.ndim == 2 else X
        B, n, d = Xb.shape
        yb = L.f64(np.asarray(y).reshape(B, n))
        m, Xsb = 0, None
        if Xs is not None:
            Xsb = L.f64(Xs)
            Xsb = Xsb[None] if Xsb.ndim == 2 else Xsb
            m = Xsb.shape[1]
        self._check(self._lib.sigp_batch_upload(self._h, B, L.ptr(Xb), n * d, L.ptr(yb), n, L.ptr(Xsb), m * d, n, d, m), "batch_upload")
        self._batch_m, self._batch_n, self._batch_d, self._batch_B = m, n, d, B
        self._check(self._lib.sigp_batch_reserve(self._h, int(group), int(concurrency)), "batch_reserve")

    def run_batch(self, first, count, ell, sn_tilde, concurrency=2, group=8):
        """Run ``count`` fits on the data sets already resident in HBM (after fit_batch / upload).
        ``group`` fits are factorised in lockstep by each launch; ``concurrency`` groups are in flight.  ``ell`` [count, d]: per-feature
        length scales per fit (``sigp_batch_run_ard``; one group in flight)."""
        ell = self._batch_ell(ell, getattr(self, "_batch_d", None))
        self.set_option("group", group)
        sn = L.f64(np.atleast_1d(sn_tilde), 1)
        out = np.zeros((count, 4))
        if len(ell) != count or len(sn) != count:
            raise ValueError("ell and sn_tilde must have `count` entries")
        mdim = getattr(self, "_batch_m", 0)
        mean = np.zeros((count, max(mdim, 1)))
        var = np.zeros((count, max(mdim, 1)))
        if ell.ndim == 2:
            rc = self._lib.sigp_batch_run_ard(self._h, int(first), int(count), self._kid, L.ptr(ell), ell.shape[1], L.ptr(sn),
                                              L.ptr(out), L.ptr(mean) if mdim else None, L.ptr(var) if mdim else None)
        else:
            rc = self._lib.sigp_batch_run(self._h, int(first), int(count), self._kid, L.ptr(ell), L.ptr(sn), int(concurrency),
                                          L.ptr(out), L.ptr(mean) if mdim else None, L.ptr(var) if mdim else None)
        self._check(rc, "batch_run")
        self._fitted = False
        return dict(sigma_f=out[:, 0], nlml=out[:, 1], info=out[:, 2].astype(np.int64), sigma_n=out[:, 3],
                    mean=mean[:, :mdim], var=var[:, :mdim])

    def nlml_batch(self, theta, first=0, grad="exact", group=8, expm="eigh", sets=None):
        """``MLII`` for many (data set, theta) pairs in one device call on the data sets staged by ``upload_batch`` / ``fit_batch``:
        theta [F, 2] = (log l, log sn~), pair i uses data set (first + i) % B.  Returns (nlml [F], grad [F, 2] or None), +inf where K~
        is not SPD or exp(theta) overflows (north/June1st.py:254-256).  This is what an optimiser over all retrospective years
        evaluates per iteration (the reference's commented-out call, :259-262).

        RBF / Matern: lockstep groups on the blocked engine; grad = 'exact' (the derivative of the profiled nlML) or None.
        Reference kernel (n <= 128 per data set): one workgroup per pair, one launch (``sigp_small_run_grad``); grad = 'ref'
        reproduces the reference's own formulae (:248-252), 'exact' the true derivative.  ``expm`` = 'eigh' (default: one
        eigendecomposition of M per data set, nothing but theta crosses the bus per call) or 'pade' (scipy's expm per pair on
        the host, the reference's own numbers at extreme l); ``sets`` [F] names the data set of every pair explicitly."""
        theta = L.f64(np.atleast_2d(theta), 2)
        if theta.shape[1] != 2:
            raise ValueError("theta must be [F, 2]")
        F = theta.shape[0]
        if self.kernel == "netdiffusion":
            _check_grad(grad, (None, "ref", "exact"))
            val, g = self._small_run(self._small_staged("nlml_batch"), theta, first, sets, expm, "nlml", {None: None, "ref": "grad_ref", "exact": "grad_exact"}[grad],
                                     grad=grad is not None)
            return val, (g if grad is not None else None)
        _check_grad(grad)
        if sets is not None:
            raise ValueError("sets= is for the reference kernel's ragged data sets; the lockstep groups pair theta i with data set (first + i) % B")
        self.set_option("group", group)
        val = np.zeros(F)
        g = np.zeros((F, 2))
        self._check(self._lib.sigp_nlml_grad_batch(self._h, int(first), F, self._kid, L.ptr(theta), 0 if grad is None else 2, L.ptr(val),
                                                   L.ptr(g) if grad is not None else None), "nlml_batch")
        self._fitted = False
        return val, (g if grad is not None else None)

    def nlml_ard_batch(self, theta, first=0, grad="exact", group=8):
        """``nlml_ard`` for many fits in one device call on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern, fp64):
        theta [F, d + 1] = (log l_1 .. log l_d, log sn~) per FIT, fit i uses data set (first + i) % B -- two fits may share a data set and
        differ in scales (several starts per data set).  Lockstep groups of ``group`` fits (``sigp_nlml_grad_ard_batch``): per group one
        staging launch divides every member's features by its scales, then the fit, K~^-1 and ``nlml_ard``'s one-pass gradient for all
        members at once.  Returns (nlml [F], grad [F, d + 1] or None); a fit whose K~ is not SPD or whose exp(theta) overflows gets +inf in
        its value and all its gradient entries, its group mates are unaffected.  The gradient pass is ``nlml_ard``'s own code: where the lockstep factorisation has the single fit's bits
        (small orders), every fit carries the bits ``nlml_ard`` returns for it."""
        _check_grad(grad)
        self._require_ard_engine()
        d = self._require_staged("nlml_ard_batch")
        theta = L.f64(np.atleast_2d(theta), 2)
        if theta.shape[1] != d + 1:
            raise ValueError("theta must be [F, d + 1] = [F, %d] (log l_1 .. log l_d, log sn~), got %s" % (d + 1, theta.shape))
        F = theta.shape[0]
        self.set_option("group", group)
        val = np.zeros(F)
        g = np.zeros((F, d + 1)) if grad is not None else None
        self._check(self._lib.sigp_nlml_grad_ard_batch(self._h, int(first), F, self._kid, L.ptr(theta), d + 1, d + 1, 0 if grad is None else 2, L.ptr(val),
                                                       L.ptr(g), d + 1), "nlml_ard_batch")
        self._fitted = False
        return val, g

    def loo_ard_batch(self, theta, first=0, criterion="loo_nlpd", sigma_f="refit", grad="exact", group=8, predictions=False):
        """``loo_ard`` for many fits in one device call on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern, fp64):
        theta [F, d + 1] = (log l_1 .. log l_d, log sn~) per FIT, fit i uses data set (first + i) % B -- two fits may share a data set and
        differ in scales.  Lockstep groups of ``group`` fits (``sigp_loo_grad_ard_batch``): per group one staging launch, the fit and
        ``loo_batch``'s launches at ell = 1 on the staged features, then ``loo_ard``'s gradient for all members at once (one cubic product
        per member, one tile pass).  Returns (value [F], grad [F, d + 1] or None) with value = the leave-one-out negative log predictive
        density (``criterion='loo_nlpd'``) or sum of squared errors (``'loo_sse'``); ``grad=None``: values only, no cubic work beyond
        ``loo_batch``'s.  ``predictions=True`` returns dict(value, grad, mean [F, n], var [F, n], nlpd [F], sse [F]) instead.  A fit whose K~
        is not SPD or whose exp(theta) overflows gets +inf in its value, both scores and all its gradient entries and NaN predictions; its
        group mates are unaffected.  The gradient pass is ``loo_ard``'s own code: where the lockstep factorisation has the single fit's
        bits (small orders), every fit carries the bits ``loo_ard`` returns for it."""
        return self._family_ard("loo", theta, (), criterion, sigma_f, grad, predictions, sigma_f_first=True, first=first, group=group)

    def _ard_score_batch(self, what, theta, grad, group, predictions, cid, call):
        """What ``loo_ard_batch``, ``cv_ard_batch`` and ``hindcast_ard_batch`` share after their own checks: the kernel / engine, the staged data, theta's width -- all
        before any device call -- then the buffers, ``call(theta, F, d, n, mean, var, score, grad)`` and the result."""
        self._require_ard_engine()
        d, n = self._require_staged(what), self._batch_n
        theta = L.f64(np.atleast_2d(theta), 2)
        if theta.shape[1] != d + 1:
            raise ValueError("theta must be [F, d + 1] = [F, %d] (log l_1 .. log l_d, log sn~), got %s" % (d + 1, theta.shape))
        F = theta.shape[0]
        self.set_option("group", group)
        score = np.zeros((F, 2))
        g = np.zeros((F, d + 1)) if grad is not None else None
        mean = np.zeros((F, n)) if predictions else None
        var = np.zeros((F, n)) if predictions else None
        self._check(call(theta, F, d, n, mean, var, score, g), what)
        self._fitted = False
        value = score[:, cid].copy()
        if not predictions:
            return value, g
        return dict(value=value, grad=g, mean=mean, var=var, nlpd=score[:, 0].copy(), sse=score[:, 1].copy())

    def cv_ard_batch(self, theta, block, gap=0, first=0, criterion="cv_nlpd", sigma_f="refit", grad="exact", group=8, predictions=False):
        """``cv_ard`` for many fits in one device call on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern, fp64):
        theta [F, d + 1] = (log l_1 .. log l_d, log sn~) per FIT, fit i uses data set (first + i) % B -- two fits may share a data set and
        differ in scales.  Lockstep groups of ``group`` fits (``sigp_cv_grad_ard_batch``): per group one staging launch, the fit and
        ``cv_batch``'s launches at ell = 1 on the staged features with the fold adjoints of all (member, fold) pairs of a pass in one
        launch, then ``cv_ard``'s gradient for all members at once (the banded product, one cubic product per member, one tile pass).
        Returns (value [F], grad [F, d + 1] or None) with value = the leave-block-out negative log predictive density
        (``criterion='cv_nlpd'``) or sum of squared errors (``'cv_sse'``) of ``cv(block, gap, sigma_f)``; ``grad=None``: values only, no
        cubic work beyond ``cv_batch``'s.  ``predictions=True`` returns dict(value, grad, mean [F, n], var [F, n], nlpd [F], sse [F])
        instead.  A fit whose K~ (or one of whose folds' blocks of K~^-1) is not SPD or whose exp(theta) overflows gets +inf in its value,
        both scores and all its gradient entries and NaN predictions; its group mates are unaffected.  The folds' terms are added in
        ascending fold order however a group splits them into passes, and the gradient pass is ``cv_ard``'s own code: where the lockstep
        factorisation has the single fit's bits (small orders), every fit carries the bits ``cv_ard`` returns for it.
        block + 2 gap <= 128 and every fold must leave a training row."""
        return self._family_ard("cv", theta, (block, gap), criterion, sigma_f, grad, predictions, sigma_f_first=True, first=first, group=group)

    def _common_scale_batch(self, theta, evaluate, d=None):
        """An objective over ONE common length scale for theta [F, 2] = (log l, log sn~) per fit -> (value [F], grad [F, 2]) in one device
        call.  A fit whose exp(theta) is not finite rides along at harmless parameters; it, and any whose value or gradient is not finite,
        gets inf in its value and both gradient entries.  With ``d``: ``evaluate(theta [F, d + 1]) -> (value, grad [F, d + 1])`` is a
        per-feature objective, called at (log l x d, log sn~) and reduced by d/dlog l = sum_k d/dlog l_k, row by row as
        ``_common_scale`` adds them.  Without: ``evaluate(l [F], sn~ [F]) -> (value, grad [F, 2])``."""
        ell, sn, ok = _finite_exp(theta)
        if d is None:
            f, g = evaluate(np.where(ok, ell, 1.0), np.where(ok, sn, 1.0))
        else:
            f, g = evaluate(np.where(ok[:, None], np.concatenate([np.repeat(theta[:, :1], d, axis=1), theta[:, 1:]], axis=1), 0.0))
            f, g = np.array(f, dtype=np.float64), np.array([[np.sum(gi[:-1]), gi[-1]] for gi in g])
        ok &= np.isfinite(f) & np.all(np.isfinite(g), axis=1)
        f[~ok] = np.inf
        g[~ok] = np.inf
        return f, g

    def _family_objective_batch(self, family, theta, args, first, criterion, sigma_f, group):
        """``cv_objective_batch`` and ``hindcast_objective_batch`` behind their signatures: the refusals in their order, then
        ``<family>_ard_batch`` through ``_common_scale_batch``"""
        fam = _FAMILIES[family]
        if criterion not in fam["ids"]:
            raise ValueError(fam["criteria"])
        own = self._family_kw(family, args, sigma_f, *self._shape(batch=True))
        self._require_ard_engine()
        d = self._require_staged(family + "_objective_batch")
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if theta.ndim != 2 or theta.shape[1] != 2:
            raise ValueError("theta must be [F, 2] = (log l, log sn~) per fit, got %s" % (theta.shape,))
        return self._common_scale_batch(theta, lambda th: getattr(self, family + "_ard_batch")(th, first=first, criterion=criterion, sigma_f=sigma_f, grad="exact", group=group, **own), d)

    def cv_objective_batch(self, theta, block, gap=0, first=0, criterion="cv_nlpd", sigma_f="refit", group=8):
        """A leave-block-out score over ONE common length scale for many fits in one device call: theta [F, 2] = (log l, log sn~) per fit
        -> (value [F], grad [F, 2]).  It is ``cv_ard_batch`` at equal scales with d/dlog l = sum_k d/dlog l_k: per fit the bits
        ``cv_objective`` returns for it where ``cv_ard_batch`` carries ``cv_ard``'s.  A fit whose exp(theta) is not finite (it rides along at
        harmless parameters) or whose K~ is not SPD gets inf in its value and both gradient entries."""
        return self._family_objective_batch("cv", theta, (block, gap), first, criterion, sigma_f, group)

    def optimize_ard_batch(self, X, y, theta0, criterion="loo_nlpd", sigma_f="refit", group=8, maxiter=50, gtol=1e-5, ftol=1e-10, max_step=2.0):
        """``optimize_ard`` for EVERY data set of a retrospective run at once: X [B, n, d], y [B, n] -> dict(x [F, d + 1], fun [F], nit [F],
        converged [F], nfev = device calls), the lockstep BFGS of ``optimize_batch`` (``optim.bfgs_lockstep``) over one length scale per
        feature and the noise, each round ONE device call for all unfinished starts.  ``criterion`` 'loo_nlpd' or 'loo_sse' minimises that
        leave-one-out score (``loo_ard_batch`` with ``sigma_f``) -- with d + 1 hyper-parameters and few data the marginal likelihood overfits
        the relevance of features, and the predictive score is the honest objective; 'nlml' is ``optimize_batch(ard=True)``.  ``theta0`` is
        [F, d + 1], [d + 1], [F, 2] or [2] (the common log l is repeated for all d features); F = S B rows are S starts per data set, start
        i on data set i % B, and all F results come back.  RBF / Matern, fp64.  The leave-block-out scores in lockstep:
        ``optimize_cv_batch``."""
        if criterion != "nlml" and criterion not in L.LOO_CRITERION_IDS:
            raise ValueError("criterion must be 'nlml', 'loo_nlpd' or 'loo_sse' (the leave-block-out scores 'cv_nlpd' / 'cv_sse': optimize_cv_batch)")
        bfgs = dict(maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)
        if criterion == "nlml":
            _check_sigma_f(sigma_f)
            self._require_ard_engine()
            return self.optimize_batch(X, y, theta0, group=group, ard=True, **bfgs)
        return self._optimize_family_batch("loo", X, y, theta0, (), criterion, sigma_f, True, group, bfgs)

    def _optimize_family_batch(self, family, X, y, theta0, args, criterion, sigma_f, ard, group, bfgs):
        """``optimize_ard_batch``, ``optimize_cv_batch`` and ``optimize_hindcast_batch`` behind their refusal of another family's criterion:
        the remaining refusals (``sigma_f``, the engine, the family's arguments on X's shape, the starts -- all before the upload), the
        upload, and the lockstep BFGS on ``<family>_ard_batch`` (``ard``) or ``<family>_objective_batch``"""
        from .optim import bfgs_lockstep
        _check_sigma_f(sigma_f)
        self._require_ard_engine()
        X = L.f64(X, 3)
        B, n, d = X.shape
        own = self._family_kw(family, args, sigma_f, n, d)
        th0 = self._starts(theta0, B, d + 1, d) if ard else self._starts(theta0, B, 2)
        self.upload_batch(X, y, None, group=group, concurrency=1)
        objective = getattr(self, family + ("_ard_batch" if ard else "_objective_batch"))
        return bfgs_lockstep(lambda t: objective(t, criterion=criterion, sigma_f=sigma_f, group=group, **own), th0, **bfgs)

    @staticmethod
    def _starts(theta0, B, p, d=None, refuse=True):
        """theta0 -> the starts [F, p] of a lockstep run on B data sets: F = S B rows are S starts per data set (start i on data set
        i % B), anything else is broadcast to one start per data set.  With ``d`` (per-feature scales, p = d + 1) theta0 may be [F, 2] or
        [2] as well: the common log l is repeated for every feature.  ``refuse=False`` leaves a theta0 of another width to NumPy's
        ``broadcast_to`` (``optimize_batch`` over two parameters)."""
        th0 = np.atleast_2d(np.asarray(theta0, dtype=np.float64))
        if d is not None and th0.ndim == 2 and th0.shape[1] == 2 and d != 1:      # (log l, log sn~): the common log l for every feature
            th0 = np.concatenate([np.repeat(th0[:, :1], d, axis=1), th0[:, 1:]], axis=1)
        if refuse and (th0.ndim != 2 or th0.shape[1] != p):
            raise ValueError("theta0 must hold 2 entries per start (log l, log sn~) with ard=False" if d is None else
                             "theta0 must hold d + 1 = %d entries per start, or 2 (log l is repeated for every feature)" % p)
        if th0.ndim == 2 and th0.shape[0] != B and th0.shape[1] == p and th0.shape[0] % B == 0:
            return np.array(th0)                                  # S starts per data set: start i uses data set i % B
        return np.broadcast_to(th0[0] if th0.ndim == 2 and th0.shape[0] == 1 else th0, (B, p))

    @staticmethod
    def _ard_starts(theta0, B, d):
        """``_starts`` over per-feature scales: theta0 [F, d + 1], [d + 1], [F, 2] or [2] -> [F, d + 1]"""
        return GPR._starts(theta0, B, d + 1, d)

    def optimize_cv_batch(self, X, y, theta0, block, gap=0, criterion="cv_nlpd", sigma_f="refit", ard=True, group=8, maxiter=50, gtol=1e-5, ftol=1e-10,
                          max_step=2.0):
        """``optimize_ard(criterion='cv_*')`` for EVERY data set of a retrospective run at once: X [B, n, d], y [B, n] -> dict(x [F, d + 1],
        fun [F], nit [F], converged [F], nfev = device calls), the lockstep BFGS of ``optimize_batch`` (``optim.bfgs_lockstep``) on the
        leave-block-out score ``criterion`` ('cv_nlpd' | 'cv_sse') of ``cv(block, gap, sigma_f)`` -- the honest objective for ordered rows
        such as consecutive years, where ``loo`` keeps a year's serially correlated neighbours in the training set and the marginal
        likelihood overfits relevance at d + 1 hyper-parameters and a few dozen years.  Each round is ONE device call for all unfinished
        starts (``cv_ard_batch``).  ``block`` has no default: it depends on the data's correlation length.
        ``ard=True``: one length scale per feature and the noise; ``theta0`` is [F, d + 1], [d + 1], [F, 2] or [2] (the common log l is
        repeated for all d features), as ``optimize_ard_batch`` takes it; F = S B rows are S starts per data set, start i on data set
        i % B, and all F results come back.  ``ard=False``: one common length scale (``cv_objective_batch``), ``theta0`` [2] or [F, 2],
        x [F, 2].  RBF / Matern, fp64; block + 2 gap <= 128 and every fold must leave a training row."""
        if criterion not in L.CV_CRITERION_IDS:
            raise ValueError(_FAMILIES["cv"]["criteria"] + " (the leave-one-out scores and 'nlml': optimize_ard_batch)")
        return self._optimize_family_batch("cv", X, y, theta0, (block, gap), criterion, sigma_f, ard, group, dict(maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step))

    def hindcast_ard_batch(self, theta, lead=1, min_train=None, first=0, criterion="hindcast_nlpd", sigma_f="refit", grad="exact", group=8, predictions=False):
        """``hindcast_ard`` for many fits in one device call on the data sets staged by ``upload_batch`` / ``fit_batch`` (RBF / Matern, fp64):
        theta [F, d + 1] = (log l_1 .. log l_d, log sn~) per FIT, fit i uses data set (first + i) % B -- two fits may share a data set and
        differ in scales.  Lockstep groups of ``group`` fits (``sigp_hindcast_grad_ard_batch``): per group one staging launch, the fit and
        ``hindcast_batch``'s launches at ell = 1 on the staged features, then ``hindcast_ard``'s gradient for all members at once (the
        inverse factor, W = U C on a kernel that keeps the row in LDS, one cubic product per member, one tile pass).  Returns (value [F],
        grad [F, d + 1] or None) with value = the hindcast negative log predictive density (``criterion='hindcast_nlpd'``) or sum of squared
        errors (``'hindcast_sse'``) of ``hindcast(lead, min_train, sigma_f)``; ``grad=None``: values only, no inverse and no cubic work.
        ``predictions=True`` returns dict(value, grad, mean [F, n], var [F, n], nlpd [F], sse [F]) instead (NaN where a row is not scored).
        A fit whose K~ is not SPD or whose exp(theta) overflows gets +inf in its value, both scores and all its gradient entries and NaN
        predictions; its group mates are unaffected.  The gradient pass forms every number by ``hindcast_ard``'s own chain of operations:
        where the lockstep factorisation has the single fit's bits (small orders), every fit carries the bits ``hindcast_ard`` returns for
        it.  ``min_train=None`` means max(2, d + 1) with d of the staged data sets, as in ``hindcast_batch``."""
        return self._family_ard("hindcast", theta, (lead, min_train), criterion, sigma_f, grad, predictions, first=first, group=group)

    def hindcast_objective_batch(self, theta, lead=1, min_train=None, first=0, criterion="hindcast_nlpd", sigma_f="refit", group=8):
        """A hindcast score over ONE common length scale for many fits in one device call: theta [F, 2] = (log l, log sn~) per fit ->
        (value [F], grad [F, 2]).  It is ``hindcast_ard_batch`` at equal scales with d/dlog l = sum_k d/dlog l_k: per fit the bits
        ``hindcast_objective`` returns for it where ``hindcast_ard_batch`` carries ``hindcast_ard``'s.  A fit whose exp(theta) is not finite
        (it rides along at harmless parameters) or whose K~ is not SPD gets inf in its value and both gradient entries."""
        return self._family_objective_batch("hindcast", theta, (lead, min_train), first, criterion, sigma_f, group)

    def optimize_hindcast_batch(self, X, y, theta0, lead=1, min_train=None, criterion="hindcast_nlpd", sigma_f="refit", ard=True, group=8, maxiter=50, gtol=1e-5,
                                ftol=1e-10, max_step=2.0):
        """``optimize_ard(criterion='hindcast_*')`` for EVERY data set of a retrospective run at once: X [B, n, d], y [B, n] -> dict(x [F, d + 1],
        fun [F], nit [F], converged [F], nfev = device calls), the lockstep BFGS of ``optimize_batch`` (``optim.bfgs_lockstep``) on the
        expanding-window hindcast score ``criterion`` ('hindcast_nlpd' | 'hindcast_sse') of ``hindcast(lead, min_train, sigma_f)`` -- the
        score the retrospective loop reports.  Each round is ONE device call for all unfinished starts (``hindcast_ard_batch``).
        ``ard=True``: one length scale per feature and the noise; ``theta0`` is [F, d + 1], [d + 1], [F, 2] or [2] (the common log l is
        repeated for all d features), as ``optimize_cv_batch`` takes it; F = S B rows are S starts per data set, start i on data set
        i % B, and all F results come back.  ``ard=False``: one common length scale (``hindcast_objective_batch``), ``theta0`` [2] or
        [F, 2], x [F, 2].  ``min_train=None`` means max(2, d + 1).  RBF / Matern, fp64; lead <= 128 and at least one scored row."""
        if criterion not in L.HINDCAST_CRITERION_IDS:
            raise ValueError(_FAMILIES["hindcast"]["criteria"] + " (the leave-block-out scores: optimize_cv_batch; the leave-one-out scores and 'nlml': optimize_ard_batch)")
        return self._optimize_family_batch("hindcast", X, y, theta0, (lead, min_train), criterion, sigma_f, ard, group,
                                           dict(maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step))

    def _loo_objective_batch(self, theta, criterion, sigma_f, group):
        """(value [F], grad [F, 2]) of a leave-one-out score for theta [F, 2] on the staged data sets, one device call (``loo_batch``)."""
        key = L.LOO_CRITERIA[criterion]

        def scores(ell, sn):
            r = self.loo_batch(ell, sn, sigma_f=sigma_f, group=group, predictions=False, grad=True)
            return r[key].copy(), r[key + "_grad"].copy()
        return self._common_scale_batch(np.atleast_2d(np.asarray(theta, dtype=np.float64)), scores)

    def optimize_batch(self, X, y, theta0, group=8, maxiter=50, gtol=1e-5, ftol=1e-10, max_step=2.0, M=None, expm="eigh", method=None,
                       criterion="nlml", sigma_f="refit", ard=False):
        """The reference's commented-out ``minimize(MLII, x0, method='CG', jac=True)`` (north/June1st.py:259-262) for EVERY data set
        of a retrospective run at once: X [B, n, d], y [B, n], theta0 [B, 2] (or [2]) -> dict(x [B, 2], fun [B], nit [B],
        converged [B], nfev = device calls).  The state of every data set lives on the host and each round is ONE device call for all
        unfinished data sets: the years advance together whatever their individual line searches do (``optim.py``).

        RBF / Matern (``method='bfgs'``): BFGS on the 2-vector (log l, log sn~) per data set with Armijo backtracking, one trial point
        per data set and round in lockstep groups (``nlml_batch``).
        Reference kernel (``method='newton'``): X / y (/ M) are sequences of ragged data sets (the 3 regions x years of
        September1st_retro.py:176-180); a round is ONE launch of one workgroup per point, value + exact gradient formed in LDS, and since
        extra points are free there each round carries several step lengths and their finite-difference neighbours: a modified-Newton
        iteration with the line search inside the launch.

        Several starts per data set (RBF / Matern): ``theta0`` may have F = S B rows; start i uses data set i % B, the batch's own pairing,
        and all F results come back -- choosing the best start of a data set is the caller's job.
        ``ard=True`` (RBF / Matern, ``criterion='nlml'``): one length scale per feature, the same lockstep BFGS on ``nlml_ard_batch`` (d + 1
        parameters per start).  ``theta0`` is [F, d + 1], [d + 1], [F, 2] or [2]; with two entries the common log l is repeated for all d
        features.  Returns x [F, d + 1].  The leave-one-out scores over per-feature scales in lockstep: ``optimize_ard_batch``; the
        leave-block-out scores: ``optimize_cv_batch``."""
        from .optim import bfgs_lockstep, newton_lockstep
        if ard and criterion != "nlml":
            raise ValueError("optimize_batch(ard=True): criterion must be 'nlml' (optimize_ard_batch minimises the leave-one-out scores over per-feature "
                             "scales in lockstep, optimize_cv_batch the leave-block-out scores; optimize_ard either, one data set at a time)")
        if ard and self.kernel == "netdiffusion":
            raise ValueError("optimize_batch(ard=True): per-feature length scales cover the RBF / Matern kernels")
        if criterion != "nlml" and criterion not in L.LOO_CRITERIA:
            raise ValueError("criterion must be 'nlml', 'loo_nlpd' or 'loo_sse'")
        if criterion != "nlml" and self.kernel == "netdiffusion":
            raise ValueError("optimize_batch: the leave-one-out criteria cover the RBF / Matern kernels; the reference kernel's batch runs one workgroup per "
                             "fit and minimises the leave-one-out and hindcast scores through optimize_small_batch(criterion=...)")
        if self.kernel == "netdiffusion":
            self.upload_batch(X, y, None, M=M)
            B = len(self._small_ids)
            th0 = np.broadcast_to(np.asarray(theta0, dtype=np.float64), (B, 2))
            if (method or "newton") == "newton":
                return newton_lockstep(lambda t, own: self.nlml_batch(t, grad="exact", expm=expm, sets=own), th0, maxiter=maxiter, gtol=gtol,
                                       ftol=min(ftol, 1e-12), max_step=max_step)
            return bfgs_lockstep(lambda t: self.nlml_batch(t, grad="exact", expm=expm), th0, maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)
        if (method or "bfgs") != "bfgs":
            raise ValueError("method='newton' needs the one-workgroup-per-point kernel (reference kernel); RBF / Matern take 'bfgs'")
        X = L.f64(X, 3)
        B = X.shape[0]
        self.upload_batch(X, y, None, group=group, concurrency=1)
        if ard:
            th0 = self._starts(theta0, B, X.shape[2] + 1, X.shape[2])
            return bfgs_lockstep(lambda t: self.nlml_ard_batch(t, grad="exact", group=group), th0, maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)
        th0 = self._starts(theta0, B, 2, refuse=False)
        if criterion != "nlml":   # the same lockstep BFGS on a leave-one-out score: one sigp_loo_grad_batch call per round
            return bfgs_lockstep(lambda t: self._loo_objective_batch(t, criterion, sigma_f, group), th0, maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)
        return bfgs_lockstep(lambda t: self.nlml_batch(t, grad="exact", group=group), th0, maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)

    def small_score_batch(self, theta, criterion="hindcast_nlpd", lead=1, min_train=2, sigma_f="refit", first=0, expm="eigh", sets=None):
        """A leave-one-out or hindcast score of the reference kernel and its exact gradient for many (data set, theta) pairs in ONE launch, one
        workgroup per pair, on the data sets staged by ``upload_batch`` (``SmallBatch.run(loo= / hindcast=, score_grad=)``): theta [F, 2] =
        (log l, log sn~), pair i uses data set (first + i) % B or ``sets[i]``.  ``criterion`` 'loo_nlpd' | 'loo_sse' | 'hindcast_nlpd' |
        'hindcast_sse'; ``lead`` / ``min_train`` as ``SmallBatch.run(hindcast=)``; ``expm`` as ``nlml_batch``.  Returns (score [F], grad [F, 2]),
        +inf where K~ is not SPD or exp(theta) overflows.  The leave-block-out scores: ``small_cv_score_batch``."""
        if self.kernel != "netdiffusion":
            raise ValueError("small_score_batch runs the reference kernel (RBF / Matern: loo_ard_batch, hindcast_ard_batch)")
        if criterion not in L.LOO_CRITERION_IDS and criterion not in L.HINDCAST_CRITERION_IDS:
            raise ValueError("criterion must be 'loo_nlpd', 'loo_sse', 'hindcast_nlpd' or 'hindcast_sse' (block-CV gradients are not built for the reference kernel)")
        _check_sigma_f(sigma_f)
        sb = self._small_staged("small_score_batch")
        theta = L.f64(np.atleast_2d(theta), 2)
        if theta.shape[1] != 2:
            raise ValueError("theta must be [F, 2]")
        kind, key = criterion.split("_")
        run = dict(loo=sigma_f) if kind == "loo" else dict(hindcast=dict(lead=lead, min_train=min_train, sigma_f=sigma_f))
        val, g = self._small_run(sb, theta, first, sets, expm, criterion, kind + "_grad", score_grad=key, **run)
        g[~np.isfinite(val)] = np.inf
        return val, g

    def small_cv_score_batch(self, theta, block, gap=0, criterion="cv_nlpd", sigma_f="refit", first=0, expm="eigh", sets=None):
        """``small_score_batch`` for the leave-block-out scores of the reference kernel (``SmallBatch.run(cv_grad=)``): folds of ``block``
        consecutive rows with ``gap`` rows removed on each side, block + 2 gap <= 32, as ``SmallBatch.run(cv=)``; ``criterion`` 'cv_nlpd' |
        'cv_sse'.  Returns (score [F], grad [F, 2]) for theta [F, 2] = (log l, log sn~) in ONE launch, +inf where K~ or a fold's block of K~^-1
        is not SPD or exp(theta) overflows."""
        if self.kernel != "netdiffusion":
            raise ValueError("small_cv_score_batch runs the reference kernel (RBF / Matern: cv_ard_batch)")
        if criterion not in L.CV_CRITERION_IDS:
            raise ValueError("criterion must be 'cv_nlpd' or 'cv_sse' (the leave-one-out and hindcast scores: small_score_batch)")
        block, gap = self._cv_args(block, gap, sigma_f, max_window=L.CV_SMALL_MAX_WINDOW)
        sb = self._small_staged("small_cv_score_batch")
        theta = L.f64(np.atleast_2d(theta), 2)
        if theta.shape[1] != 2:
            raise ValueError("theta must be [F, 2]")
        val, g = self._small_run(sb, theta, first, sets, expm, criterion, "cv_grad", cv_grad=dict(block=block, gap=gap, sigma_f=sigma_f, score=criterion.split("_")[1]))
        g[~np.isfinite(val)] = np.inf
        return val, g

    def _small_staged(self, what):
        sb = getattr(self, "_small", None)
        if sb is None:
            raise RuntimeError("%s: stage the data sets with upload_batch(X_list, y_list, Xs_list, M=M_list) first" % what)
        return sb

    def _small_run(self, sb, theta, first, sets, expm, value, gradient, **run):
        """One launch of the one-workgroup kernel for theta [F, 2] on the staged ``SmallBatch``, pair i on data set (first + i) % B or
        ``sets[i]``: the pairs whose exp(theta) is finite and whose Sigma~ can be formed are queued (scipy's expm overflowing is the except
        branch of north/June1st.py:254-256), ``sb.run(**run)`` runs them, and its entries ``value`` [.] and ``gradient`` [., 2] (None: left
        out) come back scattered into (value [F], gradient [F, 2]), +inf for every pair that did not run."""
        F, B = theta.shape[0], len(self._small_ids)
        ell, sn, ok = _finite_exp(theta)
        val, g = np.full(F, np.inf), np.full((F, 2), np.inf)
        sb.clear_fits()
        ran = []
        for i in np.flatnonzero(ok):
            try:
                sb.add_fit(self._small_ids[(first + i) % B if sets is None else int(sets[i])], ell[i], sn[i], expm=expm)
                ran.append(i)
            except (FloatingPointError, OverflowError, ValueError):
                pass
        if ran:
            r = sb.run(**run)
            val[ran] = r[value]
            if gradient is not None:
                g[ran] = r[gradient]
        return val, g

    def optimize_small_batch(self, X, y, theta0, criterion="hindcast_nlpd", lead=1, min_train=2, sigma_f="refit", M=None, expm="eigh", maxiter=50,
                             gtol=1e-5, ftol=1e-10, max_step=2.0):
        """``optimize_batch`` for the reference kernel by a leave-one-out or hindcast score instead of nlML (``optimize_batch`` keeps refusing
        those criteria for this kernel): X / y (/ M) are sequences of ragged data sets (n <= 128 rows each), theta0 [B, 2] or [2] ->
        dict(x [B, 2], fun [B], jac [B, 2], nit [B], converged [B], nfev = launches).  Lockstep BFGS (``optim.bfgs_lockstep``) over
        ``small_score_batch``: each round is ONE launch, one workgroup per data set, score and exact gradient formed in LDS.  The leave-block-out
        scores: ``optimize_small_cv_batch``."""
        from .optim import bfgs_lockstep
        if self.kernel != "netdiffusion":
            raise ValueError("optimize_small_batch runs the reference kernel (RBF / Matern: optimize_batch, optimize_ard_batch, optimize_hindcast_batch)")
        if criterion not in L.LOO_CRITERION_IDS and criterion not in L.HINDCAST_CRITERION_IDS:
            raise ValueError("criterion must be 'loo_nlpd', 'loo_sse', 'hindcast_nlpd' or 'hindcast_sse' (block-CV gradients are not built for the reference kernel)")
        self.upload_batch(X, y, None, M=M)
        th0 = np.broadcast_to(np.asarray(theta0, dtype=np.float64), (len(self._small_ids), 2))
        return bfgs_lockstep(lambda t: self.small_score_batch(t, criterion=criterion, lead=lead, min_train=min_train, sigma_f=sigma_f, expm=expm), th0,
                             maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)

    def optimize_small_cv_batch(self, X, y, theta0, block, gap=0, criterion="cv_nlpd", sigma_f="refit", M=None, expm="eigh", maxiter=50, gtol=1e-5,
                                ftol=1e-10, max_step=2.0):
        """``optimize_small_batch`` by a leave-block-out score of the reference kernel ('cv_nlpd' | 'cv_sse'; folds as ``small_cv_score_batch``,
        ``block`` has no default, as in ``optimize_cv_batch``): lockstep BFGS (``optim.bfgs_lockstep``) over ``small_cv_score_batch``, each round
        ONE launch, one workgroup per data set, the score and its exact gradient formed in LDS.  Returns dict(x [B, 2], fun [B], jac [B, 2],
        nit [B], converged [B], nfev = launches)."""
        from .optim import bfgs_lockstep
        if self.kernel != "netdiffusion":
            raise ValueError("optimize_small_cv_batch runs the reference kernel (RBF / Matern: optimize_cv_batch)")
        if criterion not in L.CV_CRITERION_IDS:
            raise ValueError("criterion must be 'cv_nlpd' or 'cv_sse' (the leave-one-out and hindcast scores: optimize_small_batch)")
        block, gap = self._cv_args(block, gap, sigma_f, max_window=L.CV_SMALL_MAX_WINDOW)
        self.upload_batch(X, y, None, M=M)
        th0 = np.broadcast_to(np.asarray(theta0, dtype=np.float64), (len(self._small_ids), 2))
        return bfgs_lockstep(lambda t: self.small_cv_score_batch(t, block, gap=gap, criterion=criterion, sigma_f=sigma_f, expm=expm), th0, maxiter=maxiter,
                             gtol=gtol, ftol=ftol, max_step=max_step)

    def upload_small_ard(self, X, y, Xs=None):
        """Stage data sets of at most 128 rows for the one-workgroup kernel's RBF / Matern-5/2 flavours (``SmallStationaryBatch``): X / y / Xs
        are sequences of ragged data sets or arrays X [B, n, d], y [B, n], Xs [B, m, d] (m <= 8).  They stay resident for
        ``small_nlml_ard_batch`` / ``optimize_small_ard_batch``; what ``upload_batch`` staged for the blocked engine is untouched."""
        from .smallstationary import SmallStationaryBatch
        if isinstance(X, np.ndarray) and X.ndim == 2:
            X, y, Xs = [X], [y], None if Xs is None else [Xs]
        B = len(X)
        Xs = [None] * B if Xs is None else list(Xs)
        if len(y) != B or len(Xs) != B:
            raise ValueError("X, y and Xs must have one entry per data set (%d)" % B)
        sb = SmallStationaryBatch(self)
        self._small_k_ids = [sb.add_dataset(X[b], y[b], Xs[b]) for b in range(B)]
        self._small_k = sb
        sb.upload()

    def small_nlml_ard_batch(self, theta, first=0, grad="exact", sets=None):
        """``nlml_ard_batch`` at the application's own size: the profiled nlML and its exact gradient for many fits in ONE launch, one
        workgroup per fit (``sigp_small_run_k_grad``), on the data sets staged by ``upload_small_ard`` (RBF / Matern-5/2, fp64, n <= 128).
        theta [F, p]: row i is (log l_1 .. log l_N, log sn~) of its data set (p = N + 1, all sets named sharing N) or (log l, log sn~), one
        common scale (p = 2); fit i uses data set (first + i) % B or ``sets[i]`` -- several fits may share a data set (several starts).
        Returns (nlml [F], grad [F, p] or None); +inf in the value and every gradient entry where K~ is not SPD or exp(theta) is not a
        finite positive number with a finite reciprocal, the neighbours unaffected."""
        _check_grad(grad)
        sb = getattr(self, "_small_k", None)
        if sb is None:
            raise RuntimeError("small_nlml_ard_batch: stage the data sets with upload_small_ard(X_list, y_list) first")
        theta = L.f64(np.atleast_2d(theta), 2)
        F, p = theta.shape
        B = len(self._small_k_ids)
        ds = [self._small_k_ids[(first + i) % B if sets is None else int(sets[i])] for i in range(F)]
        Ns = {sb._data[d][0].shape[1] for d in ds}
        if p != 2 and (len(Ns) != 1 or p != next(iter(Ns)) + 1):
            raise ValueError("theta must be [F, N + 1] (log l_1 .. log l_N, log sn~) for data sets sharing N, or [F, 2] (log l, log sn~); got %s for N in %s"
                             % (theta.shape, sorted(Ns)))
        with np.errstate(over="ignore", divide="ignore"):
            e = np.exp(theta)
            ok = np.all(np.isfinite(e), axis=1) & np.all(e[:, :-1] > 0, axis=1) & np.all(np.isfinite(1.0 / e[:, :-1]), axis=1)
        val, g = np.full(F, np.inf), np.full((F, p), np.inf)
        sb.clear_fits()
        ran = np.flatnonzero(ok)
        for i in ran:
            sb.add_fit(ds[i], e[i, :-1], e[i, -1])
        if len(ran):
            r = sb.run(grad=grad is not None)
            val[ran] = r["nlml"]
            if grad is not None:
                g[ran, :-1] = r["grad_ell"][:, :p - 1]
                g[ran, -1] = r["grad_sn"]
                g[~np.isfinite(val)] = np.inf
        return val, (g if grad is not None else None)

    def optimize_small_ard_batch(self, X, y, theta0, ard=True, criterion="nlml", maxiter=50, gtol=1e-5, ftol=1e-10, max_step=2.0):
        """``optimize_batch(ard=True)`` at the application's own size: MLII over one length scale per feature (``ard=False``: one common
        scale) and the noise for EVERY data set at once, X / y sequences of data sets of n <= 128 rows sharing N features (or X [B, n, N],
        y [B, n]).  Lockstep BFGS (``optim.bfgs_lockstep``) over ``small_nlml_ard_batch``: each round is ONE launch, one workgroup per
        (data set, start), value and exact gradient formed in LDS.  ``theta0`` is [F, N + 1], [N + 1], [F, 2] or [2] (the common log l is
        repeated for every feature); F = S B rows are S starts per data set, start i on data set i % B, and all F results come back.
        Returns dict(x [F, N + 1] or [F, 2], fun [F], jac, nit [F], converged [F], nfev = launches).  RBF / Matern-5/2, fp64.  The
        validation scores have no gradient in the one-workgroup kernel for these covariances: the blocked engine minimises them
        (``optimize_ard_batch``, ``optimize_cv_batch``, ``optimize_hindcast_batch``)."""
        from .optim import bfgs_lockstep
        if criterion != "nlml":
            raise ValueError("optimize_small_ard_batch minimises 'nlml': the one-workgroup kernel has no score gradients for the RBF / Matern kernels "
                             "(the leave-one-out scores: optimize_ard_batch, the leave-block-out scores: optimize_cv_batch, the hindcast scores: optimize_hindcast_batch)")
        self._require_ard_engine()
        Xl = list(X)
        Ns = {np.shape(x)[-1] for x in Xl}
        if len(Ns) != 1:
            raise ValueError("optimize_small_ard_batch: all data sets share the number of features (got %s)" % sorted(Ns))
        N, B = next(iter(Ns)), len(Xl)
        th0 = self._starts(theta0, B, N + 1, N) if ard else self._starts(theta0, B, 2)
        self.upload_small_ard(Xl, list(y))
        return bfgs_lockstep(lambda t: self.small_nlml_ard_batch(t, grad="exact"), th0, maxiter=maxiter, gtol=gtol, ftol=ftol, max_step=max_step)

    def nlml_grid(self, X, y, ells, sns, concurrency=2, group=8, M=None):
        """nlML on the (l, sn~) grid for one data set -- the offline 20x20 search implied by
        north/June1st.py:210-211 (``ells = LGRID, sns = SGRID`` with the reference kernel reproduces it: one launch,
        one workgroup per grid point).  Returns [len(ells), len(sns)], +inf where K~ is not SPD."""
        ells = np.asarray(ells, dtype=np.float64).reshape(-1)
        sns = np.asarray(sns, dtype=np.float64).reshape(-1)
        E, S = np.meshgrid(ells, sns, indexing="ij")
        if self.kernel == "netdiffusion":
            r = self.fit_batch(X, y, None, E.reshape(-1), S.reshape(-1), M=M)
        else:
            r = self.fit_batch(X, y, None, E.reshape(-1), S.reshape(-1), concurrency=concurrency, group=group)
        return r["nlml"].reshape(len(ells), len(sns))

    # ---- the feature pipeline's correlation threshold on the device (networks.Network.tau(engine=gp)) --------------
    def corr_tau(self, series, dof, significance):
        """Cell-to-cell correlation matrix of ``series`` [N, T] and the mean of its significantly positive entries
        (behaviour of ComplexNetworks.py:31-47): returns (R [N, N] with a NaN diagonal, tau)."""
        from scipy import stats
        series = L.f64(series, 2)
        N, T = series.shape
        t_c = float(stats.t.isf(significance, dof))
        r_crit = t_c / np.sqrt(dof + t_c * t_c)
        R = np.empty((N, N))
        s, c = C.c_double(), C.c_double()
        self._check(self._lib.sigp_corr_tau(self._h, L.ptr(series), N, T, T, r_crit, L.ptr(R), N, C.byref(s), C.byref(c)), "corr_tau")
        with np.errstate(invalid="ignore", divide="ignore"):
            return R, np.float64(s.value) / np.float64(c.value)

    def area_sums(self, data, weight, label, nareas):
        """Per-area weighted sums of ``data`` [X, Y, T] (networks.Network.intra_links(engine=gp)): out [nareas, T]."""
        data = L.f64(data, 3)
        X, Y, T = data.shape
        w = L.f64(np.broadcast_to(weight, (X, Y)), 2)
        lab = np.ascontiguousarray(label, dtype=np.int32).reshape(X * Y)
        out = np.empty((int(nareas), T))
        self._check(self._lib.sigp_area_sums(self._h, L.ptr(data), X * Y, T, L.ptr(w), L.iptr(lab), int(nareas), L.ptr(out)), "area_sums")
        return out

    def detrend_cuts(self, data, cut_lens):
        """Per-pixel line removal of ``data`` [X, Y, T] over its first ``cut_lens[c]`` steps, every cut in one launch
        (callers.detrend(engine=gp)).  Returns ([dt [X, Y, n_c] ...], [trend [X, Y, 2] ...])."""
        data = L.f64(data, 3)
        X, Y, T = data.shape
        cuts = np.ascontiguousarray(cut_lens, dtype=np.int64)
        dt = np.empty(int(X * Y * cuts.sum()))
        tr = np.empty((len(cuts), X, Y, 2))
        self._check(self._lib.sigp_detrend(self._h, L.ptr(data), X * Y, T, len(cuts), L.iptr(cuts), L.ptr(dt), L.ptr(tr)), "detrend")
        outs, o = [], 0
        for n in cuts:
            outs.append(dt[o:o + X * Y * n].reshape(X, Y, int(n)))
            o += X * Y * int(n)
        return outs, [tr[c] for c in range(len(cuts))]

    # ---- measurement ---------------------------------------------------------------------------
    def profile(self, enable=True, classes=None):
        """Bracket kernel launches with HIP events (all classes, or only the named ones, e.g. ["syrk128"])."""
        code = int(bool(enable))
        if enable and classes:
            code = 0
            for c in classes:
                code |= 1 << (8 + L.KCLASS[c])
        self._check(self._lib.sigp_profile(self._h, code), "profile")

    def profile_reset(self):
        self._check(self._lib.sigp_profile_reset(self._h), "profile_reset")

    def synchronize(self):
        """Wait for everything the handle's device has been given (sigp_synchronize): the bracket of a timed region, on the
        HIP runtime the library itself links."""
        self._check(self._lib.sigp_synchronize(self._h), "synchronize")

    def profile_get(self):
        """{kernel class: dict(ms, launches, flops, bytes)} accumulated since the last reset."""
        out = {}
        for name, k in L.KCLASS.items():
            ms, fl, by = C.c_double(), C.c_double(), C.c_double()
            nl = C.c_int64()
            self._check(self._lib.sigp_profile_get(self._h, k, C.byref(ms), C.byref(nl), C.byref(fl), C.byref(by)), "profile_get")
            out[name] = dict(ms=ms.value, launches=nl.value, flops=fl.value, bytes=by.value)
        return out
