"""Quantum PCA (QADRA) on MI355X.

Reference: ``sklearn/decomposition/_qPCA.py`` class ``qPCA`` (:113-1316).
Classical core (exact Gram/SVD or randomized range finder) runs on the
device over row-sharded data; the quantum error model - consistent phase
estimation of the singular values (Theorem 9/10/11), amplitude estimation of
retained variance, tomography of singular vectors - is applied exactly as in
the reference using :mod:`sq_learn_amd.quantum`.

Quantum knobs are constructor parameters (sklearn convention, SURVEY.md
§5.6) and may also be passed to ``fit(**kw)`` like the reference.

Fixed reference defects (§2.8): ``left_sv`` holds the left singular
*vectors* (rows = U[:, i]; the reference sliced rows of U, :631);
``fit_transform`` works; ``condition_number_estimation`` implements the
intended routine (the reference passes invalid kwargs, :944-953);
``runtime_comparison`` returns the arrays (:1292-1315 returned None);
``estimate_theta`` logs instead of printing.
"""

import logging
import math
import zlib
import contextlib
import numbers
import os
import time
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from ...exceptions import ClassicalPathWarning
from ...quantum import reference as Q
from ...quantum.device import (gaussian_tomography, tomography_rows_torch, tomography_long,
                               consistent_phase_estimation_device)
from ...runtime.device import to_numpy, resolve_device
from ...runtime.rng import RngKey
from ...utils.extmath import stable_cumsum, _infer_dimension, fast_logdet
from ...utils.validation import check_is_fitted, seed_from_random_state
from ...quantum import cost_model
from .._data import as_data, global_mean_var, best_mu_distributed, best_mu_sparse
from ._base import _BasePCA, _as_out, _stays_sparse
from ._svd import full_svd, truncated_svd
from ...ops import linalg as L

log = logging.getLogger("sq_learn_amd.qpca")

_QKNOBS = ("quantum_retained_variance", "eps", "theta_major", "theta_minor", "eta",
           "theta_estimate", "use_computed_qcomponents", "eps_theta", "p", "estimate_all", "delta",
           "true_tomography", "fs_ratio_estimation", "norm", "stop_when_reached_accuracy",
           "incremental_measure", "faster_measure_increment", "check_sv_uniform_distribution",
           "spectral_norm_est", "condition_number_est", "estimate_least_k", "quantum_truncated")


class QPCA(_BasePCA):
    """Quantum-simulated PCA (sklearn estimator API)."""

    def __init__(self, n_components=None, *, copy=True, whiten=False, svd_solver="auto", tol=0.0,
                 iterated_power="auto", random_state=None, name=None,
                 quantum_retained_variance=False, eps=0, theta_major=0, theta_minor=0, eta=0,
                 theta_estimate=False, use_computed_qcomponents=False, eps_theta=0, p=0,
                 estimate_all=False, delta=0, true_tomography=True, fs_ratio_estimation=False,
                 norm="L2", stop_when_reached_accuracy=False, incremental_measure=False,
                 faster_measure_increment=0, check_sv_uniform_distribution=False,
                 spectral_norm_est=False, condition_number_est=False, estimate_least_k=False,
                 device=None, preserve_norm_tomography=False, quantum_truncated=False):
        self.n_components = n_components
        self.copy = copy
        self.whiten = whiten
        self.svd_solver = svd_solver
        self.tol = tol
        self.iterated_power = iterated_power
        self.random_state = random_state
        self.name = name
        self.quantum_retained_variance = quantum_retained_variance
        self.eps = eps
        self.theta_major = theta_major
        self.theta_minor = theta_minor
        self.eta = eta
        self.theta_estimate = theta_estimate
        self.use_computed_qcomponents = use_computed_qcomponents
        self.eps_theta = eps_theta
        self.p = p
        self.estimate_all = estimate_all
        self.delta = delta
        self.true_tomography = true_tomography
        self.fs_ratio_estimation = fs_ratio_estimation
        self.norm = norm
        self.stop_when_reached_accuracy = stop_when_reached_accuracy
        self.incremental_measure = incremental_measure
        self.faster_measure_increment = faster_measure_increment
        self.check_sv_uniform_distribution = check_sv_uniform_distribution
        self.spectral_norm_est = spectral_norm_est
        self.condition_number_est = condition_number_est
        self.estimate_least_k = estimate_least_k
        self.device = device
        self.preserve_norm_tomography = preserve_norm_tomography
        self.quantum_truncated = quantum_truncated

    # ------------------------------------------------------------ helpers
    def _rng(self, tag):
        seed = seed_from_random_state(self.random_state)
        self._rng_calls = getattr(self, "_rng_calls", 0) + 1
        return np.random.default_rng([seed & 0xFFFFFFFF, zlib.crc32(tag.encode()), self._rng_calls])

    def _key(self, purpose, sub=0):
        return RngKey(seed_from_random_state(self.random_state), purpose, sub)

    # ------------------------------------------------------ phase timings
    @contextlib.contextmanager
    def _phase(self, name):
        """Wall-clock of one fit phase into ``fit_phases_`` (seconds) when
        SQ_QPCA_PHASES=1 (device synchronised at both ends; off: no syncs)."""
        if os.environ.get("SQ_QPCA_PHASES", "0") != "1":
            yield
            return
        dev = getattr(self, "_device_type", "cpu")
        if dev == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            yield
        finally:
            if dev == "cuda":
                torch.cuda.synchronize()
            ph = self.__dict__.setdefault("fit_phases_", {})
            ph[name] = ph.get(name, 0.0) + time.perf_counter() - t0

    # ---------------------------------------------------------------- fit
    def fit(self, X, y=None, **quantum_kw):
        """Fit the model with X (``_qPCA.py:357-465``)."""
        for k in quantum_kw:
            if k not in _QKNOBS:
                raise TypeError(f"fit() got an unexpected keyword argument '{k}'")
        knobs = {k: getattr(self, k) for k in _QKNOBS}
        knobs.update(quantum_kw)
        if knobs["quantum_retained_variance"]:
            if knobs["eps"] <= 0:
                raise ValueError("eps must be > 0")
            if knobs["theta_major"] <= 0 and not knobs["theta_estimate"]:
                raise ValueError("theta must be > 0")
        if knobs["theta_estimate"]:
            if knobs["p"] <= 0 and not isinstance(self.n_components, int):
                raise ValueError("p must be > 0")
        self._fit(X, knobs)
        return self

    def _store_knobs(self, knobs):
        # fitted copies of the quantum knobs (reference stores them in _fit :493-514)
        self.delta_ = knobs["delta"]
        self.eps_ = knobs["eps"]
        self.eps_theta_ = knobs["eps_theta"]
        self.theta_major_ = knobs["theta_major"]
        self.theta_minor_ = knobs["theta_minor"]
        self.eta_ = knobs["eta"]
        self.ret_var = knobs["p"]
        self.tomography_norm = knobs["norm"]
        self._knobs = dict(knobs)

    def _fit(self, X, knobs):
        if _stays_sparse(X):
            return self._fit_sparse_rows(X, knobs)
        if sp.issparse(X):
            X = X.toarray()        # small: the fit of the same data as an array
        data = as_data(X, device=self.device, copy=self.copy)
        self._store_knobs(knobs)
        self.n_features_in_ = data.d
        n_samples, n_features = data.n_global, data.d
        if self.n_components is None:
            self.n_components_flag = False
            n_components = min(n_samples, n_features) if self.svd_solver != "arpack" \
                else min(n_samples, n_features) - 1
        else:
            self.n_components_flag = True
            n_components = self.n_components
        solver = self.svd_solver
        if solver == "auto":
            if max(n_samples, n_features) <= 500 or n_components == "mle":
                solver = "full"
            elif 1 <= n_components < 0.8 * min(n_samples, n_features):
                solver = "randomized"
            else:
                solver = "full"
        self._fit_svd_solver = solver
        self._source_kind = data.source_kind
        self._device_type = data.device.type
        self._comm = data.comm
        self._row_offset = data.row_offset
        if solver == "full":
            return self._fit_full(data, n_components)
        if solver in ("arpack", "randomized"):
            if not knobs.get("quantum_truncated"):
                warnings.warn("Attention! This computational path is purely classic!", ClassicalPathWarning)
            return self._fit_truncated(data, n_components, solver)
        raise ValueError(f"Unrecognized svd_solver='{solver}'")

    def _fit_full(self, data, n_components):
        n_samples, n_features = data.n_global, data.d
        if n_components == "mle":
            if n_samples < n_features:
                raise ValueError("n_components='mle' is only supported if n_samples >= n_features")
        elif not 0 <= n_components <= min(n_samples, n_features):
            raise ValueError(f"n_components={n_components!r} must be between 0 and "
                             f"min(n_samples, n_features)={min(n_samples, n_features)!r} with "
                             "svd_solver='full'")
        elif n_components >= 1 and not isinstance(n_components, numbers.Integral):
            raise ValueError(f"n_components={n_components!r} must be of type int when greater "
                             f"than or equal to 1, was of type={type(n_components)!r}")
        self.__dict__.pop("fit_phases_", None)
        self._device_type = data.device.type
        with self._phase("mean"):
            mean, _ = global_mean_var(data)
        self.mean_ = to_numpy(mean)
        k_left = min(n_samples, n_features)
        if isinstance(n_components, numbers.Integral) and self.n_components_flag:
            k_left = max(int(n_components), 1)
        with self._phase("svd"):
            res = full_svd(data, mean, k_left)
        S, Vt = res.S, res.Vt
        explained_variance_ = (S ** 2) / (n_samples - 1)
        total_var = explained_variance_.sum()
        explained_variance_ratio_ = explained_variance_ / total_var
        if n_components == "mle":
            n_components = _infer_dimension(explained_variance_, n_samples)
        elif 0 < n_components < 1.0:
            ratio_cumsum = stable_cumsum(explained_variance_ratio_)
            n_components = int(np.searchsorted(ratio_cumsum, n_components, side="right") + 1)
        if n_components < min(n_features, n_samples):
            self.noise_variance_ = float(explained_variance_[n_components:].mean())
        else:
            self.noise_variance_ = 0.0
        self.n_samples_, self.n_features_ = n_samples, n_features
        if isinstance(self.ret_var, numbers.Integral) and not isinstance(self.ret_var, bool):
            self.ret_var = float(np.sum(explained_variance_ratio_[:self.ret_var]))
        if not self.n_components_flag:
            n_components = self.ret_variance(explained_variance_ratio_, self.ret_var)
            self.components_retained_ = n_components
        n_components = int(n_components)
        self.components_ = Vt[:n_components]
        self.n_components_ = n_components
        self.all_components = Vt
        self.explained_variance_all = explained_variance_
        self.explained_variance_ratio_all = explained_variance_ratio_
        self.explained_variance_ = explained_variance_[:n_components]
        self.explained_variance_ratio_ = explained_variance_ratio_[:n_components]
        self.singular_values_ = S[:n_components].copy()
        U = res.U_local
        with self._phase("left_vectors"):
            if U is not None and U.shape[1] < n_components:
                U = self._left_vectors(data, mean, n_components)
        self.left_sv = _as_out(U[:, :n_components].T.contiguous(), data.source_kind) if U is not None else None
        self.spectral_norm = float(self.singular_values_[0]) if n_components else 0.0
        fro = torch.tensor([float((S ** 2).sum())], dtype=torch.float64)
        self.frob_norm = float(np.sqrt(fro.item()))
        # mu(A) of the centred matrix with the mean fused into the power-sum
        # pass (no centred copy of X)
        with self._phase("mu"):
            self.norm_muA, self.muA = best_mu_distributed(data, start=0, end=1.0, step=0.1,
                                                          fro_sq_global=float((S ** 2).sum()),
                                                          mean=mean)
        self._data_for_tomography = data
        self._quantum_extras()
        return self

    def _left_vectors(self, data, mean, k):
        dt = torch.float64 if data.device.type == "cpu" else torch.float32
        V = torch.as_tensor(self.all_components[:k].T, dtype=dt, device=data.device)
        S = torch.as_tensor(np.asarray(self.explained_variance_all[:k] * (data.n_global - 1)) ** 0.5,
                            dtype=dt, device=data.device)
        if data.device.type == "cpu":
            return ((data.X.to(dt) - mean.to(dt).to(data.device)) @ V) / S
        # (X - mean) V in one fp64-accumulated pass (csrc/tsgemm64.hip xw)
        X = data.X if data.X.stride(1) == 1 else data.X.contiguous()
        U = L.xw(X, V.double(), mean=mean, out_dtype=dt)
        return U / S

    def _fit_truncated(self, data, n_components, svd_solver):
        n_samples, n_features = data.n_global, data.d
        if isinstance(n_components, str):
            raise ValueError(f"n_components={n_components!r} cannot be a string with "
                             f"svd_solver='{svd_solver}'")
        if not 1 <= n_components <= min(n_samples, n_features):
            raise ValueError(f"n_components={n_components!r} must be between 1 and "
                             f"min(n_samples, n_features)={min(n_samples, n_features)!r} with "
                             f"svd_solver='{svd_solver}'")
        if not isinstance(n_components, numbers.Integral):
            raise ValueError(f"n_components={n_components!r} must be of type int when greater than "
                             f"or equal to 1, was of type={type(n_components)!r}")
        if svd_solver == "arpack" and n_components == min(n_samples, n_features):
            raise ValueError(f"n_components={n_components!r} must be strictly less than "
                             f"min(n_samples, n_features)={min(n_samples, n_features)!r} with "
                             f"svd_solver='{svd_solver}'")
        self.__dict__.pop("fit_phases_", None)
        self._device_type = data.device.type
        with self._phase("mean"):
            mean, var = global_mean_var(data)
        self.mean_ = to_numpy(mean)
        n_iter = self.iterated_power
        if svd_solver == "arpack":
            n_iter = max(7, n_iter if isinstance(n_iter, int) else 7)
        with self._phase("svd"):
            res = truncated_svd(data, mean, n_components, n_iter=n_iter,
                                seed=seed_from_random_state(self.random_state))
        S, Vt = res.S, res.Vt
        self.n_samples_, self.n_features_ = n_samples, n_features
        self.components_ = Vt
        self.left_sv = _as_out(res.U_local.T.contiguous(), data.source_kind)
        self.n_components_ = n_components
        self.explained_variance_ = (S ** 2) / (n_samples - 1)
        total_var = to_numpy(var) * n_samples / (n_samples - 1)
        self.explained_variance_ratio_ = self.explained_variance_ / total_var.sum()
        self.singular_values_ = S.copy()
        if self.n_components_ < min(n_features, n_samples):
            self.noise_variance_ = (total_var.sum() - self.explained_variance_.sum())
            self.noise_variance_ /= min(n_features, n_samples) - n_components
        else:
            self.noise_variance_ = 0.0
        self.spectral_norm = float(self.singular_values_[0])
        self.scaled_singular_values = self.singular_values_ / self.spectral_norm
        if self._knobs.get("quantum_truncated"):
            # framework extension (BASELINE config 2, "randomized_svd +
            # tomography noise"): the reference's truncated path is purely
            # classical (_qPCA.py:678-751); with quantum_truncated=True the
            # quantum model of _fit_full (mu(A), CPE singular values, Theorem
            # 9/10/11 extractors with tomography of the right AND the n-long
            # left singular vectors) runs on the randomized factors.
            self.frob_norm = float(np.sqrt(total_var.sum() * (n_samples - 1)))
            self.all_components = Vt
            self.explained_variance_all = self.explained_variance_
            self.explained_variance_ratio_all = self.explained_variance_ratio_
            with self._phase("mu"):
                self.norm_muA, self.muA = best_mu_distributed(data, start=0, end=1.0, step=0.1,
                                                              fro_sq_global=self.frob_norm ** 2,
                                                              mean=mean)
            self._quantum_extras()
        return self

    def _fit_sparse_rows(self, X, knobs):
        """``scipy.sparse`` rows above the densify limit (see ``PCA``): the
        truncated fit on the centred randomized SVD of the CSR rows; with
        ``quantum_truncated=True`` the quantum model runs unchanged on the
        dense factors, mu(A) of the centred matrix from its stored entries
        (``best_mu_sparse``, csrc/spmu.hip on the GPU)."""
        self._store_knobs(knobs)
        self.n_components_flag = self.n_components is not None
        self.__dict__.pop("fit_phases_", None)
        self._device_type = resolve_device(self.device).type
        with self._phase("svd"):
            sd, mean, total_var, U, S = self._fit_sparse(X, arpack_min_iter=7)
        self._source_kind = "numpy"
        self._comm = sd.comm
        self._row_offset = 0
        if not knobs.get("quantum_truncated"):
            warnings.warn("Attention! This computational path is purely classic!",
                          ClassicalPathWarning)
        n_samples = sd.shape[0]
        self.left_sv = to_numpy(U.T.contiguous())
        self.spectral_norm = float(self.singular_values_[0])
        self.scaled_singular_values = self.singular_values_ / self.spectral_norm
        if knobs.get("quantum_truncated"):
            self.frob_norm = float(np.sqrt(total_var.sum() * (n_samples - 1)))
            self.all_components = self.components_
            self.explained_variance_all = self.explained_variance_
            self.explained_variance_ratio_all = self.explained_variance_ratio_
            with self._phase("mu"):
                self.norm_muA, self.muA = best_mu_sparse(sd, mean, start=0, end=1.0, step=0.1,
                                                         fro_sq_global=self.frob_norm ** 2)
            self._quantum_extras()
        return self

    # ------------------------------------------------------- quantum extras
    def _quantum_extras(self):
        k = self._knobs
        if k["condition_number_est"]:
            with self._phase("cond_number"):
                self.est_cond_number = self.condition_number_estimation(epsilon=k["eps"],
                                                                        delta=k["delta"])
        if k["spectral_norm_est"]:
            with self._phase("spectral_norm"):
                self.est_spectral_norm = self.spectral_norm_estimation(epsilon=k["eps"],
                                                                       delta=k["delta"])
        if k["theta_estimate"]:
            with self._phase("theta"):
                self.est_theta = self.estimate_theta(epsilon=k["eps_theta"], eta=k["eta"],
                                                     p=self.ret_var)
        if k["quantum_retained_variance"]:
            # reference attribute ``p`` (estimated retained variance); the
            # constructor parameter p (target variance) is left untouched
            with self._phase("factor_score"):
                self.p_ = self.quantum_factor_score_ratio_sum(eps=k["eps"], theta=k["theta_major"],
                                                              eta=k["eta"])
        tkw = dict(true_tomography=k["true_tomography"], norm=k["norm"],
                   stop_when_reached_accuracy=k["stop_when_reached_accuracy"],
                   incremental_measure=k["incremental_measure"],
                   faster_measure_increment=k["faster_measure_increment"],
                   check_sv_uniform_distribution=k["check_sv_uniform_distribution"])
        if k["estimate_least_k"]:
            (self.estimate_least_right_sv, self.estimate_least_left_sv, self.estimate_least_s_values,
             self.estimate_least_fs, self.estimate_least_fs_ratio) = self.least_k_sv_extractors(
                X=None, delta=k["delta"], eps=k["eps"], theta=k["theta_minor"], **tkw)
        if k["estimate_all"]:
            (self.estimate_right_sv, self.estimate_left_sv, self.estimate_s_values, self.estimate_fs,
             self.estimate_fs_ratio) = self.topk_sv_extractors(
                X=None, delta=k["delta"], eps=k["eps"], theta=k["theta_major"], **tkw)

    def _cpe_sv(self, sv_scaled, eps_pe, scale_denom, unwrap_eps, gamma):
        """CPE of wrapped singular values (vectorised): theta_i = 2 acos(sv_i)
        / scale_denom, CPE(theta_i, eps_pe, gamma), unwrapped with unwrap_eps."""
        sv = np.clip(np.asarray(sv_scaled, dtype=np.float64), -1.0, 1.0)
        theta = 2 * np.arccos(sv) / scale_denom
        if getattr(self, "_device_type", "cpu") == "cuda":
            # pe_batch_kernel draws; every rank draws the same values (same key)
            self._cpe_calls = getattr(self, "_cpe_calls", 0) + 1
            t = torch.as_tensor(theta, dtype=torch.float64, device="cuda")
            est = consistent_phase_estimation_device(t, eps_pe, gamma,
                                                     self._key("pe", self._cpe_calls)).cpu().numpy()
        else:
            est = Q.consistent_phase_estimation_batch(theta, eps_pe, gamma,
                                                      random_state=self._rng("cpe"))
        return np.cos(est * (unwrap_eps + np.pi) / 2)

    def spectral_norm_estimation(self, epsilon, delta):
        """Binary search for ||A|| (``_qPCA.py:882-907``)."""
        l, u = 0.0, 1.0
        n_it = int(np.ceil(np.log(self.frob_norm / epsilon)))
        tau = (l + u) / 2
        gamma = 1 - 1 / self.n_features_
        rng = self._rng("ae")
        for _ in range(n_it):
            est = self._cpe_sv(self.singular_values_ / self.frob_norm, epsilon / self.frob_norm,
                               (1 / epsilon) + np.pi, 1 / epsilon, gamma)
            sel = self.singular_values_[est >= tau]
            eta = float(np.sum(sel ** 2) / self.frob_norm ** 2)
            eta_est = Q.amplitude_estimation(a=min(eta, 1.0), epsilon=delta, random_state=rng)
            if eta_est == 0:
                u = tau
            else:
                l = tau
            tau = (u + l) / 2
        return tau * self.frob_norm

    def condition_number_estimation(self, epsilon, delta):
        """Intended routine of ``_qPCA.py:909-961`` (the reference raises
        TypeError on invalid kwargs): binary search on the smallest retained
        singular values; returns tau * ||A||_F and sets ``est_sing_min``."""
        l, u = 0.0, 1.0
        n_it = int(np.ceil(np.log(self.frob_norm / epsilon)))
        tau = (l + u) / 2
        gamma = 1 - 1 / self.n_features_
        rng = self._rng("ae")
        for _ in range(n_it):
            est = self._cpe_sv(self.singular_values_ / self.frob_norm, epsilon / self.frob_norm,
                               (1 / epsilon) + np.pi, 1 / epsilon, gamma)
            sel = self.singular_values_[est <= tau]
            eta = min(float(np.sum(sel ** 2) / self.frob_norm ** 2), 1.0)
            eta_est = Q.amplitude_estimation(a=eta, epsilon=delta, random_state=rng)
            if eta_est == 1:
                u = tau
            else:
                l = tau
            tau = (u + l) / 2
        self.est_sing_min = tau * self.frob_norm
        return tau * self.frob_norm

    def quantum_factor_score_ratio_sum(self, eps, theta, eta):
        """Theorem 9 (``_qPCA.py:982-999``): AE of the retained-variance ratio
        of the singular values whose CPE estimate is >= theta."""
        if not theta:
            theta = self.est_theta
        est = self._cpe_sv(self.singular_values_ / self.muA, eps, eps + np.pi, eps,
                           1 - 1 / self.n_features_)
        sel = self.singular_values_[est >= theta]
        p = float(np.sum(sel ** 2) / np.sum(self.singular_values_ ** 2))
        return Q.amplitude_estimation(a=p, epsilon=eta, random_state=self._rng("ae"))

    def estimate_theta(self, epsilon, eta, p):
        """Theorem 10 (``_qPCA.py:1002-1022``): binary search on theta."""
        l, u = 0.0, 1.0
        log.debug("estimate_theta start")
        if abs(l - p) <= eta:
            return self.muA
        if abs(u - p) <= eta:
            return 0
        n_it = int(np.ceil(np.log(self.muA / epsilon)))
        tau = (l + u) / 2
        for _ in range(n_it):
            p_est = self.quantum_factor_score_ratio_sum(eps=epsilon / self.muA, theta=tau, eta=eta / 2)
            log.debug("tau=%s p_est-p=%s", tau, p_est - p)
            if abs(p_est - p) <= eta / 2:
                return tau * self.muA
            if p_est < p:
                u = tau
            else:
                l = tau
            tau = (u + l) / 2
        raise ValueError("The binary search doesn't found any values")

    def _sv_estimates(self, eps, sv=None):
        sv = self.singular_values_ if sv is None else sv
        e = eps / self.muA
        est = self._cpe_sv(sv / self.muA, e, e + np.pi, e, 1 - 1 / self.n_features_)
        return est * self.muA

    def _tomography(self, A, delta, true_tomography, norm, stop_when_reached_accuracy,
                    incremental_measure, faster_measure_increment, tag, sharded=False):
        """Tomography of the rows of A (numpy or device tensor).  ``sharded``:
        A holds this rank's columns of vectors whose coordinates are
        row-sharded over the ranks (the left singular vectors of row-sharded
        data)."""
        if delta == 0 or (hasattr(A, "shape") and A.shape[0] == 0):
            return A
        key = self._key("tomography", zlib.crc32(tag.encode()) & 0xFFFF)
        comm = getattr(self, "_comm", None)
        if sharded and isinstance(A, torch.Tensor) and comm is not None and comm.distributed:
            n_glob = int(self.n_samples_)
            if not true_tomography:
                # Frobenius budget over the GLOBAL r x n matrix; element (i, j)
                # draws Philox element i * n_global + row_offset + j - the
                # unsharded draw (shard invariant)
                return gaussian_tomography(A, delta, key, offset=int(self._row_offset),
                                           numel=A.shape[0] * n_glob, row_stride=n_glob)
            return tomography_long(A, delta, key, norm=norm,
                                   stop_when_reached_accuracy=stop_when_reached_accuracy,
                                   incremental_measure=incremental_measure,
                                   faster_measure_increment=faster_measure_increment,
                                   preserve_norm=self.preserve_norm_tomography, comm=comm,
                                   n_global=n_glob)
        if isinstance(A, torch.Tensor):
            if not true_tomography:
                return gaussian_tomography(A, delta, key)
            return tomography_rows_torch(A.double(), delta, key, norm=norm,
                                         stop_when_reached_accuracy=stop_when_reached_accuracy,
                                         incremental_measure=incremental_measure,
                                         faster_measure_increment=faster_measure_increment,
                                         preserve_norm=self.preserve_norm_tomography)
        if not true_tomography:
            return Q.tomography(np.asarray(A), delta, true_tomography=False, random_state=self._rng(tag))
        t = torch.as_tensor(np.asarray(A, dtype=np.float64))
        out = tomography_rows_torch(t, delta, key, norm=norm,
                                    stop_when_reached_accuracy=stop_when_reached_accuracy,
                                    incremental_measure=incremental_measure,
                                    faster_measure_increment=faster_measure_increment,
                                    preserve_norm=self.preserve_norm_tomography)
        return out.numpy()

    def topk_sv_extractors(self, X, delta, eps, theta, true_tomography, norm,
                           stop_when_reached_accuracy, incremental_measure,
                           faster_measure_increment, check_sv_uniform_distribution=False):
        """Theorem 11 (``_qPCA.py:1025-1068``)."""
        if theta == 0:
            if not hasattr(self, "est_theta"):
                raise ValueError("theta_major must be > 0 (or fit with theta_estimate=True)")
            theta = self.est_theta
        est = self._sv_estimates(eps)
        mask = est >= theta
        self.top_k_true_singular_value = self.singular_values_[mask]
        sv_est = est[mask]
        if check_sv_uniform_distribution:  # pragma: no cover - plotting
            import matplotlib.pyplot as plt
            plt.plot(self.top_k_true_singular_value / sv_est)
            plt.show()
        self.topk = int(len(sv_est))
        self.topk_p = float(np.sum(self.top_k_true_singular_value ** 2) / np.sum(self.singular_values_ ** 2))
        self.topk_right_singular_vectors = self.components_[mask]
        left = self.left_sv[torch.as_tensor(mask)] if isinstance(self.left_sv, torch.Tensor) \
            else np.asarray(self.left_sv)[mask]
        self.topk_left_singular_vectors = left
        tk = (true_tomography, norm, stop_when_reached_accuracy, incremental_measure,
              faster_measure_increment)
        with self._phase("tomography_right"):
            right_est = self._tomography(self.topk_right_singular_vectors, delta, *tk, tag="right")
        with self._phase("tomography_left"):
            left_est = self._tomography(left, delta, *tk, tag="left", sharded=True)
        fro2 = self.frob_norm ** 2
        return (right_est, left_est, sv_est, (sv_est ** 2) / (self.n_samples_ - 1),
                np.array([fs / fro2 for fs in sv_est ** 2]))

    def least_k_sv_extractors(self, X, delta, eps, theta, true_tomography, norm,
                              stop_when_reached_accuracy, incremental_measure,
                              faster_measure_increment, check_sv_uniform_distribution=False):
        """Least-k mirror of Theorem 11 (``_qPCA.py:1070-1121``): among the
        non-zero singular values, those whose estimate is < theta_minor."""
        if theta == 0:
            theta = getattr(self, "least_theta", 0)
        sv = self.singular_values_
        zero = np.where(np.isclose(sv, 0))[0]
        nz = zero[0] if zero.size else len(sv)
        est = self._sv_estimates(eps, sv[:nz])
        mask = est < theta
        self.least_k_true_singular_value = sv[:nz][mask]
        sv_est = est[mask]
        self.least_k = int(len(sv_est))
        self.least_k_p = float(np.sum(self.least_k_true_singular_value ** 2) / np.sum(sv ** 2))
        self.leastk_right_singular_vectors = self.components_[:nz][mask]
        left = self.left_sv[:nz][torch.as_tensor(mask)] if isinstance(self.left_sv, torch.Tensor) \
            else np.asarray(self.left_sv)[:nz][mask]
        self.leastk_left_singular_vectors = left
        tk = (true_tomography, norm, stop_when_reached_accuracy, incremental_measure,
              faster_measure_increment)
        right_est = self._tomography(self.leastk_right_singular_vectors, delta, *tk, tag="lright")
        left_est = self._tomography(left, delta, *tk, tag="lleft", sharded=True)
        fro2 = self.frob_norm ** 2
        return (right_est, left_est, sv_est, (sv_est ** 2) / (self.n_samples_ - 1),
                np.array([fs / fro2 for fs in sv_est ** 2]))

    # ----------------------------------------------------------- transform
    def transform(self, X, classic_transform=True, epsilon_delta=0, quantum_representation=False,
                  norm="None", psi=0, true_tomography=True, use_classical_components=True,
                  tomography=None):
        """Classical projection, or the quantum representation of the projected
        data (``_qPCA.py:773-846``).  ``tomography=`` is accepted as an alias
        of ``true_tomography`` (the reference's driver passes it,
        ``MnistTrial.py:19``, and crashes with TypeError there)."""
        if tomography is not None:
            true_tomography = bool(tomography)
        if classic_transform:
            if epsilon_delta != 0 or quantum_representation or (norm not in ("None", None)) or psi != 0:
                warnings.warn("Warning! You are using the classical transform, so the quantum "
                              "parameter are useless.")
            return super().transform(X)
        X_final = super().transform(X, use_classical_components)
        if not use_classical_components:
            return X_final
        if quantum_representation:
            assert (psi > 0 if norm != "est_representation" else psi >= 0)
            assert epsilon_delta > 0
            res = self.compute_quantum_representation(X_final, psi=psi, epsilon_delta=epsilon_delta,
                                                      type=norm, true_tomography=true_tomography)
            return {"quantum_representation_results": res}
        return X_final

    def compute_error(self, U, epsilon_delta, true_tomography):
        if not true_tomography:
            epsilon_delta = np.sqrt(self.n_components_) * epsilon_delta
        A = self._tomography(U, epsilon_delta, true_tomography, "L2", True, True, 0, tag="repr")
        if isinstance(U, torch.Tensor):
            f = float(torch.linalg.norm(U.double() - A.double()))
        else:
            f = float(np.linalg.norm(np.asarray(U) - np.asarray(A)))
        return A, epsilon_delta, f

    def compute_quantum_representation(self, X, psi, epsilon_delta, true_tomography, type="None"):
        if type == "est_representation":
            return self.compute_error(X, epsilon_delta, true_tomography)
        Y = self._tomography(X, psi, true_tomography, "L2", True, True, 0, tag="qrepr")
        Yn = to_numpy(Y)
        if type == "q_state":
            f = np.linalg.norm(Yn)
            norms = np.linalg.norm(Yn, axis=1) / f
            return Q.QuantumState(registers=list(Yn / f), amplitudes=norms,
                                  random_state=self._rng("qstate"))
        if type == "None":
            return Y
        if type == "f_norm":
            return Y / np.linalg.norm(Yn)
        raise ValueError(f"unknown quantum representation type {type!r}")

    def inverse_transform(self, X, use_classical_components=True):
        return super().inverse_transform(X, use_classical_components)

    def fit_transform(self, X, y=None, **quantum_kw):
        if sp.issparse(X) and not _stays_sparse(X):
            X = X.toarray()        # small: the array path for the fit and the projection
        return self.fit(X, **quantum_kw).transform(X)

    def score_samples(self, X):
        check_is_fitted(self)
        if sp.issparse(X):
            raise TypeError("QPCA.score_samples does not support sparse input: the precision "
                            "matrix is n_features x n_features")
        X = np.asarray(to_numpy(X), dtype=np.float64)
        Xr = X - self.mean_
        n_features = X.shape[1]
        precision = self.get_precision()
        log_like = -0.5 * (Xr * (Xr @ precision)).sum(axis=1)
        log_like -= 0.5 * (n_features * np.log(2.0 * np.pi) - fast_logdet(precision))
        return log_like

    def score(self, X, y=None):
        return float(np.mean(self.score_samples(X)))

    # ---------------------------------------------------------- cost model
    def ret_variance(self, explained_variance_ratio_, variance):
        ratio_cumsum = stable_cumsum(explained_variance_ratio_)
        return int(np.searchsorted(ratio_cumsum, variance, side="right") + 1)

    def q_ret_variance(self, measurements, variance):
        """Sample the retained-variance rank from a QuantumState over the scaled
        singular values (``_qPCA.py:1210-1226``)."""
        if isinstance(self.n_components, int):
            return self.n_components
        sv = getattr(self, "scaled_singular_values", self.singular_values_ / self.spectral_norm)
        qs = Q.QuantumState(registers=list(sv), amplitudes=list(sv), random_state=self._rng("qrv"))
        est = Q.estimate_wald(list(qs.measure(measurements)))
        keys = sorted(est.keys(), reverse=True)
        vals = np.array([est[k] for k in keys])
        acc, i = 0.0, 0
        while acc <= variance and i < len(vals):
            acc += vals[i]
            i += 1
        return i

    def accumulate_q_runtime(self, n_samples, n_features, estimate_components="all"):
        if not hasattr(self, "quantum_runtime_container"):
            self.quantum_runtime_container = []
        view = _KnobView(self)
        self.quantum_runtime_container += cost_model.qpca_runtime_terms(view, n_samples, n_features,
                                                                       estimate_components)
        return self.quantum_runtime_container

    def runtime_comparison(self, n_samples, n_features, saveas=None, estimate_components="all",
                           classic_runtime="classic", plot=False):
        """(q_runtime, c_runtime) on a 100x100 grid (``_qPCA.py:1235-1315``)."""
        n, m = np.meshgrid(np.linspace(1, n_samples, dtype=np.int64, num=100),
                           np.linspace(1, n_features, dtype=np.int64, num=100))
        if classic_runtime == "rand":
            c = n * m * np.log(getattr(self, "components_retained_", self.n_components_))
        else:
            c = n * m ** 2
        self.quantum_runtime_container = []
        q = self.accumulate_q_runtime(n, m, estimate_components)
        q = np.sum(q, axis=0) if len(q) > 1 else (q[0] if q else np.zeros_like(n, dtype=float))
        if plot:
            cost_model.plot_runtime(n, m, q, c, f"{self.name} VS q-{self.name}", saveas)
        return q, c


class _KnobView:
    """Attribute view used by the cost model (fitted knob values)."""

    def __init__(self, est):
        k = est._knobs
        self.theta_estimate = k["theta_estimate"]
        self.quantum_retained_variance = k["quantum_retained_variance"]
        self.estimate_all = k["estimate_all"]
        self.estimate_least_k = k["estimate_least_k"]
        self.muA = est.muA
        self.eps = k["eps"]
        self.eps_theta = k["eps_theta"]
        self.eta = k["eta"]
        self.theta_major = k["theta_major"]
        self.theta_minor = k["theta_minor"]
        self.est_theta = getattr(est, "est_theta", 0.0)
        self.topk = getattr(est, "topk", 0)
        self.topk_p = getattr(est, "topk_p", 1.0)
        self.spectral_norm = est.spectral_norm
        self.delta = k["delta"]
        self.tomography_norm = k["norm"]
        self.singular_values_ = est.singular_values_
        self.least_k = getattr(est, "least_k", 0)
        self.least_k_p = getattr(est, "least_k_p", 1.0)


qPCA = QPCA
