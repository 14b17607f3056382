"""Device path of ``LatentDirichletAllocation`` (``device="cpu"`` /
``"cuda"``): the corpus goes to the device once per call as CSR, the E-step
and the per-document term of the bound are ``ops.sparse_lda`` (HIP kernels on
a GPU, fp64 torch twins on the CPU), the M-step and the Dirichlet
expectations are torch on the device.  The random draws stay the estimator's
numpy draws in the host path's order, so a seeded fit follows the host fit to
rounding.  Nothing here outlives the call: :meth:`DeviceLDA.store` writes the
fitted arrays back to the estimator as numpy.
"""

import math

import numpy as np
import torch

from ...ops import sparse_lda as L
from ...runtime.device import resolve_device
from .._data import as_sparse_data


# the host path's digamma law, series truncation included: torch.special.digamma
# would move a seeded fit off the host fit by about 1e-13 per evaluation
_dirichlet_expectation = L.dirichlet_expectation


def _ll(prior, distr, ddistr, size):
    s = ((prior - distr) * ddistr).sum()
    s = s + (torch.lgamma(distr) - math.lgamma(prior)).sum()
    s = s + (math.lgamma(prior * size) - torch.lgamma(distr.sum(1))).sum()
    return s


class DeviceLDA:
    """The device state of one estimator call on the validated scipy CSR
    matrix ``X``: the corpus, ``components_`` [k, F] and the transposed
    ``E[log beta]`` / ``exp(E[log beta])`` tables [F, k] of the kernels."""

    def __init__(self, est, X):
        self.est = est
        self.k = int(est.n_components)
        L.check_k(self.k)
        self.dev = resolve_device(est.device)
        self.sd = as_sparse_data(X, self.dev)
        self.n = X.shape[0]
        self.word_count = float(X.sum())
        self.comp = torch.from_numpy(np.ascontiguousarray(est.components_, dtype=np.float64)) \
            .to(self.dev)
        self.refresh()

    def refresh(self):
        self.elog_t = _dirichlet_expectation(self.comp).T.contiguous()
        self.exp_t = torch.exp(self.elog_t)

    def store(self):
        self.est.components_ = self.comp.cpu().numpy()
        self.est.exp_dirichlet_component_ = self.exp_t.T.contiguous().cpu().numpy()

    def e_step(self, a, b, cal_sstats, random_init):
        est = self.est
        dt = est.random_state_.gamma(100.0, 0.01, (b - a, self.k)) if random_init \
            else np.ones((b - a, self.k))
        dt, ss, _ = L.lda_estep(self.sd, self.exp_t, torch.from_numpy(dt).to(self.dev),
                                float(est.doc_topic_prior_), int(est.max_doc_update_iter),
                                float(est.mean_change_tol), rows=(a, b), want_stats=cal_sstats)
        return dt, ss

    def em_step(self, a, b, total_samples, batch_update):
        est = self.est
        _, ss = self.e_step(a, b, True, True)
        if batch_update:
            self.comp = est.topic_word_prior_ + ss
        else:
            w = float(np.power(est.learning_offset + est.n_batch_iter_, -est.learning_decay))
            ratio = float(total_samples) / (b - a)
            self.comp = self.comp * (1 - w)
            self.comp += w * (est.topic_word_prior_ + ratio * ss)
        self.refresh()
        est.n_batch_iter_ += 1

    def approx_bound(self, dt, sub_sampling):
        est = self.est
        ddt = _dirichlet_expectation(dt)
        score = L.lda_doc_bound(self.sd, ddt, self.elog_t).sum()
        score = score + _ll(float(est.doc_topic_prior_), dt, ddt, self.k)
        if sub_sampling:
            score = score * (float(est.total_samples) / self.n)
        score = score + _ll(float(est.topic_word_prior_), self.comp, self.elog_t.T,
                            self.comp.shape[1])
        return float(score)

    def perplexity(self, dt, sub_sampling):
        bound = self.approx_bound(dt, sub_sampling)
        wc = self.word_count * (float(self.est.total_samples) / self.n if sub_sampling else 1.0)
        return np.exp(-1.0 * bound / wc)
