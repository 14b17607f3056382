"""Corpus generator and host references shared by test_lda_device_cpu.py and
test_lda_device_gpu.py.

The corpus is 300 documents x 500 words of integer counts, fixed by seed:
document 0 is empty, document 1 has one word, the last 20 words occur in no
document, and ``long_words`` > 0 replaces document 2 by one with that many
stored words.  The reference is the host E-step ``sqh_lda_estep`` on one
thread.  Its own sensitivity to the summation order - the floor every
tolerance here is a multiple of - is measured by running it on 4
column-permuted copies of the corpus: the same mathematics, the words of every
document in another order.
"""
import ctypes
import functools
import os
from unittest import mock

import numpy as np
import scipy.sparse as sp
from scipy.special import logsumexp

from sq_learn_amd.decomposition import LatentDirichletAllocation
from sq_learn_amd.models.decomposition._extra import _dirichlet_expectation_2d
from sq_learn_amd.ops import _host

N_DOCS, N_WORDS, UNUSED = 300, 500, 20
KS = (5, 64, 70, 130)
MARGIN = 64.0          # tolerance = MARGIN x the measured floor
SS_MIN = 1e-12         # statistics entries above it are compared relatively
N_PERM = 4
EPS64 = float(np.finfo(np.float64).eps)
PROFILE = os.environ.get("SQ_LDA_RECORD")   # a file the observed floors / ratios are appended to


def _c(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


@functools.lru_cache(maxsize=None)
def corpus(long_words=0, seed=0):
    rng = np.random.RandomState(seed)
    used = N_WORDS - UNUSED
    topics = rng.dirichlet(np.full(used, 0.05), 8)
    X = np.zeros((N_DOCS, N_WORDS))
    for i in range(N_DOCS):
        mix = rng.dirichlet(np.full(8, 0.3))
        X[i, :used] = rng.multinomial(rng.randint(20, 120), mix @ topics)
    X[0] = 0
    X[1] = 0
    X[1, 17] = 3
    if long_words:
        assert long_words <= used
        X[2] = 0
        X[2, rng.permutation(used)[:long_words]] = rng.randint(1, 4, long_words)
    X = sp.csr_matrix(X)
    X.sort_indices()
    assert X[0].nnz == 0 and X[1].nnz == 1 and X[:, used:].nnz == 0
    return X


@functools.lru_cache(maxsize=None)
def tables(k, seed=0):
    """(exp_tw [k, F], elog_beta [k, F], doc_topic draws [n, k], prior)."""
    rng = np.random.RandomState(1000 + seed + k)
    comp = rng.gamma(100.0, 0.01, (k, N_WORDS))
    elog = _dirichlet_expectation_2d(comp)
    return np.exp(elog), elog, rng.gamma(100.0, 0.01, (N_DOCS, k)), 1.0 / k


def host_estep(X, exp_tw, dt0, prior, max_iters, tol, want_stats=True):
    """``sqh_lda_estep`` on one thread: (doc_topic, statistics already
    multiplied by ``exp_tw`` or None)."""
    n, F = X.shape
    k = exp_tw.shape[0]
    dt = np.ascontiguousarray(dt0, dtype=np.float64).copy()
    ss = np.zeros((k, F)) if want_stats else None
    etw = np.ascontiguousarray(exp_tw)
    # named, so that the arrays outlive the pointers taken from them
    val = np.ascontiguousarray(X.data, dtype=np.float64)
    ind, ptr = X.indices.astype(np.int64), X.indptr.astype(np.int64)
    _host.lib().sqh_lda_estep(_c(val), _c(ind), _c(ptr), n, k, F, _c(etw), float(prior),
                              int(max_iters), float(tol), _c(dt), _c(ss), 1)
    return dt, (ss * etw if want_stats else None)


def host_doc_bound(X, elog_theta, elog_beta):
    """The per-document term of ``_approx_bound``, document by document."""
    out = np.zeros(X.shape[0])
    for i in range(X.shape[0]):
        ids = X.indices[X.indptr[i]:X.indptr[i + 1]]
        cnts = X.data[X.indptr[i]:X.indptr[i + 1]]
        if ids.size:
            out[i] = cnts @ logsumexp(elog_theta[i, :, None] + elog_beta[:, ids], axis=0)
    return out


def rel_dev(a, ref, floor_abs=0.0):
    """Largest relative deviation of ``a`` from ``ref`` over the entries of
    ``ref`` above ``floor_abs`` in magnitude."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    sel = np.abs(ref) > floor_abs
    if not sel.any():
        return 0.0
    return float(np.max(np.abs(a[sel] - ref[sel]) / np.abs(ref[sel])))


def _perms(F, seed=7):
    rng = np.random.RandomState(seed)
    return [rng.permutation(F) for _ in range(N_PERM)]


def _permuted(X, p):
    Xp = sp.csr_matrix(X[:, p])
    Xp.sort_indices()
    return Xp


@functools.lru_cache(maxsize=None)
def estep_reference(k, max_iters, tol, long_words=0, n_docs=N_DOCS):
    """(doc_topic, ss, floor_dt, floor_ss) of the host E-step on the first
    ``n_docs`` documents: the floors are its largest relative deviations over
    the column-permuted copies."""
    X = corpus(long_words)[:n_docs]
    exp_tw, _, dt0, prior = tables(k)
    dt0 = dt0[:n_docs]
    dt, ss = host_estep(X, exp_tw, dt0, prior, max_iters, tol)
    f_dt = f_ss = 0.0
    for p in _perms(X.shape[1]):
        dtp, ssp = host_estep(_permuted(X, p), exp_tw[:, p], dt0, prior, max_iters, tol)
        back = np.empty_like(ssp)
        back[:, p] = ssp
        f_dt = max(f_dt, rel_dev(dtp, dt))
        f_ss = max(f_ss, rel_dev(back, ss, SS_MIN))
    return dt, ss, f_dt, f_ss


@functools.lru_cache(maxsize=None)
def bound_reference(k, long_words=0, n_docs=N_DOCS):
    """(elog_theta, per-document bound, floor) of the numpy expression on the
    first ``n_docs`` documents."""
    X = corpus(long_words)[:n_docs]
    _, elog, dt0, _ = tables(k)
    et = _dirichlet_expectation_2d(dt0[:n_docs])
    ref = host_doc_bound(X, et, elog)
    floor = 0.0
    for p in _perms(X.shape[1]):
        floor = max(floor, rel_dev(host_doc_bound(_permuted(X, p), et, elog[:, p]), ref))
    return et, ref, floor


@functools.lru_cache(maxsize=None)
def iters_reference(k, tol, max_iters=100):
    """(iterations every document performs under ``tol``, the closest any
    mean change comes to ``tol`` relative to it) from the reference sequence:
    the host E-step one iteration at a time (an iteration starts from
    ``doc_topic`` alone, so the sequence is the one of a single call)."""
    X = corpus()
    exp_tw, _, dt0, prior = tables(k)
    n = X.shape[0]
    iters = np.zeros(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    closest = np.inf
    dt = dt0.copy()
    for _ in range(max_iters):
        if not live.any():
            break
        nd, _ = host_estep(X, exp_tw, dt, prior, 1, 0.0, want_stats=False)
        mc = np.abs(nd - dt).sum(1) / k
        closest = min(closest, float(np.min(np.abs(mc[live] - tol) / tol)))
        iters[live] += 1
        dt[live] = nd[live]
        live &= ~(mc < tol)
    return iters, closest


@functools.lru_cache(maxsize=None)
def fitted_floor(method, k):
    """The host path's own largest relative deviations of the fitted
    quantities (5 EM iterations, seed 0, one host thread) over column-permuted
    copies of the corpus, each fit started from the same ``components_`` draw
    permuted with the columns: (the ``device=None`` quantities, their
    floors)."""
    X = corpus()
    base = _host_fit(method, k, X, None)
    floors = dict.fromkeys(base, 0.0)
    for p in _perms(X.shape[1]):
        got = _host_fit(method, k, _permuted(X, p), p)
        for name in base:
            floors[name] = max(floors[name], rel_dev(got[name], base[name]))
    return base, floors


class _PermutedInit(LatentDirichletAllocation):
    """The host estimator with its initial ``components_`` draw permuted with
    the columns, so that a fit of a column-permuted corpus is the same
    mathematics in another order."""

    perm = None

    def _init_latent_vars(self, d):
        super()._init_latent_vars(d)
        if self.perm is not None:
            self.components_ = np.ascontiguousarray(self.components_[:, self.perm])
            self.exp_dirichlet_component_ = np.ascontiguousarray(
                self.exp_dirichlet_component_[:, self.perm])


def quantities(est, X, perm=None):
    comp = est.components_
    if perm is not None:
        back = np.empty_like(comp)
        back[:, perm] = comp
        comp = back
    return dict(components=comp, transform=est.transform(X), perplexity=est.perplexity(X),
                score=est.score(X), bound=est.bound_)


def one_thread():
    """The host path on one thread: with more, the dynamic schedule changes
    the order in which its per-thread statistics are summed from run to run."""
    return mock.patch.dict(os.environ, {"OMP_NUM_THREADS": "1"})


def _host_fit(method, k, X, perm):
    est = _PermutedInit(k, learning_method=method, random_state=0, max_iter=5, batch_size=64)
    est.perm = perm
    with one_thread():
        return quantities(est.fit(X), X, perm)


def record(name, floor, ratio):
    """Append an observed floor and the observed deviation / floor ratio to
    the file named by SQ_LDA_RECORD (the source of profiles/lda_device.md)."""
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(f"{name}\tfloor={floor:.3e}\tratio={ratio:.3f}\n")


def check(name, got, ref, floor, floor_abs=0.0):
    """``got`` within MARGIN x floor of ``ref`` (relative, entries above
    ``floor_abs``); prints the figures before asserting."""
    # Four permutations of a single scalar (a perplexity, a score) can agree bit for bit, which
    # measures a floor of 0.  No fp64 figure is reproducible below its own rounding unit, so
    # that unit bounds every floor from below.
    floor = max(floor, EPS64)
    dev = rel_dev(got, ref, floor_abs)
    ratio = dev / floor
    print(f"{name}: floor {floor:.3e} deviation {dev:.3e} ratio {ratio:.3f}")
    record(name, floor, ratio)
    assert dev <= MARGIN * floor, (name, dev, floor, ratio)
