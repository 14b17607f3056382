"""Corpus, numpy yardsticks, measured floors and the shared checks of
test_logistic_sparse_cpu.py and test_logistic_sparse_gpu.py.

The matrix is 300 x 320 integer counts (1 to 5, about 5 % density, exact in
fp32), fixed by seed and edited so that it holds rows of 0, 1, 63, 64, 65 and
300 stored entries, a column no row uses and a column stored in every
non-empty row: its transposed row has 299 entries, five segments at ``seg=64``.
Labels come from a planted linear model with Gumbel noise; every class is
present.

Tolerances are measured (the rule of ``_nmf_data.py``): the yardstick is a
numpy fp64 expression on the densified matrix, its floor the largest deviation
of that expression over ``N_PERM`` copies whose rows, columns and class labels
are permuted, clamped from below at the fp64 rounding unit; a result must lie
within ``MARGIN`` x the floor under ``norm_dev``.  Fit-level comparisons also
assert that the floor is at most ``FLOOR_MAX``.
"""
import contextlib
import functools
import os
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from sq_learn_amd.linear_model import LogisticRegression
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.ops import sparse_logistic as S
from sq_learn_amd.ops._csr import csr_transpose

N, D = 300, 320
KS = (2, 3, 64, 65, 256, 257, 300)     # sub-tile and pass boundaries of the multinomial kernel
SETTINGS = ("random", "optimum", "huge")
MARGIN = 64.0
N_PERM = 4
FLOOR_MAX = 1e-9
EPS64 = float(np.finfo(np.float64).eps)
PROFILE = os.environ.get("SQ_LOGIT_RECORD")   # a file the observed floors / ratios are appended to

ROW_EMPTY, ROW_ONE, ROWS_TILE, ROW_LONG = 0, 20, (2, 3, 4), 5
COL_ALL, UNUSED_COL = 0, D - 1


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.RandomState(0)
    used = D - 1
    X = np.zeros((N, D))
    mask = rng.rand(N, used) < 0.05
    X[:, :used][mask] = rng.randint(1, 6, int(mask.sum()))
    X[:, COL_ALL] = rng.randint(1, 6, N)

    def fill(i, count):
        X[i] = 0
        if count:
            X[i, COL_ALL] = rng.randint(1, 6)
            X[i, 1 + rng.permutation(used - 1)[:count - 1]] = rng.randint(1, 6, count - 1)

    fill(ROW_EMPTY, 0)
    fill(ROW_ONE, 1)
    for i, c in zip(ROWS_TILE, (63, 64, 65)):
        fill(i, c)
    fill(ROW_LONG, 300)
    X = sp.csr_matrix(X)
    X.sort_indices()
    assert X[:, UNUSED_COL].nnz == 0 and X[:, COL_ALL].nnz == N - 1
    assert np.array_equal(X.data, X.data.astype(np.float32))
    return X


@functools.lru_cache(maxsize=None)
def dense():
    return corpus().toarray()


@functools.lru_cache(maxsize=None)
def labels(K):
    """Class indices from a planted model, every class present."""
    rng = np.random.RandomState(100 + K)
    z = dense() @ (0.3 * rng.randn(D, K)) + rng.gumbel(size=(N, K))
    lab = z.argmax(1)
    lab[rng.permutation(N)[:K]] = np.arange(K)
    assert len(np.unique(lab)) == K
    return lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def row_weights(weighted):
    if not weighted:
        return np.ones(N)
    sw = 2.0 * np.random.RandomState(9).rand(N)
    sw[::5] = 0.0
    return sw


@functools.lru_cache(maxsize=None)
def perms(K, seed=7):
    rng = np.random.RandomState(seed + K)
    return [(rng.permutation(N), rng.permutation(D), rng.permutation(K)) for _ in range(N_PERM)]


# ------------------------------------------------------------------ metrics
def norm_dev(a, ref):
    """max |a - ref| / max |ref|."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.max(np.abs(ref), initial=0.0))
    dev = float(np.max(np.abs(a - ref), initial=0.0))
    return dev / scale if scale > 0 else dev


def record(name, floor, ratio):
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(f"{name}\tfloor={floor:.3e}\tratio={ratio:.3f}\n")


def check(name, got, ref, floor, small_floor=False):
    """``got`` within MARGIN x floor of ``ref`` under ``norm_dev``, everything
    finite; with ``small_floor`` the floor itself must be at most FLOOR_MAX.
    Prints the figures before asserting."""
    floor = max(floor, EPS64)
    assert np.all(np.isfinite(got)), (name, "not finite")
    dev = norm_dev(got, ref)
    ratio = dev / floor
    print(f"{name}: floor {floor:.3e} deviation {dev:.3e} ratio {ratio:.3f}")
    record(name, floor, ratio)
    if small_floor:
        assert floor <= FLOOR_MAX, (name, "the reference itself is unstable here", floor)
    assert dev <= MARGIN * floor, (name, dev, floor, ratio)


# ---------------------------------------------------------------- yardsticks
def multi_expr(Xd, W, b, lab, sw):
    """(loss, R [n, K], G [K, d]) of the multinomial loss in numpy fp64."""
    z = Xd @ W.T + b
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    ar = np.arange(Xd.shape[0])
    loss = float((sw * (lse - z[ar, lab])).sum())
    R = np.exp(z - lse[:, None])
    R[ar, lab] -= 1.0
    R *= sw[:, None]
    return loss, R, R.T @ Xd


def bin_expr(Xd, w, b, lab, sw):
    """(loss, r [n], g [d]) of the binary loss in numpy fp64."""
    t = np.where(lab != 0, 1.0, -1.0)
    tz = t * (Xd @ w + b)
    with np.errstate(over="ignore"):
        loss = float((sw * (np.maximum(-tz, 0.0) + np.log1p(np.exp(-np.abs(tz))))).sum())
        r = -sw * t / (1.0 + np.exp(tz))
    return loss, r, Xd.T @ r


@contextlib.contextmanager
def one_thread():
    """The fits evaluate a small objective hundreds of times: one torch thread
    for their duration, a pool of threads only waits on itself there."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def _host_fit(Xd, y, **kw):
    with warnings.catch_warnings(), one_thread():
        warnings.simplefilter("ignore")
        return LogisticRegression(**kw).fit(Xd, y)


@functools.lru_cache(maxsize=None)
def weights(K, setting, binary=False):
    """(W [K, D] or w [D], b [K] or a float) at one of ``SETTINGS``: random
    weights, the fitted optimum (the gradient of the penalised objective
    cancels there), or weights scaled so that the logits reach about +-1e4."""
    rng = np.random.RandomState(200 + K)
    lab = labels(K)
    if setting == "optimum":
        est = _host_fit(dense(), lab, tol=1e-6, max_iter=300)
        W, b = est.coef_, est.intercept_
        if K == 2 and not binary:
            W, b = np.vstack([-W, W]) / 2, np.concatenate([-b, b]) / 2
    else:
        W, b = 0.1 * rng.randn(1 if binary else K, D), 0.1 * rng.randn(1 if binary else K)
        if setting == "huge":
            scale = 1e4 / np.abs(dense() @ W.T + b).max()
            W, b = W * scale, b * scale
    return (W[0].copy(), float(b[0])) if binary else (np.ascontiguousarray(W), b.copy())


def _floors(base, copies):
    return [max(norm_dev(c[j], base[j]) for c in copies) for j in range(len(base))]


@functools.lru_cache(maxsize=None)
def multi_reference(K, setting, weighted):
    """((loss, R, G), their floors)."""
    Xd, lab, sw = dense(), labels(K), row_weights(weighted)
    W, b = weights(K, setting)
    base = multi_expr(Xd, W, b, lab, sw)
    copies = []
    for pr, pc, pk in perms(K):
        Wp, bp = np.empty_like(W), np.empty_like(b)
        Wp[pk], bp[pk] = W, b                      # class c becomes class pk[c]
        loss, R, G = multi_expr(Xd[pr][:, pc], Wp[:, pc], bp, pk[lab[pr]], sw[pr])
        Rb, Gb = np.empty_like(R), np.empty_like(G)
        Rb[pr] = R[:, pk]
        Gb[:, pc] = G[pk]
        copies.append((loss, Rb, Gb))
    return base, _floors(base, copies)


@functools.lru_cache(maxsize=None)
def bin_reference(setting, weighted):
    """((loss, r, g), their floors) of the binary problem on ``labels(2)``."""
    Xd, lab, sw = dense(), labels(2), row_weights(weighted)
    w, b = weights(2, setting, binary=True)
    base = bin_expr(Xd, w, b, lab, sw)
    copies = []
    for pr, pc, _ in perms(2):
        loss, r, g = bin_expr(Xd[pr][:, pc], w[pc], b, lab[pr], sw[pr])
        rb, gb = np.empty_like(r), np.empty_like(g)
        rb[pr], gb[pc] = r, g
        copies.append((loss, rb, gb))
    return base, _floors(base, copies)


@functools.lru_cache(maxsize=None)
def matvec_reference(transposed):
    """(x, y = A x, floor) on the corpus or on its transpose."""
    Xd = dense().T.copy() if transposed else dense()
    x = np.random.RandomState(11).randn(Xd.shape[1])
    y = Xd @ x
    floor = 0.0
    for pr, pc, _ in perms(2):
        back = np.empty_like(y)
        rows, cols = (pc, pr) if transposed else (pr, pc)
        back[rows] = Xd[rows][:, cols] @ x[cols]
        floor = max(floor, norm_dev(back, y))
    return x, y, floor


# -------------------------------------------------------------- op checks
def _np(t):
    return t.detach().cpu().numpy()


def run_multi(device, K, setting, weighted):
    """``logit_multi`` and the gradient on ``device`` against the yardstick;
    returns the op's (loss, R) tensors."""
    (loss, R, G), (f_loss, f_r, f_g) = multi_reference(K, setting, weighted)
    W, b = weights(K, setting)
    sd = as_sparse_data(corpus(), device)
    gl, gr = S.logit_multi(sd, S.transposed_weights(W, sd.device), b, labels(K),
                           row_weights(weighted))
    assert gl.dim() == 0 and gl.dtype == torch.float64 and gl.device == sd.device
    assert gr.shape == (N, K) and gr.dtype == torch.float64
    tag = f"{device} multi K={K} {setting}{' weighted' if weighted else ''}"
    check(f"{tag} loss", float(gl), loss, f_loss)
    check(f"{tag} R", _np(gr), R, f_r)
    check(f"{tag} G", _np(S.sp_xtr(sd, gr)).T, G, f_g)
    return gl, gr


def run_bin(device, setting, weighted, seg=None):
    (loss, r, g), (f_loss, f_r, f_g) = bin_reference(setting, weighted)
    w, b = weights(2, setting, binary=True)
    sd = as_sparse_data(corpus(), device)
    gl, gr = S.logit_bin(sd, w, b, labels(2), row_weights(weighted))
    assert gl.dim() == 0 and gl.dtype == torch.float64 and gr.shape == (N,)
    tag = f"{device} bin {setting}{' weighted' if weighted else ''}"
    check(f"{tag} loss", float(gl), loss, f_loss)
    check(f"{tag} r", _np(gr), r, f_r)
    check(f"{tag} g", _np(S.sp_matvec(csr_transpose(sd), gr, seg=seg)), g, f_g)
    return gl, gr


def run_matvec(device, transposed, seg=None):
    x, y, floor = matvec_reference(transposed)
    sd = as_sparse_data(corpus(), device)
    got = S.sp_matvec(csr_transpose(sd) if transposed else sd, x, seg=seg)
    check(f"{device} matvec{'T' if transposed else ''} seg={seg}", _np(got), y, floor)
    return got


def check_refusals(device):
    import pytest
    sd = as_sparse_data(corpus(), device)
    K = 3
    W, b = weights(K, "random")
    Wt, lab, sw = S.transposed_weights(W, sd.device), labels(K), row_weights(False)
    for bad in (K, -1):
        wrong = lab.copy()
        wrong[7] = bad
        with pytest.raises(ValueError, match="outside"):
            S.logit_multi(sd, Wt, b, wrong, sw)
    with pytest.raises(ValueError, match="outside"):
        S.logit_bin(sd, W[0], 0.0, labels(3), sw)
    with pytest.raises(ValueError, match="do not match"):
        S.logit_multi(sd, Wt[:-1], b, lab, sw)
    with pytest.raises(ValueError, match="do not match"):
        S.logit_multi(sd, Wt[:, :K], b, lab, sw)          # not padded
    with pytest.raises(ValueError, match="does not match"):
        S.logit_multi(sd, Wt, b, lab[:-1], sw)
    with pytest.raises(ValueError, match="does not match"):
        S.logit_multi(sd, Wt, b, lab, sw[:-1])
    with pytest.raises(ValueError, match="does not match"):
        S.logit_bin(sd, W[0][:-1], 0.0, labels(2), sw)
    with pytest.raises(ValueError, match="does not match"):
        S.sp_matvec(sd, np.zeros(D + 1))
    with pytest.raises(TypeError):
        S.logit_multi(sd, Wt, b, lab.astype(np.float64), sw)


# --------------------------------------------------------------------- fits
FIT_NAMES = ("coef", "intercept", "proba")
FIT_CASES = {
    # id: (K, estimator parameters, weighted)
    "binary": (2, dict(), False),
    "ovr3": (3, dict(multi_class="ovr"), False),
    "multinomial3": (3, dict(), False),
    # C = 0.02: at C = 1 the host's own permuted fits of 65 classes on 300 rows differ by 2e-9
    # (L-BFGS-B stops on its function-decrease test), above FLOOR_MAX; here by 1e-11
    "multinomial65": (65, dict(C=0.02), False),
    "binary-no-intercept": (2, dict(fit_intercept=False), False),
    "multinomial3-no-intercept": (3, dict(fit_intercept=False), False),
    "binary-weighted": (2, dict(class_weight="balanced"), True),
    "multinomial3-weighted": (3, dict(class_weight="balanced"), True),
    "ovr3-newton-cg": (3, dict(multi_class="ovr", solver="newton-cg"), False),
    "binary-l1": (2, dict(penalty="l1", solver="liblinear", max_iter=60), False),
    "ovr3-l1": (3, dict(penalty="l1", solver="liblinear", max_iter=60), False),
}


def fit_weights(weighted):
    return 0.5 + np.random.RandomState(13).rand(N) if weighted else None


def fit(device, case, X=None, y=None, sw=None):
    """The fitted quantities of the case on the corpus (sparse, ``device``) or
    on the given copy (dense, host)."""
    K, kw, weighted = FIT_CASES[case]
    kw = dict(dict(tol=1e-8, max_iter=2000), **kw)
    if X is None:
        X, y, sw = corpus(), labels(K), fit_weights(weighted)
    with warnings.catch_warnings(), one_thread():
        warnings.simplefilter("ignore")
        est = LogisticRegression(device=device, **kw).fit(X, y, sample_weight=sw)
        return dict(coef=est.coef_, intercept=est.intercept_, proba=est.predict_proba(X),
                    predict=est.predict(X), n_iter=est.n_iter_, est=est)


@functools.lru_cache(maxsize=None)
def fit_reference(case):
    """(the ``device=None`` quantities on the densified corpus, their floors
    over the permuted copies).  Two classes keep their labels: the single
    coefficient row belongs to the second class."""
    K, kw, weighted = FIT_CASES[case]
    Xd, y, sw = dense(), labels(K), fit_weights(weighted)
    base = fit(None, case, Xd, y, sw)
    floors = dict.fromkeys(FIT_NAMES, 0.0)
    for pr, pc, pk in perms(K):
        if K == 2:
            pk = np.arange(2)
        got = fit(None, case, Xd[pr][:, pc], pk[y[pr]], None if sw is None else sw[pr])
        back = dict(coef=np.empty_like(base["coef"]), intercept=np.empty_like(base["intercept"]),
                    proba=np.empty_like(base["proba"]))
        rows = slice(None) if K == 2 else pk
        back["coef"][:, pc] = got["coef"][rows]
        back["intercept"][:] = got["intercept"][rows]
        back["proba"][pr] = got["proba"][:, pk]
        for name in FIT_NAMES:
            floors[name] = max(floors[name], norm_dev(back[name], base[name]))
    return base, floors


def check_fit(device, case):
    got = fit(device, case)
    base, floors = fit_reference(case)
    print(f"{device} fit {case}: n_iter {got['n_iter']} host {base['n_iter']}")
    np.testing.assert_array_equal(got["n_iter"], base["n_iter"])
    assert got["n_iter"].dtype == np.int32 and (got["n_iter"] < 2000).all()
    for name in FIT_NAMES:
        assert isinstance(got[name], np.ndarray) and got[name].shape == base[name].shape
        check(f"{device} fit {case} {name}", got[name], base[name], floors[name],
              small_floor=True)
    np.testing.assert_array_equal(got["predict"], base["predict"])
    return got["est"]


def l2_gradient(coef, K, C=1.0):
    """The numpy gradient of the l2-penalised objective without intercept at
    ``coef`` ([1, D] for two classes, else [K, D]), flattened."""
    Xd, lab, sw = dense(), labels(K), np.ones(N)
    if K == 2:
        return bin_expr(Xd, coef[0], 0.0, lab, sw)[2] + coef[0] / C
    return (multi_expr(Xd, coef, np.zeros(K), lab, sw)[2] + coef / C).ravel()
