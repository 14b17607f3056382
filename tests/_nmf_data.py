"""Corpus generator, host references and measured floors shared by
test_nmf_device_cpu.py and test_nmf_device_gpu.py.

The matrix is 300 x 500 integer counts (1 to 5, about 4 % density), fixed by
seed and edited so that it holds rows of 0, 1, 63, 64 and 65 stored entries,
for every k of ``KS`` a row of ``stage_entries(k) + 5`` entries (five more
than the ratio kernel stages, so both of its branches run), a column no row
uses and one explicitly stored zero.  The factors are ``0.3 |randn|`` with one
all-zero row each.

Tolerances are measured: a deviation must stay within ``MARGIN`` x the floor,
the reference's own largest deviation over ``N_PERM`` copies of the problem
whose rows, columns and component labels are permuted, the factors with them:
the same mathematics summed in another order.  The floor is clamped from below
at the fp64 rounding unit.  Coordinate descent clips at zero, a discrete
decision a permuted run can take differently; such a case is no yardstick, so
every coordinate-descent and fit comparison asserts that its floor is at most
``FLOOR_MAX``.
"""
import ctypes
import functools
import os
import warnings

import numpy as np
import scipy.sparse as sp

from sq_learn_amd.decomposition import NMF
from sq_learn_amd.models.decomposition import _extra as E
from sq_learn_amd.ops import _host
from sq_learn_amd.ops import sparse_nmf as S

N, D = 300, 500
KS = (1, 5, 64, 70, 130)
MARGIN = 64.0
N_PERM = 4
FLOOR_MAX = 1e-9
EPS64 = float(np.finfo(np.float64).eps)
EPSILON = S.EPSILON
PROFILE = os.environ.get("SQ_NMF_RECORD")   # a file the observed floors / ratios are appended to

# ROW_ZERO_P is an ordinary row, not one of the long rows 5 .. 9: those keep ordinary wh values
ROW_EMPTY, ROW_ONE, ROWS_TILE, ROW_LONG0, ROW_ZERO_P, COL_ZERO_Q = 0, 20, (2, 3, 4), 5, 12, 11
UNUSED_COL = D - 1


def _c(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def long_row(k):
    """The row with more stored entries than the ratio kernel stages at ``k``."""
    return ROW_LONG0 + KS.index(k)


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.RandomState(0)
    used = D - 1
    X = np.zeros((N, D))
    mask = rng.rand(N, used) < 0.04
    X[:, :used][mask] = rng.randint(1, 6, int(mask.sum()))

    def fill(i, count):
        X[i] = 0
        X[i, rng.permutation(used)[:count]] = rng.randint(1, 6, count)

    fill(ROW_EMPTY, 0)
    fill(ROW_ONE, 1)
    for i, c in zip(ROWS_TILE, (63, 64, 65)):
        fill(i, c)
    for k in KS:
        fill(long_row(k), S.stage_entries(k) + 5)
    X = sp.csr_matrix(X)
    X.sort_indices()
    z = X.indptr[10]                      # one explicitly stored zero, in row 10
    assert X.indptr[11] > z
    X.data[z] = 0.0
    assert X.nnz == X.indptr[-1] and X[:, UNUSED_COL].nnz == 0
    assert X[ROW_EMPTY].nnz == 0 and X[ROW_ONE].nnz == 1
    return X


@functools.lru_cache(maxsize=None)
def factors(k, seed=0):
    """(P [N, k], Q [D, k]): row ``ROW_ZERO_P`` of P and row ``COL_ZERO_Q`` of
    Q are zero, so ``wh == 0 -> EPSILON`` runs in both orientations."""
    rng = np.random.RandomState(1000 + seed + k)
    P = 0.3 * np.abs(rng.randn(N, k))
    Q = 0.3 * np.abs(rng.randn(D, k))
    P[ROW_ZERO_P] = 0.0
    Q[COL_ZERO_Q] = 0.0
    return P, Q


@functools.lru_cache(maxsize=None)
def perms(n, d, k, components=True, seed=7):
    rng = np.random.RandomState(seed + k)
    out = []
    for _ in range(N_PERM):
        pr, pc = rng.permutation(n), rng.permutation(d)
        pk = rng.permutation(k) if components else np.arange(k)
        out.append((pr, pc, pk))
    return out


def permuted(X, pr, pc):
    Xp = sp.csr_matrix(X[pr][:, pc])
    Xp.sort_indices()
    return Xp


# ------------------------------------------------------------------ metrics
def rel_dev(a, ref):
    """Largest entrywise relative deviation over the non-zero entries of
    ``ref``; an entry that is zero in ``ref`` must be zero."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    sel = ref != 0
    assert not np.any(a[~sel]), "an entry that is zero in the reference is not"
    if not sel.any():
        return 0.0
    return float(np.max(np.abs(a[sel] - ref[sel]) / np.abs(ref[sel])))


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


def check(name, got, ref, floor, metric=norm_dev, small_floor=False):
    """``got`` within MARGIN x floor of ``ref`` under ``metric``; with
    ``small_floor`` the floor itself must be at most FLOOR_MAX.  Prints the
    figures before asserting."""
    floor = max(floor, EPS64)
    dev = metric(got, ref)
    ratio = dev / floor
    print(f"{name}: floor {floor:.3e} deviation {dev:.3e} ratio {ratio:.3f}")
    record(name, floor, ratio)
    if small_floor:
        assert floor <= FLOOR_MAX, (name, "the reference itself is unstable here", floor)
    assert dev <= MARGIN * floor, (name, dev, floor, ratio)


# ------------------------------------------------------------- ratio (ops)
def host_ratio(X, P, Q):
    """``nmf_kl_ratio`` one row at a time in numpy: (num, div)."""
    n, k = X.shape[0], P.shape[1]
    num, div = np.zeros((n, k)), np.zeros(n)
    for i in range(n):
        c = X.indices[X.indptr[i]:X.indptr[i + 1]]
        x = X.data[X.indptr[i]:X.indptr[i + 1]]
        if not c.size:
            continue
        wh = Q[c] @ P[i]
        wh[wh == 0] = EPSILON
        num[i] = (x / wh) @ Q[c]
        big = x > EPSILON
        div[i] = x[big] @ np.log(x[big] / wh[big])
    return num, div


def oriented(k, transposed, seed=0):
    """(X, P, Q) of the ratio op on X or on its transpose."""
    P, Q = factors(k, seed)
    X = corpus()
    if transposed:
        Xt = sp.csr_matrix(X.T)
        Xt.sort_indices()
        return Xt, Q, P
    return X, P, Q


@functools.lru_cache(maxsize=None)
def ratio_reference(k, transposed=False, n_rows=None):
    """(num, div, floor_num, floor_div) of the numpy expression on the first
    ``n_rows`` rows."""
    X, P, Q = oriented(k, transposed)
    if n_rows is not None:
        X, P = X[:n_rows], P[:n_rows]
    num, div = host_ratio(X, P, Q)
    f_num = f_div = 0.0
    for pr, pc, pk in perms(X.shape[0], X.shape[1], k):
        nump, divp = host_ratio(permuted(X, pr, pc), P[pr][:, pk], Q[pc][:, pk])
        back_n, back_d = np.empty_like(num), np.empty_like(div)
        back_n[np.ix_(pr, pk)] = nump
        back_d[pr] = divp
        f_num = max(f_num, rel_dev(back_n, num))
        f_div = max(f_div, norm_dev(back_d, div))
    return num, div, f_num, f_div


# ------------------------------------------------------------- sweep (ops)
def host_cd(W, HHt, XHt, perm):
    """``sqh_cdnmf_update`` (one thread): (W after the sweep, violation)."""
    W = np.ascontiguousarray(W, dtype=np.float64).copy()
    HHt, XHt = np.ascontiguousarray(HHt), np.ascontiguousarray(XHt)
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    v = _host.lib().sqh_cdnmf_update(_c(W), _c(HHt), _c(XHt), _c(perm), W.shape[0], W.shape[1])
    return W, float(v)


@functools.lru_cache(maxsize=None)
def cd_problem(n, k, shuffled):
    """(W0 [n, k], HHt, XHt, perm) from the first ``n`` rows of the corpus:
    W0 holds exact zeros (the ``min(0, grad)`` branch) and, for k > 1, HHt has
    one zero on its diagonal (that coordinate is left alone)."""
    P, Q = factors(k)
    X = corpus()[:n]
    W0 = P[:n].copy()
    W0[::3, 0] = 0.0
    HHt = Q.T @ Q
    if k > 1:
        HHt[k // 2, k // 2] = 0.0
    XHt = np.asarray(X @ Q)
    perm = np.random.RandomState(5 + k).permutation(k) if shuffled else np.arange(k)
    return W0, HHt, XHt, perm.astype(np.int64)


K_ABOVE_HHT = S.CD_HHT_K + 9      # the sweep reads HHt through a uniform pointer there


def sweep_cases():
    """(k, n, shuffled): every k of ``KS`` at 1, 63, 65 and 300 rows, and a k
    above the HHt-in-LDS limit at 300 rows, each under the identity and under a
    shuffled permutation."""
    out = [(k, n, sh) for k in KS for n in (1, 63, 65, 300) for sh in (False, True)]
    return out + [(K_ABOVE_HHT, 300, False), (K_ABOVE_HHT, 300, True)]


@functools.lru_cache(maxsize=None)
def cd_reference(n, k, shuffled):
    """(W, violation, floor_W, floor_violation) of the host sweep."""
    W0, HHt, XHt, perm = cd_problem(n, k, shuffled)
    W, v = host_cd(W0, HHt, XHt, perm)
    f_w = f_v = 0.0
    for pr, _, pk in perms(n, D, k):
        inv = np.empty(k, dtype=np.int64)
        inv[pk] = np.arange(k)
        Wp, vp = host_cd(W0[pr][:, pk], HHt[np.ix_(pk, pk)], XHt[pr][:, pk], inv[perm])
        back = np.empty_like(W)
        back[np.ix_(pr, pk)] = Wp
        f_w = max(f_w, norm_dev(back, W))
        f_v = max(f_v, abs(vp - v) / abs(v) if v else abs(vp))
    return W, v, f_w, f_v


# --------------------------------------------------------------------- fits
FIT_NAMES = ("W", "H", "err", "transform")


def _quiet_fit(est, X, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = est.fit_transform(X, **kw)
        T = est.transform(X)
    return dict(W=W, H=est.components_, err=est.reconstruction_err_, transform=T,
                n_iter=est.n_iter_)


def _start(k, init, seed=0):
    """The initial (W0, H0) of a fit: the factor draw, or the host's own
    'random' draw (integer counts: its mean, and so the draw, is exact on
    every path)."""
    if init == "custom":
        P, Q = factors(k, seed)
        return P.copy(), np.ascontiguousarray(Q.T)
    return E._initialize_nmf(corpus().toarray(), k, init="random", random_state=0)


def fit(device, k, init="custom", **kw):
    """The quantities of ``NMF(k, device=device, **kw)`` fitted on the corpus."""
    X = corpus()
    if init == "custom":
        W0, H0 = _start(k, init)
        return _quiet_fit(NMF(k, init="custom", device=device, **kw), X, W=W0, H=H0)
    return _quiet_fit(NMF(k, init="random", device=device, random_state=0, **kw), X)


def _key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _fit_reference(k, init, key):
    kw = dict(key)
    X = corpus()
    base = fit(None, k, init, **kw)
    W0, H0 = _start(k, init)
    floors = dict.fromkeys(FIT_NAMES, 0.0)
    # coordinate descent visits the components in label order (or in a drawn order of labels), so
    # other labels are another sequence of updates, not the same sums in another order: the
    # labels are permuted for the multiplicative updates only
    for pr, pc, pk in perms(N, D, k, components=kw.get("solver", "cd") == "mu"):
        got = _quiet_fit(NMF(k, init="custom", **kw), permuted(X, pr, pc),
                         W=W0[pr][:, pk], H=H0[pk][:, pc])
        back = dict(err=got["err"])
        back["W"] = np.empty_like(got["W"])
        back["W"][np.ix_(pr, pk)] = got["W"]
        back["transform"] = np.empty_like(got["transform"])
        back["transform"][np.ix_(pr, pk)] = got["transform"]
        back["H"] = np.empty_like(got["H"])
        back["H"][np.ix_(pk, pc)] = got["H"]
        assert got["n_iter"] == base["n_iter"]
        for name in FIT_NAMES:
            floors[name] = max(floors[name], norm_dev(back[name], base[name]))
    if kw.get("beta_loss", "frobenius") == "frobenius":
        # the sparse identity ||X||^2 + ||WH||^2 - 2 cross cancels: its rounding error relative
        # to the residual, from the reference values
        WH = base["W"] @ base["H"]
        x2, wh2 = float(X.multiply(X).sum()), float((WH * WH).sum())
        cross = float(X.multiply(WH).sum())
        floors["err"] = max(floors["err"], EPS64 * (x2 + wh2 + 2 * abs(cross))
                            / (2 * base["err"] ** 2))
    return base, floors


def fit_reference(k, init="custom", **kw):
    """(the ``device=None`` quantities, their floors over the permuted copies)."""
    return _fit_reference(k, init, _key(kw))


def check_fit(tag, got, k, init="custom", **kw):
    base, floors = fit_reference(k, init, **kw)
    assert got["n_iter"] == base["n_iter"]
    for name in FIT_NAMES:
        assert isinstance(got[name], (np.ndarray, float))
        check(f"{tag} {name}", got[name], base[name], floors[name], small_floor=True)


# ----------------------------------------------------- the stopping criterion
def _criteria(solver, X, W, H, tol, max_iter=200):
    """The host's criterion sequence under ``tol``, from the host routines:
    (n_iter, the values it compares with ``tol``)."""
    X = X.toarray()
    seq = []
    if solver == "cd":
        Ht, W = np.array(H.T, order="C"), np.array(W, order="C")   # copies: swept in place
        XT = np.ascontiguousarray(X.T)
        for n_iter in range(1, max_iter + 1):
            v = E._cd_sweep(X, W, Ht, 0.0, 0.0, False, None)
            v += E._cd_sweep(XT, Ht, W, 0.0, 0.0, False, None)
            if n_iter == 1:
                v0 = v
            seq.append(v / v0)
            if v / v0 <= tol:
                break
        return n_iter, seq
    W, H = W.copy(), H.copy()
    err0 = prev = E._beta_divergence(X, W, H, 1, square_root=True)
    for n_iter in range(1, max_iter + 1):
        W *= E._mu_w(X, W, H, 1, 0.0, 0.0, 1.0, None, None, None, True)[0]
        H *= E._mu_h(X, W, H, 1, 0.0, 0.0, 1.0)
        H[H < EPS64] = 0.0
        if n_iter % 10 == 0:
            err = E._beta_divergence(X, W, H, 1, square_root=True)
            seq.append((prev - err) / err0)
            if seq[-1] < tol:
                break
            prev = err
    return n_iter, seq


@functools.lru_cache(maxsize=None)
def criterion_reference(solver, k, tol=1e-4):
    """(n_iter, margin, floor): the host's iteration count under ``tol``
    (solver 'cd', or 'mu' with the Kullback-Leibler loss), the closest its
    criterion comes to ``tol`` relative to ``tol``, and the criterion's largest
    relative deviation over the permuted copies."""
    X = corpus()
    W0, H0 = _start(k, "custom")
    n_iter, seq = _criteria(solver, X, W0, H0, tol)
    margin = min(abs(c - tol) / tol for c in seq)
    floor = 0.0
    for pr, pc, pk in perms(N, D, k, components=solver == "mu"):
        n_p, seq_p = _criteria(solver, permuted(X, pr, pc), W0[pr][:, pk], H0[pk][:, pc], tol)
        assert n_p == n_iter
        floor = max(floor, max(abs(a - b) / abs(b) for a, b in zip(seq_p, seq)))
    floor = max(floor, EPS64)
    # margin / floor: how many floors the criterion stays away from tol (at least MARGIN)
    record(f"criterion {solver} k={k} tol={tol:g} n_iter={n_iter} margin={margin:.3e}", floor,
           margin / floor)
    return n_iter, margin, floor


# ------------------------------------------------------------ estimator cases
SOLVERS = (("cd", "frobenius"), ("mu", "frobenius"), ("mu", "kullback-leibler"))


def fit_cases():
    """(id, k, init, estimator parameters) of the fit-level comparisons: all
    with ``tol=0``, so every path runs ``max_iter`` iterations."""
    out = []
    for solver, loss in SOLVERS:
        kw = dict(solver=solver, beta_loss=loss, tol=0.0)
        tag = f"{solver}-{loss[:4]}"
        for k, it in ((5, 5), (70, 5), (5, 20)):
            out.append((f"{tag}-k{k}-it{it}", k, "custom", dict(kw, max_iter=it)))
        out.append((f"{tag}-reg", 5, "custom", dict(kw, max_iter=5, alpha=0.1, l1_ratio=0.5)))
        out.append((f"{tag}-random", 5, "random", dict(kw, max_iter=5)))
    out.append(("cd-shuffle", 5, "custom", dict(solver="cd", tol=0.0, max_iter=5, shuffle=True,
                                                random_state=0)))
    return out


def dense_problem():
    """A 60 x 40 dense matrix of counts with its start (W0, H0) at k = 4."""
    rng = np.random.RandomState(3)
    X = (rng.rand(60, 40) < 0.3) * rng.randint(1, 6, (60, 40)).astype(np.float64)
    return X, 0.3 * np.abs(rng.randn(60, 4)), 0.3 * np.abs(rng.randn(4, 40))


def dense_fit(device, solver, loss, X=None, W0=None, H0=None):
    """The quantities of a 5-iteration fit of the dense problem (or of the
    given permuted copy of it)."""
    if X is None:
        X, W0, H0 = dense_problem()
    est = NMF(4, init="custom", solver=solver, beta_loss=loss, tol=0.0, max_iter=5,
              device=device)
    return _quiet_fit(est, X, W=W0.copy(), H=H0.copy())


@functools.lru_cache(maxsize=None)
def dense_reference(solver, loss):
    """(the ``device=None`` quantities of the dense problem, their floors over
    the permuted copies): the labels are permuted for solver 'mu' only.  The
    ``err`` floor has no cancellation clamp here: on dense input both paths
    subtract ``W H`` from X directly."""
    X, W0, H0 = dense_problem()
    n, d = X.shape
    k = W0.shape[1]
    base = dense_fit(None, solver, loss)
    floors = dict.fromkeys(FIT_NAMES, 0.0)
    for pr, pc, pk in perms(n, d, k, components=solver == "mu"):
        got = dense_fit(None, solver, loss, X[pr][:, pc], W0[pr][:, pk], H0[pk][:, pc])
        assert got["n_iter"] == base["n_iter"]
        back = dict(err=got["err"])
        for name, ix in (("W", (pr, pk)), ("transform", (pr, pk)), ("H", (pk, pc))):
            back[name] = np.empty_like(got[name])
            back[name][np.ix_(*ix)] = got[name]
        for name in FIT_NAMES:
            floors[name] = max(floors[name], norm_dev(back[name], base[name]))
    return base, floors


def check_dense(tag, got, solver, loss):
    base, floors = dense_reference(solver, loss)
    assert got["n_iter"] == base["n_iter"] == 5
    for name in FIT_NAMES:
        check(f"{tag} {name}", got[name], base[name], floors[name], small_floor=True)
