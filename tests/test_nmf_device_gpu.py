"""Device NMF on the GPU: the kernels of ``csrc/spnmf.hip`` against the fp64
torch twins, the numpy ratio expression and the host sweep
``sqh_cdnmf_update``, and ``NMF(device="cuda")`` against the host path
(``device=None``).

Tolerances are measured, not fixed (``_nmf_data.py``): 64 x the reference's
own largest deviation over 4 permuted copies of the problem.  One wave owns an
output row of the ratio kernel and one lane a row of the sweep, so their
results are compared bit for bit between runs and between ways of splitting
the rows."""
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _nmf_data as D
from sq_learn_amd.base import clone
from sq_learn_amd.decomposition import NMF, non_negative_factorization
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.ops import _native as nat
from sq_learn_amd.ops import sparse_nmf as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = D.fit_cases()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _t(a, device=DEV):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------ bindings, constants
def test_bindings_match_their_table():
    """The bindings of ``_C.nmf`` against ``golden/native_formats_nmf.json``,
    as ``test_native_api_gpu.py`` checks those of ``_C`` against its table."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "native_formats_nmf.json")) as f:
        formats = json.load(f)
    m = nat.native().nmf
    names = {n for n in dir(m) if not n.startswith("_") and callable(getattr(m, n))}
    assert names == set(formats)
    for name, fmt in formats.items():
        head, sep, got = getattr(m, name).__doc__.rpartition("\n\nargs: ")
        assert sep and head and got == fmt, (name, got)
    with pytest.raises(TypeError):
        m.sp_nmf_kl(0)
    with pytest.raises(TypeError):
        m.nmf_cd_sweep(0, 0)


def test_exported_constants():
    m = nat.native().nmf
    assert m.sp_nmf_stage() == S.STAGE and m.sp_nmf_stage_min_row() == S.STAGE_MIN_ROW
    assert m.sp_nmf_max_k() == S.KL_MAX_K >= 1024
    assert m.nmf_cd_max_k() == S.CD_MAX_K >= 512
    assert m.nmf_cd_hht_k() == S.CD_HHT_K
    assert S.stage_entries(70) == m.sp_nmf_stage() // 71
    assert S.stage_entries(1) == m.sp_nmf_stage() // m.sp_nmf_stage_min_row()
    # the corpus holds a staged and an unstaged row at every k
    lens = np.diff(D.corpus().indptr)
    for k in D.KS:
        assert 1 <= S.stage_entries(k) < lens[D.long_row(k)] <= D.D - 1
        assert m.sp_nmf_wpb(k) == 4
    assert m.sp_nmf_wpb(0) == 0 and m.nmf_cd_rows(S.CD_MAX_K + 1) == 0


# -------------------------------------------------------------------- ratio
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("k", D.KS)
def test_ratio_kernel(k, transposed):
    """Four waves per workgroup; the rows up to ``stage_entries(k)`` entries
    take the staged branch, the longer ones the re-gather branch: X holds both
    kinds at every k (``long_row(k)``), its transpose at k >= 64."""
    X, P, Q = D.oriented(k, transposed)
    lens = np.diff(X.indptr)
    if not transposed or k >= 64:
        assert (lens[lens > 0] <= S.stage_entries(k)).any() and (lens > S.stage_entries(k)).any()
    num, div, f_num, f_div = D.ratio_reference(k, transposed)
    sd = as_sparse_data(X, DEV)
    gn, gd = S.nmf_kl_ratio(sd, _t(P), _t(Q), want_div=True)
    assert gn.device.type == DEV and gd.device.type == DEV
    tn, td = S.nmf_kl_ratio(as_sparse_data(X, "cpu"), _t(P, "cpu"), _t(Q, "cpu"), want_div=True)
    tag = f"gpu ratio{'T' if transposed else ''} k={k}"
    D.check(f"{tag} num vs twin", gn.cpu().numpy(), tn.numpy(), f_num, D.rel_dev)
    D.check(f"{tag} num vs numpy", gn.cpu().numpy(), num, f_num, D.rel_dev)
    D.check(f"{tag} div vs twin", gd.cpu().numpy(), td.numpy(), f_div)
    D.check(f"{tag} div vs numpy", gd.cpu().numpy(), div, f_div)
    # without div (the other template instance): the same num, bit for bit
    only_num, none = S.nmf_kl_ratio(sd, _t(P), _t(Q))
    assert none is None and torch.equal(only_num, gn)
    none, only_div = S.nmf_kl_ratio(sd, _t(P), _t(Q), want_num=False, want_div=True)
    assert none is None and torch.equal(only_div, gd)
    # two runs, and one call against two calls over row ranges: the same bits
    gn2, gd2 = S.nmf_kl_ratio(sd, _t(P), _t(Q), want_div=True)
    assert torch.equal(gn2, gn) and torch.equal(gd2, gd)
    cut = 101
    an, ad = S.nmf_kl_ratio(sd, _t(P), _t(Q), want_div=True, rows=(0, cut))
    bn, bd = S.nmf_kl_ratio(sd, _t(P), _t(Q), want_div=True, rows=(cut, X.shape[0]))
    assert torch.equal(torch.cat([an, bn]), gn) and torch.equal(torch.cat([ad, bd]), gd)
    if not transposed:
        assert not gn[D.ROW_EMPTY].any() and gd[D.ROW_EMPTY] == 0


@pytest.mark.parametrize("k", [500, 600])
def test_ratio_many_components(k):
    """The first 13 rows at k = 500 (four waves per workgroup on 8 component
    tiles: all of the 65 536 bytes of LDS a workgroup may take) and at
    k = 600 (two waves, 10 tiles).  No row is staged - every row is empty or
    longer than ``stage_entries(k)``."""
    n = 13
    m = nat.native().nmf
    assert m.sp_nmf_wpb(k) == (4 if k == 500 else 2) and m.sp_nmf_wpb(512) == 4
    assert m.sp_nmf_wpb(513) == 2
    X = D.corpus()[:n]
    lens = np.diff(X.indptr)
    assert S.stage_entries(k) == m.sp_nmf_stage() // (k | 1) <= 2
    assert ((lens == 0) | (lens > S.stage_entries(k))).all() and (lens == 0).any()
    rng = np.random.RandomState(1000 + k)
    P, Q = 0.3 * np.abs(rng.randn(n, k)), 0.3 * np.abs(rng.randn(D.D, k))
    P[D.ROW_ZERO_P] = 0.0
    num, div = D.host_ratio(X, P, Q)
    f_num = f_div = 0.0
    for pr, pc, pk in D.perms(n, D.D, k):
        nump, divp = D.host_ratio(D.permuted(X, pr, pc), P[pr][:, pk], Q[pc][:, pk])
        back_n, back_d = np.empty_like(num), np.empty_like(div)
        back_n[np.ix_(pr, pk)] = nump
        back_d[pr] = divp
        f_num = max(f_num, D.rel_dev(back_n, num))
        f_div = max(f_div, D.norm_dev(back_d, div))
    gn, gd = S.nmf_kl_ratio(as_sparse_data(X, DEV), _t(P), _t(Q), want_div=True)
    D.check(f"gpu ratio k={k} num", gn.cpu().numpy(), num, f_num, D.rel_dev)
    D.check(f"gpu ratio k={k} div", gd.cpu().numpy(), div, f_div)


# -------------------------------------------------------------------- sweep
@pytest.mark.parametrize("k,n,shuffled", D.sweep_cases())
def test_sweep_kernel(k, n, shuffled):
    """Up to ``nmf_cd_hht_k`` components HHt sits in LDS, above (70, 73, 130)
    it is read through a uniform pointer; 64 rows per wave up to k = 73 and 62
    at k = 130, so n = 65 and n = 300 (and n = 63 at k = 130) run a second,
    partly filled tile."""
    m = nat.native().nmf
    assert m.nmf_cd_rows(k) == (62 if k == 130 else 64)
    assert (k <= m.nmf_cd_hht_k()) == (k in (1, 5, 64))
    W0, HHt, XHt, perm = D.cd_problem(n, k, shuffled)
    W, v, f_w, f_v = D.cd_reference(n, k, shuffled)
    got = _t(W0.copy())
    gv = S.nmf_cd_sweep(got, _t(HHt), _t(XHt), _t(perm))
    assert gv.dim() == 0 and gv.device.type == DEV
    twin = _t(W0.copy(), "cpu")
    tv = S.nmf_cd_sweep(twin, _t(HHt, "cpu"), _t(XHt, "cpu"), _t(perm, "cpu"))
    tag = f"gpu sweep k={k} n={n} {'shuffled' if shuffled else 'identity'}"
    D.check(f"{tag} W vs host", got.cpu().numpy(), W, f_w, small_floor=True)
    D.check(f"{tag} W vs twin", got.cpu().numpy(), twin.numpy(), f_w, small_floor=True)
    D.check(f"{tag} violation vs host", float(gv), v, f_v, small_floor=True)
    D.check(f"{tag} violation vs twin", float(gv), float(tv), f_v, small_floor=True)
    if k > 1:
        np.testing.assert_array_equal(got.cpu().numpy()[:, k // 2], W0[:, k // 2])   # zero Hessian
    again = _t(W0.copy())
    gv2 = S.nmf_cd_sweep(again, _t(HHt), _t(XHt), _t(perm))
    assert torch.equal(again, got) and torch.equal(gv2, gv)
    if n > 5:
        # two calls over row ranges that cut a tile: the same W, bit for bit
        split = _t(W0.copy())
        cut = n // 2 + 1
        va = S.nmf_cd_sweep(split, _t(HHt), _t(XHt), _t(perm), rows=(0, cut))
        vb = S.nmf_cd_sweep(split, _t(HHt), _t(XHt), _t(perm), rows=(cut, n))
        assert torch.equal(split, got)
        D.check(f"{tag} violation of two calls", float(va + vb), float(gv), f_v, small_floor=True)


def test_sweep_many_components():
    """k = 600: fewer than 64 rows per wave (the two tiles no longer fit), so
    the lanes past ``nmf_cd_rows(k)`` idle and 40 rows take several tiles."""
    k, n = 600, 40
    R = nat.native().nmf.nmf_cd_rows(k)
    assert 1 <= R < n
    rng = np.random.RandomState(1000 + k)
    Q = 0.3 * np.abs(rng.randn(D.D, k))
    W0 = 0.3 * np.abs(rng.randn(n, k))
    W0[::3, 0] = 0.0
    HHt, XHt = Q.T @ Q, np.asarray(D.corpus()[:n] @ Q)
    perm = rng.permutation(k).astype(np.int64)
    W, v = D.host_cd(W0, HHt, XHt, perm)
    f_w = f_v = 0.0
    for pr, _, pk in D.perms(n, D.D, k):
        inv = np.empty(k, dtype=np.int64)
        inv[pk] = np.arange(k)
        Wp, vp = D.host_cd(W0[pr][:, pk], HHt[np.ix_(pk, pk)], XHt[pr][:, pk], inv[perm])
        back = np.empty_like(W)
        back[np.ix_(pr, pk)] = Wp
        f_w, f_v = max(f_w, D.norm_dev(back, W)), max(f_v, abs(vp - v) / abs(v))
    got = _t(W0.copy())
    gv = S.nmf_cd_sweep(got, _t(HHt), _t(XHt), _t(perm))
    D.check("gpu sweep k=600 W", got.cpu().numpy(), W, f_w, small_floor=True)
    D.check("gpu sweep k=600 violation", float(gv), v, f_v, small_floor=True)


def test_launchers_refuse_bad_arguments():
    sd = as_sparse_data(D.corpus(), DEV)
    P, Q = (_t(a) for a in D.factors(5))
    m = nat.native().nmf
    out = torch.empty((D.N, 5), dtype=torch.float64, device=DEV)
    ptrs = (sd.indptr.data_ptr(), sd.indices.data_ptr(), sd.data.data_ptr())
    for k, eps, num in ((0, 1e-7, out.data_ptr()), (S.KL_MAX_K + 1, 1e-7, out.data_ptr()),
                        (5, 0.0, out.data_ptr()), (5, 1e-7, 0)):
        with pytest.raises(RuntimeError, match="invalid"):
            m.sp_nmf_kl(*ptrs, P.data_ptr(), Q.data_ptr(), 0, D.N, D.D, k, eps, num, 0,
                        nat.stream_handle(sd.device))
    for bad in (0, 3, 4):      # a null indptr, P or Q
        args = list(ptrs) + [P.data_ptr(), Q.data_ptr()]
        args[bad] = 0
        with pytest.raises(RuntimeError, match="invalid"):
            m.sp_nmf_kl(*args, 0, D.N, D.D, 5, 1e-7, out.data_ptr(), 0,
                        nat.stream_handle(sd.device))
    with pytest.raises(RuntimeError, match="invalid"):
        m.nmf_cd_sweep(P.data_ptr(), 0, 0, 0, 0, D.N, 5, 0, 0, nat.stream_handle(sd.device))
    with pytest.raises(ValueError):
        S.nmf_kl_ratio(sd, P, Q, want_num=False)
    with pytest.raises(ValueError):
        S.nmf_kl_ratio(sd, P, Q, rows=(5, D.N + 1))


# ---------------------------------------------------------------- estimator
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_estimator_follows_the_host_path(case):
    tag, k, init, kw = case
    D.check_fit(f"gpu fit {tag}", D.fit(DEV, k, init, **kw), k, init, **kw)


@pytest.mark.parametrize("solver", ["cd", "mu"])
def test_n_iter_under_the_default_tol(solver):
    k = 5
    n_iter, margin, floor = D.criterion_reference(solver, k)
    print(f"{solver}: n_iter {n_iter} margin {margin:.3e} floor {floor:.3e}")
    assert 1 < n_iter < 200
    assert margin > D.MARGIN * floor, "the criterion comes too close to tol: choose another seed"
    kw = dict(solver=solver, beta_loss="frobenius" if solver == "cd" else "kullback-leibler")
    got = D.fit(DEV, k, **kw)
    base = D.fit(None, k, **kw)
    assert got["n_iter"] == base["n_iter"] == n_iter


@pytest.mark.parametrize("solver,loss", D.SOLVERS)
def test_dense_input(solver, loss):
    """60 x 40 dense counts, k = 4, 5 iterations, against ``device=None`` within
    64 x the floor of that problem's own permuted host runs."""
    D.check_dense(f"gpu dense {solver}-{loss[:4]}", D.dense_fit(DEV, solver, loss), solver, loss)


def test_function_pickle_and_clone():
    X = D.corpus()
    P, Q = D.factors(5)
    kw = dict(init="custom", solver="mu", beta_loss="kullback-leibler", tol=0.0, max_iter=3)
    W, H, n_iter = non_negative_factorization(X, W=P.copy(), H=Q.T.copy(), n_components=5,
                                              device=DEV, **kw)
    est = NMF(5, device=DEV, **kw)
    We = est.fit_transform(X, W=P.copy(), H=Q.T.copy())
    np.testing.assert_array_equal(W, We)
    np.testing.assert_array_equal(H, est.components_)
    assert n_iter == est.n_iter_ == 3
    assert isinstance(est.components_, np.ndarray) and isinstance(est.reconstruction_err_, float)
    assert est.n_components_ == 5 and est.n_features_in_ == D.D
    a = NMF(5, init="random", random_state=0, max_iter=3, device=DEV).fit(X)
    b = pickle.loads(pickle.dumps(a))
    c = clone(a)
    assert b.device == DEV and c.device == DEV and not hasattr(c, "components_")
    np.testing.assert_array_equal(b.transform(X), a.transform(X))
    np.testing.assert_array_equal(c.fit(X).components_, a.components_)
    np.testing.assert_array_equal(NMF(5, init="random", random_state=0, max_iter=3,
                                      device="cuda:0").fit(X.tocsc()).components_, a.components_)


def test_refusals():
    X = D.corpus()
    for loss in (1.5, "itakura-saito"):
        with pytest.raises(ValueError, match="with a device supports"):
            NMF(5, solver="mu", beta_loss=loss, init="random", device=DEV).fit(X)
    with pytest.raises(ValueError, match=f"1 to {S.CD_MAX_K} components"):
        NMF(S.CD_MAX_K + 1, init="random", device=DEV).fit(X)
    with pytest.raises(ValueError, match=f"1 to {S.KL_MAX_K} components"):
        NMF(S.KL_MAX_K + 1, solver="mu", beta_loss="kullback-leibler", init="random",
            device=DEV).fit(X)
    Xn = X.copy()
    Xn.data[3] = -1.0
    with pytest.raises(ValueError, match="Negative values"):
        NMF(5, init="random", device=DEV).fit(Xn)
