"""CSR sparse-times-dense kernels (``csrc/spmm.hip``) against their fp64
torch twins, and TruncatedSVD on sparse rows on the GPU.

One sparsity structure (n = 2000, d = 1000, about 20 nonzeros per row; rows
0..8 hold exactly 0, 1, 3, 4, 5, 63, 64, 65 and 300 nonzeros - both sides of
the 64-wide load and of the 4-wide unroll - row 9 starts with an explicitly
stored zero, row 10 uses the last column, column 998 is empty) carries two
value sets:

* exact: integer values in [-8, 8] and dense operands that are multiples of
  1/8, so every fp64 product and sum is exact in any order and the GPU must
  match the twin bit for bit at every ``l`` and ``seg``;
* random: fp32-rounded normal values, checked against the dot-product bound
  ``(nnz_row + 2) * 2^-53 * sum |v| |B|`` with the row's own count.

``X`` is that structure (``sp_xw`` meets the forced row lengths: at
``seg = 64`` the 65 and 300 rows split into 2 and 5 segments).  ``XD`` is the
same with column 7 made dense (a nonzero in every row), so ``sp_xty`` meets a
transposed row of 2000 nonzeros: 2 segments at the default ``seg`` of 1024,
32 at ``seg = 64``.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _sparse_svd_data import TOPICS, planted_topics
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.models.cluster import qMeans_
from sq_learn_amd.models.decomposition import TruncatedSVD
from sq_learn_amd.ops import _native as nat
from sq_learn_amd.ops import sparse_linalg as SL
from sq_learn_amd.preprocessing import Normalizer

pytestmark = pytest.mark.gpu

SEED = 4242
N, D = 2000, 1000
FORCED = [0, 1, 3, 4, 5, 63, 64, 65, 300]
DENSE_COL, EMPTY_COL = 7, D - 2
U = 2.0 ** -53
WIDE = 300                     # above the 256 columns one pass covers
LS = [1, 7, 64, 65, 130, WIDE]
SEGS = [None, 64]


def _matrix(kind, dense_col):
    rng = np.random.RandomState(SEED)
    counts = rng.randint(10, 31, size=N)
    counts[:len(FORCED)] = FORCED
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    # columns 0 .. D - 3; D - 2 stays empty, D - 1 is set below
    indices = np.concatenate([np.sort(rng.choice(D - 2, size=c, replace=False)) for c in counts])
    indices[indptr[11] - 1] = D - 1           # row 10 uses the last column
    nnz = len(indices)
    if kind == "exact":
        v = rng.randint(1, 9, size=nnz) * rng.choice([-1.0, 1.0], size=nnz)
    else:
        v = rng.standard_normal(nnz).astype(np.float32).astype(np.float64)
    v[indptr[9]] = 0.0                        # row 9: an explicitly stored zero
    A = sp.csr_matrix((v, indices.astype(np.int32), indptr), shape=(N, D))
    if dense_col:
        A = A.tolil()
        col = rng.randint(1, 9, size=N).astype(np.float64) if kind == "exact" else \
            rng.standard_normal(N).astype(np.float32).astype(np.float64)
        A[:, DENSE_COL] = col.reshape(-1, 1)
        A = A.tocsr()
        A.sort_indices()
    return A


def _operand(kind, rows, l):
    rng = np.random.RandomState(SEED + 31 * l + rows)
    if kind == "exact":
        return torch.as_tensor(rng.randint(-16, 17, size=(rows, l)) / 8.0)
    return torch.as_tensor(rng.standard_normal((rows, l)))


class Case:
    """One matrix on both devices; twin products computed once per l."""

    def __init__(self, kind, dense_col, dev):
        self.kind = kind
        self.A = _matrix(kind, dense_col)
        self.cpu = as_sparse_data(self.A, device="cpu")
        self.gpu = as_sparse_data(self.A, device=dev)
        self.absA = abs(self.A).tocsr()
        self._xw, self._xty = {}, {}

    def xw(self, l):
        if l not in self._xw:
            W = _operand(self.kind, D, l)
            bound = (np.diff(self.A.indptr)[:, None] + 2) * U * (self.absA @ W.abs().numpy())
            self._xw[l] = (W, SL.sp_xw_torch(self.cpu, W), bound)
        return self._xw[l]

    def xty(self, l):
        if l not in self._xty:
            Y = _operand(self.kind, N, l)
            At = self.absA.T.tocsr()
            bound = (np.diff(At.indptr)[:, None] + 2) * U * (At @ Y.abs().numpy())
            self._xty[l] = (Y, SL.sp_xty_torch(self.cpu, Y), bound)
        return self._xty[l]


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind, dense_col):
        if (kind, dense_col) not in store:
            store[(kind, dense_col)] = Case(kind, dense_col, cuda)
        return store[(kind, dense_col)]
    return get


def test_fixture_structure(cases):
    X, XD = cases("random", False), cases("random", True)
    cnt = np.diff(X.A.indptr)
    assert cnt[:len(FORCED)].tolist() == FORCED and X.A.data[X.A.indptr[9]] == 0.0
    assert X.A.indices[X.A.indptr[11] - 1] == D - 1
    colcnt = np.diff(XD.A.T.tocsr().indptr)
    assert colcnt[DENSE_COL] == N and colcnt[EMPTY_COL] == 0
    assert nat.native().spmm_tile_cols() < WIDE
    tab = SL.segments(X.gpu, 64)
    assert tab.nlong == 2 and tab.slots == 2 + 5
    tt = SL.segments(SL.csr_transpose(XD.gpu), 64)
    assert tt.nlong >= 1 and int((tt.long_ptr[1:] - tt.long_ptr[:-1]).max()) == 32
    assert SL.segments(SL.csr_transpose(XD.gpu)).slots == 2


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("l", LS)
def test_xw_exact(cases, l, seg):
    c = cases("exact", False)
    W, twin, _ = c.xw(l)
    got = SL.sp_xw(c.gpu, W, seg=seg)
    assert got.dtype == torch.float64 and got.shape == (N, l)
    assert torch.equal(got.cpu(), twin)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("l", LS)
def test_xty_exact(cases, l, seg):
    c = cases("exact", True)
    Y, twin, _ = c.xty(l)
    got = SL.sp_xty(c.gpu, Y, seg=seg)
    assert got.shape == (D, l)
    assert torch.equal(got.cpu(), twin)
    assert (got[EMPTY_COL] == 0).all()


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("l", LS)
def test_xw_random(cases, l, seg):
    c = cases("random", False)
    W, twin, bound = c.xw(l)
    # preallocated with NaN, row stride wider than l
    out = torch.full((N, l + 5), float("nan"), dtype=torch.float64, device=c.gpu.device)
    got = SL.sp_xw(c.gpu, W, out=out, seg=seg)
    assert got.data_ptr() == out.data_ptr() and got.shape == (N, l)
    assert torch.isfinite(out[:, :l]).all() and torch.isnan(out[:, l:]).all()
    assert (out[0, :l] == 0).all()                                   # the empty row
    err = (got.cpu() - twin).abs().numpy()
    assert (err <= bound).all(), float((err - bound).max())
    again = SL.sp_xw(c.gpu, W, seg=seg)
    assert torch.equal(again, got)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("l", LS)
def test_xty_random(cases, l, seg):
    c = cases("random", True)
    Y, twin, bound = c.xty(l)
    got = SL.sp_xty(c.gpu, Y, seg=seg)
    assert torch.isfinite(got).all()
    err = (got.cpu() - twin).abs().numpy()
    assert (err <= bound).all(), float((err - bound).max())
    assert torch.equal(SL.sp_xty(c.gpu, Y, seg=seg), got)


def test_power_iter_matches_two_products(cases):
    c = cases("exact", True)
    W, _, _ = c.xw(7)
    got = SL.sp_power_iter(c.gpu, W)
    assert torch.equal(got.cpu(), SL.sp_power_iter(c.cpu, W))


def test_transpose_matches_scipy(cases):
    c = cases("random", True)
    t = SL.csr_transpose(c.gpu)
    ref = c.A.T.tocsr()
    ref.sort_indices()
    assert t.shape == (D, N) and t.indices.dtype == torch.int32 and t.data.dtype == torch.float32
    np.testing.assert_array_equal(t.indptr.cpu().numpy(), ref.indptr)
    np.testing.assert_array_equal(t.indices.cpu().numpy(), ref.indices)
    np.testing.assert_array_equal(t.data.cpu().numpy().astype(np.float64), ref.data)


def test_col_moments(cases):
    c = cases("random", True)
    s, ss = SL.sp_col_moments(c.gpu)
    s2, ss2 = SL.sp_col_moments(c.gpu)
    assert torch.equal(s, s2) and torch.equal(ss, ss2)
    csc = c.A.tocsc()
    cnt = np.diff(csc.indptr)
    ref_s = np.asarray(csc.sum(axis=0)).ravel()
    ref_ss = np.asarray(csc.multiply(csc).sum(axis=0)).ravel()
    b_s = (cnt + 2) * U * np.asarray(abs(csc).sum(axis=0)).ravel()
    b_ss = (cnt + 2) * U * ref_ss
    assert (np.abs(s.cpu().numpy() - ref_s) <= b_s).all()
    assert (np.abs(ss.cpu().numpy() - ref_ss) <= b_ss).all()
    assert s[EMPTY_COL] == 0 and ss[EMPTY_COL] == 0


def test_truncated_svd_gpu_matches_cpu(cuda):
    """Planted-topic fixture (fp32 values on both sides), sparse branch on both
    devices: the sums are fp64 on both, so the project's 1e-9 parity
    tolerance applies (the CPU sparse-against-dense gap is 2e-15)."""
    X = planted_topics()
    kw = dict(n_components=TOPICS, n_iter=5, random_state=0)
    cpu = TruncatedSVD(device="cpu", **kw)
    Tc = cpu.fit_transform(X)
    gpu = TruncatedSVD(device="cuda", **kw)
    Tg = gpu.fit_transform(X)
    assert isinstance(Tg, np.ndarray) and Tg.dtype == np.float64
    np.testing.assert_allclose(gpu.singular_values_, cpu.singular_values_, rtol=1e-9)
    np.testing.assert_allclose(gpu.components_, cpu.components_, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gpu.explained_variance_ratio_, cpu.explained_variance_ratio_,
                               rtol=1e-9)
    np.testing.assert_allclose(Tg, Tc, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gpu.transform(X), Tg, rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="expecting 2000 features"):
        gpu.transform(X[:, :1999])


def test_lsa_to_qmeans_recovers_planted_groups(cuda):
    from sq_learn_amd.feature_extraction.text import TfidfVectorizer
    rng = np.random.RandomState(0)
    vocab = [[f"{p}{i}" for i in range(1000)] for p in ("ax", "bx")]
    n_docs = 2100                                    # 2100 x 2000 > 4e6: the sparse branch
    docs = [" ".join(rng.choice(vocab[i % 2], size=12)) for i in range(n_docs)]
    truth = np.arange(n_docs) % 2
    X = TfidfVectorizer().fit_transform(docs)
    assert sp.issparse(X) and X.shape[0] * X.shape[1] > 4e6
    T = TruncatedSVD(2, random_state=0, device="cuda").fit_transform(X)
    Z = Normalizer().fit_transform(T)
    q = qMeans_(2, n_init=1, delta=0.05, true_distance_estimate=False, random_state=0,
                device="cuda").fit(Z)
    labels = np.asarray(q.labels_)
    assert max(np.mean(labels == truth), np.mean(labels == 1 - truth)) == 1.0
