"""CSR sparse k-means / q-means kernels (``csrc/spkmeans.hip``) against their
fp64 torch twins.

Two fixtures share one sparsity structure (n = 2000, d = 1000, about 20
nonzeros per row; rows 0..7 hold exactly 0, 1, 3, 4, 5, 63, 64, 65 nonzeros -
both sides of the 64-wide load and of the 4-wide unroll - row 8 holds 300,
row 9 an explicitly stored zero, row 10 uses the last column):

* random: fp32-rounded normal values (seed ``SEED``), centres a common
  offset plus small perturbations so the delta band has several members;
* exact: integer values in [-8, 8] and centres that are multiples of 1/8, so
  every fp64 product and sum is exact in any order and the GPU must match the
  twin bit for bit.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.models.cluster import KMeans, QMeans
from sq_learn_amd.models.cluster import _sparse
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import sparse_kmeans as S
from sq_learn_amd.runtime.rng import RngKey

pytestmark = pytest.mark.gpu

SEED = 20240   # random fixture: the band-edge precondition holds (checked on the CPU twin)
N, D = 2000, 1000
FORCED = [0, 1, 3, 4, 5, 63, 64, 65, 300]
U = 2.0 ** -53


def _structure():
    rng = np.random.RandomState(SEED)
    counts = rng.randint(10, 31, size=N)
    counts[:len(FORCED)] = FORCED
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(D, size=c, replace=False)) for c in counts])
    lo = indptr[10]
    indices[indptr[11] - 1] = D - 1          # row 10 uses the last column
    assert indices[indptr[11] - 2] < D - 1 and lo < indptr[11]
    return rng, indptr, indices.astype(np.int32)


def _matrix(kind):
    rng, indptr, indices = _structure()
    nnz = len(indices)
    if kind == "exact":
        v = rng.randint(1, 9, size=nnz) * rng.choice([-1.0, 1.0], size=nnz)
    else:
        v = rng.standard_normal(nnz).astype(np.float32).astype(np.float64)
    v[indptr[9]] = 0.0                        # row 9: an explicitly stored zero
    return sp.csr_matrix((v, indices, indptr), shape=(N, D))


def _centres(kind, k):
    rng = np.random.RandomState(SEED + k)
    if kind == "exact":
        C = rng.randint(-4, 5, size=(k, D)) / 8.0
        if k >= 3:
            C[k - 1] = C[0]                   # exact ties: the band rule at delta = 0
        return torch.as_tensor(C)
    return torch.as_tensor(0.3 * rng.standard_normal((1, D)) + 0.02 * rng.standard_normal((k, D)))


class Case:
    """One fixture on both devices, twin results computed once per (k, delta)."""

    def __init__(self, kind, n, dev):
        self.kind = kind
        self.X = _matrix(kind)[:n]
        self.cpu = as_sparse_data(self.X, device="cpu")
        self.gpu = as_sparse_data(self.X, device=dev)
        self.xn = S.sp_row_norms_torch(self.cpu)
        self.nnz_max = int(np.diff(self.X.indptr).max())
        self._twin = {}

    def operand(self, C):
        """GPU operand with the twin's centre norms (the bound below is the
        dot products' alone)."""
        CT, _ = S.center_operand(C.to(self.gpu.device))
        return CT, (C * C).sum(1).to(self.gpu.device)

    def twin(self, k, delta, key):
        if (k, delta) not in self._twin:
            C = _centres(self.kind, k)
            lab, mind, inertia = S.sp_estep_torch(self.cpu, C, delta, key, 0, xn=self.xn)
            Dm = S.sp_sqdist(self.cpu, C, xn=self.xn)
            self._twin[(k, delta)] = (C, lab, mind, inertia, Dm)
        return self._twin[(k, delta)]


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind, n=N):
        if (kind, n) not in store:
            store[(kind, n)] = Case(kind, n, cuda)
        return store[(kind, n)]
    return get


KEY = RngKey(11, "band_select", (2 << 24) | 5)


def _band_edge_clear(case, C, Dm, delta):
    """Precondition of label equality: no (row, centre) pair of the twin's
    distances within 1e-9 (xn + cn) of the row's band edge (at delta = 0 the
    minimum itself defines the edge)."""
    cn = (C * C).sum(1)
    mn, am = Dm.min(1)
    gap = (Dm - (mn + delta)[:, None]).abs()
    if delta == 0:
        gap[torch.arange(Dm.shape[0]), am] = float("inf")
    return bool((gap > 1e-9 * (case.xn[:, None] + cn[None, :])).all())


def _check_estep(case, k, delta):
    C, lab, mind, inertia, Dm = case.twin(k, delta, KEY)
    dev = case.gpu.device
    op = case.operand(C)
    xn = case.xn.to(dev)
    glab, gmind, ginertia = S.sp_estep(case.gpu, C.to(dev), delta, KEY, 0, xn=xn, operand=op)
    gD = S.sp_sqdist(case.gpu, C.to(dev), xn=xn, operand=op)
    assert glab.dtype == torch.int32 and gmind.dtype == torch.float64
    if case.kind == "exact":
        assert torch.equal(gD.cpu(), Dm)
        assert torch.equal(glab.cpu().long(), lab)
        assert torch.equal(gmind.cpu(), mind)
        assert torch.equal(ginertia.cpu(), inertia)
        if 3 <= k <= 1030:   # both copies of the duplicated centre get picked
            assert bool((lab == k - 1).any()) and bool((lab == 0).any())
        return
    cn = (C * C).sum(1)
    bound = 4.0 * (case.nnz_max + 4) * U * (case.xn[:, None] + cn[None, :])
    assert bool(((gD.cpu() - Dm).abs() <= bound).all())
    assert bool(((gmind.cpu() - mind).abs() <= bound.max(1).values).all())
    assert _band_edge_clear(case, C, Dm, delta)
    assert torch.equal(glab.cpu().long(), lab)
    assert abs(float(ginertia) - float(inertia)) <= float(bound.max(1).values.sum())
    # empty row: D_j = cn_j
    assert bool(((gD[0].cpu() - cn).abs() <= 4 * U * cn).all())


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_row_norms(cases, kind):
    case = cases(kind)
    got = S.sp_row_norms(case.gpu).cpu()
    assert got.dtype == torch.float64 and got[0] == 0.0
    if kind == "exact":
        assert torch.equal(got, case.xn)
    else:
        assert bool(((got - case.xn).abs() <= 2.0 ** -50 * case.xn).all())


@pytest.mark.parametrize("delta", [0.0, 0.5])
@pytest.mark.parametrize("k", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_estep_band(cases, kind, k, delta):
    _check_estep(cases(kind), k, delta)


@pytest.mark.parametrize("delta", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_estep_many_tiles(cases, kind, delta):
    # k = 1030: five centroid tiles, an LDS row above 8 KiB
    _check_estep(cases(kind, 1100), 1030, delta)


def test_estep_max_k(cases):
    # k = 16384: one wave per workgroup, a 128 KiB LDS row
    _check_estep(cases("exact", 100), S.MAX_K, 0.5)


def test_too_many_clusters(cases):
    case = cases("exact")
    with pytest.raises(ValueError):
        S.sp_estep(case.gpu, torch.zeros((S.MAX_K + 1, D), device=case.gpu.device), 0.0, KEY)


def test_gram_and_ipe(cases):
    case = cases("random")
    dev = case.gpu.device
    k = 130
    C = _centres("random", k)
    G = S.sp_gram(case.gpu, C.to(dev)).cpu()
    assert G.dtype == torch.float32 and tuple(G.shape) == (N, k)
    want = torch.as_tensor(case.X.toarray()) @ C.T
    ulp = torch.as_tensor(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    assert bool(((G.double() - want).abs() <= ulp).all())
    # the engine's IPE E-step: chunking only moves row_offset
    out = []
    for chunk in (256, 4096):
        eng = _sparse.SparseLloydEngine(case.gpu, k, delta=0.5, true_distance_estimate=True,
                                        seed=3, ipe_Q=5, ipe_chunk=chunk)
        eng.restart, eng.it = 1, 2
        lab, mind, _ = eng.estep(C)
        out.append((lab.clone(), mind.clone(), eng))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    eng = out[0][2]
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    mind = torch.empty(N, dtype=torch.float32, device=dev)
    CT, cn = S.center_operand(C.to(dev))
    K.ipe_estep_native(S.sp_gram(case.gpu, C.to(dev)), eng.xn.float().contiguous(),
                       cn.float().contiguous(), 0.25, 5, eng._key("ipe"), 0, labels, mind)
    assert torch.equal(labels, out[0][0])


@pytest.mark.parametrize("weighted", [False, True])
def test_centroid_sums(cases, weighted):
    case = cases("exact")
    dev = case.gpu.device
    k = 7
    rng = np.random.RandomState(5)
    labels = torch.as_tensor(rng.randint(0, k - 1, size=N))      # cluster k - 1 stays empty
    w = torch.as_tensor(rng.randint(1, 9, size=N) / 4.0) if weighted else None
    sums, counts = S.sp_centroid_sums_torch(case.cpu, labels, k, w)
    wg = None if w is None else w.to(dev)
    a = S.sp_centroid_sums(case.gpu, labels.to(dev), k, wg)
    b = S.sp_centroid_sums(case.gpu, labels.to(dev).to(torch.int32), k, wg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0].cpu(), sums) and torch.equal(a[1].cpu(), counts)
    assert float(counts[k - 1]) == 0.0


def test_engine_step_exact(cases):
    """One full iteration (band E-step + M-step) on the exact fixture: labels,
    inertia and centres bit-equal to the CPU engine."""
    case = cases("exact")
    k = 65
    C = _centres("exact", k)
    res = []
    for sd in (case.cpu, case.gpu):
        eng = _sparse.SparseLloydEngine(sd, k, delta=0.5, seed=9)
        eng.set_centers(C)
        labels, sc = eng.step()
        res.append((labels.cpu().long(), sc.cpu(), eng.centers().cpu()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1][0], res[1][1][0])      # the inertia
    assert torch.equal(res[0][2], res[1][2])


def _planted(n=1500, d=300, k=5, seed=1):
    rng = np.random.RandomState(seed)
    A = np.zeros((n, d))
    for c in range(k):
        cols = rng.choice(d, size=20, replace=False)
        A[c::k][:, cols] += rng.choice([-5.0, 5.0], size=20)
    noise = sp.random(n, d, density=10.0 / d, random_state=seed).toarray() * 0.1
    A = (A + noise).astype(np.float32).astype(np.float64)
    return sp.csr_matrix(A), A[:k].copy()


@pytest.fixture(scope="module")
def planted():
    return _planted()


@pytest.mark.parametrize("which", ["kmeans", "qmeans"])
def test_end_to_end(cuda, planted, which):
    X, init = planted

    def make(device):
        if which == "kmeans":
            return KMeans(5, n_init=1, init=init, device=device)
        return QMeans(5, n_init=1, init=init, delta=0.5, true_distance_estimate=False,
                      random_state=0, device=device)
    cpu = make("cpu").fit(X)
    g1 = make("cuda").fit(X)
    g2 = make("cuda").fit(X)
    assert np.array_equal(g1.labels_, cpu.labels_)
    assert g1.n_iter_ == cpu.n_iter_
    tol = 4.0 * X.shape[0] * U * np.abs(X.data).max() + 2.0 ** -52 * np.abs(cpu.cluster_centers_)
    assert (np.abs(g1.cluster_centers_ - cpu.cluster_centers_) <= tol).all()
    assert np.array_equal(g1.cluster_centers_, g2.cluster_centers_)
    assert np.array_equal(g1.labels_, g2.labels_) and g1.inertia_ == g2.inertia_
    assert len(np.unique(g1.labels_)) == 5


def test_predict_transform(cuda, planted):
    X, init = planted
    cpu = KMeans(5, n_init=1, init=init, device="cpu").fit(X)
    gpu = KMeans(5, n_init=1, init=init, device="cuda").fit(X)
    assert np.array_equal(gpu.predict(X), cpu.predict(X))
    assert np.allclose(gpu.transform(X), cpu.transform(X), rtol=1e-9, atol=1e-9)
    assert np.isclose(gpu.score(X), cpu.score(X), rtol=1e-12)
    q = QMeans(5, n_init=1, init=init, delta=0.5, true_distance_estimate=False, random_state=0,
               device="cuda").fit(X)
    assert np.array_equal(q.predict(X, delta=0.5), q.labels_)


def test_kmeans_plusplus_gpu_matches_cpu(cuda, planted):
    X, _ = planted
    ids = [_sparse.sparse_kmeans_plusplus(as_sparse_data(X, device=dev), 5,
                                          np.random.RandomState(4))[1] for dev in ("cpu", cuda)]
    assert np.array_equal(ids[0], ids[1])
    assert len(set(ids[0] % 5)) == 5          # one row of every planted cluster


def test_memory_refusal(cuda, cases, monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 1 << 30))
    with pytest.raises(ValueError, match="device memory"):
        _sparse.SparseLloydEngine(cases("exact").gpu, 64)
