"""Row-list CSR kernels of the sparse mini-batch step (``csrc/spminibatch.hip``)
and ``MiniBatchKMeans`` on sparse input, against the fp64 torch twins.

Kernel fixture (the idea of ``test_sparse_kmeans_gpu.py``): n = 2000,
d = 1000, about 20 nonzeros per row; rows 0..7 hold exactly 0, 1, 3, 4, 5, 63,
64, 65 nonzeros - both sides of the 64-wide load and of the 4-wide unroll -
row 8 holds 300, row 9 an explicitly stored zero, row 10 uses the last column.
Two value sets share the structure:

* exact: integer values, weights in {0.5, 1, 2}, centres multiples of 1/8 and
  integer counts, so every fp64 product, sum and quantum is exact in any
  order and the GPU must match the twin bit for bit;
* random: fp32-rounded normal values.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sq_learn_amd.cluster import MiniBatchKMeans
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import sparse_kmeans as S

pytestmark = pytest.mark.gpu

SEED = 4242    # random fixture: at most 1 % of the positions near a tie (checked on the twin)
N, D = 2000, 1000
FORCED = [0, 1, 3, 4, 5, 63, 64, 65, 300]
SPECIAL = list(range(11))   # the forced rows, the stored zero, the last column
M_LIST = 9000               # more positions than the 8192 waves of the persistent grid
U = 2.0 ** -53


def _structure():
    rng = np.random.RandomState(SEED)
    counts = rng.randint(10, 31, size=N)
    counts[:len(FORCED)] = FORCED
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(D, size=c, replace=False)) for c in counts])
    indices[indptr[11] - 1] = D - 1          # row 10 uses the last column
    assert indices[indptr[11] - 2] < D - 1 and indptr[10] < indptr[11]
    return rng, indptr, indices.astype(np.int32)


def _matrix(kind, d=D):
    rng, indptr, indices = _structure()
    nnz = len(indices)
    if kind == "exact":
        v = rng.randint(1, 9, size=nnz) * rng.choice([-1.0, 1.0], size=nnz)
    else:
        v = rng.standard_normal(nnz).astype(np.float32).astype(np.float64)
    v[indptr[9]] = 0.0                        # row 9: an explicitly stored zero
    A = sp.csr_matrix((v, indices, indptr), shape=(N, D))
    if d == 1:
        # one feature: integer values on about half of the rows, row 0 empty
        col = rng.randint(-8, 9, size=N) * (rng.rand(N) < 0.5)
        col[0] = 0
        A = sp.csr_matrix(col.reshape(N, 1).astype(np.float64))
    return A


def _centres(kind, k, d=D):
    rng = np.random.RandomState(SEED + k + d)
    if kind == "exact":
        C = rng.randint(-4, 5, size=(k, d)) / 8.0
        if k >= 2:
            C[k - 1] = C[0]                   # an exact tie on every row: the lowest index wins
        return torch.as_tensor(C)
    return torch.as_tensor(0.3 * rng.standard_normal((1, d)) + 0.05 * rng.standard_normal((k, d)))


def _row_list(m=M_LIST):
    """Row ids drawn with replacement, every special row included, with repeats."""
    rng = np.random.RandomState(SEED + 1)
    rows = rng.randint(0, N, size=m)
    rows[:len(SPECIAL)] = SPECIAL
    rows[-3:] = [8, 8, 0]                     # repeats of the long and of the empty row
    assert len(np.unique(rows)) < m
    return rows


def _weights(m):
    return np.random.RandomState(SEED + 2).choice([0.5, 1.0, 2.0], size=m)


class Case:
    def __init__(self, kind, dev, d=D):
        self.kind = kind
        self.X = _matrix(kind, d)
        self.cpu = as_sparse_data(self.X, device="cpu")
        self.gpu = as_sparse_data(self.X, device=dev)
        self.xn = S.sp_row_norms_torch(self.cpu)
        self.nnz_max = int(np.diff(self.X.indptr).max())


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind, d=D):
        if (kind, d) not in store:
            store[(kind, d)] = Case(kind, cuda, d)
        return store[(kind, d)]
    return get


# ---------------------------------------------------------------- kernel a
@pytest.fixture(scope="module")
def estep_twin(cases):
    store = {}

    def get(kind, k):
        if (kind, k) not in store:
            case = cases(kind)
            C = _centres(kind, k)
            rows, w = torch.as_tensor(_row_list()), torch.as_tensor(_weights(M_LIST))
            lab, mind, inertia = S.sp_list_estep_torch(case.cpu, C, rows, w, xn=case.xn)
            Dm = K.distances_torch(S.sp_rows_dense_torch(case.cpu, rows), C, case.xn[rows])
            store[(kind, k)] = (C, rows, w, lab, mind, inertia, Dm)
        return store[(kind, k)]
    return get


@pytest.mark.parametrize("k", [1, 3, 64, 65, 300])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_list_estep(cases, estep_twin, kind, k):
    case = cases(kind)
    dev = case.gpu.device
    C, rows, w, lab, mind, inertia, Dm = estep_twin(kind, k)
    # the GPU operand carries the twin's centre norms: the bound is the dot products' alone
    op = (S.center_operand(C.to(dev))[0], (C * C).sum(1).to(dev))
    glab, gmind, ginertia = S.sp_list_estep(case.gpu, C.to(dev), rows, w.to(dev),
                                            xn=case.xn.to(dev), operand=op)
    assert glab.dtype == torch.int32 and gmind.dtype == torch.float64
    assert glab.shape == (M_LIST,) and gmind.shape == (M_LIST,)
    glab, gmind = glab.cpu().long(), gmind.cpu()
    # the twin's label is the first index of the row minimum
    at_min = Dm == Dm.min(1).values[:, None]
    assert bool(at_min.gather(1, lab[:, None]).all())
    assert not bool((at_min & (torch.arange(k)[None, :] < lab[:, None])).any())
    if kind == "exact":
        assert torch.equal(glab, lab)
        assert torch.equal(gmind, mind)
        if k >= 2:
            assert bool((lab == 0).any()) and not bool((glab == k - 1).any())
    else:
        cn = (C * C).sum(1)
        bound = (4.0 * (case.nnz_max + 4) * U * (case.xn[rows][:, None] + cn[None, :])).max(1).values
        assert bool(((gmind - mind).abs() <= bound).all())
        if k >= 2:
            two = Dm.topk(2, dim=1, largest=False).values
            clear = (two[:, 1] - two[:, 0]) > bound
            assert float((~clear).double().mean()) <= 0.01      # the twin alone
            assert torch.equal(glab[clear], lab[clear])
        else:
            assert bool((glab == 0).all())
    np.testing.assert_allclose(float(ginertia), float(inertia), rtol=1e-12)
    # repeated ids are ordinary entries: equal rows give equal results
    assert glab[-2] == glab[-3] == glab[8] and gmind[-2] == gmind[-3] == gmind[8]


def test_list_estep_contiguous_range(cases):
    """``rows=None``: the contiguous rows, as ``compute_labels`` / ``predict`` use it."""
    case = cases("exact")
    dev = case.gpu.device
    C = _centres("exact", 65)
    lab, mind, inertia = S.sp_list_estep_torch(case.cpu, C, None, None, xn=case.xn)
    glab, gmind, ginertia = S.sp_list_estep(case.gpu, C.to(dev), xn=case.xn.to(dev))
    assert torch.equal(glab.cpu().long(), lab) and torch.equal(gmind.cpu(), mind)
    np.testing.assert_allclose(float(ginertia), float(inertia), rtol=1e-12)


# ----------------------------------------------------------- kernels b and c
def _update_inputs(kind, k, d, m, pattern):
    rng = np.random.RandomState(SEED + 3 + k + d + m)
    rows = rng.randint(0, N, size=m)
    rows[:min(m, len(SPECIAL))] = SPECIAL[:min(m, len(SPECIAL))]
    if m > 20:
        rows[-5:] = rows[:5]                                 # repeats
    if pattern == "one" or k == 1:
        labels = np.full(m, k // 2)                          # one centre takes every row
    else:
        labels = rng.choice(np.arange(0, k, 3), size=m)      # two thirds of the centres take none
    w = rng.choice([0.5, 1.0, 2.0], size=m)
    counts = rng.randint(0, 4, size=k).astype(np.float64)    # old counts include 0
    counts[k // 2] = 0.0
    if k > 1:
        counts[0] = 3.0
    return (torch.as_tensor(rows), torch.as_tensor(labels), torch.as_tensor(w),
            torch.as_tensor(counts))


def _gpu_update(case, C, counts, rows, labels, w):
    dev = case.gpu.device
    mx = float(case.cpu.data.abs().max())
    st = S.MiniBatchState(dev, C, counts, mx, float(w.max()))
    st.scatter(case.gpu, rows, labels.to(dev).to(torch.int32), w.to(dev))
    st.update()
    return st


@pytest.mark.parametrize("pattern", ["spread", "one"])
@pytest.mark.parametrize("m", [1, 700])
@pytest.mark.parametrize("d", [1, 1000])
@pytest.mark.parametrize("k", [1, 65])
def test_scatter_update_exact(cases, k, d, m, pattern):
    case = cases("exact", d)
    C = _centres("exact", k, d)
    rows, labels, w, counts = _update_inputs("exact", k, d, m, pattern)
    sums, wsum = S.sp_list_sums_torch(case.cpu, rows, labels, k, w)
    Ct, counts_t, shift_t = S.minibatch_update_torch(C, counts, sums, wsum)
    st = _gpu_update(case, C, counts, rows, labels, w)
    gC, gCT, gcn, gcounts = st.C.cpu(), st.CT.cpu(), st.cn.cpu(), st.counts.cpu()
    assert torch.equal(gC, Ct)
    assert torch.equal(gcounts, counts_t)
    assert torch.equal(gCT, S.center_operand(Ct)[0])
    want_cn = (Ct * Ct).sum(1)
    assert bool(((gcn - want_cn).abs() <= d * 2.0 ** -52 * want_cn).all())
    idle = wsum == 0
    assert bool(idle.any()) == (k > 1)
    assert torch.equal(gC[idle], C[idle]) and torch.equal(gcounts[idle], counts[idle])
    assert torch.equal(gcn[idle], (C * C).sum(1)[idle])
    assert not bool(st.q.any())                              # the quanta were consumed
    rec = st.read_record()
    np.testing.assert_allclose(rec[1], float(shift_t), rtol=1e-12)
    assert rec[2] == float(counts_t.min())
    again = _gpu_update(case, C, counts, rows, labels, w)
    assert torch.equal(again.C, st.C) and torch.equal(again.CT, st.CT)
    assert torch.equal(again.cn, st.cn) and torch.equal(again.counts, st.counts)
    assert torch.equal(again.rec, st.rec)


@pytest.mark.parametrize("k", [1, 65])
def test_scatter_random_within_quantisation(cases, k):
    """Every fixed-point sum is within m quanta of the fp64 twin: half a
    quantum per term from the rounding rule, and the twin's own rounding of
    m terms stays below the other half (2^xexp >= max|w x| m 2^-52)."""
    case = cases("random")
    dev = case.gpu.device
    m = 700
    rows, labels, w, counts = _update_inputs("random", k, D, m, "spread")
    sums, wsum = S.sp_list_sums_torch(case.cpu, rows, labels, k, w)
    st = S.MiniBatchState(dev, _centres("random", k), counts, float(case.cpu.data.abs().max()),
                          float(w.max()))
    st.scatter(case.gpu, rows, labels.to(dev).to(torch.int32), w.to(dev))
    xexp, wexp = st.exps(m)
    q = st.q.cpu()
    gsums = q[:k * D].double().view(k, D) * 2.0 ** xexp
    assert bool(((gsums - sums).abs() <= m * 2.0 ** xexp).all())
    assert bool(((q[k * D:].double() * 2.0 ** wexp - wsum).abs() <= m * 2.0 ** wexp).all())
    # the fused update on these sums is the twin's formula
    Ct, counts_t, _ = S.minibatch_update_torch(st.C.cpu(), counts, gsums, q[k * D:].double() * 2.0 ** wexp)
    st.update()
    assert torch.equal(st.C.cpu(), Ct) and torch.equal(st.counts.cpu(), counts_t)
    assert torch.equal(st.CT.cpu(), S.center_operand(Ct)[0])


def test_zero_weight_quantum_rule(cuda):
    """The one difference between the two scatters.  Row 3's weight is below
    half a weight quantum (rn(0.4) = 0) while its weighted value is above half
    a value quantum (rn(0.4 * 3.5 / 2) = rn(0.7) = 1): the Lloyd M-step keeps
    that value quantum, the mini-batch scatter drops the whole position."""
    v, w = 3.5, [1.03, 1.0, 1.0, 0.4 * 2.0 ** -49]
    assert K.fixed_point_exp(v * 1.03, 4) == -48 and K.fixed_point_exp(1.03, 4) == -49
    qx = [round(wi * v * 2.0 ** 48) for wi in w]
    qw = [round(wi * 2.0 ** 49) for wi in w]
    assert qx[3] == 1 and qw[3] == 0
    sd = as_sparse_data(sp.csr_matrix(np.full((4, 1), v)), device=cuda)
    wt = torch.as_tensor(w, dtype=torch.float64, device=cuda)
    labels = torch.zeros(4, dtype=torch.int32, device=cuda)
    sums, counts = S.sp_centroid_sums(sd, labels, 1, wt)
    assert float(sums[0, 0]) == float(sum(qx[:3]) + 1) * 2.0 ** -48
    assert float(counts[0]) == float(sum(qw[:3])) * 2.0 ** -49
    st = S.MiniBatchState(cuda, torch.zeros((1, 1)), torch.zeros(1), max_abs=v, max_w=1.03)
    st.scatter(sd, None, labels, wt)
    assert st.exps(4) == (-48, -49)
    assert st.q.tolist() == [sum(qx[:3]), sum(qw[:3])]


# ---------------------------------------------------------------- kernel d
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_rows_dense(cases, kind):
    case = cases(kind)
    dev = case.gpu.device
    rows = np.array([0, 8, 3, 8, 10, 9, 1999, 0, 8, 5, 6, 7])   # empty, 300 nonzeros, repeats
    want = torch.as_tensor(case.X[rows].toarray())
    got = S.sp_rows_dense(case.gpu, rows)
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), want)
    assert torch.equal(S.sp_rows_dense_torch(case.cpu, rows), want)
    # destination-index variant: out[dst[t]] = X[rows[t]], the other rows untouched
    dst = np.array([7, 2, 11, 0, 5, 9, 13, 4, 1, 12, 3, 15])
    for sd in (case.gpu, case.cpu):
        out = torch.full((16, D), 7.0, dtype=torch.float64, device=sd.device)
        S.sp_rows_dense(sd, rows, out=out, dst=dst)
        ref = torch.full((16, D), 7.0, dtype=torch.float64)
        ref[torch.as_tensor(dst)] = want
        assert torch.equal(out.cpu(), ref)


# --------------------------------------------------------------- estimator
EN, ED, EK = 3000, 500, 5


def _planted():
    """Dyadic values (multiples of 1/16, |v| < 8): every sum of a batch is
    exact in fp64 and a multiple of the fixed-point quantum, so the update is
    the same arithmetic on both devices."""
    rng = np.random.RandomState(99)
    lab = rng.randint(EK, size=EN)
    X = np.zeros((EN, ED))
    for i in range(EN):
        blk = np.arange(lab[i] * 40, lab[i] * 40 + 40)
        on = blk[rng.rand(40) < 0.5]
        X[i, on] = 4.0 + np.round(8 * rng.standard_normal(len(on))) / 16.0
        noise = rng.choice(ED, size=6, replace=False)
        X[i, noise] += np.round(4 * rng.standard_normal(6)) / 16.0
    assert np.array_equal(X, np.round(X * 16) / 16) and np.abs(X).max() < 8
    return sp.csr_matrix(X)


class _GapSpy:
    """Smallest best-to-second gap, relative to the distance scale, over the
    E-steps of a CPU run."""

    def __init__(self):
        self.gaps = []
        self.real = S.sp_list_estep_torch

    def __call__(self, sd, C, rows=None, weights=None, xn=None, **kw):
        r = torch.arange(sd.shape[0]) if rows is None else torch.as_tensor(rows)
        Dm = K.distances_torch(S.sp_rows_dense_torch(sd, r), C.double())
        two = Dm.topk(2, dim=1, largest=False).values
        self.gaps.append(float((two[:, 1] - two[:, 0]).min() / Dm.max()))
        return self.real(sd, C, rows, weights, xn, **kw)


def _fit(A, device):
    return MiniBatchKMeans(EK, batch_size=256, max_iter=4, random_state=8, device=device).fit(A)


def _partial(A, device):
    m = MiniBatchKMeans(EK, random_state=8, device=device)
    for a in (0, 1000, 2000):
        m.partial_fit(A[a:a + 1000])
    return m


def _no_near_tie(run):
    """``run()`` on the CPU with the precondition of the device comparison
    checked: no argmin of the run is within 1e-6 of the distance scale of
    the runner-up."""
    spy = _GapSpy()
    S.sp_list_estep_torch = spy
    try:
        out = run()
    finally:
        S.sp_list_estep_torch = spy.real
    assert len(spy.gaps) > 3 and min(spy.gaps) > 1e-6
    return out


@pytest.fixture(scope="module")
def cpu_runs():
    A = _planted()
    return A, _no_near_tie(lambda: _fit(A, "cpu")), _no_near_tie(lambda: _partial(A, "cpu"))


def _assert_same_fit(g, c):
    assert g.n_iter_ == c.n_iter_ and g.n_steps_ == c.n_steps_
    assert np.array_equal(g.labels_, c.labels_)
    assert np.array_equal(g.counts_, c.counts_)
    assert g.cluster_centers_.dtype == np.float64
    assert np.array_equal(g.cluster_centers_, c.cluster_centers_)
    np.testing.assert_allclose(g.inertia_, c.inertia_, rtol=1e-12)


def test_fit_matches_cpu(cuda, cpu_runs):
    A, c, _ = cpu_runs
    g = _fit(A, cuda)
    _assert_same_fit(g, c)
    assert len(np.unique(g.labels_)) == EK
    assert np.array_equal(g.predict(A), g.labels_)
    np.testing.assert_allclose(g.score(A), -g.inertia_, rtol=1e-12)
    np.testing.assert_allclose(g.transform(A[:100]), c.transform(A[:100]), rtol=1e-9, atol=1e-9)
    g2 = _fit(A, cuda)
    assert np.array_equal(g2.cluster_centers_, g.cluster_centers_)
    assert np.array_equal(g2.labels_, g.labels_) and g2.inertia_ == g.inertia_


def test_partial_fit_matches_cpu(cuda, cpu_runs):
    A, _, c = cpu_runs
    g = _partial(A, cuda)
    assert g.n_steps_ == 3
    assert np.array_equal(g.labels_, c.labels_) and np.array_equal(g.counts_, c.counts_)
    assert np.array_equal(g.cluster_centers_, c.cluster_centers_)
    np.testing.assert_allclose(g.inertia_, c.inertia_, rtol=1e-12)


def test_fit_reassigns_on_device(cuda, cpu_runs):
    """A far-away centre and its duplicate are starved and get replaced by
    batch rows (kernel d, destination variant); the run equals the CPU's."""
    A = cpu_runs[0]
    Xd = A.toarray()
    init = np.vstack([Xd[[np.flatnonzero(Xd[:, c * 40:c * 40 + 40].sum(1) > 40)[0] for c in range(EK)]],
                      np.full((2, ED), 64.0)])
    kw = dict(init=init, batch_size=256, max_iter=2, random_state=1, reassignment_ratio=0.3,
              max_no_improvement=None)
    c = _no_near_tie(lambda: MiniBatchKMeans(EK + 2, device="cpu", **kw).fit(A))
    g = MiniBatchKMeans(EK + 2, device=cuda, **kw).fit(A)
    assert np.abs(c.cluster_centers_).max() < 16.0          # the starved centres were replaced
    _assert_same_fit(g, c)
