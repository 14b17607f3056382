"""Gap records across the corners the 60k-row record tests do not reach
(csrc/estep_f32.hip: bounds_filter_kernel routes rows with a current record
to list B, gap_screen_kernel moves the records by the shift operand of their
base iteration's ring slot).  The records only change which kernel certifies
a row: labels, centres and the iteration scalars are bit-identical with them
on and off - with a ring of 2 or 3 base iterations (every step wraps it) and
with list-B rows that carry three or more candidates."""
import numpy as np
import pytest
import torch

from sq_learn_amd.models.cluster._lloyd import LloydEngine

pytestmark = pytest.mark.gpu


def _data(n, d, k, seed, spread):
    rs = np.random.RandomState(seed)
    G = rs.uniform(-spread, spread, (k, d))
    X = (G[rs.randint(k, size=n)] + rs.randn(n, d)).astype(np.float32)
    C0 = X[rs.choice(n, k, replace=False)]
    return X, C0


def _run(monkeypatch, X, C0, on, iters, reset_at=None, delta=2.0, each=None):
    monkeypatch.setenv("SQ_MULTI_RECORDS", "1" if on else "0")
    monkeypatch.setenv("SQ_ESTEP_BOUNDS", "1")
    monkeypatch.setenv("SQ_MSTEP_INCREMENTAL", "1")
    monkeypatch.setenv("SQ_ESTEP_KEEP_MAX", "1.0")   # always filter
    eng = LloydEngine(torch.from_numpy(X).cuda(), C0.shape[0], delta=delta,
                      intermediate_error=True, true_tomography=False, failure_prob=0.0, seed=5)
    assert eng.fast and eng.certified and eng.bounds and eng.incremental
    assert (eng.mrec is not None) == on
    eng.set_centers(torch.from_numpy(C0).cuda())
    out = []
    for it in range(iters):
        if reset_at is not None and it == reset_at:
            eng.set_centers(eng.centers().clone() * 1.01)
        labels, sc = eng.step()
        vals = sc.tolist()[:2]
        torch.cuda.synchronize()
        if each is not None:
            each(eng)
        out.append((labels.clone().cpu(), eng.centers().clone().cpu(), vals))
    return out, eng


def _same(a, b):
    assert len(a) == len(b)
    for (la, Ca, sa), (lb, Cb, sb) in zip(a, b):
        assert torch.equal(la, lb)
        assert torch.equal(Ca, Cb)
        assert sa == sb


@pytest.mark.parametrize("ring", [2, 3])
def test_ring_wrap_on_off_bit_identical(monkeypatch, ring):
    monkeypatch.setenv("SQ_GAP_RING", str(ring))
    X, C0 = _data(20011, 128, 48, seed=11, spread=3.0)
    resolved = []
    a, eng = _run(monkeypatch, X, C0, True, 12,
                  each=lambda e: resolved.append(int(e.buf.counts[4].item())))
    assert eng.dsh.shape[0] == ring
    b, _ = _run(monkeypatch, X, C0, False, 12)
    print("gap screen resolved per step:", resolved)
    assert max(resolved) > 0, "no row was resolved by the gap screen"
    _same(a, b)


def test_wide_candidate_sets_on_off_bit_identical(monkeypatch):
    X, C0 = _data(40003, 128, 96, seed=4, spread=1.2)
    widest = []

    def each(e):
        nb = int(e.buf.counts[5].item())
        rows = e.rows_b[:nb]
        widest.append(int(e.buf.multi_cand[rows, 0].max().item()) if nb else 0)

    a, _ = _run(monkeypatch, X, C0, True, 16, each=each)
    b, _ = _run(monkeypatch, X, C0, False, 16)
    print("widest candidate set on list B per step:", widest)
    assert max(widest) >= 3, "no list-B row with three or more candidates"
    _same(a, b)
