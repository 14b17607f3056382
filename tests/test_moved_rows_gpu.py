"""The gap screen's moved list (csrc/estep_f32.hip gap_screen_kernel) and the
label hand-off of pipelined steps.

A list-B row (a pruned row with a current gap record) can carry a new label
only when the gap screen resolved it with another argmin or forwarded it to
the multi list; the screen lists exactly those rows, and the incremental
M-step walks them instead of all of list B.  Labels, centres, the iteration
scalars and the fixed-point cluster statistics must be bit-identical to the
full walk over all rows (``SQ_DELTA_LISTS=0``), and the runs must exercise the
list: moved rows exist, they are fewer than list B, and some of them are rows
the screen resolved itself.

After the incremental M-step ``prev_labels`` holds the iteration's labels, so
a pipelined ``step()`` returns a view of it instead of a copy."""
import numpy as np
import pytest
import torch

from sq_learn_amd.models.cluster._lloyd import LloydEngine

pytestmark = pytest.mark.gpu

CASES = {
    #            n      d   seed  extra
    "records": (60000, 128, 1, {}),
    "reset": (60000, 128, 2, {"reset_at": 7}),
    "pipeline": (60000, 128, 3, {"pipeline": True}),
    "odd_n": (60013, 128, 4, {}),          # no multiple of 64 (nor of 4)
    "d256": (60000, 256, 5, {}),
}


def _data(n, d, k=64, seed=0, spread=3.0):
    rs = np.random.RandomState(seed)
    G = rs.uniform(-spread, spread, (k, d))
    X = (G[rs.randint(k, size=n)] + rs.randn(n, d)).astype(np.float32)
    C0 = X[rs.choice(n, k, replace=False)]
    return X, C0


def _engine(monkeypatch, X, C0, lists=None, incremental=True):
    if lists is None:
        monkeypatch.delenv("SQ_DELTA_LISTS", raising=False)   # the default
    else:
        monkeypatch.setenv("SQ_DELTA_LISTS", "1" if lists else "0")
    monkeypatch.setenv("SQ_MULTI_RECORDS", "1")
    monkeypatch.setenv("SQ_ESTEP_BOUNDS", "1")
    monkeypatch.setenv("SQ_MSTEP_INCREMENTAL", "1" if incremental else "0")
    monkeypatch.setenv("SQ_ESTEP_KEEP_MAX", "1.0")   # always filter
    eng = LloydEngine(torch.from_numpy(X).cuda(), C0.shape[0], delta=2.0,
                      intermediate_error=True, true_tomography=False, seed=5)
    assert eng.fast and eng.certified and eng.bounds
    assert eng.incremental == incremental
    assert (eng.mrec is not None) == incremental
    eng.set_centers(torch.from_numpy(C0).cuda())
    return eng


def _run(monkeypatch, X, C0, lists, iters=14, reset_at=None, pipeline=False):
    eng = _engine(monkeypatch, X, C0, lists)
    eng.pipeline = pipeline
    out, walks = [], []
    for it in range(iters):
        if reset_at is not None and it == reset_at:
            eng.set_centers(eng.centers().clone() * 1.01)
        before = getattr(eng, "delta_list_steps", 0)
        labels, sc = eng.step()
        vals = sc.tolist()[:2]
        torch.cuda.synchronize()
        out.append((labels.clone().cpu(), eng.centers().clone().cpu(), vals))
        # the counters of the E-step that ran last (pipelined: the next
        # iteration's, unpipelined: this one's) - one E-step each either way
        c = eng.buf.counts.tolist()
        walks.append({"listed": getattr(eng, "delta_list_steps", 0) > before,
                      "count_b": c[5], "n_done": c[4], "moved": c[8]})
    eng.pipeline = False
    eng.drop_pending()
    stats = (eng.sums.clone().cpu(), eng.counts.clone().cpu(), eng.qsum.clone().cpu(),
             eng.prev_labels[:eng.n].clone().cpu())
    return out, stats, walks


@pytest.mark.parametrize("case", list(CASES))
def test_moved_list_walk_bit_identical(monkeypatch, case):
    n, d, seed, kw = CASES[case]
    X, C0 = _data(n, d, seed=seed)
    a, sa, wa = _run(monkeypatch, X, C0, None, **kw)     # the default: the moved-list walk
    b, sb, wb = _run(monkeypatch, X, C0, False, **kw)    # the full walk over all rows
    print(case, [(w["listed"], w["count_b"], w["n_done"], w["moved"]) for w in wa])
    for (la, Ca, va), (lb, Cb, vb) in zip(a, b):
        assert la.dtype == torch.int32 and la.shape == (n,)
        assert torch.equal(la, lb)
        assert torch.equal(Ca, Cb)
        assert va == vb
    for ta, tb in zip(sa, sb):
        assert torch.equal(ta, tb)
    # not vacuous
    assert sum(w["listed"] for w in wa) >= 5 and not any(w["listed"] for w in wb)
    assert sum(w["moved"] for w in wa) > 0
    assert any(w["count_b"] > 0 for w in wa)
    assert all(w["moved"] < w["count_b"] for w in wa if w["count_b"] > 0)
    # a row the screen resolved itself changed its label (the forwarded rows
    # alone are count_b - n_done)
    assert any(w["moved"] > w["count_b"] - w["n_done"] for w in wa)
    # the screen does the same with and without the list walk
    assert [(w["count_b"], w["n_done"], w["moved"]) for w in wa] == \
        [(w["count_b"], w["n_done"], w["moved"]) for w in wb]


@pytest.mark.parametrize("case", ["records", "odd_n", "d256"])
def test_moved_list_content(monkeypatch, case):
    """One filtered E-step after some steps, before its M-step: the moved
    rows are list-B rows, each once, and hold every list-B row whose label
    differs from the previous iteration's."""
    n, d, seed, _ = CASES[case]
    X, C0 = _data(n, d, seed=seed)
    eng = _engine(monkeypatch, X, C0)
    seen_b = seen_changed = 0
    for it in range(10):
        labels, sc = eng.step()
        sc.tolist()
        if it < 3:
            continue
        # the next iteration's E-step, as step() would run it
        pending = eng._estep(eng._key("band_select"))
        lab = pending[0]
        torch.cuda.synchronize()
        assert eng._dlists is not None and eng._dlists[2][0] is eng.rows_moved
        c = eng.buf.counts.tolist()
        rows_b = eng.rows_b[:c[5]].cpu()
        moved = eng.rows_moved[:c[8]].cpu()
        assert moved.numel() == 0 or (int(moved.min()) >= 0 and int(moved.max()) < n)
        assert torch.unique(moved).numel() == moved.numel()
        assert torch.unique(rows_b).numel() == rows_b.numel()
        in_b = torch.zeros(n, dtype=torch.bool)
        in_b[rows_b] = True
        assert bool(in_b[moved].all())
        in_m = torch.zeros(n, dtype=torch.bool)
        in_m[moved] = True
        changed = (lab[:n].cpu() != eng.prev_labels[:n].cpu())
        assert not bool((changed & in_b & ~in_m).any())
        # and the three lists together hold every changed row
        listed = in_m.clone()
        listed[eng.rlist[:c[3]].cpu()] = True
        listed[eng.buf.multi_rows[:c[7]].cpu()] = True
        assert not bool((changed & ~listed).any())
        seen_b += c[5]
        seen_changed += int((changed & in_b).sum())
        # the next step() takes this E-step as a pipelined loop would
        eng._pending = pending
    assert seen_b > 0 and seen_changed > 0


def test_pipelined_labels_are_prev_labels(monkeypatch):
    """Incremental M-step: the pipelined step hands out prev_labels (no
    copy), equal to the unpipelined run's labels until the next step()."""
    n, d, seed, _ = CASES["pipeline"]
    X, C0 = _data(n, d, seed=seed)

    def run(pipeline):
        eng = _engine(monkeypatch, X, C0)
        eng.pipeline = pipeline
        out, shared = [], []
        for _ in range(8):
            labels, sc = eng.step()
            sc.tolist()
            shared.append(labels.untyped_storage().data_ptr()
                          == eng.prev_labels.untyped_storage().data_ptr())
            assert labels.dtype == torch.int32 and labels.shape == (n,)
            out.append(labels.clone().cpu())     # before the next step()
        eng.pipeline = False
        eng.drop_pending()
        return out, shared

    a, sh_a = run(True)
    b, sh_b = run(False)
    assert all(sh_a) and not any(sh_b)
    for la, lb in zip(a, b):
        assert torch.equal(la, lb)


def test_pipelined_labels_copy_path(monkeypatch):
    """SQ_MSTEP_INCREMENTAL=0: the pipelined step still snapshots the labels
    (the next E-step rewrites the buffer); same labels as unpipelined."""
    n, d, seed, _ = CASES["pipeline"]
    X, C0 = _data(n, d, seed=seed)

    def run(pipeline):
        eng = _engine(monkeypatch, X, C0, incremental=False)
        eng.pipeline = pipeline
        out = []
        for _ in range(6):
            labels, sc = eng.step()
            sc.tolist()
            assert labels.dtype == torch.int32 and labels.shape == (n,)
            if pipeline:
                assert labels.data_ptr() != eng.buf.labels.data_ptr()
            out.append(labels.clone().cpu())
        eng.pipeline = False
        eng.drop_pending()
        return out

    for la, lb in zip(run(True), run(False)):
        assert torch.equal(la, lb)
