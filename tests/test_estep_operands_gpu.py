"""The two table producers of the certified E-step (csrc/estep_f32.hip)
against the long-double reference of ``_estep_operand_ref.py``, and feeding
their consumers:

A. ``sq_fast_centroids`` (fast_select_kernel, fast_cc_kernel): Hamerly
   shifts, ranks, ``smax_rest``, the Elkan table ``cc`` and its row minimum;
B. ``sq_shift_operand`` (shift_operand_kernel): the snapshot ring, the fp16
   operand and every ``dq`` word, over sequences of six updates driven by the
   engine's ring rule;
C. the producers' outputs through ``bounds_filter_kernel`` and
   ``gap_screen_kernel`` on real geometry, checked against the TRUTH under
   the new centres (one-sided: no row near a threshold is left out).

Every tolerance is a margin the kernels document: 2^-19 relative for a value
"rounded down / up" through fp32 (one conversion, one product by 1 -+ 2^-20,
<= 3 fp32 roundings), 1e-30 absolute guards (two of them: 2e-30), 2e-12 for
the shifts' (1 + 1e-12).  The checks are plain numpy functions of host
arrays; a wrong output fails the matching comparison (tried on the reference
side: e_j without its upward rounding, cc rounded up, ties to the higher
index, a snapshot taken one update early, smax_rest one rank off).

Two statements of the kernel's comment are narrowed here to what holds:
the fp64 shift is exact only while the exponents of c(t+1) and c(b) are at
most 2^29 apart per coordinate (outside: soundness inequalities only), and a
coordinate 2^-30 of amax has a SUBNORMAL fp16 image, not zero (zero needs
about 2^-39; both are in every sequence).

Gap-screen chain, delta = 4: 75 % of the listed rows have every true gap
above delta + 1 (both d_pad; test_estep_operand_ref_cpu.py asserts >= 25 %).
"""
import functools
import types

import numpy as np
import pytest
import torch

import _estep_operand_ref as R
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import linalg as L

pytestmark = pytest.mark.gpu

LD = np.longdouble
UP19 = LD(1) + LD(2.0) ** -19
DOWN19 = LD(1) - LD(2.0) ** -19


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())      # (a writable copy)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ===================================================================== A
SHIFT_FILL, IDX_FILL, CC_FILL, SMAX_FILL = -7.0, -77, 12345.0, -5.0
IDX_TAIL, CC_TAIL = 4, 8


def check_fast_centroids(out, k, nf, C, shift_in, shift_sq):
    """out: shift [k] fp64, idx [max(nf, 1) + IDX_TAIL] int32, smax [1] fp64,
    cc [k (nf + 1) + CC_TAIL] fp32 as the kernel left them."""
    shift, idx, smax, cc = out.shift, out.idx, out.smax, out.cc
    if shift_sq is not None:
        true = R.sqrt_true(shift_sq)
        assert (shift >= true.astype(np.float64)).all(), "a shift below sqrt(shift_sq)"
        assert (R.wide(shift) <= true * (LD(1) + LD(2e-12))).all(), "a shift above the margin"
    else:
        assert _same_bits(shift, shift_in), "shift rewritten without shift_sq"
    order = R.rank_order(shift)
    assert idx[:nf].tolist() == order[:nf].tolist(), "rank rule"
    assert (idx[nf:] == IDX_FILL).all(), "idx written past nf"
    assert _same_bits(smax, shift[order[nf]:order[nf] + 1]), "smax_rest is not the shift of rank nf"
    rest = np.ones(k, bool)
    rest[idx[:nf]] = False
    assert (smax[0] >= shift[rest]).all()
    if nf == 0:
        assert smax[0] == shift.max()
        assert (cc == np.float32(CC_FILL)).all(), "cc written with nf = 0"
        return
    table = cc[:k * nf].reshape(k, nf)
    true = R.cc_true(C, idx[:nf])
    own = np.arange(k)[:, None] == idx[:nf][None, :]
    assert np.array_equal(np.isposinf(table), own), "+inf exactly on j == idx[f]"
    got = R.wide(table)[~own]
    assert (got <= true[~own]).all(), "cc above the true distance"
    assert (got >= true[~own] * DOWN19 - LD(2e-30)).all(), "cc further down than documented"
    assert _same_bits(cc[k * nf:k * nf + k], table.min(1)), "row minimum"
    assert (cc[k * (nf + 1):] == np.float32(CC_FILL)).all(), "cc written past k (nf + 1)"


def run_fast_centroids(k, nf, C, shift_in, shift_sq):
    shift = _t(np.full(k, SHIFT_FILL) if shift_sq is not None else shift_in)
    idx = torch.full((max(nf, 1) + IDX_TAIL,), IDX_FILL, dtype=torch.int32, device=_dev())
    smax = torch.full((1,), SMAX_FILL, dtype=torch.float64, device=_dev())
    cc = torch.full((k * (nf + 1) + CC_TAIL,), CC_FILL, dtype=torch.float32, device=_dev())
    K.fast_centroids_native(shift, _t(C), nf, idx, smax, cc,
                            shift_sq=None if shift_sq is None else _t(shift_sq))
    torch.cuda.synchronize()
    return types.SimpleNamespace(shift=shift.cpu().numpy(), idx=idx.cpu().numpy(),
                                 smax=smax.cpu().numpy(), cc=cc.cpu().numpy())


@pytest.mark.parametrize("d", [1, 63, 65, 200])
@pytest.mark.parametrize("k,nf", [(2, 1), (5, 0), (5, 3), (65, 64), (67, 16), (300, 16), (300, 7)])
def test_fast_centroids_against_reference(k, nf, d):
    for pat in R.SHIFT_PATTERNS:
        ssq = R.shift_sq_pattern(pat, k, nf)
        fast = int(R.rank_order(ssq)[0]) if nf else None
        for cen in R.CENTRE_PATTERNS:
            C = R.centre_pattern(cen, k, d, fast)
            for with_sq in (True, False):
                shift_in = None if with_sq else np.sqrt(ssq)
                out = run_fast_centroids(k, nf, C, shift_in, ssq if with_sq else None)
                try:
                    check_fast_centroids(out, k, nf, C, shift_in, ssq if with_sq else None)
                except AssertionError as e:
                    raise AssertionError(f"shifts {pat}, centres {cen}, shift_sq {with_sq}: {e}")


# ===================================================================== B
SNAP_FILL, DSH_FILL, DQ_FILL = 3.25e6, 123.0, -9.5


def _first_diff(got, want, ok, o):
    j, f = np.argwhere((_bits(got) != _bits(want)) & ok[:, None])[0]
    return (f"centroid {j} coordinate {f}: {float(got[j, f])!r} for {float(want[j, f])!r}, "
            f"beta S = {float(o.beta[j] * o.S[j, f])!r}")


def check_shift_update(before, after, o_ref, ref, C_prev, snew, valid, alpha, stats):
    """One update: ``before`` / ``after`` are (snap, dsh, dq) host copies,
    ``o_ref`` the reference's per-slot results, ``ref`` its ring."""
    ring, k, d_pad = after.dsh.shape
    d = ref.d
    for s in range(ring):
        if not (valid >> s) & 1:      # not valid: nothing of the slot is touched
            for name in ("snap", "dsh", "dq"):
                assert _same_bits(getattr(after, name)[s], getattr(before, name)[s]), (s, name)
            continue
        o = o_ref[s]
        if s == snew:
            want = np.zeros((k, d_pad), np.float32)
            want[:, :d] = C_prev
            assert _same_bits(after.snap[s], want), "snap[snew] is not C_prev, zero-padded"
        else:
            assert _same_bits(after.snap[s], before.snap[s]), f"snapshot {s} rewritten"
        assert _same_bits(after.snap[s], ref.snap[s]), "the ring disagrees with the reference's"
        dq, dsh = after.dq[s], after.dsh[s]
        ok = o.in_range
        stats["exact"] += int(ok.sum())
        stats["wild"] += int((~ok).sum())
        # ---- exactly defined outputs (inside the fp64-exact range)
        assert _same_bits(dq[ok, 4], o.inv[ok]), "dq4 is not float32(1 / (alpha beta))"
        assert _same_bits(dsh[ok], o.dsh[ok]), \
            "dsh is not float16(float32(beta S)): " + _first_diff(dsh, o.dsh, ok, o)
        assert not _bits(dsh[:, d:]).any(), "padded columns of dsh"
        assert not _bits(dq[:, 5:]).any(), "dq[5..7]"
        # beta of the kernel's own operand (a power of two; the reference's where exact)
        beta = LD(1) / (LD(alpha) * R.wide(dq[:, 4]))
        assert (np.frexp(beta)[0] == 0.5).all()
        # ---- soundness, every centroid
        q0, q1, sz, ez = (R.wide(dq[:, i]) for i in range(4))
        assert (np.abs(q0 - o.q) <= q1).all(), "err(q_j) too small"
        assert (sz >= o.norm).all(), "|S_j| not rounded up"
        e_true = R.operand_error(o.S, dsh, beta)
        assert (ez >= e_true).all(), "e_j too small"
        # ---- tightness (inside the range)
        cap = (LD(2.0) ** -24 * np.abs(o.q) + LD(1e-13) * o.nrm + LD(1e-30)) * UP19
        assert (q1[ok] <= cap[ok]).all(), "err(q_j) looser than documented"
        assert (sz[ok] <= o.norm[ok] * UP19).all(), "|S_j| looser than documented"
        assert (ez[ok] <= e_true[ok] * UP19 + LD(2e-30)).all(), "e_j looser than documented"
        hb = _bits(dsh)[:, :d]      # subnormal fp16 images: exponent field 0, fraction not
        stats["sub"] += int((((hb & 0x7C00) == 0) & ((hb & 0x3FF) != 0)).sum())


def _drive_shift_operand(k, d, d_pad, ring, alpha, strided, stats):
    seq, _ = R.operand_sequence(k, d)
    dev = _dev()
    snap = torch.full((ring, k, d_pad), SNAP_FILL, dtype=torch.float32, device=dev)
    dsh = torch.full((ring, k, d_pad), DSH_FILL, dtype=torch.float16, device=dev)
    dq = torch.full((ring, k, 8), DQ_FILL, dtype=torch.float32, device=dev)
    host = lambda: types.SimpleNamespace(**{n: v.cpu().numpy().copy() for n, v in  # noqa: E731
                                            (("snap", snap), ("dsh", dsh), ("dq", dq))})
    ref = R.ShiftOperandRef(k, d, d_pad, ring, alpha)
    rlo, ever = R.T0, 0
    after = host()
    for u in range(R.N_UPDATES):
        t = R.T0 + u
        if t == R.RLO_JUMP_AT:
            rlo = t           # the engine voids its records: older bases fall out of valid
        snew, valid, _ = R.engine_valid(t, ring, rlo)
        ever |= valid
        C_prev, C_new = seq[u], seq[u + 1]
        if strided:
            A, B = R.strided_pair(C_prev, C_new, d + 5)
            tp, tn = _t(A)[:, :d], _t(B)[:, :d]
        else:
            tp, tn = _t(C_prev), _t(C_new)
        before = after
        K.shift_operand_native(tp, tn, alpha, snap, dsh, dq, snew, valid)
        torch.cuda.synchronize()
        after = host()
        o_ref = ref.update(C_prev, C_new, snew, valid)
        try:
            check_shift_update(before, after, o_ref, ref, C_prev, snew, valid, alpha, stats)
        except AssertionError as e:
            raise AssertionError(f"alpha {alpha}, strided {strided}, update {u} (t = {t}, "
                                 f"snew {snew}, valid {valid:#b}): {e}")
    for s in range(ring):     # a slot that was never valid still holds its sentinels
        if not (ever >> s) & 1:
            assert (after.snap[s] == np.float32(SNAP_FILL)).all()
            assert (after.dsh[s] == np.float16(DSH_FILL)).all()
            assert (after.dq[s] == np.float32(DQ_FILL)).all()
    return ever


@pytest.mark.parametrize("ring", [2, 3, 8])
@pytest.mark.parametrize("d,d_pad", [(1, 128), (63, 128), (128, 128), (200, 256)])
@pytest.mark.parametrize("k", [1, 5, 67])
def test_shift_operand_against_reference(k, d, d_pad, ring):
    stats = dict(exact=0, wild=0, sub=0)
    for alpha in (1.0, 0.125):
        for strided in (False, True):
            ever = _drive_shift_operand(k, d, d_pad, ring, alpha, strided, stats)
    print(f"k {k} d {d} ring {ring}: {stats}")
    # both regimes were checked, the jump of rlo dropped slots (ring > 2), a ring of
    # 8 keeps slots that are never valid, and subnormal fp16 images occurred
    assert stats["exact"] > 0 and stats["wild"] > 0
    assert ring != 8 or ever != 0xFF
    assert d < 4 or stats["sub"] > 0


# ===================================================================== C
def _filter_run(g, nf):
    """fast_centroids (exact shift_sq) -> bounds_filter; returns the rows that
    keep their label unseen and the rewritten bounds."""
    dev = _dev()
    n, k = g.n, g.k
    shift = torch.zeros(k, dtype=torch.float64, device=dev)
    idx = torch.zeros(max(nf, 1), dtype=torch.int32, device=dev)
    smax = torch.zeros(1, dtype=torch.float64, device=dev)
    cc = torch.zeros(k * (nf + 1), dtype=torch.float32, device=dev)
    K.fast_centroids_native(shift, _t(g.C_new), nf, idx, smax, cc, shift_sq=_t(g.shift_sq))
    ub, lb = _t(g.ub), _t(g.lb)
    buf = types.SimpleNamespace(
        mflag=torch.zeros(n, dtype=torch.int32, device=dev),
        multi_rows=torch.full((n,), -1, dtype=torch.int64, device=dev),
        counts=torch.zeros(12, dtype=torch.int32, device=dev), corr=None)
    rlist = torch.full((n,), -1, dtype=torch.int64, device=dev)
    K.bounds_filter_native(_t(g.labels), ub, lb, shift, smax, g.delta, rlist, buf.counts[3:4], buf,
                           cc=cc if nf else None, nf=nf, fidx=idx if nf else None)
    torch.cuda.synchronize()
    cnt = buf.counts.tolist()
    assert cnt[2] == 0 and 0 <= cnt[3] <= n
    listed = rlist[:cnt[3]].cpu().numpy()
    assert len(set(listed.tolist())) == cnt[3] and (rlist[cnt[3]:] == -1).all()
    held = np.ones(n, bool)
    held[listed] = False
    return held, ub.cpu().numpy(), lb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _filter_runs(case):
    g = R.filter_geometry(case)
    return g, {nf: _filter_run(g, nf) for nf in (0, 3, 16)}


@pytest.mark.parametrize("case", ["d8", "d64"])
def test_filter_chain_is_sound_against_the_truth(case):
    g, runs = _filter_runs(case)
    ref_share = {nf: R.filter_rule_ref(g, nf).mean() for nf in runs}
    assert ref_share[0] >= 0.10 and (case != "d8" or ref_share[16] >= 0.50)
    for nf, (held, ub, lb) in runs.items():
        band, bad_ub, bad_lb = R.filter_unsound_rows(g, held, ub, lb)
        print(f"{case} nf {nf}: {100 * held.mean():.1f} % kept (reference "
              f"{100 * ref_share[nf]:.1f} %), unsound {len(band)} / {len(bad_ub)} / {len(bad_lb)}")
        assert len(band) == 0, f"nf {nf}: rows kept with a centroid within delta: {band[:8]}"
        assert len(bad_ub) == 0, f"nf {nf}: ub below the label distance: {bad_ub[:8]}"
        assert len(bad_lb) == 0, f"nf {nf}: lb above the nearest other: {bad_lb[:8]}"
        # bounds of the other rows are untouched
        assert _same_bits(ub[~held], g.ub[~held]) and _same_bits(lb[~held], g.lb[~held])
    # the one-sided checks are not vacuous: the kernel keeps rows, too
    assert runs[0][0].mean() >= 0.10 and (case != "d8" or runs[16][0].mean() >= 0.50)


@pytest.mark.parametrize("case", ["d8", "d64"])
def test_fast_centroids_never_lose_a_row(case):
    """Every row kept with nf = 0 (smax = the overall maximum) is kept with
    fast centroids."""
    _, runs = _filter_runs(case)
    for nf in (3, 16):
        lost = runs[0][0] & ~runs[nf][0]
        assert not lost.any(), f"nf {nf}: {np.flatnonzero(lost)[:8]}"


@functools.lru_cache(maxsize=None)
def _gap_run(d_pad):
    g = R.gap_geometry(d_pad)
    dev = _dev()
    n, k, d, ring = g.n, g.k, g.d, R.GAP_RING
    Xf = torch.zeros((n, d_pad), dtype=torch.float32, device=dev)
    Xf[:, :d] = _t(g.X)
    xn = L.row_norms_sq(Xf)
    alpha = K.choose_alpha(float(xn.max().item()), R.GAP_DELTA)
    Xh = (Xf * alpha).to(torch.float16)
    # three updates of real centres, the engine's ring rule
    snap = torch.zeros((ring, k, d_pad), dtype=torch.float32, device=dev)
    dsh = torch.zeros((ring, k, d_pad), dtype=torch.float16, device=dev)
    dq = torch.zeros((ring, k, 8), dtype=torch.float32, device=dev)
    ref = R.ShiftOperandRef(k, d, d_pad, ring, alpha)
    for u in range(3):
        t = R.GAP_T0 + u
        snew, valid, bases = R.engine_valid(t, ring, R.GAP_T0)
        K.shift_operand_native(_t(g.C[u]), _t(g.C[u + 1]), alpha, snap, dsh, dq, snew, valid)
        o_ref = ref.update(g.C[u], g.C[u + 1], snew, valid)
    it_now = R.GAP_T0 + 3
    assert sorted(bases.values()) == [it_now - 2, it_now - 1] == sorted(set(g.base.tolist()))
    listed = np.random.RandomState(d_pad).permutation(n)
    rec = _t(g.rec)
    mflag = _t((g.base + 2).astype(np.int32))
    labels = _t(g.labels)
    rows_b = _t(listed.astype(np.int64))
    cnt = lambda v=0: torch.full((1,), v, dtype=torch.int32, device=dev)   # noqa: E731
    count_b, multi_count, n_done, count_mv = cnt(n), cnt(), cnt(), cnt()
    multi_rows = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rows_mv = torch.full((n,), -1, dtype=torch.int64, device=dev)
    ydbg = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
    records = K.multi_records(rec=rec, mflag=mflag, it_now=it_now, it_lo=it_now - 2, dsh=dsh,
                              dq=dq, rows_b=rows_b, count_b=count_b, n_done=n_done,
                              rows_moved=rows_mv, count_moved=count_mv)
    K.gap_screen_native(Xh, xn, labels, multi_rows, multi_count, records, alpha, R.GAP_DELTA,
                        ydbg=ydbg)
    torch.cuda.synchronize()
    fwd = multi_rows[:int(multi_count.item())].cpu().numpy()
    return types.SimpleNamespace(
        g=g, alpha=alpha, listed=listed, o_ref=o_ref, xn=xn.cpu().numpy(), dq=dq.cpu().numpy(),
        ydbg=ydbg.cpu().numpy(), labels=labels.cpu().numpy(), forwarded=fwd,
        n_done=int(n_done.item()), mflag=mflag.cpu().numpy(), it_now=it_now)


@pytest.mark.parametrize("d_pad", [128, 256])
def test_gap_screen_dots_within_the_kernels_own_bound(d_pad):
    """|ydbg - x.S_true| <= E_c for every listed (row, candidate): the fp32
    row against the true accumulated shift, E_c from the dq the producer
    wrote."""
    r = _gap_run(d_pad)
    g, rows = r.g, r.listed
    rslot = g.base[rows] % R.GAP_RING
    jc = g.jc[rows]
    inr = np.arange(4)[None, :] < g.c_r[rows][:, None]
    S = np.stack([r.o_ref[s].S for s in range(2)])[:, :, :g.d]        # slots 0, 1: [2][k][d]
    assert set(rslot.tolist()) == {0, 1}
    x = R.wide(g.X[rows])
    want = np.stack([(x * S[rslot, jc[:, c]]).sum(1) for c in range(4)], axis=1)
    dqv = r.dq[rslot[:, None], jc].astype(np.float64)                 # [n][4][8]
    nx = np.sqrt(r.xn[rows].astype(np.float64)) * (1 + 2.0 ** -16)
    ex = 2.0 ** -11 * nx + np.sqrt(d_pad) * 2.0 ** -25 / r.alpha
    gam = (d_pad + 16) * 2.0 ** -24
    E = (ex[:, None] * dqv[:, :, 2]
         + (nx + ex)[:, None] * (dqv[:, :, 3] + gam * (dqv[:, :, 2] + dqv[:, :, 3])) + dqv[:, :, 1])
    got = r.ydbg.astype(np.float64)
    assert np.isfinite(got[inr]).all() and np.isnan(got[~inr]).all()
    excess = np.abs(R.wide(got) - want)[inr] / E[inr]
    print(f"d_pad {d_pad}: {int(inr.sum())} dots, max |error| / E_c {float(excess.max()):.4f}, "
          f"max |x.S| {float(np.abs(want[inr]).max()):.3f}, median E_c {np.median(E[inr]):.2e}")
    assert (E[inr] > 0).all() and excess.max() <= 1.0


@pytest.mark.parametrize("d_pad", [128, 256])
def test_gap_screen_resolves_only_what_the_truth_resolves(d_pad):
    r = _gap_run(d_pad)
    g = r.g
    m, margin = R.gap_true_margin(g)
    assert (margin > R.GAP_DELTA + 1).mean() >= 0.25
    fw = np.zeros(g.n, bool)
    fw[r.forwarded] = True
    assert len(set(r.forwarded.tolist())) == len(r.forwarded)
    done = ~fw                                   # every row is listed
    assert r.n_done == int(done.sum()) > 0
    ar = np.arange(g.n)
    wrong = done & (r.labels != g.jc[ar, m])
    close = done & ~(margin > LD(R.GAP_DELTA))
    moved = done & (m != g.slot)
    print(f"d_pad {d_pad}: resolved {int(done.sum())} of {g.n} ({int(moved.sum())} with a new "
          f"argmin), forwarded {int(fw.sum())}; rows with every gap > delta + 1: "
          f"{100 * (margin > R.GAP_DELTA + 1).mean():.1f} %")
    assert not wrong.any(), f"label is not the exact argmin: rows {np.flatnonzero(wrong)[:8]}"
    assert not close.any(), f"a candidate within delta: rows {np.flatnonzero(close)[:8]}"
    # with a ring of 3 every resolved record is rebased (age >= 1); forwarded rows keep theirs
    assert (r.mflag[done] == r.it_now + 2).all() and (r.mflag[fw] == g.base[fw] + 2).all()
    assert np.array_equal(r.labels[fw], g.labels[fw])
