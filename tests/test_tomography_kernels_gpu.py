"""The multinomial kernels of csrc/tomography.hip against the exact host
model of ``_tomo_ref.py`` (run on an MI355X), through the native entries.

Every draw, tree and (row, checkpoint) pair that the reference does not mark
near a decision boundary (``margin <= 1``, budgets derived in ``_tomo_ref``;
``test_tomo_ref_cpu.py`` caps their share) must equal the reference bit for
bit; a mismatch is reported with the branch and the margin of the draw, so
that a budget set too tight can be told from a kernel bug.

Seeded errors and the tests that fail on them (each applied to a scratch
copy of the kernel, the extension rebuilt as a variant and this module run
against it):

| seeded error | failing tests |
|---|---|
| BTRS constant 2.53 -> 2.54 | binomial_grid, segment_trees[2 .. 2048], segment_levels, sid_position, host_recursion[all], tomography_mode1 / mode0 / mode2 (every d >= 2) |
| squeeze bound 0.92 -> 0.93 | segment_trees[2047, 2048], host_recursion[2049, 6149] |
| ``flip ? k : n - k`` | binomial_grid, segment_trees[2 .. 2048], segment_levels, sid_position, host_recursion[all], tomography_mode1 / mode0 / mode2 (every d >= 2) |
| tomography node counter ``nodes + i + 1`` | tomography_mode1 / mode0 / mode2 (every d >= 2) |
| segment node counter ``i >> 1`` (siblings share a Philox block) | binomial_grid, segment_trees[2 .. 2048], segment_levels, sid_position, host_recursion[all] |
| total of the last node read from ``pre[M - 1]`` (one slot short at the padding boundary) | tomography_mode1 / mode0 (d = 3, 63, 255, 511), mode2 (d = 3, 255, 511) |
| sign rule 0.4 -> 0.2 | tomography_mode1 / mode0 (d = 63, 64, 255, 511), mode2 (d = 255) |
| acceptance by lgamma differences (the formula before the saddle-point form) | binomial_grid (draws at n >= 5.8e11) |

The squeeze bound moves only draws with V in (0.92 - 4.2 / b, 0.93 - 4.2 / b]
that the full test would have rejected, about one in a thousand BTRS draws:
the 4034 draws of the binomial grid hold none, the large trees do.
"""
import numpy as np
import pytest
import torch

import _tomo_ref as R

pytestmark = pytest.mark.gpu


def _native():
    from sq_learn_amd.ops import _native as nat
    return nat


def _t(a, cuda, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=cuda).contiguous()


def run_segments(cuda, W, wrow, m, Nseg, key, sid, level, pad=3):
    """mnom_segments on W [rows, ldw] (ldw >= m): counts [B, m]; the ``pad``
    columns past m of the output rows must stay untouched."""
    nat = _native()
    Wt = _t(W, cuda)
    B = len(wrow)
    wr, sd = _t(wrow, cuda, torch.int64), _t(sid, cuda, torch.int64)
    Ns = _t(np.asarray(Nseg, dtype=np.float64).reshape(-1), cuda)
    cnt = torch.full((B, m + pad), -7.0, dtype=torch.float64, device=cuda)
    nat.native().mnom_segments(Wt.data_ptr(), Wt.stride(0), wr.data_ptr(), m, B, Ns.data_ptr(),
                               cnt.data_ptr(), cnt.stride(0), key[0], key[1], key[2], key[3],
                               sd.data_ptr(), int(level), nat.stream_handle(cuda))
    torch.cuda.synchronize()
    out = cnt.cpu().numpy()
    assert np.all(out[:, m:] == -7.0)
    return out[:, :m]


def run_tomography(cuda, V, sched, key, mode, first=None, norm_inf=False, row_offset=0, stop_err=0.0):
    """One launch of the tomography entry: err [r, T] (mode 0) or out [r, d]."""
    nat = _native()
    Vt = _t(V, cuda)
    r, d = Vt.shape
    sch = _t(sched, cuda, torch.int64)
    T = sch.numel()
    err = torch.full((r, T), -7.0, dtype=torch.float64, device=cuda)
    out = torch.full((r, d), -7.0, dtype=torch.float64, device=cuda)
    ft = _t(np.zeros(r) if first is None else first, cuda, torch.int32)
    nat.native().tomography(Vt.data_ptr(), r, d, sch.data_ptr(), T, mode, ft.data_ptr(),
                            err.data_ptr(), out.data_ptr(), int(norm_inf), key[0], key[1], key[2],
                            key[3], int(row_offset), nat.stream_handle(cuda), float(stop_err))
    torch.cuda.synchronize()
    return (err if mode == 0 else out).cpu().numpy()


def _same_bits(a, b):
    return (a == b) & (np.signbit(a) == np.signbit(b))


# ------------------------------------------------------------------ binomial
def test_binomial_grid(cuda):
    """One draw per workgroup (m = 2): the (n, p) grid, the pairs around
    n pp = 12 on both sides of the flip, a clamped negative weight."""
    c = R.binomial_case()
    ref = c["ref"]
    cnt = run_segments(cuda, c["W"], np.arange(len(c["N"])), 2, c["N"], c["key"], c["sid"], 0)
    np.testing.assert_array_equal(cnt[:, 0] + cnt[:, 1], c["N"])
    assert np.all((cnt >= 0) & (cnt == np.round(cnt)))
    assert np.all(cnt[-2:, 0] == [1000.0, 0.0])            # negative weights count as 0
    off = cnt[:, 0] != ref["count"]
    bad = np.nonzero(off & (ref["margin"] > 1.0))[0]
    print(f"draws {off.size}, off the reference {int(off.sum())}, excused {int((ref['margin'] <= 1).sum())}")
    msg = [f"n={c['N'][i]:g} p={c['p'][i]!r} sid={c['sid'][i]}: device {cnt[i, 0]:.0f} reference "
           f"{ref['count'][i]:.0f} branch {R.BRANCH_NAMES[ref['branch'][i]]} trials {ref['trials'][i]} "
           f"margin {ref['margin'][i]:.3g} lv {ref['lv'][i]!r} L {ref['L'][i]!r}" for i in bad[:12]]
    assert bad.size == 0, f"{bad.size} draws differ:\n" + "\n".join(msg)


# ------------------------------------------------------------------ segment trees
def _compare_trees(tag, dev, ref_cnt, margin, N):
    """Rows of ``dev`` against ``ref_cnt``; margin [B] or [B, nseg]."""
    np.testing.assert_array_equal(dev.sum(1), N)
    assert np.all((dev >= 0) & (dev == np.round(dev)))
    tree_ok = np.asarray(margin).reshape(len(N), -1).min(1) > 1.0
    off = (dev != ref_cnt).any(1)
    bad = np.nonzero(off & tree_ok)[0]
    info = [(int(b), int(np.nonzero(dev[b] != ref_cnt[b])[0][0])) for b in bad]
    assert bad.size == 0, f"{tag}: trees (row, first outcome off) {info}"
    return int(tree_ok.sum())


@pytest.mark.parametrize("m", R.SEG_M)
def test_segment_trees(cuda, m):
    """One-segment trees: generic weights, runs of zeros with a negative
    entry, a single non-zero weight, integers; rows picked through ``wrow``
    from a matrix whose stride exceeds m."""
    c = R.segment_case(m)
    dev = run_segments(cuda, c["W"], c["wrow"], m, c["N"], c["key"], c["sid"], 0)
    checked = _compare_trees(f"m={m}", dev, c["ref"]["cnt"], c["ref"]["margin"], c["N"])
    assert checked >= 5
    if m > 1:
        assert np.all(dev[~(c["W"][c["wrow"], :m] > 0)] == 0)


def test_segment_levels_are_distinct_streams(cuda):
    outs = {}
    for lv in R.SEG_LEVELS:
        c = R.segment_case(257, lv)
        outs[lv] = run_segments(cuda, c["W"], c["wrow"], 257, c["N"], c["key"], c["sid"], lv)
        _compare_trees(f"level={lv}", outs[lv], c["ref"]["cnt"], c["ref"]["margin"], c["N"])
    for a in R.SEG_LEVELS:
        for b in R.SEG_LEVELS:
            if a < b:
                assert not np.array_equal(outs[a], outs[b])


def test_sid_is_independent_of_batch_position(cuda):
    """A one-row launch of (weights, N, sid) reproduces its row of the batch,
    and the reference."""
    c = R.segment_case(257)
    full = run_segments(cuda, c["W"], c["wrow"], 257, c["N"], c["key"], c["sid"], 0)
    for b in (0, 3, 5):
        one = run_segments(cuda, c["W"], c["wrow"][b:b + 1], 257, c["N"][b:b + 1], c["key"],
                           c["sid"][b:b + 1], 0)
        np.testing.assert_array_equal(one[0], full[b])
        if c["ref"]["margin"][b].min() > 1.0:
            np.testing.assert_array_equal(one[0], c["ref"]["cnt"][b])
    # another sid at the same position draws another tree
    other = run_segments(cuda, c["W"], c["wrow"][3:4], 257, c["N"][3:4], c["key"], c["sid"][3:4] + 1, 0)
    assert not np.array_equal(other[0], full[3])


@pytest.mark.parametrize("m", R.LONG_M)
def test_host_recursion(cuda, m):
    """Several segments (a last one of length 1 at m = 2049): the segment
    totals come from the host recursion one level up."""
    from sq_learn_amd.quantum import device as QD
    from sq_learn_amd.runtime.rng import RngKey
    c = R.long_case(m)
    key = RngKey.__new__(RngKey)
    key.k0, key.k1 = c["key"][0], c["key"][1]
    key.stream = c["key"][2] | (c["key"][3] << 32)
    dev = QD.multinomial_long(_t(c["N"], cuda), _t(c["W"], cuda), _t(c["wrow"], cuda, torch.int64),
                              key, _t(c["sid"], cuda, torch.int64)).cpu().numpy()
    checked = _compare_trees(f"m={m}", dev, c["ref"]["cnt"], c["ref"]["margin"], c["N"])
    assert checked >= 4
    assert np.all(dev[~(c["W"][c["wrow"]] > 0)] == 0)


# ------------------------------------------------------------------ tomography
TOMO_CASES = [pytest.param(d, big, id=f"d{d}" + ("-1e10" if big else "")) for d, big in R.tomo_case_list()]


def _which_round(dev, ref_est):
    return "round 1 (magnitudes)" if np.any(np.abs(dev) != np.abs(ref_est)) else "round 2 (signs)"


@pytest.mark.parametrize("d,big", TOMO_CASES)
def test_tomography_mode1(cuda, d, big):
    """The estimate of every checkpoint, bit for bit (the sign of a zero
    included), at global row offset ROW_OFFSET."""
    c = R.tomo_case(d, False, big)
    ref = c["ref"]
    checked = 0
    for t in range(len(c["sched"])):
        out = run_tomography(cuda, c["V"], c["sched"], c["key"], 1, first=np.full(c["r"], t),
                             row_offset=R.ROW_OFFSET)
        for row in range(c["r"]):
            if ref["margin2"][row, t] <= 1.0:
                continue
            checked += 1
            ok = _same_bits(out[row], ref["est"][row, t])
            assert ok.all(), (f"d={d} row {row} (exact={bool(c['exact'][row])}) checkpoint {t} "
                              f"N={c['sched'][t]}: {_which_round(out[row], ref['est'][row, t])} "
                              f"diverged at outcomes {np.nonzero(~ok)[0][:8]}; reference counts "
                              f"{ref['cnt1'][row, t][~ok][:8]} / plus {ref['cnt2'][row, t][~ok][:8]}")
    assert checked >= 0.95 * c["r"] * len(c["sched"])


@pytest.mark.parametrize("norm_inf", [False, True], ids=["l2", "linf"])
@pytest.mark.parametrize("d,big", TOMO_CASES)
def test_tomography_mode0(cuda, d, big, norm_inf):
    """Every checkpoint's error: L2 within the bound of the kernel's lane and
    butterfly order (``_tomo_ref.err_bound``), L-inf bit for bit."""
    c = R.tomo_case(d, norm_inf, big)
    ref = c["ref"]
    err = run_tomography(cuda, c["V"], c["sched"], c["key"], 0, norm_inf=norm_inf,
                         row_offset=R.ROW_OFFSET)
    sure = ref["margin2"] > 1.0
    bound = 0.0 if norm_inf else R.err_bound(d, ref["err"])
    diff = np.abs(err - ref["err"])
    rel = diff if norm_inf else diff / np.maximum(bound, 1e-300)
    print(f"d={d}: largest error difference{'' if norm_inf else ' / bound'} {rel[sure].max():.3g}")
    assert np.all((diff <= bound) | ~sure), (np.nonzero(sure & (diff > bound)), err, ref["err"])
    assert sure.mean() >= 0.95


@pytest.mark.parametrize("norm_inf", [False, True], ids=["l2", "linf"])
@pytest.mark.parametrize("d,big", TOMO_CASES)
def test_tomography_mode2(cuda, d, big, norm_inf):
    """The one-launch walk stops at the reference's checkpoint and returns
    its row; with a bound nobody meets it returns the last checkpoint."""
    c = R.tomo_case(d, norm_inf, big)
    ref = c["ref"]
    for stop in (-1.0, R.mode2_stop(c)):
        t_stop, est, excused = R.mode2_ref(ref, stop, norm_inf)
        out = run_tomography(cuda, c["V"], c["sched"], c["key"], 2, norm_inf=norm_inf,
                             row_offset=R.ROW_OFFSET, stop_err=stop)
        for row in np.nonzero(~excused)[0]:
            assert _same_bits(out[row], est[row]).all(), (d, row, stop, int(t_stop[row]))
        assert excused.mean() <= 0.2
    assert np.all(R.mode2_ref(ref, -1.0, norm_inf)[0] == len(c["sched"]) - 1)


@pytest.mark.parametrize("d", [3, 65])
def test_tomography_row_split(cuda, d):
    """Rows [a, b) launched alone with row_offset = a equal rows [a, b) of
    the full launch, in every mode."""
    c = R.tomo_case(d)
    r, T = c["r"], len(c["sched"])
    a, b = 1, r
    first = np.arange(r) % T
    full1 = run_tomography(cuda, c["V"], c["sched"], c["key"], 1, first=first, row_offset=R.ROW_OFFSET)
    part1 = run_tomography(cuda, c["V"][a:b], c["sched"], c["key"], 1, first=first[a:b],
                           row_offset=R.ROW_OFFSET + a)
    assert _same_bits(part1, full1[a:b]).all()
    full0 = run_tomography(cuda, c["V"], c["sched"], c["key"], 0, row_offset=R.ROW_OFFSET)
    part0 = run_tomography(cuda, c["V"][a:b], c["sched"], c["key"], 0, row_offset=R.ROW_OFFSET + a)
    np.testing.assert_array_equal(part0, full0[a:b])
    # without the offset the rows draw other streams
    other = run_tomography(cuda, c["V"][a:b], c["sched"], c["key"], 0, row_offset=R.ROW_OFFSET)
    assert not np.array_equal(other, full0[a:b])


def test_tomography_rejects_512_outcomes(cuda):
    """d = 512 needs 513 padded outcomes: invalid-value status, no launch."""
    V = np.zeros((2, 512))
    V[:, 0] = 1.0
    nat = _native()
    Vt = _t(V, cuda)
    sch = _t([10], cuda, torch.int64)
    out = torch.full((2, 512), -7.0, dtype=torch.float64, device=cuda)
    ft = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match=r"\(1\)"):
        nat.native().tomography(Vt.data_ptr(), 2, 512, sch.data_ptr(), 1, 1, ft.data_ptr(), 0,
                                out.data_ptr(), 0, 1, 2, 3, 4, 0, nat.stream_handle(cuda), 0.0)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
