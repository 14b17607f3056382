"""The E-step operand reference (``_estep_operand_ref.py``) on cases worked
by hand, and the preconditions of the GPU case matrix of
``test_estep_operands_gpu.py`` (they depend on the inputs alone, so they are
checked here, without a device).

Measured on the reference side:

| chain | input | share |
|---|---|---|
| filter, d = 8, delta = 40 | rows held with nf = 0 / 3 / 16 | 17.4 % / 34.4 % / 68.0 % |
| filter, d = 64, delta = 300 | rows held with nf = 0 / 3 / 16 | 33.3 % / 33.5 % / 33.6 % |
| gap screen, d_pad = 128, delta = 4 | rows with every gap above delta + 1 | 75.2 % |
| gap screen, d_pad = 256, delta = 4 | rows with every gap above delta + 1 | 74.9 % |
"""
import numpy as np
import pytest

import _estep_operand_ref as R

LD = np.longdouble


def test_long_double_has_a_64_bit_significand():
    assert np.finfo(LD).nmant >= 63


# ---------------------------------------------------------------- rank rule
def test_rank_rule_with_ties():
    s = np.array([0.5, 2.0, 0.5, 2.0, 0.0, 0.5])
    assert R.rank_of(s).tolist() == [2, 0, 3, 1, 5, 4]
    assert R.rank_order(s).tolist() == [1, 3, 0, 2, 5, 4]
    C = np.zeros((6, 1), np.float32)
    # the duplicated 2.0 straddles rank 1, the duplicated 0.5 ranks 2 .. 4
    for nf, idx, rest in [(0, [], 2.0), (1, [1], 2.0), (2, [1, 3], 0.5), (3, [1, 3, 0], 0.5),
                          (4, [1, 3, 0, 2], 0.5), (5, [1, 3, 0, 2, 5], 0.0)]:
        r = R.fast_centroids_ref(s, C, nf)
        assert r.idx.tolist() == idx and r.smax_rest == rest
    assert R.rank_order(np.zeros(4)).tolist() == [0, 1, 2, 3]
    assert R.rank_order(np.full(3, 0.37)).tolist() == [0, 1, 2]


def test_rank_order_agrees_with_the_counting_definition():
    rs = np.random.RandomState(4)
    for k in (2, 5, 67):
        s = rs.randint(0, 4, k) * 0.25        # many ties
        order = R.rank_order(s)
        assert np.array_equal(R.rank_of(s)[order], np.arange(k))


def test_shifts_and_cc_by_hand():
    C = np.array([[0, 0], [3, 4], [0, 0], [-5, 12]], np.float32)
    r = R.fast_centroids_ref(None, C, 2, shift_sq=np.array([4.0, 0.0, 9.0, 0.25]))
    assert r.idx.tolist() == [2, 0] and r.smax_rest == r.shift[3]
    want = np.array([2.0, 0.0, 3.0, 0.5])
    assert (r.shift >= want).all() and (r.shift <= want * (1 + 2e-12)).all()
    assert r.shift[1] == 0.0 and r.shift[0] > 2.0
    inf = np.inf
    assert np.array_equal(r.cc.astype(np.float64),
                          np.array([[0, inf], [5, 5], [inf, 0], [13, 13]], np.float64))
    # long double keeps what fp64 loses: sqrt(1 + 2^-60) = 1 + 2^-61 - ...
    C2 = np.array([[1, 0], [0, 2.0 ** -30]], np.float32)
    t = R.cc_true(C2, [1])[0, 0]
    assert t > 1 and abs(t - 1 - LD(2.0) ** -61) <= LD(2.0) ** -63


# --------------------------------------------------------------- beta, dsh, dq
def _one(C_prev, C_new, alpha=1.0, d_pad=4):
    C_prev, C_new = np.asarray(C_prev, np.float32), np.asarray(C_new, np.float32)
    ref = R.ShiftOperandRef(C_prev.shape[0], C_prev.shape[1], d_pad, 2, alpha)
    return ref.update(C_prev, C_new, 1, 0b10)[1], ref


def test_beta_at_a_power_of_two_amax():
    below = np.float32(0.5) - np.float32(2.0 ** -25)      # one fp32 ulp below 1/2
    o, _ = _one([[0, 0], [0, 0], [0, 0], [1, 1]], [[0.5, 0.25], [below, 0.25], [0, 0], [1, 1]])
    # amax = 1/2 = 0.5 * 2^0: ex2 = 0, beta = 2^14; an ulp below: ex2 = -1, beta = 2^15;
    # amax = 0: beta = 1
    assert o.log2_beta.tolist() == [14, 15, 0, 0]
    assert o.inv.tolist() == [2.0 ** -14, 2.0 ** -15, 1.0, 1.0]
    assert o.dsh[0].tolist() == [8192.0, 4096.0, 0.0, 0.0]
    # 2^15 (1/2 - 2^-25) = 16384 - 2^-10 is an fp32 number; its fp16 image is 16384
    assert o.dsh[1].tolist() == [16384.0, 8192.0, 0.0, 0.0]
    assert not o.dsh[2:].any()
    o8, _ = _one([[0, 0]], [[0.5, 0.25]], alpha=0.125)
    assert o8.inv.tolist() == [2.0 ** -11]


def test_operand_terms_by_hand():
    o, _ = _one([[3, 4]], [[6, 8]])
    assert o.q[0] == 75 and o.nrm[0] == 125 and o.norm[0] == 5 and o.amax[0] == 4
    # amax = 4 = 0.5 * 2^3: beta = 2^11; 2^11 * (3, 4) are fp16 numbers: e = 0
    assert o.log2_beta[0] == 11 and R.operand_error(o.S, o.dsh, o.beta)[0] == 0
    # S = (1 + 2^-12, 0): beta = 2^13, beta S = 8194 -> fp16 8192 (ulp 8): e = 2^-12
    o, _ = _one([[0, 0]], [[1 + 2.0 ** -12, 0]])
    assert o.dsh[0, 0] == 8192.0 and R.operand_error(o.S, o.dsh, o.beta)[0] == 2.0 ** -12
    # double rounding is part of the definition: 2^13 (1 + 2^-11 + 2^-24) is not an
    # fp32 number; fp32 takes it to the fp16 tie 8196, which goes to even (8192);
    # one rounding would give 8200
    o, _ = _one([[-2.0 ** -24, 0]], [[1 + 2.0 ** -11, 0]])
    assert o.S[0, 0] == 1 + LD(2.0) ** -11 + LD(2.0) ** -24 and o.log2_beta[0] == 13
    assert o.dsh[0, 0] == 8192.0
    # a coordinate 2^-30 of amax has a SUBNORMAL fp16 image (beta amax >= 2^13, so
    # the image is 2^-17 or more: 128 fp16 subnormal steps); 2^-42 of amax: zero
    o, _ = _one([[0, 0, 0]], [[0.125, 2.0 ** -33, 2.0 ** -45]])
    assert o.log2_beta[0] == 16
    assert o.dsh[0].tolist() == [8192.0, 2.0 ** -17, 0.0, 0.0]


def test_q_keeps_its_digits_under_cancellation():
    # c = 1e4 + 2^-10 against 1e4: q = 2^-10 (2e4 + 2^-10) exactly
    o, _ = _one([[1e4]], [[1e4 + 2.0 ** -10]])
    assert o.q[0] == LD(2.0) ** -10 * (LD(2e4) + LD(2.0) ** -10)
    assert float(o.q[0]) != float(np.float32(1e4 + 2.0 ** -10) ** 2 - np.float32(1e4) ** 2)


# ------------------------------------------------------------------- the ring
def test_engine_rule():
    assert R.engine_valid(5, 3, 5) == (2, 0b100, {2: 5})
    assert R.engine_valid(6, 3, 5) == (0, 0b101, {2: 5, 0: 6})
    assert R.engine_valid(7, 3, 5) == (1, 0b011, {0: 6, 1: 7})
    assert R.engine_valid(8, 3, 8) == (2, 0b100, {2: 8})        # rlo jumped
    assert R.engine_valid(7, 2, 2) == (1, 0b10, {1: 7})
    assert R.engine_valid(7, 8, 2) == (7, 0xFC, {b: b for b in range(2, 8)})
    assert R.engine_valid(10, 8, 2)[1] == 0b11110111            # bases 4 .. 10


def test_two_update_ring():
    c5 = np.array([[1, 2], [10, 20]], np.float32)
    c6 = np.array([[2, 2], [10, 21]], np.float32)
    c7 = np.array([[4, 1], [10, 21]], np.float32)
    ref = R.ShiftOperandRef(2, 2, 2, 3, 1.0)
    o = ref.update(c5, c6, *R.engine_valid(5, 3, 5)[:2])
    assert sorted(o) == [2] and sorted(ref.snap) == [2]
    assert o[2].S.tolist() == [[1, 0], [0, 1]]
    o = ref.update(c6, c7, *R.engine_valid(6, 3, 5)[:2])
    assert sorted(o) == [0, 2]
    assert np.array_equal(ref.snap[2], c5) and np.array_equal(ref.snap[0], c6)
    assert o[0].S.tolist() == [[2, -1], [0, 0]]          # c(7) - c(6)
    assert o[2].S.tolist() == [[3, -1], [0, 1]]          # c(7) - c(5): accumulated
    assert o[2].q.tolist() == [16 + 1 - 1 - 4, 441 - 400]
    assert o[0].log2_beta.tolist() == [12, 0] and o[2].log2_beta.tolist() == [12, 13]
    # slot 2 is fresh again at t = 8 and only then loses c(5)
    c8 = c7 + 1
    ref.update(c7, c8, *R.engine_valid(7, 3, 5)[:2])
    assert np.array_equal(ref.snap[2], c5)
    ref.update(c8, c8, *R.engine_valid(8, 3, 5)[:2])
    assert np.array_equal(ref.snap[2], c8)
    with pytest.raises(ValueError):
        ref.update(c8, c8, 0, 0b100)


def test_exponent_spread():
    a = np.array([[1, 0, 1], [1, 2.0 ** -29, 3], [1, 2.0 ** -30, 3]], np.float32)
    b = np.array([[2.0 ** 29, 5, 0], [1, 1.5, 3], [1, 1, 3]], np.float32)
    assert R.exponent_spread_ok(a, b).tolist() == [True, True, False]


# ------------------------------------- preconditions of the GPU case matrix
def test_fast_centroid_patterns_do_what_their_names_say():
    for k, nf in [(5, 3), (67, 16), (300, 7)]:
        s = R.shift_sq_pattern("dup_at_nf", k, nf)
        o = R.rank_order(s)
        assert s[o[nf - 1]] == s[o[nf]] == s[o[nf + 1]] and o[nf - 1] < o[nf] < o[nf + 1]
        C = R.centre_pattern("identical_pair", k, 63, int(o[0]))
        assert np.array_equal(C[o[0]], C[(o[0] + 1) % k])
        far = R.cc_true(R.centre_pattern("offset_1e4", k, 63, None), o[:nf])
        far = far[np.isfinite(far)]
        assert far.max() <= 2.0 ** -8 and np.median(far) >= 2.0 ** -10
    assert (R.shift_sq_pattern("one_zero", 67, 16) == 0).sum() == 1


@pytest.mark.parametrize("d", [1, 63, 128, 200])
@pytest.mark.parametrize("k", [1, 5, 67])
def test_operand_sequences_hold_every_edge(k, d):
    seq, kinds = R.operand_sequence(k, d)
    assert len(seq) == R.N_UPDATES + 1 and all(c.dtype == np.float32 for c in seq)
    assert set(kinds.ravel().tolist()) == set(range(6))
    seen = dict(still=0, ulp=0, pow2=0, below=0, sub=0, zero=0, tie=0, wild=0, cancel=0)
    for u in range(R.N_UPDATES):
        a, b = seq[u], seq[u + 1]
        S = R.wide(b) - R.wide(a)
        amax = np.abs(S).max(1)
        fr, ex = np.frexp(amax)
        ok = R.exponent_spread_ok(a, b)
        kd = kinds[u]
        # (a coordinate that WILD left tiny puts later updates of that centroid
        # outside the range too: the counters take the in-range pairs only)
        assert (amax[kd == R.STILL] == 0).all()
        one = kd == R.ULP
        assert ((S[one] != 0).sum(1) == 1).all()
        assert (b[one, 0] == np.nextafter(a[one, 0], np.float32(np.inf))).all()
        seen["still"] += int((ok & (kd == R.STILL)).sum())
        seen["ulp"] += int((ok & one).sum())
        seen["pow2"] += int((ok & (kd == R.POW2) & (fr == 0.5)).sum())
        # one fp32 ulp of the moved coordinate below 2^ex
        ulp0 = np.spacing(np.maximum(np.abs(a[:, 0]), np.abs(b[:, 0])))
        seen["below"] += int((ok & (kd == R.BELOW) & (fr > 0.5)
                              & (np.ldexp(LD(1), ex) - amax <= ulp0)).sum())
        seen["wild"] += int((~ok & (kd == R.WILD)).sum())
        seen["cancel"] += int((ok & (kd == R.CANCEL) & (np.abs(a).max(1) > 9e3) & (amax > 0)
                               & (amax <= 2.0 ** -8)).sum())
        if d >= 4:
            p = ok & (kd == R.POW2)
            # the double-rounding coordinate: beta S = 1 + 2^-11 + 2^-24 with beta = 2^16
            seen["tie"] += int((p & (fr == 0.5) & (ex == -2)
                                & (S[:, d - 3] * 2.0 ** 16 == 1 + LD(2.0) ** -11 + LD(2.0) ** -24)).sum())
            seen["sub"] += int((np.abs(S[p, d - 1]) == amax[p] * LD(2.0) ** -30).sum())
            seen["zero"] += int((np.abs(S[p, d - 2]) == amax[p] * LD(2.0) ** -42).sum())
    assert all(seen[n] for n in ("still", "ulp", "pow2", "below", "wild", "cancel")), seen
    assert d < 4 or (seen["sub"] and seen["zero"] and seen["tie"]), seen


@pytest.mark.parametrize("ring", [2, 3, 8])
@pytest.mark.parametrize("k,d,d_pad", [(1, 1, 128), (5, 63, 128), (67, 200, 256)])
def test_wild_pairs_keep_a_real_fp16_error(k, d, d_pad, ring):
    """Outside the fp64-exact range a coordinate of the kernel's S carries a
    2^-53 relative error.  Its e_j (slack 2^-20 - 2^-23 relative) stays sound
    where the fp16 rounding error it measures is far larger: 2^-53 |S| over
    those coordinates is at most 2^-22 e on every such (slot, centroid)."""
    seq, _ = R.operand_sequence(k, d)
    ref = R.ShiftOperandRef(k, d, d_pad, ring, 1.0)
    rlo, wild = R.T0, 0
    for u in range(R.N_UPDATES):
        t = R.T0 + u
        rlo = t if t == R.RLO_JUMP_AT else rlo
        snew, valid, _ = R.engine_valid(t, ring, rlo)
        for o in ref.update(seq[u], seq[u + 1], snew, valid).values():
            e = R.operand_error(o.S, o.dsh, o.beta)
            w = ~o.in_range
            wild += int(w.sum())
            assert (o.wild_norm[w] > 0).all() and (o.wild_norm[~w] == 0).all()
            assert (LD(2.0) ** -53 * o.wild_norm[w] <= LD(2.0) ** -22 * e[w]).all()
    assert wild > 0


@pytest.mark.parametrize("case", ["d8", "d64"])
def test_filter_geometry_keeps_enough_rows(case):
    g = R.filter_geometry(case)
    held = {nf: R.filter_rule_ref(g, nf) for nf in (0, 3, 16)}
    share = {nf: h.mean() for nf, h in held.items()}
    print(case, {nf: f"{100 * s:.1f} %" for nf, s in share.items()})
    assert share[0] >= 0.10
    if case == "d8":
        assert share[16] >= 0.50
    for nf, h in held.items():
        assert all(len(bad) == 0 for bad in R.filter_unsound_rows(g, h)), nf
    assert not (held[0] & ~held[3]).any() and not (held[0] & ~held[16]).any()
    # the exact bounds bracket the truth under C_old
    D0 = R.sq_dists(g.X, g.C_old)
    ar = np.arange(g.n)
    assert (R.wide(g.ub) >= np.sqrt(D0[ar, g.labels])).all()
    D0[ar, g.labels] = np.inf
    assert (R.wide(g.lb) <= np.sqrt(D0.min(1))).all()


@pytest.mark.parametrize("d_pad", [128, 256])
def test_gap_geometry_leaves_rows_to_resolve(d_pad):
    g = R.gap_geometry(d_pad)
    m, margin = R.gap_true_margin(g)
    share = (margin > R.GAP_DELTA + 1).mean()
    print(d_pad, f"{100 * share:.1f} % of the rows have every gap above delta + 1")
    assert share >= 0.25
    assert set(g.base.tolist()) == {3, 4} and set(g.c_r.tolist()) == {2, 3, 4}
    assert (g.rec[:, 2:6] >= 0).all() and (g.rec[np.arange(g.n), 2 + g.slot] == 0).all()
    assert (m != g.slot).any()      # some rows change their argmin by the new centres
