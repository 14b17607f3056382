"""The numpy reference of the sampling layer (tests/_qrand_ref.py) against the
published Philox known answers, the project's torch twins, and the conditions
its case matrix has to meet before the device tests
(test_qrand_kernels_gpu.py) may lean on it.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _qrand_ref as R
from sq_learn_amd.ops import random as OPS
from sq_learn_amd.runtime.rng import Philox, RngKey, philox4x32


def twin_key(key):
    k = RngKey.__new__(RngKey)
    k.k0, k.k1 = key[0], key[1]
    k.stream = key[2] | (key[3] << 32)
    assert k.as_tuple() == tuple(key)
    return k


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", R.KAT)
def test_known_answers(ctr, key, want):
    assert R.philox4x32_10(ctr, key) == want
    assert tuple(int(w) for w in R.philox_blocks(*ctr, *key)) == want
    assert tuple(int(w) for w in philox4x32(*ctr, *key)) == want


def test_vector_philox_is_the_scalar_one():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    k = [int(v) for v in rng.integers(0, 2 ** 32, size=2, dtype=np.uint64)]
    got = R.philox_blocks(c[:, 0], c[:, 1], c[:, 2], c[:, 3], *k)
    for i in range(64):
        assert tuple(int(w) for w in got[i]) == R.philox4x32_10([int(v) for v in c[i]], k)


def test_all_ones_counter_is_not_an_element_id():
    # word(e) puts e >> 2 into the counter, so its second word stays below
    # 2^30; the all-ones vector is checked on the reference only, and the
    # device runs the last block there is, (ffffffff, 3fffffff)
    e = R._ids(2 ** 64 - 4, 4)
    assert int(e[0] >> np.uint64(2)) == (0xFFFFFFFF | (0x3FFFFFFF << 32))
    w = R.flat_words(R.KEY_ONES, 2 ** 64 - 4, 4)
    assert tuple(int(v) for v in w) == R.philox4x32_10((0xFFFFFFFF, 0x3FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF),
                                                       (0xFFFFFFFF, 0xFFFFFFFF))


@pytest.mark.parametrize("offset", R.FLAT_OFFSETS)
def test_flat_streams_match_the_twins(offset):
    key = twin_key(R.KEY_U)
    for n in R.FLAT_N:
        w = R.flat_words(R.KEY_U, offset, n)
        t64 = Philox(key).uniform_flat(n, offset=offset, dtype=torch.float64).numpy()
        t32 = Philox(key).uniform_flat(n, offset=offset).numpy()
        assert np.array_equal(t64, R.u01(w))
        assert np.array_equal(t32.astype(np.float64), R.u01_f32(w))
        assert np.all((t64 > 0) & (t64 < 1))
    n = 257
    z = Philox(twin_key(R.KEY_N)).normal_flat(n, offset=offset, dtype=torch.float64).numpy()
    ref, _, _ = R.normal_ref(R.KEY_N, offset, n, exact_u=True)
    np.testing.assert_allclose(z, ref, rtol=1e-12, atol=1e-14)
    for b in R.TN_BOUNDS:
        x = torch.zeros(n, dtype=torch.float64)
        OPS.trunc_normal_add_(x, b, twin_key(R.KEY_T), offset=offset)
        np.testing.assert_allclose(x.numpy(), R.trunc_normal_ref(R.KEY_T, offset, n, b, exact_u=True),
                                   rtol=1e-9, atol=1e-12)


def test_fp32_uniform_rounding():
    w = np.array([0, 0xFF, (2 ** 23 - 1) << 8, (2 ** 23) << 8, (2 ** 23 + 1) << 8, 0xFFFFFFFF],
                 dtype=np.uint64)
    exact, held = R.u01(w), R.u01_f32(w)
    assert np.array_equal(held[:3], exact[:3])
    assert np.array_equal(np.abs(held[3:] - exact[3:]), np.full(3, 2.0 ** -25))
    assert held[-1] == 1.0 and exact[-1] < 1.0


def test_smallest_uniform_block():
    blk = R._blocks_of(R.KEY_N, np.array([R.SMALLEST_U1_BLOCK], dtype=np.uint64))[0]
    assert int(blk[0]) >> 8 == 0
    _, r, u1 = R.normal_ref(R.KEY_N, 2 * R.SMALLEST_U1_BLOCK, 2)
    assert u1[0] == 0.5 * 2.0 ** -24
    assert abs(r[0] - math.sqrt(50 * math.log(2.0))) < 1e-14


def test_erfinv_inverts_erf():
    p = np.concatenate([np.linspace(-1 + 2.0 ** -24, 1 - 2.0 ** -24, 4001), [0.0, 1e-12, -1e-300]])
    x = R.erfinv(p)
    back = np.array([math.erf(v) for v in x])
    # to a few ulp of p itself: 1e-15 in erf, so at most 1e-15 * slope
    # <= 3e-9 in x at the far end |x| = 3.83 the 24-bit uniforms reach
    assert np.all(np.abs(back - p) <= 1e-15)
    slope = math.sqrt(math.pi) / 2 * np.exp(x * x)
    assert np.abs(x).max() < 3.84 and 1e-15 * slope.max() < 3e-9
    assert np.all(np.abs(R.erf(x) - back) <= 1e-15)


# ------------------------------------------------------------------ Fejer
def test_walk_cdf_is_the_fejer_law():
    from sq_learn_amd.quantum.fejer import fejer_pmf
    for M, omega in ((41, 3.25), (128, 40.2048), (1000, 7.9), (314160, 3 + 1e-3)):
        p = fejer_pmf(omega, M)
        base = int(math.floor(omega))
        want = np.cumsum(p[np.mod(base + R.WALK_OFFS, M)])
        np.testing.assert_allclose(R.fejer_walk_cdf(omega, M), want, rtol=1e-9)
        offs, pt = R.tail_pmf(omega - base, M)
        # fejer_pmf's numerator sin(M dist pi) loses log10(M) digits far out
        np.testing.assert_allclose(pt, p[np.mod(base + offs, M)] / p[np.mod(base + offs, M)].sum(),
                                   rtol=1e-6)
        assert offs.size == M - R.WALK_OFFS.size


def test_margin_is_derived_and_small():
    assert R.walk_delta() <= R.DELTA <= 1e-5
    assert 66 * R.DELTA < 0.0007


CASES = R.fejer_cases()
CASE_IDS = [c["name"] for c in CASES]


def test_case_matrix_is_the_one_asked_for():
    names = set(CASE_IDS)
    assert len(names) == len(CASE_IDS)
    for M in (64, 128, 2 ** 20, 2 ** 30, 2 ** 40):
        for phi in R.PHI_GENERIC:
            assert f"generic-M{M}-phi{phi:.4f}" in names
    for M in R.NEAR_M:
        for phi in R.NEAR_LOW:
            assert f"nearbin-M{M}-phi{phi:g}" in names
        for d in R.NEAR_HIGH:
            assert f"nearbin-M{M}-1mphi{d:g}" in names
    for Q in (1, 3, 13, 31, 2, 4):
        for off in (0, 7, 2 ** 32 - 3):
            assert f"reps-Q{Q}-off{off}" in names
    small = R.evaluate(CASE_IDS.index("small-ae-eps0.1"))
    assert np.all(small["M"] == 35)
    het = CASES[CASE_IDS.index("hetero-m")]
    assert set(het["m"].tolist()) == {1, 5, 7, 20, 33}
    assert set(CASES[CASE_IDS.index("hetero-eps")]["eps"].tolist()) == {0.1, 0.02, 1e-3, 1e-5}
    assert CASES[CASE_IDS.index("launch-tail-n257")]["x"].shape == (257,)


@pytest.mark.parametrize("index", range(len(CASES)), ids=CASE_IDS)
def test_case_conditions_and_twin(index):
    ev = R.evaluate(index)
    c = ev["case"]
    n = c["x"].shape[0]
    # condition 1: the excused share
    for d in ev["draws"]:
        assert d["near"].mean() < 0.002
        tight = (d["branch"] == R.SMALL) | (d["branch"] == R.TAIL)
        assert not np.any(tight & (d["margin"] <= R.TIGHT) & ~ev["skip"])
    if c["name"].startswith("nearbin"):
        # the phase that fp64 yields is the one the name states, and (condition
        # 3) no first uniform is small enough to pass the heavy bin by
        phi = ev["omega"] - np.floor(ev["omega"])
        side, want = c["phase"]
        got = phi if side == "phi" else 1.0 - phi
        assert np.all(np.abs(got - want) <= 1e-3 * want)
        assert R.SampleWords(c["key"], R._ids(c["offset"], n)).u(0).min() >= R.DELTA
        heavy = ev["draws"][0]["ell"] == (0 if side == "phi" else 1)
        assert heavy.mean() > 0.99 or want >= 1e-3
    if c["name"].startswith("tail"):
        assert int((ev["draws"][0]["branch"] == R.TAIL).sum()) >= 200
    # the torch twin draws the same bins
    key = twin_key(c["key"])
    x = torch.tensor(c["x"])
    if c["op"] == "pe":
        out = OPS.phase_estimation_batch(x, torch.tensor(c["m"]), key, offset=c["offset"])
    else:
        out = OPS.amplitude_estimation_batch(x, torch.tensor(c["eps"]), key, Q=c["Q"],
                                             offset=c["offset"])
    bad, excused, off = R.compare(out.numpy(), ev)
    assert bad.size == 0, (c["name"], bad[:8], out.numpy()[bad[:8]], ev["value"][bad[:8]])
    assert excused < 0.002
    # the twin is fp64 throughout: only draws within 1e-9 of a boundary may move
    moved = np.abs(out.numpy() - ev["value"]) > R.VALUE_TOL
    assert np.all(np.min([d["margin"] for d in ev["draws"]], axis=0)[moved] < 1e-9)


def test_branch_coverage():
    # condition 2
    count = dict(exact=0, small=0, l0=0, plus=0, minus=0, tail=0)
    for i in range(len(CASES)):
        ev = R.evaluate(i)
        for d in ev["draws"]:
            b, ell = d["branch"][~ev["skip"]], d["ell"][~ev["skip"]]
            count["exact"] += int((b == R.EXACT).sum())
            count["small"] += int((b == R.SMALL).sum())
            count["tail"] += int((b == R.TAIL).sum())
            count["l0"] += int(((b == R.WALKED) & (ell == 0)).sum())
            count["plus"] += int(((b == R.WALKED) & (ell > 0)).sum())
            count["minus"] += int(((b == R.WALKED) & (ell < 0)).sum())
    assert min(count.values()) >= 50, count


def test_sample_ids_cross_the_masked_bits():
    # (offset + i) Q + q above 2^32 puts bits into the 16 masked counter bits
    c = CASES[CASE_IDS.index(f"reps-Q31-off{2 ** 32 - 3}")]
    ids = R._ids(c["offset"], 4) * np.uint64(31)
    assert int(ids[0]) >> 32 == 30 and int(ids[3]) >> 32 == 31
    a = R.SampleWords(c["key"], ids).words(5)
    k0, k1, s0, s1 = c["key"]
    for i in range(4):
        s = int(ids[i])
        blk = R.philox4x32_10((s & R.MASK32, ((s >> 32) & 0xFFFF) | (1 << 16), s0, s1), (k0, k1))
        assert int(a[i]) == blk[1]


# ------------------------------------------------------------------ contracts of the CPU path
@pytest.mark.parametrize("Q", [2, 4])
def test_even_q_averages_the_middle_pair(Q):
    # numpy.median, as the reference project's median evaluation
    assert R.median_ref(np.array([[3.0], [1.0], [2.0], [7.0]])[:Q])[0] == (2.0 if Q == 2 else 2.5)
    ev = R.evaluate(CASE_IDS.index(f"reps-Q{Q}-off7"))
    c = ev["case"]
    out = OPS.amplitude_estimation_batch(torch.tensor(c["x"]), torch.tensor(c["eps"]),
                                         twin_key(c["key"]), Q=Q, offset=7).numpy()
    reps = np.stack([R.ae_value(d["bin"], ev["M"]) for d in ev["draws"]])
    srt = np.sort(reps, axis=0)
    want = 0.5 * (srt[Q // 2 - 1] + srt[Q // 2])
    sure = ev["lo"] == ev["hi"]
    assert sure.mean() > 0.99
    np.testing.assert_allclose(out[sure], want[sure], rtol=0, atol=R.VALUE_TOL)
    # not the lower middle value wherever the pair differs
    differ = sure & (srt[Q // 2] - srt[Q // 2 - 1] > 1e-9)
    assert differ.sum() > 100 and np.all(out[differ] > srt[Q // 2 - 1][differ])


def test_phase_estimation_rejects_unsupported_m():
    om = torch.full((4,), 0.3, dtype=torch.float64)
    key = twin_key(R.KEY_F)
    for bad in (41, 64, -1):
        m = torch.tensor([7, 7, bad, 7], dtype=torch.int32)
        with pytest.raises(ValueError):
            OPS.phase_estimation_batch(om, m, key)
    OPS.phase_estimation_batch(om, torch.tensor([0, 1, 40, 7], dtype=torch.int32), key)
