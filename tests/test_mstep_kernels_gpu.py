"""The fixed-point M-step kernels of csrc/kmeans.hip against the integer
references of ``_mstep_ref.py`` (run on an MI355X).

The ops of ``ops/kmeans.py`` are called directly, the exponents derived as
the engine derives them.  Every fixed-point quantity (sums, counts, qsum, the
packed sums and counts, prev) is compared with ``equal``: the device adds
integer-valued fp64 quanta, the reference the same integers in int64, and
``test_mstep_ref_cpu.py`` checks that no partial sum can reach 2^53.  Only
the floating-point outputs (inertia parts, shifts, norms) carry a bound,
stated next to each comparison.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mstep_ref as R
from _dense_ref import U32, U64, gamma

pytestmark = pytest.mark.gpu

K0 = R.K0
_VALUES = {}


def _K():
    from sq_learn_amd.ops import kmeans as K
    return K


def _values(vp, n, d, bf16=False):
    key = (vp, n, d, bf16)
    if key not in _VALUES:
        _VALUES[key] = R.make_values(vp, n, d, bf16=bf16)
    return _VALUES[key]


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float64))


def _assert_equal(got, ref, what):
    """Bitwise equality of a device fp64 tensor and an integer / fp64 array."""
    g = got.detach().cpu().reshape(-1)
    r = _f64(ref).reshape(-1)
    if not torch.equal(g, r):
        bad = torch.nonzero(g != r).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} entries differ, first at "
                             f"{i}: got {g[i].item()!r}, reference {r[i].item()!r}")


def _reduce(cuda, X32, bf16, lab, w, k, ws=None, mind=None, C_old=None):
    """One ``centroid_reduce_native`` call on outputs prefilled with 7.0."""
    K = _K()
    n, d = X32.shape
    Xg = torch.from_numpy(X32).to(cuda)
    if bf16:
        Xg = Xg.to(torch.bfloat16)
        assert np.array_equal(Xg.float().cpu().numpy(), X32)     # the values were bf16 already
    labg = torch.from_numpy(lab).to(cuda)
    wg = None if w is None else torch.from_numpy(w).to(cuda)
    if ws is None:
        ws = K.ReduceWorkspace(n, k, cuda)
    ws.set_scale(float(np.abs(X32).max()) if n else 0.0, n, None if w is None else float(w.max()))
    sums = torch.full((k, d), 7.0, dtype=torch.float64, device=cuda)
    counts = torch.full((k,), 7.0, dtype=torch.float64, device=cuda)
    K.centroid_reduce_native(Xg, labg, wg, sums, counts, k, ws, mind=mind, C_old=C_old)
    torch.cuda.synchronize()
    return ws, sums, counts


def _check_reduce(cuda, dt, n, d, k, lp, vp, wk, ws=None):
    K = _K()
    bf16 = dt == "bf16"
    X32 = _values(vp, n, d, bf16)
    lab = R.make_labels(lp, n, k)
    w = R.make_weights(wk, n)
    ws, sums, counts = _reduce(cuda, X32, bf16, lab, w, k, ws=ws)
    if vp == "halves" and not bf16:
        assert ws.xexp == R.HALVES_XEXP
    wexp = ws.wexp if w is not None else 0
    S, N, bound = R.reduce_ref(X32, lab, k, w, ws.xexp, wexp)
    assert bound < R.LIMIT            # the precondition of exactness
    tag = f"{dt} n={n} d={d} k={k} {lp} {vp} w={wk}"
    _assert_equal(sums, S, "sums " + tag)
    _assert_equal(counts, N, "counts " + tag)
    if w is None:
        members = np.bincount(lab[(lab >= 0) & (lab < k)], minlength=k)
        _assert_equal(counts, members, "member counts " + tag)
    # the packed bucket: exact rescaling by the quanta, the inertia passed through
    inertia = torch.tensor([1.0 / 3.0], dtype=torch.float64, device=cuda)
    packed = torch.full((k * d + k + 1,), 7.0, dtype=torch.float64, device=cuda)
    K.pack_stats_native(sums, counts, inertia, packed, k, d, ws, weighted=w is not None)
    ref = np.concatenate([(S.astype(np.float64) * 2.0 ** ws.xexp).ravel(),
                          N.astype(np.float64) * 2.0 ** wexp, [1.0 / 3.0]])
    _assert_equal(packed, ref, "packed " + tag)
    return ws


# ------------------------------------------------- (a) the segmented reduce
def _reduce_groups():
    groups = {}
    for dt, n, d, k, lp, vp, wk in R.reduce_cases():
        groups.setdefault((dt, n, d, k), []).append((lp, vp, wk))
    return groups


_GROUPS = _reduce_groups()


@pytest.mark.parametrize("dt,n,d,k", sorted(_GROUPS), ids=lambda v: str(v))
def test_reduce_equals_integer_reference(cuda, dt, n, d, k):
    """sq_centroid_reduce at every dispatch branch (segment_sum_kernel<T, LPR>
    for LPR 1..32, the whole-wave rows kernels of both types with one,
    partial and several column passes), both sides of the 8192-row histogram
    chunk, every label and value pattern, unweighted and weighted."""
    for lp, vp, wk in _GROUPS[(dt, n, d, k)]:
        _check_reduce(cuda, dt, n, d, k, lp, vp, wk)


def test_reduce_rejects_k_above_the_limit(cuda):
    K = _K()
    n, d, k = 100, 4, 16385
    X = torch.zeros(n, d, device=cuda)
    lab = torch.zeros(n, dtype=torch.int32, device=cuda)
    ws = K.ReduceWorkspace(n, k, cuda)
    sums = torch.zeros(k, d, dtype=torch.float64, device=cuda)
    counts = torch.zeros(k, dtype=torch.float64, device=cuda)
    with pytest.raises(RuntimeError):
        K.centroid_reduce_native(X, lab, None, sums, counts, k, ws)


def test_reduce_workspace_reuse(cuda):
    """One workspace, three reduces in a row: a histogram the scan did not
    re-zero or a stale permutation tail read past the scanned total would
    show in the second or third."""
    ws = None
    for lp in ("random", "with_invalid", "all_invalid"):
        ws = _check_reduce(cuda, "f32", 8193, 20, K0, lp, "normal", "none", ws=ws)
    for lp in ("random", "with_invalid", "all_invalid", "random"):
        ws = _check_reduce(cuda, "f32", 8193, 20, K0, lp, "normal", "rand", ws=ws)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_reduce_empty_shard_overwrites_outputs(cuda, dt):
    """n == 0: the outputs are overwritten like at any other n (an empty
    shard's zeros enter the all-reduce)."""
    d = 16
    _, sums, counts = _reduce(cuda, np.zeros((0, d), dtype=np.float32), dt == "bf16",
                              np.zeros(0, dtype=np.int32), None, K0)
    assert torch.equal(sums, torch.zeros_like(sums))
    assert torch.equal(counts, torch.zeros_like(counts))


# ------------------------------------------------------ (b) fused exact mind
@pytest.mark.parametrize("d", [16, 32, 64, 128, 252, 256])
def test_reduce_fused_mind(cuda, d):
    """The row pass fills mind where the E-step left it negative: the lanes
    beyond the row (4 lane >= d) are outside the column loop while the others
    run the wave sum, at every padded width below 256."""
    n, k = 8193, K0
    X32 = _values("normal", n, d)
    lab = R.make_labels("with_invalid", n, k)
    rng = np.random.RandomState(5)
    C = (rng.standard_normal((k, d)) * 3).astype(np.float32)
    mind0 = np.full(n, 123.25, dtype=np.float32)
    mind0[::3] = -1.0
    mind = torch.from_numpy(mind0).to(cuda)
    ws, sums, counts = _reduce(cuda, X32, False, lab, None, k, mind=mind,
                               C_old=torch.from_numpy(C).to(cuda))
    S, N, bound = R.reduce_ref(X32, lab, k, None, ws.xexp, 0)
    assert bound < R.LIMIT
    _assert_equal(sums, S, "sums")
    _assert_equal(counts, N, "counts")
    got = mind.cpu().numpy()
    marked = mind0 < 0
    keep = ~marked | (lab < 0)
    # sentinels and the rows without a label: untouched bit for bit
    assert np.array_equal(got[keep].view(np.uint32), mind0[keep].view(np.uint32))
    rows = np.nonzero(marked & (lab >= 0))[0]
    assert rows.size > 2000
    diff = X32[rows].astype(np.float64) - C[lab[rows]].astype(np.float64)
    ref = np.array([math.fsum(r) for r in diff * diff]).astype(np.float32)
    # the device sums the exact fp64 squares in fp64 (error ~ d 2^-53, far
    # below half an fp32 ulp) and rounds once: at most the neighbouring fp32
    err = np.abs(got[rows].astype(np.float64) - ref.astype(np.float64))
    assert (err <= np.spacing(ref).astype(np.float64)).all(), float(err.max())
    assert (got[rows] == ref).mean() > 0.999


# ------------------------------------------------ (c) the incremental update
class _Delta:
    """Device buffers of one incremental sequence and the reference state."""

    def __init__(self, cuda, n, d, k, X32=None):
        K = _K()
        self.n, self.d, self.k, self.cuda = n, d, k, cuda
        self.X32 = _values("normal", n, d) if X32 is None else X32
        mx = float(np.abs(self.X32).max())
        self.Xg = torch.from_numpy(self.X32).to(cuda)
        self.ws = K.ReduceWorkspace(n, k, cuda).set_scale(mx, n, None)
        self.qexp = K.fixed_point_exp(mx ** 2 * d, n)
        self.sums = torch.zeros(k, d, dtype=torch.float64, device=cuda)
        self.counts = torch.zeros(k, dtype=torch.float64, device=cuda)
        self.qsum = torch.zeros(k, dtype=torch.float64, device=cuda)
        self.prev = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        self.perm2 = torch.empty(4 * n, dtype=torch.int32, device=cuda)
        self.S = np.zeros((k, d), dtype=np.int64)
        self.N = np.zeros(k, dtype=np.int64)
        self.Q = np.zeros(k, dtype=np.int64)
        self.prev_ref = np.full(n, -1, dtype=np.int32)

    def clone(self):
        c = object.__new__(_Delta)
        c.__dict__.update(self.__dict__)
        for name in ("sums", "counts", "qsum", "prev"):
            setattr(c, name, getattr(self, name).clone())
        c.perm2 = torch.empty_like(self.perm2)
        c.ws = _K().ReduceWorkspace(self.n, self.k, self.cuda, xexp=self.ws.xexp)
        return c

    def run(self, lab, lists=None):
        labg = torch.from_numpy(lab).to(self.cuda)
        _K().centroid_delta_native(self.Xg, labg, self.prev, self.sums, self.counts, self.qsum,
                                   self.k, self.ws, self.perm2, self.qexp, lists=lists)
        torch.cuda.synchronize()

    def advance_ref(self, lab):
        self.S, self.N, self.Q = R.delta_ref(self.S, self.N, self.Q, self.X32, lab, self.prev_ref,
                                             self.k, self.ws.xexp, self.qexp)
        self.prev_ref = lab.copy()

    def check(self, tag, full=True):
        _assert_equal(self.sums, self.S, "sums " + tag)
        _assert_equal(self.counts, self.N, "counts " + tag)
        _assert_equal(self.qsum, self.Q, "qsum " + tag)
        assert np.array_equal(self.prev.cpu().numpy(), self.prev_ref), "prev " + tag
        if full:
            S, N, bound = R.reduce_ref(self.X32, self.prev_ref, self.k, None, self.ws.xexp, 0)
            assert bound < R.LIMIT
            _assert_equal(self.sums, S, "sums vs full reduce " + tag)
            _assert_equal(self.counts, N, "counts vs full reduce " + tag)
            _assert_equal(self.qsum, R.qsum_ref(self.X32, self.prev_ref, self.k, self.qexp),
                          "qsum vs full reduce " + tag)


@pytest.mark.parametrize("n,d", R.delta_shapes(), ids=lambda v: str(v))
def test_delta_sequence(cuda, n, d):
    """delta_segment_kernel<M>, M = 1..4 with full and partial last column
    chunks: every row entering, ~3 % relabelled, nothing moved, a tenth
    leaving to -1, those coming back while others leave, all to one
    cluster - on one set of buffers, each step against ``delta_ref`` and the
    full ``reduce_ref`` / ``qsum_ref`` at its labels."""
    st = _Delta(cuda, n, d, K0)
    for i, lab in enumerate(R.delta_label_steps(n, K0)):
        st.run(lab)
        st.advance_ref(lab)
        st.check(f"n={n} d={d} step {i + 1}")


@pytest.mark.parametrize("k", [1, 1025, 16384])
def test_delta_cluster_counts(cuda, k):
    """The histogram / scatter passes at the smallest and the largest k the
    launcher accepts (delta_scatter_kernel's two LDS arrays take 8 k bytes:
    128 KiB at 16384); k = 16385 is refused."""
    n, d = 20001, 4
    st = _Delta(cuda, n, d, k)
    for i, lab in enumerate(R.delta_label_steps(n, k)[:2]):
        st.run(lab)
        st.advance_ref(lab)
        st.check(f"k={k} step {i + 1}")
    rows = np.arange(0, n, 997)
    lab = st.prev_ref.copy()
    lab[rows] = (lab[rows] + 1) % k if k > 1 else -1
    st.run(lab, lists=[_dev_list(cuda, rows)])          # the list passes at this k
    st.advance_ref(lab)
    st.check(f"k={k} list step")
    if k == 16384:
        big = _Delta(cuda, n, d, k + 1)
        with pytest.raises(RuntimeError):
            big.run(R.make_labels("random", n, k + 1))


def test_delta_long_and_short_lists(cuda):
    """1.06 M entries (every row moves between two valid labels): the
    smallest shape whose entry count / 512 exceeds the 2048-wave floor, so
    the runs spread over the whole grid; then 40 and 5 moved rows in the same
    buffers (runs of the 16-entry minimum, the last below it)."""
    n, d = R.DELTA_LONG
    st = _Delta(cuda, n, d, K0)
    l1 = R.make_labels("random", n, K0)
    l2 = ((l1 + 1) % K0).astype(np.int32)
    l3 = l2.copy()
    l3[np.arange(40) * 13001] = (l3[np.arange(40) * 13001] + 5) % K0
    l4 = l3.copy()
    l4[[7, 70001, 270001, 529998, 529999]] = 0
    l4[[7, 70001, 270001, 529998, 529999]] += (l3[[7, 70001, 270001, 529998, 529999]] == 0)
    for i, lab in enumerate((l1, l2, l3, l4)):
        moved = int((lab != st.prev_ref).sum())
        entries = moved * (1 if i == 0 else 2)
        assert entries == (n, 2 * n, 80, 10)[i]
        st.run(lab)
        st.advance_ref(lab)
        st.check(f"long step {i + 1}", full=i in (1, 3))
    assert 2 * n // 512 > 2048 >= 2 * (n - 6000) // 512


# ------------------------------------------------------------ (d) list form
def _dev_list(cuda, rows, count=None, tail=()):
    """(int64 rows, int32 [1] device length); ``tail`` rows lie beyond it."""
    full = np.concatenate([np.asarray(rows, dtype=np.int64), np.asarray(tail, dtype=np.int64)])
    if full.size == 0:
        full = np.zeros(1, dtype=np.int64)
    c = len(rows) if count is None else count
    return (torch.from_numpy(full).to(cuda), torch.tensor([c], dtype=torch.int32, device=cuda))


LIST_VARIANTS = ("three", "one_none", "count_zero", "single", "len_1_7_8", "len_9_8_7")


@pytest.mark.parametrize("d", [100, 260, 1024])
def test_delta_lists(cuda, d):
    """The list walk (delta_hist_list / delta_scatter_list, 8 entries in
    flight per thread) against the integer reference and the full walk of
    the same update: listed rows that did not move are skipped, a null list
    and a list of device length 0 are empty, rows beyond a list's length are
    never read."""
    n, k = 20001, K0
    steps = R.delta_label_steps(n, k)
    l1, l2 = steps[0], steps[1]
    base = _Delta(cuda, n, d, k)
    base.run(l1)
    base.advance_ref(l1)
    base.check(f"d={d} step 1", full=False)
    rng = np.random.RandomState(7)
    for variant in LIST_VARIANTS:
        if variant.startswith("len_"):
            lens = [int(t) for t in variant.split("_")[1:]]
            ch = np.sort(rng.permutation(n)[:sum(lens)])
            lab = l1.copy()
            lab[ch] = (lab[ch] + 1) % k
            cuts = np.cumsum(lens)[:-1]
            parts = np.split(ch, cuts)
            extra = np.zeros(0, dtype=np.int64)
        else:
            lab = l2
            ch = np.nonzero(l2 != l1)[0]
            same = np.nonzero(l2 == l1)[0]
            extra = same[rng.permutation(same.size)[:500]]       # listed, not moved
            mix = rng.permutation(np.concatenate([ch, extra]))
            parts = np.array_split(mix, 3)
        assert ch.size > 0
        if variant in ("three", "len_1_7_8", "len_9_8_7"):
            lists = [_dev_list(cuda, p, tail=ch[:5]) for p in parts]
        elif variant == "one_none":
            lists = [_dev_list(cuda, np.concatenate(parts[:2])), None, _dev_list(cuda, parts[2])]
        elif variant == "count_zero":
            # the middle list holds moved rows but has length 0: walking it
            # would count them twice
            lists = [_dev_list(cuda, np.concatenate(parts[:2])),
                     _dev_list(cuda, [], count=0, tail=ch[:64]), _dev_list(cuda, parts[2])]
        else:
            lists = [_dev_list(cuda, np.concatenate(parts))]
        st = base.clone()
        st.run(lab, lists=lists)
        st.advance_ref(lab)
        st.check(f"d={d} lists {variant}", full=variant == "three")
        walk = base.clone()
        walk.run(lab)
        for name in ("sums", "counts", "qsum", "prev"):
            assert torch.equal(getattr(st, name), getattr(walk, name)), (variant, name)


# --------------------------------------- (e) cluster parts and the statistics
CORR_N = (1, 1023, 1024, 1025, 8193, 524288 + 5)
_CORR = {}


def _corr(n):
    if n not in _CORR:
        c = (np.random.RandomState(11).standard_normal(n) * 0.25).astype(np.float32)
        _CORR[n] = (c, math.fsum(c.tolist()), math.fsum(np.abs(c).tolist()))
    return _CORR[n]


@pytest.mark.parametrize("k", [1, 37, 65])
@pytest.mark.parametrize("d", [4, 100, 256, 1024])
def test_cluster_parts_and_mstep_stats(cuda, d, k):
    K = _K()
    n = 8193
    st = _Delta(cuda, n, d, k)
    lab = R.make_labels("empty_clusters", n, k)
    st.run(lab)
    st.advance_ref(lab)
    st.check(f"d={d} k={k}", full=False)
    rng = np.random.RandomState(13)
    C32 = (rng.standard_normal((k, d)) * 3).astype(np.float32)
    C = torch.from_numpy(C32).to(cuda)
    ref, mag = R.cluster_parts_ref(st.S, st.N, st.Q, C32, st.ws.xexp, st.qexp)
    part = torch.full((512 + k,), 7.0, dtype=torch.float64, device=cuda)
    K.cluster_inertia_native(st.sums, st.counts, st.qsum, C, k, d, st.ws, st.qexp, part[512:])
    got = part[512:].cpu().numpy()
    # per lane an fma chain of ceil(d / 64) terms, a 6-level tree, then three
    # scalings and two additions (the constant 10 covers tree and closing)
    tol = gamma(math.ceil(d / 64) + 10, U64) * mag
    err = np.abs(got - ref)
    print(f"cluster parts d={d} k={k}: max err / bound = "
          f"{float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (err <= tol).all()
    empty = st.N == 0
    assert empty.sum() == (2 if k > 2 else 0)
    assert (got[empty] == 0.0).all()
    packed_ref = np.concatenate([(st.S.astype(np.float64) * 2.0 ** st.ws.xexp).ravel(),
                                 st.N.astype(np.float64)])
    for cn_ in CORR_N:
        c32, csum, cabs = _corr(cn_)
        corr = torch.from_numpy(c32).to(cuda)
        assert corr.data_ptr() % 16 == 0
        part1 = torch.full((512 + k,), 7.0, dtype=torch.float64, device=cuda)
        inertia1 = torch.full((1,), 7.0, dtype=torch.float64, device=cuda)
        packed1 = torch.full((k * d + k + 1,), 7.0, dtype=torch.float64, device=cuda)
        K.mstep_stats_native(st.sums, st.counts, st.qsum, C, k, d, st.ws, st.qexp, corr, cn_,
                             part1, inertia1, packed1)
        # the documented association: the three-launch form, bit for bit
        part2 = torch.full((512 + k,), 7.0, dtype=torch.float64, device=cuda)
        inertia2 = torch.full((1,), 7.0, dtype=torch.float64, device=cuda)
        packed2 = torch.full((k * d + k + 1,), 7.0, dtype=torch.float64, device=cuda)
        K.cluster_inertia_native(st.sums, st.counts, st.qsum, C, k, d, st.ws, st.qexp,
                                 part2[512:512 + k])
        K.sum_f32_native(corr, cn_, part2, inertia2, extra=k)
        K.pack_stats_native(st.sums, st.counts, inertia2, packed2, k, d, st.ws, weighted=False)
        torch.cuda.synchronize()
        tail = packed1[-1:].cpu()
        assert torch.equal(inertia1.cpu().view(torch.int64), tail.view(torch.int64))
        assert torch.equal(inertia1, inertia2) and torch.equal(packed1, packed2), cn_
        _assert_equal(packed1[:-1], packed_ref, f"packed d={d} k={k} n={cn_}")
        # the longest addition chain through mstep_parts_kernel and
        # pack_sum_kernel: ceil(n / 524288) float4 groups per thread of a
        # block, the closing of the 4 accumulators and the 8-level block tree
        # (12), then ceil((512 + k) / 256) partials per thread and another
        # 8-level tree in pack_sum_kernel; 24 covers both closings with slack
        idx = math.ceil(cn_ / 524288) + math.ceil((512 + k) / 256) + 24
        total = math.fsum([csum] + ref.tolist())
        tol_t = gamma(idx, U64) * (cabs + math.fsum(mag.tolist()))
        e = abs(inertia1.item() - total)
        print(f"inertia d={d} k={k} n={cn_}: err / bound = {e / tol_t:.3f}")
        assert e <= tol_t, (e, tol_t)


# ---------------------------------------------------------------- (f) finalize
def _kernel_d_pad(d):
    """The operand width ``sq_centroid_finalize`` pads d to."""
    for f in (16, 32, 64, 128, 256):
        if d <= f:
            return f
    return (d + 15) // 16 * 16


def _packed(k, d, kind, seed):
    """A packed bucket: sums = integers * 2^-20, counts with zeros (rows 0
    mod 5 and the last), integers (``int``) or non-integers (``weighted``)."""
    rng = np.random.RandomState(seed)
    sums = rng.randint(-2 ** 24, 2 ** 24, (k, d)).astype(np.float64) * 2.0 ** -20
    cnt = rng.randint(1, 6, k).astype(np.float64)
    if kind == "weighted":
        cnt = cnt * 0.125 + rng.randint(1, 8, k) / 64.0 + 1.0 / 3.0
    if k > 1:
        cnt[::5] = 0.0
        cnt[k - 1] = 0.0
    return np.concatenate([sums.ravel(), cnt, [2.5]])


FINALIZE_SHAPES = [(1, 16), (63, 20), (64, 48), (65, 256), (70, 260)]


def _finalize(cuda, packed, C_old, k, d, b, key, policy, op=None, **kw):
    K = _K()
    kp, dp = K.pad_clusters(k), _kernel_d_pad(d)
    C_new = torch.full((k, d), 7.0, dtype=torch.float32, device=cuda)
    cn = torch.full((kp,), 7.0, dtype=torch.float32, device=cuda)
    shift = torch.full((1,), 7.0, dtype=torch.float64, device=cuda)
    shift_part = torch.full((k,), 7.0, dtype=torch.float64, device=cuda)
    Cb = Cf = None
    if op == "bf16":
        Cb = torch.full(K.operand_shape(kp, dp), 7.0, dtype=torch.bfloat16, device=cuda)
    elif op == "f16":
        Cf = torch.full(K.operand_f16_shape(kp, dp), 7.0, dtype=torch.float16, device=cuda)
    K.centroid_finalize_native(packed, C_old, C_new, Cb, cn, shift, k, d, b, key,
                               empty_policy=policy, shift_part=shift_part, C_f16=Cf, k_pad=kp, **kw)
    torch.cuda.synchronize()
    return C_new, cn, shift, shift_part, Cb, Cf


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("k,d", FINALIZE_SHAPES)
def test_finalize_without_noise(cuda, k, d, policy):
    K = _K()
    from sq_learn_amd.runtime.rng import RngKey
    key = RngKey(1, "trunc_normal", 2)
    kp, dp = K.pad_clusters(k), _kernel_d_pad(d)
    rng = np.random.RandomState(17)
    old = (rng.standard_normal((k, d)) * 2).astype(np.float32)
    C_old = torch.from_numpy(old).to(cuda)
    for kind in ("int", "weighted"):
        pk = _packed(k, d, kind, seed=k + d)
        packed = torch.from_numpy(pk).to(cuda)
        ref, shift_ref = R.finalize_ref(pk, old, k, d, policy)
        C_new, cn, shift, shift_part, Cb, _ = _finalize(cuda, packed, C_old, k, d, 0.0, key,
                                                        policy, op="bf16")
        got = C_new.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, "C_new")
        if k > 1:
            assert np.array_equal(got[0], old[0] if policy == 0 else np.zeros(d, np.float32))
        # shift: per thread ceil(d / 256) squared differences, a 6-level wave
        # tree and the 4 wave partials
        sp = shift_part.cpu().numpy()
        assert (np.abs(sp - shift_ref) <= gamma(math.ceil(d / 256) + 10, U64) * shift_ref).all()
        tot = math.fsum(shift_ref.tolist())
        assert abs(shift.item() - tot) <= gamma(math.ceil(k / 256) + 10, U64) * tot
        # ||bf16(c)||^2 in fp32, the same chain
        h = torch.from_numpy(ref).to(torch.bfloat16).double().numpy()
        nn = np.array([math.fsum(r) for r in h * h])
        cng = cn.cpu().numpy()
        assert (np.abs(cng[:k].astype(np.float64) - nn)
                <= gamma(math.ceil(d / 256) + 10, U32) * nn).all()
        assert (cng[k:] > 1e37).all()
        # the bf16 operand: body as the host twin builds it, the norm chunk
        # [hi, mid, lo] of cn, zeros elsewhere (pad rows: only the norm slot)
        ref_op, _ = K.centers_to_bf16(C_new, kp, dp)
        nch = dp // 8
        assert torch.equal(Cb[:, :nch].view(torch.int16), ref_op[:, :nch].view(torch.int16))
        norm = Cb[:, nch].reshape(kp, 8).float().cpu().numpy().astype(np.float64)
        pieces = norm[:k, :3].sum(1)
        assert (np.abs(pieces - cng[:k].astype(np.float64)) <= _ulp32(cng[:k])).all()
        assert (norm[:, 3:] == 0).all() and (Cb[:, nch + 1].float() == 0).all()
        assert (norm[k:, 0] > 1e37).all() and (norm[k:, 1:3] == 0).all()
        rows = Cb[:, :nch].permute(0, 2, 1, 3).reshape(kp, dp)
        assert (rows[k:].float() == 0).all()
        # the fp16 hi / lo operand and cn = fp32(sum (alpha v)^2)
        alpha = K.choose_alpha(float((ref.astype(np.float64) ** 2).sum(1).max()))
        C_new2, cn2, shift2, _, _, Cf = _finalize(cuda, packed, C_old, k, d, 0.0, key, policy,
                                                  op="f16", alpha=alpha)
        assert torch.equal(C_new2, C_new) and torch.equal(shift2, shift)
        av = ref.astype(np.float64) * alpha
        nn64 = np.array([math.fsum(r) for r in av * av])
        cn2g = cn2.cpu().numpy()
        assert (np.abs(cn2g[:k].astype(np.float64) - nn64) <= _ulp32(nn64)).all()
        assert (cn2g[k:] > 1e37).all()
        # the twin with the norm split taken from the device's cn (the twin's
        # own fp64 sum may round to the neighbouring fp32)
        twin = K.centers_to_f16(C_new.cpu(), kp, dp, alpha)
        a, bb, c = K._split3_f16(cn2[:k].cpu())
        tw = twin.clone()
        view = tw.permute(0, 2, 1, 3)            # [tile][centroid][chunk][8]
        for j in range(k):
            view[j // 64, j % 64, nch, 0] = a[j]
            view[j // 64, j % 64, nch, 1] = bb[j]
            view[j // 64, j % 64, nch, 2] = c[j]
        # (equal as fp16 values, which for every non-zero is equal bits: the
        # kernel's fused multiply-convert gives the zeros of an empty cluster
        # under policy 1 a positive sign where the twin's -2 alpha * 0 is -0)
        assert not torch.isnan(tw.float()).any()
        assert bool((Cf.cpu() == tw).all()), (kind, "f16 operand")


@pytest.mark.parametrize("k,d", FINALIZE_SHAPES)
def test_finalize_noise_and_scalars(cuda, k, d):
    """b = 0.05: the means plus the same truncated-normal draws as
    ``trunc_normal_add_`` (the same device function and counter j d + c, the
    same fp32 add, another launcher); the iteration scalars of the launch."""
    K = _K()
    from sq_learn_amd.ops.random import trunc_normal_add_
    from sq_learn_amd.runtime.rng import RngKey
    key = RngKey(1, "trunc_normal", 2)
    b = 0.05
    rng = np.random.RandomState(19)
    old = (rng.standard_normal((k, d)) * 2).astype(np.float32)
    C_old = torch.from_numpy(old).to(cuda)
    pk = _packed(k, d, "int", seed=k + d)
    packed = torch.from_numpy(pk).to(cuda)
    means, _, _, _, _, _ = _finalize(cuda, packed, C_old, k, d, 0.0, key, 0, op="bf16")
    buf = K.EStepBuffers(8, cuda)
    buf.counts[0] = 5
    buf.ovf_clean = False
    kept = torch.tensor([123], dtype=torch.int32, device=cuda)
    scalars = torch.full((4,), 7.0, dtype=torch.float64, device=cuda)
    cmax2 = torch.full((1,), 7.0, dtype=torch.float32, device=cuda)
    C_new, cn, shift, _, _, _ = _finalize(cuda, packed, C_old, k, d, b, key, 0, op="bf16",
                                          scalars=scalars, buf=buf, cmax2=cmax2, kept=kept)
    expect = means.clone()
    trunc_normal_add_(expect.view(-1), b, key, offset=0)
    torch.cuda.synchronize()
    assert torch.equal(C_new.view(torch.int32), expect.view(torch.int32))
    dev = (C_new.double() - means.double()).abs().max().item()
    room = float(np.spacing(np.float32(means.abs().max().item() + b)))
    assert 0.5 * b < dev <= b + room or k * d < 64 and dev <= b + room
    sc = scalars.cpu()
    assert sc[0].item() == pk[-1] == 2.5
    assert torch.equal(sc[1:2].view(torch.int64), shift.cpu().view(torch.int64))
    assert sc[2].item() == 5.0 and sc[3].item() == 123.0
    assert int(buf.ovf_count.item()) == 0 and buf.ovf_clean
    assert cmax2.item() == cn[:k].max().item()


# -------------------------------------------------- (g) bf16 half-wave variant
HALF_SHAPES = ((8193, 256), (8193, 264), (20001, 512))


def _half_child():
    """Runs in a fresh process with SQ_SEG_HALF=1 (read once per process):
    the reference check of the segmented reduce for bf16."""
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    assert os.environ.get("SQ_SEG_HALF") == "1"
    cuda = torch.device("cuda", 0)
    for n, d in HALF_SHAPES:
        for wk in ("none", "rand"):
            _check_reduce(cuda, "bf16", n, d, K0, "random", "normal", wk)
            _check_reduce(cuda, "bf16", n, d, K0, "with_invalid", "normal", wk)
    print("half-wave child ok")


def test_reduce_bf16_half_wave_variant(cuda):
    """segment_sum_rows_half_kernel (SQ_SEG_HALF=1) in one fresh child."""
    env = dict(os.environ)
    env["SQ_SEG_HALF"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--half-child"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "half-wave child ok" in r.stdout


if __name__ == "__main__":
    if sys.argv[1:] == ["--half-child"]:
        _half_child()
    else:
        sys.exit("usage: test_mstep_kernels_gpu.py --half-child")
