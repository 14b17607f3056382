"""The gap screen alone (csrc/estep_f32.hip gap_screen_kernel through
``sq_gap_screen``) on crafted records: the x.S sums of every listed (row,
candidate) against fp64 dots of the same fp16 values, the addressing above
2^32 bytes, the decisions on gaps far from the threshold, and the staging
flush inside a wave's block loop.

A pass of the kernel takes list rows p and 32 + p of a block of 64; with a ring
of 3 and random slots the two halves of a pass usually read different shift
operands, and c_r drawn from {2, 3, 4} mixes the pass widths.  The dots'
tolerance is the kernel's own accumulation term, gam sum_f |x~_f S~_f| inv with
gam = (DX + 16) 2^-24."""
import functools

import numpy as np
import pytest
import torch

from sq_learn_amd.ops import kmeans as K

pytestmark = pytest.mark.gpu

N, KC, RING, IT_NOW, DELTA, ALPHA = 5000, 40, 3, 7, 8.0, 2.0
RESOLVE, FORWARD, MOVE = 0, 1, 2


def _craft(seed, m, dx, kinds):
    """m crafted rows (compact arrays, fp64 reference included).  kinds[i]:
    RESOLVE - every other candidate delta + 5 (+ up to 1) above the argmin;
    FORWARD - one candidate at delta / 2; MOVE - one candidate delta + 7 BELOW
    the argmin.  Shifts are scaled so a gap moves by less than 0.5."""
    rs = np.random.RandomState(seed)
    xh = (rs.randn(m, dx) * ALPHA).astype(np.float16)
    # shift operand: S~ = rn(beta S) near 1, beta a power of two per (slot, j)
    beta = 2.0 ** rs.choice([8, 10, 12], size=(RING, KC))
    s_true = rs.randn(RING, KC, dx) * 2.0e-4
    dsh = (s_true * beta[:, :, None]).astype(np.float16)
    dq = np.zeros((RING, KC, 8), np.float32)
    dq[:, :, 0] = rs.uniform(-0.05, 0.05, (RING, KC))                 # q_j
    dq[:, :, 1] = 1e-6                                                # its error bound
    sn = np.sqrt((dsh.astype(np.float64) ** 2).sum(-1)) / beta
    dq[:, :, 2] = (sn * (1 + 1e-6)).astype(np.float32)                # |S_j| (up)
    dq[:, :, 3] = 1e-6                                                # e_j (up)
    dq[:, :, 4] = (1.0 / (ALPHA * beta)).astype(np.float32)           # exact: powers of two
    c_r = rs.randint(2, 5, size=m)
    slot = (rs.randint(0, 1 << 16, size=m) % c_r).astype(np.int64)
    jc = np.stack([rs.permutation(KC)[:4] for _ in range(m)]).astype(np.int64)
    jc[np.arange(4)[None, :] >= c_r[:, None]] = 0
    jc = np.where(np.arange(4)[None, :] >= c_r[:, None], jc[:, :1], jc)   # past c_r: candidate 0
    base = IT_NOW - rs.randint(0, RING, size=m)        # age 0 (young) .. RING - 1
    rslot = base % RING
    # fp64 reference of the kernel's sums, and the tolerance's magnitude term
    sh = dsh[rslot[:, None], jc].astype(np.float64)                       # [m, 4, dx]
    prod = xh.astype(np.float64)[:, None, :] * sh
    inv = dq[rslot[:, None], jc, 4].astype(np.float64)
    y = prod.sum(-1) * inv
    yabs = np.abs(prod).sum(-1) * inv
    q = dq[rslot[:, None], jc, 0].astype(np.float64)
    ar = np.arange(m)
    move = 2.0 * (y[ar, slot][:, None] - y) + q - q[ar, slot][:, None]
    inr = np.arange(4)[None, :] < c_r[:, None]
    assert np.abs(move[inr]).max() < 0.5
    gold = DELTA + 5.0 + rs.uniform(0, 1, (m, 4))
    other = (slot + 1 + rs.randint(0, 1 << 16, size=m) % (c_r - 1)) % c_r   # a slot != argmin
    gold[ar[kinds == FORWARD], other[kinds == FORWARD]] = 0.5 * DELTA
    gold[ar[kinds == MOVE], other[kinds == MOVE]] = -(DELTA + 7.0)
    gold[ar, slot] = 0.0
    gold[~inr] = 0.0
    rec = np.zeros((m, 8), np.float32)
    rec[:, 0] = 50.0 + rs.uniform(0, 1, m)      # da
    rec[:, 1] = 0.01                            # err
    rec[:, 2:6] = gold
    ids = rec.view(np.uint32)
    ids[:, 6] = jc[:, 0] | slot << 14 | jc[:, 1] << 16 | (c_r - 1) << 30
    ids[:, 7] = jc[:, 2] | jc[:, 3] << 16
    gold = rec[:, 2:6].astype(np.float64)
    # the decision in fp64; err as the kernel bounds it (fp64, a shade below)
    xn = ((xh.astype(np.float64) / ALPHA) ** 2).sum(-1)
    nx = np.sqrt(xn) * (1 + 2.0 ** -16)
    ex = 2.0 ** -11 * nx + np.sqrt(dx) * 2.0 ** -25 / ALPHA
    sz = dq[rslot[:, None], jc, 2].astype(np.float64)
    gam = (dx + 16) * 2.0 ** -24
    E = ex[:, None] * sz + (nx + ex)[:, None] * (1e-6 + gam * (sz + 1e-6)) + 1e-6
    Emax = np.where(inr, E, 0).max(-1)
    err = 0.01 + 2 * (E[ar, slot] + Emax) + 2.0 ** -22 * (60 + 4 * np.abs(y).max(-1) + 0.1)
    assert err.max() < 0.1
    gn = np.where(inr, gold + move, np.inf)
    gn[ar, slot] = 0.0
    mnew = gn.argmin(-1)
    gm = gn[ar, mnew]
    rest = inr & (np.arange(4)[None, :] != mnew[:, None])
    margin = np.where(rest, (gn - gm[:, None]) - (DELTA + 2 * err[:, None]), np.inf)
    assert np.abs(margin).min() >= 1.0, "a crafted row is within 1.0 of the threshold"
    done = (margin > 0).all(-1)
    assert (done == (kinds != FORWARD)).all() and ((mnew != slot) == (kinds == MOVE)).all()
    return dict(xh=xh, dsh=dsh, dq=dq, rec=rec, base=base, jc=jc, c_r=c_r, slot=slot, y=y,
                yabs=yabs, xn=xn.astype(np.float32), done=done, mnew=mnew, dx=dx, gam=gam,
                labels=jc[ar, slot].astype(np.int32))


@functools.lru_cache(maxsize=None)
def _mixed(dx):
    kinds = np.array([RESOLVE, RESOLVE, FORWARD, MOVE])[np.arange(N) % 4]
    return _craft(100 + dx, N, dx, kinds)


@functools.lru_cache(maxsize=None)
def _all_forward():
    return _craft(7, N, 128, np.full(N, FORWARD))


def _launch(cr, rows, listed, n=None, Xh=None, grid_blocks=0):
    """Run the screen on list B = rows[listed] (rows: the global row of each
    crafted row).  Returns the device state after the launch."""
    dev = torch.device("cuda:0")
    n = N if n is None else n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows_t = t(rows.astype(np.int64))
    if Xh is None:
        Xh = torch.zeros((n, cr["dx"]), dtype=torch.float16, device=dev)
    Xh[rows_t] = t(cr["xh"])
    xn = torch.zeros(n, dtype=torch.float32, device=dev)
    xn[rows_t] = t(cr["xn"])
    rec = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rec[rows_t] = t(cr["rec"])
    mflag = torch.zeros(n, dtype=torch.int32, device=dev)
    mflag[rows_t] = t((cr["base"] + 2).astype(np.int32))
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    labels[rows_t] = t(cr["labels"])
    before = dict(rec=rec.clone(), mflag=mflag.clone(), labels=labels.clone())
    dsh, dq = t(cr["dsh"]), t(cr["dq"])
    rows_b = torch.zeros(n, dtype=torch.int64, device=dev)
    rows_b[:len(listed)] = rows_t[t(listed.astype(np.int64))]
    cnt = lambda v=0: torch.full((1,), v, dtype=torch.int32, device=dev)
    count_b, multi_count, n_done, count_mv = cnt(len(listed)), cnt(), cnt(), cnt()
    multi_rows = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rows_mv = torch.full((n,), -1, dtype=torch.int64, device=dev)
    ydbg = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
    records = K.multi_records(rec=rec, mflag=mflag, it_now=IT_NOW, it_lo=IT_NOW, dsh=dsh, dq=dq,
                              rows_b=rows_b, count_b=count_b, n_done=n_done, rows_moved=rows_mv,
                              count_moved=count_mv)
    K.gap_screen_native(Xh, xn, labels, multi_rows, multi_count, records, ALPHA, DELTA,
                        grid_blocks=grid_blocks, ydbg=ydbg)
    torch.cuda.synchronize()
    return dict(rec=rec, mflag=mflag, labels=labels, before=before, ydbg=ydbg.cpu().numpy(),
                multi=multi_rows[:int(multi_count.item())].cpu().numpy(),
                moved=rows_mv[:int(count_mv.item())].cpu().numpy(), n_done=int(n_done.item()))


def _check_dots(cr, listed, ydbg):
    """Every listed (row, candidate) with c < c_r, none excluded."""
    L = len(listed)
    inr = np.arange(4)[None, :] < cr["c_r"][listed][:, None]
    got, want = ydbg[:L].astype(np.float64), cr["y"][listed]
    tol = cr["gam"] * cr["yabs"][listed]
    assert np.isfinite(got[inr]).all(), "a listed (row, candidate) was not written"
    excess = np.abs(got - want)[inr] / tol[inr]
    print(f"dx {cr['dx']} list {L}: {int(inr.sum())} dots, max |error| / tolerance "
          f"{excess.max():.4f}")
    assert excess.max() <= 1.0
    assert np.isnan(ydbg[:L][~inr]).all() and np.isnan(ydbg[L:]).all()


@pytest.mark.parametrize("dx", [128, 256])
@pytest.mark.parametrize("length", [1, 63, 64, 65, 453])
def test_dots_match_fp64(dx, length):
    cr = _mixed(dx)
    listed = np.random.RandomState(length).permutation(N)[:length]
    out = _launch(cr, np.arange(N), listed)
    _check_dots(cr, listed, out["ydbg"])


def test_rows_above_4gib():
    """Listed rows above byte offset 2^32 of a zero Xh: a row offset cut to 32
    bits would read zeros."""
    n, dx, m = 8_400_100, 256, 453
    cr = _mixed(dx)
    sel = np.arange(m)
    sub = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (N,) else v)
           for k, v in cr.items()}
    first = (1 << 32) // (2 * dx) + 1
    rows = first + np.random.RandomState(3).permutation(n - first)[:m]
    assert (rows * 2 * dx > 1 << 32).all()
    Xh = torch.zeros((n, dx), dtype=torch.float16, device="cuda:0")
    out = _launch(sub, rows, sel, n=n, Xh=Xh)
    assert np.abs(sub["y"]).min() > 0
    _check_dots(sub, sel, out["ydbg"])


@pytest.mark.parametrize("dx", [128, 256])
def test_decisions_far_from_threshold(dx):
    cr = _mixed(dx)
    L = 4001
    listed = np.random.RandomState(11).permutation(N)[:L]
    out = _launch(cr, np.arange(N), listed)
    done, mnew, slot = cr["done"][listed], cr["mnew"][listed], cr["slot"][listed]
    moved = done & (mnew != slot)
    # lists as sets, counts exact
    assert out["n_done"] == int(done.sum())
    assert len(out["multi"]) == int((~done).sum())
    assert set(out["multi"].tolist()) == set(listed[~done].tolist())
    assert len(out["moved"]) == int((~done | moved).sum())
    assert set(out["moved"].tolist()) == set(listed[~done | moved].tolist())
    # labels: only a new argmin writes one
    want_lab = cr["labels"].copy()
    want_lab[listed[moved]] = cr["jc"][listed[moved], mnew[moved]]
    assert np.array_equal(out["labels"].cpu().numpy(), want_lab)
    # records: rebased on a new argmin or at age >= max(1, ring / 2) = 1,
    # untouched for young resolved rows, forwarded rows and unlisted rows
    age = IT_NOW - cr["base"][listed]
    reb = done & (moved | (age >= 1))
    assert reb.any() and (done & ~reb).any()
    want_flag = (cr["base"] + 2).astype(np.int32)
    want_flag[listed[reb]] = IT_NOW + 2
    assert np.array_equal(out["mflag"].cpu().numpy(), want_flag)
    rec = out["rec"].cpu().numpy()
    keep = np.ones(N, bool)
    keep[listed[reb]] = False
    assert np.array_equal(rec.view(np.uint32)[keep], cr["rec"].view(np.uint32)[keep])
    ids, ids0 = rec.view(np.uint32)[listed[reb]], cr["rec"].view(np.uint32)[listed[reb]]
    want6 = (ids0[:, 6] & ~np.uint32(3 << 14)) | (mnew[reb].astype(np.uint32) << 14)
    assert np.array_equal(ids[:, 6], want6) and np.array_equal(ids[:, 7], ids0[:, 7])
    # the rebased gaps: the new argmin's slot is 0, the others above delta
    gr = rec[listed[reb], 2:6]
    assert (gr[np.arange(len(gr)), mnew[reb]] == 0).all()
    _check_dots(cr, listed, out["ydbg"])


def test_stage_flush_inside_the_block_loop():
    """One workgroup, 4,096 forwarded rows: each wave takes 16 blocks of 64 and
    flushes its 256-entry stages inside the loop."""
    cr = _all_forward()
    listed = np.random.RandomState(5).permutation(N)[:4096]
    out = _launch(cr, np.arange(N), listed, grid_blocks=1)
    assert out["n_done"] == 0
    for name in ("multi", "moved"):
        assert len(out[name]) == 4096
        assert set(out[name].tolist()) == set(listed.tolist())
    for name in ("rec", "mflag", "labels"):
        assert torch.equal(out[name], out["before"][name])
