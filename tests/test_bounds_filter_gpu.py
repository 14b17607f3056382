"""bounds_filter_kernel (csrc/estep_f32.hip) called directly on crafted inputs
against a torch fp64 replica of its documented rule: the three row lists (as
sets) and their counts, the rewritten bounds of the rows that hold, the
untouched bounds of the others, the zeroed corrections.  Shapes: one small odd n and one that makes the launcher pick its
large-shard instantiation; k below and above the LDS-table limit (kBfLdsK =
2048), with and without fast centroids; gap records on and off.

Rows whose decision is within rounding of the threshold are left out (hipcc
contracts w*w - u*u into an fma): |w^2 - u^2 - thr| <= 1e-12 (w^2 + u^2), for
the final test and for the cheap Elkan form that chooses which w is stored.
Their share is asserted to stay below 0.1 %."""
import functools
import types

import pytest
import torch

from sq_learn_amd.ops import kmeans as K

pytestmark = pytest.mark.gpu

DELTA = 0.5
IT_NOW, IT_LO, RING = 12, 5, 8


@functools.lru_cache(maxsize=None)
def _inputs(n, k, nf):
    """Crafted inputs and the replica's per-row results (read-only: the tests
    clone what the kernel writes)."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1000 * k + nf + n % 977)
    U = lambda *s: torch.rand(*s, generator=g, device=dev, dtype=torch.float64)
    labels = torch.randint(0, k, (n,), generator=g, device=dev, dtype=torch.int32)
    labels[U(n) < 0.02] = -1
    # shifts: most small, a few large
    shift = 0.02 * U(k)
    big = torch.randperm(k, generator=g, device=dev)[:max(k // 16, 2)]
    shift[big] = 0.3 + 0.7 * U(big.numel())
    order = torch.argsort(shift, descending=True)
    fidx = order[:nf].to(torch.int32) if nf else torch.zeros(1, dtype=torch.int32, device=dev)
    rest = shift.clone()
    if nf:
        rest[order[:nf]] = 0.0
    smax = rest.max().reshape(1)
    # Elkan distances to the fast centroids (+inf on j = fidx[f]) and their minimum
    cc = None
    if nf:
        # mostly far (the cheap form through the minimum decides for small
        # ub, the per-centroid form for large ub), a few near ones that cap w
        ccm = torch.where(U(k, nf) < 0.03, 0.5 + 3.5 * U(k, nf), 5.0 + 4.0 * U(k, nf)).float()
        ccm[fidx.long(), torch.arange(nf, device=dev)] = float("inf")
        cc = torch.cat([ccm.reshape(-1), ccm.min(1).values])
    # bounds around the threshold lb^2 - ub^2 = delta: roughly half the rows hold
    ub = (1.0 + 2.0 * U(n)).float()
    lb = (torch.sqrt(ub.double() ** 2 + DELTA) + 0.25 * (U(n) - 0.5) + float(smax)).float()
    lb[U(n) < 0.01] = 0.0
    # multi flag: 0, 1, or 2 + base with bases inside and outside [IT_LO, IT_NOW - 1]
    r = U(n)
    base = torch.randint(IT_LO - 3, IT_NOW + 3, (n,), generator=g, device=dev, dtype=torch.int32)
    mflag = torch.where(r < 0.5, torch.zeros_like(base),
                        torch.where(r < 0.6, torch.ones_like(base), base + 2))

    # ---- fp64 replica of the rule
    thr = DELTA * (1.0 + 1e-9) + 1e-30
    l = labels.long().clamp(min=0)
    valid = labels >= 0
    u = ub.double() + shift[l]
    lb0 = lb.double()
    w = lb0 - smax
    near = torch.zeros(n, dtype=torch.bool, device=dev)
    n_cheap = n_tight = 0
    if nf:
        sf = shift[fidx.long()]
        sF = sf.max()
        cmin = cc[k * nf:].double()[l]
        wc = torch.minimum(w, torch.maximum(cmin - u, lb0 - sF))
        try_cheap = valid & (w > 0)
        dc = wc * wc - u * u
        cheap = try_cheap & (wc > 0) & (dc > thr)
        near |= try_cheap & (wc > 0) & ((dc - thr).abs() <= 1e-12 * (wc * wc + u * u))
        ccl = cc[:k * nf].reshape(k, nf).double()[l]
        tight = torch.minimum(w, torch.maximum(ccl - u[:, None], lb0[:, None] - sf[None, :])
                              .min(1).values)
        w = torch.where(cheap, wc, torch.where(try_cheap, tight, w))
        n_cheap = int(cheap.sum().item())
        n_tight = int((try_cheap & ~cheap & (tight > 0) & (tight * tight - u * u > thr)).sum().item())
    dd = w * w - u * u
    holds = valid & (w > 0) & (dd > thr)
    near |= valid & (w > 0) & ((dd - thr).abs() <= 1e-12 * (w * w + u * u))
    ub_new = u.float() * torch.tensor(1.0 + 2.0 ** -22, dtype=torch.float32, device=dev)
    lb_new = w.float() * torch.tensor(1.0 - 2.0 ** -22, dtype=torch.float32, device=dev)
    return types.SimpleNamespace(labels=labels, shift=shift, smax=smax, fidx=fidx, cc=cc, ub=ub,
                                 lb=lb, mflag=mflag, holds=holds, near=near, ub_new=ub_new,
                                 lb_new=lb_new, n_cheap=n_cheap, n_tight=n_tight)


def _as_set(rows, near):
    rows = rows[~near[rows]]
    s = torch.sort(rows).values
    assert torch.unique(s).numel() == s.numel(), "a row is listed twice"
    return s


@pytest.mark.parametrize("records", [True, False], ids=["records", "norecords"])
@pytest.mark.parametrize("k,nf", [(40, 0), (1024, 16), (2100, 16)])
@pytest.mark.parametrize("n", [10257, 7000003])
def test_bounds_filter_against_fp64_replica(n, k, nf, records):
    dev = torch.device("cuda:0")
    x = _inputs(n, k, nf)
    ub, lb = x.ub.clone(), x.lb.clone()
    buf = types.SimpleNamespace(
        mflag=x.mflag.clone(), multi_rows=torch.full((n,), -1, dtype=torch.int64, device=dev),
        counts=torch.zeros(12, dtype=torch.int32, device=dev),
        corr=torch.full((n,), 7.0, dtype=torch.float32, device=dev))
    rlist = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rows_b = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rec = None
    if records:
        rec = K.multi_records(torch.zeros((1, 8), dtype=torch.float32, device=dev), buf.mflag,
                              IT_NOW, IT_LO, torch.zeros((RING, 1, 128), dtype=torch.float16,
                                                         device=dev),
                              torch.zeros((RING, 1, 8), dtype=torch.float32, device=dev), rows_b,
                              buf.counts[5:6], buf.counts[4:5])
    K.bounds_filter_native(x.labels, ub, lb, x.shift, x.smax, DELTA, rlist, buf.counts[3:4],
                           buf, cc=x.cc, nf=nf, fidx=x.fidx if nf else None, records=rec)
    torch.cuda.synchronize()
    near, holds = x.near, x.holds
    n_near = int(near.sum().item())
    print(f"n={n} k={k} nf={nf}: {int(holds.sum().item())} rows hold, {n_near} left out")
    assert n_near <= 1e-3 * n
    if nf:   # both forms of the fast-centroid bound decide rows that hold
        print(f"  hold by the cheap form {x.n_cheap}, by the per-centroid form {x.n_tight}")
        assert x.n_cheap > 0 and x.n_tight > 0
    c = buf.counts.tolist()
    idx = torch.arange(n, device=dev)
    cur = (x.mflag >= IT_LO + 2) & (x.mflag <= IT_NOW + 1) if records \
        else torch.zeros(n, dtype=torch.bool, device=dev)
    exp_a = idx[~holds]
    exp_m = idx[holds & (x.mflag != 0) & ~cur]
    exp_b = idx[holds & cur]
    # the three lists as sets, and their counts (exact when no row is left out)
    for name, got, cnt, exp in (("rlist", rlist, c[3], exp_a), ("multi", buf.multi_rows, c[2], exp_m),
                                ("list B", rows_b, c[5], exp_b)):
        assert 0 <= cnt <= n, name
        assert abs(cnt - exp.numel()) <= n_near, (name, cnt, exp.numel())
        assert torch.equal(_as_set(got[:cnt], near), _as_set(exp, near)), name
        assert bool((got[cnt:] == -1).all()), name + ": written past the count"
    assert c[7] == c[2]          # the multi list's head: this pass's rows
    if records:
        assert exp_b.numel() > 0 and exp_m.numel() > 0
    else:
        assert c[5] == 0
    # bounds: rewritten exactly where they hold, untouched elsewhere
    ok = ~near
    h, nh = ok & holds, ok & ~holds
    assert torch.equal(ub[h].view(torch.int32), x.ub_new[h].view(torch.int32))
    assert torch.equal(lb[h].view(torch.int32), x.lb_new[h].view(torch.int32))
    assert torch.equal(ub[nh].view(torch.int32), x.ub[nh].view(torch.int32))
    assert torch.equal(lb[nh].view(torch.int32), x.lb[nh].view(torch.int32))
    assert int(torch.count_nonzero(buf.corr).item()) == 0
    assert torch.equal(buf.mflag, x.mflag)
