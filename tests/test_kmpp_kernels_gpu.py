"""The k-means++ seeding kernels of csrc/kmpp.hip against the exact host
model of ``_kmpp_ref.py`` (run on an MI355X).

(a) End to end on lattice data (integer coordinates with d (2 L)^2 < 2^24:
    the device's fp32 distances are exact integers, see ``_kmpp_ref``): ids,
    centres and the final potential of every driver - the one-launch winner
    path with and without the screens, the general pick / trials / argmin /
    apply loop, the batched restarts with each of their pass variants - must
    EQUAL the numpy run.
(b) Per-step invariants on real-valued data: after every step the device
    state is read back and checked against fp64 direct-form distances (bound
    ``r = 3 (d + 2) 2^-24``, derived in ``_kmpp_ref.rel_tol``) and against
    the integer potentials recomputed from the device's own fp32 values
    (exact).  A clear mask bit is checked against the truth: no screen may
    drop an improving row.
(c) The certificates of the int8 bound, by direct launcher calls.

``test_kmpp_ref_cpu.py`` checks the model on its own and the preconditions of
every parameter set below.
"""
import numpy as np
import pytest
import torch

import _kmpp_ref as R

pytestmark = pytest.mark.gpu

SEED = 11

# ------------------------------------------------------------ (a) the cases
# name: (n, d, t, k, blobs, weights, duplicates)
E2E_CASES = {
    "n1": (1, 4, 1, 1, 1, None, False),
    "n255_d4_t3": (255, 4, 3, 6, 6, None, False),            # one short block
    "n255_d20_t1": (255, 20, 1, 6, 6, None, False),          # dq padding 20 -> 64
    "n777_d4_t1": (777, 4, 1, 6, 6, None, False),            # short last block
    "n777_d20_t3": (777, 20, 3, 7, 6, None, False),
    "G274": (70001, 64, 5, 8, 8, None, False),               # pick's chunk = 2; tp = 8
    "R257": (2048 * 256 + 513, 4, 3, 8, 8, None, False),     # second pass of the per-block loops
    "R513": (2048 * 512 + 77, 8, 16, 6, 6, None, False),     # rchunk = 3, 3 batches a wave, TMAX 16
    "d68": (3000, 68, 8, 7, 7, None, False),                 # dq / 64 = 2, last feature tile of 4
    "d192": (3000, 192, 8, 7, 7, None, False),               # dq / 64 = 3
    "d256": (3000, 256, 8, 7, 7, None, False),               # dq / 64 = 4
    "d260": (3000, 260, 5, 6, 6, None, False),               # dq 320: generic bound, ops 2 / 3 / 4
    "d2112": (600, 2112, 3, 6, 6, None, False),              # dq beyond the bound's LDS limit
    "w_dyadic": (3001, 20, 3, 8, 8, "dyadic", False),
    "w_real": (3001, 20, 3, 8, 8, "real", False),
    "dups": (3500, 32, 3, 8, 6, None, True),                 # zero potentials, whole zero blocks
}
# blob sets on which the pruned run must send fewer than n rows to the exact pass
SCREEN_CASES = ("G274", "R257", "R513")
DUP_ROWS = (250, 750)        # rows of "dups" that copy one far row (blocks 1 and 2 of R = 250)
RESTARTS = (1, 3, 16)
RESTART_ENVS = (None, "SQ_KMPP_FUSED", "SQ_KMPP_PAIRS", "SQ_KMPP_EXACT2")

_DATA, _REF = {}, {}


def e2e_data(name):
    """(X fp32 lattice [n, d], w fp64 [n] or None) of a case (cached)."""
    if name not in _DATA:
        n, d, t, k, blobs, wk, dups = E2E_CASES[name]
        L = R.lattice_limit(d)
        X = R.lattice_blobs(n, d, blobs, L, seed=n + d)
        if dups:
            X[DUP_ROWS[0]:DUP_ROWS[1]] = np.float32(L)       # one far corner row, 500 times
        rs = np.random.RandomState(n)
        w = None
        if wk == "dyadic":
            w = rs.randint(1, 41, n) / 8.0
        elif wk == "real":
            w = rs.uniform(0.1, 5.0, n)
        _DATA[name] = (X, w)
    return _DATA[name]


def e2e_draws(name, nr):
    """[(first id, draws [k - 1, t])] of ``nr`` consecutive runs on one
    RandomState(SEED): the reference's draw order."""
    n, d, t, k = E2E_CASES[name][:4]
    rs = np.random.RandomState(SEED)
    return [(int(rs.randint(n)), rs.random_sample((max(k - 1, 0), t))) for _ in range(nr)]


def e2e_ref(name, r=0):
    """``kmpp_ref`` of restart ``r`` of a case (computed once)."""
    if (name, r) not in _REF:
        n, d, t, k = E2E_CASES[name][:4]
        X, w = e2e_data(name)
        fid, draws = e2e_draws(name, r + 1)[r]
        _REF[(name, r)] = R.kmpp_ref(X, k, t, fid, draws, w=w)
    return _REF[(name, r)]


def e2e_refs(name, nr):
    """The first ``nr`` restarts' references, the missing ones computed side
    by side (numpy releases the GIL in its loops; 16 runs at the largest
    shape are ~10^10 flops, computed once for all four pass variants)."""
    from concurrent.futures import ThreadPoolExecutor
    todo = [r for r in range(nr) if (name, r) not in _REF]
    if len(todo) > 1 and E2E_CASES[name][0] > 50000:
        e2e_data(name)
        with ThreadPoolExecutor(min(16, len(todo))) as ex:
            list(ex.map(lambda r: e2e_ref(name, r), todo))
    return [e2e_ref(name, r) for r in range(nr)]


def _K():
    from sq_learn_amd.ops import kmeans as K
    return K


def _data(Xt):
    from sq_learn_amd.models._data import Data
    from sq_learn_amd.parallel.comm import Comm
    return Data(Xt, Xt.shape[0], 0, Comm(None), "sharded")


def _check_run(tag, ref, ids, centres, P):
    np.testing.assert_array_equal(np.asarray(ids), ref["ids"], err_msg="ids " + tag)
    np.testing.assert_array_equal(centres.cpu().numpy(), ref["centres"], err_msg="centres " + tag)
    assert float(P) == ref["P"], f"final P {tag}: {float(P)!r} != {ref['P']!r}"


def drive(Xt, k, t, first_id, draws, w=None, prune=True, mode="finish", hook=None,
          row_offset=0, n_global=None):
    """One k-means++ run on a ``KmppState`` as ``_kmeans_plusplus_native``
    drives it: ``mode`` "finish" (the one-rank loop: pick + row copy, trials,
    one finishing launch) or "apply" (the general loop: pick, trials with the
    reduced Delta, argmin, apply).  ``hook(info)`` runs after every step.
    Returns (ids numpy, centres, final P, state)."""
    K = _K()
    n, d = Xt.shape
    dev = Xt.device
    ng = n if n_global is None else int(n_global)
    dr = torch.as_tensor(np.asarray(draws).reshape(max(k - 1, 0), t), dtype=torch.float64,
                         device=dev)
    ids = torch.empty(k, dtype=torch.int64, device=dev)
    ids[0] = first_id + row_offset
    centres = torch.empty((k, d), dtype=torch.float32, device=dev)
    centres[0] = Xt[first_id]
    st = K.KmppState(Xt, k, t, w=w, prune=prune)
    mx = st.first_centre(Xt[first_id])
    P = st.set_scale(mx.item(), ng).clone()
    if hook is not None:
        hook(dict(c=0, st=st, P_after=P, centres=centres, max_pot=mx.item()))
    cands = torch.empty((t, d), dtype=torch.float32, device=dev)
    cand_ids = torch.empty(t, dtype=torch.int64, device=dev)
    vals = (dr[0] * P) if k > 1 else torch.zeros(t, dtype=torch.float64, device=dev)
    for c in range(1, k):
        vals_used, P_before = vals.clone(), P.clone()
        pos = st.pick(vals, cands, cand_ids, row_offset, ng)
        nxt = dr[c] if c < k - 1 else None
        if mode == "finish":
            st.trials(cands, centres, c, reduce=False)
            st.finish(P, nxt, vals, cands, cand_ids, centres, ids, c)
            best = st.best
        else:
            delta = st.trials(cands, centres, c)
            pots = P - delta
            best = torch.argmin(pots)
            P = pots[best].reshape(1).clone()
            st.apply(best, c)
            centres[c] = cands[best]
            ids[c] = cand_ids[best]
            if nxt is not None:
                vals = nxt * P
        if hook is not None:
            hook(dict(c=c, st=st, vals=vals_used, pos=pos, cands=cands, cand_ids=cand_ids,
                      P_before=P_before, P_after=P, best=int(best), centres=centres, ids=ids,
                      vals_next=vals if nxt is not None else None, draws=dr))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), centres, float(P), st


def _upload(cuda, name):
    X, w = e2e_data(name)
    Xt = torch.from_numpy(X).to(cuda)
    wt = None if w is None else torch.from_numpy(w).to(cuda)
    return Xt, wt


@pytest.mark.parametrize("driver", ["prune", "noprune", "general"])
@pytest.mark.parametrize("name", list(E2E_CASES))
def test_run_equals_reference(cuda, monkeypatch, name, driver):
    """ids, centres and the final P of one run equal ``kmpp_ref`` exactly."""
    from sq_learn_amd.models.cluster._init import kmeans_plusplus
    K = _K()
    n, d, t, k = E2E_CASES[name][:4]
    ref = e2e_ref(name)
    Xt, wt = _upload(cuda, name)
    if driver == "general":
        fid, draws = e2e_draws(name, 1)[0]
        ids, C, P, _ = drive(Xt, k, t, fid, draws, w=wt, prune=True, mode="apply")
        _check_run(f"{name} general", ref, ids, C, P)
        return
    seen = {}
    set_scale, finish = K.KmppState.set_scale, K.KmppState.finish

    def spy_scale(self, *a):
        seen["P"] = set_scale(self, *a)
        return seen["P"]

    def spy_finish(self, P, *a):
        seen["P"] = P
        return finish(self, P, *a)

    monkeypatch.setattr(K.KmppState, "set_scale", spy_scale)
    monkeypatch.setattr(K.KmppState, "finish", spy_finish)
    stats = []
    C, ids = kmeans_plusplus(_data(Xt), k, np.random.RandomState(SEED), n_local_trials=t,
                             sample_weight=wt, prune=driver == "prune", stats=stats)
    torch.cuda.synchronize()
    _check_run(f"{name} {driver}", ref, ids, C, seen["P"].cpu()[0])
    stats = np.asarray(stats).reshape(-1, 2)
    if driver == "noprune":
        assert (stats[:, 1] == n).all()
    elif name in SCREEN_CASES:
        # otherwise the pruned run proves nothing about the screens
        assert stats[:, 1].min() < n, stats


@pytest.mark.parametrize("env", RESTART_ENVS, ids=lambda e: e or "default")
@pytest.mark.parametrize("name", [c for c in E2E_CASES if E2E_CASES[c][5] is None
                                  and E2E_CASES[c][3] >= 2])
def test_batched_restarts_equal_reference(cuda, monkeypatch, name, env):
    """Every restart of ``kmeans_plusplus_restarts`` (1, 3 and 16 restarts;
    the fused passes, the per-restart passes, the exact pass over whole rows
    and the lane-per-row exact pass) equals its own ``kmpp_ref`` run."""
    from sq_learn_amd.models.cluster import _init as I
    K = _K()
    n, d, t, k = E2E_CASES[name][:4]
    Xt, _ = _upload(cuda, name)
    if env is not None:
        monkeypatch.setenv(env, "0")
    got = []
    run = K.KmppBatch.run

    def spy_run(self, *a, **kw):
        C, ids = run(self, *a, **kw)
        got.extend((ids[r].cpu().numpy(), self.P[r].cpu()[0]) for r in range(self.nr))
        return C, ids

    monkeypatch.setattr(K.KmppBatch, "run", spy_run)
    refs = e2e_refs(name, max(RESTARTS))
    for nr in RESTARTS:
        del got[:]
        out = I.kmeans_plusplus_restarts(_data(Xt), k, np.random.RandomState(SEED), nr,
                                         n_local_trials=t)
        torch.cuda.synchronize()
        assert out is not None and len(out) == nr == len(got)
        for r in range(nr):
            _check_run(f"{name} {env}=0 restart {r} of {nr}", refs[r], got[r][0],
                       out[r], got[r][1])


# --------------------------------------------- (b) per-step invariants
# (n, d, t, weighted): Gaussian blobs off the lattice; rows [R, 3 R) copy row
# 0, the first centre: two whole blocks of zero potential
STEP_CASES = [(5000, 64, 5, False), (3001, 20, 3, True), (2048 * 256 + 513, 8, 4, False)]
STEP_K = 8


def step_data(n, d, weighted):
    rs = np.random.RandomState(n + d)
    G = rs.uniform(-10.0, 10.0, (STEP_K, d))
    X = (G[rs.randint(STEP_K, size=n)] + rs.standard_normal((n, d))).astype(np.float32)
    Rb, _ = R.partition(n)
    X[Rb:3 * Rb] = X[0]
    w = rs.uniform(0.1, 5.0, n) if weighted else None
    return X, w


class StepChecker:
    """Host side of (b): the truth in fp64, the integers from the device's
    own fp32 values."""

    def __init__(self, X, w, t, row_offset, n_global):
        self.X, self.w, self.t = X, w, t
        self.X64 = X.astype(np.float64)
        self.n, self.d = X.shape
        self.r = R.rel_tol(self.d)
        self.row_offset, self.ng = row_offset, n_global
        self.tmin = None          # fp64 min_m |x - C_m|^2 over the chosen centres
        self.q_eff = None         # integer potentials the next pick samples from
        self.steps = 0

    def _close(self, got32, ref64, what):
        err = np.abs(got32.astype(np.float64) - ref64)
        bad = err > self.r * ref64
        assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(ref64, 1e-300)).max()))

    def __call__(self, s):
        st, c, n, t = s["st"], s["c"], self.n, self.t
        torch.cuda.synchronize()
        C = s["centres"].cpu().numpy()
        if c == 0:
            cl = st.closest[:n].cpu().numpy()
            self.tmin = R.dist2(self.X64, C[0])[0]
            self._close(cl, self.tmin, "first closest")
            mx = float((cl.astype(np.float64) * (1.0 if self.w is None else self.w)).max())
            assert s["max_pot"] == mx
            self.scale = R.scale_for(mx, self.ng)
            assert st.scale == self.scale and self.ng * mx * self.scale <= R.LIMIT
            assert (st.R, st.G) == R.partition(n)
            self.q_eff = R.q(cl, self.w, self.scale)
            bt = R.block_totals(self.q_eff, st.R, st.G)
            np.testing.assert_array_equal(st.block_tot.cpu().numpy(), bt)
            assert float(s["P_after"]) == bt.sum()
            assert (bt[1:3] == 0).all() and bt[3] > 0
            return
        prev = 1 - st.cur
        cl = st.closest[:n].cpu().numpy()                     # effective before this step
        near = st.nearest[:n].cpu().numpy()
        mask = st.mask[prev][:n].cpu().numpy().view(np.uint16).astype(np.int64)
        D = st.D[prev][:, :n].cpu().numpy()
        cl64 = cl.astype(np.float64)
        # the sampler: positions, rows and clamped ids of this step's candidates
        pos, gid = R.pick_ref(self.q_eff, s["vals"].cpu().numpy(), n, self.row_offset, self.ng)
        np.testing.assert_array_equal(s["pos"].cpu().numpy(), pos)
        cands = s["cands"].cpu().numpy()
        np.testing.assert_array_equal(cands, self.X[pos])
        np.testing.assert_array_equal(s["cand_ids"].cpu().numpy(), gid)
        # closest / nearest against the truth
        self._close(cl, self.tmin, f"closest before step {c}")
        assert near.min() >= 0 and near.max() < c
        e = self.X64 - C[near].astype(np.float64)
        self._close(cl, np.einsum("ij,ij->i", e, e), f"distance to nearest, step {c}")
        # the trial pass
        D64 = R.dist2(self.X64, cands)
        delta = np.zeros(t)
        for j in range(t):
            bit = ((mask >> j) & 1).astype(bool)
            assert (D[j][bit] < cl[bit]).all(), f"step {c} trial {j}: set bit without improvement"
            self._close(D[j][bit], D64[j][bit], f"D step {c} trial {j}")
            miss = D64[j][~bit] < cl64[~bit] * (1.0 - 2.0 * self.r)
            assert not miss.any(), (f"step {c} trial {j}: {int(miss.sum())} improving rows dropped",
                                    np.nonzero(~bit)[0][miss][:8])
            wj = None if self.w is None else self.w[bit]
            delta[j] = (R.q(cl[bit], wj, self.scale) - R.q(D[j][bit], wj, self.scale)).sum()
        assert (mask >> t == 0).all()
        np.testing.assert_array_equal(st.delta.sum(0).cpu().numpy(), delta)
        # the winner and what it leaves behind
        Pb = float(s["P_before"])
        best = int(np.argmin(Pb - delta))
        assert s["best"] == best
        eff = R.effective_closest(cl, mask, D, best)
        self.q_eff = R.q(eff, self.w, self.scale)
        bt = R.block_totals(self.q_eff, st.R, st.G)
        np.testing.assert_array_equal(st.block_tot.cpu().numpy(), bt)
        assert float(s["P_after"]) == bt.sum() == Pb - delta[best]
        if s["vals_next"] is not None:
            np.testing.assert_array_equal(s["vals_next"].cpu().numpy(),
                                          s["draws"][c].cpu().numpy() * float(s["P_after"]))
        np.testing.assert_array_equal(C[c], cands[best])
        assert int(s["ids"][c]) == gid[best]
        self.tmin = np.minimum(self.tmin, D64[best])
        self.steps += 1

    def extra_picks(self, st):
        """Sampler edges on the final state: 0, a block's inclusive prefix,
        that + 1 (lands behind the zero blocks), inside a later block, P and
        beyond P."""
        cs = np.cumsum(self.q_eff)
        Rb, P = st.R, cs[-1]
        vals = [0.0, cs[Rb - 1], cs[Rb - 1] + 1.0, cs[3 * Rb + Rb // 2] - 1.0, cs[4 * Rb - 1],
                P, P + 1.0, 2.0 * P]
        for i in range(0, len(vals), self.t):
            v = np.asarray(vals[i:i + self.t])
            m = len(v)
            cands = torch.zeros((m, self.d), dtype=torch.float32, device=st.dev)
            cid = torch.zeros(m, dtype=torch.int64, device=st.dev)
            pos = st.pick(torch.from_numpy(v).to(st.dev), cands, cid, self.row_offset, self.ng)
            rp, rid = R.pick_ref(self.q_eff, v, self.n, self.row_offset, self.ng)
            np.testing.assert_array_equal(pos.cpu().numpy(), rp, err_msg=str(v))
            np.testing.assert_array_equal(cid.cpu().numpy(), rid)
            np.testing.assert_array_equal(cands.cpu().numpy(), self.X[rp])
        p2, _ = R.pick_ref(self.q_eff, [cs[Rb - 1] + 1.0])
        assert p2[0] >= 3 * Rb                  # behind the two zero blocks


@pytest.mark.parametrize("mode", ["finish", "apply"])
@pytest.mark.parametrize("prune", [True, False], ids=["prune", "noprune"])
@pytest.mark.parametrize("n,d,t,weighted", STEP_CASES)
def test_step_invariants(cuda, n, d, t, weighted, prune, mode):
    X, w = step_data(n, d, weighted)
    Xt = torch.from_numpy(X).to(cuda)
    wt = None if w is None else torch.from_numpy(w).to(cuda)
    rs = np.random.RandomState(n)
    draws = rs.random_sample((STEP_K - 1, t))
    # a shard in the middle of a larger set whose last rows clamp
    row_offset, ng = 7, n + 3
    chk = StepChecker(X, w, t, row_offset, ng)
    _, _, _, st = drive(Xt, STEP_K, t, 0, draws, w=wt, prune=prune, mode=mode, hook=chk,
                        row_offset=row_offset, n_global=ng)
    assert chk.steps == STEP_K - 1
    chk.extra_picks(st)


# ------------------------------------- (c) certificates of the int8 bound
BOUND_CASES = [(d, t) for d in (20, 64, 260) for t in (1, 16)]
BOUND_N = 300


def bound_data(d, t):
    """(X [300, d], candidate rows [t], the first centre's row): blob rows,
    an all-zero row, a row with one feature at 1e4 over 1e-2 noise, a copy of
    a candidate, a copy of the centre."""
    rs = np.random.RandomState(100 * d + t)
    G = rs.uniform(-10.0, 10.0, (6, d))
    X = (G[rs.randint(6, size=BOUND_N)] + rs.standard_normal((BOUND_N, d))).astype(np.float32)
    cand = np.arange(t) * 17 + 10
    X[1] = 0.0
    X[2] = (1e-2 * rs.standard_normal(d)).astype(np.float32)
    X[2, 3] = 1e4
    X[4] = X[cand[0]]
    X[5] = X[0]
    return X, cand, 0


@pytest.mark.parametrize("d,t", BOUND_CASES)
def test_int8_bound_certificates(cuda, d, t):
    from sq_learn_amd.ops import _native as nat
    K = _K()
    X, cand_rows, c0 = bound_data(d, t)
    n, r = BOUND_N, R.rel_tol(d)
    X64 = X.astype(np.float64)
    Xt = torch.from_numpy(X).to(cuda)
    st = K.KmppState(Xt, 4, t, prune=True)
    m, stream, dq = st.m, st.st, st.dq
    st.Xq.fill_(99)
    st.first_centre(Xt[c0])
    torch.cuda.synchronize()
    # ---- kmpp_init: the int8 row copy and its certificate
    xq = st.Xq.cpu().numpy()
    s = st.srow.cpu().numpy()
    e = st.erow.cpu().numpy().astype(np.float64)
    assert xq.min() >= -127 and xq.max() <= 127 and (xq[:, d:] == 0).all()
    np.testing.assert_array_equal(st.xq2.cpu().numpy(), (xq.astype(np.int64) ** 2).sum(1))
    res = X64 - s.astype(np.float64)[:, None] * xq[:, :d].astype(np.float64)
    en = np.sqrt((res * res).sum(1))
    assert (e >= en).all() and (e <= en * (1.0 + 1e-5)).all()
    assert s[1] == 1.0 and e[1] == 0.0 and (xq[1] == 0).all()
    assert (s > 0).all() and (np.abs(xq).max(1)[s != 1.0] == 127).all()
    cl = st.closest[:n].cpu().numpy()
    assert cl[0] == 0.0 and cl[5] == 0.0
    # ---- kmpp_cc: the two-term candidates, ccmin, the zeroed accumulators
    cand = X[cand_rows]
    candt = torch.from_numpy(cand).to(cuda)
    C = torch.zeros((4, d), dtype=torch.float32, device=cuda)
    C[0], C[1] = Xt[c0], Xt[50]
    st.delta.fill_(7.0)
    st.counters.fill_(7)
    st.cc.fill_(7.0)
    st.candq[:, :t].fill_(7)
    rc = m.kmpp_cc(candt.data_ptr(), C.data_ptr(), 2, d, t, st.cc.data_ptr(), st.k,
                   st.cinfo.data_ptr(), st.candq.data_ptr(), dq, st.delta.data_ptr(),
                   st.delta.numel(), st.counters.data_ptr(), stream)
    assert not rc
    torch.cuda.synchronize()
    cq = st.candq.cpu().numpy()
    cinfo = st.cinfo.cpu().numpy()
    assert (cq[:, t:] == 0).all() and (cq[:, :t, d:] == 0).all()
    assert cq.min() >= -127 and cq.max() <= 127
    ct = R.cand_tilde(cq, cinfo[:, 0], t)
    assert (ct[:, d:] == 0).all()
    ecn = np.sqrt(((cand.astype(np.float64) - ct[:, :d]) ** 2).sum(1))
    assert (cinfo[:t, 1] >= ecn).all()
    np.testing.assert_allclose(cinfo[:t, 2], (ct * ct).sum(1), rtol=1e-12, atol=0.0)
    ccref = R.dist2(C[:2].cpu().numpy().astype(np.float64), cand).min(0)
    ccmin = st.cc.cpu().numpy()[:2].astype(np.float64)
    assert (np.abs(ccmin - ccref) <= r * ccref).all(), (ccmin, ccref)
    assert (st.delta == 0).all() and (st.counters == 0).all()
    # ---- kmpp_bound: every row a survivor
    rows = torch.arange(st.G * st.R, dtype=torch.int32, device=cuda)
    st.surv.copy_(rows)
    cnt = [min(st.R, n - b * st.R) for b in range(st.G)]
    st.scount.copy_(torch.tensor(cnt, dtype=torch.int32))
    st.exact.fill_(-1)
    st.ecount.fill_(7)
    rc = m.kmpp_bound(st.Xq.data_ptr(), dq, st.srow.data_ptr(), st.erow.data_ptr(),
                      st.xq2.data_ptr(), st.closest.data_ptr(), st.candq.data_ptr(),
                      st.cinfo.data_ptr(), t, d, n, st.R, st.G, st.surv.data_ptr(),
                      st.scount.data_ptr(), st.exact.data_ptr(), st.ecount.data_ptr(), stream)
    assert not rc
    torch.cuda.synchronize()
    ex, ec = st.exact.cpu().numpy(), st.ecount.cpu().numpy()
    kept = np.zeros(n, dtype=bool)
    for b in range(st.G):
        seg = ex[b * st.R:b * st.R + ec[b]]
        assert 0 <= ec[b] <= cnt[b] and len(set(seg.tolist())) == ec[b]
        assert (seg >= b * st.R).all() and (seg < b * st.R + cnt[b]).all()
        kept[seg] = True
    cl64 = cl.astype(np.float64)
    D64 = R.dist2(X64, cand)
    wrong = ~kept & (D64 <= cl64[None, :]).any(0)
    assert not wrong.any(), ("rows rejected that a trial could improve", np.nonzero(wrong)[0])
    lb = R.bound_lb64(xq, s, e, cq, cinfo[:, 0], cinfo[:, 1], t)
    must_reject = (lb > 1.001 * cl64[None, :]).all(0)
    must_keep = (lb < 0.999 * cl64[None, :]).any(0)
    assert not (kept & must_reject).any(), np.nonzero(kept & must_reject)[0]
    assert (kept | ~must_keep).all(), np.nonzero(~kept & must_keep)[0]
    assert kept[4] and must_reject.any() and must_keep.any()
