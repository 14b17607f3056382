"""CSR latent Dirichlet allocation ops (the topic model).

Reference: ``decomposition/_online_lda_fast.pyx`` and the per-document loop of
``decomposition/_lda.py``; the law is ``csrc/host/decomposition_host.cpp:
sqh_lda_estep`` operation by operation.

Device path: ``csrc/splda.hip`` - one wave per document, the transposed
``exp_tw`` table [F, k] gathered by the document's column indices, the
sufficient statistics by 64-bit fixed-point integer atomics (order
independent, bit-reproducible, independent of how the rows are split into
calls).  A GPU input always takes the native path and raises when the
extension is missing.  The torch twins (CPU) follow the same law in fp64,
vectorised over chunks of documents padded to the chunk's longest document; a
document that met the stopping rule is frozen while its chunk goes on.

Values are fp32 on the GPU (the device policy of every CSR op): integer counts
are exact, other weights such as TF-IDF are rounded to fp32 there.
"""

import math

import torch

from . import _native as nat
from . import kmeans as K
from ._csr import chunks, csr_ptrs, native_ok

EPS = 2.220446049250313e-16
MAX_K = 4096            # csrc/splda.hip: SP_LDA_MAX_K (sp_lda_max_k), on either device
TWIN_DOUBLES = 1 << 22  # gathered doubles (documents x longest x k) per twin chunk


def check_k(k):
    if k < 1 or k > MAX_K:
        raise ValueError(f"the LDA E-step supports 1 to {MAX_K} topics, got {k}")


def stage_words(k):
    """The most stored words of a document whose gathered rows the kernel
    stages in LDS at ``k`` topics; a longer document re-gathers them from
    global memory on every iteration."""
    return nat.native().lda.sp_lda_stage() // (int(k) | 1)


def _check_scalars(prior, tol):
    prior, tol = float(prior), float(tol)
    if not (prior > 0.0 and math.isfinite(prior)):
        raise ValueError(f"doc_topic prior must be positive and finite, got {prior}")
    if not math.isfinite(tol):
        raise ValueError(f"tol must be finite, got {tol}")
    return prior, tol


def _check_rows(sd, rows):
    a, b = (0, sd.shape[0]) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= a <= b <= sd.shape[0]:
        raise ValueError(f"rows {rows} outside the {sd.shape[0]} documents")
    return a, b


class LdaStats:
    """The int64 quanta of the E-step statistics: a plane of quanta ``2^hexp``
    and a plane of remainders in quanta ``2^lexp``, both [F, k].  Every addend
    is at most a stored count, and a column's total at most its column sum, so
    ``hexp = fixed_point_exp(max|x|, largest column count)`` keeps every sum
    of the first plane below 2^52 quanta.  A remainder is at most half a
    coarse quantum, ``2^(hexp - lexp - 1)`` fine ones, and ``lexp`` is chosen
    so that a column's remainders stay below 2^62.  Calls over disjoint row
    ranges may share one object: integer addition commutes, so the result is
    the one of a single call over all the rows, bit for bit."""

    def __init__(self, sd, k):
        bound = sd._lda_bound
        if bound is None:
            mx = float(sd.data.abs().max()) if sd.nnz else 0.0
            cc = int(torch.bincount(sd.indices.to(torch.int64)).max()) if sd.nnz else 0
            bound = sd._lda_bound = (mx, cc)
        mx, cc = bound
        self.hexp = K.fixed_point_exp(mx, cc)
        self.lexp = self.hexp - min(53, 62 - max(cc - 1, 0).bit_length())
        self.k = int(k)
        self.q = torch.zeros((2, sd.shape[1], self.k), dtype=torch.int64, device=sd.device)

    def finish(self):
        """The statistics [k, F] fp64, already multiplied by ``exp_tw``."""
        ss_t = self.q[0].double() * math.ldexp(1.0, self.hexp) \
            + self.q[1].double() * math.ldexp(1.0, self.lexp)
        return ss_t.T.contiguous()


# ---------------------------------------------------------------- E-step
def lda_estep(sd, exp_tw_t, doc_topic, prior, max_iters, tol, rows=None, want_stats=True,
              want_iters=False, stats=None):
    """Variational E-step of the documents ``rows = (a, b)`` (default: all).

    ``exp_tw_t`` [F, k] fp64 is ``exp(E[log beta])`` transposed, ``doc_topic``
    [b - a, k] fp64 the initial distribution.  Returns ``(doc_topic, ss,
    iters)``: the fitted distribution (a new tensor), the statistics [k, F]
    fp64 already multiplied by ``exp_tw`` (``None`` without ``want_stats``)
    and the iterations every document performed (int32; ``None`` without
    ``want_iters``).  ``stats`` (GPU): an :class:`LdaStats` to accumulate
    into, shared between calls over disjoint row ranges; ``ss`` is then the
    total so far."""
    a, b = _check_rows(sd, rows)
    F = sd.shape[1]
    k = exp_tw_t.shape[1]
    check_k(k)
    prior, tol = _check_scalars(prior, tol)
    if exp_tw_t.shape[0] != F or tuple(doc_topic.shape) != (b - a, k):
        raise ValueError("exp_tw_t must be [n_features, k] and doc_topic [rows, k]")
    if not native_ok(sd):
        if stats is not None:
            raise ValueError("stats= accumulates the kernel's integer quanta: GPU input only")
        return lda_estep_torch(sd, exp_tw_t, doc_topic, prior, max_iters, tol, (a, b), want_stats,
                               want_iters)
    dev = sd.device
    tw = exp_tw_t.to(dev, torch.float64).contiguous()
    dt = doc_topic.to(dev, torch.float64).contiguous().clone()
    iters = torch.zeros(b - a, dtype=torch.int32, device=dev) if want_iters else None
    if want_stats and stats is None:
        stats = LdaStats(sd, k)
    if not want_stats:
        stats = None
    if stats is not None:
        assert stats.k == k and stats.q.shape[1] == F and stats.q.device == dev
    q = (0, 0, 0, 0) if stats is None else (stats.q[0].data_ptr(), stats.q[1].data_ptr(),
                                            stats.hexp, stats.lexp)
    nat.native().lda.sp_lda_estep(*csr_ptrs(sd), tw.data_ptr(), dt.data_ptr(), a, b - a, F, k,
                                  prior, int(max_iters), tol, nat.ptr(iters), *q,
                                  nat.stream_handle(dev))
    return dt, (None if stats is None else stats.finish()), iters


def _padded(sd, s, e):
    """(idx [B, L] int64, cnt [B, L] fp64) of the documents [s, e), padded
    with (0, 0) to the longest; a column outside [0, F) becomes (0, 0)."""
    ptr = sd.indptr[s:e + 1]
    lens = ptr[1:] - ptr[:-1]
    L = max(int(lens.max()) if e > s else 0, 1)
    t = torch.arange(L, dtype=torch.int64, device=sd.device)
    live = t[None, :] < lens[:, None]
    src = torch.where(live, ptr[:-1, None] + t[None, :], 0)
    if sd.nnz == 0:
        z = torch.zeros((e - s, L), dtype=torch.int64, device=sd.device)
        return z, z.double()
    idx = sd.indices[src].to(torch.int64)
    live &= (idx >= 0) & (idx < sd.shape[1])
    return torch.where(live, idx, 0), torch.where(live, sd.data[src].double(), 0.0)


def psi(x):
    """The digamma of the host file and of the kernel, elementwise in torch:
    the recurrence up to x >= 6, then the same asymptotic series.  Its
    truncation error (about 1e-13 at x = 6) is part of the law:
    ``torch.special.digamma`` is more accurate and therefore disagrees with
    the host path by that much.  An argument that is not positive gives NaN."""
    x = torch.where(x > 0, x, torch.nan)
    r = torch.zeros_like(x)
    for _ in range(6):
        low = x < 6.0
        r = torch.where(low, r - 1.0 / x, r)
        x = torch.where(low, x + 1.0, x)
    f = 1.0 / (x * x)
    t = f * (-1.0 / 12 + f * (1.0 / 120 + f * (-1.0 / 252 + f * (1.0 / 240 + f * (
        -1.0 / 132 + f * (691.0 / 32760 + f * (-1.0 / 12)))))))
    return r + torch.log(x) - 0.5 / x + t


def dirichlet_expectation(a):
    """E[log X] of the rows of ``a`` under Dirichlet(a): psi(a) - psi(row sum)."""
    return psi(a) - psi(a.sum(1, keepdim=True))


def _exp_dirichlet(dt):
    return torch.exp(dirichlet_expectation(dt))


def lda_estep_torch(sd, exp_tw_t, doc_topic, prior, max_iters, tol, rows=None, want_stats=True,
                    want_iters=False, chunk_doubles=TWIN_DOUBLES):
    a, b = _check_rows(sd, rows)
    F = sd.shape[1]
    k = exp_tw_t.shape[1]
    prior, tol = _check_scalars(prior, tol)
    dev = sd.device
    tw_t = exp_tw_t.to(dev, torch.float64)
    out = doc_topic.to(dev, torch.float64).clone()
    iters = torch.zeros(b - a, dtype=torch.int32, device=dev)
    ss_t = torch.zeros((F, k), dtype=torch.float64, device=dev) if want_stats else None
    lens = sd.indptr[a + 1:b + 1] - sd.indptr[a:b]
    longest = max(int(lens.max()) if b > a else 0, 1)
    step = max(1, chunk_doubles // (longest * k))
    for s, e in chunks(b - a, step):
        idx, cnt = _padded(sd, a + s, a + e)
        tw = tw_t[idx]                                   # [B, L, k]
        dt = out[s:e].clone()
        edt = _exp_dirichlet(dt)
        live = torch.ones(e - s, dtype=torch.bool, device=dev)
        it = torch.zeros(e - s, dtype=torch.int32, device=dev)
        for _ in range(int(max_iters)):
            if not bool(live.any()):
                break
            norm = torch.einsum("blk,bk->bl", tw, edt) + EPS
            nd = edt * torch.einsum("bl,blk->bk", cnt / norm, tw) + prior
            diff = (dt - nd).abs().sum(1) / k
            # a finished document is frozen while the chunk goes on
            dt = torch.where(live[:, None], nd, dt)
            edt = torch.where(live[:, None], _exp_dirichlet(nd), edt)
            it += live.to(torch.int32)
            live = live & ~(diff < tol)
        out[s:e] = dt
        iters[s:e] = it
        if want_stats:
            norm = torch.einsum("blk,bk->bl", tw, edt) + EPS
            add = (cnt / norm)[:, :, None] * edt[:, None, :] * tw
            ss_t.index_add_(0, idx.reshape(-1), add.reshape(-1, k))
    return out, (ss_t.T.contiguous() if want_stats else None), (iters if want_iters else None)


# ----------------------------------------------------------------- bound
def lda_doc_bound(sd, elog_theta, elog_beta_t, rows=None):
    """Per document of ``rows = (a, b)``: sum_t cnt_t logsumexp_j(
    elog_theta[row, j] + elog_beta_t[idx_t, j]), fp64 [b - a]."""
    a, b = _check_rows(sd, rows)
    F = sd.shape[1]
    k = elog_beta_t.shape[1]
    check_k(k)
    if elog_beta_t.shape[0] != F or tuple(elog_theta.shape) != (b - a, k):
        raise ValueError("elog_beta_t must be [n_features, k] and elog_theta [rows, k]")
    if not native_ok(sd):
        return lda_doc_bound_torch(sd, elog_theta, elog_beta_t, (a, b))
    dev = sd.device
    et = elog_theta.to(dev, torch.float64).contiguous()
    eb = elog_beta_t.to(dev, torch.float64).contiguous()
    out = torch.zeros(b - a, dtype=torch.float64, device=dev)
    nat.native().lda.sp_lda_bound(*csr_ptrs(sd), et.data_ptr(), eb.data_ptr(), a, b - a, F, k,
                                  out.data_ptr(), nat.stream_handle(dev))
    return out


def lda_doc_bound_torch(sd, elog_theta, elog_beta_t, rows=None, chunk_doubles=TWIN_DOUBLES):
    a, b = _check_rows(sd, rows)
    k = elog_beta_t.shape[1]
    dev = sd.device
    et = elog_theta.to(dev, torch.float64)
    eb = elog_beta_t.to(dev, torch.float64)
    out = torch.zeros(b - a, dtype=torch.float64, device=dev)
    lens = sd.indptr[a + 1:b + 1] - sd.indptr[a:b]
    longest = max(int(lens.max()) if b > a else 0, 1)
    step = max(1, chunk_doubles // (longest * k))
    for s, e in chunks(b - a, step):
        idx, cnt = _padded(sd, a + s, a + e)
        lse = torch.logsumexp(et[s:e, None, :] + eb[idx], dim=2)      # max-shifted
        out[s:e] = (cnt * lse).sum(1)
    return out
