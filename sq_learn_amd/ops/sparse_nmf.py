"""Non-negative matrix factorisation ops: the Kullback-Leibler
ratio over the stored entries of a CSR matrix and the coordinate-descent
sweep.

Reference: ``decomposition/_nmf.py`` (``_special_sparse_dot``, the
multiplicative updates and ``_beta_divergence`` on sparse X) and
``decomposition/_cdnmf_fast.pyx``; the law of the sweep is
``csrc/host/decomposition_host.cpp: sqh_cdnmf_update`` operation by operation.

Device path: ``csrc/spnmf.hip`` - the ratio kernel is one wave per CSR row
(``W H`` is evaluated at the stored entries only, one wave owns an output row:
no atomics, results bit-identical from run to run and independent of how the
rows are split into calls), the sweep is one lane per row of ``W`` with the
sums in the host's order.  A GPU input always takes the native path and
raises when the extension is missing.  The torch twins (CPU) follow the same
laws in fp64: the ratio vectorised over chunks of stored entries, the sweep
vectorised over rows and sequential over the coordinates.

Values are fp32 on the GPU (the device policy of every CSR op): integer counts
are exact, other weights such as TF-IDF are rounded to fp32 there.
"""

import numpy as np
import torch

from . import _native as nat
from ._csr import chunks, csr_ptrs, native_ok

EPSILON = float(np.finfo(np.float32).eps)
# csrc/spnmf.hip, on either device (checked against the exports by the GPU tests)
STAGE = 1024            # SP_NMF_STAGE (sp_nmf_stage)
STAGE_MIN_ROW = 4       # SP_NMF_STAGE_MIN_ROW (sp_nmf_stage_min_row)
KL_MAX_K = 1024         # SP_NMF_MAX_K (sp_nmf_max_k)
CD_MAX_K = 1024         # NMF_CD_MAX_K (nmf_cd_max_k)
CD_HHT_K = 64           # NMF_CD_HHT_K (nmf_cd_hht_k)
TWIN_DOUBLES = 1 << 22  # gathered doubles (entries x k) per twin chunk


def check_kl_k(k):
    if k < 1 or k > KL_MAX_K:
        raise ValueError(f"the NMF Kullback-Leibler ratio supports 1 to {KL_MAX_K} components, "
                         f"got {k}")


def check_cd_k(k):
    if k < 1 or k > CD_MAX_K:
        raise ValueError(f"the NMF coordinate-descent sweep supports 1 to {CD_MAX_K} components, "
                         f"got {k}")


def stage_entries(k):
    """The most stored entries of a row whose gathered operand rows the ratio
    kernel stages in LDS at ``k`` components; a longer row gathers them twice
    from global memory."""
    return STAGE // max(int(k) | 1, STAGE_MIN_ROW)


def _check_rows(n, rows):
    a, b = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= a <= b <= n:
        raise ValueError(f"rows {rows} outside the {n} rows")
    return a, b


# ----------------------------------------------------------------- ratio
def nmf_kl_ratio(sd, P, Q, want_num=True, want_div=False, rows=None):
    """For every row ``i`` of ``rows = (a, b)`` (default: all) of the CSR
    matrix with stored pairs ``(c_t, x_t)``: ``wh_t = P[i] . Q[c_t]`` (0
    becomes ``EPSILON``), ``num[i] = sum_t (x_t / wh_t) Q[c_t]`` and ``div[i] =
    sum over x_t > EPSILON of x_t log(x_t / wh_t)``.

    ``P`` [n, k] and ``Q`` [d, k] fp64.  Returns ``(num, div)``: [b - a, k]
    and [b - a] fp64, ``None`` for the one not wanted.  A column outside
    [0, d) adds nothing."""
    n, d = sd.shape
    a, b = _check_rows(n, rows)
    if P.dim() != 2 or Q.dim() != 2 or P.shape[0] != n or Q.shape[0] != d \
            or P.shape[1] != Q.shape[1]:
        raise ValueError("P must be [rows of the matrix, k] and Q [columns of the matrix, k]")
    k = P.shape[1]
    check_kl_k(k)
    if not (want_num or want_div):
        raise ValueError("nothing to compute: want_num and want_div are both false")
    if not native_ok(sd):
        return nmf_kl_ratio_torch(sd, P, Q, want_num, want_div, (a, b))
    dev = sd.device
    Pd = P.to(dev, torch.float64)[a:b].contiguous()
    Qd = Q.to(dev, torch.float64).contiguous()
    num = torch.empty((b - a, k), dtype=torch.float64, device=dev) if want_num else None
    div = torch.empty(b - a, dtype=torch.float64, device=dev) if want_div else None
    nat.native().nmf.sp_nmf_kl(*csr_ptrs(sd), Pd.data_ptr(), Qd.data_ptr(), a, b - a, d, k,
                               EPSILON, nat.ptr(num), nat.ptr(div), nat.stream_handle(dev))
    return num, div


def nmf_kl_ratio_torch(sd, P, Q, want_num=True, want_div=False, rows=None,
                       chunk_doubles=TWIN_DOUBLES):
    n, d = sd.shape
    a, b = _check_rows(n, rows)
    k = P.shape[1]
    dev = sd.device
    Pd, Qd = P.to(dev, torch.float64), Q.to(dev, torch.float64)
    num = torch.zeros((b - a, k), dtype=torch.float64, device=dev) if want_num else None
    div = torch.zeros(b - a, dtype=torch.float64, device=dev) if want_div else None
    lo, hi = int(sd.indptr[a]), int(sd.indptr[b])
    for s, e in chunks(hi - lo, max(1, chunk_doubles // k)):
        ii = sd.row_ids()[lo + s:lo + e]
        jj = sd.indices[lo + s:lo + e].to(torch.int64)
        ok = (jj >= 0) & (jj < d)
        jj = torch.where(ok, jj, 0)
        x = torch.where(ok, sd.data[lo + s:lo + e].double(), 0.0)
        q = Qd[jj]
        wh = (Pd[ii] * q).sum(1)
        wh = torch.where(wh == 0, EPSILON, wh)
        if want_num:
            num.index_add_(0, ii - a, (x / wh)[:, None] * q)
        if want_div:
            big = x > EPSILON
            term = torch.where(big, x, 1.0) * torch.log(torch.where(big, x / wh, 1.0))
            div.index_add_(0, ii - a, torch.where(big, term, 0.0))
    return num, div


# ----------------------------------------------------------------- sweep
def nmf_cd_sweep(W, HHt, XHt, perm, rows=None):
    """One coordinate-descent sweep over the rows ``rows = (a, b)`` (default:
    all) of ``W`` [n, k] fp64, in place: for ``s`` in order, ``t = perm[s]``,
    ``grad = -XHt[i, t] + sum_r HHt[t, r] W[i, r]``, ``W[i, t] = max(W[i, t] -
    grad / HHt[t, t], 0)`` unless ``HHt[t, t]`` is 0.  Returns the sum of the
    projected-gradient magnitudes as a 0-d fp64 tensor on the device of ``W``
    (no host synchronisation)."""
    if W.dim() != 2 or W.dtype != torch.float64 or not W.is_contiguous():
        raise ValueError("W must be a contiguous fp64 matrix (it is updated in place)")
    n, k = W.shape
    check_cd_k(k)
    a, b = _check_rows(n, rows)
    if tuple(HHt.shape) != (k, k) or tuple(XHt.shape) != (n, k) or perm.numel() != k:
        raise ValueError("HHt must be [k, k], XHt [n, k] and perm a permutation of k")
    dev = W.device
    HHt = HHt.to(dev, torch.float64).contiguous()
    XHt = XHt.to(dev, torch.float64).contiguous()
    perm = torch.as_tensor(perm, dtype=torch.int64).to(dev).contiguous()
    if not nat.use_native(W):
        return nmf_cd_sweep_torch(W, HHt, XHt, perm, (a, b))
    rowviol = torch.empty(max(b - a, 1), dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=torch.float64, device=dev)
    nat.native().nmf.nmf_cd_sweep(W.data_ptr(), HHt.data_ptr(), XHt.data_ptr(), perm.data_ptr(),
                                  a, b - a, k, rowviol.data_ptr(), out.data_ptr(),
                                  nat.stream_handle(dev))
    return out


def nmf_cd_sweep_torch(W, HHt, XHt, perm, rows=None):
    n, k = W.shape
    a, b = _check_rows(n, rows)
    Wv, Xv = W[a:b], XHt[a:b]
    viol = torch.zeros((), dtype=torch.float64, device=W.device)
    for t in perm.tolist():
        if not 0 <= t < k:
            continue
        grad = Wv @ HHt[t] - Xv[:, t]
        wt = Wv[:, t]
        viol = viol + torch.where(wt == 0, grad.clamp(max=0.0), grad).abs().sum()
        hess = float(HHt[t, t])
        if hess != 0.0:
            Wv[:, t] = (wt - grad / hess).clamp(min=0.0)
    return viol
