"""Logistic-regression ops on CSR rows: the multinomial and the binary loss
with their residuals and the CSR matrix-vector product (``LogisticRegression``
on ``scipy.sparse`` rows with an explicit device).

Reference: ``linear_model/_logistic.py`` (``_multinomial_loss``,
``_logistic_loss_and_grad``), which keep sparse X sparse through
``safe_sparse_dot``.

Device path: ``csrc/splogit.hip`` - one wave per CSR row; the multinomial
kernel puts its lanes across the classes and fuses the row's logits, the
max-shifted logsumexp and the residual, the binary kernel puts them across the
row's stored entries.  ``sp_matvec`` runs over the segment table of
``ops/sparse_linalg.py``, so the long rows of a transposed text matrix are
balanced.  No floating-point atomics: results are bit-identical from run to
run and independent of the launch geometry.  A GPU input always takes the
native path and raises when the extension is missing.  The torch twins (CPU)
follow the same mathematics in fp64 over the stored entries (``row_ids`` and
``index_add_``): nothing of size n x d is ever allocated.

Values are fp32 on the GPU (the device policy of every CSR op); all
arithmetic and all outputs are fp64.
"""

import torch

from . import _native as nat
from ._csr import chunks, csr_ptrs, native_ok
from .sparse_linalg import segments, sp_xty

TILE_CLASSES = 256      # classes per pass of the multinomial kernel (sp_logit_tile_classes)
TWIN_DOUBLES = 1 << 22  # gathered doubles (entries x K) per twin chunk


def pad_classes(K):
    """The column count of the transposed weights at ``K`` classes."""
    return 64 * ((int(K) + 63) // 64)


def transposed_weights(W, device):
    """``W`` [K, d] as the fp64 operand ``Wt`` [d, pad_classes(K)] of
    ``logit_multi`` on ``device``, zeros in the padding."""
    W = torch.as_tensor(W, dtype=torch.float64).to(device)
    K, d = W.shape
    Wt = torch.zeros((d, pad_classes(K)), dtype=torch.float64, device=W.device)
    Wt[:, :K] = W.T
    return Wt


def _vec(a, n, what, dev, dtype=torch.float64):
    a = torch.as_tensor(a)
    if a.dim() != 1 or a.shape[0] != n:
        raise ValueError(f"{what} of shape {tuple(a.shape)} does not match {n}")
    return a.to(device=dev, dtype=dtype).contiguous()


def _labels(lab, n, K, dev):
    lab = torch.as_tensor(lab)
    if lab.is_floating_point():
        raise TypeError("the class indices must be integers")
    lab = _vec(lab, n, "the class indices", dev, torch.int32)
    if n and (int(lab.min()) < 0 or int(lab.max()) >= K):
        raise ValueError(f"a class index lies outside [0, {K})")
    return lab


# ------------------------------------------------------------ multinomial
def logit_multi(sd, Wt, b, lab, sw):
    """Multinomial loss and residual of the CSR rows: with ``z_i = x_i Wt[:, :K]
    + b``, ``loss = sum_i sw_i (logsumexp(z_i) - z_i[lab_i])`` (a 0-d fp64
    tensor on the device of ``sd``) and ``R[i, c] = sw_i (softmax(z_i)_c -
    [c == lab_i])`` [n, K] fp64.

    ``Wt`` [d, pad_classes(K)] fp64 (``transposed_weights``), ``b`` [K],
    ``lab`` [n] integers in [0, K), ``sw`` [n]."""
    n, d = sd.shape
    dev = sd.device
    b = torch.as_tensor(b)
    if b.dim() != 1 or b.shape[0] < 1:
        raise ValueError("the intercepts must be a vector with one entry per class")
    K = b.shape[0]
    if Wt.dim() != 2 or tuple(Wt.shape) != (d, pad_classes(K)):
        raise ValueError(f"the transposed weights of shape {tuple(Wt.shape)} do not match a "
                         f"matrix with {d} columns and {K} classes padded to {pad_classes(K)}")
    b = b.to(device=dev, dtype=torch.float64).contiguous()
    lab = _labels(lab, n, K, dev)
    sw = _vec(sw, n, "the row weights", dev)
    Wt = Wt.to(device=dev, dtype=torch.float64).contiguous()
    if not native_ok(sd):
        return logit_multi_torch(sd, Wt, b, lab, sw)
    R = torch.empty((n, K), dtype=torch.float64, device=dev)
    rowloss = torch.empty(n, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    nat.native().logistic.sp_logit_multi(*csr_ptrs(sd), Wt.data_ptr(), Wt.shape[1], b.data_ptr(),
                                         lab.data_ptr(), sw.data_ptr(), n, K, R.data_ptr(),
                                         rowloss.data_ptr(), loss.data_ptr(),
                                         nat.stream_handle(dev))
    return loss, R


def logit_multi_torch(sd, Wt, b, lab, sw, chunk_doubles=TWIN_DOUBLES):
    n = sd.shape[0]
    K = b.shape[0]
    z = torch.zeros((n, K), dtype=torch.float64, device=sd.device)
    for s, e in chunks(sd.nnz, max(1, chunk_doubles // K)):
        rows = Wt[sd.indices[s:e].to(torch.int64), :K]
        z.index_add_(0, sd.row_ids()[s:e], sd.data[s:e].double()[:, None] * rows)
    z += b
    lse = torch.logsumexp(z, dim=1)
    ar = torch.arange(n, device=sd.device)
    pick = lab.to(torch.int64)
    loss = (sw * (lse - z[ar, pick])).sum()
    R = torch.exp(z - lse[:, None])
    R[ar, pick] -= 1.0
    R *= sw[:, None]
    return loss, R


def sp_xtr(sd, R, chunk_doubles=TWIN_DOUBLES):
    """The multinomial gradient ``X^T R`` [d, K] fp64: ``sp_xty`` on a GPU; on
    the CPU a sum over the stored entries (the twin of ``sp_xty`` works on
    densified row chunks)."""
    if native_ok(sd):
        return sp_xty(sd, R)
    n, d = sd.shape
    if R.dim() != 2 or R.shape[0] != n:
        raise ValueError(f"operand of shape {tuple(R.shape)} does not match a matrix with {n} "
                         "rows")
    K = R.shape[1]
    Z = torch.zeros((d, K), dtype=torch.float64, device=sd.device)
    for s, e in chunks(sd.nnz, max(1, chunk_doubles // K)):
        Z.index_add_(0, sd.indices[s:e].to(torch.int64),
                     sd.data[s:e].double()[:, None] * R[sd.row_ids()[s:e]])
    return Z


# ----------------------------------------------------------------- binary
def logit_bin(sd, w, b, lab, sw):
    """Binary loss and residual of the CSR rows: with ``z_i = x_i . w + b``
    and ``t_i = +1`` for ``lab_i != 0``, else ``-1``: ``loss = sum_i sw_i
    softplus(-t_i z_i)`` (a 0-d fp64 tensor on the device of ``sd``) and ``r_i
    = sw_i (sigmoid(t_i z_i) - 1) t_i`` [n] fp64.

    ``w`` [d] fp64, ``b`` a number, ``lab`` [n] integers in {0, 1}, ``sw`` [n]."""
    n, d = sd.shape
    dev = sd.device
    w = _vec(w, d, "the weights", dev)
    lab = _labels(lab, n, 2, dev)
    sw = _vec(sw, n, "the row weights", dev)
    b = float(b)
    if not native_ok(sd):
        return logit_bin_torch(sd, w, b, lab, sw)
    r = torch.empty(n, dtype=torch.float64, device=dev)
    rowloss = torch.empty(n, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    nat.native().logistic.sp_logit_bin(*csr_ptrs(sd), w.data_ptr(), b, lab.data_ptr(),
                                       sw.data_ptr(), n, d, r.data_ptr(), rowloss.data_ptr(),
                                       loss.data_ptr(), nat.stream_handle(dev))
    return loss, r


def logit_bin_torch(sd, w, b, lab, sw):
    t = torch.where(lab != 0, 1.0, -1.0).to(torch.float64)
    tz = t * (sp_matvec_torch(sd, w) + b)
    loss = (sw * (torch.clamp(-tz, min=0.0) + torch.log1p(torch.exp(-tz.abs())))).sum()
    return loss, -sw * t / (1.0 + torch.exp(tz))


# ---------------------------------------------------------- matrix-vector
def sp_matvec(sd, x, seg=None):
    """``y = A x`` in fp64 [n]: ``A`` CSR [n, d], ``x`` [d].  On the cached
    transpose (``_csr.csr_transpose``) this is ``X^T r``."""
    n, d = sd.shape
    dev = sd.device
    x = _vec(x, d, "the vector", dev)
    if not native_ok(sd):
        return sp_matvec_torch(sd, x)
    tab = segments(sd, seg)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    scratch = torch.empty(max(tab.slots, 1), dtype=torch.float64, device=dev)
    nat.native().logistic.sp_matvec(*csr_ptrs(sd), tab.row.data_ptr(), tab.start.data_ptr(),
                                    tab.dst.data_ptr(), tab.nseg, tab.seg,
                                    tab.long_row.data_ptr(), tab.long_ptr.data_ptr(), tab.nlong,
                                    x.data_ptr(), d, y.data_ptr(), scratch.data_ptr(),
                                    nat.stream_handle(dev))
    return y


def sp_matvec_torch(sd, x):
    y = torch.zeros(sd.shape[0], dtype=torch.float64, device=sd.device)
    if sd.nnz:
        y.index_add_(0, sd.row_ids(), sd.data.double() * x[sd.indices.to(torch.int64)])
    return y
