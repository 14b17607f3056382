"""CSR sparse-times-dense products in fp64: the row passes of
the randomized SVD on sparse input (``utils.extmath.randomized_svd_sparse``,
``TruncatedSVD`` on ``scipy.sparse`` rows).

Device path: ``csrc/spmm.hip`` - one wave per row segment of at most ``seg``
nonzeros, lanes across the columns of the dense operand, every nonzero one
contiguous row gather; rows longer than a segment go through per-segment
partials that a second kernel adds in segment order.  ``Y = X W`` runs the
kernel on X, ``Z = X^T Y`` runs the same kernel on the CSR of X^T
(``_csr.csr_transpose``, built once per matrix with torch plumbing and cached
on the ``SparseData``), so both products are gathers: no floating-point
atomics, results bit-identical from run to run and independent of the launch
geometry.  ``sp_mu_power_sums`` (``csrc/spmu.hip``): the mu(A) power sums of
the matrix centred by a column mean, as sums over the stored entries (PCA /
qPCA on sparse rows).  A GPU input always takes the native path and raises
when the extension is missing.  The torch twins (CPU) work in fp64 over
densified row chunks, as ``ops/sparse_kmeans.py`` does.
"""

import torch

from . import _native as nat
from ._csr import TWIN_CHUNK, chunks, csr_ptrs, csr_transpose, native_ok

SEG_DEFAULT = 1024     # nonzeros per unit of work (one wave)


# ----------------------------------------------------------- segment table
class Segments:
    """Row segments of at most ``seg`` nonzeros (int64 tensors on the device
    of the matrix).  Segment g covers the nonzeros ``start[g] .. start[g] +
    seg`` (cut at the row end) of row ``row[g]``; ``dst[g]`` is -1 for the
    only segment of a row (an empty row has one empty segment: it writes
    zeros) and the slot of the segment's partial otherwise.  Row
    ``long_row[r]`` owns the slots ``long_ptr[r] .. long_ptr[r + 1]``."""

    def __init__(self, sd, seg):
        n, dev = sd.shape[0], sd.device
        cnt = sd.indptr[1:] - sd.indptr[:-1]
        per_row = torch.clamp((cnt + (seg - 1)) // seg, min=1)
        self.seg = int(seg)
        self.nseg = int(per_row.sum())
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        self.row = torch.repeat_interleave(ar, per_row, output_size=self.nseg)
        first = torch.cumsum(per_row, 0) - per_row
        k = torch.arange(self.nseg, dtype=torch.int64, device=dev) - first[self.row]
        self.start = sd.indptr[:-1][self.row] + k * seg
        is_long = per_row > 1
        self.long_row = torch.nonzero(is_long).reshape(-1)
        self.nlong = int(self.long_row.numel())
        self.long_ptr = torch.zeros(self.nlong + 1, dtype=torch.int64, device=dev)
        self.long_ptr[1:] = torch.cumsum(per_row[self.long_row], 0)
        self.slots = int(self.long_ptr[-1])
        rank = torch.cumsum(is_long.to(torch.int64), 0) - 1
        self.dst = torch.where(is_long[self.row], self.long_ptr[rank.clamp(min=0)[self.row]] + k,
                               torch.full_like(k, -1))


def segments(sd, seg=None):
    """The (cached) segment table of ``sd`` for segments of ``seg`` nonzeros."""
    seg = SEG_DEFAULT if seg is None else int(seg)
    if seg < 1:
        raise ValueError(f"seg must be at least 1, got {seg}")
    if seg not in sd._segments:
        sd._segments[seg] = Segments(sd, seg)
    return sd._segments[seg]


def svd_bytes(sd, l, seg=None, centred=False, nq=0):
    """Device bytes a sparse randomized SVD with ``l`` range vectors keeps:
    X and X^T (values, indices, row pointers), their segment tables, one
    n x l and one d x l fp64 block and the scratch for long rows (at most
    nnz / seg + 1 partials beyond one per long row, bounded by 2 nnz / seg + 1
    slots on either side).  ``centred``: a second n x l block (the rank-one
    terms are applied to the product before the next one reads it).  ``nq``:
    the mu(A) pass of ``nq`` exponents on top (nq x d column sums, its
    partials)."""
    seg = SEG_DEFAULT if seg is None else int(seg)
    n, d = sd.shape
    csr = 2 * sd.nnz * 8 + (n + d + 2) * 8
    tables = 3 * 8 * (n + d + 2 * (sd.nnz // seg + 1))
    scratch = (2 * sd.nnz // seg + 1) * l * 8
    extra = n * l * 8 if centred else 0
    if nq:
        extra += nq * 8 * (d + 8192 + 2 * sd.nnz // seg + 1)
    return csr + tables + (n + d) * l * 8 + scratch + extra


def check_svd_memory(sd, l, seg=None, centred=False, nq=0):
    if sd.device.type != "cuda":
        return
    # X itself is already resident
    need = svd_bytes(sd, l, seg, centred, nq) - (sd.nnz * 8 + (sd.shape[0] + 1) * 8)
    free = torch.cuda.mem_get_info(sd.device)[0]
    if need > free:
        blocks = "two n x l blocks and a d x l fp64 block" if centred else \
            "an n x l and a d x l fp64 block"
        mu = f", the {nq} x d column sums of mu(A)" if nq else ""
        raise ValueError(f"sparse randomized SVD of a {sd.shape[0]} x {sd.shape[1]} matrix with "
                         f"{sd.nnz} stored values and {l} range vectors needs {need} more bytes "
                         f"of device memory (the transposed matrix, {blocks}, the long-row "
                         f"scratch{mu}); {free} are free")


# ---------------------------------------------------------------- products
def sp_xw(sd, W, out=None, seg=None):
    """Y = X W in fp64: X CSR [n, d], W dense [d, l].  ``out`` (fp64, unit
    column stride, any row stride): every element of ``out[:, :l]`` is
    written, nothing else.  Returns ``out[:, :l]``."""
    n, d = sd.shape
    if W.dim() != 2 or W.shape[0] != d:
        raise ValueError(f"operand of shape {tuple(W.shape)} does not match a matrix with {d} "
                         "columns")
    l = W.shape[1]
    if l < 1:
        raise ValueError("the dense operand needs at least one column")
    dev = sd.device
    Wd = W.to(device=dev, dtype=torch.float64)
    if out is None:
        out = torch.empty((n, l), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] < n or out.shape[1] < l \
            or (out.shape[1] > 1 and out.stride(1) != 1) or out.device != dev:
        raise ValueError("out must be an fp64 matrix of at least n x l with unit column stride "
                         "on the device of the sparse matrix")
    if not native_ok(sd):
        return sp_xw_torch(sd, Wd, out)
    if Wd.stride(1) != 1 or Wd.stride(0) < l:
        Wd = Wd.contiguous()
    tab = segments(sd, seg)
    scratch = torch.empty(max(tab.slots * l, 1), dtype=torch.float64, device=dev)
    ldo = out.stride(0) if n > 1 else max(out.stride(0), l)
    nat.native().spmm(*csr_ptrs(sd), tab.row.data_ptr(), tab.start.data_ptr(),
                      tab.dst.data_ptr(), tab.nseg, tab.seg, tab.long_row.data_ptr(),
                      tab.long_ptr.data_ptr(), tab.nlong, Wd.data_ptr(), max(Wd.stride(0), l), l,
                      out.data_ptr(), ldo, scratch.data_ptr(), nat.stream_handle(dev))
    return out[:n, :l]


def sp_xw_torch(sd, W, out=None):
    n = sd.shape[0]
    l = W.shape[1]
    Wd = W.to(torch.float64)
    if out is None:
        out = torch.empty((n, l), dtype=torch.float64, device=sd.device)
    for a, b in chunks(n, TWIN_CHUNK):
        out[a:b, :l] = sd.dense_rows(a, b) @ Wd
    return out[:n, :l]


def sp_xty(sd, Y, seg=None):
    """Z = X^T Y in fp64 [d, l]: the gather kernel on the cached transpose."""
    n, d = sd.shape
    if Y.dim() != 2 or Y.shape[0] != n:
        raise ValueError(f"operand of shape {tuple(Y.shape)} does not match a matrix with {n} "
                         "rows")
    if not native_ok(sd):
        return sp_xty_torch(sd, Y.to(sd.device))
    return sp_xw(csr_transpose(sd), Y, seg=seg)


def sp_xty_torch(sd, Y):
    n, d = sd.shape
    Yd = Y.to(torch.float64)
    Z = torch.zeros((d, Y.shape[1]), dtype=torch.float64, device=sd.device)
    for a, b in chunks(n, TWIN_CHUNK):
        Z += sd.dense_rows(a, b).T @ Yd[a:b]
    return Z


def sp_power_iter(sd, Z):
    """X^T (X Z) in fp64 [d, l]: one step of the range finder."""
    if not native_ok(sd):
        Zd = Z.to(device=sd.device, dtype=torch.float64)
        out = torch.zeros_like(Zd)
        for a, b in chunks(sd.shape[0], TWIN_CHUNK):
            Xc = sd.dense_rows(a, b)
            out += Xc.T @ (Xc @ Zd)
        return out
    return sp_xty(sd, sp_xw(sd, Z))


def sp_col_moments(sd):
    """(sum, sum of squares) of every column over the rows, fp64 [d] each:
    the row moments of the cached transpose (fixed summation order)."""
    d = sd.shape[1]
    if not native_ok(sd):
        return sp_col_moments_torch(sd)
    t = csr_transpose(sd)
    s = torch.empty(d, dtype=torch.float64, device=sd.device)
    ss = torch.empty(d, dtype=torch.float64, device=sd.device)
    nat.native().sp_row_moments(t.indptr.data_ptr(), t.data.data_ptr(), s.data_ptr(),
                                ss.data_ptr(), d, nat.stream_handle(sd.device))
    return s, ss


def sp_col_moments_torch(sd):
    d = sd.shape[1]
    s = torch.zeros(d, dtype=torch.float64, device=sd.device)
    ss = torch.zeros(d, dtype=torch.float64, device=sd.device)
    if sd.nnz:
        v = sd.data.double()
        c = sd.indices.to(torch.int64)
        s.index_add_(0, c, v)
        ss.index_add_(0, c, v * v)
    return s, ss


# ------------------------------------------------------------------ mu(A)
def arithmetic_grid_step(exponents):
    """b when the exponents are 0, b, 2b, ... (b > 0, the 2p of a p-grid; the
    test of ``ops/linalg.mu_power_sums_local``), else 0.0."""
    if len(exponents) >= 2 and exponents[0] == 0.0 and exponents[1] > 0.0:
        b = float(exponents[1])
        if all(abs(float(e) - i * b) <= 1e-9 * max(1.0, i * b) for i, e in enumerate(exponents)):
            return b
    return 0.0


def sp_mu_power_sums(sd, exponents, mean=None, seg=None):
    """(rowmax [nq], colsum [nq, d]) in fp64 of a = X - mean (``mean`` [d],
    optional; a = X without it, where unstored entries contribute nothing):

        rowmax[i] = max_r sum_j |a_rj|^q_i       colsum[i, j] = sum_r |a_rj|^q_i

    with |0|^q = 0 for every q (q = 0 counts the nonzero a), the convention of
    ``ops/linalg.mu_power_sums_local``.  The centred matrix is never formed:
    csrc/spmu.hip sums over the stored entries (one pass over X, one over the
    cached transpose; no atomics, bit-identical from run to run).  An
    arithmetic exponent grid 0, b, 2b, ... takes its powers by products."""
    n, d = sd.shape
    exps = [float(e) for e in exponents]
    nq = len(exps)
    if nq < 1 or min(exps) < 0.0:
        raise ValueError("mu(A) needs at least one exponent, none of them negative")
    if mean is not None:
        mean = mean.to(device=sd.device, dtype=torch.float64).reshape(-1).contiguous()
        if mean.numel() != d:
            raise ValueError(f"mean of {mean.numel()} values does not match a matrix with {d} "
                             "columns")
    if not native_ok(sd):
        return sp_mu_power_sums_torch(sd, exps, mean)
    dev = sd.device
    t = csr_transpose(sd)
    tab = segments(t, seg)
    q = torch.tensor(exps, dtype=torch.float64, device=dev)
    base = None
    if mean is not None:
        # sum_j |m_j|^q, the power sum of a row without stored entries
        am = mean.abs()
        nz = am != 0
        lg = torch.log(torch.where(nz, am, torch.ones_like(am)))
        base = torch.stack([nz.sum().double() if e == 0 else
                            torch.where(nz, torch.exp(e * lg), torch.zeros_like(am)).sum()
                            for e in exps])
    rowmax = torch.empty(nq, dtype=torch.float64, device=dev)
    colsum = torch.empty((nq, d), dtype=torch.float64, device=dev)
    lib = nat.native().mu
    part = torch.empty((lib.sp_mu_row_waves(n), nq), dtype=torch.float64, device=dev)
    scratch = torch.empty((max(tab.slots, 1), nq), dtype=torch.float64, device=dev)
    lib.sp_mu_sums(*csr_ptrs(sd), t.indptr.data_ptr(), t.data.data_ptr(), tab.row.data_ptr(),
                   tab.start.data_ptr(), tab.dst.data_ptr(), tab.nseg, tab.seg,
                   tab.long_row.data_ptr(), tab.long_ptr.data_ptr(), tab.nlong, n, d,
                   q.data_ptr(), nq, arithmetic_grid_step(exps), nat.ptr(mean), nat.ptr(base),
                   rowmax.data_ptr(), colsum.data_ptr(), part.data_ptr(), scratch.data_ptr(),
                   nat.stream_handle(dev))
    return rowmax, colsum


def sp_mu_power_sums_torch(sd, exponents, mean=None):
    """The dense law on densified row chunks: the fp64 branch of
    ``ops/linalg.mu_power_sums_local`` chunk by chunk (no use of the
    stored-entry identity of the kernel, which it is the reference for)."""
    from .linalg import mu_power_sums_local
    n, d = sd.shape
    nq = len(exponents)
    rowmax = torch.full((nq,), -float("inf"), dtype=torch.float64, device=sd.device)
    colsum = torch.zeros((nq, d), dtype=torch.float64, device=sd.device)
    for a, b in chunks(n, TWIN_CHUNK):
        rm, cs = mu_power_sums_local(sd.dense_rows(a, b), list(exponents), mean=mean)
        rowmax = torch.maximum(rowmax, rm)
        colsum += cs
    return rowmax, colsum
