"""What every CSR sparse op module (``sparse_kmeans``, ``sparse_linalg``,
``sparse_knn``, ``sparse_radius``, ``sparse_lda``, ``sparse_nmf``) needs: the native-path
test, the chunk iterator of the torch twins, the pointer triple of a launch, the row-list
normaliser, the squared row norms and the cached transpose.  The six modules
import from here and not from each other (``sparse_radius`` also uses the
k-NN operand object and epilogue; ``sparse_kernel`` builds on that operand
object and on the products of ``sparse_linalg``).
"""

import torch

from . import _native as nat

TWIN_CHUNK = 2048      # rows densified at a time by the torch twins


def native_ok(sd):
    if not nat.use_native(sd.data):
        return False
    if sd.data.dtype != torch.float32 or sd.indices.dtype != torch.int32 \
            or sd.indptr.dtype != torch.int64:
        raise TypeError("native sparse ops take fp32 values, int32 indices and int64 indptr")
    nat.native()   # raises when the HIP layer is unavailable: no silent fallback
    return True


def chunks(n, step):
    for s in range(0, n, step):
        yield s, min(n, s + step)


def csr_ptrs(sd):
    """The (indptr, indices, data) device pointers every CSR launch starts with."""
    return sd.indptr.data_ptr(), sd.indices.data_ptr(), sd.data.data_ptr()


def row_list(sd, rows):
    """``rows`` as a contiguous int64 tensor on the device of ``sd``
    (``None``, the contiguous rows [0, n), stays ``None``)."""
    if rows is None:
        return None
    rows = torch.as_tensor(rows, dtype=torch.int64)
    if rows.device != sd.device:
        rows = rows.to(sd.device)          # the batch ids go up in one copy
    return rows.contiguous()


# ------------------------------------------------------------- row norms
def sp_row_norms(sd):
    """Squared row norms (fp64, n)."""
    n = sd.shape[0]
    if native_ok(sd):
        xn = torch.empty(n, dtype=torch.float64, device=sd.device)
        nat.native().sp_row_norms(sd.indptr.data_ptr(), sd.data.data_ptr(), xn.data_ptr(), n,
                                  nat.stream_handle(sd.device))
        return xn
    return sp_row_norms_torch(sd)


def sp_row_norms_torch(sd):
    xn = torch.zeros(sd.shape[0], dtype=torch.float64, device=sd.device)
    if sd.nnz:
        v = sd.data.double()
        xn.index_add_(0, sd.row_ids(), v * v)
    return xn


# --------------------------------------------------------------- transpose
def csr_transpose(sd):
    """X^T as canonical CSR on the device of ``sd`` (cached on ``sd``): a
    stable sort of the column indices keeps the row order inside every
    column, so the transposed rows come out sorted."""
    if sd._transpose is not None:
        return sd._transpose
    from ..models._data import SparseData
    n, d = sd.shape
    if n >= 2 ** 31:
        raise ValueError("csr_transpose supports fewer than 2^31 rows (int32 indices)")
    cols = sd.indices.to(torch.int64)
    order = torch.sort(cols, stable=True).indices
    rows = sd.row_ids()[order].to(torch.int32)
    indptr = torch.zeros(d + 1, dtype=torch.int64, device=sd.device)
    if sd.nnz:
        indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=d), 0)
    sd._transpose = SparseData(indptr, rows, sd.data[order].contiguous(), (d, n))
    return sd._transpose
