"""CSR sparse k-means / q-means ops (sparse half).

Reference: ``cluster/_k_means_lloyd.pyx`` ``lloyd_iter_chunked_sparse`` and
the sparse branches of ``cluster/_dmeans.py`` (which fall back to the
classical iteration; here the delta-band and IPE label rules run on CSR).

Device path: ``csrc/spkmeans.hip`` - one wave per CSR row, lanes across
centroids, every nonzero one contiguous row gather of the transposed fp64
centre matrix; cluster sums by 64-bit fixed-point integer atomics (order
independent, bit-reproducible).  A GPU input always takes the native path
and raises when the extension is missing.  The torch twins (CPU) work in
fp64 over row chunks: a chunk of at most a few thousand rows is densified,
then ``ops.kmeans.distances_torch`` / ``band_select_torch`` /
``centroid_sums_torch`` do the work with the same Philox draws.
"""

import torch

from . import _native as nat
from . import kmeans as K

MAX_K = 16384          # LDS row of k doubles: 128 KiB at one wave per workgroup
TWIN_CHUNK = 2048      # rows densified at a time by the torch twins
_PARTS = 8192          # per-wave inertia partials of the persistent grid


def _native_ok(sd):
    if not nat.use_native(sd.data):
        return False
    if sd.data.dtype != torch.float32 or sd.indices.dtype != torch.int32 \
            or sd.indptr.dtype != torch.int64:
        raise TypeError("native sparse ops take fp32 values, int32 indices and int64 indptr")
    nat.native()   # raises when the HIP layer is unavailable: no silent fallback
    return True


def check_k(k):
    if k > MAX_K:
        raise ValueError(f"sparse E-step supports at most {MAX_K} clusters on the GPU, got {k}")


def center_operand(C):
    """(CT [d, k_pad] fp64 zero padded, cn [k] fp64) of centres ``C`` [k, d]."""
    k, d = C.shape
    k_pad = K.pad_clusters(k)
    Cd = C.double()
    CT = torch.zeros((d, k_pad), dtype=torch.float64, device=C.device)
    CT[:, :k] = Cd.T
    return CT, (Cd * Cd).sum(1).contiguous()


def _chunks(n, step):
    for s in range(0, n, step):
        yield s, min(n, s + step)


# ------------------------------------------------------------- row norms
def sp_row_norms(sd):
    """Squared row norms (fp64, n)."""
    n = sd.shape[0]
    if _native_ok(sd):
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


# ---------------------------------------------------------------- E-step
def _launch(sd, CT, cn, xn, r0, r1, k, mode, delta, key, row_offset, labels, mind, part, inertia,
            out, ldo):
    assert CT.dtype == torch.float64 and CT.is_contiguous() and CT.shape[0] == sd.shape[1]
    assert cn.dtype == torch.float64 and cn.numel() >= k and xn.dtype == torch.float64
    assert 0 <= r0 <= r1 <= sd.shape[0] and xn.numel() >= sd.shape[0]
    k0, k1, s0, s1 = key.as_tuple() if key is not None else (0, 0, 0, 0)
    nat.native().sp_estep(sd.indptr.data_ptr(), sd.indices.data_ptr(), sd.data.data_ptr(),
                          CT.data_ptr(), cn.data_ptr(), xn.data_ptr(), int(r0), int(r1),
                          sd.shape[1], int(k), CT.shape[1], int(mode), float(delta), k0, k1, s0,
                          s1, int(row_offset), nat.ptr(labels), nat.ptr(mind), nat.ptr(part),
                          nat.ptr(inertia), nat.ptr(out), int(ldo), nat.stream_handle(sd.device))


def sp_estep(sd, C, delta, key, row_offset=0, xn=None, operand=None):
    """delta-band E-step of CSR rows against centres ``C`` [k, d]:
    (labels int32 on GPU / int64 on CPU, mind fp64 - the row minimum,
    inertia fp64 [1])."""
    n = sd.shape[0]
    k = C.shape[0]
    if xn is None:
        xn = sp_row_norms(sd)
    if _native_ok(sd):
        check_k(k)
        CT, cn = operand if operand is not None else center_operand(C)
        dev = sd.device
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        mind = torch.empty(n, dtype=torch.float64, device=dev)
        part = torch.zeros(_PARTS, dtype=torch.float64, device=dev)
        inertia = torch.zeros(1, dtype=torch.float64, device=dev)
        _launch(sd, CT, cn, xn, 0, n, k, 0, delta, key, row_offset, labels, mind, part, inertia,
                None, 0)
        return labels, mind, inertia
    return sp_estep_torch(sd, C, delta, key, row_offset, xn=xn)


def sp_estep_torch(sd, C, delta, key, row_offset=0, xn=None, chunk_rows=TWIN_CHUNK):
    n = sd.shape[0]
    Cd = C.double()
    cn = (Cd * Cd).sum(1)
    k_pad = K.pad_clusters(C.shape[0])
    if xn is None:
        xn = sp_row_norms_torch(sd)
    labels = torch.empty(n, dtype=torch.int64, device=sd.device)
    mind = torch.empty(n, dtype=torch.float64, device=sd.device)
    for s, e in _chunks(n, chunk_rows):
        D = K.distances_torch(sd.dense_rows(s, e), Cd, xn[s:e].double(), cn)
        g = torch.arange(s, e, dtype=torch.int64, device=sd.device) + row_offset
        labels[s:e], mind[s:e] = K.band_select_torch(D, g, delta, key, k_pad)
    return labels, mind, mind.sum().reshape(1)


def sp_gram(sd, C, rows=None, out=None, operand=None):
    """Inner products of the CSR rows ``rows`` (a slice) with the centres:
    fp32 [m, k] on the GPU (the operand of ``ipe_estep_native``), fp64 on CPU."""
    n = sd.shape[0]
    s, e, _ = (rows if rows is not None else slice(None)).indices(n)
    k = C.shape[0]
    if _native_ok(sd):
        check_k(k)
        CT, cn = operand if operand is not None else center_operand(C)
        if out is None:
            out = torch.empty((e - s, k), dtype=torch.float32, device=sd.device)
        assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] >= e - s \
            and out.shape[1] >= k
        _launch_rows(sd, CT, cn, None, s, e, k, 1, out)
        return out[:e - s, :k]
    G = torch.empty((e - s, k), dtype=torch.float64, device=sd.device) if out is None else out
    Cd = C.double()
    for a, b in _chunks(e - s, TWIN_CHUNK):
        G[a:b, :k] = (sd.dense_rows(s + a, s + b) @ Cd.T).to(G.dtype)
    return G[:e - s, :k]


def _launch_rows(sd, CT, cn, xn, s, e, k, mode, out):
    if xn is None:
        # the gram mode does not use the norms
        xn = getattr(sd, "_zero_norms", None)
        if xn is None:
            xn = sd._zero_norms = torch.zeros(sd.shape[0], dtype=torch.float64, device=sd.device)
    _launch(sd, CT, cn, xn, s, e, k, mode, 0.0, None, 0, None, None, None, None, out,
            out.stride(0))


def sp_sqdist(sd, C, rows=None, xn=None, out=None, operand=None):
    """Squared distances (fp64 [m, k], clamped at 0) of CSR rows to centres."""
    n = sd.shape[0]
    s, e, _ = (rows if rows is not None else slice(None)).indices(n)
    k = C.shape[0]
    if xn is None:
        xn = sp_row_norms(sd)
    if _native_ok(sd):
        check_k(k)
        CT, cn = operand if operand is not None else center_operand(C)
        if out is None:
            out = torch.empty((e - s, k), dtype=torch.float64, device=sd.device)
        assert out.dtype == torch.float64 and out.stride(1) == 1 and out.shape[0] >= e - s \
            and out.shape[1] >= k
        _launch_rows(sd, CT, cn, xn, s, e, k, 2, out)
        return out[:e - s, :k]
    D = torch.empty((e - s, k), dtype=torch.float64, device=sd.device) if out is None else out
    Cd = C.double()
    cn = (Cd * Cd).sum(1)
    for a, b in _chunks(e - s, TWIN_CHUNK):
        D[a:b, :k] = K.distances_torch(sd.dense_rows(s + a, s + b), Cd,
                                       xn[s + a:s + b].double(), cn)
    return D[:e - s, :k]


# ---------------------------------------------------------------- M-step
def mstep_bytes(k, d):
    """Device bytes of a sparse fit's dense k x d state: the int64 quanta,
    the centres and the transposed operand."""
    return 3 * int(k) * int(d) * 8


def check_mstep_memory(k, d, device):
    device = torch.device(device)
    if device.type != "cuda":
        return
    free = torch.cuda.mem_get_info(device)[0]
    if mstep_bytes(k, d) > free:
        raise ValueError(f"sparse k-means with k={k}, d={d} needs {mstep_bytes(k, d)} bytes of "
                         f"device memory for its dense k x d state; {free} are free")


class SparseReduce:
    """Fixed-point exponents and the int64 quanta buffers of ``sp_centroid_sums``."""

    def __init__(self, sd, k, weights=None):
        check_mstep_memory(k, sd.shape[1], sd.device)
        mx = float(sd.data.abs().max()) if sd.nnz else 0.0
        mw = None if weights is None else float(weights.abs().max()) if weights.numel() else 0.0
        n = sd.shape[0]
        self.xexp = K.fixed_point_exp(mx * (mw if mw is not None else 1.0), n)
        self.wexp = 0 if mw is None else K.fixed_point_exp(mw, n)
        self.q = torch.zeros(k * sd.shape[1] + k, dtype=torch.int64, device=sd.device)


def sp_centroid_sums(sd, labels, k, weights=None, ws=None):
    """sums[l] = sum_{i: label_i = l} w_i x_i (fp64 [k, d]) and counts[l] = sum w_i."""
    if _native_ok(sd):
        n, d = sd.shape
        if ws is None:
            ws = SparseReduce(sd, k, weights)
        lab = labels if labels.dtype == torch.int32 else labels.to(torch.int32)
        w = None if weights is None else weights.to(torch.float64).contiguous()
        sums = torch.empty((k, d), dtype=torch.float64, device=sd.device)
        counts = torch.empty(k, dtype=torch.float64, device=sd.device)
        ws.q.zero_()
        nat.native().sp_mstep(sd.indptr.data_ptr(), sd.indices.data_ptr(), sd.data.data_ptr(),
                              lab.contiguous().data_ptr(), nat.ptr(w), n, d, int(k), ws.xexp,
                              ws.wexp, ws.q.data_ptr(), ws.q[k * d:].data_ptr(), sums.data_ptr(),
                              counts.data_ptr(), nat.stream_handle(sd.device))
        return sums, counts
    return sp_centroid_sums_torch(sd, labels, k, weights)


def sp_centroid_sums_torch(sd, labels, k, weights=None, chunk_rows=TWIN_CHUNK):
    n, d = sd.shape
    sums = torch.zeros((k, d), dtype=torch.float64, device=sd.device)
    counts = torch.zeros(k, dtype=torch.float64, device=sd.device)
    for s, e in _chunks(n, chunk_rows):
        sm, ct = K.centroid_sums_torch(sd.dense_rows(s, e), labels[s:e], k,
                                       None if weights is None else weights[s:e],
                                       acc_dtype=torch.float64)
        sums += sm
        counts += ct
    return sums, counts
