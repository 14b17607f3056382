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

The second half (``csrc/spminibatch.hip``) serves mini-batch k-means: the
same E-step and sums over a list of row ids drawn with replacement, a fused
centre update and a row densify / assign op, with :class:`MiniBatchState`
holding the device state of a fit.
"""

import torch

from . import _native as nat
from . import kmeans as K
from ._csr import (TWIN_CHUNK, chunks, csr_ptrs, native_ok, row_list, sp_row_norms,  # noqa: F401
                   sp_row_norms_torch)

MAX_K = 16384          # LDS row of k doubles: 128 KiB at one wave per workgroup
_PARTS = 8192          # per-wave inertia partials of the persistent grid


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


# ---------------------------------------------------------------- E-step
def _operand(sd, C, operand, xn):
    """(CT, cn, xn) of a native E-step-family launch: the caller's
    ``operand`` or ``center_operand(C)``, checked against the matrix.
    ``xn=None`` (the gram mode does not use the norms) stands for a cached
    zero vector."""
    k = C.shape[0]
    check_k(k)
    CT, cn = operand if operand is not None else center_operand(C)
    if xn is None:
        xn = getattr(sd, "_zero_norms", None)
        if xn is None:
            xn = sd._zero_norms = torch.zeros(sd.shape[0], dtype=torch.float64, device=sd.device)
    assert CT.dtype == torch.float64 and CT.is_contiguous() and CT.shape[0] == sd.shape[1]
    assert cn.dtype == torch.float64 and cn.numel() >= k
    assert xn.dtype == torch.float64 and xn.numel() >= sd.shape[0]
    return CT, cn, xn


def _launch(sd, CT, cn, xn, r0, r1, k, mode, delta, key, row_offset, labels, mind, part, inertia,
            out, ldo):
    assert 0 <= r0 <= r1 <= sd.shape[0]
    k0, k1, s0, s1 = key.as_tuple() if key is not None else (0, 0, 0, 0)
    nat.native().sp_estep(*csr_ptrs(sd), CT.data_ptr(), cn.data_ptr(), xn.data_ptr(), int(r0),
                          int(r1), sd.shape[1], int(k), CT.shape[1], int(mode), float(delta), k0,
                          k1, s0, s1, int(row_offset), nat.ptr(labels), nat.ptr(mind),
                          nat.ptr(part), nat.ptr(inertia), nat.ptr(out), int(ldo),
                          nat.stream_handle(sd.device))


def _launch_rows(sd, C, s, e, xn, out, operand, mode, dtype):
    """The gram (mode 1, fp32) or sqdist (mode 2, fp64) block of rows [s, e)."""
    k = C.shape[0]
    CT, cn, xn = _operand(sd, C, operand, xn)
    if out is None:
        out = torch.empty((e - s, k), dtype=dtype, device=sd.device)
    assert out.dtype == dtype and out.stride(1) == 1 and out.shape[0] >= e - s \
        and out.shape[1] >= k
    _launch(sd, CT, cn, xn, s, e, k, mode, 0.0, None, 0, None, None, None, None, out,
            out.stride(0))
    return out[:e - s, :k]


def sp_estep(sd, C, delta, key, row_offset=0, xn=None, operand=None):
    """delta-band E-step of CSR rows against centres ``C`` [k, d]:
    (labels int32 on GPU / int64 on CPU, mind fp64 - the row minimum,
    inertia fp64 [1])."""
    n = sd.shape[0]
    if xn is None:
        xn = sp_row_norms(sd)
    if native_ok(sd):
        CT, cn, xn = _operand(sd, C, operand, xn)
        dev = sd.device
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        mind = torch.empty(n, dtype=torch.float64, device=dev)
        part = torch.zeros(_PARTS, dtype=torch.float64, device=dev)
        inertia = torch.zeros(1, dtype=torch.float64, device=dev)
        _launch(sd, CT, cn, xn, 0, n, C.shape[0], 0, delta, key, row_offset, labels, mind, part,
                inertia, None, 0)
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
    for s, e in chunks(n, chunk_rows):
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
    if native_ok(sd):
        return _launch_rows(sd, C, s, e, None, out, operand, 1, torch.float32)
    G = torch.empty((e - s, k), dtype=torch.float64, device=sd.device) if out is None else out
    Cd = C.double()
    for a, b in chunks(e - s, TWIN_CHUNK):
        G[a:b, :k] = (sd.dense_rows(s + a, s + b) @ Cd.T).to(G.dtype)
    return G[:e - s, :k]


def sp_sqdist(sd, C, rows=None, xn=None, out=None, operand=None):
    """Squared distances (fp64 [m, k], clamped at 0) of CSR rows to centres."""
    n = sd.shape[0]
    s, e, _ = (rows if rows is not None else slice(None)).indices(n)
    k = C.shape[0]
    if xn is None:
        xn = sp_row_norms(sd)
    if native_ok(sd):
        return _launch_rows(sd, C, s, e, xn, out, operand, 2, torch.float64)
    D = torch.empty((e - s, k), dtype=torch.float64, device=sd.device) if out is None else out
    Cd = C.double()
    cn = (Cd * Cd).sum(1)
    for a, b in chunks(e - s, TWIN_CHUNK):
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
    if native_ok(sd):
        n, d = sd.shape
        if ws is None:
            ws = SparseReduce(sd, k, weights)
        lab = labels if labels.dtype == torch.int32 else labels.to(torch.int32)
        w = None if weights is None else weights.to(torch.float64).contiguous()
        sums = torch.empty((k, d), dtype=torch.float64, device=sd.device)
        counts = torch.empty(k, dtype=torch.float64, device=sd.device)
        ws.q.zero_()
        nat.native().sp_mstep(*csr_ptrs(sd), lab.contiguous().data_ptr(), nat.ptr(w), n, d,
                              int(k), ws.xexp, ws.wexp, ws.q.data_ptr(), ws.q[k * d:].data_ptr(),
                              sums.data_ptr(), counts.data_ptr(), nat.stream_handle(sd.device))
        return sums, counts
    return sp_centroid_sums_torch(sd, labels, k, weights)


def sp_centroid_sums_torch(sd, labels, k, weights=None, chunk_rows=TWIN_CHUNK):
    n, d = sd.shape
    sums = torch.zeros((k, d), dtype=torch.float64, device=sd.device)
    counts = torch.zeros(k, dtype=torch.float64, device=sd.device)
    for s, e in chunks(n, chunk_rows):
        sm, ct = K.centroid_sums_torch(sd.dense_rows(s, e), labels[s:e], k,
                                       None if weights is None else weights[s:e],
                                       acc_dtype=torch.float64)
        sums += sm
        counts += ct
    return sums, counts


# ------------------------------------------------------------- row lists
# (csrc/spminibatch.hip): a mini-batch is a list of CSR row ids drawn with
# replacement; ``rows=None`` means the contiguous rows [0, n).
def sp_rows_dense_torch(sd, rows, out=None, dst=None):
    rows = row_list(sd, rows)
    m, d = rows.numel(), sd.d
    if out is None:
        out = torch.zeros((m, d), dtype=torch.float64, device=sd.device)
    pos = torch.arange(m, dtype=torch.int64, device=sd.device) if dst is None \
        else torch.as_tensor(dst, dtype=torch.int64).to(sd.device)
    if dst is not None:
        out[pos] = 0.0
    lo = sd.indptr[rows]
    cnt = sd.indptr[rows + 1] - lo
    total = int(cnt.sum())
    if total:
        start = torch.cumsum(cnt, 0) - cnt
        src = torch.arange(total, dtype=torch.int64, device=sd.device) \
            + torch.repeat_interleave(lo - start, cnt, output_size=total)
        flat = torch.repeat_interleave(pos, cnt, output_size=total) * out.stride(0) \
            + sd.indices[src].to(torch.int64)
        # canonical CSR: one stored value per (row, column)
        out.view(-1)[flat] = sd.data[src].to(torch.float64)
    return out


def sp_rows_dense(sd, rows, out=None, dst=None):
    """CSR rows ``rows`` (any order, repeats allowed) as dense fp64 rows:
    ``out[t] = X[rows[t]]``, or ``out[dst[t]] = X[rows[t]]`` (the reference's
    ``assign_rows_csr``) with distinct ``dst``.  ``out`` must be contiguous."""
    rows = row_list(sd, rows)
    m = rows.numel()
    if dst is not None:
        dst = row_list(sd, dst)
        assert out is not None and dst.numel() == m
    if out is not None:
        assert out.dtype == torch.float64 and out.is_contiguous() and out.shape[1] == sd.d
    if not native_ok(sd):
        return sp_rows_dense_torch(sd, rows, out, dst)
    if out is None:
        out = torch.empty((m, sd.d), dtype=torch.float64, device=sd.device)
    nat.native().sp_rows_dense(*csr_ptrs(sd), rows.data_ptr(), nat.ptr(dst), m, sd.shape[0],
                               out.shape[0], sd.d, out.data_ptr(), out.stride(0),
                               nat.stream_handle(sd.device))
    return out


def sp_list_estep_torch(sd, C, rows=None, weights=None, xn=None, chunk_rows=TWIN_CHUNK):
    n = sd.shape[0]
    rows = row_list(sd, rows)
    m = n if rows is None else rows.numel()
    Cd = C.double()
    k = Cd.shape[0]
    cn = (Cd * Cd).sum(1)
    if xn is None:
        xn = sp_row_norms_torch(sd)
    labels = torch.empty(m, dtype=torch.int64, device=sd.device)
    mind = torch.empty(m, dtype=torch.float64, device=sd.device)
    col = torch.arange(k, dtype=torch.int64, device=sd.device)
    for s, e in chunks(m, chunk_rows):
        if rows is None:
            Xc, xc = sd.dense_rows(s, e), xn[s:e]
        else:
            Xc, xc = sp_rows_dense_torch(sd, rows[s:e]), xn[rows[s:e]]
        D = K.distances_torch(Xc, Cd, xc.double(), cn)
        mn = D.min(1).values
        # the first index of the minimum, whatever min's own tie order
        labels[s:e] = torch.where(D == mn[:, None], col[None, :], k).min(1).values
        mind[s:e] = mn
    inertia = (mind if weights is None else mind * weights.double()).sum().reshape(1)
    return labels, mind, inertia


def sp_list_estep(sd, C, rows=None, weights=None, xn=None, operand=None, inertia=None):
    """Plain argmin E-step over a row list (``rows=None``: all rows):
    (labels[t] int32 on GPU / int64 on CPU, mind[t] fp64, inertia fp64 [1] =
    sum_t w_t mind[t]).  The lowest index wins exact ties."""
    if xn is None:
        xn = sp_row_norms(sd)
    if not native_ok(sd):
        return sp_list_estep_torch(sd, C, rows, weights, xn)
    n = sd.shape[0]
    rows = row_list(sd, rows)
    m = n if rows is None else rows.numel()
    CT, cn, xn = _operand(sd, C, operand, xn)
    dev = sd.device
    w = None if weights is None else weights.to(torch.float64).contiguous()
    assert w is None or w.numel() == m
    labels = torch.empty(m, dtype=torch.int32, device=dev)
    mind = torch.empty(m, dtype=torch.float64, device=dev)
    part = torch.empty(_PARTS, dtype=torch.float64, device=dev)
    if inertia is None:
        inertia = torch.empty(1, dtype=torch.float64, device=dev)
    nat.native().sp_list_estep(*csr_ptrs(sd), CT.data_ptr(), cn.data_ptr(), xn.data_ptr(),
                               nat.ptr(rows), 0, m, n, sd.d, C.shape[0], CT.shape[1], nat.ptr(w),
                               labels.data_ptr(), mind.data_ptr(), part.data_ptr(),
                               inertia.data_ptr(), nat.stream_handle(dev))
    return labels, mind, inertia


def sp_list_sums_torch(sd, rows, labels, k, weights=None, chunk_rows=TWIN_CHUNK):
    """(sums [k, d], wsum [k]) of the listed rows by ``index_add_`` in list order."""
    rows = row_list(sd, rows)
    m = sd.shape[0] if rows is None else rows.numel()
    sums = torch.zeros((k, sd.d), dtype=torch.float64, device=sd.device)
    wsum = torch.zeros(k, dtype=torch.float64, device=sd.device)
    lab = labels.to(torch.int64)
    for s, e in chunks(m, chunk_rows):
        Xc = sd.dense_rows(s, e) if rows is None else sp_rows_dense_torch(sd, rows[s:e])
        if weights is None:
            wc = torch.ones(e - s, dtype=torch.float64, device=sd.device)
        else:
            wc = weights[s:e].double()
            Xc = Xc * wc[:, None]
        sums.index_add_(0, lab[s:e], Xc)
        wsum.index_add_(0, lab[s:e], wc)
    return sums, wsum


def minibatch_update_torch(C, counts, sums, wsum):
    """(C', counts', squared shift): c' = (c n_c + sum) / (n_c + w_c) for the
    centres with w_c > 0, separate multiply, add and divide; the others pass
    through."""
    upd = wsum > 0
    new_counts = counts + wsum
    Cn = C.clone()
    Cn[upd] = (C[upd] * counts[upd, None] + sums[upd]) / new_counts[upd, None]
    return Cn, new_counts, ((Cn - C) ** 2).sum()


class MiniBatchState:
    """Device state of a sparse mini-batch fit: centres ``C`` [k, d], the
    transposed operand ``CT`` / ``cn`` (GPU), accumulated weights ``counts``
    and the int64 quanta of the scatter.  :meth:`step` enqueues E-step,
    scatter and fused update back to back and returns after one read of the
    packed record [weighted batch inertia, squared shift, min count]."""

    def __init__(self, device, C, counts, max_abs=0.0, max_w=None):
        dev = torch.device(device)
        self.device = dev
        self.native = dev.type == "cuda"
        self.C = torch.as_tensor(C).to(dev).to(torch.float64).contiguous().clone()
        self.counts = torch.as_tensor(counts).to(dev).to(torch.float64).contiguous().clone()
        self.k, self.d = self.C.shape
        self.max_abs = float(max_abs)
        self.max_w = None if max_w is None else float(max_w)
        if self.native:
            nat.native()
            check_k(self.k)
            check_mstep_memory(self.k, self.d, dev)
            k, d = self.k, self.d
            nft = (d + 63) // 64
            self.q = torch.zeros(k * d + k, dtype=torch.int64, device=dev)
            self._pcn = torch.empty((k, nft), dtype=torch.float64, device=dev)
            self._pshift = torch.empty((k, nft), dtype=torch.float64, device=dev)
            self._shift = torch.empty(k, dtype=torch.float64, device=dev)
            self.rec = torch.zeros(3, dtype=torch.float64, device=dev)
            self._host = torch.zeros(3, dtype=torch.float64).pin_memory()
            self.rebuild_operand()

    def rebuild_operand(self):
        if self.native:
            self.CT, self.cn = center_operand(self.C)

    def operand(self):
        return (self.CT, self.cn) if self.native else None

    def exps(self, m):
        mw = self.max_w
        xexp = K.fixed_point_exp(self.max_abs * (mw if mw is not None else 1.0), m)
        return xexp, (0 if mw is None else K.fixed_point_exp(mw, m))

    # the three stages; ``reassign`` (optional) runs between E-step and scatter
    def estep(self, sd, xn, rows, weights):
        if self.native:
            return sp_list_estep(sd, self.C, rows, weights, xn=xn, operand=self.operand(),
                                 inertia=self.rec[:1])
        return sp_list_estep_torch(sd, self.C, rows, weights, xn)

    def scatter(self, sd, rows, labels, weights):
        if not self.native:
            self._sums = sp_list_sums_torch(sd, rows, labels, self.k, weights)
            return
        rows = row_list(sd, rows)
        m = sd.shape[0] if rows is None else rows.numel()
        self._exps = self.exps(m)
        w = None if weights is None else weights.to(torch.float64).contiguous()
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == m
        assert (w is None or w.numel() == m) and sd.d == self.d
        k, d = self.k, self.d
        nat.native().sp_list_mstep(*csr_ptrs(sd), nat.ptr(rows), 0, labels.data_ptr(),
                                   nat.ptr(w), m, sd.shape[0], d, k, self._exps[0], self._exps[1],
                                   self.q.data_ptr(), self.q[k * d:].data_ptr(),
                                   nat.stream_handle(self.device))

    def update(self):
        """Consumes the scattered sums; returns the squared shift (a device
        scalar on the GPU, where it is also ``rec[1]``)."""
        if not self.native:
            sums, wsum = self._sums
            self.C, self.counts, shift = minibatch_update_torch(self.C, self.counts, sums, wsum)
            return shift
        k, d = self.k, self.d
        nat.native().mb_update(self.C.data_ptr(), self.CT.data_ptr(), self.cn.data_ptr(),
                               self.counts.data_ptr(), self.q.data_ptr(),
                               self.q[k * d:].data_ptr(), k, d, self.CT.shape[1], self._exps[0],
                               self._exps[1], self._pcn.data_ptr(), self._pshift.data_ptr(),
                               self._shift.data_ptr(), self.rec.data_ptr(),
                               nat.stream_handle(self.device))
        return self.rec[1]

    def read_record(self):
        """[weighted batch inertia, squared shift, min count] of the last
        step: one device-to-host copy into pinned memory, one wait."""
        self._host.copy_(self.rec, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._host.tolist()

    def advance(self, sd, xn, rows, weights, reassign=None):
        """One step without the read: (inertia [1], squared shift) on the
        device.  ``reassign(state)`` runs between E-step and scatter and
        returns whether it replaced centres."""
        labels, _, inertia = self.estep(sd, xn, rows, weights)
        reassigned = bool(reassign(self)) if reassign is not None else False
        self.scatter(sd, rows, labels, weights)
        shift = self.update()
        if reassigned:
            # reassignments are rare: the operand is simply rebuilt
            self.rebuild_operand()
        return inertia, shift

    def step(self, sd, xn, rows, weights, reassign=None):
        """[weighted batch inertia, squared shift, min count] as floats."""
        inertia, shift = self.advance(sd, xn, rows, weights, reassign)
        if self.native:
            return self.read_record()
        return [float(inertia), float(shift), float(self.counts.min())]
