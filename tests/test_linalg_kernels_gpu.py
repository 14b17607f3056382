"""``csrc/linalg.hip`` (``col_moments``, ``row_norms``, ``mu_sums``) against
the fp64 references of ``_dense_ref`` on the dtype-rounded input.

Bounds (u32 = 2^-24, u64 = 2^-53, gamma_k = k u / (1 - k u)):

* col_moments accumulates exact fp64 terms (the square of an fp32 / bf16
  value is exact in fp64, the fma rounds once): at most n - 1 roundings per
  column against a correctly rounded reference, so |got - ref| <=
  n u64 sum|x| (and ... sum x^2); integer data is exact.
* row_norms: d rounded fp32 products and at most d - 1 effective additions
  in any order: |got - ref| <= gamma_{d+1} sum x^2; integer data with
  |x| <= 16 keeps every partial sum an integer below 2^24 and is exact.
* mu_sums: the project's own rtol = 2e-4 (``test_mu_power_sums_shapes``) is
  the assertion.  The inputs make x - mean exact, so the error is log2, exp2,
  the ARITH products and the fp32 summation only.  Measured maximum relative
  error over every case of this file on an MI355X (row maxima / column
  sums):

      dtype  ARITH   row maxima   column sums
      fp32   off     2.74e-07     9.30e-07
      fp32   on      3.94e-07     9.14e-07
      bf16   off     2.74e-07     9.30e-07
      bf16   on      3.94e-07     9.14e-07

  (bf16 equals fp32 because these inputs are exact in bf16 and the kernel
  computes in fp32 either way.)  This is the ~1e-6 the kernel comment
  expects for the products: a few fp32 roundings of log2 / exp2 per term
  and the fp32 summation, 200 times below the asserted 2e-4.
"""
import numpy as np
import pytest
import torch

import _dense_ref as R
from sq_learn_amd.ops import linalg as L

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _dev(X, dtype, cuda):
    """(device tensor of ``dtype``, fp64 numpy copy of the rounded values)."""
    t = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dtype)
    return t.to(cuda), t.double().numpy()


# ------------------------------------------------------------- col_moments
def _moments(X):
    s, ss = L.col_moments_local(X)
    assert s.dtype == ss.dtype == torch.float64 and s.shape == ss.shape == (X.shape[1],)
    return s.cpu().numpy(), ss.cpu().numpy()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 257, 600])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_col_moments(cuda, dtype, n):
    rng = np.random.RandomState(n)
    for d in (1, 63, 256, 257, 300):
        # integers: exact
        Xg, Xr = _dev(rng.randint(-64, 65, size=(n, d)), dtype, cuda)
        rs, rss = R.col_moments_ref(Xr)
        s, ss = _moments(Xg)
        np.testing.assert_array_equal(s, rs)
        np.testing.assert_array_equal(ss, rss)
        # random: bounded
        Xg, Xr = _dev(rng.standard_normal((n, d)) * 3, dtype, cuda)
        rs, rss = R.col_moments_ref(Xr)
        bs = n * R.U64 * np.abs(Xr).sum(0)
        bss = n * R.U64 * (Xr * Xr).sum(0)
        s, ss = _moments(Xg)
        assert np.all(np.abs(s - rs) <= bs) and np.all(np.abs(ss - rss) <= bss)
        # deterministic
        s2, ss2 = L.col_moments_local(Xg)
        s3, ss3 = L.col_moments_local(Xg)
        assert torch.equal(s2, s3) and torch.equal(ss2, ss3)
        # a column slice of a wider matrix (ldx > d): any over-read meets 1e30
        W = torch.full((n, d + 5), 1e30, dtype=dtype, device=cuda)
        W[:, 2:2 + d] = Xg
        s, ss = _moments(W[:, 2:2 + d])
        assert np.all(np.abs(s - rs) <= bs) and np.all(np.abs(ss - rss) <= bss)
        # a non-unit column stride
        W = torch.full((n, 2 * d), 1e30, dtype=dtype, device=cuda)
        W[:, ::2] = Xg
        V = W[:, ::2]
        assert V.stride(1) == 2
        s, ss = _moments(V)
        assert np.all(np.abs(s - rs) <= bs) and np.all(np.abs(ss - rss) <= bss)


# --------------------------------------------------------------- row_norms
ROW_D = [1, 3, 4, 8, 12, 200, 260, 520, 1027]


@pytest.mark.parametrize("n", [1, 5, 1001])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_norms(cuda, dtype, n):
    rng = np.random.RandomState(n)
    esz = 4 if dtype == torch.float32 else 2
    for d in ROW_D:
        Xg, Xr = _dev(rng.randint(-16, 17, size=(n, d)), dtype, cuda)
        ref_i = torch.from_numpy(R.row_norms_ref(Xr)).float()
        got = L.row_norms_sq(Xg)
        assert got.dtype == torch.float32 and got.shape == (n,)
        assert torch.equal(got.cpu(), ref_i)
        Yg, Yr = _dev(rng.standard_normal((n, d)) * 3, dtype, cuda)
        ref = R.row_norms_ref(Yr)
        bound = R.gamma(d + 1) * ref
        got = L.row_norms_sq(Yg).cpu().double().numpy()
        assert np.all(np.abs(got - ref) <= bound)
        # out=: written in place, canary rows behind it untouched
        buf = torch.full((n + 2,), -7.0, dtype=torch.float32, device=cuda)
        res = L.row_norms_sq(Yg, out=buf[:n])
        assert res.data_ptr() == buf.data_ptr()
        assert np.array_equal(buf[:n].cpu().double().numpy(), got) and bool((buf[n:] == -7.0).all())
        if d * esz % 16 == 0:
            # a contiguous view one element into a buffer: the base is not
            # 16-byte aligned although every row length is
            flat = torch.zeros(n * d + 9, dtype=dtype, device=cuda)
            for src, want in ((Xg, None), (Yg, ref)):
                flat[1:1 + n * d] = src.reshape(-1)
                V = flat[1:1 + n * d].view(n, d)
                assert V.is_contiguous() and V.data_ptr() % 16 != 0
                res = L.row_norms_sq(V).cpu()
                if want is None:
                    assert torch.equal(res, ref_i)       # integers: equal to the aligned copy
                else:
                    assert np.all(np.abs(res.double().numpy() - want) <= bound)


# ----------------------------------------------------------------- mu_sums
MU_RTOL = 2e-4
MU_D = [5, 8, 9, 16, 24, 40, 100, 129, 200, 257, 512, 513, 640, 1030]
MU_N = [1, 3, 257, 700]


def _rel_err(got, ref):
    """max |got - ref| / |ref|; where ref is 0 the result must be 0 too."""
    zero = ref == 0
    assert np.all(got[zero] == 0)
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / np.abs(ref[~zero])).max())


def mu_case(cuda, dtype, n, d, errors=None):
    """Every exponent set, mean on / off and planted row of one (n, d).
    ``errors``: dict (arith, "rowmax" | "colsum") -> running maximum."""
    a0, _ = R.mu_data(n, d, 0, False)
    for name, exps in R.MU_EXP_SETS.items():
        arith = name.startswith("arith")
        rows0, cols = R.mu_rowsums_ref(a0, exps)
        for rstar in R.mu_rstars(n):
            rows = rows0.copy()
            rows[:, [0, rstar]] = rows[:, [rstar, 0]]
            assert np.all(rows.argmax(1) == rstar)
            rmax = rows.max(1)
            for with_mean in (False, True):
                X, mean = R.mu_data(n, d, rstar, with_mean)
                Xg, Xr = _dev(X, dtype, cuda)
                assert np.array_equal(Xr, X)                      # exact in the dtype
                a = X if mean is None else X - mean[None, :]
                assert np.array_equal(np.delete(a, [0, rstar], 0), np.delete(a0, [0, rstar], 0))
                assert np.array_equal(a[rstar], a0[0]) and np.array_equal(a[0], a0[rstar])
                mg = None if mean is None else torch.from_numpy(mean).to(cuda)
                rm, cs = L.mu_power_sums_local(Xg, exps, mg)
                assert rm.shape == (len(exps),) and cs.shape == (len(exps), d)
                e_r = _rel_err(rm.cpu().numpy(), rmax)
                e_c = _rel_err(cs.cpu().numpy(), cols)
                if errors is not None:
                    for key, e in (((arith, "rowmax"), e_r), ((arith, "colsum"), e_c)):
                        errors[key] = max(errors.get(key, 0.0), e)
                assert e_r <= MU_RTOL, (name, n, d, rstar, with_mean, e_r)
                assert e_c <= MU_RTOL, (name, n, d, rstar, with_mean, e_c)
                if rstar == 0:
                    rm2, cs2 = L.mu_power_sums_local(Xg, exps, mg)
                    assert torch.equal(rm, rm2) and torch.equal(cs, cs2)


@pytest.mark.parametrize("d", MU_D)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mu_sums(cuda, dtype, d):
    errors = {}
    for n in MU_N:
        mu_case(cuda, dtype, n, d, errors)
    for (arith, what), e in sorted(errors.items()):
        print(f"MU_MAXERR {IDS[DTYPES.index(dtype)]} d={d} arith={int(arith)} {what} {e:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mu_sums_misaligned_slice(cuda, dtype):
    """W[:, 1:30] of a 32-column matrix: the row stride is a multiple of 8
    but the base is one element off a 16-byte boundary."""
    for n in (3, 257):
        X, mean = R.mu_data(n, 29, n - 1, True)
        W = torch.full((n, 32), 7.0, dtype=dtype, device=cuda)
        W[:, 1:30] = torch.from_numpy(X).to(dtype).to(cuda)
        V = W[:, 1:30]
        assert V.stride(0) == 32 and V.data_ptr() % 16 != 0
        mg = torch.from_numpy(mean).to(cuda)
        for exps in R.MU_EXP_SETS.values():
            rm, cs = L.mu_power_sums_local(V, exps, mg)
            rm_c, cs_c = L.mu_power_sums_local(V.contiguous(), exps, mg)
            assert torch.equal(rm, rm_c) and torch.equal(cs, cs_c)
            rmax, cols = R.mu_ref(X, exps, mean)
            assert _rel_err(rm.cpu().numpy(), rmax) <= MU_RTOL
            assert _rel_err(cs.cpu().numpy(), cols) <= MU_RTOL
