"""Device path of ``NMF`` (``device="cpu"`` / ``"cuda"``): the matrix goes to
the device once per call - a scipy sparse matrix as CSR, never densified, a
dense one as fp64 - and the solvers run there.  Coordinate descent is
``ops.sparse_nmf.nmf_cd_sweep`` around the products ``X H^T`` / ``X^T W``
(``ops.sparse_linalg`` on CSR, torch GEMMs on dense input); the Frobenius
multiplicative updates are those products plus torch; the Kullback-Leibler
updates evaluate ``W H`` at the stored entries only
(``ops.sparse_nmf.nmf_kl_ratio``, on X for W and on the cached transpose for
H).  The divergences of a CSR matrix never form ``W H`` either: Frobenius is
``||X||^2 + tr(W^T W H H^T) - 2 tr((X H^T)^T W)``, Kullback-Leibler sums
``x log(x / wh)`` over the stored entries.

Initialisation and the ``shuffle`` permutations stay the estimator's numpy
draws in the host path's order, so a seeded fit follows the host fit to
rounding.  Nothing here outlives the call: the factors go back as numpy.
"""

import numpy as np
import scipy.sparse as sp
import torch

from ...ops import sparse_linalg as SL
from ...ops import sparse_nmf as S
from ...ops._csr import csr_transpose
from ...runtime.device import resolve_device
from ...utils.validation import check_random_state
from .._data import as_sparse_data

EPS64 = float(np.finfo(np.float64).eps)


def _floor_den(den):
    return torch.where(den == 0, S.EPSILON, den)


class DeviceNMF:
    """The device state of one estimator call on ``X``: a validated scipy CSR
    matrix or a dense fp64 array."""

    def __init__(self, est, X):
        self.est = est
        self.dev = resolve_device(est.device)
        self.sparse = sp.issparse(X)
        if self.sparse:
            self.sd = as_sparse_data(X, self.dev)
            v = self.sd.data.double()
            self.norm_sq = (v * v).sum()
            self.x_sum = v[v > S.EPSILON].sum()
        else:
            self.X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(self.dev)

    def check(self, k, solver, beta):
        if solver == "cd":
            S.check_cd_k(k)
        elif beta == 1 and self.sparse:
            S.check_kl_k(k)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    # -------------------------------------------------------------- products
    def xw(self, B):
        """X B, B [d, k]."""
        return SL.sp_xw(self.sd, B) if self.sparse else self.X @ B

    def xtw(self, B):
        """X^T B, B [n, k]."""
        return SL.sp_xty(self.sd, B) if self.sparse else self.X.T @ B

    # ------------------------------------------------------------ divergence
    def divergence(self, W, Ht, beta):
        """``_beta_divergence(X, W, H, beta, square_root=True)`` as a 0-d
        tensor; ``Ht`` is H transposed, [d, k]."""
        if beta == 2:
            if self.sparse:
                cross = (self.xw(Ht) * W).sum()
                res = (self.norm_sq + ((W.T @ W) * (Ht.T @ Ht)).sum() - 2.0 * cross) / 2.0
                res = res.clamp(min=0.0)
            else:
                res = ((self.X - W @ Ht.T) ** 2).sum() / 2.0
            return torch.sqrt(res * 2)
        if self.sparse:
            first = S.nmf_kl_ratio(self.sd, W, Ht, want_num=False, want_div=True)[1].sum()
            x_sum = self.x_sum
        else:
            WH = W @ Ht.T
            big = self.X > S.EPSILON
            x, wh = self.X[big], WH[big]
            wh = torch.where(wh == 0, S.EPSILON, wh)
            first = x @ torch.log(x / wh)
            x_sum = x.sum()
        res = first + W.sum(0) @ Ht.sum(0) - x_sum
        return torch.sqrt(2 * res)

    # ---------------------------------------------------- coordinate descent
    def _cd_sweep(self, on_rows, A, B, l1, l2, shuffle, rng, fixed=None):
        """A sweep over A with B fixed: (W, H^T) on the rows of X, (H^T, W) on
        its columns.  ``fixed``: a dict that keeps the Gram matrix and the
        product with X between sweeps when B never changes (``update_H`` off)."""
        k = B.shape[1]
        if fixed:
            G, XB = fixed["G"], fixed["XB"]
        else:
            G = B.T @ B
            XB = self.xw(B) if on_rows else self.xtw(B)
            if l2 != 0.0:
                G.diagonal().add_(l2)
            if l1 != 0.0:
                XB = XB - l1
            if fixed is not None:
                fixed.update(G=G, XB=XB)
        perm = rng.permutation(k) if shuffle else np.arange(k)
        return S.nmf_cd_sweep(A, G, XB, torch.from_numpy(np.ascontiguousarray(perm, np.int64)))

    def fit_cd(self, W, H, tol, max_iter, l1W, l1H, l2W, l2H, update_H, shuffle, random_state):
        W = self.up(W)
        Ht = self.up(H.T)
        rng = check_random_state(random_state)
        fixed = None if update_H else {}
        for n_iter in range(1, max_iter + 1):
            v = self._cd_sweep(True, W, Ht, l1W, l2W, shuffle, rng, fixed)
            if update_H:
                v = v + self._cd_sweep(False, Ht, W, l1H, l2H, shuffle, rng)
            v = float(v)          # the one host read of the iteration
            if n_iter == 1:
                v0 = v
            if v0 == 0 or v / v0 <= tol:
                break
        return W, Ht, n_iter

    # ------------------------------------------------ multiplicative updates
    def _kl_num(self, on_rows, W, Ht):
        if self.sparse:
            if on_rows:
                return S.nmf_kl_ratio(self.sd, W, Ht)[0]
            return S.nmf_kl_ratio(csr_transpose(self.sd), Ht, W)[0]
        WH = W @ Ht.T
        R = self.X / torch.where(WH == 0, S.EPSILON, WH)
        return R @ Ht if on_rows else R.T @ W

    def _mu_w(self, W, Ht, beta, l1, l2, fixed=None):
        """The update factor of W.  ``fixed``: a dict that keeps what depends
        on H alone (``X H^T`` and ``H H^T``, or the row sums of H) between
        iterations when H never changes (``update_H`` off), as the host path
        does."""
        if not fixed:
            keep = dict(XHt=self.xw(Ht), HHt=Ht.T @ Ht) if beta == 2 \
                else dict(H_sum=Ht.sum(0)[None, :])
            if fixed is None:
                fixed = keep
            else:
                fixed.update(keep)
        if beta == 2:
            num = fixed["XHt"]
            den = W @ fixed["HHt"]
        else:
            num = self._kl_num(True, W, Ht)
            den = fixed["H_sum"]
        if l1 > 0:
            den = den + l1
        if l2 > 0:
            den = den + l2 * W
        return num / _floor_den(den)

    def _mu_h(self, W, Ht, beta, l1, l2):
        """The update factor of H, transposed: [d, k]."""
        if beta == 2:
            num = self.xtw(W)
            den = Ht @ (W.T @ W)
        else:
            num = self._kl_num(False, W, Ht)
            ws = W.sum(0)
            den = torch.where(ws == 0, 1.0, ws)[None, :]
        if l1 > 0:
            den = den + l1
        if l2 > 0:
            den = den + l2 * Ht
        return num / _floor_den(den)

    def fit_mu(self, W, H, beta, max_iter, tol, l1W, l1H, l2W, l2H, update_H):
        W = self.up(W)
        Ht = self.up(H.T)
        err0 = prev = float(self.divergence(W, Ht, beta))
        fixed = None if update_H else {}
        for n_iter in range(1, max_iter + 1):
            W *= self._mu_w(W, Ht, beta, l1W, l2W, fixed)
            if update_H:
                Ht *= self._mu_h(W, Ht, beta, l1H, l2H)
                if beta <= 1:
                    Ht[Ht < EPS64] = 0.0
            if tol > 0 and n_iter % 10 == 0:
                err = float(self.divergence(W, Ht, beta))
                if (prev - err) / err0 < tol:
                    break
                prev = err
        return W, Ht, n_iter

    # ------------------------------------------------------------------ fit
    def fit(self, W, H, beta, update_H):
        """The solver on the initial factors (numpy); returns the fitted
        ``(W, H, n_iter)`` as numpy."""
        est = self.est
        l1W, l1H, l2W, l2H = est._regs()
        if est.solver == "cd":
            Wd, Ht, n_iter = self.fit_cd(W, H, est.tol, est.max_iter, l1W, l1H, l2W, l2H,
                                         update_H, est.shuffle, est.random_state)
        else:
            Wd, Ht, n_iter = self.fit_mu(W, H, beta, est.max_iter, est.tol, l1W, l1H, l2W, l2H,
                                         update_H)
        self._fitted = (Wd, Ht, beta)
        return Wd.cpu().numpy(), np.ascontiguousarray(Ht.T.cpu().numpy()), n_iter

    def reconstruction_err(self):
        """The square-rooted divergence of the factors :meth:`fit` returned."""
        return float(self.divergence(*self._fitted))
