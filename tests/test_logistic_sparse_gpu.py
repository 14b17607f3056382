"""``LogisticRegression`` on sparse rows with ``device="cuda"``: the kernels of
``csrc/splogit.hip`` against the numpy yardsticks and the fp64 torch twins,
and the estimator against the host path (``device=None``) on the densified
matrix.

Tolerances are measured, not fixed (``_logistic_data.py``): 64 x the
yardstick's own largest deviation over 4 permuted copies of the problem.  No
kernel uses a floating-point atomic, so two runs are compared bit for bit."""
import json
import os
import pickle
import warnings
from unittest import mock

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _logistic_data as D
from sq_learn_amd.base import clone
from sq_learn_amd.linear_model import LogisticRegression
from sq_learn_amd.models._data import SparseData, as_sparse_data
from sq_learn_amd.ops import _native as nat
from sq_learn_amd.ops import sparse_logistic as S
from sq_learn_amd.ops._csr import csr_transpose

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings(), D.one_thread():
        warnings.simplefilter("ignore")
        yield


def test_bindings_match_their_table():
    """The bindings of ``_C.logistic`` against
    ``golden/native_formats_logistic.json``, as ``test_native_api_gpu.py`` checks
    those of ``_C`` against its table."""
    path = os.path.join(os.path.dirname(__file__), "golden", "native_formats_logistic.json")
    with open(path) as f:
        formats = json.load(f)
    m = nat.native().logistic
    names = {n for n in dir(m) if not n.startswith("_") and callable(getattr(m, n))}
    assert names == set(formats)
    for name, fmt in formats.items():
        head, sep, got = getattr(m, name).__doc__.rpartition("\n\nargs: ")
        assert sep and head and got == fmt, (name, got)
    with pytest.raises(TypeError):
        m.sp_logit_multi(0)
    with pytest.raises(TypeError):
        m.sp_matvec(0, 0)
    # the class counts of the tests sit on the kernel's pass boundary
    assert m.sp_logit_tile_classes() == S.TILE_CLASSES
    assert S.TILE_CLASSES in D.KS and S.TILE_CLASSES + 1 in D.KS


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("setting", D.SETTINGS)
@pytest.mark.parametrize("K", D.KS)
def test_multi_kernel(K, setting, weighted):
    loss, R = D.run_multi(DEV, K, setting, weighted)
    assert R.device.type == DEV
    tl, tR = D.run_multi("cpu", K, setting, weighted)
    (_, _, _), (f_loss, f_r, _) = D.multi_reference(K, setting, weighted)
    D.check(f"gpu multi K={K} {setting} R vs twin", R.cpu().numpy(), tR.numpy(), f_r)
    D.check(f"gpu multi K={K} {setting} loss vs twin", float(loss), float(tl), f_loss)
    loss2, R2 = D.run_multi(DEV, K, setting, weighted)
    assert torch.equal(loss2, loss) and torch.equal(R2, R)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("setting", D.SETTINGS)
def test_bin_kernel(setting, weighted):
    loss, r = D.run_bin(DEV, setting, weighted, seg=64)
    assert r.device.type == DEV
    loss2, r2 = D.run_bin(DEV, setting, weighted)
    assert torch.equal(loss2, loss) and torch.equal(r2, r)


@pytest.mark.parametrize("transposed", [False, True])
def test_matvec_kernel(transposed):
    """``seg=64`` cuts the transposed row of the column every row stores into
    five segments and the 300-entry row of X as well; the default keeps every
    row whole."""
    a = D.run_matvec(DEV, transposed, seg=64)
    b = D.run_matvec(DEV, transposed)
    assert torch.equal(a, D.run_matvec(DEV, transposed, seg=64))
    _, y, floor = D.matvec_reference(transposed)
    D.check(f"gpu matvec{'T' if transposed else ''} seg 64 vs default", a.cpu().numpy(),
            b.cpu().numpy(), floor)
    sd = as_sparse_data(D.corpus(), DEV)
    sd = csr_transpose(sd) if transposed else sd
    assert S.segments(sd, 64).nlong >= 1 and S.segments(sd).nlong == 0


def test_refusals():
    D.check_refusals(DEV)
    X = D.corpus()
    sd64 = SparseData(torch.as_tensor(X.indptr.astype(np.int64)).to(DEV),
                      torch.as_tensor(X.indices.astype(np.int32)).to(DEV),
                      torch.as_tensor(X.data.astype(np.float64)).to(DEV), X.shape)
    W, b = D.weights(3, "random")
    with pytest.raises(TypeError, match="fp32 values"):
        S.logit_multi(sd64, S.transposed_weights(W, DEV), b, D.labels(3), D.row_weights(False))
    with pytest.raises(TypeError, match="fp32 values"):
        S.logit_bin(sd64, W[0], 0.0, D.labels(2), D.row_weights(False))
    with pytest.raises(TypeError, match="fp32 values"):
        S.sp_matvec(sd64, np.zeros(D.D))


@pytest.mark.parametrize("case", sorted(D.FIT_CASES))
def test_estimator_follows_the_host_path(case):
    est = D.check_fit(DEV, case)
    assert isinstance(est.coef_, np.ndarray) and isinstance(est.intercept_, np.ndarray)


@pytest.mark.parametrize("K", [2, 3])
def test_strong_convexity_bound_against_scikit_learn(K):
    """Without intercept, penalty l2 and C = 1 the objective is 1-strongly
    convex: ``||a - b|| <= C (||g(a)|| + ||g(b)||)`` for any two points, g the
    numpy gradient."""
    from sklearn.linear_model import LogisticRegression as Ref
    X, y = D.corpus(), D.labels(K)
    a = LogisticRegression(fit_intercept=False, tol=1e-8, max_iter=2000, device=DEV).fit(X, y)
    b = Ref(fit_intercept=False, tol=1e-8, max_iter=2000).fit(X, y)
    ga, gb = D.l2_gradient(a.coef_, K), D.l2_gradient(b.coef_, K)
    dist = float(np.linalg.norm(a.coef_ - b.coef_))
    bound = float(np.linalg.norm(ga) + np.linalg.norm(gb))
    print(f"K={K}: distance {dist:.3e} bound {bound:.3e}")
    assert dist <= bound and bound < 1e-3


def _boom(*a, **k):
    raise AssertionError("the device path densified a sparse matrix")


def test_sparse_input_is_never_densified():
    X, y = D.corpus(), D.labels(3)
    kinds = [sp.csr_matrix, sp.csc_matrix, sp.coo_matrix]
    patches = [mock.patch.object(c, m, _boom) for c in kinds for m in ("toarray", "todense")]
    for p in patches:
        p.start()
    try:
        for A in (X, X.tocsc(), X.tocoo()):
            for yy, kw in ((y, {}), (y, dict(multi_class="ovr")), (D.labels(2), {}),
                           (y, dict(penalty="l1", solver="liblinear"))):
                est = LogisticRegression(max_iter=10, device=DEV, **kw).fit(A, yy)
                assert est.decision_function(A).shape[0] == D.N
                assert est.predict_proba(A).shape == (D.N, len(est.classes_))
                assert 0.0 <= est.score(A, yy) <= 1.0
    finally:
        for p in patches:
            p.stop()


def test_pickle_clone_and_mismatch_message():
    X, y = D.corpus(), D.labels(3)
    a = LogisticRegression(max_iter=15, device=DEV).fit(X, y)
    b = pickle.loads(pickle.dumps(a))
    c = clone(a)
    assert b.device == DEV and c.device == DEV and not hasattr(c, "coef_")
    np.testing.assert_array_equal(b.decision_function(X), a.decision_function(X))
    np.testing.assert_array_equal(c.fit(X, y).coef_, a.coef_)
    with pytest.raises(ValueError, match=f"X has 10 features per sample; expecting {D.D}"):
        a.decision_function(X[:, :10])
