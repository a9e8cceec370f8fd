"""The numpy restatement of the device SVM (tests/svm_ref.py) pinned against scikit-learn / libsvm, and the host side of
mr_gan_amd.svm and of mr_svm(backend='hip') that runs without a GPU."""
import numpy as np
import pytest

from mr_gan_amd import synthetic_mreo
from tests import svm_ref as R


@pytest.mark.parametrize("d,trials,per,sep,C,gamma", [(37, 20, 24, 1.5, 1.0, 1.0 / 37), (16, 30, 40, 0.5, 1.0, 0.5),
                                                      (37, 20, 24, 1.5, 100.0, 1.0 / 37)])
def test_restatement_matches_libsvm_on_the_rounded_gram(d, trials, per, sep, C, gamma):
    """SVC(kernel='precomputed') reads the fp32-rounded Gram matrix and rounds its Q to float as well: both sides solve the same
    problem, so at tol = 1e-8 the one-vs-one decision values agree to 1e-7 (measured: <= 9.5e-9)"""
    from sklearn.svm import SVC
    xl, yl, cs, K = R.mreo_labeled(d, trials, per, sep, gamma)
    coef, rho, iters = R.solve_ovo(K, cs, C, 1e-8)
    svc = SVC(kernel='precomputed', C=C, tol=1e-8, decision_function_shape='ovo').fit(K.astype(np.float64), yl)
    dec = R.decisions(coef, rho, K, cs)
    want = svc.decision_function(K.astype(np.float64))
    print("max |dec - libsvm| = %.3g, iterations <= %d" % (np.abs(dec - want).max(), iters.max()))
    assert np.abs(dec - want).max() <= 1e-7
    assert (R.vote(dec, 6) == svc.predict(K.astype(np.float64))).all()
    assert np.abs(-rho - svc.intercept_).max() <= 1e-7
    for i, j in R.ovo_pairs(6):
        rows, y = R.pair_rows(cs, i, j)
        alpha = R.pair_alpha(coef, cs, i, j)
        assert (alpha >= 0).all() and (alpha <= C).all()
        assert R.kkt_gap(K[np.ix_(rows, rows)], y, alpha, C) < 1e-8 * (1 + 1e-6)
    if C == 1.0 and sep == 0.5:
        assert np.mean(np.abs(svc.dual_coef_[svc.dual_coef_ != 0]) >= C) > 0.2        # the bounded-heavy case is bounded-heavy


def test_class_sort_unsort_and_dual_coef_layout():
    """class_sort is a stable sort by class; unsort_coef brings [(K-1), n] coefficients back to the caller's row order, where
    they are SVC.dual_coef_ scattered to SVC.support_ (labels need not be 0..K-1 or sorted)"""
    from sklearn.svm import SVC
    from mr_gan_amd.svm import class_sort, unsort_coef
    xl, yl, _, _ = R.mreo_labeled(37, 20, 24, 1.5, 1.0 / 37)
    rs = np.random.RandomState(5)
    keep = rs.permutation(len(yl))[:100]                      # unequal classes, shuffled rows
    x, y = xl[keep], np.array([3, 7, 9, 11, 20, 21])[yl[keep]]
    classes, order, cs = class_sort(y)
    assert list(classes) == [3, 7, 9, 11, 20, 21] and cs[0] == 0 and cs[-1] == 100 and cs.dtype == np.int64
    assert (np.diff(cs) == np.bincount(yl[keep])).all()
    ys = y[order]
    assert (np.diff(ys) >= 0).all()
    for c in classes:                                         # stable: the caller's order inside a class
        assert (np.diff(order[ys == c]) > 0).all()
    K = R.rbf_gram(x, x, 1.0 / 37).astype(np.float32)
    coef_sorted, rho, _ = R.solve_ovo(K[np.ix_(order, order)], cs, 1.0, 1e-8)
    dense = unsort_coef(coef_sorted, order)
    assert (dense[:, order] == coef_sorted).all()
    svc = SVC(kernel='precomputed', C=1.0, tol=1e-8, decision_function_shape='ovo').fit(K.astype(np.float64), y)
    want = R.dense_from_svc(svc, len(y))
    assert ((dense != 0) == (want != 0)).all()                # the same support vectors in the same places
    assert np.abs(dense - want).max() <= 1e-7
    assert np.abs(-rho - svc.intercept_).max() <= 1e-7

    with pytest.raises(ValueError):
        class_sort(np.zeros((2, 2)))


def test_rbfsvm_checks_arguments_before_any_device_call():
    from mr_gan_amd import RBFSVM
    for kw in (dict(gamma='scale'), dict(gamma=0.0), dict(C=0.0), dict(tol=-1.0), dict(max_iter=0), dict(C=float('nan'))):
        with pytest.raises(ValueError):
            RBFSVM(**kw)
    clf = RBFSVM()
    assert (clf.C, clf.gamma, clf.tol, clf.max_iter) == (1.0, 'auto', 1e-3, 10_000_000)
    x = np.zeros((4, 3))
    with pytest.raises(ValueError, match="non-finite"):
        clf.fit(np.array([[0.0, np.inf, 0.0]] * 4), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="non-finite"):
        clf.fit(np.array([[0.0, np.nan, 0.0]] * 4), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="2 to 32 classes"):
        clf.fit(x, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="rows"):
        clf.fit(x, [0, 1, 1])
    with pytest.raises(ValueError, match="MRGAN_SVM_MAX_PAIR"):
        clf.fit(np.zeros((2049, 1)), [0] * 1025 + [1] * 1024)
    with pytest.raises(RuntimeError, match="fit"):
        clf.predict(x)


def test_backend_flag_and_hip_backend_calls_rbfsvm(monkeypatch, capsys):
    """--backend parses to sklearn (default) or hip and reaches fn only when it is not the default; mr_svm(backend='hip') fits
    and scores an RBFSVM(C=1, gamma='auto') on the prologue's labeled subset and returns 1 - score"""
    import mr_gan_amd.mr_svm as S
    rs = np.random.RandomState(0)

    def fake_dataset(modalities=0, leaveObjectOut=False, **kw):
        if leaveObjectOut:
            return {'m%d_o%d' % (m, o): {'x': rs.randn(4, 3).tolist(), 'y': [m] * 4} for m in range(6) for o in range(2)}
        return rs.randn(36, 3), np.arange(36) % 6
    seen = []
    S.main(['--tables', '4', '--backend', 'hip'], dataset_fn=fake_dataset, fn=lambda X, y, **kw: seen.append(kw.get('backend')) or 0.5)
    assert seen and set(seen) == {'hip'}
    seen.clear()
    S.main(['--tables', '4'], dataset_fn=fake_dataset, fn=lambda X, y, **kw: seen.append(kw.get('backend')) or 0.5)
    assert seen and set(seen) == {None}
    with pytest.raises(SystemExit):
        S.main(['--tables', '4', '--backend', 'cuda'], dataset_fn=fake_dataset)
    capsys.readouterr()
    with pytest.raises(ValueError, match="backend"):
        S.mr_svm(None, None, trainTestSets=[np.zeros((12, 2)), np.zeros((6, 2)), np.arange(12) % 6, np.arange(6)], backend='cuda')

    made = []

    class FakeSVM:
        def __init__(self, **kw):
            self.kw = kw
            made.append(self)

        def fit(self, X, y):
            self.fit_shapes = (np.asarray(X).shape, np.asarray(y).shape)
            return self

        def score(self, X, y):
            self.score_shapes = (np.asarray(X).shape, np.asarray(y).shape)
            return 0.75

        def predict(self, X):
            return np.asarray(X)[:, 0] * 0
    monkeypatch.setattr(S, 'RBFSVM', FakeSVM)
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    tr = np.arange(len(y)) % 6 != 0
    sets = [X[tr], X[~tr], y[tr], y[~tr]]
    got = S.mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, backend='hip')
    assert got == 1.0 - 0.75 and len(made) == 1
    assert made[0].kw == dict(C=1.0, gamma='auto')
    assert made[0].fit_shapes == ((120, 40), (120,)) and made[0].score_shapes == (((~tr).sum(), 40), ((~tr).sum(),))
    # the default backend never touches RBFSVM
    S.mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3)
    assert len(made) == 1
