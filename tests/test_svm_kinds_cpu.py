"""The numpy restatement of the device nu-SVC (tests/svm_kinds_ref.py) pinned against scikit-learn / libsvm, and the host side of
mr_gan_amd.svm.KernelSVM and of mr_svm(classifier=...) that runs without a GPU."""
import numpy as np
import pytest

from mr_gan_amd import synthetic_mreo
from tests import svm_kinds_ref as N
from tests import svm_ref as R
from tests.test_svm_gpu import solver_case

NU_CASES = [('two_rows', 0.5), ('unequal', 0.1), ('unequal', 0.3), ('single_row_class', 0.1), ('pair_2048', 0.5),
            ('c100_all_free', 0.1), ('bounded_heavy', 0.5)]


@pytest.mark.parametrize("name,nu", NU_CASES)
def test_nu_restatement_matches_libsvm_on_the_rounded_gram(name, nu):
    """NuSVC(kernel='precomputed', tol=1e-8) and the restatement solve the same rounded problem.  Both stop with the violation of
    the un-normalised problem below tol; the model is that solution divided by r, so the decisions agree to 10 tol / r (the
    factor 10 of test_svm_cpu.py's C-SVC check, carried through the division).  Measured max |dec - libsvm|:
    two_rows 0, unequal 1.11e-15 (nu 0.1) and 5.69e-9 (nu 0.3), single_row_class 1.52e-8, pair_2048 8.88e-15 (635 iterations
    on both sides), c100_all_free 1.0e-7, bounded_heavy 1.33e-15"""
    from sklearn.svm import NuSVC
    y, cs, K, _ = solver_case(name)
    assert N.nu_feasible(cs, nu) is None
    coef, rho, r, iters = N.solve_ovo_nu(K, cs, nu, 1e-8)
    K64 = K.astype(np.float64)
    svc = NuSVC(kernel='precomputed', nu=nu, tol=1e-8, decision_function_shape='ovo').fit(K64, y)
    want = svc.decision_function(K64)
    if len(cs) == 3:
        want = -want[:, None]                # scikit-learn flips the sign of a two-class decision function; libsvm does not
    dec = R.decisions(coef, rho, K64, cs)
    print("%s nu %g: max |dec - libsvm| = %.3g, iterations %s, libsvm's %s, r >= %.3g"
          % (name, nu, np.abs(dec - want).max(), iters.tolist(), np.asarray(svc.n_iter_).tolist(), r.min()))
    assert (r > 0).all() and (iters < 10_000_000).all()
    assert np.abs(dec - want).max() <= 10 * 1e-8 / r.min()
    if name == 'two_rows':
        assert iters.tolist() == [0]
    for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
        rows, yy = R.pair_rows(cs, i, j)
        alpha = R.pair_alpha(coef, cs, i, j) * r[p]
        alpha = np.where(np.abs(alpha - 1.0) <= 4 * 2.0 ** -53, 1.0, alpha)       # coef r: two roundings away from the bound
        assert (alpha >= 0).all() and (alpha <= 1).all()
        for sign in (1.0, -1.0):
            assert abs(alpha[yy == sign].sum() - nu * len(yy) / 2) <= 64 * np.finfo(np.float64).eps * nu * len(yy) / 2
        assert N.nu_kkt_gap(K64[np.ix_(rows, rows)], yy, alpha) < 1e-8 * (1 + 1e-6)


@pytest.mark.parametrize("name", ['two_rows', 'unequal', 'single_row_class', 'pair_2048', 'c100_all_free', 'bounded_heavy'])
@pytest.mark.parametrize("nu", [0.1, 0.5])
def test_nu_feasible_is_scikit_learns_verdict(name, nu):
    """libsvm refuses nu where nu (n_i + n_j) / 2 > min(n_i, n_j) for some pair: 'unequal' and 'single_row_class' at nu = 0.5"""
    from sklearn.svm import NuSVC
    from mr_gan_amd.svm import nu_infeasible_pair
    y, cs, K, _ = solver_case(name)
    if name == 'pair_2048':
        y, cs, K = y[512:1536], np.array([0, 512, 1024]), K[512:1536, 512:1536]      # the same verdict (equal classes), a quicker fit
    try:
        NuSVC(kernel='precomputed', nu=nu, tol=1e-1).fit(K.astype(np.float64), y)
        refused = False
    except ValueError as e:
        assert "infeasible" in str(e)
        refused = True
    assert (N.nu_feasible(cs, nu) is not None) == refused
    assert nu_infeasible_pair(cs, nu) == N.nu_feasible(cs, nu)
    if nu == 0.5:
        assert refused == (name in ('unequal', 'single_row_class'))
    if nu == 0.1:
        assert not refused


def test_linear_gram_restatement():
    rs = np.random.RandomState(0)
    A, B = rs.randn(5, 3).astype(np.float32), rs.randn(4, 3).astype(np.float32)
    G = N.linear_gram(A, B)
    assert G.dtype == np.float64 and G.shape == (5, 4)
    assert np.abs(G - np.array([[float(np.dot(a.astype(np.float64), b.astype(np.float64))) for b in B] for a in A])).max() <= 1e-15


def test_kernelsvm_checks_arguments_before_any_device_call():
    from mr_gan_amd import KernelSVM
    for kw in (dict(kernel='poly'), dict(kernel=None), dict(nu=0.0), dict(nu=-0.1), dict(nu=1.5), dict(nu=float('nan')), dict(nu='0.5'),
               dict(gamma='scale'), dict(gamma=0.0), dict(C=0.0), dict(tol=-1.0), dict(max_iter=0), dict(C=float('nan'))):
        with pytest.raises(ValueError):
            KernelSVM(**kw)
    clf = KernelSVM()
    assert (clf.kernel, clf.nu, clf.C, clf.gamma, clf.tol, clf.max_iter, clf.r_) == ('rbf', None, 1.0, 'auto', 1e-3, 10_000_000, None)
    assert KernelSVM(kernel='linear', nu=1).nu == 1.0
    x = np.zeros((4, 3))
    with pytest.raises(ValueError, match="non-finite"):
        clf.fit(np.array([[0.0, np.inf, 0.0]] * 4), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="KernelSVM needs 2 to 32 classes"):
        clf.fit(x, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="rows"):
        clf.fit(x, [0, 1, 1])
    with pytest.raises(ValueError, match="MRGAN_SVM_MAX_PAIR"):
        clf.fit(np.zeros((2049, 1)), [0] * 1025 + [1] * 1024)
    with pytest.raises(RuntimeError, match="KernelSVM: fit"):
        clf.predict(x)
    # nu-feasibility from the class counts, in scikit-learn's words, naming the classes: 0.5 * (7 + 33) / 2 = 10 > 7
    with pytest.raises(ValueError, match="specified nu is infeasible.*classes 3 and 8"):
        KernelSVM(nu=0.5).fit(np.zeros((40, 2)), [3] * 7 + [8] * 33)
    # the same counts pass this check at nu = 0.1; C-SVC never makes it
    for ok in (KernelSVM(nu=0.1), KernelSVM(kernel='linear')):
        ok._check_classes(np.array([3, 8]), np.array([0, 7, 40]))


def test_classifier_flag_reaches_fn_and_both_backends_build_the_right_class(monkeypatch, capsys):
    """--classifier parses to one of the four kinds and reaches fn only when it is not the default; --group-folds refuses the
    others; the scikit-learn backend builds SVC / NuSVC(nu=0.5) with the kind's kernel, the hip backend KernelSVM"""
    import sklearn.svm
    import mr_gan_amd.mr_svm as S
    rs = np.random.RandomState(0)

    def fake_dataset(modalities=0, leaveObjectOut=False, **kw):
        if leaveObjectOut:
            return {'m%d_o%d' % (m, o): {'x': rs.randn(4, 3).tolist(), 'y': [m] * 4} for m in range(6) for o in range(2)}
        return rs.randn(36, 3), np.arange(36) % 6
    seen = []
    fn = lambda X, y, **kw: seen.append(kw) or 0.5
    S.main(['--tables', '4'], dataset_fn=fake_dataset, fn=fn)
    assert seen and all('classifier' not in kw and 'backend' not in kw for kw in seen)
    seen.clear()
    S.main(['--tables', '4', '--classifier', 'svc-rbf', '--backend', 'hip'], dataset_fn=fake_dataset, fn=fn)
    assert seen and all('classifier' not in kw and kw.get('backend') == 'hip' for kw in seen)
    for name in ('svc-linear', 'nu-rbf', 'nu-linear'):
        seen.clear()
        S.main(['--tables', '4', '--classifier', name], dataset_fn=fake_dataset, fn=fn)
        assert seen and all(kw.get('classifier') == name and 'backend' not in kw for kw in seen)
    for bad in (['--classifier', 'linear-svc'], ['--backend', 'hip', '--group-folds', '--classifier', 'nu-rbf']):
        with pytest.raises(SystemExit):
            S.main(['--tables', '4'] + bad, dataset_fn=fake_dataset, fn=fn)
    capsys.readouterr()
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    tr = np.arange(len(y)) % 6 != 0
    sets = [X[tr], X[~tr], y[tr], y[~tr]]
    with pytest.raises(ValueError, match="classifier"):
        S.mr_svm(None, None, trainTestSets=sets, classifier='linear-svc')

    made = []

    def fake(cls_name):
        class Fake:
            def __init__(self, **kw):
                self.name, self.kw = cls_name, kw
                made.append(self)

            def fit(self, X, y):
                self.fit_shapes = (np.asarray(X).shape, np.asarray(y).shape)
                return self

            def score(self, X, y):
                return 0.75

            def predict(self, X):
                return np.asarray(X)[:, 0] * 0
        return Fake
    monkeypatch.setattr(S, 'RBFSVM', fake('RBFSVM'))
    monkeypatch.setattr(S, 'KernelSVM', fake('KernelSVM'))
    monkeypatch.setattr(sklearn.svm, 'SVC', fake('SVC'))
    monkeypatch.setattr(sklearn.svm, 'NuSVC', fake('NuSVC'))
    want = {('hip', 'svc-rbf'): ('RBFSVM', dict(C=1.0, gamma='auto')),
            ('hip', 'svc-linear'): ('KernelSVM', dict(kernel='linear', nu=None, C=1.0, gamma='auto')),
            ('hip', 'nu-rbf'): ('KernelSVM', dict(kernel='rbf', nu=0.5, C=1.0, gamma='auto')),
            ('hip', 'nu-linear'): ('KernelSVM', dict(kernel='linear', nu=0.5, C=1.0, gamma='auto')),
            ('sklearn', 'svc-rbf'): ('SVC', dict(kernel='rbf', C=1.0, gamma='auto')),
            ('sklearn', 'svc-linear'): ('SVC', dict(kernel='linear', C=1.0, gamma='auto')),
            ('sklearn', 'nu-rbf'): ('NuSVC', dict(kernel='rbf', nu=0.5, gamma='auto')),
            ('sklearn', 'nu-linear'): ('NuSVC', dict(kernel='linear', nu=0.5, gamma='auto'))}
    for (backend, classifier), (cls_name, kw) in want.items():
        made.clear()
        got = S.mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, backend=backend, classifier=classifier)
        assert got == 1.0 - 0.75 and len(made) == 1
        assert (made[0].name, made[0].kw) == (cls_name, kw)
        assert made[0].fit_shapes == ((120, 40), (120,))
