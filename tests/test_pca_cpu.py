"""PCA pre-stage without a GPU: the restatement of tests/pca_ref.py against scikit-learn's full solver, the preconditions of the
designed cases, pca_scale against a transcription of the reference's pcaScale, the host checks of PCA (no device call before
they pass), mr_svm(pca=) and mr_gan_pca on stand-ins, and the declared entries."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import pca_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against scikit-learn -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_restatement_matches_sklearn_full(name):
    from sklearn import decomposition
    X, k, p, tol = R.case(name)
    sk = decomposition.PCA(n_components=k, svd_solver='full').fit(X)
    ref = R.fit(X, k)
    # an eigenvector moves by (error of the matrix) / gap: float64 eigh on C against float64 SVD on X
    comp_tol = 1e-13 / R.gaps(ref['spectrum'], k) + 1e-10
    assert (np.linalg.norm(ref['components'] - sk.components_, axis=1) <= comp_tol).all()          # signs included
    np.testing.assert_allclose(ref['explained_variance'], sk.explained_variance_, rtol=1e-9)
    np.testing.assert_allclose(ref['explained_variance_ratio'], sk.explained_variance_ratio_, rtol=1e-9)
    np.testing.assert_allclose(ref['singular_values'], sk.singular_values_, rtol=1e-9)
    np.testing.assert_allclose(ref['noise_variance'], sk.noise_variance_, rtol=1e-9)
    np.testing.assert_allclose(ref['mean'], sk.mean_, rtol=1e-13, atol=1e-13)
    Z, Zsk = R.transform(X, ref['mean'], ref['components']), sk.transform(X)
    assert (np.abs(Z - Zsk) <= np.linalg.norm(X - sk.mean_, axis=1)[:, None] * comp_tol[None, :] + 1e-10).all()
    back = R.inverse_transform(Z, ref['mean'], ref['components'])
    np.testing.assert_allclose(back, sk.inverse_transform(Zsk), atol=1e-8)


def test_sign_rule_takes_the_first_of_tied_maxima():
    W = np.array([[0.5, -2.0, 2.0], [-1.0, 0.25, 1.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(R.sign_rule(W), [[-0.5, 2.0, -2.0], [1.0, -0.25, -1.0], [0.0, 0.0, 0.0]])


# ---- 2. the preconditions of the cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_designed_cases_separate_their_eigenvalues(name):
    from mr_gan_amd.pca import block_width
    X, k, p, tol = R.case(name)
    lam = R.fit(X, k)['spectrum']
    m = R.SEPARATED[name]
    assert block_width(k, X.shape[1]) == p
    assert R.gaps(lam, k)[:m].min() >= 100 * tol * lam[0]
    assert m == k or name == 'C'                               # C asks for more components than its design can separate (pca_ref.SEPARATED)
    if name == 'C':
        assert lam[k - 1] > 2.0 ** -20 * lam[0]                # ... but every wanted direction stays above the rank floor (2^-40 in Lambda = lambda^2)


def test_degenerate_cases_are_what_they_claim():
    from mr_gan_amd.pca import block_width
    rank = lambda X: np.linalg.matrix_rank(R.covariance(X, R.mean(X)))
    X, k, p, _ = R.case('D')
    assert p == X.shape[1] == block_width(k, X.shape[1]) and rank(X) == p          # the block is the whole space
    X, k, p, _ = R.case('E')
    assert k <= rank(X) == 11 < p == block_width(k, X.shape[1])                    # the guard directions collapse
    X, k, p, _ = R.case('F')
    assert rank(X) == 7 < k                                                        # the rank error


# ---- 3. pca_scale against the reference's function -------------------------------------------------------------------------
def pcaScale(Xtrain, Xtest, PCA=0, scale=None):
    """others/wganlpctsemi.py:129-139, transcribed"""
    from sklearn import decomposition, preprocessing
    if PCA > 0:
        pca = decomposition.PCA(n_components=PCA)
        Xtrain = pca.fit_transform(Xtrain)
        Xtest = pca.transform(Xtest)
    if scale is not None:
        scaler = preprocessing.Normalizer() if scale == 'norm' else preprocessing.StandardScaler()
        Xtrain = scaler.fit_transform(Xtrain)
        Xtest = scaler.transform(Xtest)
    return Xtrain, Xtest


@pytest.mark.parametrize("n_components", [0, 5])
@pytest.mark.parametrize("scale", [None, 'norm', 'standard'])
def test_pca_scale_sklearn_backend_is_pcaScale(n_components, scale):
    from mr_gan_amd.pca import pca_scale
    rng = np.random.default_rng(2)
    Xtr, Xte = rng.standard_normal((120, 40)) * (1 + np.arange(40)), rng.standard_normal((30, 40))       # (a shape whose 'auto' solver is 'full')
    want = pcaScale(Xtr, Xte, PCA=n_components, scale=scale)
    got = pca_scale(Xtr, Xte, PCA=n_components, scale=scale, backend='sklearn')
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-10)
    with pytest.raises(ValueError, match="backend"):
        pca_scale(Xtr, Xte, PCA=5, backend='cuda')


# ---- 4. the host checks come before any device call ------------------------------------------------------------------------
def test_pca_checks_arguments_before_any_device_call(monkeypatch):
    from mr_gan_amd import engine as E
    from mr_gan_amd.pca import PCA
    monkeypatch.setattr(E.DeviceCalls, '_call', lambda self, *a: pytest.fail("no library call before the checks pass"))
    monkeypatch.setattr(E.DeviceCalls, '_require_gpu', lambda self: pytest.fail("no device before the checks pass"))
    for bad in (0, 65, 2.5, -1):
        with pytest.raises(ValueError, match="n_components"):
            PCA(bad)
    for kw in (dict(tol=0.0), dict(tol=float('nan')), dict(max_iter=0), dict(max_iter=1.5)):
        with pytest.raises(ValueError, match="tol|max_iter"):
            PCA(3, **kw)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((12, 9))
    with pytest.raises(ValueError, match="non-finite"):
        PCA(3).fit(np.where(np.arange(9) == 4, np.inf, X))
    with pytest.raises(ValueError, match="matrix"):
        PCA(3).fit(X[0])
    with pytest.raises(ValueError, match=r"min\(n_samples - 1, n_features"):
        PCA(9).fit(X[:9])                                      # n - 1 = 8 < 9
    with pytest.raises(ValueError, match=r"min\(n_samples - 1, n_features"):
        PCA(10).fit(X)                                         # d = 9 < 10
    with pytest.raises(ValueError, match="MRGAN_PCA_MAX_FEATURES"):
        PCA(1).fit(np.zeros((3, 4097)))
    pca = PCA(3)
    for call in (lambda: pca.transform(X), lambda: pca.inverse_transform(X[:, :3])):
        with pytest.raises(RuntimeError, match="fit"):
            call()
    pca.components_, pca.n_features_in_ = np.zeros((3, 9)), 9              # as after a fit
    with pytest.raises(ValueError, match="8 features, the model was fitted on 9"):
        pca.transform(X[:, :8])
    with pytest.raises(ValueError, match="4 features, the model was fitted on 3"):
        pca.inverse_transform(X[:, :4])
    with pytest.raises(ValueError, match="chunk"):
        pca.transform(X, chunk=0)


def test_pca_has_no_cpu_path(monkeypatch):
    import torch
    from mr_gan_amd.pca import PCA
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match="PCA runs on the GPU only"):
        PCA(2).fit(np.random.default_rng(0).standard_normal((8, 5)))


# ---- 5. mr_svm(pca=) -------------------------------------------------------------------------------------------------------
def _svm_sets(seed=0):
    X, y = R.six_classes(n_per_class=40, d=30, seed=seed)
    test = np.arange(len(y)) % 4 == 3
    return [X[~test], X[test], y[~test], y[test]]


def test_mr_svm_without_pca_issues_todays_calls(monkeypatch):
    from mr_gan_amd import mr_svm as S
    seen = []
    real = S.prologue

    def recording(sets, percentlabeled, percentunlabeled, rs, num_classes, **kw):
        seen.append(kw)
        return real(sets, percentlabeled, percentunlabeled, rs, num_classes, **kw)
    monkeypatch.setattr(S, 'prologue', recording)
    sets = _svm_sets()
    a = S.mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3)
    b = S.mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, pca=0)
    assert a == b and seen == [dict(transform=None), dict(transform=None)]
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="pca"):
            S.mr_svm(None, None, trainTestSets=sets, pca=bad)
    with pytest.raises(ValueError, match="pca"):
        S.mr_svm_folds([sets], pca=-2)


def test_mr_svm_with_pca_on_sklearn_is_prologue_pca_svc():
    from sklearn import decomposition
    from sklearn.svm import SVC
    from sklearn.utils import shuffle
    from mr_gan_amd.data import select_labeled, standard_scale
    from mr_gan_amd.mr_svm import mr_svm
    sets = _svm_sets(4)
    got = mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=7, backend='sklearn', pca=10)
    rs = np.random.RandomState(7)
    Xtr, Xte = standard_scale(sets[0], sets[1])
    pca = decomposition.PCA(n_components=10, svd_solver='full')
    Ztr, Zte = pca.fit_transform(Xtr), pca.transform(Xte)
    Ztr, ytr = shuffle(Ztr, sets[2], random_state=rs)
    xl, yl, _ = select_labeled(Ztr, ytr, 20)
    assert xl.shape == (120, 10)
    want = 1.0 - SVC(kernel='rbf', C=1.0, gamma='auto').fit(xl, yl).score(Zte, sets[3])
    assert got == want


def test_mr_svm_command_line_takes_pca(capsys):
    from mr_gan_amd import mr_svm as S
    calls, fold_calls = [], []

    def fake_dataset(modalities=0, **kw):
        rng = np.random.default_rng(modalities)
        return rng.standard_normal((72, 5)), np.arange(72) % 6

    def fn(X, y, percentlabeled=50, trainTestSets=None, verbose=False, **kw):
        calls.append(kw)
        return 0.25

    def folds_fn(sets, percentlabeled=50, verbose=False, **kw):
        fold_calls.append(kw)
        return [0.5] * len(sets)
    S.main(['--tables', '2', '--pca', '10'], dataset_fn=fake_dataset, fn=fn)
    assert calls and all(kw == dict(pca=10) for kw in calls)
    del calls[:]
    S.main(['--tables', '2'], dataset_fn=fake_dataset, fn=fn)
    assert calls and all(kw == {} for kw in calls)             # the default leaves every call as it was
    S.main(['--tables', '2', '--backend', 'hip', '--group-folds', '--pca', '4'], dataset_fn=fake_dataset, fn=fn, folds_fn=folds_fn)
    assert fold_calls and all(kw == dict(pca=4) for kw in fold_calls)
    with pytest.raises(SystemExit):
        S.main(['--tables', '2', '--pca', '-3'], dataset_fn=fake_dataset, fn=fn)
    capsys.readouterr()


# ---- 6. mr_gan_pca on stand-ins --------------------------------------------------------------------------------------------
def test_mr_gan_pca_on_stand_ins(monkeypatch, capsys):
    from mr_gan_amd import autoencoder as A
    from mr_gan_amd import pca as P
    from mr_gan_amd.data import synthetic_mreo
    X, y, _ = synthetic_mreo(d=40, objects_per_class=3, trials=40)
    X = X * 3.0 + 7.0
    rng = np.random.default_rng(0)
    te = np.zeros(len(y), bool)
    for c in range(6):
        te[rng.permutation(np.flatnonzero(y == c))[:10]] = True
    sets = [X[~te], X[te], y[~te], y[te]]
    n_tr, n_te = int((~te).sum()), int(te.sum())
    seen = {}

    class FakePCA(object):
        def __init__(self, n_components, tol, max_iter, random_state, device):
            seen['pca'] = (n_components, tol, max_iter, device)
            self.k = n_components

        def fit_transform(self, X):
            seen['fit'] = X.copy()
            return np.full((len(X), self.k), 1.0, np.float32)

        def transform(self, X):
            seen['transform'] = X.copy()
            return np.full((len(X), self.k), 2.0, np.float32)

    class FakeGAN(object):
        def __init__(self, input_dim, **kw):
            seen['gan'] = (input_dim, kw['batch_size'], kw['num_classes'])

        def fit(self, x_labeled, y_labeled, x_unlabeled, epochs, verbose, validation_data, x_unlabeled_pool, rng):
            seen['gan_fit'] = (x_labeled.shape, x_unlabeled.shape, validation_data[0].shape, epochs, x_unlabeled_pool)
            seen['codes'] = (float(x_unlabeled[0, 0]), float(validation_data[0][0, 0]))
            return [dict(test_err=0.5)]

        def evaluate(self, X, y):
            return 0.125

        def close(self):
            pass
    monkeypatch.setattr(P, 'PCA', FakePCA)
    monkeypatch.setattr(A, 'MRGAN', FakeGAN)
    acc = P.mr_gan_pca(None, None, percentlabeled=2, epochs=3, trainTestSets=sets, n_components=7, seed=1, verbose=True)
    assert acc == 1.0 - 0.125                                  # the ACCURACY, as mr_gan_autoencoder returns
    assert seen['pca'] == (7, 1e-6, 1000, 'cuda:0')
    mu, sd = sets[0].mean(axis=0), sets[0].std(axis=0)         # fitted on the standard-scaled training rows, applied to the scaled test rows
    np.testing.assert_allclose(seen['fit'], (sets[0] - mu) / sd, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(seen['transform'], (sets[1] - mu) / sd, rtol=1e-9, atol=1e-9)
    assert seen['gan'] == (7, 50, 6)                           # the GAN sees n_components inputs
    assert seen['gan_fit'] == ((6 * 20, 7), (n_tr, 7), (n_te, 7), 3, None) and seen['codes'] == (1.0, 2.0)
    assert "(%d, 7) (%d, 7)" % (n_tr, n_te) in capsys.readouterr().out          # the shape line of mr_gan_autoencoder
    with pytest.raises(ValueError):
        P.mr_gan_pca(None, None, trainTestSets=sets, noise='white')             # refused before any data is touched


def test_the_two_pre_stages_share_one_body():
    from mr_gan_amd import autoencoder as A
    from mr_gan_amd import pca as P
    assert 'gan_on_codes(' in inspect.getsource(A.mr_gan_autoencoder) and 'gan_on_codes(' in inspect.getsource(P.mr_gan_pca)
    assert 'MRGAN(' not in inspect.getsource(P)


# ---- 7. the entries --------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    import mr_gan_amd
    from mr_gan_amd import engine as E
    abi = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    dbg = open(os.path.join(ROOT, "include", "mrgan_debug.h")).read()
    declared = lambda src: set(re.findall(r"\b(mrgan_(?:debug_)?pca_[a-z0-9_]+)\s*\(", src))
    public = {"mrgan_pca_mean", "mrgan_pca_covariance", "mrgan_pca_covariance_workspace_bytes", "mrgan_pca_eig", "mrgan_pca_eig_workspace_bytes",
              "mrgan_pca_transform", "mrgan_pca_inverse_transform"}
    debug = {"mrgan_debug_pca_covariance", "mrgan_debug_pca_covariance_workspace_bytes", "mrgan_debug_pca_orthonormalize"}
    assert declared(abi) == public and declared(dbg) == debug
    lib = E.load_library()
    for name in public | debug:
        assert name in E.EXPORTS and hasattr(lib, name)
    vals = {m: int(re.search(r"#define %s \(?(-?\d+)\)?" % m, abi).group(1))
            for m in ("MRGAN_PCA_MAX_COMPONENTS", "MRGAN_PCA_GUARD", "MRGAN_PCA_MAX_FEATURES", "MRGAN_PCA_RANK_DEFICIENT")}
    assert list(vals.values()) == [E.PCA_MAX_COMPONENTS, E.PCA_GUARD, E.PCA_MAX_FEATURES, E.PCA_RANK_DEFICIENT] == [64, 16, 4096, -4]
    # the workspace queries are host arithmetic: they answer without a device
    assert lib.mrgan_pca_eig_workspace_bytes(1200, 16) == (2 * 32 * 32 + 3 * 32 + 2) * 8 + 2 * 32 * 1200 * 4
    assert lib.mrgan_pca_eig_workspace_bytes(20, 10) == (2 * 20 * 20 + 3 * 20 + 2) * 8 + 2 * 20 * 20 * 4           # p = d
    assert lib.mrgan_pca_eig_workspace_bytes(1200, 65) == -1 and lib.mrgan_pca_covariance_workspace_bytes(6000, 4097) == -1
    assert lib.mrgan_pca_covariance_workspace_bytes(6000, 1200) == lib.mrgan_debug_pca_covariance_workspace_bytes(6000, 1200, 0, 0) > 0
    assert lib.mrgan_debug_pca_covariance_workspace_bytes(17, 257, 64, 5) == 2 * 15 * 64 * 64 * 4                  # 5 ranges clamp to ceil(17 / 16)
    for name in ("PCA", "pca_scale", "mr_gan_pca"):
        assert name in mr_gan_amd.__all__ and hasattr(mr_gan_amd, name)
