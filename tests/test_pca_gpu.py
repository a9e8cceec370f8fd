"""The PCA pre-stage (csrc/pca.hip, mr_gan_amd/pca.py) on the GPU, stage by stage against the float64 restatement of
tests/pca_ref.py: every bound is a theorem (Rayleigh-Ritz residual bounds, Davis-Kahan, Weyl) or computed from the operands
(u = 2^-24 per rounding), none is tuned on the code under test.  Then PCA end to end against scikit-learn's full solver and
mr_svm(pca=10, backend='hip') on the harness."""
import warnings

import numpy as np
import pytest

from tests import pca_ref as R

pytestmark = pytest.mark.gpu
U = R.U
U64_SUM = 2.0 ** -40            # a float64 sum of d <= 4096 diagonal entries: d 2^-53, with room
DEV = "cuda:0"


def _torch():
    import torch
    return torch


def to_dev(a, dtype=np.float32):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def stages(k=1, **kw):
    from mr_gan_amd.pca import PCA
    return PCA(k, **kw)


_dev_cache = {}


def device_fit_parts(name):
    """case -> (X, k, p, tol, mean32, C_dev as float64), the device's own mean and covariance, computed once"""
    if name not in _dev_cache:
        X, k, p, tol = R.case(name)
        s = stages()
        x = to_dev(X)
        mean = s.mean_dev(x)
        cov = host(s.covariance_dev(x, mean)).astype(np.float64)
        cov.setflags(write=False)
        _dev_cache[name] = (X, k, p, tol, host(mean), cov)
    return _dev_cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# mean
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "one-row"])
def test_mean_against_fp64(which):
    X = R.case('A')[0] if which == "A" else R.plain(1, 97, 3)
    got = host(stages().mean_dev(to_dev(X))).astype(np.float64)
    err, bound = np.abs(got - R.mean(X)), R.mean_bound(X)
    print("mean %s: max err / bound = %.3f" % (which, (err / bound).max()))
    assert (err <= bound).all()
    if which == "one-row":
        np.testing.assert_array_equal(got, X[0])


# ---------------------------------------------------------------------------------------------------------------------
# covariance
# ---------------------------------------------------------------------------------------------------------------------
def cov_data(which):
    return R.case(which)[0] if which in R.CASES else R.plain(17, 257, 5)


def cov_check(X, mean32, got, label):
    want = R.covariance(X, mean32)
    Xc = np.abs(X - mean32.astype(np.float64))
    n = len(X)
    bound = (n + 2) * U * (Xc.T @ Xc) / (n - 1) + 2.0 ** -149
    err = np.abs(got.astype(np.float64) - want)
    print("covariance %s: max err / bound = %.4f, max err = %.3g" % (label, (err / bound).max(), err.max()))
    assert (err <= bound).all()
    np.testing.assert_array_equal(got, got.T)                  # bit for bit


@pytest.mark.parametrize("which", ["A", "B", "17x257"])
def test_covariance_against_fp64_and_symmetric(which):
    X = cov_data(which)
    s, x = stages(), to_dev(X)
    mean = s.mean_dev(x)
    got = host(s.covariance_dev(x, mean))
    cov_check(X, host(mean), got, which)
    again = host(s.covariance_dev(x, mean))
    np.testing.assert_array_equal(got, again)                  # two runs, identical bits


@pytest.mark.parametrize("which", ["A", "B", "17x257"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("split", [1, 2, 5])
def test_covariance_forced_tile_and_split(which, tile, split):
    X = cov_data(which)
    s, x = stages(), to_dev(X)
    mean = s.mean_dev(x)
    cov_check(X, host(mean), host(s.covariance_dev(x, mean, tile=tile, split=split)), "%s tile %d split %d" % (which, tile, split))


def test_covariance_pitched_buffers_keep_their_padding():
    torch = _torch()
    X = R.case('A')[0]
    n, d = X.shape
    xbuf = torch.full((n, d + 5), float('nan'), dtype=torch.float32, device=DEV)          # a read past the row poisons the result
    xbuf[:, :d] = to_dev(X)
    s = stages()
    mean = s.mean_dev(xbuf[:, :d])
    out = torch.full((d + 1, d + 3), -7.0, dtype=torch.float32, device=DEV)
    s.covariance_dev(xbuf[:, :d], mean, out=out[:d, :d])
    full = host(out)
    assert (full[:, d:] == -7.0).all() and (full[d] == -7.0).all()
    cov_check(X, host(mean), full[:d, :d], "A pitched")
    np.testing.assert_array_equal(full[:d, :d], host(s.covariance_dev(to_dev(X), mean)))


# ---------------------------------------------------------------------------------------------------------------------
# orthonormalisation stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random 28x97", "ill-conditioned 80x160"])
def test_orthonormalisation_stage(which):
    rng = np.random.default_rng(7)
    if which.startswith("random"):
        Y = rng.standard_normal((28, 97))
    else:
        Y = rng.standard_normal((80, 160)) * np.logspace(0, -5, 80)[:, None]          # the block's directions at scales 1 .. 1e-5
    Y = Y.astype(np.float32)
    p, d = Y.shape
    q, lam = stages().orthonormalize_dev(to_dev(Y))
    Q, lam, Y64 = host(q).astype(np.float64), host(lam), Y.astype(np.float64)
    ortho = np.abs(Q @ Q.T - np.eye(p)).max()
    A = Y64 @ Q.T
    resid, bound = np.abs(Y64 - A @ Q), R.chain_bound(A, Q, d)
    print("orthonormalise %s: |QQ^T - I| = %.3g (bound %.3g), row space err / bound = %.4f, lam %.3g .. %.3g"
          % (which, ortho, (d + 2) * U, (resid / bound).max(), lam[0], lam[-1]))
    assert ortho <= (d + 2) * U
    assert (resid <= bound).all()
    assert (np.diff(lam) <= 0).all() and lam[-1] > 0
    want = np.linalg.eigvalsh(Y64 @ Y64.T)[::-1]
    assert np.abs(lam - want).max() <= 1e-10 * want[0]


# ---------------------------------------------------------------------------------------------------------------------
# eigen stage: the device's own covariance, downloaded and taken as exact
# ---------------------------------------------------------------------------------------------------------------------
MAX_ITER = 300


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_eigen_stage(name):
    X, k, p, tol, _, C = device_fit_parts(name)
    d = C.shape[0]
    from mr_gan_amd.pca import block_width
    assert block_width(k, d) == p
    s = stages(k, tol=tol, max_iter=MAX_ITER)
    w, theta, res_dev, iters = s.eig_dev(to_dev(C))
    W = host(w).astype(np.float64)
    lam, V = R.spectrum(C)
    slack = R.matvec_bound(C)
    res = np.linalg.norm(W @ C - theta[:, None] * W, axis=1) / np.linalg.norm(W, axis=1)
    limit = tol * theta[0] + slack
    delta = R.gaps_from(theta, lam)
    sines = np.array([R.sine(W[i], V[i]) for i in range(k)])
    ortho = np.abs(W @ W.T - np.eye(k)).max()
    print("eig %s: %d products, max res = %.3g (device %.3g, limit %.3g), max |theta - lam| = %.3g, max sine / bound = %.3g, "
          "|WW^T - I| = %.3g" % (name, iters, res.max(), res_dev.max(), limit, np.abs(theta - lam[:k]).max(),
                                 (sines / np.maximum(res / delta, 1e-300)).max(), ortho))
    assert 1 <= iters < MAX_ITER and res_dev.max() <= tol * theta.max()          # converged
    assert (res <= limit).all()
    assert (np.abs(theta - lam[:k]) <= limit).all()
    assert (sines <= res / delta * (1 + 1e-9) + 1e-12).all()   # Davis-Kahan on the pair's own residual (vacuous where delta_i is below it)
    assert (sines <= limit / delta).all()
    assert ortho <= (d + 2) * U
    assert (np.diff(theta) <= 0).all()
    np.testing.assert_array_equal(W, R.sign_rule(W))
    if name in R.SEPARATED:                                    # where the design separates the eigenvalues the bound is a real one
        m = R.SEPARATED[name]
        assert (limit / delta[:m]).max() < 0.2 and sines[:m].max() < 0.2


def test_eigen_stage_stops_at_max_iter_with_outputs_written():
    X, k, p, tol, _, C = device_fit_parts('B')
    w, theta, res, iters = stages(k, tol=tol, max_iter=1).eig_dev(to_dev(C))
    W = host(w)
    assert iters == 1 and res.max() > tol * theta.max()
    assert np.isfinite(W).all() and (np.abs(W).max(axis=1) > 0).all() and (theta > 0).all() and (np.diff(theta) <= 0).all()
    np.testing.assert_array_equal(W, R.sign_rule(W))


def test_rank_below_n_components_is_the_rank_error():
    from mr_gan_amd import engine as E
    from mr_gan_amd.pca import PCA
    X, k, p, tol = R.case('F')                                 # 8 rows: rank 7 < k = 10; the estimator's n_components <= n - 1 is
    s = stages(k, tol=tol)                                     # bypassed by calling the entry on the device's covariance
    x = to_dev(X)
    cov = s.covariance_dev(x, s.mean_dev(x))
    with pytest.raises(E.MrganError, match="numerical rank below n_components") as info:
        s.eig_dev(cov)
    assert info.value.code == E.PCA_RANK_DEFICIENT
    with pytest.raises(ValueError, match="numerical rank"):    # the estimator: the same rows twice pass its host check
        PCA(k, tol=tol).fit(np.concatenate([X, X]))


# ---------------------------------------------------------------------------------------------------------------------
# transform / inverse
# ---------------------------------------------------------------------------------------------------------------------
def test_transform_and_inverse_under_the_product_bound():
    X, k, p, tol, mean32, C = device_fit_parts('A')
    d = X.shape[1]
    s = stages(k, tol=tol)
    w = s.eig_dev(to_dev(C))[0]
    W, mean = host(w), to_dev(mean32)
    z = s.transform_dev(to_dev(X), mean, w)
    Z = host(z)
    Xc = X - mean32.astype(np.float64)
    err, bound = np.abs(Z - Xc @ W.astype(np.float64).T), R.chain_bound(Xc, W.T, d)
    print("transform: max err / bound = %.4f" % (err / bound).max())
    assert (err <= bound).all()
    back = host(s.inverse_dev(z, mean, w))
    want = R.inverse_transform(Z, mean32, W)
    bound = (k + 2) * U * (np.abs(Z.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(mean32.astype(np.float64)))
    err = np.abs(back - want)
    print("inverse: max err / bound = %.4f" % (err / bound).max())
    assert (err <= bound).all()


def test_transform_chunks_change_no_bit():
    from mr_gan_amd.pca import PCA
    X, k, p, tol = R.case('A')
    pca = PCA(k, tol=tol).fit(X)
    whole = pca.transform(X)
    np.testing.assert_array_equal(pca.transform(X, chunk=7), whole)
    np.testing.assert_array_equal(pca.inverse_transform(whole, chunk=7), pca.inverse_transform(whole))
    with pytest.raises(ValueError, match="features"):
        pca.transform(X[:, :-1])


# ---------------------------------------------------------------------------------------------------------------------
# PCA end to end against scikit-learn's full solver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pca_against_sklearn_full(name):
    from sklearn import decomposition
    from mr_gan_amd.pca import PCA
    X, k, p, tol = R.case(name)
    n, d = X.shape
    sk = decomposition.PCA(n_components=k, svd_solver='full').fit(X)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # no convergence warning
        pca = PCA(k, tol=tol).fit(X)
    _, _, _, _, mean32, C_dev = device_fit_parts(name)
    ref = R.fit(X, k)
    dC = np.linalg.norm(C_dev - ref['cov'], 2)
    resid = tol * pca.explained_variance_[0] + R.matvec_bound(C_dev)
    delta = R.gaps(ref['spectrum'], k)
    comp_bound = np.sqrt(2.0) * (resid + dC) / delta + 2 * U
    comp_err = np.linalg.norm(pca.components_ - sk.components_, axis=1)
    tight = comp_bound < 1.0                                   # beyond that the bound says nothing (not even the sign)
    print("PCA %s: %d products, |C_dev - C_64|_2 = %.3g, max comp err / bound = %.3g over %d of %d components"
          % (name, pca.n_iter_, dC, (comp_err[tight] / comp_bound[tight]).max(), tight.sum(), k))
    assert tight[:R.SEPARATED[name]].all()
    assert (comp_err[tight] <= comp_bound[tight]).all()
    # variances: Weyl on C_dev - C_64 plus the residual
    var_bound = resid + dC
    assert (np.abs(pca.explained_variance_ - sk.explained_variance_) <= var_bound).all()
    assert (np.abs(pca.singular_values_ ** 2 - sk.singular_values_ ** 2) <= var_bound * (n - 1)).all()
    total = sk.explained_variance_[0] / sk.explained_variance_ratio_[0]
    trace_bound = d * np.abs(C_dev - ref['cov']).max() + d * U64_SUM * total
    assert (np.abs(pca.explained_variance_ratio_ - sk.explained_variance_ratio_) <= (var_bound + trace_bound) / total * 1.01).all()
    assert abs(pca.noise_variance_ - sk.noise_variance_) <= (k * var_bound + trace_bound) / (min(n, d) - k)
    assert (np.abs(pca.mean_ - sk.mean_) <= R.mean_bound(X)).all() and pca.n_features_in_ == d
    # codes: the component error seen from the row, the product chain, and the mean's rounding
    Z, Zsk = pca.transform(X).astype(np.float64), sk.transform(X)
    code_bound = (np.linalg.norm(X - sk.mean_, axis=1)[:, None] * comp_bound[None, :] + np.linalg.norm(pca.mean_ - sk.mean_)
                  + R.chain_bound(X - pca.mean_.astype(np.float64), pca.components_.T, d))
    code_err = np.abs(Z - Zsk)
    print("PCA %s: max code err / bound = %.3g" % (name, (code_err[:, tight] / code_bound[:, tight]).max()))
    assert (code_err[:, tight] <= code_bound[:, tight]).all()


def test_mr_svm_with_pca_on_the_device():
    """mr_svm(pca=10, backend='hip') runs and returns the error of an RBFSVM fitted by hand on PCA codes, bit for bit (no
    accuracy claim against the CPU backend)"""
    from sklearn.utils import shuffle
    from mr_gan_amd.data import select_labeled, standard_scale
    from mr_gan_amd.mr_svm import mr_svm
    from mr_gan_amd.pca import PCA
    from mr_gan_amd.svm import RBFSVM
    X, y = R.six_classes()
    test = np.zeros(len(y), bool)
    test[np.arange(len(y)) % 6 == 5] = True                    # 10 rows of every class
    sets = [X[~test], X[test], y[~test], y[test]]
    got = mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=5, backend='hip', pca=10)
    rs = np.random.RandomState(5)
    Xtr, Xte = standard_scale(sets[0], sets[1])
    pca = PCA(10).fit(Xtr)
    Ztr, Zte = pca.transform(Xtr), pca.transform(Xte)
    Ztr, ytr = shuffle(Ztr, sets[2], random_state=rs)
    xl, yl, _ = select_labeled(Ztr, ytr, 20)
    want = 1.0 - RBFSVM(C=1.0, gamma='auto').fit(xl, yl).score(Zte, sets[3])
    print("mr_svm(pca=10): test error %.4f" % got)
    assert got == want and 0.0 <= got < 5.0 / 6.0
