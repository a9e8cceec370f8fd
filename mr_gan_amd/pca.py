"""PCA pre-stage on the GPU: the other dimensionality reduction of the reference (others/wganlpctsemi.py:129-139, pcaScale:
decomposition.PCA(n_components=PCA) in front of every classifier of that file's grid), the classical baseline beside the
autoencoder's codes.

    pca = PCA(n_components=16).fit(X_train); Z_train, Z_test = pca.transform(X_train), pca.transform(X_test)
    Z_train, Z_test = pca_scale(X_train, X_test, PCA=10, scale='norm')          # pcaScale itself
    acc = mr_gan_pca(X, y, n_components=16)                                      # mr_gan_autoencoder on principal components

Four stages of csrc/pca.hip behind include/mrgan_abi.h: mrgan_pca_mean (fp64 column sums), mrgan_pca_covariance (the centred
fp32 covariance on the matrix cores), mrgan_pca_eig (the leading eigenpairs by block iteration, to a stated residual) and
mrgan_pca_transform / mrgan_pca_inverse_transform.  Unlike scikit-learn, which switches to a randomized solver above 1000
features, the fit is exact up to residuals_: |C w_i - lambda_i w_i|_2 <= tol * lambda_1 for the device's covariance C.  There is
no CPU path: without the library or a GPU every entry raises.  The numpy restatement the tests compare against lives in
tests/pca_ref.py.
Out of scope: whiten, n < d through the n x n Gram matrix, more than 4096 features, more than 64 components, grouped fits."""
import functools
import warnings

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.autoencoder import gan_on_codes
from mr_gan_amd.svm import _finite_matrix

BACKENDS = ('sklearn', 'hip')


class PCAConvergenceWarning(UserWarning):
    """the block iteration stopped at max_iter before the residuals reached tol (the role of SVMConvergenceWarning)"""


def block_width(n_components, d):
    """rows of the iterated block: min(d, n_components + MRGAN_PCA_GUARD)"""
    return min(int(d), int(n_components) + E.PCA_GUARD)


class PCA(E.DeviceCalls):
    """decomposition.PCA(n_components) on one MI355X, without whiten:

        PCA(n_components, tol=1e-6, max_iter=1000, random_state=0, device='cuda:0')

    fit(X) leaves components_ [k, d] (rows by descending variance, each with its largest-magnitude entry positive: scikit-learn's
    sign rule), explained_variance_, explained_variance_ratio_ (of the trace of the device's covariance), singular_values_,
    mean_, noise_variance_, n_iter_ (products of the block iteration), residuals_ (|C w_i - lambda_i w_i|_2) and n_features_in_.
    The iteration starts from RandomState(random_state).standard_normal((p, d)) and stops at max residual <= tol * lambda_1;
    reaching max_iter first raises a PCAConvergenceWarning.  A numerical rank below n_components is a ValueError."""
    _gpu_only = ('PCA', 'mrgan_pca_*')

    def __init__(self, n_components, tol=1e-6, max_iter=1000, random_state=0, device='cuda:0'):
        if int(n_components) != n_components or not 1 <= n_components <= E.PCA_MAX_COMPONENTS:
            raise ValueError("n_components must be an integer in [1, %d], got %r" % (E.PCA_MAX_COMPONENTS, n_components))
        if not (np.isfinite(tol) and tol > 0):
            raise ValueError("tol must be positive, got %r" % (tol,))
        if int(max_iter) != max_iter or not 1 <= max_iter < 2 ** 31:
            raise ValueError("max_iter must be an integer in [1, 2^31), got %r" % (max_iter,))
        self.n_components, self.tol, self.max_iter, self.random_state = int(n_components), float(tol), int(max_iter), random_state
        self.device = torch.device(device)
        self.times_ = {}                 # seconds of the last fit / transform per stage, filled only while time_stages is set
        self.time_stages = False
        self.components_ = None

    # ---- the stages on device tensors (float32, rows contiguous) ----
    def _empty(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _work(self, nbytes):
        return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=self.device)

    def mean_dev(self, x):
        mean = self._empty(x.shape[1])
        self._call("mrgan_pca_mean", x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], mean.data_ptr())
        return mean

    def covariance_dev(self, x, mean, out=None, tile=None, split=None):
        """the d x d covariance into `out` (a d-column window of a pitched tensor) or a new tensor; tile / split: the debug entry's
        forced block tile and row split"""
        n, d = x.shape
        cov = self._empty((d, d)) if out is None else out
        lib = E.load_library()
        if tile is None and split is None:
            work = self._work(lib.mrgan_pca_covariance_workspace_bytes(n, d))
            self._call("mrgan_pca_covariance", x.data_ptr(), x.stride(0), n, d, mean.data_ptr(), cov.data_ptr(), cov.stride(0),
                       work.data_ptr(), work.numel())
        else:
            work = self._work(lib.mrgan_debug_pca_covariance_workspace_bytes(n, d, tile or 0, split or 0))
            self._call("mrgan_debug_pca_covariance", x.data_ptr(), x.stride(0), n, d, mean.data_ptr(), cov.data_ptr(), cov.stride(0),
                       work.data_ptr(), work.numel(), tile or 0, split or 0)
        return cov

    def orthonormalize_dev(self, y):
        """the orthonormalisation stage alone: Y [p, d] -> (Q [p, d], Lambda [p] float64)"""
        p, d = y.shape
        work = self._work((2 * p * p + 3 * p + 2) * 8 + 2 * p * d * 4)
        q, lam = self._empty((p, d)), self._empty(p, torch.float64)
        self._call("mrgan_debug_pca_orthonormalize", y.data_ptr(), y.stride(0), p, d, work.data_ptr(), work.numel(), q.data_ptr(), q.stride(0),
                   lam.data_ptr())
        return q, lam

    def eig_dev(self, cov, q0=None, k=None):
        """the leading k eigenpairs of cov -> (components [k, d] on the device, values [k], residuals [k], products taken)"""
        d = cov.shape[0]
        k = self.n_components if k is None else int(k)
        p = block_width(k, d)
        if q0 is None:
            q0 = torch.from_numpy(np.random.RandomState(self.random_state).standard_normal((p, d)).astype(np.float32)).to(self.device)
        work = self._work(E.load_library().mrgan_pca_eig_workspace_bytes(d, k))
        w = self._empty((k, d))
        values, residuals, iters = np.zeros(k), np.zeros(k), np.zeros(1, np.int32)
        self._call("mrgan_pca_eig", cov.data_ptr(), cov.stride(0), d, k, q0.data_ptr(), q0.stride(0), p, self.tol, self.max_iter,
                   work.data_ptr(), work.numel(), w.data_ptr(), w.stride(0), values.ctypes.data, residuals.ctypes.data, iters.ctypes.data)
        return w, values, residuals, int(iters[0])

    def transform_dev(self, x, mean, w, out=None):
        out = self._empty((x.shape[0], w.shape[0])) if out is None else out
        self._call("mrgan_pca_transform", x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], mean.data_ptr(), w.data_ptr(), w.stride(0),
                   w.shape[0], out.data_ptr(), out.stride(0))
        return out

    def inverse_dev(self, z, mean, w, out=None):
        out = self._empty((z.shape[0], w.shape[1])) if out is None else out
        self._call("mrgan_pca_inverse_transform", z.data_ptr(), z.stride(0), z.shape[0], z.shape[1], w.data_ptr(), w.stride(0), w.shape[1],
                   mean.data_ptr(), out.data_ptr(), out.stride(0))
        return out

    # ---- the estimator ----
    def fit(self, X):
        X32 = _finite_matrix(X, "X")
        n, d = X32.shape
        if d > E.PCA_MAX_FEATURES:
            raise ValueError("X has %d features; the covariance is one d x d buffer of at most %d (MRGAN_PCA_MAX_FEATURES)" % (d, E.PCA_MAX_FEATURES))
        if not self.n_components <= min(n - 1, d):
            raise ValueError("n_components = %d must lie in [1, min(n_samples - 1, n_features, %d)] = [1, %d]"
                             % (self.n_components, E.PCA_MAX_COMPONENTS, min(n - 1, d, E.PCA_MAX_COMPONENTS)))
        self._require_gpu()
        self.times_ = {}
        self.components_ = None
        x = torch.from_numpy(X32).to(self.device)
        mean = self._timed('mean', lambda: self.mean_dev(x))
        cov = self._timed('covariance', lambda: self.covariance_dev(x, mean))
        try:
            w, values, residuals, iters = self._timed('eig', lambda: self.eig_dev(cov))
        except E.MrganError as e:
            if e.code == E.PCA_RANK_DEFICIENT:
                raise ValueError("PCA: the numerical rank of the data is below n_components = %d (%s)" % (self.n_components, e)) from None
            raise
        total = float(torch.diagonal(cov).double().sum())
        self._mean, self._w = mean, w
        self.mean_, self.components_ = mean.cpu().numpy(), w.cpu().numpy()
        self.explained_variance_, self.residuals_, self.n_iter_ = values, residuals, iters
        self.explained_variance_ratio_ = values / total
        self.singular_values_ = np.sqrt(values * (n - 1))
        rest = min(n, d) - self.n_components             # scikit-learn: the mean of the remaining min(n, d) - k variances
        self.noise_variance_ = (total - values.sum()) / rest if rest > 0 else 0.0
        self.n_features_in_, self.n_samples_ = d, n
        if residuals.max() > self.tol * values.max():
            warnings.warn("PCA: the block iteration stopped at max_iter = %d with residual %.3g > tol * lambda_1 = %.3g"
                          % (self.max_iter, residuals.max(), self.tol * values.max()), PCAConvergenceWarning, stacklevel=2)
        return self

    def _rows(self, X, name, width_in, width_out, chunk, fn):
        """fn(rows on the device, their window of the output) over chunks of `chunk` rows of X -> the output on the host"""
        if self.components_ is None:
            raise RuntimeError("PCA: fit() first")
        X32 = _finite_matrix(X, name, width_in(self))
        if chunk is None:
            chunk = 4096
        if int(chunk) != chunk or chunk < 1:
            raise ValueError("chunk must be a positive integer, got %r" % (chunk,))
        self._require_gpu()
        out = self._empty((X32.shape[0], width_out(self)))

        def run():
            # every row's values depend on that row alone: chunk edges change no bit
            for r0 in range(0, X32.shape[0], int(chunk)):
                fn(torch.from_numpy(X32[r0:r0 + int(chunk)]).to(self.device), out[r0:r0 + int(chunk)])
        self._timed('transform', run)
        return out.cpu().numpy()

    def transform(self, X, chunk=None):
        """(X - mean_) components_^T -> [rows, n_components] float32, worked in chunks of `chunk` rows (default 4096)"""
        return self._rows(X, "X", lambda s: s.n_features_in_, lambda s: s.n_components, chunk,
                          lambda x, out: self.transform_dev(x, self._mean, self._w, out))

    def fit_transform(self, X):
        return self.fit(X).transform(X)

    def inverse_transform(self, Z, chunk=None):
        """Z components_ + mean_ -> [rows, n_features] float32"""
        return self._rows(Z, "Z", lambda s: s.n_components, lambda s: s.n_features_in_, chunk,
                          lambda z, out: self.inverse_dev(z, self._mean, self._w, out))


def _device_pca(n_components, **kw):
    return PCA(n_components, **kw)                     # (pca_scale's own argument is called PCA, as the reference's is)


def pca_scale(X_train, X_test, PCA=0, scale=None, backend='hip'):
    """pcaScale of others/wganlpctsemi.py:129-139: PCA > 0 fits that many components on the training rows and applies them to
    both sets (backend 'hip': the device PCA of this module; 'sklearn': decomposition.PCA(svd_solver='full') on the CPU), then
    scale == 'norm' -> the row Normalizer, any other scale that is not None -> StandardScaler fitted on the training rows
    (both on the host) -> (X_train, X_test)"""
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s, got %r" % (BACKENDS, backend))
    n_components = PCA
    if n_components > 0:
        if backend == 'hip':
            pca = _device_pca(n_components)
        else:
            from sklearn import decomposition
            pca = decomposition.PCA(n_components=n_components, svd_solver='full')
        X_train = pca.fit_transform(X_train)
        X_test = pca.transform(X_test)
    if scale is not None:
        from sklearn import preprocessing
        scaler = preprocessing.Normalizer() if scale == 'norm' else preprocessing.StandardScaler()
        X_train = scaler.fit_transform(X_train)
        X_test = scaler.transform(X_test)
    return X_train, X_test


def pca_transform_hook(n_components, backend):
    """the prologue's transform= for mr_svm(pca=): None for 0, else pcaScale without a scaler"""
    if int(n_components) != n_components or n_components < 0:
        raise ValueError("pca must be a non-negative integer (0: no PCA), got %r" % (n_components,))
    return functools.partial(pca_scale, PCA=int(n_components), backend=backend) if n_components else None


def mr_gan_pca(X, y, percentlabeled=50, percentunlabeled=None, epochs=100, trainTestSets=None, n_components=16, verbose=False,
               batch_size=50, dtype='float32', seed=None, device='cuda:0', noise='irwin-hall', num_classes=None, tol=1e-6, max_iter=1000):
    """mr_gan_autoencoder with principal components in place of the autoencoder's codes: split and standard-scale, fit PCA on
    X_train, replace both sets by their n_components-wide codes (not rescaled), then the unchanged GAN training on the codes.
    Returns the test ACCURACY, as mr_gan_autoencoder does, and prints the same shape line."""
    E.noise_flags(noise)                                           # an unknown value fails before any data is touched

    def codes(X_train, X_test, rs):
        pca = PCA(n_components, tol=tol, max_iter=max_iter, random_state=int(rs.randint(1 << 31)), device=device)
        return pca.fit_transform(X_train), pca.transform(X_test)
    return gan_on_codes(codes, X, y, percentlabeled, percentunlabeled, epochs, trainTestSets, verbose, batch_size, dtype, seed, device,
                        noise, num_classes)
