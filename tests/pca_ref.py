"""float64 restatement of the PCA pre-stage (mr_gan_amd/pca.py, csrc/pca.hip), the rounding bounds its tests assert, and the
designed cases they run on.  Nothing here imports the package or touches a device."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
U64 = 2.0 ** -53


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def mean(X):
    return np.asarray(X, np.float64).mean(axis=0)


def covariance(X, mu):
    """(X - mu)^T (X - mu) / (n - 1) for the GIVEN mu (the device subtracts the float32 mean it is handed)"""
    Xc = np.asarray(X, np.float64) - np.asarray(mu, np.float64)
    return Xc.T @ Xc / (len(Xc) - 1)


def sign_rule(W):
    """each row's largest-magnitude entry positive, first index on ties: scikit-learn's svd_flip(u_based_decision=False)"""
    W = np.array(W, np.float64)
    at = np.argmax(np.abs(W), axis=1)
    s = np.sign(W[np.arange(len(W)), at])
    s[s == 0] = 1.0
    return W * s[:, None]


def spectrum(C):
    """all eigenpairs of the symmetric C, descending: (values [d], vectors as ROWS [d, d])"""
    lam, V = np.linalg.eigh(np.asarray(C, np.float64))
    return lam[::-1].copy(), V[:, ::-1].T.copy()


def fit(X, k):
    """what decomposition.PCA(n_components=k, svd_solver='full').fit(X) leaves, by the covariance route"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    mu = mean(X)
    C = covariance(X, mu)
    lam, V = spectrum(C)
    lam = np.maximum(lam, 0.0)
    rest = min(n, d) - k
    return dict(mean=mu, cov=C, spectrum=lam, components=sign_rule(V[:k]), explained_variance=lam[:k],
                explained_variance_ratio=lam[:k] / lam.sum(), singular_values=np.sqrt(lam[:k] * (n - 1)),
                noise_variance=lam[k:min(n, d)].mean() if rest > 0 else 0.0)


def transform(X, mu, W):
    return (np.asarray(X, np.float64) - np.asarray(mu, np.float64)) @ np.asarray(W, np.float64).T


def inverse_transform(Z, mu, W):
    return np.asarray(Z, np.float64) @ np.asarray(W, np.float64) + np.asarray(mu, np.float64)


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def chain_bound(A, B, L):
    """a length-L float32 product chain sum_k a_k b_k (one rounding per fused step) on operands that carry one rounding each
    errs by at most (L + 2) u sum |a||b|: |A| @ |B| scaled, elementwise for the matrix product A @ B"""
    return (L + 2) * U * (np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)))


def matvec_bound(C):
    """|fl(C q) - C q|_2 <= (d + 2) u |C|_F for a unit q"""
    C = np.asarray(C, np.float64)
    return (C.shape[0] + 2) * U * np.linalg.norm(C)


def mean_bound(X):
    """the float64 sum of n terms in any order, divided and rounded once to float32"""
    X = np.asarray(X, np.float64)
    return U * np.abs(X.mean(axis=0)) + (len(X) + 1) * U64 * np.abs(X).mean(axis=0) + 1e-45


def sine(w, v):
    """sin of the angle between w and the unit vector v, without cancellation"""
    w, v = np.asarray(w, np.float64), np.asarray(v, np.float64)
    return np.linalg.norm(w - v * (v @ w)) / np.linalg.norm(w)


def gaps(lam, k):
    """delta_i, i < k: the distance of lam[i] from the rest of the spectrum lam"""
    lam = np.asarray(lam, np.float64)
    return np.array([np.abs(np.delete(lam, i) - lam[i]).min() for i in range(k)])


def gaps_from(theta, lam):
    """delta_i: the distance of theta[i] from the spectrum lam without its i-th value"""
    lam = np.asarray(lam, np.float64)
    return np.array([np.abs(np.delete(lam, i) - t).min() for i, t in enumerate(theta)])


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def designed(n, d, r, decay, seed, floor=2e-3, offset=3.0):
    """X = U diag(s) V^T + floor * noise + offset with s_j = sqrt(n - 1) decay^j, U [n, r] orthonormal and orthogonal to the ones
    vector, V [d, r] orthonormal: the covariance has the eigenvalues decay^(2 j), j < r, over a floor of about floor^2.  Returned as
    float32-representable float64, so every reader sees the same numbers."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, r))
    Uo, _ = np.linalg.qr(A - A.mean(axis=0))
    Vo, _ = np.linalg.qr(rng.standard_normal((d, r)))
    s = np.sqrt(n - 1.0) * decay ** np.arange(r)
    X = (Uo * s) @ Vo.T + floor * rng.standard_normal((n, d)) + offset * rng.standard_normal(d)
    return X.astype(np.float32).astype(np.float64)


def plain(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * (1.0 + np.arange(d) % 3) + rng.standard_normal(d)).astype(np.float32).astype(np.float64)


# name -> (X builder, k, p, tol).  A - C have a designed spectrum; D: the block is the whole space; E: rank 11 < p, the guard
# directions collapse; F: rank 7 < k, the rank error.  tol of D - F is this file's choice (fp32 residuals sit near 1e-7 lambda_1).
CASES = {
    'A': (lambda: designed(301, 97, 50, 0.9, 11), 12, 28, 1e-5),
    'B': (lambda: designed(600, 160, 60, 0.93, 12), 10, 26, 1e-6),
    'C': (lambda: designed(600, 160, 60, 0.93, 12), 64, 80, 1e-5),
    'D': (lambda: plain(40, 20, 14), 10, 20, 1e-5),
    'E': (lambda: plain(12, 97, 15), 10, 26, 1e-5),
    'F': (lambda: plain(8, 97, 16), 10, 26, 1e-5),
}
# the leading eigenvalues of a case whose separation the design guarantees: min gap >= 100 tol lambda_1.  C asks for 64 of a
# rank-60 design with lambda_j = 0.93^(2 j): from j = 34 on the gaps 0.135 lambda_j fall below 100 tol lambda_1 = 1e-3, so only the
# first 34 can be (and are) separated; the per-pair bounds of the GPU tests hold for any gap.
SEPARATED = {'A': 12, 'B': 10, 'C': 34}

_cache = {}


def case(name):
    """-> (X float64 of float32 values, k, p, tol), built once"""
    if name not in _cache:
        build, k, p, tol = CASES[name]
        X = build()
        X.setflags(write=False)
        _cache[name] = (X, k, p, tol)
    return _cache[name]


def six_classes(n_per_class=60, d=97, seed=21):
    """a 6-class designed set: class centres on a low-rank designed spectrum -> X [6 n_per_class, d], y"""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((6, d))
    y = np.repeat(np.arange(6), n_per_class)
    X = centres[y] + designed(6 * n_per_class, d, 30, 0.9, seed + 1, floor=1e-2, offset=0.0)
    return X.astype(np.float32).astype(np.float64), y
