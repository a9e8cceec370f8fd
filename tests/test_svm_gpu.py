"""The device SVM (csrc/svm.hip) on the GPU: the Gram kernel against fp64 under a bound derived from its operands, the SMO
solver through mrgan_svm_solve against its own optimality conditions and against libsvm, RBFSVM end to end against scikit-learn,
and mr_svm(backend='hip') on the harness."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svm_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                      # unit roundoff of float32
EXPF_ULP = 1.0                      # documented maximum error of the device expf (HIP math API: 1 ulp)


def _torch():
    import torch
    return torch


def _lib():
    from mr_gan_amd import engine as E
    return E.load_library()


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def to_dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# Gram
# ---------------------------------------------------------------------------------------------------------------------
def gram_bound(A, B, gamma):
    """per-element bound on |device - fp64| for K = expf(-gamma max(0, fl(fl(na + nb) - 2 dot))) with na, nb, dot k-ordered
    fmaf chains of length d (relative error gamma_d = d u / (1 - d u) of sum |terms|): pushed through exp, plus the expf error
    and one output rounding.  -> (fp64 values, bound)"""
    A, B = A.astype(np.float64), B.astype(np.float64)
    d, g = A.shape[1], float(gamma)
    gd = d * U / (1 - d * U)
    NA, NB, S = (A * A).sum(1)[:, None], (B * B).sum(1)[None, :], np.abs(A) @ np.abs(B).T
    d2 = np.maximum(NA + NB - 2.0 * (A @ B.T), 0.0)
    E = gd * (NA + NB + 2.0 * S)                 # the three chains
    E = E + U * (NA + NB + E)                    # fl(na + nb)
    E = E + U * (d2 + E)                         # the final fma rounds once; max(0, .) moves nothing away from d2 >= 0
    delta = g * E + U * g * (d2 + E)             # fl(-gamma d2)
    y = np.exp(-g * d2)
    bound = y * np.expm1(delta) + (2.0 * EXPF_ULP + 1.0) * U * y * np.exp(delta) + 2.0 ** -148 + 1e-14 * y
    return y, bound


def run_gram(A, B, gamma, ld_a=None, ld_b=None, ld_out=None, tile=None, same=False):
    """-> the m x n window, the whole padded output buffer"""
    torch, lib = _torch(), _lib()
    m, d = A.shape
    n = B.shape[0]
    ld_a, ld_b, ld_out = ld_a or d, ld_b or d, ld_out or n

    def padded(x, ld):
        buf = np.full((x.shape[0], ld), np.nan, np.float32)          # a read past the row's width poisons the result
        buf[:, :x.shape[1]] = x
        return to_dev(buf)
    a = padded(A, ld_a)
    b = a if same else padded(B, ld_b)
    out = torch.full((m + 1, ld_out), -7.0, dtype=torch.float32, device="cuda:0")
    args = [a.data_ptr(), ld_a, m, b.data_ptr(), ld_b, n, d, float(gamma), out.data_ptr(), ld_out]
    rc = lib.mrgan_svm_gram(*args, _stream()) if tile is None else lib.mrgan_debug_svm_gram(*args, tile, _stream())
    assert rc == 0, lib.mrgan_last_error()
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    return full[:m, :n].copy(), full


GRAM_SHAPES = [(1, 1, 1, False), (70, 70, 3, True), (64, 64, 16, False), (130, 97, 37, False)]


@pytest.mark.parametrize("m,n,d,sym", GRAM_SHAPES)
def test_gram_against_fp64(m, n, d, sym):
    rs = np.random.RandomState(100 + m + d)
    A = rs.randn(m, d).astype(np.float32)
    B = A if sym else rs.randn(n, d).astype(np.float32)
    gamma = np.float32(1.0 / d)
    got, full = run_gram(A, B, gamma, same=sym)
    want, bound = gram_bound(A, B, gamma)
    err = np.abs(got.astype(np.float64) - want)
    print("gram (%d, %d, %d): max err / bound = %.3f, max err = %.3g" % (m, n, d, (err / bound).max(), err.max()))
    assert (err <= bound).all()
    assert (full[m:] == -7.0).all()
    if sym:
        assert (got.view(np.uint32) == got.T.view(np.uint32)).all()
        assert (np.diag(got) == np.float32(1.0)).all()


def test_gram_pitches_tiles_and_symmetry():
    """(129, 129, 130): more than one block in each direction at both tile sizes, every pitch wider than its row, both tiles
    forced: the same bits, nothing written outside the window"""
    m = n = 129
    d = 130
    rs = np.random.RandomState(7)
    A = rs.randn(m, d).astype(np.float32)
    gamma = np.float32(1.0 / d)
    want, bound = gram_bound(A, A, gamma)
    outs = []
    for tile in (None, 64, 128):
        got, full = run_gram(A, A, gamma, ld_a=d + 3, ld_b=d + 3, ld_out=n + 5, tile=tile, same=True)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all()
        assert (full[:, n:] == -7.0).all() and (full[m:] == -7.0).all()
        assert (got.view(np.uint32) == got.T.view(np.uint32)).all() and (np.diag(got) == np.float32(1.0)).all()
        outs.append(got)
    assert (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all() and (outs[1].view(np.uint32) == outs[2].view(np.uint32)).all()
    # cross form with two different operand buffers and pitches, both tiles
    B = rs.randn(97, d).astype(np.float32)
    w2, b2 = gram_bound(A, B, gamma)
    x64, _ = run_gram(A, B, gamma, ld_a=d + 1, ld_b=d + 7, ld_out=97 + 2, tile=64)
    x128, _ = run_gram(A, B, gamma, ld_a=d + 1, ld_b=d + 7, ld_out=97 + 2, tile=128)
    assert (np.abs(x64.astype(np.float64) - w2) <= b2).all() and (x64.view(np.uint32) == x128.view(np.uint32)).all()


def test_gram_refuses_bad_arguments():
    torch, lib = _torch(), _lib()
    a = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    o = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    for gamma, ld_out in ((0.0, 4), (-1.0, 4), (float('nan'), 4), (1.0, 3)):
        assert lib.mrgan_svm_gram(a.data_ptr(), 4, 4, a.data_ptr(), 4, 4, 4, gamma, o.data_ptr(), ld_out, _stream()) < 0
        assert b"svm_gram" in lib.mrgan_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# solver through mrgan_svm_solve (the Gram matrix is made on the host: fp64, rounded to fp32)
# ---------------------------------------------------------------------------------------------------------------------
def run_solve(K32, cs, Cc=1.0, tol=1e-3, max_iter=10_000_000):
    torch, lib = _torch(), _lib()
    n, nc = K32.shape[0], len(cs) - 1
    pairs = nc * (nc - 1) // 2
    Kd = to_dev(K32.astype(np.float32))
    coef = torch.full((nc - 1, n), float('nan'), dtype=torch.float64, device="cuda:0")
    rho = torch.full((pairs,), float('nan'), dtype=torch.float64, device="cuda:0")
    iters = torch.full((pairs,), -1, dtype=torch.int32, device="cuda:0")
    arr = (C.c_int64 * (nc + 1))(*[int(v) for v in cs])
    rc = lib.mrgan_svm_solve(Kd.data_ptr(), Kd.stride(0), n, nc, arr, Cc, tol, max_iter, coef.data_ptr(), rho.data_ptr(),
                             iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, coef.cpu().numpy(), rho.cpu().numpy(), iters.cpu().numpy()


def blobs(sizes, d, dist, seed):
    """Gaussian classes whose centres lie about `dist` standard deviations apart -> float32 rows, labels, class_start"""
    rs = np.random.RandomState(seed)
    cen = rs.randn(len(sizes), d) * dist / np.sqrt(2 * d)
    x = np.concatenate([rs.randn(s, d) + cen[c] for c, s in enumerate(sizes)]).astype(np.float32)
    return x, np.repeat(np.arange(len(sizes)), sizes), np.concatenate([[0], np.cumsum(sizes)])


@functools.lru_cache(maxsize=None)
def solver_case(name):
    """-> labels, class_start, fp32-rounded Gram matrix, C"""
    if name == 'two_rows':
        x, y, cs = np.array([[0.0], [1.0]], np.float32), np.array([0, 1]), np.array([0, 1, 2])
        return y, cs, R.rbf_gram(x, x, 0.5).astype(np.float32), 1.0
    if name == 'bounded_heavy':          # 40 rows per class, gamma = 8 / d: about a quarter of libsvm's coefficients sit at C
        _, y, cs, K = R.mreo_labeled(16, 30, 40, 0.5, 8.0 / 16)
        return y, cs, K, 1.0
    sizes, d, dist, Cc, gamma, seed = {'unequal': ((7, 33), 5, 2.0, 1.0, 0.2, 1), 'single_row_class': ((9, 1, 14), 5, 2.0, 1.0, 0.2, 2),
                                      'pair_2048': ((1024, 1024), 8, 3.0, 1.0, 0.125, 3),
                                      'c100_all_free': ((20, 20, 20), 5, 4.0, 100.0, 0.2, 4)}[name]
    x, y, cs = blobs(sizes, d, dist, seed)
    return y, cs, R.rbf_gram(x, x, gamma).astype(np.float32), Cc


SOLVER_CASES = ['two_rows', 'unequal', 'single_row_class', 'pair_2048', 'c100_all_free', 'bounded_heavy']


def check_feasible(coef, cs, Cc):
    for i, j in R.ovo_pairs(len(cs) - 1):
        rows, y = R.pair_rows(cs, i, j)
        alpha = R.pair_alpha(coef, cs, i, j)
        assert np.isfinite(alpha).all() and (alpha >= 0).all() and (alpha <= Cc).all()
        assert abs((y * alpha).sum()) <= 64 * np.finfo(np.float64).eps * alpha.sum()


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_solver_optimality(name):
    """definition of done: the KKT gap, recomputed in fp64 from the returned coefficients and the Gram matrix, is below tol"""
    y, cs, K, Cc = solver_case(name)
    tol, max_iter = 1e-3, 10_000_000
    rc, coef, rho, iters = run_solve(K, cs, Cc, tol, max_iter)
    assert rc == 0, _lib().mrgan_last_error()
    assert np.isfinite(coef).all() and np.isfinite(rho).all()
    check_feasible(coef, cs, Cc)
    for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
        rows, yy = R.pair_rows(cs, i, j)
        Kp = K[np.ix_(rows, rows)]
        alpha = R.pair_alpha(coef, cs, i, j)
        gap = R.kkt_gap(Kp, yy, alpha, Cc)
        want_rho = R.calculate_rho(yy, R.gradient(Kp, yy, alpha), alpha, Cc)
        print("%s pair (%d, %d): gap / tol = %.4f, |rho - calculate_rho| = %.3g, iterations = %d, at C: %.0f %%"
              % (name, i, j, gap / tol, abs(rho[p] - want_rho), iters[p], 100 * np.mean(alpha[alpha > 0] >= Cc)))
        assert gap < tol * (1 + 1e-6)
        assert abs(rho[p] - want_rho) <= 1e-12
        assert 0 < iters[p] < max_iter
    if name == 'c100_all_free':
        assert np.abs(coef).max() < Cc


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_solver_matches_libsvm_at_tight_tolerance(name):
    """tol = 1e-8 on both sides: decisions from the device coefficients (fp64, on the training rows) within 1e-7 = 10 tol of
    SVC(kernel='precomputed'); the restatement sits at <= 0.95 tol, the factor covers another pivot order"""
    from sklearn.svm import SVC
    y, cs, K, Cc = solver_case(name)
    rc, coef, rho, iters = run_solve(K, cs, Cc, 1e-8)
    assert rc == 0 and (iters < 10_000_000).all()
    check_feasible(coef, cs, Cc)
    K64 = K.astype(np.float64)
    svc = SVC(kernel='precomputed', C=Cc, tol=1e-8, decision_function_shape='ovo').fit(K64, y)
    want = svc.decision_function(K64)
    if len(cs) == 3:
        want = -want[:, None]                # scikit-learn flips the sign of a two-class decision function; libsvm does not
    got = R.decisions(coef, rho, K64, cs)
    print("%s: max |dec - libsvm| = %.3g, iterations %s" % (name, np.abs(got - want).max(), iters.tolist()))
    assert np.abs(got - want).max() <= 1e-7


def test_solver_stops_at_max_iter_and_repeats_bit_for_bit():
    y, cs, K, Cc = solver_case('unequal')
    rc, coef, rho, iters = run_solve(K, cs, Cc, 1e-3, max_iter=5)
    assert rc == 0 and (iters == 5).all() and np.isfinite(rho).all()
    check_feasible(coef, cs, Cc)
    y, cs, K, Cc = solver_case('bounded_heavy')
    a, b = run_solve(K, cs, Cc), run_solve(K, cs, Cc)
    for u, v in zip(a[1:], b[1:]):
        assert u.tobytes() == v.tobytes()


def test_solver_refuses_bad_arguments():
    torch, lib = _torch(), _lib()
    n = 2049
    Kd = torch.ones((n, n), dtype=torch.float32, device="cuda:0")
    coef = torch.zeros((31, n), dtype=torch.float64, device="cuda:0")
    rho = torch.zeros(496, dtype=torch.float64, device="cuda:0")
    iters = torch.zeros(496, dtype=torch.int32, device="cuda:0")

    def call(nn, cs, Cc=1.0, tol=1e-3, max_iter=100):
        arr = (C.c_int64 * len(cs))(*cs)
        return lib.mrgan_svm_solve(Kd.data_ptr(), n, nn, len(cs) - 1, arr, Cc, tol, max_iter, coef.data_ptr(), rho.data_ptr(),
                                   iters.data_ptr(), _stream())
    assert call(2049, [0, 1024, 2049]) < 0 and b"MRGAN_SVM_MAX_PAIR" in lib.mrgan_last_error()      # a pair of 2049 rows
    assert call(10, [0, 10]) < 0                                      # one class
    assert call(40, list(range(34)) + [40]) < 0                       # 34 classes
    assert call(10, [0, 5, 5, 10]) < 0 and b"class" in lib.mrgan_last_error()      # an empty class
    assert call(10, [0, 5, 9]) < 0                                    # class_start does not end at n
    for kw in (dict(Cc=0.0), dict(Cc=-1.0), dict(tol=0.0), dict(max_iter=0), dict(Cc=float('nan'))):
        assert call(10, [0, 5, 10], **kw) < 0 and b"positive" in lib.mrgan_last_error()
    assert call(10, [0, 5, 10]) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# end to end through RBFSVM
# ---------------------------------------------------------------------------------------------------------------------
E2E_CASES = [(40, 20, 20, 3.0, 1.0), (37, 20, 24, 1.5, 1.0), (130, 30, 40, 1.0, 1.0), (37, 20, 24, 1.5, 100.0)]      # gamma = 1 / d


@functools.lru_cache(maxsize=None)
def e2e_data(d, trials, per, sep):
    from sklearn import preprocessing
    from mr_gan_amd import synthetic_mreo
    X, y, _ = synthetic_mreo(d=d, trials=trials, objects_per_class=4, sep=sep)
    tr = np.arange(len(y)) % 6 != 0
    sc = preprocessing.StandardScaler()
    a, b = sc.fit_transform(X[tr]), sc.transform(X[~tr])
    xl = np.concatenate([a[y[tr] == c][:per] for c in range(6)])
    return xl, np.repeat(np.arange(6), per), b, y[~tr]


@functools.lru_cache(maxsize=None)
def e2e_reference(d, trials, per, sep, Cc):
    """dec* of SVC at tol = 1e-8, its labels, and S = max |dec of SVC at tol = 1e-3 - dec*|: from scikit-learn alone"""
    from sklearn.svm import SVC
    xl, yl, xt, _ = e2e_data(d, trials, per, sep)
    tight = SVC(kernel='rbf', C=Cc, gamma=1.0 / d, tol=1e-8, decision_function_shape='ovo').fit(xl, yl)
    loose = SVC(kernel='rbf', C=Cc, gamma=1.0 / d, tol=1e-3, decision_function_shape='ovo').fit(xl, yl)
    dec = tight.decision_function(xt)
    return dec, tight.predict(xt), np.abs(loose.decision_function(xt) - dec).max()


@pytest.mark.parametrize("d,trials,per,sep,Cc", E2E_CASES)
def test_rbfsvm_against_scikit_learn(d, trials, per, sep, Cc):
    from mr_gan_amd import RBFSVM
    xl, yl, xt, yt = e2e_data(d, trials, per, sep)
    dec_ref, lab_ref, S = e2e_reference(d, trials, per, sep, Cc)
    clf = RBFSVM(C=Cc, gamma=1.0 / d, tol=1e-3).fit(xl, yl)
    dec = clf.decision_function(xt)
    lab = clf.predict(xt)
    err = np.abs(dec - dec_ref).max()
    sure = (np.abs(dec_ref) > 4 * S).all(1)
    print("RBFSVM (d %d, per %d, sep %g, C %g): max |dec - dec*| = %.3g = %.2f S (S = %.3g), rows left out %.2f %%, iterations <= %d"
          % (d, per, sep, Cc, err, err / S, S, 100 * (1 - sure.mean()), clf.n_iter_.max()))
    assert err <= 4 * S
    assert (lab[sure] == lab_ref[sure]).all()
    assert 1 - sure.mean() <= 0.05
    assert (clf.n_iter_ < clf.max_iter).all() and clf.classes_.tolist() == list(range(6))
    assert clf.dual_coef_dense_.shape == (5, len(yl)) and np.abs(clf.intercept_ - (-clf._rho.cpu().numpy())).max() == 0
    assert clf.score(xt, yt) == np.mean(lab == yt)
    # chunk edges change no bit
    for chunk in (1, 7):
        assert clf.decision_function(xt, chunk=chunk).tobytes() == dec.tobytes()
        assert (clf.predict(xt, chunk=chunk) == lab).all()


def test_rbfsvm_row_order_and_label_values_do_not_matter():
    """rows interleaved by class (the order inside every class kept: the sort is stable) and labels {3, 7, 9} give the bits of
    the sorted 0 / 1 / 2 problem; gamma='auto' is 1 / n_features"""
    from mr_gan_amd import RBFSVM
    xl, yl, xt, _ = e2e_data(37, 20, 24, 1.5)
    keep = yl < 3
    x, y = xl[keep], yl[keep]
    base = RBFSVM(gamma=1.0 / 37).fit(x, y)
    dec, lab = base.decision_function(xt), base.predict(xt)
    perm = np.argsort(np.arange(len(y)) % 24, kind='stable')         # class 0 row 0, class 1 row 0, class 2 row 0, class 0 row 1, ..
    assert (np.diff(y[perm]) != 0).all()
    mixed = RBFSVM(gamma='auto').fit(x[perm], np.array([3, 7, 9])[y[perm]])
    assert mixed.classes_.tolist() == [3, 7, 9]
    assert mixed.decision_function(xt).tobytes() == dec.tobytes()
    assert (mixed.predict(xt) == np.array([3, 7, 9])[lab]).all()
    assert mixed.dual_coef_dense_.tobytes() == base.dual_coef_dense_[:, perm].tobytes()
    assert mixed.intercept_.tobytes() == base.intercept_.tobytes() and (mixed.n_iter_ == base.n_iter_).all()


def test_rbfsvm_warns_at_max_iter():
    from mr_gan_amd import RBFSVM
    from mr_gan_amd.svm import SVMConvergenceWarning
    xl, yl, xt, _ = e2e_data(37, 20, 24, 1.5)
    with pytest.warns(SVMConvergenceWarning):
        clf = RBFSVM(gamma='auto', max_iter=3).fit(xl, yl)
    assert (clf.n_iter_ == 3).all() and clf.predict(xt).shape == (len(xt),)


def test_mr_svm_hip_backend_on_the_harness():
    """the sets of test_dataset.py::test_svm_baseline_and_its_tables: the hip backend's test error equals the scikit-learn
    backend's.  (Both misclassify the same one of the 240 test rows, row 93: the error is 1 / 240 on this problem, not 0.)"""
    from mr_gan_amd import synthetic_mreo
    from mr_gan_amd.mr_svm import mr_svm
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    tr = np.arange(len(y)) % 6 != 0
    sets = [X[tr], X[~tr], y[tr], y[~tr]]
    got = mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, backend='hip')
    want = mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, backend='sklearn')
    assert got == want and got == 1.0 - 239.0 / 240.0
