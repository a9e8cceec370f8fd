"""The linear kernel and nu-SVC of the device SVM (csrc/svm.hip) on the GPU: the linear Gram kernel against fp64 under a bound
derived from its operands, the nu solver through mrgan_svm_solve_nu against its own optimality conditions and against libsvm,
KernelSVM end to end against scikit-learn's SVC / NuSVC, and mr_svm(backend='hip', classifier=...) on the harness."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svm_kinds_ref as N
from tests import svm_ref as R
from tests.test_svm_gpu import E2E_CASES, GRAM_SHAPES, U, _lib, _stream, _torch, e2e_data, solver_case, to_dev

pytestmark = pytest.mark.gpu
RBF, LINEAR = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# linear Gram
# ---------------------------------------------------------------------------------------------------------------------
def linear_bound(A, B):
    """per-element bound on |device - fp64| for a k-ordered fp32 chain of d fused multiply-adds: gamma_d sum_k |a_k b_k| with
    gamma_d = d u / (1 - d u) (Higham, Accuracy and Stability, eq. 3.5), plus fp32's smallest subnormal for a sum that
    underflows.  -> (fp64 values, bound)"""
    d = A.shape[1]
    S = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    return N.linear_gram(A, B), d * U / (1 - d * U) * S + 2.0 ** -149


def run_kernel_matrix(kind, A, B, gamma=1.0, ld_a=None, ld_b=None, ld_out=None, tile=None, same=False):
    """test_svm_gpu.run_gram through mrgan_svm_kernel_matrix -> the m x n window, the whole padded output buffer"""
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
    args = [kind, a.data_ptr(), ld_a, m, b.data_ptr(), ld_b, n, d, float(gamma), out.data_ptr(), ld_out]
    rc = lib.mrgan_svm_kernel_matrix(*args, _stream()) if tile is None else lib.mrgan_debug_svm_kernel_matrix(*args, tile, _stream())
    assert rc == 0, lib.mrgan_last_error()
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    return full[:m, :n].copy(), full


@pytest.mark.parametrize("m,n,d,sym", GRAM_SHAPES)
def test_linear_gram_against_fp64(m, n, d, sym):
    rs = np.random.RandomState(100 + m + d)
    A = rs.randn(m, d).astype(np.float32)
    B = A if sym else rs.randn(n, d).astype(np.float32)
    got, full = run_kernel_matrix(LINEAR, A, B, gamma=float('nan'), same=sym)          # gamma is ignored
    want, bound = linear_bound(A, B)
    err = np.abs(got.astype(np.float64) - want)
    print("linear gram (%d, %d, %d): max err / bound = %.3f, max err = %.3g" % (m, n, d, (err / bound).max(), err.max()))
    assert (err <= bound).all()
    assert (full[m:] == -7.0).all()
    if sym:
        assert (got.view(np.uint32) == got.T.view(np.uint32)).all()


def test_linear_gram_pitches_tiles_and_symmetry():
    """(129, 129, 130): more than one block in each direction at both tile sizes, every pitch wider than its row, both tiles
    forced: the same bits, nothing written outside the window"""
    m = n = 129
    d = 130
    rs = np.random.RandomState(7)
    A = rs.randn(m, d).astype(np.float32)
    want, bound = linear_bound(A, A)
    outs = []
    for tile in (None, 64, 128):
        got, full = run_kernel_matrix(LINEAR, A, A, ld_a=d + 3, ld_b=d + 3, ld_out=n + 5, tile=tile, same=True)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all()
        assert (full[:, n:] == -7.0).all() and (full[m:] == -7.0).all()
        assert (got.view(np.uint32) == got.T.view(np.uint32)).all()
        outs.append(got)
    assert (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all() and (outs[1].view(np.uint32) == outs[2].view(np.uint32)).all()
    B = rs.randn(97, d).astype(np.float32)
    w2, b2 = linear_bound(A, B)
    x64, _ = run_kernel_matrix(LINEAR, A, B, ld_a=d + 1, ld_b=d + 7, ld_out=97 + 2, tile=64)
    x128, _ = run_kernel_matrix(LINEAR, A, B, ld_a=d + 1, ld_b=d + 7, ld_out=97 + 2, tile=128)
    assert (np.abs(x64.astype(np.float64) - w2) <= b2).all() and (x64.view(np.uint32) == x128.view(np.uint32)).all()


@pytest.mark.parametrize("m,n,d,sym", GRAM_SHAPES)
def test_rbf_kind_is_mrgan_svm_gram_bit_for_bit(m, n, d, sym):
    from tests.test_svm_gpu import run_gram
    rs = np.random.RandomState(100 + m + d)
    A = rs.randn(m, d).astype(np.float32)
    B = A if sym else rs.randn(n, d).astype(np.float32)
    gamma = np.float32(1.0 / d)
    for tile in (None, 64, 128):
        old, old_full = run_gram(A, B, gamma, ld_out=n + 3, tile=tile, same=sym)
        new, new_full = run_kernel_matrix(RBF, A, B, gamma, ld_out=n + 3, tile=tile, same=sym)
        assert old_full.tobytes() == new_full.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# nu solver through mrgan_svm_solve_nu (the Gram matrix is made on the host: fp64, rounded to fp32)
# ---------------------------------------------------------------------------------------------------------------------
def run_solve_nu(K32, cs, nu, tol=1e-3, max_iter=10_000_000, want_r=True):
    torch, lib = _torch(), _lib()
    n, nc = K32.shape[0], len(cs) - 1
    pairs = nc * (nc - 1) // 2
    Kd = to_dev(K32.astype(np.float32))
    coef = torch.full((nc - 1, n), float('nan'), dtype=torch.float64, device="cuda:0")
    rho = torch.full((pairs,), float('nan'), dtype=torch.float64, device="cuda:0")
    r = torch.full((pairs,), float('nan'), dtype=torch.float64, device="cuda:0")
    iters = torch.full((pairs,), -1, dtype=torch.int32, device="cuda:0")
    arr = (C.c_int64 * (nc + 1))(*[int(v) for v in cs])
    rc = lib.mrgan_svm_solve_nu(Kd.data_ptr(), Kd.stride(0), n, nc, arr, nu, tol, max_iter, coef.data_ptr(), rho.data_ptr(),
                                r.data_ptr() if want_r else None, iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, coef.cpu().numpy(), rho.cpu().numpy(), r.cpu().numpy(), iters.cpu().numpy()


def pair_alpha_nu(coef, cs, i, j, r):
    """the pair's alpha out of coef = fl(alpha fl(y / r)): coef r carries two roundings, so a variable at the bound 1 comes back
    within 2 units of 2^-53 of it; those are put back on the bound (the solver's own test is alpha >= 1)"""
    alpha = R.pair_alpha(coef, cs, i, j) * r
    return np.where(np.abs(alpha - 1.0) <= 4 * 2.0 ** -53, 1.0, alpha)


def check_feasible_nu(coef, r, cs, nu):
    for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
        rows, y = R.pair_rows(cs, i, j)
        alpha = pair_alpha_nu(coef, cs, i, j, r[p])
        assert np.isfinite(alpha).all() and (alpha >= 0).all() and (alpha <= 1).all()
        want = nu * len(y) / 2
        for sign in (1.0, -1.0):
            # every alpha carries the two roundings of coef r, and the updates keep a sign's sum to one rounding each
            assert abs(alpha[y == sign].sum() - want) <= 64 * np.finfo(np.float64).eps * want


NU_CASES = [('two_rows', 0.5), ('unequal', 0.1), ('unequal', 0.3), ('single_row_class', 0.1), ('pair_2048', 0.5),
            ('c100_all_free', 0.1), ('bounded_heavy', 0.5)]


@pytest.mark.parametrize("name,nu", NU_CASES)
def test_nu_solver_optimality(name, nu):
    """definition of done: Solver_NU's stopping quantity, recomputed in fp64 from the returned coefficients times r and the Gram
    matrix, is below tol; rho and r are calculate_rho of the returned point"""
    y, cs, K, _ = solver_case(name)
    tol, max_iter = 1e-3, 10_000_000
    rc, coef, rho, r, iters = run_solve_nu(K, cs, nu, tol, max_iter)
    assert rc == 0, _lib().mrgan_last_error()
    assert np.isfinite(coef).all() and np.isfinite(rho).all() and (r > 0).all()
    check_feasible_nu(coef, r, cs, nu)
    for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
        rows, yy = R.pair_rows(cs, i, j)
        Kp = K[np.ix_(rows, rows)]
        alpha = pair_alpha_nu(coef, cs, i, j, r[p])
        gap = N.nu_kkt_gap(Kp, yy, alpha)
        want_rho, want_r = N.nu_calculate_rho(yy, N.nu_gradient(Kp, yy, alpha), alpha)
        print("%s nu %g pair (%d, %d): gap / tol = %.4f, |rho r - calculate_rho| = %.3g, |r - r'| = %.3g, iterations = %d, at 1: %.0f %%"
              % (name, nu, i, j, gap / tol, abs(rho[p] * r[p] - want_rho), abs(r[p] - want_r), iters[p],
                 100 * np.mean(alpha[alpha > 0] >= 1)))
        assert gap < tol * (1 + 1e-6)
        assert abs(rho[p] * r[p] - want_rho) <= 1e-12 and abs(r[p] - want_r) <= 1e-12
        assert 0 <= iters[p] < max_iter
        if name == 'two_rows':
            assert iters[p] == 0                      # the start point (0.5, 0.5) is the optimum


# max |dec - libsvm| of the fp64 restatement (tests/svm_kinds_ref.py), measured on the CPU against NuSVC(kernel='precomputed',
# tol=1e-8) -- tests/test_svm_kinds_cpu.py prints them
RESTATEMENT_VS_LIBSVM = {('two_rows', 0.5): 0.0, ('unequal', 0.1): 1.11e-15, ('unequal', 0.3): 5.69e-9, ('single_row_class', 0.1): 1.52e-8,
                         ('pair_2048', 0.5): 8.88e-15, ('c100_all_free', 0.1): 1.0e-7, ('bounded_heavy', 0.5): 1.33e-15}


@pytest.mark.parametrize("name,nu", NU_CASES)
def test_nu_solver_matches_libsvm_at_tight_tolerance(name, nu):
    """tol = 1e-8 on both sides: decisions from the device coefficients (fp64, on the training rows) against
    NuSVC(kernel='precomputed').  nu decisions carry a factor 1 / r, so C-SVC's 1e-7 does not transfer; the bound is four times
    what the fp64 restatement shows against libsvm on the same case, measured on the CPU:

        two_rows 0.5: 0          unequal 0.1: 1.11e-15     unequal 0.3: 5.69e-9      single_row_class 0.1: 1.52e-8
        pair_2048 0.5: 8.88e-15  c100_all_free 0.1: 1.0e-7  bounded_heavy 0.5: 1.33e-15

    The values of 1e-15 and the 0 say that the restatement walks libsvm's pivots with libsvm's roundings; the device solver keeps
    fp64 contraction off and sums in libsvm's order to do the same."""
    from sklearn.svm import NuSVC
    y, cs, K, _ = solver_case(name)
    rc, coef, rho, r, iters = run_solve_nu(K, cs, nu, 1e-8)
    assert rc == 0 and (iters < 10_000_000).all()
    check_feasible_nu(coef, r, cs, nu)
    K64 = K.astype(np.float64)
    svc = NuSVC(kernel='precomputed', nu=nu, tol=1e-8, decision_function_shape='ovo').fit(K64, y)
    want = svc.decision_function(K64)
    if len(cs) == 3:
        want = -want[:, None]                # scikit-learn flips the sign of a two-class decision function; libsvm does not
    got = R.decisions(coef, rho, K64, cs)
    ref = N.solve_ovo_nu(K, cs, nu, 1e-8)
    print("%s nu %g: max |dec - libsvm| = %.3g (restatement %.3g), iterations %s, restatement's %s, max |coef - restatement| = %.3g"
          % (name, nu, np.abs(got - want).max(), RESTATEMENT_VS_LIBSVM[name, nu], iters.tolist(), ref[3].tolist(), np.abs(coef - ref[0]).max()))
    assert np.abs(got - want).max() <= 4 * RESTATEMENT_VS_LIBSVM[name, nu]


def test_nu_solver_stops_at_max_iter_and_repeats_bit_for_bit():
    y, cs, K, _ = solver_case('unequal')
    rc, coef, rho, r, iters = run_solve_nu(K, cs, 0.3, 1e-3, max_iter=5)
    assert rc == 0 and (iters == 5).all() and np.isfinite(rho).all() and np.isfinite(r).all()
    check_feasible_nu(coef, r, cs, 0.3)
    y, cs, K, _ = solver_case('bounded_heavy')
    a, b = run_solve_nu(K, cs, 0.5), run_solve_nu(K, cs, 0.5)
    for u, v in zip(a[1:], b[1:]):
        assert u.tobytes() == v.tobytes()
    # r_dev is optional and changes nothing else
    c = run_solve_nu(K, cs, 0.5, want_r=False)
    assert c[0] == 0 and c[1].tobytes() == a[1].tobytes() and c[2].tobytes() == a[2].tobytes() and np.isnan(c[3]).all()


def test_new_entries_refuse_bad_arguments():
    torch, lib = _torch(), _lib()
    n = 2049
    Kd = torch.ones((n, n), dtype=torch.float32, device="cuda:0")
    coef = torch.zeros((31, n), dtype=torch.float64, device="cuda:0")
    rho = torch.zeros(496, dtype=torch.float64, device="cuda:0")
    r = torch.zeros(496, dtype=torch.float64, device="cuda:0")
    iters = torch.zeros(496, dtype=torch.int32, device="cuda:0")

    def call(nn, cs, nu=0.5, tol=1e-3, max_iter=100):
        arr = (C.c_int64 * len(cs))(*cs)
        return lib.mrgan_svm_solve_nu(Kd.data_ptr(), n, nn, len(cs) - 1, arr, nu, tol, max_iter, coef.data_ptr(), rho.data_ptr(),
                                      r.data_ptr(), iters.data_ptr(), _stream())
    # class sizes (20, 7, 33): nu (n_i + n_j) / 2 = 6.75 <= 7, 13.25 <= 20, but 10 > 7 for the classes 1 and 2; the message names them
    assert call(60, [0, 20, 27, 60]) < 0
    msg = lib.mrgan_last_error()
    assert b"nu is infeasible" in msg and b"classes 1 and 2" in msg
    assert call(40, [0, 7, 40], nu=0.1) == 0
    for nu in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        assert call(10, [0, 5, 10], nu=nu) < 0 and b"nu must lie in (0, 1]" in lib.mrgan_last_error()
    # the existing argument errors
    assert call(2049, [0, 1024, 2049]) < 0 and b"MRGAN_SVM_MAX_PAIR" in lib.mrgan_last_error()      # a pair of 2049 rows
    assert call(10, [0, 10]) < 0                                      # one class
    assert call(40, list(range(34)) + [40]) < 0                       # 34 classes
    assert call(10, [0, 5, 5, 10]) < 0 and b"class" in lib.mrgan_last_error()      # an empty class
    assert call(10, [0, 5, 9]) < 0                                    # class_start does not end at n
    for kw in (dict(tol=0.0), dict(max_iter=0), dict(tol=float('nan'))):
        assert call(10, [0, 5, 10], **kw) < 0 and b"positive" in lib.mrgan_last_error()
    assert lib.mrgan_svm_solve_nu(None, n, 10, 2, (C.c_int64 * 3)(0, 5, 10), 0.5, 1e-3, 100, coef.data_ptr(), rho.data_ptr(), None,
                                  iters.data_ptr(), _stream()) < 0 and b"null" in lib.mrgan_last_error()
    assert call(10, [0, 5, 10]) == 0
    # the kernel matrix: an unknown kind, and mrgan_svm_gram's errors; gamma is checked for RBF only
    a = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    o = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")

    def km(kind, gamma=1.0, ld_out=4):
        return lib.mrgan_svm_kernel_matrix(kind, a.data_ptr(), 4, 4, a.data_ptr(), 4, 4, 4, gamma, o.data_ptr(), ld_out, _stream())
    for kind in (2, -1):
        assert km(kind) < 0 and b"unknown kernel kind" in lib.mrgan_last_error()
    for gamma, ld_out in ((0.0, 4), (-1.0, 4), (float('nan'), 4), (1.0, 3)):
        assert km(RBF, gamma, ld_out) < 0 and b"svm_gram" in lib.mrgan_last_error()
    assert km(LINEAR, 1.0, 3) < 0 and b"pitch" in lib.mrgan_last_error()
    assert km(LINEAR, 0.0) == 0 and km(RBF) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# end to end through KernelSVM
# ---------------------------------------------------------------------------------------------------------------------
LINEAR_C_CASES = [(130, 30, 40, 2.0, 1.0), (130, 30, 40, 1.0, 0.01), (37, 20, 24, 1.5, 0.01)]
KIND_CASES = ([('linear', None) + c for c in LINEAR_C_CASES]
              + [(kernel, nu) + c[:4] + (1.0,) for kernel in ('rbf', 'linear') for nu in (0.5, 0.2) for c in E2E_CASES[:3]])


@functools.lru_cache(maxsize=None)
def kinds_reference(kernel, nu, d, trials, per, sep, Cc):
    """dec* of scikit-learn's classifier at tol = 1e-8, its labels, and S = max |dec at tol = 1e-3 - dec*|: from scikit-learn alone"""
    from sklearn.svm import SVC, NuSVC
    xl, yl, xt, _ = e2e_data(d, trials, per, sep)

    def make(tol):
        kw = dict(kernel=kernel, gamma=1.0 / d, tol=tol, decision_function_shape='ovo')
        return (SVC(C=Cc, **kw) if nu is None else NuSVC(nu=nu, **kw)).fit(xl, yl)
    tight, loose = make(1e-8), make(1e-3)
    dec = tight.decision_function(xt)
    return dec, tight.predict(xt), np.abs(loose.decision_function(xt) - dec).max()


@pytest.mark.parametrize("kernel,nu,d,trials,per,sep,Cc", KIND_CASES)
def test_kernelsvm_against_scikit_learn(kernel, nu, d, trials, per, sep, Cc):
    from mr_gan_amd import KernelSVM
    xl, yl, xt, yt = e2e_data(d, trials, per, sep)
    dec_ref, lab_ref, S = kinds_reference(kernel, nu, d, trials, per, sep, Cc)
    clf = KernelSVM(kernel=kernel, nu=nu, C=Cc, gamma=1.0 / d, tol=1e-3).fit(xl, yl)
    dec = clf.decision_function(xt)
    lab = clf.predict(xt)
    err = np.abs(dec - dec_ref).max()
    sure = (np.abs(dec_ref) > 4 * S).all(1)
    print("KernelSVM %s nu %s (d %d, per %d, sep %g, C %g): max |dec - dec*| = %.3g = %.2f S (S = %.3g), rows left out %.2f %%, iterations <= %d"
          % (kernel, nu, d, per, sep, Cc, err, err / S, S, 100 * (1 - sure.mean()), clf.n_iter_.max()))
    assert err <= 4 * S
    assert (lab[sure] == lab_ref[sure]).all()
    assert 1 - sure.mean() <= 0.05
    assert (clf.n_iter_ < clf.max_iter).all() and clf.classes_.tolist() == list(range(6))
    assert clf.dual_coef_dense_.shape == (5, len(yl)) and np.abs(clf.intercept_ - (-clf._rho.cpu().numpy())).max() == 0
    assert clf.score(xt, yt) == np.mean(lab == yt)
    assert (clf.r_ is None) if nu is None else (clf.r_.shape == (15,) and (clf.r_ > 0).all())


def test_kernelsvm_rbf_is_rbfsvm_bit_for_bit():
    from mr_gan_amd import RBFSVM, KernelSVM
    for d, trials, per, sep, Cc in (E2E_CASES[1], E2E_CASES[3]):
        xl, yl, xt, _ = e2e_data(d, trials, per, sep)
        a = RBFSVM(C=Cc, gamma='auto').fit(xl, yl)
        b = KernelSVM(kernel='rbf', C=Cc, gamma='auto').fit(xl, yl)
        assert a.dual_coef_dense_.tobytes() == b.dual_coef_dense_.tobytes() and a.intercept_.tobytes() == b.intercept_.tobytes()
        assert a.n_iter_.tobytes() == b.n_iter_.tobytes() and b.r_ is None
        assert a.decision_function(xt).tobytes() == b.decision_function(xt).tobytes()
        assert (a.predict(xt) == b.predict(xt)).all()


@pytest.mark.parametrize("kernel,nu", [('linear', None), ('rbf', 0.5)])
def test_kernelsvm_chunk_edges_change_no_bit(kernel, nu):
    from mr_gan_amd import KernelSVM
    xl, yl, xt, _ = e2e_data(37, 20, 24, 1.5)
    clf = KernelSVM(kernel=kernel, nu=nu, C=0.01).fit(xl, yl)
    dec, lab = clf.decision_function(xt), clf.predict(xt)
    for chunk in (1, 7):
        assert clf.decision_function(xt, chunk=chunk).tobytes() == dec.tobytes()
        assert (clf.predict(xt, chunk=chunk) == lab).all()


def test_kernelsvm_refuses_infeasible_nu_and_warns_at_max_iter():
    from mr_gan_amd import KernelSVM
    from mr_gan_amd.svm import SVMConvergenceWarning
    xl, yl, xt, _ = e2e_data(37, 20, 24, 1.5)
    keep = np.concatenate([np.flatnonzero(yl == 0)[:5], np.flatnonzero(yl > 0)])
    with pytest.raises(ValueError, match="specified nu is infeasible"):
        KernelSVM(nu=0.5).fit(xl[keep], yl[keep])
    with pytest.warns(SVMConvergenceWarning, match="KernelSVM"):
        clf = KernelSVM(kernel='linear', nu=0.5, max_iter=3).fit(xl, yl)
    assert (clf.n_iter_ == 3).all() and clf.predict(xt).shape == (len(xt),)


@pytest.mark.parametrize("classifier", ['svc-linear', 'nu-rbf', 'nu-linear'])
def test_mr_svm_hip_backend_classifiers_on_the_harness(classifier):
    """mr_svm(backend='hip', classifier=...) on the synthetic set is KernelSVM on the prologue's labeled subset"""
    from mr_gan_amd import KernelSVM, synthetic_mreo
    from mr_gan_amd.data import prologue, resolve_num_classes, train_test_sets
    from mr_gan_amd.mr_svm import CLASSIFIERS, mr_svm
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    tr = np.arange(len(y)) % 6 != 0
    sets = [X[tr], X[~tr], y[tr], y[~tr]]
    got = mr_svm(None, None, percentlabeled=2, trainTestSets=sets, seed=3, backend='hip', classifier=classifier)
    rs, nc = np.random.RandomState(3), resolve_num_classes(None)
    x_labeled, y_labeled, _, _, X_test, y_test, _ = prologue(train_test_sets(None, None, sets, rs, nc), 2, None, rs, nc)
    kernel, nu = CLASSIFIERS[classifier]
    want = 1.0 - KernelSVM(kernel=kernel, nu=nu, C=1.0, gamma='auto').fit(x_labeled, y_labeled).score(X_test, y_test)
    assert got == want and 0.0 <= got < 0.5
