"""The grouped twins of the SVM kinds (mrgan_svm_kernel_matrix_group, mrgan_svm_solve_nu_group) on the GPU: every item of a ragged
group against the single entry called on that item, bit for bit; the grouped nu solver also on its own terms; KernelSVMGroup
against KernelSVM objects and against RBFSVMGroup; mr_svm_folds(classifier=...) against mr_svm(backend='hip', classifier=...)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svm_kinds_ref as N
from tests import svm_ref as R
from tests import test_svm_gpu as T
from tests import test_svm_groups_gpu as G
from tests import test_svm_kinds_gpu as KT

pytestmark = pytest.mark.gpu
RBF, LINEAR = 0, 1
bits = G.bits


def _E():
    from mr_gan_amd import engine as E
    return E


# ---------------------------------------------------------------------------------------------------------------------
# kernel matrix
# ---------------------------------------------------------------------------------------------------------------------
def km_single(c, kind, gamma):
    """mrgan_svm_kernel_matrix on the device operands of one GramCase -> the whole padded output buffer"""
    out = c.fresh()
    rc = T._lib().mrgan_svm_kernel_matrix(kind, c.a.data_ptr(), c.ld_a, c.m, c.b.data_ptr(), c.ld_b, c.n, c.d, float(gamma),
                                          out.data_ptr(), c.ld_out, T._stream())
    assert rc == 0, T._lib().mrgan_last_error()
    return out.cpu().numpy()


def km_group(kind, cases, d, gamma, tile=None, count=None, null_items=False):
    """one grouped launch -> rc, the whole padded output buffer of every item"""
    E, lib = _E(), T._lib()
    outs = [c.fresh() for c in cases]
    items = None if null_items else (E.SvmGramItem * len(cases))(*[c.item(o) for c, o in zip(cases, outs)])
    count = len(cases) if count is None else count
    if tile is None:
        rc = lib.mrgan_svm_kernel_matrix_group(kind, items, count, d, float(gamma), T._stream())
    else:
        rc = lib.mrgan_debug_svm_kernel_matrix_group(kind, items, count, d, float(gamma), tile, T._stream())
    T._torch().cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


def check_km_group(kind, cases, d, gamma, tiles):
    want = [km_single(c, kind, gamma) for c in cases]
    for tile in tiles:
        rc, got = km_group(kind, cases, d, gamma, tile)
        assert rc == 0, T._lib().mrgan_last_error()
        for i, (c, g, w) in enumerate(zip(cases, got, want)):
            win = g[:c.m, :c.n]
            assert bits(win) == bits(w[:c.m, :c.n]), (tile, i)
            assert (g[c.m:] == -7.0).all() and (g[:, c.n:] == -7.0).all(), (tile, i)      # nothing outside the window
            assert np.isfinite(win).all()
            if c.sym:
                assert bits(win) == bits(win.T), (tile, i)
                if kind == RBF:
                    assert (np.diag(win) == np.float32(1.0)).all(), (tile, i)
        if kind == RBF:                     # the very kernel of mrgan_svm_gram_group: the whole padded buffers
            rc, old = G.gram_group(cases, d, gamma, tile)
            assert rc == 0 and all(bits(a) == bits(b) for a, b in zip(got, old)), tile


@pytest.mark.parametrize("kind", [RBF, LINEAR])
def test_kernel_matrix_group_ragged_items_match_the_single_entry(kind):
    d = 37
    rs = np.random.RandomState(11)
    cases = [G.GramCase(rs, 1, 1, d, False), G.GramCase(rs, 70, 70, d, True), G.GramCase(rs, 64, 64, d, False),
             G.GramCase(rs, 130, 97, d, False), G.GramCase(rs, 129, 129, d, True, pad=(3, 3, 5))]
    gamma = np.float32(1.0 / d) if kind == RBF else float('nan')          # the linear kind ignores gamma
    check_km_group(kind, cases, d, gamma, (None, 64, 128))
    check_km_group(kind, cases[3:4], d, gamma, (None, 64, 128))           # count = 1


def test_linear_group_of_sixteen_takes_the_large_tile():
    """16 x (384, 384): 16 x 9 = 144 tiles of 128, so the launcher itself picks 128; the single entry picks 64 for each item"""
    d = 3
    rs = np.random.RandomState(12)
    cases = [G.GramCase(rs, 384, 384, d, i % 2 == 1) for i in range(16)]
    check_km_group(LINEAR, cases, d, 1.0, (None,))


def test_kernel_matrix_group_refuses_before_any_launch():
    E, lib = _E(), T._lib()
    d = 5
    rs = np.random.RandomState(13)
    cases = [G.GramCase(rs, 9, 7, d, False) for _ in range(17)]

    def refused(rc, outs, *words):
        msg = lib.mrgan_last_error()
        assert rc < 0 and all(w in msg for w in words), msg
        assert all((o == -7.0).all() for o in outs)
    for kind in (RBF, LINEAR):
        for count in (0, 17, -1):
            refused(*km_group(kind, cases, d, 0.2, count=count), b"svm_gram", b"count")
        refused(*km_group(kind, cases[:3], d, 0.2, null_items=True), b"svm_gram", b"null item list")
    for kind in (2, -1):
        refused(*km_group(kind, cases[:3], d, 0.2), b"unknown kernel kind")
    refused(*km_group(LINEAR, cases[:3], d, 0.2, tile=32), b"tile")
    cases = cases[:6]
    cases[3].ld_out = cases[3].n - 1                                  # a pitch smaller than the row in item 3
    for kind, tile in ((RBF, None), (LINEAR, None), (LINEAR, 64)):
        rc, outs = km_group(kind, cases, d, 0.2, tile)
        refused(rc, outs, b"svm_gram", b"pitch")                      # items 0 .. 2 were not launched either
        assert lib.mrgan_last_error().endswith(b"(item 3)")
    # gamma is checked for the RBF kind only
    rc, outs = km_group(RBF, cases[:3], d, float('nan'))
    refused(rc, outs, b"gamma", b"(item 0)")
    assert km_group(LINEAR, cases[:3], d, float('nan'))[0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# nu solver
# ---------------------------------------------------------------------------------------------------------------------
def nu_group(name):
    """-> [(class_start, Gram matrix)], [nu]"""
    if name == 'k2':
        return [T.solver_case(n)[1:3] for n in ('two_rows', 'unequal', 'pair_2048')], [0.5, 0.3, 0.5]
    if name == 'k3':
        return [T.solver_case(n)[1:3] for n in ('single_row_class', 'c100_all_free')], [0.1, 0.1]
    return [T.solver_case('bounded_heavy')[1:3], G.trimmed_bounded_heavy(7)], [0.5, 0.5]


def run_solve_nu_group(probs, nus, tol=1e-3, max_iter=10_000_000, want_r=None, share_k=False, count=None, null_items=False):
    """one grouped launch; every buffer is one row / element larger than the problem needs, NaN / -1 pre-filled; share_k: every
    item reads the first item's device matrix -> rc, [(coef, rho, r, iters)] whole buffers"""
    torch, lib, E = T._torch(), T._lib(), _E()
    nc = len(probs[0][0]) - 1
    pairs = nc * (nc - 1) // 2
    want_r = [True] * len(probs) if want_r is None else want_r
    keep, items = [], []
    for (cs, K32), nu, wr in zip(probs, nus, want_r):
        n = K32.shape[0]
        Kd = keep[0][0] if share_k and keep else T.to_dev(K32.astype(np.float32))
        coef = torch.full((nc, n), float('nan'), dtype=torch.float64, device="cuda:0")
        rho = torch.full((pairs + 1,), float('nan'), dtype=torch.float64, device="cuda:0")
        r = torch.full((pairs + 1,), float('nan'), dtype=torch.float64, device="cuda:0")
        iters = torch.full((pairs + 1,), -1, dtype=torch.int32, device="cuda:0")
        arr = (C.c_int64 * (nc + 1))(*[int(v) for v in cs])
        keep.append((Kd, coef, rho, r, iters, arr))
        items.append(E.SvmSolveNuItem(Kd.data_ptr(), Kd.stride(0), n, arr, nu, coef.data_ptr(), rho.data_ptr(),
                                      r.data_ptr() if wr else None, iters.data_ptr()))
    arr = None if null_items else (E.SvmSolveNuItem * len(items))(*items)
    rc = lib.mrgan_svm_solve_nu_group(arr, len(items) if count is None else count, nc, tol, max_iter, T._stream())
    torch.cuda.synchronize()
    return rc, [tuple(t.cpu().numpy() for t in k[1:5]) for k in keep]


@functools.lru_cache(maxsize=None)
def single_nu(name_or_drop, nu, tol, max_iter):
    """mrgan_svm_solve_nu on one problem, computed once: a solver_case name, or the rows dropped from bounded_heavy"""
    cs, K32 = G.trimmed_bounded_heavy(name_or_drop) if isinstance(name_or_drop, int) else T.solver_case(name_or_drop)[1:3]
    out = KT.run_solve_nu(K32, cs, nu, tol, max_iter)
    assert out[0] == 0, T._lib().mrgan_last_error()
    return out[1:]


GROUP_KEYS = {'k2': ('two_rows', 'unequal', 'pair_2048'), 'k3': ('single_row_class', 'c100_all_free'), 'k6': ('bounded_heavy', 7)}


@functools.lru_cache(maxsize=None)
def grouped_nu(name, max_iter=10_000_000):
    probs, nus = nu_group(name)
    rc, got = run_solve_nu_group(probs, nus, 1e-3, max_iter)
    assert rc == 0, T._lib().mrgan_last_error()
    return got


def assert_untouched_guards(got, with_r=None):
    for i, (coef, rho, r, iters) in enumerate(got):
        assert np.isnan(coef[-1]).all() and np.isnan(rho[-1]) and np.isnan(r[-1]) and iters[-1] == -1, i
        if with_r is not None and not with_r[i]:
            assert np.isnan(r).all(), i


def assert_matches_single_nu(keys, nus, got, tol, max_iter):
    for i, (key, nu, (coef, rho, r, iters)) in enumerate(zip(keys, nus, got)):
        c1, rho1, r1, i1 = single_nu(key, nu, tol, max_iter)
        assert bits(coef[:-1]) == bits(c1) and bits(rho[:-1]) == bits(rho1) and bits(iters[:-1]) == bits(i1), (i, key)
        assert bits(r[:-1]) == bits(r1), (i, key)
    assert_untouched_guards(got)


@pytest.mark.parametrize("name", ['k2', 'k3', 'k6'])
def test_solve_nu_group_matches_the_single_entry(name):
    """per-item nu (k2: 0.5, 0.3, 0.5 on 2, 40 and 2048 rows), K = 3 and K = 6: coef, rho, r and iters of every item"""
    _, nus = nu_group(name)
    got = grouped_nu(name)
    assert_matches_single_nu(GROUP_KEYS[name], nus, got, 1e-3, 10_000_000)
    full = [g[3][:-1] for g in got]
    assert all((f < 10_000_000).all() for f in full)
    # max_iter = 5: the same bits again; 5 updates wherever the start point is not optimal, none on the two-row problem, whose
    # start point (0.5, 0.5) is the optimum
    got = grouped_nu(name, 5)
    assert_matches_single_nu(GROUP_KEYS[name], nus, got, 1e-3, 5)
    for i, g in enumerate(got):
        print("%s item %d: updates %s at max_iter = 5, %s without" % (name, i, g[3][:-1].tolist(), full[i].tolist()))
        assert (g[3][:-1] == np.minimum(5, full[i])).all(), (i, g[3])
        if name == 'k2' and i == 0:
            assert g[3][0] == 0 and full[i][0] == 0
        else:
            assert (g[3][:-1] == 5).all(), (i, g[3])


def test_solve_nu_group_repeats_bit_for_bit_and_r_is_optional():
    probs, nus = nu_group('k6')
    a = grouped_nu('k6')
    rc, b = run_solve_nu_group(probs, nus)
    assert rc == 0
    for u, v in zip(a, b):
        assert all(bits(x) == bits(y) for x, y in zip(u, v))
    # r_dev null in item 1: that r buffer stays at its fill and nothing else changes
    rc, c = run_solve_nu_group(probs, nus, want_r=[True, False])
    assert rc == 0
    assert_untouched_guards(c, [True, False])
    for i, (u, v) in enumerate(zip(a, c)):
        assert bits(u[0]) == bits(v[0]) and bits(u[1]) == bits(v[1]) and bits(u[3]) == bits(v[3]), i
    assert bits(a[0][2]) == bits(c[0][2])


def test_solve_nu_group_one_gram_matrix_at_several_nu():
    """bounded_heavy three times in one launch at nu 0.2, 0.5 and 0.8: the items share k_dev, which they only read"""
    prob = T.solver_case('bounded_heavy')[1:3]
    nus = [0.2, 0.5, 0.8]
    rc, got = run_solve_nu_group([prob] * 3, nus, share_k=True)
    assert rc == 0, T._lib().mrgan_last_error()
    assert_matches_single_nu(['bounded_heavy'] * 3, nus, got, 1e-3, 10_000_000)
    assert len({bits(g[0]) for g in got}) == 3 and all((g[3][:-1] > 0).all() for g in got)


def test_solve_nu_group_on_its_own_terms():
    """the criteria of test_nu_solver_optimality on the grouped outputs themselves (K = 6, nu = 0.5, tol = 1e-3)"""
    probs, nus = nu_group('k6')
    tol, max_iter = 1e-3, 10_000_000
    for q, ((cs, K), nu, (coef, rho, r, iters)) in enumerate(zip(probs, nus, grouped_nu('k6'))):
        coef, rho, r, iters = coef[:-1], rho[:-1], r[:-1], iters[:-1]
        assert np.isfinite(coef).all() and np.isfinite(rho).all() and (r > 0).all()
        KT.check_feasible_nu(coef, r, cs, nu)
        for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
            rows, yy = R.pair_rows(cs, i, j)
            Kp = K[np.ix_(rows, rows)]
            alpha = KT.pair_alpha_nu(coef, cs, i, j, r[p])
            gap = N.nu_kkt_gap(Kp, yy, alpha)
            want_rho, want_r = N.nu_calculate_rho(yy, N.nu_gradient(Kp, yy, alpha), alpha)
            print("problem %d pair (%d, %d): gap / tol = %.4f, |rho r - calculate_rho| = %.3g, |r - r'| = %.3g, iterations = %d"
                  % (q, i, j, gap / tol, abs(rho[p] * r[p] - want_rho), abs(r[p] - want_r), iters[p]))
            assert gap < tol * (1 + 1e-6)
            assert abs(rho[p] * r[p] - want_rho) <= 1e-12 and abs(r[p] - want_r) <= 1e-12
            assert 0 <= iters[p] < max_iter


def test_solve_nu_group_refuses_before_any_launch():
    torch, lib, E = T._torch(), T._lib(), _E()
    probs, nus = nu_group('k2')

    def refused(rc, got, *words):
        msg = lib.mrgan_last_error()
        assert rc < 0 and all(w in msg for w in words), msg
        for coef, rho, r, iters in got:                               # no item was launched
            assert np.isnan(coef).all() and np.isnan(rho).all() and np.isnan(r).all() and (iters == -1).all()
    for count in (0, 17, -1):
        refused(*run_solve_nu_group(probs, nus, count=count), b"svm_solve_nu", b"count")
    refused(*run_solve_nu_group(probs, nus, null_items=True), b"svm_solve_nu", b"null item list")
    for bad in (0.0, 1.5):
        rc, got = run_solve_nu_group(probs, [0.5, 0.3, bad])
        refused(rc, got, b"nu must lie in (0, 1]")
        assert lib.mrgan_last_error().endswith(b"(item 2)")
    # nu = 0.5 in every item: `unequal`, 7 + 33 rows, is infeasible above 0.35
    rc, got = run_solve_nu_group(probs, [0.5, 0.5, 0.5])
    refused(rc, got, b"specified nu is infeasible", b"classes 0 and 1")
    assert lib.mrgan_last_error().endswith(b"(item 1)")
    for kw in (dict(tol=0.0), dict(max_iter=0)):
        refused(*run_solve_nu_group(probs, nus, **kw), b"positive", b"(item 0)")
    # item 1 holds a pair of 2049 rows
    n = 2049
    Kd = torch.eye(n, dtype=torch.float32, device="cuda:0")           # r = 0.5 on item 0 (a matrix of ones gives libsvm's unguarded r = 0)
    coef = torch.full((2, n), float('nan'), dtype=torch.float64, device="cuda:0")
    rho = torch.full((2,), float('nan'), dtype=torch.float64, device="cuda:0")
    r = torch.full((2,), float('nan'), dtype=torch.float64, device="cuda:0")
    iters = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
    small, big = (C.c_int64 * 3)(0, 5, 10), (C.c_int64 * 3)(0, 1024, 2049)
    items = (E.SvmSolveNuItem * 2)(
        E.SvmSolveNuItem(Kd.data_ptr(), n, 10, small, 0.5, coef.data_ptr(), rho.data_ptr(), r.data_ptr(), iters.data_ptr()),
        E.SvmSolveNuItem(Kd.data_ptr(), n, n, big, 0.5, coef[1:].data_ptr(), rho[1:].data_ptr(), r[1:].data_ptr(), iters[1:].data_ptr()))
    assert lib.mrgan_svm_solve_nu_group(items, 2, 2, 1e-3, 100, T._stream()) < 0
    msg = lib.mrgan_last_error()
    assert b"MRGAN_SVM_MAX_PAIR" in msg and msg.endswith(b"(item 1)"), msg
    torch.cuda.synchronize()
    assert torch.isnan(coef).all() and torch.isnan(rho).all() and torch.isnan(r).all() and (iters == -1).all()
    assert lib.mrgan_svm_solve_nu_group(items, 1, 2, 1e-3, 100, T._stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(coef[0, :10]).all() and torch.isnan(coef[0, 10:]).all() and torch.isnan(coef[1]).all()
    assert r[0] > 0 and torch.isnan(r[1])


# ---------------------------------------------------------------------------------------------------------------------
# KernelSVMGroup
# ---------------------------------------------------------------------------------------------------------------------
KINDS = [('linear', None, 0.01), ('rbf', 0.5, 1.0), ('linear', 0.5, 1.0)]        # kernel, nu, C (the C of test_svm_kinds_gpu's linear cases)
SEQ_NU = (0.5, 0.3, 0.2, 0.5, 0.4, 0.6)


@functools.lru_cache(maxsize=None)
def single_fit(kernel, nu, Cc, i):
    """KernelSVM on problem i of ragged_problems(), fitted once -> the classifier, its decisions, labels and score"""
    from mr_gan_amd import KernelSVM
    x, y, xt, yt = G.ragged_problems()[i]
    clf = KernelSVM(kernel=kernel, nu=nu, C=Cc, gamma='auto').fit(x, y)
    return clf, clf.decision_function(xt), clf.predict(xt), clf.score(xt, yt)


def assert_kind_group_equals_singles(group, kernel, nus, Cc, idx, chunk=None, fitted=True):
    probs = G.ragged_problems()
    xts, yts = [probs[i][2] for i in idx], [probs[i][3] for i in idx]
    dec, lab, score = group.decision_function(xts, chunk=chunk), group.predict(xts, chunk=chunk), group.score(xts, yts)
    assert len(group) == len(idx) == len(dec) == len(lab) == len(score)
    for p, i in enumerate(idx):
        clf, d1, l1, s1 = single_fit(kernel, nus[p], Cc, i)
        if fitted:
            f = group[p]
            assert f.classes_.tolist() == clf.classes_.tolist()
            assert bits(f.dual_coef_dense_) == bits(clf.dual_coef_dense_) and f.dual_coef_dense_.shape == clf.dual_coef_dense_.shape
            assert bits(f.intercept_) == bits(clf.intercept_) and bits(f.n_iter_) == bits(clf.n_iter_)
            assert (f.r_ is None and clf.r_ is None) if nus[p] is None else bits(f.r_) == bits(clf.r_)
            assert (f.n_iter_ < group.max_iter).all()
        assert bits(dec[p]) == bits(d1) and dec[p].shape == d1.shape
        assert (lab[p] == l1).all() and lab[p].shape == l1.shape and score[p] == s1


@pytest.mark.parametrize("kernel,nu,Cc", KINDS)
def test_kernel_group_equals_six_single_fits(kernel, nu, Cc):
    from mr_gan_amd import KernelSVMGroup
    probs = G.ragged_problems()
    group = KernelSVMGroup(kernel=kernel, nu=nu, C=Cc, gamma='auto').fit([q[0] for q in probs], [q[1] for q in probs])
    assert group[1].classes_.tolist() == G.REMAP.tolist()
    assert_kind_group_equals_singles(group, kernel, [nu] * 6, Cc, range(6))
    for chunk in (1, 7):
        assert_kind_group_equals_singles(group, kernel, [nu] * 6, Cc, range(6), chunk=chunk, fitted=False)


@pytest.mark.parametrize("kernel,nu,Cc", KINDS)
def test_kernel_group_sub_groups_change_no_bit(kernel, nu, Cc):
    """17 problems are two sub-groups (16 + 1); a Gram budget of two matrices makes sub-groups of two"""
    from mr_gan_amd import KernelSVMGroup
    from mr_gan_amd.svm import plan_subgroups
    probs = G.ragged_problems()
    idx = [i % 6 for i in range(17)]
    group = KernelSVMGroup(kernel=kernel, nu=nu, C=Cc).fit([probs[i][0] for i in idx], [probs[i][1] for i in idx])
    assert_kind_group_equals_singles(group, kernel, [nu] * 17, Cc, idx)
    budget = 2 * 4 * 144 * 144
    assert max(len(s) for s in plan_subgroups([4 * len(q[1]) ** 2 for q in probs], budget)) == 2
    group = KernelSVMGroup(kernel=kernel, nu=nu, C=Cc, gram_bytes=budget).fit([q[0] for q in probs], [q[1] for q in probs])
    assert_kind_group_equals_singles(group, kernel, [nu] * 6, Cc, range(6))
    assert_kind_group_equals_singles(group, kernel, [nu] * 6, Cc, range(6), chunk=7, fitted=False)


def test_kernel_group_takes_a_nu_per_problem():
    from mr_gan_amd import KernelSVMGroup
    probs = G.ragged_problems()
    group = KernelSVMGroup(kernel='rbf', nu=SEQ_NU).fit([q[0] for q in probs], [q[1] for q in probs])
    assert_kind_group_equals_singles(group, 'rbf', SEQ_NU, 1.0, range(6))
    assert bits(group[0].r_) != bits(group[1].r_)              # the same rows under other label values: nu 0.5 against 0.3


def test_kernel_group_rbf_is_rbfsvm_group_bit_for_bit():
    from mr_gan_amd import KernelSVMGroup, RBFSVMGroup
    probs = G.ragged_problems()
    Xs, ys, xts = [q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs]
    a, b = RBFSVMGroup(gamma='auto').fit(Xs, ys), KernelSVMGroup(kernel='rbf', gamma='auto').fit(Xs, ys)
    for p in range(6):
        assert bits(a[p].dual_coef_dense_) == bits(b[p].dual_coef_dense_) and bits(a[p].intercept_) == bits(b[p].intercept_)
        assert bits(a[p].n_iter_) == bits(b[p].n_iter_) and b[p].r_ is None and a[p].classes_.tolist() == b[p].classes_.tolist()
    for da, db in zip(a.decision_function(xts), b.decision_function(xts)):
        assert bits(da) == bits(db)
    assert all((la == lb).all() for la, lb in zip(a.predict(xts), b.predict(xts)))


def test_kernel_group_refuses_infeasible_nu_and_warns_at_max_iter():
    from mr_gan_amd import KernelSVMGroup
    from mr_gan_amd.svm import SVMConvergenceWarning
    probs = G.ragged_problems()
    x, y = probs[0][0], probs[0][1]
    keep = np.concatenate([np.flatnonzero(y == 0)[:5], np.flatnonzero(y > 0)])
    with pytest.raises(ValueError, match=r"specified nu is infeasible.*\(problem 1\)"):
        KernelSVMGroup(nu=0.5).fit([x, x[keep]], [y, y[keep]])
    with pytest.warns(SVMConvergenceWarning, match=r"KernelSVMGroup: problems \[0, 1\]"):
        group = KernelSVMGroup(kernel='linear', nu=0.5, max_iter=3).fit([x, probs[2][0]], [y, probs[2][1]])
    assert (group[0].n_iter_ == 3).all() and (group[1].n_iter_ == 3).all()
    assert group.predict([probs[0][2], probs[2][2]])[1].shape == (len(probs[2][2]),)


# ---------------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classifier", ['svc-linear', 'nu-rbf', 'nu-linear'])
def test_mr_svm_folds_equals_mr_svm_per_fold(classifier):
    from mr_gan_amd import synthetic_mreo
    from mr_gan_amd.mr_svm import mr_svm, mr_svm_folds
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    fold = np.arange(len(y)) % 3
    sets = [[X[fold != f], X[fold == f], y[fold != f], y[fold == f]] for f in range(3)]
    got = mr_svm_folds(sets, percentlabeled=2, seed=3, classifier=classifier)
    want = [mr_svm(None, None, percentlabeled=2, trainTestSets=sets[f], seed=3 + f, backend='hip', classifier=classifier) for f in range(3)]
    assert got == want and all(0.0 <= e < 0.5 for e in got)
