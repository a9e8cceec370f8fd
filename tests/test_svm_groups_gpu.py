"""The grouped SVM entries (mrgan_svm_gram_group, mrgan_svm_solve_group, mrgan_svm_decide_group) on the GPU: every item of a
ragged group against the single entry called on that item, bit for bit; the grouped solver also on its own terms; RBFSVMGroup
against RBFSVM objects; mr_svm_folds against mr_svm(backend='hip')."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svm_ref as R
from tests import test_svm_gpu as T

pytestmark = pytest.mark.gpu


def _E():
    from mr_gan_amd import engine as E
    return E


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Gram
# ---------------------------------------------------------------------------------------------------------------------
class GramCase:
    """device operands (padding NaN-filled) of one item and a fresh -7-filled output buffer per run"""

    def __init__(self, rs, m, n, d, sym, pad=(0, 0, 0)):
        self.m, self.n, self.d, self.sym = m, n, d, sym
        self.ld_a, self.ld_b, self.ld_out = d + pad[0], d + (pad[0] if sym else pad[1]), n + pad[2]

        def padded(rows, ld):
            buf = np.full((rows, ld), np.nan, np.float32)            # a read past the row's width poisons the result
            buf[:, :d] = rs.randn(rows, d)
            return T.to_dev(buf)
        self.a = padded(m, self.ld_a)
        self.b = self.a if sym else padded(n, self.ld_b)

    def fresh(self):
        return T._torch().full((self.m + 1, self.ld_out), -7.0, dtype=T._torch().float32, device="cuda:0")

    def item(self, out):
        return _E().SvmGramItem(self.a.data_ptr(), self.ld_a, self.m, self.b.data_ptr(), self.ld_b, self.n, out.data_ptr(), self.ld_out)

    def single(self, gamma):
        out = self.fresh()
        rc = T._lib().mrgan_svm_gram(self.a.data_ptr(), self.ld_a, self.m, self.b.data_ptr(), self.ld_b, self.n, self.d, float(gamma),
                                     out.data_ptr(), self.ld_out, T._stream())
        assert rc == 0, T._lib().mrgan_last_error()
        return out.cpu().numpy()


def gram_group(cases, d, gamma, tile=None, count=None):
    """one grouped launch -> rc, the whole padded output buffer of every item"""
    E, lib = _E(), T._lib()
    outs = [c.fresh() for c in cases]
    items = (E.SvmGramItem * len(cases))(*[c.item(o) for c, o in zip(cases, outs)])
    count = len(cases) if count is None else count
    if tile is None:
        rc = lib.mrgan_svm_gram_group(items, count, d, float(gamma), T._stream())
    else:
        rc = lib.mrgan_debug_svm_gram_group(items, count, d, float(gamma), tile, T._stream())
    T._torch().cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


def check_gram_group(cases, d, gamma, tiles):
    want = [c.single(gamma) for c in cases]
    for tile in tiles:
        rc, got = gram_group(cases, d, gamma, tile)
        assert rc == 0, T._lib().mrgan_last_error()
        for i, (c, g, w) in enumerate(zip(cases, got, want)):
            win = g[:c.m, :c.n]
            assert bits(win) == bits(w[:c.m, :c.n]), (tile, i)
            assert (g[c.m:] == -7.0).all() and (g[:, c.n:] == -7.0).all(), (tile, i)      # nothing outside the window
            assert np.isfinite(win).all()
            if c.sym:
                assert bits(win) == bits(win.T) and (np.diag(win) == np.float32(1.0)).all(), (tile, i)


def test_gram_group_ragged_items_match_the_single_entry():
    d = 37
    rs = np.random.RandomState(11)
    cases = [GramCase(rs, 1, 1, d, False), GramCase(rs, 70, 70, d, True), GramCase(rs, 64, 64, d, False),
             GramCase(rs, 130, 97, d, False), GramCase(rs, 129, 129, d, True, pad=(3, 3, 5))]
    check_gram_group(cases, d, np.float32(1.0 / d), (None, 64, 128))
    check_gram_group(cases[3:4], d, np.float32(1.0 / d), (None, 64, 128))                # count = 1


def test_gram_group_of_sixteen_takes_the_large_tile():
    """16 x (384, 384): 16 x 9 = 144 tiles of 128, so the launcher itself picks 128; the single entry picks 64 for each item"""
    d = 3
    rs = np.random.RandomState(12)
    cases = [GramCase(rs, 384, 384, d, i % 2 == 1) for i in range(16)]
    check_gram_group(cases, d, np.float32(1.0 / d), (None, 64, 128))


def test_gram_group_refuses_before_any_launch():
    E, lib = _E(), T._lib()
    d = 5
    rs = np.random.RandomState(13)
    cases = [GramCase(rs, 9, 7, d, False) for _ in range(17)]
    for count in (0, 17, -1):
        rc, outs = gram_group(cases, d, 0.2, count=count)
        msg = lib.mrgan_last_error()
        assert rc < 0 and b"svm_gram" in msg and b"count" in msg, msg
        assert all((o == -7.0).all() for o in outs)
    cases = cases[:6]
    cases[3].ld_out = cases[3].n - 1                                  # a pitch smaller than the row in item 3
    for tile in (None, 64):
        rc, outs = gram_group(cases, d, 0.2, tile)
        msg = lib.mrgan_last_error()
        assert rc < 0 and b"svm_gram" in msg and b"pitch" in msg and b"item 3" in msg, msg
        assert all((o == -7.0).all() for o in outs)                   # items 0 .. 2 were not launched either
    rc, _ = gram_group(cases[:3], d, float('nan'))
    assert rc < 0 and b"gamma" in lib.mrgan_last_error() and b"item 0" in lib.mrgan_last_error()
    assert lib.mrgan_debug_svm_gram_group((E.SvmGramItem * 1)(cases[0].item(cases[0].fresh())), 1, d, 0.2, 32, T._stream()) < 0
    assert b"tile" in lib.mrgan_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# solver
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trimmed_bounded_heavy(drop):
    """bounded_heavy without the last `drop` rows of every class -> class_start, Gram matrix"""
    _, cs, K, _ = T.solver_case('bounded_heavy')
    keep = np.concatenate([np.arange(cs[c], cs[c + 1] - drop) for c in range(6)])
    return np.arange(7) * (40 - drop), np.ascontiguousarray(K[np.ix_(keep, keep)])


def solver_group(name):
    """-> [(class_start, Gram matrix)], C"""
    if name == 'k2':
        return [T.solver_case(n)[1:3] for n in ('two_rows', 'unequal', 'pair_2048')], 1.0
    if name == 'k3':
        return [T.solver_case(n)[1:3] for n in ('single_row_class', 'c100_all_free')], 100.0
    return [T.solver_case('bounded_heavy')[1:3], trimmed_bounded_heavy(7)], 1.0


def run_solve_group(probs, Cc, tol=1e-3, max_iter=10_000_000):
    """one grouped launch; every buffer is one row / element larger than the problem needs, NaN / -1 pre-filled
    -> rc, [(coef, rho, iters)] whole buffers"""
    torch, lib, E = T._torch(), T._lib(), _E()
    nc = len(probs[0][0]) - 1
    pairs = nc * (nc - 1) // 2
    keep, items = [], []
    for cs, K32 in probs:
        n = K32.shape[0]
        Kd = T.to_dev(K32.astype(np.float32))
        coef = torch.full((nc, n), float('nan'), dtype=torch.float64, device="cuda:0")
        rho = torch.full((pairs + 1,), float('nan'), dtype=torch.float64, device="cuda:0")
        iters = torch.full((pairs + 1,), -1, dtype=torch.int32, device="cuda:0")
        arr = (C.c_int64 * (nc + 1))(*[int(v) for v in cs])
        keep.append((Kd, coef, rho, iters, arr))
        items.append(E.SvmSolveItem(Kd.data_ptr(), Kd.stride(0), n, arr, coef.data_ptr(), rho.data_ptr(), iters.data_ptr()))
    rc = lib.mrgan_svm_solve_group((E.SvmSolveItem * len(items))(*items), len(items), nc, Cc, tol, max_iter, T._stream())
    torch.cuda.synchronize()
    return rc, [(k[1].cpu().numpy(), k[2].cpu().numpy(), k[3].cpu().numpy()) for k in keep]


def assert_matches_single(probs, got, Cc, tol, max_iter):
    for i, ((cs, K32), (coef, rho, iters)) in enumerate(zip(probs, got)):
        rc, c1, r1, i1 = T.run_solve(K32, cs, Cc, tol, max_iter)
        assert rc == 0
        assert bits(coef[:-1]) == bits(c1) and bits(rho[:-1]) == bits(r1) and bits(iters[:-1]) == bits(i1), i
        assert np.isnan(coef[-1]).all() and np.isnan(rho[-1]) and iters[-1] == -1, i          # nothing else is written


@pytest.mark.parametrize("name", ['k2', 'k3', 'k6'])
def test_solve_group_matches_the_single_entry(name):
    probs, Cc = solver_group(name)
    rc, got = run_solve_group(probs, Cc)
    assert rc == 0, T._lib().mrgan_last_error()
    assert_matches_single(probs, got, Cc, 1e-3, 10_000_000)
    assert all((g[2][:-1] > 0).all() and (g[2][:-1] < 10_000_000).all() for g in got)
    full = [g[2][:-1] for g in got]
    # max_iter = 5: the same bits again, and every pair stops at 5 updates unless it was done before.  The two-row problem is
    # done after one (its first update puts both alphas at C, where nothing can move; tests/svm_ref.py stops there too); every
    # other pair here takes 13 updates or more
    rc, got = run_solve_group(probs, Cc, max_iter=5)
    assert rc == 0
    assert_matches_single(probs, got, Cc, 1e-3, 5)
    for i, g in enumerate(got):
        print("%s item %d: iterations %s at max_iter = 5, %s without" % (name, i, g[2][:-1].tolist(), full[i].tolist()))
        assert (g[2][:-1] == np.minimum(5, full[i])).all(), (i, g[2])
        if name == 'k2' and i == 0:
            assert g[2][0] == 1
        else:
            assert (g[2][:-1] == 5).all(), (i, g[2])


def test_solve_group_repeats_bit_for_bit_and_refuses_a_large_pair():
    torch, lib, E = T._torch(), T._lib(), _E()
    probs, Cc = solver_group('k6')
    (ra, a), (rb, b) = run_solve_group(probs, Cc), run_solve_group(probs, Cc)
    assert ra == 0 and rb == 0
    for u, v in zip(a, b):
        assert all(bits(x) == bits(y) for x, y in zip(u, v))
    # item 1 holds a pair of 2049 rows
    n = 2049
    Kd = torch.ones((n, n), dtype=torch.float32, device="cuda:0")
    coef = torch.full((2, n), float('nan'), dtype=torch.float64, device="cuda:0")
    rho = torch.full((2,), float('nan'), dtype=torch.float64, device="cuda:0")
    iters = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
    small, big = (C.c_int64 * 3)(0, 5, 10), (C.c_int64 * 3)(0, 1024, 2049)
    items = (E.SvmSolveItem * 2)(E.SvmSolveItem(Kd.data_ptr(), n, 10, small, coef.data_ptr(), rho.data_ptr(), iters.data_ptr()),
                                 E.SvmSolveItem(Kd.data_ptr(), n, n, big, coef[1:].data_ptr(), rho[1:].data_ptr(), iters[1:].data_ptr()))
    assert lib.mrgan_svm_solve_group(items, 2, 2, 1.0, 1e-3, 100, T._stream()) < 0
    msg = lib.mrgan_last_error()
    assert b"MRGAN_SVM_MAX_PAIR" in msg and b"item 1" in msg, msg
    torch.cuda.synchronize()
    assert torch.isnan(coef).all() and torch.isnan(rho).all() and (iters == -1).all()      # item 0 was not launched either
    for count in (0, 17):
        assert lib.mrgan_svm_solve_group(items, count, 2, 1.0, 1e-3, 100, T._stream()) < 0
        assert b"svm_solve" in lib.mrgan_last_error() and b"count" in lib.mrgan_last_error()
    assert lib.mrgan_svm_solve_group(items, 1, 2, 0.0, 1e-3, 100, T._stream()) < 0 and b"positive" in lib.mrgan_last_error()
    assert lib.mrgan_svm_solve_group(items, 1, 2, 1.0, 1e-3, 100, T._stream()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(coef[0, :10]).any() and torch.isnan(coef[0, 10:]).all() and torch.isnan(coef[1]).all()


def test_solve_group_on_its_own_terms():
    """the criteria of test_solver_optimality on the grouped outputs themselves (K = 6, tol = 1e-3)"""
    probs, Cc = solver_group('k6')
    tol, max_iter = 1e-3, 10_000_000
    rc, got = run_solve_group(probs, Cc, tol, max_iter)
    assert rc == 0
    for q, ((cs, K), (coef, rho, iters)) in enumerate(zip(probs, got)):
        coef, rho, iters = coef[:-1], rho[:-1], iters[:-1]
        assert np.isfinite(coef).all() and np.isfinite(rho).all()
        T.check_feasible(coef, cs, Cc)
        for p, (i, j) in enumerate(R.ovo_pairs(len(cs) - 1)):
            rows, yy = R.pair_rows(cs, i, j)
            Kp = K[np.ix_(rows, rows)]
            alpha = R.pair_alpha(coef, cs, i, j)
            gap = R.kkt_gap(Kp, yy, alpha, Cc)
            want_rho = R.calculate_rho(yy, R.gradient(Kp, yy, alpha), alpha, Cc)
            print("problem %d pair (%d, %d): gap / tol = %.4f, |rho - calculate_rho| = %.3g, iterations = %d"
                  % (q, i, j, gap / tol, abs(rho[p] - want_rho), iters[p]))
            assert gap < tol * (1 + 1e-6)
            assert abs(rho[p] - want_rho) <= 1e-12
            assert 0 < iters[p] < max_iter


# ---------------------------------------------------------------------------------------------------------------------
# decide
# ---------------------------------------------------------------------------------------------------------------------
def test_decide_group_matches_the_single_entry():
    """m = 1, 7 and 130 test rows against three fitted problems of n = 240, 198 and 222 rows; the second item has a wide
    pitch and no decision matrix"""
    torch, lib, E = T._torch(), T._lib(), _E()
    rs = np.random.RandomState(21)
    probs = [T.solver_case('bounded_heavy')[1:3], trimmed_bounded_heavy(7), trimmed_bounded_heavy(3)]
    nc, pairs = 6, 15
    keep, items, singles = [], [], []
    for (cs, K32), m, pad, want_dec in zip(probs, (1, 7, 130), (0, 9, 0), (True, False, True)):
        n = K32.shape[0]
        rc, coef, rho, _ = T.run_solve(K32, cs)
        assert rc == 0
        kt = np.full((m, n + pad), np.nan, np.float32)
        kt[:, :n] = rs.uniform(0.05, 1.0, size=(m, n))
        ktd, cd, rd = T.to_dev(kt), T.to_dev(coef), T.to_dev(rho)
        arr = (C.c_int64 * (nc + 1))(*[int(v) for v in cs])
        bufs = []
        for _ in range(2):              # grouped, single
            dec = torch.full((m + 1, pairs), float('nan'), dtype=torch.float64, device="cuda:0")
            lab = torch.full((m + 1,), -1, dtype=torch.int32, device="cuda:0")
            bufs.append((dec, lab))
        keep.append((ktd, cd, rd, arr, bufs, kt[:, :n], coef, rho, cs, m, want_dec))
        items.append(E.SvmDecideItem(ktd.data_ptr(), n + pad, m, n, arr, cd.data_ptr(), rd.data_ptr(),
                                     bufs[0][0].data_ptr() if want_dec else None, bufs[0][1].data_ptr()))
        singles.append((ktd.data_ptr(), n + pad, m, n, nc, arr, cd.data_ptr(), rd.data_ptr(),
                        bufs[1][0].data_ptr() if want_dec else None, bufs[1][1].data_ptr()))
    assert lib.mrgan_svm_decide_group((E.SvmDecideItem * 3)(*items), 3, nc, T._stream()) == 0, lib.mrgan_last_error()
    for s in singles:
        assert lib.mrgan_svm_decide(*s, T._stream()) == 0, lib.mrgan_last_error()
    torch.cuda.synchronize()
    for ktd, cd, rd, arr, bufs, kt, coef, rho, cs, m, want_dec in keep:
        (gd, gl), (sd, sl) = [(d.cpu().numpy(), l.cpu().numpy()) for d, l in bufs]
        assert bits(gl) == bits(sl) and bits(gd) == bits(sd)
        assert gl[m] == -1 and (gl[:m] >= 0).all() and np.isnan(gd[m]).all()
        assert np.isnan(gd[:m]).all() if not want_dec else np.isfinite(gd[:m]).all()
        if want_dec:
            # the vote of the returned decisions; the decisions against fp64 numpy: at most 80 terms |coef k| <= 1 per sum,
            # so another summation order moves them by <= 240 eps 80 ~ 4e-12
            assert (gl[:m] == R.vote(gd[:m], nc)).all()
            assert np.abs(gd[:m] - R.decisions(coef, rho, kt, cs)).max() <= 1e-9
    for count in (0, 17):
        assert lib.mrgan_svm_decide_group((E.SvmDecideItem * 3)(*items), count, nc, T._stream()) < 0
        assert b"svm_decide" in lib.mrgan_last_error() and b"count" in lib.mrgan_last_error()
    items[2].ld_kt = 10
    assert lib.mrgan_svm_decide_group((E.SvmDecideItem * 3)(*items), 3, nc, T._stream()) < 0
    assert b"pitch" in lib.mrgan_last_error() and b"item 2" in lib.mrgan_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# RBFSVMGroup
# ---------------------------------------------------------------------------------------------------------------------
REMAP = np.array([3, 7, 9, 11, 20, 21])


@functools.lru_cache(maxsize=None)
def ragged_problems():
    """six problems out of e2e_data(37, 20, 24, 1.5): the full set; the full set under other label values; four with rows
    dropped per class (and fewer test rows) -> [(x, y, x_test, y_test)]"""
    xl, yl, xt, yt = T.e2e_data(37, 20, 24, 1.5)
    within = np.arange(len(yl)) % 24                       # position of a row inside its class
    out = [(xl, yl, xt, yt), (xl, REMAP[yl], xt, REMAP[yt])]
    for p in range(2, 6):
        keep = within < 24 - p - (yl % 3)
        out.append((xl[keep], yl[keep], xt[:len(xt) - 5 * p], yt[:len(xt) - 5 * p]))
    return out


@functools.lru_cache(maxsize=None)
def single_fits():
    from mr_gan_amd import RBFSVM
    fits = []
    for x, y, xt, yt in ragged_problems():
        clf = RBFSVM(gamma='auto').fit(x, y)
        fits.append((clf, clf.decision_function(xt), clf.predict(xt), clf.score(xt, yt)))
    return fits


def assert_group_equals_singles(group, idx, chunk=None, fitted=True):
    probs, fits = ragged_problems(), single_fits()
    xts, yts = [probs[i][2] for i in idx], [probs[i][3] for i in idx]
    dec, lab, score = group.decision_function(xts, chunk=chunk), group.predict(xts, chunk=chunk), group.score(xts, yts)
    assert len(group) == len(idx) == len(dec) == len(lab) == len(score)
    for p, i in enumerate(idx):
        clf, d1, l1, s1 = fits[i]
        if fitted:
            assert group[p].classes_.tolist() == clf.classes_.tolist()
            assert bits(group[p].dual_coef_dense_) == bits(clf.dual_coef_dense_) and group[p].dual_coef_dense_.shape == clf.dual_coef_dense_.shape
            assert bits(group[p].intercept_) == bits(clf.intercept_) and bits(group[p].n_iter_) == bits(clf.n_iter_)
        assert bits(dec[p]) == bits(d1) and dec[p].shape == d1.shape
        assert (lab[p] == l1).all() and lab[p].shape == l1.shape and score[p] == s1


def test_rbfsvm_group_equals_six_single_fits():
    from mr_gan_amd import RBFSVMGroup
    probs = ragged_problems()
    assert len({len(q[1]) for q in probs}) == 5 and len({len(q[3]) for q in probs}) == 5        # ragged in both row counts
    group = RBFSVMGroup(gamma='auto').fit([q[0] for q in probs], [q[1] for q in probs])
    assert group[1].classes_.tolist() == REMAP.tolist()
    assert_group_equals_singles(group, range(6))
    for chunk in (1, 7):
        assert_group_equals_singles(group, range(6), chunk=chunk, fitted=False)


def test_rbfsvm_group_sub_groups_change_no_bit():
    """17 problems are two sub-groups (16 + 1); a Gram budget of two matrices makes sub-groups of two"""
    from mr_gan_amd import RBFSVMGroup
    from mr_gan_amd.svm import plan_subgroups
    probs = ragged_problems()
    idx = [i % 6 for i in range(17)]
    group = RBFSVMGroup().fit([probs[i][0] for i in idx], [probs[i][1] for i in idx])
    assert_group_equals_singles(group, idx)
    budget = 2 * 4 * 144 * 144
    assert max(len(s) for s in plan_subgroups([4 * len(q[1]) ** 2 for q in probs], budget)) == 2
    group = RBFSVMGroup(gram_bytes=budget).fit([q[0] for q in probs], [q[1] for q in probs])
    assert_group_equals_singles(group, range(6))
    assert_group_equals_singles(group, range(6), chunk=7, fitted=False)


def test_rbfsvm_group_refuses_mixed_shapes_and_warns_at_max_iter():
    from mr_gan_amd import RBFSVMGroup
    from mr_gan_amd.svm import SVMConvergenceWarning
    probs = ragged_problems()
    x, y = probs[0][0], probs[0][1]
    with pytest.raises(ValueError, match="feature count"):
        RBFSVMGroup().fit([x, x[:, :30]], [y, y])
    with pytest.raises(ValueError, match="class count"):
        RBFSVMGroup().fit([x, x[y < 5]], [y, y[y < 5]])
    with pytest.warns(SVMConvergenceWarning, match=r"problems \[0, 1\]"):
        group = RBFSVMGroup(max_iter=3).fit([x, probs[2][0]], [y, probs[2][1]])
    assert (group[0].n_iter_ == 3).all() and (group[1].n_iter_ == 3).all()
    assert group.predict([probs[0][2], probs[2][2]])[1].shape == (len(probs[2][2]),)


# ---------------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------------
def test_mr_svm_folds_equals_mr_svm_per_fold():
    from mr_gan_amd import synthetic_mreo
    from mr_gan_amd.mr_svm import mr_svm, mr_svm_folds
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    fold = np.arange(len(y)) % 3
    sets = [[X[fold != f], X[fold == f], y[fold != f], y[fold == f]] for f in range(3)]
    got = mr_svm_folds(sets, percentlabeled=2, seed=3)
    want = [mr_svm(None, None, percentlabeled=2, trainTestSets=sets[f], seed=3 + f, backend='hip') for f in range(3)]
    assert got == want and all(0.0 <= e < 0.5 for e in got)
