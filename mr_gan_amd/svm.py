"""RBF-kernel C-SVC on the GPU: the SVM baseline of the reference (mr_svm.py:106, SVC(kernel='rbf', C=1.0)) without scikit-learn.

    clf = RBFSVM(C=1.0, gamma='auto').fit(x_labeled, y_labeled); err = 1.0 - clf.score(X_test, y_test)

Three launches of csrc/svm.hip behind include/mrgan_abi.h: mrgan_svm_gram (fp32 Gram matrix on the matrix cores),
mrgan_svm_solve (libsvm's SMO, one workgroup per one-vs-one pair, fp64 state on chip) and mrgan_svm_decide (decision values
and the vote).  There is no CPU path: without the library or a GPU every entry raises.  The numpy restatement the tests
compare against lives in tests/svm_ref.py.  RBFSVMGroup fits and scores several independent problems (the folds of a table cell)
through the grouped entries mrgan_svm_*_group, one launch set for up to 16 of them, with RBFSVM's bits per problem.

KernelSVM covers the other libsvm classifiers of the reference's wider SVM grid (others/wganlpctsemi.py:205-208) with
RBFSVM's surface and conventions: kernel='rbf' | 'linear' through mrgan_svm_kernel_matrix (the linear Gram matrix is the
same matrix-core chain without norms and exp), and nu=None (C-SVC, mrgan_svm_solve) or a nu in (0, 1] (nu-SVC,
mrgan_svm_solve_nu: libsvm's Solver_NU, coefficients alpha y / r, r in r_).  mrgan_svm_decide serves every kind.  The nu
solver's restatement lives in tests/svm_kinds_ref.py.  KernelSVMGroup is to KernelSVM what RBFSVMGroup is to RBFSVM, through
mrgan_svm_kernel_matrix_group and mrgan_svm_solve_nu_group (nu per problem); the two group classes share one body (_GroupSVM).

Conventions are libsvm's: pairs (i, j), i < j, in the order of scikit-learn's decision_function_shape='ovo'; a positive
decision value votes for classes_[i]; intercept_ = -rho.  Two classes give ONE column with that same sign (scikit-learn flips
the sign of its binary decision_function; this class does not).
Out of scope: shrinking, probability estimates, class weights, polynomial and sigmoid kernels, LinearSVC (liblinear, another
algorithm), groups with mixed feature or class counts, a C per problem."""
import ctypes as C
import warnings

import numpy as np
import torch

from mr_gan_amd import engine as E


class SVMConvergenceWarning(UserWarning):
    """a one-vs-one problem stopped at max_iter (the role of sklearn.exceptions.ConvergenceWarning)"""


def class_sort(y):
    """labels -> (classes, order, class_start): classes = sorted distinct labels; order = the STABLE permutation that sorts the
    rows by class (row order[k] of the caller is row k on the device); class_start[c] = first sorted row of class c, [-1] = n"""
    y = np.asarray(y)
    if y.ndim != 1 or y.shape[0] == 0:
        raise ValueError("y must be a non-empty vector of labels, got shape %s" % (y.shape,))
    classes, codes = np.unique(y, return_inverse=True)
    order = np.argsort(codes, kind='stable')
    class_start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=len(classes)))]).astype(np.int64)
    return classes, order, class_start


def unsort_coef(coef_sorted, order):
    """[(K-1), n] coefficients in device (class-sorted) row order -> the caller's row order"""
    out = np.empty_like(coef_sorted)
    out[:, order] = coef_sorted
    return out


def _finite_matrix(X, name, d=None):
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] == 0 or X.shape[1] == 0:
        raise ValueError("%s must be a non-empty matrix [rows, features], got shape %s" % (name, X.shape))
    if d is not None and X.shape[1] != d:
        raise ValueError("%s has %d features, the model was fitted on %d" % (name, X.shape[1], d))
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    if not np.isfinite(X32).all():
        raise ValueError("%s holds non-finite values (or values beyond float32)" % name)
    return X32


class _DeviceSVM(E.DeviceCalls):
    """what RBFSVM and RBFSVMGroup share: the hyper-parameters and their checks; the library call on the current stream and
    the per-stage device-event timer are engine.DeviceCalls'"""

    def __init__(self, C, gamma, tol, max_iter, device):
        if not (isinstance(gamma, str) and gamma == 'auto') and not (np.isreal(gamma) and np.isfinite(gamma) and gamma > 0):
            raise ValueError("gamma must be 'auto' (1 / n_features, the reference's kernel width) or a positive number, got %r" % (gamma,))
        if not (np.isfinite(C) and C > 0 and np.isfinite(tol) and tol > 0):
            raise ValueError("C and tol must be positive, got C=%r tol=%r" % (C, tol))
        if int(max_iter) != max_iter or not 1 <= max_iter < 2 ** 31:
            raise ValueError("max_iter must be an integer in [1, 2^31), got %r" % (max_iter,))
        self.C, self.gamma, self.tol, self.max_iter, self.device = float(C), gamma, float(tol), int(max_iter), torch.device(device)
        self.times_ = {}                 # seconds of the last fit / predict per stage, filled only while time_stages is set
        self.time_stages = False


class _SingleSVM(_DeviceSVM):
    """one problem on the device, what RBFSVM and KernelSVM share: fit = kernel matrix + solve, chunked decide, the estimator's
    surface.  A subclass names itself (_name, for the messages) and supplies _gram(a, b) -> the kernel matrix between two
    row sets on the device, _solve(gram, n, K, iters) -> the solver launch, and may refuse class counts in _check_classes."""
    _name = None

    def _check_classes(self, classes, class_start):
        pass

    def _after_solve(self):
        pass

    # ---- the estimator ----
    def fit(self, X, y):
        X32 = _finite_matrix(X, "X")
        classes, order, class_start = class_sort(y)
        if len(y) != X32.shape[0]:
            raise ValueError("X has %d rows, y has %d labels" % (X32.shape[0], len(y)))
        K = len(classes)
        if not 2 <= K <= E.SVM_MAX_CLASSES:
            raise ValueError("%s needs 2 to %d classes, got %d" % (self._name, E.SVM_MAX_CLASSES, K))
        sizes = np.sort(np.diff(class_start))
        if sizes[-1] + sizes[-2] > E.SVM_MAX_PAIR:
            raise ValueError("the two largest classes have %d rows together; one one-vs-one problem holds at most %d "
                             "(MRGAN_SVM_MAX_PAIR)" % (sizes[-1] + sizes[-2], E.SVM_MAX_PAIR))
        self._check_classes(classes, class_start)
        self._require_gpu()
        n, d = X32.shape
        self._gamma = 1.0 / d if isinstance(self.gamma, str) else float(self.gamma)
        self.times_ = {}
        self._cs = (C.c_int64 * (K + 1))(*[int(v) for v in class_start])
        self._x = torch.from_numpy(X32[order]).to(self.device)
        self._coef = torch.empty((K - 1, n), dtype=torch.float64, device=self.device)
        self._rho = torch.empty(K * (K - 1) // 2, dtype=torch.float64, device=self.device)
        iters = torch.empty(K * (K - 1) // 2, dtype=torch.int32, device=self.device)
        gram = self._timed('gram', lambda: self._gram(self._x, self._x))
        self._timed('solve', lambda: self._solve(gram, n, K, iters))
        self.n_iter_ = iters.cpu().numpy()
        del gram
        self.dual_coef_dense_ = unsort_coef(self._coef.cpu().numpy(), order)
        self.intercept_ = -self._rho.cpu().numpy()
        self._after_solve()
        self.classes_, self._order, self.n_features_in_ = classes, order, d
        if (self.n_iter_ >= self.max_iter).any():
            warnings.warn("%s: %d of %d one-vs-one problems stopped at max_iter = %d before reaching tol = %g"
                          % (self._name, int((self.n_iter_ >= self.max_iter).sum()), len(self.n_iter_), self.max_iter, self.tol),
                          SVMConvergenceWarning, stacklevel=2)
        return self

    def _decide(self, X, chunk, want_dec):
        if self.classes_ is None:
            raise RuntimeError("%s: fit() first" % self._name)
        X32 = _finite_matrix(X, "X", self.n_features_in_)
        if chunk is None:
            chunk = 4096
        if int(chunk) != chunk or chunk < 1:
            raise ValueError("chunk must be a positive integer, got %r" % (chunk,))
        self._require_gpu()
        m, K, n = X32.shape[0], len(self.classes_), self._x.shape[0]
        pairs = K * (K - 1) // 2
        labels = torch.empty(m, dtype=torch.int32, device=self.device)
        dec = torch.empty((m, pairs), dtype=torch.float64, device=self.device) if want_dec else None

        def run():
            # the cross-Gram buffer holds one chunk of rows; every row's values depend on that row alone
            for r0 in range(0, m, int(chunk)):
                xt = torch.from_numpy(X32[r0:r0 + int(chunk)]).to(self.device)
                kt = self._gram(xt, self._x)
                self._call("mrgan_svm_decide", kt.data_ptr(), kt.stride(0), xt.shape[0], n, K, self._cs, self._coef.data_ptr(),
                           self._rho.data_ptr(), dec[r0:].data_ptr() if want_dec else None, labels[r0:].data_ptr())
        self._timed('predict', run)
        return labels.cpu().numpy(), (dec.cpu().numpy() if want_dec else None)

    def decision_function(self, X, chunk=None):
        """[rows, K (K - 1) / 2] one-vs-one decision values, columns in scikit-learn's 'ovo' order"""
        return self._decide(X, chunk, True)[1]

    def predict(self, X, chunk=None):
        """labels of the rows of X, worked in chunks of `chunk` rows (default 4096); chunk edges change no value"""
        return self.classes_[self._decide(X, chunk, False)[0]]

    def score(self, X, y, chunk=None):
        return float(np.mean(self.predict(X, chunk) == np.asarray(y)))


class RBFSVM(_SingleSVM):
    _name = 'RBFSVM'

    def __init__(self, C=1.0, gamma='auto', tol=1e-3, max_iter=10_000_000, device='cuda:0'):
        _DeviceSVM.__init__(self, C, gamma, tol, max_iter, device)
        self.classes_ = None

    def _gram(self, a, b):
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=self.device)
        self._call("mrgan_svm_gram", a.data_ptr(), a.stride(0), a.shape[0], b.data_ptr(), b.stride(0), b.shape[0], a.shape[1],
                   self._gamma, out.data_ptr(), out.stride(0))
        return out

    def _solve(self, gram, n, K, iters):
        self._call("mrgan_svm_solve", gram.data_ptr(), gram.stride(0), n, K, self._cs, self.C, self.tol, self.max_iter,
                   self._coef.data_ptr(), self._rho.data_ptr(), iters.data_ptr())


def nu_infeasible_pair(class_start, nu):
    """libsvm's svm_check_parameter for NU_SVC: nu (n_i + n_j) / 2 > min(n_i, n_j) makes the pair's start point impossible
    -> the first such pair of class indices (i, j), or None"""
    sizes = np.diff(np.asarray(class_start))
    for i in range(len(sizes)):
        for j in range(i + 1, len(sizes)):
            if nu * (sizes[i] + sizes[j]) / 2 > min(sizes[i], sizes[j]):
                return i, j
    return None


class KernelSVM(_SingleSVM):
    """The libsvm classifiers of the reference's SVM grid (others/wganlpctsemi.py:205-208) on the device, with RBFSVM's surface:

        KernelSVM(kernel='rbf' | 'linear', nu=None | float in (0, 1], C=1.0, gamma='auto', tol=1e-3, max_iter=10_000_000)

    nu=None is C-SVC (SVC(kernel=..., C=C)); a float is nu-SVC (NuSVC(kernel=..., nu=nu)) and C is unused.  gamma is the RBF
    kernel's width and unused by the linear kernel.  KernelSVM(kernel='rbf') gives RBFSVM's bits.  A nu fit adds r_ (per pair:
    dual_coef_dense_ * r_ is alpha y with alpha in [0, 1]) and raises ValueError where the solver returns non-finite
    coefficients (libsvm divides by an r it does not guard)."""
    _name = 'KernelSVM'

    def __init__(self, kernel='rbf', nu=None, C=1.0, gamma='auto', tol=1e-3, max_iter=10_000_000, device='cuda:0'):
        if kernel not in E.SVM_KERNELS:
            raise ValueError("kernel must be one of %s, got %r" % (sorted(E.SVM_KERNELS), kernel))
        if nu is not None and not (np.isreal(nu) and 0 < nu <= 1):
            raise ValueError("nu must be None (C-SVC) or a number in (0, 1], got %r" % (nu,))
        _DeviceSVM.__init__(self, C, gamma, tol, max_iter, device)
        self.kernel, self.nu = kernel, None if nu is None else float(nu)
        self.classes_, self.r_ = None, None

    def _check_classes(self, classes, class_start):
        bad = None if self.nu is None else nu_infeasible_pair(class_start, self.nu)
        if bad is not None:
            raise ValueError("specified nu is infeasible: nu = %g needs nu (n_i + n_j) / 2 <= min(n_i, n_j), which fails for classes %s and %s"
                             % (self.nu, classes[bad[0]], classes[bad[1]]))

    def _gram(self, a, b):
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=self.device)
        self._call("mrgan_svm_kernel_matrix", E.SVM_KERNELS[self.kernel], a.data_ptr(), a.stride(0), a.shape[0], b.data_ptr(), b.stride(0),
                   b.shape[0], a.shape[1], self._gamma, out.data_ptr(), out.stride(0))
        return out

    def _solve(self, gram, n, K, iters):
        if self.nu is None:
            self._r = None
            return RBFSVM._solve(self, gram, n, K, iters)
        self._r = torch.empty(K * (K - 1) // 2, dtype=torch.float64, device=self.device)
        self._call("mrgan_svm_solve_nu", gram.data_ptr(), gram.stride(0), n, K, self._cs, self.nu, self.tol, self.max_iter,
                   self._coef.data_ptr(), self._rho.data_ptr(), self._r.data_ptr(), iters.data_ptr())

    def _after_solve(self):
        self.r_ = None if self._r is None else self._r.cpu().numpy()
        if not (np.isfinite(self.dual_coef_dense_).all() and np.isfinite(self.intercept_).all()):
            self.classes_ = None
            raise ValueError("KernelSVM: the nu-SVC solver returned non-finite coefficients (r = %s): libsvm's r <= 0, nu = %g does "
                             "not suit this problem" % (self.r_, self.nu))


def plan_subgroups(nbytes, budget, max_group=E.SVM_MAX_GROUP):
    """consecutive sub-groups of the problems 0 .. len(nbytes) - 1, in order: at most max_group problems each and at most
    `budget` bytes of nbytes together; a single problem above the budget is a sub-group of its own -> list of index lists"""
    groups, cur, used = [], [], 0
    for p, b in enumerate(nbytes):
        if cur and (len(cur) == max_group or used + b > budget):
            groups.append(cur)
            cur, used = [], 0
        cur.append(p)
        used += b
    if cur:
        groups.append(cur)
    return groups


class _Fitted:
    """one problem of a fitted group: what a fitted RBFSVM / KernelSVM exposes (r_: the nu solver's r per pair, None for C-SVC)"""

    def __init__(self, classes, dual_coef_dense, intercept, n_iter, r=None):
        self.classes_, self.dual_coef_dense_, self.intercept_, self.n_iter_, self.r_ = classes, dual_coef_dense, intercept, n_iter, r


class _GroupSVM(_DeviceSVM):
    """several problems of one feature count and one class count in grouped launches, what RBFSVMGroup and KernelSVMGroup share:
    validation, sorting, uploads, the sub-group plan, chunked prediction through mrgan_svm_decide_group, the convergence
    warning.  A subclass names itself (_name), supplies _gram_group(items, count, d) -> the grouped kernel-matrix launch and
    _solve_group(sub, grams, K, iters) -> a callable that makes the grouped solver launch on the problems `sub`, and may
    refuse problems from their class counts in _check_problems (before any device call), prepare per-problem buffers in
    _before_solve and refuse results in _after_solve."""
    _name = None

    def __init__(self, C, gamma, tol, max_iter, device, gram_bytes):
        _DeviceSVM.__init__(self, C, gamma, tol, max_iter, device)
        if int(gram_bytes) != gram_bytes or gram_bytes < 1:
            raise ValueError("gram_bytes must be a positive integer, got %r" % (gram_bytes,))
        self.gram_bytes = int(gram_bytes)
        self._fitted = None

    def _check_problems(self, probs):
        pass

    def _before_solve(self, count, pairs):
        pass

    def _r_of(self, p):
        return None

    def _after_solve(self, fitted):
        pass

    def __len__(self):
        return 0 if self._fitted is None else len(self._fitted)

    def __getitem__(self, p):
        if self._fitted is None:
            raise RuntimeError("%s: fit() first" % self._name)
        return self._fitted[p]

    def fit(self, Xs, ys):
        if len(Xs) != len(ys) or len(Xs) == 0:
            raise ValueError("fit: %d row sets and %d label sets; a group needs as many of one as of the other, at least one" % (len(Xs), len(ys)))
        probs = []
        for p, (X, y) in enumerate(zip(Xs, ys)):
            X32 = _finite_matrix(X, "Xs[%d]" % p)
            classes, order, class_start = class_sort(y)
            if len(y) != X32.shape[0]:
                raise ValueError("Xs[%d] has %d rows, ys[%d] has %d labels" % (p, X32.shape[0], p, len(y)))
            K = len(classes)
            if not 2 <= K <= E.SVM_MAX_CLASSES:
                raise ValueError("%s needs 2 to %d classes, problem %d has %d" % (self._name, E.SVM_MAX_CLASSES, p, K))
            sizes = np.sort(np.diff(class_start))
            if sizes[-1] + sizes[-2] > E.SVM_MAX_PAIR:
                raise ValueError("the two largest classes of problem %d have %d rows together; one one-vs-one problem holds at most %d "
                                 "(MRGAN_SVM_MAX_PAIR)" % (p, sizes[-1] + sizes[-2], E.SVM_MAX_PAIR))
            probs.append((X32, classes, order, class_start))
        if len({q[0].shape[1] for q in probs}) != 1:
            raise ValueError("a group shares one feature count, got %s" % sorted({q[0].shape[1] for q in probs}))
        if len({len(q[1]) for q in probs}) != 1:
            raise ValueError("a group shares one class count, got %s" % sorted({len(q[1]) for q in probs}))
        self._check_problems(probs)
        self._require_gpu()
        d, K = probs[0][0].shape[1], len(probs[0][1])
        pairs = K * (K - 1) // 2
        self._gamma = 1.0 / d if isinstance(self.gamma, str) else float(self.gamma)
        self.times_ = {}
        self.n_features_in_, self._K = d, K
        self._cs = [(C.c_int64 * (K + 1))(*[int(v) for v in q[3]]) for q in probs]
        self._x = [torch.from_numpy(q[0][q[2]]).to(self.device) for q in probs]
        self._coef = [torch.empty((K - 1, len(x)), dtype=torch.float64, device=self.device) for x in self._x]
        self._rho = [torch.empty(pairs, dtype=torch.float64, device=self.device) for _ in probs]
        iters = [torch.empty(pairs, dtype=torch.int32, device=self.device) for _ in probs]
        self._before_solve(len(probs), pairs)
        for sub in plan_subgroups([4 * len(x) * len(x) for x in self._x], self.gram_bytes):
            grams = [torch.empty((len(self._x[p]), len(self._x[p])), dtype=torch.float32, device=self.device) for p in sub]
            gi = (E.SvmGramItem * len(sub))(*[E.SvmGramItem(self._x[p].data_ptr(), self._x[p].stride(0), len(self._x[p]),
                                                            self._x[p].data_ptr(), self._x[p].stride(0), len(self._x[p]),
                                                            g.data_ptr(), g.stride(0)) for p, g in zip(sub, grams)])
            solve = self._solve_group(sub, grams, K, iters)        # its descriptors are built outside the timed stage
            self._timed('gram', lambda: self._gram_group(gi, len(sub), d))
            self._timed('solve', solve)
            del grams                # back to the stream-ordered allocator: the next sub-group's launches come after these
        self._fitted = None
        fitted = [_Fitted(q[1], unsort_coef(self._coef[p].cpu().numpy(), q[2]), -self._rho[p].cpu().numpy(), iters[p].cpu().numpy(),
                          self._r_of(p)) for p, q in enumerate(probs)]
        self._after_solve(fitted)
        self._fitted = fitted
        late = [p for p, f in enumerate(self._fitted) if (f.n_iter_ >= self.max_iter).any()]
        if late:
            warnings.warn("%s: problems %s have one-vs-one pairs that stopped at max_iter = %d before reaching tol = %g"
                          % (self._name, late, self.max_iter, self.tol), SVMConvergenceWarning, stacklevel=2)
        return self

    def _decide(self, Xs, chunk, want_dec):
        if self._fitted is None:
            raise RuntimeError("%s: fit() first" % self._name)
        if len(Xs) != len(self._fitted):
            raise ValueError("the group was fitted on %d problems, got %d row sets" % (len(self._fitted), len(Xs)))
        X32 = [_finite_matrix(X, "Xs[%d]" % p, self.n_features_in_) for p, X in enumerate(Xs)]
        if chunk is None:
            chunk = 4096
        if int(chunk) != chunk or chunk < 1:
            raise ValueError("chunk must be a positive integer, got %r" % (chunk,))
        chunk = int(chunk)
        self._require_gpu()
        K, d = self._K, self.n_features_in_
        pairs = K * (K - 1) // 2
        labels = [torch.empty(len(x), dtype=torch.int32, device=self.device) for x in X32]
        dec = [torch.empty((len(x), pairs), dtype=torch.float64, device=self.device) if want_dec else None for x in X32]

        def run():
            # a chunk step takes rows r0 .. r0 + chunk - 1 of every problem of the sub-group that still has rows there; every
            # row's values depend on that row and its problem alone
            for sub in plan_subgroups([4 * min(chunk, len(X32[p])) * len(self._x[p]) for p in range(len(X32))], self.gram_bytes):
                for r0 in range(0, max(len(X32[p]) for p in sub), chunk):
                    live = [p for p in sub if r0 < len(X32[p])]
                    xt = [torch.from_numpy(X32[p][r0:r0 + chunk]).to(self.device) for p in live]
                    kt = [torch.empty((len(t), len(self._x[p])), dtype=torch.float32, device=self.device) for p, t in zip(live, xt)]
                    gi = (E.SvmGramItem * len(live))(*[E.SvmGramItem(t.data_ptr(), t.stride(0), len(t), self._x[p].data_ptr(),
                                                                     self._x[p].stride(0), len(self._x[p]), k.data_ptr(), k.stride(0))
                                                       for p, t, k in zip(live, xt, kt)])
                    di = (E.SvmDecideItem * len(live))(*[E.SvmDecideItem(k.data_ptr(), k.stride(0), len(t), len(self._x[p]), self._cs[p],
                                                                         self._coef[p].data_ptr(), self._rho[p].data_ptr(),
                                                                         dec[p][r0:].data_ptr() if want_dec else None, labels[p][r0:].data_ptr())
                                                         for p, t, k in zip(live, xt, kt)])
                    self._gram_group(gi, len(live), d)
                    self._call("mrgan_svm_decide_group", di, len(live), K)
        self._timed('predict', run)
        return [l.cpu().numpy() for l in labels], [v.cpu().numpy() if want_dec else None for v in dec]

    def decision_function(self, Xs, chunk=None):
        """per problem [rows, K (K - 1) / 2] one-vs-one decision values, columns in scikit-learn's 'ovo' order"""
        return self._decide(Xs, chunk, True)[1]

    def predict(self, Xs, chunk=None):
        """per problem the labels of the rows of Xs[p], worked in chunks of `chunk` rows (default 4096)"""
        return [f.classes_[l] for f, l in zip(self._fitted, self._decide(Xs, chunk, False)[0])]

    def score(self, Xs, ys, chunk=None):
        if len(ys) != len(Xs):
            raise ValueError("score: %d row sets and %d label sets" % (len(Xs), len(ys)))
        return [float(np.mean(l == np.asarray(y))) for l, y in zip(self.predict(Xs, chunk), ys)]


class RBFSVMGroup(_GroupSVM):
    """Independent RBFSVM problems of one feature count and one class count (the folds of a table cell), fitted and scored in
    grouped launches: mrgan_svm_gram_group, mrgan_svm_solve_group, mrgan_svm_decide_group serve up to 16 ragged problems
    each.  Problem p's results are those of RBFSVM(...).fit(Xs[p], ys[p]) bit for bit.

        group = RBFSVMGroup().fit(Xs, ys); errors = [1.0 - s for s in group.score(X_tests, y_tests)]; group[p].n_iter_

    More than 16 problems, or Gram matrices above gram_bytes together, are worked in consecutive sub-groups (plan_subgroups);
    prediction takes the problems' rows in chunks, one cross-Gram launch and one decide launch per chunk step of a sub-group.
    Neither changes a bit.  There is no CPU path."""
    _name = 'RBFSVMGroup'

    def __init__(self, C=1.0, gamma='auto', tol=1e-3, max_iter=10_000_000, device='cuda:0', gram_bytes=4 << 30):
        _GroupSVM.__init__(self, C, gamma, tol, max_iter, device, gram_bytes)

    def _gram_group(self, items, count, d):
        self._call("mrgan_svm_gram_group", items, count, d, self._gamma)

    def _solve_group(self, sub, grams, K, iters):
        si = (E.SvmSolveItem * len(sub))(*[E.SvmSolveItem(g.data_ptr(), g.stride(0), len(self._x[p]), self._cs[p], self._coef[p].data_ptr(),
                                                          self._rho[p].data_ptr(), iters[p].data_ptr()) for p, g in zip(sub, grams)])
        return lambda: self._call("mrgan_svm_solve_group", si, len(sub), K, self.C, self.tol, self.max_iter)


class KernelSVMGroup(_GroupSVM):
    """KernelSVM's kinds for a group of problems, with RBFSVMGroup's surface:

        KernelSVMGroup(kernel='rbf' | 'linear', nu=None | float in (0, 1] | one such float per problem, C=1.0, gamma='auto', ...)

    mrgan_svm_kernel_matrix_group makes the Gram and the cross-Gram matrices, mrgan_svm_solve_group (nu=None, C-SVC) or
    mrgan_svm_solve_nu_group (nu-SVC; nu travels per item, so a sequence gives every problem its own) solves, and
    mrgan_svm_decide_group votes.  Problem p's results are those of KernelSVM(kernel, nu_p, ...).fit(Xs[p], ys[p]) bit for bit,
    r_ included; KernelSVMGroup(kernel='rbf') gives RBFSVMGroup's bits.  A nu that is infeasible for a problem is a ValueError
    before any device call; non-finite coefficients in any problem are a ValueError that names the problems and leaves the
    group unfitted."""
    _name = 'KernelSVMGroup'

    def __init__(self, kernel='rbf', nu=None, C=1.0, gamma='auto', tol=1e-3, max_iter=10_000_000, device='cuda:0', gram_bytes=4 << 30):
        if kernel not in E.SVM_KERNELS:
            raise ValueError("kernel must be one of %s, got %r" % (sorted(E.SVM_KERNELS), kernel))
        if nu is not None and np.ndim(nu) == 0 and not (np.isreal(nu) and 0 < nu <= 1):
            raise ValueError("nu must be None (C-SVC) or a number in (0, 1], got %r" % (nu,))
        _GroupSVM.__init__(self, C, gamma, tol, max_iter, device, gram_bytes)
        self.kernel = kernel
        self.nu = None if nu is None else float(nu) if np.ndim(nu) == 0 else list(nu)        # a sequence is checked at fit

    def _check_problems(self, probs):
        self._nus = None
        if self.nu is None:
            return
        nus = [self.nu] * len(probs) if isinstance(self.nu, float) else self.nu
        if len(nus) != len(probs):
            raise ValueError("nu holds %d values, the group %d problems; a sequence needs one nu per problem" % (len(nus), len(probs)))
        for p, (nu, q) in enumerate(zip(nus, probs)):
            if not (np.ndim(nu) == 0 and np.isreal(nu) and 0 < nu <= 1):
                raise ValueError("nu must be None (C-SVC) or a number in (0, 1], got %r (problem %d)" % (nu, p))
            bad = nu_infeasible_pair(q[3], float(nu))
            if bad is not None:
                raise ValueError("specified nu is infeasible: nu = %g needs nu (n_i + n_j) / 2 <= min(n_i, n_j), which fails for classes %s and %s "
                                 "(problem %d)" % (nu, q[1][bad[0]], q[1][bad[1]], p))
        self._nus = [float(nu) for nu in nus]

    def _before_solve(self, count, pairs):
        self._r = None if self._nus is None else [torch.empty(pairs, dtype=torch.float64, device=self.device) for _ in range(count)]

    def _r_of(self, p):
        return None if self._r is None else self._r[p].cpu().numpy()

    def _gram_group(self, items, count, d):
        self._call("mrgan_svm_kernel_matrix_group", E.SVM_KERNELS[self.kernel], items, count, d, self._gamma)

    def _solve_group(self, sub, grams, K, iters):
        if self._nus is None:
            return RBFSVMGroup._solve_group(self, sub, grams, K, iters)
        si = (E.SvmSolveNuItem * len(sub))(*[E.SvmSolveNuItem(g.data_ptr(), g.stride(0), len(self._x[p]), self._cs[p], self._nus[p],
                                                              self._coef[p].data_ptr(), self._rho[p].data_ptr(), self._r[p].data_ptr(),
                                                              iters[p].data_ptr()) for p, g in zip(sub, grams)])
        return lambda: self._call("mrgan_svm_solve_nu_group", si, len(sub), K, self.tol, self.max_iter)

    def _after_solve(self, fitted):
        bad = [p for p, f in enumerate(fitted) if not (np.isfinite(f.dual_coef_dense_).all() and np.isfinite(f.intercept_).all())]
        if bad:
            raise ValueError("KernelSVMGroup: the nu-SVC solver returned non-finite coefficients in problems %s (libsvm's r <= 0: r = %s, "
                             "nu = %s): nu does not suit them" % (bad, [fitted[p].r_ for p in bad], [self._nus[p] for p in bad] if self._nus else None))
