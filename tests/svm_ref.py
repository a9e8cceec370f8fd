"""fp64 numpy restatement of csrc/svm.hip: the RBF Gram matrix, the one-vs-one split of a class-sorted problem, the KKT gap,
libsvm's calculate_rho, decision values and votes from dense coefficients, and a plain SMO of the same algorithm (libsvm's
C-SVC Solver without shrinking: WSS2 selection, ties to the highest index, libsvm's clipping order).

Kernel values are float32 everywhere a solver reads them (libsvm's Qfloat; the device Gram matrix); alpha and G are float64."""
import numpy as np

TAU = 1e-12


def rbf_gram(A, B, gamma):
    """exp(-gamma max(0, |a|^2 + |b|^2 - 2 a.b)) in fp64"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    return np.exp(-float(gamma) * np.maximum(d2, 0.0))


def ovo_pairs(num_classes):
    """(i, j), i < j, in libsvm's order = the columns of scikit-learn's decision_function_shape='ovo'"""
    return [(i, j) for i in range(num_classes) for j in range(i + 1, num_classes)]


def pair_rows(class_start, i, j):
    """rows of pair (i, j) in the class-sorted order and their y (+1 on class i)"""
    a, b = np.arange(class_start[i], class_start[i + 1]), np.arange(class_start[j], class_start[j + 1])
    return np.concatenate([a, b]), np.concatenate([np.ones(len(a)), -np.ones(len(b))])


def gradient(Kp, y, alpha):
    """G = Q alpha - e from scratch, Q = y y^T K"""
    return y * (np.asarray(Kp, np.float64) @ (y * alpha)) - 1.0


def up_low(y, alpha, C):
    up = np.where(y > 0, alpha < C, alpha > 0)
    low = np.where(y > 0, alpha > 0, alpha < C)
    return up, low


def kkt_gap(Kp, y, alpha, C):
    """max over I_up of -y G  -  min over I_low of -y G, with G recomputed from scratch (the solver stops below tol)"""
    v = -y * gradient(Kp, y, alpha)
    up, low = up_low(y, alpha, C)
    if not up.any() or not low.any():
        return -np.inf
    return v[up].max() - v[low].min()


def calculate_rho(y, G, alpha, C):
    yG = y * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        return yG[free].sum() / free.sum()
    ub_set = (upper & (y < 0)) | (lower & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & (y < 0))
    ub = yG[ub_set].min() if ub_set.any() else np.inf
    lb = yG[lb_set].max() if lb_set.any() else -np.inf
    return (ub + lb) / 2


def _last_argmax(v):
    return int(np.flatnonzero(v == v.max())[-1])


def smo(Kp, y, C, tol, max_iter):
    """-> alpha, rho, iterations.  Kp: the pair's kernel matrix (read as float32), y: +-1"""
    Kp = np.asarray(Kp, np.float32).astype(np.float64)
    l = len(y)
    QD = np.diag(Kp).copy()
    alpha, G = np.zeros(l), -np.ones(l)
    it = 0
    while it < max_iter:
        up, low = up_low(y, alpha, C)
        if not up.any():
            break
        v = np.where(up, -y * G, -np.inf)
        i = _last_argmax(v)
        Gmax = v[i]
        yG = y * G
        if not low.any():
            break
        Gmax2 = yG[low].max()
        gd = Gmax + yG
        cand = low & (gd > 0)
        if Gmax + Gmax2 < tol or not cand.any():
            break
        q = QD[i] + QD - 2.0 * Kp[i]
        q = np.where(q > 0, q, TAU)
        obj = np.where(cand, gd * gd / q, -np.inf)
        j = _last_argmax(obj)
        qij = QD[i] + QD[j] - 2.0 * Kp[i, j]
        if not qij > 0:
            qij = TAU
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            delta, diff = (-G[i] - G[j]) / qij, ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0.0, diff
            elif ni < 0:
                ni, nj = 0.0, -diff
            if diff > 0:
                if ni > C:
                    ni, nj = C, C - diff
            elif nj > C:
                nj, ni = C, C + diff
        else:
            delta, s = (G[i] - G[j]) / qij, ai + aj
            ni, nj = ai - delta, aj + delta
            if s > C:
                if ni > C:
                    ni, nj = C, s - C
            elif nj < 0:
                nj, ni = 0.0, s
            if s > C:
                if nj > C:
                    nj, ni = C, s - C
            elif ni < 0:
                ni, nj = 0.0, s
        alpha[i], alpha[j] = ni, nj
        G += Kp[i] * (y[i] * y) * (ni - ai) + Kp[j] * (y[j] * y) * (nj - aj)
        it += 1
    return alpha, calculate_rho(y, G, alpha, C), it


def solve_ovo(Kmat, class_start, C, tol, max_iter=10_000_000):
    """the whole one-vs-one problem on a class-sorted kernel matrix -> coef [(K-1), n] (alpha y in libsvm's sv_coef rows),
    rho [pairs], iterations [pairs]"""
    num_classes, n = len(class_start) - 1, int(class_start[-1])
    coef, rho, iters = np.zeros((num_classes - 1, n)), [], []
    for i, j in ovo_pairs(num_classes):
        rows, y = pair_rows(class_start, i, j)
        alpha, r, it = smo(np.asarray(Kmat)[np.ix_(rows, rows)], y, C, tol, max_iter)
        ni = class_start[i + 1] - class_start[i]
        coef[j - 1, rows[:ni]] = alpha[:ni]
        coef[i, rows[ni:]] = -alpha[ni:]
        rho.append(r)
        iters.append(it)
    return coef, np.array(rho), np.array(iters)


def pair_alpha(coef, class_start, i, j):
    """the pair's alpha (>= 0) out of the dense coefficients, in pair_rows order"""
    rows, y = pair_rows(class_start, i, j)
    ni = class_start[i + 1] - class_start[i]
    return np.concatenate([coef[j - 1, rows[:ni]], coef[i, rows[ni:]]]) * y


def decisions(coef, rho, Kt, class_start):
    """[m, pairs]: sum_t coef_t K(x, x_t) - rho over the pair's two class ranges, fp64"""
    Kt = np.asarray(Kt, np.float64)
    num_classes = len(class_start) - 1
    out = np.empty((Kt.shape[0], num_classes * (num_classes - 1) // 2))
    for p, (i, j) in enumerate(ovo_pairs(num_classes)):
        a, b = slice(class_start[i], class_start[i + 1]), slice(class_start[j], class_start[j + 1])
        out[:, p] = Kt[:, a] @ coef[j - 1, a] + Kt[:, b] @ coef[i, b] - rho[p]
    return out


def vote(dec, num_classes):
    """class index per row: i where dec > 0 else j; the first class with the most votes"""
    votes = np.zeros((dec.shape[0], num_classes), np.int64)
    for p, (i, j) in enumerate(ovo_pairs(num_classes)):
        pos = dec[:, p] > 0
        votes[pos, i] += 1
        votes[~pos, j] += 1
    return votes.argmax(1)


def dense_from_svc(svc, n):
    """SVC.support_ / dual_coef_ -> [(K-1), n] in the row order the SVC was fitted on (multi-class convention; scikit-learn
    flips the sign of a two-class model, undone here)"""
    dense = np.zeros((svc.dual_coef_.shape[0], n))
    dense[:, svc.support_] = svc.dual_coef_ if len(svc.classes_) > 2 else -svc.dual_coef_
    return dense


def mreo_labeled(d, trials, per, sep, gamma):
    """six classes of synthetic_mreo(objects_per_class=4), standard-scaled, the first `per` rows per class (float32 rows)
    -> x, y, class_start, the fp64 Gram matrix rounded to float32"""
    from mr_gan_amd import synthetic_mreo
    X, y, _ = synthetic_mreo(d=d, trials=trials, objects_per_class=4, sep=sep)
    X = (X - X.mean(0)) / X.std(0)
    xl = np.concatenate([X[y == c][:per] for c in range(6)]).astype(np.float32)
    return xl, np.repeat(np.arange(6), per), np.arange(7) * per, rbf_gram(xl, xl, gamma).astype(np.float32)
