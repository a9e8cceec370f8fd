"""fp64 numpy restatement of what csrc/svm.hip adds to the RBF C-SVC of tests/svm_ref.py: the linear Gram matrix and libsvm's
nu-SVC (solve_nu_svc and Solver_NU without shrinking) on a precomputed kernel matrix.

    start point    in pair-local order (class i's rows first, y = +1), per sign: alpha_t = min(1, remaining), remaining starting
                   at nu l / 2; p = 0, Cp = Cn = 1
    gradient       G_t = sum over alpha_s > 0, ascending s, of alpha_s (float)(y_s y_t K_st)
    selection      Gmaxp / Gmaxn with ip / in per sign, j by the second-order rule inside its own sign, i = ip or in by j's sign,
                   ties to the higher index (libsvm scans upwards with >= and <=)
    update         libsvm's equal-sign branch with bound 1
    rho, r         r1, r2 from the free variables of each sign (else the midpoint of the sign's bounds); r = (r1 + r2) / 2,
                   rho = (r1 - r2) / 2; the model is coef = alpha y / r with rho / r

Kernel values are float32 wherever a solver reads them, alpha and G are float64, as in svm_ref.py."""
import numpy as np

from tests import svm_ref as R

TAU = R.TAU


def linear_gram(A, B):
    """A_a . B_b in fp64"""
    return np.asarray(A, np.float64) @ np.asarray(B, np.float64).T


def nu_feasible(class_start, nu):
    """libsvm's svm_check_parameter: every pair needs nu (n_i + n_j) / 2 <= min(n_i, n_j) -> the first infeasible pair, or None"""
    sizes = np.diff(np.asarray(class_start))
    for i, j in R.ovo_pairs(len(sizes)):
        if nu * (sizes[i] + sizes[j]) / 2 > min(sizes[i], sizes[j]):
            return (i, j)
    return None


def nu_start(y, nu):
    alpha = np.zeros(len(y))
    for sign in (1.0, -1.0):
        remaining = nu * len(y) / 2
        for t in np.flatnonzero(y == sign):
            alpha[t] = min(1.0, remaining)
            remaining -= alpha[t]
    return alpha


def nu_gradient(Kp, y, alpha):
    """G = Q alpha from scratch (p = 0), Q = y y^T K"""
    return y * (np.asarray(Kp, np.float64) @ (y * alpha))


def _sides(y, alpha, G):
    """per sign: (max of -G over the rows that may grow, max of G over the rows that may shrink) for y = +1, and the mirrored
    pair for y = -1 (libsvm's Gmaxp, Gmaxp2, Gmaxn, Gmaxn2)"""
    pos, neg = y > 0, y < 0
    def mx(v, m):
        return v[m].max() if m.any() else -np.inf
    return (mx(-G, pos & (alpha < 1)), mx(G, pos & (alpha > 0)), mx(G, neg & (alpha > 0)), mx(-G, neg & (alpha < 1)))


def nu_kkt_gap(Kp, y, alpha):
    """max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) with G recomputed from scratch: Solver_NU stops below tol"""
    gp, gp2, gn, gn2 = _sides(y, alpha, nu_gradient(Kp, y, alpha))
    return max(gp + gp2, gn + gn2)


def nu_calculate_rho(y, G, alpha):
    """-> rho, r of Solver_NU::calculate_rho"""
    r12 = []
    for sign in (1.0, -1.0):
        m = y == sign
        upper, lower = m & (alpha >= 1), m & (alpha <= 0)
        free = m & ~upper & ~lower
        if free.any():
            r12.append(G[free].sum() / free.sum())
        else:
            ub = G[lower].min() if lower.any() else np.inf
            lb = G[upper].max() if upper.any() else -np.inf
            r12.append((ub + lb) / 2)
    return (r12[0] - r12[1]) / 2, (r12[0] + r12[1]) / 2


def _last_argmax(v):
    return int(np.flatnonzero(v == v.max())[-1])


def smo_nu(Kp, y, nu, tol, max_iter):
    """-> alpha (in [0, 1], before the division by r), rho, r, iterations.  Kp: the pair's kernel matrix (read as float32)"""
    Kp = np.asarray(Kp, np.float32).astype(np.float64)
    QD = np.diag(Kp).copy()
    alpha = nu_start(y, nu)
    G = np.zeros(len(y))
    for s in np.flatnonzero(alpha > 0):
        G += alpha[s] * (y[s] * y * Kp[s])
    pos, neg = y > 0, y < 0
    it = 0
    while it < max_iter:
        gp, gp2, gn, gn2 = _sides(y, alpha, G)
        ip = _last_argmax(np.where(pos & (alpha < 1), -G, -np.inf)) if gp > -np.inf else -1
        im = _last_argmax(np.where(neg & (alpha > 0), G, -np.inf)) if gn > -np.inf else -1
        obj = np.full(len(y), -np.inf)
        for lead, side, gmax, sgn in ((ip, pos & (alpha > 0), gp, 1.0), (im, neg & (alpha < 1), gn, -1.0)):
            if lead < 0:
                continue
            gd = gmax + sgn * G
            cand = side & (gd > 0)
            q = QD[lead] + QD - 2.0 * Kp[lead]
            q = np.where(q > 0, q, TAU)
            obj = np.where(cand, gd * gd / q, obj)
        if max(gp + gp2, gn + gn2) < tol or not (obj > -np.inf).any():
            break
        j = _last_argmax(obj)
        i = ip if y[j] > 0 else im
        qij = QD[i] + QD[j] - 2.0 * Kp[i, j]
        if not qij > 0:
            qij = TAU
        ai, aj = alpha[i], alpha[j]
        delta, s = (G[i] - G[j]) / qij, ai + aj
        ni, nj = ai - delta, aj + delta
        if s > 1:
            if ni > 1:
                ni, nj = 1.0, s - 1
        elif nj < 0:
            nj, ni = 0.0, s
        if s > 1:
            if nj > 1:
                nj, ni = 1.0, s - 1
        elif ni < 0:
            ni, nj = 0.0, s
        alpha[i], alpha[j] = ni, nj
        G += Kp[i] * (y[i] * y) * (ni - ai) + Kp[j] * (y[j] * y) * (nj - aj)
        it += 1
    rho, r = nu_calculate_rho(y, G, alpha)
    return alpha, rho, r, it


def solve_ovo_nu(Kmat, class_start, nu, tol, max_iter=10_000_000):
    """the whole one-vs-one problem on a class-sorted kernel matrix -> coef [(K-1), n] (alpha y / r in libsvm's sv_coef rows),
    rho / r [pairs], r [pairs], iterations [pairs]"""
    num_classes, n = len(class_start) - 1, int(class_start[-1])
    coef, rho, rs, iters = np.zeros((num_classes - 1, n)), [], [], []
    for i, j in R.ovo_pairs(num_classes):
        rows, y = R.pair_rows(class_start, i, j)
        alpha, rh, r, it = smo_nu(np.asarray(Kmat)[np.ix_(rows, rows)], y, nu, tol, max_iter)
        ni = class_start[i + 1] - class_start[i]
        coef[j - 1, rows[:ni]] = alpha[:ni] * (1.0 / r)          # libsvm: alpha[i] *= y[i] / r
        coef[i, rows[ni:]] = alpha[ni:] * (-1.0 / r)
        rho.append(rh / r)
        rs.append(r)
        iters.append(it)
    return coef, np.array(rho), np.array(rs), np.array(iters)
