"""fp64 restatements of the operations behind the non-GEMM kernels (csrc/aux_kernels.hip), written from the reference
arithmetic (mr_gan.py:112, :128, :146-154, :161-167; mr_nn.py:112) and tied to oracle/mrgan_oracle.py by
tests/test_aux_refs_cpu.py.  tests/test_aux_kernels.py holds the kernels to them.  numpy only; every argument is taken as float64.
"""
import numpy as np

LAB, UNL, FAKE, EVAL, LOGITS, MSE = range(6)          # segment kinds of the loss head (csrc/aux_kernels.h)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- BatchNorm with batch statistics and the biased variance (mr_gan.py:112) ----
def bn_stats(s1, s2, count, eps):
    """column sums of h and h^2 over `count` rows -> (mean, biased variance, 1 / sqrt(var + eps)).  E[h^2] - mean^2 is the biased
    variance; below zero it can only be rounding, hence the clamp."""
    mean = _f64(s1) / count
    var = np.maximum(_f64(s2) / count - mean * mean, 0.0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def bn_apply(h, mean, rstd, gamma, beta):
    return _f64(gamma) * ((_f64(h) - mean) * rstd) + _f64(beta)


def bn_bwd(dy, h, mean, rstd, gamma, count, sum_dy=None, sum_dy_xhat=None):
    """gradient of the loss w.r.t. the pre-activation of the softplus layer in front of the BatchNorm, h = softplus(pre):
    dh = gamma rstd / count (count dy - sum dy - xhat sum(dy xhat)), dpre = dh sigmoid(pre) = dh (1 - exp(-h)).
    The two column sums default to those of dy itself (one shard holds the whole batch) -> (dpre, dbeta, dgamma)"""
    dy, h = _f64(dy), _f64(h)
    xhat = (h - mean) * rstd
    dbeta = dy.sum(axis=0) if sum_dy is None else _f64(sum_dy)
    dgamma = (dy * xhat).sum(axis=0) if sum_dy_xhat is None else _f64(sum_dy_xhat)
    dh = (_f64(gamma) * rstd / count) * (count * dy - dbeta - xhat * dgamma)
    return dh * -np.expm1(-h), dbeta, dgamma


# ---- loss head (mr_gan.py:128, :146-149, :161; mr_nn.py:112) ----
def _lse(l):
    m = l.max(axis=1)
    return m + np.log(np.exp(l - m[:, None]).sum(axis=1))


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def head_rows(logits, kind, labels, inv_count, unl_weight=1.0):
    """per row of one segment: (labeled / MSE loss term, unlabeled / fake loss term, train error, dlogits [rows][classes]).
    The segment's losses are the row terms summed times inv_count; dlogits carry inv_count already.  A label of -1 (MSE: the
    padding rows of a short batch) contributes to nothing.  argmax ties go to the first index."""
    l = _f64(logits)
    B, K = l.shape
    loss0, loss1, err, dl = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros((B, K))
    am = np.argmax(l, axis=1)
    if kind in (LAB, EVAL, MSE):
        y = np.asarray(labels).astype(np.int64)
        live = y >= 0 if kind == MSE else np.ones(B, bool)
        onehot = np.zeros((B, K))
        onehot[np.arange(B)[live], y[live]] = 1.0
        err = (live & (am != y)).astype(np.float64)
    if kind == LOGITS or kind == EVAL:
        return loss0, loss1, err, dl
    if kind == MSE:
        d = (l - onehot) * live[:, None]
        return (d * d).mean(axis=1), loss1, err, 2.0 * d / K * inv_count
    lse = _lse(l)
    p = np.exp(l - lse[:, None])
    if kind == LAB:
        return lse - l[np.arange(B), y], loss1, err, (p - onehot) * inv_count
    sg = _sigmoid(lse)
    if kind == UNL:
        return loss0, 0.5 * (_softplus(lse) - lse), err, 0.5 * inv_count * unl_weight * (sg - 1.0)[:, None] * p
    return loss0, 0.5 * _softplus(lse), err, 0.5 * inv_count * unl_weight * sg[:, None] * p


def head_backward(f, w6, dlogits, live=None):
    """last dense backwards: (dW6, db6, dL/d(pre5), bias gradient of the feature layer); `live` = the feature layer's relu
    mask, by default f > 0"""
    f, w6, dl = _f64(f), _f64(w6), _f64(dlogits)
    dpre = (dl @ w6.T) * ((f > 0) if live is None else live)
    return f.T @ dl, dl.sum(axis=0), dpre, dpre.sum(axis=0)


# ---- feature matching (mr_gan.py:152-154) ----
def fm(sum_fake, sum_real, count, grad_scale=1.0):
    """column sums of the features over `count` fake and `count` real rows -> (loss, dL/df of every fake row [feat])"""
    diff = (_f64(sum_fake) - _f64(sum_real)) / count
    return float(np.mean(diff * diff)), grad_scale * 2.0 / (diff.size * count) * diff


# ---- Keras 2.0.9 Adam (mr_gan.py:165-167): eps outside the square root, the bias correction inside lr_t ----
def adam_lr_t(lr, b1, b2, iterations):
    """the step size of the update made at Keras `iterations` (t = iterations + 1)"""
    t = float(iterations) + 1.0
    return lr * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)


def adam(p, m, v, g, lr_t, b1, b2, eps):
    g = _f64(g)
    m = b1 * _f64(m) + (1.0 - b1) * g
    v = b2 * _f64(v) + (1.0 - b2) * g * g
    return _f64(p) - lr_t * m / (np.sqrt(v) + eps), m, v
