"""Reference arithmetic of the input-gradient saliency (mrgan_input_gradient), on O.MRGANMirror.

input_gradient is the gradient of a per-row objective of the noise-free discriminator forward with respect to the input row;
heatmap restates the three lines the reference's others/mr_nn_activation_map.py applies to it (:132-135 normalize, :163
absolute value, :171 min-max), with the engine's rule for a constant row."""
import functools

import numpy as np

from oracle import mrgan_oracle as O
from tests.helpers import Case

OBJECTIVES = ('logit', 'xent', 'mse')
B = 50                                # local batch of every handle of the GPU tests: S = 128, so padding rows exist
WIDE_HEAD = (256, 256, 256, 256, 512)  # a feature layer of two HEAD_CHUNKs
DECIDED = 1e-5                        # a row is decided when every fp64 pre-activation is at least this far from zero


def dlogits(logits, targets, objective):
    """per-row d objective / d logits at target class targets[i]: no batch mean"""
    n, K = logits.shape
    onehot = np.zeros_like(logits)
    onehot[np.arange(n), targets] = 1.0
    if objective == 'logit':
        return onehot
    if objective == 'xent':
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True) - onehot
    if objective == 'mse':
        return 2.0 * (logits - onehot) / K
    raise ValueError(objective)


def input_gradient(d, x, targets, objective, quantize=None):
    """d: the discriminator's tensors (Keras order); x [n, D]; targets [n] or None (the argmax of the logits, ties to the first
    class).  quantize None: the exact gradient in x's precision; 'bf16': rounded where the engine stores bf16 (the layer-0 dX
    it hands to the finishing kernel included).
    -> (gradient [n, D], logits [n, K], targets used, the forward's cache)"""
    mir = O.MRGANMirror([], d, quantize=quantize)
    c = mir._disc_fwd(mir.q(x), None, None)
    W6, b6 = mir.d[-2], mir.d[-1]
    logits = c['feat_q'] @ W6 + b6
    t = np.argmax(logits, axis=1) if targets is None else np.asarray(targets)
    dl = dlogits(logits, t, objective)
    dp = (dl @ W6.T) * (c['feat_q'] > 0)
    _, _, dx = mir._disc_bwd(c, dp, None, to_input=True)
    return mir.q(dx), logits, t.astype(np.int32), c


def preactivations(d, x):
    """the five pre-activations of the noise-free forward, unrounded"""
    pre, a = [], x
    for l in range(len(d) // 2 - 1):
        pre.append(a @ d[2 * l] + d[2 * l + 1])
        a = O.relu(pre[-1])
    return pre


def heatmap(g):
    """rows of gradients -> rows in [0, 1]: g / (rms + 1e-5), absolute value, min-max over the row; a constant row -> zeros"""
    g = np.asarray(g)
    ghat = g / (np.sqrt(np.mean(np.square(g), axis=1, keepdims=True)) + g.dtype.type(1e-5))
    a = np.abs(ghat)
    lo, hi = a.min(axis=1, keepdims=True), a.max(axis=1, keepdims=True)
    rng = hi - lo
    return np.where(rng > 0, (a - lo) / np.where(rng > 0, rng, 1), 0).astype(g.dtype)


# ---- the shared problems of the CPU and GPU tests of mrgan_input_gradient and mrgan_attribution (never modified) -----
@functools.lru_cache(maxsize=None)
def problem(K, D, d_hidden=None, n=130):
    """(case, n rows as the engine gets them)"""
    kw = dict(d_hidden=d_hidden) if d_hidden else {}
    case = Case(K=K, D=D, B=B, steps=1, **kw)
    x32 = np.random.default_rng(3).standard_normal((n, D)).astype(np.float32)
    return case, x32


@functools.lru_cache(maxsize=None)
def decided_problem(K, D, n, d_hidden=None):
    """(case, rows as the engine gets them, the same rows in fp64, decided rows)"""
    case, x32 = problem(K, D, d_hidden, n)
    x = x32.astype(np.float64)
    decided = np.all([np.abs(p).min(axis=1) >= DECIDED for p in preactivations(case.d0, x)], axis=0)
    return case, x32, x, decided


@functools.lru_cache(maxsize=None)
def reference(K, D, n, objective, planted, quantize=None, d_hidden=None):
    """fp64 (or mirror) gradient at the fp64 argmax, or at planted targets (argmax + 1)"""
    case, _, x, _ = decided_problem(K, D, n, d_hidden)
    t = input_gradient(case.d0, x, None, objective)[2]
    if planted:
        t = ((t + 1) % K).astype(np.int32)
    g, _, t, _ = input_gradient(case.d0, x, t, objective, quantize=quantize)
    return g, t
