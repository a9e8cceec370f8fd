"""Reference arithmetic of the input-gradient saliency (mrgan_input_gradient), on O.MRGANMirror.

input_gradient is the gradient of a per-row objective of the noise-free discriminator forward with respect to the input row;
heatmap restates the three lines the reference's others/mr_nn_activation_map.py applies to it (:132-135 normalize, :163
absolute value, :171 min-max), with the engine's rule for a constant row."""
import numpy as np

from oracle import mrgan_oracle as O

OBJECTIVES = ('logit', 'xent', 'mse')


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
