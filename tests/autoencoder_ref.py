"""The autoencoder step (mrgan_ae_step: others/mr_gan_autoencoder.py:109-127 of the reference) restated in numpy.

  * the fp64 restatement: forward, mse, closed-form backward and one step with the oracle's Keras Adam, on the oracle's own
    discriminator forward / backward with the last layer d_in wide;
  * the MIRROR: the same algebra with `q` (O.bf16_round) exactly where the engine stores bf16 -- the staged input, the six
    weights, every activation including y, dY and every stored dpre.  The loss and dY come from the stored y against the
    caller's UNROUNDED row; the last bias gradient sums the stored dY (the reconstruction head sums what it stores), the five
    others the unrounded dpre (the dX epilogue's column sums).  q = identity gives the restatement again.
"""
import numpy as np

from oracle import mrgan_oracle as O

AE_LR, AE_B1 = 0.001, 0.9                    # Keras' Adam defaults (compile(optimizer='adam'))


def widths(nodes):
    """n0 n1 n2 -> the five hidden widths n0 n1 n2 n1 n0"""
    n0, n1, n2 = nodes
    return (n0, n1, n2, n1, n0)


def init(D, nodes, seed, dtype=np.float64):
    """six (W, b) pairs D -> n0 -> n1 -> n2 -> n1 -> n0 -> D: glorot weights, and nonzero biases so every path carries signal"""
    rng = np.random.default_rng(seed)
    d = []
    for (shape_w, shape_b) in zip(O.d_shapes(D, widths(nodes), K=D)[0::2], O.d_shapes(D, widths(nodes), K=D)[1::2]):
        d.append(O.glorot_uniform(rng, shape_w[0], shape_w[1], dtype))
        d.append((0.05 * rng.standard_normal(shape_b)).astype(dtype))
    return d


def _ident(x):
    return x


# ---- the fp64 restatement -----------------------------------------------------------------------------------------------
def forward(d, x):
    """-> (y, cache of O.disc_forward): relu after the first five layers, linear last, no noise"""
    y, _, cache = O.disc_forward(d, x, noise=None)
    return y, cache


def encode(d, x):
    """the relu output of dense 3"""
    return forward(d, x)[1]['ins'][3]


def grads(d, x, rows_valid=None):
    """Keras 'mse' over the first rows_valid rows -> (loss, the 12 gradients)"""
    B, D = x.shape
    rv = B if not rows_valid else rows_valid
    y, cache = forward(d, x)
    diff = y - x
    diff[rv:] = 0.0
    loss = float((diff * diff).sum() / (rv * D))
    g, _ = O.disc_backward(d, cache, dlogits=(2.0 / (rv * D)) * diff)
    return loss, g


class Restatement(object):
    """weights + Keras Adam: step(x, rows_valid) is one train_on_batch(x, x)"""

    def __init__(self, d0, lr=AE_LR, b1=AE_B1):
        self.d = [p.copy() for p in d0]
        self.adam = O.Adam([], self.d, lr=lr, b1=b1)

    def grads(self, x, rows_valid=None):
        return grads(self.d, x, rows_valid)

    def step(self, x, rows_valid=None):
        loss, g = self.grads(x, rows_valid)
        self.adam.apply(self.d, g, 'd')
        return loss

    def encode(self, x):
        return encode(self.d, x)

    def reconstruct(self, x):
        return forward(self.d, x)[0]


# ---- the mirror ---------------------------------------------------------------------------------------------------------
class Mirror(Restatement):
    """the engine's dataflow with the storage rounding q (default bf16; None: no rounding, the restatement's numbers)"""

    def __init__(self, d0, q=O.bf16_round, **adam):
        Restatement.__init__(self, d0, **adam)
        self.q = q or _ident

    def _forward(self, x):
        q = self.q
        a, ins, pres = q(x), [], []
        for l in range(5):
            ins.append(a)
            pre = a @ q(self.d[2 * l]) + self.d[2 * l + 1]
            pres.append(pre)
            a = q(O.relu(pre))
        y = q(a @ q(self.d[10]) + self.d[11])
        return y, a, ins, pres

    def grads(self, x, rows_valid=None):
        q = self.q
        B, D = x.shape
        rv = B if not rows_valid else rows_valid
        y, feat, ins, pres = self._forward(x)
        diff = y - x                                               # the caller's row, not the staged copy
        diff[rv:] = 0.0
        loss = float((diff * diff).sum() / (rv * D))
        dy = q((2.0 / (rv * D)) * diff)
        g = [None] * 12
        g[10], g[11] = feat.T @ dy, dy.sum(axis=0)
        da = dy @ q(self.d[10]).T
        for l in range(4, -1, -1):
            dpre = da * (pres[l] > 0)
            g[2 * l + 1] = dpre.sum(axis=0)
            dpre = q(dpre)
            g[2 * l] = ins[l].T @ dpre
            da = dpre @ q(self.d[2 * l]).T
        return loss, g

    def encode(self, x):
        return self._forward(x)[2][3]

    def reconstruct(self, x):
        return self._forward(x)[0]
