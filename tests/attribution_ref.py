"""Reference arithmetic of mrgan_attribution (SmoothGrad and integrated gradients accumulated on the device), on O.MRGANMirror.

Draw d of a call is one input gradient of tests/saliency_ref.py at a forward of its own: method 'noise' adds the GaussianNoise of
the five sites, drawn at (site, segment 255, step d, row0 = 0 over all n rows of the call); method 'path' evaluates the noise-free
forward at v = fmaf(alpha_d, x - b, b), alpha_d = (d + 0.5f) / (float)draws in fp32, as include/mrgan_abi.h states it.  The mean
over draws is taken in fp64."""
import functools

import numpy as np

from oracle import mrgan_oracle as O
from tests import saliency_ref as R
from tests.helpers import SEED

NOISE_SEG = 255                       # MRGAN_ATTR_NOISE_SEG
DECIDED = R.DECIDED                   # a row is decided when every fp64 pre-activation of every draw is at least this far from zero
B, N, DRAWS = R.B, 130, 3             # S = 128: two chunks of 128 + 2 rows
WIDE_HEAD = R.WIDE_HEAD
SHAPES = [(6, 72, None), (10, 400, None), (6, 96, WIDE_HEAD)]                      # (K, D, d_hidden) of the fp32 tests
BF16_SHAPES = [(6, 400, None), (10, 96, None), (6, 96, WIDE_HEAD)]                 # those of the bf16 saliency tests
OWN = (0.3, 0.5)                      # mrgan_config.sigma: input, hidden
# name -> (method, (sigma_input, sigma_hidden), baseline, multiply); 'random' = standard normals of default_rng(5)
MODES = {'own': ('noise', OWN, None, 0), 'input': ('noise', (0.3, 0.0), None, 0),
         'path0': ('path', (0.0, 0.0), None, 1), 'pathb': ('path', (0.0, 0.0), 'random', 1)}


def path_point(x32, b32, d, draws):
    """fp32 v = fmaf(alpha_d, x - b, b): the difference rounded to fp32, the product exact in fp64 (24 x 24 bits), one sum"""
    alpha = np.float32((np.float32(d) + np.float32(0.5)) / np.float32(draws))
    diff = (x32 - b32).astype(np.float32)
    return (np.float64(alpha) * diff.astype(np.float64) + b32.astype(np.float64)).astype(np.float32)


def attribution(d, x32, targets, objective, method, draws, sigmas=(0.0, 0.0), baseline=None, multiply=0, quantize=None,
                seed=SEED, normal=O.device_normal, noise_fn=None):
    """d: the discriminator's tensors; x32 [n, D] float32; targets [n] or None (the argmax of the noise-free forward at x).
    noise_fn(site, draw, cols) -> [n, cols]: the normals to use instead of normal(seed, site, 255, draw, n, cols).
    -> (attribution [n, D] float64, targets used, per-row min |pre-activation| over every draw and layer)"""
    n, D = x32.shape
    nl = len(d) // 2
    dims = (D,) + tuple(p.shape[1] for p in d[0:2 * (nl - 1):2])
    sig = (sigmas[0],) + (sigmas[1],) * (nl - 2)
    mir = O.MRGANMirror([], d, quantize=quantize, sigmas=sig)
    x = x32.astype(np.float64)
    b32 = np.zeros(D, np.float32) if baseline is None else np.asarray(baseline, np.float32)
    t = R.input_gradient(d, x, None, objective, quantize=quantize)[2] if targets is None else np.asarray(targets, np.int32)
    W6, b6 = mir.d[-2], mir.d[-1]
    total, margin = np.zeros((n, D)), np.full(n, np.inf)
    for k in range(draws):
        if method == 'noise':
            def nz(site):
                if sig[site] == 0:
                    return np.zeros((n, dims[site]))
                return noise_fn(site, k, dims[site]) if noise_fn else normal(seed, site, NOISE_SEG, k, n, dims[site], row0=0)
            noise = [nz(site) for site in range(nl - 1)]
            xin0 = mir._stage(x, noise[0])
        else:
            noise, xin0 = None, mir.q(path_point(x32, b32, k, draws).astype(np.float64))
        c = mir._disc_fwd(xin0, noise, None)
        for l in range(nl - 1):
            margin = np.minimum(margin, np.abs(c['xin'][l] @ mir.plain.w(l) + mir.d[2 * l + 1]).min(axis=1))
        logits = c['feat_q'] @ W6 + b6
        dp = (R.dlogits(logits, t, objective) @ W6.T) * (c['feat_q'] > 0)
        total += mir.q(mir._disc_bwd(c, dp, None, to_input=True)[2])
    out = total / draws
    if multiply:
        out = out * (x - b32.astype(np.float64))
    return out, t, margin


# ---- the shared problems of the CPU and GPU tests (never modified) ---------------------------------------------------
def problem(K, D, d_hidden=None, n=N):
    return R.problem(K, D, d_hidden, n)


def random_baseline(D):
    return np.random.default_rng(5).standard_normal(D).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(K, D, d_hidden, mode, objective='xent', planted=False, quantize=None, draws=DRAWS):
    """(attribution, targets, decided rows) of one GPU case: targets = the fp64 argmax at x, or (planted) argmax + 1"""
    case, x32 = problem(K, D, d_hidden)
    method, sigmas, baseline, multiply = MODES[mode]
    b = random_baseline(D) if baseline == 'random' else None
    t = R.input_gradient(case.d0, x32.astype(np.float64), None, objective)[2]
    if planted:
        t = ((t + 1) % K).astype(np.int32)
    out, t, margin = attribution(case.d0, x32, t, objective, method, draws, sigmas, b, multiply, quantize)
    if quantize is not None:      # decided by the fp64 forward, whatever the mirror rounds
        margin = attribution(case.d0, x32, t, objective, method, draws, sigmas, b, multiply)[2]
    return out, t, margin >= DECIDED
