"""numpy restatement of the engine's true-Gaussian generator (csrc/common.h: gauss_pairhash / gauss_block, selected by
MRGAN_FLAG_GAUSS_NOISE), and tests.helpers' noise_set / draw_z / Case drawing from it.

The normal at global row R, column C of (seed, site, seg, step):
    key = noise_key(seed, site*256 + seg, step)
    ph  = mix32((key ^ 0x47415553) + (R >> 1) * 0x9E3779B1)          one hash per row pair
    w0  = mix32(ph ^ (2C) * 0x85EBCA77),  w1 = mix32(ph ^ (2C + 1) * 0x85EBCA77)
    u1  = (2 (w0 >> 9) + 1) * 2^-24 in (0, 1),  u2 = (w1 >> 8) * 2^-24 in [0, 1)       (exact in float32)
    n   = sqrt(-2 ln u1) * cos(2 pi u2) if R is even, * sin(2 pi u2) if R is odd
The integer part is exact on both sides; the transcendentals here are float64, on the device precise float32."""
import numpy as np

from oracle.mrgan_oracle import mix32, noise_key
from tests import helpers as H

GAUSS_DOMAIN = 0x47415553
SUPPORT = float(np.sqrt(48.0 * np.log(2.0)))            # u1 >= 2^-24: |n| <= sqrt(-2 ln 2^-24) = 5.768


def gaussian_uniforms(seed, site, seg, step, rows, cols, row0=0):
    """(u1, u2) as float64 arrays [rows, cols]; both are integers * 2^-24, i.e. exact float32 values"""
    key = noise_key(seed, site * 256 + seg, step)
    with np.errstate(over='ignore'):
        R = np.arange(rows, dtype=np.uint32) + np.uint32(row0)
        ph = mix32((key ^ np.uint32(GAUSS_DOMAIN)) + (R >> np.uint32(1)) * np.uint32(0x9E3779B1))          # [rows]
        C = np.arange(cols, dtype=np.uint32)
        w0 = mix32(ph[:, None] ^ ((np.uint32(2) * C) * np.uint32(0x85EBCA77))[None, :])
        w1 = mix32(ph[:, None] ^ ((np.uint32(2) * C + np.uint32(1)) * np.uint32(0x85EBCA77))[None, :])
    u1 = (2.0 * (w0 >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w1 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def gaussian_normal(seed, site, seg, step, rows, cols, row0=0, dtype=np.float64):
    """Standard normals [rows, cols] as a MRGAN_FLAG_GAUSS_NOISE handle draws them.  row0 = global index of the first row."""
    u1, u2 = gaussian_uniforms(seed, site, seg, step, rows, cols, row0)
    r = np.sqrt(-2.0 * np.log(u1))
    odd = ((np.arange(rows) + row0) & 1).astype(bool)[:, None]
    return np.where(odd, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2)).astype(dtype)


def noise_set(*args, **kw):
    return H.noise_set(*args, normal=gaussian_normal, **kw)


def draw_z(*args, **kw):
    return H.draw_z(*args, normal=gaussian_normal, **kw)


class GaussCase(H.Case):
    """tests.helpers.Case with layer noise and device z from the true-Gaussian generator.  The oracle and the mirror take z
    and the layer noise as inputs, so nothing else changes."""

    def __init__(self, *args, **kw):
        H.Case.__init__(self, *args, normal=gaussian_normal, **kw)


def moments(x):
    """(mean, std, excess kurtosis) of all elements"""
    x = np.asarray(x, np.float64).ravel()
    m, s = x.mean(), x.std()
    return float(m), float(s), float(((x - m) ** 4).mean() / s ** 4 - 3.0)


def ks_distance(x):
    """Kolmogorov-Smirnov distance of the sample to N(0, 1)"""
    from scipy.special import ndtr
    x = np.sort(np.asarray(x, np.float64).ravel())
    n = x.size
    cdf = ndtr(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)))


def pair_and_column_corr(x):
    """correlation between the two members of a row pair (rows 2i, 2i+1 of one column) and between adjacent columns"""
    x = np.asarray(x, np.float64)
    pair = np.corrcoef(x[0::2].ravel(), x[1::2].ravel())[0, 1]
    colc = np.corrcoef(x[:, :-1].ravel(), x[:, 1:].ravel())[0, 1]
    return float(pair), float(colc)


def check_distribution(x):
    """the distribution thresholds shared by the CPU test of the restatement and the GPU test of the device draw
    (2048 x 512 values at (1, 1, 3)); returns the figures"""
    m, s, k = moments(x)
    ks = ks_distance(x)
    pc, cc = pair_and_column_corr(x)
    amax = float(np.abs(x).max())
    fig = dict(mean=m, std=s, excess_kurtosis=k, ks=ks, max_abs=amax, pair_corr=pc, col_corr=cc)
    print("\ndistribution:", {a: float("%.3g" % b) for a, b in fig.items()})
    assert abs(m) < 5e-3 and abs(s - 1) < 5e-3, fig
    assert abs(k) < 0.02, fig                   # four standard errors at 10^6 samples; the default generator has -0.0415
    assert ks < 1.95e-3, fig                    # alpha = 1e-3 at n = 2^20
    assert amax <= 5.77 and amax > 4.9, fig     # support sqrt(48 ln 2); a clipped Box-Muller on 16-bit uniforms stops at 4.7
    assert abs(pc) < 5e-3 and abs(cc) < 5e-3, fig
    return fig
