"""Kernel-level parity of every GEMM block tile and epilogue variant (gemm_bf16.hip, gemm_f32.hip, the epilogue of gemm.h),
through mrgan_debug_gemm_launch: one launch per case, caller-owned buffers with leading dimensions wider than the logical
sizes and sentinel-filled outputs, the launched kernel's name asserted.

Reference: operands are drawn once and rounded to bf16, so kernel and reference multiply identical numbers (a bf16 x bf16
product is exact in fp32); the reference is their fp64 product (torch.float64), the noise term is the oracle's exact integer
restatement.

Tolerance, per element and derived ("Kernel-level GEMM tolerance"), with mag = |A||B| + |bias|:
    fp32 accumulation of K exact products in any order   |err| <= 2 K 2^-24 mag      (2 x gamma_K: the MFMA's internal sum)
    bf16 stored outputs add the rounding                  2^-8 |value|
    fp32 outputs (slabs, column sums, fp32 kernels) add nothing.
Relu is 1-Lipschitz and keeps the bound.  An element whose reference pre-activation is within its accumulation bound of zero
is undecided: it is left out of the mask comparison and of the masked-dX comparison (share printed and capped at 0.5 % for
K <= 1024, 2 % above).  Column sums: fp64 sums per 64-row group of the reference values the epilogue keeps (after bias and
activation / derivative, before noise, unrounded); bound = sum of the elements' bounds + 64 * 2^-24 * sum |v|.
Every case prints its largest err / bound ("usage"); fp32 outputs also print the share of the accumulation term alone.
"""
import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests.helpers import DEV, SENT, _assert_close, _assert_sentinel, _embed, _rng, _usage, colsum_groups, colsum_rows, mask_decode, mask_encode

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
FWD, DX, SLAB = 0, 1, 2
LIN, RELU, SOFTPLUS = 0, 1, 2
CS_NONE, CS_SUM, CS_SUM_SQ, CS_SUM_XHAT = 0, 1, 2, 3
VAR_NOISE, VAR_MASK = 4, 8
KS_GROUP_MAX, TUNE_BIT_NO_KS_GROUP = 6, 4
U = 2.0 ** -24                   # fp32 unit roundoff
BF16_RND = 2.0 ** -8             # a float32 matmul of bf16 operands rounded to bf16 uses 98 % of it against fp64; 2^-9 fails
# softplus_fast(x) = max(x, 0) + ln2 * log2(1 + exp2(-log2e |x|)) on the hardware transcendentals.  The ISA manual gives
# v_exp_f32 and v_log_f32 an accuracy of 1 ulp.  exp2: the argument's rounding, 2^-24 |t|, moves e = 2^-t by at most
# ln2 t 2^-t 2^-24 <= 0.37 * 2^-24, 1 ulp of e <= 1 is 2^-23; 1 + e rounds by <= 2^-23; d log2(y) / dy <= 1.45 for y >= 1;
# 1 ulp of a log2 in [0, 1] is <= 2^-23; the product with ln2 and the final sum round by 2^-24 of their values.  Together
# under 7 * 2^-24 absolute + 2^-23 relative; the constants allow twice that.  The fp32 kernels' softplus_f (__expf + log1pf)
# is held to the same.
SOFTPLUS_ABS, SOFTPLUS_REL = 2.0 ** -20, 2.0 ** -22
# one_minus_exp_neg_fast(h) = 1 - exp2(-log2e h), h >= 0: exp2 as above (<= 1.4 * 2^-23) + the subtraction's 2^-24; twice that
SIGMOID_ABS = 2.0 ** -21
MASK_SENT = 0x5A5A
PAD, GAP = 64, 5                 # extra columns of every leading dimension, extra rows between batches
TILE = {0: (64, 128, 2, 2, 3), 1: (128, 128, 2, 2, 2), 3: (256, 256, 2, 4, 2), 5: (64, 128, 2, 2, 2), 7: (128, 128, 2, 4, 2),
        9: (64, 64, 2, 2, 3)}


def kc_name(epi, cfg, n, var):
    """the instantiation the documented shape fallbacks lead to (comment above launch_kc_tile)"""
    h_tile = epi == DX and (var & 3) != RELU
    if cfg in (3, 5, 7) and n % 128:
        cfg = 0
    if cfg == 3 and n % 256:
        cfg = 1
    if h_tile and cfg in (3, 5, 7):
        cfg = 1
    return "gemm_bf16_kc_kernel<%d, %d, %d, %d, %d, %d, %d>" % ((epi,) + TILE[cfg] + (var,))


def f32_name(epi, m, n, nbatch=1, splits=1):
    blocks128 = -(-n // 128) * -(-m // 128) * nbatch * splits
    return "gemm_f32_kernel<%d, %d>" % (epi, 128 if blocks128 >= 128 else 64)


def _draw(rng, shape, scale=1.0):
    """N(0, scale^2) rounded to bf16, as float64 on the device"""
    return torch.from_numpy(rng.standard_normal(shape) * scale).to(torch.bfloat16).to(DEV, torch.float64)


def _launch(E, desc, **kw):
    rc, name = E.debug_gemm_launch(desc, **kw)
    assert rc == 0, (rc, E.load_library().mrgan_last_error())
    return name


def run_kc(dtype, op, m, n, k, cfg=-1, act=LIN, nbatch=1, n_valid=None, noise=None, mask=None, cs_mode=CS_NONE, key=0,
           expect=None):
    """One forward / dX launch checked against fp64: outputs, relu mask, column sums, and every sentinel.
    noise = dict(sigma, site, seg0, seg_step, iter_step, row0, seed, iter); mask: FWD True = write one, DX: bool [nb][m][n]
    reference bits, or (device words, reference bits, decided) from a forward launch.  Returns a dict for round trips."""
    from mr_gan_amd import engine as E
    bf = dtype == BF16
    tdt = torch.bfloat16 if bf else torch.float32
    n_valid = n if n_valid is None else n_valid
    rng = _rng(dtype, op, m, n, k, cfg + 1, act, nbatch, key)
    label = "%s op%d %dx%dx%d nb%d cfg%d act%d" % ("bf16" if bf else "f32", op, m, n, k, nbatch, cfg, act)
    a = _draw(rng, (nbatch, m, k))
    bt = _draw(rng, (n, k), 1.0 / np.sqrt(k))
    bt[n_valid:] = 0                                   # padding columns have zero weights, as in the product
    bias = _draw(rng, (n,))                            # non-zero beyond n_valid too: it must not leak
    lda, ldb, ldo = k + PAD, k + PAD, n + PAD
    abuf = _embed(a, m + GAP, lda, tdt)
    d = dict(dtype=dtype, op=op, m=m, n=n, k=k, nbatch=nbatch, kc_cfg=cfg, act=act, n_valid=n_valid,
             a=abuf, a_bs=(m + GAP) * lda, a_si=lda, a_sk=1, ldo=ldo, out_bs=(m + GAP) * ldo)
    if not bf and op == FWD:                           # the fp32 forward reads the master weight [K][N]
        bbuf = _embed(bt.t()[None], k + GAP, n + PAD, tdt)
        d.update(b=bbuf, b_sk=n + PAD, b_sj=1)
    else:
        bbuf = _embed(bt[None], n + GAP, ldb, tdt)
        d.update(b=bbuf, b_sk=1, b_sj=ldb)
    out = torch.full((nbatch, m + GAP, ldo), SENT, dtype=tdt, device=DEV)
    d["out"] = out
    acc = a @ bt.t()
    mag = a.abs() @ bt.abs().t()
    nblk = (m + 31) // 32
    ldm = n + PAD
    mwords = ref_bits = decided = h = None
    if op == FWD:
        d["bias"] = bias.to(torch.float32)
        bias_v = bias.clone()
        bias_v[n_valid:] = 0
        pre = acc + bias_v
        accb = 2 * k * U * (mag + bias_v.abs())
        if act == RELU:
            v, vb = pre.clamp_min(0), accb
        elif act == SOFTPLUS:
            v = torch.logaddexp(pre, torch.zeros_like(pre))
            v[:, :, n_valid:] = 0
            vb = accb + SOFTPLUS_ABS + SOFTPLUS_REL * v
            vb[:, :, n_valid:] = 0
        else:
            v, vb = pre, accb
        ref, bound = v, vb
        var = act
        if noise:
            nz = torch.stack([torch.from_numpy(O.device_noise_sums(noise["seed"], noise["site"], noise["seg0"] + b * noise["seg_step"],
                                                                   noise["iter"] + b * noise["iter_step"], m, n, noise["row0"]).astype(np.float64))
                              for b in range(nbatch)]).to(DEV) * (noise["sigma"] * O.NOISE_SCALE)
            nz[:, :, n_valid:] = 0
            ref = v + nz
            bound = vb + 4 * U * nz.abs()              # sigma * NOISE_SCALE rounded to fp32, then one fma
            d.update(noise)
            var |= VAR_NOISE
        if mask:
            mwords = torch.full((nbatch, nblk + 1, ldm, 2), MASK_SENT, dtype=torch.int16, device=DEV)
            d.update(mask=mwords, mask_bs=(nblk + 1) * ldm * 2, ldm=ldm)
            var |= VAR_MASK
    else:
        var = act
        accb = 2 * k * U * mag
        v, vb = acc, accb
        if act == RELU:
            if isinstance(mask, tuple):
                mwords, ref_bits, decided = mask
            else:
                # the reference bits where an element lives, random bits everywhere else (rows >= M of the last block, columns >= N)
                ref_bits = mask
                junk = np.stack([mask_encode(rng.random((nblk * 32, n)) < 0.5, ldm) for _ in range(nbatch)])
                junk[:, :, n:, :] = 0xFFFF
                own = mask_encode(np.ones((m, n), bool), ldm)[None]
                w = (junk & ~own) | np.stack([mask_encode(ref_bits[b].cpu().numpy(), ldm) for b in range(nbatch)])
                mwords = torch.from_numpy(w.view(np.int16)).to(DEV)
            d.update(mask=mwords, mask_bs=mwords.shape[1] * ldm * 2, ldm=ldm)
            v = acc * ref_bits
        elif act == SOFTPLUS or cs_mode == CS_SUM_XHAT:
            h = _draw(rng, (nbatch, m, n)).abs() if act == SOFTPLUS else (_draw(rng, (nbatch, m, n)) + 0.5).to(torch.bfloat16).double()
            d.update(h=_embed(h, m + GAP, n + PAD, tdt), h_bs=(m + GAP) * (n + PAD), ldh=n + PAD)
            if act == SOFTPLUS:
                sg = -torch.expm1(-h)
                v, vb = acc * sg, accb * sg + acc.abs() * SIGMOID_ABS + 2 * U * (acc * sg).abs()
        ref, bound = v, vb
    acc_only = None if bf else bound
    if bf:
        bound = bound + BF16_RND * (ref.abs() + bound)
    tiles_m, _ = colsum_rows(m, nbatch)
    ldcs = n + PAD
    if cs_mode != CS_NONE:
        cs1 = torch.full((nbatch * tiles_m + 2, ldcs), SENT, dtype=torch.float32, device=DEV)
        cs2 = torch.full((nbatch * tiles_m + 2, ldcs), SENT, dtype=torch.float32, device=DEV)
        d.update(cs_mode=cs_mode, cs1=cs1, cs2=cs2, ldcs=ldcs)
        if cs_mode == CS_SUM_XHAT:
            mu32, rstd32 = (_draw(rng, (n,), 0.5) + 0.5).float(), (_draw(rng, (n,), 0.2).abs() + 0.8).float()
            mu, rstd = mu32.double(), rstd32.double()
            d.update(bn_mu=mu32, bn_rstd=rstd32)

    name = _launch(E, E.debug_gemm_desc(**d))
    want_name = expect or (kc_name(op, cfg, n, var) if bf else f32_name(op, m, n, nbatch))
    assert name == want_name, (label, name, want_name)

    # ---- outputs and their sentinels -------------------------------------------------------------------------
    got = out.to(torch.float64)
    got_in = got[:, :m, :n]
    assert not bool((out[:, :m, :n] == SENT).any()), label + ": output elements inside [M][N] were not written"
    if decided is not None:                            # masked dX: undecided elements take no part
        got_in = torch.where(decided, got_in, ref)
    use = _assert_close(label + " out [%s]" % name, got_in, ref, bound, acc_only)
    inside = torch.zeros_like(out, dtype=torch.bool)
    inside[:, :m, :n] = True
    _assert_sentinel(label + " out", out.to(torch.float32), inside)
    if n_valid < n:
        assert bool((got[:, :m, n_valid:n] == 0).all()), label + ": columns [n_valid, N) must be exact zeros"
    res = dict(name=name, usage=use)

    # ---- relu mask written by the forward ---------------------------------------------------------------------
    if op == FWD and mask:
        words = mwords.cpu().numpy().view(np.uint16)
        bits = np.stack([mask_decode(words[b], m, n) for b in range(nbatch)])
        want = (pre > 0).cpu().numpy()
        und = (pre.abs() <= accb).cpu().numpy()
        und[:, :, n_valid:] = False                   # padding columns: pre-activation exactly 0, bit exactly 0
        share = und[:, :, :n_valid].mean()
        cap = 0.005 if k <= 1024 else 0.02
        print("%s mask: undecided share %.5f %% (cap %.1f %%)" % (label, 100 * share, 100 * cap))
        assert share <= cap, (label, share)
        wrong = (bits != want) & ~und
        assert not wrong.any(), "%s: %d mask bits differ, first at %s" % (label, wrong.sum(), tuple(np.argwhere(wrong)[0]))
        # words of row blocks >= M and of columns >= N keep their sentinel
        keep = np.ones(words.shape, bool)
        keep[:, :nblk, :n, :] = False
        assert (words[keep] == MASK_SENT).all(), label + ": mask words outside [ceil(M / 32)][N] were written"
        res.update(mask=(mwords, torch.from_numpy(want).to(DEV), torch.from_numpy(~und).to(DEV)), undecided=share)

    # ---- column sums -------------------------------------------------------------------------------------------
    if cs_mode != CS_NONE:
        g = lambda t: torch.from_numpy(colsum_groups(t.cpu().numpy())).to(DEV)
        rows = nbatch * tiles_m
        inside = torch.zeros_like(cs1, dtype=torch.bool)
        inside[:rows, :n] = True
        s1, b1 = g(v), g(vb) + 64 * U * g(v.abs())
        _assert_close(label + " cs1", cs1[:rows, :n].double(), s1, b1, b1)
        _assert_sentinel(label + " cs1", cs1, inside)
        if cs_mode == CS_SUM:
            _assert_sentinel(label + " cs2", cs2, torch.zeros_like(inside))
        else:
            if cs_mode == CS_SUM_SQ:
                s2, b2 = g(v * v), g(2 * v.abs() * vb + vb * vb) + 66 * U * g(v * v)
            else:
                xh = (h - mu) * rstd
                xh[:, :, n_valid:] = 0
                # h - mu, its product with v and the fma round once each; the 64-term sum as above
                s2, b2 = g(v * xh), g(vb * xh.abs()) + 68 * U * g((v * xh).abs())
            _assert_close(label + " cs2", cs2[:rows, :n].double(), s2, b2, b2)
            _assert_sentinel(label + " cs2", cs2, inside)
    return res


# =============================================================================================================
# 1. tiles x products (bf16)
# =============================================================================================================
PRODUCTS = {"fwd-linear": (FWD, LIN), "fwd-relu": (FWD, RELU), "fwd-softplus": (FWD, SOFTPLUS),
            "dx-linear": (DX, LIN), "dx-relumask": (DX, RELU), "dx-softplus": (DX, SOFTPLUS)}
# M not a multiple of 32; N % 128 == 64 and N % 256 == 128; one, two and sixteen k-tiles
RAGGED = [(50, 192, 64), (300, 384, 128), (1000, 320, 1024)]


def _tile_shapes(cfg):
    bm, bn = TILE[cfg][:2]
    return [(2 * bm, 2 * bn, 128)] + RAGGED


def _random_bits(m, n, nbatch, key):
    return torch.from_numpy(_rng(m, n, nbatch, key).random((nbatch, m, n)) < 0.5).to(DEV)


@pytest.mark.parametrize("shape", range(4), ids=["exact", "m50-n192-k64", "m300-n384-k128", "m1000-n320-k1024"])
@pytest.mark.parametrize("product", sorted(PRODUCTS))
@pytest.mark.parametrize("cfg", sorted(TILE))
def test_tile_product(cfg, product, shape):
    op, act = PRODUCTS[product]
    m, n, k = _tile_shapes(cfg)[shape]
    mask = _random_bits(m, n, 1, cfg) if (op, act) == (DX, RELU) else None
    run_kc(BF16, op, m, n, k, cfg=cfg, act=act, mask=mask)


def test_documented_tile_fallbacks_by_name():
    """3 / 5 / 7 need N % 128 == 0 (else 0), 3 needs N % 256 == 0 (else 1), the dX epilogues that stage h exist for 0, 1, 9 only"""
    kc = "gemm_bf16_kc_kernel<%d, %s, %d>"
    t0, t1 = "64, 128, 2, 2, 3", "128, 128, 2, 2, 2"
    for cfg in (3, 5, 7):
        run_kc(BF16, FWD, 100, 192, 64, cfg=cfg, act=RELU, expect=kc % (0, t0, 1))
        run_kc(BF16, DX, 100, 256, 64, cfg=cfg, act=SOFTPLUS, expect=kc % (1, t1, 2))
        run_kc(BF16, DX, 100, 256, 64, cfg=cfg, act=LIN, expect=kc % (1, t1, 0))
    run_kc(BF16, FWD, 100, 384, 64, cfg=3, act=LIN, expect=kc % (0, t1, 0))
    run_kc(BF16, DX, 100, 384, 64, cfg=3, act=RELU, mask=_random_bits(100, 384, 1, 3), expect=kc % (1, t1, 1))


@pytest.mark.parametrize("op,m,n,k,nbatch,cfg", [
    (FWD, 2048, 3072, 128, 1, 7),          # t128 = 384
    (DX, 2048, 3072, 128, 1, 7),
    (FWD, 4096, 4096, 2048, 1, 3),         # K >= 2048 and t256 = 256: the largest case
    (FWD, 4096, 512, 1024, 3, 5),          # t128 = 384, K in [1024, 2048), N <= 512
    (FWD, 2048, 2048, 1024, 1, 7),         # t128 = 256, K in [1024, 2048)
    (DX, 2048, 2048, 1024, 1, 0),          # ... which is a forward rule only
    (FWD, 2048, 2048, 128, 1, 0),          # 512 blocks of 64 x 128
    (FWD, 300, 256, 128, 1, 9),            # <= 256 blocks of 64 x 128
], ids=lambda v: str(v))
def test_measured_table_branches(op, m, n, k, nbatch, cfg):
    """kc_cfg = -1: one shape per branch of the measured table in launch_kc_tile, the chosen tile asserted by name"""
    mask = _random_bits(m, n, nbatch, 11) if op == DX else None
    run_kc(BF16, op, m, n, k, cfg=-1, act=RELU, nbatch=nbatch, mask=mask, expect=kc_name(op, cfg, n, RELU))


# =============================================================================================================
# 2. epilogue features, nbatch = 3 (sentinels, 3., are part of every case)
# =============================================================================================================
FEATURE_TILES = (9, 7, 3, 0, 1)
NOISE = dict(sigma=0.5, site=3, seg0=1, seg_step=1, iter_step=0, row0=0, seed=0x5EED5EED0BADF00D, iter=7)


@pytest.mark.parametrize("m,n,n_valid", [(300, 1024, 1000), (200, 256, 250)])
@pytest.mark.parametrize("act", [LIN, RELU, SOFTPLUS])
@pytest.mark.parametrize("cfg", FEATURE_TILES)
def test_n_valid_columns_stay_zero(cfg, act, m, n, n_valid):
    """columns [n_valid, N): zero weights, a non-zero bias entry and (linear, relu) noise -- none of it may show"""
    noise = None if act == SOFTPLUS else NOISE
    run_kc(BF16, FWD, m, n, 128, cfg=cfg, act=act, nbatch=3, n_valid=n_valid, noise=noise, mask=(act == RELU))


@pytest.mark.parametrize("keying", ["seg_step", "iter_step", "row0"])
@pytest.mark.parametrize("act", [LIN, RELU])
@pytest.mark.parametrize("cfg", FEATURE_TILES)
def test_noise_keys(cfg, act, keying):
    noise = dict(NOISE)
    if keying == "iter_step":
        noise.update(seg_step=0, iter_step=1)
    if keying == "row0":
        noise.update(row0=37, seg_step=2)
    run_kc(BF16, FWD, 300, 256, 128, cfg=cfg, act=act, nbatch=3, noise=noise, mask=(act == RELU))


@pytest.mark.parametrize("noisy", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("m,n,k", [(300, 256, 128), (1000, 512, 1024)])
@pytest.mark.parametrize("cfg", FEATURE_TILES)
def test_mask_round_trip(cfg, m, n, k, noisy):
    """relu (+ noise) + mask in one forward launch; the mask it wrote drives the matching dX launch"""
    fwd = run_kc(BF16, FWD, m, n, k, cfg=cfg, act=RELU, nbatch=3, noise=NOISE if noisy else None, mask=True)
    run_kc(BF16, DX, m, n, 192, cfg=cfg, act=RELU, nbatch=3, mask=fwd["mask"], key=1)


# N = 512: every tile is itself; N = 320: the 128-wide tiles straddle N (3 / 7 fall back to 0).  M = 300: 64-row groups past M
@pytest.mark.parametrize("n,n_valid", [(512, 506), (320, 314)])
@pytest.mark.parametrize("cs_mode", [CS_SUM, CS_SUM_SQ])
@pytest.mark.parametrize("act", [LIN, RELU, SOFTPLUS])
@pytest.mark.parametrize("cfg", FEATURE_TILES)
def test_forward_column_sums(cfg, act, cs_mode, n, n_valid):
    run_kc(BF16, FWD, 300, n, 128, cfg=cfg, act=act, nbatch=3, n_valid=n_valid, cs_mode=cs_mode, noise=NOISE if act == LIN else None)


@pytest.mark.parametrize("n,n_valid", [(512, 506), (320, 314)])
@pytest.mark.parametrize("cs_mode,act", [(CS_SUM, LIN), (CS_SUM, RELU), (CS_SUM, SOFTPLUS), (CS_SUM_XHAT, LIN)])
@pytest.mark.parametrize("cfg", FEATURE_TILES)
def test_dx_column_sums(cfg, cs_mode, act, n, n_valid):
    """bias-gradient sums and the BatchNorm-backward pair (sum dy, sum dy * xhat); h through the LDS tile (0, 1, 9) and,
    for 3 / 7, through the fallback to tile 1"""
    mask = _random_bits(300, n, 3, cfg) if act == RELU else None
    run_kc(BF16, DX, 300, n, 192, cfg=cfg, act=act, nbatch=3, n_valid=n_valid, cs_mode=cs_mode, mask=mask)


# =============================================================================================================
# 4. weight gradients
# =============================================================================================================
def slab_problem(dtype, m, n, k, splits, kchunk=None, seg=None, key=0):
    """operands X [k][m + PAD], dY [k][n + PAD] (pads and hole rows NaN), sentinel slabs, per-split fp64 reference"""
    bf = dtype == BF16
    tdt = torch.bfloat16 if bf else torch.float32
    rng = _rng(dtype, m, n, k, splits, key)
    x, dy = _draw(rng, (k, m)), _draw(rng, (k, n))
    seg_stride, seg_rows = seg or (0, 0)
    rows = np.arange(k)
    valid = torch.from_numpy((rows % seg_stride) < seg_rows if seg_stride else rows < k).to(DEV)
    xb, dyb = _embed(x[None], k + GAP, m + PAD, tdt)[0], _embed(dy[None], k + GAP, n + PAD, tdt)[0]
    xb[:k][~valid] = float("nan")
    dyb[:k][~valid] = float("nan")
    bk = 64 if bf else 16
    if kchunk is None:
        per_split = -(-k // splits)
        kchunk = -(-per_split // bk) * bk
    ldo = n + PAD
    slab = torch.full((splits, m + GAP, ldo), SENT, dtype=torch.float32, device=DEV)
    d = dict(dtype=dtype, op=SLAB, m=m, n=n, k=k, splits=splits, kchunk=kchunk, seg_stride=seg_stride, seg_rows=seg_rows,
             a=xb, a_si=1, a_sk=m + PAD, b=dyb, b_sk=n + PAD, b_sj=1, slab=slab, slab_stride=(m + GAP) * ldo, ldo=ldo)
    refs, bounds = [], []
    for s in range(splits):
        sel = valid.clone()
        sel[:min(k, s * kchunk)] = False
        sel[min(k, (s + 1) * kchunk):] = False
        xs, ds = x[sel], dy[sel]
        refs.append(xs.t() @ ds)
        bounds.append(2 * max(1, int(sel.sum())) * U * (xs.abs().t() @ ds.abs()))
    return d, slab, torch.stack(refs), torch.stack(bounds)


def check_slabs(label, slab, ref, bound, m, n):
    got = slab[:, :m, :n].double()
    assert bool(torch.isfinite(got).all()), label + ": non-finite slab (a hole row or a pad column was read)"
    for s in range(ref.shape[0]):
        _assert_close("%s slab %d" % (label, s), got[s], ref[s], bound[s], bound[s])
    _assert_close(label + " sum", got.sum(0), ref.sum(0), bound.sum(0))
    inside = torch.zeros_like(slab, dtype=torch.bool)
    inside[:, :m, :n] = True
    _assert_sentinel(label, slab, inside)


KS_FAST, KS_KERNEL, KS_GROUP = "gemm_bf16_ks_fast_kernel<3, 2, 4>", "gemm_bf16_ks_kernel", "gemm_bf16_ks_group_kernel<2, 2, 4>"


@pytest.mark.parametrize("m,n,k,splits,kchunk,want", [
    (256, 384, 1024, 1, None, KS_FAST), (200, 192, 1024, 3, None, KS_FAST), (256, 128, 1024, 8, None, KS_FAST),
    (192, 320, 640, 3, 256, KS_FAST),      # last split short: 128 of 256
    (192, 320, 512, 3, 256, KS_FAST),      # last split empty
    (256, 384, 1000, 1, None, KS_KERNEL), (200, 192, 1000, 3, None, KS_KERNEL), (256, 128, 1000, 8, None, KS_KERNEL),
    (192, 320, 600, 3, 256, KS_KERNEL),    # last split short
    (192, 320, 500, 3, 256, KS_KERNEL),    # last split empty
], ids=lambda v: str(v))
def test_weight_gradient_splits(m, n, k, splits, kchunk, want):
    """the LDS-DMA kernel (reduction length a multiple of 64) and the register-staged one (any length)"""
    from mr_gan_amd import engine as E
    d, slab, ref, bound = slab_problem(BF16, m, n, k, splits, kchunk)
    name = _launch(E, E.debug_gemm_desc(**d))
    assert name == want
    check_slabs("dW %dx%dx%d/%d %s" % (m, n, k, splits, name), slab, ref, bound, m, n)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("seg_rows,seg_stride", [(50, 64), (200, 256)])
def test_weight_gradient_over_segments_with_holes(seg_rows, seg_stride, splits):
    """three segments of seg_rows valid rows at a stride of seg_stride: the hole rows of both operands hold NaN and must be
    zero-filled by predicate (gemm_bf16_ks_kernel), in the ragged (last segment cut) and the padded reduction range"""
    from mr_gan_amd import engine as E
    for k in (2 * seg_stride + seg_rows, 3 * seg_stride):
        d, slab, ref, bound = slab_problem(BF16, 256, 192, k, splits, seg=(seg_stride, seg_rows))
        name = _launch(E, E.debug_gemm_desc(**d))
        assert name == KS_KERNEL
        check_slabs("dW holes %d/%d k%d splits%d" % (seg_rows, seg_stride, k, splits), slab, ref, bound, 256, 192)


GROUP_PROBLEMS = [(256, 384, 1024, 2), (64, 128, 512, 1), (200, 192, 1024, 3), (128, 64, 256, 4), (384, 256, 512, 1), (64, 64, 64, 1)]


@pytest.mark.parametrize("with_fold", [False, True], ids=["nofold", "fold"])
@pytest.mark.parametrize("count", [1, 3, 6])
def test_grouped_weight_gradients(count, with_fold):
    """problems of unequal size in one grouped launch, with and without the fold blocks behind them"""
    from mr_gan_amd import engine as E
    probs = [slab_problem(BF16, m, n, k, s, key=i) for i, (m, n, k, s) in enumerate(GROUP_PROBLEMS[:count])]
    fold = None
    if with_fold:
        nsrc, ngroups, fn, stride = 29, 3, 700, 704        # nsrc not a multiple of ngroups; both loops of the fold run
        src = torch.from_numpy(_rng(count, 5).standard_normal((nsrc, stride)).astype(np.float32)).to(DEV)
        dst = torch.full((ngroups + 1, stride), SENT, dtype=torch.float32, device=DEV)
        fold = (src, dst, stride, nsrc, fn, ngroups)
    rc, name = E.debug_gemm_launch([E.debug_gemm_desc(**p[0]) for p in probs], grouped=True, fold=fold)
    assert (rc, name) == (0, KS_GROUP), (rc, name)
    for i, (d, slab, ref, bound) in enumerate(probs):
        check_slabs("group %d/%d" % (i, count), slab, ref, bound, d["m"], d["n"])
    if with_fold:
        s64 = src.double()
        want = torch.stack([s64[g::ngroups].sum(0) for g in range(ngroups)])
        fb = torch.stack([s64[g::ngroups].abs().sum(0) for g in range(ngroups)]) * (-(-nsrc // ngroups)) * U
        _assert_close("fold", dst[:ngroups, :fn].double(), want[:, :fn], fb[:, :fn], fb[:, :fn])
        inside = torch.zeros_like(dst, dtype=torch.bool)
        inside[:ngroups, :fn] = True
        _assert_sentinel("fold", dst, inside)


def test_grouped_launch_refusals():
    """1 = not applicable, nothing launched: a strided problem, more than KS_GROUP_MAX problems, TUNE_BIT_NO_KS_GROUP"""
    from mr_gan_amd import engine as E
    ok = slab_problem(BF16, 128, 128, 256, 1)
    holes = slab_problem(BF16, 128, 128, 178, 1, seg=(64, 50), key=1)
    ragged = slab_problem(BF16, 128, 128, 200, 1, key=2)
    off = slab_problem(BF16, 128, 128, 256, 1, key=3)
    off[0]["tune_bits"] = TUNE_BIT_NO_KS_GROUP
    for descs in ([ok[0], holes[0]], [ok[0], ragged[0]], [ok[0]] * (KS_GROUP_MAX + 1), [off[0]]):
        rc, name = E.debug_gemm_launch([E.debug_gemm_desc(**d) for d in descs], grouped=True)
        assert (rc, name) == (1, "")
    for p in (ok, holes, ragged, off):
        _assert_sentinel("refused group", p[1], torch.zeros_like(p[1], dtype=torch.bool))


# =============================================================================================================
# 5. fp32 kernels
# =============================================================================================================
@pytest.mark.parametrize("m,n,k,ts", [(1024, 2048, 128, 128), (1000, 1024, 128, 64), (50, 192, 64, 64)])
@pytest.mark.parametrize("product", sorted(PRODUCTS))
def test_f32_products(product, m, n, k, ts):
    op, act = PRODUCTS[product]
    mask = _random_bits(m, n, 1, 5) if (op, act) == (DX, RELU) else None
    cs = CS_SUM_SQ if op == FWD else (CS_SUM_XHAT if act == LIN else CS_SUM)
    run_kc(F32, op, m, n, k, act=act, mask=mask, cs_mode=cs, n_valid=n - 6, expect="gemm_f32_kernel<%d, %d>" % (op, ts))


@pytest.mark.parametrize("m,n,k,splits,ts", [(512, 512, 1024, 8, 128), (512, 512, 1000, 3, 64), (200, 192, 178, 1, 64)])
def test_f32_weight_gradient(m, n, k, splits, ts):
    from mr_gan_amd import engine as E
    seg = (64, 50) if k == 178 else None
    d, slab, ref, bound = slab_problem(F32, m, n, k, splits, seg=seg)
    name = _launch(E, E.debug_gemm_desc(**d))
    assert name == "gemm_f32_kernel<2, %d>" % ts
    check_slabs("f32 dW %dx%dx%d/%d" % (m, n, k, splits), slab, ref, bound, m, n)


@pytest.mark.parametrize("op", [FWD, DX, SLAB])
def test_f32_tiles_are_bit_identical(op):
    """launch_gemm_f32 promises that the 64 x 64 and the 128 x 128 kernel give the same bits: every output element is the same
    k-ordered chain.  The same problem once as one launch (128 blocks of 128 x 128) and once as two launches over halves of
    its columns (64 blocks each: the 64 x 64 kernel)."""
    from mr_gan_amd import engine as E
    m, n, k = (1024, 2048, 256) if op != SLAB else (1024, 2048, 320)
    rng = _rng(op, 99)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    if op == SLAB:
        a, b = f(k, m), f(k, n)
        base = dict(dtype=F32, op=SLAB, m=m, k=k, a=a, a_si=1, a_sk=m, b_sk=n, b_sj=1, ldo=n, slab_stride=m * n)
    else:
        a = f(m, k)
        b = f(k, n) if op == FWD else f(n, k)
        base = dict(dtype=F32, op=op, m=m, k=k, a=a, a_si=k, a_sk=1, ldo=n, act=SOFTPLUS if op == FWD else LIN)
        base.update(dict(b_sk=n, b_sj=1) if op == FWD else dict(b_sk=1, b_sj=k))
    bias = f(n)
    outs = []
    for parts in (1, 2):
        out = torch.full((m, n), SENT, dtype=torch.float32, device=DEV)
        w = n // parts
        for p in range(parts):
            d = dict(base, n=w, n_valid=w)
            d["b"] = b[p * w:] if op == DX else b[:, p * w:]
            d["slab" if op == SLAB else "out"] = out[:, p * w:]
            if op == FWD:
                d["bias"] = bias[p * w:]
            name = _launch(E, E.debug_gemm_desc(**d))
            assert name == "gemm_f32_kernel<%d, %d>" % (op, 128 if parts == 1 else 64)
        outs.append(out)
    assert bool((outs[0] != SENT).all())
    assert torch.equal(outs[0], outs[1]), "%d elements differ between the 64 x 64 and the 128 x 128 kernel" % int((outs[0] != outs[1]).sum())


# =============================================================================================================
# 6. refusals
# =============================================================================================================
def test_launcher_refusals():
    """launch_gemm_bf16 returns -3, and launches nothing, for K % 64 != 0, splits != 1 on a forward / dX product, a reduction
    index that is not innermost, and operands of 2 GiB or more (the 32-bit range of a buffer descriptor; checked on the
    strides alone, the buffers stay small); the entry refuses kc_cfg values that are not block tiles"""
    from mr_gan_amd import engine as E
    a = torch.zeros((64, 256), dtype=torch.bfloat16, device=DEV)
    b = torch.zeros((64, 256), dtype=torch.bfloat16, device=DEV)
    out = torch.full((64, 64), SENT, dtype=torch.bfloat16, device=DEV)
    base = dict(dtype=BF16, op=FWD, m=64, n=64, k=128, a=a, a_si=256, a_sk=1, b=b, b_sk=1, b_sj=256, out=out, ldo=64, n_valid=64)
    big = 1 << 24                                    # 64 rows * 2^24 elements * 2 bytes = 2^31
    assert 64 * big * 2 >= 1 << 31 and 64 * (big - 8) * 2 < 1 << 31
    cases = [dict(k=96), dict(splits=2), dict(a_si=big), dict(b_sj=big), dict(op=DX, k=96), dict(op=DX, splits=3),
             dict(a_sk=2), dict(b_sk=2)]
    for c in cases:
        assert E.debug_gemm_launch(E.debug_gemm_desc(**dict(base, **c)))[0] == -3, c
    for cfg in (2, 4, 6, 8, 10, -2):
        assert E.debug_gemm_launch(E.debug_gemm_desc(**dict(base, kc_cfg=cfg)))[0] == -1, cfg
    slab = torch.full((64, 64), SENT, dtype=torch.float32, device=DEV)
    d = dict(dtype=BF16, op=SLAB, m=64, n=64, k=64, a=a, a_si=2, a_sk=256, b=b, b_sk=256, b_sj=1, slab=slab, slab_stride=4096, ldo=64)
    assert E.debug_gemm_launch(E.debug_gemm_desc(**d))[0] == -3
    assert bool((out == SENT).all()) and bool((slab == SENT).all())
    assert E.debug_gemm_launch(E.debug_gemm_desc(**base))[0] == 0          # and the unmodified problem runs
    assert bool((out == 0).all())
