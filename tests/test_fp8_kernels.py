"""Kernel-level parity of the fp8 GEMM family (gemm_fp8.hip: the three products, both block tiles, every epilogue
instantiation of launch_gemm_fp8, the fp8-output epilogue of gemm.h with copy_tile), of quant8_kernel and of
fp8_update_scales_kernel, through mrgan_debug_gemm_launch / mrgan_debug_quant8 / mrgan_debug_fp8_update_scales: one launch per
case on caller-owned buffers, the launched kernel's name asserted.

Reference: the operands are drawn once, cast to the product's fp8 formats, and handed to the kernel as BYTES; their fp64
dequantised values are the reference operands, so kernel and reference multiply identical numbers (an fp8 x fp8 product has at
most 8 significand bits: exact in fp32).  Operand padding -- columns >= K, rows >= M, the rows between batches -- holds 0x7F, NaN
in e4m3 and in e5m2: a read outside the descriptor poisons the result.

Tolerance, per element ("Kernel-level GEMM tolerance"), with mag = |A||B| + |bias| on de-scaled values:
    fp32 accumulation of K exact products                 2 K 2^-24 mag
        (its second factor also carries the fp32 roundings of the epilogue's own adds: bias, and the noise fma's 2^-24 |value|)
    v_mfma_scale_f32_32x32x64_f8f6f4 adds                 7 2^-13 (A^ B^)       accb = the sum of the two
        The instruction does not add the 64 products in fp32.  Measured on an MI355X, one wave and one MFMA per experiment
        against fp64 (DESIGN.md has the experiments): within each group of 8 consecutive reduction indices every product is cut
        (towards zero) to a multiple of 2^(E - 13), E = the largest ea + eb of the group (the operands' exponents, subnormals
        counting with the smallest normal exponent); the eight group sums and C are then added to within a few fp32 ulp.  So a
        group loses less than 7 quanta, 7 2^-13 2^E, and with x^ = 2^(exponent of x) (0 for 0), 2^E <= the group's share of
        A^ B^.  The plain fp32 rule alone is exceeded (largest use seen 1.20, weight gradient at 128 reduction rows per slab).
    bf16 stored outputs add                               2^-8 |value|
    a noise term adds                                     4 2^-24 |noise|
    fp32 outputs (slabs, column sums) add nothing (column sums: + 64 2^-24 sum |v| for the 64-term sum).
fp8 outputs take NO rounding tolerance.  Q(x) = saturating round-to-nearest-even of x * (output slot's scale) onto the format's
grid is monotone, so a kernel value within b of the reference r must come out as a code g with Q(r - b) <= g <= Q(r + b)
(through relu: relu(pre -+ accb), then the noise).  0x00 and 0x80 are the same value.  No element is left out; the share of
elements whose two ends differ is printed.  fp8 output buffers are filled with 0x7F, which the saturating packer cannot emit.
Relu masks: an element with |pre| <= accb is undecided (share capped at 0.5 %, K <= 1024 throughout).
"""
import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests import gaussian_noise as G
from tests.helpers import DEV, SENT, _assert_close, _assert_sentinel, _embed, _rng, _usage, colsum_groups, colsum_rows, mask_decode, mask_encode

pytestmark = pytest.mark.gpu

FP8 = 2
FWD, DX, SLAB = 0, 1, 2
LIN, RELU, SOFTPLUS = 0, 1, 2
CS_NONE, CS_SUM, CS_SUM_SQ, CS_SUM_XHAT = 0, 1, 2, 3
E4M3, E5M2 = 0, 1
TDT = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
GRID = {E4M3: O.FP8_FORMATS['e4m3'], E5M2: O.FP8_FORMATS['e5m2']}       # mantissa bits, smallest normal exponent, largest finite
TARGET = {E4M3: O.FP8_TARGETS['e4m3'], E5M2: O.FP8_TARGETS['e5m2']}
FMT_A = {FWD: E4M3, DX: E5M2, SLAB: E4M3}
FMT_B = {FWD: E4M3, DX: E4M3, SLAB: E5M2}
FMT_OUT = {FWD: E4M3, DX: E5M2}
U = 2.0 ** -24
BF16_RND = 2.0 ** -8
# softplus_fast on the hardware transcendentals: the derivation stands in test_gemm_kernels.py
SOFTPLUS_ABS, SOFTPLUS_REL = 2.0 ** -20, 2.0 ** -22
POISON = 0x7F                    # NaN in both formats: operand padding and the sentinel of fp8 outputs
MASK_SENT = 0x5A5A
PAD, GAP = 64, 5                 # spare columns of every leading dimension, spare rows between batches
TGAP = 16                        # spare bytes between the batches of a transposed image (its batch pitch is a multiple of 16)
NOISE = dict(sigma=0.5, site=3, seg0=1, seg_step=1, iter_step=0, row0=0, seed=0x5EED5EED0BADF00D, iter=7)
# device Box-Muller against the fp64 restatement: |dev - ref| <= A + B |ref| (tests/test_gaussian_noise_gpu.py, measured there)
GAUSS_ABS, GAUSS_REL = 4 * 1.79e-7, 4 * 2.26e-7
# largest use of the accumulation bound and of the plain fp32 rule alone (fp32 outputs), largest "two admissible codes" share
WORST = dict(acc=0.0, plain=0.0, two=0.0)


def _name(op, tile):
    return "gemm_fp8_kc_kernel<%d, %d, %d>" % (op, tile, tile)


def _q8(x, fmt):
    """oracle.fp8_round on a float64 device tensor: saturating round-to-nearest-even onto the grid of `fmt`"""
    mant, emin, lim = GRID[fmt]
    x = x.clamp(-lim, lim)
    _, e = torch.frexp(x.abs())
    quantum = torch.exp2((e - 1).clamp_min(emin).to(torch.float64) - mant)
    return torch.round(x / quantum) * quantum


def _encode(v32, fmt):
    """float32 (CPU tensor) -> fp8 bytes: clamp as the packer does, then torch's cast (pinned to the mirror's grid by
    tests/test_host.py::test_fp8_round_equals_torch_casts_on_every_bf16_value)"""
    lim = GRID[fmt][2]
    return v32.clamp(-lim, lim).to(TDT[fmt]).view(torch.uint8)


def _decode(b, fmt):
    """fp8 bytes -> float64, through a table built on the CPU"""
    table = torch.arange(256, dtype=torch.uint8).view(TDT[fmt]).to(torch.float64).to(b.device)
    return table[b.long()]


def _draw8(rng, shape, std, scale, fmt):
    """N(0, std^2) * scale cast to `fmt` -> (bytes on the device, the de-scaled fp64 values v they stand for, and v^ = 2^(the
    operand's exponent, the smallest normal one for subnormals) / scale, 0 where v is 0)"""
    b = _encode(torch.from_numpy((rng.standard_normal(shape) * (std * scale)).astype(np.float32)), fmt).to(DEV)
    v = _decode(b, fmt)
    _, e = torch.frexp(v.abs())
    hat = torch.where(v != 0, torch.exp2((e - 1).clamp_min(GRID[fmt][1]).to(torch.float64)), torch.zeros_like(v))
    return b, v / scale, hat / scale


MFMA_CUT = 7 * 2.0 ** -13        # per group of 8 products: 7 of them cut to multiples of 2^-13 of the group's largest 2^(ea + eb)


def _acc_bound(k, mag, hat):
    """fp32 accumulation of k products (mag = |A||B| (+ |bias|)) + the MFMA's alignment cuts (hat = A^ B^) -> (bound, plain rule)"""
    plain = 2 * k * U * mag
    return plain + MFMA_CUT * hat, plain


def _embed8(b, rows, ld):
    return _embed(b, rows, ld, torch.uint8, fill=POISON)


def _slots(*rows):
    from mr_gan_amd import engine as E
    return E.fp8_slots([(0.0, s, 1.0 / s, t) for s, t in rows], DEV)


def _launch(E, desc):
    rc, name = E.debug_gemm_launch(desc)
    assert rc == 0, (rc, E.load_library().mrgan_last_error())
    return name


def _interval_check(label, got_bytes, lo, hi, so, fmt):
    """every decoded code lies in [Q(lo), Q(hi)]; NaN codes (the sentinel, a poisoned sum) fail"""
    g = _decode(got_bytes, fmt)
    qlo, qhi = _q8(lo * so, fmt), _q8(hi * so, fmt)
    bad = ~((g >= qlo) & (g <= qhi))
    two = float((qlo != qhi).double().mean())
    WORST["two"] = max(WORST["two"], two)
    print("%s fp8 codes: %d elements, two admissible codes on %.3f %%, exactly the reference's code on %.3f %%"
          % (label, g.numel(), 100 * two, 100 * float((g == _q8((lo + hi) * 0.5 * so, fmt)).double().mean())))
    if bool(bad.any()):
        at = tuple(int(v[0]) for v in torch.nonzero(bad, as_tuple=True))
        raise AssertionError("%s: %d codes outside [Q(r - b), Q(r + b)], first at %s: byte 0x%02x = %r, interval [%r, %r] (scaled)"
                             % (label, int(bad.sum()), at, int(got_bytes[at]), float(g[at]), float(qlo[at]), float(qhi[at])))


def _check_images(label, q8, q8t, m, n, nbatch, q8t_bs):
    """sentinels and explicit zeros of the two images, and their agreement byte for byte"""
    mp = -(-m // 16) * 16
    if q8 is not None:
        inside = torch.zeros_like(q8, dtype=torch.bool)
        inside[:, :m, :n] = True
        _assert_sentinel(label + " q8", q8, inside, value=POISON)
        assert not bool((q8[:, :m, :n] == POISON).any()), label + ": row-major bytes inside [M][N] were not written"
    if q8t is not None:
        inside = torch.zeros_like(q8t, dtype=torch.bool)
        for b in range(nbatch):
            inside[:n, b * q8t_bs:b * q8t_bs + mp] = True
            tail = q8t[:n, b * q8t_bs + m:b * q8t_bs + mp]
            assert bool((tail == 0).all()), "%s: transposed bytes [M, round_up(M, 16)) of batch %d must be exact zeros" % (label, b)
            assert not bool((q8t[:n, b * q8t_bs:b * q8t_bs + m] == POISON).any()), label + ": transposed bytes were not written"
        _assert_sentinel(label + " q8t", q8t, inside, value=POISON)
    if q8 is not None and q8t is not None:
        tr = torch.stack([q8t[:n, b * q8t_bs:b * q8t_bs + m].t() for b in range(nbatch)])
        diff = tr != q8[:, :m, :n]
        assert not bool(diff.any()), "%s: the two images differ in %d bytes, first at %s" % (
            label, int(diff.sum()), tuple(int(v[0]) for v in torch.nonzero(diff, as_tuple=True)))


def run8(op, m, n, k, tile, cfg, act=LIN, nbatch=1, n_valid=None, out="bf16", noise=None, gauss=False, mask=None,
         cs_mode=CS_NONE, scales=(1.0, 1.0, 1.0), null_slots=False, key=0):
    """One forward / dX launch checked against fp64.  out: "bf16", or the fp8 images "both" / "q8" / "q8t".  scales = (operand A,
    operand B, output) slot scales; null_slots: no operand slots (unit scales through acc_scale).  mask: FWD True = write one;
    DX: bool [nb][m][n] reference bits.  Returns the figures of the case."""
    from mr_gan_amd import engine as E
    n_valid = n if n_valid is None else n_valid
    sa, sb, so = (1.0, 1.0, scales[2]) if null_slots else scales
    out8 = out != "bf16"
    rng = _rng(8, op, m, n, k, cfg + 1, act, nbatch, key)
    label = "fp8 op%d %dx%dx%d nb%d cfg%d act%d %s" % (op, m, n, k, nbatch, cfg, act, out)
    ab, a, ah = _draw8(rng, (nbatch, m, k), 1.0 if op == FWD else 2.0 ** -6, sa, FMT_A[op])
    bb, bt, bh = _draw8(rng, (n, k), 1.0 / np.sqrt(k), sb, FMT_B[op])
    bb[n_valid:] = 0                                    # padding columns have zero weights, as in the product
    bt[n_valid:] = 0
    bh[n_valid:] = 0
    lda, ldb, ldo = k + PAD, k + PAD, n + PAD
    abuf, bbuf = _embed8(ab, m + GAP, lda), _embed8(bb[None], n + GAP, ldb)
    slots = _slots((sa, TARGET[FMT_A[op]]), (sb, TARGET[FMT_B[op]]), (so, TARGET[FMT_OUT[op]]))
    slots0 = slots.clone()
    d = dict(dtype=FP8, op=op, m=m, n=n, k=k, nbatch=nbatch, kc_cfg=cfg, act=act, n_valid=n_valid,
             a=abuf, a_bs=(m + GAP) * lda, a_si=lda, a_sk=1, b=bbuf, b_sk=1, b_sj=ldb)
    if not null_slots:
        d.update(slot_a=slots[0], slot_b=slots[1])
    obuf = q8 = q8t = None
    mp = -(-m // 16) * 16
    q8t_bs = mp + TGAP
    if out8:
        d["slot_o"] = slots[2]
        if out in ("both", "q8"):
            q8 = torch.full((nbatch, m + GAP, ldo), POISON, dtype=torch.uint8, device=DEV)
            d.update(q8=q8, q8_bs=(m + GAP) * ldo, ldq8=ldo)
        if out in ("both", "q8t"):
            q8t = torch.full((n + GAP, nbatch * q8t_bs + PAD), POISON, dtype=torch.uint8, device=DEV)
            d.update(q8t=q8t, q8t_bs=q8t_bs, ldq8t=nbatch * q8t_bs + PAD)
    else:
        obuf = torch.full((nbatch, m + GAP, ldo), SENT, dtype=torch.bfloat16, device=DEV)
        d.update(out=obuf, out_bs=(m + GAP) * ldo, ldo=ldo)
    acc = a @ bt.t()
    mag = a.abs() @ bt.abs().t()
    hat = ah @ bh.t()
    nblk = (m + 31) // 32
    ldm = n + PAD
    mwords = pre = h = None
    if op == FWD:
        bias = torch.from_numpy(rng.standard_normal(n)).to(torch.bfloat16).to(DEV, torch.float64)     # non-zero beyond n_valid too
        d["bias"] = bias.to(torch.float32)
        bias_v = bias.clone()
        bias_v[n_valid:] = 0
        pre = acc + bias_v
        accb, _ = _acc_bound(k, mag + bias_v.abs(), hat)
        if act == RELU:
            v, lo, hi = pre.clamp_min(0), (pre - accb).clamp_min(0), (pre + accb).clamp_min(0)
        elif act == SOFTPLUS:
            v = torch.logaddexp(pre, torch.zeros_like(pre))
            v[:, :, n_valid:] = 0
            vb = accb + SOFTPLUS_ABS + SOFTPLUS_REL * v
            vb[:, :, n_valid:] = 0
            lo, hi = v - vb, v + vb
        else:
            v, lo, hi = pre, pre - accb, pre + accb
        vb = torch.maximum(v - lo, hi - v)
        ref = v
        if noise:
            if gauss:
                nz = torch.stack([torch.from_numpy(G.gaussian_normal(noise["seed"], noise["site"], noise["seg0"] + b * noise["seg_step"],
                                                                     noise["iter"] + b * noise["iter_step"], m, n, row0=noise["row0"]))
                                  for b in range(nbatch)]).to(DEV) * noise["sigma"]
                nzb = noise["sigma"] * (GAUSS_ABS + GAUSS_REL * nz.abs() / noise["sigma"]) + 4 * U * nz.abs()
            else:
                nz = torch.stack([torch.from_numpy(O.device_noise_sums(noise["seed"], noise["site"], noise["seg0"] + b * noise["seg_step"],
                                                                       noise["iter"] + b * noise["iter_step"], m, n, noise["row0"]).astype(np.float64))
                                  for b in range(nbatch)]).to(DEV) * (noise["sigma"] * O.NOISE_SCALE)
                nzb = 4 * U * nz.abs()                 # sigma * NOISE_SCALE rounded to fp32, then one fma
            nz[:, :, n_valid:] = 0
            nzb[:, :, n_valid:] = 0
            ref, lo, hi = v + nz, lo + nz - nzb, hi + nz + nzb
            d.update(noise, gauss=1 if gauss else 0)
        if mask:
            mwords = torch.full((nbatch, nblk + 1, ldm, 2), MASK_SENT, dtype=torch.int16, device=DEV)
            d.update(mask=mwords, mask_bs=(nblk + 1) * ldm * 2, ldm=ldm)
    else:
        accb, _ = _acc_bound(k, mag, hat)
        v, vb = acc, accb
        if act == RELU:
            # the reference bits where an element lives, random bits everywhere else (rows >= M of the last block, columns >= N)
            junk = np.stack([mask_encode(rng.random((nblk * 32, n)) < 0.5, ldm) for _ in range(nbatch)])
            junk[:, :, n:, :] = 0xFFFF
            own = mask_encode(np.ones((m, n), bool), ldm)[None]
            w = (junk & ~own) | np.stack([mask_encode(mask[b].cpu().numpy(), ldm) for b in range(nbatch)])
            mwords = torch.from_numpy(w.view(np.int16)).to(DEV)
            d.update(mask=mwords, mask_bs=mwords.shape[1] * ldm * 2, ldm=ldm)
            v, vb = acc * mask, accb * mask
        elif cs_mode == CS_SUM_XHAT:
            h = (torch.from_numpy(rng.standard_normal((nbatch, m, n))).to(torch.bfloat16).to(DEV, torch.float64) + 0.5).to(torch.bfloat16).double()
            d.update(h=_embed(h, m + GAP, n + PAD, torch.bfloat16), h_bs=(m + GAP) * (n + PAD), ldh=n + PAD)
        ref, lo, hi = v, v - vb, v + vb
    tiles_m, _ = colsum_rows(m, nbatch)
    ldcs = n + PAD
    if cs_mode != CS_NONE:
        cs1 = torch.full((nbatch * tiles_m + 2, ldcs), SENT, dtype=torch.float32, device=DEV)
        cs2 = torch.full((nbatch * tiles_m + 2, ldcs), SENT, dtype=torch.float32, device=DEV)
        d.update(cs_mode=cs_mode, cs1=cs1, cs2=cs2, ldcs=ldcs)
        if cs_mode == CS_SUM_XHAT:
            f = lambda s: torch.from_numpy(rng.standard_normal(n) * s).to(torch.bfloat16).to(DEV, torch.float64)
            mu32, rstd32 = (f(0.5) + 0.5).float(), (f(0.2).abs() + 0.8).float()
            mu, rstd = mu32.double(), rstd32.double()
            d.update(bn_mu=mu32, bn_rstd=rstd32)

    name = _launch(E, E.debug_gemm_desc(**d))
    assert name == _name(op, tile), (label, name)
    res = dict(name=name)

    # ---- outputs and their sentinels -------------------------------------------------------------------------
    if out8:
        fmt = FMT_OUT[op]
        want_img = q8[:, :m, :n] if q8 is not None else torch.stack([q8t[:n, b * q8t_bs:b * q8t_bs + m].t() for b in range(nbatch)])
        _interval_check(label + " [%s]" % name, want_img, lo, hi, so, fmt)
        _check_images(label, q8, q8t, m, n, nbatch, q8t_bs)
        if n_valid < n:
            assert bool(((want_img[:, :, n_valid:] & 0x7F) == 0).all()), label + ": columns [n_valid, N) must be zero bytes"
        # output slot: amax within the interval's reach, everything else (and the operand slots) untouched
        bits, rest = E.fp8_slots_read(slots)
        bits0, rest0 = E.fp8_slots_read(slots0)
        assert np.array_equal(rest.view(np.uint32), rest0.view(np.uint32)) and bits[0] == 0 and bits[1] == 0, label + ": slots were written"
        amax = float(bits[2:3].view(np.float32)[0])
        least = torch.where(lo > 0, lo, torch.where(hi < 0, -hi, torch.zeros_like(lo)))
        a_lo, a_hi = float(least.max()), float(torch.maximum(lo.abs(), hi.abs()).max())
        print("%s amax %.9g in [%.9g, %.9g]" % (label, amax, a_lo, a_hi))
        assert a_lo <= amax <= a_hi, (label, amax, a_lo, a_hi)
        res.update(amax_bits=int(bits[2]))
    else:
        bound = vb + BF16_RND * (ref.abs() + vb)          # (no noisy form has a bf16 output)
        got = obuf.to(torch.float64)
        assert not bool((obuf[:, :m, :n] == SENT).any()), label + ": output elements inside [M][N] were not written"
        res["usage"] = _assert_close(label + " out [%s]" % name, got[:, :m, :n], ref, bound)
        inside = torch.zeros_like(obuf, dtype=torch.bool)
        inside[:, :m, :n] = True
        _assert_sentinel(label + " out", obuf.to(torch.float32), inside)
        if n_valid < n:
            assert bool((got[:, :m, n_valid:n] == 0).all()), label + ": columns [n_valid, N) must be exact zeros"
        bits, _ = E.fp8_slots_read(slots)
        assert torch.equal(slots, slots0) and not bits.any(), label + ": slots were written"

    # ---- relu mask written by the forward ---------------------------------------------------------------------
    if op == FWD and mask:
        words = mwords.cpu().numpy().view(np.uint16)
        bits = np.stack([mask_decode(words[b], m, n) for b in range(nbatch)])
        want = (pre > 0).cpu().numpy()
        und = (pre.abs() <= accb).cpu().numpy()
        und[:, :, n_valid:] = False                   # padding columns: pre-activation exactly 0, bit exactly 0
        share = und[:, :, :n_valid].mean()
        print("%s mask: undecided share %.5f %% (cap 0.5 %%)" % (label, 100 * share))
        assert k <= 1024 and share <= 0.005, (label, share)
        wrong = (bits != want) & ~und
        assert not wrong.any(), "%s: %d mask bits differ, first at %s" % (label, wrong.sum(), tuple(np.argwhere(wrong)[0]))
        keep = np.ones(words.shape, bool)
        keep[:, :nblk, :n, :] = False
        assert (words[keep] == MASK_SENT).all(), label + ": mask words outside [ceil(M / 32)][N] were written"

    # ---- column sums -------------------------------------------------------------------------------------------
    if cs_mode != CS_NONE:
        g = lambda t: torch.from_numpy(colsum_groups(t.cpu().numpy())).to(DEV)
        rows = nbatch * tiles_m
        inside = torch.zeros_like(cs1, dtype=torch.bool)
        inside[:rows, :n] = True
        s1, b1 = g(v), g(vb) + 64 * U * g(v.abs())
        _assert_close(label + " cs1", cs1[:rows, :n].double(), s1, b1, b1)
        WORST["acc"] = max(WORST["acc"], _usage((cs1[:rows, :n].double() - s1).abs(), b1)[0])
        _assert_sentinel(label + " cs1", cs1, inside)
        if cs_mode == CS_SUM:
            _assert_sentinel(label + " cs2", cs2, torch.zeros_like(inside))
        else:
            xh = (h - mu) * rstd
            xh[:, :, n_valid:] = 0
            # h - mu, its product with v and the fma round once each; the 64-term sum as above
            s2, b2 = g(v * xh), g(vb * xh.abs()) + 68 * U * g((v * xh).abs())
            _assert_close(label + " cs2", cs2[:rows, :n].double(), s2, b2, b2)
            _assert_sentinel(label + " cs2", cs2, inside)
    return res


def _random_bits(m, n, nbatch, key):
    return torch.from_numpy(_rng(m, n, nbatch, key).random((nbatch, m, n)) < 0.5).to(DEV)


# =============================================================================================================
# 0. the test's own encoder / decoder / Q on the device
# =============================================================================================================
@pytest.mark.parametrize("fmt", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_reference_rounding_on_the_device_is_the_mirrors(fmt):
    """_q8 (float64 on the device) equals oracle.fp8_round, and _decode inverts _encode on the grid"""
    x = _rng(fmt, 1).standard_normal(200000) * 10.0 ** _rng(fmt, 2).uniform(-7, 5, 200000)
    lim = GRID[fmt][2]
    x = np.concatenate([x, [0.0, -0.0, lim, -lim, 1.01 * lim, 1e30, -1e30], 2.0 ** np.arange(-20.0, 17.0), 1.5 * 2.0 ** np.arange(-20.0, 16.0),
                        1.25 * 2.0 ** np.arange(-20.0, 16.0)])
    want = O.fp8_round(x, 'e4m3' if fmt == E4M3 else 'e5m2')
    got = _q8(torch.from_numpy(x).to(DEV), fmt).cpu().numpy()
    assert np.array_equal(got, want)
    codes = torch.arange(256, dtype=torch.uint8, device=DEV)
    vals = _decode(codes, fmt)
    finite = torch.isfinite(vals)
    assert torch.equal(_encode(vals[finite].float().cpu(), fmt).to(DEV) & 0x7F | (codes[finite] & 0x80), codes[finite])
    assert bool(torch.isnan(vals[POISON])) and bool(torch.isnan(vals[0xFF]))


# =============================================================================================================
# 1. products x output forms (nbatch 3), on both tiles
# =============================================================================================================
SCALED = {FWD: (2.0 ** 4, 2.0 ** 7, 2.0 ** 5), DX: (2.0 ** 12, 2.0 ** 6, 2.0 ** 16)}       # non-unit, unequal
TILE_SHAPES = {1: [(256, 256, 128), (50, 192, 256), (300, 192, 384), (512, 384, 256)],      # exact; ragged M, tile astride N; ring wraps; patches
               3: [(512, 512, 256), (300, 512, 384)]}
ALL_SHAPES = [(1, 128) + s for s in TILE_SHAPES[1]] + [(3, 256) + s for s in TILE_SHAPES[3]] + [(3, 128, 300, 192, 256)]   # N % 256 != 0: the small tile
SHAPE_IDS = ["%d-%dx%dx%d" % (s[0], s[2], s[3], s[4]) for s in ALL_SHAPES]


@pytest.mark.parametrize("cfg,tile,m,n,k", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("images", ["both", "q8", "q8t"])
def test_forward_to_fp8(cfg, tile, m, n, k, images):
    """relu + noise (Irwin-Hall) + mask, e4m3 images under non-unit unequal slot scales; rows [M, round_up(M, 16)) of the
    transposed image are zeros although the noise alone would make them non-zero"""
    run8(FWD, m, n, k, tile, cfg, act=RELU, nbatch=3, out=images, noise=NOISE, mask=True, scales=SCALED[FWD])


@pytest.mark.parametrize("cfg,tile,m,n,k", [ALL_SHAPES[1], ALL_SHAPES[5]], ids=[SHAPE_IDS[1], SHAPE_IDS[5]])
def test_forward_to_fp8_true_gaussian_noise(cfg, tile, m, n, k):
    run8(FWD, m, n, k, tile, cfg, act=RELU, nbatch=3, out="both", noise=dict(NOISE, row0=36, seg_step=2), gauss=True, mask=True,
         scales=SCALED[FWD])


@pytest.mark.parametrize("cfg,tile,m,n,k", [ALL_SHAPES[2], ALL_SHAPES[4]], ids=[SHAPE_IDS[2], SHAPE_IDS[4]])
def test_forward_to_fp8_unit_scales_without_operand_slots(cfg, tile, m, n, k):
    """null operand slots: the accumulator is taken through acc_scale"""
    run8(FWD, m, n, k, tile, cfg, act=RELU, nbatch=3, out="both", noise=dict(NOISE, iter_step=1, seg_step=0), mask=True, null_slots=True)


@pytest.mark.parametrize("cfg,tile,m,n,k", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("form", ["relu-mask", "relu", "linear-cs", "softplus"])
def test_forward_to_bf16(cfg, tile, m, n, k, form):
    act = dict(relu=RELU, linear=LIN, softplus=SOFTPLUS)[form.split("-")[0]]
    run8(FWD, m, n, k, tile, cfg, act=act, nbatch=3, mask=(form == "relu-mask"), cs_mode=CS_SUM if form == "linear-cs" else CS_NONE,
         scales=SCALED[FWD] if form != "relu" else (1.0, 1.0, 1.0))


@pytest.mark.parametrize("cfg,tile,m,n,k", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("images,cs_mode", [("both", CS_NONE), ("both", CS_SUM), ("q8", CS_SUM), ("q8t", CS_NONE)],
                         ids=["both-nocs", "both-cs", "q8-cs", "q8t-nocs"])
def test_dx_to_fp8(cfg, tile, m, n, k, cs_mode, images):
    """e5m2 x e4m3 -> e5m2 through the relu mask (random reference bits, junk bits outside [M][N]), bias-gradient sums on the fly"""
    run8(DX, m, n, k, tile, cfg, act=RELU, nbatch=3, out=images, mask=_random_bits(m, n, 3, cfg), cs_mode=cs_mode,
         scales=SCALED[DX] if cs_mode == CS_SUM else (1.0, 1.0, 2.0 ** 10))


@pytest.mark.parametrize("cfg,tile,m,n,k", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cs_mode", [CS_NONE, CS_SUM, CS_SUM_XHAT], ids=["nocs", "cs", "xhat"])
def test_dx_to_bf16(cfg, tile, m, n, k, cs_mode):
    run8(DX, m, n, k, tile, cfg, act=LIN, nbatch=3, cs_mode=cs_mode, scales=SCALED[DX], n_valid=n)


def test_all_zero_output_leaves_amax_at_zero():
    res = run8(DX, 300, 192, 256, 128, 1, act=RELU, nbatch=3, out="both", mask=torch.zeros((3, 300, 192), dtype=torch.bool, device=DEV),
               scales=SCALED[DX])
    assert res["amax_bits"] == 0


@pytest.mark.parametrize("cfg,tile", [(1, 128), (3, 256)])
@pytest.mark.parametrize("out", ["both", "bf16"])
def test_n_valid_columns_stay_zero(cfg, tile, out):
    """columns [n_valid, N): zero weights, a non-zero bias entry and noise -- none of it may show, and their mask bits are 0"""
    run8(FWD, 200, 256, 128, tile, cfg, act=RELU, nbatch=3, n_valid=250, out=out, noise=NOISE if out == "both" else None, mask=True,
         scales=SCALED[FWD])


@pytest.mark.parametrize("m,n,k,nbatch,tile", [(2048, 2048, 512, 3, 256), (1792, 2048, 512, 3, 128), (2048, 2048, 384, 3, 128)],
                         ids=["t256=192-k512", "t256=168-k512", "t256=192-k384"])
def test_measured_choice_of_tile(m, n, k, nbatch, tile):
    """kc_cfg = -1: the large tile from K >= 512 and 192 tiles of 256 x 256 on, the small one on either side of that"""
    run8(FWD, m, n, k, tile, -1, act=LIN, nbatch=nbatch, scales=SCALED[FWD])


@pytest.mark.parametrize("m,n,nbatch,cfg,tile", [(1024, 3072, 3, 1, 128), (2048, 2304, 4, 3, 256)], ids=["576-tiles-512-blocks", "288-tiles-256-blocks"])
def test_more_tiles_than_blocks(m, n, nbatch, cfg, tile):
    """the persistent loop takes a second tile on some blocks; the tile count is a multiple of 8 (xcd_tile remaps) and the tile
    rows a multiple of 4 (patch order)"""
    run8(FWD, m, n, 128, tile, cfg, act=RELU, nbatch=nbatch, out="both", noise=NOISE, mask=True, scales=SCALED[FWD])


# =============================================================================================================
# 2. weight gradient: e4m3 x e5m2 -> fp32 slabs, split-K
# =============================================================================================================
def slab8(m, n, k, splits, cfg, scales, kchunk=None, key=0):
    rng = _rng(8, SLAB, m, n, k, splits, key)
    sa, sb = scales
    xb, x, xh = _draw8(rng, (m, k), 1.0, sa, E4M3)                   # X^T [M][reduction]
    db, dy, dh = _draw8(rng, (n, k), 2.0 ** -6, sb, E5M2)            # dY^T [N][reduction]
    ldo = n + PAD
    slab = torch.full((splits, m + GAP, ldo), SENT, dtype=torch.float32, device=DEV)
    slots = _slots((sa, TARGET[E4M3]), (sb, TARGET[E5M2]))
    kchunk = k // splits if kchunk is None else kchunk
    d = dict(dtype=FP8, op=SLAB, m=m, n=n, k=k, splits=splits, kchunk=kchunk, kc_cfg=cfg, a=_embed8(xb[None], m + GAP, k + PAD), a_si=k + PAD, a_sk=1,
             b=_embed8(db[None], n + GAP, k + PAD), b_sk=1, b_sj=k + PAD, slab=slab, slab_stride=(m + GAP) * ldo, ldo=ldo,
             slot_a=slots[0], slot_b=slots[1])
    refs, bounds, plains = [], [], []
    for s in range(splits):
        sl = slice(s * kchunk, (s + 1) * kchunk)
        xs, ds = x[:, sl], dy[:, sl]
        refs.append(xs @ ds.t())
        b, plain = _acc_bound(kchunk, xs.abs() @ ds.abs().t(), xh[:, sl] @ dh[:, sl].t())
        bounds.append(b)
        plains.append(plain)
    return d, slab, torch.stack(refs), (torch.stack(bounds), torch.stack(plains)), slots


def check_slabs(label, slab, ref, bounds, m, n):
    """per slab and summed; "accumulation term used" = the error over the plain fp32 rule 2 K 2^-24 mag, for information"""
    bound, plain = bounds
    got = slab[:, :m, :n].double()
    assert bool(torch.isfinite(got).all()), label + ": non-finite slab (a pad column or a row outside the operand was read)"
    for s in range(ref.shape[0]):
        WORST["plain"] = max(WORST["plain"], _usage((got[s] - ref[s]).abs(), plain[s])[0])
        WORST["acc"] = max(WORST["acc"], _assert_close("%s slab %d" % (label, s), got[s], ref[s], bound[s], plain[s]))
    _assert_close(label + " sum", got.sum(0), ref.sum(0), bound.sum(0))
    inside = torch.zeros_like(slab, dtype=torch.bool)
    inside[:, :m, :n] = True
    _assert_sentinel(label, slab, inside)


@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("m,n,cfg,tile", [(200, 192, 1, 128), (256, 512, 3, 256), (256, 512, 1, 128)], ids=["200x192-small", "256x512-large", "256x512-small"])
def test_weight_gradient_splits(m, n, cfg, tile, splits):
    from mr_gan_amd import engine as E
    d, slab, ref, bound, slots = slab8(m, n, 512, splits, cfg, (2.0 ** 3, 2.0 ** 13) if splits != 2 else (1.0, 1.0))
    slots0 = slots.clone()
    name = _launch(E, E.debug_gemm_desc(**d))
    assert name == _name(SLAB, tile)
    check_slabs("fp8 dW %dx%dx512/%d %s" % (m, n, splits, name), slab, ref, bound, m, n)
    assert torch.equal(slots, slots0)


# =============================================================================================================
# 3. quant8_kernel
# =============================================================================================================
def _quant_problem(fmt, rows, prow, cols, ld, nb, scale, key=0):
    rng = _rng(88, fmt, rows, cols, key)
    lim = GRID[fmt][2]
    # magnitudes from far below the smallest subnormal of v * scale to above the saturation limit, both present by construction
    x = rng.standard_normal((nb, rows, cols)) * 10.0 ** rng.uniform(-7, 1, (nb, rows, cols))
    x[:, 0, :8] = [4 * lim / scale, -4 * lim / scale, 1.001 * lim / scale, lim / scale, 2.0 ** (GRID[fmt][1] - GRID[fmt][0]) / scale,
                   -1.5 * 2.0 ** (GRID[fmt][1] - GRID[fmt][0]) / scale, 0.5 * 2.0 ** (GRID[fmt][1] - GRID[fmt][0]) / scale, 0.0]
    v = torch.from_numpy(x).to(torch.bfloat16)
    want = _encode(v.float() * scale, fmt)                         # bf16 x power of two: exact in fp32, then clamp and cast
    amax = v.float().abs().max().numpy().view(np.uint32)
    src = _embed(v.to(DEV), rows + GAP, ld, torch.bfloat16)
    return src, want.to(DEV), int(amax)


def _same_bytes(a, b):
    """equal, +0 and -0 taken as one code"""
    return (a == b) | (((a | b) & 0x7F) == 0)


@pytest.mark.parametrize("rows,prow,cols,ld,scale", [(300, 320, 192, 256, 2.0 ** 3), (64, 64, 64, 64, 2.0 ** -2)], ids=["300-320-192", "64-64-64"])
@pytest.mark.parametrize("images", ["both", "dst", "dstt"])
@pytest.mark.parametrize("fmt", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_quant8(fmt, images, rows, prow, cols, ld, scale):
    from mr_gan_amd import engine as E
    nb = 3
    src, want, amax_bits = _quant_problem(fmt, rows, prow, cols, ld, nb, scale)
    slot = _slots((scale, TARGET[fmt]))
    slot0 = slot.clone()
    ldd, bs = cols + PAD, prow + TGAP
    lddt = nb * bs + PAD
    dst = torch.full((nb, prow + GAP, ldd), POISON, dtype=torch.uint8, device=DEV) if images != "dstt" else None
    dstt = torch.full((cols + GAP, lddt), POISON, dtype=torch.uint8, device=DEV) if images != "dst" else None
    rc = E.debug_quant8(src, (rows + GAP) * ld, ld, rows, cols, nb, prow, slot[0], fmt, dst=dst, dst_bs=(prow + GAP) * ldd, ldd=ldd,
                        dstt=dstt, dstt_bs=bs, lddt=lddt)
    assert rc == 0, (rc, E.load_library().mrgan_last_error())
    label = "quant8 fmt%d %s %dx%d" % (fmt, images, rows, cols)
    if dst is not None:
        bad = ~_same_bytes(dst[:, :rows, :cols], want)
        assert not bool(bad.any()), "%s: %d bytes differ from the encoder, first at %s" % (label, int(bad.sum()), tuple(int(v[0]) for v in torch.nonzero(bad, as_tuple=True)))
        assert bool((dst[:, rows:prow, :cols] == 0).all()), label + ": rows [rows, prow) must be zero bytes"
        inside = torch.zeros_like(dst, dtype=torch.bool)
        inside[:, :prow, :cols] = True
        _assert_sentinel(label + " dst", dst, inside, value=POISON)
    if dstt is not None:
        inside = torch.zeros_like(dstt, dtype=torch.bool)
        for b in range(nb):
            bad = ~_same_bytes(dstt[:cols, b * bs:b * bs + rows].t(), want[b])
            assert not bool(bad.any()), "%s: %d transposed bytes of batch %d differ from the encoder" % (label, int(bad.sum()), b)
            assert bool((dstt[:cols, b * bs + rows:b * bs + prow] == 0).all()), label + ": transposed rows [rows, prow) must be zero bytes"
            inside[:cols, b * bs:b * bs + prow] = True
        _assert_sentinel(label + " dstt", dstt, inside, value=POISON)
    bits, rest = E.fp8_slots_read(slot)
    assert int(bits[0]) == amax_bits, (label, hex(int(bits[0])), hex(amax_bits))
    assert np.array_equal(rest.view(np.uint32), E.fp8_slots_read(slot0)[1].view(np.uint32))


def test_quant8_refusals():
    from mr_gan_amd import engine as E
    nb, rows, prow, cols, ld = 2, 64, 64, 64, 64
    src = torch.zeros((nb, rows, ld), dtype=torch.bfloat16, device=DEV)
    slot = _slots((1.0, TARGET[E4M3]))
    ldd, bs, lddt = 128, 128, 512
    dst = torch.full((nb, prow, ldd), POISON, dtype=torch.uint8, device=DEV)
    dstt = torch.full((cols, lddt), POISON, dtype=torch.uint8, device=DEV)
    base = dict(src=src, src_bs=rows * ld, ld=ld, rows=rows, cols=cols, nb=nb, prow=prow, slot=slot[0], fmt=E4M3, dst=dst, dst_bs=prow * ldd,
                ldd=ldd, dstt=dstt, dstt_bs=bs, lddt=lddt)
    for c in (dict(cols=32), dict(prow=96, rows=60), dict(ld=68), dict(slot=None), dict(nb=0), dict(ldd=120), dict(lddt=520), dict(dstt_bs=136)):
        assert E.debug_quant8(**dict(base, **c)) == -3, c
    assert bool((dst == POISON).all()) and bool((dstt == POISON).all()) and not E.fp8_slots_read(slot)[0].any()
    assert E.debug_quant8(**base) == 0                             # and the unmodified problem runs
    assert bool((dst[:, :, :cols] == 0).all()) and bool((dstt[:, :prow] == 0).all()) and bool((dstt[:, bs:bs + prow] == 0).all())


# =============================================================================================================
# 4. fp8_update_scales_kernel
# =============================================================================================================
def test_update_scales_matches_the_mirror_bit_for_bit():
    from mr_gan_amd import engine as E
    f = np.float32
    t4, t5 = f(TARGET[E4M3]), f(TARGET[E5M2])
    at = f(224.0 / 64.0)                                         # target / amax = 2^6 exactly
    amax = [f(0.0), f(1e-40), f(1.1754942e-38), np.nextafter(at, f(np.inf)), at, np.nextafter(at, f(0.0)),
            f(224.0 * 2.0 ** -110), f(3.0e38), f(2.0 ** 100), f(1.0), f(3.7), f(224.0), f(225.0), f(2.0 ** -20)]
    rows = []
    for i, a in enumerate(amax):
        for tgt, sc in ((t4, f(2.0 ** 5)), (t5, f(2.0 ** -3))):
            rows.append((a, sc, f(1.0) / sc, tgt))
    rows = rows + [(f(7.0), f(4.0), f(0.25), t4)] * 41            # more slots than one block of 64 threads
    slots = E.fp8_slots(rows, DEV)
    assert 0 < float(amax[1]) < 1.1754942e-38                     # a subnormal amax: target / amax overflows to infinity
    E.debug_fp8_update_scales(slots)
    bits, rest = E.fp8_slots_read(slots)
    assert not bits.any(), "amax_bits must be cleared"
    for i, (a, sc, inv, tgt) in enumerate(rows):
        m = O.Fp8Slots()
        key, fmt = 'x', ('e4m3' if tgt == t4 else 'e5m2')
        m.scale[key], m.amax[key], m.fmt[key] = sc, a, fmt
        m.update()
        want = np.array([m.scale[key], f(1.0) / m.scale[key] if a > 0 else inv, tgt], dtype=np.float32)
        assert np.array_equal(rest[i].view(np.uint32), want.view(np.uint32)), (i, float(a), float(tgt), rest[i].tolist(), want.tolist())
        if a == 0:
            assert rest[i][0] == sc and rest[i][1] == inv            # nobody wrote: the scale stays


# =============================================================================================================
# 5. refusals
# =============================================================================================================
def test_launcher_refusals():
    """launch_gemm_fp8 returns -3 and launches nothing; every sentinel stays"""
    from mr_gan_amd import engine as E
    m = n = 128
    k, ld = 128, 256
    a = torch.zeros((m, ld), dtype=torch.uint8, device=DEV)
    b = torch.zeros((n, ld), dtype=torch.uint8, device=DEV)
    out = torch.full((m, n), SENT, dtype=torch.bfloat16, device=DEV)
    q8 = torch.full((m, n + 32), POISON, dtype=torch.uint8, device=DEV)
    q8t = torch.full((n, m + 32), POISON, dtype=torch.uint8, device=DEV)
    slab = torch.full((2, m, n), SENT, dtype=torch.float32, device=DEV)
    mask = torch.full((m // 32, n, 2), MASK_SENT, dtype=torch.int16, device=DEV)
    cs1 = torch.full((2, n), SENT, dtype=torch.float32, device=DEV)
    cs2 = torch.full((2, n), SENT, dtype=torch.float32, device=DEV)
    slots = _slots((1.0, 224.0), (1.0, 224.0), (1.0, 224.0))
    slots0 = slots.clone()
    ops = dict(dtype=FP8, m=m, n=n, k=k, a=a, a_si=ld, a_sk=1, b=b, b_sk=1, b_sj=ld, n_valid=n, slot_a=slots[0], slot_b=slots[1])
    to_bf16 = dict(ops, op=FWD, out=out, ldo=n)
    images = dict(q8=q8, ldq8=n + 32, q8t=q8t, ldq8t=m + 32, q8t_bs=m + 16, slot_o=slots[2])
    fwd8 = dict(ops, op=FWD, act=RELU, mask=mask, ldm=n, **dict(images, **NOISE))
    dx8 = dict(ops, op=DX, act=RELU, mask=mask, ldm=n, **images)
    dw = dict(ops, op=SLAB, slab=slab, slab_stride=m * n, ldo=n, k=256, splits=2, kchunk=128)
    big = 1 << 24                                    # 128 rows * 2^24 bytes = 2^31
    assert m * big >= 1 << 31 and m * (big - 16) < 1 << 31
    cases = [
        dict(to_bf16, k=192), dict(to_bf16, a_sk=2), dict(to_bf16, b_sk=2), dict(to_bf16, splits=2), dict(dx8, splits=2),
        dict(dw, kchunk=256),                                        # kchunk * splits != K
        dict(dw, splits=1, kchunk=128),                              # one slab must cover K
        dict(fwd8, slot_o=None), dict(dx8, slot_o=None),
        dict(fwd8, ldq8=n + 24), dict(fwd8, q8t_bs=m + 24), dict(fwd8, ldq8t=m + 40),
        dict(fwd8, out=out, ldo=n), dict(to_bf16, out=None),         # both output forms, neither
        dict(fwd8, sigma=0.0), dict(fwd8, cs_mode=CS_SUM, cs1=cs1, ldcs=n),
        dict(dx8, q8=None, q8t=None, slot_o=None, out=out, ldo=n),   # dX relu -> bf16
        dict(dx8, act=LIN, mask=None),                               # dX linear -> fp8
        dict(ops, op=DX, out=out, ldo=n, cs_mode=CS_SUM_SQ, cs1=cs1, cs2=cs2, ldcs=n),
        dict(dw, slab=None),
        dict(to_bf16, slot_a=None), dict(to_bf16, slot_b=None),
        dict(to_bf16, a_si=big), dict(to_bf16, b_sj=big),
    ]
    for c in cases:
        rc, name = E.debug_gemm_launch(E.debug_gemm_desc(**c))
        assert (rc, name) == (-3, ""), ({kk: vv for kk, vv in c.items() if not isinstance(vv, torch.Tensor)}, rc, E.load_library().mrgan_last_error())
    assert bool((out == SENT).all()) and bool((slab == SENT).all()) and bool((cs1 == SENT).all()) and bool((cs2 == SENT).all())
    assert bool((q8 == POISON).all()) and bool((q8t == POISON).all()) and bool((mask == MASK_SENT).all()) and torch.equal(slots, slots0)
    # and the unmodified problems run
    for d, tile_op in ((to_bf16, FWD), (fwd8, FWD), (dx8, DX), (dw, SLAB)):
        rc, name = E.debug_gemm_launch(E.debug_gemm_desc(**d))
        assert (rc, name) == (0, _name(tile_op, 128)), (rc, name, E.load_library().mrgan_last_error())
    assert bool((out == 0).all()) and bool((slab == 0).all())


def test_session_figures():
    """prints the largest accumulation-term usage and two-code share the cases above saw (DESIGN.md quotes them)"""
    print("fp8 kernel tests: largest usage of the accumulation bound on fp32 outputs %.4f (of the plain fp32 rule alone %.4f), "
          "largest share of elements with two admissible codes %.4f %%" % (WORST["acc"], WORST["plain"], 100 * WORST["two"]))
