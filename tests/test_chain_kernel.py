"""Kernel-level parity of the row-block chain kernel (csrc/gemm_chain.hip, csrc/chain.h) through mrgan_debug_chain: one launch per
case, every one of the 16 instantiations (variant x 64/32-row blocks x Irwin-Hall/true-Gaussian x single/group), the kernel's
name asserted.  Caller-owned buffers: every pitch wider than its width, GAP rows between segments, the models model_stride
bytes apart inside one arena; outputs pre-filled with SENT (masks MASK_SENT words), everything outside the written region of
include/mrgan_debug.h asserted untouched.

Reference, stage by stage in fp64 (one fp64 run of all three products would diverge wherever a relu decision or a bf16 rounding
differs): stage j's input is the bf16 image the kernel itself stored for stage j - 1 -- copy_out copies the very LDS image
the next product reads, so an image overwritten too early shows as stage j - 1 failing its own reference.
    forward   v = relu(A W^T + bias), out = bf16(v + sigma * noise); padding columns exact zeros (the bias beyond n_valid is non-zero)
    masks     decoded and compared on valid rows; elements with |pre| within the accumulation bound are undecided (share capped
              at 0.5 %, held for the reference alone by tests/test_chain_cases_cpu.py)
    dX        out = bit ? A W : 0 with the kernel's own HBM mask words as `bit` (D tail: the words fwd[1] / fwd[0] wrote in the same
              launch for dx[0] / dx[1], the caller's for dx[2]; G backward: all the caller's) -- no dX element is undecided
    cs        per (segment, row block): the fp64 sum of the kept, unrounded values over the valid rows
    head      aux_refs.head_rows / head_backward on the kernel's stored features and stored fwd[2] mask
    fm        aux_refs.fm on the fp64 sums of the fp32 partial rows; the relu sign is fm_feat > 0
Tolerances ("Kernel-level tolerance of the chain kernel"), U = 2^-24: a product element 2 K U (|A||W| + |bias|); a bf16
store adds 2^-8 |value|; Irwin-Hall noise is exact and its fma rounds once (4 U |noise| as in test_gemm_kernels.py); true Gaussian
sigma (GAUSS_A + GAUSS_B |n|) + U |value|; a column sum: the sum of its elements' bounds + block_rows U sum |v|; head and fm: the
bounds of test_head_wide and test_fm (tests/test_aux_kernels.py), the fm gradient with the one-fold term because chain_fmgrad
adds the fake and subtracts the real partial rows in one accumulator.
"""
import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests import aux_refs as R
from tests import gaussian_noise as GN
from tests.helpers import DEV, SENT, _assert_sentinel, _rng, mask_decode, mask_encode
from tests.test_aux_kernels import (BF16, BF16_RND, GAP, GAUSS_A, GAUSS_B, U, Arena, _blocks, _close, _fm_bounds, _head_delta, _head_grad_bounds,
                                    _head_row_bounds, _head_undecided, _split)
from tests.test_gemm_kernels import MASK_SENT

DT, GF, GB = 0, 1, 2
SEED = 0x5EED5EED0BADF00D
ITER = 7
SIGMA = (0.5, 0.3, 0.2)              # layer noise behind the three forward products; sites 3, 4, 5 as in the engine
MASK_CAP = 0.005                     # test_gemm_kernels.py: the undecided share of a relu mask for K <= 1024
KP = 8
# K0(valid) -> N1 -> N2 -> N3; the dX run is the mirror image
WIDTHS = {"stock": ((512, 500), (256, 250), (256, 250), (256, 250)),       # the engine's tail: dX through D3 takes two full passes
          "min": ((128, 100), (128, 100), (128, 128), (128, 72)),          # every reduction exactly two k-tiles
          "mixed": ((320, 300), (192, 180), (128, 100), (256, 250))}       # waves without columns, a second pass of 64 columns


def _c(variant, widths, rows, nseg, block_rows, models=1, gauss=0, row0=0, cs=True, stream=False, npf=3, npr=3, key=0):
    return dict(variant=variant, widths=widths, rows=rows, nseg=nseg, block_rows=block_rows, models=models, gauss=gauss, row0=row0, cs=cs,
                stream=stream, npf=npf, npr=npr, key=key)


CASES = [
    _c(DT, "stock", 130, 3, 64), _c(DT, "stock", 50, 3, 64, gauss=1, row0=6), _c(DT, "min", 130, 2, 64, stream=True),
    _c(DT, "min", 50, 1, 64, models=3), _c(DT, "mixed", 130, 3, 64, row0=38), _c(DT, "mixed", 50, 2, 64, models=3, gauss=1),
    _c(DT, "stock", 64, 1, 64), _c(DT, "mixed", 64, 3, 64, gauss=1, cs=False), _c(DT, "stock", 130, 3, 64, models=3, key=1),
    _c(GF, "stock", 130, 2, 64), _c(GF, "stock", 50, 2, 32), _c(GF, "stock", 130, 1, 32, gauss=1, row0=6, cs=False),
    _c(GF, "stock", 50, 3, 64, gauss=1), _c(GF, "min", 130, 2, 32), _c(GF, "min", 50, 1, 64, models=3, cs=False),
    _c(GF, "min", 64, 2, 32, models=3), _c(GF, "mixed", 130, 3, 64, models=3, gauss=1), _c(GF, "mixed", 50, 2, 32, models=3, gauss=1, row0=38),
    _c(GF, "mixed", 130, 2, 32, cs=False), _c(GF, "mixed", 50, 1, 64), _c(GF, "min", 130, 2, 64, gauss=1), _c(GF, "min", 50, 2, 32, gauss=1),
    _c(GB, "stock", 130, 1, 64), _c(GB, "stock", 50, 1, 32, npf=70, npr=5), _c(GB, "stock", 130, 1, 32, models=3, npf=5, npr=70),
    _c(GB, "stock", 50, 1, 64, models=3, npf=1, npr=1, cs=False), _c(GB, "min", 130, 1, 32, npf=1, npr=1), _c(GB, "min", 50, 1, 64, npf=2, npr=3),
    _c(GB, "mixed", 130, 1, 64, npf=17, npr=70), _c(GB, "mixed", 50, 1, 32, cs=False), _c(GB, "mixed", 64, 2, 32, models=3, npf=66, npr=65),
    _c(GB, "min", 64, 1, 64, models=3), _c(GB, "mixed", 130, 1, 32, npf=4, npr=1),
]
ALL_KERNELS = sorted("chain_kernel<%d, %d, %d, %d>" % (v, mi, g, grp) for v in (DT, GF, GB) for mi in (2, 1) for g in (0, 1) for grp in (0, 1)
                     if not (v == DT and mi == 1) and not (v == GB and g == 1))
SEEN = {}                            # case id -> the kernel name the launch reported


def case_id(c):
    return "%s-%s-r%d-s%d-b%d-m%d-g%d-o%d-cs%d-st%d-p%d+%d-k%d" % (("DT", "GF", "GB")[c["variant"]], c["widths"], c["rows"], c["nseg"], c["block_rows"],
                                                                 c["models"], c["gauss"], c["row0"], c["cs"], c["stream"], c["npf"], c["npr"], c["key"])


def kernel_name(c):
    return "chain_kernel<%d, %d, %d, %d>" % (c["variant"], c["block_rows"] // 32, 1 if (c["gauss"] and c["variant"] != GB) else 0, 1 if c["models"] > 1 else 0)


def _bf16(x):
    """float64 array -> the nearest bf16 values (ties to even), as float64; numpy only"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + (((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def fwd_specs(c):
    w = WIDTHS[c["widths"]]
    return [(w[i][0], w[i + 1][0], w[i + 1][1]) for i in range(3)]          # (K, N, n_valid)


def dx_specs(c):
    w = WIDTHS[c["widths"]]
    return [(w[3 - i][0], w[2 - i][0], w[2 - i][1]) for i in range(3)]


def chain_inputs(c):
    """every draw of a case, numpy only (tests/test_chain_cases_cpu.py walks the same list); all values exact in their storage type"""
    w = WIDTHS[c["widths"]]
    M, S, rows = c["models"], c["nseg"], c["rows"]
    rng = _rng(31, c["variant"], rows, S, c["block_rows"], M, c["gauss"], c["key"], *[v for p in w for v in p])
    d = dict(rng=rng)
    a0 = _bf16(rng.standard_normal((M, S, rows, w[0][0])))
    a0[..., w[0][1]:] = 0.0                                # the padding columns of an activation are zeros in the engine
    d["a0"] = a0
    d["Wf"], d["bf"], d["Wd"], d["dxbits"] = [], [], [], []
    for K, N, nv in fwd_specs(c):
        W = _bf16(rng.standard_normal((M, N, K)) / np.sqrt(K))
        W[:, nv:] = 0.0                                    # padding columns have zero weights ...
        d["Wf"].append(W)
        d["bf"].append(_bf16(0.3 * rng.standard_normal((M, N))))          # ... and a bias that must not leak
    for K, N, nv in dx_specs(c):
        W = _bf16(rng.standard_normal((M, N, K)) / np.sqrt(K))
        W[:, nv:] = 0.0
        d["Wd"].append(W)
        d["dxbits"].append(rng.random((M, S, rows, N)) < 0.5)
    feat, fv = w[3]
    c1, c2 = 1, 5
    W6 = (rng.standard_normal((M, feat, KP)) / np.sqrt(feat)).astype(np.float32)      # junk in columns >= classes, rows >= feat_valid
    W6[:, :, c2] = W6[:, :, c1]                            # two identical logits: argmax ties go to the first
    b6 = (0.3 * rng.standard_normal((M, KP))).astype(np.float32)
    b6[:, c2] = b6[:, c1]
    d.update(W6=W6, b6=b6, labels=rng.integers(0, 6, (M, 3, rows)).astype(np.int32), c1=c1, c2=c2)
    ff = _bf16(np.maximum(rng.standard_normal((M, rows, feat)) - 0.3, 0.0))
    ff[..., fv:] = 0.0
    d["fm_feat"] = ff
    return d


def noise(c, m, site, seg, N):
    """(sigma-free) standard normals [rows][N] of model m at (site, segment) as the kernel keys them, and their bound"""
    args = (SEED + m, site, seg, ITER, c["rows"], N, c["row0"])
    if c["gauss"]:
        n = GN.gaussian_normal(*args)
        return n, GAUSS_A + GAUSS_B * np.abs(n)
    n = O.device_noise_sums(*args).astype(np.float64) * O.NOISE_SCALE
    return n, 4 * U * np.abs(n)                            # sigma * NOISE_SCALE rounded to fp32, then one fma


def fwd_reference(c, m, i, x, W, b):
    """stage input x [S][rows][K] -> (pre, accb, v, ref, bound before the bf16 store) of forward product i"""
    K, N, nv = fwd_specs(c)[i]
    bv = b.copy()
    bv[nv:] = 0.0
    pre = x @ W.T + bv
    accb = 2 * K * U * (np.abs(x) @ np.abs(W).T + np.abs(bv))
    v = np.maximum(pre, 0.0)
    nz, nzb = np.zeros_like(v), np.zeros_like(v)
    for s in range(c["nseg"]):
        n, e = noise(c, m, 3 + i, s, N)
        nz[s], nzb[s] = SIGMA[i] * n, SIGMA[i] * e
    nz[..., nv:], nzb[..., nv:] = 0.0, 0.0
    ref = v + nz
    return pre, accb, v, ref, accb + nzb + (U * np.abs(ref) if c["gauss"] else 0.0)


def _E():
    from mr_gan_amd import engine as E
    return E


def _np(t):
    return t.detach().to("cpu", torch.float64).numpy() if t.dtype != torch.int16 else t.detach().cpu().numpy().view(np.uint16)


def _inside(t, *sl):
    r = torch.zeros_like(t, dtype=torch.bool)
    r[sl] = True
    return r


def _words(bits, rng, nb32, ldm):
    """caller-supplied mask words [S][nb32 + 1][ldm][2] that carry `bits` [S][rows][N] where an element lives and junk elsewhere"""
    S, rows, N = bits.shape
    out = np.zeros((S, nb32 + 1, ldm, 2), dtype=np.uint16)
    own = mask_encode(np.ones((rows, N), bool), ldm)
    for s in range(S):
        junk = mask_encode(rng.random((nb32 * 32, ldm)) < 0.5, ldm)
        out[s, :nb32] = (junk & ~own) | mask_encode(bits[s], ldm)
        out[s, nb32] = 0xA5A5
    return out.view(np.int16)


def run_chain(c):
    E = _E()
    variant, rows, S, br, M = c["variant"], c["rows"], c["nseg"], c["block_rows"], c["models"]
    has_fwd, has_dx = variant != GB, variant != GF
    label = "chain " + case_id(c)
    nrb, nb32, srows = -(-rows // br), -(-rows // 32), rows + GAP
    w = WIDTHS[c["widths"]]
    feat, fvalid = w[3]
    inp = chain_inputs(c)
    rng = inp["rng"]
    ar = Arena(8 << 20, M)
    bf, f32, i16 = torch.bfloat16, torch.float32, torch.int16
    worst, shares = [0.0], []

    def close(tag, got, ref, bound):
        worst[0] = max(worst[0], _close(tag, got, ref, bound))

    def op_bufs(K, N, with_cs, in_words=None):
        ldo, ldm, ldcs = N + 8, N + 16, N + 8
        o = dict(K=K, N=N, ldo=ldo, ldm=ldm, ldcs=ldcs, out_t=ar.alloc((S, srows, ldo), bf, SENT),
                 mask_t=ar.alloc((S, nb32 + 1, ldm, 2), i16, MASK_SENT if in_words is None else in_words), words_in=in_words)
        o["kw"] = dict(K=K, N=N, out=o["out_t"][0], out_bs=srows * ldo, ldo=ldo, mask=o["mask_t"][0], mask_bs=(nb32 + 1) * ldm * 2, ldm=ldm)
        if with_cs:
            o["cs_t"] = ar.alloc((S * nrb + 1, ldcs), f32, SENT)
            o["kw"].update(cs=o["cs_t"][0], ldcs=ldcs)
        return o

    kw = dict(variant=variant, rows=rows, nseg=S, block_rows=br, models=M, model_stride=ar.stride if M > 1 else 0, seg0=0, seed=SEED,
              row0=c["row0"], gauss=c["gauss"], iter=ITER, batch=2 if c["stream"] else 0)
    fops, dops = [], []
    if has_fwd:
        K0 = w[0][0]
        lda = K0 + 8
        abuf = np.full((M, S, srows, lda), np.nan)
        abuf[:, :, :rows, :K0] = inp["a0"]
        a_t = ar.alloc((S, srows, lda), bf, abuf)
        kw.update(a=a_t[0], a_bs=srows * lda, lda=lda, a_cols=K0)
        for i, (K, N, nv) in enumerate(fwd_specs(c)):
            o = op_bufs(K, N, c["cs"] and variant == GF and i == 2)
            o["W_t"] = ar.alloc((N, K), bf, inp["Wf"][i])
            o["b_t"] = ar.alloc((N,), f32, inp["bf"][i])
            o["kw"].update(n_valid=nv, W=o["W_t"][0], bias=o["b_t"][0], sigma=SIGMA[i], site=3 + i)
            fops.append(o)
    if has_dx:
        for i, (K, N, nv) in enumerate(dx_specs(c)):
            own = variant == GB or i == 2                   # whose words this product follows: the caller's, or a forward product's
            words = np.stack([_words(inp["dxbits"][i][m], rng, nb32, N + 16) for m in range(M)])
            o = op_bufs(K, N, c["cs"], words)
            o["own"] = own
            o["W_t"] = ar.alloc((N, K), bf, inp["Wd"][i])
            o["kw"].update(n_valid=nv, W=o["W_t"][0])
            dops.append(o)
    head = fm = None
    if variant == DT:
        kinds = (R.LAB, R.UNL, R.FAKE)[:S] if S > 1 else (R.LAB,)
        ldd, off_db = feat + 16, feat * KP + 4
        off_dbf = off_db + KP + 4
        pstride = off_dbf + feat + 4
        w6_t, b6_t = ar.alloc((feat, KP), f32, inp["W6"]), ar.alloc((KP,), f32, inp["b6"])
        hd_t, part_t, lp_t = ar.alloc((S, srows, ldd), bf, SENT), ar.alloc((S * nrb + 1, pstride), f32, SENT), ar.alloc((S * nrb + 1, 4), f32, SENT)
        labels_t = torch.from_numpy(inp["labels"]).to(DEV)
        inv, w_unl = 1.0 / rows, 0.75
        head = dict(rows=rows, nseg=S, seg_kind=list(kinds), feat=feat, feat_valid=fvalid, classes=6, w=w6_t[0], ldw=KP, b=b6_t[0], labels=labels_t,
                    labels_stream=1 if c["stream"] else 0, inv_count=inv, unl_weight=w_unl, dpre=hd_t[0], dpre_bs=srows * ldd, ldd=ldd,
                    part=part_t[0], part_stride=pstride, off_db=off_db, off_dbf=off_dbf, loss_part=lp_t[0], models=M,
                    model_stride=ar.stride if M > 1 else 0, labels_ms=3 * rows)
    if variant == GB:
        npf, npr = c["npf"], c["npr"]
        ldcs, ldf, ldd = feat + 8, feat + 8, feat + 16
        count, gs = float(rows), 0.5
        splits = [[_split(rng, rows * rng.uniform(0, 1, feat), n) for n in (npf, npr)] for _ in range(M)]
        csb = np.full((M, npf + npr + 1, ldcs), np.nan, dtype=np.float32)
        for m in range(M):
            csb[m, :npf, :feat], csb[m, npf:npf + npr, :feat] = splits[m][0][0], splits[m][1][0]
        fbuf = np.full((M, srows, ldf), np.nan)
        fbuf[:, :rows, :feat] = inp["fm_feat"]
        cs_t, ff_t = ar.alloc((npf + npr + 1, ldcs), f32, csb), ar.alloc((srows, ldf), bf, fbuf)
        fd_t, scal_t = ar.alloc((srows, ldd), bf, SENT), ar.alloc((4,), f32, np.tile(np.array([SENT, 3.25, SENT, SENT]), (M, 1)))
        fm = dict(cs=cs_t[0], npart_fake=npf, npart_real=npr, ldcs=ldcs, count=count, grad_scale=gs, feat=feat, feat_valid=fvalid, dpre=fd_t[0], ldd=ldd,
                  loss_out=scal_t[0][0:], accum=scal_t[0][1:])
        kw.update(fm_feat=ff_t[0], fm_ldf=ldf)

    rc, name = E.debug_chain(fwd=[o["kw"] for o in fops], dx=[o["kw"] for o in dops], head=head, fm=fm, **kw)
    assert rc == 0, (label, rc, E.load_library().mrgan_last_error())
    assert name == kernel_name(c), (label, name)
    SEEN[case_id(c)] = name
    ar.check_gaps(label)

    def check_out(tag, o, m, ref, bound, nv):
        got = _np(o["out_t"][m])
        N = o["N"]
        assert not (got[:, :rows, :N] == SENT).any(), tag + ": output elements inside [rows][N] were not written"
        close(tag + " out", got[:, :rows, :N], ref, bound + BF16_RND * (np.abs(ref) + bound))
        assert (got[:, :rows, nv:N] == 0).all(), tag + ": columns [n_valid, N) must be exact zeros"
        _assert_sentinel(tag + " out", o["out_t"][m].float(), _inside(o["out_t"][m], slice(None), slice(0, rows), slice(0, N)))
        return got[:, :rows, :N]

    def check_cs(tag, o, m, v, vb):
        """column sums of v [S][rows][N] (bounds vb) per (segment, row block) of br rows"""
        if "cs_t" not in o:
            return
        N = o["N"]
        wr = min(256 * -(-N // 256), o["ldcs"])
        got = _np(o["cs_t"][m])
        blk = lambda x: np.concatenate([_blocks(x[s], nrb, br) for s in range(S)])
        close(tag + " cs", got[:S * nrb, :N], blk(v), blk(vb) + br * U * blk(np.abs(v)))
        assert (got[:S * nrb, N:wr] == 0).all(), tag + ": column sums beyond N must be exact zeros"
        _assert_sentinel(tag + " cs", o["cs_t"][m], _inside(o["cs_t"][m], slice(0, S * nrb), slice(0, wr)))

    for m in range(M):
        mtag = "%s m%d" % (label, m)
        fbits = []
        x = inp["a0"][m] if has_fwd else None
        # ---- forward products ----
        for i, o in enumerate(fops):
            tag = "%s fwd%d" % (mtag, i)
            K, N, nv = fwd_specs(c)[i]
            pre, accb, v, ref, bound = fwd_reference(c, m, i, x, inp["Wf"][i][m], inp["bf"][i][m])
            x = check_out(tag, o, m, ref, bound, nv)
            words = _np(o["mask_t"][m])
            bits = np.stack([mask_decode(words[s], rows, N) for s in range(S)])
            und = np.abs(pre) <= accb
            und[..., nv:] = False                          # padding columns: pre-activation exactly 0, bit exactly 0
            share = und[..., :nv].mean()
            shares.append(share)
            assert share <= MASK_CAP, (tag, share)
            wrong = (bits != (pre > 0)) & ~und
            assert not wrong.any(), "%s: %d mask bits differ, first at %s" % (tag, wrong.sum(), tuple(np.argwhere(wrong)[0]))
            keep = np.ones(words.shape, bool)
            keep[:, :nb32, :N, :] = False
            assert (words[keep] == MASK_SENT).all(), tag + ": mask words outside [ceil(rows / 32)][N] were written"
            fbits.append(bits)
            check_cs(tag, o, m, v, accb)
        # ---- loss head ----
        if variant == DT:
            W64, b64 = inp["W6"][m].astype(np.float64), inp["b6"][m].astype(np.float64)
            Wv = W64[:, :6].copy()
            Wv[fvalid:] = 0.0
            y = inp["labels"][m, 2 if c["stream"] else 0].astype(np.int64)
            got_dpre, got_part, got_lp = _np(hd_t[m]), _np(part_t[m]), _np(lp_t[m])
            c1, c2 = inp["c1"], inp["c2"]
            for s, kind in enumerate(kinds):
                tag = "%s head seg%d" % (mtag, s)
                fs, live = x[s], fbits[2][s]
                l = fs @ Wv + b64[:6]
                l[:, c2] = l[:, c1]
                delta = _head_delta(BF16, KP, feat, True) * (np.abs(fs) @ np.abs(Wv) + np.abs(b64[:6]))
                loss0, loss1, err, dl = R.head_rows(l, kind, y, inv, w_unl)
                e0, e1, e_dl = _head_row_bounds(kind, l, delta, y, inv, w_unl, KP)
                e_dl = e_dl + 2.0 ** -133                   # dlogits travel as three bf16 addends: the last one may underflow
                lp = got_lp[s * nrb:(s + 1) * nrb]
                close(tag + " loss0", lp[:, 0], _blocks(loss0, nrb, 64), _blocks(e0, nrb, 64) + 64 * U * _blocks(np.abs(loss0), nrb, 64))
                close(tag + " loss1", lp[:, 1], _blocks(loss1, nrb, 64), _blocks(e1, nrb, 64) + 64 * U * _blocks(np.abs(loss1), nrb, 64))
                assert (lp[:, 3] == 0).all()
                if kind == R.LAB:
                    und = _head_undecided(l, delta, c2)
                    lo, hi = _blocks(err * ~und, nrb, 64), _blocks(err * ~und + und, nrb, 64)
                    assert ((lp[:, 2] >= lo) & (lp[:, 2] <= hi)).all(), (tag, lp[:, 2], lo, hi)
                else:
                    assert (lp[:, 2] == 0).all()
                _, _, dp, _ = R.head_backward(fs, Wv, dl, live=live)
                gb = _head_grad_bounds(fs, Wv, dl, e_dl, dp, live, BF16, KP, 64, nrb, True)
                close(tag + " dpre", got_dpre[s, :rows, :feat], dp, gb["dpre"])
                assert (got_dpre[s, rows:] == SENT).all() and (got_dpre[s, :rows, feat:] == SENT).all(), tag + ": dpre written outside [rows][feat]"
                pr = got_part[s * nrb:(s + 1) * nrb]
                gw = pr[:, :feat * KP].reshape(nrb, feat, KP)
                close(tag + " dW6", gw[:, :, :6], gb["dw_ref"], gb["dw"])
                assert (gw[:, :, 6:] == 0).all(), tag + ": dW6 columns >= classes must be exact zeros"
                close(tag + " db6", pr[:, off_db:off_db + 6], _blocks(dl, nrb, 64), gb["db6"])
                assert (pr[:, off_db + 6:off_db + KP] == 0).all()
                close(tag + " dbf", pr[:, off_dbf:off_dbf + feat], _blocks(dp, nrb, 64), gb["dbf"])
                for a0, a1 in ((feat * KP, off_db), (off_db + KP, off_dbf), (off_dbf + feat, pstride)):
                    assert (pr[:, a0:a1] == SENT).all(), tag + ": part row written outside dW6 / db6 / dbf"
            assert (got_part[S * nrb] == SENT).all() and (got_lp[S * nrb] == SENT).all(), mtag + ": a partial row beyond the blocks was written"
            x = got_dpre[:, :rows, :feat]
        # ---- feature-matching gradient ----
        if variant == GB:
            (pf, tf, af), (pr_, tr, ar_) = splits[m]
            fv = slice(0, fvalid)
            loss, gj, _, e_gj, e_loss = _fm_bounds(tf[fv], tr[fv], af[fv], ar_[fv], npf, npr, count, gs)
            live = inp["fm_feat"][m] > 0
            ref, bound = np.zeros((rows, feat)), np.zeros((rows, feat))
            ref[:, fv] = np.where(live[:, fv], gj[None, :], 0.0)
            bound[:, fv] = np.where(live[:, fv], e_gj[None, :], 0.0)
            got = _np(fd_t[m])
            close(mtag + " fm dpre", got[:rows, :feat], ref, bound + BF16_RND * (np.abs(ref) + bound))
            _assert_sentinel(mtag + " fm dpre", fd_t[m].float(), _inside(fd_t[m], slice(0, rows), slice(0, feat)))
            sc = _np(scal_t[m])
            close(mtag + " fm loss", sc[0:1], [loss], [e_loss])
            close(mtag + " fm accum", sc[1:2], [3.25 + loss], [e_loss + U * (3.25 + loss)])
            assert sc[2] == SENT and sc[3] == SENT
            x = np.broadcast_to(got[None, :rows, :feat], (S, rows, feat))
        # ---- dX products ----
        for i, o in enumerate(dops):
            tag = "%s dx%d" % (mtag, i)
            K, N, nv = dx_specs(c)[i]
            W = inp["Wd"][i][m]
            assert np.array_equal(_np(o["mask_t"][m]), o["words_in"][m].view(np.uint16)), tag + ": a dX mask is read only"
            bits = inp["dxbits"][i][m] if o["own"] else fbits[1 - i]      # (D tail: dx[0] follows fwd[1]'s words, dx[1] fwd[0]'s)
            acc = x @ W.T
            accb = 2 * K * U * (np.abs(x) @ np.abs(W).T)
            v, vb = np.where(bits, acc, 0.0), np.where(bits, accb, 0.0)
            x = check_out(tag, o, m, v, vb, nv)
            check_cs(tag, o, m, v, vb)
    share = max(shares) if shares else 0.0
    print("%s [%s]: largest usage %.3f, largest undecided mask share %.5f %%" % (label, name, worst[0], 100 * share))
    assert worst[0] <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_chain(case):
    run_chain(case)


@pytest.mark.gpu
def test_every_instantiation_ran():
    """the parametrisation names all 16 instantiations (every launch asserts its reported name against this prediction), and
    when the whole module ran, the reported names are those 16"""
    assert sorted(set(kernel_name(c) for c in CASES)) == ALL_KERNELS and len(ALL_KERNELS) == 16
    if len(SEEN) == len(CASES):
        assert sorted(set(SEEN.values())) == ALL_KERNELS


def test_case_list_covers_what_it_must():
    """each width set, rows 130 and rows 50 in each variant, at both block sizes where the variant has both; the head's and fm's
    special cases"""
    for v in (DT, GF, GB):
        mine = [c for c in CASES if c["variant"] == v]
        assert set(c["widths"] for c in mine) == set(WIDTHS)
        for br in ((64,) if v == DT else (64, 32)):
            assert {50, 130} <= set(c["rows"] for c in mine if c["block_rows"] == br), (v, br)
    assert any(c["rows"] == 64 for c in CASES) and set(c["nseg"] for c in CASES) == {1, 2, 3} and set(c["models"] for c in CASES) == {1, 3}
    assert any(c["variant"] == DT and c["stream"] for c in CASES) and any(c["variant"] == DT and c["nseg"] == 3 for c in CASES)
    gb = [c for c in CASES if c["variant"] == GB]
    assert any(c["npf"] != c["npr"] and max(c["npf"], c["npr"]) > 64 for c in gb) and any(c["npf"] == 1 and c["npr"] == 1 for c in gb)
    assert any(c["cs"] for c in CASES if c["variant"] == GF) and any(not c["cs"] for c in CASES if c["variant"] == GF)
    assert any(c["row0"] for c in CASES) and all(c["row0"] % 2 == 0 for c in CASES)
    assert 30 <= len(CASES) <= 40 and len(set(case_id(c) for c in CASES)) == len(CASES)
