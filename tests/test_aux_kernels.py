"""Kernel-level parity of the non-GEMM kernels (csrc/aux_kernels.hip, csrc/head_wide.hip) against the fp64 restatements of tests/aux_refs.py (tied to
the oracle by tests/test_aux_refs_cpu.py), one launch per case through the mrgan_debug_* entries of the launchers: caller-owned
buffers with leading dimensions wider than the logical widths and gap rows between segments and models, outputs filled with
SENT (bytes 0x7F, masks their own words), every element outside the documented written region asserted untouched.

Inputs are drawn once with _rng and rounded to the kernel's storage type before both sides read them; partial-sum rows are
random splits of a total, and the reference takes the fp64 sum of the fp32 rows as its input, so only the total matters.
Every case prints its largest err / bound ("usage").

Tolerances are forward-error bounds of the written formulas ("Kernel-level tolerance of the non-GEMM kernels"),
U = 2^-24:
    a fold of n fp32 terms in any order            n U sum |term|
    each further fp32 operation                    U |value|
    bf16 stores                                    2^-8 |value|
    1 - exp(-h) (expm1f)                           SIGMOID_ABS of test_gemm_kernels.py
    expf / logf chains of the loss head            SOFTPLUS_ABS + SOFTPLUS_REL |value| of test_gemm_kernels.py
BatchNorm: mean = S1 / n carries e_mean = npart U sum |part| / n + U |mean|; var = S2 / n - mean^2 carries the same for S2,
2 |mean| e_mean and the cancellation term U (E[x^2] + 2 mean^2); rstd = (var + eps)^-1/2 carries rstd^3 / 2 times that + 3 U rstd.
Adam (Keras 2.0.9, eps outside the root), with e_g = nslab U sum |g_slab| the error of the gradient sum:
    m' = b1 m + (1 - b1) g                         (1 - b1) e_g + 3 U (|b1 m| + |(1 - b1) g|)
    v' = b2 v + (1 - b2) g^2                       (1 - b2) (2 |g| e_g + e_g^2) + 4 U (b2 v + (1 - b2) g^2)
    den = sqrt(v') + eps                           min(e_v / (2 sqrt v'), sqrt e_v) + 2 U den
    p' = p - lr_t m' / den                         lr_t (e_m / den + |m'| e_den / den^2) + 4 U |lr_t m' / den| + U (|p| + |lr_t m' / den|)
(1 - b1 and 1 - b2 are exact in fp32 for b >= 0.5; lr_t is the fp32 value both sides read.)  The weight copies are checked
exactly against the kernel's own fp32 p.
Written regions beyond the logical ones (asserted with their values): bn_apply / bn_bwd / fm work on all `ld` / `feat` padded
columns and write zeros in the columns beyond the logical width; the transposed weight copies of Adam are written in groups
of 16 rows, zeros beyond the tile's rows.
"""
import numpy as np
import pytest
import torch

from tests import aux_refs as R
from tests.helpers import DEV, SENT, _assert_close, _assert_sentinel, _rng, mask_encode

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
U = 2.0 ** -24
BF16_RND = 2.0 ** -8
SOFTPLUS_ABS, SOFTPLUS_REL = 2.0 ** -20, 2.0 ** -22     # derived in test_gemm_kernels.py
SIGMOID_ABS = 2.0 ** -21
UF = 2.0 ** -149                 # gradual underflow: an fp32 result near zero is off by up to half this spacing, whatever its size
FLUSH = 2.0 ** -126              # expf may return zero for a result below the smallest normal number
GAP = 3                          # spare rows between segments / behind the last row
BYTE_SENT = 0x7F                 # NaN in e4m3 and e5m2: the saturating packers cannot emit it
TDT = {F32: torch.float32, BF16: torch.bfloat16}


def _E():
    from mr_gan_amd import engine as E
    return E


def _ok(rc):
    assert rc == 0, (rc, _E().load_library().mrgan_last_error())


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _close(label, got, ref, bound):
    """got: tensor or array, compared on the host in fp64"""
    got = got.detach().to("cpu", torch.float64) if isinstance(got, torch.Tensor) else _t64(got)
    return _assert_close(label, got, _t64(ref), _t64(bound))


def _round_to(x, dtype):
    """fp64 array -> the values the storage type holds, as fp64"""
    return torch.from_numpy(np.asarray(x, np.float64)).to(TDT[dtype]).to(torch.float64).numpy()


def _split(rng, total, npart):
    """[n] totals -> fp32 partial rows [npart][n] of mixed sign that sum to about `total`, and their exact fp64 sum.
    The Gaussian weights make sum |part| many times |total| (the engine's partial sums of h^2 or of one-signed features do not
    cancel like this), so the fold term n U sum |part| of the BatchNorm and feature-matching bounds is wider here than in
    production: the price of partial rows whose order and grouping cannot hide behind equal magnitudes."""
    w = rng.standard_normal((npart, total.size)) + 1.0 / npart
    w += (1.0 - w.sum(axis=0)) / npart
    parts = (w * total[None, :]).astype(np.float32)
    return parts, parts.astype(np.float64).sum(axis=0), np.abs(parts.astype(np.float64)).sum(axis=0)


def _embed_rows(parts, rows, ld, fill=np.nan):
    """[r][n] -> float32 [rows][ld] with `fill` elsewhere"""
    out = np.full((rows, ld), fill, dtype=np.float32)
    out[:parts.shape[0], :parts.shape[1]] = parts
    return out


# =====================================================================================================================
# stage: gather rows of the fp32 matrix, add sigma * noise, convert, zero the padding columns
#   Irwin-Hall: out = fma(sigs, n, x) with n the exact integer sum and sigs = fp32(sigma) * fp32(NOISE_SCALE) rounded once, which
#   the reference restates: one rounding, U |ref|.  bf16 adds 2^-8 |ref|.  True Gaussian: the per-variate bound of
#   test_gaussian_noise_gpu.py (A + B |n|) times sigma, and the fma's U |ref|.  sigma = 0: a pure convert, bit-exact.
# Written: out[r][0 .. cols_pad) for r < rows of every model, zeros in [cols, cols_pad).
# =====================================================================================================================
GAUSS_A, GAUSS_B = 4 * 1.79e-7, 4 * 2.26e-7          # measured and derived in test_gaussian_noise_gpu.py
STAGE_SEED = 0x5EED5EED0BADF00D


def _stage_seg(rows, cols, ld, cols_pad, sigma=0.5, site=1, seg=0, idx=False, stream=False, gen=False, iter_off=0, src_off=0, shared=False):
    return dict(rows=rows, cols=cols, ld=ld, cols_pad=cols_pad, sigma=sigma, site=site, seg=seg, idx=idx, stream=stream, gen=gen,
                iter_off=iter_off, src_off=src_off, shared=shared)


STAGE_CASES = {
    # ragged 32-row wave with the vector path (cols 16 / ld 16); ragged 128-row block on the scalar path (ld 21, the source one
    # float off a 16-byte boundary) with repeated and descending row indices
    "two": (dict(row0=0, it=0, batch=0, models=1),
            [_stage_seg(50, 16, 16, 16, sigma=0.3), _stage_seg(129, 20, 21, 24, idx=True, src_off=1, site=2, seg=1)]),
    # five segments of different shapes (early-return blocks): ragged 8-group with zero fill, stream rows of batch 2, device-drawn
    # z with a later sub-step's key, a pure convert; first global row 64
    "five": (dict(row0=64, it=7, batch=2, models=1),
             [_stage_seg(50, 16, 16, 16, sigma=0.3), _stage_seg(129, 250, 252, 256, stream=True, site=3, seg=2),
              _stage_seg(40, 20, 21, 24, idx=True, stream=True, site=0, seg=1), _stage_seg(70, 100, 0, 104, gen=True, site=16, iter_off=1),
              _stage_seg(33, 40, 40, 40, sigma=0.0)]),
    # model groups: every model gathers from one matrix through its own indices (src_ms = 0), or reads its own matrix
    "models": (dict(row0=0, it=3, batch=0, models=3),
               [_stage_seg(50, 20, 24, 24, idx=True, shared=True), _stage_seg(129, 16, 16, 16, sigma=0.3, site=2, seg=1)]),
}


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("gauss", [0, 1])
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_stage(dtype, gauss, case):
    from oracle import mrgan_oracle as O
    from tests import gaussian_noise as G
    E = _E()
    launch, segs = STAGE_CASES[case]
    row0, it, batch, models = launch["row0"], launch["it"], launch["batch"], launch["models"]
    tdt, es = TDT[dtype], 2 if dtype == BF16 else 4
    rng = _rng(21, dtype, gauss, len(segs), models)
    label = "stage %s %s %s" % ("bf16" if dtype else "f32", "gauss" if gauss else "irwin-hall", case)
    descs, keep = [], []
    for sp in segs:
        rows, cols, ld, cols_pad = sp["rows"], sp["cols"], sp["ld"], sp["cols_pad"]
        nsrc = (batch + 1) * rows + 5
        ldo = cols_pad + 8
        out = torch.full((models, rows + GAP, ldo), SENT, dtype=tdt, device=DEV)
        d = dict(rows=rows, cols=cols, cols_pad=cols_pad, ld=ld, out=out, ldo=ldo, sigma=sp["sigma"], site=sp["site"], seg=sp["seg"],
                 gen=1 if sp["gen"] else 0, stream=1 if sp["stream"] else 0, iter_off=sp["iter_off"], models=models,
                 out_ms=(rows + GAP) * ldo * es)
        src = idx = None
        if not sp["gen"]:
            nmat = 1 if sp["shared"] else models
            src = rng.standard_normal((nmat, nsrc, ld)).astype(np.float32)
            src[:, :, cols:] = np.nan                      # the pitch's spare columns are never read
            flat = torch.full((nmat * nsrc * ld + 8,), float("nan"), dtype=torch.float32, device=DEV)
            flat[sp["src_off"]:sp["src_off"] + src.size] = _dev(src).reshape(-1)
            d.update(src=flat[sp["src_off"]:], src_ms=0 if sp["shared"] else nsrc * ld)
            keep.append(flat)
            if sp["idx"]:
                n = (batch + 1) * rows
                idx = np.stack([(nsrc - 1 - ((np.arange(n) * (m + 2)) % 37)) for m in range(models)]).astype(np.int32)   # descending, repeated
                d.update(idx=_dev(idx, torch.int32), idx_ms=n)
        descs.append(d)
        sp["_t"] = (out, src, idx)
    _ok(E.debug_stage(descs, dtype=dtype, seed=STAGE_SEED, row0=row0, iter=it, batch=batch, gauss=gauss))
    worst = 0.0
    for sp in segs:
        rows, cols, cols_pad = sp["rows"], sp["cols"], sp["cols_pad"]
        out, src, idx = sp["_t"]
        noisy = sp["gen"] or sp["sigma"] > 0
        sig = np.float32(1.0 if sp["gen"] else sp["sigma"])
        for m in range(models):
            x = np.zeros((rows, cols))
            if not sp["gen"]:
                o = batch * rows if sp["stream"] else 0
                r = idx[m, o:o + rows] if idx is not None else np.arange(o, o + rows)
                x = src[0 if sp["shared"] else m][r, :cols].astype(np.float64)
            tag = "%s seg %dx%d m%d" % (label, rows, cols, m)
            got = out[m, :rows, :cols]
            if not noisy:
                assert torch.equal(got.cpu(), torch.from_numpy(x).to(tdt)), tag + ": sigma = 0 must be a pure convert"
            else:
                step = it + sp["iter_off"]
                if gauss:
                    n = G.gaussian_normal(STAGE_SEED + m, sp["site"], sp["seg"], step, rows, cols, row0=row0)
                    ref = x + float(sig) * n
                    bound = float(sig) * (GAUSS_A + GAUSS_B * np.abs(n)) + U * np.abs(ref)
                else:
                    sigs = float(sig * np.float32(O.NOISE_SCALE))
                    n = O.device_noise_sums(STAGE_SEED + m, sp["site"], sp["seg"], step, rows, cols, row0).astype(np.float64)
                    ref = x + sigs * n
                    bound = U * np.abs(ref)
                if dtype == BF16:
                    bound = bound + BF16_RND * (np.abs(ref) + bound)
                worst = max(worst, _close(tag, got, ref, bound))
            assert bool((out[m, :rows, cols:cols_pad] == 0).all()), tag + ": the padding columns must be exact zeros"
        inside = torch.zeros_like(out, dtype=torch.bool)
        inside[:, :rows, :cols_pad] = True
        _assert_sentinel(label, out.float(), inside)
    print("%s: largest usage %.3f" % (label, worst))


def test_stage_refusals():
    E = _E()
    src = torch.zeros((64, 16), dtype=torch.float32, device=DEV)
    out = torch.zeros((3, 40, 24), dtype=torch.float32, device=DEV)
    seg = dict(src=src, ld=16, rows=40, cols=16, cols_pad=16, out=out, ldo=24, sigma=0.5, site=1, seg=0)
    kw = dict(dtype=F32, seed=1, row0=0, iter=0, batch=0, gauss=0)
    assert E.debug_stage([seg], **kw) == 0
    assert E.debug_stage([dict(seg, ldo=20)], **kw) == -1                 # 16-byte stores
    assert E.debug_stage([dict(seg, cols_pad=12)], **kw) == -1            # cols_pad below cols
    assert E.debug_stage([seg], **dict(kw, gauss=1, row0=1)) == -1        # a row pair split
    assert E.debug_stage([dict(seg, models=3, out_ms=40 * 24 * 4), dict(seg, models=1)], **kw) == -3      # every segment once per model


# =====================================================================================================================
# reduce_partials, colsum_finalize
# =====================================================================================================================
def test_reduce_partials_every_tail_and_model_stride():
    E = _E()
    n, stride, models = 300, 300 + 20, 2
    worst = 0.0
    for nsrc in (1, 5, 8, 13):
        for ngroups in (1, 3, 8):
            rng = _rng(11, nsrc, ngroups)
            rows = nsrc + ngroups + 1                      # per model: the partial rows, the result rows, one spare row
            src = rng.standard_normal((models, nsrc, stride)).astype(np.float32)
            buf = torch.full((models, rows, stride), SENT, dtype=torch.float32, device=DEV)
            buf[:, :nsrc] = _dev(src)
            _ok(E.debug_reduce_partials(buf[0, 0], nsrc, stride, n, ngroups, buf[0, nsrc], models, rows * stride * 4))
            s64 = src.astype(np.float64)
            ref = np.zeros((models, ngroups, n))
            mag = np.zeros((models, ngroups, n))
            for p in range(nsrc):
                ref[:, p % ngroups] += s64[:, p, :n]
                mag[:, p % ngroups] += np.abs(s64[:, p, :n])
            nterms = -(-nsrc // ngroups)
            worst = max(worst, _close("reduce_partials nsrc %d ngroups %d" % (nsrc, ngroups), buf[:, nsrc:nsrc + ngroups, :n], ref, nterms * U * mag))
            assert torch.equal(buf[:, :nsrc].cpu(), torch.from_numpy(src)), "reduce_partials changed its source"
            inside = torch.zeros_like(buf, dtype=torch.bool)
            inside[:, :nsrc] = True
            inside[:, nsrc:nsrc + ngroups, :n] = True
            _assert_sentinel("reduce_partials", buf, inside)
    print("reduce_partials: largest usage %.3f" % worst)
    assert E.debug_reduce_partials(buf[0, 0], 4, n - 1, n, 2, buf[0, 4]) == -1


@pytest.mark.parametrize("n,ld,npart", [(68, 72, 17), (256, 320, 33), (68, 68, 2)])
def test_colsum_finalize(n, ld, npart):
    E = _E()
    nseg = 2
    rng = _rng(12, n, ld, npart)
    p1 = rng.standard_normal((nseg * npart, ld)).astype(np.float32)
    p2 = rng.standard_normal((nseg * npart, ld)).astype(np.float32)
    p1[:, n:] = np.nan
    p2[:, n:] = np.nan
    out = torch.full((nseg * 2 * n + 16,), SENT, dtype=torch.float32, device=DEV)
    _ok(E.debug_colsum_finalize(_dev(p1), _dev(p2), npart, ld, n, out, nseg))
    ref = np.stack([np.stack([p.astype(np.float64).reshape(nseg, npart, ld)[s, :, :n].sum(axis=0) for p in (p1, p2)]) for s in range(nseg)])
    mag = np.stack([np.stack([np.abs(p.astype(np.float64)).reshape(nseg, npart, ld)[s, :, :n].sum(axis=0) for p in (p1, p2)]) for s in range(nseg)])
    _close("colsum_finalize n %d npart %d" % (n, npart), out[:nseg * 2 * n].reshape(nseg, 2, n), ref, npart * U * mag)
    assert bool((out[nseg * 2 * n:] == SENT).all())
    # the launcher's refusal of n % 4, and the entry's of a pitch the 16-byte loads cannot take
    assert E.debug_colsum_finalize(_dev(p1), _dev(p2), npart, ld, n - 2, out, nseg) == -3
    assert E.debug_colsum_finalize(_dev(p1), _dev(p2), npart, n - 4, n, out, nseg) == -1


# =====================================================================================================================
# BatchNorm forward / backward
# =====================================================================================================================
BN_CASES = [(1, 40, 64, 50, 1), (2, 250, 256, 130, 1), (16, 40, 64, 130, 3), (17, 250, 256, 50, 1), (33, 40, 64, 50, 3),
            (49, 250, 256, 130, 1)]
CONST_COL, CONST_VAL = 3, 1.5


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("npart,cols,ld,rows,nseg", BN_CASES)
def test_bn_apply(dtype, npart, cols, ld, rows, nseg):
    E = _E()
    rng = _rng(13, dtype, npart, cols, rows, nseg)
    label = "bn_apply %s npart %d cols %d rows %d nseg %d" % ("bf16" if dtype else "f32", npart, cols, rows, nseg)
    eps32 = np.float32(2e-5)
    eps = float(eps32)
    seg_rows, ldcs, cs_gap = rows + GAP, ld + 8, 2
    # column means in [-2, 2], variances >= 0.25; the padding columns [cols, ld) hold finite values of the same kind (the kernel
    # computes their statistics too and writes zeros for them)
    mean_c, std_c = rng.uniform(-2, 2, (nseg, 1, ld)), rng.uniform(0.5, 1.5, (nseg, 1, ld))
    h = _round_to(mean_c + std_c * rng.standard_normal((nseg, rows, ld)), dtype)
    h[:, :, CONST_COL] = CONST_VAL
    gamma = rng.uniform(0.5, 1.5, cols).astype(np.float32)
    beta = rng.uniform(-1, 1, cols).astype(np.float32)
    cs_rows = npart + cs_gap
    cs1 = np.full((nseg, cs_rows, ldcs), np.nan, dtype=np.float32)
    cs2 = np.full((nseg, cs_rows, ldcs), np.nan, dtype=np.float32)
    t1, t2, a1, a2 = [np.zeros((nseg, ld)) for _ in range(4)]
    for s in range(nseg):
        p1, t1[s], a1[s] = _split(rng, h[s].sum(axis=0), npart)
        p2, t2[s], a2[s] = _split(rng, (h[s] * h[s]).sum(axis=0), npart)
        # the constant column: partial rows that any fp32 summation adds exactly, the sum of squares a little BELOW n c^2, so
        # E[x^2] - mean^2 < 0 exactly and only the clamp keeps the root real
        w = np.zeros(npart)
        w[:] = np.floor(rows * 64 / npart) / 64
        w[0] += rows - w.sum()
        p1[:, CONST_COL] = (CONST_VAL * w).astype(np.float32)
        p2[:, CONST_COL] = (CONST_VAL * CONST_VAL * w).astype(np.float32)
        p2[0, CONST_COL] -= np.float32(2.0 ** -6)
        for p, t, a in ((p1, t1, a1), (p2, t2, a2)):
            t[s, CONST_COL] = p[:, CONST_COL].astype(np.float64).sum()
            a[s, CONST_COL] = np.abs(p[:, CONST_COL].astype(np.float64)).sum()
        cs1[s, :npart, :ld], cs2[s, :npart, :ld] = p1, p2
    assert t1[0, CONST_COL] == CONST_VAL * rows and t2[0, CONST_COL] < CONST_VAL ** 2 * rows
    hbuf = torch.full((nseg, seg_rows, ld), float("nan"), dtype=TDT[dtype], device=DEV)
    hbuf[:, :rows] = _dev(h, TDT[dtype])
    out = torch.full((nseg, seg_rows, ld), SENT, dtype=TDT[dtype], device=DEV)
    mu = torch.full((nseg + 1, ld), SENT, dtype=torch.float32, device=DEV)
    rstd = torch.full((nseg + 1, ld), SENT, dtype=torch.float32, device=DEV)
    kw = dict(dtype=dtype, h=hbuf, out=out, ld=ld, rows=rows, cols=cols, cs1=_dev(cs1), cs2=_dev(cs2), npart=npart, ldcs=ldcs,
              count=float(rows), eps=eps, gamma=_dev(gamma), beta=_dev(beta), mu=mu, rstd=rstd,
              cs_seg_stride=cs_rows * ldcs, nseg=nseg, seg_rows=seg_rows)
    _ok(E.debug_bn_apply(**kw))
    mean, var, rs = R.bn_stats(t1, t2, rows, eps)
    e2 = t2 / rows
    e_mean = npart * U * a1 / rows + U * np.abs(mean)
    e_var = npart * U * a2 / rows + U * e2 + 2 * np.abs(mean) * e_mean + U * (e2 + 2 * mean * mean)
    e_rstd = 0.5 * rs ** 3 * e_var + 3 * U * rs
    _close(label + " mu", mu[:nseg], mean, e_mean)
    _close(label + " rstd", rstd[:nseg], rs, e_rstd)
    assert bool((mu[nseg] == SENT).all()) and bool((rstd[nseg] == SENT).all())
    # the clamp: the variance of the constant column is exactly zero on both sides
    assert var[0, CONST_COL] == 0.0
    got_r = rstd[:nseg, CONST_COL].cpu().double().numpy()
    assert np.all(mu[:nseg, CONST_COL].cpu().numpy() == CONST_VAL), label + ": the constant column's mean is exact"
    assert np.all(np.abs(got_r - 1.0 / np.sqrt(eps)) <= 3 * U / np.sqrt(eps)), (label, got_r, 1.0 / np.sqrt(eps))
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    hv, mv, rv = h[:, :, :cols], mean[:, None, :cols], rs[:, None, :cols]
    ref = R.bn_apply(hv, mv, rv, g64, b64)
    bound = (np.abs(g64) * rv * e_mean[:, None, :cols] + np.abs(g64 * (hv - mv)) * e_rstd[:, None, :cols]
             + 3 * U * (np.abs(hv) + np.abs(mv)) * np.abs(g64) * rv + U * np.abs(b64) + 2 * U * np.abs(ref))
    if dtype == BF16:
        bound = bound + BF16_RND * (np.abs(ref) + bound)
    _close(label + " out", out[:, :rows, :cols], ref, bound)
    # (the constant column comes out as beta: (h - mean) is exactly zero in the reference)
    assert np.all(ref[:, :, CONST_COL] == b64[CONST_COL])
    assert bool((out[:, :rows, cols:] == 0).all()), label + ": the padding columns must be exact zeros"
    inside = torch.zeros_like(out, dtype=torch.bool)
    inside[:, :rows] = True
    _assert_sentinel(label, out.float(), inside)
    if nseg == 3 and npart == 16:                          # what the launcher takes on trust, refused by the entry
        assert E.debug_bn_apply(**dict(kw, ldcs=ld - 4)) == -1            # partial rows narrower than the columns folded
        assert E.debug_bn_apply(**dict(kw, ld=ld - 4)) == -1              # 16-byte accesses of 8 elements
        assert E.debug_bn_apply(**dict(kw, seg_rows=rows - 1)) == -1      # segments that overlap


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("npart,cols,ld,rows", [c[:4] for c in BN_CASES])
def test_bn_bwd(dtype, npart, cols, ld, rows):
    E = _E()
    rng = _rng(14, dtype, npart, cols, rows)
    label = "bn_bwd %s npart %d cols %d rows %d" % ("bf16" if dtype else "f32", npart, cols, rows)
    ldcs = ld + 8
    # h = softplus(pre) >= 0, with exact zeros and values above 20 (1 - exp(-h) = 1 to fp32)
    h = np.abs(rng.standard_normal((rows, ld))) * 1.5
    h[rng.random((rows, ld)) < 0.05] = 0.0
    h[rng.random((rows, ld)) < 0.05] *= 20.0
    h = _round_to(h, dtype)
    assert (h == 0).any() and (h > 20).any()
    dy = _round_to(rng.standard_normal((rows, ld)), dtype)
    gamma = rng.uniform(0.5, 1.5, ld).astype(np.float32)
    mu = rng.uniform(0.5, 1.5, ld).astype(np.float32)
    rs = rng.uniform(0.5, 2.0, ld).astype(np.float32)
    g64, m64, r64 = [x.astype(np.float64) for x in (gamma, mu, rs)]
    xhat = (h - m64) * r64
    p1, t1, a1 = _split(rng, dy.sum(axis=0), npart)
    p2, t2, a2 = _split(rng, (dy * xhat).sum(axis=0), npart)
    nblk = -(-rows // 64)
    tdt = TDT[dtype]
    # gamma / mu / rstd are read below `cols` only: NaN behind it
    for x in (gamma, mu, rs):
        x[cols:] = np.nan
    dpre = torch.full((rows + GAP, ld), SENT, dtype=tdt, device=DEV)
    dbp = torch.full((nblk + 1, ld), SENT, dtype=torch.float32, device=DEV)
    hb = torch.full((rows + GAP, ld), float("nan"), dtype=tdt, device=DEV)
    db = torch.full((rows + GAP, ld), float("nan"), dtype=tdt, device=DEV)
    hb[:rows], db[:rows] = _dev(h, tdt), _dev(dy, tdt)
    _ok(E.debug_bn_bwd(dtype=dtype, dy=db, h=hb, dpre=dpre, ld=ld, rows=rows, cols=cols, cs1=_dev(_embed_rows(p1, npart + 2, ldcs)),
                       cs2=_dev(_embed_rows(p2, npart + 2, ldcs)), npart=npart, ldcs=ldcs, count=float(rows), gamma=_dev(gamma), mu=_dev(mu),
                       rstd=_dev(rs), db_part=dbp))
    c = slice(0, cols)
    ref, _, _ = R.bn_bwd(dy[:, c], h[:, c], m64[c], r64[c], g64[c], rows, t1[c], t2[c])
    xh = xhat[:, c]
    T1, T2, T3 = rows * np.abs(dy[:, c]), np.abs(t1[c]), np.abs(xh * t2[c])
    e_in = npart * U * a1[c] + np.abs(xh) * npart * U * a2[c] + 3 * U * (T1 + T2) + 6 * U * T3
    cA = g64[c] * r64[c] / rows
    sig = -np.expm1(-h[:, c])
    dh = cA * (rows * dy[:, c] - t1[c] - xh * t2[c])
    e_dh = np.abs(cA) * e_in + 3 * U * np.abs(dh)
    e_o = sig * e_dh + np.abs(dh) * SIGMOID_ABS + U * np.abs(ref)
    bound = e_o + BF16_RND * (np.abs(ref) + e_o) if dtype == BF16 else e_o
    _close(label + " dpre", dpre[:rows, :cols], ref, bound)
    assert bool((dpre[:rows, cols:] == 0).all()), label + ": the padding columns must be exact zeros"
    inside = torch.zeros_like(dpre, dtype=torch.bool)
    inside[:rows] = True
    _assert_sentinel(label + " dpre", dpre.float(), inside)
    # bias-gradient partial rows: the column sums of the kernel's own fp32 values over each 64-row block
    pad = np.zeros((nblk * 64 - rows, cols))
    blk = lambda x: np.concatenate([x, pad]).reshape(nblk, 64, cols).sum(axis=1)
    _close(label + " db_part", dbp[:nblk, :cols], blk(ref), blk(e_o) + 64 * U * blk(np.abs(ref)))
    assert bool((dbp[:nblk, cols:] == 0).all()) and bool((dbp[nblk] == SENT).all())
    if npart == 1 and dtype == BF16:
        assert E.debug_bn_bwd(dtype=dtype, dy=db, h=hb, dpre=dpre, ld=ld - 4, rows=rows, cols=cols, cs1=_dev(p1), cs2=_dev(p2), npart=npart,
                              ldcs=ldcs, count=float(rows), gamma=_dev(gamma), mu=_dev(mu), rstd=_dev(rs), db_part=dbp) == -1


# =====================================================================================================================
# feature matching
# =====================================================================================================================
def _e5m2_neighbour(byte_vals, y):
    """whether each decoded e5m2 value is a nearest grid neighbour of y (ties either way): |dec - y| <= half an e5m2 step at y"""
    ay = np.maximum(np.abs(y), 2.0 ** -14)
    step = 2.0 ** (np.floor(np.log2(ay)) - 2)
    return np.abs(byte_vals - y) <= 0.5 * step


def _fm_bounds(tf, tr, af, ar, npf, npr, count, gs):
    """the valid columns' fp64 totals tf / tr of npf fake and npr real partial rows (af / ar: the sums of their magnitudes) ->
    (loss, gj, e_gj, e_gj_mixed, e_loss).  e_gj: the gradient from two folds, one per stream; e_gj_mixed: from ONE fold that takes
    the rows of both streams in any order (what the loss of every kernel and the gradient inside the chain kernel do)"""
    fvn = tf.size
    loss, gj = R.fm(tf, tr, count, gs)
    diff = (tf - tr) / count
    e_diff = (npf * U * af + npr * U * ar + U * np.abs(tf - tr)) / count + U * np.abs(diff)
    scale = np.abs(gs * 2.0 / (fvn * count))
    # the loss: the mixed fold of fake and real rows (any order), the square, the sum over the features (any order)
    e_d2 = ((npf + npr) * U * (af + ar) / count + U * np.abs(diff))
    e_loss = (np.sum(2 * np.abs(diff) * e_d2 + e_d2 ** 2 + 3 * U * diff * diff) + fvn * U * np.sum(diff * diff)) / fvn + U * loss
    return loss, gj, scale * e_diff + 4 * U * np.abs(gj), scale * e_d2 + 4 * U * np.abs(gj), e_loss


def _run_fm(dtype, feat, feat_valid, rows, npf, npr, q8=False, dist=False, launches=1, key=0):
    E = _E()
    rng = _rng(15, dtype, feat, feat_valid, rows, npf, npr, key)
    tdt = TDT[dtype]
    label = "fm %s feat %d/%d rows %d npart %d+%d%s%s" % ("bf16" if dtype else "f32", feat, feat_valid, rows, npf, npr, " q8" if q8 else "", " dist" if dist else "")
    ldcs, ldm, ldd, ldq = feat + 8, feat + 16, feat + 8, feat + 8
    count, gs = float(rows), 0.5
    pf, tf, af = _split(rng, rows * rng.uniform(0, 1, feat), npf)
    pr, tr, ar = _split(rng, rows * rng.uniform(0, 1, feat), npr)
    cs = np.full((npf + npr + 1, ldcs), np.nan, dtype=np.float32)
    cs[:npf, :feat], cs[npf:npf + npr, :feat] = pf, pr
    bits = rng.random((rows, feat)) < 0.5
    nblk = -(-rows // 32)
    junk = mask_encode(rng.random((nblk * 32, ldm)) < 0.5, ldm)              # set bits where no element lives: they must not matter
    own = mask_encode(np.ones((rows, feat), bool), ldm)
    words = (junk & ~own) | mask_encode(bits, ldm)
    mask = torch.from_numpy(words.view(np.int16)).to(DEV)
    dpre = torch.full((rows + GAP, ldd), SENT, dtype=tdt, device=DEV)
    scal = torch.full((4,), SENT, dtype=torch.float32, device=DEV)          # loss_out, accum, two spare words
    scal[1] = 3.25
    kw = dict(dtype=dtype, cs=_dev(cs), npart_fake=npf, npart_real=npr, ldcs=ldcs, count=count, grad_scale=gs, feat=feat, feat_valid=feat_valid,
              mask=mask, ldm=ldm, dpre=dpre, ldd=ldd, rows=rows, loss_out=scal[0:], accum=scal[1:])
    gx = feat // 64
    if dist:
        lscr = torch.full((gx + 2,), SENT, dtype=torch.float32, device=DEV)
        lcount = torch.zeros(2, dtype=torch.int32, device=DEV)
        lcount[1] = 0x5A5A
        kw.update(lscratch=lscr, lcount=lcount)
    if q8:
        scale = 2.0 ** 12
        q8buf = torch.full((rows + GAP, ldq), BYTE_SENT, dtype=torch.uint8, device=DEV)
        slot = E.fp8_slots([(0.0, scale, 1.0 / scale, 28672.0)])
        kw.update(q8=q8buf, ldq8=ldq, q8_slot=slot)
    for _ in range(launches):
        _ok(E.debug_fm(**kw))
    fv = slice(0, feat_valid)
    loss, gj, e_gj, _, e_loss = _fm_bounds(tf[fv], tr[fv], af[fv], ar[fv], npf, npr, count, gs)
    ref = np.zeros((rows, feat))
    ref[:, fv] = np.where(bits[:, fv], gj[None, :], 0.0)
    bound = np.zeros((rows, feat))
    bound[:, fv] = np.where(bits[:, fv], e_gj[None, :], 0.0)
    if dtype == BF16:
        bound = bound + BF16_RND * (np.abs(ref) + bound)
    use = _close(label + " dpre", dpre[:rows, :feat], ref, bound)
    inside = torch.zeros_like(dpre, dtype=torch.bool)
    inside[:rows, :feat] = True
    _assert_sentinel(label + " dpre", dpre.float(), inside)
    got = scal.cpu().double().numpy()
    _close(label + " loss", got[0:1], [loss], [e_loss])
    _close(label + " accum", got[1:2], [3.25 + launches * loss], [launches * (e_loss + U * (3.25 + launches * loss))])
    assert got[2] == SENT and got[3] == SENT
    res = dict(dpre=dpre.clone(), loss=got[0], e_loss=e_loss, usage=use)
    if dist:
        assert lcount.cpu().tolist() == [0, 0x5A5A], label + ": the ticket counter must be left at zero"
        l = lscr.cpu().numpy()
        assert not (l[:gx] == SENT).any() and l[gx] == SENT and l[gx + 1] == SENT
    if q8:
        qb = q8buf.cpu()
        assert bool((qb[rows:] == BYTE_SENT).all()) and bool((qb[:rows, feat:] == BYTE_SENT).all())
        dec = qb[:rows, :feat].contiguous().view(torch.float8_e5m2).to(torch.float64).numpy()
        mine = dpre[:rows, :feat].cpu().double().numpy() * scale
        if dtype == F32:                                   # packed from the very fp32 values the kernel stored
            want = torch.from_numpy(mine).to(torch.float32).to(torch.float8_e5m2).to(torch.float64).numpy()
            assert np.array_equal(dec, want), label + ": e5m2 copy differs from the pack of the stored fp32 values"
        else:                                              # packed from the fp32 value whose bf16 rounding is stored
            assert _e5m2_neighbour(dec, mine).all(), label + ": e5m2 copy is not a neighbour of the stored value"
        amax_bits, _ = E.fp8_slots_read(slot)
        amax = float(amax_bits.view(np.float32)[0])
        stored_max = float(dpre[:rows, :feat].abs().max())
        assert float(torch.tensor(amax).to(tdt)) == stored_max, (label, amax, stored_max)
    return res


@pytest.mark.parametrize("dtype,q8", [(F32, False), (BF16, False), (BF16, True), (F32, True)])
@pytest.mark.parametrize("feat,feat_valid,rows,npf,npr", [(64, 64, 50, 1, 5), (256, 250, 130, 17, 16), (256, 250, 50, 1, 16), (64, 64, 130, 17, 5)])
def test_fm_narrow(dtype, q8, feat, feat_valid, rows, npf, npr):
    _run_fm(dtype, feat, feat_valid, rows, npf, npr, q8=q8)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows", [96, 2100])
def test_fm_distributed_matches_narrow_form(dtype, rows):
    """feat 1024: 16 column blocks, the loss from the per-block partials by the last block to arrive.  rows 2100: the launcher
    gives every block 96 rows (round_up(ceil(2100 / 32), 32)); a wrong `rb` leaves rows unwritten or writes the gap rows."""
    narrow = _run_fm(dtype, 1024, 1024, rows, 5, 3)
    dist = _run_fm(dtype, 1024, 1024, rows, 5, 3, dist=True)
    assert torch.equal(narrow["dpre"], dist["dpre"]), "the two forms must give the same gradient bit for bit"
    assert abs(narrow["loss"] - dist["loss"]) <= narrow["e_loss"] + dist["e_loss"]
    # a second launch on the same buffers: the counter is at zero again, the accumulator has grown twice
    _run_fm(dtype, 1024, 1000, rows, 5, 3, dist=True, launches=2, key=1)


def test_fm_refusals():
    E = _E()
    cs = torch.zeros((4, 72), dtype=torch.float32, device=DEV)
    mask = torch.zeros((2, 72, 2), dtype=torch.int16, device=DEV)
    dpre = torch.zeros((40, 72), dtype=torch.float32, device=DEV)
    kw = dict(dtype=F32, cs=cs, npart_fake=2, npart_real=2, ldcs=72, count=40.0, grad_scale=1.0, feat=64, feat_valid=64, mask=mask, ldm=72,
              dpre=dpre, ldd=72, rows=40)
    assert E.debug_fm(**kw) == 0
    assert E.debug_fm(**dict(kw, ldd=60)) == -1
    assert E.debug_fm(**dict(kw, ldcs=70)) == -1
    assert E.debug_fm(**dict(kw, feat=60, feat_valid=60)) == -3       # launch_fm: feat % 8


# =====================================================================================================================
# Adam
# =====================================================================================================================
class Arena(object):
    """One byte buffer per launch that holds every tensor of every model, model m `stride` bytes behind model 0 (the kernel's
    model_stride applies to every pointer alike); bytes nobody allocated keep 0xEE."""

    def __init__(self, nbytes, models):
        self.stride = (nbytes + 4096 + 255) // 256 * 256
        self.models = models
        self.buf = torch.full((models * self.stride,), 0xEE, dtype=torch.uint8, device=DEV)
        self.off = 0
        self.taken = torch.zeros(self.stride, dtype=torch.bool)

    def alloc(self, shape, dtype, fill):
        """-> [per-model view]; fill: scalar, or an array [models, *shape]"""
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        off = self.off
        self.off = (off + n + 255) // 256 * 256
        assert self.off <= self.stride - 4096
        self.taken[off:off + n] = True
        views = []
        for m in range(self.models):
            v = self.buf[m * self.stride + off:m * self.stride + off + n].view(dtype).view(*shape)
            if np.isscalar(fill):
                v.fill_(fill)
            else:
                v.copy_(torch.from_numpy(np.ascontiguousarray(fill[m])).to(dtype))
            views.append(v)
        return views

    def check_gaps(self, label):
        b = self.buf.cpu().view(self.models, self.stride)
        assert bool((b[:, ~self.taken] == 0xEE).all()), label + ": bytes outside every tensor were written"


# rows, cols, the copies it keeps: w16, wt16, e4m3
ADAM_TILES = [(64, 64, True, True, False), (40, 24, True, True, False), (64, 64, True, True, True), (40, 24, True, True, True),
              (1, 64, False, False, False), (1, 16, True, False, False), (1, 8, False, False, False), (1, 252, False, False, False),
              (3, 20, True, False, False), (2, 64, True, False, False)]          # 2 x 64: 32 groups, the small path at QL = 64
W8_SCALE = 64.0


def _adam_case(nslab, b1, it, models=1, key=0, advance=1, flat16=False):
    """the tile table's tensors in an arena + the launch keywords; one (rows, cols) entry wider than 64 columns becomes several
    tiles of one tensor, as the engine cuts them"""
    rng = _rng(16, nslab, it, models, key)
    ar = Arena(4 << 20, models)
    tens, tiles = [], []
    for rows, cols, w16, wt16, w8 in ADAM_TILES:
        w8 = w8 and models == 1                            # model groups keep no fp8 copies
        ld, ldt, srows = cols + 12, 80, rows + 1
        t = dict(rows=rows, cols=cols, ld=ld, ldt=ldt, nslab=nslab, srows=srows)
        shape = (models, rows, cols)
        mag = 10.0 ** rng.uniform(-10, 0, (models, nslab, rows, cols))
        g = (mag * np.where(rng.random(mag.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
        g[rng.random(g.shape) < 0.1] = 0.0
        t["g0"] = g
        init = dict(p=rng.standard_normal(shape), m=rng.standard_normal(shape) * 1e-2, v=rng.uniform(1e-6, 1e-3, shape))
        for name in ("p", "m", "v"):
            full = np.full((models, srows, ld), SENT, dtype=np.float32)
            full[:, :rows, :cols] = init[name].astype(np.float32)
            t[name + "0"] = full
            t[name] = ar.alloc((srows, ld), torch.float32, full)
        gfull = np.full((models, nslab, srows, ld), np.nan, dtype=np.float32)
        gfull[:, :, :rows, :cols] = g
        t["g"] = ar.alloc((nslab, srows, ld), torch.float32, gfull)
        t["flat"] = ar.alloc((srows, ld), torch.float32, SENT)
        t["flat16"] = ar.alloc((srows, ld), torch.bfloat16, SENT)
        t["w16"] = ar.alloc((srows, ld), torch.bfloat16, SENT) if w16 else None
        t["wt16"] = ar.alloc((cols + 1, ldt), torch.bfloat16, SENT) if wt16 else None
        t["w8"] = ar.alloc((srows, ld), torch.uint8, BYTE_SENT) if w8 else None
        t["w8t"] = ar.alloc((cols + 1, ldt), torch.uint8, BYTE_SENT) if w8 else None
        t["slot"] = _E().fp8_slots([(0.0, W8_SCALE, 1.0 / W8_SCALE, 224.0)]) if w8 else None
        tens.append(t)
        for c0 in range(0, cols, 64):
            d = dict(p=t["p"][0][0, c0:], m=t["m"][0][0, c0:], v=t["v"][0][0, c0:], g=t["g"][0][0, 0, c0:], nslab=nslab, slab_stride=srows * ld,
                     flat=t["flat"][0][0, c0:], ld=ld, ldt=ldt, rows=rows, cols=min(64, cols - c0))
            if flat16:                                     # the kernel then reads and writes flat16 in place of flat
                d["flat16"] = t["flat16"][0][0, c0:]
            for name, field in (("w16", "w16"), ("wt16", "wt16"), ("w8", "w8"), ("w8t", "w8t"), ("slot", "w8_slot")):
                if t[name] is not None:
                    d[field] = t[name][0] if name == "slot" else t[name][0][0, c0:] if name in ("w16", "w8") else t[name][0][c0:]
            tiles.append(d)
    lr, b2, eps = 0.0006, 0.999, 1e-8
    lr_t = np.float32(R.adam_lr_t(lr, b1, b2, it))
    kw = dict(b1=b1, b2=b2, eps=eps, iter=it, batch=5, lr_t=float(lr_t), lr=lr, advance_batch=advance, models=models,
              model_stride=ar.stride if models > 1 else 0)
    return ar, tens, tiles, kw


def _adam_reference(t, kw, g_sum, e_g):
    """fp64 update of one tensor from the gradient sum (and the sum's error bound) -> refs and bounds of p, m, v"""
    b1, b2, eps = [float(np.float32(kw[k])) for k in ("b1", "b2", "eps")]
    lr_t = float(np.float32(kw["lr_t"]))
    rows, cols = t["rows"], t["cols"]
    p0, m0, v0 = [t[n + "0"][:, :rows, :cols].astype(np.float64) for n in ("p", "m", "v")]
    p, m, v = R.adam(p0, m0, v0, g_sum, lr_t, b1, b2, eps)
    e_m = (1 - b1) * e_g + 3 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * g_sum))
    e_v = (1 - b2) * (2 * np.abs(g_sum) * e_g + e_g ** 2) + 4 * U * (b2 * v0 + (1 - b2) * g_sum ** 2)
    den = np.sqrt(v) + eps
    e_den = np.minimum(e_v / (2 * np.sqrt(v)), np.sqrt(e_v)) + 2 * U * den
    upd = lr_t * m / den
    e_p = lr_t * (e_m / den + np.abs(m) * e_den / den ** 2) + 4 * U * np.abs(upd) + U * (np.abs(p0) + np.abs(upd))
    return (p, e_p), (m, e_m), (v, e_v)


def _check_update(label, t, kw, g_sum, e_g, models):
    """p / m / v against the reference, their sentinels, and every copy against the kernel's own p"""
    rows, cols, ld, ldt = t["rows"], t["cols"], t["ld"], t["ldt"]
    refs = _adam_reference(t, kw, g_sum, e_g)
    worst = 0.0
    for name, (ref, bound) in zip(("p", "m", "v"), refs):
        got = torch.stack(t[name])
        worst = max(worst, _close("%s %s" % (label, name), got[:, :rows, :cols], ref, bound))
        inside = torch.zeros_like(got, dtype=torch.bool)
        inside[:, :rows, :cols] = True
        _assert_sentinel("%s %s" % (label, name), got, inside)
    p = torch.stack(t["p"])[:, :rows, :cols]
    if t["w16"] is not None:
        w16 = torch.stack(t["w16"])
        assert torch.equal(w16[:, :rows, :cols], p.to(torch.bfloat16)), label + ": w16 != bf16(p)"
        inside = torch.zeros_like(w16, dtype=torch.bool)
        inside[:, :rows, :cols] = True
        _assert_sentinel(label + " w16", w16.float(), inside)
    r16 = -(-rows // 16) * 16
    if t["wt16"] is not None:
        wt = torch.stack(t["wt16"])
        assert torch.equal(wt[:, :cols, :rows], w16[:, :rows, :cols].transpose(1, 2)), label + ": wt16 != w16^T"
        assert bool((wt[:, :cols, rows:r16] == 0).all()), label + ": wt16 rows up to the 16-row group must be zeros"
        inside = torch.zeros_like(wt, dtype=torch.bool)
        inside[:, :cols, :r16] = True
        _assert_sentinel(label + " wt16", wt.float(), inside)
    if t["w8"] is not None:
        w8, w8t = torch.stack(t["w8"]), torch.stack(t["w8t"])
        pack = lambda x: (x.float() * W8_SCALE).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        zero = lambda b: torch.where(b == 0x80, torch.zeros_like(b), b)          # +0 and -0 are the same value
        assert torch.equal(zero(w8[:, :rows, :cols]), zero(pack(w16[:, :rows, :cols]))), label + ": w8 != e4m3(w16 * scale)"
        assert torch.equal(zero(w8t[:, :cols, :r16]), zero(pack(wt[:, :cols, :r16]))), label + ": w8t != e4m3(wt16 * scale)"
        assert bool((w8[:, rows:] == BYTE_SENT).all()) and bool((w8[:, :rows, cols:] == BYTE_SENT).all())
        assert bool((w8t[:, cols:] == BYTE_SENT).all()) and bool((w8t[:, :cols, r16:] == BYTE_SENT).all())
        amax_bits, _ = _E().fp8_slots_read(t["slot"])
        assert float(amax_bits.view(np.float32)[0]) == float(w16[0, :rows, :cols].float().abs().max()), label + ": slot amax != max |w16|"
    return worst


def _g_sum(t):
    g = t["g0"].astype(np.float64)
    return g.sum(axis=1), t["nslab"] * U * np.abs(g).sum(axis=1)


@pytest.mark.parametrize("nslab,b1,it", [(1, 0.5, 0), (3, 0.9, 7), (4, 0.5, 7), (7, 0.9, 0), (8, 0.5, 0), (33, 0.9, 7)])
def test_adam_fused(nslab, b1, it):
    E = _E()
    ar, tens, tiles, kw = _adam_case(nslab, b1, it)
    rng = _rng(17, nslab)
    nloss = 257 if nslab % 2 else 3
    lp = rng.standard_normal((nloss + 1, 4)).astype(np.float32)
    out = torch.full((2, 4), SENT, dtype=torch.float32, device=DEV)          # step_out, accum
    out[1, :3] = torch.tensor([1.5, -2.25, 0.75])
    rc, nxt = E.debug_adam(tiles, mode=E.ADAM_FUSED, publish_next=1, loss_part=_dev(lp), nloss_part=nloss, inv_rows=1.0 / 50, step_out=out[0],
                           accum=out[1], **kw)
    _ok(rc)
    label = "adam fused nslab %d b1 %.1f iter %d" % (nslab, b1, it)
    worst = max(_check_update("%s tile %dx%d" % (label, t["rows"], t["cols"]), t, kw, *_g_sum(t), models=1) for t in tens)
    ar.check_gaps(label)
    print("%s: largest usage %.3f" % (label, worst))
    for t in tens:                                         # nothing but the documented tensors: the flat buffers stay untouched
        assert bool((t["flat"][0] == SENT).all()) and bool((t["flat16"][0].float() == SENT).all())
    # the next DevState: iterations + 1, batch + advance_batch, lr_t of the update after this one
    assert int(nxt[0]) == it + 1 and int(nxt[1]) == 5 + 1 and int(nxt[3]) == 0, nxt
    want = R.adam_lr_t(kw["lr"], float(np.float32(b1)), float(np.float32(kw["b2"])), it + 1)
    got = float(nxt[2:3].view(np.float32)[0])
    print("%s: next lr_t %.9g want %.9g" % (label, got, want))
    assert abs(got - want) <= 2.0 ** -22 * want
    # the metrics finish
    s = lp[:nloss, :3].astype(np.float64).sum(axis=0) / 50
    e_s = (nloss * U * np.abs(lp[:nloss, :3].astype(np.float64)).sum(axis=0) / 50 + 2 * U * np.abs(s))
    o = out.cpu().double().numpy()
    acc0 = np.array([1.5, -2.25, 0.75])
    _close(label + " step_out", o[0, :3], s, e_s)
    _close(label + " accum", o[1, :3], acc0 + s, e_s + U * np.abs(acc0 + s))
    assert o[0, 3] == SENT and o[1, 3] == SENT


def test_adam_reduce_only_then_from_flat_equals_fused():
    E = _E()
    nslab, b1, it = 7, 0.9, 7
    label = "adam flat"
    ar_f, tens_f, tiles_f, kw = _adam_case(nslab, b1, it)
    _ok(E.debug_adam(tiles_f, mode=E.ADAM_FUSED, publish_next=0, **kw)[0])
    ar, tens, tiles, kw = _adam_case(nslab, b1, it)                          # the same draws again
    lp = _rng(18).standard_normal((3, 4)).astype(np.float32)
    tail = torch.full((6,), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((2, 4), SENT, dtype=torch.float32, device=DEV)
    rc, nxt = E.debug_adam(tiles, mode=E.ADAM_REDUCE_ONLY, publish_next=1, loss_part=_dev(lp), nloss_part=3, inv_rows=0.5, step_out=out[0],
                           accum=out[1], flat_tail=tail, **kw)
    _ok(rc)
    assert [int(x) for x in nxt] == [0xA5A5A5A5] * 4, "ADAM_REDUCE_ONLY publishes no DevState"
    assert bool((out == SENT).all()), "ADAM_REDUCE_ONLY writes its sums to flat_tail only"
    s = lp[:, :3].astype(np.float64).sum(axis=0) * 0.5
    tl = tail.cpu().double().numpy()
    _close(label + " flat_tail", tl[:3], s, 3 * U * np.abs(lp[:, :3].astype(np.float64)).sum(axis=0) * 0.5 + 2 * U * np.abs(s))
    assert tl[3] == 0.0 and tl[4] == SENT and tl[5] == SENT
    for t in tens:
        rows, cols = t["rows"], t["cols"]
        g_sum, e_g = _g_sum(t)
        flat = t["flat"][0]
        _close("%s %dx%d flat" % (label, rows, cols), flat[:rows, :cols], g_sum[0], e_g[0])
        inside = torch.zeros_like(flat, dtype=torch.bool)
        inside[:rows, :cols] = True
        _assert_sentinel(label + " flat", flat, inside)
        for name in ("p", "m", "v"):                       # untouched, sentinels included
            assert torch.equal(t[name][0].cpu(), torch.from_numpy(t[name + "0"][0])), "%s: REDUCE_ONLY wrote %s" % (label, name)
        for name in ("w16", "wt16", "flat16"):
            assert t[name] is None or bool((t[name][0].float() == SENT).all())
        for name in ("w8", "w8t"):
            assert t[name] is None or bool((t[name][0] == BYTE_SENT).all())
    ar.check_gaps(label)
    # ADAM_FROM_FLAT on those sums: the fused update bit for bit (p, m, v and every copy)
    out2 = torch.full((2, 4), SENT, dtype=torch.float32, device=DEV)
    out2[1] = 0
    rc, nxt = E.debug_adam(tiles, mode=E.ADAM_FROM_FLAT, publish_next=1, step_out=out2[0], accum=out2[1], flat_tail=tail, **kw)
    _ok(rc)
    assert int(nxt[0]) == it + 1
    assert torch.equal(out2[0, :3], tail[:3]) and torch.equal(out2[1, :3], tail[:3]) and float(out2[0, 3]) == SENT
    for t, tf in zip(tens, tens_f):
        for name in ("p", "m", "v", "w16", "wt16", "w8", "w8t"):
            if t[name] is not None:
                a, b = t[name][0], tf[name][0]
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s: FROM_FLAT %s of tile %dx%d differs from FUSED" % (label, name, t["rows"], t["cols"])
    ar.check_gaps(label + " from_flat")


def test_adam_bf16_flat_gradients():
    """MRGAN_FLAG_GRAD_BF16: REDUCE_ONLY stores the sums as bf16, FROM_FLAT updates from exactly those values"""
    E = _E()
    ar, tens, tiles, kw = _adam_case(4, 0.5, 0, key=2, flat16=True)
    _ok(E.debug_adam(tiles, mode=E.ADAM_REDUCE_ONLY, publish_next=0, **kw)[0])
    for t in tens:
        rows, cols = t["rows"], t["cols"]
        g_sum, e_g = _g_sum(t)
        f16 = t["flat16"][0]
        _close("adam flat16 %dx%d" % (rows, cols), f16[:rows, :cols], g_sum[0], e_g[0] + BF16_RND * (np.abs(g_sum[0]) + e_g[0]))
        inside = torch.zeros_like(f16, dtype=torch.bool)
        inside[:rows, :cols] = True
        _assert_sentinel("adam flat16", f16.float(), inside)
        assert bool((t["flat"][0] == SENT).all())
    _ok(E.debug_adam(tiles, mode=E.ADAM_FROM_FLAT, publish_next=0, **kw)[0])
    for t in tens:
        g = t["flat16"][0][:t["rows"], :t["cols"]].cpu().double().numpy()[None]
        _check_update("adam from flat16 %dx%d" % (t["rows"], t["cols"]), t, kw, g, np.zeros_like(g), models=1)


def test_adam_model_groups():
    E = _E()
    ar, tens, tiles, kw = _adam_case(3, 0.5, 7, models=2)
    lp = _rng(19).standard_normal((2, 3, 4)).astype(np.float32)
    lpt = ar.alloc((3, 4), torch.float32, lp)
    out = ar.alloc((2, 4), torch.float32, np.zeros((2, 2, 4), np.float32))
    rc, nxt = E.debug_adam(tiles, mode=E.ADAM_FUSED, publish_next=1, loss_part=lpt[0], nloss_part=3, inv_rows=1.0, step_out=out[0][0], accum=out[0][1], **kw)
    _ok(rc)
    assert int(nxt[0]) == 8 and int(nxt[1]) == 6          # published once, by model 0
    worst = max(_check_update("adam models tile %dx%d" % (t["rows"], t["cols"]), t, kw, *_g_sum(t), models=2) for t in tens)
    print("adam model groups: largest usage %.3f" % worst)
    for m in range(2):
        s = lp[m, :, :3].astype(np.float64).sum(axis=0)
        _close("adam models step_out %d" % m, out[m][0, :3], s, 5 * U * np.abs(lp[m, :, :3].astype(np.float64)).sum(axis=0))
    ar.check_gaps("adam models")
    # the other modes take one model only
    assert E.debug_adam(tiles, mode=E.ADAM_REDUCE_ONLY, publish_next=0, **kw)[0] == -3
    assert E.debug_adam(tiles, mode=E.ADAM_FROM_FLAT, publish_next=0, **kw)[0] == -3
    tiles[0]["ld"] = tiles[0]["ld"] + 1                    # a pitch the 16-byte accesses cannot take
    assert E.debug_adam(tiles, mode=E.ADAM_FUSED, publish_next=0, **dict(kw, models=1, model_stride=0))[0] == -1


# =====================================================================================================================
# head_kernel (the scalar loss head): <float>, <bf16>, <bf16, Q8>, <float, KWIDE>, <bf16, KWIDE> (fp64 accumulators)
#
# delta = 2 feat U (|f||W6| + |b|) per logit (the KWIDE bf16 kernel sums in fp64: 2 U (|f||W6| + |b|)); d_row = its row maximum.
#   lse = mx + log(sum exp(l - mx))   e_lse = d_row + 2 U span + KP U + 4 SOFTPLUS_REL + SOFTPLUS_ABS + SOFTPLUS_REL |lse|
#                                     (1-Lipschitz in the max norm; exp of an argument rounded by U span; a sum of KP terms)
#   softmax p_c                       e_p = p_c (2 d_row + 2 U span + KP U + 4 SOFTPLUS_REL)
#   LAB   loss = lse - l_y            e_lse + d_row + U (|lse| + |l_y|);  dl = (p - 1_y) / B: (e_p + 2 U |p - 1_y|) / B
#   UNL / FAKE  sp = softplus(lse)    e_sp = e_lse + SOFTPLUS_ABS + SOFTPLUS_REL sp;  sigmoid: e_sg = e_lse / 4 + SIGMOID_ABS
#               k = w (sg - 1 | sg) / 2B: e_k = w e_sg / 2B + 3 U |k|;  dl = k p: e_k p + |k| e_p + 3 U |dl|
#   MSE   d = l - 1_y                 e_d = delta + U |d|; loss = mean d^2: sum (2 |d| e_d + e_d^2) / K + (K + 2) U loss
#   block sums of 32 rows             sum of the rows' bounds + 32 U sum |term|
#   dL/d(pre5) = (dl W6^T) [f > 0]    sum_c e_dl |W6| + 2 KP U sum_c |dl||W6|  (fp64 accumulators: 2 U)
#   dW6 = f^T dl per block            sum_r |f| e_dl + 32 U sum_r |f||dl|
# Underflow (found on the FAKE rows with logits near -80, where dl is an fp32 subnormal): a softmax term may be flushed by expf
# (FLUSH = 2^-126 absolute on p), and every fp32 result carries up to half a subnormal spacing whatever its size (UF = 2^-149 per
# operation: 4 on a dlogit, one per term of the sums above).
# Train error: a row whose two largest reference logits are closer than 2 d_row is undecided (a block with such rows may count
# each either way); the two identical W6 columns count as one logit there, argmax takes the first of them.
# =====================================================================================================================
KINDS3 = (R.LAB, R.UNL, R.FAKE)


def _head_row_bounds(kind, l, delta, y, inv, w, KP):
    """per-row bounds of (loss0, loss1, dlogits) around the reference logits l [rows][classes]"""
    B, K = l.shape
    d_row = delta.max(axis=1)
    if kind == R.MSE:
        live = (y >= 0)[:, None]
        onehot = np.zeros_like(l)
        onehot[np.arange(B)[y >= 0], y[y >= 0]] = 1
        d = (l - onehot) * live
        e_d = (delta + U * np.abs(d)) * live
        loss = (d * d).mean(axis=1)
        return (2 * np.abs(d) * e_d + e_d ** 2).sum(axis=1) / K + (K + 2) * U * loss, np.zeros(B), 2 * inv / K * e_d + 3 * U * np.abs(2 * d / K * inv) + 4 * UF
    mx = l.max(axis=1)
    span = mx - l.min(axis=1)
    lse = mx + np.log(np.exp(l - mx[:, None]).sum(axis=1))
    p = np.exp(l - lse[:, None])
    rel = 2 * U * span + KP * U + 4 * SOFTPLUS_REL
    e_lse = d_row + rel + SOFTPLUS_ABS + SOFTPLUS_REL * np.abs(lse)
    e_p = p * (2 * d_row + rel)[:, None] + FLUSH
    if kind == R.LAB:
        onehot = np.zeros_like(l)
        onehot[np.arange(B), y] = 1
        ly = l[np.arange(B), y]
        return e_lse + d_row + U * (np.abs(lse) + np.abs(ly)), np.zeros(B), inv * (e_p + 2 * U * np.abs(p - onehot)) + 4 * UF
    sp = np.maximum(lse, 0) + np.log1p(np.exp(-np.abs(lse)))
    sg = 1.0 / (1.0 + np.exp(-lse))
    e_sp = e_lse + SOFTPLUS_ABS + SOFTPLUS_REL * sp
    e_sg = 0.25 * e_lse + SIGMOID_ABS
    k = 0.5 * inv * w * (sg - 1.0 if kind == R.UNL else sg)
    e_k = 0.5 * inv * w * e_sg + 3 * U * np.abs(k)
    dl = k[:, None] * p
    e_l1 = 0.5 * (e_sp + (e_lse if kind == R.UNL else 0.0)) + 2 * U * (sp + np.abs(lse))
    return np.zeros(B), e_l1, e_k[:, None] * p + np.abs(k)[:, None] * e_p + 3 * U * np.abs(dl) + 4 * UF


def _blocks(x, nblk, hb=32):
    """[rows, ...] -> sums over hb-row blocks [nblk, ...]"""
    pad = np.zeros((nblk * hb - x.shape[0],) + x.shape[1:])
    return np.concatenate([x, pad]).reshape((nblk, hb) + x.shape[1:]).sum(axis=1)


def _head_delta(dtype, KP, feat, wide):
    """the factor of (|f||W6| + |b|) in a logit's bound: fp32 chains of `feat` fmas; fp64 accumulators at the 32-class pitch of the
    bf16 head_kernel; three bf16 addends of W6 per feature in fp32 MFMA accumulators on the wide head"""
    return 2 * 3 * feat * U if wide else 2 * U if (KP == 32 and dtype == BF16) else 2 * feat * U


def _head_undecided(l, delta, c2):
    """rows whose two largest reference logits (the tie pair counting as one) are closer than twice the row's logit bound"""
    lx = np.delete(l, c2, axis=1)
    if lx.shape[1] < 2:
        return np.zeros(l.shape[0], bool)
    top = np.sort(lx, axis=1)
    return top[:, -1] - top[:, -2] < 2 * delta.max(axis=1)


def _head_grad_bounds(fs, Wv, dl, e_dl, dp, bits, dtype, KP, HB, nblk, wide):
    """bounds of the head's gradients around the reference dlogits dl (bound e_dl) and dL/d(pre5) dp of one segment (formulas in
    the comment above; shared with tests/test_chain_kernel.py, whose head is the matrix-core one at KP = 8) ->
    e_dp (dpre before the store), dpre (as stored), dw_ref / dw (dW6 per HB-row block), db6, dbf (per block)"""
    aW = np.abs(Wv)
    fp64_acc = KP == 32 and dtype == BF16 and not wide
    # wide: six addend pairs x 16-deep k-steps of exact products in fp32 accumulators, the dropped pairs below 4 U
    acc_df = (2 * 6 * 16 * (1 if KP == 8 else 2) + 4) * U if wide else 2 * U if fp64_acc else 2 * KP * U
    e_df = e_dl @ aW.T + acc_df * (np.abs(dl) @ aW.T) + KP * UF
    e_dp = e_df * bits
    ndw = 2 * 3 * 64 if wide else 32                   # wide: 64 rows x three addends of dlogits in fp32 MFMA accumulators
    blk = lambda x, i: x[i * HB:(i + 1) * HB]
    return dict(
        e_dp=e_dp, dpre=e_dp + BF16_RND * (np.abs(dp) + e_dp) if dtype == BF16 else e_dp,
        dw_ref=np.stack([blk(fs, i).T @ blk(dl, i) for i in range(nblk)]),
        dw=np.stack([np.abs(blk(fs, i)).T @ (blk(e_dl, i) + ndw * U * np.abs(blk(dl, i))) for i in range(nblk)]) + HB * UF,
        db6=_blocks(e_dl, nblk, HB) + HB * U * _blocks(np.abs(dl), nblk, HB) + HB * UF,
        dbf=_blocks(e_dp, nblk, HB) + HB * U * _blocks(np.abs(dp), nblk, HB) + HB * UF)


def _head_inputs(dtype, kinds, classes, feat, feat_valid, rows, models=1, stream=False, hot=False, key=0, wide=False, **_):
    """The draws of one head case (numpy only, so the CPU suite can hold the seeds: tests/test_aux_refs_cpu.py) ->
    (rng, f, W6, b, labels, batch, (undecided rows, rows with a label, tie rows)).  The labels of the rows on which the two identical
    W6 columns hold the maximum are set afterwards, the first two thirds to the first column and the rest to the second: a
    kernel that took the LAST index of a tie then counts another number of errors, whatever the seed."""
    KP = 8 if classes <= 8 else 32
    nseg = len(kinds)
    rng = _rng(20 + wide, dtype, classes, feat, feat_valid, rows, models, key, *kinds)
    c1, c2 = (1, classes - 1) if classes > 2 else (0, 1)
    f = np.maximum(rng.standard_normal((models, nseg, rows, feat)) - 0.3, 0.0)
    if hot:
        f[:, :, :32] *= 100.0                               # one row block of every segment with logits near +-80
    f[..., feat_valid:] = 0.0                               # the padding columns of the features are zeros in the engine
    f = _round_to(f, dtype)
    assert (f[..., :feat_valid] == 0).any()
    W = (rng.standard_normal((models, feat, KP)) / np.sqrt(feat)).astype(np.float32)      # junk in columns >= classes, rows >= feat_valid
    W[:, :, c2] = W[:, :, c1]
    b = (0.3 * rng.standard_normal((models, KP))).astype(np.float32)
    b[:, c1] += 0.75
    b[:, c2] = b[:, c1]
    labels = rng.integers(0, classes, (models, 2, rows)).astype(np.int32)
    if R.MSE in kinds:
        labels[:, :, rows - 7:] = -1
    batch = 1 if stream else 0
    und_n = lab_n = tie_n = 0
    for m in range(models):
        for s, kind in enumerate(kinds):
            if kind not in (R.LAB, R.EVAL, R.MSE):
                continue
            Wv = W[m].astype(np.float64)[:, :classes].copy()
            Wv[feat_valid:] = 0.0
            b64 = b[m].astype(np.float64)[:classes]
            l = f[m, s] @ Wv + b64
            l[:, c2] = l[:, c1]
            delta = _head_delta(dtype, KP, feat, wide) * (np.abs(f[m, s]) @ np.abs(Wv) + np.abs(b64))
            live = labels[m, batch] >= 0
            und = _head_undecided(l, delta, c2) & live
            tie = np.nonzero((l[:, c1] == l.max(axis=1)) & live & ~und)[0]
            labels[m, batch, tie[:(2 * len(tie) + 2) // 3]] = c1
            labels[m, batch, tie[(2 * len(tie) + 2) // 3:]] = c2
            und_n, lab_n, tie_n = und_n + int(und.sum()), lab_n + int(live.sum()), tie_n + len(tie)
    return rng, f, W, b, labels, batch, (und_n, lab_n, tie_n)


def _run_head(dtype, kinds, classes, feat, feat_valid, rows, models=1, stream=False, hot=False, q8=False, key=0, wide=False):
    E = _E()
    tdt, KP = TDT[dtype], 8 if classes <= 8 else 32
    HB = 64 if wide else 32                                 # rows per block: head_wide_kernel works on 64
    nseg, nblk = len(kinds), -(-rows // HB)
    label = "%s %s kinds %s K %d feat %d/%d rows %d%s%s" % ("head_wide" if wide else "head", "bf16" if dtype else "f32", list(kinds), classes, feat, feat_valid, rows,
                                                              " models %d" % models if models > 1 else "", " q8" if q8 else "")
    inv, w_unl = 1.0 / rows, 0.75
    ldf, ldd, srows = feat + 8, feat + 16, rows + GAP
    off_db = feat * KP + 4
    off_dbf = off_db + KP + 4
    pstride = off_dbf + feat + 4
    c1, c2 = (1, classes - 1) if classes > 2 else (0, 1)
    ar = Arena(12 << 20, models)
    # ---- inputs ----
    rng, f, W, b, labels, batch, _ = _head_inputs(dtype, kinds, classes, feat, feat_valid, rows, models, stream, hot, key, wide)
    fbuf = np.full((models, nseg, srows, ldf), np.nan)
    fbuf[:, :, :rows, :feat] = f
    tf = ar.alloc((nseg, srows, ldf), tdt, fbuf)
    tw = ar.alloc((feat, KP), torch.float32, W)
    tb = ar.alloc((KP,), torch.float32, b)
    logits = ar.alloc((nseg, srows, KP), torch.float32, SENT)
    dpre = ar.alloc((nseg, srows, ldd), tdt, SENT)
    part = ar.alloc((nseg * nblk + 1, pstride), torch.float32, SENT)
    lpart = ar.alloc((nseg * nblk + 1, 4), torch.float32, SENT)
    tl = _dev(labels, torch.int32)
    kw = dict(dtype=dtype, f=tf[0], f_bs=srows * ldf, ldf=ldf, rows=rows, nseg=nseg, seg_kind=list(kinds), feat=feat, feat_valid=feat_valid,
              classes=classes, w=tw[0], ldw=KP, b=tb[0], labels=tl, labels_stream=1 if stream else 0, batch=batch, inv_count=inv,
              unl_weight=w_unl, logits=logits[0], logits_bs=srows * KP, dpre=dpre[0], dpre_bs=srows * ldd, ldd=ldd, part=part[0],
              part_stride=pstride, off_db=off_db, off_dbf=off_dbf, loss_part=lpart[0], models=models,
              model_stride=ar.stride if models > 1 else 0, labels_ms=2 * rows)
    errc = None
    if R.EVAL in kinds:
        errc = torch.full((2,), 100, dtype=torch.int32, device=DEV)
        kw["err_count"] = errc
    if q8:
        scale, r32 = 2.0 ** 14, nblk * HB
        q8t_bs = r32 + 16
        ldq8, ldq8t = feat + 16, (nseg - 1) * q8t_bs + r32 + 16
        q8b = torch.full((nseg, srows, ldq8), BYTE_SENT, dtype=torch.uint8, device=DEV)
        q8tb = torch.full((feat + 1, ldq8t), BYTE_SENT, dtype=torch.uint8, device=DEV)
        slot = E.fp8_slots([(0.0, scale, 1.0 / scale, 28672.0)])
        kw.update(q8=q8b, q8_bs=srows * ldq8, ldq8=ldq8, q8t=q8tb, q8t_bs=q8t_bs, ldq8t=ldq8t, q8_slot=slot)
    bits = f > 0
    if wide:
        # the relu mask the wide head follows: f > 0, except a few elements flipped either way (the mask decides, not f)
        flip = rng.random(f.shape) < 0.01
        flip[..., feat_valid:] = False
        bits = bits ^ flip
        assert (bits & (f == 0)).any() and (~bits & (f > 0)).any()
        nb32, ldm = -(-rows // 32), feat + 16
        words = np.zeros((nseg, nb32 + 1, ldm, 2), dtype=np.uint16)
        for s in range(nseg):
            junk = mask_encode(rng.random((nb32 * 32, ldm)) < 0.5, ldm)
            own = mask_encode(np.ones((rows, feat), bool), ldm)
            words[s, :nb32] = (junk & ~own) | mask_encode(bits[0, s], ldm)
        w6c = torch.full((3 * KP * feat + 64,), SENT, dtype=torch.bfloat16, device=DEV)
        w6r = torch.full((3 * KP * feat + 64,), SENT, dtype=torch.bfloat16, device=DEV)
        kw.pop("dtype")
        if q8:
            kw.pop("dpre")                                  # the e5m2 images leave in its place
        _ok(E.debug_head_wide(mask=torch.from_numpy(words.view(np.int16)).to(DEV), mask_bs=(nb32 + 1) * ldm * 2, ldm=ldm, w6c=w6c, w6r=w6r, **kw))
        # the addends of W6: zeros outside [feat_valid][classes], and their sum is W6 exactly
        Wm = np.zeros((feat, KP))
        Wm[:feat_valid, :classes] = W[0, :feat_valid, :classes]
        c3 = w6c[:3 * KP * feat].double().cpu().numpy().reshape(3, KP, feat)
        r3 = w6r[:3 * KP * feat].double().cpu().numpy().reshape(3, feat, KP)
        assert np.array_equal(c3.sum(axis=0), Wm.T) and np.array_equal(r3.sum(axis=0), Wm), label + ": the bf16 addends do not sum to W6"
        assert np.array_equal(c3, r3.transpose(0, 2, 1))
        assert bool((w6c[3 * KP * feat:].float() == SENT).all()) and bool((w6r[3 * KP * feat:].float() == SENT).all())
    else:
        _ok(E.debug_head(**kw))
    ar.check_gaps(label)
    # ---- reference and checks, per model and segment ----
    worst, undecided, nrows, tie_rows = 0.0, 0, 0, 0
    q8_lo = q8_hi = 0.0
    training = [k for k in kinds if k not in (R.EVAL, R.LOGITS)]
    err_total = 0
    for m in range(models):
        W64, b64 = W[m].astype(np.float64), b[m].astype(np.float64)
        Wv = W64[:, :classes].copy()
        Wv[feat_valid:] = 0.0
        y = labels[m, batch].astype(np.int64)
        got_logits = logits[m].cpu().double().numpy()
        got_dpre = dpre[m].float().cpu().double().numpy()
        got_part = part[m].cpu().double().numpy()
        got_lp = lpart[m].cpu().double().numpy()
        for s, kind in enumerate(kinds):
            tag = "%s m%d seg%d" % (label, m, s)
            fs = f[m, s]
            l = fs @ Wv + b64[:classes]
            l[:, c2] = l[:, c1]                             # identical columns: identical sums on both sides
            mag = np.abs(fs) @ np.abs(Wv) + np.abs(b64[:classes])
            # (wide: three bf16 addends of W6 per feature, exact products, fp32 MFMA accumulators: 3 feat terms)
            delta = _head_delta(dtype, KP, feat, wide) * mag
            worst = max(worst, _close(tag + " logits", got_logits[s, :rows, :classes], l, delta))
            assert (got_logits[s, :rows, classes:] == 0).all(), tag + ": logits columns >= classes must be exact zeros"
            assert (got_logits[s, rows:] == SENT).all()
            loss0, loss1, err, dl = R.head_rows(l, kind, y, inv, w_unl)
            if kind in (R.LAB, R.EVAL, R.MSE):
                d_row = delta.max(axis=1)
                und = _head_undecided(l, delta, c2)          # (the tie pair as one logit)
                if kind == R.MSE:
                    und &= y >= 0
                tie = (l[:, c1] == l.max(axis=1))
                assert not (tie & und).any(), tag + ": a constructed tie row is undecided (change the seed)"
                tie_rows += int(tie.sum())
                undecided += int(und.sum())
                nrows += rows
                lo, hi = _blocks(err * ~und, nblk, HB), _blocks(err * ~und + und, nblk, HB)
                if tie.any():
                    # a kernel that took the LAST index of a tie must come out with another block sum somewhere
                    live_y = (y >= 0) if kind == R.MSE else np.ones(rows, bool)
                    wrong = np.where(tie, (live_y & (y != c2)).astype(np.float64), err)
                    assert (_blocks(wrong * ~und, nblk, HB) != lo).any(), tag + ": the tie rows would not show a wrong tie order (change the seed)"
                if kind == R.EVAL:
                    err_total += int(round(float((err * ~und).sum())))
                    assert not und.any(), tag + ": undecided rows in an error count (change the seed)"
            if kind in (R.EVAL, R.LOGITS):
                continue
            e0, e1, e_dl = _head_row_bounds(kind, l, delta, y, inv, w_unl, KP)
            if wide:
                e_dl = e_dl + 2.0 ** -133                   # dlogits travel as three bf16 addends: the last one may underflow
            blk0 = s * nblk
            lp = got_lp[blk0:blk0 + nblk]
            worst = max(worst, _close(tag + " loss0", lp[:, 0], _blocks(loss0, nblk, HB), _blocks(e0, nblk, HB) + HB * U * _blocks(np.abs(loss0), nblk, HB)))
            worst = max(worst, _close(tag + " loss1", lp[:, 1], _blocks(loss1, nblk, HB), _blocks(e1, nblk, HB) + HB * U * _blocks(np.abs(loss1), nblk, HB)))
            assert (lp[:, 3] == 0).all()
            if kind in (R.LAB, R.MSE):
                assert ((lp[:, 2] >= lo) & (lp[:, 2] <= hi)).all(), (tag, lp[:, 2], lo, hi)
            else:
                assert (lp[:, 2] == 0).all()
            dw6, db6, dp, dbf = R.head_backward(fs, Wv, dl, live=bits[m, s])
            gb = _head_grad_bounds(fs, Wv, dl, e_dl, dp, bits[m, s], dtype, KP, HB, nblk, wide)
            e_dp, bound = gb["e_dp"], gb["dpre"]
            if wide and q8:
                assert (got_dpre == SENT).all(), tag + ": the fp8 form writes no dpre"
            else:
                worst = max(worst, _close(tag + " dpre", got_dpre[s, :rows, :feat], dp, bound))
                assert (got_dpre[s, rows:] == SENT).all() and (got_dpre[s, :rows, feat:] == SENT).all()
            pr = got_part[blk0:blk0 + nblk]
            gw = pr[:, :feat * KP].reshape(nblk, feat, KP)
            worst = max(worst, _close(tag + " dW6", gw[:, :, :classes], gb["dw_ref"], gb["dw"]))
            assert (gw[:, :, classes:] == 0).all(), tag + ": dW6 columns >= classes must be exact zeros"
            worst = max(worst, _close(tag + " db6", pr[:, off_db:off_db + classes], _blocks(dl, nblk, HB), gb["db6"]))
            assert (pr[:, off_db + classes:off_db + KP] == 0).all()
            worst = max(worst, _close(tag + " dbf", pr[:, off_dbf:off_dbf + feat], _blocks(dp, nblk, HB), gb["dbf"]))
            for a0, a1 in ((feat * KP, off_db), (off_db + KP, off_dbf), (off_dbf + feat, pstride)):
                assert (pr[:, a0:a1] == SENT).all(), tag + ": part row written outside dW6 / db6 / dbf"
            if q8:
                qb, qt = q8b[s].cpu(), q8tb.cpu()
                dec = qb[:rows, :feat].contiguous().view(torch.float8_e5m2).to(torch.float64).numpy()
                if wide:                                    # no dpre to compare with: the code must lie between those of ref -+ bound
                    from oracle import mrgan_oracle as O
                    qlo, qhi = O.fp8_round((dp - e_dp) * scale, 'e5m2'), O.fp8_round((dp + e_dp) * scale, 'e5m2')
                    assert ((dec >= qlo) & (dec <= qhi)).all(), tag + ": q8 outside the codes of ref -+ bound"
                    q8_lo = max(q8_lo, float((np.abs(dp) - e_dp).max()))
                    q8_hi = max(q8_hi, float((np.abs(dp) + e_dp).max()))
                else:
                    assert _e5m2_neighbour(dec, got_dpre[s, :rows, :feat] * scale).all(), tag + ": q8 is not a neighbour of the stored dpre"
                assert bool((qb[rows:] == BYTE_SENT).all()) and bool((qb[:rows, feat:] == BYTE_SENT).all())
                seg_t = qt[:feat, s * q8t_bs:s * q8t_bs + r32]
                assert torch.equal(seg_t[:, :rows].contiguous(), qb[:rows, :feat].t().contiguous()), tag + ": q8t != q8^T"
                assert bool(((seg_t[:, rows:] & 0x7F) == 0).all()), tag + ": q8t rows beyond the segment must be zeros"
                assert bool((qt[:feat, s * q8t_bs + r32:(s + 1) * q8t_bs if s + 1 < nseg else ldq8t] == BYTE_SENT).all()) and bool((qt[feat] == BYTE_SENT).all())
        if not training:
            assert (got_part == SENT).all() and (got_lp == SENT).all() and (got_dpre == SENT).all(), label + ": a non-training kind wrote gradients"
        else:
            assert (got_part[nseg * nblk] == SENT).all() and (got_lp[nseg * nblk] == SENT).all()
    if errc is not None:
        assert errc.cpu().tolist() == [100 + err_total, 100], (label, errc.cpu().tolist(), err_total)
    if q8:
        amax_bits, _ = E.fp8_slots_read(slot)
        amax = float(amax_bits.view(np.float32)[0])
        if wide:
            assert q8_lo <= amax <= q8_hi, (label, amax, q8_lo, q8_hi)
        else:
            assert float(torch.tensor(amax).to(tdt)) == float(torch.stack(dpre)[:, :, :rows, :feat].float().abs().max()), label + ": slot amax"
    share = undecided / max(1, nrows)
    print("%s: largest usage %.3f, undecided rows %d / %d, tie rows %d" % (label, worst, undecided, nrows, tie_rows))
    assert share <= 0.01
    return tie_rows


def _hc(dtype, kinds, classes, feat, feat_valid, rows, **kw):
    return dict(dtype=dtype, kinds=tuple(kinds), classes=classes, feat=feat, feat_valid=feat_valid, rows=rows, **kw)


# every launch of the head tests, as data: the CPU suite walks the same list to hold the seeds (no undecided row, tie rows present)
HEAD_CASES = (
    [_hc(d, KINDS3, *c, hot=True) for d in (F32, BF16) for c in [(6, 256, 250, 40), (2, 64, 64, 70), (8, 320, 320, 40), (9, 512, 500, 70),
                                                                  (20, 64, 64, 40), (32, 256, 250, 70)]]
    + [_hc(d, (k,), K, 320 if K == 6 else 256, 320 if K == 6 else 250, 70, stream=k in (R.LAB, R.MSE))
       for d in (F32, BF16) for k in (R.LAB, R.UNL, R.FAKE, R.EVAL, R.LOGITS, R.MSE) for K in (6, 20)]
    + [c for d, K in ((F32, 6), (BF16, 6), (BF16, 20)) for c in (_hc(d, KINDS3, K, 256, 250, 40, models=2),
                                                                 _hc(d, (R.MSE,), K, 64, 64, 70, models=2, stream=True, key=1))]
    + [_hc(BF16, KINDS3, 6, 256, 250, 40, q8=True), _hc(BF16, KINDS3, 8, 320, 320, 70, q8=True, hot=True, key=1)])
WIDE_CASES = (
    [_hc(BF16, k, *c[:4], hot=True, wide=True, key=c[4] if len(c) > 4 else 0) for c, k in [((6, 256, 250, 40), KINDS3), ((8, 512, 512, 70), KINDS3), ((2, 512, 512, 40), (R.LAB,)),
                                                        ((6, 256, 250, 70), (R.UNL,)), ((8, 512, 512, 40), (R.FAKE,)), ((9, 256, 250, 70), KINDS3),
                                                        ((20, 512, 512, 40, 2), KINDS3), ((32, 256, 250, 70), KINDS3), ((20, 512, 512, 70), (R.LAB,))]]
    + [_hc(BF16, KINDS3, 6, 256, 250, 40, q8=True, wide=True), _hc(BF16, KINDS3, 8, 512, 512, 70, q8=True, wide=True, hot=True, key=2)])


def _case_id(c):
    return "-".join(str(v) if not isinstance(v, tuple) else "k" + "".join(map(str, v)) for v in c.values())


@pytest.mark.parametrize("case", HEAD_CASES, ids=_case_id)
def test_head(case):
    _run_head(**case)


def test_head_refusals():
    E = _E()
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    kw = dict(dtype=BF16, f=z(40, 72, dt=torch.bfloat16), f_bs=0, ldf=72, rows=40, nseg=1, seg_kind=[R.LAB], feat=64, feat_valid=64, classes=6,
              w=z(96, 8), ldw=8, b=z(8), labels=z(40, dt=torch.int32), inv_count=1.0 / 40, unl_weight=1.0, logits=z(40, 8),
              dpre=z(40, 72, dt=torch.bfloat16), ldd=72, part=z(2, 1024), part_stride=1024, off_db=512, off_dbf=520, loss_part=z(2, 4))
    assert E.debug_head(**kw) == 0
    assert E.debug_head(**dict(kw, feat=96, feat_valid=96, ldf=96, ldd=96, f=z(40, 96, dt=torch.bfloat16), dpre=z(40, 96, dt=torch.bfloat16),
                               off_db=768, off_dbf=776)) == -3                       # feat % 64
    slot = E.fp8_slots([(0.0, 1.0, 1.0, 28672.0)])
    q8 = torch.zeros((40, 64), dtype=torch.uint8, device=DEV)
    wide = dict(kw, classes=20, ldw=32, w=z(64, 32), b=z(32), logits=z(40, 32), part=z(2, 4096), part_stride=4096, off_db=2048, off_dbf=2080)
    assert E.debug_head(**wide) == 0
    assert E.debug_head(**dict(wide, q8=q8, ldq8=64, q8_slot=slot)) == -3            # no e5m2 epilogue at the 32-class pitch
    assert E.debug_head(**dict(kw, q8=q8, ldq8=64, q8_slot=slot, models=2, model_stride=0)) == -3     # model groups keep no fp8 copies
    assert E.debug_head(**dict(kw, ldf=60)) == -1                                    # a pitch below the feature width
    assert E.debug_head(**dict(kw, ldf=68)) == -1                                    # a pitch the 16-byte loads cannot take


# =====================================================================================================================
# head_wide_kernel + w6_split_kernel (the matrix-core head): <false>, <true> (e5m2 images), <false, KWIDE>
# The same reference and row bounds as head_kernel, with the terms of its own products: W6 and dlogits enter as three bf16 addends
# (exact: 3 x 8 significant bits), every product of two addends is exact in fp32, and the MFMA accumulators add 3 feat terms
# per logit (delta = 2 * 3 feat U (|f||W6| + |b|)), 6 addend pairs x 16 classes per k-step for dL/d(pre5) (+ 4 U for the three
# dropped pairs) and 64 rows x 3 addends for dW6.  Blocks are 64 rows.  dL/d(pre5) follows the relu MASK, which the test makes
# disagree with f > 0 on 1 % of the elements.
# =====================================================================================================================
@pytest.mark.parametrize("case", WIDE_CASES, ids=_case_id)
def test_head_wide(case):
    _run_head(**case)


def test_head_wide_refusals():
    E = _E()
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    bf = torch.bfloat16
    kw = dict(f=z(40, 264, dt=bf), f_bs=0, ldf=264, rows=40, nseg=1, seg_kind=[R.LAB], feat=256, feat_valid=256, classes=6, w=z(256, 8), ldw=8,
              b=z(8), labels=z(40, dt=torch.int32), inv_count=1.0 / 40, unl_weight=1.0, logits=z(40, 8), dpre=z(40, 264, dt=bf), ldd=264,
              part=z(1, 4096), part_stride=4096, off_db=2048, off_dbf=2056, loss_part=z(1, 4),
              mask=z(2, 264, 2, dt=torch.int16), ldm=264, w6c=z(3 * 8 * 256, dt=bf), w6r=z(3 * 8 * 256, dt=bf))
    assert E.debug_head_wide(**kw) == 0
    assert E.debug_head_wide(**dict(kw, seg_kind=[R.EVAL])) == -3                    # training kinds only
    assert E.debug_head_wide(**dict(kw, seg_kind=[R.MSE])) == -3
    assert E.debug_head_wide(**dict(kw, feat=192, feat_valid=192, off_db=1536, off_dbf=1544)) == -3     # feat % 256
    assert E.debug_head_wide(**dict(kw, ldd=260)) == -1                              # 16-byte stores of dpre
    assert E.debug_head_wide(**dict(kw, ldm=200)) == -1                              # a mask pitch below the feature width
