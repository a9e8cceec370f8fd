"""The step-level GPU parity checks, once: the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Every engine variant (the default engine, MRGAN_FLAG_GAUSS_NOISE, more than eight classes) is held to the SAME bodies with the
same bounds; what distinguishes a variant is a Variant, passed explicitly.  The test files parametrise these bodies and keep
what is specific to their variant.

Tolerances.  north_star: logits within 1e-3 rel of the reference arithmetic for the fp32 mode.  "rel" is
scale-relative (max |err| / max |ref|).  Weights after Adam steps are compared relative to the size of the
update: early Adam moves every weight by ~lr * sign(g), so an element whose true gradient is at rounding level
may legitimately move the other way (documented in DESIGN.md).  bf16 mode is held to 3e-2 on logits and is pinned
for accuracy, not logits, by north_star (+-0.5 % accuracy).
"""
import collections
import functools

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.dist import DataParallel, EngineBackend, PhaseBackend, dp_flags
from oracle import mrgan_oracle as O
from tests.gaussian_noise import gaussian_normal
from tests.helpers import SEED, Case, cosine, frob_rel_err, noise_set, rel_err, update_rel_err

DEV = "cuda:0"


def to_dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def engine(D, B, dtype, flags=0, rank=0, world=1, d_hidden=None, g_hidden=None, **cfg_fields):
    """a handle on DEV; cfg_fields = further mrgan_config fields (num_classes, lr, beta1, seed, ...)"""
    cfg = E.default_config(D, B)
    cfg.dtype, cfg.seed, cfg.flags, cfg.rank, cfg.world = dtype, SEED, flags, rank, world
    for i, w in enumerate(d_hidden or ()):
        cfg.d_hidden[i] = w
    for i, w in enumerate(g_hidden or ()):
        cfg.g_hidden[i] = w
    for k, v in cfg_fields.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return E.Engine(cfg, DEV)


def load(eng, case):
    eng.set_weights(E.NET_G, [p.astype(np.float32) for p in case.g0])
    eng.set_weights(E.NET_D, [p.astype(np.float32) for p in case.d0])


def disc_args(case, t, device_z=False, rows=slice(None)):
    """arguments of D sub-step t (optionally of a row shard); device_z: the engine draws z"""
    return E.Engine.disc_args(to_dev(case.x_lab[t][rows]), to_dev(case.labels[t][rows], torch.int32), to_dev(case.x_unl[t][rows]),
                              None if device_z else to_dev(case.z1[t][rows]))


def gen_args(case, t, device_z=False, rows=slice(None)):
    return E.Engine.gen_args(to_dev(case.x_unl2[t][rows]), None if device_z else to_dev(case.z2[t][rows]))


def run_engine(eng, case, device_z=False):
    """the compiled functions of mr_gan.py:169-171 over the case's (D, G) pairs; same keys as Case.run_oracle"""
    out = dict(disc=[], gen=[])
    out['logits0'] = eng.predict_logits(to_dev(case.probe)).cpu().numpy()
    for t in range(case.steps):
        out['disc'].append(eng.disc_step(disc_args(case, t, device_z)))
        out['gen'].append(eng.gen_step(gen_args(case, t, device_z)))
    out['logits'] = eng.predict_logits(to_dev(case.probe)).cpu().numpy()
    out['g'] = eng.get_weights(E.NET_G)
    out['d'] = eng.get_weights(E.NET_D)
    return out


class Variant(collections.namedtuple("Variant", "flags num_classes normal")):
    """What distinguishes an engine variant in the bodies below: the flags OR-ed into every handle, the class count (None =
    the reference's six, mrgan_default_config's) and the restated generator its problems draw noise and device z from."""

    def case(self, **kw):
        return Case(normal=self.normal, K=self.num_classes, **kw)

    def engine(self, D, B, dtype, flags=0, **kw):
        if self.num_classes is not None:
            kw['num_classes'] = self.num_classes
        return engine(D, B, dtype, flags | self.flags, **kw)

    def noise_set(self, *args, **kw):
        return noise_set(*args, normal=self.normal, **kw)


DEFAULT = Variant(0, None, O.device_normal)
GAUSSIAN = Variant(E.FLAG_GAUSS_NOISE, None, gaussian_normal)


def classes(K):
    return Variant(0, K, O.device_normal)


# ---------------------------------------------------------------------------------------------------------
# fp32 against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------
def fp32_gradients_match_oracle(variant, D, B, steps=1, device_z=False):
    """Flat-gradient mode exposes the raw gradients of one D step and one G step.  Returns the D gradients."""
    case = variant.case(D=D, B=B, steps=steps, device_z=device_z)
    orc = O.MRGANOracle(case.g0, case.d0)
    (ll, lu, err), gd, _ = orc.disc_grads(**case.disc_inputs(0, 0))
    eng = variant.engine(D, B, 0, flags=E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS)
    load(eng, case)
    da = disc_args(case, 0, device_z)
    eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
    got_d = eng.get_slot(E.NET_D, 2)
    for i, (a, b) in enumerate(zip(got_d, gd)):
        assert rel_err(a, b) < 2e-5, ("dD", i, rel_err(a, b))          # measured ~5e-7 (scripts/parity_probe.py)
    out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
    np.testing.assert_allclose(out, (ll, lu, err), rtol=2e-4, atol=2e-5)
    orc.adam.apply(orc.d, gd, 'd')
    loss, gg, _ = orc.gen_grads(**case.gen_inputs(0, 1))
    ga = gen_args(case, 0, device_z)
    eng.gen_step(ga, E.G_GEN, E.G_TAIL, want_outputs=False)
    for i, (a, b) in enumerate(zip(eng.get_slot(E.NET_G, 2), gg)):
        assert rel_err(a, b) < 2e-4, ("dG", i, rel_err(a, b))          # measured ~1e-5 on db1 (cancellation), ~1e-6 elsewhere
    assert abs(eng.gen_step(ga, E.G_ADAM, E.G_ADAM) - loss) < 2e-3 * abs(loss) + 1e-9
    eng.close()
    return got_d


@functools.lru_cache(maxsize=None)
def _fp32_problem(variant, D, B, device_z):
    """(case, its fp64 trajectory, the restatement's float32 trajectory) of three (D, G) pairs; shared, never modified"""
    case = variant.case(D=D, B=B, steps=3, device_z=device_z)
    return case, case.run_oracle(), variant.case(D=D, B=B, steps=3, device_z=device_z, dtype=np.float32).run_oracle()


def fp32_steps_match_oracle(variant, D, B, device_z=False):
    case, ref, r32 = _fp32_problem(variant, D, B, device_z)
    eng = variant.engine(D, B, 0)
    load(eng, case)
    got = run_engine(eng, case, device_z)
    assert rel_err(got['logits0'], ref['logits0']) < 1e-5
    # Everything after the first Adam update is bounded by what plain float32 arithmetic allows: the restatement evaluated
    # in float32 on the same inputs (r32) deviates from its own fp64 run (rounding differences of near-zero gradients pass
    # through Adam's m / (sqrt(v) + eps) as +-lr steps; tests/test_oracle.py shows > 1e-3 on logits at (800, 256)), so the
    # engine gets max(the tight tolerance, 3 x that float32-vs-float64 deviation).  The first sub-step has no such slack.
    for t in range(case.steps):
        dev = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(r32['disc'][t][:2], ref['disc'][t][:2]))
        np.testing.assert_allclose(got['disc'][t][:2], ref['disc'][t][:2], rtol=2e-4 if t == 0 else max(2e-4, 3 * dev), atol=2e-5)
        assert abs(got['disc'][t][2] - ref['disc'][t][2]) <= (1e-6 if t == 0 else 1.01 / B)
        dev = abs(r32['gen'][t] - ref['gen'][t]) / abs(ref['gen'][t])
        np.testing.assert_allclose(got['gen'][t], ref['gen'][t], rtol=max(2e-3, 3 * dev), atol=1e-9)
    # weights after three (D, G) pairs: pins the shared Adam counter (t = 2n-1 / 2n)
    for key, w0s in (('d', case.d0), ('g', case.g0)):
        for i, (w, wr, w0, w32) in enumerate(zip(got[key], ref[key], w0s, r32[key])):
            e, e32 = update_rel_err(w, wr, w0), update_rel_err(w32, wr, w0)
            assert e < max(0.02, 3 * e32), (key, i, e, e32)
    # logits of fresh rows after the three updates.  north_star's 1e-3 holds wherever plain float32 arithmetic allows it:
    # with e32 the float32 restatement's own deviation from fp64 (e32 > 1e-3 at (800, 256)), the engine is bounded by
    # max(1e-3, 2 * e32)
    e32 = rel_err(r32['logits'], ref['logits'])
    assert rel_err(got['logits'], ref['logits']) < max(1e-3, 2.0 * e32), (rel_err(got['logits'], ref['logits']), e32)
    assert eng.get_iterations() == 2 * case.steps
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# engine against mirror against fp64
# ---------------------------------------------------------------------------------------------------------
def grad_parity(variant, D, B, dtype, quantize, tol, tol_loss, d_hidden=None, g_hidden=None, eval_first=True, frac=0.6,
                loose=(0.995, 0.98, 0.25)):
    """One D sub-step and one G sub-step in flat-gradient mode: all 20 gradient tensors and the four losses.

    fp32 engine (quantize None): against the fp64 restatement at `tol`.
    bf16 engine: against the oracle MIRROR, which rounds to bf16 exactly where the engine stores bf16.  What is left
    between engine and mirror is fp32-vs-fp64 accumulation: a pre-activation is a sum of K signed terms, so its fp32 error
    relative to its own size is ~sqrt(K) * 1e-7 ~ 1e-5 .. 1e-4, which flips the bf16 rounding of a few per cent of the stored
    activations by one ulp (2^-8); ten chained layers and the cancellation in the bias gradients bring that to 1e-3 .. 2e-2
    on the gradients (measured: scripts/parity_probe.py).  A wrong kernel shows up as an error against the mirror as
    large as the error against the fp64 oracle, so the bound is: err(engine, mirror) < max(tol, frac * err(mirror, fp64)), frac = 0.6
    -- the mirror must explain most of what bf16 does -- and, labelled loose, the direction against fp64.
    fp8 engine: the same rule against MRGANMirror(quantize='fp8')."""
    kw = {k: v for k, v in (('d_hidden', d_hidden), ('g_hidden', g_hidden)) if v}
    case = variant.case(D=D, B=B, steps=1, **kw)
    mir = O.MRGANMirror(case.g0, case.d0, quantize=quantize)
    orc = O.MRGANOracle(case.g0, case.d0)
    (ll, lu, err), gd_m, _ = mir.disc_grads(**case.disc_inputs(0, 0))
    (ll_o, lu_o, _), gd_o, _ = orc.disc_grads(**case.disc_inputs(0, 0))
    eng = variant.engine(D, B, dtype, flags=E.FLAG_FLAT_GRADS, **kw)
    load(eng, case)
    if eval_first:
        # an evaluation first: it fills ALL rows of the activation buffers (also the padding rows of a ragged batch),
        # which the training step afterwards must tolerate
        rs = np.random.RandomState(5)
        eng.eval_error(to_dev(rs.randn(3 * 128 + 7, D).astype(np.float32)), to_dev(rs.randint(0, case.K, size=3 * 128 + 7), torch.int32))
    da = disc_args(case, 0)
    eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
    report = []

    def check(name, got, want_m, want_o, cos_min):
        for i, (a, m, o) in enumerate(zip(got, want_m, want_o)):
            em, eo, emo = frob_rel_err(a, m), frob_rel_err(a, o), frob_rel_err(m, o)
            report.append("%s%-2d %.1e %.1e %.1e" % (name, i, em, eo, emo))
            assert em < max(tol, frac * emo), (name + " vs mirror", i, em, emo)
            if quantize:      # loose, vs fp64: ten chained contractions on bf16 operands keep the gradient's direction
                assert cosine(a, o) > cos_min and eo < loose[2], (name + " vs fp64", i, cosine(a, o), eo)

    try:
        check("dD", eng.get_slot(E.NET_D, 2), gd_m, gd_o, loose[0])
        out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
        # losses: the same rule as the gradients -- within tol_loss of the mirror, or within `frac` of what the storage format itself
        # does to the loss (mirror vs fp64), whichever is larger (reductions of length 4096 in fp8: 2.0e-3 against a mirror that is
        # itself 1 % from fp64)
        for got_l, m_l, o_l in zip(out[:2], (ll, lu), (ll_o, lu_o)):
            np.testing.assert_allclose(got_l, m_l, rtol=max(tol_loss, frac * abs(m_l - o_l) / max(abs(o_l), 1e-12)), atol=tol_loss * 0.1)
        assert abs(out[2] - err) <= ((4.01 if quantize == 'fp8' else 1.01) / B if quantize else 1e-6)      # an argmax or two may flip
        # the G sub-step sees the D network AFTER its update: give engine, mirror and oracle the same updated weights
        mir.adam.apply(mir.d, gd_m, 'd')
        if quantize == 'fp8':           # mrgan_set_weights below re-measures the fp8 weight copies in two passes; so does the mirror
            for _ in range(2):
                mir._refresh_w8()
                mir.slots.update()
        orc.d = [p.copy() for p in mir.d]
        orc.adam.iterations = 1
        eng.set_weights(E.NET_D, [p.astype(np.float32) for p in mir.d])
        loss, gg_m, _ = mir.gen_grads(**case.gen_inputs(0, 1))
        _, gg_o, _ = orc.gen_grads(**case.gen_inputs(0, 1))
        ga = gen_args(case, 0)
        eng.gen_step(ga, E.G_GEN, E.G_TAIL, want_outputs=False)
        check("dG", eng.get_slot(E.NET_G, 2), gg_m, gg_o, loose[1])
        lg = eng.gen_step(ga, E.G_ADAM, E.G_ADAM)
        assert abs(lg - loss) < 5 * tol_loss * abs(loss) + 1e-12, (lg, loss)
    finally:
        eng.close()
        shape = ("K=%d, " % case.K if variant.num_classes else "") + "D=%d, B=%d" % (D, B)
        print("\n(%s) tensor: err vs mirror | vs fp64 | mirror vs fp64\n  " % shape + "\n  ".join(report))


def supervised_steps_match_oracle(variant, dtype, D, B, short):
    """mrgan_sup_step = one train_on_batch of the NN baseline (mr_nn.py:101-118).  fp32 against the fp64 restatement, bf16
    against the bf16 mirror (tolerance rule of test_bf16_steps_match_bf16_mirror); `short` = Keras' short last batch."""
    case = variant.case(D=D, B=B, steps=3)
    kw = dict(lr=O.NN_ADAM_LR, b1=O.NN_ADAM_B1)
    ref = O.MRGANOracle(case.g0, case.d0, **kw)
    mir = O.MRGANMirror(case.g0, case.d0, quantize='bf16' if dtype else None, **kw)
    eng = variant.engine(D, B, dtype, lr=O.NN_ADAM_LR, beta1=O.NN_ADAM_B1)
    load(eng, case)
    for t in range(case.steps):
        n = short if (short and t == 1) else B
        x, y = case.x_lab[t].astype(np.float64), case.labels[t]
        noise = [m[:n] for m in variant.noise_set(SEED, 0, t, B, D)]
        yb = y.copy()
        yb[n:] = -1
        got = eng.sup_step(E.Engine.sup_args(to_dev(case.x_lab[t]), to_dev(yb, torch.int32), rows_valid=0 if n == B else n))
        want, wm = ref.sup_step(x[:n], y[:n], noise), mir.sup_step(x[:n], y[:n], noise)
        slack = 0.0 if t == 0 else 0.25
        if dtype == 0:
            assert abs(got[0] - want[0]) < (2e-4 + slack * 0.02) * want[0], (t, got, want)
        else:
            assert abs(got[0] - wm[0]) < max(3e-3, 0.6 * abs(wm[0] - want[0]) / want[0] + slack * 0.2) * want[0], (t, got, wm, want)
        assert abs(got[1] - (want[1] if dtype == 0 else wm[1])) <= (1e-6 if t == 0 else 2.01 / n)
    for i, (a, b, m, w0) in enumerate(zip(eng.get_weights(E.NET_D), ref.d, mir.d, case.d0)):
        if dtype == 0:
            assert update_rel_err(a, b, w0) < 0.03, ("D", i, update_rel_err(a, b, w0))
        else:
            assert update_rel_err(a, m, w0) < max(0.05, 0.85 * update_rel_err(m, b, w0)), ("D", i, update_rel_err(a, m, w0), update_rel_err(m, b, w0))
    assert eng.get_iterations() == case.steps
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# two launch forms of the same arithmetic
# ---------------------------------------------------------------------------------------------------------
def _dpre_within_one_ulp(a, b, what):
    """bf16 dL/d(pre) of two summation orders of the loss head: within one ulp (2^-7 of the largest element), on < 5 % of rows"""
    d = np.abs(a - b)
    assert d.max() <= 2.0 ** -7 * np.abs(b).max() and (d.max(axis=2) > 0).mean() < 0.05, (what, d.max(), (d.max(axis=2) > 0).mean())


def matrix_core_loss_head_equals_scalar_head(variant, dtype, B, kernel_names=False):
    """Feature layers wider than the chain holds (here 512 columns = two chunks; BASELINE configs[4]: 4096) run the loss head of
    the D sub-step as the stand-alone MFMA kernel over 64-row blocks (head_wide.hip: head_wide_kernel; TUNE_HEAD_MFMA = 1, the
    default) instead of head_kernel's fmaf loops over 32-row blocks.  Same rule as the chain body below: three-addend bf16 splits
    make every product exact, only the fp32 summation order differs -- losses to 1e-6, the bf16 dL/d(pre5) within one ulp on a few
    rows (fp8 mode: the e5m2 copies are what leaves the kernel; compared through the weight gradients), D gradients to 5e-4.
    B = 200: a ragged last row block (8 valid rows); dtype 2: the fp8 engine (e5m2 row-major + transposed copies, amax slot).
    kernel_names: also check through the profiler which head kernel ran, and that the D-tail chain did not."""
    D, hid = 96, (256, 256, 256, 512, 512)
    case = variant.case(D=D, B=B, steps=1, device_z=True, d_hidden=hid)
    res = []
    for mfma in (1, 0):
        eng = variant.engine(D, B, dtype, flags=E.FLAG_FLAT_GRADS, d_hidden=hid)
        eng.set_tuning(E.TUNE_HEAD_MFMA, mfma)
        load(eng, case)
        da = disc_args(case, 0, device_z=True)
        if kernel_names:
            eng.profile_begin()
        eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
        if kernel_names:
            names = set(eng.profile_end())
            assert ("head_wide_kernel" in names) == bool(mfma) and ("head_kernel" in names) != bool(mfma), names
            assert "chain_kernel<0>" not in names
        gd = eng.get_slot(E.NET_D, 2)
        dpre = eng.debug_buffer(1, 4).cpu().numpy()[:, :B] if dtype == 1 else None
        out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
        res.append((gd, out, dpre))
        eng.close()
    (gd1, out1, dp1), (gd0, out0, dp0) = res
    np.testing.assert_allclose(out1, out0, rtol=1e-6, atol=1e-7)
    if dtype == 1:
        d = np.abs(dp1 - dp0)
        print("\nK=%d: max |d dpre| %.3e of %.3e, rows that differ %.4f, dD %s"
              % (case.K, d.max(), np.abs(dp0).max(), (d.max(axis=2) > 0).mean(), " ".join("%.1e" % rel_err(a, b) for a, b in zip(gd1, gd0))))
        _dpre_within_one_ulp(dp1, dp0, "dpre5")
    for i, (a, b) in enumerate(zip(gd1, gd0)):
        assert rel_err(a, b) < (5e-4 if dtype == 1 else 5e-3), ("dD", i, rel_err(a, b))


def chain_launches_equal_per_layer_launches(variant, D, B):
    """The 256-wide tail D3..D5 + loss head (+ its dX chain) as row-block chain launches (gemm_chain.hip) against the same
    products launched layer by layer (B = 50: a ragged, partly empty row block).
    * Every dense product has the identical MFMA accumulation order and epilogue arithmetic in both forms: the stored layer
      inputs xin[l] and the features are BIT-IDENTICAL, and so is the whole G sub-step (no loss head in it) when both engines
      start it from the same discriminator weights.
    * The loss head inside the chain runs on the matrix cores (three-addend bf16 splits of the fp32 factors: exact products,
      fp32 accumulation), head_kernel of the per-layer path is an fmaf chain: the same fp32 arithmetic in another summation
      order.  The losses agree to 1e-6; dlogits differ by ~1e-7 relative, which flips the bf16 rounding of a few stored
      dL/d(pre) values by one ulp (measured at (400, 256): 19 of 768 rows hold such an element) -- the gradients therefore agree
      to ~1e-4 of their largest element instead of bit for bit."""
    case = variant.case(D=D, B=B, steps=1, device_z=True)
    res, engines = [], []
    for chain in (1, 0):
        eng = variant.engine(D, B, 1, flags=E.FLAG_FLAT_GRADS)
        eng.set_tuning(E.TUNE_CHAIN, chain)
        load(eng, case)
        da = disc_args(case, 0, device_z=True)
        eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
        gd = eng.get_slot(E.NET_D, 2)
        acts = [eng.debug_buffer(0, l).cpu().numpy()[:, :B] for l in range(5)] + [eng.debug_buffer(2, 0).cpu().numpy()[:, :B]]
        dpre = [eng.debug_buffer(1, l).cpu().numpy()[:, :B] for l in range(5)]
        out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
        res.append((gd, out, acts, dpre))
        engines.append(eng)
    (gd1, out1, acts1, dpre1), (gd0, out0, acts0, dpre0) = res
    np.testing.assert_allclose(out1, out0, rtol=1e-6, atol=1e-7)
    for l, (a, b) in enumerate(zip(acts1, acts0)):
        np.testing.assert_array_equal(a, b, err_msg="layer input / features %d" % l)
    for l, (a, b) in enumerate(zip(dpre1, dpre0)):
        _dpre_within_one_ulp(a, b, ("dpre", l))
    for i, (a, b) in enumerate(zip(gd1, gd0)):
        assert rel_err(a, b) < 5e-4, ("dD", i, rel_err(a, b))
    # the G sub-step from identical discriminator weights (Adam turns rounding-level gradient differences into +-lr steps)
    wd = engines[0].get_weights(E.NET_D)
    gres = []
    for eng in engines:
        eng.set_weights(E.NET_D, wd)
        ga = gen_args(case, 0, device_z=True)
        eng.gen_step(ga, E.G_GEN, E.G_TAIL, want_outputs=False)
        gg = eng.get_slot(E.NET_G, 2)
        gres.append((gg, eng.gen_step(ga, E.G_ADAM, E.G_ADAM)))
        eng.close()
    (gg1, lg1), (gg0, lg0) = gres
    assert abs(lg1 - lg0) <= 1e-6 * abs(lg0)
    for i, (a, b) in enumerate(zip(gg1, gg0)):
        assert rel_err(a, b) < 2e-5, ("dG", i, rel_err(a, b))


# ---------------------------------------------------------------------------------------------------------
# data parallelism, emulated on one GPU: rank handles whose "all-reduce" is a host-side add
# ---------------------------------------------------------------------------------------------------------
def rank_args(case, t, world=2):
    """([disc_args of rank r], [gen_args of rank r]) of pair t: equal row shards, z drawn on the device"""
    h = case.B // world
    shards = [slice(r * h, (r + 1) * h) for r in range(world)]
    return [disc_args(case, t, True, s) for s in shards], [gen_args(case, t, True, s) for s in shards]


D_EXCHANGES = ((E.D_GEN, E.REGION_BN_STATS, True), (E.D_MAIN, E.REGION_GRAD_D, False))      # (phase, what it produced, a batch statistic?)
G_EXCHANGES = ((E.G_GEN, E.REGION_BN_STATS, True), (E.G_FEAT, E.REGION_FM_MOMENTS, True), (E.G_BWD, E.REGION_BN_BWD, True),
               (E.G_TAIL, E.REGION_GRAD_G, False))


def _walk(step, exchanges, ranks, args, allreduce, exact):
    for ph, reg, statistic in exchanges:
        for e, a in zip(ranks, args):
            getattr(e, step)(a, ph, ph, want_outputs=False)
        if exact or not statistic:                 # per-shard statistics (exact=False): only the gradients travel
            allreduce(reg)


def disc_walk(ranks, da, allreduce, exact=True):
    """the D sub-step up to its all-reduced flat gradients (get_slot(NET_D, 2) reads them); D_ADAM is left to the caller"""
    _walk("disc_step", D_EXCHANGES, ranks, da, allreduce, exact)


def gen_walk(ranks, ga, allreduce, exact=True):
    _walk("gen_step", G_EXCHANGES, ranks, ga, allreduce, exact)


def phase_walk(ranks, da, ga, allreduce):
    """One (D, G) pair through the data-parallel phases (mr_gan_amd/dist.py): every phase on every rank, then the all-reduce
    of the region it produced, then the Adam phase.  -> (the D outputs per rank, the G loss per rank)"""
    disc_walk(ranks, da, allreduce)
    d_out = [e.disc_step(a, E.D_ADAM, E.D_ADAM) for e, a in zip(ranks, da)]
    gen_walk(ranks, ga, allreduce)
    return d_out, [e.gen_step(a, E.G_ADAM, E.G_ADAM) for e, a in zip(ranks, ga)]


def two_rank_emulation_equals_full_batch(variant):
    """rows are global: two shards of 32 rows draw rows 0 .. 31 and 32 .. 63 of the full batch's noise and z"""
    B, D = 64, 32
    case = variant.case(D=D, B=B, steps=2, device_z=True)
    ref = case.run_oracle()
    ranks = [variant.engine(D, B // 2, 0, flags=E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS, rank=r, world=2) for r in range(2)]
    for e in ranks:
        load(e, case)

    def allreduce(region):
        views = [e.region(region) for e in ranks]
        tot = views[0] + views[1]
        for v in views:
            v.copy_(tot)

    for t in range(case.steps):
        d_out, g_out = phase_walk(ranks, *rank_args(case, t), allreduce=allreduce)
        np.testing.assert_allclose(d_out[0], ref['disc'][t], rtol=3e-4, atol=3e-5)
        np.testing.assert_allclose(d_out[1], d_out[0], rtol=0, atol=0)
        np.testing.assert_allclose(g_out[0], ref['gen'][t], rtol=3e-3, atol=1e-9)
    w0, w1 = ranks[0].get_weights(E.NET_D), ranks[1].get_weights(E.NET_D)
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)                    # replicas stay bit-identical
    for i, (w, wr, wi) in enumerate(zip(w0, ref['d'], case.d0)):
        assert update_rel_err(w, wr, wi) < 0.05, ("D", i)
    for e in ranks:
        e.close()


# ---------------------------------------------------------------------------------------------------------
# W rank handles in lock step on one GPU (tests/test_data_parallel_gpu.py): the all-reduce is a device-side add over the
# ranks' exchange regions, the control flow is dist.DataParallel's own
# ---------------------------------------------------------------------------------------------------------
def sum_exchange(backends, on_exchange=None):
    """-> allreduce(which): the sum over the backends' exchange_regions(which), in rank order, written back to every one of
    them.  fp32 regions add in fp32; a bfloat16 payload adds in fp32 and rounds once, like a bf16 all-reduce
    (test_two_rank_emulation_with_bf16_gradient_payload).  on_exchange(which) is called behind each exchange."""
    def allreduce(which):
        for views in zip(*(b.exchange_regions(which) for b in backends)):
            acc = torch.float32 if views[0].dtype == torch.bfloat16 else views[0].dtype
            tot = views[0].to(acc)
            for v in views[1:]:
                tot = tot + v.to(acc)
            tot = tot.to(views[0].dtype)
            for v in views:
                v.copy_(tot)
        if on_exchange is not None:
            on_exchange(which)
    return allreduce


class LockstepBackend(PhaseBackend):
    """W PhaseBackends (one per rank: EngineBackend, or the oracle stand-in of the CPU tests) as the one backend DataParallel
    drives: each call goes to every rank in turn, the step arguments are a list with one entry per rank (its row shard).
    pair_hint and fp8_calibration exist when every rank has them, as DataParallel asks (getattr)."""

    def __init__(self, backends):
        self.backends = list(backends)
        dtypes = {getattr(b, "grad_dtype", None) for b in self.backends}
        assert len(dtypes) == 1, dtypes
        self.grad_dtype = dtypes.pop()
        if all(hasattr(b, "pair_hint") for b in self.backends):
            self.pair_hint = self._pair_hint
        if all(hasattr(b, "fp8_calibration") for b in self.backends):
            self.fp8_calibration = self._fp8_calibration

    def disc_phase(self, args, phase):
        for b, a in zip(self.backends, args):
            b.disc_phase(a, phase)

    def gen_phase(self, args, phase):
        for b, a in zip(self.backends, args):
            b.gen_phase(a, phase)

    def region(self, which):
        raise NotImplementedError("a lock-step backend has one region per rank: LockstepDataParallel sums them")

    def _pair_hint(self, on=True):
        for b in self.backends:
            b.pair_hint(on)

    def _fp8_calibration(self, kind, action):
        rcs = {b.fp8_calibration(kind, action) for b in self.backends}
        assert len(rcs) == 1, ("the replicas disagree about their calibration state", kind, action, rcs)
        return rcs.pop()


class LockstepDataParallel(DataParallel):
    """dist.DataParallel over W ranks in one process: train_pair / disc_step / gen_step run unchanged (pair hint, fp8
    calibration order, which exchanges a sub-step skips); only the all-reduce is replaced, by sum_exchange."""

    def __init__(self, backends, exact=True, on_exchange=None):
        super().__init__(LockstepBackend(backends), exact=exact)
        self.world = len(backends)
        self._sum = sum_exchange(self.backend.backends, on_exchange)

    def _allreduce(self, which):
        self._sum(which)


def lockstep(ranks, exact=True, on_exchange=None):
    """LockstepDataParallel over engine handles"""
    return LockstepDataParallel([EngineBackend(e) for e in ranks], exact=exact, on_exchange=on_exchange)


def _equal_on_all_ranks(per_rank, what):
    for r, other in enumerate(per_rank[1:], 1):
        for i, (a, b) in enumerate(zip(per_rank[0], other)):
            np.testing.assert_array_equal(b, a, err_msg="%s %d: rank %d differs from rank 0" % (what, i, r))


def shard_mean_reference(case, make, shards, d_after=None):
    """One D and one G sub-step of `shards` independent references make() -> MRGANOracle | MRGANMirror, reference r on the rows
    [r h, (r + 1) h) of the batch with the noise and z of those GLOBAL rows: the mean over the references of their gradients and
    D outputs, and each one's generator loss.  shards = 1 is the full-batch step.  With per-shard statistics every rank scales its
    sums by 1 / B_global and its feature-matching gradient by 1 / world, so the all-reduced sum is this mean of shard means.
    The G sub-step runs on d_after (default: the D weights after Adam on the mean D gradients, as every replica applies them)."""
    h = case.B // shards
    models = [make() for _ in range(shards)]
    mean = lambda parts: [sum(ts) / shards for ts in zip(*parts)]
    outs, grads = zip(*[m.disc_grads(**case.disc_inputs(0, 0, rows=h, row0=r * h))[:2] for r, m in enumerate(models)])
    res = dict(d_out=np.mean(np.array(outs, np.float64), axis=0), gd=mean(grads))
    if d_after is None:
        models[0].adam.apply(models[0].d, res['gd'], 'd')
        d_after = models[0].d
    res['d_after'] = [np.array(p) for p in d_after]
    for m in models:
        m.d = [p.copy() for p in res['d_after']]
        m.adam.iterations = 1
    losses, grads = zip(*[m.gen_grads(**case.gen_inputs(0, 1, rows=h, row0=r * h))[:2] for r, m in enumerate(models)])
    res.update(g_loss=[float(l) for l in losses], gg=mean(grads))
    return res


@functools.lru_cache(maxsize=None)
def _dp_problem(variant, D, B, d_hidden, shards, quantize):
    """(case, the tight reference, the fp64 reference on the tight one's updated D weights); shared, never modified"""
    case = variant.case(D=D, B=B, steps=1, device_z=True, **({'d_hidden': d_hidden} if d_hidden else {}))
    o64 = lambda: O.MRGANOracle(case.g0, case.d0)
    if not quantize:
        ref = shard_mean_reference(case, o64, shards)
        return case, ref, ref
    mir = shard_mean_reference(case, lambda: O.MRGANMirror(case.g0, case.d0, quantize=quantize), shards)
    return case, mir, shard_mean_reference(case, o64, shards, d_after=mir['d_after'])


@functools.lru_cache(maxsize=None)
def _full_batch_handle_grads(variant, D, B, d_hidden, dtype, quantize):
    """(D gradients, G gradients) of ONE full-batch FLAT_GRADS | SYNC_STATS handle on the problem above: what W ranks should
    reproduce up to summation order.  Reported beside the references, not asserted."""
    case, ref, _ = _dp_problem(variant, D, B, d_hidden, 1, quantize)
    eng = variant.engine(D, B, dtype, flags=E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS, **({'d_hidden': d_hidden} if d_hidden else {}))
    try:
        load(eng, case)
        none = lambda which: None
        da, ga = [disc_args(case, 0, True)], [gen_args(case, 0, True)]
        disc_walk([eng], da, none)
        gd = eng.get_slot(E.NET_D, 2)
        eng.disc_step(da[0], E.D_ADAM, E.D_ADAM)
        eng.set_weights(E.NET_D, [p.astype(np.float32) for p in ref['d_after']])
        gen_walk([eng], ga, none)
        return gd, eng.get_slot(E.NET_G, 2)
    finally:
        eng.close()


FP32_GRAD_TOL = dict(dD=2e-5, dG=2e-4)        # the rel_err bounds of fp32_gradients_match_oracle


def dp_grad_parity(variant, D, B, world, dtype, tol=None, tol_loss=None, d_hidden=None, frac=0.6, loose=(0.995, 0.98, 0.25), exact=True):
    """The data-parallel twin of grad_parity: W rank handles at B / W rows (rank r: global rows [r h, (r + 1) h)), one D and one
    G sub-step through the phases with the all-reduces of the protocol in between; the all-reduced flat gradients and the
    outputs of the Adam phases against references of the FULL batch.
    exact (FLAT_GRADS | SYNC_STATS): the references are the full-batch MRGANMirror(quantize='bf16') and the fp64 oracle under
    the rule of grad_parity -- err(engine, mirror) < max(tol, frac * err(mirror, fp64)), and the loose direction bound.
    not exact (FLAT_GRADS, per-shard statistics): the mean over ranks of W shard-sized references (shard_mean_reference).
    dtype 0: the fp64 oracle alone, at the bounds of fp32_gradients_match_oracle.
    Every rank must hold the same all-reduced gradients and Adam outputs bit for bit.  The G sub-step starts from the same
    updated D weights on the engine, the mirror and the oracle, as in grad_parity."""
    quantize = 'bf16' if dtype else None
    kw = {'d_hidden': d_hidden} if d_hidden else {}
    case, ref_m, ref_o = _dp_problem(variant, D, B, d_hidden, 1 if exact else world, quantize)
    full = _full_batch_handle_grads(variant, D, B, d_hidden, dtype, quantize) if exact else None
    flags = E.FLAG_FLAT_GRADS | (E.FLAG_SYNC_STATS if exact else 0)
    ranks = [variant.engine(D, B // world, dtype, flags=flags, rank=r, world=world, **kw) for r in range(world)]
    allreduce = sum_exchange(ranks)
    report = []

    def check(name, k, want_m, want_o, cos_min):
        per_rank = [e.get_slot(E.NET_D if name == "dD" else E.NET_G, 2) for e in ranks]
        for i, (a, m, o) in enumerate(zip(per_rank[0], want_m, want_o)):
            em, eo, emo = frob_rel_err(a, m), frob_rel_err(a, o), frob_rel_err(m, o)
            report.append("%s%-2d %.1e %.1e %.1e" % (name, i, em, eo, emo) + (" %.1e" % frob_rel_err(a, full[k][i]) if full else ""))
        _equal_on_all_ranks(per_rank, name)
        for i, (a, m, o) in enumerate(zip(per_rank[0], want_m, want_o)):
            if quantize:
                em, emo = frob_rel_err(a, m), frob_rel_err(m, o)
                assert em < max(tol, frac * emo), (name + " vs mirror", i, em, emo)
                assert cosine(a, o) > cos_min and frob_rel_err(a, o) < loose[2], (name + " vs fp64", i, cosine(a, o), frob_rel_err(a, o))
            else:
                assert rel_err(a, o) < FP32_GRAD_TOL[name], (name, i, rel_err(a, o))

    try:
        for e in ranks:
            load(e, case)
        da, ga = rank_args(case, 0, world)
        disc_walk(ranks, da, allreduce, exact)
        check("dD", 0, ref_m['gd'], ref_o['gd'], loose[0])
        outs = [e.disc_step(a, E.D_ADAM, E.D_ADAM) for e, a in zip(ranks, da)]
        print("\nD outputs %s, reference %s" % (outs[0], tuple(ref_m['d_out'])))
        for out in outs[1:]:
            assert out == outs[0], outs                                 # the loss sums travel behind the gradients
        if quantize:             # the loss rule of grad_parity
            for got_l, m_l, o_l in zip(outs[0][:2], ref_m['d_out'][:2], ref_o['d_out'][:2]):
                np.testing.assert_allclose(got_l, m_l, rtol=max(tol_loss, frac * abs(m_l - o_l) / max(abs(o_l), 1e-12)), atol=tol_loss * 0.1)
            assert abs(outs[0][2] - ref_m['d_out'][2]) <= 1.01 / B      # an argmax may flip
        else:                    # fp32_gradients_match_oracle's
            np.testing.assert_allclose(outs[0], ref_o['d_out'], rtol=2e-4, atol=2e-5)
        for e in ranks:
            e.set_weights(E.NET_D, [p.astype(np.float32) for p in ref_m['d_after']])
        gen_walk(ranks, ga, allreduce, exact)
        check("dG", 1, ref_m['gg'], ref_o['gg'], loose[1])
        lgs = [e.gen_step(a, E.G_ADAM, E.G_ADAM) for e, a in zip(ranks, ga)]
        print("G loss per rank %s, reference %s" % (lgs, ref_m['g_loss']))
        # synchronised statistics: one loss, of the all-reduced moments; per-shard statistics: every rank its own shard's
        want = ref_m['g_loss'] * world if exact else ref_m['g_loss']
        assert not exact or all(lg == lgs[0] for lg in lgs), lgs
        for lg, loss in zip(lgs, want):
            assert abs(lg - loss) < ((5 * tol_loss) if quantize else 2e-3) * abs(loss) + (1e-12 if quantize else 1e-9), (lgs, want)
    finally:
        for e in ranks:
            e.close()
        print("(D=%d, B=%d, W=%d%s) tensor: err vs %s | vs fp64 | reference vs fp64%s\n  " % (
            D, B, world, "" if exact else ", per-shard statistics", "mirror" if quantize else "fp64", " | vs one full-batch handle" if full else "") + "\n  ".join(report))


def shards_stage_the_rows_of_the_full_batch(variant, dtype, D, B, world):
    """D_GEN + D_MAIN on W rank handles and on one full-batch handle with the same flags, every handle forced to one product tile
    (TUNE_KC_CFG 0): rows [0, h) of the two real-row segments on rank r against rows [r h, (r + 1) h) of the full batch's.
    * xin[0], the staged rows with their noise: a function of (seed, site, segment, iteration, GLOBAL row, column) alone.
    * xin[1], the first discriminator product with its noise epilogue: a row's reduction order does not depend on how many
      rows the launch has."""
    flags = E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS
    case = variant.case(D=D, B=B, steps=1, device_z=True)
    h = B // world
    full = variant.engine(D, B, dtype, flags=flags)
    ranks = [variant.engine(D, h, dtype, flags=flags, rank=r, world=world) for r in range(world)]
    try:
        for e in [full] + ranks:
            e.set_tuning(E.TUNE_KC_CFG, 0)
            load(e, case)
        disc_walk([full], [disc_args(case, 0, True)], lambda which: None)
        disc_walk(ranks, rank_args(case, 0, world)[0], sum_exchange(ranks))
        for l, what in ((0, "staged rows"), (1, "first product")):
            want = full.debug_buffer(0, l).cpu().numpy()
            assert np.abs(want[:2, :B]).max() > 0.1, what
            for r, e in enumerate(ranks):
                got = e.debug_buffer(0, l).cpu().numpy()
                for seg in (0, 1):
                    np.testing.assert_array_equal(got[seg, :h], want[seg, r * h:(r + 1) * h], err_msg="%s, segment %d, rank %d" % (what, seg, r))
    finally:
        for e in [full] + ranks:
            e.close()


def fp8_replicas_calibrate_in_lock_step(D, B, world):
    """One D and one G sub-step of W fp8 replicas through the lock-step DataParallel with synchronised statistics: the HOST runs
    the calibration passes, with real exchanges between the replicas.  -> nothing; asserts inside."""
    case = Case(D=D, B=B, steps=1, device_z=True)
    ranks = [engine(D, B // world, E.FP8, flags=dp_flags(exact=True), rank=r, world=world) for r in range(world)]
    seen = {}

    def tap(which):            # the all-reduced gradients, before the Adam phase
        if which in (E.REGION_GRAD_D, E.REGION_GRAD_G):
            seen.setdefault(which, []).append([e.get_slot(E.NET_D if which == E.REGION_GRAD_D else E.NET_G, 2) for e in ranks])

    try:
        for e in ranks:
            load(e, case)
        dp = lockstep(ranks, exact=True, on_exchange=tap)
        da, ga = rank_args(case, 0, world)
        orc = O.MRGANOracle(case.g0, case.d0)
        _, gd_o, _ = orc.disc_grads(**case.disc_inputs(0, 0))
        dp.disc_step(da)
        wd = [e.get_weights(E.NET_D) for e in ranks]
        orc.d = [p.astype(np.float64) for p in wd[0]]
        orc.adam.iterations = 1
        _, gg_o, _ = orc.gen_grads(**case.gen_inputs(0, 1))
        dp.gen_step(ga)
        assert len(seen[E.REGION_GRAD_D]) == 1 and len(seen[E.REGION_GRAD_G]) == 1       # the dry passes exchange no gradients
        for name, which, want, cos_min in (("dD", E.REGION_GRAD_D, gd_o, 0.9), ("dG", E.REGION_GRAD_G, gg_o, 0.8)):
            per_rank = seen[which][0]
            print("\n%s: cosine / err vs fp64 %s" % (name, " ".join("%.3f/%.2f" % (cosine(a, o), frob_rel_err(a, o)) for a, o in zip(per_rank[0], want))))
            _equal_on_all_ranks(per_rank, name)
            for i, (a, o) in enumerate(zip(per_rank[0], want)):
                assert cosine(a, o) > cos_min and frob_rel_err(a, o) < 0.6, (name + " vs fp64", i, cosine(a, o), frob_rel_err(a, o))
        _equal_on_all_ranks(wd, "D weight")
        _equal_on_all_ranks([e.get_weights(E.NET_G) for e in ranks], "G weight")
        for e in ranks:
            assert e.fp8_calibration(0, E.Engine.FP8_CAL_QUERY) == 1 and e.fp8_calibration(1, E.Engine.FP8_CAL_QUERY) == 1
    finally:
        for e in ranks:
            e.close()


@functools.lru_cache(maxsize=None)
def _pairs_problem(D, B, d_hidden, steps):
    """(case, its fp64 trajectory, the bf16 mirror's) of `steps` full-batch (D, G) pairs; shared, never modified"""
    case = Case(D=D, B=B, steps=steps, device_z=True, **({'d_hidden': d_hidden} if d_hidden else {}))
    return case, case.run_oracle(), case.run_oracle(mirror=True, quantize='bf16')


@functools.lru_cache(maxsize=None)
def lockstep_pairs(D, B, world, d_hidden=None, grad_dtype=None, paired=True, steps=2):
    """`steps` (D, G) pairs of W bf16 replicas with synchronised statistics through the lock-step DataParallel -- paired: train_pair
    (the pair hint: both generator segments in the D sub-step's one BN_STATS all-reduce), else disc_step + gen_step with no
    hint.  -> per rank (D weights, G weights, read_metrics); the replicas' weights are asserted bit-identical.  Shared, never modified."""
    case = _pairs_problem(D, B, d_hidden, steps)[0]
    kw = {'d_hidden': d_hidden} if d_hidden else {}
    ranks = [engine(D, B // world, E.BF16, flags=dp_flags(exact=True, grad_dtype=grad_dtype), rank=r, world=world, **kw) for r in range(world)]
    try:
        for e in ranks:
            load(e, case)
        dp = lockstep(ranks, exact=True)
        for t in range(steps):
            da, ga = rank_args(case, t, world)
            if paired:
                dp.train_pair(da, ga)
            else:
                dp.disc_step(da)
                dp.gen_step(ga)
        torch.cuda.synchronize()
        res = [(e.get_weights(E.NET_D), e.get_weights(E.NET_G), e.read_metrics(reset=False)) for e in ranks]
        assert all(e.get_iterations() == 2 * steps for e in ranks)
    finally:
        for e in ranks:
            e.close()
    _equal_on_all_ranks([d + g for d, g, _ in res], "weight")
    return res


def lockstep_pairs_match_mirror(D, B, world, d_hidden=None, steps=2):
    """(i) .. (iii) of the train_pair test: see tests/test_data_parallel_gpu.py"""
    case, ref, mir = _pairs_problem(D, B, d_hidden, steps)
    paired = lockstep_pairs(D, B, world, d_hidden, None, True, steps)           # (i) inside
    apart = lockstep_pairs(D, B, world, d_hidden, None, False, steps)
    # (ii) the paired generator pass is what the G sub-step would compute on its own
    for (d1, g1, m1), (d0, g0, m0) in zip(paired, apart):
        for i, (a, b) in enumerate(zip(d1 + g1, d0 + g0)):
            np.testing.assert_array_equal(a, b, err_msg="tensor %d: train_pair differs from disc_step + gen_step" % i)
        np.testing.assert_array_equal(np.asarray(m1), np.asarray(m0))
    # (iii) the rule of test_bf16_steps_match_bf16_mirror
    report = []
    for name, ws, wm, wr_, w0 in (("D", paired[0][0], mir['d'], ref['d'], case.d0), ("G", paired[0][1], mir['g'], ref['g'], case.g0)):
        for i, (w, wm_i, wr, wi) in enumerate(zip(ws, wm, wr_, w0)):
            report.append((name, i, update_rel_err(w, wm_i, wi), update_rel_err(w, wr, wi), update_rel_err(wm_i, wr, wi)))
    print("\nweights after %d pairs on %d ranks, error / update size: vs mirror | vs fp64 | mirror vs fp64\n  " % (steps, world) +
          "\n  ".join("%s%-2d %.3f %.3f %.3f" % r for r in report))
    for name, i, em, eo, emo in report:
        assert em < max(0.05, 0.9 * emo), (name, i, em, emo)
        assert eo < 0.5, (name, i, eo)


def phases_equal_whole_steps(D, B, exact, steps=2):
    """one bf16 rank: a FLAT_GRADS handle stepping through whole sub-steps against a dp_flags(exact) handle driven by
    dist.DataParallel -> per net, per tensor: update_rel_err of the phased weights against the whole-step ones, and whether
    they are bit-identical"""
    case = Case(D=D, B=B, steps=steps, device_z=True)
    plain = engine(D, B, E.BF16, flags=E.FLAG_FLAT_GRADS)
    phased = engine(D, B, E.BF16, flags=dp_flags(exact=exact))
    try:
        for e in (plain, phased):
            load(e, case)
        dp = DataParallel(EngineBackend(phased), exact=exact)
        for t in range(steps):
            da, ga = disc_args(case, t, device_z=True), gen_args(case, t, device_z=True)
            plain.disc_step(da, want_outputs=False)
            plain.gen_step(ga, want_outputs=False)
            dp.disc_step(da)
            dp.gen_step(ga)
        return [(net, i, update_rel_err(b, a, w0), bool(np.array_equal(a, b)))
                for net, w0s in ((E.NET_D, case.d0), (E.NET_G, case.g0))
                for i, (a, b, w0) in enumerate(zip(plain.get_weights(net), phased.get_weights(net), w0s))]
    finally:
        plain.close()
        phased.close()
