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


def phase_walk(ranks, da, ga, allreduce):
    """One (D, G) pair through the data-parallel phases (mr_gan_amd/dist.py): every phase on every rank, then the all-reduce
    of the region it produced, then the Adam phase.  -> (the D outputs per rank, the G loss per rank)"""
    for ph, reg in ((E.D_GEN, E.REGION_BN_STATS), (E.D_MAIN, E.REGION_GRAD_D)):
        for e, a in zip(ranks, da):
            e.disc_step(a, ph, ph, want_outputs=False)
        allreduce(reg)
    d_out = [e.disc_step(a, E.D_ADAM, E.D_ADAM) for e, a in zip(ranks, da)]
    for ph, reg in ((E.G_GEN, E.REGION_BN_STATS), (E.G_FEAT, E.REGION_FM_MOMENTS), (E.G_BWD, E.REGION_BN_BWD), (E.G_TAIL, E.REGION_GRAD_G)):
        for e, a in zip(ranks, ga):
            e.gen_step(a, ph, ph, want_outputs=False)
        allreduce(reg)
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
