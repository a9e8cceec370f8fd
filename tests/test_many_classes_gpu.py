"""More than eight classes (class pitch 32): the scalar loss head in fp32 and bf16, the stand-alone matrix-core head in bf16,
prediction, evaluation, the supervised step and the data-parallel regions, against the same references and with the same
bounds as the six-class tests of test_gpu_parity.py.  The problems are built here: tests/helpers.Case draws six classes."""
import functools

import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests.helpers import SEED, Case, cosine, frob_rel_err, noise_set, rel_err, update_rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID_TWO_CHUNKS = (256, 256, 256, 256, 512)      # feature layer of 512 columns: two chunks of the matrix-core head


class KCase(Case):
    """Case with K classes: the discriminator's last dense from O.init_params(K=K), labels from 0 .. K-1 with class 8 and
    class K-1 present in every batch."""

    def __init__(self, K, D, B, steps=3, seed=7, dtype=np.float64, device_z=False, d_hidden=O.D_HIDDEN, g_hidden=O.G_HIDDEN):
        Case.__init__(self, D=D, B=B, steps=steps, seed=seed, dtype=dtype, device_z=device_z, d_hidden=d_hidden, g_hidden=g_hidden)
        rng = np.random.default_rng(seed + 1000 * K)
        g, d = O.init_params(D, seed=seed, dtype=dtype, g_hidden=self.g_hidden, d_hidden=self.d_hidden, K=K)
        self.g0 = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in g]
        self.d0 = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in d]
        self.labels = rng.integers(0, K, (steps, B)).astype(np.int32)
        self.labels[:, 0], self.labels[:, B - 1] = 8, K - 1
        self.K = K
        assert self.d0[-2].shape[1] == K and (self.labels >= 8).any() and (self.labels == K - 1).any()


def _engine(K, D, B, dtype, flags=0, rank=0, world=1, d_hidden=None, **cfg_kw):
    from mr_gan_amd import engine as E
    cfg = E.default_config(D, B)
    cfg.dtype, cfg.seed, cfg.flags, cfg.num_classes = dtype, SEED, flags, K
    cfg.rank, cfg.world = rank, world
    for i, w in enumerate(d_hidden or ()):
        cfg.d_hidden[i] = w
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    return E.Engine(cfg, DEV)


def _load(eng, case):
    from mr_gan_amd import engine as E
    eng.set_weights(E.NET_G, [p.astype(np.float32) for p in case.g0])
    eng.set_weights(E.NET_D, [p.astype(np.float32) for p in case.d0])


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _disc_args(case, t, device_z=False):
    from mr_gan_amd import engine as E
    return E.Engine.disc_args(_t(case.x_lab[t]), _t(case.labels[t], torch.int32), _t(case.x_unl[t]), None if device_z else _t(case.z1[t]))


def _gen_args(case, t, device_z=False):
    from mr_gan_amd import engine as E
    return E.Engine.gen_args(_t(case.x_unl2[t]), None if device_z else _t(case.z2[t]))


# ---------------------------------------------------------------------------------------------------------
# 1. create
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("K", [9, 10, 32])
def test_create_above_eight_classes(K, dtype):
    from mr_gan_amd import engine as E
    eng = _engine(K, 16, 50, dtype)
    assert eng.full_shape(E.NET_D, 10) == (250, K) and eng.full_shape(E.NET_D, 11) == (K,)
    eng.close()


def test_create_refuses_what_is_not_built():
    from mr_gan_amd import engine as E
    with pytest.raises(E.MrganError, match=r"\[2,32\]"):
        _engine(33, 16, 50, 0)
    with pytest.raises(E.MrganError, match=r"\[2,32\]"):
        _engine(33, 16, 50, 1)
    with pytest.raises(E.MrganError, match="fp8 engine supports at most 8 classes"):
        _engine(9, 128, 64, E.FP8)


@pytest.mark.parametrize("K", [6, 8])
def test_workspace_of_the_eight_class_pitch_is_unchanged(K):
    """mrgan_workspace_bytes of the commit before the 32-class pitch, pinned"""
    import ctypes as C
    from mr_gan_amd import engine as E
    for (D, B, dtype, hid), want in (((400, 50, E.BF16, None), 49338624), ((16, 50, E.F32, None), 34548224),
                                     ((512, 1024, E.BF16, (4096,) * 5), 1976676096)):
        cfg = E.default_config(D, B)
        cfg.dtype, cfg.num_classes = dtype, K
        for i, w in enumerate(hid or ()):
            cfg.d_hidden[i] = w
        n = C.c_size_t(0)
        assert E.load_library().mrgan_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
        assert n.value == want, (D, B, dtype, n.value, want)


# ---------------------------------------------------------------------------------------------------------
# 2. fp32 against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------
FP32_CASES = [(K, D, B) for K in (9, 10, 32) for D, B in ((16, 50), (72, 132))]


@functools.lru_cache(maxsize=None)
def _fp32_case(K, D, B):
    case = KCase(K, D, B, steps=3)
    return case, case.run_oracle(), KCase(K, D, B, steps=3, dtype=np.float32).run_oracle()


@pytest.mark.parametrize("K,D,B", FP32_CASES)
def test_fp32_gradients_match_oracle(K, D, B):
    """bounds of test_gpu_parity.test_fp32_gradients_match_oracle"""
    from mr_gan_amd import engine as E
    case = _fp32_case(K, D, B)[0]
    orc = O.MRGANOracle(case.g0, case.d0)
    (ll, lu, err), gd, _ = orc.disc_grads(**case.disc_inputs(0, 0))
    eng = _engine(K, D, B, 0, flags=E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS)
    _load(eng, case)
    da = _disc_args(case, 0)
    eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
    got = eng.get_slot(E.NET_D, 2)
    assert got[10].shape == (250, K)
    for i, (a, b) in enumerate(zip(got, gd)):
        assert rel_err(a, b) < 2e-5, ("dD", i, rel_err(a, b))
    out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
    np.testing.assert_allclose(out, (ll, lu, err), rtol=2e-4, atol=2e-5)
    orc.adam.apply(orc.d, gd, 'd')
    loss, gg, _ = orc.gen_grads(**case.gen_inputs(0, 1))
    ga = _gen_args(case, 0)
    eng.gen_step(ga, E.G_GEN, E.G_TAIL, want_outputs=False)
    got = eng.get_slot(E.NET_G, 2)
    for i, (a, b) in enumerate(zip(got, gg)):
        assert rel_err(a, b) < 2e-4, ("dG", i, rel_err(a, b))
    assert abs(eng.gen_step(ga, E.G_ADAM, E.G_ADAM) - loss) < 2e-3 * abs(loss) + 1e-9
    eng.close()


@pytest.mark.parametrize("K,D,B", FP32_CASES)
def test_fp32_steps_match_oracle(K, D, B):
    """weights and the iteration count after three (D, G) pairs: bounds of test_gpu_parity.test_fp32_steps_match_oracle"""
    from mr_gan_amd import engine as E
    case, ref, r32 = _fp32_case(K, D, B)
    eng = _engine(K, D, B, 0)
    _load(eng, case)
    assert rel_err(eng.predict_logits(_t(case.probe)).cpu().numpy(), ref['logits0']) < 1e-5
    for t in range(case.steps):
        got_d = eng.disc_step(_disc_args(case, t))
        got_g = eng.gen_step(_gen_args(case, t))
        dev = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(r32['disc'][t][:2], ref['disc'][t][:2]))
        np.testing.assert_allclose(got_d[:2], ref['disc'][t][:2], rtol=2e-4 if t == 0 else max(2e-4, 3 * dev), atol=2e-5)
        assert abs(got_d[2] - ref['disc'][t][2]) <= (1e-6 if t == 0 else 1.01 / B)
        dev = abs(r32['gen'][t] - ref['gen'][t]) / abs(ref['gen'][t])
        np.testing.assert_allclose(got_g, ref['gen'][t], rtol=max(2e-3, 3 * dev), atol=1e-9)
    for net, key, w0s in ((E.NET_D, 'd', case.d0), (E.NET_G, 'g', case.g0)):
        for i, (w, wr, w0, w32) in enumerate(zip(eng.get_weights(net), ref[key], w0s, r32[key])):
            e, e32 = update_rel_err(w, wr, w0), update_rel_err(w32, wr, w0)
            assert e < max(0.02, 3 * e32), (key, i, e, e32)
    e32 = rel_err(r32['logits'], ref['logits'])
    got = eng.predict_logits(_t(case.probe)).cpu().numpy()
    assert rel_err(got, ref['logits']) < max(1e-3, 2.0 * e32), (rel_err(got, ref['logits']), e32)
    assert eng.get_iterations() == 2 * case.steps
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 3. bf16 against the bf16 mirror
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,B,hid", [(10, 400, 50, None), (32, 400, 50, None),       # one ragged 64-row block, Fp = 256 in a single chunk
                                       (10, 96, 130, None), (32, 96, 130, None),       # three blocks, the last one with 2 valid rows
                                       (10, 96, 130, HID_TWO_CHUNKS)])                 # two chunks: pass 2 walks them back
def test_bf16_gradients_match_bf16_mirror(K, D, B, hid):
    """rule and constants of test_gpu_parity.test_bf16_gradients_match_bf16_mirror: err(engine, mirror) <
    max(3e-3, 0.6 err(mirror, fp64)) per tensor, losses to 5e-4, and the labelled direction check against fp64"""
    from mr_gan_amd import engine as E
    tol, tol_loss, frac, loose = 3e-3, 5e-4, 0.6, (0.995, 0.98, 0.25)
    kw = dict(d_hidden=hid) if hid else {}
    case = KCase(K, D, B, steps=1, **kw)
    mir = O.MRGANMirror(case.g0, case.d0, quantize='bf16')
    orc = O.MRGANOracle(case.g0, case.d0)
    (ll, lu, err), gd_m, _ = mir.disc_grads(**case.disc_inputs(0, 0))
    (ll_o, lu_o, _), gd_o, _ = orc.disc_grads(**case.disc_inputs(0, 0))
    eng = _engine(K, D, B, 1, flags=E.FLAG_FLAT_GRADS, **kw)
    _load(eng, case)
    # an evaluation first: it fills all rows of the activation buffers, which the training step afterwards must tolerate
    rs = np.random.RandomState(5)
    eng.eval_error(_t(rs.randn(3 * 128 + 7, D).astype(np.float32)), _t(rs.randint(0, K, size=3 * 128 + 7), torch.int32))
    da = _disc_args(case, 0)
    eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
    report = []

    def check(name, got, want_m, want_o, cos_min):
        for i, (a, m, o) in enumerate(zip(got, want_m, want_o)):
            em, eo, emo = frob_rel_err(a, m), frob_rel_err(a, o), frob_rel_err(m, o)
            report.append("%s%-2d %.1e %.1e %.1e" % (name, i, em, eo, emo))
            assert em < max(tol, frac * emo), (name + " vs mirror", i, em, emo)
            assert cosine(a, o) > cos_min and eo < loose[2], (name + " vs fp64", i, cosine(a, o), eo)

    try:
        check("dD", eng.get_slot(E.NET_D, 2), gd_m, gd_o, loose[0])
        out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
        for got_l, m_l, o_l in zip(out[:2], (ll, lu), (ll_o, lu_o)):
            np.testing.assert_allclose(got_l, m_l, rtol=max(tol_loss, frac * abs(m_l - o_l) / max(abs(o_l), 1e-12)), atol=tol_loss * 0.1)
        assert abs(out[2] - err) <= 1.01 / B
        # the G sub-step sees the D network after its update: give engine, mirror and oracle the same updated weights
        mir.adam.apply(mir.d, gd_m, 'd')
        orc.d = [p.copy() for p in mir.d]
        orc.adam.iterations = 1
        eng.set_weights(E.NET_D, [p.astype(np.float32) for p in mir.d])
        loss, gg_m, _ = mir.gen_grads(**case.gen_inputs(0, 1))
        _, gg_o, _ = orc.gen_grads(**case.gen_inputs(0, 1))
        ga = _gen_args(case, 0)
        eng.gen_step(ga, E.G_GEN, E.G_TAIL, want_outputs=False)
        check("dG", eng.get_slot(E.NET_G, 2), gg_m, gg_o, loose[1])
        lg = eng.gen_step(ga, E.G_ADAM, E.G_ADAM)
        assert abs(lg - loss) < 5 * tol_loss * abs(loss) + 1e-12, (lg, loss)
    finally:
        eng.close()
        print("\n(K=%d, D=%d, B=%d) tensor: err vs mirror | vs fp64 | mirror vs fp64\n  " % (K, D, B) + "\n  ".join(report))


# ---------------------------------------------------------------------------------------------------------
# 4. matrix-core head against scalar head at the 32-class pitch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 32])
def test_matrix_core_loss_head_equals_scalar_head(K):
    """comparisons and bounds of test_gpu_parity.test_matrix_core_loss_head_equals_scalar_head for bf16; B = 200: a ragged last
    row block (8 valid rows), a 512-column feature layer (two chunks)"""
    from mr_gan_amd import engine as E
    D, B, hid = 96, 200, (256, 256, 256, 512, 512)
    case = KCase(K, D, B, steps=1, device_z=True, d_hidden=hid)
    res = []
    for mfma in (1, 0):
        eng = _engine(K, D, B, 1, flags=E.FLAG_FLAT_GRADS, d_hidden=hid)
        eng.set_tuning(E.TUNE_HEAD_MFMA, mfma)
        _load(eng, case)
        da = _disc_args(case, 0, device_z=True)
        eng.profile_begin()
        eng.disc_step(da, E.D_GEN, E.D_MAIN, want_outputs=False)
        names = set(eng.profile_end())
        assert ("head_wide_kernel" in names) == bool(mfma) and ("head_kernel" in names) != bool(mfma), names
        assert "chain_kernel<0>" not in names
        gd = eng.get_slot(E.NET_D, 2)
        dpre = eng.debug_buffer(1, 4).cpu().numpy()[:, :B]
        out = eng.disc_step(da, E.D_ADAM, E.D_ADAM)
        res.append((gd, out, dpre))
        eng.close()
    (gd1, out1, dp1), (gd0, out0, dp0) = res
    np.testing.assert_allclose(out1, out0, rtol=1e-6, atol=1e-7)
    d = np.abs(dp1 - dp0)
    print("\nK=%d: max |d dpre| %.3e of %.3e, rows that differ %.4f, dD %s"
          % (K, d.max(), np.abs(dp0).max(), (d.max(axis=2) > 0).mean(), " ".join("%.1e" % rel_err(a, b) for a, b in zip(gd1, gd0))))
    assert d.max() <= 2.0 ** -7 * np.abs(dp0).max() and (d.max(axis=2) > 0).mean() < 0.05, (d.max(), (d.max(axis=2) > 0).mean())
    for i, (a, b) in enumerate(zip(gd1, gd0)):
        assert rel_err(a, b) < 5e-4, ("dD", i, rel_err(a, b))


# ---------------------------------------------------------------------------------------------------------
# 5. prediction and evaluation
# ---------------------------------------------------------------------------------------------------------
def test_predict_and_eval_at_ten_classes():
    from mr_gan_amd import engine as E
    K, D, B, n = 10, 48, 50, 77
    case = KCase(K, D, B, steps=1)
    rng = np.random.default_rng(3)
    # planted: classes 8 and 9 carry the largest weights, so they win on a good share of the rows
    case.d0[-2][:, 8:] *= 4.0
    x = rng.standard_normal((n, D)).astype(np.float32)
    y = rng.integers(0, K, n).astype(np.int32)
    want = O.MRGANOracle(case.g0, case.d0).predict_logits(x.astype(np.float64))
    am = np.argmax(want, axis=1)
    assert (am == 8).any() and (am == 9).any()
    eng = _engine(K, D, B, 0)
    _load(eng, case)
    got = eng.predict_logits(_t(x)).cpu().numpy()
    assert got.shape == (n, K)
    assert rel_err(got, want) < 1e-5, rel_err(got, want)            # a wrong copy pitch shifts every row but the first
    assert eng.eval_error(_t(x), _t(y, torch.int32)) == pytest.approx(float(np.mean(am != y)), abs=1e-7)
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 6. supervised step
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,B,short", [(0, 48, 20, 7), (1, 72, 50, 33)])
def test_supervised_steps_match_oracle(dtype, D, B, short):
    """bounds of test_gpu_parity.test_supervised_steps_match_oracle, ten classes"""
    from mr_gan_amd import engine as E
    K = 10
    case = KCase(K, D, B, steps=3)
    kw = dict(lr=O.NN_ADAM_LR, b1=O.NN_ADAM_B1)
    ref = O.MRGANOracle(case.g0, case.d0, **kw)
    mir = O.MRGANMirror(case.g0, case.d0, quantize='bf16' if dtype else None, **kw)
    eng = _engine(K, D, B, dtype, lr=O.NN_ADAM_LR, beta1=O.NN_ADAM_B1)
    _load(eng, case)
    for t in range(case.steps):
        n = short if t == 1 else B
        x, y = case.x_lab[t].astype(np.float64), case.labels[t]
        noise = [m[:n] for m in noise_set(SEED, 0, t, B, D)]
        yb = y.copy()
        yb[n:] = -1
        got = eng.sup_step(E.Engine.sup_args(_t(case.x_lab[t]), _t(yb, torch.int32), rows_valid=0 if n == B else n))
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


def test_nn_baseline_runs_an_epoch_at_ten_classes():
    from mr_gan_amd.mr_nn import MRNN
    rng = np.random.default_rng(5)
    y = np.repeat(np.arange(10), 9).astype(np.int32)                # 90 rows: 4 batches of 20 + one of 10
    x = rng.standard_normal((len(y), 40)).astype(np.float32)
    model = MRNN(40, seed=3, num_classes=10)
    hist = model.fit(x, y, epochs=1, rng=np.random.RandomState(1))
    assert model.engine.get_iterations() == 5 and np.isfinite(hist[-1]['loss'])
    assert model.predict_logits(x).shape == (90, 10)
    model.engine.close()


# ---------------------------------------------------------------------------------------------------------
# 7. reproducibility, 8. padding invariant
# ---------------------------------------------------------------------------------------------------------
def _three_pairs(eng, case):
    for t in range(case.steps):
        eng.disc_step(_disc_args(case, t, device_z=True), want_outputs=False)
        eng.gen_step(_gen_args(case, t, device_z=True), want_outputs=False)


def test_substeps_are_bit_reproducible():
    """bf16, ten classes, (400, 50): the same three pairs from the same state on two fresh handles, every weight, every Adam slot
    and every stored activation / gradient identical bit for bit (the two-round fold of the logits tiles has a fixed order)"""
    from mr_gan_amd import engine as E
    K, D, B = 10, 400, 50
    case = KCase(K, D, B, steps=3, device_z=True)
    ref = None
    for rep in range(2):
        eng = _engine(K, D, B, 1)
        _load(eng, case)
        _three_pairs(eng, case)
        cur = eng.get_weights(E.NET_D) + eng.get_weights(E.NET_G) + eng.get_slot(E.NET_D, 0) + eng.get_slot(E.NET_D, 1)
        cur += [eng.debug_buffer(0, l, 2).cpu().numpy() for l in range(5)] + [eng.debug_buffer(1, l, 1).cpu().numpy() for l in range(5)]
        cur.append(eng.debug_buffer(2, 0, 2).cpu().numpy())
        eng.close()
        if ref is None:
            ref = cur
        else:
            for i, (a, b) in enumerate(zip(cur, ref)):
                np.testing.assert_array_equal(a, b, err_msg="tensor %d differs between run %d and run 0" % (i, rep))


def test_pitch_and_padding_columns_play_no_part():
    from mr_gan_amd import engine as E
    K, D, B = 10, 400, 50
    case = KCase(K, D, B, steps=3, device_z=True)
    eng = _engine(K, D, B, 1)
    _load(eng, case)
    _three_pairs(eng, case)
    wd, wg = eng.get_weights(E.NET_D), eng.get_weights(E.NET_G)
    assert wd[10].shape == (250, K) and wd[11].shape == (K,)
    eng.set_weights(E.NET_D, wd)
    for a, b in zip(eng.get_weights(E.NET_D), wd):
        np.testing.assert_array_equal(a, b)
    logits = eng.predict_logits(_t(case.probe)).cpu().numpy()

    def widen(ts):
        ts = [t.copy() for t in ts]
        w6, b6 = np.zeros((250, 32), np.float32), np.zeros(32, np.float32)
        w6[:, :K], b6[:K] = ts[10], ts[11]
        ts[10], ts[11] = w6, b6
        return ts

    big = _engine(32, D, B, 1)
    big.set_weights(E.NET_G, wg)
    big.set_weights(E.NET_D, widen(wd))
    for slot in (0, 1):
        big.set_slot(E.NET_D, slot, widen(eng.get_slot(E.NET_D, slot)))
    got = big.predict_logits(_t(case.probe)).cpu().numpy()
    np.testing.assert_array_equal(got[:, :K], logits)
    np.testing.assert_array_equal(got[:, K:], np.zeros_like(got[:, K:]))
    eng.close()
    big.close()


# ---------------------------------------------------------------------------------------------------------
# 9. data parallel: the region sizes depend on the pitch
# ---------------------------------------------------------------------------------------------------------
def test_two_rank_emulation_equals_full_batch():
    """test_gpu_parity.test_two_rank_emulation_equals_full_batch at ten classes, same bounds"""
    from mr_gan_amd import engine as E
    K, B, D = 10, 64, 32
    case = KCase(K, D, B, steps=2, device_z=True)
    ref = case.run_oracle()
    flags = E.FLAG_FLAT_GRADS | E.FLAG_SYNC_STATS
    ranks = [_engine(K, D, B // 2, 0, flags=flags, rank=r, world=2) for r in range(2)]
    for e in ranks:
        _load(e, case)

    def allreduce(region):
        views = [e.region(region) for e in ranks]
        tot = views[0] + views[1]
        for v in views:
            v.copy_(tot)

    h = B // 2
    for t in range(case.steps):
        da = [E.Engine.disc_args(_t(case.x_lab[t][r * h:(r + 1) * h]), _t(case.labels[t][r * h:(r + 1) * h], torch.int32),
                                 _t(case.x_unl[t][r * h:(r + 1) * h])) for r in range(2)]
        for e, a in zip(ranks, da):
            e.disc_step(a, E.D_GEN, E.D_GEN, want_outputs=False)
        allreduce(E.REGION_BN_STATS)
        for e, a in zip(ranks, da):
            e.disc_step(a, E.D_MAIN, E.D_MAIN, want_outputs=False)
        allreduce(E.REGION_GRAD_D)
        outs = [e.disc_step(a, E.D_ADAM, E.D_ADAM) for e, a in zip(ranks, da)]
        np.testing.assert_allclose(outs[0], ref['disc'][t], rtol=3e-4, atol=3e-5)
        np.testing.assert_allclose(outs[1], outs[0], rtol=0, atol=0)
        ga = [E.Engine.gen_args(_t(case.x_unl2[t][r * h:(r + 1) * h])) for r in range(2)]
        for ph, reg in ((E.G_GEN, E.REGION_BN_STATS), (E.G_FEAT, E.REGION_FM_MOMENTS), (E.G_BWD, E.REGION_BN_BWD),
                        (E.G_TAIL, E.REGION_GRAD_G)):
            for e, a in zip(ranks, ga):
                e.gen_step(a, ph, ph, want_outputs=False)
            allreduce(reg)
        outs = [e.gen_step(a, E.G_ADAM, E.G_ADAM) for e, a in zip(ranks, ga)]
        np.testing.assert_allclose(outs[0], ref['gen'][t], rtol=3e-3, atol=1e-9)
    w0, w1 = ranks[0].get_weights(E.NET_D), ranks[1].get_weights(E.NET_D)
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)                    # replicas stay bit-identical
    for i, (w, wr, wi) in enumerate(zip(w0, ref['d'], case.d0)):
        assert update_rel_err(w, wr, wi) < 0.05, ("D", i)
    for e in ranks:
        e.close()


# ---------------------------------------------------------------------------------------------------------
# 10. the default path is untouched
# ---------------------------------------------------------------------------------------------------------
def test_default_path_is_untouched():
    """two six-class bf16 handles at (400, 50), the second created after a ten-class handle has trained on the same device: the
    same weights bit for bit after three train_pair steps, the same kernels, the D-tail chain among them"""
    from mr_gan_amd import engine as E
    D, B = 400, 50
    case = Case(D=D, B=B, steps=3, device_z=True)

    def run():
        eng = _engine(6, D, B, 1)
        _load(eng, case)
        xl, yl, xu, xu2 = (_t(case.x_lab.reshape(-1, D)), _t(case.labels.reshape(-1), torch.int32), _t(case.x_unl.reshape(-1, D)),
                           _t(case.x_unl2.reshape(-1, D)))
        eng.set_iterations(0, 0)
        da, ga = E.Engine.disc_args(xl, yl, xu, stream_mode=1), E.Engine.gen_args(xu2, stream_mode=1)
        eng.profile_begin()
        for _ in range(case.steps):
            eng.train_pair(da, ga)
        prof = eng.profile_end()
        w = eng.get_weights(E.NET_D) + eng.get_weights(E.NET_G)
        eng.close()
        return w, {k: v[1] for k, v in prof.items()}

    w_a, names_a = run()
    ten = KCase(10, D, B, steps=3, device_z=True)
    eng = _engine(10, D, B, 1)
    _load(eng, ten)
    eng.profile_begin()
    _three_pairs(eng, ten)
    names_ten = set(eng.profile_end())
    eng.close()
    w_b, names_b = run()
    for a, b in zip(w_a, w_b):
        np.testing.assert_array_equal(a, b)
    assert names_a == names_b and "chain_kernel<0>" in names_a and "head_wide_kernel" not in names_a, (names_a, names_b)
    # the ten-class handle: per-layer D tail + the stand-alone matrix-core head; the G sub-step's two chains stay on
    assert "chain_kernel<0>" not in names_ten and {"head_wide_kernel", "chain_kernel<1>", "chain_kernel<2>"} <= names_ten, names_ten
