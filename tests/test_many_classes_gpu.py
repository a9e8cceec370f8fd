"""More than eight classes (class pitch 32): the scalar loss head in fp32 and bf16, the stand-alone matrix-core head in bf16,
prediction, evaluation, the supervised step and the data-parallel regions.  The step-level tests are the bodies of
tests/parity.py on the variant P.classes(K): the same references and bounds as for six classes; tests.helpers.Case(K=K)
builds the problems."""
import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests import parity as P
from tests.helpers import Case, rel_err

pytestmark = pytest.mark.gpu

HID_TWO_CHUNKS = (256, 256, 256, 256, 512)      # feature layer of 512 columns: two chunks of the matrix-core head
_load, _t, _disc_args, _gen_args = P.load, P.to_dev, P.disc_args, P.gen_args


def KCase(K, D, B, **kw):
    return Case(K=K, D=D, B=B, **kw)


def _engine(K, D, B, dtype, **kw):
    return P.engine(D, B, dtype, num_classes=K, **kw)


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


@pytest.mark.parametrize("K,D,B", FP32_CASES)
def test_fp32_gradients_match_oracle(K, D, B):
    got = P.fp32_gradients_match_oracle(P.classes(K), D, B, steps=3)
    assert got[10].shape == (250, K)


@pytest.mark.parametrize("K,D,B", FP32_CASES)
def test_fp32_steps_match_oracle(K, D, B):
    """weights and the iteration count after three (D, G) pairs"""
    P.fp32_steps_match_oracle(P.classes(K), D, B)


# ---------------------------------------------------------------------------------------------------------
# 3. bf16 against the bf16 mirror
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,B,hid", [(10, 400, 50, None), (32, 400, 50, None),       # one ragged 64-row block, Fp = 256 in a single chunk
                                       (10, 96, 130, None), (32, 96, 130, None),       # three blocks, the last one with 2 valid rows
                                       (10, 96, 130, HID_TWO_CHUNKS)])                 # two chunks: pass 2 walks them back
def test_bf16_gradients_match_bf16_mirror(K, D, B, hid):
    P.grad_parity(P.classes(K), D, B, 1, 'bf16', tol=3e-3, tol_loss=5e-4, d_hidden=hid)


# ---------------------------------------------------------------------------------------------------------
# 4. matrix-core head against scalar head at the 32-class pitch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 32])
def test_matrix_core_loss_head_equals_scalar_head(K):
    """bf16; B = 200: a ragged last row block (8 valid rows), a 512-column feature layer (two chunks).  Also checked: which head
    kernel ran"""
    P.matrix_core_loss_head_equals_scalar_head(P.classes(K), 1, 200, kernel_names=True)


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
    P.supervised_steps_match_oracle(P.classes(10), dtype, D, B, short)


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
    P.two_rank_emulation_equals_full_batch(P.classes(10))


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
