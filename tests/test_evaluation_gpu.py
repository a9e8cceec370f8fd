"""mrgan_predict_logits and mrgan_eval_error on the GPU: the host routine that every reported number of the project comes out of
(eval_rows, engine.hip -- chunks of 3 S rows through the training activations) on fp32, bf16 and fp8 handles, against the
references of tests/evaluation_ref.py, at the chunk edges, through gathers and pitches, under every forward tile, with the
current weights, and without a trace in the training state."""
import ctypes as C

import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from tests import evaluation_ref as R
from tests import parity as P
from tests import saliency_gpu as G
from tests.helpers import Case, rel_err

pytestmark = pytest.mark.gpu

QUANT = {E.F32: None, E.BF16: 'bf16', E.FP8: 'fp8'}
DTYPE_NAME = {E.F32: 'fp32', E.BF16: 'bf16', E.FP8: 'fp8'}
CASES = [(name, dt) for name in R.PROBLEMS for dt in (E.F32, E.BF16, E.FP8) if not (name == 'k10' and dt == E.FP8)]
case_ids = ["%s-%s" % (name, DTYPE_NAME[dt]) for name, dt in CASES]
N_NAN = 3 * R.S + 7                   # NaN rows of the disturbances: two chunks, every padding row of every segment
SENT = G.SENT


def _engine(name, dtype, weights=None):
    kw = dict(d_hidden=R.d_hidden(name)) if R.d_hidden(name) else {}
    eng = P.engine(R.D, R.B, dtype, num_classes=R.classes(name), **kw)
    P.load(eng, R.problem(name))
    if weights is not None:
        eng.set_weights(E.NET_D, weights)
    return eng


def _logits(eng, x, idx=None):
    out = eng.predict_logits(x, None if idx is None else P.to_dev(idx, torch.int32))
    return out.cpu().numpy()


def _error(eng, x, y, idx=None):
    return eng.eval_error(x, P.to_dev(y, torch.int32), None if idx is None else P.to_dev(idx, torch.int32))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(G.bits(a), G.bits(b))


def _offset_rows(x32):
    """the rows on the device with pitch D + 4 (a multiple of 16 bytes), the first element one float behind a 16-byte boundary,
    NaN around every row"""
    n, D = x32.shape
    buf = torch.full((n * (D + 4) + 4,), float("nan"), device=P.DEV)
    off = 1 + (-(buf.data_ptr() // 4)) % 4
    view = buf[off:off + n * (D + 4)].view(n, D + 4)[:, :D]
    view.copy_(P.to_dev(x32))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == D + 4
    return view


# ---- 1. logits against the reference, whole set ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASES, ids=case_ids)
def test_logits_match_the_reference_on_the_whole_set(name, dtype):
    """fp32: within 1e-5 of fp64 (the bound of parity.fp32_steps_match_oracle).  bf16 and fp8: within max(2e-3, 0.6 err(mirror,
    fp64)) of the mirror (test_bf16_steps_match_bf16_mirror's 2e-3, grad_parity's 0.6), and loosely within 3e-2 of fp64."""
    eng = _engine(name, dtype)
    got = _logits(eng, P.to_dev(R.rows()))
    eng.close()
    ref, quant = R.reference(name), QUANT[dtype]
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    eo = rel_err(got, ref)
    if quant is None:
        print("%s fp32: engine-fp64 %.2e" % (name, eo))
        assert eo < R.FP32_TOL, eo
        return
    mir = R.reference(name, quant)
    em, emo = rel_err(got, mir), rel_err(mir, ref)
    print("%s %s: engine-mirror %.2e engine-fp64 %.2e mirror-fp64 %.2e" % (name, quant, em, eo, emo))
    assert em < max(R.BF16_TOL, R.MIRROR_FRAC * emo), (em, emo)
    assert eo < R.LOOSE_TOL, eo


# ---- 2. a row's logits do not depend on where the row sits ----------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASES, ids=case_ids)
def test_logits_do_not_depend_on_the_position_of_a_row(name, dtype):
    """Bit for bit.  Every output element of a forward product accumulates its k-steps in the same order on every tile
    (test_forced_kc_tiles_equal_the_measured_table; launch_gemm_f32 for its two tiles), the evaluation forward has no batch
    statistics, and head_kernel reduces each row over a fixed lane pattern: the chunk a row falls into, its offset there, the M
    of the launch and the tile the table picks for it cannot show."""
    X, K = R.rows(), R.classes(name)
    eng = _engine(name, dtype)
    xd = P.to_dev(X)
    L = _logits(eng, xd)
    for n in R.PREFIXES:
        assert _same(_logits(eng, xd[:n]), L[:n]), ("prefix", n)
    for n in R.SUFFIXES:
        assert _same(_logits(eng, xd[R.N - n:]), L[-n:]), ("suffix", n)
    # gathered from a source of odd pitch (stage_kernel's scalar loads), NaN behind every row: three chunks with repeats
    idx = R.gather_index()
    assert _same(_logits(eng, G.wide_rows(X), idx), L[idx]), "gather"
    assert _same(_logits(eng, _offset_rows(X)), L), "offset source"
    # the entry itself: nothing behind the n K logits is written
    out = torch.full((R.N * K + 64,), SENT, device=P.DEV)
    rc = eng.lib.mrgan_predict_logits(eng.handle, C.c_void_p(xd.data_ptr()), None, C.c_int64(R.D), C.c_int64(R.N), C.c_void_p(out.data_ptr()),
                                      E._stream())
    raw = out.cpu().numpy()
    eng.close()
    assert rc == 0
    assert _same(raw[:R.N * K].reshape(R.N, K), L), "raw entry"
    assert (raw[R.N * K:] == SENT).all()


# ---- 3. the error is the count of the engine's own wrong rows ------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASES, ids=case_ids)
def test_error_is_the_count_of_the_engines_wrong_rows(name, dtype):
    """exactly: the label offset of the later chunks, the count per 32-row block and the atomic sum.  Against the reference:
    the engine's class is the reference's on every decided row, so the counts differ by at most the undecided rows."""
    X, y, quant = R.rows(), R.labels(name), QUANT[dtype]
    ref, und = R.reference(name, quant), R.undecided(name, quant)
    eng = _engine(name, dtype)
    xd = P.to_dev(X)
    L = _logits(eng, xd)
    cls = R.argmax_first(L)
    assert np.array_equal(cls[~und], R.argmax_first(ref)[~und])
    idx = R.gather_index()
    wide = G.wide_rows(X)
    forms = [(xd[:n], np.arange(n), None) for n in R.PREFIXES] + [(wide, idx, idx)]
    report = []
    for x, sel, gather in forms:
        n = len(sel)
        cnt, cnt_ref = int(np.sum(cls[sel] != y[sel])), R.error_count(ref[sel], y[sel])
        got = _error(eng, x, y[sel], gather)
        report.append((n, cnt, cnt_ref, int(und[sel].sum())))
        assert got == float(np.float32(cnt / n)), (n, got, cnt)
        assert abs(cnt - cnt_ref) <= int(und[sel].sum()), (n, cnt, cnt_ref)
    assert _same(_logits(eng, xd), L)                         # (and the logits after the counting calls are the logits before)
    eng.close()
    print("%s %s (n, wrong rows, the reference's, undecided):" % (name, DTYPE_NAME[dtype]), report)


# ---- 4. forced block tiles -----------------------------------------------------------------------------------------------
def test_forced_forward_tiles_give_the_same_bits():
    """every forward tile MRGAN_TUNE_KC_CFG accepts on 385 rows of a bf16 handle (a chunk of 384 rows: one and a half 256-row
    tiles; a chunk of one row), against the measured table's choice; forced 7 and forced 3 do run the 128 x 128 and the 256 x 256
    instantiation on every layer whose width allows it (gemm_bf16.hip: launch_kc_tile)"""
    n = R.CHUNK + 1
    eng = _engine('stock', E.BF16)
    xd = P.to_dev(R.rows()[:n])
    want = _logits(eng, xd)
    widths = [-(-w // 64) * 64 for w in R.problem('stock').d_hidden]
    for cfg in (0, 1, 3, 5, 7, 9):
        eng.set_tuning(E.TUNE_KC_CFG, cfg)
        assert _same(_logits(eng, xd), want), cfg
        if cfg in (3, 7):
            tile, need = {3: ("256, 256", 256), 7: ("128, 128", 128)}[cfg]
            eng.profile_begin()
            got = _logits(eng, xd)
            prof = eng.profile_end()
            print(cfg, sorted((k, v[1]) for k, v in prof.items()))
            assert _same(got, want), cfg
            allowed = sum(1 for w in widths if w % need == 0)
            assert allowed > 0
            assert sum(v[1] for k, v in prof.items() if k.startswith("gemm_bf16_kc_kernel<") and ", %s," % tile in k) == 2 * allowed
    eng.set_tuning(E.TUNE_KC_CFG, -1)
    assert _same(_logits(eng, xd), want)
    eng.close()


# ---- 5. evaluation sees the current weights --------------------------------------------------------------------------------
def _other_weights():
    return [p.astype(np.float32) for p in Case(D=R.D, B=R.B, steps=1, seed=8).d0]


@pytest.mark.parametrize("dtype", [E.BF16, E.FP8], ids=["bf16", "fp8"])
def test_evaluation_after_set_weights_is_a_fresh_handles(dtype):
    X, y = R.rows(), R.labels('stock')
    xd, yd = P.to_dev(X), P.to_dev(y, torch.int32)
    eng = _engine('stock', dtype)
    before, err_before = _logits(eng, xd), eng.eval_error(xd, yd)
    eng.set_weights(E.NET_D, _other_weights())
    after, err_after = _logits(eng, xd), eng.eval_error(xd, yd)
    eng.close()
    fresh = _engine('stock', dtype, _other_weights())
    want, err_want = _logits(fresh, xd), fresh.eval_error(xd, yd)
    fresh.close()
    assert not np.array_equal(before, after) and err_before != err_after
    assert _same(after, want) and err_after == err_want


@pytest.mark.parametrize("dtype", [E.BF16, E.FP8], ids=["bf16", "fp8"])
def test_evaluation_after_training_is_a_fresh_handles(dtype):
    """two (D, G) pairs with device-drawn z: the bf16 weight copies the evaluation reads are those Adam refreshed, i.e. the
    roundings of the fp32 weights get_weights returns"""
    case = Case(D=R.D, B=R.B, steps=2, device_z=True)
    xd = P.to_dev(R.rows()[:R.CHUNK + 1])
    eng = P.engine(R.D, R.B, dtype)
    P.load(eng, case)
    before = _logits(eng, xd)
    for t in range(case.steps):
        eng.disc_step(P.disc_args(case, t, True))
        eng.gen_step(P.gen_args(case, t, True))
    after = _logits(eng, xd)
    trained = eng.get_weights(E.NET_D)
    eng.close()
    fresh = P.engine(R.D, R.B, dtype)
    P.load(fresh, case)
    fresh.set_weights(E.NET_D, trained)
    want = _logits(fresh, xd)
    fresh.close()
    assert np.isfinite(after).all() and not np.array_equal(before, after)
    assert _same(after, want)


@pytest.mark.parametrize("name", ['stock', 'wide'])
def test_fp8_and_bf16_handles_evaluate_alike(name):
    """the evaluation of an fp8 handle reads the bf16 weight copies through the bf16 kernels; the handle only pads widths to 128
    instead of 64 with zeros, which add exact zeros behind every sum"""
    xd = P.to_dev(R.rows())
    got = []
    for dtype in (E.BF16, E.FP8):
        eng = _engine(name, dtype)
        got.append(_logits(eng, xd))
        eng.close()
    assert _same(*got)


# ---- 6. training is undisturbed where fit evaluates ------------------------------------------------------------------------
def _evaluate_nan_rows(eng, D, device=P.DEV):
    nan = torch.full((N_NAN, D), float("nan"), device=device)
    labels = torch.zeros((N_NAN,), dtype=torch.int32, device=device)
    assert eng.predict_logits(nan).shape == (N_NAN, 6)
    eng.eval_error(nan, labels)


def test_fp8_training_is_undisturbed_by_evaluation_calls():
    """test_training_is_undisturbed_by_evaluation_calls (tests/test_saliency_gpu.py) on an fp8 handle: NaN rows evaluated in
    front of every (D, G) pair -- the first in front of the calibration passes -- leave the same finite state as none"""
    case = Case(D=R.D, B=R.B, steps=2, device_z=True)
    states = []
    for disturb in (False, True):
        eng = P.engine(R.D, R.B, E.FP8)
        P.load(eng, case)
        for t in range(case.steps):
            if disturb:
                _evaluate_nan_rows(eng, R.D)
            eng.disc_step(P.disc_args(case, t, True))
            eng.gen_step(P.gen_args(case, t, True))
        states.append(G.state(eng))
        eng.close()
    assert states[0][1] == 2 * case.steps
    G.assert_finite_state(states[0])
    G.assert_same_state(*states)


def test_graph_replay_is_undisturbed_by_evaluation_calls():
    """the same in front of every replay of the captured pair of a bf16 handle: where fit(validation_data=...) evaluates"""
    G.graph_replay_is_undisturbed_by(lambda eng, big, t: _evaluate_nan_rows(eng, big.shape[1], big.device))


# ---- 7. the launches of one call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16, E.FP8], ids=["fp32", "bf16", "fp8"])
def test_kernels_of_one_call(dtype):
    """per chunk one stage_kernel, five forward products and one head_kernel, and nothing else -- on an fp8 handle too, whose
    evaluation takes no fp8 product and no quantiser"""
    eng = _engine('stock', dtype)
    y = R.labels('stock')
    for n, chunks in ((R.CHUNK + 1, 2), (1, 1)):
        xd, yd = P.to_dev(R.rows()[:n]), P.to_dev(y[:n], torch.int32)
        for entry in ("predict_logits", "eval_error"):
            eng.profile_begin()
            if entry == "predict_logits":
                eng.predict_logits(xd)
            else:
                eng.eval_error(xd, yd)
            prof = eng.profile_end()
            print(entry, n, sorted((k, v[1]) for k, v in prof.items()))
            assert prof["stage_kernel"][1] == chunks and prof["head_kernel"][1] == chunks
            G.assert_no_training_kernels(prof, 5 * chunks)
            for k in prof:
                assert k in ("stage_kernel", "head_kernel") or k.startswith("gemm"), k
                assert "fp8" not in k and "quant8" not in k, k
                assert k.startswith("gemm_f32") == (dtype == E.F32) or not k.startswith("gemm"), k
    eng.close()


# ---- 8. refusals and the Python front --------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    X, y = R.rows()[:R.S + 1], R.labels('stock')[:R.S + 1]
    n = len(X)
    eng = _engine('stock', E.BF16)
    xd, yd = P.to_dev(X), P.to_dev(y, torch.int32)
    want, want_err = _logits(eng, xd), eng.eval_error(xd, yd)
    out = torch.full((n, 6), SENT, device=P.DEV)
    err = C.c_float(-1.0)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def predict(x=ptr(xd), ld=R.D, rows=n, logits=ptr(out)):
        return eng.lib.mrgan_predict_logits(eng.handle, x, None, C.c_int64(ld), C.c_int64(rows), logits, E._stream())

    def error(x=ptr(xd), ld=R.D, labels=ptr(yd), rows=n, res=C.byref(err)):
        return eng.lib.mrgan_eval_error(eng.handle, x, None, C.c_int64(ld), labels, C.c_int64(rows), res, E._stream())

    for call, bad, status in ((predict, dict(rows=0), -1), (predict, dict(rows=-1), -1), (predict, dict(x=None), -1),
                              (predict, dict(logits=None), -1), (predict, dict(ld=R.D - 1), -2),
                              (error, dict(rows=0), -1), (error, dict(rows=-1), -1), (error, dict(x=None), -1),
                              (error, dict(labels=None), -1), (error, dict(res=None), -1), (error, dict(ld=R.D - 1), -2)):
        assert call(**bad) == status, (call.__name__, bad)
        msg = eng.lib.mrgan_last_error()
        assert (b"predict_logits" if call is predict else b"eval_error") in msg, msg
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and err.value == -1.0      # a refused call writes nothing
    with pytest.raises(E.MrganError, match="error -2"):
        eng.predict_logits(torch.zeros((4, R.D - 1), device=P.DEV))
    # the handle still evaluates
    assert predict() == 0 and error() == 0
    assert _same(out.cpu().numpy(), want) and err.value == want_err
    eng.close()


@pytest.mark.parametrize("front", ["MRGAN", "MRNN"])
def test_front_ends_take_any_host_array(front):
    """float64 rows and int64 labels as non-contiguous views: the result of the engine on the contiguous float32 / int32 copies"""
    from mr_gan_amd import MRGAN
    from mr_gan_amd.mr_nn import MRNN
    n = 2 * R.S + 1
    X64 = np.repeat(R.rows()[:n].astype(np.float64), 2, axis=0)
    X64[1::2] = np.nan
    y64 = np.repeat(R.labels('stock')[:n].astype(np.int64), 2)
    y64[1::2] = -7
    Xv, yv = X64[::2], y64[::2]
    assert not Xv.flags.c_contiguous and not yv.flags.c_contiguous
    m = MRGAN(R.D, batch_size=R.B, dtype='bfloat16', seed=5) if front == "MRGAN" else MRNN(R.D, batch_size=20, seed=5)
    logits, err = m.predict_logits(Xv), m.evaluate(Xv, yv)
    pred = m.predict(Xv) if front == "MRGAN" else np.argmax(logits, axis=1)
    torch.cuda.synchronize()
    xd, yd = P.to_dev(Xv.astype(np.float32)), P.to_dev(yv.astype(np.int32), torch.int32)
    want, want_err = m.engine.predict_logits(xd).cpu().numpy(), m.engine.eval_error(xd, yd)
    m.engine.close()
    assert logits.shape == (n, 6) and _same(logits, want)
    assert np.array_equal(pred, np.argmax(want, axis=1))
    assert err == want_err and 0.0 < err <= 1.0
    assert err == float(np.float32(np.sum(np.argmax(want, axis=1) != yv) / n))
