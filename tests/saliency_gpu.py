"""What the GPU tests of mrgan_input_gradient and mrgan_attribution share: handles with a loaded case, bit views, sentinel
buffers, and the bodies of the checks both entries answer alike -- what a call must leave alone, the group handle, the fp8
refusal and the kernels a call may launch.  The problems themselves are those of tests/saliency_ref.py."""
import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from oracle import mrgan_oracle as O
from tests import parity as P
from tests import saliency_ref as R
from tests.helpers import Case

B, WIDE_HEAD, DECIDED = R.B, R.WIDE_HEAD, R.DECIDED
FP32_TOL = 2e-4                       # parity.fp32_gradients_match_oracle's bound on gradients behind the same dX chain
SENT = -768.0


def engine(case, D, dtype, **kw):
    if case.d_hidden != tuple(O.D_HIDDEN):
        kw['d_hidden'] = case.d_hidden
    eng = P.engine(D, B, dtype, num_classes=case.K, **kw)
    P.load(eng, case)
    return eng


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wide_rows(x32):
    """the rows on the device with a pitch of D + 9, NaN behind every row"""
    n, D = x32.shape
    wide = torch.full((n, D + 9), float("nan"), device=P.DEV)
    wide[:, :D] = P.to_dev(x32)
    return wide


def sentinel_buffers(n, D):
    """(out of pitch D + 5 full of SENT, classes_out full of -1)"""
    return torch.full((n, D + 5), SENT, device=P.DEV), torch.full((n,), -1, dtype=torch.int32, device=P.DEV)


def dead_row_engine(dtype, K=6, D=72, n=200):
    """(a handle whose first-layer biases are negative, so a zero row has every unit of layer 1 dead; five rows, row 2 zero)"""
    case, x32 = R.problem(K, D, None, n)
    eng = P.engine(D, B, dtype, num_classes=K)
    d = [p.astype(np.float32) for p in case.d0]
    d[1] = -np.abs(d[1]) - 0.5
    eng.set_weights(E.NET_D, d)
    x = x32[:5].copy()
    x[2] = 0.0
    return eng, x


# ---- what a call must leave alone ----------------------------------------------------------------------------------
def state(eng):
    out = []
    for net in (E.NET_G, E.NET_D):
        out += eng.get_weights(net) + eng.get_slot(net, 0) + eng.get_slot(net, 1)
    return out, eng.get_iterations(), eng.read_metrics(reset=False)


def assert_same_state(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a[1] == b[1]
    assert np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


def assert_finite_state(a):
    assert all(np.isfinite(x).all() for x in a[0]) and np.isfinite(np.asarray(a[2], np.float32)).all()


def training_is_undisturbed_by(disturb):
    """three (D, G) pairs of a bf16 handle with disturb(eng, big, t) in front of each, big = 199 large rows (two chunks, every
    padding row of segment 0): the same state as without"""
    D = 400
    case = Case(D=D, B=B, steps=3, device_z=True)
    big = P.to_dev(1e3 * np.random.default_rng(9).standard_normal((3 * 64 + 7, D)).astype(np.float32))
    states = []
    for on in (False, True):
        eng = P.engine(D, B, E.BF16)
        P.load(eng, case)
        for t in range(case.steps):
            if on:
                disturb(eng, big, t)
            eng.disc_step(P.disc_args(case, t, True))
            eng.gen_step(P.gen_args(case, t, True))
        states.append(state(eng))
        eng.close()
    assert states[0][1] == 2 * case.steps
    assert_same_state(*states)


def graph_replay_is_undisturbed_by(disturb):
    """the same in front of every replay of the captured pair"""
    from mr_gan_amd import MRGAN
    D, n = 400, 4 * B
    case = Case(D=D, B=B, steps=1, device_z=True)
    rs = np.random.RandomState(3)
    X, xl = rs.randn(n, D).astype(np.float32), rs.randn(2 * B, D).astype(np.float32)
    yl = rs.randint(0, 6, size=2 * B).astype(np.int32)
    big = 1e3 * rs.randn(3 * 64 + 7, D).astype(np.float32)
    states = []
    for on in (False, True):
        m = MRGAN(D, batch_size=B, dtype='bfloat16', seed=77, use_graph=True, init_weights=False)
        P.load(m.engine, case)
        with m._on_stream():
            xu, xlab, bigd = m._dev(X), m._dev(xl), m._dev(big)
            idx_lab = m._dev(np.arange(n, dtype=np.int32) % (2 * B), torch.int32)
            labs = m._dev(yl[np.arange(n) % (2 * B)], torch.int32)
            idx_u1 = m._dev(np.arange(n, dtype=np.int32)[::-1].copy(), torch.int32)
            idx_u2 = m._dev(np.roll(np.arange(n, dtype=np.int32), 7), torch.int32)
            dargs = E.Engine.disc_args(xlab, labs, xu, None, idx_lab, idx_u1, stream_mode=1)
            gargs = E.Engine.gen_args(xu, None, idx_u2, stream_mode=1)
            m.engine.set_iterations(0, 0)
            for t in range(n // B):
                if on:
                    disturb(m.engine, bigd, t)
                m.engine.train_pair(dargs, gargs)
            torch.cuda.synchronize()
            states.append(state(m.engine))
        m.engine.close()
    assert states[0][1] == 2 * (n // B)
    assert_same_state(*states)


# ---- what both entries answer alike --------------------------------------------------------------------------------
def group_handle_serves_the_selected_model(dtype, n, **kw):
    """saliency(m, X, **kw) of a group of three equals the single model of seed + m, bit for bit -> the group's results"""
    from mr_gan_amd import MRGAN, MRGANGroup
    D, seed = 40, 123
    X = np.random.default_rng(3).standard_normal((n, D)).astype(np.float32)
    grp = MRGANGroup(D, 3, batch_size=B, dtype=dtype, seed=seed)
    got = [grp.saliency(m, X, **kw) for m in (2, 0, 1)]
    grp.engine.close()
    for (maps, cls), m in zip(got, (2, 0, 1)):
        one = MRGAN(D, batch_size=B, dtype=dtype, seed=seed + m)
        want, wcls = one.saliency(X, **kw)
        one.engine.close()
        assert maps.shape == (n, D) and maps.dtype == np.float32
        assert np.array_equal(bits(maps), bits(want)) and np.array_equal(cls, wcls)
    assert not np.array_equal(got[0][0], got[1][0])
    return got


def fp8_handle_is_refused(call):
    eng = P.engine(64, 128, E.FP8)
    with pytest.raises(E.MrganError) as ei:
        call(eng, torch.zeros((4, 64), device=P.DEV))
    eng.close()
    msg = str(ei.value)
    assert "error -3" in msg and "fp32" in msg and "bf16" in msg


def profiled_engine(dtype, d_hidden, rows):
    """(a handle of D = 96 with a loaded case, `rows` rows on the device)"""
    D = 96
    kw = dict(d_hidden=d_hidden) if d_hidden else {}
    eng = P.engine(D, B, dtype, **kw)
    P.load(eng, Case(D=D, B=B, steps=1, **kw))
    return eng, P.to_dev(np.random.default_rng(3).standard_normal((rows, D)).astype(np.float32))


def assert_no_training_kernels(prof, gemms):
    """no matrix-core head, no chain launch, no weight gradient, no update; `gemms` products"""
    for name in prof:
        assert not any(s in name for s in ("head_wide", "chain_kernel", "adam", "_ks_", "w6_split", "reduce_partials", "fm_kernel")), name
        assert not name.startswith(("gemm_f32_kernel<2", "gemm_bf16_kc_kernel<2")), name
    assert sum(v[1] for k, v in prof.items() if k.startswith("gemm")) == gemms
