"""Data-parallel parity of the bf16 and fp8 engines: W rank handles at B / W rows on one GPU against the FULL batch.

The ABI states that rows are global: the shards of a batch draw what the full batch would, so W ranks with synchronised
statistics are the full-batch step up to summation order.  The references are independent of the engine: the full-batch
MRGANMirror (bf16 roundings where the engine stores bf16) and the fp64 oracle.  Everything runs in one process; the all-reduce
is a device-side add over the ranks' exchange regions (tests/parity.py: sum_exchange), and where whole sub-steps or pairs are
driven, the control flow is dist.DataParallel's own (LockstepDataParallel: pair hint, fp8 calibration order, skipped exchanges).

Geometries (reference hidden widths unless stated, z drawn on the device):
  a  bf16 D 96  B 200  W 1, 2   h = 100: ragged against 32- and 64-row blocks, rank 1 starts at global row 100; the chain runs
  b  bf16 D 96  B 400  W 2, 4   h = 200: two weight-gradient slabs per D tensor; W = 4: row0 = 200 and 300
  c  bf16 D 96  B 256  W 2      d_hidden = WIDE_HEAD: the matrix-core head with inv_count = 1 / B_global
  d  bf16 D 96  B 200  W 2      ten classes: the 32-class pitch, D3 .. D5 layer by layer
  e  bf16 D 96  B 200  W 2      FLAG_GAUSS_NOISE: row pairs from row0 = 100
  f  fp8  D 200 B 256  W 2      h = 128
The bounds of the gradient tests are those of the single-handle grad_parity cases at the same widths and class count
(test_gpu_parity.py::test_bf16_gradients_match_bf16_mirror, ::test_wide_head_bf16_gradients_match_bf16_mirror,
test_many_classes_gpu.py::test_bf16_gradients_match_bf16_mirror, test_gaussian_noise_gpu.py::..._gaussian)."""
import numpy as np
import pytest

from tests import parity as P
from tests.helpers import update_rel_err
from tests.saliency_ref import WIDE_HEAD

pytestmark = pytest.mark.gpu

D, B_A = 96, 200
BF16_BOUNDS = dict(tol=3e-3, tol_loss=5e-4)          # frac 0.6, loose (0.995, 0.98, 0.25): grad_parity's defaults


# ---------------------------------------------------------------------------------------------------------
# 1. global rows, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [P.DEFAULT, P.GAUSSIAN], ids=["a", "e"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_shards_stage_the_rows_of_the_full_batch(variant, dtype):
    """Rank 1 of two (row0 = 100, no multiple of 32) holds rows 100 .. 199 of the full batch's staged real rows and of its first
    discriminator product, bit for bit: the noise is keyed by the global row, and with one forced tile a row's reduction order
    does not depend on the launch's row count."""
    P.shards_stage_the_rows_of_the_full_batch(variant, dtype, D, B_A, 2)


# ---------------------------------------------------------------------------------------------------------
# 2. all-reduced gradients against the full-batch mirror
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_gradients_match_full_batch_mirror_a(world):
    """W = 1: a single FLAT_GRADS | SYNC_STATS handle -- bf16 with the statistics through colsum_finalize against the mirror"""
    P.dp_grad_parity(P.DEFAULT, D, B_A, world, 1, **BF16_BOUNDS)


@pytest.mark.parametrize("world", [2, 4])
def test_gradients_match_full_batch_mirror_b(world):
    P.dp_grad_parity(P.DEFAULT, D, 400, world, 1, **BF16_BOUNDS)


def test_gradients_match_full_batch_mirror_c_wide_head():
    P.dp_grad_parity(P.DEFAULT, D, 256, 2, 1, d_hidden=WIDE_HEAD, **BF16_BOUNDS)


def test_gradients_match_full_batch_mirror_d_ten_classes():
    P.dp_grad_parity(P.classes(10), D, B_A, 2, 1, **BF16_BOUNDS)


def test_gradients_match_full_batch_mirror_e_gaussian():
    P.dp_grad_parity(P.GAUSSIAN, D, B_A, 2, 1, **BF16_BOUNDS)


# ---------------------------------------------------------------------------------------------------------
# 3. fp8
# ---------------------------------------------------------------------------------------------------------
def test_fp8_replicas_calibrate_in_lock_step():
    """Geometry f through the lock-step DataParallel with exact=True: the host runs the calibration passes of both sub-step kinds
    with real BN_STATS / FM_MOMENTS / BN_BWD exchanges between two replicas.  The replicas' all-reduced flat gradients and their
    weights are bit-identical, both kinds report themselves calibrated on both ranks, and the gradients keep the LOOSE fp64
    bound of test_fp8_gradients_match_fp8_mirror (cosine > 0.9 for D, > 0.8 for G, error < 0.6).
    There is no mirror-tight bound here: each rank settles its activation and gradient scales from its own shard's amax (the
    scaling slots are not exchanged), so a full-batch fp8 mirror, which calibrates on the amax of all rows, is not a
    like-for-like reference for the replicas' roundings."""
    P.fp8_replicas_calibrate_in_lock_step(200, 256, 2)


# ---------------------------------------------------------------------------------------------------------
# 4. per-shard statistics
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_per_shard_statistics_match_the_mean_of_shard_references(dtype):
    """exact=False: each rank normalises with its own 100 rows, scales its sums by 1 / B_global and its feature-matching gradient by
    fm_scale = 1 / world; the all-reduced gradients are the mean over ranks of shard-sized references (tests/test_dp_refs_cpu.py
    pins that reference against the protocol's oracle stand-in).  bf16: the mirror rule of test 2; fp32: the bounds of
    fp32_gradients_match_oracle."""
    P.dp_grad_parity(P.DEFAULT, D, B_A, 2, dtype, exact=False, **(BF16_BOUNDS if dtype else {}))


# ---------------------------------------------------------------------------------------------------------
# 5. two pairs through train_pair
# ---------------------------------------------------------------------------------------------------------
PAIR_GEOMETRIES = [pytest.param(B_A, None, id="a"), pytest.param(256, WIDE_HEAD, id="c")]


@pytest.mark.parametrize("B,d_hidden", PAIR_GEOMETRIES)
def test_train_pair_on_two_ranks_matches_full_batch_mirror(B, d_hidden):
    """(i) the replicas' D and G weights are bit-identical after two pairs; (ii) the same pairs as disc_step + gen_step without the
    hint give bit-identical weights and metrics -- the paired pass, whose two BN_STATS segments travel in one all-reduce, is what the
    G sub-step would compute on its own; (iii) the weights against the full-batch mirror trajectory under the rule of
    test_bf16_steps_match_bf16_mirror."""
    P.lockstep_pairs_match_mirror(D, B, 2, d_hidden)


@pytest.mark.parametrize("B,d_hidden", PAIR_GEOMETRIES)
def test_train_pair_on_two_ranks_with_bf16_gradient_payload(B, d_hidden):
    """MRGAN_FLAG_GRAD_BF16 on a bf16 engine: replicas bit-identical, and the weights are those of the fp32 payload up to the
    bf16 rounding of the gradients -- the window of test_two_rank_emulation_with_bf16_gradient_payload, against the fp32-payload run"""
    case = P._pairs_problem(D, B, d_hidden, 2)[0]
    w16 = P.lockstep_pairs(D, B, 2, d_hidden, 'bf16', True, 2)[0][0]
    w32 = P.lockstep_pairs(D, B, 2, d_hidden, None, True, 2)[0][0]
    errs = [update_rel_err(a, b, w0) for a, b, w0 in zip(w16, w32, case.d0)]
    print("\nD weights, bf16 payload vs fp32 payload, error / update size: %s" % " ".join("%.1e" % e for e in errs))
    assert 1e-6 < max(errs) < 0.3, errs


# ---------------------------------------------------------------------------------------------------------
# 6. one rank: phases against whole steps
# ---------------------------------------------------------------------------------------------------------
def test_bf16_phase_protocol_equals_whole_steps_bit_for_bit():
    """per-shard statistics: the phases launch the kernels of the whole sub-steps in the same order"""
    for net, i, err, same in P.phases_equal_whole_steps(D, B_A, exact=False):
        assert same, (net, i, err)


def test_bf16_phase_protocol_with_synchronised_statistics_equals_whole_steps():
    """synchronised statistics take the BatchNorm sums and the feature-matching moments through colsum_finalize: another summation
    order, held to the bound test_fp8_phase_protocol_equals_whole_steps has for the same difference"""
    res = P.phases_equal_whole_steps(D, B_A, exact=True)
    print("\nerror / update size: %s" % " ".join("%.1e" % err for _, _, err, _ in res))
    for net, i, err, _ in res:
        assert err < 2e-2, (net, i, err)
