"""The references of tests/test_data_parallel_gpu.py, pinned on the CPU against the protocol's oracle stand-in.

tests/parity.py::shard_mean_reference says what W ranks exchange: with per-shard statistics the mean over ranks of the gradients
of W independent shard-sized steps, with synchronised statistics the full-batch gradient.  Here the fp64 oracle cut into the
phases of the C ABI (tests/test_dist_cpu.py::OraclePhases, one per rank) runs through the same lock-step DataParallel the GPU
tests use, and what it all-reduces must be that reference to 1e-12 -- so a wrong reference, or a lock-step driver that skips or
misplaces an exchange, fails here, without a GPU."""
import numpy as np
import pytest

from oracle import mrgan_oracle as O
from tests import parity as P
from tests.helpers import Case, rel_err
from tests.test_dist_cpu import OraclePhases, _flat


def _exchanged(case, world, exact):
    """the gradient regions W oracle ranks hold behind their all-reduces in one D and one G sub-step -> (flat dD, flat dG)"""
    from mr_gan_amd import engine as E
    h = case.B // world
    ranks = [OraclePhases(case.g0, case.d0, world, exact) for _ in range(world)]
    seen = {}
    dp = P.LockstepDataParallel(ranks, exact=exact, on_exchange=lambda which: seen.setdefault(which, []).append(
        [b.region(which).numpy().copy() for b in ranks]))
    dp.disc_step([case.disc_inputs(0, 0, rows=h, row0=r * h) for r in range(world)])
    dp.gen_step([case.gen_inputs(0, 1, rows=h, row0=r * h) for r in range(world)])
    stats = [E.REGION_BN_STATS, E.REGION_BN_STATS, E.REGION_FM_MOMENTS, E.REGION_BN_BWD] if exact else []
    assert sorted(w for w in seen for _ in seen[w]) == sorted(stats + [E.REGION_GRAD_D, E.REGION_GRAD_G]), seen.keys()
    out = []
    for which in (E.REGION_GRAD_D, E.REGION_GRAD_G):
        per_rank = seen[which][0]
        for other in per_rank[1:]:
            np.testing.assert_array_equal(other, per_rank[0])
        out.append(per_rank[0][:-4])
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_per_shard_statistics_exchange_the_mean_of_shard_gradients(world):
    case = Case(D=12, B=16, steps=1)
    gd, gg = _exchanged(case, world, exact=False)
    ref = P.shard_mean_reference(case, lambda: O.MRGANOracle(case.g0, case.d0), world)
    assert rel_err(gd, _flat(ref['gd'])) < 1e-12 and rel_err(gg, _flat(ref['gg'])) < 1e-12
    # and that is another algorithm than the full-batch step
    full = P.shard_mean_reference(case, lambda: O.MRGANOracle(case.g0, case.d0), 1)
    assert rel_err(gg, _flat(full['gg'])) > 1e-4


@pytest.mark.parametrize("world", [2, 4])
def test_synchronised_statistics_exchange_the_full_batch_gradient(world):
    case = Case(D=12, B=16, steps=1)
    gd, gg = _exchanged(case, world, exact=True)
    orc = O.MRGANOracle(case.g0, case.d0)
    _, gd_o, _ = orc.disc_grads(**case.disc_inputs(0, 0))
    orc.adam.apply(orc.d, gd_o, 'd')
    _, gg_o, _ = orc.gen_grads(**case.gen_inputs(0, 1))
    assert rel_err(gd, _flat(gd_o)) < 1e-12 and rel_err(gg, _flat(gg_o)) < 1e-12
    # shard_mean_reference(shards = 1) is that full-batch step
    ref = P.shard_mean_reference(case, lambda: O.MRGANOracle(case.g0, case.d0), 1)
    assert rel_err(_flat(ref['gd']), _flat(gd_o)) < 1e-12 and rel_err(_flat(ref['gg']), _flat(gg_o)) < 1e-12


def test_shard_outputs_average_to_the_full_batch_losses():
    """the D outputs are sums scaled by 1 / B_global: the mean over shards of those of the labelled rows (loss, training error) is
    the full batch's; the unlabelled loss sees generated rows normalised per shard, and the generator loss of a shard is a square
    of ITS moment difference: neither averages to the full batch's"""
    case = Case(D=12, B=16, steps=1)
    make = lambda: O.MRGANOracle(case.g0, case.d0)
    full, halves = P.shard_mean_reference(case, make, 1), P.shard_mean_reference(case, make, 2)
    np.testing.assert_allclose(halves['d_out'][[0, 2]], full['d_out'][[0, 2]], rtol=1e-12, atol=1e-14)
    assert abs(halves['d_out'][1] - full['d_out'][1]) > 1e-6 * full['d_out'][1]
    assert len(halves['g_loss']) == 2 and abs(np.mean(halves['g_loss']) - full['g_loss'][0]) > 1e-6 * full['g_loss'][0]
