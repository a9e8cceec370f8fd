"""The inputs of the GPU parity tests, pinned.  Several measured bounds sit close to what the engine gives on exactly these
draws (at K = 32 the matrix-core head differs from the scalar head on 4.17 % of rows, bound 5 %), so an edit of
tests.helpers.Case that moves them would quietly change what those tests measure.  The digests were computed with the
classes as they stood when the bounds were measured (Case, GaussCase and the many-classes KCase, before they became one)."""
import hashlib

import numpy as np
import pytest

from tests.gaussian_noise import GaussCase
from tests.helpers import Case

HID_WIDE_HEAD = (256, 256, 256, 512, 512)


def case_digest(case, **shard):
    """sha256 over the raw bytes of g0, d0, labels, x_lab, x_unl, x_unl2, z1, z2, probe and of disc_inputs(0, 0) and
    gen_inputs(0, 1) (keys in sorted order; `shard` = rows / row0 of the two calls)"""
    h = hashlib.sha256()

    def add(a):
        for x in (a if isinstance(a, (list, tuple)) else [a]):
            h.update(b"none" if x is None else np.ascontiguousarray(x).tobytes())

    for a in (case.g0, case.d0, case.labels, case.x_lab, case.x_unl, case.x_unl2, case.z1, case.z2, case.probe):
        add(a)
    for inputs in (case.disc_inputs(0, 0, **shard), case.gen_inputs(0, 1, **shard)):
        for key in sorted(inputs):
            add(inputs[key])
    return h.hexdigest()


PINNED = [
    ("default", lambda: Case(D=16, B=50), {}, "705369b76e806b57170973ea4bb3e4d903334dc72dad6998cd4b7e1608f7f069"),
    ("default_device_z", lambda: Case(D=48, B=50, steps=1, device_z=True), {}, "45105a953714eecf40471d78a82c6c6fb3fcba0bff2f8b3cb6b76cfe9df080ee"),
    ("gaussian", lambda: GaussCase(D=48, B=50, steps=1, device_z=True), {}, "a2da4b833950d649c34856ba04538641d22b0fc7ab2043a8aa326f0a990a1ece"),
    ("k10", lambda: Case(K=10, D=16, B=50), {}, "703edbfec4f27c035cece70d577072e55bf168d75fc6885e9ad3b92d2f14dfd5"),
    ("k32_wide_head", lambda: Case(K=32, D=96, B=200, d_hidden=HID_WIDE_HEAD, device_z=True), {}, "8199a296ba2d7950de487e17fa4ce474287e588b9dc16901fc5b21040cc27612"),
    ("k10_row_shard", lambda: Case(K=10, D=32, B=64, steps=2, device_z=True), dict(rows=32, row0=32), "efa3251f67fe887bc972d2906ca8222e58991f0ec88575d2362124f1530faa34"),
]


@pytest.mark.parametrize("name,build,shard,want", PINNED, ids=[p[0] for p in PINNED])
def test_case_draws_are_pinned(name, build, shard, want):
    assert case_digest(build(), **shard) == want
