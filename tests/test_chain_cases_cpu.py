"""The cases of tests/test_chain_kernel.py, without a GPU: the reference alone -- the three forward products in fp64 on the case's
own draws, each stage's output rounded to bf16 as the kernel stores it -- leaves fewer relu decisions within the accumulation
bound of zero than the cap the GPU test holds the kernel's masks to, for every case in the list."""
import numpy as np
import pytest

from tests import test_chain_kernel as T


@pytest.mark.parametrize("case", [c for c in T.CASES if c["variant"] != T.GB], ids=T.case_id)
def test_reference_masks_are_decided(case):
    inp = T.chain_inputs(case)
    worst = 0.0
    for m in range(case["models"]):
        x = inp["a0"][m]
        for i, (K, N, nv) in enumerate(T.fwd_specs(case)):
            pre, accb, v, ref, bound = T.fwd_reference(case, m, i, x, inp["Wf"][i][m], inp["bf"][i][m])
            share = float((np.abs(pre) <= accb)[..., :nv].mean())
            worst = max(worst, share)
            assert share <= T.MASK_CAP, (T.case_id(case), m, i, share)
            assert (ref[..., nv:] == 0).all()
            x = T._bf16(ref)
    print("%s: largest undecided share %.5f %%" % (T.case_id(case), 100 * worst))
