"""Model groups, the parts that need no GPU: the boundary structs against the header, the workspace size of a group, and the
--group-folds harness of mr_nn."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_structs_match_header():
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(mrgan_sup_group_args), offsetof(mrgan_sup_group_args, labels_dev),
         offsetof(mrgan_sup_group_args, ld_x), offsetof(mrgan_sup_group_args, x_model_stride),
         offsetof(mrgan_sup_group_args, idx_model_stride), offsetof(mrgan_sup_group_args, labels_model_stride),
         offsetof(mrgan_sup_group_args, rows_valid), offsetof(mrgan_config, models), sizeof(mrgan_config), MRGAN_MAX_MODELS);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    A, Cf = E.SupGroupArgs, E.Config
    assert vals == [ctypes.sizeof(A), A.labels.offset, A.ld_x.offset, A.x_model_stride.offset, A.idx_model_stride.offset,
                    A.labels_model_stride.offset, A.rows_valid.offset, Cf.models.offset, ctypes.sizeof(Cf), E.MAX_MODELS]
    # the field took the place of `reserved`: the last four bytes of a config whose size did not change
    assert Cf.models.offset == ctypes.sizeof(Cf) - 4 == Cf.flags.offset + 4
    assert {"mrgan_select_model", "mrgan_sup_step_group"} <= set(E.EXPORTS)


def test_default_config_leaves_models_zero_and_group_workspace_is_g_times_the_single_one():
    """mrgan_workspace_bytes(models = G) = G x the single size (itself a multiple of 256); there is no shared part beside the
    copies: the shared DevState slots are model 0's"""
    from mr_gan_amd import engine as E
    lib = E.load_library()
    for D, B, dtype in ((48, 20, E.F32), (1200, 20, E.BF16), (72, 50, E.BF16)):
        cfg = E.default_config(D, B)
        assert cfg.models == 0
        cfg.dtype = dtype
        sizes = {}
        for models in (0, 1, 2, 6, 16):
            cfg.models = models
            n = ctypes.c_size_t(0)
            assert lib.mrgan_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
            sizes[models] = n.value
        one = sizes[0]
        assert one % 256 == 0 and sizes[1] == one
        assert [sizes[g] for g in (2, 6, 16)] == [2 * one, 6 * one, 16 * one]
    cfg = E.default_config(48, 20)
    n = ctypes.c_size_t(0)
    for bad in (-1, 17):
        cfg.models = bad
        assert lib.mrgan_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1
        assert b"models" in lib.mrgan_last_error()
    cfg.models, cfg.dtype = 2, E.FP8
    assert lib.mrgan_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -3 and b"group" in lib.mrgan_last_error()


def test_group_folds_harness_prints_the_ungrouped_lines(capsys):
    """--tables 2 --group-folds with a stub mr_nn_folds against the ungrouped harness with a stub fn returning the same errors:
    the same lines, six folds per group, the percentages in the reference's order"""
    from mr_gan_amd.mr_nn import main

    def fake_dataset(modalities=0, leaveObjectOut=False, **kw):
        rs = np.random.RandomState(modalities)
        return rs.randn(36, 3), np.arange(36) % 6

    errs = [0.125, 0.25, 0.5, 0.0, 0.375, 0.25]
    groups, calls = [], []

    def folds(sets, percentlabeled=None, verbose=False):
        groups.append((percentlabeled, [tuple(np.shape(a) for a in s) for s in sets]))
        return list(errs)

    def fn(X, y, percentlabeled=None, **kw):
        calls.append(percentlabeled)
        return errs[(len(calls) - 1) % 6]

    main(['--tables', '2', '--group-folds'], dataset_fn=fake_dataset, folds_fn=folds)
    grouped = capsys.readouterr().out
    main(['--tables', '2'], dataset_fn=fake_dataset, fn=fn)
    plain = capsys.readouterr().out
    assert grouped == plain and grouped.count('Average error: 0.25 Average accuracy: 0.75') == 14
    assert [g[0] for g in groups] == [1, 2, 4, 8, 16, 50, 100] * 2 and len(calls) == 14 * 6
    for _, shapes in groups:
        assert shapes == [((30, 3), (6, 3), (30,), (6,))] * 6
    # without the flag the folds hook is not used, and a fold function never sees table 4
    groups.clear()
    main(['--tables', '2'], dataset_fn=fake_dataset, fn=fn, folds_fn=folds)
    assert not groups
