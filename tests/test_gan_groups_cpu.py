"""Model groups, the GAN hot loop -- the parts that need no GPU: the two group argument structs against the header, the
bindings of the new entries, and the --group-folds harness of mr_gan."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D_FIELDS = ["x_lab_dev", "idx_lab_dev", "labels_dev", "x_unl_dev", "idx_unl_dev", "z_dev", "ld_x_lab", "ld_x_unl", "x_lab_model_stride",
            "idx_lab_model_stride", "labels_model_stride", "x_unl_model_stride", "idx_unl_model_stride", "z_model_stride", "stream_mode",
            "reserved"]
G_FIELDS = ["x_unl_dev", "idx_unl_dev", "z_dev", "ld_x_unl", "x_unl_model_stride", "idx_unl_model_stride", "z_model_stride",
            "stream_mode", "reserved"]


def test_gan_group_structs_match_header():
    """size and every field offset of mrgan_disc_group_args / mrgan_gen_group_args against a C program compiled from the header;
    the leading fields lie where those of mrgan_disc_args / mrgan_gen_args lie"""
    from mr_gan_amd import engine as E
    lines = ['printf("%zu\\n", sizeof(mrgan_disc_group_args));', 'printf("%zu\\n", sizeof(mrgan_gen_group_args));']
    lines += ['printf("%%zu\\n", offsetof(mrgan_disc_group_args, %s));' % f for f in D_FIELDS]
    lines += ['printf("%%zu\\n", offsetof(mrgan_gen_group_args, %s));' % f for f in G_FIELDS]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mrgan_abi.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    A, B = E.DiscGroupArgs, E.GenGroupArgs
    py = lambda S: [getattr(S, n).offset for n, _ in S._fields_]
    assert [n for n, _ in A._fields_] == [f[:-4] if f.endswith("_dev") else f for f in D_FIELDS]
    assert [n for n, _ in B._fields_] == [f[:-4] if f.endswith("_dev") else f for f in G_FIELDS]
    assert vals == [ctypes.sizeof(A), ctypes.sizeof(B)] + py(A) + py(B)
    assert ctypes.sizeof(A) == 14 * 8 + 8 and ctypes.sizeof(B) == 7 * 8 + 8
    for S, single, n in ((A, E.DiscArgs, 8), (B, E.GenArgs, 4)):
        assert [(f, getattr(S, f).offset) for f, _ in S._fields_[:n]] == [(f, getattr(single, f).offset) for f, _ in single._fields_[:n]]


def test_engine_binds_every_new_entry():
    from mr_gan_amd import engine as E
    new = {"mrgan_disc_step_group", "mrgan_gen_step_group", "mrgan_train_pair_group"}
    assert new <= set(E.EXPORTS)
    lib = E.load_library()
    for name in new:
        assert getattr(lib, name).restype is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    for name in new:
        assert "int %s(" % name in header
    for method in ("disc_group_args", "gen_group_args", "disc_step_group", "gen_step_group", "train_pair_group"):
        assert callable(getattr(E.Engine, method))
    import mr_gan_amd
    assert mr_gan_amd.MRGANGroup is __import__("mr_gan_amd.model", fromlist=["MRGANGroup"]).MRGANGroup and "MRGANGroup" in mr_gan_amd.__all__


def _fake_dataset(n):
    def fake_dataset(modalities=0, leaveObjectOut=False, **kw):
        rs = np.random.RandomState(modalities)
        return rs.randn(n, 3), np.arange(n) % 6
    return fake_dataset


ERRS = [0.125, 0.25, 0.5, 0.0, 0.375, 0.25]


def test_group_folds_harness_prints_the_ungrouped_lines(capsys):
    """--tables 1 --group-folds with a stub mr_gan_folds against the ungrouped harness with a stub mr_gan returning the same
    errors: the same lines in the same order, six folds per group, the percentages in the reference's order"""
    from mr_gan_amd.mr_gan import main
    groups, calls = [], []

    def folds(sets, percentlabeled=None, **kw):
        assert set(kw) == {"epochs", "dtype", "verbose"}
        groups.append((percentlabeled, [tuple(np.shape(a) for a in s) for s in sets]))
        return list(ERRS)

    def fn(X, y, percentlabeled=None, trainTestSets=None, **kw):
        calls.append(percentlabeled)
        return ERRS[(len(calls) - 1) % 6]

    main(['--tables', '1', '--group-folds'], dataset_fn=_fake_dataset(36), mr_gan_fn=fn, folds_fn=folds)
    grouped = capsys.readouterr().out
    assert not calls
    main(['--tables', '1'], dataset_fn=_fake_dataset(36), mr_gan_fn=fn)
    plain = capsys.readouterr().out
    assert grouped == plain and grouped.count('Average error: 0.25 Average accuracy: 0.75') == 49
    assert [g[0] for g in groups] == [1, 2, 4, 8, 16, 50, 100] * 7 and len(calls) == 49 * 6
    for _, shapes in groups:
        assert shapes == [((30, 3), (6, 3), (30,), (6,))] * 6
    # without the flag the folds hook is not used
    groups.clear()
    main(['--tables', '1'], dataset_fn=_fake_dataset(36), mr_gan_fn=fn, folds_fn=folds)
    capsys.readouterr()
    assert not groups


def test_group_folds_table_6_groups_each_amount_of_unlabeled_data(capsys):
    from mr_gan_amd.mr_gan import main
    groups = []

    def folds(sets, percentlabeled=None, percentunlabeled=None, **kw):
        groups.append((percentlabeled, percentunlabeled, len(sets)))
        return list(ERRS)

    main(['--tables', '6', '--group-folds'], dataset_fn=_fake_dataset(36), mr_gan_fn=None, folds_fn=folds)
    assert groups == [(4, u, 6) for u in [0, 4, 8, 16, 32, 64, 96]] * 2
    assert capsys.readouterr().out.count('Average error: 0.25') == 14


def test_group_folds_is_refused_with_gpus(capsys):
    from mr_gan_amd.mr_gan import main
    made = []
    with pytest.raises(SystemExit):
        main(['--tables', '1', '--group-folds', '--gpus', '2'], dataset_fn=_fake_dataset(36), scheduler_factory=lambda **kw: made.append(kw))
    assert "scheduling groups over GPUs" in capsys.readouterr().err and not made


def test_unequal_fold_lengths_fall_back_to_the_ungrouped_path(capsys):
    """38 rows: the six stratified folds train on 31 or 32 rows, so no cell can be one group; and a folds function that finds
    unequal labelled sets (UnequalFolds) sends its cell to the ungrouped path too.  The lines are the ungrouped harness's."""
    from mr_gan_amd.mr_gan import UnequalFolds, main
    groups, calls = [], []

    def folds(sets, **kw):
        groups.append(len(sets))
        raise UnequalFolds("labelled sets differ")

    def fn(X, y, percentlabeled=None, trainTestSets=None, **kw):
        calls.append(len(trainTestSets[0]))
        return ERRS[(len(calls) - 1) % 6]

    main(['--tables', '1', '--group-folds'], dataset_fn=_fake_dataset(38), mr_gan_fn=fn, folds_fn=folds)
    out = capsys.readouterr().out
    assert not groups and len(calls) == 49 * 6 and set(calls) == {31, 32}
    assert out.count('Average error: 0.25 Average accuracy: 0.75') == 49
    calls.clear()
    main(['--tables', '1', '--group-folds'], dataset_fn=_fake_dataset(36), mr_gan_fn=fn, folds_fn=folds)
    assert groups == [6] * 49 and len(calls) == 49 * 6 and set(calls) == {30}
    assert capsys.readouterr().out == out
