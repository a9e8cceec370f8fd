"""The host side of the grouped SVM that runs without a GPU: the sub-group plan, the --group-folds flag, the hooks of
baseline_tables and the ctypes twins of the grouped entries' descriptors."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_subgroups_keeps_order_and_bounds():
    from mr_gan_amd.svm import plan_subgroups
    rs = np.random.RandomState(0)
    cases = [([10] * 6, 100, 16), ([10] * 17, 10 ** 9, 16), ([10] * 40, 35, 16), ([50, 200, 10, 10, 300, 5], 100, 16),
             ([1], 1, 16), (rs.randint(1, 60, size=50).tolist(), 100, 4)]
    for nbytes, budget, cap in cases:
        plan = plan_subgroups(nbytes, budget, cap)
        assert [p for sub in plan for p in sub] == list(range(len(nbytes)))           # every problem once, in order
        for sub in plan:
            assert 1 <= len(sub) <= cap
            assert sum(nbytes[p] for p in sub) <= budget or len(sub) == 1             # above the budget only alone
        for a, b in zip(plan, plan[1:]):                                              # greedy: the next one did not fit
            assert len(a) == cap or sum(nbytes[p] for p in a) + nbytes[b[0]] > budget
    assert plan_subgroups([10] * 6, 100) == [[0, 1, 2, 3, 4, 5]]
    assert [len(s) for s in plan_subgroups([10] * 17, 10 ** 9)] == [16, 1]
    assert plan_subgroups([50, 200, 10, 10, 300, 5], 100) == [[0], [1], [2, 3], [4], [5]]
    assert plan_subgroups([], 100) == []


def test_group_checks_arguments_before_any_device_call():
    from mr_gan_amd import RBFSVMGroup
    with pytest.raises(ValueError):
        RBFSVMGroup(gram_bytes=0)
    with pytest.raises(ValueError):
        RBFSVMGroup(gamma='scale')
    g = RBFSVMGroup()
    assert (g.C, g.gamma, g.tol, g.max_iter, g.gram_bytes) == (1.0, 'auto', 1e-3, 10_000_000, 4 << 30)
    x, y = np.zeros((4, 3)), [0, 0, 1, 1]
    with pytest.raises(ValueError, match="feature count"):
        g.fit([x, np.zeros((4, 2))], [y, y])
    with pytest.raises(ValueError, match="class count"):
        g.fit([x, x], [y, [0, 1, 2, 2]])
    with pytest.raises(ValueError, match="non-finite"):
        g.fit([x, np.full((4, 3), np.nan)], [y, y])
    with pytest.raises(ValueError, match="at least one"):
        g.fit([], [])
    with pytest.raises(RuntimeError, match="fit"):
        g.predict([x])
    with pytest.raises(RuntimeError, match="fit"):
        g[0]


def _fake_dataset():
    rs = np.random.RandomState(0)

    def fake_dataset(modalities=0, leaveObjectOut=False, **kw):
        if leaveObjectOut:          # 30 objects: two full runs of twelve and a run of six
            return {'m%d_o%d' % (m, o): {'x': rs.randn(4, 3).tolist(), 'y': [m] * 4} for m in range(6) for o in range(5)}
        return rs.randn(36, 3), np.arange(36) % 6
    return fake_dataset


def _err(s):
    """a test error that depends on the sets alone"""
    return float(np.round(np.abs(np.asarray(s[1])).sum() % 1.0, 6))


def test_group_folds_flag_needs_the_hip_backend(capsys):
    import mr_gan_amd.mr_svm as S
    for argv in (['--tables', '2', '--group-folds'], ['--tables', '2', '--group-folds', '--backend', 'sklearn']):
        with pytest.raises(SystemExit) as e:
            S.main(argv, dataset_fn=_fake_dataset(), fn=lambda X, y, **kw: 0.5)
        assert e.value.code == 2
        assert '--group-folds needs --backend hip' in capsys.readouterr().err


@pytest.mark.parametrize("table", ['2', '4'])
def test_baseline_tables_prints_the_same_lines_through_the_hooks(table, capsys, monkeypatch):
    """fn alone, and stub folds_fn / objects_fn hooks returning fn's values: the same lines in the same order; the hooks get
    the six folds of a table-2 cell and runs of at most twelve objects of a table-4 cell"""
    import sklearn.model_selection as M
    import mr_gan_amd.mr_svm as S

    base = M.StratifiedKFold

    class Folds(base):                              # baseline_tables' folds are unseeded: pin them for the comparison
        def __init__(self, n_splits=6, shuffle=True):
            base.__init__(self, n_splits=n_splits, shuffle=shuffle, random_state=5)
    monkeypatch.setattr(M, 'StratifiedKFold', Folds)

    def fn(X, y, percentlabeled=50, trainTestSets=None, verbose=False):
        return _err(trainTestSets)
    seen = []

    def hook(sets, percentlabeled=50, verbose=False):
        seen.append(len(sets))
        return [_err(s) for s in sets]
    S.baseline_tables([table], fn, _fake_dataset(), False)
    plain = capsys.readouterr().out
    S.baseline_tables([table], fn, _fake_dataset(), False, folds_fn=None, objects_fn=None)
    assert capsys.readouterr().out == plain
    S.baseline_tables([table], fn, _fake_dataset(), False, folds_fn=hook, objects_fn=hook)
    hooked = capsys.readouterr().out
    assert hooked == plain and len(plain.splitlines()) > 20
    assert seen == ([6] * 14 if table == '2' else [12, 12, 6] * 10)
    if table == '4':
        assert plain.count('Test error:') == 30 * 10 and 'm0_o0 Test error:' in plain


def test_group_folds_reaches_both_tables_through_main(capsys):
    import mr_gan_amd.mr_svm as S
    seen = []

    def hook(sets, percentlabeled=50, verbose=False):
        seen.append(len(sets))
        return [0.25] * len(sets)
    S.main(['--tables', '2', '4', '--backend', 'hip', '--group-folds'], dataset_fn=_fake_dataset(),
           fn=lambda X, y, **kw: pytest.fail("fn must not be called"), folds_fn=hook)
    assert seen == [6] * 14 + [12, 12, 6] * 10
    assert 'Average error: 0.25' in capsys.readouterr().out
    # mr_nn passes no object hook: its table 4 calls fn per object
    from mr_gan_amd import mr_nn as N
    calls = []
    N.main(['--tables', '4', '--group-folds'], dataset_fn=_fake_dataset(), fn=lambda X, y, **kw: calls.append(1) or 0.5, folds_fn=hook)
    assert len(calls) == 30 * 10
    capsys.readouterr()


def test_group_item_layouts_match_header():
    """mrgan_svm_{gram,solve,decide}_item against their ctypes twins: size and the offset of the last field"""
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(mrgan_svm_gram_item), offsetof(mrgan_svm_gram_item, ld_out),
         sizeof(mrgan_svm_solve_item), offsetof(mrgan_svm_solve_item, iters_dev),
         sizeof(mrgan_svm_decide_item), offsetof(mrgan_svm_decide_item, labels_dev), MRGAN_SVM_MAX_GROUP);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert vals == [ctypes.sizeof(E.SvmGramItem), E.SvmGramItem.ld_out.offset, ctypes.sizeof(E.SvmSolveItem), E.SvmSolveItem.iters.offset,
                    ctypes.sizeof(E.SvmDecideItem), E.SvmDecideItem.labels.offset, E.SVM_MAX_GROUP]
    assert E.SvmGramItem._fields_[-1][0] == "ld_out" and E.SvmSolveItem._fields_[-1][0] == "iters" and E.SvmDecideItem._fields_[-1][0] == "labels"
    assert E.SVM_MAX_GROUP == E.MAX_MODELS
