"""The host side of the grouped SVM kinds that runs without a GPU: the ctypes twin of mrgan_svm_solve_nu_item, the new entries in
the headers and in EXPORTS, KernelSVMGroup's checks, the entries and item fields KernelSVMGroup and RBFSVMGroup issue (on a
recording stand-in for the library), and mr_svm_folds(classifier=...)."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mrgan_svm_kernel_matrix_group", "mrgan_svm_solve_nu_group", "mrgan_debug_svm_kernel_matrix_group")


def test_solve_nu_item_layout_matches_header():
    """mrgan_svm_solve_nu_item against SvmSolveNuItem: 72 bytes, the offsets of nu, r_dev and iters_dev"""
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mrgan_svm_solve_nu_item), offsetof(mrgan_svm_solve_nu_item, class_start_host),
         offsetof(mrgan_svm_solve_nu_item, nu), offsetof(mrgan_svm_solve_nu_item, coef_dev), offsetof(mrgan_svm_solve_nu_item, r_dev),
         offsetof(mrgan_svm_solve_nu_item, iters_dev));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    I = E.SvmSolveNuItem
    assert vals == [ctypes.sizeof(I), I.class_start.offset, I.nu.offset, I.coef.offset, I.r.offset, I.iters.offset]
    assert vals[0] == 72 and vals[2] == 32 and vals[4] == 56 and vals[5] == 64
    assert [f[0] for f in I._fields_] == ['k', 'ld_k', 'n', 'class_start', 'nu', 'coef', 'rho', 'r', 'iters']


def test_new_entries_are_declared_and_exported():
    from mr_gan_amd import engine as E
    abi = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    dbg = open(os.path.join(ROOT, "include", "mrgan_debug.h")).read()
    for name in NEW_ENTRIES:
        assert name in E.EXPORTS
        assert re.search(r"^int %s\(" % name, dbg if name.startswith("mrgan_debug_") else abi, re.M), name
    assert "mrgan_svm_decide_group serves all four kinds unchanged" in abi
    import mr_gan_amd
    assert mr_gan_amd.KernelSVMGroup is mr_gan_amd.svm.KernelSVMGroup and "KernelSVMGroup" in mr_gan_amd.__all__


def test_kernel_group_checks_arguments_before_any_device_call(monkeypatch):
    from mr_gan_amd import KernelSVMGroup
    from mr_gan_amd import engine as E
    from mr_gan_amd import svm as S
    monkeypatch.setattr(E, 'load_library', lambda: pytest.fail("no library call before the checks pass"))
    monkeypatch.setattr(S._DeviceSVM, '_call', lambda self, *a: pytest.fail("no library call before the checks pass"))
    with pytest.raises(ValueError, match="kernel must be one of"):
        KernelSVMGroup(kernel='poly')
    for nu in (0.0, 1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match=r"nu must be None \(C-SVC\) or a number in \(0, 1\]"):
            KernelSVMGroup(nu=nu)
    with pytest.raises(ValueError):
        KernelSVMGroup(gram_bytes=0)
    g = KernelSVMGroup()
    assert (g.kernel, g.nu, g.C, g.gamma, g.tol, g.max_iter, g.gram_bytes) == ('rbf', None, 1.0, 'auto', 1e-3, 10_000_000, 4 << 30)
    x, y = np.zeros((4, 3)), [0, 0, 1, 1]
    for g in (KernelSVMGroup(kernel='linear'), KernelSVMGroup(nu=0.5)):
        with pytest.raises(ValueError, match="feature count"):
            g.fit([x, np.zeros((4, 2))], [y, y])
        with pytest.raises(ValueError, match="class count"):
            g.fit([x, x], [y, [0, 1, 2, 2]])
        with pytest.raises(ValueError, match="non-finite"):
            g.fit([x, np.full((4, 3), np.nan)], [y, y])
        with pytest.raises(ValueError, match="at least one"):
            g.fit([], [])
        with pytest.raises(RuntimeError, match="KernelSVMGroup: fit"):
            g.predict([x])
        with pytest.raises(RuntimeError, match="KernelSVMGroup: fit"):
            g[0]
        assert len(g) == 0
    # a nu sequence is checked at fit: its length, then every value
    with pytest.raises(ValueError, match="one nu per problem"):
        KernelSVMGroup(nu=[0.5, 0.5, 0.5]).fit([x, x], [y, y])
    with pytest.raises(ValueError, match=r"number in \(0, 1\].*problem 1"):
        KernelSVMGroup(nu=[0.5, 1.5]).fit([x, x], [y, y])
    # infeasible on problem 1 of two: 0.5 * (7 + 33) / 2 = 10 > 7, KernelSVM's words and the problem
    big, yb = np.zeros((40, 3)), [3] * 7 + [8] * 33
    with pytest.raises(ValueError, match=r"specified nu is infeasible.*classes 3 and 8 \(problem 1\)"):
        KernelSVMGroup(nu=0.5).fit([big, big], [[3] * 20 + [8] * 20, yb])
    with pytest.raises(ValueError, match=r"specified nu is infeasible.*problem 1"):
        KernelSVMGroup(kernel='linear', nu=[0.1, 0.5]).fit([big, big], [yb, yb])


class Recorder:
    """stands in for _DeviceSVM._call on device='cpu': records (entry, arguments with the descriptors unpacked) and zeroes what
    a solver item writes, so that the host side reads finite results"""

    def __init__(self, K):
        self.calls, self.K = [], K

    def __call__(self, obj, name, *args):
        out = []
        for a in args:
            if isinstance(a, ctypes.Array) and isinstance(a[0], ctypes.Structure):
                out.append([{f[0]: getattr(it, f[0]) for f in it._fields_} for it in a])
            else:
                out.append(a)
        self.calls.append((name, out))
        pairs = self.K * (self.K - 1) // 2
        if name in ("mrgan_svm_solve_group", "mrgan_svm_solve_nu_group"):
            for it in args[0]:
                ctypes.memset(it.coef, 0, 8 * (self.K - 1) * it.n)
                ctypes.memset(it.rho, 0, 8 * pairs)
                ctypes.memset(it.iters, 0, 4 * pairs)
                if name.endswith("nu_group"):
                    ctypes.memset(it.r, 0, 8 * pairs)


def _recorded_fit(monkeypatch, make, sizes, K=2):
    from mr_gan_amd import svm as S
    rec = Recorder(K)
    monkeypatch.setattr(S._DeviceSVM, '_call', lambda self, name, *a: rec(self, name, *a))
    monkeypatch.setattr(S._DeviceSVM, '_require_gpu', lambda self: None)
    rs = np.random.RandomState(0)
    Xs = [rs.randn(n, 3) for n in sizes]
    ys = [np.arange(n) % K for n in sizes]
    group = make().fit(Xs, ys)
    return group, rec.calls


def test_kernel_group_issues_the_grouped_entries_per_sub_group(monkeypatch):
    """19 problems are sub-groups of 16 and 3: per sub-group one kernel-matrix launch and one solver launch, with the kind, the
    group's scalars and per-item fields"""
    from mr_gan_amd import KernelSVMGroup
    from mr_gan_amd import engine as E
    sizes = [4 + (p % 5) for p in range(19)]
    # C-SVC, linear kernel
    group, calls = _recorded_fit(monkeypatch, lambda: KernelSVMGroup(kernel='linear', C=2.0, device='cpu'), sizes)
    assert [c[0] for c in calls] == ["mrgan_svm_kernel_matrix_group", "mrgan_svm_solve_group"] * 2
    for (name, a), cnt, first in zip(calls[::2], (16, 3), (0, 16)):
        assert a[0] == E.SVM_KERNEL_LINEAR and len(a[1]) == cnt and a[2:] == [cnt, 3, 1.0 / 3]
        for k, it in enumerate(a[1]):
            n = sizes[first + k]
            assert (it['m'], it['n'], it['ld_a'], it['ld_b'], it['ld_out']) == (n, n, 3, 3, n) and it['a'] == it['b']
    for (name, a), cnt, first in zip(calls[1::2], (16, 3), (0, 16)):
        assert len(a[0]) == cnt and a[1:] == [cnt, 2, 2.0, 1e-3, 10_000_000]
        assert [it['n'] for it in a[0]] == sizes[first:first + cnt] and all('nu' not in it for it in a[0])
    assert len(group) == 19 and all(group[p].r_ is None for p in range(19))
    # nu-SVC with a nu per problem, RBF kernel
    nus = [0.1 + 0.04 * p for p in range(19)]
    group, calls = _recorded_fit(monkeypatch, lambda: KernelSVMGroup(nu=nus, gamma=0.25, tol=1e-2, max_iter=77, device='cpu'), sizes)
    assert [c[0] for c in calls] == ["mrgan_svm_kernel_matrix_group", "mrgan_svm_solve_nu_group"] * 2
    assert calls[0][1][0] == E.SVM_KERNEL_RBF and calls[0][1][2:] == [16, 3, 0.25]
    grams = [it['out'] for c in calls[::2] for it in c[1][1]]
    seen = []
    for (name, a), cnt in zip(calls[1::2], (16, 3)):
        assert len(a[0]) == cnt and a[1:] == [cnt, 2, 1e-2, 77]
        seen += a[0]
    assert [it['nu'] for it in seen] == nus and [it['n'] for it in seen] == sizes
    assert [it['k'] for it in seen] == grams and all(it['r'] and it['coef'] and it['rho'] and it['iters'] for it in seen)
    assert len({it['r'] for it in seen}) == 19
    assert all(group[p].r_.shape == (1,) and group[p].n_iter_.tolist() == [0] for p in range(19))
    # a scalar nu reaches every item
    group, calls = _recorded_fit(monkeypatch, lambda: KernelSVMGroup(kernel='linear', nu=0.5, device='cpu'), [4, 6, 8])
    assert [c[0] for c in calls] == ["mrgan_svm_kernel_matrix_group", "mrgan_svm_solve_nu_group"]
    assert [it['nu'] for it in calls[1][1][0]] == [0.5] * 3 and calls[0][1][0] == E.SVM_KERNEL_LINEAR


def test_rbfsvm_group_issues_the_entries_it_issued_before(monkeypatch):
    from mr_gan_amd import RBFSVMGroup
    sizes = [4, 7, 5]
    group, calls = _recorded_fit(monkeypatch, lambda: RBFSVMGroup(C=3.0, device='cpu'), sizes)
    assert [c[0] for c in calls] == ["mrgan_svm_gram_group", "mrgan_svm_solve_group"]
    (_, g), (_, s) = calls
    assert g[1:] == [3, 3, 1.0 / 3] and [(it['m'], it['n']) for it in g[0]] == [(n, n) for n in sizes]
    assert s[1:] == [3, 2, 3.0, 1e-3, 10_000_000] and [it['k'] for it in s[0]] == [it['out'] for it in g[0]]
    assert sorted(s[0][0]) == ['class_start', 'coef', 'iters', 'k', 'ld_k', 'n', 'rho']
    assert len(group) == 3 and group[1].dual_coef_dense_.shape == (1, 7)


def test_mr_svm_folds_builds_the_right_group(monkeypatch):
    import mr_gan_amd.mr_svm as S
    from mr_gan_amd import synthetic_mreo
    made = []

    def fake(cls_name):
        class Fake:
            def __init__(self, **kw):
                self.name, self.kw = cls_name, kw
                made.append(self)

            def fit(self, Xs, ys):
                self.fitted = len(Xs)
                return self

            def score(self, Xs, ys):
                return [0.75] * len(Xs)
        return Fake
    monkeypatch.setattr(S, 'RBFSVMGroup', fake('RBFSVMGroup'))
    monkeypatch.setattr(S, 'KernelSVMGroup', fake('KernelSVMGroup'))
    X, y, _ = synthetic_mreo(d=40, trials=20, sep=3.0)
    fold = np.arange(len(y)) % 3
    sets = [[X[fold != f], X[fold == f], y[fold != f], y[fold == f]] for f in range(3)]
    want = {None: ('RBFSVMGroup', dict(C=1.0, gamma='auto')), 'svc-rbf': ('RBFSVMGroup', dict(C=1.0, gamma='auto')),
            'svc-linear': ('KernelSVMGroup', dict(kernel='linear', nu=None, C=1.0, gamma='auto')),
            'nu-rbf': ('KernelSVMGroup', dict(kernel='rbf', nu=0.5, C=1.0, gamma='auto')),
            'nu-linear': ('KernelSVMGroup', dict(kernel='linear', nu=0.5, C=1.0, gamma='auto'))}
    for classifier, (cls_name, kw) in want.items():
        made.clear()
        extra = {} if classifier is None else dict(classifier=classifier)
        assert S.mr_svm_folds(sets, percentlabeled=2, seed=3, **extra) == [0.25] * 3
        assert len(made) == 1 and (made[0].name, made[0].kw, made[0].fitted) == (cls_name, kw, 3)
    made.clear()
    with pytest.raises(ValueError, match="classifier"):
        S.mr_svm_folds(sets, percentlabeled=2, seed=3, classifier='linear-svc')
    assert not made


def test_group_folds_flag_still_refuses_the_other_classifiers(capsys):
    import mr_gan_amd.mr_svm as S
    with pytest.raises(SystemExit) as e:
        S.main(['--tables', '2', '--backend', 'hip', '--group-folds', '--classifier', 'nu-rbf'],
               dataset_fn=lambda **kw: pytest.fail("no data is read"), fn=lambda X, y, **kw: pytest.fail("fn must not be called"))
    assert e.value.code == 2 and 'svc-rbf only' in capsys.readouterr().err
