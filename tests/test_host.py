"""CPU tests: golden fixtures vs the oracle, host-side data logic, and the C-ABI surface (load + exported
symbols + struct layout).  No compute call is made without a GPU."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import mrgan_oracle as O
from tests.helpers import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- golden fixtures pin the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_d16_b50.npz", "case_d400_b50_devz.npz"])
def test_oracle_reproduces_golden(name):
    g = np.load(os.path.join(GOLD, name))
    case = Case(D=int(g['D']), B=int(g['B']), steps=int(g['steps']), seed=int(g['seed']), device_z=bool(g['device_z']))
    ref = case.run_oracle()
    np.testing.assert_allclose(np.array(ref['disc']), g['disc'], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(np.array(ref['gen']), g['gen'], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(ref['logits'], g['logits'], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(ref['d'][10], g['d_w6'], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(ref['g'][2], g['g_gamma'], rtol=1e-8, atol=1e-10)


def test_tiling_golden_and_host_function():
    from mr_gan_amd.data import tiled_permutation
    g = np.load(os.path.join(GOLD, "tiling.npz"))
    for ntr, nlab in ((6000, 480), (6000, 960), (7100, 6000)):
        want = g['tiling_%d_%d' % (ntr, nlab)]
        got = tiled_permutation(np.random.RandomState(1234), nlab, ntr)
        np.testing.assert_array_equal(got, want)
        assert got.max() < nlab and len(got) == ntr
        tail = ntr % nlab
        if tail:
            assert got[-tail:].max() < tail              # mr_gan.py:189 tail quirk


def test_prologue_matches_restatement():
    from mr_gan_amd.data import select_labeled, standard_scale
    rng = np.random.default_rng(1)
    X = rng.standard_normal((600, 9)) * 2 + 3
    y = np.arange(600) % 6
    Xte = rng.standard_normal((60, 9))
    a, b = standard_scale(X, Xte)
    a2, b2 = O.standard_scale(X, Xte)
    np.testing.assert_allclose(a, a2, atol=1e-12)
    np.testing.assert_allclose(b, b2, atol=1e-12)
    xl, yl, xu = select_labeled(a, y, 10, 5)
    xl2, yl2 = O.select_labeled(a2, y, 10)
    np.testing.assert_array_equal(xl, xl2)
    np.testing.assert_array_equal(yl, yl2)
    assert xu.shape == (90, 9) and np.array_equal(xu[:10], xl[:10])
    with pytest.raises(ValueError):
        select_labeled(a, y, 101)


def test_synthetic_generators_shapes():
    from mr_gan_amd.data import synthetic_blobs, synthetic_mreo
    X, y = synthetic_blobs(n=600, d=32)
    assert X.shape == (600, 32) and X.dtype == np.float32 and set(y) == set(range(6))
    X, y, obj = synthetic_mreo(d=40, objects_per_class=2, trials=5)
    assert X.shape == (60, 40) and len(set(obj)) == 12


# ---- harness keeps the reference's CLI and print format (mr_gan.py:236-261) ------------------------------------
def test_tables_harness_format(capsys):
    import importlib
    M = importlib.import_module('mr_gan_amd.mr_gan')     # the package re-exports the function under the same name
    calls = []

    def fake_dataset(modalities=0, **kw):
        rng = np.random.default_rng(modalities)
        return rng.standard_normal((72, 5)), np.arange(72) % 6

    def fake_mr_gan(X, y, percentlabeled=50, trainTestSets=None, **kw):
        calls.append((percentlabeled, trainTestSets[0].shape, trainTestSets[1].shape))
        return 0.25
    M.main(['--tables', '1'], dataset_fn=fake_dataset, mr_gan_fn=fake_mr_gan)
    out = capsys.readouterr().out
    assert len(calls) == 7 * 7 * 6                          # modalities x percents x folds
    assert calls[0][1] == (60, 5) and calls[0][2] == (12, 5)
    assert 'Test error: 0.25 Test accuracy: 0.75' in out
    assert 'Average error: 0.25 Average accuracy: 0.75' in out
    assert 'Percentage of training data labeled: 16%' in out
    with pytest.raises(SystemExit):
        M.main([], dataset_fn=fake_dataset, mr_gan_fn=fake_mr_gan)      # --tables is required (mr_gan.py:240)


# ---- C ABI surface ------------------------------------------------------------------------------------------
def _declared_symbols():
    """every function declared in include/*.h (the drop-in boundary mrgan_abi.h and the diagnostics of mrgan_debug.h)"""
    src = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read() + open(os.path.join(ROOT, "include", "mrgan_debug.h")).read()
    return sorted(set(re.findall(r"\b(mrgan_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from mr_gan_amd import engine as E
    lib = E.load_library()
    names = _declared_symbols()
    assert len(names) >= 20 and "mrgan_debug_chain" in names
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(E.EXPORTS) == names
    # the boundary header has no diagnostic entry point, and nothing in the library reads the environment
    assert "mrgan_debug_" not in open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    for f in os.listdir(os.path.join(ROOT, "mr_gan_amd", "csrc")):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(ROOT, "mr_gan_amd", "csrc", f)).read(), f


def test_struct_layout_matches_header():
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mrgan_config), offsetof(mrgan_config, sigma), offsetof(mrgan_config, seed),
         offsetof(mrgan_config, flags), sizeof(mrgan_disc_args), sizeof(mrgan_gen_args));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert vals == [ctypes.sizeof(E.Config), E.Config.sigma.offset, E.Config.seed.offset, E.Config.flags.offset,
                    ctypes.sizeof(E.DiscArgs), ctypes.sizeof(E.GenArgs)]


def test_debug_gemm_desc_layout_matches_header():
    """mrgan_debug_gemm_desc (mrgan_debug.h) against engine.DebugGemmDesc: size, the last field from before the fp8 fields, and
    the first and last of those"""
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_debug.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mrgan_debug_gemm_desc), offsetof(mrgan_debug_gemm_desc, seed),
         offsetof(mrgan_debug_gemm_desc, slab_stride), offsetof(mrgan_debug_gemm_desc, q8), offsetof(mrgan_debug_gemm_desc, gauss),
         sizeof(mrgan_debug_fold));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    D = E.DebugGemmDesc
    assert vals == [ctypes.sizeof(D), D.seed.offset, D.slab_stride.offset, D.q8.offset, D.gauss.offset, ctypes.sizeof(E.DebugFold)]
    assert D._fields_[-1][0] == "gauss" and D.q8.offset == D.slab_stride.offset + 8


def test_debug_aux_desc_layouts_match_header():
    """the descriptors of the non-GEMM debug entries (mrgan_debug.h) against their ctypes twins: size, one field from the middle
    and the last field of each"""
    from mr_gan_amd import engine as E
    pins = [("mrgan_debug_stage_seg", E.DebugStageSeg, ("ld", "out", "sigma", "iter_off", "out_ms")),
            ("mrgan_debug_stage_desc", E.DebugStageDesc, ("s", "nseg", "seed", "gauss")),
            ("mrgan_debug_bn_apply_desc", E.DebugBnApplyDesc, ("cs1", "gamma", "seg_rows")),
            ("mrgan_debug_bn_bwd_desc", E.DebugBnBwdDesc, ("cs1", "count", "db_part")),
            ("mrgan_debug_head_desc", E.DebugHeadDesc, ("seg_kind", "labels", "batch", "part_stride", "model_stride", "err_count", "q8_slot")),
            ("mrgan_debug_head_wide_desc", E.DebugHeadWideDesc, ("mask", "ldm", "w6r")),
            ("mrgan_debug_fm_desc", E.DebugFmDesc, ("mask", "loss_out", "ldq8", "lcount")),
            ("mrgan_debug_chain_op", E.DebugChainOp, ("W", "sigma", "out_bs", "mask", "ldm", "ldcs")),
            ("mrgan_debug_chain_desc", E.DebugChainDesc, ("dx", "rows", "model_stride", "a_cols", "seed", "gauss", "batch", "head", "fm", "fm_feat",
                                                          "fm_ldf")),
            ("mrgan_debug_adam_tile", E.DebugAdamTile, ("slab_stride", "w8_slot", "cols")),
            ("mrgan_debug_adam_desc", E.DebugAdamDesc, ("lr_t", "loss_part", "flat_tail", "lr", "model_stride"))]
    body = "".join('  printf("%%zu", sizeof(%s));%s  printf("\\n");\n'
                   % (c, "".join(' printf(" %%zu", offsetof(%s, %s));' % (c, f) for f in fields)) for c, _, fields in pins)
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mrgan_debug.h"\nint main(void) {\n%s  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()
    assert len(lines) == len(pins)
    for line, (cname, S, fields) in zip(lines, pins):
        assert [int(v) for v in line.split()] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields], cname
        assert S._fields_[-1][0] == fields[-1], cname


# ---- the chain launcher's refusals: chain_args_ok (csrc/gemm_chain.hip) is pure host code and runs before any device call ------
CHAIN_P = 0x70000000         # a non-null, 16-byte aligned stand-in for every device pointer: a refused descriptor is never dereferenced


def _chain_stock(variant):
    """the engine's tail 512(500) -> 256(250) -> 256(250) -> 256(250), 130 rows per segment, as keywords of engine.debug_chain"""
    P, rows, srows = CHAIN_P, 130, 133
    w, v = [512, 256, 256, 256], [500, 250, 250, 250]
    nseg = {0: 3, 1: 2, 2: 1}[variant]
    op = lambda K, N, nv, **kw: dict(K=K, N=N, n_valid=nv, W=P, out=P, out_bs=srows * (N + 8), ldo=N + 8, mask=P, mask_bs=6 * (N + 8) * 2, ldm=N + 8, **kw)
    fwd = [op(w[i], w[i + 1], v[i + 1], bias=P, sigma=0.5, site=i + 3) for i in range(3)]
    dx = [op(w[3 - i], w[2 - i], v[2 - i], cs=P, ldcs=w[2 - i] + 8) for i in range(3)]
    head = dict(rows=rows, nseg=3, seg_kind=[0, 1, 2], feat=256, feat_valid=250, classes=6, w=P, ldw=8, b=P, labels=P, inv_count=1.0 / rows,
                unl_weight=1.0, dpre=P, dpre_bs=srows * 264, ldd=264, part=P, part_stride=2320, off_db=2048, off_dbf=2056, loss_part=P)
    fm = dict(cs=P, npart_fake=3, npart_real=3, ldcs=264, count=float(rows), grad_scale=1.0, feat=256, feat_valid=250, dpre=P, ldd=264,
              loss_out=P, accum=P)
    return dict(variant=variant, fwd=fwd, dx=dx, head=head, fm=fm, rows=rows, nseg=nseg, block_rows=64, models=1, a=P, a_bs=srows * 520, lda=520,
                a_cols=512, seed=1, row0=0, gauss=0, iter=3, fm_feat=P, fm_ldf=264)


def _chain_rc(variant, **changes):
    """the entry's return code for the stock descriptor with `changes`: 'fwd_1_K' = field K of fwd[1], 'head_feat', 'fm_ldcs', or a
    field of the launch itself"""
    import copy
    from mr_gan_amd import engine as E
    kw = copy.deepcopy(_chain_stock(variant))
    for path, val in changes.items():
        head, _, rest = path.partition("_")
        if head in ("fwd", "dx") and rest[:1].isdigit():
            kw[head][int(rest[0])][rest[2:]] = val
        elif head == "head" or (head == "fm" and rest not in ("feat", "ldf")):      # (fm_feat / fm_ldf are the launch's own)
            kw[head][rest] = val
        else:
            kw[path] = val
    rc, name = E.debug_chain(**kw)
    assert name == ""
    return rc


def test_chain_launcher_refusals_without_a_device():
    """Every descriptor below differs from a valid one in the named field(s) only and is refused before the entry allocates or
    launches anything, so the test needs no GPU (and launches nothing where there is one).  -3: launch_chain's own refusals
    (chain_args_ok); -1: what the launcher takes on trust about memory, which the entry judges only on a shape chain_args_ok
    accepted -- so every -1 below also shows that the stock descriptor of its variant passes chain_args_ok."""
    D, GF, GB = 0, 1, 2
    P = CHAIN_P
    refused = [
        # ---- the refusals launch_chain always made ----
        (D, dict(fwd_1_K=200)), (GF, dict(fwd_0_K=448)),                     # K not a multiple of 64
        (D, dict(dx_2_K=64)), (GF, dict(fwd_1_K=64)),                        # K < 128
        (GF, dict(fwd_0_K=576)), (GB, dict(dx_0_K=576)),                     # K > 512
        (GF, dict(fwd_2_N=320)), (D, dict(fwd_0_N=512)),                     # forward N > 256
        (GB, dict(dx_2_N=576)),                                              # dX N > 512
        (D, dict(fwd_1_bias=0)), (GB, dict(dx_1_mask=0)), (D, dict(dx_0_mask=0)), (GF, dict(fwd_0_W=0)), (GB, dict(dx_2_W=0)),
        (GF, dict(a_cols=448)), (D, dict(a_cols=256)),                       # a_cols != fwd[0].K
        (D, dict(block_rows=32)),                                            # no D tail at 32-row blocks
        (D, dict(head_classes=9)), (D, dict(head_ldw=32)),
        # ---- consistency between the products ----
        (GF, dict(fwd_0_N=192)), (D, dict(fwd_1_N=192)), (GF, dict(fwd_1_K=192)), (D, dict(fwd_2_K=128)),
        (GB, dict(dx_0_N=192)), (D, dict(dx_1_N=192)), (GB, dict(dx_1_K=128)), (D, dict(dx_2_K=128)),
        (GB, dict(dx_0_N=512)), (D, dict(dx_1_N=512)),                       # a two-pass product that does not end the chain ...
        (GB, dict(dx_0_N=512, dx_1_K=512)), (D, dict(dx_1_N=512, dx_2_K=512)),      # ... refused for that alone: the widths agree
        (D, dict(dx_0_K=128)), (D, dict(head_feat=192)), (D, dict(head_feat=128, dx_0_K=128)),      # dx[0].K == fwd[2].N == head.feat
        (D, dict(head_feat_valid=257)), (D, dict(head_feat_valid=0)),
        (GB, dict(dx_0_K=512)),                                              # fm.feat == dx[0].K (more below)
        (GB, dict(fm_feat_valid=300)), (GB, dict(fm_feat_valid=0)),
        (D, dict(rows=0)), (GF, dict(rows=-5)), (GB, dict(nseg=0)), (D, dict(nseg=4)),
        (GF, dict(block_rows=48)), (GB, dict(block_rows=128)), (GF, dict(block_rows=0)),
        # ---- what the kernel would dereference untested ----
        (GF, dict(fwd_2_n_valid=0)), (GF, dict(fwd_0_n_valid=300)), (D, dict(head_dpre=0)), (D, dict(head_part=0)), (D, dict(head_loss_part=0)),
        (D, dict(head_seg_kind=[0, 3, 2])), (D, dict(head_labels=0)), (GB, dict(fm_dpre=0)), (GB, dict(fm_cs=0)), (GB, dict(fm_feat=0)),
        (GF, dict(a=0)),
    ]
    for variant, ch in refused:
        assert _chain_rc(variant, **ch) == -3, (variant, ch)
    # fm.feat against dx[0].K and the image: the field is fm's `feat` (the launch's fm_feat is the pointer)
    from mr_gan_amd import engine as E
    for feat, k0 in ((192, 256), (512, 512)):
        kw = _chain_stock(GB)
        kw["fm"]["feat"] = feat
        kw["dx"][0]["K"] = k0
        assert E.debug_chain(**kw)[0] == -3, (feat, k0)
    trusted = [
        (GF, dict(a=P + 8)), (GF, dict(lda=516)), (GF, dict(lda=504)), (D, dict(a_bs=133 * 520 + 4)),
        (GF, dict(fwd_0_W=P + 8)), (GB, dict(dx_1_W=P + 2)),
        (GF, dict(fwd_1_out=P + 8)), (GF, dict(fwd_1_ldo=248)), (GB, dict(dx_2_ldo=516)), (D, dict(dx_0_out_bs=133 * 264 + 4)),
        (GF, dict(fwd_0_ldm=200)), (GB, dict(dx_2_ldm=500)),
        (D, dict(dx_2_ldcs=504)), (D, dict(dx_1_cs=P + 8)), (D, dict(dx_0_ldcs=266)),
        (GF, dict(gauss=1, row0=3)), (D, dict(gauss=1, row0=1)),
        (GF, dict(models=2, model_stride=1 << 20 | 8)),
        (GB, dict(fm_feat=P + 8)), (GB, dict(fm_ldf=248)), (GB, dict(fm_ldf=260)), (GB, dict(fm_ldcs=248)), (GB, dict(fm_ldcs=262)),
        (GB, dict(fm_cs=P + 4)), (GB, dict(fm_ldd=260)), (GB, dict(fm_ldd=248)), (GB, dict(fm_dpre=P + 8)),
        (D, dict(head_ldd=248)), (D, dict(head_ldd=260)), (D, dict(head_dpre=P + 8)), (D, dict(head_part=P + 8)), (D, dict(head_w=P + 4)),
        (D, dict(head_off_db=2044)), (D, dict(head_off_dbf=2052)), (D, dict(head_part_stride=2300)),
    ]
    for variant, ch in trusted:
        assert _chain_rc(variant, **ch) == -1, (variant, ch)
    assert b"debug_chain" in E.load_library().mrgan_last_error()


def test_fp8_round_equals_torch_casts_on_every_bf16_value():
    """The kernel-level fp8 tests encode operands and decode outputs with torch's float8 casts (tensor.view(torch.uint8)); the
    mirror rounds with oracle.fp8_round.  Both are the same grid: every finite bf16 bit pattern, times a power-of-two slot scale,
    clamped to the format's largest finite value as the packer does, gives the same dequantised value."""
    import torch
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]                    # exponent 255: infinities and NaNs
    assert bits.size == 65280
    x = (bits << 16).astype(np.uint32).view(np.float32)
    for fmt, tdt in (('e4m3', torch.float8_e4m3fn), ('e5m2', torch.float8_e5m2)):
        lim = np.float32(O.FP8_FORMATS[fmt][2])
        for scale in (1.0, 2.0 ** -7, 2.0 ** 9):
            with np.errstate(over='ignore'):                     # the largest bf16 values times 2^9: infinity, then the clamp
                v = np.clip(x * np.float32(scale), -lim, lim)
            got = torch.from_numpy(v).to(tdt)
            want = O.fp8_round(v, fmt)
            diff = int((got.to(torch.float64).numpy() != want).sum())
            assert diff == 0, (fmt, scale, diff)
            # and the byte decoder: bytes -> values is the inverse on the grid
            back = got.view(torch.uint8).view(tdt).to(torch.float64).numpy()
            assert np.array_equal(back, want)
            # 0x7F / 0xFF (NaN in both formats) is never emitted: the byte the GPU tests use as sentinel and as poison
            assert not ((got.view(torch.uint8).numpy() & 0x7F) == 0x7F).any()


def test_tuning_knobs_match_header():
    """engine.TUNE_* carry the values of the MRGAN_TUNE_* enumerators, and nothing else (retired knob numbers stay retired)"""
    from mr_gan_amd import engine as E
    src = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMRGAN_(TUNE_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    python = {n: getattr(E, n) for n in dir(E) if n.startswith("TUNE_")}
    assert len(header) >= 5
    assert python == header


def test_fp8_constants_match_headers():
    """the mirror's dry-pass count and scaling targets are the engine's: MRGAN_FP8_DRY_PASSES (mrgan_abi.h), FP8_TARGET_E4M3 /
    FP8_TARGET_E5M2 (engine_internal.h)"""
    from oracle import mrgan_oracle as O
    abi = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    internal = open(os.path.join(ROOT, "mr_gan_amd", "csrc", "engine_internal.h")).read()
    dry = re.search(r"\bMRGAN_FP8_DRY_PASSES\s*=\s*(\d+)", abi)
    targets = {m.group(1).lower(): float(m.group(2)) for m in re.finditer(r"\bFP8_TARGET_(E4M3|E5M2)\s*=\s*([0-9.]+)f", internal)}
    assert dry and O.FP8_DRY_PASSES == int(dry.group(1))
    assert sorted(targets) == ['e4m3', 'e5m2'] and O.FP8_TARGETS == targets
    # half the largest finite value of each format
    assert all(O.FP8_TARGETS[f] == O.FP8_FORMATS[f][2] / 2 for f in targets)


def test_default_config_and_workspace_size_without_gpu():
    from mr_gan_amd import engine as E
    cfg = E.default_config(512, 4096)
    assert (cfg.noise_size, list(cfg.g_hidden), list(cfg.d_hidden), cfg.num_classes) == (100, [500, 500], [1000, 500, 250, 250, 250], 6)
    assert abs(cfg.lr - 0.0006) < 1e-9 and abs(cfg.beta1 - 0.5) < 1e-9 and abs(cfg.bn_eps - 2e-5) < 1e-12
    n = ctypes.c_size_t()
    lib = E.load_library()
    for dtype, lo, hi in ((E.F32, 200e6, 900e6), (E.BF16, 100e6, 600e6)):
        cfg.dtype = dtype
        assert lib.mrgan_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
        assert lo < n.value < hi
    cfg.num_classes = 40
    assert lib.mrgan_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) != 0
    assert b"num_classes" in lib.mrgan_last_error()


def test_product_path_never_imports_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may use oracle/ (mentions in comments are fine)."""
    pkg = os.path.join(ROOT, "mr_gan_amd")
    pat = re.compile(r"^\s*(from\s+oracle|import\s+oracle|#\s*include\s*[\"<][^\">]*oracle)|import_module\(['\"]oracle|dlopen\([^)]*oracle", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                assert not pat.search(open(os.path.join(dirpath, f)).read()), f


def test_engine_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mr_gan_amd import engine as E
    with pytest.raises(RuntimeError):
        E.Engine(E.default_config(16, 50))


def test_bench_algorithmic_flops_match_survey():
    """D-step 2B[P_G + 3P_D + 3P_D + 3(P_D - 1000D)], G-step 2B[P_G + 2P_mid + P_mid + P_G + (P_G - 50000)];
    85.13 + 44.27 = 129.40 GFLOP per step at B = 4096, D = 512 -- the figure bench.py's roofline.step uses."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, D = 4096, 512
    fl = bench.algorithmic_flops(B, D)
    PD = 1000 * D + 751500
    Pmid = PD - 1500
    PG = 300000 + 500 * D
    d_step = 2.0 * B * (PG + 3 * PD + 3 * PD + 3 * (PD - 1000 * D))
    g_step = 2.0 * B * (PG + 2 * Pmid + Pmid + PG + (PG - 50000))
    assert abs(fl["total"] - (d_step + g_step)) < 1e-6 * fl["total"]
    assert abs(fl["total"] / 1e9 - 129.40) < 0.01
    assert abs(d_step / 1e9 - 85.13) < 0.01 and abs(g_step / 1e9 - 44.27) < 0.01


def test_bench_dump_outputs_stay_under_the_cap_with_a_fixed_sample(tmp_path):
    """--dump-outputs writes every tensor in full while they fit in DUMP_MAX_BYTES; above it, each tensor becomes a sample whose
    indices depend only on the geometry, so two runs of a wide stack stay comparable element for element."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class FakeEngine(object):
        def __init__(self, shapes):
            self.shapes = shapes

        def read_metrics(self, reset=True):
            return [10.0, 20.0, 30.0, 40.0, 0.5, 0.25, 0.125, 2.0]

        def get_weights(self, net):
            return [np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) + net for s in self.shapes[net]]

    E = type("E", (), {"NET_G": 0, "NET_D": 1})
    small = FakeEngine({0: [(100, 50), (50,)], 1: [(16, 30), (30,), (30, 6), (6,)]})
    bench.dump_outputs(str(tmp_path / "small"), small, E)
    assert sorted(os.listdir(str(tmp_path / "small"))) == ["disc_00.npy", "disc_01.npy", "disc_02.npy", "disc_03.npy",
                                                            "gen_00.npy", "gen_01.npy", "losses.npy"]
    assert np.load(str(tmp_path / "small" / "losses.npy")).tolist() == [0.5, 0.25, 0.125, 2.0]
    np.testing.assert_array_equal(np.load(str(tmp_path / "small" / "disc_02.npy")), small.get_weights(1)[2])

    old = bench.DUMP_MAX_BYTES
    bench.DUMP_MAX_BYTES = 40000
    try:
        wide = FakeEngine({0: [(100, 64), (64,)], 1: [(64, 64), (64,)]})
        for d in ("a", "b"):
            bench.dump_outputs(str(tmp_path / d), wide, E)
    finally:
        bench.DUMP_MAX_BYTES = old
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 40000
    for f in files:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
    g0 = np.load(str(tmp_path / "a" / "gen_00.npy"))
    assert 0 < g0.size < 6400 and np.all(np.diff(g0) > 0)       # a sorted sample of the distinct elements 0 .. 6399
