"""ctypes binding of libmrgan_hip.so (include/mrgan_abi.h).

PyTorch is used here only for device memory (the workspace and I/O tensors), the current HIP stream
and, in dist.py, torch.distributed.  There is no CPU or eager-PyTorch fallback: if the HIP library
is missing or fails, every entry point raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmrgan_hip.so")

F32, BF16, FP8 = 0, 1, 2
NET_G, NET_D = 0, 1
FLAG_SYNC_STATS, FLAG_FLAT_GRADS, FLAG_GRAPH, FLAG_GRAD_BF16, FLAG_GAUSS_NOISE = 1, 2, 4, 8, 16
FLAG_AUTOENCODER = 32         # MRGAN_FLAG_AUTOENCODER: NET_D is a dense autoencoder (ae_step / ae_encode / ae_reconstruct)
NOISE_MODES = ('irwin-hall', 'gaussian')
D_GEN, D_MAIN, D_ADAM = 0, 1, 2
G_GEN, G_FEAT, G_BWD, G_TAIL, G_ADAM = 0, 1, 2, 3, 4
TUNE_CHAIN, TUNE_KC_CFG, TUNE_KS_GROUP, TUNE_PAIR_GEN, TUNE_HEAD_MFMA = 0, 1, 4, 5, 6
REGION_BN_STATS, REGION_FM_MOMENTS, REGION_BN_BWD, REGION_GRAD_D, REGION_GRAD_G, REGION_WORKSPACE = range(6)
REGION_GRAD_D_BF16, REGION_GRAD_G_BF16, REGION_TAIL_D, REGION_TAIL_G = 6, 7, 8, 9

EXPORTS = [
    "mrgan_default_config", "mrgan_workspace_bytes", "mrgan_create", "mrgan_destroy", "mrgan_last_error",
    "mrgan_num_tensors", "mrgan_tensor_shape", "mrgan_set_weights", "mrgan_get_weights", "mrgan_get_slot",
    "mrgan_set_slot", "mrgan_get_iterations", "mrgan_set_iterations", "mrgan_disc_step", "mrgan_gen_step",
    "mrgan_train_pair", "mrgan_sup_step", "mrgan_fp8_calibration", "mrgan_logmel", "mrgan_logmel_frames", "mrgan_region", "mrgan_eval_error", "mrgan_predict_logits", "mrgan_read_metrics",
    "mrgan_pair_hint", "mrgan_set_tuning", "mrgan_debug_noise", "mrgan_debug_tr_probe", "mrgan_debug_gemm_launch", "mrgan_profile_begin", "mrgan_profile_end", "mrgan_debug_ablate", "mrgan_debug_gemm_time", "mrgan_debug_buffer", "mrgan_debug_gemm_fp8",
    "mrgan_debug_quant8", "mrgan_debug_fp8_update_scales",
    "mrgan_debug_stage", "mrgan_debug_reduce_partials","mrgan_debug_colsum_finalize", "mrgan_debug_bn_apply", "mrgan_debug_bn_bwd", "mrgan_debug_head", "mrgan_debug_head_wide",
    "mrgan_debug_fm", "mrgan_debug_adam", "mrgan_debug_chain",
    "mrgan_select_model", "mrgan_sup_step_group",
    "mrgan_disc_step_group", "mrgan_gen_step_group", "mrgan_train_pair_group",
    "mrgan_input_gradient", "mrgan_attribution",
    "mrgan_ae_step", "mrgan_ae_encode", "mrgan_ae_reconstruct",
    "mrgan_svm_gram", "mrgan_svm_solve", "mrgan_svm_decide", "mrgan_debug_svm_gram",
    "mrgan_svm_gram_group", "mrgan_svm_solve_group", "mrgan_svm_decide_group", "mrgan_debug_svm_gram_group",
    "mrgan_svm_kernel_matrix", "mrgan_svm_solve_nu", "mrgan_debug_svm_kernel_matrix",
    "mrgan_svm_kernel_matrix_group", "mrgan_svm_solve_nu_group", "mrgan_debug_svm_kernel_matrix_group",
    "mrgan_pca_mean", "mrgan_pca_covariance_workspace_bytes", "mrgan_pca_covariance", "mrgan_pca_eig_workspace_bytes", "mrgan_pca_eig",
    "mrgan_pca_transform", "mrgan_pca_inverse_transform",
    "mrgan_debug_pca_covariance_workspace_bytes", "mrgan_debug_pca_covariance", "mrgan_debug_pca_orthonormalize",
]
PCA_MAX_COMPONENTS = 64       # MRGAN_PCA_MAX_COMPONENTS
PCA_GUARD = 16                # MRGAN_PCA_GUARD: extra rows of the iterated block
PCA_MAX_FEATURES = 4096       # MRGAN_PCA_MAX_FEATURES: the covariance is one d x d buffer
PCA_RANK_DEFICIENT = -4       # MRGAN_PCA_RANK_DEFICIENT: mrgan_pca_eig's "numerical rank below n_components"
SVM_MAX_PAIR = 2048           # MRGAN_SVM_MAX_PAIR: rows of one one-vs-one problem
SVM_MAX_CLASSES = 32
SVM_MAX_GROUP = 16            # MRGAN_SVM_MAX_GROUP: problems of one grouped launch
SVM_KERNEL_RBF, SVM_KERNEL_LINEAR = 0, 1
SVM_KERNELS = {'rbf': SVM_KERNEL_RBF, 'linear': SVM_KERNEL_LINEAR}
SAL_LOGIT, SAL_XENT, SAL_MSE = 0, 1, 2
SAL_RAW, SAL_HEATMAP = 0, 1
SAL_OBJECTIVES = {'logit': SAL_LOGIT, 'xent': SAL_XENT, 'mse': SAL_MSE}
ATTR_NOISE, ATTR_PATH = 0, 1
ATTR_MAX_DRAWS = 4096
ATTR_NOISE_SEG = 255          # MRGAN_ATTR_NOISE_SEG: the noise segment id of the attribution draws (no training draw uses it)
ATTR_METHODS = ('gradient', 'smoothgrad', 'integrated')
MAX_MODELS = 16
PROF_NAME_LEN = 96


class Config(C.Structure):
    _fields_ = [
        ("d_in", C.c_int32), ("batch", C.c_int32), ("noise_size", C.c_int32),
        ("g_hidden", C.c_int32 * 2), ("d_hidden", C.c_int32 * 5),
        ("num_classes", C.c_int32), ("dtype", C.c_int32),
        ("sigma", C.c_float * 5),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
        ("bn_eps", C.c_float), ("unlabeled_weight", C.c_float),
        ("seed", C.c_uint64),
        ("rank", C.c_int32), ("world", C.c_int32), ("flags", C.c_int32), ("models", C.c_int32),
    ]


class DiscArgs(C.Structure):
    _fields_ = [
        ("x_lab", C.c_void_p), ("idx_lab", C.c_void_p), ("labels", C.c_void_p),
        ("x_unl", C.c_void_p), ("idx_unl", C.c_void_p), ("z", C.c_void_p),
        ("ld_x_lab", C.c_int64), ("ld_x_unl", C.c_int64),
        ("stream_mode", C.c_int32), ("reserved", C.c_int32),
    ]


class GenArgs(C.Structure):
    _fields_ = [
        ("x_unl", C.c_void_p), ("idx_unl", C.c_void_p), ("z", C.c_void_p),
        ("ld_x_unl", C.c_int64),
        ("stream_mode", C.c_int32), ("reserved", C.c_int32),
    ]


class SupArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("idx", C.c_void_p), ("labels", C.c_void_p),
        ("ld_x", C.c_int64),
        ("stream_mode", C.c_int32), ("rows_valid", C.c_int32),
    ]


class AeArgs(C.Structure):
    """mrgan_ae_args"""
    _fields_ = [
        ("x", C.c_void_p), ("idx", C.c_void_p),
        ("ld_x", C.c_int64),
        ("stream_mode", C.c_int32), ("rows_valid", C.c_int32),
    ]


class SupGroupArgs(C.Structure):
    """mrgan_sup_group_args: the model strides count elements"""
    _fields_ = [
        ("x", C.c_void_p), ("idx", C.c_void_p), ("labels", C.c_void_p),
        ("ld_x", C.c_int64),
        ("x_model_stride", C.c_int64), ("idx_model_stride", C.c_int64), ("labels_model_stride", C.c_int64),
        ("stream_mode", C.c_int32), ("rows_valid", C.c_int32),
    ]


class DiscGroupArgs(C.Structure):
    """mrgan_disc_group_args: mrgan_disc_args + element strides between models"""
    _fields_ = [
        ("x_lab", C.c_void_p), ("idx_lab", C.c_void_p), ("labels", C.c_void_p),
        ("x_unl", C.c_void_p), ("idx_unl", C.c_void_p), ("z", C.c_void_p),
        ("ld_x_lab", C.c_int64), ("ld_x_unl", C.c_int64),
        ("x_lab_model_stride", C.c_int64), ("idx_lab_model_stride", C.c_int64), ("labels_model_stride", C.c_int64),
        ("x_unl_model_stride", C.c_int64), ("idx_unl_model_stride", C.c_int64), ("z_model_stride", C.c_int64),
        ("stream_mode", C.c_int32), ("reserved", C.c_int32),
    ]


class GenGroupArgs(C.Structure):
    """mrgan_gen_group_args: mrgan_gen_args + element strides between models"""
    _fields_ = [
        ("x_unl", C.c_void_p), ("idx_unl", C.c_void_p), ("z", C.c_void_p),
        ("ld_x_unl", C.c_int64),
        ("x_unl_model_stride", C.c_int64), ("idx_unl_model_stride", C.c_int64), ("z_model_stride", C.c_int64),
        ("stream_mode", C.c_int32), ("reserved", C.c_int32),
    ]


class SvmGramItem(C.Structure):
    """mrgan_svm_gram_item"""
    _fields_ = [
        ("a", C.c_void_p), ("ld_a", C.c_int64), ("m", C.c_int64),
        ("b", C.c_void_p), ("ld_b", C.c_int64), ("n", C.c_int64),
        ("out", C.c_void_p), ("ld_out", C.c_int64),
    ]


class SvmSolveItem(C.Structure):
    """mrgan_svm_solve_item"""
    _fields_ = [
        ("k", C.c_void_p), ("ld_k", C.c_int64), ("n", C.c_int64),
        ("class_start", C.POINTER(C.c_int64)),
        ("coef", C.c_void_p), ("rho", C.c_void_p), ("iters", C.c_void_p),
    ]


class SvmSolveNuItem(C.Structure):
    """mrgan_svm_solve_nu_item"""
    _fields_ = [
        ("k", C.c_void_p), ("ld_k", C.c_int64), ("n", C.c_int64),
        ("class_start", C.POINTER(C.c_int64)),
        ("nu", C.c_double),
        ("coef", C.c_void_p), ("rho", C.c_void_p), ("r", C.c_void_p), ("iters", C.c_void_p),
    ]


class SvmDecideItem(C.Structure):
    """mrgan_svm_decide_item"""
    _fields_ = [
        ("kt", C.c_void_p), ("ld_kt", C.c_int64), ("m", C.c_int64), ("n", C.c_int64),
        ("class_start", C.POINTER(C.c_int64)),
        ("coef", C.c_void_p), ("rho", C.c_void_p), ("dec", C.c_void_p), ("labels", C.c_void_p),
    ]


class SaliencyArgs(C.Structure):
    """mrgan_saliency_args"""
    _fields_ = [
        ("x", C.c_void_p), ("idx", C.c_void_p), ("ld_x", C.c_int64), ("n", C.c_int64),
        ("targets", C.c_void_p),
        ("objective", C.c_int32), ("post", C.c_int32),
        ("out", C.c_void_p), ("ld_out", C.c_int64),
        ("classes_out", C.c_void_p),
    ]


class AttributionArgs(C.Structure):
    """mrgan_attribution_args"""
    _fields_ = SaliencyArgs._fields_ + [
        ("method", C.c_int32), ("draws", C.c_int32),
        ("sigma_input", C.c_float), ("sigma_hidden", C.c_float),
        ("baseline", C.c_void_p),
        ("multiply", C.c_int32), ("reserved", C.c_int32),
    ]


def attribution_plan(method, draws=None, sigma=None, baseline=None, times_input=False, d_in=None, own_sigmas=(0.3, 0.5)):
    """The keywords of MRGAN.saliency -> the dict of Engine.attribution's keywords (method, draws, sigma_input, sigma_hidden,
    baseline, multiply).  Everything is checked here, before any device call:
      'gradient'    one gradient of the noise-free forward; draws, sigma and baseline do not apply; times_input: x input
      'smoothgrad'  the mean over draws (default 16) forwards with GaussianNoise: sigma None = the network's own sigmas
                    (own_sigmas: input, hidden), a float = input-only noise, (input, hidden) = both; times_input: x input
      'integrated'  integrated gradients over draws (default 16) points of the path from baseline (None: zeros; else [d_in])
                    to the row; always x (input - baseline)"""
    if method not in ATTR_METHODS:
        raise ValueError("method must be one of %s, got %r" % (ATTR_METHODS, method))
    if method == 'gradient':
        for name, v in (('draws', draws), ('sigma', sigma), ('baseline', baseline)):
            if v is not None:
                raise ValueError("%s does not apply to method 'gradient' (use 'smoothgrad' or 'integrated')" % name)
        return dict(method=ATTR_NOISE, draws=1, sigma_input=0.0, sigma_hidden=0.0, baseline=None, multiply=1 if times_input else 0)
    if draws is None:
        draws = 16
    if isinstance(draws, bool) or not isinstance(draws, (int, np.integer)) or not 1 <= int(draws) <= ATTR_MAX_DRAWS:
        raise ValueError("draws must be an integer in [1, %d], got %r" % (ATTR_MAX_DRAWS, draws))
    if method == 'smoothgrad':
        if baseline is not None:
            raise ValueError("baseline belongs to method 'integrated', not 'smoothgrad'")
        if sigma is None:
            sig = tuple(own_sigmas)
        elif isinstance(sigma, (tuple, list)):
            if len(sigma) != 2:
                raise ValueError("sigma must be a float (input only) or a pair (input, hidden), got %r" % (sigma,))
            sig = tuple(sigma)
        else:
            sig = (sigma, 0.0)
        try:
            sig = (float(sig[0]), float(sig[1]))
        except (TypeError, ValueError):
            raise ValueError("sigma must be a float (input only) or a pair (input, hidden), got %r" % (sigma,))
        if not all(np.isfinite(v) and v >= 0.0 for v in sig):
            raise ValueError("sigma must be finite and >= 0, got %r" % (sigma,))
        return dict(method=ATTR_NOISE, draws=int(draws), sigma_input=sig[0], sigma_hidden=sig[1], baseline=None,
                    multiply=1 if times_input else 0)
    if sigma is not None:
        raise ValueError("sigma belongs to method 'smoothgrad'; 'integrated' is noise-free")
    if baseline is not None:
        baseline = np.asarray(baseline, dtype=np.float32)
        if baseline.ndim != 1 or (d_in is not None and baseline.shape[0] != d_in) or not np.isfinite(baseline).all():
            raise ValueError("baseline must be a finite vector of d_in%s values, got shape %s"
                             % ("" if d_in is None else " = %d" % d_in, baseline.shape))
    return dict(method=ATTR_PATH, draws=int(draws), sigma_input=0.0, sigma_hidden=0.0, baseline=baseline, multiply=1)


def saliency_objective(objective):
    """'logit' | 'xent' | 'mse' -> MRGAN_SAL_*"""
    if objective not in SAL_OBJECTIVES:
        raise ValueError("objective must be one of %s, got %r" % (sorted(SAL_OBJECTIVES), objective))
    return SAL_OBJECTIVES[objective]


_lib = None


def load_library(path=None):
    """Load the HIP library; raises (never falls back) when it is absent.  `path` (first call only) selects another build
    of the same library, e.g. the diagnostic one with in-kernel stamps (make STAMPS=1)."""
    global _lib, LIB_PATH
    if _lib is not None:
        return _lib
    if path is not None:
        LIB_PATH = path
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmrgan_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the training path)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.mrgan_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name != "mrgan_last_error":
            getattr(lib, name).restype = C.c_int
    # the handle-free SVM entries mix float, double and 64-bit arguments: declared, so ctypes converts plain Python numbers
    gram = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_int64]
    lib.mrgan_svm_gram.argtypes = gram + [C.c_void_p]
    lib.mrgan_debug_svm_gram.argtypes = gram + [C.c_int32, C.c_void_p]
    lib.mrgan_svm_solve.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_double, C.c_double, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mrgan_svm_decide.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mrgan_svm_kernel_matrix.argtypes = [C.c_int32] + gram + [C.c_void_p]
    lib.mrgan_debug_svm_kernel_matrix.argtypes = [C.c_int32] + gram + [C.c_int32, C.c_void_p]
    lib.mrgan_svm_solve_nu.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_double, C.c_double, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mrgan_svm_gram_group.argtypes = [C.POINTER(SvmGramItem), C.c_int32, C.c_int64, C.c_float, C.c_void_p]
    lib.mrgan_debug_svm_gram_group.argtypes = [C.POINTER(SvmGramItem), C.c_int32, C.c_int64, C.c_float, C.c_int32, C.c_void_p]
    lib.mrgan_svm_solve_group.argtypes = [C.POINTER(SvmSolveItem), C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    lib.mrgan_svm_decide_group.argtypes = [C.POINTER(SvmDecideItem), C.c_int32, C.c_int32, C.c_void_p]
    lib.mrgan_svm_kernel_matrix_group.argtypes = [C.c_int32, C.POINTER(SvmGramItem), C.c_int32, C.c_int64, C.c_float, C.c_void_p]
    lib.mrgan_debug_svm_kernel_matrix_group.argtypes = [C.c_int32, C.POINTER(SvmGramItem), C.c_int32, C.c_int64, C.c_float, C.c_int32, C.c_void_p]
    lib.mrgan_svm_solve_nu_group.argtypes = [C.POINTER(SvmSolveNuItem), C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p]
    # the handle-free PCA entries, declared for the same reason; the workspace queries return a byte count
    cov = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.mrgan_pca_mean.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.mrgan_pca_covariance_workspace_bytes.argtypes, lib.mrgan_pca_covariance_workspace_bytes.restype = [C.c_int64, C.c_int64], C.c_int64
    lib.mrgan_debug_pca_covariance_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    lib.mrgan_debug_pca_covariance_workspace_bytes.restype = C.c_int64
    lib.mrgan_pca_covariance.argtypes = cov + [C.c_void_p]
    lib.mrgan_debug_pca_covariance.argtypes = cov + [C.c_int32, C.c_int32, C.c_void_p]
    lib.mrgan_pca_eig_workspace_bytes.argtypes, lib.mrgan_pca_eig_workspace_bytes.restype = [C.c_int64, C.c_int64], C.c_int64
    lib.mrgan_pca_eig.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int32, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mrgan_debug_pca_orthonormalize.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_void_p]
    lib.mrgan_pca_transform.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int64, C.c_void_p]
    lib.mrgan_pca_inverse_transform.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_int64, C.c_void_p]
    _lib = lib
    return lib


class MrganError(RuntimeError):
    code = None              # the entry's status where a library call raised it


class DeviceCalls:
    """what the estimators over the handle-free entries share (svm.py, pca.py): the library call on the current stream of
    self.device, the per-stage device-event timer (self.time_stages, self.times_) and the refusal to run without a GPU"""
    _gpu_only = ('RBFSVM', 'mrgan_svm_*')                  # who refuses, and the entries it needs

    def _call(self, name, *args):
        lib = load_library()
        with torch.cuda.device(self.device):
            rc = getattr(lib, name)(*args, torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            err = MrganError("%s failed (%d): %s" % (name, rc, lib.mrgan_last_error().decode()))
            err.code = rc
            raise err

    def _timed(self, key, fn):
        if not self.time_stages:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(self.device))
        out = fn()
        b.record(torch.cuda.current_stream(self.device))
        b.synchronize()
        self.times_[key] = self.times_.get(key, 0.0) + a.elapsed_time(b) * 1e-3
        return out

    def _require_gpu(self):
        load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("%s runs on the GPU only (%s); no HIP device is visible and there is no CPU fallback" % self._gpu_only)


def _check(rc):
    if rc != 0:
        raise MrganError("libmrgan_hip error %d: %s" % (rc, load_library().mrgan_last_error().decode()))


def default_config(d_in, batch):
    cfg = Config()
    _check(load_library().mrgan_default_config(C.byref(cfg), int(d_in), int(batch)))
    return cfg


def noise_flags(noise):
    """handle flag of a layer-noise / device-z generator: 'irwin-hall' (the default: sums of 32 uniform bytes on the matrix
    cores) or 'gaussian' (true N(0, 1) by Box-Muller, FLAG_GAUSS_NOISE: a different random stream, slower epilogues)"""
    if noise not in NOISE_MODES:
        raise ValueError("noise must be one of %s, got %r" % (NOISE_MODES, noise))
    return FLAG_GAUSS_NOISE if noise == 'gaussian' else 0


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, dev):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def exchange_regions(region, grad_dtype, which):
    """the regions a data-parallel host all-reduces at exchange point `which` (a REGION_* of the phase protocol), given
    region(REGION_*) -> tensor and the gradient payload: a gradient exchange with grad_dtype 'bf16' is the bfloat16 body plus
    the four fp32 loss scalars"""
    if grad_dtype == 'bf16' and which in (REGION_GRAD_D, REGION_GRAD_G):
        d = which == REGION_GRAD_D
        return (region(REGION_GRAD_D_BF16 if d else REGION_GRAD_G_BF16), region(REGION_TAIL_D if d else REGION_TAIL_G))
    return (region(which),)


# What a single handle's argument struct and its group twin share.  The row pitch is that of the matrix itself, whether it
# is stacked [models, rows, D] or not; the structs hold raw pointers, so _refs keeps the tensors alive.
def _fill_disc(a, x_lab, labels, x_unl, z, idx_lab, idx_unl, stream_mode):
    a.x_lab, a.idx_lab, a.labels = _ptr(x_lab), _ptr(idx_lab), _ptr(labels)
    a.x_unl, a.idx_unl, a.z = _ptr(x_unl), _ptr(idx_unl), _ptr(z)
    a.ld_x_lab, a.ld_x_unl = x_lab.stride(-2), x_unl.stride(-2)
    a.stream_mode = stream_mode
    a._refs = (x_lab, labels, x_unl, z, idx_lab, idx_unl)
    return a


def _fill_gen(a, x_unl, z, idx_unl, stream_mode):
    a.x_unl, a.idx_unl, a.z = _ptr(x_unl), _ptr(idx_unl), _ptr(z)
    a.ld_x_unl = x_unl.stride(-2)
    a.stream_mode = stream_mode
    a._refs = (x_unl, z, idx_unl)
    return a


def _fill_sup(a, x, labels, idx, stream_mode, rows_valid):
    a.x, a.idx, a.labels = _ptr(x), _ptr(idx), _ptr(labels)
    a.ld_x = x.stride(-2)
    a.stream_mode, a.rows_valid = stream_mode, rows_valid
    a._refs = (x, labels, idx)
    return a


def _model_stride(t, stacked_dim):
    """elements between the models' parts of a tensor stacked [models, ...] (stacked_dim dimensions); 0: one tensor for all"""
    return t.stride(0) if t is not None and t.dim() == stacked_dim else 0


class Engine(object):
    """One handle = the Keras shared state of one mr_gan() call (weights, Adam slots, iteration counter)
    plus the three compiled functions of mr_gan.py:169-171."""

    def __init__(self, cfg, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("mr_gan_amd needs a HIP device; there is no CPU path")
        self.lib = load_library()
        self.cfg = cfg
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        nbytes = C.c_size_t()
        _check(self.lib.mrgan_workspace_bytes(C.byref(cfg), C.byref(nbytes)))
        self.workspace = torch.empty(nbytes.value + 512, dtype=torch.uint8, device=self.device)
        base = self.workspace.data_ptr()
        self._ws_off = (-base) % 256
        self.handle = C.c_void_p()
        _check(self.lib.mrgan_create(C.byref(cfg), C.c_void_p(base + self._ws_off), C.c_size_t(nbytes.value), _stream(),
                                     C.byref(self.handle)))
        self._keep = []

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            torch.cuda.synchronize(self.device)
            self.lib.mrgan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights (Keras order) ---------------------------------------------------------------------
    def num_tensors(self, net):
        n = C.c_int()
        _check(self.lib.mrgan_num_tensors(self.handle, net, C.byref(n)))
        return n.value

    def tensor_shape(self, net, idx):
        r, c = C.c_int(), C.c_int()
        _check(self.lib.mrgan_tensor_shape(self.handle, net, idx, C.byref(r), C.byref(c)))
        return r.value, c.value

    def set_weights(self, net, tensors):
        for i, t in enumerate(tensors):
            r, c = self.tensor_shape(net, i)
            t = _f32(t, self.device)
            if t.numel() != r * c:
                raise ValueError("tensor %d of net %d: expected %d x %d, got %s" % (i, net, r, c, tuple(t.shape)))
            _check(self.lib.mrgan_set_weights(self.handle, net, i, _ptr(t), _stream()))
            self._keep.append(t)
        torch.cuda.current_stream().synchronize()
        self._keep = []

    def _fetch(self, net, fn, *extra):
        out = []
        for i in range(self.num_tensors(net)):
            r, c = self.tensor_shape(net, i)
            t = torch.empty(r * c, dtype=torch.float32, device=self.device)
            _check(fn(self.handle, net, i, *extra, _ptr(t), _stream()))
            full = self.full_shape(net, i)
            out.append(t.cpu().numpy().reshape(full))
        return out

    def full_shape(self, net, idx):
        r, c = self.tensor_shape(net, idx)
        is_matrix = (net == NET_D and idx % 2 == 0) or (net == NET_G and idx in (0, 4, 6))
        return (r, c) if is_matrix else (c,)

    def get_weights(self, net):
        return self._fetch(net, self.lib.mrgan_get_weights)

    def get_slot(self, net, which):
        return self._fetch(net, self.lib.mrgan_get_slot, which)

    def set_slot(self, net, which, tensors):
        for i, t in enumerate(tensors):
            t = _f32(t, self.device)
            _check(self.lib.mrgan_set_slot(self.handle, net, i, which, _ptr(t), _stream()))
            self._keep.append(t)
        torch.cuda.current_stream().synchronize()
        self._keep = []

    def get_iterations(self):
        it = C.c_uint32()
        _check(self.lib.mrgan_get_iterations(self.handle, _stream(), C.byref(it)))
        return it.value

    def set_iterations(self, iterations, batch_counter=0):
        _check(self.lib.mrgan_set_iterations(self.handle, C.c_uint32(iterations), C.c_uint32(batch_counter), _stream()))

    # ---- the compiled functions -------------------------------------------------------------------------
    @staticmethod
    def disc_args(x_lab, labels, x_unl, z=None, idx_lab=None, idx_unl=None, stream_mode=0):
        return _fill_disc(DiscArgs(), x_lab, labels, x_unl, z, idx_lab, idx_unl, stream_mode)

    @staticmethod
    def gen_args(x_unl, z=None, idx_unl=None, stream_mode=0):
        return _fill_gen(GenArgs(), x_unl, z, idx_unl, stream_mode)

    def disc_step(self, args, first=0, last=-1, want_outputs=True):
        """train_batch_disc -> (loss_lab, loss_unl, train_err)"""
        out = (C.c_float * 3)()
        _check(self.lib.mrgan_disc_step(self.handle, C.byref(args), first, last, out if want_outputs else None, _stream()))
        return tuple(out) if want_outputs else None

    def gen_step(self, args, first=0, last=-1, want_outputs=True):
        """train_batch_gen -> loss_gen"""
        out = (C.c_float * 1)()
        _check(self.lib.mrgan_gen_step(self.handle, C.byref(args), first, last, out if want_outputs else None, _stream()))
        return out[0] if want_outputs else None

    @staticmethod
    def sup_args(x, labels, idx=None, stream_mode=0, rows_valid=0):
        return _fill_sup(SupArgs(), x, labels, idx, stream_mode, rows_valid)

    def sup_step(self, args, want_outputs=True):
        """one supervised train_on_batch of the NN baseline (mr_nn.py:117) -> (mse loss, training error of the batch)"""
        out = (C.c_float * 2)()
        _check(self.lib.mrgan_sup_step(self.handle, C.byref(args), out if want_outputs else None, _stream()))
        return tuple(out) if want_outputs else None

    # ---- autoencoder handles (FLAG_AUTOENCODER) ----------------------------------------------------------------------
    @staticmethod
    def ae_args(x, idx=None, stream_mode=0, rows_valid=0):
        a = AeArgs()
        a.x, a.idx, a.ld_x = _ptr(x), _ptr(idx), x.stride(-2)
        a.stream_mode, a.rows_valid = stream_mode, rows_valid
        a._refs = (x, idx)
        return a

    def ae_step(self, args, want_outputs=True):
        """one train_on_batch(x, x) of the autoencoder (loss 'mse', Adam) -> the loss of the batch"""
        out = (C.c_float * 1)()
        _check(self.lib.mrgan_ae_step(self.handle, C.byref(args), out if want_outputs else None, _stream()))
        return out[0] if want_outputs else None

    def ae_encode(self, x, idx=None, out=None):
        """mrgan_ae_encode -> codes fp32 [n, >= d_hidden[2]] (out: a buffer to write into; its further columns are left alone)"""
        n = x.shape[0] if idx is None else idx.numel()
        if out is None:
            out = torch.empty((n, self.cfg.d_hidden[2]), dtype=torch.float32, device=self.device)
        _check(self.lib.mrgan_ae_encode(self.handle, _ptr(x), _ptr(idx), C.c_int64(x.stride(0)), C.c_int64(n), _ptr(out),
                                        C.c_int64(out.stride(0)), _stream()))
        return out

    def ae_reconstruct(self, x, idx=None, out=None, want_out=True, want_mse=True):
        """mrgan_ae_reconstruct -> (y fp32 [n, >= d_in] or None, mse over all n x d_in elements or None)"""
        n = x.shape[0] if idx is None else idx.numel()
        if out is None and want_out:
            out = torch.empty((n, self.cfg.d_in), dtype=torch.float32, device=self.device)
        mse = C.c_float()
        _check(self.lib.mrgan_ae_reconstruct(self.handle, _ptr(x), _ptr(idx), C.c_int64(x.stride(0)), C.c_int64(n), _ptr(out),
                                             C.c_int64(out.stride(0) if out is not None else 0), C.byref(mse) if want_mse else None,
                                             _stream()))
        return out, (mse.value if want_mse else None)

    # ---- model groups (cfg.models > 1): G equal-shape trainings in one launch set ----------------------------------
    @property
    def models(self):
        return max(1, int(self.cfg.models))

    def select_model(self, model):
        """the model that set_weights / get_weights, get_slot / set_slot, eval_error, predict_logits (and debug_buffer) address"""
        _check(self.lib.mrgan_select_model(self.handle, int(model)))

    @staticmethod
    def sup_group_args(x, labels, idx=None, stream_mode=0, rows_valid=0, x_model_stride=None, idx_model_stride=None,
                       labels_model_stride=None):
        """x [models, rows, D] (or [rows, D] with x_model_stride = 0: one matrix, gathered through idx [models, n]); labels
        [models, n].  The strides default to those of the tensors' first dimension."""
        a = _fill_sup(SupGroupArgs(), x, labels, idx, stream_mode, rows_valid)
        a.x_model_stride = _model_stride(x, 3) if x_model_stride is None else x_model_stride
        a.idx_model_stride = _model_stride(idx, 2) if idx_model_stride is None else idx_model_stride
        a.labels_model_stride = _model_stride(labels, 2) if labels_model_stride is None else labels_model_stride
        return a

    def sup_step_group(self, args, want_outputs=True):
        """sup_step once per model of a group handle, as one launch set -> [(mse loss, training error)] per model"""
        out = (C.c_float * (2 * MAX_MODELS))()
        _check(self.lib.mrgan_sup_step_group(self.handle, C.byref(args), out if want_outputs else None, _stream()))
        return [(out[2 * m], out[2 * m + 1]) for m in range(self.models)] if want_outputs else None

    # the GAN sub-steps of a group handle: stacked [models, ...] tensors, strides derived as in sup_group_args
    @staticmethod
    def disc_group_args(x_lab, labels, x_unl, z=None, idx_lab=None, idx_unl=None, stream_mode=0):
        """x_lab / x_unl [models, rows, D] (or [rows, D]: one matrix every model gathers from through its idx_* [models, n]);
        labels [models, n]; z [models, n, noise] or None (model m draws z on the device with seed + m)"""
        a = _fill_disc(DiscGroupArgs(), x_lab, labels, x_unl, z, idx_lab, idx_unl, stream_mode)
        ms = _model_stride
        a.x_lab_model_stride, a.idx_lab_model_stride, a.labels_model_stride = ms(x_lab, 3), ms(idx_lab, 2), ms(labels, 2)
        a.x_unl_model_stride, a.idx_unl_model_stride, a.z_model_stride = ms(x_unl, 3), ms(idx_unl, 2), ms(z, 3)
        return a

    @staticmethod
    def gen_group_args(x_unl, z=None, idx_unl=None, stream_mode=0):
        a = _fill_gen(GenGroupArgs(), x_unl, z, idx_unl, stream_mode)
        a.x_unl_model_stride, a.idx_unl_model_stride, a.z_model_stride = _model_stride(x_unl, 3), _model_stride(idx_unl, 2), _model_stride(z, 3)
        return a

    def disc_step_group(self, args, want_outputs=True):
        """disc_step once per model of a group handle, as one launch set -> [(loss_lab, loss_unl, train_err)] per model"""
        out = (C.c_float * (3 * MAX_MODELS))()
        _check(self.lib.mrgan_disc_step_group(self.handle, C.byref(args), out if want_outputs else None, _stream()))
        return [tuple(out[3 * m:3 * m + 3]) for m in range(self.models)] if want_outputs else None

    def gen_step_group(self, args, want_outputs=True):
        """gen_step once per model of a group handle, as one launch set -> [loss_gen] per model"""
        out = (C.c_float * MAX_MODELS)()
        _check(self.lib.mrgan_gen_step_group(self.handle, C.byref(args), out if want_outputs else None, _stream()))
        return [out[m] for m in range(self.models)] if want_outputs else None

    def train_pair_group(self, dargs, gargs):
        _check(self.lib.mrgan_train_pair_group(self.handle, C.byref(dargs), C.byref(gargs), _stream()))

    FP8_DRY_PASSES = 5
    FP8_CAL_QUERY, FP8_CAL_BEGIN, FP8_CAL_END_PASS, FP8_CAL_DONE = 0, 1, 2, 3

    def fp8_calibration(self, kind, action):
        """phase-wise hosts (mr_gan_amd/dist.py): settle the fp8 scales of sub-step kind 0 (D) / 1 (G); see mrgan_abi.h"""
        rc = self.lib.mrgan_fp8_calibration(self.handle, int(kind), int(action), _stream())
        if rc < 0:
            _check(rc)
        return rc

    def train_pair(self, dargs, gargs):
        _check(self.lib.mrgan_train_pair(self.handle, C.byref(dargs), C.byref(gargs), _stream()))

    def set_tuning(self, knob, value):
        """launch-structure knobs (TUNE_*): results stay within rounding"""
        _check(self.lib.mrgan_set_tuning(self.handle, int(knob), int(value)))

    def pair_hint(self, on=True):
        """the next disc_step is followed by a gen_step with device-drawn z: share the generator pass (no-op with synced statistics)"""
        _check(self.lib.mrgan_pair_hint(self.handle, 1 if on else 0))

    def eval_error(self, x, labels, idx=None):
        """test_batch -> err"""
        err = C.c_float()
        _check(self.lib.mrgan_eval_error(self.handle, _ptr(x), _ptr(idx), C.c_int64(x.stride(0)), _ptr(labels),
                                         C.c_int64(labels.numel() if idx is None else idx.numel()), C.byref(err), _stream()))
        return err.value

    def predict_logits(self, x, idx=None):
        n = x.shape[0] if idx is None else idx.numel()
        out = torch.empty((n, self.cfg.num_classes), dtype=torch.float32, device=self.device)
        _check(self.lib.mrgan_predict_logits(self.handle, _ptr(x), _ptr(idx), C.c_int64(x.stride(0)), C.c_int64(n), _ptr(out),
                                             _stream()))
        return out

    def _map_args(self, a, x, targets, objective, post, idx, out, classes_out):
        """the fields mrgan_saliency_args and mrgan_attribution_args share, the buffers allocated where not given -> (out, classes_out)"""
        n = x.shape[0] if idx is None else idx.numel()
        if out is None:
            out = torch.empty((n, self.cfg.d_in), dtype=torch.float32, device=self.device)
        if classes_out is None:
            classes_out = torch.empty((n,), dtype=torch.int32, device=self.device)
        a.x, a.idx, a.ld_x, a.n = _ptr(x), _ptr(idx), x.stride(0), n
        a.targets, a.objective, a.post = _ptr(targets), int(objective), int(post)
        a.out, a.ld_out, a.classes_out = _ptr(out), out.stride(0), _ptr(classes_out)
        return out, classes_out

    def input_gradient(self, x, targets=None, objective=SAL_XENT, post=SAL_RAW, idx=None, out=None, classes_out=None):
        """mrgan_input_gradient -> (maps fp32 [n, >= d_in], classes int32 [n]): per row the gradient of `objective` (SAL_*) at
        its target class -- targets[i], or the predicted class -- with respect to the input row, raw or as the reference's
        heat-map (post = SAL_HEATMAP).  out / classes_out: buffers to write into (out may have a row pitch above d_in; its
        further columns are left alone)."""
        a = SaliencyArgs()
        res = self._map_args(a, x, targets, objective, post, idx, out, classes_out)
        _check(self.lib.mrgan_input_gradient(self.handle, C.byref(a), _stream()))
        return res

    def attribution(self, x, targets=None, objective=SAL_XENT, post=SAL_RAW, idx=None, out=None, classes_out=None,
                    method=ATTR_NOISE, draws=1, sigma_input=0.0, sigma_hidden=0.0, baseline=None, multiply=0):
        """mrgan_attribution -> (maps fp32 [n, >= d_in], classes int32 [n]): input_gradient averaged over `draws` forwards on
        the device -- ATTR_NOISE: with GaussianNoise of sigma_input at the input and sigma_hidden behind dense 1 .. 4
        (SmoothGrad); ATTR_PATH: at the midpoints of `draws` pieces of the path from baseline (device fp32 [d_in], or None:
        zeros) to the row -- times (x - baseline) when multiply is 1.  The defaults are input_gradient itself."""
        a = AttributionArgs()
        res = self._map_args(a, x, targets, objective, post, idx, out, classes_out)
        a.method, a.draws, a.sigma_input, a.sigma_hidden = int(method), int(draws), float(sigma_input), float(sigma_hidden)
        a.baseline, a.multiply = _ptr(baseline), int(multiply)
        _check(self.lib.mrgan_attribution(self.handle, C.byref(a), _stream()))
        return res

    def read_metrics(self, reset=True):
        out = (C.c_float * 8)()
        _check(self.lib.mrgan_read_metrics(self.handle, out, 1 if reset else 0, _stream()))
        return list(out)

    def profile_begin(self):
        _check(self.lib.mrgan_profile_begin(self.handle))

    def profile_end(self, max_kernels=64):
        """-> {kernel instantiation name: (total ms, launches, algorithmic flops, algorithmic bytes)} since profile_begin"""
        names = C.create_string_buffer(max_kernels * PROF_NAME_LEN)
        ms, cnt = (C.c_float * max_kernels)(), (C.c_int32 * max_kernels)()
        fl, by, n = (C.c_double * max_kernels)(), (C.c_double * max_kernels)(), C.c_int()
        _check(self.lib.mrgan_profile_end(self.handle, _stream(), max_kernels, names, ms, cnt, fl, by, C.byref(n)))
        out = {}
        for i in range(n.value):
            name = names.raw[i * PROF_NAME_LEN:(i + 1) * PROF_NAME_LEN].split(b"\0")[0].decode()
            if name != "(start)":
                out[name] = (ms[i], cnt[i], fl[i], by[i])
        return out

    def region(self, which):
        """torch view of a workspace region (aliases library memory: used for all-reduce): fp32, bfloat16 for the
        REGION_GRAD_*_BF16 regions of a FLAG_GRAD_BF16 handle."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib.mrgan_region(self.handle, which, C.byref(p), C.byref(n)))
        off = p.value - self.workspace.data_ptr()
        return self.workspace[off:off + n.value].view(torch.bfloat16 if which in (REGION_GRAD_D_BF16, REGION_GRAD_G_BF16) else torch.float32)

    @property
    def grad_dtype(self):
        """payload of the gradient exchanges, decided by the handle: 'bf16' (FLAG_GRAD_BF16) or None (fp32)"""
        return 'bf16' if self.cfg.flags & FLAG_GRAD_BF16 else None

    def exchange_regions(self, which):
        return exchange_regions(self.region, self.grad_dtype, which)

    def debug_ablate(self, bits):
        _check(self.lib.mrgan_debug_ablate(self.handle, int(bits)))

    def debug_buffer(self, kind, l, nseg=3):
        """activation buffer (0 xin[l], 1 dpre[l], 2 features) as a float32 tensor [nseg, S, ld] (a copy)"""
        p, rows, ld, es = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        _check(self.lib.mrgan_debug_buffer(self.handle, kind, l, C.byref(p), C.byref(rows), C.byref(ld), C.byref(es)))
        off = p.value - self.workspace.data_ptr()
        n = nseg * rows.value * ld.value * es.value
        raw = self.workspace[off:off + n]
        t = raw.view(torch.bfloat16 if es.value == 2 else torch.float32)
        return t.reshape(nseg, rows.value, ld.value).float().clone()

    def debug_noise(self, site, seg, step, rows, cols, row0=0):
        out = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        _check(self.lib.mrgan_debug_noise(self.handle, site, seg, step, row0, rows, cols, _ptr(out), _stream()))
        return out


class DebugGemmDesc(C.Structure):
    """mrgan_debug_gemm_desc (include/mrgan_debug.h)"""
    _fields_ = [
        ("dtype", C.c_int32), ("op", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
        ("nbatch", C.c_int32), ("splits", C.c_int32), ("kchunk", C.c_int32), ("kc_cfg", C.c_int32), ("tune_bits", C.c_int32),
        ("seg_stride", C.c_int32), ("seg_rows", C.c_int32),
        ("a", C.c_void_p), ("a_bs", C.c_int64), ("a_si", C.c_int64), ("a_sk", C.c_int64),
        ("b", C.c_void_p), ("b_bs", C.c_int64), ("b_sk", C.c_int64), ("b_sj", C.c_int64),
        ("act", C.c_int32), ("n_valid", C.c_int32), ("bias", C.c_void_p),
        ("out", C.c_void_p), ("out_bs", C.c_int64), ("ldo", C.c_int32),
        ("sigma", C.c_float), ("site", C.c_uint32), ("seg0", C.c_uint32), ("seg_step", C.c_int32),
        ("iter_step", C.c_uint32), ("row0", C.c_uint32), ("iter", C.c_uint32), ("seed", C.c_uint64),
        ("mask", C.c_void_p), ("mask_bs", C.c_int64), ("ldm", C.c_int32),
        ("h", C.c_void_p), ("h_bs", C.c_int64), ("ldh", C.c_int32),
        ("cs_mode", C.c_int32), ("cs1", C.c_void_p), ("cs2", C.c_void_p), ("ldcs", C.c_int32),
        ("bn_mu", C.c_void_p), ("bn_rstd", C.c_void_p),
        ("slab", C.c_void_p), ("slab_stride", C.c_int64),
        ("q8", C.c_void_p), ("q8_bs", C.c_int64), ("ldq8", C.c_int32),
        ("q8t", C.c_void_p), ("q8t_bs", C.c_int64), ("ldq8t", C.c_int32),
        ("slot_a", C.c_void_p), ("slot_b", C.c_void_p), ("slot_o", C.c_void_p),
        ("gauss", C.c_int32),
    ]


class DebugFold(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("stride", C.c_int64), ("nsrc", C.c_int32), ("n", C.c_int32),
                ("ngroups", C.c_int32)]


def debug_gemm_desc(**kw):
    """a DebugGemmDesc from keywords; tensors become device pointers (and are kept alive by the descriptor)"""
    d = DebugGemmDesc()
    d.kc_cfg, d.nbatch, d.splits = -1, 1, 1
    d._refs = []
    for name, v in kw.items():
        if isinstance(v, torch.Tensor):
            d._refs.append(v)
            v = v.data_ptr()
        setattr(d, name, v)
    return d


def debug_gemm_launch(descs, grouped=False, fold=None):
    """One launch through mrgan_debug_gemm_launch -> (return code, kernel name).  Codes the launchers use to refuse a product
    (-3, and 1 for the grouped launch) and the entry's own -1 are returned, anything else raises."""
    if isinstance(descs, DebugGemmDesc):
        descs = [descs]
    arr = (DebugGemmDesc * len(descs))(*descs)
    name = C.create_string_buffer(PROF_NAME_LEN)
    f = None
    if fold is not None:
        src, dst, stride, nsrc, n, ngroups = fold
        f = DebugFold(src.data_ptr(), dst.data_ptr(), stride, nsrc, n, ngroups)
    rc = load_library().mrgan_debug_gemm_launch(arr, len(descs), 1 if grouped else 0, C.byref(f) if f is not None else None,
                                                name, PROF_NAME_LEN, _stream())
    if rc not in (0, 1, -1, -3):
        _check(rc)
    return rc, name.value.decode()


# ---- the non-GEMM kernels: one descriptor per launcher (include/mrgan_debug.h) ----------------------------------------
HEAD_LAB, HEAD_UNL, HEAD_FAKE, HEAD_EVAL, HEAD_LOGITS, HEAD_MSE = range(6)
ADAM_FUSED, ADAM_REDUCE_ONLY, ADAM_FROM_FLAT = range(3)


class DebugStageSeg(C.Structure):
    """mrgan_debug_stage_seg"""
    _fields_ = [
        ("src", C.c_void_p), ("idx", C.c_void_p), ("ld", C.c_int64),
        ("rows", C.c_int32), ("cols", C.c_int32), ("cols_pad", C.c_int32),
        ("out", C.c_void_p), ("ldo", C.c_int32),
        ("sigma", C.c_float), ("site", C.c_uint32), ("seg", C.c_uint32),
        ("gen", C.c_int32), ("stream", C.c_int32), ("iter_off", C.c_uint32),
        ("models", C.c_int32), ("src_ms", C.c_int64), ("idx_ms", C.c_int64), ("out_ms", C.c_int64),
    ]


class DebugStageDesc(C.Structure):
    """mrgan_debug_stage_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("s", DebugStageSeg * 5), ("nseg", C.c_int32),
        ("seed", C.c_uint64), ("row0", C.c_uint32), ("iter", C.c_uint32), ("batch", C.c_uint32), ("gauss", C.c_int32),
    ]


class DebugBnApplyDesc(C.Structure):
    """mrgan_debug_bn_apply_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("h", C.c_void_p), ("out", C.c_void_p), ("ld", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("cs1", C.c_void_p), ("cs2", C.c_void_p), ("npart", C.c_int32), ("ldcs", C.c_int32),
        ("count", C.c_float), ("eps", C.c_float), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("mu", C.c_void_p), ("rstd", C.c_void_p), ("cs_seg_stride", C.c_int64), ("nseg", C.c_int32), ("seg_rows", C.c_int64),
    ]


class DebugBnBwdDesc(C.Structure):
    """mrgan_debug_bn_bwd_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("dy", C.c_void_p), ("h", C.c_void_p), ("dpre", C.c_void_p),
        ("ld", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("cs1", C.c_void_p), ("cs2", C.c_void_p), ("npart", C.c_int32), ("ldcs", C.c_int32), ("count", C.c_float),
        ("gamma", C.c_void_p), ("mu", C.c_void_p), ("rstd", C.c_void_p), ("db_part", C.c_void_p),
    ]


class DebugHeadDesc(C.Structure):
    """mrgan_debug_head_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("f", C.c_void_p), ("f_bs", C.c_int64), ("ldf", C.c_int32),
        ("rows", C.c_int32), ("nseg", C.c_int32), ("seg_kind", C.c_int32 * 3),
        ("feat", C.c_int32), ("feat_valid", C.c_int32), ("classes", C.c_int32),
        ("w", C.c_void_p), ("ldw", C.c_int32), ("b", C.c_void_p),
        ("labels", C.c_void_p), ("labels_stream", C.c_int32), ("batch", C.c_uint32),
        ("inv_count", C.c_float), ("unl_weight", C.c_float),
        ("logits", C.c_void_p), ("logits_bs", C.c_int64),
        ("dpre", C.c_void_p), ("dpre_bs", C.c_int64), ("ldd", C.c_int32),
        ("part", C.c_void_p), ("part_stride", C.c_int64), ("off_db", C.c_int32), ("off_dbf", C.c_int32),
        ("loss_part", C.c_void_p),
        ("models", C.c_int32), ("model_stride", C.c_int64), ("labels_ms", C.c_int64),
        ("err_count", C.c_void_p),
        ("q8", C.c_void_p), ("q8_bs", C.c_int64), ("ldq8", C.c_int32),
        ("q8t", C.c_void_p), ("q8t_bs", C.c_int64), ("ldq8t", C.c_int32),
        ("q8_slot", C.c_void_p),
    ]


class DebugHeadWideDesc(C.Structure):
    """mrgan_debug_head_wide_desc"""
    _fields_ = [("h", DebugHeadDesc), ("mask", C.c_void_p), ("mask_bs", C.c_int64), ("ldm", C.c_int32), ("w6c", C.c_void_p), ("w6r", C.c_void_p)]


class DebugFmDesc(C.Structure):
    """mrgan_debug_fm_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("cs", C.c_void_p), ("npart_fake", C.c_int32), ("npart_real", C.c_int32), ("ldcs", C.c_int32),
        ("count", C.c_float), ("grad_scale", C.c_float), ("feat", C.c_int32), ("feat_valid", C.c_int32),
        ("mask", C.c_void_p), ("ldm", C.c_int32), ("dpre", C.c_void_p), ("ldd", C.c_int32), ("rows", C.c_int32),
        ("loss_out", C.c_void_p), ("accum", C.c_void_p),
        ("q8", C.c_void_p), ("ldq8", C.c_int32), ("q8_slot", C.c_void_p),
        ("lscratch", C.c_void_p), ("lcount", C.c_void_p),
    ]


class DebugChainOp(C.Structure):
    """mrgan_debug_chain_op"""
    _fields_ = [
        ("K", C.c_int32), ("N", C.c_int32), ("n_valid", C.c_int32),
        ("W", C.c_void_p), ("bias", C.c_void_p), ("sigma", C.c_float), ("site", C.c_uint32),
        ("out", C.c_void_p), ("out_bs", C.c_int64), ("ldo", C.c_int32),
        ("mask", C.c_void_p), ("mask_bs", C.c_int64), ("ldm", C.c_int32),
        ("cs", C.c_void_p), ("ldcs", C.c_int32),
    ]


class DebugChainDesc(C.Structure):
    """mrgan_debug_chain_desc"""
    _fields_ = [
        ("variant", C.c_int32), ("fwd", DebugChainOp * 3), ("dx", DebugChainOp * 3),
        ("rows", C.c_int32), ("nseg", C.c_int32), ("block_rows", C.c_int32),
        ("models", C.c_int32), ("model_stride", C.c_int64),
        ("a", C.c_void_p), ("a_bs", C.c_int64), ("lda", C.c_int32), ("a_cols", C.c_int32),
        ("seg0", C.c_int32), ("seed", C.c_uint64), ("row0", C.c_uint32), ("gauss", C.c_int32),
        ("iter", C.c_uint32), ("batch", C.c_uint32),
        ("head", DebugHeadDesc),
        ("fm", DebugFmDesc), ("fm_feat", C.c_void_p), ("fm_ldf", C.c_int32),
    ]


class DebugAdamTile(C.Structure):
    """mrgan_debug_adam_tile"""
    _fields_ = [
        ("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p),
        ("g", C.c_void_p), ("nslab", C.c_int32), ("slab_stride", C.c_int64),
        ("flat", C.c_void_p), ("flat16", C.c_void_p), ("w16", C.c_void_p), ("wt16", C.c_void_p),
        ("w8", C.c_void_p), ("w8t", C.c_void_p), ("w8_slot", C.c_void_p),
        ("ld", C.c_int32), ("ldt", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
    ]


class DebugAdamDesc(C.Structure):
    """mrgan_debug_adam_desc"""
    _fields_ = [
        ("tiles", C.POINTER(DebugAdamTile)), ("ntiles", C.c_int32), ("mode", C.c_int32),
        ("b1", C.c_float), ("b2", C.c_float), ("eps", C.c_float),
        ("iter", C.c_uint32), ("batch", C.c_uint32), ("lr_t", C.c_float),
        ("loss_part", C.c_void_p), ("nloss_part", C.c_int32), ("inv_rows", C.c_float), ("step_out", C.c_void_p), ("accum", C.c_void_p),
        ("flat_tail", C.c_void_p),
        ("publish_next", C.c_int32), ("advance_batch", C.c_int32), ("lr", C.c_float),
        ("models", C.c_int32), ("model_stride", C.c_int64),
    ]


def _debug_fill(d, kw):
    """keywords -> fields of a descriptor; tensors become device pointers (and are kept alive by the descriptor)"""
    d._refs = []
    for name, v in kw.items():
        if isinstance(v, torch.Tensor):
            d._refs.append(v)
            v = v.data_ptr()
        elif name == "seg_kind":
            v = (C.c_int32 * 3)(*(list(v) + [0] * (3 - len(v))))
        setattr(d, name, v)
    return d


def _debug_rc(rc):
    """the launchers' refusal (-3) and the entries' own (-1) are returned, anything else raises"""
    if rc not in (0, -1, -3):
        _check(rc)
    return rc


def debug_stage(segs, **kw):
    """segs: [dict of DebugStageSeg fields], at most five; kw: the launch's own fields"""
    d = _debug_fill(DebugStageDesc(), kw)
    keep = [_debug_fill(DebugStageSeg(), s) for s in segs]
    for i, s in enumerate(keep[:5]):
        d.s[i] = s
    d.nseg = len(segs)
    return _debug_rc(load_library().mrgan_debug_stage(C.byref(d), _stream()))


def debug_reduce_partials(src, nsrc, stride, n, ngroups, dst, models=1, model_stride=0):
    return _debug_rc(load_library().mrgan_debug_reduce_partials(_ptr(src), int(nsrc), C.c_int64(stride), int(n), int(ngroups), _ptr(dst),
                                                                int(models), C.c_int64(model_stride), _stream()))


def debug_colsum_finalize(part1, part2, npart, ld, n, out, nseg=1):
    return _debug_rc(load_library().mrgan_debug_colsum_finalize(_ptr(part1), _ptr(part2), int(npart), int(ld), int(n), _ptr(out), int(nseg),
                                                                _stream()))


def debug_bn_apply(**kw):
    return _debug_rc(load_library().mrgan_debug_bn_apply(C.byref(_debug_fill(DebugBnApplyDesc(), kw)), _stream()))


def debug_bn_bwd(**kw):
    return _debug_rc(load_library().mrgan_debug_bn_bwd(C.byref(_debug_fill(DebugBnBwdDesc(), kw)), _stream()))


def debug_head(**kw):
    return _debug_rc(load_library().mrgan_debug_head(C.byref(_debug_fill(DebugHeadDesc(), kw)), _stream()))


def debug_head_wide(mask=None, mask_bs=0, ldm=0, w6c=None, w6r=None, **kw):
    """launch_w6_split + launch_head_wide; kw: the fields of the head descriptor"""
    d = DebugHeadWideDesc()
    d.h = _debug_fill(DebugHeadDesc(), kw)
    _debug_fill(d, dict(mask=mask, mask_bs=mask_bs, ldm=ldm, w6c=w6c, w6r=w6r))
    return _debug_rc(load_library().mrgan_debug_head_wide(C.byref(d), _stream()))


def debug_fm(**kw):
    return _debug_rc(load_library().mrgan_debug_fm(C.byref(_debug_fill(DebugFmDesc(), kw)), _stream()))


CH_V_DTAIL, CH_V_GFWD, CH_V_GBWD = range(3)


def debug_chain(fwd=(), dx=(), head=None, fm=None, **kw):
    """One launch of the row-block chain kernel through mrgan_debug_chain -> (return code, kernel name).  fwd / dx: up to three
    dicts of DebugChainOp fields each, head / fm: dicts of DebugHeadDesc / DebugFmDesc fields, kw: the launch's own fields.
    Pointers may be tensors or plain integers (a refused descriptor is never dereferenced, so the refusals need no device)."""
    d = _debug_fill(DebugChainDesc(), kw)
    keep = [d._refs]
    for name, ops in (("fwd", fwd), ("dx", dx)):
        for i, o in enumerate(list(ops)[:3]):
            op = _debug_fill(DebugChainOp(), o)
            keep.append(op._refs)
            getattr(d, name)[i] = op
    if head is not None:
        h = _debug_fill(DebugHeadDesc(), head)
        keep.append(h._refs)
        d.head = h
    if fm is not None:
        f = _debug_fill(DebugFmDesc(), fm)
        keep.append(f._refs)
        d.fm = f
    name = C.create_string_buffer(PROF_NAME_LEN)
    stream = _stream() if torch.cuda.is_available() else None
    rc = _debug_rc(load_library().mrgan_debug_chain(C.byref(d), name, PROF_NAME_LEN, stream))
    del keep
    return rc, name.value.decode()


def debug_adam(tiles, **kw):
    """tiles: [dict of DebugAdamTile fields] -> (return code, the four words of the published `next` DevState as uint32, or
    None when publish_next is not set)"""
    arr = (DebugAdamTile * len(tiles))(*[_debug_fill(DebugAdamTile(), t) for t in tiles])
    d = _debug_fill(DebugAdamDesc(), kw)
    d.tiles, d.ntiles = arr, len(tiles)
    nxt = (C.c_uint32 * 4)()
    rc = _debug_rc(load_library().mrgan_debug_adam(C.byref(d), nxt, _stream()))
    return rc, (np.array(list(nxt), dtype=np.uint32) if d.publish_next and rc == 0 else None)


def debug_gemm(dtype, op, a, b, bias=None, act=0, splits=1):
    """Raw kernel-level product for parity tests. op 0: act(a b + bias); 1: a b^T; 2: a^T b.  fp32 tensors in and out: the
    operands are rounded to the dtype here (to nearest even), the bf16 forward gets the transposed weight copy it reads,
    and the weight gradient's slabs are added in index order."""
    td = torch.bfloat16 if dtype == BF16 else torch.float32
    m = a.shape[0]
    k, n = (a.shape[1], b.shape[1]) if op == 2 else b.shape
    if n % 64 or k % 64:
        raise ValueError("debug_gemm: n and k must be multiples of 64")
    a, b = a.to(td).contiguous(), b.to(td).contiguous()
    if op == 0:
        wt = dtype == BF16
        out = torch.zeros((m, n), dtype=td, device=a.device)
        d = debug_gemm_desc(dtype=dtype, op=0, m=m, n=n, k=k, a=a, a_si=k, a_sk=1, b=b.t().contiguous() if wt else b,
                            b_sk=1 if wt else n, b_sj=k if wt else 1, act=act, n_valid=n, bias=bias, out=out, ldo=n)
    elif op == 1:
        out = torch.zeros((m, k), dtype=td, device=a.device)
        d = debug_gemm_desc(dtype=dtype, op=1, m=m, n=k, k=n, a=a, a_si=n, a_sk=1, b=b, b_sk=1, b_sj=n, n_valid=k, out=out, ldo=k)
    else:
        splits = max(1, splits)
        out = torch.zeros((splits, k, n), dtype=torch.float32, device=a.device)
        d = debug_gemm_desc(dtype=dtype, op=2, m=k, n=n, k=m, splits=splits, kchunk=-(-(-(-m // splits)) // 64) * 64,
                            a=a, a_si=1, a_sk=k, b=b, b_sk=n, b_sj=1, slab=out, slab_stride=k * n, ldo=n)
    _check(debug_gemm_launch(d)[0])
    for s in range(1, splits if op == 2 else 0):
        out[0] += out[s]
    return out[0] if op == 2 else out.float()


def fp8_slots(rows, device="cuda:0"):
    """[(amax, scale, inv_scale, target)] -> device tensor int32 [n][4], the words of n Fp8Slot (csrc/common.h); row i is the
    slot pointer a descriptor takes"""
    return torch.from_numpy(np.array(rows, dtype=np.float32).reshape(-1, 4).view(np.int32)).to(device)


def fp8_slots_read(slots):
    """-> (amax_bits uint32 [n], float32 [n][3] = scale, inv_scale, target)"""
    w = slots.cpu().numpy()
    return w[:, 0].view(np.uint32).copy(), w[:, 1:].copy().view(np.float32)


def debug_quant8(src, src_bs, ld, rows, cols, nb, prow, slot, fmt, dst=None, dst_bs=0, ldd=0, dstt=None, dstt_bs=0, lddt=0):
    """One launch of the bf16 -> fp8 quantiser through mrgan_debug_quant8 -> return code (0, or the refusals -1 / -3)"""
    rc = load_library().mrgan_debug_quant8(_ptr(src), C.c_int64(src_bs), int(ld), int(rows), int(cols), int(nb), int(prow), _ptr(dst),
                                           C.c_int64(dst_bs), int(ldd), _ptr(dstt), C.c_int64(dstt_bs), int(lddt), _ptr(slot), int(fmt),
                                           _stream())
    if rc not in (0, -1, -3):
        _check(rc)
    return rc


def debug_fp8_update_scales(slots):
    """the delayed-scaling update on a tensor of slots (fp8_slots), in place"""
    _check(load_library().mrgan_debug_fp8_update_scales(_ptr(slots), int(slots.shape[0]), _stream()))


def debug_tr_probe(device="cuda:0"):
    out = torch.zeros(1024, dtype=torch.int16, device=device)
    _check(load_library().mrgan_debug_tr_probe(_ptr(out), _stream()))
    return out.cpu().numpy().astype(np.uint16).reshape(2, 64, 8)


def debug_gemm_time(op, m, n, k, nbatch=1, splits=1, reps=50, ablate=0, kc_cfg=-1):
    us = C.c_float()
    _check(load_library().mrgan_debug_gemm_time(op, m, n, k, nbatch, splits, reps, ablate, kc_cfg, C.byref(us)))
    return us.value


def debug_gemm_fp8(a, b, bias=None, act=0, scale_a=1.0, scale_b=1.0, reps=0, kc_cfg=-1):
    """e4m3 forward product act((q(a sa) q(b sb)) / (sa sb) + bias) -> (fp32 [m, n] result, average us per launch if reps > 0)"""
    m, k = a.shape
    n = b.shape[1]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    us = C.c_float()
    _check(load_library().mrgan_debug_gemm_fp8(m, n, k, _ptr(a), _ptr(b), _ptr(bias), act, C.c_float(scale_a), C.c_float(scale_b), _ptr(out),
                                               reps, C.byref(us), int(kc_cfg), _stream()))
    return out, us.value
