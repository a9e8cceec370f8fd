/* libmrgan_hip -- C ABI of the MI355X-native mr_gan training path.
 *
 * Drop-in boundary: the three Theano-compiled callables of the reference,
 *     train_batch_disc([phase, x_lab, labels, x_unl, noise]) -> [loss_lab, loss_unl, train_err]   (mr_gan.py:169)
 *     train_batch_gen ([phase, x_unl, noise])               -> loss_gen                           (mr_gan.py:170)
 *     test_batch      ([phase, x_lab, labels])              -> test_err                           (mr_gan.py:171)
 * plus the state they close over (Keras shared variables: weights of mr_gan.py:110-128, the two Adam update
 * lists and their single iteration counter, mr_gan.py:165-167).
 *
 * Conventions: every function returns 0 on success and a negative code on failure; the message is available
 * from mrgan_last_error() (thread-local).  Nothing throws across the ABI.  All pointers named *_dev are device
 * pointers (HBM); the caller owns inputs and outputs, the handle owns weights, optimiser state and workspace.
 * Calls are asynchronous on `stream` unless a host output pointer is passed (then the call synchronises the
 * stream before returning).  One handle per device; a handle is not thread-safe.  Training state lives in the handle only
 * (tuning and the diagnostic switches of mrgan_debug.h are per handle; nothing reads the environment); the library keeps two
 * process-wide caches, both keyed by device id and safe to share between threads: which kernels have had their LDS limit
 * raised on a device, and the mel filter banks of mrgan_logmel per (device, sr, n_mels).
 * No torch types appear here: the Python host passes tensor.data_ptr() and the raw hipStream_t.
 */
#ifndef MRGAN_ABI_H
#define MRGAN_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrgan_handle mrgan_handle;
typedef void* mrgan_stream;               /* hipStream_t */

/* arithmetic of the dense stacks: fp32 MFMA (parity) / bf16 MFMA (speed) / fp8: the discriminator's dense products on
 * the fp8 matrix cores (e4m3 activations and weights, e5m2 gradients, fp32 accumulate, delayed per-tensor power-of-two
 * scales; the generator, the loss head and evaluation stay bf16; every padded width becomes a multiple of 128) */
enum { MRGAN_F32 = 0, MRGAN_BF16 = 1, MRGAN_FP8 = 2 };
enum { MRGAN_NET_G = 0, MRGAN_NET_D = 1 };
enum {
    MRGAN_FLAG_SYNC_STATS = 1,   /* batch statistics (BN, feature-matching moments) are exchanged between phases   */
    MRGAN_FLAG_FLAT_GRADS = 2,   /* gradients are reduced into the flat buffers; Adam runs as its own phase        */
    MRGAN_FLAG_GRAPH      = 4,   /* stream-mode arguments only: mrgan_train_pair replays a captured hipGraph of the whole
                                  * pair.  No effect with MRGAN_FLAG_FLAT_GRADS: the phases always launch eagerly          */
    MRGAN_FLAG_GRAD_BF16  = 8,   /* with MRGAN_FLAG_FLAT_GRADS: the gradients travel as bfloat16.  The reduce phase writes
                                  * MRGAN_REGION_GRAD_*_BF16 (rounded once from the fp32 sums) instead of the fp32 flat
                                  * buffers and the Adam phase reads them back: the host all-reduces those regions in place,
                                  * nothing is cast or allocated per step.  The four fp32 scalars behind the fp32 buffers
                                  * (MRGAN_REGION_TAIL_*) still travel in fp32, and mrgan_region refuses
                                  * MRGAN_REGION_GRAD_D / _G, whose fp32 bodies no phase reads.  A labelled, different
                                  * numerical path.                                                                       */
    MRGAN_FLAG_GAUSS_NOISE = 16, /* the five GaussianNoise sites and the device-drawn z are true N(0, 1) variates (Box-Muller
                                  * on the same counter keys, support +-5.77 sigma) instead of the default Irwin-Hall(32)
                                  * sums: what the reference's K.random_normal draws, for comparisons against it.  A
                                  * DIFFERENT random stream (results are not comparable draw by draw with a default handle)
                                  * and a slower epilogue in every noisy forward product and in the staging kernel.  Every
                                  * entry honours it: mrgan_disc_step / mrgan_gen_step and their phases, mrgan_train_pair
                                  * with and without graph replay, data-parallel shards (rows stay global: the shards of a
                                  * batch draw what the full batch would), mrgan_sup_step, the _group entries.  Host-supplied z is untouched.  */
    MRGAN_FLAG_AUTOENCODER = 32  /* a handle of another kind: MRGAN_NET_D is a dense autoencoder (mrgan_ae_step and the text
                                  * above it); it trains through mrgan_ae_step and is read through mrgan_ae_encode /
                                  * mrgan_ae_reconstruct only                                                             */
};

#define MRGAN_MAX_CLASSES 32   /* largest mrgan_config.num_classes */
#define MRGAN_MAX_MODELS 16    /* largest mrgan_config.models */

/* Hyper-parameters are literals inside mr_gan() in the reference (mr_gan.py:77-79, :111-128, :165);
 * mrgan_default_config() fills exactly those values. */
typedef struct mrgan_config {
    int32_t d_in;             /* D = X_train.shape[1]                                  (mr_gan.py:114, :117)  */
    int32_t batch;            /* rows per sub-batch on THIS rank; reference batchSize = 50      (mr_gan.py:78) */
    int32_t noise_size;       /* 100                                                            (mr_gan.py:77) */
    int32_t g_hidden[2];      /* 500, 500                                                  (mr_gan.py:111-113) */
    int32_t d_hidden[5];      /* 1000, 500, 250, 250, 250                                  (mr_gan.py:119-127) */
    int32_t num_classes;      /* 6 materials; the fake class is the implicit zero logit        (mr_gan.py:128).
                               * 2 .. MRGAN_MAX_CLASSES for MRGAN_F32 / MRGAN_BF16 (the last dense is stored at a class pitch of
                               * 8 up to 8 classes and of 32 above, padding columns exact zeros); 2 .. 8 for MRGAN_FP8          */
    int32_t dtype;            /* MRGAN_F32 | MRGAN_BF16 | MRGAN_FP8 */
    float sigma[5];           /* GaussianNoise std before discriminator dense 1..5: .3 .5 .5 .5 .5 (:118-126)  */
    float lr, beta1, beta2, adam_eps;      /* Adam(lr=0.0006, beta_1=0.5), Keras defaults         (mr_gan.py:165) */
    float bn_eps;             /* 2e-5                                                          (mr_gan.py:112) */
    float unlabeled_weight;   /* 1                                                              (mr_gan.py:79) */
    uint64_t seed;            /* key of the device Philox streams (layer noise, z) */
    int32_t rank, world;      /* data-parallel position: global batch = batch*world, noise rows offset by rank*batch */
    int32_t flags;
    int32_t models;           /* 0 or 1: one model (the handle every other entry describes).  2 .. MRGAN_MAX_MODELS: a GROUP handle,
                               * `models` independent trainings of this shape that step together in one launch set
                               * (the _group entries).  Model m draws what a single handle with seed + m draws.             */
} mrgan_config;

int mrgan_default_config(mrgan_config* cfg, int32_t d_in, int32_t batch);

/* Workspace: all device memory of a handle is one block.  Pass workspace_dev = NULL to let the library
 * hipMalloc it, or allocate `bytes` yourself (e.g. a torch uint8 tensor) to be able to alias sub-regions. */
int mrgan_workspace_bytes(const mrgan_config* cfg, size_t* bytes);
int mrgan_create(const mrgan_config* cfg, void* workspace_dev, size_t bytes, mrgan_stream stream, mrgan_handle** out);
int mrgan_destroy(mrgan_handle* h);
const char* mrgan_last_error(void);

/* Group handles (mrgan_config.models > 1): G trainings of equal shape with different weights whose steps -- the supervised
 * step and the GAN sub-steps -- run as ONE launch set each (one launch per kernel kind, whatever G is).  The workspace holds the single-model layout once per model
 * (mrgan_workspace_bytes = models x the single size rounded up to 256 B); the iteration counter and the batch counter are
 * shared, all models step together.  mrgan_create refuses models > 1 together with MRGAN_FP8, MRGAN_FLAG_FLAT_GRADS,
 * MRGAN_FLAG_SYNC_STATS or world != 1.  A group handle trains through the _group entries only (mrgan_sup_step_group,
 * mrgan_disc_step_group, mrgan_gen_step_group, mrgan_train_pair_group): mrgan_disc_step, mrgan_gen_step, mrgan_train_pair,
 * mrgan_fp8_calibration and mrgan_sup_step fail with status -3.  mrgan_select_model chooses the model (default 0) that mrgan_set_weights / mrgan_get_weights, mrgan_get_slot /
 * mrgan_set_slot, mrgan_eval_error and mrgan_predict_logits address; evaluation runs model by model with the single-model
 * kernels.  mrgan_tensor_shape, mrgan_num_tensors and mrgan_get_iterations are the same for every model. */
int mrgan_select_model(mrgan_handle* h, int model);

/* Weights in Keras order.  G: W1 b1 gamma beta W2 b2 W3 b3 (generator.trainable_weights, mr_gan.py:131);
 * D: (W,b) x 6 (discriminator.trainable_weights, mr_gan.py:132).  Dense fp32 [rows, cols] row-major. */
int mrgan_num_tensors(const mrgan_handle* h, int net, int* n);
int mrgan_tensor_shape(const mrgan_handle* h, int net, int idx, int* rows, int* cols);
int mrgan_set_weights(mrgan_handle* h, int net, int idx, const float* src_dev, mrgan_stream stream);
int mrgan_get_weights(mrgan_handle* h, int net, int idx, float* dst_dev, mrgan_stream stream);
/* which: 0 = Adam m, 1 = Adam v, 2 = last flat gradient (only meaningful with MRGAN_FLAG_FLAT_GRADS) */
int mrgan_get_slot(mrgan_handle* h, int net, int idx, int which, float* dst_dev, mrgan_stream stream);
int mrgan_set_slot(mrgan_handle* h, int net, int idx, int which, const float* src_dev, mrgan_stream stream);
int mrgan_get_iterations(mrgan_handle* h, mrgan_stream stream, uint32_t* iterations_host);
int mrgan_set_iterations(mrgan_handle* h, uint32_t iterations, uint32_t batch_counter, mrgan_stream stream);

/* train_batch_disc (mr_gan.py:169, :207).  x_* are fp32 row-major with pitch ld_x; if idx_* is non-NULL row r
 * of the batch is x[idx[r]] (device-side gather from a resident pool, replacing the host slicing of
 * mr_gan.py:190-195, :207).  z_dev = NULL draws z on the device.  stream_mode = 1: idx/labels/z address whole-epoch
 * streams and the batch offset comes from the device batch counter (advanced by the generator step). */
typedef struct mrgan_disc_args {
    const float* x_lab_dev; const int32_t* idx_lab_dev; const int32_t* labels_dev;
    const float* x_unl_dev; const int32_t* idx_unl_dev;
    const float* z_dev;
    int64_t ld_x_lab, ld_x_unl;
    int32_t stream_mode, reserved;
} mrgan_disc_args;

/* train_batch_gen (mr_gan.py:170, :213) */
typedef struct mrgan_gen_args {
    const float* x_unl_dev; const int32_t* idx_unl_dev;
    const float* z_dev;
    int64_t ld_x_unl;
    int32_t stream_mode, reserved;
} mrgan_gen_args;

/* Phases exist for data-parallel drivers: a statistic or gradient exchange (RCCL all-reduce issued by the
 * host on the regions below) sits between consecutive phases.  Single-GPU callers pass (0, -1) = everything. */
enum { MRGAN_D_GEN = 0, MRGAN_D_MAIN = 1, MRGAN_D_ADAM = 2, MRGAN_D_NPHASES = 3 };
enum { MRGAN_G_GEN = 0, MRGAN_G_FEAT = 1, MRGAN_G_BWD = 2, MRGAN_G_TAIL = 3, MRGAN_G_ADAM = 4, MRGAN_G_NPHASES = 5 };
/* out3_host (optional): loss_lab, loss_unl, train_err -- the outputs of train_batch_disc */
int mrgan_disc_step(mrgan_handle* h, const mrgan_disc_args* a, int phase_first, int phase_last,
                    float* out3_host, mrgan_stream stream);
/* out1_host (optional): loss_gen */
int mrgan_gen_step(mrgan_handle* h, const mrgan_gen_args* a, int phase_first, int phase_last,
                   float* out1_host, mrgan_stream stream);
/* fp8 mode, phase-wise callers only (data-parallel hosts; whole-sub-step callers need none of this: mrgan_disc_step /
 * mrgan_gen_step / mrgan_train_pair settle the scales themselves).  The delayed scales of a sub-step kind (0 = D, 1 = G) are
 * settled by running its forward + backward phases (D_GEN .. D_MAIN, or G_GEN .. G_BWD, with the host's exchanges in between)
 * MRGAN_FP8_DRY_PASSES times WITHOUT the update phases, between BEGIN and DONE and each followed by END_PASS.  A handle
 * with synchronised statistics refuses a phase-wise first sub-step that was not calibrated this way. */
enum { MRGAN_FP8_DRY_PASSES = 5 };
enum { MRGAN_FP8_CAL_QUERY = 0, MRGAN_FP8_CAL_BEGIN = 1, MRGAN_FP8_CAL_END_PASS = 2, MRGAN_FP8_CAL_DONE = 3 };
/* QUERY returns 1 (calibrated, or not an fp8 handle) or 0; the other actions return 0 or a negative status */
int mrgan_fp8_calibration(mrgan_handle* h, int kind, int action, mrgan_stream stream);

/* Supervised baseline on the same discriminator stack (mr_nn.py:101-118): one Keras train_on_batch of the 6-layer MLP with
 * GaussianNoise, loss = mse against the one-hot label, Adam with the handle's lr / beta_1 (Keras defaults 0.001 / 0.9: set
 * them in mrgan_config).  Uses the D network and its Adam slots only; one iteration counter step per call.  A handle should
 * run either the GAN loop or this loop.  out2_host (optional): loss, training error of the batch.
 * rows_valid (0 = batch): Keras' short last batch of an epoch -- the first rows_valid rows count (means over rows_valid),
 * the remaining rows must be readable and carry label -1. */
typedef struct mrgan_sup_args {
    const float* x_dev; const int32_t* idx_dev; const int32_t* labels_dev;
    int64_t ld_x;
    int32_t stream_mode, rows_valid;
} mrgan_sup_args;
int mrgan_sup_step(mrgan_handle* h, const mrgan_sup_args* a, float* out2_host, mrgan_stream stream);
/* mrgan_sup_step once per model of a group handle, as one launch set.  Model m reads x_dev + m * x_model_stride (row pitch
 * ld_x), idx_dev + m * idx_model_stride (when idx_dev is given) and labels_dev + m * labels_model_stride; the strides count
 * elements.  x_model_stride = 0 lets every model gather from one matrix through its own index vector.  rows_valid and
 * stream_mode are common to all models.  out2_host (optional): [models][2] = loss, training error per model.  A single-model
 * handle refuses this entry (status -3). */
typedef struct mrgan_sup_group_args {
    const float* x_dev; const int32_t* idx_dev; const int32_t* labels_dev;
    int64_t ld_x;
    int64_t x_model_stride, idx_model_stride, labels_model_stride;
    int32_t stream_mode, rows_valid;
} mrgan_sup_group_args;
int mrgan_sup_step_group(mrgan_handle* h, const mrgan_sup_group_args* a, float* out2_host, mrgan_stream stream);

/* Autoencoder pre-stage (others/mr_gan_autoencoder.py:109-140 of the reference): the dimensionality reduction of the raw
 * contact-microphone vector whose codes the unchanged GAN then trains on.  A handle created with MRGAN_FLAG_AUTOENCODER holds, as
 * MRGAN_NET_D, the six dense layers d_in -> d_hidden[0] -> ... -> d_hidden[4] -> d_in (relu after the first five, linear last;
 * the reference's three encoderNodes n0 n1 n2 are d_hidden = n0 n1 n2 n1 n0).  Tensor 10 is [d_hidden[4], d_in] and tensor 11
 * [d_in], padded like a hidden layer, the last weight with the bf16 copies of the other five.  num_classes is validated and
 * unused; the generator tensors exist and nothing reads them.  mrgan_config adds no field.
 * mrgan_create refuses such a handle with a nonzero sigma[i] (status -1: no denoising variant), and (status -3) with
 * MRGAN_FP8, models > 1, world != 1, MRGAN_FLAG_FLAT_GRADS, MRGAN_FLAG_SYNC_STATS or MRGAN_FLAG_GRAD_BF16.  On such a handle
 * every GAN, supervised, group, fp8-calibration, evaluation (mrgan_eval_error, mrgan_predict_logits), saliency and attribution
 * entry returns -3; on any other handle the three entries below do.
 *
 * mrgan_ae_step: one Keras train_on_batch(x, x) with loss = 'mse' and Adam (the handle's lr / beta_1 / beta_2 / eps; Keras'
 * defaults are 0.001 / 0.9 / 0.999 / 1e-8).  x_dev / idx_dev / ld_x / stream_mode / rows_valid mean what they mean in
 * mrgan_sup_args: gather, whole-epoch index stream with the device batch counter, Keras' short last batch; a short batch in
 * stream mode is refused.  loss = mean over rows_valid x d_in of (y - x)^2 with y the stored output of the last layer (the
 * engine's activation type) and x the caller's fp32 row, read again through the same gather; dY = 2 (y - x) / (rows_valid d_in).
 * Every reduction folds per-block partials in a fixed order: a step is bit-reproducible.  One iteration-counter step.
 * out1_host (optional): the loss.  mrgan_read_metrics: out8[0] accumulates the loss, out8[4] is the last one.
 *
 * mrgan_ae_encode: the learning-phase-0 forward through dense 3; the relu output of dense 3 (the code, d_hidden[2] wide) is
 * written as fp32 [n][ld_code], ld_code >= d_hidden[2]; further columns of the caller's rows are left untouched.
 * mrgan_ae_reconstruct: the full forward; y as fp32 [n][ld_out] (ld_out >= d_in, further columns untouched) where out_dev is
 * given, the mse over all n x d_in elements where mse_host is given (fp32 sums per chunk in a fixed order, the chunks folded in
 * order; the call synchronises then); both NULL is status -2.
 * Both run in chunks of 3 S rows (S = batch rounded up to 128) through the training activations, leave weights, Adam slots,
 * counters and metrics untouched and re-zero the padding rows they reached, so that a following step is unchanged bit for
 * bit; two calls give identical bits.  Status -2: null x / output, n < 1, a pitch smaller than the row it holds. */
typedef struct mrgan_ae_args {
    const float* x_dev; const int32_t* idx_dev;
    int64_t ld_x;
    int32_t stream_mode, rows_valid;
} mrgan_ae_args;
int mrgan_ae_step(mrgan_handle* h, const mrgan_ae_args* a, float* out1_host, mrgan_stream stream);
int mrgan_ae_encode(mrgan_handle* h, const float* x_dev, const int32_t* idx_dev, int64_t ld_x, int64_t n,
                    float* code_dev, int64_t ld_code, mrgan_stream stream);
int mrgan_ae_reconstruct(mrgan_handle* h, const float* x_dev, const int32_t* idx_dev, int64_t ld_x, int64_t n,
                         float* out_dev, int64_t ld_out, float* mse_host, mrgan_stream stream);

/* Log-mel front end of the contact-microphone modality (mr_gan.py:42-47: librosa.feature.melspectrogram(y, sr, n_mels=128)
 * followed by librosa.logamplitude(S, ref_power=np.max); n_fft 2048, hop 512, Slaney mel basis, -80 dB floor).  No handle:
 * the only state is the cached filter bank per (device, sr, n_mels), built on first use under a mutex.
 * y_dev: n_trials rows of n_samples float32 (pitch ld_y); out_dev: n_trials rows of n_mels * mrgan_logmel_frames(n_samples)
 * float32, mel-major like log_S.flatten() (pitch ld_out). */
int32_t mrgan_logmel_frames(int64_t n_samples);
int mrgan_logmel(const float* y_dev, int64_t n_trials, int64_t n_samples, int64_t ld_y, int32_t sr, int32_t n_mels,
                 float* out_dev, int64_t ld_out, mrgan_stream stream);

/* RBF-kernel C-SVC of the SVM baseline (mr_svm.py:106: SVC(kernel='rbf', C=1)) on the device.  No handle and no state: three
 * launches the host chains on one stream.  Rows are SORTED BY CLASS: class c owns rows class_start_host[c] ..
 * class_start_host[c + 1] - 1 (num_classes + 1 host values, from 0 to n), and the one-vs-one pairs are numbered (0,1), (0,2), ..,
 * (1,2), .. as libsvm and scikit-learn's decision_function_shape='ovo' number them.  2 <= num_classes <= 32, no class is empty,
 * and the two largest classes together have at most MRGAN_SVM_MAX_PAIR rows (a larger pair is an error, never another path).
 *   mrgan_svm_gram    out[a, b] = exp(-gamma * max(0, |A_a|^2 + |B_b|^2 - 2 A_a . B_b)) for the m rows of a_dev and the n rows
 *                     of b_dev (d float32 features each; row pitches ld_a, ld_b, ld_out in elements).  With a_dev == b_dev the
 *                     result is symmetric bit for bit and its diagonal is exactly 1.  Nothing outside the m x n window is written.
 *   mrgan_svm_solve   libsvm's C-SVC solver (SMO, second-order working-set selection, no shrinking) on a precomputed n x n
 *                     kernel matrix, one workgroup per pair; stops at max(-y G over I_up) - min(-y G over I_low) < tol or after
 *                     max_iter updates.  coef_dev: [num_classes - 1][n] float64, alpha_t y_t in libsvm's sv_coef /
 *                     scikit-learn's dual_coef_ row convention (a row of class c holds its coefficients against the other
 *                     classes in class order); rho_dev: [pairs] float64; iters_dev: [pairs] int32, == max_iter where a pair
 *                     did not converge.  Results are bit-identical from run to run.
 *   mrgan_svm_decide  kt_dev: m x n kernel values between test rows and the training rows.  dec = sum_t coef_t K(x, x_t) - rho
 *                     per pair (float64), vote i where dec > 0 else j, labels_dev[row] = the first class with the most votes
 *                     (int32 class index).  dec_dev (optional): [m][pairs] float64. */
#define MRGAN_SVM_MAX_PAIR 2048
int mrgan_svm_gram(const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n, int64_t d, float gamma,
                   float* out_dev, int64_t ld_out, mrgan_stream stream);
int mrgan_svm_solve(const float* k_dev, int64_t ld_k, int64_t n, int32_t num_classes, const int64_t* class_start_host, double C,
                    double tol, int32_t max_iter, double* coef_dev, double* rho_dev, int32_t* iters_dev, mrgan_stream stream);
int mrgan_svm_decide(const float* kt_dev, int64_t ld_kt, int64_t m, int64_t n, int32_t num_classes, const int64_t* class_start_host,
                     const double* coef_dev, const double* rho_dev, double* dec_dev, int32_t* labels_dev, mrgan_stream stream);

/* The other libsvm classifiers of the reference's SVM grid (others/wganlpctsemi.py:204-208: SVC and NuSVC, kernel 'rbf' or
 * 'linear') through the same three stages.  Rows, classes, pairs and limits are those of the block above.
 *   mrgan_svm_kernel_matrix  mrgan_svm_gram with a kernel kind.  MRGAN_SVM_KERNEL_RBF is mrgan_svm_gram bit for bit.
 *                     MRGAN_SVM_KERNEL_LINEAR writes out[a, b] = A_a . B_b (the same k-ordered fp32 chain; gamma is ignored).
 *                     With a_dev == b_dev the result is symmetric bit for bit; its diagonal is what the chain gives for |x|^2.
 *                     Any other kind is an error.
 *   mrgan_svm_solve_nu  libsvm's nu-SVC solver (Solver_NU: SMO inside each sign, second-order working-set selection, no
 *                     shrinking) on a precomputed n x n kernel matrix, one workgroup per pair; 0 < nu <= 1.  Stops at
 *                     max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) < tol or after max_iter updates.  coef_dev: alpha_t y_t / r in
 *                     mrgan_svm_solve's layout (0 <= alpha <= 1, each sign's alpha sum to nu l / 2 over the pair's l rows);
 *                     rho_dev: [pairs] rho / r; r_dev (optional): [pairs] r, so coef * r gives alpha y back; iters_dev as in
 *                     mrgan_svm_solve (0 where the start point is already optimal).  r <= 0 is not guarded, as in libsvm: the
 *                     coefficients are then non-finite or negated.  nu is infeasible for a pair (i, j) when
 *                     nu (n_i + n_j) / 2 > min(n_i, n_j): an error before any launch, its message names the pair.
 *                     Results are bit-identical from run to run.
 * mrgan_svm_decide serves all four classifiers unchanged: it sees kernel values, coefficients and rho only. */
enum { MRGAN_SVM_KERNEL_RBF = 0, MRGAN_SVM_KERNEL_LINEAR = 1 };
int mrgan_svm_kernel_matrix(int32_t kernel, const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n,
                            int64_t d, float gamma, float* out_dev, int64_t ld_out, mrgan_stream stream);
int mrgan_svm_solve_nu(const float* k_dev, int64_t ld_k, int64_t n, int32_t num_classes, const int64_t* class_start_host, double nu,
                       double tol, int32_t max_iter, double* coef_dev, double* rho_dev, double* r_dev, int32_t* iters_dev,
                       mrgan_stream stream);

/* The same three entries for a GROUP of 1 .. MRGAN_SVM_MAX_GROUP independent problems (the folds of a table cell) in ONE launch
 * each.  The problems are ragged -- every item has its own row counts, class sizes, pitches and buffers -- and share d, gamma,
 * num_classes, C, tol and max_iter.  items_host is a host array of `count` descriptors, read during the call only; the calls
 * allocate nothing, do not synchronise and keep no state.  Every item gets exactly the checks of its single entry, before any
 * launch; a message about an item ends in "(item i)".  Each item's outputs are bit-identical to the single entry called on
 * that item.  The items of one call must not overlap in what they write. */
#define MRGAN_SVM_MAX_GROUP 16
typedef struct {
    const float* a_dev; int64_t ld_a, m;
    const float* b_dev; int64_t ld_b, n;
    float* out_dev; int64_t ld_out;
} mrgan_svm_gram_item;
typedef struct {
    const float* k_dev; int64_t ld_k, n;
    const int64_t* class_start_host;      /* num_classes + 1 host values */
    double* coef_dev; double* rho_dev; int32_t* iters_dev;
} mrgan_svm_solve_item;
typedef struct {
    const float* kt_dev; int64_t ld_kt, m, n;
    const int64_t* class_start_host;
    const double* coef_dev; const double* rho_dev;
    double* dec_dev;                      /* optional */
    int32_t* labels_dev;
} mrgan_svm_decide_item;
int mrgan_svm_gram_group(const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma, mrgan_stream stream);
int mrgan_svm_solve_group(const mrgan_svm_solve_item* items_host, int32_t count, int32_t num_classes, double C, double tol,
                          int32_t max_iter, mrgan_stream stream);
int mrgan_svm_decide_group(const mrgan_svm_decide_item* items_host, int32_t count, int32_t num_classes, mrgan_stream stream);

/* The grouped twins of mrgan_svm_kernel_matrix and mrgan_svm_solve_nu, under the rules of the block above: handle-free, no
 * allocation, no copy, no synchronisation, descriptors read during the call only, every item's single-entry checks before any
 * launch, "(item i)" at the end of a message about an item, each item's outputs bit-identical to the single entry on that item.
 *   mrgan_svm_kernel_matrix_group  mrgan_svm_gram_group with a kernel kind.  MRGAN_SVM_KERNEL_RBF launches the very kernel of
 *                     mrgan_svm_gram_group; MRGAN_SVM_KERNEL_LINEAR ignores gamma; any other kind is an error.
 *   mrgan_svm_solve_nu_group  mrgan_svm_solve_nu per item.  nu belongs to the ITEM (tol and max_iter to the group), so one call
 *                     can solve one kernel matrix at several nu: items may share k_dev, which they only read, while coef_dev,
 *                     rho_dev, r_dev and iters_dev must not overlap.  r_dev is optional per item.  An infeasible nu names the
 *                     pair of classes as the single entry does, then the item.
 * mrgan_svm_decide_group serves all four kinds unchanged: it sees kernel values, coefficients and rho only. */
typedef struct {
    const float* k_dev; int64_t ld_k, n;
    const int64_t* class_start_host;      /* num_classes + 1 host values */
    double nu;                            /* this item's nu, 0 < nu <= 1 */
    double* coef_dev; double* rho_dev;
    double* r_dev;                        /* optional */
    int32_t* iters_dev;
} mrgan_svm_solve_nu_item;
int mrgan_svm_kernel_matrix_group(int32_t kernel, const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma,
                                  mrgan_stream stream);
int mrgan_svm_solve_nu_group(const mrgan_svm_solve_nu_item* items_host, int32_t count, int32_t num_classes, double tol,
                             int32_t max_iter, mrgan_stream stream);

/* PCA pre-stage (others/wganlpctsemi.py:129-139, pcaScale: decomposition.PCA(n_components)) on the device.  No handle and no
 * state; everything runs on the caller's stream; row pitches in elements; float32 rows unless stated.  Every entry's results
 * are bit-identical from run to run (no float atomics).
 *   mrgan_pca_mean        mean_dev[d]: the column means of the n rows of x_dev, summed in float64 in a fixed order and rounded
 *                         once.
 *   mrgan_pca_covariance  cov_dev[d x d] = (X - mean)^T (X - mean) / (n - 1), n >= 2, d <= MRGAN_PCA_MAX_FEATURES: the k-ordered
 *                         fp32 matrix-core chain of mrgan_svm_kernel_matrix over the ROWS, the mean subtracted from the operands.
 *                         The row range is split into slabs that are summed in a fixed order; cov[i, j] and cov[j, i] are written
 *                         from one value.  work_dev: mrgan_pca_covariance_workspace_bytes(n, d) bytes (-1: n or d out of range).
 *                         Nothing outside the d x d window is written.
 *   mrgan_pca_eig         the k leading eigenpairs of the symmetric cov_dev by block (subspace) iteration, 1 <= k <=
 *                         MRGAN_PCA_MAX_COMPONENTS, with a block of p = min(d, k + MRGAN_PCA_GUARD) rows started from q0_dev [p x d]
 *                         (any full-rank rows).  One iteration: Y = Q C (mrgan_svm_kernel_matrix's linear kernel), the Rayleigh
 *                         quotients theta_j = q_j . y_j and residuals |y_j - theta_j q_j|_2 in float64, then Q <- the orthonormal
 *                         rows Lambda^-1/2 V^T Y from the eigen-decomposition Y Y^T = V Lambda V^T (cyclic Jacobi in one
 *                         workgroup), sorted by descending Lambda; directions with Lambda_j <= 2^-40 Lambda_1 become zero rows.
 *                         It stops when max_{j<k} residual_j <= tol * max_{j<k} theta_j, or after max_iter products (the outputs
 *                         are written either way; the caller compares).  The call SYNCHRONISES the stream once per iteration to
 *                         read 2 p + 1 doubles; nothing waits on the device.  components_dev [k x d]: rows by descending theta,
 *                         each with its largest-magnitude entry positive (first index on ties); values_host, residuals_host [k]
 *                         float64 and iters_host (products taken) are HOST memory.  work_dev: mrgan_pca_eig_workspace_bytes(d, k)
 *                         bytes, 8-byte aligned.  Status MRGAN_PCA_RANK_DEFICIENT: fewer than k directions survived
 *                         ("numerical rank below n_components").
 *   mrgan_pca_transform   out_dev[m x k] = (X - mean) W^T for the k rows of components_dev; a row's values depend on that row
 *                         alone, so working the rows in chunks changes no bit.
 *   mrgan_pca_inverse_transform  out_dev[m x d] = Z W + mean. */
#define MRGAN_PCA_MAX_COMPONENTS 64
#define MRGAN_PCA_GUARD 16
#define MRGAN_PCA_MAX_FEATURES 4096
#define MRGAN_PCA_RANK_DEFICIENT (-4)
int mrgan_pca_mean(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, float* mean_dev, mrgan_stream stream);
int64_t mrgan_pca_covariance_workspace_bytes(int64_t n, int64_t d);
int mrgan_pca_covariance(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, const float* mean_dev, float* cov_dev, int64_t ld_cov,
                         void* work_dev, int64_t work_bytes, mrgan_stream stream);
int64_t mrgan_pca_eig_workspace_bytes(int64_t d, int64_t k);
int mrgan_pca_eig(const float* cov_dev, int64_t ld_cov, int64_t d, int64_t k, const float* q0_dev, int64_t ld_q0, int64_t p, double tol,
                  int32_t max_iter, void* work_dev, int64_t work_bytes, float* components_dev, int64_t ld_w, double* values_host,
                  double* residuals_host, int32_t* iters_host, mrgan_stream stream);
int mrgan_pca_transform(const float* x_dev, int64_t ld_x, int64_t m, int64_t d, const float* mean_dev, const float* components_dev,
                        int64_t ld_w, int64_t k, float* out_dev, int64_t ld_out, mrgan_stream stream);
int mrgan_pca_inverse_transform(const float* z_dev, int64_t ld_z, int64_t m, int64_t k, const float* components_dev, int64_t ld_w,
                                int64_t d, const float* mean_dev, float* out_dev, int64_t ld_out, mrgan_stream stream);

/* one iteration of the hot loop (mr_gan.py:204-213): D step then G step */
int mrgan_train_pair(mrgan_handle* h, const mrgan_disc_args* d, const mrgan_gen_args* g, mrgan_stream stream);
/* For hosts that drive the phases themselves (data parallel) and know that the next mrgan_disc_step is followed by a
 * mrgan_gen_step whose z is drawn on the device: on != 0 lets that D sub-step also run the G sub-step's generator
 * forward as a second segment of the same launches (what mrgan_train_pair does by itself).  With
 * MRGAN_FLAG_SYNC_STATS the BN_STATS region then holds both segments and ONE all-reduce after D_GEN serves both
 * sub-steps: the host skips the exchange after that G sub-step's G_GEN.  One D sub-step per hint. */
int mrgan_pair_hint(mrgan_handle* h, int on);

/* The GAN hot loop of a group handle: mrgan_disc_step / mrgan_gen_step / mrgan_train_pair once per model, each sub-step as ONE
 * launch set with the kernel names and launch counts of a single handle's (no host loop over models).  Model m is bit-identical
 * to a single handle created with seed + m that holds model m's weights.  The fields are those of mrgan_disc_args /
 * mrgan_gen_args plus element strides between models: model m reads x_* + m * x_*_model_stride (row pitch ld_x_*), idx_* +
 * m * idx_*_model_stride (when the index vector is given), labels + m * labels_model_stride and z + m * z_model_stride.  An
 * x_*_model_stride of 0 lets every model gather from one matrix through its own index vector; z_dev = NULL: model m draws z on
 * the device with seed + m.  stream_mode is common to all models.  Whole sub-steps only (no phase range: groups stay on one
 * GPU).  out3_host (optional): [models][3] = loss_lab, loss_unl, train_err per model; out1_host (optional): [models] loss_gen.
 * step_out / accum are per model (mrgan_read_metrics addresses the selected model).  A group handle's D sub-step runs the
 * chain head at the 8-class pitch and the scalar head kernel wherever a single handle would take the matrix-core head
 * (feature layers wider than 256, the 32-class pitch): there the single handle to compare with has MRGAN_TUNE_HEAD_MFMA = 0.
 * mrgan_train_pair_group replays a captured graph under the conditions of mrgan_train_pair; its two generator forwards run
 * separately (bit-identical to the paired pass).  A single-model handle refuses these entries (status -3). */
typedef struct mrgan_disc_group_args {
    const float* x_lab_dev; const int32_t* idx_lab_dev; const int32_t* labels_dev;
    const float* x_unl_dev; const int32_t* idx_unl_dev;
    const float* z_dev;
    int64_t ld_x_lab, ld_x_unl;
    int64_t x_lab_model_stride, idx_lab_model_stride, labels_model_stride;
    int64_t x_unl_model_stride, idx_unl_model_stride, z_model_stride;
    int32_t stream_mode, reserved;
} mrgan_disc_group_args;
typedef struct mrgan_gen_group_args {
    const float* x_unl_dev; const int32_t* idx_unl_dev;
    const float* z_dev;
    int64_t ld_x_unl;
    int64_t x_unl_model_stride, idx_unl_model_stride, z_model_stride;
    int32_t stream_mode, reserved;
} mrgan_gen_group_args;
int mrgan_disc_step_group(mrgan_handle* h, const mrgan_disc_group_args* a, float* out3_host, mrgan_stream stream);
int mrgan_gen_step_group(mrgan_handle* h, const mrgan_gen_group_args* a, float* out1_host, mrgan_stream stream);
int mrgan_train_pair_group(mrgan_handle* h, const mrgan_disc_group_args* d, const mrgan_gen_group_args* g, mrgan_stream stream);

/* Launch-structure knobs of one handle (results stay within rounding; defaults are the measured best).  Call between
 * steps, never inside a captured pair.  Knobs 2 and 3 are retired: mrgan_set_tuning refuses them, and their numbers are
 * not reused. */
enum {
    MRGAN_TUNE_CHAIN = 0,        /* 1 (default where the layer widths allow): the 256-wide tail D3..D5 + loss head of the
                                  * discriminator runs as row-block chain launches; 0: one launch per layer            */
    MRGAN_TUNE_KC_CFG = 1,       /* forward / input-gradient tile: -1 (default) measured table; 0 64x128 / 3 stages,
                                  * 1 128x128 / 4 waves, 3 256x256, 5 64x128 / 2 stages, 7 128x128 / 8 waves, 9 64x64; any
                                  * other value is an error.  Shapes a tile cannot serve fall back to 0 or 1; the fp8
                                  * products read 1 and 3 only (128x128 / 256x256)                                         */
    MRGAN_TUNE_KS_GROUP = 4,     /* 0: one launch per weight gradient instead of one grouped launch (default 1)        */
    MRGAN_TUNE_PAIR_GEN = 5,     /* 0: mrgan_train_pair runs the two generator forwards separately (default 1: as one) */
    MRGAN_TUNE_HEAD_MFMA = 6     /* feature layers wider than 256 columns (bf16 / fp8): 1 (default) the loss head of the D
                                  * sub-step runs on the matrix cores over 64-row blocks; 0: the scalar head kernel       */
};
int mrgan_set_tuning(mrgan_handle* h, int knob, int value);

/* regions a data-parallel host all-reduces (sum) between phases; fp32 */
enum {
    MRGAN_REGION_BN_STATS = 0,   /* after *_GEN : [2 segments][2][N1p]  sum h, sum h^2 of the generator BatchNorm
                                  * input; segment 1 carries the G sub-step's batch after mrgan_pair_hint            */
    MRGAN_REGION_FM_MOMENTS = 1, /* after G_FEAT: [2][Fp]   sum_b f(fake), sum_b f(real)                         */
    MRGAN_REGION_BN_BWD = 2,     /* after G_BWD : [2][N1p]  sum dy, sum dy*xhat                                  */
    MRGAN_REGION_GRAD_D = 3,     /* after D_MAIN: flat padded gradients of the 12 D tensors + 4 scalars
                                  * (MRGAN_FLAG_GRAD_BF16: an error, exchange GRAD_D_BF16 and TAIL_D instead)          */
    MRGAN_REGION_GRAD_G = 4,     /* after G_TAIL: flat padded gradients of the 8 G tensors + 4 scalars (same rule)   */
    MRGAN_REGION_WORKSPACE = 5,
    MRGAN_REGION_GRAD_D_BF16 = 6, /* MRGAN_FLAG_GRAD_BF16: bfloat16 [n] flat padded gradients of the D tensors (same element order) */
    MRGAN_REGION_GRAD_G_BF16 = 7, /* ... of the G tensors                                                                    */
    MRGAN_REGION_TAIL_D = 8,      /* the 4 fp32 scalars at the end of MRGAN_REGION_GRAD_D (loss sums of the D sub-step)        */
    MRGAN_REGION_TAIL_G = 9
};
int mrgan_region(mrgan_handle* h, int region, void** ptr_dev, size_t* bytes);

/* test_batch (mr_gan.py:171, :221-222, :230): learning phase 0, discriminator only.
 * err_host = mean(argmax(logits) != labels) over the n rows. */
int mrgan_eval_error(mrgan_handle* h, const float* x_dev, const int32_t* idx_dev, int64_t ld_x,
                     const int32_t* labels_dev, int64_t n, float* err_host, mrgan_stream stream);
/* logits_dev: fp32 [n, num_classes] */
int mrgan_predict_logits(mrgan_handle* h, const float* x_dev, const int32_t* idx_dev, int64_t ld_x, int64_t n,
                         float* logits_dev, mrgan_stream stream);

/* Input-gradient saliency of a trained discriminator (the reference's others/mr_nn_activation_map.py): per row, the gradient
 * of an objective of the noise-free forward (learning phase 0) with respect to the input row, from the engine's own forward and
 * dX products.  Objectives, with t the row's target class (targets_dev[i], or the predicted class -- argmax of the logits,
 * ties to the first class -- when targets_dev is NULL):
 *   MRGAN_SAL_LOGIT  the class score l_t
 *   MRGAN_SAL_XENT   -log softmax(l)_t, the labelled loss term of mr_gan.py:146 for one row
 *   MRGAN_SAL_MSE    mean_c (l_c - onehot(t)_c)^2, the loss of the linear-output baseline (mr_nn.py:112) for one row
 * post MRGAN_SAL_RAW writes the gradient; MRGAN_SAL_HEATMAP the reference's map: g / (rms(g) + 1e-5), absolute value, min-max
 * scaled to [0, 1] over the d_in columns of the row.  A row whose map is constant (an all-dead row has a zero gradient) is
 * written as zeros; the reference would print NaN there.  out_dev: fp32 [n][ld_out], columns >= d_in are left untouched.
 * classes_out_dev (optional) receives the t each row used.  A target outside [0, num_classes) is a caller error: the gradient
 * of that row is then the objective's without the onehot term (it is not checked).
 * x_dev / idx_dev / ld_x: as mrgan_predict_logits.  The call uses the training activations as scratch, S = batch rounded up
 * to 128 rows at a time, and leaves the weights, the Adam slots, the iteration and batch counters, the metrics and a captured
 * mrgan_train_pair graph untouched; two calls give identical bits.  A group handle serves the model of mrgan_select_model.
 * Status -2: null x / out, n < 0, a pitch smaller than d_in, unknown objective or post.  Status -3: an fp8 handle (use an fp32
 * or bf16 engine with the same weights). */
enum { MRGAN_SAL_LOGIT = 0, MRGAN_SAL_XENT = 1, MRGAN_SAL_MSE = 2 };
enum { MRGAN_SAL_RAW = 0, MRGAN_SAL_HEATMAP = 1 };
typedef struct mrgan_saliency_args {
    const float* x_dev; const int32_t* idx_dev; int64_t ld_x; int64_t n;
    const int32_t* targets_dev;      /* [n] or NULL: the predicted class */
    int32_t objective;               /* MRGAN_SAL_LOGIT | MRGAN_SAL_XENT | MRGAN_SAL_MSE */
    int32_t post;                    /* MRGAN_SAL_RAW | MRGAN_SAL_HEATMAP */
    float* out_dev; int64_t ld_out;  /* [n][ld_out], ld_out >= d_in */
    int32_t* classes_out_dev;        /* optional [n]: the target class used */
} mrgan_saliency_args;
int mrgan_input_gradient(mrgan_handle* h, const mrgan_saliency_args* a, mrgan_stream stream);

/* Attribution maps averaged over `draws` forwards, accumulated on the device: the mean over d = 0 .. draws - 1 of the input
 * gradient g_d of mrgan_input_gradient's objective, taken at a forward that differs per draw.  x_dev .. classes_out_dev mean what
 * they mean in mrgan_saliency_args.
 *   method MRGAN_ATTR_NOISE (SmoothGrad): draw d is the learning-phase-1 forward at x with fresh GaussianNoise.  Site 0 is the
 *     staged input, sites 1 .. 4 the outputs of dense 1 .. 4; draw d of site s adds sigma * N(0, 1) with sigma = sigma_input at
 *     site 0 and sigma_hidden at sites 1 .. 4.  A sigma of exactly 0 leaves that site noise-free (the kernels the evaluation
 *     runs); mrgan_config.sigma[0] and sigma[1] (0.3 and 0.5) give the training forward; (s, 0) is the classic input-only
 *     SmoothGrad.  The gradient is taken with respect to the noisy input, which is the gradient with respect to x.
 *   method MRGAN_ATTR_PATH: draw d is the noise-free forward at the point
 *         v = fmaf(alpha_d, x - b, b),   alpha_d = (d + 0.5f) / (float)draws      (all fp32; the midpoint rule on [0, 1])
 *     of the straight path from the baseline b (baseline_dev: fp32 [d_in], or NULL for zeros -- the training mean of
 *     standard-scaled data) to the row x.
 *   multiply = 1 multiplies the mean gradient elementwise by (x - b), x the caller's fp32 row and b the baseline (zeros when
 *     NULL): gradient x input for MRGAN_ATTR_NOISE, integrated gradients for MRGAN_ATTR_PATH (they sum to l_t(x) - l_t(b) under
 *     MRGAN_SAL_LOGIT as draws grows).  multiply = 0 leaves the mean gradient.
 * The sum over draws is fp32, in draw order, without atomics; the last draw divides by draws, applies multiply and then post
 * (MRGAN_SAL_HEATMAP: the map of mrgan_input_gradient, constant-row rule included, of that final quantity).  draws = 1, both
 * sigmas 0, MRGAN_ATTR_NOISE, multiply = 0 gives the bits of mrgan_input_gradient.
 * Noise keys: site s, draw d of the call draws its normals at (seed + selected model, s * 256 + MRGAN_ATTR_NOISE_SEG, step d,
 * row = the row's index in the call), from the generator of the handle (MRGAN_FLAG_GAUSS_NOISE: the true-Gaussian one).  Segment
 * id MRGAN_ATTR_NOISE_SEG is used by no training or evaluation draw, and the step is the draw index, not the handle's iteration:
 * a map is a function of (weights, seed, rows, arguments) alone -- training further or mrgan_set_iterations do not move it, nor
 * does the chunking of the call.
 * Target class: targets_dev[i], or with targets_dev NULL the predicted class of the noise-free forward at x (what
 * mrgan_input_gradient reports), computed once per chunk of S rows by one extra clean forward, written to classes_out_dev and
 * used for every draw; classes_out_dev is required in that case.
 * Leaves untouched what mrgan_input_gradient leaves untouched; two calls give identical bits; a group handle serves the model
 * of mrgan_select_model.
 * Status -2: what mrgan_input_gradient refuses; an unknown method; draws outside [1, MRGAN_ATTR_MAX_DRAWS]; multiply not 0 or 1;
 * a negative or non-finite sigma; a nonzero sigma with MRGAN_ATTR_PATH or a baseline with MRGAN_ATTR_NOISE; targets_dev and
 * classes_out_dev both NULL.  Status -3: an fp8 handle. */
enum { MRGAN_ATTR_NOISE = 0, MRGAN_ATTR_PATH = 1 };
enum { MRGAN_ATTR_MAX_DRAWS = 4096, MRGAN_ATTR_NOISE_SEG = 255 };
typedef struct mrgan_attribution_args {
    const float* x_dev; const int32_t* idx_dev; int64_t ld_x; int64_t n;
    const int32_t* targets_dev;      /* [n] or NULL: the predicted class of the noise-free forward at x */
    int32_t objective;               /* MRGAN_SAL_LOGIT | MRGAN_SAL_XENT | MRGAN_SAL_MSE */
    int32_t post;                    /* MRGAN_SAL_RAW | MRGAN_SAL_HEATMAP */
    float* out_dev; int64_t ld_out;  /* [n][ld_out], ld_out >= d_in */
    int32_t* classes_out_dev;        /* [n]: the target class used; optional when targets_dev is given */
    int32_t method;                  /* MRGAN_ATTR_NOISE | MRGAN_ATTR_PATH */
    int32_t draws;                   /* 1 .. MRGAN_ATTR_MAX_DRAWS */
    float sigma_input, sigma_hidden; /* MRGAN_ATTR_NOISE: sigma of site 0 / of sites 1 .. 4; 0 with MRGAN_ATTR_PATH */
    const float* baseline_dev;       /* MRGAN_ATTR_PATH: [d_in] or NULL (zeros); NULL with MRGAN_ATTR_NOISE */
    int32_t multiply;                /* 1: times (x - baseline) */
    int32_t reserved;
} mrgan_attribution_args;
int mrgan_attribution(mrgan_handle* h, const mrgan_attribution_args* a, mrgan_stream stream);

/* epoch metrics accumulated on the device (mr_gan.py:208-210 accumulate on the host and force a sync per step):
 * out8_host = sum loss_lab, sum loss_unl, sum train_err, sum loss_gen, last loss_lab, last loss_unl, last err,
 * last loss_gen.  reset != 0 zeroes the sums afterwards. */
int mrgan_read_metrics(mrgan_handle* h, float* out8_host, int reset, mrgan_stream stream);

/* Per-kernel timing with hipEvents on the launch stream (bench.py's live roofline figure): while profiling is on,
 * every kernel of the step is launched with a (start, stop) event pair stamped at its own begin and end on the device
 * (hipExtLaunchKernelGGL), i.e. the interval rocprofv3's kernel trace reports; mrgan_train_pair launches eagerly
 * (no graph replay) behind a short delay kernel per sub-step so that the kernels still run back to back.
 * mrgan_profile_end returns, per distinct kernel instantiation (named as rocprofv3 prints it, MRGAN_PROF_NAME_LEN
 * bytes each): summed time, launch count, summed ALGORITHMIC flops (2 x logical M*N*K of the dense layer) and summed
 * ALGORITHMIC bytes (operands read once + outputs written once; 0 where the library does not account them). */
enum { MRGAN_PROF_NAME_LEN = 96 };
int mrgan_profile_begin(mrgan_handle* h);
int mrgan_profile_end(mrgan_handle* h, mrgan_stream stream, int max_kernels, char* names, float* ms, int32_t* launches,
                      double* flops, double* bytes, int* n_kernels);

#ifdef __cplusplus
}
#endif
#endif
