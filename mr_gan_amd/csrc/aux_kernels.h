// Argument blocks + launchers for the non-GEMM kernels of the mr_gan training path.
#pragma once
#include "common.h"

namespace mrgan {

constexpr int KMAX = 8;            // class pitch KP of a handle with <= 8 classes (reference: 6 materials, mr_gan.py:80)
constexpr int KWIDE = 32;          // class pitch of a handle with 9 .. 32 classes; columns >= classes of W6 / b6 / logits are zeros
constexpr int class_pitch(int classes) { return classes <= KMAX ? KMAX : KWIDE; }
constexpr int HEAD_ROWS = 32;      // rows per loss-head block
constexpr int HEAD_CHUNK = 256;    // feature columns of the loss head held in LDS at a time (wider layers are walked in chunks)

// ---- staging: rows of the (scaled) data matrix -> noisy discriminator input; z -> generator input ----
struct StageSeg {
    const float* src; const int32_t* idx; long ld;   // row r comes from src[(idx ? idx[o+r] : o+r) * ld + c]
    int rows, cols, cols_pad;
    void* out; int ldo;                             // T [rows][ldo]; columns >= cols are zero-filled
    float sigma; uint32_t site, seg;
    int gen;                                        // 1: out = N(0,1) only (z drawn on device), src ignored
    int stream;                                     // 1: o = batch * rows from the device batch counter
    uint32_t iter_off;                              // noise key uses DevState::iter + iter_off (z of a later sub-step)
    // Model groups: the segment once per model (0 or 1: one model; the same count in every segment of a launch).  Model m reads
    // src + m * src_ms and idx + m * idx_ms (elements; src_ms = 0: every model gathers from one matrix), writes out + m * out_ms
    // (bytes) and draws its noise with seed + m.
    int models; long src_ms, idx_ms, out_ms;
};
struct StageArgs {
    StageSeg s[5]; int nseg;
    uint64_t seed; uint32_t row0;
    const DevState* cur;
    int gauss;                                      // 0 = Irwin-Hall noise / z, 1 = true Gaussian (MRGAN_FLAG_GAUSS_NOISE)
    // set by launch_stage: grid.y = model * ry + row block, model = (blockIdx.y * ry_mul) >> 16 (ry_mul = 0: one model)
    int ry; uint32_t ry_mul;
};
int launch_stage(int bf16, const StageArgs& a, hipStream_t s);

// ---- BatchNorm (batch statistics, biased variance; mr_gan.py:112) ----
struct BnApplyArgs {
    const void* h; void* out; int ld; int rows; int cols;      // cols = logical width
    const float* cs1; const float* cs2; int npart; int ldcs;   // column partial sums of h and h^2
    float count, eps;                                          // global batch size
    const float* gamma; const float* beta;
    float* mu; float* rstd;                                    // saved for the backward pass
    long cs_seg_stride;                                        // floats between the partial sums of consecutive segments
    int nseg; long seg_rows;                                   // nseg independent batches, seg_rows rows apart in h / out; their
                                                               // partial sums follow each other (npart rows each), mu / rstd ld apart
    // Model groups: grid.z = model * nseg + segment (0 or 1: one model), model = (blockIdx.z * seg_mul) >> 16 (set by
    // launch_bn_apply).  Model m's h, out, cs1 / cs2, gamma, beta, mu and rstd lie model_stride BYTES behind model 0's.
    int models; long model_stride; uint32_t seg_mul;
};
int launch_bn_apply(int bf16, const BnApplyArgs& a, hipStream_t s);

struct BnBwdArgs {
    const void* dy; const void* h; void* dpre; int ld; int rows; int cols;
    const float* cs1; const float* cs2; int npart; int ldcs;   // sum(dy), sum(dy*xhat) partials
    float count;
    const float* gamma; const float* mu; const float* rstd;
    float* db_part;                                            // [stat_row_blocks(rows)][ld] column sums of dpre
    // Model groups: grid.z = models (0 or 1: one model).  Model m's dy, h, dpre, cs1 / cs2, gamma, mu, rstd and db_part lie
    // model_stride BYTES behind model 0's.
    int models; long model_stride;
};
int launch_bn_bwd(int bf16, const BnBwdArgs& a, hipStream_t s);
int stat_row_blocks(int rows);                                 // row blocks of the column-statistic kernels

// ---- loss head (mr_gan.py:128, :146-149, :161-162): last dense + losses + their gradients ----
enum { HEAD_LAB = 0, HEAD_UNL = 1, HEAD_FAKE = 2, HEAD_EVAL = 3, HEAD_LOGITS = 4,
       HEAD_MSE = 5,     // supervised baseline (mr_nn.py:112): mean squared error against the one-hot label
       // Saliency row kinds (head_kernel only; every segment of a launch, or none): dpre = the PER-ROW gradient of the class
       // score / the cross-entropy / the squared error of the target class (head.h: head_row), no 1 / batch.  labels = the
       // targets, or null: the row's argmax.  Such a launch writes dpre and classes_out (and logits where given), nothing else:
       // no loss_part, no part, no err_count.
       HEAD_SAL_LOGIT = 6, HEAD_SAL_XENT = 7, HEAD_SAL_MSE = 8 };
struct HeadArgs {
    const void* f; long f_bs; int ldf;         // features [seg][rows][ldf]
    int rows, nseg, seg_kind[3];
    int feat, feat_valid, classes;             // padded / logical feature width, number of classes
    const float* w; int ldw; const float* b;   // last dense: w[feat][ldw], b[classes]; ldw = the class pitch KP (8 or 32)
    const int32_t* labels;                     // [rows] (stream mode: offset by batch*rows)
    const DevState* st; int labels_stream;
    float inv_count, unl_weight;               // 1/(global batch), mr_gan.py:79
    float* logits; long logits_bs;             // optional [seg][rows][KP]
    void* dpre; long dpre_bs; int ldd;         // dL/d(pre-activation of the feature layer), T
    float* part; long part_stride;             // per-block partial gradients: part[blk][0 .. feat*KP) = dW6,
    int off_db, off_dbf;                       //   [off_db .. +KP) = db6, [off_dbf .. +feat) = bias grad of the feature layer
    float* loss_part;                          // [blk][4] : sum loss_lab, sum loss_unl terms, sum err, 0
    // Model groups: grid.z = models (0 or 1: one model).  Model m's f, w, b, logits, dpre, part and loss_part lie model_stride
    // BYTES behind model 0's, its labels labels_ms elements behind; st is shared.  Training heads without fp8 copies only.
    int models; long model_stride, labels_ms;
    union {                                    // (one pointer: the kinds that use them never share a launch)
        int* err_count;                        // HEAD_EVAL: integer count of argmax != label
        int32_t* classes_out;                  // HEAD_SAL_*: optional [rows], the target class each row used
    };
    // fp8 mode: dpre leaves as e5m2 copies scaled by q8_slot->scale (row-major [seg][rows][ldq8] and transposed [feat][ldq8t] with
    // segment s at row offset s * q8t_bs), max |dpre| -> q8_slot; dpre itself may then be null
    unsigned char* q8; long q8_bs; int ldq8;
    unsigned char* q8t; long q8t_bs; int ldq8t;
    Fp8Slot* q8_slot;
};
int launch_head(int bf16, const HeadArgs& a, hipStream_t s);
// dst[g][i] = sum over partial rows p = g, g+ngroups, ... of src[p][i]  (i < n, rows `stride` apart)
// (model groups: the fold once per model, src / dst of model m model_stride bytes behind model 0's)
int launch_reduce_partials(const float* src, int nsrc, long stride, int n, int ngroups, float* dst, hipStream_t s, int models = 1,
                           long model_stride = 0);
int init_kernel_attributes();

// ---- saliency map of a trained discriminator: rows of d objective / d input (the layer-0 dX) -> the caller's fp32 rows ----
// SAL_RAW: the gradient, widened.  SAL_HEATMAP (others/mr_nn_activation_map.py:170-178 of the reference): g_hat = g / (rms(g) +
// 1e-5), a = |g_hat|, out = (a - min a) / (max a - min a), mean and extrema over the row's `cols` columns.  A row with max a ==
// min a (an all-dead row: zero gradient) is written as zeros, where the reference divides 0 by 0.
enum { SAL_RAW = 0, SAL_HEATMAP = 1 };

// ---- maps over draws (mrgan_attribution; mrgan_input_gradient is one draw): a path point as the input, and the accumulator ----
// out[r][c] = T(fmaf(alpha, x[r][c] - b[c], b[c])) for c < cols, 0 for cols <= c < cols_pad; row r of x is
// src[(idx ? idx[r] : r) * ld + c], b = baseline[c] or 0.  The gather of the stage kernel without its noise.
struct PathStageArgs {
    const float* src; const int32_t* idx; long ld;
    const float* baseline;                     // [cols] or null: zeros
    float alpha;
    int rows, cols, cols_pad;
    void* out; int ldo;                        // T [rows][ldo], ldo a multiple of 8 and >= cols_pad
};
int launch_path_stage(int bf16, const PathStageArgs& a, hipStream_t s);
// Draw `draw` of `draws`: out = g (draw 0) or out += g (fp32, in draw order); the last draw then divides by draws, multiplies
// by (x - baseline) where asked (x gathered as in PathStageArgs) and stores that, or its SAL_HEATMAP map.  draws = 1 never reads
// out.  Columns >= cols of out are never touched.
struct AttrAccumArgs {
    const void* g; int ldg;                    // T [rows][ldg]: this draw's layer-0 dX
    int rows, cols;
    float* out; long ldo;
    int mode;                                  // SAL_RAW | SAL_HEATMAP, applied by the last draw
    int draw, draws;
    int multiply;
    const float* x; const int32_t* idx; long ld_x;      // multiply: the caller's rows (idx already offset to the chunk)
    const float* baseline;
};
int launch_attr_accum(int bf16, const AttrAccumArgs& a, hipStream_t s);

// ---- autoencoder (MRGAN_FLAG_AUTOENCODER): the reconstruction head and the copy-out of the read-only entries ----
// The mse head over the stored output y of the last layer against the caller's own fp32 rows x (row r of the batch is
// src[(idx ? idx[o + r] : o + r) * ld_x + c], o = batch counter * batch_rows in stream mode): for r < rows_valid, c < cols
//     dY[r][c] = T(scale * (y - x)),   loss partial += (y - x)^2
// and exact zeros in every other element of the rows x cols_pad the grid covers (rows and cols_pad multiples of 64).  One block
// = 64 rows x 64 columns: cs[row block][c] = the column sums of the STORED dY (what the weight-gradient product reads),
// loss_part[(row block * column blocks + column block) * 4] = the block's sum of squares (the three further floats zero: the
// layout the Adam launch's metrics pass folds).  Thread, wave and block sums in a fixed order, no atomics.  dy = cs = null:
// the loss partials alone (mrgan_ae_reconstruct).
struct ReconHeadArgs {
    const void* y; int ldy;                    // T [rows][ldy]
    const float* x; const int32_t* idx; long ld_x;
    const DevState* st; int stream, batch_rows;
    int rows, rows_valid, cols, cols_pad;
    float scale;                               // 2 / (rows_valid * cols)
    void* dy; int ldd;                         // T [rows][ldd] or null
    float* cs; int ldcs;                       // [rows / 64][ldcs] or null
    float* loss_part;                          // [rows / 64][cols_pad / 64][4]
};
int launch_recon_head(int bf16, const ReconHeadArgs& a, hipStream_t s);
// acc[0] = (first ? 0 : acc[0]) + the sum of part[4 i], i < n, in a fixed order (one block)
int launch_fold_loss(const float* part, int n, float* acc, int first, hipStream_t s);
// dst[r][c] = (float)src[r][c] for c < cols: rows of a padded activation T [rows][lds] -> the caller's fp32 rows [rows][ldd];
// columns >= cols of dst are never touched
int launch_cast_rows(int bf16, const void* src, int lds, int rows, int cols, float* dst, long ldd, hipStream_t s);

// ---- feature matching (mr_gan.py:152-154) ----
struct FmArgs {
    const float* cs; int npart_fake, npart_real, ldcs;   // column partial sums of f: fake rows first, then real
    float count, grad_scale; int feat, feat_valid;        // rows behind each mean; 1/world for per-shard statistics
    const uint16_t* mask; int ldm;                        // lane-native relu mask (gemm.h) of the fake rows' feature layer
    void* dpre; int ldd; int rows;
    float* loss_out; float* accum;                        // step scalar + epoch accumulator (block 0 only)
    unsigned char* q8; int ldq8; Fp8Slot* q8_slot;        // fp8 mode: e5m2 copy of dpre (row-major), scaled by the slot; dpre may be null
    int rb;                                               // rows per block (set by launch_fm)
    // wide feature layers: the loss is assembled from per-column-block partials (lscratch[gridDim.x]) by the last block to
    // arrive (*lcount: ticket, left at zero again) in a fixed order, instead of by one extra block that walks every column
    float* lscratch; unsigned int* lcount;
    // Model groups: grid.z = models (0 or 1: one model).  Model m's cs, mask, dpre, loss_out, accum, lscratch and lcount (its own
    // ticket) lie model_stride BYTES behind model 0's.  Without fp8 copies only.
    int models; long model_stride;
};
int launch_fm(int bf16, const FmArgs& a, hipStream_t s);

// ---- collapse per-row-tile partial sums to one row (data-parallel statistic exchange) ----
int launch_colsum_finalize(const float* part1, const float* part2, int npart, int ld, int n, float* out /* [nseg][2][n] */, hipStream_t s,
                           int nseg = 1 /* segments: partial rows npart * ld floats apart */);

// ---- multi-tensor Adam (Keras 2.0.9 formula, mr_gan.py:165-167) ----
struct AdamTile {
    float* p; float* m; float* v;
    const float* g; int nslab; long slab_stride;       // gradient = sum of nslab slabs
    float* flat;                                       // flat gradient buffer (tile origin)
    __bf16* flat16;                                    // MRGAN_FLAG_GRAD_BF16: bfloat16 flat gradient buffer instead (null otherwise)
    __bf16* w16; __bf16* wt16;                         // bf16 copies [K][N] and [N][K] (null for fp32 / 1-D)
    unsigned char* w8; unsigned char* w8t; Fp8Slot* w8_slot;      // fp8 mode: e4m3 copies of the bf16 values (same tile origins)
    int ld, ldt;                                       // row pitch of p/m/v/g/w16 ; of wt16
    int rows, cols;                                    // tile extent (<= 64 x 64)
};
enum { ADAM_FUSED = 0, ADAM_REDUCE_ONLY = 1, ADAM_FROM_FLAT = 2 };
struct AdamArgs {
    const AdamTile* tiles; int ntiles; int mode;
    float b1, b2, eps;
    const DevState* st;
    // metrics finish (block 0): loss partials of this sub-step -> step_out[0..2] and epoch accumulators
    const float* loss_part; int nloss_part; float inv_rows; float* step_out; float* accum;
    float* flat_tail;                                  // 4 floats after the flat gradients (travel with the all-reduce)
    // The updating launch is the last kernel of a sub-step: it publishes the next sub-step's DevState slot
    // (iterations + 1, batch counter + advance_batch, lr_t of the new iteration).  Null for ADAM_REDUCE_ONLY.
    DevState* next; int advance_batch; float lr;
    // Model groups: grid.y = models (0 or 1: one model).  Model m's tensors (every pointer of a tile), loss_part, step_out and
    // accum lie model_stride BYTES behind model 0's; st / next are shared, and model 0's block 0 alone publishes `next`.
    int models; long model_stride;
};
int launch_adam(const AdamArgs& a, hipStream_t s);

int launch_noise_debug(int gauss, uint64_t seed, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0, int rows, int cols,
                       float* out, hipStream_t s);

}  // namespace mrgan
