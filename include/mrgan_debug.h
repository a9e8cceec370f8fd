/* libmrgan_hip -- diagnostic entry points (parity tests, kernel timing experiments).  Not part of the drop-in boundary:
 * a host that replaces mr_gan.py:169-171 needs include/mrgan_abi.h only. */
#ifndef MRGAN_DEBUG_H
#define MRGAN_DEBUG_H

#include "mrgan_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[rows][cols] = the standard normals the handle's generator draws at (site, seg, step), first global row row0: the
 * Irwin-Hall variates by default, the true-Gaussian ones on a MRGAN_FLAG_GAUSS_NOISE handle (which draws whole row pairs:
 * row0 must be even there) */
int mrgan_debug_noise(mrgan_handle* h, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0, int rows, int cols,
                      float* out_dev, mrgan_stream stream);
int mrgan_debug_tr_probe(uint16_t* out1024_dev, mrgan_stream stream);
/* timing experiments only (results become wrong): 2 = skip the GEMM epilogues, 4 = skip the GEMM main loops */
int mrgan_debug_ablate(mrgan_handle* h, int bits);
int mrgan_debug_buffer(mrgan_handle* h, int kind, int l, void** ptr_dev, int* rows_per_seg, int* ld, int* elem_size);
/* average device time (us) of `reps` back-to-back launches of one bf16 product on scratch buffers:
 * op 0 forward (relu+noise+mask), 1 input-gradient (relu mask), 2 weight-gradient with `splits` slabs */
int mrgan_debug_gemm_time(int op, int m, int n, int k, int nbatch, int splits, int reps, int ablate, int kc_cfg, float* avg_us);

/* One GEMM launch described field by field, for kernel-level tests of every tile and epilogue variant.  Nothing is allocated,
 * converted or cleared except the DevState that carries `iter`: every buffer is the caller's device memory in the kernel's own
 * element type (dtype MRGAN_BF16: bf16 operands / h / out; MRGAN_F32: float), so a caller that pre-fills the buffers sees
 * every element the kernel did not write.  dtype MRGAN_FP8 (csrc/gemm_fp8.hip): `a` and `b` are the caller's fp8 bytes in the
 * product's formats (op 0: e4m3 x e4m3, 1: e5m2 x e4m3, 2: e4m3 x e5m2), strides in bytes, both operands reduction-contiguous
 * (a_sk == b_sk == 1) for all three ops; the output is bf16 (`out`) or the fp8 images q8 / q8t.
 *   op 0 (forward) / 1 (input gradient): out[b][i][j] = epilogue(sum_k A(b,i,k) B(b,k,j)), i < m, j < n, reduction length k
 *   op 2 (weight gradient): slab[split][i][j] = sum of A(i,v) B(v,j) over the reduction rows v of that split, v < k
 *   A(b,i,k) at a + b*a_bs + i*a_si + k*a_sk ; B(b,k,j) at b + b*b_bs + k*b_sk + j*b_sj  (strides in elements).
 * The remaining fields are those of the library's GEMM argument block (csrc/gemm.h), which documents them. */
typedef struct mrgan_debug_gemm_desc {
    int32_t dtype, op, m, n, k, nbatch, splits;
    int32_t kchunk;                      /* reduction elements per split; 0 = k */
    int32_t kc_cfg;                      /* bf16 forward / dX block tile, as MRGAN_TUNE_KC_CFG: -1 = the measured table */
    int32_t tune_bits;
    int32_t seg_stride, seg_rows;        /* op 2: reduction row v is valid when v % seg_stride < seg_rows; 0 = no holes */
    const void* a; int64_t a_bs, a_si, a_sk;
    const void* b; int64_t b_bs, b_sk, b_sj;
    int32_t act, n_valid;
    const float* bias;
    void* out; int64_t out_bs; int32_t ldo;
    float sigma; uint32_t site, seg0; int32_t seg_step; uint32_t iter_step, row0;
    uint32_t iter;                       /* DevState::iter of the launch */
    uint64_t seed;
    uint16_t* mask; int64_t mask_bs; int32_t ldm;
    const void* h; int64_t h_bs; int32_t ldh;
    int32_t cs_mode; float* cs1; float* cs2; int32_t ldcs;
    const float* bn_mu; const float* bn_rstd;
    float* slab; int64_t slab_stride;
    /* MRGAN_FP8 only (Epi of csrc/gemm.h): the fp8 images of the output, row-major [b][i][ldq8] and transposed [j][ldq8t] with
     * batch b at byte b * q8t_bs; device slots {amax_bits, scale, inv_scale, target} (4 x 32 bits) of operand A, operand B (both
     * null: the accumulator is taken as it is) and of the output */
    void* q8; int64_t q8_bs; int32_t ldq8;
    void* q8t; int64_t q8t_bs; int32_t ldq8t;
    const void* slot_a; const void* slot_b; void* slot_o;
    int32_t gauss;                       /* forward noise from the true-Gaussian generator (row0 even) */
} mrgan_debug_gemm_desc;
/* per-block partial rows folded by the tail blocks of a grouped weight-gradient launch:
 * dst[g][i] = sum of src[p][i] over p = g, g + ngroups, ... < nsrc  (i < n, rows `stride` floats apart) */
typedef struct mrgan_debug_fold { const float* src; float* dst; int64_t stride; int32_t nsrc, n, ngroups; } mrgan_debug_fold;
/* grouped = 0: launches d[0] (count must be 1) through the dtype's launcher.  grouped = 1: `count` bf16 weight-gradient
 * products (+ the optional fold) as one grouped launch; returns 1 when the grouped kernel does not apply (nothing launched).
 * Returns -1 for arguments the entry refuses (kc_cfg among them), the launcher's code (-3) for products it refuses.
 * kname (optional, kname_len bytes) receives the name of the kernel that ran.  Synchronises the stream. */
int mrgan_debug_gemm_launch(const mrgan_debug_gemm_desc* d, int count, int grouped, const mrgan_debug_fold* fold,
                            char* kname, int kname_len, mrgan_stream stream);

/* fp8 (OCP e4m3) forward product on the matrix cores, operands quantised from the fp32 inputs with per-tensor scales:
 * out[m,n] = act((q(a * scale_a) q(b * scale_b)) / (scale_a scale_b) + bias).  reps > 0 also times `reps` launches.
 * kc_cfg: -1 = the launcher's choice, 1 = 128x128 blocks, 3 = 256x256 blocks. */
int mrgan_debug_gemm_fp8(int m, int n, int k, const float* a_dev, const float* b_dev, const float* bias_dev, int act, float scale_a,
                         float scale_b, float* out_dev, int reps, float* avg_us, int kc_cfg, mrgan_stream stream);

/* One launch of the bf16 -> fp8 quantiser (csrc/gemm.h Quant8Args, every buffer the caller's): src [nb][rows][ld] bf16 ->
 * dst [nb][prow][ldd] and / or the transposed dstt [cols][lddt] (batch b at byte b * dstt_bs) = fp8(v * slot->scale), fmt 0 =
 * e4m3, 1 = e5m2; rows [rows, prow) are written as zeros; max |v| goes to the device slot.  Returns the launcher's -3 for
 * arguments it refuses.  Synchronises the stream. */
int mrgan_debug_quant8(const void* src, int64_t src_bs, int ld, int rows, int cols, int nb, int prow, void* dst, int64_t dst_bs, int ldd,
                       void* dstt, int64_t dstt_bs, int lddt, void* slot_dev, int fmt, mrgan_stream stream);
/* the delayed-scaling update on the caller's array of n device slots.  Synchronises the stream. */
int mrgan_debug_fp8_update_scales(void* slots_dev, int n, mrgan_stream stream);

/* ---- one launch of a non-GEMM kernel (csrc/aux_kernels.h), for kernel-level tests ----
 * One entry per launcher; every descriptor mirrors the launcher's argument block field by field (csrc/aux_kernels.h documents
 * the fields), `dtype` (MRGAN_F32 / MRGAN_BF16) is the launcher's element-type argument.  Every data buffer is the caller's
 * device memory in the kernel's own element type; nothing is converted or cleared, so a caller that pre-fills a buffer sees
 * every element the kernel did not write.  The entries allocate only the DevState a kernel reads as launch state.  They
 * synchronise the stream, return the launcher's -3 unchanged, and refuse with -1 only what the launcher takes on trust: the
 * alignment of the 16-byte accesses and pitches smaller than the logical widths (message behind mrgan_last_error). */

/* stage_kernel through launch_stage (StageArgs / StageSeg; `ry` / `ry_mul` are the launcher's).  iter / batch: the DevState of the
 * launch.  Written per segment and model: out[r][0 .. cols_pad) for r < rows, columns >= cols zeros; nothing else.  The
 * kernel itself chooses between 16-byte and scalar source loads (ld % 4, the alignment of src); the entry refuses only the
 * output side: out / out_ms not 16-byte aligned, ldo not a multiple of 8 or below cols_pad, cols_pad not a multiple of 8 or
 * below cols, ld below cols, and an odd row0 with the true-Gaussian generator (it draws whole row pairs). */
typedef struct mrgan_debug_stage_seg {
    const float* src; const int32_t* idx; int64_t ld;
    int32_t rows, cols, cols_pad;
    void* out; int32_t ldo;
    float sigma; uint32_t site, seg;
    int32_t gen, stream; uint32_t iter_off;
    int32_t models; int64_t src_ms, idx_ms, out_ms;
} mrgan_debug_stage_seg;
typedef struct mrgan_debug_stage_desc {
    int32_t dtype;
    mrgan_debug_stage_seg s[5]; int32_t nseg;
    uint64_t seed; uint32_t row0;
    uint32_t iter, batch;
    int32_t gauss;
} mrgan_debug_stage_desc;
int mrgan_debug_stage(const mrgan_debug_stage_desc* d, mrgan_stream stream);

/* dst[g][i] = sum of src[p][i] over p = g, g + ngroups, ... < nsrc (i < n, rows `stride` floats apart), once per model
 * (model m's src / dst model_stride BYTES behind model 0's).  Written: dst[g][0 .. n) for g < ngroups, nothing else. */
int mrgan_debug_reduce_partials(const float* src, int nsrc, int64_t stride, int n, int ngroups, float* dst, int models,
                                int64_t model_stride, mrgan_stream stream);
/* out[seg][0][0 .. n) = column sums of part1's npart rows of segment seg (rows ld floats apart, segments npart * ld floats
 * apart), out[seg][1][0 .. n) those of part2.  Written: exactly those 2 n floats per segment.  n % 4 != 0: -3. */
int mrgan_debug_colsum_finalize(const float* part1, const float* part2, int npart, int ld, int n, float* out, int nseg,
                                mrgan_stream stream);

/* BatchNorm forward from column partial sums (BnApplyArgs).  The kernel works on all `ld` columns: it writes out[r][0 .. ld) for
 * r < rows of every segment (columns >= cols: h * 0 + 0, zeros for finite h) and mu / rstd [seg][0 .. ld) (columns >= cols:
 * the statistics of whatever the partial sums hold there). */
typedef struct mrgan_debug_bn_apply_desc {
    int32_t dtype;
    const void* h; void* out; int32_t ld, rows, cols;
    const float* cs1; const float* cs2; int32_t npart, ldcs;
    float count, eps;
    const float* gamma; const float* beta;
    float* mu; float* rstd;
    int64_t cs_seg_stride;
    int32_t nseg; int64_t seg_rows;
} mrgan_debug_bn_apply_desc;
int mrgan_debug_bn_apply(const mrgan_debug_bn_apply_desc* d, mrgan_stream stream);

/* BatchNorm backward fused with the softplus derivative (BnBwdArgs).  Written: dpre[r][0 .. ld) for r < rows (columns >= cols
 * are zeros: gamma, mu and rstd count as 0 there) and db_part[blk][0 .. ld) for blk < ceil(rows / 64). */
typedef struct mrgan_debug_bn_bwd_desc {
    int32_t dtype;
    const void* dy; const void* h; void* dpre; int32_t ld, rows, cols;
    const float* cs1; const float* cs2; int32_t npart, ldcs;
    float count;
    const float* gamma; const float* mu; const float* rstd;
    float* db_part;
} mrgan_debug_bn_bwd_desc;
int mrgan_debug_bn_bwd(const mrgan_debug_bn_bwd_desc* d, mrgan_stream stream);

/* head_kernel through launch_head (HeadArgs); `batch` is DevState::batch of the launch (labels_stream).  Written, per model and
 * segment: logits[row][0 .. KP) (KP = ldw; zeros in columns >= classes), dpre[row][0 .. feat), and per 32-row block blk =
 * seg * ceil(rows / 32) + b: loss_part[blk][0 .. 4), part[blk][0 .. feat * KP) = dW6, [off_db .. + KP) = db6,
 * [off_dbf .. + feat) = the feature layer's bias gradient.  HEAD_EVAL adds to *err_count and writes nothing else but logits;
 * HEAD_LOGITS writes logits only.  The saliency kinds (6 .. 8, one segment, labels = targets or null) write dpre, logits where
 * given and, through the err_count field, the target class of every row (int32 [rows], or null).  q8 / q8t (fp8 mode): e5m2 bytes [row][0 .. feat) and [col][0 .. round_up(rows, 32)) (rows
 * beyond `rows` zero), max |dpre| into q8_slot. */
typedef struct mrgan_debug_head_desc {
    int32_t dtype;
    const void* f; int64_t f_bs; int32_t ldf;
    int32_t rows, nseg, seg_kind[3];
    int32_t feat, feat_valid, classes;
    const float* w; int32_t ldw; const float* b;
    const int32_t* labels; int32_t labels_stream; uint32_t batch;
    float inv_count, unl_weight;
    float* logits; int64_t logits_bs;
    void* dpre; int64_t dpre_bs; int32_t ldd;
    float* part; int64_t part_stride; int32_t off_db, off_dbf;
    float* loss_part;
    int32_t models; int64_t model_stride, labels_ms;
    int32_t* err_count;
    void* q8; int64_t q8_bs; int32_t ldq8;
    void* q8t; int64_t q8t_bs; int32_t ldq8t;
    void* q8_slot;
} mrgan_debug_head_desc;
int mrgan_debug_head(const mrgan_debug_head_desc* d, mrgan_stream stream);

/* The matrix-core head (csrc/head_wide.h: HeadWideArgs): launch_w6_split, then launch_head_wide, on one descriptor.  h: as above
 * with bf16 features (h.dtype is ignored), one model, training kinds, feat % 256 == 0; blocks are 64 rows, so blk = seg *
 * ceil(rows / 64) + b in loss_part / part.  mask: the feature layer's lane-native relu mask (csrc/gemm.h), segment s mask_bs
 * uint16 words behind segment 0, [ceil(rows / 32)][ldm][2] words each: dL/d(pre5) follows its bits, not f > 0.  w6c / w6r:
 * scratch the split kernel writes in full, the bf16 addends of W6 class-major [3][ldw][feat] and row-major [3][feat][ldw] (zeros
 * for rows >= feat_valid and columns >= classes; the three addends sum to W6 exactly).  With h.q8_slot the head writes no dpre
 * but the e5m2 images: q8[row][0 .. feat), q8t[col][0 .. round_up(rows, 64)) per segment, 16 bytes at a time. */
typedef struct mrgan_debug_head_wide_desc {
    mrgan_debug_head_desc h;
    const uint16_t* mask; int64_t mask_bs; int32_t ldm;
    void* w6c; void* w6r;
} mrgan_debug_head_wide_desc;
int mrgan_debug_head_wide(const mrgan_debug_head_wide_desc* d, mrgan_stream stream);

/* feature matching (FmArgs; `rb` is the launcher's).  Written: dpre[r][0 .. feat) for r < rows (zeros in columns >= feat_valid
 * and where the mask bit is clear), *loss_out, *accum += loss; with q8_slot the e5m2 bytes q8[r][0 .. feat) and the slot's amax.
 * lscratch / lcount select the distributed loss when feat >= 1024: lscratch[0 .. feat / 64) is written, *lcount must be zero
 * before the launch and is zero after it. */
typedef struct mrgan_debug_fm_desc {
    int32_t dtype;
    const float* cs; int32_t npart_fake, npart_real, ldcs;
    float count, grad_scale; int32_t feat, feat_valid;
    const uint16_t* mask; int32_t ldm;
    void* dpre; int32_t ldd; int32_t rows;
    float* loss_out; float* accum;
    void* q8; int32_t ldq8; void* q8_slot;
    float* lscratch; uint32_t* lcount;
} mrgan_debug_fm_desc;
int mrgan_debug_fm(const mrgan_debug_fm_desc* d, mrgan_stream stream);

/* ---- one launch of the row-block chain kernel (csrc/chain.h: ChainArgs / ChainOp, which document the fields) through
 * launch_chain.  variant: 0 = D tail [F F F H X X X], 1 = G forward [F F F], 2 = G backward [fm X X X]; the products a variant
 * does not run are ignored.  Every data buffer is the caller's device memory (bf16 activations and weights, fp32 bias / cs /
 * head and fm tensors, uint16 mask words); nothing is converted or cleared, the entry allocates only the DevState that carries
 * iter / batch, and it synchronises the stream.  W is [N][K] with pitch K exactly (rows beyond N read as zeros); rows [n_valid, N)
 * of a forward W are the caller's zeros.  head.dtype / f / logits / q8* and fm.dtype / mask / rows / q8* / lscratch / lcount are
 * not read.  Model m's tensors lie model_stride bytes behind model 0's (head: head.model_stride, labels head.labels_ms elements).
 * Written, per model (nrb = ceil(rows / block_rows), npass = ceil(N / 256)) -- and nothing else:
 *   out of a product    out[seg][r][0 .. N) for r < rows (16 bytes at a time); forward columns >= n_valid are zeros
 *   mask of a FORWARD product   words [seg][0 .. ceil(rows / 32))[0 .. N)[2]; the bits of rows >= `rows` in a ragged 32-row
 *                       group are unspecified (those rows carry relu(bias) + noise inside the block).  A dX mask is only read
 *                       (D tail: dx[2].mask alone; dx[0] / dx[1] follow the words fwd[1] / fwd[0] keep in registers)
 *   cs of a product     cs[seg * nrb + rb][0 .. min(256 npass, ldcs)): the column sums of the kept, unrounded values over the
 *                       block's valid rows (forward: before the noise), zeros from column N on
 *   head (D tail)       dpre[seg][r][0 .. feat) for r < rows (zeros from feat_valid on); per block blk = seg * nrb + rb:
 *                       loss_part[blk][0 .. 4), part[blk][0 .. feat * 8) = dW6, [off_db .. + 8) = db6, [off_dbf .. + feat) = the
 *                       feature layer's bias gradient
 *   fm (G backward)     fm.dpre[r][0 .. feat) for r < rows (every segment the same rows), *loss_out, *accum += loss
 * Returns launch_chain's -3 unchanged -- chain_args_ok runs before any device call, so a refused descriptor touches no device
 * -- and -1 for what the launcher takes on trust about memory: a, W, out, fm_feat, fm.dpre, head.dpre / w / part, fm.cs and
 * model_stride not 16-byte aligned; lda / ldo / ldd / fm_ldf / a_bs / out_bs / dpre_bs not a multiple of 8 or a pitch below its
 * width; fm.ldcs not a multiple of 4 or below feat; ldm / ldcs of a product below N; the head's part row layout; an odd row0
 * with gauss.  kname (optional, kname_len bytes) receives "chain_kernel<V, MI, GAUSS, GROUP>" of the instantiation that ran. */
typedef struct mrgan_debug_chain_op {
    int32_t K, N, n_valid;
    const void* W; const float* bias;
    float sigma; uint32_t site;
    void* out; int64_t out_bs; int32_t ldo;
    uint16_t* mask; int64_t mask_bs; int32_t ldm;
    float* cs; int32_t ldcs;
} mrgan_debug_chain_op;
typedef struct mrgan_debug_chain_desc {
    int32_t variant;
    mrgan_debug_chain_op fwd[3], dx[3];
    int32_t rows, nseg, block_rows;
    int32_t models; int64_t model_stride;
    const void* a; int64_t a_bs; int32_t lda, a_cols;
    int32_t seg0; uint64_t seed; uint32_t row0; int32_t gauss;
    uint32_t iter, batch;                /* the DevState of the launch */
    mrgan_debug_head_desc head;
    mrgan_debug_fm_desc fm; const void* fm_feat; int32_t fm_ldf;
} mrgan_debug_chain_desc;
int mrgan_debug_chain(const mrgan_debug_chain_desc* d, char* kname, int kname_len, mrgan_stream stream);

/* multi-tensor Adam (AdamArgs).  `tiles` is a HOST array of ntiles tile descriptors (copied to the device by the entry); every
 * pointer inside is device memory.  iter / batch / lr_t: the DevState the launch reads.  publish_next != 0: the launch gets a
 * `next` slot, pre-filled with 0xA5 bytes, whose four words are returned in next_out (an updating launch writes
 * {iter + 1, batch + advance_batch, bits of lr_t(iter + 2), 0}; a launch that publishes nothing leaves 0xA5A5A5A5).
 * Written per tile (rows x cols, cols % 4 == 0, both <= 64): m, v, p, w16 (and w8) [r][0 .. cols); with wt16 the transposed
 * copy wt16 (and w8t) [c][0 .. round_up(rows, 16)) for c < cols, zeros beyond `rows`; ADAM_REDUCE_ONLY writes flat / flat16
 * [r][0 .. cols) and flat_tail[0 .. 4) only.  The metrics finish (step_out != null) writes step_out[0 .. 3), accum[0 .. 3) +=. */
typedef struct mrgan_debug_adam_tile {
    float* p; float* m; float* v;
    const float* g; int32_t nslab; int64_t slab_stride;
    float* flat; void* flat16;
    void* w16; void* wt16;
    void* w8; void* w8t; void* w8_slot;
    int32_t ld, ldt, rows, cols;
} mrgan_debug_adam_tile;
typedef struct mrgan_debug_adam_desc {
    const mrgan_debug_adam_tile* tiles; int32_t ntiles, mode;
    float b1, b2, eps;
    uint32_t iter, batch; float lr_t;
    const float* loss_part; int32_t nloss_part; float inv_rows; float* step_out; float* accum;
    float* flat_tail;
    int32_t publish_next, advance_batch; float lr;
    int32_t models; int64_t model_stride;
} mrgan_debug_adam_desc;
int mrgan_debug_adam(const mrgan_debug_adam_desc* d, uint32_t next_out[4], mrgan_stream stream);

/* mrgan_svm_gram with the block tile forced (tile = 64 or 128; 0 = the shape's own choice): both tiles give the same bits */
int mrgan_debug_svm_gram(const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n, int64_t d, float gamma,
                         float* out_dev, int64_t ld_out, int32_t tile, mrgan_stream stream);
/* mrgan_svm_kernel_matrix with the block tile forced in the same way */
int mrgan_debug_svm_kernel_matrix(int32_t kernel, const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n,
                                  int64_t d, float gamma, float* out_dev, int64_t ld_out, int32_t tile, mrgan_stream stream);
/* mrgan_svm_gram_group with the launch's one tile forced in the same way */
int mrgan_debug_svm_gram_group(const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma, int32_t tile, mrgan_stream stream);
/* mrgan_svm_kernel_matrix_group with the launch's one tile forced in the same way */
int mrgan_debug_svm_kernel_matrix_group(int32_t kernel, const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma,
                                        int32_t tile, mrgan_stream stream);

/* mrgan_pca_covariance with the block tile (64 or 128; 0 = the shape's own choice) and the number of row ranges (0 = the shape's
 * own choice; more than one per 16 rows is clamped) forced; the workspace query takes the same two */
int64_t mrgan_debug_pca_covariance_workspace_bytes(int64_t n, int64_t d, int32_t tile, int32_t split);
int mrgan_debug_pca_covariance(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, const float* mean_dev, float* cov_dev, int64_t ld_cov,
                               void* work_dev, int64_t work_bytes, int32_t tile, int32_t split, mrgan_stream stream);
/* the orthonormalisation stage of mrgan_pca_eig alone: y_dev [p x d] -> q_dev [p x d], orthonormal rows spanning the rows of Y,
 * sorted by descending lam_dev [p] (float64: the eigenvalues of Y Y^T); rows with lam_j <= 2^-40 lam_1 are zero.  p <= 80;
 * work_dev: what mrgan_pca_eig needs for a block of p rows, 2 p p + 3 p + 2 doubles and 2 p d floats, 8-byte aligned */
int mrgan_debug_pca_orthonormalize(const float* y_dev, int64_t ld_y, int64_t p, int64_t d, void* work_dev, int64_t work_bytes, float* q_dev,
                                   int64_t ld_q, double* lam_dev, mrgan_stream stream);

#ifdef __cplusplus
}
#endif
#endif
