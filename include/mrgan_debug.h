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

#ifdef __cplusplus
}
#endif
#endif
