// Loss head, device side (mr_gan.py:128, :146-149, :161): the pieces the head kernels share.
//   head_row                      per-row softmax, losses, train error, closed-form dlogits: head_kernel (aux_kernels.hip, scalar
//                                 fmaf products) and the two matrix-core heads (gemm_chain.hip, head_wide.hip)
//   everything else               the matrix-core heads only (chain_head inside the D-tail chain launch, head_wide_kernel for
//                                 feature layers wider than 256 columns): the three small products as MFMAs at fp32 accuracy
//                                 (see chain_head) over a block of CH_ROWS rows and the 256 feature columns of one LDS image.
// Each kernel keeps its own operand staging (where W6, the label and the relu-mask words come from) and its own barriers.
// KP: the class pitch (aux_kernels.h).  KP = 8 is the layout of chain_head and of every 8-class head; at KP = 32 (head_kernel and
// head_wide_kernel) all 32 columns of the logits product are kept, dL/d(pre5) takes two 16-deep k-steps and dW6^T stores all
// sixteen accumulator registers.
#pragma once
#include "chain.h"

namespace mrgan {

__device__ __forceinline__ bf16x8 zero8() {
    return (bf16x8){(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
}
// v = hi + mid + lo exactly (8 + 8 + 8 significant bits)
__device__ __forceinline__ void split3(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
    hi = (__bf16)v;
    float r = v - (float)hi;            // exact: the remainder of a round-to-nearest has at most 16 significant bits
    mid = (__bf16)r;
    r -= (float)mid;                    // exact: at most 8 significant bits remain
    lo = (__bf16)r;
}

// One row from its bias-free logits l[] (b: the bias, added here; y: the row's label where the kind has one): loss terms, train
// error and dlogits of the row's segment kind.  loss0 = labeled (or MSE) loss, loss1 = unlabeled / fake loss; a row beyond the
// segment gives zeros.
// ALL_KINDS: head_kernel also serves HEAD_MSE, HEAD_EVAL and HEAD_LOGITS; the matrix-core heads are launched with the three
// training kinds only (their launchers check it) and compile those branches out.
// SAL (head_kernel's saliency instantiation only): the row kinds HEAD_SAL_* and nothing else.  dl is the PER-ROW d objective /
// d logits of target class t -- no 1 / batch, no loss terms -- with t = y, or the row's argmax (ties -> first index, as
// HEAD_EVAL decides it) where y < 0; *target receives t.
//   HEAD_SAL_LOGIT  onehot(t)                                   the class score
//   HEAD_SAL_XENT   softmax over the real logits - onehot(t)    HEAD_LAB without the batch mean (mr_gan.py:146)
//   HEAD_SAL_MSE    2 (l - onehot(t)) / classes                 HEAD_MSE without the batch mean
template <bool ALL_KINDS, int KP = KMAX, bool SAL = false>
__device__ __forceinline__ void head_row(float (&l)[KP], const float (&b)[KP], int kind, int y, int classes, float inv_count, float unl_weight,
                                         bool rowvalid, float& loss0, float& loss1, float& err, float (&dl)[KP], int* target = nullptr) {
    static_assert(ALL_KINDS || !SAL, "the saliency kinds belong to head_kernel");
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        if (c < classes) { l[c] += b[c]; mx = fmaxf(mx, l[c]); }
    }
    int am = 0;
    float se = 0.f, p[KP];
#pragma unroll
    for (int c = KP - 1; c >= 0; --c) {
        p[c] = (c < classes) ? expf(l[c] - mx) : 0.f;
        se += p[c];
        if (c < classes && l[c] == mx) am = c;            // ties -> first index (theano argmax)
    }
    const float lse = mx + logf(se);
    const float inv_se = 1.0f / se;
    loss0 = 0.f; loss1 = 0.f; err = 0.f;
#pragma unroll
    for (int c = 0; c < KP; ++c) dl[c] = 0.f;
    if (!rowvalid) return;
    if constexpr (SAL) {
        const int t = y >= 0 ? y : am;
        if (target) *target = t;
        const float invc = 1.0f / (float)classes;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (c < classes) {
                const float oh = c == t ? 1.f : 0.f;
                dl[c] = kind == HEAD_SAL_LOGIT ? oh : kind == HEAD_SAL_XENT ? p[c] * inv_se - oh : 2.0f * (l[c] - oh) * invc;
            }
        }
        return;
    }
    if (ALL_KINDS && kind == HEAD_MSE) {
        // Keras 'mse' on one-hot targets (mr_nn.py:99, :112): mean over the classes, then over the batch
        err = (y >= 0 && am != y) ? 1.f : 0.f;
        const float invc = 1.0f / (float)classes;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (c < classes && y >= 0) {                  // label -1: padding row of a short last batch, no contribution
                const float d = l[c] - (c == y ? 1.f : 0.f);
                loss0 = fmaf(d * d, invc, loss0);
                dl[c] = 2.0f * d * invc * inv_count;
            }
        }
    } else if (kind == HEAD_LAB || (ALL_KINDS && kind == HEAD_EVAL)) {
        err = (am != y) ? 1.f : 0.f;
        if (kind == HEAD_LAB) {
            float ly = 0.f;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                if (c == y) ly = l[c];
                dl[c] = (p[c] * inv_se - (c == y ? 1.f : 0.f)) * inv_count;
            }
            loss0 = lse - ly;
        }
    } else if (!ALL_KINDS || kind != HEAD_LOGITS) {
        const float sg = sigmoid_f(lse), sp = softplus_f(lse);
        const float k = 0.5f * inv_count * unl_weight * (kind == HEAD_UNL ? (sg - 1.0f) : sg);
        loss1 = (kind == HEAD_UNL) ? 0.5f * (sp - lse) : 0.5f * sp;
#pragma unroll
        for (int c = 0; c < KP; ++c) dl[c] = k * p[c] * inv_se;
    }
}
// whether head_row reads the label of a row of this kind
__device__ __forceinline__ bool head_kind_has_label(int kind) { return kind == HEAD_LAB || kind == HEAD_EVAL || kind == HEAD_MSE; }

// ---- logits = F W6: every wave takes 32 of a feature image's 256 columns as its share of the reduction ----
// one k-step (features 16 kg .. 16 kg + 15 of the image) x 2 row tiles x the 3 addends of W6; fb: the B fragments, lane <->
// (class lc, features 16 kg + 8 lh .. + 7), zeros for lc >= KMAX
__device__ __forceinline__ void head_logits_step(f32x16 (&acc)[2], const char* fimg, int kg, const bf16x8 (&fb)[3], int lc, int lh) {
    const char* As = fimg + (kg >> 2) * (CH_ROWS * 128);
    const int ch = (kg & 3) * 2 + lh;
    const bf16x8 fa0 = *(const bf16x8*)(As + kc_off(lc, ch)), fa1 = *(const bf16x8*)(As + kc_off(32 + lc, ch));
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb[p], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb[p], acc[1], 0, 0, 0);
    }
}
// the wave's partial [64][KP] tile -> slot `slot` of lpart [slots][CH_ROWS][head_lpitch(KP)].  KP = 8: one slot per wave, columns
// 8 .. 31 of the product are padding.  KP = 32: eight [64][32] fp32 tiles are 64 KB, more than the kernel has beside its feature
// images, so the tiles meet in FOUR slots in two rounds: waves 0 .. 3 store (head_logits_scatter), and behind a barrier wave
// 4 + i adds its tile to slot i (head_logits_fold; every element belongs to one lane, so the order of the sum is fixed).  The
// row pitch of 36 floats spreads the 64 rows of the gather's 16-byte reads over all banks.
constexpr int head_lpitch(int KP) { return KP == KMAX ? KMAX : KP + 4; }
constexpr int head_lslots(int KP) { return KP == KMAX ? CH_THREADS / 64 : CH_THREADS / 128; }
template <int KP = KMAX>
__device__ __forceinline__ void head_logits_scatter(const f32x16 (&acc)[2], float* lpart, int slot, int lc, int lh) {
    if (lc < KP) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) lpart[(slot * CH_ROWS + mi * 32 + acc_row(r, lh)) * head_lpitch(KP) + lc] = acc[mi][r];
    }
}
template <int KP>
__device__ __forceinline__ void head_logits_fold(const f32x16 (&acc)[2], float* lpart, int slot, int lc, int lh) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) lpart[(slot * CH_ROWS + mi * 32 + acc_row(r, lh)) * head_lpitch(KP) + lc] += acc[mi][r];
}
// row r's logits: the sum of the slots, slot 0 first
template <int KP = KMAX>
__device__ __forceinline__ void head_logits_gather(const float* lpart, int r, float (&l)[KP]) {
#pragma unroll
    for (int c = 0; c < KP; ++c) l[c] = 0.f;
#pragma unroll
    for (int w = 0; w < head_lslots(KP); ++w) {
        f32x4 p[KP / 4];
#pragma unroll
        for (int g = 0; g < KP / 4; ++g) p[g] = *(const f32x4*)(lpart + (w * CH_ROWS + r) * head_lpitch(KP) + 4 * g);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < KP / 4; ++g) l[4 * g + c] += p[g][c];
    }
}

// ---- row r's results -> LDS: dlogits as bf16 addends dl_rc [3][CH_ROWS][KP] (row-major, A operand of dL/d(pre5)) and
// dl_t [3][KP][CH_ROWS] (class-major, A operand of dW6^T), and red [3 + KP][CH_ROWS] ----
template <int KP = KMAX>
__device__ __forceinline__ void head_rows_to_lds(const float (&dl)[KP], float loss0, float loss1, float err, int r, __bf16* dl_rc, __bf16* dl_t,
                                                 float* red) {
    bf16x8 d3[3][KP / 8];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        __bf16 p0, p1, p2;
        split3(dl[c], p0, p1, p2);
        d3[0][c >> 3][c & 7] = p0; d3[1][c >> 3][c & 7] = p1; d3[2][c >> 3][c & 7] = p2;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int g = 0; g < KP / 8; ++g) *(bf16x8*)(dl_rc + (q * CH_ROWS + r) * KP + 8 * g) = d3[q][g];
#pragma unroll
        for (int c = 0; c < KP; ++c) dl_t[(q * KP + c) * CH_ROWS + r] = d3[q][c >> 3][c & 7];
    }
    // the 3 + KP per-row quantities whose sums over the 64 rows leave the block (three loss terms, db6 = column sums of
    // dlogits): to LDS, row-contiguous; 3 + KP lanes of the last wave add them up behind the barrier (as wave-wide shuffle
    // reductions -- eleven six-step ds_bpermute chains on this one wave at KP = 8 -- they cost ~3 us with the other seven waves
    // waiting)
    red[0 * CH_ROWS + r] = loss0; red[1 * CH_ROWS + r] = loss1; red[2 * CH_ROWS + r] = err;
#pragma unroll
    for (int c = 0; c < KP; ++c) red[(3 + c) * CH_ROWS + r] = dl[c];
}
// ... and the 3 + KP sums (behind a barrier): loss terms -> loss_part[blk], db6 -> the block's partial-gradient row
template <int KP = KMAX>
__device__ __forceinline__ void head_block_sums(const float* red, const HeadArgs& h, int blk, float* part_row, int wave, int lane,
                                                long moff = 0 /* model groups: bytes to this model's loss_part */) {
    if (wave == CH_THREADS / 64 - 1 && lane < 3 + KP) {
        float* const loss_part = (float*)((char*)h.loss_part + moff);
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CH_ROWS / 4; ++i) {
            const f32x4 v = *(const f32x4*)(red + lane * CH_ROWS + 4 * i);
            s4[i & 3] += (v[0] + v[1]) + (v[2] + v[3]);
        }
        const float tot = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        if (lane < 3) loss_part[blk * 4 + lane] = tot;
        else part_row[h.off_db + lane - 3] = tot;
        if (lane == 0) loss_part[blk * 4 + 3] = 0.f;
    }
}

// ---- dL/d(pre5) = (dlogits W6^T) * relu'(pre5) for the wave's 32 feature columns.  KP = 8: one 16-deep k-step (8 classes +
// 8 zeros).  KP = 32: two k-steps, classes 0 .. 15 and 16 .. 31 ----
// A fragments of k-step ks: the dlogits addends of rows 32 mi + lc.  KP = 8: lh = 1 is k = 8 .. 15, padding.  KP = 32: lane <->
// classes 16 ks + 8 lh .. + 7
template <int KP = KMAX>
__device__ __forceinline__ void head_load_dl_rows(const __bf16* dl_rc, int lc, int lh, bf16x8 (&da)[2][3], int ks = 0) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if constexpr (KP == KMAX) {
                da[mi][q] = *(const bf16x8*)(dl_rc + (q * CH_ROWS + mi * 32 + lc) * KMAX);
                if (lh) da[mi][q] = zero8();
            } else {
                da[mi][q] = *(const bf16x8*)(dl_rc + (q * CH_ROWS + mi * 32 + lc) * KP + 16 * ks + 8 * lh);
            }
        }
}
// NKS k-steps; bw: the W6 addends of this lane's feature (k = class; KP = 8: zeros for lh = 1).  The smallest terms of ALL
// k-steps come first: every MFMA rounds its sum at the size of the accumulator, so only the NKS (hi, hi) products at the end
// round at the size of the result.  (k-step by k-step, the five small pairs of the second step would each round a full-size
// accumulator: seven such roundings instead of two, and visibly more bf16 results that differ from head_kernel's.)
template <int NKS>
__device__ __forceinline__ void head_dpre_product(f32x16 (&acc)[2], const bf16x8 (&da)[NKS][2][3], const bf16x8 (&bw)[NKS][3]) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
    // addend pairs down to 2^-24 of the product: (hi, hi) (hi, mid) (mid, hi) (hi, lo) (lo, hi) (mid, mid)
    constexpr int PA[6] = {0, 0, 1, 0, 2, 1}, PB[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
    for (int i = 5; i >= 0; --i)                              // smallest terms first
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[ks][mi][PA[i]], bw[ks][PB[i]], acc[mi], 0, 0, 0);
}
// the masked product as bf16 into column cip of an activation image (the next product's A operand); returns this lane's
// share of the column sum (the feature layer's bias gradient)
__device__ __forceinline__ float head_dpre_to_image(const f32x16 (&acc)[2], const uint32_t (&mw)[2], char* oimg, int cip, int lh) {
    int obase[4];
    img_col_bases<CH_ROWS>(obase, cip, lh);
    float s1 = 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float av = acc[mi][r];
            const float v = ((mw[mi] >> r) & 1u) ? av : 0.f;  // (a select: see chain_gemm)
            s1 += v;
            *(__bf16*)(oimg + img_elem_off(obase, mi, r)) = (__bf16)v;
        }
    return s1;
}

// ---- dW6^T [class][feature] = dlogits^T F for the wave's 32 features: registers 4 g .. 4 g + 3 of the result are classes
// 8 g + 4 lh .. + 3 of feature 32 wave + lc (KP = 8: only g = 0 is stored) ----
// A fragments of k-step ks (rows 16 ks .. + 15): lane <-> (class lc, rows 16 ks + 8 lh .. + 7), zeros for lc >= KP
template <int KP = KMAX>
__device__ __forceinline__ void head_load_dl_cols(const __bf16* dl_t, int ks, int lc, int lh, bf16x8 (&fa)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        fa[q] = *(const bf16x8*)(dl_t + (q * KP + (lc & (KP - 1))) * CH_ROWS + 16 * ks + 8 * lh);
        if (KP < 32 && lc >= KP) fa[q] = zero8();
    }
}
__device__ __forceinline__ void head_dw6t_step(f32x16& acc, const char* fimg, int ks, const bf16x8 (&fa)[3], int wave, int lane) {
    const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    const int f0 = wave * 32 + (g4 & 1) * 16 + 4 * pp;
    // B fragment: eight consecutive rows (k) of this lane's feature column, by the transposing read
    const int m0 = ks * 16 + (g4 >> 1) * 8 + q;
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(fimg + act_off(m0, f0)));
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(fimg + act_off(m0 + 4, f0)));
    const bf16x8 fb = __builtin_bit_cast(bf16x8, __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
    for (int p = 2; p >= 0; --p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[p], fb, acc, 0, 0, 0);
}

}  // namespace mrgan
