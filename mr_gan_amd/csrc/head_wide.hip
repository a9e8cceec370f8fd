// Stand-alone loss head on the matrix cores (head_wide.h): the D sub-step's head where the D-tail chain does not run.
#include "head_wide.h"

#include "gemm.h"
#include "head.h"

namespace mrgan {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// Stand-alone loss head for wide feature layers (head_wide.h: HeadWideArgs).  The same three MFMA products as chain_head, with the
// feature dimension walked in chunks of 256 columns: the block's 64 rows x 256 features arrive by LDS-DMA into one of two
// images (the next chunk is in flight while the current one is consumed), wave w owns features [32 w, 32 w + 32) of a chunk.
//   pass 1 (chunks ascending): logits partial products, accumulated over ALL chunks in the wave's registers
//   row phase (wave 0): losses, error, dlogits as bf16 addends
//   pass 2 (chunks descending: the last chunk is still resident): dL/d(pre5) of the chunk -> output images -> HBM, dW6^T
// W6 enters as bf16 addends prepared once per launch by w6_split_kernel (class-major for the logits' B operand, row-major for
// dL/d(pre5)'s), so a fragment is one 16-byte load from a 200 KB array that stays in L2.
// Q8: dL/d(pre5) leaves as the two e5m2 images the fp8 products read (row-major and transposed), packed from the accumulators:
// a lane's four consecutive rows of one column are one dword of the transposed image, the row-major dword comes from a 4 x 4
// byte transpose inside the lane quad (gemm.h does the same in the fp8 epilogues); both images are assembled in LDS and leave
// as 16-byte stores.  Otherwise dL/d(pre5) leaves as bf16 through the chain's image + copy_out.
// KP: the class pitch.  KP = 32 (9 .. 32 classes, bf16 only) keeps all 32 columns of the logits product, folds the eight partial
// logits tiles into four LDS slots in two rounds (head.h: head_logits_fold), runs dL/d(pre5) as two k-steps and stores all
// sixteen registers of dW6^T; it also serves a 256-wide feature layer as a single chunk (the D-tail chain is an 8-class kernel).
// ------------------------------------------------------------------------------------------------------------------
constexpr int HW_FIMG = CH_ROWS * CH_PW * 2;                  // 32 KiB per feature image
constexpr int HW_TPITCH = CH_ROWS + 16, HW_RPITCH = CH_PW + 16;
constexpr int HW_X = 2 * HW_FIMG, HW_X_BYTES = 40 * 1024;     // pass 1: logits partials; pass 2: output image(s)
constexpr int HW_SMALL = HW_X + HW_X_BYTES;
constexpr int hw_lds(int KP) { return HW_SMALL + 2 * 3 * CH_ROWS * KP * 2 + (3 + KP) * CH_ROWS * 4; }
constexpr int HW_LDS = hw_lds(KMAX);
static_assert(CH_PW * HW_TPITCH + CH_ROWS * HW_RPITCH <= HW_X_BYTES && 8 * CH_ROWS * KMAX * 4 <= HW_X_BYTES, "head_wide LDS map");
static_assert(head_lslots(KWIDE) * CH_ROWS * head_lpitch(KWIDE) * 4 <= HW_X_BYTES && hw_lds(KWIDE) <= 160 * 1024, "head_wide LDS map, 32 classes");

template <int KP>
__global__ __launch_bounds__(256) void w6_split_kernel(const float* w, int ldw, int feat, int feat_valid, int classes, __bf16* w6c, __bf16* w6r) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= feat) return;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        const float v = (j < feat_valid && c < classes) ? w[(long)j * ldw + c] : 0.f;
        __bf16 p0, p1, p2;
        split3(v, p0, p1, p2);
        w6c[(0L * KP + c) * feat + j] = p0; w6c[(1L * KP + c) * feat + j] = p1; w6c[(2L * KP + c) * feat + j] = p2;
        w6r[(0L * feat + j) * KP + c] = p0; w6r[(1L * feat + j) * KP + c] = p1; w6r[(2L * feat + j) * KP + c] = p2;
    }
}

template <bool Q8, int KP = KMAX>
__global__ __launch_bounds__(CH_THREADS) void head_wide_kernel(const HeadWideArgs a) {
    static_assert(KP == KMAX || !Q8, "the e5m2 epilogue exists at the 8-class pitch only");
    constexpr int NKS = KP == KMAX ? 1 : KP / 16;             // k-steps of the dL/d(pre5) product
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const HeadArgs& h = a.h;
    char* xreg = lds + HW_X;
    __bf16* dl_rc = (__bf16*)(lds + HW_SMALL);                // [3][CH_ROWS][KP]   dlogits addends, row-major
    __bf16* dl_t = dl_rc + 3 * CH_ROWS * KP;                  // [3][KP][CH_ROWS]   ... class-major
    float* red = (float*)(dl_t + 3 * KP * CH_ROWS);           // [3 + KP][CH_ROWS]
    const int t = threadIdx.x, lane = t & 63, lc = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int seg = blockIdx.y, rb = blockIdx.x, nrb = gridDim.x, kind = h.seg_kind[seg];
    const int row_blk = rb * CH_ROWS, rows_valid = min(CH_ROWS, h.rows - row_blk), blk = seg * nrb + rb;
    const int nch = h.feat / CH_PW;

    // ---- feature chunks by LDS-DMA: [4 k-tiles][64 rows][64 k] with the chain's swizzle; rows >= h.rows arrive as zeros ----
    const __bf16* fseg = (const __bf16*)h.f + (long)seg * h.f_bs;
    const __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc((void*)fseg, 0, (int)((long)h.rows * h.ldf * 2), 0x00020000);
    int fvoff[4], fdst[4];
    {
        const int lrow = lane >> 3, lp = lane & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pce = wave + 8 * i, kt = pce >> 3, pr = pce & 7, R = pr * 8 + lrow;
            fvoff[i] = (int)(((long)(row_blk + R) * h.ldf + kt * 64 + ((lp ^ ((R >> 1) & 7)) << 3)) * 2);
            fdst[i] = kt * (CH_ROWS * 128) + pr * 1024;
        }
    }
    auto issue_chunk = [&](int c) {
        char* img = lds + (c & 1) * HW_FIMG;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(rsF, img + fdst[i], fvoff[i], c * (CH_PW * 2));
    };
    // B fragments of the logits product for chunk c: lane <-> (class lc, features 16 (2 wave + u) + 8 lh .. + 7 of the chunk)
    auto load_w6c = [&](int c, bf16x8 (&fb)[2][3]) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const bf16x8 v = *(const bf16x8*)(a.w6c + ((long)p * KP + (lc & (KP - 1))) * h.feat + c * CH_PW + 16 * (2 * wave + u) + 8 * lh);
                fb[u][p] = (KP == 32 || lc < KP) ? v : zero8();   // KP = 8: columns 8 .. 31 of the product are padding; KP = 32:
                                                                // w6_split_kernel left zeros in the columns >= classes
            }
    };

    // =========================== pass 1: logits ===========================
    f32x16 lacc[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[mi][r] = 0.f;
    bf16x8 fbn[2][3];
    issue_chunk(0);
    load_w6c(0, fbn);
    for (int c = 0; c < nch; ++c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of chunk c and its W6 fragments
        __builtin_amdgcn_s_barrier();                         // ... everyone's pieces; everyone is done with chunk c - 1
        asm volatile("" ::: "memory");
        bf16x8 fb[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[u][p] = fbn[u][p];
        if (c + 1 < nch) { issue_chunk(c + 1); load_w6c(c + 1, fbn); }
        const char* fimg = lds + (c & 1) * HW_FIMG;
#pragma unroll
        for (int u = 0; u < 2; ++u) head_logits_step(lacc, fimg, 2 * wave + u, fb[u], lc, lh);
    }
    float* lpart = (float*)xreg;                              // [head_lslots(KP)][CH_ROWS][head_lpitch(KP)]
    if constexpr (KP == KMAX) {
        head_logits_scatter(lacc, lpart, wave, lc, lh);
    } else {
        // eight [64][32] tiles into four slots: waves 0 .. 3 store, then wave 4 + i adds to slot i (a fixed order of the sum)
        if (wave < head_lslots(KP)) head_logits_scatter<KP>(lacc, lpart, wave, lc, lh);
        lds_barrier();
        if (wave >= head_lslots(KP)) head_logits_fold<KP>(lacc, lpart, wave - head_lslots(KP), lc, lh);
    }
    lds_barrier();
    // the chunk before the last one is needed next (pass 2 walks downwards): its image is free now
    if (nch > 1) issue_chunk(nch - 2);

    // =========================== row phase (wave 0: lane <-> row), as chain_head step 3 ===========================
    float* part_row = h.part + (long)blk * h.part_stride;
    if (wave == 0) {
        const int r = lane;
        const bool rowvalid = r < rows_valid;
        float l[KP];
        head_logits_gather(lpart, r, l);
        float b[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) b[c] = (c < h.classes) ? h.b[c] : 0.f;
        int y = 0;
        if (rowvalid && kind == HEAD_LAB) {
            const long lo = h.labels_stream ? (long)h.st->batch * h.rows : 0;
            y = h.labels[lo + row_blk + r];
        }
        float loss0, loss1, err, dl[KP];
        head_row<false>(l, b, kind, y, h.classes, h.inv_count, h.unl_weight, rowvalid, loss0, loss1, err, dl);
        if (rowvalid && h.logits) {
            float* lp = h.logits + (long)seg * h.logits_bs + (long)(row_blk + r) * KP;
#pragma unroll
            for (int c = 0; c < KP; ++c) lp[c] = (c < h.classes) ? l[c] : 0.f;
        }
        head_rows_to_lds(dl, loss0, loss1, err, r, dl_rc, dl_t, red);
    }
    lds_barrier();
    head_block_sums<KP>(red, h, blk, part_row, wave, lane);

    // =========================== pass 2: dL/d(pre5) and dW6^T, chunk by chunk ===========================
    // A operands that do not depend on the chunk, in registers for the whole pass
    bf16x8 da[NKS][2][3], dt[4][3];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) head_load_dl_rows<KP>(dl_rc, lc, lh, da[ks], ks);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) head_load_dl_cols<KP>(dl_t, ks, lc, lh, dt[ks]);
    const uint16_t* mseg = a.mask + (long)seg * a.mask_bs;
    // per chunk: the W6 rows of this lane's feature as bf16 addends (B operand, k = class) and the relu-mask words of its column
    // (KP = 32: k-step ks holds classes 16 ks + 8 lh .. + 7)
    auto load_chunk_inputs = [&](int c, bf16x8 (&bw)[NKS][3], uint32_t (&mw)[2]) {
        const int col = c * CH_PW + wave * 32 + lc;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if constexpr (KP == KMAX) {
                const bf16x8 v = *(const bf16x8*)(a.w6r + ((long)q * h.feat + col) * KMAX);
                bw[0][q] = lh ? zero8() : v;                    // lh = 1: k = 8 .. 15, zeros
            } else {
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) bw[ks][q] = *(const bf16x8*)(a.w6r + ((long)q * h.feat + col) * KP + 16 * ks + 8 * lh);
            }
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const bool ok = row_blk + mi * 32 < h.rows;
            const uint32_t w = mseg[((long)((ok ? row_blk + mi * 32 : 0) >> 5) * a.ldm + col) * 2 + lh];
            mw[mi] = ok ? w : 0u;
        }
    };
    const float q8s = Q8 ? h.q8_slot->scale : 1.f;
    float q8_amax = 0.f;
    bf16x8 bwn[NKS][3];
    uint32_t mwn[2];
    load_chunk_inputs(nch - 1, bwn, mwn);
    for (int c = nch - 1; c >= 0; --c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // chunk c (this wave's pieces), its inputs; the previous copy-out
        __builtin_amdgcn_s_barrier();                         // ... everyone's: the output region and chunk c + 1's image are free
        asm volatile("" ::: "memory");
        bf16x8 bw[NKS][3];
        uint32_t mw[2];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int q = 0; q < 3; ++q) bw[ks][q] = bwn[ks][q];
        mw[0] = mwn[0]; mw[1] = mwn[1];
        if (c >= 1) load_chunk_inputs(c - 1, bwn, mwn);
        if (c >= 1 && c != nch - 1) issue_chunk(c - 1);       // (chunk nch - 2 was issued before the row phase)
        const char* fimg = lds + (c & 1) * HW_FIMG;
        const int c0 = c * CH_PW, cip = wave * 32 + lc;
        // ---- dL/d(pre5) = (dlogits W6^T) * relu'(pre5): NKS 16-deep k-steps x 6 addend pairs ----
        {
            f32x16 acc[2];
            head_dpre_product<NKS>(acc, da, bw);
            float s1 = 0.f;
            if constexpr (Q8) {
                unsigned char* timg = (unsigned char*)xreg;
                unsigned char* rimg = timg + CH_PW * HW_TPITCH;
                const int kq = lane & 3;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float o4[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int r = 4 * g + j;
                            const float av = acc[mi][r];
                            o4[j] = ((mw[mi] >> r) & 1u) ? av : 0.f;              // (a select: see chain_gemm)
                            s1 += o4[j];
                            q8_amax = fmaxf(q8_amax, fabsf(o4[j]));
                        }
                        const uint32_t w = fp8_pack4<FP8_E5M2>(o4[0], o4[1], o4[2], o4[3], q8s);
                        const int rl = mi * 32 + 8 * g + 4 * lh;                    // rows rl .. rl + 3 of column cip
                        *(uint32_t*)(timg + cip * HW_TPITCH + rl) = w;
                        *(uint32_t*)(rimg + (rl + kq) * HW_RPITCH + (cip - kq)) = quad_byte_transpose(w);
                    }
            } else {
                s1 = head_dpre_to_image(acc, mw, xreg, cip, lh);
            }
            s1 += __shfl_xor(s1, 32, 64);
            if (lh == 0) part_row[h.off_dbf + c0 + cip] = s1;                   // bias gradient of the feature layer
        }
        // ---- dW6^T [class][feature] = dlogits^T F for this wave's 32 features of the chunk ----
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < CH_ROWS / 16; ++ks) head_dw6t_step(acc, fimg, ks, dt[ks], wave, lane);
#pragma unroll
            for (int g = 0; g < KP / 8; ++g)                  // registers 4 g .. 4 g + 3 = classes 8 g + 4 lh .. + 3
                *(f32x4*)(part_row + (long)(c0 + cip) * KP + 8 * g + 4 * lh) = (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        }
        lds_barrier();                                        // the output image(s) of the chunk are complete
        if constexpr (Q8) {
            const unsigned char* timg = (const unsigned char*)xreg;
            const unsigned char* rimg = timg + CH_PW * HW_TPITCH;
            unsigned char* q8t = h.q8t ? h.q8t + (long)seg * h.q8t_bs : nullptr;
            unsigned char* q8 = h.q8 ? h.q8 + (long)seg * h.q8_bs : nullptr;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qi = t + CH_THREADS * u;
                // transposed copy: column (row of q8t) x 16 rows; rows >= h.rows of the block are zero bytes (zero dlogits)
                if (q8t) *(u32x4*)(q8t + (long)(c0 + (qi >> 2)) * h.ldq8t + row_blk + 16 * (qi & 3)) = *(const u32x4*)(timg + (qi >> 2) * HW_TPITCH + 16 * (qi & 3));
                if (q8 && (qi >> 4) < rows_valid) *(u32x4*)(q8 + (long)(row_blk + (qi >> 4)) * h.ldq8 + c0 + 16 * (qi & 15)) = *(const u32x4*)(rimg + (qi >> 4) * HW_RPITCH + 16 * (qi & 15));
            }
        } else {
            copy_out<CH_ROWS>(xreg, (__bf16*)h.dpre + (long)seg * h.dpre_bs + (long)row_blk * h.ldd, h.ldd, c0, h.feat, rows_valid, t);
        }
    }
    if constexpr (Q8) fp8_amax_commit(h.q8_slot, q8_amax);
}

}  // namespace

// the bf16 addends of W6 for launch_head_wide (once per D sub-step: W6 changes with every Adam update)
int launch_w6_split(const HeadWideArgs& a, hipStream_t s) {
    const HeadArgs& h = a.h;
    if (!a.w6c || !a.w6r || !h.w) return -3;
    if (h.ldw == KWIDE) MRGAN_LAUNCH(w6_split_kernel<KWIDE>, dim3((h.feat + 255) / 256), dim3(256), 0, s, h.w, h.ldw, h.feat, h.feat_valid, h.classes, a.w6c, a.w6r);
    else MRGAN_LAUNCH(w6_split_kernel<KMAX>, dim3((h.feat + 255) / 256), dim3(256), 0, s, h.w, h.ldw, h.feat, h.feat_valid, h.classes, a.w6c, a.w6r);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_head_wide(const HeadWideArgs& a, hipStream_t s) {
    const HeadArgs& h = a.h;
    const int kp = h.ldw;                                     // the class pitch of W6, its addends, the logits and the partial rows
    if ((h.feat % CH_PW) != 0 || (kp != KMAX && kp != KWIDE) || h.classes > kp || !a.mask || !a.w6c || !a.w6r || !h.part || !h.loss_part) return -3;
    for (int i = 0; i < h.nseg; ++i)
        if (h.seg_kind[i] != HEAD_LAB && h.seg_kind[i] != HEAD_UNL && h.seg_kind[i] != HEAD_FAKE) return -3;
    if ((long)h.rows * h.ldf * 2 >= (1L << 31)) return -3;
    const bool q8 = h.q8_slot != nullptr;
    if (q8 ? !(h.q8 || h.q8t) : !h.dpre) return -3;
    // (the dynamic-LDS limit of both instantiations is raised by head_wide_init_attributes, outside any stream capture)
    const dim3 grid((h.rows + CH_ROWS - 1) / CH_ROWS, h.nseg), block(CH_THREADS);
    if (kp == KWIDE) {
        if (q8) return -3;
        MRGAN_LAUNCH((head_wide_kernel<false, KWIDE>), grid, block, hw_lds(KWIDE), s, a);
    } else if (q8) MRGAN_LAUNCH((head_wide_kernel<true>), grid, block, HW_LDS, s, a);
    else MRGAN_LAUNCH((head_wide_kernel<false>), grid, block, HW_LDS, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// the dynamic-LDS limits, raised once per handle outside any stream capture (mrgan_create)
int head_wide_init_attributes() {
    hipError_t e = hipFuncSetAttribute((const void*)head_wide_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, HW_LDS);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)head_wide_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, HW_LDS);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)head_wide_kernel<false, KWIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, hw_lds(KWIDE));
    return e == hipSuccess ? 0 : -2;
}

}  // namespace mrgan
