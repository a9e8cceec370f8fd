// Row-block chain kernel (see chain.h): consecutive dense products of one 64-row block inside one launch.
//
// One workgroup = 8 waves = one block of 64 rows of one segment.  The block's current activation is an LDS image
// [K/64 k-tiles][64 rows][64 k] bf16 with the XOR swizzle of the stand-alone forward kernels (lds_ring.h: kc_off), so the
// MFMA A fragments are conflict-free ds_read_b128; the weights stream through a 2-stage ring of [256 columns][64 k] tiles
// filled by LDS-DMA (lds_ring.h: glds16) from the XCD's L2 -- a per-wave, barrier-free ring of its own (BTile, wait_vm).
// Wave w owns output columns [32 w, 32 w + 32) of a 256-column pass over all 64 rows (two 32x32 accumulators): its column
// sums need no cross-wave step, and the epilogue writes the bf16 result straight into the LDS image that is the next
// product's A operand; a copy of it leaves for HBM in 16-byte stores because the weight-gradient launch needs every
// layer's input and output gradient.
// The ring never drains between products: the weight tile stream is one flat sequence over (product, pass, k-tile), and
// the first tile of the next product is already in flight while the current epilogue runs.
#include <algorithm>

#include "chain.h"
#include "gemm.h"
#include "head.h"

namespace mrgan {
namespace {

// wait until at most n of this wave's vector-memory operations are outstanding (they retire in issue order)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    }
}

// per-phase cycle counters of the diagnostic build (make STAMPS=1: [block][8] to ChainArgs::stamps); empty otherwise, and
// passed along all the same
#ifdef MRGAN_STAMPS
struct Stamps {
    unsigned long long acc[8], prev;
    __device__ void start() { for (int i = 0; i < 8; ++i) acc[i] = 0; prev = __builtin_amdgcn_s_memtime(); }
    __device__ void store(unsigned long long* out) const { if (out) for (int i = 0; i < 8; ++i) out[((long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + i] = acc[i]; }
};
#define CH_STAMP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); st.acc[i] += n_ - st.prev; st.prev = n_; } while (0)
#else
struct Stamps {
    __device__ void start() {}
    __device__ void store(unsigned long long*) const {}
};
#define CH_STAMP(i)
#endif

// The weight tiles of a chain form one flat sequence over (product, pass, k-tile): the tile issued while tile g is consumed is
// tile g + 1 -- of this product, or the first tile of the next one, whose three scalars (Bt, K, N) the caller passes along.
// Everything the issue needs lives in registers for the whole product (a descriptor in SGPRs, four per-lane row offsets): no
// load from the argument block inside the k-loops.
struct BTile {
    __amdgpu_buffer_rsrc_t rs; int voff[4]; int pass_bytes;       // byte offset of 256 more columns of Bt
};
__device__ __forceinline__ void btile_setup(BTile& b, const __bf16* W, int K, int N, int wave, int lane) {
    b.rs = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, (int)((long)N * K * 2), 0x00020000);      // rows >= N of Bt read as zeros
    const int lrow = lane >> 3, lp = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int R = (wave * 4 + i) * 8 + lrow;                   // column of the pass = row of Bt
        b.voff[i] = (R * K + ((lp ^ ((R >> 1) & 7)) << 3)) * 2;
    }
    b.pass_bytes = CH_PW * K * 2;
}
// one weight tile [256 columns][64 k] into a ring stage: 4 wave-instructions per wave, each wave its own 32 columns
__device__ __forceinline__ void issue_btile(const BTile& b, int pass, int kt, char* stage, int wave) {
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(b.rs, stage + (wave * 4 + i) * 1024, b.voff[i] + pass * b.pass_bytes, kt * 128);
}

// Shared state of the weight-tile stream of one block (all wave-uniform)
struct Stream {
    int gtile;                 // tiles consumed so far: tile g lives in ring stage g % (number of stages)
    int inflight;              // tiles issued and not yet consumed (tile gtile is the oldest)
    // The copy of a finished output image to HBM is DEFERRED to the end of the next pass's k-loop.  Stores count in vmcnt in issue
    // order with the weight-tile DMAs: issued right behind the image barrier (round 2) they sat in front of the next tile's
    // DMA, and the wait for that tile -- one k-tile of MFMAs later -- also waited for the stores' acknowledgement (~1 us per
    // pass, measured by ablation).  At the end of a k-loop the only DMA in flight is OLDER than the stores (the next product's
    // first tile), and the following wait comes a whole epilogue later.  The image is read-only until the product after next.
    const char* cp_img; __bf16* cp_out; int cp_ldo, cp_col0, cp_ncols;
};
template <int ROWS = CH_ROWS>
__device__ __forceinline__ void flush_copy(Stream& sm, int rows_valid, int t) {
    if (sm.cp_img) copy_out<ROWS>(sm.cp_img, sm.cp_out, sm.cp_ldo, sm.cp_col0, sm.cp_ncols, rows_valid, t);
    sm.cp_img = nullptr;
}

// ------------------------------------------------------------------------------------------------------------------
// loss head on the block's 64 rows (mr_gan.py:128, :146-149, :161), on the matrix cores.
// The three small products of the head -- logits = F W6, dL/d(pre5) = (dlogits W6^T) * relu', dW6 = F^T dlogits -- were scalar
// fmaf loops (24 k cycles per block, 22 % of the launch for 0.1 % of its FLOPs).  They are MFMA products now, at fp32
// accuracy: the features are exact bf16 values already, and every fp32 factor (W6, dlogits) enters as THREE bf16 addends
// hi + mid + lo that reproduce it exactly (8 + 8 + 8 significant bits), so each bf16 x bf16 product is exact in the fp32
// accumulator and only the summation order differs from head_kernel's fmaf chain (aux_kernels.hip).
//   1. W6 -> LDS as [3 addends][class][feature] bf16 (the B operand of the logits product, k = feature contiguous)
//   2. logits: every wave takes 32 of the features as its share of the reduction (2 k-steps x 2 row tiles x 3 addends), the
//      eight partial [64][8] tiles meet in LDS
//   3. wave 0, one lane per row: softmax / losses / closed-form dlogits, dlogits -> LDS as bf16 addends, row-major
//      (A operand of 4) and class-major (A operand of 5)
//   4. dL/d(pre5) for the wave's 32 feature columns: one 16-deep k-step (8 classes + 8 zeros) x 6 addend pairs, masked with
//      the relu bits the D5 forward epilogue left in registers, written as the next product's A image (+ bias-gradient sums)
//   5. dW6^T [class][feature] = dlogits^T F for the wave's 32 features: F enters through the transposing LDS read
// The products, the row arithmetic and the LDS hand-over between them are head.h's; what is here is this kernel's staging.
// ------------------------------------------------------------------------------------------------------------------

// what the head reads from global memory, fetched in the kernel's prologue: inside the head each of these would be an exposed
// L2 / HBM round trip with the whole block waiting at the next barrier (the labels even two dependent ones)
struct HeadInputs { f32x4 w0, w1, bw0, bw1, b0, b1; int label; };
template <bool GROUP>
__device__ __forceinline__ void head_prefetch(const ChainArgs& a, HeadInputs& hi, int seg, int row_blk, int rows_valid, int t) {
    const HeadArgs& h = a.head;
    const int lane = t & 63, lc = lane & 31, wave = t >> 6;
    const int k = min(t & (CH_PW - 1), h.feat_valid - 1), j = min(wave * 32 + lc, h.feat_valid - 1);
    const long hoff = chain_moff<GROUP>(h.model_stride);      // model groups: this model's W6 / b6 (bytes) and labels (elements)
    const float* const w6 = chain_model(h.w, hoff);
    const float* const b6 = chain_model(h.b, hoff);
    hi.w0 = *(const f32x4*)(w6 + (long)k * h.ldw); hi.w1 = *(const f32x4*)(w6 + (long)k * h.ldw + 4);
    hi.bw0 = *(const f32x4*)(w6 + (long)j * h.ldw); hi.bw1 = *(const f32x4*)(w6 + (long)j * h.ldw + 4);
    hi.b0 = (f32x4){0.f, 0.f, 0.f, 0.f}; hi.b1 = hi.b0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { hi.b0[c] = b6[min(c, h.classes - 1)]; hi.b1[c] = b6[min(4 + c, h.classes - 1)]; }
    hi.label = 0;
    if (h.seg_kind[seg] == HEAD_LAB) {
        const long lo = (h.labels_stream ? (long)h.st->batch * h.rows : 0) + chain_moff<GROUP>(h.labels_ms);
        hi.label = h.labels[lo + row_blk + min(lane, rows_valid - 1)];
    }
}

template <bool GROUP>
__device__ __forceinline__ void chain_head(const ChainArgs& a, char* lds, Stream& sm, const HeadInputs& hi, const uint32_t (&mw)[2][2], int seg,
                                           int rb, int nrb, int row_blk, int rows_valid, int t) {
    const HeadArgs& h = a.head;
    const char* fimg = lds + chain_img(CH_ROWS, 1);           // the features: the third forward product's output (chain.h)
    char* oimg = lds + chain_img(CH_ROWS, 0);                 // dL/d(pre5): the first dX product's A image
    __bf16* w6t = (__bf16*)(lds + chain_head_scratch());      // [3][KMAX][CH_PW]
    __bf16* dl_rc = w6t + 3 * KMAX * CH_PW;                   // [3][CH_ROWS][KMAX]   dlogits addends, row-major
    __bf16* dl_t = dl_rc + 3 * CH_ROWS * KMAX;                // [3][KMAX][CH_ROWS]   ... class-major
    float* red = (float*)(dl_t + 3 * KMAX * CH_ROWS);         // [3 + KMAX][CH_ROWS]  per-row loss terms and dlogits (fp32)
    float* lpart = (float*)oimg;                              // [8 waves][CH_ROWS][KMAX]: dead before the dpre image is written
    const int lane = t & 63, lc = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int kind = h.seg_kind[seg];
    const int blk = seg * nrb + rb;

    if (!(a.ablate & CH_ABL_COPY)) flush_copy(sm, rows_valid, t);      // the feature image -> HBM (no DMA wait follows inside the head)
    // ---- 1. W6: thread <-> feature ----
    if (t < CH_PW) {
        const f32x4 w0 = hi.w0, w1 = hi.w1;
#pragma unroll
        for (int c = 0; c < KMAX; ++c) {
            const float wv = (t < h.feat_valid && c < h.classes) ? (c < 4 ? w0[c & 3] : w1[c & 3]) : 0.f;
            __bf16 p0, p1, p2;
            split3(wv, p0, p1, p2);
            w6t[(0 * KMAX + c) * CH_PW + t] = p0; w6t[(1 * KMAX + c) * CH_PW + t] = p1; w6t[(2 * KMAX + c) * CH_PW + t] = p2;
        }
    }
    // B operand of product 4 (k = class, column = feature 32 wave + lc): the eight class weights of this lane's feature
    bf16x8 bw[1][3] = {{zero8(), zero8(), zero8()}};               // (one k-step: head_dpre_product<1>)
    {
        const int j = wave * 32 + lc;
        const f32x4 w0 = hi.bw0, w1 = hi.bw1;
#pragma unroll
        for (int c = 0; c < KMAX; ++c) {
            const float wv = (lh == 0 && j < h.feat_valid && c < h.classes) ? (c < 4 ? w0[c & 3] : w1[c & 3]) : 0.f;      // lh = 1: k = 8 .. 15, zeros
            __bf16 p0, p1, p2;
            split3(wv, p0, p1, p2);
            bw[0][0][c] = p0; bw[0][1][c] = p1; bw[0][2][c] = p2;
        }
    }
    lds_barrier();

    // ---- 2. logits: this wave's 32 features of the reduction ----
    {
        f32x16 acc[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int kg = 2 * wave + u;                      // k-step: features 16 kg .. 16 kg + 15
            if (16 * kg < h.feat) {                           // (wave-uniform)
                bf16x8 fb[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    fb[p] = *(const bf16x8*)(w6t + (p * KMAX + (lc & (KMAX - 1))) * CH_PW + 16 * kg + 8 * lh);
                    if (lc >= KMAX) fb[p] = zero8();          // columns 8 .. 31 of the product are padding
                }
                head_logits_step(acc, fimg, kg, fb, lc, lh);
            }
        }
        head_logits_scatter(acc, lpart, wave, lc, lh);
    }
    lds_barrier();

    // ---- 3. per row (wave 0: lane <-> row): losses, error, dlogits ----
    const long hoff = chain_moff<GROUP>(h.model_stride);      // model groups: this model's partial rows, loss partials and dpre
    float* part_row = chain_model(h.part, hoff) + (long)blk * h.part_stride;
    if (wave == 0) {
        const int r = lane;
        float l[KMAX];
        head_logits_gather(lpart, r, l);
        float b[KMAX], loss0, loss1, err, dl[KMAX];
#pragma unroll
        for (int c = 0; c < KMAX; ++c) b[c] = c < 4 ? hi.b0[c & 3] : hi.b1[c & 3];
        head_row<false>(l, b, kind, hi.label, h.classes, h.inv_count, h.unl_weight, r < rows_valid, loss0, loss1, err, dl);
        head_rows_to_lds(dl, loss0, loss1, err, r, dl_rc, dl_t, red);
    }
    lds_barrier();

    // ---- 4. dL/d(pre5) = (dlogits W6^T) * relu'(pre5) for columns 32 wave .. + 31: the next product's A image ----
    {
        f32x16 acc[2];
        bf16x8 da[1][2][3];
        head_load_dl_rows(dl_rc, lc, lh, da[0]);
        head_dpre_product<1>(acc, da, bw);
        const int cip = wave * 32 + lc;
        float s1 = head_dpre_to_image(acc, mw[0], oimg, cip, lh);
        s1 += __shfl_xor(s1, 32, 64);
        if (lh == 0 && cip < h.feat) part_row[h.off_dbf + cip] = s1;       // bias gradient of the feature layer
    }
    // ---- 5. dW6^T [class][feature] = dlogits^T F, features 32 wave .. + 31 ----
    {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < CH_ROWS / 16; ++ks) {
            bf16x8 fa[3];
            head_load_dl_cols(dl_t, ks, lc, lh, fa);
            head_dw6t_step(acc, fimg, ks, fa, wave, lane);
        }
        const int j = wave * 32 + lc;                         // registers 0 .. 3 = classes 4 lh .. 4 lh + 3 of feature j
        if (j < h.feat) *(f32x4*)(part_row + (long)j * KMAX + 4 * lh) = (f32x4){acc[0], acc[1], acc[2], acc[3]};
    }
    head_block_sums(red, h, blk, part_row, wave, lane, hoff);
    lds_barrier();
    // dL/d(pre5): the next product's A image is complete; its copy for the weight-gradient launch leaves at the end of that
    // product's k-loop
    sm.cp_img = oimg; sm.cp_out = (__bf16*)chain_model_opt(h.dpre, hoff) + (long)seg * h.dpre_bs + (long)row_blk * h.ldd;
    sm.cp_ldo = h.ldd; sm.cp_col0 = 0; sm.cp_ncols = h.feat;
}

// ------------------------------------------------------------------------------------------------------------------
// feature-matching gradient as the first A image (mr_gan.py:152-154): dL/d(pre5) = relu-mask ? 2/(J B) (m_gen - m_real) : 0
// ------------------------------------------------------------------------------------------------------------------
template <int ROWS, bool GROUP>
__device__ __forceinline__ void chain_fmgrad(const ChainArgs& a, char* lds, int rb, int row_blk, int rows_valid, int t, Stamps& st) {
    const FmArgs& f = a.fm;
    const long moff = chain_moff<GROUP>(a.model_stride);      // model groups: this model's features, moments and loss scalars
    const __bf16* const fm_feat = chain_model(a.fm_feat, moff);
    const float* const cs = chain_model(f.cs, moff);
    // the stored features of this block's rows (their sign is relu'(pre5), used at the end): requested first, so that their round
    // trip runs beside the fold of the partial sums instead of behind it
    constexpr int NCH = ROWS * CH_PW / 8 / CH_THREADS;
    bf16x8 fv[NCH];
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const int q = t + CH_THREADS * u, r = q >> 5, c0 = (q & 31) * 8;
        const bool ok = r < rows_valid && c0 < f.feat;
        fv[u] = *(const bf16x8*)(fm_feat + (long)(row_blk + (ok ? r : 0)) * a.fm_ldf + (ok ? c0 : 0));
    }
    float* gj = (float*)(lds + chain_img(ROWS, 1));          // 9 KiB in the first product's output image: idle until its epilogue (both ring stages are in flight)
    float* scr = gj + CH_PW;                                  // [8][256]
    const float* cs_real = cs + (long)f.npart_fake * f.ldcs;
    // fold the per-row-block partial sums: thread <-> (4 columns, every 8th partial row), 64 partial rows of both streams per
    // round trip (16 loads of 16 bytes in flight per thread), then an 8-way combine through LDS
    {
        const int cq = (t & 63) * 4, pg = t >> 6;
        f32x4 u = {0.f, 0.f, 0.f, 0.f};
        if (cq < f.feat) {
            // unconditional loads from clamped rows, zero weight beyond the end: a load under a runtime condition makes
            // hipcc branch around it and wait for each one (16 serialized round trips, ~30 k cycles measured here); and a
            // remainder loop `for (p = pg + 64; p < npart; p += 8) u += load` is one round trip per iteration (the 32-row
            // blocks of the G sub-step leave 128 partial rows per stream: 16 of them, 20 k cycles of a 43 k-cycle launch)
            const int nmax = max(f.npart_fake, f.npart_real);
            for (int base = 0; base < nmax; base += 64) {
                f32x4 vf[8], vr[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) vf[i] = *(const f32x4*)(cs + (long)min(base + pg + 8 * i, f.npart_fake - 1) * f.ldcs + cq);
#pragma unroll
                for (int i = 0; i < 8; ++i) vr[i] = *(const f32x4*)(cs_real + (long)min(base + pg + 8 * i, f.npart_real - 1) * f.ldcs + cq);
#pragma unroll
                for (int i = 0; i < 8; ++i) u += vf[i] * ((base + pg + 8 * i < f.npart_fake) ? 1.0f : 0.0f);
#pragma unroll
                for (int i = 0; i < 8; ++i) u -= vr[i] * ((base + pg + 8 * i < f.npart_real) ? 1.0f : 0.0f);
            }
        }
        *(f32x4*)(scr + pg * 256 + cq) = u;                   // scr: [8][256]
    }
    __syncthreads();
    CH_STAMP(1);
    const int c = t & 255, hf = t >> 8;
    float sq = 0.f;
    if (hf == 0) {
        float sd = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) sd += scr[g * 256 + c];
        const float diff = (c < f.feat_valid) ? sd / f.count : 0.f;
        gj[c] = f.grad_scale * 2.0f / ((float)f.feat_valid * f.count) * diff;
        sq = diff * diff;
    }
    if (rb == 0 && blockIdx.x == 0) {                         // the loss scalar, once (per model)
        sq = wave_sum(sq);
        __syncthreads();
        if ((t & 63) == 0) scr[t >> 6] = sq;
        __syncthreads();
        if (t == 0) {
            const float loss = (scr[0] + scr[1] + scr[2] + scr[3]) / (float)f.feat_valid;
            if (f.loss_out) *chain_model(f.loss_out, moff) = loss;      // (tested non-null: the plain offset)
            if (f.accum) *chain_model(f.accum, moff) += loss;
        }
    }
    __syncthreads();
    CH_STAMP(2);
    char* img = lds + chain_img(ROWS, 0);
    // thread <-> (row, 8 columns): one 16-byte chunk of the image.  relu'(pre5) comes from the stored features of the
    // generated rows (f > 0 <=> pre5 > 0; bf16 keeps every positive value positive): one unconditional 16-byte load per chunk
    // from a clamped row, all four in flight together.  (Decoding the lane-native mask words here instead costs 8 scattered
    // loads per chunk: ~18 k cycles per block, measured.)
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const int q = t + CH_THREADS * u, r = q >> 5, cch = q & 31, c0 = cch * 8;
        const bool ok = r < rows_valid && c0 < f.feat;
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (__bf16)((ok && (float)fv[u][i] > 0.f) ? gj[c0 + i] : 0.f);
        *(bf16x8*)(img + (cch >> 3) * (ROWS * 128) + kc_off(r, cch & 7)) = v;
    }
    __syncthreads();
    CH_STAMP(6);
    CH_STAMP(7);        // (the image's copy to HBM is deferred to the end of the first product's k-loop: see Stream)
}

// one dense product of the chain on the block's rows.  MODE and J, the product's place in its run of three (which decides its
// images: chain.h), are compile-time; `bias` (forward) and `mw` (the relu-mask words
// of the output tile: read by dX, returned by forward) live in registers, loaded or produced before this call.
// GAUSS: forward noise from the true-Gaussian generator (common.h: gauss_block; rowhash[] then holds row-pair hashes)
template <int MODE, int J, int MI, bool GAUSS, bool GROUP>
__device__ __forceinline__ void chain_gemm(const ChainArgs& a, const ChainOp& op, const __bf16* nextW, const int nextK, const int nextN,
                                           char* lds, Stream& sm, const float bias,
                                           uint32_t (&mw)[2][MI], const int seg, const int nrb, const int rb, const int row_blk,
                                           const int rows_valid, const uint32_t iter, const i32x4 hfrag, const int t, Stamps& st) {
    const int lane = t & 63, lc = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr bool fwd = MODE == CH_FWD_RELU;
    constexpr int ROWS = 32 * MI, NS = chain_stages(ROWS), a_off = chain_img(ROWS, J), o_off = chain_img(ROWS, J + 1);
    const int K = op.K, N = op.N;
    const int npass = (N + CH_PW - 1) / CH_PW, nk = K / 64;
    const bool noisy = fwd && op.sigma > 0.f;
    uint32_t rowhash[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) rowhash[mi] = 0u;
    if (noisy) {
        const uint32_t nkey = noise_key(a.seed + (uint64_t)chain_model_index<GROUP>(), op.site * 256u + (uint32_t)(a.seg0 + seg), iter);      // (model m: seed + m)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            if constexpr (GAUSS) rowhash[mi] = gauss_pairhash(nkey, a.row0 + (uint32_t)(row_blk + mi * 32), lane);
            else rowhash[mi] = noise_rowhash(nkey, a.row0 + (uint32_t)(row_blk + mi * 32 + lc));
        }
    }
    uint16_t* mask = op.mask ? op.mask + (long)seg * op.mask_bs : nullptr;
    BTile bt;
    btile_setup(bt, op.W, K, N, wave, lane);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass >= npass) break;
        const int col = pass * CH_PW + wave * 32 + lc;
        const bool colin = col < N, colvalid = col < op.n_valid;
        f32x16 acc[MI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
        CH_STAMP(1);               // pass setup
        for (int kt = 0; kt < nk; ++kt) {
            // No workgroup barrier inside the k-loop: a wave reads only ITS OWN 32 columns of a weight tile, and those are
            // exactly the pieces it loads itself (issue_btile), so its own counted vmcnt orders the LDS-DMA before its reads;
            // the stage refilled below was last read by this wave during tile gtile - 1, whose fragments its MFMAs have
            // already consumed.  The A image is read-only for the whole product (completed behind the barrier that ended the
            // previous product / the prologue).  The waves of a block drift apart inside a product -- one wave's MFMAs beside
            // another's epilogue -- and meet again at the image barrier that ends the pass.
            // Two tiles of the flat sequence are in flight while tile gtile is consumed (at one tile the wait below was the L2 round
            // trip of every tile).  With the 3-stage ring (32-row blocks) tile gtile + 2 is issued before the reads of tile gtile;
            // with the 2-stage ring (64-row blocks: the images leave 64 KiB) it goes into tile gtile's OWN stage as soon as this wave
            // has the tile's four B fragments in registers.  vmcnt counts in issue order: all but the youngest 4 operations done =
            // tile gtile has landed (stores issued since then only make the wait stricter).
            // (sm.inflight tiles are issued and not yet consumed, tile gtile the oldest of them: at the tail of the last product no
            //  younger tile exists and the wait must cover everything)
            if (!(a.ablate & CH_ABL_STREAM)) {
                if (sm.inflight > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            --sm.inflight;
            CH_STAMP(3);                                   // wait for the weight tile
            auto issue_ahead = [&](char* stage) {
                const int kk = kt + 2;                     // (every product of a chain has at least 2 k-tiles: launch_chain)
                if (kk < nk) { issue_btile(bt, pass, kk, stage, wave); ++sm.inflight; }
                else if (pass + 1 < npass) { issue_btile(bt, pass + 1, kk - nk, stage, wave); ++sm.inflight; }
                else if (nextW) { BTile nb; btile_setup(nb, nextW, nextK, nextN, wave, lane); issue_btile(nb, 0, kk - nk, stage, wave); ++sm.inflight; }
            };
            const char* As = lds + a_off + kt * (ROWS * 128);
            char* Bs = lds + chain_ring(ROWS) + (sm.gtile % NS) * CH_STAGE_BYTES;
            if constexpr (NS == 3) { if (!(a.ablate & CH_ABL_STREAM)) issue_ahead(lds + chain_ring(ROWS) + ((sm.gtile + 2) % NS) * CH_STAGE_BYTES); }
            ++sm.gtile;
            if (a.ablate & CH_ABL_MFMA) { if constexpr (NS == 2) { if (!(a.ablate & CH_ABL_STREAM)) issue_ahead(Bs); } continue; }
            // fragments of two k-steps per batch: their LDS latency is paid once per batch (the other wave of the SIMD
            // covers the rest); a deeper batch costs registers the epilogue needs
            if constexpr (NS == 3) {
#pragma unroll
                for (int kg = 0; kg < 4; kg += 2) {
                    bf16x8 fa[2][MI], fb[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi) fa[ks][mi] = *(const bf16x8*)(As + kc_off(mi * 32 + lc, (kg + ks) * 2 + lh));
                        fb[ks] = *(const bf16x8*)(Bs + kc_off(wave * 32 + lc, (kg + ks) * 2 + lh));
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][mi], fb[ks], acc[mi], 0, 0, 0);
                }
            } else {
                // (named registers, not an array: hipcc puts an array it indexes in a loop into scratch memory)
                const bf16x8 fb0 = *(const bf16x8*)(Bs + kc_off(wave * 32 + lc, 0 + lh)), fb1 = *(const bf16x8*)(Bs + kc_off(wave * 32 + lc, 2 + lh));
                const bf16x8 fb2 = *(const bf16x8*)(Bs + kc_off(wave * 32 + lc, 4 + lh)), fb3 = *(const bf16x8*)(Bs + kc_off(wave * 32 + lc, 6 + lh));
                bf16x8 fa0[MI], fa1[MI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    fa0[mi] = *(const bf16x8*)(As + kc_off(mi * 32 + lc, 0 + lh));
                    fa1[mi] = *(const bf16x8*)(As + kc_off(mi * 32 + lc, 2 + lh));
                }
                // the stage may be refilled once its fragments are in registers (the LDS-DMA write must not overtake the reads)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (!(a.ablate & CH_ABL_STREAM)) issue_ahead(Bs);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0[mi], fb0, acc[mi], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1[mi], fb1, acc[mi], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    fa0[mi] = *(const bf16x8*)(As + kc_off(mi * 32 + lc, 4 + lh));
                    fa1[mi] = *(const bf16x8*)(As + kc_off(mi * 32 + lc, 6 + lh));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0[mi], fb2, acc[mi], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1[mi], fb3, acc[mi], 0, 0, 0);
            }
            CH_STAMP(5);                                   // tile issue + fragment reads + MFMAs
        }

        if (!(a.ablate & CH_ABL_COPY)) flush_copy<ROWS>(sm, rows_valid, t);      // the previous pass's image -> HBM (see Stream)
        // every pass of a product assembles its 256 columns in the SAME image: a second pass may only overwrite them when every
        // wave has copied the first pass's out (the only such product, dX through D3, ends the chain)
        if (pass > 0) lds_barrier();
        // ---- epilogue: bias / relu / mask / noise, bf16 into the output image, column sums ----
        char* oimg = lds + o_off;
        const int cip = wave * 32 + lc;                    // column inside the pass = column of the output image
        int obase[4];
        img_col_bases<ROWS>(obase, cip, lh);
        const float sig = (noisy && colvalid) ? (GAUSS ? op.sigma : op.sigma * NOISE_SCALE) : 0.f;
        float s1 = 0.f;
        auto ostore = [&](int mi, int r, float o) {
#ifdef MRGAN_CH_NO_OSTORE       // timing experiment (compile-time: a run-time test per element perturbs the epilogue it measures)
            asm volatile("" :: "v"(o)); return;
#endif
            *(__bf16*)(oimg + img_elem_off(obase, mi, r)) = (__bf16)o;
        };
        if (a.ablate & CH_ABL_EPI) {
            if (acc[0][0] == 12345.678f) ostore(0, 0, s1);
        } else if constexpr (fwd) {
            const float bv = colvalid ? bias : 0.f;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                i32x16 nzs = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                f32x16 nzg = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if constexpr (GAUSS) { if (noisy) nzg = gauss_block(rowhash[mi], (uint32_t)col, lane); }
                else if (noisy) nzs = noise_block(rowhash[mi], (uint32_t)col >> 5, lane, hfrag);
                uint32_t mbits = 0u;
                // Rows >= rows_valid of a ragged block carry relu(bias) + noise instead of zeros.  That is harmless: every
                // product is row-local, copy_out never stores those rows, the head gives them zero dlogits -- only a
                // column sum must leave them out (below).  Masking them here would cost a compare per element, whose 32
                // lane masks hipcc keeps in SGPR pairs for the whole kernel (250 spilled SGPRs, ~2 k cycles per pass).
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = fmaxf(acc[mi][r] + bv, 0.f);
                    mbits |= min(__builtin_bit_cast(uint32_t, v), 1u) << r;
                    s1 += v;
                    acc[mi][r] = v;
                    if constexpr (GAUSS) ostore(mi, r, fmaf(sig, nzg[r], v));
                    else ostore(mi, r, fmaf(sig, (float)nzs[r], v));       // sig = 0 without noise
                }
                mw[pass][mi] = mbits;
                if (mask && colin && row_blk + mi * 32 < a.rows)
                    mask[((long)((row_blk + mi * 32) >> 5) * op.ldm + col) * 2 + lh] = (uint16_t)mbits;
            }
        } else {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // rows >= rows_valid and padding columns arrive as exact zeros (zero A rows / zero weights).
                    // (a select, not a bit-AND on the accumulator element: hipcc 7.2 mis-folds that form)
                    const float av = acc[mi][r];
                    const float v = ((mw[pass][mi] >> r) & 1u) ? av : 0.f;
                    s1 += v;
                    ostore(mi, r, v);
                }
            }
        }
        if (op.cs) {
            if (fwd && rows_valid < ROWS) {                 // ragged block: the column sum again, without the padding rows
                s1 = 0.f;
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s1 += (mi * 32 + acc_row(r, lh) < rows_valid) ? acc[mi][r] : 0.f;
            }
            s1 += __shfl_xor(s1, 32, 64);
            if (lh == 0 && col < op.ldcs) op.cs[((long)seg * nrb + rb) * op.ldcs + col] = s1;
        }
        CH_STAMP(6);                                       // epilogue math + image writes
        lds_barrier();                                     // the output image is complete
        if (op.out) {                                      // this pass's columns: copied out at the end of the next k-loop
            sm.cp_img = oimg; sm.cp_out = op.out + (long)seg * op.out_bs + (long)row_blk * op.ldo;
            sm.cp_ldo = op.ldo; sm.cp_col0 = pass * CH_PW; sm.cp_ncols = N;
        }
        CH_STAMP(7);                                       // image barrier + copy-out issue
    }
}

// relu-mask words of a dX product's output tile, from HBM (written by an earlier launch)
template <int MI, bool GROUP>
__device__ __forceinline__ void load_mask_words(const ChainArgs& a, const ChainOp& op, uint32_t (&mw)[2][MI], int seg, int row_blk, int wave, int lc, int lh) {
    const uint16_t* mask = chain_model(op.mask, chain_moff<GROUP>(a.model_stride)) + (long)seg * op.mask_bs;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int col = pass * CH_PW + wave * 32 + lc;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            // branch-free (see chain_fmgrad): clamped address, result zeroed when out of range
            const bool ok = col < op.N && row_blk + mi * 32 < a.rows;
            const uint32_t w = mask[((long)((ok ? row_blk + mi * 32 : 0) >> 5) * op.ldm + (ok ? col : 0)) * 2 + lh];
            mw[pass][mi] = ok ? w : 0u;
        }
    }
}

// VARIANT: the three chains of one training step (chain.h).  The list of products is fixed per variant, so the loop over products is
// unrolled at compile time: epilogue inputs are loaded once at the top (before the weight stream loads the memory
// pipeline), relu masks of products whose forward ran in this launch never leave registers, and no per-op descriptor
// reload sits between two products.
// MI: 32-row groups per block (2: 64 rows, the D sub-step's launch; 1: 32 rows, for launches that would leave most CUs idle)
// GAUSS: the forward products draw their layer noise from the true-Gaussian generator (ChainArgs::gauss; never with CH_V_GBWD)
// GROUP: the launch covers the models of a group handle, grid.y = models (chain.h: chain_moff); false: the single handle's kernel
template <int VARIANT, int MI, bool GAUSS = false, bool GROUP = false>
__global__ __launch_bounds__(CH_THREADS) void chain_kernel(const ChainArgs a) {
    constexpr int ROWS = 32 * MI;
    static_assert(VARIANT != CH_V_DTAIL || MI == 2, "the loss head works on 64-row blocks");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int t = threadIdx.x, lane = t & 63, lc = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nrb = (a.rows + ROWS - 1) / ROWS;
    const int seg = blockIdx.x / nrb, rb = blockIdx.x - seg * nrb;
    const int row_blk = rb * ROWS, rows_valid = min(ROWS, a.rows - row_blk);
    const long moff = chain_moff<GROUP>(a.model_stride);      // model groups (ChainArgs::models): bytes to this model's tensors

    Stamps st;
    st.start();
    // Keras iteration of this sub-step (noise key): loaded before the weight stream starts and pinned in an SGPR -- sunk to its
    // first use, the load would sit behind a vmcnt(0) that also drains the weight-tile DMA
    uint32_t iter = a.st ? __builtin_amdgcn_readfirstlane((int)a.st->iter) : 0u;
    asm volatile("" : "+s"(iter));
    // ---- epilogue inputs of every product: biases (forward) and the relu masks that come from HBM ----
    const int col0 = wave * 32 + lc;
    float bias[3] = {0.f, 0.f, 0.f};
    uint32_t mwA[2][MI], mwB[2][MI], mwC[2][MI];
#pragma unroll
    for (int p_ = 0; p_ < 2; ++p_)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) { mwA[p_][mi] = 0u; mwB[p_][mi] = 0u; mwC[p_][mi] = 0u; }
    if constexpr (VARIANT != CH_V_GBWD) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { const float bv = chain_model(a.fwd[i].bias, moff)[min(col0, a.fwd[i].n_valid - 1)]; bias[i] = col0 < a.fwd[i].n_valid ? bv : 0.f; }
    }
    if constexpr (VARIANT == CH_V_DTAIL) load_mask_words<MI, GROUP>(a, a.dx[2], mwC, seg, row_blk, wave, lc, lh);      // dX through D3 needs D2's mask
    HeadInputs hin;
    if constexpr (VARIANT == CH_V_DTAIL) head_prefetch<GROUP>(a, hin, seg, row_blk, rows_valid, t);
    if constexpr (VARIANT == CH_V_GBWD) {
        load_mask_words<MI, GROUP>(a, a.dx[0], mwA, seg, row_blk, wave, lc, lh);
        load_mask_words<MI, GROUP>(a, a.dx[1], mwB, seg, row_blk, wave, lc, lh);
        load_mask_words<MI, GROUP>(a, a.dx[2], mwC, seg, row_blk, wave, lc, lh);
    }

    // ---- first A image ----
    constexpr int a0_off = chain_img(ROWS, 0);
    if constexpr (VARIANT != CH_V_GBWD) {
        const __bf16* src = chain_model(a.a, moff) + (long)seg * a.a_bs;
        const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)((long)a.rows * a.lda * 2), 0x00020000);
        const int lrow = lane >> 3, lp = lane & 7, nkt = a.a_cols / 64;
        // ROWS / 8 pieces of [8 rows][128 B] per k-tile, spread over the waves: rows >= a.rows arrive as zeros
        constexpr int PPT = ROWS / 8;
        for (int pce = wave; pce < nkt * PPT; pce += CH_THREADS / 64) {
            const int kt = pce / PPT, pr = pce - kt * PPT, R = pr * 8 + lrow;
            const int voff = (int)(((long)(row_blk + R) * a.lda + ((lp ^ ((R >> 1) & 7)) << 3)) * 2);
            glds16(rsA, lds + a0_off + kt * (ROWS * 128) + pr * 1024, voff, kt * 128);
        }
    }
    // ---- the weight-tile stream (per wave: its own 32 columns of every tile) ----
    Stream sm;
    constexpr int AHEAD = 2;       // tiles in flight (see chain_gemm)
    sm.gtile = 0; sm.cp_img = nullptr; sm.inflight = AHEAD;
    {
        const ChainOp& first = VARIANT == CH_V_GBWD ? a.dx[0] : a.fwd[0];
        BTile b0;
        btile_setup(b0, chain_model(first.W, moff), first.K, first.N, wave, lane);
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) issue_btile(b0, 0, i, lds + chain_ring(ROWS) + i * CH_STAGE_BYTES, wave);
    }
    if constexpr (VARIANT != CH_V_GBWD) {
        wait_vm(4 * AHEAD);        // this wave's pieces of the A image have landed (the weight-tile pieces are younger) ...
        __builtin_amdgcn_s_barrier();      // ... everyone's: the k-loops below run without workgroup barriers
        asm volatile("" ::: "memory");
    } else {
        chain_fmgrad<ROWS, GROUP>(a, lds, rb, row_blk, rows_valid, t, st);      // (ends with a workgroup barrier)
        sm.cp_img = lds + a0_off; sm.cp_out = (__bf16*)chain_model_opt(a.fm.dpre, moff) + (long)row_blk * a.fm.ldd;
        sm.cp_ldo = a.fm.ldd; sm.cp_col0 = 0; sm.cp_ncols = a.fm.feat;
    }
    CH_STAMP(0);                   // prologue (epilogue inputs, first tile issue, A image)

    const i32x4 hfrag = hadamard_frag(lane);
    // the product's index goes through an opaque asm so that the descriptor's scalar loads happen at the product's start: hoisted to
    // the top of the kernel (what hipcc does with a constant index) seven descriptors overflow the SGPR file and every
    // pass pays ~2 k cycles of spill traffic
    auto opq = [](int i) { asm volatile("" : "+s"(i)); return i; };
    // ... and the descriptor is copied as a whole (wide scalar loads, one wait) instead of field by field at the points of use
    // OPS[J]: the product (fwd or dx: its direction); NOPS[NEXT]: the product that follows (NEXT = -1: none) -- its first weight
    // tile is issued during this product's last k-tile
    // (model groups: the copy's pointers move to this model's tensors -- scalar adds on the descriptor, null stays null)
#define CH_GEMM(OPS, J, NOPS, NEXT, BIAS, MW) do { ChainOp op_ = a.OPS[opq(J)];                                                          \
        op_.W = chain_model(op_.W, moff); op_.out = chain_model_opt(op_.out, moff);                                                        \
        op_.mask = chain_model_opt(op_.mask, moff); op_.cs = chain_model_opt(op_.cs, moff);                                                    \
        const int nx_ = opq(NEXT < 0 ? 0 : NEXT);                                                                                      \
        chain_gemm<CH_GEMM_MODE_##OPS, J, MI, GAUSS, GROUP>(a, op_, NEXT < 0 ? nullptr : chain_model(a.NOPS[nx_].W, moff), a.NOPS[nx_].K, a.NOPS[nx_].N, lds, sm, BIAS, MW,   \
                         seg, nrb, rb, row_blk, rows_valid, iter, hfrag, t, st); } while (0)
    constexpr int CH_GEMM_MODE_fwd = CH_FWD_RELU, CH_GEMM_MODE_dx = CH_DX_RELU;
    if constexpr (VARIANT == CH_V_DTAIL) {
        // D3 D4 D5 forward: the masks of D3 / D4 stay in registers for the way back
        uint32_t mw4[2][MI];
        CH_GEMM(fwd, 0, fwd, 1, bias[0], mwB);
        CH_GEMM(fwd, 1, fwd, 2, bias[1], mwA);
        CH_GEMM(fwd, 2, dx, 0, bias[2], mw4);
        CH_STAMP(1);               // (the feature image is complete: chain_gemm ended with the image barrier; the weight tile in
                                   //  flight lands in the ring, which the head does not touch)
        if constexpr (MI == 2) { if (!(a.ablate & CH_ABL_HEAD)) chain_head<GROUP>(a, lds, sm, hin, mw4, seg, rb, nrb, row_blk, rows_valid, t); }
        CH_STAMP(2);               // loss head
        CH_GEMM(dx, 0, dx, 1, 0.f, mwA);       // dX through D5 * relu'(D4)
        CH_GEMM(dx, 1, dx, 2, 0.f, mwB);       // dX through D4 * relu'(D3)
        CH_GEMM(dx, 2, dx, -1, 0.f, mwC);      // dX through D3 * relu'(D2)
    } else if constexpr (VARIANT == CH_V_GFWD) {
        uint32_t mwx[2][MI];
        CH_GEMM(fwd, 0, fwd, 1, bias[0], mwx);
        CH_GEMM(fwd, 1, fwd, 2, bias[1], mwx);
        CH_GEMM(fwd, 2, fwd, -1, bias[2], mwx);
    } else {
        CH_GEMM(dx, 0, dx, 1, 0.f, mwA);
        CH_GEMM(dx, 1, dx, 2, 0.f, mwB);
        CH_GEMM(dx, 2, dx, -1, 0.f, mwC);
    }
#undef CH_GEMM
    if (!(a.ablate & CH_ABL_COPY)) flush_copy<ROWS>(sm, rows_valid, t);      // the last image
    if (t == 0) st.store(a.stamps);
}

}  // namespace

// every instantiation of chain_kernel: launch_chain picks its kernel here, chain_init_attributes raises the LDS limit of each
struct ChainKernel { int variant, block_rows, gauss, group; void (*kernel)(const ChainArgs); };
#define CH_K(V, MI, G) {V, 32 * MI, G, 0, chain_kernel<V, MI, G != 0, false>}, {V, 32 * MI, G, 1, chain_kernel<V, MI, G != 0, true>}
static const ChainKernel chain_kernels[] = {
    CH_K(CH_V_DTAIL, 2, 0), CH_K(CH_V_GFWD, 2, 0), CH_K(CH_V_GBWD, 2, 0), CH_K(CH_V_GFWD, 1, 0), CH_K(CH_V_GBWD, 1, 0),
    CH_K(CH_V_DTAIL, 2, 1), CH_K(CH_V_GFWD, 2, 1), CH_K(CH_V_GFWD, 1, 1),
};
#undef CH_K

int chain_init_attributes() {
    for (const ChainKernel& k : chain_kernels)
        if (hipFuncSetAttribute((const void*)k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, chain_lds_bytes(k.block_rows)) != hipSuccess) return -2;
    return 0;
}

// one product's shape limits; fwd: a forward product (its output is the next product's A image), else a dX product
static bool chain_op_ok(const ChainOp& op, bool fwd) {
    if ((op.K % 64) || (op.N % 64) || op.K > CH_KMAX || op.K < 128 || op.N < 64 || op.N > 2 * CH_PW || !op.W) return false;
    // (the bias of a forward product is read at min(column, n_valid - 1): the kernel's prologue)
    if (fwd ? (op.N > CH_PW || !op.bias || op.n_valid < 1 || op.n_valid > op.N) : !op.mask) return false;
    return (long)op.N * op.K * 2 < (1L << 31);
}

// the instantiation a launch runs: (the 32-row blocks have no D-tail kernel; the dX products draw no noise, so CH_V_GBWD has one
// kernel for both generators)
static const ChainKernel* chain_pick(const ChainArgs& a) {
    const int gauss = a.variant != CH_V_GBWD && a.gauss, group = a.models > 1;
    for (const ChainKernel& c : chain_kernels)
        if (c.variant == a.variant && c.block_rows == a.block_rows && c.gauss == gauss && c.group == group) return &c;
    return nullptr;
}

bool chain_kernel_name(const ChainArgs& a, char* name, int len) {
    const ChainKernel* k = chain_pick(a);
    if (k && name && len > 0) snprintf(name, (size_t)len, "chain_kernel<%d, %d, %d, %d>", k->variant, k->block_rows / 32, k->gauss, k->group);
    return k != nullptr;
}

// Everything launch_chain refuses (-3), as a pure host function: no HIP call, so a refused descriptor never reaches the device.
// Beside each product's own limits (chain_op_ok) the products of a run must fit each other, because the kernel compiles in
// which LDS image holds what (chain.h) and takes every width from the descriptors:
bool chain_args_ok(const ChainArgs& a) {
    const bool has_fwd = a.variant != CH_V_GBWD, has_dx = a.variant != CH_V_GFWD;
    // block_rows is 32 or 64, and 64 for the D tail: the table holds nothing else
    if (!chain_pick(a)) return false;
    if (a.rows < 1 || a.nseg < 1) return false;
    for (int i = 0; i < 3; ++i)
        if ((has_fwd && !chain_op_ok(a.fwd[i], true)) || (has_dx && !chain_op_ok(a.dx[i], false))) return false;
    if (has_fwd) {
        if (!a.a || (a.a_cols % 64) || a.a_cols > CH_KMAX || a.a_cols != a.fwd[0].K || (long)a.rows * a.lda * 2 >= (1L << 31)) return false;
        // chain_gemm reads nk = K / 64 k-tiles of the image the previous epilogue wrote N columns of (`As = lds + a_off + kt * ...`)
        if (a.fwd[0].N != a.fwd[1].K || a.fwd[1].N != a.fwd[2].K) return false;
    }
    if (has_dx) {
        if (a.dx[0].N != a.dx[1].K || a.dx[1].N != a.dx[2].K) return false;      // the same hand-over, on the way back
        // every pass of a product lands in columns 0 .. 255 of ONE image (chain_gemm: `cip`, not `col`, addresses oimg): the
        // product after a two-pass one would read the second pass only, and image 1 holds CH_PW columns
        if (a.dx[0].N > CH_PW || a.dx[1].N > CH_PW) return false;
    }
    if (a.variant == CH_V_DTAIL) {
        const HeadArgs& h = a.head;
        // the head inside the D-tail chain is an 8-class kernel (its scratch is half of image 0) ...
        if (h.classes < 1 || h.classes > KMAX || h.ldw != KMAX) return false;
        if (a.nseg > 3) return false;                                             // HeadArgs::seg_kind[3], indexed by the block's segment
        // ... that reads `feat` columns of the feature image fwd[2] wrote (chain_head 2.) and writes dL/d(pre5) into the lower
        // 256 columns of image 0, whose upper half is its scratch (chain_head_scratch): dx[0] may read no k-tile beyond them
        if (h.feat != a.fwd[2].N || a.dx[0].K != h.feat || h.feat > CH_PW || h.feat_valid < 1 || h.feat_valid > h.feat) return false;
        // (every one of these is dereferenced or stored through without a test: head_prefetch, chain_head 3. .. 5., head_block_sums)
        if (!h.w || !h.b || !h.part || !h.loss_part || !h.dpre) return false;
        for (int i = 0; i < a.nseg; ++i) {
            if (h.seg_kind[i] < HEAD_LAB || h.seg_kind[i] > HEAD_FAKE) return false;      // head_row<false>: the training kinds
            if (h.seg_kind[i] == HEAD_LAB && !h.labels) return false;
        }
    }
    if (a.variant == CH_V_GBWD) {
        const FmArgs& f = a.fm;
        // chain_fmgrad builds 256 columns of image 0 (zeros from column `feat` on) and folds `feat` <= 256 columns of moments
        if (f.feat != a.dx[0].K || f.feat > CH_PW || f.feat_valid < 1 || f.feat_valid > f.feat) return false;
        if (!f.cs || !a.fm_feat || !f.dpre || f.npart_fake < 1 || f.npart_real < 1) return false;      // (the copy of image 0 goes to dpre untested)
    }
    return true;
}

int launch_chain(const ChainArgs& a, hipStream_t s) {
    if (!chain_args_ok(a)) return -3;
    const ChainKernel* k = chain_pick(a);
    const int nrb = (a.rows + a.block_rows - 1) / a.block_rows;
    MRGAN_LAUNCH(k->kernel, dim3(nrb * a.nseg, std::max(1, a.models)), dim3(CH_THREADS), chain_lds_bytes(a.block_rows), s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace mrgan
