// Non-GEMM kernels of the mr_gan training path: HBM-bound elementwise / reduction work.
// Access pattern everywhere: 16-byte loads/stores per lane along the contiguous (feature) dimension,
// 256-thread blocks laid out as 32 column-groups x 8 row-lanes, >= 128 blocks per launch.
#include "aux_kernels.h"
#include "head.h"

namespace mrgan {
namespace {

// 8 consecutive elements of T <-> 8 floats
template <typename T> __device__ __forceinline__ void load8(const T* p, float v[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float v[8]) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}
template <> __device__ __forceinline__ void load8<__bf16>(const __bf16* p, float v[8]) {
    const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float v[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float v[8]) {
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[4 + i]; }
    *(f32x4*)p = a; *(f32x4*)(p + 4) = b;
}
template <> __device__ __forceinline__ void store8<__bf16>(__bf16* p, const float v[8]) {
    bf16x8 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (__bf16)v[i];
    *(bf16x8*)p = a;
}

// =========================================================================================
// stage: gather rows (optionally by index) of the resident fp32 matrix, add GaussianNoise(sigma)
// (mr_gan.py:118), convert to T, zero the padding columns.  Also draws z when asked to.
// wave <-> 32 rows x 128 columns.  The noise generator (common.h) delivers a 32x32 block in the MFMA accumulator
// layout (lane = column, 16 rows in registers); the integer sums (|s| <= 4064) go through a per-wave int16 LDS image so
// that global loads and stores move 8 consecutive columns per lane (2 x 16 B in, 16 B out).
// =========================================================================================
// GAUSS (StageArgs::gauss): the true-Gaussian generator's floats go through a per-wave fp32 image of one 32 x 32 block at a
// time; the lanes whose 8 columns lie in that block add it.
template <typename T, bool GAUSS = false>
__global__ __launch_bounds__(256) void stage_kernel(const StageArgs a) {
    // int16 sums [4][32][128 + 8] (+8: rows 272 B apart, bank spread for the 2-byte writes), or (GAUSS) floats [4][32][32 + 4]
    __shared__ __attribute__((aligned(16))) char nraw[GAUSS ? 4 * 32 * (32 + 4) * 4 : 4 * 32 * (128 + 8) * 2];
    short (*nlds)[32][128 + 8] = (short (*)[32][128 + 8])nraw;
    float (*glds)[32][32 + 4] = (float (*)[32][32 + 4])nraw;
    const DevState st = *a.cur;
    const StageSeg& sg = a.s[blockIdx.z];
    // model groups (StageSeg::models): grid.y = model * ry + row block; a multiply instead of a division, and nothing the
    // segment's fields wait for
    const int model = (int)((blockIdx.y * a.ry_mul) >> 16), yblk = (int)blockIdx.y - model * a.ry;
    const uint64_t seed = a.seed + (uint64_t)model;
    const int lane = threadIdx.x & 63, lc = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rbase = (yblk * 4 + wave) * 32, cbase = (int)blockIdx.x * 128;
    if (rbase >= sg.rows || cbase >= sg.cols_pad) return;          // wave-uniform; no block-level barrier below
    const long o = sg.stream ? (long)st.batch * sg.rows : 0;
    T* out = (T*)((char*)sg.out + (long)model * sg.out_ms);
    const float* const xsrc = sg.src + (long)model * sg.src_ms;
    const int32_t* const xidx = sg.idx ? sg.idx + (long)model * sg.idx_ms : nullptr;
    const bool noisy = sg.gen || sg.sigma > 0.f;
    const float sigs = (sg.gen ? 1.0f : sg.sigma) * (GAUSS ? 1.0f : NOISE_SCALE);
    const int cg = (lane & 15) * 8, rl = lane >> 4;                // lane <-> (8 columns, every 4th row)
    const int col = cbase + cg;
    const bool vec_ok = !sg.gen && (sg.ld & 3) == 0 && ((uintptr_t)xsrc & 15) == 0 && col + 7 < sg.cols;
    // source rows first, then every row's loads in flight together (a dependent index -> row chain per iteration is
    // latency-bound: this kernel is 40 MB of traffic and must not take longer than a GEMM)
    long srow[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int row = rbase + it * 4 + rl;
        srow[it] = (!sg.gen && row < sg.rows) ? (xidx ? (long)xidx[o + row] : (o + row)) : 0;
    }
    float v[8][8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[it][c] = 0.f;
        const int row = rbase + it * 4 + rl;
        if (!sg.gen && row < sg.rows) {
            const float* src = xsrc + srow[it] * sg.ld + col;
            if (vec_ok) load8<float>(src, v[it]);
            else {
#pragma unroll
                for (int c = 0; c < 8; ++c) if (col + c < sg.cols) v[it][c] = src[c];
            }
        }
    }
    // the noise of the wave's 32 x 128 block is generated while the row loads above are in flight (it was generated first in
    // round 2, with nothing in flight)
    if constexpr (GAUSS) {
        if (noisy) {
            const uint32_t ph = gauss_pairhash(noise_key(seed, sg.site * 256u + sg.seg, st.iter + sg.iter_off), a.row0 + (uint32_t)rbase, lane);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int c0 = cbase + cb * 32;
                if (c0 >= sg.cols) break;                          // wave-uniform
                const f32x16 nz = gauss_block(ph, (uint32_t)(c0 + lc), lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) glds[wave][acc_row(r, lh)][lc] = nz[r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if ((cg >> 5) == cb) {
#pragma unroll
                    for (int it = 0; it < 8; ++it) {
                        const f32x4 n0 = *(const f32x4*)&glds[wave][it * 4 + rl][cg & 31], n1 = *(const f32x4*)&glds[wave][it * 4 + rl][(cg & 31) + 4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (col + c < sg.cols) v[it][c] = fmaf(sigs, n0[c], v[it][c]);
                            if (col + 4 + c < sg.cols) v[it][4 + c] = fmaf(sigs, n1[c], v[it][4 + c]);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();                   // the next block overwrites the image
            }
        }
    } else if (noisy) {
        const uint32_t rowhash = noise_rowhash(noise_key(seed, sg.site * 256u + sg.seg, st.iter + sg.iter_off), a.row0 + (uint32_t)(rbase + lc));
        const i32x4 hfrag = hadamard_frag(lane);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int c0 = cbase + cb * 32;
            if (c0 >= sg.cols) break;                              // wave-uniform; columns beyond are never read back
            const i32x16 nz = noise_block(rowhash, (uint32_t)c0 >> 5, lane, hfrag);
#pragma unroll
            for (int r = 0; r < 16; ++r) nlds[wave][acc_row(r, lh)][cb * 32 + lc] = (short)nz[r];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                           // same wave, in-order LDS: the reads below see the writes
    }
    if (col >= sg.cols_pad) return;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int rr = it * 4 + rl, row = rbase + rr;
        if (row >= sg.rows) break;
        if (!GAUSS && noisy && col < sg.cols) {
            const s16x8 nz = *(const s16x8*)&nlds[wave][rr][cg];
#pragma unroll
            for (int c = 0; c < 8; ++c) if (col + c < sg.cols) v[it][c] = fmaf(sigs, (float)nz[c], v[it][c]);
        }
        store8<T>(out + (long)row * sg.ldo + col, v[it]);
    }
}

// =========================================================================================
// Column-statistic kernels (BatchNorm forward / backward, feature matching).
// Block = CB (64) columns x RB (64) rows, 256 threads.  Prologue: the per-64-row partial sums of the block's
// columns are folded by 16 "partial lanes" (thread = 4 columns x every 16th partial row, 16-byte loads) and
// combined through LDS; body: thread = 8 columns (16 B of bf16) x every 32nd row.  ld/64 x rows/64 blocks keep
// >= 256 blocks in flight for the shapes of this model.
// =========================================================================================
constexpr int RB = 64, CB = 64;

__device__ __forceinline__ void fold_partials(const float* part, int npart, int ldcs, int col0, int ncols, float (*scr)[CB], float* out) {
    const int t = threadIdx.x, cq = (t & 15) * 4, pl = t >> 4;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (col0 + cq < ncols) {
        int p = pl;
        for (; p + 16 < npart; p += 32) {
            s0 += *(const f32x4*)(part + (long)p * ldcs + col0 + cq);
            s1 += *(const f32x4*)(part + (long)(p + 16) * ldcs + col0 + cq);
        }
        for (; p < npart; p += 16) s0 += *(const f32x4*)(part + (long)p * ldcs + col0 + cq);
    }
    s0 += s1;
    *(f32x4*)(&scr[pl][cq]) = s0;
    __syncthreads();
    if (t < CB) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += scr[k][t];
        out[t] = s;
    }
    __syncthreads();
}

// BatchNorm forward with batch statistics (biased variance, eps inside the sqrt; mr_gan.py:112)
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const BnApplyArgs a) {
    __shared__ float sc[CB], sh[CB];
    __shared__ float scr[16][CB], f1[CB], f2[CB];
    const int t = threadIdx.x, col0 = blockIdx.x * CB;
    // model groups (BnApplyArgs::models): grid.z = model * nseg + segment; seg_mul = 0: one model
    const int model = (int)((blockIdx.z * a.seg_mul) >> 16), seg = (int)blockIdx.z - model * a.nseg;
    const long moff = (long)model * a.model_stride;
    const float* const gamma = (const float*)((const char*)a.gamma + moff);
    const float* const beta = (const float*)((const char*)a.beta + moff);
    float* const mu = (float*)((char*)a.mu + moff);
    float* const rstd_out = (float*)((char*)a.rstd + moff);
    fold_partials((const float*)((const char*)a.cs1 + moff) + (long)seg * a.cs_seg_stride, a.npart, a.ldcs, col0, a.ld, scr, f1);
    fold_partials((const float*)((const char*)a.cs2 + moff) + (long)seg * a.cs_seg_stride, a.npart, a.ldcs, col0, a.ld, scr, f2);
    if (t < CB) {
        const int col = col0 + t;
        float scale = 0.f, shift = 0.f;
        if (col < a.ld) {
            const float mean = f1[t] / a.count;
            const float var = fmaxf(f2[t] / a.count - mean * mean, 0.f);
            const float rstd = 1.0f / sqrtf(var + a.eps);
            if (col < a.cols) { scale = gamma[col] * rstd; shift = beta[col] - mean * scale; }
            if (blockIdx.y == 0) { mu[(long)seg * a.ld + col] = mean; rstd_out[(long)seg * a.ld + col] = rstd; }
        }
        sc[t] = scale; sh[t] = shift;
    }
    __syncthreads();
    const int cg = t & 7, rl = t >> 3, c0 = col0 + cg * 8;
    if (c0 >= a.ld) return;
    const T* h = (const T*)((const char*)a.h + moff) + (long)seg * a.seg_rows * a.ld;
    T* out = (T*)((char*)a.out + moff) + (long)seg * a.seg_rows * a.ld;
    const int r1 = min(a.rows, (int)(blockIdx.y + 1) * RB);
    for (int r = blockIdx.y * RB + rl; r < r1; r += 32) {
        float v[8];
        load8<T>(h + (long)r * a.ld + c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = v[i] * sc[cg * 8 + i] + sh[cg * 8 + i];
        store8<T>(out + (long)r * a.ld + c0, v);
    }
}

// BatchNorm backward fused with the softplus derivative of the dense layer in front of it
// (h = softplus(pre)  =>  sigmoid(pre) = 1 - exp(-h)); emits the bias-gradient partial sums.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_kernel(const BnBwdArgs a) {
    __shared__ float cA[CB], cB[CB], cM[CB], cR[CB], cG[CB];   // gamma*rstd/count ; dbeta ; mu ; rstd ; dgamma
    __shared__ float red[32][CB];
    const int t = threadIdx.x, col0 = blockIdx.x * CB;
    const long moff = (long)blockIdx.z * a.model_stride;          // model groups (BnBwdArgs::models): this model's tensors
    fold_partials((const float*)((const char*)a.cs1 + moff), a.npart, a.ldcs, col0, a.ld, red, cB);
    fold_partials((const float*)((const char*)a.cs2 + moff), a.npart, a.ldcs, col0, a.ld, red, cG);
    if (t < CB) {
        const int col = col0 + t;
        float g = 0.f, mu = 0.f, rs = 0.f;
        if (col < a.cols) {
            g = ((const float*)((const char*)a.gamma + moff))[col]; mu = ((const float*)((const char*)a.mu + moff))[col];
            rs = ((const float*)((const char*)a.rstd + moff))[col];
        }
        cA[t] = g * rs / a.count; cM[t] = mu; cR[t] = rs;
    }
    __syncthreads();
    const int cg = t & 7, rl = t >> 3, c0 = col0 + cg * 8;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    if (c0 < a.ld) {
        const T* dy = (const T*)((const char*)a.dy + moff);
        const T* h = (const T*)((const char*)a.h + moff);
        T* dpre = (T*)((char*)a.dpre + moff);
        const int r1 = min(a.rows, (int)(blockIdx.y + 1) * RB);
        for (int r = blockIdx.y * RB + rl; r < r1; r += 32) {
            float hv[8], d[8], o[8];
            load8<T>(h + (long)r * a.ld + c0, hv);
            load8<T>(dy + (long)r * a.ld + c0, d);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = cg * 8 + i;
                const float xh = (hv[i] - cM[c]) * cR[c];
                const float dh = cA[c] * (a.count * d[i] - cB[c] - xh * cG[c]);
                o[i] = dh * (-expm1f(-hv[i]));
                acc[i] += o[i];
            }
            store8<T>(dpre + (long)r * a.ld + c0, o);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[rl][cg * 8 + i] = acc[i];
    __syncthreads();
    if (t < CB && col0 + t < a.ld) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) s += red[k][t];
        ((float*)((char*)a.db_part + moff))[(long)blockIdx.y * a.ld + col0 + t] = s;
    }
}

// =========================================================================================
// loss head: logits = f W6 + b6 ; labeled / unlabeled / fake losses of mr_gan.py:146-149 ; train error
// :161 ; closed-form dlogits ; dW6, db6 ; and dL/d(pre5) = (dlogits W6^T) * [f > 0].
// One block = HEAD_ROWS rows of one segment.  LDS: f tile as fp32 [HR][feat+8], W6 [feat][KP], dlogits [HR][KP].
// KP: the class pitch (8, or 32 for more than 8 classes): classes move as KP / 4 f32x4 groups.
// Per-block partial gradients go to part[blk][...]; reduce_partials_kernel folds them to <= 8 slabs.
// =========================================================================================
constexpr int HR = HEAD_ROWS;
// Accumulator of the two row products (logits, dlogits W6^T).  The bf16 head at the 32-class pitch sums them in fp64.  In the
// bf16 engine's D sub-step this kernel stands in for head_wide_kernel<false, 32> (feature width no multiple of 256,
// MRGAN_TUNE_HEAD_MFMA = 0) and has to give what that kernel gives: there every sum rounds a handful of times (exact bf16
// addend products, fp32 MFMA accumulators), here a logit is a chain of 64 fp32 roundings per 256 features and an element of
// dL/d(pre5) one of 32.  With up to 32 terms of mixed sign an element of dL/d(pre5) is worse conditioned than at 8 classes,
// and with fp32 chains its bf16 rounding differs from the matrix-core head's on more rows than the two heads are allowed
// (DESIGN.md section 4 has the figures and the cost).  make HEAD_ACC_F32=1 builds the fp32-chain variant they were taken
// against.  The fp32 engine keeps fp32 chains: it has one head and is held against the fp64 oracle with fp32 bounds.
template <bool WIDE> struct HeadAcc { typedef float type; };
#ifndef MRGAN_HEAD_ACC_F32
template <> struct HeadAcc<true> { typedef double type; };
#endif
__device__ __forceinline__ float head_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double head_fma(float a, float b, double c) { return fma((double)a, (double)b, c); }
// Q8 (fp8 mode): dpre leaves as e5m2 copies (row-major + transposed) packed from the fp32 values; a separate instantiation,
// so the bf16 / fp32 kernels keep their rolled row loop and register count
// SAL: the saliency row kinds HEAD_SAL_* (aux_kernels.h), again an instantiation of its own: the per-row dlogits go on through
// W6 and the feature layer's relu mask into dpre as in a training launch, and nothing else leaves the kernel -- no loss
// partials, no partial gradients, no error count -- beside the optional target classes (and logits)
template <typename T, bool Q8 = false, int KP = KMAX, bool SAL = false>
__global__ __launch_bounds__(256) void head_kernel(const HeadArgs a) {
    constexpr int KG = KP / 4;                 // f32x4 groups of classes
    typedef typename HeadAcc<(KP > KMAX && sizeof(T) == 2)>::type acc_t;
    extern __shared__ __attribute__((aligned(16))) float hl[];
    // the feature dimension is walked in chunks of CH <= 256 columns (one chunk for the reference's 250-wide layer)
    const int CH = min(a.feat, HEAD_CHUNK), nch = (a.feat + CH - 1) / CH;     // a ragged last chunk is zero-filled
    const int LDF = CH + 8;
    float* f_lds = hl;                         // [HR][LDF]   current chunk of f
    float* w_lds = f_lds + HR * LDF;           // [CH][KP]  matching rows of W6
    float* dl_lds = w_lds + CH * KP;           // [HR][KP]
    float* red = dl_lds + HR * KP;             // [4 waves][4]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int seg = blockIdx.y, kind = a.seg_kind[seg];
    const int row_blk = blockIdx.x * HR;
    const int blk = seg * gridDim.x + blockIdx.x;
    const long moff = (long)blockIdx.z * a.model_stride;          // model groups (HeadArgs::models): this model's tensors
    const T* f = (const T*)((const char*)a.f + moff) + (long)seg * a.f_bs;
    const float* const w6 = (const float*)((const char*)a.w + moff);

    const int cpr = CH / 8;                    // 8-element chunks per row
    auto load_chunk = [&](int c0) {
        for (int ci = t; ci < HR * cpr; ci += 256) {
            const int r = ci / cpr, c = (ci - r * cpr) * 8;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (row_blk + r < a.rows && c0 + c < a.feat) load8<T>(f + (long)(row_blk + r) * a.ldf + c0 + c, v);
            *(f32x4*)(f_lds + r * LDF + c) = (f32x4){v[0], v[1], v[2], v[3]};
            *(f32x4*)(f_lds + r * LDF + c + 4) = (f32x4){v[4], v[5], v[6], v[7]};
        }
        for (int k = t; k < CH; k += 256) {
            f32x4 w[KG];
#pragma unroll
            for (int g = 0; g < KG; ++g) w[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (c0 + k < a.feat_valid) {
#pragma unroll
                for (int g = 0; g < KG; ++g) w[g] = *(const f32x4*)(w6 + (long)(c0 + k) * a.ldw + 4 * g);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int g = 0; g < KG; ++g) if (c + 4 * g >= a.classes) w[g][c] = 0.f;
#pragma unroll
            for (int g = 0; g < KG; ++g) *(f32x4*)(w_lds + k * KP + 4 * g) = w[g];
        }
    };

    // ---- logits: LPR lanes per row, each over an interleaved slice of the features ----
    constexpr int LPR = 256 / HR;
    const int r = t / LPR, part = t % LPR;
    acc_t la[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) la[c] = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();                   // every thread is done with the previous chunk
        load_chunk(ch * CH);
        __syncthreads();
        for (int kk = 0; kk < CH / LPR; ++kk) {
            const int k = kk * LPR + part;
            const float fv = f_lds[r * LDF + k];
            f32x4 w[KG];
#pragma unroll
            for (int g = 0; g < KG; ++g) w[g] = *(const f32x4*)(w_lds + k * KP + 4 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int g = 0; g < KG; ++g) la[4 * g + c] = head_fma(fv, w[g][c], la[4 * g + c]);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) la[c] += __shfl_xor(la[c], m, 64);
    }
    float l[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) l[c] = (float)la[c];
    const int row = row_blk + r;
    const bool rowvalid = row < a.rows;
    float b[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) b[c] = (c < a.classes) ? ((const float*)((const char*)a.b + moff))[c] : 0.f;
    int y = SAL ? -1 : 0, target = 0;              // (SAL without targets: y < 0, the row's argmax)
    if (rowvalid && (SAL ? a.labels != nullptr : head_kind_has_label(kind))) {
        const long lo = a.labels_stream ? (long)a.st->batch * a.rows : 0;
        y = a.labels[(long)blockIdx.z * a.labels_ms + lo + row];
    }
    float loss0, loss1, err, dl[KP];
    head_row<true, KP, SAL>(l, b, kind, y, a.classes, a.inv_count, a.unl_weight, rowvalid, loss0, loss1, err, dl, &target);
    if (part == 0) {
        if constexpr (SAL) { if (a.classes_out && rowvalid) a.classes_out[row] = target; }
#pragma unroll
        for (int g = 0; g < KG; ++g) *(f32x4*)(dl_lds + r * KP + 4 * g) = (f32x4){dl[4 * g], dl[4 * g + 1], dl[4 * g + 2], dl[4 * g + 3]};
        if (a.logits && rowvalid) {
            float* lp = (float*)((char*)a.logits + moff) + (long)seg * a.logits_bs + (long)row * KP;
#pragma unroll
            for (int c = 0; c < KP; ++c) lp[c] = (c < a.classes) ? l[c] : 0.f;
        }
    } else { loss0 = 0.f; loss1 = 0.f; err = 0.f; }
    if constexpr (!SAL) {
        loss0 = wave_sum(loss0); loss1 = wave_sum(loss1); err = wave_sum(err);
        if (lane == 0) { red[wave * 4 + 0] = loss0; red[wave * 4 + 1] = loss1; red[wave * 4 + 2] = err; }
    }
    __syncthreads();                               // (also: dl_lds is complete)
    if (!SAL && t == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int w = 0; w < 4; ++w) { s0 += red[w * 4 + 0]; s1 += red[w * 4 + 1]; s2 += red[w * 4 + 2]; }
        if (kind == HEAD_EVAL) { if (a.err_count) atomicAdd(a.err_count, (int)(s2 + 0.5f)); }
        else if (kind != HEAD_LOGITS) {
            float* lpart = (float*)((char*)a.loss_part + moff);
            lpart[blk * 4 + 0] = s0; lpart[blk * 4 + 1] = s1;
            lpart[blk * 4 + 2] = s2; lpart[blk * 4 + 3] = 0.f;
        }
    }
    if (kind == HEAD_EVAL || kind == HEAD_LOGITS) return;

    // ---- backward of the last dense: thread <-> feature column j ----
    float* part_row = SAL ? nullptr : (float*)((char*)a.part + moff) + (long)blk * a.part_stride;
    if (!SAL && t < KP) {
        float s = 0.f;
        for (int rr = 0; rr < HR; ++rr) s += dl_lds[rr * KP + t];
        part_row[a.off_db + t] = s;
    }
    T* dpre = a.dpre ? (T*)((char*)a.dpre + moff) + (long)seg * a.dpre_bs : nullptr;
    // fp8 mode: the e5m2 copies of dpre that the dX / dW products read (one column's HR rows = HR contiguous bytes of the
    // transposed copy); packed from the fp32 value
    const float q8s = a.q8_slot ? a.q8_slot->scale : 1.f;
    float q8_amax = 0.f;
    unsigned char* q8 = a.q8 ? a.q8 + (long)seg * a.q8_bs : nullptr;
    unsigned char* q8t = a.q8t ? a.q8t + (long)seg * a.q8t_bs : nullptr;
    // the last chunk is still in LDS: walk the chunks backwards and reload only the others
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int c0 = ch * CH;
        if (ch != nch - 1) { __syncthreads(); load_chunk(c0); __syncthreads(); }
        for (int j = t; j < CH && c0 + j < a.feat; j += 256) {
            float wj[KP], dw[KP];
#pragma unroll
            for (int c = 0; c < KP; ++c) { wj[c] = w_lds[j * KP + c]; dw[c] = 0.f; }
            float dbf = 0.f;
            auto row_step = [&](int rr) -> float {
                const float fv = f_lds[rr * LDF + j];
                f32x4 d[KG];
#pragma unroll
                for (int g = 0; g < KG; ++g) d[g] = *(const f32x4*)(dl_lds + rr * KP + 4 * g);
                acc_t dfe = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int g = 0; g < KG; ++g) dfe = head_fma(d[g][c], wj[4 * g + c], dfe);
#pragma unroll
                    for (int g = 0; g < KG; ++g) dw[4 * g + c] = fmaf(fv, d[g][c], dw[4 * g + c]);
                }
                const float dp = (fv > 0.f) ? (float)dfe : 0.f;
                if (dpre && row_blk + rr < a.rows) dpre[(long)(row_blk + rr) * a.ldd + c0 + j] = Elem<T>::from_f32(dp);
                dbf += dp;
                return dp;
            };
            if constexpr (Q8) {
                // 16 rows at a time: four dwords = 16 contiguous bytes of the transposed copy; the row-major copy trades bytes
                // inside the lane quad (4 neighbouring columns; CH and the column stride are multiples of 4) and stores one
                // dword per four rows.  Rows >= a.rows have dl == 0, hence dp == 0: zero bytes.
                typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
                const int kq = t & 3;
#pragma unroll 1
                for (int k16 = 0; k16 < HR / 16; ++k16) {
                    uint32_t qw[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float q4[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) { q4[i] = row_step(16 * k16 + 4 * k + i); q8_amax = fmaxf(q8_amax, fabsf(q4[i])); }
                        qw[k] = fp8_pack4<FP8_E5M2>(q4[0], q4[1], q4[2], q4[3], q8s);
                        __builtin_amdgcn_sched_barrier(0);      // keep the LDS reads of the next four rows from being hoisted (registers)
                    }
                    if (q8t) *(u32x4_t*)(q8t + (long)(c0 + j) * a.ldq8t + row_blk + 16 * k16) = (u32x4_t){qw[0], qw[1], qw[2], qw[3]};
                    if (q8) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t w = quad_byte_transpose(qw[k]);
                            const int row = row_blk + 16 * k16 + 4 * k + kq;
                            if (row < a.rows) *(uint32_t*)(q8 + (long)row * a.ldq8 + c0 + j - kq) = w;
                        }
                    }
                }
            } else {
                for (int rr = 0; rr < HR; ++rr) row_step(rr);
            }
            if constexpr (!SAL) {
#pragma unroll
                for (int g = 0; g < KG; ++g)
                    *(f32x4*)(part_row + (long)(c0 + j) * KP + 4 * g) = (f32x4){dw[4 * g], dw[4 * g + 1], dw[4 * g + 2], dw[4 * g + 3]};
                part_row[a.off_dbf + c0 + j] = dbf;
            }
        }
    }
    if constexpr (Q8) fp8_amax_commit(a.q8_slot, q8_amax);
}

// =========================================================================================
// saliency maps (mrgan_input_gradient, mrgan_attribution): the layer-0 dX of a draw -> the caller's fp32 rows
// =========================================================================================
// the heat-map's row statistics (one block = one row, every thread calls): a thread's sum g^2, max |g| and min |g| over its
// columns -> the row's denominator rms + 1e-5, min a and max a - min a
struct HeatRow { float denom, amin, range; };
__device__ __forceinline__ void heat_accum(const float v[8], int c, int cols, float& ss, float& mx, float& mn) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (c + i < cols) { ss = fmaf(v[i], v[i], ss); mx = fmaxf(mx, fabsf(v[i])); mn = fminf(mn, fabsf(v[i])); }
    }
}
__device__ __forceinline__ HeatRow heat_row(float ss, float mx, float mn, int cols, float (*red)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o, 64); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    if (lane == 0) { red[0][wave] = ss; red[1][wave] = mx; red[2][wave] = mn; }
    __syncthreads();
    ss = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    mn = fminf(fminf(red[2][0], red[2][1]), fminf(red[2][2], red[2][3]));
    HeatRow h;
    h.denom = sqrtf(ss / (float)cols) + 1e-5f;
    h.amin = mn / h.denom;
    h.range = mx / h.denom - h.amin;
    return h;
}
__device__ __forceinline__ void heat_map8(float v[8], const HeatRow& h) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h.range > 0.f ? (fabsf(v[i]) / h.denom - h.amin) / h.range : 0.f;
}

// path stage: block = 256 threads x 8 consecutive columns of one row (grid.y = rows); AttrAccumArgs / PathStageArgs, aux_kernels.h
template <typename T>
__global__ __launch_bounds__(256) void path_stage_kernel(const PathStageArgs a) {
    const int row = blockIdx.y, c = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 8;
    if (c >= a.cols_pad) return;                                   // (cols_pad is a multiple of 8: the group lies inside it)
    const float* src = a.src + (a.idx ? (long)a.idx[row] : (long)row) * a.ld + c;
    float v[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = 0.f; b[i] = 0.f; }
    if (c + 7 < a.cols && (a.ld & 3) == 0 && ((uintptr_t)a.src & 15) == 0) load8<float>(src, v);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (c + i < a.cols) v[i] = src[i];
    }
    if (a.baseline) {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (c + i < a.cols) b[i] = a.baseline[c + i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = c + i < a.cols ? fmaf(a.alpha, v[i] - b[i], b[i]) : 0.f;
    store8<T>((T*)a.out + (long)row * a.ldo + c, v);
}

// accumulate (the only kernel that writes a map): one block = one row of the layer-0 dX (T, pitch ldg) -> one fp32 row of the
// caller (AttrAccumArgs), thread <-> 8 consecutive columns, every 2048th column group.  Each thread reads and writes only its
// own columns of out, so the second pass of the heat-map reads back what the same thread stored (or, for the one-draw map
// without multiply, the same values from g again: measured, profiles/README.md).  SAL_HEATMAP: sum g^2, max |g|
// and min |g| of the row by wave shuffles, then over the four waves through LDS in wave order -- no atomics: the same bits on
// every call.  |g| / denom is monotone in |g|, so min a and max a are the quotients of min |g| and max |g|, and the elements
// that attain them come out as exactly 0 and 1.
template <typename T>
__global__ __launch_bounds__(256) void attribution_accum_kernel(const AttrAccumArgs a) {
    __shared__ float red[3][4];
    const int t = threadIdx.x, row = blockIdx.x;
    const T* g = (const T*)a.g + (long)row * a.ldg;
    float* out = a.out + (long)row * a.ldo;
    const bool last = a.draw == a.draws - 1, heat = last && a.mode == SAL_HEATMAP;
    const bool once = heat && a.draws == 1 && !a.multiply;     // the map of g itself: g is read twice, out written once (block-uniform)
    const bool vec = (((uintptr_t)out) & 15) == 0;
    const float* xr = (last && a.multiply) ? a.x + (a.idx ? (long)a.idx[row] : (long)row) * a.ld_x : nullptr;
    const float ndraws = (float)a.draws;
    float ss = 0.f, mx = 0.f, mn = 3.0e38f;
    for (int c = t * 8; c < a.cols; c += 2048) {           // (ldg is a multiple of 8: the group lies inside the padded row)
        float v[8];
        load8<T>(g + c, v);
        const bool full = vec && c + 7 < a.cols;
        if (a.draw > 0) {
            float o[8];
            if (full) load8<float>(out + c, o);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = c + i < a.cols ? out[c + i] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = o[i] + v[i];
        }
        if (last) {
            if (a.draws > 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = v[i] / ndraws;
            }
            if (xr) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (c + i < a.cols) v[i] *= xr[c + i] - (a.baseline ? a.baseline[c + i] : 0.f);
            }
            if (heat) heat_accum(v, c, a.cols, ss, mx, mn);
        }
        if (once) continue;
        if (full) store8<float>(out + c, v);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) if (c + i < a.cols) out[c + i] = v[i];
        }
    }
    if (!heat) return;                                     // (block-uniform)
    const HeatRow hr = heat_row(ss, mx, mn, a.cols, red);
    for (int c = t * 8; c < a.cols; c += 2048) {
        float v[8];
        const bool full = vec && c + 7 < a.cols;
        if (once) load8<T>(g + c, v);
        else if (full) load8<float>(out + c, v);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = c + i < a.cols ? out[c + i] : 0.f;
        }
        heat_map8(v, hr);
        if (full) store8<float>(out + c, v);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) if (c + i < a.cols) out[c + i] = v[i];
        }
    }
}

// =========================================================================================
// autoencoder: the reconstruction (mse) head, the fold of its loss partials across the chunks of mrgan_ae_reconstruct, and the
// copy of stored activation rows to the caller's fp32 rows (ReconHeadArgs, aux_kernels.h)
// block = 64 rows x 64 columns; thread <-> 8 consecutive columns x rows (t >> 3) and (t >> 3) + 32
// =========================================================================================
template <typename T>
__global__ __launch_bounds__(256) void recon_head_kernel(const ReconHeadArgs a) {
    __shared__ float red[32][CB + 1];
    __shared__ float wsum[4];
    const int t = threadIdx.x, cg = (t & 7) * 8, rl = t >> 3;
    const int col = (int)blockIdx.x * CB + cg, row0 = (int)blockIdx.y * RB;
    const long o = a.stream ? (long)a.st->batch * a.batch_rows : 0;
    const bool xvec = (a.ld_x & 3) == 0 && ((uintptr_t)a.x & 15) == 0 && col + 7 < a.cols;
    float csum[8], sq = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) csum[c] = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = row0 + rl + 32 * i;
        float g[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) g[c] = 0.f;
        if (row < a.rows_valid && col < a.cols) {
            float y[8], x[8];
            load8<T>((const T*)a.y + (long)row * a.ldy + col, y);
            const float* xr = a.x + (a.idx ? (long)a.idx[o + row] : o + row) * a.ld_x + col;
            if (xvec) load8<float>(xr, x);
            else {
#pragma unroll
                for (int c = 0; c < 8; ++c) x[c] = col + c < a.cols ? xr[c] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float d = col + c < a.cols ? y[c] - x[c] : 0.f;
                sq = fmaf(d, d, sq);
                g[c] = Elem<T>::to_f32(Elem<T>::from_f32(a.scale * d));      // the stored value: what the dW product reads
                csum[c] += g[c];
            }
        }
        if (a.dy && row < a.rows) store8<T>((T*)a.dy + (long)row * a.ldd + col, g);
    }
    if (a.cs) {
#pragma unroll
        for (int c = 0; c < 8; ++c) red[rl][cg + c] = csum[c];
    }
    sq = wave_sum(sq);
    if ((t & 63) == 0) wsum[t >> 6] = sq;
    __syncthreads();
    if (a.cs && t < CB) {
        float s = 0.f;
        for (int k = 0; k < 32; ++k) s += red[k][t];                          // fixed order: reproducible
        a.cs[(long)blockIdx.y * a.ldcs + (int)blockIdx.x * CB + t] = s;
    }
    if (t == 0) {
        float* lp = a.loss_part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        lp[0] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]); lp[1] = 0.f; lp[2] = 0.f; lp[3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void fold_loss_kernel(const float* part, int n, float* acc, int first) {
    __shared__ float ms[256];
    const int t = threadIdx.x;
    float s = 0.f;
    for (int i = t; i < n; i += 256) s += part[(long)i * 4];
    ms[t] = s;
    __syncthreads();
    if (t == 0) {
        float tot = 0.f;
        for (int k = 0; k < 256; ++k) tot += ms[k];                           // fixed order: reproducible
        acc[0] = (first ? 0.f : acc[0]) + tot;
    }
}

// block = 256 threads x 8 consecutive columns of one row (grid.y = rows), as path_stage_kernel
template <typename T>
__global__ __launch_bounds__(256) void cast_rows_kernel(const T* src, int lds, int cols, float* dst, long ldd) {
    const int row = blockIdx.y, c = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 8;
    if (c >= cols) return;                                     // (lds is a multiple of 8 and >= cols: the group lies inside the padded row)
    float v[8];
    load8<T>(src + (long)row * lds + c, v);
    float* out = dst + (long)row * ldd + c;
    if (c + 7 < cols && (ldd & 3) == 0 && ((uintptr_t)dst & 15) == 0) store8<float>(out, v);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (c + i < cols) out[i] = v[i];
    }
}

// dst[g][i] = sum of src[p][i] over the partial rows p of group g (p = g, g + ngroups, ...)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* src, int nsrc, long stride, int n, int ngroups, float* dst,
                                                              long model_stride) {
    const int i = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (i >= n) return;
    src = (const float*)((const char*)src + (long)blockIdx.z * model_stride);      // model groups: grid.z = models
    dst = (float*)((char*)dst + (long)blockIdx.z * model_stride);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = g;
    for (; p + 3 * ngroups < nsrc; p += 4 * ngroups) {
        s0 += src[(long)p * stride + i]; s1 += src[(long)(p + ngroups) * stride + i];
        s2 += src[(long)(p + 2 * ngroups) * stride + i]; s3 += src[(long)(p + 3 * ngroups) * stride + i];
    }
    for (; p < nsrc; p += ngroups) s0 += src[(long)p * stride + i];
    dst[(long)g * stride + i] = (s0 + s1) + (s2 + s3);
}

// =========================================================================================
// feature matching: loss = mean_j (mean_b f_fake - mean_b f_real)^2 ; dL/df_fake broadcast over rows,
// masked by the feature layer's ReLU.
// =========================================================================================
template <typename T>
__global__ __launch_bounds__(256) void fm_kernel(const FmArgs a) {
    __shared__ float gj_lds[CB];
    __shared__ float scr[16][CB], sf[CB], sr[CB];
    const int t = threadIdx.x, col0 = blockIdx.x * CB;
    const long moff = (long)blockIdx.z * a.model_stride;          // model groups (FmArgs::models): this model's tensors
    const float* const cs = (const float*)((const char*)a.cs + moff);
    const float* cs_real = cs + (long)a.npart_fake * a.ldcs;
    const bool dist_loss = a.lscratch != nullptr;
    float* const loss_out = a.loss_out ? (float*)((char*)a.loss_out + moff) : nullptr;
    float* const accum = a.accum ? (float*)((char*)a.accum + moff) : nullptr;
    if (!dist_loss && blockIdx.y == gridDim.y - 1) {
        // the extra block row: block x == 0 produces the loss scalar, which needs every column.  Thread = 4 columns x
        // every 4th partial row, all loads independent, so this block is no slower than the row blocks.
        if (blockIdx.x != 0) return;
        float* dsc = &scr[0][0];                          // [4][256] view of the 16 x 64 scratch
        float tot = 0.f;
        const int q = (t & 63) * 4, pl = t >> 6;
        for (int c0 = 0; c0 < a.feat; c0 += 256) {
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (c0 + q < a.feat) {
                // four independent partial sums per stream: the loads of a wide feature layer's 128 partial rows overlap
                // instead of forming one dependent chain (this single block was the kernel's critical path: 0.27 ms)
                f32x4 s0 = d, s1 = d, s2 = d, s3 = d;
                int p = pl;
                for (; p + 12 < a.npart_fake; p += 16) {
                    s0 += *(const f32x4*)(cs + (long)p * a.ldcs + c0 + q); s1 += *(const f32x4*)(cs + (long)(p + 4) * a.ldcs + c0 + q);
                    s2 += *(const f32x4*)(cs + (long)(p + 8) * a.ldcs + c0 + q); s3 += *(const f32x4*)(cs + (long)(p + 12) * a.ldcs + c0 + q);
                }
                for (; p < a.npart_fake; p += 4) s0 += *(const f32x4*)(cs + (long)p * a.ldcs + c0 + q);
                p = pl;
                for (; p + 12 < a.npart_real; p += 16) {
                    s0 -= *(const f32x4*)(cs_real + (long)p * a.ldcs + c0 + q); s1 -= *(const f32x4*)(cs_real + (long)(p + 4) * a.ldcs + c0 + q);
                    s2 -= *(const f32x4*)(cs_real + (long)(p + 8) * a.ldcs + c0 + q); s3 -= *(const f32x4*)(cs_real + (long)(p + 12) * a.ldcs + c0 + q);
                }
                for (; p < a.npart_real; p += 4) s0 -= *(const f32x4*)(cs_real + (long)p * a.ldcs + c0 + q);
                d = (s0 + s1) + (s2 + s3);
            }
            __syncthreads();
            *(f32x4*)(dsc + pl * 256 + q) = d;
            __syncthreads();
            float v = 0.f;
            if (c0 + t < a.feat_valid) { v = (dsc[t] + dsc[256 + t] + dsc[512 + t] + dsc[768 + t]) / a.count; v *= v; }
            v = wave_sum(v);
            if ((t & 63) == 0) sf[t >> 6] = v;
            __syncthreads();
            if (t == 0) tot += sf[0] + sf[1] + sf[2] + sf[3];
        }
        if (t == 0) {
            const float loss = tot / (float)a.feat_valid;
            if (loss_out) *loss_out = loss;
            if (accum) *accum += loss;
        }
        return;
    }
    fold_partials(cs, a.npart_fake, a.ldcs, col0, a.feat, scr, sf);
    fold_partials(cs_real, a.npart_real, a.ldcs, col0, a.feat, scr, sr);
    if (t < CB) {
        const float diff = (col0 + t < a.feat_valid) ? (sf[t] - sr[t]) / a.count : 0.f;
        gj_lds[t] = a.grad_scale * 2.0f / ((float)a.feat_valid * a.count) * diff;
        if (dist_loss && blockIdx.y == 0) {
            // this column block's share of sum_j diff_j^2 (one wave: CB == 64), then the ticket
            const float part = wave_sum(diff * diff);
            __shared__ unsigned int ticket;
            float* const lscratch = (float*)((char*)a.lscratch + moff);              // (each model its own partials and ticket)
            unsigned int* const lcount = (unsigned int*)((char*)a.lcount + moff);
            if (t == 0) {
                lscratch[blockIdx.x] = part;
                __threadfence();
                ticket = atomicAdd(lcount, 1u);
            }
            if (t == 0 && ticket == gridDim.x - 1) {
                __threadfence();
                float tot = 0.f;
                for (unsigned int i = 0; i < gridDim.x; ++i) tot += ((volatile float*)lscratch)[i];      // fixed order: reproducible
                const float loss = tot / (float)a.feat_valid;
                if (loss_out) *loss_out = loss;
                if (accum) *accum += loss;
                *lcount = 0u;
            }
        }
    }
    __syncthreads();
    const int cg = t & 7, rl = t >> 3, c0 = col0 + cg * 8;
    if (c0 >= a.feat) return;
    T* dpre = a.dpre ? (T*)((char*)a.dpre + moff) : nullptr;
    const uint16_t* const mask = (const uint16_t*)((const char*)a.mask + moff);
    const float q8s = a.q8_slot ? a.q8_slot->scale : 1.f;
    float q8_amax = 0.f;
    const int r1 = min(a.rows, (int)(blockIdx.y + 1) * a.rb);
    for (int r = blockIdx.y * a.rb + rl; r < r1; r += 32) {
        // lane-native mask layout (gemm.h): per (32-row block, column) two u16 words, one per lane half
        const int rr = r & 31, half = (rr >> 2) & 1, bit = (rr & 3) | ((rr >> 3) << 2);
        const uint32_t* mp = (const uint32_t*)(mask + ((long)(r >> 5) * a.ldm + c0) * 2);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (((mp[i] >> (16 * half)) >> bit) & 1u) ? gj_lds[cg * 8 + i] : 0.f;
        if (dpre) store8<T>(dpre + (long)r * a.ldd + c0, v);
        if (a.q8_slot) {                          // fp8 mode: the e5m2 copy the dX product reads
#pragma unroll
            for (int i = 0; i < 8; ++i) q8_amax = fmaxf(q8_amax, fabsf(v[i]));
            typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
            *(u32x2_t*)(a.q8 + (long)r * a.ldq8 + c0) = (u32x2_t){fp8_pack4<FP8_E5M2>(v[0], v[1], v[2], v[3], q8s), fp8_pack4<FP8_E5M2>(v[4], v[5], v[6], v[7], q8s)};
        }
    }
    if (a.q8_slot) fp8_amax_commit(a.q8_slot, q8_amax);
}

// two sets of per-row-tile partial sums -> two rows of `out` (out[0..n) and out[n..2n)); blockIdx.y picks the set
// blockIdx.z: independent segments (their partial rows follow each other, `seg_part` floats apart; their results 2 n apart)
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* part1, const float* part2, int npart, int ld, int n, float* out, long seg_part) {
    __shared__ float scr[16][CB], res[CB];
    const int col0 = blockIdx.x * CB;
    fold_partials((blockIdx.y ? part2 : part1) + (long)blockIdx.z * seg_part, npart, ld, col0, n, scr, res);
    if (threadIdx.x < CB && col0 + threadIdx.x < n) out[((long)blockIdx.z * 2 + blockIdx.y) * n + col0 + threadIdx.x] = res[threadIdx.x];
}

// =========================================================================================
// Adam, Keras 2.0.9: m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr_t m / (sqrt(v) + eps).
// One block = one 64x64 tile of one tensor.  The gradient is the sum of `nslab` fp32 slabs (split-K
// weight-gradient slabs, per-row-tile bias partial sums), so no separate reduction pass exists on
// one GPU.  Also refreshes the bf16 weight copies W[K][N] and W^T[N][K] the bf16 GEMMs read.
// Small tiles (<= 64 four-element groups: biases, BN affine) spread their slabs over the otherwise
// idle threads ("slab lanes") and combine through LDS.
// =========================================================================================
__device__ __forceinline__ f32x4 adam_sum_slabs(const float* g, long stride, int first, int step, int nslab) {
    f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0, g2 = g0, g3 = g0;
    int sl = first;
    for (; sl + 3 * step < nslab; sl += 4 * step) {
        g0 += *(const f32x4*)(g + (long)sl * stride);
        g1 += *(const f32x4*)(g + (long)(sl + step) * stride);
        g2 += *(const f32x4*)(g + (long)(sl + 2 * step) * stride);
        g3 += *(const f32x4*)(g + (long)(sl + 3 * step) * stride);
    }
    for (; sl < nslab; sl += step) g0 += *(const f32x4*)(g + (long)sl * stride);
    return (g0 + g1) + (g2 + g3);
}

// the flat gradient of one four-element group: fp32, or bfloat16 when the gradients travel as bfloat16 (MRGAN_FLAG_GRAD_BF16)
__device__ __forceinline__ f32x4 flat_load(const AdamTile& tile, long off) {
    if (tile.flat16) { const bf16x4 v = *(const bf16x4*)(tile.flat16 + off); return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }
    return *(const f32x4*)(tile.flat + off);
}
__device__ __forceinline__ void flat_store(const AdamTile& tile, long off, const f32x4 g) {
    if (tile.flat16) *(bf16x4*)(tile.flat16 + off) = (bf16x4){(__bf16)g[0], (__bf16)g[1], (__bf16)g[2], (__bf16)g[3]};
    else *(f32x4*)(tile.flat + off) = g;
}

template <typename P>
__device__ __forceinline__ void shift_ptr(P*& p, long bytes) { if (p) p = (P*)((char*)p + bytes); }

__global__ __launch_bounds__(256) void adam_kernel(const AdamArgs a) {
    __shared__ float tl[64 * 65];
    const int t = threadIdx.x;
    // block 0 is the serial one (next DevState with two double-precision pow(), the loss partials folded in a fixed order): first
    // in dispatch order, so that it runs beside the tile blocks instead of behind them
    const int tile_id = (int)blockIdx.x - 1;
    if (tile_id >= 0) {
    AdamTile tile = a.tiles[tile_id];
    {   // model groups (AdamArgs::models): the table describes model 0, this block works on model blockIdx.y
        const long mo = (long)blockIdx.y * a.model_stride;
        shift_ptr(tile.p, mo); shift_ptr(tile.m, mo); shift_ptr(tile.v, mo); shift_ptr(tile.g, mo); shift_ptr(tile.flat, mo);
        shift_ptr(tile.flat16, mo); shift_ptr(tile.w16, mo); shift_ptr(tile.wt16, mo);
    }
    const float lr_t = a.st->lr_t;
    const int qpr = tile.cols >> 2;                       // four-element groups per row
    const int nq = tile.rows * qpr;
    const bool small = nq <= 64 && !tile.wt16;            // slab-parallel mode
    const float w8_scale = tile.w8_slot ? tile.w8_slot->scale : 1.f;
    float w8_amax = 0.f;
    const int QL = nq <= 16 ? 16 : 64;                    // element-group slots; the other threads are slab lanes
    const int lanes = small ? 256 / QL : 1;
    // update of one four-element group: Keras-2.0.9 Adam (eps outside the square root) + the bf16 / fp8 weight copies
    auto update = [&](const f32x4 g, f32x4 m, f32x4 v, f32x4& pn, long off) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m[i] = a.b1 * m[i] + (1.0f - a.b1) * g[i];
            v[i] = a.b2 * v[i] + (1.0f - a.b2) * g[i] * g[i];
            pn[i] = pn[i] - lr_t * m[i] / (sqrtf(v[i]) + a.eps);
        }
        *(f32x4*)(tile.m + off) = m; *(f32x4*)(tile.v + off) = v; *(f32x4*)(tile.p + off) = pn;
        if (tile.w16) {
            bf16x4 w = {(__bf16)pn[0], (__bf16)pn[1], (__bf16)pn[2], (__bf16)pn[3]};
            *(bf16x4*)(tile.w16 + off) = w;
            if (tile.w8_slot) {           // fp8 mode: e4m3 copy of the bf16 values (what quant8_kernel would produce from w16)
#pragma unroll
                for (int i = 0; i < 4; ++i) { pn[i] = (float)w[i]; w8_amax = fmaxf(w8_amax, fabsf(pn[i])); }
                *(uint32_t*)(tile.w8 + off) = fp8_pack4<FP8_E4M3>(pn[0], pn[1], pn[2], pn[3], w8_scale);
            }
        }
    };
    if (small) {
        int sl0 = t / QL;
        const int qi = t & (QL - 1);
        int r = qi / qpr;
        const int tc = (qi - r * qpr) * 4;
        if (qi >= nq) r = tile.rows;
        const bool valid = r < tile.rows && tc < tile.cols;
        const long off = (long)r * tile.ld + tc;
        f32x4 g = {0.f, 0.f, 0.f, 0.f}, pn = g;
        if (valid) {
            if (a.mode == ADAM_FROM_FLAT) { if (sl0 == 0) g = flat_load(tile, off); }
            else g = adam_sum_slabs(tile.g + off, tile.slab_stride, sl0, lanes, tile.nslab);
        }
        *(f32x4*)(tl + t * 4) = g;                        // combine the slab lanes
        __syncthreads();
        if (sl0 == 0)
            for (int k = 1; k < lanes; ++k) g += *(const f32x4*)(tl + (t + QL * k) * 4);
        if (valid && sl0 == 0) {
            if (a.mode == ADAM_REDUCE_ONLY) flat_store(tile, off, g);
            else { pn = *(const f32x4*)(tile.p + off); update(g, *(const f32x4*)(tile.m + off), *(const f32x4*)(tile.v + off), pn, off); }
        }
    } else {
        // four row groups per thread; all their loads (gradient slabs, m, v, p) are issued before the first store (a load behind
        // a store through another pointer is not hoisted by the compiler)
        const int tc = (t & 15) * 4;
        f32x4 g[4], m[4], v[4], pn[4];
        long off[4];
        bool valid[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = (t >> 4) + 16 * u;
            valid[u] = r < tile.rows && tc < tile.cols;
            off[u] = (long)r * tile.ld + tc;
            g[u] = m[u] = v[u] = pn[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (valid[u]) {
                g[u] = a.mode == ADAM_FROM_FLAT ? flat_load(tile, off[u]) : adam_sum_slabs(tile.g + off[u], tile.slab_stride, 0, 1, tile.nslab);
                if (a.mode != ADAM_REDUCE_ONLY) { m[u] = *(const f32x4*)(tile.m + off[u]); v[u] = *(const f32x4*)(tile.v + off[u]); pn[u] = *(const f32x4*)(tile.p + off[u]); }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = (t >> 4) + 16 * u;
            if (valid[u]) {
                if (a.mode == ADAM_REDUCE_ONLY) flat_store(tile, off[u], g[u]);
                else update(g[u], m[u], v[u], pn[u], off[u]);
            }
            if (tile.wt16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) tl[(tc + i) * 65 + r] = pn[u][i];
            }
        }
    }
    if (tile.wt16 && a.mode != ADAM_REDUCE_ONLY) {
        __syncthreads();
        const int cc = t >> 2, rr0 = (t & 3) * 16;
        if (cc < tile.cols && rr0 < tile.rows) {
            bf16x8 lo, hi;
#pragma unroll
            for (int i = 0; i < 8; ++i) { lo[i] = (__bf16)tl[cc * 65 + rr0 + i]; hi[i] = (__bf16)tl[cc * 65 + rr0 + 8 + i]; }
            *(bf16x8*)(tile.wt16 + (long)cc * tile.ldt + rr0) = lo;
            *(bf16x8*)(tile.wt16 + (long)cc * tile.ldt + rr0 + 8) = hi;
            if (tile.w8_slot) {
                typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
                float f[16];
#pragma unroll
                for (int i = 0; i < 8; ++i) { f[i] = (float)lo[i]; f[8 + i] = (float)hi[i]; }
                *(u32x4_t*)(tile.w8t + (long)cc * tile.ldt + rr0) =
                    (u32x4_t){fp8_pack4<FP8_E4M3>(f[0], f[1], f[2], f[3], w8_scale), fp8_pack4<FP8_E4M3>(f[4], f[5], f[6], f[7], w8_scale),
                              fp8_pack4<FP8_E4M3>(f[8], f[9], f[10], f[11], w8_scale), fp8_pack4<FP8_E4M3>(f[12], f[13], f[14], f[15], w8_scale)};
            }
        }
    }
    if (tile.w8_slot && a.mode != ADAM_REDUCE_ONLY) fp8_amax_commit(tile.w8_slot, w8_amax);
    }
    // ---- block 0: the next sub-step's DevState, and this sub-step's loss partials ----
    if (tile_id < 0 && t == 0 && blockIdx.y == 0 && a.next && a.mode != ADAM_REDUCE_ONLY) {
        const DevState st = *a.st;
        DevState nx;
        nx.iter = st.iter + 1;
        nx.batch = st.batch + (uint32_t)a.advance_batch;
        const double tt = (double)nx.iter + 1.0;
        nx.lr_t = (float)((double)a.lr * sqrt(1.0 - pow((double)a.b2, tt)) / (1.0 - pow((double)a.b1, tt)));
        nx.pad = 0;
        *a.next = nx;
    }
    if (tile_id < 0 && a.step_out) {
        __shared__ float ms[3][256];
        const long mo = (long)blockIdx.y * a.model_stride;         // the metrics finish runs per model
        const float* const loss_part = (const float*)((const char*)a.loss_part + mo);
        float* const step_out = (float*)((char*)a.step_out + mo);
        float* const accum = (float*)((char*)a.accum + mo);
        float s[3] = {0.f, 0.f, 0.f};
        if (a.mode == ADAM_FROM_FLAT) { if (t == 0) for (int i = 0; i < 3; ++i) s[i] = a.flat_tail[i]; }
        else {
            for (int b = t; b < a.nloss_part; b += 256)
                for (int i = 0; i < 3; ++i) s[i] += loss_part[b * 4 + i];
            for (int i = 0; i < 3; ++i) ms[i][t] = s[i];
            __syncthreads();
            if (t == 0) {
                for (int i = 0; i < 3; ++i) {
                    float acc = 0.f;
                    for (int k = 0; k < 256; ++k) acc += ms[i][k];       // fixed order: reproducible
                    s[i] = acc * a.inv_rows;
                }
            }
        }
        if (t == 0) {
            if (a.mode == ADAM_REDUCE_ONLY) { for (int i = 0; i < 3; ++i) a.flat_tail[i] = s[i]; a.flat_tail[3] = 0.f; }
            else { for (int i = 0; i < 3; ++i) { step_out[i] = s[i]; accum[i] += s[i]; } }
        }
    }
}

// what a handle's generator draws: NOISE_SCALE * noise_block, or (gauss) gauss_block as it is
__global__ __launch_bounds__(64) void noise_debug_kernel(int gauss, uint64_t seed, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0,
                                                         int rows, int cols, float* out) {
    const int lane = threadIdx.x, lc = lane & 31, lh = lane >> 5;
    const int rbase = blockIdx.y * 32, c0 = blockIdx.x * 32;
    if (gauss) {                                                   // (kernel argument: wave-uniform)
        const f32x16 ng = gauss_block(gauss_pairhash(noise_key(seed, site * 256u + seg, step), row0 + (uint32_t)rbase, lane), (uint32_t)(c0 + lc), lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rbase + acc_row(r, lh);
            if (row < rows && c0 + lc < cols) out[(long)row * cols + c0 + lc] = ng[r];
        }
        return;
    }
    const uint32_t rh = noise_rowhash(noise_key(seed, site * 256u + seg, step), row0 + (uint32_t)(rbase + lc));
    const i32x16 nz = noise_block(rh, (uint32_t)c0 >> 5, lane, hadamard_frag(lane));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = rbase + acc_row(r, lh);
        if (row < rows && c0 + lc < cols) out[(long)row * cols + c0 + lc] = NOISE_SCALE * (float)nz[r];
    }
}

}  // namespace

#define LAUNCH_T(kern, grid, block, smem, s, args)                                  \
    do {                                                                            \
        if (bf16) MRGAN_LAUNCH(kern<__bf16>, grid, block, smem, s, args);     \
        else MRGAN_LAUNCH(kern<float>, grid, block, smem, s, args);           \
    } while (0)
#define RET_LAUNCH return hipGetLastError() == hipSuccess ? 0 : -2

int launch_stage(int bf16, const StageArgs& a, hipStream_t s) {
    int maxc = 0, maxr = 0, maxm = 1;
    for (int i = 0; i < a.nseg; ++i) { maxc = max(maxc, a.s[i].cols_pad); maxr = max(maxr, a.s[i].rows); maxm = max(maxm, a.s[i].models); }
    for (int i = 0; i < a.nseg; ++i) if (max(1, a.s[i].models) != maxm) return -3;      // every segment of a launch once per model
    StageArgs b = a;
    b.ry = ceil_div(maxr, 128); b.ry_mul = 0;
    if (maxm > 1) {
        // the kernel's multiply-shift is the exact quotient while grid.y * ry < 65536 (batches up to 8192 rows at 16 models)
        if ((long)b.ry * maxm * b.ry >= 65536) return -3;
        b.ry_mul = div_mul16(b.ry);
    }
    dim3 grid(ceil_div(maxc, 128), b.ry * maxm, a.nseg);
    if (a.gauss) {
        if (bf16) MRGAN_LAUNCH((stage_kernel<__bf16, true>), grid, dim3(256), 0, s, b);
        else MRGAN_LAUNCH((stage_kernel<float, true>), grid, dim3(256), 0, s, b);
    } else LAUNCH_T(stage_kernel, grid, dim3(256), 0, s, b);
    RET_LAUNCH;
}

int launch_bn_apply(int bf16, const BnApplyArgs& a, hipStream_t s) {
    BnApplyArgs b = a;
    b.nseg = std::max(1, a.nseg);
    const int models = std::max(1, a.models);
    b.seg_mul = models > 1 ? div_mul16(b.nseg) : 0u;      // (exact far beyond MRGAN_MAX_MODELS x 2 segments)
    dim3 grid(ceil_div(a.ld, CB), ceil_div(a.rows, RB), b.nseg * models);
    LAUNCH_T(bn_apply_kernel, grid, dim3(256), 0, s, b);
    RET_LAUNCH;
}

int stat_row_blocks(int rows) { return ceil_div(rows, RB); }

int launch_bn_bwd(int bf16, const BnBwdArgs& a, hipStream_t s) {
    dim3 grid(ceil_div(a.ld, CB), ceil_div(a.rows, RB), std::max(1, a.models));
    LAUNCH_T(bn_bwd_kernel, grid, dim3(256), 0, s, a);
    RET_LAUNCH;
}

int init_kernel_attributes() {
    // must run outside stream capture; called from mrgan_create
    hipError_t e = hipFuncSetAttribute((const void*)head_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<__bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<float, false, KWIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<__bf16, false, KWIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    // ... and its saliency instantiations
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<float, false, KMAX, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<__bf16, false, KMAX, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<float, false, KWIDE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)head_kernel<__bf16, false, KWIDE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    return e == hipSuccess ? 0 : -2;
}

int launch_head(int bf16, const HeadArgs& a, hipStream_t s) {
    const int ch = std::min(a.feat, HEAD_CHUNK);
    const int kp = a.ldw;                      // the class pitch of W6, the logits and the partial-gradient rows
    if ((a.feat % 64) != 0 || (kp != KMAX && kp != KWIDE) || a.classes > kp) return -3;
    const size_t smem = sizeof(float) * ((size_t)HR * (ch + 8) + (size_t)ch * kp + HR * kp + 16);
    dim3 grid(ceil_div(a.rows, HR), a.nseg, std::max(1, a.models));
    if (a.models > 1 && (a.q8_slot || a.err_count)) return -3;      // model groups: training heads without fp8 copies
    int nsal = 0;
    for (int i = 0; i < a.nseg; ++i) nsal += a.seg_kind[i] >= HEAD_SAL_LOGIT && a.seg_kind[i] <= HEAD_SAL_MSE;
    if (nsal) {                                // the saliency kinds: every segment, one model, no fp8 copies, dpre required
        if (nsal != a.nseg || a.models > 1 || a.q8_slot || !a.dpre) return -3;
        if (kp == KWIDE) {
            if (bf16) MRGAN_LAUNCH((head_kernel<__bf16, false, KWIDE, true>), grid, dim3(256), smem, s, a);
            else MRGAN_LAUNCH((head_kernel<float, false, KWIDE, true>), grid, dim3(256), smem, s, a);
        } else {
            if (bf16) MRGAN_LAUNCH((head_kernel<__bf16, false, KMAX, true>), grid, dim3(256), smem, s, a);
            else MRGAN_LAUNCH((head_kernel<float, false, KMAX, true>), grid, dim3(256), smem, s, a);
        }
        RET_LAUNCH;
    }
    if (kp == KWIDE) {
        if (a.q8_slot) return -3;              // the e5m2 packing epilogue exists at the 8-class pitch only
        if (bf16) MRGAN_LAUNCH((head_kernel<__bf16, false, KWIDE>), grid, dim3(256), smem, s, a);
        else MRGAN_LAUNCH((head_kernel<float, false, KWIDE>), grid, dim3(256), smem, s, a);
    } else if (a.q8_slot) {
        if (!bf16 || !(a.q8 || a.q8t)) return -3;
        static DeviceOnce attr;
        if (attr.first()) {
            if (hipFuncSetAttribute((const void*)head_kernel<__bf16, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) return -2;
            attr.mark();
        }
        MRGAN_LAUNCH((head_kernel<__bf16, true>), grid, dim3(256), smem, s, a);
    } else {
        LAUNCH_T(head_kernel, grid, dim3(256), smem, s, a);
    }
    RET_LAUNCH;
}

int launch_path_stage(int bf16, const PathStageArgs& a, hipStream_t s) {
    if (a.rows <= 0) return 0;
    if (!a.src || !a.out || a.cols <= 0 || a.cols > a.cols_pad || (a.cols_pad % 8) != 0 || a.ldo < a.cols_pad || (a.ldo % 8) != 0 || a.ld < a.cols)
        return -3;
    LAUNCH_T(path_stage_kernel, dim3(ceil_div(a.cols_pad, 2048), a.rows), dim3(256), 0, s, a);
    RET_LAUNCH;
}

int launch_attr_accum(int bf16, const AttrAccumArgs& a, hipStream_t s) {
    if (a.rows <= 0) return 0;
    if ((a.mode != SAL_RAW && a.mode != SAL_HEATMAP) || a.cols <= 0 || a.cols > a.ldg || (a.ldg % 8) != 0 || a.ldo < a.cols) return -3;
    if (a.draws < 1 || a.draw < 0 || a.draw >= a.draws || !a.g || !a.out) return -3;
    if (a.multiply && (!a.x || a.ld_x < a.cols)) return -3;
    LAUNCH_T(attribution_accum_kernel, dim3(a.rows), dim3(256), 0, s, a);
    RET_LAUNCH;
}

int launch_recon_head(int bf16, const ReconHeadArgs& a, hipStream_t s) {
    if (a.rows <= 0) return 0;
    if (!a.y || !a.x || !a.loss_part || a.cols <= 0 || a.cols > a.cols_pad || (a.cols_pad % CB) != 0 || a.ldy < a.cols_pad || (a.ldy % 8) != 0 ||
        a.ld_x < a.cols || a.rows_valid < 0 || a.rows_valid > a.rows || (a.stream && !a.st))
        return -3;
    // the training form writes whole blocks of dY and one column-sum row per block
    if (a.dy && ((a.rows % RB) != 0 || a.ldd < a.cols_pad || (a.ldd % 8) != 0)) return -3;
    if (a.cs && (!a.dy || a.ldcs < a.cols_pad)) return -3;
    LAUNCH_T(recon_head_kernel, dim3(a.cols_pad / CB, ceil_div(a.rows, RB)), dim3(256), 0, s, a);
    RET_LAUNCH;
}

int launch_fold_loss(const float* part, int n, float* acc, int first, hipStream_t s) {
    if (!part || !acc || n < 0) return -3;
    MRGAN_LAUNCH(fold_loss_kernel, dim3(1), dim3(256), 0, s, part, n, acc, first);
    RET_LAUNCH;
}

int launch_cast_rows(int bf16, const void* src, int lds, int rows, int cols, float* dst, long ldd, hipStream_t s) {
    if (rows <= 0) return 0;
    if (!src || !dst || cols <= 0 || cols > lds || (lds % 8) != 0 || ldd < cols) return -3;
    for (int r0 = 0; r0 < rows; r0 += 32768) {             // (grid.y stays below its limit of 65535)
        const dim3 grid(ceil_div(cols, 2048), std::min(32768, rows - r0));
        if (bf16) MRGAN_LAUNCH(cast_rows_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)src + (long)r0 * lds, lds, cols, dst + (long)r0 * ldd, ldd);
        else MRGAN_LAUNCH(cast_rows_kernel<float>, grid, dim3(256), 0, s, (const float*)src + (long)r0 * lds, lds, cols, dst + (long)r0 * ldd, ldd);
    }
    RET_LAUNCH;
}

int launch_reduce_partials(const float* src, int nsrc, long stride, int n, int ngroups, float* dst, hipStream_t s, int models,
                           long model_stride) {
    MRGAN_LAUNCH(reduce_partials_kernel, dim3(ceil_div(n, 256), ngroups, std::max(1, models)), dim3(256), 0, s, src, nsrc, stride, n, ngroups,
                 dst, model_stride);
    RET_LAUNCH;
}

int launch_fm(int bf16, const FmArgs& a, hipStream_t s) {
    if ((a.feat % 8) != 0) return -3;
    if (a.models > 1 && a.q8_slot) return -3;      // model groups: without fp8 copies
    // every block first folds the column partial sums of its 64 columns (all row tiles): with a wide feature layer that
    // prologue would be repeated by thousands of 64-row blocks (0.34 ms at 4096 features x 8192 rows), so blocks take more rows
    // once ~512 of them exist
    FmArgs b = a;
    const int gx = ceil_div(a.feat, CB);
    b.rb = std::max(RB, (int)round_up(ceil_div(a.rows, std::max(1, 512 / gx)), 32));
    const bool dist = gx >= 16 && a.lscratch && a.lcount;
    if (!dist) { b.lscratch = nullptr; b.lcount = nullptr; }
    dim3 grid(gx, ceil_div(a.rows, b.rb) + (dist ? 0 : 1), std::max(1, a.models));      // + the loss block row of the narrow form
    LAUNCH_T(fm_kernel, grid, dim3(256), 0, s, b);
    RET_LAUNCH;
}

int launch_colsum_finalize(const float* part1, const float* part2, int npart, int ld, int n, float* out, hipStream_t s, int nseg) {
    if (n % 4) return -3;
    MRGAN_LAUNCH(colsum_finalize_kernel, dim3(ceil_div(n, CB), 2, nseg), dim3(256), 0, s, part1, part2, npart, ld, n, out, (long)npart * ld);
    RET_LAUNCH;
}

int launch_adam(const AdamArgs& a, hipStream_t s) {
    if (a.models > 1 && a.mode != ADAM_FUSED) return -3;      // model groups: the fused update only
    MRGAN_LAUNCH(adam_kernel, dim3(a.ntiles + 1, std::max(1, a.models)), dim3(256), 0, s, a);
    RET_LAUNCH;
}

int launch_noise_debug(int gauss, uint64_t seed, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0, int rows, int cols,
                       float* out, hipStream_t s) {
    MRGAN_LAUNCH(noise_debug_kernel, dim3(ceil_div(cols, 32), ceil_div(rows, 32)), dim3(64), 0, s, gauss, seed, site, seg,
                       step, row0, rows, cols, out);
    RET_LAUNCH;
}

}  // namespace mrgan
