// bf16-in / fp32-accumulate MFMA GEMMs (v_mfma_f32_32x32x16_bf16) for gfx950.
//
// Kernels, by where the reduction index lives in memory:
//   KC  ("k contiguous"): A[i][k], Bt[j][k] both have the reduction index innermost.
//        forward  Y = X Wt^T   (A = activations [M][K], Bt = transposed bf16 weight copy [N][K])
//        dX       dX = dY W^T  (A = dY [M][N], Bt = bf16 weight copy W [K][N]; reduction over N)
//        fragments are 16-B ds_read_b128 from an XOR-swizzled [row][64 k] image.
//   KS  ("k strided"): A[k][i], B[k][j] have the reduction index outermost.
//        dW = X^T dY (reduction over the batch rows): both operands are row-major activations, so the
//        MFMA fragments (8 consecutive k for one row/col) are gathered with the hardware transposing
//        LDS read ds_read_b64_tr_b16 from a [k][free] image.
//
// Staging is LDS-DMA into an XOR-swizzled LDS ring, one raw s_barrier per k-tile, persistent blocks in XCD-aware tile
// order: the scheme, its helpers, the tile order and the ring main loop of both LDS-DMA kernels are lds_ring.h's.
//
// KC: the block tiles and the measured table that picks one are listed in one place, above launch_kc_tile.
// KS: 128 x 128 x 64 blocks of 8 waves (64x32 each).
// The weight-gradient product over ragged segments (batch not a multiple of 128) keeps a register-staged
// kernel that can zero-fill arbitrary reduction rows.
#include <algorithm>
#include <cstring>
#include <string>

#include "gemm.h"
#include "lds_ring.h"

namespace mrgan {

namespace {
constexpr int BN = 128, BK = RING_BK;
constexpr int KS_PITCH = 320;                   // register-staged KS image: 256 data + 64 pad bytes per k-row
constexpr int KS_TILE_BYTES = 64 * KS_PITCH;

// =====================================================================================================
// KC: forward and input-gradient products
// =====================================================================================================
// Block tile BM x BNT, WM x WN waves (each (BM/WM) x (BNT/WN), as MR x NR accumulators of 32x32), NS-stage ring.
// LDS-DMA issue is the scarce resource of this loop (~60-100 issue cycles per 1 KiB wave-instruction), so the
// achievable MFMA share grows with the tile's arithmetic intensity BM*BNT/(BM+BNT): 64x128 -> 43, 128x128 -> 64,
// 256x256 -> 128 flop per staged byte.
#ifdef MRGAN_STAMPS
struct KcStamps { unsigned long long acc[6], prev, epi[5]; };      // make STAMPS=1: cycles per phase, summed over the block's tiles
#define KC_STAMPS_PARAM , KcStamps& stamps_
#define KC_STAMPS_ARG , stamps_
#else
#define KC_STAMPS_PARAM
#define KC_STAMPS_ARG
#endif
// one output tile (batch, tile_m, tile_n) of the product described by g: prologue, main loop, epilogue, ending with
// the barrier after which the LDS ring may be refilled
template <int EPI, int BM, int BNT, int WM, int WN, int NS, int VAR>
__device__ __forceinline__ void kc_tile(const GemmArgs& g, const int batch /* segment */, const int model, const int tile_m, const int tile_n, char* lds KC_STAMPS_PARAM) {
    constexpr int NW = WM * WN;
    constexpr int MR = BM / WM / 32, NR = BNT / WN / 32;   // 32x32 accumulators per wave
    constexpr int A_BYTES = BM * 128, B_BYTES = BNT * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BNT / 8 / NW;   // wave-instructions per wave per k-tile (8 rows each)
    static_assert(MR >= 1 && NR >= 1 && A_INSTR >= 1 && B_INSTR >= 1 && BM % (8 * NW) == 0 && BNT % (8 * NW) == 0, "tile/wave layout");
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane >> 3, lp = lane & 7;
    const int lr = lane & 31, lh = lane >> 5;
    const int nk = (g.e.ablate & 4) ? 0 : g.K / BK;
#ifdef MRGAN_STAMPS
#define STAMP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); stamps_.acc[i] += n_ - stamps_.prev; stamps_.prev = n_; } while (0)
#else
#define STAMP(i)
#endif
    {
        const int row_blk = tile_m * BM, col_blk = tile_n * BNT;

        // descriptors bounded at the operand's end: rows >= M (A) / >= N (Bt) read as zeros
        const __bf16* Ab = model_ptr((const __bf16*)g.A, g.e, model) + (long)batch * g.a_bs;
        const __bf16* Bb = model_ptr((const __bf16*)g.B, g.e, model) + (long)batch * g.b_bs;
        const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)Ab, 0, (int)((long)g.M * g.a_si * 2), 0x00020000);
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Bb, 0, (int)((long)g.N * g.b_sj * 2), 0x00020000);
        int voffA[A_INSTR], voffB[B_INSTR];          // swizzled per-lane source offsets
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const int R = (wave * A_INSTR + i) * 8 + lrow;
            voffA[i] = (int)(((long)(row_blk + R) * g.a_si + ((lp ^ ((R >> 1) & 7)) << 3)) * 2);
        }
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i) {
            const int R = (wave * B_INSTR + i) * 8 + lrow;
            voffB[i] = (int)(((long)(col_blk + R) * g.b_sj + ((lp ^ ((R >> 1) & 7)) << 3)) * 2);
        }
        auto issue = [&](int k0, int buf) {
            char* a_dst = lds + buf * STAGE + wave * A_INSTR * 1024;
            char* b_dst = lds + buf * STAGE + A_BYTES + wave * B_INSTR * 1024;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i) glds16(rsA, a_dst + i * 1024, voffA[i], k0 * 2);
#pragma unroll
            for (int i = 0; i < B_INSTR; ++i) glds16(rsB, b_dst + i * 1024, voffB[i], k0 * 2);
        };

#pragma unroll
        for (int p = 0; p < NS - 1; ++p)
            if (p < nk) issue(p * BK, p);


        // DX epilogues that read e.h element-wise (softplus derivative, xhat sums: one column per lane, rows strided)
        // get the block's tile of h copied into LDS behind the ring with 16-byte LDS-DMA loads; it lands under the main
        // loop (the loads are older than every k-tile group issued inside the loop, so the counted waits cover them)
        const __bf16* htile = nullptr;
        if constexpr (EPI == EPI_DX && (VAR & VAR_ACT_MASK) != ACT_RELU) {
            if (dx_needs_h<VAR>(g.e)) {
                constexpr int OUTB = BM * BNT * 2 + 4 * WM * BNT * 4, RING = NS * STAGE;
                char* hdst = lds + (RING > OUTB ? RING : OUTB);
                const __bf16* hb = model_ptr((const __bf16*)g.e.h, g.e, model) + (long)batch * g.e.h_bs;
                const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc((void*)hb, 0, (int)((long)g.M * g.e.ldh * 2), 0x00020000);
                constexpr int RPI = 1024 / (BNT * 2);              // tile rows per wave-instruction
                constexpr int LPR = 64 / RPI;                      // lanes per row
                constexpr int HI = BM / RPI / NW;                  // wave-instructions per wave
#pragma unroll
                for (int i = 0; i < HI; ++i) {
                    const int R = (wave * HI + i) * RPI + lane / LPR;
                    const int voff = (int)(((long)(row_blk + R) * g.e.ldh + col_blk) * 2) + (lane % LPR) * 16;
                    glds16(rsH, hdst + (wave * HI + i) * 1024, voff, 0);
                }
                htile = (const __bf16*)hdst;
            }
        }

        f32x16 acc[MR][NR];
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // bias / relu-mask words of this wave's sub-tiles: their global-load latency hides under the main loop.
        // (issued after the LDS-DMA groups so that the counted waits below still cover every DMA group)
        EpiPrefetch<MR, NR> pf;
        epilogue_prefetch<__bf16, EPI, MR, NR, VAR>(pf, g, batch, model, row_blk, col_blk, wm, wn, lane);

#define KC_FRAG_A(As, mi, ks) *(const bf16x8*)(As + kc_off((wm * MR + mi) * 32 + lr, (ks) * 2 + lh))
#define KC_FRAG_B(Bs, ni, ks) *(const bf16x8*)(Bs + kc_off((wn * NR + ni) * 32 + lr, (ks) * 2 + lh))
        RING_MAINLOOP(NS, A_INSTR + B_INSTR, MR, NR, nk, acc, issue, 0, KC_FRAG_A, KC_FRAG_B, lds, STAGE, A_BYTES, STAMP)
#undef KC_FRAG_A
#undef KC_FRAG_B
        STAMP(2);               // main loop
        __syncthreads();
        STAMP(3);               // barrier after the main loop
        // the BM x BNT bf16 output tile is assembled at the start of the (now dead) ring, column-sum scratch behind it
        epilogue<__bf16, EPI, MR, NR, WM, true, VAR>(acc, g, batch, model, 0, tile_m, row_blk, col_blk, wm, wn, lane,
                                                     (float*)(lds + BM * BNT * 2), BNT, (__bf16*)lds, &pf, htile
#ifdef MRGAN_STAMPS
                                                     , stamps_.epi
#endif
                                                     );
        STAMP(4);               // epilogue (math, staging, copy-out issue, column sums)
        __syncthreads();        // the copy-out has read the staged tile: the ring may be refilled
        STAMP(5);
    }
#undef STAMP
}

// Persistent block: walks the tiles bid, bid + grid, ...  One tile's output stores drain while the next tile's
// loads and MFMAs run, and co-resident blocks drift out of phase instead of all hitting HBM at once.
template <int EPI, int BM, int BNT, int WM, int WN, int NS, int VAR>
__global__ __launch_bounds__(64 * WM * WN) void gemm_bf16_kc_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char lds[];        // max(NS * STAGE, BM * BNT * 2 + scratch) bytes
    const int ntn = (g.N + BNT - 1) / BNT, ntm = (g.M + BM - 1) / BM;
    const int ntiles = ntn * ntm * g.nbatch;
#ifdef MRGAN_STAMPS
    KcStamps stamps_ = {{0, 0, 0, 0, 0, 0}, __builtin_amdgcn_s_memtime(), {0, 0, 0, 0, 0}};
#endif
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int tidx = xcd_tile(tl, ntiles);
        const int bidx = tidx / (ntn * ntm), rem = tidx - bidx * (ntn * ntm);
        const int model = batch_model(g.e, bidx), batch = batch_segment(g.e, bidx, model);      // (model groups: gemm.h, Epi::segs)
        // large problems only (operands beyond an XCD's L2): patches of 4 tile rows (lds_ring.h, tile order)
        int tile_m, tile_n;
        if ((ntm & 3) == 0 && ntn >= 8 && g.K >= 2048) {
            const int grp = rem / (4 * ntn), in = rem - grp * (4 * ntn);
            tile_m = grp * 4 + (in & 3); tile_n = in >> 2;
        } else { tile_m = rem / ntn; tile_n = rem - tile_m * ntn; }
        kc_tile<EPI, BM, BNT, WM, WN, NS, VAR>(g, batch, model, tile_m, tile_n, lds KC_STAMPS_ARG);
    }
#ifdef MRGAN_STAMPS
    if (g.e.slab && threadIdx.x == 0)
    {
        for (int i = 0; i < 6; ++i) ((unsigned long long*)g.e.slab)[(long)blockIdx.x * 12 + i] = stamps_.acc[i];
        for (int i = 0; i < 4; ++i) ((unsigned long long*)g.e.slab)[(long)blockIdx.x * 12 + 6 + i] = stamps_.epi[i];
    }
#endif
}

thread_local const char* g_last_kernel = "";

template <int EPI, int BM, int BNT, int WM, int WN, int NS, int VAR>
int launch_kc(const GemmArgs& g, hipStream_t s) {
    static const std::string name = "gemm_bf16_kc_kernel<" + std::to_string(EPI) + ", " + std::to_string(BM) + ", " +
                                    std::to_string(BNT) + ", " + std::to_string(WM) + ", " + std::to_string(WN) + ", " +
                                    std::to_string(NS) + ", " + std::to_string(VAR) + ">";
    g_last_kernel = name.c_str();
    constexpr int STAGE = BM * 128 + BNT * 128;
    // staged output tile + column-sum scratch (+ the tile of e.h for the DX epilogues that read it)
    constexpr int OUT = BM * BNT * 2 + 4 * WM * BNT * 4;
    constexpr int LDS = (NS * STAGE > OUT ? NS * STAGE : OUT) + ((EPI == EPI_DX && (VAR & VAR_ACT_MASK) != ACT_RELU) ? BM * BNT * 2 : 0);
    const int tiles = ceil_div(g.M, BM) * ceil_div(g.N, BNT) * g.nbatch;
    return launch_with_dyn_lds<gemm_bf16_kc_kernel<EPI, BM, BNT, WM, WN, NS, VAR>, LDS>(dim3(persistent_grid(tiles, LDS)), dim3(64 * WM * WN), s, g);
}

// =====================================================================================================
// KS: weight-gradient product, LDS-DMA version (reduction rows contiguous and a multiple of 64)
// LDS image [64 k][128 free] bf16 with 256-B rows; 16-B chunk c of k-row kr sits at chunk c ^ ((kr&3)<<2),
// which makes the four k-rows x two 32-B column blocks that a 32-lane half of ds_read_b64_tr_b16 touches
// hit eight distinct 32-B bank groups.
// =====================================================================================================
__device__ __forceinline__ bf16x8 ks_frag_swz(const char* tile, int fb, int ks, int lane) {
    const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    const int f0 = fb + (g4 & 1) * 16;
    const int m0 = ks * 16 + (g4 >> 1) * 8;                        // multiple of 8: (m0 + q) & 3 == q
    const char* a0 = tile + (m0 + q) * 256 + ((((f0 >> 3) + (p >> 1)) ^ (q << 2)) << 4) + ((p & 1) << 3);
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * 256));
    const s16x8 tt = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, tt);
}

template <int NS, int WM, int WN>
__device__ __forceinline__ void ks_fast_body(const GemmArgs& g, const int bid, const int model /* model groups: blockIdx.y */) {
    constexpr int NW = WM * WN;
    constexpr int MR = 128 / WM / 32, NR = 128 / WN / 32;
    constexpr int T_BYTES = 64 * 256, STAGE = 2 * T_BYTES;
    constexpr int T_INSTR = 16 / NW;                    // wave-instructions per wave per operand tile (4 k-rows x 256 B each)
    static_assert(MR >= 1 && NR >= 1 && T_INSTR >= 1, "tile/wave layout");
    extern __shared__ __attribute__((aligned(16))) char lds[];        // NS * STAGE bytes

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int ntn = (g.N + 127) / 128, ntm = (g.M + 127) / 128;
    const int tidx = xcd_tile(bid, ntn * ntm * g.splits);
    const int split = tidx / (ntn * ntm), rem = tidx - split * (ntn * ntm);
    // wide layers only: patches of 8 tile rows for the 64 resident blocks of an XCD (lds_ring.h, tile order)
    int tile_m, tile_n;
    if ((ntm & 7) == 0 && ntn >= 16) {
        const int grp = rem / (8 * ntn), in = rem - grp * (8 * ntn);
        tile_m = grp * 8 + (in & 7); tile_n = in >> 3;
    } else { tile_m = rem / ntn; tile_n = rem - tile_m * ntn; }
    const int row_blk = tile_m * 128, col_blk = tile_n * 128;
    const int k_begin = split * g.kchunk;
    const int k_end = (g.e.ablate & 4) ? k_begin : min(g.K, k_begin + g.kchunk);

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)model_ptr(g.A, g.e, model), 0, (int)((long)g.K * g.a_sk * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)model_ptr(g.B, g.e, model), 0, (int)((long)g.K * g.b_sk * 2), 0x00020000);
    // a wave-instruction covers 4 k-rows x 256 B; lane -> (k-row, swizzled source chunk)
    const int lrow = lane >> 4, lp = lane & 15;
    int voffA[T_INSTR], voffB[T_INSTR];
#pragma unroll
    for (int i = 0; i < T_INSTR; ++i) {
        const int kr = (wave * T_INSTR + i) * 4 + lrow;
        const int c = lp ^ ((kr & 3) << 2);
        voffA[i] = (int)(((long)kr * g.a_sk + row_blk + c * 8) * 2);
        voffB[i] = (int)(((long)kr * g.b_sk + col_blk + c * 8) * 2);
    }
    auto issue = [&](int k0, int buf) {
        char* a_dst = lds + buf * STAGE + wave * T_INSTR * 1024;
        char* b_dst = a_dst + T_BYTES;
#pragma unroll
        for (int i = 0; i < T_INSTR; ++i) glds16(rsA, a_dst + i * 1024, voffA[i], (int)((long)k0 * g.a_sk * 2));
#pragma unroll
        for (int i = 0; i < T_INSTR; ++i) glds16(rsB, b_dst + i * 1024, voffB[i], (int)((long)k0 * g.b_sk * 2));
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (k_end - k_begin + BK - 1) / BK;
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nk) issue(k_begin + p * BK, p);
#define KS_FRAG_A(As, mi, ks) ks_frag_swz(As, (wm * MR + mi) * 32, ks, lane)
#define KS_FRAG_B(Bs, ni, ks) ks_frag_swz(Bs, (wn * NR + ni) * 32, ks, lane)
#define KS_NO_STAMP(i)
    RING_MAINLOOP(NS, 2 * T_INSTR, MR, NR, nk, acc, issue, k_begin, KS_FRAG_A, KS_FRAG_B, lds, STAGE, T_BYTES, KS_NO_STAMP)
#undef KS_FRAG_A
#undef KS_FRAG_B
#undef KS_NO_STAMP
    __syncthreads();
    epilogue<__bf16, EPI_SLAB, MR, NR, WM>(acc, g, 0, model, split, tile_m, row_blk, col_blk, wm, wn, lane, (float*)lds, BN);
}

template <int NS, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void gemm_bf16_ks_fast_kernel(const GemmArgs g) {
    ks_fast_body<NS, WM, WN>(g, blockIdx.x, blockIdx.y);
}

// All weight-gradient products of one sub-step in ONE launch: they have no consumer before the Adam kernel, each is
// small (32 .. 256 blocks, 5-7 us of launch + drain per launch for 3-12 us of work), and together they fill the chip.
// Block b works on problem i with blk_end[i-1] <= b < blk_end[i].  Blocks whose index inside the problem agrees mod 8
// still share an XCD (a constant rotation of b % 8), which is all the XCD-aware tile order of ks_fast_body relies on.
template <int NS, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void gemm_bf16_ks_group_kernel(const KsGroup grp) {
    const int ngemm = grp.blk_end[grp.n - 1];
    if ((int)blockIdx.x >= ngemm) {
        // the fold job's blocks (see FoldJob): only the first 256 threads of a block take part
        const FoldJob& f = grp.fold;
        const float* fsrc = (const float*)((const char*)f.src + (long)blockIdx.y * f.model_stride);      // (model groups: this model's partial rows)
        float* fdst = (float*)((char*)f.dst + (long)blockIdx.y * f.model_stride);
        const int fb = (int)blockIdx.x - ngemm, gidx = fb / f.blocks_x;
        const int i = (fb - gidx * f.blocks_x) * 256 + (int)threadIdx.x;
        if (threadIdx.x >= 256 || i >= f.n) return;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int p = gidx;
        for (; p + 3 * f.ngroups < f.nsrc; p += 4 * f.ngroups) {
            s0 += fsrc[(long)p * f.stride + i]; s1 += fsrc[(long)(p + f.ngroups) * f.stride + i];
            s2 += fsrc[(long)(p + 2 * f.ngroups) * f.stride + i]; s3 += fsrc[(long)(p + 3 * f.ngroups) * f.stride + i];
        }
        for (; p < f.nsrc; p += f.ngroups) s0 += fsrc[(long)p * f.stride + i];
        fdst[(long)gidx * f.stride + i] = (s0 + s1) + (s2 + s3);
        return;
    }
    int i = 0, b0 = 0;
#pragma unroll
    for (int j = 0; j < KS_GROUP_MAX - 1; ++j)
        if (j + 1 < grp.n && (int)blockIdx.x >= grp.blk_end[j]) { i = j + 1; b0 = grp.blk_end[j]; }
    ks_fast_body<NS, WM, WN>(grp.g[i], (int)blockIdx.x - b0, blockIdx.y);
}

template <int NS, int WM, int WN>
int launch_ks_fast(const GemmArgs& g, hipStream_t s) {
    static const std::string name = "gemm_bf16_ks_fast_kernel<" + std::to_string(NS) + ", " + std::to_string(WM) + ", " + std::to_string(WN) + ">";
    g_last_kernel = name.c_str();
    constexpr int STAGE = 2 * 64 * 256;
    dim3 grid(ceil_div(g.N, 128) * ceil_div(g.M, 128) * g.splits, gemm_models(g));
    return launch_with_dyn_lds<gemm_bf16_ks_fast_kernel<NS, WM, WN>, NS * STAGE>(grid, dim3(64 * WM * WN), s, g);
}

// =====================================================================================================
// KS, register-staged: handles reduction ranges with holes (segments of a batch that is not a multiple
// of 128) by zero-filling rows per lane.  LDS image [64 k][128 free] with a 320-B pitch.
// =====================================================================================================
__device__ __forceinline__ bf16x8 ks_frag(const char* tile, int fb, int ks, int lane) {
    const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    const int f0 = fb + (g4 & 1) * 16;
    const int m0 = ks * 16 + (g4 >> 1) * 8;
    const char* a0 = tile + (m0 + q) * KS_PITCH + (f0 + 4 * p) * 2;
    // (the v4i16 form: per-element use of the v4bf16 form's result is mis-folded by hipcc 7.2)
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * KS_PITCH));
    const s16x8 tt = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, tt);
}

__global__ __launch_bounds__(256) void gemm_bf16_ks_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) char lds[2 * KS_TILE_BYTES];
    char* As = lds;
    char* Bs = lds + KS_TILE_BYTES;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x, tile_m = blockIdx.y;
    const int bidx = blockIdx.z / g.splits, split = blockIdx.z % g.splits;
    const int model = batch_model(g.e, bidx), batch = batch_segment(g.e, bidx, model);      // (model groups: gemm.h, Epi::segs)
    const int row_blk = tile_m * 128, col_blk = tile_n * BN;
    const int k_begin = split * g.kchunk;
    const int k_end = (g.e.ablate & 4) ? k_begin : min(g.K, k_begin + g.kchunk);

    const __bf16* A = model_ptr((const __bf16*)g.A, g.e, model) + (long)batch * g.a_bs;
    const __bf16* B = model_ptr((const __bf16*)g.B, g.e, model) + (long)batch * g.b_bs;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    u32x4 ra[4], rb[4];
    auto load_tile = [&](int k0) {
        const int kloc = k0 % g.seg_stride;             // BK divides seg_stride: a tile never straddles segments
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cidx = t + 256 * u, kr = cidx >> 4, c = cidx & 15;
            const u32x4 z = {0u, 0u, 0u, 0u};
            const bool kok = (k0 + kr) < k_end && (kloc + kr) < g.seg_rows;
            ra[u] = (kok && row_blk + c * 8 < g.M) ? *(const u32x4*)(A + (long)(k0 + kr) * g.a_sk + row_blk + c * 8) : z;
            rb[u] = (kok && col_blk + c * 8 < g.N) ? *(const u32x4*)(B + (long)(k0 + kr) * g.b_sk + col_blk + c * 8) : z;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cidx = t + 256 * u, kr = cidx >> 4, c = cidx & 15;
            *(u32x4*)(As + kr * KS_PITCH + c * 16) = ra[u];
            *(u32x4*)(Bs + kr * KS_PITCH + c * 16) = rb[u];
        }
    };

    if (k_begin < k_end) {
        load_tile(k_begin);
        for (int k0 = k_begin; k0 < k_end; k0 += BK) {
            __syncthreads();
            store_tile();
            __syncthreads();
            if (k0 + BK < k_end) load_tile(k0 + BK);
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                bf16x8 a[2], b[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) a[mi] = ks_frag(As, (wm * 2 + mi) * 32, ks, lane);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) b[ni] = ks_frag(Bs, (wn * 2 + ni) * 32, ks, lane);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    }
    __syncthreads();
    epilogue<__bf16, EPI_SLAB, 2, 2, 2>(acc, g, batch, model, split, tile_m, row_blk, col_blk, wm, wn, lane, (float*)lds, BN);
}

// diagnostic: out[0..511]  = what ds_read_b64_tr_b16 returns when lane l supplies the address of u16 elements
//                            4l..4l+3 of a linear image whose element i holds the value i;
//             out[512..1023] = ks_frag() on a [16][160] image whose element (row, col) holds row<<8 | col.
__global__ void tr_probe_kernel(unsigned short* out) {
    __shared__ __attribute__((aligned(16))) unsigned short img[16 * 160];
    const int l = threadIdx.x;
    for (int i = l; i < 16 * 160; i += 64) img[i] = (unsigned short)i;
    __syncthreads();
    const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)((const char*)img + l * 8));
    for (int j = 0; j < 4; ++j) out[l * 8 + j] = (unsigned short)t[j];
    for (int j = 4; j < 8; ++j) out[l * 8 + j] = 0;
    __syncthreads();
    for (int i = l; i < 16 * 160; i += 64) img[i] = (unsigned short)(((i / 160) << 8) | (i % 160));
    __syncthreads();
    const s16x8 f = __builtin_bit_cast(s16x8, ks_frag((const char*)img, 0, 0, l));
    for (int j = 0; j < 8; ++j) out[512 + l * 8 + j] = (unsigned short)f[j];
}
}  // namespace

// epilogue variants compiled for the bf16 path (anything else is a host-side error)
// Block tiles (BM x BN, waves, LDS ring stages), by config number:
//   0 = 64x128, 4 waves of 32x64, 3 stages      1 = 128x128, 4 waves of 64x64, 2 stages   3 = 256x256, 8 waves of 128x64, 2 stages
//   5 = 64x128, 4 waves, 2 stages (three blocks per CU)   7 = 128x128, 8 waves of 64x32, 2 stages   9 = 64x64, 4 waves of 32x32, 3 stages
// The default (-1) picks one by the measured table below; mrgan_set_tuning(MRGAN_TUNE_KC_CFG) forces one (kc_cfg_supported).
// Shape fallbacks apply to both: 3 / 5 / 7 need N % 128 == 0 (else 0), 3 needs N % 256 == 0 (else 1), and the DX epilogues
// that stage a tile of e.h in LDS only exist for 0, 1 and 9 (3 / 5 / 7 become 1).
template <int EPI, int VAR>
static int launch_kc_tile(const GemmArgs& g, hipStream_t s) {
    int cfg = g.e.tune_kc_cfg;
    if (cfg < 0) {
        // measured on MI355X (scripts/gemm_bench.py): bigger tiles win once they still give >= ~1.5 blocks per CU
        // (a model group counts the tiles of ONE model, so it takes the tile a single model's launch takes: the same kernels and,
        //  element by element, the same sums; tiles for whole groups have not been measured)
        const int nbm = gemm_model_batches(g);
        const int t128 = ceil_div(g.M, 128) * ceil_div(g.N, 128) * nbm;
        const int t256 = ceil_div(g.M, 256) * ceil_div(g.N, 256) * nbm;
        // 128 x 128 tiles as EIGHT waves of 64 x 32 (cfg 7; two blocks = 16 waves per CU): more waves hide the barrier -> LDS read ->
        // MFMA chain of the short k-loops better than four waves of 64 x 64 (cfg 1) although they read 1.5 instead of 1.0
        // fragments per MFMA: D1 forward over 3 segments 22.9 -> 21.3 us, dX through D2 20.3 -> 18.7 us (scripts/gemm_bench.py)
        cfg = t128 >= 384 ? 7 : 0;
        // long reductions with enough 256x256 tiles to fill the chip (the wide stack of BASELINE configs[4]: K = N = 4096):
        // 128 flop per staged byte instead of 64 -- 1.37 vs 0.95 PFLOP/s measured at 24576 x 4096 x 4096 (scripts/fp8_bench.py)
        if (g.K >= 2048 && t256 >= 256 && (g.N % 256) == 0) cfg = 3;
        // long reductions into a narrow output (D2 forward: K = 1024, N = 512): three 64x128 blocks per CU with a
        // 2-stage ring hide the k-loop latency better than two 128x128 blocks (20.7 vs 21.7 us)
        if (EPI == EPI_FWD && cfg == 7 && g.K >= 1024 && g.K < 2048 && g.N <= 512) cfg = 5;
        // ... and with exactly one 128x128 tile per CU (D2 forward over the two segments of the G sub-step) the 8-wave tile
        // beats two 64x128 blocks per CU: 13.9 vs 15.0 us (scripts/gemm_bench.py, KC_CFG sweep)
        if (EPI == EPI_FWD && cfg == 0 && g.K >= 1024 && g.K < 2048 && t128 >= 256 && (g.N % 128) == 0) cfg = 7;
        // launches with at most one 64x128 tile per CU (the one-segment products of the G sub-step, small batches): 64x64 tiles
        // put twice as many blocks on the chip -- dX through D1 11.5 -> 9.7 us, d(BatchNorm output) 11.0 -> 8.5, G2 forward of one
        // segment 8.6 -> 7.4; with two tiles per CU already (two-segment launches) the smaller tile loses (10.5 -> 12.4)
        if (cfg == 0 && ceil_div(g.M, 64) * ceil_div(g.N, 128) * nbm <= 256) cfg = 9;
    }
    if (cfg >= 2 && cfg != 9 && (g.N % 128) != 0) cfg = 0;
    if (cfg == 3 && (g.N % 256) != 0) cfg = 1;
    constexpr bool H_TILE = EPI == EPI_DX && (VAR & VAR_ACT_MASK) != ACT_RELU;
    if (H_TILE && cfg >= 2 && cfg != 9) cfg = 1;
    if constexpr (!H_TILE) {
        if (cfg == 7) return launch_kc<EPI, 128, 128, 2, 4, 2, VAR>(g, s);
        if (cfg == 3) return launch_kc<EPI, 256, 256, 2, 4, 2, VAR>(g, s);
    }
    if (cfg == 9) return launch_kc<EPI, 64, 64, 2, 2, 3, VAR>(g, s);       // 48 KiB ring: three blocks per CU
    if (cfg == 1) return launch_kc<EPI, 128, 128, 2, 2, 2, VAR>(g, s);
    if (cfg == 5) return launch_kc<EPI, 64, 128, 2, 2, 2, VAR>(g, s);      // 48 KiB ring: three blocks per CU
    return launch_kc<EPI, 64, 128, 2, 2, 3, VAR>(g, s);
}

static int launch_kc_any(int epi, const GemmArgs& g, hipStream_t s) {
    const int var = epi_variant(epi, g.e);
    if (epi == EPI_FWD) {
        switch (var) {
            // (the true-Gaussian variants exist beside the noisy ones only: every other instantiation is the default build's)
            case ACT_RELU | VAR_NOISE | VAR_MASK | VAR_GAUSS: return launch_kc_tile<EPI_FWD, ACT_RELU | VAR_NOISE | VAR_MASK | VAR_GAUSS>(g, s);
            case ACT_LINEAR | VAR_NOISE | VAR_GAUSS: return launch_kc_tile<EPI_FWD, ACT_LINEAR | VAR_NOISE | VAR_GAUSS>(g, s);
            case ACT_RELU | VAR_NOISE | VAR_MASK: return launch_kc_tile<EPI_FWD, ACT_RELU | VAR_NOISE | VAR_MASK>(g, s);
            case ACT_RELU | VAR_MASK: return launch_kc_tile<EPI_FWD, ACT_RELU | VAR_MASK>(g, s);
            case ACT_RELU: return launch_kc_tile<EPI_FWD, ACT_RELU>(g, s);
            case ACT_LINEAR | VAR_NOISE: return launch_kc_tile<EPI_FWD, ACT_LINEAR | VAR_NOISE>(g, s);
            case ACT_LINEAR: return launch_kc_tile<EPI_FWD, ACT_LINEAR>(g, s);
            case ACT_SOFTPLUS: return launch_kc_tile<EPI_FWD, ACT_SOFTPLUS>(g, s);
            default: return -3;
        }
    }
    switch (var) {
        case ACT_RELU: return launch_kc_tile<EPI_DX, ACT_RELU>(g, s);
        case ACT_SOFTPLUS: return launch_kc_tile<EPI_DX, ACT_SOFTPLUS>(g, s);
        default: return launch_kc_tile<EPI_DX, ACT_LINEAR>(g, s);
    }
}

static bool ks_dense_k(const GemmArgs& g) {
    // (one segment: nbatch = the number of models, which the launch spreads over grid.y)
    return g.a_si == 1 && g.b_sj == 1 && gemm_model_batches(g) == 1 && (g.K % BK) == 0 && (g.kchunk % BK) == 0 &&
           (g.seg_rows >= g.seg_stride || g.K <= g.seg_rows) &&
           (long)g.K * g.a_sk * 2 < (1L << 31) && (long)g.K * g.b_sk * 2 < (1L << 31);
}

// n weight-gradient products as one launch; returns 1 (nothing launched) when a problem does not fit the grouped kernel
int launch_gemm_bf16_dw_group(const GemmArgs* gs, int n, hipStream_t s, const char** kname, const FoldJob* fold) {
    if (n < 1 || n > KS_GROUP_MAX) return 1;
    if (gs[0].e.tune_bits & TUNE_BIT_NO_KS_GROUP) return 1;
    KsGroup grp;
    memset(&grp, 0, sizeof grp);
    grp.n = n;
    int total = 0;
    const int models = gemm_models(gs[0]);      // model groups: every block of the launch once per model (grid.y)
    for (int i = 0; i < n; ++i) {
        if (!ks_dense_k(gs[i]) || gemm_models(gs[i]) != models) return 1;
        const int blocks = ceil_div(gs[i].N, 128) * ceil_div(gs[i].M, 128) * gs[i].splits;
        total += blocks;
        grp.blk_end[i] = total;
        grp.g[i] = gs[i];
    }
    if (fold && fold->n > 0) {
        grp.fold = *fold;
        grp.fold.blocks_x = ceil_div(fold->n, 256);
        total += grp.fold.blocks_x * fold->ngroups;
    }
    // Block shape, by measurement (B = 4096, D = 512, the discriminator's launch): 8 waves of 64x32 with a 2-stage ring, two
    // blocks = 16 waves per CU: 58.7 us; 4 waves of 64x64, two blocks per CU (round 2's default, 1.0 instead of 1.5 transposing
    // reads per MFMA): 64.7 us; 8 waves with a 3-stage ring, one block per CU: 89 us.  More resident waves hide the
    // barrier -> LDS read -> MFMA chain; the LDS read rate is not the limit at two blocks per CU.
    constexpr int STAGE = 2 * 64 * 256, LDS = 2 * STAGE;
    if (const int r = launch_with_dyn_lds<gemm_bf16_ks_group_kernel<2, 2, 4>, LDS>(dim3(total, models), dim3(512), s, grp)) return r;
    if (kname) *kname = "gemm_bf16_ks_group_kernel<2, 2, 4>";
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_gemm_bf16(int epi, const GemmArgs& g, hipStream_t s, const char** kname) {
    int r = 0;
    if (epi == EPI_SLAB) {
        if (g.a_si != 1 || g.b_sj != 1) return -3;
        if (ks_dense_k(g)) {
            r = launch_ks_fast<3, 2, 4>(g, s);      // single product: 8 waves (64x32 each), 3-stage ring
        } else {
            dim3 grid(ceil_div(g.N, BN), ceil_div(g.M, 128), g.nbatch * g.splits);
            MRGAN_LAUNCH(gemm_bf16_ks_kernel, grid, dim3(256), 0, s, g);
            g_last_kernel = "gemm_bf16_ks_kernel";
        }
    } else {
        if (g.a_sk != 1 || g.b_sk != 1 || g.splits != 1 || (g.K % BK) != 0) return -3;
        if ((long)g.M * g.a_si * 2 >= (1L << 31) || (long)g.N * g.b_sj * 2 >= (1L << 31)) return -3;
        r = launch_kc_any(epi, g, s);
    }
    if (r) return r;
    if (kname) *kname = g_last_kernel;
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_tr_probe(unsigned short* out, hipStream_t s) {
    MRGAN_LAUNCH(tr_probe_kernel, dim3(1), dim3(64), 0, s, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace mrgan
