// LDS-DMA staging shared by the dense MFMA products (gemm_bf16.hip, gemm_fp8.hip; the pieces gemm_chain.hip borrows).
//
// `buffer_load_dwordx4 ... offen lds` (16 B per lane, 1 KiB per wave-instruction) moves an operand tile straight from
// HBM / L2 into an LDS image -- no VGPR round trip, no ds_write pass:
//   * the LDS destination of a wave-instruction is lane-linear, so the bank-conflict swizzle is applied to the per-lane
//     SOURCE address and undone by the same XOR on the fragment read (kc_off);
//   * the k-offset of a tile is the instruction's SGPR offset: advancing a tile costs no VALU;
//   * rows past the end of an operand fall outside the buffer descriptor's range and arrive as zeros, which is what
//     makes ragged M / N safe without per-lane predicates;
//   * the images form a ring of NS stages with one raw s_barrier per k-tile: wait own loads (counted vmcnt) -> barrier ->
//     refill the stage read one tile ago -> MFMA on this tile, so the next tiles' loads fly under this tile's MFMAs.
// Blocks are persistent and walk the output tiles in an XCD-aware order (xcd_tile, patch order).
// Device code only, all of it force-inlined: no kernel lives here.
#pragma once
#include "common.h"

namespace mrgan {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((address_space(3))) void lds_void;

// byte offset of 16-B chunk `chunk` (0..7) of row `row` in a [rows][128 B] image; (row>>1)&7 spreads the 16 rows of a
// ds_read_b128 lane group over all sixteen 16-B slots of the 256-B bank row
__device__ __forceinline__ int kc_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rs, char* lds_dst, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)lds_dst, 16, voff, soff, 0, 0);
}

// counted wait: all but the newest `n` LDS-DMA groups of LPT instructions each have landed
template <int LPT>
__device__ __forceinline__ void wait_groups(int n) {
    if (n >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- tile order ----------------------------------------------------------------------------------------------------
// XCD-aware tile index: blocks b and b+8 share an XCD, so give XCD x the tiles [x*nt/8, (x+1)*nt/8): a contiguous run
// that shares operand panels in the XCD's private L2
__device__ __forceinline__ int xcd_tile(int bid, int nt) {
    return (nt & 7) == 0 ? (bid & 7) * (nt >> 3) + (bid >> 3) : bid;
}
// Patch order: within an XCD's run the plain order is row-major, so the blocks resident on one XCD at any moment cover
// 2 tile rows x 16 columns (2 x 32 for the 64 resident dW blocks).  Where the kernels below say "patches of P tile rows"
// (ntm a multiple of P), consecutive tiles walk P tile rows column by column instead -- 4 x 8 (8 x 8) patches -- and a
// third (a half) less distinct operand data has to enter that XCD's L2 per k-step.  When to patch was measured per
// kernel family, so each kernel spells its own condition; the arithmetic stays written out in each of them, like the
// operand-panel set-up, because moving either behind a function changes the register allocation of those kernels.

// ---- the bf16 ring ---------------------------------------------------------------------------------------------------
// acc += A B^T over the nk k-tiles of a ring of NS stages (stage s at lds + s * STAGE, the B image B_OFF bytes into it)
// whose first NS-1 tiles the caller has issued.  issue(k0, stage) starts the LDS-DMA group (LPT instructions per wave) of
// the 64 reduction elements at k0; K_BASE is the block's first reduction element.  FRAG_A(As, mi, ks) / FRAG_B(Bs, ni, ks)
// read the MFMA fragment of 32-row block mi / ni of the wave's tile for k-step ks (16 elements) of a stage; STAMP(0) /
// STAMP(1) bracket the first tile's wait in the STAMPS build.
// A macro on purpose: behind any function boundary (force-inlined template, lambdas for the fragment reads) hipcc hoists
// the fragment addresses differently and the k-loop of every KC kernel gains scalar adds; expanded in place, the loop
// compiles to the same instructions as when it was written out in each kernel.
// vmcnt counts in issue order: whatever the wave issued before the group being waited for (stores of the previous tile,
// epilogue prefetch loads) is retired by the same wait.
constexpr int RING_BK = 64;
#define RING_MAINLOOP(NS, LPT, MR, NR, nk, acc, issue, K_BASE, FRAG_A, FRAG_B, lds, STAGE, B_OFF, STAMP)                \
    {                                                                                                                  \
        static_assert(NS >= 2 && NS <= 4, "ring depth");                                                               \
        int buf = 0;                                                                                                   \
        for (int kt = 0; kt < nk; ++kt) {                                                                              \
            if (kt == 0) STAMP(0);                                      /* tile setup + issue */                       \
            wait_groups<LPT>(min(NS - 2, nk - 1 - kt));                 /* this wave's loads of k-tile kt have landed */ \
            __builtin_amdgcn_s_barrier();                               /* ... everyone's; everyone finished kt-1 */    \
            asm volatile("" ::: "memory");                                                                             \
            if (kt == 0) STAMP(1);                                      /* first k-tile landed (pipeline fill) */      \
            if (kt + NS - 1 < nk) {                                     /* refill the stage read during k-tile kt-1 */ \
                int nb = buf + NS - 1; if (nb >= NS) nb -= NS;                                                         \
                issue(K_BASE + (kt + NS - 1) * RING_BK, nb);                                                           \
            }                                                                                                          \
            const char* As = lds + buf * STAGE;                                                                        \
            const char* Bs = As + B_OFF;                                                                               \
            buf = (buf + 1 == NS) ? 0 : buf + 1;                                                                       \
            /* fragments of KG k-steps are fetched as one batch ahead of their MFMAs: the LDS latency is paid once */  \
            /* per batch (counted lgkmcnt waits) instead of once per MFMA */                                           \
            constexpr int KG = (MR + NR <= 4) ? 4 : 2;                                                                 \
            _Pragma("unroll") for (int kg = 0; kg < RING_BK / 16; kg += KG) {                                          \
                bf16x8 a[KG][MR], b[KG][NR];                                                                           \
                _Pragma("unroll") for (int kk = 0; kk < KG; ++kk) {                                                    \
                    _Pragma("unroll") for (int mi = 0; mi < MR; ++mi) a[kk][mi] = FRAG_A(As, mi, kg + kk);             \
                    _Pragma("unroll") for (int ni = 0; ni < NR; ++ni) b[kk][ni] = FRAG_B(Bs, ni, kg + kk);             \
                }                                                                                                      \
                __builtin_amdgcn_sched_barrier(0);   /* keep the scheduler from re-serialising read -> wait -> MFMA */ \
                _Pragma("unroll") for (int kk = 0; kk < KG; ++kk)                                                      \
                    _Pragma("unroll") for (int mi = 0; mi < MR; ++mi)                                                  \
                        _Pragma("unroll") for (int ni = 0; ni < NR; ++ni)                                              \
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kk][mi], b[kk][ni], acc[mi][ni], 0, 0, 0); \
            }                                                                                                          \
        }                                                                                                              \
    }

}  // namespace mrgan
