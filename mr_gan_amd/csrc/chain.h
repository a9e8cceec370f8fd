// Row-block chain kernel: several consecutive dense products of one 64-row block run inside ONE launch, the block's
// activations staying in LDS between them (gemm_chain.hip).
//
// Why: the narrow tail of the discriminator (mr_gan.py:123-128: 500 -> 250 -> 250 -> 250 -> 6) is 5 % of the step's
// FLOPs but, launched layer by layer, 12 of its 34 launches -- each a 6-13 us kernel whose main loop is shorter than
// its prologue + epilogue.  The weights of these layers total 0.5 MB, so every block can stream all of them from its
// XCD's L2 while the block's rows never leave the CU:
//     D sub-step :  D3 D4 D5 forward -> loss head (mr_gan.py:128, :146-149) -> dX through D5 D4 D3      (1 launch, was 7)
//     G sub-step :  D3 D4 D5 forward (+ feature-matching column sums)                                  (1 launch, was 3)
//                   feature-matching gradient (mr_gan.py:152-154) -> dX through D5 D4 D3               (1 launch, was 4)
// Row blocks are independent (the losses are per-row sums scaled by 1/B), so there is no inter-workgroup traffic at all.
#pragma once
#include "aux_kernels.h"
#include "common.h"
#include "lds_ring.h"

namespace mrgan {

constexpr int CH_ROWS = 64;            // rows per block
constexpr int CH_THREADS = 512;        // 8 waves: wave w owns columns [32 w, 32 w + 32) of a 256-column pass, all 64 rows
constexpr int CH_PW = 256;             // output columns per pass (wider layers take several passes over the resident A)
constexpr int CH_KMAX = 512;           // widest resident activation (reduction length of any product in a chain)
constexpr int CH_STAGE_BYTES = CH_PW * 128;      // one ring stage: a weight tile [256 columns][64 k], 32 KiB
// LDS map (bytes) of a block of `rows` rows (64, or 32 for launches with few row blocks):
//     image 0 (up to 512 columns) | image 1 (up to 256 columns) | the ring of weight tiles          64 rows: 64 + 32 + 2 x 32 KiB, the whole CU
// Which image holds what is fixed, and compiled into the kernel:
//   * product j (0, 1, 2) of a run of three reads image j & 1 and writes the other one; the first A image of every chain
//     (the inputs of D3, or the feature-matching gradient) is therefore image 0, and the features land in image 1;
//   * the loss head reads the features in image 1 and writes dL/d(pre5) into image 0, the A image of the first dX product;
//     the upper half of image 0 is its scratch, and image 0's lower half holds the partial logits until dL/d(pre5) is written;
//   * chain_fmgrad builds its image in image 0 and keeps the folded moments in image 1, idle until the first epilogue.
constexpr int chain_buf0(int rows) { return 0; }
constexpr int chain_buf1(int rows) { return rows * CH_KMAX * 2; }
constexpr int chain_ring(int rows) { return rows * (CH_KMAX + CH_PW) * 2; }
constexpr int chain_stages(int rows) { return rows <= 32 ? 3 : 2; }      // ring depth: what fits beside the images in 160 KiB
constexpr int chain_lds_bytes(int rows) { return chain_ring(rows) + chain_stages(rows) * CH_STAGE_BYTES; }
constexpr int chain_img(int rows, int i) { return (i & 1) ? chain_buf1(rows) : chain_buf0(rows); }
constexpr int chain_head_scratch() { return chain_buf0(CH_ROWS) + CH_ROWS * CH_KMAX; }      // (64-row blocks only)

enum { CH_FWD_RELU = 0, CH_DX_RELU = 1 };
// the three chains of a training step: [F F F H X X X], [F F F], [X X X] (F forward, H loss head, X dX)
enum { CH_V_DTAIL = 0, CH_V_GFWD = 1, CH_V_GBWD = 2 };
// timing experiments (results are wrong): skip the loss head / the copies to HBM / the MFMAs / the weight stream / the epilogue math
enum { CH_ABL_HEAD = 256, CH_ABL_COPY = 512, CH_ABL_MFMA = 1024, CH_ABL_STREAM = 2048, CH_ABL_EPI = 4096 };

// one dense product: out[rows][N] = epilogue(A[rows][K] Bt[N][K]^T)
struct ChainOp {
    int K, N, n_valid;                 // padded reduction / output widths (multiples of 64), logical output width
    const __bf16* W;                   // Bt: [N][K], reduction index contiguous (forward: W^T copy; dX: W copy)
    const float* bias;                 // forward
    float sigma; uint32_t site;        // forward: out += sigma * N(0,1) (the next layer's GaussianNoise); site of the draw
    __bf16* out; long out_bs; int ldo; // global copy of the output [seg][S][ldo]
    uint16_t* mask; long mask_bs; int ldm;      // lane-native relu mask (gemm.h): written by a forward product, read by a dX product
    float* cs; int ldcs;               // optional column sums of the (unrounded) output: one partial row per (segment, row block)
};

struct ChainArgs {
    int variant;                       // CH_V_*
    ChainOp fwd[3];                    // D3 D4 D5 forward (CH_V_DTAIL, CH_V_GFWD)
    ChainOp dx[3];                     // dX through D5 D4 D3 (CH_V_DTAIL, CH_V_GBWD)
    int rows, nseg;                    // valid rows per segment, segments
    // Model groups (the GROUP instantiations): grid.y = models (0 or 1: one model); the row block index (grid.x) and the LDS choreography are a single
    // model's.  Model m's tensors -- W, bias, out, mask and cs of every ChainOp, a, fm_feat, and cs / dpre / loss_out / accum of
    // fm -- lie model_stride BYTES behind model 0's; the head's follow HeadArgs::model_stride / labels_ms; noise seed + m.
    long model_stride; int models;
    int block_rows;                    // rows per block: 64, or 32 (CH_V_GFWD / CH_V_GBWD only)
    const __bf16* a; long a_bs; int lda; int a_cols;      // forward chains: the first A image, rows of a[seg][S][lda], a_cols (padded) columns
    // CH_V_GBWD: the first A image = relu-mask ? gj : 0 with gj from the feature-matching moments (mr_gan.py:152-154)
    FmArgs fm;
    const __bf16* fm_feat; int fm_ldf;                     // features of the generated rows [rows][fm_ldf] (their sign is the relu mask)
    HeadArgs head;                     // CH_V_DTAIL
    int seg0;                          // noise segment id of segment 0
    uint64_t seed; uint32_t row0; const DevState* st;
    int gauss;                         // layer noise of the forward products: 0 = Irwin-Hall, 1 = true Gaussian (MRGAN_FLAG_GAUSS_NOISE)
    unsigned long long* stamps;        // diagnostic build only (make STAMPS=1): [block][8] cycles per phase
    int ablate;                        // timing experiments only (mrgan_debug_ablate): CH_ABL_* bits
};

// What launch_chain accepts (it returns -3 otherwise); a pure host function, no HIP call.  Per product: K in 128 .. 512 and N in
// 64 .. 256 (dX: .. 512) in steps of 64, W (+ bias and 1 <= n_valid <= N forward, + mask dX).  Across products: fwd[i].N ==
// fwd[i + 1].K and dx[i].N == dx[i + 1].K (a product's output image is the next one's A image), dx[0].N and dx[1].N <= CH_PW (only
// the product that ends a chain may take two passes), a_cols == fwd[0].K.  D tail: 64-row blocks, nseg <= 3 training segments,
// classes <= KMAX at pitch KMAX, head.feat == fwd[2].N == dx[0].K <= CH_PW.  G backward: fm.feat == dx[0].K <= CH_PW.
// 1 <= feat_valid <= feat; rows, nseg >= 1; block_rows 32 or 64; no null W6 / b6 / part / loss_part / dpre / cs / fm_feat.
bool chain_args_ok(const ChainArgs& a);
int launch_chain(const ChainArgs& a, hipStream_t s);
// "chain_kernel<V, MI, GAUSS, GROUP>" of the instantiation launch_chain selects for `a` (false: there is none)
bool chain_kernel_name(const ChainArgs& a, char* name, int len);
int chain_init_attributes();           // the dynamic-LDS limit of every chain kernel: once per handle, outside any stream capture

// ---- device side: the activation image [K/64 k-tiles][ROWS rows][64 k] bf16, 16-byte chunks XOR-swizzled per row (kc_off) ----
// byte offset of element (row, col) inside an activation image
template <int ROWS = CH_ROWS>
__device__ __forceinline__ int act_off(int row, int col) {
    return (col >> 6) * (ROWS * 128) + kc_off(row, (col & 63) >> 3) + (col & 7) * 2;
}
// The same for an epilogue that walks a lane's accumulator registers: element (row 32 mi + acc_row(r, lh), column cip) sits at
// obase[sel(r)] + a compile-time offset.  The swizzle term (row>>1)&7 of that row is ((r>>1)&1) | lh<<1 | ((r>>2)&1)<<2, i.e. a
// lane part and 4 register cases.
template <int ROWS>
__device__ __forceinline__ void img_col_bases(int (&obase)[4], int cip, int lh) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        obase[i] = (cip >> 6) * (ROWS * 128) + lh * 512 + (((((cip & 63) >> 3) ^ (lh << 1)) ^ ((i & 1) | ((i >> 1) << 2))) << 4) + (cip & 7) * 2;
}
__device__ __forceinline__ int img_elem_off(const int (&obase)[4], int mi, int r) {
    return obase[((r >> 1) & 1) | (((r >> 2) & 1) << 1)] + (mi * 32 + acc_row(r, 0)) * 128;
}

// Model groups are a compile-time property of a chain kernel (GROUP): the D-tail chain sits at the SGPR limit, and the
// offset arithmetic in the prologue of the two forward chains cost a single handle 0.5 .. 0.8 us per launch when it was
// run-time.  A single handle's instantiation (GROUP = false) has offset 0 and model 0 as constants,
// so everything below folds away.
// bytes from model 0's copy of a tensor to this block's model's (wave-uniform)
template <bool GROUP>
__device__ __forceinline__ long chain_moff(long model_stride) {
    if constexpr (GROUP) return (long)blockIdx.y * model_stride;
    else return 0;
}
template <bool GROUP>
__device__ __forceinline__ uint32_t chain_model_index() {
    if constexpr (GROUP) return blockIdx.y;
    else return 0u;
}
// this model's copy of a per-model tensor that the launcher guarantees (W, bias, a, the masks of dX, the head's tensors) ...
template <typename P>
__device__ __forceinline__ P* chain_model(P* p, long moff) { return (P*)((char*)p + moff); }
template <typename P>
__device__ __forceinline__ const P* chain_model(const P* p, long moff) { return (const P*)((const char*)p + moff); }
// ... and of an optional one (out, a forward mask, cs, the loss scalars): null stays null
template <typename P>
__device__ __forceinline__ P* chain_model_opt(P* p, long moff) { return p ? (P*)((char*)p + moff) : p; }

// LDS writes of every wave visible to every wave; VMEM left in flight
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// copy a [ROWS rows][256 columns] bf16 LDS image (columns col0 .. of the global tensor) out with 16-byte stores
template <int ROWS = CH_ROWS>
__device__ __forceinline__ void copy_out(const char* img, __bf16* out, int ldo, int col0, int ncols, int rows_valid, int t) {
#pragma unroll
    for (int u = 0; u < ROWS * CH_PW / 8 / CH_THREADS; ++u) {
        const int q = t + CH_THREADS * u, r = q >> 5, cch = q & 31;
        if (r < rows_valid && col0 + cch * 8 < ncols)
            *(u32x4*)(out + (long)r * ldo + col0 + cch * 8) = *(const u32x4*)(img + (cch >> 3) * (ROWS * 128) + kc_off(r, cch & 7));
    }
}

}  // namespace mrgan
