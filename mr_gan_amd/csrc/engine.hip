// Engine behind include/mrgan_abi.h: workspace layout in HBM, the launch sequence of one discriminator
// sub-step and one generator sub-step (mr_gan.py:204-213), evaluation, and the C ABI itself.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mrgan_abi.h"
#include "../../include/mrgan_debug.h"
#include "aux_kernels.h"
#include "chain.h"
#include "logmel.h"
#include "gemm.h"

using namespace mrgan;

namespace mrgan {
thread_local LaunchTimer g_launch_timer = {nullptr, nullptr, 0, 0};      // see MRGAN_LAUNCH (common.h)
int launch_tr_probe(unsigned short* out, hipStream_t s);
}

namespace {

thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x)                                                                               \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return fail(-10, "%s failed: %s", #x, hipGetErrorString(e_));     \
    } while (0)
#define CHK(x)                                                          \
    do {                                                                \
        int r_ = (x);                                                   \
        if (r_ != 0) return r_ < -9 ? r_ : fail(r_, "launch failed (%d) at %s:%d", r_, __FILE__, __LINE__); \
    } while (0)

constexpr int PADW = 64;       // every feature dimension is padded to a multiple of 64 (zero-filled); 128 in the fp8 mode
thread_local int g_padw = PADW;
constexpr int SEG_ALIGN = 128; // segment row stride is a multiple of the GEMM block tile

struct Tensor {                // one trainable tensor (padded fp32 master + Adam slots)
    int rows, cols;            // logical (1-D: rows = 1)
    int prow, pcol;            // padded
    float *p, *m, *v;
    __bf16 *w16, *wt16;
    float* flat;               // position inside the flat gradient buffer
    __bf16* flat16;            // ... inside the bfloat16 one (MRGAN_FLAG_GRAD_BF16)
    const float* g; int nslab; long slab_stride;      // fused-mode gradient source
};

struct Dense {
    int K, N, Kp, Np, act;
    Tensor *W, *b;
    float* slabs; int splits;   // weight-gradient slabs [nseg*splits][Kp][Np]
};

struct ProfRec { int cat; hipEvent_t start, stop; double flops, bytes; };      // device-side begin / end of one kernel (MRGAN_LAUNCH)

// fp8 scaling slots: kind 0 = D sub-step, 1 = G sub-step; X = activations (e4m3), G = gradients (e5m2), W = weights (e4m3)
constexpr int FP8_NSLOT = 28, FP8_DRY_PASSES = MRGAN_FP8_DRY_PASSES;
inline int slot_x(int kind, int l) { return kind * 10 + l; }
inline int slot_g(int kind, int l) { return kind * 10 + 5 + l; }
inline int slot_w(int l) { return 20 + l; }
// the generator's 4096 x 4096-class layer G2 (hbn -> h2): input, output gradient, weight
constexpr int SLOT_GX = 25, SLOT_GG = 26, SLOT_GW = 27;
constexpr float FP8_TARGET_E4M3 = 224.0f, FP8_TARGET_E5M2 = 28672.0f;      // half the largest finite value: 2x headroom

struct Arena {
    char* base = nullptr; size_t off = 0, cap = 0;
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

}  // namespace

struct mrgan_handle {
    mrgan_config cfg;
    bool bf16, sync_stats, flat_grads, own_ws;
    int es;                               // activation element size
    int B, S, tiles_m, Bg;                // local batch, segment stride, row tiles per segment, global batch
    float stat_count, fm_scale;           // rows behind a batch statistic; 1/world when statistics stay per-shard
    int Dp, nzp, Fp, F;                   // padded input / z / feature widths
    char* ws; size_t ws_bytes;

    std::vector<Tensor> gt, dt;           // Keras order
    Dense g[3], d[6];

    DevState* state;                      // [2]
    int cur;                              // host mirror of the live slot
    float* step_out;                      // [4]
    float* accum;                         // [4]
    int* err_count;
    float *flat_d, *flat_g; size_t flat_d_n, flat_g_n;
    __bf16 *flat16_d, *flat16_g;          // MRGAN_FLAG_GRAD_BF16
    float *r_bn_stats, *r_fm, *r_bn_bwd;

    // activations (T = float | __bf16)
    void *zbuf, *h1, *hbn, *h2;          // the generator activations the current sub-step works on (views into *_all)
    void *zbuf_all, *h1_all, *hbn_all, *h2_all;   // [2][S] rows: segment 1 = the G sub-step's batch when a pair runs its two
                                                  // generator forwards as one (pair_gen)
    int pair_gen, gen_ready;             // train_pair: D_GEN also ran the G sub-step's generator forward
    const mrgan_gen_args* pair_g; int real_staged;   // train_pair: ... and staged the G sub-step's real rows
    int xbase;                           // first xin[0] slot of the current G sub-step (0, or 3 after a paired forward)
    void* xin[5]; void* feat; uint16_t* mask[5]; int ldm[5];
    void* dpre[5];
    void *dxfake, *dpre2g, *dhbn, *dpre1g;
    float* logits;
    float *bn_mu, *bn_rstd, *bn_mu_all, *bn_rstd_all;
    // partial sums
    float *cs_bn1, *cs_bn2, *cs_db[4], *cs_f, *cs_db3g, *cs_db2g, *cs_dbeta, *cs_dgamma, *db1g_part;
    float *head_part, *head_red, *loss_part; int head_stride, head_groups;
    int nblk_head, bnb_blocks;
    // fp8 mode (gemm_fp8.hip): fp8 copies of the discriminator's activations x8 / gradients g8 (row-major and transposed),
    // of its weights, and the scaling slots (index fp8_slot())
    bool fp8; int fp8_kind; int fp8_cal[2];
    unsigned char *x8[5], *x8t[5], *g8[5], *g8t[5], *w8[5], *w8t[5];
    unsigned char *hbn8, *hbn8t, *dp2g8, *dp2g8t, *gw8, *gw8t;      // generator layer G2: BN(h1) [2][S][N1], dpre2 [S][N2], W2
    int gen_seg;                                                  // segment the generator views point at (set_gen_view)
    Fp8Slot* slots; float* slot_targets; float* accum_save;
    float* fm_scratch; unsigned int* fm_count;       // feature-matching loss partials of a wide feature layer (aux_kernels.hip)
    bool chain_ok, use_chain;            // the 256-wide tail of the discriminator runs as row-block chain launches (gemm_chain.hip)
    bool head_wide_ok, head_wide; __bf16 *w6c, *w6r;   // feature layers wider than the chain holds: the stand-alone MFMA loss head (chain.h: HeadWideArgs)
    int tune_kc_cfg, tune_bits, tune_pair_gen;      // mrgan_set_tuning
    int ablate;                                      // mrgan_debug_ablate (timing experiments)
    AdamTile *tiles_g_dev, *tiles_d_dev; int ntiles_g, ntiles_d;

    // per-launch hipEvent profiling (bench.py's live roofline measurement)
    bool prof; std::vector<ProfRec> prof_recs; std::vector<std::string> prof_names;

    // graph replay of (D step, G step)
    hipGraphExec_t graph_exec; bool graph_ready; int graph_cur; mrgan_disc_args graph_d; mrgan_gen_args graph_g;
};

namespace {

// ------------------------------------------------------------------------------------------------
// small utility kernels (weights in/out, debug GEMM staging)
// ------------------------------------------------------------------------------------------------
__global__ void refresh_bf16_kernel(const float* p, __bf16* w16, __bf16* wt16, int prow, int pcol) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= prow || c >= pcol) return;
    const __bf16 v = (__bf16)p[(long)r * pcol + c];
    if (w16) w16[(long)r * pcol + c] = v;
    if (wt16) wt16[(long)c * prow + r] = v;
}
template <typename T>
__global__ void convert_kernel(const float* src, long lds, T* dst, long ldd, int rows, int cols, int prow, int pcol, int transpose) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= prow || c >= pcol) return;
    const float v = (r < rows && c < cols) ? src[(long)r * lds + c] : 0.f;
    if (transpose) dst[(long)c * ldd + r] = Elem<T>::from_f32(v);
    else dst[(long)r * ldd + c] = Elem<T>::from_f32(v);
}
template <typename T>
__global__ void to_f32_kernel(const T* src, long lds, float* dst, long ldd, int rows, int cols) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= rows || c >= cols) return;
    dst[(long)r * ldd + c] = Elem<T>::to_f32(src[(long)r * lds + c]);
}
__global__ void sum_slabs_kernel(const float* slabs, int nslab, long stride, long n, float* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += slabs[k * stride + i];
    out[i] = s;
}
__global__ void init_state_kernel(DevState* st, uint32_t iter, uint32_t batch, float lr, float b1, float b2) {
    DevState s;
    s.iter = iter; s.batch = batch; s.pad = 0;
    const double t = (double)iter + 1.0;
    s.lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    st[0] = s; st[1] = s;
}

inline dim3 grid2d(int prow, int pcol) { return dim3(ceil_div(pcol, 64), ceil_div(prow, 4)); }

// ------------------------------------------------------------------------------------------------
// layout
// ------------------------------------------------------------------------------------------------
int pad64(int x) { return (int)round_up(x, g_padw); }

constexpr int MAX_SLABS = 16;
// Reduction splits (= fp32 slabs per tensor, summed by the Adam kernel) of the weight-gradient products of one
// network.  The products of a sub-step run as ONE grouped launch (dense_dw_all) of 128x128 blocks, two of which share
// a CU, and every block costs the same per reduction row: the best grid is a single round that fills most of the 512
// block slots, with as few slabs as that allows (each slab is read again by Adam).
// Measured on MI355X (B=4096, D=512, ms/step): D network 5 splits (400 blocks) 0.449, 6 -> 0.455, 4 -> 0.459, 8 -> 0.472.
int choose_splits(int group_tiles, int vrows) {
    int s = 435 / std::max(1, group_tiles);     // ~85 % of 512 slots
    s = std::min(s, 6);
    s = std::min(s, ceil_div(vrows, 512));      // keep >= 512 reduction rows per slab
    return std::max(1, std::min(s, MAX_SLABS));
}
int dw_tiles(const Dense& L) { return ceil_div(L.Kp, 128) * ceil_div(L.Np, 128); }
int fp8_dw_splits(int tiles, int rows) {
    int s = 1;
    while (s < 4 && tiles * s * 2 <= 512 && tiles >= 64 && (rows % (s * 2 * 128)) == 0 && rows / (s * 2) >= 2048) s *= 2;
    return s;
}

int validate(const mrgan_config& c) {
    if (c.d_in < 1 || c.batch < 1) return fail(-1, "d_in and batch must be positive");
    if (c.num_classes < 2 || c.num_classes > KMAX) return fail(-1, "num_classes must be in [2,%d]", KMAX);
    if (c.dtype != MRGAN_F32 && c.dtype != MRGAN_BF16 && c.dtype != MRGAN_FP8) return fail(-1, "unknown dtype");
    if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return fail(-1, "bad rank/world");
    if (c.world > 1 && (c.batch % 4) != 0) return fail(-1, "data-parallel shards need batch %% 4 == 0 (noise row groups)");
    if (c.world > 1 && (c.flags & (MRGAN_FLAG_FLAT_GRADS)) == 0) return fail(-1, "world > 1 requires MRGAN_FLAG_FLAT_GRADS");
    if ((c.flags & MRGAN_FLAG_GRAD_BF16) && !(c.flags & MRGAN_FLAG_FLAT_GRADS)) return fail(-1, "MRGAN_FLAG_GRAD_BF16 requires MRGAN_FLAG_FLAT_GRADS");
    for (int i = 0; i < 5; ++i) if (c.d_hidden[i] < 1) return fail(-1, "bad d_hidden");
    if (c.g_hidden[0] < 1 || c.g_hidden[1] < 1 || c.noise_size < 1) return fail(-1, "bad generator sizes");
    return 0;
}

int count_adam_tiles(const std::vector<Tensor>& ts);
// carve the workspace; with base == nullptr only computes the size
int layout(mrgan_handle* h, char* base, size_t* bytes_out) {
    const mrgan_config& c = h->cfg;
    h->fp8 = c.dtype == MRGAN_FP8;
    h->bf16 = c.dtype == MRGAN_BF16 || h->fp8;            // the fp8 mode keeps the whole bf16 machinery (generator, head, evaluation)
    h->es = h->bf16 ? 2 : 4;
    g_padw = h->fp8 ? 128 : PADW;
    h->sync_stats = (c.flags & MRGAN_FLAG_SYNC_STATS) != 0;
    h->flat_grads = (c.flags & MRGAN_FLAG_FLAT_GRADS) != 0;
    h->B = c.batch; h->S = (int)round_up(c.batch, SEG_ALIGN); h->tiles_m = ceil_div(c.batch, 64);   // 64-row column-sum partials
    h->Bg = c.batch * c.world;
    h->stat_count = (float)(h->sync_stats ? h->Bg : h->B);
    h->fm_scale = h->sync_stats ? 1.0f : 1.0f / (float)c.world;
    h->Dp = pad64(c.d_in); h->nzp = pad64(c.noise_size);
    h->F = c.d_hidden[4]; h->Fp = pad64(h->F);
    const int B = h->B, S = h->S, tm = h->tiles_m;
    Arena a; a.base = base;

    h->state = a.take<DevState>(2);
    h->step_out = a.take<float>(4);
    h->accum = a.take<float>(4);
    h->err_count = a.take<int>(4);

    // ---- tensors -----------------------------------------------------------------------------
    const int gdim[4] = {c.noise_size, c.g_hidden[0], c.g_hidden[1], c.d_in};
    const int ddim[7] = {c.d_in, c.d_hidden[0], c.d_hidden[1], c.d_hidden[2], c.d_hidden[3], c.d_hidden[4], c.num_classes};
    h->gt.assign(8, Tensor());
    h->dt.assign(12, Tensor());
    auto mk = [&](Tensor& t, int rows, int cols, int prow, int pcol, bool copies) {
        t.rows = rows; t.cols = cols; t.prow = prow; t.pcol = pcol;
        const size_t n = (size_t)prow * pcol;
        t.p = a.take<float>(n); t.m = a.take<float>(n); t.v = a.take<float>(n);
        t.w16 = t.wt16 = nullptr;
        if (copies && h->bf16) { t.w16 = a.take<__bf16>(n); t.wt16 = a.take<__bf16>(n); }
        t.g = nullptr; t.nslab = 0; t.slab_stride = 0; t.flat = nullptr; t.flat16 = nullptr;
    };
    // generator: W1 b1 gamma beta W2 b2 W3 b3
    const int gW[3] = {0, 4, 6}, gb[3] = {1, 5, 7};
    for (int l = 0; l < 3; ++l) {
        const int K = gdim[l], N = gdim[l + 1], Kp = pad64(K), Np = pad64(N);
        mk(h->gt[gW[l]], K, N, Kp, Np, true);
        mk(h->gt[gb[l]], 1, N, 1, Np, false);
        h->g[l] = Dense{K, N, Kp, Np, l < 2 ? ACT_SOFTPLUS : ACT_LINEAR, &h->gt[gW[l]], &h->gt[gb[l]], nullptr, 1};
    }
    mk(h->gt[2], 1, gdim[1], 1, pad64(gdim[1]), false);
    mk(h->gt[3], 1, gdim[1], 1, pad64(gdim[1]), false);
    for (int l = 0; l < 6; ++l) {
        const int K = ddim[l], N = ddim[l + 1], Kp = pad64(K), Np = (l == 5) ? KMAX : pad64(N);
        mk(h->dt[2 * l], K, N, Kp, Np, l < 5);
        mk(h->dt[2 * l + 1], 1, N, 1, Np, false);
        h->d[l] = Dense{K, N, Kp, Np, l < 5 ? ACT_RELU : ACT_LINEAR, &h->dt[2 * l], &h->dt[2 * l + 1], nullptr, 1};
    }
    // flat gradient buffers (padded layout, Keras order) + 4 scalars
    const bool g16 = (c.flags & MRGAN_FLAG_GRAD_BF16) != 0;
    auto flat = [&](std::vector<Tensor>& ts, float*& buf, __bf16*& buf16, size_t& n) {
        n = 0;
        for (auto& t : ts) n += (size_t)t.prow * t.pcol;
        buf = a.take<float>(n + 4);
        buf16 = g16 ? a.take<__bf16>(n) : nullptr;
        size_t o = 0;
        for (auto& t : ts) { t.flat = buf ? buf + o : nullptr; t.flat16 = buf16 ? buf16 + o : nullptr; o += (size_t)t.prow * t.pcol; }
    };
    flat(h->gt, h->flat_g, h->flat16_g, h->flat_g_n);
    flat(h->dt, h->flat_d, h->flat16_d, h->flat_d_n);
    const int N1p = h->g[0].Np;
    h->r_bn_stats = a.take<float>(4 * N1p);                 // [segment][sum h | sum h^2][N1p]
    h->r_fm = a.take<float>(2 * h->Fp);
    h->r_bn_bwd = a.take<float>(2 * N1p);
    h->bn_mu_all = a.take<float>(2 * N1p);
    h->bn_rstd_all = a.take<float>(2 * N1p);

    // ---- activations ---------------------------------------------------------------------------
    const size_t es = h->es;
    auto act = [&](size_t rows, size_t cols) { return (void*)a.take<char>(rows * cols * es); };
    h->zbuf_all = act(2 * (size_t)S, h->nzp);
    h->h1_all = act(2 * (size_t)S, N1p); h->hbn_all = act(2 * (size_t)S, N1p); h->h2_all = act(2 * (size_t)S, h->g[1].Np);
    for (int l = 0; l < 5; ++l) {
        // xin[0]: slots 0..2 = the D sub-step's segments, 3..4 = the G sub-step's (fake, real) after a paired forward
        h->xin[l] = act((l == 0 ? 5 : 3) * (size_t)S, h->d[l].Kp);
        h->ldm[l] = h->d[l].Np;                                   // lane-native relu mask: 2 x u16 per (32 rows, column)
        h->mask[l] = a.take<uint16_t>(3 * (size_t)(S / 32) * h->ldm[l] * 2);
        h->dpre[l] = act(3 * (size_t)S, h->d[l].Np);
    }
    h->feat = act(3 * (size_t)S, h->Fp);
    if (h->fp8) {
        for (int l = 0; l < 5; ++l) {
            const Dense& L = h->d[l];
            h->x8[l] = a.take<unsigned char>(3 * (size_t)S * L.Kp); h->x8t[l] = a.take<unsigned char>(3 * (size_t)S * L.Kp);
            h->g8[l] = a.take<unsigned char>(3 * (size_t)S * L.Np); h->g8t[l] = a.take<unsigned char>(3 * (size_t)S * L.Np);
            h->w8[l] = a.take<unsigned char>((size_t)L.Kp * L.Np); h->w8t[l] = a.take<unsigned char>((size_t)L.Kp * L.Np);
        }
        {
            const Dense& L = h->g[1];
            h->hbn8 = a.take<unsigned char>(2 * (size_t)S * L.Kp); h->hbn8t = a.take<unsigned char>(2 * (size_t)S * L.Kp);
            h->dp2g8 = a.take<unsigned char>((size_t)S * L.Np); h->dp2g8t = a.take<unsigned char>((size_t)S * L.Np);
            h->gw8 = a.take<unsigned char>((size_t)L.Kp * L.Np); h->gw8t = a.take<unsigned char>((size_t)L.Kp * L.Np);
        }
        h->slots = a.take<Fp8Slot>(FP8_NSLOT); h->slot_targets = a.take<float>(FP8_NSLOT); h->accum_save = a.take<float>(4);
    }
    h->dxfake = act(S, h->Dp); h->dpre2g = act(S, h->g[1].Np); h->dhbn = act(S, N1p); h->dpre1g = act(S, N1p);
    h->logits = a.take<float>(3 * (size_t)S * KMAX);
    h->fm_scratch = a.take<float>(ceil_div(h->Fp, 64)); h->fm_count = a.take<unsigned int>(4);

    // ---- partial sums ----------------------------------------------------------------------------
    h->cs_bn1 = a.take<float>(2 * (size_t)tm * N1p); h->cs_bn2 = a.take<float>(2 * (size_t)tm * N1p);
    for (int l = 0; l < 4; ++l) h->cs_db[l] = a.take<float>(3 * (size_t)tm * h->d[l].Np);
    h->cs_f = a.take<float>(2 * (size_t)ceil_div(B, 32) * h->Fp);      // per (segment, row block): 64-row tiles, or the chain's 32-row blocks
    h->cs_db3g = a.take<float>((size_t)tm * h->Dp);
    h->cs_db2g = a.take<float>((size_t)tm * h->g[1].Np);
    h->cs_dbeta = a.take<float>((size_t)tm * N1p); h->cs_dgamma = a.take<float>((size_t)tm * N1p);
    h->bnb_blocks = stat_row_blocks(B);
    h->db1g_part = a.take<float>((size_t)h->bnb_blocks * N1p);
    // the tail D3..D5 + head as chain launches: bf16, A image <= 512 columns, outputs <= 256 columns
    // (every reduction of a chain needs two k-tiles: the weight stream keeps two tiles in flight)
    h->chain_ok = h->bf16 && !h->fp8 && h->d[2].Kp <= CH_KMAX && h->d[2].Np <= CH_PW && h->d[3].Np <= CH_PW && h->d[4].Np <= CH_PW &&
                  std::min(std::min(h->d[2].Kp, h->d[2].Np), std::min(h->d[3].Np, h->d[4].Np)) >= 128;
    h->use_chain = h->chain_ok;
    // bf16 / fp8 engines whose feature layer is wider than the chain's 256 columns (the wide stack) run the loss head of the D
    // sub-step on the matrix cores too (64-row blocks, as the chain's)
    h->head_wide_ok = h->head_wide = h->bf16 && h->Fp > CH_PW && (h->Fp % CH_PW) == 0;
    h->w6c = h->w6r = nullptr;
    if (h->head_wide) { h->w6c = a.take<__bf16>((size_t)3 * KMAX * h->Fp); h->w6r = a.take<__bf16>((size_t)3 * KMAX * h->Fp); }
    h->nblk_head = 3 * ceil_div(B, HEAD_ROWS);                            // capacity; the chain path fills 3 * ceil(B / 64) of them
    h->head_stride = (int)round_up(h->Fp * KMAX + KMAX + h->Fp, 64);      // dW6 | db6 | bias grad of the feature layer
    h->head_groups = std::min(8, 3 * ceil_div(B, CH_ROWS));
    h->head_part = a.take<float>((size_t)h->nblk_head * h->head_stride);
    h->head_red = a.take<float>((size_t)h->head_groups * h->head_stride);
    h->loss_part = a.take<float>((size_t)h->nblk_head * 4);

    // ---- weight-gradient slabs ---------------------------------------------------------------------
    int tiles_d = 0, tiles_g = 0;
    for (int l = 0; l < 5; ++l) tiles_d += dw_tiles(h->d[l]);
    for (int l = 0; l < 3; ++l) tiles_g += dw_tiles(h->g[l]);
    // (256 x 128 output tiles with one 8-wave block per CU were tried for the discriminator's launch in round 3: 25 % fewer staged
    //  bytes per flop, but 54.5 us against 47.5 us with two- and three-stage rings -- 200 blocks leave a fifth of the CUs idle)
    const int splits_d = choose_splits(tiles_d, 2 * S + B), splits_g = choose_splits(tiles_g, B);
    for (int l = 0; l < 5; ++l) {
        Dense& L = h->d[l];
        // fp8: one product per layer over all 3 S rows; only a layer with too few 128 x 128 output tiles to fill the chip
        // (the first layer of a wide stack) splits its reduction
        L.splits = h->fp8 ? fp8_dw_splits(dw_tiles(L), 3 * S) : splits_d;
        L.slabs = a.take<float>((size_t)L.splits * L.Kp * L.Np);
    }
    for (int l = 0; l < 3; ++l) {
        Dense& L = h->g[l];
        L.splits = (h->fp8 && l == 1) ? 1 : splits_g;       // fp8: G2's weight gradient is one fp8 product
        L.slabs = a.take<float>((size_t)L.splits * L.Kp * L.Np);
    }
    // ---- fused-mode gradient sources ----------------------------------------------------------------
    auto src = [&](Tensor& t, const float* g, int nslab, long stride) { t.g = g; t.nslab = nslab; t.slab_stride = stride; };
    for (int l = 0; l < 5; ++l) src(*h->d[l].W, h->d[l].slabs, h->d[l].splits, (long)h->d[l].Kp * h->d[l].Np);
    for (int l = 0; l < 4; ++l) src(*h->d[l].b, h->cs_db[l], 3 * tm, h->d[l].Np);
    src(*h->d[4].b, h->head_red + h->Fp * KMAX + KMAX, h->head_groups, h->head_stride);
    src(*h->d[5].W, h->head_red, h->head_groups, h->head_stride);
    src(*h->d[5].b, h->head_red + h->Fp * KMAX, h->head_groups, h->head_stride);
    for (int l = 0; l < 3; ++l) src(*h->g[l].W, h->g[l].slabs, h->g[l].splits, (long)h->g[l].Kp * h->g[l].Np);
    src(*h->g[0].b, h->db1g_part, h->bnb_blocks, N1p);
    src(h->gt[2], h->cs_dgamma, tm, N1p);
    src(h->gt[3], h->cs_dbeta, tm, N1p);
    src(*h->g[1].b, h->cs_db2g, tm, h->g[1].Np);
    src(*h->g[2].b, h->cs_db3g, tm, h->Dp);

    // ---- Adam tile tables ------------------------------------------------------------------------------
    h->ntiles_g = count_adam_tiles(h->gt); h->ntiles_d = count_adam_tiles(h->dt);
    h->tiles_g_dev = a.take<AdamTile>(h->ntiles_g);
    h->tiles_d_dev = a.take<AdamTile>(h->ntiles_d);

    *bytes_out = (a.off + 255) & ~(size_t)255;
    return 0;
}

// Rows per Adam tile (one 256-thread block each).  The update is pure streaming (48 B per parameter in the bf16 mode) and a block's
// loads are one dependent round: what hides the latency is blocks per CU.  64 x 64 tiles give the discriminator of the reference
// 330 blocks on 256 CUs (15 us, 4 TB/s); 16-row tiles give 1 300.  Wide stacks have thousands of 64-row tiles already.
int adam_tile_rows(const std::vector<Tensor>& ts) {
    long n64 = 0;
    for (auto& t : ts) n64 += (long)ceil_div(t.prow, 64) * ceil_div(t.pcol, 64);
    return n64 >= 2048 ? 64 : 16;
}
int count_adam_tiles(const std::vector<Tensor>& ts) {
    const int tr = adam_tile_rows(ts);
    int n = 0;
    for (auto& t : ts) n += ceil_div(t.prow, tr) * ceil_div(t.pcol, 64);
    return n;
}

int upload_tiles(mrgan_handle* h, std::vector<Tensor>& ts, AdamTile* dev, int n, hipStream_t s) {
    std::vector<AdamTile> v;
    const int TR = adam_tile_rows(ts);
    for (auto& t : ts)
        for (int r0 = 0; r0 < t.prow; r0 += TR)
            for (int c0 = 0; c0 < t.pcol; c0 += 64) {
                AdamTile a;
                const long off = (long)r0 * t.pcol + c0;
                a.p = t.p + off; a.m = t.m + off; a.v = t.v + off;
                a.g = t.g + off; a.nslab = t.nslab; a.slab_stride = t.slab_stride;
                a.flat = t.flat + off; a.flat16 = t.flat16 ? t.flat16 + off : nullptr;
                a.w16 = t.w16 ? t.w16 + off : nullptr;
                a.wt16 = t.wt16 ? t.wt16 + (long)c0 * t.prow + r0 : nullptr;
                a.w8 = a.w8t = nullptr; a.w8_slot = nullptr;
                for (int l = 0; l < 5 && h->fp8; ++l)
                    if (&t == h->d[l].W) { a.w8 = h->w8[l] + off; a.w8t = h->w8t[l] + (long)c0 * t.prow + r0; a.w8_slot = h->slots + slot_w(l); }
                if (h->fp8 && &t == h->g[1].W) { a.w8 = h->gw8 + off; a.w8t = h->gw8t + (long)c0 * t.prow + r0; a.w8_slot = h->slots + SLOT_GW; }
                a.ld = t.pcol; a.ldt = t.prow;
                a.rows = std::min(TR, t.prow - r0); a.cols = std::min(64, t.pcol - c0);
                v.push_back(a);
            }
    if ((int)v.size() != n) return fail(-20, "tile count mismatch");
    HIPCHK(hipMemcpyAsync(dev, v.data(), sizeof(AdamTile) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));      // v dies at scope exit
    return 0;
}

// ------------------------------------------------------------------------------------------------
// optional per-launch timing: one hipEvent pair per launch, on the launch stream
// ------------------------------------------------------------------------------------------------
// Per-kernel timing of the profiling pass: every launch of the step goes through MRGAN_LAUNCH (common.h), which takes
// a (start, stop) event pair stamped at the kernel's own begin and end on the device.
int prof_cat(mrgan_handle* h, const char* name) {
    for (size_t i = 0; i < h->prof_names.size(); ++i)
        if (h->prof_names[i] == name) return (int)i;
    h->prof_names.push_back(name);
    return (int)h->prof_names.size() - 1;
}
// Profiling pass only: a ~0.4 ms single-wave delay at the head of each sub-step.  While it runs the host enqueues
// the sub-step's launches behind it, so the kernels execute back to back as they do in the graph replay (caches and
// clocks in the same state) instead of at the host's launch rate.
__global__ void prof_delay_kernel(int us) {
    for (int i = 0; i < us; ++i) __builtin_amdgcn_s_sleep(36);      // 36 * 64 cycles ~ 1 us
}


void prof_backlog(mrgan_handle* h, hipStream_t s) {
    if (!h->prof) return;
    hipLaunchKernelGGL(prof_delay_kernel, dim3(1), dim3(64), 0, s, 400);
}
// arm the launch timer for the next MRGAN_LAUNCH ...
void prof_arm(mrgan_handle* h) {
    if (!h->prof) return;
    LaunchTimer& lt = g_launch_timer;
    lt.armed = lt.fired = 0;
    if (hipEventCreate(&lt.start) != hipSuccess) return;
    if (hipEventCreate(&lt.stop) != hipSuccess) { hipEventDestroy(lt.start); return; }
    lt.armed = 1;
}
// ... and book the launch it timed under `name`
// flops / bytes: ALGORITHMIC work of the launch (2 x logical M N K; operands read once + outputs written once)
void prof_done(mrgan_handle* h, const char* name, double flops, double bytes = 0.0) {
    if (!h->prof) return;
    LaunchTimer& lt = g_launch_timer;
    if (lt.fired) h->prof_recs.push_back(ProfRec{prof_cat(h, name), lt.start, lt.stop, flops, bytes});
    else if (lt.armed) { hipEventDestroy(lt.start); hipEventDestroy(lt.stop); }
    lt.armed = lt.fired = 0;
}
#define PROFB(name, call, bytes)            \
    do {                                    \
        prof_arm(h);                        \
        const int prc_ = (call);            \
        prof_done(h, name, 0, bytes);       \
        CHK(prc_);                          \
    } while (0)
#define PROF(name, call) PROFB(name, call, 0.0)

// ------------------------------------------------------------------------------------------------
// GEMM call sites
// ------------------------------------------------------------------------------------------------
// algo_flops / algo_bytes: the ALGORITHMIC work of the product: logical, unpadded shapes, 2 FLOP per MAC,
// operands read once + outputs written once -- no padding, no split-K slabs, no re-reads
int run_gemm(mrgan_handle* h, int epi, const GemmArgs& g, double algo_flops, double algo_bytes, hipStream_t s) {
    const char* kname = "gemm";
    prof_arm(h);
    const int r = h->bf16 ? launch_gemm_bf16(epi, g, s, &kname) : launch_gemm_f32(epi, g, s, &kname);
    prof_done(h, kname, algo_flops, algo_bytes);
    CHK(r);
    return 0;
}
// activations [rows][K] in, [rows][N] out (element size es), the weight matrix once
double dense_bytes(const mrgan_handle* h, double rows, const Dense& L) { return (rows * ((double)L.K + L.N) + (double)L.K * L.N) * h->es; }
// weight gradient: both activation operands once, the fp32 gradient once
double dw_bytes(const mrgan_handle* h, double rows, const Dense& L) { return rows * ((double)L.K + L.N) * h->es + (double)L.K * L.N * 4.0; }

Epi base_epi(mrgan_handle* h) {
    Epi e;
    memset(&e, 0, sizeof e);
    e.seed = h->cfg.seed;
    e.row0 = (uint32_t)(h->cfg.rank * h->B);
    e.st = h->state + h->cur;
    e.ablate = h->ablate; e.tune_kc_cfg = h->tune_kc_cfg; e.tune_bits = h->tune_bits;
    e.seg_step = 1;
    return e;
}

// Y = act(X W + b): X [nb][S][Kp] -> out [nb][S][Np]
int dense_fwd(mrgan_handle* h, const Dense& L, const void* x, int rows, int nb, void* out, int act, float sigma, uint32_t site,
              uint32_t seg0, uint16_t* mask, int ldm, int cs_mode, float* cs1, float* cs2, bool noise_state, hipStream_t s,
              int seg_step = 1, uint32_t iter_step = 0) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = rows; g.N = L.Np; g.K = L.Kp; g.nbatch = nb; g.splits = 1; g.kchunk = L.Kp; g.tiles_m = ceil_div(rows, 64);
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.A = x; g.a_bs = (long)h->S * L.Kp; g.a_si = L.Kp; g.a_sk = 1;
    if (h->bf16) { g.B = L.W->wt16; g.b_sj = L.Kp; g.b_sk = 1; }
    else { g.B = L.W->p; g.b_sk = L.Np; g.b_sj = 1; }
    g.e = base_epi(h);
    if (!noise_state) g.e.st = nullptr;
    g.e.act = act; g.e.n_valid = L.N; g.e.bias = L.b->p;
    g.e.out = out; g.e.out_bs = (long)h->S * L.Np; g.e.ldo = L.Np;
    g.e.sigma = sigma; g.e.site = site; g.e.seg0 = seg0; g.e.seg_step = seg_step; g.e.iter_step = iter_step;
    g.e.mask = mask; g.e.mask_bs = (long)(h->S / 32) * ldm * 2; g.e.ldm = ldm;
    g.e.cs_mode = cs_mode; g.e.cs1 = cs1; g.e.cs2 = cs2; g.e.ldcs = L.Np;
    return run_gemm(h, EPI_FWD, g, 2.0 * rows * nb * L.K * L.N, dense_bytes(h, (double)rows * nb, L), s);
}

// dX = (dY W^T) * act'(prev): dY [nb][S][Np] -> out [nb][S][Kp]
int dense_dx(mrgan_handle* h, const Dense& L, const void* dy, int rows, int nb, void* out, int act, int n_valid,
             const uint16_t* mask, int ldm, const void* hprev, int cs_mode, float* cs1, float* cs2, hipStream_t s) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = rows; g.N = L.Kp; g.K = L.Np; g.nbatch = nb; g.splits = 1; g.kchunk = L.Np; g.tiles_m = ceil_div(rows, 64);
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.A = dy; g.a_bs = (long)h->S * L.Np; g.a_si = L.Np; g.a_sk = 1;
    g.B = h->bf16 ? (const void*)L.W->w16 : (const void*)L.W->p; g.b_sk = 1; g.b_sj = L.Np;
    g.e = base_epi(h);
    g.e.act = act; g.e.n_valid = n_valid;
    g.e.out = out; g.e.out_bs = (long)h->S * L.Kp; g.e.ldo = L.Kp;
    g.e.mask = (uint16_t*)mask; g.e.mask_bs = (long)(h->S / 32) * ldm * 2; g.e.ldm = ldm;
    g.e.h = hprev; g.e.h_bs = (long)h->S * L.Kp; g.e.ldh = L.Kp;
    g.e.cs_mode = cs_mode; g.e.cs1 = cs1; g.e.cs2 = cs2; g.e.ldcs = L.Kp;
    g.e.bn_mu = h->bn_mu; g.e.bn_rstd = h->bn_rstd;
    return run_gemm(h, EPI_DX, g, 2.0 * rows * nb * L.K * L.N, dense_bytes(h, (double)rows * nb, L), s);
}

// dW slabs = X^T dY.  The nseg segments ([nseg][S] rows, `rows` valid in each) form ONE virtual reduction
// range that is cut into L.splits slabs, so the Adam kernel sums at most MAX_SLABS slabs per tensor.
double dw_args(mrgan_handle* h, GemmArgs& g, const Dense& L, const void* x, const void* dy, int rows, int nseg) {
    memset(&g, 0, sizeof g);
    // bf16: reduce over ALL S rows of every segment.  The rows >= `rows` of dY are never written by any kernel (they keep
    // the zeros of mrgan_create) and those of X are finite, so they add exact zeros -- and the reduction range becomes
    // dense, which is what the LDS-DMA weight-gradient kernel and the grouped launch need (a ragged batch such as the
    // reference's 50 otherwise fell back to one register-staged launch per product).
    const bool dense = h->bf16 != 0;
    const int vrows = dense ? nseg * h->S : (nseg - 1) * h->S + rows;
    g.M = L.Kp; g.N = L.Np; g.K = vrows; g.nbatch = 1; g.splits = L.splits; g.tiles_m = ceil_div(L.Kp, 128);
    g.kchunk = (int)round_up(ceil_div(vrows, L.splits), 64);
    g.seg_stride = h->S; g.seg_rows = dense ? h->S : rows;
    g.A = x; g.a_si = 1; g.a_sk = L.Kp;
    g.B = dy; g.b_sk = L.Np; g.b_sj = 1;
    g.e = base_epi(h);
    g.e.ldo = L.Np; g.e.slab = L.slabs; g.e.slab_stride = (long)L.Kp * L.Np;
    return 2.0 * rows * nseg * L.K * L.N;
}

struct DwJob { const Dense* L; const void* x; const void* dy; };

// the weight-gradient products of one sub-step: one grouped launch when the bf16 fast path takes them all,
// one launch per product otherwise
int dense_dw_all(mrgan_handle* h, const DwJob* jobs, int n, int rows, int nseg, hipStream_t s, const FoldJob* fold = nullptr) {
    GemmArgs gs[KS_GROUP_MAX];
    double fl[KS_GROUP_MAX], total = 0.0;
    if (n > KS_GROUP_MAX) return fail(-1, "dense_dw_all: too many products");
    for (int i = 0; i < n; ++i) { fl[i] = dw_args(h, gs[i], *jobs[i].L, jobs[i].x, jobs[i].dy, rows, nseg); total += fl[i]; }
    if (h->bf16) {
        const char* kname = "gemm";
        prof_arm(h);
        const int r = launch_gemm_bf16_dw_group(gs, n, s, &kname, fold);
        double bytes = 0.0;
        for (int i = 0; i < n; ++i) bytes += dw_bytes(h, (double)rows * nseg, *jobs[i].L);
        prof_done(h, kname, total, bytes);
        if (r < 0) return fail(r, "grouped weight-gradient launch failed");
        if (r == 0) return 0;
    }
    for (int i = 0; i < n; ++i) CHK(run_gemm(h, EPI_SLAB, gs[i], fl[i], dw_bytes(h, (double)rows * nseg, *jobs[i].L), s));
    if (fold) PROF("reduce_partials_kernel", launch_reduce_partials(fold->src, fold->nsrc, fold->stride, fold->n, fold->ngroups, fold->dst, s));
    return 0;
}

void* rowptr(mrgan_handle* h, void* base, long row, int ld) { return (char*)base + (size_t)row * ld * h->es; }

// ---------------------------------------------------------------------------------------------------
// fp8 mode: the discriminator's dense products on gemm_fp8.hip.  Activations / gradients live as fp8 copies x8[l] / g8[l]
// ([3][S][width], written by the producing product's epilogue) and, when the sub-step computes weight gradients, their
// transposes x8t[l] / g8t[l] ([width][3 S]); weights as w8 [K][N] and w8t [N][K], refreshed after the D sub-step's Adam.
// ---------------------------------------------------------------------------------------------------
int run_gemm_fp8(mrgan_handle* h, int epi, const GemmArgs& g, double algo_flops, hipStream_t s) {
    const char* kname = "gemm_fp8";
    prof_arm(h);
    const int r = launch_gemm_fp8(epi, g, s, &kname);
    // operands are bytes; outputs: fp8 (+ transposed copy) or bf16, the weight gradient fp32
    const Epi& e = g.e;
    const double out_b = epi == EPI_SLAB ? 4.0 : (e.out ? 2.0 : 0.0) + (e.q8 ? 1.0 : 0.0) + (e.q8t ? 1.0 : 0.0);
    const double bytes = (double)g.nbatch * g.M * g.K + (double)g.K * g.N + (double)g.nbatch * g.M * g.N * out_b;
    prof_done(h, kname, algo_flops, bytes);
    if (r) return fail(r, "fp8 product launch failed (%d)", r);
    return 0;
}
int fp8_quant(mrgan_handle* h, const void* src, long src_bs, int ld, int rows, int cols, int prow, int nb, unsigned char* dst, long dst_bs,
              int ldd, unsigned char* dstt, long dstt_bs, int lddt, int slot, int fmt, hipStream_t s) {
    Quant8Args q;
    memset(&q, 0, sizeof q);
    q.src = (const __bf16*)src; q.src_bs = src_bs; q.ld = ld; q.rows = rows; q.cols = cols; q.prow = prow; q.nb = nb;
    q.dst = dst; q.dst_bs = dst_bs; q.ldd = ldd; q.dstt = dstt; q.dstt_bs = dstt_bs; q.lddt = lddt;
    q.slot = h->slots + slot; q.fmt = fmt;
    PROFB("quant8_kernel", launch_quant8(q, s), (double)nb * prow * cols * (2.0 + (dst ? 1.0 : 0.0) + (dstt ? 1.0 : 0.0)));
    return 0;
}
// the noisy input rows of dense 1 (xin[0] slots x0_slot .. + nb) -> x8[0] (+ transposed)
int fp8_quant_x0(mrgan_handle* h, int x0_slot, int nb, bool want_t, hipStream_t s) {
    const int S = h->S, Dp = h->Dp;
    return fp8_quant(h, rowptr(h, h->xin[0], (long)x0_slot * S, Dp), (long)S * Dp, Dp, h->B, Dp, (int)round_up(h->B, 64), nb, h->x8[0],
                     (long)S * Dp, Dp, want_t ? h->x8t[0] : nullptr, S, 3 * S, slot_x(h->fp8_kind, 0), FP8_E4M3, s);
}
GemmArgs fp8_args(mrgan_handle* h, int M, int N, int K, int nb);
int fp8_refresh_weights(mrgan_handle* h, int net, hipStream_t s) {
    if (net == MRGAN_NET_G) {
        const Dense& L = h->g[1];
        return fp8_quant(h, L.W->w16, 0, L.Np, L.Kp, L.Np, L.Kp, 1, h->gw8, 0, L.Np, h->gw8t, 0, L.Kp, SLOT_GW, FP8_E4M3, s);
    }
    for (int l = 0; l < 5; ++l) {
        const Dense& L = h->d[l];
        CHK(fp8_quant(h, L.W->w16, 0, L.Np, L.Kp, L.Np, L.Kp, 1, h->w8[l], 0, L.Np, h->w8t[l], 0, L.Kp, slot_w(l), FP8_E4M3, s));
    }
    return 0;
}
// generator layer G2 in fp8 (the one wide product of the generator): h2 = softplus(BN(h1) W2 + b2) over nb segments from the
// current view; BN(h1) is quantised with its transpose (the weight gradient of the G sub-step reads it)
int fp8_gen_g2_fwd(mrgan_handle* h, int nb, hipStream_t s) {
    const Dense& L = h->g[1];
    const int S = h->S;
    unsigned char* x8 = h->hbn8 + (size_t)h->gen_seg * S * L.Kp;
    CHK(fp8_quant(h, h->hbn, (long)S * L.Kp, L.Kp, h->B, L.Kp, (int)round_up(h->B, 64), nb, x8, (long)S * L.Kp, L.Kp,
                  h->hbn8t + (size_t)h->gen_seg * S, S, 2 * S, SLOT_GX, FP8_E4M3, s));
    GemmArgs g = fp8_args(h, h->B, L.Np, L.Kp, nb);
    g.A = x8; g.a_bs = (long)S * L.Kp; g.a_si = L.Kp;
    g.B = h->gw8t; g.b_sj = L.Kp;
    Epi& e = g.e;
    e.act = ACT_SOFTPLUS; e.n_valid = L.N; e.bias = L.b->p;
    e.out = h->h2; e.out_bs = (long)S * L.Np; e.ldo = L.Np;
    e.qa = h->slots + SLOT_GX; e.qb = h->slots + SLOT_GW;
    return run_gemm_fp8(h, EPI_FWD, g, 2.0 * h->B * nb * L.K * L.N, s);
}
// backward through G2: dpre2 (bf16, from the G3 dX product) -> e5m2 (+ transpose); d(BN out) = dpre2 W2^T with the BatchNorm
// backward sums; dW2 = BN(h1)^T dpre2
int fp8_gen_g2_bwd(mrgan_handle* h, hipStream_t s) {
    const Dense& L = h->g[1];
    const int S = h->S;
    CHK(fp8_quant(h, h->dpre2g, 0, L.Np, h->B, L.Np, (int)round_up(h->B, 64), 1, h->dp2g8, 0, L.Np, h->dp2g8t, 0, S, SLOT_GG, FP8_E5M2, s));
    GemmArgs g = fp8_args(h, h->B, L.Kp, L.Np, 1);
    g.A = h->dp2g8; g.a_si = L.Np;
    g.B = h->gw8; g.b_sj = L.Np;
    Epi& e = g.e;
    e.act = ACT_LINEAR; e.n_valid = h->g[0].N;
    e.out = h->dhbn; e.ldo = L.Kp;
    e.h = h->h1; e.ldh = L.Kp;
    e.cs_mode = CS_SUM_XHAT; e.cs1 = h->cs_dbeta; e.cs2 = h->cs_dgamma; e.ldcs = L.Kp;
    e.bn_mu = h->bn_mu; e.bn_rstd = h->bn_rstd;
    e.qa = h->slots + SLOT_GG; e.qb = h->slots + SLOT_GW;
    return run_gemm_fp8(h, EPI_DX, g, 2.0 * h->B * L.K * L.N, s);
}
int fp8_gen_g2_dw(mrgan_handle* h, hipStream_t s) {
    const Dense& L = h->g[1];
    const int S = h->S;
    GemmArgs g = fp8_args(h, L.Kp, L.Np, S, 1);
    g.tiles_m = ceil_div(L.Kp, 128);
    g.A = h->hbn8t + (size_t)h->gen_seg * S; g.a_si = 2 * S;
    g.B = h->dp2g8t; g.b_sj = S;
    g.e.qa = h->slots + SLOT_GX; g.e.qb = h->slots + SLOT_GG;
    g.e.ldo = L.Np; g.e.slab = L.slabs; g.e.slab_stride = (long)L.Kp * L.Np;
    return run_gemm_fp8(h, EPI_SLAB, g, 2.0 * h->B * L.K * L.N, s);
}
int fp8_update_scales(mrgan_handle* h, hipStream_t s) {
    PROF("fp8_update_scales_kernel", launch_fp8_update_scales(h->slots, FP8_NSLOT, s));
    return 0;
}
GemmArgs fp8_args(mrgan_handle* h, int M, int N, int K, int nb) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = M; g.N = N; g.K = K; g.nbatch = nb; g.splits = 1; g.kchunk = K; g.tiles_m = ceil_div(M, 64);
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.a_sk = 1; g.b_sk = 1;
    g.e = base_epi(h);
    return g;
}
// dense l + relu (+ the next layer's GaussianNoise): x8[l] -> x8[l + 1] (+ transposed), the feature layer -> feat (bf16)
int fp8_fwd(mrgan_handle* h, int l, int nb, bool want_t, bool fm_sums, hipStream_t s) {
    const Dense& L = h->d[l];
    const int S = h->S, kind = h->fp8_kind;
    const bool last = l == 4;
    GemmArgs g = fp8_args(h, h->B, L.Np, L.Kp, nb);
    g.A = h->x8[l]; g.a_bs = (long)S * L.Kp; g.a_si = L.Kp;
    g.B = h->w8t[l]; g.b_sj = L.Kp;
    Epi& e = g.e;
    e.act = ACT_RELU; e.n_valid = L.N; e.bias = L.b->p;
    e.out = last ? h->feat : nullptr; e.out_bs = (long)S * L.Np; e.ldo = L.Np;
    e.sigma = last ? 0.f : h->cfg.sigma[l + 1]; e.site = (uint32_t)(l + 1); e.seg0 = 0;
    e.mask = h->mask[l]; e.mask_bs = (long)(S / 32) * h->ldm[l] * 2; e.ldm = h->ldm[l];
    e.cs_mode = (last && fm_sums) ? CS_SUM : CS_NONE; e.cs1 = h->cs_f; e.ldcs = L.Np;
    e.qa = h->slots + slot_x(kind, l); e.qb = h->slots + slot_w(l);
    if (!last) {
        e.qo = h->slots + slot_x(kind, l + 1);
        e.q8 = h->x8[l + 1]; e.q8_bs = (long)S * L.Np; e.ldq8 = L.Np;
        if (want_t) { e.q8t = h->x8t[l + 1]; e.q8t_bs = S; e.ldq8t = 3 * S; }
    }
    return run_gemm_fp8(h, EPI_FWD, g, 2.0 * h->B * nb * L.K * L.N, s);
}
// dX through dense l: g8[l] -> g8[l - 1] (+ transposed) with the relu mask of layer l - 1 and its bias-gradient column sums;
// l == 0: d loss / d(generator output) -> dxfake (bf16)
int fp8_dx(mrgan_handle* h, int l, int nb, bool want_t, bool bias_sums, hipStream_t s) {
    const Dense& L = h->d[l];
    const int S = h->S, kind = h->fp8_kind;
    GemmArgs g = fp8_args(h, h->B, L.Kp, L.Np, nb);
    g.A = h->g8[l]; g.a_bs = (long)S * L.Np; g.a_si = L.Np;
    g.B = h->w8[l]; g.b_sj = L.Np;
    Epi& e = g.e;
    e.qa = h->slots + slot_g(kind, l); e.qb = h->slots + slot_w(l);
    e.ldcs = L.Kp;
    if (l > 0) {
        e.act = ACT_RELU; e.n_valid = h->d[l - 1].N;
        e.mask = h->mask[l - 1]; e.mask_bs = (long)(S / 32) * h->ldm[l - 1] * 2; e.ldm = h->ldm[l - 1];
        e.cs_mode = bias_sums ? CS_SUM : CS_NONE; e.cs1 = h->cs_db[l - 1];
        e.qo = h->slots + slot_g(kind, l - 1);
        e.q8 = h->g8[l - 1]; e.q8_bs = (long)S * L.Kp; e.ldq8 = L.Kp;
        if (want_t) { e.q8t = h->g8t[l - 1]; e.q8t_bs = S; e.ldq8t = 3 * S; }
    } else {
        e.act = ACT_LINEAR; e.n_valid = h->cfg.d_in;
        e.out = h->dxfake; e.out_bs = (long)S * L.Kp; e.ldo = L.Kp;
        e.cs_mode = CS_SUM; e.cs1 = h->cs_db3g;
    }
    return run_gemm_fp8(h, EPI_DX, g, 2.0 * h->B * nb * L.K * L.N, s);
}
// dW_l = x8t[l] g8t[l]^T over the 3 S rows of the D sub-step (rows >= batch of a segment are zero in both), one fp32 slab
int fp8_dw(mrgan_handle* h, int l, int nseg, hipStream_t s) {
    const Dense& L = h->d[l];
    const int S = h->S, kind = h->fp8_kind;
    GemmArgs g = fp8_args(h, L.Kp, L.Np, nseg * S, 1);
    g.tiles_m = ceil_div(L.Kp, 128);
    g.splits = (nseg == 3) ? L.splits : 1; g.kchunk = nseg * S / g.splits;
    g.A = h->x8t[l]; g.a_si = 3 * S;
    g.B = h->g8t[l]; g.b_sj = 3 * S;
    g.e.qa = h->slots + slot_x(kind, l); g.e.qb = h->slots + slot_g(kind, l);
    g.e.ldo = L.Np; g.e.slab = L.slabs; g.e.slab_stride = (long)L.Kp * L.Np;
    return run_gemm_fp8(h, EPI_SLAB, g, 2.0 * h->B * nseg * L.K * L.N, s);
}
int fp8_disc_fwd(mrgan_handle* h, int nb, bool want_t, bool fm_sums, int x0_slot, hipStream_t s) {
    CHK(fp8_quant_x0(h, x0_slot, nb, want_t, s));
    for (int l = 0; l < 5; ++l) CHK(fp8_fwd(h, l, nb, want_t, fm_sums, s));
    return 0;
}
// per-block partial rows the loss head wrote in this sub-step
int head_blocks(const mrgan_handle* h) { return 3 * ceil_div(h->B, (h->use_chain || h->head_wide) ? CH_ROWS : HEAD_ROWS); }

int run_adam(mrgan_handle* h, int net, int mode, bool with_metrics, hipStream_t s, int advance_batch = 0) {
    AdamArgs a;
    memset(&a, 0, sizeof a);
    if (mode != ADAM_REDUCE_ONLY) { a.next = h->state + (h->cur ^ 1); a.advance_batch = advance_batch; a.lr = h->cfg.lr; }
    a.tiles = net == MRGAN_NET_D ? h->tiles_d_dev : h->tiles_g_dev;
    a.ntiles = net == MRGAN_NET_D ? h->ntiles_d : h->ntiles_g;
    a.mode = mode; a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.adam_eps;
    a.st = h->state + h->cur;
    if (with_metrics) {
        a.loss_part = h->loss_part; a.nloss_part = head_blocks(h); a.inv_rows = 1.0f / (float)h->Bg;
        a.step_out = h->step_out; a.accum = h->accum;
        a.flat_tail = h->flat_d + h->flat_d_n;
    }
    {
        // Keras Adam reads p, m, v and the gradient and writes p, m, v: 28 B per parameter (+ the extra gradient slabs and the
        // two bf16 weight copies of the bf16 mode)
        const std::vector<Tensor>& ts = net == MRGAN_NET_D ? h->dt : h->gt;
        double bytes = 0.0;
        for (const Tensor& t : ts) bytes += (double)t.prow * t.pcol * (24.0 + 4.0 * std::max(1, t.nslab) + (t.w16 ? 4.0 : 0.0));
        PROFB("adam_kernel", launch_adam(a, s), bytes);
    }
    return 0;
}

// which of the two generator-activation segments the following kernels work on
void set_gen_view(mrgan_handle* h, int seg) {
    h->gen_seg = seg;
    const int N1p = h->g[0].Np;
    h->zbuf = rowptr(h, h->zbuf_all, (long)seg * h->S, h->nzp);
    h->h1 = rowptr(h, h->h1_all, (long)seg * h->S, N1p);
    h->hbn = rowptr(h, h->hbn_all, (long)seg * h->S, N1p);
    h->h2 = rowptr(h, h->h2_all, (long)seg * h->S, h->g[1].Np);
    h->bn_mu = h->bn_mu_all + (size_t)seg * N1p;
    h->bn_rstd = h->bn_rstd_all + (size_t)seg * N1p;
}

// generator forward up to the BatchNorm statistics (phase *_GEN) and from there to the fake rows.
// nb = 2 (pair_gen): segment 0 is this D sub-step's batch, segment 1 the following G sub-step's (its z, noise
// iteration and noise segment id are those the G sub-step would use on its own, so the results are identical).
int gen_fwd_head(mrgan_handle* h, int nb, hipStream_t s) {
    CHK(dense_fwd(h, h->g[0], h->zbuf, h->B, nb, h->h1, ACT_SOFTPLUS, 0.f, 0, 0, nullptr, 0, CS_SUM_SQ, h->cs_bn1, h->cs_bn2,
                  true, s));
    if (h->sync_stats) {
        const int n = h->g[0].Np;          // both segments of a paired forward in one launch
        PROF("colsum_finalize_kernel", launch_colsum_finalize(h->cs_bn1, h->cs_bn2, h->tiles_m, n, n, h->r_bn_stats, s, nb));
    }
    return 0;
}
int gen_fwd_tail(mrgan_handle* h, int nb, int fake_seg_slot, uint32_t fake_seg_id, hipStream_t s) {
    const int n = h->g[0].Np;
    BnApplyArgs b;
    memset(&b, 0, sizeof b);
    b.h = h->h1; b.out = h->hbn; b.ld = n; b.rows = h->B; b.cols = h->g[0].N;
    b.nseg = nb; b.seg_rows = h->S;
    if (h->sync_stats) { b.cs1 = h->r_bn_stats; b.cs2 = h->r_bn_stats + n; b.npart = 1; b.cs_seg_stride = 2 * n; }
    else { b.cs1 = h->cs_bn1; b.cs2 = h->cs_bn2; b.npart = h->tiles_m; b.cs_seg_stride = (long)h->tiles_m * n; }
    b.ldcs = n; b.count = h->stat_count; b.eps = h->cfg.bn_eps;
    b.gamma = h->gt[2].p; b.beta = h->gt[3].p; b.mu = h->bn_mu; b.rstd = h->bn_rstd;
    PROF("bn_apply_kernel", launch_bn_apply(h->bf16, b, s));
    if (h->fp8) CHK(fp8_gen_g2_fwd(h, nb, s));
    else CHK(dense_fwd(h, h->g[1], h->hbn, h->B, nb, h->h2, ACT_SOFTPLUS, 0.f, 0, 0, nullptr, 0, CS_NONE, nullptr, nullptr, true, s));
    // generator output + GaussianNoise(sigma0) = the discriminator's noisy input rows of the fake segment.
    // Paired: segment 1 lands in the next xin[0] slot and is drawn as (segment id 0, iteration + 1), the G sub-step's fake rows.
    void* out = rowptr(h, h->xin[0], (long)fake_seg_slot * h->S, h->Dp);
    CHK(dense_fwd(h, h->g[2], h->h2, h->B, nb, out, ACT_LINEAR, h->cfg.sigma[0], 0, fake_seg_id, nullptr, 0, CS_NONE, nullptr,
                  nullptr, true, s, nb > 1 ? -(int)fake_seg_id : 1, nb > 1 ? 1u : 0u));
    return 0;
}

// discriminator dense 1..5 over nb segments (learning phase 1: noise on)
int disc_fwd_train(mrgan_handle* h, int nb, bool fm_sums, int x0_slot, hipStream_t s, int l_end = 5) {
    if (h->fp8) return fp8_disc_fwd(h, nb, /*want_t=*/h->fp8_kind == 0, fm_sums, x0_slot, s);
    for (int l = 0; l < l_end; ++l) {
        const void* in = l == 0 ? rowptr(h, h->xin[0], (long)x0_slot * h->S, h->Dp) : h->xin[l];
        void* out = l < 4 ? h->xin[l + 1] : h->feat;
        const float sigma = l < 4 ? h->cfg.sigma[l + 1] : 0.f;
        const bool last = l == 4;
        CHK(dense_fwd(h, h->d[l], in, h->B, nb, out, ACT_RELU, sigma, (uint32_t)(l + 1), 0, h->mask[l], h->ldm[l],
                      (last && fm_sums) ? CS_SUM : CS_NONE, h->cs_f, nullptr, true, s));
    }
    return 0;
}

// ---- row-block chain launches for the tail D3..D5 (+ head) of the discriminator (gemm_chain.hip) ----
ChainOp chain_fwd_op(mrgan_handle* h, int l, int a_off, int o_off, bool fm_sums) {
    const Dense& L = h->d[l];
    ChainOp o;
    memset(&o, 0, sizeof o);
    o.kind = CH_OP_GEMM; o.K = L.Kp; o.N = L.Np; o.n_valid = L.N; o.W = L.W->wt16; o.a_off = a_off; o.o_off = o_off;
    o.mode = CH_FWD_RELU; o.bias = L.b->p; o.sigma = l < 4 ? h->cfg.sigma[l + 1] : 0.f; o.site = (uint32_t)(l + 1);
    o.out = (__bf16*)(l < 4 ? h->xin[l + 1] : h->feat); o.out_bs = (long)h->S * L.Np; o.ldo = L.Np;
    o.mask = h->mask[l]; o.mask_bs = (long)(h->S / 32) * h->ldm[l] * 2; o.ldm = h->ldm[l];
    if (fm_sums) { o.cs = h->cs_f; o.ldcs = L.Np; }
    return o;
}
// dX of layer l: dpre[l] -> dpre[l-1]
ChainOp chain_dx_op(mrgan_handle* h, int l, int a_off, int o_off, bool bias_sums) {
    const Dense& L = h->d[l];
    ChainOp o;
    memset(&o, 0, sizeof o);
    o.kind = CH_OP_GEMM; o.K = L.Np; o.N = L.Kp; o.n_valid = h->d[l - 1].N; o.W = L.W->w16; o.a_off = a_off; o.o_off = o_off;
    o.mode = CH_DX_RELU;
    o.out = (__bf16*)h->dpre[l - 1]; o.out_bs = (long)h->S * L.Kp; o.ldo = L.Kp;
    o.mask = h->mask[l - 1]; o.mask_bs = (long)(h->S / 32) * h->ldm[l - 1] * 2; o.ldm = h->ldm[l - 1];
    if (bias_sums) { o.cs = h->cs_db[l - 1]; o.ldcs = L.Kp; }
    return o;
}
// rows per block of a G sub-step chain launch: 32 when 64-row blocks would leave more than half of the CUs without a block
// (the 3-stage weight ring of the 32-row blocks keeps two k-tiles in flight: every reduction of the chain must have two)
int chain_block_rows(const mrgan_handle* h, int nseg) {
    const int kmin = std::min(std::min(h->d[2].Kp, h->d[2].Np), std::min(h->d[3].Np, h->d[4].Np));
    return (nseg * ceil_div(h->B, 64) <= 128 && kmin >= 128) ? 32 : 64;
}
void chain_common(mrgan_handle* h, ChainArgs& c, int nseg) {
    c.rows = h->B; c.nseg = nseg; c.S = h->S; c.seg0 = 0; c.block_rows = 64;
    c.seed = h->cfg.seed; c.row0 = (uint32_t)(h->cfg.rank * h->B); c.st = h->state + h->cur;
    c.ablate = h->ablate;
}
double chain_flops(const mrgan_handle* h, const ChainArgs& c, bool with_head) {
    double f = 0.0;
    for (int l = 2; l < 5; ++l) f += 2.0 * h->B * c.nseg * h->d[l].K * h->d[l].N;     // each product appears once per direction
    return f * (with_head ? 2.0 : 1.0);
}
int run_chain(mrgan_handle* h, const ChainArgs& c0, double flops, hipStream_t s) {
    ChainArgs c = c0;
#ifdef MRGAN_STAMPS
    // diagnostic build: per-phase cycles of every block, printed per launch (never for timing runs)
    static unsigned long long* stamps = nullptr;
    if (!stamps) hipMalloc((void**)&stamps, 4096 * 8 * sizeof(unsigned long long));
    hipMemsetAsync(stamps, 0, 4096 * 8 * sizeof(unsigned long long), s);
    c.stamps = stamps;
#endif
    prof_arm(h);
    const int r = launch_chain(c, s);
#ifdef MRGAN_STAMPS
    {
        std::vector<unsigned long long> hs(4096 * 8);
        hipStreamSynchronize(s);
        hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        double tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int nb = 0;
        for (int b = 0; b < 4096; ++b) if (hs[b * 8]) { ++nb; for (int i = 0; i < 8; ++i) tot[i] += (double)hs[b * 8 + i]; }
        if (nb) fprintf(stderr, "chain stamps (kcycles per block, %d blocks, %d ops): prologue %.1f | pass setup %.1f | head %.1f | tile wait %.1f | barrier %.1f | "
                        "issue+reads+mfma %.1f | epilogue %.1f | image barrier+copy-out %.1f\n", nb, c.nops, tot[0] / nb / 1e3, tot[1] / nb / 1e3,
                        tot[2] / nb / 1e3, tot[3] / nb / 1e3, tot[4] / nb / 1e3, tot[5] / nb / 1e3, tot[6] / nb / 1e3, tot[7] / nb / 1e3);
    }
#endif
    // algorithmic bytes (logical widths, bf16): the first A image, every product's weights and stored output
    double bytes = 0.0;
    const double nrows = (double)c.rows * c.nseg;
    const bool has_fwd = c.variant != CH_V_GBWD, has_dx = c.variant != CH_V_GFWD;
    if (has_fwd) bytes += nrows * h->d[2].K * 2.0;
    else bytes += nrows * h->F * 2.0;                                  // the stored features whose sign is the relu mask
    for (int l = 2; l < 5; ++l) {
        const double w = (double)h->d[l].K * h->d[l].N * 2.0;
        if (has_fwd) bytes += w + nrows * h->d[l].N * 2.0;
        if (has_dx) bytes += w + nrows * h->d[l].K * 2.0;
    }
    static const char* names[3] = {"chain_kernel<0>", "chain_kernel<1>", "chain_kernel<2>"};     // as rocprofv3 prints them
    prof_done(h, names[c.variant], flops, bytes);
    CHK(r);
    return 0;
}

int stage_common(StageArgs& st, mrgan_handle* h, const float* z, int stream_mode, int slot, bool paired_z = false) {
    if (slot >= 0) {
        StageSeg& zs = st.s[slot];
        memset(&zs, 0, sizeof zs);
        zs.src = z; zs.ld = h->cfg.noise_size; zs.rows = h->B; zs.cols = h->cfg.noise_size; zs.cols_pad = h->nzp;
        zs.out = h->zbuf; zs.ldo = h->nzp; zs.sigma = 0.f; zs.site = SITE_Z; zs.seg = 0; zs.gen = z ? 0 : 1; zs.stream = z ? stream_mode : 0;
        st.nseg = slot + 1;
        if (paired_z) {                                 // the following G sub-step's z (drawn on device at iteration + 1)
            StageSeg& z2 = st.s[slot + 1];
            z2 = zs;
            z2.out = rowptr(h, h->zbuf_all, h->S, h->nzp); z2.gen = 1; z2.src = nullptr; z2.stream = 0; z2.iter_off = 1;
            st.nseg = slot + 2;
        }
    }
    st.seed = h->cfg.seed; st.row0 = (uint32_t)(h->cfg.rank * h->B);
    st.cur = h->state + h->cur;
    return 0;
}
void data_seg(StageSeg& sg, mrgan_handle* h, const float* x, const int32_t* idx, long ld, int slot, uint32_t seg_id, int stream_mode) {
    memset(&sg, 0, sizeof sg);
    sg.src = x; sg.idx = idx; sg.ld = ld; sg.rows = h->B; sg.cols = h->cfg.d_in; sg.cols_pad = h->Dp;
    sg.out = rowptr(h, h->xin[0], (long)slot * h->S, h->Dp); sg.ldo = h->Dp;
    sg.sigma = h->cfg.sigma[0]; sg.site = 0; sg.seg = seg_id; sg.gen = 0; sg.stream = stream_mode;
}

// ---------------------------------------------------------------------------------------------------
// discriminator sub-step
// ---------------------------------------------------------------------------------------------------
int disc_phase(mrgan_handle* h, const mrgan_disc_args* a, int phase, hipStream_t s) {
    const int B = h->B;
    h->fp8_kind = 0;
    if (phase == MRGAN_D_GEN) {
        prof_backlog(h, s);
        StageArgs st;
        memset(&st, 0, sizeof st);
        data_seg(st.s[0], h, a->x_lab_dev, a->idx_lab_dev, a->ld_x_lab, 0, 0, a->stream_mode);
        data_seg(st.s[1], h, a->x_unl_dev, a->idx_unl_dev, a->ld_x_unl, 1, 1, a->stream_mode);
        set_gen_view(h, 0);
        stage_common(st, h, a->z_dev, a->stream_mode, 2, h->pair_gen != 0);
        h->real_staged = 0;
        if (h->pair_gen && h->pair_g) {
            // mrgan_train_pair: the G sub-step's real rows (its x_unl batch, drawn at iteration + 1) ride in this launch too
            const mrgan_gen_args* g = h->pair_g;
            StageSeg& rs = st.s[st.nseg];
            data_seg(rs, h, g->x_unl_dev, g->idx_unl_dev, g->ld_x_unl, 4, 1, g->stream_mode);
            rs.iter_off = 1;
            st.nseg += 1;
            h->real_staged = 1;
        }
        PROF("stage_kernel", launch_stage(h->bf16, st, s));
        CHK(gen_fwd_head(h, h->pair_gen ? 2 : 1, s));
    } else if (phase == MRGAN_D_MAIN) {
        CHK(gen_fwd_tail(h, h->pair_gen ? 2 : 1, 2, 2, s));               // fake rows -> slot 2 (+ the G sub-step's -> slot 3)
        h->gen_ready = h->pair_gen;
        h->pair_gen = 0;                                                  // one D sub-step per hint
        CHK(disc_fwd_train(h, 3, false, 0, s, h->use_chain ? 2 : 5));
        HeadArgs hd;
        memset(&hd, 0, sizeof hd);
        hd.f = h->feat; hd.f_bs = (long)h->S * h->Fp; hd.ldf = h->Fp; hd.rows = B; hd.nseg = 3;
        hd.seg_kind[0] = HEAD_LAB; hd.seg_kind[1] = HEAD_UNL; hd.seg_kind[2] = HEAD_FAKE;
        hd.feat = h->Fp; hd.feat_valid = h->F; hd.classes = h->cfg.num_classes;
        hd.w = h->dt[10].p; hd.ldw = KMAX; hd.b = h->dt[11].p;
        hd.labels = a->labels_dev; hd.st = h->state + h->cur; hd.labels_stream = a->stream_mode;
        hd.inv_count = 1.0f / (float)h->Bg; hd.unl_weight = h->cfg.unlabeled_weight;
        hd.logits = h->logits; hd.logits_bs = (long)h->S * KMAX;
        hd.dpre = h->dpre[4]; hd.dpre_bs = (long)h->S * h->Fp; hd.ldd = h->Fp;
        hd.part = h->head_part; hd.part_stride = h->head_stride; hd.off_db = h->Fp * KMAX; hd.off_dbf = h->Fp * KMAX + KMAX;
        hd.loss_part = h->loss_part;
        if (h->fp8) {                 // the head writes the e5m2 copies of dpre itself (no bf16 dpre, no quantiser pass)
            hd.dpre = nullptr;
            hd.q8 = h->g8[4]; hd.q8_bs = (long)h->S * h->Fp; hd.ldq8 = h->Fp;
            hd.q8t = h->g8t[4]; hd.q8t_bs = h->S; hd.ldq8t = 3 * h->S;
            hd.q8_slot = h->slots + slot_g(0, 4);
        }
        if (h->use_chain) {
            // D3 D4 D5 forward -> loss head -> dX through D5 D4 D3, one launch: the rows of a block never leave its CU
            ChainArgs c;
            memset(&c, 0, sizeof c);
            chain_common(h, c, 3);
            c.variant = CH_V_DTAIL;
            c.a_kind = CH_A_GLOBAL; c.a = (const __bf16*)h->xin[2]; c.a_bs = (long)h->S * h->d[2].Kp; c.lda = h->d[2].Kp; c.a_cols = h->d[2].Kp;
            c.op[0] = chain_fwd_op(h, 2, CH_BUF0, CH_BUF1, false);
            c.op[1] = chain_fwd_op(h, 3, CH_BUF1, CH_BUF0, false);
            c.op[2] = chain_fwd_op(h, 4, CH_BUF0, CH_BUF1, false);
            // the relu masks of D3 .. D5 never leave the launch's registers (their dX products follow in the same launch, and
            // nothing else reads them in a D sub-step): no copies to HBM
            for (int i = 0; i < 3; ++i) c.op[i].mask = nullptr;
            c.op[3].kind = CH_OP_HEAD;
            c.head = hd; c.head_f_off = CH_BUF1; c.head_o_off = CH_BUF0; c.head_scratch_off = CH_BUF0 + CH_BUF0_BYTES / 2;
            c.op[4] = chain_dx_op(h, 4, CH_BUF0, CH_BUF1, true);
            c.op[5] = chain_dx_op(h, 3, CH_BUF1, CH_BUF0, true);
            c.op[6] = chain_dx_op(h, 2, CH_BUF0, CH_BUF1, true);
            c.nops = 7;
            CHK(run_chain(h, c, chain_flops(h, c, true), s));
        } else if (h->head_wide) {
            HeadWideArgs hw;
            memset(&hw, 0, sizeof hw);
            hw.h = hd; hw.mask = h->mask[4]; hw.mask_bs = (long)(h->S / 32) * h->ldm[4] * 2; hw.ldm = h->ldm[4];
            hw.w6c = h->w6c; hw.w6r = h->w6r;
            PROF("w6_split_kernel", launch_w6_split(hw, s));
            PROF("head_wide_kernel", launch_head_wide(hw, s));
        } else {
            PROF("head_kernel", launch_head(h->bf16, hd, s));
        }
        if (h->fp8) {
            for (int l = 4; l >= 1; --l) CHK(fp8_dx(h, l, 3, true, true, s));
            for (int l = 0; l < 5; ++l) CHK(fp8_dw(h, l, 3, s));
            PROF("reduce_partials_kernel", launch_reduce_partials(h->head_part, head_blocks(h), h->head_stride, h->head_stride, h->head_groups, h->head_red, s));
        } else {
        for (int l = h->use_chain ? 1 : 4; l >= 1; --l)
            CHK(dense_dx(h, h->d[l], h->dpre[l], B, 3, h->dpre[l - 1], ACT_RELU, h->d[l - 1].N, h->mask[l - 1], h->ldm[l - 1],
                         nullptr, CS_SUM, h->cs_db[l - 1], nullptr, s));
        {
            DwJob jobs[5];
            for (int l = 0; l < 5; ++l) jobs[l] = DwJob{&h->d[l], h->xin[l], h->dpre[l]};
            // the loss head's per-block weight-gradient partials are folded by extra blocks of the same launch
            const FoldJob fold = {h->head_part, h->head_red, (long)h->head_stride, head_blocks(h), h->head_stride, h->head_groups, 0};
            CHK(dense_dw_all(h, jobs, 5, B, 3, s, &fold));
        }
        }
        if (h->flat_grads) CHK(run_adam(h, MRGAN_NET_D, ADAM_REDUCE_ONLY, true, s));
    } else if (phase == MRGAN_D_ADAM) {
        CHK(run_adam(h, MRGAN_NET_D, h->flat_grads ? ADAM_FROM_FLAT : ADAM_FUSED, true, s));
        if (h->fp8) CHK(fp8_update_scales(h, s));        // (the Adam kernel rewrote the fp8 weight copies and their amax)
        h->cur ^= 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// generator sub-step
// ---------------------------------------------------------------------------------------------------
int gen_phase(mrgan_handle* h, const mrgan_gen_args* a, int phase, hipStream_t s) {
    const int B = h->B, tm = h->tiles_m, N1p = h->g[0].Np;
    h->fp8_kind = 1;
    if (phase == MRGAN_G_GEN) {
        prof_backlog(h, s);
        StageArgs st;
        memset(&st, 0, sizeof st);
        // after a paired forward (train_pair) the fake rows already sit in slot 3 and the generator activations in
        // segment 1; otherwise this sub-step runs its own generator forward into slot 0 / segment 0
        const bool ready = h->gen_ready && !a->z_dev;
        h->gen_ready = ready ? 1 : 0;
        h->xbase = ready ? 3 : 0;
        set_gen_view(h, ready ? 1 : 0);
        const bool staged = ready && h->real_staged;           // the D sub-step's stage launch already placed the real rows in slot 4
        h->real_staged = 0;
        if (!staged) {
            data_seg(st.s[0], h, a->x_unl_dev, a->idx_unl_dev, a->ld_x_unl, h->xbase + 1, 1, a->stream_mode);   // real rows
            st.nseg = 1;
            stage_common(st, h, a->z_dev, a->stream_mode, ready ? -1 : 1);
            PROF("stage_kernel", launch_stage(h->bf16, st, s));
        }
        if (!ready) CHK(gen_fwd_head(h, 1, s));
    } else if (phase == MRGAN_G_FEAT) {
        if (!h->gen_ready) CHK(gen_fwd_tail(h, 1, 0, 0, s));                                    // fake rows -> slot 0
        h->gen_ready = 0;
        CHK(disc_fwd_train(h, 2, true, h->xbase, s, h->use_chain ? 2 : 5));
        if (h->use_chain) {
            ChainArgs c;
            memset(&c, 0, sizeof c);
            chain_common(h, c, 2);
            c.variant = CH_V_GFWD;
            c.block_rows = chain_block_rows(h, 2);
            const int b0 = chain_buf0(c.block_rows), b1 = chain_buf1(c.block_rows);
            c.a_kind = CH_A_GLOBAL; c.a = (const __bf16*)h->xin[2]; c.a_bs = (long)h->S * h->d[2].Kp; c.lda = h->d[2].Kp; c.a_cols = h->d[2].Kp;
            c.op[0] = chain_fwd_op(h, 2, b0, b1, false);
            c.op[1] = chain_fwd_op(h, 3, b1, b0, false);
            c.op[2] = chain_fwd_op(h, 4, b0, b1, true);       // + the feature-matching column sums (one partial row per row block)
            c.nops = 3;
            CHK(run_chain(h, c, chain_flops(h, c, false), s));
        }
        if (h->sync_stats) {
            const int np = h->use_chain ? ceil_div(B, chain_block_rows(h, 2)) : tm;
            PROF("colsum_finalize_kernel", launch_colsum_finalize(h->cs_f, h->cs_f + (size_t)np * h->Fp, np, h->Fp, h->Fp, h->r_fm, s));
        }
    } else if (phase == MRGAN_G_BWD) {
        FmArgs f;
        memset(&f, 0, sizeof f);
        if (h->sync_stats) { f.cs = h->r_fm; f.npart_fake = 1; f.npart_real = 1; }
        else {          // per-row-block partial sums as the producer left them: 64-row tiles, or the chain launch's row blocks
            const int np = h->use_chain ? ceil_div(B, chain_block_rows(h, 2)) : tm;
            f.cs = h->cs_f; f.npart_fake = np; f.npart_real = np;
        }
        f.ldcs = h->Fp; f.count = h->stat_count; f.grad_scale = h->fm_scale; f.feat = h->Fp; f.feat_valid = h->F;
        f.mask = h->mask[4]; f.ldm = h->ldm[4]; f.dpre = h->dpre[4]; f.ldd = h->Fp; f.rows = B;
        f.loss_out = h->step_out + 3; f.accum = h->accum + 3;
        f.lscratch = h->fm_scratch; f.lcount = h->fm_count;
        if (h->fp8) { f.dpre = nullptr; f.q8 = h->g8[4]; f.ldq8 = h->Fp; f.q8_slot = h->slots + slot_g(1, 4); }
        if (h->use_chain) {
            // feature-matching gradient -> dX through D5 D4 D3 on the generated rows, one launch
            ChainArgs c;
            memset(&c, 0, sizeof c);
            chain_common(h, c, 1);
            c.variant = CH_V_GBWD;
            c.block_rows = chain_block_rows(h, 1);
            const int b0 = chain_buf0(c.block_rows), b1 = chain_buf1(c.block_rows);
            c.a_kind = CH_A_FMGRAD; c.fm = f; c.fm_feat = (const __bf16*)h->feat; c.fm_ldf = h->Fp;
            c.op[0] = chain_dx_op(h, 4, b0, b1, false);
            c.op[1] = chain_dx_op(h, 3, b1, b0, false);
            c.op[2] = chain_dx_op(h, 2, b0, b1, false);
            c.nops = 3;
            CHK(run_chain(h, c, chain_flops(h, c, false), s));
        } else {
            PROF("fm_kernel", launch_fm(h->bf16, f, s));
        }
        if (h->fp8) {
            for (int l = 4; l >= 0; --l) CHK(fp8_dx(h, l, 1, false, false, s));
        } else {
        for (int l = h->use_chain ? 1 : 4; l >= 1; --l)
            CHK(dense_dx(h, h->d[l], h->dpre[l], B, 1, h->dpre[l - 1], ACT_RELU, h->d[l - 1].N, h->mask[l - 1], h->ldm[l - 1],
                         nullptr, CS_NONE, nullptr, nullptr, s));
        // d loss / d(generator output): noise is additive, so this is also d/d(fake x)
        CHK(dense_dx(h, h->d[0], h->dpre[0], B, 1, h->dxfake, ACT_LINEAR, h->cfg.d_in, nullptr, 0, nullptr, CS_SUM, h->cs_db3g,
                     nullptr, s));
        }
        CHK(dense_dx(h, h->g[2], h->dxfake, B, 1, h->dpre2g, ACT_SOFTPLUS, h->g[1].N, nullptr, 0, h->h2, CS_SUM, h->cs_db2g,
                     nullptr, s));
        if (h->fp8) CHK(fp8_gen_g2_bwd(h, s));
        else CHK(dense_dx(h, h->g[1], h->dpre2g, B, 1, h->dhbn, ACT_LINEAR, h->g[0].N, nullptr, 0, h->h1, CS_SUM_XHAT, h->cs_dbeta,
                          h->cs_dgamma, s));
        if (h->sync_stats) {
            PROF("colsum_finalize_kernel", launch_colsum_finalize(h->cs_dbeta, h->cs_dgamma, tm, N1p, N1p, h->r_bn_bwd, s));
        }
    } else if (phase == MRGAN_G_TAIL) {
        BnBwdArgs b;
        memset(&b, 0, sizeof b);
        b.dy = h->dhbn; b.h = h->h1; b.dpre = h->dpre1g; b.ld = N1p; b.rows = B; b.cols = h->g[0].N;
        if (h->sync_stats) { b.cs1 = h->r_bn_bwd; b.cs2 = h->r_bn_bwd + N1p; b.npart = 1; }
        else { b.cs1 = h->cs_dbeta; b.cs2 = h->cs_dgamma; b.npart = tm; }
        b.ldcs = N1p; b.count = h->stat_count; b.gamma = h->gt[2].p; b.mu = h->bn_mu; b.rstd = h->bn_rstd;
        b.db_part = h->db1g_part;
        PROF("bn_bwd_kernel", launch_bn_bwd(h->bf16, b, s));
        {
            const DwJob jobs[3] = {{&h->g[2], h->h2, h->dxfake}, {&h->g[0], h->zbuf, h->dpre1g}, {&h->g[1], h->hbn, h->dpre2g}};
            if (h->fp8) { CHK(dense_dw_all(h, jobs, 2, B, 1, s)); CHK(fp8_gen_g2_dw(h, s)); }
            else CHK(dense_dw_all(h, jobs, 3, B, 1, s));
        }
        if (h->flat_grads) CHK(run_adam(h, MRGAN_NET_G, ADAM_REDUCE_ONLY, false, s));
    } else if (phase == MRGAN_G_ADAM) {
        CHK(run_adam(h, MRGAN_NET_G, h->flat_grads ? ADAM_FROM_FLAT : ADAM_FUSED, false, s, a->stream_mode ? 1 : 0));
        if (h->fp8) CHK(fp8_update_scales(h, s));
        h->cur ^= 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// supervised step of the NN baseline (mr_nn.py:101-118): the discriminator stack alone, one segment, mse head
// ---------------------------------------------------------------------------------------------------
int sup_step(mrgan_handle* h, const mrgan_sup_args* a, hipStream_t s) {
    const int B = h->B;
    prof_backlog(h, s);
    StageArgs st;
    memset(&st, 0, sizeof st);
    data_seg(st.s[0], h, a->x_dev, a->idx_dev, a->ld_x, 0, 0, a->stream_mode);
    st.nseg = 1;
    stage_common(st, h, nullptr, 0, -1);
    PROF("stage_kernel", launch_stage(h->bf16, st, s));
    CHK(disc_fwd_train(h, 1, false, 0, s, 5));
    HeadArgs hd;
    memset(&hd, 0, sizeof hd);
    hd.f = h->feat; hd.f_bs = (long)h->S * h->Fp; hd.ldf = h->Fp; hd.rows = B; hd.nseg = 1;
    hd.seg_kind[0] = HEAD_MSE;
    hd.feat = h->Fp; hd.feat_valid = h->F; hd.classes = h->cfg.num_classes;
    hd.w = h->dt[10].p; hd.ldw = KMAX; hd.b = h->dt[11].p;
    hd.labels = a->labels_dev; hd.st = h->state + h->cur; hd.labels_stream = a->stream_mode;
    hd.inv_count = 1.0f / (float)(a->rows_valid > 0 ? a->rows_valid : B); hd.unl_weight = 0.f;
    hd.logits = h->logits; hd.logits_bs = (long)h->S * KMAX;
    hd.dpre = h->dpre[4]; hd.dpre_bs = (long)h->S * h->Fp; hd.ldd = h->Fp;
    hd.part = h->head_part; hd.part_stride = h->head_stride; hd.off_db = h->Fp * KMAX; hd.off_dbf = h->Fp * KMAX + KMAX;
    hd.loss_part = h->loss_part;
    PROF("head_kernel", launch_head(h->bf16, hd, s));
    for (int l = 4; l >= 1; --l)
        CHK(dense_dx(h, h->d[l], h->dpre[l], B, 1, h->dpre[l - 1], ACT_RELU, h->d[l - 1].N, h->mask[l - 1], h->ldm[l - 1], nullptr,
                     CS_SUM, h->cs_db[l - 1], nullptr, s));
    DwJob jobs[5];
    for (int l = 0; l < 5; ++l) jobs[l] = DwJob{&h->d[l], h->xin[l], h->dpre[l]};
    const FoldJob fold = {h->head_part, h->head_red, (long)h->head_stride, ceil_div(B, HEAD_ROWS), h->head_stride, h->head_groups, 0};
    CHK(dense_dw_all(h, jobs, 5, B, 1, s, &fold));
    // (the bias / loss partial rows of the two other segments of the GAN step keep the zeros of mrgan_create)
    const bool chain = h->use_chain, wide = h->head_wide;
    h->use_chain = h->head_wide = false;                    // head_blocks(): the per-layer head wrote 32-row blocks
    const int r = run_adam(h, MRGAN_NET_D, ADAM_FUSED, true, s, a->stream_mode ? 1 : 0);
    h->use_chain = chain; h->head_wide = wide;
    CHK(r);
    h->cur ^= 1;
    return 0;
}

int check_disc_args(const mrgan_handle* h, const mrgan_disc_args* a) {
    if (!a || !a->x_lab_dev || !a->x_unl_dev || !a->labels_dev) return fail(-2, "disc_step: x_lab, x_unl and labels are required");
    if (a->ld_x_lab < h->cfg.d_in || a->ld_x_unl < h->cfg.d_in) return fail(-2, "disc_step: row pitch smaller than d_in");
    return 0;
}
int check_gen_args(const mrgan_handle* h, const mrgan_gen_args* a) {
    if (!a || !a->x_unl_dev) return fail(-2, "gen_step: x_unl is required");
    if (a->ld_x_unl < h->cfg.d_in) return fail(-2, "gen_step: row pitch smaller than d_in");
    return 0;
}

// forward-only discriminator over n rows (learning phase 0), chunked through the training activations
int eval_rows(mrgan_handle* h, const float* x, const int32_t* idx, long ld, const int32_t* labels, long n, float* logits_out,
              hipStream_t s) {
    const long cap = 3L * h->S;
    for (long r0 = 0; r0 < n; r0 += cap) {
        const int rows = (int)std::min(cap, n - r0);
        StageArgs st;
        memset(&st, 0, sizeof st);
        StageSeg& sg = st.s[0];
        sg.src = idx ? x : x + r0 * ld; sg.idx = idx ? idx + r0 : nullptr; sg.ld = ld; sg.rows = rows;
        sg.cols = h->cfg.d_in; sg.cols_pad = h->Dp; sg.out = h->xin[0]; sg.ldo = h->Dp;
        st.nseg = 1; st.seed = h->cfg.seed; st.cur = h->state + h->cur;
        PROF("stage_kernel", launch_stage(h->bf16, st, s));
        for (int l = 0; l < 5; ++l) {
            // one "segment" of `rows` contiguous rows: batch stride is irrelevant with nb = 1
            CHK(dense_fwd(h, h->d[l], h->xin[l], rows, 1, l < 4 ? h->xin[l + 1] : h->feat, ACT_RELU, 0.f, 0, 0, nullptr, 0, CS_NONE,
                          nullptr, nullptr, false, s));
        }
        HeadArgs hd;
        memset(&hd, 0, sizeof hd);
        hd.f = h->feat; hd.ldf = h->Fp; hd.rows = rows; hd.nseg = 1; hd.seg_kind[0] = HEAD_EVAL;
        hd.feat = h->Fp; hd.feat_valid = h->F; hd.classes = h->cfg.num_classes;
        hd.w = h->dt[10].p; hd.ldw = KMAX; hd.b = h->dt[11].p;
        hd.labels = labels ? labels + r0 : nullptr;
        if (!labels) hd.seg_kind[0] = HEAD_LOGITS;
        hd.st = h->state + h->cur; hd.labels_stream = 0;
        hd.logits = h->logits; hd.err_count = labels ? h->err_count : nullptr;
        PROF("head_kernel", launch_head(h->bf16, hd, s));
        if (logits_out)
            HIPCHK(hipMemcpy2DAsync(logits_out + r0 * h->cfg.num_classes, sizeof(float) * h->cfg.num_classes, h->logits,
                                    sizeof(float) * KMAX, sizeof(float) * h->cfg.num_classes, rows, hipMemcpyDeviceToDevice, s));
    }
    // The evaluation used the training activations as scratch and filled rows [0, 3S) of every layer input, i.e. also the
    // padding rows B..S of each training segment.  The bf16 weight gradients reduce over all S rows of a segment (zero dY
    // padding rows x FINITE X padding rows): a non-finite value left there by an evaluation input would turn into NaN
    // gradients from then on (0 * NaN).  Ragged batches only: re-zero those rows.
    if (h->B < h->S) {
        for (int l = 0; l < 5; ++l)
            for (int sg = 0; sg < (l == 0 ? 5 : 3); ++sg) {
                char* p = (char*)h->xin[l] + ((size_t)sg * h->S + h->B) * h->d[l].Kp * h->es;
                HIPCHK(hipMemsetAsync(p, 0, (size_t)(h->S - h->B) * h->d[l].Kp * h->es, s));
            }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// fp8 calibration of a sub-step kind (0 = D, 1 = G): dry passes (forward + backward phases, no update) between begin and
// done, each followed by end_pass, settle the delayed scales, one layer of the gradient chain per pass.  Whole sub-steps run
// them by themselves, phase-wise hosts through mrgan_fp8_calibration.  The G sub-step's feature-matching kernel adds its loss
// to the epoch accumulator, which the dry passes must leave alone.
// ---------------------------------------------------------------------------------------------------
int fp8_cal_begin(mrgan_handle* h, int kind, hipStream_t s) {
    h->fp8_cal[kind] = 2;                         // in progress: the phases run as they are
    if (kind == 1) HIPCHK(hipMemcpyAsync(h->accum_save, h->accum, 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
int fp8_cal_end_pass(mrgan_handle* h, int /*kind*/, hipStream_t s) {
    CHK(fp8_update_scales(h, s));
    return 0;
}
int fp8_cal_done(mrgan_handle* h, int kind, hipStream_t s) {
    if (kind == 1) HIPCHK(hipMemcpyAsync(h->accum, h->accum_save, 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    h->fp8_cal[kind] = 1;
    return 0;
}

Tensor* find_tensor(mrgan_handle* h, int net, int idx) {
    std::vector<Tensor>& ts = net == MRGAN_NET_G ? h->gt : h->dt;
    if (net != MRGAN_NET_G && net != MRGAN_NET_D) return nullptr;
    if (idx < 0 || idx >= (int)ts.size()) return nullptr;
    return &ts[idx];
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* mrgan_last_error(void) { return g_err.c_str(); }

int mrgan_default_config(mrgan_config* c, int32_t d_in, int32_t batch) {
    if (!c) return fail(-1, "null config");
    memset(c, 0, sizeof *c);
    c->d_in = d_in; c->batch = batch; c->noise_size = 100;
    c->g_hidden[0] = 500; c->g_hidden[1] = 500;
    const int dh[5] = {1000, 500, 250, 250, 250};
    const float sg[5] = {0.3f, 0.5f, 0.5f, 0.5f, 0.5f};
    for (int i = 0; i < 5; ++i) { c->d_hidden[i] = dh[i]; c->sigma[i] = sg[i]; }
    c->num_classes = 6; c->dtype = MRGAN_F32;
    c->lr = 0.0006f; c->beta1 = 0.5f; c->beta2 = 0.999f; c->adam_eps = 1e-8f; c->bn_eps = 2e-5f;
    c->unlabeled_weight = 1.0f; c->seed = 0x5EED5EEDULL; c->rank = 0; c->world = 1; c->flags = 0;
    return 0;
}

int mrgan_workspace_bytes(const mrgan_config* cfg, size_t* bytes) {
    if (!cfg || !bytes) return fail(-1, "null argument");
    int r = validate(*cfg);
    if (r) return r;
    mrgan_handle tmp;
    tmp.cfg = *cfg;
    return layout(&tmp, nullptr, bytes);
}

int mrgan_create(const mrgan_config* cfg, void* workspace, size_t bytes, mrgan_stream stream, mrgan_handle** out) {
    if (!cfg || !out) return fail(-1, "null argument");
    int r = validate(*cfg);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    mrgan_handle* h = new mrgan_handle();
    h->cfg = *cfg;
    size_t need = 0;
    layout(h, nullptr, &need);
    h->own_ws = workspace == nullptr;
    if (workspace) {
        if (bytes < need) { delete h; return fail(-3, "workspace too small: %zu < %zu", bytes, need); }
        if (((uintptr_t)workspace & 255) != 0) { delete h; return fail(-3, "workspace must be 256-byte aligned"); }
        h->ws = (char*)workspace;
    } else {
        hipError_t e = hipMalloc((void**)&h->ws, need);
        if (e != hipSuccess) { delete h; return fail(-10, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); }
    }
    h->ws_bytes = need;
    layout(h, h->ws, &need);
    set_gen_view(h, 0);
    h->cur = 0; h->graph_ready = false; h->graph_exec = nullptr; h->prof = false;
    h->pair_gen = h->gen_ready = 0; h->pair_g = nullptr; h->real_staged = 0;
    h->tune_kc_cfg = -1; h->tune_bits = 0; h->tune_pair_gen = 1; h->ablate = 0;
    h->fp8_kind = 0; h->fp8_cal[0] = h->fp8_cal[1] = 0;
    if (init_kernel_attributes() != 0 || chain_init_attributes() != 0) { if (h->own_ws) hipFree(h->ws); delete h; return fail(-10, "hipFuncSetAttribute failed"); }
#define CREATE_CHK(x)                                           \
    do {                                                        \
        if ((x) != hipSuccess) {                                \
            fail(-10, "%s failed during create", #x);           \
            if (h->own_ws) hipFree(h->ws);                      \
            delete h;                                           \
            return -10;                                         \
        }                                                       \
    } while (0)
    // zero everything: padding of weights/activations must be exactly zero and stays so
    CREATE_CHK(hipMemsetAsync(h->ws, 0, h->ws_bytes, s));
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, s, h->state, 0u, 0u, cfg->lr, cfg->beta1, cfg->beta2);
    r = upload_tiles(h, h->gt, h->tiles_g_dev, h->ntiles_g, s);
    if (!r) r = upload_tiles(h, h->dt, h->tiles_d_dev, h->ntiles_d, s);
    if (r) { if (h->own_ws) hipFree(h->ws); delete h; return r; }
    if (h->fp8) {
        float tg[FP8_NSLOT];
        for (int k = 0; k < 2; ++k)
            for (int l = 0; l < 5; ++l) { tg[slot_x(k, l)] = FP8_TARGET_E4M3; tg[slot_g(k, l)] = FP8_TARGET_E5M2; }
        for (int l = 0; l < 5; ++l) tg[slot_w(l)] = FP8_TARGET_E4M3;
        tg[SLOT_GX] = FP8_TARGET_E4M3; tg[SLOT_GG] = FP8_TARGET_E5M2; tg[SLOT_GW] = FP8_TARGET_E4M3;
        CREATE_CHK(hipMemcpyAsync(h->slot_targets, tg, sizeof tg, hipMemcpyHostToDevice, s));
        CREATE_CHK(hipStreamSynchronize(s));
        if (launch_fp8_init_slots(h->slots, FP8_NSLOT, h->slot_targets, s) != 0) { if (h->own_ws) hipFree(h->ws); delete h; return fail(-10, "fp8 slot init failed"); }
    }
    // BN gamma defaults to one (Keras); dense weights stay zero until mrgan_set_weights
    std::vector<float> ones(h->gt[2].cols, 1.0f);
    CREATE_CHK(hipMemcpyAsync(h->gt[2].p, ones.data(), sizeof(float) * ones.size(), hipMemcpyHostToDevice, s));
    CREATE_CHK(hipStreamSynchronize(s));
    *out = h;
    return 0;
}

int mrgan_destroy(mrgan_handle* h) {
    if (!h) return 0;
    if (h->graph_exec) hipGraphExecDestroy(h->graph_exec);
    if (h->own_ws && h->ws) hipFree(h->ws);
    delete h;
    return 0;
}

int mrgan_num_tensors(const mrgan_handle* h, int net, int* n) {
    if (!h || !n) return fail(-1, "null argument");
    *n = net == MRGAN_NET_G ? 8 : 12;
    return 0;
}

int mrgan_tensor_shape(const mrgan_handle* h, int net, int idx, int* rows, int* cols) {
    Tensor* t = find_tensor((mrgan_handle*)h, net, idx);
    if (!t) return fail(-1, "no such tensor (%d,%d)", net, idx);
    *rows = t->rows; *cols = t->cols;
    return 0;
}

int mrgan_set_weights(mrgan_handle* h, int net, int idx, const float* src, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !src) return fail(-1, "set_weights: bad tensor or null source");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpy2DAsync(t->p, sizeof(float) * t->pcol, src, sizeof(float) * t->cols, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, s));
    if (t->w16) hipLaunchKernelGGL(refresh_bf16_kernel, grid2d(t->prow, t->pcol), dim3(256), 0, s, t->p, t->w16, t->wt16, t->prow, t->pcol);
    if (h->fp8 && t->w16 && (net == MRGAN_NET_D || t == h->g[1].W)) {
        // fp8 copies of the discriminator's weights: the first pass only measures max |w|, the second stores with that scale
        for (int pass = 0; pass < 2; ++pass) { CHK(fp8_refresh_weights(h, net, s)); CHK(fp8_update_scales(h, s)); }
    }
    return 0;
}

int mrgan_get_weights(mrgan_handle* h, int net, int idx, float* dst, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !dst) return fail(-1, "get_weights: bad tensor or null destination");
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * t->cols, t->p, sizeof(float) * t->pcol, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mrgan_get_slot(mrgan_handle* h, int net, int idx, int which, float* dst, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !dst || which < 0 || which > 2) return fail(-1, "get_slot: bad argument");
    if (which == 2 && t->flat16) return fail(-3, "get_slot: the flat gradients of this handle are bfloat16 (MRGAN_REGION_GRAD_*_BF16)");
    const float* src = which == 0 ? t->m : which == 1 ? t->v : t->flat;
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * t->cols, src, sizeof(float) * t->pcol, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mrgan_set_slot(mrgan_handle* h, int net, int idx, int which, const float* src, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !src || which < 0 || which > 1) return fail(-1, "set_slot: bad argument");
    float* dst = which == 0 ? t->m : t->v;
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * t->pcol, src, sizeof(float) * t->cols, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mrgan_get_iterations(mrgan_handle* h, mrgan_stream stream, uint32_t* it) {
    if (!h || !it) return fail(-1, "null argument");
    DevState st;
    HIPCHK(hipMemcpyAsync(&st, h->state + h->cur, sizeof st, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    *it = st.iter;
    return 0;
}

int mrgan_set_iterations(mrgan_handle* h, uint32_t iterations, uint32_t batch_counter, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->state, iterations, batch_counter,
                       h->cfg.lr, h->cfg.beta1, h->cfg.beta2);
    return 0;
}

int mrgan_disc_step(mrgan_handle* h, const mrgan_disc_args* a, int p0, int p1, float* out3, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = check_disc_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    if (p1 < 0) p1 = MRGAN_D_NPHASES - 1;
    if (h->fp8 && p0 == 0 && !h->fp8_cal[0] && p1 < MRGAN_D_NPHASES - 1 && h->sync_stats)
        return fail(-3, "fp8 with synchronised statistics: a phase-wise host runs the calibration passes itself (mrgan_fp8_calibration)");
    if (h->fp8 && p0 == 0 && !h->fp8_cal[0]) {
        // first D sub-step of an fp8 handle: calibrate with dry passes
        CHK(fp8_cal_begin(h, 0, s));
        for (int i = 0; i < FP8_DRY_PASSES; ++i) {
            for (int p = MRGAN_D_GEN; p <= MRGAN_D_MAIN; ++p) { r = disc_phase(h, a, p, s); if (r) return r; }
            CHK(fp8_cal_end_pass(h, 0, s));
        }
        CHK(fp8_cal_done(h, 0, s));
    }
    for (int p = p0; p <= p1; ++p) { r = disc_phase(h, a, p, s); if (r) return r; }
    if (out3) {
        HIPCHK(hipMemcpyAsync(out3, h->step_out, 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}

int mrgan_gen_step(mrgan_handle* h, const mrgan_gen_args* a, int p0, int p1, float* out1, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = check_gen_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    if (p1 < 0) p1 = MRGAN_G_NPHASES - 1;
    if (h->fp8 && p0 == 0 && !h->fp8_cal[1] && p1 < MRGAN_G_NPHASES - 1 && h->sync_stats)
        return fail(-3, "fp8 with synchronised statistics: a phase-wise host runs the calibration passes itself (mrgan_fp8_calibration)");
    if (h->fp8 && p0 == 0 && !h->fp8_cal[1]) {
        // same for the G sub-step's tensors (its own slots: the feature-matching gradient has another scale than the D loss's)
        CHK(fp8_cal_begin(h, 1, s));
        for (int i = 0; i < FP8_DRY_PASSES; ++i) {
            for (int p = MRGAN_G_GEN; p <= MRGAN_G_BWD; ++p) { r = gen_phase(h, a, p, s); if (r) return r; }
            CHK(fp8_cal_end_pass(h, 1, s));
        }
        CHK(fp8_cal_done(h, 1, s));
    }
    for (int p = p0; p <= p1; ++p) { r = gen_phase(h, a, p, s); if (r) return r; }
    if (out1) {
        HIPCHK(hipMemcpyAsync(out1, h->step_out + 3, sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}

int mrgan_fp8_calibration(mrgan_handle* h, int kind, int action, mrgan_stream stream) {
    if (!h || kind < 0 || kind > 1) return fail(-1, "fp8_calibration: bad handle or kind");
    hipStream_t s = (hipStream_t)stream;
    if (action == MRGAN_FP8_CAL_QUERY) return (!h->fp8 || h->fp8_cal[kind] == 1) ? 1 : 0;
    if (!h->fp8) return 0;
    switch (action) {
        case MRGAN_FP8_CAL_BEGIN: return fp8_cal_begin(h, kind, s);
        case MRGAN_FP8_CAL_END_PASS: return fp8_cal_end_pass(h, kind, s);
        case MRGAN_FP8_CAL_DONE: return fp8_cal_done(h, kind, s);
        default: return fail(-1, "fp8_calibration: unknown action %d", action);
    }
}

int32_t mrgan_logmel_frames(int64_t n_samples) { return n_samples > 0 ? logmel_frames((long)n_samples) : 0; }

int mrgan_logmel(const float* y_dev, int64_t n_trials, int64_t n_samples, int64_t ld_y, int32_t sr, int32_t n_mels, float* out_dev,
                 int64_t ld_out, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_logmel(y_dev, (long)n_trials, (long)n_samples, (long)ld_y, sr, n_mels, out_dev, (long)ld_out,
                                (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_sup_step(mrgan_handle* h, const mrgan_sup_args* a, float* out2, mrgan_stream stream) {
    if (!h || !a || !a->x_dev || !a->labels_dev) return fail(-1, "sup_step: x and labels are required");
    if (a->ld_x < h->cfg.d_in) return fail(-2, "sup_step: row pitch smaller than d_in");
    if (h->flat_grads || h->cfg.world != 1) return fail(-3, "sup_step: single-GPU handles only");
    if (h->fp8) return fail(-3, "sup_step: the fp8 mode covers the GAN step only");
    if (a->rows_valid < 0 || a->rows_valid > h->B) return fail(-2, "sup_step: rows_valid outside [0, batch]");
    if (a->rows_valid && a->stream_mode) return fail(-2, "sup_step: a short batch cannot be combined with stream mode");
    hipStream_t s = (hipStream_t)stream;
    int r = sup_step(h, a, s);
    if (r) return r;
    if (out2) {
        float o[3];
        HIPCHK(hipMemcpyAsync(o, h->step_out, 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const float k = a->rows_valid > 0 ? (float)h->B / (float)a->rows_valid : 1.f;     // the metrics pass divides by the batch
        out2[0] = o[0] * k; out2[1] = o[2] * k;
    }
    return 0;
}

int mrgan_train_pair(mrgan_handle* h, const mrgan_disc_args* d, const mrgan_gen_args* g, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = check_disc_args(h, d);
    if (!r) r = check_gen_args(h, g);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    const bool want_graph = !h->prof && (h->cfg.flags & MRGAN_FLAG_GRAPH) && d->stream_mode && g->stream_mode && !h->flat_grads && !h->sync_stats;
    // Both sub-steps of a pair use the same generator weights (the D sub-step does not touch them), so their two
    // generator forwards run as one two-segment pass inside the D sub-step when the G sub-step draws its z on the
    // device and no statistic exchange sits between the generator's layers.
    const int pair_env = h->tune_pair_gen;
    auto both = [&]() {
        h->pair_gen = (pair_env && !h->sync_stats && !g->z_dev) ? 1 : 0;
        h->pair_g = h->pair_gen ? g : nullptr;
        int rr = mrgan_disc_step(h, d, 0, -1, nullptr, stream);
        h->pair_gen = 0; h->pair_g = nullptr;
        if (!rr) rr = mrgan_gen_step(h, g, 0, -1, nullptr, stream);
        h->gen_ready = 0;
        return rr;
    };
    if (!want_graph || (h->fp8 && !(h->fp8_cal[0] == 1 && h->fp8_cal[1] == 1))) return both();     // (the calibrating first pair runs eagerly)
    // A pair flips the state slot twice, so every kernel argument is identical on every replay as long as
    // the slot parity and the caller's pointers are those of the capture.
    if (h->graph_ready && (h->graph_cur != h->cur || memcmp(&h->graph_d, d, sizeof *d) != 0 || memcmp(&h->graph_g, g, sizeof *g) != 0)) {
        hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr; h->graph_ready = false;
    }
    if (!h->graph_ready) {
        hipGraph_t graph;
        const int cur0 = h->cur;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        r = both();
        graph = nullptr;
        hipError_t e = hipStreamEndCapture(s, &graph);
        if (r) { if (graph) hipGraphDestroy(graph); return r; }       // a launch failed during capture: drop the partial graph
        if (e != hipSuccess) return fail(-10, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (e != hipSuccess) return fail(-10, "hipGraphInstantiate: %s", hipGetErrorString(e));
        h->graph_d = *d; h->graph_g = *g; h->graph_cur = cur0; h->graph_ready = true;
    }
    HIPCHK(hipGraphLaunch(h->graph_exec, s));
    return 0;
}

int mrgan_set_tuning(mrgan_handle* h, int knob, int value) {
    if (!h) return fail(-1, "null handle");
    if (h->graph_exec) { hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; h->graph_ready = false; }   // launches change
    switch (knob) {
        case MRGAN_TUNE_CHAIN: h->use_chain = value != 0 && h->chain_ok; break;
        case MRGAN_TUNE_KC_CFG:
            if (!kc_cfg_supported(value)) return fail(-1, "unsupported forward / dX tile config %d", value);
            h->tune_kc_cfg = value; break;
        case MRGAN_TUNE_KS_GROUP: h->tune_bits = (h->tune_bits & ~TUNE_BIT_NO_KS_GROUP) | (value ? 0 : TUNE_BIT_NO_KS_GROUP); break;
        case MRGAN_TUNE_PAIR_GEN: h->tune_pair_gen = value ? 1 : 0; break;
        case MRGAN_TUNE_HEAD_MFMA: h->head_wide = value != 0 && h->head_wide_ok; break;
        default: return fail(-1, "unknown tuning knob %d", knob);
    }
    return 0;
}

int mrgan_pair_hint(mrgan_handle* h, int on) {
    if (!h) return fail(-1, "null handle");
    h->pair_gen = on ? 1 : 0;
    return 0;
}

int mrgan_region(mrgan_handle* h, int region, void** ptr, size_t* bytes) {
    if (!h || !ptr || !bytes) return fail(-1, "null argument");
    const size_t n1 = (size_t)h->g[0].Np;
    switch (region) {
        case MRGAN_REGION_BN_STATS: *ptr = h->r_bn_stats; *bytes = 4 * n1 * 4; break;
        case MRGAN_REGION_FM_MOMENTS: *ptr = h->r_fm; *bytes = 2 * (size_t)h->Fp * 4; break;
        case MRGAN_REGION_BN_BWD: *ptr = h->r_bn_bwd; *bytes = 2 * n1 * 4; break;
        case MRGAN_REGION_GRAD_D: case MRGAN_REGION_GRAD_G: {
            // the reduce / Adam phases of a bfloat16-payload handle never touch the fp32 bodies: exchanging them would leave
            // the replicas' gradients unreduced
            if (h->flat16_d) return fail(-3, "region %d: the gradients of this handle travel as bfloat16 (MRGAN_FLAG_GRAD_BF16): "
                                             "all-reduce MRGAN_REGION_GRAD_*_BF16 and MRGAN_REGION_TAIL_*", region);
            const bool d = region == MRGAN_REGION_GRAD_D;
            *ptr = d ? h->flat_d : h->flat_g; *bytes = ((d ? h->flat_d_n : h->flat_g_n) + 4) * 4;
            break;
        }
        case MRGAN_REGION_WORKSPACE: *ptr = h->ws; *bytes = h->ws_bytes; break;
        case MRGAN_REGION_GRAD_D_BF16: case MRGAN_REGION_GRAD_G_BF16: {
            if (!h->flat16_d) return fail(-3, "the bfloat16 gradient regions exist with MRGAN_FLAG_GRAD_BF16 only");
            const bool d = region == MRGAN_REGION_GRAD_D_BF16;
            *ptr = d ? h->flat16_d : h->flat16_g; *bytes = (d ? h->flat_d_n : h->flat_g_n) * 2;
            break;
        }
        case MRGAN_REGION_TAIL_D: *ptr = h->flat_d + h->flat_d_n; *bytes = 16; break;
        case MRGAN_REGION_TAIL_G: *ptr = h->flat_g + h->flat_g_n; *bytes = 16; break;
        default: return fail(-1, "unknown region %d", region);
    }
    return 0;
}

int mrgan_eval_error(mrgan_handle* h, const float* x, const int32_t* idx, int64_t ld, const int32_t* labels, int64_t n,
                     float* err_host, mrgan_stream stream) {
    if (!h || !x || !labels || !err_host || n < 1) return fail(-1, "eval_error: bad argument");
    if (ld < h->cfg.d_in) return fail(-2, "eval_error: row pitch smaller than d_in");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(h->err_count, 0, sizeof(int), s));
    int r = eval_rows(h, x, idx, ld, labels, n, nullptr, s);
    if (r) return r;
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, h->err_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *err_host = (float)((double)cnt / (double)n);
    return 0;
}

int mrgan_predict_logits(mrgan_handle* h, const float* x, const int32_t* idx, int64_t ld, int64_t n, float* logits,
                         mrgan_stream stream) {
    if (!h || !x || !logits || n < 1) return fail(-1, "predict_logits: bad argument");
    if (ld < h->cfg.d_in) return fail(-2, "predict_logits: row pitch smaller than d_in");
    return eval_rows(h, x, idx, ld, nullptr, n, logits, (hipStream_t)stream);
}

int mrgan_read_metrics(mrgan_handle* h, float* out8, int reset, mrgan_stream stream) {
    if (!h || !out8) return fail(-1, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out8, h->accum, 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out8 + 4, h->step_out, 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(h->accum, 0, 4 * sizeof(float), s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int mrgan_profile_begin(mrgan_handle* h) {
    if (!h) return fail(-1, "null handle");
    h->prof = true;
    return 0;
}

int mrgan_profile_end(mrgan_handle* h, mrgan_stream stream, int max_kernels, char* names, float* ms, int32_t* launches,
                      double* flops, double* bytes, int* n_kernels) {
    if (!h || !names || !ms || !launches || !flops || !bytes || !n_kernels) return fail(-1, "null argument");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const int n = std::min(max_kernels, (int)h->prof_names.size());
    for (int i = 0; i < n; ++i) {
        ms[i] = 0.f; launches[i] = 0; flops[i] = 0.0; bytes[i] = 0.0;
        snprintf(names + (size_t)i * MRGAN_PROF_NAME_LEN, MRGAN_PROF_NAME_LEN, "%s", h->prof_names[i].c_str());
    }
    for (const ProfRec& r : h->prof_recs) {
        float t = 0.f;
        if (r.cat < n && hipEventElapsedTime(&t, r.start, r.stop) == hipSuccess) { ms[r.cat] += t; launches[r.cat] += 1; flops[r.cat] += r.flops; bytes[r.cat] += r.bytes; }
    }
    for (auto& r : h->prof_recs) { hipEventDestroy(r.start); hipEventDestroy(r.stop); }
    h->prof_recs.clear(); h->prof_names.clear();
    h->prof = false;
    *n_kernels = n;
    return 0;
}

int mrgan_debug_noise(mrgan_handle* h, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0, int rows, int cols, float* out,
                      mrgan_stream stream) {
    if (!h || !out) return fail(-1, "null argument");
    CHK(launch_noise_debug(h->cfg.seed, site, seg, step, row0, rows, cols, out, (hipStream_t)stream));
    return 0;
}

int mrgan_debug_ablate(mrgan_handle* h, int bits) {
    if (!h) return fail(-1, "null handle");
    if (h->graph_exec) { hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; h->graph_ready = false; }
    h->ablate = bits;
    return 0;
}

// activation buffers of the discriminator for activation-level tests: kind 0 = xin[l] (noisy layer input), 1 = dpre[l]
// (gradient w.r.t. the layer's pre-activation), 2 = features.  Elements are fp32 or bf16 (the handle's dtype), laid out
// [segment][S rows][ld].
int mrgan_debug_buffer(mrgan_handle* h, int kind, int l, void** ptr, int* rows_per_seg, int* ld, int* elem_size) {
    if (!h || !ptr || l < 0 || l > 4) return fail(-1, "debug_buffer: bad argument");
    switch (kind) {
        case 0: *ptr = h->xin[l]; *ld = h->d[l].Kp; break;
        case 1: *ptr = h->dpre[l]; *ld = h->d[l].Np; break;
        case 2: *ptr = h->feat; *ld = h->Fp; break;
        default: return fail(-1, "debug_buffer: unknown kind");
    }
    *rows_per_seg = h->S; *elem_size = h->es;
    return 0;
}

// Kernel-level timing of one bf16 product on scratch buffers (contents irrelevant): op 0 forward (relu + noise +
// mask), 1 input-gradient (relu mask), 2 weight-gradient.  Returns the average device time of `reps` back-to-back
// launches in microseconds (hipEvent pair around the whole run, so launch gaps are included).
int mrgan_debug_gemm_time(int op, int m, int n, int k, int nbatch, int splits, int reps, int ablate, int kc_cfg, float* avg_us) {
    if ((n % 64) || (k % 64) || !avg_us) return fail(-1, "debug_gemm_time: bad argument");
    const size_t rows = (size_t)m * nbatch;
    const bool is_dx = op == 1 || op >= 5;
    const int a_cols = is_dx ? n : k, o_cols = is_dx ? k : n;
    if (op < 0 || op > 8) return fail(-1, "debug_gemm_time: bad op");
    if (!kc_cfg_supported(kc_cfg)) return fail(-1, "debug_gemm_time: unsupported forward / dX tile config %d", kc_cfg);
    __bf16 *ta = nullptr, *tb = nullptr, *to = nullptr;
    uint16_t* mask = nullptr; float* slabs = nullptr; float* bias = nullptr; DevState* st = nullptr;
    HIPCHK(hipMalloc((void**)&ta, rows * std::max(a_cols, n) * 2));
    HIPCHK(hipMalloc((void**)&tb, (size_t)std::max((size_t)k, rows) * n * 2));
    HIPCHK(hipMalloc((void**)&to, rows * std::max(o_cols, n) * 2));
    HIPCHK(hipMalloc((void**)&mask, (rows / 32 + 4) * std::max(n, k) * 4));
    HIPCHK(hipMalloc((void**)&bias, (size_t)std::max(n, k) * 4));
    HIPCHK(hipMalloc((void**)&st, sizeof(DevState) * 2));
    HIPCHK(hipMemset(ta, 0x3c, rows * std::max(a_cols, n) * 2));      // bf16 ~0.0115 everywhere: finite, non-trivial bits
    HIPCHK(hipMemset(tb, 0x3c, (size_t)std::max((size_t)k, rows) * n * 2));
    HIPCHK(hipMemset(mask, 0x55, (rows / 32 + 4) * std::max(n, k) * 4));
    HIPCHK(hipMemset(bias, 0, (size_t)std::max(n, k) * 4));
    HIPCHK(hipMemset(st, 0, sizeof(DevState) * 2));
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.nbatch = nbatch; g.splits = 1; g.A = ta; g.B = tb;
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.e.st = st; g.e.out = to; g.e.ablate = ablate; g.e.tune_kc_cfg = kc_cfg; g.e.seed = 1;
    int epi;
    if (op == 0 || op == 3 || op == 4) {       // 0: relu + noise + mask ; 3: relu + mask ; 4: plain relu
        epi = EPI_FWD; g.M = m; g.N = n; g.K = k; g.kchunk = k; g.a_bs = (long)m * k; g.a_si = k; g.a_sk = 1; g.b_sj = k; g.b_sk = 1;
        g.e.act = ACT_RELU; g.e.n_valid = n; g.e.bias = bias; g.e.ldo = n; g.e.out_bs = (long)m * n;
        g.e.sigma = op == 0 ? 0.5f : 0.f; g.e.site = 1;
        if (op != 4) { g.e.mask = mask; g.e.ldm = n; g.e.mask_bs = (long)(m / 32 + 1) * n * 2; }
    } else if (is_dx) {
        // 1: relu mask ; 5: softplus' with e.h + column sums ; 6: linear + xhat sums ; 7: linear + column sums ; 8: linear
        epi = EPI_DX; g.M = m; g.N = k; g.K = n; g.kchunk = n; g.a_bs = (long)m * n; g.a_si = n; g.a_sk = 1; g.b_sk = 1; g.b_sj = n;
        g.e.act = op == 1 ? ACT_RELU : op == 5 ? ACT_SOFTPLUS : ACT_LINEAR; g.e.n_valid = k; g.e.ldo = k; g.e.out_bs = (long)m * k;
        if (op == 1) { g.e.mask = mask; g.e.ldm = k; g.e.mask_bs = (long)(m / 32 + 1) * k * 2; }
        if (op == 5 || op == 6) { g.e.h = ta; g.e.ldh = k; g.e.h_bs = (long)m * k; }
        if (op >= 5 && op <= 7) {
            HIPCHK(hipMalloc((void**)&slabs, (size_t)2 * (rows / 64 + 1) * k * 4));
            g.e.cs_mode = op == 6 ? CS_SUM_XHAT : CS_SUM; g.e.cs1 = slabs; g.e.cs2 = slabs + (size_t)(rows / 64 + 1) * k; g.e.ldcs = k;
            g.e.bn_mu = bias; g.e.bn_rstd = bias;
        }
    } else {
        epi = EPI_SLAB; g.M = k; g.N = n; g.K = m * nbatch; g.nbatch = 1; g.splits = std::max(1, splits);
        g.kchunk = (int)round_up(ceil_div(g.K, g.splits), 64);
        g.a_si = 1; g.a_sk = k; g.b_sk = n; g.b_sj = 1;
        HIPCHK(hipMalloc((void**)&slabs, (size_t)g.splits * k * n * 4));
        g.e.slab = slabs; g.e.slab_stride = (long)k * n; g.e.ldo = n;
    }
    g.tiles_m = ceil_div(g.M, 64);
#ifdef MRGAN_STAMPS
    unsigned long long* stamps = nullptr;
    if (op != 2) {
        HIPCHK(hipMalloc((void**)&stamps, 4096 * 12 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(stamps, 0, 4096 * 12 * sizeof(unsigned long long)));
        g.e.slab = (float*)stamps;
    }
#endif
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    int r = 0;
    for (int i = 0; i < 3 && !r; ++i) r = launch_gemm_bf16(epi, g, 0);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(e0, 0));
    for (int i = 0; i < reps && !r; ++i) r = launch_gemm_bf16(epi, g, 0);
    HIPCHK(hipEventRecord(e1, 0));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = 1e3f * ms / (float)reps;
#ifdef MRGAN_STAMPS
    if (stamps) {
        std::vector<unsigned long long> hs(4096 * 12);
        hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        double tot[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; int nb = 0;
        for (int b = 0; b < 4096; ++b) if (hs[b * 12 + 2]) { ++nb; for (int i = 0; i < 10; ++i) tot[i] += (double)hs[b * 12 + i]; }
        if (nb) fprintf(stderr, "  stamps (kcycles per block, %d blocks): setup %.1f | fill %.1f | mainloop %.1f | barrier %.1f | epilogue %.1f (math+staging %.1f, barrier %.1f, copy-out %.1f, column sums %.1f) | tail-barrier %.1f\n",
                        nb, tot[0] / nb / 1e3, tot[1] / nb / 1e3, tot[2] / nb / 1e3, tot[3] / nb / 1e3, tot[4] / nb / 1e3, tot[6] / nb / 1e3, tot[7] / nb / 1e3, tot[8] / nb / 1e3,
                        tot[9] / nb / 1e3, tot[5] / nb / 1e3);
        hipFree(stamps);
    }
#endif
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(ta); hipFree(tb); hipFree(to); hipFree(mask); hipFree(bias); hipFree(st);
    if (slabs) hipFree(slabs);
    if (r) return fail(r, "debug_gemm_time: launch failed (%d)", r);
    return 0;
}

// fp8 forward product (gemm_fp8.hip): out[m,n] = act((q(a * scale_a) q(b * scale_b)) / (scale_a scale_b) + bias), q = e4m3 RNE.
// reps > 0: returns the average device time of `reps` launches in *avg_us instead of writing `out` through fp32.
int mrgan_debug_gemm_fp8(int m, int n, int k, const float* a, const float* b, const float* bias, int act, float scale_a, float scale_b,
                         float* out, int reps, float* avg_us, int kc_cfg, mrgan_stream stream) {
    if ((n % 64) || (k % 128) || !a || !b) return fail(-1, "debug_gemm_fp8: n %% 64 == 0 and k %% 128 == 0 are required");
    hipStream_t s = (hipStream_t)stream;
    unsigned char *ta = nullptr, *tb = nullptr;
    __bf16* to = nullptr;
    HIPCHK(hipMalloc((void**)&ta, (size_t)m * k));
    HIPCHK(hipMalloc((void**)&tb, (size_t)n * k));
    HIPCHK(hipMalloc((void**)&to, (size_t)m * n * 2));
    CHK(launch_to_fp8(a, k, ta, k, m, k, m, k, scale_a, 0, s));
    CHK(launch_to_fp8(b, n, tb, k, k, n, k, n, scale_b, 1, s));          // Bt[n][k] = b[k][n]
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = m; g.N = n; g.K = k; g.nbatch = 1; g.splits = 1; g.kchunk = k; g.tiles_m = ceil_div(m, 64);
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.A = ta; g.a_si = k; g.a_sk = 1; g.B = tb; g.b_sj = k; g.b_sk = 1;
    g.e.act = act; g.e.n_valid = n; g.e.bias = bias; g.e.out = to; g.e.ldo = n; g.e.acc_scale = 1.0f / (scale_a * scale_b);
    g.e.tune_kc_cfg = kc_cfg;
#ifdef MRGAN_STAMPS
    unsigned long long* stamps = nullptr;
    HIPCHK(hipMalloc((void**)&stamps, 4096 * 4 * sizeof(unsigned long long)));
    g.e.cs2 = (float*)stamps;
#endif
    int r = launch_gemm_fp8(EPI_FWD, g, s);
#ifdef MRGAN_STAMPS
    HIPCHK(hipMemsetAsync(stamps, 0, 4096 * 4 * sizeof(unsigned long long), s));
#endif
    if (!r && reps > 0 && avg_us) {
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipEventRecord(e0, s));
        for (int i = 0; i < reps && !r; ++i) r = launch_gemm_fp8(EPI_FWD, g, s);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = 1e3f * ms / (float)reps;
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    if (!r && out) hipLaunchKernelGGL(to_f32_kernel<__bf16>, grid2d(m, n), dim3(256), 0, s, (const __bf16*)to, (long)n, out, (long)n, m, n);
    hipStreamSynchronize(s);
#ifdef MRGAN_STAMPS
    {
        std::vector<unsigned long long> hs(4096 * 4);
        hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        double cyc = 0, wait = 0, rt = 0, tiles = 0; int nb = 0;
        for (int b = 0; b < 4096; ++b) if (hs[b * 4 + 3]) { cyc += hs[b * 4]; wait += hs[b * 4 + 1]; rt += hs[b * 4 + 2]; tiles += hs[b * 4 + 3]; ++nb; }
        if (nb) fprintf(stderr, "[stamps] fp8 %dx%dx%d: blocks %d, tiles/block %.1f, k-loop cycles/tile %.0f (wait+barrier %.0f = %.1f %%), per k-tile %.0f, clock %.3f GHz\n",
                        m, n, k, nb, tiles / nb, cyc / tiles, wait / tiles, 100.0 * wait / cyc, cyc / tiles / (k / 128), cyc / rt * 0.1);
        hipFree(stamps);
    }
#endif
    hipFree(ta); hipFree(tb); hipFree(to);
    if (r) return fail(r, "debug_gemm_fp8: launch failed (%d)", r);
    return 0;
}

int mrgan_debug_tr_probe(uint16_t* out, mrgan_stream stream) {
    if (!out) return fail(-1, "null argument");
    CHK(launch_tr_probe(out, (hipStream_t)stream));
    return 0;
}

int mrgan_debug_gemm(int dtype, int op, int m, int n, int k, const float* a, const float* b, const float* bias, int act,
                     int splits, float* out, mrgan_stream stream) {
    // op 0: out[m,n] = act(a[m,k] b[k,n] + bias) ; op 1: out[m,k] = a[m,n] b[k,n]^T ; op 2: out[k,n] = a[m,k]^T b[m,n]
    if ((n % 64) || (k % 64)) return fail(-1, "debug_gemm: n and k must be multiples of 64");
    hipStream_t s = (hipStream_t)stream;
    const bool bf = dtype == MRGAN_BF16;
    const size_t es = bf ? 2 : 4;
    const int a_cols = op == 1 ? n : k, b_rows = op == 2 ? m : k;
    const int o_rows = op == 2 ? k : m, o_cols = op == 1 ? k : n;
    void *ta = nullptr, *tb = nullptr, *to = nullptr;
    float* slabs = nullptr;
    DevState* st = nullptr;
    HIPCHK(hipMalloc(&ta, (size_t)m * a_cols * es));
    HIPCHK(hipMalloc(&tb, (size_t)b_rows * n * es));
    HIPCHK(hipMalloc(&to, (size_t)o_rows * o_cols * es));
    HIPCHK(hipMalloc((void**)&st, sizeof(DevState) * 2));
    HIPCHK(hipMemsetAsync(st, 0, sizeof(DevState) * 2, s));
    const bool tr_b = bf && op == 0;       // the bf16 forward reads the transposed weight copy
    if (bf) {
        hipLaunchKernelGGL(convert_kernel<__bf16>, grid2d(m, a_cols), dim3(256), 0, s, a, (long)a_cols, (__bf16*)ta, (long)a_cols, m, a_cols, m, a_cols, 0);
        hipLaunchKernelGGL(convert_kernel<__bf16>, grid2d(b_rows, n), dim3(256), 0, s, b, (long)n, (__bf16*)tb, (long)(tr_b ? b_rows : n), b_rows, n, b_rows, n, tr_b ? 1 : 0);
    } else {
        HIPCHK(hipMemcpyAsync(ta, a, (size_t)m * a_cols * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(tb, b, (size_t)b_rows * n * 4, hipMemcpyDeviceToDevice, s));
    }
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.nbatch = 1; g.splits = 1; g.A = ta; g.B = tb;
    g.seg_stride = 1 << 30; g.seg_rows = 1 << 30;
    g.e.st = st; g.e.out = to; g.e.tune_kc_cfg = -1;
    int epi;
    if (op == 0) {
        epi = EPI_FWD; g.M = m; g.N = n; g.K = k; g.kchunk = k; g.a_si = k; g.a_sk = 1;
        if (bf) { g.b_sj = k; g.b_sk = 1; } else { g.b_sk = n; g.b_sj = 1; }
        g.e.act = act; g.e.n_valid = n; g.e.bias = bias; g.e.ldo = n;
    } else if (op == 1) {
        epi = EPI_DX; g.M = m; g.N = k; g.K = n; g.kchunk = n; g.a_si = n; g.a_sk = 1; g.b_sk = 1; g.b_sj = n;
        g.e.act = ACT_LINEAR; g.e.n_valid = k; g.e.ldo = k;
    } else {
        epi = EPI_SLAB; g.M = k; g.N = n; g.K = m; g.splits = std::max(1, splits);
        g.kchunk = (int)round_up(ceil_div(m, g.splits), 64);
        g.a_si = 1; g.a_sk = k; g.b_sk = n; g.b_sj = 1;
        HIPCHK(hipMalloc((void**)&slabs, (size_t)g.splits * k * n * 4));
        g.e.slab = slabs; g.e.slab_stride = (long)k * n; g.e.ldo = n;
    }
    g.tiles_m = ceil_div(g.M, 64);
    int r = bf ? launch_gemm_bf16(epi, g, s) : launch_gemm_f32(epi, g, s);
    if (!r) {
        if (op == 2) hipLaunchKernelGGL(sum_slabs_kernel, dim3(ceil_div((long)k * n, 256)), dim3(256), 0, s, slabs, g.splits, (long)k * n, (long)k * n, out);
        else if (bf) hipLaunchKernelGGL(to_f32_kernel<__bf16>, grid2d(o_rows, o_cols), dim3(256), 0, s, (const __bf16*)to, (long)o_cols, out, (long)o_cols, o_rows, o_cols);
        else hipMemcpyAsync(out, to, (size_t)o_rows * o_cols * 4, hipMemcpyDeviceToDevice, s);
    }
    hipStreamSynchronize(s);
    hipFree(ta); hipFree(tb); hipFree(to); hipFree(st);
    if (slabs) hipFree(slabs);
    if (r) return fail(r, "debug_gemm: launch failed (%d)", r);
    return 0;
}

// one descriptor -> the launchers' argument block; the checks are the preconditions the kernels state for themselves
static int debug_gemm_args(const mrgan_debug_gemm_desc& d, const DevState* st, GemmArgs& g, int& epi) {
    const bool bf = d.dtype == MRGAN_BF16;
    if (d.dtype != MRGAN_BF16 && d.dtype != MRGAN_F32) return fail(-1, "debug_gemm_launch: dtype must be fp32 or bf16");
    if (d.op < 0 || d.op > 2) return fail(-1, "debug_gemm_launch: op must be 0, 1 or 2");
    if (!kc_cfg_supported(d.kc_cfg)) return fail(-1, "debug_gemm_launch: kc_cfg %d is not a block tile", d.kc_cfg);
    if (d.m < 1 || d.n < 1 || d.k < 1 || d.nbatch < 1 || d.splits < 1 || !d.a || !d.b) return fail(-1, "debug_gemm_launch: empty problem");
    if (d.n % 64) return fail(-1, "debug_gemm_launch: n must be a multiple of 64");
    memset(&g, 0, sizeof g);
    epi = d.op == 0 ? EPI_FWD : d.op == 1 ? EPI_DX : EPI_SLAB;
    g.M = d.m; g.N = d.n; g.K = d.k; g.nbatch = d.nbatch; g.splits = d.splits;
    g.kchunk = d.kchunk > 0 ? d.kchunk : d.k;
    g.tiles_m = ceil_div(d.m, 64);
    g.seg_stride = d.seg_stride > 0 ? d.seg_stride : 1 << 30; g.seg_rows = d.seg_stride > 0 ? d.seg_rows : 1 << 30;
    g.A = d.a; g.a_bs = d.a_bs; g.a_si = d.a_si; g.a_sk = d.a_sk;
    g.B = d.b; g.b_bs = d.b_bs; g.b_sk = d.b_sk; g.b_sj = d.b_sj;
    Epi& e = g.e;
    e.act = d.act; e.n_valid = d.n_valid; e.bias = d.bias;
    e.out = d.out; e.out_bs = d.out_bs; e.ldo = d.ldo;
    e.sigma = d.sigma; e.site = d.site; e.seg0 = d.seg0; e.seg_step = d.seg_step; e.iter_step = d.iter_step; e.row0 = d.row0; e.seed = d.seed;
    e.mask = d.mask; e.mask_bs = d.mask_bs; e.ldm = d.ldm;
    e.h = d.h; e.h_bs = d.h_bs; e.ldh = d.ldh;
    e.cs_mode = d.cs_mode; e.cs1 = d.cs1; e.cs2 = d.cs2; e.ldcs = d.ldcs; e.bn_mu = d.bn_mu; e.bn_rstd = d.bn_rstd;
    e.slab = d.slab; e.slab_stride = d.slab_stride;
    e.st = st; e.acc_scale = 1.f; e.tune_kc_cfg = d.kc_cfg; e.tune_bits = d.tune_bits;
    if (epi == EPI_SLAB) {
        const int bk = bf ? 64 : 16;
        if (!d.slab || d.ldo < d.n) return fail(-1, "debug_gemm_launch: weight gradient needs slab and ldo >= n");
        if ((g.kchunk % bk) || (g.seg_stride % bk)) return fail(-1, "debug_gemm_launch: kchunk and seg_stride must be multiples of %d", bk);
        // 16-byte operand loads of the bf16 kernels: 8 elements per predicate
        if (bf && ((d.a_sk % 8) || (d.b_sk % 8) || d.a_sk < round_up(d.m, 8))) return fail(-1, "debug_gemm_launch: bf16 row pitches must be multiples of 8");
    } else {
        if (!d.out || d.ldo < d.n || d.n_valid < 0 || d.n_valid > d.n) return fail(-1, "debug_gemm_launch: needs out, ldo >= n and n_valid <= n");
        if (bf && ((d.ldo % 8) || (d.a_si % 8) || (d.b_sj % 8))) return fail(-1, "debug_gemm_launch: bf16 row pitches must be multiples of 8");
        if (d.cs_mode != CS_NONE && (!d.cs1 || d.ldcs < d.n || (d.cs_mode != CS_SUM && !d.cs2))) return fail(-1, "debug_gemm_launch: column sums need cs1 / cs2 and ldcs >= n");
        if (d.cs_mode == CS_SUM_XHAT && (epi != EPI_DX || !d.bn_mu || !d.bn_rstd || !d.h)) return fail(-1, "debug_gemm_launch: xhat sums need bn_mu, bn_rstd and h on a dX product");
        if (epi == EPI_DX && d.act == ACT_SOFTPLUS && !d.h) return fail(-1, "debug_gemm_launch: the softplus derivative needs h");
        if (epi == EPI_DX && d.act == ACT_RELU && !d.mask) return fail(-1, "debug_gemm_launch: the relu derivative needs mask");
        if (d.h && (d.ldh < d.n || (bf && (d.ldh % 8)))) return fail(-1, "debug_gemm_launch: ldh");
        if (d.mask && d.ldm < d.n) return fail(-1, "debug_gemm_launch: ldm >= n");
    }
    return 0;
}

int mrgan_debug_gemm_launch(const mrgan_debug_gemm_desc* d, int count, int grouped, const mrgan_debug_fold* fold,
                            char* kname, int kname_len, mrgan_stream stream) {
    if (!d || count < 1) return fail(-1, "null argument");
    if (kname && kname_len > 0) kname[0] = 0;
    hipStream_t s = (hipStream_t)stream;
    DevState* st = nullptr;
    DevState hst[2];
    memset(hst, 0, sizeof hst);
    hst[0].iter = hst[1].iter = d[0].iter;
    HIPCHK(hipMalloc((void**)&st, sizeof hst));
    hipError_t he = hipMemcpy(st, hst, sizeof hst, hipMemcpyHostToDevice);
    const char* name = "";
    int r = he == hipSuccess ? 0 : fail(-10, "hipMemcpy failed: %s", hipGetErrorString(he));
    if (!r && !grouped) {
        GemmArgs g;
        int epi = 0;
        if (count != 1) r = fail(-1, "debug_gemm_launch: one product per plain launch");
        if (!r) r = debug_gemm_args(d[0], st, g, epi);
        if (!r) {
            r = d[0].dtype == MRGAN_BF16 ? launch_gemm_bf16(epi, g, s, &name) : launch_gemm_f32(epi, g, s, &name);
            if (r) fail(r, "debug_gemm_launch: launch refused (%d)", r);
        }
    } else if (!r) {
        // (a count beyond KS_GROUP_MAX is the launcher's refusal to make: it looks at no descriptor then)
        GemmArgs gs[KS_GROUP_MAX];
        for (int i = 0; i < count && i < KS_GROUP_MAX && !r; ++i) {
            int epi = 0;
            r = debug_gemm_args(d[i], st, gs[i], epi);
            if (!r && (epi != EPI_SLAB || d[i].dtype != MRGAN_BF16)) r = fail(-1, "debug_gemm_launch: grouped launches are bf16 weight gradients");
        }
        FoldJob fj;
        memset(&fj, 0, sizeof fj);
        if (!r && fold) {
            if (!fold->src || !fold->dst || fold->nsrc < 1 || fold->n < 1 || fold->ngroups < 1 || fold->stride < fold->n)
                r = fail(-1, "debug_gemm_launch: fold");
            fj.src = fold->src; fj.dst = fold->dst; fj.stride = fold->stride; fj.nsrc = fold->nsrc; fj.n = fold->n; fj.ngroups = fold->ngroups;
        }
        if (!r) {
            r = launch_gemm_bf16_dw_group(gs, count, s, &name, fold ? &fj : nullptr);
            if (r < 0) fail(r, "debug_gemm_launch: grouped launch failed (%d)", r);
        }
    }
    he = hipStreamSynchronize(s);
    hipFree(st);
    if (!r && he != hipSuccess) return fail(-10, "debug_gemm_launch: %s", hipGetErrorString(he));
    if (!r && kname && kname_len > 0) snprintf(kname, (size_t)kname_len, "%s", name);
    return r;
}

}  // extern "C"
