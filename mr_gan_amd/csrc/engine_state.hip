// Engine state behind include/mrgan_abi.h: workspace layout in HBM, create / destroy, weights and Adam slots in and out,
// the regions a data-parallel host exchanges, tuning knobs.
#include <stdarg.h>

#include "engine_internal.h"

namespace mrgan {

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

void set_gen_view(mrgan_handle* h, int seg) {
    h->g[1].q.xseg = seg;
    const int N1p = h->g[0].Np;
    h->zbuf = rowptr(h, h->zbuf_all, (long)seg * h->S, h->nzp);
    h->h1 = rowptr(h, h->h1_all, (long)seg * h->S, N1p);
    h->hbn = rowptr(h, h->hbn_all, (long)seg * h->S, N1p);
    h->h2 = rowptr(h, h->h2_all, (long)seg * h->S, h->g[1].Np);
    h->bn_mu = h->bn_mu_all + (size_t)seg * N1p;
    h->bn_rstd = h->bn_rstd_all + (size_t)seg * N1p;
}

}  // namespace mrgan

namespace {

struct Arena {
    char* base = nullptr; size_t off = 0, cap = 0;
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};


__global__ void refresh_bf16_kernel(const float* p, __bf16* w16, __bf16* wt16, int prow, int pcol) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= prow || c >= pcol) return;
    const __bf16 v = (__bf16)p[(long)r * pcol + c];
    if (w16) w16[(long)r * pcol + c] = v;
    if (wt16) wt16[(long)c * prow + r] = v;
}
__global__ void init_state_kernel(DevState* st, uint32_t iter, uint32_t batch, float lr, float b1, float b2) {
    DevState s;
    s.iter = iter; s.batch = batch; s.pad = 0;
    const double t = (double)iter + 1.0;
    s.lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    st[0] = s; st[1] = s;
}
// the constant slots of mrgan_attribution: slot d carries the draw index as its noise step (engine_internal.h: draw_state)
__global__ void init_draw_state_kernel(DevState* st, int n) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    DevState s;
    s.iter = (uint32_t)d; s.batch = 0; s.lr_t = 0.f; s.pad = 0;
    st[d] = s;
}

// ------------------------------------------------------------------------------------------------
// layout
// ------------------------------------------------------------------------------------------------
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
    if (c.num_classes < 2 || c.num_classes > MRGAN_MAX_CLASSES) return fail(-1, "num_classes must be in [2,%d]", MRGAN_MAX_CLASSES);
    if (c.dtype != MRGAN_F32 && c.dtype != MRGAN_BF16 && c.dtype != MRGAN_FP8) return fail(-1, "unknown dtype");
    if (c.flags & MRGAN_FLAG_AUTOENCODER) {
        // an autoencoder trains through mrgan_ae_step: fp32 / bf16, one model, fused Adam, one device, no GaussianNoise
        if (c.dtype == MRGAN_FP8) return fail(-3, "an autoencoder handle cannot be an fp8 handle: its last layer has no fp8 images");
        if (c.models > 1) return fail(-3, "an autoencoder handle cannot be a model group (models = %d)", c.models);
        if (c.world != 1) return fail(-3, "an autoencoder handle needs world = 1: the data-parallel step is not built");
        if (c.flags & (MRGAN_FLAG_FLAT_GRADS | MRGAN_FLAG_SYNC_STATS | MRGAN_FLAG_GRAD_BF16))
            return fail(-3, "an autoencoder handle cannot have MRGAN_FLAG_FLAT_GRADS, MRGAN_FLAG_SYNC_STATS or MRGAN_FLAG_GRAD_BF16: the data-parallel step is not built");
        for (int i = 0; i < 5; ++i)
            if (c.sigma[i] != 0.f) return fail(-1, "an autoencoder handle needs sigma[%d] = 0 (got %g): the denoising variant is not built", i, (double)c.sigma[i]);
    }
    if (c.dtype == MRGAN_FP8 && c.num_classes > KMAX)
        return fail(-1, "the fp8 engine supports at most %d classes (num_classes = %d): its loss head packs e5m2 at the 8-class pitch only", KMAX, c.num_classes);
    if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return fail(-1, "bad rank/world");
    if (c.world > 1 && (c.batch % 4) != 0) return fail(-1, "data-parallel shards need batch %% 4 == 0 (noise row groups)");
    if (c.world > 1 && (c.flags & (MRGAN_FLAG_FLAT_GRADS)) == 0) return fail(-1, "world > 1 requires MRGAN_FLAG_FLAT_GRADS");
    if ((c.flags & MRGAN_FLAG_GRAD_BF16) && !(c.flags & MRGAN_FLAG_FLAT_GRADS)) return fail(-1, "MRGAN_FLAG_GRAD_BF16 requires MRGAN_FLAG_FLAT_GRADS");
    for (int i = 0; i < 5; ++i) if (c.d_hidden[i] < 1) return fail(-1, "bad d_hidden");
    if (c.g_hidden[0] < 1 || c.g_hidden[1] < 1 || c.noise_size < 1) return fail(-1, "bad generator sizes");
    if (c.models < 0 || c.models > MRGAN_MAX_MODELS) return fail(-1, "models must be in [0,%d]", MRGAN_MAX_MODELS);
    if (c.models > 1) {
        // a group trains through mrgan_sup_step_group: fp32 / bf16, fused Adam, one device
        if (c.world != 1) return fail(-3, "a model group (models = %d) needs world = 1: data-parallel groups are not built", c.models);
        if (c.dtype == MRGAN_FP8) return fail(-3, "a model group (models = %d) cannot be an fp8 handle: fp8 images and scaling slots per model are not built", c.models);
        if (c.flags & (MRGAN_FLAG_FLAT_GRADS | MRGAN_FLAG_SYNC_STATS))
            return fail(-3, "a model group (models = %d) cannot have MRGAN_FLAG_FLAT_GRADS or MRGAN_FLAG_SYNC_STATS: data-parallel groups are not built", c.models);
    }
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

// carve the workspace of ONE model; with base == nullptr only computes the size
int layout_model(mrgan_handle* h, char* base, size_t* bytes_out) {
    const mrgan_config& c = h->cfg;
    h->fp8 = c.dtype == MRGAN_FP8;
    h->bf16 = c.dtype == MRGAN_BF16 || h->fp8;            // the fp8 mode keeps the whole bf16 machinery (generator, head, evaluation)
    h->es = h->bf16 ? 2 : 4;
    const int padw = h->fp8 ? 128 : 64;      // every feature dimension is padded (zero-filled) to a multiple of this
    auto padded = [padw](int x) { return (int)round_up(x, padw); };
    h->sync_stats = (c.flags & MRGAN_FLAG_SYNC_STATS) != 0;
    h->gauss = (c.flags & MRGAN_FLAG_GAUSS_NOISE) ? 1 : 0;
    h->flat_grads = (c.flags & MRGAN_FLAG_FLAT_GRADS) != 0;
    h->ae = (c.flags & MRGAN_FLAG_AUTOENCODER) != 0;
    h->B = c.batch; h->S = (int)round_up(c.batch, SEG_ALIGN); h->tiles_m = ceil_div(c.batch, 64);   // 64-row column-sum partials
    h->Bg = c.batch * c.world;
    h->stat_count = (float)(h->sync_stats ? h->Bg : h->B);
    h->fm_scale = h->sync_stats ? 1.0f : 1.0f / (float)c.world;
    h->Dp = padded(c.d_in); h->nzp = padded(c.noise_size);
    h->F = c.d_hidden[4]; h->Fp = padded(h->F);
    h->KP = class_pitch(c.num_classes);
    const int KP = h->KP;
    const int B = h->B, S = h->S, tm = h->tiles_m;
    Arena a; a.base = base;

    h->state = a.take<DevState>(2);
    h->step_out = a.take<float>(4);
    h->accum = a.take<float>(4);
    h->err_count = a.take<int>(4);

    // ---- tensors -----------------------------------------------------------------------------
    const int gdim[4] = {c.noise_size, c.g_hidden[0], c.g_hidden[1], c.d_in};
    // (an autoencoder handle: the last dense is the full-width layer d_hidden[4] x d_in, stored like a hidden one)
    const int ddim[7] = {c.d_in, c.d_hidden[0], c.d_hidden[1], c.d_hidden[2], c.d_hidden[3], c.d_hidden[4], h->ae ? c.d_in : c.num_classes};
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
        const int K = gdim[l], N = gdim[l + 1], Kp = padded(K), Np = padded(N);
        mk(h->gt[gW[l]], K, N, Kp, Np, true);
        mk(h->gt[gb[l]], 1, N, 1, Np, false);
        h->g[l] = Dense{K, N, Kp, Np, l < 2 ? ACT_SOFTPLUS : ACT_LINEAR, &h->gt[gW[l]], &h->gt[gb[l]], nullptr, 1, Fp8Images()};
        h->gt[gW[l]].layer = &h->g[l];
    }
    mk(h->gt[2], 1, gdim[1], 1, padded(gdim[1]), false);
    mk(h->gt[3], 1, gdim[1], 1, padded(gdim[1]), false);
    for (int l = 0; l < 6; ++l) {
        const int K = ddim[l], N = ddim[l + 1], Kp = padded(K), Np = (l == 5 && !h->ae) ? KP : padded(N);
        mk(h->dt[2 * l], K, N, Kp, Np, l < 5 || h->ae);
        mk(h->dt[2 * l + 1], 1, N, 1, Np, false);
        h->d[l] = Dense{K, N, Kp, Np, l < 5 ? ACT_RELU : ACT_LINEAR, &h->dt[2 * l], &h->dt[2 * l + 1], nullptr, 1, Fp8Images()};
        h->dt[2 * l].layer = &h->d[l];
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
        // the images of a layer whose input spans xseg segments and whose gradient gseg; slots: input and gradient of the D and
        // of the G sub-step, weight
        auto images = [&](Dense& L, int xseg, int gseg, int sx0, int sx1, int sg0, int sg1, int sw) {
            Fp8Images& q = L.q;
            q.on = true; q.xseg = 0;
            q.ldxt = xseg * S; q.ldgt = gseg * S;
            q.x8 = a.take<unsigned char>((size_t)q.ldxt * L.Kp); q.x8t = a.take<unsigned char>((size_t)q.ldxt * L.Kp);
            q.g8 = a.take<unsigned char>((size_t)q.ldgt * L.Np); q.g8t = a.take<unsigned char>((size_t)q.ldgt * L.Np);
            q.w8 = a.take<unsigned char>((size_t)L.Kp * L.Np); q.w8t = a.take<unsigned char>((size_t)L.Kp * L.Np);
            q.sx[0] = sx0; q.sx[1] = sx1; q.sg[0] = sg0; q.sg[1] = sg1; q.sw = sw;
        };
        // discriminator: the three segments of the D sub-step (the G sub-step uses two, then one), slots per sub-step kind
        for (int l = 0; l < 5; ++l) images(h->d[l], 3, 3, l, 10 + l, 5 + l, 15 + l, 20 + l);      // slots [kind][x | g][l], then w[l]
        // generator layer G2 (the one wide product of the generator): BN(h1) of both segments of a paired forward, dpre2 of the G
        // sub-step; the D sub-step's generator pass may be the G sub-step's too, so the two kinds share their slots
        images(h->g[1], 2, 1, 25, 25, 26, 26, 27);
        h->slots = a.take<Fp8Slot>(FP8_NSLOT); h->slot_targets = a.take<float>(FP8_NSLOT); h->accum_save = a.take<float>(4);
    }
    h->dxfake = act(S, h->Dp); h->dpre2g = act(S, h->g[1].Np); h->dhbn = act(S, N1p); h->dpre1g = act(S, N1p);
    h->logits = a.take<float>(3 * (size_t)S * KP);
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
    // sub-step on the matrix cores too (64-row blocks, as the chain's); at the 32-class pitch, where the D-tail chain does not
    // run, so does a 256-wide feature layer (one chunk)
    h->head_wide_ok = h->head_wide = h->bf16 && (h->Fp > CH_PW || (KP > KMAX && h->Fp == CH_PW)) && (h->Fp % CH_PW) == 0;
    h->w6c = h->w6r = nullptr;
    if (h->head_wide) { h->w6c = a.take<__bf16>((size_t)3 * KP * h->Fp); h->w6r = a.take<__bf16>((size_t)3 * KP * h->Fp); }
    const int head_cap = 3 * ceil_div(B, HEAD_ROWS);                      // partial rows of the per-layer head; the 64-row heads fill fewer
    h->head_stride = (int)round_up(h->Fp * KP + KP + h->Fp, 64);      // dW6 | db6 | bias grad of the feature layer
    h->head_groups = std::min(8, 3 * ceil_div(B, CH_ROWS));
    h->head_part = a.take<float>((size_t)head_cap * h->head_stride);
    h->head_red = a.take<float>((size_t)h->head_groups * h->head_stride);
    h->loss_part = a.take<float>((size_t)head_cap * 4);
    h->cs_db[4] = nullptr; h->ae_y = h->ae_dy = nullptr; h->ae_cs = h->ae_loss_part = h->ae_mse = nullptr;
    if (h->ae) {
        h->ae_y = act(3 * (size_t)S, h->Dp); h->ae_dy = act(S, h->Dp);
        h->cs_db[4] = a.take<float>((size_t)tm * h->Fp); h->ae_cs = a.take<float>((size_t)tm * h->Dp);
        h->ae_loss_part = a.take<float>((size_t)(3 * S / 64) * (h->Dp / 64) * 4);      // (a chunk of mrgan_ae_reconstruct: 3 S rows)
        h->ae_mse = a.take<float>(4);
    }

    // ---- weight-gradient slabs ---------------------------------------------------------------------
    int tiles_d = 0, tiles_g = 0;
    const int nl_d = h->ae ? 6 : 5;                  // discriminator layers whose weight gradient is a product of its own
    for (int l = 0; l < nl_d; ++l) tiles_d += dw_tiles(h->d[l]);
    for (int l = 0; l < 3; ++l) tiles_g += dw_tiles(h->g[l]);
    // (256 x 128 output tiles with one 8-wave block per CU were tried for the discriminator's launch in round 3: 25 % fewer staged
    //  bytes per flop, but 54.5 us against 47.5 us with two- and three-stage rings -- 200 blocks leave a fifth of the CUs idle)
    // (the autoencoder step has one segment)
    const int splits_d = choose_splits(tiles_d, h->ae ? S : 2 * S + B), splits_g = choose_splits(tiles_g, B);
    for (int l = 0; l < nl_d; ++l) {
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
    for (int l = 0; l < nl_d; ++l) src(*h->d[l].W, h->d[l].slabs, h->d[l].splits, (long)h->d[l].Kp * h->d[l].Np);
    for (int l = 0; l < 4; ++l) src(*h->d[l].b, h->cs_db[l], 3 * tm, h->d[l].Np);
    if (h->ae) {
        // the dX product through the last layer leaves the column sums behind b5, the reconstruction head those behind b6
        src(*h->d[4].b, h->cs_db[4], tm, h->Fp);
        src(*h->d[5].b, h->ae_cs, tm, h->Dp);
    } else {
        src(*h->d[4].b, h->head_red + h->Fp * KP + KP, h->head_groups, h->head_stride);
        src(*h->d[5].W, h->head_red, h->head_groups, h->head_stride);
        src(*h->d[5].b, h->head_red + h->Fp * KP, h->head_groups, h->head_stride);
    }
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

// The whole workspace: the layout above once per model, W bytes apart.  Everything -- split counts, slab
// and tile counts, the Adam tile tables -- is chosen from the per-model shape and describes model 0; a grouped launch reaches
// model m's copy with the one stride W.  The generator's regions are present and unused in every copy; the DevState slots of
// model 0's copy are the shared ones.
int layout(mrgan_handle* h, char* base, size_t* bytes_out) {
    size_t one = 0;
    const int r = layout_model(h, base, &one);
    h->models = std::max(1, (int)h->cfg.models);
    h->W = h->models > 1 ? one : 0;                 // (already a multiple of 256)
    *bytes_out = one * (size_t)h->models;
    return r;
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
                if (t.layer && t.layer->q.on) {
                    const Fp8Images& q = t.layer->q;
                    a.w8 = q.w8 + off; a.w8t = q.w8t + (long)c0 * t.prow + r0; a.w8_slot = h->slots + q.sw;
                }
                a.ld = t.pcol; a.ldt = t.prow;
                a.rows = std::min(TR, t.prow - r0); a.cols = std::min(64, t.pcol - c0);
                v.push_back(a);
            }
    if ((int)v.size() != n) return fail(-20, "tile count mismatch");
    HIPCHK(hipMemcpyAsync(dev, v.data(), sizeof(AdamTile) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));      // v dies at scope exit
    return 0;
}

Tensor* find_tensor(mrgan_handle* h, int net, int idx) {
    std::vector<Tensor>& ts = net == MRGAN_NET_G ? h->gt : h->dt;
    if (net != MRGAN_NET_G && net != MRGAN_NET_D) return nullptr;
    if (idx < 0 || idx >= (int)ts.size()) return nullptr;
    return &ts[idx];
}

}  // namespace

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
    h->head_nblk = 0; h->fp8_cal[0] = h->fp8_cal[1] = 0;
    h->sel = 0; h->grouped = 1;
    if (init_kernel_attributes() != 0 || chain_init_attributes() != 0 || head_wide_init_attributes() != 0) { if (h->own_ws) hipFree(h->ws); delete h; return fail(-10, "hipFuncSetAttribute failed"); }
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
    if (!h->fp8) {      // (mrgan_attribution refuses an fp8 handle)
        CREATE_CHK(hipMalloc((void**)&h->draw_state, sizeof(DevState) * MRGAN_ATTR_MAX_DRAWS));
        hipLaunchKernelGGL(init_draw_state_kernel, dim3(ceil_div(MRGAN_ATTR_MAX_DRAWS, 256)), dim3(256), 0, s, h->draw_state, (int)MRGAN_ATTR_MAX_DRAWS);
    }
    r = upload_tiles(h, h->gt, h->tiles_g_dev, h->ntiles_g, s);
    if (!r) r = upload_tiles(h, h->dt, h->tiles_d_dev, h->ntiles_d, s);
    if (r) { if (h->own_ws) hipFree(h->ws); delete h; return r; }
    if (h->fp8) {
        float tg[FP8_NSLOT] = {};
        for (int net : {MRGAN_NET_D, MRGAN_NET_G}) {
            int n;
            const Dense* Ls = net_layers(h, net, &n);
            for (int l = 0; l < n; ++l) {
                const Fp8Images& q = Ls[l].q;
                if (!q.on) continue;
                for (int k = 0; k < 2; ++k) { tg[q.sx[k]] = FP8_TARGET_E4M3; tg[q.sg[k]] = FP8_TARGET_E5M2; }
                tg[q.sw] = FP8_TARGET_E4M3;
            }
        }
        CREATE_CHK(hipMemcpyAsync(h->slot_targets, tg, sizeof tg, hipMemcpyHostToDevice, s));
        CREATE_CHK(hipStreamSynchronize(s));
        if (launch_fp8_init_slots(h->slots, FP8_NSLOT, h->slot_targets, s) != 0) { if (h->own_ws) hipFree(h->ws); delete h; return fail(-10, "fp8 slot init failed"); }
    }
    // BN gamma defaults to one (Keras); dense weights stay zero until mrgan_set_weights
    std::vector<float> ones(h->gt[2].cols, 1.0f);
    for (int m = 0; m < h->models; ++m)
        CREATE_CHK(hipMemcpyAsync(model_at(h, h->gt[2].p, m), ones.data(), sizeof(float) * ones.size(), hipMemcpyHostToDevice, s));
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

int mrgan_select_model(mrgan_handle* h, int model) {
    if (!h) return fail(-1, "null handle");
    if (model < 0 || model >= h->models) return fail(-1, "select_model: model %d outside [0,%d)", model, h->models);
    h->sel = model;
    return 0;
}

// (the per-model entries below address the selected model's copy of the tensor: selected(), engine_internal.h)
int mrgan_set_weights(mrgan_handle* h, int net, int idx, const float* src, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !src) return fail(-1, "set_weights: bad tensor or null source");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpy2DAsync(selected(h, t->p), sizeof(float) * t->pcol, src, sizeof(float) * t->cols, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, s));
    if (t->w16) hipLaunchKernelGGL(refresh_bf16_kernel, grid2d(t->prow, t->pcol), dim3(256), 0, s, selected(h, t->p), selected(h, t->w16), selected(h, t->wt16), t->prow, t->pcol);
    if (t->layer && t->layer->q.on) {
        // fp8 copies of the network's weights: the first pass only measures max |w|, the second stores with that scale
        for (int pass = 0; pass < 2; ++pass) { CHK(fp8_refresh_weights(h, net, s)); CHK(fp8_update_scales(h, s)); }
    }
    return 0;
}

int mrgan_get_weights(mrgan_handle* h, int net, int idx, float* dst, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !dst) return fail(-1, "get_weights: bad tensor or null destination");
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * t->cols, selected(h, t->p), sizeof(float) * t->pcol, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mrgan_get_slot(mrgan_handle* h, int net, int idx, int which, float* dst, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !dst || which < 0 || which > 2) return fail(-1, "get_slot: bad argument");
    if (which == 2 && t->flat16) return fail(-3, "get_slot: the flat gradients of this handle are bfloat16 (MRGAN_REGION_GRAD_*_BF16)");
    const float* src = selected(h, which == 0 ? t->m : which == 1 ? t->v : t->flat);
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * t->cols, src, sizeof(float) * t->pcol, sizeof(float) * t->cols, t->rows,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int mrgan_set_slot(mrgan_handle* h, int net, int idx, int which, const float* src, mrgan_stream stream) {
    Tensor* t = find_tensor(h, net, idx);
    if (!t || !src || which < 0 || which > 1) return fail(-1, "set_slot: bad argument");
    float* dst = selected(h, which == 0 ? t->m : t->v);
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

int mrgan_read_metrics(mrgan_handle* h, float* out8, int reset, mrgan_stream stream) {
    if (!h || !out8) return fail(-1, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out8, selected(h, h->accum), 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out8 + 4, selected(h, h->step_out), 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(selected(h, h->accum), 0, 4 * sizeof(float), s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
