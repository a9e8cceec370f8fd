// The launch sequence of one discriminator sub-step and one generator sub-step (mr_gan.py:204-213), evaluation, and the
// step entries of include/mrgan_abi.h.
#include "engine_internal.h"

namespace mrgan {
thread_local LaunchTimer g_launch_timer = {nullptr, nullptr, 0, 0};      // see MRGAN_LAUNCH (common.h)
}

namespace {

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
    const Epi& e = g.e;
    const bool fp8 = e.qa != nullptr;                 // the description carries fp8 operands
    const char* kname = fp8 ? "gemm_fp8" : "gemm";
    algo_flops *= gemm_models(g); algo_bytes *= gemm_models(g);      // (a model group: the caller counted one model)
    prof_arm(h);
    const int r = fp8 ? launch_gemm_fp8(epi, g, s, &kname) : h->bf16 ? launch_gemm_bf16(epi, g, s, &kname) : launch_gemm_f32(epi, g, s, &kname);
    if (fp8) {
        // operands are bytes; outputs: fp8 (+ transposed copy) or bf16, the weight gradient fp32
        const double out_b = epi == EPI_SLAB ? 4.0 : (e.out ? 2.0 : 0.0) + (e.q8 ? 1.0 : 0.0) + (e.q8t ? 1.0 : 0.0);
        algo_bytes = (double)g.nbatch * g.M * g.K + (double)g.K * g.N + (double)g.nbatch * g.M * g.N * out_b;
    }
    prof_done(h, kname, algo_flops, algo_bytes);
    CHK(r);
    return 0;
}
// activations [rows][K] in, [rows][N] out (element size es), the weight matrix once
double dense_bytes(const mrgan_handle* h, double rows, const Dense& L) { return (rows * ((double)L.K + L.N) + (double)L.K * L.N) * h->es; }
// weight gradient: both activation operands once, the fp32 gradient once
double dw_bytes(const mrgan_handle* h, double rows, const Dense& L) { return rows * ((double)L.K + L.N) * h->es + (double)L.K * L.N * 4.0; }

// what every product of the engine takes from the handle: noise key, live state slot, tuning
GemmArgs with_handle(mrgan_handle* h, GemmArgs g) {
    Epi& e = g.e;
    e.seed = h->cfg.seed;
    e.gauss = h->gauss;
    e.row0 = (uint32_t)(h->cfg.rank * h->B);
    e.st = h->state + h->cur;
    e.ablate = h->ablate; e.tune_kc_cfg = h->tune_kc_cfg; e.tune_bits = h->tune_bits;
    e.seg_step = 1;
    // a grouped step: the launch covers every model, model m's tensors W bytes behind model m - 1's
    return gemm_group(g, h->grouped, (long)h->W);
}

// ---- what a dense product is told beside its operands ----
// who runs it: a sub-step kind (which scaling slots a layer's fp8 images use), or the evaluation (learning phase 0: no noise
// state, and bf16 operands whatever the layer owns)
enum { KIND_EVAL = -1, KIND_D = 0, KIND_G = 1 };
// GaussianNoise added to a forward product's output: drawn at (site, seg0 + batch * seg_step, iteration + batch * iter_step)
struct NoiseSite { float sigma; uint32_t site, seg0; int seg_step; uint32_t iter_step; };
const NoiseSite NO_NOISE = {0.f, 0, 0, 1, 0};
struct ReluMask { const uint16_t* words; int ldm; };      // lane-native relu mask: written by a forward product, read by a dX
const ReluMask NO_MASK = {nullptr, 0};
struct ColSums { int mode; float* cs1; float* cs2; };     // column partial sums per 64 rows
const ColSums NO_SUMS = {CS_NONE, nullptr, nullptr};
// a layer with fp8 images (Fp8Images, engine_internal.h) reads its operand from them; this says how they are filled:
//   to        the layer whose images take the product's output -- a forward product's next layer (its input images), a dX
//             product's previous one (its gradient images); the bf16 tensor `out` is not stored then, nothing reads it
//   wgrad     weight gradients follow in this sub-step: the transposed images are written too
//   quant_in  the operand is a stored bf16 tensor (xin_0, BN(h1), dpre2 of the generator): a quantiser pass fills the
//             layer's own images first
struct Fp8Use { const Dense* to; bool wgrad, quant_in; };
const Fp8Use NO_FP8 = {nullptr, false, false};
// mrgan_attribution: what keys the noise of draw d of an evaluation forward -- a constant state slot whose iter is d
// (mrgan_handle::draw_state), the selected model's seed and the chunk's first row
struct DrawKey { const DevState* st; uint64_t seed; uint32_t row0; };

ReluMask relu_mask(const mrgan_handle* h, int l) { return ReluMask{h->mask[l], h->ldm[l]}; }
void epi_mask(mrgan_handle* h, Epi& e, const ReluMask& m) {
    e.mask = (uint16_t*)m.words; e.mask_bs = mask_pitch(h->S, m.ldm); e.ldm = m.ldm;
}
void epi_sums(Epi& e, const ColSums& cs, int ldcs) { e.cs_mode = cs.mode; e.cs1 = cs.cs1; e.cs2 = cs.cs2; e.ldcs = ldcs; }
// the product's output goes to fp8 images [nb][S][ld] (+ transposed, pitch ldt) under `slot` instead of the bf16 tensor
void epi_images(mrgan_handle* h, Epi& e, unsigned char* img, unsigned char* imgt, int ld, int ldt, int slot) {
    e.out = nullptr;
    e.qo = h->slots + slot;
    e.q8 = img; e.q8_bs = (long)h->S * ld; e.ldq8 = ld;
    if (imgt) { e.q8t = imgt; e.q8t_bs = h->S; e.ldq8t = ldt; }
}
unsigned char* x8_view(const mrgan_handle* h, const Dense& L) { return L.q.x8 + (size_t)L.q.xseg * h->S * L.Kp; }
unsigned char* x8t_view(const mrgan_handle* h, const Dense& L) { return L.q.x8t + (size_t)L.q.xseg * h->S; }

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
// a stored bf16 tensor [nb][S][width] -> fp8 images (row-major; transposed with pitch ldt where imgt is given)
int fp8_quant_images(mrgan_handle* h, const void* src, int width, int nb, unsigned char* img, unsigned char* imgt, int ldt, int slot,
                     int fmt, hipStream_t s) {
    const long bs = (long)h->S * width;
    return fp8_quant(h, src, bs, width, h->B, width, (int)round_up(h->B, 64), nb, img, bs, width, imgt, h->S, ldt, slot, fmt, s);
}

// Y = act(X W + b): X [nb][S][Kp] -> out [nb][S][Np]
int dense_fwd(mrgan_handle* h, const Dense& L, int kind, const void* x, int rows, int nb, void* out, int act, const NoiseSite& nz,
              const ReluMask& m, const ColSums& cs, hipStream_t s, const Fp8Use& f8 = NO_FP8, const DrawKey* dk = nullptr) {
    const Fp8Images& q = L.q;
    const bool fp8 = q.on && kind != KIND_EVAL;
    const long a_bs = (long)h->S * L.Kp;
    if (fp8 && f8.quant_in)
        CHK(fp8_quant_images(h, x, L.Kp, nb, x8_view(h, L), f8.wgrad ? x8t_view(h, L) : nullptr, q.ldxt, q.sx[kind], FP8_E4M3, s));
    GemmArgs g = with_handle(h, fp8       ? gemm_fwd_args(rows, L.Kp, L.Np, nb, x8_view(h, L), a_bs, L.Kp, q.w8t, L.Kp, true)
                                : h->bf16 ? gemm_fwd_args(rows, L.Kp, L.Np, nb, x, a_bs, L.Kp, L.W->wt16, L.Kp, true)
                                          : gemm_fwd_args(rows, L.Kp, L.Np, nb, x, a_bs, L.Kp, L.W->p, L.Np, false));
    Epi& e = g.e;
    e.act = act; e.n_valid = L.N; e.bias = L.b->p;
    if (kind == KIND_EVAL) {        // evaluation runs model by model: the selected model's weights (x and out are the caller's)
        e.st = nullptr;
        if (dk) { e.st = dk->st; e.seed = dk->seed; e.row0 = dk->row0; }      // (noise of an attribution draw)
        g.B = selected(h, g.B); e.bias = selected(h, e.bias);
    }
    e.out = out; e.out_bs = (long)h->S * L.Np; e.ldo = L.Np;
    e.sigma = nz.sigma; e.site = nz.site; e.seg0 = nz.seg0; e.seg_step = nz.seg_step; e.iter_step = nz.iter_step;
    epi_mask(h, e, m);
    epi_sums(e, cs, L.Np);
    if (fp8) {
        e.qa = h->slots + q.sx[kind]; e.qb = h->slots + q.sw;
        if (f8.to && f8.to->q.on) epi_images(h, e, f8.to->q.x8, f8.wgrad ? f8.to->q.x8t : nullptr, L.Np, f8.to->q.ldxt, f8.to->q.sx[kind]);
    }
    return run_gemm(h, EPI_FWD, g, 2.0 * rows * nb * L.K * L.N, dense_bytes(h, (double)rows * nb, L), s);
}

// dX = (dY W^T) * act'(prev): dY [nb][S][Np] -> out [nb][S][Kp]
int dense_dx(mrgan_handle* h, const Dense& L, int kind, const void* dy, int rows, int nb, void* out, int act, int n_valid,
             const ReluMask& m, const void* hprev, const ColSums& cs, hipStream_t s, const Fp8Use& f8 = NO_FP8) {
    const Fp8Images& q = L.q;
    const long a_bs = (long)h->S * L.Np;
    if (q.on && f8.quant_in)
        CHK(fp8_quant_images(h, dy, L.Np, nb, q.g8, f8.wgrad ? q.g8t : nullptr, q.ldgt, q.sg[kind], FP8_E5M2, s));
    GemmArgs g = with_handle(h, q.on ? gemm_dx_args(rows, L.Kp, L.Np, nb, q.g8, a_bs, L.Np, q.w8, L.Np)
                                     : gemm_dx_args(rows, L.Kp, L.Np, nb, dy, a_bs, L.Np,
                                                    h->bf16 ? (const void*)L.W->w16 : (const void*)L.W->p, L.Np));
    Epi& e = g.e;
    e.act = act; e.n_valid = n_valid;
    if (kind == KIND_EVAL) g.B = selected(h, g.B);      // (model by model, as dense_fwd: dy, out and the mask are the caller's)
    e.out = out; e.out_bs = (long)h->S * L.Kp; e.ldo = L.Kp;
    epi_mask(h, e, m);
    e.h = hprev; e.h_bs = (long)h->S * L.Kp; e.ldh = L.Kp;
    epi_sums(e, cs, L.Kp);
    e.bn_mu = h->bn_mu; e.bn_rstd = h->bn_rstd;
    if (q.on) {
        e.qa = h->slots + q.sg[kind]; e.qb = h->slots + q.sw;
        if (f8.to && f8.to->q.on) epi_images(h, e, f8.to->q.g8, f8.wgrad ? f8.to->q.g8t : nullptr, L.Kp, f8.to->q.ldgt, f8.to->q.sg[kind]);
    }
    return run_gemm(h, EPI_DX, g, 2.0 * rows * nb * L.K * L.N, dense_bytes(h, (double)rows * nb, L), s);
}

// dW slabs = X^T dY.  The nseg segments ([nseg][S] rows, `rows` valid in each) form ONE virtual reduction
// range that is cut into L.splits slabs, so the Adam kernel sums at most MAX_SLABS slabs per tensor.
double dw_args(mrgan_handle* h, GemmArgs& g, const Dense& L, int kind, const void* x, const void* dy, int rows, int nseg) {
    // bf16 and fp8: reduce over ALL S rows of every segment.  The rows >= `rows` of dY are never written by any kernel (they keep
    // the zeros of mrgan_create; an fp8 image stores them as zeros) and those of X are finite, so they add exact zeros -- and the
    // reduction range becomes dense, which is what the LDS-DMA weight-gradient kernel and the grouped launch need (a ragged batch
    // such as the reference's 50 otherwise fell back to one register-staged launch per product).
    const bool dense = h->bf16 != 0;
    const int vrows = dense ? nseg * h->S : (nseg - 1) * h->S + rows;
    if (L.q.on) {       // the transposed images: reduction index contiguous in both operands
        g = with_handle(h, gemm_dw_args(L.Kp, L.Np, vrows, L.splits, vrows / L.splits, 0, 0, x8t_view(h, L), L.q.ldxt, L.q.g8t, L.q.ldgt,
                                        true, L.slabs));
        g.e.qa = h->slots + L.q.sx[kind]; g.e.qb = h->slots + L.q.sg[kind];
    } else {
        g = with_handle(h, gemm_dw_args(L.Kp, L.Np, vrows, L.splits, gemm_dw_kchunk(vrows, L.splits), h->S, dense ? h->S : rows,
                                        x, L.Kp, dy, L.Np, false, L.slabs));
    }
    return 2.0 * rows * nseg * L.K * L.N;
}

struct DwJob { const Dense* L; const void* x; const void* dy; };

// the weight-gradient products of sub-step `kind`: those of the bf16 fast path as one grouped launch, one launch per product
// otherwise -- a layer with fp8 images, fp32, or a group the launcher declines -- with the fold as a launch of its own then
int dense_dw_all(mrgan_handle* h, int kind, const DwJob* jobs, int n, int rows, int nseg, hipStream_t s, const FoldJob* fold = nullptr) {
    GemmArgs gs[KS_GROUP_MAX];
    DwJob js[KS_GROUP_MAX];
    double fl[KS_GROUP_MAX], total = 0.0, bytes = 0.0;
    if (n > KS_GROUP_MAX) return fail(-1, "dense_dw_all: too many products");
    std::copy(jobs, jobs + n, js);
    // the jobs without images first (order kept): the candidates of the grouped launch
    const int ngroup = (int)(std::stable_partition(js, js + n, [](const DwJob& j) { return !j.L->q.on; }) - js);
    for (int i = 0; i < n; ++i) fl[i] = dw_args(h, gs[i], *js[i].L, kind, js[i].x, js[i].dy, rows, nseg);
    for (int i = 0; i < ngroup; ++i) { total += fl[i] * h->grouped; bytes += dw_bytes(h, (double)rows * nseg, *js[i].L) * h->grouped; }
    int first = 0;
    if (h->bf16 && ngroup > 0) {
        const char* kname = "gemm";
        prof_arm(h);
        const int r = launch_gemm_bf16_dw_group(gs, ngroup, s, &kname, fold);
        prof_done(h, kname, total, bytes);
        if (r < 0) return fail(r, "grouped weight-gradient launch failed");
        if (r == 0) { first = ngroup; fold = nullptr; }
    }
    for (int i = first; i < n; ++i) CHK(run_gemm(h, EPI_SLAB, gs[i], fl[i], dw_bytes(h, (double)rows * nseg, *js[i].L), s));
    if (fold) PROF("reduce_partials_kernel", launch_reduce_partials(fold->src, fold->nsrc, fold->stride, fold->n, fold->ngroups, fold->dst, s,
                                                                    h->grouped, fold->model_stride));
    return 0;
}

}  // namespace
int mrgan::fp8_update_scales(mrgan_handle* h, hipStream_t s) {
    PROF("fp8_update_scales_kernel", launch_fp8_update_scales(h->slots, FP8_NSLOT, s));
    return 0;
}
// the fp8 weight copies of the layers of `net` that own images, from the bf16 copies
int mrgan::fp8_refresh_weights(mrgan_handle* h, int net, hipStream_t s) {
    int n;
    const Dense* Ls = net_layers(h, net, &n);
    for (int l = 0; l < n; ++l) {
        const Dense& L = Ls[l];
        if (L.q.on) CHK(fp8_quant(h, L.W->w16, 0, L.Np, L.Kp, L.Np, L.Kp, 1, L.q.w8, 0, L.Np, L.q.w8t, 0, L.Kp, L.q.sw, FP8_E4M3, s));
    }
    return 0;
}
namespace {

// lp (optional): the loss partials [nlp][4] and their scale instead of the loss head's (the autoencoder step)
int run_adam(mrgan_handle* h, int net, int mode, bool with_metrics, hipStream_t s, int advance_batch = 0, const float* lp = nullptr,
             int nlp = 0, float lp_scale = 0.f) {
    AdamArgs a;
    memset(&a, 0, sizeof a);
    if (mode != ADAM_REDUCE_ONLY) { a.next = h->state + (h->cur ^ 1); a.advance_batch = advance_batch; a.lr = h->cfg.lr; }
    a.tiles = net == MRGAN_NET_D ? h->tiles_d_dev : h->tiles_g_dev;
    a.ntiles = net == MRGAN_NET_D ? h->ntiles_d : h->ntiles_g;
    a.mode = mode; a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.adam_eps;
    a.st = h->state + h->cur;
    if (with_metrics) {
        a.loss_part = h->loss_part; a.nloss_part = h->head_nblk; a.inv_rows = 1.0f / (float)h->Bg;
        a.step_out = h->step_out; a.accum = h->accum;
        a.flat_tail = h->flat_d + h->flat_d_n;
        if (lp) { a.loss_part = lp; a.nloss_part = nlp; a.inv_rows = lp_scale; }
    }
    a.models = h->grouped; a.model_stride = (long)h->W;
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

// generator forward up to the BatchNorm statistics (phase *_GEN) and from there to the fake rows.
// nb = 2 (pair_gen): segment 0 is this D sub-step's batch, segment 1 the following G sub-step's (its z, noise
// iteration and noise segment id are those the G sub-step would use on its own, so the results are identical).
// Either sub-step runs these passes as KIND_D: a paired pass serves both, so G2's images share their slots between the kinds.
int gen_fwd_head(mrgan_handle* h, int nb, hipStream_t s) {
    CHK(dense_fwd(h, h->g[0], KIND_D, h->zbuf, h->B, nb, h->h1, ACT_SOFTPLUS, NO_NOISE, NO_MASK, ColSums{CS_SUM_SQ, h->cs_bn1, h->cs_bn2}, s));
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
    b.models = h->grouped; b.model_stride = (long)h->W;
    PROF("bn_apply_kernel", launch_bn_apply(h->bf16, b, s));
    // fp8: BN(h1) is quantised with its transpose (the weight gradient of the G sub-step reads it, also after a paired pass)
    CHK(dense_fwd(h, h->g[1], KIND_D, h->hbn, h->B, nb, h->h2, ACT_SOFTPLUS, NO_NOISE, NO_MASK, NO_SUMS, s, Fp8Use{nullptr, true, true}));
    // generator output + GaussianNoise(sigma0) = the discriminator's noisy input rows of the fake segment.
    // Paired: segment 1 lands in the next xin[0] slot and is drawn as (segment id 0, iteration + 1), the G sub-step's fake rows.
    void* out = rowptr(h, h->xin[0], (long)fake_seg_slot * h->S, h->Dp);
    const NoiseSite nz = {h->cfg.sigma[0], 0, fake_seg_id, nb > 1 ? -(int)fake_seg_id : 1, nb > 1 ? 1u : 0u};
    CHK(dense_fwd(h, h->g[2], KIND_D, h->h2, h->B, nb, out, ACT_LINEAR, nz, NO_MASK, NO_SUMS, s));
    return 0;
}

// discriminator dense 1..5 over nb segments of sub-step `kind` (learning phase 1: noise on).  fp8: the noisy input rows of
// dense 1 are quantised, every product fills the next layer's images, transposed too where weight gradients follow (D)
int disc_fwd_train(mrgan_handle* h, int kind, int nb, bool fm_sums, int x0_slot, hipStream_t s, int l_end = 5) {
    for (int l = 0; l < l_end; ++l) {
        const void* in = l == 0 ? rowptr(h, h->xin[0], (long)x0_slot * h->S, h->Dp) : h->xin[l];
        void* out = l < 4 ? h->xin[l + 1] : h->feat;
        const NoiseSite nz = {l < 4 ? h->cfg.sigma[l + 1] : 0.f, (uint32_t)(l + 1), 0, 1, 0};
        const bool last = l == 4;
        CHK(dense_fwd(h, h->d[l], kind, in, h->B, nb, out, ACT_RELU, nz, relu_mask(h, l), ColSums{(last && fm_sums) ? CS_SUM : CS_NONE, h->cs_f, nullptr},
                      s, Fp8Use{last ? nullptr : &h->d[l + 1], kind == KIND_D, l == 0}));
    }
    return 0;
}

// ---- row-block chain launches for the tail D3..D5 (+ head) of the discriminator (gemm_chain.hip) ----
ChainOp chain_fwd_op(mrgan_handle* h, int l, bool fm_sums) {
    const Dense& L = h->d[l];
    ChainOp o;
    memset(&o, 0, sizeof o);
    o.K = L.Kp; o.N = L.Np; o.n_valid = L.N; o.W = L.W->wt16;
    o.bias = L.b->p; o.sigma = l < 4 ? h->cfg.sigma[l + 1] : 0.f; o.site = (uint32_t)(l + 1);
    o.out = (__bf16*)(l < 4 ? h->xin[l + 1] : h->feat); o.out_bs = (long)h->S * L.Np; o.ldo = L.Np;
    o.mask = h->mask[l]; o.mask_bs = mask_pitch(h->S, h->ldm[l]); o.ldm = h->ldm[l];
    if (fm_sums) { o.cs = h->cs_f; o.ldcs = L.Np; }
    return o;
}
// dX of layer l: dpre[l] -> dpre[l-1]
ChainOp chain_dx_op(mrgan_handle* h, int l, bool bias_sums) {
    const Dense& L = h->d[l];
    ChainOp o;
    memset(&o, 0, sizeof o);
    o.K = L.Np; o.N = L.Kp; o.n_valid = h->d[l - 1].N; o.W = L.W->w16;
    o.out = (__bf16*)h->dpre[l - 1]; o.out_bs = (long)h->S * L.Kp; o.ldo = L.Kp;
    o.mask = h->mask[l - 1]; o.mask_bs = mask_pitch(h->S, h->ldm[l - 1]); o.ldm = h->ldm[l - 1];
    if (bias_sums) { o.cs = h->cs_db[l - 1]; o.ldcs = L.Kp; }
    return o;
}
// rows per block of a G sub-step chain launch: 32 when 64-row blocks would leave more than half of the CUs without a block
// (the 3-stage weight ring of the 32-row blocks keeps two k-tiles in flight: every reduction of the chain must have two)
int chain_block_rows(const mrgan_handle* h, int nseg) {
    const int kmin = std::min(std::min(h->d[2].Kp, h->d[2].Np), std::min(h->d[3].Np, h->d[4].Np));
    return (nseg * ceil_div(h->B, 64) <= 128 && kmin >= 128) ? 32 : 64;
}
double chain_flops(const mrgan_handle* h, const ChainArgs& c, bool with_head) {
    double f = 0.0;
    for (int l = 2; l < 5; ++l) f += 2.0 * h->B * c.nseg * h->d[l].K * h->d[l].N;     // each product appears once per direction
    return f * (with_head ? 2.0 : 1.0) * std::max(1, c.models);       // (a model group: every model's products)
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
        if (nb) fprintf(stderr, "chain stamps (kcycles per block, %d blocks): prologue %.1f | pass setup %.1f | head %.1f | tile wait %.1f | barrier %.1f | "
                        "issue+reads+mfma %.1f | epilogue %.1f | image barrier+copy-out %.1f\n", nb, tot[0] / nb / 1e3, tot[1] / nb / 1e3,
                        tot[2] / nb / 1e3, tot[3] / nb / 1e3, tot[4] / nb / 1e3, tot[5] / nb / 1e3, tot[6] / nb / 1e3, tot[7] / nb / 1e3);
    }
#endif
    // algorithmic bytes (logical widths, bf16): the first A image, every product's weights and stored output
    double bytes = 0.0;
    const double nrows = (double)c.rows * c.nseg * std::max(1, c.models);
    const bool has_fwd = c.variant != CH_V_GBWD, has_dx = c.variant != CH_V_GFWD;
    if (has_fwd) bytes += nrows * h->d[2].K * 2.0;
    else bytes += nrows * h->F * 2.0;                                  // the stored features whose sign is the relu mask
    for (int l = 2; l < 5; ++l) {
        const double w = (double)h->d[l].K * h->d[l].N * 2.0 * std::max(1, c.models);
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
        if (h->grouped > 1) { zs.models = h->grouped; zs.src_ms = h->gs.z; zs.out_ms = (long)h->W; }      // (a grouped sub-step: every model its own z)
        st.nseg = slot + 1;
        if (paired_z) {                                 // the following G sub-step's z (drawn on device at iteration + 1)
            StageSeg& z2 = st.s[slot + 1];
            z2 = zs;
            z2.out = rowptr(h, h->zbuf_all, h->S, h->nzp); z2.gen = 1; z2.src = nullptr; z2.stream = 0; z2.iter_off = 1;
            st.nseg = slot + 2;
        }
    }
    st.seed = h->cfg.seed; st.row0 = (uint32_t)(h->cfg.rank * h->B); st.gauss = h->gauss;
    st.cur = h->state + h->cur;
    return 0;
}
// (src_ms / idx_ms: elements between the models' rows and index vectors in a grouped step)
void data_seg(StageSeg& sg, mrgan_handle* h, const float* x, const int32_t* idx, long ld, int slot, uint32_t seg_id, int stream_mode,
              long src_ms, long idx_ms) {
    memset(&sg, 0, sizeof sg);
    if (h->grouped > 1) { sg.models = h->grouped; sg.src_ms = src_ms; sg.idx_ms = idx_ms; sg.out_ms = (long)h->W; }
    sg.src = x; sg.idx = idx; sg.ld = ld; sg.rows = h->B; sg.cols = h->cfg.d_in; sg.cols_pad = h->Dp;
    sg.out = rowptr(h, h->xin[0], (long)slot * h->S, h->Dp); sg.ldo = h->Dp;
    sg.sigma = h->cfg.sigma[0]; sg.site = 0; sg.seg = seg_id; sg.gen = 0; sg.stream = stream_mode;
}

// ---------------------------------------------------------------------------------------------------
// loss head
// ---------------------------------------------------------------------------------------------------
// The head over `rows` rows of each of kinds.size() segments of h->feat.  train: the segments lie S rows apart and the head
// leaves its gradients (dpre of the feature layer, per-block partials of dW6 | db6 | the feature layer's bias gradient) and
// loss partials; otherwise one run of contiguous rows, logits only.  Labels and the loss scale are the caller's.
HeadArgs head_args(mrgan_handle* h, std::initializer_list<int> kinds, int rows, bool train) {
    HeadArgs hd;
    memset(&hd, 0, sizeof hd);
    hd.f = h->feat; hd.ldf = h->Fp; hd.rows = rows;
    for (int k : kinds) hd.seg_kind[hd.nseg++] = k;
    hd.feat = h->Fp; hd.feat_valid = h->F; hd.classes = h->cfg.num_classes;
    hd.w = h->dt[10].p; hd.ldw = h->KP; hd.b = h->dt[11].p;
    hd.st = h->state + h->cur;
    hd.logits = h->logits;
    if (!train) return hd;
    hd.f_bs = (long)h->S * h->Fp; hd.logits_bs = (long)h->S * h->KP;
    hd.dpre = h->dpre[4]; hd.dpre_bs = (long)h->S * h->Fp; hd.ldd = h->Fp;
    hd.part = h->head_part; hd.part_stride = h->head_stride; hd.off_db = h->Fp * h->KP; hd.off_dbf = h->Fp * h->KP + h->KP;
    hd.loss_part = h->loss_part;
    if (h->grouped > 1) { hd.models = h->grouped; hd.model_stride = (long)h->W; }
    hd.labels_ms = h->gs.labels;
    return hd;
}

// a chain launch over nseg segments; every variant but the G backward reads its first A image from the inputs of D3
ChainArgs chain_args(mrgan_handle* h, int variant, int nseg, int block_rows) {
    ChainArgs c;
    memset(&c, 0, sizeof c);
    c.variant = variant; c.block_rows = block_rows;
    c.rows = h->B; c.nseg = nseg; c.seg0 = 0;
    c.seed = h->cfg.seed; c.row0 = (uint32_t)(h->cfg.rank * h->B); c.st = h->state + h->cur; c.gauss = h->gauss;
    c.ablate = h->ablate;
    c.models = h->grouped; c.model_stride = (long)h->W;
    if (variant != CH_V_GBWD) { c.a = (const __bf16*)h->xin[2]; c.a_bs = (long)h->S * h->d[2].Kp; c.lda = h->d[2].Kp; c.a_cols = h->d[2].Kp; }
    return c;
}

// ---------------------------------------------------------------------------------------------------
// discriminator sub-step
// ---------------------------------------------------------------------------------------------------
// D sub-step: the loss head over (labelled, unlabelled, generated) rows.  With the chain this launch also runs D3 .. D5 forward
// before the head and their dX after it (8-class pitch only: at the 32-class pitch D3 .. D5 run per layer and the head alone).  Records how many partial rows of head_part / loss_part it wrote.
int disc_head(mrgan_handle* h, const mrgan_disc_args* a, hipStream_t s) {
    HeadArgs hd = head_args(h, {HEAD_LAB, HEAD_UNL, HEAD_FAKE}, h->B, true);
    hd.labels = a->labels_dev; hd.labels_stream = a->stream_mode;
    hd.inv_count = 1.0f / (float)h->Bg; hd.unl_weight = h->cfg.unlabeled_weight;
    if (h->fp8) {                 // the head writes the e5m2 copies of dpre itself (no bf16 dpre, no quantiser pass)
        hd.dpre = nullptr;
        const Fp8Images& q = h->d[4].q;
        hd.q8 = q.g8; hd.q8_bs = (long)h->S * h->Fp; hd.ldq8 = h->Fp;
        hd.q8t = q.g8t; hd.q8t_bs = h->S; hd.ldq8t = q.ldgt;
        hd.q8_slot = h->slots + q.sg[KIND_D];
    }
    if (h->dtail_chain()) {
        // D3 D4 D5 forward -> loss head -> dX through D5 D4 D3, one launch: the rows of a block never leave its CU
        ChainArgs c = chain_args(h, CH_V_DTAIL, 3, CH_ROWS);
        // the relu masks of D3 .. D5 never leave the launch's registers (their dX products follow in the same launch, and
        // nothing else reads them in a D sub-step): no copies to HBM
        for (int i = 0; i < 3; ++i) { c.fwd[i] = chain_fwd_op(h, 2 + i, false); c.fwd[i].mask = nullptr; }
        c.head = hd;
        for (int i = 0; i < 3; ++i) c.dx[i] = chain_dx_op(h, 4 - i, true);
        h->head_nblk = 3 * ceil_div(h->B, CH_ROWS);
        return run_chain(h, c, chain_flops(h, c, true), s);
    }
    if (h->head_wide && h->grouped <= 1) {       // (head_wide_kernel / w6_split_kernel carry no model index: a group takes head_kernel)
        HeadWideArgs hw;
        memset(&hw, 0, sizeof hw);
        hw.h = hd; hw.mask = h->mask[4]; hw.mask_bs = mask_pitch(h->S, h->ldm[4]); hw.ldm = h->ldm[4];
        hw.w6c = h->w6c; hw.w6r = h->w6r;
        h->head_nblk = 3 * ceil_div(h->B, HEAD_WIDE_ROWS);
        PROF("w6_split_kernel", launch_w6_split(hw, s));
        PROF("head_wide_kernel", launch_head_wide(hw, s));
        return 0;
    }
    h->head_nblk = 3 * ceil_div(h->B, HEAD_ROWS);
    PROF("head_kernel", launch_head(h->bf16, hd, s));
    return 0;
}

// backward of the discriminator stack below dpre[l_top], nseg segments: dX with the bias-gradient column sums down to layer 1,
// then the five weight gradients and the fold of the loss head's fold_rows per-block partial rows (dense_dw_all: bf16 as one
// grouped launch whose tail blocks fold, fp8 one product per layer over the 3 S rows of the images)
int disc_bwd(mrgan_handle* h, int nseg, int l_top, int fold_rows, hipStream_t s) {
    for (int l = l_top; l >= 1; --l)
        CHK(dense_dx(h, h->d[l], KIND_D, h->dpre[l], h->B, nseg, h->dpre[l - 1], ACT_RELU, h->d[l - 1].N, relu_mask(h, l - 1), nullptr,
                     ColSums{CS_SUM, h->cs_db[l - 1], nullptr}, s, Fp8Use{&h->d[l - 1], true, false}));
    DwJob jobs[6];
    for (int l = 0; l < 5; ++l) jobs[l] = DwJob{&h->d[l], h->xin[l], h->dpre[l]};
    if (h->ae) {        // the last layer is a product like the others (features x dY), and no loss head left partials to fold
        jobs[5] = DwJob{&h->d[5], h->feat, h->ae_dy};
        return dense_dw_all(h, KIND_D, jobs, 6, h->B, nseg, s);
    }
    const FoldJob fold = {h->head_part, h->head_red, (long)h->head_stride, fold_rows, h->head_stride, h->head_groups, 0,
                          h->grouped > 1 ? (long)h->W : 0};
    return dense_dw_all(h, KIND_D, jobs, 5, h->B, nseg, s, &fold);
}

int disc_phase(mrgan_handle* h, const mrgan_disc_args* a, int phase, hipStream_t s) {
    if (phase == MRGAN_D_GEN) {
        prof_backlog(h, s);
        StageArgs st;
        memset(&st, 0, sizeof st);
        data_seg(st.s[0], h, a->x_lab_dev, a->idx_lab_dev, a->ld_x_lab, 0, 0, a->stream_mode, h->gs.x_lab, h->gs.idx_lab);
        data_seg(st.s[1], h, a->x_unl_dev, a->idx_unl_dev, a->ld_x_unl, 1, 1, a->stream_mode, h->gs.x_unl, h->gs.idx_unl);
        set_gen_view(h, 0);
        stage_common(st, h, a->z_dev, a->stream_mode, 2, h->pair_gen != 0);
        h->real_staged = 0;
        if (h->pair_gen && h->pair_g) {
            // mrgan_train_pair: the G sub-step's real rows (its x_unl batch, drawn at iteration + 1) ride in this launch too
            const mrgan_gen_args* g = h->pair_g;
            StageSeg& rs = st.s[st.nseg];
            data_seg(rs, h, g->x_unl_dev, g->idx_unl_dev, g->ld_x_unl, 4, 1, g->stream_mode, 0, 0);      // (single handles only)
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
        CHK(disc_fwd_train(h, 0, 3, false, 0, s, h->dtail_chain() ? 2 : 5));
        CHK(disc_head(h, a, s));
        CHK(disc_bwd(h, 3, h->dtail_chain() ? 1 : 4, h->head_nblk, s));
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
// partial rows per segment of the feature-matching column sums as their producer left them: 64-row tiles, or the chain
// launch's row blocks
int fm_parts(const mrgan_handle* h) { return h->use_chain ? ceil_div(h->B, chain_block_rows(h, 2)) : h->tiles_m; }

// D3 D4 D5 forward over (generated, real) rows + the feature-matching column sums, one launch
int gen_chain_fwd(mrgan_handle* h, hipStream_t s) {
    ChainArgs c = chain_args(h, CH_V_GFWD, 2, chain_block_rows(h, 2));
    for (int i = 0; i < 3; ++i) c.fwd[i] = chain_fwd_op(h, 2 + i, i == 2);      // D5: + the feature-matching column sums (one partial row per row block)
    return run_chain(h, c, chain_flops(h, c, false), s);
}

// feature-matching loss and its gradient on the generated rows -> dpre[4]; with the chain, on through D5 D4 D3 -> dpre[1]
int fm_grad(mrgan_handle* h, hipStream_t s) {
    FmArgs f;
    memset(&f, 0, sizeof f);
    if (h->sync_stats) { f.cs = h->r_fm; f.npart_fake = 1; f.npart_real = 1; }
    else { f.cs = h->cs_f; f.npart_fake = f.npart_real = fm_parts(h); }
    f.ldcs = h->Fp; f.count = h->stat_count; f.grad_scale = h->fm_scale; f.feat = h->Fp; f.feat_valid = h->F;
    f.mask = h->mask[4]; f.ldm = h->ldm[4]; f.dpre = h->dpre[4]; f.ldd = h->Fp; f.rows = h->B;
    f.loss_out = h->step_out + 3; f.accum = h->accum + 3;
    f.lscratch = h->fm_scratch; f.lcount = h->fm_count;
    f.models = h->grouped; f.model_stride = (long)h->W;
    if (h->fp8) { f.dpre = nullptr; f.q8 = h->d[4].q.g8; f.ldq8 = h->Fp; f.q8_slot = h->slots + h->d[4].q.sg[KIND_G]; }
    if (!h->use_chain) {
        PROF("fm_kernel", launch_fm(h->bf16, f, s));
        return 0;
    }
    ChainArgs c = chain_args(h, CH_V_GBWD, 1, chain_block_rows(h, 1));
    c.fm = f; c.fm_feat = (const __bf16*)h->feat; c.fm_ldf = h->Fp;
    for (int i = 0; i < 3; ++i) c.dx[i] = chain_dx_op(h, 4 - i, false);
    return run_chain(h, c, chain_flops(h, c, false), s);
}

// dX through the discriminator layers fm_grad left, down to d loss / d(generator output) -> dxfake (noise is additive, so
// this is also d / d(fake x)), with the column sums behind the generator's last bias gradient
int disc_dx_to_input(mrgan_handle* h, hipStream_t s) {
    for (int l = h->use_chain ? 1 : 4; l >= 1; --l)
        CHK(dense_dx(h, h->d[l], KIND_G, h->dpre[l], h->B, 1, h->dpre[l - 1], ACT_RELU, h->d[l - 1].N, relu_mask(h, l - 1), nullptr,
                     NO_SUMS, s, Fp8Use{&h->d[l - 1], false, false}));
    return dense_dx(h, h->d[0], KIND_G, h->dpre[0], h->B, 1, h->dxfake, ACT_LINEAR, h->cfg.d_in, NO_MASK, nullptr,
                    ColSums{CS_SUM, h->cs_db3g, nullptr}, s);
}

int gen_phase(mrgan_handle* h, const mrgan_gen_args* a, int phase, hipStream_t s) {
    const int B = h->B, tm = h->tiles_m, N1p = h->g[0].Np;
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
            data_seg(st.s[0], h, a->x_unl_dev, a->idx_unl_dev, a->ld_x_unl, h->xbase + 1, 1, a->stream_mode, h->gs.x_unl, h->gs.idx_unl);   // real rows
            st.nseg = 1;
            stage_common(st, h, a->z_dev, a->stream_mode, ready ? -1 : 1);
            PROF("stage_kernel", launch_stage(h->bf16, st, s));
        }
        if (!ready) CHK(gen_fwd_head(h, 1, s));
    } else if (phase == MRGAN_G_FEAT) {
        if (!h->gen_ready) CHK(gen_fwd_tail(h, 1, 0, 0, s));                                    // fake rows -> slot 0
        h->gen_ready = 0;
        CHK(disc_fwd_train(h, 1, 2, true, h->xbase, s, h->use_chain ? 2 : 5));
        if (h->use_chain) CHK(gen_chain_fwd(h, s));
        if (h->sync_stats) {
            const int np = fm_parts(h);
            PROF("colsum_finalize_kernel", launch_colsum_finalize(h->cs_f, h->cs_f + (size_t)np * h->Fp, np, h->Fp, h->Fp, h->r_fm, s));
        }
    } else if (phase == MRGAN_G_BWD) {
        CHK(fm_grad(h, s));
        CHK(disc_dx_to_input(h, s));
        CHK(dense_dx(h, h->g[2], KIND_G, h->dxfake, B, 1, h->dpre2g, ACT_SOFTPLUS, h->g[1].N, NO_MASK, h->h2,
                     ColSums{CS_SUM, h->cs_db2g, nullptr}, s));
        // d(BN out) = dpre2 W2^T with the BatchNorm backward sums; fp8: dpre2 (bf16, from the G3 dX product) -> e5m2 (+ transpose)
        CHK(dense_dx(h, h->g[1], KIND_G, h->dpre2g, B, 1, h->dhbn, ACT_LINEAR, h->g[0].N, NO_MASK, h->h1,
                     ColSums{CS_SUM_XHAT, h->cs_dbeta, h->cs_dgamma}, s, Fp8Use{nullptr, true, true}));
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
        b.models = h->grouped; b.model_stride = (long)h->W;
        PROF("bn_bwd_kernel", launch_bn_bwd(h->bf16, b, s));
        // the generator's weight gradients; in fp8 the wide one (G2) is a product of its own, after the grouped launch
        const DwJob jobs[3] = {{&h->g[2], h->h2, h->dxfake}, {&h->g[0], h->zbuf, h->dpre1g}, {&h->g[1], h->hbn, h->dpre2g}};
        CHK(dense_dw_all(h, KIND_G, jobs, 3, B, 1, s));
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
    data_seg(st.s[0], h, a->x_dev, a->idx_dev, a->ld_x, 0, 0, a->stream_mode, h->gs.x_lab, h->gs.idx_lab);
    st.nseg = 1;
    stage_common(st, h, nullptr, 0, -1);
    PROF("stage_kernel", launch_stage(h->bf16, st, s));
    CHK(disc_fwd_train(h, 0, 1, false, 0, s, 5));
    HeadArgs hd = head_args(h, {HEAD_MSE}, B, true);
    hd.labels = a->labels_dev; hd.labels_stream = a->stream_mode;
    hd.inv_count = 1.0f / (float)(a->rows_valid > 0 ? a->rows_valid : B); hd.unl_weight = 0.f;
    PROF("head_kernel", launch_head(h->bf16, hd, s));
    // the metrics pass of the Adam launch sums the partial rows of a three-segment step; those of the two other segments
    // keep the zeros of mrgan_create
    h->head_nblk = 3 * ceil_div(B, HEAD_ROWS);
    CHK(disc_bwd(h, 1, 4, ceil_div(B, HEAD_ROWS), s));
    CHK(run_adam(h, MRGAN_NET_D, ADAM_FUSED, true, s, a->stream_mode ? 1 : 0));
    h->cur ^= 1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// autoencoder step (others/mr_gan_autoencoder.py:109-127): the supervised step's stack with a full-width last layer whose
// target is the input row itself -- stage, dense 1..5 (relu, masks), dense 6 (linear) -> y, the reconstruction head -> dY, its
// column sums and the loss partials, dX through dense 6 (relu mask of dense 5) and on down, six weight gradients, fused Adam
// ---------------------------------------------------------------------------------------------------
ReconHeadArgs recon_head_args(mrgan_handle* h, const float* x, const int32_t* idx, long ld, int rows, int rows_valid) {
    ReconHeadArgs r;
    memset(&r, 0, sizeof r);
    r.y = h->ae_y; r.ldy = h->Dp;
    r.x = x; r.idx = idx; r.ld_x = ld;
    r.st = h->state + h->cur; r.batch_rows = h->B;
    r.rows = rows; r.rows_valid = rows_valid; r.cols = h->cfg.d_in; r.cols_pad = h->Dp;
    r.loss_part = h->ae_loss_part;
    return r;
}
int ae_step(mrgan_handle* h, const mrgan_ae_args* a, hipStream_t s) {
    const int B = h->B, rows_valid = a->rows_valid > 0 ? a->rows_valid : B;
    prof_backlog(h, s);
    StageArgs st;
    memset(&st, 0, sizeof st);
    data_seg(st.s[0], h, a->x_dev, a->idx_dev, a->ld_x, 0, 0, a->stream_mode, 0, 0);
    st.nseg = 1;
    stage_common(st, h, nullptr, 0, -1);
    PROF("stage_kernel", launch_stage(h->bf16, st, s));
    CHK(disc_fwd_train(h, KIND_D, 1, false, 0, s, 5));
    const Dense& L6 = h->d[5];
    CHK(dense_fwd(h, L6, KIND_D, h->feat, B, 1, h->ae_y, ACT_LINEAR, NO_NOISE, NO_MASK, NO_SUMS, s));
    // dY over whole 64-row blocks: rows >= rows_valid are zeros there, and the rows behind them keep the zeros of mrgan_create
    ReconHeadArgs r = recon_head_args(h, a->x_dev, a->idx_dev, a->ld_x, h->tiles_m * 64, rows_valid);
    r.stream = a->stream_mode;
    r.scale = 2.0f / ((float)rows_valid * (float)h->cfg.d_in);
    r.dy = h->ae_dy; r.ldd = h->Dp; r.cs = h->ae_cs; r.ldcs = h->Dp;
    PROFB("recon_head_kernel", launch_recon_head(h->bf16, r, s), (double)rows_valid * h->cfg.d_in * (4.0 + 2.0 * h->es));
    CHK(dense_dx(h, L6, KIND_D, h->ae_dy, B, 1, h->dpre[4], ACT_RELU, h->d[4].N, relu_mask(h, 4), nullptr,
                 ColSums{CS_SUM, h->cs_db[4], nullptr}, s));
    CHK(disc_bwd(h, 1, 4, 0, s));
    CHK(run_adam(h, MRGAN_NET_D, ADAM_FUSED, true, s, a->stream_mode ? 1 : 0, h->ae_loss_part, h->tiles_m * (h->Dp / 64),
                 1.0f / ((float)rows_valid * (float)h->cfg.d_in)));
    h->cur ^= 1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// what the step entries ask of their arguments
// ---------------------------------------------------------------------------------------------------
// an autoencoder handle (MRGAN_FLAG_AUTOENCODER) serves mrgan_ae_step / mrgan_ae_encode / mrgan_ae_reconstruct and no other
// step, evaluation or saliency entry; every other handle refuses those three (status -3)
int refuse_ae(const mrgan_handle* h, const char* entry) {
    if (!h->ae) return 0;
    return fail(-3, "%s: not on an autoencoder handle (MRGAN_FLAG_AUTOENCODER): its last layer is no class layer; it trains through mrgan_ae_step and is read through mrgan_ae_encode / mrgan_ae_reconstruct", entry);
}
int require_ae(const mrgan_handle* h, const char* entry) {
    if (h->ae) return 0;
    return fail(-3, "%s: not an autoencoder handle (create it with MRGAN_FLAG_AUTOENCODER)", entry);
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
// entry: "sup_step" or "sup_step_group" (a group handle is never data-parallel or fp8: mrgan_create refuses those)
int check_sup_args(const mrgan_handle* h, const mrgan_sup_args& a, const char* entry) {
    if (a.ld_x < h->cfg.d_in) return fail(-2, "%s: row pitch smaller than d_in", entry);
    if (h->flat_grads || h->cfg.world != 1) return fail(-3, "%s: single-GPU handles only", entry);
    if (h->fp8) return fail(-3, "%s: the fp8 mode covers the GAN step only", entry);
    if (a.rows_valid < 0 || a.rows_valid > h->B) return fail(-2, "%s: rows_valid outside [0, batch]", entry);
    if (a.rows_valid && a.stream_mode) return fail(-2, "%s: a short batch cannot be combined with stream mode", entry);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// the steps of a group handle: sup_step / disc_phase / gen_phase with every launch covering all models
// ---------------------------------------------------------------------------------------------------
// For the scope of one grouped step the handle describes all models: h->grouped (every argument builder adds the model
// count and the stride W) and h->gs (the strides of the caller's inputs).  Every return path leaves the handle single.
// Each launch is then the single handle's launch with the model as a further grid index: model m stages its own rows, draws
// its noise with seed + m and updates its own copy of the weights; the iteration counter is shared.
// (pair_gen / pair_g: a group never shares a generator pass.  Only disc_phase / gen_phase read them, so clearing them is
// nothing to the supervised step, and a hint left by mrgan_pair_hint was cleared by the next grouped D sub-step anyway.)
struct GroupScope {
    mrgan_handle* h;
    GroupScope(mrgan_handle* h_, const mrgan_handle::GroupStrides& gs) : h(h_) { h->grouped = h->models; h->gs = gs; h->pair_gen = 0; h->pair_g = nullptr; }
    ~GroupScope() { h->grouped = 1; memset(&h->gs, 0, sizeof h->gs); }
};
mrgan_disc_args single_args(const mrgan_disc_group_args* a) {
    mrgan_disc_args d;
    memset(&d, 0, sizeof d);
    d.x_lab_dev = a->x_lab_dev; d.idx_lab_dev = a->idx_lab_dev; d.labels_dev = a->labels_dev;
    d.x_unl_dev = a->x_unl_dev; d.idx_unl_dev = a->idx_unl_dev; d.z_dev = a->z_dev;
    d.ld_x_lab = a->ld_x_lab; d.ld_x_unl = a->ld_x_unl; d.stream_mode = a->stream_mode;
    return d;
}
mrgan_gen_args single_args(const mrgan_gen_group_args* a) {
    mrgan_gen_args g;
    memset(&g, 0, sizeof g);
    g.x_unl_dev = a->x_unl_dev; g.idx_unl_dev = a->idx_unl_dev; g.z_dev = a->z_dev; g.ld_x_unl = a->ld_x_unl; g.stream_mode = a->stream_mode;
    return g;
}
mrgan_sup_args single_args(const mrgan_sup_group_args* a) {
    mrgan_sup_args u;
    memset(&u, 0, sizeof u);
    u.x_dev = a->x_dev; u.idx_dev = a->idx_dev; u.labels_dev = a->labels_dev; u.ld_x = a->ld_x;
    u.stream_mode = a->stream_mode; u.rows_valid = a->rows_valid;
    return u;
}
int sup_step_group(mrgan_handle* h, const mrgan_sup_group_args* a, hipStream_t s) {
    // (the one data segment and the labels of the supervised step travel in the labelled slots)
    GroupScope scope(h, {(long)a->x_model_stride, (long)a->idx_model_stride, (long)a->labels_model_stride, 0, 0, 0});
    const mrgan_sup_args u = single_args(a);
    return sup_step(h, &u, s);
}
int disc_step_group(mrgan_handle* h, const mrgan_disc_group_args* a, hipStream_t s) {
    GroupScope scope(h, {(long)a->x_lab_model_stride, (long)a->idx_lab_model_stride, (long)a->labels_model_stride,
                         (long)a->x_unl_model_stride, (long)a->idx_unl_model_stride, (long)a->z_model_stride});
    const mrgan_disc_args d = single_args(a);
    for (int p = 0; p < MRGAN_D_NPHASES; ++p) { const int r = disc_phase(h, &d, p, s); if (r) return r; }
    return 0;
}
int gen_step_group(mrgan_handle* h, const mrgan_gen_group_args* a, hipStream_t s) {
    GroupScope scope(h, {0, 0, 0, (long)a->x_unl_model_stride, (long)a->idx_unl_model_stride, (long)a->z_model_stride});
    const mrgan_gen_args g = single_args(a);
    h->gen_ready = 0;                                  // (a group's G sub-step always runs its own generator forward)
    for (int p = 0; p < MRGAN_G_NPHASES; ++p) { const int r = gen_phase(h, &g, p, s); if (r) return r; }
    return 0;
}
int check_group_handle(const mrgan_handle* h, const char* entry) {
    if (h->models > 1) return 0;
    return fail(-3, "%s: not a group handle (mrgan_config.models = %d); a single model steps through mrgan_disc_step / mrgan_gen_step / mrgan_train_pair",
                entry, (int)h->cfg.models);
}
int check_disc_group_args(const mrgan_handle* h, const mrgan_disc_group_args* a) {
    if (!a) return fail(-2, "disc_step_group: null arguments");
    const mrgan_disc_args d = single_args(a);
    const int r = check_disc_args(h, &d);
    if (r) return r;
    if (a->x_lab_model_stride < 0 || a->idx_lab_model_stride < 0 || a->labels_model_stride < 0 || a->x_unl_model_stride < 0 ||
        a->idx_unl_model_stride < 0 || a->z_model_stride < 0)
        return fail(-2, "disc_step_group: negative model stride");
    return 0;
}
int check_gen_group_args(const mrgan_handle* h, const mrgan_gen_group_args* a) {
    if (!a) return fail(-2, "gen_step_group: null arguments");
    const mrgan_gen_args g = single_args(a);
    const int r = check_gen_args(h, &g);
    if (r) return r;
    if (a->x_unl_model_stride < 0 || a->idx_unl_model_stride < 0 || a->z_model_stride < 0) return fail(-2, "gen_step_group: negative model stride");
    return 0;
}

// One (D sub-step, G sub-step) pair, `both`, launched eagerly or -- want_graph -- as the replay of a captured graph.
// A pair flips the state slot twice, so every kernel argument is identical on every replay as long as the slot parity and the
// caller's argument blocks (dargs / gargs: the single or the group ones, compared byte by byte) are those of the capture.
template <typename Both>
int run_pair(mrgan_handle* h, bool want_graph, const void* dargs, size_t dn, const void* gargs, size_t gn, hipStream_t s, Both both) {
    if (!want_graph) return both();
    if (dn + gn > sizeof h->graph_key) return fail(-1, "run_pair: argument blocks larger than the graph key");
    if (h->graph_ready && (h->graph_cur != h->cur || h->graph_key_d != dn || h->graph_key_g != gn || memcmp(h->graph_key, dargs, dn) != 0 ||
                           memcmp(h->graph_key + dn, gargs, gn) != 0)) {
        hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr; h->graph_ready = false;
    }
    if (!h->graph_ready) {
        hipGraph_t graph;
        const int cur0 = h->cur;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int r = both();
        graph = nullptr;
        hipError_t e = hipStreamEndCapture(s, &graph);
        if (r) { if (graph) hipGraphDestroy(graph); return r; }       // a launch failed during capture: drop the partial graph
        if (e != hipSuccess) return fail(-10, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (e != hipSuccess) return fail(-10, "hipGraphInstantiate: %s", hipGetErrorString(e));
        memcpy(h->graph_key, dargs, dn); memcpy(h->graph_key + dn, gargs, gn);
        h->graph_key_d = dn; h->graph_key_g = gn; h->graph_cur = cur0; h->graph_ready = true;
    }
    HIPCHK(hipGraphLaunch(h->graph_exec, s));
    return 0;
}

// what a group handle does not do (status -3)
int refuse_group(const mrgan_handle* h, const char* entry) {
    if (h->models <= 1) return 0;
    return fail(-3, "%s: a group handle (models = %d) trains through the _group entries (mrgan_sup_step_group, mrgan_disc_step_group, mrgan_gen_step_group, mrgan_train_pair_group)", entry, h->models);
}

// ---------------------------------------------------------------------------------------------------
// evaluation and saliency: forward-only passes (learning phase 0) that use the training activations as scratch
// ---------------------------------------------------------------------------------------------------
ReluMask eval_mask(const mrgan_handle* h, int l) { return ReluMask{selected(h, h->mask[l]), h->ldm[l]}; }

// what makes an evaluation forward draw d of mrgan_attribution.  MRGAN_ATTR_NOISE: the stage and the epilogues of dense 1 .. 4
// add the site's noise (sigma_in at site 0, sigma_hid at sites 1 .. 4) under `key`, segment id MRGAN_ATTR_NOISE_SEG;
// MRGAN_ATTR_PATH (path): the noise-free forward at the point alpha of the way from the baseline (null: zeros) to the row
struct Draw { DrawKey key; float sigma_in, sigma_hid; bool path; float alpha; const float* baseline; };

// One chunk: `rows` rows from r0 of the caller's matrix (gathered through idx when given) -> xin[0], then dense 1..5 -> feat,
// as one run of contiguous rows from row 0 (nb = 1: the batch stride is irrelevant).  keep_masks: the relu masks are
// written for a dX chain that follows.  draw: null for the noise-free forward at the rows themselves (no state slot beside the
// current one, the plain stage instantiation).  A group handle evaluates the selected model: its activations here, its weights
// in dense_fwd.
int eval_forward(mrgan_handle* h, const float* x, const int32_t* idx, long ld, long r0, int rows, bool keep_masks, hipStream_t s,
                 const Draw* draw = nullptr, int l_end = 5 /* dense 1 .. l_end only (mrgan_ae_encode) */) {
    const float* src = idx ? x : x + r0 * ld;
    const int32_t* ridx = idx ? idx + r0 : nullptr;
    if (draw && draw->path) {
        PathStageArgs ps;
        memset(&ps, 0, sizeof ps);
        ps.src = src; ps.idx = ridx; ps.ld = ld; ps.baseline = draw->baseline; ps.alpha = draw->alpha;
        ps.rows = rows; ps.cols = h->cfg.d_in; ps.cols_pad = h->Dp; ps.out = selected(h, h->xin[0]); ps.ldo = h->Dp;
        PROFB("path_stage_kernel", launch_path_stage(h->bf16, ps, s), (double)rows * h->cfg.d_in * (4.0 + h->es));
    } else {
        StageArgs st;
        memset(&st, 0, sizeof st);
        StageSeg& sg = st.s[0];
        sg.src = src; sg.idx = ridx; sg.ld = ld; sg.rows = rows;
        sg.cols = h->cfg.d_in; sg.cols_pad = h->Dp; sg.out = selected(h, h->xin[0]); sg.ldo = h->Dp;
        st.nseg = 1; st.seed = h->cfg.seed; st.cur = h->state + h->cur;
        if (draw) {
            sg.sigma = draw->sigma_in; sg.site = 0; sg.seg = MRGAN_ATTR_NOISE_SEG;
            st.seed = draw->key.seed; st.row0 = draw->key.row0; st.cur = draw->key.st;
            st.gauss = draw->sigma_in > 0.f ? h->gauss : 0;      // (sigma 0: the instantiation of the noise-free forward)
        }
        PROF("stage_kernel", launch_stage(h->bf16, st, s));
    }
    for (int l = 0; l < l_end; ++l) {
        const bool noisy = draw && l < 4 && draw->sigma_hid > 0.f;
        const NoiseSite nz = {noisy ? draw->sigma_hid : 0.f, (uint32_t)(l + 1), (uint32_t)MRGAN_ATTR_NOISE_SEG, 1, 0};
        CHK(dense_fwd(h, h->d[l], KIND_EVAL, selected(h, h->xin[l]), rows, 1, selected(h, l < 4 ? h->xin[l + 1] : h->feat), ACT_RELU,
                      noisy ? nz : NO_NOISE, keep_masks ? eval_mask(h, l) : NO_MASK, NO_SUMS, s, NO_FP8, noisy ? &draw->key : nullptr));
    }
    return 0;
}

// the head of such a chunk on the selected model: `kind` over `rows` rows of feat with `labels` (null where the kind takes
// none).  HEAD_EVAL / HEAD_LOGITS keep the logits; the saliency kinds (want_dpre) write the per-row dpre[4] instead -- at
// labels, or null: at the row's argmax -- and report the class each row used to classes_out where given
HeadArgs eval_head(mrgan_handle* h, int kind, const int32_t* labels, int32_t* classes_out, bool want_dpre, int rows) {
    HeadArgs hd = head_args(h, {kind}, rows, false);
    hd.f = selected(h, hd.f); hd.w = selected(h, hd.w); hd.b = selected(h, hd.b);
    hd.logits = want_dpre ? nullptr : selected(h, hd.logits);
    hd.labels = labels; hd.classes_out = classes_out;
    if (want_dpre) { hd.dpre = selected(h, h->dpre[4]); hd.ldd = h->Fp; }
    return hd;
}

// The chunks above fill rows from row 0 of every layer input, i.e. also the padding rows B .. S of the training segments they
// reach.  The bf16 weight gradients reduce over all S rows of a segment, zero dY padding rows x FINITE X padding rows (dw_args):
// a non-finite value left there by an evaluation input would turn into NaN gradients from then on (0 * NaN), and a nonzero dY
// would add to them.  Ragged batches only: re-zero the padding rows of the first nseg_x0 segments of xin[0] and the first nseg
// of xin[1..4]; grads: also those of segment 0 of the dY tensors a dX chain wrote, dpre[l] and dxfake (the dY of the generator's
// last layer).  (feat and the masks: every training forward rewrites what its sub-step reads, and the padding rows of feat meet
// zero dlogits only.)
int rezero_padding(mrgan_handle* h, int nseg_x0, int nseg, bool grads, hipStream_t s) {
    if (h->B >= h->S) return 0;
    const size_t pad = (size_t)(h->S - h->B);
    auto clear = [&](void* t, int seg, int ld) {
        return hipMemsetAsync((char*)selected(h, t) + ((size_t)seg * h->S + h->B) * ld * h->es, 0, pad * ld * h->es, s);
    };
    for (int l = 0; l < 5; ++l) {
        for (int seg = 0; seg < (l == 0 ? nseg_x0 : nseg); ++seg) HIPCHK(clear(h->xin[l], seg, h->d[l].Kp));
        if (grads) HIPCHK(clear(h->dpre[l], 0, h->d[l].Np));
    }
    if (grads) HIPCHK(clear(h->dxfake, 0, h->Dp));
    return 0;
}

// forward-only discriminator over n rows (learning phase 0), chunked through the training activations
int eval_rows(mrgan_handle* h, const float* x, const int32_t* idx, long ld, const int32_t* labels, long n, float* logits_out,
              hipStream_t s) {
    const long cap = 3L * h->S;
    for (long r0 = 0; r0 < n; r0 += cap) {
        const int rows = (int)std::min(cap, n - r0);
        const int r = eval_forward(h, x, idx, ld, r0, rows, false, s);
        if (r) return r;
        HeadArgs hd = eval_head(h, labels ? HEAD_EVAL : HEAD_LOGITS, labels ? labels + r0 : nullptr, nullptr, false, rows);
        hd.err_count = labels ? h->err_count : nullptr;
        PROF("head_kernel", launch_head(h->bf16, hd, s));
        if (logits_out)
            HIPCHK(hipMemcpy2DAsync(logits_out + r0 * h->cfg.num_classes, sizeof(float) * h->cfg.num_classes, selected(h, h->logits),
                                    sizeof(float) * h->KP, sizeof(float) * h->cfg.num_classes, rows, hipMemcpyDeviceToDevice, s));
    }
    return rezero_padding(h, 5, 3, false, s);      // the chunks reach rows [0, 3S); xin[0]: all five segments, whatever n
}

// The read-only entries of an autoencoder handle, chunked like eval_rows.  through = 3: the code, the stored relu output of
// dense 3 (the input of dense 4) -> out; through = 6: the whole forward, y -> out where given, and where mse is wanted the
// reconstruction head without its dY over the chunk, its partials folded into ae_mse chunk after chunk.  The chunks reach what
// eval_rows' reach, and the features: their padding rows are the X operand of the last weight gradient (dw_args).
int ae_rows(mrgan_handle* h, const float* x, const int32_t* idx, long ld, long n, int through, float* out, long ld_out, bool mse,
            hipStream_t s) {
    const long cap = 3L * h->S;
    for (long r0 = 0; r0 < n; r0 += cap) {
        const int rows = (int)std::min(cap, n - r0);
        const int r = eval_forward(h, x, idx, ld, r0, rows, false, s, nullptr, through == 3 ? 3 : 5);
        if (r) return r;
        if (through == 3) {
            PROFB("cast_rows_kernel", launch_cast_rows(h->bf16, h->xin[3], h->d[3].Kp, rows, h->d[3].K, out + r0 * ld_out, ld_out, s),
                  (double)rows * h->d[3].K * (4.0 + h->es));
            continue;
        }
        CHK(dense_fwd(h, h->d[5], KIND_EVAL, h->feat, rows, 1, h->ae_y, ACT_LINEAR, NO_NOISE, NO_MASK, NO_SUMS, s));
        if (out)
            PROFB("cast_rows_kernel", launch_cast_rows(h->bf16, h->ae_y, h->Dp, rows, h->cfg.d_in, out + r0 * ld_out, ld_out, s),
                  (double)rows * h->cfg.d_in * (4.0 + h->es));
        if (mse) {
            const ReconHeadArgs rh = recon_head_args(h, idx ? x : x + r0 * ld, idx ? idx + r0 : nullptr, ld, rows, rows);
            PROFB("recon_head_kernel", launch_recon_head(h->bf16, rh, s), (double)rows * h->cfg.d_in * (4.0 + h->es));
            PROF("fold_loss_kernel", launch_fold_loss(h->ae_loss_part, ceil_div(rows, 64) * (h->Dp / 64), h->ae_mse, r0 == 0 ? 1 : 0, s));
        }
    }
    CHK(rezero_padding(h, 5, 3, false, s));
    if (h->B < h->S) HIPCHK(hipMemsetAsync((char*)h->feat + (size_t)h->B * h->Fp * h->es, 0, (size_t)(h->S - h->B) * h->Fp * h->es, s));
    return 0;
}
int check_ae_rows(const mrgan_handle* h, const char* entry, const float* x, int64_t ld, int64_t n) {
    if (!x) return fail(-2, "%s: x is required", entry);
    if (n < 1) return fail(-2, "%s: row count n must be positive", entry);
    if (ld < h->cfg.d_in) return fail(-2, "%s: row pitch ld_x smaller than d_in", entry);
    return 0;
}

// the backward half of a chunk: the per-row saliency head of `objective` (targets, or null: the row's argmax; classes_out optional)
// into dpre[4], the masked dX chain down to layer 1 and the linear layer-0 dX into dxfake
int saliency_backward(mrgan_handle* h, int objective, const int32_t* targets, int32_t* classes_out, int rows, hipStream_t s) {
    static const int kinds[3] = {HEAD_SAL_LOGIT, HEAD_SAL_XENT, HEAD_SAL_MSE};
    PROF("head_kernel", launch_head(h->bf16, eval_head(h, kinds[objective], targets, classes_out, true, rows), s));
    for (int l = 4; l >= 1; --l)
        CHK(dense_dx(h, h->d[l], KIND_EVAL, selected(h, h->dpre[l]), rows, 1, selected(h, h->dpre[l - 1]), ACT_RELU, h->d[l - 1].N, eval_mask(h, l - 1),
                     nullptr, NO_SUMS, s));
    CHK(dense_dx(h, h->d[0], KIND_EVAL, selected(h, h->dpre[0]), rows, 1, selected(h, h->dxfake), ACT_LINEAR, h->cfg.d_in, NO_MASK, nullptr,
                 NO_SUMS, s));
    return 0;
}
// Saliency maps of n rows (mrgan_attribution; mrgan_input_gradient is its call of one noise-free draw).  Per chunk of at most
// S rows: the target classes (given, or one clean forward + head when the draws themselves are not that forward), then per
// draw d the evaluation forward WITH its relu masks -- at the rows themselves, or (Draw) with the noise keyed by slot d of
// draw_state (step d), seed + selected model and the chunk's first row, or at the path point alpha_d -- the per-row saliency
// head into dpre[4], the masked dX chain down to layer 1, the linear layer-0 dX into dxfake and the accumulate launch into the
// caller's rows.  Everything lives in segment 0 of the training activations (xin[l], mask[l], dpre[l], feat) as one run of
// contiguous rows; dxfake holds S rows, which is what bounds the chunk.  No column sums, no weight gradients: cur, the
// counters and the cached graph are not touched.  Draws are the inner loop: a chunk's out rows stay in L2.
int attribution_rows(mrgan_handle* h, const mrgan_attribution_args* a, hipStream_t s) {
    const long cap = h->S, n = a->n;
    const bool path = a->method == MRGAN_ATTR_PATH;
    const bool noise_free = !path && a->sigma_input == 0.f && a->sigma_hidden == 0.f;      // every draw is the clean forward at x
    const bool clean_pass = !a->targets_dev && !noise_free;      // (noise-free: the draw's own head finds the predicted class)
    for (long r0 = 0; r0 < n; r0 += cap) {
        const int rows = (int)std::min(cap, n - r0);
        int32_t* classes = a->classes_out_dev ? a->classes_out_dev + r0 : nullptr;
        const int32_t* targets = a->targets_dev ? a->targets_dev + r0 : nullptr;
        if (clean_pass) {
            const int r = eval_forward(h, a->x_dev, a->idx_dev, a->ld_x, r0, rows, false, s);
            if (r) return r;
            // (for its argmax: dpre[4] is rewritten by every draw)
            PROF("head_kernel", launch_head(h->bf16, eval_head(h, HEAD_SAL_LOGIT, nullptr, classes, true, rows), s));
            targets = classes;
        }
        for (int d = 0; d < a->draws; ++d) {
            const Draw draw = {{h->draw_state + d, h->cfg.seed + (uint64_t)h->sel, (uint32_t)r0}, a->sigma_input, a->sigma_hidden, path,
                               ((float)d + 0.5f) / (float)a->draws, a->baseline_dev};
            const int r = eval_forward(h, a->x_dev, a->idx_dev, a->ld_x, r0, rows, true, s, noise_free ? nullptr : &draw);
            if (r) return r;
            // draw 0 reports the classes unless the clean pass has; without targets (the noise-free call) its head finds them, and
            // the later draws read them back
            CHK(saliency_backward(h, a->objective, targets, (d == 0 && targets != classes) ? classes : nullptr, rows, s));
            if (!targets) targets = classes;
            AttrAccumArgs f;
            memset(&f, 0, sizeof f);
            f.g = selected(h, h->dxfake); f.ldg = h->Dp; f.rows = rows; f.cols = h->cfg.d_in;
            f.out = a->out_dev + r0 * a->ld_out; f.ldo = a->ld_out; f.mode = a->post == MRGAN_SAL_HEATMAP ? SAL_HEATMAP : SAL_RAW;
            f.draw = d; f.draws = a->draws; f.multiply = a->multiply;
            f.x = a->idx_dev ? a->x_dev : a->x_dev + r0 * a->ld_x; f.idx = a->idx_dev ? a->idx_dev + r0 : nullptr; f.ld_x = a->ld_x;
            f.baseline = a->baseline_dev;
            PROFB("attribution_accum_kernel", launch_attr_accum(h->bf16, f, s),
                  (double)rows * h->cfg.d_in * (h->es + (d > 0 ? 8.0 : 4.0) + (a->multiply && d == a->draws - 1 ? 4.0 : 0.0)));
        }
    }
    return n > h->B ? rezero_padding(h, 1, 1, true, s) : 0;      // (no chunk reached the padding rows of segment 0 otherwise)
}

// what mrgan_input_gradient and mrgan_attribution refuse alike, under the entry's name (a: null, or the call as an attribution)
int check_attribution(const mrgan_handle* h, const char* entry, const mrgan_attribution_args* a) {
    if (!h) return fail(-1, "null handle");
    if (refuse_ae(h, entry)) return -3;
    if (h->fp8) return fail(-3, "%s: not on an fp8 handle (its dX products read fp8-scaled images and would disturb the calibration); use an fp32 or a bf16 engine", entry);
    if (!a || !a->x_dev || !a->out_dev) return fail(-2, "%s: x and out are required", entry);
    if (a->n < 0) return fail(-2, "%s: negative row count n", entry);
    if (a->ld_x < h->cfg.d_in) return fail(-2, "%s: row pitch ld_x smaller than d_in", entry);
    if (a->ld_out < h->cfg.d_in) return fail(-2, "%s: row pitch ld_out smaller than d_in", entry);
    if (a->objective != MRGAN_SAL_LOGIT && a->objective != MRGAN_SAL_XENT && a->objective != MRGAN_SAL_MSE)
        return fail(-2, "%s: unknown objective %d", entry, (int)a->objective);
    if (a->post != MRGAN_SAL_RAW && a->post != MRGAN_SAL_HEATMAP) return fail(-2, "%s: unknown post mode %d", entry, (int)a->post);
    if (a->method != MRGAN_ATTR_NOISE && a->method != MRGAN_ATTR_PATH) return fail(-2, "%s: unknown method %d", entry, (int)a->method);
    if (a->draws < 1 || a->draws > MRGAN_ATTR_MAX_DRAWS)
        return fail(-2, "%s: draws = %d outside [1, %d]", entry, (int)a->draws, (int)MRGAN_ATTR_MAX_DRAWS);
    if (a->multiply != 0 && a->multiply != 1) return fail(-2, "%s: multiply must be 0 or 1, got %d", entry, (int)a->multiply);
    if (!(a->sigma_input >= 0.f) || !std::isfinite(a->sigma_input)) return fail(-2, "%s: sigma_input must be finite and >= 0", entry);
    if (!(a->sigma_hidden >= 0.f) || !std::isfinite(a->sigma_hidden)) return fail(-2, "%s: sigma_hidden must be finite and >= 0", entry);
    if (a->method == MRGAN_ATTR_PATH && (a->sigma_input != 0.f || a->sigma_hidden != 0.f))
        return fail(-2, "%s: sigma_input / sigma_hidden belong to MRGAN_ATTR_NOISE; MRGAN_ATTR_PATH is noise-free", entry);
    if (a->method == MRGAN_ATTR_NOISE && a->baseline_dev) return fail(-2, "%s: baseline_dev belongs to MRGAN_ATTR_PATH", entry);
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
// The first whole sub-step of `kind` on an fp8 handle (phases p0 .. p1 of nphases, starting at 0) calibrates by itself: dry
// passes over the phases 0 .. dry_last of `phase` (disc_phase / gen_phase; each kind has its own slots: the feature-matching
// gradient has another scale than the D loss's).
template <typename Args>
int fp8_calibrate(mrgan_handle* h, int kind, int p0, int p1, int nphases, int dry_last, int (*phase)(mrgan_handle*, const Args*, int, hipStream_t),
                  const Args* a, hipStream_t s) {
    if (!h->fp8 || p0 != 0 || h->fp8_cal[kind]) return 0;
    if (p1 < nphases - 1 && h->sync_stats)
        return fail(-3, "fp8 with synchronised statistics: a phase-wise host runs the calibration passes itself (mrgan_fp8_calibration)");
    CHK(fp8_cal_begin(h, kind, s));
    for (int i = 0; i < FP8_DRY_PASSES; ++i) {
        for (int p = 0; p <= dry_last; ++p) { const int r = phase(h, a, p, s); if (r) return r; }
        CHK(fp8_cal_end_pass(h, kind, s));
    }
    CHK(fp8_cal_done(h, kind, s));
    return 0;
}

// `count` floats from `offset` of the step_out of each of the first `models` models -> out [models][count], and wait for them
int read_step_out(mrgan_handle* h, int models, int offset, int count, float* out, hipStream_t s) {
    for (int m = 0; m < models; ++m)
        HIPCHK(hipMemcpyAsync(out + (size_t)m * count, model_at(h, h->step_out, m) + offset, count * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
// the supervised step's outputs of `models` models -> out2 [models][2] = loss, training error.  The metrics pass divides by
// the batch: a short batch (rows_valid) is rescaled here.
int read_sup_out(mrgan_handle* h, int models, int rows_valid, float* out2, hipStream_t s) {
    float o[MRGAN_MAX_MODELS][3];
    const int r = read_step_out(h, models, 0, 3, &o[0][0], s);
    if (r) return r;
    const float k = rows_valid > 0 ? (float)h->B / (float)rows_valid : 1.f;
    for (int m = 0; m < models; ++m) { out2[2 * m] = o[m][0] * k; out2[2 * m + 1] = o[m][2] * k; }
    return 0;
}

}  // namespace

extern "C" {

int mrgan_disc_step(mrgan_handle* h, const mrgan_disc_args* a, int p0, int p1, float* out3, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "disc_step");
    if (!r) r = refuse_group(h, "disc_step");
    if (!r) r = check_disc_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    if (p1 < 0) p1 = MRGAN_D_NPHASES - 1;
    r = fp8_calibrate(h, 0, p0, p1, MRGAN_D_NPHASES, MRGAN_D_MAIN, disc_phase, a, s);
    if (r) return r;
    for (int p = p0; p <= p1; ++p) { r = disc_phase(h, a, p, s); if (r) return r; }
    return out3 ? read_step_out(h, 1, 0, 3, out3, s) : 0;
}

int mrgan_gen_step(mrgan_handle* h, const mrgan_gen_args* a, int p0, int p1, float* out1, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "gen_step");
    if (!r) r = refuse_group(h, "gen_step");
    if (!r) r = check_gen_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    if (p1 < 0) p1 = MRGAN_G_NPHASES - 1;
    r = fp8_calibrate(h, 1, p0, p1, MRGAN_G_NPHASES, MRGAN_G_BWD, gen_phase, a, s);
    if (r) return r;
    for (int p = p0; p <= p1; ++p) { r = gen_phase(h, a, p, s); if (r) return r; }
    return out1 ? read_step_out(h, 1, 3, 1, out1, s) : 0;
}

int mrgan_fp8_calibration(mrgan_handle* h, int kind, int action, mrgan_stream stream) {
    if (!h || kind < 0 || kind > 1) return fail(-1, "fp8_calibration: bad handle or kind");
    if (refuse_ae(h, "fp8_calibration") || refuse_group(h, "fp8_calibration")) return -3;
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

int mrgan_svm_gram(const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n, int64_t d, float gamma,
                   float* out_dev, int64_t ld_out, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_gram(a_dev, (long)ld_a, (long)m, b_dev, (long)ld_b, (long)n, (long)d, gamma, out_dev, (long)ld_out, 0,
                                  (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_svm_solve(const float* k_dev, int64_t ld_k, int64_t n, int32_t num_classes, const int64_t* class_start_host, double C,
                    double tol, int32_t max_iter, double* coef_dev, double* rho_dev, int32_t* iters_dev, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_solve(k_dev, (long)ld_k, (long)n, num_classes, class_start_host, C, tol, max_iter, coef_dev, rho_dev,
                                   iters_dev, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_svm_decide(const float* kt_dev, int64_t ld_kt, int64_t m, int64_t n, int32_t num_classes, const int64_t* class_start_host,
                     const double* coef_dev, const double* rho_dev, double* dec_dev, int32_t* labels_dev, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_decide(kt_dev, (long)ld_kt, (long)m, (long)n, num_classes, class_start_host, coef_dev, rho_dev, dec_dev,
                                    labels_dev, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_svm_kernel_matrix(int32_t kernel, const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n,
                            int64_t d, float gamma, float* out_dev, int64_t ld_out, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_kernel_matrix(kernel, a_dev, (long)ld_a, (long)m, b_dev, (long)ld_b, (long)n, (long)d, gamma, out_dev,
                                           (long)ld_out, 0, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_svm_solve_nu(const float* k_dev, int64_t ld_k, int64_t n, int32_t num_classes, const int64_t* class_start_host, double nu,
                       double tol, int32_t max_iter, double* coef_dev, double* rho_dev, double* r_dev, int32_t* iters_dev,
                       mrgan_stream stream) {
    const char* msg = "";
    int bi = -1, bj = -1;
    const int r = launch_svm_solve_nu(k_dev, (long)ld_k, (long)n, num_classes, class_start_host, nu, tol, max_iter, coef_dev, rho_dev,
                                      r_dev, iters_dev, (hipStream_t)stream, &msg, &bi, &bj);
    if (r && bi >= 0) return fail(r, "%s for the pair of classes %d and %d", msg, bi, bj);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_svm_gram_group(const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma, mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_gram_group(items_host, count, (long)d, gamma, 0, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_svm_solve_group(const mrgan_svm_solve_item* items_host, int32_t count, int32_t num_classes, double C, double tol,
                          int32_t max_iter, mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_solve_group(items_host, count, num_classes, C, tol, max_iter, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_svm_decide_group(const mrgan_svm_decide_item* items_host, int32_t count, int32_t num_classes, mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_decide_group(items_host, count, num_classes, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_svm_kernel_matrix_group(int32_t kernel, const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma,
                                  mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_kernel_matrix_group(kernel, items_host, count, (long)d, gamma, 0, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_svm_solve_nu_group(const mrgan_svm_solve_nu_item* items_host, int32_t count, int32_t num_classes, double tol,
                             int32_t max_iter, mrgan_stream stream) {
    const char* msg = "";
    int item = -1, bi = -1, bj = -1;
    const int r = launch_svm_solve_nu_group(items_host, count, num_classes, tol, max_iter, (hipStream_t)stream, &msg, &item, &bi, &bj);
    if (r && bi >= 0) return fail(r, "%s for the pair of classes %d and %d (item %d)", msg, bi, bj, item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_pca_mean(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, float* mean_dev, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_mean(x_dev, (long)ld_x, (long)n, (long)d, mean_dev, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int64_t mrgan_pca_covariance_workspace_bytes(int64_t n, int64_t d) { return pca_covariance_workspace_bytes((long)n, (long)d, 0, 0); }

int mrgan_pca_covariance(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, const float* mean_dev, float* cov_dev, int64_t ld_cov,
                         void* work_dev, int64_t work_bytes, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_covariance(x_dev, (long)ld_x, (long)n, (long)d, mean_dev, cov_dev, (long)ld_cov, work_dev, (long)work_bytes, 0, 0,
                                        (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int64_t mrgan_pca_eig_workspace_bytes(int64_t d, int64_t k) {
    return k < 1 || k > PCA_MAX_COMPONENTS ? -1 : pca_eig_workspace_bytes((long)d, (long)std::min<int64_t>(d, k + PCA_GUARD));
}

int mrgan_pca_eig(const float* cov_dev, int64_t ld_cov, int64_t d, int64_t k, const float* q0_dev, int64_t ld_q0, int64_t p, double tol,
                  int32_t max_iter, void* work_dev, int64_t work_bytes, float* components_dev, int64_t ld_w, double* values_host,
                  double* residuals_host, int32_t* iters_host, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_eig(cov_dev, (long)ld_cov, (long)d, (long)k, q0_dev, (long)ld_q0, (long)p, tol, max_iter, work_dev, (long)work_bytes,
                                 components_dev, (long)ld_w, values_host, residuals_host, iters_host, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_pca_transform(const float* x_dev, int64_t ld_x, int64_t m, int64_t d, const float* mean_dev, const float* components_dev,
                        int64_t ld_w, int64_t k, float* out_dev, int64_t ld_out, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_transform(x_dev, (long)ld_x, (long)m, (long)d, mean_dev, components_dev, (long)ld_w, (long)k, out_dev, (long)ld_out,
                                       (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_pca_inverse_transform(const float* z_dev, int64_t ld_z, int64_t m, int64_t k, const float* components_dev, int64_t ld_w,
                                int64_t d, const float* mean_dev, float* out_dev, int64_t ld_out, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_inverse_transform(z_dev, (long)ld_z, (long)m, (long)k, components_dev, (long)ld_w, (long)d, mean_dev, out_dev,
                                               (long)ld_out, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_sup_step(mrgan_handle* h, const mrgan_sup_args* a, float* out2, mrgan_stream stream) {
    if (!h || !a || !a->x_dev || !a->labels_dev) return fail(-1, "sup_step: x and labels are required");
    if (refuse_ae(h, "sup_step") || refuse_group(h, "sup_step")) return -3;
    int r = check_sup_args(h, *a, "sup_step");
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    r = sup_step(h, a, s);
    if (r) return r;
    return out2 ? read_sup_out(h, 1, a->rows_valid, out2, s) : 0;
}

int mrgan_sup_step_group(mrgan_handle* h, const mrgan_sup_group_args* a, float* out2, mrgan_stream stream) {
    if (!h || !a || !a->x_dev || !a->labels_dev) return fail(-1, "sup_step_group: x and labels are required");
    if (refuse_ae(h, "sup_step_group")) return -3;
    if (h->models <= 1) return fail(-3, "sup_step_group: not a group handle (mrgan_config.models = %d); a single model steps through mrgan_sup_step", (int)h->cfg.models);
    int r = check_sup_args(h, single_args(a), "sup_step_group");
    if (r) return r;
    if (a->x_model_stride < 0 || a->idx_model_stride < 0 || a->labels_model_stride < 0) return fail(-2, "sup_step_group: negative model stride");
    hipStream_t s = (hipStream_t)stream;
    r = sup_step_group(h, a, s);
    if (r) return r;
    return out2 ? read_sup_out(h, h->models, a->rows_valid, out2, s) : 0;
}

int mrgan_ae_step(mrgan_handle* h, const mrgan_ae_args* a, float* out1, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    if (require_ae(h, "ae_step")) return -3;
    if (!a || !a->x_dev) return fail(-2, "ae_step: x is required");
    mrgan_sup_args u;       // (the fields mean what they mean in the supervised step)
    memset(&u, 0, sizeof u);
    u.ld_x = a->ld_x; u.stream_mode = a->stream_mode; u.rows_valid = a->rows_valid;
    int r = check_sup_args(h, u, "ae_step");
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    r = ae_step(h, a, s);
    if (r) return r;
    return out1 ? read_step_out(h, 1, 0, 1, out1, s) : 0;
}

int mrgan_ae_encode(mrgan_handle* h, const float* x, const int32_t* idx, int64_t ld, int64_t n, float* code, int64_t ld_code,
                    mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    if (require_ae(h, "ae_encode")) return -3;
    const int r = check_ae_rows(h, "ae_encode", x, ld, n);
    if (r) return r;
    if (!code) return fail(-2, "ae_encode: code_dev is required");
    if (ld_code < h->cfg.d_hidden[2]) return fail(-2, "ae_encode: row pitch ld_code smaller than d_hidden[2]");
    return ae_rows(h, x, idx, (long)ld, (long)n, 3, code, (long)ld_code, false, (hipStream_t)stream);
}

int mrgan_ae_reconstruct(mrgan_handle* h, const float* x, const int32_t* idx, int64_t ld, int64_t n, float* out, int64_t ld_out,
                         float* mse_host, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    if (require_ae(h, "ae_reconstruct")) return -3;
    int r = check_ae_rows(h, "ae_reconstruct", x, ld, n);
    if (r) return r;
    if (!out && !mse_host) return fail(-2, "ae_reconstruct: out_dev and mse_host are both null");
    if (out && ld_out < h->cfg.d_in) return fail(-2, "ae_reconstruct: row pitch ld_out smaller than d_in");
    hipStream_t s = (hipStream_t)stream;
    r = ae_rows(h, x, idx, (long)ld, (long)n, 6, out, (long)ld_out, mse_host != nullptr, s);
    if (r || !mse_host) return r;
    float sum = 0.f;
    HIPCHK(hipMemcpyAsync(&sum, h->ae_mse, sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *mse_host = (float)((double)sum / ((double)n * (double)h->cfg.d_in));
    return 0;
}

int mrgan_train_pair(mrgan_handle* h, const mrgan_disc_args* d, const mrgan_gen_args* g, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "train_pair");
    if (!r) r = refuse_group(h, "train_pair");
    if (!r) r = check_disc_args(h, d);
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
    // (the calibrating first pair of an fp8 handle runs eagerly)
    return run_pair(h, want_graph && !(h->fp8 && !(h->fp8_cal[0] == 1 && h->fp8_cal[1] == 1)), d, sizeof *d, g, sizeof *g, s, both);
}

int mrgan_disc_step_group(mrgan_handle* h, const mrgan_disc_group_args* a, float* out3, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "disc_step_group");
    if (!r) r = check_group_handle(h, "disc_step_group");
    if (!r) r = check_disc_group_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    r = disc_step_group(h, a, s);
    if (r) return r;
    return out3 ? read_step_out(h, h->models, 0, 3, out3, s) : 0;
}

int mrgan_gen_step_group(mrgan_handle* h, const mrgan_gen_group_args* a, float* out1, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "gen_step_group");
    if (!r) r = check_group_handle(h, "gen_step_group");
    if (!r) r = check_gen_group_args(h, a);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    r = gen_step_group(h, a, s);
    if (r) return r;
    return out1 ? read_step_out(h, h->models, 3, 1, out1, s) : 0;
}

int mrgan_train_pair_group(mrgan_handle* h, const mrgan_disc_group_args* d, const mrgan_gen_group_args* g, mrgan_stream stream) {
    if (!h) return fail(-1, "null handle");
    int r = refuse_ae(h, "train_pair_group");
    if (!r) r = check_group_handle(h, "train_pair_group");
    if (!r) r = check_disc_group_args(h, d);
    if (!r) r = check_gen_group_args(h, g);
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    const bool want_graph = !h->prof && (h->cfg.flags & MRGAN_FLAG_GRAPH) && d->stream_mode && g->stream_mode;
    // the two generator forwards run separately: bit-identical to the paired two-segment pass of mrgan_train_pair
    auto both = [&]() {
        int rr = disc_step_group(h, d, s);
        if (!rr) rr = gen_step_group(h, g, s);
        return rr;
    };
    return run_pair(h, want_graph, d, sizeof *d, g, sizeof *g, s, both);
}

int mrgan_eval_error(mrgan_handle* h, const float* x, const int32_t* idx, int64_t ld, const int32_t* labels, int64_t n,
                     float* err_host, mrgan_stream stream) {
    if (!h || !x || !labels || !err_host || n < 1) return fail(-1, "eval_error: bad argument");
    if (refuse_ae(h, "eval_error")) return -3;
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
    if (refuse_ae(h, "predict_logits")) return -3;
    if (ld < h->cfg.d_in) return fail(-2, "predict_logits: row pitch smaller than d_in");
    return eval_rows(h, x, idx, ld, nullptr, n, logits, (hipStream_t)stream);
}

// the attribution of one noise-free draw: nothing reads the classes back, so classes_out_dev may be null, and no draw slot is read
int mrgan_input_gradient(mrgan_handle* h, const mrgan_saliency_args* a, mrgan_stream stream) {
    mrgan_attribution_args f;
    memset(&f, 0, sizeof f);
    if (a) {
        f.x_dev = a->x_dev; f.idx_dev = a->idx_dev; f.ld_x = a->ld_x; f.n = a->n;
        f.targets_dev = a->targets_dev; f.objective = a->objective; f.post = a->post;
        f.out_dev = a->out_dev; f.ld_out = a->ld_out; f.classes_out_dev = a->classes_out_dev;
        f.method = MRGAN_ATTR_NOISE; f.draws = 1;
    }
    const int r = check_attribution(h, "input_gradient", a ? &f : nullptr);
    return r ? r : attribution_rows(h, &f, (hipStream_t)stream);
}

int mrgan_attribution(mrgan_handle* h, const mrgan_attribution_args* a, mrgan_stream stream) {
    const int r = check_attribution(h, "attribution", a);
    if (r) return r;
    if (!a->targets_dev && !a->classes_out_dev)
        return fail(-2, "attribution: classes_out_dev is required when targets_dev is null (the predicted classes are kept there between draws)");
    if (!h->draw_state) return fail(-1, "attribution: the handle has no draw slots");
    return attribution_rows(h, a, (hipStream_t)stream);
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

}  // extern "C"
