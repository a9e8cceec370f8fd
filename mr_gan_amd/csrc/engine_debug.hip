// Diagnostic entries of include/mrgan_debug.h: parity tests and kernel timing experiments.  They describe their launches
// through the same builders (gemm.h) as the engine.
#include "engine_internal.h"

namespace mrgan {
int launch_tr_probe(unsigned short* out, hipStream_t s);
}

namespace {

template <typename T>
__global__ void to_f32_kernel(const T* src, long lds, float* dst, long ldd, int rows, int cols) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= rows || c >= cols) return;
    dst[(long)r * ldd + c] = Elem<T>::to_f32(src[(long)r * lds + c]);
}

}  // namespace

extern "C" {

int mrgan_debug_noise(mrgan_handle* h, uint32_t site, uint32_t seg, uint32_t step, uint32_t row0, int rows, int cols, float* out,
                      mrgan_stream stream) {
    if (!h || !out) return fail(-1, "null argument");
    if (h->gauss && (row0 & 1u)) return fail(-1, "debug_noise: a true-Gaussian handle draws row pairs, row0 must be even");
    CHK(launch_noise_debug(h->gauss, h->cfg.seed, site, seg, step, row0, rows, cols, out, (hipStream_t)stream));
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
        case 0: *ptr = selected(h, h->xin[l]); *ld = h->d[l].Kp; break;      // (group handles: the selected model's buffer)
        case 1: *ptr = selected(h, h->dpre[l]); *ld = h->d[l].Np; break;
        case 2: *ptr = selected(h, h->feat); *ld = h->Fp; break;
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
    int epi;
    if (op == 0 || op == 3 || op == 4) {       // 0: relu + noise + mask ; 3: relu + mask ; 4: plain relu
        epi = EPI_FWD; g = gemm_fwd_args(m, k, n, nbatch, ta, (long)m * k, k, tb, k, true);
        g.e.act = ACT_RELU; g.e.n_valid = n; g.e.bias = bias; g.e.ldo = n; g.e.out_bs = (long)m * n;
        g.e.sigma = op == 0 ? 0.5f : 0.f; g.e.site = 1;
        if (op != 4) { g.e.mask = mask; g.e.ldm = n; g.e.mask_bs = (long)(m / 32 + 1) * n * 2; }
    } else if (is_dx) {
        // 1: relu mask ; 5: softplus' with e.h + column sums ; 6: linear + xhat sums ; 7: linear + column sums ; 8: linear
        epi = EPI_DX; g = gemm_dx_args(m, k, n, nbatch, ta, (long)m * n, n, tb, n);
        g.e.act = op == 1 ? ACT_RELU : op == 5 ? ACT_SOFTPLUS : ACT_LINEAR; g.e.n_valid = k; g.e.ldo = k; g.e.out_bs = (long)m * k;
        if (op == 1) { g.e.mask = mask; g.e.ldm = k; g.e.mask_bs = (long)(m / 32 + 1) * k * 2; }
        if (op == 5 || op == 6) { g.e.h = ta; g.e.ldh = k; g.e.h_bs = (long)m * k; }
        if (op >= 5 && op <= 7) {
            HIPCHK(hipMalloc((void**)&slabs, (size_t)2 * (rows / 64 + 1) * k * 4));
            g.e.cs_mode = op == 6 ? CS_SUM_XHAT : CS_SUM; g.e.cs1 = slabs; g.e.cs2 = slabs + (size_t)(rows / 64 + 1) * k; g.e.ldcs = k;
            g.e.bn_mu = bias; g.e.bn_rstd = bias;
        }
    } else {
        epi = EPI_SLAB; splits = std::max(1, splits);
        HIPCHK(hipMalloc((void**)&slabs, (size_t)splits * k * n * 4));
        g = gemm_dw_args(k, n, m * nbatch, splits, gemm_dw_kchunk(m * nbatch, splits), 0, 0, ta, k, tb, n, false, slabs);
    }
    g.e.st = st; g.e.out = to; g.e.ablate = ablate; g.e.tune_kc_cfg = kc_cfg; g.e.seed = 1;
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
    GemmArgs g = gemm_fwd_args(m, k, n, 1, ta, 0, k, tb, k, true);
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

// one descriptor -> the launchers' argument block; the checks are the preconditions the kernels state for themselves
static int debug_gemm_args(const mrgan_debug_gemm_desc& d, const DevState* st, GemmArgs& g, int& epi) {
    const bool bf = d.dtype == MRGAN_BF16, f8 = d.dtype == MRGAN_FP8;
    if (!bf && !f8 && d.dtype != MRGAN_F32) return fail(-1, "debug_gemm_launch: dtype must be fp32, bf16 or fp8");
    if (d.op < 0 || d.op > 2) return fail(-1, "debug_gemm_launch: op must be 0, 1 or 2");
    if (!kc_cfg_supported(d.kc_cfg)) return fail(-1, "debug_gemm_launch: kc_cfg %d is not a block tile", d.kc_cfg);
    if (d.m < 1 || d.n < 1 || d.k < 1 || d.nbatch < 1 || d.splits < 1 || !d.a || !d.b) return fail(-1, "debug_gemm_launch: empty problem");
    if (d.n % 64) return fail(-1, "debug_gemm_launch: n must be a multiple of 64");
    // (a descriptor's m, n are the output's rows and columns: the builders take the layer's widths)
    epi = d.op == 0 ? EPI_FWD : d.op == 1 ? EPI_DX : EPI_SLAB;
    if (epi == EPI_FWD) g = gemm_fwd_args(d.m, d.k, d.n, d.nbatch, d.a, d.a_bs, d.a_si, d.b, d.b_sj, true);
    else if (epi == EPI_DX) g = gemm_dx_args(d.m, d.n, d.k, d.nbatch, d.a, d.a_bs, d.a_si, d.b, d.b_sj);
    else if (f8) g = gemm_dw_args(d.m, d.n, d.k, 1, d.k, 0, 0, d.a, d.a_si, d.b, d.b_sj, true, d.slab);
    else g = gemm_dw_args(d.m, d.n, d.k, 1, d.k, 0, 0, d.a, d.a_sk, d.b, d.b_sk, false, d.slab);
    // the descriptor states every stride, the split and the holes of the reduction itself: the tests also describe launches
    // the engine never makes, to see them refused
    g.nbatch = d.nbatch; g.splits = d.splits;
    if (d.kchunk > 0) g.kchunk = d.kchunk;
    if (d.seg_stride > 0) { g.seg_stride = d.seg_stride; g.seg_rows = d.seg_rows; }
    g.a_bs = d.a_bs; g.a_si = d.a_si; g.a_sk = d.a_sk;
    g.b_bs = d.b_bs; g.b_sk = d.b_sk; g.b_sj = d.b_sj;
    Epi& e = g.e;
    e.act = d.act; e.n_valid = d.n_valid; e.bias = d.bias;
    e.out = d.out; e.out_bs = d.out_bs; e.ldo = d.ldo;
    e.sigma = d.sigma; e.site = d.site; e.seg0 = d.seg0; e.seg_step = d.seg_step; e.iter_step = d.iter_step; e.row0 = d.row0; e.seed = d.seed;
    e.mask = d.mask; e.mask_bs = d.mask_bs; e.ldm = d.ldm;
    e.h = d.h; e.h_bs = d.h_bs; e.ldh = d.ldh;
    e.cs_mode = d.cs_mode; e.cs1 = d.cs1; e.cs2 = d.cs2; e.ldcs = d.ldcs; e.bn_mu = d.bn_mu; e.bn_rstd = d.bn_rstd;
    e.slab = d.slab; e.slab_stride = d.slab_stride;
    e.st = st; e.acc_scale = 1.f; e.tune_kc_cfg = d.kc_cfg; e.tune_bits = d.tune_bits;
    e.gauss = d.gauss;
    if (f8) {
        // which products, operand layouts, output forms and slots exist is the launcher's to refuse (-3); the entry refuses only
        // what the launcher takes on trust: images narrower than the tile rows they receive, the bf16 tile's 16-byte stores
        e.q8 = d.q8; e.q8_bs = d.q8_bs; e.ldq8 = d.ldq8; e.q8t = d.q8t; e.q8t_bs = d.q8t_bs; e.ldq8t = d.ldq8t;
        e.qa = (const Fp8Slot*)d.slot_a; e.qb = (const Fp8Slot*)d.slot_b; e.qo = (Fp8Slot*)d.slot_o;
        if (epi == EPI_SLAB ? d.ldo < d.n : (d.out && (d.ldo < d.n || (d.ldo % 8)))) return fail(-1, "debug_gemm_launch: fp8 product needs ldo >= n (bf16: a multiple of 8)");
        if ((d.a_si % 16) || (d.b_sj % 16) || (d.a_bs % 16) || (d.b_bs % 16)) return fail(-1, "debug_gemm_launch: fp8 row and batch pitches must be multiples of 16 bytes");
        if (d.q8 && (d.q8_bs % 16)) return fail(-1, "debug_gemm_launch: q8_bs must be a multiple of 16");
        if (d.q8 && d.ldq8 < d.n) return fail(-1, "debug_gemm_launch: ldq8 >= n");
        if (d.q8t && (d.q8t_bs < 0 || d.ldq8t < (d.nbatch - 1) * d.q8t_bs + round_up(d.m, 16))) return fail(-1, "debug_gemm_launch: ldq8t must hold nbatch batches of round_up(m, 16) bytes");
    }
    if (epi == EPI_SLAB && !f8) {
        const int bk = bf ? 64 : 16;
        if (!d.slab || d.ldo < d.n) return fail(-1, "debug_gemm_launch: weight gradient needs slab and ldo >= n");
        if ((g.kchunk % bk) || (g.seg_stride % bk)) return fail(-1, "debug_gemm_launch: kchunk and seg_stride must be multiples of %d", bk);
        // 16-byte operand loads of the bf16 kernels: 8 elements per predicate
        if (bf && ((d.a_sk % 8) || (d.b_sk % 8) || d.a_sk < round_up(d.m, 8))) return fail(-1, "debug_gemm_launch: bf16 row pitches must be multiples of 8");
    } else if (epi != EPI_SLAB) {
        if ((!f8 && !d.out) || (d.out && d.ldo < d.n) || d.n_valid < 0 || d.n_valid > d.n) return fail(-1, "debug_gemm_launch: needs out, ldo >= n and n_valid <= n");
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
            r = d[0].dtype == MRGAN_FP8    ? launch_gemm_fp8(epi, g, s, &name)
                : d[0].dtype == MRGAN_BF16 ? launch_gemm_bf16(epi, g, s, &name)
                                           : launch_gemm_f32(epi, g, s, &name);
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

int mrgan_debug_quant8(const void* src, int64_t src_bs, int ld, int rows, int cols, int nb, int prow, void* dst, int64_t dst_bs, int ldd,
                       void* dstt, int64_t dstt_bs, int lddt, void* slot, int fmt, mrgan_stream stream) {
    if (!src || rows < 0 || rows > prow || cols < 1 || cols > ld || (fmt != FP8_E4M3 && fmt != FP8_E5M2)) return fail(-1, "debug_quant8: bad argument");
    if ((dst && ldd < cols) || (dstt && (dstt_bs < 0 || lddt < (int64_t)(nb - 1) * dstt_bs + prow))) return fail(-1, "debug_quant8: ldd >= cols, lddt >= nb batches of prow bytes");
    Quant8Args a;
    memset(&a, 0, sizeof a);
    a.src = (const __bf16*)src; a.src_bs = src_bs; a.ld = ld; a.rows = rows; a.cols = cols; a.nb = nb; a.prow = prow;
    a.dst = (unsigned char*)dst; a.dst_bs = dst_bs; a.ldd = ldd;
    a.dstt = (unsigned char*)dstt; a.dstt_bs = dstt_bs; a.lddt = lddt;
    a.slot = (Fp8Slot*)slot; a.fmt = fmt;
    hipStream_t s = (hipStream_t)stream;
    const int r = launch_quant8(a, s);
    if (r) return fail(r, "debug_quant8: launch refused (%d)", r);
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int mrgan_debug_fp8_update_scales(void* slots, int n, mrgan_stream stream) {
    if (!slots || n < 1) return fail(-1, "debug_fp8_update_scales: bad argument");
    hipStream_t s = (hipStream_t)stream;
    CHK(launch_fp8_update_scales((Fp8Slot*)slots, n, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
