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

// ---- the non-GEMM kernels (aux_kernels.h), one entry per launcher.  The checks are what the launchers take on trust: 16-byte
// accesses and pitches that hold the logical widths. ----
static inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }
// the launcher's code after the stream has drained: -3 unchanged, a failed synchronisation as -10
static int debug_finish(const char* who, int r, hipStream_t s) {
    const hipError_t he = hipStreamSynchronize(s);
    if (r == -3) return fail(-3, "%s: launch refused (-3)", who);
    if (r) return fail(r, "%s: launch failed (%d)", who, r);
    if (he != hipSuccess) return fail(-10, "%s: %s", who, hipGetErrorString(he));
    return 0;
}
static void debug_head_args(const mrgan_debug_head_desc* d, const DevState* st, HeadArgs& a);     // descriptor -> HeadArgs, field by field
// a DevState pair on the device (the kernels read slot 0)
static int debug_devstate(uint32_t iter, uint32_t batch, float lr_t, DevState** out) {
    DevState hst[2];
    memset(hst, 0, sizeof hst);
    hst[0].iter = hst[1].iter = iter; hst[0].batch = hst[1].batch = batch; hst[0].lr_t = hst[1].lr_t = lr_t;
    HIPCHK(hipMalloc((void**)out, sizeof hst));
    const hipError_t he = hipMemcpy(*out, hst, sizeof hst, hipMemcpyHostToDevice);
    if (he != hipSuccess) { hipFree(*out); *out = nullptr; return fail(-10, "hipMemcpy failed: %s", hipGetErrorString(he)); }
    return 0;
}

int mrgan_debug_stage(const mrgan_debug_stage_desc* d, mrgan_stream stream) {
    if (!d || d->nseg < 1 || d->nseg > 5) return fail(-1, "debug_stage: 1 .. 5 segments");
    if (d->dtype != MRGAN_F32 && d->dtype != MRGAN_BF16) return fail(-1, "debug_stage: dtype must be fp32 or bf16");
    if (d->gauss && (d->row0 & 1u)) return fail(-1, "debug_stage: the true-Gaussian generator draws row pairs, row0 must be even");
    StageArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < d->nseg; ++i) {
        const mrgan_debug_stage_seg& g = d->s[i];
        StageSeg& o = a.s[i];
        if (!g.out || g.rows < 1 || g.cols < 1 || (!g.gen && !g.src)) return fail(-1, "debug_stage: segment %d: null argument", i);
        if (g.cols_pad < g.cols || (g.cols_pad % 8) || g.ldo < g.cols_pad || (g.ldo % 8) || !al(g.out, 16) || (g.out_ms % 16))
            return fail(-1, "debug_stage: segment %d: rows of out are stored 8 elements at a time (out, out_ms, ldo %% 8, cols <= cols_pad <= ldo, cols_pad %% 8)", i);
        if (!g.gen && g.ld < g.cols) return fail(-1, "debug_stage: segment %d: ld >= cols", i);
        o.src = g.src; o.idx = g.idx; o.ld = g.ld; o.rows = g.rows; o.cols = g.cols; o.cols_pad = g.cols_pad;
        o.out = g.out; o.ldo = g.ldo; o.sigma = g.sigma; o.site = g.site; o.seg = g.seg; o.gen = g.gen; o.stream = g.stream;
        o.iter_off = g.iter_off; o.models = g.models; o.src_ms = g.src_ms; o.idx_ms = g.idx_ms; o.out_ms = g.out_ms;
    }
    a.nseg = d->nseg; a.seed = d->seed; a.row0 = d->row0; a.gauss = d->gauss;
    DevState* st = nullptr;
    if (int r = debug_devstate(d->iter, d->batch, 0.f, &st)) return r;
    a.cur = st;
    hipStream_t s = (hipStream_t)stream;
    const int r = debug_finish("debug_stage", launch_stage(d->dtype == MRGAN_BF16, a, s), s);
    hipFree(st);
    return r;
}

int mrgan_debug_reduce_partials(const float* src, int nsrc, int64_t stride, int n, int ngroups, float* dst, int models, int64_t model_stride,
                                mrgan_stream stream) {
    if (!src || !dst || nsrc < 1 || n < 1 || ngroups < 1 || models < 1) return fail(-1, "debug_reduce_partials: empty problem");
    if (stride < n) return fail(-1, "debug_reduce_partials: stride >= n");
    if (model_stride % 4) return fail(-1, "debug_reduce_partials: model_stride counts bytes of whole floats");
    hipStream_t s = (hipStream_t)stream;
    return debug_finish("debug_reduce_partials", launch_reduce_partials(src, nsrc, stride, n, ngroups, dst, s, models, model_stride), s);
}

int mrgan_debug_colsum_finalize(const float* part1, const float* part2, int npart, int ld, int n, float* out, int nseg, mrgan_stream stream) {
    if (!part1 || !part2 || !out || npart < 1 || n < 1 || nseg < 1) return fail(-1, "debug_colsum_finalize: empty problem");
    if (!al(part1, 16) || !al(part2, 16) || (ld % 4)) return fail(-1, "debug_colsum_finalize: partial rows are read 16 bytes at a time (pointers, ld %% 4)");
    if (ld < n) return fail(-1, "debug_colsum_finalize: ld >= n");
    hipStream_t s = (hipStream_t)stream;
    return debug_finish("debug_colsum_finalize", launch_colsum_finalize(part1, part2, npart, ld, n, out, s, nseg), s);
}

// column partial sums as fold_partials reads them: four floats at a time over the `width` columns the kernel works on
static int debug_cs_check(const char* who, const float* cs1, const float* cs2, int npart, int ldcs, int width) {
    if (!cs1 || !cs2 || npart < 1) return fail(-1, "%s: column partial sums missing", who);
    if (!al(cs1, 16) || !al(cs2, 16) || (ldcs % 4)) return fail(-1, "%s: partial sums are read 16 bytes at a time (pointers, ldcs %% 4)", who);
    if (ldcs < width) return fail(-1, "%s: ldcs must hold the %d columns the kernel folds", who, width);
    return 0;
}

int mrgan_debug_bn_apply(const mrgan_debug_bn_apply_desc* d, mrgan_stream stream) {
    if (!d || !d->h || !d->out || !d->gamma || !d->beta || !d->mu || !d->rstd || d->rows < 1 || d->cols < 1) return fail(-1, "debug_bn_apply: null argument");
    if (d->dtype != MRGAN_F32 && d->dtype != MRGAN_BF16) return fail(-1, "debug_bn_apply: dtype must be fp32 or bf16");
    if (int r = debug_cs_check("debug_bn_apply", d->cs1, d->cs2, d->npart, d->ldcs, d->ld)) return r;
    if (d->ld < d->cols || (d->ld % 8) || !al(d->h, 16) || !al(d->out, 16)) return fail(-1, "debug_bn_apply: ld >= cols, ld %% 8 == 0 and 16-byte aligned h / out");
    if (d->nseg > 1 && ((d->cs_seg_stride % 4) || d->seg_rows < d->rows)) return fail(-1, "debug_bn_apply: cs_seg_stride %% 4 == 0 and seg_rows >= rows");
    BnApplyArgs a;
    memset(&a, 0, sizeof a);
    a.h = d->h; a.out = d->out; a.ld = d->ld; a.rows = d->rows; a.cols = d->cols;
    a.cs1 = d->cs1; a.cs2 = d->cs2; a.npart = d->npart; a.ldcs = d->ldcs; a.count = d->count; a.eps = d->eps;
    a.gamma = d->gamma; a.beta = d->beta; a.mu = d->mu; a.rstd = d->rstd;
    a.cs_seg_stride = d->cs_seg_stride; a.nseg = d->nseg; a.seg_rows = d->seg_rows;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish("debug_bn_apply", launch_bn_apply(d->dtype == MRGAN_BF16, a, s), s);
}

int mrgan_debug_bn_bwd(const mrgan_debug_bn_bwd_desc* d, mrgan_stream stream) {
    if (!d || !d->dy || !d->h || !d->dpre || !d->gamma || !d->mu || !d->rstd || !d->db_part || d->rows < 1 || d->cols < 1) return fail(-1, "debug_bn_bwd: null argument");
    if (d->dtype != MRGAN_F32 && d->dtype != MRGAN_BF16) return fail(-1, "debug_bn_bwd: dtype must be fp32 or bf16");
    if (int r = debug_cs_check("debug_bn_bwd", d->cs1, d->cs2, d->npart, d->ldcs, d->ld)) return r;
    if (d->ld < d->cols || (d->ld % 8) || !al(d->h, 16) || !al(d->dy, 16) || !al(d->dpre, 16)) return fail(-1, "debug_bn_bwd: ld >= cols, ld %% 8 == 0 and 16-byte aligned dy / h / dpre");
    BnBwdArgs a;
    memset(&a, 0, sizeof a);
    a.dy = d->dy; a.h = d->h; a.dpre = d->dpre; a.ld = d->ld; a.rows = d->rows; a.cols = d->cols;
    a.cs1 = d->cs1; a.cs2 = d->cs2; a.npart = d->npart; a.ldcs = d->ldcs; a.count = d->count;
    a.gamma = d->gamma; a.mu = d->mu; a.rstd = d->rstd; a.db_part = d->db_part;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish("debug_bn_bwd", launch_bn_bwd(d->dtype == MRGAN_BF16, a, s), s);
}

int mrgan_debug_head(const mrgan_debug_head_desc* d, mrgan_stream stream) {
    if (!d || !d->f || !d->w || !d->b || d->rows < 1 || d->nseg < 1 || d->nseg > 3 || d->feat < 1 || d->classes < 1) return fail(-1, "debug_head: null argument");
    if (d->dtype != MRGAN_F32 && d->dtype != MRGAN_BF16) return fail(-1, "debug_head: dtype must be fp32 or bf16");
    const int es = d->dtype == MRGAN_BF16 ? 2 : 4, kp = d->ldw;
    bool losses = false, labels = false;       // losses: a training kind, which also writes gradients
    for (int i = 0; i < d->nseg; ++i) {
        const int k = d->seg_kind[i];
        if (k < HEAD_LAB || k > HEAD_MSE) return fail(-1, "debug_head: unknown segment kind %d", k);
        losses |= k != HEAD_EVAL && k != HEAD_LOGITS;
        labels |= k == HEAD_LAB || k == HEAD_EVAL || k == HEAD_MSE;
    }
    if (d->feat_valid < 0 || d->feat_valid > d->feat || d->ldf < d->feat) return fail(-1, "debug_head: feat_valid <= feat <= ldf");
    // the feature rows are read 8 elements at a time, W6 / the partial rows / the logits' LDS image four floats at a time
    if (!al(d->f, 16) || ((int64_t)d->ldf * es % 16) || (d->f_bs * es % 16)) return fail(-1, "debug_head: feature rows are read 16 bytes at a time (f, ldf, f_bs)");
    if (!al(d->w, 16)) return fail(-1, "debug_head: w must be 16-byte aligned");
    if (labels && !d->labels) return fail(-1, "debug_head: the segment kinds need labels");
    if (losses && !d->loss_part) return fail(-1, "debug_head: training kinds need loss_part");
    if (losses && (!d->part || !al(d->part, 16) || (d->part_stride % 4) || (d->off_db % 4) || d->off_db < (int64_t)d->feat * kp || d->off_dbf < d->off_db + kp ||
                  d->part_stride < (int64_t)d->off_dbf + d->feat))
        return fail(-1, "debug_head: part rows hold dW6 [feat * ldw), db6 at off_db, the bias gradient at off_dbf, 16-byte aligned");
    if (d->dpre && d->ldd < d->feat) return fail(-1, "debug_head: ldd >= feat");
    if (d->models > 1 && (d->model_stride % 16)) return fail(-1, "debug_head: model_stride must keep the 16-byte alignments");
    if (d->q8_slot) {
        if (d->q8 && (!al(d->q8, 4) || (d->ldq8 % 4) || (d->q8_bs % 4) || d->ldq8 < d->feat)) return fail(-1, "debug_head: q8 is stored 4 bytes at a time, ldq8 >= feat");
        if (d->q8t && (!al(d->q8t, 16) || (d->ldq8t % 16) || (d->q8t_bs % 16) || d->q8t_bs < 0 ||
                       d->ldq8t < (int64_t)(d->nseg - 1) * d->q8t_bs + round_up(d->rows, HEAD_ROWS)))
            return fail(-1, "debug_head: q8t is stored 16 bytes at a time and holds nseg segments of round_up(rows, 32) bytes");
    }
    DevState* st = nullptr;
    if (int r = debug_devstate(0, d->batch, 0.f, &st)) return r;
    HeadArgs a;
    debug_head_args(d, st, a);
    hipStream_t s = (hipStream_t)stream;
    // the dynamic-LDS limits mrgan_create raises for a handle: no handle here, so once per process
    static int attr = init_kernel_attributes();
    int r = attr;
    if (!r) r = launch_head(d->dtype == MRGAN_BF16, a, s);
    r = debug_finish("debug_head", r, s);
    hipFree(st);
    return r;
}

static void debug_head_args(const mrgan_debug_head_desc* d, const DevState* st, HeadArgs& a) {
    memset(&a, 0, sizeof a);
    a.f = d->f; a.f_bs = d->f_bs; a.ldf = d->ldf; a.rows = d->rows; a.nseg = d->nseg;
    for (int i = 0; i < 3; ++i) a.seg_kind[i] = d->seg_kind[i];
    a.feat = d->feat; a.feat_valid = d->feat_valid; a.classes = d->classes;
    a.w = d->w; a.ldw = d->ldw; a.b = d->b; a.labels = d->labels; a.st = st; a.labels_stream = d->labels_stream;
    a.inv_count = d->inv_count; a.unl_weight = d->unl_weight;
    a.logits = d->logits; a.logits_bs = d->logits_bs; a.dpre = d->dpre; a.dpre_bs = d->dpre_bs; a.ldd = d->ldd;
    a.part = d->part; a.part_stride = d->part_stride; a.off_db = d->off_db; a.off_dbf = d->off_dbf; a.loss_part = d->loss_part;
    a.models = d->models; a.model_stride = d->model_stride; a.labels_ms = d->labels_ms; a.err_count = d->err_count;
    a.q8 = (unsigned char*)d->q8; a.q8_bs = d->q8_bs; a.ldq8 = d->ldq8;
    a.q8t = (unsigned char*)d->q8t; a.q8t_bs = d->q8t_bs; a.ldq8t = d->ldq8t; a.q8_slot = (Fp8Slot*)d->q8_slot;
}

int mrgan_debug_head_wide(const mrgan_debug_head_wide_desc* w, mrgan_stream stream) {
    if (!w || !w->h.f || !w->h.w || !w->h.b || w->h.rows < 1 || w->h.nseg < 1 || w->h.nseg > 3 || w->h.feat < 1 || w->h.classes < 1)
        return fail(-1, "debug_head_wide: null argument");
    const mrgan_debug_head_desc* d = &w->h;
    const int kp = d->ldw;
    if (d->models > 1) return fail(-1, "debug_head_wide: one model");
    if (d->feat_valid < 0 || d->feat_valid > d->feat || d->ldf < d->feat) return fail(-1, "debug_head_wide: feat_valid <= feat <= ldf");
    // the feature rows arrive 16 bytes at a time (LDS-DMA), the addends of W6 are read and dpre is stored 16 bytes at a time
    if (!al(d->f, 16) || (d->ldf % 8) || (d->f_bs % 8)) return fail(-1, "debug_head_wide: feature rows are read 16 bytes at a time (f, ldf, f_bs)");
    if (w->w6c && w->w6r && (!al(w->w6c, 16) || !al(w->w6r, 16))) return fail(-1, "debug_head_wide: w6c / w6r must be 16-byte aligned");
    if (w->mask && w->ldm < d->feat) return fail(-1, "debug_head_wide: ldm >= feat");
    if (!d->labels) return fail(-1, "debug_head_wide: labels");
    if (d->part && (!al(d->part, 16) || (d->part_stride % 4) || (d->off_db % 4) || d->off_db < (int64_t)d->feat * kp || d->off_dbf < d->off_db + kp ||
                    d->part_stride < (int64_t)d->off_dbf + d->feat))
        return fail(-1, "debug_head_wide: part rows hold dW6 [feat * ldw), db6 at off_db, the bias gradient at off_dbf, 16-byte aligned");
    if (d->dpre && (!al(d->dpre, 16) || (d->ldd % 8) || (d->dpre_bs % 8) || d->ldd < d->feat)) return fail(-1, "debug_head_wide: dpre is stored 16 bytes at a time, ldd >= feat");
    if (d->q8_slot) {
        if (d->q8 && (!al(d->q8, 16) || (d->ldq8 % 16) || (d->q8_bs % 16) || d->ldq8 < d->feat)) return fail(-1, "debug_head_wide: q8 is stored 16 bytes at a time, ldq8 >= feat");
        if (d->q8t && (!al(d->q8t, 16) || (d->ldq8t % 16) || (d->q8t_bs % 16) || d->q8t_bs < 0 ||
                       d->ldq8t < (int64_t)(d->nseg - 1) * d->q8t_bs + round_up(d->rows, HEAD_WIDE_ROWS)))
            return fail(-1, "debug_head_wide: q8t is stored 16 bytes at a time and holds nseg segments of round_up(rows, 64) bytes");
    }
    DevState* st = nullptr;
    if (int r = debug_devstate(0, d->batch, 0.f, &st)) return r;
    HeadWideArgs a;
    debug_head_args(d, st, a.h);
    a.mask = w->mask; a.mask_bs = w->mask_bs; a.ldm = w->ldm; a.w6c = (__bf16*)w->w6c; a.w6r = (__bf16*)w->w6r;
    hipStream_t s = (hipStream_t)stream;
    static int attr = head_wide_init_attributes();          // as in debug_head: once per process
    int r = attr;
    if (!r) r = launch_w6_split(a, s);
    if (!r) r = launch_head_wide(a, s);
    r = debug_finish("debug_head_wide", r, s);
    hipFree(st);
    return r;
}

int mrgan_debug_fm(const mrgan_debug_fm_desc* d, mrgan_stream stream) {
    if (!d || !d->cs || !d->mask || d->rows < 1 || d->feat < 1 || d->npart_fake < 1 || d->npart_real < 1) return fail(-1, "debug_fm: null argument");
    if (d->dtype != MRGAN_F32 && d->dtype != MRGAN_BF16) return fail(-1, "debug_fm: dtype must be fp32 or bf16");
    const int es = d->dtype == MRGAN_BF16 ? 2 : 4;
    if (!d->dpre && !d->q8_slot) return fail(-1, "debug_fm: needs dpre or the fp8 copy");
    if (d->feat_valid < 1 || d->feat_valid > d->feat) return fail(-1, "debug_fm: feat_valid <= feat");
    if (!al(d->cs, 16) || (d->ldcs % 4) || d->ldcs < d->feat) return fail(-1, "debug_fm: partial sums are read 16 bytes at a time, ldcs >= feat");
    if (!al(d->mask, 4) || d->ldm < d->feat) return fail(-1, "debug_fm: mask words are read in pairs, ldm >= feat");
    if (d->dpre && (!al(d->dpre, 16) || ((int64_t)d->ldd * es % 16) || d->ldd < d->feat)) return fail(-1, "debug_fm: dpre is stored 16 bytes at a time, ldd >= feat");
    if (d->q8_slot && (!d->q8 || !al(d->q8, 8) || (d->ldq8 % 8) || d->ldq8 < d->feat)) return fail(-1, "debug_fm: q8 is stored 8 bytes at a time, ldq8 >= feat");
    FmArgs a;
    memset(&a, 0, sizeof a);
    a.cs = d->cs; a.npart_fake = d->npart_fake; a.npart_real = d->npart_real; a.ldcs = d->ldcs;
    a.count = d->count; a.grad_scale = d->grad_scale; a.feat = d->feat; a.feat_valid = d->feat_valid;
    a.mask = d->mask; a.ldm = d->ldm; a.dpre = d->dpre; a.ldd = d->ldd; a.rows = d->rows;
    a.loss_out = d->loss_out; a.accum = d->accum;
    a.q8 = (unsigned char*)d->q8; a.ldq8 = d->ldq8; a.q8_slot = (Fp8Slot*)d->q8_slot;
    a.lscratch = d->lscratch; a.lcount = d->lcount;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish("debug_fm", launch_fm(d->dtype == MRGAN_BF16, a, s), s);
}

// one product's descriptor -> ChainOp; the checks are what chain_gemm / copy_out / load_mask_words take on trust
static int debug_chain_op(const mrgan_debug_chain_op& d, ChainOp& o, const char* what, int i) {
    memset(&o, 0, sizeof o);
    o.K = d.K; o.N = d.N; o.n_valid = d.n_valid; o.W = (const __bf16*)d.W; o.bias = d.bias; o.sigma = d.sigma; o.site = d.site;
    o.out = (__bf16*)d.out; o.out_bs = d.out_bs; o.ldo = d.ldo; o.mask = d.mask; o.mask_bs = d.mask_bs; o.ldm = d.ldm;
    o.cs = d.cs; o.ldcs = d.ldcs;
    if (!al(d.W, 16)) return fail(-1, "debug_chain: %s[%d]: W is read 16 bytes at a time", what, i);
    if (d.out && (!al(d.out, 16) || (d.ldo % 8) || (d.out_bs % 8) || d.ldo < d.N)) return fail(-1, "debug_chain: %s[%d]: out is stored 16 bytes at a time, ldo >= N", what, i);
    if (d.mask && d.ldm < d.N) return fail(-1, "debug_chain: %s[%d]: ldm >= N", what, i);
    // (the partial rows are what chain_fmgrad and the folds read back four floats at a time)
    if (d.cs && (!al(d.cs, 16) || (d.ldcs % 4) || d.ldcs < d.N)) return fail(-1, "debug_chain: %s[%d]: cs rows are 16-byte aligned, ldcs >= N", what, i);
    return 0;
}

int mrgan_debug_chain(const mrgan_debug_chain_desc* d, char* kname, int kname_len, mrgan_stream stream) {
    if (!d) return fail(-1, "null argument");
    if (kname && kname_len > 0) kname[0] = 0;
    if (d->variant < CH_V_DTAIL || d->variant > CH_V_GBWD) return fail(-1, "debug_chain: variant must be 0, 1 or 2");
    const bool has_fwd = d->variant != CH_V_GBWD, has_dx = d->variant != CH_V_GFWD;
    ChainArgs a;
    memset(&a, 0, sizeof a);
    a.variant = d->variant; a.rows = d->rows; a.nseg = d->nseg; a.block_rows = d->block_rows;
    a.models = d->models; a.model_stride = d->model_stride;
    a.a = (const __bf16*)d->a; a.a_bs = d->a_bs; a.lda = d->lda; a.a_cols = d->a_cols;
    a.seg0 = d->seg0; a.seed = d->seed; a.row0 = d->row0; a.gauss = d->gauss;
    int rop = 0;                               // (the launcher's refusals come first: a pitch is only judged on a shape it accepts)
    for (int i = 0; i < 3; ++i) {
        if (has_fwd) { if (int r = debug_chain_op(d->fwd[i], a.fwd[i], "fwd", i)) rop = rop ? rop : r; }
        if (has_dx) { if (int r = debug_chain_op(d->dx[i], a.dx[i], "dx", i)) rop = rop ? rop : r; }
    }
    if (d->variant == CH_V_DTAIL) debug_head_args(&d->head, nullptr, a.head);
    if (d->variant == CH_V_GBWD) {
        const mrgan_debug_fm_desc& f = d->fm;
        a.fm.cs = f.cs; a.fm.npart_fake = f.npart_fake; a.fm.npart_real = f.npart_real; a.fm.ldcs = f.ldcs;
        a.fm.count = f.count; a.fm.grad_scale = f.grad_scale; a.fm.feat = f.feat; a.fm.feat_valid = f.feat_valid;
        a.fm.dpre = f.dpre; a.fm.ldd = f.ldd; a.fm.rows = d->rows; a.fm.loss_out = f.loss_out; a.fm.accum = f.accum;
        a.fm_feat = (const __bf16*)d->fm_feat; a.fm_ldf = d->fm_ldf;
    }
    // before anything touches the device: a refused descriptor never reaches a launch
    if (!chain_args_ok(a)) return fail(-3, "debug_chain: launch refused (-3)");
    if (rop) return rop;
    if (d->models > 1 && (d->model_stride % 16)) return fail(-1, "debug_chain: model_stride must keep the 16-byte alignments");
    if (has_fwd && (!al(d->a, 16) || (d->lda % 8) || (d->a_bs % 8) || d->lda < d->a_cols)) return fail(-1, "debug_chain: the first A image is read 16 bytes at a time (a, a_bs, lda %% 8), lda >= a_cols");
    if (has_fwd && d->gauss && (d->row0 & 1u)) return fail(-1, "debug_chain: the true-Gaussian generator draws row pairs, row0 must be even");
    if (d->variant == CH_V_DTAIL) {
        const mrgan_debug_head_desc& h = d->head;
        if (!al(h.w, 16) || !al(h.part, 16) || (h.part_stride % 4) || (h.off_db % 4) || h.off_db < (int64_t)h.feat * KMAX || h.off_dbf < h.off_db + KMAX ||
            h.part_stride < (int64_t)h.off_dbf + h.feat)
            return fail(-1, "debug_chain: w and part are accessed 16 bytes at a time; part rows hold dW6 [feat * 8), db6 at off_db, the bias gradient at off_dbf");
        if (!al(h.dpre, 16) || (h.ldd % 8) || (h.dpre_bs % 8) || h.ldd < h.feat) return fail(-1, "debug_chain: head.dpre is stored 16 bytes at a time, ldd >= feat");
        if (d->models > 1 && (h.model_stride % 16)) return fail(-1, "debug_chain: head.model_stride must keep the 16-byte alignments");
    }
    if (d->variant == CH_V_GBWD) {
        const mrgan_debug_fm_desc& f = d->fm;
        if (!al(f.cs, 16) || (f.ldcs % 4) || f.ldcs < f.feat) return fail(-1, "debug_chain: fm.cs is read 16 bytes at a time, ldcs >= feat");
        if (!al(d->fm_feat, 16) || (d->fm_ldf % 8) || d->fm_ldf < f.feat) return fail(-1, "debug_chain: fm_feat is read 16 bytes at a time, fm_ldf >= feat");
        if (!al(f.dpre, 16) || (f.ldd % 8) || f.ldd < f.feat) return fail(-1, "debug_chain: fm.dpre is stored 16 bytes at a time, ldd >= feat");
    }
    DevState* st = nullptr;
    if (int r = debug_devstate(d->iter, d->batch, 0.f, &st)) return r;
    a.st = st; a.head.st = st;
    hipStream_t s = (hipStream_t)stream;
    static int attr = chain_init_attributes();              // as in debug_head: once per process
    int r = attr;
    if (!r) r = launch_chain(a, s);
    r = debug_finish("debug_chain", r, s);
    hipFree(st);
    if (!r && kname && kname_len > 0) chain_kernel_name(a, kname, kname_len);
    return r;
}

int mrgan_debug_adam(const mrgan_debug_adam_desc* d, uint32_t next_out[4], mrgan_stream stream) {
    if (!d || !d->tiles || d->ntiles < 1 || d->ntiles > 4096) return fail(-1, "debug_adam: null argument");
    if (d->mode < ADAM_FUSED || d->mode > ADAM_FROM_FLAT) return fail(-1, "debug_adam: unknown mode %d", d->mode);
    if (d->models > 1 && (d->model_stride % 16)) return fail(-1, "debug_adam: model_stride must keep the 16-byte alignments");
    if (d->step_out && (!d->accum || (d->mode == ADAM_FROM_FLAT ? !d->flat_tail : (!d->loss_part || d->nloss_part < 0)))) return fail(-1, "debug_adam: the metrics finish needs loss_part (or flat_tail) and accum");
    if (d->mode == ADAM_REDUCE_ONLY && d->step_out && !d->flat_tail) return fail(-1, "debug_adam: ADAM_REDUCE_ONLY needs flat_tail");
    std::vector<AdamTile> tiles((size_t)d->ntiles);
    for (int i = 0; i < d->ntiles; ++i) {
        const mrgan_debug_adam_tile& t = d->tiles[i];
        AdamTile& o = tiles[(size_t)i];
        if (t.rows < 1 || t.rows > 64 || t.cols < 4 || t.cols > 64 || (t.cols % 4)) return fail(-1, "debug_adam: tile %d: rows in 1 .. 64, cols a multiple of 4 in 4 .. 64", i);
        if (t.ld < t.cols || (t.ld % 4)) return fail(-1, "debug_adam: tile %d: ld >= cols, ld %% 4 == 0", i);
        const bool upd = d->mode != ADAM_REDUCE_ONLY, slabs = d->mode != ADAM_FROM_FLAT;
        if (upd && (!t.p || !t.m || !t.v || !al(t.p, 16) || !al(t.m, 16) || !al(t.v, 16))) return fail(-1, "debug_adam: tile %d: p / m / v are read 16 bytes at a time", i);
        if (slabs && (!t.g || !al(t.g, 16) || t.nslab < 1 || (t.slab_stride % 4))) return fail(-1, "debug_adam: tile %d: gradient slabs are read 16 bytes at a time", i);
        if (!slabs || !upd) {
            if (!t.flat && !t.flat16) return fail(-1, "debug_adam: tile %d: the mode needs flat or flat16", i);
            if ((t.flat && !al(t.flat, 16)) || (t.flat16 && !al(t.flat16, 8))) return fail(-1, "debug_adam: tile %d: flat / flat16 alignment", i);
        }
        if (t.w16 && !al(t.w16, 8)) return fail(-1, "debug_adam: tile %d: w16 is stored 8 bytes at a time", i);
        if (t.wt16 && (!t.w16 || !al(t.wt16, 16) || (t.ldt % 8) || t.ldt < round_up(t.rows, 16))) return fail(-1, "debug_adam: tile %d: wt16 is stored 16 bytes at a time, ldt >= round_up(rows, 16)", i);
        if (t.w8_slot && (!t.w16 || !t.w8 || !al(t.w8, 4) || (t.wt16 && (!t.w8t || !al(t.w8t, 16) || (t.ldt % 16))))) return fail(-1, "debug_adam: tile %d: the e4m3 copies follow w16 / wt16 (w8 4-byte, w8t 16-byte stores)", i);
        o.p = t.p; o.m = t.m; o.v = t.v; o.g = t.g; o.nslab = t.nslab; o.slab_stride = t.slab_stride;
        o.flat = t.flat; o.flat16 = (__bf16*)t.flat16; o.w16 = (__bf16*)t.w16; o.wt16 = (__bf16*)t.wt16;
        o.w8 = (unsigned char*)t.w8; o.w8t = (unsigned char*)t.w8t; o.w8_slot = (Fp8Slot*)t.w8_slot;
        o.ld = t.ld; o.ldt = t.ldt; o.rows = t.rows; o.cols = t.cols;
    }
    DevState* st = nullptr;
    if (int r = debug_devstate(d->iter, d->batch, d->lr_t, &st)) return r;
    AdamTile* dt = nullptr;
    DevState* next = nullptr;
    hipError_t he = hipMalloc((void**)&dt, tiles.size() * sizeof(AdamTile));
    if (he == hipSuccess) he = hipMemcpy(dt, tiles.data(), tiles.size() * sizeof(AdamTile), hipMemcpyHostToDevice);
    if (he == hipSuccess && d->publish_next) {
        he = hipMalloc((void**)&next, sizeof(DevState));
        if (he == hipSuccess) he = hipMemset(next, 0xA5, sizeof(DevState));
    }
    int r = he == hipSuccess ? 0 : fail(-10, "debug_adam: %s", hipGetErrorString(he));
    hipStream_t s = (hipStream_t)stream;
    if (!r) {
        AdamArgs a;
        memset(&a, 0, sizeof a);
        a.tiles = dt; a.ntiles = d->ntiles; a.mode = d->mode; a.b1 = d->b1; a.b2 = d->b2; a.eps = d->eps; a.st = st;
        a.loss_part = d->loss_part; a.nloss_part = d->nloss_part; a.inv_rows = d->inv_rows; a.step_out = d->step_out; a.accum = d->accum;
        a.flat_tail = d->flat_tail; a.next = next; a.advance_batch = d->advance_batch; a.lr = d->lr;
        a.models = d->models; a.model_stride = d->model_stride;
        r = debug_finish("debug_adam", launch_adam(a, s), s);
    }
    if (!r && next && next_out) {
        he = hipMemcpy(next_out, next, sizeof(DevState), hipMemcpyDeviceToHost);
        if (he != hipSuccess) r = fail(-10, "debug_adam: %s", hipGetErrorString(he));
    }
    hipFree(st);
    if (dt) hipFree(dt);
    if (next) hipFree(next);
    return r;
}

int mrgan_debug_svm_gram(const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n, int64_t d, float gamma,
                         float* out_dev, int64_t ld_out, int32_t tile, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_gram(a_dev, (long)ld_a, (long)m, b_dev, (long)ld_b, (long)n, (long)d, gamma, out_dev, (long)ld_out, tile,
                                  (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_debug_svm_kernel_matrix(int32_t kernel, const float* a_dev, int64_t ld_a, int64_t m, const float* b_dev, int64_t ld_b, int64_t n,
                                  int64_t d, float gamma, float* out_dev, int64_t ld_out, int32_t tile, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_svm_kernel_matrix(kernel, a_dev, (long)ld_a, (long)m, b_dev, (long)ld_b, (long)n, (long)d, gamma, out_dev,
                                           (long)ld_out, tile, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_debug_svm_gram_group(const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma, int32_t tile, mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_gram_group(items_host, count, (long)d, gamma, tile, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int mrgan_debug_svm_kernel_matrix_group(int32_t kernel, const mrgan_svm_gram_item* items_host, int32_t count, int64_t d, float gamma,
                                        int32_t tile, mrgan_stream stream) {
    const char* msg = "";
    int item = -1;
    const int r = launch_svm_kernel_matrix_group(kernel, items_host, count, (long)d, gamma, tile, (hipStream_t)stream, &msg, &item);
    return r ? svm_group_fail(r, msg, item) : 0;
}

int64_t mrgan_debug_pca_covariance_workspace_bytes(int64_t n, int64_t d, int32_t tile, int32_t split) {
    return pca_covariance_workspace_bytes((long)n, (long)d, tile, split);
}

int mrgan_debug_pca_covariance(const float* x_dev, int64_t ld_x, int64_t n, int64_t d, const float* mean_dev, float* cov_dev, int64_t ld_cov,
                               void* work_dev, int64_t work_bytes, int32_t tile, int32_t split, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_covariance(x_dev, (long)ld_x, (long)n, (long)d, mean_dev, cov_dev, (long)ld_cov, work_dev, (long)work_bytes, tile,
                                        split, (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

int mrgan_debug_pca_orthonormalize(const float* y_dev, int64_t ld_y, int64_t p, int64_t d, void* work_dev, int64_t work_bytes, float* q_dev,
                                   int64_t ld_q, double* lam_dev, mrgan_stream stream) {
    const char* msg = "";
    const int r = launch_pca_orthonormalize(y_dev, (long)ld_y, (long)p, (long)d, work_dev, (long)work_bytes, q_dev, (long)ld_q, lam_dev,
                                            (hipStream_t)stream, &msg);
    return r ? fail(r, "%s", msg) : 0;
}

}  // extern "C"
