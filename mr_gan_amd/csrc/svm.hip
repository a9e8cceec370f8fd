// RBF-kernel C-SVC on the device: what SVC(kernel='rbf', C=1) of the reference's SVM baseline (mr_svm.py:106) computes.
//
//   svm_gram_kernel    K[a, b] = exp(-gamma * max(0, |A_a|^2 + |B_b|^2 - 2 A_a . B_b)), fp32.  The dot product is the k-ordered
//                      v_mfma_f32_32x32x2_f32 chain of gemm_f32.hip (same fragments, same k-major LDS image); the row norms are
//                      the same chain written with fmaf over the staged tile, so with A == B the diagonal's distance is exactly
//                      0 and K_ii exactly 1.0f, and K[a, b] == K[b, a] bit for bit (products and the norm sum commute).
//   svm_smo_kernel     libsvm's C-SVC Solver without shrinking, one 1024-thread workgroup per one-vs-one pair: alpha and G
//                      (fp64) stay in LDS for the whole solve, an iteration is two block reductions (working-set selection
//                      WSS2) and two coalesced fp32 Gram rows.  No grid barrier, nothing polls memory, every loop ends at max_iter.
//   svm_decide_kernel  per test row: the pairs' decision values (fp64 sums) and the one-vs-one vote.
// The other libsvm classifiers of the reference's grid (others/wganlpctsemi.py:205-208) reuse the three stages:
//   svm_gram_kernel<TS, LINEAR>  K[a, b] = A_a . B_b: the same chain, no norms, no expf (SVC / NuSVC(kernel='linear'))
//   svm_smo_nu_kernel  libsvm's nu-SVC (solve_nu_svc, Solver_NU) without shrinking, under svm_smo_kernel's discipline
//
// Each has a grouped twin (svm_*_group_kernel) for up to SVM_MAX_GROUP ragged problems in one launch: the same __device__ body
// (gram_tile, smo_pair, smo_nu_pair, decide_row), a block finding its problem from blockIdx through the descriptors in the
// kernel arguments: svm_gram_group_kernel<TS, KIND> for both kernel kinds, svm_smo_group_kernel and svm_smo_nu_group_kernel (nu per
// item) for the two solvers, svm_decide_group_kernel for every kind.
//
// Rows are sorted by class: pair (i, j), i < j, is the two contiguous row ranges of classes i and j, y = +1 on class i.
#include <math.h>

#include "common.h"
#include "svm.h"

namespace mrgan {

namespace {
constexpr int BK = 16;
constexpr int RBF = MRGAN_SVM_KERNEL_RBF, LINEAR = MRGAN_SVM_KERNEL_LINEAR;

// one TS x TS tile of the window, rows from row_blk and columns from col_blk: the body of the single and of the grouped kernel.
// KIND == LINEAR writes the dot product's chain itself: no norms, no expf, gamma unused.
template <int TS, int KIND = RBF>
__device__ __forceinline__ void gram_tile(const float* __restrict__ A, long ld_a, int M, const float* __restrict__ B, long ld_b, int N, int D,
                                          float gamma, float* __restrict__ out, long ld_out, int row_blk, int col_blk) {
    constexpr int LDT = TS, MR = TS / 64, KPT = TS / 16;      // KPT: k values staged per thread
    __shared__ __attribute__((aligned(16))) float lds[2 * BK * TS + 2 * TS];
    float* As = lds;
    float* Bs = lds + BK * LDT;
    float* nrm = lds + 2 * BK * LDT;                         // [0, TS): |A_row|^2, [TS, 2 TS): |B_row|^2

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // staging map: thread -> (row t % TS of the tile, KPT consecutive k starting at (t / TS) * KPT)
    const int si = t % TS, sk = (t / TS) * KPT;
    const bool a_row_ok = (row_blk + si) < M;
    const bool b_row_ok = (col_blk + si) < N;
    const float* a_ptr = A + (long)(row_blk + si) * ld_a;
    const float* b_ptr = B + (long)(col_blk + si) * ld_b;

    f32x16 acc[MR][MR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < MR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float ra[KPT], rb[KPT];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int k = k0 + sk + j;
            ra[j] = (a_row_ok && k < D) ? a_ptr[k] : 0.f;
            rb[j] = (b_row_ok && k < D) ? b_ptr[k] : 0.f;
        }
    };
    // the norm of tile row t (A) or t - TS (B): the dot product's own chain, fmaf(v_k, v_k, .) in k order; a padded k adds 0
    const float* nsrc = t < TS ? As + t : Bs + (t - TS);
    float nacc = 0.f;

    load_tile(0);
    for (int k0 = 0; k0 < D; k0 += BK) {
        __syncthreads();                 // previous tile's fragment reads done
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            As[(sk + j) * LDT + si] = ra[j];
            Bs[(sk + j) * LDT + si] = rb[j];
        }
        __syncthreads();
        if (k0 + BK < D) load_tile(k0 + BK);      // in flight under the MFMAs below
        if (KIND == RBF && t < 2 * TS) {
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) {
                const float v = nsrc[kk * LDT];
                nacc = fmaf(v, v, nacc);
            }
        }
        const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[MR], b[MR];
#pragma unroll
            for (int mi = 0; mi < MR; ++mi) a[mi] = As[(2 * kk + lh) * LDT + (wm * MR + mi) * 32 + lr];
#pragma unroll
            for (int ni = 0; ni < MR; ++ni) b[ni] = Bs[(2 * kk + lh) * LDT + (wn * MR + ni) * 32 + lr];
#pragma unroll
            for (int mi = 0; mi < MR; ++mi)
#pragma unroll
                for (int ni = 0; ni < MR; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
    }
    if (KIND == RBF) {
        if (t < 2 * TS) nrm[t] = nacc;
        __syncthreads();
    }

    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < MR; ++mi)
#pragma unroll
        for (int ni = 0; ni < MR; ++ni) {
            const int lc = (wn * MR + ni) * 32 + lr, col = col_blk + lc;
            if (col >= N) continue;
            const float nb = KIND == RBF ? nrm[TS + lc] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = (wm * MR + mi) * 32 + acc_row(r, lh), row = row_blk + lrow;
                if (row >= M) continue;
                if (KIND == RBF) {
                    const float d2 = fmaxf(0.f, fmaf(-2.f, acc[mi][ni][r], nrm[lrow] + nb));
                    out[(long)row * ld_out + col] = expf(-gamma * d2);
                } else {
                    out[(long)row * ld_out + col] = acc[mi][ni][r];
                }
            }
        }
}

template <int TS, int KIND = RBF>
__global__ __launch_bounds__(256) void svm_gram_kernel(const float* __restrict__ A, long ld_a, int M, const float* __restrict__ B, long ld_b,
                                                       int N, int D, float gamma, float* __restrict__ out, long ld_out) {
    gram_tile<TS, KIND>(A, ld_a, M, B, ld_b, N, D, gamma, out, ld_out, blockIdx.y * TS, blockIdx.x * TS);
}

// The descriptors of a group reach the kernels BY VALUE in the kernel arguments (no device table: the entries neither
// allocate nor copy).  A block indexes them with blockIdx alone, so the item's fields are scalar loads from the
// argument segment into SGPRs.  The HIP programming guide gives 4 KB as the size of a kernel's arguments.
constexpr int KERNARG_LIMIT = 4096;

struct GramItem { const float* a; const float* b; float* out; long ld_a, ld_b, ld_out; int m, n; };
// the grid is the concatenation of the items' tile lists: item i owns blocks tile_start[i] .. tile_start[i + 1] - 1, row-major
// over its tiles (tiles_x[i] per tile row), as blockIdx.x / .y order them in the single launch
struct GramGroup { GramItem item[SVM_MAX_GROUP]; int tile_start[SVM_MAX_GROUP + 1]; int tiles_x[SVM_MAX_GROUP]; };
static_assert(sizeof(GramGroup) + 16 <= KERNARG_LIMIT, "svm_gram_group_kernel: descriptors beyond the kernel argument limit");

template <int TS, int KIND = RBF>
__global__ __launch_bounds__(256) void svm_gram_group_kernel(const GramGroup g, int count, int D, float gamma) {
    const int bid = blockIdx.x;
    int it = 0;
    while (it + 1 < count && bid >= g.tile_start[it + 1]) ++it;       // wave-uniform: blockIdx and arguments only
    const GramItem& d = g.item[it];
    const int local = bid - g.tile_start[it], tx = g.tiles_x[it], ty = local / tx;
    gram_tile<TS, KIND>(d.a, d.ld_a, d.m, d.b, d.ld_b, d.n, D, gamma, d.out, d.ld_out, ty * TS, (local - ty * tx) * TS);
}

// ---------------------------------------------------------------------------------------------------------------------
// SMO
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SMO_THREADS = 1024, SMO_WAVES = SMO_THREADS / 64, SMO_PER = SVM_MAX_PAIR / SMO_THREADS;
constexpr double SMO_TAU = 1e-12;

// pair index p -> classes (ci < cj), in the order (0,1), (0,2), .., (1,2), ..  (libsvm's, scikit-learn's 'ovo' columns)
__device__ __forceinline__ void pair_classes(int p, int num_classes, int& ci, int& cj) {
    ci = 0;
    while (p >= num_classes - 1 - ci) { p -= num_classes - 1 - ci; ++ci; }
    cj = ci + 1 + p;
}

// (value, index) candidates: larger value wins, equal values go to the higher index -- what libsvm's ascending `>=` scan keeps
__device__ __forceinline__ void take_max(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
}

// The whole solve of pair `pair` = classes (ci, cj) of one problem by one workgroup: the body of the single and of the grouped
// kernel (one copy of the solver).  s1, n1 / s2, n2: first row and size of the two classes; rho and iters are the problem's.
__device__ __forceinline__ void smo_pair(const float* __restrict__ K, long ld_k, int n, int pair, int ci, int cj, int s1, int n1, int s2, int n2,
                                         double C, double tol, int max_iter, double* __restrict__ coef, double* __restrict__ rho,
                                         int* __restrict__ iters) {
    __shared__ double s_alpha[SVM_MAX_PAIR], s_G[SVM_MAX_PAIR];
    __shared__ float s_diag[SVM_MAX_PAIR], s_Ki[SVM_MAX_PAIR];
    __shared__ double r1_v[SMO_WAVES], r2_v[SMO_WAVES], r2_m[SMO_WAVES];
    __shared__ int r1_i[SMO_WAVES], r2_i[SMO_WAVES];
    __shared__ double f_ub[SMO_WAVES], f_lb[SMO_WAVES], f_sum[SMO_WAVES];
    __shared__ int f_cnt[SMO_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = n1 + n2;                                   // <= SVM_MAX_PAIR (checked by the launcher)
    auto grow = [&](int t) { return t < n1 ? s1 + t : s2 + (t - n1); };     // row of the Gram matrix behind local index t

    int own[SMO_PER], gown[SMO_PER];
    double yown[SMO_PER];
#pragma unroll
    for (int e = 0; e < SMO_PER; ++e) {
        const int t = tid + e * SMO_THREADS;
        own[e] = t;
        gown[e] = t < l ? grow(t) : 0;
        yown[e] = t < n1 ? 1.0 : -1.0;
        if (t < l) {
            s_alpha[t] = 0.0;
            s_G[t] = -1.0;
            s_diag[t] = K[(long)gown[e] * ld_k + gown[e]];
        }
    }
    __syncthreads();

    int it = 0;
    while (it < max_iter) {
        // ---- i = argmax over I_up of -y G ----
        double bv = -INFINITY;
        int bi = -1;
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                const double a = s_alpha[t];
                const bool up = yown[e] > 0 ? a < C : a > 0.0;
                if (up) take_max(bv, bi, -yown[e] * s_G[t], t);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) take_max(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) { r1_v[wave] = bv; r1_i[wave] = bi; }
        __syncthreads();                                                           // (1)
        bv = r1_v[0]; bi = r1_i[0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) take_max(bv, bi, r1_v[w], r1_i[w]);
        const int i = bi;
        const double Gmax = bv;
        if (i < 0) break;                                                          // block-uniform: every thread reduced the same values

        const long gi = grow(i);
        float ki[SMO_PER];
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) ki[e] = own[e] < l ? K[gi * ld_k + gown[e]] : 0.f;
        const double a_i = s_alpha[i], G_i = s_G[i], QD_i = (double)s_diag[i], y_i = i < n1 ? 1.0 : -1.0;

        // ---- j = argmin over I_low, b_t > 0, of -b_t^2 / a_t;  Gmax2 = max over I_low of y G ----
        double ov = -INFINITY, gm2 = -INFINITY;                                    // ov holds +b^2/a: the largest is libsvm's smallest
        int oj = -1;
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                s_Ki[t] = ki[e];
                const double a = s_alpha[t];
                const bool low = yown[e] > 0 ? a > 0.0 : a < C;
                if (low) {
                    const double yG = yown[e] * s_G[t];
                    gm2 = fmax(gm2, yG);
                    const double gd = Gmax + yG;
                    if (gd > 0.0) {
                        double q = QD_i + (double)s_diag[t] - 2.0 * (double)ki[e];
                        if (!(q > 0.0)) q = SMO_TAU;
                        take_max(ov, oj, (gd * gd) / q, t);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            take_max(ov, oj, __shfl_xor(ov, o, 64), __shfl_xor(oj, o, 64));
            gm2 = fmax(gm2, __shfl_xor(gm2, o, 64));
        }
        if (lane == 0) { r2_v[wave] = ov; r2_i[wave] = oj; r2_m[wave] = gm2; }
        __syncthreads();                                                           // (2)
        ov = r2_v[0]; oj = r2_i[0]; gm2 = r2_m[0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) { take_max(ov, oj, r2_v[w], r2_i[w]); gm2 = fmax(gm2, r2_m[w]); }
        if (Gmax + gm2 < tol || oj < 0) break;                                     // block-uniform
        const int j = oj;

        const long gj = grow(j);
        float kj[SMO_PER];
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) kj[e] = own[e] < l ? K[gj * ld_k + gown[e]] : 0.f;
        const double a_j = s_alpha[j], G_j = s_G[j], QD_j = (double)s_diag[j], y_j = j < n1 ? 1.0 : -1.0;

        // ---- the two-variable update, libsvm's clipping order (every thread computes the same values) ----
        double q = QD_i + QD_j - 2.0 * (double)s_Ki[j];
        if (!(q > 0.0)) q = SMO_TAU;
        double na_i = a_i, na_j = a_j;
        if (y_i != y_j) {
            const double delta = (-G_i - G_j) / q, diff = a_i - a_j;
            na_i += delta; na_j += delta;
            if (diff > 0.0) { if (na_j < 0.0) { na_j = 0.0; na_i = diff; } }
            else { if (na_i < 0.0) { na_i = 0.0; na_j = -diff; } }
            if (diff > 0.0) { if (na_i > C) { na_i = C; na_j = C - diff; } }
            else { if (na_j > C) { na_j = C; na_i = C + diff; } }
        } else {
            const double delta = (G_i - G_j) / q, sum = a_i + a_j;
            na_i -= delta; na_j += delta;
            if (sum > C) { if (na_i > C) { na_i = C; na_j = sum - C; } }
            else { if (na_j < 0.0) { na_j = 0.0; na_i = sum; } }
            if (sum > C) { if (na_j > C) { na_j = C; na_i = sum - C; } }
            else { if (na_i < 0.0) { na_i = 0.0; na_j = sum; } }
        }
        const double da_i = na_i - a_i, da_j = na_j - a_j;
        __syncthreads();                                                           // (3) alpha, G, Ki of i and j are read everywhere
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                if (t == i) s_alpha[t] = na_i;
                if (t == j) s_alpha[t] = na_j;
                // Q_i[t] = y_i y_t K_it is a float in libsvm as well; the products and the sum are fp64
                s_G[t] += (double)ki[e] * (y_i * yown[e]) * da_i + (double)kj[e] * (y_j * yown[e]) * da_j;
            }
        }
        ++it;
        // the next reads of another thread's alpha / G come after barrier (1) of the next iteration
    }
    __syncthreads();

    // ---- rho = calculate_rho: mean of y G over the free variables, else the midpoint of the bounds ----
    double ub = INFINITY, lb = -INFINITY, sum_free = 0.0;
    int nr_free = 0;
#pragma unroll
    for (int e = 0; e < SMO_PER; ++e) {
        const int t = own[e];
        if (t < l) {
            const double a = s_alpha[t], yG = yown[e] * s_G[t];
            if (a >= C) { if (yown[e] < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
            else if (a <= 0.0) { if (yown[e] > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
            else { ++nr_free; sum_free += yG; }
            const double c = a * yown[e];
            if (t < n1) coef[(long)(cj - 1) * n + gown[e]] = c;             // libsvm's sv_coef rows: class i's rows against class j
            else coef[(long)ci * n + gown[e]] = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ub = fmin(ub, __shfl_xor(ub, o, 64));
        lb = fmax(lb, __shfl_xor(lb, o, 64));
        sum_free += __shfl_xor(sum_free, o, 64);
        nr_free += __shfl_xor(nr_free, o, 64);
    }
    if (lane == 0) { f_ub[wave] = ub; f_lb[wave] = lb; f_sum[wave] = sum_free; f_cnt[wave] = nr_free; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SMO_WAVES; ++w) {
            ub = fmin(ub, f_ub[w]); lb = fmax(lb, f_lb[w]); sum_free += f_sum[w]; nr_free += f_cnt[w];
        }
        rho[pair] = nr_free > 0 ? sum_free / nr_free : (ub + lb) / 2;
        iters[pair] = it;
    }
}

__global__ __launch_bounds__(SMO_THREADS) void svm_smo_kernel(const float* __restrict__ K, long ld_k, int n, int num_classes,
                                                              const SvmClasses cls, double C, double tol, int max_iter,
                                                              double* __restrict__ coef, double* __restrict__ rho, int* __restrict__ iters) {
    int ci, cj;
    pair_classes(blockIdx.x, num_classes, ci, cj);
    const int s1 = cls.start[ci], n1 = cls.start[ci + 1] - s1, s2 = cls.start[cj], n2 = cls.start[cj + 1] - s2;
    smo_pair(K, ld_k, n, blockIdx.x, ci, cj, s1, n1, s2, n2, C, tol, max_iter, coef, rho, iters);
}

struct SmoItem { const float* k; long ld_k; double* coef; double* rho; int* iters; int n; SvmClasses cls; };
struct SmoGroup { SmoItem item[SVM_MAX_GROUP]; };
static_assert(sizeof(SmoGroup) + 32 <= KERNARG_LIMIT, "svm_smo_group_kernel: descriptors beyond the kernel argument limit");

// grid (pairs, count): blockIdx.y is the problem, blockIdx.x its pair.  No block waits for another: a group is count x pairs
// independent solves, each ending at max_iter.
__global__ __launch_bounds__(SMO_THREADS) void svm_smo_group_kernel(const SmoGroup g, int num_classes, double C, double tol, int max_iter) {
    const SmoItem& d = g.item[blockIdx.y];
    int ci, cj;
    pair_classes(blockIdx.x, num_classes, ci, cj);
    const int s1 = d.cls.start[ci], n1 = d.cls.start[ci + 1] - s1, s2 = d.cls.start[cj], n2 = d.cls.start[cj + 1] - s2;
    smo_pair(d.k, d.ld_k, d.n, blockIdx.x, ci, cj, s1, n1, s2, n2, C, tol, max_iter, d.coef, d.rho, d.iters);
}

// ---------------------------------------------------------------------------------------------------------------------
// nu-SVC: libsvm's solve_nu_svc / Solver_NU without shrinking, under smo_pair's discipline (one workgroup per pair, fp64 alpha
// and G in LDS, two block reductions per iteration, every loop ends at max_iter).  It shares take_max and pair_classes with
// smo_pair and nothing else.  The box is [0, 1], the linear term 0, and the two signs never mix: i and j of an update share
// their sign, so an iteration needs row ip or row in of the Gram matrix per COLUMN (by the column's sign) for the selection,
// and the chosen one of the two whole rows for the update.  Both rows are read up front in one round trip, row j in a second.
// fp64 contraction is off: every product and sum rounds as libsvm's does, and the sums run in libsvm's order, so a pair
// follows libsvm's pivots for as long as the two agree bit for bit.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void smo_nu_pair(const float* __restrict__ K, long ld_k, int n, int pair, int ci, int cj, int s1, int n1, int s2, int n2,
                                            double nu, double tol, int max_iter, double* __restrict__ coef, double* __restrict__ rho,
                                            double* __restrict__ r_out, int* __restrict__ iters) {
#pragma clang fp contract(off)
    __shared__ double s_alpha[SVM_MAX_PAIR], s_G[SVM_MAX_PAIR];
    __shared__ float s_diag[SVM_MAX_PAIR], s_Km[SVM_MAX_PAIR];      // s_Km[t]: K[ip][t] on class i's columns, K[in][t] on class j's
    __shared__ double r1_p[SMO_WAVES], r1_n[SMO_WAVES], r2_v[SMO_WAVES], r2_p[SMO_WAVES], r2_n[SMO_WAVES];
    __shared__ int r1_ip[SMO_WAVES], r1_in[SMO_WAVES], r2_i[SMO_WAVES];
    __shared__ double s_r;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = n1 + n2;                                   // <= SVM_MAX_PAIR (checked by the launcher)
    auto grow = [&](int t) { return t < n1 ? s1 + t : s2 + (t - n1); };     // row of the Gram matrix behind local index t

    // ---- start point: per sign alpha = min(1, remaining), remaining from nu l / 2.  remaining after k rows is nu l / 2 - k
    // exactly (a double minus a smaller integer is representable), so row k of its sign holds min(1, max(0, nu l / 2 - k)) ----
    const double half = nu * (double)l / 2;
    int own[SMO_PER], gown[SMO_PER];
    bool pos[SMO_PER];
#pragma unroll
    for (int e = 0; e < SMO_PER; ++e) {
        const int t = tid + e * SMO_THREADS;
        own[e] = t;
        gown[e] = t < l ? grow(t) : 0;
        pos[e] = t < n1;
        if (t < l) {
            s_alpha[t] = fmin(1.0, fmax(0.0, half - (double)(t < n1 ? t : t - n1)));
            s_diag[t] = K[(long)gown[e] * ld_k + gown[e]];
        }
    }
    __syncthreads();
    // ---- initial gradient: G_t = sum over alpha_s > 0, ascending s, of alpha_s * Q_st (Q a float, the sum fp64): a thread
    // owns its t and walks the rows s; the reads K[row(s)][own t] are coalesced ----
    {
        double g[SMO_PER];
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) g[e] = 0.0;
        for (int s = 0; s < l; ++s) {
            const double a = s_alpha[s];                     // block-uniform
            if (!(a > 0.0)) continue;
            const long gs = grow(s);
            const bool spos = s < n1;
#pragma unroll
            for (int e = 0; e < SMO_PER; ++e)
                if (own[e] < l) {
                    const float k = K[gs * ld_k + gown[e]];
                    g[e] += a * (double)(spos == pos[e] ? k : -k);
                }
        }
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e)
            if (own[e] < l) s_G[own[e]] = g[e];
    }
    __syncthreads();

    int it = 0;
    while (it < max_iter) {
        // ---- ip = argmax of -G over y = +1, alpha < 1;  in = argmax of G over y = -1, alpha > 0 ----
        double vp = -INFINITY, vn = -INFINITY;
        int ip = -1, in = -1;
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                const double a = s_alpha[t], g = s_G[t];
                if (pos[e]) { if (a < 1.0) take_max(vp, ip, -g, t); }
                else { if (a > 0.0) take_max(vn, in, g, t); }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            take_max(vp, ip, __shfl_xor(vp, o, 64), __shfl_xor(ip, o, 64));
            take_max(vn, in, __shfl_xor(vn, o, 64), __shfl_xor(in, o, 64));
        }
        if (lane == 0) { r1_p[wave] = vp; r1_ip[wave] = ip; r1_n[wave] = vn; r1_in[wave] = in; }
        __syncthreads();                                                           // (1)
        vp = r1_p[0]; ip = r1_ip[0]; vn = r1_n[0]; in = r1_in[0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) { take_max(vp, ip, r1_p[w], r1_ip[w]); take_max(vn, in, r1_n[w], r1_in[w]); }
        const double Gmaxp = vp, Gmaxn = vn;                                       // -inf with index -1 where a sign has no candidate

        // rows ip and in, whole: the selection reads each on its own sign's columns, the update the one that becomes i
        const long gp = ip >= 0 ? grow(ip) : 0, gn = in >= 0 ? grow(in) : 0;
        float kp[SMO_PER], kn[SMO_PER];
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            kp[e] = (ip >= 0 && own[e] < l) ? K[gp * ld_k + gown[e]] : 0.f;
            kn[e] = (in >= 0 && own[e] < l) ? K[gn * ld_k + gown[e]] : 0.f;
        }
        const double QD_p = ip >= 0 ? (double)s_diag[ip] : 0.0, QD_n = in >= 0 ? (double)s_diag[in] : 0.0;

        // ---- j = argmin of -b^2 / a inside its own sign, against Q_ip or Q_in;  Gmaxp2 = max G over y = +1, alpha > 0;
        // Gmaxn2 = max -G over y = -1, alpha < 1 ----
        double ov = -INFINITY, gp2 = -INFINITY, gn2 = -INFINITY;                   // ov holds +b^2/a: the largest is libsvm's smallest
        int oj = -1;
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                const float km = pos[e] ? kp[e] : kn[e];
                s_Km[t] = km;
                const double a = s_alpha[t], g = s_G[t];
                if (pos[e] ? a > 0.0 : a < 1.0) {
                    const double gd = pos[e] ? Gmaxp + g : Gmaxn - g;
                    if (pos[e]) gp2 = fmax(gp2, g); else gn2 = fmax(gn2, -g);
                    if (gd > 0.0) {                                                // never with Gmaxp / Gmaxn = -inf
                        double q = (pos[e] ? QD_p : QD_n) + (double)s_diag[t] - 2.0 * (double)km;
                        if (!(q > 0.0)) q = SMO_TAU;
                        take_max(ov, oj, (gd * gd) / q, t);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            take_max(ov, oj, __shfl_xor(ov, o, 64), __shfl_xor(oj, o, 64));
            gp2 = fmax(gp2, __shfl_xor(gp2, o, 64));
            gn2 = fmax(gn2, __shfl_xor(gn2, o, 64));
        }
        if (lane == 0) { r2_v[wave] = ov; r2_i[wave] = oj; r2_p[wave] = gp2; r2_n[wave] = gn2; }
        __syncthreads();                                                           // (2)
        ov = r2_v[0]; oj = r2_i[0]; gp2 = r2_p[0]; gn2 = r2_n[0];
#pragma unroll
        for (int w = 1; w < SMO_WAVES; ++w) { take_max(ov, oj, r2_v[w], r2_i[w]); gp2 = fmax(gp2, r2_p[w]); gn2 = fmax(gn2, r2_n[w]); }
        if (fmax(Gmaxp + gp2, Gmaxn + gn2) < tol || oj < 0) break;                 // block-uniform
        const int j = oj;
        const bool jpos = j < n1;
        const int i = jpos ? ip : in;                                              // >= 0: j was a candidate of that sign

        const long gj = grow(j);
        float kj[SMO_PER];
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) kj[e] = own[e] < l ? K[gj * ld_k + gown[e]] : 0.f;
        const double a_i = s_alpha[i], G_i = s_G[i], a_j = s_alpha[j], G_j = s_G[j];

        // ---- libsvm's equal-sign update with bound 1 (every thread computes the same values) ----
        double q = (jpos ? QD_p : QD_n) + (double)s_diag[j] - 2.0 * (double)s_Km[j];
        if (!(q > 0.0)) q = SMO_TAU;
        const double delta = (G_i - G_j) / q, sum = a_i + a_j;
        double na_i = a_i - delta, na_j = a_j + delta;
        if (sum > 1.0) { if (na_i > 1.0) { na_i = 1.0; na_j = sum - 1.0; } }
        else { if (na_j < 0.0) { na_j = 0.0; na_i = sum; } }
        if (sum > 1.0) { if (na_j > 1.0) { na_j = 1.0; na_i = sum - 1.0; } }
        else { if (na_i < 0.0) { na_i = 0.0; na_j = sum; } }
        const double da_i = na_i - a_i, da_j = na_j - a_j;
        __syncthreads();                                                           // (3) alpha, G, Km of i and j are read everywhere
#pragma unroll
        for (int e = 0; e < SMO_PER; ++e) {
            const int t = own[e];
            if (t < l) {
                if (t == i) s_alpha[t] = na_i;
                if (t == j) s_alpha[t] = na_j;
                const float ki = jpos ? kp[e] : kn[e];
                const bool same = pos[e] == jpos;                                  // y_i = y_j: Q_i[t] = +-K_it, Q_j[t] = +-K_jt
                s_G[t] += (double)(same ? ki : -ki) * da_i + (double)(same ? kj[e] : -kj[e]) * da_j;
            }
        }
        ++it;
        // the next reads of another thread's alpha / G come after barrier (1) of the next iteration
    }
    __syncthreads();

    // ---- Solver_NU::calculate_rho by one thread in libsvm's order (the sums of the free G round as libsvm's), then
    // coef = alpha y / r and rho / r ----
    if (tid == 0) {
        double ub1 = INFINITY, ub2 = INFINITY, lb1 = -INFINITY, lb2 = -INFINITY, sum1 = 0.0, sum2 = 0.0;
        int nf1 = 0, nf2 = 0;
        for (int t = 0; t < l; ++t) {
            const double a = s_alpha[t], g = s_G[t];
            if (t < n1) {
                if (a >= 1.0) lb1 = fmax(lb1, g);
                else if (a <= 0.0) ub1 = fmin(ub1, g);
                else { ++nf1; sum1 += g; }
            } else {
                if (a >= 1.0) lb2 = fmax(lb2, g);
                else if (a <= 0.0) ub2 = fmin(ub2, g);
                else { ++nf2; sum2 += g; }
            }
        }
        const double r1 = nf1 > 0 ? sum1 / nf1 : (ub1 + lb1) / 2, r2 = nf2 > 0 ? sum2 / nf2 : (ub2 + lb2) / 2;
        const double r = (r1 + r2) / 2;
        s_r = r;
        rho[pair] = ((r1 - r2) / 2) / r;
        if (r_out) r_out[pair] = r;
        iters[pair] = it;
    }
    __syncthreads();
    const double r = s_r;
#pragma unroll
    for (int e = 0; e < SMO_PER; ++e) {
        const int t = own[e];
        if (t < l) {
            const double c = s_alpha[t] * ((pos[e] ? 1.0 : -1.0) / r);             // libsvm: alpha[i] *= y[i] / r
            if (t < n1) coef[(long)(cj - 1) * n + gown[e]] = c;                    // libsvm's sv_coef rows: class i's rows against class j
            else coef[(long)ci * n + gown[e]] = c;
        }
    }
}

__global__ __launch_bounds__(SMO_THREADS) void svm_smo_nu_kernel(const float* __restrict__ K, long ld_k, int n, int num_classes,
                                                                 const SvmClasses cls, double nu, double tol, int max_iter,
                                                                 double* __restrict__ coef, double* __restrict__ rho,
                                                                 double* __restrict__ r_out, int* __restrict__ iters) {
    int ci, cj;
    pair_classes(blockIdx.x, num_classes, ci, cj);
    const int s1 = cls.start[ci], n1 = cls.start[ci + 1] - s1, s2 = cls.start[cj], n2 = cls.start[cj + 1] - s2;
    smo_nu_pair(K, ld_k, n, blockIdx.x, ci, cj, s1, n1, s2, n2, nu, tol, max_iter, coef, rho, r_out, iters);
}

// nu differs from item to item (one Gram matrix at several nu is one launch: items may share k, which they only read); tol and
// max_iter are the group's
struct SmoNuItem { const float* k; long ld_k; double* coef; double* rho; double* r; int* iters; double nu; int n; SvmClasses cls; };
struct SmoNuGroup { SmoNuItem item[SVM_MAX_GROUP]; };
static_assert(sizeof(SmoNuGroup) + 32 <= KERNARG_LIMIT, "svm_smo_nu_group_kernel: descriptors beyond the kernel argument limit");

// grid (pairs, count) as svm_smo_group_kernel: count x pairs independent solves, each ending at max_iter
__global__ __launch_bounds__(SMO_THREADS) void svm_smo_nu_group_kernel(const SmoNuGroup g, int num_classes, double tol, int max_iter) {
    const SmoNuItem& d = g.item[blockIdx.y];
    int ci, cj;
    pair_classes(blockIdx.x, num_classes, ci, cj);
    const int s1 = d.cls.start[ci], n1 = d.cls.start[ci + 1] - s1, s2 = d.cls.start[cj], n2 = d.cls.start[cj + 1] - s2;
    smo_nu_pair(d.k, d.ld_k, d.n, blockIdx.x, ci, cj, s1, n1, s2, n2, d.nu, tol, max_iter, d.coef, d.rho, d.r, d.iters);
}

// ---------------------------------------------------------------------------------------------------------------------
// decision values and the vote: one block per test row, a wave per pair (round robin)
// ---------------------------------------------------------------------------------------------------------------------
// test row `row` of one problem by one block: the body of the single and of the grouped kernel
__device__ __forceinline__ void decide_row(const float* __restrict__ Kt, long ld_kt, int n, int num_classes, const SvmClasses& cls,
                                           const double* __restrict__ coef, const double* __restrict__ rho, double* __restrict__ dec,
                                           int* __restrict__ labels, long row) {
    __shared__ double s_dec[SVM_MAX_PAIRS];
    __shared__ int s_votes[SVM_MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pairs = num_classes * (num_classes - 1) / 2;
    const float* kr = Kt + row * ld_kt;
    for (int p = wave; p < pairs; p += 4) {
        int ci, cj;
        pair_classes(p, num_classes, ci, cj);
        const double* c1 = coef + (long)(cj - 1) * n;      // class i's rows against class j
        const double* c2 = coef + (long)ci * n;            // class j's rows against class i
        double s = 0.0;
        for (int t = cls.start[ci] + lane; t < cls.start[ci + 1]; t += 64) s = fma(c1[t], (double)kr[t], s);
        for (int t = cls.start[cj] + lane; t < cls.start[cj + 1]; t += 64) s = fma(c2[t], (double)kr[t], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) s_dec[p] = s - rho[p];
    }
    if (tid < SVM_MAX_CLASSES) s_votes[tid] = 0;
    __syncthreads();
    if (dec)
        for (int p = tid; p < pairs; p += 256) dec[row * pairs + p] = s_dec[p];
    if (tid == 0) {
        int p = 0;
        for (int ci = 0; ci < num_classes; ++ci)
            for (int cj = ci + 1; cj < num_classes; ++cj, ++p) s_votes[s_dec[p] > 0.0 ? ci : cj] += 1;
        int best = 0;
        for (int c = 1; c < num_classes; ++c)
            if (s_votes[c] > s_votes[best]) best = c;       // the first class with the most votes
        labels[row] = best;
    }
}

__global__ __launch_bounds__(256) void svm_decide_kernel(const float* __restrict__ Kt, long ld_kt, int n, int num_classes, const SvmClasses cls,
                                                         const double* __restrict__ coef, const double* __restrict__ rho,
                                                         double* __restrict__ dec, int* __restrict__ labels) {
    decide_row(Kt, ld_kt, n, num_classes, cls, coef, rho, dec, labels, blockIdx.x);
}

struct DecideItem { const float* kt; long ld_kt; const double* coef; const double* rho; double* dec; int* labels; int n; SvmClasses cls; };
// the grid is the concatenation of the items' test rows: item i owns blocks row_start[i] .. row_start[i + 1] - 1
struct DecideGroup { DecideItem item[SVM_MAX_GROUP]; int row_start[SVM_MAX_GROUP + 1]; };
static_assert(sizeof(DecideGroup) + 8 <= KERNARG_LIMIT, "svm_decide_group_kernel: descriptors beyond the kernel argument limit");

__global__ __launch_bounds__(256) void svm_decide_group_kernel(const DecideGroup g, int count, int num_classes) {
    const int bid = blockIdx.x;
    int it = 0;
    while (it + 1 < count && bid >= g.row_start[it + 1]) ++it;        // wave-uniform: blockIdx and arguments only
    const DecideItem& d = g.item[it];
    decide_row(d.kt, d.ld_kt, d.n, num_classes, d.cls, d.coef, d.rho, d.dec, d.labels, bid - g.row_start[it]);
}

int fill_classes(long n, int num_classes, const int64_t* class_start, SvmClasses& cls, const char** err) {
    if (num_classes < 2 || num_classes > SVM_MAX_CLASSES) { *err = "svm: num_classes outside [2, 32]"; return -1; }
    if (!class_start) { *err = "svm: class_start is required"; return -1; }
    if (n < 2 || n > (1 << 24)) { *err = "svm: n outside [2, 2^24]"; return -1; }
    if (class_start[0] != 0 || class_start[num_classes] != n) { *err = "svm: class_start must run from 0 to n"; return -1; }
    for (int c = 0; c < num_classes; ++c) {
        if (class_start[c + 1] <= class_start[c]) { *err = "svm: every class needs at least one row (class_start must increase)"; return -1; }
        cls.start[c] = (int)class_start[c];
    }
    cls.start[num_classes] = (int)n;
    for (int c = num_classes + 1; c <= SVM_MAX_CLASSES; ++c) cls.start[c] = (int)n;
    return 0;
}

// The argument checks of the three entries: a single call makes them on its one problem, a grouped call on every item, before
// any launch.
int check_gram(const float* a, long ld_a, long m, const float* b, long ld_b, long n, long d, float gamma, const float* out, long ld_out,
               int tile, const char** err, int kind = RBF) {
    if (kind != RBF && kind != LINEAR) { *err = "svm_gram: unknown kernel kind (MRGAN_SVM_KERNEL_RBF = 0 or MRGAN_SVM_KERNEL_LINEAR = 1)"; return -1; }
    if (!a || !b || !out) { *err = "svm_gram: null buffer"; return -1; }
    if (m < 1 || n < 1 || d < 1 || m > (1 << 21) || n > (1 << 21) || d > (1 << 24)) { *err = "svm_gram: m, n in [1, 2^21] and d in [1, 2^24]"; return -1; }
    if (ld_a < d || ld_b < d || ld_out < n) { *err = "svm_gram: row pitch smaller than the row"; return -1; }
    if (kind == RBF && (!(gamma > 0.f) || !isfinite(gamma))) { *err = "svm_gram: gamma must be positive and finite"; return -1; }
    if (tile != 0 && tile != 64 && tile != 128) { *err = "svm_gram: tile must be 0, 64 or 128"; return -1; }
    return 0;
}

// what the C-SVC and the nu-SVC solver check alike, in two parts around their own parameter check
int check_solve_buffers(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, const double* coef,
                        const double* rho, const int* iters, SvmClasses& cls, const char** err) {
    if (!k || !coef || !rho || !iters) { *err = "svm_solve: null buffer"; return -1; }
    const int r = fill_classes(n, num_classes, class_start, cls, err);
    if (r) return r;
    if (ld_k < n) { *err = "svm_solve: row pitch smaller than the row"; return -1; }
    return 0;
}

int check_solve_pair_size(int num_classes, const SvmClasses& cls, const char** err) {
    // the two largest classes make the largest pair
    int big1 = 0, big2 = 0;
    for (int c = 0; c < num_classes; ++c) {
        const int sz = cls.start[c + 1] - cls.start[c];
        if (sz > big1) { big2 = big1; big1 = sz; } else if (sz > big2) big2 = sz;
    }
    if (big1 + big2 > SVM_MAX_PAIR) { *err = "svm_solve: a one-vs-one pair has more than MRGAN_SVM_MAX_PAIR = 2048 rows"; return -1; }
    return 0;
}

int check_solve(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double C, double tol, int max_iter,
                const double* coef, const double* rho, const int* iters, SvmClasses& cls, const char** err) {
    const int r = check_solve_buffers(k, ld_k, n, num_classes, class_start, coef, rho, iters, cls, err);
    if (r) return r;
    if (!(C > 0.0) || !isfinite(C) || !(tol > 0.0) || !isfinite(tol) || max_iter < 1) { *err = "svm_solve: C, tol and max_iter must be positive"; return -1; }
    return check_solve_pair_size(num_classes, cls, err);
}

// *bad_i, *bad_j: the classes of the first pair nu is infeasible for (libsvm's svm_check_parameter), else untouched
int check_solve_nu(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double nu, double tol, int max_iter,
                   const double* coef, const double* rho, const int* iters, SvmClasses& cls, const char** err, int* bad_i, int* bad_j) {
    int r = check_solve_buffers(k, ld_k, n, num_classes, class_start, coef, rho, iters, cls, err);
    if (r) return r;
    if (!(nu > 0.0) || !(nu <= 1.0)) { *err = "svm_solve_nu: nu must lie in (0, 1]"; return -1; }
    if (!(tol > 0.0) || !isfinite(tol) || max_iter < 1) { *err = "svm_solve_nu: tol and max_iter must be positive"; return -1; }
    r = check_solve_pair_size(num_classes, cls, err);
    if (r) return r;
    for (int i = 0; i < num_classes; ++i)
        for (int j = i + 1; j < num_classes; ++j) {
            const int ni = cls.start[i + 1] - cls.start[i], nj = cls.start[j + 1] - cls.start[j];
            if (nu * (ni + nj) / 2 > (ni < nj ? ni : nj)) {
                *bad_i = i; *bad_j = j;
                *err = "svm_solve_nu: specified nu is infeasible";
                return -1;
            }
        }
    return 0;
}

int check_decide(const float* kt, long ld_kt, long m, long n, int num_classes, const int64_t* class_start, const double* coef,
                 const double* rho, const int* labels, SvmClasses& cls, const char** err) {
    if (!kt || !coef || !rho || !labels) { *err = "svm_decide: null buffer"; return -1; }
    const int r = fill_classes(n, num_classes, class_start, cls, err);
    if (r) return r;
    if (m < 1 || m > (1 << 24)) { *err = "svm_decide: m outside [1, 2^24]"; return -1; }
    if (ld_kt < n) { *err = "svm_decide: row pitch smaller than the row"; return -1; }
    return 0;
}

// items == null or count outside [1, SVM_MAX_GROUP]: the group's own check (*bad_item stays -1)
int check_group(const void* items, int count, const char* null_msg, const char* count_msg, int* bad_item, const char** err) {
    *bad_item = -1;
    if (!items) { *err = null_msg; return -1; }
    if (count < 1 || count > SVM_MAX_GROUP) { *err = count_msg; return -1; }
    return 0;
}
}  // namespace

int launch_svm_kernel_matrix(int kind, const float* a, long ld_a, long m, const float* b, long ld_b, long n, long d, float gamma, float* out,
                             long ld_out, int tile, hipStream_t s, const char** err) {
    const int r = check_gram(a, ld_a, m, b, ld_b, n, d, gamma, out, ld_out, tile, err, kind);
    if (r) return r;
    // 64x64 blocks while 128x128 ones would leave most CUs without work, as launch_gemm_f32 chooses; every output element is
    // the same k-ordered chain in both
    const bool small = tile ? tile == 64 : (long)ceil_div(n, 128) * ceil_div(m, 128) < 128;
    const dim3 block(256);
    if (small) {
        const dim3 grid(ceil_div(n, 64), ceil_div(m, 64));
        if (kind == RBF) MRGAN_LAUNCH((svm_gram_kernel<64>), grid, block, 0, s, a, ld_a, (int)m, b, ld_b, (int)n, (int)d, gamma, out, ld_out);
        else MRGAN_LAUNCH((svm_gram_kernel<64, LINEAR>), grid, block, 0, s, a, ld_a, (int)m, b, ld_b, (int)n, (int)d, 0.f, out, ld_out);
    } else {
        const dim3 grid(ceil_div(n, 128), ceil_div(m, 128));
        if (kind == RBF) MRGAN_LAUNCH((svm_gram_kernel<128>), grid, block, 0, s, a, ld_a, (int)m, b, ld_b, (int)n, (int)d, gamma, out, ld_out);
        else MRGAN_LAUNCH((svm_gram_kernel<128, LINEAR>), grid, block, 0, s, a, ld_a, (int)m, b, ld_b, (int)n, (int)d, 0.f, out, ld_out);
    }
    if (hipGetLastError() != hipSuccess) { *err = "svm_gram: launch failed"; return -10; }
    return 0;
}

int launch_svm_gram(const float* a, long ld_a, long m, const float* b, long ld_b, long n, long d, float gamma, float* out, long ld_out,
                    int tile, hipStream_t s, const char** err) {
    return launch_svm_kernel_matrix(RBF, a, ld_a, m, b, ld_b, n, d, gamma, out, ld_out, tile, s, err);
}

int launch_svm_solve(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double C, double tol, int max_iter,
                     double* coef, double* rho, int* iters, hipStream_t s, const char** err) {
    SvmClasses cls;
    const int r = check_solve(k, ld_k, n, num_classes, class_start, C, tol, max_iter, coef, rho, iters, cls, err);
    if (r) return r;
    const int pairs = num_classes * (num_classes - 1) / 2;
    MRGAN_LAUNCH(svm_smo_kernel, dim3(pairs), dim3(SMO_THREADS), 0, s, k, ld_k, (int)n, num_classes, cls, C, tol, max_iter, coef, rho, iters);
    if (hipGetLastError() != hipSuccess) { *err = "svm_solve: launch failed"; return -10; }
    return 0;
}

int launch_svm_solve_nu(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double nu, double tol, int max_iter,
                        double* coef, double* rho, double* r_out, int* iters, hipStream_t s, const char** err, int* bad_i, int* bad_j) {
    SvmClasses cls;
    *bad_i = *bad_j = -1;
    const int r = check_solve_nu(k, ld_k, n, num_classes, class_start, nu, tol, max_iter, coef, rho, iters, cls, err, bad_i, bad_j);
    if (r) return r;
    const int pairs = num_classes * (num_classes - 1) / 2;
    MRGAN_LAUNCH(svm_smo_nu_kernel, dim3(pairs), dim3(SMO_THREADS), 0, s, k, ld_k, (int)n, num_classes, cls, nu, tol, max_iter, coef, rho,
                 r_out, iters);
    if (hipGetLastError() != hipSuccess) { *err = "svm_solve_nu: launch failed"; return -10; }
    return 0;
}

int launch_svm_decide(const float* kt, long ld_kt, long m, long n, int num_classes, const int64_t* class_start, const double* coef,
                      const double* rho, double* dec, int* labels, hipStream_t s, const char** err) {
    SvmClasses cls;
    const int r = check_decide(kt, ld_kt, m, n, num_classes, class_start, coef, rho, labels, cls, err);
    if (r) return r;
    MRGAN_LAUNCH(svm_decide_kernel, dim3((unsigned)m), dim3(256), 0, s, kt, ld_kt, (int)n, num_classes, cls, coef, rho, dec, labels);
    if (hipGetLastError() != hipSuccess) { *err = "svm_decide: launch failed"; return -10; }
    return 0;
}

int launch_svm_kernel_matrix_group(int kind, const mrgan_svm_gram_item* items, int count, long d, float gamma, int tile, hipStream_t s,
                                   const char** err, int* bad_item) {
    int r = check_group(items, count, "svm_gram: null item list", "svm_gram: count outside [1, MRGAN_SVM_MAX_GROUP = 16]", bad_item, err);
    if (r) return r;
    long tiles128 = 0;
    for (int i = 0; i < count; ++i) {
        const mrgan_svm_gram_item& it = items[i];
        r = check_gram(it.a_dev, (long)it.ld_a, (long)it.m, it.b_dev, (long)it.ld_b, (long)it.n, d, gamma, it.out_dev, (long)it.ld_out, tile, err, kind);
        if (r) { *bad_item = i; return r; }
        tiles128 += (long)ceil_div(it.n, 128) * ceil_div(it.m, 128);
    }
    // launch_svm_gram's rule on the group's total: one tile size per launch
    const int ts = tile ? tile : (tiles128 < 128 ? 64 : 128);
    GramGroup g = {};
    long total = 0;
    for (int i = 0; i < count; ++i) {
        const mrgan_svm_gram_item& it = items[i];
        g.item[i] = {it.a_dev, it.b_dev, it.out_dev, (long)it.ld_a, (long)it.ld_b, (long)it.ld_out, (int)it.m, (int)it.n};
        g.tile_start[i] = (int)total;
        g.tiles_x[i] = ceil_div(it.n, ts);
        total += (long)g.tiles_x[i] * ceil_div(it.m, ts);
        if (total > 0x7fffffffL) { *bad_item = i; *err = "svm_gram: the group has more than 2^31 - 1 tiles"; return -1; }
    }
    for (int i = count; i <= SVM_MAX_GROUP; ++i) g.tile_start[i] = (int)total;
    for (int i = count; i < SVM_MAX_GROUP; ++i) g.tiles_x[i] = 1;
    const dim3 grid((unsigned)total), block(256);
    if (ts == 64) {
        if (kind == RBF) MRGAN_LAUNCH((svm_gram_group_kernel<64>), grid, block, 0, s, g, count, (int)d, gamma);
        else MRGAN_LAUNCH((svm_gram_group_kernel<64, LINEAR>), grid, block, 0, s, g, count, (int)d, 0.f);
    } else {
        if (kind == RBF) MRGAN_LAUNCH((svm_gram_group_kernel<128>), grid, block, 0, s, g, count, (int)d, gamma);
        else MRGAN_LAUNCH((svm_gram_group_kernel<128, LINEAR>), grid, block, 0, s, g, count, (int)d, 0.f);
    }
    if (hipGetLastError() != hipSuccess) { *err = "svm_gram: group launch failed"; return -10; }
    return 0;
}

int launch_svm_gram_group(const mrgan_svm_gram_item* items, int count, long d, float gamma, int tile, hipStream_t s, const char** err,
                          int* bad_item) {
    return launch_svm_kernel_matrix_group(RBF, items, count, d, gamma, tile, s, err, bad_item);
}

int launch_svm_solve_group(const mrgan_svm_solve_item* items, int count, int num_classes, double C, double tol, int max_iter, hipStream_t s,
                           const char** err, int* bad_item) {
    int r = check_group(items, count, "svm_solve: null item list", "svm_solve: count outside [1, MRGAN_SVM_MAX_GROUP = 16]", bad_item, err);
    if (r) return r;
    SmoGroup g = {};
    for (int i = 0; i < count; ++i) {
        const mrgan_svm_solve_item& it = items[i];
        r = check_solve(it.k_dev, (long)it.ld_k, (long)it.n, num_classes, it.class_start_host, C, tol, max_iter, it.coef_dev, it.rho_dev,
                        it.iters_dev, g.item[i].cls, err);
        if (r) { *bad_item = i; return r; }
        g.item[i].k = it.k_dev; g.item[i].ld_k = (long)it.ld_k; g.item[i].coef = it.coef_dev; g.item[i].rho = it.rho_dev;
        g.item[i].iters = it.iters_dev; g.item[i].n = (int)it.n;
    }
    const int pairs = num_classes * (num_classes - 1) / 2;
    MRGAN_LAUNCH(svm_smo_group_kernel, dim3(pairs, count), dim3(SMO_THREADS), 0, s, g, num_classes, C, tol, max_iter);
    if (hipGetLastError() != hipSuccess) { *err = "svm_solve: group launch failed"; return -10; }
    return 0;
}

int launch_svm_solve_nu_group(const mrgan_svm_solve_nu_item* items, int count, int num_classes, double tol, int max_iter, hipStream_t s,
                              const char** err, int* bad_item, int* bad_i, int* bad_j) {
    *bad_i = *bad_j = -1;
    int r = check_group(items, count, "svm_solve_nu: null item list", "svm_solve_nu: count outside [1, MRGAN_SVM_MAX_GROUP = 16]", bad_item, err);
    if (r) return r;
    SmoNuGroup g = {};
    for (int i = 0; i < count; ++i) {
        const mrgan_svm_solve_nu_item& it = items[i];
        r = check_solve_nu(it.k_dev, (long)it.ld_k, (long)it.n, num_classes, it.class_start_host, it.nu, tol, max_iter, it.coef_dev, it.rho_dev,
                           it.iters_dev, g.item[i].cls, err, bad_i, bad_j);
        if (r) { *bad_item = i; return r; }
        g.item[i].k = it.k_dev; g.item[i].ld_k = (long)it.ld_k; g.item[i].coef = it.coef_dev; g.item[i].rho = it.rho_dev;
        g.item[i].r = it.r_dev; g.item[i].iters = it.iters_dev; g.item[i].nu = it.nu; g.item[i].n = (int)it.n;
    }
    const int pairs = num_classes * (num_classes - 1) / 2;
    MRGAN_LAUNCH(svm_smo_nu_group_kernel, dim3(pairs, count), dim3(SMO_THREADS), 0, s, g, num_classes, tol, max_iter);
    if (hipGetLastError() != hipSuccess) { *err = "svm_solve_nu: group launch failed"; return -10; }
    return 0;
}

int launch_svm_decide_group(const mrgan_svm_decide_item* items, int count, int num_classes, hipStream_t s, const char** err, int* bad_item) {
    int r = check_group(items, count, "svm_decide: null item list", "svm_decide: count outside [1, MRGAN_SVM_MAX_GROUP = 16]", bad_item, err);
    if (r) return r;
    DecideGroup g = {};
    long total = 0;
    for (int i = 0; i < count; ++i) {
        const mrgan_svm_decide_item& it = items[i];
        r = check_decide(it.kt_dev, (long)it.ld_kt, (long)it.m, (long)it.n, num_classes, it.class_start_host, it.coef_dev, it.rho_dev,
                         it.labels_dev, g.item[i].cls, err);
        if (r) { *bad_item = i; return r; }
        g.item[i].kt = it.kt_dev; g.item[i].ld_kt = (long)it.ld_kt; g.item[i].coef = it.coef_dev; g.item[i].rho = it.rho_dev;
        g.item[i].dec = it.dec_dev; g.item[i].labels = it.labels_dev; g.item[i].n = (int)it.n;
        g.row_start[i] = (int)total;
        total += (long)it.m;                                 // <= 16 * 2^24
    }
    for (int i = count; i <= SVM_MAX_GROUP; ++i) g.row_start[i] = (int)total;
    MRGAN_LAUNCH(svm_decide_group_kernel, dim3((unsigned)total), dim3(256), 0, s, g, count, num_classes);
    if (hipGetLastError() != hipSuccess) { *err = "svm_decide: group launch failed"; return -10; }
    return 0;
}

}  // namespace mrgan
