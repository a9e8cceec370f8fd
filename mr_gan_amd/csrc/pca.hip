// PCA on the device: what decomposition.PCA(n_components) of the reference's pcaScale (others/wganlpctsemi.py:129-139) computes,
// exact to a stated residual.
//
//   pca_mean_kernel        column means: fp64 sums in a fixed order, rounded once to fp32.
//   pca_cov_kernel         C = (X - mu)^T (X - mu) / (n - 1).  The reduction runs over ROWS, so the k-major LDS image [k][column] of
//                          svm_gram_kernel is a coalesced read of X[k0 : k0 + BK, block columns]; mu[column] is subtracted while
//                          staging (centring in the operands), padded rows and columns stage 0.  The product is the k-ordered
//                          v_mfma_f32_32x32x2_f32 chain of svm_gram_kernel (same fragments).  Only the tiles on and below the
//                          diagonal are computed; the row range is split across blockIdx.z into slabs of the caller's workspace.
//   pca_cov_reduce_kernel  sums the slabs of a tile in split order, divides by n - 1 and writes C[i, j] and C[j, i] from the one
//                          value (i >= j): symmetric bit for bit, no atomics, identical bits from run to run.
//   block iteration        (launch_pca_eig, host loop) Y = Q C by svm_gram_kernel<LINEAR> (C is symmetric), pca_rayleigh_kernel
//                          (theta_j = q_j . y_j, |y_j - theta_j q_j|, fp64 from the fp32 operands), one readback of 2 p + 1 doubles,
//                          then the orthonormalisation by the small SVD route, stable for an ill-conditioned Y:
//                            pca_yyt_kernel     S = Y Y^T, p x p, fp64
//                            pca_jacobi_kernel  cyclic Jacobi on S in ONE workgroup, S and V in LDS (fp64, <= 102 KB at p = 80),
//                                               round-robin pairs: p / 2 disjoint rotations per step; every loop is bounded
//                            pca_apply_kernel   Q = Lambda^-1/2 V^T Y, rows by descending Lambda; Lambda_j <= 2^-40 Lambda_1: zero row
//                          Nothing spins on the device and no block waits for another.
//   pca_finalize_kernel    the first k rows by descending theta, each with its largest-magnitude entry positive (first index on
//                          ties: scikit-learn's svd_flip(u_based_decision=False)).
//   pca_transform_kernel   (X - mu) W^T: a wave per four rows, lanes stride the features, one butterfly per value: a row's bits
//                          depend on that row alone.
//   pca_inverse_kernel     Z W + mu: a thread per column, the k-ordered fmaf chain.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "pca.h"
#include "svm.h"

namespace mrgan {

namespace {
constexpr int BK = 16;

// ---------------------------------------------------------------------------------------------------------------------
// mean
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MEAN_COLS = 32, MEAN_GROUPS = 32, MEAN_THREADS = MEAN_COLS * MEAN_GROUPS;

// block = 32 columns x 32 row groups: group g sums rows g, g + 32, .. in fp64 (two interleaved partial sums, so two loads are
// in flight), the groups are added in order
__global__ __launch_bounds__(MEAN_THREADS) void pca_mean_kernel(const float* __restrict__ x, long ld_x, int n, int d, float* __restrict__ mean) {
    __shared__ double part[MEAN_GROUPS][MEAN_COLS];
    const int tx = threadIdx.x % MEAN_COLS, g = threadIdx.x / MEAN_COLS, col = blockIdx.x * MEAN_COLS + tx;
    double s0 = 0.0, s1 = 0.0;
    if (col < d) {
        int r = g;
        for (; r + MEAN_GROUPS < n; r += 2 * MEAN_GROUPS) {
            s0 += (double)x[(long)r * ld_x + col];
            s1 += (double)x[(long)(r + MEAN_GROUPS) * ld_x + col];
        }
        if (r < n) s0 += (double)x[(long)r * ld_x + col];
    }
    part[g][tx] = s0 + s1;
    __syncthreads();
    if (g == 0 && col < d) {
        double tot = part[0][tx];
        for (int q = 1; q < MEAN_GROUPS; ++q) tot += part[q][tx];
        mean[col] = (float)(tot / (double)n);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// covariance
// ---------------------------------------------------------------------------------------------------------------------
// tiles on and below the diagonal, row-major: tile (ti, tj <= ti) is number ti (ti + 1) / 2 + tj
__device__ __host__ inline long lower_tile(int ti, int tj) { return (long)ti * (ti + 1) / 2 + tj; }

// one TS x TS tile of (X - mu)^T (X - mu) over the rows [r_begin, r_end) into its slab: rows of the tile are the columns
// ti * TS .. of X, columns of the tile the columns tj * TS .. of X.  The whole tile is written (padding holds zeros).
template <int TS>
__global__ __launch_bounds__(256) void pca_cov_kernel(const float* __restrict__ X, long ld_x, int n, int d, const float* __restrict__ mean,
                                                      float* __restrict__ slabs, int rows_per_split) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;                                     // block-uniform: the upper tiles are the mirror of the lower ones
    constexpr int LDT = TS, MR = TS / 64, KPT = TS / 16;      // KPT: k values staged per thread
    __shared__ __attribute__((aligned(16))) float lds[2 * BK * TS];
    float* As = lds;
    float* Bs = lds + BK * LDT;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r_begin = blockIdx.z * rows_per_split, r_end = min(n, r_begin + rows_per_split);

    // staging map: thread -> (column t % TS of the tile, KPT consecutive rows of X starting at (t / TS) * KPT): a wave reads 64
    // consecutive floats of one row of X per load
    const int si = t % TS, sk = (t / TS) * KPT;
    const int ca = ti * TS + si, cb = tj * TS + si;
    const bool a_ok = ca < d, b_ok = cb < d;
    const float ma = a_ok ? mean[ca] : 0.f, mb = b_ok ? mean[cb] : 0.f;

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
            const int r = k0 + sk + j;
            const bool ok = r < r_end;
            ra[j] = (a_ok && ok) ? X[(long)r * ld_x + ca] - ma : 0.f;
            rb[j] = (b_ok && ok) ? X[(long)r * ld_x + cb] - mb : 0.f;
        }
    };

    load_tile(r_begin);
    for (int k0 = r_begin; k0 < r_end; k0 += BK) {
        __syncthreads();                 // previous tile's fragment reads done
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            As[(sk + j) * LDT + si] = ra[j];
            Bs[(sk + j) * LDT + si] = rb[j];
        }
        __syncthreads();
        if (k0 + BK < r_end) load_tile(k0 + BK);      // in flight under the MFMAs below
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

    const long tiles = lower_tile(gridDim.y - 1, gridDim.y - 1) + 1;
    float* slab = slabs + ((long)blockIdx.z * tiles + lower_tile(ti, tj)) * (TS * TS);
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < MR; ++mi)
#pragma unroll
        for (int ni = 0; ni < MR; ++ni) {
            const int lc = (wn * MR + ni) * 32 + lr;
#pragma unroll
            for (int r = 0; r < 16; ++r) slab[((wm * MR + mi) * 32 + acc_row(r, lh)) * TS + lc] = acc[mi][ni][r];
        }
}

template <int TS>
__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const float* __restrict__ slabs, int splits, int n, int d, float* __restrict__ cov,
                                                             long ld_cov) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    const long tiles = lower_tile(gridDim.y - 1, gridDim.y - 1) + 1;
    const float* slab = slabs + lower_tile(ti, tj) * (TS * TS);
    const float denom = (float)(n - 1);                      // exact: n <= 2^24
    for (int e = threadIdx.x; e < TS * TS; e += 256) {
        const int gi = ti * TS + e / TS, gj = tj * TS + e % TS;
        if (gi >= d || gj > gi) continue;                     // (gj <= gi < d)
        float v = slab[e];
        for (int s = 1; s < splits; ++s) v += slab[(long)s * tiles * (TS * TS) + e];
        v /= denom;
        cov[(long)gi * ld_cov + gj] = v;
        cov[(long)gj * ld_cov + gi] = v;
    }
}

struct CovPlan { int ts, nt, splits, rows_per_split; long tiles; };

// the tile and the row split of a covariance launch (tile, split: 0 = from the shape); n, d already checked
CovPlan cov_plan(long n, long d, int tile, int split) {
    CovPlan p;
    p.ts = tile ? tile : (d <= 256 ? 64 : 128);
    p.nt = ceil_div(d, p.ts);
    p.tiles = lower_tile(p.nt - 1, p.nt - 1) + 1;
    // about two blocks per CU of the 256, at least 64 rows per block; a forced split: at most one range per BK rows
    long want = split ? split : std::min<long>(32, std::min<long>(ceil_div(512, p.tiles), std::max<long>(1, n / 64)));
    want = std::max<long>(1, std::min<long>(want, ceil_div(n, BK)));
    p.rows_per_split = (int)round_up(ceil_div(n, want), BK);
    p.splits = ceil_div(n, p.rows_per_split);
    return p;
}

int check_cov_shape(long n, long d, int tile, int split, const char** err) {
    if (n < 2 || n > (1 << 24)) { *err = "pca_covariance: n outside [2, 2^24]"; return -1; }
    if (d < 1 || d > PCA_MAX_FEATURES) { *err = "pca_covariance: d outside [1, MRGAN_PCA_MAX_FEATURES = 4096]"; return -1; }
    if (tile != 0 && tile != 64 && tile != 128) { *err = "pca_covariance: tile must be 0, 64 or 128"; return -1; }
    if (split < 0 || split > 4096) { *err = "pca_covariance: split outside [0, 4096]"; return -1; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// block iteration
// ---------------------------------------------------------------------------------------------------------------------
// a block-wide fp64 sum in a fixed order (lanes by butterfly, the four waves in order); every thread gets the total
__device__ __forceinline__ double block_sum256(double v, double* scratch) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                          // scratch is free again
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// row j: theta_j = q_j . y_j and |y_j - theta_j q_j|_2 -> status[j], status[p + j]
__global__ __launch_bounds__(256) void pca_rayleigh_kernel(const float* __restrict__ Q, const float* __restrict__ Y, int d, int p,
                                                           double* __restrict__ status) {
    __shared__ double scratch[4];
    const int j = blockIdx.x;
    const float* q = Q + (long)j * d;
    const float* y = Y + (long)j * d;
    double s = 0.0;
    for (int c = threadIdx.x; c < d; c += 256) s = fma((double)q[c], (double)y[c], s);
    const double theta = block_sum256(s, scratch);
    double r = 0.0;
    for (int c = threadIdx.x; c < d; c += 256) {
        const double e = (double)y[c] - theta * (double)q[c];
        r = fma(e, e, r);
    }
    r = block_sum256(r, scratch);
    if (threadIdx.x == 0) { status[j] = theta; status[p + j] = sqrt(r); }
}

// S = Y Y^T: block i, its waves take the j <= i round robin
__global__ __launch_bounds__(256) void pca_yyt_kernel(const float* __restrict__ Y, long ld_y, int d, int p, double* __restrict__ S) {
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* yi = Y + (long)i * ld_y;
    for (int j = wave; j <= i; j += 4) {
        const float* yj = Y + (long)j * ld_y;
        double s = 0.0;
        for (int c = lane; c < d; c += 64) s = fma((double)yi[c], (double)yj[c], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) { S[(long)i * p + j] = s; S[(long)j * p + i] = s; }
    }
}

constexpr int JACOBI_THREADS = 1024, JACOBI_MAX_SWEEPS = 60;
constexpr double JACOBI_EPS = 2.220446049250313e-16;          // 2^-52: a rotation is skipped when |s_ab| <= eps sqrt(s_aa s_bb)
constexpr double RANK_FLOOR = 9.094947017729282e-13;          // 2^-40

// round-robin schedule over m (even) players: step in [0, m - 1), slot i in [0, m / 2) -> the disjoint pair (a, b)
__device__ __forceinline__ void jacobi_pair(int step, int i, int m, int& a, int& b) {
    a = (step + i) % (m - 1);
    b = i == 0 ? m - 1 : (step - i + (m - 1)) % (m - 1);
}

inline long jacobi_lds_bytes(int p) { return 2L * p * (p | 1) * (long)sizeof(double); }

// S = V Lambda V^T by cyclic Jacobi (Golub & Van Loan 8.4) in one workgroup; then M = Lambda^-1/2 V^T with its rows sorted by
// descending Lambda (zero rows where Lambda_j <= 2^-40 Lambda_1), lam = the sorted Lambda, *nvalid = the number of nonzero rows
__global__ __launch_bounds__(JACOBI_THREADS) void pca_jacobi_kernel(const double* __restrict__ S, int p, double* __restrict__ M,
                                                                    double* __restrict__ lam, double* __restrict__ nvalid) {
    extern __shared__ __attribute__((aligned(16))) double jl[];
    __shared__ double rc[PCA_MAX_BLOCK / 2], rs[PCA_MAX_BLOCK / 2], ev[PCA_MAX_BLOCK], scale[PCA_MAX_BLOCK];
    __shared__ int src_of[PCA_MAX_BLOCK];
    __shared__ int rotated;
    const int P = p | 1;                                      // odd pitch: a column walk touches every bank
    double* A = jl;
    double* V = jl + (long)p * P;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < p * p; idx += JACOBI_THREADS) {
        const int r = idx / p, c = idx - r * p;
        A[r * P + c] = S[idx];
        V[r * P + c] = r == c ? 1.0 : 0.0;
    }
    const int m = (p + 1) & ~1, npairs = m / 2;               // an odd p plays with a bye
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        if (tid == 0) rotated = 0;
        __syncthreads();
        for (int step = 0; step < m - 1; ++step) {
            if (tid < npairs) {
                int a, b;
                jacobi_pair(step, tid, m, a, b);
                double c = 1.0, s = 0.0;
                if (a < p && b < p) {
                    const double app = A[a * P + a], aqq = A[b * P + b], apq = A[a * P + b];
                    if (apq != 0.0 && fabs(apq) > JACOBI_EPS * sqrt(fabs(app * aqq))) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + tt * tt);
                        s = tt * c;
                        atomicAdd(&rotated, 1);
                    }
                }
                rc[tid] = c; rs[tid] = s;
            }
            __syncthreads();
            // S J and V J: the pairs' columns are disjoint
            for (int idx = tid; idx < npairs * p; idx += JACOBI_THREADS) {
                const int pr = idx / p, r = idx - pr * p;
                const double s = rs[pr];
                if (s == 0.0) continue;
                const double c = rc[pr];
                int a, b;
                jacobi_pair(step, pr, m, a, b);
                const double x = A[r * P + a], y = A[r * P + b];
                A[r * P + a] = c * x - s * y; A[r * P + b] = s * x + c * y;
                const double vx = V[r * P + a], vy = V[r * P + b];
                V[r * P + a] = c * vx - s * vy; V[r * P + b] = s * vx + c * vy;
            }
            __syncthreads();
            // J^T (S J): the pairs' rows are disjoint
            for (int idx = tid; idx < npairs * p; idx += JACOBI_THREADS) {
                const int pr = idx / p, r = idx - pr * p;
                const double s = rs[pr];
                if (s == 0.0) continue;
                const double c = rc[pr];
                int a, b;
                jacobi_pair(step, pr, m, a, b);
                const double x = A[a * P + r], y = A[b * P + r];
                A[a * P + r] = c * x - s * y; A[b * P + r] = s * x + c * y;
            }
            __syncthreads();
        }
        const int any = rotated;
        __syncthreads();                                      // everyone has read it before the next sweep clears it
        if (!any) break;                                      // block-uniform
    }
    if (tid < p) ev[tid] = A[tid * P + tid];
    __syncthreads();
    if (tid < p) {
        const double mine = ev[tid];
        double top = ev[0];
        int rank = 0;
        for (int i = 0; i < p; ++i) {
            const double o = ev[i];
            top = fmax(top, o);
            if (o > mine || (o == mine && i < tid)) ++rank;
        }
        const bool valid = mine > 0.0 && mine > RANK_FLOOR * top;
        lam[rank] = mine;
        src_of[rank] = tid;
        scale[rank] = valid ? 1.0 / sqrt(mine) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int i = 0; i < p; ++i) cnt += scale[i] != 0.0 ? 1 : 0;
        *nvalid = (double)cnt;
    }
    for (int idx = tid; idx < p * p; idx += JACOBI_THREADS) {
        const int r = idx / p, i = idx - r * p;
        M[idx] = V[i * P + src_of[r]] * scale[r];
    }
}

// Q[j, c] = sum_i M[j, i] Y[i, c] in fp64, rounded once: block (column chunk, row j)
__global__ __launch_bounds__(256) void pca_apply_kernel(const double* __restrict__ M, const float* __restrict__ Y, long ld_y, int d, int p,
                                                        float* __restrict__ Q, long ld_q) {
    const int c = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (c >= d) return;
    const double* mj = M + (long)j * p;
    double s = 0.0;
    for (int i = 0; i < p; ++i) s = fma(mj[i], (double)Y[(long)i * ld_y + c], s);
    Q[(long)j * ld_q + c] = (float)s;
}

struct PcaOrder { int src[PCA_MAX_COMPONENTS]; };            // by value in the kernel arguments

// output row r = row order.src[r] of Q with the sign that makes its largest-magnitude entry (first index on ties) positive
__global__ __launch_bounds__(256) void pca_finalize_kernel(const float* __restrict__ Q, int d, const PcaOrder order, float* __restrict__ W,
                                                           long ld_w) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    __shared__ float sign;
    const float* q = Q + (long)order.src[blockIdx.x] * d;
    float best = -1.f;
    int at = 0;
    for (int c = threadIdx.x; c < d; c += 256) {
        const float v = fabsf(q[c]);
        if (v > best) { best = v; at = c; }                   // ascending c: the first index of the thread's maximum
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t)
            if (bv[t] > best || (bv[t] == best && bi[t] < at)) { best = bv[t]; at = bi[t]; }
        sign = q[at] < 0.f ? -1.f : 1.f;
    }
    __syncthreads();
    const float sg = sign;
    for (int c = threadIdx.x; c < d; c += 256) W[(long)blockIdx.x * ld_w + c] = sg * q[c];
}

// the parts of the eigen stage's workspace, doubles first
struct EigWork { double *S, *M, *lam, *status; float *Q, *Y; };
EigWork eig_work(void* work, long d, long p) {
    EigWork w;
    w.S = (double*)work;
    w.M = w.S + p * p;
    w.lam = w.M + p * p;
    w.status = w.lam + p;                                     // theta [p], residual [p], the surviving directions [1]
    w.Q = (float*)(w.status + 2 * p + 2);
    w.Y = w.Q + p * d;
    return w;
}

DeviceOnce jacobi_once;

int orthonormalize(const float* y, long ld_y, int p, int d, double* S, double* M, double* lam, double* nvalid, float* q, long ld_q,
                   hipStream_t s, const char** err) {
    const long lds = jacobi_lds_bytes(p);
    if (jacobi_once.first()) {
        if (hipFuncSetAttribute((const void*)pca_jacobi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)jacobi_lds_bytes(PCA_MAX_BLOCK)) != hipSuccess) {
            *err = "pca_eig: the Jacobi kernel's LDS limit could not be raised";
            return -10;
        }
        jacobi_once.mark();
    }
    MRGAN_LAUNCH(pca_yyt_kernel, dim3(p), dim3(256), 0, s, y, ld_y, d, p, S);
    MRGAN_LAUNCH(pca_jacobi_kernel, dim3(1), dim3(JACOBI_THREADS), (size_t)lds, s, (const double*)S, p, M, lam, nvalid);
    MRGAN_LAUNCH(pca_apply_kernel, dim3(ceil_div(d, 256), p), dim3(256), 0, s, (const double*)M, y, ld_y, d, p, q, ld_q);
    if (hipGetLastError() != hipSuccess) { *err = "pca_eig: orthonormalisation launch failed"; return -10; }
    return 0;
}

int check_block(long p, long d, const char** err) {
    if (d < 1 || d > PCA_MAX_FEATURES) { *err = "pca_eig: d outside [1, MRGAN_PCA_MAX_FEATURES = 4096]"; return -1; }
    if (p < 1 || p > PCA_MAX_BLOCK || p > d) { *err = "pca_eig: block width p outside [1, min(d, 80)]"; return -1; }
    return 0;
}
}  // namespace

int launch_pca_mean(const float* x, long ld_x, long n, long d, float* mean, hipStream_t s, const char** err) {
    if (!x || !mean) { *err = "pca_mean: null buffer"; return -1; }
    if (n < 1 || n > (1 << 24) || d < 1 || d > (1 << 24)) { *err = "pca_mean: n, d outside [1, 2^24]"; return -1; }
    if (ld_x < d) { *err = "pca_mean: row pitch smaller than the row"; return -1; }
    MRGAN_LAUNCH(pca_mean_kernel, dim3(ceil_div(d, MEAN_COLS)), dim3(MEAN_THREADS), 0, s, x, ld_x, (int)n, (int)d, mean);
    if (hipGetLastError() != hipSuccess) { *err = "pca_mean: launch failed"; return -10; }
    return 0;
}

long pca_covariance_workspace_bytes(long n, long d, int tile, int split) {
    const char* err = "";
    if (check_cov_shape(n, d, tile, split, &err)) return -1;
    const CovPlan p = cov_plan(n, d, tile, split);
    return (long)p.splits * p.tiles * p.ts * p.ts * (long)sizeof(float);
}

int launch_pca_covariance(const float* x, long ld_x, long n, long d, const float* mean, float* cov, long ld_cov, void* work,
                          long work_bytes, int tile, int split, hipStream_t s, const char** err) {
    if (!x || !mean || !cov || !work) { *err = "pca_covariance: null buffer"; return -1; }
    const int r = check_cov_shape(n, d, tile, split, err);
    if (r) return r;
    if (ld_x < d || ld_cov < d) { *err = "pca_covariance: row pitch smaller than the row"; return -1; }
    const CovPlan p = cov_plan(n, d, tile, split);
    if (work_bytes < (long)p.splits * p.tiles * p.ts * p.ts * (long)sizeof(float)) {
        *err = "pca_covariance: workspace smaller than mrgan_pca_covariance_workspace_bytes";
        return -1;
    }
    const dim3 grid(p.nt, p.nt, p.splits), rgrid(p.nt, p.nt), block(256);
    if (p.ts == 64) {
        MRGAN_LAUNCH(pca_cov_kernel<64>, grid, block, 0, s, x, ld_x, (int)n, (int)d, mean, (float*)work, p.rows_per_split);
        MRGAN_LAUNCH(pca_cov_reduce_kernel<64>, rgrid, block, 0, s, (const float*)work, p.splits, (int)n, (int)d, cov, ld_cov);
    } else {
        MRGAN_LAUNCH(pca_cov_kernel<128>, grid, block, 0, s, x, ld_x, (int)n, (int)d, mean, (float*)work, p.rows_per_split);
        MRGAN_LAUNCH(pca_cov_reduce_kernel<128>, rgrid, block, 0, s, (const float*)work, p.splits, (int)n, (int)d, cov, ld_cov);
    }
    if (hipGetLastError() != hipSuccess) { *err = "pca_covariance: launch failed"; return -10; }
    return 0;
}

long pca_eig_workspace_bytes(long d, long p) {
    const char* err = "";
    if (check_block(p, d, &err)) return -1;
    return (2 * p * p + 3 * p + 2) * (long)sizeof(double) + 2 * p * d * (long)sizeof(float);      // eig_work's parts
}

int launch_pca_orthonormalize(const float* y, long ld_y, long p, long d, void* work, long work_bytes, float* q, long ld_q, double* lam,
                              hipStream_t s, const char** err) {
    if (!y || !work || !q || !lam) { *err = "pca_orthonormalize: null buffer"; return -1; }
    const int r = check_block(p, d, err);
    if (r) return r;
    if (ld_y < d || ld_q < d) { *err = "pca_orthonormalize: row pitch smaller than the row"; return -1; }
    if (((uintptr_t)work & 7) || work_bytes < pca_eig_workspace_bytes(d, p)) {
        *err = "pca_orthonormalize: workspace misaligned or smaller than mrgan_pca_eig_workspace_bytes";
        return -1;
    }
    const EigWork w = eig_work(work, d, p);
    return orthonormalize(y, ld_y, (int)p, (int)d, w.S, w.M, lam, w.status + 2 * p, q, ld_q, s, err);
}

int launch_pca_eig(const float* cov, long ld_cov, long d, long k, const float* q0, long ld_q0, long p, double tol, int max_iter, void* work,
                   long work_bytes, float* components, long ld_w, double* values_host, double* residuals_host, int* iters_host,
                   hipStream_t s, const char** err) {
    if (!cov || !q0 || !work || !components || !values_host || !residuals_host || !iters_host) { *err = "pca_eig: null buffer"; return -1; }
    int r = check_block(p, d, err);
    if (r) return r;
    if (k < 1 || k > PCA_MAX_COMPONENTS || k > d) { *err = "pca_eig: k outside [1, min(d, MRGAN_PCA_MAX_COMPONENTS = 64)]"; return -1; }
    if (p != std::min<long>(d, k + PCA_GUARD)) { *err = "pca_eig: p must be min(d, k + MRGAN_PCA_GUARD)"; return -1; }
    if (ld_cov < d || ld_q0 < d || ld_w < d) { *err = "pca_eig: row pitch smaller than the row"; return -1; }
    if (!(tol > 0.0) || !isfinite(tol) || max_iter < 1) { *err = "pca_eig: tol and max_iter must be positive"; return -1; }
    if (((uintptr_t)work & 7) || work_bytes < pca_eig_workspace_bytes(d, p)) {
        *err = "pca_eig: workspace misaligned or smaller than mrgan_pca_eig_workspace_bytes";
        return -1;
    }
    const EigWork w = eig_work(work, d, p);
    const int P = (int)p, D = (int)d, K = (int)k;
    double* nvalid = w.status + 2 * p;
    r = orthonormalize(q0, ld_q0, P, D, w.S, w.M, w.lam, nvalid, w.Q, d, s, err);
    if (r) return r;
    double host[2 * PCA_MAX_BLOCK + 1];
    *iters_host = 0;
    for (int it = 1; it <= max_iter; ++it) {
        // Y^T = Q C: C is symmetric, so row j of Y is the linear Gram of q_j against the rows of C
        r = launch_svm_kernel_matrix(MRGAN_SVM_KERNEL_LINEAR, w.Q, d, p, cov, ld_cov, d, d, 0.f, w.Y, d, 0, s, err);
        if (r) return r;
        MRGAN_LAUNCH(pca_rayleigh_kernel, dim3(P), dim3(256), 0, s, (const float*)w.Q, (const float*)w.Y, D, P, w.status);
        if (hipGetLastError() != hipSuccess) { *err = "pca_eig: launch failed"; return -10; }
        if (hipMemcpyAsync(host, w.status, (size_t)(2 * P + 1) * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            *err = "pca_eig: the convergence readback failed";
            return -10;
        }
        *iters_host = it;
        if (host[2 * P] < (double)K) { *err = "pca_eig: numerical rank below n_components"; return PCA_RANK_ERROR; }
        double theta_max = 0.0, res_max = 0.0;
        for (int j = 0; j < K; ++j) { theta_max = fmax(theta_max, host[j]); res_max = fmax(res_max, host[P + j]); }
        if (res_max <= tol * theta_max || it == max_iter) break;
        r = orthonormalize(w.Y, d, P, D, w.S, w.M, w.lam, nvalid, w.Q, d, s, err);
        if (r) return r;
    }
    // the first k rows by descending theta (stable), their signs on the device
    PcaOrder order;
    for (int j = 0; j < PCA_MAX_COMPONENTS; ++j) order.src[j] = j < K ? j : 0;
    for (int a = 1; a < K; ++a) {
        const int v = order.src[a];
        int b = a;
        while (b > 0 && host[order.src[b - 1]] < host[v]) { order.src[b] = order.src[b - 1]; --b; }
        order.src[b] = v;
    }
    for (int j = 0; j < K; ++j) { values_host[j] = host[order.src[j]]; residuals_host[j] = host[P + order.src[j]]; }
    MRGAN_LAUNCH(pca_finalize_kernel, dim3(K), dim3(256), 0, s, (const float*)w.Q, D, order, components, ld_w);
    if (hipGetLastError() != hipSuccess) { *err = "pca_eig: launch failed"; return -10; }
    return 0;
}

namespace {
constexpr int TR_ROWS = 4, TR_JB = 16;       // rows per wave, components per pass

__global__ __launch_bounds__(256) void pca_transform_kernel(const float* __restrict__ x, long ld_x, int m, int d, const float* __restrict__ mean,
                                                            const float* __restrict__ w, long ld_w, int k, float* __restrict__ out, long ld_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = ((long)blockIdx.x * 4 + wave) * TR_ROWS;
    if (row0 >= m) return;                                    // wave-uniform
    for (int jb = 0; jb < k; jb += TR_JB) {
        float acc[TR_ROWS][TR_JB];
#pragma unroll
        for (int r = 0; r < TR_ROWS; ++r)
#pragma unroll
            for (int jj = 0; jj < TR_JB; ++jj) acc[r][jj] = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float mu = mean[c];
            float xv[TR_ROWS];
#pragma unroll
            for (int r = 0; r < TR_ROWS; ++r) xv[r] = row0 + r < m ? x[(row0 + r) * ld_x + c] - mu : 0.f;
#pragma unroll
            for (int jj = 0; jj < TR_JB; ++jj) {
                const float wv = jb + jj < k ? w[(long)(jb + jj) * ld_w + c] : 0.f;
#pragma unroll
                for (int r = 0; r < TR_ROWS; ++r) acc[r][jj] = fmaf(xv[r], wv, acc[r][jj]);
            }
        }
#pragma unroll
        for (int r = 0; r < TR_ROWS; ++r)
#pragma unroll
            for (int jj = 0; jj < TR_JB; ++jj) {
                float v = acc[r][jj];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == jj && row0 + r < m && jb + jj < k) out[(row0 + r) * ld_out + jb + jj] = v;
            }
    }
}

constexpr int INV_ROWS = 8;

__global__ __launch_bounds__(256) void pca_inverse_kernel(const float* __restrict__ z, long ld_z, int m, int k, const float* __restrict__ w,
                                                          long ld_w, int d, const float* __restrict__ mean, float* __restrict__ out, long ld_out) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= d) return;
    const float mu = mean[c];
    for (int r = 0; r < INV_ROWS; ++r) {
        const long row = (long)blockIdx.x * INV_ROWS + r;
        if (row >= m) break;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc = fmaf(z[row * ld_z + j], w[(long)j * ld_w + c], acc);
        out[row * ld_out + c] = acc + mu;
    }
}

// what the two projections check alike
int check_project(const char* what_null, const char* what_shape, const void* a, const void* b, const void* c, const void* o, long m, long d,
                  long k, const char** err) {
    if (!a || !b || !c || !o) { *err = what_null; return -1; }
    if (m < 1 || m > (1 << 24) || d < 1 || d > PCA_MAX_FEATURES || k < 1 || k > PCA_MAX_COMPONENTS || k > d) { *err = what_shape; return -1; }
    return 0;
}
}  // namespace

int launch_pca_transform(const float* x, long ld_x, long m, long d, const float* mean, const float* w, long ld_w, long k, float* out,
                         long ld_out, hipStream_t s, const char** err) {
    const int r = check_project("pca_transform: null buffer", "pca_transform: m in [1, 2^24], d in [1, 4096], k in [1, min(d, 64)]", x, mean, w, out,
                                m, d, k, err);
    if (r) return r;
    if (ld_x < d || ld_w < d || ld_out < k) { *err = "pca_transform: row pitch smaller than the row"; return -1; }
    MRGAN_LAUNCH(pca_transform_kernel, dim3(ceil_div(m, 4 * TR_ROWS)), dim3(256), 0, s, x, ld_x, (int)m, (int)d, mean, w, ld_w, (int)k, out, ld_out);
    if (hipGetLastError() != hipSuccess) { *err = "pca_transform: launch failed"; return -10; }
    return 0;
}

int launch_pca_inverse_transform(const float* z, long ld_z, long m, long k, const float* w, long ld_w, long d, const float* mean, float* out,
                                 long ld_out, hipStream_t s, const char** err) {
    const int r = check_project("pca_inverse_transform: null buffer",
                                "pca_inverse_transform: m in [1, 2^24], d in [1, 4096], k in [1, min(d, 64)]", z, mean, w, out, m, d, k, err);
    if (r) return r;
    if (ld_z < k || ld_w < d || ld_out < d) { *err = "pca_inverse_transform: row pitch smaller than the row"; return -1; }
    MRGAN_LAUNCH(pca_inverse_kernel, dim3(ceil_div(m, INV_ROWS), ceil_div(d, 256)), dim3(256), 0, s, z, ld_z, (int)m, (int)k, w, ld_w, (int)d, mean,
                 out, ld_out);
    if (hipGetLastError() != hipSuccess) { *err = "pca_inverse_transform: launch failed"; return -10; }
    return 0;
}

}  // namespace mrgan
