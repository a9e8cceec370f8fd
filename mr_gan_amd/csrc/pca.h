// PCA pre-stage on the device (pca.hip): what decomposition.PCA(n_components) of the reference's pcaScale
// (others/wganlpctsemi.py:129-139) computes -- column means, centred covariance, leading eigenpairs, projection.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrgan_abi.h"

namespace mrgan {

constexpr int PCA_MAX_COMPONENTS = MRGAN_PCA_MAX_COMPONENTS, PCA_GUARD = MRGAN_PCA_GUARD;
constexpr int PCA_MAX_BLOCK = PCA_MAX_COMPONENTS + PCA_GUARD;      // rows of the iterated block
constexpr int PCA_MAX_FEATURES = MRGAN_PCA_MAX_FEATURES;
constexpr int PCA_RANK_ERROR = MRGAN_PCA_RANK_DEFICIENT;

// All of them: 0 on success, -1 bad argument, -10 HIP failure (message in *err, static storage).
int launch_pca_mean(const float* x, long ld_x, long n, long d, float* mean, hipStream_t s, const char** err);
// tile: 0 = chosen from the shape, 64 or 128 = forced; split: 0 = chosen from the shape, else the number of row ranges
// (at most one per 16 rows).  launch_pca_covariance needs pca_covariance_workspace_bytes of the same (n, d, tile, split) in work.
long pca_covariance_workspace_bytes(long n, long d, int tile, int split);
int launch_pca_covariance(const float* x, long ld_x, long n, long d, const float* mean, float* cov, long ld_cov, void* work,
                          long work_bytes, int tile, int split, hipStream_t s, const char** err);
// the orthonormalisation stage of the block iteration: Y [p x d] -> Q [p x d] with orthonormal rows spanning Y's rows, sorted
// by descending lam (the eigenvalues of Y Y^T, [p] float64); rows with lam_j <= 2^-40 lam_1 are zero.  work: pca_eig_workspace_bytes
long pca_eig_workspace_bytes(long d, long p);
int launch_pca_orthonormalize(const float* y, long ld_y, long p, long d, void* work, long work_bytes, float* q, long ld_q, double* lam,
                              hipStream_t s, const char** err);
// the leading k eigenpairs of the symmetric cov by block iteration; synchronises the stream between iterations (one readback of
// 2 p + 1 doubles each).  PCA_RANK_ERROR: fewer than k directions survive the orthonormalisation.
int launch_pca_eig(const float* cov, long ld_cov, long d, long k, const float* q0, long ld_q0, long p, double tol, int max_iter, void* work,
                   long work_bytes, float* components, long ld_w, double* values_host, double* residuals_host, int* iters_host,
                   hipStream_t s, const char** err);
int launch_pca_transform(const float* x, long ld_x, long m, long d, const float* mean, const float* w, long ld_w, long k, float* out,
                         long ld_out, hipStream_t s, const char** err);
int launch_pca_inverse_transform(const float* z, long ld_z, long m, long k, const float* w, long ld_w, long d, const float* mean, float* out,
                                 long ld_out, hipStream_t s, const char** err);

}  // namespace mrgan
