// The libsvm classifiers of the SVM baseline on the device (svm.hip): Gram matrix (RBF, mr_svm.py:106, or linear), SMO solver
// (C-SVC or nu-SVC), one-vs-one vote.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrgan_abi.h"

namespace mrgan {

constexpr int SVM_MAX_GROUP = MRGAN_SVM_MAX_GROUP;     // problems of one grouped launch
constexpr int SVM_MAX_PAIR = 2048;         // rows of one one-vs-one problem (MRGAN_SVM_MAX_PAIR): two per thread of the solver's block
constexpr int SVM_MAX_CLASSES = 32;
constexpr int SVM_MAX_PAIRS = SVM_MAX_CLASSES * (SVM_MAX_CLASSES - 1) / 2;

// first row of every class in the class-sorted row order, start[num_classes] = n (passed to the kernels by value)
struct SvmClasses { int start[SVM_MAX_CLASSES + 1]; };

// All of them: 0 on success, -1 bad argument, -10 HIP failure (message in *err, static storage).
// out[a, b] = exp(-gamma * max(0, |A_a|^2 + |B_b|^2 - 2 A_a . B_b)); tile: 0 = chosen from the shape, 64 or 128 = forced
int launch_svm_gram(const float* a, long ld_a, long m, const float* b, long ld_b, long n, long d, float gamma, float* out, long ld_out,
                    int tile, hipStream_t s, const char** err);
int launch_svm_solve(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double C, double tol, int max_iter,
                     double* coef, double* rho, int* iters, hipStream_t s, const char** err);
int launch_svm_decide(const float* kt, long ld_kt, long m, long n, int num_classes, const int64_t* class_start, const double* coef,
                      const double* rho, double* dec, int* labels, hipStream_t s, const char** err);
// launch_svm_gram with a kernel kind: MRGAN_SVM_KERNEL_RBF is launch_svm_gram itself (the same kernel, the same bits);
// MRGAN_SVM_KERNEL_LINEAR writes out[a, b] = A_a . B_b, the same k-ordered chain, and ignores gamma
int launch_svm_kernel_matrix(int kind, const float* a, long ld_a, long m, const float* b, long ld_b, long n, long d, float gamma, float* out,
                             long ld_out, int tile, hipStream_t s, const char** err);
// libsvm's nu-SVC (Solver_NU) on a precomputed kernel matrix: coef = alpha y / r, rho / r, r itself (r_out optional), iterations.
// An infeasible nu is an error before any launch: *bad_i, *bad_j = the classes of the first such pair (-1 otherwise).
int launch_svm_solve_nu(const float* k, long ld_k, long n, int num_classes, const int64_t* class_start, double nu, double tol, int max_iter,
                        double* coef, double* rho, double* r_out, int* iters, hipStream_t s, const char** err, int* bad_i, int* bad_j);

// The same three for up to SVM_MAX_GROUP ragged problems in one launch each (items: host arrays of the ABI's descriptors,
// copied into the kernel arguments).  Every item gets its single entry's checks before any launch; *bad_item = the item a
// message is about, -1 where it is about the group.  Each item's outputs are the single launch's bit for bit.
int launch_svm_gram_group(const mrgan_svm_gram_item* items, int count, long d, float gamma, int tile, hipStream_t s, const char** err,
                          int* bad_item);
int launch_svm_solve_group(const mrgan_svm_solve_item* items, int count, int num_classes, double C, double tol, int max_iter, hipStream_t s,
                           const char** err, int* bad_item);
int launch_svm_decide_group(const mrgan_svm_decide_item* items, int count, int num_classes, hipStream_t s, const char** err, int* bad_item);
// launch_svm_gram_group with a kernel kind, as launch_svm_kernel_matrix is to launch_svm_gram: MRGAN_SVM_KERNEL_RBF is
// launch_svm_gram_group itself (the same kernel); an unknown kind is refused
int launch_svm_kernel_matrix_group(int kind, const mrgan_svm_gram_item* items, int count, long d, float gamma, int tile, hipStream_t s,
                                   const char** err, int* bad_item);
// launch_svm_solve_nu on every item with that item's nu (tol and max_iter are the group's).  *bad_i, *bad_j: the classes of the
// pair the nu of item *bad_item is infeasible for (-1 otherwise)
int launch_svm_solve_nu_group(const mrgan_svm_solve_nu_item* items, int count, int num_classes, double tol, int max_iter, hipStream_t s,
                              const char** err, int* bad_item, int* bad_i, int* bad_j);

}  // namespace mrgan
