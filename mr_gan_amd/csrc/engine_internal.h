// What the engine's translation units share: the handle, its parts, error reporting.
//   engine_state.hip  workspace layout, create / destroy, weights and Adam slots in and out, regions, tuning
//   engine.hip        the launch call sites, the phases of the sub-steps, the public step entries
//   engine_debug.hip  the diagnostic entries of include/mrgan_debug.h
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mrgan_abi.h"
#include "../../include/mrgan_debug.h"
#include "aux_kernels.h"
#include "chain.h"
#include "head_wide.h"
#include "logmel.h"
#include "pca.h"
#include "svm.h"
#include "gemm.h"

namespace mrgan {

int fail(int code, const char* fmt, ...);      // records the message behind mrgan_last_error (per thread), returns code
// a grouped SVM launcher's message, naming the item it is about (item < 0: about the group itself)
inline int svm_group_fail(int code, const char* msg, int item) {
    return item < 0 ? fail(code, "%s", msg) : fail(code, "%s (item %d)", msg, item);
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

constexpr int SEG_ALIGN = 128; // segment row stride is a multiple of the GEMM block tile

struct Dense;
struct Tensor {                // one trainable tensor (padded fp32 master + Adam slots)
    int rows, cols;            // logical (1-D: rows = 1)
    int prow, pcol;            // padded
    float *p, *m, *v;
    __bf16 *w16, *wt16;
    float* flat;               // position inside the flat gradient buffer
    __bf16* flat16;            // ... inside the bfloat16 one (MRGAN_FLAG_GRAD_BF16)
    const float* g; int nslab; long slab_stride;      // fused-mode gradient source
    const Dense* layer;                               // the dense layer whose weight matrix this is (null: bias, BatchNorm)
};

// fp8 storage of a dense layer (gemm_fp8.hip): e4m3 images of its input and e5m2 images of its output gradient dpre, each
// row-major [segments][S][width] and transposed [width][pitch] (segment b at column b S), written by the producing product's
// epilogue, the loss head, the feature-matching kernel or a quantiser pass; e4m3 weight copies w8 [K][N] / w8t [N][K],
// refreshed by the Adam kernel.  Forward reads x8 x w8t, dX g8 x w8, dW x8t x g8t over the whole pitch (rows >= batch of a
// segment are zero in both).  Every image has a scaling slot per sub-step kind (0 = D, 1 = G).
struct Fp8Images {
    bool on;                                  // false: the layer's products take the bf16 / fp32 tensors
    unsigned char *x8, *x8t; int ldxt;
    unsigned char *g8, *g8t; int ldgt;
    unsigned char *w8, *w8t;
    int xseg;                                 // segment of x8 / x8t the products work on (G2: the generator view's, set_gen_view)
    int sx[2], sg[2], sw;                     // slot indices: input and gradient per sub-step kind, weight
};

struct Dense {
    int K, N, Kp, Np, act;
    Tensor *W, *b;
    float* slabs; int splits;   // weight-gradient slabs [nseg*splits][Kp][Np]
    Fp8Images q;                // fp8 handles: the discriminator's D1 .. D5 and the generator's wide layer G2
};

struct ProfRec { int cat; hipEvent_t start, stop; double flops, bytes; };      // device-side begin / end of one kernel (MRGAN_LAUNCH)

// fp8 scaling slots (Fp8Images: activations and weights e4m3, gradients e5m2); layout() hands them out
constexpr int FP8_NSLOT = 28, FP8_DRY_PASSES = MRGAN_FP8_DRY_PASSES;
constexpr float FP8_TARGET_E4M3 = 224.0f, FP8_TARGET_E5M2 = 28672.0f;      // half the largest finite value: 2x headroom


}  // namespace mrgan

using namespace mrgan;      // (the handle is a global type of the C ABI)

struct mrgan_handle {
    mrgan_config cfg;
    bool bf16, sync_stats, flat_grads, own_ws;
    int gauss;               // MRGAN_FLAG_GAUSS_NOISE: layer noise and device-drawn z come from the true-Gaussian generator
    int es;                               // activation element size
    int B, S, tiles_m, Bg;                // local batch, segment stride, row tiles per segment, global batch
    float stat_count, fm_scale;           // rows behind a batch statistic; 1/world when statistics stay per-shard
    int Dp, nzp, Fp, F;                   // padded input / z / feature widths
    char* ws; size_t ws_bytes;
    // Model groups (mrgan_config.models > 1).  The workspace holds the single-model layout once per model, W bytes apart (W = 0
    // for a single model); every pointer of this struct is MODEL 0's, model m's tensor lies m * W bytes behind it (model_at).
    // The two DevState slots alone are shared: all models step together.
    int models;                           // >= 1
    size_t W;                             // model stride in bytes
    int sel;                              // mrgan_select_model: the model the per-model entries address
    int grouped;                          // models while a grouped step builds its launches (every launch covers all models), else 1
    // element strides between the models' inputs of the grouped step being built (mrgan_disc_group_args / mrgan_gen_group_args;
    // mrgan_sup_group_args: its x, idx and labels in the labelled slots); all zero outside one
    struct GroupStrides { long x_lab, idx_lab, labels, x_unl, idx_unl, z; } gs;

    std::vector<Tensor> gt, dt;           // Keras order
    Dense g[3], d[6];

    DevState* state;                      // [2]
    // mrgan_attribution: [MRGAN_ATTR_MAX_DRAWS] constant slots, slot d with iter = d and batch = 0 -- the kernels of draw d read
    // their noise step from slot d, so no training kernel learns about draws.  An allocation of its own (64 KB), not workspace.
    DevState* draw_state = nullptr;
    ~mrgan_handle() { if (draw_state) hipFree(draw_state); }
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
    float *cs_bn1, *cs_bn2, *cs_db[5], *cs_f, *cs_db3g, *cs_db2g, *cs_dbeta, *cs_dgamma, *db1g_part;
    float *head_part, *head_red, *loss_part; int head_stride, head_groups;
    int head_nblk;                        // partial rows of head_part / loss_part behind the last loss head (set where it is launched)
    int bnb_blocks;
    // MRGAN_FLAG_AUTOENCODER: d[5] is a full-width layer d_hidden[4] x d_in.  y = its stored output [3 S][Dp], dY [S][Dp] (rows >=
    // batch keep the zeros of mrgan_create), the per-64-row column sums of dY [tiles_m][Dp] (the last bias gradient; cs_db[4] is
    // that of the layer below), the loss partials [row block][column block][4] of the reconstruction head and the mse
    // accumulator of mrgan_ae_reconstruct.  All null / zero on every other handle, whose layout they leave alone.
    bool ae; void *ae_y, *ae_dy; float *ae_cs, *ae_loss_part, *ae_mse;
    // fp8 mode (gemm_fp8.hip): the layers' Fp8Images and their scaling slots
    bool fp8; int fp8_cal[2];
    Fp8Slot* slots; float* slot_targets; float* accum_save;
    float* fm_scratch; unsigned int* fm_count;       // feature-matching loss partials of a wide feature layer (aux_kernels.hip)
    int KP;                              // class pitch (aux_kernels.h): columns of W6 / b6 / logits / the head's partial rows
    bool chain_ok, use_chain;            // the 256-wide tail of the discriminator runs as row-block chain launches (gemm_chain.hip)
    bool dtail_chain() const { return use_chain && KP == KMAX; }   // ... the D sub-step's too: its head is an 8-class kernel
    bool head_wide_ok, head_wide; __bf16 *w6c, *w6r;   // feature layers wider than the chain holds, or more than 8 classes: the stand-alone MFMA loss head (head_wide.h: HeadWideArgs)
    int tune_kc_cfg, tune_bits, tune_pair_gen;      // mrgan_set_tuning
    int ablate;                                      // mrgan_debug_ablate (timing experiments)
    AdamTile *tiles_g_dev, *tiles_d_dev; int ntiles_g, ntiles_d;

    // per-launch hipEvent profiling (bench.py's live roofline measurement)
    bool prof; std::vector<ProfRec> prof_recs; std::vector<std::string> prof_names;

    // graph replay of (D step, G step)
    // (graph_key: the bytes of the two argument blocks the graph was captured with -- the single or the group ones)
    hipGraphExec_t graph_exec; bool graph_ready; int graph_cur;
    unsigned char graph_key[sizeof(mrgan_disc_group_args) + sizeof(mrgan_gen_group_args)]; size_t graph_key_d, graph_key_g;
};

namespace mrgan {

// model m's copy of a per-model tensor of the workspace
template <typename P> inline P* model_at(const mrgan_handle* h, P* p, int m) { return p ? (P*)((char*)p + (size_t)m * h->W) : p; }
template <typename P> inline P* selected(const mrgan_handle* h, P* p) { return model_at(h, p, h->sel); }
inline void* rowptr(mrgan_handle* h, void* base, long row, int ld) { return (char*)base + (size_t)row * ld * h->es; }
inline Dense* net_layers(mrgan_handle* h, int net, int* n) { *n = net == MRGAN_NET_G ? 3 : 6; return net == MRGAN_NET_G ? h->g : h->d; }
inline dim3 grid2d(int prow, int pcol) { return dim3(ceil_div(pcol, 64), ceil_div(prow, 4)); }
// which of the two generator-activation segments the following kernels work on
void set_gen_view(mrgan_handle* h, int seg);
// fp8 copies of a network's weights / the delayed scales of every slot (launches; mrgan_set_weights needs them too)
int fp8_refresh_weights(mrgan_handle* h, int net, hipStream_t s);
int fp8_update_scales(mrgan_handle* h, hipStream_t s);

}  // namespace mrgan
