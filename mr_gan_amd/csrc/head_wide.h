// Stand-alone loss head on the matrix cores for what the chain cannot hold (head_wide.hip): feature layers wider than 256 columns
// (BASELINE configs[4]: 4096), and more than 8 classes (class pitch 32) at any multiple of 256 columns: the three products of
// chain_head over 64-row blocks, the feature dimension walked in 256-column chunks.
// feat % 256 == 0; bf16 features; segment kinds LAB / UNL / FAKE (training); mask = the feature layer's lane-native relu mask.
#pragma once
#include "aux_kernels.h"
#include "chain.h"

namespace mrgan {

struct HeadWideArgs {
    HeadArgs h;
    const uint16_t* mask; long mask_bs; int ldm;
    __bf16* w6c; __bf16* w6r;          // scratch: the bf16 addends of W6, class-major [3][KP][feat] and row-major [3][feat][KP] (KP = h.ldw)
};
constexpr int HEAD_WIDE_ROWS = CH_ROWS;
int launch_w6_split(const HeadWideArgs& a, hipStream_t s);       // first: the addends of the current W6
int launch_head_wide(const HeadWideArgs& a, hipStream_t s);
int head_wide_init_attributes();

}  // namespace mrgan
