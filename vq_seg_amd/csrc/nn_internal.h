// Host-side state shared by the NN kernel units only (nn_bn / nn_spatial / nn_head / nn_stem / nn_host): the dispatch options and the
// grid size of the grid-stride kernels.  Everything other units may call is in nn_kernels.h.  Nothing here depends on a build flag,
// so a unit compiled with -DBN_UNROLL / -DIM2COL_ABL links with the regular objects.
#pragma once
#include "nn_kernels.h"

namespace vqseg {

// Tunables of the NN launchers (vqseg_set_option; the key of each field: NN_OPTIONS in nn_host.hip, where the one instance lives)
struct NnOptions {
    int grid_cap = 8192;                // workgroups of the grid-stride elementwise kernels (option "nn_grid_cap")
    // debug only (timing experiments, results garbage): bit 1 skip the forward statistics merge + finalize, 2 the backward finalize,
    // 4 the weight-gradient slab sums -- "what do the ~950 tiny launches of a step cost on the wall clock?" (VQSEG_OPTS=debug_skip_small=7)
    int debug_skip_small = 0;
    int bn_bwd_premask = 1;             // residual layers: masked gradient written by the reduce pass (0: r3, both passes read g_out + out)
    int bilinear_up2 = 1;               // exact-2x fast kernels (bit-identical to the generic ones); 2: one input row per thread in the backward (r3)
    int im2col_strip = 1;               // the stem's patch matrix from LDS-staged strips (0: the gather kernel, r3)
};
extern NnOptions g_nn_opt;

inline unsigned grid_for(long work, int per_block = 256, long cap = 0) {
    if (cap == 0) cap = g_nn_opt.grid_cap;
    long b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

}  // namespace vqseg
