// nn_host.hip -- the option table of the NN kernel units (no kernel here): the one NnOptions instance, its vqseg_set_option keys, and
// the grid cap other modules size their grids by.
#include <limits.h>
#include <string.h>

#include "nn_internal.h"
#include "options.h"

namespace vqseg {

NnOptions g_nn_opt;
long nn_grid_cap() { return g_nn_opt.grid_cap; }            // data_kernels.hip sizes its grid by the same cap

static const Option NN_OPTIONS[] = {
    {"debug_skip_small", &g_nn_opt.debug_skip_small},
    {"bn_bwd_premask", &g_nn_opt.bn_bwd_premask, OPT_FLAG},
    {"nn_grid_cap", &g_nn_opt.grid_cap, OPT_RANGE_FAIL, 256, INT_MAX},
    {"im2col_strip", &g_nn_opt.im2col_strip, OPT_FLAG},
    {"bilinear_up2", &g_nn_opt.bilinear_up2},
};

int nn_set_option(const char* key, int value) {
    if (key && !strcmp(key, "bilinear_up2") && value > 2) value = 1;      // 0 / 1 / 2 name kernels; anything above means "on"
    return apply_option(NN_OPTIONS, key, value);
}

}  // namespace vqseg
