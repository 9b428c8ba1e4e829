// conv_host.hip -- host-side state of the convolution path: the dispatch options and the per-launch event profile.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "conv_internal.h"
#include "options.h"

namespace vqseg {

ConvOptions g_conv_opt;

static const Option CONV_OPTIONS[] = {
    {"conv3x3_patch_min_workgroups", &g_conv_opt.patch_min_wgs},
    {"conv_wgrad1x1_narrow", &g_conv_opt.wgrad1x1_narrow},
    {"stem_fused", &g_conv_opt.stem_fused, OPT_FLAG},
    {"conv_wgrad_round_pct", &g_conv_opt.wgrad_round_pct, OPT_RANGE_KEEP, 10, 400},
    {"conv_wgrad_xcd", &g_conv_opt.wgrad_xcd},
    {"conv_dgrad_s2_merge", &g_conv_opt.dgrad_s2_merge, OPT_FLAG},
    {"conv_wgrad3x3_fill", &g_conv_opt.wgrad3x3_fill},
    {"conv_wgrad3x3_stride2", &g_conv_opt.wgrad3x3_s2},
    {"conv_short_k_small_tile", &g_conv_opt.short_k_small},
    {"conv_short_k_single_buffer", &g_conv_opt.short_k_single},
    {"conv3x3_patch_unroll", &g_conv_opt.patch_unroll},
    {"conv_linear_prologue", &g_conv_opt.glds_lin, OPT_FLAG},
    {"conv_xcd_pair", &g_conv_opt.glds_pair},
    {"conv3x3_patch_xcd_pair", &g_conv_opt.patch_pair, OPT_FLAG},
    {"conv3x3_patch_chunk_stage", &g_conv_opt.patch_chunk_stage, OPT_FLAG},
    {"conv3x3_patch_tile512", &g_conv_opt.patch_tile512},
    {"conv3x3_patch_tile512_launches", &g_conv_opt.patch_tile512_launches},   // returns the counter, then sets it to `value`
    {"conv3x3_patch_tile512_min_workgroups", &g_conv_opt.patch_tile512_min_wgs},
    {"conv3x3_patch_wide_tile_s3", &g_conv_opt.patch_wide_s3, OPT_FLAG},
    {"conv3x3_patch_wide_tile", &g_conv_opt.patch_wide, OPT_FLAG},
    {"conv_last_variant", &g_conv_opt.last_variant},                          // returns the id (conv_internal.h), then sets it to `value`
};

int conv_set_option(const char* key, int value) { return apply_option(CONV_OPTIONS, key, value); }

// ---- optional per-launch timing of the convolution kernels (bench.py's roofline_conv leg): event pairs on the launch stream
struct ConvProfile {
    bool enabled = false;
    int capacity = 0, count = 0;
    hipEvent_t* ev = nullptr;
    double* flops = nullptr;
    int* kind = nullptr;                                    // KH * 100 + precision tag (0 bf16, 1 precise, 2 split-3)
    int* shape = nullptr;                                   // [4]: output pixels / 1024, Cin (logical), Cout, stride * 10 + up
};
static ConvProfile g_cprof;

hipError_t conv_profile_begin(int capacity) {
    conv_profile_release();
    g_cprof.ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * (size_t)capacity);
    g_cprof.flops = (double*)malloc(sizeof(double) * (size_t)capacity);
    g_cprof.kind = (int*)malloc(sizeof(int) * (size_t)capacity);
    g_cprof.shape = (int*)malloc(sizeof(int) * 4 * (size_t)capacity);
    if (!g_cprof.ev || !g_cprof.flops || !g_cprof.kind || !g_cprof.shape) return hipErrorOutOfMemory;
    for (int i = 0; i < 2 * capacity; ++i) {
        hipError_t rc = hipEventCreate(&g_cprof.ev[i]);
        if (rc != hipSuccess) return rc;
    }
    g_cprof.capacity = capacity;
    g_cprof.count = 0;
    g_cprof.enabled = true;
    return hipSuccess;
}

void conv_profile_release() {
    if (g_cprof.ev)
        for (int i = 0; i < 2 * g_cprof.capacity; ++i) (void)hipEventDestroy(g_cprof.ev[i]);
    free(g_cprof.ev);
    free(g_cprof.flops);
    free(g_cprof.kind);
    free(g_cprof.shape);
    g_cprof = ConvProfile{};
}

int conv_profile_collect(int max_records, double* flops, int* kind, float* ms, int* shape) {
    g_cprof.enabled = false;
    int out = 0;
    for (int i = 0; i < g_cprof.count && out < max_records; ++i) {
        if (hipEventSynchronize(g_cprof.ev[2 * i + 1]) != hipSuccess) break;
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_cprof.ev[2 * i], g_cprof.ev[2 * i + 1]) != hipSuccess) break;
        flops[out] = g_cprof.flops[i];
        kind[out] = g_cprof.kind[i];
        if (shape)
            for (int e = 0; e < 4; ++e) shape[4 * out + e] = g_cprof.shape[4 * i + e];
        ms[out] = t;
        ++out;
    }
    conv_profile_release();
    return out;
}

ConvProfileScope::ConvProfileScope(hipStream_t st, double flops, int kind, int shape0, int shape1, int shape2, int shape3)
    : st_(st), slot_(g_cprof.enabled && g_cprof.count < g_cprof.capacity ? g_cprof.count : -1) {
    if (slot_ < 0) return;
    g_cprof.flops[slot_] = flops;
    g_cprof.kind[slot_] = kind;
    g_cprof.shape[4 * slot_ + 0] = shape0;
    g_cprof.shape[4 * slot_ + 1] = shape1;
    g_cprof.shape[4 * slot_ + 2] = shape2;
    g_cprof.shape[4 * slot_ + 3] = shape3;
    ++g_cprof.count;
    (void)hipEventRecord(g_cprof.ev[2 * slot_], st_);
}

ConvProfileScope::~ConvProfileScope() {
    if (slot_ >= 0) (void)hipEventRecord(g_cprof.ev[2 * slot_ + 1], st_);
}

}  // namespace vqseg
