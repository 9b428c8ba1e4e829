// The two device functions every bilinear resize of the library goes through (nn_spatial.hip: the generic and the exact-2x kernels and
// their split-3 instantiations; predict_kernels.hip: the fused resize + arg-max; render_kernels.hip: the sheet's image panels), in ONE copy: the kernels that share them round
// identically by construction.  ATen upsample_bilinear2d semantics:
//   align_corners: src = dst * (in-1)/(out-1);  else src = max((dst+0.5)*in/out - 0.5, 0)
#pragma once
#include <hip/hip_runtime.h>

namespace vqseg {

// (1 - lh) * ((1 - lw) * v00 + lw * v01) + lh * ((1 - lw) * v10 + lw * v11) with the multiply-adds spelled out: the generic and the
// exact-2x kernels (and their split-3 instantiations) must round identically, and the compiler's own choice of which product of a sum to fuse
// differs between kernels whose weights are run-time values and kernels whose weights are constants
__device__ __forceinline__ float bil_mix(float v00, float v01, float v10, float v11, float lh, float lw) {
    const float top = __builtin_fmaf(lw, v01, (1.0f - lw) * v00);
    const float bot = __builtin_fmaf(lw, v11, (1.0f - lw) * v10);
    return __builtin_fmaf(lh, bot, (1.0f - lh) * top);
}

__device__ __forceinline__ void bil_src(int d, int in, int out, int align, int& i0, int& i1, float& l1) {
    float s;
    if (align) s = out > 1 ? (float)d * ((float)(in - 1) / (float)(out - 1)) : 0.0f;
    else {
        s = ((float)d + 0.5f) * ((float)in / (float)out) - 0.5f;
        if (s < 0.0f) s = 0.0f;
    }
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

// ATen upsample_nearest ('nearest', not 'nearest-exact'): the source index of destination index d when `in` samples are read at `out`
// positions -- min((int)(d * ((float)in / out)), in - 1).  The one copy: the sheet's target panels (render_kernels.hip) and the contrastive
// loss's labels (supcon_kernels.hip) read a larger int64 target through it.
__device__ __forceinline__ int nearest_src(int d, int in, int out) {
    const int s = (int)((float)d * ((float)in / (float)out));
    return s < in - 1 ? s : in - 1;
}

}  // namespace vqseg
