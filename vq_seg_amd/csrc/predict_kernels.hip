// predict_kernels.hip -- the prediction path's one kernel: bilinear resize of the class logits to the output size, the mean over up to
// four views (networks of an ensemble, flipped test-time views), arg-max, top probability and confusion counts in a single pass
// (vq_seg_amd/nnf.py: resize_argmax; vq_seg_amd/predict.py; evaluate.test_loop(fused=True)).
//
// What it replaces: vqseg_bilinear_f writing an (N, C, Ho, Wo) f32 tensor that vqseg_softmax_stats_f / vqseg_confusion_counts_f read
// back once -- 4 C bytes written and 4 C read per output pixel for a 1-byte label.  Here the output side is a streaming write (1 byte
// label, 4 bytes top probability, 8 bytes of target read per pixel) and the input side a gather from the low-resolution logits, which
// stay in the L2.  The arithmetic is the two-kernel path's own, expression by expression:
//     a_v   = bil_mix(four taps of view v through bil_src)          (bilinear_device.h: the functions vqseg_bilinear_f runs)
//     acc   = a_0 (+ a_1 (+ a_2 + a_3)), f32 adds in view order;  V > 1: acc *= 1 / V   (V in {1, 2, 4}: an exact scale)
//     label = first maximum (`z > mx` from -inf: a NaN never wins, all-NaN gives class 0),  top = 1 / sum_c expf(acc_c - max)
// as softmax_stats_kernel / confusion_kernel (loss_kernels.hip) have them, so V = 1 without a flip is bit-identical to that path.
// A flip is an index map on the source grid (column i reads W - 1 - i, row i reads H - 1 - i); the weights do not change.
//
// Work unit: a tile of 1024 consecutive output pixels of ONE image per workgroup and iteration, 256 per wave; lane l takes the pixels
// l, l + 64, l + 128, l + 192 of its wave's run, so every load and store instruction of the wave covers 64 ADJACENT pixels (the taps of
// adjacent output pixels are adjacent or equal source pixels: a gather instruction touches a few cache lines, where four adjacent
// pixels per lane would put the lanes four pixels apart).  top goes out as four 256-byte stores per wave, the targets come in as four
// 512-byte loads; the u8 labels are packed across lanes (four shuffles) so that lane q stores the word of pixels 4 q .. 4 q + 3 -- one
// 4-byte store per lane instead of four byte stores -- for a wave's whole run at a 4-byte aligned address; a partial last run, or an
// image at another offset, goes byte by byte.  Taps and weights are computed once per pixel for all classes and views, and the four
// pixels' loads of a view are issued together.
// Counts: per wave, one ballot per (target, label) bin, lane k keeping bin k's running count; on the way out of an image they go through
// a per-workgroup LDS histogram and then one integer atomic per bin -- order-independent, as confusion_kernel's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "bilinear_device.h"
#include "nn_kernels.h"
#include "predict_epilogue.h"     // RA_PX, RA_TILE and everything after the mean logits, shared with tile_kernels.hip

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

struct ResizeArgmaxArgs {                                   // the views travel as kernel arguments: no device-side table, no copy
    const float* view[RA_MAXV];
    int flip[RA_MAXV];                                      // bit 0: columns, bit 1: rows
    int V;
    long sb, sc, sp;                                        // batch, class and pixel strides of every view, in elements (rows dense)
    int B, H, W, Ho, Wo;
    int vec;                                                // label 4-byte aligned: a wave's whole run of 256 labels may go out as words
    uint8_t* label;
    float* top;
    const long long* target;
    unsigned long long* counts;
};

template <int C, bool NARROW>
__global__ __launch_bounds__(256, 4) void resize_argmax_kernel(const ResizeArgmaxArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned cnt[RA_MAXC * RA_MAXC];
    const bool counting = a.counts != nullptr;
    if (threadIdx.x < RA_MAXC * RA_MAXC) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long HW = (long)a.Ho * a.Wo;
    const long per = (HW + RA_TILE - 1) / RA_TILE;          // tiles per image
    const long tiles = per * a.B;
    const float scale = 1.0f / (float)a.V;
    const int lane = threadIdx.x & 63;
    unsigned mine = 0;                                      // lane k < C * C: this wave's count of bin k in the current image
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int b = (int)(tile / per);                    // uniform across the workgroup
        const long img = (long)b * HW;
        // a wave takes 256 consecutive pixels of the image, lane l the pixels l, l + 64, l + 128, l + 192 of them
        const long pw = (tile - b * per) * RA_TILE + (threadIdx.x >> 6) * (64 * RA_PX);
        int arg[RA_PX], key[RA_PX];
        float inv[RA_PX];
        long long tg[RA_PX];
        int h0[RA_PX], h1[RA_PX], w0[RA_PX], w1[RA_PX];
        float lh[RA_PX], lw[RA_PX];
        // Taps and weights of the four pixels, without a branch between them, so that each view's 16 C loads below sit in one block and
        // are in flight together.  A pixel past the image's end gets coordinates past the last row: bil_src clamps its taps into the
        // source, its loads are valid and its results are not stored.
        const unsigned Wo = (unsigned)a.Wo;
        unsigned y = (unsigned)(pw + lane) / Wo, x = (unsigned)(pw + lane) - y * Wo;
#pragma unroll
        for (int j = 0; j < RA_PX; ++j) {
            if (j > 0) {                                    // 64 pixels on
                x += 64;
                if (NARROW) {                               // Wo < 64: several rows on
                    const unsigned q = x / Wo;
                    y += q, x -= q * Wo;
                } else {                                    // at most one row end in between
                    const bool wrap = x >= Wo;
                    x -= wrap ? Wo : 0u, y += wrap ? 1u : 0u;
                }
            }
            bil_src((int)y, a.H, a.Ho, 0, h0[j], h1[j], lh[j]);
            bil_src((int)x, a.W, a.Wo, 0, w0[j], w1[j], lw[j]);
            const long p = pw + j * 64 + lane;
            tg[j] = counting && p < HW ? a.target[img + p] : -1;
        }
        float acc[RA_PX][C];
#pragma unroll
        for (int v = 0; v < RA_MAXV; ++v)
            if (v < a.V) {                                  // uniform
                const int f = a.flip[v];
                const float* s = a.view[v] + (long)b * a.sb;
                const unsigned W = (unsigned)a.W, sp = (unsigned)a.sp, sc = (unsigned)a.sc;     // offsets inside an image fit 32 bits (host check)
#pragma unroll
                for (int j = 0; j < RA_PX; ++j) {
                    const unsigned r0 = (f & 2) ? a.H - 1 - h0[j] : h0[j], r1 = (f & 2) ? a.H - 1 - h1[j] : h1[j];
                    const unsigned c0 = (f & 1) ? a.W - 1 - w0[j] : w0[j], c1 = (f & 1) ? a.W - 1 - w1[j] : w1[j];
                    const unsigned o00 = (r0 * W + c0) * sp, o01 = (r0 * W + c1) * sp, o10 = (r1 * W + c0) * sp, o11 = (r1 * W + c1) * sp;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const unsigned oc = c * sc;
                        const float m = bil_mix(s[o00 + oc], s[o01 + oc], s[o10 + oc], s[o11 + oc], lh[j], lw[j]);
                        acc[j][c] = v == 0 ? m : acc[j][c] + m;
                    }
                }
            }
#pragma unroll
        for (int j = 0; j < RA_PX; ++j) {
            ra_argmax_top<C>(acc[j], a.V > 1, scale, a.top != nullptr, arg[j], inv[j]);
            key[j] = tg[j] >= 0 && tg[j] < C ? (int)tg[j] * C + arg[j] : -1;
        }
        if (a.top) {                                        // 256 contiguous bytes per wave and store
#pragma unroll
            for (int j = 0; j < RA_PX; ++j)
                if (pw + j * 64 + lane < HW) a.top[img + pw + j * 64 + lane] = inv[j];
        }
        if (a.label) ra_store_labels(a.label + img, img, pw, HW, lane, a.vec, arg);
        if (counting) {
            ra_count<C>(key, lane, mine);
            const long next = tile + gridDim.x;
            if (next >= tiles || (int)(next / per) != b)    // leaving image b (uniform): waves -> LDS histogram -> one atomic per bin
                ra_flush_counts<C>(cnt, mine, lane, a.counts + (long)b * C * C);
        }
    }
}

static hipError_t launch_resize_argmax(const ResizeArgmaxArgs& a, int c, hipStream_t st) {
    if (a.counts) {
        hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.B * c * c * sizeof(long long), st);
        if (e != hipSuccess) return e;
    }
    const long HW = (long)a.Ho * a.Wo;
    long blocks = (HW + RA_TILE - 1) / RA_TILE * a.B;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
#define VQSEG_RA(C)                                                                                                        \
    if (a.Wo < 64) hipLaunchKernelGGL((resize_argmax_kernel<C, true>), dim3((unsigned)blocks), dim3(256), 0, st, a);        \
    else hipLaunchKernelGGL((resize_argmax_kernel<C, false>), dim3((unsigned)blocks), dim3(256), 0, st, a)
    switch (c) {
        case 2: VQSEG_RA(2); break;
        case 3: VQSEG_RA(3); break;
        default: VQSEG_RA(4); break;
    }
#undef VQSEG_RA
    return hipGetLastError();
}

}  // namespace vqseg

extern "C" {

int vqseg_resize_argmax_f(const float* const* views_host, const int* flips_host, int n_views, int64_t stride_b, int64_t stride_c,
                          int64_t stride_px, int b, int c, int h, int w, int ho, int wo, uint8_t* label, float* top,
                          const int64_t* target, int64_t* counts, void* stream) {
    using namespace vqseg;
    if (n_views != 1 && n_views != 2 && n_views != 4)
        return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: 1, 2 or 4 views (the mean's 1 / V must be exact)");
    if (!views_host || !flips_host) return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: null views_host or flips_host");
    if (c < 2 || c > RA_MAXC) return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: 2..4 classes");
    if (b <= 0 || h <= 0 || w <= 0 || ho <= 0 || wo <= 0)
        return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: b, h, w, ho and wo must be positive");
    if ((long)h * w > (1L << 27) || (long)ho * wo > (1L << 30) || h > (1 << 24) || w > (1 << 24) || ho > (1 << 24) || wo > (1 << 24))
        return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: a source above 2^27 pixels (32-bit offsets inside an image), an output above 2^30 or a side above 2^24");
    for (int v = 0; v < n_views; ++v) {
        if (!views_host[v]) return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: null view");
        if (flips_host[v] < 0 || flips_host[v] > 3)
            return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: a flip code is 0..3 (bit 0 columns, bit 1 rows)");
    }
    if ((target == nullptr) != (counts == nullptr))
        return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: target and counts go together");
    if (!label && !top && !counts) return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: null label, top and counts: nothing to compute");
    // rows dense: planar (pixel stride 1, classes h * w apart) or interleaved (class stride 1, pixels c apart)
    const bool planar = stride_px == 1 && stride_c == (int64_t)h * w;
    const bool interleaved = stride_c == 1 && stride_px == c;
    if (!planar && !interleaved)
        return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: layout must be planar (NCHW) or interleaved (channels_last) with dense rows");
    if (b > 1 && stride_b < (int64_t)c * h * w) return vqseg_set_error(VQSEG_EINVAL, "resize_argmax: batch stride smaller than an image");
    ResizeArgmaxArgs a = {};
    for (int v = 0; v < n_views; ++v) {
        a.view[v] = views_host[v];
        a.flip[v] = flips_host[v];
    }
    a.V = n_views;
    a.sb = stride_b, a.sc = stride_c, a.sp = stride_px;
    a.B = b, a.H = h, a.W = w, a.Ho = ho, a.Wo = wo;
    a.vec = ((uintptr_t)label & 3u) == 0;
    a.label = label, a.top = top;
    a.target = reinterpret_cast<const long long*>(target);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    const hipError_t e = launch_resize_argmax(a, c, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        char buf[160];
        snprintf(buf, sizeof(buf), "resize_argmax_kernel: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

}  // extern "C"
