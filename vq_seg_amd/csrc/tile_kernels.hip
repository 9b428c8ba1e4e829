// tile_kernels.hip -- tiled (sliding-window) prediction: the two launches around the network's forwards (vq_seg_amd/nnf.py:
// extract_windows, merge_argmax; vq_seg_amd/predict.py: Predictor(window=...)).
//
// The window rule, the same arithmetic on the host (nnf.window_starts) and here (win_start / win_count / win_range):
//     n = ceil((extent - window) / stride) + 1,   start[k] = min(k * stride, extent - window),   1 <= stride <= window <= extent
// Only the last window is clamped ((n - 2) * stride < extent - window), so the windows that hold a position y are a contiguous run
//     k_lo = y < window ? 0 : (y - window) / stride + 1   ..   k_hi = y >= extent - window ? n - 1 : y / stride
// The kernels take (extent, window, stride) per axis and derive the starts: no start table, no cap on the number of windows.
//
// extract_windows_kernel: images (B, 3, H, W) -> (F, B * T, 3, nh, nw), window row = b * T + j * nx + i.  A thread takes one pixel
// of one window's resized crop: taps and weights once (bil_src clamps the taps into the WINDOW: its extent is the source size),
// three channels through bil_mix, and one store per channel and requested flip at the flipped position -- a wave's 64 adjacent
// pixels store 64 adjacent floats, in reverse order under a column flip.  Down-scaling is ATen's un-antialiased rule.
//
// merge_argmax_kernel: per output pixel and view, the weighted mean over the windows that hold the pixel of the window's logits
// resized to the window's extent; then the views' mean, arg-max, top probability and confusion counts exactly as
// resize_argmax_kernel has them (predict_epilogue.h: one copy).  Work unit as there: a wave takes 256 consecutive output pixels
// of one image, lane l the pixels l, l + 64, l + 128, l + 192, so the lanes of a gather instruction sit on adjacent pixels of --
// except at a window edge -- the same windows: adjacent or equal taps of one window's logits.  The window loops run per lane
// between the lane's own bounds; those are equal along a row segment except where a window begins or ends, and that is where
// the wave diverges.  Taps and weights of a (pixel, window) are computed once for all classes and views.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "bilinear_device.h"
#include "nn_kernels.h"
#include "predict_epilogue.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

__host__ __device__ __forceinline__ int win_count(int extent, int window, int stride) { return (extent - window + stride - 1) / stride + 1; }

__device__ __forceinline__ int win_start(int k, int extent, int window, int stride) {
    const int s = k * stride;
    return s < extent - window ? s : extent - window;
}

// the windows k_lo .. k_hi (never empty) that hold position y
__device__ __forceinline__ void win_range(int y, int extent, int window, int stride, int n, int& k_lo, int& k_hi) {
    k_lo = y < window ? 0 : (y - window) / stride + 1;
    k_hi = y >= extent - window ? n - 1 : y / stride;
}

// ------------------------------------------------------------------------------------------------------------------------------
struct ExtractArgs {
    const float* images;
    long sb, sc, sp;                                        // batch, channel and pixel strides in elements (rows dense)
    int B, H, W;
    int wh, ww, sy, sx, ny, nx;                             // window extent, stride and grid
    int nh, nw;                                             // the network's input size
    int F;
    int flip[4];                                            // bit 0: columns, bit 1: rows
    float* out;                                             // (F, B * T, 3, nh, nw)
};

__global__ __launch_bounds__(256) void extract_windows_kernel(const ExtractArgs a) {
#pragma clang fp contract(off)
    const long plane = (long)a.nh * a.nw;                   // <= 2^27 (host check)
    const int T = a.ny * a.nx;
    const long rows = (long)a.B * T;
    const long total = rows * plane;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long row = idx / plane;
        const unsigned p = (unsigned)(idx - row * plane);
        const unsigned ry = p / (unsigned)a.nw, rx = p - ry * (unsigned)a.nw;
        const int b = (int)(row / T), t = (int)(row - (long)b * T);
        const int j = t / a.nx, i = t - j * a.nx;
        const int y0 = win_start(j, a.H, a.wh, a.sy), x0 = win_start(i, a.W, a.ww, a.sx);
        int h0, h1, w0, w1;
        float lh, lw;
        bil_src((int)ry, a.wh, a.nh, 0, h0, h1, lh);        // taps inside the window: 0 .. wh - 1
        bil_src((int)rx, a.ww, a.nw, 0, w0, w1, lw);
        const float* s = a.images + (long)b * a.sb;
        const unsigned W = (unsigned)a.W, sp = (unsigned)a.sp;                          // offsets inside an image fit 32 bits (host check)
        const unsigned o00 = ((y0 + h0) * W + x0 + w0) * sp, o01 = ((y0 + h0) * W + x0 + w1) * sp;
        const unsigned o10 = ((y0 + h1) * W + x0 + w0) * sp, o11 = ((y0 + h1) * W + x0 + w1) * sp;
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned oc = c * (unsigned)a.sc;
            m[c] = bil_mix(s[o00 + oc], s[o01 + oc], s[o10 + oc], s[o11 + oc], lh, lw);
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
            if (f < a.F) {                                  // uniform
                const unsigned oy = (a.flip[f] & 2) ? a.nh - 1 - ry : ry, ox = (a.flip[f] & 1) ? a.nw - 1 - rx : rx;
                float* o = a.out + ((long)f * rows + row) * 3 * plane + (long)oy * a.nw + ox;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane] = m[c];
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
struct MergeArgs {                                          // the views travel as kernel arguments: no device-side table, no copy
    const float* view[RA_MAXV];
    int flip[RA_MAXV];                                      // bit 0: columns, bit 1: rows
    int V;
    long sb, sc, sp;                                        // window-row, class and pixel strides of every view, in elements (rows dense)
    int B, lh, lw;                                          // images; the size of a window's logits
    int Ho, Wo, wh, ww, sy, sx, ny, nx;
    int linear;                                             // blend: 0 uniform (w = 1), 1 linear (w = min(r + 1, window - r) per axis)
    int vec;                                                // label 4-byte aligned
    uint8_t* label;
    float* top;
    const long long* target;
    unsigned long long* counts;
};

template <int C>
__global__ __launch_bounds__(256, 2) void merge_argmax_kernel(const MergeArgs a) {
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
    const int T = a.ny * a.nx;
    const unsigned LW = (unsigned)a.lw, sp = (unsigned)a.sp, sc = (unsigned)a.sc;       // offsets inside a window's logits fit 32 bits (host check)
    unsigned mine = 0;                                      // lane k < C * C: this wave's count of bin k in the current image
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int b = (int)(tile / per);                    // uniform across the workgroup
        const long img = (long)b * HW;
        const long pw = (tile - b * per) * RA_TILE + (threadIdx.x >> 6) * (64 * RA_PX);
        int arg[RA_PX], key[RA_PX];
        float inv[RA_PX];
#pragma unroll
        for (int q = 0; q < RA_PX; ++q) {
            const long p = pw + q * 64 + lane;
            const bool live = p < HW;                       // a pixel past the image's end computes the last pixel's result and stores nothing
            const unsigned pc = (unsigned)(live ? p : HW - 1);
            const int y = (int)(pc / (unsigned)a.Wo), x = (int)(pc - (unsigned)y * (unsigned)a.Wo);
            const long long tg = counting && live ? a.target[img + p] : -1;
            int j_lo, j_hi, i_lo, i_hi;
            win_range(y, a.Ho, a.wh, a.sy, a.ny, j_lo, j_hi);
            win_range(x, a.Wo, a.ww, a.sx, a.nx, i_lo, i_hi);
            float acc[RA_MAXV][C];
#pragma unroll
            for (int v = 0; v < RA_MAXV; ++v)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[v][c] = 0.0f;
            float ws = 0.0f;
            for (int j = j_lo; j <= j_hi; ++j) {
                const int ry = y - win_start(j, a.Ho, a.wh, a.sy);                      // 0 .. wh - 1
                int h0, h1;
                float fh;
                bil_src(ry, a.lh, a.wh, 0, h0, h1, fh);
                const float wy = a.linear ? (float)(ry + 1 < a.wh - ry ? ry + 1 : a.wh - ry) : 1.0f;
                for (int i = i_lo; i <= i_hi; ++i) {
                    const int rx = x - win_start(i, a.Wo, a.ww, a.sx);
                    int w0, w1;
                    float fw;
                    bil_src(rx, a.lw, a.ww, 0, w0, w1, fw);
                    const float wx = a.linear ? (float)(rx + 1 < a.ww - rx ? rx + 1 : a.ww - rx) : 1.0f;
                    const float w = wy * wx;                // a product of two integers <= 2048: exact
                    ws += w;
                    const long row = ((long)b * T + (long)j * a.nx + i) * a.sb;
#pragma unroll
                    for (int v = 0; v < RA_MAXV; ++v)
                        if (v < a.V) {                      // uniform
                            const int f = a.flip[v];
                            const float* s = a.view[v] + row;
                            const unsigned r0 = (f & 2) ? a.lh - 1 - h0 : h0, r1 = (f & 2) ? a.lh - 1 - h1 : h1;
                            const unsigned c0 = (f & 1) ? a.lw - 1 - w0 : w0, c1 = (f & 1) ? a.lw - 1 - w1 : w1;
                            const unsigned o00 = (r0 * LW + c0) * sp, o01 = (r0 * LW + c1) * sp, o10 = (r1 * LW + c0) * sp, o11 = (r1 * LW + c1) * sp;
#pragma unroll
                            for (int c = 0; c < C; ++c) {
                                const unsigned oc = c * sc;
                                const float m = bil_mix(s[o00 + oc], s[o01 + oc], s[o10 + oc], s[o11 + oc], fh, fw);
                                acc[v][c] = __builtin_fmaf(w, m, acc[v][c]);
                            }
                        }
                }
            }
            float z[C];
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = acc[0][c] / ws;                          // IEEE fp32 division
#pragma unroll
            for (int v = 1; v < RA_MAXV; ++v)
                if (v < a.V) {
#pragma unroll
                    for (int c = 0; c < C; ++c) z[c] = z[c] + acc[v][c] / ws;
                }
            ra_argmax_top<C>(z, a.V > 1, scale, a.top != nullptr, arg[q], inv[q]);
            key[q] = tg >= 0 && tg < C ? (int)tg * C + arg[q] : -1;
        }
        if (a.top) {                                        // 256 contiguous bytes per wave and store
#pragma unroll
            for (int q = 0; q < RA_PX; ++q)
                if (pw + q * 64 + lane < HW) a.top[img + pw + q * 64 + lane] = inv[q];
        }
        if (a.label) ra_store_labels(a.label + img, img, pw, HW, lane, a.vec, arg);
        if (counting) {
            ra_count<C>(key, lane, mine);
            const long next = tile + gridDim.x;
            if (next >= tiles || (int)(next / per) != b)    // leaving image b (uniform)
                ra_flush_counts<C>(cnt, mine, lane, a.counts + (long)b * C * C);
        }
    }
}

static hipError_t launch_merge_argmax(const MergeArgs& a, int c, hipStream_t st) {
    if (a.counts) {
        hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.B * c * c * sizeof(long long), st);
        if (e != hipSuccess) return e;
    }
    const long HW = (long)a.Ho * a.Wo;
    long blocks = (HW + RA_TILE - 1) / RA_TILE * a.B;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    switch (c) {
        case 2: hipLaunchKernelGGL((merge_argmax_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((merge_argmax_kernel<3>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((merge_argmax_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    }
    return hipGetLastError();
}

// what both entry points ask of a window grid; nullptr when it is in order
static const char* grid_error(int extent_y, int extent_x, int wh, int ww, int sy, int sx) {
    if (wh <= 0 || ww <= 0 || sy <= 0 || sx <= 0) return "window and stride must be positive";
    if (wh > extent_y || ww > extent_x) return "a window larger than the image (no padding)";
    if (sy > wh || sx > ww) return "a stride larger than the window leaves pixels uncovered";
    if (wh > 4096 || ww > 4096) return "a window side above 4096 (a linear blend weight must stay an exact fp32 integer)";
    return nullptr;
}

}  // namespace vqseg

extern "C" {

int vqseg_extract_windows_f(const float* images, int64_t stride_b, int64_t stride_c, int64_t stride_px, int b, int h, int w, int wh, int ww,
                            int sy, int sx, int nh, int nw, const int* flips_host, int n_flips, float* out, void* stream) {
    using namespace vqseg;
    char buf[200];
    if (!images || !out || !flips_host) return vqseg_set_error(VQSEG_EINVAL, "extract_windows: null images, out or flips_host");
    if (n_flips < 1 || n_flips > 4) return vqseg_set_error(VQSEG_EINVAL, "extract_windows: 1..4 flip codes");
    for (int f = 0; f < n_flips; ++f)
        if (flips_host[f] < 0 || flips_host[f] > 3)
            return vqseg_set_error(VQSEG_EINVAL, "extract_windows: a flip code is 0..3 (bit 0 columns, bit 1 rows)");
    if (b <= 0 || h <= 0 || w <= 0 || nh <= 0 || nw <= 0)
        return vqseg_set_error(VQSEG_EINVAL, "extract_windows: b, h, w, nh and nw must be positive");
    if (const char* g = grid_error(h, w, wh, ww, sy, sx)) {
        snprintf(buf, sizeof(buf), "extract_windows: %s", g);
        return vqseg_set_error(VQSEG_EINVAL, buf);
    }
    if ((long)h * w > (1L << 27) || (long)nh * nw > (1L << 27) || h > (1 << 24) || w > (1 << 24) || nh > (1 << 24) || nw > (1 << 24))
        return vqseg_set_error(VQSEG_EINVAL, "extract_windows: an image or a network input above 2^27 pixels (32-bit offsets inside an image) or a side above 2^24");
    const bool planar = stride_px == 1 && stride_c == (int64_t)h * w;
    const bool interleaved = stride_c == 1 && stride_px == 3;
    if (!planar && !interleaved)
        return vqseg_set_error(VQSEG_EINVAL, "extract_windows: layout must be planar (NCHW) or interleaved (channels_last) with dense rows");
    if (b > 1 && stride_b < (int64_t)3 * h * w) return vqseg_set_error(VQSEG_EINVAL, "extract_windows: batch stride smaller than an image");
    ExtractArgs a = {};
    a.images = images;
    a.sb = stride_b, a.sc = stride_c, a.sp = stride_px;
    a.B = b, a.H = h, a.W = w;
    a.wh = wh, a.ww = ww, a.sy = sy, a.sx = sx;
    a.ny = win_count(h, wh, sy), a.nx = win_count(w, ww, sx);
    a.nh = nh, a.nw = nw;
    a.F = n_flips;
    for (int f = 0; f < n_flips; ++f) a.flip[f] = flips_host[f];
    a.out = out;
    const long rows = (long)b * a.ny * a.nx;
    if (rows > (1L << 40) / ((long)nh * nw))
        return vqseg_set_error(VQSEG_EINVAL, "extract_windows: more than 2^40 output pixels per channel and flip");
    long blocks = (rows * nh * nw + 255) / 256;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(extract_windows_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(buf, sizeof(buf), "extract_windows_kernel: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

int vqseg_merge_argmax_f(const float* const* views_host, const int* flips_host, int n_views, int64_t stride_b, int64_t stride_c,
                         int64_t stride_px, int b, int c, int lh, int lw, int ho, int wo, int wh, int ww, int sy, int sx, int blend,
                         uint8_t* label, float* top, const int64_t* target, int64_t* counts, void* stream) {
    using namespace vqseg;
    char buf[200];
    if (n_views != 1 && n_views != 2 && n_views != 4)
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: 1, 2 or 4 views (the mean's 1 / V must be exact)");
    if (!views_host || !flips_host) return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: null views_host or flips_host");
    if (c < 2 || c > RA_MAXC) return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: 2..4 classes");
    if (b <= 0 || lh <= 0 || lw <= 0 || ho <= 0 || wo <= 0)
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: b, lh, lw, ho and wo must be positive");
    if (const char* g = grid_error(ho, wo, wh, ww, sy, sx)) {
        snprintf(buf, sizeof(buf), "merge_argmax: %s", g);
        return vqseg_set_error(VQSEG_EINVAL, buf);
    }
    if (blend != VQSEG_BLEND_UNIFORM && blend != VQSEG_BLEND_LINEAR)
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: blend is 0 (uniform) or 1 (linear)");
    if ((long)lh * lw > (1L << 27) || (long)ho * wo > (1L << 30) || lh > (1 << 24) || lw > (1 << 24) || ho > (1 << 24) || wo > (1 << 24))
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: window logits above 2^27 pixels (32-bit offsets inside a window), an output above 2^30 or a side above 2^24");
    for (int v = 0; v < n_views; ++v) {
        if (!views_host[v]) return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: null view");
        if (flips_host[v] < 0 || flips_host[v] > 3)
            return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: a flip code is 0..3 (bit 0 columns, bit 1 rows)");
    }
    if ((target == nullptr) != (counts == nullptr))
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: target and counts go together");
    if (!label && !top && !counts) return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: null label, top and counts: nothing to compute");
    const bool planar = stride_px == 1 && stride_c == (int64_t)lh * lw;
    const bool interleaved = stride_c == 1 && stride_px == c;
    if (!planar && !interleaved)
        return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: layout must be planar (NCHW) or interleaved (channels_last) with dense rows");
    if (stride_b < (int64_t)c * lh * lw) return vqseg_set_error(VQSEG_EINVAL, "merge_argmax: window stride smaller than a window's logits");
    MergeArgs a = {};
    for (int v = 0; v < n_views; ++v) {
        a.view[v] = views_host[v];
        a.flip[v] = flips_host[v];
    }
    a.V = n_views;
    a.sb = stride_b, a.sc = stride_c, a.sp = stride_px;
    a.B = b, a.lh = lh, a.lw = lw;
    a.Ho = ho, a.Wo = wo, a.wh = wh, a.ww = ww, a.sy = sy, a.sx = sx;
    a.ny = win_count(ho, wh, sy), a.nx = win_count(wo, ww, sx);
    a.linear = blend == VQSEG_BLEND_LINEAR;
    a.vec = ((uintptr_t)label & 3u) == 0;
    a.label = label, a.top = top;
    a.target = reinterpret_cast<const long long*>(target);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    const hipError_t e = launch_merge_argmax(a, c, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        snprintf(buf, sizeof(buf), "merge_argmax_kernel: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

}  // extern "C"
