// render_kernels.hip -- the visualisation path's one kernel: labels, targets and the input image of a batch become the RGB bytes of a
// panel sheet in a single pass (vq_seg_amd/nnf.py: render_sheet; vq_seg_amd/utils/visualize.py; Predictor.render;
// CPSTrainer.example_image; evaluate.test_loop(visualize=...)).
//
// What it replaces: the logits and images copied off the device and a float64 numpy composition on the host.  Here the sources stay
// where they are -- the u8 labels nnf.resize_argmax wrote, the i64 targets, the f32 image -- and only the u8 sheet is written: 3 bytes
// per sheet pixel, against reads of 1 byte (label), 8 bytes (target) and a bilinear gather from the image per panel pixel.
//
// The sheet is (rows = B * Ho) x cols full-resolution pixels; image b takes rows b Ho .. (b + 1) Ho - 1 of every panel, a panel the
// columns x0 .. x0 + width - 1.  A full-resolution pixel (y, x) of panel p, with yy = y - b Ho and xx = x - x0:
//     image   v_c   = bil_mix(four taps through bil_src(yy, h, Ho), bil_src(xx, w, Wo))     (bilinear_device.h, align_corners = 0)
//     pred    pr    = pred[b][yy][xx];                    row(PRED)   = pr < C ? pr : 2 C   (the `ignore` row)
//     target  t     = target[b][min((int)(yy * ((float)ht / Ho)), ht - 1)][min((int)(xx * ((float)wt / Wo)), wt - 1)]   (ATen nearest)
//                                                          row(TARGET) = 0 <= t < C ? t : 2 C
//                                                          row(DETAIL) = pr >= C ? 2 C : pr != t ? pr + C : pr
//     IMAGE       colour = v                                                     (not clipped before a box mean, as the reference's sheet)
//     TARGET / PRED / DETAIL / FILL   colour = palette row (FILL: the fill colour)
//     MIX_*       colour_c = clip(v_c * (1.0f - alpha) + palette_f[row][c] * alpha, 0, 1)    two products, one add, no contraction; this clip
//                 keeps a NaN (x < 0 ? 0 : x > 1 ? 1 : x, as np.clip), so that a NaN reaches the box mean as it does in the reference
// Quantisation: q(x) = (int)floorf(clip(x, 0, 1) * 255.0f), with clip(x, 0, 1) = x > 0 ? (x < 1 ? x : 1) : 0 so that a NaN gives 0.
//   box2 off: a palette-row pixel writes the row's u8 colour (floor(colour * 255) in float64 on the host: float32(230 / 255) * 255 does
//             not floor to 230), every other pixel q(colour_c).
//   box2 on:  output pixel (Y, X) takes the full-resolution pixels (2 Y, 2 X), (2 Y, 2 X + 1), (2 Y + 1, 2 X), (2 Y + 1, 2 X + 1) = c00, c01,
//             c10, c11 -- each with its own panel and image -- and writes q(((c00 + c01) + (c10 + c11)) * 0.25f), f32 palette rows for
//             palette-row pixels; four pixels of the SAME palette row write that row's u8 colour (their mean is the colour itself).
//
// Work unit: the canvas is cut into groups of 4 adjacent output pixels of one row (12 bytes); a wave takes 64 consecutive groups -- a run
// of 256 pixels of one sheet row where the sheet is that wide, several whole rows where it is narrow, so that a 20-column sheet keeps its
// lanes busy as well -- and a lane one group: three aligned 4-byte stores when canvas and pitch are 4-byte aligned and all four pixels
// belong to panels, byte stores otherwise.  Only bytes of panel pixels are written.  Taps and weights are computed once per pixel for the
// three channels.  The panels (at most 8, sorted by x0 on the host) and the palette travel as kernel arguments; the panel of a column is
// found by 8 predicated compares without a branch, and the palette is put into LDS once per workgroup because it is indexed per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "bilinear_device.h"
#include "nn_kernels.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int RS_MAXP = 8, RS_MAXC = 4;
constexpr int RS_ROWS = 2 * RS_MAXC + 2;                    // class, wrong, ignore, fill
constexpr int RS_PX = 4;                                    // adjacent output pixels per lane
enum { RS_IMAGE = 0, RS_TARGET, RS_PRED, RS_DETAIL, RS_MIX_PRED, RS_MIX_DETAIL, RS_FILL, RS_KINDS };

struct RenderArgs {
    const float* image;
    long isb;                                               // batch stride in elements
    unsigned isc, isp;                                      // channel and pixel strides: offsets inside an image fit 32 bits (host check)
    int H, W;
    const uint8_t* pred;
    const long long* target;
    int Ht, Wt;
    int B, Ho, Wo, C;
    int np;
    int kind[RS_MAXP], x0[RS_MAXP], width[RS_MAXP];         // sorted by x0, disjoint
    float palf[RS_ROWS * 3];                                // rows 0 .. 2 C: the palette; row 2 C + 1: the fill colour
    unsigned palu[RS_ROWS];                                 // the same rows as bytes: r | g << 8 | b << 16
    float alpha;
    uint8_t* canvas;
    long pitch;
    int orows, ocols;                                       // canvas pixels (the sheet's, halved with box2)
    int vec;                                                // canvas and pitch 4-byte aligned
};

struct SheetPixel {
    float r, g, b;
    int row;                                                // >= 0: a palette row (r, g, b are its f32 colour); -1: computed; -2: no panel
};

__device__ __forceinline__ float clip01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }      // NaN -> 0
__device__ __forceinline__ float clip_keep_nan(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ unsigned quant(float x) { return (unsigned)(int)floorf(clip01(x) * 255.0f); }

// the colour of full-resolution sheet pixel (y, x); y < B * Ho
__device__ __forceinline__ SheetPixel sheet_pixel(const RenderArgs& a, const float* palf, unsigned y, unsigned x) {
#pragma clang fp contract(off)
    int kind = -1, xs = 0;
#pragma unroll
    for (int i = 0; i < RS_MAXP; ++i) {                     // panel arguments sit in scalar registers: compares and selects, no branch
        const bool in = i < a.np && x >= (unsigned)a.x0[i] && x < (unsigned)(a.x0[i] + a.width[i]);
        kind = in ? a.kind[i] : kind;
        xs = in ? a.x0[i] : xs;
    }
    SheetPixel px = {0.0f, 0.0f, 0.0f, -2};
    if (kind < 0) return px;
    const int C = a.C;
    if (kind == RS_FILL) {
        px.row = 2 * C + 1;
    } else {
        const unsigned b = y / (unsigned)a.Ho, yy = y - b * (unsigned)a.Ho, xx = x - (unsigned)xs;        // xx < Wo: a non-FILL panel is Wo wide
        const bool want_img = kind == RS_IMAGE || kind == RS_MIX_PRED || kind == RS_MIX_DETAIL;
        const bool want_pred = kind == RS_PRED || kind == RS_DETAIL || kind == RS_MIX_PRED || kind == RS_MIX_DETAIL;
        const bool want_tgt = kind == RS_TARGET || kind == RS_DETAIL || kind == RS_MIX_DETAIL;
        int row = -1;
        unsigned pr = 0;
        long long t = -1;
        if (want_pred) pr = a.pred[((long)b * a.Ho + yy) * a.Wo + xx];
        if (want_tgt) {
            const int ty = nearest_src((int)yy, a.Ht, a.Ho), tx = nearest_src((int)xx, a.Wt, a.Wo);
            t = a.target[((long)b * a.Ht + ty) * a.Wt + tx];
        }
        if (kind == RS_TARGET) row = t >= 0 && t < C ? (int)t : 2 * C;
        else if (kind == RS_PRED || kind == RS_MIX_PRED) row = pr < (unsigned)C ? (int)pr : 2 * C;
        else if (kind == RS_DETAIL || kind == RS_MIX_DETAIL) row = pr >= (unsigned)C ? 2 * C : ((long long)pr != t ? (int)pr + C : (int)pr);
        if (want_img) {
            int h0, h1, w0, w1;
            float lh, lw;
            bil_src((int)yy, a.H, a.Ho, 0, h0, h1, lh);
            bil_src((int)xx, a.W, a.Wo, 0, w0, w1, lw);
            const float* s = a.image + (long)b * a.isb;
            const unsigned W = (unsigned)a.W;
            const unsigned o00 = (h0 * W + w0) * a.isp, o01 = (h0 * W + w1) * a.isp, o10 = (h1 * W + w0) * a.isp, o11 = (h1 * W + w1) * a.isp;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned oc = c * a.isc;
                v[c] = bil_mix(s[o00 + oc], s[o01 + oc], s[o10 + oc], s[o11 + oc], lh, lw);
            }
            if (kind != RS_IMAGE) {
                const float keep = 1.0f - a.alpha;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = clip_keep_nan(v[c] * keep + palf[row * 3 + c] * a.alpha);
            }
            px.r = v[0], px.g = v[1], px.b = v[2], px.row = -1;
            return px;
        }
        px.row = row;
    }
    px.r = palf[px.row * 3], px.g = palf[px.row * 3 + 1], px.b = palf[px.row * 3 + 2];
    return px;
}

template <bool BOX2>
__global__ __launch_bounds__(256) void render_sheet_kernel(const RenderArgs a) {
#pragma clang fp contract(off)
    __shared__ float palf[RS_ROWS * 3];
    __shared__ unsigned palu[RS_ROWS];
    if (threadIdx.x < RS_ROWS * 3) palf[threadIdx.x] = a.palf[threadIdx.x];
    if (threadIdx.x < RS_ROWS) palu[threadIdx.x] = a.palu[threadIdx.x];
    __syncthreads();
    const unsigned G = ((unsigned)a.ocols + RS_PX - 1) / RS_PX;     // groups per canvas row
    const unsigned groups = G * (unsigned)a.orows;                   // < 2^31 (host check)
    for (unsigned first = blockIdx.x * 256u; first < groups; first += gridDim.x * 256u) {
        const unsigned gid = first + threadIdx.x;                    // a wave: 64 consecutive groups
        if (gid >= groups) continue;
        const unsigned Y = gid / G, X = (gid - Y * G) * RS_PX;
        unsigned rgb[RS_PX];
        bool have[RS_PX];
#pragma unroll
        for (int j = 0; j < RS_PX; ++j) {
            const unsigned xo = X + j;
            have[j] = false, rgb[j] = 0;
            if (xo >= (unsigned)a.ocols) continue;
            if (!BOX2) {
                const SheetPixel p = sheet_pixel(a, palf, Y, xo);
                if (p.row == -2) continue;
                have[j] = true;
                rgb[j] = p.row >= 0 ? palu[p.row] : quant(p.r) | (quant(p.g) << 8) | (quant(p.b) << 16);
            } else {
                const SheetPixel c00 = sheet_pixel(a, palf, 2 * Y, 2 * xo), c01 = sheet_pixel(a, palf, 2 * Y, 2 * xo + 1);
                if (c00.row == -2 || c01.row == -2) continue;         // the host admits no 2 x 2 block that is half inside the panels
                const SheetPixel c10 = sheet_pixel(a, palf, 2 * Y + 1, 2 * xo), c11 = sheet_pixel(a, palf, 2 * Y + 1, 2 * xo + 1);
                have[j] = true;
                if (c00.row >= 0 && c00.row == c01.row && c00.row == c10.row && c00.row == c11.row) rgb[j] = palu[c00.row];
                else
                    rgb[j] = quant(((c00.r + c01.r) + (c10.r + c11.r)) * 0.25f) | (quant(((c00.g + c01.g) + (c10.g + c11.g)) * 0.25f) << 8) |
                             (quant(((c00.b + c01.b) + (c10.b + c11.b)) * 0.25f) << 16);
            }
        }
        uint8_t* out = a.canvas + (long)Y * a.pitch + 3l * X;        // 12 bytes per group: 4-byte aligned when canvas and pitch are
        if (a.vec && have[0] && have[1] && have[2] && have[3]) {
            unsigned* o = reinterpret_cast<unsigned*>(out);
            o[0] = rgb[0] | (rgb[1] << 24);
            o[1] = (rgb[1] >> 8) | (rgb[2] << 16);
            o[2] = (rgb[2] >> 16) | (rgb[3] << 8);
        } else {
#pragma unroll
            for (int j = 0; j < RS_PX; ++j)
                if (have[j]) {
                    out[3 * j] = (uint8_t)rgb[j];
                    out[3 * j + 1] = (uint8_t)(rgb[j] >> 8);
                    out[3 * j + 2] = (uint8_t)(rgb[j] >> 16);
                }
        }
    }
}

}  // namespace vqseg

extern "C" {

int vqseg_render_sheet_u8(const float* image, int64_t stride_b, int64_t stride_c, int64_t stride_px, int h, int w, const uint8_t* pred,
                          const int64_t* target, int ht, int wt, int b, int ho, int wo, int c, const int* kinds_host, const int* x0_host,
                          const int* width_host, int n_panels, const float* palette_f_host, const uint8_t* palette_u8_host,
                          const float* fill_f_host, const uint8_t* fill_u8_host, float alpha, int box2, uint8_t* canvas, int64_t pitch,
                          int rows, int cols, void* stream) {
    using namespace vqseg;
#define RS_BAD(msg) return vqseg_set_error(VQSEG_EINVAL, "render_sheet: " msg)
    if (!canvas) RS_BAD("null canvas");
    if (n_panels < 1 || n_panels > RS_MAXP) RS_BAD("1..8 panels");
    if (!kinds_host || !x0_host || !width_host) RS_BAD("null kinds_host, x0_host or width_host");
    if (!palette_f_host || !palette_u8_host || !fill_f_host || !fill_u8_host) RS_BAD("null palette or fill colour");
    if (c < 2 || c > RS_MAXC) RS_BAD("2..4 classes");
    if (b <= 0 || ho <= 0 || wo <= 0 || rows <= 0 || cols <= 0) RS_BAD("b, ho, wo, rows and cols must be positive");
    if (ho > (1 << 24) || wo > (1 << 24) || (long)rows * cols > (1L << 30)) RS_BAD("a side above 2^24 or a sheet above 2^30 pixels");
    if ((long)b * ho != rows) RS_BAD("rows must be b * ho (the full-resolution sheet, before box2 halves it)");
    if (box2 && ((rows | cols) & 1)) RS_BAD("box2 needs a sheet of even height and width");
    const int orows = box2 ? rows / 2 : rows, ocols = box2 ? cols / 2 : cols;
    if (pitch < 3l * ocols) RS_BAD("pitch smaller than a canvas row (3 bytes per pixel)");
    RenderArgs a = {};
    bool need_img = false, need_pred = false, need_tgt = false;
    for (int i = 0; i < n_panels; ++i) {                    // insertion sort by x0
        const int k = kinds_host[i], x = x0_host[i], wd = width_host[i];
        if (k < 0 || k >= RS_KINDS) RS_BAD("a panel kind is 0..6 (IMAGE, TARGET, PRED, DETAIL, MIX_PRED, MIX_DETAIL, FILL)");
        if (x < 0 || wd <= 0 || (long)x + wd > cols) RS_BAD("a panel lies outside the canvas");
        if (k != RS_FILL && wd != wo) RS_BAD("every panel but FILL is wo wide");
        need_img |= k == RS_IMAGE || k == RS_MIX_PRED || k == RS_MIX_DETAIL;
        need_pred |= k == RS_PRED || k == RS_DETAIL || k == RS_MIX_PRED || k == RS_MIX_DETAIL;
        need_tgt |= k == RS_TARGET || k == RS_DETAIL || k == RS_MIX_DETAIL;
        int j = i;
        for (; j > 0 && a.x0[j - 1] > x; --j) a.kind[j] = a.kind[j - 1], a.x0[j] = a.x0[j - 1], a.width[j] = a.width[j - 1];
        a.kind[j] = k, a.x0[j] = x, a.width[j] = wd;
    }
    for (int i = 0; i + 1 < n_panels; ++i)
        if (a.x0[i] + a.width[i] > a.x0[i + 1]) RS_BAD("overlapping panels");
    if (box2)                                               // a 2 x 2 block lies inside the panels or outside them, never half
        for (int i = 0; i < n_panels; ++i) {
            const int end = a.x0[i] + a.width[i];
            if (((a.x0[i] & 1) && (i == 0 || a.x0[i - 1] + a.width[i - 1] != a.x0[i])) || ((end & 1) && (i + 1 == n_panels || a.x0[i + 1] != end)))
                RS_BAD("box2: a panel edge at an odd column needs the next panel to start there");
        }
    if (need_img) {
        if (!image) RS_BAD("an IMAGE or MIX panel needs the image (null)");
        if (h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24) || (long)h * w > (1L << 27)) RS_BAD("image height and width must be positive, at most 2^27 pixels");
        const bool planar = stride_px == 1 && stride_c == (int64_t)h * w;
        const bool interleaved = stride_c == 1 && stride_px == 3;
        if (!planar && !interleaved) RS_BAD("image layout must be planar (NCHW) or interleaved (channels_last) with dense rows");
        if (b > 1 && stride_b < (int64_t)3 * h * w) RS_BAD("image batch stride smaller than an image");
    }
    if (need_pred && !pred) RS_BAD("a PRED, DETAIL or MIX panel needs pred (null)");
    if (need_tgt) {
        if (!target) RS_BAD("a TARGET, DETAIL or MIX_DETAIL panel needs the target (null)");
        if (ht <= 0 || wt <= 0 || ht > (1 << 24) || wt > (1 << 24)) RS_BAD("target height and width must be positive, at most 2^24");
    }
#undef RS_BAD
    a.image = image, a.isb = stride_b, a.isc = (unsigned)stride_c, a.isp = (unsigned)stride_px, a.H = h, a.W = w;
    a.pred = pred, a.target = reinterpret_cast<const long long*>(target), a.Ht = ht, a.Wt = wt;
    a.B = b, a.Ho = ho, a.Wo = wo, a.C = c, a.np = n_panels;
    for (int r = 0; r < 2 * c + 2; ++r) {
        const float* f = r <= 2 * c ? palette_f_host + 3 * r : fill_f_host;
        const uint8_t* u = r <= 2 * c ? palette_u8_host + 3 * r : fill_u8_host;
        a.palf[3 * r] = f[0], a.palf[3 * r + 1] = f[1], a.palf[3 * r + 2] = f[2];
        a.palu[r] = (unsigned)u[0] | ((unsigned)u[1] << 8) | ((unsigned)u[2] << 16);
    }
    a.alpha = alpha;
    a.canvas = canvas, a.pitch = pitch, a.orows = orows, a.ocols = ocols;
    a.vec = (((uintptr_t)canvas | (uintptr_t)pitch) & 3u) == 0;
    const long groups = (long)((ocols + RS_PX - 1) / RS_PX) * orows;
    long blocks = (groups + 255) / 256;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (box2) hipLaunchKernelGGL((render_sheet_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((render_sheet_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[160];
        snprintf(buf, sizeof(buf), "render_sheet_kernel: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

}  // extern "C"
