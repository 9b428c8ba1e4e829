// photometric_kernels.hip -- the photometric strong augmentation (vq_seg_amd/data/augmentations.py: photometric / StrongPhotometric;
// CPSConfig.hard_aug = "photometric"): brightness, contrast, saturation, hue, grayscale and a Gaussian blur of an RGB f32 batch, one
// parameter row per sample, in one pass over the batch (plus a reduction pass when a sample's contrast is on).
//
// The definition is include/vqseg.h's (vqseg_photometric_f) and tests/photometric_cases.py restates it in float64.  No reference
// counterpart: the reference's hard augmentation stops at CutMix.  All arithmetic is f32; an op whose parameter has its identity value
// is skipped, and a sample whose six parameters are all identity is copied by bits.
//
// Mean pass (only when some sample of the launch has c != 1): the contrast op needs m = the mean over the sample's pixels of
// g(clamp(b p)).  A sample's pixels are dealt to P = photometric_mean_blocks(h w) workgroups of 256 threads, pixel q to thread
// q % (256 P); a thread adds its pixels in order, a wave folds its 64 sums with shuffles, the workgroup its 4 wave sums pairwise, and the
// result goes to partials[sample][block].  The main pass folds the P <= 64 partials with one more shuffle tree, in every wave, and
// divides by h w.  P, the dealing and every order of addition depend on h w alone: no atomics, two calls agree bit for bit, and a
// sample's m does not depend on the batch it travels in.
//
// Main pass: a workgroup owns a 16 x 64 tile of output pixels of one sample.
//   fully-identity sample    a copy of the tile
//   sigma = 0                steps 1-5 per pixel, registers only
//   sigma > 0, R = ceil(3 sigma)   steps 1-5 for the tile plus an R-wide halo -> LDS A [3][16 + 2R][64 + 2R] (halo coordinates are
//                            reflected BEFORE the load, so the halo holds jittered pixels of the image itself); row pass A -> LDS B
//                            [3][16 + 2R][64]; column pass B -> global
// Tile choice: at R = 6 the two buffers take (28 * 76 + 28 * 64) * 12 B = 47 KB, three workgroups per CU (160 KB), which is what hides
// one workgroup's barrier-separated phases (load + colour math / row pass / column pass + store) under another's; at R = 8 they take
// 54 KB, inside the 64 KB a launch gets without asking.  The price is the halo's colour math: 28 * 76 / (16 * 64) = 2.1 x at R = 6, where
// a 32 x 64 tile pays 1.6 x but stages 74 KB and leaves two workgroups per CU.  The colour math is a few dozen f32 operations per
// pixel against 24 B of HBM traffic, so the smaller tile was taken.  LDS is sized per launch from the largest R among its samples.
// Access shape: consecutive lanes take consecutive pixels of a tile row in every phase.  Planar (NCHW): a wave's load or store of a
// plane is one dense 256-byte row segment (304 B with the halo).  Interleaved (channels_last, 12-byte pixels): the wave's three
// dword accesses cover one dense 768-byte segment between them.  LDS rows are walked with stride 1 across lanes: no bank conflicts.
// The blur adds the two taps of equal weight first (v[-i] + v[i]) and accumulates from the outermost pair inwards, smallest terms first.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int PHOTO_ARG_SAMPLES = 32;                       // samples per launch: 32 parameter rows = 1.75 KiB of kernel arguments
constexpr int PHOTO_MAX_R = 8, PHOTO_TAPS = PHOTO_MAX_R + 1;
constexpr int PHOTO_TH = 16, PHOTO_TW = 64;                 // the output tile
constexpr int PHOTO_MEAN_PIXELS = 4096;                     // pixels per workgroup of the mean pass before a second one is added ...
constexpr int PHOTO_MEAN_MAX_BLOCKS = 64;                   // ... up to one partial per lane of the folding wave

struct PhotoArgs {
    float b[PHOTO_ARG_SAMPLES], c[PHOTO_ARG_SAMPLES], sat[PHOTO_ARG_SAMPLES], hue[PHOTO_ARG_SAMPLES];
    int gray[PHOTO_ARG_SAMPLES], radius[PHOTO_ARG_SAMPLES];
    float taps[PHOTO_ARG_SAMPLES][PHOTO_TAPS];              // w_0 .. w_R (w_-i = w_i), zeros beyond
};

__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ inline float gray_of(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

struct Rgb {
    float r, g, b;
};

__device__ inline Rgb load_rgb(const float* px, long stride_p) { return {px[0], px[stride_p], px[2 * stride_p]}; }
__device__ inline void store_rgb(float* px, long stride_p, Rgb v) { px[0] = v.r, px[stride_p] = v.g, px[2 * stride_p] = v.b; }

__device__ inline Rgb brightness(Rgb p, float b) { return {clamp01(b * p.r), clamp01(b * p.g), clamp01(b * p.b)}; }

__device__ inline Rgb hue_shift(Rgb p, float hue) {
    const float mx = fmaxf(p.r, fmaxf(p.g, p.b)), mn = fminf(p.r, fminf(p.g, p.b));
    const float v = mx, cr = mx - mn;
    const float s = cr == 0.0f ? 0.0f : cr / mx;
    const float d = cr == 0.0f ? 1.0f : cr;
    const float rc = (mx - p.r) / d, gc = (mx - p.g) / d, bc = (mx - p.b) / d;
    const float h6 = mx == p.r ? bc - gc : mx == p.g ? 2.0f + rc - bc : 4.0f + gc - rc;
    float h = h6 / 6.0f + 1.0f;
    h = h - floorf(h);
    h = h + hue;
    h = h - floorf(h);                                      // in [0, 1]; 1.0 (a rounded-away tiny negative) lands in sector 0 with f = 0
    const float h6b = 6.0f * h;
    const float fi = floorf(h6b);
    const float f = h6b - fi;
    const int i = (int)fi % 6;
    const float p_ = clamp01(v * (1.0f - s)), q = clamp01(v * (1.0f - f * s)), t = clamp01(v * (1.0f - (1.0f - f) * s));
    switch (i) {
        case 0: return {v, t, p_};
        case 1: return {q, v, p_};
        case 2: return {p_, v, t};
        case 3: return {p_, q, v};
        case 4: return {t, p_, v};
        default: return {v, p_, q};
    }
}

// steps 1-5 of the definition for one pixel; `m`: the sample's mean (read only when c != 1)
__device__ inline Rgb colour_ops(Rgb p, float b, float c, float sat, float hue, int gray, float m) {
    if (b != 1.0f) p = brightness(p, b);
    if (c != 1.0f) {
        const float o = (1.0f - c) * m;
        p = {clamp01(c * p.r + o), clamp01(c * p.g + o), clamp01(c * p.b + o)};
    }
    if (sat != 1.0f) {
        const float o = (1.0f - sat) * gray_of(p.r, p.g, p.b);
        p = {clamp01(sat * p.r + o), clamp01(sat * p.g + o), clamp01(sat * p.b + o)};
    }
    if (hue != 0.0f) p = hue_shift(p, hue);
    if (gray) {
        const float g = gray_of(p.r, p.g, p.b);
        p = {g, g, g};
    }
    return p;
}

__device__ inline float wave_sum_all(float v) {             // every lane gets the same bits: a + b is commutative at each level
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// grid (P, samples of the launch): partials[(s0 + i) * P + j] = the sum of g(clamp(b p)) over the pixels q = j * 256 + t + k * 256 P
__global__ __launch_bounds__(256) void photometric_mean_kernel(PhotoArgs a, const float* __restrict__ src, long stride_s, long stride_p,
                                                               long stride_px, long pixels, float* __restrict__ partials) {
    __shared__ float s_part[4];
    const int i = blockIdx.y, P = gridDim.x;
    const float c = a.c[i], b = a.b[i];
    if (c == 1.0f) return;                                  // uniform: this sample's mean is never read
    const float* img = src + i * stride_s;
    float sum = 0.0f;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < pixels; q += (long)P * 256) {
        Rgb p = load_rgb(img + q * stride_px, stride_p);
        if (b != 1.0f) p = brightness(p, b);
        sum += gray_of(p.r, p.g, p.b);
    }
    sum = wave_sum_all(sum);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)i * P + blockIdx.x] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// grid (tiles_x, tiles_y, samples of the launch); dynamic LDS: 3 * (TH + 2 Rmax) * (2 TW + 2 Rmax) floats, Rmax over the launch
__global__ __launch_bounds__(256) void photometric_kernel(PhotoArgs a, const float* __restrict__ src, float* __restrict__ out, long stride_s,
                                                          long stride_p, long stride_px, int h, int w, const float* __restrict__ partials,
                                                          int P, float* __restrict__ means) {
    extern __shared__ float lds[];
    const int i = blockIdx.z;
    const float b = a.b[i], c = a.c[i], sat = a.sat[i], hue = a.hue[i];
    const int gray = a.gray[i], R = a.radius[i];
    const int x0 = blockIdx.x * PHOTO_TW, y0 = blockIdx.y * PHOTO_TH;
    const float* img = src + i * stride_s;
    float* dst = out + i * stride_s;
    const int lx = threadIdx.x & (PHOTO_TW - 1), ly = threadIdx.x >> 6;      // 4 tile rows per sweep of the workgroup
    const bool colour = b != 1.0f || c != 1.0f || sat != 1.0f || hue != 0.0f || gray != 0;
    if (!colour && R == 0) {                                // the whole row is identity: by bits
        const int x = x0 + lx;
        for (int y = y0 + ly; y < y0 + PHOTO_TH && y < h && x < w; y += 4) {
            const long at = ((long)y * w + x) * stride_px;
            store_rgb(dst + at, stride_p, load_rgb(img + at, stride_p));
        }
        return;
    }
    float m = 0.0f;
    if (c != 1.0f) {                                        // fold the sample's partials: the same tree in every wave of every workgroup
        const int l = threadIdx.x & 63;
        m = wave_sum_all(l < P ? partials[(long)i * P + l] : 0.0f) / (float)((long)h * w);
        if (means && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) means[i] = m;
    }
    if (R == 0) {
        const int x = x0 + lx;
        for (int y = y0 + ly; y < y0 + PHOTO_TH && y < h && x < w; y += 4) {
            const long at = ((long)y * w + x) * stride_px;
            store_rgb(dst + at, stride_p, colour_ops(load_rgb(img + at, stride_p), b, c, sat, hue, gray, m));
        }
        return;
    }
    const int tw = w - x0 < PHOTO_TW ? w - x0 : PHOTO_TW, th = h - y0 < PHOTO_TH ? h - y0 : PHOTO_TH;     // the tile's part inside the image
    const int SW = PHOTO_TW + 2 * R, SH = PHOTO_TH + 2 * R;
    float* A = lds;                                         // [3][SH][SW]: jittered pixels, tile + halo
    float* B = lds + 3 * SH * SW;                           // [3][SH][TW]: after the row pass
    // stage: staged pixel (py, px) is image pixel (y0 - R + py, x0 - R + px) reflected into the image.  Only what an output pixel of
    // the image reads is loaded (px < tw + 2R, py < th + 2R): R <= min(h, w) - 1 then makes ONE reflection land inside the image
    for (int idx = threadIdx.x; idx < SH * SW; idx += 256) {
        const int py = idx / SW, px = idx - py * SW;
        Rgb p = {0.0f, 0.0f, 0.0f};
        if (px < tw + 2 * R && py < th + 2 * R) {
            int gx = x0 - R + px, gy = y0 - R + py;
            gx = gx < 0 ? -gx : gx >= w ? 2 * (w - 1) - gx : gx;
            gy = gy < 0 ? -gy : gy >= h ? 2 * (h - 1) - gy : gy;
            p = load_rgb(img + ((long)gy * w + gx) * stride_px, stride_p);
            if (colour) p = colour_ops(p, b, c, sat, hue, gray, m);
        }
        A[idx] = p.r, A[SH * SW + idx] = p.g, A[2 * SH * SW + idx] = p.b;
    }
    __syncthreads();
    float tap[PHOTO_TAPS];
#pragma unroll
    for (int k = 0; k < PHOTO_TAPS; ++k) tap[k] = a.taps[i][k];
    // row pass: a wave takes one row of one plane per sweep
    for (int idx = threadIdx.x; idx < 3 * SH * PHOTO_TW; idx += 256) {
        const int row = idx >> 6, x = idx & (PHOTO_TW - 1);
        const float* v = A + row * SW + x + R;              // the centre tap
        float acc = 0.0f;
#pragma unroll
        for (int k = PHOTO_MAX_R; k >= 1; --k)              // (unrolled over the largest radius: the taps stay in registers)
            if (k <= R) acc += tap[k] * (v[-k] + v[k]);
        B[idx] = acc + tap[0] * v[0];
    }
    __syncthreads();
    const int x = x0 + lx;
    for (int ty = ly; ty < th && x < w; ty += 4) {
        float o[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const float* v = B + (p * SH + ty + R) * PHOTO_TW + lx;
            float acc = 0.0f;
#pragma unroll
            for (int k = PHOTO_MAX_R; k >= 1; --k)
                if (k <= R) acc += tap[k] * (v[-k * PHOTO_TW] + v[k * PHOTO_TW]);
            o[p] = acc + tap[0] * v[0];
        }
        store_rgb(dst + ((long)(y0 + ty) * w + x) * stride_px, stride_p, {o[0], o[1], o[2]});
    }
}

static int photo_fail(const char* what) {
    char buf[200];
    snprintf(buf, sizeof(buf), "photometric: %s", what);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

static int photo_mean_blocks(int64_t pixels) {
    const int64_t p = (pixels + PHOTO_MEAN_PIXELS - 1) / PHOTO_MEAN_PIXELS;
    return (int)(p < 1 ? 1 : p > PHOTO_MEAN_MAX_BLOCKS ? PHOTO_MEAN_MAX_BLOCKS : p);
}

}  // namespace vqseg

extern "C" {

int vqseg_photometric_mean_blocks(int64_t pixels) { return pixels <= 0 ? vqseg::photo_fail("pixels must be positive") : vqseg::photo_mean_blocks(pixels); }

int vqseg_photometric_f(const float* src, float* out, int n, int h, int w, int64_t stride_s, int64_t stride_p, int64_t stride_px,
                        const float* params_host, const int32_t* radii_host, const float* taps_host, float* partials, float* means,
                        void* stream) {
    using namespace vqseg;
    if (n <= 0 || h <= 0 || w <= 0) return photo_fail("n, h and w must be positive");
    if (h > (1 << 20) || w > (1 << 20) || (long)h * w > (1L << 28)) return photo_fail("a side above 2^20 or a sample larger than 2^28 pixels");
    if (!src || !out || !params_host || !radii_host || !taps_host) return photo_fail("null src, out, params_host, radii_host or taps_host");
    if (src == out) return photo_fail("out of place only (a blurred pixel reads neighbours that another workgroup may have written)");
    const long pixels = (long)h * w;
    const bool planar = stride_px == 1 && stride_p == pixels;
    const bool interleaved = stride_p == 1 && stride_px == 3;
    if (!planar && !interleaved) return photo_fail("layout must be planar (NCHW) or interleaved (channels_last) RGB with dense rows");
    if (n > 1 && stride_s < 3 * pixels) return photo_fail("sample stride smaller than a sample");
    bool any_mean = false;
    for (long s = 0; s < n; ++s) {
        const float* p = params_host + 6 * s;
        for (int k = 0; k < 6; ++k)
            if (!(p[k] - p[k] == 0.0f)) return photo_fail("a parameter is not finite");
        if (p[0] < 0.0f || p[1] < 0.0f || p[2] < 0.0f) return photo_fail("brightness, contrast and saturation factors must be >= 0");
        if (!(p[3] >= -0.5f && p[3] <= 0.5f)) return photo_fail("hue must lie in [-0.5, 0.5]");
        if (p[4] != 0.0f && p[4] != 1.0f) return photo_fail("gray must be 0 or 1");
        if (p[5] < 0.0f) return photo_fail("sigma must be >= 0");
        const int r = radii_host[s];
        if (r < 0 || r > PHOTO_MAX_R) return photo_fail("a blur radius outside 0..8");
        if ((r == 0) != (p[5] == 0.0f)) return photo_fail("radius 0 goes with sigma 0 and only with it");
        if (r > (h < w ? h : w) - 1) return photo_fail("a blur radius above min(h, w) - 1 (one reflection must land inside the image)");
        for (int k = 0; k < PHOTO_TAPS; ++k) {
            const float t = taps_host[PHOTO_TAPS * s + k];
            if (!(t >= 0.0f && t <= 1.0f) || (k > r && t != 0.0f)) return photo_fail("taps must lie in [0, 1] and be 0 beyond the radius");
        }
        any_mean = any_mean || p[1] != 1.0f;
    }
    if (any_mean && !partials) return photo_fail("a contrast factor other than 1 needs the partials workspace (n * vqseg_photometric_mean_blocks floats)");
    const int P = photo_mean_blocks(pixels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 tiles((unsigned)((w + PHOTO_TW - 1) / PHOTO_TW), (unsigned)((h + PHOTO_TH - 1) / PHOTO_TH), 1);
    if (tiles.y > 65535u) return photo_fail("more than 65535 rows of tiles");
    for (int s0 = 0; s0 < n; s0 += PHOTO_ARG_SAMPLES) {
        const int nb = n - s0 < PHOTO_ARG_SAMPLES ? n - s0 : PHOTO_ARG_SAMPLES;
        PhotoArgs a = {};
        int rmax = 0;
        bool mean = false;
        for (int i = 0; i < nb; ++i) {
            const float* p = params_host + 6 * (long)(s0 + i);
            a.b[i] = p[0], a.c[i] = p[1], a.sat[i] = p[2], a.hue[i] = p[3], a.gray[i] = p[4] != 0.0f, a.radius[i] = radii_host[s0 + i];
            for (int k = 0; k < PHOTO_TAPS; ++k) a.taps[i][k] = taps_host[PHOTO_TAPS * (long)(s0 + i) + k];
            rmax = a.radius[i] > rmax ? a.radius[i] : rmax;
            mean = mean || p[1] != 1.0f;
        }
        const float* in = src + (long)s0 * stride_s;
        float* part = partials ? partials + (long)s0 * P : nullptr;
        hipError_t e = hipSuccess;
        if (mean) {
            hipLaunchKernelGGL(photometric_mean_kernel, dim3((unsigned)P, (unsigned)nb), dim3(256), 0, st, a, in, (long)stride_s, (long)stride_p,
                               (long)stride_px, pixels, part);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            const size_t lds = rmax ? sizeof(float) * 3 * (PHOTO_TH + 2 * rmax) * (2 * PHOTO_TW + 2 * rmax) : 0;     // <= 54 KB at R = 8
            hipLaunchKernelGGL(photometric_kernel, dim3(tiles.x, tiles.y, (unsigned)nb), dim3(256), lds, st, a, in, out + (long)s0 * stride_s,
                               (long)stride_s, (long)stride_p, (long)stride_px, h, w, part, P, means ? means + s0 : nullptr);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            char buf[160];
            snprintf(buf, sizeof(buf), "photometric_kernel: %s", hipGetErrorString(e));
            return vqseg_set_error((int)e, buf);
        }
    }
    return 0;
}

}  // extern "C"
