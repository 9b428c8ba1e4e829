// data_kernels.hip -- batch assembly of the device-resident data loader (vq_seg_amd/data/device_loader.py), and the box mix of
// CutMix / CutOut (vq_seg_amd/data/augmentations.py; second half of this file).
//
// Reference: BaseDataset.__getitem__ (data/dataset.py:47-57) turns a decoded, resized uint8 HWC image into float32 / 255
// (TF.to_tensor) and returns the uint8 mask as it is; the training loop then maps the mask through img_to_label
// (utils/seg_tools.py:3-8, chained torch.where passes) and copies the batch to the device.  The loader decodes and resizes every
// file once, on the host, into a ragged uint8 cache in HBM; per batch this file gathers the B samples from that cache and does
// the rest in one launch:
//     img_out[s, y, x, c]  = f32_lut[img_cache[img_off[s] + (y * w + x) * 3 + c]]      (NHWC = torch channels_last)
//     target_out[s, y, x]  = mask_cache[mask_off[s] + y * mw + x]
//     label_out[s, y, x]   = label_lut[target_out[s, y, x]]
// Both tables are built on the host with the reference's own torch ops over all 256 byte values, so the result is exact by
// construction.  HBM-bound: per image byte 1 B read + 4 B written, per mask byte 1 B read + 1 B (+ 8 B label) written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "nn_kernels.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

constexpr int BATCH_ARG_SAMPLES = 64;                       // samples per launch: 2 x 64 offsets = 1 KiB of kernel arguments

struct BatchOffsets {
    int64_t img[BATCH_ARG_SAMPLES];
    int64_t mask[BATCH_ARG_SAMPLES];
};

// Work unit: a 1 KiB tile of one sample (the last tile of a sample may be partial), one per wave and iteration -- 16 bytes per
// lane.  `chunk` c counts 16-byte units over the launch's samples, ceil(bytes / 1024) tiles of 64 units each per sample; the grid
// stride is a multiple of 64, so the 64 lanes of a wave always share one tile, and the branch below is uniform across the wave.
// A whole tile whose sample output is 16-byte aligned (`vec`: every pointer / offset aligned, and s * bytes % 4 == 0) takes the
// vector body: lane l takes the 4-byte words l, l + 64, l + 128, l + 192, so every 16-byte f32 store instruction of the wave writes
// 1 KiB contiguously (one 16-byte load per lane instead leaves its four stores 64 bytes apart: 1.5x slower, profiles/data_path.md).
// Any other tile (a partial last tile, a sample at an unaligned output position) goes byte by byte, still coalesced: byte
// t + l + 64 j of the tile in step j.
__global__ __launch_bounds__(256) void batch_u8_kernel(BatchOffsets off, int nb, int vec, const uint8_t* __restrict__ img_cache,
                                                       const uint8_t* __restrict__ mask_cache, long img_bytes, long mask_bytes,
                                                       const float* __restrict__ f32_lut, const int64_t* __restrict__ label_lut,
                                                       float* __restrict__ img_out, uint8_t* __restrict__ target_out,
                                                       int64_t* __restrict__ label_out) {
    __shared__ float lut_f[256];
    __shared__ int64_t lut_l[256];
    lut_f[threadIdx.x] = f32_lut[threadIdx.x];
    if (label_lut) lut_l[threadIdx.x] = label_lut[threadIdx.x];
    __syncthreads();
    const long stride = (long)gridDim.x * 256;
    const long first = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_img = (img_bytes + 1023) / 1024 * 64, per_mask = (mask_bytes + 1023) / 1024 * 64;
    for (long c = first; c < per_img * nb; c += stride) {
        const int s = (int)(c / per_img);
        const long q = (c - s * per_img) * 16;
        const long t = q & ~1023L;
        const int l = (int)(q & 1023) >> 4;
        const uint8_t* src = img_cache + off.img[s] + t;
        float* dst = img_out + s * img_bytes + t;
        if (vec && t + 1024 <= img_bytes && ((s * img_bytes) & 3) == 0) {
            unsigned w4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w4[k] = *reinterpret_cast<const unsigned*>(src + 4 * l + 256 * k);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned u = w4[k];
                f32x4 o;
                o[0] = lut_f[u & 255u], o[1] = lut_f[(u >> 8) & 255u], o[2] = lut_f[(u >> 16) & 255u], o[3] = lut_f[u >> 24];
                *reinterpret_cast<f32x4*>(dst + 4 * l + 256 * k) = o;
            }
        } else {
            for (int j = 0; j < 16; ++j) {
                const long b = l + 64 * j;
                if (t + b < img_bytes) dst[b] = lut_f[src[b]];
            }
        }
    }
    if (!mask_cache) return;
    for (long c = first; c < per_mask * nb; c += stride) {
        const int s = (int)(c / per_mask);
        const long q = (c - s * per_mask) * 16;
        const long t = q & ~1023L;
        const int l = (int)(q & 1023) >> 4;
        const uint8_t* src = mask_cache + off.mask[s] + t;
        const long o = s * mask_bytes + t;
        if (vec && t + 1024 <= mask_bytes && ((s * mask_bytes) & 3) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long e = 4 * l + 256 * k;
                const unsigned u = *reinterpret_cast<const unsigned*>(src + e);
                *reinterpret_cast<unsigned*>(target_out + o + e) = u;
                if (label_out) {
                    i64x2 a, b;
                    a[0] = lut_l[u & 255u], a[1] = lut_l[(u >> 8) & 255u], b[0] = lut_l[(u >> 16) & 255u], b[1] = lut_l[u >> 24];
                    reinterpret_cast<i64x2*>(label_out + o + e)[0] = a;
                    reinterpret_cast<i64x2*>(label_out + o + e)[1] = b;
                }
            }
        } else {
            for (int j = 0; j < 16; ++j) {
                const long b = l + 64 * j;
                if (t + b < mask_bytes) {
                    const uint8_t u = src[b];
                    target_out[o + b] = u;
                    if (label_out) label_out[o + b] = lut_l[u];
                }
            }
        }
    }
}

// ---- box mix (vq_seg_amd/data/augmentations.py: CutMix / CutOut / augmentation; the CPS step's strong augmentation) ---------------
//
// Reference: CutMix.__call__ / augmentation() (data/augmentations.py:11-30, 62-73) compute batch[i] * mask + batch[(i + 1) % B] * (1 - mask)
// with a 0 / 1 box mask per sample of the batch, in Python.  With a 0 / 1 mask that arithmetic is a selection, and this kernel does it
// as one: out[s, p, y, x] = inside(box[s], y, x) ? (MIX: src[(s + 1) % n, p, y, x] | FILL: fill) : src[s, p, y, x], by BITS (no
// arithmetic), so float and integer tensors of the same element width share one instantiation and -0.0 / NaN payloads pass unchanged.
// HBM-bound: per element one read (of the sample or of its partner, never both for a whole 16-byte unit outside / inside the box) and
// one write, 2 x sizeof(element) bytes -- 8 B per f32, 16 B per int64 label, 4 B per bf16, 2 B per uint8.
//
// A sample is a dense run of `elems` = planes * h * w elements in either layout; it is walked as `lines` of `line` elements: planar
// (NCHW, 3-D labels) planes * h lines of w elements, interleaved (channels_last) h lines of w * planes.  Element f lies in line f / line,
// image row (f / line) % h, and in the box iff that row is in [y1, y1 + ch) and f % line in [x1 * g, (x1 + cw) * g), g = elements per pixel.
// Work unit as in batch_u8_kernel: a 1 KiB tile of one sample per wave and iteration.  A whole tile of a 16-byte aligned sample takes
// one 16-byte load and store per lane (contiguous across the wave); each element of the unit is selected on its own, so a box edge (or
// a line end) inside a unit -- the rule with 12-byte channels_last f32 pixels -- is exact.  A sample's partial last tile, and every
// tile of a sample that does not start on a 16-byte boundary, goes element by element, lane l taking elements l, l + 64, ... of the tile.
constexpr int BOX_MODE_MIX = 0, BOX_MODE_FILL = 1;

struct BoxArgs {                                            // 1 KiB of kernel arguments: BATCH_ARG_SAMPLES boxes
    int y1[BATCH_ARG_SAMPLES], x1[BATCH_ARG_SAMPLES], ch[BATCH_ARG_SAMPLES], cw[BATCH_ARG_SAMPLES];
};

template <typename T>
__global__ __launch_bounds__(256) void box_mix_kernel(BoxArgs box, int s0, int nb, int n, int mode, int vec, const T* __restrict__ src,
                                                      T* __restrict__ out, long stride_s, long elems, long line, int h, int g, T fill) {
    constexpr int K = 16 / (int)sizeof(T);                  // elements per 16-byte unit
    constexpr long TILE = 64L * K;                          // elements per 1 KiB tile
    union Unit {
        uint4 v;
        T e[K];
    };
    const long stride = (long)gridDim.x * 256;
    const long per = (elems + TILE - 1) / TILE * 64;        // units per sample, whole tiles
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < per * nb; c += stride) {
        const int i = (int)(c / per);
        const long u = c - i * per;
        const long t = (u >> 6) * TILE;
        const int l = (int)(u & 63);
        const long s = s0 + i, p = s + 1 == n ? 0 : s + 1;  // the partner may lie in another launch's block: src is the whole tensor
        const T* a = src + s * stride_s;
        const T* b = src + p * stride_s;
        T* o = out + s * stride_s;
        const int y1 = box.y1[i], y2 = y1 + box.ch[i];
        const long e1 = (long)box.x1[i] * g, e2 = e1 + (long)box.cw[i] * g;
        if (vec && ((s * stride_s * (long)sizeof(T)) & 15) == 0 && t + TILE <= elems) {
            const long f = t + (long)l * K;
            Unit ua;
            ua.v = *reinterpret_cast<const uint4*>(a + f);
            const long ln = f / line;
            long pos = f - ln * line;
            int y = (int)(ln % h);
            unsigned m = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                m |= (unsigned)(y >= y1 && y < y2 && pos >= e1 && pos < e2) << k;
                if (++pos == line) {
                    pos = 0;
                    if (++y == h) y = 0;
                }
            }
            if (m) {
                if (mode == BOX_MODE_FILL) {
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if ((m >> k) & 1u) ua.e[k] = fill;
                } else if (((p * stride_s * (long)sizeof(T)) & 15) == 0) {
                    Unit ub;
                    ub.v = *reinterpret_cast<const uint4*>(b + f);
#pragma unroll
                    for (int k = 0; k < K; ++k) ua.e[k] = ((m >> k) & 1u) ? ub.e[k] : ua.e[k];
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if ((m >> k) & 1u) ua.e[k] = b[f + k];
                }
            }
            *reinterpret_cast<uint4*>(o + f) = ua.v;
        } else {
            for (int j = 0; j < K; ++j) {
                const long f = t + l + 64L * j;
                if (f >= elems) break;
                const long ln = f / line;
                const long pos = f - ln * line;
                const int y = (int)(ln % h);
                const bool in = y >= y1 && y < y2 && pos >= e1 && pos < e2;
                o[f] = in ? (mode == BOX_MODE_FILL ? fill : b[f]) : a[f];
            }
        }
    }
}

template <typename T>
static hipError_t launch_box_mix(const BoxArgs& box, int s0, int nb, int n, int mode, int vec, const void* src, void* out, long stride_s,
                                 long elems, long line, int h, int g, unsigned long long fill_bits, hipStream_t st) {
    constexpr long TILE = 64L * (16 / (long)sizeof(T));
    long blocks = ((elems + TILE - 1) / TILE * nb + 3) / 4;  // 4 waves per workgroup, one tile per wave and iteration
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(box_mix_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, box, s0, nb, n, mode, vec, static_cast<const T*>(src),
                       static_cast<T*>(out), stride_s, elems, line, h, g, (T)fill_bits);
    return hipGetLastError();
}

// ---- affine warp (vq_seg_amd/data/augmentations.py: similarity_transform / inverse_similarity_transform / warp_batch; the CPS step's
// easy augmentation) -------------------------------------------------------------------------------------------------------------------
//
// Reference: similarity_transform / inverse_similarity_transform (data/augmentations.py:108-148) flip and TF.rotate a batch; on tensors
// TF.rotate is F.grid_sample on an affine grid (align_corners=False, zero padding).  In pixel space that is, for output pixel (x, y) of an
// h x w image with cx = (w - 1) / 2, cy = (h - 1) / 2, dx = x - cx, dy = y - cy and the sample's 2 x 2 matrix M:
//     xs = (M00 * dx + M01 * dy) + cx        ys = (M10 * dx + M11 * dy) + cy          (f32, this order, no FMA contraction)
// cx, cy, dx, dy are exact in f32, so for M with entries in {0, +-1} (identity, flips, quarter turns) xs and ys are exact integers.
//   BILINEAR (f32, bf16): taps (x0, y0) = floor(xs, ys) and its right / lower neighbours, weights from fx = xs - x0, fy = ys - y0,
//     accumulated in f32 in the order 00, 01, 10, 11; bf16 rounded once (nearest even).  A tap outside the image contributes nothing
//     (zero padding) and a tap whose weight is exactly zero is not read; with fx == fy == 0 the one tap is copied by BITS, so identity,
//     flips and quarter turns pass NaN payloads, infinities and -0.0 through as the box mix does.
//   NEAREST (1 / 2 / 4 / 8-byte elements, by bits): the source pixel is (rintf(xs), rintf(ys)) -- round half to even, as grid_sample --
//     and a source outside the image gives `fill`.
// A gather bound by HBM / L2: one read and one write per element when the source footprint stays in cache.  A 256-thread workgroup
// takes a 2-D tile of OUTPUT pixels (16 x 16, or 32 x 8 / 64 x 4 for pixels of <= 4 / <= 2 bytes, so a tile row stays >= 64 bytes of
// coalesced stores): under a rotation the tile's source footprint is a rotated rectangle whose cache lines are reused by the tile's
// rows, where 256 pixels of one output row would touch a new line per pixel.  Coordinates and weights are computed once per pixel and
// applied to all its planes.  The matrices travel as kernel arguments, BATCH_ARG_SAMPLES per launch.
constexpr int WARP_BILINEAR = 0, WARP_NEAREST = 1;

struct WarpArgs {                                           // 1 KiB of kernel arguments: BATCH_ARG_SAMPLES 2 x 2 matrices
    float m00[BATCH_ARG_SAMPLES], m01[BATCH_ARG_SAMPLES], m10[BATCH_ARG_SAMPLES], m11[BATCH_ARG_SAMPLES];
};

__device__ inline float warp_value(uint32_t bits) { return __uint_as_float(bits); }
__device__ inline float warp_value(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }     // bf16

template <typename T>
__device__ inline T warp_bits(float v) {
    uint32_t u = __float_as_uint(v);
    if constexpr (sizeof(T) == 4) {
        return u;
    } else {                                                // bf16, round to nearest even; a NaN stays a (quiet) NaN
        if ((u & 0x7fffffffu) > 0x7f800000u) return (T)((u >> 16) | 0x40u);
        return (T)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void affine_warp_kernel(WarpArgs mat, int nb, const T* __restrict__ src, T* __restrict__ out,
                                                          long src_stride_s, long out_stride_s, int planes, int h, int w, long stride_p,
                                                          long stride_px, int tw_log2, T fill) {
#pragma clang fp contract(off)
    const int tw = 1 << tw_log2, th = 256 >> tw_log2;
    const int tiles_x = (w + tw - 1) >> tw_log2, tiles_y = (h + th - 1) / th;
    const long per = (long)tiles_x * tiles_y;               // tiles per sample
    const int lx = threadIdx.x & (tw - 1), ly = threadIdx.x >> tw_log2;
    const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
    for (long tile = blockIdx.x; tile < per * nb; tile += gridDim.x) {
        const int i = (int)(tile / per);                    // uniform across the workgroup: the matrix is read from scalar registers
        const long r = tile - i * per;
        const int ty = (int)(r / tiles_x), tx = (int)(r - (long)ty * tiles_x);
        const int x = (tx << tw_log2) + lx, y = ty * th + ly;
        if (x >= w || y >= h) continue;
        const float dx = (float)x - cx, dy = (float)y - cy;
        const float xs = (mat.m00[i] * dx + mat.m01[i] * dy) + cx;
        const float ys = (mat.m10[i] * dx + mat.m11[i] * dy) + cy;
        const T* a = src + i * src_stride_s;
        T* o = out + i * out_stride_s + ((long)y * w + x) * stride_px;
        if constexpr (MODE == WARP_NEAREST) {
            bool in = xs > -1.0f && xs < (float)w + 1.0f && ys > -1.0f && ys < (float)h + 1.0f;     // (false for a NaN: inf - inf)
            long at = 0;
            if (in) {
                const int xi = (int)rintf(xs), yi = (int)rintf(ys);
                in = xi >= 0 && xi < w && yi >= 0 && yi < h;
                at = ((long)yi * w + xi) * stride_px;
            }
            for (int p = 0; p < planes; ++p) o[p * stride_p] = in ? a[at + p * stride_p] : fill;
        } else {
            if (!(xs > -1.0f && xs < (float)w && ys > -1.0f && ys < (float)h)) {      // all four taps outside (or a NaN coordinate)
                for (int p = 0; p < planes; ++p) o[p * stride_p] = (T)0;
                continue;
            }
            const float xf = floorf(xs), yf = floorf(ys);
            const float fx = xs - xf, fy = ys - yf;
            const int x0 = (int)xf, y0 = (int)yf;           // in [-1, w - 1] x [-1, h - 1]
            const long at = ((long)y0 * w + x0) * stride_px;
            if (fx == 0.0f && fy == 0.0f) {                 // an integer source pixel (inside: xs > -1 and whole): by bits
                for (int p = 0; p < planes; ++p) o[p * stride_p] = a[at + p * stride_p];
                continue;
            }
            const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
            const float w00 = wy0 * wx0, w01 = wy0 * fx, w10 = fy * wx0, w11 = fy * fx;
            const bool r00 = w00 != 0.0f && x0 >= 0 && y0 >= 0, r01 = w01 != 0.0f && x0 + 1 < w && y0 >= 0;
            const bool r10 = w10 != 0.0f && x0 >= 0 && y0 + 1 < h, r11 = w11 != 0.0f && x0 + 1 < w && y0 + 1 < h;
            const long right = stride_px, down = (long)w * stride_px;
            for (int p = 0; p < planes; ++p) {
                const T* t = a + at + p * stride_p;
                const float v00 = r00 ? warp_value(t[0]) : 0.0f, v01 = r01 ? warp_value(t[right]) : 0.0f;
                const float v10 = r10 ? warp_value(t[down]) : 0.0f, v11 = r11 ? warp_value(t[down + right]) : 0.0f;
                float acc = r00 ? w00 * v00 : 0.0f;
                if (r01) acc += w01 * v01;
                if (r10) acc += w10 * v10;
                if (r11) acc += w11 * v11;
                o[p * stride_p] = warp_bits<T>(acc);
            }
        }
    }
}

template <typename T, int MODE>
static hipError_t launch_affine_warp(const WarpArgs& mat, int nb, const void* src, void* out, long src_stride_s, long out_stride_s, int planes,
                                     int h, int w, long stride_p, long stride_px, unsigned long long fill_bits, hipStream_t st) {
    const long pixel_bytes = (long)sizeof(T) * (stride_px > 1 ? planes : 1);
    const int tw_log2 = pixel_bytes <= 2 ? 6 : pixel_bytes <= 4 ? 5 : 4;
    const int tw = 1 << tw_log2, th = 256 >> tw_log2;
    long blocks = (long)((w + tw - 1) / tw) * ((h + th - 1) / th) * nb;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((affine_warp_kernel<T, MODE>), dim3((unsigned)blocks), dim3(256), 0, st, mat, nb, static_cast<const T*>(src),
                       static_cast<T*>(out), src_stride_s, out_stride_s, planes, h, w, stride_p, stride_px, tw_log2, (T)fill_bits);
    return hipGetLastError();
}

}  // namespace vqseg

extern "C" {

int vqseg_batch_u8_f(int n, const uint8_t* img_cache, const uint8_t* mask_cache, const int64_t* img_offsets_host,
                     const int64_t* mask_offsets_host, int h, int w, int mh, int mw, const float* f32_lut, const int64_t* label_lut,
                     float* img_out, uint8_t* target_out, int64_t* label_out, void* stream) {
    using namespace vqseg;
    if (n <= 0 || h <= 0 || w <= 0) return vqseg_set_error(VQSEG_EINVAL, "batch_u8: n, h and w must be positive");
    if (!img_cache || !img_offsets_host || !f32_lut || !img_out)
        return vqseg_set_error(VQSEG_EINVAL, "batch_u8: null img_cache, img_offsets_host, f32_lut or img_out");
    const bool masks = mask_cache != nullptr;
    if (masks && (!mask_offsets_host || !target_out || mh <= 0 || mw <= 0))
        return vqseg_set_error(VQSEG_EINVAL, "batch_u8: a mask cache needs mask_offsets_host, target_out and positive mh, mw");
    if (!masks && (target_out || label_lut || label_out))
        return vqseg_set_error(VQSEG_EINVAL, "batch_u8: target_out / label_lut / label_out without a mask cache");
    if (!label_lut != !label_out) return vqseg_set_error(VQSEG_EINVAL, "batch_u8: label_lut and label_out go together");
    if ((long)h * w > (1L << 28) || (masks && (long)mh * mw > (1L << 28)))
        return vqseg_set_error(VQSEG_EINVAL, "batch_u8: sample larger than 2^28 pixels");
    const long img_bytes = (long)h * w * 3, mask_bytes = masks ? (long)mh * mw : 0;
    // the vector body needs 4-byte aligned sources and 16-byte aligned outputs (per-sample output alignment: in the kernel)
    const uintptr_t ptrs = (uintptr_t)img_cache | (uintptr_t)mask_cache | (uintptr_t)img_out | (uintptr_t)target_out | (uintptr_t)label_out;
    bool vec = (ptrs & 15u) == 0;
    for (int i = 0; i < n; ++i) {
        if (img_offsets_host[i] < 0 || (masks && mask_offsets_host[i] < 0))
            return vqseg_set_error(VQSEG_EINVAL, "batch_u8: negative sample offset");
        vec = vec && (img_offsets_host[i] & 3) == 0 && (!masks || (mask_offsets_host[i] & 3) == 0);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long cap = nn_grid_cap();
    for (int s0 = 0; s0 < n; s0 += BATCH_ARG_SAMPLES) {
        const int nb = n - s0 < BATCH_ARG_SAMPLES ? n - s0 : BATCH_ARG_SAMPLES;
        BatchOffsets off = {};
        for (int i = 0; i < nb; ++i) {
            off.img[i] = img_offsets_host[s0 + i];
            off.mask[i] = masks ? mask_offsets_host[s0 + i] : 0;
        }
        const long tiles = ((img_bytes > mask_bytes ? img_bytes : mask_bytes) + 1023) / 1024;
        long blocks = (tiles * nb + 3) / 4;                 // 4 waves per workgroup, one 1 KiB tile per wave and iteration
        if (blocks > cap) blocks = cap;
        float* io = img_out + (long)s0 * img_bytes;
        uint8_t* to = masks ? target_out + (long)s0 * mask_bytes : nullptr;
        int64_t* lo = label_out ? label_out + (long)s0 * mask_bytes : nullptr;
        // a launch after the first starts at sample s0: its outputs' alignment is that of sample s0's position
        const int v = vec && ((long)s0 * img_bytes % 4 == 0) && ((long)s0 * mask_bytes % 4 == 0);
        hipLaunchKernelGGL(batch_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, off, nb, v, img_cache, mask_cache, img_bytes,
                           mask_bytes, f32_lut, label_lut, io, to, lo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_u8_kernel: %s", hipGetErrorString(e));
            return vqseg_set_error((int)e, buf);
        }
    }
    return 0;
}

int vqseg_box_mix_f(int mode, int elem_bytes, const void* src, void* out, int n, int planes, int h, int w, int64_t stride_s,
                    int64_t stride_p, int64_t stride_px, const int32_t* boxes_host, uint64_t fill_bits, void* stream) {
    using namespace vqseg;
    if (mode != BOX_MODE_MIX && mode != BOX_MODE_FILL) return vqseg_set_error(VQSEG_EINVAL, "box_mix: mode must be 0 (mix) or 1 (fill)");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return vqseg_set_error(VQSEG_EINVAL, "box_mix: element width must be 1, 2, 4 or 8 bytes");
    if (n <= 0 || planes <= 0 || h <= 0 || w <= 0) return vqseg_set_error(VQSEG_EINVAL, "box_mix: n, planes, h and w must be positive");
    if ((long)planes * h * w > (1L << 40)) return vqseg_set_error(VQSEG_EINVAL, "box_mix: sample larger than 2^40 elements");
    if (!src || !out || !boxes_host) return vqseg_set_error(VQSEG_EINVAL, "box_mix: null src, out or boxes_host");
    if (src == out) return vqseg_set_error(VQSEG_EINVAL, "box_mix: out of place only (a sample's partner is read after the sample is written)");
    const long elems = (long)planes * h * w;
    // rows dense, and the sample one dense run: planar (pixel stride 1, planes h * w apart) or interleaved (plane stride 1, pixels `planes` apart)
    const bool planar = stride_px == 1 && (planes == 1 || stride_p == (int64_t)h * w);
    const bool interleaved = planes > 1 && stride_p == 1 && stride_px == planes;
    if (!planar && !interleaved)
        return vqseg_set_error(VQSEG_EINVAL, "box_mix: layout must be planar (NCHW, 3-D labels) or interleaved (channels_last) with dense rows");
    if (n > 1 && stride_s < elems) return vqseg_set_error(VQSEG_EINVAL, "box_mix: sample stride smaller than a sample");
    for (int i = 0; i < n; ++i) {
        const int32_t* b = boxes_host + 4 * (long)i;
        if (b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] < 0 || (long)b[0] + b[2] > h || (long)b[1] + b[3] > w)
            return vqseg_set_error(VQSEG_EINVAL, "box_mix: a box (y1, x1, cut_h, cut_w) lies outside the image");
    }
    const long line = planar ? w : (long)w * planes;
    const int g = planar ? 1 : planes;
    const int vec = (((uintptr_t)src | (uintptr_t)out) & 15u) == 0;      // per-sample alignment (s * stride_s): in the kernel
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int s0 = 0; s0 < n; s0 += BATCH_ARG_SAMPLES) {
        const int nb = n - s0 < BATCH_ARG_SAMPLES ? n - s0 : BATCH_ARG_SAMPLES;
        BoxArgs box = {};
        for (int i = 0; i < nb; ++i) {
            const int32_t* b = boxes_host + 4 * (long)(s0 + i);
            box.y1[i] = b[0], box.x1[i] = b[1], box.ch[i] = b[2], box.cw[i] = b[3];
        }
        hipError_t e;
        switch (elem_bytes) {
            case 1: e = launch_box_mix<uint8_t>(box, s0, nb, n, mode, vec, src, out, stride_s, elems, line, h, g, fill_bits, st); break;
            case 2: e = launch_box_mix<uint16_t>(box, s0, nb, n, mode, vec, src, out, stride_s, elems, line, h, g, fill_bits, st); break;
            case 4: e = launch_box_mix<uint32_t>(box, s0, nb, n, mode, vec, src, out, stride_s, elems, line, h, g, fill_bits, st); break;
            default: e = launch_box_mix<uint64_t>(box, s0, nb, n, mode, vec, src, out, stride_s, elems, line, h, g, fill_bits, st); break;
        }
        if (e != hipSuccess) {
            char buf[160];
            snprintf(buf, sizeof(buf), "box_mix_kernel: %s", hipGetErrorString(e));
            return vqseg_set_error((int)e, buf);
        }
    }
    return 0;
}

int vqseg_affine_warp_f(int mode, int elem_bytes, const void* src, void* out, int n, int planes, int h, int w, int64_t src_stride_s,
                        int64_t out_stride_s, int64_t stride_p, int64_t stride_px, const float* matrices_host, uint64_t fill_bits,
                        void* stream) {
    using namespace vqseg;
    if (mode != WARP_BILINEAR && mode != WARP_NEAREST)
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: mode must be 0 (bilinear) or 1 (nearest)");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: element width must be 1, 2, 4 or 8 bytes");
    if (mode == WARP_BILINEAR && elem_bytes != 2 && elem_bytes != 4)
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: bilinear takes element width 4 (f32) or 2 (bf16) only; other widths are nearest");
    if (n <= 0 || planes <= 0 || h <= 0 || w <= 0) return vqseg_set_error(VQSEG_EINVAL, "affine_warp: n, planes, h and w must be positive");
    if (h > (1 << 24) || w > (1 << 24) || (long)planes * h * w > (1L << 40))
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: h or w above 2^24 (the image centre must be exact in f32) or sample larger than 2^40 elements");
    if (!src || !out || !matrices_host) return vqseg_set_error(VQSEG_EINVAL, "affine_warp: null src, out or matrices_host");
    if (src == out) return vqseg_set_error(VQSEG_EINVAL, "affine_warp: out of place only (a pixel's source is read after other pixels are written)");
    const long elems = (long)planes * h * w;
    const bool planar = stride_px == 1 && (planes == 1 || stride_p == (int64_t)h * w);
    const bool interleaved = planes > 1 && stride_p == 1 && stride_px == planes;
    if (!planar && !interleaved)
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: layout must be planar (NCHW, 3-D labels) or interleaved (channels_last) with dense rows");
    if (n > 1 && (src_stride_s < elems || out_stride_s < elems))
        return vqseg_set_error(VQSEG_EINVAL, "affine_warp: sample stride smaller than a sample");
    for (long i = 0; i < 6L * n; ++i)
        if (!(matrices_host[i] - matrices_host[i] == 0.0f))
            return vqseg_set_error(VQSEG_EINVAL, "affine_warp: a matrix entry is not finite");
    for (long i = 0; i < n; ++i)
        if (matrices_host[6 * i + 2] != 0.0f || matrices_host[6 * i + 5] != 0.0f)
            return vqseg_set_error(VQSEG_EINVAL, "affine_warp: the translation slots (entries 2 and 5 of a row) are reserved and must be 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int s0 = 0; s0 < n; s0 += BATCH_ARG_SAMPLES) {
        const int nb = n - s0 < BATCH_ARG_SAMPLES ? n - s0 : BATCH_ARG_SAMPLES;
        WarpArgs mat = {};
        for (int i = 0; i < nb; ++i) {
            const float* m = matrices_host + 6 * (long)(s0 + i);
            mat.m00[i] = m[0], mat.m01[i] = m[1], mat.m10[i] = m[3], mat.m11[i] = m[4];
        }
        const char* a = static_cast<const char*>(src) + (long)s0 * src_stride_s * elem_bytes;
        char* o = static_cast<char*>(out) + (long)s0 * out_stride_s * elem_bytes;
        hipError_t e;
#define VQSEG_WARP(T, MODE) launch_affine_warp<T, MODE>(mat, nb, a, o, src_stride_s, out_stride_s, planes, h, w, stride_p, stride_px, fill_bits, st)
        if (mode == WARP_BILINEAR) {
            e = elem_bytes == 4 ? VQSEG_WARP(uint32_t, WARP_BILINEAR) : VQSEG_WARP(uint16_t, WARP_BILINEAR);
        } else {
            switch (elem_bytes) {
                case 1: e = VQSEG_WARP(uint8_t, WARP_NEAREST); break;
                case 2: e = VQSEG_WARP(uint16_t, WARP_NEAREST); break;
                case 4: e = VQSEG_WARP(uint32_t, WARP_NEAREST); break;
                default: e = VQSEG_WARP(uint64_t, WARP_NEAREST); break;
            }
        }
#undef VQSEG_WARP
        if (e != hipSuccess) {
            char buf[160];
            snprintf(buf, sizeof(buf), "affine_warp_kernel: %s", hipGetErrorString(e));
            return vqseg_set_error((int)e, buf);
        }
    }
    return 0;
}

}  // extern "C"
