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

}  // extern "C"
