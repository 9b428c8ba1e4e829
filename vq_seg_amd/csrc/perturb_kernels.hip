// perturb_kernels.hip -- the feature-perturbation stream of the CPS step (vq_seg_amd.nnf.channel_keep / channel_dropout_cat;
// models/networks/modified_vqunet/net.py: decode with a perturbation spec; CPSConfig.feature_perturb).
//
// Reference: UniMatch's second stream (deprecated/train_UNIMatch.py:172,183-185; models/networks/deeplabv3/net.py:109-116) runs
// decoder(torch.cat((f, nn.Dropout2d(0.5)(f)))) on the weak view's encoder features: per (sample, channel) a Bernoulli keep, the kept
// channels scaled by 1 / (1 - p).  Here the keep table is a counter-based draw (Philox4x32-10: a pure function of seed, stream id,
// step and element index -- no generator state, no host-to-device copy), and the concatenation and the dropout are ONE pass:
//     out[i]     = x[i]                                                              by bits
//     out[n + i] = scale[i, c] == 0 ? +0.0 : round(float(x[i, c, ..]) * scale[i, c])   a SELECTION where the channel is dropped
// with the backward pass folding the two halves of the gradient in one pass as well:
//     gx[i] = scale[i, c] == 0 ? g[i] : round(float(g[i]) + round_f32(float(g[n + i]) * scale[i, c]))
// HBM-bound: forward 1 read + 2 writes per element, backward 2 reads + 1 write; the scale row of a sample (C floats) is re-read from L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "nn_kernels.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

// The backward pass promises the product rounded to f32 BEFORE the add.  Under the default -ffp-contract=fast the compiler contracts
// a * b + c into one FMA -- and __fmul_rn / __fadd_rn do not stop it: the headers define them as plain * and + in inline functions of
// their own, which carry the contraction flag with them.  So the arithmetic below is written with plain operators under this pragma,
// which is lexically scoped and therefore stands at file scope, in front of the inline helpers (tests pin the bits).
#pragma clang fp contract(off)

// ---- the keep / scale table ----------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32 x 32 -> 64-bit products, the key bumped by the Weyl constants between
// rounds.  Plain integer arithmetic; word 0 of the block of counter (e, stream, step_lo, step_hi) under key (seed_lo, seed_hi) decides
// element e.  Known answers: tests/test_feature_perturb_cpu.py.
__device__ inline uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return c0;
}

__global__ __launch_bounds__(256) void channel_keep_kernel(float* __restrict__ scale, long total, uint32_t seed_lo, uint32_t seed_hi,
                                                           uint32_t stream_id, uint32_t step_lo, uint32_t step_hi, uint32_t threshold,
                                                           float inv_keep) {
    const long stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride)
        scale[e] = philox_word0((uint32_t)e, stream_id, step_lo, step_hi, seed_lo, seed_hi) >= threshold ? inv_keep : 0.0f;
}

// ---- forward: copy + perturbed copy ----------------------------------------------------------------------------------------------------
// Work decomposition of box_mix_kernel (data_kernels.hip): a 1 KiB tile of one sample per wave and iteration.  A whole tile whose three
// addresses (the sample in x, in the clean half and in the perturbed half of out) are 16-byte aligned takes one 16-byte load and two
// 16-byte stores per lane, contiguous across the wave; a sample's partial last tile, and every tile of a sample one of whose bases is not
// aligned, goes element by element, lane l taking elements l, l + 64, ... of the tile.  The scale is picked per ELEMENT: in channels_last
// a 16-byte unit spans channels (and pixels, when C is below the unit), in NCHW a unit may cross a plane boundary.
__device__ inline uint32_t perturb_bits(uint32_t v, float s) {
    return s == 0.0f ? 0u : __float_as_uint(__uint_as_float(v) * s);
}

__device__ inline uint16_t bf16_bits(float r) {              // round to nearest even; a NaN becomes the canonical quiet NaN, as torch's cast
    const uint32_t u = __float_as_uint(r);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ inline uint16_t perturb_bits(uint16_t v, float s) {
    return s == 0.0f ? (uint16_t)0 : bf16_bits(__uint_as_float((uint32_t)v << 16) * s);
}

__device__ inline uint32_t fold_bits(uint32_t a, uint32_t b, float s) {
    return s == 0.0f ? a : __float_as_uint(__uint_as_float(a) + __uint_as_float(b) * s);
}

__device__ inline uint16_t fold_bits(uint16_t a, uint16_t b, float s) {
    return s == 0.0f ? a : bf16_bits(__uint_as_float((uint32_t)a << 16) + __uint_as_float((uint32_t)b << 16) * s);
}

// FOLD == 0: a = x, o = out (clean half), p = out + n * elems (perturbed half, written)
// FOLD == 1: a = g (first half), p = g + n * elems (second half, read), o = gx
template <typename T, int FOLD>
__global__ __launch_bounds__(256) void channel_dropout_kernel(const T* __restrict__ a_all, T* __restrict__ o_all, T* p_all,
                                                              const float* __restrict__ scale, int n, int c, long elems, long hw, int cl,
                                                              int vec) {
    constexpr int K = 16 / (int)sizeof(T);                  // elements per 16-byte unit
    constexpr long TILE = 64L * K;                          // elements per 1 KiB tile
    union Unit {
        uint4 v;
        T e[K];
    };
    const long stride = (long)gridDim.x * 256;
    const long per = (elems + TILE - 1) / TILE * 64;        // units per sample, whole tiles
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < per * n; q += stride) {
        const long i = q / per;
        const long u = q - i * per;
        const long t = (u >> 6) * TILE;
        const int l = (int)(u & 63);
        const T* a = a_all + i * elems;
        T* o = o_all + i * elems;
        T* p = p_all + i * elems;
        const float* sc = scale + i * c;
        if (vec && ((i * elems * (long)sizeof(T)) & 15) == 0 && t + TILE <= elems) {
            const long f = t + (long)l * K;
            Unit ua, ub;
            ua.v = *reinterpret_cast<const uint4*>(a + f);
            if (FOLD) ub.v = *reinterpret_cast<const uint4*>(p + f);
            long ch = cl ? f % c : f / hw;
            long pos = cl ? 0 : f - ch * hw;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float s = sc[ch];
                if (FOLD)
                    ua.e[k] = fold_bits(ua.e[k], ub.e[k], s);
                else
                    ub.e[k] = perturb_bits(ua.e[k], s);
                if (cl) {
                    if (++ch == c) ch = 0;
                } else if (++pos == hw) {
                    pos = 0;
                    if (++ch == c) ch = 0;                  // (only behind the unit's last element: t + TILE <= elems)
                }
            }
            *reinterpret_cast<uint4*>(o + f) = ua.v;
            if (!FOLD) *reinterpret_cast<uint4*>(p + f) = ub.v;
        } else {
            for (int j = 0; j < K; ++j) {
                const long f = t + l + 64L * j;
                if (f >= elems) break;
                const float s = sc[cl ? f % c : f / hw];
                const T v = a[f];
                if (FOLD) {
                    o[f] = fold_bits(v, p[f], s);
                } else {
                    o[f] = v;
                    p[f] = perturb_bits(v, s);
                }
            }
        }
    }
}

template <typename T, int FOLD>
static hipError_t launch_channel_dropout(const void* a, void* o, void* p, const float* scale, int n, int c, long elems, long hw, int cl,
                                         hipStream_t st) {
    constexpr long TILE = 64L * (16 / (long)sizeof(T));
    long blocks = ((elems + TILE - 1) / TILE * n + 3) / 4;  // 4 waves per workgroup, one tile per wave and iteration
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    // every pointer 16-byte aligned, and the second half n * elems elements further on as well (per-sample alignment: in the kernel)
    const int vec = ((((uintptr_t)a | (uintptr_t)o | (uintptr_t)p) & 15u) == 0);
    hipLaunchKernelGGL((channel_dropout_kernel<T, FOLD>), dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const T*>(a),
                       static_cast<T*>(o), static_cast<T*>(p), scale, n, c, elems, hw, cl, vec);
    return hipGetLastError();
}

static int channel_dropout_check(const char* who, int bf16, const void* a, const float* scale, const void* o, int n, int c, int h, int w,
                                 int channels_last) {
    char buf[160];
    const char* msg = nullptr;
    if (bf16 != 0 && bf16 != 1) msg = "bf16 must be 0 (f32) or 1 (bf16)";
    else if (channels_last != 0 && channels_last != 1) msg = "channels_last must be 0 (NCHW) or 1";
    else if (n <= 0 || c <= 0 || h <= 0 || w <= 0) msg = "n, c, h and w must be positive";
    else if ((long)c * h * w > (1L << 40) || (long)n * c > (1L << 31)) msg = "sample larger than 2^40 elements or table larger than 2^31";
    else if (!a || !scale || !o) msg = "null tensor";
    else if (a == o) msg = "out of place only";
    if (!msg) return 0;
    snprintf(buf, sizeof(buf), "%s: %s", who, msg);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

static int channel_dropout_done(const char* who, hipError_t e) {
    if (e == hipSuccess) return 0;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %s", who, hipGetErrorString(e));
    return vqseg_set_error((int)e, buf);
}

}  // namespace vqseg

extern "C" {

int vqseg_channel_keep_f(float* scale, int64_t total, uint64_t seed, int64_t stream_id, uint64_t step, int64_t threshold, float inv_keep,
                         void* stream) {
    using namespace vqseg;
    if (!scale) return vqseg_set_error(VQSEG_EINVAL, "channel_keep: null scale");
    if (total <= 0 || total > 0xffffffffLL) return vqseg_set_error(VQSEG_EINVAL, "channel_keep: total must lie in 1 .. 2^32 - 1");
    if (stream_id < 0 || stream_id > 0xffffffffLL) return vqseg_set_error(VQSEG_EINVAL, "channel_keep: stream_id must lie in 0 .. 2^32 - 1");
    if (threshold < 0 || threshold > 0xffffffffLL) return vqseg_set_error(VQSEG_EINVAL, "channel_keep: threshold must lie in 0 .. 2^32 - 1");
    if (!(inv_keep >= 1.0f) || inv_keep - inv_keep != 0.0f) return vqseg_set_error(VQSEG_EINVAL, "channel_keep: inv_keep must be finite and >= 1");
    long blocks = (total + 255) / 256;
    const long cap = nn_grid_cap();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(channel_keep_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), scale, (long)total,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)step, (uint32_t)(step >> 32),
                       (uint32_t)threshold, inv_keep);
    return channel_dropout_done("channel_keep_kernel", hipGetLastError());
}

int vqseg_channel_dropout_cat_f(int bf16, const void* x, const float* scale, void* out, int n, int c, int h, int w, int channels_last,
                                void* stream) {
    using namespace vqseg;
    if (const int rc = channel_dropout_check("channel_dropout_cat", bf16, x, scale, out, n, c, h, w, channels_last)) return rc;
    const long hw = (long)h * w, elems = hw * c;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e =
        bf16 ? launch_channel_dropout<uint16_t, 0>(x, out, static_cast<uint16_t*>(out) + (long)n * elems, scale, n, c, elems, hw, channels_last, st)
             : launch_channel_dropout<uint32_t, 0>(x, out, static_cast<uint32_t*>(out) + (long)n * elems, scale, n, c, elems, hw, channels_last, st);
    return channel_dropout_done("channel_dropout_cat_kernel", e);
}

int vqseg_channel_dropout_fold_f(int bf16, const void* g, const float* scale, void* gx, int n, int c, int h, int w, int channels_last,
                                 void* stream) {
    using namespace vqseg;
    if (const int rc = channel_dropout_check("channel_dropout_fold", bf16, g, scale, gx, n, c, h, w, channels_last)) return rc;
    const long hw = (long)h * w, elems = hw * c;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the second half of g is only read: the kernel's shared signature takes it as a plain pointer
    const hipError_t e =
        bf16 ? launch_channel_dropout<uint16_t, 1>(g, gx, const_cast<uint16_t*>(static_cast<const uint16_t*>(g)) + (long)n * elems, scale, n, c,
                                                   elems, hw, channels_last, st)
             : launch_channel_dropout<uint32_t, 1>(g, gx, const_cast<uint32_t*>(static_cast<const uint32_t*>(g)) + (long)n * elems, scale, n, c,
                                                   elems, hw, channels_last, st);
    return channel_dropout_done("channel_dropout_fold_kernel", e);
}

}  // extern "C"
