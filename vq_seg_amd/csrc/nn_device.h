// Device-only helpers shared by the NN kernel units (nn_bn / nn_spatial / nn_head / nn_stem) and, for the split-3 row format, by the
// vector quantiser (vq_internal.h); no other file includes this: element
// and 16-byte vector access to NHWC "rows" (pixel-major, channels contiguous; T = float in precise mode, or __bf16), the flat-index
// split, and the split-3 row format with its one pair of accessors.  Every function here is __device__ __forceinline__.
#pragma once
#include <hip/hip_runtime.h>

namespace vqseg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float ld(const T* p, long i) { return (float)p[i]; }
template <typename T>
__device__ __forceinline__ void st(T* p, long i, float v) { p[i] = (T)v; }

// 16-byte vector access: 4 floats or 8 bf16 per thread (index i = first element, 16-byte aligned)
template <typename T>
struct VecN { static constexpr int N = 16 / sizeof(T); };
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void ldv(const T* p, long i, float (&v)[VecN<T>::N]) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(p + i);
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(raw[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = __uint_as_float(raw[e] << 16);
            v[2 * e + 1] = __uint_as_float(raw[e] & 0xffff0000u);
        }
    }
}
template <typename T>
__device__ __forceinline__ void stv(T* p, long i, const float (&v)[VecN<T>::N]) {
    u32x4 raw;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) raw[e] = __float_as_uint(v[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const __bf16 a = (__bf16)v[2 * e], b = (__bf16)v[2 * e + 1];
            raw[e] = (unsigned int)__builtin_bit_cast(unsigned short, a) | ((unsigned int)__builtin_bit_cast(unsigned short, b) << 16);
        }
    }
    *reinterpret_cast<u32x4*>(p + i) = raw;
}

// Each thread handles VC consecutive channels of one pixel (VC = 16-byte vector when C allows, else 1).
template <typename T, int VC>
__device__ __forceinline__ void ldc(const T* p, long i, float (&v)[VecN<T>::N]) {
    if constexpr (VC == 1) v[0] = ld(p, i);
    else if constexpr (VC == 3) {                          // the 3-class logits: one pixel per thread, three scalar accesses
#pragma unroll
        for (int e = 0; e < 3; ++e) v[e] = ld(p, i + e);
    } else ldv(p, i, v);
}
template <typename T, int VC>
__device__ __forceinline__ void stc(T* p, long i, const float (&v)[VecN<T>::N]) {
    if constexpr (VC == 1) st(p, i, v[0]);
    else if constexpr (VC == 3) {
#pragma unroll
        for (int e = 0; e < 3; ++e) st(p, i + e, v[e]);
    } else stv(p, i, v);
}

// flat index -> (channel group, x, y, image): 32-bit divisions whenever the index fits (it does for every tensor of the
// model: 64-bit integer division costs more ALU time than these copy-like kernels spend on memory)
__device__ __forceinline__ void split_nhwc(long i, int cv, int W, int H, int& c, int& w, int& h, int& n) {
    if (i < (1L << 31)) {
        unsigned u = (unsigned)i;
        c = (int)(u % (unsigned)cv);
        u /= (unsigned)cv;
        w = (int)(u % (unsigned)W);
        u /= (unsigned)W;
        h = (int)(u % (unsigned)H);
        n = (int)(u / (unsigned)H);
    } else {
        c = (int)(i % cv);
        long t = i / cv;
        w = (int)(t % W);
        t /= W;
        h = (int)(t % H);
        n = (int)(t / H);
    }
}

// ---------------------------------------------------------------------------------------------
// "split-3" activations (the fp32-precision eval forward on the bf16 kernels): a logical fp32 tensor [rows][C] is stored as
// [rows][2C] bf16 = [hi | lo], hi = bf16(v), lo = bf16(v - hi).  A bf16 convolution over the logical channels [hi | lo | hi]
// (the K loop reads hi twice) with weights [w_hi | w_hi | w_lo] computes x_hi w_hi + x_lo w_hi + x_hi w_lo -- the three
// products of the precise mode.
// Elementwise ops on such tensors work on v = hi + lo (exact in fp32) and re-split.  8 logical channels per thread.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void s3_load8(const unsigned short* row, int C, int c, float (&v)[8]) {
    const u32x4 h = *reinterpret_cast<const u32x4*>(row + c), l = *reinterpret_cast<const u32x4*>(row + C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = __builtin_bit_cast(float, h[e] << 16) + __builtin_bit_cast(float, l[e] << 16);
        v[2 * e + 1] = __builtin_bit_cast(float, h[e] & 0xFFFF0000u) + __builtin_bit_cast(float, l[e] & 0xFFFF0000u);
    }
}
__device__ __forceinline__ unsigned s3_pack2(float a, float b) {
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ void s3_store8(unsigned short* row, int C, int c, const float (&v)[8]) {
    u32x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = s3_pack2(v[2 * e], v[2 * e + 1]);
        const float h0 = __builtin_bit_cast(float, h[e] << 16), h1 = __builtin_bit_cast(float, h[e] & 0xFFFF0000u);
        l[e] = s3_pack2(v[2 * e] - h0, v[2 * e + 1] - h1);
    }
    *reinterpret_cast<u32x4*>(row + c) = h;
    *reinterpret_cast<u32x4*>(row + C + c) = l;
}

// Element-type tag of split-3 rows (head_fwd_kernel, the stem's patch kernels, the pooling / resize forward kernels): a kernel
// instantiated on it goes through s3_load8 / s3_store8; VecN<S3Row>::N = 8 logical channels per thread
struct S3Row { unsigned short raw; };

// VC channels from channel c of pixel `pix` of an NHWC tensor of C logical channels: a plain row holds C elements (the address is
// p + pix * C + c, as the callers of ldc spell it), a split-3 row 2C (and the accessor needs C to find lo)
template <typename T, int VC>
__device__ __forceinline__ void ldpx(const T* p, long pix, int C, int c, float (&v)[VecN<T>::N]) {
    if constexpr (__is_same(T, S3Row)) s3_load8(reinterpret_cast<const unsigned short*>(p) + pix * 2 * C, C, c, v);
    else ldc<T, VC>(p, pix * C + c, v);
}
template <typename T, int VC>
__device__ __forceinline__ void stpx(T* p, long pix, int C, int c, const float (&v)[VecN<T>::N]) {
    if constexpr (__is_same(T, S3Row)) s3_store8(reinterpret_cast<unsigned short*>(p) + pix * 2 * C, C, c, v);
    else stc<T, VC>(p, pix * C + c, v);
}

}  // namespace vqseg
