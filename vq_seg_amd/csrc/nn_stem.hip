// nn_stem.hip -- what feeds the network's first layer (gfx950), HBM-bound: the stem's im2col patch rows (fp32, bf16 or split-3),
// the split-3 split / merge of an fp32 tensor (format: nn_device.h), and the fp32 <-> bf16 casts.
//
// Reference op: the 7x7 stride-2 stem convolution of the ResNet encoder (models/encoders/resnet.py), run here as a 1x1
// convolution over the patch rows.  Rows are NHWC pixels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nn_device.h"
#include "nn_internal.h"

namespace vqseg {

// ---------------------------------------------------------------------------------------------
// stem im2col: x [N,H,W,3] -> rows [N*Ho*Wo][Kp] with the 7x7x3 patch (kh, kw, ci order), stride 2, pad 3
// (zero or reflect), columns >= 147 zero.  The stem then runs as a 1x1 convolution with Cin = Kp.
// ---------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void im2col_stem_kernel(const TI* __restrict__ x, int N, int H, int W, int Cin, int KH, int KW,
                                                          int stride, int pad, int reflect, int Ho, int Wo, int Kp,
                                                          TO* __restrict__ out) {
    const long total = (long)N * Ho * Wo * Kp;
    const int K = KH * KW * Cin;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k = (int)(i % Kp);
        long t = i / Kp;
        const int ow = (int)(t % Wo);
        t /= Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        float v = 0.0f;
        if (k < K) {
            const int ci = k % Cin, kw = (k / Cin) % KW, kh = k / (Cin * KW);
            int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
            if (reflect) {
                if (ih < 0) ih = -ih;
                if (ih >= H) ih = 2 * H - 2 - ih;
                if (iw < 0) iw = -iw;
                if (iw >= W) iw = 2 * W - 2 - iw;
            }
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = (float)x[(((long)n * H + ih) * W + iw) * Cin + ci];
        }
        out[i] = (TO)v;
    }
}

// the stem's own shape (7x7x3, compile-time divisors), 8 columns = one 16-byte (bf16) / two 16-byte (f32) stores per thread;
// TO = S3Row: split-3 patch rows
template <typename TO>
__global__ __launch_bounds__(256) void im2col_stem7_kernel(const float* __restrict__ x, int N, int H, int W, int stride, int pad,
                                                           int reflect, int Ho, int Wo, int Kp, TO* __restrict__ out) {
    constexpr int KW = 7, CIN = 3, K = 147;
    const unsigned cpr = Kp / 8;                            // 8-column chunks per row
    const unsigned total = (unsigned)N * Ho * Wo * cpr;     // < 2^32 (checked by the launcher): 32-bit index arithmetic --
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {   // 64-bit divisions cost more than the copy
        const int ch = (int)(i % cpr);
        unsigned t = i / cpr;
        const int ow = (int)(t % (unsigned)Wo);
        t /= (unsigned)Wo;
        const int oh = (int)(t % (unsigned)Ho);
        const int n = (int)(t / (unsigned)Ho);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = ch * 8 + e;
            v[e] = 0.0f;
            if (k < K) {
                const int ci = k % CIN, kw = (k / CIN) % KW, kh = k / (CIN * KW);
                int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
                if (reflect) {
                    if (ih < 0) ih = -ih;
                    if (ih >= H) ih = 2 * H - 2 - ih;
                    if (iw < 0) iw = -iw;
                    if (iw >= W) iw = 2 * W - 2 - iw;
                }
                if (ih >= 0 && ih < H && iw >= 0 && iw < W) v[e] = x[(((long)n * H + ih) * W + iw) * CIN + ci];
            }
        }
        if constexpr (__is_same(TO, S3Row)) {              // split-3 rows [2 * Kp]: chunk ch of hi | lo
            const size_t row = (size_t)(i / cpr);
            s3_store8(reinterpret_cast<unsigned short*>(out) + row * 2 * Kp, Kp, ch * 8, v);
        } else {
        TO* dst = out + (size_t)i * 8;
        if constexpr (sizeof(TO) == 2) {
            u32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 lo = (__bf16)v[2 * e], hi = (__bf16)v[2 * e + 1];
                r[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
            }
            *reinterpret_cast<u32x4*>(dst) = r;
        } else {
            *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
        }
    }
}

// r4: the same patch rows from an LDS-staged strip.  The gather kernel above spends its time on address arithmetic and 8 scattered
// 4-byte loads per 16-byte store (464 us for the bench's 671 MB bf16 patch matrix = 1.7 TB/s, and both networks of a CPS pair wait for
// it).  Here a workgroup owns 64 consecutive output pixels of one output row: the 7 input rows x (2 * 63 + 7 = 133) input pixels x 3
// channels they read (padding applied while staging: reflect or zero) go to LDS with coalesced loads -- 3.4 x fewer global loads --
// and a patch column k = (kh, kw, ci) of pixel p is LDS word kh * ROW + 6 p + (k - 21 kh): for a fixed kh the 21 columns are
// CONSECUTIVE input floats.  320 threads = 16 pixels x 20 column chunks: a thread keeps its chunk (its eight LDS offsets are computed
// once) and walks TP / 16 pixels; ROW = 22 mod 32 puts the 20 chunks of a pixel in different banks.  Stride 2 / pad 3 / 160 columns
// (the stem).  Values identical to the gather kernel's.  Measured at the bench's shape (tools/bench_im2col.py; gather kernel -> strips
// of 64 -> of 128 pixels): bf16 rows 475 -> 236 -> 194 us (4.0 TB/s), split-3 rows 604 -> 311 -> 319, fp32 rows 583 -> 359 -> 381:
// bf16 takes 128-pixel strips (one load round trip per 8 KB stored instead of per 4 KB), the 32-byte-per-element forms 64.
#ifndef IM2COL_ABL
#define IM2COL_ABL 0              // debug builds only (results wrong): 1 no global stores, 2 no global loads
#endif
template <typename TO, int TP, int KP>
__global__ __launch_bounds__(2 * KP) void im2col_stem7_strip_kernel(const float* __restrict__ x, int N, int H, int W, int reflect, int Ho, int Wo,
                                                                 TO* __restrict__ out) {
    constexpr int NCOL = (2 * (TP - 1) + 7) * 3, CPR = KP / 8, NT = 16 * CPR;   // threads: 16 pixels x CPR column chunks (KP = 160: 320, 192: 384)   // NCOL floats of an input row feed the strip
    constexpr int ROW = (NCOL + 31 - 22) / 32 * 32 + 22;    // >= NCOL, = 22 mod 32 (406 for 64-pixel strips)
    constexpr int NH = (NCOL + NT - 1) / NT;
    __shared__ float strip[7 * ROW];
    const int strips = (Wo + TP - 1) / TP;
    const int sx = blockIdx.x % strips;
    const int oh = (blockIdx.x / strips) % Ho, n = blockIdx.x / (strips * Ho);
    const int ow0 = sx * TP, iw0 = 2 * ow0 - 3;
    const int t = threadIdx.x;
    // staging: a thread owns NH columns of the strip in all seven rows.  The loads are UNCONDITIONAL (clamped address, value selected
    // afterwards) and all issued before the first LDS write: a load under a divergent branch is waited for right there -- fourteen
    // serialised round trips per workgroup (measured: 190 us of a 300 us launch).  One strip per workgroup: a loop over strips with
    // the next strip's loads in flight was SLOWER (285 vs 234 us) -- gfx950 counts loads and stores on one in-order counter, so waiting
    // for the prefetch drains the stores issued after it.
    const float* xn = x + (size_t)n * H * W * 3;
    float r[NH][7];
#pragma unroll
    for (int half = 0; half < NH; ++half) {
        const int c = t + NT * half;
        const int px = c / 3, ci = c - 3 * px;
        int iw = iw0 + px;
        if (reflect) {
            if (iw < 0) iw = -iw;
            if (iw >= W) iw = 2 * W - 2 - iw;
        }
        const bool cok = c < NCOL && iw >= 0 && iw < W;     // (beyond a ragged last strip: unused)
        const int coff = cok ? iw * 3 + ci : 0;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            int ih = 2 * oh - 3 + kh;                       // workgroup-uniform
            if (reflect) {
                if (ih < 0) ih = -ih;
                if (ih >= H) ih = 2 * H - 2 - ih;
            }
            const bool ok = cok && ih >= 0 && ih < H;
#if IM2COL_ABL == 2
            const float v = (float)coff;
#else
            const float v = xn[(ok ? ih : 0) * W * 3 + coff];
#endif
            r[half][kh] = ok ? v : 0.0f;
        }
    }
#pragma unroll
    for (int half = 0; half < NH; ++half)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh)
            if (t + NT * half < NCOL) strip[kh * ROW + t + NT * half] = r[half][kh];
    __syncthreads();
    const int ch = t % CPR, p0 = t / CPR;                   // this thread's column chunk; pixels p0, p0 + 16, ...
    int off[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = ch * 8 + e;
        const int kh = k / 21;
        off[e] = k < 147 ? kh * ROW + (k - 21 * kh) : -1;
    }
    const int npx = Wo - ow0 < TP ? Wo - ow0 : TP;
    const size_t row0 = ((size_t)n * Ho + oh) * Wo + ow0;
#pragma unroll
    for (int it = 0; it < TP / 16; ++it) {
        const int p = p0 + 16 * it;
        if (p < npx) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = off[e] >= 0 ? strip[off[e] + 6 * p] : 0.0f;
#if IM2COL_ABL == 1
            if (v[0] != 12345.678f) continue;
#endif
            if constexpr (__is_same(TO, S3Row)) {          // split-3 rows [2 * KP]: chunk ch of hi | lo
                s3_store8(reinterpret_cast<unsigned short*>(out) + (row0 + p) * 2 * KP, KP, ch * 8, v);
            } else {
                TO* dst = out + (row0 + p) * KP + ch * 8;
                if constexpr (sizeof(TO) == 2) {
                    u32x4 q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const __bf16 lo = (__bf16)v[2 * e], hi = (__bf16)v[2 * e + 1];
                        q[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
                    }
                    *reinterpret_cast<u32x4*>(dst) = q;
                } else {
                    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void s3_split_kernel(const float* __restrict__ x, long rows, int C, unsigned short* __restrict__ y) {
    const int cv = C / 8;
    const long total = rows * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / cv;
        const int c = (int)(i - r * cv) * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * C + c), b = *reinterpret_cast<const f32x4*>(x + r * C + c + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        s3_store8(y + r * 2 * C, C, c, v);
    }
}

__global__ __launch_bounds__(256) void s3_merge_kernel(const unsigned short* __restrict__ x, long rows, int C, float* __restrict__ y) {
    const int cv = C / 8;
    const long total = rows * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / cv;
        const int c = (int)(i - r * cv) * 8;
        float v[8];
        s3_load8(x + r * 2 * C, C, c, v);
        *reinterpret_cast<f32x4*>(y + r * C + c) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(y + r * C + c + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ x, long n, TO* __restrict__ y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = (TO)(float)x[i];
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_im2col_stem(int out_bf16, const float* x, int N, int H, int W, int Cin, int KH, int KW, int stride, int pad,
                              int reflect, int Ho, int Wo, int Kp, void* out, hipStream_t st_) {
    if (g_nn_opt.im2col_strip && KH == 7 && KW == 7 && Cin == 3 && stride == 2 && pad == 3 && (Kp == 160 || (Kp == 192 && out_bf16 == 2)) &&
        (long)H * W * 3 < (1L << 31) && (long)N * Ho * ((Wo + 63) / 64) < (1L << 31)) {
        const unsigned g64 = (unsigned)((long)N * Ho * ((Wo + 63) / 64)), g128 = (unsigned)((long)N * Ho * ((Wo + 127) / 128));
        if (out_bf16 == 2 && Kp == 192)                     // (the split-3 forward pads its patch rows to 64 columns)
            hipLaunchKernelGGL((im2col_stem7_strip_kernel<S3Row, 64, 192>), dim3(g64), dim3(384), 0, st_, x, N, H, W, reflect, Ho, Wo, (S3Row*)out);
        else if (out_bf16 == 2)
            hipLaunchKernelGGL((im2col_stem7_strip_kernel<S3Row, 64, 160>), dim3(g64), dim3(320), 0, st_, x, N, H, W, reflect, Ho, Wo, (S3Row*)out);
        else if (out_bf16)
            hipLaunchKernelGGL((im2col_stem7_strip_kernel<__bf16, 128, 160>), dim3(g128), dim3(320), 0, st_, x, N, H, W, reflect, Ho, Wo, (__bf16*)out);
        else
            hipLaunchKernelGGL((im2col_stem7_strip_kernel<float, 64, 160>), dim3(g64), dim3(320), 0, st_, x, N, H, W, reflect, Ho, Wo, (float*)out);
        return hipGetLastError();
    }
    if (KH == 7 && KW == 7 && Cin == 3 && Kp % 8 == 0 && (long)N * Ho * Wo * (Kp / 8) < (1L << 31)) {
        const unsigned g8 = grid_for((long)N * Ho * Wo * (Kp / 8));
        if (out_bf16 == 2)
            hipLaunchKernelGGL((im2col_stem7_kernel<S3Row>), dim3(g8), dim3(256), 0, st_, x, N, H, W, stride, pad, reflect, Ho, Wo, Kp,
                               (S3Row*)out);
        else if (out_bf16)
            hipLaunchKernelGGL((im2col_stem7_kernel<__bf16>), dim3(g8), dim3(256), 0, st_, x, N, H, W, stride, pad, reflect, Ho, Wo, Kp,
                               (__bf16*)out);
        else
            hipLaunchKernelGGL((im2col_stem7_kernel<float>), dim3(g8), dim3(256), 0, st_, x, N, H, W, stride, pad, reflect, Ho, Wo, Kp,
                               (float*)out);
        return hipGetLastError();
    }
    if (out_bf16 == 2) return hipErrorInvalidValue;          // split-3 patches: the 7x7x3 stem shape only
    const unsigned gr = grid_for((long)N * Ho * Wo * Kp);
    if (out_bf16)
        hipLaunchKernelGGL((im2col_stem_kernel<float, __bf16>), dim3(gr), dim3(256), 0, st_, x, N, H, W, Cin, KH, KW, stride, pad,
                           reflect, Ho, Wo, Kp, (__bf16*)out);
    else
        hipLaunchKernelGGL((im2col_stem_kernel<float, float>), dim3(gr), dim3(256), 0, st_, x, N, H, W, Cin, KH, KW, stride, pad,
                           reflect, Ho, Wo, Kp, (float*)out);
    return hipGetLastError();
}

hipError_t launch_s3_split(const float* x, long rows, int C, void* y, hipStream_t st_) {
    hipLaunchKernelGGL(s3_split_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, st_, x, rows, C, (unsigned short*)y);
    return hipGetLastError();
}
hipError_t launch_s3_merge(const void* x, long rows, int C, float* y, hipStream_t st_) {
    hipLaunchKernelGGL(s3_merge_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, st_, (const unsigned short*)x, rows, C, y);
    return hipGetLastError();
}

hipError_t launch_cast(int to_bf16, const void* x, long n, void* y, hipStream_t st_) {
    const unsigned gr = grid_for(n);
    if (to_bf16) hipLaunchKernelGGL((cast_kernel<float, __bf16>), dim3(gr), dim3(256), 0, st_, (const float*)x, n, (__bf16*)y);
    else hipLaunchKernelGGL((cast_kernel<__bf16, float>), dim3(gr), dim3(256), 0, st_, (const __bf16*)x, n, (float*)y);
    return hipGetLastError();
}

}  // namespace vqseg
