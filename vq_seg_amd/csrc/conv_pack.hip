// conv_pack.hip -- the kernel-side images of a convolution weight (bf16 hi / lo, transposed + tap-flipped, split-3, stride-2 classes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_device.h"

namespace vqseg {

// ------------------------------------------------------------------------------------
// weight packing: nn.Conv2d weight [Cout][Cin][KH][KW] f32 -> [Cout][KH][KW][Cin] bf16 hi (+ lo)
//   transpose_flip: data-gradient form  [Cin][KH][KW][Cout] with taps flipped
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_pack_weights(const float* __restrict__ w, int Cout, int Cin, int KH, int KW,
                                                         int transpose_flip, unsigned short* __restrict__ hi,
                                                         unsigned short* __restrict__ lo) {
    // destination [R][KH][KW][Cc_p]: R rows, Cc contraction channels padded to a multiple of 32 with zeros
    const int R = transpose_flip ? Cin : Cout, Cc = transpose_flip ? Cout : Cin;
    const int Cp = (Cc + 31) / 32 * 32;
    const long total = (long)R * KH * KW * Cp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % Cp);
        long t = i / Cp;
        const int kw = (int)(t % KW);
        t /= KW;
        const int kh = (int)(t % KH);
        const int rr = (int)(t / KH);
        float v = 0.0f;
        if (c < Cc) {
            if (transpose_flip) v = w[(((long)c * Cin + rr) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)];
            else v = w[(((long)rr * Cin + c) * KH + kh) * KW + kw];
        }
        const __bf16 bh = (__bf16)v;
        hi[i] = __builtin_bit_cast(unsigned short, bh);
        if (lo) {
            const __bf16 bl = (__bf16)(v - (float)bh);
            lo[i] = __builtin_bit_cast(unsigned short, bl);
        }
    }
}

// split-3 image for activations stored as [hi | lo | hi] (per concat segment): [Cout][KH][KW][3 * Cin] bf16 with the channel
// order [w_hi(seg) | w_hi(seg) | w_lo(seg)] for seg = the first C1 channels, then the remaining Cin - C1, so that the plain bf16
// contraction over the 3 * Cin channels is  x_hi w_hi + x_lo w_hi + x_hi w_lo  (the three products of the precise mode)
__global__ __launch_bounds__(256) void conv_pack_weights_s3(const float* __restrict__ w, int Cout, int Cin, int C1, int KH, int KW,
                                                            unsigned short* __restrict__ out) {
    const int C3 = 3 * Cin;
    const long total = (long)Cout * KH * KW * C3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int j = (int)(i % C3);
        long t = i / C3;
        const int kw = (int)(t % KW);
        t /= KW;
        const int kh = (int)(t % KH);
        const int co = (int)(t / KH);
        const bool second = j >= 3 * C1;
        const int cs = second ? Cin - C1 : C1;
        if (second) j -= 3 * C1;
        const int part = j / cs, c = (second ? C1 : 0) + (j - part * cs);
        const float v = w[(((long)co * Cin + c) * KH + kh) * KW + kw];
        const __bf16 bh = (__bf16)v;
        const __bf16 o = part == 2 ? (__bf16)(v - (float)bh) : bh;
        out[i] = __builtin_bit_cast(unsigned short, o);
    }
}

// Data gradient of a STRIDE-2 convolution without the dilated grid.  Forward: y[oh, ow] = sum_{kh, kw} Xp[2 oh + kh, 2 ow + kw] w[kh, kw]
// (Xp: the padded input).  An input row ip receives only the taps with (ip - kh) even:
//   3 taps:  ip = 2 i   <- kh = 2 from output row i - 1, kh = 0 from row i      (a 2-tap window starting at i - 1: "pad" 1)
//            ip = 2 i + 1 <- kh = 1 from row i                                    (1 tap, pad 0)
//   1 tap (1x1 layers):  ip = 2 i <- row i;  odd rows receive nothing (the output is zero-filled first).
// So the gradient is 4 (or 1) small stride-1 convolutions over gy -- one per parity class (ph, pw) of the output pixel -- whose
// results land on pixels (2 i + ph, 2 j + pw) (ConvArgs::omap): 9 taps of MFMA work per 4 output pixels instead of 36.
// Sub-images, data-gradient form [Cin][KH'][KW'][Cout padded to 32] (contraction over Cout), in class order (0,0), (0,1), (1,0), (1,1):
// class parity 0 holds the forward taps (2, 0) in window order, parity 1 the tap (1).
__global__ __launch_bounds__(256) void conv_pack_weights_s2(const float* __restrict__ w, int Cout, int Cin, int K,
                                                            unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
    const int Cp = (Cout + 31) / 32 * 32;
    const long per_tap = (long)Cp;                          // elements per (ci, tap)
    const int taps_total = K * K;                           // 9 (or 1): the classes partition the taps
    const long total = (long)Cin * taps_total * per_tap;
    // class (ph, pw): window sizes nh = (K == 3 ? (ph ? 1 : 2) : 1), same for nw; element order inside a class: [ci][th][tw][co]
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long t = i;
        int ph = 0, pw = 0, nh = 1, nw = 1;
        long base = 0;
        if (K == 3) {
            for (int cls = 0; cls < 4; ++cls) {
                ph = cls >> 1;
                pw = cls & 1;
                nh = ph ? 1 : 2;
                nw = pw ? 1 : 2;
                const long sz = (long)Cin * nh * nw * per_tap;
                if (t < base + sz) break;
                base += sz;
            }
        }
        t -= base;
        const int co = (int)(t % Cp);
        t /= Cp;
        const int tw = (int)(t % nw);
        t /= nw;
        const int th = (int)(t % nh);
        const int ci = (int)(t / nh);
        const int kh = K == 3 ? (ph ? 1 : (th == 0 ? 2 : 0)) : 0;
        const int kw = K == 3 ? (pw ? 1 : (tw == 0 ? 2 : 0)) : 0;
        float v = 0.0f;
        if (co < Cout) v = w[(((long)co * Cin + ci) * K + kh) * K + kw];
        const __bf16 bh = (__bf16)v;
        hi[i] = __builtin_bit_cast(unsigned short, bh);
        if (lo) {
            const __bf16 bl = (__bf16)(v - (float)bh);
            lo[i] = __builtin_bit_cast(unsigned short, bl);
        }
    }
}

size_t packed_elems(int Cout, int Cin, int KH, int KW, int transpose_flip) {
    const int R = transpose_flip ? Cin : Cout, Cc = transpose_flip ? Cout : Cin;
    return (size_t)R * KH * KW * ((Cc + 31) / 32 * 32);
}

// All kernel-side images of one K x K (K = 1 or 3) weight in ONE launch: a workgroup transposes a 32 (co) x 32 (ci) x K^2 tile
// through LDS (the fp32 weight is read once, in whole contiguous runs) and writes 64-byte runs of
//   fwd [Cout][K][K][Cin_p]            (bf16 hi; the forward image of conv_pack_weights)
//   tr  [Cin][K][K][Cout_p], taps flipped (the data-gradient image)
//   s3  [Cout][K][K][3 Cin]  = [w_hi | w_hi | w_lo] per concat segment (split-3, conv_pack_weights_s3)
// -- each optional.  Replaces three launches per layer and step (the weights change with every optimiser step).
template <int K>                                             // compile-time tap count: the index arithmetic is divisions by K * K
__global__ __launch_bounds__(256) void conv_pack_all_kernel(const float* __restrict__ w, int Cout, int Cin, int C1,
                                                            unsigned short* __restrict__ fwd, unsigned short* __restrict__ tr,
                                                            unsigned short* __restrict__ s3) {
    constexpr int KK = K * K;
    __shared__ float tile[32][32 * KK + 1];
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int Cin_p = (Cin + 31) / 32 * 32, Cout_p = (Cout + 31) / 32 * 32;
    constexpr int run = 32 * KK;                            // floats per co row of the tile (contiguous in w when ci0 + 32 <= Cin)
    for (int i = threadIdx.x; i < 32 * run; i += 256) {
        const int cr = i / run, e = i - cr * run;           // e = ci_local * KK + tap
        const int co = co0 + cr, ci = ci0 + e / KK;
        tile[cr][e] = (co < Cout && ci < Cin) ? w[((long)co * Cin + ci0) * KK + e] : 0.0f;
    }
    __syncthreads();
    // forward / split-3 images: (co, tap) rows, 32 ci contiguous = four 16-byte stores (8 bf16) per row
    auto pack8 = [](const float (&v)[8], u32x4& hi, u32x4* lo) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hi[e] = pack2(v[2 * e], v[2 * e + 1]);
            if (lo) (*lo)[e] = pack2(v[2 * e] - bf16_round(v[2 * e]), v[2 * e + 1] - bf16_round(v[2 * e + 1]));
        }
    };
    for (int i = threadIdx.x; i < 32 * KK * 4; i += 256) {
        const int c8 = i & 3, rt = i >> 2;                  // 8-channel chunk of the ci run, (co_local, tap)
        const int cr = rt / KK, tap = rt - cr * KK;
        const int co = co0 + cr, ci = ci0 + c8 * 8;
        if (co >= Cout || ci >= Cin_p) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[cr][(c8 * 8 + e) * KK + tap];
        u32x4 h4, l4;
        pack8(v, h4, &l4);
        if (fwd) *reinterpret_cast<u32x4*>(fwd + ((long)co * KK + tap) * Cin_p + ci) = h4;
        if (s3 && ci < Cin) {                               // Cin % 32 == 0 here: whole chunks
            const bool second = ci >= C1;
            const int cs = second ? Cin - C1 : C1, cloc = second ? ci - C1 : ci;
            unsigned short* row = s3 + ((long)co * KK + tap) * 3 * Cin + (second ? 3 * C1 : 0);
            *reinterpret_cast<u32x4*>(row + cloc) = h4;
            *reinterpret_cast<u32x4*>(row + cs + cloc) = h4;
            *reinterpret_cast<u32x4*>(row + 2 * cs + cloc) = l4;
        }
    }
    // data-gradient image: (ci, flipped tap) rows, 32 co contiguous
    if (tr)
        for (int i = threadIdx.x; i < 32 * KK * 4; i += 256) {
            const int c8 = i & 3, rt = i >> 2;              // 8-channel chunk of the co run, (ci_local, tap)
            const int cl = rt / KK, tap = rt - cl * KK;
            const int ci = ci0 + cl, co = co0 + c8 * 8;
            if (ci >= Cin || co >= Cout_p) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = tile[c8 * 8 + e][cl * KK + tap];     // rows co >= Cout of the tile are zero
            u32x4 h4;
            pack8(v, h4, nullptr);
            *reinterpret_cast<u32x4*>(tr + ((long)ci * KK + (KK - 1 - tap)) * Cout_p + co) = h4;
        }
}

hipError_t launch_pack_all(const float* w, int Cout, int Cin, int K, int C1, unsigned short* fwd, unsigned short* tr, unsigned short* s3,
                           hipStream_t st) {
    dim3 grid((unsigned)((Cin + 31) / 32), (unsigned)((Cout + 31) / 32));
    if (K == 3) hipLaunchKernelGGL(conv_pack_all_kernel<3>, grid, dim3(256), 0, st, w, Cout, Cin, C1, fwd, tr, s3);
    else hipLaunchKernelGGL(conv_pack_all_kernel<1>, grid, dim3(256), 0, st, w, Cout, Cin, C1, fwd, tr, s3);
    return hipGetLastError();
}

hipError_t launch_pack_weights_s2(const float* w, int Cout, int Cin, int K, unsigned short* hi, unsigned short* lo, hipStream_t st) {
    const long total = (long)Cin * K * K * ((Cout + 31) / 32 * 32);
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv_pack_weights_s2, dim3((unsigned)blocks), dim3(256), 0, st, w, Cout, Cin, K, hi, lo);
    return hipGetLastError();
}

hipError_t launch_pack_weights_s3(const float* w, int Cout, int Cin, int C1, int KH, int KW, unsigned short* out, hipStream_t st) {
    const long total = (long)Cout * KH * KW * 3 * Cin;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv_pack_weights_s3, dim3((unsigned)blocks), dim3(256), 0, st, w, Cout, Cin, C1, KH, KW, out);
    return hipGetLastError();
}

hipError_t launch_pack_weights(const float* w, int Cout, int Cin, int KH, int KW, int transpose_flip, unsigned short* hi,
                               unsigned short* lo, hipStream_t st) {
    const long total = (long)packed_elems(Cout, Cin, KH, KW, transpose_flip);
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv_pack_weights, dim3((unsigned)blocks), dim3(256), 0, st, w, Cout, Cin, KH, KW, transpose_flip, hi,
                       lo);
    return hipGetLastError();
}

}  // namespace vqseg
