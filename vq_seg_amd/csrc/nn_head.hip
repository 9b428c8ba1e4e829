// nn_head.hip -- the 1x1 segmentation head (gfx950), HBM-bound, and the slab sum of per-block partials that the weight gradients of
// the head and of the convolutions end with.
//
// Reference op: the 1x1 head conv (modified_vqunet/net.py:1169).  Rows are NHWC pixels (T = float, __bf16, or split-3: S3Row).
// Reductions are two-level with fixed order (no float atomics): results are run-to-run deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nn_device.h"
#include "nn_internal.h"

namespace vqseg {

// ---------------------------------------------------------------------------------------------
// 1x1 segmentation head (Cin <= 64 -> Cout <= 4, no bias): forward, data gradient, weight gradient
// ---------------------------------------------------------------------------------------------
// 8 consecutive channels of row `row` (Cin per row) as floats: T = float / __bf16 rows, or split-3 rows (S3Row tag: [hi | lo])
template <typename T>
__device__ __forceinline__ void ld8(const T* __restrict__ x, long row, int Cin, int c, float (&v)[8]) {
    if constexpr (__is_same(T, S3Row)) s3_load8(reinterpret_cast<const unsigned short*>(x) + row * 2 * Cin, Cin, c, v);
    else if constexpr (sizeof(T) == 2) ldv(x, row * Cin + c, v);
    else {
        float a[4], b[4];
        ldv(x, row * Cin + c, a);
        ldv(x, row * Cin + c + 4, b);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a[e], v[4 + e] = b[e];
    }
}

// forward: one pixel row per thread, 16-byte loads, the weights in LDS; the channel order of the fmaf chain is ascending (as the
// scalar form it replaces: bit-identical results).  Cin % 8 == 0, Cin <= 64, Cout <= 4.
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, long M, int Cin,
                                                       int Cout, float* __restrict__ y) {
    __shared__ float ws[4 * 64];
    for (int i = threadIdx.x; i < Cout * Cin; i += 256) ws[i] = w[i];
    __syncthreads();
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < Cin; c += 8) {
            float v[8];
            ld8<T>(x, m, Cin, c, v);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < Cout) acc[o] = __builtin_fmaf(v[e], ws[o * Cin + c + e], acc[o]);
        }
        for (int o = 0; o < Cout; ++o) y[m * Cout + o] = acc[o];
    }
}

// data gradient: thread = (row, 8-channel chunk), one 16-byte (bf16) / two 16-byte (f32) stores
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_data_kernel(const float* __restrict__ g, const float* __restrict__ w, long M,
                                                            int Cin, int Cout, T* __restrict__ gx, const T* __restrict__ gx_add) {
    __shared__ float ws[4 * 64];
    for (int i = threadIdx.x; i < Cout * Cin; i += 256) ws[i] = w[i];
    __syncthreads();
    const int cv = Cin / 8;
    const long total = M * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / cv;
        const int c = (int)(i - m * cv) * 8;
        float gv[4] = {0.f, 0.f, 0.f, 0.f};
        for (int o = 0; o < Cout; ++o) gv[o] = g[m * Cout + o];
        float out[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (o < Cout) a = __builtin_fmaf(gv[o], ws[o * Cin + c + e], a);
            out[e] = a;
        }
        if (gx_add) {
            // fan-in: the other consumer's gradient of the same tensor, added the way autograd would add the two (each rounded to T first)
            float ad[8];
            if constexpr (sizeof(T) == 2) {
                const u32x4 r = *reinterpret_cast<const u32x4*>(gx_add + m * Cin + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ad[2 * e] = __builtin_bit_cast(float, r[e] << 16);
                    ad[2 * e + 1] = __builtin_bit_cast(float, r[e] & 0xFFFF0000u);
                }
            } else {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(gx_add + m * Cin + c), a1 = *reinterpret_cast<const f32x4*>(gx_add + m * Cin + c + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) ad[e] = a0[e], ad[4 + e] = a1[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] = (float)(T)out[e] + ad[e];
        }
        if constexpr (sizeof(T) == 2) {
            u32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 lo = (__bf16)out[2 * e], hi = (__bf16)out[2 * e + 1];
                r[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
            }
            *reinterpret_cast<u32x4*>(gx + m * Cin + c) = r;
        } else {
            *reinterpret_cast<f32x4*>(gx + m * Cin + c) = f32x4{out[0], out[1], out[2], out[3]};
            *reinterpret_cast<f32x4*>(gx + m * Cin + c + 4) = f32x4{out[4], out[5], out[6], out[7]};
        }
    }
}

constexpr int HEAD_ROWS = 2048;
// weight gradient: block -> HEAD_ROWS rows; thread -> (row slot, 8-channel chunk): one 16-byte x load feeds 8 x Cout accumulators;
// the 256 / (Cin / 8) row slots are folded through LDS in slot order (deterministic); partial[blk][Cout * Cin]
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_weight_kernel(const T* __restrict__ x, const float* __restrict__ g, long M, int Cin,
                                                              int Cout, float* __restrict__ partial) {
    extern __shared__ float sh[];                              // [slots][Cout * Cin]
    const int cv = Cin / 8, slots = 256 / cv;
    const int cc = threadIdx.x % cv, sl = threadIdx.x / cv;
    const long row0 = (long)blockIdx.x * HEAD_ROWS;
    float acc[4][8];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[o][e] = 0.0f;
    if (sl < slots) {
        long end = row0 + HEAD_ROWS;
        if (end > M) end = M;
        for (long m = row0 + sl; m < end; m += slots) {
            float v[8];
            ld8<T>(x, m, Cin, cc * 8, v);
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (o < Cout) {
                    const float gv = g[m * Cout + o];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[o][e] = __builtin_fmaf(gv, v[e], acc[o][e]);
                }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < Cout)
#pragma unroll
                for (int e = 0; e < 8; ++e) sh[(sl * Cout + o) * Cin + cc * 8 + e] = acc[o][e];
    }
    __syncthreads();
    if ((int)threadIdx.x < Cin * Cout) {
        float s = 0.0f;
        for (int l = 0; l < slots; ++l) s += sh[l * Cout * Cin + threadIdx.x];
        partial[(long)blockIdx.x * Cin * Cout + threadIdx.x] = s;
    }
}

// sum partial[blk][n] over blk -> out[n] (double accumulate, fixed order).  A block covers 64 x 4 consecutive
// elements (float4 per thread); its 4 thread rows take the slabs b = row, row + 4, ... (two independent chains
// each, so several loads are in flight) and are folded through LDS in row order.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, long n_blocks, long n,
                                                              float* __restrict__ out, int accumulate) {
    __shared__ double sh[4][64][4];
    const int col = threadIdx.x & 63, rowl = threadIdx.x >> 6;
    const long i = ((long)blockIdx.x * 64 + col) * 4;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    const bool vec = (n & 3) == 0 && i + 3 < n;      // 16-byte aligned slab rows
    if (i < n) {
        long b = rowl;
        // the slab sums are latency bound (a thread's loads are its only work): four independent 16-byte loads in flight per
        // thread, added in the SAME order as the two-load loop below (s0: slabs b, b + 8, ...; s1: b + 4, b + 12, ...)
        if (vec)
            for (; b + 12 < n_blocks; b += 16) {
                const f32x4 u0 = *reinterpret_cast<const f32x4*>(partial + b * n + i);
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(partial + (b + 4) * n + i);
                const f32x4 u1 = *reinterpret_cast<const f32x4*>(partial + (b + 8) * n + i);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(partial + (b + 12) * n + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s0[e] += (double)u0[e];
                    s1[e] += (double)v0[e];
                    s0[e] += (double)u1[e];
                    s1[e] += (double)v1[e];
                }
            }
        for (; b + 4 < n_blocks; b += 8) {
            if (vec) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(partial + b * n + i);
                const f32x4 v = *reinterpret_cast<const f32x4*>(partial + (b + 4) * n + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s0[e] += (double)u[e];
                    s1[e] += (double)v[e];
                }
            } else {
                for (int e = 0; e < 4 && i + e < n; ++e) {
                    s0[e] += (double)partial[b * n + i + e];
                    s1[e] += (double)partial[(b + 4) * n + i + e];
                }
            }
        }
        if (b < n_blocks) {
            if (vec) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(partial + b * n + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) s0[e] += (double)u[e];
            } else {
                for (int e = 0; e < 4 && i + e < n; ++e) s0[e] += (double)partial[b * n + i + e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[rowl][col][e] = s0[e] + s1[e];
    __syncthreads();
    if (rowl == 0 && i < n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e < n) {
                const double t = ((sh[0][col][e] + sh[1][col][e]) + sh[2][col][e]) + sh[3][col][e];
                out[i + e] = accumulate ? out[i + e] + (float)t : (float)t;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_head_fwd(int bf16, const void* x, const float* w, long M, int Cin, int Cout, float* y, hipStream_t st_) {
    // bf16: 0 f32 rows, 1 bf16 rows, 2 split-3 rows
    const unsigned gr = grid_for(M);
    if (bf16 == 2) hipLaunchKernelGGL(head_fwd_kernel<S3Row>, dim3(gr), dim3(256), 0, st_, (const S3Row*)x, w, M, Cin, Cout, y);
    else if (bf16) hipLaunchKernelGGL(head_fwd_kernel<__bf16>, dim3(gr), dim3(256), 0, st_, (const __bf16*)x, w, M, Cin, Cout, y);
    else hipLaunchKernelGGL(head_fwd_kernel<float>, dim3(gr), dim3(256), 0, st_, (const float*)x, w, M, Cin, Cout, y);
    return hipGetLastError();
}

long head_bwd_blocks(long M) { return (M + HEAD_ROWS - 1) / HEAD_ROWS; }

template <typename T>
static void head_bwd_t(const void* x, const float* w, const float* g, long M, int Cin, int Cout, void* gx, float* partial,
                       const void* gx_add, long nb, hipStream_t st_) {
    hipLaunchKernelGGL(head_bwd_data_kernel<T>, dim3(grid_for(M * (Cin / 8))), dim3(256), 0, st_, g, w, M, Cin, Cout, (T*)gx, (const T*)gx_add);
    const size_t lds = (size_t)(256 / (Cin / 8)) * Cout * Cin * sizeof(float);
    hipLaunchKernelGGL(head_bwd_weight_kernel<T>, dim3((unsigned)nb), dim3(256), lds, st_, (const T*)x, g, M, Cin, Cout, partial);
}

hipError_t launch_head_bwd(int bf16, const void* x, const float* w, const float* g, long M, int Cin, int Cout, void* gx,
                           float* gw, float* partial, const void* gx_add, hipStream_t st_) {
    const long nb = head_bwd_blocks(M);
    if (bf16) head_bwd_t<__bf16>(x, w, g, M, Cin, Cout, gx, partial, gx_add, nb, st_);
    else head_bwd_t<float>(x, w, g, M, Cin, Cout, gx, partial, gx_add, nb, st_);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((Cin * Cout + 255) / 256), dim3(256), 0, st_, partial, nb, (long)Cin * Cout, gw, 0);
    return hipGetLastError();
}

hipError_t launch_reduce_partials(const float* partial, long n_blocks, long n, float* out, int accumulate, hipStream_t st_) {
    if (!(g_nn_opt.debug_skip_small & 4))
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st_, partial, n_blocks, n, out, accumulate);
    return hipGetLastError();
}

}  // namespace vqseg
