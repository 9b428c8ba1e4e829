// vq_tail.hip -- what runs around the argmin of the vector quantiser: the pre-set of a grouped launch, keys -> indices and the code
// histogram, gather + straight-through + commitment loss, and the two backward kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_internal.h"

namespace vqseg {

// the pre-set of a grouped launch (VqInitGroup, vq_internal.h)
static_assert(F_LISTS + 1 <= 128, "the init launch zeroes 128 ints of a level's counter block");
__global__ __launch_bounds__(256) void vq_group_init_kernel(const VqInitGroup g) {
    int q = 0;
    while (q + 1 < g.n && blockIdx.x >= g.lv[q].end) ++q;
    const VqInitLevel& L = g.lv[q];
    const unsigned first = q ? g.lv[q - 1].end : 0u, nb = L.end - first, b = blockIdx.x - first;
    for (long i = (long)b * 256 + threadIdx.x; i < L.n; i += (long)nb * 256) L.keys[i] = ~0ull;
    if (b == 0) {
        if (L.amb && threadIdx.x < 128) L.amb[threadIdx.x] = 0;
        for (int k = threadIdx.x; k < L.kp; k += 256) L.hist[k] = 0;
    }
}

// keys -> int64 code indices (+ the winning distance), and the code histogram of the dead-code statistic (vq_img.py:173-175):
// counted per workgroup in LDS (few codes win most rows -- thousands of rows per address: global atomics would serialise in the
// L2 atomic units; round 1 did that from the gather kernel and sat at ~1 TB/s), then one global add per NON-EMPTY bin and
// workgroup.  Integer adds: order independent, deterministic.
__global__ __launch_bounds__(256) void vq_unpack_keys(const unsigned long long* __restrict__ keys, long N,
                                                      long long* __restrict__ idx, float* __restrict__ dmin,
                                                      int* __restrict__ hist, int K, int lds_hist) {
    extern __shared__ int lh[];
    if (hist && lds_hist)
        for (int k = threadIdx.x; k < K; k += 256) lh[k] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        const unsigned long long k = keys[i];
        unsigned code = (unsigned)(k & 0xffffffffull);
        if (code >= (unsigned)K) code = 0u;                       // last line of defence (no path should leave such a key): idx feeds unchecked gathers
        idx[i] = (long long)code;
        if (dmin) dmin[i] = __uint_as_float((unsigned int)(k >> 32));
        if (hist && code < (unsigned)K) atomicAdd((lds_hist ? lh : hist) + code, 1);   // K beyond the LDS budget: global bins
    }
    if (hist && lds_hist) {
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 256) {
            const int c = lh[k];
            if (c) atomicAdd(hist + k, c);
        }
    }
}

// ------------------------------------------------------------------------------------
// gather + straight-through + commitment partial sums + code histogram (HBM-bound)
// ------------------------------------------------------------------------------------
template <typename TA>
__device__ __forceinline__ f32x4 ld4(const TA* p, long v) {                 // elements 4v .. 4v+3 as floats
    if constexpr (sizeof(TA) == 4) {
        return reinterpret_cast<const f32x4*>(p)[v];
    } else {
        const u32x2 r = reinterpret_cast<const u32x2*>(p)[v];
        return f32x4{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xFFFF0000u),
                     __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xFFFF0000u)};
    }
}
template <typename TA>
__device__ __forceinline__ void st4(TA* p, long v, const f32x4& q) {
    if constexpr (sizeof(TA) == 4) {
        reinterpret_cast<f32x4*>(p)[v] = q;
    } else {
        u32x2 r;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const __bf16 lo = (__bf16)q[2 * e], hi = (__bf16)q[2 * e + 1];
            r[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
        }
        reinterpret_cast<u32x2*>(p)[v] = r;
    }
}

// TA = S3Row (eval only: split-3 rows never reach a training forward): quant is [N][2C] = [hi | lo] of the winning fp32 code row,
// split by s3_store8 -- the function s3_split_kernel applies, so the bytes are those of the fp32 gather followed by that kernel; x
// is not read.  8 channels per lane there (C % 8 == 0).
template <typename TA>
__global__ __launch_bounds__(256) void vq_gather_kernel(const TA* __restrict__ x, const float* __restrict__ W,
                                                        const long long* __restrict__ idx, long N, int C,
                                                        int training, TA* __restrict__ quant,
                                                        float* __restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = C >> 2;
    float sq = 0.0f;
    // one wave per group of RG consecutive rows (their loads are all issued before the first use), grid-stride over groups.
    // (Per-lane squared-error partials accumulate in a fixed (group, chunk, row) order: deterministic.)
    constexpr int RG = 4;
    for (long row0 = ((long)blockIdx.x * 4 + wave) * RG; row0 < N; row0 += (long)gridDim.x * 4 * RG) {
        long long k[RG];
#pragma unroll
        for (int j = 0; j < RG; ++j) k[j] = row0 + j < N ? idx[row0 + j] : 0;
        if constexpr (__is_same(TA, S3Row)) {
            for (int v = lane; v < (C >> 3); v += 64) {
                f32x4 e0[RG], e1[RG];
#pragma unroll
                for (int j = 0; j < RG; ++j)
                    if (row0 + j < N) {
                        e0[j] = reinterpret_cast<const f32x4*>(W + k[j] * (long)C)[2 * v];
                        e1[j] = reinterpret_cast<const f32x4*>(W + k[j] * (long)C)[2 * v + 1];
                    }
#pragma unroll
                for (int j = 0; j < RG; ++j)
                    if (row0 + j < N) {
                        const float q[8] = {e0[j][0], e0[j][1], e0[j][2], e0[j][3], e1[j][0], e1[j][1], e1[j][2], e1[j][3]};
                        s3_store8(reinterpret_cast<unsigned short*>(quant) + (row0 + j) * 2L * C, C, 8 * v, q);
                    }
            }
            continue;
        }
        for (int v = lane; v < c4; v += 64) {
            f32x4 e[RG], xv[RG];
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                if (row0 + j < N) {
                    e[j] = reinterpret_cast<const f32x4*>(W + k[j] * (long)C)[v];
                    if (training) xv[j] = ld4<TA>(x + (row0 + j) * (long)C, v);
                }
            }
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                if (row0 + j < N) {
                    TA* qr = quant + (row0 + j) * (long)C;
                    if (training) {
                        f32x4 q;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            q[i] = xv[j][i] + (e[j][i] - xv[j][i]);   // vq_img.py:236, fp32
                            const float dlt = q[i] - xv[j][i];
                            sq = __builtin_fmaf(dlt, dlt, sq);
                        }
                        st4<TA>(qr, v, q);
                    } else {
                        st4<TA>(qr, v, e[j]);
                    }
                }
            }
        }
    }
    // deterministic block reduction (fixed shuffle tree, fixed wave order)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m);
    __shared__ float wsum[4];
    if (lane == 0) wsum[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void vq_finalize_kernel(const float* __restrict__ partial, int n_partial,
                                                          const int* __restrict__ hist, int K, int training,
                                                          float commitment_weight, double numel,
                                                          float* __restrict__ loss, float* __restrict__ dead_pct) {
    __shared__ double sd[256];
    __shared__ int sz[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += (double)partial[i];
    int z = 0;
    for (int k = threadIdx.x; k < K; k += 256) z += (hist[k] == 0);
    sd[threadIdx.x] = s;
    sz[threadIdx.x] = z;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) {
            sd[threadIdx.x] += sd[threadIdx.x + m];
            sz[threadIdx.x] += sz[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float l = 0.0f;
        if (training && commitment_weight > 0.0f) l = (float)(sd[0] / numel) * commitment_weight;
        loss[0] = l;
        dead_pct[0] = 100.0f * ((float)sz[0] / (float)K);       // vq_img.py:174-175
    }
}

__global__ __launch_bounds__(256) void vq_backward_kernel(const float* __restrict__ gq, const float* __restrict__ gloss,
                                                          const float* __restrict__ x, const float* __restrict__ q,
                                                          long n4, float coef, float* __restrict__ gx) {
    const float k = gloss ? gloss[0] * coef : 0.0f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 g = reinterpret_cast<const f32x4*>(gq)[i];
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 qv = reinterpret_cast<const f32x4*>(q)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(k, xv[j] - qv[j], g[j]);
        reinterpret_cast<f32x4*>(gx)[i] = o;
    }
}

// bf16 activations: the quantised rows are not kept for backward (their bf16 image would cost the commitment gradient
// its accuracy); the code index is, and e = W[idx] is re-read in fp32:  gx = g + k (x - e)
__global__ __launch_bounds__(256) void vq_backward_idx_kernel(const __bf16* __restrict__ gq, const float* __restrict__ gloss,
                                                              const __bf16* __restrict__ x, const long long* __restrict__ idx,
                                                              const float* __restrict__ W, long N, int C, float coef,
                                                              __bf16* __restrict__ gx) {
    const float k = gloss ? gloss[0] * coef : 0.0f;
    const int c4 = C >> 2;
    const long n4 = N * c4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const long row = i / c4;
        const int v = (int)(i - row * c4);
        const f32x4 g = ld4<__bf16>(gq, i), xv = ld4<__bf16>(x, i);
        const f32x4 e = reinterpret_cast<const f32x4*>(W + idx[row] * (long)C)[v];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(k, xv[j] - e[j], g[j]);
        st4<__bf16>(gx, i, o);
    }
}

// ------------------------------------------------------------------------------------
// launchers (init / unpack: called by vq_host.hip inside a grouped launch; the rest: by the C ABI)
// ------------------------------------------------------------------------------------
void launch_group_init(const VqInitGroup& ig, hipStream_t st) {
    hipLaunchKernelGGL(vq_group_init_kernel, dim3(ig.lv[ig.n - 1].end), dim3(256), 0, st, ig);
}

void launch_unpack_level(int i, const int64_t* N, const int* K, const VqPlan* plans, char* const* ws, int64_t* const* idx,
                         float* const* dmin, hipStream_t st) {
    int* hist = reinterpret_cast<int*>(ws[i] + plans[i].off_hist);       // (zeroed by the init launch)
    long blocks = (N[i] + 1023) / 1024;                      // >= 1024 rows per workgroup: the LDS histogram pays
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    const int lds_hist = K[i] <= 8192;                       // 32 KB of LDS bins; larger codebooks count in global memory (rare
                                                             // winners per address there, so the L2 atomics do not serialise)
    hipLaunchKernelGGL(vq_unpack_keys, dim3((unsigned)blocks), dim3(256), lds_hist ? (size_t)K[i] * sizeof(int) : 0, st,
                       reinterpret_cast<unsigned long long*>(ws[i] + plans[i].off_keys), (long)N[i],
                       reinterpret_cast<long long*>(idx[i]), dmin ? dmin[i] : nullptr, hist, K[i], lds_hist);
}

hipError_t launch_gather(const void* x, int bf16, const float* W, const int64_t* idx, int64_t N, int C, int K, int training,
                         float cw, const VqPlan& p, char* ws, void* quant, float* loss, float* dead, hipStream_t st) {
    int* hist = reinterpret_cast<int*>(ws + p.off_hist);
    float* partial = reinterpret_cast<float*>(ws + p.off_partial);
    // hist: filled by launch_assign (vq_unpack_keys), which every forward runs first on the same workspace
    if (bf16 == VQ_ROWS_S3)
        hipLaunchKernelGGL(vq_gather_kernel<S3Row>, dim3(p.gather_blocks), dim3(256), 0, st, static_cast<const S3Row*>(x), W,
                           reinterpret_cast<const long long*>(idx), (long)N, C, 0, static_cast<S3Row*>(quant), partial);
    else if (bf16)
        hipLaunchKernelGGL(vq_gather_kernel<__bf16>, dim3(p.gather_blocks), dim3(256), 0, st, static_cast<const __bf16*>(x), W,
                           reinterpret_cast<const long long*>(idx), (long)N, C, training, static_cast<__bf16*>(quant), partial);
    else
        hipLaunchKernelGGL(vq_gather_kernel<float>, dim3(p.gather_blocks), dim3(256), 0, st, static_cast<const float*>(x), W,
                           reinterpret_cast<const long long*>(idx), (long)N, C, training, static_cast<float*>(quant), partial);
    hipLaunchKernelGGL(vq_finalize_kernel, dim3(1), dim3(256), 0, st, partial, p.gather_blocks, hist, K, training, cw,
                       (double)N * (double)C, loss, dead);
    return hipGetLastError();
}

hipError_t launch_backward(const float* gq, const float* gloss, const float* x, const float* q, int64_t N, int C,
                           float cw, float* gx, hipStream_t st) {
    const long n4 = (long)N * C / 4;
    const float coef = (float)((double)cw * 2.0 / ((double)N * (double)C));
    long blocks = (n4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(vq_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, st, gq, gloss, x, q, n4, coef, gx);
    return hipGetLastError();
}

hipError_t launch_backward_idx(const void* gq, const float* gloss, const void* x, const int64_t* idx, const float* W, int64_t N,
                               int C, float cw, void* gx, hipStream_t st) {
    const long n4 = (long)N * C / 4;
    const float coef = (float)((double)cw * 2.0 / ((double)N * (double)C));
    long blocks = (n4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(vq_backward_idx_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const __bf16*>(gq), gloss,
                       static_cast<const __bf16*>(x), reinterpret_cast<const long long*>(idx), W, (long)N, C, coef,
                       static_cast<__bf16*>(gx));
    return hipGetLastError();
}

}  // namespace vqseg
