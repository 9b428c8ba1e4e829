// vq_codebook.hip -- everything that produces or updates a codebook: the exact kernel's image of it, the k-means update step (code sums),
// the EMA update and dead-code revival.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_internal.h"

namespace vqseg {

// ------------------------------------------------------------------------------------
// codebook preparation ("prepared codebook" blob, valid until the codebook changes):
//   E4[c/4][k][4]  (Cp/4 x Kp x 4, zero padded)  -- 4 channels of one code are one 16-byte
//                  LDS/HBM word, so one ds_read_b128 feeds four MFMAs
//   enorm[k]       |e_k|^2 as an ascending fmaf chain; +inf for k >= K (never selected)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vq_pack_codebook(const float* __restrict__ W, int K, int C,
                                                        float* __restrict__ E4, int Kp, int Cp) {
    // one thread per (c4, k): reads 16 B of row k, writes 16 B
    const long total = (long)(Cp / 4) * Kp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k = (int)(i % Kp);
        const int c = (int)(i / Kp) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < K && c < C) v = *reinterpret_cast<const f32x4*>(W + (size_t)k * C + c);   // C % 4 == 0
        reinterpret_cast<f32x4*>(E4)[i] = v;
    }
}

__global__ __launch_bounds__(64) void vq_code_norms(const float* __restrict__ W, int K, int C, int Kp,
                                                    float* __restrict__ enorm) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= Kp) return;
    float s = __builtin_inff();
    if (k < K) {
        s = 0.0f;
        const f32x4* row = reinterpret_cast<const f32x4*>(W + (size_t)k * C);
        const int n4 = C >> 2;
        int i = 0;
        for (; i + 8 <= n4; i += 8) {                            // 8 independent 16-B loads in flight
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = row[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) s = __builtin_fmaf(v[u][e], v[u][e], s);
        }
        for (; i < n4; ++i) {
            const f32x4 v = row[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_fmaf(v[e], v[e], s);
        }
    }
    enorm[k] = s;
}

// ------------------------------------------------------------------------------------
// k-means update step: per-cluster sums of the member rows, deterministic and insensitive to skewed cluster sizes.
//   1. km_hist:    row blocks of KM_RB rows -> hist[block][k] (LDS histogram, no global atomics)
//   2. km_scan:    counts[k], member-list offsets[k], per-(block, k) write cursors, and segment offsets
//                  (a cluster's member list is cut into segments of KM_SEG members)
//   3. km_lists:   one wave per row block walks its rows in order and appends them to the member lists (stable:
//                  lists are in row order)
//   4. km_segsum:  block = (segment, 64-channel group): 4 waves stride the segment's members, combine in wave order
//   5. km_sums:    per cluster, its segment partials are added in segment order
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_hist_kernel(const long long* __restrict__ idx, long N, int K, int* __restrict__ hist) {
    extern __shared__ int lh[];
    for (int k = threadIdx.x; k < K; k += 256) lh[k] = 0;
    __syncthreads();
    const long r0 = (long)blockIdx.x * KM_RB;
    for (int i = threadIdx.x; i < KM_RB; i += 256)
        if (r0 + i < N) atomicAdd(&lh[idx[r0 + i]], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) hist[(long)blockIdx.x * K + k] = lh[k];
}

// single block: counts, exclusive scans (member offsets, segment offsets), per-block cursors (in place of hist)
__global__ __launch_bounds__(1024) void km_scan_kernel(int* __restrict__ hist, int n_blocks, int K, int* __restrict__ counts,
                                                       int* __restrict__ offsets, int* __restrict__ segoff) {
    __shared__ int part[1024], spart[1024];
    const int per = (K + 1023) / 1024;
    const int b = threadIdx.x * per;
    int s = 0, ss = 0;
    for (int i = 0; i < per; ++i)
        if (b + i < K) {
            int c = 0;
            for (int j = 0; j < n_blocks; ++j) c += hist[(long)j * K + b + i];
            counts[b + i] = c;
            s += c;
            ss += (c + KM_SEG - 1) / KM_SEG;
        }
    part[threadIdx.x] = s;
    spart[threadIdx.x] = ss;
    __syncthreads();
    for (int m = 1; m < 1024; m <<= 1) {
        const int v = (threadIdx.x >= m) ? part[threadIdx.x - m] : 0;
        const int w = (threadIdx.x >= m) ? spart[threadIdx.x - m] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        spart[threadIdx.x] += w;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s, srun = spart[threadIdx.x] - ss;
    for (int i = 0; i < per; ++i)
        if (b + i < K) {
            const int c = counts[b + i];
            offsets[b + i] = run;
            segoff[b + i] = srun;
            int cur = run;                                  // cursor of each row block inside this cluster's list
            for (int j = 0; j < n_blocks; ++j) {
                const int h = hist[(long)j * K + b + i];
                hist[(long)j * K + b + i] = cur;
                cur += h;
            }
            run += c;
            srun += (c + KM_SEG - 1) / KM_SEG;
        }
    if (threadIdx.x == 1023) {
        offsets[K] = part[1023];
        segoff[K] = spart[1023];
    }
}

__global__ __launch_bounds__(64) void km_lists_kernel(const long long* __restrict__ idx, long N, int K,
                                                      const int* __restrict__ cursors, int* __restrict__ members) {
    // one wave per row block; rows in order, 64 at a time; equal clusters inside a chunk are ranked by lane
    extern __shared__ int cur[];
    const int lane = threadIdx.x;
    for (int k = lane; k < K; k += 64) cur[k] = cursors[(long)blockIdx.x * K + k];
    __syncthreads();
    const long r0 = (long)blockIdx.x * KM_RB;
    for (int base = 0; base < KM_RB && r0 + base < N; base += 64) {
        const long i = r0 + base + lane;
        const bool valid = i < N;
        const int k = valid ? (int)idx[i] : -1;
        bool todo = valid;
        while (__ballot(todo)) {
            const int lead = __ffsll((long long)__ballot(todo)) - 1;
            const int kk = __shfl(k, lead);
            const unsigned long long same = __ballot(todo && k == kk);
            if (todo && k == kk) {
                members[cur[kk] + __popcll(same & ((1ull << lane) - 1ull))] = (int)i;
                todo = false;
            }
            __syncthreads();                                // (one wave) order the cursor update after the reads
            if (lane == lead) cur[kk] += __popcll(same);
            __syncthreads();
        }
    }
}

template <typename TS>
__global__ __launch_bounds__(256) void km_segsum_kernel(const TS* __restrict__ samples, int C, int K,
                                                        const int* __restrict__ offsets, const int* __restrict__ segoff,
                                                        const int* __restrict__ members, float* __restrict__ partial) {
    const int seg = blockIdx.x;
    if (seg >= segoff[K]) return;
    int lo = 0, hi = K;                                     // cluster of this segment: last k with segoff[k] <= seg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segoff[mid] <= seg) lo = mid;
        else hi = mid;
    }
    const int k = lo;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const int b = offsets[k] + (seg - segoff[k]) * KM_SEG;
    int e = b + KM_SEG;
    if (e > offsets[k + 1]) e = offsets[k + 1];
    float s = 0.0f;
    if (c < C)
        for (int m = b + wave; m < e; m += 4) s += (float)samples[(size_t)members[m] * C + c];
    __shared__ float sh[4][64];
    sh[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C) partial[(size_t)seg * C + c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

__global__ __launch_bounds__(256) void km_sums_kernel(const float* __restrict__ partial, int C, const int* __restrict__ segoff,
                                                      float* __restrict__ sums) {
    // block = (cluster, 64-channel group); 4 thread rows stride the cluster's segments, folded in row order
    __shared__ float sh[4][64];
    const int k = blockIdx.x;
    const int lane = threadIdx.x & 63, rowl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    float s = 0.0f;
    if (c < C)
        for (int g = segoff[k] + rowl; g < segoff[k + 1]; g += 4) s += partial[(size_t)g * C + c];
    sh[rowl][lane] = s;
    __syncthreads();
    if (rowl == 0 && c < C) sums[(size_t)k * C + c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

__global__ __launch_bounds__(256) void km_counts64_kernel(const int* __restrict__ counts, int K, long long* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) out[k] = counts[k];
}

__global__ __launch_bounds__(256) void km_finalize_kernel(const float* __restrict__ sums, const long long* __restrict__ counts,
                                                          float* __restrict__ means, int C) {
    const int k = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const long long n = counts[k];
    if (n > 0) means[(size_t)k * C + c] = sums[(size_t)k * C + c] / (float)n;      // vq_img.py:53; :58-61 keep if empty
}

// ---- opt-in EMA codebook update (an EXTENSION: the reference keeps `decay`/`eps` but never updates the codebook).
// The published rule the reference's module descends from (vector-quantize-pytorch EuclideanCodebook.forward):
//   cluster_size <- d cluster_size + (1-d) counts;  embed_avg <- d embed_avg + (1-d) sums;
//   codebook     <- embed_avg / ((cluster_size + eps) / (sum cluster_size + K eps) * sum cluster_size)
// Both steps exist plain and with dead-code revival fused in (REVIVE, below): one body each, so that the two cannot drift apart -- *total
// sums the updated counts in the same tree either way.
template <bool REVIVE>
__device__ __forceinline__ void ema_counts_body(float* __restrict__ cluster_size, const long long* __restrict__ counts, int K, float decay,
                                                float* __restrict__ total, const float* __restrict__ ok, float threshold,
                                                float* __restrict__ revive, long long* __restrict__ t, long long* __restrict__ revived) {
    // one workgroup: update the K moving counts and leave their sum (fixed tree order) in *total.  REVIVE: + the expiry: revive[k] = 1
    // and cluster_size[k] = threshold where the updated count is below the threshold and the candidate is usable (*total sums the
    // updated counts BEFORE any reset); one more update counted
    __shared__ float sh[256];
    __shared__ int shn[REVIVE ? 256 : 1];
    float s = 0.0f;
    int n = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float v = __builtin_fmaf(cluster_size[k], decay, (1.0f - decay) * (float)counts[k]);
        if constexpr (REVIVE) {
            const bool r = v < threshold && ok[k] > 0.0f;
            cluster_size[k] = r ? threshold : v;
            revive[k] = r ? 1.0f : 0.0f;
            n += r ? 1 : 0;
        } else {
            cluster_size[k] = v;
        }
        s += v;
    }
    sh[threadIdx.x] = s;
    if constexpr (REVIVE) shn[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[threadIdx.x] += sh[threadIdx.x + w];
            if constexpr (REVIVE) shn[threadIdx.x] += shn[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = sh[0];
        if constexpr (REVIVE) {
            *revived = shn[0];
            *t = *t + 1;
        }
    }
}

template <bool REVIVE>
__device__ __forceinline__ void ema_embed_body(float* __restrict__ embed_avg, const float* __restrict__ sums,
                                               const float* __restrict__ cluster_size, const float* __restrict__ total,
                                               float* __restrict__ codebook, int K, int C, float decay, float eps,
                                               const float* __restrict__ cand, const float* __restrict__ revive, float threshold) {
    const int k = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const size_t o = (size_t)k * C + c;
    if constexpr (REVIVE) {
        if (revive[k] > 0.0f) {                              // uniform over the block
            const float s = cand[o];
            embed_avg[o] = s * threshold;
            codebook[o] = s;
            return;
        }
    }
    const float n = *total;
    const float smoothed = (cluster_size[k] + eps) / (n + (float)K * eps) * n;
    const float avg = __builtin_fmaf(embed_avg[o], decay, (1.0f - decay) * sums[o]);
    embed_avg[o] = avg;
    codebook[o] = avg / smoothed;
}

__global__ __launch_bounds__(256) void ema_counts_kernel(float* __restrict__ cluster_size, const long long* __restrict__ counts, int K,
                                                         float decay, float* __restrict__ total) {
    ema_counts_body<false>(cluster_size, counts, K, decay, total, nullptr, 0.0f, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void ema_embed_kernel(float* __restrict__ embed_avg, const float* __restrict__ sums,
                                                        const float* __restrict__ cluster_size, const float* __restrict__ total,
                                                        float* __restrict__ codebook, int K, int C, float decay, float eps) {
    ema_embed_body<false>(embed_avg, sums, cluster_size, total, codebook, K, C, decay, eps, nullptr, nullptr, 0.0f);
}

// ---- dead-code revival, the companion of the EMA rule in the same library (EXTENSION, include/vqseg.h): a code whose UPDATED
// moving count lies below the threshold takes a row of the current batch.  Which row is a pure function of (seed, t, k):
// splitmix64 at counter t * 2^32 + k + 1, reduced modulo world * N; nothing is drawn from a generator and nothing is kept.
__device__ __forceinline__ unsigned long long revive_hash(unsigned long long seed, unsigned long long t, unsigned k) {
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * ((t << 32) + (unsigned long long)k + 1ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7F800000u) != 0x7F800000u; }

template <typename TS>
__global__ __launch_bounds__(256) void revive_candidates_kernel(const TS* __restrict__ rows, long N, int C, unsigned long long seed,
                                                                const long long* __restrict__ t, int rank, int world,
                                                                float* __restrict__ cand, float* __restrict__ ok) {
    // block = code k: its candidate row (16-byte loads, float4 stores) if this rank holds it, zeros if another rank does -- the sum over
    // ranks (the all-reduce the code sums travel in) is then the row itself
    const int k = blockIdx.x;
    const unsigned long long g = revive_hash(seed, (unsigned long long)*t, (unsigned)k) % ((unsigned long long)world * (unsigned long long)N);
    const unsigned long long NN = (unsigned long long)N;
    const bool mine = g / NN == (unsigned long long)rank;
    const size_t j = (size_t)(g % NN);
    float4* __restrict__ out = reinterpret_cast<float4*>(cand + (size_t)k * C);
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    if (!mine) {
        for (int q = threadIdx.x; q < C / 4; q += 256) out[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (threadIdx.x == 0) ok[k] = 0.0f;
        return;
    }
    bool nonfinite = false;
    if constexpr (sizeof(TS) == 4) {
        const uint4* __restrict__ in = reinterpret_cast<const uint4*>(rows + j * C);
        for (int q = threadIdx.x; q < C / 4; q += 256) {
            const uint4 v = in[q];
            nonfinite |= !(finite_bits(v.x) && finite_bits(v.y) && finite_bits(v.z) && finite_bits(v.w));
            out[q] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    } else {
        const uint4* __restrict__ in = reinterpret_cast<const uint4*>(rows + j * C);      // 8 bf16: float32 = the bits << 16, exactly
        for (int q = threadIdx.x; q < C / 8; q += 256) {
            const uint4 v = in[q];
            const unsigned w[8] = {v.x << 16, v.x & 0xFFFF0000u, v.y << 16, v.y & 0xFFFF0000u,
                                   v.z << 16, v.z & 0xFFFF0000u, v.w << 16, v.w & 0xFFFF0000u};
            for (int i = 0; i < 8; ++i) nonfinite |= !finite_bits(w[i]);
            out[2 * q] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
            out[2 * q + 1] = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]), __uint_as_float(w[7]));
        }
    }
    if (nonfinite) bad = 1;                                  // every writer stores the same value
    __syncthreads();
    if (threadIdx.x == 0) ok[k] = bad ? 0.0f : 1.0f;
}

__global__ __launch_bounds__(256) void ema_counts_revive_kernel(float* __restrict__ cluster_size, const long long* __restrict__ counts,
                                                                int K, float decay, float* __restrict__ total,
                                                                const float* __restrict__ ok, float threshold, float* __restrict__ revive,
                                                                long long* __restrict__ t, long long* __restrict__ revived) {
    ema_counts_body<true>(cluster_size, counts, K, decay, total, ok, threshold, revive, t, revived);
}

__global__ __launch_bounds__(256) void ema_embed_revive_kernel(float* __restrict__ embed_avg, const float* __restrict__ sums,
                                                               const float* __restrict__ cluster_size, const float* __restrict__ total,
                                                               float* __restrict__ codebook, int K, int C, float decay, float eps,
                                                               const float* __restrict__ cand, const float* __restrict__ revive,
                                                               float threshold) {
    ema_embed_body<true>(embed_avg, sums, cluster_size, total, codebook, K, C, decay, eps, cand, revive, threshold);
}

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
void launch_prepare_exact(const float* W, int K, int C, int Kp, float* E4, float* enorm, hipStream_t st) {
    long total = (long)(C / 4) * Kp;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(vq_pack_codebook, dim3((unsigned)blocks), dim3(256), 0, st, W, K, C, E4, Kp, C);
    hipLaunchKernelGGL(vq_code_norms, dim3((Kp + 63) / 64), dim3(64), 0, st, W, K, C, Kp, enorm);
}

template <typename TS>
static hipError_t code_sums_from_idx(const TS* samples, const int64_t* idx, int64_t N, int C, int K, const KmPlan& p, char* ws,
                                     float* sums, int64_t* counts64, hipStream_t st) {
    int* counts = reinterpret_cast<int*>(ws + p.off_counts);
    int* offsets = reinterpret_cast<int*>(ws + p.off_offsets);
    int* members = reinterpret_cast<int*>(ws + p.off_members);
    int* hist = reinterpret_cast<int*>(ws + p.off_hist);
    int* segoff = reinterpret_cast<int*>(ws + p.off_segoff);
    float* partial = reinterpret_cast<float*>(ws + p.off_partial);
    const long long* idx64 = reinterpret_cast<const long long*>(idx);
    hipLaunchKernelGGL(km_hist_kernel, dim3(p.row_blocks), dim3(256), (size_t)K * sizeof(int), st, idx64, (long)N, K, hist);
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, st, hist, p.row_blocks, K, counts, offsets, segoff);
    hipLaunchKernelGGL(km_lists_kernel, dim3(p.row_blocks), dim3(64), (size_t)K * sizeof(int), st, idx64, (long)N, K, hist, members);
    hipLaunchKernelGGL(km_segsum_kernel<TS>, dim3(p.max_segments, (C + 63) / 64), dim3(256), 0, st, samples, C, K, offsets, segoff,
                       members, partial);
    hipLaunchKernelGGL(km_sums_kernel, dim3(K, (C + 63) / 64), dim3(256), 0, st, partial, C, segoff, sums);
    hipLaunchKernelGGL(km_counts64_kernel, dim3((K + 255) / 256), dim3(256), 0, st, counts, K,
                       reinterpret_cast<long long*>(counts64));
    return hipGetLastError();
}

hipError_t launch_code_sums(const void* x, int x_bf16, const int64_t* idx, int64_t N, int C, int K, const KmPlan& p, char* ws,
                            float* sums, int64_t* counts64, hipStream_t st) {
    return x_bf16 ? code_sums_from_idx(static_cast<const __bf16*>(x), idx, N, C, K, p, ws, sums, counts64, st)
                  : code_sums_from_idx(static_cast<const float*>(x), idx, N, C, K, p, ws, sums, counts64, st);
}

hipError_t launch_ema_update(float* cluster_size, float* embed_avg, float* codebook, const float* sums, const int64_t* counts64,
                             int K, int C, float decay, float eps, float* total, hipStream_t st) {
    hipLaunchKernelGGL(ema_counts_kernel, dim3(1), dim3(256), 0, st, cluster_size, reinterpret_cast<const long long*>(counts64), K,
                       decay, total);
    hipLaunchKernelGGL(ema_embed_kernel, dim3(K, (C + 255) / 256), dim3(256), 0, st, embed_avg, sums, cluster_size, total, codebook,
                       K, C, decay, eps);
    return hipGetLastError();
}

hipError_t launch_revive_candidates(const void* x, int x_bf16, int64_t N, int C, int K, uint64_t seed, const int64_t* t, int rank,
                                    int world, float* cand, float* ok, hipStream_t st) {
    const long long* tp = reinterpret_cast<const long long*>(t);
    if (x_bf16)
        hipLaunchKernelGGL(revive_candidates_kernel<__bf16>, dim3(K), dim3(256), 0, st, static_cast<const __bf16*>(x), (long)N, C,
                           (unsigned long long)seed, tp, rank, world, cand, ok);
    else
        hipLaunchKernelGGL(revive_candidates_kernel<float>, dim3(K), dim3(256), 0, st, static_cast<const float*>(x), (long)N, C,
                           (unsigned long long)seed, tp, rank, world, cand, ok);
    return hipGetLastError();
}

hipError_t launch_ema_update_revive(float* cluster_size, float* embed_avg, float* codebook, const float* sums, const int64_t* counts64,
                                    int K, int C, float decay, float eps, float* scratch, const float* cand, const float* ok,
                                    float threshold, int64_t* t, int64_t* revived, hipStream_t st) {
    float* total = scratch;                                  // scratch: [total | revive flags K]
    float* revive = scratch + 1;
    hipLaunchKernelGGL(ema_counts_revive_kernel, dim3(1), dim3(256), 0, st, cluster_size, reinterpret_cast<const long long*>(counts64), K,
                       decay, total, ok, threshold, revive, reinterpret_cast<long long*>(t), reinterpret_cast<long long*>(revived));
    hipLaunchKernelGGL(ema_embed_revive_kernel, dim3(K, (C + 255) / 256), dim3(256), 0, st, embed_avg, sums, cluster_size, total,
                       codebook, K, C, decay, eps, cand, revive, threshold);
    return hipGetLastError();
}

hipError_t launch_km_finalize(const float* sums, const int64_t* counts64, float* means, int C, int K, hipStream_t st) {
    hipLaunchKernelGGL(km_finalize_kernel, dim3(K, (C + 255) / 256), dim3(256), 0, st, sums,
                       reinterpret_cast<const long long*>(counts64), means, C);
    return hipGetLastError();
}

}  // namespace vqseg
