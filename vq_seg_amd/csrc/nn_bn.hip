// nn_bn.hip -- BatchNorm on NHWC rows (gfx950), HBM-bound: statistics merge / finalize, eval coefficients, apply (+ ReLU, residual),
// and the backward through the fused ReLU / residual.
//
// Reference ops: nn.BatchNorm2d + nn.ReLU inside conv_bn_relu (models/networks/unet/decoder.py:7-10) and the ResNet blocks.
// Reductions are two-level with fixed order (no float atomics): results are run-to-run deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nn_device.h"
#include "nn_internal.h"

namespace vqseg {

#ifndef BN_UNROLL
#define BN_UNROLL 1               // vectors in flight per thread in the streaming BatchNorm loops (A/B builds: make ab ABFLAGS=-DBN_UNROLL=2)
#endif
// ---------------------------------------------------------------------------------------------
// BatchNorm forward statistics
// ---------------------------------------------------------------------------------------------
// Merge the per-slot partials (mean_s, M2_s over rows_per_slot rows) written by the conv epilogue.  In DOUBLE
// the plain power sums are exact enough (the inputs are floats: 29 spare bits against the cancellation in
// S2 - M mean^2) and need no divisions:
//   S1 = sum n_s mean_s        S2 = sum (M2_s + n_s mean_s^2)        mean = S1 / M        M2 = S2 - M mean^2
// Level 1 (bn_stats_merge_kernel): grid (64-channel groups, slot groups); a block sums its slots (reads coalesced
// along the channels, fixed order) and writes (S1, S2) back IN PLACE into its first two slots as (hi, lo) float
// pairs, so the whole merge stays in double.  Level 2 (bn_finalize_kernel) sums the group results and derives
// scale = gamma * invstd, shift = beta - mean * scale and the running-stat update (nn.BatchNorm2d: biased
// variance to normalise, unbiased for running_var).
// device-coherent accesses (sc1: written through / read past this XCD's L2) for results one workgroup hands to another inside a launch
__device__ __forceinline__ void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct PowerSums {
    double s1, s2;
};

// sum slots s0, s0 + step, ... < s1 for 64 channels; `merged`: the slots hold level-1 (hi, lo) results
template <bool COHERENT = false>                           // COHERENT: the slots were written by OTHER workgroups of this launch (st_agent)
__device__ __forceinline__ PowerSums fold_slots(const float* partial, long s0, long s1, long step, bool merged,
                                                int rows_per_slot, long M, int C, int c, PowerSums* lds) {
    const int ty = threadIdx.x >> 6, cl = threadIdx.x & 63;
    PowerSums a{0.0, 0.0};
    auto rd = [&](long idx) { return COHERENT ? ld_agent(partial + idx) : partial[idx]; };
    long i_first = s0 + ty * step;
    if (c < C && merged) {
        // level-2 fold (bn_finalize): up to 32 dependent-free iterations of four loads each were issued one iteration at a time
        // (16 us for a kernel of C / 64 workgroups on the critical path conv -> statistics -> apply); four iterations' loads in
        // flight, added in the same order
        for (; i_first + 12 * step + 1 < s1; i_first += 16 * step) {
            float u[4], v[4], ul[4], vl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long i = i_first + 4 * step * q;
                u[q] = rd((i * 2 + 0) * C + c);
                v[q] = rd((i * 2 + 1) * C + c);
                ul[q] = rd((i * 2 + 2) * C + c);
                vl[q] = rd((i * 2 + 3) * C + c);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a.s1 += (double)u[q];
                a.s2 += (double)v[q];
                a.s1 += (double)ul[q];
                a.s2 += (double)vl[q];
            }
        }
    }
    if (c < C)
        for (long i = i_first; i < s1; i += 4 * step) {
            const double u = (double)rd((i * 2 + 0) * C + c), v = (double)rd((i * 2 + 1) * C + c);
            if (merged && i + 1 < s1) {                     // (hi, lo) pairs in the group's first two slots
                a.s1 += u;
                a.s2 += v;
                a.s1 += (double)rd((i * 2 + 2) * C + c);
                a.s2 += (double)rd((i * 2 + 3) * C + c);
            } else {                                        // a raw slot: level 1, or a last group of ONE slot, which level 1 leaves as it is
                                                            // (it has no second slot for the low parts; S2 as one float costs the variance
                                                            // 2^-24 mean^2 / var of that slot's weight: 2e-4 at |mean| = 1e3 std)
                long n = M - i * rows_per_slot;
                n = n < 0 ? 0 : (n > rows_per_slot ? rows_per_slot : n);
                a.s1 += (double)n * u;
                a.s2 += v + (double)n * u * u;
            }
        }
    lds[ty * 64 + cl] = a;
    __syncthreads();
    PowerSums r = lds[cl];
    if (ty == 0)
        for (int t = 1; t < 4; ++t) {
            r.s1 += lds[t * 64 + cl].s1;
            r.s2 += lds[t * 64 + cl].s2;
        }
    return r;                                               // valid on ty == 0
}

__global__ __launch_bounds__(256) void bn_stats_merge_kernel(float* __restrict__ partial, long n_slots, long slots_per_group,
                                                             int rows_per_slot, long M, int C) {
    __shared__ PowerSums lds[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const long s0 = (long)blockIdx.y * slots_per_group;
    long s1 = s0 + slots_per_group;
    if (s1 > n_slots) s1 = n_slots;
    const PowerSums r = fold_slots(partial, s0, s1, 1, false, rows_per_slot, M, C, c, lds);
    if ((threadIdx.x >> 6) == 0 && c < C && s0 + 1 < s1) {  // every read of this block's slots happened before the barrier
        const float h1 = (float)r.s1, h2 = (float)r.s2;     // (a group of one slot stays raw: see fold_slots)
        partial[(s0 * 2 + 0) * C + c] = h1;
        partial[(s0 * 2 + 1) * C + c] = h2;
        partial[(s0 * 2 + 2) * C + c] = (float)(r.s1 - (double)h1);
        partial[(s0 * 2 + 3) * C + c] = (float)(r.s2 - (double)h2);
    }
}

// "Last workgroup done" hand-over (used by the fused merge + finalize kernels below): every workgroup of a channel group publishes
// its result (device-scope release fence), then takes a ticket from sync[group]; the one that draws the last ticket acquires and
// runs the group's final step alone, in a fixed order -> deterministic, and one launch instead of two.  sync[] holds zeros between
// launches (the finishing workgroup resets its counter); the caller owns it and never shares it between concurrent launches.
// The results handed over travel through st_agent / ld_agent: device-coherent accesses (sc1: written through / read past this XCD's
// L2).  NOT __threadfence(): on gfx950 an agent-scope release / acquire fence writes back and invalidates the XCD's whole L2
// (buffer_wbl2 / buffer_inv), per workgroup -- measured: the step 165 -> 225 ms, mostly in the OTHER stream's kernels.
// The ordering this relies on (sc1 write-through stores performed at vmcnt(0), then a relaxed agent-scope ticket) is what gfx942 /
// gfx950 hardware does, NOT a guarantee of the HIP memory model: the path is opt-in (py_bn_fused, default off), and the host side
// zeroes a module's counters whenever one of the fused entry points returns an error (nnf._check_fused_bn).

__device__ __forceinline__ bool last_workgroup_of(int* sync, int group, unsigned total) {
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's coherent stores have been performed
    __syncthreads();                                        // ... and every wave's of the workgroup
    if (threadIdx.x == 0) {
        const unsigned t = (unsigned)__hip_atomic_fetch_add(sync + group, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == total - 1);
        if (s_last) __hip_atomic_store(sync + group, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    __syncthreads();
    return s_last != 0;
}

__device__ __forceinline__ void bn_finalize_channel(const PowerSums& r, long M, int c, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ run_mean, float* __restrict__ run_var,
                                                    float momentum, float eps, float* __restrict__ scale, float* __restrict__ shift,
                                                    float* __restrict__ save_mean, float* __restrict__ save_invstd) {
    const double mean = r.s1 / (double)M;
    double m2 = r.s2 - (double)M * mean * mean;
    if (m2 < 0.0) m2 = 0.0;
    const double var = m2 / (double)M;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - (float)mean * sc;
    save_mean[c] = (float)mean;
    save_invstd[c] = invstd;
    if (run_mean) {
        const double unbiased = M > 1 ? m2 / (double)(M - 1) : var;
        run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * (float)mean;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (float)unbiased;
    }
}

// bn_stats_merge_kernel + bn_finalize_kernel in ONE launch: grid (64-channel groups, slot groups); the last workgroup of a channel
// group folds the group results (same order, same arithmetic as bn_finalize_kernel: bit-identical statistics).
__global__ __launch_bounds__(256) void bn_stats_merge_finalize_kernel(float* partial, long n_slots, long slots_per_group, int rows_per_slot,
                                                                      long M, int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float* __restrict__ run_mean, float* __restrict__ run_var, float momentum,
                                                                      float eps, float* __restrict__ scale, float* __restrict__ shift,
                                                                      float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                      long long* __restrict__ num_batches_tracked, int* sync) {
    __shared__ PowerSums lds[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const long s0 = (long)blockIdx.y * slots_per_group;
    long s1 = s0 + slots_per_group;
    if (s1 > n_slots) s1 = n_slots;
    const PowerSums r = fold_slots(partial, s0, s1, 1, false, rows_per_slot, M, C, c, lds);
    if ((threadIdx.x >> 6) == 0 && c < C && s0 + 1 < s1) {
        const float h1 = (float)r.s1, h2 = (float)r.s2;
        st_agent(partial + (s0 * 2 + 0) * C + c, h1);
        st_agent(partial + (s0 * 2 + 1) * C + c, h2);
        st_agent(partial + (s0 * 2 + 2) * C + c, (float)(r.s1 - (double)h1));
        st_agent(partial + (s0 * 2 + 3) * C + c, (float)(r.s2 - (double)h2));
    }
    if (!last_workgroup_of(sync, blockIdx.x, gridDim.y)) return;
    if (num_batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;   // nn.BatchNorm2d bookkeeping
    __syncthreads();                                        // lds is reused
    const PowerSums t = fold_slots<true>(partial, 0, n_slots, slots_per_group, true, rows_per_slot, M, C, c, lds);
    if ((threadIdx.x >> 6) == 0 && c < C)
        bn_finalize_channel(t, M, c, gamma, beta, run_mean, run_var, momentum, eps, scale, shift, save_mean, save_invstd);
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, long n_slots, long slots_per_group,
                                                          int rows_per_slot, long M, int C, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ run_mean,
                                                          float* __restrict__ run_var, float momentum, float eps,
                                                          float* __restrict__ scale, float* __restrict__ shift,
                                                          float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                          long long* __restrict__ num_batches_tracked) {
    __shared__ PowerSums lds[256];
    if (num_batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;   // nn.BatchNorm2d bookkeeping
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const PowerSums r = fold_slots(partial, 0, n_slots, slots_per_group, slots_per_group > 1, rows_per_slot, M, C, c, lds);
    if ((threadIdx.x >> 6) == 0 && c < C)
        bn_finalize_channel(r, M, c, gamma, beta, run_mean, run_var, momentum, eps, scale, shift, save_mean, save_invstd);
}

// eval mode: scale/shift from the running statistics
__global__ __launch_bounds__(256) void bn_eval_coeffs_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ run_mean, const float* __restrict__ run_var,
                                                             float eps, float* __restrict__ scale, float* __restrict__ shift,
                                                             float* __restrict__ save_mean, float* __restrict__ save_invstd) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float invstd = 1.0f / sqrtf(run_var[c] + eps);
    const float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - run_mean[c] * sc;
    save_mean[c] = run_mean[c];
    save_invstd[c] = invstd;
}

// (stored value > 0) of V values as a bit field: the test runs on the value ROUNDED to T, i.e. on what `out > 0` reads back later
template <typename T, int V>
__device__ inline unsigned char relu_bits(const float (&v)[V]) {
    unsigned b = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) b |= ((float)(T)v[e] > 0.0f ? 1u : 0u) << e;
    return (unsigned char)b;
}

// out = [relu]( y * scale[c] + shift[c] [+ res] )      (16 bytes per thread when C allows, else scalar)
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const T* __restrict__ res,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       long M, int C, int relu, T* __restrict__ out,
                                                       unsigned char* __restrict__ bits = nullptr) {
    // bits (nullable; 8-element vectors only, i.e. bf16 with C % 8 == 0): bit e of bits[i / 8] = (out[i + e] > 0), the ReLU mask
    // the backward of a residual layer reads instead of `out` (1/16 of its bytes)
    constexpr int V = VecN<T>::N;
    const long total = M * C;
    if (C % V == 0 && (256 * V) % C == 0) {
        // the per-thread channel offset is invariant under the grid stride: keep scale/shift in registers
        const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
        const int c = (int)(i0 % C);
        float sc[V], sh[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            sc[e] = scale[c + e];
            sh[e] = shift[c + e];
        }
#pragma unroll BN_UNROLL
        for (long i = i0; i < total; i += (long)gridDim.x * 256 * V) {
            float v[V], r[V];
            ldv(y, i, v);
            if (res) ldv(res, i, r);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float t = __builtin_fmaf(v[e], sc[e], sh[e]);
                if (res) t += r[e];
                v[e] = (relu && !(t > 0.0f)) ? 0.0f : t;
            }
            stv(out, i, v);
            if (V == 8 && bits) bits[i >> 3] = relu_bits<T, V>(v);
        }
    } else if (C % V == 0) {
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (long)gridDim.x * 256 * V) {
            const int c = (int)(i % C);
            float v[V], r[V];
            ldv(y, i, v);
            if (res) ldv(res, i, r);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float t = __builtin_fmaf(v[e], scale[c + e], shift[c + e]);
                if (res) t += r[e];
                v[e] = (relu && !(t > 0.0f)) ? 0.0f : t;
            }
            stv(out, i, v);
            if (V == 8 && bits) bits[i >> 3] = relu_bits<T, V>(v);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int c = (int)(i % C);
            float t = ld(y, i) * scale[c] + shift[c];
            if (res) t += ld(res, i);
            st(out, i, (relu && !(t > 0.0f)) ? 0.0f : t);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// BatchNorm backward (through the fused ReLU / residual):  gz = g_out * (out > 0)
//   partial[blk][0][c] = sum gz,   partial[blk][1][c] = sum gz * xhat,   xhat = (y - mean) * invstd
// ---------------------------------------------------------------------------------------------
constexpr int BNB_ROWS_MIN = 256;  // rows per block of the reduce kernel (more for tall tensors: at most ~512 row blocks)
constexpr int BNB_CG = 64;         // channels per block

// grid (row chunks, channel groups).  Each thread owns V consecutive channels (one 16-byte load) of every
// (256 / threads-per-row)-th row of the chunk; row lanes are folded through LDS in a fixed order.
// MASK: 0 no ReLU, 1 mask from `out`, 2 mask recomputed as fma(y, fsc, fsh) > 0 (the forward's expression; no residual),
//       3 mask from the forward's bit field (`out` then points at bytes: bit e of byte i/8 = out[i + e] > 0; 8-element vectors only)
// Finalize arguments of the fused reduce (sync != null): see bn_bwd_finalize_kernel
struct BnBwdFin {
    const float* gamma;
    int training, accumulate;
    float* dgamma;
    float* dbeta;
    float* coef;
    int* sync;                                             // [channel groups], zeros between launches; null: separate finalize launch
};

template <typename T, int MASK>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ g_out, const T* __restrict__ out,
                                                            const T* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ fsc,
                                                            const float* __restrict__ fsh, long M, int C, int relu,
                                                            float* partial, int rows_per_block, const BnBwdFin fin, T* __restrict__ gz_out = nullptr) {
    constexpr int V = VecN<T>::N;
    __shared__ float sh[2][256 * V];                       // [sum kind][row lane][channel in group]
    const int cg = C < BNB_CG ? C : BNB_CG;                // channels handled by this block
    const int c0 = blockIdx.y * BNB_CG;
    const int BNB_ROWS = rows_per_block;
    const long row0 = (long)blockIdx.x * BNB_ROWS;
    float s0[V], s1[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s0[e] = s1[e] = 0.0f;
    int tpr, lanes, rl = 0, cv = 0;
    if (C % V == 0) {
        tpr = cg / V;                                      // threads per row
        lanes = 256 / tpr;
        rl = threadIdx.x / tpr;
        cv = (threadIdx.x % tpr) * V;
        if (rl < lanes && c0 + cv < C) {
            float mu[V], is[V], sc[V], sf[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                mu[e] = mean[c0 + cv + e];
                is[e] = invstd[c0 + cv + e];
                sc[e] = MASK == 2 ? fsc[c0 + cv + e] : 0.0f;
                sf[e] = MASK == 2 ? fsh[c0 + cv + e] : 0.0f;
            }
#pragma unroll BN_UNROLL
            for (int rr = rl; rr < BNB_ROWS; rr += lanes) {
                const long m = row0 + rr;
                if (m >= M) break;
                float g[V], o[V], yy[V];
                ldv(g_out, m * C + c0 + cv, g);
                ldv(y, m * C + c0 + cv, yy);
                if (MASK == 1) ldv(out, m * C + c0 + cv, o);
                if (MASK == 3) {
                    const unsigned mb = reinterpret_cast<const unsigned char*>(out)[(m * C + c0 + cv) >> 3];
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = (mb >> (e & 7)) & 1u ? 1.0f : 0.0f;
                }
                if (MASK == 2) {
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = __builtin_fmaf(yy[e], sc[e], sf[e]);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float gz = (MASK != 0 && !(o[e] > 0.0f)) ? 0.0f : g[e];
                    s0[e] += gz;
                    s1[e] = __builtin_fmaf(gz, (yy[e] - mu[e]) * is[e], s1[e]);
                    g[e] = gz;
                }
                // r4 (residual layers, MASK == 1): the masked gradient IS the residual branch's gradient -- written here, the apply pass
                // then reads it instead of (g_out, out): one tensor read less per backward of a residual layer
                if ((MASK == 1 || MASK == 3) && gz_out) stv(gz_out, m * C + c0 + cv, g);
            }
        }
    } else {                                               // scalar fallback (odd channel counts): one channel per thread
        tpr = cg;
        lanes = 256 / tpr;
        rl = threadIdx.x / tpr;
        cv = threadIdx.x % tpr;
        if (rl < lanes && c0 + cv < C) {
            const float mu = mean[c0 + cv], is = invstd[c0 + cv];
            for (int rr = rl; rr < BNB_ROWS; rr += lanes) {
                const long m = row0 + rr;
                if (m >= M) break;
                float gz = ld(g_out, m * C + c0 + cv);
                const float yv = ld(y, m * C + c0 + cv);
                if (MASK != 0 && !((MASK == 1 ? ld(out, m * C + c0 + cv) : yv * fsc[c0 + cv] + fsh[c0 + cv]) > 0.0f)) gz = 0.0f;
                if (MASK == 1 && gz_out) st(gz_out, m * C + c0 + cv, gz);
                s0[0] += gz;
                s1[0] = __builtin_fmaf(gz, (yv - mu) * is, s1[0]);
            }
        }
    }
    const int vv = (C % V == 0) ? V : 1;
    if (rl < lanes) {
        for (int e = 0; e < vv; ++e) {
            sh[0][rl * cg + cv + e] = s0[e];
            sh[1][rl * cg + cv + e] = s1[e];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < cg && c0 + (int)threadIdx.x < C) {
        float a = 0.0f, b = 0.0f;
        for (int l = 0; l < lanes; ++l) {
            a += sh[0][l * cg + threadIdx.x];
            b += sh[1][l * cg + threadIdx.x];
        }
        if (fin.sync) {
            st_agent(partial + ((long)blockIdx.x * 2 + 0) * C + c0 + threadIdx.x, a);
            st_agent(partial + ((long)blockIdx.x * 2 + 1) * C + c0 + threadIdx.x, b);
        } else {
            partial[((long)blockIdx.x * 2 + 0) * C + c0 + threadIdx.x] = a;
            partial[((long)blockIdx.x * 2 + 1) * C + c0 + threadIdx.x] = b;
        }
    }
    if (!fin.sync) return;
    // ---- fused finalize (was bn_bwd_finalize_kernel, a second launch): the last workgroup of this channel group sums the row
    // blocks' partials in block order (4 row lanes x 64 channels, coalesced along the channels, lanes folded in lane order:
    // fixed order -> deterministic) and writes dgamma / dbeta / the apply pass's coefficients for its channels.
    if (!last_workgroup_of(fin.sync, blockIdx.y, gridDim.x)) return;
    __shared__ double fr[2][256];
    const int cl = threadIdx.x & 63, ty = threadIdx.x >> 6, c = c0 + cl;
    double a = 0.0, b = 0.0;
    if (c < C && cl < cg) {
        // eight row blocks' partials in flight at a time (device-coherent loads are not batched by the compiler), added in block order
        const long nbk = (long)gridDim.x;
        for (long i0 = ty; i0 < nbk; i0 += 32) {
            float va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = i0 + 4 * u;
                va[u] = i < nbk ? ld_agent(partial + (i * 2 + 0) * C + c) : 0.0f;
                vb[u] = i < nbk ? ld_agent(partial + (i * 2 + 1) * C + c) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a += (double)va[u];
                b += (double)vb[u];
            }
        }
    }
    fr[0][threadIdx.x] = a;
    fr[1][threadIdx.x] = b;
    __syncthreads();
    if (ty == 0 && c < C && cl < cg) {
        for (int t = 1; t < 4; ++t) {
            a += fr[0][t * 64 + cl];
            b += fr[1][t * 64 + cl];
        }
        fin.dbeta[c] = fin.accumulate ? fin.dbeta[c] + (float)a : (float)a;
        fin.dgamma[c] = fin.accumulate ? fin.dgamma[c] + (float)b : (float)b;
        fin.coef[0 * C + c] = fin.gamma[c] * invstd[c];
        fin.coef[1 * C + c] = fin.training ? (float)(a / (double)M) : 0.0f;
        fin.coef[2 * C + c] = fin.training ? (float)(b / (double)M) : 0.0f;
    }
}

// dgamma = sum gz*xhat, dbeta = sum gz; coefficients of the apply pass:
//   train: g_y = k0[c] * (gz - k1[c] - xhat * k2[c]),  k0 = gamma*invstd, k1 = mean(gz), k2 = mean(gz*xhat)
//   eval : g_y = k0[c] * gz
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, long n_blocks, long M, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                              int training, int accumulate, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x;
    __shared__ double r0[256], r1[256];
    double a = 0.0, b = 0.0;
    long i = threadIdx.x;
    for (; i + 768 < n_blocks; i += 1024) {                // four row blocks' partials in flight (latency bound), same order of adds
        float va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            va[u] = partial[((i + 256 * u) * 2 + 0) * C + c];
            vb[u] = partial[((i + 256 * u) * 2 + 1) * C + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a += (double)va[u];
            b += (double)vb[u];
        }
    }
    for (; i < n_blocks; i += 256) {
        a += (double)partial[(i * 2 + 0) * C + c];
        b += (double)partial[(i * 2 + 1) * C + c];
    }
    r0[threadIdx.x] = a;
    r1[threadIdx.x] = b;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) {
            r0[threadIdx.x] += r0[threadIdx.x + m];
            r1[threadIdx.x] += r1[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        dbeta[c] = accumulate ? dbeta[c] + (float)r0[0] : (float)r0[0];
        dgamma[c] = accumulate ? dgamma[c] + (float)r1[0] : (float)r1[0];
        coef[0 * C + c] = gamma[c] * invstd[c];
        coef[1 * C + c] = training ? (float)(r0[0] / (double)M) : 0.0f;
        coef[2 * C + c] = training ? (float)(r1[0] / (double)M) : 0.0f;
    }
}

template <typename T, int MASK>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ g_out, const T* __restrict__ out,
                                                           const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ coef,
                                                           const float* __restrict__ fsc, const float* __restrict__ fsh,
                                                           long M, int C, int relu, T* __restrict__ g_y, T* __restrict__ g_res) {
    constexpr int V = VecN<T>::N;
    const long total = M * C;
    if (C % V == 0 && (256 * V) % C == 0) {
        const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
        const int c = (int)(i0 % C);
        float mu[V], is[V], k0[V], k1[V], k2[V], sc[V], sf[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            mu[e] = mean[c + e];
            is[e] = invstd[c + e];
            k0[e] = coef[c + e];
            k1[e] = coef[C + c + e];
            k2[e] = coef[2 * C + c + e];
            sc[e] = MASK == 2 ? fsc[c + e] : 0.0f;
            sf[e] = MASK == 2 ? fsh[c + e] : 0.0f;
        }
#pragma unroll BN_UNROLL
        for (long i = i0; i < total; i += (long)gridDim.x * 256 * V) {
            float g[V], o[V], yy[V], r[V];
            ldv(g_out, i, g);
            ldv(y, i, yy);
            if (MASK == 1) ldv(out, i, o);
            if (MASK == 2) {
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = __builtin_fmaf(yy[e], sc[e], sf[e]);
            }
            if (MASK == 3) {                                // the forward's bit field (see bn_bwd_reduce_kernel)
                const unsigned mb = reinterpret_cast<const unsigned char*>(out)[i >> 3];
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = (mb >> (e & 7)) & 1u ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float gz = (MASK != 0 && !(o[e] > 0.0f)) ? 0.0f : g[e];
                const float xh = (yy[e] - mu[e]) * is[e];
                r[e] = gz;
                g[e] = k0[e] * (gz - k1[e] - xh * k2[e]);
            }
            stv(g_y, i, g);
            if (g_res) stv(g_res, i, r);
        }
    } else if (C % V == 0) {
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (long)gridDim.x * 256 * V) {
            const int c = (int)(i % C);
            float g[V], o[V], yy[V], r[V];
            ldv(g_out, i, g);
            ldv(y, i, yy);
            if (MASK == 1) ldv(out, i, o);
            if (MASK == 2) {
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = __builtin_fmaf(yy[e], fsc[c + e], fsh[c + e]);
            }
            if (MASK == 3) {
                const unsigned mb = reinterpret_cast<const unsigned char*>(out)[i >> 3];
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = (mb >> (e & 7)) & 1u ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float gz = (MASK != 0 && !(o[e] > 0.0f)) ? 0.0f : g[e];
                const float xh = (yy[e] - mean[c + e]) * invstd[c + e];
                r[e] = gz;
                g[e] = coef[c + e] * (gz - coef[C + c + e] - xh * coef[2 * C + c + e]);
            }
            stv(g_y, i, g);
            if (g_res) stv(g_res, i, r);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int c = (int)(i % C);
            float g = ld(g_out, i);
            const float yv = ld(y, i);
            if (MASK != 0 && !((MASK == 1 ? ld(out, i) : yv * fsc[c] + fsh[c]) > 0.0f)) g = 0.0f;
            const float xh = (yv - mean[c]) * invstd[c];
            st(g_y, i, coef[c] * (g - coef[C + c] - xh * coef[2 * C + c]));
            if (g_res) st(g_res, i, g);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_bn_finalize(float* partial, long n_slots, int rows_per_slot, long M, int C, const float* gamma,
                              const float* beta, float* run_mean, float* run_var, float momentum, float eps, float* scale,
                              float* shift, float* save_mean, float* save_invstd, long long* num_batches_tracked, int* sync,
                              hipStream_t st_) {
    long spg = 1;                                           // slots per group of level 1
    if (g_nn_opt.debug_skip_small & 1) return hipSuccess;
    if (n_slots > 128) {
        spg = (n_slots + 127) / 128;
        if (spg < 16) spg = 16;
        const long groups = (n_slots + spg - 1) / spg;
        if (sync && groups > 1) {                           // one launch: the last workgroup of every channel group finalizes
            hipLaunchKernelGGL(bn_stats_merge_finalize_kernel, dim3((C + 63) / 64, (unsigned)groups), dim3(256), 0, st_, partial, n_slots, spg,
                               rows_per_slot, M, C, gamma, beta, run_mean, run_var, momentum, eps, scale, shift, save_mean, save_invstd,
                               num_batches_tracked, sync);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(bn_stats_merge_kernel, dim3((C + 63) / 64, (unsigned)groups), dim3(256), 0, st_, partial, n_slots, spg,
                           rows_per_slot, M, C);
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(256), 0, st_, partial, n_slots, spg, rows_per_slot, M, C, gamma,
                       beta, run_mean, run_var, momentum, eps, scale, shift, save_mean, save_invstd, num_batches_tracked);
    return hipGetLastError();
}

hipError_t launch_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* run_mean, const float* run_var,
                                 float eps, float* scale, float* shift, float* save_mean, float* save_invstd, hipStream_t st_) {
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((C + 255) / 256), dim3(256), 0, st_, C, gamma, beta, run_mean, run_var, eps,
                       scale, shift, save_mean, save_invstd);
    return hipGetLastError();
}

template <typename T>
static hipError_t bn_apply_t(const void* y, const void* res, const float* scale, const float* shift, long M, int C, int relu,
                             void* out, hipStream_t st_, unsigned char* bits) {
    if (bits && (VecN<T>::N != 8 || C % 8 != 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(M * C / (C % VecN<T>::N ? 1 : VecN<T>::N))), dim3(256), 0, st_, (const T*)y,
                       (const T*)res, scale, shift, M, C, relu, (T*)out, bits);
    return hipGetLastError();
}
hipError_t launch_bn_apply(int bf16, const void* y, const void* res, const float* scale, const float* shift, long M, int C,
                           int relu, void* out, hipStream_t st_, unsigned char* bits) {
    return bf16 ? bn_apply_t<__bf16>(y, res, scale, shift, M, C, relu, out, st_, bits)
                : bn_apply_t<float>(y, res, scale, shift, M, C, relu, out, st_, bits);
}

long bn_bwd_blocks(long M) { return (M + BNB_ROWS_MIN - 1) / BNB_ROWS_MIN; }       // upper bound (workspace sizing)
// rows per workgroup of the reduce: 256, more for tall tensors so that the final sum over the row blocks (done by ONE workgroup per
// channel group when the finalize is fused) stays short -- at most 512 row blocks
static int bn_bwd_rows_per_block(long M) {
    long r = BNB_ROWS_MIN;
    while ((M + r - 1) / r > 512) r *= 2;
    return (int)r;
}

template <typename T, int MASK>
static hipError_t bn_bwd_t(const void* g_out, const void* out, const void* y, const float* mean, const float* invstd,
                           const float* gamma, const float* fsc, const float* fsh, long M, int C, int relu, int training,
                           int accumulate, float* partial, float* coef,
                           float* dgamma, float* dbeta, void* g_y, void* g_res, int* sync, hipStream_t st_) {
    const int rpb = sync ? bn_bwd_rows_per_block(M) : BNB_ROWS_MIN;
    const long nb = (M + rpb - 1) / rpb;
    const BnBwdFin fin{gamma, training, accumulate, dgamma, dbeta, coef, (g_nn_opt.debug_skip_small & 2) ? nullptr : sync};
    // residual layers (MASK == 1 with a g_res output): the reduce pass writes the masked gradient = g_res, the apply pass runs unmasked on it
    // bit-field form (MASK == 3): with a g_res output as above; without one (the residual branch's consumer masks g_out with the
    // bits itself, vqseg_conv2d_affine_bits_f) both passes read (g_out, bits) and no masked gradient is written at all
    const bool premask = (MASK == 1 || MASK == 3) && g_res != nullptr && (g_nn_opt.bn_bwd_premask || MASK == 3);
    if (MASK == 3 && (C % VecN<T>::N != 0 || VecN<T>::N != 8)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MASK>), dim3((unsigned)nb, (unsigned)((C + BNB_CG - 1) / BNB_CG)), dim3(256), 0, st_,
                       (const T*)g_out, (const T*)out, (const T*)y, mean, invstd, fsc, fsh, M, C, relu, partial, rpb, fin,
                       premask ? (T*)g_res : (T*)nullptr);
    if (!(g_nn_opt.debug_skip_small & 2) && !sync)
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, st_, partial, nb, M, C, gamma, invstd, training, accumulate, dgamma,
                       dbeta, coef);
    if (premask)
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, 0>), dim3(grid_for(M * C / (C % VecN<T>::N ? 1 : VecN<T>::N))), dim3(256), 0, st_,
                           (const T*)g_res, (const T*)nullptr, (const T*)y, mean, invstd, coef, fsc, fsh, M, C, 0, (T*)g_y, (T*)nullptr);
    else
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, MASK>), dim3(grid_for(M * C / (C % VecN<T>::N ? 1 : VecN<T>::N))), dim3(256), 0, st_,
                       (const T*)g_out, (const T*)out, (const T*)y, mean, invstd, coef, fsc, fsh, M, C, relu, (T*)g_y, (T*)g_res);
    return hipGetLastError();
}
hipError_t launch_bn_backward(int bf16, const void* g_out, const void* out, const void* y, const float* mean,
                              const float* invstd, const float* gamma, const float* fsc, const float* fsh, long M, int C, int relu,
                              int training, int accumulate, float* partial,
                              float* coef, float* dgamma, float* dbeta, void* g_y, void* g_res, int* sync, hipStream_t st_,
                              const unsigned char* bits) {
    const int mask = !relu ? 0 : (bits ? 3 : out ? 1 : 2);
    if (mask == 3) out = bits;
#define BN_BWD_CASE(T_, MASK_)                                                                                                   \
    if (mask == MASK_)                                                                                                            \
        return bn_bwd_t<T_, MASK_>(g_out, out, y, mean, invstd, gamma, fsc, fsh, M, C, relu, training, accumulate, partial, coef, dgamma, dbeta, \
                                   g_y, g_res, sync, st_);
    if (bf16) {
        BN_BWD_CASE(__bf16, 0) BN_BWD_CASE(__bf16, 1) BN_BWD_CASE(__bf16, 2) BN_BWD_CASE(__bf16, 3)
    } else {
        BN_BWD_CASE(float, 0) BN_BWD_CASE(float, 1) BN_BWD_CASE(float, 2)
    }
#undef BN_BWD_CASE
    return hipErrorInvalidValue;
}

}  // namespace vqseg
