// Device helpers shared by more than one convolution unit (conv_igemm / conv_patch / conv_wgrad / conv_pack): bf16 packing, the
// K-loop barrier, row / padding index arithmetic, the A-operand source selection, the LDS-DMA load with its zero page, and the
// epilogue of the forward kernels.  Everything here is __device__ __forceinline__ (or a type): a unit pays only for what it uses.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_kernels.h"

namespace vqseg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned int pack2(float a, float b) {
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (unsigned int)__builtin_bit_cast(unsigned short, x) | ((unsigned int)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ void unpack8(const u32x4 a, float (&v)[8]) {      // 8 bf16 -> fp32
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = __builtin_bit_cast(float, a[e] << 16);
        v[2 * e + 1] = __builtin_bit_cast(float, a[e] & 0xFFFF0000u);
    }
}
__device__ __forceinline__ float bf16_round(float a) { return (float)((__bf16)a); }

// Raw workgroup barrier of the software-pipelined K loops.  __builtin_amdgcn_s_barrier() alone is no memory barrier: the
// compiler may move LDS reads of the stage just computed past it, and a wave's ds_reads may still be pending there -- while
// another wave, released by the barrier, already DMAs the next stage into that same buffer (run-to-run differences).
// The "memory" clobbers pin every load and store to its side of the barrier, lgkmcnt(0) retires this wave's LDS reads first;
// vmcnt is left alone (the DMA of later stages stays in flight).
__device__ __forceinline__ void stage_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// pixel row m -> (image n, offset inside the image): 32-bit division whenever the row count allows (a 64-bit
// division is ~100 emulated instructions, which matters in layers whose whole K loop is one or two stages)
__device__ __forceinline__ void split_row(long m, int hw, long M, int& n, int& rem) {
    if (M <= 0x7fffffffL) {
        const unsigned int um = (unsigned int)m;
        n = (int)(um / (unsigned int)hw);
        rem = (int)(um - (unsigned int)n * (unsigned int)hw);
    } else {
        n = (int)(m / hw);
        rem = (int)(m - (long)n * hw);
    }
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// Which source tensor holds contraction channels [ci, ci + chunk): the concat fusion ([0, C1) -> x, [C1, Cin) -> x2), and for
// split-3 INPUTS (p.s3_in) the fold of the logical [hi | lo | hi] segment (3 Cs channels) onto its stored [hi | lo] rows (2 Cs
// channels per pixel): the third part re-reads hi (from L2 -- the bytes were fetched a few stages ago).
struct ASource {
    const char* src;
    int csrc, cbase;                                        // channels per pixel row of the source, channel offset inside the row
};
__device__ __forceinline__ ASource a_source(const ConvArgs& p, int ci) {
    const bool second = ci >= p.C1;
    ASource a;
    a.src = reinterpret_cast<const char*>(second ? p.x2 : p.x);
    a.csrc = second ? (p.Cin - p.C1) : p.C1;
    a.cbase = second ? (ci - p.C1) : ci;
    if (p.s3_in) {
        const int cs2 = 2 * (second ? p.s3_cs2 : p.s3_cs1);
        a.csrc = cs2;
        if (a.cbase >= cs2) a.cbase -= cs2;
    }
    return a;
}

// Strided output placement (p.omap): GEMM row m = (n, oh, ow) of the Ho x Wo problem lands on pixel (n, 2 oh + ph, 2 ow + pw) of
// an OH x OW grid -- the parity classes of a stride-2 data gradient (launch_dgrad_s2).  Two 32-bit divisions per written row.
__device__ __forceinline__ long out_row(const ConvArgs& p, long m) {
    if (!p.omap) return m;
    const unsigned hw = (unsigned)(p.Ho * p.Wo), um = (unsigned)m;
    const unsigned n = um / hw, rem = um - n * hw;
    const unsigned oh = rem / (unsigned)p.Wo, ow = rem - oh * (unsigned)p.Wo;
    if (p.omap_fold) {                                       // (i, j) on the padded grid -> the unpadded gradient / ring / dump row
        const int i = 2 * (int)oh + p.omap_ph, j = 2 * (int)ow + p.omap_pw, H = p.omap_h, W = p.omap_w;
        const long body = (long)p.N * H * W;
        if (i >= 1 && j >= 1 && i <= H && j <= W) return ((long)n * H + i - 1) * W + j - 1;
        if (p.omap_fold == 1) {
            const int rl = W + 1 + H;
            if (i == 0 && j <= W) return body + (long)n * rl + j;
            if (j == 0 && i <= H) return body + (long)n * rl + W + i;          // i >= 1 here
            return body + (long)p.N * rl;
        }
        return body;
    }
    return ((long)n * p.omap_h + 2 * oh + p.omap_ph) * p.omap_w + 2 * ow + p.omap_pw;
}

#ifndef GLDS_ABL                  // (here and not at conv_igemm_glds_kernel, which it ablates: bits 1 and 4 are read by the epilogue below)
#define GLDS_ABL 0                // debug builds only (results wrong): 1 no y stores, 2 no epilogue, 4 no BN partials, 8 no A-tile DMA
#endif
// ---- shared epilogue: per-wave BN partials from the accumulators, then Y through LDS as 16-byte row segments
struct LinearRows {                                          // tile row -> output pixel row (NHWC-flattened)
    long m0;
    __device__ __forceinline__ long operator()(int row) const { return m0 + row; }
};

// FAST: compile the whole-tile fast paths (the register-staged conv_igemm_kernel opts out: they cost it 24 VGPRs = half its occupancy)
template <int TBM, int BN, bool PRECISE, int MT, int NTT, int NT, int NTHR, typename RowMap = LinearRows, bool S3 = false, bool FAST = true>
__device__ __forceinline__ void conv_epilogue(f32x16 (&acc)[MT][NTT], const ConvArgs& p, char* smem, long M, long m0, int co0,
                                              int wm, int wn, int r, int h, int tid, RowMap row_to_m = LinearRows{-1}) {
    if constexpr (__is_same(RowMap, LinearRows)) row_to_m.m0 = m0;
    const long wrow0 = m0 + (long)wm * MT * 32;
    if constexpr (S3) {
        // split-3 output: the fp32 result v = acc * scale + shift (+ residual, ReLU) leaves as [hi | lo] bf16, hi = bf16(v),
        // lo = bf16(v - hi): 2 * Cout channels per pixel row (the consumer's K loop reads hi twice: a_source).  Staged through LDS as two bf16 tiles so that the stores (and the
        // residual loads) are whole 16-byte row segments.  Host side guarantees Cout % 8 == 0 and a fused epilogue.
        static_assert(!PRECISE, "split-3 output belongs to the bf16 kernels");
        // (r4: a tile whose two staging tiles do not fit LDS -- the 256 x 256 tile: 270 KB -- leaves in two column halves)
        constexpr int HALVES = ((size_t)TBM * (BN + 8) * 4 > 160u * 1024u) ? 2 : 1;
        constexpr int BNH = BN / HALVES, OS = BNH + 8;
        __bf16* th = reinterpret_cast<__bf16*>(smem);
        __bf16* tl = th + TBM * OS;
        const bool ep_res = p.ep_res != nullptr;
        constexpr int CPR = BNH / 8;
        const long rs = 2L * p.Cout;                         // output (and residual) row stride in elements: [hi | lo]
#pragma unroll
        for (int hf = 0; hf < HALVES; ++hf) {
            if (hf) __syncthreads();                         // the previous half has been read out of LDS
#pragma unroll
            for (int b = 0; b < NTT; ++b) {
                const int col = (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
                if (HALVES > 1 && ((BN >= 64 ? (wn * NT + b) * 32 : 0) / BNH) != hf) continue;      // wave-uniform
                const int lc = col - hf * BNH;
                const bool cok = co0 + col < p.Cout;
                const float esc = cok ? p.ep_scale[co0 + col] : 1.0f, esh = cok ? p.ep_shift[co0 + col] : 0.0f;
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = (wm * MT + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        float v = __builtin_fmaf(acc[a][b][i], esc, esh);
                        if (p.ep_relu && !ep_res && !(v > 0.0f)) v = 0.0f;
                        const __bf16 vh = (__bf16)v;
                        th[row * OS + lc] = vh;
                        tl[row * OS + lc] = (__bf16)(v - (float)vh);
                    }
            }
            __syncthreads();
            for (int idx = tid; idx < TBM * CPR; idx += NTHR) {
                const int row = idx / CPR, ch = idx % CPR;
                const long m = row_to_m(row);
                const int co = co0 + hf * BNH + ch * 8;
                if (m < M && co < p.Cout) {
                    u32x4 vh = *reinterpret_cast<const u32x4*>(th + (size_t)row * OS + ch * 8);
                    u32x4 vl = *reinterpret_cast<const u32x4*>(tl + (size_t)row * OS + ch * 8);
                    if (ep_res) {
                        const unsigned short* rp = reinterpret_cast<const unsigned short*>(p.ep_res) + m * rs + co;
                        const u32x4 rh = *reinterpret_cast<const u32x4*>(rp);
                        const u32x4 rl = *reinterpret_cast<const u32x4*>(rp + p.Cout);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v0 = (__builtin_bit_cast(float, vh[e] << 16) + __builtin_bit_cast(float, vl[e] << 16)) +
                                       (__builtin_bit_cast(float, rh[e] << 16) + __builtin_bit_cast(float, rl[e] << 16));
                            float v1 = (__builtin_bit_cast(float, vh[e] & 0xFFFF0000u) + __builtin_bit_cast(float, vl[e] & 0xFFFF0000u)) +
                                       (__builtin_bit_cast(float, rh[e] & 0xFFFF0000u) + __builtin_bit_cast(float, rl[e] & 0xFFFF0000u));
                            if (p.ep_relu && !(v0 > 0.0f)) v0 = 0.0f;
                            if (p.ep_relu && !(v1 > 0.0f)) v1 = 0.0f;
                            vh[e] = pack2(v0, v1);
                            vl[e] = pack2(v0 - bf16_round(v0), v1 - bf16_round(v1));
                        }
                    }
                    unsigned short* yp = reinterpret_cast<unsigned short*>(p.y) + m * rs + co;
                    *reinterpret_cast<u32x4*>(yp) = vh;
                    *reinterpret_cast<u32x4*>(yp + p.Cout) = vl;
                }
            }
        }
        return;
    }
    // Whole tile inside the output (always for the 2-D pixel tiles of the patch kernel; every tile but the last one otherwise): the
    // per-element row tests (a 64-bit compare + select each, twice per accumulator in the statistics, once per store) drop out.
    // These epilogues are VALU-issue bound on the short-K layers (see the LIN note at conv_igemm_glds_kernel).
    const bool full = FAST && (!__is_same(RowMap, LinearRows) || m0 + TBM <= M);          // workgroup-uniform
    if (p.stat_partial && !(GLDS_ABL & 4)) {
        // one (mean, M2) partial per SLOT of RPS consecutive rows: 64 rows (two 32-row tiles) or 32 when the wave has one
        constexpr int TPS = (MT >= 2 && BN >= 64) ? 2 : 1, RPS = TPS * 32;   // vqseg_conv_stat_slots: 64 rows per slot from 64 output channels on, else 32
#pragma unroll
        for (int b = 0; b < NTT; ++b) {
            const int co = co0 + (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
            const bool cok = co < p.Cout;
#pragma unroll
            for (int g = 0; g < MT / TPS; ++g) {
                const long srow0 = wrow0 + g * RPS;
                float sum = 0.0f, mean, m2 = 0.0f;
                if (full) {
#pragma unroll
                    for (int a = g * TPS; a < (g + 1) * TPS; ++a)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sum += acc[a][b][i];
                    sum += __shfl_xor(sum, 32);
                    mean = sum / (float)RPS;
#pragma unroll
                    for (int a = g * TPS; a < (g + 1) * TPS; ++a)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const float d = acc[a][b][i] - mean;
                            m2 = __builtin_fmaf(d, d, m2);
                        }
                } else {
#pragma unroll
                    for (int a = g * TPS; a < (g + 1) * TPS; ++a)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const long m = wrow0 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                            if (m < M) sum += acc[a][b][i];
                        }
                    long cnt_l = M - srow0;
                    const float cnt = (float)(cnt_l < 0 ? 0 : (cnt_l > RPS ? RPS : cnt_l));
                    sum += __shfl_xor(sum, 32);
                    mean = cnt > 0.f ? sum / cnt : 0.f;
#pragma unroll
                    for (int a = g * TPS; a < (g + 1) * TPS; ++a)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const long m = wrow0 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                            const float d = acc[a][b][i] - mean;
                            if (m < M) m2 = __builtin_fmaf(d, d, m2);
                        }
                }
                m2 += __shfl_xor(m2, 32);
                if (h == 0 && cok) {
                    const long slot = srow0 / RPS;                        // global slot index along M
                    p.stat_partial[(slot * 2 + 0) * p.Cout + co] = mean;
                    p.stat_partial[(slot * 2 + 1) * p.Cout + co] = m2;
                }
            }
        }
    }
    constexpr int O_EPC = PRECISE ? 4 : 8;                  // output elements per 16-byte store
    if (p.Cout % O_EPC == 0) {
        // the main loop's last barrier has passed: LDS is free.  Tile [BM][BN] of the output element type.
        constexpr int OS = BN + O_EPC;                      // row stride (elements) -- padded against bank conflicts
        char* ot = smem;
        const bool ep = p.ep_scale != nullptr, ep_res = ep && p.ep_res != nullptr;
#pragma unroll
        for (int b = 0; b < NTT; ++b) {
            const int col = (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
            const bool cok = co0 + col < p.Cout;
            const float esc = ep && cok ? p.ep_scale[co0 + col] : 1.0f, esh = ep && cok ? p.ep_shift[co0 + col] : 0.0f;
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (wm * MT + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    float v = acc[a][b][i];
                    if (ep) {
                        v = __builtin_fmaf(v, esc, esh);
                        if (p.ep_relu && !ep_res && !(v > 0.0f)) v = 0.0f;
                    }
                    if (PRECISE) reinterpret_cast<float*>(ot)[row * OS + col] = v;
                    else reinterpret_cast<__bf16*>(ot)[row * OS + col] = (__bf16)v;
                }
        }
        __syncthreads();
        constexpr int CPR = BN / O_EPC;                     // 16-byte chunks per tile row
        if constexpr (FAST && __is_same(RowMap, LinearRows) && NTHR % CPR == 0 && (TBM * CPR) % NTHR == 0) {
            if (full && !ep_res && !p.omap) {
                // whole tile, plain rows: one base address per thread, then constant strides (the generic loop below spends ~25 VALU
                // instructions per 16-byte store on row tests and 64-bit address arithmetic)
                const int ch = tid % CPR, row0 = tid / CPR;
                if (co0 + ch * O_EPC < p.Cout) {
                    constexpr int ESZ = PRECISE ? 4 : 2;
                    char* gp = reinterpret_cast<char*>(p.y) + ((m0 + row0) * (long)p.Cout + co0 + ch * O_EPC) * ESZ;
                    const long gstep = (long)(NTHR / CPR) * p.Cout * ESZ;
                    const char* lp = ot + ((size_t)row0 * OS + ch * O_EPC) * ESZ;
#pragma unroll
                    for (int it = 0; it < TBM * CPR / NTHR; ++it) {
#if GLDS_ABL & 1
                        if (it == 12345)
#endif
                        *reinterpret_cast<u32x4*>(gp) = *reinterpret_cast<const u32x4*>(lp + (size_t)it * (NTHR / CPR) * OS * ESZ);
                        gp += gstep;
                    }
                }
                return;
            }
        }
        for (int idx = tid; idx < TBM * CPR; idx += NTHR) {
            const int row = idx / CPR, ch = idx % CPR;
            const long m = row_to_m(row);
            const int co = co0 + ch * O_EPC;
            if (m < M && co < p.Cout) {
                u32x4 v = *reinterpret_cast<const u32x4*>(ot + ((size_t)row * OS + ch * O_EPC) * (PRECISE ? 4 : 2));
                const long mo = out_row(p, m);
                if (ep_res) {                               // residual add (+ ReLU) on the way out
                    const long mr = p.ep_res_out ? mo : m;
                    u32x4 rv = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(p.ep_res) + (mr * p.Cout + co) * (PRECISE ? 4 : 2));
                    if (!PRECISE && p.ep_res_bits) {            // masked shortcut gradient: one byte of mask bits per 16-byte chunk
                        const unsigned mb = p.ep_res_bits[(mr * p.Cout + co) >> 3];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            rv[e] &= ((mb >> (2 * e)) & 1u ? 0x0000FFFFu : 0u) | ((mb >> (2 * e + 1)) & 1u ? 0xFFFF0000u : 0u);
                    }
                    if (PRECISE) {
                        f32x4 a4 = __builtin_bit_cast(f32x4, v);
                        const f32x4 r4 = __builtin_bit_cast(f32x4, rv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            a4[e] += r4[e];
                            if (p.ep_relu && !(a4[e] > 0.0f)) a4[e] = 0.0f;
                        }
                        v = __builtin_bit_cast(u32x4, a4);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float lo = __builtin_bit_cast(float, v[e] << 16) + __builtin_bit_cast(float, rv[e] << 16);
                            float hi = __builtin_bit_cast(float, v[e] & 0xFFFF0000u) + __builtin_bit_cast(float, rv[e] & 0xFFFF0000u);
                            if (p.ep_relu && !(lo > 0.0f)) lo = 0.0f;
                            if (p.ep_relu && !(hi > 0.0f)) hi = 0.0f;
                            v[e] = pack2(lo, hi);
                        }
                    }
                }
#if GLDS_ABL & 1
                if (v[0] == 0x12345678u)
#endif
                *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(p.y) + (mo * p.Cout + co) * (PRECISE ? 4 : 2)) = v;
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < NTT; ++b) {
            const int co = co0 + (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const long mv = wrow0 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    const long m = row_to_m((int)(mv - m0));
                    if (mv < M && co < p.Cout) {
                        float v = acc[a][b][i];
                        const long mo = out_row(p, m);
                        if (p.ep_scale) {
                            v = __builtin_fmaf(v, p.ep_scale[co], p.ep_shift[co]);
                            if (p.ep_res) {
                                const long mr = p.ep_res_out ? mo : m;
                                if (!PRECISE) v = (float)((__bf16)v);       // same rounding points as the staged path
                                v += PRECISE ? reinterpret_cast<const float*>(p.ep_res)[mr * p.Cout + co]
                                             : (float)reinterpret_cast<const __bf16*>(p.ep_res)[mr * p.Cout + co];
                            }
                            if (p.ep_relu && !(v > 0.0f)) v = 0.0f;
                        }
                        if (PRECISE) reinterpret_cast<float*>(p.y)[mo * p.Cout + co] = v;
                        else reinterpret_cast<__bf16*>(p.y)[mo * p.Cout + co] = (__bf16)v;
                    }
                }
        }
    }
}

struct TileRows {                                           // tile row -> output pixel row of a 2-D pixel tile
    long base;                                              // (n * H + oh0) * W + ow0
    int tw_shift, W;
    __device__ __forceinline__ long operator()(int row) const {
        return base + (long)(row >> tw_shift) * W + (row & ((1 << tw_shift) - 1));
    }
};

// What zero padding / out-of-range rows / channels read through the LDS-DMA: 256 bytes of zeros in the code object.  The library is
// linked without relocatable device code, so a __device__ variable cannot be shared between units: every unit whose kernels read it
// gets its own copy (256 bytes each).
static __device__ __attribute__((aligned(256))) unsigned int g_zero_page[64];

__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

}  // namespace vqseg
