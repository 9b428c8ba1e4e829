// conv_wgrad.hip -- weight gradients of the convolutions: the per-tap kernel (fp32 / bf16), the nine-tap 3x3 and the 1x1 LDS-DMA
// kernels (bf16), their slab plans, and the fixed-order slab reduction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_device.h"
#include "conv_internal.h"

namespace vqseg {

// =====================================================================================================
// Weight gradient:  dW[co][tap][ci] = sum_m GY[m][co] * A_tap[m][ci]      (m = pixel rows, the GEMM K dim)
//
// Both operands are pixel-major in HBM (NHWC), i.e. K is their SLOW dimension.  They are staged as
// [32 pixels][channels] bf16 tiles in LDS (rows padded to +64 B: conflict-free) and the MFMA fragments
// (8 consecutive pixels of one channel per lane) are fetched with the gfx950 transposing LDS read
// ds_read_b64_tr_b16 -- no explicit transpose pass.  The pixel range is split over gridDim.z slabs
// (deterministic: each slab writes its own fp32 partial, reduced in fixed order by wgrad_reduce_kernel,
// which also converts [Cout][taps][Cin] to nn.Conv2d's [Cout][Cin][KH][KW]).
// =====================================================================================================
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int TM, int TN>
struct WgradCfg {
    static constexpr int WGM = (TM >= 4 && TN == 1) ? 4 : (TM >= 2 ? 2 : 1);
    static constexpr int WGN = (TN >= 4 && TM == 1) ? 4 : ((TN >= 2 && WGM <= 2) ? 2 : 1);
    static constexpr int PM = TM / WGM, PN = TN / WGN;
};

__device__ __forceinline__ bf16x8 tr_frag(const __bf16* tile, int row_stride, int pix0, int col0, int lane) {
    // fragment for MFMA 32x32x16: lane (r = lane & 31, h = lane >> 5) gets column (col0 + r), rows pix0 + 8h .. +7
    const int g = lane >> 4;                      // 16-lane group: (g & 1) -> column block, (g >> 1) -> h
    const int q = (lane & 15) >> 2, pp = lane & 3;
    const __bf16* a0 = tile + (pix0 + 8 * (g >> 1) + q) * row_stride + col0 + 16 * (g & 1) + 4 * pp;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 4 * row_stride));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int TM, int TN, bool PRECISE>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs p) {
    using Cfg = WgradCfg<TM, TN>;
    constexpr int BKM = 32;                               // pixels per stage
    constexpr int GS = TM * 32 + 32;                      // LDS row stride (bf16) of the GY tile (+64 B pad)
    constexpr int AS = TN * 32 + 32;
    constexpr int EPC = PRECISE ? 4 : 8;                  // elements per 16-byte chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* G_hi = reinterpret_cast<__bf16*>(smem);
    __bf16* G_lo = G_hi + (PRECISE ? BKM * GS : 0);
    __bf16* A_hi = G_lo + BKM * GS;
    __bf16* A_lo = A_hi + (PRECISE ? BKM * AS : 0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
    const bool active = wave < Cfg::WGM * Cfg::WGN;

    const int ci_tiles = (p.Cin + TN * 32 - 1) / (TN * 32);
    const int tap = blockIdx.x / ci_tiles;
    const int ci0 = (blockIdx.x - tap * ci_tiles) * (TN * 32);
    const int co0 = blockIdx.y * (TM * 32);
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const long M = (long)p.N * p.Ho * p.Wo;
    const long Ma = (long)p.Na * p.Ho * p.Wo;               // rows of the first source (== M without a second one)
    long mz = (M + gridDim.z - 1) / gridDim.z;
    mz = (mz + BKM - 1) / BKM * BKM;
    const long m_begin = (long)blockIdx.z * mz;
    long m_end = m_begin + mz;
    if (m_end > M) m_end = M;

    f32x16 acc[Cfg::PM][Cfg::PN];
#pragma unroll
    for (int a = 0; a < Cfg::PM; ++a)
#pragma unroll
        for (int b = 0; b < Cfg::PN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

    constexpr int G_CPR = TM * 32 / EPC, A_CPR = TN * 32 / EPC;     // 16-byte chunks per tile row
    constexpr int G_N = (BKM * G_CPR + 255) / 256, A_N = (BKM * A_CPR + 255) / 256;
    u32x4 g_reg[G_N], a_reg[A_N];

    // (n, oh, ow) of each A chunk's pixel row, advanced by BKM rows per stage without divisions
    int pn[A_N], poh[A_N], pow_[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int idx = tid + 256 * i;
        long m = m_begin + (idx < BKM * A_CPR ? idx / A_CPR : 0);
        if (m >= M) m = M - 1;
        pn[i] = (int)(m / ((long)p.Ho * p.Wo));
        const int rem = (int)(m - (long)pn[i] * p.Ho * p.Wo);
        poh[i] = rem / p.Wo;
        pow_[i] = rem - poh[i] * p.Wo;
    }
    auto advance_rows = [&]() {
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            pow_[i] += BKM;
            while (pow_[i] >= p.Wo) {
                pow_[i] -= p.Wo;
                if (++poh[i] >= p.Ho) {
                    poh[i] = 0;
                    ++pn[i];
                }
            }
        }
    };

    auto load_stage = [&](long mb) {
#pragma unroll
        for (int i = 0; i < G_N; ++i) {
            const int idx = tid + 256 * i;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (idx < BKM * G_CPR) {
                const int row = idx / G_CPR, ch = idx % G_CPR;
                const long m = mb + row;
                const int co = co0 + ch * EPC;
                if (m < m_end && co < p.Cout) {
                    const bool sb = m >= Ma;                         // second source of a two-use launch
                    v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(sb ? p.gy_b : p.gy) + ((sb ? m - Ma : m) * p.Cout + co) * (PRECISE ? 4 : 2));
                }
            }
            g_reg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            const int idx = tid + 256 * i;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (idx < BKM * A_CPR) {
                const int row = idx / A_CPR, ch = idx % A_CPR;
                const long m = mb + row;
                const int cg = ci0 + ch * EPC;                       // global input channel of this chunk
                const bool second = cg >= p.C1;
                const bool sb = pn[i] >= p.Na;
                const char* xsrc = reinterpret_cast<const char*>(second ? (sb ? p.x2_b : p.x2) : (sb ? p.x_b : p.x));
                const int csrc = second ? (p.Cin - p.C1) : p.C1;
                const int cbase = second ? (cg - p.C1) : cg;
                if (m < m_end && cg < p.Cin) {
                    const int n = sb ? pn[i] - p.Na : pn[i], oh = poh[i], ow = pow_[i];    // tracked incrementally (advance_rows)
                    int ih = oh * p.stride - p.pad + kh, iw = ow * p.stride - p.pad + kw;
                    if (p.reflect) {
                        ih = reflect_idx(ih, p.H);
                        iw = reflect_idx(iw, p.W);
                    }
                    if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
                        const long off = (((long)n * p.H + ih) * p.W + iw) * csrc + cbase;
                        v = *reinterpret_cast<const u32x4*>(xsrc + off * (PRECISE ? 4 : 2));
                    }
                }
            }
            a_reg[i] = v;
        }
    };

    auto store_tile = [&](const u32x4& v, __bf16* hi, __bf16* lo, int row, int ch, int stride_) {
        if (PRECISE) {
            const f32x4 f = __builtin_bit_cast(f32x4, v);
            u32x2 h2, l2;
            h2[0] = pack2(f[0], f[1]);
            h2[1] = pack2(f[2], f[3]);
            l2[0] = pack2(f[0] - bf16_round(f[0]), f[1] - bf16_round(f[1]));
            l2[1] = pack2(f[2] - bf16_round(f[2]), f[3] - bf16_round(f[3]));
            *reinterpret_cast<u32x2*>(hi + row * stride_ + ch * 4) = h2;
            *reinterpret_cast<u32x2*>(lo + row * stride_ + ch * 4) = l2;
        } else {
            *reinterpret_cast<u32x4*>(hi + row * stride_ + ch * 8) = v;
        }
    };

    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < G_N; ++i) {
            const int idx = tid + 256 * i;
            if (idx < BKM * G_CPR) store_tile(g_reg[i], G_hi, G_lo, idx / G_CPR, idx % G_CPR, GS);
        }
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            const int idx = tid + 256 * i;
            if (idx < BKM * A_CPR) store_tile(a_reg[i], A_hi, A_lo, idx / A_CPR, idx % A_CPR, AS);
        }
    };

    if (m_begin < m_end) {
        load_stage(m_begin);
        advance_rows();
    }
    for (long mb = m_begin; mb < m_end; mb += BKM) {
        store_stage();
        __syncthreads();
        if (mb + BKM < m_end) {
            load_stage(mb + BKM);
            advance_rows();
        }
        if (active) {
#pragma unroll
            for (int kk = 0; kk < BKM / 16; ++kk) {
                bf16x8 gh[Cfg::PM], gl[Cfg::PM], ah[Cfg::PN], al[Cfg::PN];
#pragma unroll
                for (int a = 0; a < Cfg::PM; ++a) {
                    const int col = (wm * Cfg::PM + a) * 32;
                    gh[a] = tr_frag(G_hi, GS, kk * 16, col, lane);
                    if (PRECISE) gl[a] = tr_frag(G_lo, GS, kk * 16, col, lane);
                }
#pragma unroll
                for (int b = 0; b < Cfg::PN; ++b) {
                    const int col = (wn * Cfg::PN + b) * 32;
                    ah[b] = tr_frag(A_hi, AS, kk * 16, col, lane);
                    if (PRECISE) al[b] = tr_frag(A_lo, AS, kk * 16, col, lane);
                }
#pragma unroll
                for (int a = 0; a < Cfg::PM; ++a)
#pragma unroll
                    for (int b = 0; b < Cfg::PN; ++b) {
                        if (PRECISE) {
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[a], ah[b], acc[a][b], 0, 0, 0);
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[a], al[b], acc[a][b], 0, 0, 0);
                        }
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[a], ah[b], acc[a][b], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }

    // ---- epilogue: slab [z][Cout][taps][Cin] fp32 (row = co on registers, column = ci on lanes)
    if (active) {
        const int r = lane & 31, h = lane >> 5;
        const long taps = (long)p.KH * p.KW;
        float* slab = p.partial + (long)blockIdx.z * p.Cout * taps * p.Cin;
#pragma unroll
        for (int a = 0; a < Cfg::PM; ++a)
#pragma unroll
            for (int b = 0; b < Cfg::PN; ++b) {
                const int ci = ci0 + (wn * Cfg::PN + b) * 32 + r;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int co = co0 + (wm * Cfg::PM + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (co < p.Cout && ci < p.Cin) slab[((long)co * taps + tap) * p.Cin + ci] = acc[a][b][i];
                }
            }
    }
}

// sum the slabs in order; emit nn.Conv2d layout [Cout][Cin_out][KH][KW] (Cin_out <= Cin: the stem's padded
// im2col columns are dropped)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int slabs, int Cout, int Cin,
                                                           int Cin_out, int KH, int KW, int im2col, int accumulate,
                                                           float* __restrict__ gw) {
    // threads walk the SOURCE (packed) layout so the slabs are read coalesced; the transposing write happens once
    const long slab = (long)Cout * (im2col ? 1 : KH * KW) * Cin;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < slab; i += (long)gridDim.x * 256) {
        int co, kh, kw, ci;
        if (im2col) {                                       // source [Cout][Cin = padded (kh, kw, ci) columns]
            co = (int)(i / Cin);
            const int col = (int)(i % Cin);
            if (col >= KH * KW * Cin_out) continue;
            ci = col % Cin_out;
            kw = (col / Cin_out) % KW;
            kh = col / (Cin_out * KW);
        } else {                                            // source [Cout][KH][KW][Cin]
            ci = (int)(i % Cin);
            long t = i / Cin;
            kw = (int)(t % KW);
            t /= KW;
            kh = (int)(t % KH);
            co = (int)(t / KH);
            if (ci >= Cin_out) continue;
        }
        double s = 0.0;
        int z = 0;
        for (; z + 3 < slabs; z += 4) {                     // four slabs' values in flight (latency bound), added in slab order
            const float v0 = partial[(long)z * slab + i], v1 = partial[(long)(z + 1) * slab + i];
            const float v2 = partial[(long)(z + 2) * slab + i], v3 = partial[(long)(z + 3) * slab + i];
            s += (double)v0;
            s += (double)v1;
            s += (double)v2;
            s += (double)v3;
        }
        for (; z < slabs; ++z) s += (double)partial[(long)z * slab + i];
        float* dst = gw + (((long)co * Cin_out + ci) * KH + kh) * KW + kw;
        *dst = accumulate ? *dst + (float)s : (float)s;
    }
}

// =====================================================================================================
// Weight gradient of 3x3 / stride 1 / pad 1 layers, ALL NINE TAPS IN ONE WORKGROUP (bf16 activations).
//
// The per-tap kernel above re-reads the GY tile and a shifted copy of the input for each tap: 64 B of operand
// per MFMA clock and CU, far above what L2 -> LDS delivers.  Here a workgroup owns (32*COT output channels) x
// (32*CIT input channels) x 9 taps and walks 4 x 16 blocks of output pixels: per block it stages ONE GY tile
// [64 px][32*COT] and ONE input patch [6 x 18 px][32*CIT] (halo included) and feeds all nine taps from shifted
// windows of that patch -- the MFMA K dimension (16 pixels) is one block row, so a tap's window is 16
// consecutive patch pixels.  Both tiles arrive by LDS-DMA (global_load_lds_dwordx4) into a 3-deep ring with
// counted vmcnt; rows are unpadded and 16-byte chunks are XOR-swizzled through the SOURCE address so the
// transposing fragment reads (ds_read_b64_tr_b16, 4 pixel rows x 64 B per half-wave) are conflict-free.
// Waves split (ci tile) x (co pair) x (tap range); a wave keeps its G fragments for all its taps.
// Output: the same per-slab fp32 partials [z][Cout][9][Cin] as the per-tap kernel (fixed-order reduction).
// =====================================================================================================
// S = 2 (r4): the stride-2 layers (first conv2 of a Bottleneck stage / first conv1 of a BasicBlock stage) ran on the per-tap kernel at
// 6-8 % MFMA busy and 3-4 x the algorithmic bytes (r04_conv_weak_layers_pmc.md).  Same machinery with a 2 x 16 output block and its
// 5 x 33 input patch; the DMA de-interleaves the patch columns into an even plane (17 pixels) and an odd plane (16) per patch row, so
// a tap's 16 input pixels (columns 2 ow + kw - 1) are again CONSECUTIVE patch pixels: kw = 0 / 2 read the even plane at ow / ow + 1,
// kw = 1 the odd plane at ow.
template <int COT, int CIT, int S = 1>
struct Wg3 {
    static constexpr int BH = S == 1 ? 4 : 2;               // output rows of a block (16 columns): one MFMA K step per row
    static constexpr int PR = S * BH + 3 - S, PC = S * 16 + 3 - S, NPATCH = PR * PC;   // patch rows / columns / pixels (halo included)
    static constexpr int PM = COT >= 2 ? 2 : 1;             // co tiles per wave
    static constexpr int WO = COT / PM, WC = CIT;            // wave groups over co pairs / ci tiles
    static constexpr int NW = (COT == 4 && CIT == 2) ? 8 : 4;
    static constexpr int WT = NW / (WO * WC);                // wave groups over taps
    static constexpr int NTM = (9 + WT - 1) / WT;            // taps per wave (upper bound)
    static constexpr int RBG = COT * 64, RBA = CIT * 64;     // row bytes of the GY tile / the patch
    static constexpr int G_INSTR = BH * 16 * RBG / 1024;     // 1 KB DMA wave-instructions for the GY tile
    static constexpr int G_PER = G_INSTR / NW;
    static constexpr int P_INSTR = (NPATCH * RBA + 1023) / 1024;
    static constexpr int P_PER = (P_INSTR + NW - 1) / NW;    // every wave issues the same count (counted vmcnt)
    static constexpr int G_BYTES = BH * 16 * RBG, P_BYTES = P_PER * NW * 1024;
    static constexpr int STAGE = G_BYTES + P_BYTES;
    static constexpr int NBUF = 3;
    static_assert(G_INSTR % NW == 0, "GY tile must split evenly over the waves");
};

template <int RB>
__device__ __forceinline__ int swz_chunk(int row) {
    return RB == 256 ? ((row & 3) << 2) : (RB == 128 ? (((row >> 1) & 1) << 2) : 0);
}

// transposing fragment read from an unpadded, chunk-swizzled [rows][RB bytes] bf16 tile:
// lane (r = lane & 31, h = lane >> 5) gets column col0 + r, rows pix0 + 8h .. +7
template <int RB>
__device__ __forceinline__ bf16x8 tr_frag_swz(const char* tile, int pix0, int col0, int lane) {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int row = pix0 + 8 * (g >> 1) + q;
    const int cbyte = 2 * col0 + 32 * (g & 1) + 8 * pp;
    const char* a0 = tile + row * RB + (((cbyte >> 4) ^ swz_chunk<RB>(row)) << 4) + (cbyte & 8);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 4 * RB));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

#ifndef WGRAD_WALK_DOWN
#define WGRAD_WALK_DOWN 1
#endif
template <int COT, int CIT, int S = 1>
__global__ __launch_bounds__((Wg3<COT, CIT, S>::NW * 64)) void conv_wgrad3x3_kernel(const WgradArgs p, int blocks_per_slab) {
    using C = Wg3<COT, CIT, S>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave % C::WC, wo = (wave / C::WC) % C::WO, wt = wave / (C::WC * C::WO);
    const int t0 = (9 * wt + C::WT - 1) / C::WT, t1 = (9 * (wt + 1) + C::WT - 1) / C::WT;

    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (p.xcd_slabs > 0) {                                  // 1-D grid, a slab's tiles on one XCD (WgradArgs::xcd_slabs)
        const int cit = p.Cin / (32 * CIT), t_all = cit * (p.Cout / (32 * COT));
        const int q = blockIdx.x >> 3, t = q % t_all;
        bz = (q / t_all) * 8 + (int)(blockIdx.x & 7u);
        if (bz >= p.xcd_slabs) return;
        bx = t % cit, by = t / cit;
    }
    const int ci0 = bx * (32 * CIT), co0 = by * (32 * COT);
    const int bw = p.Wo >> 4, bh = p.Ho / C::BH;
    const int n_blk = p.N * bh * bw;
    const int b_begin = bz * blocks_per_slab;
    int b_end = b_begin + blocks_per_slab;
    if (b_end > n_blk) b_end = n_blk;
    const int ns = b_end > b_begin ? b_end - b_begin : 0;

    const bool second = ci0 >= p.C1;
    const char* xsrc_a = reinterpret_cast<const char*>(second ? p.x2 : p.x);
    const char* xsrc_b = reinterpret_cast<const char*>(second ? p.x2_b : p.x_b);     // second source (two-use launch), images >= Na
    const int csrc = second ? (p.Cin - p.C1) : p.C1;
    const int cbase = second ? (ci0 - p.C1) : ci0;
    const char* gsrc_a = reinterpret_cast<const char*>(p.gy);
    const char* gsrc_b = reinterpret_cast<const char*>(p.gy_b);
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    // ---- stage-invariant lane roles of the DMA instructions
    int g_rel[C::G_PER];                                   // element offset of this lane's GY chunk inside a block
#pragma unroll
    for (int i = 0; i < C::G_PER; ++i) {
        const int j = wave + C::NW * i;
        const int bp = j * (1024 / C::RBG) + (lane * 16) / C::RBG;          // block pixel 0..16 BH - 1
        const int slot = lane & (C::RBG / 16 - 1);
        const int chunk = slot ^ swz_chunk<C::RBG>(bp);
        g_rel[i] = ((bp >> 4) * p.Wo + (bp & 15)) * p.Cout + co0 + chunk * 8;
    }
    int p_dr[C::P_PER], p_dc[C::P_PER], p_ch[C::P_PER];   // patch row / column (relative to the block) and channel
#pragma unroll
    for (int i = 0; i < C::P_PER; ++i) {
        const int j = wave + C::NW * i;
        const int pp = j * (1024 / C::RBA) + (lane * 16) / C::RBA;          // patch pixel 0..NPATCH - 1 (beyond: zero page)
        const int slot = lane & (C::RBA / 16 - 1);
        const int chunk = slot ^ swz_chunk<C::RBA>(pp);
        const int pr = pp / C::PC;
        const int q = pp - C::PC * pr;                                      // position inside the LDS patch row
        const int pc = S == 1 ? q : (q < 17 ? 2 * q : 2 * (q - 17) + 1);   // S = 2: even plane first, then the odd plane
        p_dr[i] = pp < C::NPATCH ? pr - 1 : -(1 << 20);
        p_dc[i] = pc - 1;
        p_ch[i] = cbase + chunk * 8;
    }

    int toff[C::NTM];                                      // patch pixel offset of each of this wave's taps
#pragma unroll
    for (int t = 0; t < C::NTM; ++t) {
        const int tap = t0 + t < 9 ? t0 + t : 8;
        const int kw = tap % 3;
        toff[t] = (tap / 3) * C::PC + (S == 1 ? kw : (kw == 1 ? 17 : kw >> 1));
    }

    f32x16 acc[C::PM][C::NTM];
#pragma unroll
    for (int a = 0; a < C::PM; ++a)
#pragma unroll
        for (int t = 0; t < C::NTM; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][t][i] = 0.0f;

    // block being issued: (image, block column, block row), advanced without divisions.  r4: the walk goes DOWN a column of blocks
    // first (WGRAD_WALK_DOWN): consecutive blocks then share the 2 halo rows of the same 18 / 33 patch columns, re-read by the very
    // next stage out of L2, instead of 16+ blocks later when a row-major walk comes back one block row further down (the vertical
    // halo was 1/3 of the patch traffic: counters 1.5 x the input bytes; the horizontal one, 2 of 18 columns, still comes around late).
    // Any bijection of the block index is a valid order: a slab is a range of it.
#if WGRAD_WALK_DOWN
    int in_ = b_begin / (bh * bw);
    int ibx = (b_begin - in_ * bh * bw) / bh;
    int iby = b_begin - (in_ * bw + ibx) * bh;
#else
    int in_ = b_begin / (bh * bw);
    int iby = (b_begin - in_ * bh * bw) / bw;
    int ibx = b_begin - (in_ * bh + iby) * bw;
#endif

    auto stage = [&](int buf) {
        char* Gs = smem + buf * C::STAGE;
        char* Ps = Gs + C::G_BYTES;
        const int oh0 = iby * C::BH, ow0 = ibx * 16;
        const bool sb = in_ >= p.Na;                        // wave-uniform: the block's image belongs to the second source
        const int img = sb ? in_ - p.Na : in_;
        const char* gsrc = sb ? gsrc_b : gsrc_a;
        const char* xsrc = sb ? xsrc_b : xsrc_a;
        const long gbase = (((long)img * p.Ho + oh0) * p.Wo + ow0) * p.Cout;
#pragma unroll
        for (int i = 0; i < C::G_PER; ++i) glds16(gsrc + (gbase + g_rel[i]) * 2, Gs + (wave + C::NW * i) * 1024);
#pragma unroll
        for (int i = 0; i < C::P_PER; ++i) {
            int ih = S * oh0 + p_dr[i], iw = S * ow0 + p_dc[i];
            if (p.reflect) {
                if (ih > -(1 << 19)) ih = reflect_idx(ih, p.H);
                iw = reflect_idx(iw, p.W);
            }
            const bool ok = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            const long off = (((long)img * p.H + ih) * p.W + iw) * csrc + p_ch[i];
            glds16(ok ? xsrc + off * 2 : zero, Ps + (wave + C::NW * i) * 1024);
        }
#if WGRAD_WALK_DOWN
        if (++iby == bh) {
            iby = 0;
            if (++ibx == bw) {
                ibx = 0;
                ++in_;
            }
        }
#else
        if (++ibx == bw) {
            ibx = 0;
            if (++iby == bh) {
                iby = 0;
                ++in_;
            }
        }
#endif
    };

    auto compute = [&](int buf) {
        const char* Gs = smem + buf * C::STAGE;
        const char* Ps = Gs + C::G_BYTES;
#pragma unroll
        for (int kk = 0; kk < C::BH; ++kk) {               // block row kk = 16 pixels = one MFMA K step
            bf16x8 gf[C::PM];
#pragma unroll
            for (int a = 0; a < C::PM; ++a) gf[a] = tr_frag_swz<C::RBG>(Gs, kk * 16, (wo * C::PM + a) * 32, lane);
#pragma unroll
            for (int t = 0; t < C::NTM; ++t) {
                if (t0 + t < t1) {                          // wave-uniform
                    const bf16x8 af = tr_frag_swz<C::RBA>(Ps, kk * S * C::PC + toff[t], wc * 32, lane);
#pragma unroll
                    for (int a = 0; a < C::PM; ++a)
                        acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf[a], af, acc[a][t], 0, 0, 0);
                }
            }
        }
    };

    // ring: see conv_igemm_glds_kernel
    constexpr int G = C::G_PER + C::P_PER;
    auto wait_in_flight = [&](int stages) {
        if (stages >= 1) __builtin_amdgcn_s_waitcnt((G & 0xF) | ((G >> 4) << 14) | 0x0F70);
        else __builtin_amdgcn_s_waitcnt(0x0F70);
    };
#pragma unroll
    for (int i = 0; i < C::NBUF - 1; ++i)
        if (i < ns) stage(i);
    int slot_c = 0, slot_i = C::NBUF - 1;
    for (int s = 0; s < ns; ++s) {
        const int behind = ns - 1 - s;
        wait_in_flight(behind < C::NBUF - 2 ? behind : C::NBUF - 2);
        stage_barrier();
        if (s + C::NBUF - 1 < ns) stage(slot_i);
        compute(slot_c);
        slot_c = slot_c == C::NBUF - 1 ? 0 : slot_c + 1;
        slot_i = slot_i == C::NBUF - 1 ? 0 : slot_i + 1;
    }

    // ---- epilogue: slab [z][Cout][Cin][9] fp32 = nn.Conv2d's own layout, so the slab reduction is a plain vector
    // sum.  The accumulators (row = co on registers, column = ci on lanes, tap = register array) go through LDS
    // 16 output channels at a time as [co][ci][tap] and leave as contiguous 16-byte stores.
    const int r = lane & 31, h = lane >> 5;
    float* slab = p.partial + (long)bz * p.Cout * 9 * p.Cin;
    float* tile = reinterpret_cast<float*>(smem);
    constexpr int ROW = 32 * CIT * 9;                      // floats per output channel of this workgroup's tile
    __syncthreads();                                       // ring slots are free
#pragma unroll
    for (int ag = 0; ag < COT; ++ag) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            if (wo == ag / C::PM) {
#pragma unroll
                for (int t = 0; t < C::NTM; ++t) {
                    if (t0 + t < t1) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int row = (j & 3) + 8 * (j >> 2) + 4 * h;
                            tile[(row * (32 * CIT) + wc * 32 + r) * 9 + t0 + t] = acc[ag % C::PM][t][hf * 8 + j];
                        }
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < 16 * (ROW / 4); i += C::NW * 64) {
                const int row = i / (ROW / 4), q4 = i - row * (ROW / 4);
                const int co = co0 + ag * 32 + hf * 16 + row;
                *reinterpret_cast<f32x4*>(slab + ((long)co * p.Cin + ci0) * 9 + q4 * 4) = *reinterpret_cast<const f32x4*>(tile + row * ROW + q4 * 4);
            }
            __syncthreads();
        }
    }
}

// =====================================================================================================
// Weight gradient of 1x1 layers (bf16; stride 1 or 2, no padding): dW[co][ci] = sum_m GY[m][co] * X[m'][ci].
// Same machinery as the nine-tap kernel without the halo: 64 pixel rows per stage, GY tile [64][32*COT] and X tile
// [64][32*CIT] by LDS-DMA into a 3-deep ring (counted vmcnt), swizzled transposing fragment reads, 8 waves each owning
// PM x PN accumulator tiles.  The weight is small, the pixel count large: most workgroups are pixel slabs, so each
// operand row is fetched once or twice in total -- these layers are HBM-bound.  Partials [z][Cout][Cin] are already
// in nn.Conv2d's layout (fixed-order slab sum afterwards).
// =====================================================================================================
template <int COT, int CIT>
struct Wg1 {
    // 64-output-channel layers (r4): <2, 5> = the stem's patch matrix (160 columns: ALL of them in one workgroup, ten waves -- the
    // per-tap kernel read GY once per 32-column tile, 2 GB for a 0.94 GB problem), <2, 2> = 64 -> 64 (four waves)
    static constexpr int NW = (COT == 2 && CIT == 5) ? 10 : ((COT == 2 && CIT == 2) ? 4 : 8);
    static constexpr int WO = COT < 4 ? COT : 4, PM = COT / WO;   // wave groups over co, co tiles per wave
    static constexpr int WC = NW / WO, PN = CIT / WC;             // wave groups over ci, ci tiles per wave
    static constexpr int RBG = COT * 64, RBA = CIT * 64;         // row bytes
    static constexpr int G_BYTES = 64 * RBG, A_BYTES = 64 * RBA;
    // every wave issues the same number of 1 KB DMA instructions (counted vmcnt); instructions beyond a tile read the zero page into
    // the padding of its region
    static constexpr int G_PER = (G_BYTES / 1024 + NW - 1) / NW, A_PER = (A_BYTES / 1024 + NW - 1) / NW;
    static constexpr int G_REGION = G_PER * NW * 1024;
    static constexpr int STAGE = G_REGION + A_PER * NW * 1024;
    static constexpr int NBUF = 3;
    static_assert(WO * WC == NW && PN * WC == CIT && PM * WO == COT, "unsupported tile");
    static_assert(RBG <= 256 || RBG == 512, "GY rows: 64..256 B swizzle classes, or 512 B");
};

// chunk swizzle for 512-byte rows (32 chunks): as for 256-byte rows, rows q = 0..3 of a fragment read land in
// different 64-byte bank groups
template <int RB>
__device__ __forceinline__ int swz_chunk_w(int row) {
    // 320-byte rows (the stem's 160 patch columns) need none: consecutive rows start 16 banks apart, the four 64-byte row segments
    // of a half-wave's fragment read cover the 64 banks once
    return RB == 320 ? 0 : (RB >= 256 ? ((row & 3) << 2) : (RB == 128 ? (((row >> 1) & 1) << 2) : 0));
}
template <int RB>
__device__ __forceinline__ bf16x8 tr_frag_w(const char* tile, int pix0, int col0, int lane) {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int row = pix0 + 8 * (g >> 1) + q;
    const int cbyte = 2 * col0 + 32 * (g & 1) + 8 * pp;
    const char* a0 = tile + row * RB + (((cbyte >> 4) ^ swz_chunk_w<RB>(row)) << 4) + (cbyte & 8);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 4 * RB));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int COT, int CIT>
__global__ __launch_bounds__((Wg1<COT, CIT>::NW * 64)) void conv_wgrad1x1_kernel(const WgradArgs p, int stages_per_slab) {
    using C = Wg1<COT, CIT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave % C::WO, wc = wave / C::WO;
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (p.xcd_slabs > 0) {                                  // 1-D grid, a slab's tiles on one XCD (WgradArgs::xcd_slabs)
        const int cit = p.Cin / (32 * CIT), t_all = cit * (p.Cout / (32 * COT));
        const int q = blockIdx.x >> 3, t = q % t_all;
        bz = (q / t_all) * 8 + (int)(blockIdx.x & 7u);
        if (bz >= p.xcd_slabs) return;
        bx = t % cit, by = t / cit;
    }
    const int ci0 = bx * (32 * CIT), co0 = by * (32 * COT);
    const long M = (long)p.N * p.Ho * p.Wo;
    const long n_stage_all = (M + 63) / 64;
    const long s_begin = (long)bz * stages_per_slab;
    long s_end = s_begin + stages_per_slab;
    if (s_end > n_stage_all) s_end = n_stage_all;
    const int ns = s_end > s_begin ? (int)(s_end - s_begin) : 0;
    const char* gsrc_a = reinterpret_cast<const char*>(p.gy);
    const char* gsrc_b = reinterpret_cast<const char*>(p.gy_b);       // second source (two-use launch): rows >= Ma / images >= Na
    const char* xsrc_a = reinterpret_cast<const char*>(p.x);
    const char* xsrc_b = reinterpret_cast<const char*>(p.x_b);
    const long Ma = (long)p.Na * p.Ho * p.Wo;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    // ---- lane roles of the DMA instructions: instruction j covers tile rows j * (1024 / RB) ...
    int g_row[C::G_PER], g_col[C::G_PER];
#pragma unroll
    for (int i = 0; i < C::G_PER; ++i) {
        const int j = wave + C::NW * i;
        g_row[i] = j * (1024 / C::RBG) + (lane * 16) / C::RBG;     // rows >= 64: instruction beyond the tile (zero page)
        const int slot = lane & (C::RBG / 16 - 1);
        g_col[i] = co0 + ((slot ^ swz_chunk_w<C::RBG>(g_row[i])) << 3);
    }
    int a_row[C::A_PER], a_col[C::A_PER];
    int a_n[C::A_PER], a_oh[C::A_PER], a_ow[C::A_PER];     // output pixel of the row in the stage being issued
#pragma unroll
    for (int i = 0; i < C::A_PER; ++i) {
        const int j = wave + C::NW * i;
        const int byte = j * 1024 + lane * 16;                   // (rows need not divide 1 KB: 320-byte rows)
        a_row[i] = byte / C::RBA;                                // rows >= 64: instruction beyond the tile (zero page)
        const int slot = (byte - a_row[i] * C::RBA) >> 4;
        a_col[i] = ci0 + ((slot ^ swz_chunk_w<C::RBA>(a_row[i])) << 3);
        long m = s_begin * 64 + a_row[i];
        if (m >= M) m = M - 1;
        int rem;
        split_row(m, p.Ho * p.Wo, M, a_n[i], rem);
        a_oh[i] = rem / p.Wo;
        a_ow[i] = rem - a_oh[i] * p.Wo;
    }

    f32x16 acc[C::PM][C::PN];
#pragma unroll
    for (int a = 0; a < C::PM; ++a)
#pragma unroll
        for (int b = 0; b < C::PN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

    long issue_m0 = s_begin * 64;                          // first pixel row of the stage being issued
    auto stage = [&](int buf) {
        char* Gs = smem + buf * C::STAGE;
        char* As = Gs + C::G_REGION;
#pragma unroll
        for (int i = 0; i < C::G_PER; ++i) {
            const long m = issue_m0 + g_row[i];
            const bool sb = m >= Ma;
            glds16(g_row[i] < 64 && m < M ? (sb ? gsrc_b : gsrc_a) + ((sb ? m - Ma : m) * p.Cout + g_col[i]) * 2 : zero,
                   Gs + (wave + C::NW * i) * 1024);
        }
#pragma unroll
        for (int i = 0; i < C::A_PER; ++i) {
            const long m = issue_m0 + a_row[i];
            const bool ok = a_row[i] < 64 && m < M;
            const bool sb = a_n[i] >= p.Na;
            const long pix = ((long)(sb ? a_n[i] - p.Na : a_n[i]) * p.H + a_oh[i] * p.stride) * p.W + a_ow[i] * p.stride;
            glds16(ok ? (sb ? xsrc_b : xsrc_a) + (pix * p.Cin + a_col[i]) * 2 : zero, As + (wave + C::NW * i) * 1024);
            a_ow[i] += 64;                                  // this lane's row of the next stage
            while (a_ow[i] >= p.Wo) {
                a_ow[i] -= p.Wo;
                if (++a_oh[i] >= p.Ho) {
                    a_oh[i] = 0;
                    ++a_n[i];
                }
            }
        }
        issue_m0 += 64;
    };
    auto compute = [&](int buf) {
        const char* Gs = smem + buf * C::STAGE;
        const char* As = Gs + C::G_REGION;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8 gf[C::PM], af[C::PN];
#pragma unroll
            for (int a = 0; a < C::PM; ++a) gf[a] = tr_frag_w<C::RBG>(Gs, kk * 16, (wo * C::PM + a) * 32, lane);
#pragma unroll
            for (int b = 0; b < C::PN; ++b) af[b] = tr_frag_w<C::RBA>(As, kk * 16, (wc * C::PN + b) * 32, lane);
#pragma unroll
            for (int a = 0; a < C::PM; ++a)
#pragma unroll
                for (int b = 0; b < C::PN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf[a], af[b], acc[a][b], 0, 0, 0);
        }
    };

    constexpr int G = C::G_PER + C::A_PER;
    auto wait_in_flight = [&](int stages) {
        if (stages >= 1) __builtin_amdgcn_s_waitcnt((G & 0xF) | ((G >> 4) << 14) | 0x0F70);
        else __builtin_amdgcn_s_waitcnt(0x0F70);
    };
#pragma unroll
    for (int i = 0; i < C::NBUF - 1; ++i)
        if (i < ns) stage(i);
    int slot_c = 0, slot_i = C::NBUF - 1;
    for (int s = 0; s < ns; ++s) {
        const int behind = ns - 1 - s;
        wait_in_flight(behind < C::NBUF - 2 ? behind : C::NBUF - 2);
        stage_barrier();
        if (s + C::NBUF - 1 < ns) stage(slot_i);
        compute(slot_c);
        slot_c = slot_c == C::NBUF - 1 ? 0 : slot_c + 1;
        slot_i = slot_i == C::NBUF - 1 ? 0 : slot_i + 1;
    }

    // ---- slab [z][Cout][Cin] fp32 (row = co on registers, column = ci on lanes: 128-byte runs)
    const int r = lane & 31, h = lane >> 5;
    float* slab = p.partial + (long)bz * p.Cout * p.Cin;
#pragma unroll
    for (int a = 0; a < C::PM; ++a)
#pragma unroll
        for (int b = 0; b < C::PN; ++b) {
            const int ci = ci0 + (wc * C::PN + b) * 32 + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + (wo * C::PM + a) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                slab[(long)co * p.Cin + ci] = acc[a][b][i];
            }
        }
}

struct Wg1Plan {
    int cot, cit, slabs, stages_per_slab;                  // cot == 0: not eligible
};

static Wg1Plan wgrad1x1_plan(const WgradArgs& a, int precise, bool shape_only) {
    Wg1Plan pl{0, 0, 0, 0};
    if (precise || a.KH != 1 || a.KW != 1 || (!shape_only && a.C1 != a.Cin)) return pl;
    if (!shape_only && (a.pad != 0 || (a.stride != 1 && a.stride != 2))) return pl;
    int cot, cit;
    if (a.per_tap_only) {                                   // the stem's patch matrix: 7 x 7 x 3 taps padded to 160 columns
        if (!g_conv_opt.wgrad1x1_narrow || a.Cout % 64 || a.Cin != 160) return pl;
        cot = 2, cit = 5;
    } else if (a.Cout % 256 == 0 && a.Cin % 128 == 0) cot = 8, cit = 4;
    else if (a.Cout % 256 == 0 && a.Cin % 64 == 0) cot = 8, cit = 2;
    else if (a.Cout % 128 == 0 && a.Cin % 128 == 0) cot = 4, cit = 4;
    else if (a.Cout % 128 == 0 && a.Cin % 64 == 0) cot = 4, cit = 2;
    else if (a.Cout % 64 == 0 && a.Cin % 128 == 0) cot = 2, cit = 4;
    else if (g_conv_opt.wgrad1x1_narrow && a.Cout % 64 == 0 && a.Cin % 64 == 0) cot = 2, cit = 2;
    else return pl;
    const long tiles = (long)(a.Cin / (32 * cit)) * (a.Cout / (32 * cot));
    const long n_stage = ((long)a.N * a.Ho * a.Wo + 63) / 64;
    if (n_stage > (1L << 30)) return pl;
    long s = ((cit == 2 && cot == 2 ? 768 : 256) * g_conv_opt.wgrad_round_pct / 100 + tiles - 1) / tiles;   // one resident round of workgroups (4-wave ones: three per CU)
    const long max_s = (n_stage + 3) / 4;                   // at least 4 stages (256 pixels) per slab
    if (s > max_s) s = max_s;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    const long sps = (n_stage + s - 1) / s;
    s = (n_stage + sps - 1) / sps;
    pl.cot = cot;
    pl.cit = cit;
    pl.slabs = (int)s;
    pl.stages_per_slab = (int)sps;
    return pl;
}

template <int COT, int CIT>
static void wgrad1x1_launch_t(const WgradArgs& a, const Wg1Plan& pl, hipStream_t st) {
    using C = Wg1<COT, CIT>;
    const unsigned tiles = (unsigned)(a.Cin / (32 * CIT)) * (unsigned)(a.Cout / (32 * COT));
    if (g_conv_opt.wgrad_xcd && tiles > 1 && pl.slabs >= 8) {
        WgradArgs b = a;
        b.xcd_slabs = pl.slabs;
        g_conv_opt.last_variant = conv_variant_wgrad1x1(COT, CIT, true);
        hipLaunchKernelGGL((conv_wgrad1x1_kernel<COT, CIT>), dim3(8u * tiles * (unsigned)((pl.slabs + 7) / 8)), dim3(C::NW * 64), (size_t)C::NBUF * C::STAGE, st,
                           b, pl.stages_per_slab);
        return;
    }
    dim3 grid((unsigned)(a.Cin / (32 * CIT)), (unsigned)(a.Cout / (32 * COT)), (unsigned)pl.slabs);
    g_conv_opt.last_variant = conv_variant_wgrad1x1(COT, CIT, false);
    hipLaunchKernelGGL((conv_wgrad1x1_kernel<COT, CIT>), grid, dim3(C::NW * 64), (size_t)C::NBUF * C::STAGE, st, a, pl.stages_per_slab);
}

struct Wg3Plan {
    int cot, cit, slabs, blocks_per_slab;                  // cot == 0: not eligible
    int stride;
};

static Wg3Plan wgrad3x3_plan(const WgradArgs& a, int precise, bool shape_only, int force_cit = 0) {
    Wg3Plan pl{0, 0, 0, 0, 1};
    const bool s2 = g_conv_opt.wgrad3x3_s2 && a.H == 2 * a.Ho && a.W == 2 * a.Wo;       // stride 2 (pad 1): Cout % 128 only (COT = 4)
    if (precise || a.per_tap_only || a.KH != 3 || a.KW != 3 || a.Cout % 32 || a.Cin % 32 || a.Wo % 16) return pl;
    if (s2 ? (a.Ho % 2 || a.Cout % 128) : (a.Ho != a.H || a.Wo != a.W || a.Ho % 4)) return pl;
    if (!shape_only && (a.stride != (s2 ? 2 : 1) || a.pad != 1)) return pl;
    int cit = (a.Cin % 64 == 0 && force_cit != 1) ? 2 : 1;
    if (!shape_only && a.C1 != a.Cin && a.C1 % (32 * cit)) {
        if (a.C1 % 32) return pl;
        cit = 1;
    }
    const int cot = a.Cout % 128 == 0 ? 4 : (a.Cout % 64 == 0 ? 2 : 1);
    const long tiles = (long)(a.Cin / (32 * cit)) * (a.Cout / (32 * cot));
    const long n_blk = (long)a.N * (a.Ho / (s2 ? 2 : 4)) * (a.Wo / 16);
    if (n_blk > (1L << 30)) return pl;
    // every workgroup writes its whole (co x ci x 9) fp32 tile once, so the partial volume is (#workgroups x tile
    // bytes) whatever the layer: one resident round of workgroups is the cheapest split
    long target = (cot == 4 && cit == 2) ? 256 : 512;
    long s = (target + tiles - 1) / tiles;
    long cap = 256;
    if (g_conv_opt.wgrad3x3_fill) {
        // r4: ONE FULL round, never one workgroup more.  192 -> 32 at 256^2 ran 3 x 171 = 513 workgroups on 512 slots (two 54 KB
        // workgroups per CU): the 513th ran alone after the others -- twice the time (647 us).  And the narrow tiles left the chip
        // mostly empty (32 -> 32: 256 four-wave workgroups = one per CU where four fit).  Slots = CUs x workgroups per CU by LDS and
        // wave slots; slabs = slots / tiles rounded DOWN, up to 1024 of them while the partials stay under 64 MB.
        const int bh = s2 ? 2 : 4, npatch = s2 ? 165 : 108, nw = (cot == 4 && cit == 2) ? 8 : 4;
        const long g_bytes = (long)bh * 16 * cot * 64;
        const long p_instr = ((long)npatch * cit * 64 + 1023) / 1024;
        const long stage = g_bytes + (p_instr + nw - 1) / nw * nw * 1024;
        long per_cu = (160 * 1024) / (3 * stage);
        if (per_cu > 32 / nw) per_cu = 32 / nw;
        if (per_cu < 1) per_cu = 1;
        target = 256 * per_cu * g_conv_opt.wgrad_round_pct / 100;
        s = target / tiles;
        cap = 1024;
        const long tile_bytes = (long)cot * 32 * cit * 32 * 9 * 4;
        while (cap > 256 && cap * tiles * tile_bytes > (64L << 20)) cap >>= 1;
    }
    const long max_s = s2 ? (n_blk + 15) / 16 : (n_blk + 7) / 8;   // at least 512 pixels per slab
    if (s > max_s) s = max_s;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    const long bps = (n_blk + s - 1) / s;
    s = (n_blk + bps - 1) / bps;                            // no empty slabs
    pl.stride = s2 ? 2 : 1;
    pl.cot = cot;
    pl.cit = cit;
    pl.slabs = (int)s;
    pl.blocks_per_slab = (int)bps;
    return pl;
}

template <int COT, int CIT, int S = 1>
static void wgrad3x3_launch_t(const WgradArgs& a, const Wg3Plan& pl, hipStream_t st) {
    using C = Wg3<COT, CIT, S>;
    const unsigned tiles = (unsigned)(a.Cin / (32 * CIT)) * (unsigned)(a.Cout / (32 * COT));
    if (g_conv_opt.wgrad_xcd && tiles > 1 && pl.slabs >= 8) {
        WgradArgs b = a;
        b.xcd_slabs = pl.slabs;
        g_conv_opt.last_variant = conv_variant_wgrad3x3(COT, CIT, S, true);
        hipLaunchKernelGGL((conv_wgrad3x3_kernel<COT, CIT, S>), dim3(8u * tiles * (unsigned)((pl.slabs + 7) / 8)), dim3(C::NW * 64), (size_t)C::NBUF * C::STAGE,
                           st, b, pl.blocks_per_slab);
        return;
    }
    dim3 grid((unsigned)(a.Cin / (32 * CIT)), (unsigned)(a.Cout / (32 * COT)), (unsigned)pl.slabs);
    g_conv_opt.last_variant = conv_variant_wgrad3x3(COT, CIT, S, false);
    hipLaunchKernelGGL((conv_wgrad3x3_kernel<COT, CIT, S>), grid, dim3(C::NW * 64), (size_t)C::NBUF * C::STAGE, st, a, pl.blocks_per_slab);
}

template <int TM, int TN, bool PRECISE>
static void wgrad_launch_t(const WgradArgs& a, int slabs, hipStream_t st) {
    constexpr int GS = TM * 32 + 32, AS = TN * 32 + 32;
    const size_t lds = (size_t)32 * (GS + AS) * 2 * (PRECISE ? 2 : 1);
    dim3 grid((unsigned)(a.KH * a.KW * ((a.Cin + TN * 32 - 1) / (TN * 32))), (unsigned)((a.Cout + TM * 32 - 1) / (TM * 32)),
              (unsigned)slabs);
    g_conv_opt.last_variant = conv_variant_wgrad_tap(TM, TN, PRECISE);
    hipLaunchKernelGGL((conv_wgrad_kernel<TM, TN, PRECISE>), grid, dim3(256), lds, st, a);
}

static int wgrad_slabs_per_tap(const WgradArgs& a) {
    const int tm = a.Cout >= 128 ? 4 : (a.Cout >= 64 ? 2 : 1);
    const int tn = (a.Cin % 128 == 0) ? 4 : 1;
    const long tiles = (long)a.KH * a.KW * ((a.Cin + tn * 32 - 1) / (tn * 32)) * ((a.Cout + tm * 32 - 1) / (tm * 32));
    const long M = (long)a.N * a.Ho * a.Wo;
    long s = (1024 + tiles - 1) / tiles;                   // aim at >= ~1024 workgroups
    const long max_s = (M + 255) / 256;                     // at least 256 pixels per slab
    if (s > max_s) s = max_s;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    return (int)s;
}

// slabs the launch will use (precise/stride/pad known) ...
int wgrad_slabs(const WgradArgs& a, int precise) {
    const Wg3Plan pl = wgrad3x3_plan(a, precise, false);
    if (pl.cot) return pl.slabs;
    const Wg1Plan p1 = wgrad1x1_plan(a, precise, false);
    return p1.cot ? p1.slabs : wgrad_slabs_per_tap(a);
}

// ... and an upper bound from the shape alone (workspace sizing)
int wgrad_slabs_max(const WgradArgs& a) {
    int m = wgrad_slabs_per_tap(a);
    for (int cit = 1; cit <= 2; ++cit) {                    // a channel split may force the narrower ci tile
        const Wg3Plan pl = wgrad3x3_plan(a, 0, true, cit);
        if (pl.cot && pl.slabs > m) m = pl.slabs;
    }
    const Wg1Plan p1 = wgrad1x1_plan(a, 0, true);
    if (p1.cot && p1.slabs > m) m = p1.slabs;
    WgradArgs ap = a;                                       // the same shape as a patch matrix (the stem)
    ap.per_tap_only = 1;
    const Wg1Plan p2 = wgrad1x1_plan(ap, 0, true);
    if (p2.cot && p2.slabs > m) m = p2.slabs;
    return m;
}

static hipError_t launch_wgrad_impl(const WgradArgs& a, int precise, int slabs, int* final_layout, hipStream_t st) {
    const Wg3Plan pl = wgrad3x3_plan(a, precise, false);
    *final_layout = pl.cot ? 1 : 0;                          // 1: slabs already are [Cout][Cin][KH][KW]
    if (pl.cot && pl.stride == 2) {
        if (pl.cit == 2) wgrad3x3_launch_t<4, 2, 2>(a, pl, st);
        else wgrad3x3_launch_t<4, 1, 2>(a, pl, st);
        return hipGetLastError();
    }
    if (pl.cot) {
#define WG3_CASE(COT_, CIT_) \
    if (pl.cot == COT_ && pl.cit == CIT_) wgrad3x3_launch_t<COT_, CIT_>(a, pl, st);
        WG3_CASE(4, 2) WG3_CASE(2, 2) WG3_CASE(1, 2) WG3_CASE(4, 1) WG3_CASE(2, 1) WG3_CASE(1, 1)
#undef WG3_CASE
        return hipGetLastError();
    }
    const Wg1Plan p1 = wgrad1x1_plan(a, precise, false);
    if (p1.cot) {
        *final_layout = a.per_tap_only ? 0 : 1;             // [Cout][Cin] == [Cout][Cin][1][1]; a patch matrix: [Cout][1][columns], as the per-tap kernel
#define WG1_CASE(COT_, CIT_) \
    if (p1.cot == COT_ && p1.cit == CIT_) wgrad1x1_launch_t<COT_, CIT_>(a, p1, st);
        WG1_CASE(8, 4) WG1_CASE(8, 2) WG1_CASE(4, 4) WG1_CASE(4, 2) WG1_CASE(2, 4) WG1_CASE(2, 5) WG1_CASE(2, 2)
#undef WG1_CASE
        return hipGetLastError();
    }
    const int tm = a.Cout >= 128 ? 4 : (a.Cout >= 64 ? 2 : 1);
    const int tn = (a.Cin % 128 == 0) ? 4 : 1;
#define WG_CASE(TM_, TN_)                                               \
    if (tm == TM_ && tn == TN_) {                                       \
        if (precise) wgrad_launch_t<TM_, TN_, true>(a, slabs, st);      \
        else wgrad_launch_t<TM_, TN_, false>(a, slabs, st);             \
    }
    WG_CASE(4, 4) WG_CASE(4, 1) WG_CASE(2, 4) WG_CASE(2, 1) WG_CASE(1, 4) WG_CASE(1, 1)
#undef WG_CASE
    return hipGetLastError();
}

// the convolution profile files weight-gradient launches under kind KH * 100 + 50 + precise (the slab sums that follow are separate,
// unrecorded launches); flops = 2 * taps * Cin * Cout * output pixels, the same count as the forward layer
hipError_t launch_wgrad(const WgradArgs& a, int precise, int slabs, int* final_layout, hipStream_t st) {
    const double px = (double)a.N * a.Ho * a.Wo;
    const ConvProfileScope prof(st, 2.0 * a.KH * a.KW * (double)a.Cin * a.Cout * px, a.KH * 100 + 50 + (precise ? 1 : 0),
                                (int)(((long)a.N * a.Ho * a.Wo) >> 10), a.Cin, a.Cout, a.stride * 10 + 1);
    return launch_wgrad_impl(a, precise, slabs, final_layout, st);
}

hipError_t launch_wgrad_reduce(const float* partial, int slabs, int Cout, int Cin, int Cin_out, int KH, int KW, int im2col,
                               int accumulate, float* gw, hipStream_t st) {
    const long total = (long)Cout * (im2col ? 1 : KH * KW) * Cin;
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, partial, slabs, Cout, Cin, Cin_out, KH, KW,
                       im2col, accumulate, gw);
    return hipGetLastError();
}

}  // namespace vqseg
