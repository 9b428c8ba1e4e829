// conv_igemm.hip -- implicit-GEMM convolution on the bf16 matrix cores of gfx950 (MI355X).
//
// Reference ops replaced: nn.Conv2d inside conv_bn_relu (models/networks/unet/decoder.py:7-10) and inside
// the ResNet bottlenecks (models/encoders/resnet.py:117-190 on torchvision's Bottleneck): 3x3 / 1x1 / 7x7,
// stride 1 / 2, zero or reflect padding, no bias.  One kernel covers the forward convolution, the data
// gradient (same kernel on the output gradient with tap-flipped, channel-transposed weights and an
// up-sampled ("dilated") input grid for stride-2 layers) and -- through `x2` -- the channel concatenation
// of the decoder (decoder.py:35-37), so torch.cat never materialises.
//
// GEMM view:  Y[m, co] = sum_{tap, ci} A[m, (tap, ci)] * Wp[co, (tap, ci)],   m = (n, oh, ow) pixel rows, NHWC.
//   workgroup = 4 waves = 128 pixel rows x BN output channels, wave = 64 x (BN/2) via v_mfma_f32_32x32x16_bf16
//   K loop: taps outer, channel chunks of BK inner; A rows are gathered (zero / reflect / dilated), staged
//   global -> registers -> LDS (rows padded by 16 B => conflict-free ds_read_b128), weights likewise.
// Precision modes (template PRECISE):
//   fast    : activations and weights bf16, fp32 accumulate                       (BK = 64)
//   precise : activations fp32 in HBM, split on the fly into bf16 hi + lo; weights pre-split;
//             acc += a_lo*b_hi + a_hi*b_lo + a_hi*b_hi  (3 MFMAs)  ~ 2^-16 relative per product (BK = 32).
//             This is the parity mode (logits within 1e-3 of the fp32 CPU reference) at 3/16 of the cost
//             of the fp32 MFMA.
// Optional epilogue: per-wave partial BatchNorm statistics (count, mean, M2 over the wave's 64 rows) for a
// deterministic two-level Welford merge (no float atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_device.h"
#include "conv_internal.h"

namespace vqseg {

constexpr int BM = 128;

template <int BN, bool PRECISE, int BK, bool S3 = false>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvArgs p) {
    constexpr int BKP = BK + 8;                          // bf16 elements per LDS row (16-byte pad)
    constexpr int NT = BN / 64;                          // 32-wide N tiles per wave (BN=128 -> 2; 64 -> 1)
    constexpr int WN = (BN >= 64) ? 2 : 1;               // waves along N
    constexpr int WM = 4 / WN;                           // waves along M
    constexpr int MT = BM / (WM * 32);                   // 32-tall M tiles per wave
    constexpr int NTT = (BN >= 64) ? NT : 1;
    constexpr int A_EPC = PRECISE ? 4 : 8;               // elements per 16-byte global chunk of A
    constexpr int A_CPR = BK / A_EPC;                    // 16-byte chunks per A row and stage (8, or 4 for fast BK=32)
    constexpr int A_RPP = 256 / A_CPR;                   // rows per pass
    constexpr int A_PASSES = BM / A_RPP;
    constexpr int B_CPR = BK / 8;                        // 16-byte chunks per weight row and stage
    constexpr int B_CHUNKS = BN * B_CPR * (PRECISE ? 2 : 1);
    constexpr int B_PER_THREAD = (B_CHUNKS + 255) / 256;

    constexpr int STAGE_ELEMS = (BM + BN) * BKP * (PRECISE ? 2 : 1);    // bf16 elements of one LDS stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* As_hi = reinterpret_cast<__bf16*>(smem);                   // stage 0; stage 1 at + STAGE_ELEMS
    __bf16* As_lo = As_hi + (PRECISE ? BM * BKP : 0);
    __bf16* Bs_hi = As_lo + BM * BKP;
    __bf16* Bs_lo = Bs_hi + (PRECISE ? BN * BKP : 0);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;

    const long M = (long)p.N * p.Ho * p.Wo;
    const long m0 = (long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;

    // ---- per-thread A rows: A_PASSES passes of A_RPP rows, A_CPR chunks per row
    const int a_chunk = tid % A_CPR;
    const int a_row0 = tid / A_CPR;
    int a_n[A_PASSES], a_oh[A_PASSES], a_ow[A_PASSES];
    bool a_ok[A_PASSES];
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        long m = m0 + a_row0 + A_RPP * i;
        a_ok[i] = m < M;
        if (!a_ok[i]) m = M - 1;
        int n, rem;
        split_row(m, p.Ho * p.Wo, M, n, rem);
        a_n[i] = n;
        a_oh[i] = rem / p.Wo;
        a_ow[i] = rem - a_oh[i] * p.Wo;
    }

    f32x16 acc[MT][NTT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NTT; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

    const int n_taps = p.KH * p.KW;
    const int cin_p = (p.Cin + 31) / 32 * 32;            // packed weights pad Cin to a multiple of 32 with zeros
    const int chunks_per_tap = (cin_p + BK - 1) / BK;
    const int n_stage = n_taps * chunks_per_tap;
    const long w_row = (long)n_taps * cin_p;              // packed weight row length (bf16 elements)

    // ---- software pipeline: global loads run TWO stages ahead (two register sets), LDS is double buffered,
    //      one barrier per stage:   iteration s:  issue loads(s+2) | MFMAs on LDS[s&1] | regs(s+1) -> LDS[(s+1)&1] | barrier
    u32x4 a_r0[A_PASSES], a_r1[A_PASSES];
    u32x4 b_r0[B_PER_THREAD], b_r1[B_PER_THREAD];

    // pixel offset (in pixels, -1 = padding / out of range) of each of this thread's rows for the CURRENT tap;
    // recomputed only when the tap changes (every chunks_per_tap stages)
    long a_pix[A_PASSES];
    int cur_tap = -1;
    auto set_tap = [&](int tap) {
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            int ih = a_oh[i] * p.stride - p.pad + kh;
            int iw = a_ow[i] * p.stride - p.pad_w + kw;
            bool ok = a_ok[i];
            if (p.reflect) {
                ih = reflect_idx(ih, p.H * p.up);
                iw = reflect_idx(iw, p.W * p.up);
            }
            if (p.up == 2) {                                 // dilated input grid (stride-2 data gradient)
                ok = ok && ih >= 0 && iw >= 0 && !((ih | iw) & 1);
                ih >>= 1;
                iw >>= 1;
            }
            ok = ok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            a_pix[i] = ok ? ((long)a_n[i] * p.H + ih) * p.W + iw : -1;
        }
        cur_tap = tap;
    };

    auto load_stage = [&](int s, u32x4 (&a_reg)[A_PASSES], u32x4 (&b_reg)[B_PER_THREAD]) {
        const int tap = s / chunks_per_tap;
        const int ci0 = (s - tap * chunks_per_tap) * BK;
        if (tap != cur_tap) set_tap(tap);
        // which source tensor holds this thread's 16-byte chunk (concat fusion): [0, C1) -> x, [C1, Cin) -> x2
        const int cg = ci0 + a_chunk * A_EPC;              // global input channel of the chunk
        const ASource as = a_source(p, cg);
        const char* src = as.src;
        const int csrc = as.csrc, cbase = as.cbase;
        const bool c_ok = cg < p.Cin;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (c_ok && a_pix[i] >= 0) v = *reinterpret_cast<const u32x4*>(src + (a_pix[i] * csrc + cbase) * (PRECISE ? 4 : 2));
            a_reg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i) {
            const int idx = tid + 256 * i;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (idx < B_CHUNKS) {
                const int arr = PRECISE ? idx / (BN * B_CPR) : 0;
                const int rem = PRECISE ? idx % (BN * B_CPR) : idx;
                const int row = rem / B_CPR, ch = rem % B_CPR;
                const unsigned short* wsrc = arr ? p.w_lo : p.w_hi;
                const int co = co0 + row;
                if (co < p.Cout && ci0 + ch * 8 < cin_p)
                    v = *reinterpret_cast<const u32x4*>(wsrc + (long)co * w_row + (long)tap * cin_p + ci0 + ch * 8);
            }
            b_reg[i] = v;
        }
    };

    auto store_stage = [&](int buf, const u32x4 (&a_reg)[A_PASSES], const u32x4 (&b_reg)[B_PER_THREAD]) {
        __bf16* Ah = As_hi + buf * STAGE_ELEMS;
        __bf16* Al = As_lo + buf * STAGE_ELEMS;
        __bf16* Bh = Bs_hi + buf * STAGE_ELEMS;
        __bf16* Bl = Bs_lo + buf * STAGE_ELEMS;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            const int row = a_row0 + A_RPP * i;
            if (PRECISE) {
                const f32x4 f = __builtin_bit_cast(f32x4, a_reg[i]);
                u32x2 hi, lo;
                hi[0] = pack2(f[0], f[1]);
                hi[1] = pack2(f[2], f[3]);
                lo[0] = pack2(f[0] - bf16_round(f[0]), f[1] - bf16_round(f[1]));
                lo[1] = pack2(f[2] - bf16_round(f[2]), f[3] - bf16_round(f[3]));
                *reinterpret_cast<u32x2*>(Ah + row * BKP + a_chunk * 4) = hi;
                *reinterpret_cast<u32x2*>(Al + row * BKP + a_chunk * 4) = lo;
            } else {
                *reinterpret_cast<u32x4*>(Ah + row * BKP + a_chunk * 8) = a_reg[i];
            }
        }
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i) {
            const int idx = tid + 256 * i;
            if (idx < B_CHUNKS) {
                const int arr = PRECISE ? idx / (BN * B_CPR) : 0;
                const int rem = PRECISE ? idx % (BN * B_CPR) : idx;
                const int row = rem / B_CPR, ch = rem % B_CPR;
                __bf16* dst = arr ? Bl : Bh;
                *reinterpret_cast<u32x4*>(dst + row * BKP + ch * 8) = b_reg[i];
            }
        }
    };

    auto compute = [&](int buf) {
        const __bf16* Ah = As_hi + buf * STAGE_ELEMS;
        const __bf16* Al = As_lo + buf * STAGE_ELEMS;
        const __bf16* Bh = Bs_hi + buf * STAGE_ELEMS;
        const __bf16* Bl = Bs_lo + buf * STAGE_ELEMS;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 a_hi[MT], a_lo[MT], b_hi[NTT], b_lo[NTT];
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int row = (wm * MT + a) * 32 + r;
                a_hi[a] = *reinterpret_cast<const bf16x8*>(Ah + row * BKP + kk * 16 + h * 8);
                if (PRECISE) a_lo[a] = *reinterpret_cast<const bf16x8*>(Al + row * BKP + kk * 16 + h * 8);
            }
#pragma unroll
            for (int b = 0; b < NTT; ++b) {
                const int row = (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
                b_hi[b] = *reinterpret_cast<const bf16x8*>(Bh + row * BKP + kk * 16 + h * 8);
                if (PRECISE) b_lo[b] = *reinterpret_cast<const bf16x8*>(Bl + row * BKP + kk * 16 + h * 8);
            }
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NTT; ++b) {
                    if (PRECISE) {
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo[a], b_hi[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[a], b_lo[b], acc[a][b], 0, 0, 0);
                    }
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[a], b_hi[b], acc[a][b], 0, 0, 0);
                }
        }
    };

    load_stage(0, a_r0, b_r0);
    if (n_stage > 1) load_stage(1, a_r1, b_r1);
    store_stage(0, a_r0, b_r0);
    __syncthreads();
    for (int s = 0; s < n_stage; s += 2) {
        // even stage s: registers set 0 is free (stored last iteration / prologue), set 1 holds stage s+1
        if (s + 2 < n_stage) load_stage(s + 2, a_r0, b_r0);
        compute(0);
        if (s + 1 < n_stage) store_stage(1, a_r1, b_r1);
        __syncthreads();
        if (s + 1 >= n_stage) break;
        // odd stage s+1
        if (s + 3 < n_stage) load_stage(s + 3, a_r1, b_r1);
        compute(1);
        if (s + 2 < n_stage) store_stage(0, a_r0, b_r0);
        __syncthreads();
    }

    conv_epilogue<BM, BN, PRECISE, MT, NTT, NT, 256, LinearRows, S3, false>(acc, p, smem, M, m0, co0, wm, wn, r, h, tid);
}

// =====================================================================================================
// Fast-mode (bf16) convolution with LDS-DMA staging.
//
// The register-staged kernel above is LDS-bound in bf16 mode: every stage pushes 32 KiB through the ds_write
// path (~79 B/clk/CU) on top of 64 KiB of fragment reads.  Here both operand tiles go global -> LDS directly
// (global_load_lds_dwordx4: no VGPR staging, no ds_write), which leaves only the fragment reads on the LDS.
//   * LDS image: [row][64 bf16] = 128-byte rows, UNPADDED (a wave-instruction writes 1 KiB = 8 whole rows,
//     lane l -> row l>>3, 16-byte slot l&7), XOR-swizzled through the SOURCE address: slot p of row R holds
//     channel chunk c = p ^ ((R >> 1) & 7); readers apply the same XOR.  With two rows per 256-byte bank row this
//     makes every 16-lane ds_read_b128 group hit 16 distinct slots (conflict-free).
//   * zero padding / out-of-range rows / channels read a 256-byte zero page in the code object.
//   * double-buffered stages, one barrier per stage, the next stage's DMA issued before the current MFMAs.
// Requires every tap's channel range to be whole 64-channel chunks (Cin % 64 == 0, concat split % 64 == 0).
// =====================================================================================================
// LIN: 1x1 / stride 1 / no padding, output pixel grid == input pixel grid: GEMM row m IS input pixel m.  The generic prologue
// spends ~600 VALU instructions per wave on (image, row, column) splits and tap geometry that such a layer does not need -- and
// these launches are VALU-ISSUE bound, not memory bound (rocprofv3 SQ_INSTS_VALU: 1544 per wave for a tile whose K loop is 16 MFMAs;
// 16 resident waves per CU x 1544 x 4 cycles = 94 of the 111 us of the 64 -> 256 layer at 128^2; profiles/LEDGER.md, round 3).
template <int TBM, int BN, int NW, int NBUF, int MINW = 1, bool S3 = false, bool LIN = false, bool CLS = false>
__global__ __launch_bounds__(NW * 64, MINW) void conv_igemm_glds_kernel(const ConvArgs pk) {
    // CLS: the launch holds several convolution problems over the same input (pk.cls: the parity classes of a stride-2 data
    // gradient); this workgroup's class replaces the per-problem fields.  All of it is workgroup-uniform (scalar registers).
    ConvArgs pc;
    long cls_tile0 = 0;
    if constexpr (CLS) {
        pc = pk;
        int c = 0;
        while (c + 1 < pk.n_cls && blockIdx.x >= pk.cls[c].tile_end) ++c;
        cls_tile0 = c ? pk.cls[c - 1].tile_end : 0;
        const ConvArgs::Cls& k = pk.cls[c];
        pc.KH = k.KH, pc.KW = k.KW, pc.pad = k.pad, pc.pad_w = k.pad_w, pc.Ho = k.Ho, pc.Wo = k.Wo;
        pc.omap_ph = k.ph, pc.omap_pw = k.pw;
        pc.w_hi = pk.w_hi + k.w_off;
    }
    const ConvArgs& p = CLS ? pc : pk;
    constexpr int BK = 64;
    // wave grid WM x WN over the TBM x BN tile; wave tile (MT*32) x (NT*32)
    constexpr int WN = (BN >= 256) ? 4 : (BN >= 64 ? 2 : 1);
    constexpr int WM = NW / WN;
    constexpr int MT = TBM / (WM * 32);
    constexpr int NT = (BN >= 64) ? BN / (WN * 32) : 1;
    constexpr int NTT = NT;
    constexpr int STAGE_BYTES = (TBM + BN) * BK * 2;
    constexpr int A_INSTR = TBM / 8 / NW;                // wave-instructions per wave for the A tile (8 rows each)
    constexpr int B_ROWS_PER_WAVE = BN / NW;
    constexpr int B_INSTR = (B_ROWS_PER_WAVE + 7) / 8;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;

    const long M = (long)p.N * p.Ho * p.Wo;
    // 1-D launch (pair_chunks > 0): the Cout chunks of an M tile sit 8 workgroup ids apart = on the same XCD at about the
    // same time, so the A rows come from HBM once and from that XCD's L2 for the other chunks
    long m_tile = blockIdx.x - cls_tile0;
    int co_chunk = blockIdx.y;
    if (p.pair_chunks > 0) {
        const unsigned group = 8u * (unsigned)p.pair_chunks, within = blockIdx.x % group;
        m_tile = (long)(blockIdx.x / group) * 8 + (within & 7u);
        co_chunk = (int)(within >> 3);
        if (m_tile >= p.pair_tiles) return;
    }
    const long m0 = m_tile * TBM;
    const int co0 = co_chunk * BN;

    // ---- this lane's A rows: instruction i of this wave covers tile rows 8*(A_INSTR*wave + i) .. +7; lane -> row l>>3
    const int slot = lane & 7;
    int a_n[A_INSTR], a_oh[A_INSTR], a_ow[A_INSTR], a_chunk[A_INSTR];
    bool a_ok[A_INSTR];
    long a_pix[A_INSTR];                                   // pixel offset of this lane's rows for the current tap, -1 = zero
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int trow = 8 * (A_INSTR * wave + i) + (lane >> 3);
        long m = m0 + trow;
        a_ok[i] = m < M;
        a_chunk[i] = slot ^ ((trow >> 1) & 7);           // channel chunk (8 bf16) this lane fetches for its slot
        if constexpr (LIN) {
            a_pix[i] = a_ok[i] ? m : -1;
            a_n[i] = a_oh[i] = a_ow[i] = 0;
        } else {
            if (!a_ok[i]) m = M - 1;
            int n, rem;
            split_row(m, p.Ho * p.Wo, M, n, rem);
            a_n[i] = n;
            a_oh[i] = rem / p.Wo;
            a_ow[i] = rem - a_oh[i] * p.Wo;
            if (p.ring) {                                    // rem = position on the border ring of a ring_h x ring_w grid
                const int q = rem, wp = p.ring_w, hp = p.ring_h;
                if (q < wp) a_oh[i] = 0, a_ow[i] = q;
                else if (q < 2 * wp) a_oh[i] = hp - 1, a_ow[i] = q - wp;
                else if (q < 2 * wp + hp - 2) a_oh[i] = 1 + (q - 2 * wp), a_ow[i] = 0;
                else a_oh[i] = 1 + (q - 2 * wp - (hp - 2)), a_ow[i] = wp - 1;
            }
        }
    }
    // ---- this lane's B rows (weights): wave w covers tile rows [w * BN/NW, (w+1) * BN/NW)
    // byte offset of (row, swizzled slot) inside the packed image, ~0u: no such row (zero page); the (tap, chunk) part of the
    // address is uniform and lives in scalar registers
    unsigned w_off[B_INSTR];
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int b_row = B_ROWS_PER_WAVE * wave + 8 * i + (lane >> 3);
        const int co = co0 + b_row;
        const bool ok = co < p.Cout && b_row < B_ROWS_PER_WAVE * (wave + 1);
        w_off[i] = ok ? ((unsigned)co * (unsigned)(p.KH * p.KW * ((p.Cin + 31) / 32 * 32)) + (unsigned)((slot ^ ((b_row >> 1) & 7)) << 3)) * 2u
                      : ~0u;
    }

    f32x16 acc[MT][NTT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NTT; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

    const int n_taps = p.KH * p.KW;
    const int cin_p = (p.Cin + 31) / 32 * 32;
    const int chunks_per_tap = p.Cin / BK;
    const int n_stage = n_taps * chunks_per_tap;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    int cur_tap = LIN ? 0 : -1;                            // LIN: one tap, a_pix set above
    auto set_tap = [&](int tap) {
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            int ih = a_oh[i] * p.stride - p.pad + kh;
            int iw = a_ow[i] * p.stride - p.pad_w + kw;
            bool ok = a_ok[i];
            if (p.reflect) {
                ih = reflect_idx(ih, p.H * p.up);
                iw = reflect_idx(iw, p.W * p.up);
            }
            if (p.up == 2) {
                ok = ok && ih >= 0 && iw >= 0 && !((ih | iw) & 1);
                ih >>= 1;
                iw >>= 1;
            }
            ok = ok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            a_pix[i] = ok ? ((long)a_n[i] * p.H + ih) * p.W + iw : -1;
        }
        cur_tap = tap;
    };

    auto stage = [&](int s, int buf) {
        char* As = smem + buf * STAGE_BYTES;
        char* Bs = As + TBM * BK * 2;
        const int tap = s / chunks_per_tap;
        const int ci0 = (s - tap * chunks_per_tap) * BK;
        if (tap != cur_tap) set_tap(tap);
        const ASource as = a_source(p, ci0);               // whole stage comes from one source (split % 64 == 0)
        const char* src = as.src;
        const int csrc = as.csrc, cbase = as.cbase;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const long off = a_pix[i] * csrc + cbase + a_chunk[i] * 8;
            if (!(GLDS_ABL & 8)) glds16(a_pix[i] >= 0 ? src + off * 2 : zero, As + (A_INSTR * wave + i) * 1024);
        }
        const char* wbase = reinterpret_cast<const char*>(p.w_hi) + ((long)tap * cin_p + ci0) * 2;             // uniform
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i)
            glds16(w_off[i] != ~0u ? wbase + w_off[i] : zero, Bs + (B_ROWS_PER_WAVE * wave + 8 * i) * 128);
    };

    auto compute = [&](int buf) {
        const char* As = smem + buf * STAGE_BYTES;
        const char* Bs = As + TBM * BK * 2;
#pragma unroll MT * NTT >= 8 ? 1 : 4
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 af[MT], bfr[NTT];
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int row = (wm * MT + a) * 32 + r;
                const int sl = (kk * 2 + h) ^ ((row >> 1) & 7);
                af[a] = *reinterpret_cast<const bf16x8*>(As + row * 128 + sl * 16);
            }
#pragma unroll
            for (int b = 0; b < NTT; ++b) {
                const int row = (BN >= 64 ? (wn * NT + b) * 32 : 0) + r;
                const int sl = (kk * 2 + h) ^ ((row >> 1) & 7);
                bfr[b] = *reinterpret_cast<const bf16x8*>(Bs + row * 128 + sl * 16);
            }
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NTT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
        }
    };

    // NBUF-deep ring, DMA NBUF-1 stages ahead, ONE raw barrier per stage and COUNTED vmcnt (never drained in the loop):
    //   iteration s:  wait until this wave's pieces of stage s have landed (later stages may still fly)  ->  s_barrier
    //   (everyone's pieces landed, everyone finished the MFMAs of stage s-1, so the slot of stage s-1 is free)  ->  issue
    //   the DMA of stage s+NBUF-1 into it  ->  MFMAs of stage s.  A slot is read only AFTER wait + barrier.
    constexpr int G = A_INSTR + B_INSTR;                   // DMA wave-instructions per wave and stage
    auto wait_in_flight = [&](int stages) {                // s_waitcnt vmcnt(stages * G), expcnt/lgkmcnt untouched
        if (stages >= 2 && NBUF >= 4) __builtin_amdgcn_s_waitcnt(((2 * G) & 0xF) | (((2 * G) >> 4) << 14) | 0x0F70);
        else if (stages >= 1 && NBUF >= 3) __builtin_amdgcn_s_waitcnt((G & 0xF) | ((G >> 4) << 14) | 0x0F70);
        else __builtin_amdgcn_s_waitcnt(0x0F70);
    };
    if constexpr (NBUF == 1) {
        // one stage buffer: no overlap inside the workgroup -- the point is its small footprint (several workgroups per
        // CU cover each other's loads and epilogues), for layers whose whole K loop is a few stages
        for (int s = 0; s < n_stage; ++s) {
            stage(s, 0);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            stage_barrier();
            compute(0);
            stage_barrier();
        }
    } else {
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i)
        if (i < n_stage) stage(i, i);
    int slot_c = 0, slot_i = NBUF - 1;                     // ring slots of stage s (compute) and s+NBUF-1 (issue)
    for (int s = 0; s < n_stage; ++s) {
        const int behind = n_stage - 1 - s;                // stages issued after stage s that may still be in flight
        wait_in_flight(behind < NBUF - 2 ? behind : NBUF - 2);
        stage_barrier();
        if (s + NBUF - 1 < n_stage) stage(s + NBUF - 1, slot_i);
        compute(slot_c);
        slot_c = slot_c == NBUF - 1 ? 0 : slot_c + 1;
        slot_i = slot_i == NBUF - 1 ? 0 : slot_i + 1;
    }
    }
    __syncthreads();                                       // all MFMAs done: LDS is free for the output tile
#if GLDS_ABL & 2
    {
        float sink = 0.0f;
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NTT; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) sink += acc[a][b][i];
        if (sink == 12345.678f) reinterpret_cast<float*>(p.y)[0] = sink;
        return;
    }
#endif
    conv_epilogue<TBM, BN, false, MT, NTT, NT, NW * 64, LinearRows, S3>(acc, p, smem, M, m0, co0, wm, wn, r, h, tid);
}

// =====================================================================================================
// The stem (7x7 / stride 2 / pad 3 on the 3-channel fp32 image) WITHOUT its patch matrix (r4).
//
// As a 1x1 convolution over a materialised [pixels][160] patch matrix the stem moved 11.5 GB per step: the bf16 matrix written once
// per batch (0.67 GB) and read by both networks' forward and again by their weight gradients, the split-3 matrix of the pseudo-label
// forwards 1.6 GB written and read twice.  Here a workgroup owns 128 consecutive output pixels of one output row x all 64 output
// channels: it stages the 7 input rows x 261 input pixels x 3 channels those pixels read (fp32, padding applied while staging, as
// im2col_stem7_strip_kernel) and the weight image in LDS.  The contraction runs over k' = kh * 24 + (kw * 3 + ci) -- each kernel
// row's 21 taps padded to 24, 7 x 24 = 168 padded to 176 = eleven MFMA K steps -- so that the 8 operands of a fragment are 8
// CONSECUTIVE words of one staged input row (offset 6 * pixel + 8 * (k' / 8 % 3)): four ds_read_b64 and four conversions per
// fragment, no per-element address arithmetic (the first version kept the patch matrix's k order and spent ~1300 VALU instructions
// per lane on it: 313 us, slower than the 280 us it replaced).  The padded positions meet zero weights; what they read is the next
// pixel's first words (finite) -- the row tails are zero-filled.  Same v_mfma_f32_32x32x16_bf16, another summation grouping than the
// patch-matrix kernel: equal to rounding, not bit-identical.  Split-3: hi w_hi, lo w_hi, hi w_lo per K step.  Same epilogue (raw y +
// BatchNorm partials, or the fused affine epilogue).  Reads the image, writes y.
// Weight image: [64][176] bf16 (split-3: [64][2][176] = w_hi | w_lo), columns kh * 24 + kw * 3 + ci, zero elsewhere.
// =====================================================================================================
#ifndef STEM_ABL
#define STEM_ABL 0                // debug builds only (results wrong): 1 no image loads, 2 no epilogue
#endif
template <bool S3>
__global__ __launch_bounds__(256) void stem7_fused_kernel(const ConvArgs p) {
    constexpr int TP = 128, NCOL = (2 * (TP - 1) + 7) * 3, ROW = 790, KQ = 176, KPW = KQ + 8, NH = (ROW + 255) / 256, NK = KQ / 16;
    static_assert(ROW >= NCOL + 2 && ROW % 2 == 0, "strip row: room for the 2 words a padded fragment reads past the last pixel; 4-byte rows");
    // The strip is kept as bf16 (split-3: a hi plane and a lo plane): the fragments are what bounds this kernel -- every wave gathers
    // 22 x 2 fragments from LDS (fp32 words: 360 KB of LDS reads per workgroup, 200 us for the loop alone) -- and bf16 halves the bytes
    // and drops the conversions from the gather.
    constexpr int PLANE = 7 * ROW;                                          // bf16 elements of one plane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* strip = reinterpret_cast<__bf16*>(smem);                        // [planes][7][ROW]
    __bf16* Bh = reinterpret_cast<__bf16*>(smem + (S3 ? 2 : 1) * ((PLANE * 2 + 15) / 16 * 16));     // [64][KPW] w_hi
    __bf16* Bl = Bh + 64 * KPW;                                             // [64][KPW] w_lo (split-3)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                                // wave tile 64 pixels x 32 channels: MT = 2, NTT = 1
    const int r = lane & 31, h = lane >> 5;
    const int strips = p.Wo / TP;
    const int sx = blockIdx.x % strips;
    const int oh = (blockIdx.x / strips) % p.Ho, n = blockIdx.x / (strips * p.Ho);
    const int H = p.H, W = p.W;
    const long M = (long)p.N * p.Ho * p.Wo;
    const long m0 = ((long)n * p.Ho + oh) * p.Wo + (long)sx * TP;
    const int iw0 = 2 * sx * TP - 3;
    // ---- stage the image strip (unconditional loads, clamped addresses: see im2col_stem7_strip_kernel) and the weights
    const float* xn = reinterpret_cast<const float*>(p.x) + (size_t)n * H * W * 3;
    float rv[NH][7];
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        const int c = tid + 256 * q;
        const int px = c / 3, ci = c - 3 * px;
        int iw = iw0 + px;
        if (p.reflect) {
            if (iw < 0) iw = -iw;
            if (iw >= W) iw = 2 * W - 2 - iw;
        }
        const bool cok = c < NCOL && iw >= 0 && iw < W;
        const int coff = cok ? iw * 3 + ci : 0;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            int ih = 2 * oh - 3 + kh;
            if (p.reflect) {
                if (ih < 0) ih = -ih;
                if (ih >= H) ih = 2 * H - 2 - ih;
            }
            const bool ok = cok && ih >= 0 && ih < H;
#if STEM_ABL & 1
            const float v = (float)coff;
#else
            const float v = xn[(ok ? ih : 0) * W * 3 + coff];
#endif
            rv[q][kh] = ok ? v : 0.0f;
        }
    }
    {
        const int row_len = S3 ? 2 * KQ : KQ;
        for (int i = tid; i < 64 * (KQ / 8); i += 256) {
            const int co = i / (KQ / 8), ch = i - co * (KQ / 8);
            *reinterpret_cast<u32x4*>(Bh + co * KPW + ch * 8) = *reinterpret_cast<const u32x4*>(p.w_hi + (size_t)co * row_len + ch * 8);
            if constexpr (S3)
                *reinterpret_cast<u32x4*>(Bl + co * KPW + ch * 8) = *reinterpret_cast<const u32x4*>(p.w_hi + (size_t)co * row_len + KQ + ch * 8);
        }
    }
#pragma unroll
    for (int q = 0; q < NH; ++q)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh)
            if (tid + 256 * q < ROW) {                      // (columns >= NCOL: zeros)
                const __bf16 hi = (__bf16)rv[q][kh];
                strip[kh * ROW + tid + 256 * q] = hi;
                if constexpr (S3) strip[PLANE + kh * ROW + tid + 256 * q] = (__bf16)(rv[q][kh] - (float)hi);
            }
    __syncthreads();

    // ---- K loop.  A fragments: K step kk, lane half h -> 8-group g8 = 2 kk + h of k' = kernel row g8 / 3 (clamped: the last group is
    // padding), taps 8 (g8 % 3) .. + 7 of that row: 8 consecutive bf16 = four 4-byte LDS reads (a pixel is 6 elements = 12 bytes
    // further on).  Fragments are used as they arrive (few registers: four workgroups per CU cover each other's load / store phases);
    // split-3: the three products of a K step back to back.
    f32x16 acc[2][1];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][0][i] = 0.0f;
    const __bf16* brow = Bh + (wn * 32 + r) * KPW + h * 8;
    const __bf16* blrow = Bl + (wn * 32 + r) * KPW + h * 8;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
        const int g8 = 2 * kk + h;
        int kh = (g8 * 11) >> 5;                                            // g8 / 3 for g8 < 32
        const int j0 = 8 * (g8 - 3 * kh);
        if (kh > 6) kh = 6;
        const __bf16* src = strip + kh * ROW + j0;
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(brow + kk * 16);
        bf16x8 bl;
        if constexpr (S3) bl = *reinterpret_cast<const bf16x8*>(blrow + kk * 16);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const unsigned* sp = reinterpret_cast<const unsigned*>(src + 6 * ((wm * 2 + a) * 32 + r));
            const bf16x8 ah = __builtin_bit_cast(bf16x8, u32x4{sp[0], sp[1], sp[2], sp[3]});
            acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b, acc[a][0], 0, 0, 0);
            if constexpr (S3) {
                const unsigned* sl = sp + PLANE / 2;
                const bf16x8 al = __builtin_bit_cast(bf16x8, u32x4{sl[0], sl[1], sl[2], sl[3]});
                acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc[a][0], 0, 0, 0);
                acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[a][0], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                       // LDS is free for the output tile
#if STEM_ABL & 2
    if (acc[0][0][0] != 12345.678f) return;
#endif
    conv_epilogue<TP, 64, false, 2, 1, 1, 256, LinearRows, S3, true>(acc, p, smem, M, m0, 0, wm, wn, r, h, tid);
}

template <int TBM, int BN, int NW, int NBUF, int MINW, bool LIN>
static void launch_glds_lin(const ConvArgs& a, hipStream_t st) {
    const int n_stage = a.KH * a.KW * (a.Cin / 64);
    // ring slots actually used: a short K loop (1x1 layers with 64..128 input channels) then leaves LDS for more
    // resident workgroups, whose loads overlap each other's epilogues
    size_t lds = (size_t)(TBM + BN) * 64 * 2 * (n_stage < NBUF ? n_stage : NBUF);
    const size_t out_tile = (size_t)TBM * (BN + 8) * 2 * (a.out_s3 ? 2 : 1);
    if (out_tile > lds) lds = out_tile;
    const long M = (long)a.N * a.Ho * a.Wo;
    const long m_tiles = (M + TBM - 1) / TBM;
    const int chunks = (a.Cout + BN - 1) / BN;
    if (chunks > 1 && chunks <= g_conv_opt.glds_pair && m_tiles < (1L << 30)) {
        ConvArgs b = a;
        b.pair_chunks = chunks;
        b.pair_tiles = (int)m_tiles;
        const dim3 grid1((unsigned)((m_tiles + 7) / 8 * 8 * chunks));
        g_conv_opt.last_variant = conv_variant_glds(TBM, BN, NW, NBUF, MINW, a.out_s3, LIN, false, true);
        if (a.out_s3) hipLaunchKernelGGL((conv_igemm_glds_kernel<TBM, BN, NW, NBUF, MINW, true, LIN>), grid1, dim3(NW * 64), lds, st, b);
        else hipLaunchKernelGGL((conv_igemm_glds_kernel<TBM, BN, NW, NBUF, MINW, false, LIN>), grid1, dim3(NW * 64), lds, st, b);
        return;
    }
    dim3 grid((unsigned)m_tiles, (unsigned)chunks);
    g_conv_opt.last_variant = conv_variant_glds(TBM, BN, NW, NBUF, MINW, a.out_s3, LIN, false, false);
    if (a.out_s3) hipLaunchKernelGGL((conv_igemm_glds_kernel<TBM, BN, NW, NBUF, MINW, true, LIN>), grid, dim3(NW * 64), lds, st, a);
    else hipLaunchKernelGGL((conv_igemm_glds_kernel<TBM, BN, NW, NBUF, MINW, false, LIN>), grid, dim3(NW * 64), lds, st, a);
}

template <int TBM, int BN, int NW, int NBUF, int MINW = 1>
static void launch_glds_t(const ConvArgs& a, hipStream_t st) {
    const bool lin = g_conv_opt.glds_lin && a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.pad_w == 0 && a.up == 1 && !a.omap &&
                     a.Ho == a.H && a.Wo == a.W;
    if (lin) launch_glds_lin<TBM, BN, NW, NBUF, MINW, true>(a, st);
    else launch_glds_lin<TBM, BN, NW, NBUF, MINW, false>(a, st);
}

// ------------------------------------------------------------------------------------
// host-side launch
// ------------------------------------------------------------------------------------
template <int BN, bool PRECISE, int BK>
static void launch_t(const ConvArgs& a, hipStream_t st) {
    constexpr int BKP = BK + 8;
    size_t lds = (size_t)(BM + BN) * BKP * 2 * (PRECISE ? 2 : 1) * 2;                 // two stages
    const size_t out_tile = (size_t)BM * (BN + (PRECISE ? 4 : 8)) * (PRECISE ? 4 : 2);  // epilogue staging tile
    if (out_tile > lds) lds = out_tile;
    const long M = (long)a.N * a.Ho * a.Wo;
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((a.Cout + BN - 1) / BN));
    g_conv_opt.last_variant = conv_variant_igemm(BN, PRECISE, BK, !PRECISE && a.out_s3);
    if constexpr (!PRECISE) {
        if (a.out_s3) {
            const size_t s3_tile = (size_t)BM * (BN + 8) * 2 * 2;
            if (s3_tile > lds) lds = s3_tile;
            hipLaunchKernelGGL((conv_igemm_kernel<BN, PRECISE, BK, true>), grid, dim3(256), lds, st, a);
            return;
        }
    }
    hipLaunchKernelGGL((conv_igemm_kernel<BN, PRECISE, BK>), grid, dim3(256), lds, st, a);
}

#ifndef SHORTK_MINW
#define SHORTK_MINW 4               // waves per SIMD the short-K tiles are compiled for (4: 128 registers, the epilogue spills ~18)
#endif
static hipError_t launch_conv_impl(const ConvArgs& a, int precise, hipStream_t st) {
    const int bn = a.Cout >= 128 ? 128 : (a.Cout >= 64 ? 64 : 32);
    const bool k64 = !precise && a.Cin % 64 == 0 && (a.C1 == a.Cin || a.C1 % 64 == 0);
    if (a.ring) {                                            // border ring of a full correlation: few rows, generic LDS-DMA kernel
        if (!k64) return hipErrorInvalidValue;
        if (bn == 128) launch_glds_t<128, 128, 4, 2>(a, st);
        else if (bn == 64) launch_glds_t<128, 64, 4, 3>(a, st);
        else launch_glds_t<128, 32, 4, 3>(a, st);
        return hipGetLastError();
    }
    if (precise) {
        if (bn == 128) launch_t<128, true, 32>(a, st);
        else if (bn == 64) launch_t<64, true, 32>(a, st);
        else launch_t<32, true, 32>(a, st);
    } else if (launch_conv3x3_patch(a, k64, st)) {
        // a 3x3 / stride 1 / pad 1 layer of the patch kernels: launched there (conv_patch.hip)
    } else if (k64) {
        // L2 -> LDS operand traffic bounds this kernel (~35 B/clk/CU): prefer the largest tile that still yields
        // at least ~2 waves of workgroups over the 256 CUs
        const long M = (long)a.N * a.Ho * a.Wo;
        const long t256x128 = ((M + 255) / 256) * ((a.Cout + 127) / 128);
        const int n_stage = a.KH * a.KW * (a.Cin / 64);
        if (n_stage <= g_conv_opt.short_k_small && bn == 128) launch_glds_t<128, 128, 4, 2, SHORTK_MINW>(a, st);
        else if (n_stage <= g_conv_opt.short_k_single && bn == 128) launch_glds_t<128, 128, 4, 1, SHORTK_MINW>(a, st);   // epilogue-bound: more, independent workgroups per CU
        else if (a.Cout % 128 == 0 && t256x128 >= 512) launch_glds_t<256, 128, 8, 3>(a, st);
        else if (bn == 128) launch_glds_t<128, 128, 4, 2>(a, st);
        else if (bn == 64) launch_glds_t<128, 64, 4, 3>(a, st);
        else launch_glds_t<128, 32, 4, 3>(a, st);
    } else {
        if (bn == 128) launch_t<128, false, 32>(a, st);
        else if (bn == 64) launch_t<64, false, 32>(a, st);
        else launch_t<32, false, 32>(a, st);
    }
    return hipGetLastError();
}

hipError_t launch_conv(const ConvArgs& a_in, int precise, hipStream_t st) {
    ConvArgs a = a_in;
    if (a.pad_w < 0) a.pad_w = a.pad;
    // algorithmic flops: 2 * taps * Cin * Cout per output pixel (a split-3 launch contracts over 3 x the logical channels:
    // its algorithmic work is the logical convolution's; `up` launches are data gradients of strided layers: the
    // up-sampled grid's zero rows are not work, so count the forward layer's pixels = input pixels of this launch)
    const double cin = a.out_s3 ? a.Cin / 3.0 : (double)a.Cin;
    const double px = a.up == 2 ? (double)a.N * a.H * a.W : (double)a.N * a.Ho * a.Wo;
    const ConvProfileScope prof(st, 2.0 * a.KH * a.KW * cin * a.Cout * px, (a.prof_k ? a.prof_k : a.KH) * 100 + (a.out_s3 ? 2 : (precise ? 1 : 0)),
                                (int)(((long)a.N * a.Ho * a.Wo) >> 10), (int)cin, a.Cout,
                                a.stride * 10 + a.up + (a.omap ? 2 : 0));              // ..3: a parity class of a stride-2 data gradient
    return launch_conv_impl(a, precise, st);
}

// x: image [N][H][W][3] f32; w_img: [64][176] bf16, columns kh * 24 + kw * 3 + ci (s3: [64][2][176] = w_hi | w_lo); y [N][Ho][Wo][64] bf16 (s3: [..][128] = hi | lo); either
// stat_partial (raw y + BatchNorm partials) or ep_scale / ep_shift (fused affine [+ ReLU]; required for s3)
hipError_t launch_stem7_fused(const float* x, const unsigned short* w_img, void* y, float* stat_partial, const float* ep_scale, const float* ep_shift,
                              int relu, int N, int H, int W, int reflect, int s3, hipStream_t st) {
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    if (!g_conv_opt.stem_fused || Wo % 128 || H < 4 || W < 4 || (long)H * W * 3 >= (1L << 31) || (long)N * Ho * (Wo / 128) >= (1L << 31) || (s3 && !ep_scale))
        return hipErrorInvalidValue;
    ConvArgs a;
    a.x = x; a.x2 = nullptr; a.C1 = 160; a.w_hi = w_img; a.w_lo = nullptr; a.y = y; a.stat_partial = stat_partial;
    a.N = N; a.H = H; a.W = W; a.Cin = 160; a.Ho = Ho; a.Wo = Wo; a.Cout = 64; a.KH = 1; a.KW = 1; a.stride = 1; a.pad = 0; a.reflect = reflect; a.up = 1;
    a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.ep_res = nullptr; a.ep_relu = relu; a.out_s3 = s3 ? 1 : 0;
    const unsigned grid = (unsigned)((long)N * Ho * (Wo / 128));
    const size_t strip_b = (size_t)(s3 ? 2 : 1) * ((7 * 790 * 2 + 15) / 16 * 16), w_b = (size_t)64 * 184 * 2 * (s3 ? 2 : 1);
    size_t lds = strip_b + w_b;
    const size_t out_tile = (size_t)128 * (64 + 8) * 2 * (s3 ? 2 : 1);
    if (out_tile > lds) lds = out_tile;
    {
        const ConvProfileScope prof(st, 2.0 * 160 * 64 * (double)N * Ho * Wo, 100 + (s3 ? 2 : 0), (int)(((long)N * Ho * Wo) >> 10), 160, 64, 11);
        if (s3) hipLaunchKernelGGL((stem7_fused_kernel<true>), dim3(grid), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((stem7_fused_kernel<false>), dim3(grid), dim3(256), lds, st, a);
    }
    return hipGetLastError();
}

// gx (n, OH, OW, Cin) = data gradient of a stride-2 K x K convolution (K = 3: padded-input grid OH = H + 2 with the reflect /
// zero fold left to the caller; K = 1: the input grid itself) from gy (n, Ho, Wo, Cout) and conv_pack_weights_s2's sub-images
// per-channel unit scale / zero shift for launches that use the fused epilogue only for its residual add
constexpr int UNIT_AFFINE_MAX = 4096;
struct UnitAffine {
    float one[UNIT_AFFINE_MAX];
    float zero[UNIT_AFFINE_MAX];
    constexpr UnitAffine() : one(), zero() {
        for (int i = 0; i < UNIT_AFFINE_MAX; ++i) one[i] = 1.0f;
    }
};
__device__ __attribute__((used)) UnitAffine g_unit_affine{};       // not `const`: a const namespace-scope object has internal linkage and is
                                                                    // not registered with the runtime (hipGetSymbolAddress aborts on it)

// `accumulate` (K == 1 only): gx already holds a gradient of the same tensor (the OTHER consumer's contribution to a fan-in);
// the data gradient is added to it in place at the pixels it touches -- no memset, no separate add pass.
hipError_t launch_dgrad_s2(const void* gy, const unsigned short* w_hi, const unsigned short* w_lo, void* gx, int N, int Ho, int Wo,
                           int Cout, int Cin, int K, int OH, int OW, int precise, int accumulate, hipStream_t st) {
    const int Cp = (Cout + 31) / 32 * 32;
    if (accumulate && (K != 1 || Cin > UNIT_AFFINE_MAX)) return hipErrorInvalidValue;
    static const UnitAffine* ua = nullptr;                   // one device per process (one process per GPU)
    if (accumulate && !ua) {
        hipError_t e = hipGetSymbolAddress((void**)&ua, HIP_SYMBOL(g_unit_affine));
        if (e != hipSuccess) return e;
    }
    if (K == 1 && !accumulate) {
        hipError_t e = hipMemsetAsync(gx, 0, (size_t)N * OH * OW * Cin * (precise ? 4 : 2), st);
        if (e != hipSuccess) return e;
    }
    size_t off = 0;
    for (int cls = 0; cls < (K == 3 ? 4 : 1); ++cls) {
        const int ph = cls >> 1, pw = cls & 1;
        const int nh = K == 3 ? (ph ? 1 : 2) : 1, nw = K == 3 ? (pw ? 1 : 2) : 1;
        ConvArgs a;
        a.x = gy; a.x2 = nullptr; a.C1 = Cout;
        a.w_hi = w_hi + off; a.w_lo = w_lo ? w_lo + off : nullptr;
        a.y = gx; a.stat_partial = nullptr;
        a.N = N; a.H = Ho; a.W = Wo; a.Cin = Cout; a.Cout = Cin; a.KH = nh; a.KW = nw;
        a.Ho = (OH - ph + 1) / 2; a.Wo = (OW - pw + 1) / 2;              // output pixels of this parity class
        a.stride = 1; a.pad = K == 3 ? (ph ? 0 : 1) : 0; a.pad_w = K == 3 ? (pw ? 0 : 1) : 0; a.reflect = 0; a.up = 1;
        a.ep_scale = nullptr; a.ep_shift = nullptr; a.ep_res = nullptr; a.ep_relu = 0;
        if (accumulate) {
            a.ep_scale = ua->one; a.ep_shift = ua->zero; a.ep_res = gx; a.ep_res_out = 1;
        }
        a.omap = 1; a.omap_h = OH; a.omap_w = OW; a.omap_ph = ph; a.omap_pw = pw;
        a.prof_k = K;
        if ((long)a.N * a.Ho * a.Wo >= (1L << 31)) return hipErrorInvalidValue;
        hipError_t e = launch_conv(a, precise, st);
        if (e != hipSuccess) return e;
        off += (size_t)Cin * nh * nw * Cp;
    }
    return hipGetLastError();
}

long dgrad_s2_fold_rows(int N, int H, int W, int reflect) {
    return (long)N * H * W + (reflect ? (long)N * (W + 1 + H) : 0) + 1;
}

// x row 1 += padded row 0 (columns 1..W -> x columns 0..W-1), x column 1 += padded column 0 (rows 1..H -> x rows 0..H-1),
// x (1, 1) += the padded corner: the reflect-padding fold of a stride-2 layer (padded row H+1 / column W+1 carry no gradient:
// H, W even).  ring [N][W + 1 + H][C] as out_row writes it; fp32 sums, one rounding.  8 channels per thread.
__global__ __launch_bounds__(256) void reflect_s2_ring_add_kernel(const __bf16* __restrict__ ring, int N, int H, int W, int C, __bf16* __restrict__ gx) {
    const int cv = C / 8, rl = W + 1 + H;
    const long total = (long)N * (W + H - 1) * cv;         // row 1 (W pixels) + column 1 without (1, 1)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % cv) * 8;
        long t = i / cv;
        const int q = (int)(t % (W + H - 1)), n = (int)(t / (W + H - 1));
        const __bf16* rn = ring + (long)n * rl * C;
        int xr, xc;
        float v[8];
        if (q < W) {                                        // x (1, q)
            xr = 1, xc = q;
            const u32x4 a = *reinterpret_cast<const u32x4*>(rn + (long)(q + 1) * C + c);
            unpack8(a, v);
            if (q == 1) {                                   // + padded (2, 0) + padded (0, 0)
                float w8[8];
                unpack8(*reinterpret_cast<const u32x4*>(rn + (long)(W + 2) * C + c), w8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += w8[e];
                unpack8(*reinterpret_cast<const u32x4*>(rn + c), w8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += w8[e];
            }
        } else {                                            // x (r, 1), r != 1: padded (r + 1, 0) = ring slot W + r + 1
            int r = q - W;
            if (r >= 1) ++r;
            xr = r, xc = 1;
            unpack8(*reinterpret_cast<const u32x4*>(rn + (long)(W + r + 1) * C + c), v);
        }
        __bf16* dst = gx + (((long)n * H + xr) * W + xc) * C + c;
        float g[8];
        unpack8(*reinterpret_cast<const u32x4*>(dst), g);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2(g[2 * e] + v[2 * e], g[2 * e + 1] + v[2 * e + 1]);
        *reinterpret_cast<u32x4*>(dst) = o;
    }
}

hipError_t launch_dgrad_s2_fold(const void* gy, const unsigned short* w_hi, void* gx, int N, int Ho, int Wo, int Cout, int Cin, int H, int W,
                                int reflect, hipStream_t st) {
    // (Cout: channels of gy = the contraction; Cin: channels of gx = the GEMM's output channels)
    if (!g_conv_opt.dgrad_s2_merge || H != 2 * Ho || W != 2 * Wo || Cout % 64 || Cin % 8 || Cin < 64 || H < 4 || W < 4) return hipErrorInvalidValue;
    const long body = dgrad_s2_fold_rows(N, H, W, reflect);
    if ((long)N * (Ho + 1) * (Wo + 1) >= (1L << 31) || body >= (1L << 31)) return hipErrorInvalidValue;
    const int Cp = (Cout + 31) / 32 * 32;
    ConvArgs a;
    a.x = gy; a.x2 = nullptr; a.C1 = Cout; a.w_hi = w_hi; a.w_lo = nullptr; a.y = gx; a.stat_partial = nullptr;
    a.N = N; a.H = Ho; a.W = Wo; a.Cin = Cout; a.Cout = Cin; a.stride = 1; a.reflect = 0; a.up = 1;
    a.ep_scale = nullptr; a.ep_shift = nullptr; a.ep_res = nullptr; a.ep_relu = 0;
    a.omap = 1; a.omap_h = H; a.omap_w = W; a.omap_fold = reflect ? 1 : 2; a.prof_k = 3;
    const int bn = Cin >= 128 ? 128 : 64;
    size_t off = 0;
    unsigned tiles = 0;
    a.n_cls = 4;
    for (int cls = 0; cls < 4; ++cls) {                     // the padded grid's parity classes, as launch_dgrad_s2 (OH = H + 2)
        const int ph = cls >> 1, pw = cls & 1;
        ConvArgs::Cls& k = a.cls[cls];
        k.KH = ph ? 1 : 2, k.KW = pw ? 1 : 2, k.pad = ph ? 0 : 1, k.pad_w = pw ? 0 : 1, k.ph = ph, k.pw = pw;
        k.Ho = (H + 2 - ph + 1) / 2, k.Wo = (W + 2 - pw + 1) / 2;
        k.w_off = (unsigned)off;
        tiles += (unsigned)(((long)N * k.Ho * k.Wo + 127) / 128);
        k.tile_end = tiles;
        off += (size_t)Cin * k.KH * k.KW * Cp;
    }
    a.KH = 2, a.KW = 2, a.pad = 1, a.pad_w = 1, a.Ho = a.cls[0].Ho, a.Wo = a.cls[0].Wo;      // (class 0; the kernel substitutes)
    const ConvProfileScope prof(st, 2.0 * 9 * (double)Cout * Cin * (double)N * Ho * Wo, 300, (int)(((long)N * H * W) >> 10), Cout, Cin, 13);
    const dim3 grid(tiles, (unsigned)((Cin + bn - 1) / bn));
    if (bn == 128 && 4 * (Cout / 64) <= g_conv_opt.short_k_single) {   // K loops of a few stages: epilogue-bound -- single buffer, four workgroups per CU
        const size_t lds = (size_t)128 * (128 + 8) * 2;       // (the output tile is the larger of the two uses)
        g_conv_opt.last_variant = conv_variant_glds(128, 128, 4, 1, SHORTK_MINW, false, false, true, false);
        hipLaunchKernelGGL((conv_igemm_glds_kernel<128, 128, 4, 1, SHORTK_MINW, false, false, true>), grid, dim3(256), lds, st, a);
    } else if (bn == 128) {
        const size_t lds = (size_t)(128 + 128) * 64 * 2 * 2;
        g_conv_opt.last_variant = conv_variant_glds(128, 128, 4, 2, 1, false, false, true, false);
        hipLaunchKernelGGL((conv_igemm_glds_kernel<128, 128, 4, 2, 1, false, false, true>), grid, dim3(256), lds, st, a);
    } else {
        const size_t lds = (size_t)(128 + 64) * 64 * 2 * 3;
        g_conv_opt.last_variant = conv_variant_glds(128, 64, 4, 3, 1, false, false, true, false);
        hipLaunchKernelGGL((conv_igemm_glds_kernel<128, 64, 4, 3, 1, false, false, true>), grid, dim3(256), lds, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && reflect) {
        const __bf16* ring = reinterpret_cast<const __bf16*>(gx) + (long)N * H * W * Cin;
        const long total = (long)N * (W + H - 1) * (Cin / 8);
        long blocks = (total + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(reflect_s2_ring_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ring, N, H, W, Cin, reinterpret_cast<__bf16*>(gx));
        e = hipGetLastError();
    }
    return e;
}

// ring [N][2 (W + 2) + 2 H][Cgx] = the full 3x3 correlation of gy [N][H][W][Cgy] with the tap-flipped transposed weights, evaluated
// on the border ring of the (H + 2) x (W + 2) grid only (bf16; Cgy % 64 == 0)
hipError_t launch_reflect_ring(const void* gy, const unsigned short* t_hi, void* ring, int N, int H, int W, int Cgy, int Cgx, hipStream_t st) {
    ConvArgs a;
    a.x = gy; a.x2 = nullptr; a.C1 = Cgy;
    a.w_hi = t_hi; a.w_lo = nullptr;
    a.y = ring; a.stat_partial = nullptr;
    a.N = N; a.H = H; a.W = W; a.Cin = Cgy; a.Cout = Cgx; a.KH = 3; a.KW = 3;
    a.ring = 1; a.ring_h = H + 2; a.ring_w = W + 2;
    a.Ho = 1; a.Wo = 2 * (W + 2) + 2 * H;
    a.stride = 1; a.pad = 2; a.pad_w = 2; a.reflect = 0; a.up = 1;
    a.ep_scale = nullptr; a.ep_shift = nullptr; a.ep_res = nullptr; a.ep_relu = 0;
    a.prof_k = 3;
    if ((long)a.N * a.Wo >= (1L << 31)) return hipErrorInvalidValue;
    return launch_conv(a, 0, st);
}

}  // namespace vqseg
