// conv_patch.hip -- the 3x3 / stride 1 / pad 1 convolution with patch reuse (bf16) and its dispatch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_device.h"
#include "conv_internal.h"

namespace vqseg {

// =====================================================================================================
// 3x3 / stride 1 / pad 1 convolution with PATCH REUSE (bf16; forward of every such layer and the data gradient
// of the zero-padded ones).
//
// The generic kernel (conv_igemm.hip) fetches a shifted copy of the input tile for each of the nine taps (A traffic 9x).
// Here a workgroup owns a 2-D tile of 256 output pixels (8 x 32, or 16 x 16 for narrow images) x BN output
// channels.  Per 64-channel chunk of the input it stages ONE haloed patch [(TH+2) x (TW+2) px][64 ci] and feeds
// all nine taps from shifted windows of it: the MFMA row (32 consecutive tile pixels) of tap (kh, kw) is the same
// LDS rows displaced by kh * (TW+2) + kw.  Only the weights [BN][64 ci] change per tap.
//   LDS: two patch buffers (the next chunk's patch arrives, one DMA instruction per wave and tap, under the taps
//   of the current chunk) + a ring of NBW weight stages; counted vmcnt, one raw barrier per tap.
// Rows are unpadded 128 B with the 16-byte chunks XOR-swizzled through the DMA source address.
// =====================================================================================================
#ifndef PATCH_ABL
#define PATCH_ABL 0               // debug builds only (results wrong): 1 no weight DMA after the prologue, 2 no patch DMA after chunk 0,
#endif                            // 4 no per-tap barrier, 8 no per-tap vmcnt wait  (tools/ab_conv.py with VQSEG_LIB: DESIGN 4.2, "what bounds it")
#ifndef CONV_SETPRIO
#define CONV_SETPRIO 0            // 1: s_setprio pair around every MFMA cluster of the patch kernel (measured: see DESIGN 4.2)
#endif

// CK: input channels per chunk (64, or 32 for layers whose channel count is not a multiple of 64: rows of 64 bytes,
// four 16-byte chunks swizzled by (row >> 2) & 3, two K steps per tap)
// TBM: output pixels per workgroup (256, or 512 with 32-channel chunks: twice the pixels per staged weight tile -- half the weight
// DMA per MFMA -- and wave tiles twice as tall: a quarter fewer fragment reads per MFMA (a third for the 32-channel-wide tiles))
template <int BN, int NBW, bool UNROLL_TAPS, int CK = 64, bool S3 = false, int TBM = 256>
__global__ __launch_bounds__(512) void conv3x3_patch_kernel(const ConvArgs p) {
    constexpr int NW = 8;
    static_assert(TBM == 256 || (TBM == 512 && CK == 32), "512-pixel tiles stage 32-channel chunks (two patch buffers must fit the LDS)");
    constexpr int PATCH_PX = TBM == 256 ? 344 : 616;       // haloed patch pixels, rounded up: 10 x 34 (18 x 18) / 18 x 34 (34 x 18)
    constexpr int NT = BN >= 128 ? 2 : 1;                  // 32-channel tiles per wave
    constexpr int WN = BN / (32 * NT), WM = NW / WN;       // wave grid; wave tile (MT*32) px x (NT*32) co
    constexpr int MT = TBM / (WM * 32);                    // BN 256/128/64/32 -> MT 4/2/2/1 (64/32-row BN stat slots)
    constexpr int ROWB = CK * 2;                           // bytes per LDS row (one pixel / one output channel)
    constexpr int RPI = 1024 / ROWB;                       // rows per 1 KB DMA instruction
    constexpr int KS = CK / 16;                            // MFMA K steps per tap
    constexpr int PI = (PATCH_PX + RPI * NW - 1) / (RPI * NW);   // patch DMA instructions per wave and chunk (6 or 3; 5 for 512 pixels)
    constexpr int PATCH_BYTES = PI * NW * 1024;
    constexpr int W_ROWS = (BN * ROWB >= NW * 1024) ? BN : NW * 1024 / ROWB;   // weight rows staged per tap (rows >= Cout: zero page)
    constexpr int W_BYTES = W_ROWS * ROWB;
    constexpr int WI = W_BYTES / 1024 / NW;                // weight DMA instructions per wave and tap
    static_assert(W_BYTES % (1024 * NW) == 0 && (CK == 64 || CK == 32), "weight tile must split evenly over the waves");
    // NBW == 0, "chunk stages": the weights of ALL nine taps of a chunk travel with its patch (one wait + one barrier per
    // chunk, none per tap).  For tiles whose taps are one or two K steps long a tap-by-tap ring only adds a DMA latency and a
    // barrier to every tap; the whole tap set of such a tile is small (9 x BN x CK x 2 B).
    constexpr bool CHUNK_STAGE = NBW == 0;
    constexpr int WT_BYTES = CHUNK_STAGE ? BN * ROWB : W_BYTES;             // LDS bytes per tap
    constexpr int WCI = 9 * BN * ROWB / 1024, WCW = (WCI + NW - 1) / NW;    // chunk-stage weight DMA instructions: all / per wave
    static_assert(!CHUNK_STAGE || (BN * ROWB) % 1024 == 0, "a tap's weight tile must be whole DMA instructions");
    auto swz = [](int row) { return CK == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); };

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const patch0 = smem;
    char* const wring = smem + ((CHUNK_STAGE && p.Cin / CK == 1) ? 1 : 2) * PATCH_BYTES;     // single-chunk layers: one patch buffer
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;

    // ---- tile geometry (host guarantees H % TH == 0, W % TW == 0, Ho == H, Wo == W)
    const int tw_shift = (p.W & 31) == 0 ? 5 : 4;
    const int TW = 1 << tw_shift, TH = TBM >> tw_shift, PW = TW + 2, PH = TH + 2;
    const int tiles_x = p.W >> tw_shift, tiles_y = p.H / TH;
    // 1-D launch (pair_chunks > 0): the workgroups that share a pixel tile (one per Cout chunk) sit 8 ids apart, i.e. on the
    // same XCD at about the same time, so the patch is fetched from HBM once and then served by that XCD's L2
    int tile_id = blockIdx.x, co_chunk = blockIdx.y;
    if (p.pair_chunks > 0) {
        const unsigned group = 8u * (unsigned)p.pair_chunks, within = blockIdx.x % group;
        tile_id = (int)(blockIdx.x / group) * 8 + (int)(within & 7u);
        co_chunk = (int)(within >> 3);
        if (tile_id >= p.pair_tiles) return;
    }
    int t = tile_id;
    const int txi = t % tiles_x;
    t /= tiles_x;
    const int tyi = t % tiles_y;
    const int n = t / tiles_y;
    const int oh0 = tyi * TH, ow0 = txi * TW;
    const int co0 = co_chunk * BN;

    const int slot = lane & (ROWB / 16 - 1), lrow = lane / (ROWB / 16);     // 16-byte slot and row of this lane in a DMA instruction
    // ---- this lane's weight rows: byte offset of (row, swizzled 16-byte slot) inside the packed image; the (tap, chunk) part of
    // the address is uniform and stays in scalar registers (one 32-bit VGPR per DMA instruction instead of a 64-bit pointer
    // per instruction and tap).  Rows past Cout (tiles narrower than the DMA granule) re-read the last row: their outputs are
    // never stored.
    unsigned w_off[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = RPI * (wave * WI + i) + lrow;
        int co = co0 + row;
        co = co < p.Cout ? co : p.Cout - 1;
        w_off[i] = ((unsigned)co * (unsigned)(9 * ((p.Cin + 31) / 32 * 32)) + (unsigned)((slot ^ swz(row)) << 3)) * 2u;
    }
    // ---- MFMA A rows: tile row -> patch pixel (tap (0, 0))
    int a_pp[MT];
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        const int row = (wm * MT + a) * 32 + r;
        a_pp[a] = (row >> tw_shift) * PW + (row & (TW - 1));
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

    const int cin_p = (p.Cin + 31) / 32 * 32;
    const int n_chunks = p.Cin / CK;
    const int n_stage = n_chunks * 9;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    // patch rows: instruction i (0..PI-1) of this wave covers patch pixels RPI * (wave + NW * i) .. + RPI - 1.  The row's
    // input pixel is recomputed per instruction (a handful of VALU ops per tap) rather than kept in 18 registers.
    auto issue_patch = [&](int chunk, int i) {
        const int pp = RPI * (wave + NW * i) + lrow;
        const int pr = pp / PW, pc = pp - pr * PW;
        int ih = oh0 - 1 + pr, iw = ow0 - 1 + pc;
        bool ok = pr < PH;
        if (p.reflect && ok) {
            ih = reflect_idx(ih, p.H);
            iw = reflect_idx(iw, p.W);
        }
        ok = ok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        const long pix = ((long)n * p.H + ih) * p.W + iw;
        const int ci0 = chunk * CK;
        const ASource as = a_source(p, ci0);
        const char* src = as.src;
        const int csrc = as.csrc, cbase = as.cbase;
        const long off = pix * csrc + cbase + ((slot ^ swz(pp)) << 3);
        glds16(ok ? src + off * 2 : zero, patch0 + (chunk & 1) * PATCH_BYTES + (wave + NW * i) * 1024);
    };
    auto issue_weights = [&](int chunk, int tap, int wslot) {
        char* Bs = wring + wslot * W_BYTES;
        const char* sbase = reinterpret_cast<const char*>(p.w_hi) + ((long)tap * cin_p + chunk * CK) * 2;      // uniform
#pragma unroll
        for (int i = 0; i < WI; ++i) glds16(sbase + w_off[i], Bs + (wave * WI + i) * 1024);
    };
    auto compute = [&](int chunk, int tapoff, const char* Bs) {
        const char* Ps = patch0 + (chunk & 1) * PATCH_BYTES;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            bf16x8 af[MT], bfr[NT];
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int pp = a_pp[a] + tapoff;
                af[a] = *reinterpret_cast<const bf16x8*>(Ps + pp * ROWB + (((kk * 2 + h) ^ swz(pp)) << 4));
            }
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const int row = (wn * NT + b) * 32 + r;
                bfr[b] = *reinterpret_cast<const bf16x8*>(Bs + row * ROWB + (((kk * 2 + h) ^ swz(row)) << 4));
            }
#if CONV_SETPRIO
            __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
#if CONV_SETPRIO
            __builtin_amdgcn_s_setprio(0);
#endif
        }
    };

    if constexpr (CHUNK_STAGE) {
        auto issue_chunk = [&](int chunk) {
#pragma unroll
            for (int i = 0; i < PI; ++i) issue_patch(chunk, i);
            char* wb = wring + (chunk & 1) * (9 * WT_BYTES);
#pragma unroll
            for (int i = 0; i < WCW; ++i) {
                const int j = wave * WCW + i;                          // wave-uniform
                if (j < WCI) {
                    const int tap = j / (BN * ROWB / 1024), rg = j % (BN * ROWB / 1024);
                    const int row = RPI * rg + lrow;
                    int co = co0 + row;
                    co = co < p.Cout ? co : p.Cout - 1;                // outputs of such rows are never stored
                    const unsigned short* wp = p.w_hi + (long)co * (9L * cin_p) + (long)tap * cin_p + chunk * CK + ((slot ^ swz(row)) << 3);
                    glds16(reinterpret_cast<const char*>(wp), wb + j * 1024);
                }
            }
        };
        issue_chunk(0);
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __builtin_amdgcn_s_waitcnt(0x0F70);                       // vmcnt(0): this chunk's patch and weights have landed
            stage_barrier();                              // ... for every wave; the other buffers are free
            if (chunk + 1 < n_chunks) issue_chunk(chunk + 1);
            const char* wb = wring + (chunk & 1) * (9 * WT_BYTES);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) compute(chunk, (tap / 3) * PW + tap % 3, wb + tap * WT_BYTES);
        }
        __syncthreads();
        const long M = (long)p.N * p.H * p.W;
        const TileRows rows{((long)n * p.H + oh0) * p.W + ow0, tw_shift, p.W};
        conv_epilogue<TBM, BN, false, MT, NT, NT, NW * 64, TileRows, S3>(acc, p, smem, M, (long)tile_id * TBM, co0, wm, wn, r, h, tid, rows);
        return;
    }
    // ---- prologue: whole patch of chunk 0, weights of the first NBW - 1 stages
#pragma unroll
    for (int i = 0; i < PI; ++i) issue_patch(0, i);
#pragma unroll
    for (int s = 0; s < NBW - 1; ++s)
        if (s < n_stage) issue_weights(s / 9, s % 9, s);

    // stage = (chunk, tap).  Issue order inside a stage: [patch piece of chunk + 1 (taps 0..PI-1)] [weights of stage
    // s + NBW - 1].  At the top of stage s the DMA instructions younger than the weights of stage s are those of the
    // NBW - 2 later weight stages plus the patch pieces issued with them; vmcnt completes in order.
    int wslot = 0;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const bool more = chunk + 1 < n_chunks;
#pragma unroll UNROLL_TAPS ? 9 : 1
        for (int tap = 0; tap < 9; ++tap) {
            const int s = chunk * 9 + tap;
            // DMA instructions younger than the weights of stage s (issued in stages s-NBW+2 .. s-1: the weights of
            // stages s+1 .. s+NBW-2 and the patch pieces that went with them) may still be in flight
            int young = 0;
#pragma unroll
            for (int d = 1; d <= NBW - 2; ++d) {
                if (s + d < n_stage) young += WI;
                const int t = s - d;                                   // stage that issued them
                if (t >= 0) {
                    const int tt = t % 9, tc = t / 9;
                    if (tt < PI && tc + 1 < n_chunks) young += 1;
                }
            }
            if (!(PATCH_ABL & 9)) switch (young) {
#define VM_CASE(N_) case N_: __builtin_amdgcn_s_waitcnt(((N_) & 0xF) | 0x0F70); break;
                VM_CASE(1) VM_CASE(2) VM_CASE(3) VM_CASE(4) VM_CASE(5) VM_CASE(6) VM_CASE(7) VM_CASE(8) VM_CASE(9) VM_CASE(10)
#undef VM_CASE
                default: __builtin_amdgcn_s_waitcnt(0x0F70); break;
            }
            if (!(PATCH_ABL & 4)) stage_barrier();
            auto issue_next = [&]() {
                if (tap < PI && more && !(PATCH_ABL & 2)) issue_patch(chunk + 1, tap);
                const int s2 = s + NBW - 1;
                if (s2 < n_stage && !(PATCH_ABL & 1)) {
                    const int c2 = tap + NBW - 1 >= 9 ? chunk + 1 : chunk, t2 = tap + NBW - 1 >= 9 ? tap + NBW - 1 - 9 : tap + NBW - 1;
                    int ws2 = wslot + NBW - 1;
                    if (ws2 >= NBW) ws2 -= NBW;
                    issue_weights(c2, t2, ws2);
                }
            };
            // NBW == 4: the slot being refilled was last read a whole stage ago, so the DMA issue can follow this stage's
            // MFMAs (which then start right behind the barrier) instead of preceding them
            if (NBW < 4) issue_next();
            compute(chunk, (tap / 3) * PW + tap % 3, wring + wslot * W_BYTES);
            if (NBW >= 4) issue_next();
            wslot = wslot == NBW - 1 ? 0 : wslot + 1;
        }
    }
    __syncthreads();                                       // all MFMAs done: LDS is free for the output tile
    const long M = (long)p.N * p.H * p.W;
    const TileRows rows{((long)n * p.H + oh0) * p.W + ow0, tw_shift, p.W};
    conv_epilogue<TBM, BN, false, MT, NT, NT, NW * 64, TileRows, S3>(acc, p, smem, M, (long)tile_id * TBM, co0, wm, wn, r, h, tid, rows);
}

static bool conv3x3_patch_ok(const ConvArgs& a) {
    if (a.omap || a.pad_w != a.pad) return false;
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.up != 1 || a.Ho != a.H || a.Wo != a.W) return false;
    const int ck = a.Cin % 64 == 0 && (a.C1 == a.Cin || a.C1 % 64 == 0) ? 64 : 32;
    if (a.Cin % ck || (a.C1 != a.Cin && a.C1 % ck) || (a.Cout % 128 && a.Cout != 64 && a.Cout != 32)) return false;
    const int tw = (a.W % 32 == 0) ? 32 : 16, th = 256 / tw;
    if (a.W % tw || a.H % th) return false;
    const int bn = a.Cout % 128 == 0 ? 128 : a.Cout;
    return (long)a.N * (a.H / th) * (a.W / tw) * (a.Cout / bn) >= g_conv_opt.patch_min_wgs;   // at least one workgroup per CU
}

template <int BN, int NBW, bool UNROLL_TAPS, int CK = 64, int TBM = 256>
static void launch_patch_t(const ConvArgs& a, hipStream_t st) {
    constexpr int ROWB = CK * 2, RPI = 1024 / ROWB, PI = ((TBM == 256 ? 344 : 616) + RPI * 8 - 1) / (RPI * 8);
    constexpr int W_ROWS = (BN * ROWB >= 8 * 1024) ? BN : 8 * 1024 / ROWB;
    size_t lds = 2 * (size_t)PI * 8 * 1024 + (size_t)NBW * W_ROWS * ROWB;
    if (NBW == 0) {                                          // chunk stages: one or two (patch + nine taps of weights) buffers
        const int nb = a.Cin / CK > 1 ? 2 : 1;
        lds = (size_t)nb * ((size_t)PI * 8 * 1024 + 9 * (size_t)BN * ROWB);
    }
    size_t out_tile = (size_t)TBM * (BN + 8) * 2 * (a.out_s3 ? 2 : 1);
    if (a.out_s3 && out_tile > 160u * 1024u) out_tile = (size_t)TBM * (BN / 2 + 8) * 4;      // (conv_epilogue: split-3 tiles this large leave in two column halves)
    if (out_tile > lds) lds = out_tile;
    const int tw = (a.W % 32 == 0) ? 32 : 16, th = TBM / tw;
    const long tiles = (long)a.N * (a.H / th) * (a.W / tw);
    const int chunks = a.Cout / BN;
    if (g_conv_opt.patch_pair && chunks > 1) {
        ConvArgs b = a;
        b.pair_chunks = chunks;
        b.pair_tiles = (int)tiles;
        const dim3 grid1((unsigned)((tiles + 7) / 8 * 8 * chunks));
        g_conv_opt.last_variant = conv_variant_patch(BN, NBW, UNROLL_TAPS, CK, a.out_s3, TBM, true);
        if (a.out_s3) hipLaunchKernelGGL((conv3x3_patch_kernel<BN, NBW, UNROLL_TAPS, CK, true, TBM>), grid1, dim3(512), lds, st, b);
        else hipLaunchKernelGGL((conv3x3_patch_kernel<BN, NBW, UNROLL_TAPS, CK, false, TBM>), grid1, dim3(512), lds, st, b);
        return;
    }
    dim3 grid((unsigned)tiles, (unsigned)chunks);
    g_conv_opt.last_variant = conv_variant_patch(BN, NBW, UNROLL_TAPS, CK, a.out_s3, TBM, false);
    if (a.out_s3) hipLaunchKernelGGL((conv3x3_patch_kernel<BN, NBW, UNROLL_TAPS, CK, true, TBM>), grid, dim3(512), lds, st, a);
    else hipLaunchKernelGGL((conv3x3_patch_kernel<BN, NBW, UNROLL_TAPS, CK, false, TBM>), grid, dim3(512), lds, st, a);
}

// 512-pixel tiles: geometry (16 x 32 or 32 x 16 pixel tiles must divide the image), LDS of the split-3 output tile, enough workgroups
static bool conv3x3_tile512_ok(const ConvArgs& a, int bn) {
    if (a.Cin % 32 || (a.C1 != a.Cin && a.C1 % 32)) return false;
    const int tw = (a.W % 32 == 0) ? 32 : 16, th = 512 / tw;
    if (a.W % tw || a.H % th) return false;
    if (a.out_s3 && (size_t)512 * (bn + 8) * 2 * 2 > 160 * 1024) return false;
    return (long)a.N * (a.H / th) * (a.W / tw) * (a.Cout / bn) >= g_conv_opt.patch_tile512_min_wgs;
}

// The dispatcher's entry point (launch_conv_impl, bf16 launches): picks the instantiation.  k64: every tap's channel range is whole
// 64-channel chunks.  false: not a shape of this kernel, nothing launched.
bool launch_conv3x3_patch(const ConvArgs& a, bool k64, hipStream_t st) {
    if (!conv3x3_patch_ok(a)) return false;
    if ((g_conv_opt.patch_tile512 & 2) && (a.Cout == 32 || (a.Cout == 64 && a.Cin >= 64)) && conv3x3_tile512_ok(a, a.Cout)) {
        // 32 / 64 output channels: the 256-pixel tile gives every wave ONE 32-pixel row block (two LDS fragment reads per MFMA: the
        // LDS port is the limit); 512 pixels make it two (1.5 reads per MFMA) and halve the weight DMA per MFMA.  Measured (B = 32):
        // 192 -> 32 at 256^2 469 -> 337 us, 64 -> 64 at 128^2 83 -> 75 us, 32 -> 32 at 256^2 97 -> 91 us; single-chunk 32 -> 64 is
        // 14 % slower and stays on the 256-pixel tile; the 128-channel tile was 10-17 % slower at 512 pixels (and spilled in its epilogue):
        // not instantiated
        ++g_conv_opt.patch_tile512_launches;
        if (a.Cout == 64) launch_patch_t<64, 0, true, 32, 512>(a, st);
        else launch_patch_t<32, 0, true, 32, 512>(a, st);
    } else if (!k64) {                                              // 32-channel chunks (the last decoder level and its gradients)
        // taps of one or two K steps: all nine taps' weights ride with the patch (chunk stages) where that fits LDS
        if (g_conv_opt.patch_chunk_stage && a.Cout == 64) launch_patch_t<64, 0, true, 32>(a, st);
        else if (g_conv_opt.patch_chunk_stage && a.Cout == 32) launch_patch_t<32, 0, true, 32>(a, st);
        else if (g_conv_opt.patch_chunk_stage && a.Cin == 32) launch_patch_t<128, 0, true, 32>(a, st);
        else if (a.Cout == 64) launch_patch_t<64, 3, true, 32>(a, st);
        else if (a.Cout == 32) launch_patch_t<32, 3, true, 32>(a, st);
        else launch_patch_t<128, 3, true, 32>(a, st);
    } else {
        const int tw = (a.W % 32 == 0) ? 32 : 16, th = 256 / tw;
        const long tiles = (long)a.N * (a.H / th) * (a.W / tw);
        // 256-wide channel tile (wave tile 128 px x 64 co: 25 % fewer LDS fragment reads per MFMA) when it still fills the chip
        if (a.Cout == 64) launch_patch_t<64, 3, true>(a, st);
        else if (a.Cout == 32) launch_patch_t<32, 3, true>(a, st);
        else if (a.Cout % 256 == 0 && g_conv_opt.patch_wide && (!a.out_s3 || g_conv_opt.patch_wide_s3) && tiles * (a.Cout / 256) >= g_conv_opt.patch_min_wgs)
            launch_patch_t<256, 2, false>(a, st);
        else if (g_conv_opt.patch_unroll == 2)
            launch_patch_t<128, 4, true>(a, st);
        else if (g_conv_opt.patch_unroll)
            launch_patch_t<128, 3, true>(a, st);
        else
            launch_patch_t<128, 3, false>(a, st);
    }
    return true;
}

}  // namespace vqseg
