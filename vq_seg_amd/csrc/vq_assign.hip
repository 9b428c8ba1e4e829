// vq_assign.hip -- vector-quantiser hot path for gfx950 (MI355X, CDNA4).
//
// Reference algorithm: vector_quantizer/vq_img.py:160-177 (EuclideanCodebook.forward) and
// :228-244 (VectorQuantizer.forward); k-means init :29-63.  Nothing here is translated
// from the reference (which is stock ATen calls); the design is MI355X-first:
//
//   * the (N, K) distance matrix is never materialised: a wave owns a 32-row strip and
//     keeps 32 x 256 distances in 128 accumulator registers (8 tiles of
//     v_mfma_f32_32x32x2_f32, exact fp32 == a k-ordered fmaf chain), reduces them to a
//     running (min, index) per row in registers, and walks the codebook in 256-code
//     chunks;
//   * the codebook is pre-transposed once per call to ET[c][k] so that the MFMA B
//     fragment is a conflict-free 128-byte ds_read_b32 per half-wave, streamed through
//     LDS with direct global->LDS loads (global_load_lds_dwordx4), double buffered;
//   * pixel rows (A fragments) go global -> registers in fragment shape (each lane one
//     16-byte load per 8 channels); they are read once per 256-code chunk;
//   * 2 workgroups (8 waves) per CU: one wave's VALU epilogue (|x|^2 + |e|^2 - 2x.e,
//     clamp, sqrt, compare) overlaps the partner wave's MFMAs on the same SIMD.
//
// Arithmetic contract (shared with oracle/vq_chain.c, order "mfma8"):
//   dot(x, e)  = fmaf chain over channels in the order, per block of 8 channels 8j..8j+7:
//                8j, 8j+4, 8j+1, 8j+5, 8j+2, 8j+6, 8j+3, 8j+7
//   |x|^2      = (chain over channels with (c & 7) < 4, ascending) + (chain over the rest)
//   |e|^2      = chain over channels ascending
//   d          = sqrt(max(fmaf(-2, dot, |x|^2) + |e|^2, 0))        (correctly rounded sqrt)
//   idx        = lowest k attaining min d
//
// This unit: the exact kernel and its launch.  The other kernel families live in vq_filter.hip (bf16 candidate filter),
// vq_tail.hip (init, unpack, gather, backward) and vq_codebook.hip (codebook image, k-means, EMA); vq_host.hip plans and wires them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_internal.h"

namespace vqseg {

// ------------------------------------------------------------------------------------
// fused distance + argmin
//
// Work item (one workgroup, 4 waves): 128 pixel rows x (32*T) codes, all channels.
//   wave w owns rows [32w, 32w+32): T accumulator tiles of 32x32 (16 VGPRs each);
//   the code slab E4[:, code0 : code0+32T, :] streams through LDS in stages of BK channels
//   (BK*T = 128, i.e. 16 KiB per stage, double buffered, filled by global_load_lds);
//   B fragments are fetched one 8-channel block ahead of the MFMAs that use them.
// Results of different code groups of the same row are merged with a 64-bit atomicMin on
//   key = (float_bits(d) << 32) | code   (d >= 0, so unsigned order == float order and the
//   low word breaks ties towards the lowest code) -- order independent, hence deterministic.
// ------------------------------------------------------------------------------------
constexpr int ROWS_PER_WAVE = 32;
constexpr int WAVES = 4;
static_assert(ROWS_PER_WG == ROWS_PER_WAVE * WAVES, "the host's workgroup count (vq_internal.h) is this kernel's row tile");
#ifndef VQ_TIMELINE
#define VQ_TIMELINE 0             // debug build only (`make timeline` -> libvqseg_hip_tl.so; tools/vq_timeline.py): per-workgroup clock stamps
#endif
// The kernel's argument.  Its layout depends on VQ_TIMELINE, so it never leaves this unit: launch_assign_levels builds it from the
// levels the host hands over.
struct VqGroup {
    VqLevel lv[VQ_MAX_LEVELS];
    int n;
#if VQ_TIMELINE
    unsigned long long* tl;     // [workgroups][16]: (s_memrealtime, s_memtime) at 6 points of wave 0 + HW_ID + XCC_ID, or null
#endif
};
#ifndef VQ_BIG_STAGE
#define VQ_BIG_STAGE 0
#endif
#ifndef VQ_SHAPE16
#define VQ_SHAPE16 0              // 1: timing-only experiment build (wrong results), see mfma_block
#endif
// floats per LDS stage = BK * 32T: 16 KiB, or (VQ_BIG_STAGE, wide workgroups) 32 KiB = half as many barriers
constexpr int stage_floats(int T) { return (VQ_BIG_STAGE && T >= 4) ? 8192 : 4096; }

__device__ __forceinline__ void glds16(const float* g, float* lds_wave_base) {
    // one wave-instruction: 64 lanes x 16 B -> 1 KiB contiguous in LDS at lds_wave_base
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <typename TX> struct RawFrag { typedef f32x4 type; };
template <> struct RawFrag<__bf16> { typedef u32x2 type; };
template <> struct RawFrag<S3Row> { typedef u32x4 type; };   // 4 channels: [hi (2 words) | lo (2 words)]

// TX: storage type of the pixel rows (float, or __bf16 -- every bf16 value is an exact float, the arithmetic is the same -- or S3Row:
// split-3 rows [N][2C], merged to the fp32 value hi + lo where bf16 rows are widened; everything after that load is the same)
// One launch serves up to VQ_MAX_LEVELS independent quantisation problems ("levels": the three VQ layers of one forward).
// Workgroup ids [wg_end of the previous level, wg_end) belong to a level; the host orders the levels longest workgroup
// first (most channels), so that the short workgroups of the last level fill the tail of the launch.
#if VQ_TIMELINE
// per-workgroup timeline (debug build): stamp k of wave 0 = (constant 100 MHz real-time counter, shader cycle counter)
#define TL_STAMP(k_)                                                          \
    if (g.tl && threadIdx.x == 0) {                                           \
        tl_rt[k_] = __builtin_amdgcn_s_memrealtime();                         \
        tl_ck[k_] = __builtin_amdgcn_s_memtime();                             \
    }
#else
#define TL_STAMP(k_)
#endif

template <int T, typename TX = float>
__global__ __launch_bounds__(256, 2) void vq_assign_f32_kernel(const VqGroup g) {
#if VQ_TIMELINE
    unsigned long long tl_rt[6] = {0, 0, 0, 0, 0, 0}, tl_ck[6] = {0, 0, 0, 0, 0, 0};
    TL_STAMP(0)
#endif
    int lvl = 0;
    while (lvl + 1 < g.n && blockIdx.x >= g.lv[lvl].wg_end) ++lvl;                 // uniform (scalar) search
    const unsigned bid = blockIdx.x - (lvl ? g.lv[lvl - 1].wg_end : 0u);           // level offsets are multiples of 8 (XCD pairing below)
    const TX* __restrict__ x = static_cast<const TX*>(g.lv[lvl].x);
    const float* __restrict__ E4 = g.lv[lvl].E4;
    const float* __restrict__ enorm = g.lv[lvl].enorm;
    unsigned long long* __restrict__ keys = g.lv[lvl].keys;
    if (g.lv[lvl].gate && *g.lv[lvl].gate <= g.lv[lvl].gate_cap) return;       // the bf16 filter's overflow fallback: not needed (the usual case)
    const long N = g.lv[lvl].N;
    const int C = g.lv[lvl].C, Cp = g.lv[lvl].C, Kp = g.lv[lvl].Kp;
    constexpr int CODES = 32 * T;                // codes per workgroup
    constexpr int STAGE_FLOATS = stage_floats(T);
    constexpr int BK = STAGE_FLOATS / (32 * T);  // channels per stage
    constexpr int JB = BK / 8;                   // 8-channel blocks per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Bs = reinterpret_cast<float*>(smem);                 // [2][BK/4][CODES][4]
    float* xn_s = Bs + 2 * STAGE_FLOATS + 256;                  // [WAVES][32]  (after the key scratch, which aliases Bs)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n_stage = (Cp + BK - 1) / BK;
    // Workgroup id -> (row tile, code chunk).  The `chunks` workgroups that share a row tile sit 8 ids apart: the
    // dispatcher deals consecutive ids round-robin over the 8 XCDs, so they land on the SAME XCD at about the same time and
    // the second reader of the rows hits that XCD's L2 instead of HBM (HBM fetch 435 -> ~300 MB per launch at K = 512).
    const int chunks = Kp / CODES;
    const unsigned within = bid % (8u * chunks);
    const long row_tile = (long)(bid / (8u * chunks)) * 8 + (within & 7u);
    if (row_tile * ROWS_PER_WG >= N) return;                     // padding of the last group of 8 (whole workgroup exits)
    const int code0 = (int)(within >> 3) * CODES;
    const long row0 = row_tile * ROWS_PER_WG + wave * ROWS_PER_WAVE;
    long row = row0 + r;
    if (row > N - 1) row = N - 1;                               // clamp: loads stay in bounds
    constexpr bool S3 = __is_same(TX, S3Row);
    const TX* xrow = x + row * (S3 ? 2L * C : (long)C) + 4 * h;

    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    float xn_part = 0.0f;

    // stage fill: the stage is (BK/4) slabs of CODES*4 floats; one wave-instruction moves 256 floats
    // (64 codes x 4 channels).  A stage is 16 wave-instructions, 4 per wave.
    auto fill = [&](int stage, int buf) {
        float* dst = Bs + buf * STAGE_FLOATS;
#pragma unroll
        for (int q = 0; q < STAGE_FLOATS / 1024; ++q) {
            const int piece = wave * (STAGE_FLOATS / 1024) + q; // 256 floats each
            const int fl = piece * 256 + lane * 4;              // float offset inside the stage
            const int c4 = fl / (CODES * 4);                    // slab (4-channel group) inside the stage
            const int code = (fl % (CODES * 4)) >> 2;
            int slab = stage * (BK / 4) + c4;
            if (slab > Cp / 4 - 1) slab = Cp / 4 - 1;           // past the last channel: A is zero there, any finite B works
            const float* src = E4 + ((size_t)slab * Kp + code0 + code) * 4;
            glds16(src, dst + piece * 256);
        }
    };
    // bf16 rows stay RAW (8 bytes = 4 bf16 per block) until their stage becomes current (widen_a): converting at the
    // load would put the wait for the global load in front of the current stage's MFMAs
    using RawA = typename RawFrag<TX>::type;
    auto load_a = [&](int stage, RawA (&a)[JB]) {
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const int col = stage * BK + 8 * j + 4 * h;
            if (col >= C) {
                a[j] = RawA{};
            } else if constexpr (S3) {
                const u32x2 hi = *reinterpret_cast<const u32x2*>(xrow + stage * BK + 8 * j), lo = *reinterpret_cast<const u32x2*>(xrow + C + stage * BK + 8 * j);
                a[j] = RawA{hi[0], hi[1], lo[0], lo[1]};
            } else {
                a[j] = *reinterpret_cast<const RawA*>(xrow + stage * BK + 8 * j);
            }
        }
    };

    // Software pipeline (one barrier per stage, no exposed LDS latency):
    //   stage s lives in LDS buffer s&1.  B fragments are fetched into registers one 8-channel block AHEAD of the
    //   MFMAs that consume them, so by the time the stage's last block starts every fragment of the stage is in
    //   registers: the barrier sits right there, the freed buffer is refilled for stage s+2, and the first block of
    //   stage s+1 is fetched under the last block's MFMAs.
    f32x4 a_cur[JB];
    RawA a_nxt[JB];
    fill(0, 0);
    if (n_stage > 1) fill(1, 1);
    auto widen_a = [&](f32x4 (&dst)[JB], const RawA (&src)[JB]) {
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            if constexpr (sizeof(TX) == 4) {
                dst[j] = src[j];
            } else {
                const unsigned lo = src[j][0], hi = src[j][1];
                dst[j] = f32x4{__builtin_bit_cast(float, lo << 16), __builtin_bit_cast(float, lo & 0xFFFF0000u),
                               __builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xFFFF0000u)};
                if constexpr (S3) {                                  // + the lo half: the merged value, as s3_load8 forms it
                    const unsigned l0 = src[j][2], l1 = src[j][3];
                    dst[j] += f32x4{__builtin_bit_cast(float, l0 << 16), __builtin_bit_cast(float, l0 & 0xFFFF0000u),
                                    __builtin_bit_cast(float, l1 << 16), __builtin_bit_cast(float, l1 & 0xFFFF0000u)};
                }
            }
        }
    };
    load_a(0, a_nxt);
    widen_a(a_cur, a_nxt);
#pragma unroll
    for (int j = 0; j < JB; ++j) a_nxt[j] = RawA{};
    __syncthreads();                                           // drains vmcnt, then barrier
    TL_STAMP(1)                                                // prologue done: the first MFMA follows

    // B fragment of lane (r, h) for block j, tile t: Bs[buf][2j + h][32 t + r][0..3]
    const float* bs_lane = Bs + (h * CODES + r) * 4;
    f32x4 b_cur[T], b_nxt[T];
#pragma unroll
    for (int t = 0; t < T; ++t) b_cur[t] = *reinterpret_cast<const f32x4*>(bs_lane + t * 128);

    auto mfma_block = [&](int j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = a_cur[j][e];
            xn_part = __builtin_fmaf(a, a, xn_part);
#if VQ_SHAPE16
            // TIMING EXPERIMENT ONLY (results garbage; VERDICT r3 item 2 ii): the same flops as one 32x32x2 per (e, t) issued as TWO
            // v_mfma_f32_16x16x4_f32 on quarters of the accumulator tile, inside the real kernel -- does the chip hold another clock?
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x4 q0 = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]}, q1 = {acc[t][8], acc[t][9], acc[t][10], acc[t][11]};
                q0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_cur[t][e], q0, 0, 0, 0);
                q1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_cur[t][e], q1, 0, 0, 0);
                acc[t][0] = q0[0], acc[t][1] = q0[1], acc[t][2] = q0[2], acc[t][3] = q0[3];
                acc[t][8] = q1[0], acc[t][9] = q1[1], acc[t][10] = q1[2], acc[t][11] = q1[3];
            }
#else
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_cur[t][e], acc[t], 0, 0, 0);
#endif
        }
        // issue order: one LDS read per four MFMAs (the reads belong to the NEXT block and are never waited on here)
#pragma unroll
        for (int t = 0; t < T; ++t) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
    };

    for (int s = 0; s < n_stage; ++s) {
        const float* bsrc = bs_lane + (s & 1) * STAGE_FLOATS;
        if (s + 1 < n_stage) load_a(s + 1, a_nxt);
#pragma unroll
        for (int j = 0; j < JB - 1; ++j) {
#pragma unroll
            for (int t = 0; t < T; ++t)
                b_nxt[t] = *reinterpret_cast<const f32x4*>(bsrc + (2 * (j + 1)) * CODES * 4 + t * 128);
            mfma_block(j);
#pragma unroll
            for (int t = 0; t < T; ++t) b_cur[t] = b_nxt[t];
        }
        __syncthreads();                                       // stage s+1 landed; nobody reads buffer s&1 any more
        if (s + 2 < n_stage) fill(s + 2, s & 1);
        if (s + 1 < n_stage) {
            const float* bnext = bs_lane + ((s + 1) & 1) * STAGE_FLOATS;
#pragma unroll
            for (int t = 0; t < T; ++t) b_nxt[t] = *reinterpret_cast<const f32x4*>(bnext + t * 128);
        }
        mfma_block(JB - 1);
#pragma unroll
        for (int t = 0; t < T; ++t) b_cur[t] = b_nxt[t];
        widen_a(a_cur, a_nxt);
    }

    // |e|^2 of this lane's code in every tile: ONE batch of loads, issued while the last MFMAs drain (the fragment registers of the
    // main loop are dead now; holding these through the loop spilled 67 registers)
    float en[T];
#pragma unroll
    for (int t = 0; t < T; ++t) en[t] = enorm[code0 + t * 32 + r];
    // the clamp's lower bound: 0 for a real code (a NaN distance becomes 0, like the oracle's `d > 0 ? d : 0`), +inf for a padding
    // code K .. Kp - 1.  Padding has zero entries and |e|^2 = +inf, so its distance is +inf for a finite row -- but NaN for a row
    // with a NaN or an Inf (inf * 0), which the clamp to 0 would turn into a winner.  max(d2, +inf) = +inf whatever d2 is.
    float floor_t[T];
#pragma unroll
    for (int t = 0; t < T; ++t) floor_t[t] = code0 + t * 32 + r < g.lv[lvl].K ? 0.0f : __builtin_inff();
    TL_STAMP(2)                                                // main loop issued (the last MFMAs are still draining)
    // ---- epilogue: distances -> (min, code) per row over this workgroup's codes
    {
        const float xn = xn_part + __shfl_xor(xn_part, 32);
        if (h == 0) xn_s[wave * 32 + r] = xn;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): xn_s visible within the wave
    __builtin_amdgcn_wave_barrier();
    float xnr[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xn_s + wave * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) xnr[4 * g + e] = v[e];
    }
    // Running per-lane minimum in SQUARED-distance space.
    float best2[16];
    int best_i[16];
    // Row by row (the 16 rows of a lane are independent; within a row the codes arrive in increasing index order).
    // FAST scan, branch-free: only "clearly better" candidates (below the holder by more than the collapse band 2^-20) move the
    // holder; a candidate inside the band raises `band`.  Without a band event anywhere in the wave the result IS the exact scan's
    // (every decision was a clear one).  With one (rare: two codes within 1e-6 relative of a row's running minimum) the wave redoes
    // that row on the EXACT path: the reference argmins over sqrt(d2), whose rounding can collapse nearly equal d2 into one float --
    // then the LOWER index wins -- so a candidate inside the band compares correctly-rounded square roots, and "keep the holder on
    // a tie" is the tie rule.  One wave-uniform branch per row instead of one per (row, tile); the tiles' |e|^2 come from en[] (they
    // used to be loaded tile by tile behind that branch: eight serialised L2 latencies, 19 us of a 141 us workgroup --
    // profiles/r03_vq_wg_timeline_before.md).
    // The holder starts at the lane's FIRST code with distance +inf: a row whose distances are all +inf (|x|^2 overflows, or a
    // -Inf entry against positive codes) moves no holder, every lane hands its first code to the merge, and the lowest key of the
    // row is (bits(+inf), code 0) -- the oracle's answer.  A padding lane's start code is >= K but loses to that key (code 0 is real
    // and every row gets a key from its lane); for a row with any finite distance nothing changes: a start holder never survives.
    const int code_r = code0 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float b2 = __builtin_inff(), thr = __builtin_inff();
        int bi = code_r;
        bool band = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            float d2 = __builtin_fmaf(-2.0f, acc[t][i], xnr[i]);
            d2 = d2 + en[t];
            d2 = __builtin_fmaxf(d2, floor_t[t]);
            const bool clear = d2 < thr;                                       // better by more than the collapse band
            band = band || (!clear && d2 < b2);                                // inside the band
            bi = clear ? code_r + 32 * t : bi;
            b2 = clear ? d2 : b2;
            thr = clear ? d2 * 0.99999905f : thr;
        }
        if (__builtin_expect(__any(band), 0)) {
            b2 = __builtin_inff();
            thr = __builtin_inff();
            bi = code_r;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                float d2 = __builtin_fmaf(-2.0f, acc[t][i], xnr[i]);
                d2 = d2 + en[t];
                d2 = __builtin_fmaxf(d2, floor_t[t]);
                const bool clear = d2 < thr;
                const bool near = !clear && d2 < b2;
                if (near) {
                    const bool better = __builtin_sqrtf(d2) < __builtin_sqrtf(b2);
                    bi = better ? code_r + 32 * t : bi;
                    b2 = d2;                                                   // same sqrt class or better: safe to lower
                    thr = d2 * 0.99999905f;
                }
                bi = clear ? code_r + 32 * t : bi;
                b2 = clear ? d2 : b2;
                thr = clear ? d2 * 0.99999905f : thr;
            }
        }
        best2[i] = b2;
        best_i[i] = bi;
    }
    TL_STAMP(3)                                                // running minima done (waited on every accumulator)
    // ---- merge the 32 code lanes of each half: keys (float_bits(sqrt d2) << 32 | code) through LDS, 2 lanes per row
    // (the B stage buffers are free: after the last stage barrier every fragment lives in registers)
    unsigned long long* ks = reinterpret_cast<unsigned long long*>(Bs) + wave * (32 * 33);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned long long key =
            ((unsigned long long)__float_as_uint(__builtin_sqrtf(best2[i])) << 32) | (unsigned int)best_i[i];
        ks[(h * 16 + i) * 33 + r] = key;                                       // row (h, i), candidate lane r
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                                        // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    {
        const int rw = lane >> 1, part = lane & 1;                             // rw = h' * 16 + i'
        unsigned long long m = ~0ull;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long v = ks[rw * 33 + part * 16 + j];
            m = v < m ? v : m;
        }
        const unsigned long long o = __shfl_xor(m, 1);
        m = o < m ? o : m;
        const int hh = rw >> 4, ii = rw & 15;
        const long orow = row0 + (ii & 3) + 8 * (ii >> 2) + 4 * hh;
        TL_STAMP(4)
        if (part == 0 && orow < N) atomicMin(keys + orow, m);
    }
#if VQ_TIMELINE
    TL_STAMP(5)
    if (g.tl && threadIdx.x == 0) {
        unsigned long long* o = g.tl + (size_t)blockIdx.x * 16;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            o[2 * k] = tl_rt[k];
            o[2 * k + 1] = tl_ck[k];
        }
        o[12] = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13
        o[13] = __builtin_amdgcn_s_getreg((31 << 11) | 20);     // HW_REG_XCC_ID
        o[14] = (unsigned long long)lvl;
        o[15] = (unsigned long long)row_tile;
    }
#endif
}

#if VQ_TIMELINE
static unsigned long long* g_timeline = nullptr;
#endif

template <int T, typename TX>
static void launch_assign_t(const VqGroup& g, hipStream_t st) {
    constexpr int STAGE_FLOATS = stage_floats(T);
    static_assert((size_t)WAVES * 32 * 33 * sizeof(unsigned long long) <= (2 * STAGE_FLOATS + 256) * sizeof(float), "key scratch aliases the B stages");
    const size_t lds = (size_t)(2 * STAGE_FLOATS + 256 + WAVES * 32) * sizeof(float);
    hipLaunchKernelGGL((vq_assign_f32_kernel<T, TX>), dim3(g.lv[g.n - 1].wg_end), dim3(256), lds, st, g);
}

void launch_assign_levels(const VqLevel* lv, int n, int T, int row_type, hipStream_t st) {
    VqGroup g;
    g.n = n;
    for (int q = 0; q < n; ++q) g.lv[q] = lv[q];
#if VQ_TIMELINE
    g.tl = g_timeline;
#endif
#define VQ_ASSIGN(T_)                                                 \
    if (row_type == VQ_ROWS_S3) launch_assign_t<T_, S3Row>(g, st);    \
    else if (row_type) launch_assign_t<T_, __bf16>(g, st);            \
    else launch_assign_t<T_, float>(g, st)
    switch (T) {
        case 8: VQ_ASSIGN(8); break;
        case 4: VQ_ASSIGN(4); break;
        case 2: VQ_ASSIGN(2); break;
        default: VQ_ASSIGN(1); break;
    }
#undef VQ_ASSIGN
}

}  // namespace vqseg

#if VQ_TIMELINE
// debug build only: device buffer [workgroups][16] u64 the next assign launches write their stamps to (null: off)
extern "C" int vqseg_debug_timeline(void* buf) {
    vqseg::g_timeline = static_cast<unsigned long long*>(buf);
    return 0;
}
#endif
