// vq_filter.hip -- the bf16 candidate filter of the vector quantiser: three stages, its image of the codebook, and the exact distance of
// the winning code.  The arithmetic contract it reproduces is the exact kernel's (vq_assign.hip, file header).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vq_internal.h"

namespace vqseg {

// ------------------------------------------------------------------------------------
// bf16 candidate filter (r4): the distance + argmin of BF16 pixel rows at bf16-MFMA speed with the exact kernel's result.
//
// The rows are exact bf16 values (autocast activations); the fp32 codebook is split e = e_hi + e_lo + rho (bf16 each,
// |rho| <= 2^-18 |e|).  Stage 1 (this kernel) computes approximate scores
//       s~_k = |e_k|^2 - 2 (x . e_hi_k + x . e_lo_k)        on v_mfma_f32_32x32x16_bf16 (fp32 accumulation)
// for a 128-row x 256-code tile per workgroup and leaves, per row and 128-code sub-chunk, the minimum score, its code and the number
// of codes within the row's BAND of that minimum; every further code inside the band goes to a list of candidate pairs.  Stage 2
// (vq_resolve_kernel) takes the minimum over the sub-chunks: a row with exactly ONE code inside the band of the global minimum is
// decided (that code wins under the exact arithmetic too); for every other row the surviving sub-chunks' best codes join the pair
// list.  Stage 3 (vq_rescore_kernel) evaluates the EXACT kernel's fmaf chains for the listed (row, code) pairs on the vector ALU --
// one lane per pair -- and merges them with the exact kernel's own key rule: index AND distance bits are those of the exact chain.
// Whatever share of the rows is open (4 % on well separated codebooks, half of them on the 2048-channel level of an untrained
// network), only their few candidates are re-scored, not their K codes.  A pair list that overflows (degenerate codebooks: more
// than four candidates per row on average) switches the level to the exact kernel on every row (gated launch).
//
// The band.  Let D_k be the exact kernel's squared distance (fl(fl(|x|^2 - 2 dot_chain_k) + |e_k|^2)) and S = sum_i |x_i| |e_ki|
// <= sqrt(|x|^2 max_k |e_k|^2) =: S_max.  Errors against the real value |x|^2 + |e_k|^2 - 2 x.e_k:
//     exact chain of C fmaf's               |dot_chain - x.e| <= C 2^-24 S
//     split residual                         |x.rho|           <= 2^-18 S
//     C / 8 bf16 MFMAs, products exact, each sum of 17 addends aligned to the largest one and truncated below 2^-24 of it
//     (tools/micro/mfma_bf16_rounding.hip: errors up to 2^-23.3 of the magnitude sum on crafted rows, never more than
//      17 * 2^-24 of the largest addend)     |dot~ - x.(e_hi + e_lo)| <= (C / 8) 17 2^-24 S
//     the final roundings of both paths      <= 2^-22 (|x|^2 + |e|^2 + 2 S)
// so |(|x|^2 + s~_k) - D_k| <= eps := 2 (C 2^-24 + 2^-18 + (C / 8) 17 2^-24) S_max + 2^-22 (|x|^2 + E + 2 S_max), E = max |e|^2.
// The reference argmins over sqrt(D): codes whose D differ by less than 2^-20 relative can collapse into one float, the lower index
// wins.  Hence: if D_a <= D_b (1 + 2^-20) then s~_a <= s~_b + 2 eps + 2^-20 (|x|^2 + E + 2 S_max) =: BAND (x 1.25 for margin).
// Any code that can win or tie under the exact arithmetic lies within BAND of the approximate minimum.
//
// Split-3 rows (row type VQ_ROWS_S3, the template argument S3): a row is [hi | lo], two bf16 values per channel (nn_device.h), and
// its logical value is x = fl(hi + lo), the fp32 sum s3_merge_kernel writes.  hi and lo ARE bf16 MFMA operands, so stage 1 issues
//       s~_k = |e_k|^2 - 2 (x_hi . e_hi_k + x_hi . e_lo_k + x_lo . e_hi_k)
// into the same accumulators (the LDS stage of Eb is read once for both row halves) and leaves out x_lo . e_lo -- a fourth product
// would cost a third more MFMA time to remove a term that is a tenth of the band at C = 512 and less above (the truncation term
// below dominates); stages 2 and 3 are row-type blind resp. read the merged value.  The band, term by term, S as above with |x| = |hi + lo|:
//     exact chain of C fmaf's on the merged row            |dot_chain - x.e| <= C 2^-24 S                      (as for bf16 rows)
//     the merge rounds once: x = (hi + lo)(1 + d), |d| <= 2^-24 (d = 0 for rows s3_store8 wrote from an fp32 value: hi + lo is then
//     a multiple of that value's ulp below twice its binade; rows handed in through the ABI need not be)    <= 2^-24 S
//     split residual of the codebook, |rho| <= 2^-16 |e|: hi = RN_bf16(e) leaves |e - hi| <= half an ulp of 8 significant bits
//     <= 2^-8 |e| (attained just above a power of two), lo = RN_bf16(e - hi) leaves 2^-8 of that          |x.rho| <= 2^-16 S
//     the dropped product: s3_store8 rounds hi = RN_bf16(v) (s3_pack2: the (__bf16) conversion, round to nearest even) and
//     lo = RN_bf16(v - hi), v - hi exact in fp32, so |x_lo| <= 2^-8 |v| and |v| <= |x| (1 + 2^-15); with |e_lo| <= 2^-8 |e|
//                                                           |x_lo . e_lo| <= 2^-16 S (1 + 2^-15)
//       (NOT 2^-18 S: v = 1 + 2^-8 - 2^-23 splits into hi = 1, lo = 2^-8 - 2^-16; the margin factor absorbs the 2^-15)
//     3 C / 16 bf16 MFMAs (three per 16 channels), each as above                      |dot~ - (the three products)| <= (3 C / 16) 17 2^-24 S
//     |x|^2 of the band: the fp32 sum of squares of the merged values (the exact kernel's operand), the final roundings as above
// so eps_S3 = 2 (C 2^-24 + 2^-24 + 2^-16 + 2^-16 + (3 C / 16) 17 2^-24) S_max + 2^-22 (|x|^2 + E + 2 S_max), BAND as above from eps_S3.
//
// Roles are swapped against the exact kernel: codes are the MFMA's M dimension (LDS, staged by LDS-DMA), pixels the N dimension
// (registers, straight from global in fragment shape), so that a lane owns ONE pixel per fragment and the minimum / band count over
// its codes needs no cross-lane traffic (the two half-waves meet in one shuffle).
// Workgroup: 4 waves = 2 (64 pixels) x 2 (128 codes); wave tile = 2 pixel fragments x 4 code tiles = 8 accumulators.
// ------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int F_BK = 32;                                   // channels per LDS stage (two MFMA K steps)
constexpr int F_STAGE_BYTES = 2 * (F_BK / 8) * F_CODES * 16; // [hi | lo][4 slabs of 8 channels][256 codes][8 bf16] = 32 KiB

__device__ __forceinline__ void glds16b(const void* g, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lds_wave_base,
                                     16, 0, 0);
}

// exclusive prefix sum of v over the 64 lanes; total = the wave's sum
__device__ __forceinline__ int wave_excl_scan(int v, int& total) {
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if ((int)(threadIdx.x & 63) >= d) inc += o;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

struct FilterConsts {
    float c_s, c_r;             // BAND = c_s * sqrt(|x|^2 * E) + c_r * (|x|^2 + E)   (per level: depends on C)
};

template <bool S3>
__global__ __launch_bounds__(256, 2) void vq_filter_bf16_kernel(const VqFilterGroup g, const FilterConsts fc0, const FilterConsts fc1,
                                                                const FilterConsts fc2, const FilterConsts fc3) {
    constexpr int NH = S3 ? 2 : 1;                              // bf16 fragments per channel of a row: hi, and lo of a split-3 row
    int lvl = 0;
    while (lvl + 1 < g.n && blockIdx.x >= g.lv[lvl].wg_end) ++lvl;
    const unsigned bid = blockIdx.x - (lvl ? g.lv[lvl - 1].wg_end : 0u);
    const FilterConsts fc = lvl == 0 ? fc0 : (lvl == 1 ? fc1 : (lvl == 2 ? fc2 : fc3));
    const unsigned short* __restrict__ x = static_cast<const unsigned short*>(g.lv[lvl].x);
    const unsigned short* __restrict__ Eb = g.lv[lvl].Eb;
    const long N = g.lv[lvl].N;
    const int C = g.lv[lvl].C, Kp = g.lv[lvl].Kp;
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    char* Bs = fsm;                                             // [2 buffers][F_STAGE_BYTES]
    float* en_s = reinterpret_cast<float*>(fsm + 2 * F_STAGE_BYTES);   // [F_CODES]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave & 1, wc = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const int n_stage = C / F_BK;
    // workgroup id -> (row tile, code chunk): the chunks of a row tile sit 8 ids apart = same XCD, about the same time (see the exact kernel)
    const int chunks = Kp / F_CODES;
    const unsigned within = bid % (8u * chunks);
    const long row_tile = (long)(bid / (8u * chunks)) * 8 + (within & 7u);
    if (row_tile * F_ROWS >= N) return;
    const int chunk = (int)(within >> 3);
    const int code0 = chunk * F_CODES;

    en_s[tid] = g.lv[lvl].enorm[code0 + tid];                   // 256 threads, 256 codes

    const unsigned short* xrow[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        long row = row_tile * F_ROWS + wp * 64 + p * 32 + r;
        if (row > N - 1) row = N - 1;
        xrow[p] = x + row * (long)(NH * C) + 8 * h;              // split-3: the lo half of the row starts C elements further
    }

    f32x16 acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[p][t][i] = 0.0f;
    float xn_part[2] = {0.0f, 0.0f};

    // stage fill: 32 wave-instructions of 1 KiB (64 codes x 16 B of one (hi|lo, slab)), 8 per wave
    auto fill = [&](int stage, int buf) {
        char* dst = Bs + buf * F_STAGE_BYTES;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int piece = wave * 8 + q;
            const int hlslab = piece >> 2, quarter = piece & 3;
            const int hl = hlslab >> 2, slab = hlslab & 3;
            const unsigned short* src = Eb + (((size_t)hl * (C / 8) + (size_t)stage * 4 + slab) * Kp + code0 + quarter * 64 + lane) * 8;
            glds16b(src, dst + (hlslab * F_CODES + quarter * 64) * 16);
        }
    };
    auto load_x = [&](int stage, u32x4 (&xf)[2][2][NH]) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int w = 0; w < NH; ++w) xf[p][q][w] = *reinterpret_cast<const u32x4*>(xrow[p] + w * C + stage * F_BK + q * 16);
    };

    u32x4 xcur[2][2][NH], xnxt[2][2][NH];
    fill(0, 0);
    if (n_stage > 1) fill(1, 1);
    load_x(0, xcur);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int w = 0; w < NH; ++w) xnxt[p][q][w] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    const char* a_lane = Bs + ((h * F_CODES) + wc * 128 + r) * 16;     // + buf * STAGE + ((hl * 4 + 2 q) * F_CODES + 32 t) * 16
    for (int s = 0; s < n_stage; ++s) {
        const char* abase = a_lane + (s & 1) * F_STAGE_BYTES;
        if (s + 1 < n_stage) load_x(s + 1, xnxt);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            bf16x8 ah[4], al[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                ah[t] = *reinterpret_cast<const bf16x8*>(abase + ((0 * 4 + 2 * q) * F_CODES + 32 * t) * 16);
                al[t] = *reinterpret_cast<const bf16x8*>(abase + ((1 * 4 + 2 * q) * F_CODES + 32 * t) * 16);
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const bf16x8 xb = __builtin_bit_cast(bf16x8, xcur[p][q][0]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {                     // |x|^2 of this lane's 8 channels (fp32; only the band needs it)
                    float lo = __builtin_bit_cast(float, xcur[p][q][0][e] << 16), hi = __builtin_bit_cast(float, xcur[p][q][0][e] & 0xFFFF0000u);
                    if constexpr (S3) {                           // of the merged values, as s3_load8 forms them
                        lo += __builtin_bit_cast(float, xcur[p][q][NH - 1][e] << 16);
                        hi += __builtin_bit_cast(float, xcur[p][q][NH - 1][e] & 0xFFFF0000u);
                    }
                    xn_part[p] = __builtin_fmaf(lo, lo, xn_part[p]);
                    xn_part[p] = __builtin_fmaf(hi, hi, xn_part[p]);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], xb, acc[p][t], 0, 0, 0);
                    acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], xb, acc[p][t], 0, 0, 0);
                }
                if constexpr (S3) {                               // x_lo . e_hi (x_lo . e_lo is left to the band)
                    const bf16x8 xl = __builtin_bit_cast(bf16x8, xcur[p][q][NH - 1]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], xl, acc[p][t], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                        // stage s + 1 landed (issued a whole stage ago); buffer s & 1 is free
        if (s + 2 < n_stage) fill(s + 2, s & 1);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int w = 0; w < NH; ++w) xcur[p][q][w] = xnxt[p][q][w];
    }

    // ---- epilogue: scores of this lane's 64 codes per pixel fragment, minimum, band count
    const float en_max = *g.lv[lvl].en_max;
    const int sub = chunk * 2 + wc, n_sub = Kp / F_SUB;
    const float* en_l = en_s + wc * 128 + 4 * h;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float m = __builtin_inff();
        int bi = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x4 en4 = *reinterpret_cast<const f32x4*>(en_l + 32 * t + 8 * gq);    // codes 32 t + 8 gq + 4 h + (0..3): same address in a half-wave
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sc = __builtin_fmaf(-2.0f, acc[p][t][4 * gq + e], en4[e]);
                    acc[p][t][4 * gq + e] = sc;
                    const bool better = sc < m;                   // codes arrive in increasing index order: the first minimum is kept
                    bi = better ? 32 * t + 8 * gq + e : bi;
                    m = better ? sc : m;
                }
            }
        bi += 4 * h;
        {   // the other half-wave holds the other 64 codes of this pixel
            const float mo = __shfl_xor(m, 32);
            const int bo = __shfl_xor(bi, 32);
            const bool take = mo < m || (mo == m && bo < bi);
            m = take ? mo : m;
            bi = take ? bo : bi;
        }
        const float xn = xn_part[p] + __shfl_xor(xn_part[p], 32);
        const float band = __builtin_fmaf(fc.c_s, __builtin_sqrtf(xn * en_max), fc.c_r * (xn + en_max));
        const float thr = m + band;
        // which of this half-wave's 64 codes lie inside the band: bit 16 t + i of (lo, hi) <-> acc[p][t][i]
        unsigned lo = 0u, hi = 0u;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) lo |= acc[p][t][i] <= thr ? (1u << (16 * t + i)) : 0u;
#pragma unroll
        for (int t = 2; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) hi |= acc[p][t][i] <= thr ? (1u << (16 * (t - 2) + i)) : 0u;
        const int mine = __popc(lo) + __popc(hi);
        const int cnt = mine + __shfl_xor(mine, 32);
        const long row = row_tile * F_ROWS + wp * 64 + p * 32 + r;
        const bool live = row < N;
        if (h == 0 && live) {
            const unsigned hiw = (unsigned)(code0 + wc * 128 + bi) | ((unsigned)(cnt > 0xffff ? 0xffff : cnt) << 16);
            g.lv[lvl].summary[row * n_sub + sub] = ((unsigned long long)hiw << 32) | __float_as_uint(m);
            if (sub == 0) g.lv[lvl].brow[row] = band;
        }
        // candidates beyond the best code -> the pair list (one reservation per wave; only lanes that have any walk their bits)
        if ((bi & 4) == 4 * h) {                                  // the best code sits in this half-wave: clear its bit
            const int bb = 16 * (bi >> 5) + 4 * ((bi >> 3) & 3) + (bi & 3);
            if (bb < 32) lo &= ~(1u << bb);
            else hi &= ~(1u << (bb - 32));
        }
        const int extra = live ? __popc(lo) + __popc(hi) : 0;
        if (__any(extra > 0)) {                                   // wave-uniform
            int total;
            const int before = wave_excl_scan(extra, total);
            const int list = blockIdx.x & (F_LISTS - 1), cap = g.lv[lvl].pair_cap;
            int base = 0;
            if (lane == 0) {
                base = atomicAdd(g.lv[lvl].pair_count + list, total);
                if (base + total > cap) g.lv[lvl].pair_count[F_LISTS] = 1;       // overflow: the gated exact launch serves the level
            }
            base = __shfl(base, 0);
            if (extra > 0) {
                int slot = base + before;
                unsigned long long* out = g.lv[lvl].pair_rc + (size_t)list * cap;
                unsigned long long bits = ((unsigned long long)hi << 32) | lo;
                while (bits) {
                    const int b = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const int cl = 32 * (b >> 4) + 8 * ((b >> 2) & 3) + 4 * h + (b & 3);
                    if (slot < cap) out[slot] = ((unsigned long long)row << 32) | (unsigned)(code0 + wc * 128 + cl);
                    ++slot;
                }
            }
        }
    }
}

// Stage 2 (all levels of the launch): per row the minimum over its sub-chunk summaries; exactly one code inside the band -> decided
// (key written directly, the row's threshold word set to -inf: its listed candidates are skipped); otherwise the best code of every
// surviving sub-chunk joins the pair list and brow keeps +inf-free "open" (the threshold itself).
constexpr int F_MAX_SUB = 16;                               // sub-chunk summaries a row can have in registers (K <= 2048); more: re-read
__global__ __launch_bounds__(256) void vq_resolve_kernel(const VqFilterGroup g, int force_all) {
    int lvl = 0;
    while (lvl + 1 < g.n && blockIdx.x >= g.lv[lvl].rblk_end) ++lvl;
    const VqFilterLevel& L = g.lv[lvl];
    const long N = L.N;
    const int n_sub = L.Kp / F_SUB;
    long row = (long)(blockIdx.x - (lvl ? g.lv[lvl - 1].rblk_end : 0u)) * 256 + threadIdx.x;
    const bool valid = row < N;
    if (!valid) row = N - 1;                                   // keep the wave whole for the scan below
    const unsigned long long* sm = L.summary + row * n_sub;
    unsigned long long v[F_MAX_SUB];
#pragma unroll
    for (int j = 0; j < F_MAX_SUB; j += 2)
        if (j < n_sub) {                                        // n_sub is even (K % 256 == 0): 16-byte loads
            const u32x4 w = *reinterpret_cast<const u32x4*>(sm + j);
            v[j] = ((unsigned long long)w[1] << 32) | w[0];
            v[j + 1] = ((unsigned long long)w[3] << 32) | w[2];
        }
    float m = __builtin_inff();
    unsigned best = 0;
#pragma unroll
    for (int j = 0; j < F_MAX_SUB; ++j)
        if (j < n_sub) {
            const float mj = __uint_as_float((unsigned)(v[j] & 0xffffffffull));
            const unsigned cj = (unsigned)(v[j] >> 32) & 0xffffu;
            if (mj < m || (mj == m && cj < best)) m = mj, best = cj;
        }
    for (int j = F_MAX_SUB; j < n_sub; ++j) {                   // K > 2048
        const float mj = __uint_as_float((unsigned)(sm[j] & 0xffffffffull));
        const unsigned cj = (unsigned)(sm[j] >> 32) & 0xffffu;
        if (mj < m || (mj == m && cj < best)) m = mj, best = cj;
    }
    const float thr = m + L.brow[row];
    unsigned cnt = 0;
    int alive = 0;
#pragma unroll
    for (int j = 0; j < F_MAX_SUB; ++j)
        if (j < n_sub && __uint_as_float((unsigned)(v[j] & 0xffffffffull)) <= thr) cnt += (unsigned)(v[j] >> 48), ++alive;
    for (int j = F_MAX_SUB; j < n_sub; ++j)
        if (__uint_as_float((unsigned)(sm[j] & 0xffffffffull)) <= thr) cnt += (unsigned)(sm[j] >> 48), ++alive;
    // Non-finite rows and codebooks.  A NaN score is never below a minimum nor inside a band, so a row with a NaN / Inf entry, a
    // row whose |x|^2 overflows, or any row under a codebook with a non-finite |e_k|^2 (en_max, hence the band) would end "open"
    // with no candidate -- its key never written.  Every such row has a threshold that is not finite (m = +-inf / NaN, or band =
    // inf / NaN; the band holds |x|^2 and en_max).  Chosen remedy: it sets the overflow flag pair_count[F_LISTS], i.e. the level
    // goes to the gated exact launch, which writes the exact kernel's key for every row (the other option, writing that key here,
    // would repeat the exact chain in this kernel).  Costs the filter's speed only while non-finite values are present.
    const bool bad = valid && !(__builtin_fabsf(thr) < __builtin_inff());
    if (__any(bad) && (threadIdx.x & 63) == 0) L.pair_count[F_LISTS] = 1;
    const bool open = valid && (bad || !(cnt == 1 && !force_all));
    if (valid) {
        if (!open) L.keys[row] = (unsigned long long)best;    // distance word 0: decided rows carry no exact distance (see vq_exact_dist_kernel)
        L.brow[row] = open ? thr : -__builtin_inff();
    }
    if (!__any(open)) return;
    int total;
    const int before = wave_excl_scan(open ? alive : 0, total);
    const int list = blockIdx.x & (F_LISTS - 1), cap = L.pair_cap;
    int base = 0;
    if ((threadIdx.x & 63) == 0) {
        base = atomicAdd(L.pair_count + list, total);
        if (base + total > cap) L.pair_count[F_LISTS] = 1;
    }
    base = __shfl(base, 0);
    if (open) {
        int slot = base + before;
        unsigned long long* out = L.pair_rc + (size_t)list * cap;
        for (int j = 0; j < n_sub; ++j) {
            const unsigned long long vj = sm[j];
            if (__uint_as_float((unsigned)(vj & 0xffffffffull)) <= thr) {
                if (slot < cap) out[slot] = ((unsigned long long)row << 32) | ((unsigned)(vj >> 32) & 0xffffu);
                ++slot;
            }
        }
    }
}

// Stage 3 (all levels): the exact kernel's arithmetic for the listed (row, code) pairs of OPEN rows, one lane per pair: dot = the
// "mfma8" fmaf chain, |x|^2 its two half chains, |e|^2 from the prepared blob, d = sqrt(max(fmaf(-2, dot, |x|^2) + |e|^2, 0)),
// key = (bits(d) << 32) | code merged by atomicMin like the exact kernel's code groups (the lowest code wins a tie).
template <bool S3>
struct RescoreTrip {                                        // 32 channels of one (row, code) pair
    u32x4 xw[4][S3 ? 2 : 1];                                // split-3 rows: [hi, lo], merged where the chain reads them
    f32x4 e0[4], e1[4];
};

template <bool ROWMAJOR, bool S3>
__device__ __forceinline__ void rescore_load(RescoreTrip<S3>& t, const unsigned short* xr, const float* er, int c, int Kp, int C) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        t.xw[u][0] = *reinterpret_cast<const u32x4*>(xr + c + 8 * u);
        if constexpr (S3) t.xw[u][1] = *reinterpret_cast<const u32x4*>(xr + C + c + 8 * u);
        if (ROWMAJOR) {
            t.e0[u] = *reinterpret_cast<const f32x4*>(er + c + 8 * u);
            t.e1[u] = *reinterpret_cast<const f32x4*>(er + c + 8 * u + 4);
        } else {                                                // prepared image: 4-channel groups Kp * 16 bytes apart
            t.e0[u] = *reinterpret_cast<const f32x4*>(er + (size_t)((c + 8 * u) / 4) * Kp * 4);
            t.e1[u] = *reinterpret_cast<const f32x4*>(er + (size_t)((c + 8 * u) / 4 + 1) * Kp * 4);
        }
    }
}

template <bool S3>
__device__ __forceinline__ void rescore_fma(const RescoreTrip<S3>& t, float& dot, float& xa, float& xb) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float xv[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xv[2 * e] = __builtin_bit_cast(float, t.xw[u][0][e] << 16);
            xv[2 * e + 1] = __builtin_bit_cast(float, t.xw[u][0][e] & 0xFFFF0000u);
            if constexpr (S3) {                                   // the merged value (s3_load8)
                xv[2 * e] += __builtin_bit_cast(float, t.xw[u][1][e] << 16);
                xv[2 * e + 1] += __builtin_bit_cast(float, t.xw[u][1][e] & 0xFFFF0000u);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dot = __builtin_fmaf(xv[e], t.e0[u][e], dot);
            dot = __builtin_fmaf(xv[4 + e], t.e1[u][e], dot);
            xa = __builtin_fmaf(xv[e], xv[e], xa);
            xb = __builtin_fmaf(xv[4 + e], xv[4 + e], xb);
        }
    }
}

// one sub-list of one level: lane i takes pairs i, i + nthreads, ...; a chain is serial (C dependent fmaf's), so its loads run two
// 32-channel trips ahead of the arithmetic
template <bool ROWMAJOR, bool S3>
__device__ __forceinline__ void rescore_pairs(const VqFilterLevel& L, int list, int tid, int nthreads) {
    int n = L.pair_count[list];
    if (n > L.pair_cap) n = L.pair_cap;                        // overflow: the gated exact launch serves the level anyway
    const int C = L.C, Kp = L.Kp;
    const unsigned short* __restrict__ x = static_cast<const unsigned short*>(L.x);
    const unsigned long long* pairs = L.pair_rc + (size_t)list * L.pair_cap;
    for (int i = tid; i < n; i += nthreads) {
        const unsigned long long rc = pairs[i];
        const long row = (long)(rc >> 32);
        const unsigned k = (unsigned)(rc & 0xffffffffull);
        if (L.brow[row] == -__builtin_inff()) continue;         // a decided row
        const unsigned short* xr = x + row * (long)(S3 ? 2 * C : C);
        const float* er = ROWMAJOR ? L.W + (size_t)k * C : L.E4 + (size_t)k * 4;
        float dot = 0.0f, xa = 0.0f, xb = 0.0f;
        RescoreTrip<S3> t0, t1, t2;                              // C % 32 == 0 on this path
        rescore_load<ROWMAJOR>(t0, xr, er, 0, Kp, C);
        if (C > 32) rescore_load<ROWMAJOR>(t1, xr, er, 32, Kp, C);
        int c = 0;
        for (; c + 96 <= C; c += 96) {
            if (c + 64 < C) rescore_load<ROWMAJOR>(t2, xr, er, c + 64, Kp, C);
            rescore_fma(t0, dot, xa, xb);
            if (c + 96 < C) rescore_load<ROWMAJOR>(t0, xr, er, c + 96, Kp, C);
            rescore_fma(t1, dot, xa, xb);
            if (c + 128 < C) rescore_load<ROWMAJOR>(t1, xr, er, c + 128, Kp, C);
            rescore_fma(t2, dot, xa, xb);
        }
        if (c < C) {                                            // one or two trips left (already loaded into t0 / t1)
            rescore_fma(t0, dot, xa, xb);
            if (c + 32 < C) rescore_fma(t1, dot, xa, xb);
        }
        float d2 = __builtin_fmaf(-2.0f, dot, xa + xb) + L.enorm[k];
        d2 = __builtin_fmaxf(d2, 0.0f);
        atomicMin(L.keys + row, ((unsigned long long)__float_as_uint(__builtin_sqrtf(d2)) << 32) | k);
    }
}

// Stage 3 launch: every level gets its own workgroups (a multiple of F_LISTS), workgroup b of a level serves sub-list b % F_LISTS
template <bool S3>
__global__ __launch_bounds__(256) void vq_rescore_kernel(const VqFilterGroup g) {
    int lvl = 0;
    while (lvl + 1 < g.n && blockIdx.x >= g.lv[lvl].sblk_end) ++lvl;
    const unsigned first = lvl ? g.lv[lvl - 1].sblk_end : 0u;
    const unsigned b = blockIdx.x - first, per_list = (g.lv[lvl].sblk_end - first) / F_LISTS;
    const int list = (int)(b % F_LISTS), tid = (int)(b / F_LISTS) * 256 + threadIdx.x, nthreads = (int)per_list * 256;
    if (g.lv[lvl].W) rescore_pairs<true, S3>(g.lv[lvl], list, tid, nthreads);
    else rescore_pairs<false, S3>(g.lv[lvl], list, tid, nthreads);
}

// The exact kernel's distance of ONE given code per row on the vector ALU (tests ask for the winning distance; rows the filter
// decided never went through the exact kernel): the same fmaf chains in the same order (file header, "mfma8").
template <bool S3>
__global__ __launch_bounds__(256) void vq_exact_dist_kernel(const unsigned short* __restrict__ x, const float* __restrict__ E4, int Kp,
                                                            const float* __restrict__ enorm, const long long* __restrict__ idx, long N, int C,
                                                            float* __restrict__ dmin) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    const unsigned short* xr = x + row * (long)(S3 ? 2 * C : C);
    const long long k = idx[row];
    float dot = 0.0f, xa = 0.0f, xb = 0.0f;
    for (int c = 0; c + 8 <= C; c += 8) {
        float xv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = S3 ? s3_elem(xr, C, c + e) : __builtin_bit_cast(float, (unsigned)xr[c + e] << 16);
        const f32x4 e0 = *reinterpret_cast<const f32x4*>(E4 + ((size_t)(c / 4) * Kp + k) * 4);          // channels c .. c + 3 of code k
        const f32x4 e1 = *reinterpret_cast<const f32x4*>(E4 + ((size_t)(c / 4 + 1) * Kp + k) * 4);      // channels c + 4 .. c + 7
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dot = __builtin_fmaf(xv[e], e0[e], dot);
            dot = __builtin_fmaf(xv[4 + e], e1[e], dot);
            xa = __builtin_fmaf(xv[e], xv[e], xa);
            xb = __builtin_fmaf(xv[4 + e], xv[4 + e], xb);
        }
    }
    float d2 = __builtin_fmaf(-2.0f, dot, xa + xb) + enorm[k];
    d2 = __builtin_fmaxf(d2, 0.0f);
    dmin[row] = __builtin_sqrtf(d2);
}

// bf16 hi / lo split of the codebook for the candidate filter: Eb[hl][c / 8][k][8]  (hl = 0: bf16(e), 1: bf16(e - hi)); zero for
// k >= K.  One thread per (c8, k): two 16-byte loads, two 16-byte stores.
__global__ __launch_bounds__(256) void vq_pack_codebook_bf16(const float* __restrict__ W, int K, int C, int Kp, unsigned short* __restrict__ Eb) {
    const long total = (long)(C / 8) * Kp;
    const size_t half = (size_t)C * Kp;                          // elements per (hi | lo) image
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k = (int)(i % Kp);
        const int c = (int)(i / Kp) * 8;
        u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
        if (k < K) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(W + (size_t)k * C + c), v1 = *reinterpret_cast<const f32x4*>(W + (size_t)k * C + c + 4);
            const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 h0 = (__bf16)v[2 * e], h1 = (__bf16)v[2 * e + 1];
                const __bf16 l0 = (__bf16)(v[2 * e] - (float)h0), l1 = (__bf16)(v[2 * e + 1] - (float)h1);
                hi[e] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
                lo[e] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
            }
        }
        *reinterpret_cast<u32x4*>(Eb + (size_t)i * 8) = hi;
        *reinterpret_cast<u32x4*>(Eb + half + (size_t)i * 8) = lo;
    }
}

// the larger of two values, NaN if either is one (fmaxf would drop it)
__device__ __forceinline__ float max_keep_nan(float a, float b) { return a != a ? a : (!(b <= a) ? b : a); }

// max_k |e_k|^2 over the real codes (one workgroup; the padding entries of enorm are +inf).  A NaN or +inf |e_k|^2 (a code with a
// non-finite entry, or one whose norm overflows) REACHES the result: the filter's band is then not finite and vq_resolve_kernel
// hands the level to the exact kernel -- the filter has no error bound for such a code and must not rank it.
__global__ __launch_bounds__(256) void vq_enorm_max(const float* __restrict__ enorm, int K, float* __restrict__ out) {
    __shared__ float sh[256];
    float m = 0.0f;
    for (int k = threadIdx.x; k < K; k += 256) m = max_keep_nan(m, enorm[k]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = max_keep_nan(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ------------------------------------------------------------------------------------
// launchers (called by vq_host.hip)
// ------------------------------------------------------------------------------------
void launch_prepare_filter(const float* W, int K, int C, int Kp, const float* enorm, unsigned short* Eb, float* en_max, hipStream_t st) {
    long b2 = ((long)(C / 8) * Kp + 255) / 256;
    if (b2 > 4096) b2 = 4096;
    hipLaunchKernelGGL(vq_pack_codebook_bf16, dim3((unsigned)b2), dim3(256), 0, st, W, K, C, Kp, Eb);
    hipLaunchKernelGGL(vq_enorm_max, dim3(1), dim3(256), 0, st, enorm, K, en_max);
}

void launch_filter(const VqFilterGroup& fg, int row_type, int force_all, hipStream_t st) {
    const bool s3 = row_type == VQ_ROWS_S3;
    FilterConsts fc[VQ_MAX_LEVELS] = {};
    for (int q = 0; q < fg.n; ++q) {
        // BAND = 1.25 * [ 2 eps + 2^-20 (|x|^2 + E + 2 S) ],  eps = 2 (C 2^-24 + 2^-18 + (C / 8) 17 2^-24) S + 2^-22 (|x|^2 + E + 2 S),
        // S = sqrt(|x|^2 E); split-3 rows: eps = 2 (C 2^-24 + 2^-24 + 2^-16 + 2^-16 + (3 C / 16) 17 2^-24) S + the same tail
        // (both derivations at vq_filter_bf16_kernel)
        const double u = ldexp(1.0, -24), cc = (double)fg.lv[q].C;
        const double per_s = s3 ? 2.0 * (cc * u + u + 2.0 * ldexp(1.0, -16) + (3.0 * cc / 16.0) * 17.0 * u)
                                : 2.0 * (cc * u + ldexp(1.0, -18) + (cc / 8.0) * 17.0 * u);
        const double tail = 2.0 * ldexp(1.0, -22) + ldexp(1.0, -20);
        fc[q].c_s = (float)(1.25 * (2.0 * per_s + 2.0 * tail));
        fc[q].c_r = (float)(1.25 * tail);
    }
    const VqFilterLevel& last = fg.lv[fg.n - 1];
    const size_t lds = (size_t)(2 * F_STAGE_BYTES + F_CODES * sizeof(float));
    if (s3) hipLaunchKernelGGL(vq_filter_bf16_kernel<true>, dim3(last.wg_end), dim3(256), lds, st, fg, fc[0], fc[1], fc[2], fc[3]);
    else hipLaunchKernelGGL(vq_filter_bf16_kernel<false>, dim3(last.wg_end), dim3(256), lds, st, fg, fc[0], fc[1], fc[2], fc[3]);
    hipLaunchKernelGGL(vq_resolve_kernel, dim3(last.rblk_end), dim3(256), 0, st, fg, force_all);
    if (s3) hipLaunchKernelGGL(vq_rescore_kernel<true>, dim3(last.sblk_end), dim3(256), 0, st, fg);
    else hipLaunchKernelGGL(vq_rescore_kernel<false>, dim3(last.sblk_end), dim3(256), 0, st, fg);
}

void launch_exact_dist(const void* x, int row_type, const float* E4, int Kp, const float* enorm, const int64_t* idx, int64_t N, int C,
                       float* dmin, hipStream_t st) {
    const dim3 grid((unsigned)((N + 255) / 256));
    const unsigned short* xr = static_cast<const unsigned short*>(x);
    const long long* ix = reinterpret_cast<const long long*>(idx);
    if (row_type == VQ_ROWS_S3) hipLaunchKernelGGL(vq_exact_dist_kernel<true>, grid, dim3(256), 0, st, xr, E4, Kp, enorm, ix, (long)N, C, dmin);
    else hipLaunchKernelGGL(vq_exact_dist_kernel<false>, grid, dim3(256), 0, st, xr, E4, Kp, enorm, ix, (long)N, C, dmin);
}

}  // namespace vqseg
