// Declarations shared by the vector-quantiser units only (vq_assign / vq_filter / vq_tail / vq_codebook / vq_host): the kernel-argument
// structs one unit fills and another launches, the geometry constants both a kernel and a workspace plan read, and the launchers
// vq_host.hip wires together.  Everything other units may call is in vq_kernels.h.
// No struct in this file depends on a build flag, so a unit compiled with -DVQ_TIMELINE / -DVQ_SHAPE16 / -DVQ_BIG_STAGE links with the
// regular objects.  The one struct whose layout does (VqGroup: the timeline pointer) is private to vq_assign.hip.
#pragma once
#include "nn_device.h"        // split-3 rows: S3Row, s3_pack2 (the one pair of split / merge functions of the format)
#include "vq_kernels.h"

namespace vqseg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- geometry (the kernel that owns each constant explains it)
constexpr int ROWS_PER_WG = 128;                            // vq_assign_f32_kernel: 4 waves x 32 pixel rows
constexpr int F_ROWS = 128, F_CODES = 256, F_SUB = 128;      // vq_filter_bf16_kernel: workgroup tile; codes per summary
constexpr int F_LISTS = 64;                                 // sub-lists of a level's candidate pair list (bf16 filter)
constexpr int GATHER_BLOCKS_MAX = 2048;
constexpr int GATHER_ROWS_PER_BLOCK = 16;   // 4 waves x 4 rows in flight
constexpr int KM_RB = 1024;    // rows per block of the histogram / list passes
constexpr int KM_SEG = 128;    // members per segment of the sum pass

// ---- row types of the distance launch (the `x_bf16` / `bf16` argument of the launchers and of the C ABI): fp32 rows [N][C], bf16
// rows [N][C], split-3 rows [N][2C] bf16 = [hi | lo] (nn_device.h).  The logical value of a split-3 element is the fp32 sum
// hi + lo -- what s3_load8 / s3_merge_kernel produce -- and every result is defined by it.
constexpr int VQ_ROWS_F32 = 0, VQ_ROWS_BF16 = 1, VQ_ROWS_S3 = 2;
// the merged value of element c of a split-3 row (hi at [0, C), lo at [C, 2C)): s3_load8's sum, one element
__device__ __forceinline__ float s3_elem(const unsigned short* row, int C, int c) {
    return __builtin_bit_cast(float, (unsigned)row[c] << 16) + __builtin_bit_cast(float, (unsigned)row[C + c] << 16);
}

// ---- one level of the exact distance + argmin launch (vq_assign_f32_kernel)
struct VqLevel {
    const void* x;              // pixel rows [N][C] (f32 or bf16) or [N][2C] (split-3): one type per launch
    const float* E4;            // prepared codebook
    const float* enorm;
    unsigned long long* keys;   // [N] (distance bits << 32 | code), pre-set to ~0
    long N;
    int C, Kp;
    unsigned wg_end;            // exclusive end of this level's workgroup ids in the launch
    // gated mode (the bf16 filter's overflow fallback): the level runs, in full, only if the filter's candidate list overflowed
    // (*gate > gate_cap) -- degenerate codebooks; otherwise every workgroup exits at once
    const int* gate = nullptr;
    int gate_cap = 0;
    int K = 0;                  // real codes: codes K .. Kp - 1 are padding and never win, whatever the row holds (set by the host)
};
// one level of the bf16 candidate filter launch (vq_filter_bf16_kernel)
struct VqFilterLevel {
    const void* x;              // bf16 pixel rows [N][C], or split-3 rows [N][2C] (one type per launch)
    const unsigned short* Eb;   // [2][C / 8][Kp][8] bf16: hi / lo split of the codebook
    const float* enorm;         // |e_k|^2 (the exact kernel's values)
    const float* en_max;        // max_k |e_k|^2
    unsigned long long* summary;// [N][Kp / 128]: (best code | candidate count << 16) << 32 | float bits of the sub-chunk's minimum score
    float* brow;                // [N] band of the row (score space)
    // candidate pairs (row << 32 | code) for the exact re-score: every code inside the band of its sub-chunk's minimum other than
    // that minimum's own code (stage 1), the surviving minima of open rows (stage 2); pair_count[0] counts every append
    // The list is cut into F_LISTS sub-lists (a workgroup appends to sub-list blockIdx % F_LISTS) with a counter each -- thousands of
    // waves adding to ONE address serialise in the L2 atomic unit (measured: +50 us on the filter kernel); pair_count[F_LISTS] is
    // the overflow flag (an append beyond a sub-list's capacity sets it: the gated exact launch then serves the level)
    unsigned long long* pair_rc;
    int* pair_count;
    int pair_cap;               // capacity of ONE sub-list
    unsigned long long* keys;   // [N] the exact kernel's keys (decided rows: written by stage 2; open rows: atomicMin of stage 3)
    const float* W;             // fp32 codebook [K][C] (nullable: the re-score then reads the prepared image E4)
    const float* E4;
    long N;
    int C, Kp;
    unsigned wg_end;            // stage 1 launch: exclusive end of this level's workgroup ids
    unsigned rblk_end;          // stage 2 launch: exclusive end of this level's 256-row blocks
    unsigned sblk_end;          // stage 3 launch: exclusive end of this level's workgroups (a multiple of F_LISTS per level)
};
struct VqFilterGroup {
    VqFilterLevel lv[VQ_MAX_LEVELS];
    int n;
};
// r4: everything a grouped launch wants pre-set, in ONE launch instead of up to three memsets per level (each a launch of its own, in a
// phase where the chip runs nothing else): keys = all ones (the atomicMin identity), the filter's sub-list counters + overflow flag = 0,
// the usage histogram = 0.
struct VqInitLevel {
    unsigned long long* keys;
    long n;
    int* amb;                   // 128 ints, or null
    int* hist;
    int kp;
    unsigned end;               // cumulative workgroup count
};
struct VqInitGroup {
    VqInitLevel lv[VQ_MAX_LEVELS];
    int n;
};

// ---- the parts of a prepared codebook blob (vq_host.hip, next to prepared_layout).  Eb and en_max exist where the candidate filter
// serves the shape; readers take the pointers as const.
struct PreparedView {
    float* E4;
    float* enorm;
    float* en_max;
    unsigned short* Eb;
};
PreparedView prepared_view(const void* prepared, int C, int K);

// ---- launchers one unit offers to vq_host.hip.  Like the kernels' own launches they report nothing: the caller reads hipGetLastError.
// vq_assign.hip: n levels in one launch of vq_assign_f32_kernel<T, float | bf16 | S3Row> (row_type: VQ_ROWS_*); the grid is lv[n - 1].wg_end
void launch_assign_levels(const VqLevel* lv, int n, int T, int row_type, hipStream_t st);
// vq_filter.hip: the filter's image of the codebook (after launch_prepare_exact: reads enorm); the three stages (grids: the last
// level's wg_end / rblk_end / sblk_end); the exact distance of each row's winning code
void launch_prepare_filter(const float* W, int K, int C, int Kp, const float* enorm, unsigned short* Eb, float* en_max, hipStream_t st);
void launch_filter(const VqFilterGroup& fg, int row_type, int force_all, hipStream_t st);      // row_type: VQ_ROWS_BF16 or VQ_ROWS_S3
void launch_exact_dist(const void* x, int row_type, const float* E4, int Kp, const float* enorm, const int64_t* idx, int64_t N, int C, float* dmin,
                       hipStream_t st);
// vq_tail.hip: the pre-set of a grouped launch (grid: the last level's end); keys -> idx / dmin / histogram of level i
void launch_group_init(const VqInitGroup& ig, hipStream_t st);
void launch_unpack_level(int i, const int64_t* N, const int* K, const VqPlan* plans, char* const* ws, int64_t* const* idx,
                         float* const* dmin, hipStream_t st);
// vq_codebook.hip: the exact kernel's image of the codebook and |e_k|^2
void launch_prepare_exact(const float* W, int K, int C, int Kp, float* E4, float* enorm, hipStream_t st);

}  // namespace vqseg
