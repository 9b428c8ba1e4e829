// Launch-helper declarations of the vector quantiser that the C ABI files call (the VQ units themselves share vq_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vqseg {

constexpr int VQ_MAX_LEVELS = 4;

struct VqPlan {
    int Cp, Kp;                 // channels; codes padded to a multiple of 32
    int T;                      // accumulator tiles (32 codes each) per wave chosen for this shape
    size_t off_prepared, off_keys, off_hist, off_partial, bytes;
    int gather_blocks;
    // bf16 candidate filter (r4): per (row, 128-code sub-chunk) summaries, per-row band / threshold, candidate pair list (its counter
    // first: off_amb), pair capacity
    size_t off_summary, off_brow, off_amb, off_pair_rc;
    int pair_cap;
};
// Layout of the prepared codebook blob: [E4: C * Kp f32][enorm: Kp f32][en_max: 64 f32 (first one used)][Eb: 2 * C * Kp bf16]
// (Eb = the bf16 hi / lo split of the codebook for the candidate filter: [hl][C / 8][Kp][8]); every part 256-byte aligned.
struct PreparedLayout {
    size_t off_e4, off_enorm, off_enmax, off_eb, bytes;
};
PreparedLayout prepared_layout(int C, int K);
int vq_set_option(const char* key, int value);              // returns the previous value, -1: unknown key / bad value
struct KmPlan {
    VqPlan vq;
    size_t off_idx, off_counts, off_offsets, off_members, off_sums, off_counts64, off_hist, off_segoff, off_partial, bytes;
    int row_blocks, max_segments;
};

hipError_t profile_begin(int capacity);
void profile_release();
int profile_collect(int max_records, int64_t* n, int* c, int* k, float* ms, int* kind);

VqPlan vq_plan(int64_t N, int C, int K);
KmPlan km_plan(int64_t N, int C, int K);

size_t prepared_bytes(int C, int K);
hipError_t launch_prepare(const float* W, int K, int C, void* prepared, hipStream_t st);
// `codebook(s)` (nullable): the fp32 [K][C] weight the prepared blob was built from -- the bf16 filter's re-score reads contiguous
// code rows from it instead of the strided prepared image
hipError_t launch_assign(const void* x, int x_bf16, int64_t N, int C, int K, const void* prepared, const VqPlan& p, char* ws,
                         int64_t* idx, float* dmin, hipStream_t st, const float* codebook = nullptr);
int vq_group_tiles(int n, const int64_t* N, const int* K);
hipError_t launch_assign_group(int n, const void* const* x, int x_bf16, const int64_t* N, const int* C, const int* K,
                               const void* const* prepared, const VqPlan* plans, char* const* ws, int64_t* const* idx,
                               float* const* dmin, int T, hipStream_t st, const float* const* codebooks = nullptr);
hipError_t launch_gather(const void* x, int bf16, const float* W, const int64_t* idx, int64_t N, int C, int K, int training,
                         float cw, const VqPlan& p, char* ws, void* quant, float* loss, float* dead, hipStream_t st);
hipError_t launch_backward(const float* gq, const float* gloss, const float* x, const float* q, int64_t N, int C,
                           float cw, float* gx, hipStream_t st);
hipError_t launch_backward_idx(const void* gq, const float* gloss, const void* x, const int64_t* idx, const float* W, int64_t N,
                               int C, float cw, void* gx, hipStream_t st);
hipError_t launch_km_accumulate(const float* samples, const float* means, int64_t N, int C, int K, const KmPlan& p,
                                char* ws, float* sums, int64_t* counts64, hipStream_t st);
// per-code sums / counts of rows already assigned (idx from a forward): the k-means accumulation without the distance pass
hipError_t launch_code_sums(const void* x, int x_bf16, const int64_t* idx, int64_t N, int C, int K, const KmPlan& p, char* ws,
                            float* sums, int64_t* counts64, hipStream_t st);
hipError_t launch_ema_update(float* cluster_size, float* embed_avg, float* codebook, const float* sums, const int64_t* counts64,
                             int K, int C, float decay, float eps, float* total, hipStream_t st);
// dead-code revival (include/vqseg.h, EMA EXTENSION): the candidate rows of this rank, and the EMA update with the expiry fused in
// (scratch: 1 + K floats)
hipError_t launch_revive_candidates(const void* x, int x_bf16, int64_t N, int C, int K, uint64_t seed, const int64_t* t, int rank,
                                    int world, float* cand, float* ok, hipStream_t st);
hipError_t launch_ema_update_revive(float* cluster_size, float* embed_avg, float* codebook, const float* sums, const int64_t* counts64,
                                    int K, int C, float decay, float eps, float* scratch, const float* cand, const float* ok,
                                    float threshold, int64_t* t, int64_t* revived, hipStream_t st);
hipError_t launch_km_finalize(const float* sums, const int64_t* counts64, float* means, int C, int K, hipStream_t st);

}  // namespace vqseg
