/*
 * vqseg.h -- C ABI of libvqseg_hip.so: the MI355X (gfx950) hot path of the VQ-UNet
 * segmentation trainer (reference: chaeyeongyun/VQ_SEG, Python/PyTorch only).
 *
 * The reference has no FFI layer; its boundary for this path is the Python nn.Module
 * surface.  These entry points are what that surface binds: each one cites
 * the reference function (file:line, relative to the reference root) whose arithmetic
 * it replaces.  Plain pointers and sizes only -- no torch types, no C++ exceptions.  Process-global
 * state: the thread-local last-error string, the dispatch options of vqseg_set_option and the two
 * measurement recorders (vqseg_profile_*, vqseg_conv_profile_*) -- none of them thread safe; launches
 * themselves keep no state between calls.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is
 *     enqueued asynchronously on it, nothing synchronises, nothing allocates: the caller
 *     supplies a workspace of at least the size the matching *_workspace_bytes() returns;
 *   - return value: 0 = success, otherwise a negative VQSEG_E* code or a positive
 *     hipError_t; vqseg_last_error() returns a message for the calling thread;
 *   - alignment: activation tensors, weight images and workspaces are 16-byte aligned wherever a kernel moves them in 16-byte
 *     vectors, and the entry point checks it (VQSEG_EINVAL, nothing enqueued).  Besides the pointers named at the entry points
 *     below that is: y / res / out of vqseg_bn_apply_f / vqseg_bn_apply_bits_f, g_out / out / y / g_y / g_res of vqseg_bn_backward_f / _bits_f, x / g /
 *     out / gx_add / gx of the max-pool entry points, src / dst of vqseg_bilinear_f and gp / gx of vqseg_reflect_fold_f when the
 *     channel count is a multiple of 8 (bf16) or 4 (fp32) -- with any other channel count a thread moves one channel and the
 *     element's own alignment is enough; the images the four weight-pack entry points write; the 7x7x3 patch rows of vqseg_im2col_f with kp % 8 == 0; gy / x / x2 of the weight-gradient
 *     entry points; the workspaces of the BatchNorm backward, head backward and weight-gradient entry points.
 *     Per-channel fp32 vectors (scale, shift, gamma, statistics, dgamma ...), the head's weights, gradients and logits, fp32 images
 *     read by vqseg_im2col_f, the buffers of vqseg_cast_f, scalars, counters and the uint8 index / bit tensors need only their
 *     element's alignment;
 *   - activations are "rows": N = B*H*W pixel rows of C contiguous channels (NHWC /
 *     torch channels_last), which is the (B, HW, C) frame vq_img.py:232 rearranges into.
 */
#ifndef VQSEG_H
#define VQSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQSEG_ABI_VERSION 1

#define VQSEG_EINVAL  (-1)   /* bad argument (shape, alignment, null pointer)          */
#define VQSEG_ENOSPC  (-2)   /* workspace too small                                    */
#define VQSEG_ENODEV  (-3)   /* no gfx950 device / kernel image not loadable           */

int         vqseg_abi_version(void);
const char* vqseg_last_error(void);
/* Name of the dominant kernel symbol of an entry point (for rocprof matching). */
const char* vqseg_kernel_name(const char* entry_point);

/* Dispatch tunables (tests use them to reach every kernel with small shapes).  Keys:
 *   "conv3x3_patch_min_workgroups"  minimum grid of the patch-reuse 3x3 kernel before the generic implicit-GEMM
 *                                   kernel is preferred, and of its 256-channel tile (default 128, r4; r3: 256 = one workgroup per CU)
 *   "conv3x3_patch_unroll", "conv3x3_patch_wide_tile"   variants of that kernel (tap loop unrolled; 256-channel tile: default ON from r4 -- half
 *                                   the input re-reads; slower on a layer alone, faster in the two-stream step)
 *   "vq_max_tiles_per_wave"         cap (8, 4, 2, 1) on the 32-code accumulator tiles a wave of the VQ distance kernel
 *                                   holds (default 8; 4 measured equal within 2 % on every benchmark shape)
 *   "vq_bf16_filter"                1 (default): bf16 rows of layers with K % 256 == 0 and C % 32 == 0 take the bf16-MFMA candidate
 *                                   filter + exact re-score (same indices and distances as the exact kernel); 0: exact kernel on every row.
 *                                   "vq_filter_force_all" = 1 (tests): the filter decides nothing, every row is re-scored;
 *                                   "vq_filter_launches": returns the number of launches that took the filter so far, sets the counter
 *   "vq_s3_filter"                  1 (default): split-3 rows (row type 2) of such layers take the same filter on their [hi | lo] halves;
 *                                   0: the exact kernel on every row, merging hi + lo as it loads
 *   "conv_xcd_pair"                 implicit-GEMM layers with 2..value Cout chunks launch 1-D so that the chunks of an
 *                                   M tile run on the same XCD and share the input rows through its L2 (default 8, r4; r3: 4; 0: off)
 *   "conv3x3_patch_chunk_stage"     1 (default): 3x3 layers with 32-channel K chunks and <= 64 outputs (or 32 inputs) load all nine
 *                                   taps' weights with the patch -- one wait and barrier per chunk instead of per tap; 0: tap ring
 *   "conv3x3_patch_tile512"         512-pixel tiles of the patch kernel (32-channel chunks) for 32 / 64 output channels: 2 (default) on, 0
 *                                   off (192 -> 32 at 256^2 is 28 % faster with them; for 128 outputs they measured 10-17 % slower);
 *                                   "conv3x3_patch_tile512_min_workgroups" their minimum grid (default 512);
 *                                   "conv3x3_patch_tile512_launches" returns the number of launches that took such a tile so far and
 *                                   sets the counter to the value passed (tests)
 *   "conv_last_variant"             returns the id of the kernel instantiation the last convolution / weight-gradient launch took (0: none
 *                                   since it was last set to 0) and sets it to the value passed (tests).  One hexadecimal digit per
 *                                   template argument, the kernel family in the top digit:
 *                                     0x1TBWUMf  LDS-DMA implicit GEMM: T = pixel tile / 128, B = Cout tile / 32, W = waves, U = buffers, M = min
 *                                                waves per SIMD, f = split-3 * 8 + linear-pixel prologue * 4 + parity classes * 2 + XCD-pair 1-D grid
 *                                     0x20B0KPf  generic implicit GEMM: B = Cout tile / 32, K = K step / 32, P = precise, f = split-3 * 8
 *                                     0x3TBWKUf  3x3 patch kernel: T = pixel tile / 256, B = Cout tile / 32, W = weight ring slots (0: chunk stages),
 *                                                K = channel chunk / 32, U = taps unrolled, f = split-3 * 8 + XCD-pair 1-D grid
 *                                     0x40OIS0f  nine-tap weight gradient: O, I = Cout / Cin tile / 32, S = stride, f = XCD-aware 1-D grid
 *                                     0x50OI00f  1x1 weight gradient: the same digits;  0x60MN0P0  per-tap weight gradient: tiles / 32, P = precise
 *   "conv3x3_patch_xcd_pair"        1: the Cout chunks of a pixel tile are dispatched onto the same XCD (default 0:
 *                                   measured equal; the kernel does not wait on HBM for its patches)
 *   "conv_short_k_small_tile", "conv_short_k_single_buffer"   K loops of up to that many 64-channel stages take the
 *                                   128x128 tile at 4 waves/SIMD, double- resp. single-buffered (defaults 1 and 8)
 *   "conv_wgrad3x3_stride2"         1 (default): stride-2 3x3 weight gradients (Cout % 128 == 0, Wo % 16 == 0) on the nine-tap LDS-DMA
 *                                   kernel (r4); 0: the per-tap kernel
 *   "conv_wgrad1x1_narrow"          1 (default): 64-output-channel 1x1 weight gradients -- the stem's 160-column patch matrix, 64 -> 64
 *                                   -- on the LDS-DMA kernel (r4); 0: the per-tap kernel
 *   "conv_dgrad_s2_merge"           1 (default): vqseg_conv2d_dgrad_s2_fold_f available (r4); 0: it returns VQSEG_EINVAL (callers take the
 *                                   four-launch path with the padded grid)
 *   "conv_wgrad3x3_fill"            1 (default): nine-tap weight gradients split into one FULL round of resident workgroups (r4);
 *                                   0: r3's split
 *   "conv3x3_patch_wide_tile_s3"    1 (default): the split-3 3x3 launches take the 256-channel tile too (r4); "conv_wgrad_round_pct": workgroups the
 *                                   LDS-DMA weight gradients aim at, in percent of one resident round (default 100; 10..400)
 *   "stem_fused"                    1 (default): vqseg_stem7_conv_f available (r4); 0: it returns VQSEG_EINVAL (patch-matrix path)
 *   "conv_wgrad_xcd"                1 (default): a pixel slab's (ci, co) tiles of the LDS-DMA weight-gradient kernels on one XCD (r4); 0: 3-D grid
 *   "im2col_strip"                  1 (default): the stem's patch matrix from LDS-staged strips (r4, bit-identical); 0: the gather kernel
 *   "bn_bwd_premask"                1 (default): vqseg_bn_backward_f with `out` and a g_res output (a residual layer): the reduce pass writes
 *                                   g_res, the apply pass reads it instead of (g_out, out) (r4, bit-identical); 0: r3's two passes over both
 *   "bilinear_up2"                  1 (default): exact-2x resizes on their own kernels (bit-identical to the generic ones), the backward with four
 *                                   input rows per thread (r4); 2: one row per thread (r3); 0: the generic kernels
 *   "vq_fine_split"                 1 (default, r4): the distance kernel takes 4 code tiles per wave instead of 8 when that brings a launch to
 *                                   >= 4096 workgroups (a shorter last round: K = 512 on 172 k rows 0.76 -> 0.81 of the fp32 MFMA peak); 0: r3's choice
 *   "nn_grid_cap"                   8192 (default): most workgroups a grid-stride elementwise kernel (BatchNorm passes, resizes, pools) is launched with
 * The environment variable VQSEG_OPTS="key=value,..." applies options when the Python binding loads the library.
 * Returns the previous value, or VQSEG_EINVAL for an unknown key / negative value.  Not thread safe. */
int vqseg_set_option(const char* key, int value);

/* Measurement aid (bench.py roofline leg): while enabled, every launch of the distance+argmin
 * kernel is bracketed by a hipEvent pair on its own stream.  vqseg_profile_collect waits for the
 * recorded launches, writes per-launch (n_rows, channels, n_codes, milliseconds) to HOST arrays,
 * disables recording and returns the number of records (>= 0).  Not thread safe. */
int vqseg_profile_begin(int capacity);
int vqseg_profile_collect(int max_records, int64_t* n_rows_host, int* channels_host,
                          int* n_codes_host, float* ms_host,
                          int* kind_host /* nullable; 0: exact fp32-MFMA kernel on f32 rows (or split-3 rows, merged on load), 1: on bf16 rows, 2: bf16 candidate filter + exact re-score (bf16 or split-3 rows) */);

/* The same for the convolution kernels (forward, data gradient, fused-epilogue and split-3 launches of vqseg_conv2d_*): per launch
 * the ALGORITHMIC flops 2 * KH * KW * Cin * Cout * output pixels (logical channels for split-3; forward-layer pixels for the
 * data gradient of a strided layer), kind = KH * 100 + {0 bf16, 1 precise, 2 split-3; 50 / 51: the weight-gradient kernel of
 * vqseg_conv2d_wgrad_f in bf16 / precise mode, without its slab sum}, the in-stream milliseconds and the shape. */
int vqseg_conv_profile_begin(int capacity);
int vqseg_conv_profile_collect(int max_records, double* flops_host, int* kind_host, float* ms_host,
                               int* shape_host /* optional [4] per record: output pixels / 1024, Cin, Cout, stride * 10 + up */);

/* ---------------------------------------------------------------------------------- *
 * Vector quantiser forward.
 * Replaces EuclideanCodebook.forward (vector_quantizer/vq_img.py:160-177: cdist ->
 * argmin -> one_hot -> matmul -> bincount) and the straight-through / commitment part
 * of VectorQuantizer.forward (vq_img.py:228-244) in one call.
 *
 *   x         [N, C] f32   pixel rows (C % 4 == 0, 16-byte aligned)
 *   codebook  [K, C] f32   nn.Embedding weight (vq_img.py:152)
 *   quant     [N, C] f32   out: eval  -> codebook[idx]            (vq_img.py:170)
 *                               train -> x + (codebook[idx] - x)  (vq_img.py:236)
 *   idx       [N]    i64   out: argmin_k sqrt(max(|x|^2 + |e_k|^2 - 2 x.e_k, 0)), first
 *                               minimum wins (vq_img.py:167-168)
 *   loss      [1]    f32   out: training ? commitment_weight * mean((quant - x)^2) : 0
 *                               (vq_img.py:234-240)
 *   dead_pct  [1]    f32   out: 100 * (#codes never selected) / K  (vq_img.py:173-175)
 *   dmin      [N]    f32   optional out (may be NULL): the winning distance, for tests
 * ---------------------------------------------------------------------------------- */
size_t vqseg_vq_workspace_bytes(int64_t n_rows, int channels, int n_codes);
int vqseg_vq_forward_f32(const float* x, const float* codebook, const void* prepared,
                         int64_t n_rows, int channels, int n_codes, int training,
                         float commitment_weight, float* quant, int64_t* idx, float* loss,
                         float* dead_pct, float* dmin, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same forward for up to 4 independent layers ("levels") in ONE distance + argmin launch: the three VQ layers of a
 * VQ-UNet forward (net.py:1183-1191 calls them one after the other; they are independent).  Arrays of n_levels entries;
 * every level with its own workspace (vqseg_vq_workspace_bytes of ITS shape); one row type per call: bf16 = 0 f32 rows / quantised
 * rows, 1 bf16 rows / quantised rows, 2 split-3 rows -- x[i] is [n_rows][2 * channels] bf16 = [hi | lo] (what vqseg_s3_split_f writes),
 * its logical value the fp32 sum hi + lo (what vqseg_s3_merge_f writes): idx is that of the f32 call on the merged rows, and quant[i]
 * is [n_rows][2 * channels] bf16 = the split of the winning fp32 code rows, byte for byte vqseg_s3_split_f of the f32 call's quant.
 * Split-3 rows are an eval-mode format: bf16 = 2 needs training = 0 and channels % 8 == 0 (VQSEG_EINVAL otherwise, nothing is
 * launched).  Every level is checked before anything is enqueued: a refused call (VQSEG_EINVAL, VQSEG_ENOSPC) has written nothing,
 * not even the prepared codebooks of the levels in front of the offending one.  Results are bit-identical to n_levels single calls. */
int vqseg_vq_forward_group(int n_levels, int bf16, const void* const* x, const float* const* codebook,
                           const void* const* prepared, const int64_t* n_rows, const int* channels, const int* n_codes,
                           int training, const float* commitment_weight, void* const* quant, int64_t* const* idx,
                           float* const* loss, float* const* dead_pct, void* const* workspace,
                           const size_t* workspace_bytes, void* stream);

/* Diagnostics of the bf16 candidate filter (options "vq_bf16_filter", "vq_s3_filter"): byte offset, inside the workspace of a bf16 or split-3 call of this shape,
 * of the 64 int32 counters (one per sub-list; their sum = the (row, code) candidate pairs the filter handed to the exact re-score;
 * valid after the call's stream work has finished; a 65th int is the overflow flag: the exact kernel served the level); 0 if the shape does not take the filter
 * (needs n_codes % 256 == 0 and channels % 32 == 0). */
size_t vqseg_vq_filter_counter_offset(int64_t n_rows, int channels, int n_codes);

/* Host-only query: the code tiles per wave (T = 8, 4, 2 or 1) the distance + argmin launch of these levels takes under the current
 * options ("vq_max_tiles_per_wave", "vq_fine_split") -- one level: a single call of that shape; several: vqseg_vq_forward_group.
 * HOST arrays of n_levels (1..4) entries.  VQSEG_EINVAL for a bad argument.  Touches no device. */
int vqseg_vq_tiles_per_wave(int n_levels, const int64_t* n_rows_host, const int* n_codes_host);

/* Assignment only (no gather): used by k-means and by tests. */
int vqseg_vq_assign_f32(const float* x, const float* codebook, const void* prepared,
                        int64_t n_rows, int channels, int n_codes, int64_t* idx, float* dmin,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same for bf16 rows (autocast activations; every bf16 value is an exact float, the arithmetic is the fp32 one). */
int vqseg_vq_assign_bf16(const void* x, const float* codebook, const void* prepared,
                         int64_t n_rows, int channels, int n_codes, int64_t* idx, float* dmin,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same for split-3 rows: x [n_rows][2 * channels] bf16 = [hi | lo]; idx and dmin are those of vqseg_vq_assign_f32 on the merged
 * rows (vqseg_s3_merge_f), without that pass over memory.  channels % 8 == 0.  Option "vq_s3_filter" chooses the kernels. */
int vqseg_vq_assign_s3(const void* x, const float* codebook, const void* prepared,
                       int64_t n_rows, int channels, int n_codes, int64_t* idx, float* dmin,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Prepared codebook: the kernel-side image of an nn.Embedding weight (4-channel
 * interleaved, code-padded copy + |e_k|^2).  The reference's codebook never changes after
 * its k-means init (no gradient, no EMA -- vq_img.py:236-239), so callers prepare once
 * and pass the blob to every forward; `prepared == NULL` makes forward/assign prepare
 * into the workspace on every call instead.  The blob is opaque: its parts start at 256-byte boundaries, and the bytes of the
 * gaps between them (and of parts a shape does not use) are unspecified -- vqseg_vq_prepare_f32 need not write them. */
size_t vqseg_vq_prepared_bytes(int channels, int n_codes);
int vqseg_vq_prepare_f32(const float* codebook, int channels, int n_codes, void* prepared,
                         size_t prepared_bytes, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Vector quantiser backward (analytic; autograd of vq_img.py:236-240):
 *   grad_x = grad_quant + grad_loss[0] * commitment_weight * 2 (x - quant) / (N*C)
 * `quant` is the training-mode forward output.  grad_loss may be NULL (treated as 0).
 * ---------------------------------------------------------------------------------- */
int vqseg_vq_backward_f32(const float* grad_quant, const float* grad_loss, const float* x,
                          const float* quant, int64_t n_rows, int channels,
                          float commitment_weight, float* grad_x, void* stream);

/* The same layer on bf16 activations (the trainer's autocast mode): x and quant are bf16 rows, every bf16 value is an
 * exact float and all arithmetic (distances, argmin, straight-through value, commitment) is the fp32 arithmetic of the
 * f32 entry points, so the indices are identical to those of the up-cast rows; quant is rounded to bf16 on store.
 * Backward re-reads e = codebook[idx] in fp32 (the bf16 quant would cost the commitment gradient its accuracy):
 *   grad_x = grad_quant + (2 w grad_loss / (n c)) (x - e).
 * Precondition: every idx[i] lies in [0, n_codes) -- what a forward returns; it addresses the codebook unchecked. */
int vqseg_vq_forward_bf16(const void* x, const float* codebook, const void* prepared, int64_t n_rows, int channels,
                          int n_codes, int training, float commitment_weight, void* quant, int64_t* idx, float* loss,
                          float* dead_pct, float* dmin, void* workspace, size_t workspace_bytes, void* stream);
int vqseg_vq_backward_bf16(const void* grad_quant, const float* grad_loss, const void* x, const int64_t* idx,
                           const float* codebook, int64_t n_rows, int channels, float commitment_weight,
                           void* grad_x, void* stream);

/* ---------------------------------------------------------------------------------- *
 * k-means codebook initialisation, Lloyd iterations GIVEN the initial means.
 * Replaces kmeans() (vq_img.py:29-63, euclidean branch) after its RNG draw (:10-17,
 * done by the host with torch.randperm):  per iteration  assign (argmax of -cdist ==
 * argmin of cdist) -> per-cluster counts -> per-cluster sums -> divide -> clusters with no
 * member keep their mean.  The sums are deterministic but not in scatter_add_'s single running order:
 * member lists are in row order, cut into segments of 128 members, four interleaved partial sums per
 * segment, a cluster's segments folded as four interleaved chains in fixed order (fp32; agreement with the CPU order is at rounding level, asserted
 * at 1e-5 in tests/test_vq_gpu.py).
 *
 *   samples [N, C] f32, means [K, C] f32 in/out, bins [K] i64 out (last iteration).
 *   samples, means and the workspace are 16-byte aligned (read in 16-byte vectors; checked: VQSEG_EINVAL); sums, counts, bins and
 *   the means of vqseg_kmeans_finalize_f32 need only their element's alignment.
 *
 * Data-parallel use: vqseg_kmeans_accumulate_f32 produces this rank's sums/counts so
 * the host can all-reduce them (RCCL) before vqseg_kmeans_finalize_f32.
 * ---------------------------------------------------------------------------------- */
size_t vqseg_kmeans_workspace_bytes(int64_t n_rows, int channels, int n_codes);
int vqseg_kmeans_f32(const float* samples, float* means, int64_t* bins, int64_t n_rows,
                     int channels, int n_codes, int iters, void* workspace,
                     size_t workspace_bytes, void* stream);
int vqseg_kmeans_accumulate_f32(const float* samples, const float* means, int64_t n_rows,
                                int channels, int n_codes, float* sums, int64_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream);
int vqseg_kmeans_finalize_f32(const float* sums, const int64_t* counts, float* means,
                              int channels, int n_codes, void* stream);


/* ---------------------------------------------------------------------------------- *
 * EXTENSION -- EMA codebook update (opt-in; BASELINE.json north_star names it, the reference does not have it:
 * vq_img.py:72,83,140,151 accept and store `decay` / `eps` but the codebook is never written after the k-means init,
 * SURVEY 0.1 / q6).  The rule is the published one of the module the reference descends from (vector-quantize-pytorch,
 * EuclideanCodebook.forward: ema_inplace + laplace_smoothing); there is no reference output to pin it against, so its
 * tests compare with a tensor-op restatement of that rule ("parity unpinned").
 *   vqseg_vq_code_sums:      sums[k][c] = sum of the rows assigned to code k, counts[k] = how many -- from the idx a
 *                            forward returned (no second distance pass); rows f32 or bf16; deterministic (the k-means
 *                            member-list reduction).  workspace: vqseg_kmeans_workspace_bytes(n_rows, channels, n_codes).
 *                            Data-parallel use: all-reduce sums and counts (RCCL) before the update.
 *                            Precondition: every idx[i] lies in [0, n_codes); it addresses the histograms unchecked.
 *   vqseg_vq_ema_update_f32: cluster_size <- d cluster_size + (1-d) counts;  embed_avg <- d embed_avg + (1-d) sums;
 *                            codebook <- embed_avg / ((cluster_size + eps) / (S + K eps) * S),  S = sum cluster_size.
 *                            scratch: 1 float on the device.
 *
 * Dead-code revival (opt-in on top of the EMA rule; that library never ships the EMA rule without it: its
 * `threshold_ema_dead_code`.  No copy of it exists to compare with, so the rule below IS the specification; parity unpinned,
 * like the EMA rule itself).  After the update above, on the state it has just written, with tau = threshold:
 *     expired[k] = cluster_size[k] < tau                      (the UPDATED moving count, before any reset)
 *     for expired k whose candidate row s_k is entirely finite:
 *         codebook[k] = s_k;   embed_avg[k] = s_k * tau (one fp32 multiply);   cluster_size[k] = tau
 *     every other code keeps exactly what vqseg_vq_ema_update_f32 writes; S sums the updated counts BEFORE any reset.
 *   The candidate is a pure function of (seed, t, k), t = the number of EMA updates of this codebook so far -- no generator, no state.
 *   With M = 2^64:
 *     x = (seed + 0x9E3779B97F4A7C15 * (t * 2^32 + k + 1)) mod M              (splitmix64 at counter t * 2^32 + k + 1)
 *     x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) mod M;   x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) mod M;   h = x ^ (x >> 31)
 *     g = h mod (world * n_rows);   owner = g / n_rows;   j = g mod n_rows;   s_k = float32(rows of rank `owner`[j])
 *   (every rank holds n_rows rows; world = 1, rank = 0 without data parallelism).  Two ranks on two shards revive what one process
 *   on the concatenated shards revives.
 *   vqseg_vq_revive_candidates:     cand[k][c] (f32) = the row if this rank is its owner, bit for bit (bf16 widened), else zeros;
 *                                   ok[k] (f32) = 1 if this rank owns code k's candidate and the row is entirely finite, else 0.  One
 *                                   launch; t is read from `counter` on the device.  Data-parallel use: all-reduce cand and ok together
 *                                   with the code sums (one message).  rows f32 (channels % 4 == 0) or bf16 (channels % 8 == 0).
 *   vqseg_vq_ema_update_revive_f32: vqseg_vq_ema_update_f32 (same operations in the same order, same reduction tree for S) with the
 *                                   expiry fused in: two launches.  Writes the number of revived codes to `revived` and increments
 *                                   *counter; both stay on the device.  scratch: 1 + n_codes floats on the device.
 * ---------------------------------------------------------------------------------- */
int vqseg_vq_code_sums(int bf16, const void* x, const int64_t* idx, int64_t n_rows, int channels, int n_codes,
                       float* sums, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int vqseg_vq_ema_update_f32(float* cluster_size, float* embed_avg, float* codebook, const float* sums,
                            const int64_t* counts, int channels, int n_codes, float decay, float eps, float* scratch,
                            void* stream);
int vqseg_vq_revive_candidates(int bf16, const void* x, int64_t n_rows, int channels, int n_codes, uint64_t seed,
                               const int64_t* counter, int rank, int world, float* cand, float* ok, void* stream);
int vqseg_vq_ema_update_revive_f32(float* cluster_size, float* embed_avg, float* codebook, const float* sums,
                                   const int64_t* counts, int channels, int n_codes, float decay, float eps, float* scratch,
                                   const float* cand, const float* ok, float threshold, int64_t* counter, int64_t* revived,
                                   void* stream);

/* ================================================================================== *
 * Encoder / decoder blocks.  Tensors are NHWC rows; `precise` = 1: activations fp32, bf16x3
 * split MFMA (parity mode); 0: activations bf16 (fast mode).  `bf16` flags name the
 * element type of the activation tensors (0 = f32, 1 = bf16).
 * ================================================================================== */

/* nn.Conv2d weights [Cout][Cin][KH][KW] f32 -> MFMA-side image [Cout][KH][KW][Cin] bf16 (hi, and lo
 * when `lo` != NULL).  transpose_flip = 1 builds the data-gradient image [Cin][KH][KW][Cout] with the
 * taps flipped.  The contracted channel count is zero-padded to a multiple of 32; each array holds
 * vqseg_conv_packed_elems() 16-bit elements. */
size_t vqseg_conv_packed_elems(int cout, int cin, int kh, int kw, int transpose_flip);
int vqseg_conv_pack_weights_f32(const float* w, int cout, int cin, int kh, int kw, int transpose_flip,
                                void* hi, void* lo, void* stream);

/* Implicit-GEMM convolution, no bias.  Replaces nn.Conv2d in conv_bn_relu
 * (models/networks/unet/decoder.py:7-10) and in the ResNet blocks (models/encoders/resnet.py:117-190):
 *   y[n,oh,ow,co] = sum_{kh,kw,ci} in[n, (oh*stride - pad + kh)/up, (ow*stride - pad + kw)/up, ci] * w[co,kh,kw,ci]
 * with zero padding, or reflect padding (nn.Conv2d(padding_mode='reflect'), resnet.py:134-148) when
 * `reflect`; `up` > 1 reads the input on an up-sampled grid (only exact multiples exist): the data
 * gradient of a stride-`up` convolution.  Channels [0,c1) come from x, [c1,cin) from x2 -- the decoder's
 * torch.cat((upsampled, skip), 1) (decoder.py:35-37) fused into the loader (c1 == cin: no concat).
 * stat_partial (nullable): per-wave (mean, M2) BatchNorm partials, vqseg_conv_stat_slots() x 2 x cout floats. */
int64_t vqseg_conv_stat_slots(int64_t m_rows, int cout);
int vqseg_conv2d_f(const void* x, const void* x2, int c1, const void* w_hi, const void* w_lo, void* y,
                   float* stat_partial, int n, int h, int w, int cin, int cout, int kh, int kw, int stride,
                   int pad, int reflect, int up, int ho, int wo, int precise, void* stream);

/* Weight gradient of the same convolution: gw[co][ci][kh][kw] (nn.Conv2d layout, f32) =
 * sum_m gy[m][co] * in_tap[m][ci].  im2col = 1: x is a [M][cin] patch matrix of a kh x kw x cin_out
 * convolution (the 7x7 stem) and gw gets [cout][cin_out][kh][kw]. */
/* The same convolution with a fused per-channel affine epilogue: y = relu?( conv * scale[c] + shift[c] (+ res) ).
 * This is conv -> eval-mode nn.BatchNorm2d (scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean *
 * scale; vqseg_bn_finalize_f with training = 0 yields both) -> [+ residual] -> [ReLU] in one pass, for the
 * no-grad pseudo-label forwards (train_vqreptunet1x1v2.py eval passes). */
int vqseg_conv2d_affine_f(const void* x, const void* x2, int c1, const void* w_hi, const void* w_lo,
                          const float* scale, const float* shift, const void* res, int relu, void* y,
                          int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int reflect,
                          int ho, int wo, int precise, void* stream);
/* bf16, stride 1, zero padding, no concat: y = conv * scale[c] + shift[c] + res .* bits, with bits as written by
 * vqseg_bn_apply_bits_f over res's flat [n*ho*wo*cout] index (cout % 8 == 0).  This is the data gradient of a residual block's
 * first convolution meeting the block's shortcut gradient g_out .* (out > 0) (resnet.py:106-108) without that product ever
 * being stored. */
int vqseg_conv2d_affine_bits_f(const void* x, const void* w_hi, const float* scale, const float* shift, const void* res,
                               const unsigned char* res_bits, void* y, int n, int h, int w, int cin, int cout, int kh, int kw,
                               int pad, int ho, int wo, void* stream);

/* `accumulate` (here and in vqseg_bn_backward_f): the parameter gradient is ADDED to gw / dgamma / dbeta (the
 * optimiser's gradient buffer) instead of overwriting it -- autograd's own accumulate kernel is then not needed. */
size_t vqseg_conv2d_wgrad_workspace_bytes(int n, int h, int w, int cin, int ho, int wo, int cout, int kh, int kw);
int vqseg_conv2d_wgrad_f(const void* gy, const void* x, const void* x2, int c1, int n, int h, int w, int cin,
                         int ho, int wo, int cout, int kh, int kw, int stride, int pad, int reflect, int precise,
                         int cin_out, int im2col, int accumulate, void* workspace, size_t workspace_bytes, float* gw,
                         void* stream);
/* The same weight gradient summed over TWO uses of the layer in one launch: (gy, x, x2) with n images and (gy_b, x_b, x2_b) with
 * n_b images of the same geometry form a virtual batch of n + n_b images.  In a cross-pseudo-supervision step every weight is
 * used by two training forwards per network (labelled and unlabelled batch: train_vqreptunet1x1v2.py:153-156, one backward
 * :199): the caller queues the first use's (gy, x) and issues one launch over both -- twice the contraction length per
 * workgroup, half the slab sums.  n_b == 0: identical to vqseg_conv2d_wgrad_f.  Workspace: vqseg_conv2d_wgrad_workspace_bytes
 * with n + n_b images. */
int vqseg_conv2d_wgrad2_f(const void* gy, const void* x, const void* x2, int n, const void* gy_b, const void* x_b, const void* x2_b,
                          int n_b, int c1, int h, int w, int cin, int ho, int wo, int cout, int kh, int kw, int stride, int pad,
                          int reflect, int precise, int cin_out, int im2col, int accumulate, void* workspace, size_t workspace_bytes,
                          float* gw, void* stream);

/* nn.BatchNorm2d (+ fused residual add and ReLU).  Training: batch statistics merged from the conv
 * epilogue partials (Welford/Chan, double, fixed order), running stats updated like nn.BatchNorm2d
 * (biased variance to normalise, unbiased into running_var).  Eval: running statistics.
 *   finalize -> scale[c] = gamma*invstd, shift[c] = beta - mean*scale, save_mean, save_invstd
 *               (`partial` is CONSUMED: the two-level merge folds group results back into it in place)
 *   apply    -> out = relu?( y*scale + shift (+ res) )
 *   backward -> gz = g_out * (out > 0); dgamma, dbeta; g_y (train: with the batch-statistics terms);
 *               g_res = gz when a residual branch exists.  Without a residual `out` may be NULL: the mask is then
 *               recomputed as fma(y, fwd_scale, fwd_shift) > 0, the forward's own expression (one tensor read less). */
/* `sync` (nullable; finalize and backward): vqseg_bn_sync_ints(c) ints that hold ZEROS between launches (zero them once; the
 * library leaves them zero) and that no two concurrent launches share -- e.g. one buffer per BatchNorm module and direction.
 * With it the statistics merge + finalize (forward) / the reduction + finalize (backward) run as ONE launch each: the last
 * workgroup of a 64-channel group does the final fold, in a fixed order (deterministic; r3: ~700 launches per training step
 * less).  NULL: the two-launch form. */
int vqseg_bn_sync_ints(int c);
int vqseg_bn_finalize_f(float* partial, int64_t m_rows, int c, const float* gamma, const float* beta,
                        float* run_mean, float* run_var, float momentum, float eps, int training,
                        float* scale, float* shift, float* save_mean, float* save_invstd,
                        int64_t* num_batches_tracked /* nullable: += 1 in training mode */, int* sync, void* stream);
int vqseg_bn_apply_f(int bf16, const void* y, const void* res, const float* scale, const float* shift,
                     int64_t m_rows, int c, int relu, void* out, void* stream);
size_t vqseg_bn_backward_workspace_floats(int64_t m_rows, int c);
int vqseg_bn_backward_f(int bf16, const void* g_out, const void* out, const void* y, const float* mean,
                        const float* invstd, const float* gamma, const float* fwd_scale, const float* fwd_shift,
                        int64_t m_rows, int c, int relu, int training, int accumulate,
                        float* workspace, float* dgamma, float* dbeta, void* g_y, void* g_res, int* sync, void* stream);
/* r4, residual layers in bf16 (out = relu(y*scale + shift + res), resnet.py:106-108 / 67-69; c % 8 == 0): the apply pass also
 * writes the ReLU mask as a bit field, bits[i / 8] bit (i % 8) = (out[i] > 0) over the flat [m_rows * c] index (m_rows * c / 8
 * bytes), and the backward reads that instead of `out` (1/16 of its bytes).  g_res (nullable) = g_out * mask, the residual
 * branch's gradient; NULL when its consumer applies the bits to g_out itself (vqseg_conv2d_affine_bits_f: the block's first
 * convolution adds the masked gradient in its data-gradient epilogue), which saves writing and re-reading that tensor.
 * Results are bit-identical to vqseg_bn_apply_f / vqseg_bn_backward_f with `out`. */
int vqseg_bn_apply_bits_f(const void* y, const void* res, const float* scale, const float* shift, int64_t m_rows, int c,
                          void* out, unsigned char* bits, void* stream);
int vqseg_bn_backward_bits_f(const void* g_out, const unsigned char* bits, const void* y, const float* mean,
                             const float* invstd, const float* gamma, int64_t m_rows, int c, int training, int accumulate,
                             float* workspace, float* dgamma, float* dbeta, void* g_y, void* g_res, int* sync, void* stream);

/* nn.MaxPool2d(3, 2, 1) (resnet.py:167) forward / backward (first maximum in scan order).
 * idx (nullable, uint8 [n, ho, wo, c]): forward writes the window position (kh*3+kw) of each maximum; backward
 * reads it instead of recomputing the arg-max from x (x may then be NULL). */
int vqseg_maxpool3x3s2_f(int bf16, int backward, const void* x, const void* g, int n, int h, int w, int c,
                         void* out, unsigned char* idx, void* stream);

/* Bilinear resize: F.interpolate(mode='bilinear') (decoder.py:35, align_corners = 0) and
 * nn.UpsamplingBilinear2d (modified_vqunet/net.py:1172, align_corners = 1).
 * forward: src [n,h,w,c] -> dst [n,ho,wo,c];  backward: src = grad [n,ho,wo,c] -> dst [n,h,w,c]. */
int vqseg_bilinear_f(int bf16, int backward, const void* src, int n, int h, int w, int c, int ho, int wo,
                     int align_corners, void* dst, void* stream);

/* 1x1 segmentation head, nn.Conv2d(32, num_classes, 1, bias=False) (net.py:1169): logits f32.  Cin % 8 == 0, Cin <= 64, Cout <= 4.
 * Row type `bf16`: 0 f32, 1 bf16, 2 (forward only) split-3 rows [2 * Cin] (see "Split-3" below). */
int vqseg_head1x1_forward_f(int bf16, const void* x, const float* w, int64_t m_rows, int cin, int cout,
                            float* y, void* stream);
size_t vqseg_head1x1_backward_workspace_floats(int64_t m_rows, int cin, int cout);
int vqseg_head1x1_backward_f(int bf16, const void* x, const float* w, const float* g, int64_t m_rows, int cin,
                             int cout, void* gx, float* gw, float* workspace, void* stream);
/* Fan-in forms (r4): the tensor whose gradient these produce has a second consumer whose gradient `gx_add` (same shape and type;
 * NULL: none) is added on the way out -- rounded as autograd's own add of the two tensors would round (each to the activation
 * type first).  head: the decoder output feeds the head AND the prototype loss (net.py:1193-1203); max-pool: the stem output feeds
 * the pool AND the last decoder block (resnet.py:164-171, decoder.py:35-37). */
int vqseg_head1x1_backward_add_f(int bf16, const void* x, const float* w, const float* g, int64_t m_rows, int cin,
                                 int cout, void* gx, float* gw, float* workspace, const void* gx_add, void* stream);
int vqseg_maxpool3x3s2_backward_add_f(int bf16, const void* g, const unsigned char* idx, const void* gx_add, int n, int h, int w,
                                      int c, void* gx, void* stream);

/* Stem support: patch matrix of the 7x7/2 convolution (resnet.py:122-125; zero or reflect padding),
 * columns (kh, kw, ci) padded with zeros to kp; gradient fold of reflect padding 1; f32 <-> bf16 cast.
 * Reflect padding needs pad < h and pad < w (one reflection, as F.pad), else VQSEG_EINVAL. */
int vqseg_im2col_f(int out_bf16, const float* x, int n, int h, int w, int cin, int kh, int kw, int stride,
                   int pad, int reflect, int ho, int wo, int kp, void* out, void* stream);
int vqseg_reflect_fold_f(int bf16, const void* gp, int n, int h, int w, int c, void* gx, void* stream);
/* r4: the stem convolution (7x7 / stride 2 / pad 3, 3 -> 64 channels: resnet.py:122-125) STRAIGHT from the fp32 image x [n][h][w][3], without
 * the patch matrix: a workgroup stages the input rows its 128 output pixels read and takes its MFMA operands from them.  The contraction
 * runs over k' = kh * 24 + (kw * 3 + ci) (each kernel row's 21 taps padded to 24; 176 columns = eleven K steps): a fragment is then 8
 * consecutive words of one staged row.  Equal to the 1x1 convolution over vqseg_im2col_f's matrix up to the summation grouping (bf16
 * outputs within one unit in the last place).  w_img: [64][176] bf16, column kh * 24 + kw * 3 + ci = bf16(w[co][ci][kh][kw]), zero
 * elsewhere; s3 = 1: [64][2][176] = the hi image | the lo image (bf16 of the remainder), y = split-3 rows [n][ho][wo][128] = hi | lo.
 * Either stat_partial (raw y + BatchNorm partials: vqseg_conv_stat_slots) or scale / shift (+ relu): the fused eval epilogue (required
 * for s3).  Output width (w + 6 - 7) / 2 + 1 must be a multiple of 128, else VQSEG_EINVAL (callers keep the patch-matrix path). */
int vqseg_stem7_conv_f(int s3, const float* x, const void* w_img, void* y, float* stat_partial, const float* scale, const float* shift, int relu,
                       int n, int h, int w, int reflect, void* stream);
/* The data gradient of a 3x3 / stride 1 / REFLECT-pad-1 convolution (resnet.py:134-148: every Bottleneck conv2) without the padded
 * gradient tensor (r4): gx [n][h][w][cgx] must already hold the ZERO-padded data gradient of gy (vqseg_conv2d_f with the transposed
 * image and pad 1: the padded gradient's interior, on the fast patch kernel); this call evaluates the full correlation only on the
 * border ring of the (h + 2) x (w + 2) grid -- ring [n][2 (w + 2) + 2 h][cgx], scratch -- and folds the ring onto rows 1 / h-2 and
 * columns 1 / w-2 of gx in place.  bf16 activations; cgy % 64 == 0 (gy's channels), cgx % 8 == 0; h, w >= 4. */
int vqseg_reflect_ring_f(const void* gy, const void* t_hi, void* ring, void* gx, int n, int h, int w, int cgy, int cgx, void* stream);

/* ----------------------------------------------------------------------------------
 * "Split-3" activations: the fp32-precision NO-GRAD EVAL forward (the trainers' pseudo-label passes, outside autocast:
 * train_vqreptunet1x1v2.py:143-149) on the bf16 MFMA kernels.  A logical fp32 tensor [rows][C] is kept as [rows][2C] bf16 =
 * [hi | lo] with hi = bf16(v), lo = bf16(v - hi) (v = hi + lo to ~2^-17).  A bf16 convolution whose K loop runs over the logical
 * channels [hi | lo | hi] (hi read twice) with the weight image [w_hi | w_hi | w_lo] computes x_hi w_hi + x_lo w_hi + x_hi w_lo:
 * the same three products, fp32 accumulation, as the "precise" kernels (vqseg_conv2d_f precise = 1), on the LDS-DMA / patch-reuse
 * kernels instead.
 *   vqseg_conv2d_affine_f(..., precise = 2): x / x2 / res / y are split-3 tensors, cin / c1 / cout LOGICAL channel counts
 *       (Cin, C1 % 32 == 0, Cout % 8 == 0), w_hi = vqseg_conv_pack_weights_s3_f32's image, w_lo unused.
 *   vqseg_im2col_f(out_bf16 = 2, ...): split-3 patch rows [2 * kp] (7x7x3 stem only).
 *   split / merge: fp32 rows <-> split-3 rows;  maxpool / bilinear: the forward ops of vqseg_maxpool3x3s2_f /
 *       vqseg_bilinear_f on split-3 tensors (values hi + lo, re-split on the way out).  channels % 8 == 0.
 * ---------------------------------------------------------------------------------- */
int vqseg_conv_pack_weights_s3_f32(const float* w, int cout, int cin, int c1, int kh, int kw, void* out, void* stream);

/* Data gradient of a STRIDE-2 convolution (encoder: the 3x3 conv2 of a stage's first bottleneck and its 1x1 projection shortcut,
 * resnet.py:117-190 on torchvision's Bottleneck) without the 4x wasted work of an up-sampled ("dilated") gradient grid: the
 * output pixels split into parity classes, each a small stride-1 convolution over gy (k = 3: 2x2, 2x1, 1x2, 1x1 taps; k = 1:
 * one class, the other pixels are zero).  gx is (n, oh, ow, cin): for k = 3 the PADDED input grid (oh = h + 2; fold reflect /
 * crop zero padding afterwards), for k = 1 the input grid.  Weights: vqseg_conv_pack_weights_s2_f32's sub-images
 * (vqseg_conv_packed_s2_elems elements each for hi / lo; lo only in precise mode). */
/* The forward (vqseg_conv_pack_weights_f32, transpose_flip = 0, hi), data-gradient (transpose_flip = 1, hi) and split-3
 * (vqseg_conv_pack_weights_s3_f32) images of one k x k weight (k = 1 or 3) in ONE launch; any of the three outputs may be NULL.
 * Bit-identical to the single-image entry points. */
int vqseg_conv_pack_all_f32(const float* w, int cout, int cin, int k, int c1, void* fwd, void* tr, void* s3, void* stream);
size_t vqseg_conv_packed_s2_elems(int cout, int cin, int k);
int vqseg_conv_pack_weights_s2_f32(const float* w, int cout, int cin, int k, void* hi, void* lo, void* stream);
/* `accumulate` (k == 1 only, r4): gx already holds the gradient the tensor received from its OTHER consumer (an encoder feature feeds
 * the next stage AND the decoder / VQ layer); the data gradient is added to it in place at the pixels it touches -- no memset and no
 * separate add pass (bit-identical to adding the two tensors). */
int vqseg_conv2d_dgrad_s2_f(const void* gy, const void* w_hi, const void* w_lo, void* gx, int n, int ho, int wo, int cout, int cin,
                            int k, int oh, int ow, int precise, int accumulate, void* stream);
/* r4: the 3x3 / stride 2 / pad 1 data gradient (bf16; the first conv2 of a Bottleneck stage, reflect-padded in the VQ-UNet's encoder:
 * resnet.py:134-148; the first conv1 of a BasicBlock stage, zero-padded) written STRAIGHT into the unpadded gx [n][h][w][cin]
 * (h = 2 ho, w = 2 wo): the four parity classes in ONE launch, no padded-grid tensor, no fold / crop pass over it.  gx must hold
 * vqseg_conv2d_dgrad_s2_fold_rows(n, h, w, reflect) rows of cin elements: behind the n * h * w pixel rows, reflect padding keeps
 * the gradients of the padded top row / left column (a ring of n * (w + 1 + h) rows, added onto x row 1 / column 1 by a second
 * small launch) and one dump row.  w_hi: vqseg_conv_pack_weights_s2_f32's image (k = 3).  VQSEG_EINVAL for shapes outside the
 * merged path (cout % 64, cin % 8, cin >= 64) or with option "conv_dgrad_s2_merge" = 0: use vqseg_conv2d_dgrad_s2_f then. */
int64_t vqseg_conv2d_dgrad_s2_fold_rows(int n, int h, int w, int reflect);
int vqseg_conv2d_dgrad_s2_fold_f(const void* gy, const void* w_hi, void* gx, int n, int ho, int wo, int cout, int cin, int h, int w,
                                 int reflect, void* stream);
int vqseg_s3_split_f(const float* x, int64_t rows, int channels, void* y, void* stream);
int vqseg_s3_merge_f(const void* x, int64_t rows, int channels, float* y, void* stream);
int vqseg_s3_maxpool3x3s2_f(const void* x, int n, int h, int w, int c, void* y, void* stream);
int vqseg_s3_bilinear_f(const void* x, int n, int h, int w, int c, int ho, int wo, int align_corners, void* y, void* stream);
int vqseg_cast_f(int to_bf16, const void* x, int64_t n, void* y, void* stream);

/* Reliable prototype losses (models/modules/prototype.py:500-613 ReliablePrototypeLoss = variant 1, :778-888
 * ReliablePrototypeLossv2 = variant 2) after the host-side label resize / entropy threshold: fused forward (scalar loss,
 * double) and backward (d loss / d x in the activation type; variant 2 also d loss / d prototypes [k][c], nullable).
 *   x [m][c] decoder features (f32 or bf16), proto [k][c] L2-normalised, labels [m] i64,
 *   keep [m] u8 (variant 1: entropy <= percentile; NULL = all), conf [m] f32 (variant 2 confidence mask; NULL = 1),
 *   margin / scale / easy_margin: the module's ArcFace parameters; g_loss: upstream gradient (device scalar). */
size_t vqseg_proto_loss_workspace_bytes(int64_t m_rows, int c, int k);
int vqseg_proto_loss_forward_f(int bf16, const void* x, const float* proto, const int64_t* labels,
                               const unsigned char* keep, const float* conf, int64_t m_rows, int c, int k,
                               int variant, float scale, float margin, int easy_margin,
                               void* workspace, size_t workspace_bytes, double* loss, void* stream);
int vqseg_proto_loss_backward_f(int bf16, const void* x, const float* proto, const int64_t* labels,
                                const unsigned char* keep, const float* conf, int64_t m_rows, int c, int k,
                                int variant, float scale, float margin, int easy_margin, const float* g_loss,
                                void* gx, float* gproto, void* workspace, size_t workspace_bytes, void* stream);

/* Soft Dice sums of loss/dice_loss.py:5-37 (softmax form, 2..4 classes; ignored pixels: zero logits, class-0 target):
 *   inter[b][c] = sum_px p_c 1[t == c],  sets[b][c] = sum_px (p_c + 1[t == c]);  the scalar formula on these (B x C)
 * sums stays with the host.  logits element (b, c, px) at b*stride_b + c*stride_c + px*stride_px (NCHW or NHWC);
 * backward writes d loss / d logits in the same layout from d loss / d inter, d loss / d sets. */
size_t vqseg_dice_workspace_bytes(int b, int c, int64_t hw);
int vqseg_dice_sums_forward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                              const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index,
                              void* workspace, size_t workspace_bytes, float* inter, float* sets, void* stream);
int vqseg_dice_sums_backward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                               const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index,
                               const float* g_inter, const float* g_sets, float* g_logits, void* stream);

/* The same pass with the cross-entropy term of the v2 recipe riding along (train_vqreptunet1x1v2.py:165-187:
 * 0.5 * nn.CrossEntropyLoss(ignore_index=255) + Dice on the same logits and targets):
 *   ce[b][0] = sum over pixels with target != ignore_index of -log softmax(logits)[target],  ce[b][1] = their number;
 * the mean CE is sum_b ce[b][0] / sum_b ce[b][1] on the host.  backward adds g_ce[b][0] * (softmax - onehot) on those pixels.
 * `ce` / `g_ce` may be NULL (= the two entry points above). */
int vqseg_dice_ce_sums_forward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                                 const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index,
                                 void* workspace, size_t workspace_bytes, float* inter, float* sets, float* ce,
                                 void* stream);
int vqseg_dice_ce_sums_backward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                                  const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index,
                                  const float* g_inter, const float* g_sets, const float* g_ce, float* g_logits,
                                  void* stream);

/* Pseudo-label statistics in one pass over the logits (layout as for the Dice sums): per pixel the arg-max class (i64),
 * the entropy -sum p log(p + 1e-10) and the top probability of softmax(logits); any output may be NULL.  Replaces
 * softmax -> argmax / log / mul / sum / max of make_regularized_pseudo_label (deprecated/train_with_test_pt_pseudo_entropy_reg.py:30-39),
 * score_mask (train_vqreptunet1x1v2.py:43-46) and the entropy map of VQRePTUnet1x1.forward (net.py:1199-1201). */
int vqseg_softmax_stats_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px, int b, int c,
                          int64_t hw, int64_t* label, float* entropy, float* top, void* stream);

/* Confusion counts per image: counts[b][t][p] = number of pixels with ground truth t (in [0, c); others skipped) and
 * arg-max class p (first maximum).  Replaces Measurement._make_confusion_matrix (measurement.py:12-20: np.bincount of
 * c * target + pred on the host) without the host round trip torch.bincount needs.  logits layout as for the Dice
 * sums; 2..4 classes; counts [b][c][c] i64, overwritten. */
int vqseg_confusion_counts_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                             const int64_t* target, int b, int c, int64_t hw, int64_t* counts, void* stream);

/* Focal loss of loss/focal_loss.py:6-50 in one pass over the logits (layout, 2..4 classes and int64 targets as for the Dice
 * sums).  Per pixel, with keep = target != ignore_index:
 *   z = keep ? logits : 0,  t = keep ? target : 0,  p = softmax(z),  l = alpha * w[t] * (1 - p_t)^gamma * (-log p_t)
 * with -log p_t in log-softmax form (log sum exp(z - max) + max - z_t) and w = `weight`, C floats in DEVICE memory, or NULL = 1.
 * The reference's quirks are kept: an ignored pixel is not skipped but a zero-logit class-0 pixel that contributes
 * alpha * w[0] * (1 - 1/C)^gamma * log C (:12-14); 'mean' divides by all b * hw pixels (:43); the weights normalise nothing
 * (:42 is overwritten by :43).  pre_softmax != 0 is the MODULE FocalLoss.forward (:62-68), which softmaxes before calling
 * focal_loss: z = keep ? softmax(logits) : 0, then the same; backward goes through both softmaxes in closed form.
 * A target outside [0, c) other than ignore_index contributes 0 (the reference raises).  gamma == 0 or gamma >= 1 (between
 * the two the derivative is unbounded at p_t = 1: rejected); integer gamma <= 4 is evaluated by multiplications.
 *   forward : per_image[b] = sum_px l in double (block partials folded in block order), loss2[0] = sum_b per_image[b]
 *             ('sum'), loss2[1] = that / (b * hw) ('mean'); loss_map (nullable) [b][hw] = l ('none').
 *   backward: g_logits (the logits' layout) = d (sum_px g l) / d logits with g = g_scalar[0] * scale (DEVICE scalar; scale = 1
 *             for 'sum', 1 / (b * hw) for 'mean') or g = g_map[b][px]; exactly one of g_scalar / g_map.  Ignored pixels: 0.
 * workspace: vqseg_focal_workspace_bytes(b, hw) (also what vqseg_wce_sums_forward_f needs). */
size_t vqseg_focal_workspace_bytes(int b, int64_t hw);
int vqseg_focal_forward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                          const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index, const float* weight,
                          float alpha, float gamma, int pre_softmax, void* workspace, size_t workspace_bytes,
                          double* per_image, float* loss2, float* loss_map, void* stream);
int vqseg_focal_backward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                           const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index, const float* weight,
                           float alpha, float gamma, int pre_softmax, const float* g_scalar, float scale,
                           const float* g_map, float* g_logits, void* stream);

/* Class-weighted cross-entropy sums of F.cross_entropy(logits, target, weight=w, ignore_index) with w in DEVICE memory:
 *   ce[b][0] = sum over kept pixels of w[t] * (-log softmax(logits)[t]),  ce[b][1] = sum over kept pixels of w[t];
 * the weighted mean is sum_b ce[b][0] / sum_b ce[b][1] on the caller's side.  backward: g_logits = g_ce[b][0] * w[t] *
 * (softmax - onehot) on kept pixels, 0 elsewhere (g_ce [b][2], [b][0] used).  Layout as for the Dice sums. */
int vqseg_wce_sums_forward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                             const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index, const float* weight,
                             void* workspace, size_t workspace_bytes, float* ce, void* stream);
int vqseg_wce_sums_backward_f(const float* logits, int64_t stride_b, int64_t stride_c, int64_t stride_px,
                              const int64_t* target, int b, int c, int64_t hw, int64_t ignore_index, const float* weight,
                              const float* g_ce, float* g_logits, void* stream);

/* compute_class_weight of loss/__init__.py:28-33 without torch.bincount's host round trip: counts[c] = number of labels
 * equal to c for c < num_classes, counts[num_classes] = number of labels >= 0 (bincount's total: a label >= num_classes grows
 * its vector, so it counts in the sum, but has no entry here; negative labels, which bincount refuses, are skipped), and
 *   weight[c] = 1 - (float)counts[c] / (float)counts[num_classes]                                      (float32, as torch divides)
 * counts [num_classes + 1] i64 and weight [num_classes] f32, both overwritten; 1..256 classes. */
int vqseg_class_weight_f(const int64_t* labels, int64_t n, int num_classes, int64_t* counts, float* weight, void* stream);

/* Exact order statistics of n floats by radix select: out2[0] = the k-th smallest (0-based), out2[1] = the (k+1)-th
 * (clamped to the last).  The two values bracket the virtual index of np.percentile in make_regularized_pseudo_label
 * (deprecated/train_with_test_pt_pseudo_entropy_reg.py:35); the host interpolates.  Replaces the full device sort of
 * torch.quantile (and its 2^24-element input limit).  0 <= k < n < 2^32. */
/* The loss combination of a CPS iteration in ONE launch (r4; train_vqreptunet1x1v2.py:165-192: sup_1 + sup_2 + cps_weight * (cps_1 +
 * cps_2) + commitment + prototype, each supervised / CPS term = ce_weight * CE + Dice loss from the sums of vqseg_dice[_ce]_sums_*):
 *   term_i = ce_weight * ce_i[:, 0].sum() / ce_i[:, 1].sum() + (1 - mean_c mean_b 2 inter_i / (sets_i + eps))     (dice_loss.py:27-37)
 *   commitment = sum_l (sum_k commit[k][l]) * commit_weight,  prototype = (sum_k *proto[k]) * proto_weight  (float64 inputs)
 *   out[0] = total, out[1] = commitment, out[2] = prototype, out[3] = cps_1 + cps_2, out[4 + i] = term_i (supervised terms first)
 * and the gradient of the total with respect to every inter / sets / ce entry (g_*: same shapes; the commitment / prototype inputs'
 * gradients are the constants commit_weight / proto_weight).  It replaces ~45 scalar autograd nodes forward and ~70 tiny kernels
 * backward that ran one by one with the GPU idle.  ce / g_ce (and their entries) nullable: no cross-entropy part.  Pointer arrays
 * are host arrays of device pointers. */
int vqseg_cps_loss_combine_f(int n_sup, int n_cps, int c, const float* const* inter, const float* const* sets, const float* const* ce,
                             const int* b, float cps_weight, float ce_weight, float eps, const float* const* commit, int n_commit,
                             int levels, float commit_weight, const double* const* proto, int n_proto, float proto_weight,
                             float* const* g_inter, float* const* g_sets, float* const* g_ce, float* out, void* stream);
size_t vqseg_order_stats_workspace_bytes(void);
int vqseg_order_stats_f(const float* x, int64_t n, int64_t k, void* workspace, size_t workspace_bytes, float* out2,
                        void* stream);

/* ---------------------------------------------------------------------------------- *
 * The optimiser step: torch.optim.Adam(model.parameters(), lr, betas=(0.9, 0.999)) created at train_vqreptunet1x1v2.py:106-107
 * and stepped at :200-201 (eps 1e-8, no weight decay, no amsgrad), for ALL parameters of a network in ONE launch, with the
 * kernel-side bf16 images of the k x k convolution weights (the three images of vqseg_conv_pack_all_f32) rewritten in the same
 * pass from the freshly updated values.  fp32 arithmetic in the operation order of torch/optim/adam.py::_single_tensor_adam:
 *     m = fma(1 - b1, g - m, m);  v = fma((1 - b2) g, g, v b2);  p = p + (-(lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * (`step` = t >= 1, the value AFTER this step's increment; the scalars are evaluated in double like torch's Python floats).
 *   params_dev [n_params] VqsegAdamParam records in DEVICE memory; items_dev [n_items][2] int32 (parameter index, tile index) in
 *   DEVICE memory: for every parameter its vqseg_adam_work_items() tiles 0 .. count-1, in any order.
 *   k = 0: plain parameter, tiles are flat chunks of VQSEG_ADAM_CHUNK elements;
 *   k = 1 / 3: nn.Conv2d weight [cout][cin][k][k], tiles of 32 output x 128 / 32 input channels; fwd / tr / s3 (each nullable):
 *   the images [cout][k][k][cin^32], [cin][k][k flipped][cout^32], [cout][k][k][3 cin] ([w_hi | w_hi | w_lo] per concat segment
 *   split at c1; needs cin % 32 == 0 and c1 % 32 == 0) -- bit-identical to vqseg_conv_pack_all_f32 of the updated weight.
 * Preconditions the entry point cannot check (the tables live in device memory): p / g / m / v hold numel floats each and do not
 * overlap (4-byte alignment is enough; a parameter whose four pointers are all 16-byte aligned takes 16-byte accesses, with
 * bit-identical results); for k = 1 / 3 numel == cout * cin * k * k; every non-NULL image is 16-byte aligned and holds
 * cout k k cin^32 / cin k k cout^32 / cout k k 3 cin 16-bit elements; 0 < c1 <= cin; every (parameter, tile) pair appears exactly once
 * (a parameter with numel == 0 has no tile).  Arithmetic is IEEE float32 with subnormals (no flush to zero): NaN / Inf gradients
 * propagate into m, v and p of their own element only.  The image outputs of the pack entry points above must be 16-byte aligned too.
 * ---------------------------------------------------------------------------------- */
#define VQSEG_ADAM_CHUNK 4096
typedef struct VqsegAdamParam {
    float* p;            /* parameter        [numel] f32, updated in place */
    const float* g;      /* gradient         [numel] f32 */
    float* m;            /* exp_avg          [numel] f32, updated in place */
    float* v;            /* exp_avg_sq       [numel] f32, updated in place */
    int64_t numel;
    int32_t k, cout, cin, c1;
    void* fwd;
    void* tr;
    void* s3;
} VqsegAdamParam;
int64_t vqseg_adam_work_items(int64_t numel, int k, int cout, int cin);
int vqseg_adam_step_f32(const VqsegAdamParam* params_dev, const int32_t* items_dev, int n_items, double lr, double beta1,
                        double beta2, double eps, int64_t step, void* stream);

/* The same launch with an exponential moving average ("teacher") of the network kept in the same pass: ema_dev holds one
 * VqsegEmaParam per VqsegAdamParam record, same index.  With p' the float32 parameter value this launch has just stored and
 * w = (float)(1.0 - ema_decay) (formed in double, cast once):
 *     average:  e' = fmaf(w, p' - e, e)      (the difference rounded once, the fma rounded once; IEEE float32 with subnormals)
 *     copy:     e' = the stored bits of p'   (a record whose `copy` is non-zero, or every record when copy_all != 0; e is not read)
 * and the teacher's images fwd / tr / s3 (each nullable) are written from e' in the layouts, sizes and alignment rules of the
 * student's (k, cout, cin, c1 of the VqsegAdamParam record).  A record with e == NULL behaves exactly as under vqseg_adam_step_f32.
 * Average-only records: under THIS entry point a record with g == NULL skips the Adam rule -- p is read only, m and v may be NULL,
 * only e and its images are produced (BatchNorm running statistics).  Under vqseg_adam_step_f32 g == NULL stays a precondition
 * violation.  Tiles, chunk size, item table and the other preconditions are those of vqseg_adam_step_f32; e holds numel floats and
 * overlaps none of p / g / m / v (a flat record takes 16-byte accesses when e and the record's other pointers are all 16-byte
 * aligned, with bit-identical results).  ema_decay must lie in [0, 1). */
typedef struct VqsegEmaParam {
    float* e;            /* averaged values  [numel] f32, updated in place; NULL: this record keeps no average */
    int32_t copy;        /* non-zero: e takes the NEW p bit for bit instead of the average */
    int32_t reserved;    /* 0 */
    void* fwd;           /* images of e, each nullable */
    void* tr;
    void* s3;
} VqsegEmaParam;
int vqseg_adam_ema_step_f32(const VqsegAdamParam* params_dev, const VqsegEmaParam* ema_dev, const int32_t* items_dev, int n_items,
                            double lr, double beta1, double beta2, double eps, int64_t step, double ema_decay, int copy_all,
                            void* stream);

/* ---------------------------------------------------------------------------------- *
 * Batch assembly of the device-resident data loader (vq_seg_amd.data.DeviceLoader): the per-sample work of BaseDataset.__getitem__
 * after its decode / resize (data/dataset.py:47-57: uint8 HWC -> float32 / 255, the raw uint8 mask) and of the loop's
 * img_to_label (utils/seg_tools.py:3-8) for n samples cached in HBM.
 *   img_cache           ragged uint8 cache: sample i's (h, w, 3) image at byte img_offsets_host[i] (HOST array of n offsets)
 *   mask_cache          ragged uint8 cache: sample i's (mh, mw) mask at byte mask_offsets_host[i]; NULL for the unlabelled split
 *   f32_lut    [256]    f32: the value of each byte (the host's uint8 -> float32 / 255, so the result does not depend on a division here)
 *   label_lut  [256]    i64: img_to_label of each byte value; NULL: no label output
 *   img_out    [n, h, w, 3]   f32 out (NHWC: torch channels_last of (n, 3, h, w))
 *   target_out [n, mh, mw]    u8 out (NULL iff mask_cache is NULL);  label_out [n, mh, mw] i64 out (NULL iff label_lut is NULL)
 * The offsets travel as kernel arguments (no host-to-device copy per batch); n above the argument block's capacity splits into
 * several launches.  A wave moves a 1 KiB tile of one sample per iteration: whole tiles with 16-byte f32 stores that are contiguous
 * across the wave (pointers 16-byte, offsets 4-byte aligned, the sample's output position a multiple of 4 elements), a sample's
 * partial last tile (and any tile without that alignment) byte by byte.  Bit-exact by construction (a table lookup and copies). */
int vqseg_batch_u8_f(int n, const uint8_t* img_cache, const uint8_t* mask_cache, const int64_t* img_offsets_host,
                     const int64_t* mask_offsets_host, int h, int w, int mh, int mw, const float* f32_lut, const int64_t* label_lut,
                     float* img_out, uint8_t* target_out, int64_t* label_out, void* stream);

/* Box mix: CutMix / CutOut of a batch in one pass (vq_seg_amd.data.augmentations; the reference's CutMix.__call__ and augmentation(),
 * data/augmentations.py:11-30, 62-73: batch[i] * mask + batch[(i + 1) % B] * (1 - mask) with a 0 / 1 box mask).  For a tensor of logical
 * shape (n, planes, h, w):
 *     out[s, p, y, x] = inside(box[s], y, x) ? (mode 0 MIX: src[(s + 1) % n, p, y, x] | mode 1 FILL: fill) : src[s, p, y, x]
 * a selection by bits (no arithmetic): one kernel per element width (elem_bytes 1, 2, 4, 8: uint8, bf16, f32, int64).
 *   src, out            out of place, the same layout; src is never written
 *   stride_s/_p/_px     sample, plane and pixel strides in ELEMENTS (as vqseg_softmax_stats_f takes them), rows dense: planar (pixel stride 1,
 *                       plane stride h * w: NCHW-contiguous, and 3-D label maps with planes = 1) or interleaved (plane stride 1, pixel
 *                       stride planes: channels_last); anything else is VQSEG_EINVAL
 *   boxes_host [n][4]   HOST array of (y1, x1, cut_h, cut_w) per sample; 0 <= y1, y1 + cut_h <= h, likewise x; cut_h or cut_w 0: empty box.
 *                       The boxes travel as kernel arguments (64 samples per launch; the kernel sees the whole src and its block's first
 *                       sample, since a sample's partner may belong to another block): no host-to-device copy, no synchronisation
 *   fill_bits           mode 1: the fill value's bit pattern in the low elem_bytes bytes
 * HBM-bound: one read and one write per element.  16-byte loads / stores where a sample starts on a 16-byte boundary (an edge of the
 * box inside a 16-byte unit is exact), element-wise and coalesced elsewhere.  Grid capped by option "nn_grid_cap". */
int vqseg_box_mix_f(int mode, int elem_bytes, const void* src, void* out, int n, int planes, int h, int w, int64_t stride_s,
                    int64_t stride_p, int64_t stride_px, const int32_t* boxes_host, uint64_t fill_bits, void* stream);

/* Affine warp: a whole batch resampled out of place in one pass, one 2 x 2 matrix per sample (vq_seg_amd.data.augmentations:
 * similarity_transform / inverse_similarity_transform / warp_batch; the reference's flips and TF.rotate, data/augmentations.py:108-148,
 * TF.rotate on tensors being grid_sample with align_corners=False and zero padding).  For output pixel (x, y) of an h x w image, with
 * cx = (w - 1) / 2, cy = (h - 1) / 2, dx = x - cx, dy = y - cy:
 *     xs = (M00 * dx + M01 * dy) + cx        ys = (M10 * dx + M11 * dy) + cy          (f32, this order, no FMA contraction)
 * so for M with entries in {0, +-1} every (xs, ys) is an exact integer.
 *   mode 0 BILINEAR     elem_bytes 4 (f32) or 2 (bf16): four taps, weights from xs - floor(xs), ys - floor(ys), f32 accumulation, bf16 rounded
 *                       once (nearest even); a tap outside the image contributes nothing (zero padding); a tap of weight exactly zero is not
 *                       read, and an integer (xs, ys) is copied by bits: identity, flips and quarter turns pass every bit pattern through
 *   mode 1 NEAREST      elem_bytes 1, 2, 4, 8 (uint8 ... int64 label maps, anything by bits): source pixel (rintf(xs), rintf(ys)), round half
 *                       to even; a source outside the image gives fill_bits (its low elem_bytes bytes)
 *   src, out            out of place; the same layout, each with its own sample stride (ELEMENTS, >= planes * h * w when n > 1)
 *   stride_p/_px        plane and pixel strides in ELEMENTS, rows dense, as vqseg_box_mix_f takes them: planar (pixel stride 1, plane stride
 *                       h * w) or interleaved (plane stride 1, pixel stride planes); anything else is VQSEG_EINVAL
 *   matrices_host [n][6] HOST rows (M00, M01, 0, M10, M11, 0): the layout of a 2 x 3 affine matrix whose translation slots are reserved and
 *                       must be 0; every entry finite.  The matrices travel as kernel arguments (64 samples per launch): no device
 *                       allocation, no host-to-device copy, no synchronisation
 * A gather bound by HBM / L2: a 256-thread workgroup takes a 2-D tile of output pixels, so that the rotated source footprint's cache lines
 * are reused inside the tile and the stores stay coalesced; coordinates and weights once per pixel for all its planes.  h, w <= 2^24.
 * Grid capped by option "nn_grid_cap". */
int vqseg_affine_warp_f(int mode, int elem_bytes, const void* src, void* out, int n, int planes, int h, int w, int64_t src_stride_s,
                        int64_t out_stride_s, int64_t stride_p, int64_t stride_px, const float* matrices_host, uint64_t fill_bits,
                        void* stream);

/* Prediction: bilinear resize (align_corners = 0) of class logits to ho x wo, the mean over n_views logit tensors, arg-max, top
 * probability and confusion counts in one pass, without the (b, c, ho, wo) tensor in between (vq_seg_amd.nnf.resize_argmax,
 * vq_seg_amd.predict, evaluate.test_loop(fused=True)).  Per output pixel (y, x):
 *     a_v   = bilinear interpolation of view v at (y, x), per class     (the arithmetic of vqseg_bilinear_f, bit for bit)
 *     acc   = a_0 (+ a_1 (+ a_2 + a_3))   plain f32 adds in view order;  n_views > 1: acc *= 1 / n_views
 *     label = first maximum of acc over the classes (a NaN never wins; all-NaN gives class 0)
 *     top   = 1 / sum_c expf(acc_c - max)                               (the top probability of vqseg_softmax_stats_f)
 *     counts[b][t][label] += 1  where t = target[b][y][x] lies in [0, c)   (others skipped, as vqseg_confusion_counts_f)
 * With one view and no flip, label / top / counts equal what vqseg_softmax_stats_f and vqseg_confusion_counts_f give on the output of
 * vqseg_bilinear_f, bit for bit.
 *   views_host [n_views]  HOST array of device pointers: f32 logits of logical shape (b, c, h, w), all with the strides below
 *   flips_host [n_views]  HOST array of flip codes 0..3: bit 0 flips the columns, bit 1 the rows of that view before it is resized -- an
 *                         index map on the source grid (tap column i reads w - 1 - i), the weights do not change
 *   n_views               1, 2 or 4 (1 / n_views exact); anything else is VQSEG_EINVAL
 *   stride_b/_c/_px       batch, class and pixel strides in ELEMENTS (as vqseg_softmax_stats_f takes them), rows dense: planar (pixel
 *                         stride 1, class stride h * w) or interleaved (class stride 1, pixel stride c); 2..4 classes
 *   label  [b][ho][wo] u8 out, top [b][ho][wo] f32 out, counts [b][c][c] i64 out (overwritten; rows = ground truth): each may be NULL,
 *                         not all three;  target [b][ho][wo] i64, non-NULL iff counts is
 * Pointers and flip codes travel as kernel arguments: no device allocation, no host-to-device copy, no synchronisation.  A wave takes
 * 256 consecutive output pixels, four per lane and 64 apart, so that its gathers, its top stores and its target loads each cover 64
 * adjacent pixels; the u8 labels are packed across lanes into one 4-byte store per lane.  Counts go through wave ballots, a
 * per-workgroup LDS histogram and integer atomics (order-independent).  Source images up to 2^27 pixels, outputs up to 2^30.  Grid
 * capped by option "nn_grid_cap". */
int vqseg_resize_argmax_f(const float* const* views_host, const int* flips_host, int n_views, int64_t stride_b, int64_t stride_c,
                          int64_t stride_px, int b, int c, int h, int w, int ho, int wo, uint8_t* label, float* top,
                          const int64_t* target, int64_t* counts, void* stream);

/* Tiled (sliding-window) prediction: the network runs on native-resolution windows of an image and overlapping windows are blended
 * (vq_seg_amd.nnf.extract_windows / merge_argmax, vq_seg_amd.predict.Predictor(window=...)).  The window rule, per axis, which host and
 * device share (vq_seg_amd.nnf.window_starts):
 *     n = ceil((extent - window) / stride) + 1,   start[k] = min(k * stride, extent - window),   1 <= stride <= window <= extent
 * The last window is clamped to end at the border.  A grid is ny x nx windows per image, row-major (t = j * nx + i); window rows are
 * image-major (row = b * T + t, T = ny * nx).  Both entry points take (extent, window, stride) per axis and derive the starts: there is
 * no start table and no cap on the number of windows.  Windows up to 4096 a side (the linear blend's weights and their products
 * are then exact f32 integers; their sum ws is an f32 running sum in the order stated below, exact while it stays below 2^24 --
 * strides near window / 2 -- and rounded like any other f32 sum beyond that).
 *
 * vqseg_extract_windows_f: images f32 logical (b, 3, h, w), batch / channel / pixel strides in ELEMENTS as vqseg_resize_argmax_f takes
 * them (planar or interleaved, rows dense) -> out [n_flips][b * T][3][nh][nw] f32.  Every window's crop (wh x ww image pixels at its
 * start) is resized bilinearly (align_corners = 0, the arithmetic of vqseg_bilinear_f, bit for bit) to the network's size nh x nw with
 * the taps clamped INSIDE the window, and stored once per flip code of flips_host (0..3: bit 0 columns, bit 1 rows; an index map on
 * the output).  With (wh, ww) == (nh, nw) the crop is copied exactly.  Down-scaling is ATen's un-antialiased rule (two taps per axis
 * whatever the factor), as everywhere in this library.  Pointers and scalars travel as kernel arguments: no device allocation, no
 * host-to-device copy, no synchronisation.  Images and network inputs up to 2^27 pixels.  Grid capped by option "nn_grid_cap".
 *
 * vqseg_merge_argmax_f: n_views (1, 2 or 4) f32 logit tensors of logical shape (b * T, c, lh, lw), window rows stride_b ELEMENTS apart,
 * planar or interleaved as vqseg_resize_argmax_f takes them, one flip code per view -> label / top / counts at ho x wo.  For output
 * pixel (y, x) of image b and view v:
 *     acc = 0, ws = 0
 *     for j ascending over the windows with ys[j] <= y < ys[j] + wh,  for i ascending over those with xs[i] <= x < xs[i] + ww:
 *         s   = bilinear sample (align_corners = 0, lh x lw -> wh x ww, the arithmetic of vqseg_bilinear_f) of the un-flipped view's
 *               row b * T + j * nx + i at the local position (y - ys[j], x - xs[i])
 *         w   = wy(y - ys[j]) * wx(x - xs[i]);   acc = fmaf(w, s, acc);   ws += w
 *     m_v = acc / ws                                                     (IEEE f32 division)
 *     z   = m_0 (+ m_1 (+ m_2 + m_3)) in view order;  n_views > 1: z *= 1 / n_views
 * blend VQSEG_BLEND_UNIFORM: w = 1;  VQSEG_BLEND_LINEAR: wy(r) = min(r + 1, wh - r), wx(r) = min(r + 1, ww - r) -- integers.
 * label, top and counts from z, their NULL rules, target and the argument errors: exactly as vqseg_resize_argmax_f.  With one window
 * per image and the uniform blend the result is vqseg_resize_argmax_f's, bit for bit; with disjoint windows and the uniform blend it is
 * vqseg_resize_argmax_f of every window on its own, pasted together.  Kernel shape as vqseg_resize_argmax_f (a wave takes 256 consecutive
 * output pixels, four per lane and 64 apart; packed label stores; ballots, LDS histogram and integer atomics for the counts); the
 * window loops run between per-pixel bounds that change only at window edges.  Window logits up to 2^27 pixels, outputs up to 2^30.
 * Grid capped by option "nn_grid_cap". */
#define VQSEG_BLEND_UNIFORM 0
#define VQSEG_BLEND_LINEAR 1
int vqseg_extract_windows_f(const float* images, int64_t stride_b, int64_t stride_c, int64_t stride_px, int b, int h, int w, int wh, int ww,
                            int sy, int sx, int nh, int nw, const int* flips_host, int n_flips, float* out, void* stream);
int vqseg_merge_argmax_f(const float* const* views_host, const int* flips_host, int n_views, int64_t stride_b, int64_t stride_c,
                         int64_t stride_px, int b, int c, int lh, int lw, int ho, int wo, int wh, int ww, int sy, int sx, int blend,
                         uint8_t* label, float* top, const int64_t* target, int64_t* counts, void* stream);

/* Visualisation: the RGB bytes of a panel sheet for a batch in one pass (vq_seg_amd.nnf.render_sheet, vq_seg_amd.utils.visualize,
 * Predictor.render).  The full-resolution sheet is rows = b * ho by cols pixels; image i takes rows i * ho .. (i + 1) * ho - 1 of every
 * panel, panel p the columns x0[p] .. x0[p] + width[p] - 1.  Panel kinds:
 *     0 IMAGE       the image resized bilinearly (align_corners = 0, the arithmetic of vqseg_bilinear_f) to ho x wo
 *     1 TARGET      palette row t (the target, brought to ho x wo by ATen's nearest rule), row 2 c (`ignore`) for t outside [0, c)
 *     2 PRED        palette row pr (the pred byte), row 2 c for pr >= c
 *     3 DETAIL      palette row pr + c * [pr != t]  (a target outside [0, c) makes the pixel wrong), row 2 c for pr >= c
 *     4 MIX_PRED    clip(image * (1 - alpha) + colour(PRED) * alpha, 0, 1)       f32: two products, one add
 *     5 MIX_DETAIL  clip(image * (1 - alpha) + colour(DETAIL) * alpha, 0, 1)
 *     6 FILL        the fill colour, any width
 * Every panel but FILL is wo wide.  A byte is floor(clip(x, 0, 1) * 255) in f32, 0 for a NaN; TARGET / PRED / DETAIL / FILL pixels write
 * the u8 palette rows as given.  box2: the canvas is the sheet halved in both directions, every canvas pixel the f32 mean
 * ((c00 + c01) + (c10 + c11)) * 0.25 of its 2 x 2 sheet pixels' float colours, quantised after the mean (four pixels of one palette row
 * write that row's u8 colour); rows and cols must be even.
 *   image   f32 logical (b, 3, h, w), batch / channel / pixel strides in ELEMENTS as vqseg_resize_argmax_f takes them (planar or
 *           interleaved, rows dense); pred u8 [b][ho][wo]; target i64 [b][ht][wt]: each may be NULL when no panel needs it
 *   kinds_host / x0_host / width_host [n_panels]  HOST arrays, 1..8 panels, in any order, disjoint, inside the sheet
 *   palette_f_host [2 c + 1][3] f32 HOST: c class colours, c "wrong" colours, the ignore colour; palette_u8_host the same rows as
 *           bytes (floor(colour * 255) taken in float64 by the caller); fill_f_host [3] / fill_u8_host [3] the FILL colour; c in 2..4
 *   canvas  u8 out, interleaved RGB, pitch bytes per row (>= 3 * canvas columns); rows / cols: the FULL-RESOLUTION sheet (rows = b * ho);
 *           with box2 the canvas holds rows / 2 by cols / 2 pixels.  Only bytes of panel pixels are written.
 * Panels and palette travel as kernel arguments: no device allocation, no host-to-device copy, no synchronisation.  A lane takes 4
 * adjacent canvas pixels (three 4-byte stores when canvas and pitch are 4-byte aligned, byte stores otherwise), a wave 64 consecutive
 * such groups.  Images up to 2^27 pixels, sheets up to 2^30.  Grid capped by option "nn_grid_cap". */
int vqseg_render_sheet_u8(const float* image, int64_t stride_b, int64_t stride_c, int64_t stride_px, int h, int w, const uint8_t* pred,
                          const int64_t* target, int ht, int wt, int b, int ho, int wo, int c, const int* kinds_host, const int* x0_host,
                          const int* width_host, int n_panels, const float* palette_f_host, const uint8_t* palette_u8_host,
                          const float* fill_f_host, const uint8_t* fill_u8_host, float alpha, int box2, uint8_t* canvas, int64_t pitch,
                          int rows, int cols, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Pixel-pair supervised contrastive loss (loss/contrastive_loss.py:9-30; vq_seg_amd.nnf.supcon, vq_seg_amd.loss.SupConLoss) of the
 * feature rows f1, f2 ([h * w][c], f32 or bf16 by the `bf16` flag, row_stride elements apart: images 0 and 1 of a channels_last
 * tensor) and their int64 targets gt1, gt2 ([ht][wt] each; larger than the feature map: read through ATen's `nearest` rule):
 *     z_ij = (f1_i . f2_j) / T,  pos_ij = (gt1_i == gt2_j)  -- the target VALUES are compared, 255 is a class like any other --
 *     logA = log sum_ij exp z_ij,  logP = log sum_pos exp z_ij,  loss = (logA - logP) / (hw * hw)
 * The (hw, hw) matrix is never written: an MFMA product over all row pairs (v_mfma_f32_32x32x2_f32 for f32 rows, v_mfma_f32_32x32x16_bf16
 * for bf16 rows) reduced on the fly with a running maximum and a rescaled sum per row -- one pair over all columns, one over the positives --, so the value is finite at every finite input
 * (the reference's exp overflows at z > 88) and equal to the reference's wherever that is finite.  No atomics: per-row partials of
 * every column split go to the workspace and ONE workgroup merges them in a fixed order in double; two calls agree bit for bit.
 *   forward : out[0] = loss (+inf when there is no positive pair, as the reference), out[1] = logA, out[2] = logP, out[3..7] = what the
 *             backward reads (the base-2 logs as hi + lo floats, and whether a positive pair exists); out: 8 floats, DEVICE.
 *   backward: dz_ij = g / (hw * hw) * (exp(z_ij - logA) - pos_ij exp(z_ij - logP)),  d_f1 = dz f2 / T,  d_f2 = dz^T f1 / T, with
 *             g = g_scalar[0] read on the DEVICE (under a gradient scaler it holds the scale); `stats` is the forward's `out`.  The
 *             z tile is recomputed; one kernel, launched twice with the roles of the images swapped, accumulates the gradient of
 *             the rows it owns over all columns.  Gradients leave in the rows' type, grad_row_stride elements apart.  No positive
 *             pair: the positive term is absent and the gradient finite (the reference: NaN).
 * c: a multiple of 16 up to 128; h * w <= 2^30; rows 16-byte aligned.  workspace: vqseg_supcon_workspace_bytes(h * w).
 * ---------------------------------------------------------------------------------- */
size_t vqseg_supcon_workspace_bytes(int64_t hw);
int vqseg_supcon_forward_f(int bf16, const void* f1, const void* f2, int64_t row_stride, int h, int w, int c, const int64_t* gt1,
                           const int64_t* gt2, int ht, int wt, float temperature, void* workspace, size_t workspace_bytes, float* out,
                           void* stream);
int vqseg_supcon_backward_f(int bf16, const void* f1, const void* f2, int64_t row_stride, int h, int w, int c, const int64_t* gt1,
                            const int64_t* gt2, int ht, int wt, float temperature, const float* stats, const float* g_scalar, void* d_f1,
                            void* d_f2, int64_t grad_row_stride, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Confidence-weighted soft cross-pseudo-supervision loss (conf_ce_loss of deprecated/train_vq_pt_unet_conf_ce.py:50-113;
 * vq_seg_amd.nnf.conf_ce / conf_ce_pair, vq_seg_amd.loss.conf_ce_loss) of INPUT logits x and TARGET logits t, both logical
 * (b, c, hw) f32 with 2..4 classes, each addressed through its own batch / class / pixel strides in ELEMENTS (NCHW or channels_last,
 * as the Dice sums take them).  Per pixel, q = softmax(t), w = max q, k = first arg-max of t, p = softmax(x):
 *     pos = w * (logsumexp(x) - x_k), summed over the M pixels with w >= threshold
 *     n_c = -[c != k'] log clamp(1 - p_c, 1e-7, 1), summed over the Mn elements with softmax(t / temperature)_c < threshold_neg
 *           (k' = first arg-max of t / temperature; the element c == k' adds 0 but counts)
 *     loss = sum pos / M + [threshold_neg > 0] (sum n / Mn + 0.5 sum p_c^2 / (b c hw)),   a sum over nothing divided by 0 is 0
 * 1 - p_c is (sum of the other classes' exponentials) / (sum of all), never a subtraction.  pair = 1: stats / loss slot 0 is
 * loss(x <- t), slot 1 is loss(t <- x), the roles swapped, from one read of both tensors.
 *   forward : stats [pair + 1][8] f64 DEVICE = (sum pos, sum n, sum p^2, M, Mn, 1/M or 0, 1/Mn or 0, loss); loss [pair + 1] f32.
 *             Block sums in double and integer counts, folded in a fixed order by one workgroup: no atomics, two calls agree
 *             bit for bit; nothing returns to the host.  workspace: vqseg_conf_ce_workspace_bytes(b, hw), 8-byte aligned.
 *   backward: `stats` as the forward wrote it, g_scalar [pair + 1] f32 DEVICE (the upstream scalar of each slot).
 *             pair = 0: g_x = g[0] d loss / d x; g_t = g[0] d loss / d t -- the path through the weight w: the targets are NOT
 *             detached -- unless detach_targets (then g_t may be NULL and is not written).
 *             pair = 1: g_x = g[0] d loss(x <- t) / d x + g[1] d loss(t <- x) / d x, g_t likewise; detach_targets drops the
 *             target-side half of each.  Masks and arg-maxes are constants.  g_x takes x's strides, g_t takes t's.
 * temperature > 0, threshold_neg >= 0, b <= 65535.
 * ---------------------------------------------------------------------------------- */
size_t vqseg_conf_ce_workspace_bytes(int b, int64_t hw);
int vqseg_conf_ce_forward_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const float* t, int64_t t_stride_b,
                            int64_t t_stride_c, int64_t t_stride_px, int b, int c, int64_t hw, float threshold, float threshold_neg,
                            float temperature, int pair, void* workspace, size_t workspace_bytes, double* stats, float* loss, void* stream);
int vqseg_conf_ce_backward_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const float* t, int64_t t_stride_b,
                             int64_t t_stride_c, int64_t t_stride_px, int b, int c, int64_t hw, float threshold, float threshold_neg,
                             float temperature, int pair, int detach_targets, const double* stats, const float* g_scalar, float* g_x,
                             float* g_t, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Fully connected CRF refinement of class probabilities (utils/crf.py: DenseCRF; vq_seg_amd.nnf.dense_crf,
 * vq_seg_amd.utils.crf.DenseCRF, vq_seg_amd.predict.Predictor(crf=...)): mean-field inference with a Potts compatibility and
 * symmetrically normalised kernels, computed EXACTLY over all pixel pairs of a truncated support -- no lattice, no approximation of
 * the filter.  Inference only.  Per image, pixels i, j at integer (x, y), c in 2..4 classes:
 *     rgb      = trunc(clamp(image, 0, 1) * 255)  (the product in f32), integers 0..255;   U = -log(clip(prob, 1e-5, 1))
 *     k_pos    = exp(-(dx^2 + dy^2) / (2 pos_xy_std^2))                                                 inside |dx|, |dy| <= R_pos
 *     k_bi     = exp(-(dx^2 + dy^2) / (2 bi_xy_std^2) - |rgb_i - rgb_j|^2 / (2 bi_rgb_std^2))            inside |dx|, |dy| <= R_bi
 *     R        = ceil(truncate * xy_std) of that kernel (in double); k = 0 outside its support; both include j = i;
 *                truncate = +inf: full support.  The truncation is part of the definition.
 *     n_i      = 1 / sqrt(sum_j k(i, j) + 1e-20)  per kernel;      m_i[c] = n_i sum_j k(i, j) n_j Q_j[c]
 *     E_i      = -U_i + pos_w m_pos,i + bi_w m_bi,i;   Q_i = softmax_c(E_i);   Q^0 = softmax(-U) = clip(prob) / sum_c clip(prob)
 * All buffers are the caller's, none larger than b * c * h * w elements; internal layout planar: rgb u32 [b][h * w] (r | g << 8 |
 * b << 16), unary / q [b][c][h * w] f32, norm_pos f32 [h * w] (the same for every image), norm_bi f32 [b][h * w], table f32 [w + h].
 *
 * vqseg_crf_prepare_f: image f32 logical (b, 3, h, w) and prob f32 logical (b, c, h, w), each through its own batch / channel / pixel
 * strides in ELEMENTS as vqseg_resize_argmax_f takes them (planar or interleaved, rows dense) -> rgb, unary, q0 and, when
 * iter_max > 0, both kernels' n_i: the positional one from its separable row and column sums (table, taken in double), the bilateral
 * one from an all-pairs pass of its own.  iter_max = 0: norm_pos, norm_bi and table may be NULL and are not written.
 *
 * vqseg_crf_step_f: one update q_in -> q_out (two different buffers: ping-pong) for all b images in one launch; energies != 0 writes
 * E instead of Q (the last launch of a caller that wants logits: softmax(E) = Q).  A workgroup owns 8 x 64 pixels i and streams the
 * pixels j of its window through LDS; it touches the pairs inside the larger support plus the tile's overhang, never all (h w)^2; both
 * kernels share that one pass, the positional one costing an exponential only inside its own window.  No atomics, fixed summation
 * order (j rows ascending, columns ascending): two calls agree bit for bit.  Colour differences and squared distances are exact
 * integers; the weight is one v_exp_f32.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, c outside 2..4, non-positive b / h / w, b > 65535, a side
 * above 2048, stds that are not in (0, 1e18], iter_max < 0, truncate < 0 or NaN, non-finite weights, q_in == q_out.
 * ---------------------------------------------------------------------------------- */
int vqseg_crf_prepare_f(const float* image, int64_t image_stride_b, int64_t image_stride_c, int64_t image_stride_px, const float* prob,
                        int64_t prob_stride_b, int64_t prob_stride_c, int64_t prob_stride_px, int b, int c, int h, int w, int iter_max,
                        double bi_xy_std, double bi_rgb_std, double pos_xy_std, double truncate, uint32_t* rgb, float* unary, float* q0,
                        float* norm_pos, float* norm_bi, float* table, void* stream);
int vqseg_crf_step_f(const uint32_t* rgb, const float* unary, const float* norm_pos, const float* norm_bi, const float* q_in, float* q_out,
                     int b, int c, int h, int w, double bi_w, double bi_xy_std, double bi_rgb_std, double pos_w, double pos_xy_std,
                     double truncate, int energies, void* stream);

/* ---------------------------------------------------------------------------------- *
 * SLIC superpixels and the mean over the segments of a label map (deprecated/train_slic.py:44-69,152-160; vq_seg_amd.nnf.slic,
 * vq_seg_amd.nnf.segment_mean, vq_seg_amd.utils.superpixel, CPSConfig.superpixel_mean, predict.Predictor(superpixels=...)).  The
 * algorithm is this project's own statement of SLIC in its gSLIC (gather) form; no parity with fast_slic or skimage is claimed.
 * fp32 throughout, labels int32, one launch for the whole batch.
 *
 * Colour: image f32 logical (b, 3, h, w) in [0, 1] (not quantised), sRGB -> CIELAB per pixel:
 *     lin(v) = ((v + 0.055) / 1.055)^2.4 above 0.04045, else v / 12.92
 *     X = (0.412453 r + 0.357580 g + 0.180423 b) / 0.95047;  Y = 0.212671 r + 0.715160 g + 0.072169 b;
 *     Z = (0.019334 r + 0.119193 g + 0.950227 b) / 1.08883;   f(t) = cbrt(t) above 0.008856, else 7.787 t + 16 / 116
 *     L = 116 f(Y) - 16;  a = 500 (f(X) - f(Y));  b = 200 (f(Y) - f(Z))                          lab: planar f32 [b][3][h * w]
 * Grid: gy x gx cells (1 <= gy <= h, 1 <= gx <= w; the caller derives them from the component count), cluster (i, j) has index
 * i * gx + j; centers f32 [b][gy * gx][5] = (L, a, b, y, x).  A pixel's home cell is (y * gy / h, x * gx / w) in integers.
 *
 * vqseg_slic_lab_f: lab of every pixel, and the initial centre of every cluster: the Lab value and the coordinates of pixel
 * (floor((i + 1/2) h / gy), floor((j + 1/2) w / gx)).  The image through batch / channel / pixel strides in ELEMENTS (planar or
 * interleaved, rows dense).
 * vqseg_slic_assign_f: labels[p] = the cluster of smallest D = |Lab_p - c_Lab|^2 + spatial_weight ((y - c_y)^2 + (x - c_x)^2) among the
 * clusters of the 3 x 3 cells around p's home cell that exist; ties go to the lowest cluster index; a pixel whose distances are
 * all NaN gets its home cell.  spatial_weight = (compactness / S)^2, S = sqrt(h w / num_components).  A gather, no atomics.
 * vqseg_slic_update_f: centers[k] = the mean of (L, a, b, y, x) over the pixels labelled k among those of the 3 x 3 cells around
 * cell k (where an assignment of this grid can put them); a cluster without pixels keeps its centre, bit for bit.  Summed in a fixed
 * order, no atomics: two calls agree bit for bit.
 *
 * vqseg_segment_sums_f: sums f32 [b][k][c] and counts i32 [b][k] of x f32 logical (b, c, hw) over the pixels of each label, per image,
 * for ANY label map; both tables are zeroed first.  A label outside [0, k) is not counted and never addressed.
 * vqseg_segment_broadcast_f: y[b, :, p] = sums[b, l, :] / counts[b, l] with l = labels[b, p]; y = x where l lies outside [0, k).  x and
 * y each through their own strides.  Applied to sums of x this is the segment mean, a symmetric projection: its adjoint is itself
 * (the backward pass is the same two launches on the incoming gradient).  The sums use one float atomic per run of equal labels
 * inside a wave, so their last bits can differ between calls; the output is exactly constant within a segment in every call.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, non-positive sizes, b > 65535 or a side above 4096 (slic),
 * a grid outside 1..h x 1..w, a spatial_weight that is negative or not finite, c > 1024, a layout that is neither planar nor
 * interleaved.
 * ---------------------------------------------------------------------------------- */
int vqseg_slic_lab_f(const float* image, int64_t image_stride_b, int64_t image_stride_c, int64_t image_stride_px, int b, int h, int w, int gy,
                     int gx, float* lab, float* centers, void* stream);
int vqseg_slic_assign_f(const float* lab, const float* centers, int b, int h, int w, int gy, int gx, float spatial_weight, int32_t* labels,
                        void* stream);
int vqseg_slic_update_f(const float* lab, const int32_t* labels, int b, int h, int w, int gy, int gx, float* centers, void* stream);
int vqseg_segment_sums_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const int32_t* labels, int b, int c,
                         int64_t hw, int k, float* sums, int32_t* counts, void* stream);
int vqseg_segment_broadcast_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const int32_t* labels,
                              const float* sums, const int32_t* counts, int b, int c, int64_t hw, int k, float* y, int64_t y_stride_b,
                              int64_t y_stride_c, int64_t y_stride_px, void* stream);

/* ---------------------------------------------------------------------------------- *
 * RBD saliency over SLIC superpixels ("Saliency Optimization from Robust Background Detection", Zhu et al., CVPR 2014, as
 * saliency_map/saliency.py:74-231 restates it; vq_seg_amd.nnf.saliency_rbd, vq_seg_amd.utils.saliency, CPSConfig.salient_mask).
 * fp32 throughout, one launch per phase for the whole batch, no atomics, fixed summation orders: every output is bit-identical
 * between calls, and an image's outputs do not depend on the batch it travels in.
 *
 * Inputs: lab f32 planar [b][3][h * w] as vqseg_slic_lab_f writes it; labels i32 [b][h * w] of the gy x gx grid above, k = gy * gx <=
 * RBD_MAX_SEGMENTS = 1024; sigma_clr (10), sigma_bndcon (1), sigma_spa (0.25), mu (0.1).  Only label maps as slic makes them are
 * supported: a pixel's label names a cluster of the 3 x 3 cells around the pixel's home cell.  A label that does not is IGNORED --
 * the pixel belongs to no cluster, is nobody's neighbour and is painted 0 -- and is never used as an index.
 *
 * Region statistics, per cluster k: n_k pixels; the mean Lab and the mean (y, x) over them; bnd_k = 1 if one of them lies in the
 * first or last row or column.  n_k = 0: the cluster is INACTIVE, takes part in nothing, and all its outputs are 0.
 *     stats f32 [b][k][8] = (L, a, b, y, x, n, bnd, 0)
 * Adjacency: adj[k][l] = 1 if a pixel of k has a 4-neighbour labelled l != k; symmetric by construction.   adj u8 [b][k][k]
 * Edge weights: W[k][l] = |Lab_k - Lab_l|_2 where (adj[k][l] or both are boundary clusters) and both are active; W[k][k] = 0;
 *     +inf otherwise.
 * Geodesic: G = all-pairs shortest path lengths over W (finite between active clusters of a map that covers the image; +inf is
 *     carried without a NaN).
 * Row passes, sums over the active clusters l, d_spa[k][l] = |centre_k - centre_l| / sqrt(h^2 + w^2):
 *     area_k = sum exp(-G[k][l]^2 / (2 sigma_clr^2));   len_k = the same sum over boundary clusters l only
 *     w_bg_k = 1 - exp(-(len_k / sqrt(area_k))^2 / (2 sigma_bndcon^2))
 *     wCtr_k = sum G[k][l] exp(-d_spa[k][l]^2 / (2 sigma_spa^2)) w_bg_l
 *     wCtr is then normalised to [0, 1] by its min and max over the active clusters; all 0 if they are equal.
 * Solve: s[k][l] = adj[k][l] (exp(-G[k][l]^2 / (2 sigma_clr^2)) + mu);  A = diag(2 w_bg + 2 wCtr + 2 sum_l s[.][l]) - 2 s;  b = 2 wCtr;
 *     A x = b over the active clusters.  A is a graph Laplacian plus a non-negative diagonal that is positive at every boundary
 *     cluster: symmetric positive definite, eliminated without pivoting.
 * Map: sal[p] = (x[label_p] - min x) / (max x - min x) over the active clusters, all 0 if max = min; f32 in [0, 1].
 *
 * vqseg_region_graph_f: stats and adj (zeroed here first).  A workgroup owns one cluster, scans the 3 x 3 cells around its cell and
 *     writes only its own rows.
 * vqseg_rbd_weights_f: W f32 [b][k][k].
 * vqseg_rbd_geodesic_f: G in place of W: blocked Floyd-Warshall on 64 x 64 tiles in LDS, three launches per pivot block, from
 *     the host; no cooperative launch, no waiting between workgroups.  Keeps a symmetric W symmetric bit for bit.
 * vqseg_rbd_background_f: w_bg f32 [b][k].      vqseg_rbd_contrast_f: wCtr f32 [b][k], not yet normalised.
 * vqseg_rbd_solve_f: one workgroup per image: wctr_norm, x and xnorm (the normalised x), each f32 [b][k]; work f32 [b][k][k] holds A.
 * vqseg_rbd_paint_f: sal f32 [b][h * w], exactly constant within a superpixel.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, non-positive sizes, b > 65535, a side above 4096, a grid
 * outside 1..h x 1..w, k above 1024, a sigma outside (0, 1e18], mu outside [0, 1e18].
 * ---------------------------------------------------------------------------------- */
int vqseg_region_graph_f(const float* lab, const int32_t* labels, int b, int h, int w, int gy, int gx, float* stats, uint8_t* adj,
                         void* stream);
int vqseg_rbd_weights_f(const float* stats, const uint8_t* adj, int b, int k, float* weights, void* stream);
int vqseg_rbd_geodesic_f(float* g, int b, int k, void* stream);
int vqseg_rbd_background_f(const float* g, const float* stats, int b, int k, float sigma_clr, float sigma_bndcon, float* w_bg, void* stream);
int vqseg_rbd_contrast_f(const float* g, const float* stats, const float* w_bg, int b, int k, int h, int w, float sigma_spa, float* wctr,
                         void* stream);
int vqseg_rbd_solve_f(const float* g, const float* stats, const uint8_t* adj, const float* w_bg, const float* wctr, int b, int k,
                      float sigma_clr, float mu, float* work, float* wctr_norm, float* x, float* xnorm, void* stream);
int vqseg_rbd_paint_f(const float* xnorm, const int32_t* labels, int b, int h, int w, int gy, int gx, float* sal, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Photometric strong augmentation: colour jitter, grayscale and Gaussian blur of an RGB batch, one parameter row per sample
 * (vq_seg_amd.data.augmentations.photometric / StrongPhotometric; CPSConfig.hard_aug = "photometric").  No reference counterpart (its
 * hard augmentation stops at CutMix) and no parity with torchvision or PIL is claimed: THIS is the definition, restated in float64 by
 * tests/photometric_cases.py.
 *
 * x: (n, 3, h, w) f32, RGB planes, values meant to lie in [0, 1]; NaN is unspecified.  Sample s has the row (b, c, sat, hue, gray,
 * sigma).  The ops run in this order, all arithmetic in f32.  An op whose parameter has its identity value is SKIPPED, not evaluated,
 * and a sample whose six parameters are all identity is copied bit for bit (no clamp).  g(p) = 0.299 r + 0.587 g + 0.114 b.
 *   1 brightness (identity b = 1)     p = clamp(b p, 0, 1)
 *   2 contrast   (identity c = 1)     p = clamp(c p + (1 - c) m, 0, 1),  m = the mean of g over all h w pixels of the sample after step 1
 *   3 saturation (identity sat = 1)   p = clamp(sat p + (1 - sat) g(p), 0, 1)
 *   4 hue        (identity hue = 0; |hue| <= 0.5)   RGB -> HSV, h = (h + hue) mod 1, HSV -> RGB by the hexcone formulas:
 *         v = max, cr = max - min, s = cr / max (0 when cr == 0); rc = (max - r) / cr, gc, bc likewise (divisor 1 when cr == 0);
 *         h6 = bc - gc if max == r, else 2 + rc - bc if max == g, else 4 + gc - rc;  h = (h6 / 6 + 1) mod 1
 *         back: i = floor(6 h), f = 6 h - i, i mod 6;  p_ = clamp(v (1 - s)), q = clamp(v (1 - f s)), t = clamp(v (1 - (1 - f) s));
 *         (r, g, b) = (v, t, p_), (q, v, p_), (p_, v, t), (p_, q, v), (t, p_, v), (v, p_, q) for i = 0..5
 *   5 grayscale  (identity gray = 0)  r = g = b = g(p)
 *   6 blur       (identity sigma = 0) R = ceil(3 sigma), 1 <= R <= 8; taps w_i = exp(-i^2 / 2 sigma^2) / sum_j exp(-j^2 / 2 sigma^2), i in
 *         [-R, R], computed on the HOST in float64 and rounded to f32; rows first, then columns, each plane on its own; reflect-101
 *         borders (index -i -> i, n - 1 + i -> n - 1 - i), which needs R <= min(h, w) - 1
 *
 *   src, out              out of place, the same layout and sample stride; src is never written
 *   stride_s/_p/_px       sample, plane and pixel strides in ELEMENTS, rows dense: planar (pixel stride 1, plane stride h * w) or interleaved
 *                         (plane stride 1, pixel stride 3: channels_last); anything else is VQSEG_EINVAL
 *   params_host [n][6]    HOST rows (b, c, sat, hue, gray, sigma): finite; b, c, sat, sigma >= 0; gray 0 or 1
 *   radii_host  [n]       HOST R per sample: 0 exactly where sigma is 0
 *   taps_host   [n][9]    HOST w_0 .. w_8 per sample (w_-i = w_i), 0 beyond R
 *   partials              device workspace of n * vqseg_photometric_mean_blocks(h w) floats; required when some c != 1, else may be null
 *   means                 null, or n device floats: means[s] = m of every sample with c != 1 (the others are not written)
 * Parameters and taps travel as kernel arguments, 32 samples per launch: no device allocation, no host-to-device copy, no
 * synchronisation.  Per launch: a mean pass when one of its samples has c != 1 (per-(sample, workgroup) partial sums in a fixed order,
 * folded by the main pass in a fixed order; NO atomics: two calls agree bit for bit, and a sample's result does not depend on the batch
 * it travels in, nor on the layout), then the main pass: a workgroup owns a 16 x 64 tile of output pixels, evaluates steps 1-5 for the
 * tile plus an R-wide reflected halo into LDS and runs the row and the column pass from there; sigma = 0 takes no halo and no stencil,
 * an all-identity row a copy.  The blur adds the two taps of equal weight first and accumulates from the outermost pair inwards.
 * vqseg_photometric_mean_blocks: the workgroups P (1..64) that share a sample's reduction, a function of the pixel count alone; pixel
 * q goes to thread q % (256 P), so a thread adds ceil(h w / (256 P)) values in sequence and the folds add 6 + 2 + 6 levels.
 * ---------------------------------------------------------------------------------- */
int vqseg_photometric_mean_blocks(int64_t pixels);
int vqseg_photometric_f(const float* src, float* out, int n, int h, int w, int64_t stride_s, int64_t stride_p, int64_t stride_px,
                        const float* params_host, const int32_t* radii_host, const float* taps_host, float* partials, float* means,
                        void* stream);

/* ---------------------------------------------------------------------------------- *
 * Connected regions of an integer map: roots, ids, the instance table, areas and the area filter (vq_seg_amd.nnf.region_roots /
 * region_ids / region_table / region_areas / filter_regions, vq_seg_amd.utils.regions, predict.Predictor(min_area=...) and
 * .instances, CPSConfig.pseudo_min_area).  The reference labels on the host, per file, with skimage / cv2; THIS is the definition,
 * restated by a plain union-find in tests/region_cases.py.  Integers throughout: every output is exact, bit-identical between calls,
 * and an image's outputs do not depend on the batch it travels in.
 *
 * Inputs: values u8 or i32 [b][h * w]; connectivity 4 or 8; 0 to 4 ignored values (ignore0.. are read up to n_ignore).
 * Limits: 1 <= b <= 65535, 1 <= h, w <= 4096; for the table 1 <= capacity and b * capacity <= 2^26 rows (2 GiB of table).
 *
 * Region: a maximal set of non-ignored pixels of ONE image with equal value, connected through 4- or 8-neighbours.
 *   root  i32 [b][h * w]   the smallest row-major index y * w + x among the pixels of the pixel's region; -1 for an ignored pixel
 *   id    i32 [b][h * w]   the region's 0-based rank among the image's regions by rising root; -1 where root is -1
 *   count i32 [b]          the number of regions of the image (id + 1 with ignore = {0} on a binary map is scipy.ndimage.label's
 *                          numbering, cross structure for 4, full 3 x 3 for 8)
 *   table i32 [b][capacity][8] = (value, area, ymin, xmin, ymax, xmax, root, 0), row `id`; moments i64 [b][capacity][2] = (sum y, sum x).
 *                          Rows from min(count, capacity) on are zero; a region with id >= capacity is counted, keeps its id in the id
 *                          map and writes no row
 *   area  i32 [b][h * w]   the region's area at its root index, 0 elsewhere
 *   filter                 out[p] = values[p] where p belongs to no region or its region's area >= min_area; otherwise the fill: the
 *                          constant `fill`, or with neighbour = 1 the INPUT value of the pixel before the region's root: (y, x - 1) if
 *                          the root has x > 0, else (y - 1, x) if y > 0, else the pixel keeps its value.  That pixel lies outside the
 *                          region and its value differs from the region's (equal and adjacent, it would be the root).  Single shot:
 *                          no cascade of merges.
 * Maps handed in (root, id) are never trusted as indices: a root outside [0, h * w) -- or, for the ids, one that is not its own
 * root -- is a pixel of no region; an id outside [0, capacity) writes no row.
 *
 * vqseg_region_roots_u8 / _i32: three launches.  Local: a workgroup per 16 x 64 tile, union-find in LDS (links to the left and upper
 *     neighbours, the two upper diagonals for 8; a link is an atomicMin on the larger root, so parents only fall), then a flatten in
 *     LDS and a store of the local root's global index to `parent` (a workspace of b * h * w i32, not `root`).  Merge: the tiles'
 *     border pixels join across the borders by find + atomicMin on `parent`, tile corners included; the find loads are agent-scope
 *     relaxed atomic loads.  Flatten: every pixel follows its chain in `parent` and writes `root`.  Whatever order the merges run
 *     in, the root is the region's smallest index.
 * vqseg_region_ids_i32: four launches: roots counted per 1024 pixels, a scan per image over `partial` (a workspace of
 *     b * vqseg_region_ids_partials(h, w) i32), ranks at the roots, id[p] = id[root[p]] elsewhere.
 * vqseg_region_table_i32: table and moments are zeroed; the roots write value, ymin and root, then integer atomics add area, box and
 *     moments, one set per run of equal ids among the 64 consecutive pixels of a wave.  value_bytes: 1 (values is u8) or 4 (i32).
 * vqseg_region_areas_i32: area is zeroed; the runs of equal roots of a workgroup's 256 pixels are gathered in LDS, then one atomicAdd per root.
 * vqseg_region_filter_u8 / _i32: a gather, out of place.  neighbour 0: the constant `fill` (0..255 for u8).
 * No workgroup waits for another; every find / union loop has a trip bound of at most h * w and falls through at it.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, sizes outside the limits, a connectivity other than 4 or 8,
 * n_ignore outside 0..4, parent == root, root == id, out == values, a capacity outside its limit, a fill outside the element type.
 * ---------------------------------------------------------------------------------- */
int vqseg_region_roots_u8(const uint8_t* values, int b, int h, int w, int connectivity, int n_ignore, int ignore0, int ignore1, int ignore2,
                          int ignore3, int32_t* parent, int32_t* root, void* stream);
int vqseg_region_roots_i32(const int32_t* values, int b, int h, int w, int connectivity, int n_ignore, int ignore0, int ignore1, int ignore2,
                           int ignore3, int32_t* parent, int32_t* root, void* stream);
int64_t vqseg_region_ids_partials(int h, int w);
int vqseg_region_ids_i32(const int32_t* root, int b, int h, int w, int32_t* partial, int32_t* id, int32_t* count, void* stream);
int vqseg_region_table_i32(const void* values, int value_bytes, const int32_t* root, const int32_t* id, int b, int h, int w, int capacity,
                           int32_t* table, int64_t* moments, void* stream);
int vqseg_region_areas_i32(const int32_t* root, int b, int h, int w, int32_t* area, void* stream);
int vqseg_region_filter_u8(const uint8_t* values, const int32_t* root, const int32_t* area, int b, int h, int w, int min_area, int neighbour,
                           int fill, uint8_t* out, void* stream);
int vqseg_region_filter_i32(const int32_t* values, const int32_t* root, const int32_t* area, int b, int h, int w, int min_area, int neighbour,
                            int fill, int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Boundary metrics: the class boundaries of a label map, the exact squared Euclidean distance transform (EDT) of seed planes, and
 * the count table behind boundary F1, boundary IoU and the Hausdorff distance (vq_seg_amd.nnf.class_boundaries / edt_sq /
 * boundary_counts, vq_seg_amd.utils.boundary, evaluate.test_loop(boundary=...)).  The reference scores region overlap only; THIS is
 * the definition, restated in plain numpy in tests/boundary_cases.py.  Integers throughout: every output is exact, bit-identical
 * between calls, and an image's outputs do not depend on the batch it travels in.
 *
 * Inputs: labels u8 or i32 [b][h * w]; C = num_classes in 1..32; 0 to 4 ignored values (ignore0.. are read up to n_ignore).
 * Limits: 1 <= h, w <= 2048 (the distance along a row is kept in 16 bits; the region kernels' limit of 4096 does not apply here),
 *         1 <= planes = b * C <= 2^19 per launch.  The largest real squared distance, 2 * 2047^2, fits an int32.
 *
 * Boundary  seeds u8 [b][C][h * w] of 0 / 1: pixel p is a boundary pixel of class c when labels[p] == c and at least one of its
 *           4-neighbours q INSIDE the image has a value that is neither c nor one of the ignored values.  The image border makes no
 *           boundary, an ignored neighbour makes none, a neighbour with any other value (>= C included) does.  A label is compared
 *           with the class, never used as an index.
 * Distance  d2 i32 [planes][h * w]: d2[p] = min over q with seeds[q] != 0 of (py - qy)^2 + (px - qx)^2; VQSEG_EDT_NONE = 2^31 - 1
 *           everywhere on a plane without a seed.  Planes are independent.  Where the plane has a seed, d2 is
 *           rint(scipy.ndimage.distance_transform_edt(seeds == 0)^2) (scipy measures to the nearest ZERO).
 * Counts    table i32 [b][C][8] from pred and target (class maps of one size), bp / bg = the boundaries of pred / target and
 *           dp / dg = their squared distances, tol_sq = floor(tolerance^2) and width_sq = floor(width^2).  A pixel is VALID when
 *           target[p] is not ignored; only valid pixels are counted:
 *             0 n_pred      valid pixels with bp                  1 hit_pred    of those, dg <= tol_sq
 *             2 n_gt        valid pixels with bg                  3 hit_gt      of those, dp <= tol_sq
 *             4 band_inter  valid pixels in both Pd and Gd        5 band_union  valid pixels in Pd or Gd
 *             6 hd_pred_sq  max of dg over the pixels of column 0; -1 if column 0 is 0 or the target has no boundary of c
 *             7 hd_gt_sq    max of dp over the pixels of column 2; -1 likewise
 *           with the inner bands Pd = (pred == c) & (dp <= width_sq), Gd = (target == c) & (dg <= width_sq): the mask pixels within
 *           `width` of the mask's own contour (Cheng et al.'s boundary IoU, except that the image border is no contour).
 * Scores (host, float64): P = hit_pred / n_pred, R = hit_gt / n_gt, F = 2 P R / (P + R); F is NaN (undefined) when n_pred == n_gt
 *           == 0, and 0 when exactly one of them is 0 or P + R == 0.  BIoU = band_inter / band_union, NaN when band_union == 0.
 *           HD = sqrt(max(column 6, column 7)), NaN when either is -1.  Means skip NaN; a class that is NaN for every image is left
 *           out of the class mean; the mean of nothing is NaN.
 *
 * vqseg_boundary_seeds_u8 / _i32: one launch, a thread per pixel, every plane of the pixel written.
 * vqseg_boundary_edt_rows_u8: one launch, a workgroup per plane row: g u16 [planes][h * w] = the distance along the row to the row's
 *     nearest seed (0xffff in a row without one), from ballot words in LDS and clz / ctz; row_has u8 [planes][h] = the row has a seed.
 * vqseg_boundary_edt_cols_i32: one launch, a workgroup per 64 x 64 tile: d2[y][x] = min over j of g[j][x]^2 + (y - j)^2, searched
 *     outwards from y through the rows that have a seed only (compacted from row_has in LDS) until (y - j)^2 >= best; a plane
 *     without a seed is filled with VQSEG_EDT_NONE.  A g of 0xffff is skipped, whatever row_has says.
 * vqseg_boundary_counts_i32: the table is preset (zeros, -1 in columns 6 and 7) by a small launch, then one pass over pred, target,
 *     bp, bg, dp and dg: a wave folds its lanes by shuffles and makes one integer atomicAdd / atomicMax per class and column.
 *     pred_bytes / target_bytes: 1 (u8) or 4 (i32).
 * Integer atomics only; no workgroup waits for another; every loop is bounded by h, w, C or a constant.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, sizes outside the limits, num_classes outside 1..32,
 * n_ignore outside 0..4, element sizes other than 1 and 4, tol_sq or width_sq outside 0..2^31 - 2.
 * ---------------------------------------------------------------------------------- */
#define VQSEG_EDT_NONE 2147483647
int vqseg_boundary_seeds_u8(const uint8_t* labels, int b, int h, int w, int num_classes, int n_ignore, int ignore0, int ignore1, int ignore2,
                            int ignore3, uint8_t* seeds, void* stream);
int vqseg_boundary_seeds_i32(const int32_t* labels, int b, int h, int w, int num_classes, int n_ignore, int ignore0, int ignore1, int ignore2,
                             int ignore3, uint8_t* seeds, void* stream);
int vqseg_boundary_edt_rows_u8(const uint8_t* seeds, int planes, int h, int w, uint16_t* g, uint8_t* row_has, void* stream);
int vqseg_boundary_edt_cols_i32(const uint16_t* g, const uint8_t* row_has, int planes, int h, int w, int32_t* d2, void* stream);
int vqseg_boundary_counts_i32(const void* pred, int pred_bytes, const void* target, int target_bytes, const uint8_t* bp, const uint8_t* bg,
                              const int32_t* dp, const int32_t* dg, int b, int h, int w, int num_classes, int tol_sq, int width_sq,
                              int n_ignore, int ignore0, int ignore1, int ignore2, int ignore3, int32_t* table, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Panoptic quality: the overlap of two region labellings, the one-to-one matching at IoU > 0.5 and the per-class instance counts
 * (vq_seg_amd.nnf.instance_overlap / instance_tally, vq_seg_amd.utils.instances, evaluate.test_loop(panoptic=...)).  The reference
 * scores pixels only; THIS is the definition, restated by brute force over all pairs in tests/instance_cases.py.  Every table is
 * integer and exact; iou_sum is a float64 sum in a fixed order, bit-identical between calls; an image's outputs do not depend on the
 * batch it travels in.
 *
 * Inputs: pred and target class maps [b][h * w]; C = num_classes in 1..255; things, a subset of 0..C-1 (default 1..C-1); 0 to 4 void
 *         values, none of them a thing class (default {255}); connectivity 4 or 8; capacity in 1..65535 rows per image and side.
 * Limits: those of the region kernels (1 <= b <= 65535, 1 <= h, w <= 4096).
 *
 * Regions   prediction regions are the connected regions of pred (the region definition above) with every value that is not a thing
 *           class ignored; ground-truth regions the same on target.  pred_id / gt_id i32 [b][h * w], pred_count / gt_count i32 [b]
 *           and pred_table / gt_table i32 [b][capacity][8] are what vqseg_region_ids_i32 / vqseg_region_table_i32 make of them
 *           (column 0 the value, column 1 the area).  The host makes the "ignored" maps; these entry points start from ids and tables.
 * Void      void[b][p] = the number of pixels of prediction region p (p < capacity) that belong to no ground-truth region and whose
 *           target value is a void value (a void value is no thing class, so a void pixel never has a ground-truth id).
 * IoU       inter(g, p) = the number of pixels with gt_id == g and pred_id == p; union = area[p] - void[p] + area[g] - inter.
 * Match     p and g match when value[p] == value[g] and 2 * inter > union: integers, strict (2 * inter == union is no match), so a
 *           region has at most one partner.  match i32 [b][capacity] = the partner of ground-truth row g or -1; inter and uni i32
 *           [b][capacity] = inter and union of that match, 0 without one; matched i32 [b][capacity] = 1 for a prediction row that
 *           has a partner, else 0.
 * Overflow  overflow i32 [b] = 1 when pred_count or gt_count exceeds capacity: the image matches nothing (match -1, inter, uni and
 *           matched 0), all its counts and sums are 0, and the caller raises capacity.  void is counted all the same.
 * Counts    tally i32 [b][C][5] per class c = (tp, fp, fn, n_pred, n_gt): tp the matched ground-truth regions of value c, fn the
 *           unmatched ones, fp the unmatched prediction regions of value c with 2 * void[p] <= area[p] (one lying mostly on void is
 *           dropped, as in the panoptic reference evaluation), n_pred / n_gt the regions of value c.  iou_sum f64 [b][C] = the sum of
 *           (double)inter / (double)union over the matches of c, added one by one in rising ground-truth id, starting from 0.0.
 * Scores (host, float64, counts summed over the images of a data set first): RQ = tp / (tp + fp / 2 + fn / 2), SQ = iou_sum / tp,
 *           PQ = SQ * RQ, NaN where the denominator is 0; pq, sq, rq the means over the thing classes, NaN skipped.
 * Maps handed in are never trusted as indices: an id outside [0, capacity) is a pixel of no region, a candidate is range-checked, a
 * count is clamped to [0, capacity], a value outside [0, C) is counted nowhere.
 *
 * vqseg_instance_vote_bits: NB = the bit length of capacity (0 for a capacity outside its limits).
 * vqseg_instance_vote_i32: votes i32 [b][capacity][NB] and void_count i32 [b][capacity] are zeroed, then one pass over pred_id, gt_id and
 *     target (target_bytes 1: u8, 4: i32; read only where there is a prediction id and no ground-truth id): a pixel of g and p adds
 *     1 to votes[b][g][k] for every set bit k of p + 1.  The runs of equal (g, p) among a wave's 64 consecutive pixels are folded,
 *     gathered per workgroup in a direct-mapped LDS table over 2048 pixels, and the table's slots make the global integer atomics.
 * vqseg_instance_overlap_i32: two launches.  cand i32 [b][capacity]: bit k of cand + 1 is 2 * votes[b][g][k] > area[g] -- the id of
 *     the prediction region that holds more than half of g if there is one (a match needs that: union >= area[g]), garbage
 *     otherwise, hence range-checked: an id in [0, capacity) or -1.  inter i32 [b][capacity] is zeroed, then a pass over both id
 *     maps counts the pixels with gt_id == g and pred_id == cand[g], with the same folding.
 * vqseg_instance_match_i32: matched is zeroed; a thread per ground-truth row tests its candidate and writes match, uni, matched
 *     and inter (in-out: the overlap with the candidate comes in, the overlap of the match goes out).
 * vqseg_instance_tally_i32: one launch, a workgroup per image: tally, iou_sum (one thread per class walks the rows) and overflow.
 * Integer atomics only; no workgroup waits for another; every loop is bounded by the pixel count, capacity, NB or C.
 *
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, sizes or a capacity outside the limits, n_void outside
 * 0..4, a target_bytes other than 1 and 4, cand == inter, num_classes outside 1..255.
 * ---------------------------------------------------------------------------------- */
int vqseg_instance_vote_bits(int capacity);
int vqseg_instance_vote_i32(const int32_t* pred_id, const int32_t* gt_id, const void* target, int target_bytes, int b, int h, int w, int capacity,
                            int n_void, int void0, int void1, int void2, int void3, int32_t* votes, int32_t* void_count, void* stream);
int vqseg_instance_overlap_i32(const int32_t* pred_id, const int32_t* gt_id, const int32_t* votes, const int32_t* gt_table, int b, int h, int w,
                               int capacity, int32_t* cand, int32_t* inter, void* stream);
int vqseg_instance_match_i32(const int32_t* cand, const int32_t* void_count, const int32_t* pred_table, const int32_t* gt_table,
                             const int32_t* pred_count, const int32_t* gt_count, int b, int capacity, int32_t* inter, int32_t* match,
                             int32_t* uni, int32_t* matched, void* stream);
int vqseg_instance_tally_i32(const int32_t* match, const int32_t* matched, const int32_t* inter, const int32_t* uni, const int32_t* void_count,
                             const int32_t* pred_table, const int32_t* gt_table, const int32_t* pred_count, const int32_t* gt_count, int b,
                             int capacity, int num_classes, int32_t* tally, double* iou_sum, int32_t* overflow, void* stream);

/* ---------------------------------------------------------------------------------- *
 * Feature perturbation: channel dropout of the decoder's inputs, fused with the concatenation that doubles the batch
 * (vq_seg_amd.nnf.channel_keep / channel_dropout_cat; the model's decode with a perturbation spec; CPSConfig.feature_perturb).
 * The reference's UniMatch stream is decoder(torch.cat((f, nn.Dropout2d(0.5)(f)))) (deprecated/train_UNIMatch.py:172,183-185;
 * models/networks/deeplabv3/net.py:109-116).  THIS is the definition; vq_seg_amd.nnf restates it with torch ops, bit for bit.
 *
 * vqseg_channel_keep_f: the keep / scale table of one forward, all levels in one launch.
 *     word0(e)  = word 0 of Philox4x32-10 with counter (e, stream_id, step & 0xffffffff, step >> 32) and key (seed & 0xffffffff, seed >> 32)
 *     scale[e]  = word0(e) >= threshold ? inv_keep : 0.0f                    for e in [0, total)
 *   The host supplies threshold = clamp(round(p * 2^32), 0, 2^32 - 1) and inv_keep = float32(1 / (1 - p)), 0 <= p < 1.  The caller
 *   lays the table out level-major: level l is a dense [B][C_l] block at offset B * sum_{j < l} C_j.  Philox rounds: (c0, c1, c2, c3)
 *   <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), M0 = 0xD2511F53, M1 = 0xCD9E8D57, then (k0, k1) +=
 *   (0x9E3779B9, 0xBB67AE85); ten rounds.  Integer arithmetic only: two calls agree bit for bit, on any device.
 *   total in 1 .. 2^32 - 1; stream_id and threshold in 0 .. 2^32 - 1; inv_keep finite, >= 1.
 *
 * vqseg_channel_dropout_cat_f: x [n][c][h][w] (bf16 = 0: f32, 1: bf16; channels_last = 0: NCHW-contiguous, 1: channels_last storage),
 *   scale f32 [n][c], out [2 n][c][h][w] in x's type and layout, out of place:
 *     out[i]        = x[i]                                                     by bits (NaN payloads, infinities, -0.0 unchanged)
 *     out[n + i, k] = scale[i, k] == 0 ? +0.0 : round(float(x[i, k]) * scale[i, k])
 *   a SELECTION of +0.0 where the channel is dropped (an Inf or NaN activation there does not leak); the product is the f32 product
 *   (round to nearest), for bf16 rounded once more to bf16 (nearest even; a NaN becomes 0x7fc0) -- what (x.float() * scale).to(dtype)
 *   computes.  scale = 2 (p = 0.5) is exact.
 * vqseg_channel_dropout_fold_f: its backward pass.  g [2 n][c][h][w], gx [n][c][h][w], the same type and layout:
 *     gx[i, k] = scale[i, k] == 0 ? g[i, k] (by bits) : round(float(g[i, k]) + round_f32(float(g[n + i, k]) * scale[i, k]))
 *   The product is rounded to f32 BEFORE the add (no FMA contraction), so separate multiply and add operators give the same bits;
 *   where the channel was dropped the second term is absent: an Inf or NaN in g[n + i, k] does not reach gx.
 * Both are HBM-bound (forward 1 read + 2 writes per element, backward 2 reads + 1 write): a 1 KiB tile of one sample per wave and
 * iteration, 16-byte loads / stores where the sample's position in every tensor is 16-byte aligned, element-wise and coalesced
 * elsewhere (a partial last tile; a sample or a half at an unaligned position); the scale is picked per element and re-read from
 * L2.  No alignment is required of any pointer beyond the element's own.  Grid capped by option "nn_grid_cap".
 * Errors (VQSEG_EINVAL before anything touches a device): null pointers, in-place calls, flags other than 0 / 1, sizes <= 0,
 * c h w > 2^40, n c > 2^31.
 * ---------------------------------------------------------------------------------- */
int vqseg_channel_keep_f(float* scale, int64_t total, uint64_t seed, int64_t stream_id, uint64_t step, int64_t threshold, float inv_keep,
                         void* stream);
int vqseg_channel_dropout_cat_f(int bf16, const void* x, const float* scale, void* out, int n, int c, int h, int w, int channels_last,
                                void* stream);
int vqseg_channel_dropout_fold_f(int bf16, const void* g, const float* scale, void* gx, int n, int c, int h, int w, int channels_last,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQSEG_H */
