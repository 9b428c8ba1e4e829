// Host-side declarations shared by the convolution units only (conv_igemm / conv_patch / conv_wgrad / conv_host): the dispatch
// options, the profile scope, and the patch kernels' entry point.  Everything other units may call is in conv_kernels.h.
#pragma once
#include "conv_kernels.h"

namespace vqseg {

// Dispatch tunables of the convolution path (vqseg_set_option; the key of each field: the table in conv_host.hip).  The defaults
// are the measured dispatch; the one instance lives in conv_host.hip.
struct ConvOptions {
    int glds_pair = 8;                  // layers with 2..this many Cout chunks: the chunks of an M tile share an XCD
                                        // (1-D launch, see the kernel; alone: -3..-6 % at 2-4 chunks, +5 % at 8; in the two-stream step 8 wins: r4)
    int glds_lin = 1;                   // 1x1 / stride 1 / pad 0 layers take the linear-pixel prologue (LIN)
    int patch_min_wgs = 128;            // (r4: 256 -> 128: in the two-stream step the other network's kernels fill what a 128-workgroup launch leaves idle)
    int patch_pair = 0;                 // 1: Cout chunks of a pixel tile share an XCD (1-D launch, see the kernel)
    int patch_chunk_stage = 1;          // 32-channel chunks: chunk stages instead of the per-tap weight ring
    int patch_wide_s3 = 1;              // ... also for the split-3 launches (their output tile leaves in two column halves)
    int patch_wide = 1;                 // 1 (r4): the 256-channel tile where it fills the chip -- 3-5 % slower than the unrolled 128 tile ALONE, but it reads the input rows once
                                        // per 256 instead of per 128 output channels: in the two-stream step (fabric-bound as a whole) -0.9 ms; 0: r3
    int short_k_small = 1;              // K loops of up to this many stages take the 128x128 tile at 4 waves/SIMD
    int short_k_single = 8;             // K loops of up to this many stages: single-buffered 128x128 tile, 4 workgroups/CU
    int patch_tile512 = 2;              // 512-pixel tiles for 32 / 64 output channels: 0 off, 2 on
    int patch_tile512_min_wgs = 512;
    int patch_tile512_launches = 0;     // launches that took a 512-pixel tile (tests read it to see the dispatch)
    int patch_unroll = 1;               // 128-channel tile: tap loop unrolled
    int wgrad1x1_narrow = 1;            // 64-output-channel 1x1 weight gradients (stem patch matrix, 64 -> 64) on the LDS-DMA kernel
    int wgrad_round_pct = 100;          // LDS-DMA weight gradients: workgroups aimed at, in percent of one resident round (fewer slabs = less partial traffic)
    int wgrad_xcd = 1;                  // LDS-DMA weight gradients: a slab's (ci, co) tiles on one XCD (WgradArgs::xcd_slabs); 0: 3-D grid
    int wgrad3x3_fill = 1;              // nine-tap weight gradients: slabs sized to one full round of resident workgroups (0: r3's split)
    int wgrad3x3_s2 = 1;                // stride-2 3x3 weight gradients on the nine-tap kernel (0: the per-tap kernel, r3)
    int stem_fused = 1;                 // the stem without its patch matrix (0: callers keep the patch-matrix path)
    int dgrad_s2_merge = 1;             // stride-2 3x3 data gradients: one launch, unpadded output (0: four launches + fold / crop)
    int last_variant = 0;               // id of the instantiation the last convolution / weight-gradient launch took (conv_variant_*; tests read it to see the dispatch)
};
extern ConvOptions g_conv_opt;

// Instantiation ids ("conv_last_variant"): one hexadecimal digit per template argument that selects different code, the kernel
// family in the top digit, so that two instantiations never share an id and an id reads back as its arguments:
//   0x1 T B W U M f   conv_igemm_glds_kernel<TBM, BN, NW, NBUF, MINW, S3, LIN, CLS>: T = TBM / 128, B = BN / 32, W = NW, U = NBUF, M = MINW,
//                     f = S3 * 8 + LIN * 4 + CLS * 2 + (the 1-D XCD-pair grid ? 1 : 0)
//   0x2 0 B 0 K P f   conv_igemm_kernel<BN, PRECISE, BK, S3>: B = BN / 32, K = BK / 32, P = PRECISE, f = S3 * 8
//   0x3 T B W K U f   conv3x3_patch_kernel<BN, NBW, UNROLL_TAPS, CK, S3, TBM>: T = TBM / 256, B = BN / 32, W = NBW, K = CK / 32, U = UNROLL_TAPS,
//                     f = S3 * 8 + (the 1-D XCD-pair grid ? 1 : 0)
//   0x4 0 O I S 0 f   conv_wgrad3x3_kernel<COT, CIT, S>: O = COT, I = CIT, S = stride, f = (the XCD-aware 1-D grid ? 1 : 0)
//   0x5 0 O I 0 0 f   conv_wgrad1x1_kernel<COT, CIT>: the same digits
//   0x6 0 M N 0 P 0   conv_wgrad_kernel<TM, TN, PRECISE> (per tap): M = TM, N = TN, P = PRECISE
// e.g. 0x1248314: the eight-wave 256 x 128 tile, three buffers, linear-pixel prologue, 2-D grid.
enum ConvFamily { CONV_FAM_GLDS = 1, CONV_FAM_IGEMM = 2, CONV_FAM_PATCH = 3, CONV_FAM_WGRAD3X3 = 4, CONV_FAM_WGRAD1X1 = 5, CONV_FAM_WGRAD_TAP = 6 };
constexpr int conv_variant_id(int family, int d5, int d4, int d3, int d2, int d1, int flags) {
    return family << 24 | d5 << 20 | d4 << 16 | d3 << 12 | d2 << 8 | d1 << 4 | flags;
}
constexpr int conv_variant_glds(int tbm, int bn, int nw, int nbuf, int minw, bool s3, bool lin, bool cls, bool pair) {
    return conv_variant_id(CONV_FAM_GLDS, tbm / 128, bn / 32, nw, nbuf, minw, s3 * 8 + lin * 4 + cls * 2 + pair);
}
constexpr int conv_variant_igemm(int bn, bool precise, int bk, bool s3) { return conv_variant_id(CONV_FAM_IGEMM, 0, bn / 32, 0, bk / 32, precise, s3 * 8); }
constexpr int conv_variant_patch(int bn, int nbw, bool unroll, int ck, bool s3, int tbm, bool pair) {
    return conv_variant_id(CONV_FAM_PATCH, tbm / 256, bn / 32, nbw, ck / 32, unroll, s3 * 8 + pair);
}
constexpr int conv_variant_wgrad3x3(int cot, int cit, int stride, bool xcd) { return conv_variant_id(CONV_FAM_WGRAD3X3, 0, cot, cit, stride, 0, xcd); }
constexpr int conv_variant_wgrad1x1(int cot, int cit, bool xcd) { return conv_variant_id(CONV_FAM_WGRAD1X1, 0, cot, cit, 0, 0, xcd); }
constexpr int conv_variant_wgrad_tap(int tm, int tn, bool precise) { return conv_variant_id(CONV_FAM_WGRAD_TAP, 0, tm, tn, 0, precise, 0); }

// One record of the convolution profile (bench.py's roofline_conv leg) around the launches of the enclosing block: when
// recording is on and a slot is free it files flops / kind / shape[4] and records the start event on `st`; the end event
// follows when the scope is left.
class ConvProfileScope {
public:
    ConvProfileScope(hipStream_t st, double flops, int kind, int shape0, int shape1, int shape2, int shape3);
    ~ConvProfileScope();
    ConvProfileScope(const ConvProfileScope&) = delete;
    ConvProfileScope& operator=(const ConvProfileScope&) = delete;

private:
    hipStream_t st_;
    int slot_;                          // -1: not recording
};

// the 3x3 / stride 1 / pad 1 patch kernels (bf16): false = the shape is not theirs, nothing was launched
bool launch_conv3x3_patch(const ConvArgs& a, bool k64, hipStream_t st);

}  // namespace vqseg
