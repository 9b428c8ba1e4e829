// What the prediction kernels do once a lane holds the mean logits of its four output pixels, in ONE copy: predict_kernels.hip
// (resize_argmax_kernel) and tile_kernels.hip (merge_argmax_kernel) differ in how they arrive at the logits and share everything after.
// The work unit both use: a workgroup of 256 threads takes RA_TILE consecutive output pixels of ONE image per iteration, a wave 256 of
// them starting at `pw`, lane l the pixels pw + l, + 64, + 128, + 192.
//   ra_argmax_top   first maximum (`z > mx` from -inf: a NaN never wins, all-NaN gives class 0) and 1 / sum_c expf(z_c - max)
//   ra_store_labels the u8 labels of a wave's run: packed across lanes (four shuffles) so that lane q stores the word of pixels
//                   4 q .. 4 q + 3 when the run is whole and 4-byte aligned, byte by byte otherwise
//   ra_count        one ballot per (target, label) bin and pixel slot, lane k keeping bin k's running count of its wave
//   ra_flush_counts on the way out of an image: waves -> LDS histogram -> one integer atomic per bin (order-independent)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vqseg {

constexpr int RA_MAXV = 4, RA_MAXC = 4;
constexpr int RA_PX = 4;                                    // output pixels per thread (64 apart)
constexpr int RA_TILE = 256 * RA_PX;                        // output pixels per workgroup and iteration

// z: the summed logits of one pixel; scaled by `scale` first when `scaled` (V > 1).  inv is 0 unless want_top.
template <int C>
__device__ __forceinline__ void ra_argmax_top(float (&z)[C], bool scaled, float scale, bool want_top, int& arg, float& inv) {
#pragma clang fp contract(off)
    float mx = -__builtin_inff();
    arg = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (scaled) z[c] = z[c] * scale;
        if (z[c] > mx) {                                    // first maximum, as torch.argmax
            mx = z[c];
            arg = c;
        }
    }
    inv = 0.0f;
    if (want_top) {                                         // uniform
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) sum += expf(z[c] - mx);
        inv = 1.0f / sum;                                   // exp(0) / sum: the probability of the arg-max class
    }
}

// label: the image's first label byte; img: its offset from the buffer's start; vec: the buffer itself is 4-byte aligned
__device__ __forceinline__ void ra_store_labels(uint8_t* label, long img, long pw, long HW, int lane, int vec, const int (&arg)[RA_PX]) {
    if (pw + 64 * RA_PX <= HW && vec && (img & 3) == 0) {   // uniform across the wave: lane q stores the labels of pixels 4 q .. 4 q + 3
        const unsigned mine4 = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
        const int shift = (lane >> 4) * 8;                  // pixel 4 q + i sits in lane (4 q + i) & 63 as its byte (4 q + i) >> 6 = q >> 4
        unsigned word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) word |= (((unsigned)__shfl((int)mine4, (4 * lane + i) & 63) >> shift) & 0xffu) << (8 * i);
        *reinterpret_cast<unsigned*>(label + pw + 4 * lane) = word;
    } else {
#pragma unroll
        for (int j = 0; j < RA_PX; ++j)
            if (pw + j * 64 + lane < HW) label[pw + j * 64 + lane] = (uint8_t)arg[j];
    }
}

// key: target * C + label of the lane's four pixels, -1 for a pixel that is not counted.  Every lane of the wave must call it.
template <int C>
__device__ __forceinline__ void ra_count(const int (&key)[RA_PX], int lane, unsigned& mine) {
#pragma unroll
    for (int j = 0; j < RA_PX; ++j)
#pragma unroll
        for (int k = 0; k < C * C; ++k) {
            const unsigned n = (unsigned)__popcll(__ballot(key[j] == k));
            mine += lane == k ? n : 0u;
        }
}

// cnt: the workgroup's LDS histogram (zero on entry and on exit); counts: the image's C * C bins.  Every thread must call it.
template <int C>
__device__ __forceinline__ void ra_flush_counts(unsigned* cnt, unsigned& mine, int lane, unsigned long long* counts) {
    if (lane < C * C && mine) atomicAdd(&cnt[lane], mine);
    mine = 0;
    __syncthreads();
    if (threadIdx.x < C * C) {
        const unsigned n = cnt[threadIdx.x];
        if (n) atomicAdd(&counts[threadIdx.x], (unsigned long long)n);
        cnt[threadIdx.x] = 0;
    }
    __syncthreads();
}

}  // namespace vqseg
