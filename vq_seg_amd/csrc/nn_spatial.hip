// nn_spatial.hip -- the spatial companions of the convolution kernel (gfx950), HBM-bound: 3x3 stride-2 max-pool, bilinear resampling
// (both corner conventions, with the exact-2x forms) and the gradient folds of reflect padding.
//
// Reference ops: nn.MaxPool2d(3,2,1) (models/encoders/resnet.py:167); F.interpolate(mode='bilinear') (models/networks/unet/decoder.py:35,
// align_corners=False); nn.UpsamplingBilinear2d (modified_vqunet/net.py:1172, align_corners=True).
// All tensors are NHWC "rows" (pixel-major, channels contiguous).  T = float (precise mode) or __bf16; the forward kernels of the
// pool and the resize also run on split-3 rows (T = S3Row, VC = 8: the row accessors of nn_device.h), so the split-3 path rounds
// exactly as the fp32 one.  No atomics: results are run-to-run deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bilinear_device.h"
#include "nn_device.h"
#include "nn_internal.h"

namespace vqseg {

// ---------------------------------------------------------------------------------------------
// max-pool 3x3 stride 2 pad 1 (NHWC).  Backward recomputes the arg-max (first maximum in window scan
// order kh, kw -- the order ATen's max_pool2d uses) and gathers: deterministic, no atomics.
// Each thread handles VC consecutive channels of one pixel (ldc / stc / ldpx / stpx: nn_device.h).
// ---------------------------------------------------------------------------------------------
template <typename T, int VC>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, int N, int H, int W, int C, int Ho, int Wo,
                                                          T* __restrict__ y, unsigned char* __restrict__ idx) {
    constexpr int V = VecN<T>::N;
    constexpr bool POS = !__is_same(T, S3Row);              // no window positions on split-3 rows: that path never runs a backward
    const int cv = C / VC;
    const long total = (long)N * Ho * Wo * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, ow, oh, n;
        split_nhwc(i, cv, Wo, Ho, c, ow, oh, n);
        c *= VC;
        float best[V];
        unsigned char bpos[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) {
            best[e] = -__builtin_inff();
            bpos[e] = 255;
        }
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = oh * 2 - 1 + kh;
            if (ih < 0 || ih >= H) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = ow * 2 - 1 + kw;
                if (iw < 0 || iw >= W) continue;
                float v[V];
                ldpx<T, VC>(x, ((long)n * H + ih) * W + iw, C, c, v);
#pragma unroll
                for (int e = 0; e < VC; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) {
                        best[e] = v[e];
                        if constexpr (POS) bpos[e] = (unsigned char)(kh * 3 + kw);
                    }
            }
        }
        if constexpr (POS) {
            const long o = (((long)n * Ho + oh) * Wo + ow) * C + c;
            stc<T, VC>(y, o, best);
            if (idx) {                                      // window position (kh * 3 + kw) of the maximum, for the backward
#pragma unroll
                for (int e = 0; e < VC; ++e) idx[o + e] = bpos[e];
            }
        } else stpx<T, VC>(y, ((long)n * Ho + oh) * Wo + ow, C, c, best);
    }
}

// backward from the saved window positions: an input pixel gathers g of the (at most four) windows whose maximum it is
template <typename T, int VC>
__global__ __launch_bounds__(256) void maxpool_bwd_idx_kernel(const unsigned char* __restrict__ idx, const T* __restrict__ g, int N,
                                                              int H, int W, int C, int Ho, int Wo, T* __restrict__ gx, const T* __restrict__ gx_add) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, iw, ih, n;
        split_nhwc(i, cv, W, H, c, iw, ih, n);
        c *= VC;
        float acc[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) acc[e] = 0.0f;
        for (int oh = ih / 2; oh <= (ih + 1) / 2 && oh < Ho; ++oh) {
            const int kh = ih - (oh * 2 - 1);
            if (kh < 0 || kh > 2) continue;
            for (int ow = iw / 2; ow <= (iw + 1) / 2 && ow < Wo; ++ow) {
                const int kw = iw - (ow * 2 - 1);
                if (kw < 0 || kw > 2) continue;
                const long o = (((long)n * Ho + oh) * Wo + ow) * C + c;
                const unsigned char me = (unsigned char)(kh * 3 + kw);
                unsigned char pos[V];
                if constexpr (VC == 8) {
                    const unsigned long long raw = *reinterpret_cast<const unsigned long long*>(idx + o);
#pragma unroll
                    for (int e = 0; e < 8; ++e) pos[e] = (unsigned char)(raw >> (8 * e));
                } else if constexpr (VC == 4) {
                    const unsigned int raw = *reinterpret_cast<const unsigned int*>(idx + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) pos[e] = (unsigned char)(raw >> (8 * e));
                } else {
                    pos[0] = idx[o];
                }
                bool any = false;
#pragma unroll
                for (int e = 0; e < VC; ++e) any = any || pos[e] == me;
                if (!any) continue;
                float gv[V];
                ldc<T, VC>(g, o, gv);
#pragma unroll
                for (int e = 0; e < VC; ++e)
                    if (pos[e] == me) acc[e] += gv[e];
            }
        }
        if (gx_add) {                                       // fan-in: the pooled tensor's other consumer (autograd's add: both rounded to T first)
            float ad[V];
            ldc<T, VC>(gx_add, (((long)n * H + ih) * W + iw) * C + c, ad);
#pragma unroll
            for (int e = 0; e < VC; ++e) acc[e] = (float)(T)acc[e] + ad[e];
        }
        stc<T, VC>(gx, (((long)n * H + ih) * W + iw) * C + c, acc);
    }
}

template <typename T, int VC>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ g, int N, int H, int W,
                                                          int C, int Ho, int Wo, T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, iw, ih, n;
        split_nhwc(i, cv, W, H, c, iw, ih, n);
        c *= VC;
        float acc[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) acc[e] = 0.0f;
        // output windows that contain (ih, iw): oh in [ih/2 .. (ih+1)/2]
        for (int oh = ih / 2; oh <= (ih + 1) / 2 && oh < Ho; ++oh) {
            if (ih < oh * 2 - 1 || ih > oh * 2 + 1) continue;
            for (int ow = iw / 2; ow <= (iw + 1) / 2 && ow < Wo; ++ow) {
                if (iw < ow * 2 - 1 || iw > ow * 2 + 1) continue;
                // arg-max of this window (first maximum in scan order), per channel
                float best[V];
                int bpos[V];
#pragma unroll
                for (int e = 0; e < VC; ++e) {
                    best[e] = -__builtin_inff();
                    bpos[e] = -1;
                }
                for (int kh = 0; kh < 3; ++kh) {
                    const int jh = oh * 2 - 1 + kh;
                    if (jh < 0 || jh >= H) continue;
                    for (int kw = 0; kw < 3; ++kw) {
                        const int jw = ow * 2 - 1 + kw;
                        if (jw < 0 || jw >= W) continue;
                        float v[V];
                        ldc<T, VC>(x, (((long)n * H + jh) * W + jw) * C + c, v);
#pragma unroll
                        for (int e = 0; e < VC; ++e)
                            if (v[e] > best[e] || v[e] != v[e]) {
                                best[e] = v[e];
                                bpos[e] = jh * W + jw;
                            }
                    }
                }
                float gv[V];
                ldc<T, VC>(g, (((long)n * Ho + oh) * Wo + ow) * C + c, gv);
#pragma unroll
                for (int e = 0; e < VC; ++e)
                    if (bpos[e] == ih * W + iw) acc[e] += gv[e];
            }
        }
        stc<T, VC>(gx, (((long)n * H + ih) * W + iw) * C + c, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// bilinear resize (NHWC), both corner conventions (ATen upsample_bilinear2d semantics)
//   align_corners: src = dst * (in-1)/(out-1);  else src = max((dst+0.5)*in/out - 0.5, 0)
// bil_src (taps and weight of one output coordinate) and bil_mix (the three multiply-adds): bilinear_device.h, shared with the fused
// resize + arg-max of predict_kernels.hip
// ---------------------------------------------------------------------------------------------
template <typename T, int VC>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const T* __restrict__ x, int N, int H, int W, int C, int Ho, int Wo,
                                                           int align, T* __restrict__ y) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const long total = (long)N * Ho * Wo * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, ow, oh, n;
        split_nhwc(i, cv, Wo, Ho, c, ow, oh, n);
        c *= VC;
        int h0, h1, w0, w1;
        float lh, lw;
        bil_src(oh, H, Ho, align, h0, h1, lh);
        bil_src(ow, W, Wo, align, w0, w1, lw);
        const long b = (long)n * H;
        float v00[V], v01[V], v10[V], v11[V], o[V];
        ldpx<T, VC>(x, (b + h0) * W + w0, C, c, v00);
        ldpx<T, VC>(x, (b + h0) * W + w1, C, c, v01);
        ldpx<T, VC>(x, (b + h1) * W + w0, C, c, v10);
        ldpx<T, VC>(x, (b + h1) * W + w1, C, c, v11);
#pragma unroll
        for (int e = 0; e < VC; ++e)
            o[e] = bil_mix(v00[e], v01[e], v10[e], v11[e], lh, lw);
        stpx<T, VC>(y, ((long)n * Ho + oh) * Wo + ow, C, c, o);
    }
}

// Output positions [lo, hi] that can have input position i among their two taps (a superset; the caller tests each through bil_src).
// Output d reads taps floor(s), floor(s) + 1 of its source coordinate s, so it touches i iff i - 1 < s < i + 1:
//   align_corners: s = d (in-1)/(out-1)          ->  (i-1) (out-1)/(in-1) < d < (i+1) (out-1)/(in-1)
//   else:          s = (d + 1/2) in/out - 1/2    ->  (i - 1/2) out/in - 1/2 < d < (i + 3/2) out/in - 1/2   (s clamps at 0: i = 0 reaches down to d = 0)
// evaluated in integers and widened by one position each way, which covers the rounding of the fp32 s in bil_src.  A fixed radius of
// out/in + 1 around i * out/in (the form this replaces) is short of the upper bound once out/in > 3 and under align_corners whenever
// (out-1)/(in-1) is much larger than out/in (in = 2, out = 17: input row 0 lost outputs 11..15).  Extents < 2^15: 32-bit products.
__device__ __forceinline__ void bil_bwd_range(int i, int in, int out, int align, int& lo, int& hi) {
    if (in == 1 || out == 1) {
        lo = 0;
        hi = out - 1;
        return;
    }
    if (align) {
        lo = i > 0 ? ((i - 1) * (out - 1)) / (in - 1) - 1 : 0;
        hi = ((i + 1) * (out - 1) + in - 2) / (in - 1) + 1;
    } else {
        lo = i > 0 ? ((2 * i - 1) * out) / (2 * in) - 1 : 0;
        hi = ((2 * i + 3) * out + 2 * in - 1) / (2 * in);
    }
    if (lo < 0) lo = 0;
    if (hi > out - 1) hi = out - 1;
}

// backward as a gather over the (few) output pixels whose footprint touches the input pixel
template <typename T, int VC>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const T* __restrict__ g, int N, int H, int W, int C, int Ho, int Wo,
                                                           int align, T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, iw, ih, n;
        split_nhwc(i, cv, W, H, c, iw, ih, n);
        c *= VC;
        int oh_lo, oh_hi, ow_lo, ow_hi;
        bil_bwd_range(ih, H, Ho, align, oh_lo, oh_hi);
        bil_bwd_range(iw, W, Wo, align, ow_lo, ow_hi);
        float acc[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) acc[e] = 0.0f;
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            int h0, h1;
            float lh;
            bil_src(oh, H, Ho, align, h0, h1, lh);
            float wh = 0.0f;
            if (h0 == ih) wh += 1.0f - lh;
            if (h1 == ih) wh += lh;
            if (wh == 0.0f) continue;
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                int w0, w1;
                float lw;
                bil_src(ow, W, Wo, align, w0, w1, lw);
                float ww = 0.0f;
                if (w0 == iw) ww += 1.0f - lw;
                if (w1 == iw) ww += lw;
                if (ww == 0.0f) continue;
                float gv[V];
                ldc<T, VC>(g, (((long)n * Ho + oh) * Wo + ow) * C + c, gv);
#pragma unroll
                for (int e = 0; e < VC; ++e) acc[e] = __builtin_fmaf(wh * ww, gv[e], acc[e]);
            }
        }
        stc<T, VC>(gx, (((long)n * H + ih) * W + iw) * C + c, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// Exact 2x up-sampling with align_corners = false (the decoder's resize to the next skip, decoder.py:35, whenever the skip is twice
// the size -- every power-of-two input) on power-of-two extents.  The generic kernels above are VALU-ISSUE bound (rocprofv3
// SQ_INSTS_VALU: issue time / kernel time 0.95 forward, 1.07 backward -- profiles/r03_step_valu_issue.txt): per vector they
// spend three run-time integer divisions on the index split, and the backward searches 7 x 7 candidate output pixels through
// bil_src() for the (at most) 4 x 4 that touch an input pixel.  At scale 2 the source coordinate of output o is o / 2 - 1/4:
//   o = 2 i (> 0): taps (i - 1, i) with weights (1/4, 3/4);   o = 2 i + 1: taps (i, min(i + 1, in - 1)) with (3/4, 1/4);   o = 0: tap 0
// -- all exactly representable, so these kernels evaluate the SAME expressions on the SAME values in the SAME order as the generic
// ones (bit-identical; tests/test_nn_gpu.py compares them), with shifts for the index split.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void up2_src(int o, int in, int& i0, int& i1, float& l1) {
    const int i = o >> 1;
    if (o & 1) {
        i0 = i;
        i1 = i + (i < in - 1 ? 1 : 0);
        l1 = 0.25f;
    } else if (o == 0) {
        i0 = 0;
        i1 = in > 1 ? 1 : 0;
        l1 = 0.0f;
    } else {
        i0 = i - 1;
        i1 = i;
        l1 = 0.75f;
    }
}

template <typename T, int VC>
__global__ __launch_bounds__(256) void bilinear_up2_fwd_kernel(const T* __restrict__ x, int N, int H, int W, int C, int lcv, int lwo, int lho,
                                                               T* __restrict__ y) {
    constexpr int V = VecN<T>::N;
    const int Ho = 2 * H, Wo = 2 * W;
    const long total = ((long)N << (lcv + lwo + lho));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = ((int)i & ((1 << lcv) - 1)) * VC;
        const int ow = (int)(i >> lcv) & (Wo - 1), oh = (int)(i >> (lcv + lwo)) & (Ho - 1), n = (int)(i >> (lcv + lwo + lho));
        int h0, h1, w0, w1;
        float lh, lw;
        up2_src(oh, H, h0, h1, lh);
        up2_src(ow, W, w0, w1, lw);
        const long b = (long)n * H;
        float v00[V], v01[V], v10[V], v11[V], o[V];
        ldpx<T, VC>(x, (b + h0) * W + w0, C, c, v00);
        ldpx<T, VC>(x, (b + h0) * W + w1, C, c, v01);
        ldpx<T, VC>(x, (b + h1) * W + w0, C, c, v10);
        ldpx<T, VC>(x, (b + h1) * W + w1, C, c, v11);
#pragma unroll
        for (int e = 0; e < VC; ++e)
            o[e] = bil_mix(v00[e], v01[e], v10[e], v11[e], lh, lw);
        // i enumerates (n, oh, ow, c / VC): the output's own order on plain rows; a split-3 row holds hi and lo C elements apart
        if constexpr (__is_same(T, S3Row)) stpx<T, VC>(y, ((long)n * Ho + oh) * Wo + ow, C, c, o);
        else stc<T, VC>(y, i * VC, o);
    }
}

template <typename T, int VC>
__global__ __launch_bounds__(256) void bilinear_up2_bwd_kernel(const T* __restrict__ g, int N, int H, int W, int C, int lcv, int lw_, int lh_,
                                                               T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int Ho = 2 * H, Wo = 2 * W;
    const long total = ((long)N << (lcv + lw_ + lh_));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = ((int)i & ((1 << lcv) - 1)) * VC;
        const int iw = (int)(i >> lcv) & (W - 1), ih = (int)(i >> (lcv + lw_)) & (H - 1), n = (int)(i >> (lcv + lw_ + lh_));
        float acc[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) acc[e] = 0.0f;
        // output rows 2 ih - 1 .. 2 ih + 2 touch input row ih with weights 1/4, 3/4, 3/4, 1/4; at the borders the clamped neighbour folds
        // onto the same row: output 0 gives row 0 weight 1, output 2 H - 1 gives row H - 1 weight 3/4 + 1/4 (the generic kernel's sums)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int oh = 2 * ih - 1 + a;
            if (oh < 0 || oh >= Ho) continue;
            float wh = (a == 0 || a == 3) ? 0.25f : 0.75f;
            if (a == 1 && ih == 0) wh = 1.0f;
            if (a == 2 && ih == H - 1) wh = 0.75f + 0.25f;
#pragma unroll
            for (int bq = 0; bq < 4; ++bq) {
                const int ow = 2 * iw - 1 + bq;
                if (ow < 0 || ow >= Wo) continue;
                float ww = (bq == 0 || bq == 3) ? 0.25f : 0.75f;
                if (bq == 1 && iw == 0) ww = 1.0f;
                if (bq == 2 && iw == W - 1) ww = 0.75f + 0.25f;
                float gv[V];
                ldc<T, VC>(g, (((long)n * Ho + oh) * Wo + ow) * C + c, gv);
#pragma unroll
                for (int e = 0; e < VC; ++e) acc[e] = __builtin_fmaf(wh * ww, gv[e], acc[e]);
            }
        }
        stc<T, VC>(gx, i * VC, acc);
    }
}

// r4: R input rows per thread.  The one-row form reads four gradient rows for two fresh ones and leaves the re-use of the shared pair to
// the L2 (measured: 1.7x the tensor fetched past the L2s); here a thread walks 2R + 2 rows for 2R fresh ones (R = 4: 1.25x at worst).
// Every output's own fmaf chain runs in the same order (row, then column, ascending) as above: bit-identical.
template <typename T, int VC, int R>
__global__ __launch_bounds__(256) void bilinear_up2_bwd_rows_kernel(const T* __restrict__ g, int N, int H, int W, int C, int lcv, int lw_, int lhr,
                                                                    T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int Ho = 2 * H, Wo = 2 * W;
    const long total = ((long)N << (lcv + lw_ + lhr));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = ((int)i & ((1 << lcv) - 1)) * VC;
        const int iw = (int)(i >> lcv) & (W - 1), pr = (int)(i >> (lcv + lw_)) & ((H / R) - 1), n = (int)(i >> (lcv + lw_ + lhr));
        float acc[R][V];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < VC; ++e) acc[r][e] = 0.0f;
#pragma unroll
        for (int t = 0; t < 2 * R + 2; ++t) {
            const int oh = 2 * R * pr - 1 + t;
            if (oh < 0 || oh >= Ho) continue;
#pragma unroll
            for (int bq = 0; bq < 4; ++bq) {
                const int ow = 2 * iw - 1 + bq;
                if (ow < 0 || ow >= Wo) continue;
                float ww = (bq == 0 || bq == 3) ? 0.25f : 0.75f;
                if (bq == 1 && iw == 0) ww = 1.0f;
                if (bq == 2 && iw == W - 1) ww = 0.75f + 0.25f;
                float gv[V];
                ldc<T, VC>(g, (((long)n * Ho + oh) * Wo + ow) * C + c, gv);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int a = t - 2 * r;                 // this gradient row's position in output row r's window
                    if (a < 0 || a > 3) continue;
                    const int ih = R * pr + r;
                    float wh = (a == 0 || a == 3) ? 0.25f : 0.75f;
                    if (a == 1 && ih == 0) wh = 1.0f;
                    if (a == 2 && ih == H - 1) wh = 0.75f + 0.25f;
#pragma unroll
                    for (int e = 0; e < VC; ++e) acc[r][e] = __builtin_fmaf(wh * ww, gv[e], acc[r][e]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) stc<T, VC>(gx, (((long)n * H + R * pr + r) * W + iw) * C + c, acc[r]);
    }
}

// gradient of reflect padding (pad 1): gp [N, H+2, W+2, C] -> gx [N, H, W, C]
template <typename T, int VC>
__global__ __launch_bounds__(256) void reflect_fold_kernel(const T* __restrict__ gp, int N, int H, int W, int C, T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const long total = (long)N * H * W * cv;
    const int Hp = H + 2, Wp = W + 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c, w, h, n;
        split_nhwc(i, cv, W, H, c, w, h, n);
        c *= VC;
        // padded rows mapping to h: h+1 always; 0 if h == 1; Hp-1 if h == H-2
        int hs[3], ws[3], nh = 0, nw = 0;
        hs[nh++] = h + 1;
        if (h == 1) hs[nh++] = 0;
        if (h == H - 2) hs[nh++] = Hp - 1;
        ws[nw++] = w + 1;
        if (w == 1) ws[nw++] = 0;
        if (w == W - 2) ws[nw++] = Wp - 1;
        float acc[V];
#pragma unroll
        for (int e = 0; e < VC; ++e) acc[e] = 0.0f;
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nw; ++b) {
                float v[V];
                ldc<T, VC>(gp, (((long)n * Hp + hs[a]) * Wp + ws[b]) * C + c, v);
#pragma unroll
                for (int e = 0; e < VC; ++e) acc[e] += v[e];
            }
        stc<T, VC>(gx, (((long)n * H + h) * W + w) * C + c, acc);
    }
}

// gradient of reflect padding (pad 1) when only the border RING of the padded gradient was computed (conv ring mode): gx [N, H, W, C]
// already holds the padded gradient's interior (= the zero-padded data gradient); the pixels of rows 1 / H-2 and columns 1 / W-2
// gather the ring positions that reflect onto them.  ring [N][2 (W + 2) + 2 H][C]: top row, bottom row, left column, right column.
template <typename T, int VC>
__global__ __launch_bounds__(256) void reflect_ring_fold_kernel(const T* __restrict__ ring, int N, int H, int W, int C, T* __restrict__ gx) {
    constexpr int V = VecN<T>::N;
    const int cv = C / VC;
    const int Hp = H + 2, Wp = W + 2, rl = 2 * Wp + 2 * H, nb = 2 * W + 2 * (H - 2);      // border pixels of gx that receive something
    const long total = (long)N * nb * cv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % cv) * VC;
        long t = i / cv;
        const int b = (int)(t % nb);
        const int n = (int)(t / nb);
        int h, w;
        if (b < W) h = 1, w = b;
        else if (b < 2 * W) h = H - 2, w = b - W;
        else {                                              // columns 1 and W-2 of the rows other than 1 and H-2
            const int q = b - 2 * W, half = H - 2;
            int r = q < half ? q : q - half;                // index among the rows {0, 2, 3, ..., H-3, H-1}
            h = r == 0 ? 0 : (r == half - 1 ? H - 1 : r + 1);
            w = q < half ? 1 : W - 2;
        }
        int hs[3], ws[3], nh = 0, nw = 0;
        hs[nh++] = h + 1;
        if (h == 1) hs[nh++] = 0;
        if (h == H - 2) hs[nh++] = Hp - 1;
        ws[nw++] = w + 1;
        if (w == 1) ws[nw++] = 0;
        if (w == W - 2) ws[nw++] = Wp - 1;
        float acc[V];
        const long o = (((long)n * H + h) * W + w) * C + c;
        ldc<T, VC>(gx, o, acc);
        for (int a = 0; a < nh; ++a)
            for (int bb = 0; bb < nw; ++bb) {
                if (a == 0 && bb == 0) continue;           // the interior position itself: already in gx
                const int pa = hs[a], pb = ws[bb];
                const int q = pa == 0 ? pb : (pa == Hp - 1 ? Wp + pb : (pb == 0 ? 2 * Wp + pa - 1 : 2 * Wp + (Hp - 2) + pa - 1));
                float v[V];
                ldc<T, VC>(ring, ((long)n * rl + q) * C + c, v);
#pragma unroll
                for (int e = 0; e < VC; ++e) acc[e] += v[e];
            }
        stc<T, VC>(gx, o, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// Element type and channels per thread of a launch, and the ladder that picks them: 16-byte vectors (8 bf16 / 4 floats) when C allows,
// else one channel.  Split-3 rows are always RowVec<S3Row, 8> and forward only.
template <typename T_, int VC_>
struct RowVec {};
template <typename F>
static void dispatch_rows(int bf16, int C, F&& f) {
    if (bf16) {
        if (C % 8 == 0) f(RowVec<__bf16, 8>{});
        else f(RowVec<__bf16, 1>{});
    } else {
        if (C % 4 == 0) f(RowVec<float, 4>{});
        else f(RowVec<float, 1>{});
    }
}

template <typename T, int VC>
static void maxpool_t(RowVec<T, VC>, int backward, const void* x, const void* g, int N, int H, int W, int C, int Ho, int Wo, void* out,
                      unsigned char* idx, hipStream_t st_) {
    if (!backward) {
        hipLaunchKernelGGL((maxpool_fwd_kernel<T, VC>), dim3(grid_for((long)N * Ho * Wo * (C / VC))), dim3(256), 0, st_, (const T*)x, N, H,
                           W, C, Ho, Wo, (T*)out, idx);
        return;
    }
    if constexpr (!__is_same(T, S3Row)) {
        if (idx)
            hipLaunchKernelGGL((maxpool_bwd_idx_kernel<T, VC>), dim3(grid_for((long)N * H * W * (C / VC))), dim3(256), 0, st_, idx,
                               (const T*)g, N, H, W, C, Ho, Wo, (T*)out, (const T*)(backward == 2 ? x : nullptr));
        else
            hipLaunchKernelGGL((maxpool_bwd_kernel<T, VC>), dim3(grid_for((long)N * H * W * (C / VC))), dim3(256), 0, st_, (const T*)x,
                               (const T*)g, N, H, W, C, Ho, Wo, (T*)out);
    }
}

hipError_t launch_maxpool(int bf16, int backward, const void* x, const void* g, int N, int H, int W, int C, void* out,
                          unsigned char* idx, hipStream_t st_) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    dispatch_rows(bf16, C, [&](auto rv) { maxpool_t(rv, backward, x, g, N, H, W, C, Ho, Wo, out, idx, st_); });
    return hipGetLastError();
}
hipError_t launch_s3_maxpool(const void* x, int N, int H, int W, int C, void* y, hipStream_t st_) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    maxpool_t(RowVec<S3Row, 8>{}, 0, x, nullptr, N, H, W, C, Ho, Wo, y, nullptr, st_);
    return hipGetLastError();
}

static int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

template <typename T, int VC>
static void bilinear_t(RowVec<T, VC>, int backward, const void* src, int N, int H, int W, int C, int Ho, int Wo, int align, void* dst,
                       hipStream_t st_) {
    const int cv = C / VC;
    const bool up2 = g_nn_opt.bilinear_up2 && VC > 1 && !align && Ho == 2 * H && Wo == 2 * W && is_pow2(cv) && is_pow2(H) && is_pow2(W) &&
                     (long)N * Ho * Wo * cv < (1L << 40);
    if (!backward) {
        if (up2)
            hipLaunchKernelGGL((bilinear_up2_fwd_kernel<T, VC>), dim3(grid_for((long)N * Ho * Wo * cv)), dim3(256), 0, st_, (const T*)src, N, H,
                               W, C, ilog2(cv), ilog2(Wo), ilog2(Ho), (T*)dst);
        else
            hipLaunchKernelGGL((bilinear_fwd_kernel<T, VC>), dim3(grid_for((long)N * Ho * Wo * cv)), dim3(256), 0, st_, (const T*)src, N, H, W,
                               C, Ho, Wo, align, (T*)dst);
        return;
    }
    if constexpr (!__is_same(T, S3Row)) {
        if (!up2)
            hipLaunchKernelGGL((bilinear_bwd_kernel<T, VC>), dim3(grid_for((long)N * H * W * cv)), dim3(256), 0, st_, (const T*)src, N, H, W, C,
                               Ho, Wo, align, (T*)dst);
        else if (g_nn_opt.bilinear_up2 == 1 && H >= 4)
            hipLaunchKernelGGL((bilinear_up2_bwd_rows_kernel<T, VC, 4>), dim3(grid_for((long)N * (H / 4) * W * cv)), dim3(256), 0, st_,
                               (const T*)src, N, H, W, C, ilog2(cv), ilog2(W), ilog2(H / 4), (T*)dst);
        else
            hipLaunchKernelGGL((bilinear_up2_bwd_kernel<T, VC>), dim3(grid_for((long)N * H * W * cv)), dim3(256), 0, st_, (const T*)src, N, H, W,
                               C, ilog2(cv), ilog2(W), ilog2(H), (T*)dst);
    }
}

hipError_t launch_bilinear(int bf16, int backward, const void* src, int N, int H, int W, int C, int Ho, int Wo, int align,
                           void* dst, hipStream_t st_) {
    // forward: src [N,H,W,C] -> dst [N,Ho,Wo,C];  backward: src = grad [N,Ho,Wo,C] -> dst = grad_x [N,H,W,C]
    if (!bf16 && C == 3) bilinear_t(RowVec<float, 3>{}, backward, src, N, H, W, C, Ho, Wo, align, dst, st_);   // the 3-class logits
    else dispatch_rows(bf16, C, [&](auto rv) { bilinear_t(rv, backward, src, N, H, W, C, Ho, Wo, align, dst, st_); });
    return hipGetLastError();
}
hipError_t launch_s3_bilinear(const void* x, int N, int H, int W, int C, int Ho, int Wo, int align, void* y, hipStream_t st_) {
    bilinear_t(RowVec<S3Row, 8>{}, 0, x, N, H, W, C, Ho, Wo, align, y, st_);
    return hipGetLastError();
}

template <typename T, int VC>
static void reflect_fold_t(RowVec<T, VC>, const void* gp, int N, int H, int W, int C, void* gx, hipStream_t st_) {
    hipLaunchKernelGGL((reflect_fold_kernel<T, VC>), dim3(grid_for((long)N * H * W * (C / VC))), dim3(256), 0, st_, (const T*)gp, N, H,
                       W, C, (T*)gx);
}
template <typename T, int VC>
static void reflect_ring_fold_t(RowVec<T, VC>, const void* ring, int N, int H, int W, int C, void* gx, hipStream_t st_) {
    const long work = (long)N * (2 * W + 2 * (H - 2));
    hipLaunchKernelGGL((reflect_ring_fold_kernel<T, VC>), dim3(grid_for(work * (C / VC))), dim3(256), 0, st_, (const T*)ring, N, H, W, C,
                       (T*)gx);
}

hipError_t launch_reflect_fold(int bf16, const void* gp, int N, int H, int W, int C, void* gx, hipStream_t st_) {
    dispatch_rows(bf16, C, [&](auto rv) { reflect_fold_t(rv, gp, N, H, W, C, gx, st_); });
    return hipGetLastError();
}
hipError_t launch_reflect_ring_fold(int bf16, const void* ring, int N, int H, int W, int C, void* gx, hipStream_t st_) {
    dispatch_rows(bf16, C, [&](auto rv) { reflect_ring_fold_t(rv, ring, N, H, W, C, gx, st_); });
    return hipGetLastError();
}

}  // namespace vqseg
