// crf_kernels.hip -- fully connected CRF refinement of class probabilities: exact mean-field inference on a truncated support
// (vq_seg_amd/nnf.py: dense_crf; vq_seg_amd/utils/crf.py: DenseCRF; vq_seg_amd/predict.py: Predictor(crf=...)).  The contract is
// stated in include/vqseg.h; here is how the kernels meet it.
//
// One all-pairs kernel, crf_pairs_kernel, serves the bilateral norm (NORM: sum_j k_bi(i, j)) and the mean-field update (both
// messages, then the softmax).  Work unit: a workgroup of 4 waves owns a tile of 8 rows x 64 columns of i pixels of one image; a
// wave owns P = 2 consecutive rows of it and a lane ONE column of those rows, so the P pixels of a lane share dx and everything
// that depends on it.  The j pixels of the tile's window -- the tile widened by the larger support radius on every side, cut at the
// image -- stream through LDS in chunks of up to 256 pixels of one row, one j record per thread:
//     colour (r, g, b as f32 integers) | nb_j Q_j[c] | np_j Q_j[c]                    three float4, read back as broadcasts
// The next chunk's record is loaded into registers before the current chunk is consumed.  A wave skips a chunk whose row lies
// outside both windows of all of its rows (wave-uniform), and splits the chunk's columns into [before | inside | after]
// the positional window of its columns, so the positional kernel costs an exponential only where it can be non-zero: both kernels
// share one pass over j.  Inside a chunk every lane walks the same j in the same order -- rows ascending, columns ascending -- and
// adds into its own registers: no atomics, a fixed summation order, two calls agree bit for bit.
//
// Exact arithmetic of a pair: dx, dy and the colour differences are integers held in f32 (exact below 2^24: sides up to 2048), so
// d2 = dx^2 + dy^2 and c2 = |rgb_i - rgb_j|^2 carry no rounding; the weight is v_exp_f32 of a2_xy d2 + a2_rgb c2 with
// a2 = -log2(e) / (2 std^2) rounded once on the host.  A pair outside the support has d2 = +inf on that axis, so its weight is
// exp2(-inf) = 0 exactly -- the truncation is part of the definition.  Cost per pair: one exponential and about a dozen VALU
// operations; per j record and lane: three broadcast LDS reads, shared by the lane's P pixels (one pixel per lane would double
// the LDS reads per pair: by the instruction counts the LDS pipe would then bound the CU -- estimated, not measured).  Four rows
// per wave measured 5 - 25 % slower than two: half the workgroups, and a workgroup walks its whole window, tens of milliseconds
// at the default supports (profiles/crf.md).  Built with -fno-slp-vectorize (Makefile): under plain -O3 the compiler packs the
// accumulator updates into v_pk_fma_f32 plus register shuffles; the scalar v_fmac_f32 form measured 0 - 8 % faster.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/vqseg.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int CRF_TX = 64;                                  // columns of a tile: one per lane
#ifndef CRF_ROWS
#define CRF_ROWS 2                                          // (A/B builds: make ab ABSRC=crf_kernels ABFLAGS="-fno-slp-vectorize -DCRF_ROWS=4")
#endif
constexpr int CRF_P = CRF_ROWS;                             // rows per wave: the pixels of a lane
constexpr int CRF_WAVES = 4;
constexpr int CRF_TY = CRF_P * CRF_WAVES;                   // rows of a tile
constexpr int CRF_CHUNK = 256;                              // j records per LDS chunk: one per thread
constexpr int CRF_MAX_SIDE = 2048;                          // 2 * 2047^2 < 2^24: squared distances are exact f32 integers

struct CrfPairsArgs {
    const uint32_t* rgb;                                    // [B][N] r | g << 8 | b << 16
    const float* unary;                                     // [B][C][N]
    const float* norm_pos;                                  // [N]      (the positional norm does not depend on the image)
    const float* norm_bi;                                   // [B][N]   (NORM: written here)
    const float* q_in;                                      // [B][C][N]
    float* out;                                             // [B][C][N] Q or E;  NORM: norm_bi
    int H, W;
    int rb, rp;                                             // support radii, already cut to the image (<= max(H, W) - 1)
    float a_bxy, a_rgb, a_pxy;                              // -log2(e) / (2 std^2)
    float bi_w, pos_w;
    int energies;                                           // write E instead of softmax(E)
};

__device__ __forceinline__ float crf_exp2(float x) { return __builtin_amdgcn_exp2f(x); }     // v_exp_f32: 1 ulp, exp2(-inf) = 0

// NQ: accumulated channels (the classes; NORM: 1, the constant 1).  NORM: no positional kernel, the result is 1 / sqrt(sum + 1e-20).
template <int NQ, bool NORM>
__global__ __launch_bounds__(256) void crf_pairs_kernel(const CrfPairsArgs a) {
    __shared__ float4 s_col[CRF_CHUNK], s_qb[CRF_CHUNK], s_qp[CRF_CHUNK];
    const int H = a.H, W = a.W;
    const long N = (long)H * W;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * CRF_TX, y0 = blockIdx.y * CRF_TY;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int yw = y0 + wave * CRF_P;                       // the wave's first row (uniform)
    const int x = x0 + lane;
    const int xc = x < W ? x : W - 1;                       // a lane past the image computes the last column's pixel and stores nothing
    const float fx = (float)xc;
    const float fRb = (float)a.rb, fRp = (float)a.rp;
    const float INF = __builtin_inff();

    const uint32_t* rgb = a.rgb + (long)b * N;
    float ci[CRF_P][3];
#pragma unroll
    for (int p = 0; p < CRF_P; ++p) {
        const int yc = yw + p < H ? yw + p : H - 1;
        const uint32_t v = rgb[(long)yc * W + xc];
        ci[p][0] = (float)(v & 255u), ci[p][1] = (float)((v >> 8) & 255u), ci[p][2] = (float)((v >> 16) & 255u);
    }
    float accb[CRF_P][NQ], accp[CRF_P][NQ];
#pragma unroll
    for (int p = 0; p < CRF_P; ++p)
#pragma unroll
        for (int c = 0; c < NQ; ++c) accb[p][c] = 0.0f, accp[p][c] = 0.0f;

    // the window of the tile under the wider of the two supports, cut at the image (never empty: the tile's own pixels lie inside)
    const int rw = NORM || a.rb > a.rp ? a.rb : a.rp;
    const int ylo = y0 - rw > 0 ? y0 - rw : 0, yhi = y0 + CRF_TY - 1 + rw < H - 1 ? y0 + CRF_TY - 1 + rw : H - 1;
    const int xlo = x0 - rw > 0 ? x0 - rw : 0, xhi = x0 + CRF_TX - 1 + rw < W - 1 ? x0 + CRF_TX - 1 + rw : W - 1;
    const int ncc = (xhi - xlo + CRF_CHUNK) / CRF_CHUNK;    // chunks per row
    const int chunks = (yhi - ylo + 1) * ncc;
    const float* nb_img = a.norm_bi + (long)b * N;
    const float* q_img = a.q_in + (long)b * NQ * N;

    // this thread's record of chunk t (nothing for a thread past the chunk's end: its record is never read)
    auto load = [&](int t, float4& col, float4& qb, float4& qp) {
        const int jy = ylo + t / ncc, cx = xlo + (t % ncc) * CRF_CHUNK;
        const int jx = cx + tid;
        col = make_float4(0.f, 0.f, 0.f, 0.f), qb = col, qp = col;
        if (jx <= xhi) {
            const long j = (long)jy * W + jx;
            const uint32_t v = rgb[j];
            col.x = (float)(v & 255u), col.y = (float)((v >> 8) & 255u), col.z = (float)((v >> 16) & 255u);
            if (NORM) {
                qb.x = 1.0f;
            } else {
                const float nb = nb_img[j], np = a.norm_pos[j];
                float q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NQ; ++c) q[c] = q_img[(long)c * N + j];
                qb = make_float4(nb * q[0], nb * q[1], nb * q[2], nb * q[3]);
                qp = make_float4(np * q[0], np * q[1], np * q[2], np * q[3]);
            }
        }
    };

    float4 r_col, r_qb, r_qp;
    load(0, r_col, r_qb, r_qp);
    for (int t = 0; t < chunks; ++t) {
        __syncthreads();                                    // the previous chunk has been consumed
        s_col[tid] = r_col, s_qb[tid] = r_qb;
        if (!NORM) s_qp[tid] = r_qp;
        __syncthreads();
        if (t + 1 < chunks) load(t + 1, r_col, r_qb, r_qp);
        const int jy = ylo + t / ncc, cx = xlo + (t % ncc) * CRF_CHUNK;
        const int cnt = xhi - cx + 1 < CRF_CHUNK ? xhi - cx + 1 : CRF_CHUNK;
        // per row of the wave: dy^2, +inf outside the kernel's window (all wave-uniform)
        float dyb[CRF_P], dyp[CRF_P];
        bool any_b = false, any_p = false;
#pragma unroll
        for (int p = 0; p < CRF_P; ++p) {
            const int dy = jy - (yw + p), ady = dy < 0 ? -dy : dy;
            const float d2 = (float)(dy * dy);
            dyb[p] = ady <= a.rb ? d2 : INF;
            dyp[p] = ady <= a.rp ? d2 : INF;
            any_b |= ady <= a.rb, any_p |= ady <= a.rp;
        }
        if (!any_b && !any_p) continue;                               // uniform; the barriers sit at the loop's head
        const float fcx = (float)cx;

        auto pairs = [&](int lo, int hi, auto with_pos) {
            constexpr bool POS = decltype(with_pos)::value;
            for (int jj = lo; jj < hi; ++jj) {
                const float4 col = s_col[jj], qb = s_qb[jj];
                const float fdx = (fcx + (float)jj) - fx;   // integers below 2^12: exact
                const float dx2 = fdx * fdx;
                const float dxb = __builtin_fabsf(fdx) > fRb ? INF : dx2;
                const float qbv[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                for (int p = 0; p < CRF_P; ++p) {
                    const float dr = ci[p][0] - col.x, dg = ci[p][1] - col.y, db = ci[p][2] - col.z;
                    const float c2 = __builtin_fmaf(db, db, __builtin_fmaf(dg, dg, dr * dr));      // < 2^18: exact
                    const float k = crf_exp2(__builtin_fmaf(c2, a.a_rgb, (dxb + dyb[p]) * a.a_bxy));
#pragma unroll
                    for (int c = 0; c < NQ; ++c) accb[p][c] = __builtin_fmaf(k, qbv[c], accb[p][c]);
                }
                if (POS) {
                    const float4 qp = s_qp[jj];
                    const float dxp = __builtin_fabsf(fdx) > fRp ? INF : dx2;
                    const float qpv[4] = {qp.x, qp.y, qp.z, qp.w};
#pragma unroll
                    for (int p = 0; p < CRF_P; ++p) {
                        const float k = crf_exp2((dxp + dyp[p]) * a.a_pxy);
#pragma unroll
                        for (int c = 0; c < NQ; ++c) accp[p][c] = __builtin_fmaf(k, qpv[c], accp[p][c]);
                    }
                }
            }
        };
        // the chunk's columns inside the positional window of the tile's columns: local indices pl .. ph
        int pl = x0 - a.rp - cx, ph = x0 + CRF_TX - 1 + a.rp - cx;
        pl = pl > 0 ? pl : 0, ph = ph < cnt - 1 ? ph : cnt - 1;
        if (NORM || !any_p || pl > ph) {
            pairs(0, cnt, std::false_type{});
        } else {
            pairs(0, pl, std::false_type{});
            pairs(pl, ph + 1, std::true_type{});
            pairs(ph + 1, cnt, std::false_type{});
        }
    }

    if (x >= W) return;                                     // (no barrier follows)
#pragma unroll
    for (int p = 0; p < CRF_P; ++p) {
        const int y = yw + p;
        if (y >= H) break;
        const long i = (long)y * W + x;
        if (NORM) {
            a.out[(long)b * N + i] = 1.0f / sqrtf(accb[p][0] + 1e-20f);
        } else {
            const float nb = nb_img[i], np = a.norm_pos[i];
            float e[NQ];
            float mx = -INF;
#pragma unroll
            for (int c = 0; c < NQ; ++c) {
                const float mb = nb * accb[p][c], mp = np * accp[p][c];
                e[c] = (a.pos_w * mp + a.bi_w * mb) - a.unary[((long)b * NQ + c) * N + i];
                mx = e[c] > mx ? e[c] : mx;
            }
            float* o = a.out + (long)b * NQ * N + i;
            if (a.energies) {
#pragma unroll
                for (int c = 0; c < NQ; ++c) o[(long)c * N] = e[c];
            } else {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < NQ; ++c) e[c] = expf(e[c] - mx), s += e[c];
                const float inv = 1.0f / s;
#pragma unroll
                for (int c = 0; c < NQ; ++c) o[(long)c * N] = e[c] * inv;
            }
        }
    }
}

// the positional kernel is separable: sum_j k_pos(i, j) = sx[x] * sy[y] with sx[x] = sum over the columns x' of the image with
// |x' - x| <= rp of exp(-dx^2 / (2 std^2)), sy likewise.  table = [sx (W) | sy (H)], f32 values of sums taken in double.
__global__ __launch_bounds__(256) void crf_pos_table_kernel(float* table, int H, int W, int rp, double a_pxy_e) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= W + H) return;
    const int extent = t < W ? W : H, at = t < W ? t : t - W;
    const int lo = at - rp > 0 ? at - rp : 0, hi = at + rp < extent - 1 ? at + rp : extent - 1;
    double s = 0.0;
    for (int k = lo; k <= hi; ++k) {
        const double d = (double)(k - at);
        s += exp(a_pxy_e * d * d);
    }
    table[t] = (float)s;
}

struct CrfUnaryArgs {
    const float* image;
    long isb, isc, isp;                                     // batch, channel and pixel strides in elements (rows dense)
    const float* prob;
    long psb, psc, psp;
    int B, H, W;
    const float* table;                                     // [sx (W) | sy (H)], or null: no norms asked for
    uint32_t* rgb;
    float* unary;
    float* q0;
    float* norm_pos;
};

// per pixel: the colour bytes, U = -log(clip(prob, 1e-5, 1)), Q0 = softmax(-U) = clip(prob) / sum, and (image 0) the positional norm
template <int C>
__global__ __launch_bounds__(256) void crf_unary_kernel(const CrfUnaryArgs a) {
#pragma clang fp contract(off)
    const long N = (long)a.H * a.W, total = N * a.B;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / N, i = idx - b * N;
        const float* im = a.image + b * a.isb + i * a.isp;
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f = im[c * a.isc];
            f = f > 0.0f ? f : 0.0f;                        // a NaN becomes 0
            f = f < 1.0f ? f : 1.0f;
            v |= (uint32_t)(f * 255.0f) << (8 * c);         // the product in f32, then truncated
        }
        a.rgb[idx] = v;
        const float* pr = a.prob + b * a.psb + i * a.psp;
        float p[C];
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float f = pr[c * a.psc];
            f = f > 1e-5f ? f : 1e-5f;                      // a NaN becomes 1e-5
            f = f < 1.0f ? f : 1.0f;
            p[c] = f, s += f;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            a.unary[(b * C + c) * N + i] = -logf(p[c]);
            a.q0[(b * C + c) * N + i] = p[c] / s;
        }
        if (b == 0 && a.table) {
            const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
            a.norm_pos[i] = 1.0f / sqrtf(a.table[x] * a.table[a.W + y] + 1e-20f);
        }
    }
}

// what both entry points ask of the sizes and the kernel settings; nullptr when they are in order
static const char* crf_config_error(int b, int c, int h, int w, double bi_xy_std, double bi_rgb_std, double pos_xy_std, double truncate) {
    if (c < 2 || c > 4) return "2..4 classes";
    if (b <= 0 || h <= 0 || w <= 0) return "b, h and w must be positive";
    if (b > 65535) return "at most 65535 images per launch";
    if (h > CRF_MAX_SIDE || w > CRF_MAX_SIDE) return "a side above 2048 (squared pixel distances must stay exact f32 integers)";
    if (!(bi_xy_std > 0.0 && bi_xy_std <= 1e18) || !(bi_rgb_std > 0.0 && bi_rgb_std <= 1e18) || !(pos_xy_std > 0.0 && pos_xy_std <= 1e18))
        return "bi_xy_std, bi_rgb_std and pos_xy_std must be positive (and at most 1e18)";
    if (!(truncate >= 0.0)) return "truncate must be >= 0 (+inf: full support)";
    return nullptr;
}

// R = ceil(truncate * std), cut to the largest offset the image holds
static int crf_radius(double truncate, double xy_std, int h, int w) {
    const int far = (h > w ? h : w) - 1;
    const double r = ceil(truncate * xy_std);
    return r >= (double)far ? far : (int)r;
}

static const double CRF_LOG2E = 1.4426950408889634;

static hipError_t crf_launch_pairs(const CrfPairsArgs& a, int b, int c, bool norm, hipStream_t st) {
    const dim3 grid((unsigned)((a.W + CRF_TX - 1) / CRF_TX), (unsigned)((a.H + CRF_TY - 1) / CRF_TY), (unsigned)b);
    if (norm) hipLaunchKernelGGL((crf_pairs_kernel<1, true>), grid, dim3(256), 0, st, a);
    else if (c == 2) hipLaunchKernelGGL((crf_pairs_kernel<2, false>), grid, dim3(256), 0, st, a);
    else if (c == 3) hipLaunchKernelGGL((crf_pairs_kernel<3, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((crf_pairs_kernel<4, false>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace vqseg

extern "C" {

int vqseg_crf_prepare_f(const float* image, int64_t image_stride_b, int64_t image_stride_c, int64_t image_stride_px, const float* prob,
                        int64_t prob_stride_b, int64_t prob_stride_c, int64_t prob_stride_px, int b, int c, int h, int w, int iter_max,
                        double bi_xy_std, double bi_rgb_std, double pos_xy_std, double truncate, uint32_t* rgb, float* unary, float* q0,
                        float* norm_pos, float* norm_bi, float* table, void* stream) {
    using namespace vqseg;
    char buf[200];
    if (!image || !prob || !rgb || !unary || !q0) return vqseg_set_error(VQSEG_EINVAL, "crf_prepare: null image, prob, rgb, unary or q0");
    if (iter_max < 0) return vqseg_set_error(VQSEG_EINVAL, "crf_prepare: iter_max must be >= 0");
    if (iter_max > 0 && (!norm_pos || !norm_bi || !table))
        return vqseg_set_error(VQSEG_EINVAL, "crf_prepare: null norm_pos, norm_bi or table (needed when iter_max > 0)");
    if (const char* e = crf_config_error(b, c, h, w, bi_xy_std, bi_rgb_std, pos_xy_std, truncate)) {
        snprintf(buf, sizeof(buf), "crf_prepare: %s", e);
        return vqseg_set_error(VQSEG_EINVAL, buf);
    }
    const int64_t n = (int64_t)h * w;
    const bool img_ok = (image_stride_px == 1 && image_stride_c == n) || (image_stride_c == 1 && image_stride_px == 3);
    const bool prob_ok = (prob_stride_px == 1 && prob_stride_c == n) || (prob_stride_c == 1 && prob_stride_px == c);
    if (!img_ok || !prob_ok)
        return vqseg_set_error(VQSEG_EINVAL, "crf_prepare: layout must be planar (NCHW) or interleaved (channels_last) with dense rows");
    if (b > 1 && (image_stride_b < 3 * n || prob_stride_b < c * n))
        return vqseg_set_error(VQSEG_EINVAL, "crf_prepare: batch stride smaller than an image");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rb = crf_radius(truncate, bi_xy_std, h, w), rp = crf_radius(truncate, pos_xy_std, h, w);
    hipError_t e = hipSuccess;
    if (iter_max > 0) {
        hipLaunchKernelGGL(crf_pos_table_kernel, dim3((unsigned)((h + w + 255) / 256)), dim3(256), 0, st, table, h, w, rp,
                           -0.5 / (pos_xy_std * pos_xy_std));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        CrfUnaryArgs u = {};
        u.image = image, u.isb = image_stride_b, u.isc = image_stride_c, u.isp = image_stride_px;
        u.prob = prob, u.psb = prob_stride_b, u.psc = prob_stride_c, u.psp = prob_stride_px;
        u.B = b, u.H = h, u.W = w;
        u.table = iter_max > 0 ? table : nullptr;
        u.rgb = rgb, u.unary = unary, u.q0 = q0, u.norm_pos = norm_pos;
        int64_t blocks = (n * b + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        if (c == 2) hipLaunchKernelGGL((crf_unary_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, u);
        else if (c == 3) hipLaunchKernelGGL((crf_unary_kernel<3>), dim3((unsigned)blocks), dim3(256), 0, st, u);
        else hipLaunchKernelGGL((crf_unary_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, st, u);
        e = hipGetLastError();
    }
    if (e == hipSuccess && iter_max > 0) {
        CrfPairsArgs a = {};
        a.rgb = rgb, a.norm_bi = norm_bi, a.q_in = unary /* not read */, a.out = norm_bi;
        a.H = h, a.W = w, a.rb = rb, a.rp = rp;
        a.a_bxy = (float)(-0.5 * CRF_LOG2E / (bi_xy_std * bi_xy_std)), a.a_rgb = (float)(-0.5 * CRF_LOG2E / (bi_rgb_std * bi_rgb_std));
        e = crf_launch_pairs(a, b, c, true, st);
    }
    if (e != hipSuccess) {
        snprintf(buf, sizeof(buf), "crf_prepare kernels: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

int vqseg_crf_step_f(const uint32_t* rgb, const float* unary, const float* norm_pos, const float* norm_bi, const float* q_in, float* q_out,
                     int b, int c, int h, int w, double bi_w, double bi_xy_std, double bi_rgb_std, double pos_w, double pos_xy_std,
                     double truncate, int energies, void* stream) {
    using namespace vqseg;
    char buf[200];
    if (!rgb || !unary || !norm_pos || !norm_bi || !q_in || !q_out)
        return vqseg_set_error(VQSEG_EINVAL, "crf_step: null rgb, unary, norm_pos, norm_bi, q_in or q_out");
    if (q_in == q_out) return vqseg_set_error(VQSEG_EINVAL, "crf_step: q_in and q_out must be two buffers (ping-pong)");
    if (const char* e = crf_config_error(b, c, h, w, bi_xy_std, bi_rgb_std, pos_xy_std, truncate)) {
        snprintf(buf, sizeof(buf), "crf_step: %s", e);
        return vqseg_set_error(VQSEG_EINVAL, buf);
    }
    if (!(fabs(bi_w) <= 1e18) || !(fabs(pos_w) <= 1e18)) return vqseg_set_error(VQSEG_EINVAL, "crf_step: bi_w and pos_w must be finite");
    CrfPairsArgs a = {};
    a.rgb = rgb, a.unary = unary, a.norm_pos = norm_pos, a.norm_bi = norm_bi, a.q_in = q_in, a.out = q_out;
    a.H = h, a.W = w;
    a.rb = crf_radius(truncate, bi_xy_std, h, w), a.rp = crf_radius(truncate, pos_xy_std, h, w);
    a.a_bxy = (float)(-0.5 * CRF_LOG2E / (bi_xy_std * bi_xy_std)), a.a_rgb = (float)(-0.5 * CRF_LOG2E / (bi_rgb_std * bi_rgb_std));
    a.a_pxy = (float)(-0.5 * CRF_LOG2E / (pos_xy_std * pos_xy_std));
    a.bi_w = (float)bi_w, a.pos_w = (float)pos_w;
    a.energies = energies != 0;
    const hipError_t e = crf_launch_pairs(a, b, c, false, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        snprintf(buf, sizeof(buf), "crf_pairs_kernel: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    return 0;
}

}  // extern "C"
