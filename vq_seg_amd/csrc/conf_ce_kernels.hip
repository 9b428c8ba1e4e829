// conf_ce_kernels.hip -- the confidence-weighted soft cross-pseudo-supervision loss of deprecated/train_vq_pt_unet_conf_ce.py:50-113
// (vq_seg_amd/nnf.py: conf_ce, conf_ce_pair; vq_seg_amd/loss/conf_ce_loss.py) in one pass forward and one backward over the INPUT
// logits x and the TARGET logits t, both (B, C, H, W) float32 with 2..4 classes, NCHW or channels_last.
//
// Per pixel:   q = softmax(t),  w = max_c q_c,  k = first arg-max of t,   p = softmax(x),  u_c = 1 - p_c
//     pos = w * (logsumexp(x) - x_k)                       counted where w >= threshold                  (M pixels)
//     n_c = -[c != k'] * log clamp(u_c, 1e-7, 1)           counted where r_c < threshold_neg, r = softmax(t / T), k' its arg-max (Mn)
//     loss = sum pos / M  [+ sum n / Mn + 0.5 * sum_c p_c^2 / (B C HW)   when threshold_neg > 0]
// with sum / 0 := 0 (the reference: a detached 0 for M = 0, NaN for Mn = 0).  The targets are logits and are NOT detached: the
// gradient reaches t through the weight w (d pos / d t_c = pos * (1[c == k] - q_c)); masks and arg-maxes are constants.
//
// 1 - p_c is never formed by subtraction: u_c = (sum of the other classes' exponentials) / (sum of all), so the negative term and its
// gradient p_c / u_c keep their digits where p_c rounds to 1 (the reference's float32 `1 - softmax` is all cancellation there).
// k' is taken as the first maximum of t / T (T > 0), the order r has wherever its float32 values differ.
//
// The pair form evaluates loss(a <- b) and loss(b <- a) from one read of a and b: the same per-pixel function with the roles
// swapped.  Floating-point contraction is off in this file, so a direction computes the same bits in either form, and the pair's
// gradients equal the float32 sum of two single calls'.
//
// Determinism: no atomics.  A workgroup walks DICE_PX_PER_BLOCK pixels of one image and writes its sums (double) and counts
// (int64); one workgroup folds them image by image in block order, then the images in order, and writes the stats record the
// backward pass reads its 1 / M and 1 / Mn from.  Nothing returns to the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"
#include "loss_kernels.h"

#pragma clang fp contract(off)

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int CONF_STATS = 8;       // per direction: sum pos, sum n, sum p^2, M, Mn, 1/M (0: M = 0), 1/Mn (0: Mn = 0), loss
constexpr float CONF_CLAMP = 1e-7f;

struct ConfArgs {
    const float* a;                 // element (b, c, px) at b * asb + c * asc + px * asp
    const float* b;
    long asb, asc, asp, bsb, bsc, bsp;
    int B;
    long HW;
    float thr, thrn, T;
    int detach;
};

namespace {
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// one direction at one pixel: input logits x, target logits t
template <int C>
struct ConfPx {
    float p[C], u[C], q[C];         // softmax(x), 1 - softmax(x), softmax(t)
    float w, omq, nll, p2;          // q_k, 1 - q_k, logsumexp(x) - x_k, sum_c p_c^2
    int k, kn;                      // first arg-max of t, of t / T
    bool mask, neg[C];              // w >= threshold; r_c < threshold_neg
};

template <int C>
__device__ __forceinline__ void softmax_parts(const float (&z)[C], float (&e)[C], float& mx, float& sum, int& arg) {
    mx = z[0], arg = 0;
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (z[c] > mx) mx = z[c], arg = c;
    sum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        e[c] = expf(z[c] - mx);
        sum += e[c];
    }
}

// sum of the other classes' entries, in class order
template <int C>
__device__ __forceinline__ float rest_of(const float (&e)[C], int c) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < C; ++j)
        if (j != c) s += e[j];
    return s;
}

template <int C>
__device__ __forceinline__ void conf_pixel(const float (&x)[C], const float (&t)[C], float thr, float thrn, float T, ConfPx<C>& r) {
    float e[C], mx, sum;
    int kx;
    softmax_parts<C>(t, e, mx, sum, r.k);
    const float inv_t = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) r.q[c] = e[c] * inv_t;
    r.w = inv_t;                                            // exp(0) / sum: the largest entry of softmax(t)
    r.omq = rest_of<C>(e, r.k) * inv_t;
    r.mask = r.w >= thr;
    r.kn = r.k;
#pragma unroll
    for (int c = 0; c < C; ++c) r.neg[c] = false;
    if (thrn > 0.0f) {
        if (T == 1.0f) {
#pragma unroll
            for (int c = 0; c < C; ++c) r.neg[c] = r.q[c] < thrn;
        } else {
            float z[C], ez[C], mz, sz;
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = t[c] / T;
            softmax_parts<C>(z, ez, mz, sz, r.kn);
            const float inv_z = 1.0f / sz;
#pragma unroll
            for (int c = 0; c < C; ++c) r.neg[c] = ez[c] * inv_z < thrn;
        }
    }
    softmax_parts<C>(x, e, mx, sum, kx);
    const float inv_x = 1.0f / sum;
    r.p2 = 0.0f;
    float xk = x[0];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        r.p[c] = e[c] * inv_x;
        r.u[c] = rest_of<C>(e, c) * inv_x;
        r.p2 += r.p[c] * r.p[c];
        if (c == r.k) xk = x[c];
    }
    r.nll = (logf(sum) + mx) - xk;
}

template <int C>
__device__ __forceinline__ void conf_accumulate(const ConfPx<C>& r, float thrn, double (&s)[3], int (&n)[2]) {
    if (r.mask) {
        s[0] += (double)(r.w * r.nll);
        n[0] += 1;
    }
    if (thrn > 0.0f) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (r.neg[c]) {
                n[1] += 1;                                  // the arg-max class inside the mask adds 0 but counts
                if (c != r.kn) s[1] += (double)(-logf(fminf(fmaxf(r.u[c], CONF_CLAMP), 1.0f)));
            }
        s[2] += (double)r.p2;
    }
}

// gx = g * d loss / d x, gt = g * d loss / d t of one direction at one pixel; cp = g / M, cn = g / Mn, cr = g / (B C HW)
template <int C>
__device__ __forceinline__ void conf_gradient(const ConfPx<C>& r, float thrn, float cp, float cn, float cr, bool want_t, float (&gx)[C],
                                              float (&gt)[C]) {
    const float kw = r.mask ? cp * r.w : 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) gx[c] = kw * (c == r.k ? -r.u[c] : r.p[c]);
    if (thrn > 0.0f) {
        float a[C], act[C], sq[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            // torch's clamp hands the gradient on where 1e-7 <= u <= 1 (u <= 1 always holds)
            const bool on = r.neg[c] && c != r.kn && r.u[c] >= CONF_CLAMP;
            act[c] = on ? 1.0f : 0.0f;
            a[c] = on ? r.p[c] / r.u[c] : 0.0f;
            sq[c] = r.p[c] * r.p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            // d (-log u_j) / d x_c = p_j (1[c == j] - p_c) / u_j, and p_c (1 - p_c) / u_c = p_c
            gx[c] += cn * (r.p[c] * (act[c] - rest_of<C>(a, c)));
            // sum_j p_j^2 (1[c == j] - p_c) = p_c (p_c u_c - sum_{j != c} p_j^2)
            gx[c] += cr * (r.p[c] * (r.p[c] * r.u[c] - rest_of<C>(sq, c)));
        }
    }
    if (want_t) {
        const float kt = r.mask ? (cp * r.nll) * r.w : 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) gt[c] = kt * (c == r.k ? r.omq : -r.q[c]);
    }
}

template <int C>
__device__ __forceinline__ void conf_load(const ConfArgs& a, int b, long px, float (&xa)[C], float (&xb)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xa[c] = a.a[(long)b * a.asb + c * a.asc + px * a.asp];
        xb[c] = a.b[(long)b * a.bsb + c * a.bsc + px * a.bsp];
    }
}

// partial sums: psum[dir][b][block][3] (double), pcnt[dir][b][block][2] (int64)
template <int C, bool PAIR>
__global__ __launch_bounds__(256) void conf_ce_fwd_kernel(const ConfArgs a, double* __restrict__ psum, long long* __restrict__ pcnt) {
    constexpr int ND = PAIR ? 2 : 1;
    __shared__ double red_s[4][ND * 3];
    __shared__ int red_n[4][ND * 2];
    const int b = blockIdx.y;
    const long p0 = (long)blockIdx.x * DICE_PX_PER_BLOCK;
    double s[ND][3] = {};
    int n[ND][2] = {};
    for (long px = p0 + threadIdx.x; px < p0 + DICE_PX_PER_BLOCK && px < a.HW; px += 256) {
        float xa[C], xb[C];
        conf_load<C>(a, b, px, xa, xb);
        ConfPx<C> r;
        conf_pixel<C>(xa, xb, a.thr, a.thrn, a.T, r);
        conf_accumulate<C>(r, a.thrn, s[0], n[0]);
        if (PAIR) {
            conf_pixel<C>(xb, xa, a.thr, a.thrn, a.T, r);
            conf_accumulate<C>(r, a.thrn, s[ND - 1], n[ND - 1]);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double v = wave_sum(s[d][i]);
            if (lane == 0) red_s[wave][d * 3 + i] = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int v = wave_sum(n[d][i]);
            if (lane == 0) red_n[wave][d * 2 + i] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < ND * 5) {
        const int d = threadIdx.x / 5, i = threadIdx.x % 5;
        const long slot = ((long)d * a.B + b) * gridDim.x + blockIdx.x;
        if (i < 3) psum[slot * 3 + i] = ((red_s[0][d * 3 + i] + red_s[1][d * 3 + i]) + red_s[2][d * 3 + i]) + red_s[3][d * 3 + i];
        else pcnt[slot * 2 + (i - 3)] = (long long)red_n[0][d * 2 + i - 3] + red_n[1][d * 2 + i - 3] + red_n[2][d * 2 + i - 3] + red_n[3][d * 2 + i - 3];
    }
}

// one workgroup: image by image the block partials in block order (isum / icnt: [dir][b]), then the images in image order
__global__ __launch_bounds__(256) void conf_ce_final_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt, long n_blocks,
                                                            int B, int nd, float thrn, double inv_n, double* __restrict__ isum,
                                                            long long* __restrict__ icnt, double* __restrict__ stats, float* __restrict__ loss) {
    for (int i = threadIdx.x; i < nd * B; i += 256) {
        double s[3] = {0.0, 0.0, 0.0};
        long long n[2] = {0, 0};
        for (long j = 0; j < n_blocks; ++j) {
            const long slot = (long)i * n_blocks + j;
            s[0] += psum[slot * 3], s[1] += psum[slot * 3 + 1], s[2] += psum[slot * 3 + 2];
            n[0] += pcnt[slot * 2], n[1] += pcnt[slot * 2 + 1];
        }
        isum[i * 3] = s[0], isum[i * 3 + 1] = s[1], isum[i * 3 + 2] = s[2];
        icnt[i * 2] = n[0], icnt[i * 2 + 1] = n[1];
    }
    __syncthreads();
    if ((int)threadIdx.x < nd) {
        const int d = threadIdx.x;
        double s[3] = {0.0, 0.0, 0.0};
        long long n[2] = {0, 0};
        for (int b = 0; b < B; ++b) {
            const long i = (long)d * B + b;
            s[0] += isum[i * 3], s[1] += isum[i * 3 + 1], s[2] += isum[i * 3 + 2];
            n[0] += icnt[i * 2], n[1] += icnt[i * 2 + 1];
        }
        const double inv_m = n[0] > 0 ? 1.0 / (double)n[0] : 0.0, inv_mn = n[1] > 0 ? 1.0 / (double)n[1] : 0.0;
        double l = s[0] * inv_m;
        if (thrn > 0.0f) l = (l + s[1] * inv_mn) + 0.5 * s[2] * inv_n;
        double* o = stats + d * CONF_STATS;
        o[0] = s[0], o[1] = s[1], o[2] = s[2], o[3] = (double)n[0], o[4] = (double)n[1], o[5] = inv_m, o[6] = inv_mn, o[7] = l;
        loss[d] = (float)l;
    }
}

// single: g_a = g[0] d loss(a <- b) / d a, g_b = g[0] d loss(a <- b) / d b (unless detached)
// pair  : g_a = g[0] d loss(a <- b) / d a + g[1] d loss(b <- a) / d a, g_b likewise (the target-side halves unless detached)
template <int C, bool PAIR>
__global__ __launch_bounds__(256) void conf_ce_bwd_kernel(const ConfArgs a, const double* __restrict__ stats, const float* __restrict__ g,
                                                          float inv_n, float* __restrict__ g_a, float* __restrict__ g_b) {
    constexpr int ND = PAIR ? 2 : 1;
    const int b = blockIdx.y;
    const long p0 = (long)blockIdx.x * DICE_PX_PER_BLOCK;
    const bool want_t = !a.detach;
    float cp[ND], cn[ND], cr[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float gd = g[d];
        cp[d] = gd * (float)stats[d * CONF_STATS + 5];
        cn[d] = gd * (float)stats[d * CONF_STATS + 6];
        cr[d] = gd * inv_n;
    }
    for (long px = p0 + threadIdx.x; px < p0 + DICE_PX_PER_BLOCK && px < a.HW; px += 256) {
        float xa[C], xb[C], gx[C], gt[C], hx[C], ht[C];
        conf_load<C>(a, b, px, xa, xb);
        ConfPx<C> r;
        conf_pixel<C>(xa, xb, a.thr, a.thrn, a.T, r);
        conf_gradient<C>(r, a.thrn, cp[0], cn[0], cr[0], want_t, gx, gt);
        if (PAIR) {
            conf_pixel<C>(xb, xa, a.thr, a.thrn, a.T, r);
            conf_gradient<C>(r, a.thrn, cp[ND - 1], cn[ND - 1], cr[ND - 1], want_t, hx, ht);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long ia = (long)b * a.asb + c * a.asc + px * a.asp, ib = (long)b * a.bsb + c * a.bsc + px * a.bsp;
            if (PAIR) {
                g_a[ia] = want_t ? gx[c] + ht[c] : gx[c];
                g_b[ib] = want_t ? hx[c] + gt[c] : hx[c];
            } else {
                g_a[ia] = gx[c];
                if (want_t) g_b[ib] = gt[c];
            }
        }
    }
}

struct ConfPlan {
    long nb;
    size_t psum, pcnt, isum, icnt, bytes;                   // byte offsets into the workspace
};

ConfPlan conf_plan(int b, int64_t hw) {
    ConfPlan p = {};
    p.nb = dice_blocks(hw);
    const size_t slots = (size_t)2 * b * p.nb, imgs = (size_t)2 * b;
    p.psum = 0;
    p.pcnt = p.psum + slots * 3 * sizeof(double);
    p.isum = p.pcnt + slots * 2 * sizeof(long long);
    p.icnt = p.isum + imgs * 3 * sizeof(double);
    p.bytes = p.icnt + imgs * 2 * sizeof(long long);
    return p;
}

int conf_bad(const char* what) {
    char buf[200];
    snprintf(buf, sizeof(buf), "conf_ce: %s", what);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

int conf_hip_fail(hipError_t e, const char* what) {
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    return vqseg_set_error((int)e, buf);
}

int conf_args(ConfArgs& a, const float* x, int64_t xsb, int64_t xsc, int64_t xsp, const float* t, int64_t tsb, int64_t tsc, int64_t tsp, int b,
              int c, int64_t hw, float thr, float thrn, float temperature, int pair, int detach) {
    if (!x || !t) return conf_bad("null pointer argument");
    if (b <= 0 || hw <= 0 || b > 65535) return conf_bad("batch must lie in 1..65535 and the images must not be empty");
    if (c < 2 || c > 4) return conf_bad("2..4 classes");
    if (!(temperature > 0.0f) || !(temperature < 3.0e38f)) return conf_bad("temperature must be positive and finite");
    if (!(thr == thr) || !(thrn >= 0.0f)) return conf_bad("threshold must be a number, threshold_neg >= 0");
    if ((pair != 0 && pair != 1) || (detach != 0 && detach != 1)) return conf_bad("pair and detach are 0 or 1");
    a.a = x, a.asb = xsb, a.asc = xsc, a.asp = xsp, a.b = t, a.bsb = tsb, a.bsc = tsc, a.bsp = tsp;
    a.B = b, a.HW = hw, a.thr = thr, a.thrn = thrn, a.T = temperature, a.detach = detach;
    return 0;
}

template <bool PAIR>
void conf_launch_fwd(int c, dim3 grid, hipStream_t st, const ConfArgs& a, double* psum, long long* pcnt) {
    switch (c) {
        case 2: hipLaunchKernelGGL((conf_ce_fwd_kernel<2, PAIR>), grid, dim3(256), 0, st, a, psum, pcnt); break;
        case 3: hipLaunchKernelGGL((conf_ce_fwd_kernel<3, PAIR>), grid, dim3(256), 0, st, a, psum, pcnt); break;
        default: hipLaunchKernelGGL((conf_ce_fwd_kernel<4, PAIR>), grid, dim3(256), 0, st, a, psum, pcnt); break;
    }
}

template <bool PAIR>
void conf_launch_bwd(int c, dim3 grid, hipStream_t st, const ConfArgs& a, const double* stats, const float* g, float inv_n, float* g_a,
                     float* g_b) {
    switch (c) {
        case 2: hipLaunchKernelGGL((conf_ce_bwd_kernel<2, PAIR>), grid, dim3(256), 0, st, a, stats, g, inv_n, g_a, g_b); break;
        case 3: hipLaunchKernelGGL((conf_ce_bwd_kernel<3, PAIR>), grid, dim3(256), 0, st, a, stats, g, inv_n, g_a, g_b); break;
        default: hipLaunchKernelGGL((conf_ce_bwd_kernel<4, PAIR>), grid, dim3(256), 0, st, a, stats, g, inv_n, g_a, g_b); break;
    }
}
}  // namespace

}  // namespace vqseg

extern "C" {

size_t vqseg_conf_ce_workspace_bytes(int b, int64_t hw) {
    if (b <= 0 || hw <= 0) return 0;
    return vqseg::conf_plan(b, hw).bytes;
}

int vqseg_conf_ce_forward_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const float* t, int64_t t_stride_b,
                            int64_t t_stride_c, int64_t t_stride_px, int b, int c, int64_t hw, float threshold, float threshold_neg,
                            float temperature, int pair, void* workspace, size_t workspace_bytes, double* stats, float* loss, void* stream) {
    using namespace vqseg;
    ConfArgs a;
    if (int rc = conf_args(a, x, x_stride_b, x_stride_c, x_stride_px, t, t_stride_b, t_stride_c, t_stride_px, b, c, hw, threshold, threshold_neg,
                           temperature, pair, 0))
        return rc;
    if (!workspace || !stats || !loss) return conf_bad("null pointer argument");
    const ConfPlan p = conf_plan(b, hw);
    if (workspace_bytes < p.bytes) return vqseg_set_error(VQSEG_ENOSPC, "conf_ce: workspace too small");
    if ((uintptr_t)workspace & 7) return conf_bad("the workspace must be 8-byte aligned");
    char* ws = static_cast<char*>(workspace);
    double* psum = reinterpret_cast<double*>(ws + p.psum);
    long long* pcnt = reinterpret_cast<long long*>(ws + p.pcnt);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)p.nb, (unsigned)b);
    if (pair) conf_launch_fwd<true>(c, grid, st, a, psum, pcnt);
    else conf_launch_fwd<false>(c, grid, st, a, psum, pcnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return conf_hip_fail(e, "conf_ce_fwd_kernel");
    hipLaunchKernelGGL(conf_ce_final_kernel, dim3(1), dim3(256), 0, st, psum, pcnt, p.nb, b, pair ? 2 : 1, threshold_neg,
                       1.0 / ((double)b * (double)c * (double)hw), reinterpret_cast<double*>(ws + p.isum),
                       reinterpret_cast<long long*>(ws + p.icnt), stats, loss);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : conf_hip_fail(e, "conf_ce_final_kernel");
}

int vqseg_conf_ce_backward_f(const float* x, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_px, const float* t, int64_t t_stride_b,
                             int64_t t_stride_c, int64_t t_stride_px, int b, int c, int64_t hw, float threshold, float threshold_neg,
                             float temperature, int pair, int detach_targets, const double* stats, const float* g_scalar, float* g_x,
                             float* g_t, void* stream) {
    using namespace vqseg;
    ConfArgs a;
    if (int rc = conf_args(a, x, x_stride_b, x_stride_c, x_stride_px, t, t_stride_b, t_stride_c, t_stride_px, b, c, hw, threshold, threshold_neg,
                           temperature, pair, detach_targets))
        return rc;
    if (!stats || !g_scalar || !g_x) return conf_bad("null pointer argument");
    if (!g_t && (pair || !detach_targets)) return conf_bad("the target-side gradient is left out only by a single call with detached targets");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)dice_blocks(hw), (unsigned)b);
    const float inv_n = (float)(1.0 / ((double)b * (double)c * (double)hw));
    if (pair) conf_launch_bwd<true>(c, grid, st, a, stats, g_scalar, inv_n, g_x, g_t);
    else conf_launch_bwd<false>(c, grid, st, a, stats, g_scalar, inv_n, g_x, g_t);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : conf_hip_fail(e, "conf_ce_bwd_kernel");
}

}  // extern "C"
