// saliency_kernels.hip -- RBD saliency (Zhu et al., CVPR 2014) over SLIC superpixels, for a whole batch per launch
// (vq_seg_amd/nnf.py: saliency_rbd and the _rbd_* stages; vq_seg_amd/utils/saliency.py; CPSConfig.salient_mask).
// The definition is stated in include/vqseg.h; here is how the kernels meet it.  fp32 throughout, no atomics anywhere, every sum in a
// fixed order: all outputs are bit-identical between calls, and an image's do not depend on the batch it travels in (no kernel reads
// another image's data, and no launch shape depends on b except the grid's batch axis).
//
// rbd_region_kernel     a workgroup owns ONE cluster and scans the pixels of the 3 x 3 cells around its cell (slic_update_kernel's
//                       pattern and summation order: the means are that kernel's, bit for bit).  A pixel of the cluster also looks at
//                       its four neighbours and marks their labels in the cluster's OWN row of adj: byte stores of 1 into one row,
//                       no other workgroup writes there.  A label is used only after rbd_label has checked it against the grid.
// rbd_weights_kernel    a thread per (k, l).
// rbd_fw_pivot_kernel   blocked Floyd-Warshall on 64 x 64 tiles, three launches per pivot block p.  (1) the pivot tile in LDS, plain
// rbd_fw_panel_kernel   Floyd-Warshall with a barrier per step.  (2) the tiles of block row p and block column p: since the pivot tile P
// rbd_fw_rest_kernel    is now closed under min-plus (zero diagonal), the step-by-step update equals ONE min-plus product with the
//                       tile as it was: C = P (x) C (row) or C (x) P (column).  (3) every other tile: C = min(C, A (x) B) with A in
//                       block column p and B in block row p.  (2) and (3) are one device function: A (padded, scalar reads) and B
//                       (float4 reads) in LDS, 32.25 KiB, a 4 x 4 block of C in each thread's registers, no barrier in the loop.  A
//                       tile past the matrix edge is padded with +inf, which min and + carry without a NaN.  The three phases keep
//                       a symmetric matrix symmetric bit for bit: transposed tiles see the same sums, and min is exact.
// rbd_background_kernel a workgroup per row k: lanes stride over l, shuffle fold, waves through LDS in wave order.
// rbd_contrast_kernel   the same shape; needs every w_bg, hence a launch of its own.
// rbd_solve_kernel      ONE workgroup per image.  Normalises wCtr, builds the lower triangle of A in the [k][k] workspace (a wave per
//                       row), then eliminates column by column without pivoting (A is symmetric positive definite; the symmetric
//                       form: U[j][c] of the reduced system is the stored A[c][j]) with the right-hand side carried along, one barrier
//                       per column: the thread that updates an element of the next column also leaves it in LDS for the next step.
//                       A row whose multiplier is 0 is skipped (A starts as sparse as the adjacency).  Back substitution by rows
//                       (contiguous), one barrier per unknown.  Then the min / max normalisation of x.
// rbd_paint_kernel      a thread per pixel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int RBD_MAX_SEGMENTS = 1024;
constexpr int RBD_MAX_SIDE = 4096;                          // as slic
constexpr int RBD_T = 64;                                   // the Floyd-Warshall tile
constexpr int RBD_SOLVE_THREADS = 512;
constexpr int RBD_STAT = 8;                                 // floats per cluster: L, a, b, y, x, n, bnd, 0

struct RbdGrid {
    int B, H, W, gy, gx;
};

__device__ __forceinline__ int rbd_cell_start(int i, int n, int g) { return (int)(((long)i * n + g - 1) / g); }

// the label of pixel (y, x) if it names a cluster of the 3 x 3 cells around the pixel's home cell, else -1 (never an index then)
__device__ __forceinline__ int rbd_label(const int* lb, int y, int x, const RbdGrid& q) {
    const int l = lb[(long)y * q.W + x];
    if (l < 0 || l >= q.gy * q.gx) return -1;
    const int hi = (int)((long)y * q.gy / q.H), hj = (int)((long)x * q.gx / q.W);
    const int ci = l / q.gx, cj = l - ci * q.gx;
    return (ci - hi >= -1 && ci - hi <= 1 && cj - hj >= -1 && cj - hj <= 1) ? l : -1;
}

__global__ __launch_bounds__(256) void rbd_region_kernel(const float* lab, const int* labels, RbdGrid q, float* stats, uint8_t* adj) {
    __shared__ float s_part[4][7];
    const int H = q.H, W = q.W, gy = q.gy, gx = q.gx;
    const long N = (long)H * W;
    const int K = gy * gx;
    const int b = blockIdx.y, k = blockIdx.x;
    const int ci = k / gx, cj = k - ci * gx;
    const int ylo = rbd_cell_start(ci > 0 ? ci - 1 : 0, H, gy), yhi = ci + 2 < gy ? rbd_cell_start(ci + 2, H, gy) : H;
    const int xlo = rbd_cell_start(cj > 0 ? cj - 1 : 0, W, gx), xhi = cj + 2 < gx ? rbd_cell_start(cj + 2, W, gx) : W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* lb = labels + (long)b * N;
    const float* p = lab + (long)b * 3 * N;
    uint8_t* row = adj + ((long)b * K + k) * K;
    float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // L, a, b, y, x, count, boundary pixels
    for (int y = ylo + wave; y < yhi; y += 4) {
        for (int x = xlo + lane; x < xhi; x += 64) {
            const long i = (long)y * W + x;
            if (lb[i] != k) continue;                       // (y, x) lies in the 3 x 3 cells around cell k: the label is a valid one
            acc[0] += p[i], acc[1] += p[N + i], acc[2] += p[2 * N + i];
            acc[3] += (float)y, acc[4] += (float)x, acc[5] += 1.0f;
            if (y == 0 || y == H - 1 || x == 0 || x == W - 1) acc[6] += 1.0f;
            int l;
            if (y > 0 && (l = rbd_label(lb, y - 1, x, q)) >= 0 && l != k) row[l] = 1;
            if (y + 1 < H && (l = rbd_label(lb, y + 1, x, q)) >= 0 && l != k) row[l] = 1;
            if (x > 0 && (l = rbd_label(lb, y, x - 1, q)) >= 0 && l != k) row[l] = 1;
            if (x + 1 < W && (l = rbd_label(lb, y, x + 1, q)) >= 0 && l != k) row[l] = 1;
        }
    }
#pragma unroll
    for (int v = 0; v < 7; ++v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[v] += __shfl_down(acc[v], d, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < 7; ++v) s_part[wave][v] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x < RBD_STAT) {
        const int v = threadIdx.x;
        const float n = ((s_part[0][5] + s_part[1][5]) + s_part[2][5]) + s_part[3][5];
        float o = 0.0f;
        if (n > 0.0f && v < 7) {
            const float s = ((s_part[0][v] + s_part[1][v]) + s_part[2][v]) + s_part[3][v];
            o = v < 5 ? s / n : (v == 5 ? n : (s > 0.0f ? 1.0f : 0.0f));
        }
        stats[((long)b * K + k) * RBD_STAT + v] = o;
    }
}

__global__ __launch_bounds__(256) void rbd_weights_kernel(const float* stats, const uint8_t* adj, int B, int K, float* wgt) {
    const long KK = (long)K * K, total = KK * B;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / KK, r = idx - b * KK;
        const int k = (int)(r / K), l = (int)(r - (long)k * K);
        const float* sk = stats + (b * K + k) * RBD_STAT;
        const float* sl = stats + (b * K + l) * RBD_STAT;
        float v = __builtin_inff();
        if (k == l) {
            v = 0.0f;
        } else if (sk[5] > 0.0f && sl[5] > 0.0f && ((adj[idx] | adj[b * KK + (long)l * K + k]) || (sk[6] > 0.0f && sl[6] > 0.0f))) {
            const float dl = sk[0] - sl[0], da = sk[1] - sl[1], db = sk[2] - sl[2];
            v = sqrtf((dl * dl + da * da) + db * db);
        }
        wgt[idx] = v;
    }
}

// ---- blocked Floyd-Warshall ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rbd_fw_pivot_kernel(float* g, int K, int p) {
    __shared__ float s[RBD_T][RBD_T + 1];
    float* gb = g + (long)blockIdx.x * K * K;
    const int o = p * RBD_T, tid = threadIdx.x;
    for (int t = tid; t < RBD_T * RBD_T; t += 256) {
        const int r = t >> 6, c = t & 63;
        s[r][c] = (o + r < K && o + c < K) ? gb[(long)(o + r) * K + o + c] : __builtin_inff();
    }
    __syncthreads();
    const int c = tid & 63, r0 = tid >> 6;
    for (int k = 0; k < RBD_T; ++k) {
        // row k and column k do not change in step k (s[k][k] is 0, or +inf past the edge): updating in place is the step
        const float kc = s[k][c];
#pragma unroll
        for (int i = 0; i < RBD_T / 4; ++i) {
            const int r = r0 + 4 * i;
            s[r][c] = fminf(s[r][c], s[r][k] + kc);
        }
        __syncthreads();
    }
    for (int t = tid; t < RBD_T * RBD_T; t += 256) {
        const int r = t >> 6, cc = t & 63;
        if (o + r < K && o + cc < K) gb[(long)(o + r) * K + o + cc] = s[r][cc];
    }
}

// tile (ti, tj) = min(itself, tile (ti, tp) (x) tile (tp, tj)) in min-plus; both factors are read whole before anything is written
__device__ __forceinline__ void rbd_minplus_tile(float* gb, int K, int ti, int tj, int tp) {
    __shared__ float sa[RBD_T][RBD_T + 1];
    __shared__ __attribute__((aligned(16))) float sb[RBD_T][RBD_T];
    const int tid = threadIdx.x;
    const int ro = ti * RBD_T, co = tj * RBD_T, po = tp * RBD_T;
    for (int t = tid; t < RBD_T * RBD_T; t += 256) {
        const int r = t >> 6, c = t & 63;
        sa[r][c] = (ro + r < K && po + c < K) ? gb[(long)(ro + r) * K + po + c] : __builtin_inff();
        sb[r][c] = (po + r < K && co + c < K) ? gb[(long)(po + r) * K + co + c] : __builtin_inff();
    }
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ro + ty * 4 + i, c = co + tx * 4 + j;
            acc[i][j] = (r < K && c < K) ? gb[(long)r * K + c] : __builtin_inff();
        }
    }
    __syncthreads();
    for (int k = 0; k < RBD_T; ++k) {
        const float4 bv = *reinterpret_cast<const float4*>(&sb[k][tx * 4]);
        const float bj[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = sa[ty * 4 + i][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fminf(acc[i][j], a + bj[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ro + ty * 4 + i, c = co + tx * 4 + j;
            if (r < K && c < K) gb[(long)r * K + c] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void rbd_fw_panel_kernel(float* g, int K, int p) {
    const int t = blockIdx.x;
    if (t == p) return;                                     // (uniform: before any barrier)
    float* gb = g + (long)blockIdx.z * K * K;
    if (blockIdx.y == 0) rbd_minplus_tile(gb, K, p, t, p);  // block row p:    C = P (x) C
    else rbd_minplus_tile(gb, K, t, p, p);                  // block column p: C = C (x) P
}

__global__ __launch_bounds__(256) void rbd_fw_rest_kernel(float* g, int K, int p) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti == p || tj == p) return;
    rbd_minplus_tile(g + (long)blockIdx.z * K * K, K, ti, tj, p);
}

// ---- the row passes --------------------------------------------------------------------------------------------------------------
// the sum of v over a 256-thread workgroup, to every thread: shuffle fold inside a wave, then the four waves in wave order
__device__ __forceinline__ float rbd_sum256(float v, float* s4) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = ((s4[0] + s4[1]) + s4[2]) + s4[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void rbd_background_kernel(const float* g, const float* stats, int K, float two_clr2, float two_bnd2,
                                                             float* w_bg) {
    __shared__ float s4[4];
    const int b = blockIdx.y, k = blockIdx.x;
    const float* st = stats + (long)b * K * RBD_STAT;
    if (!(st[k * RBD_STAT + 5] > 0.0f)) {                   // uniform
        if (threadIdx.x == 0) w_bg[(long)b * K + k] = 0.0f;
        return;
    }
    const float* row = g + ((long)b * K + k) * K;
    float area = 0.0f, len = 0.0f;
    for (int l = threadIdx.x; l < K; l += 256) {
        if (st[l * RBD_STAT + 5] > 0.0f) {
            const float d = row[l];
            const float e = expf(-(d * d) / two_clr2);
            area += e;
            if (st[l * RBD_STAT + 6] > 0.0f) len += e;
        }
    }
    area = rbd_sum256(area, s4), len = rbd_sum256(len, s4);
    if (threadIdx.x == 0) {
        const float bc = len / sqrtf(area);                 // area >= 1: the cluster's own term
        w_bg[(long)b * K + k] = 1.0f - expf(-(bc * bc) / two_bnd2);
    }
}

__global__ __launch_bounds__(256) void rbd_contrast_kernel(const float* g, const float* stats, const float* w_bg, int K, float diag2,
                                                           float two_spa2, float* wctr) {
    __shared__ float s4[4];
    const int b = blockIdx.y, k = blockIdx.x;
    const float* st = stats + (long)b * K * RBD_STAT;
    if (!(st[k * RBD_STAT + 5] > 0.0f)) {
        if (threadIdx.x == 0) wctr[(long)b * K + k] = 0.0f;
        return;
    }
    const float* row = g + ((long)b * K + k) * K;
    const float* wb = w_bg + (long)b * K;
    const float cy = st[k * RBD_STAT + 3], cx = st[k * RBD_STAT + 4];
    float acc = 0.0f;
    for (int l = threadIdx.x; l < K; l += 256) {
        if (st[l * RBD_STAT + 5] > 0.0f) {                  // an inactive l has G = +inf and w_bg = 0: never multiplied
            const float dy = cy - st[l * RBD_STAT + 3], dx = cx - st[l * RBD_STAT + 4];
            const float d2 = (dy * dy + dx * dx) / diag2;
            acc += row[l] * expf(-d2 / two_spa2) * wb[l];
        }
    }
    acc = rbd_sum256(acc, s4);
    if (threadIdx.x == 0) wctr[(long)b * K + k] = acc;
}

// ---- the solve -------------------------------------------------------------------------------------------------------------------
// min and max of v over the workgroup's threads (exact, so the order is immaterial), to every thread
__device__ __forceinline__ void rbd_minmax(float& lo, float& hi, float* s_lo, float* s_hi) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lo = fminf(lo, __shfl_xor(lo, d, 64)), hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    constexpr int NW = RBD_SOLVE_THREADS / 64;
    if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
    __syncthreads();
    lo = s_lo[0], hi = s_hi[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) lo = fminf(lo, s_lo[w]), hi = fmaxf(hi, s_hi[w]);
    __syncthreads();
}

__global__ __launch_bounds__(RBD_SOLVE_THREADS) void rbd_solve_kernel(const float* g, const float* stats, const uint8_t* adj,
                                                                      const float* w_bg, const float* wctr, int K, float two_clr2,
                                                                      float mu, float* work, float* wctr_norm, float* x, float* xnorm) {
    constexpr int NT = RBD_SOLVE_THREADS, NW = NT / 64;
    __shared__ float s_col[2][RBD_MAX_SEGMENTS];
    __shared__ float s_y[RBD_MAX_SEGMENTS];
    __shared__ float s_w[RBD_MAX_SEGMENTS];
    __shared__ float s_lo[NW], s_hi[NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* gb = g + (long)b * K * K;
    const float* st = stats + (long)b * K * RBD_STAT;
    const uint8_t* ab = adj + (long)b * K * K;
    const float* wb = w_bg + (long)b * K;
    float* A = work + (long)b * K * K;
    const float inf = __builtin_inff();

    // wCtr to [0, 1] over the active clusters
    float lo = inf, hi = -inf;
    for (int k = tid; k < K; k += NT) {
        if (st[k * RBD_STAT + 5] > 0.0f) {
            const float v = wctr[(long)b * K + k];
            lo = fminf(lo, v), hi = fmaxf(hi, v);
        }
    }
    rbd_minmax(lo, hi, s_lo, s_hi);
    for (int k = tid; k < K; k += NT) {
        const float v = (st[k * RBD_STAT + 5] > 0.0f && hi > lo) ? (wctr[(long)b * K + k] - lo) / (hi - lo) : 0.0f;
        s_w[k] = v, wctr_norm[(long)b * K + k] = v;
    }
    __syncthreads();

    // A = diag(2 w_bg + 2 wCtr + 2 sum_l s) - 2 s, lower triangle; an inactive cluster is an identity row and column
    for (int i = wave; i < K; i += NW) {
        const bool act = st[i * RBD_STAT + 5] > 0.0f;
        float rs = 0.0f;
        for (int l = lane; l < K; l += 64) {
            float s = 0.0f;
            if (act && l != i && st[l * RBD_STAT + 5] > 0.0f && (ab[(long)i * K + l] | ab[(long)l * K + i])) {
                const float d = gb[(long)i * K + l];
                s = expf(-(d * d) / two_clr2) + mu;
            }
            if (l < i) A[(long)i * K + l] = -2.0f * s;
            rs += s;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) rs += __shfl_down(rs, d, 64);
        if (lane == 0) {
            A[(long)i * K + i] = act ? (2.0f * wb[i] + 2.0f * s_w[i]) + 2.0f * rs : 1.0f;
            s_y[i] = act ? 2.0f * s_w[i] : 0.0f;
        }
    }
    __syncthreads();
    for (int i = tid; i < K; i += NT) s_col[0][i] = A[(long)i * K];

    // elimination: step j reads column j (left in LDS by step j - 1) and updates the columns after it
    for (int j = 0; j < K; ++j) {
        __syncthreads();
        const float* cur = s_col[j & 1];
        float* nxt = s_col[(j + 1) & 1];
        const float piv = cur[j];
        const float yj = s_y[j];
        for (int i = j + 1 + wave; i < K; i += NW) {
            const float f = cur[i] / piv;
            float* row = A + (long)i * K;
            if (f != 0.0f) {
                for (int c = j + 1 + lane; c <= i; c += 64) {
                    const float v = row[c] - f * cur[c];
                    row[c] = v;
                    if (c == j + 1) nxt[i] = v;
                }
                if (lane == 0) s_y[i] -= f * yj;
            } else if (lane == 0) {
                nxt[i] = row[j + 1];
            }
        }
    }
    // back substitution: U[i][j] = A[j][i] (i < j), so unknown j is taken out of the rows above it along row j of the store
    for (int j = K - 1; j >= 0; --j) {
        __syncthreads();
        const float xj = s_y[j] / A[(long)j * K + j];
        for (int i = tid; i < j; i += NT) s_y[i] -= A[(long)j * K + i] * xj;
        if (tid == 0) s_w[j] = xj;                          // s_w is free from here on: it becomes x
    }
    __syncthreads();

    lo = inf, hi = -inf;
    for (int k = tid; k < K; k += NT) {
        const bool act = st[k * RBD_STAT + 5] > 0.0f;
        const float v = act ? s_w[k] : 0.0f;
        x[(long)b * K + k] = v;
        if (act) lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    rbd_minmax(lo, hi, s_lo, s_hi);
    for (int k = tid; k < K; k += NT)
        xnorm[(long)b * K + k] = (st[k * RBD_STAT + 5] > 0.0f && hi > lo) ? (s_w[k] - lo) / (hi - lo) : 0.0f;
}

__global__ __launch_bounds__(256) void rbd_paint_kernel(const float* xnorm, const int* labels, RbdGrid q, float* sal) {
    const long N = (long)q.H * q.W, total = N * q.B;
    const int K = q.gy * q.gx;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / N, i = idx - b * N;
        const int y = (int)(i / q.W), x = (int)(i - (long)y * q.W);
        const int l = rbd_label(labels + b * N, y, x, q);
        sal[idx] = l >= 0 ? xnorm[b * K + l] : 0.0f;
    }
}

static int rbd_fail(const char* who, const char* what) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

static int rbd_done(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s kernel: %s", who, hipGetErrorString(e));
    return vqseg_set_error((int)e, buf);
}

static const char* rbd_grid_error(int b, int h, int w, int gy, int gx) {
    if (b <= 0 || h <= 0 || w <= 0) return "b, h and w must be positive";
    if (b > 65535) return "at most 65535 images per launch";
    if (h > RBD_MAX_SIDE || w > RBD_MAX_SIDE) return "a side above 4096";
    if (gy < 1 || gx < 1 || gy > h || gx > w) return "the grid must have 1..h rows and 1..w columns of cells (a cell is at least one pixel)";
    if ((long)gy * gx > RBD_MAX_SEGMENTS) return "at most 1024 superpixels (RBD_MAX_SEGMENTS)";
    return nullptr;
}

static const char* rbd_table_error(int b, int k) {
    if (b <= 0 || k <= 0) return "b and k must be positive";
    if (b > 65535) return "at most 65535 images per launch";
    if (k > RBD_MAX_SEGMENTS) return "at most 1024 superpixels (RBD_MAX_SEGMENTS)";
    return nullptr;
}

static bool rbd_sigma_ok(float s) { return s > 0.0f && s <= 1e18f; }

static unsigned rbd_blocks(int64_t elems) {
    const int64_t blocks = (elems + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

}  // namespace vqseg

extern "C" {

int vqseg_region_graph_f(const float* lab, const int32_t* labels, int b, int h, int w, int gy, int gx, float* stats, uint8_t* adj,
                         void* stream) {
    using namespace vqseg;
    if (!lab || !labels || !stats || !adj) return rbd_fail("region_graph", "null lab, labels, stats or adj");
    if (const char* e = rbd_grid_error(b, h, w, gy, gx)) return rbd_fail("region_graph", e);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int k = gy * gx;
    const hipError_t e = hipMemsetAsync(adj, 0, (size_t)b * k * k, st);
    if (e != hipSuccess) {
        char buf[200];
        snprintf(buf, sizeof(buf), "region_graph memset: %s", hipGetErrorString(e));
        return vqseg_set_error((int)e, buf);
    }
    const RbdGrid q = {b, h, w, gy, gx};
    hipLaunchKernelGGL(rbd_region_kernel, dim3((unsigned)k, (unsigned)b), dim3(256), 0, st, lab, labels, q, stats, adj);
    return rbd_done("region_graph");
}

int vqseg_rbd_weights_f(const float* stats, const uint8_t* adj, int b, int k, float* weights, void* stream) {
    using namespace vqseg;
    if (!stats || !adj || !weights) return rbd_fail("rbd_weights", "null stats, adj or weights");
    if (const char* e = rbd_table_error(b, k)) return rbd_fail("rbd_weights", e);
    hipLaunchKernelGGL(rbd_weights_kernel, dim3(rbd_blocks((int64_t)b * k * k)), dim3(256), 0, static_cast<hipStream_t>(stream), stats, adj, b,
                       k, weights);
    return rbd_done("rbd_weights");
}

int vqseg_rbd_geodesic_f(float* g, int b, int k, void* stream) {
    using namespace vqseg;
    if (!g) return rbd_fail("rbd_geodesic", "null g");
    if (const char* e = rbd_table_error(b, k)) return rbd_fail("rbd_geodesic", e);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = (k + RBD_T - 1) / RBD_T;
    for (int p = 0; p < nb; ++p) {
        hipLaunchKernelGGL(rbd_fw_pivot_kernel, dim3((unsigned)b), dim3(256), 0, st, g, k, p);
        if (nb > 1) {
            hipLaunchKernelGGL(rbd_fw_panel_kernel, dim3((unsigned)nb, 2, (unsigned)b), dim3(256), 0, st, g, k, p);
            hipLaunchKernelGGL(rbd_fw_rest_kernel, dim3((unsigned)nb, (unsigned)nb, (unsigned)b), dim3(256), 0, st, g, k, p);
        }
        if (const int rc = rbd_done("rbd_geodesic")) return rc;
    }
    return 0;
}

int vqseg_rbd_background_f(const float* g, const float* stats, int b, int k, float sigma_clr, float sigma_bndcon, float* w_bg, void* stream) {
    using namespace vqseg;
    if (!g || !stats || !w_bg) return rbd_fail("rbd_background", "null g, stats or w_bg");
    if (const char* e = rbd_table_error(b, k)) return rbd_fail("rbd_background", e);
    if (!rbd_sigma_ok(sigma_clr) || !rbd_sigma_ok(sigma_bndcon)) return rbd_fail("rbd_background", "the sigmas must lie in (0, 1e18]");
    hipLaunchKernelGGL(rbd_background_kernel, dim3((unsigned)k, (unsigned)b), dim3(256), 0, static_cast<hipStream_t>(stream), g, stats, k,
                       2.0f * sigma_clr * sigma_clr, 2.0f * sigma_bndcon * sigma_bndcon, w_bg);
    return rbd_done("rbd_background");
}

int vqseg_rbd_contrast_f(const float* g, const float* stats, const float* w_bg, int b, int k, int h, int w, float sigma_spa, float* wctr,
                         void* stream) {
    using namespace vqseg;
    if (!g || !stats || !w_bg || !wctr) return rbd_fail("rbd_contrast", "null g, stats, w_bg or wctr");
    if (const char* e = rbd_table_error(b, k)) return rbd_fail("rbd_contrast", e);
    if (h <= 0 || w <= 0 || h > RBD_MAX_SIDE || w > RBD_MAX_SIDE) return rbd_fail("rbd_contrast", "sides of 1..4096");
    if (!rbd_sigma_ok(sigma_spa)) return rbd_fail("rbd_contrast", "sigma_spa must lie in (0, 1e18]");
    hipLaunchKernelGGL(rbd_contrast_kernel, dim3((unsigned)k, (unsigned)b), dim3(256), 0, static_cast<hipStream_t>(stream), g, stats, w_bg, k,
                       (float)((long)h * h + (long)w * w), 2.0f * sigma_spa * sigma_spa, wctr);
    return rbd_done("rbd_contrast");
}

int vqseg_rbd_solve_f(const float* g, const float* stats, const uint8_t* adj, const float* w_bg, const float* wctr, int b, int k,
                      float sigma_clr, float mu, float* work, float* wctr_norm, float* x, float* xnorm, void* stream) {
    using namespace vqseg;
    if (!g || !stats || !adj || !w_bg || !wctr || !work || !wctr_norm || !x || !xnorm)
        return rbd_fail("rbd_solve", "null g, stats, adj, w_bg, wctr, work, wctr_norm, x or xnorm");
    if (const char* e = rbd_table_error(b, k)) return rbd_fail("rbd_solve", e);
    if (!rbd_sigma_ok(sigma_clr)) return rbd_fail("rbd_solve", "sigma_clr must lie in (0, 1e18]");
    if (!(mu >= 0.0f && mu <= 1e18f)) return rbd_fail("rbd_solve", "mu must lie in [0, 1e18]");
    hipLaunchKernelGGL(rbd_solve_kernel, dim3((unsigned)b), dim3(RBD_SOLVE_THREADS), 0, static_cast<hipStream_t>(stream), g, stats, adj, w_bg,
                       wctr, k, 2.0f * sigma_clr * sigma_clr, mu, work, wctr_norm, x, xnorm);
    return rbd_done("rbd_solve");
}

int vqseg_rbd_paint_f(const float* xnorm, const int32_t* labels, int b, int h, int w, int gy, int gx, float* sal, void* stream) {
    using namespace vqseg;
    if (!xnorm || !labels || !sal) return rbd_fail("rbd_paint", "null xnorm, labels or sal");
    if (const char* e = rbd_grid_error(b, h, w, gy, gx)) return rbd_fail("rbd_paint", e);
    const RbdGrid q = {b, h, w, gy, gx};
    hipLaunchKernelGGL(rbd_paint_kernel, dim3(rbd_blocks((int64_t)b * h * w)), dim3(256), 0, static_cast<hipStream_t>(stream), xnorm, labels, q,
                       sal);
    return rbd_done("rbd_paint");
}

}  // extern "C"
