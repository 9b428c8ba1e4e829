// boundary_kernels.hip -- contour-level scoring on the device: the class boundaries of a label map, the exact squared Euclidean distance
// transform of seed planes, and the per-image, per-class count table behind boundary F1, boundary IoU and the Hausdorff distance
// (vq_seg_amd/nnf.py: class_boundaries, edt_sq, boundary_counts; vq_seg_amd/utils/boundary.py; evaluate.test_loop(boundary=...)).
// The definition is stated in include/vqseg.h; here is how the kernels meet it.
//
// boundary_seeds_kernel  a thread per pixel: its value and its four neighbours inside the image; the pixel is a seed of its own class's
//                        plane when one of them is neither that value nor ignored.  Every plane of the pixel is written (C byte stores,
//                        each coalesced along the row).  The class is a loop counter compared with the value, never an index made of it.
// edt_rows_kernel        a workgroup per plane row.  Nearest seed to the left and to the right of every pixel without a scan loop: a wave
//                        ballots the seeds of its 64 columns into one 64-bit word in LDS (at most 32 words per row), wave 0 ballots which
//                        words are non-zero, and a pixel finds the nearest set bit on either side with clz / ctz on its own word, else on
//                        the nearest non-zero word.  g = the smaller distance (u16), EDT_ROW_NONE for a row without a seed; row_has[row]
//                        says whether the row has one.
// edt_cols_kernel        a workgroup per 64 columns x 64 rows of a plane.  It first compacts the plane's rows that have a seed into a list
//                        in LDS (rank[y] = how many such rows lie above y), so rows without a seed are never visited and a plane without
//                        any is filled with EDT_NONE at once.  A lane owns a column (adjacent lanes adjacent columns: every load of a row
//                        of g is coalesced) and searches the list outwards from y, downwards then upwards, and stops a direction as soon
//                        as dy^2 >= best.  Exact: the minimum over j of g[j][x]^2 + (y - j)^2 in int32.
// boundary_counts_kernel a workgroup per 2048 consecutive pixels of one image, eight per thread, kept in registers.  For every class that
//                        occurs among a wave's pixels the lanes gather their eight columns, the wave folds them by shuffles, and lane 0
//                        makes one atomicAdd / atomicMax per column that has something to add.  A pixel touches the planes of its
//                        predicted and of its target class only.
// Integer atomics only; no workgroup waits for another; every loop is bounded by h, w, the class count or a constant.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int EDT_MAX_SIDE = 2048;
constexpr int EDT_MAX_PLANES = 1 << 19;
constexpr int EDT_WORDS = EDT_MAX_SIDE / 64;                 // ballot words of one row
constexpr unsigned EDT_ROW_NONE = 0xffffu;                   // g of a row without a seed
constexpr int EDT_TILE = 64;                                 // rows and columns of a column-pass tile
constexpr int BND_MAX_CLASSES = 32;
constexpr int BND_SPAN = 2048;                               // pixels per workgroup of the counts: eight per thread
constexpr int BND_GRID_Y = 32768;                            // planes (images) go to grid y and z: index = z * BND_GRID_Y + y, so no grid dimension
                                                             // times the 256 threads of a workgroup comes near 2^32 at 2^19 planes

struct BndIgnore {
    int n, v[4];
};

__device__ __forceinline__ bool bnd_ignored(int v, const BndIgnore& q) {
    bool ig = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) ig |= k < q.n && v == q.v[k];
    return ig;
}

template <typename T>
__global__ __launch_bounds__(256) void boundary_seeds_kernel(const T* labels, int B, int H, int W, int C, BndIgnore q, uint8_t* seeds) {
    const long n = (long)H * W, total = (long)B * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / n, p = idx - b * n;
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const int v = (int)labels[idx];
        bool edge = false;
        if (x > 0) { const int u = (int)labels[idx - 1]; edge |= u != v && !bnd_ignored(u, q); }
        if (x + 1 < W) { const int u = (int)labels[idx + 1]; edge |= u != v && !bnd_ignored(u, q); }
        if (y > 0) { const int u = (int)labels[idx - W]; edge |= u != v && !bnd_ignored(u, q); }
        if (y + 1 < H) { const int u = (int)labels[idx + W]; edge |= u != v && !bnd_ignored(u, q); }
        uint8_t* out = seeds + b * C * n + p;
        for (int c = 0; c < C; ++c) out[(long)c * n] = (uint8_t)(edge && v == c);
    }
}

__global__ __launch_bounds__(256) void edt_rows_kernel(const uint8_t* seeds, int planes, int H, int W, uint16_t* g, uint8_t* row_has) {
    __shared__ unsigned long long s_mask[EDT_WORDS];
    __shared__ unsigned s_nz;
    const int plane = blockIdx.z * BND_GRID_Y + blockIdx.y;
    if (plane >= planes) return;                             // (uniform over the workgroup, before any barrier)
    const long row = (long)plane * H + blockIdx.x;
    const uint8_t* sr = seeds + row * W;
    uint16_t* gr = g + row * W;
    const int t = threadIdx.x, lane = t & 63;
    const int trips = (W + 255) >> 8;                        // <= 8
    for (int k = 0; k < trips; ++k) {
        const int x = k * 256 + t;
        const unsigned long long m = __ballot(x < W && sr[x] != 0);
        if (lane == 0) s_mask[x >> 6] = m;                   // x >> 6 < 32: every word up to the last trip's is written, a zero past the row
    }
    __syncthreads();
    if (t < 64) {
        const int words = trips * 4;
        const unsigned long long nz = __ballot(t < words && s_mask[t] != 0);
        if (t == 0) s_nz = (unsigned)nz;
    }
    __syncthreads();
    const unsigned nz = s_nz;
    if (t == 0) row_has[row] = nz != 0;
    for (int k = 0; k < trips; ++k) {
        const int x = k * 256 + t;
        if (x >= W) break;
        unsigned d = EDT_ROW_NONE;
        if (nz) {
            const int wd = x >> 6, bit = x & 63;
            const unsigned long long own = s_mask[wd];
            int left = -1, right = -1;                       // columns of the nearest seeds at or before x, at or after x
            const unsigned long long lo = own & (~0ull >> (63 - bit));
            if (lo) {
                left = wd * 64 + 63 - __builtin_clzll(lo);
            } else {
                const unsigned before = wd > 0 ? nz & (~0u >> (32 - wd)) : 0u;
                if (before) {
                    const int pw = 31 - __builtin_clz(before);
                    left = pw * 64 + 63 - __builtin_clzll(s_mask[pw]);
                }
            }
            const unsigned long long hi = own >> bit;
            if (hi) {
                right = x + __builtin_ctzll(hi);
            } else {
                const unsigned after = wd < 31 ? nz >> (wd + 1) : 0u;
                if (after) {
                    const int nw = wd + 1 + __builtin_ctz(after);
                    right = nw * 64 + __builtin_ctzll(s_mask[nw]);
                }
            }
            const unsigned dl = left >= 0 ? (unsigned)(x - left) : EDT_ROW_NONE;
            const unsigned dr = right >= 0 ? (unsigned)(right - x) : EDT_ROW_NONE;
            d = dl < dr ? dl : dr;
        }
        gr[x] = (uint16_t)d;
    }
}

__global__ __launch_bounds__(256) void edt_cols_kernel(const uint16_t* g, const uint8_t* row_has, int planes, int H, int W, int tiles_x,
                                                       int32_t* d2) {
    __shared__ uint16_t s_list[EDT_MAX_SIDE];                // the rows of the plane that have a seed, rising
    __shared__ uint16_t s_rank[EDT_MAX_SIDE];                // how many of them lie above row y
    __shared__ int s_wave[4];
    __shared__ int s_total;
    const int plane = blockIdx.z * BND_GRID_Y + blockIdx.y;
    if (plane >= planes) return;                             // (uniform over the workgroup, before any barrier)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint8_t* fl = row_has + (long)plane * H;
    int base = 0;
    const int trips = (H + 255) >> 8;                        // <= 8, uniform over the workgroup
    for (int k = 0; k < trips; ++k) {
        const int y = k * 256 + t;
        const bool has = y < H && fl[y] != 0;
        const unsigned long long m = __ballot(has);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int at = base + __popcll(m & ~(~0ull << lane));
        for (int w2 = 0; w2 < wave; ++w2) at += s_wave[w2];
        if (y < H) {
            s_rank[y] = (uint16_t)at;
            if (has) s_list[at] = (uint16_t)y;
        }
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();                                     // before the next trip overwrites the wave counts
    }
    if (t == 0) s_total = base;
    __syncthreads();
    const int n = s_total;
    const int x = tx * EDT_TILE + lane;
    if (x >= W) return;
    const uint16_t* gp = g + (long)plane * H * W;
    int32_t* dp = d2 + (long)plane * H * W;
    const int y0 = ty * EDT_TILE;
    for (int i = 0; i < EDT_TILE / 4; ++i) {
        const int y = y0 + wave + 4 * i;
        if (y >= H) break;
        int best = VQSEG_EDT_NONE;
        const int at = s_rank[y];                            // the first listed row at or below y
        for (int k = at; k < n; ++k) {
            const int j = s_list[k], dy = j - y;
            if (dy * dy >= best) break;
            const int v = gp[(long)j * W + x];
            if (v != (int)EDT_ROW_NONE) {
                const int c = v * v + dy * dy;
                best = c < best ? c : best;
            }
        }
        for (int k = at - 1; k >= 0; --k) {
            const int j = s_list[k], dy = y - j;
            if (dy * dy >= best) break;
            const int v = gp[(long)j * W + x];
            if (v != (int)EDT_ROW_NONE) {
                const int c = v * v + dy * dy;
                best = c < best ? c : best;
            }
        }
        dp[(long)y * W + x] = best;
    }
}

__global__ __launch_bounds__(256) void boundary_table_init_kernel(int32_t* table, long rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < rows * 8) table[i] = (i & 7) >= 6 ? -1 : 0;
}

struct CountArgs {
    const void* pred;
    const void* target;
    int pred_bytes, target_bytes;                            // 1 (u8) or 4 (i32)
    const uint8_t* bp;
    const uint8_t* bg;
    const int32_t* dp;
    const int32_t* dg;
    int B, H, W, C, tol_sq, width_sq;
    BndIgnore ig;
    int32_t* table;                                          // [B][C][8]
};

__device__ __forceinline__ int bnd_label(const void* p, int bytes, long i) {
    return bytes == 1 ? (int)static_cast<const uint8_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
}

__global__ __launch_bounds__(256) void boundary_counts_kernel(const CountArgs a) {
    const long n = (long)a.H * a.W;
    const long b = (long)blockIdx.z * BND_GRID_Y + blockIdx.y;
    if (b >= a.B) return;                                    // (uniform over the workgroup; the kernel has no barrier)
    const long p0 = (long)blockIdx.x * BND_SPAN + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int pv[8], tv[8];
    bool ok[8];                                              // a pixel of the image whose target is not ignored
    unsigned seen_p = 0, seen_t = 0;                         // the classes among this lane's pixels, as bits
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long p = p0 + i * 256;
        pv[i] = tv[i] = -1, ok[i] = false;
        if (p < n) {
            pv[i] = bnd_label(a.pred, a.pred_bytes, b * n + p);
            tv[i] = bnd_label(a.target, a.target_bytes, b * n + p);
            ok[i] = !bnd_ignored(tv[i], a.ig);
            if (ok[i] && pv[i] >= 0 && pv[i] < a.C) seen_p |= 1u << pv[i];
            if (ok[i] && tv[i] >= 0 && tv[i] < a.C) seen_t |= 1u << tv[i];
        }
    }
    unsigned seen = seen_p | seen_t;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) seen |= __shfl_xor(seen, d, 64);     // of the wave
    for (int c = 0; c < a.C; ++c) {
        if (!(seen >> c & 1u)) continue;                     // (uniform over the wave)
        const long plane = (b * a.C + c) * n;
        int col[6] = {0, 0, 0, 0, 0, 0};
        int hd_p = -1, hd_g = -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool isp = ok[i] && pv[i] == c, isg = ok[i] && tv[i] == c;
            if (!isp && !isg) continue;
            const long at = plane + p0 + i * 256;
            const int dp = a.dp[at], dg = a.dg[at];
            bool pd = false, gd = false;
            if (isp) {
                if (a.bp[at]) {
                    col[0] += 1, col[1] += dg <= a.tol_sq;
                    const int far = dg == VQSEG_EDT_NONE ? -1 : dg;
                    hd_p = far > hd_p ? far : hd_p;
                }
                pd = dp <= a.width_sq;
            }
            if (isg) {
                if (a.bg[at]) {
                    col[2] += 1, col[3] += dp <= a.tol_sq;
                    const int far = dp == VQSEG_EDT_NONE ? -1 : dp;
                    hd_g = far > hd_g ? far : hd_g;
                }
                gd = dg <= a.width_sq;
            }
            col[4] += pd && gd, col[5] += pd || gd;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) col[k] += __shfl_xor(col[k], d, 64);
            const int op = __shfl_xor(hd_p, d, 64), og = __shfl_xor(hd_g, d, 64);
            hd_p = op > hd_p ? op : hd_p, hd_g = og > hd_g ? og : hd_g;
        }
        if (lane == 0) {
            int32_t* row = a.table + (b * a.C + c) * 8;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (col[k]) atomicAdd(row + k, col[k]);
            if (hd_p >= 0) atomicMax(row + 6, hd_p);
            if (hd_g >= 0) atomicMax(row + 7, hd_g);
        }
    }
}

static int bnd_fail(const char* who, const char* what) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

static int bnd_done(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, hipGetErrorString(e));
    return vqseg_set_error((int)e, buf);
}

static const char* bnd_map_error(int b, int h, int w, int num_classes, int n_ignore) {
    if (b < 1 || h < 1 || w < 1) return "b, h and w must be positive";
    if (h > EDT_MAX_SIDE || w > EDT_MAX_SIDE) return "a side above 2048";
    if (num_classes < 1 || num_classes > BND_MAX_CLASSES) return "num_classes must lie in 1..32";
    if ((int64_t)b * num_classes > EDT_MAX_PLANES) return "at most 2^19 planes (b * num_classes) per launch";
    if (n_ignore < 0 || n_ignore > 4) return "0 to 4 ignored values";
    return nullptr;
}

static const char* edt_plane_error(int planes, int h, int w) {
    if (planes < 1 || h < 1 || w < 1) return "planes, h and w must be positive";
    if (h > EDT_MAX_SIDE || w > EDT_MAX_SIDE) return "a side above 2048";
    if (planes > EDT_MAX_PLANES) return "at most 2^19 planes per launch";
    return nullptr;
}

static dim3 bnd_grid(unsigned x, int count) {                // `count` planes or images in y and z
    const unsigned y = count < BND_GRID_Y ? (unsigned)count : (unsigned)BND_GRID_Y;
    return dim3(x, y, (unsigned)((count + BND_GRID_Y - 1) / BND_GRID_Y));
}

static unsigned bnd_blocks(int64_t elems) {
    const int64_t blocks = (elems + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

template <typename T>
static int boundary_seeds(const char* who, const T* labels, int b, int h, int w, int num_classes, int n_ignore, const int* ignore,
                          uint8_t* seeds, void* stream) {
    if (!labels || !seeds) return bnd_fail(who, "null labels or seeds");
    if (const char* e = bnd_map_error(b, h, w, num_classes, n_ignore)) return bnd_fail(who, e);
    BndIgnore q = {n_ignore, {ignore[0], ignore[1], ignore[2], ignore[3]}};
    hipLaunchKernelGGL(boundary_seeds_kernel<T>, dim3(bnd_blocks((int64_t)b * h * w)), dim3(256), 0, static_cast<hipStream_t>(stream), labels, b,
                       h, w, num_classes, q, seeds);
    return bnd_done(who);
}

}  // namespace vqseg

extern "C" {

int vqseg_boundary_seeds_u8(const uint8_t* labels, int b, int h, int w, int num_classes, int n_ignore, int ignore0, int ignore1, int ignore2,
                            int ignore3, uint8_t* seeds, void* stream) {
    const int ignore[4] = {ignore0, ignore1, ignore2, ignore3};
    return vqseg::boundary_seeds<uint8_t>("boundary_seeds_u8", labels, b, h, w, num_classes, n_ignore, ignore, seeds, stream);
}

int vqseg_boundary_seeds_i32(const int32_t* labels, int b, int h, int w, int num_classes, int n_ignore, int ignore0, int ignore1, int ignore2,
                             int ignore3, uint8_t* seeds, void* stream) {
    const int ignore[4] = {ignore0, ignore1, ignore2, ignore3};
    return vqseg::boundary_seeds<int32_t>("boundary_seeds_i32", labels, b, h, w, num_classes, n_ignore, ignore, seeds, stream);
}

int vqseg_boundary_edt_rows_u8(const uint8_t* seeds, int planes, int h, int w, uint16_t* g, uint8_t* row_has, void* stream) {
    using namespace vqseg;
    if (!seeds || !g || !row_has) return bnd_fail("boundary_edt_rows", "null seeds, g or row_has");
    if (const char* e = edt_plane_error(planes, h, w)) return bnd_fail("boundary_edt_rows", e);
    hipLaunchKernelGGL(edt_rows_kernel, bnd_grid((unsigned)h, planes), dim3(256), 0, static_cast<hipStream_t>(stream), seeds, planes, h, w, g,
                       row_has);
    return bnd_done("boundary_edt_rows");
}

int vqseg_boundary_edt_cols_i32(const uint16_t* g, const uint8_t* row_has, int planes, int h, int w, int32_t* d2, void* stream) {
    using namespace vqseg;
    if (!g || !row_has || !d2) return bnd_fail("boundary_edt_cols", "null g, row_has or d2");
    if (const char* e = edt_plane_error(planes, h, w)) return bnd_fail("boundary_edt_cols", e);
    const int tiles_x = (w + EDT_TILE - 1) / EDT_TILE, tiles_y = (h + EDT_TILE - 1) / EDT_TILE;
    hipLaunchKernelGGL(edt_cols_kernel, bnd_grid((unsigned)(tiles_x * tiles_y), planes), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       row_has, planes, h, w, tiles_x, d2);
    return bnd_done("boundary_edt_cols");
}

int vqseg_boundary_counts_i32(const void* pred, int pred_bytes, const void* target, int target_bytes, const uint8_t* bp, const uint8_t* bg,
                              const int32_t* dp, const int32_t* dg, int b, int h, int w, int num_classes, int tol_sq, int width_sq,
                              int n_ignore, int ignore0, int ignore1, int ignore2, int ignore3, int32_t* table, void* stream) {
    using namespace vqseg;
    const char* who = "boundary_counts";
    if (!pred || !target || !bp || !bg || !dp || !dg || !table) return bnd_fail(who, "null pred, target, bp, bg, dp, dg or table");
    if ((pred_bytes != 1 && pred_bytes != 4) || (target_bytes != 1 && target_bytes != 4))
        return bnd_fail(who, "pred_bytes and target_bytes are 1 (u8) or 4 (i32)");
    if (const char* e = bnd_map_error(b, h, w, num_classes, n_ignore)) return bnd_fail(who, e);
    if (tol_sq < 0 || width_sq < 0 || tol_sq == VQSEG_EDT_NONE || width_sq == VQSEG_EDT_NONE)
        return bnd_fail(who, "tol_sq and width_sq must lie in 0..2^31 - 2");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t rows = (int64_t)b * num_classes;
    hipLaunchKernelGGL(boundary_table_init_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st, table, (long)rows);
    CountArgs a = {pred, target, pred_bytes, target_bytes, bp, bg, dp, dg, b, h, w, num_classes, tol_sq, width_sq,
                   {n_ignore, {ignore0, ignore1, ignore2, ignore3}}, table};
    const int64_t per = ((int64_t)h * w + BND_SPAN - 1) / BND_SPAN;
    hipLaunchKernelGGL(boundary_counts_kernel, bnd_grid((unsigned)per, b), dim3(256), 0, st, a);
    return bnd_done(who);
}

}  // extern "C"
