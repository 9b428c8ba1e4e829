// region_kernels.hip -- connected regions of an integer map on the device: roots, ids, the instance table, areas and the area filter
// (vq_seg_amd/nnf.py: region_roots, region_ids, region_table, region_areas, filter_regions; vq_seg_amd/utils/regions.py;
// predict.Predictor(min_area=...), CPSConfig.pseudo_min_area).  The definition is stated in include/vqseg.h; here is how the kernels meet it.
//
// region_local_kernel    a workgroup owns a tile of 16 rows x 64 columns of one image, a thread four pixels of one column.  Union-find in
//                        LDS over the tile's own index li = ly * 64 + lx, which rises with the row-major index of the image: a pixel starts
//                        at the head of its horizontal run (a wave holds a row: one ballot) and links to its upper neighbour (and the two
//                        upper diagonals for 8) of equal value by find + atomicMin on the larger root, so parents only ever fall and a
//                        tree's root is its smallest index; links that other links imply are not made.  After a barrier every pixel
//                        follows its chain and stores the GLOBAL index of its local root; -1 for an ignored pixel.
// region_merge_kernel    the same grid: the tile's top row, left column and right column join across the tile border with the same rule
//                        on the global parent array (the links a pixel has are those above; exactly those that leave the tile are made
//                        here, the two diagonals across a tile corner included).  `find` loads are agent-scope relaxed atomic loads.
// region_flatten_kernel  a thread per pixel follows its chain in `parent` and writes the root to ANOTHER buffer.
// region_flags_kernel    a workgroup counts the roots (root[p] == p) among 1024 consecutive pixels of one image -> partial[b][blk]
// region_scan_kernel     a workgroup per image: the exclusive prefix sum of its partials in place, and count[b]
// region_rank_kernel     the workgroup of region_flags_kernel again: id[p] = partial + the rank of p among its block's roots, for roots only
// region_gather_kernel   every other pixel: id[p] = id[root[p]] (roots are not written in this launch), -1 where there is no region
// region_table_*         `init` lets every root with a row write the columns it knows alone (value, ymin, root) and its own position as
//                        the start of the bounding box; `fold` adds area, box and moments with integer atomics, one set per RUN of equal
//                        ids among a wave's 64 consecutive pixels (segmented folds by shuffles, as seg_sums_kernel does for its floats),
//                        gathered per workgroup in a small LDS table first.
// region_areas_kernel    the same runs on root, gathered per workgroup in a small LDS table first: one atomicAdd per root and 256 pixels.
// region_filter_kernel   a gather: root, area[root], and the input value of the pixel before the root.
// No workgroup waits for another; every find / union loop is bounded by the number of indices it runs over and falls through.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vqseg.h"

extern "C" int vqseg_set_error(int code, const char* msg);   // vqseg_abi.hip

namespace vqseg {

constexpr int REG_TX = 64;                                  // columns of a tile: one per lane, 64 contiguous elements per row
constexpr int REG_TY = 16;                                  // rows of it: four per wave
constexpr int REG_TILE = REG_TX * REG_TY;
constexpr int REG_MAX_SIDE = 4096;
constexpr int REG_BLOCK = 1024;                             // pixels per workgroup of the compaction: four per thread

struct RegionMap {
    int B, H, W, conn;
    int n_ignore, ignore[4];
};

__device__ __forceinline__ bool reg_ignored(int v, const RegionMap& q) {
    bool ig = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) ig |= k < q.n_ignore && v == q.ignore[k];
    return ig;
}

// LDS union-find.  Other threads lower parents while this one reads them: every read is an atomic load, never a cached register.
__device__ __forceinline__ int reg_find_lds(int* parent, int i) {
    for (int n = 0; n < REG_TILE; ++n) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == i) break;
        i = p;
    }
    return i;
}

__device__ __forceinline__ void reg_union_lds(int* parent, int a, int b) {
    for (int n = 0; n < REG_TILE; ++n) {
        a = reg_find_lds(parent, a), b = reg_find_lds(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b, b = t; }       // a is the larger root
        const int old = atomicMin(parent + a, b);
        if (old == a) return;                               // a was still a root: linked
        a = old;                                            // somebody lowered it first: go on with (old, b)
    }
}

template <typename T>
__global__ __launch_bounds__(256) void region_local_kernel(const T* values, RegionMap q, int* parent_out) {
    __shared__ int s_val[REG_TILE];
    __shared__ int s_par[REG_TILE];
    const int H = q.H, W = q.W;
    const long N = (long)H * W;
    const int x0 = blockIdx.x * REG_TX, y0 = blockIdx.y * REG_TY;
    const T* vb = values + (long)blockIdx.z * N;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly, li = ly * REG_TX + lx;
        const bool in = x < W && y < H;
        const int v = in ? (int)vb[(long)y * W + x] : 0;
        const bool valid = in && !reg_ignored(v, q);
        // a wave holds one row of the tile: a pixel starts at the first pixel of its horizontal run, which makes every left link
        const int vl = __shfl_up(v, 1, 64), validl = __shfl_up((int)valid, 1, 64);
        const bool head = !(lx > 0 && valid && validl && vl == v);
        const unsigned long long heads = __ballot(head);    // (lane 0 is always a head)
        const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lx)));
        s_val[li] = v;
        s_par[li] = valid ? ly * REG_TX + start : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, li = ly * REG_TX + lx;
        if (s_par[li] < 0) continue;                        // (-1 never changes: only indices >= 0 are ever written)
        const int v = s_val[li];
        if (ly > 0) {
            // Links that others imply are not made: the upper link where the left neighbours of both pixels belong to their runs (the
            // pixel to the left makes it), a diagonal link where the upper link exists (the upper row's run holds the diagonal pixel).
            const int up = li - REG_TX;
            const bool sl = lx > 0 && s_par[li - 1] >= 0 && s_val[li - 1] == v;
            const bool su = s_par[up] >= 0 && s_val[up] == v;
            const bool sul = lx > 0 && s_par[up - 1] >= 0 && s_val[up - 1] == v;
            const bool sur = lx < REG_TX - 1 && s_par[up + 1] >= 0 && s_val[up + 1] == v;
            if (su && !(sl && sul)) reg_union_lds(s_par, li, up);
            if (q.conn == 8 && !su) {
                if (sul) reg_union_lds(s_par, li, up - 1);
                if (sur) reg_union_lds(s_par, li, up + 1);
            }
        }
    }
    __syncthreads();
    int* pb = parent_out + (long)blockIdx.z * N;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly, li = ly * REG_TX + lx;
        if (x >= W || y >= H) continue;
        int r = -1;
        if (s_par[li] >= 0) {
            const int lr = reg_find_lds(s_par, li);         // nobody writes any more
            r = (y0 + lr / REG_TX) * W + x0 + (lr & (REG_TX - 1));
        }
        pb[(long)y * W + x] = r;
    }
}

// global union-find of one image (n indices).  Parents written by a workgroup on another XCD must not be read stale from a cache.
__device__ __forceinline__ int reg_find(int* parent, int i, int n) {
    for (int t = 0; t < n; ++t) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == i || p < 0 || p >= n) break;               // (a parent is an index of the image by construction; never trusted)
        i = p;
    }
    return i;
}

__device__ __forceinline__ void reg_union(int* parent, int a, int b, int n) {
    for (int t = 0; t < n; ++t) {
        a = reg_find(parent, a, n), b = reg_find(parent, b, n);
        if (a == b) return;
        if (a < b) { const int s = a; a = b, b = s; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

template <typename T>
__global__ __launch_bounds__(128) void region_merge_kernel(const T* values, RegionMap q, int* parent) {
    const int H = q.H, W = q.W;
    const int n = H * W;                                    // <= 2^24
    const int x0 = blockIdx.x * REG_TX, y0 = blockIdx.y * REG_TY;
    const T* vb = values + (long)blockIdx.z * n;
    int* pb = parent + (long)blockIdx.z * n;
    const int t = threadIdx.x;
    // the pixel (y, x) of this thread and which of its links (left, up, up-left, up-right) leave the tile
    int y, x;
    bool left = false, up = false, upl = false, upr = false;
    if (t < 64) {                                           // the top row: everything that goes up
        y = y0, x = x0 + t;
        up = true, upl = upr = q.conn == 8;
    } else if (t < 80) {                                    // the left column: left, and up-left below the corner (the top row made the corner's)
        y = y0 + (t - 64), x = x0;
        left = true, upl = q.conn == 8 && t > 64;
    } else if (t < 96) {                                    // the right column: up-right below the corner
        y = y0 + (t - 80), x = x0 + REG_TX - 1;
        upr = q.conn == 8 && t > 80;
    } else {
        return;
    }
    if (y >= H || x >= W) return;
    const int i = y * W + x;
    const int v = (int)vb[i];
    if (reg_ignored(v, q)) return;
    // (a value equal to v is not an ignored one.)  The links that others imply are left out as in the local kernel; the horizontal links
    // they rest on are made there or by the left-column threads here.
    const bool sl = x > 0 && (int)vb[i - 1] == v;
    if (left && sl) reg_union(pb, i, i - 1, n);
    if (y > 0) {
        const bool su = (int)vb[i - W] == v;
        const bool sul = x > 0 && (int)vb[i - W - 1] == v, sur = x + 1 < W && (int)vb[i - W + 1] == v;
        if (up && su && !(sl && sul)) reg_union(pb, i, i - W, n);
        if (!su) {
            if (upl && sul) reg_union(pb, i, i - W - 1, n);
            if (upr && sur) reg_union(pb, i, i - W + 1, n);
        }
    }
}

__global__ __launch_bounds__(256) void region_flatten_kernel(const int* parent, int B, int n, int* root) {
    const long total = (long)B * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / n;
        const int* pb = parent + b * n;
        int i = (int)(idx - b * n);
        int r = -1;
        if (pb[i] >= 0) {
            for (int t = 0; t < n; ++t) {
                const int p = pb[i];
                if (p == i || p < 0 || p >= n) break;
                i = p;
            }
            r = i;
        }
        root[idx] = r;
    }
}

// ---- compaction: id = the rank of the region's root among the image's roots ----
__device__ __forceinline__ int reg_block_sum(int v, int* s_wave) {    // the sum over the 256 threads, for all of them
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ __launch_bounds__(256) void region_flags_kernel(const int* root, int n, int nblk, int* partial) {
    __shared__ int s_wave[4];
    const int blk = blockIdx.x, b = blockIdx.y;
    const int* rb = root + (long)b * n;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = blk * REG_BLOCK + threadIdx.x * 4 + k;
        c += p < n && rb[p] == p;
    }
    c = reg_block_sum(c, s_wave);
    if (threadIdx.x == 0) partial[(long)b * nblk + blk] = c;
}

__global__ __launch_bounds__(256) void region_scan_kernel(int* partial, int nblk, int* count) {
    __shared__ int s_sum[256];
    const int b = blockIdx.x, t = threadIdx.x;
    int* pb = partial + (long)b * nblk;
    const int per = (nblk + 255) / 256;                     // consecutive partials of one thread
    const int lo = t * per < nblk ? t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += pb[i];
    s_sum[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                     // inclusive scan over the threads
        const int o = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += o;
        __syncthreads();
    }
    int run = s_sum[t] - s;                                 // exclusive
    for (int i = lo; i < hi; ++i) {
        const int v = pb[i];
        pb[i] = run;
        run += v;
    }
    if (t == 255) count[b] = s_sum[255];
}

__global__ __launch_bounds__(256) void region_rank_kernel(const int* root, const int* partial, int n, int nblk, int* id) {
    __shared__ int s_wave[4];
    const int blk = blockIdx.x, b = blockIdx.y;
    const int* rb = root + (long)b * n;
    int* ib = id + (long)b * n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = blk * REG_BLOCK + threadIdx.x * 4;
    bool f[4];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = p0 + k < n && rb[p0 + k] == p0 + k, c += f[k];
    int inc = c;                                            // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int at = partial[(long)b * nblk + blk] + inc - c;
    for (int w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (f[k]) ib[p0 + k] = at++;
}

__global__ __launch_bounds__(256) void region_gather_kernel(const int* root, int B, int n, int* id) {
    const long total = (long)B * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / n;
        const int p = (int)(idx - b * n), r = root[idx];
        if (r == p) continue;                               // a root: the rank launch wrote it, and this launch reads it
        int v = -1;
        if (r >= 0 && r < n && root[b * n + r] == r) v = id[b * n + r];
        id[idx] = v;
    }
}

// ---- runs of equal keys among the 64 consecutive pixels of a wave ----
struct RegRun {
    bool head;                                              // this lane opens a run
    int end;                                                // the lane after the run's last
};

__device__ __forceinline__ RegRun reg_run(int key, int lane) {
    const int prev = __shfl_up(key, 1, 64);
    RegRun r;
    r.head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(r.head);
    const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
    r.end = later ? lane + 1 + __builtin_ctzll(later) : 64;
    return r;
}

// A giant region would take every run's atomic at ONE address.  The workgroup first gathers its runs in a small direct-mapped table in LDS
// (a slot belongs to the first root that claims it; a root that finds its slot taken by another adds to global memory itself), then adds
// every slot once: one global atomic per root and 256 pixels instead of one per run.  Integer sums: the result does not depend on who won.
constexpr int REG_SLOTS = 64;

__global__ __launch_bounds__(256) void region_areas_kernel(const int* root, int B, int n, int* area) {
    __shared__ int s_key[REG_SLOTS], s_cnt[REG_SLOTS];
    const long per = ((long)n + 255) / 256;                 // workgroups per image: a workgroup never straddles two images
    const int lane = threadIdx.x & 63;
    for (long blk = blockIdx.x; blk < per * B; blk += gridDim.x) {         // (uniform over the workgroup: the barriers are safe)
        if (threadIdx.x < REG_SLOTS) s_key[threadIdx.x] = -1, s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const long b = blk / per, i = (blk - b * per) * 256 + threadIdx.x;
        int r = i < n ? root[b * n + i] : -1;
        if (r < 0 || r >= n) r = -1;
        const RegRun run = reg_run(r, lane);
        if (run.head && r >= 0) {
            const int slot = (r ^ (r >> 6) ^ (r >> 12)) & (REG_SLOTS - 1);
            const int old = atomicCAS(s_key + slot, -1, r);
            if (old == -1 || old == r) atomicAdd(s_cnt + slot, run.end - lane);
            else atomicAdd(area + b * n + r, run.end - lane);
        }
        __syncthreads();
        if (threadIdx.x < REG_SLOTS && s_key[threadIdx.x] >= 0) atomicAdd(area + b * n + s_key[threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();                                    // before the next round clears the table
    }
}

struct TableArgs {
    const void* values;
    int value_bytes;                                        // 1 (u8) or 4 (i32)
    const int* root;
    const int* id;
    int B, H, W, capacity;
    int* table;                                             // [B][capacity][8]
    unsigned long long* moments;                            // [B][capacity][2]
};

__global__ __launch_bounds__(256) void region_table_init_kernel(const TableArgs a) {
    const int n = a.H * a.W;
    const long total = (long)a.B * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / n;
        const int p = (int)(idx - b * n);
        if (a.root[idx] != p) continue;
        const int l = a.id[idx];
        if (l < 0 || l >= a.capacity) continue;
        const int y = p / a.W, x = p - y * a.W;
        int* row = a.table + (b * a.capacity + l) * 8;
        row[0] = a.value_bytes == 1 ? (int)static_cast<const uint8_t*>(a.values)[idx] : static_cast<const int*>(a.values)[idx];
        row[2] = y, row[3] = x, row[4] = y, row[5] = x, row[6] = p;       // the root's row IS ymin; the others are bounds the fold tightens
    }
}

__device__ __forceinline__ void reg_table_add(const TableArgs& a, long b, int l, int cnt, int xmin, int ymax, int xmax, int sy, int sx) {
    int* row = a.table + (b * a.capacity + l) * 8;
    atomicAdd(row + 1, cnt);
    atomicMin(row + 3, xmin);
    atomicMax(row + 4, ymax);
    atomicMax(row + 5, xmax);
    unsigned long long* m = a.moments + (b * a.capacity + l) * 2;
    atomicAdd(m, (unsigned long long)sy);
    atomicAdd(m + 1, (unsigned long long)sx);
}

// The runs of a workgroup's 256 pixels are gathered per id in the direct-mapped LDS table of region_areas_kernel first (six fields per
// slot; y and x sums of 256 pixels fit an int), so a giant region takes one set of global atomics per 256 pixels, not one per run.
__global__ __launch_bounds__(256) void region_table_fold_kernel(const TableArgs a) {
    __shared__ int s_key[REG_SLOTS], s_cnt[REG_SLOTS], s_xmin[REG_SLOTS], s_ymax[REG_SLOTS], s_xmax[REG_SLOTS], s_sy[REG_SLOTS], s_sx[REG_SLOTS];
    const int n = a.H * a.W;
    const long per = ((long)n + 255) / 256;
    const int lane = threadIdx.x & 63, t = threadIdx.x;
    for (long blk = blockIdx.x; blk < per * a.B; blk += gridDim.x) {       // (uniform over the workgroup: the barriers are safe)
        if (t < REG_SLOTS) s_key[t] = -1, s_cnt[t] = 0, s_xmin[t] = 0x7fffffff, s_ymax[t] = -1, s_xmax[t] = -1, s_sy[t] = 0, s_sx[t] = 0;
        __syncthreads();
        const long b = blk / per, i = (blk - b * per) * 256 + t;
        int l = -1;
        if (i < n) {
            const int r = a.root[b * n + i];
            l = a.id[b * n + i];
            if (r < 0 || r >= n || l < 0 || l >= a.capacity) l = -1;
        }
        const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
        const RegRun run = reg_run(l, lane);
        int sy = y, sx = x, xmin = x, xmax = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int oy = __shfl_down(sy, d, 64), ox = __shfl_down(sx, d, 64);
            const int omin = __shfl_down(xmin, d, 64), omax = __shfl_down(xmax, d, 64);
            if (lane + d < run.end) {
                sy += oy, sx += ox;
                xmin = omin < xmin ? omin : xmin, xmax = omax > xmax ? omax : xmax;
            }
        }
        const int ymax = __shfl(y, run.end - 1, 64);        // rows rise along a run
        if (run.head && l >= 0) {
            const int slot = (l ^ (l >> 6)) & (REG_SLOTS - 1);
            const int old = atomicCAS(s_key + slot, -1, l);
            if (old == -1 || old == l) {
                atomicAdd(s_cnt + slot, run.end - lane);
                atomicMin(s_xmin + slot, xmin);
                atomicMax(s_ymax + slot, ymax);
                atomicMax(s_xmax + slot, xmax);
                atomicAdd(s_sy + slot, sy);
                atomicAdd(s_sx + slot, sx);
            } else {
                reg_table_add(a, b, l, run.end - lane, xmin, ymax, xmax, sy, sx);
            }
        }
        __syncthreads();
        if (t < REG_SLOTS && s_key[t] >= 0) reg_table_add(a, b, s_key[t], s_cnt[t], s_xmin[t], s_ymax[t], s_xmax[t], s_sy[t], s_sx[t]);
        __syncthreads();                                    // before the next round clears the table
    }
}

template <typename T>
__global__ __launch_bounds__(256) void region_filter_kernel(const T* values, const int* root, const int* area, int B, int H, int W,
                                                            int min_area, int neighbour, int fill, T* out) {
    const int n = H * W;
    const long total = (long)B * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / n;
        const int r = root[idx];
        T v = values[idx];
        if (r >= 0 && r < n && area[b * n + r] < min_area) {
            if (!neighbour) {
                v = (T)fill;
            } else {
                const int ry = r / W, rx = r - ry * W;
                if (rx > 0) v = values[b * n + r - 1];
                else if (ry > 0) v = values[b * n + r - W];
            }
        }
        out[idx] = v;
    }
}

static int region_fail(const char* who, const char* what) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return vqseg_set_error(VQSEG_EINVAL, buf);
}

static int region_hip(const char* who, hipError_t e) {
    if (e == hipSuccess) return 0;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, hipGetErrorString(e));
    return vqseg_set_error((int)e, buf);
}

static int region_done(const char* who) { return region_hip(who, hipGetLastError()); }

static const char* region_size_error(int b, int h, int w) {
    if (b < 1 || h < 1 || w < 1) return "b, h and w must be positive";
    if (b > 65535) return "at most 65535 images per launch";
    if (h > REG_MAX_SIDE || w > REG_MAX_SIDE) return "a side above 4096";
    return nullptr;
}

static unsigned region_blocks(int64_t elems) {
    const int64_t blocks = (elems + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

template <typename T>
static int region_roots(const char* who, const T* values, int b, int h, int w, int connectivity, int n_ignore, const int* ignore,
                        int32_t* parent, int32_t* root, void* stream) {
    if (!values || !parent || !root) return region_fail(who, "null values, parent or root");
    if (parent == root) return region_fail(who, "parent and root must be two buffers");
    if (const char* e = region_size_error(b, h, w)) return region_fail(who, e);
    if (connectivity != 4 && connectivity != 8) return region_fail(who, "connectivity must be 4 or 8");
    if (n_ignore < 0 || n_ignore > 4) return region_fail(who, "0 to 4 ignored values");
    RegionMap q = {b, h, w, connectivity, n_ignore, {ignore[0], ignore[1], ignore[2], ignore[3]}};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((w + REG_TX - 1) / REG_TX), (unsigned)((h + REG_TY - 1) / REG_TY), (unsigned)b);
    hipLaunchKernelGGL(region_local_kernel<T>, grid, dim3(256), 0, st, values, q, parent);
    if (grid.x > 1 || grid.y > 1) hipLaunchKernelGGL(region_merge_kernel<T>, grid, dim3(128), 0, st, values, q, parent);
    hipLaunchKernelGGL(region_flatten_kernel, dim3(region_blocks((int64_t)b * h * w)), dim3(256), 0, st, parent, b, h * w, root);
    return region_done(who);
}

template <typename T>
static int region_filter(const char* who, const T* values, const int32_t* root, const int32_t* area, int b, int h, int w, int min_area,
                         int neighbour, int fill, T* out, void* stream) {
    if (!values || !root || !area || !out) return region_fail(who, "null values, root, area or out");
    if (values == out) return region_fail(who, "out of place only: the fill is read from the input");
    if (const char* e = region_size_error(b, h, w)) return region_fail(who, e);
    if (neighbour != 0 && neighbour != 1) return region_fail(who, "neighbour is 0 (the constant fill) or 1");
    hipLaunchKernelGGL(region_filter_kernel<T>, dim3(region_blocks((int64_t)b * h * w)), dim3(256), 0, static_cast<hipStream_t>(stream), values,
                       root, area, b, h, w, min_area, neighbour, fill, out);
    return region_done(who);
}

}  // namespace vqseg

extern "C" {

int vqseg_region_roots_u8(const uint8_t* values, int b, int h, int w, int connectivity, int n_ignore, int ignore0, int ignore1, int ignore2,
                          int ignore3, int32_t* parent, int32_t* root, void* stream) {
    const int ignore[4] = {ignore0, ignore1, ignore2, ignore3};
    return vqseg::region_roots<uint8_t>("region_roots_u8", values, b, h, w, connectivity, n_ignore, ignore, parent, root, stream);
}

int vqseg_region_roots_i32(const int32_t* values, int b, int h, int w, int connectivity, int n_ignore, int ignore0, int ignore1, int ignore2,
                           int ignore3, int32_t* parent, int32_t* root, void* stream) {
    const int ignore[4] = {ignore0, ignore1, ignore2, ignore3};
    return vqseg::region_roots<int32_t>("region_roots_i32", values, b, h, w, connectivity, n_ignore, ignore, parent, root, stream);
}

int64_t vqseg_region_ids_partials(int h, int w) {
    using namespace vqseg;
    if (h < 1 || w < 1 || h > REG_MAX_SIDE || w > REG_MAX_SIDE) return 0;
    return ((int64_t)h * w + REG_BLOCK - 1) / REG_BLOCK;
}

int vqseg_region_ids_i32(const int32_t* root, int b, int h, int w, int32_t* partial, int32_t* id, int32_t* count, void* stream) {
    using namespace vqseg;
    if (!root || !partial || !id || !count) return region_fail("region_ids", "null root, partial, id or count");
    if (root == id) return region_fail("region_ids", "root and id must be two buffers");
    if (const char* e = region_size_error(b, h, w)) return region_fail("region_ids", e);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = h * w, nblk = (int)vqseg_region_ids_partials(h, w);
    const dim3 grid((unsigned)nblk, (unsigned)b);
    hipLaunchKernelGGL(region_flags_kernel, grid, dim3(256), 0, st, root, n, nblk, partial);
    hipLaunchKernelGGL(region_scan_kernel, dim3((unsigned)b), dim3(256), 0, st, partial, nblk, count);
    hipLaunchKernelGGL(region_rank_kernel, grid, dim3(256), 0, st, root, partial, n, nblk, id);
    hipLaunchKernelGGL(region_gather_kernel, dim3(region_blocks((int64_t)b * n)), dim3(256), 0, st, root, b, n, id);
    return region_done("region_ids");
}

int vqseg_region_table_i32(const void* values, int value_bytes, const int32_t* root, const int32_t* id, int b, int h, int w, int capacity,
                           int32_t* table, int64_t* moments, void* stream) {
    using namespace vqseg;
    if (!values || !root || !id || !table || !moments) return region_fail("region_table", "null values, root, id, table or moments");
    if (value_bytes != 1 && value_bytes != 4) return region_fail("region_table", "value_bytes is 1 (u8) or 4 (i32)");
    if (const char* e = region_size_error(b, h, w)) return region_fail("region_table", e);
    if (capacity < 1 || (int64_t)b * capacity > (int64_t)1 << 26) return region_fail("region_table", "capacity must be positive and b * capacity at most 2^26");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = region_hip("region_table memset", hipMemsetAsync(table, 0, sizeof(int32_t) * 8 * (size_t)b * capacity, st))) return rc;
    if (const int rc = region_hip("region_table memset", hipMemsetAsync(moments, 0, sizeof(int64_t) * 2 * (size_t)b * capacity, st))) return rc;
    TableArgs a = {values, value_bytes, root, id, b, h, w, capacity, table, reinterpret_cast<unsigned long long*>(moments)};
    const int64_t n = (int64_t)h * w;
    hipLaunchKernelGGL(region_table_init_kernel, dim3(region_blocks(b * n)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(region_table_fold_kernel, dim3(region_blocks((n + 255) / 256 * 256 * b)), dim3(256), 0, st, a);
    return region_done("region_table");
}

int vqseg_region_areas_i32(const int32_t* root, int b, int h, int w, int32_t* area, void* stream) {
    using namespace vqseg;
    if (!root || !area) return region_fail("region_areas", "null root or area");
    if (const char* e = region_size_error(b, h, w)) return region_fail("region_areas", e);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)h * w;
    if (const int rc = region_hip("region_areas memset", hipMemsetAsync(area, 0, sizeof(int32_t) * (size_t)b * n, st))) return rc;
    hipLaunchKernelGGL(region_areas_kernel, dim3(region_blocks((n + 255) / 256 * 256 * b)), dim3(256), 0, st, root, b, (int)n, area);
    return region_done("region_areas");
}

int vqseg_region_filter_u8(const uint8_t* values, const int32_t* root, const int32_t* area, int b, int h, int w, int min_area, int neighbour,
                           int fill, uint8_t* out, void* stream) {
    if (fill < 0 || fill > 255) return vqseg::region_fail("region_filter_u8", "fill must lie in 0..255");
    return vqseg::region_filter<uint8_t>("region_filter_u8", values, root, area, b, h, w, min_area, neighbour, fill, out, stream);
}

int vqseg_region_filter_i32(const int32_t* values, const int32_t* root, const int32_t* area, int b, int h, int w, int min_area, int neighbour,
                            int fill, int32_t* out, void* stream) {
    return vqseg::region_filter<int32_t>("region_filter_i32", values, root, area, b, h, w, min_area, neighbour, fill, out, stream);
}

}  // extern "C"
