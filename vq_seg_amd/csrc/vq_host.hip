// vq_host.hip -- the host side of the vector quantiser, no kernels: workspace plans, the option table, event profiling, the
// tiles-per-wave rule and the grouped launch that wires the kernel units (vq_assign / vq_filter / vq_tail / vq_codebook) together.
// Called by the C ABI in vqseg_abi.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "options.h"
#include "vq_internal.h"

namespace vqseg {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the candidate filter serves bf16 rows of layers with whole 256-code chunks and 32-channel stages
static bool filter_shape_ok(int C, int K) { return K % 256 == 0 && C % 32 == 0 && K <= 65536; }

PreparedLayout prepared_layout(int C, int K) {
    const int Kp = round_up(K, 32);
    PreparedLayout l;
    l.off_e4 = 0;
    l.off_enorm = (size_t)C * Kp * sizeof(float);               // (kept adjacent to E4: the exact kernel's blob of rounds 1-3)
    l.off_enmax = up256(l.off_enorm + (size_t)Kp * sizeof(float));
    l.off_eb = l.off_enmax + 256;
    l.bytes = filter_shape_ok(C, K) ? up256(l.off_eb + (size_t)2 * C * Kp * sizeof(unsigned short)) : l.off_eb;
    return l;
}

PreparedView prepared_view(const void* prepared, int C, int K) {
    const PreparedLayout l = prepared_layout(C, K);
    char* base = const_cast<char*>(static_cast<const char*>(prepared));
    return {reinterpret_cast<float*>(base + l.off_e4), reinterpret_cast<float*>(base + l.off_enorm),
            reinterpret_cast<float*>(base + l.off_enmax), reinterpret_cast<unsigned short*>(base + l.off_eb)};
}

size_t prepared_bytes(int C, int K) { return prepared_layout(C, K).bytes; }

static int g_vq_max_tiles = 8;                              // cap on T (option "vq_max_tiles_per_wave": 8, 4, 2 or 1)
static int g_vq_fine_split = 1;                             // option "vq_fine_split": 0 = r3's choice of T (see vq_group_tiles)
static int g_vq_bf16_filter = 1;                            // bf16 rows: candidate filter + exact re-score (0: the exact kernel on every row)
static int g_vq_filter_force_all = 0;                       // tests: 1 = every row is re-scored by the exact kernel (the filter decides nothing)
static int g_vq_filter_launches = 0;                        // launches that took the filter path (tests read and reset it)
static int g_vq_s3_filter = 1;                              // split-3 rows: the same filter on [hi | lo] (0: the exact kernel, merging on load)
static const Option VQ_OPTIONS[] = {
    {"vq_max_tiles_per_wave", &g_vq_max_tiles, OPT_POW2_FAIL, 1, 8},
    {"vq_fine_split", &g_vq_fine_split, OPT_FLAG},
    {"vq_bf16_filter", &g_vq_bf16_filter, OPT_FLAG},
    {"vq_filter_force_all", &g_vq_filter_force_all, OPT_FLAG},
    {"vq_filter_launches", &g_vq_filter_launches},
    {"vq_s3_filter", &g_vq_s3_filter, OPT_FLAG},
};

int vq_set_option(const char* key, int value) { return apply_option(VQ_OPTIONS, key, value); }

VqPlan vq_plan(int64_t N, int C, int K) {
    VqPlan p;
    p.Cp = C;
    p.Kp = round_up(K, 32);
    size_t off = 0;
    p.off_prepared = off;
    off += prepared_bytes(C, K);
    p.off_keys = off;
    off += up256((size_t)N * sizeof(unsigned long long));
    p.off_hist = off;
    off += up256((size_t)p.Kp * sizeof(int));
    p.off_partial = off;
    off += (size_t)GATHER_BLOCKS_MAX * sizeof(float);
    off = up256(off);
    p.off_summary = p.off_brow = p.off_amb = p.off_pair_rc = off;
    p.pair_cap = 0;
    if (filter_shape_ok(C, K)) {
        p.off_summary = off;
        off += up256((size_t)N * (p.Kp / F_SUB) * sizeof(unsigned long long));
        p.off_brow = off;
        off += up256((size_t)N * sizeof(float));
        p.off_amb = off;                                        // the pair sub-lists' counters [F_LISTS] + the overflow flag
        off += 512;
        const long total_cap = 4 * N < (1L << 30) ? 4 * N : (1L << 30);
        p.pair_cap = (int)((total_cap + F_LISTS - 1) / F_LISTS);     // per sub-list: four candidates per row on average
        if (p.pair_cap < 1024) p.pair_cap = 1024;
        p.off_pair_rc = off;
        off += up256((size_t)p.pair_cap * F_LISTS * sizeof(unsigned long long));
    }
    p.bytes = up256(off);
    long blocks = (N + GATHER_ROWS_PER_BLOCK - 1) / GATHER_ROWS_PER_BLOCK;
    p.gather_blocks = (int)(blocks < GATHER_BLOCKS_MAX ? (blocks > 0 ? blocks : 1) : GATHER_BLOCKS_MAX);
    // tiles per wave: see vq_group_tiles
    const int k1 = K;
    p.T = vq_group_tiles(1, &N, &k1);
    return p;
}

hipError_t launch_prepare(const float* W, int K, int C, void* prepared, hipStream_t st) {
    const int Kp = round_up(K, 32);
    const PreparedView pv = prepared_view(prepared, C, K);
    launch_prepare_exact(W, K, C, Kp, pv.E4, pv.enorm, st);
    if (filter_shape_ok(C, K)) launch_prepare_filter(W, K, C, Kp, pv.enorm, pv.Eb, pv.en_max, st);   // the candidate filter's image of the same codebook
    return hipGetLastError();
}

// ---- optional per-launch timing of the assign kernel (bench.py's roofline leg): event pairs on the launch stream
struct ProfShape {
    int64_t n;
    int c, k;
    int slot, group;            // first record of the launch this level ran in (its event pair), number of levels in that launch
    int kind;                   // 0: exact fp32 MFMA kernel on f32 rows (or split-3 rows merged on load), 1: on bf16 rows, 2: bf16 candidate
                                // filter + exact re-score (bf16 or split-3 rows)
};
struct Profile {
    bool enabled = false;
    int capacity = 0;
    std::vector<hipEvent_t> ev;
    std::vector<ProfShape> shape;
};
static Profile g_prof;

hipError_t profile_begin(int capacity) {
    profile_release();
    g_prof.ev.resize((size_t)capacity * 2);
    for (auto& e : g_prof.ev) {
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
    }
    g_prof.shape.clear();
    g_prof.capacity = capacity;
    g_prof.enabled = true;
    return hipSuccess;
}

void profile_release() {
    for (auto& e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear();
    g_prof.shape.clear();
    g_prof.enabled = false;
    g_prof.capacity = 0;
}

int profile_collect(int max_records, int64_t* n, int* c, int* k, float* ms, int* kind) {
    g_prof.enabled = false;
    const int cnt = (int)g_prof.shape.size();
    int out = 0;
    for (int i = 0; i < cnt && out < max_records; ++i) {
        const ProfShape& sh = g_prof.shape[i];
        if (hipEventSynchronize(g_prof.ev[2 * sh.slot + 1]) != hipSuccess) break;
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof.ev[2 * sh.slot], g_prof.ev[2 * sh.slot + 1]) != hipSuccess) break;
        double mine = 2.0 * (double)sh.n * sh.c * sh.k, all = 0.0;   // a grouped launch: this level's share of the flops
        for (int j = sh.slot; j < sh.slot + sh.group && j < cnt; ++j) all += 2.0 * (double)g_prof.shape[j].n * g_prof.shape[j].c * g_prof.shape[j].k;
        n[out] = sh.n;
        c[out] = sh.c;
        k[out] = sh.k;
        ms[out] = (float)(t * (all > 0 ? mine / all : 1.0));
        if (kind) kind[out] = sh.kind;
        ++out;
    }
    profile_release();
    return out;
}


static unsigned assign_workgroups(int64_t N, int Kp, int T) {
    const long row_tiles = (N + ROWS_PER_WG - 1) / ROWS_PER_WG;
    return (unsigned)((row_tiles + 7) / 8 * 8 * (Kp / (32 * T)));               // see the id mapping in the kernel (vq_assign.hip)
}

// tiles per wave for a group of levels.  r4: first the largest T in {8,4} that divides every level's tile count and gives the launch
// >= VQ_FINE_WGS workgroups -- the workgroups of a launch differ 4x in length between the levels, and with fewer, longer ones the
// last round leaves the chip half empty (K = 512 on 172 k rows: T = 8 -> 2688 workgroups, 0.76 of the fp32 MFMA peak; T = 4 -> 5376,
// 0.81; K = 256 / K = 1024 / twice the rows: T = 8 stays best, T = 2 loses 9 % of the per-wave rate: LEDGER r4).  Else, as before, the
// largest T in {8,4,2,1} that still yields >= 2 workgroups per CU over the whole launch; if none does, the smallest.
constexpr long VQ_FINE_WGS = 4096;
static long vq_group_wgs(int n, const int64_t* N, const int* K, int t) {     // workgroups of the launch at T = t; -1: t does not divide
    long wgs = 0;
    for (int i = 0; i < n; ++i) {
        const int tiles = round_up(K[i], 32) / 32;
        if (tiles % t) return -1;
        wgs += ((N[i] + ROWS_PER_WG - 1) / ROWS_PER_WG) * (tiles / t);
    }
    return wgs;
}
int vq_group_tiles(int n, const int64_t* N, const int* K) {
    if (g_vq_fine_split)
        for (int t = g_vq_max_tiles; t >= 4; t >>= 1)
            if (vq_group_wgs(n, N, K, t) >= VQ_FINE_WGS) return t;
    for (int t = g_vq_max_tiles; t >= 1; t >>= 1) {
        const long wgs = vq_group_wgs(n, N, K, t);
        if (wgs >= 0 && (wgs >= 512 || t == 1)) return t;
    }
    return 1;
}

// the distance + argmin pass of n <= VQ_MAX_LEVELS levels in ONE launch (keys pre-set, unpack per level afterwards)
hipError_t launch_assign_group(int n, const void* const* x, int x_bf16, const int64_t* N, const int* C, const int* K,
                               const void* const* prepared, const VqPlan* plans, char* const* ws, int64_t* const* idx,
                               float* const* dmin, int T, hipStream_t st, const float* const* codebooks) {
    if (n < 1 || n > VQ_MAX_LEVELS) return hipErrorInvalidValue;
    int order[VQ_MAX_LEVELS];
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 0; i < n; ++i)                                  // longest workgroups (most channels) first
        for (int j = i + 1; j < n; ++j)
            if (C[order[j]] > C[order[i]]) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    // bf16 and split-3 rows of layers with whole 256-code chunks take the candidate filter: bf16 MFMA scores -> per-row decision -> the
    // exact kernel (indirect mode) on the rows the filter left open.  Same keys as the exact kernel on every row.
    bool filter = x_bf16 == VQ_ROWS_S3 ? g_vq_s3_filter != 0 : (x_bf16 && g_vq_bf16_filter);
    for (int i = 0; i < n; ++i) filter = filter && filter_shape_ok(C[i], K[i]);
    VqLevel lv[VQ_MAX_LEVELS];
    VqFilterGroup fg;
    fg.n = n;
    unsigned end = 0, fend = 0, rend = 0, send = 0, iend = 0;
    VqInitGroup ig;
    ig.n = n;
    for (int q = 0; q < n; ++q) {
        const int i = order[q];
        const PreparedView pv = prepared_view(prepared[i], C[i], K[i]);
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws[i] + plans[i].off_keys);
        {
            long ib = (N[i] + 4095) / 4096;                      // 16 keys per thread
            ib = ib < 1 ? 1 : (ib > 256 ? 256 : ib);
            iend += (unsigned)ib;
            ig.lv[q] = VqInitLevel{keys, (long)N[i], nullptr, reinterpret_cast<int*>(ws[i] + plans[i].off_hist), plans[i].Kp, iend};
        }
        end += assign_workgroups(N[i], plans[i].Kp, T);
        lv[q] = VqLevel{x[i], pv.E4, pv.enorm, keys, (long)N[i], C[i], plans[i].Kp, end};
        lv[q].K = K[i];
        if (filter) {
            int* amb = reinterpret_cast<int*>(ws[i] + plans[i].off_amb);
            ig.lv[q].amb = amb;                                   // the sub-lists' counters and the overflow flag: zeroed by the init launch
            // a pair list that overflows (more than four candidates per row on average: degenerate codebooks) switches the level to the
            // exact kernel on every row -- the gated launch below
            lv[q].gate = amb + F_LISTS;                           // the overflow flag
            lv[q].gate_cap = 0;
            const long row_tiles = (N[i] + F_ROWS - 1) / F_ROWS;
            fend += (unsigned)((row_tiles + 7) / 8 * 8 * (plans[i].Kp / F_CODES));
            rend += (unsigned)((N[i] + 255) / 256);
            {   // stage 3: a thread per expected pair (about one per row at most), whole multiples of F_LISTS workgroups, 4 .. 16 per sub-list
                long per = (N[i] / 256 + F_LISTS - 1) / F_LISTS;
                if (per < 4) per = 4;
                if (per > 16) per = 16;
                send += (unsigned)(per * F_LISTS);
            }
            fg.lv[q] = VqFilterLevel{x[i], pv.Eb, pv.enorm, pv.en_max,
                                     reinterpret_cast<unsigned long long*>(ws[i] + plans[i].off_summary),
                                     reinterpret_cast<float*>(ws[i] + plans[i].off_brow),
                                     reinterpret_cast<unsigned long long*>(ws[i] + plans[i].off_pair_rc), amb, plans[i].pair_cap, keys,
                                     codebooks ? codebooks[i] : nullptr, pv.E4, (long)N[i], C[i], plans[i].Kp, fend, rend, send};
        }
    }
    launch_group_init(ig, st);
    const bool rec = g_prof.enabled && (int)g_prof.shape.size() + n <= g_prof.capacity;
    const size_t slot = g_prof.shape.size();
    if (rec) {
        // one event pair for the launch; its time is apportioned to the levels by their flops (2 N K C) when collected
        for (int i = 0; i < n; ++i) g_prof.shape.push_back({N[i], C[i], K[i], (int)slot, n, filter ? 2 : (x_bf16 == VQ_ROWS_BF16 ? 1 : 0)});
        (void)hipEventRecord(g_prof.ev[2 * slot], st);
    }
    if (filter) {
        ++g_vq_filter_launches;
        launch_filter(fg, x_bf16, g_vq_filter_force_all, st);
    }
    launch_assign_levels(lv, n, T, x_bf16, st);
    if (rec) (void)hipEventRecord(g_prof.ev[2 * slot + 1], st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int i = 0; i < n; ++i) {
        launch_unpack_level(i, N, K, plans, ws, idx, dmin, st);
        if (filter && dmin && dmin[i]) {
            // rows the filter decided carry no exact distance: recompute the winner's on the vector ALU, in the exact kernel's order
            const PreparedView pv = prepared_view(prepared[i], C[i], K[i]);
            launch_exact_dist(x[i], x_bf16, pv.E4, plans[i].Kp, pv.enorm, idx[i], N[i], C[i], dmin[i], st);
        }
    }
    return hipGetLastError();
}

hipError_t launch_assign(const void* x, int x_bf16, int64_t N, int C, int K, const void* prepared, const VqPlan& p, char* ws,
                         int64_t* idx, float* dmin, hipStream_t st, const float* codebook) {
    return launch_assign_group(1, &x, x_bf16, &N, &C, &K, &prepared, &p, &ws, &idx, &dmin, p.T, st, codebook ? &codebook : nullptr);
}

KmPlan km_plan(int64_t N, int C, int K) {
    KmPlan p;
    p.vq = vq_plan(N, C, K);
    size_t off = p.vq.bytes;
    p.off_idx = off;
    off += (size_t)N * sizeof(int64_t);
    p.off_counts = off;
    off += (size_t)round_up(K + 1, 64) * sizeof(int);
    p.off_offsets = off;
    off += (size_t)round_up(K + 1, 64) * sizeof(int);
    p.off_members = off;
    off += (size_t)N * sizeof(int);
    p.off_sums = off;
    off += (size_t)K * C * sizeof(float);
    p.off_counts64 = off;
    off += (size_t)round_up(K, 32) * sizeof(int64_t);
    p.row_blocks = (int)((N + KM_RB - 1) / KM_RB);
    p.max_segments = (int)(N / KM_SEG + K);
    p.off_hist = off;
    off += (size_t)round_up(p.row_blocks * K, 64) * sizeof(int);
    p.off_segoff = off;
    off += (size_t)round_up(K + 1, 64) * sizeof(int);
    p.off_partial = off;
    off += (size_t)p.max_segments * C * sizeof(float);
    p.bytes = up256(off);
    return p;
}

hipError_t launch_km_accumulate(const float* samples, const float* means, int64_t N, int C, int K, const KmPlan& p,
                                char* ws, float* sums, int64_t* counts64, hipStream_t st) {
    hipError_t e = launch_prepare(means, K, C, ws + p.vq.off_prepared, st);
    if (e != hipSuccess) return e;
    int64_t* idx = reinterpret_cast<int64_t*>(ws + p.off_idx);
    e = launch_assign(samples, 0, N, C, K, ws + p.vq.off_prepared, p.vq, ws, idx, nullptr, st);
    if (e != hipSuccess) return e;
    return launch_code_sums(samples, 0, idx, N, C, K, p, ws, sums, counts64, st);
}

}  // namespace vqseg
