#include <algorithm>
#include <cmath>
// psh_capi.hip -- the C ABI declared in include/psh.h: argument checking, workspace
// carving, launch planning.  Everything is enqueued on the caller's stream; no
// allocation, no global state (a thread-local string holds the last HIP error text).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "psh.h"
#include "psh_kernels.h"

using namespace psh;

namespace {

thread_local char g_hip_err[256] = "";

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            snprintf(g_hip_err, sizeof(g_hip_err), "%s -> %s (%s:%d)", #expr,                \
                     hipGetErrorString(e__), __FILE__, __LINE__);                            \
            return PSH_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

struct DeviceGuard {   // launch on the caller's device, restore the previous one
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != device && hipSetDevice(device) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// every entry point that launches: the rest of its body runs on `device`
#define GUARD_DEVICE(device)                                                                 \
    DeviceGuard g(device);                                                                   \
    if (!g.ok) { snprintf(g_hip_err, sizeof(g_hip_err), "hipSetDevice(%d) failed", device); return PSH_ERR_HIP; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int next_pow2(int x) { int p = 2; while (p < x) p <<= 1; return p; }
inline int tile_floats_for(int W) {
    const int logical = PSH_SEG + W + 32;               // SEG + W - 1 used, slack for the sliding refills
    return (logical + ((logical >> 6) << 2) + 8 + 3) & ~3;
}
// the matrix-core scans read the fp32 tile only window by window (no sliding refills past the segment): SEG + W - 1 values
// rounded up to whole float4 stores, padded layout
inline int mx_tile_floats(int W) {
    const int logical = PSH_SEG + W + 3;
    return (logical + ((logical >> 6) << 2) + 4 + 3) & ~3;
}
inline int64_t seg_count(int64_t Tp) { return (Tp + PSH_SEG - 1) / PSH_SEG; }     // wave-segments of PSH_SEG windows per row
// a grid over `units` of work, `per_block` to a block: at most `resident` blocks (one round on the compute units), at most
// `max_blocks` (the candidate slices: PSH_MAX_BLOCKS), at least one
inline int64_t per_cu_grid(int64_t units, int per_block, int64_t resident, int64_t max_blocks = INT64_MAX) {
    int64_t g = (units + per_block - 1) / per_block;
    if (g > resident) g = resident;
    if (g > max_blocks) g = max_blocks;
    return g < 1 ? 1 : g;
}
// rows_kernel (one-window rows, a row per lane): 128 rows per block, up to eight blocks per compute unit
inline int64_t rows_grid(int64_t n_rows, int ncu, int64_t max_blocks = INT64_MAX) { return per_cu_grid(n_rows, 128, 8 * (int64_t)ncu, max_blocks); }

struct Workspace {
    FusedHdr* fused;      // state of the fused single-launch scan: ALWAYS the first PSH_FUSED_BYTES of the workspace
    EmbedPlan* eplan;     // embedded scan: what embed_plan_kernel found in the kernel matrix (PSH_PLAN_BYTES)
    QueryState* qstate;
    int* total;
    float* minbuf;
    int64_t min_stride;
    int* bcount;
    int* bcount2;         // PSH_MAX_BLOCKS ints: second-class counts of the single-query matrix-core scan
    float* blockmax;      // PSH_MAX_BLOCKS floats: per-block max |y| of the bootstrap scan
    void* mq_frag;        // (B rounded up to 4) x 256 f16: B fragments of the batched matrix-core scan
    int2* sel_rt;
    float* cand_d;
    int2* cand_rt;
    int cap;
    int kpad;
};

// bootstrap sample: which rows (spread over the ensemble) feed the admission threshold,
// and at which granularity their minima are kept.  The scan then admits about
// k * R / rows windows.
//   per-wave mode: one minimum per 1024-window segment, 1/16 of the rows (more, up to a
//                  quarter, until there are >= 8k of them);
//   half-segment mode (per_wave = 2; the single-query matrix-core scan, whose two-class slices keep the
//                  selection cheap whatever tau admits): two minima per segment, half the rows -- the
//                  bootstrap is a latency-bound launch and one segment per wave is one round trip less;
//   per-lane mode: one minimum per 16 windows, for ensembles too small for the above;
//   rows == 0    : sample too thin to be useful -> exhaustive path.
struct BootPlan { int64_t rows; int per_wave; int64_t entries; };
// `estimate`: the scan admits below the sampled ESTIMATE of the k-th distance (embedded scan), so the sample only has
// to carry that estimate's rank (~2k * sampled fraction) comfortably -- 2k minima instead of the 8k that keep the
// provable k-th smallest tight.  (Never more entries than the plain plan: the workspace is sized for that one.)
// `thin` (with `estimate`): 1/64 of the rows -- the scans whose sample is itself expensive (the batched matrix-core scan's
// costs 2.2x a scan of the same rows: 0.58 of 4.9 ms at 512 queries with 1/16); the estimate's rank is then ~48.
BootPlan boot_plan(int64_t R, int64_t Tp, int k, bool halves = false, bool estimate = false, bool thin = false, double margin = 12.0) {
    BootPlan bp{0, 0, 0};
    const int64_t nseg = seg_count(Tp);
    const int64_t quarter = R / 4;
    int64_t rows = estimate ? (thin ? R / 64 : R / 32) : R / 16;
    // >= 8k segment minima for the provable bound; an estimate wants its rank (~1.5 k x the sampled fraction + 16) well
    // inside the sample: >= 1024 minima and >= 8 x the rank
    int64_t need_rows = (8 * (int64_t)k + nseg - 1) / nseg;
    if (estimate) {
        need_rows = (1024 + nseg - 1) / nseg;
        const double per_row = (double)nseg - margin * (double)k / (double)R;            // entries - 8 x rank (margin 12; 4.5: 3 x rank), per sampled row
        if (per_row > 0.25) { const int64_t nr = (int64_t)(128.0 / per_row) + 1; if (nr > need_rows) need_rows = nr; }
        else need_rows = quarter + 1;                                                    // k too close to the ensemble's size: no sample
    }
    if (rows < need_rows) rows = need_rows;
    if (rows >= 1 && rows <= quarter) {
        if (halves && rows >= 2) { bp.rows = (rows + 1) / 2; bp.per_wave = 2; bp.entries = bp.rows * nseg * 2; return bp; }
        bp.rows = rows; bp.per_wave = 1; bp.entries = rows * nseg; return bp;
    }
    const int64_t lanes_per_row = (Tp + PSH_L - 1) / PSH_L;             // real minima per row
    rows = ((estimate ? 4 : 32) * (int64_t)k + lanes_per_row - 1) / lanes_per_row;
    if (rows > quarter) rows = quarter;
    if (rows < 1 || rows * lanes_per_row < 4 * (int64_t)k) return bp;
    bp.rows = rows; bp.per_wave = 0; bp.entries = rows * nseg * 64;
    return bp;
}
// workspace sizing: the larger of the two per-segment variants (half-segment mode rounds the rows up)
int64_t boot_entries(int64_t R, int64_t Tp, int k) {
    const int64_t a = boot_plan(R, Tp, k, false).entries, b = boot_plan(R, Tp, k, true).entries;
    return a > b ? a : b;
}

// fixed part + cap * 12 bytes per query (the block slices / window slots)
size_t fixed_bytes(int B, int kpad, int64_t min_stride) {
    size_t o = PSH_FUSED_BYTES + PSH_PLAN_BYTES;
    o += align_up(sizeof(QueryState) * (size_t)B, 256);
    o += align_up(sizeof(int) * (size_t)B, 256);
    o += align_up(sizeof(float) * (size_t)B * (size_t)min_stride, 256);
    o += align_up(sizeof(int) * (size_t)B * PSH_MAX_BLOCKS, 256);
    o += align_up(sizeof(int) * PSH_MAX_BLOCKS, 256);
    o += align_up(sizeof(float) * PSH_MAX_BLOCKS, 256);
    o += align_up((size_t)512 * (size_t)((B + 3) & ~3), 256);
    o += align_up(sizeof(int2) * (size_t)B * kpad, 256);
    return o + 1024;  // alignment slack for the four candidate arrays
}

int carve(void* ws, size_t bytes, int B, int k, int64_t min_stride, Workspace* out) {
    const int kpad = next_pow2(k);
    const size_t fixed = fixed_bytes(B, kpad, min_stride);
    if (!ws || bytes <= fixed) return PSH_ERR_WORKSPACE;
    int64_t cap = (int64_t)((bytes - fixed) / (12 * (size_t)B));
    cap &= ~(int64_t)63;
    if (cap > (1 << 30)) cap = 1 << 30;
    if (cap <= 0) return PSH_ERR_WORKSPACE;
    char* p = (char*)ws;
    if (((uintptr_t)p & 255u) != 0) return PSH_ERR_ARG;   // torch allocations are >= 512-byte aligned
    out->fused = (FusedHdr*)p;    p += PSH_FUSED_BYTES;
    out->eplan = (EmbedPlan*)p;   p += PSH_PLAN_BYTES;
    out->qstate = (QueryState*)p; p += align_up(sizeof(QueryState) * (size_t)B, 256);
    out->total = (int*)p;         p += align_up(sizeof(int) * (size_t)B, 256);
    out->minbuf = (float*)p;      p += align_up(sizeof(float) * (size_t)B * (size_t)min_stride, 256);
    out->min_stride = min_stride;
    out->bcount = (int*)p;        p += align_up(sizeof(int) * (size_t)B * PSH_MAX_BLOCKS, 256);
    out->bcount2 = (int*)p;       p += align_up(sizeof(int) * PSH_MAX_BLOCKS, 256);
    out->blockmax = (float*)p;    p += align_up(sizeof(float) * PSH_MAX_BLOCKS, 256);
    out->mq_frag = (void*)p;      p += align_up((size_t)512 * (size_t)((B + 3) & ~3), 256);
    out->sel_rt = (int2*)p;       p += align_up(sizeof(int2) * (size_t)B * kpad, 256);
    out->cand_d = (float*)p;      p += align_up(sizeof(float) * (size_t)B * cap, 256);
    out->cand_rt = (int2*)p;
    out->cap = (int)cap;
    out->kpad = kpad;
    return PSH_OK;
}

// The overlap-friendly launches' lists of admitted windows (psh_stream.hip): 16-byte entries, one compact list per query.
// The workspace's two candidate arrays (4 + 8 bytes per entry of `cap`, adjacent) are taken as ONE region -- up to 65536
// entries per query (the ranking compares every pair: 64 k entries are ~0.3 ms, still a fraction of the separate launches a
// PSH_STATUS_RETRY costs) -- and FusedHdr::cand (16384 entries for the call) serves a workspace too small for more.
#define PSH_STREAM_LIST_MAX 65536
static void stream_cand_list(const Workspace& w, int B, void** list, int* cap_per_query) {
    const int64_t region = (int64_t)((char*)w.cand_rt - (char*)w.cand_d) + (int64_t)sizeof(int2) * B * (int64_t)w.cap;
    int64_t per = region / 16 / B;
    if (per > PSH_STREAM_LIST_MAX) per = PSH_STREAM_LIST_MAX;
    if (per > PSH_STREAM_CAND_CAP / B) { *list = (void*)w.cand_d; *cap_per_query = (int)per; }
    else { *list = (void*)w.fused->cand; *cap_per_query = PSH_STREAM_CAND_CAP / B; }
}

// candidate capacity per query: the scan writes one slice per block (up to
// PSH_MAX_BLOCKS of them), the exhaustive path one slot per window of a row chunk
int recommended_cap(int64_t Tp, int k) {
    const int64_t nseg = seg_count(Tp);
    int64_t cap = 128 * (int64_t)PSH_MAX_BLOCKS;          // 128 entries per block slice
    if (cap < 64 * (int64_t)k) cap = 64 * (int64_t)k;
    if (cap < k + 4 * nseg * PSH_SEG) cap = k + 4 * nseg * PSH_SEG;   // exhaustive: >= 4 rows per chunk
    return (int)((cap + 63) & ~(int64_t)63);
}

struct Problem {
    int64_t R, T, r_offset, Tp, N;
    int B, W, h, k;
    bool aligned;
    const float* ker;     // embedded scan: emb_d x W kernel matrix (device), else nullptr
    int emb_d;
    int qlen;             // floats per query vector handed over: W, or emb_d (pre-embedded queries)
    bool emb_dense;       // PSH_FLAG_EMBED_DENSE
    bool rows_generic;    // PSH_FLAG_ROWS_GENERIC
    bool emb_taps;        // PSH_FLAG_EMBED_TAPS
    bool emx_split;       // PSH_FLAG_EMBED_MX_SPLIT
    const EmbedPlan* eplan;   // embedded scan, sampled path: the plan region of the workspace when embed_plan_kernel runs, else nullptr
    bool emx;             // PSH_FLAG_EMBED_MX and the kernel fits: embed_mx_kernel (BOOT / FILTER)
};

int check_problem(const float* dataset, int64_t R, int64_t T, int64_t r_offset, const float* queries,
                  int B, int W, int h, int k, float* out_d, int32_t* out_idx, Problem* p,
                  const float* ker = nullptr, int emb_d = 0) {
    if (!dataset || !queries || !out_d || !out_idx) return PSH_ERR_ARG;
    if (emb_d < 0 || (emb_d > 0 && !ker)) return PSH_ERR_ARG;
    if (emb_d > PSH_EMB_MAX_D || (int64_t)emb_d * ((W + 3) & ~3) > PSH_EMB_MAX_TAPS) return PSH_ERR_UNSUPPORTED;
    if (R <= 0 || T <= 0 || B <= 0 || W <= 0 || h < 0 || k <= 0 || r_offset < 0) return PSH_ERR_ARG;
    if (W > PSH_MAX_W || k > PSH_MAX_K || B > PSH_MAX_B_PER_LAUNCH) return PSH_ERR_UNSUPPORTED;
    const int64_t Tp = T - W - h + 1;
    if (Tp <= 0) return PSH_ERR_ARG;
    if (T >= (1ll << 31) - PSH_SEG - 1024 || r_offset + R >= (1ll << 31)) return PSH_ERR_UNSUPPORTED;
    const int64_t N = R * Tp;
    if ((int64_t)k > N) return PSH_ERR_ARG;   // the reference raises too (topk: k out of range)
    p->R = R; p->T = T; p->r_offset = r_offset; p->Tp = Tp; p->N = N;
    p->B = B; p->W = W; p->h = h; p->k = k;
    p->aligned = (((uintptr_t)dataset & 15u) == 0) && (T % 4 == 0);
    p->ker = emb_d > 0 ? ker : nullptr;
    p->emb_d = emb_d;
    p->qlen = emb_d > 0 ? emb_d : W;
    p->emb_dense = false;
    p->rows_generic = false;
    p->emb_taps = false;
    p->emx_split = false;
    p->eplan = nullptr;
    p->emx = false;
    return PSH_OK;
}

// (row, t) packed into one 32-bit key -- rows r_offset .. r_offset + R - 1, t < Tp: the bits t takes, or -1 when the two do not fit
inline int index_tbits(const Problem& p) {
    int tb = 0;
    while ((1ll << tb) < p.Tp) ++tb;
    return ((p.R + p.r_offset) <= (1ll << (32 - tb))) ? tb : -1;
}

struct Plan { int grid; int n_qgroups; int q_per_group; int tile_floats; int wide; };
#define PSH_RESERVED_CUS 4           // PSH_FLAG_RESERVE_CUS: compute units a scan leaves to the side stream (collective, merge)

// Launch-geometry overrides and device-side time stamps for the scripts under tools/: compiled into the
// tuning build only (-DPSH_TUNING, `python -m shadowing_amd._build --tuning`).  The product library reads no
// environment variable and takes no pointer from anywhere but its arguments.
struct Tuning { int mq_i8; int dbg; int px_r1; int wide_min; bool narrow; int bpc; int rows_frac; unsigned long long* dbg_times; unsigned long long* dbg_select; int xcd_skew; int stream_pgrid_per_cu; int stream_skip; int stream_units; int stream_rgrid_per_cu; };
inline Tuning tuning() {
    Tuning t{1, 0, 0, PSH_EMB_WIDE_MIN_B, false, 0, 64, nullptr, nullptr, PSH_FUSED_XCD_SKEW, 2, 0, 2048, 2};
#ifdef PSH_TUNING
    if (const char* e = getenv("PSH_DBG")) t.dbg = atoi(e);
    if (const char* e = getenv("PSH_MQ_I8")) t.mq_i8 = atoi(e);                       // batched scan: 0 = the f16 rejection test (A/B), 2 = the 8-bit one whatever the batch
    if (const char* e = getenv("PSH_PX_R1")) { const int v = atoi(e); if (v >= 2) t.px_r1 = v; }   // prefix-sum scan: rows of the first phase (a large value: one phase)
    if (const char* e = getenv("PSH_EMBED_WIDE_MIN_B")) { const int v = atoi(e); if (v >= 1) t.wide_min = v; }
    t.narrow = getenv("PSH_EMBED_NARROW") != nullptr;
    if (const char* e = getenv("PSH_BLOCKS_PER_CU")) { const int v = atoi(e); if (v > 0) t.bpc = v; }
    if (const char* e = getenv("PSH_ROWS_FRAC")) { const int v = atoi(e); if (v >= 2) t.rows_frac = v; }
    if (const char* e = getenv("PSH_XCD_SKEW")) { const int v = atoi(e); if (v >= -64 && v <= 64) t.xcd_skew = v; }
    if (const char* e = getenv("PSH_STREAM_PGRID")) { const int v = atoi(e); if (v >= 1 && v <= 16) t.stream_pgrid_per_cu = v; }
    if (const char* e = getenv("PSH_STREAM_SKIP")) t.stream_skip = atoi(e);      // bit 0: no sample launch, 1: no ranking, 2: no scan (timing ablations: results are stale)
    if (const char* e = getenv("PSH_STREAM_RGRID")) { const int v = atoi(e); if (v >= 1 && v <= 8) t.stream_rgrid_per_cu = v; }
    if (const char* e = getenv("PSH_STREAM_UNITS")) { const int v = atoi(e); if (v >= 256 && v <= PSH_FUSED_MAX_UNITS) t.stream_units = v; }
    if (const char* e = getenv("PSH_DBG_TIMES_PTR")) t.dbg_times = (unsigned long long*)strtoull(e, nullptr, 0);
    if (const char* e = getenv("PSH_DBG_SELECT_PTR")) t.dbg_select = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
    return t;
}
inline int flags_of(const psh_profile* prof) { return prof ? prof->flags : 0; }

// One scan call: where it runs, the caller's pointers, and what is read ONCE per call -- the flag word, the profile mode, the
// device's CU count (behind the device guard), the tuning build's overrides.  Every route takes this, the Problem and the Workspace.
struct Call {
    int device; hipStream_t s;
    const float* dataset; const float* queries; const float* qnorm;
    float* out_d; int32_t* out_idx; int32_t* out_status;
    psh_profile* profile;
    int flags;            // psh_profile.flags (0 without a profile)
    bool stages, events;  // PSH_PROFILE_STAGES; PSH_PROFILE_EVENTS with both events given
    int ncu; Tuning tn;
    psh_filter_copy* fc;  // psh_scan_topk_copy: the resident f16 copy of `dataset` (nullable)
};
Call make_call(int device, void* stream, const float* dataset, const float* queries, const float* qnorm,
               float* out_d, int32_t* out_idx, int32_t* out_status, psh_profile* prof) {
    return Call{device, (hipStream_t)stream, dataset, queries, qnorm, out_d, out_idx, out_status, prof, flags_of(prof),
                prof && prof->mode == PSH_PROFILE_STAGES,
                prof && prof->mode == PSH_PROFILE_EVENTS && prof->ev_scan_begin && prof->ev_scan_end, 0, tuning()};
}

int plan_scan(const Call& c, const Problem& p, int64_t n_rows, Plan* plan) {
    const int tile_floats = tile_floats_for(p.W);
    int threads = 512, bpc = 1;       // embed_mx_kernel: 8 waves (two per SIMD), one block per CU
    bool wide = false;
    if (!p.emx) {
        // embedded scan of a batch: 512-thread blocks whose waves carry 12 (suffix rows: 6) queries per evaluation of the
        // embedding (256 VGPRs, one block per CU)
        wide = p.ker && p.B >= c.tn.wide_min && !c.tn.narrow;
        // a kernel matrix too large to sit in LDS beside sixteen wave tiles (Foveal(1.15, 0.9, 252): 39 x 252) runs the
        // 8-wave instantiation whatever the batch size
        if (p.ker && !wide && scan_shmem_bytes(tile_floats, p.B, p.emb_d, p.W, PSH_SCAN_THREADS) > PSH_LDS_BYTES) wide = true;
        threads = wide ? 512 : PSH_SCAN_THREADS;
        const size_t shmem = scan_shmem_bytes(tile_floats, p.B, p.emb_d, p.W, threads);
        if (shmem > PSH_LDS_BYTES) return PSH_ERR_UNSUPPORTED;
        if (!wide) HIP_TRY(scan_blocks_per_cu(p.W, p.aligned, p.ker != nullptr, shmem, &bpc));
        if (c.tn.bpc > 0) bpc = c.tn.bpc;
        if (bpc < 1) bpc = 1;
        if (bpc > 8) bpc = 8;
    }
    const int64_t n_rs = n_rows * seg_count(p.Tp);
    const int64_t waves = (int64_t)bpc * c.ncu * (threads / 64);
    // not enough (row, segment) units to fill the chip: also split the queries
    int n_qgroups = 1;
    if (n_rs < waves && p.B > 1) {
        int64_t g = (waves + n_rs - 1) / n_rs;
        n_qgroups = (int)(g < p.B ? g : p.B);
    }
    const int q_per_group = (p.B + n_qgroups - 1) / n_qgroups;
    n_qgroups = (p.B + q_per_group - 1) / q_per_group;
    const int64_t units = n_rs * n_qgroups;
    if (units >= (1ll << 31)) return PSH_ERR_UNSUPPORTED;
    plan->grid = (int)per_cu_grid(units, threads / 64, (int64_t)bpc * c.ncu, PSH_MAX_BLOCKS);
    plan->n_qgroups = n_qgroups;
    plan->q_per_group = q_per_group;
    plan->tile_floats = tile_floats;
    plan->wide = wide ? 1 : 0;
    return PSH_OK;
}

ScanArgs make_scan_args(const Call& c, const Problem& p, const Workspace& w,
                        const Plan& plan, int64_t row0, int64_t row_stride, int64_t n_rows) {
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.dataset = c.dataset;
    a.T = p.T;
    a.Tp = (int)p.Tp;
    a.nseg = (int)seg_count(p.Tp);
    a.W = p.W;
    a.row0 = row0;
    a.row_stride = row_stride;
    a.n_rows = (int)n_rows;
    {   // magic numbers of the unit decode: floor(2^32 / d), see fast_div
        const uint64_t n_rs = (uint64_t)n_rows * (uint64_t)a.nseg;
        a.magic_nrs = n_rs > 1 ? (unsigned)((1ull << 32) / n_rs) : 0u;
        a.magic_nseg = a.nseg > 1 ? (unsigned)((1ull << 32) / (uint64_t)a.nseg) : 0u;
    }
    a.r_offset = p.r_offset;
    a.queries = c.queries;
    a.ker = p.ker;
    a.hx = p.ker ? c.queries : nullptr;
    a.emb_d = p.emb_d;
    a.emb_wide = plan.wide;
    a.emb_dense = p.emb_dense ? 1 : 0;                  // PSH_FLAG_EMBED_DENSE: skip the suffix-rows fast path (A/B tests)
    a.emb_mx = p.emx ? (p.emx_split ? 3 : 1) : 0;
    a.emb_taps = p.emb_taps ? 1 : 0;
    a.emb_r1 = c.tn.px_r1;
    a.dbg = c.tn.dbg;
    a.plan = p.eplan;
    a.B = p.B;
    a.n_qgroups = plan.n_qgroups;
    a.q_per_group = plan.q_per_group;
    a.tile_floats = plan.tile_floats;
    a.k = p.k;
    a.qstate = w.qstate;
    a.minbuf = w.minbuf;
    a.min_stride = w.min_stride;
    a.cand_d = w.cand_d;
    a.cand_rt = w.cand_rt;
    a.bcount = w.bcount;
    a.slice = w.cap / plan.grid;
    a.cap = w.cap;
    return a;
}

// slices = true : rank what the FILTER scan left in `nblk` block slices; the queries' status words are written
// slices = false: rank the first n_fixed flat entries (r < 0 = empty)
SelectArgs make_select_args(const Call& c, const Problem& p, const Workspace& w, bool slices, int nblk, int n_fixed) {
    SelectArgs s;
    memset(&s, 0, sizeof(s));
    s.cand_d = w.cand_d;
    s.cand_rt = w.cand_rt;
    s.cand_stride = w.cap;
    s.bcount = slices ? w.bcount : nullptr;
    s.nblk = nblk;
    s.slice = slices ? w.cap / nblk : 0;
    s.total = w.total;
    s.n_fixed = n_fixed;
    s.cap = w.cap;
    s.k = p.k;
    s.kpad = w.kpad;
    s.skip_negative_rows = slices ? 0 : 1;
    s.out_d = c.out_d;
    s.out_idx = c.out_idx;
    s.sel_rt = w.sel_rt;
    s.sort_scratch = reinterpret_cast<uint64_t*>(w.cand_rt);   // (r, t) of the selected are in sel_rt by the time the ordering runs
    s.status = slices ? c.out_status : nullptr;
    s.qstate = w.qstate;
    return s;
}

int max_total(const Workspace& w, int B, int* out) {
    int cmax = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        int tmp[256];
        const int nb = (B - b0) < 256 ? (B - b0) : 256;
        HIP_TRY(hipMemcpy(tmp, w.total + b0, sizeof(int) * nb, hipMemcpyDeviceToHost));
        for (int i = 0; i < nb; ++i) cmax = tmp[i] > cmax ? tmp[i] : cmax;
    }
    *out = cmax;
    return PSH_OK;
}

struct Timer {   // optional per-stage HIP events
    bool on;
    hipStream_t s;
    hipEvent_t ev[8];
    int n = 0;
    Timer(bool enable, hipStream_t stream) : on(enable), s(stream) {}
    int init() {
        if (!on) return PSH_OK;
        for (int i = 0; i < 8; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        return PSH_OK;
    }
    int mark() {
        if (!on) return PSH_OK;
        HIP_TRY(hipEventRecord(ev[n++], s));
        return PSH_OK;
    }
    int elapsed(int i, int j, float* ms) {
        *ms = 0.f;
        if (!on) return PSH_OK;
        HIP_TRY(hipEventElapsedTime(ms, ev[i], ev[j]));
        return PSH_OK;
    }
    ~Timer() { if (on) for (int i = 0; i < 8; ++i) (void)hipEventDestroy(ev[i]); }
};

// ---- path 1: every window of the ensemble is ranked, a chunk of rows at a time
int run_exhaustive(const Call& c, const Problem& p_in, const Workspace& w) {
    Problem p = p_in;
    p.emx = false;                 // every window is ranked here: the dense chains of embed_scan_kernel, no rejection test
    p.eplan = nullptr;
    psh_profile* const prof = c.profile;
    const bool rows_path = p.Tp == 1 && !p.ker && !p.rows_generic;   // one-window rows: a slot per row (rows_kernel)
    const int64_t slots_per_row = rows_path ? 1 : seg_count(p.Tp) * PSH_SEG;
    if ((int64_t)w.cap < (int64_t)p.k + slots_per_row) return PSH_ERR_WORKSPACE;
    Timer tm(c.stages, c.s);
    int rc = tm.init(); if (rc) return rc;
    rc = tm.mark(); if (rc) return rc;
    PrepArgs pa{c.queries, c.qnorm, p.B, p.qlen, w.qstate, w.total, c.out_status};
    HIP_TRY(launch_prep(pa, c.s));
    rc = tm.mark(); if (rc) return rc;
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)prof->ev_scan_begin, c.s));
    int64_t rows_per_chunk = ((int64_t)w.cap - p.k) / slots_per_row;
    if (rows_per_chunk > p.R) rows_per_chunk = p.R;
    int grid_used = 0;
    for (int64_t r0 = 0; r0 < p.R; r0 += rows_per_chunk) {
        const int64_t nr = (r0 + rows_per_chunk <= p.R) ? rows_per_chunk : (p.R - r0);
        Plan plan;
        rc = plan_scan(c, p, nr, &plan); if (rc) return rc;
        grid_used = plan.grid;
        const int n_slots = (int)(nr * slots_per_row);
        // the running best (empty on the first chunk) sits right behind the window slots
        ReseedArgs ra{c.out_d, c.out_idx, w.qstate, w.cand_d, w.cand_rt, (int64_t)w.cap, n_slots, p.k};
        HIP_TRY(launch_reseed(ra, p.B, c.s));
        ScanArgs sa = make_scan_args(c, p, w, plan, r0, 1, nr);
        if (rows_path) HIP_TRY(launch_rows(sa, PSH_MODE_ALL, (int)rows_grid(nr, c.ncu), c.s));
        else HIP_TRY(launch_scan(sa, PSH_MODE_ALL, p.aligned, plan.grid, c.s));
        SelectArgs se = make_select_args(c, p, w, false, 0, n_slots + p.k);
        HIP_TRY(launch_select(se, p.B, c.s));
    }
    rc = tm.mark(); if (rc) return rc;
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)prof->ev_scan_end, c.s));
    if (prof) { prof->path = 1; prof->grid_blocks = grid_used; prof->n_sample_rows = 0; }
    if (c.stages) {
        HIP_TRY(hipStreamSynchronize(c.s));
        tm.elapsed(0, 1, &prof->prep_ms);
        tm.elapsed(1, 2, &prof->scan_ms);
        tm.elapsed(0, 2, &prof->total_ms);
        prof->sample_ms = prof->threshold_ms = prof->select_ms = 0.f;
        rc = max_total(w, p.B, &prof->n_candidates); if (rc) return rc;
    }
    return PSH_OK;
}

}  // namespace

extern "C" {

int psh_version(void) { return PSH_VERSION; }

const char* psh_strerror(int code) {
    switch (code) {
        case PSH_OK: return "ok";
        case PSH_ERR_ARG: return "invalid argument (null pointer, non-positive size, k larger than the number of windows, misaligned workspace)";
        case PSH_ERR_UNSUPPORTED: return "unsupported size (W > PSH_MAX_W, k > PSH_MAX_K, or int32 index overflow)";
        case PSH_ERR_WORKSPACE: return "workspace too small (see psh_workspace_bytes)";
        case PSH_ERR_HIP: return "HIP runtime error (see psh_last_hip_error)";
        case PSH_ERR_COMM: return "RCCL error (see psh_last_comm_error)";
        default: return "unknown error";
    }
}

const char* psh_last_hip_error(void) { return g_hip_err; }

int psh_workspace_bytes(int64_t R, int64_t T, int B, int W, int h, int k, size_t* out_bytes) {
    if (!out_bytes || R <= 0 || T <= 0 || B <= 0 || W <= 0 || h < 0 || k <= 0) return PSH_ERR_ARG;
    if (W > PSH_MAX_W || k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    const int64_t Tp = T - W - h + 1;
    if (Tp <= 0) return PSH_ERR_ARG;
    const int cap = recommended_cap(Tp, k);
    *out_bytes = fixed_bytes(B, next_pow2(k), boot_entries(R, Tp, k)) + (size_t)12 * (size_t)B * (size_t)cap + 64 * 12 * (size_t)B;
    return PSH_OK;
}

int psh_stream_create_reserving(int device, int reserve_cus, void** out_stream, int* out_reserved) {
    if (!out_stream || reserve_cus < 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    if (reserve_cus * 4 > ncu) reserve_cus = 0;             // a small device: nothing is reserved
    // one bit per compute unit; the FIRST `reserve_cus` bits are cleared (on a multi-XCD part the bits interleave over
    // the XCDs, so eight of them are one compute unit per XCD; were they not, they would be eight units of one XCD --
    // either way that many units stay free)
    uint32_t mask[32];
    const int words = (ncu + 31) / 32;
    if (words > 32) return PSH_ERR_UNSUPPORTED;
    for (int w = 0; w < words; ++w) {
        uint32_t m = 0xffffffffu;
        const int rem = ncu - 32 * w;
        if (rem < 32) m = (rem <= 0) ? 0u : ((1u << rem) - 1u);
        mask[w] = m;
    }
    for (int b = 0; b < reserve_cus; ++b) mask[b / 32] &= ~(1u << (b % 32));
    hipStream_t s = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask));
    *out_stream = (void*)s;
    if (out_reserved) *out_reserved = reserve_cus;
    return PSH_OK;
}

int psh_stream_destroy(int device, void* stream) {
    if (!stream) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return PSH_OK;
}

int psh_workspace_init(int device, void* stream, void* workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 255u) != 0) return PSH_ERR_ARG;
    if (workspace_bytes < PSH_FUSED_BYTES) return PSH_ERR_WORKSPACE;
    GUARD_DEVICE(device);
    HIP_TRY(launch_fused_init((FusedHdr*)workspace, (hipStream_t)stream));
    return PSH_OK;
}

int psh_query_norm(int device, void* stream, const float* queries, int B, int W, float* out_qnorm) {
    if (!queries || !out_qnorm || B <= 0 || W <= 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    HIP_TRY(launch_qnorm(queries, B, W, out_qnorm, (hipStream_t)stream));
    return PSH_OK;
}

static int scan_exhaustive_impl(Call c, int64_t R, int64_t T, int64_t r_offset, int B, int W, int h, int k, const float* ker, int emb_d,
                                void* workspace, size_t workspace_bytes) {
    Problem p;
    int rc = check_problem(c.dataset, R, T, r_offset, c.queries, B, W, h, k, c.out_d, c.out_idx, &p, ker, emb_d);
    if (rc) return rc;
    p.emb_dense = (c.flags & PSH_FLAG_EMBED_DENSE) != 0;
    p.rows_generic = (c.flags & PSH_FLAG_ROWS_GENERIC) != 0;
    Workspace w;
    rc = carve(workspace, workspace_bytes, B, k, boot_entries(p.R, p.Tp, k), &w);
    if (rc) return rc;
    GUARD_DEVICE(c.device);
    HIP_TRY(hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, c.device));
    return run_exhaustive(c, p, w);
}

int psh_scan_topk_exhaustive(int device, void* stream, const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                             const float* queries, const float* qnorm, int B, int W, int h, int k,
                             float* out_d, int32_t* out_idx, int32_t* out_status,
                             void* workspace, size_t workspace_bytes, psh_profile* profile) {
    return scan_exhaustive_impl(make_call(device, stream, dataset, queries, qnorm, out_d, out_idx, out_status, profile),
                                R, T, r_offset, B, W, h, k, nullptr, 0, workspace, workspace_bytes);
}

int psh_scan_topk_embedded_exhaustive(int device, void* stream, const float* dataset, int64_t R, int64_t T,
                                      int64_t r_offset, const float* kernel, int d, int K,
                                      const float* hx, const float* hxnorm, int B, int h, int k,
                                      float* out_d, int32_t* out_idx, int32_t* out_status,
                                      void* workspace, size_t workspace_bytes, psh_profile* profile) {
    if (!kernel || d <= 0) return PSH_ERR_ARG;
    if (T == (int64_t)K + h) return PSH_ERR_UNSUPPORTED;     // one-window rows: psh_embed_rows + psh_scan_topk (see psh.h)
    return scan_exhaustive_impl(make_call(device, stream, dataset, hx, hxnorm, out_d, out_idx, out_status, profile),
                                R, T, r_offset, B, K, h, k, kernel, d, workspace, workspace_bytes);
}

// queries one step of the long-window scan serves (34 <= W <= 256): up to three -- as many as put their fragment tables in LDS beside
// the waves' rows (W <= ~230: three; up to 256: two); 0 = not a long window
static int long_queries_per_step(int W) {
    if (!stream_long_supported(W)) return 0;
    for (int nq = PSH_STREAM_MAX_Q; nq > 1; --nq)
        if (stream_scan_long_shmem_bytes(W, nq) <= PSH_LDS_BYTES) return nq;
    return 1;
}

// what psh_shadow_blocking adds to a one-query call: the fused launch gathers the winners' paths itself and sets completion
// words the host polls; `taken` says whether the call was served that way (else: the caller enqueues the gather and waits
// for the stream)
struct BlockingExtras {
    const float* g_ds; float* g_out; int64_t g_T; int g_C, g_len;
    unsigned* done; unsigned done_val;
    bool taken; int shards;
    const float* q_host; const float* hint_host;      // the query (W floats) and, nullable, the admission level as the HOST reads them
};

// Several queries with a window the batched kernels' bands do not reach (they stop at W = 25): who serves them.
//   long_q:   queries one step of the three launches takes with this window (0: not a long window);
//   use_lq:   four queries and more with a long window -- or two / three that do not ride one pass of the three launches (W > 97 /
//             145: their tables do not fit beside the scan's rows) --: ONE pass per chunk of queries of the batched long-window scan
//             (psh_lq.hip) through the separate launches' pipeline, instead of the loop of steps;
//   per_step: a LOOP of the steps that do have a matrix-core rejection test, inside the call (scan_in_chunks) --
//     34 <= W <= 256: up to three queries per step (the three launches with the long-window scan, psh_stream.hip: the
//                     queries share the pass, the conversion and the energies' MFMAs);
//     26 <= W <= 33, four queries and more: three queries per step (the three launches' 2-3 query form).
// Round 6: what is left to the loop is PSH_FLAG_LONG_LOOP and shapes the batched long-window scan does not take (use_lq
// serves four queries and more with 26 <= W <= 256 and two / three that do not ride one pass).
// The one-pass vector-ALU filter costs W fma per window and query: R = 32768, T = 4096, W = 126 -- 2 / 4 / 16 / 64 queries
// 1.14 / 2.19 / 8.6 / 33.6 ms in one pass, 0.34 / 0.65 / 2.6 / 10.6 ms as a loop; W = 252: 2.2 .. 67 against 0.50 .. 16.2 ms
// (tools/long_batch_probe.py).
struct LongPlan { int long_q; bool use_lq; int per_step; };
static LongPlan plan_long(const Problem& p, int flags) {
    LongPlan lp;
    lp.long_q = long_queries_per_step(p.W);
    lp.use_lq = !p.ker && p.Tp > 1 && (p.B >= 4 || (lp.long_q > 0 && p.B > lp.long_q)) && scan_lq_supported(p.W, p.B, p.T) &&
                !(flags & (PSH_FLAG_FILTER_VALU | PSH_FLAG_NO_FUSE | PSH_FLAG_LONG_LOOP));
    lp.per_step = !p.ker && p.Tp > 1 ? (lp.long_q > 0 && p.B > lp.long_q ? lp.long_q : (p.W >= 26 && p.W <= 33 && p.B > PSH_STREAM_MAX_Q ? PSH_STREAM_MAX_Q : 0)) : 0;
    return lp;
}

static int scan_topk_impl(Call c, int64_t R, int64_t T, int64_t r_offset, int B, int W, int h, int k, const float* ker, int emb_d,
                          void* workspace, size_t workspace_bytes, BlockingExtras* bx = nullptr);

// The call as sub-calls of at most `per` queries each (the steps of a long window, the chunks of the matrix-core embedded
// scan): outputs, status words, query norms and hints at the queries' offsets.  Status words stay per query; a RETRY of
// any step sends the caller's WHOLE call to PSH_FLAG_NO_FUSE, as the protocol says.  psh_profile then describes the LAST
// sub-call: path, grid, and in PSH_PROFILE_EVENTS mode the bracket of that step's scan (the caller's tau_hint pointer stays).
static int scan_in_chunks(const Call& c, const Problem& p, int per, void* workspace, size_t workspace_bytes) {
    psh_profile sub;
    for (int b = 0; b < p.B; b += per) {
        const int nb = p.B - b < per ? p.B - b : per;
        Call cc = c;
        cc.queries = c.queries + (size_t)b * p.qlen;
        cc.qnorm = c.qnorm ? c.qnorm + b : nullptr;
        cc.out_d = c.out_d + (size_t)b * p.k;
        cc.out_idx = c.out_idx + (size_t)b * p.k * 2;
        cc.out_status = c.out_status + b;
        if (c.profile) { sub = *c.profile; if (sub.tau_hint) sub.tau_hint += b; cc.profile = &sub; }
        const int rc = scan_topk_impl(cc, p.R, p.T, p.r_offset, nb, p.W, p.h, p.k, p.ker, p.emb_d, workspace, workspace_bytes);
        if (rc) return rc;
    }
    if (c.profile) { const float* hint0 = c.profile->tau_hint; *c.profile = sub; c.profile->tau_hint = hint0; }
    return PSH_OK;
}

// Which route serves a call, and the sample it draws: decided here, launched elsewhere.
struct Route {
    bool use_mx, use_mq, use_lq;        // the full scan's cheap test on the matrix cores: one query; batched (4 queries x 8 shifts per MFMA); batched, long window
    bool mq_i8;                         // the batched scan's rejection test as the 8-bit product
    bool rows_path, rows_wave_min;      // one-window rows (rows_kernel, a row per lane); their bootstrap keeps one minimum per chunk of 64 sampled rows
    bool mx_estimate, boot_emx;         // one query with a large k admits below an estimate; the matrix-core embedded scan samples half segments itself
    bool exhaustive;                    // path 1
    int long_q;
    BootPlan bp;
    int64_t n_sample, stride, row0;     // the sampled rows: row0 + i * stride
    const float* hint;                  // the caller's admission levels (psh_profile.tau_hint): no bootstrap sample anywhere
};

static Route decide_route(const Call& c, const Problem& p, const Workspace& w, const LongPlan& lp) {
    Route rt{};
    rt.long_q = lp.long_q;
    rt.use_lq = lp.use_lq;
    // the cheap test of the full scan runs on the matrix cores where that is implemented
    // (PSH_FLAG_FILTER_VALU keeps it on the vector ALUs: comparison runs, tools/)
    rt.use_mx = !p.ker && scan_mx_supported(p.W, p.B);
    rt.use_mq = !p.ker && scan_mq_supported(p.W, p.B);
    if (c.flags & PSH_FLAG_FILTER_VALU) rt.use_mx = rt.use_mq = false;
    // the batched scan's rejection test: the 8-bit product (scan_mq8_kernel) unless the caller asks for f16
    // (from 32 queries on: a segment's set-up is ~1.5 k cycles dearer with the 8-bit test -- two passes over the staged values, the
    //  energies turned into integers, the levels of every query -- and that is what a small batch pays for; 4 queries 230 against
    //  179 us per call, 16: 303 / 279, 32: 373 / 395, 128: 778 / 1083)
    rt.mq_i8 = c.tn.mq_i8 != 0 && !(c.flags & PSH_FLAG_MQ_F16) && (p.B >= 32 || c.tn.mq_i8 > 1);
    // (half-segment mode measured for the single-query scan: bootstrap 17.4 -> 12.3 us, but tau admits twice as
    // much and the scan's exact rechecks cost 4.3 us more -- 135.7 vs 134.3 us per step; left off)
    // (the matrix-core embedded scan samples one minimum per HALF segment; a sample too thin for that plan is taken by
    // embed_scan_kernel instead -- the full scan still runs on the matrix cores)
    rt.bp = boot_plan(p.R, p.Tp, p.k, p.emx, p.ker != nullptr || !rt.use_mx, !p.ker && !rt.use_mx);
    // A single query with a LARGE k (the reference's own example call: Identity(20), R = 32768, k = 8192 -- testing.ipynb): the
    // provable bound wants 8 k segment minima, more than a quarter of the rows have; the plan then fell to one minimum per LANE
    // (264 k minima, 0.19 ms to find the k-th among them, a bound that admitted 4.6 k candidates per k).  Such a call admits below
    // an ESTIMATE instead, like the embedded scans do: 1/32 of the rows, the r2-th smallest of their segment minima with ~1.5 k
    // windows of the ensemble expected below it; fewer than k found -> status -> the caller's exhaustive pass.
    // (a sample of moderate size keeps its provable bound: per lane up to 100 k minima, per segment up to an eighth of the rows)
    if (rt.use_mx && ((rt.bp.per_wave == 0 && rt.bp.entries > 100000) || (rt.bp.per_wave == 1 && rt.bp.rows * 8 > p.R))) {
        const BootPlan be = boot_plan(p.R, p.Tp, p.k, false, true, false, 4.5);
        if (be.per_wave == 1 && be.entries <= w.min_stride) { rt.bp = be; rt.mx_estimate = true; }
    }
    rt.boot_emx = p.emx && rt.bp.per_wave == 2;
    if (p.emx && !rt.boot_emx) rt.bp = boot_plan(p.R, p.Tp, p.k, false, true);
    // one-window rows (T == W + h; PathDistance.forward_topk's N pre-embedded points): rows_kernel, a row per lane.
    // Its bootstrap takes one exact value per sampled row.
    rt.rows_path = p.Tp == 1 && !p.ker && !p.rows_generic;
    if (rt.rows_path) {
        const int frac = c.tn.rows_frac;
        int64_t ns = p.R / frac > 16 * (int64_t)p.k ? p.R / frac : 16 * (int64_t)p.k;
        if (ns > p.R / 2) ns = p.R / 2;
        if (ns > w.min_stride) ns = w.min_stride;
        rt.bp.rows = ns >= 2 * (int64_t)p.k ? ns : 0;
        rt.bp.per_wave = 1;
        rt.bp.entries = rt.bp.rows;
        // the estimate's rank (sample_ranks) against the chunks of 64 rows of the sample: sparse enough -> one minimum per chunk
        const int64_t r2r = (6 * (int64_t)p.k * rt.bp.rows + 2 * p.R - 1) / (2 * p.R) + 16, chunks = (rt.bp.rows + 63) / 64;
        rt.rows_wave_min = rt.bp.rows > 0 && r2r < p.k && 8 * r2r <= chunks;
        if (rt.rows_wave_min) rt.bp.entries = chunks;
        rt.use_mx = rt.use_mq = false;
    }
    rt.hint = c.profile ? c.profile->tau_hint : nullptr;
    rt.n_sample = rt.bp.rows;
    // small problems (everything fits the candidate buffer), one-window rows (their
    // numerator uses another reduction order, handled by the exhaustive kernel only) or
    // a sample too thin to be useful: exhaustive path
    rt.exhaustive = p.R * seg_count(p.Tp) * PSH_SEG + p.k <= (int64_t)w.cap || (p.Tp == 1 && !rt.rows_path) || (rt.n_sample == 0 && !rt.hint);
    rt.stride = rt.n_sample > 0 ? p.R / rt.n_sample : 1;
    rt.row0 = rt.stride / 2;
    return rt;
}

// what the fused launch (path 2) and the three overlap-friendly launches (path 3) are told alike: a sample of `units` (row,
// segment) units over `rows` rows spread over the ensemble, and the rank of the admission level among their minima
static FusedArgs fused_args(const Call& c, const Problem& p, const Workspace& w, const Route& rt, int64_t units, int64_t rows, int64_t rank) {
    FusedArgs fu;
    memset(&fu, 0, sizeof(fu));
    fu.hdr = w.fused;
    fu.boot_units = (int)units;
    fu.boot_row_stride = p.R / rows;
    fu.boot_row0 = fu.boot_row_stride / 2;
    fu.rank = (int)rank;
    fu.qnorm_in = c.qnorm;
    fu.out_d = c.out_d;
    fu.out_idx = c.out_idx;
    fu.status = c.out_status;
    fu.total = w.total;
    fu.tbits = index_tbits(p);
    fu.tau_hint = rt.hint;
    return fu;
}

// ---- path 3: the step as three overlap-friendly launches (psh_stream.hip: sample + levels in one-wave blocks, the barrier-free
// scan, the ranking): ONE query when the caller says other steps are in flight on other streams (PSH_FLAG_OVERLAP), and
// always for two or three queries -- they ride one pass over the ensemble at about one query's cost, where the batched
// scan (sized for hundreds of queries) streams at half rate.  *served: the launches are enqueued and the profile is filled.
static int try_stream_step(const Call& c, const Problem& p, const Workspace& w, const Route& rt, bool* served) {
    *served = false;
    const int B = p.B;
    const bool small_batch = !p.ker && !rt.rows_path && B >= 2 && B <= PSH_STREAM_MAX_Q && !(c.flags & PSH_FLAG_FILTER_VALU);
    const bool one_overlap = rt.use_mx && B == 1 && (c.flags & PSH_FLAG_OVERLAP);
    // ONE query with a long window (34 <= W <= 256): the same three launches, flag or no flag, with the scan's banded product
    // as a K-loop (stream_scan_long_kernel) -- otherwise such a call has only the vector-ALU filter of scan_kernel
    // (the long-window scan's deferred survivors pack t into 30 bits)
    const bool one_long = !p.ker && !rt.rows_path && rt.long_q > 0 && B <= rt.long_q && !(c.flags & PSH_FLAG_FILTER_VALU) && p.T < (1ll << 30);
    if (!((small_batch || one_overlap || one_long) && !rt.rows_path && !c.stages && !(c.flags & PSH_FLAG_NO_FUSE) &&
          (scan_fused_supported(p.W) || one_long)))
        return PSH_OK;
    const Tuning& tn = c.tn;
    const int64_t nseg = seg_count(p.Tp);
    // a thinner sample than the fused launch's: its megabytes are HBM traffic beside ANOTHER step's scan here.  2048
    // units (what the exchange area holds, split between the queries); the level is the r2p-th smallest minimum (below): the
    // k best windows of the ensemble put kf = k x sampled fraction = 16 expected minima below their level at the benchmark's
    // sizes, P(Poisson(16) >= 40) = 3e-7 that fewer than k windows lie below the estimate (-> PSH_STATUS_RETRY)
    int64_t units_cap = tn.stream_units < 2048 ? tn.stream_units : 2048;     // (the sample kernel keeps a query's minima in registers: <= 2048)
    // (a long window's exact sample chains cost W / 20 of the benchmark's: half the units -- the level's rank stays at its
    //  floor of 24 with 8 minima expected below the k-th distance)
    // (round 6: without a hint a long window's sample runs on the matrix cores -- stream_sample_long_kernel, upper bounds of the
    //  minima -- and takes the full 2048 units; PSH_STREAM_SKIP bit 3 of the tuning build: the exact chains, for A/B runs)
    const bool long_mx_sample = one_long && !rt.hint && !(tn.stream_skip & 8) &&
                                stream_sample_long_shmem_bytes(p.W, B) <= (size_t)PSH_LDS_BYTES;
    if (one_long && !long_mx_sample && units_cap > 1024) units_cap = 1024;
    if (units_cap > PSH_FUSED_MAX_UNITS / B) units_cap = PSH_FUSED_MAX_UNITS / B;
    int64_t rows_p = units_cap / nseg;
    if (rows_p > p.R / 4) rows_p = p.R / 4;
    if (rows_p < 1) rows_p = 1;
    const int64_t units_p = rows_p * nseg;
    // the level's rank among the sampled minima: the k best windows of the ensemble put at most kf = k x sampled fraction
    // minima below their level (Poisson), so the (kf + 5 sqrt(kf) + 4)-th smallest lies above it but for five sigma -- 40 at
    // the benchmark's kf = 16 (what 2 kf + 8 gave until round 6: the same there, but twelve sigma at kf = 128, where it
    // admitted twice the windows a smooth ensemble's lists hold)
    const double kf = (double)p.k * (double)rows_p / (double)p.R;
    int64_t r2p = (int64_t)ceil(kf + 5.0 * sqrt(kf)) + 4;
    if (r2p < 24) r2p = 24;
    int64_t grid_p = (int64_t)tn.stream_pgrid_per_cu * c.ncu;
    // (a long window's sample is its exact chains -- 1024 windows x W taps per unit, 11 us at W = 126 -- not its bytes:
    //  one unit per wave instead of two, unless the caller says other steps' scans share the chip: three streams measured
    //  +2 % with it, a lone stream's call 3 - 10 % less -- 3 queries with W = 126: 317 -> 284 us)
    if (one_long && !(c.flags & PSH_FLAG_OVERLAP)) grid_p *= 2;
    if (grid_p > units_p) grid_p = units_p;
    int64_t grid_s = c.ncu;
    // a stream made by psh_stream_create_reserving: one block per compute unit the stream may use
    if ((c.flags & PSH_FLAG_RESERVE_CUS) && c.ncu >= 4 * PSH_STREAM_RESERVED_CUS) grid_s = c.ncu - PSH_STREAM_RESERVED_CUS;
    const int64_t n_rs = p.R * nseg;
    if (grid_s * (PSH_SCAN_THREADS / 64) > n_rs) grid_s = (n_rs + (PSH_SCAN_THREADS / 64) - 1) / (PSH_SCAN_THREADS / 64);
    const int front = B == 1 ? PSH_FUSED_FRONT : 2 * PSH_FUSED_FRONT;
    int cand_cap = 0;
    void* cand_list = nullptr;
    stream_cand_list(w, B, &cand_list, &cand_cap);
    const int tile_fl = mx_tile_floats(p.W);
    // (copy_scan_kernel's LDS -- copy_scan_shmem_bytes -- is stream_scan_kernel's less 64 KB: where the fp32 scan fits, it fits)
    if (!((one_long ? stream_scan_long_shmem_bytes(p.W, B) : stream_scan_shmem_bytes_q(tile_fl, B)) <= PSH_LDS_BYTES &&
          ((units_p >= 256 && r2p <= units_p / 2) || rt.hint) &&
          5 * (int64_t)p.k <= (int64_t)cand_cap && 5 * (int64_t)p.k * B <= grid_s * front * 2))
        return PSH_OK;
    const Plan plan_s{(int)grid_s, 1, B, tile_fl, 0};
    ScanArgs fa = make_scan_args(c, p, w, plan_s, 0, 1, p.R);
    fa.dbg_times = tn.dbg_times;
    FusedArgs fu = fused_args(c, p, w, rt, units_p, rows_p, r2p);
    fu.front = front;
    fu.nq = B;
    fu.units_stride = (int)((PSH_FUSED_MAX_UNITS / B) & ~3);
    fu.cand_cap = cand_cap;
    fu.cand_list = cand_list;
    fu.k_out = p.k;
    // the caller's resident f16 copy serves ONE route: one query, W <= 33, PSH_FLAG_OVERLAP (with a tau_hint or without: the sample
    // launch's last block derives the step's scale either way) -- and only a copy of this shape
    CopyArgs cp{nullptr, nullptr, 0};
    if (c.fc) {
        c.fc->served = 0;
        if (!(one_overlap && !one_long)) c.fc->reason = PSH_COPY_NOT_ROUTE;
        else if (!(c.fc->copy && c.fc->R == p.R && c.fc->T == p.T && c.fc->pitch_halves == filter_copy_pitch(p.T) && p.r_offset + p.R < (1ll << 31) &&
                   ((uintptr_t)c.fc->copy & 15) == 0))
            c.fc->reason = PSH_COPY_MISMATCH;
        else {
            cp.hdr = reinterpret_cast<const CopyHdr*>(c.fc->copy);
            cp.rows = reinterpret_cast<const unsigned short*>(cp.hdr + 1);
            cp.pitch = c.fc->pitch_halves;
            fu.copy_ec = &cp.hdr->e_c;
        }
    }
    if (rt.hint) grid_p = 1;                  // nothing is sampled: one block derives scale, thresholds and the fragment table from the hints
    if (!(tn.stream_skip & 1)) HIP_TRY(long_mx_sample ? launch_stream_sample_long(fa, fu, (int)grid_p, c.s)
                                                      : launch_stream_sample(fa, fu, p.aligned, (int)grid_p, tile_floats_for(p.W), c.s));
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_begin, c.s));
    if (!(tn.stream_skip & 4)) HIP_TRY(cp.hdr ? launch_copy_scan(fa, fu, cp, (int)grid_s, c.s)
                                       : one_long ? launch_stream_scan_long(fa, fu, p.aligned, (int)grid_s, c.s)
                                                  : launch_stream_scan(fa, fu, p.aligned, (int)grid_s, c.s));
    if (cp.hdr) { c.fc->served = 1; c.fc->reason = PSH_COPY_SERVED; }
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_end, c.s));
    // (~2.5 k candidates per query: <= 8 own ones per wave, ONE pass over all of them)
    if (!(tn.stream_skip & 2)) HIP_TRY(launch_stream_rank(fa, fu, tn.stream_rgrid_per_cu * c.ncu, c.s));
    if (c.profile) { c.profile->path = 3; c.profile->n_sample_rows = (int)rows_p; c.profile->grid_blocks = (int)grid_s; }
    *served = true;
    return PSH_OK;
}

// ---- path 2: the whole step as ONE launch (psh_fused.hip): a single query on the matrix-core scan whose bootstrap sample is
// one minimum per (row, segment) unit and fits the exchange area.  Anything that goes wrong inside raises
// PSH_STATUS_RETRY in out_status and the caller reruns with PSH_FLAG_NO_FUSE.  `bx` (psh_shadow_blocking): the launch also
// gathers the winners' paths and sets the completion words.  *served: the launch is enqueued and the profile is filled.
static int try_fused_step(const Call& c, const Problem& p, const Workspace& w, const Route& rt, BlockingExtras* bx, bool* served) {
    *served = false;
    if (!(rt.use_mx && !rt.rows_path && !c.stages && !(c.flags & PSH_FLAG_NO_FUSE) && scan_fused_supported(p.W))) return PSH_OK;
    Plan plan_f;
    const int rc = plan_scan(c, p, p.R, &plan_f); if (rc) return rc;
    if ((c.flags & PSH_FLAG_RESERVE_CUS) && plan_f.grid > 2 * PSH_RESERVED_CUS) plan_f.grid -= PSH_RESERVED_CUS;
    // its own sample: only an ESTIMATE of the k-th smallest acc is needed (what is admitted is verified exactly, and
    // "at least k admitted" proves the result complete), so at most PSH_FUSED_MAX_UNITS (row, segment) units -- one
    // minimum each -- spread over at most a quarter of the ensemble
    const int64_t nseg = seg_count(p.Tp);
    int64_t rows_f = PSH_FUSED_MAX_UNITS / nseg;
    if (rows_f > p.R / 4) rows_f = p.R / 4;
    const int64_t units_f = rows_f * nseg;
    // the admission level: the rank-th smallest sampled minimum -- ~2k windows of the whole ensemble expected below it
    // (~3k when that rank is small and therefore noisy)
    int64_t r2 = rows_f > 0 ? (2 * (int64_t)p.k * rows_f + p.R - 1) / p.R : 0;
    r2 += r2 < 64 ? r2 / 2 + 16 : 8;
    // (~2.5 k candidates are expected: they must fit the blocks' front lists with room to spare)
    if (!(plan_f.grid <= PSH_FUSED_MAX_BLOCKS && ((rows_f >= 1 && units_f >= 256 && r2 <= units_f / 2) || rt.hint) &&
          5 * (int64_t)p.k <= (int64_t)plan_f.grid * PSH_FUSED_FRONT))
        return PSH_OK;
    const int tile_fl = mx_tile_floats(p.W);
    if (scan_fused_shmem_bytes(tile_fl) > PSH_LDS_BYTES) return PSH_OK;
    // (a caller that asked for the overlap-friendly launches may be on a stream that cannot hold the fused
    //  launch's blocks all at once -- a CU mask, other scans in flight: where they do not apply, the separate
    //  launches serve the call, never the fused one)
    if (c.flags & PSH_FLAG_OVERLAP) return PSH_OK;
    ScanArgs fa = make_scan_args(c, p, w, plan_f, 0, 1, p.R);
    fa.tile_floats = tile_fl;
    fa.dbg_times = c.tn.dbg_times;
    if (rows_f < 1) rows_f = 1;
    FusedArgs fu = fused_args(c, p, w, rt, units_f, rows_f, r2);
    // give-up time of a poll at the 100 MHz wall clock: 2 ms (a block that is not resident); 20 ms when a
    // collective shares the chip (its workgroups may hold a few CUs until the peers arrive)
    fu.spin_ticks = (c.flags & PSH_FLAG_RESERVE_CUS) ? 2000000 : 200000;
    fu.xcd_skew = (plan_f.grid % 8 == 0) ? c.tn.xcd_skew : 0;      // (a grid that is not whole rounds of the 8 XCDs: no assumption)
    if (bx) {
        fu.g_ds = bx->g_ds; fu.g_out = bx->g_out; fu.g_T = bx->g_T; fu.g_C = bx->g_C; fu.g_len = bx->g_len;
        fu.done = bx->done; fu.done_val = bx->done_val;
        memcpy(fu.qv, bx->q_host, sizeof(float) * (size_t)p.W);              // (W <= 33: scan_fused_supported)
        if (bx->hint_host) fu.hint_v = *bx->hint_host;
        fu.done_shards = plan_f.grid < PSH_FUSED_DONE_SHARDS ? plan_f.grid : PSH_FUSED_DONE_SHARDS;
        bx->taken = true; bx->shards = fu.done_shards;
    }
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_begin, c.s));
    HIP_TRY(launch_scan_fused(fa, fu, p.aligned, plan_f.grid, c.s));
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_end, c.s));
    if (c.profile) { c.profile->path = 2; c.profile->n_sample_rows = (int)rows_f; c.profile->grid_blocks = plan_f.grid; }
    *served = true;
    return PSH_OK;
}

// ---- path 0, first launch: the bootstrap sample -- minima of the sampled rows into w.minbuf, for the threshold kernel.
// *n_blockmax: the blocks whose max |y| the threshold kernel reads (the matrix-core scans' scale).
static int launch_bootstrap(const Call& c, const Problem& p, const Workspace& w, const Route& rt, int* n_blockmax) {
    const int64_t n_rows = rt.n_sample > 0 ? rt.n_sample : 1;
    Plan plan_s;
    const int rc = plan_scan(c, p, n_rows, &plan_s); if (rc) return rc;
    ScanArgs sa = make_scan_args(c, p, w, plan_s, rt.row0, rt.stride, n_rows);
    sa.boot_per_wave = rt.bp.per_wave;
    sa.emb_mx = rt.boot_emx ? 1 : 0;
    sa.blockmax = (rt.use_mx || rt.use_mq) ? w.blockmax : nullptr;
    *n_blockmax = plan_s.grid;
    // the batch's tables and constants (the bootstrap's f16 copies, nx~, the f16 scale; the 8-bit test's step and residue
    // norms): whichever bootstrap follows, the threshold kernel reads the meta words
    if (rt.use_mq) HIP_TRY(launch_mq_prep(c.queries, p.B, p.W, w.mq_frag, c.s));
    // (a single query is better served by the exact bootstrap: 8192 segments are a latency-bound launch either
    // way -- 20.8 vs 18.7 us measured -- and the exact minima admit 9 % fewer candidates)
    if (rt.hint) {
        // the caller's levels: nothing is sampled (the threshold kernel takes tau = tau2 = hint[b])
        *n_blockmax = 0;
    } else if (rt.use_mq && rt.bp.per_wave == 1 && boot_mq_supported(p.W)) {
        // segment minima as matrix-core upper bounds (boot_mq_kernel) instead of exact chains
        const int chunks = boot_mq_chunks(p.B);
        int64_t gx = per_cu_grid(rt.n_sample * sa.nseg, 8, c.ncu);
        while (gx * chunks > PSH_MAX_BLOCKS) gx /= 2;
        if (gx < 1) gx = 1;
        *n_blockmax = (int)gx * chunks;
        sa.mq_frag = w.mq_frag;
        // (the rank the threshold kernel will select, sample_ranks: an estimate's rank -> the minima may be estimates too)
        const int64_t r2e = (4 * (int64_t)p.k * rt.n_sample + 2 * p.R - 1) / (2 * p.R) + 8;
        sa.boot_estimate = (r2e < p.k && r2e <= rt.bp.entries) ? 1 : 0;
        HIP_TRY(launch_boot_mq(sa, p.aligned, (int)gx, c.s));
    } else if (rt.use_lq && rt.bp.per_wave == 1) {
        // upper bounds of the segment minima of every query from the batched long-window kernel (one pass over the sampled rows)
        sa.q_per_group = scan_lq_chunk(p.W, p.B);
        sa.n_qgroups = (p.B + sa.q_per_group - 1) / sa.q_per_group;
        HIP_TRY(launch_scan_lq(sa, PSH_MODE_BOOT, (int)per_cu_grid(rt.n_sample * sa.nseg, 8, c.ncu), c.s));
    } else if (rt.rows_path) {
        sa.boot_wave_min = rt.rows_wave_min ? 1 : 0;
        HIP_TRY(launch_rows(sa, PSH_MODE_BOOT, (int)rows_grid(rt.n_sample, c.ncu), c.s));
    } else {
        HIP_TRY(launch_scan(sa, PSH_MODE_BOOT, p.aligned, plan_s.grid, c.s));
    }
    return PSH_OK;
}

// path 0: the ranks the threshold kernel reads off the sample.  k_thr: the rank it selects exactly (the admission level);
// rank2 > 0: a single query on the matrix cores files its candidates in two classes around an ESTIMATE of the k-th
// smallest acc (the rank2-th smallest sampled minimum ~ 2k windows of the whole ensemble below it).
struct SampleRanks { int k_thr; int rank2; };
static SampleRanks sample_ranks(const Problem& p, const Route& rt) {
    SampleRanks sr{p.k, 0};
    const int64_t k = p.k, n_sample = rt.n_sample;
    if (rt.hint) {
        // one class of candidates below the caller's level
    } else if (rt.use_mx && rt.mx_estimate) {
        // the number of sampled minima below the ensemble's k-th smallest value is ~ Binomial(entries, k / windows): mean m = k x
        // the sampled fraction, deviation sqrt(m) -- the rank m + 4.5 sqrt(m) + 8 falls short of k windows once in ~10^5 calls
        // (-> status -> the exhaustive pass) and admits ~1.3 k candidates at k = 8192 instead of the 1.6 k of a flat 1.5 m
        const double m = (double)k * (double)n_sample / (double)p.R;
        const int64_t r2 = (int64_t)(m + 4.5 * sqrt(m) + 8.0) + 1;
        if (r2 < k && r2 <= rt.bp.entries) sr.k_thr = (int)r2;
    } else if (rt.use_mx) {
        const int64_t r2 = (2 * k * n_sample + p.R - 1) / p.R + 8;
        sr.rank2 = (r2 < k && r2 <= rt.bp.entries) ? (int)r2 : 0;
    } else {            // every other scan: the embedded ones, one-window rows, the batched matrix-core scan, the VALU-filter scans
        // The embedded scan (and the scan of one-window rows) ADMITS below an estimate: a candidate costs it an exact
        // d x K chain, and the provable tau of a 1/16 sample lets ~16 k of them through.  The estimate is the r2-th
        // smallest sampled minimum, r2 ~ 1.5 k x the sampled fraction (3 k for the thin 1/64 sample of one-window
        // rows) + 16: ~1.5 k (3 k) windows of the whole ensemble lie below it, k only after a 4..14 sigma shortfall.
        // Everything with acc below it is found, so when at least k windows are, the result is the exact top-k; when
        // fewer are, the selection raises the query's status and the caller takes the exhaustive path, as for an
        // overflow.  The threshold kernel selects THIS rank exactly (tau = tau2 = the estimate): read off a bucket edge
        // of the rank-k selection it came out 1.5x too generous, and 25 k candidates per query miss the selection's
        // LDS-resident path (16384 keys) that 12 k take.
        // (the batched matrix-core scan too, at ~2 k: with the provable tau nearly every second group of 4 queries met a
        //  candidate in a segment and left the fast path of its loop -- the handling of survivors was half its instructions)
        // (the thin 1/64 sample of the batched / VALU-filter scans: + 8 on a rank of ~32 -- k windows of the ensemble
        //  put 16 expected minima of the sample below their level, P(Poisson(16) >= 40) = 3e-7 per query; the minima are
        //  upper bounds, which only adds to the margin)
        const bool thin = !p.ker && !rt.rows_path;
        const int64_t r2 = ((p.ker ? 3 : (rt.rows_path ? 6 : 4)) * k * n_sample + 2 * p.R - 1) / (2 * p.R) + (thin ? 8 : 16);
        if (r2 < k && r2 <= rt.bp.entries) sr.k_thr = (int)r2;
    }
    return sr;
}

// ---- path 0, third launch: the full scan, admitting below the threshold kernel's levels into one slice of the candidate
// arrays per block.  *nblk: the blocks whose slices the selection reads.
static int launch_filter(const Call& c, const Problem& p, const Workspace& w, const Route& rt, int rank2, int* nblk) {
    Plan plan_f;
    const int rc = plan_scan(c, p, p.R, &plan_f); if (rc) return rc;
    // a CU-masked stream (psh_stream_create_reserving): one resident round of blocks on the compute units it may use
    if ((c.flags & PSH_FLAG_RESERVE_CUS) && (c.flags & PSH_FLAG_OVERLAP) && plan_f.grid > 4 * PSH_STREAM_RESERVED_CUS && !p.ker)
        plan_f.grid -= PSH_STREAM_RESERVED_CUS;
    ScanArgs fa = make_scan_args(c, p, w, plan_f, 0, 1, p.R);
    fa.use_mx = rt.use_mx ? 1 : 0;
    fa.bcount2 = (rt.use_mx && rank2 > 0) ? w.bcount2 : nullptr;
    // scan_mx_kernel reads the fp32 tile only window by window (no sliding refills past the segment):
    // SEG + W - 1 values rounded up to whole float4 stores, padded layout -- every byte counts, the
    // kernel uses 155+ of the 160 KB of LDS
    if (rt.use_mx) fa.tile_floats = mx_tile_floats(p.W);
    fa.dbg_times = c.tn.dbg_times;
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_begin, c.s));
    *nblk = plan_f.grid;
    if (rt.use_mq || rt.use_lq) {
        // one block of 8 waves per CU and query chunk (grid.y); a query's candidates come from the blocks of its
        // chunk only, so slices are indexed by blockIdx.x alone.  (A 16x16x32 layout -- 2 queries x 8 shifts per
        // MFMA, 12 waves per block at 168 VGPRs -- was built and measured: 6.4 ms against 4.7 for the scan.)
        *nblk = (int)per_cu_grid(p.R * seg_count(p.Tp), 8, c.ncu, PSH_MAX_BLOCKS);
        fa.slice = w.cap / *nblk;
        if (rt.use_mq) {
            fa.mq_frag = w.mq_frag;
            fa.mq_i8 = rt.mq_i8 ? 1 : 0;
            HIP_TRY(launch_scan_mq(fa, p.aligned, *nblk, c.s));
        } else {
            fa.q_per_group = scan_lq_chunk(p.W, p.B);
            fa.n_qgroups = (p.B + fa.q_per_group - 1) / fa.q_per_group;
            HIP_TRY(launch_scan_lq(fa, PSH_MODE_FILTER, *nblk, c.s));
        }
    } else if (rt.rows_path) {
        *nblk = (int)rows_grid(p.R, c.ncu, PSH_MAX_BLOCKS);
        fa.slice = w.cap / *nblk;
        HIP_TRY(launch_rows(fa, PSH_MODE_FILTER, *nblk, c.s));
    } else {
        HIP_TRY(launch_scan(fa, PSH_MODE_FILTER, p.aligned, plan_f.grid, c.s));
    }
    if (c.events) HIP_TRY(hipEventRecord((hipEvent_t)c.profile->ev_scan_end, c.s));
    return PSH_OK;
}

// ---- path 0, last launch: the k best of what the scan left in its `nblk` block slices
static int launch_selection(const Call& c, const Problem& p, const Workspace& w, const Route& rt, int rank2, int nblk) {
    SelectArgs se = make_select_args(c, p, w, true, nblk, 0);
    se.unsorted_ok = (c.flags & PSH_FLAG_UNSORTED) ? 1 : 0;
    se.bcount2 = (rt.use_mx && rank2 > 0) ? w.bcount2 : nullptr;
    if (rt.use_mx && rank2 > 0) { se.dataset = c.dataset; se.queries = c.queries; se.T = p.T; se.r_offset = p.r_offset; se.W = p.W; }
    se.dbg_times = c.tn.dbg_select;
    // (the flags sit behind the B <= 8 totals in their 256-byte slot of the workspace: ints 32 .. 39)
    if (p.B <= PSH_RANK_MAX_B && !(c.flags & PSH_FLAG_SELECT_ONE_BLOCK)) {
        se.rank_tbits = index_tbits(p);
        se.handled = w.total + 32;
    }
    HIP_TRY(launch_select(se, p.B, c.s));
    return PSH_OK;
}

// ---- path 0: the separate launches -- bootstrap sample, threshold, filter scan, selection
static int run_sampled(const Call& c, const Problem& p, const Workspace& w, const Route& rt) {
    psh_profile* const profile = c.profile;
    Timer tm(c.stages, c.s);
    int rc = tm.init(); if (rc) return rc;
    rc = tm.mark(); if (rc) return rc;                                       // 0
    PrepArgs pa{c.queries, c.qnorm, p.B, p.qlen, w.qstate, w.total, c.out_status};  // runs inside the threshold kernel
    rc = tm.mark(); if (rc) return rc;                                       // 1
    int n_blockmax = 0;
    rc = launch_bootstrap(c, p, w, rt, &n_blockmax); if (rc) return rc;
    rc = tm.mark(); if (rc) return rc;                                       // 2
    const SampleRanks sr = sample_ranks(p, rt);
    ThresholdArgs ta{w.minbuf, w.min_stride, rt.hint ? 0 : (int)rt.bp.entries, w.qstate, sr.k_thr, 0,
                     ((rt.use_mx || rt.use_mq) && !rt.hint) ? w.blockmax : nullptr, n_blockmax, rt.use_mq ? w.mq_frag : nullptr,
                     rt.mq_i8 ? 1 : 0, sr.rank2, pa, rt.hint};
    HIP_TRY(launch_threshold(ta, p.B, c.s));
    rc = tm.mark(); if (rc) return rc;                                       // 3
    int nblk = 0;
    rc = launch_filter(c, p, w, rt, sr.rank2, &nblk); if (rc) return rc;
    rc = tm.mark(); if (rc) return rc;                                       // 4
    rc = launch_selection(c, p, w, rt, sr.rank2, nblk); if (rc) return rc;
    rc = tm.mark(); if (rc) return rc;                                       // 5
    if (profile) {
        profile->path = 0;
        profile->n_sample_rows = rt.hint ? 0 : (int)rt.n_sample;
        profile->grid_blocks = nblk;           // the blocks whose slices the selection read (psh_candidates_layout)
    }
    if (c.stages) {
        HIP_TRY(hipStreamSynchronize(c.s));
        tm.elapsed(0, 1, &profile->prep_ms);
        tm.elapsed(1, 2, &profile->sample_ms);
        tm.elapsed(2, 3, &profile->threshold_ms);
        tm.elapsed(3, 4, &profile->scan_ms);
        tm.elapsed(4, 5, &profile->select_ms);
        tm.elapsed(0, 5, &profile->total_ms);
        rc = max_total(w, p.B, &profile->n_candidates); if (rc) return rc;
    }
    return PSH_OK;
}

// psh_scan_topk, psh_scan_topk_embedded (ker, emb_d) and psh_shadow_blocking (bx): check, the chunk loops, then
// carve -> device guard -> embed plan -> route -> exhaustive? the three launches? the fused launch? the separate launches
static int scan_topk_impl(Call c, int64_t R, int64_t T, int64_t r_offset, int B, int W, int h, int k, const float* ker, int emb_d,
                          void* workspace, size_t workspace_bytes, BlockingExtras* bx) {
    Problem p;
    int rc = check_problem(c.dataset, R, T, r_offset, c.queries, B, W, h, k, c.out_d, c.out_idx, &p, ker, emb_d);
    if (rc) return rc;
    if (!c.out_status) return PSH_ERR_ARG;
    const LongPlan lp = plan_long(p, c.flags);
    // (the loop pays only when its sub-calls get the three launches: 5 k candidates in a query's list of 65536, a sample of 256
    //  units and more -- a call outside that would be B / 3 passes with the vector-ALU filter instead of one)
    const bool step_fits = 5 * (int64_t)k <= 65536 && p.R * seg_count(p.Tp) >= 1024;
    if (lp.per_step && step_fits && !lp.use_lq && !c.stages && !(c.flags & (PSH_FLAG_FILTER_VALU | PSH_FLAG_NO_FUSE)))
        return scan_in_chunks(c, p, lp.per_step, workspace, workspace_bytes);
    // A dense embedding's batch beyond what the matrix-core scan takes in one call (its per-query pass runs on the matrix cores
    // for up to 256 queries -- PSH_EMX_QM_MAX_B -- and the queries' constants sit in LDS): chunks of the largest supported size inside the call instead of the vector-ALU
    // scan for all of them (configs[4] with 512 query dates: 46 -> 10 ms per GPU).  Status words stay per query.
    if (p.ker && (c.flags & PSH_FLAG_EMBED_MX) && !(c.flags & PSH_FLAG_EMBED_DENSE) && p.Tp > 1 && B > 3 &&
        (B > 256 || !embed_mx_supported(emb_d, W, B, tile_floats_for(W))) && !c.stages) {
        int chunk = 0;
        for (int n = B < 256 ? B : 256; n >= 3; n = n > 32 ? n - 32 : n - 1)
            if (embed_mx_supported(emb_d, W, n, tile_floats_for(W))) { chunk = n; break; }
        if (chunk >= 3) {
            const int n_chunks = (B + chunk - 1) / chunk;
            return scan_in_chunks(c, p, (B + n_chunks - 1) / n_chunks, workspace, workspace_bytes);   // even chunks
        }
    }
    p.emb_dense = (c.flags & PSH_FLAG_EMBED_DENSE) != 0;
    p.rows_generic = (c.flags & PSH_FLAG_ROWS_GENERIC) != 0;
    p.emb_taps = (c.flags & PSH_FLAG_EMBED_TAPS) != 0;
    p.emx_split = (c.flags & PSH_FLAG_EMBED_MX_SPLIT) != 0;
    p.emx = p.ker && (c.flags & PSH_FLAG_EMBED_MX) && !p.emb_dense && p.Tp > 1 &&
            embed_mx_supported(p.emb_d, p.W, p.B, tile_floats_for(p.W));
    Workspace w;
    rc = carve(workspace, workspace_bytes, B, k, boot_entries(p.R, p.Tp, k), &w);
    if (rc) return rc;
    if ((int64_t)w.cap < (int64_t)k + seg_count(p.Tp) * PSH_SEG) return PSH_ERR_WORKSPACE;
    GUARD_DEVICE(c.device);
    HIP_TRY(hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, c.device));
    // a linear embedding that may be Foveal-like on one interval: the matrix is looked at on the device (one small launch),
    // and of the two kernels launched per stage the one the structure belongs to does the work (psh_embed_px.hip)
    const bool want_plan = p.ker && !p.emb_dense && !p.emb_taps && !p.emx && p.Tp > 1 &&
                           embed_px_supported(tile_floats_for(p.W), p.B, p.emb_d, p.W, false) &&
                           embed_px_supported(tile_floats_for(p.W), p.B, p.emb_d, p.W, true);
    // (in front of the decision between the sampled and the exhaustive path: with PSH_FLAG_EMBED_PLAN_KEEP the next call may
    //  take the other one)
    if (want_plan && !(c.flags & PSH_FLAG_EMBED_PLAN_KEEP)) HIP_TRY(launch_embed_plan(p.ker, p.emb_d, p.W, w.eplan, c.s));
    const Route rt = decide_route(c, p, w, lp);
    if (rt.exhaustive) return run_exhaustive(c, p, w);
    if (want_plan) p.eplan = w.eplan;
    bool served = false;
    rc = try_stream_step(c, p, w, rt, &served);
    if (rc || served) return rc;
    rc = try_fused_step(c, p, w, rt, bx, &served);
    if (rc || served) return rc;
    return run_sampled(c, p, w, rt);
}

int psh_scan_topk(int device, void* stream, const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                  const float* queries, const float* qnorm, int B, int W, int h, int k,
                  float* out_d, int32_t* out_idx, int32_t* out_status,
                  void* workspace, size_t workspace_bytes, psh_profile* profile) {
    return scan_topk_impl(make_call(device, stream, dataset, queries, qnorm, out_d, out_idx, out_status, profile),
                          R, T, r_offset, B, W, h, k, nullptr, 0, workspace, workspace_bytes);
}

int psh_filter_copy_bytes(int64_t R, int64_t T, size_t* bytes, int64_t* pitch_halves) {
    if (!bytes || !pitch_halves || R <= 0 || T <= 0) return PSH_ERR_ARG;
    if (T >= (1ll << 31) - PSH_SEG - 1024 || R >= (1ll << 31)) return PSH_ERR_UNSUPPORTED;
    const int64_t pitch = filter_copy_pitch(T);
    *pitch_halves = pitch;
    *bytes = sizeof(CopyHdr) + (size_t)R * (size_t)pitch * 2;
    return PSH_OK;
}

int psh_filter_copy_build(int device, void* stream, const float* dataset, int64_t R, int64_t T, void* out, size_t out_bytes,
                          void* scratch, size_t scratch_bytes) {
    size_t need = 0;
    int64_t pitch = 0;
    if (!dataset || !out || !scratch) return PSH_ERR_ARG;
    const int rc = psh_filter_copy_bytes(R, T, &need, &pitch); if (rc) return rc;
    if (out_bytes < need || scratch_bytes < PSH_FILTER_COPY_SCRATCH_BYTES) return PSH_ERR_WORKSPACE;
    if (((uintptr_t)out & 15) || ((uintptr_t)scratch & 7)) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    HIP_TRY(launch_filter_copy_build(dataset, R, T, out, scratch, (hipStream_t)stream));
    return PSH_OK;
}

int psh_scan_topk_copy(int device, void* stream, const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                       const float* queries, const float* qnorm, int B, int W, int h, int k,
                       float* out_d, int32_t* out_idx, int32_t* out_status,
                       void* workspace, size_t workspace_bytes, psh_profile* profile, psh_filter_copy* copy) {
    Call c = make_call(device, stream, dataset, queries, qnorm, out_d, out_idx, out_status, profile);
    c.fc = copy;
    // (every route but the one the copy serves leaves these as they are: the call went the ordinary way)
    if (copy) { copy->served = 0; copy->reason = PSH_COPY_NOT_ROUTE; }
    return scan_topk_impl(c, R, T, r_offset, B, W, h, k, nullptr, 0, workspace, workspace_bytes);
}

int psh_scan_topk_embedded(int device, void* stream, const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                           const float* kernel, int d, int K, const float* hx, const float* hxnorm, int B, int h, int k,
                           float* out_d, int32_t* out_idx, int32_t* out_status,
                           void* workspace, size_t workspace_bytes, psh_profile* profile) {
    if (!kernel || d <= 0) return PSH_ERR_ARG;
    if (T == (int64_t)K + h) return PSH_ERR_UNSUPPORTED;     // one-window rows: psh_embed_rows + psh_scan_topk (see psh.h)
    return scan_topk_impl(make_call(device, stream, dataset, hx, hxnorm, out_d, out_idx, out_status, profile),
                          R, T, r_offset, B, K, h, k, kernel, d, workspace, workspace_bytes);
}

int psh_merge_workspace_bytes(int B, int k, size_t* out_bytes) {
    if (!out_bytes || B <= 0 || k <= 0) return PSH_ERR_ARG;
    if (k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    *out_bytes = align_up(sizeof(int2) * (size_t)B * next_pow2(k), 256);
    return PSH_OK;
}

int psh_merge_topk(int device, void* stream, const float* d_lists, const int32_t* idx_lists, int B, int n_in, int k,
                   float* out_d, int32_t* out_idx, void* workspace, size_t workspace_bytes) {
    if (!d_lists || !idx_lists || !out_d || !out_idx || !workspace || B <= 0 || n_in <= 0 || k <= 0) return PSH_ERR_ARG;
    if (k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    if (((uintptr_t)idx_lists & 7u) != 0 || ((uintptr_t)workspace & 7u) != 0) return PSH_ERR_ARG;
    const int kpad = next_pow2(k);
    if (workspace_bytes < sizeof(int2) * (size_t)B * kpad) return PSH_ERR_WORKSPACE;
    GUARD_DEVICE(device);
    SelectArgs s;
    memset(&s, 0, sizeof(s));
    s.cand_d = d_lists;
    s.cand_rt = (const int2*)idx_lists;
    s.cand_stride = n_in;
    s.bcount = nullptr;
    s.n_fixed = n_in;
    s.cap = n_in;
    s.k = k;
    s.kpad = kpad;
    s.skip_negative_rows = 1;
    s.out_d = out_d;
    s.out_idx = out_idx;
    s.sel_rt = (int2*)workspace;
    s.status = nullptr;
    s.qstate = nullptr;
    HIP_TRY(launch_select(s, B, (hipStream_t)stream));
    return PSH_OK;
}

int psh_merge_topk_gathered(int device, void* stream, const float* d_gathered, const int32_t* idx_gathered,
                            int G, int64_t rank_stride, int64_t rank_stride_idx, int B, int k_in, int k,
                            float* out_d, int32_t* out_idx, void* workspace, size_t workspace_bytes) {
    if (!d_gathered || !idx_gathered || !out_d || !out_idx || !workspace || G <= 0 || B <= 0 || k_in <= 0 || k <= 0) return PSH_ERR_ARG;
    if (rank_stride < (int64_t)B * k_in || rank_stride_idx < (int64_t)B * k_in || (int64_t)G * k_in >= (1ll << 31)) return PSH_ERR_ARG;
    if (k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    if (((uintptr_t)idx_gathered & 7u) != 0 || ((uintptr_t)workspace & 7u) != 0) return PSH_ERR_ARG;
    const int kpad = next_pow2(k);
    if (workspace_bytes < sizeof(int2) * (size_t)B * kpad) return PSH_ERR_WORKSPACE;
    GUARD_DEVICE(device);
    SelectArgs s;
    memset(&s, 0, sizeof(s));
    s.cand_d = d_gathered;
    s.cand_rt = (const int2*)idx_gathered;
    s.cand_stride = k_in;              // query b's lists start b * k_in into every rank block
    s.bcount = nullptr;
    s.n_fixed = G * k_in;
    s.list_len = k_in;
    s.list_stride = rank_stride;
    s.list_stride_rt = rank_stride_idx;
    s.cap = G * k_in;
    s.k = k;
    s.kpad = kpad;
    s.skip_negative_rows = 1;
    s.out_d = out_d;
    s.out_idx = out_idx;
    s.sel_rt = (int2*)workspace;
    HIP_TRY(launch_select(s, B, (hipStream_t)stream));
    return PSH_OK;
}

int psh_merge_sorted_gathered(int device, void* stream, const float* d_gathered, const int32_t* idx_gathered,
                              int G, int64_t rank_stride, int64_t rank_stride_idx, int B, int k_in, int k,
                              float* out_d, int32_t* out_idx) {
    if (!d_gathered || !idx_gathered || !out_d || !out_idx || G <= 0 || B <= 0 || k_in <= 0 || k <= 0) return PSH_ERR_ARG;
    if (rank_stride < (int64_t)B * k_in || rank_stride_idx < (int64_t)B * k_in) return PSH_ERR_ARG;
    if (((uintptr_t)idx_gathered & 7u) != 0) return PSH_ERR_ARG;
    if (G > 64 || (int64_t)G * k_in * 4 > 128 * 1024 || (int64_t)k > (int64_t)G * k_in + PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    GUARD_DEVICE(device);
    MergeSortedArgs m{d_gathered, (const int2*)idx_gathered, rank_stride, rank_stride_idx, G, k_in, k, out_d, out_idx};
    HIP_TRY(launch_merge_sorted(m, B, (hipStream_t)stream));
    return PSH_OK;
}

size_t psh_embed_plan_offset(void) { return PSH_FUSED_BYTES; }

int psh_candidates_layout(int64_t R, int64_t T, int B, int W, int h, int k, size_t workspace_bytes, int64_t* out14) {
    int64_t* out12 = out14;
    if (!out12 || R <= 0 || T <= 0 || B <= 0 || W <= 0 || h < 0 || k <= 0) return PSH_ERR_ARG;
    if (W > PSH_MAX_W || k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    const int64_t Tp = T - W - h + 1;
    if (Tp <= 0) return PSH_ERR_ARG;
    Workspace w;
    char* const base = (char*)(uintptr_t)4096;             // (carve only does pointer arithmetic: any 256-byte aligned base)
    const int rc = carve(base, workspace_bytes, B, k, boot_entries(R, Tp, k), &w);
    if (rc) return rc;
    out12[0] = (char*)w.qstate - base;
    out12[1] = (char*)w.bcount - base;
    out12[2] = (char*)w.bcount2 - base;
    out12[3] = (char*)w.cand_d - base;
    out12[4] = (char*)w.cand_rt - base;
    out12[5] = w.cap;
    out12[6] = (int64_t)offsetof(FusedHdr, cand);
    out12[7] = (int64_t)offsetof(FusedHdr, blk);
    out12[8] = (int64_t)(offsetof(FusedHdr, stream) + offsetof(StreamCtl, ncand));
    out12[9] = PSH_MAX_BLOCKS;
    out12[10] = PSH_FUSED_MAX_BLOCKS;
    out12[11] = PSH_FUSED_FRONT;
    {   // the overlap-friendly launches' lists (w.fused sits at the base)
        void* list = nullptr;
        int per = 0;
        stream_cand_list(w, B, &list, &per);
        out14[12] = (char*)list - base;
        out14[13] = per;
    }
    return PSH_OK;
}

int psh_embedded_supported(int d, int K) {
    if (d <= 0 || K <= 0 || d > PSH_EMB_MAX_D || K > PSH_MAX_W || (int64_t)d * ((K + 3) & ~3) > PSH_EMB_MAX_TAPS) return 0;
    return scan_shmem_bytes(tile_floats_for(K), PSH_MAX_B_PER_LAUNCH, d, K, 512) <= PSH_LDS_BYTES ? 1 : 0;
}

int psh_embed_rows(int device, void* stream, const float* dataset, int64_t R, int64_t T,
                   const float* kernel, int d, int K, float* out) {
    if (!dataset || !kernel || !out || R <= 0 || T <= 0 || d <= 0 || K <= 0 || K > T) return PSH_ERR_ARG;
    if (d > PSH_EMB_MAX_D || (int64_t)d * ((K + 3) & ~3) > PSH_EMB_MAX_TAPS) return PSH_ERR_UNSUPPORTED;
    GUARD_DEVICE(device);
    HIP_TRY(launch_embed_rows(dataset, R, T, kernel, d, K, out, (hipStream_t)stream));
    return PSH_OK;
}

int psh_gather_paths(int device, void* stream, const float* dataset, int64_t R, int64_t C, int64_t T, int64_t r_offset,
                     const int32_t* idx, int64_t n, int len, float* out) {
    if (!dataset || !idx || !out || R <= 0 || C <= 0 || T <= 0 || n < 0 || len <= 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    GatherArgs a{dataset, R, C, T, r_offset, idx, n, (int64_t)len, out};
    HIP_TRY(launch_gather(a, (hipStream_t)stream));
    return PSH_OK;
}

// ---- one BLOCKING shadow() of one Identity query (reference path_shadowing.py:181-218) --------------------------------
int psh_shadow_block_layout(int W, int h, int k, int64_t C, size_t* out7) {
    if (!out7 || W <= 0 || W > PSH_MAX_W || h < 0 || k <= 0 || k > PSH_MAX_K || C <= 0) return PSH_ERR_ARG;
    const size_t n_d = (size_t)4 * k, n_i = (size_t)8 * k, n_p = (size_t)4 * k * (size_t)C * (size_t)(W + h);
    const size_t o_d = PSH_SHADOW_OFF_QUERY + (size_t)4 * PSH_MAX_W;
    const size_t o_i = align_up(o_d + n_d, 256), o_p = align_up(o_i + n_i, 256);
    out7[0] = align_up(o_p + n_p, 256);
    out7[1] = PSH_SHADOW_OFF_STATUS; out7[2] = PSH_SHADOW_OFF_QUERY; out7[3] = PSH_SHADOW_OFF_HINT;
    out7[4] = o_d; out7[5] = o_i; out7[6] = o_p;
    return PSH_OK;
}

static inline double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

int psh_shadow_blocking(int device, void* stream, const float* rows, int64_t R, int64_t T, int64_t r_offset,
                        const float* dataset3, int64_t C, int W, int h, int k,
                        void* host_block, size_t host_block_bytes, int with_hint,
                        void* workspace, size_t workspace_bytes, psh_profile* profile) {
    size_t lay[7];
    int rc = psh_shadow_block_layout(W, h, k, C, lay);
    if (rc) return rc;
    if (!host_block || host_block_bytes < lay[0] || !dataset3 || !rows) return PSH_ERR_ARG;
    char* hb = static_cast<char*>(host_block);
    volatile unsigned* done = reinterpret_cast<volatile unsigned*>(hb + PSH_SHADOW_OFF_DONE);
    unsigned* seqp = reinterpret_cast<unsigned*>(hb + PSH_SHADOW_OFF_SEQ);
    const unsigned seq = (*seqp = *seqp + 1u == 0u ? 1u : *seqp + 1u);       // never 0: a fresh block's words
    int32_t* status = reinterpret_cast<int32_t*>(hb + PSH_SHADOW_OFF_STATUS);
    *status = -1;                                                              // (a call that never ran leaves no OK behind)
    psh_profile pf;
    if (profile) pf = *profile; else memset(&pf, 0, sizeof(pf));
    pf.mode = PSH_PROFILE_EVENTS;
    pf.ev_scan_begin = pf.ev_scan_end = nullptr;
    pf.tau_hint = with_hint ? reinterpret_cast<const float*>(hb + PSH_SHADOW_OFF_HINT) : nullptr;
    const double t_begin = now_s();
    BlockingExtras bx{dataset3, reinterpret_cast<float*>(hb + lay[6]), T, (int)C, W + h,
                      const_cast<unsigned*>(done), seq, false, 0,
                      reinterpret_cast<const float*>(hb + PSH_SHADOW_OFF_QUERY), with_hint ? reinterpret_cast<const float*>(hb + PSH_SHADOW_OFF_HINT) : nullptr};
    __atomic_thread_fence(__ATOMIC_SEQ_CST);                                   // query, hint, status: in memory before the doorbell
    rc = scan_topk_impl(make_call(device, stream, rows, reinterpret_cast<const float*>(hb + PSH_SHADOW_OFF_QUERY), nullptr,
                                  reinterpret_cast<float*>(hb + lay[4]), reinterpret_cast<int32_t*>(hb + lay[5]), status, &pf),
                        R, T, r_offset, 1, W, h, k, nullptr, 0, workspace, workspace_bytes, &bx);
    if (profile) { const float* th = profile->tau_hint; const int md = profile->mode; void* e0 = profile->ev_scan_begin; void* e1 = profile->ev_scan_end;
                   *profile = pf; profile->tau_hint = th; profile->mode = md; profile->ev_scan_begin = e0; profile->ev_scan_end = e1; }
    if (rc) return rc;
    GUARD_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    if (!bx.taken) {
        // not the fused launch (a window or a k it does not serve, a small ensemble): the gather as its own launch, and the
        // stream's end is the call's end
        GatherArgs a{dataset3, R, C, T, r_offset, reinterpret_cast<const int32_t*>(hb + lay[5]), (int64_t)k, (int64_t)(W + h),
                     reinterpret_cast<float*>(hb + lay[6])};
        HIP_TRY(launch_gather(a, s));
        HIP_TRY(hipStreamSynchronize(s));
        return PSH_OK;
    }
    // the launch's completion words (one per shard of its blocks) land in this block as the last thing it writes; a launch
    // that returned early (RETRY before its scan) sets none -- the stream says so
    const double t0 = now_s();
    reinterpret_cast<float*>(hb + PSH_SHADOW_OFF_TIMES)[0] = (float)(1e6 * (t0 - t_begin));     // diagnostics: us spent enqueueing
    double t_query = t0 + 60e-6;
    volatile unsigned* started = reinterpret_cast<volatile unsigned*>(hb + PSH_SHADOW_OFF_STARTED);
    bool seen_start = false, seen_first = false;
    for (unsigned spin = 1;; ++spin) {
        if (!seen_start && *started == seq) { seen_start = true; reinterpret_cast<float*>(hb + PSH_SHADOW_OFF_TIMES)[2] = (float)(1e6 * (now_s() - t0)); }
        bool all = true, any = false;
        for (int i = 0; i < bx.shards; ++i) { const bool d = done[i] == seq; all = all && d; any = any || d; }
        if (any && !seen_first) { seen_first = true; reinterpret_cast<float*>(hb + PSH_SHADOW_OFF_TIMES)[3] = (float)(1e6 * (now_s() - t0)); }
        if (all) break;
        __builtin_ia32_pause();
        if ((spin & 63u) == 0u) {
            const double t = now_s();
            if (t >= t_query) {
                const hipError_t q = hipStreamQuery(s);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) { snprintf(g_hip_err, sizeof(g_hip_err), "hipStreamQuery -> %s", hipGetErrorString(q)); return PSH_ERR_HIP; }
                t_query = now_s() + 15e-6;
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    reinterpret_cast<float*>(hb + PSH_SHADOW_OFF_TIMES)[1] = (float)(1e6 * (now_s() - t0));          // ... and waiting
    return PSH_OK;
}

int psh_count_nonfinite(int device, void* stream, const float* x, int64_t n, unsigned long long* out_count) {
    if (!x || !out_count || n < 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    HIP_TRY(launch_count_nonfinite(x, n, out_count, (hipStream_t)stream));
    return PSH_OK;
}

int psh_rows_nonfinite(int device, void* stream, const float* dataset, int64_t R, int64_t C, int64_t T, int32_t* out_flags) {
    if (!dataset || !out_flags || R < 0 || C <= 0 || T <= 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    HIP_TRY(launch_rows_nonfinite(dataset, R, C * T, out_flags, (hipStream_t)stream));
    return PSH_OK;
}

int psh_smear_nonfinite(int device, void* stream, const float* dataset, int64_t R, int64_t C, int64_t T, int back, int fwd, float* out) {
    if (!dataset || !out || R < 0 || C <= 0 || T <= 0 || back < 0 || fwd < 0) return PSH_ERR_ARG;
    if (R * T >= ((int64_t)1 << 31) * 256) return PSH_ERR_UNSUPPORTED;
    GUARD_DEVICE(device);
    HIP_TRY(launch_smear_nonfinite(dataset, R, C, T, back, fwd, out, (hipStream_t)stream));
    return PSH_OK;
}

int psh_weighted_moments(int device, void* stream, const float* values, const double* weights, int B, int k, int m,
                         double* out_mean, double* out_std) {
    if (!values || !out_mean || !out_std || B <= 0 || k <= 0 || m <= 0) return PSH_ERR_ARG;
    GUARD_DEVICE(device);
    MomentsArgs a{values, weights, B, k, m, out_mean, out_std};
    HIP_TRY(launch_moments(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_realized_variance(int device, void* stream, const float* x, int64_t n_rows, int64_t row_stride, int len,
                          const int* Ts, int nT, int vol, float* out) {
    if (!x || !Ts || !out || n_rows < 0 || len <= 0 || row_stride < len || nT <= 0) return PSH_ERR_ARG;
    if (nT > PSH_RV_MAX_T) return PSH_ERR_UNSUPPORTED;
    if (n_rows == 0) return PSH_OK;
    GUARD_DEVICE(device);
    RvArgs a{};
    a.x = x; a.n_rows = n_rows; a.row_stride = row_stride; a.nT = nT; a.vol = vol ? 1 : 0; a.out = out;
    for (int i = 0; i < nT; ++i) {
        if (Ts[i] <= 0) return PSH_ERR_ARG;
        a.Ts[i] = Ts[i] < len ? Ts[i] : len;                 // numpy: x[..., :T] clips to the row
    }
    HIP_TRY(launch_realized_variance(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_weighted_quantiles(int device, void* stream, const float* values, const double* weights, int B, int k, int m,
                           const double* levels, int n_levels, double* out_q, double* out_lower, double* out_upper,
                           int32_t* out_status) {
    if (!values || !levels || !out_q || !out_lower || !out_upper || B <= 0 || k <= 0 || m <= 0 || n_levels <= 0 ||
        n_levels > PSH_QUANTILE_MAX_LEVELS)
        return PSH_ERR_ARG;
    QuantileArgs a{};
    for (int i = 0; i < n_levels; ++i) {
        if (!(levels[i] > 0.0 && levels[i] < 1.0)) return PSH_ERR_ARG;      // (NaN fails both)
        a.levels[i] = levels[i];
    }
    if (k > PSH_MAX_K || (int64_t)B * m >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;   // (one workgroup per column)
    a.values = values; a.weights = weights; a.B = B; a.k = k; a.m = m; a.n_levels = n_levels;
    a.q = out_q; a.lower = out_lower; a.upper = out_upper; a.status = out_status;
    GUARD_DEVICE(device);
    if (out_status) HIP_TRY(hipMemsetAsync(out_status, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream));
    HIP_TRY(launch_quantiles(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_score_ensemble(int device, void* stream, const float* values, const double* weights, const float* obs, int B, int k,
                       int m, int n_sets, double* out_crps, double* out_pit_lo, double* out_pit_hi, double* out_mean,
                       int32_t* out_status) {
    if (!values || !obs || !out_crps || !out_pit_lo || !out_pit_hi || !out_mean || B <= 0 || k <= 0 || m <= 0 || n_sets <= 0 ||
        n_sets > PSH_SCORE_MAX_SETS || (!weights && n_sets != 1))
        return PSH_ERR_ARG;
    if (k > PSH_MAX_K || (int64_t)B * m >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;   // (one workgroup per column)
    ScoreArgs a{};
    a.values = values; a.weights = weights; a.obs = obs; a.B = B; a.k = k; a.m = m; a.n_sets = n_sets;
    a.crps = out_crps; a.pit_lo = out_pit_lo; a.pit_hi = out_pit_hi; a.mean = out_mean; a.status = out_status;
    GUARD_DEVICE(device);
    if (out_status) HIP_TRY(hipMemsetAsync(out_status, 0, (size_t)n_sets * B * sizeof(int32_t), (hipStream_t)stream));
    HIP_TRY(launch_score(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_softmax_weights(int device, void* stream, const float* distances, int B, int k, const double* etas, int n_etas,
                        const int* ks, int n_ks, double* out_weights) {
    if (!distances || !etas || !out_weights || B <= 0 || k <= 0 || n_etas <= 0 || n_ks <= 0 ||
        (int64_t)n_etas * n_ks > PSH_SCORE_MAX_SETS)
        return PSH_ERR_ARG;
    WeightsArgs a{};
    for (int i = 0; i < n_etas; ++i) {
        if (!(etas[i] > 0.0)) return PSH_ERR_ARG;                           // (NaN fails it too)
        a.s[i] = 2.0 * (etas[i] * etas[i]);                                 // +infinity stays +infinity: uniform weights
    }
    for (int i = 0; i < n_ks; ++i) {
        const int kc = ks ? ks[i] : k;
        if (kc < 1 || kc > k || (!ks && n_ks != 1)) return PSH_ERR_ARG;
        a.ks[i] = kc;
    }
    if (k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;                          // (one workgroup per row)
    a.distances = distances; a.B = B; a.k = k; a.n_etas = n_etas; a.n_ks = n_ks; a.out = out_weights;
    GUARD_DEVICE(device);
    HIP_TRY(launch_softmax_weights(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_separate_topk(int device, void* stream, const float* d, const int32_t* idx, int B, int K, int k, int delta,
                      float* out_d, int32_t* out_idx, int32_t* out_pos, int32_t* out_count, int32_t* out_status) {
    if (!d || !idx || !out_d || !out_idx || !out_pos || !out_count || !out_status || B <= 0 || K <= 0 || k <= 0 || k > K ||
        delta < 0)
        return PSH_ERR_ARG;
    if (K > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;                          // (one workgroup per query, the list in LDS)
    SeparateArgs a{};
    a.d = d; a.idx = idx; a.B = B; a.K = K; a.k = k; a.delta = delta;
    a.out_d = out_d; a.out_idx = out_idx; a.out_pos = out_pos; a.out_count = out_count; a.out_status = out_status;
    GUARD_DEVICE(device);
    HIP_TRY(launch_separate(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_calibrate_workspace_bytes(int B, int k, int nT, size_t* out) {
    if (!out || B <= 0 || k <= 0 || nT <= 0) return PSH_ERR_ARG;
    if (k > PSH_MAX_K || nT > PSH_CAL_MAX_INSTRUMENTS) return PSH_ERR_UNSUPPORTED;
    *out = (size_t)B * (nT + 1) * k * sizeof(double);                      // the terminal prices; a_i / e_i of a trial
    return PSH_OK;
}

int psh_calibrate_weights(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                          const double* prior, double x_init, double rate, const int* Ts, int nT, const double* strike,
                          const double* target, int nM, int kind, int martingale, double eps, double tol, int max_iter,
                          double* out_weights, double* out_lambda, double* out_model, double* out_info, int32_t* out_status,
                          void* workspace, size_t workspace_bytes) {
    if (!dlnx || !Ts || !strike || !target || !out_weights || !out_lambda || !out_model || !out_info || !out_status ||
        !workspace || B <= 0 || k <= 0 || len <= 0 || row_stride < len || nT <= 0 || nM <= 0 || kind < PSH_HMC_OTM ||
        kind > PSH_HMC_PUT || !std::isfinite(x_init) || !(x_init > 0.0) || !std::isfinite(rate) || !(eps >= 0.0) ||
        !std::isfinite(eps) || !(tol > 0.0) || max_iter < 0)
        return PSH_ERR_ARG;
    for (int i = 0; i < nT; ++i)
        if (Ts[i] < 1 || Ts[i] > len) return PSH_ERR_ARG;
    const int64_t J = (int64_t)nT * nM + (martingale ? nT : 0);
    if (k > PSH_MAX_K || J > PSH_CAL_MAX_INSTRUMENTS) return PSH_ERR_UNSUPPORTED;
    if ((int64_t)B * k * row_stride >= ((int64_t)1 << 40) || (int64_t)B * ((k + 255) / 256) >= ((int64_t)1 << 31))
        return PSH_ERR_UNSUPPORTED;
    size_t need = 0;
    psh_calibrate_workspace_bytes(B, k, nT, &need);
    if (workspace_bytes < need) return PSH_ERR_WORKSPACE;
    CalArgs a{};
    a.x = dlnx; a.row_stride = row_stride; a.B = B; a.k = k; a.len = len; a.prior = prior; a.x_init = x_init;
    a.inv_x = 1.0 / x_init; a.eps = eps; a.tol = tol; a.max_iter = max_iter; a.nT = nT; a.nM = nM; a.kind = kind;
    a.J = (int)J;
    const double rho = rate / 252.0;
    for (int i = 0; i < nT; ++i) {
        a.Ts[i] = Ts[i];
        a.Tmax = std::max(a.Tmax, Ts[i]);
        a.disc[i] = std::exp(-(rho * (double)Ts[i]));
        a.fwd[i] = x_init * std::exp(rho * (double)Ts[i]);
    }
    a.strike = strike; a.target = target; a.w = out_weights; a.lam = out_lambda; a.model = out_model; a.info = out_info;
    a.status = out_status; a.st = (double*)workspace;
    GUARD_DEVICE(device);
    HIP_TRY(launch_calibrate(a, (hipStream_t)stream));
    return PSH_OK;
}

// what every hedged Monte Carlo entry point asks of the paths, the grid of maturities and strikes and the regression
static int hmc_check_sizes(const float* dlnx, int64_t row_stride, int B, int k, int len, double x_init, double rate, const int* Ts,
                           int nT, const double* Ms, int nM, int degree, int kind) {
    if (!dlnx || !Ts || !Ms || B <= 0 || k <= 0 || len <= 0 || row_stride < len || nT <= 0 || nM <= 0 || degree < 1 ||
        kind < PSH_HMC_OTM || kind > PSH_HMC_PUT || !std::isfinite(x_init) || !(x_init > 0.0) || !std::isfinite(rate))
        return PSH_ERR_ARG;
    if (degree > 5 || nT > PSH_HMC_MAX_T || nM > PSH_HMC_MAX_M) return PSH_ERR_UNSUPPORTED;
    return PSH_OK;
}

// ... and the checked copy of that grid into the launch arguments (HmcArgs, HedgeReplayArgs)
static int hmc_copy_grid(int* to_Ts, double* to_Ms, int len, const int* Ts, int nT, const double* Ms, int nM) {
    for (int i = 0; i < nT; ++i) {
        if (Ts[i] < 1 || Ts[i] > len) return PSH_ERR_ARG;
        to_Ts[i] = Ts[i];
    }
    for (int i = 0; i < nM; ++i) {
        if (!std::isfinite(Ms[i])) return PSH_ERR_ARG;
        to_Ms[i] = Ms[i];
    }
    return PSH_OK;
}

// the argument checks and the launch arguments that psh_hedged_mc and psh_hedged_mc_policy share
static int hmc_fill_args(HmcArgs& a, const float* dlnx, int64_t row_stride, int B, int k, int len, const double* weights,
                         double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM, int degree, int kind,
                         double* out_price, double* out_iv, double* out_strike, double* out_sigma, int32_t* out_status) {
    if (!out_price || !out_iv || !out_strike) return PSH_ERR_ARG;
    int rc = hmc_check_sizes(dlnx, row_stride, B, k, len, x_init, rate, Ts, nT, Ms, nM, degree, kind);
    if (rc != PSH_OK) return rc;
    if (k > PSH_MAX_K) return PSH_ERR_UNSUPPORTED;
    if ((int64_t)B * k * row_stride >= ((int64_t)1 << 40) || (int64_t)B * nT * ((nM + PSH_HMC_SG - 1) / PSH_HMC_SG) >= ((int64_t)1 << 31))
        return PSH_ERR_UNSUPPORTED;
    a.x = dlnx; a.row_stride = row_stride; a.B = B; a.k = k; a.len = len; a.w = weights; a.x_init = x_init; a.rate = rate;
    a.nT = nT; a.nM = nM; a.degree = degree; a.kind = kind; a.ngroups = (nM + PSH_HMC_SG - 1) / PSH_HMC_SG;
    rc = hmc_copy_grid(a.Ts, a.Ms, len, Ts, nT, Ms, nM);
    if (rc != PSH_OK) return rc;
    a.price = out_price; a.iv = out_iv; a.strike = out_strike; a.sigma = out_sigma; a.status = out_status;
    return PSH_OK;
}

int psh_hedged_mc(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                  const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                  int degree, int kind, double* out_price, double* out_iv, double* out_strike, double* out_sigma,
                  int32_t* out_status) {
    HmcArgs a{};
    const int rc = hmc_fill_args(a, dlnx, row_stride, B, k, len, weights, x_init, rate, Ts, nT, Ms, nM, degree, kind,
                                 out_price, out_iv, out_strike, out_sigma, out_status);
    if (rc != PSH_OK) return rc;
    GUARD_DEVICE(device);
    HIP_TRY(launch_hedged_mc(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_hmc_policy_doubles(int B, int nT, int nM, int Tmax, int degree, size_t* out) {
    if (!out || B <= 0 || nT <= 0 || nM <= 0 || Tmax <= 0 || degree < 1) return PSH_ERR_ARG;
    if (degree > 5 || nT > PSH_HMC_MAX_T || nM > PSH_HMC_MAX_M) return PSH_ERR_UNSUPPORTED;
    *out = (size_t)B * nT * nM * Tmax * (2 * degree + 4);
    return PSH_OK;
}

int psh_hedged_mc_policy(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                         const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                         int degree, int kind, double* out_price, double* out_iv, double* out_strike, double* out_sigma,
                         int32_t* out_status, double* out_policy) {
    if (!out_policy) return PSH_ERR_ARG;
    HmcArgs a{};
    const int rc = hmc_fill_args(a, dlnx, row_stride, B, k, len, weights, x_init, rate, Ts, nT, Ms, nM, degree, kind,
                                 out_price, out_iv, out_strike, out_sigma, out_status);
    if (rc != PSH_OK) return rc;
    GUARD_DEVICE(device);
    HIP_TRY(launch_hedged_mc_policy(a, out_policy, (hipStream_t)stream));
    return PSH_OK;
}

int psh_hedge_replay_workspace_bytes(int B, int k, int nT, int nM, size_t* out) {
    if (!out || B <= 0 || k <= 0 || nT <= 0 || nM <= 0) return PSH_ERR_ARG;
    if (nT > PSH_HMC_MAX_T || nM > PSH_HMC_MAX_M) return PSH_ERR_UNSUPPORTED;
    const size_t ntiles = ((size_t)k + PSH_HEDGE_TILE - 1) / PSH_HEDGE_TILE;
    *out = (size_t)B * nT * nM * ntiles * PSH_HEDGE_NPART * sizeof(double);
    return PSH_OK;
}

int psh_hedge_replay(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                     const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                     int degree, int kind, const double* policy, const double* strike, const double* centre,
                     double* out_sums, double* out_pnl, int32_t* out_status, void* workspace, size_t workspace_bytes) {
    if (!policy || !strike || !centre || !out_sums || !workspace) return PSH_ERR_ARG;
    int rc = hmc_check_sizes(dlnx, row_stride, B, k, len, x_init, rate, Ts, nT, Ms, nM, degree, kind);
    if (rc != PSH_OK) return rc;
    HedgeReplayArgs a{};
    a.ngroups = (nM + PSH_HMC_SG - 1) / PSH_HMC_SG;
    a.ntiles = (int)(((int64_t)k + PSH_HEDGE_TILE - 1) / PSH_HEDGE_TILE);
    if ((int64_t)B * k * row_stride >= ((int64_t)1 << 40) || (int64_t)B * nT * a.ngroups * a.ntiles >= ((int64_t)1 << 31))
        return PSH_ERR_UNSUPPORTED;
    rc = hmc_copy_grid(a.Ts, a.Ms, len, Ts, nT, Ms, nM);
    if (rc != PSH_OK) return rc;
    a.Tmax = *std::max_element(a.Ts, a.Ts + nT);
    if (hedge_replay_lds_bytes(a.Tmax, degree) > PSH_HEDGE_MAX_LDS) return PSH_ERR_UNSUPPORTED;   // (the policy rows sit in LDS)
    size_t need = 0;
    psh_hedge_replay_workspace_bytes(B, k, nT, nM, &need);
    if (workspace_bytes < need) return PSH_ERR_WORKSPACE;
    a.x = dlnx; a.row_stride = row_stride; a.B = B; a.k = k; a.len = len; a.w = weights; a.x_init = x_init; a.rate = rate;
    a.nT = nT; a.nM = nM; a.degree = degree; a.kind = kind;
    a.policy = policy; a.strike = strike; a.centre = centre; a.sums = out_sums; a.pnl = out_pnl; a.status = out_status;
    a.part = (double*)workspace;
    GUARD_DEVICE(device);
    HIP_TRY(launch_hedge_replay(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_pdv_generate(int device, void* stream, int B, int64_t S, int n_steps, const double* lams1, const double* lams2,
                     const double* decay1, const double* decay2, const double* thetas, const double* betas, int n_betas,
                     double S0, double sqrt_dt, double nu, const double* R10, const double* R20, const double* draws,
                     uint64_t seed, double* out_sigma, double* out_St, float* out_dlnx, double* out_draws,
                     double* out_dw) {
    if (!lams1 || !lams2 || !decay1 || !decay2 || !thetas || !betas || !R10 || !R20 || B < 1 || S < 1 || n_steps < 1 ||
        (n_betas != 3 && n_betas != 4) || !std::isfinite(nu) || nu < 0.0)
        return PSH_ERR_ARG;
    if (S > INT64_MAX / B || (int64_t)B * S > INT64_MAX / n_steps) return PSH_ERR_ARG;
    if ((int64_t)B * S >= ((int64_t)1 << 39)) return PSH_ERR_UNSUPPORTED;   // (the grid is B * S / 256 blocks)
    PdvArgs a{};
    a.n_paths = (int64_t)B * S; a.S = S; a.n = n_steps; a.n_betas = n_betas;
    for (int i = 0; i < 2; ++i) {
        a.lam1[i] = lams1[i]; a.lam2[i] = lams2[i]; a.decay1[i] = decay1[i]; a.decay2[i] = decay2[i];
        a.theta[i] = thetas[i];
    }
    for (int i = 0; i < n_betas; ++i) a.beta[i] = betas[i];
    a.S0 = S0; a.sqdt = sqrt_dt; a.nu = nu; a.nexp = nu > 0.0 ? -2.0 / nu : 0.0;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32);
    a.R10 = R10; a.R20 = R20; a.draws = draws;
    a.sigma = out_sigma; a.St = out_St; a.dlnx = out_dlnx; a.raw = out_draws; a.dw = out_dw;
    GUARD_DEVICE(device);
    HIP_TRY(launch_pdv(a, (hipStream_t)stream));
    return PSH_OK;
}

// what both generators ask of the ensemble's size, the noise and the increments' row stride; log2 of the FFT length
static int mrw_check_sizes(int64_t R, int n, double sigma, double c0, const float* out_dlnx, int64_t dlnx_row_stride, int* logM) {
    if (R < 1 || n < 2 || !std::isfinite(sigma) || sigma < 0.0 || !std::isfinite(c0) || (out_dlnx && dlnx_row_stride < n))
        return PSH_ERR_ARG;
    if (n > PSH_MRW_MAX_N || R >= ((int64_t)1 << 32)) return PSH_ERR_UNSUPPORTED;   // (the grid is R / 2 workgroups)
    if (out_dlnx && R > INT64_MAX / dlnx_row_stride) return PSH_ERR_ARG;
    *logM = 2;
    while ((1 << *logM) < 2 * n) ++*logM;
    return PSH_OK;
}

int psh_mrw_generate(int device, void* stream, int64_t R, int n, double sigma, const double* a_omega, const double* a_eps,
                     double c0, uint64_t seed, float* out_dlnx, int64_t dlnx_row_stride, double* out_lnx,
                     double* out_omega) {
    if (!a_omega) return PSH_ERR_ARG;
    MrwArgs a{};
    const int rc = mrw_check_sizes(R, n, sigma, c0, out_dlnx, dlnx_row_stride, &a.logM);
    if (rc != PSH_OK) return rc;
    a.R = R; a.n = n;
    a.sigma = sigma; a.c0 = c0; a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32);
    a.a_omega = a_omega; a.a_eps = a_eps;
    a.dlnx = out_dlnx; a.dlnx_stride = dlnx_row_stride; a.lnx = out_lnx; a.omega = out_omega;
    GUARD_DEVICE(device);
    HIP_TRY(launch_mrw(a, (hipStream_t)stream));
    return PSH_OK;
}

int psh_smrw_generate(int device, void* stream, int64_t R, int n, int m, double sigma, const double* a_omega,
                      const double* k_hat, double c0, double v, uint64_t seed, float* out_dlnx, int64_t dlnx_row_stride,
                      double* out_lnx, double* out_logvol) {
    if (!a_omega || !k_hat || m < 1 || !std::isfinite(v)) return PSH_ERR_ARG;
    SmrwArgs a{};
    const int rc = mrw_check_sizes(R, n, sigma, c0, out_dlnx, dlnx_row_stride, &a.logM);
    if (rc != PSH_OK) return rc;
    a.R = R; a.n = n; a.m = m;
    if (m > (1 << a.logM) - n) return PSH_ERR_ARG;           // the convolution would wrap
    a.sigma = sigma; a.cv = c0 + v; a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32);
    a.a_omega = a_omega; a.k_hat = (const double2*)k_hat;
    a.dlnx = out_dlnx; a.dlnx_stride = dlnx_row_stride; a.lnx = out_lnx; a.logvol = out_logvol;
    GUARD_DEVICE(device);
    HIP_TRY(launch_smrw(a, (hipStream_t)stream));
    return PSH_OK;
}

// the argument checks of both psh_lagged_moments entry points, and the plan (units, lags per lane) for the sizes
static int lagged_moments_plan(int64_t R, int m, int64_t G, MomentsLagArgs* a, size_t* bytes) {
    if (R < 1 || m < 0 || G < 1 || G > R) return PSH_ERR_ARG;
    if (m > PSH_MOMENTS_MAX_LAG || R >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;   // (g * R stays in int64)
    moments_lag_plan(R, G, m, a);
    const int64_t units = G * a->upg;
    if (units >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;                          // (one workgroup per unit)
    *bytes = (size_t)units * (4 * (size_t)(m + 1) * sizeof(double) + sizeof(int64_t));
    return PSH_OK;
}

int psh_lagged_moments_workspace_bytes(int64_t R, int m, int64_t G, size_t* out_bytes) {
    if (!out_bytes) return PSH_ERR_ARG;
    MomentsLagArgs a{};
    return lagged_moments_plan(R, m, G, &a, out_bytes);
}

int psh_lagged_moments(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int m, int64_t G,
                       double* out_sums, int64_t* out_rows_used, int32_t* out_status, void* workspace,
                       size_t workspace_bytes) {
    if (!x || !out_sums || !out_rows_used || !workspace || n < 1 || row_stride < n || m >= n) return PSH_ERR_ARG;
    MomentsLagArgs a{};
    size_t need = 0;
    const int rc = lagged_moments_plan(R, m, G, &a, &need);
    if (rc != PSH_OK) return rc;
    if (R > INT64_MAX / row_stride) return PSH_ERR_ARG;
    if (workspace_bytes < need) return PSH_ERR_WORKSPACE;
    a.x = x; a.R = R; a.stride = row_stride; a.G = G; a.n = n; a.m = m;
    a.partial = (double*)workspace;
    a.unit_rows = (int64_t*)(a.partial + G * a.upg * 4 * (int64_t)(m + 1));
    a.out = out_sums; a.rows_used = out_rows_used; a.status = out_status;
    GUARD_DEVICE(device);
    HIP_TRY(launch_lagged_moments(a, (hipStream_t)stream));
    return PSH_OK;
}

// what the scattering spectra and their gradient ask of the row length n, the scales J and the groups G; log2(n)
static int scattering_check_sizes(int64_t R, int n, int J, int64_t G, int* logn_out) {
    if (n < 8 || (n & (n - 1)) != 0 || R < 1 || J < 1 || G < 1 || G > R) return PSH_ERR_ARG;
    int logn = 3;
    while (logn < 30 && (1 << logn) < n) ++logn;
    if (J > logn - 2) return PSH_ERR_ARG;
    if (n > PSH_SCAT_MAX_N) return PSH_ERR_UNSUPPORTED;
    *logn_out = logn;
    return PSH_OK;
}

// the argument checks both psh_scattering_spectra entry points share, and the plan (units, outputs) for the sizes
static int scattering_spectra_plan(int64_t R, int J, int64_t G, ScatArgs* a, size_t* bytes) {
    if (R < 1 || J < 1 || G < 1 || G > R) return PSH_ERR_ARG;
    if (J > PSH_SCAT_MAX_J || R >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;        // (g * R stays in int64)
    scattering_plan(R, G, J, a);
    const int64_t units = G * a->upg;
    if (units >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;                          // (one workgroup per unit)
    *bytes = (size_t)units * ((size_t)a->nout * sizeof(double) + sizeof(int64_t));
    return PSH_OK;
}

int psh_scattering_spectra_workspace_bytes(int64_t R, int J, int64_t G, size_t* out_bytes) {
    if (!out_bytes) return PSH_ERR_ARG;
    ScatArgs a{};
    return scattering_spectra_plan(R, J, G, &a, out_bytes);
}

int psh_scattering_spectra(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int J,
                           const double* psi_hat, int64_t G, double* out_sums, int64_t* out_rows_used,
                           int32_t* out_status, void* workspace, size_t workspace_bytes) {
    if (!x || !psi_hat || !out_sums || !out_rows_used || !workspace || row_stride < n) return PSH_ERR_ARG;
    int logn = 0;
    int rc = scattering_check_sizes(R, n, J, G, &logn);
    if (rc != PSH_OK) return rc;
    ScatArgs a{};
    size_t need = 0;
    rc = scattering_spectra_plan(R, J, G, &a, &need);
    if (rc != PSH_OK) return rc;
    if (R > INT64_MAX / row_stride) return PSH_ERR_ARG;
    if (workspace_bytes < need) return PSH_ERR_WORKSPACE;
    a.x = x; a.R = R; a.stride = row_stride; a.G = G; a.n = n; a.logn = logn; a.J = J; a.psi = psi_hat;
    a.partial = (double*)workspace;
    a.unit_rows = (int64_t*)(a.partial + G * a.upg * (int64_t)a.nout);
    a.out = out_sums; a.rows_used = out_rows_used; a.status = out_status;
    GUARD_DEVICE(device);
    HIP_TRY(launch_scattering(a, (hipStream_t)stream));
    return PSH_OK;
}

// the argument checks both psh_scattering_vjp entry points share (the forward's), log2(n) and the workspace for the sizes
static int scattering_vjp_plan(int64_t R, int n, int J, int64_t G, int* logn_out, size_t* bytes) {
    const int rc = scattering_check_sizes(R, n, J, G, logn_out);
    if (rc != PSH_OK) return rc;
    if (R >= ((int64_t)1 << 31)) return PSH_ERR_UNSUPPORTED;                                // ((r + 1) * G stays in int64)
    *bytes = (size_t)scattering_grad_workgroups(R) * sizeof(int32_t);
    return PSH_OK;
}

int psh_scattering_vjp_workspace_bytes(int64_t R, int n, int J, int64_t G, size_t* out_bytes) {
    if (!out_bytes) return PSH_ERR_ARG;
    int logn = 0;
    return scattering_vjp_plan(R, n, J, G, &logn, out_bytes);
}

int psh_scattering_vjp(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int J,
                       const double* psi_hat, int64_t G, const double* cot, double* out_grad, int64_t grad_stride,
                       int32_t* out_status, void* workspace, size_t workspace_bytes) {
    if (!x || !psi_hat || !cot || !out_grad || !workspace || row_stride < n || grad_stride < n) return PSH_ERR_ARG;
    int logn = 0;
    size_t need = 0;
    const int rc = scattering_vjp_plan(R, n, J, G, &logn, &need);
    if (rc != PSH_OK) return rc;
    if (R > INT64_MAX / row_stride || R > INT64_MAX / grad_stride) return PSH_ERR_ARG;
    if (workspace_bytes < need) return PSH_ERR_WORKSPACE;
    ScatGradArgs a{};
    a.x = x; a.R = R; a.stride = row_stride; a.G = G; a.n = n; a.logn = logn; a.J = J;
    a.nout = 2 * J + J * (J + 1) + J * (J + 1) * (J + 2) / 3;
    a.wgs = scattering_grad_workgroups(R);
    a.psi = psi_hat; a.cot = cot; a.grad = out_grad; a.gstride = grad_stride;
    a.flags = (int32_t*)workspace; a.status = out_status;
    GUARD_DEVICE(device);
    HIP_TRY(launch_scattering_grad(a, (hipStream_t)stream));
    return PSH_OK;
}

}  // extern "C"
