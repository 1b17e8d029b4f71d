// psh_probe.hip -- TEST INFRASTRUCTURE ONLY: one thin kernel around each primitive of psh_wave.h, psh_sort_lds.h and
// psh_long.h (and fast_div of psh_device.h, unit_queue of psh_segment.h), so that tests/test_gpu_wave_primitives.py,
// tests/test_gpu_sort_primitives.py and tests/test_gpu_long_primitives.py can compare each of them, bit for bit, with the
// numpy twins of tests/_wave_twin.py and tests/_long_twin.py.
// Built by tests/_probe.py with the product's flags into tests/csrc/lib/libpsh_probe.so; nothing in shadowing_amd/ links
// or loads it and libpsh_hip.so exports none of its symbols.
//
// Every kernel here launches WHOLE waves only: the primitives assume 64 active lanes (the butterflies, the DPP row
// operations and the readlanes read lanes that must be live), so the launchers refuse a size that is no multiple of the
// block and no partial wave is ever tested.  Every launcher returns -1 for a shape it does not take, else the
// hipGetLastError() of its launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psh_device.h"
#include "psh_long.h"
#include "psh_segment.h"
#include "psh_sort_lds.h"
#include "psh_wave.h"

namespace psh {

namespace {

// ---------------------------------------------------------------------------------- wave reductions and scans
enum { W_SUM = 0, W_MIN = 1, W_MAX = 2, W_OR = 3, W_MINMAX = 4, W_SCAN = 5 };
enum { T_F32 = 0, T_F64 = 1, T_I32 = 2, T_U32 = 3 };

// lane i of wave w reads a[64 w + i] (and b[] for the hi of wave_minmax) and writes what the primitive returned to it
template <typename T, int OP>
__global__ __launch_bounds__(256) void wave_kernel(const T* a, const T* b, T* out, T* out2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const T v = a[i];
    if constexpr (OP == W_SUM) out[i] = wave_sum(v);
    else if constexpr (OP == W_MIN) out[i] = wave_min(v);
    else if constexpr (OP == W_MAX) out[i] = wave_max(v);
    else if constexpr (OP == W_OR) out[i] = wave_or(v);
    else if constexpr (OP == W_MINMAX) {
        T lo = v, hi = b[i];
        wave_minmax(lo, hi);
        out[i] = lo;
        out2[i] = hi;
    } else out[i] = wave_scan_inclusive(v, lane);
}

template <typename T, bool INTEGER>
hipError_t launch_wave(int op, const void* a, const void* b, void* out, void* out2, int64_t n, hipStream_t s) {
    const dim3 grid((unsigned)(n / 256)), block(256);
    const T *pa = (const T*)a, *pb = (const T*)b;
    T *po = (T*)out, *po2 = (T*)out2;
    switch (op) {
    case W_SUM: hipLaunchKernelGGL((wave_kernel<T, W_SUM>), grid, block, 0, s, pa, pb, po, po2); break;
    case W_MIN: hipLaunchKernelGGL((wave_kernel<T, W_MIN>), grid, block, 0, s, pa, pb, po, po2); break;
    case W_MAX: hipLaunchKernelGGL((wave_kernel<T, W_MAX>), grid, block, 0, s, pa, pb, po, po2); break;
    case W_OR:
        if constexpr (INTEGER) { hipLaunchKernelGGL((wave_kernel<T, W_OR>), grid, block, 0, s, pa, pb, po, po2); break; }
        else return hipErrorInvalidValue;
    case W_MINMAX: hipLaunchKernelGGL((wave_kernel<T, W_MINMAX>), grid, block, 0, s, pa, pb, po, po2); break;
    case W_SCAN: hipLaunchKernelGGL((wave_kernel<T, W_SCAN>), grid, block, 0, s, pa, pb, po, po2); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the DPP forms: 0 wave_max_nonneg, 1 wave_sum_dpp (float words), 2 wave_scan_inclusive_dpp, 3 wave_total_dpp (int words)
template <int OP>
__global__ __launch_bounds__(256) void dpp_kernel(const unsigned* a, unsigned* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned v = a[i];
    if constexpr (OP == 0) out[i] = __float_as_uint(wave_max_nonneg(__uint_as_float(v)));
    else if constexpr (OP == 1) out[i] = __float_as_uint(wave_sum_dpp(__uint_as_float(v)));
    else if constexpr (OP == 2) out[i] = (unsigned)wave_scan_inclusive_dpp((int)v);
    else out[i] = (unsigned)wave_total_dpp((int)v);
}

// ---------------------------------------------------------------------------------- the workgroup tree
// every thread of a block of 64 WAVES threads writes what block_reduce returned to it; TAIL: a second reduction of
// other data through the same red[] right behind the first -- nothing but block_reduce's own tail barrier separates them
template <typename T, typename Op, int WAVES, bool TAIL>
__global__ __launch_bounds__(WAVES * 64) void block_kernel(const T* a, const T* b, T* out, T* out2) {
    __shared__ T red[WAVES];
    const size_t i = (size_t)blockIdx.x * (WAVES * 64) + threadIdx.x;
    const T va = a[i], vb = b[i];
    const T r1 = block_reduce<WAVES, TAIL>(va, red, Op{});
    if constexpr (TAIL) {
        const T r2 = block_reduce<WAVES, TAIL>(vb, red, Op{});
        out2[i] = r2;
    }
    out[i] = r1;
}

template <typename T, typename Op, int WAVES>
hipError_t launch_block3(int tail, const T* a, const T* b, T* out, T* out2, int nblocks, hipStream_t s) {
    const dim3 grid((unsigned)nblocks), block(WAVES * 64);
    if (tail) hipLaunchKernelGGL((block_kernel<T, Op, WAVES, true>), grid, block, 0, s, a, b, out, out2);
    else hipLaunchKernelGGL((block_kernel<T, Op, WAVES, false>), grid, block, 0, s, a, b, out, out2);
    return hipGetLastError();
}
template <typename T, typename Op>
hipError_t launch_block2(int waves, int tail, const T* a, const T* b, T* out, T* out2, int nblocks, hipStream_t s) {
    switch (waves) {
    case 1: return launch_block3<T, Op, 1>(tail, a, b, out, out2, nblocks, s);
    case 2: return launch_block3<T, Op, 2>(tail, a, b, out, out2, nblocks, s);
    case 4: return launch_block3<T, Op, 4>(tail, a, b, out, out2, nblocks, s);
    case 8: return launch_block3<T, Op, 8>(tail, a, b, out, out2, nblocks, s);
    case 16: return launch_block3<T, Op, 16>(tail, a, b, out, out2, nblocks, s);
    default: return hipErrorInvalidValue;
    }
}
template <typename T>
hipError_t launch_block1(int op, int waves, int tail, const void* a, const void* b, void* out, void* out2, int nblocks, hipStream_t s) {
    const T *pa = (const T*)a, *pb = (const T*)b;
    T *po = (T*)out, *po2 = (T*)out2;
    switch (op) {
    case W_SUM: return launch_block2<T, WaveSum>(waves, tail, pa, pb, po, po2, nblocks, s);
    case W_MIN: return launch_block2<T, WaveMin>(waves, tail, pa, pb, po, po2, nblocks, s);
    case W_MAX: return launch_block2<T, WaveMax>(waves, tail, pa, pb, po, po2, nblocks, s);
    default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------- the rank search
// One block of 256 threads per histogram of 64 PER counters, kept in LDS as the callers keep theirs.  rank_bucket is
// documented for ONE wave of a larger block: each of the four waves calls it in turn.  Per (histogram, wave, rank) five
// words: the owner's RankBucket {bucket, before, count} (left as the host filled them when nobody owns the rank), the
// popcount of the ballot of the returned flag and the lane that returned true.  one_hist: every rank of the histogram is
// asked of ONE RankHist (the two-rank caller's form), else each of a fresh rank_bucket.
template <int PER>
__global__ __launch_bounds__(256) void rank_kernel(const unsigned* hists, const unsigned* ranks, int nranks, int one_hist, unsigned* out) {
    __shared__ unsigned hist[64 * PER];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned* h = hists + (size_t)blockIdx.x * (64 * PER);
    for (int c = tid; c < 64 * PER; c += 256) hist[c] = h[c];
    __syncthreads();
    const unsigned* rk = ranks + (size_t)blockIdx.x * nranks;
    unsigned* o = out + ((size_t)blockIdx.x * 4 + wave) * (size_t)nranks * 5;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
            const RankHist<PER> rh(hist, lane);
            for (int r = 0; r < nranks; ++r) {
                auto owner = [&](const RankBucket& rb) {
                    o[5 * r + 0] = (unsigned)rb.bucket;
                    o[5 * r + 1] = rb.before;
                    o[5 * r + 2] = rb.count;
                };
                const bool mine = one_hist ? rh.find(rk[r], owner) : rank_bucket<PER>(hist, lane, rk[r], owner);
                const unsigned long long m = __ballot(mine);
                if (lane == 0) {
                    o[5 * r + 3] = (unsigned)__popcll(m);
                    o[5 * r + 4] = m ? (unsigned)(__ffsll((long long)m) - 1) : 0xffffffffu;
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void edge_kernel(const unsigned* kmin, const unsigned* kmax, const int* bucket, const int* shift, unsigned* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    out[i] = bucket_upper_edge(kmin[i], kmax[i], bucket[i], shift[i]);
}

// ---------------------------------------------------------------------------------- keys, sort, scan
__global__ __launch_bounds__(64) void key_kernel(const unsigned* xbits, unsigned* key, unsigned* back) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint32_t k = qnt_key(__uint_as_float(xbits[i]));
    key[i] = k;
    back[i] = __float_as_uint(qnt_value(k));
}

// one block per input of n2 entries: stored at i + i / 16 as the callers store them, a barrier, qnt_sort, and read back
// through the same layout HERE (the test never sees the physical order)
template <int NB, int THREADS>
__global__ __launch_bounds__(THREADS) void sort_kernel(const uint64_t* in, uint64_t* out, int n2) {
    constexpr int CAP = (1 << NB) * THREADS;
    __shared__ uint64_t ent[CAP + CAP / 16];
    const int tid = (int)threadIdx.x;
    const uint64_t* src = in + (size_t)blockIdx.x * n2;
    uint64_t* dst = out + (size_t)blockIdx.x * n2;
    for (int j = tid; j < n2; j += THREADS) ent[qnt_phys(j)] = src[j];
    __syncthreads();
    qnt_sort<NB, THREADS>(ent, n2, tid);
    for (int j = tid; j < n2; j += THREADS) dst[j] = ent[qnt_phys(j)];
}

// two scans back to back on the same arrays, the second of other data: what each thread got back and the total it then
// read from g[GROUPS], as the callers read it
template <int THREADS, bool MAX>
__global__ __launch_bounds__(THREADS) void scan_kernel(const double* a, const double* b, double* pre1, double* tot1, double* pre2, double* tot2) {
    constexpr int RUNS = THREADS / PSH_QNT_RUN, GROUPS = RUNS / PSH_QNT_GRP;
    __shared__ double sc[THREADS], rc[RUNS], gc[GROUPS + 1];
    const int tid = (int)threadIdx.x;
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const double va = a[i], vb = b[i];
    const double p1 = qnt_scan<THREADS, MAX>(sc, rc, gc, va, tid);
    const double t1 = gc[GROUPS];
    const double p2 = qnt_scan<THREADS, MAX>(sc, rc, gc, vb, tid);
    const double t2 = gc[GROUPS];
    pre1[i] = p1;
    tot1[i] = t1;
    pre2[i] = p2;
    tot2[i] = t2;
}
template <int THREADS>
hipError_t launch_scan(int is_max, const double* a, const double* b, double* pre1, double* tot1, double* pre2, double* tot2, int nblocks, hipStream_t s) {
    const dim3 grid((unsigned)nblocks), block(THREADS);
    if (is_max) hipLaunchKernelGGL((scan_kernel<THREADS, true>), grid, block, 0, s, a, b, pre1, tot1, pre2, tot2);
    else hipLaunchKernelGGL((scan_kernel<THREADS, false>), grid, block, 0, s, a, b, pre1, tot1, pre2, tot2);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- divide and queue
__global__ __launch_bounds__(64) void fast_div_kernel(const unsigned* u, const unsigned* magic, const unsigned* d, unsigned* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    out[i] = fast_div(u[i], magic[i], d[i]);
}

// block b of the grid writes its share [lo, hi) of each of the nn unit counts
__global__ __launch_bounds__(64) void unit_queue_kernel(const unsigned* n, int nn, unsigned* lo, unsigned* hi) {
    __shared__ int next;
    if (threadIdx.x == 0) {
        for (int k = 0; k < nn; ++k) {
            const UnitQueue uq = unit_queue(n[k], &next);
            lo[(size_t)k * gridDim.x + blockIdx.x] = uq.lo;
            hi[(size_t)k * gridDim.x + blockIdx.x] = uq.hi;
        }
    }
}

// ---------------------------------------------------------------------------------- the long-window front end (psh_long.h)
// One WAVE per case, all cases of a piece in one launch: block c reads its PSH_PROBE_LONG_PARAMS ints at par + c * that.
#define PSH_PROBE_LONG_PARAMS 136
enum { L_STAGE0 = 0, L_STAGE2 = 1, L_OPERAND_LO = 2, L_OPERAND_HI = 3, L_TILE_MIN = 4, L_TABLES = 5, L_EXACT_SCALAR = 6,
       L_EXACT_VECTOR = 7, L_BOUND = 8, L_ZERO = 9 };

// par: {row, T, seg_start, nfloat}; out[c][4 (lane + 64 q) + i]: the staged words, all bits set where nothing is loaded
template <int AUX>
__global__ __launch_bounds__(64) void long_stage_kernel(const float* ds, const int* par, unsigned* out) {
    const int lane = (int)threadIdx.x;
    const int* p = par + (size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS;
    Stage st;
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q) st.v[q] = f32x4{__uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u)};
    long_stage_row<AUX>(st, ds, (int64_t)p[1], (int64_t)p[0], p[2], p[3], lane);
    unsigned* o = out + (size_t)blockIdx.x * (256 * PSH_NSTAGE);
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[4 * (lane + 64 * q) + i] = __float_as_uint(st.v[q][i]);
}
// in[c][PSH_LONG_SFLOATS]: prefix sums; par: {W}; out[c][16 lane + r]
template <bool UPPER>
__global__ __launch_bounds__(64) void long_operand_kernel(const float* in, const int* par, float* out) {
    const int lane = (int)threadIdx.x, m = lane & 31, hk = lane >> 5;
    const float* ps_lo = in + (size_t)blockIdx.x * PSH_LONG_SFLOATS + m + 128 * hk;
    const f32x16 ce = long_energy_operand<UPPER>(ps_lo, ps_lo + par[(size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS]);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[((size_t)blockIdx.x * 64 + lane) * 16 + r] = ce[r];
}
// in[c][16 lane + r]: a tile; par: {nvalid}; out[c][lane]
__global__ __launch_bounds__(64) void long_tile_min_kernel(const float* in, const int* par, float* out) {
    const int lane = (int)threadIdx.x;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = in[((size_t)blockIdx.x * 64 + lane) * 16 + r];
    out[(size_t)blockIdx.x * 64 + lane] = long_tile_min(c, par[(size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS], lane);
}
// in[c][3][256]: queries; par: {nks bucket, nq, W, scale bits}; out[c][3 * 3328] halves: the tables as the kernels hold them
#define PSH_PROBE_TAB_HALVES (3 * (lq_query_bytes(18) / 2))
__global__ __launch_bounds__(64) void long_tables_kernel(const float* in, const int* par, unsigned short* out) {
    __shared__ __attribute__((aligned(16))) float xs[3 * 256];
    __shared__ __attribute__((aligned(16))) _Float16 tab[PSH_PROBE_TAB_HALVES];
    const int lane = (int)threadIdx.x;
    const int* p = par + (size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS;
    const int nks = p[0], nq = p[1], W = p[2];
    const float scale = __uint_as_float((unsigned)p[3]);
    for (int e = lane; e < nq * W; e += 64) xs[e] = in[(size_t)blockIdx.x * 768 + e];
    for (int e = lane; e < PSH_PROBE_TAB_HALVES; e += 64) tab[e] = (_Float16)1.0f;          // what the call must overwrite
    wave_lds_fence();
    if (nks == 6) long_query_tables<6>(tab, xs, nq, W, scale, lane, 64);
    else if (nks == 10) long_query_tables<10>(tab, xs, nq, W, scale, lane, 64);
    else if (nks == 14) long_query_tables<14>(tab, xs, nq, W, scale, lane, 64);
    else long_query_tables<18>(tab, xs, nq, W, scale, lane, 64);
    wave_lds_fence();
    for (int e = lane; e < PSH_PROBE_TAB_HALVES; e += 64) out[(size_t)blockIdx.x * PSH_PROBE_TAB_HALVES + e] = reinterpret_cast<const unsigned short*>(tab)[e];
}
// y, x: float arrays; par: {W, qn, x offset (scalar kind), -, t[64] at 8, x offsets[64] at 72}; out[c][lane]: the chain, 0 past qn
template <bool VECTOR>
__global__ __launch_bounds__(64) void long_exact_kernel(const float* y, const float* x, const int* par, float* out) {
    const int lane = (int)threadIdx.x;
    const int* p = par + (size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS;
    const int W = p[0];
    float v = 0.0f;
    if (lane < p[1]) {
        if constexpr (VECTOR) v = long_exact_window(y + p[8 + lane], x + p[72 + lane], W);
        else v = long_exact_window(y + p[8 + lane], (const_f32p)x + p[2], W);
    }
    out[(size_t)blockIdx.x * 64 + lane] = v;
}
// est[c][lane], nx[c][lane]; par: {W, sexp}
__global__ __launch_bounds__(64) void long_bound_kernel(const float* est, const float* nx, const int* par, float* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int* p = par + (size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS;
    out[i] = long_upper_bound(est[i], nx[i], p[0], p[1]);
}
// par: {words}; out[c][1024]: a buffer of 1024 words, all bits set, after long_zero_rows(buffer, words, lane)
__global__ __launch_bounds__(64) void long_zero_kernel(const int* par, unsigned* out) {
    __shared__ __attribute__((aligned(16))) unsigned buf[1024];
    const int lane = (int)threadIdx.x;
    for (int e = lane; e < 1024; e += 64) buf[e] = ~0u;
    wave_lds_fence();
    long_zero_rows(reinterpret_cast<_Float16*>(buf), par[(size_t)blockIdx.x * PSH_PROBE_LONG_PARAMS], lane);
    wave_lds_fence();
    for (int e = lane; e < 1024; e += 64) out[(size_t)blockIdx.x * 1024 + e] = buf[e];
}

}  // namespace

}  // namespace psh

using namespace psh;

extern "C" {

int psh_probe_version(void) { return 2; }

// type: 0 float32, 1 float64, 2 int32, 3 uint32; op: 0 sum, 1 min, 2 max, 3 or (integers), 4 minmax (lo from a, hi from b,
// the maxima to out2), 5 wave_scan_inclusive; n lanes, whole blocks of 256
int psh_probe_wave(int type, int op, const void* a, const void* b, void* out, void* out2, int64_t n, void* stream) {
    if (n <= 0 || n % 256) return -1;
    hipStream_t s = (hipStream_t)stream;
    switch (type) {
    case T_F32: return (int)launch_wave<float, false>(op, a, b, out, out2, n, s);
    case T_F64: return (int)launch_wave<double, false>(op, a, b, out, out2, n, s);
    case T_I32: return (int)launch_wave<int, true>(op, a, b, out, out2, n, s);
    case T_U32: return (int)launch_wave<unsigned, true>(op, a, b, out, out2, n, s);
    default: return -1;
    }
}

// op: 0 wave_max_nonneg, 1 wave_sum_dpp, 2 wave_scan_inclusive_dpp, 3 wave_total_dpp; 32-bit words in and out
int psh_probe_dpp(int op, const void* a, void* out, int64_t n, void* stream) {
    if (n <= 0 || n % 256) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(n / 256)), block(256);
    const unsigned* pa = (const unsigned*)a;
    unsigned* po = (unsigned*)out;
    switch (op) {
    case 0: hipLaunchKernelGGL((dpp_kernel<0>), grid, block, 0, s, pa, po); break;
    case 1: hipLaunchKernelGGL((dpp_kernel<1>), grid, block, 0, s, pa, po); break;
    case 2: hipLaunchKernelGGL((dpp_kernel<2>), grid, block, 0, s, pa, po); break;
    case 3: hipLaunchKernelGGL((dpp_kernel<3>), grid, block, 0, s, pa, po); break;
    default: return -1;
    }
    return (int)hipGetLastError();
}

// type: 0 float32, 1 float64; op: 0 sum, 1 min, 2 max; nblocks blocks of 64 waves threads; tail: TAIL_BARRIER and a
// second reduction (of b, to out2) behind the first
int psh_probe_block_reduce(int type, int op, int waves, int tail, const void* a, const void* b, void* out, void* out2, int nblocks, void* stream) {
    if (nblocks <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (type == T_F32) return (int)launch_block1<float>(op, waves, tail, a, b, out, out2, nblocks, s);
    if (type == T_F64) return (int)launch_block1<double>(op, waves, tail, a, b, out, out2, nblocks, s);
    return -1;
}

// nhist histograms of 64 per counters, nranks ranks each; out: [nhist][4 waves][nranks][5] words, filled by the host
int psh_probe_rank(int per, const void* hists, int nhist, const void* ranks, int nranks, int one_hist, void* out, void* stream) {
    if (nhist <= 0 || nranks <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nhist), block(256);
    const unsigned *ph = (const unsigned*)hists, *pr = (const unsigned*)ranks;
    unsigned* po = (unsigned*)out;
    switch (per) {
    case 1: hipLaunchKernelGGL((rank_kernel<1>), grid, block, 0, s, ph, pr, nranks, one_hist, po); break;
    case 16: hipLaunchKernelGGL((rank_kernel<16>), grid, block, 0, s, ph, pr, nranks, one_hist, po); break;
    case 32: hipLaunchKernelGGL((rank_kernel<32>), grid, block, 0, s, ph, pr, nranks, one_hist, po); break;
    default: return -1;
    }
    return (int)hipGetLastError();
}

int psh_probe_bucket_edge(const void* kmin, const void* kmax, const void* bucket, const void* shift, void* out, int64_t n, void* stream) {
    if (n <= 0 || n % 64) return -1;
    hipLaunchKernelGGL(edge_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, (hipStream_t)stream, (const unsigned*)kmin,
                       (const unsigned*)kmax, (const int*)bucket, (const int*)shift, (unsigned*)out);
    return (int)hipGetLastError();
}

int psh_probe_key(const void* xbits, void* key, void* back, int64_t n, void* stream) {
    if (n <= 0 || n % 64) return -1;
    hipLaunchKernelGGL(key_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, (hipStream_t)stream, (const unsigned*)xbits,
                       (unsigned*)key, (unsigned*)back);
    return (int)hipGetLastError();
}

// nb: 2, 3, 4 -> qnt_sort<2, 256>, <3, 512>, <4, 1024>; ninputs inputs of n2 entries each, a power of two in [2^nb, capacity]
int psh_probe_sort(int nb, const void* in, void* out, int n2, int ninputs, void* stream) {
    if (ninputs <= 0 || n2 <= 0 || (n2 & (n2 - 1))) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ninputs);
    const uint64_t* pi = (const uint64_t*)in;
    uint64_t* po = (uint64_t*)out;
    if (nb == 2 && n2 >= 4 && n2 <= 1024) hipLaunchKernelGGL((sort_kernel<2, 256>), grid, dim3(256), 0, s, pi, po, n2);
    else if (nb == 3 && n2 >= 8 && n2 <= 4096) hipLaunchKernelGGL((sort_kernel<3, 512>), grid, dim3(512), 0, s, pi, po, n2);
    else if (nb == 4 && n2 >= 16 && n2 <= 16384) hipLaunchKernelGGL((sort_kernel<4, 1024>), grid, dim3(1024), 0, s, pi, po, n2);
    else return -1;
    return (int)hipGetLastError();
}

// threads: 256, 512, 1024; nblocks blocks, one double per thread in a (first scan) and b (second scan)
int psh_probe_scan(int threads, int is_max, const void* a, const void* b, void* pre1, void* tot1, void* pre2, void* tot2, int nblocks, void* stream) {
    if (nblocks <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const double *pa = (const double*)a, *pb = (const double*)b;
    double *p1 = (double*)pre1, *t1 = (double*)tot1, *p2 = (double*)pre2, *t2 = (double*)tot2;
    if (threads == 256) return (int)launch_scan<256>(is_max, pa, pb, p1, t1, p2, t2, nblocks, s);
    if (threads == 512) return (int)launch_scan<512>(is_max, pa, pb, p1, t1, p2, t2, nblocks, s);
    if (threads == 1024) return (int)launch_scan<1024>(is_max, pa, pb, p1, t1, p2, t2, nblocks, s);
    return -1;
}

int psh_probe_fast_div(const void* u, const void* magic, const void* d, void* out, int64_t n, void* stream) {
    if (n <= 0 || n % 64) return -1;
    hipLaunchKernelGGL(fast_div_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, (hipStream_t)stream, (const unsigned*)u,
                       (const unsigned*)magic, (const unsigned*)d, (unsigned*)out);
    return (int)hipGetLastError();
}

// a grid of `grid` blocks; lo, hi: [nn][grid] words
int psh_probe_unit_queue(const void* n, int nn, void* lo, void* hi, int grid, void* stream) {
    if (nn <= 0 || grid <= 0) return -1;
    hipLaunchKernelGGL(unit_queue_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, (const unsigned*)n, nn,
                       (unsigned*)lo, (unsigned*)hi);
    return (int)hipGetLastError();
}

// the pieces of psh_long.h, one wave per case: what = 0 / 1 long_stage_row<0> / <2> (a = the ensemble), 2 / 3
// long_energy_operand<false> / <true> (a = prefix sums), 4 long_tile_min (a = tiles), 5 long_query_tables (a = queries),
// 6 / 7 long_exact_window with a scalar / a per-lane query pointer (a = y, b = x), 8 long_upper_bound (a = est, b = nx),
// 9 long_zero_rows; par: ncases x 136 ints, laid out as the kernels above say
int psh_probe_long(int what, const void* a, const void* b, const void* par, void* out, int ncases, void* stream) {
    if (ncases <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ncases), block(64);
    const float *fa = (const float*)a, *fb = (const float*)b;
    const int* p = (const int*)par;
    switch (what) {
    case L_STAGE0: hipLaunchKernelGGL((long_stage_kernel<0>), grid, block, 0, s, fa, p, (unsigned*)out); break;
    case L_STAGE2: hipLaunchKernelGGL((long_stage_kernel<2>), grid, block, 0, s, fa, p, (unsigned*)out); break;
    case L_OPERAND_LO: hipLaunchKernelGGL((long_operand_kernel<false>), grid, block, 0, s, fa, p, (float*)out); break;
    case L_OPERAND_HI: hipLaunchKernelGGL((long_operand_kernel<true>), grid, block, 0, s, fa, p, (float*)out); break;
    case L_TILE_MIN: hipLaunchKernelGGL(long_tile_min_kernel, grid, block, 0, s, fa, p, (float*)out); break;
    case L_TABLES: hipLaunchKernelGGL(long_tables_kernel, grid, block, 0, s, fa, p, (unsigned short*)out); break;
    case L_EXACT_SCALAR: hipLaunchKernelGGL((long_exact_kernel<false>), grid, block, 0, s, fa, fb, p, (float*)out); break;
    case L_EXACT_VECTOR: hipLaunchKernelGGL((long_exact_kernel<true>), grid, block, 0, s, fa, fb, p, (float*)out); break;
    case L_BOUND: hipLaunchKernelGGL(long_bound_kernel, grid, block, 0, s, fa, fb, p, (float*)out); break;
    case L_ZERO: hipLaunchKernelGGL(long_zero_kernel, grid, block, 0, s, p, (unsigned*)out); break;
    default: return -1;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
