// psh_stream_copy.hip -- a resident f16 copy of the ensemble and the one-query overlap scan that streams it (gfx950).
// Part of libpsh_hip.so: psh_filter_copy_build and psh_scan_topk_copy (psh_capi.hip) launch what is here.
//
// Why.  stream_scan_kernel (psh_stream.hip) reads the ensemble at the rate a copy kernel reaches; what its rejection test
// consumes are f16 values, made from the fp32 samples again on every call.  An ensemble that stays where it is for thousands of
// calls (predict() loops over query dates, shadow_async keeps it resident) can be converted ONCE: the scan then streams two
// bytes a sample, and only the windows that survive the test -- about 1e-4 of them -- fetch their fp32 samples for the exact
// chain, from the ensemble itself.  Results are what the fp32 route gives: the test only ever decides which windows are looked
// at exactly.
//
// The copy.  A 64-byte header (CopyHdr), then R rows of `pitch` halves, pitch = T rounded up to whole segments + 32: every
// segment's PSH_SEG + 32 halves lie inside its row, the tail of a row is zero.  A value is  c = (f16)(y 2^e_c), rounded to
// nearest even, with ONE exponent e_c for the ensemble: the one that puts the rms of its finite samples into [0.5, 1) (f16
// then reaches 65504 rms upwards and 6e-5 rms downwards before it loses bits).  A product that leaves f16's range, and a
// sample that is not finite, is stored as a NaN: a window that holds one survives the test (NaN-safe compare) whatever the
// step's scale -- a stored +-inf scaled down below would reject windows the step's smaller scale cannot speak for.
// e_c is computed on the device (sum of squares as per-block partial sums in double, added in a fixed order by a second
// launch: no floating-point atomics) and stays there: the host never reads it, enqueueing never synchronises.
//
// The scale of a step.  stream_sample_finish chooses min(the exponent the query's proof allows, e_c) when FusedArgs::copy_ec is
// set; the scan multiplies the copy's values by 2^delta, delta = that exponent - e_c <= 0, with packed f16 multiplies: exact
// unless the result is an f16 subnormal.
//
// The bound (the fp32 route's derivation: psh_scan.hip, above scan_mx_kernel; same notation).  u = 2^-11, eta = 2^-25 (half
// the smallest f16 subnormal); y~ = 2^s y and x~ = 2^s x are the real scaled values, s the step's exponent.
//   y^ = fl16(fl16(y 2^e_c) 2^delta) = y~ (1 + e1) + d,         |e1| <= u, |d| <= 2 eta   (the build's rounding, the multiply's)
//   (y^2)^ = fl16(y^ y^)             = y^ y^ (1 + e3) + d3,     |e3| <= u, |d3| <= eta    (ONE rounding of the exact product)
//   energies:     y^ y^ = y~^2 (1 + e1)^2 + 2 y~ (1 + e1) d + d^2, and 2 |y~| (1 + u) 2 eta <= rho y~^2 + 4 eta^2 (1 + u)^2 / rho, so
//                 |(y^2)^ - y~^2| <= ((1 + u)^3 - 1 + rho (1 + u)) y~^2 + eta + 4 eta^2 (2 + 1 / rho)      per tap
//   correlation:  x^ = x~ (1 + ex) + dx, |ex| <= u, |dx| <= eta (2 |y^| eta <= rho y^2 + eta^2 / rho: another rho of the relative part),
//                 2 |x^ y^ - x~ y~| <= (2 u + u^2) 2 |x~ y~| + 2 |x^| 2 eta <= (2 u + u^2)(x~^2 + y~^2) + rho x~^2 (1 + u)^2 + 4 eta^2 / rho
//   accumulation: <= 128 fp32 additions of exact products, |terms| summing to <= 2 (nx~ + ny~)(1 + 3 u):  2^-15 (nx~ + ny~)
// With rho = 2^-14 the relative parts add up to (3.003 + 2.001 + 0.0625 + 0.375) u = 5.44 u (nx~ + ny~) and the absolute ones to
// W (eta + 2^-33) <= 33 x 2^-25 (1 + 2^-8) < 2^-19.9.  The copy route's pair is
//     a = 1 / 320 = 6.4 u   (the fp32 route: 4 u),     b = 2^-17 (W <= 31; (2 W + 2) / 64 of it beyond)
// -- PSH_COPY_A, PSH_COPY_B in psh_segment.h, used by stream_threshold_of --: a seventh of `a` and a factor of seven of `b` are
// spare.  The rest of the argument is unchanged: ny~ <= 2 (acc~ + nx~), so a window with t^ > tau~ (1 + 2^-17)(1 + 2 a) -
// nx~ (1 - 3 a) + b has a real acc above the level and is skipped.  b no longer sits under a scale that is maximal for the
// query (the step's exponent may be e_c < what the proof allows): tau~ is then smaller against b and fewer windows are
// rejected -- never a wrong one.  tests/test_filter_copy_bound_cpu.py emulates this chain in numpy float16.
//
// Survivors.  A window the test keeps goes to the wave's queue (row, t: 8 bytes, in the wave's fp32 tile) and the queue is
// verified when it is full and when the wave has no unit left (stream_scan_long_kernel's deferred survivors): a lane a window,
// its W fp32 samples from the ENSEMBLE in memory, the exact chain in the reference's order -- a handful of windows in a wave's
// life on ordinary data, one round trip at its end instead of a stall in one segment out of four.  A segment with more
// than PSH_COPY_DENSE = 16 survivors (1/64 of its windows) is staged as fp32 into the wave's LDS tile once and its chains run
// from there, as stream_scan_kernel's do.  The crossover: a deferred survivor fetches W fp32 samples at any 4-byte offset (80 -
// 132 bytes: 1.6 - 2 lines of 128 bytes) and, for the audit below, W halves of the copy (1.3 - 1.5 lines): 3 - 3.5 lines;
// the segment's tile is 4.2 KB = 33 lines, so ten survivors fetch what the tile does -- but the tile is a round trip in the
// middle of the wave's stream where the queue is one for 64 windows at once, so the switch sits above that: 16.  A smooth
// ensemble or a query much quieter than the data, where most windows survive, then costs about the fp32 scan plus the f16
// read and not an unbounded gather.
//
// The audit.  Every survivor has its fp32 samples at hand: (f16)(y 2^e_c) is computed again and compared bit for bit with
// what the copy holds (its halves from memory, deferred or staged alike: the segment was just streamed, the lines are in L2).  A
// mismatch -- the copy is of other data than the ensemble -- sets StreamCtl::ovf: the ranking reports PSH_STATUS_RETRY and the
// caller reruns through the separate launches and drops the copy.  Only survivors are audited: a copy of another ensemble is
// caught at once, a sparse edit the caller hid from the copy's owner may not be.
#include "psh_launch.h"
#include "psh_segment.h"

namespace psh {

#define PSH_COPY_DENSE 16             // survivors of a segment above which its fp32 tile is staged (see above)
#define PSH_COPY_QCAP 64              // deferred survivors a wave keeps (8-byte entries at the start of its fp32 tile)
#define PSH_COPY_NAN 0x7e00u

// a sample as the copy holds it: (f16)(y sc), round to nearest even; what is not a finite f16 is the quiet NaN.
// The compiler makes ONE instruction of the product and the conversion, a mixed-precision fma, and gives `(_Float16)(y * sc)`
// the addend +0: -0 sc + 0 is +0, so a sample of -0 was stored as 0x0000 where the format says 0x8000
// (tests/test_gpu_filter_copy_bytes.py).  The addend is therefore spelled out as -0, which keeps every product's value and
// sign (sc is a power of two: the product is exact, the one rounding is the conversion's), and handed over through an empty
// asm statement: a -0 the compiler can see is folded away and the +0 comes back.
__device__ __forceinline__ unsigned short copy_encode(float y, float sc) {
    float nz = -0.0f;
    asm("" : "+s"(nz));
    const _Float16 h = (_Float16)__builtin_fmaf(y, sc, nz);
    const unsigned short b = __builtin_bit_cast(unsigned short, h);
    return (b & 0x7c00u) == 0x7c00u ? (unsigned short)PSH_COPY_NAN : b;
}

// ------------------------------------------------------------------------------------------------------------------
// the build: sum of squares -> e_c -> the rows
// ------------------------------------------------------------------------------------------------------------------
// pass 1: the finite samples' squares, a double and a count per block, every block's own sum in a fixed order
__global__ __launch_bounds__(256) void copy_sumsq_kernel(const float* __restrict__ ds, long long n, double* part, unsigned long long* cnt) {
    __shared__ double sh_s[256];
    __shared__ unsigned long long sh_c[256];
    double s = 0.0;
    unsigned long long c = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = ds[i];
        if (fabsf(v) < __uint_as_float(PSH_INF_BITS)) { s += (double)v * (double)v; ++c; }
    }
    sh_s[threadIdx.x] = s;
    sh_c[threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh_s[threadIdx.x] += sh_s[threadIdx.x + off]; sh_c[threadIdx.x] += sh_c[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x] = sh_s[0]; cnt[blockIdx.x] = sh_c[0]; }
}
// the partial sums in a fixed order, the exponent, the header (one block)
__global__ __launch_bounds__(256) void copy_exponent_kernel(const double* part, const unsigned long long* cnt, int nblk, CopyHdr* hdr,
                                                            long long R, long long T, long long pitch) {
    __shared__ double sh_s[256];
    __shared__ unsigned long long sh_c[256];
    double s = 0.0;
    unsigned long long c = 0ull;
    for (int i = (int)threadIdx.x; i < nblk; i += 256) { s += part[i]; c += cnt[i]; }
    sh_s[threadIdx.x] = s;
    sh_c[threadIdx.x] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh_s[threadIdx.x] += sh_s[threadIdx.x + off]; sh_c[threadIdx.x] += sh_c[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int ec = 0;
        const double ms = sh_c[0] ? sh_s[0] / (double)sh_c[0] : 0.0;
        if (ms > 0.0 && ms < 1.0e300) {
            // rms = m 2^ex, m in [0.5, 1)  ->  e_c = -ex (kept inside what the step's scale may be: stream_sexp_of's +-60)
            int ex = 0;
            (void)frexp(sqrt(ms), &ex);
            ec = -ex;
            ec = ec < -60 ? -60 : (ec > 60 ? 60 : ec);
        }
        hdr->magic = PSH_COPY_MAGIC;
        hdr->e_c = ec;
        hdr->R = R; hdr->T = T; hdr->pitch = pitch;
        for (int i = 0; i < 8; ++i) hdr->pad[i] = 0u;
    }
}
// pass 2: a thread writes 8 halves (16 bytes); beyond T a row holds zeros
__global__ __launch_bounds__(256) void copy_write_kernel(const float* __restrict__ ds, long long R, long long T, long long pitch,
                                                         const CopyHdr* hdr, unsigned short* rows) {
    const int ec = hdr->e_c;
    const float sc = __uint_as_float((unsigned)(127 + ec) << 23);
    const long long per_row = pitch >> 3, n = R * per_row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / per_row, t0 = (i - r * per_row) << 3;
        const float* y = ds + r * T;
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned lo = t0 + 2 * e < T ? copy_encode(y[t0 + 2 * e], sc) : 0u;
            const unsigned hi = t0 + 2 * e + 1 < T ? copy_encode(y[t0 + 2 * e + 1], sc) : 0u;
            w[e] = lo | (hi << 16);
        }
        *reinterpret_cast<u32x4v*>(rows + r * pitch + t0) = u32x4v{w[0], w[1], w[2], w[3]};
    }
}

hipError_t launch_filter_copy_build(const float* ds, long long R, long long T, void* out, void* scratch, hipStream_t s) {
    const long long pitch = filter_copy_pitch(T);
    double* part = reinterpret_cast<double*>(scratch);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(part + PSH_COPY_BUILD_BLOCKS);
    CopyHdr* hdr = reinterpret_cast<CopyHdr*>(out);
    unsigned short* rows = reinterpret_cast<unsigned short*>(hdr + 1);
    const long long n = R * T;
    long long g1 = (n + 255) / 256;
    if (g1 > PSH_COPY_BUILD_BLOCKS) g1 = PSH_COPY_BUILD_BLOCKS;
    hipLaunchKernelGGL(copy_sumsq_kernel, dim3((unsigned)g1), dim3(256), 0, s, ds, n, part, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(copy_exponent_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const unsigned long long*)cnt, (int)g1, hdr, R, T, pitch);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    long long g2 = (R * (pitch >> 3) + 255) / 256;
    if (g2 > 8192) g2 = 8192;
    hipLaunchKernelGGL(copy_write_kernel, dim3((unsigned)g2), dim3(256), 0, s, ds, R, T, pitch, (const CopyHdr*)hdr, rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// S on the copy: stream_scan_kernel's place in the three launches (one query, W <= 33)
// ------------------------------------------------------------------------------------------------------------------
struct CStage {  // one unit in flight: its four A fragments, 4 x 16 bytes per lane (two sets per wave: 32 registers)
    u32x4v v[4];
};
enum { CS_FRONT = 0, CS_NEXT = 1 };

// Fragments from memory.  The copy's halves lie in memory exactly as an A fragment of the banded product wants them: row m of A
// is the 64 halves [32 m, 32 m + 64) of the segment, and lane (m = lane & 31, hk = lane >> 5) holds, for K-step s, the eight
// halves [32 m + 16 s + 8 hk, + 8) -- ONE 16-byte load (see `load`).  A unit is therefore four loads per lane, scaled by 2^delta
// and squared with packed f16 multiplies in registers: nothing of a segment passes through LDS.  (Until this was so the
// halves were staged as 16-byte pieces and written, with their squares, into two f16 arrays per wave, read back as fragments:
// 6 ds_write_b128 + 8 ds_read_b128 a unit beside the 8 for the B fragments, 42 % of the launch's cycles with the LDS array
// busy -- profiles/copy_scan_fragments.txt.)
// The halves beyond the segment's last window.  Row 31 of A ends at half seg_start + 1055; the segment's windows end at
// seg_start + PSH_SEG + W - 2.  The 33 - W halves in between are real halves of the row now -- the next segment's first
// samples, or the row's zero tail (the staged arrays held zeros there).  They only meet zero taps of B: finite values add exact
// zeros and every sum is what it was.  A NaN there (a non-finite sample, or one out of f16's range), and a value whose square
// overflows f16 (inf x 0), poisons the accumulators of windows 992 .. 1023 of the segment: the NaN-safe compare KEEPS those
// windows, the exact fp32 chain decides them, and no result changes -- every difference runs towards keeping
// (tests/test_gpu_copy_scan_fragments.py).
// The loads carry no cache hint.  The four loads of a unit ask for every 128-byte line of the segment from four instructions in
// a row (a lane's 16 bytes are 64 bytes from its neighbour's): the vector L1 merges them while the line is in flight, and the L2
// sees FEWER requests than from the pieces (2.14 M a launch against 2.41 M, FETCH_SIZE unchanged).  With the non-temporal hint
// the piece loads had, the L1 keeps no line: 8.7 M requests and 29 % more bytes fetched, 101 us a step against 66; the hint on
// some of the four, and K-steps 2 and 3 taken from lane m + 1 by DPP instead of loaded, all measured slower than four plain loads.
// The LDS of a block: 64 control words, the block's list, a 4.5 KB fp32 tile per wave and 8 KB for the eight B fragments (band of
// ones, shifted query), block-shared and read per use -- 8 ds_read_b128 a unit, all the LDS traffic a unit has left; with them in
// registers two stage sets spill at 112.  81 KB, where stream_scan_kernel takes 146.  The tile holds the wave's queue of deferred
// survivors; a dense segment's fp32 samples take it over (the queue is verified first).  At most 112 registers, like the scan
// it replaces: a sample or ranking wave of another stream's step still fits beside four of these on a SIMD.
// Stage sets: a wave owns TWO (32 registers): while one unit is scaled, squared and its set reloaded, the other's is in flight.
// Measured (profiles/copy_scan_fragments.txt): 51.6 us a step (51.4 - 51.7) against the staged halves' 66.0 (65.5 - 66.1), every run
// faster than the fastest of those; a launch alone on the chip 51.1 us against 65.8 = 5.3 TB/s of the 6.29 a copy kernel reaches,
// consecutive steps' scans start 50.2 us apart; the LDS array is busy 13.7 % of the launch's cycles (42.5 %); the same bytes
// (FETCH_SIZE 132935 KiB a launch) and exactly the same windows kept.
// The sets take turns in a loop body spelled out twice, every load unconditional: see the loop.
template <int WT>
__global__ __launch_bounds__(PSH_SCAN_THREADS) __attribute__((amdgpu_num_vgpr(56))) void copy_scan_kernel(ScanArgs a, FusedArgs f, CopyArgs cp) {
    static_assert(WT >= 0 && WT <= 33, "the shifted-query band must fit K = 64 (WT = 0: run-time W <= 33)");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = PSH_SCAN_THREADS / 64;
    constexpr int NFL = PSH_FUSED_FRONT;
    // (the lane from the execution mask, not from the thread index: nothing keeps the index register alive across the loop)
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool first = wave == 0 && lane == 0;
    int* ctl = reinterpret_cast<int*>(smem);                                 // 64 control words
    u32x4* fl = reinterpret_cast<u32x4*>(ctl + 64);                           // NFL entries {acc bits, r, t, query}
    float* tiles = reinterpret_cast<float*>(fl + NFL);
    float* tile = tiles + (size_t)wave * a.tile_floats;
    u64* sq = reinterpret_cast<u64*>(tile);                                   // deferred survivors: row | t << 32
    _Float16* bol = reinterpret_cast<_Float16*>(tiles + (size_t)NW * a.tile_floats);   // the band of ones' four fragments, block-shared (4 KB)
    FusedHdr* hdr = f.hdr;
    const StreamCtl* sc = &hdr->stream;

    const int W = WT > 0 ? WT : a.W;
    const int nhalf = PSH_SEG + W - 1;
    const UnitQueue uq = unit_queue((unsigned)a.n_rows * (unsigned)a.nseg, &ctl[CS_NEXT]);
    // The A fragment of K-step s for lane (m = lane & 31, hk = lane >> 5) is the eight halves [32 m + 16 s + 8 hk, + 8) of the
    // segment (mx_load_a's rule): in the copy ONE 16-byte aligned load -- the header is 64 bytes, the pitch a multiple of 32 halves,
    // a segment starts at a multiple of 1024 -- and the highest half touched, seg_start + 1055, lies inside the row (the pitch).
    // A unit's four loads are issued whatever the unit: one past the block's share reads the copy's header instead, every lane at
    // offset 0 -- straight-line code, so that the wait in front of a stage set's use counts exactly the loads of the OTHER set
    // that may stay in flight (behind a branch it would wait for all of them)
    const int frag0 = 32 * (lane & 31) + 8 * (lane >> 5);
    auto load = [&](CStage& st, unsigned uu) __attribute__((always_inline)) {
        const bool on = uu < uq.hi;
        const Unit c = unit_decode(a, on ? uu : uq.lo);
        const unsigned short* src = on ? cp.rows + c.row(a) * cp.pitch + c.seg_start() + frag0
                                       : reinterpret_cast<const unsigned short*>(cp.hdr);
#pragma unroll
        for (int s = 0; s < 4; ++s) st.v[s] = *reinterpret_cast<const u32x4v*>(src + (on ? 16 * s : 0));
    };
    // the first two units of every wave are requested before anything else (static; the queue starts behind them)
    CStage s0, s1;
    unsigned u0 = uq.lo + (unsigned)wave, u1 = u0 + NW;
    load(s0, u0);
    load(s1, u1);
    // what the sample kernel left (an earlier launch on this stream: plain loads)
    _Float16* bxl = bol + 4 * 64 * 8;                                         // ... and the shifted query's, behind them
    if (wave == 1) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            *reinterpret_cast<f16x8*>(bxl + (size_t)(s * 64 + lane) * 8) = *reinterpret_cast<const f16x8*>(hdr->bxtab + (size_t)(s * 64 + lane) * 8);
    }
    const unsigned armed_w = sc->armed;
    const unsigned scale_bits = sc->scale_bits;
    const float tau2 = __uint_as_float(sc->tau2_bits[0]), thr2 = __uint_as_float(sc->thr2_bits[0]), xn = __uint_as_float(sc->xn_bits[0]);
    // the copy's own word: a header the build never wrote, or one of another shape, is no copy of this ensemble
    const bool hdr_ok = cp.hdr->magic == PSH_COPY_MAGIC && cp.hdr->R == (long long)a.n_rows && cp.hdr->T == (long long)a.T && cp.hdr->pitch == cp.pitch;
    int ec = cp.hdr->e_c;
    ec = ec < -60 ? -60 : (ec > 60 ? 60 : ec);
    if (first) { ctl[CS_FRONT] = 0; ctl[CS_NEXT] = 2 * NW; }
    if (wave == 0) {                                                          // (window energies: arithmetic only)
        f16x8 bo[4];
        mx_band_ones(bo, W, lane);
#pragma unroll
        for (int s = 0; s < 4; ++s) *reinterpret_cast<f16x8*>(bol + (size_t)(s * 64 + lane) * 8) = bo[s];
    }
    const _Float16* bop = bol + (size_t)lane * 8;
    __syncthreads();
    if (armed_w == 0u) return;                                                // uniform: the ranking reports PSH_STATUS_RETRY
    if (!hdr_ok) {
        if (first) store_sc1(const_cast<unsigned*>(&sc->ovf), 1u);
        return;
    }
    // 2^delta as a half (delta = the step's exponent - e_c in [-14, 0]; below that the sample has switched the test off) and
    // 2^e_c as a float (the audit)
    int delta = (int)((scale_bits >> 23) & 255u) - 127 - ec;
    delta = delta > 0 ? 0 : (delta < -14 ? -14 : delta);
    const _Float16 hd = __builtin_bit_cast(_Float16, (unsigned short)((15 + delta) << 10));
    const float sc_c = __uint_as_float((unsigned)(127 + ec) << 23);
    const const_f32p x = (const_f32p)a.queries;
    const int Wr = a.W;                                                       // the survivors' loops take the run-time length: compact code, and no
                                                                              // query sample is kept in a scalar register across the unit loop
    // the audit's verdict: a lane that met a value the copy does not hold raises the step's give-up word at once (rare: no register
    // is kept for it)
    auto give_up = [&](bool stale) __attribute__((always_inline)) {
        if (stale) store_sc1(const_cast<unsigned*>(&sc->ovf), 1u);
    };
    int qn = 0;                                                               // entries in the queue (uniform)
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a window starts at any float

    // an admitted window -> the block's front list; a full list spills to memory
    auto admit_hits = [&](bool hit, float v, int r_global, int t) __attribute__((always_inline)) {
        const unsigned long long mask = __ballot(hit);
        if (!mask) return;
        int base = 0;
        if (lane == 0) base = atomicAdd(&ctl[CS_FRONT], __popcll(mask));
        base = __builtin_amdgcn_readfirstlane(base);
        if (hit) {
            const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (slot < NFL) fl[slot] = u32x4{__float_as_uint(v), (unsigned)r_global, (unsigned)t, 0u};
            else spill_candidate(hdr, f.cand_list, f.cand_cap, 0, xn, v, r_global, t);
        }
    };
    // the queue: a lane a window -- its fp32 samples and the copy's halves from memory, the chain in the reference's order, the audit
    auto verify_queue = [&]() __attribute__((always_inline)) {
        int ln = lane;
        asm volatile("" : "+v"(ln));                                          // (this rare path's addresses are made here, not kept across the unit loop)
        const bool have = ln < qn;
        const u64 mine = have ? sq[ln] : 0ull;
        const long long row = (long long)(unsigned)mine;
        const unsigned t = (unsigned)(mine >> 32);
        const float* y = a.dataset + row * a.T + t;
        const unsigned short* hc = cp.rows + row * cp.pitch + t;
        float v = 0.0f;
        bool stale = false;
        if (have) {
            int j = 0;
#pragma unroll 2
            for (; j + 4 <= Wr; j += 4) {
                const f32x4u yy = *reinterpret_cast<const f32x4u*>(y + j);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float D = __fsub_rn(x[j + c], yy[c]);
                    v = __builtin_fmaf(D, D, v);
                    stale = stale || copy_encode(yy[c], sc_c) != hc[j + c];
                }
            }
            for (; j < Wr; ++j) {
                const float yj = y[j];
                const float D = __fsub_rn(x[j], yj);
                v = __builtin_fmaf(D, D, v);
                stale = stale || copy_encode(yj, sc_c) != hc[j];
            }
        }
        give_up(stale);
        admit_hits(have && (v < tau2), v, (int)(row + a.r_offset), (int)t);
        wave_lds_fence();                                                     // (the queue is read: it may be written again)
        qn = 0;
    };
    // one unit: the staged fragments scaled and squared in registers, the next unit's request, the eight MFMAs, the survivors
    auto process = [&](CStage& st, unsigned u) __attribute__((always_inline)) -> unsigned {
        const bool on = u < uq.hi;                                            // (see the loop below)
        const Unit c = unit_decode(a, on ? u : uq.lo);
        const int seg_start = c.seg_start();
        const long long row = c.row(a);
        f16x8 fa[4], fb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            fb[s] = __builtin_bit_cast(f16x8, st.v[s]) * hd;                  // y^
            fa[s] = fb[s] * fb[s];                                            // (y^2)^
        }
        const unsigned un = uq.grab(lane);
        load(st, un);

        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        acc = mx_mac4(fa, [&](int s) { return *reinterpret_cast<const f16x8*>(bop + (size_t)s * 64 * 8); }, acc);
        const f32x16 aq = mx_mac4(fb, [&](int s) { return *reinterpret_cast<const f16x8*>(bop + (size_t)(4 + s) * 64 * 8); }, acc);
        if (on && mx_any_keep(aq, thr2)) {
            const unsigned hm = mx_keep_mask(aq, thr2);
            int n = 0;                                                        // survivors of the segment (uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                n += (int)__popcll(__ballot((((hm >> r) & 1u) != 0u) && (seg_start + mx_window(r, lane) < a.Tp)));
#ifdef PSH_TUNING
            // (the tuning build counts the windows the test keeps -- FusedHdr::pad[12], read by tools/filter_copy_survivors.py)
            if (lane == 0) atomicAdd(&hdr->pad[12], (unsigned)n);
#endif
            if (n > PSH_COPY_DENSE) {
                // a dense segment: its fp32 samples into the tile (the queue lives there: verified first), the chains from LDS
                if (qn > 0) verify_queue();
                const float* yrow = a.dataset + row * a.T;
                const unsigned short* hrow = cp.rows + row * cp.pitch + seg_start;
                const int lastf = (int)(a.T - seg_start) - 1;                 // (clamped tail: only inadmissible windows see it)
                int ln = lane;
                asm volatile("" : "+v"(ln));                                  // (this branch's addresses are made here, not kept across the unit loop)
#pragma unroll 1
                for (int i = ln; i < nhalf; i += 64) tile[lds_pad(i)] = yrow[seg_start + (i > lastf ? lastf : i)];
                wave_lds_fence();
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {
                    const int p = mx_window(r, lane);
                    const bool keep = (((hm >> r) & 1u) != 0u) && (seg_start + p < a.Tp);
                    if (!__ballot(keep)) continue;
                    float v = 0.0f;
                    bool stale = false;
                    if (keep) {
                        v = exact_one_rt(tile, p, x, Wr);                     // (the same chain as exact_one<W>; a rare branch: compact code)
                        // the audit: the samples' own encoding against the copy's halves (the segment was just streamed: L2)
                        for (int j = 0; j < Wr; ++j) stale = stale || copy_encode(tile[lds_pad(p + j)], sc_c) != hrow[p + j];
                    }
                    give_up(stale);
                    admit_hits(keep && (v < tau2), v, (int)(row + a.r_offset), seg_start + p);
                }
                wave_lds_fence();                                             // the tile is the queue again
            } else if (n > 0) {
                if (qn + n > PSH_COPY_QCAP) verify_queue();
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {
                    const bool keep = (((hm >> r) & 1u) != 0u) && (seg_start + mx_window(r, lane) < a.Tp);
                    const unsigned long long mask = __ballot(keep);
                    if (!mask) continue;
                    if (keep) {
                        const int slot = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                        sq[slot] = (u64)(unsigned)row | ((u64)(unsigned)(seg_start + mx_window(r, lane)) << 32);
                    }
                    qn += (int)__popcll(mask);
                }
                wave_lds_fence();                                             // (verify_queue reads other lanes' entries)
            }
        }
        return un;
    };
    // The two stage sets take turns, ALWAYS both: a set whose unit lies past the block's share (the last turns of a wave) holds the
    // header's bytes, its test runs on them and its verdict is dropped (`on`).  A turn that could be skipped would make the set
    // used next the one loaded last on some path, and the wait in front of it one for every load in flight.
    while (u0 < uq.hi || u1 < uq.hi) {
        u0 = process(s0, u0);
        u1 = process(s1, u1);
    }
    if (qn > 0) verify_queue();
    __syncthreads();
    // the block's candidates (distances in place of acc) go to the query's compact list behind ONE device-scope atomicAdd
    // (stream_scan_kernel's publication)
    if (wave == 0) {
        const int nfront = ctl[CS_FRONT];
        const int mown = nfront < NFL ? nfront : NFL;
        const bool have = lane < mown;
        static_assert(NFL == 64, "one entry a lane");
        const u32x4 e = have ? fl[lane] : u32x4{0u, 0u, 0u, 0u};
        const unsigned long long mask = __ballot(have);
        if (mask) {
            unsigned base = 0u;
            if (lane == 0) base = __hip_atomic_fetch_add((gu32*)&hdr->stream.ncand[0], (unsigned)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            if (have) {
                const unsigned slot = base + (unsigned)lane;
                if (slot < (unsigned)f.cand_cap) {
                    u32x4 o = e;
                    o[0] = __float_as_uint(dist_from_acc(__uint_as_float(e[0]), xn));
                    reinterpret_cast<u32x4*>(f.cand_list)[slot] = o;
                }
            }
        }
    }
}

// stream_scan_kernel's LDS without its two f16 arrays per wave (the A fragments come from memory), and 8 KB: the B fragments --
// band of ones, shifted query -- sit in LDS instead of 32 registers
size_t copy_scan_shmem_bytes(int tile_floats) {
    return stream_scan_shmem_bytes(tile_floats) - (size_t)(PSH_SCAN_THREADS / 64) * 2 * PSH_MX_NHALF * sizeof(_Float16) + 2 * 4 * 64 * 8 * sizeof(_Float16);
}

hipError_t launch_copy_scan(const ScanArgs& a, const FusedArgs& f, const CopyArgs& cp, int grid, hipStream_t s) {
    return pick<20, 0>(a.W == 20 ? 20 : 0, [&](auto WT) {
        return launch(copy_scan_kernel<WT()>, grid, PSH_SCAN_THREADS, copy_scan_shmem_bytes(a.tile_floats), s, a, f, cp); });
}

}  // namespace psh
