/*
 * psh.h -- C ABI of libpsh_hip.so: the MI355X (gfx950) k-nearest-path scan.
 *
 * This is the drop-in boundary for ONE hot path of RudyMorel/shadowing:
 * PathShadowing.shadow() with the Identity embedding, the RelativeMSE distance
 * and a PredictionContext -- the sliding-window distance scan over an ensemble
 * of R trajectories followed by the top-k selection.  The reference has no FFI
 * of its own (it is pure Python on torch); the seam these entry points sit
 * under is PathShadowing.batched_distance (reference
 * shadowing/path_shadowing/path_shadowing.py:97-179) and the path gather of
 * shadow() (path_shadowing.py:211-216).  INTEGRATION.md shows the ctypes stub
 * a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is HBM on `device`.
 *   - the caller owns every buffer (torch tensors -> data_ptr()); the library
 *     allocates nothing persistent, keeps no global state and reads no
 *     environment variable.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t, NULL = the
 *     default stream) and returns; the caller synchronises.
 *   - return value: PSH_OK or a negative PSH_ERR_*; nothing throws or aborts.
 *   - re-entrant and thread-safe given distinct workspaces.
 *   - results are bit-exact with the reference's CPU run (cuda=False): float32
 *     distances d = fl(fl(sqrt(acc))/||x||) with acc the sequential fp32 FMA
 *     chain over the window, indices (r_global, t) int32, rows sorted by
 *     (d, r, t) ascending -- the canonical order among the reference's
 *     arbitrarily ordered exact ties.
 */
#ifndef PSH_H
#define PSH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSH_VERSION 3      /* 2: psh_profile.tau_hint, psh_candidates_layout; 3: psh_shadow_blocking, psh_shadow_block_layout */

#define PSH_OK                 0
#define PSH_ERR_ARG           -1   /* NULL pointer / non-positive size / k > number of windows */
#define PSH_ERR_UNSUPPORTED   -2   /* W > PSH_MAX_W, k > PSH_MAX_K, index would overflow int32 */
#define PSH_ERR_WORKSPACE     -3   /* workspace too small (see psh_workspace_bytes) */
#define PSH_ERR_HIP           -4   /* a HIP runtime call failed (psh_last_hip_error) */
#define PSH_ERR_COMM          -5   /* RCCL could not be opened or a collective call failed (psh_last_comm_error) */

#define PSH_MAX_W      256         /* longest query window handled natively */
#define PSH_MAX_K      16384       /* largest k handled natively */

/* per-query status words written to `out_status` (device) by psh_scan_topk */
#define PSH_STATUS_OK        0
#define PSH_STATUS_OVERFLOW  1     /* candidate buffer overflowed -- or (embedded scan) fewer than k windows
                                      lay below the sampled estimate of the k-th distance: results of that
                                      query are INVALID, rerun it with the _exhaustive entry point */
#define PSH_STATUS_RETRY     2     /* the fused single-launch scan gave up (estimate short of k, a block with too many
                                      candidates, a block that was not resident, a workspace never initialised):
                                      results are INVALID, rerun the call with PSH_FLAG_NO_FUSE */

/*
 * Optional instrumentation of psh_scan_topk / psh_scan_topk_exhaustive.
 *   mode PSH_PROFILE_STAGES: HIP events are recorded on `stream` between the stages,
 *        the call SYNCHRONISES the stream and fills the *_ms fields.
 *   mode PSH_PROFILE_EVENTS: nothing is synchronised; the two caller-created
 *        hipEvent_t handles are recorded on `stream` immediately before and after the
 *        dominant kernel (the full sliding-window scan), so that a benchmark can time
 *        that kernel live inside its own timed loop.
 */
/* (PSH_PROFILE_STAGES implies the separate launches; PSH_PROFILE_EVENTS brackets the fused launch when that runs) */
#define PSH_PROFILE_STAGES 0
#define PSH_PROFILE_EVENTS 1
/* flags: the k best of every query are returned in ARBITRARY order (the sharded scan merges and
 * orders them after the all-gather anyway; saves the ordering stage of the selection kernel).
 * Honoured by psh_scan_topk on the sampled path only. */
#define PSH_FLAG_UNSORTED 1
/* A/B switches of the test-suite and the tools (results are identical either way):
 *   FILTER_VALU   the rejection test of the Identity scan on the vector ALUs instead of the matrix cores
 *   EMBED_DENSE   psh_scan_topk_embedded: dense fma chains over every tap even when the kernel has suffix rows / zero taps
 *   ROWS_GENERIC  one-window rows (T == W + h) through the generic exhaustive path instead of rows_kernel
 *   NO_FUSE       psh_scan_topk: the separate bootstrap / threshold / scan / select launches instead of the
 *                 single fused launch */
#define PSH_FLAG_FILTER_VALU  2
#define PSH_FLAG_EMBED_DENSE  4
#define PSH_FLAG_ROWS_GENERIC 8
#define PSH_FLAG_NO_FUSE      16
/* EMBED_MX: psh_scan_topk_embedded with a DENSE kernel (no suffix structure: a wavelet bank, a user kernel; d <= 12):
 * the rejection test as a split-precision banded product on the matrix cores (embed_mx_kernel), exact dense chains for the
 * survivors -- same results as without the flag.  (The library cannot look at the kernel matrix without a device
 * synchronisation, so the caller says which it is: Foveal-like kernels are faster WITHOUT the flag, on the suffix-rows path.) */
#define PSH_FLAG_EMBED_MX     64
/* EMBED_TAPS: psh_scan_topk_embedded on a suffix-rows kernel whose supports form ONE interval (Foveal): the running sums
 * by walking the taps, as for kernels with a gap, instead of differences of prefix sums (A/B tests; same results). */
#define PSH_FLAG_EMBED_TAPS   128
/* EMBED_PLAN_KEEP: psh_scan_topk_embedded: the caller's word that the previous sampled call on THIS workspace scanned with
 * the SAME kernel matrix (same contents): what that call found in the matrix (the plan region of the workspace) is used
 * again instead of being worked out by one more small launch (~25 us).  Wrong results if the matrix differs. */
#define PSH_FLAG_EMBED_PLAN_KEEP 256
/* EMBED_MX_SPLIT: with EMBED_MX: the full scan's rejection test with the three split-precision products the bootstrap uses
 * instead of one f16 product (a ten times smaller radius, three times the matrix-core work; A/B tests -- same results). */
#define PSH_FLAG_EMBED_MX_SPLIT 512
/* SELECT_ONE_BLOCK: the selection of a one- or two-query scan by the one-block radix select + sort even where the
 * ranking on all CUs applies (k <= 4096 and at most 8192 candidates; same results: A/B tests, timing). */
#define PSH_FLAG_SELECT_ONE_BLOCK 1024
/* RESERVE_CUS: the scan leaves a few compute units free: set by callers that run a collective and a merge on a side
 * stream beside the NEXT scan -- a scan otherwise owns every CU of the chip, and work on another stream would wait for
 * it (or make its last block wait).  Fused launch: grid = CUs - 4.  With PSH_FLAG_OVERLAP: grid = CUs -
 * PSH_STREAM_RESERVED_CUS, for streams made by psh_stream_create_reserving (consecutive scans overlap there, so only a
 * CU mask keeps compute units free). */
#define PSH_FLAG_RESERVE_CUS  32
/* OVERLAP: psh_scan_topk with ONE query (W <= 33): the step as three launches -- sample + admission level, scan, ranking
 * (psh_stream.hip) -- sized so that the small ones fit on the compute units BESIDE the scan of a call on ANOTHER stream, and
 * with no barrier inside the scan, so that its blocks take over a compute unit the moment the previous scan's block leaves
 * it.  For callers with independent queries in flight on two or three streams (a server; a sharded run overlapping its
 * exchange): per-step time in steady state is the ensemble's streaming time, not the fused launch's ~25 us more.  A
 * single stream is better served by the fused launch (the default).  Same results, same status protocol
 * (PSH_STATUS_RETRY -> rerun with PSH_FLAG_NO_FUSE); one workspace per stream, armed by psh_workspace_init. */
#define PSH_FLAG_OVERLAP      2048
/* MQ_F16: psh_scan_topk with a batch of queries (W <= 25): the rejection test of the batched scan as the f16 banded product
 * of rounds 2-4 (two K = 16 steps per tile) instead of the 8-bit product (one K = 32 step; since round 4 the default for
 * calls with 32 queries and more -- below that a segment's dearer set-up outweighs the halved matrix-core work).  The
 * 8-bit test puts every query of the batch on ONE quantisation step: a batch whose queries differ in amplitude by more than
 * ~4x is better served by f16 (a much smaller query keeps too many windows for its exact recheck -- slower, never wrong).
 * Same results either way (A/B tests; callers that know their batch). */
#define PSH_FLAG_MQ_F16       4096
/* LONG_LOOP: psh_scan_topk with four queries and more and a window of 34 .. 256 samples: the loop of one- to three-query steps of
 * rounds 5 (a pass over the ensemble per step) instead of the batched long-window scan (round 6: one pass per chunk of queries,
 * the queries' fragment tables in LDS, a segment's fragments in registers for all of them).  Same results (A/B tests, timing). */
#define PSH_FLAG_LONG_LOOP    8192
typedef struct psh_profile {
    int   mode;           /* in */
    int   flags;          /* in: PSH_FLAG_* */
    void* ev_scan_begin;  /* in (PSH_PROFILE_EVENTS): hipEvent_t */
    void* ev_scan_end;    /* in (PSH_PROFILE_EVENTS): hipEvent_t */
    float prep_ms;        /* query norms + state reset                      */
    float sample_ms;      /* sample-rows scan -> histogram of lane minima   */
    float threshold_ms;   /* histogram -> admission threshold               */
    float scan_ms;        /* the full sliding-window scan + filter (HBM-bound kernel) */
    float select_ms;      /* radix select + bitonic sort of the survivors   */
    float total_ms;
    int   path;           /* 0 = sampled threshold path, 1 = exhaustive path, 2 = sampled path as ONE fused launch,
                             3 = the three overlap-friendly launches (PSH_FLAG_OVERLAP) */
    int   n_sample_rows;
    int   grid_blocks;    /* blocks of the scan kernel */
    int   n_candidates;   /* PSH_PROFILE_STAGES: largest per-query candidate count the scan admitted */
    /* in (version 2), optional: the caller's ADMISSION HINT -- device-addressable, B floats, or NULL.
     * hint[b] is a level on acc = sum_j (x_j - y_{t+j})^2 = (d ||x||)^2 (behind an embedding: sum_i (hx_i - hy_i)^2): the call
     * admits the windows of query b with acc < hint[b] and takes NO bootstrap sample (no sample launch; the fused launch skips
     * its sample phase and its first grid barrier).  The results are the exact top-k whenever at least k windows lie below
     * the hint; when fewer do -- or the hint is not a positive finite number, or it admits more than the candidate lists hold --
     * the query's status says PSH_STATUS_OVERFLOW / PSH_STATUS_RETRY as for a sampled level that fell short, and the caller
     * reruns the call WITHOUT the hint.  Meant for consecutive queries whose k-th distance is known roughly (rolling query
     * dates: the previous call's out_d[b][k-1] -> hint = (d_k ||x||)^2 x margin), and for tests that pin the admitted set
     * (psh_candidates_layout).  The small-problem / exhaustive paths ignore it.  Mind the window length: the number of windows
     * below a level grows like level^(W / 2), so a margin of 10 % on acc admits ~2.6 k windows for k = 1024 at W = 20 and
     * hundreds of thousands at W = 126 (-> slow, or PSH_STATUS_RETRY beyond the lists' 65536 entries): margin ~ 2.6^(2 / W). */
    const float* tau_hint;
} psh_profile;

int         psh_version(void);
const char* psh_strerror(int code);
const char* psh_last_hip_error(void);   /* text of the last failing HIP call on this thread */

/*
 * Bytes of device workspace psh_scan_topk / psh_scan_topk_exhaustive want for
 * this problem (a larger workspace is used as a larger candidate buffer).
 */
int psh_workspace_bytes(int64_t R, int64_t T, int B, int W, int h, int k, size_t* out_bytes);
/*
 * Arm the fused single-launch scan for this workspace: psh_scan_topk with ONE query (W <= 33) then runs bootstrap,
 * threshold, scan and selection in one launch whose blocks exchange data through a header at the start of the
 * workspace.  Call once after allocating the workspace (and again after a PSH_STATUS_RETRY caused by a time-out);
 * a workspace that was never initialised is detected on the device and the call reports PSH_STATUS_RETRY.
 * The header keeps an epoch across launches: one workspace serves ONE stream at a time.
 */
int psh_workspace_init(int device, void* stream, void* workspace, size_t workspace_bytes);

/*
 * ||x||_2 of each query in the reduction order of the reference's
 * x.norm(dim=-1) (path_distance.py:65).  queries: device B x W.  out: device B.
 */
int psh_query_norm(int device, void* stream, const float* queries, int B, int W, float* out_qnorm);

/*
 * The scan: k nearest windows of every query.  Replaces the loop body of
 * PathShadowing.batched_distance (path_shadowing.py:149-173: embed, distance,
 * topk, index decode, running merge) for Identity + RelativeMSE +
 * PredictionContext(horizon = h).
 *
 *   dataset   device, R x T row-major float32 (single channel), resident in HBM
 *   r_offset  added to the row index in out_idx (shard -> global row)
 *   queries   device, B x W float32
 *   qnorm     device, B floats, or NULL: computed as psh_query_norm does
 *   h         PredictionContext.horizon (0 for None): windows t in [0, T-W-h]
 *   out_d     device, B x k float32, ascending
 *   out_idx   device, B x k x 2 int32 = [r_offset + r, t]
 *   out_status device, B int32 (PSH_STATUS_*)
 *
 * "device" for the small arguments (queries, out_d, out_idx, out_status; paths of psh_gather_paths) means device-ADDRESSABLE:
 * pinned host memory mapped into the device's address space (hipHostMalloc) is fine -- a blocking caller can have the kernels
 * read its query from and write its results into host memory and spare two copies (what shadowing_amd's shadow() does for one
 * query: 80 bytes in, B*k*12 bytes + the gathered paths out).  The ensemble and the workspace belong in HBM.
 * Requires R*(T-W-h+1) >= k (the reference raises for k larger than a split,
 * path_shadowing.py:165) and r_offset + R, T < 2^31.
 * One-window rows (T == W + h, e.g. N pre-embedded points of PathDistance.forward_topk with
 * W = T = d): the reference's numerator is then the contiguous 8-lane reduce, and the scan
 * runs a row per lane (rows_kernel) instead of a segment per wave.
 *
 * STATUS PROTOCOL -- every caller looks at out_status before it uses the results (PSH_FLAG_NO_FUSE or not, whatever B):
 *   PSH_STATUS_OK        out_d / out_idx of that query are the exact answer.
 *   PSH_STATUS_OVERFLOW  that query's candidate slices overflowed (massive exact ties) or fewer than k windows lay below the
 *                        sampled estimate: its results are INVALID -> psh_scan_topk_exhaustive for that query.
 *   PSH_STATUS_RETRY     the launches that serve 1, 2 or 3 queries (W <= 33) -- the fused single launch for one query,
 *                        the three overlap-friendly launches for one query under PSH_FLAG_OVERLAP and for EVERY call with
 *                        B = 2 or 3, flag or no flag -- admit below a statistical estimate and give up when it falls short
 *                        of k, when the candidate lists overflow (the fused launch: 64 entries per block; the three
 *                        launches: a query's list in the workspace, out[13] of psh_candidates_layout), or on a workspace
 *                        psh_workspace_init never armed:
 *                        results of EVERY query of the call are INVALID -- since version 2 the launches overwrite them with NaN
 *                        distances and (-1, -1) indices instead of leaving an earlier call's numbers -> the same call with PSH_FLAG_NO_FUSE
 *                        (the separate launches: a provable bound, per-query OVERFLOW as above).
 *   A call with psh_profile.tau_hint whose status is not OK for some query: the hint fell short (or was useless) -> the
 *                        same call WITHOUT the hint, then as above.
 * shadowing_amd/_native.py: scan_topk_checked is this protocol in 20 lines.
 *
 * WINDOW LENGTHS.  The rejection test of a scan runs on the matrix cores for ONE query with W <= 256 (W <= 33: the fused
 * launch / the three overlap-friendly launches with the shifted-query band in registers; 34 <= W <= 256: the three launches
 * with the band as a K-loop over ceil((W + 46) / 16) steps, flag or no flag -- stream_scan_long_kernel; round 6: the window
 * energies from fp32 prefix sums, one MFMA a step), for two or three queries with W <= 33 or a long window (they ride one pass
 * of the three launches: three up to W = 97, two up to W = 145 -- what fits LDS), for
 * larger batches with W <= 25, for four queries and more with 26 <= W <= 256 and for two or three beyond what rides one pass --
 * round 6: the batched long-window scan (psh_lq.hip) through the separate launches, one pass per chunk of queries;
 * PSH_FLAG_LONG_LOOP: round 5's loop of two- or three-query steps inside the call -- (status words per query as always);
 * PSH_FLAG_FILTER_VALU / PSH_FLAG_NO_FUSE calls use the vector-ALU filter or the exact chains.  Results do not depend on
 * which.
 */
int psh_scan_topk(int device, void* stream,
                  const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                  const float* queries, const float* qnorm, int B, int W, int h, int k,
                  float* out_d, int32_t* out_idx, int32_t* out_status,
                  void* workspace, size_t workspace_bytes, psh_profile* profile);

/*
 * A resident f16 copy of an ensemble that stays where it is from call to call, and the one-query overlap scan that
 * streams it instead of the fp32 samples (psh_stream_copy.hip: half the bytes of the pass; results are psh_scan_topk's,
 * bit for bit -- the copy only feeds the rejection test, the exact chains read the ensemble).
 *
 * psh_filter_copy_bytes: host arithmetic.  The copy is a 64-byte header, then R rows of *pitch_halves f16 values:
 * T rounded up to whole segments of 1024, plus 32 (a 16-byte load of a segment's 1024 + 32 halves never leaves its
 * row; the tail of a row is zero).
 * psh_filter_copy_build: enqueues three launches on `stream` -- the sum of squares of the finite samples (per-block
 * partial sums added in a fixed order: two builds give identical bits), ONE power-of-two exponent e_c for the ensemble
 * (its rms times 2^e_c lies in [0.5, 1); 0 for an rms that is zero or not finite) written into the header ON THE
 * DEVICE, and the rows (f16)(y 2^e_c), round to nearest even; what is not a finite f16 is stored as a NaN.  `out`:
 * out_bytes >= *bytes, 16-byte aligned; `scratch`: PSH_FILTER_COPY_SCRATCH_BYTES, free again when the launches have run.
 * Nothing is read back: the call never synchronises.
 * psh_scan_topk_copy: psh_scan_topk with a descriptor of such a copy OF THE SAME `dataset`.  The copy serves exactly one
 * route -- one query, W <= 33, PSH_FLAG_OVERLAP, no PSH_FLAG_FILTER_VALU / PSH_FLAG_NO_FUSE (a tau_hint is fine) --; every other
 * call, and a NULL descriptor, behaves as psh_scan_topk does.  copy->served says which: 1 = the copy scan was
 * launched (psh_profile.path is 3, sample rows and grid as on the fp32 route), 0 = the call went the ordinary way and
 * copy->reason says why.  Every window that survives the rejection test has its copy values audited against its fp32
 * samples; a mismatch (the copy is of other data) makes the call report PSH_STATUS_RETRY: rerun it through the
 * separate launches and drop the copy.  Only survivors are audited: keeping the copy in step with edits of the
 * ensemble is the caller's business.
 */
#define PSH_FILTER_COPY_SCRATCH_BYTES 16384
#define PSH_COPY_SERVED     0   /* psh_filter_copy.reason */
#define PSH_COPY_NOT_ROUTE  1   /* not the one-query overlap route with W <= 33 */
#define PSH_COPY_MISMATCH   2   /* the descriptor does not describe a copy of an (R, T) ensemble */
typedef struct psh_filter_copy {
    const void* copy;          /* what psh_filter_copy_build wrote */
    int64_t pitch_halves;      /* as psh_filter_copy_bytes gives it */
    int64_t R, T;              /* the ensemble the copy was built from */
    int served;                /* out */
    int reason;                /* out: PSH_COPY_* */
} psh_filter_copy;
int psh_filter_copy_bytes(int64_t R, int64_t T, size_t* bytes, int64_t* pitch_halves);
int psh_filter_copy_build(int device, void* stream, const float* dataset, int64_t R, int64_t T,
                          void* out, size_t out_bytes, void* scratch, size_t scratch_bytes);
int psh_scan_topk_copy(int device, void* stream,
                       const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                       const float* queries, const float* qnorm, int B, int W, int h, int k,
                       float* out_d, int32_t* out_idx, int32_t* out_status,
                       void* workspace, size_t workspace_bytes, psh_profile* profile, psh_filter_copy* copy);

/*
 * Same contract, no sampling and no admission threshold: the dataset is
 * processed in row chunks whose every window fits the candidate buffer.
 * Always exact (any amount of ties), several times slower.  out_status is
 * always PSH_STATUS_OK.
 */
int psh_scan_topk_exhaustive(int device, void* stream,
                             const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                             const float* queries, const float* qnorm, int B, int W, int h, int k,
                             float* out_d, int32_t* out_idx, int32_t* out_status,
                             void* workspace, size_t workspace_bytes, psh_profile* profile);

/*
 * The scan behind a general LINEAR embedding (Foveal, any PathEmbedding kernel):
 * replaces the same loop body (path_shadowing.py:149-173) when the embedding is
 * conv1d with a (d, 1, K) kernel (path_embedding.py:117-132, Foveal :142-172) and the
 * distance is RelativeMSE.  For every window t in [0, T-K-h] of every row
 *     hy_i = sum_j kernel[i][j] * y[t+j]         i < d   (fma chain, increasing j)
 *     acc  = sum_i (hx_i - hy_i)^2                        (fma chain, increasing i)
 *     d    = sqrt(acc) / hxnorm
 *   kernel  device, d x K row-major float32 (the UNPADDED kernel: the context's zero
 *           taps over the horizon are the integer h)
 *   hx      device, B x d float32: the embedded queries (embedding(x_context))
 *   hxnorm  device, B floats, or NULL: ||hx|| in the order of psh_query_norm
 * Everything else as psh_scan_topk (same workspace: psh_workspace_bytes with W = K).
 * The reference evaluates these sums in library-chosen orders, so agreement with IT is
 * to ~1e-6 relative (tested at 1e-5) with indices equal outside near-ties; agreement
 * with the oracle's restatement of the order above is bit-exact.  Requires d <= 128, K <= PSH_MAX_W and a
 * kernel matrix that fits LDS beside the wave tiles (psh_embedded_supported: up to 64 x 256, or 39 x 252 --
 * Foveal(1.15, 0.9, 252)), finite data, and MORE than one window per row:
 * T == K + h returns PSH_ERR_UNSUPPORTED -- that layout is scanned as R pre-embedded points, psh_embed_rows
 * followed by psh_scan_topk (below).
 * Kernels whose rows are one constant each on a common support from some tap onwards
 * (Foveal, also with an ImputationContext's gap; recognised on the device, K <= 256) are
 * scanned bound-then-verify over shared running sums -- same results, ~5x faster; when the
 * common support is one interval (Foveal itself) the running sums are differences of prefix sums
 * of the segment -- another ~2x (PSH_FLAG_EMBED_TAPS: the tap walk instead).
 * PSH_FLAG_EMBED_DENSE forces the dense chains over ALL K taps of every row, zero taps included (A/B tests; and the
 * exhaustive pass over rows that hold non-finite samples: 0 * NaN = NaN as in the reference's conv -- psh_rows_nonfinite).
 */
int psh_embedded_supported(int d, int K);   /* 1 when a d x K kernel fits the embedded scan (LDS), else 0 */
/* Diagnostics: byte offset, inside the workspace, of what the last sampled psh_scan_topk_embedded call found in its kernel
 * matrix -- four int32 {one_interval, ktop, merged_rows, d}: one_interval != 0 says the prefix-sum scan did the work
 * (tests and tools read it after synchronising the stream). */
size_t psh_embed_plan_offset(void);
/* Diagnostics (tests, tools): where a psh_scan_topk / psh_scan_topk_embedded call with these sizes on a workspace of
 * `workspace_bytes` leaves the windows its scan ADMITTED (acc below the level), before the selection picks k of them:
 *   out[0] byte offset of the per-query state (48 bytes a query: ||x||, the level's float bits, ...)
 *   out[1] byte offset of bcount  (int32 [B][out[9]]: entries block i appended to the FRONT of its slice of query b)
 *   out[2] byte offset of bcount2 (int32 [out[9]]: single-query matrix-core scan with two-class slices: entries at the BACK)
 *   out[3] byte offset of cand_d  (float [B][cap]: distances; 0xffffffff = a back entry whose distance was not computed)
 *   out[4] byte offset of cand_rt (int32 [B][cap][2]: (r_global, t))
 *   out[5] cap (entries per query); block i's slice of query b starts at b * cap + i * (cap / grid_blocks) -- grid_blocks
 *          from psh_profile after the call -- front entries upwards from its start, back entries downwards from its end
 *   out[6] byte offset of the fused / overlap-friendly launches' candidate area (16-byte entries), out[7] of the fused
 *          launch's per-block records (uint64 [out[10]]: low 31 bits = entries of block i, which start at entry i * out[11];
 *          an entry = {d bits | r << 32, t}), out[8] of the overlap-friendly launches' per-query counts (uint32 [4])
 *   out[9] PSH_MAX_BLOCKS, out[10] blocks of the fused launch at most, out[11] entries a fused block may publish
 *   out[12] byte offset of the overlap-friendly launches' lists (16-byte entries {d bits, r, t, q}; query q's list starts at
 *          entry q * out[13]), out[13] entries a query's list holds: the region of cand_d / cand_rt taken as one array, at
 *          most 65536 per query (a block whose own 64-entry list is full appends there directly: clustered matches in a
 *          smooth ensemble), or out[6] with out[10] * out[11] / B entries on a workspace too small for more
 * Nothing is launched; PSH_ERR_WORKSPACE when the workspace is too small for the sizes. */
int psh_candidates_layout(int64_t R, int64_t T, int B, int W, int h, int k, size_t workspace_bytes, int64_t* out14);
int psh_scan_topk_embedded(int device, void* stream,
                           const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                           const float* kernel, int d, int K,
                           const float* hx, const float* hxnorm, int B, int h, int k,
                           float* out_d, int32_t* out_idx, int32_t* out_status,
                           void* workspace, size_t workspace_bytes, psh_profile* profile);
int psh_scan_topk_embedded_exhaustive(int device, void* stream,
                           const float* dataset, int64_t R, int64_t T, int64_t r_offset,
                           const float* kernel, int d, int K,
                           const float* hx, const float* hxnorm, int B, int h, int k,
                           float* out_d, int32_t* out_idx, int32_t* out_status,
                           void* workspace, size_t workspace_bytes, psh_profile* profile);

/*
 * One-window rows behind a linear embedding (T == K + h).  The reference's embedded view (S, 1, d) is then
 * contiguous and RelativeMSE reduces over d in the 8-lane order (path_embedding.py:129-132, path_distance.py:65),
 * exactly what psh_scan_topk computes for rows ONE window long.  So:
 *     psh_embed_rows(dataset R x T, kernel d x K)  ->  out R x d:  out[r][i] = sum_j kernel[i][j] * y[r][j]
 *                                                                  (fma chain over increasing j)
 *     psh_scan_topk(dataset = out, R, T = d, queries = hx (B x d), W = d, h = 0)      (t is 0 in every index)
 * out: device, R x d float32, caller-owned.
 */
int psh_embed_rows(int device, void* stream, const float* dataset, int64_t R, int64_t T,
                   const float* kernel, int d, int K, float* out);

/*
 * Merge G sorted-or-not candidate lists per query into the k best by (d, r, t):
 * the running merge of path_shadowing.py:170-173 and the cross-GPU merge after
 * the all-gather of per-shard results.
 *   d_lists   device, B x n_in float32   (n_in = G * k_in, lists concatenated)
 *   idx_lists device, B x n_in x 2 int32 (entries with r < 0 are padding)
 *   workspace device, >= psh_merge_workspace_bytes(B, k)
 */
int psh_merge_workspace_bytes(int B, int k, size_t* out_bytes);
/* The same for G lists that sit where an all-gather left them, without a repacking copy:
 * list g of query b starts at d_gathered + g*rank_stride + b*k_in (floats) and at
 * idx_gathered + 2*(g*rank_stride_idx + b*k_in) (int32; the stride counts (r,t) pairs). */
int psh_merge_topk_gathered(int device, void* stream,
                            const float* d_gathered, const int32_t* idx_gathered,
                            int G, int64_t rank_stride, int64_t rank_stride_idx, int B, int k_in, int k,
                            float* out_d, int32_t* out_idx, void* workspace, size_t workspace_bytes);
/* The same when every list arrives SORTED by (d, r, t) (what psh_scan_topk returns) and list g holds
 * smaller rows than list g+1 (ranks own ascending row blocks): no selection, no sort -- each entry's
 * merged position is its own position plus a binary-search count per other list.  No workspace.
 * Requires G <= 64 and G * k_in <= 32768 (the distance keys sit in LDS); PSH_ERR_UNSUPPORTED otherwise. */
int psh_merge_sorted_gathered(int device, void* stream,
                              const float* d_gathered, const int32_t* idx_gathered,
                              int G, int64_t rank_stride, int64_t rank_stride_idx, int B, int k_in, int k,
                              float* out_d, int32_t* out_idx);
int psh_merge_topk(int device, void* stream,
                   const float* d_lists, const int32_t* idx_lists, int B, int n_in, int k,
                   float* out_d, int32_t* out_idx, void* workspace, size_t workspace_bytes);

/*
 * ---- multi-GPU: the exchange of the row-sharded scan (the reference has no multi-GPU path) ------------
 * One process per GPU.  Rank g keeps rows [lo_g, hi_g) resident, scans them with r_offset = lo_g (psh_scan_topk),
 * and the per-rank top-k lists meet in ONE all-gather of B*k*12 bytes per rank (RCCL over xGMI), after which every
 * rank merges the G sorted lists with the same (d, r, t) order -- results identical for any G.
 * RCCL is opened at run time from `librccl_path` (NULL: "librccl.so"); hand over the library the process already
 * uses (PyTorch-ROCm's torch/lib/librccl.so) so that there is one RCCL in the process.
 *   psh_comm_unique_id   rank 0 creates the 128-byte id; the caller broadcasts it by its own means
 *   psh_comm_create      collective over the `world` ranks (ncclCommInitRank)
 *   psh_exchange_merge   enqueues, without synchronising the host:
 *                          compute stream: record ev_scan_done            (the local scan wrote `send` before it)
 *                          side stream   : wait ev_scan_done; all-gather send -> gathered; merge -> out_d / out_idx;
 *                                          record ev_merged
 *                        so the collective and the merge run beside whatever the compute stream does next (the scan
 *                        of the next query batch); the consumer of out_d / out_idx waits for ev_merged.
 *     send      device, 3*B*k int32: the (B,k) float32 distances (bit patterns), then the (B,k,2) int32 indices --
 *               psh_scan_topk writes straight into it (out_d = send, out_idx = send + B*k)
 *     gathered  device, G x 3*B*k int32 (the all-gather's receive buffer, caller-owned)
 *     merge_workspace  psh_merge_workspace_bytes(B, k); only used when the sorted merge does not apply (G > 64 or
 *               G*k > 32768)
 *     ev_scan_done, ev_merged   hipEvent_t created by the caller
 *   Requires B*k even.  Buffers must stay alive until ev_merged has completed.
 */
#define PSH_COMM_ID_BYTES 128
typedef struct psh_comm psh_comm;
const char* psh_last_comm_error(void);
int psh_comm_unique_id(const char* librccl_path, void* out_id);
int psh_comm_create(const char* librccl_path, int device, int world, int rank, const void* id, psh_comm** out);
int psh_comm_destroy(psh_comm* comm);
int psh_comm_world(const psh_comm* comm);
int psh_exchange_merge(psh_comm* comm, void* compute_stream, void* side_stream,
                       const int32_t* send, int32_t* gathered, int B, int k,
                       float* out_d, int32_t* out_idx, void* merge_workspace, size_t merge_workspace_bytes,
                       void* ev_scan_done, void* ev_merged);

/*
 * A HIP stream whose kernels never run on `reserve_cus` of the device's compute units (hipExtStreamCreateWithCUMask): for
 * callers that keep a collective and a merge in flight on ANOTHER stream beside their scans.  A scan block holds its
 * compute unit for ~75 us; a foreign workgroup that does not fit into what the scan leaves free (one wave slot, 64 VGPRs
 * per SIMD, 16 KB of LDS) would otherwise wait for a block to leave -- and delay the next scan's block there by as much.
 * Scans on such a stream must be issued with PSH_FLAG_RESERVE_CUS (their grid then matches the compute units they can
 * use).  out_reserved receives the number actually reserved (0 when the device has too few).  The stream belongs to the
 * caller: psh_stream_destroy (or hipStreamDestroy).  (The reference has no counterpart: its multi-GPU story is absent.)
 */
#define PSH_STREAM_RESERVED_CUS 8
int psh_stream_create_reserving(int device, int reserve_cus, void** out_stream, int* out_reserved);
int psh_stream_destroy(int device, void* stream);

/*
 * Path gather of shadow() (path_shadowing.py:211-216):
 *   out[i, c, :] = dataset[idx[i,0] - r_offset, c, idx[i,1] : idx[i,1] + len]
 * dataset: device R x C x T;  idx: device n x 2;  out: device n x C x len.
 * Entries whose row is outside [0, R) (other shards' rows, padding) are left
 * untouched.
 */
int psh_gather_paths(int device, void* stream,
                     const float* dataset, int64_t R, int64_t C, int64_t T, int64_t r_offset,
                     const int32_t* idx, int64_t n, int len, float* out);

/*
 * ONE BLOCKING shadow() OF ONE Identity QUERY -- the reference's own call (README.md:47-57; path_shadowing.py:181-218:
 * normalise, batched_distance, the path gather, .cpu().numpy()) as ONE library call that returns when the results ARE in the
 * caller's host memory.  The only entry point that waits: it is the latency of this call that a caller of the reference's
 * API sees, and it is dominated by what lies around the ~100 us scan -- a second launch for the gather, the copies out, the
 * runtime's end-of-kernel notification.  Here
 *   - the query (and the optional admission hint) are read by the kernels from `host_block`, and the k distances, indices
 *     and gathered paths are WRITTEN BY THE KERNELS straight into it (write-through stores over PCIe: 172 KB at k = 1024);
 *   - when the fused single launch serves the call (W <= 33, the sizes psh_scan_topk takes it for), the ranking phase of that
 *     launch gathers the winners' paths itself -- no psh_gather_paths launch -- and its last blocks set completion words in the
 *     block which this function polls: it returns ~1 us after the last result byte has landed instead of after the
 *     runtime has noticed the kernel's end;
 *   - otherwise (long windows, large k, small ensembles): psh_scan_topk's launches + the gather launch, then
 *     hipStreamSynchronize.
 *   host_block        pinned host memory the device can address (hipHostMalloc / torch pin_memory; fine-grained, the HIP
 *                     default), >= out7[0] bytes of psh_shadow_block_layout; the CALLER writes the W query samples at byte
 *                     PSH_SHADOW_OFF_QUERY (and, with_hint != 0, the admission level -- psh_profile.tau_hint's meaning -- at
 *                     PSH_SHADOW_OFF_HINT) before the call and reads after it: int32 status at out7[1] (PSH_STATUS_*, the
 *                     STATUS PROTOCOL of psh_scan_topk: anything but OK -> the results are invalid, rerun through
 *                     psh_scan_topk with PSH_FLAG_NO_FUSE / without the hint), float32 d[k] at out7[4], int32 idx[k][2] at
 *                     out7[5], float32 paths[k][C][W + h] at out7[6].  The words in between belong to the library.
 *   rows              device, R x T: what the scan reads (channel 0; the smeared rows of an ensemble with non-finite samples)
 *   dataset3          device, R x C x T: what the paths are gathered from (== rows when C == 1)
 *   workspace         as psh_scan_topk's (B = 1), armed by psh_workspace_init; one workspace and one host block per stream
 *   profile           optional: flags in, path / grid_blocks out (path 2 = the fused launch served the call); its tau_hint and
 *                     events are ignored (with_hint selects the hint in the block)
 * Returns PSH_OK when the call has COMPLETED on the device (whatever the status word says), else a PSH_ERR_*.
 */
#define PSH_SHADOW_OFF_STATUS 0
#define PSH_SHADOW_OFF_DONE   64     /* 8 completion words + the call counter at 96: the library's */
#define PSH_SHADOW_OFF_SEQ    96
#define PSH_SHADOW_OFF_TIMES  16     /* diagnostics, 4 floats: us the last call spent enqueueing / waiting / until its launch had started / until the first completion word (fused launch) */
#define PSH_SHADOW_OFF_STARTED 60     /* diagnostics: the launch's first block sets it to the call counter when it starts */
#define PSH_SHADOW_OFF_HINT   112
#define PSH_SHADOW_OFF_QUERY  128    /* PSH_MAX_W floats */
int psh_shadow_block_layout(int W, int h, int k, int64_t C, size_t* out7);   /* {bytes, status, query, hint, d, idx, paths} */
int psh_shadow_blocking(int device, void* stream,
                        const float* rows, int64_t R, int64_t T, int64_t r_offset,
                        const float* dataset3, int64_t C, int W, int h, int k,
                        void* host_block, size_t host_block_bytes, int with_hint,
                        void* workspace, size_t workspace_bytes, psh_profile* profile);

/*
 * NON-FINITE SAMPLES.  The scans above judge a window by its own samples -- psh_scan_topk by all W of them,
 * psh_scan_topk_embedded by the taps [lo, hi) that the span of some kernel row covers (first to last tap with a non-zero
 * entry in any row) -- a NaN among those: distance NaN, never returned while k clean windows exist.  The reference's
 * embedding is a conv1d whose kernel is ZERO-PADDED by the horizon (path_embedding.py:48-51), and 0 * NaN = 0 * inf =
 * NaN: there a window is NaN as soon as one sample of y[r, :, t : t+K+h] -- the window, its h future samples, any channel
 * -- is NaN or +-inf.  A caller that wants exactly that for an ensemble holding such samples scans rows in which every
 * non-finite sample has been written over the h + (K - hi) samples before it and the lo samples after it:
 *   psh_count_nonfinite  *out_count (device, 8 bytes) = number of NaN / +-inf among n floats: 0 (almost always) -> scan
 *                        the ensemble as it is;
 *   psh_smear_nonfinite  out[r, q] (device R x T) = NaN if any channel of dataset (device R x C x T) holds a non-finite sample in
 *                        [q - fwd, q + back], else dataset[r, 0, q]; pass `out` as the scan's dataset with back = h + K - hi,
 *                        fwd = lo, gather paths from the original.  shadowing_amd.PathShadowing does this once per
 *                        resident ensemble.
 */
int psh_count_nonfinite(int device, void* stream, const float* x, int64_t n, unsigned long long* out_count);
/*   psh_rows_nonfinite   out_flags[r] (device, R int32) = 1 if row r of dataset (device R x C x T) holds a non-finite sample in any
 *                        channel, else 0.  For the EMBEDDED scans, whose rejection tests assume finite data (prefix sums and
 *                        matrix-core tiles spread a NaN over clean windows): a caller scans the clean rows with
 *                        psh_scan_topk_embedded, the dirty ones -- smeared with back = h, fwd = 0 -- with
 *                        psh_scan_topk_embedded_exhaustive (dense chains over all K taps: 0 * NaN = NaN exactly where the
 *                        reference's zero-padded conv has it), and merges the two lists (psh_merge_topk).
 *                        shadowing_amd.PathShadowing does this. */
int psh_rows_nonfinite(int device, void* stream, const float* dataset, int64_t R, int64_t C, int64_t T, int32_t* out_flags);
int psh_smear_nonfinite(int device, void* stream, const float* dataset, int64_t R, int64_t C, int64_t T, int back, int fwd, float* out);

/*
 * The reductions of predict_from_paths() (path_shadowing.py:245-252: `proba.avg(values, axis=1)`,
 * `proba.std(values, axis=1)` over the k shadowing paths):
 *   out_mean[b, i] = sum_j w[b, j] * values[b, j, i]
 *   out_std [b, i] = sqrt(sum_j w[b, j] * (values[b, j, i] - out_mean[b, i])^2)
 * values: device B x k x m float32 (the statistic `to_predict` evaluated on the out-context of the k paths);
 * weights: device B x k float64 AS GIVEN (the averaging class's, normalised or not -- nothing is renormalised), or NULL:
 * uniform 1/k;  out_mean, out_std: device B x m float64.  Sums in double, fixed order.
 */
int psh_weighted_moments(int device, void* stream, const float* values, const double* weights, int B, int k, int m,
                         double* out_mean, double* out_std);

/*
 * realized_variance (shadowing/statistics.py:5-16) of n_rows rows of log-returns:
 *   out[r, i] = mean(x[r, :Ts[i]]^2) * 252        (its square root if vol != 0)
 * x: device, row r starts at x + r * row_stride and holds `len` samples (a view into gathered paths: row_stride = W + h,
 * x = paths + W, len = h);  Ts: HOST array of nT <= 64 maturities in samples (clipped to len, as numpy's slice is);
 * out: device n_rows x nT float32.  Squares in fp32, sums in double.
 */
int psh_realized_variance(int device, void* stream, const float* x, int64_t n_rows, int64_t row_stride, int len,
                          const int* Ts, int nT, int vol, float* out);

/*
 * Weighted quantiles and tail means over the k shadowing paths: VaR and expected shortfall of the conditional ensemble.
 * One column is one (b, i) of values (device B x k x m float32); its weights are weights[b, 0 .. k-1] (device B x k
 * float64, AS GIVEN, never renormalised), or NULL: w_j = 1.  levels: HOST array of n_levels <= PSH_QUANTILE_MAX_LEVELS
 * levels 0 < p < 1, in any order.  With the k paths ordered by (value ascending, path index ascending), x_(i) and w_(i) the
 * sorted values and weights, all arithmetic in double and the float32 values converted exactly:
 *   C_i = sum_{l<=i} w_(l)     S_i = sum_{l<=i} w_(l) x_(l)     W = C_{k-1} (as computed)     t = p * W
 *   i*  = the first i with C_i >= t
 *   out_q     = x_(i*)                                                   the lower weighted quantile (inverted CDF)
 *   out_lower = ( S_{i*-1} + (t - C_{i*-1}) x_(i*) ) / t                 mean of the lowest p of the mass
 *   out_upper = ( (C_{i*} - t) x_(i*) + (S_{k-1} - S_{i*}) ) / (W - t)   mean of the highest 1 - p of the mass
 * out_q, out_lower, out_upper: device B x n_levels x m float64;  out_status: device B int32 (PSH_QUANTILE_STATUS_* bits),
 * or NULL.  A path of weight exactly 0 contributes nothing, whatever its value.  A non-finite value at a positive weight:
 * the column's results are NaN, PSH_QUANTILE_STATUS_NONFINITE.  A non-finite or negative weight, or W not > 0: all the
 * query's results are NaN, PSH_QUANTILE_STATUS_WEIGHTS.  -0.0 and +0.0 are equal values; which zero a quantile returns is
 * unspecified.  No floating-point atomics: two calls give identical bits, and so do weights scaled by a power of two.
 * A NULL values, levels or output, B, k, m or n_levels < 1, n_levels > PSH_QUANTILE_MAX_LEVELS, or a level that is not
 * inside (0, 1): PSH_ERR_ARG before anything touches the device; k > PSH_MAX_K or B * m >= 2^31: PSH_ERR_UNSUPPORTED.
 * The method heads shadowing_amd/csrc/psh_quantiles.hip; shadowing_amd/quantiles.py is its numpy twin.
 */
#define PSH_QUANTILE_MAX_LEVELS 32
#define PSH_QUANTILE_STATUS_OK         0
#define PSH_QUANTILE_STATUS_NONFINITE  1   /* a path with positive weight has a non-finite value in some column */
#define PSH_QUANTILE_STATUS_WEIGHTS    2   /* a non-finite or negative weight, or a weight sum that is not > 0 */
int psh_weighted_quantiles(int device, void* stream, const float* values, const double* weights, int B, int k, int m,
                           const double* levels, int n_levels, double* out_q, double* out_lower, double* out_upper,
                           int32_t* out_status);

/*
 * Scores of weighted predictive ensembles against what happened: the CRPS (continuous ranked probability score), the PIT
 * (probability integral transform: the predictive CDF at the outcome) and the mean, for a grid of weightings in one call.
 * One column is one (b, i) of values (device B x k x m float32); y = obs[b, i] (device B x m float32) is the realised
 * statistic.  Weight set e of query b is weights[e, b, 0 .. k-1] (device n_sets x B x k float64, AS GIVEN, never
 * renormalised), or NULL: one set, w_j = 1.  n_sets <= PSH_SCORE_MAX_SETS.  For one column and one set, keep the paths with
 * w > 0, order them by (value ascending, path index ascending), write x_(0..n-1), w_(i) for the sorted values and weights;
 * all arithmetic is in double and the float32 values are converted exactly:
 *   C_i = sum_{l<=i} w_(l)     S_i = sum_{l<=i} w_(l) x_(l)     W = C_{n-1} (as computed)
 *   out_mean   = S_{n-1} / W
 *   out_pit_lo = (sum of w_(i) with x_(i) <  y) / W          F(y-)
 *   out_pit_hi = (sum of w_(i) with x_(i) <= y) / W          F(y)
 *   c_i        = min(max(y, x_(i)), x_(i+1))
 *   out_crps   = (x_(0) - y)_+ + (y - x_(n-1))_+
 *                + (1 / W^2) sum_{i=0}^{n-2} [ C_i^2 (c_i - x_(i)) + (W - C_i)^2 (x_(i+1) - c_i) ]
 * out_crps is the integral of (F(z) - 1[z >= y])^2 gap by gap, every term non-negative; it equals E|X - y| - 1/2 E|X - X'|
 * under p = w / W.  out_crps, out_pit_lo, out_pit_hi, out_mean: device n_sets x B x m float64;  out_status: device
 * n_sets x B int32 (PSH_SCORE_STATUS_* bits), zeroed by the call, or NULL.  A path of weight exactly 0 contributes nothing,
 * whatever its value.  A non-finite value at a positive weight: the column's four results are NaN for that set,
 * PSH_SCORE_STATUS_NONFINITE.  A non-finite or negative weight, or W not > 0: all of (e, b) is NaN, PSH_SCORE_STATUS_WEIGHTS
 * (the values are then not looked at).  A non-finite obs[b, i]: the column is NaN for every set, PSH_SCORE_STATUS_OBS in
 * every status[e, b].  -0.0 and +0.0 are one value.  So crps >= 0; n = 1 gives |x - y|; pit_lo <= pit_hi, equal unless a
 * weighted path equals y.  No floating-point atomics: two calls give identical bits, so do weights scaled by a power of two
 * (while W^2 neither overflows nor underflows), and a set's results do not depend on which other sets ride the call.
 * A NULL values, obs or double output, B, k, m or n_sets < 1, n_sets > PSH_SCORE_MAX_SETS, or weights == NULL with
 * n_sets != 1: PSH_ERR_ARG before anything touches the device; k > PSH_MAX_K or B * m >= 2^31: PSH_ERR_UNSUPPORTED.
 * The method heads shadowing_amd/csrc/psh_scoring.hip; shadowing_amd/scoring.py is its numpy twin.
 */
#define PSH_SCORE_MAX_SETS 64
#define PSH_SCORE_STATUS_OK         0
#define PSH_SCORE_STATUS_NONFINITE  1   /* a path with positive weight has a non-finite value in some column */
#define PSH_SCORE_STATUS_WEIGHTS    2   /* a non-finite or negative weight, or a weight sum that is not > 0 */
#define PSH_SCORE_STATUS_OBS        4   /* a non-finite observation in some column of the query */
int psh_score_ensemble(int device, void* stream, const float* values, const double* weights, const float* obs,
                       int B, int k, int m, int n_sets,
                       double* out_crps, double* out_pit_lo, double* out_pit_hi, double* out_mean, int32_t* out_status);

/*
 * The averaging weights of the k shadowing paths of every query, formed from their distances where they lie, for a grid of
 * (eta, k') weightings in one call: what psh_weighted_moments, psh_weighted_quantiles, psh_score_ensemble and psh_hedged_mc
 * take as given.  distances: device B x k float32.  etas (HOST, n_etas doubles) are the widths, ks (HOST, n_ks ints, each
 * in 1 .. k; NULL with n_ks = 1: the one cut-off k) the cut-offs; set e = a * n_ks + c is (etas[a], ks[c]), and
 * n_etas * n_ks <= PSH_SCORE_MAX_SETS.  out_weights: device (n_etas * n_ks) x B x k float64.  For one query and one set:
 *   1. Order the paths by (distance ascending as numbers, path index ascending): -0.0 and +0.0 are equal, a NaN of either
 *      sign comes after +inf, NaNs among themselves go by index (numpy's stable argsort).
 *   2. The first k' paths are kept; every other path gets weight exactly 0.0.
 *   3. With d_j converted to double and s = 2.0 * (eta * eta), computed once on the host in double:
 *        z_j = -(d_j * d_j) / s      zmax = max of z over the kept paths (NaN if any kept z is NaN)
 *        a_j = z_j - zmax            e_j = exp(a_j)      Z = sum of e_j over the kept paths, in a fixed order
 *        w_j = e_j / Z
 *      d_j * d_j is exact, so a_j is three IEEE operations and is bit-identical to the numpy twin's; the weights differ
 *      from the twin's by exp (1 ulp a side), the order of the sum and the division: within (2 k' + 16) 2^-53 relative.
 *   4. eta = +infinity is w_j = 1.0 / k' for the kept paths, whatever their distances.
 *   5. A NaN among the kept distances makes every kept weight of that (e, b) NaN, and so do kept distances that are all
 *      infinite; the consumers answer with their *_STATUS_WEIGHTS.  A NaN or inf past the cut-off is harmless.
 *   6. No floating-point atomics: two calls give identical bits, and a set's bits do not depend on which other sets ride
 *      the call.
 * A NULL distances, etas or out_weights, B, k, n_etas or n_ks < 1, more than PSH_SCORE_MAX_SETS sets, an eta that is NaN or
 * not > 0, a k' outside 1 .. k, or ks == NULL with n_ks != 1: PSH_ERR_ARG before anything touches the device; k > PSH_MAX_K:
 * PSH_ERR_UNSUPPORTED.  The method heads shadowing_amd/csrc/psh_weights.hip; shadowing_amd/weights.py is its numpy twin.
 */
int psh_softmax_weights(int device, void* stream, const float* distances, int B, int k,
                        const double* etas, int n_etas, const int* ks, int n_ks, double* out_weights);

/*
 * Time-separated nearest windows: the exclusion zone of subsequence search on the list a scan returns.  The K nearest
 * SLIDING windows of a query may hold windows t and t + 1 of one trajectory, which share all but one of their future
 * samples; this entry keeps, of every group of such near-copies, the nearest.  d: device B x K float32; idx: device
 * B x K x 2 int32 = [r, t], as psh_scan_topk leaves them.  For one query, with its K entries (d_i, r_i, t_i) in the order
 * given (the scans hand them over ascending in (d, r, t)) and delta >= 0 an integer number of samples:
 *     keep_i  =  r_i >= 0  and  there is no j < i with keep_j, r_j == r_i and |t_j - t_i| <= delta
 * The rule reads positions and indices only, never d.  Row b of the outputs holds the first k kept entries in list order:
 *   out_d     device B x k float32: the input's bits, NaN included;
 *   out_idx   device B x k x 2 int32: [r, t];
 *   out_pos   device B x k int32: the position i in the input list (a caller who has gathered the K paths picks rows by it);
 *   out_count device B int32: the number kept among all K; it may exceed k;
 *   out_status device B int32: PSH_SEPARATE_STATUS_SHORT when out_count[b] < k; the slots past the count then hold +inf,
 *             (-1, -1) and -1.
 * What follows from the rule:
 *   - Prefix exactness: whether entry i is kept depends on the entries before i only.  So the kept entries of an exact
 *     top-K list are exactly the first kept entries of the greedy walk over ALL windows, and if out_count >= k the answer
 *     is exact whatever K was: over-asking the scan and separating is rigorous.
 *   - delta = 0 returns the first k entries with r >= 0 (two entries never share (r, t)).
 *   - An entry with r < 0 is padding: never kept, and it suppresses nothing.  t >= 0 wherever r >= 0.
 *   - Kept entries of one row are more than delta apart pairwise; every dropped entry has a kept entry of its row within
 *     delta at a smaller position.
 *   - delta goes up to 2^31 - 1 with r, t < 2^31: |t_j - t_i| is formed as a difference, nothing is added to delta.
 *   - The result of a query does not depend on the other queries of the call.
 *   - No atomics and no floating-point arithmetic at all: two calls give identical bits.
 * Stream-ordered: no workspace, no allocation, no synchronisation; capturable into a graph.
 * A NULL pointer, B, K or k < 1, k > K, or delta < 0: PSH_ERR_ARG before anything touches the device; K > PSH_MAX_K:
 * PSH_ERR_UNSUPPORTED.  The method heads shadowing_amd/csrc/psh_separate.hip; shadowing_amd/separation.py is its numpy twin.
 */
#define PSH_SEPARATE_STATUS_OK     0
#define PSH_SEPARATE_STATUS_SHORT  1   /* fewer than k of the K entries are kept */
int psh_separate_topk(int device, void* stream, const float* d, const int32_t* idx, int B, int K, int k, int delta,
                      float* out_d, int32_t* out_idx, int32_t* out_pos, int32_t* out_count, int32_t* out_status);

/*
 * Hedged Monte Carlo (Potters, Bouchaud, Sestovic 2001) on the k shadowing paths of each of B dates: the option prices,
 * Black-Scholes implied vols and strikes of a smile.  The method, in full, heads shadowing_amd/csrc/psh_hmc.hip (and
 * README "Option pricing"); shadowing_amd/pricing.py is its numpy twin.
 *   dlnx:  device float32 log-returns, row b * k + i (path i of date b) starts at dlnx + (b * k + i) * row_stride and holds
 *          `len` samples (the out-context view of psh_gather_paths output: dlnx = paths + c * (W + h) + W,
 *          row_stride = C * (W + h), len = h -- no copy);
 *   weights: device B x k float64 (normalised here by their sum), or NULL: uniform;
 *   Ts: HOST array of nT <= 64 maturities in samples, 1 <= T <= len;  Ms: HOST array of nM <= 64 rescaled log-moneyness;
 *   degree: 1..5 (basis u^0..u^degree);  kind: PSH_HMC_OTM / PSH_HMC_CALL / PSH_HMC_PUT;
 *   out_price, out_iv, out_strike: device B x nT x nM float64;  out_sigma: device B x nT (sigma_T) or NULL;
 *   out_status: device B int32 (PSH_HMC_STATUS_* bits; NONFINITE / WEIGHTS: all the date's results are NaN) or NULL.
 * k > PSH_MAX_K or degree > 5: PSH_ERR_UNSUPPORTED.  Sums in double, fixed order: two calls give identical bits.
 */
#define PSH_HMC_OTM   0        /* a call for M >= 0, a put for M < 0 */
#define PSH_HMC_CALL  1
#define PSH_HMC_PUT   2
#define PSH_HMC_STATUS_OK         0
#define PSH_HMC_STATUS_NONFINITE  1   /* a path with non-zero weight has a non-finite return in [0, max Ts) */
#define PSH_HMC_STATUS_WEIGHTS    2   /* a non-finite weight, or a weight sum that is not > 0 */
#define PSH_HMC_STATUS_ILL_CONDITIONED 4   /* a maturity whose fit is nearly singular or whose hedge is nearly riskless
                                              (psh_hmc.hip): its prices and IVs are NaN, its strikes and sigma stay */
int psh_hedged_mc(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                  const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                  int degree, int kind, double* out_price, double* out_iv, double* out_strike, double* out_sigma,
                  int32_t* out_status);

/*
 * The weights of the k shadowing paths of each of B dates, calibrated to quoted vanillas: the weighted Monte Carlo of
 * Avellaneda, Buff, Friedman, Grandchamp, Kruk and Newman (2001).  The weights move as little as possible in relative
 * entropy from the prior until the weighted paths reprice the quotes; the result is a (B, k) float64 array that
 * psh_hedged_mc, psh_hedge_replay, psh_weighted_quantiles, psh_weighted_moments and psh_score_ensemble take as given.  The
 * method heads shadowing_amd/csrc/psh_calibrate.hip (and README "Calibrating to market quotes"); shadowing_amd/calibration.py
 * (calibrate_host) is its numpy twin.
 *   dlnx, row_stride, B, k, len: as psh_hedged_mc;  prior: device B x k float64 prior weights p_i >= 0, or NULL: 1;
 *   Ts: HOST array of nT maturities in samples, 1 <= T <= len;  strike, target: device B x nT x nM float64, the quoted
 *   strikes and prices; a NaN target: not quoted;  kind: PSH_HMC_OTM (a call iff K >= x_init exp(rho T)) / CALL / PUT;
 *   martingale != 0: each maturity adds the instrument "forward", payoff S_T, target x_init exp(rho T) undiscounted.
 * For one date, all in double, rho = rate / 252:
 *     l_0 = 0, l_{n+1} = l_n + r[i, n]  (sequential)      S_{T,i} = x_init exp(l_T)
 *     g_ij = exp(-rho T_j) payoff_j(S_{T_j, i})           forward: g = exp(-rho T) S_T, c = x_init
 *     h_ij = (g_ij - c_j) / x_init                        instrument j = q * nM + m;  forwards: nT * nM + q
 *     J = nT * nM + (martingale ? nT : 0) <= PSH_CAL_MAX_INSTRUMENTS       (beyond: PSH_ERR_UNSUPPORTED)
 *     a_i = sum_j lambda_j h_ij     amax = max of a over p_i > 0     e_i = p_i exp(a_i - amax)     Z = sum e_i (fixed order)
 *     q_i = e_i / Z                 P = sum p_i
 *   lambda minimises Phi = amax + ln(Z / P) + (eps / 2) |lambda|^2, eps >= 0 (0: the hard constraint; > 0 always has a
 *   solution, which reprices quote j with error -eps lambda_j x_init):
 *     grad_j = mu_j + eps lambda_j,  mu_j = sum_i q_i h_ij,   H_jl = sum_i q_i h_ij h_il - mu_j mu_l + eps delta_jl
 *   by Newton steps from lambda = 0: success when max_j |grad_j| <= tol; else H d = -grad by Cholesky in instrument order
 *   (an unknown whose diagonal is not > 0 or whose pivot is <= 1e-10 of it is dropped: step 0; an unquoted instrument is
 *   never an unknown), t = 1, 1/2, ..., 2^-40 until Phi(lambda + t d) <= Phi(lambda) + 1e-4 t grad.d, at most max_iter
 *   steps.  Every unknown dropped above tol, a failed line search, or max_iter steps: the last iterate, NOT_CONVERGED.
 *   out_weights: device B x k (q; exactly 0 where p_i = 0);  out_lambda: B x J (0 for unquoted and dropped unknowns);
 *   out_model: B x J, sum_i q_i g_ij of every instrument;  out_info: B x 4 = [kl = sum q_i (a_i - amax) - ln(Z / P),
 *   n_eff = 1 / sum q_i^2, Newton steps taken, max_j |grad_j| at the end];  out_status: B int32, PSH_CAL_STATUS_* bits.
 *   workspace: device, psh_calibrate_workspace_bytes(B, k, nT) bytes (PSH_ERR_WORKSPACE when smaller).
 * A path with p_i = 0 contributes nothing whatever its returns; scaling the prior by a power of two changes no bit; no
 * floating-point atomics: two calls give identical bits, and a date's bits do not depend on the other dates of the call.
 * A NULL pointer (prior apart), a size < 1, row_stride < len, eps negative or NaN, tol not > 0, max_iter < 0, a T outside
 * 1 .. len: PSH_ERR_ARG before anything touches the device; k > PSH_MAX_K or J > PSH_CAL_MAX_INSTRUMENTS: PSH_ERR_UNSUPPORTED.
 */
#define PSH_CAL_MAX_INSTRUMENTS 32
#define PSH_CAL_STATUS_OK            0
#define PSH_CAL_STATUS_NONFINITE     1   /* a path with p_i > 0 has a non-finite return in [0, max Ts): all outputs NaN */
#define PSH_CAL_STATUS_WEIGHTS       2   /* a prior weight negative or not finite, or their sum not > 0: all outputs NaN */
#define PSH_CAL_STATUS_QUOTES        4   /* a strike not finite and > 0, or an infinite target: all outputs NaN */
#define PSH_CAL_STATUS_NOT_CONVERGED 8   /* the outputs are the last iterate */
#define PSH_CAL_STATUS_DROPPED       16  /* an unknown was dropped in the last solve (redundant quotes): informational */
int psh_calibrate_workspace_bytes(int B, int k, int nT, size_t* out);
int psh_calibrate_weights(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                          const double* prior, double x_init, double rate, const int* Ts, int nT, const double* strike,
                          const double* target, int nM, int kind, int martingale, double eps, double tol, int max_iter,
                          double* out_weights, double* out_lambda, double* out_model, double* out_info, int32_t* out_status,
                          void* workspace, size_t workspace_bytes);

/*
 * The hedge of a smile: the fit of psh_hedged_mc with its policy kept, and the replay of a policy on paths.  The
 * definition, in full, heads shadowing_amd/csrc/psh_hmc_report.hip (and README "Option pricing"); pricing.py
 * (replay_host) is the numpy twin.
 *   The policy of one (date b, maturity q, strike j) holds, for every step n < Ts[q], mu_n, isd_n (the standardisation of
 *   S_n), gamma_n[0..P] and beta_n[0..P] of the fit (P = degree; dropped unknowns are 0), double, row-major:
 *     policy[b][q][j][n][c],  n < Tmax = max Ts,  c < 2P + 4 = [mu, isd, gamma_0..P, beta_0..P];  rows n >= Ts[q] are 0.
 *   delta = beta_0[0] = policy[b][q][j][0][P + 3], the hedge ratio at inception.
 *   psh_hmc_policy_doubles: the doubles of a policy, B * nT * nM * Tmax * (2 degree + 4) (host only).
 *   psh_hedged_mc_policy: psh_hedged_mc -- the same arguments, the same five outputs bit for bit -- and out_policy.
 *   psh_hedge_replay: on B x k paths (any k; dlnx, row_stride, len, weights as psh_hedged_mc) with the policy, `strike` and
 *   `centre` (device B x nT x nM: the FIT's out_strike and out_price) and the fit's x_init, rate, Ts, Ms, degree, kind:
 *     l_0 = 0, l_{n+1} = l_n + r[i, n];  S_n = x_init exp(l_n), S_0 = x_init;  u_n = (S_n - mu_n) isd_n;
 *     phi_n = sum_a beta_n[a] u_n^a (Horner);  D_n = e^-rho S_{n+1} - S_n, rho = rate / 252;
 *     gain_i = sum_{n<T} exp(-rho n) phi_n D_n;  pay_i = exp(-rho T) payoff_j(S_T);  pnl_i = pay_i - gain_i;
 *   out_sums: device B x nT x nM x 9 float64, with c = centre and w the weights normalised by their sum:
 *     [a1 = sum w (pnl - c), a2 = sum w (pnl - c)^2, b1 = sum w^2 (pnl - c), b2 = sum w^2 (pnl - c)^2,
 *      p1, p2, q1, q2: the same four of pay, s2 = sum w^2]:
 *     mean = c + a1, risk = sqrt(max(a2 - a1^2, 0)), se = sqrt(max(b2 - 2 a1 b1 + a1^2 s2, 0)), mc = c + p1,
 *     risk_unhedged and se_unhedged likewise from p and q, n_eff = 1 / s2.  se treats the policy as fixed: honest on
 *     paths the policy was not fitted on, optimistic on the fit's own.
 *   out_pnl: device B x nT x nM x k float64 or NULL (a path of weight 0: NaN);
 *   out_status: device B int32 or NULL (NONFINITE / WEIGHTS as psh_hedged_mc: all the date's sums and pnl are NaN);
 *   a centre that is not finite (a maturity the fit flagged): NaN sums and pnl there;
 *   workspace: device, psh_hedge_replay_workspace_bytes(B, k, nT, nM) bytes (PSH_ERR_WORKSPACE when smaller).
 * degree > 5, or max Ts beyond what the policy rows of a strike group fit in LDS (833 at degree 5): PSH_ERR_UNSUPPORTED.
 * Sums in double, fixed order, no floating-point atomics: two calls give identical bits.
 */
int psh_hmc_policy_doubles(int B, int nT, int nM, int Tmax, int degree, size_t* out);
int psh_hedged_mc_policy(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                         const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                         int degree, int kind, double* out_price, double* out_iv, double* out_strike, double* out_sigma,
                         int32_t* out_status, double* out_policy);
int psh_hedge_replay_workspace_bytes(int B, int k, int nT, int nM, size_t* out);
int psh_hedge_replay(int device, void* stream, const float* dlnx, int64_t row_stride, int B, int k, int len,
                     const double* weights, double x_init, double rate, const int* Ts, int nT, const double* Ms, int nM,
                     int degree, int kind, const double* policy, const double* strike, const double* centre,
                     double* out_sums /* B x nT x nM x 9 */, double* out_pnl /* B x nT x nM x k, or NULL */,
                     int32_t* out_status, void* workspace, size_t workspace_bytes);

/*
 * Path generation of the discrete path-dependent volatility model (Guyon, Lekeufack 2024): S paths of n_steps steps for
 * each of B dates, one lane per path, in double.  The method, in full, heads shadowing_amd/csrc/psh_pdv.hip (and README
 * "PDV model"); shadowing_amd/pdv.py (PDVModelDiscrete.gen, pdv_future_paths) is its numpy twin.
 *   lams1, lams2, decay1, decay2, thetas: HOST arrays of 2 (decay = exp(-lams / 252) as the caller computed it);
 *   betas: HOST array of n_betas = 3 or 4;  S0: the first price of every path;  sqrt_dt: the scale of the draws;
 *   nu: 0 for Gaussian draws, > 0 for Student-t(nu) draws (unused when draws != NULL);
 *   R10, R20: device B x 2 float64, the initial factors of each date;
 *   draws: device (B*S) x n_steps float64 raw draws (normalised here), or NULL: Philox4x32-10 keyed by `seed`, the draws
 *          of path g = b * S + p at step t depending only on (seed, g, t);
 *   out_sigma, out_St: device (B*S) x n_steps float64;  out_dlnx: device (B*S) x (n_steps - 1) float32 log1p of the
 *   returns (the layout psh_hedged_mc reads);  out_draws, out_dw: device (B*S) x n_steps float64 raw and normalised
 *   draws.  Each output may be NULL.
 * A NULL input, B < 1, S < 1, n_steps < 1, n_betas not 3 or 4, nu < 0 or not finite, or B * S * n_steps past int64:
 * PSH_ERR_ARG before anything touches the device; B * S >= 2^39: PSH_ERR_UNSUPPORTED.  Two calls give identical bits.
 */
int psh_pdv_generate(int device, void* stream, int B, int64_t S, int n_steps, const double* lams1, const double* lams2,
                     const double* decay1, const double* decay2, const double* thetas, const double* betas, int n_betas,
                     double S0, double sqrt_dt, double nu, const double* R10, const double* R20, const double* draws,
                     uint64_t seed, double* out_sigma, double* out_St, float* out_dlnx, double* out_draws,
                     double* out_dw);

/*
 * An ensemble of R log-normal multifractal random walks (Bacry, Delour, Muzy 2001) of n returns each, made on the
 * device: r[t] = sigma * eps[t] * exp(omega[t] - c0), omega Gaussian with the log-correlated covariance c, eps
 * fractional Gaussian noise (white for H = 0.5), both by circulant embedding, one workgroup and one in-LDS transform per
 * pair of paths, in double.  The method, in full, heads shadowing_amd/csrc/psh_mrw.hip (and README "MRW ensemble");
 * shadowing_amd/mrw.py (mrw_log_returns, MRWGenerator) is its numpy twin and computes the tables.
 *   M: the smallest power of two >= 2n;
 *   a_omega: device M float64, sqrt(max(s[k], 0) / M) with s the eigenvalues of omega's circulant covariance;
 *   a_eps: the same table for fractional Gaussian noise, or NULL: H = 0.5, eps is white noise drawn directly;
 *   c0: c[0] = Var omega, so that E[r^2] = sigma^2;  seed: the Philox4x32-10 key -- the samples of path g depend only on
 *   (seed, g, n, the tables), never on R;
 *   out_dlnx: device float32, row g at out_dlnx + g * dlnx_row_stride (n floats; the bytes between rows are left alone),
 *   so a (R, 1, n) ensemble is written where the scan reads it;  out_lnx: device R x (n + 1) float64 log-prices from 0;
 *   out_omega: device R x n float64.  Each output may be NULL.
 * A NULL a_omega, R < 1, n < 2, sigma < 0 or not finite, c0 not finite, or dlnx_row_stride < n with out_dlnx:
 * PSH_ERR_ARG before anything touches the device; n > 4096 (the transform leaves LDS) or R >= 2^32:
 * PSH_ERR_UNSUPPORTED.  Two calls give identical bits.
 */
int psh_mrw_generate(int device, void* stream, int64_t R, int n, double sigma, const double* a_omega, const double* a_eps,
                     double c0, uint64_t seed, float* out_dlnx, int64_t dlnx_row_stride, double* out_lnx,
                     double* out_omega);

/*
 * An ensemble of R skewed multifractal random walks (Pochart, Bouchaud 2002) of n returns each: the MRW above with white
 * noise and a leverage term in the log-volatility,
 *   lv[t] = omega[t] - A[t],  A[t] = sum_{j=1..m} K(j) eps[t - j],  r[t] = sigma * eps[t] * exp(lv[t] - c0 - v),
 * K(j) = K0 / j^alpha, v = sum_j K(j)^2, so E[r^2] = sigma^2 at every t and E[r_t r_{t+tau}^2] < 0 for K0 > 0.  The
 * method, in full, heads shadowing_amd/csrc/psh_smrw.hip (and README "Skewed MRW"); shadowing_amd/mrw.py
 * (smrw_log_returns, SMRWGenerator) is its numpy twin and computes the tables.
 *   M, a_omega, c0, sigma, seed, out_dlnx, dlnx_row_stride, out_lnx: as psh_mrw_generate; omega and eps[t], t >= 0, are
 *   that function's draws at H = 0.5, and the pre-history eps[-m .. -1] is drawn on a stream of its own;
 *   m: the memory of the kernel in lags, 1 <= m <= M - n (the convolution is linear inside the circulant of size M);
 *   k_hat: device M complex float64 (2 M doubles, re then im), k_hat[k] = conj(F[k]) exp(-2 pi i k m / M) / M with
 *   F = FFT_M of (0, K(1), .., K(m), 0, ..): the index reversal, the shift by m and the 1 / M of the inverse transform
 *   folded in, so that A = FFT_M(k_hat[k] X[(-k) mod M]) with X the transform of the noise.  All zeros is the MRW;
 *   v: sum_j K(j)^2;  out_logvol: device R x n float64, lv = omega - A.  Each output may be NULL.
 * A NULL a_omega or k_hat, R < 1, n < 2, m < 1, n + m > M, sigma < 0 or not finite, c0 or v not finite, or
 * dlnx_row_stride < n with out_dlnx: PSH_ERR_ARG before anything touches the device; n > 4096 or R >= 2^32:
 * PSH_ERR_UNSUPPORTED (and then m is not looked at).  Two calls give identical bits; a path depends only on
 * (seed, path, n, m, the tables), never on R.
 */
int psh_smrw_generate(int device, void* stream, int64_t R, int n, int m, double sigma, const double* a_omega,
                      const double* k_hat, double c0, double v, uint64_t seed, float* out_dlnx, int64_t dlnx_row_stride,
                      double* out_lnx, double* out_logvol);

/*
 * The stylised facts of an ensemble where it lies: lagged cross-moments of (x, x^2) with itself.  x: device float32, row r
 * starts at x + r * row_stride and holds n samples (the (R, 1, n) tensors of the generators and a scan dataset are read in
 * place);  m: the largest lag, 0 <= m <= min(n - 1, 1024);  G: row groups, 1 <= G <= R, group g holding rows
 * [floor(g R / G), floor((g+1) R / G)).  For each group and each lag tau = 0 .. m, the sums over the group's rows and over
 * t = 0 .. n - 1 - tau (pairs never cross a row) of
 *   xx = x[t] x[t+tau],   xx2 = x[t] x[t+tau]^2,   x2x = x[t]^2 x[t+tau],   x2x2 = x[t]^2 x[t+tau]^2
 * with every sample converted to double first, all products and sums in double.
 *   out_sums: device G x 4 x (m + 1) float64, (xx, xx2, x2x, x2x2) in that order;  out_rows_used: device G int64;
 *   out_status: device int32 (PSH_MOMENTS_STATUS_*), or NULL;  workspace: device, psh_lagged_moments_workspace_bytes.
 * A row that holds a NaN or an inf contributes nothing, is not counted in out_rows_used, and sets
 * PSH_MOMENTS_STATUS_ROWS_EXCLUDED.  The summation order is fixed by (R, n, m, G) alone (no floating-point atomics, no
 * dependence on the number of workgroups that ran): two calls give identical bits.
 * A NULL pointer, R < 1, n < 1, row_stride < n, m < 0, m >= n, G < 1 or G > R: PSH_ERR_ARG before anything touches the
 * device; m > 1024 or R >= 2^31: PSH_ERR_UNSUPPORTED; a workspace that is too small: PSH_ERR_WORKSPACE.
 * The method, in full, heads shadowing_amd/csrc/psh_moments.hip; shadowing_amd/stylized.py is its numpy twin.
 */
#define PSH_MOMENTS_STATUS_OK             0
#define PSH_MOMENTS_STATUS_ROWS_EXCLUDED  1   /* at least one row held a NaN or an inf and was left out */
/* host only, nothing is launched: the bytes psh_lagged_moments needs for these sizes */
int psh_lagged_moments_workspace_bytes(int64_t R, int m, int64_t G, size_t* out_bytes);
int psh_lagged_moments(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int m, int64_t G,
                       double* out_sums, int64_t* out_rows_used, int32_t* out_status, void* workspace,
                       size_t workspace_bytes);

/*
 * The wavelet scattering spectra of an ensemble where it lies (Morel et al., arXiv 2204.10177, in this project's own
 * terms).  x: device float32, row r starts at x + r * row_stride and holds n samples, n a power of two, 8 <= n <= 4096;
 * J: scales, 1 <= J <= log2(n) - 2;  psi_hat: device J x n/2 float64, psi_hat[j][k] the real Fourier multiplier of the
 * analytic wavelet of scale j = 1 .. J at bin k < n/2, taken to be zero outside n / 2^(j+2) < k < n / 2^j and never read
 * there;  G: row groups, 1 <= G <= R, group g holding rows [floor(g R / G), floor((g+1) R / G)).  Per row, F the DFT of
 * size n (convolutions are circular), every sample converted to double first, all arithmetic in double:
 *   W_j = IDFT(F[x] psi_hat[j]),   U_j = |W_j|,   V_{j1,j2} = IDFT(F[U_j1] psi_hat[j2]), j1 <= j2,
 *   S1[j] = mean_t U_j,   S2[j] = mean_t U_j^2,   C3[j1,j2] = mean_t W_j2 conj(V_{j1,j2}), j1 <= j2,
 *   C4[j1,j1',j2] = mean_t V_{j1,j2} conj(V_{j1',j2}), j1 <= j1' <= j2.
 *   out_sums: device G x NOUT float64, NOUT = 2 J + 2 P3 + 2 P4, P3 = J (J + 1) / 2, P4 = J (J + 1) (J + 2) / 6: the sums of
 *   the per-row values over the group's rows, laid out [S1 (J), S2 (J), Re C3 (P3), Im C3 (P3), Re C4 (P4), Im C4 (P4)]
 *   with p3 = j2 (j2 - 1) / 2 + (j1 - 1) and p4 = (j2 - 1) j2 (j2 + 1) / 6 + j1' (j1' - 1) / 2 + (j1 - 1);
 *   out_rows_used: device G int64;  out_status: device int32 (PSH_SCATTERING_STATUS_*), or NULL;
 *   workspace: device, psh_scattering_spectra_workspace_bytes.
 * A row that holds a NaN or an inf contributes nothing, is not counted in out_rows_used, and sets
 * PSH_SCATTERING_STATUS_ROWS_EXCLUDED.  The summation order is fixed by (R, n, J, G) alone (no floating-point atomics, no
 * dependence on the number of workgroups that ran): two calls give identical bits, and a group's sums depend on its own
 * rows alone.  Every transform stays in LDS: a row's spectra never go to device memory.
 * A NULL pointer, R < 1, n not a power of two or n < 8, row_stride < n, J < 1, J > log2(n) - 2, G < 1 or G > R:
 * PSH_ERR_ARG before anything touches the device; n > 4096 or R >= 2^31 (and, where n is not known, J > 10):
 * PSH_ERR_UNSUPPORTED; a workspace that is too small: PSH_ERR_WORKSPACE.
 * The method, in full, heads shadowing_amd/csrc/psh_scattering.hip; shadowing_amd/scattering.py is its numpy twin and
 * computes the stock wavelets.
 */
#define PSH_SCATTERING_STATUS_OK             0
#define PSH_SCATTERING_STATUS_ROWS_EXCLUDED  1   /* at least one row held a NaN or an inf and was left out */
/* host only, nothing is launched: the bytes psh_scattering_spectra needs for these sizes */
int psh_scattering_spectra_workspace_bytes(int64_t R, int J, int64_t G, size_t* out_bytes);
int psh_scattering_spectra(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int J,
                           const double* psi_hat, int64_t G, double* out_sums, int64_t* out_rows_used,
                           int32_t* out_status, void* workspace, size_t workspace_bytes);

/*
 * The gradient of each row's scattering spectra with respect to the row (a vector-Jacobian product).  x, R, row_stride, n,
 * J, psi_hat, G, the group bounds and the NOUT layout are psh_scattering_spectra's;  cot: device G x NOUT float64, the
 * cotangent of each group's sums;  out_grad: device float64, row r at out_grad + r * grad_stride, grad_stride >= n (what
 * lies between the rows is left untouched).  For row r of group g, with out_o(x_r) the row's own value of output o (what
 * the row adds to its group's sum), every sample converted to double first and all arithmetic in double:
 *   out_grad[r * grad_stride + t] = sum_o cot[g][o] d out_o(x_r) / d x_r[t].
 * A row that holds a NaN or an inf gets n zeros and sets PSH_SCATTERING_STATUS_ROWS_EXCLUDED in out_status (device int32,
 * or NULL).  The cotangent of Im C4[j1, j1, j2] is ignored: that output is identically 0.  Where W_j(t) = 0 the phase
 * W / |W| is taken as 0, so an all-zero row gets an all-zero gradient and never a NaN.
 * A row's gradient depends on that row and on its group's cot row alone: two calls give identical bits, and the bits do
 * not depend on R, G, the row's position or how many workgroups ran (no atomics).  Every transform stays in LDS.
 *   workspace: device, psh_scattering_vjp_workspace_bytes.
 * The argument checks and error codes are psh_scattering_spectra's, and grad_stride < n is PSH_ERR_ARG too.
 * The formulas and the method head shadowing_amd/csrc/psh_scattering_grad.hip; the torch twin in
 * shadowing_amd/scattering.py (torch.fft on the time-domain definition, differentiated by autograd) is an independent
 * derivation.
 */
/* host only, nothing is launched: the bytes psh_scattering_vjp needs for these sizes */
int psh_scattering_vjp_workspace_bytes(int64_t R, int n, int J, int64_t G, size_t* out_bytes);
int psh_scattering_vjp(int device, void* stream, const float* x, int64_t R, int64_t row_stride, int n, int J,
                       const double* psi_hat, int64_t G, const double* cot /* G x NOUT */, double* out_grad,
                       int64_t grad_stride, int32_t* out_status, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PSH_H */
