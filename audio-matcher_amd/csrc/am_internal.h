// am_internal.h -- what the host files of libaudiomatch_amd.so share: the context, plans, options, the
// needle handle, the engine's request types and the helpers more than one file calls.
#pragma once
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "am_kernels.h"
#include "am_spans.h"

namespace am {

// ---------------------------------------------------------------------------
extern thread_local std::string t_err;   // am_last_error_string
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#define AM_HIP(call)                                         \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #call);    \
    } while (0)

// progress hooks (audio_matcher.rs:102-117, 129); a call works on the snapshot it takes on entry
struct Hooks {
    am_progress_fn fn = nullptr;
    void* user = nullptr;
    am_chunk_progress_fn chunk_fn = nullptr;
    void* chunk_user = nullptr;
};
Hooks snapshot_hooks();

// The options of am_set_option, as every entry point sees them: read once, on entry (snapshot_opts), so that a
// concurrent am_set_option never changes a call half way; "log_n" and "half_pipeline" can also be fixed per needle
// handle (am_needle_set_option), which wins over the default.  Each member is one row of the option table
// (am_context.hip), which says what it means.
struct Opts {
    long long log_n, pairs_per_group, half, batch_overlap, needle_group, dense, device_redo, debug_no_realloc, debug_redo_arm_at;
    long long peak_filter_order, distance_rule, tail_window, surrounding_from, k3_group, pick_group, tail_block, host_pick_wait;
    long long profile_mask, profile_every, pick_priority;
    long long score_norm, score_norm_floor_db;
    long long trace_form;
    PeakPolicy peak_policy() const { return PeakPolicy{(int)peak_filter_order, (int)(distance_rule & 1), (int)((distance_rule >> 1) & 1)}; }
};
static const float kHalfGain = 1024.0f;      // keeps the stored values of a normalised score near 1
static const double kMinEfficiency = 0.75;  // hop / N the auto plan accepts
static const int kLogNMin = 10, kLogNMax = 23;
// needles longer than this run on N = 2^22 (measured crossover between 2 and 5 s of 44.1 kHz
// audio, tools/needle_sweep.py, profiles/r03/needle_sweep.txt: 2 s 0.674 against 0.685 ms per hour of
// audio, 5 s 0.725 against 0.702)
static const long long kWideFromSamples = 140000;
// needles longer than this run on N = 2^23 = 1024 x 8192 (measured crossover between 30 and 36 s of 44.1 kHz
// audio, profiles/r03/needle_sweep.txt: the 1024-row column kernels cost more per point, the hop is longer)
static const long long kWidestFromSamples = 1500000;
// Needles longer than this (half a 2^23 transform) are cut into segments of at most 2^22 samples:
// corr(hay, needle)[j] = sum_i corr(hay, segment_i)[j + offset_i], every segment on the register kernels
// of the 2^23 plan (hop efficiency of at least one half), the partial sums added up in the score array by
// K3 (MyConvolve::correlate accepts any length, audio_matcher.rs:414-457).
static const long long kSegmentFrom = 1ll << 22;
static const long long kSegmentLen = 1ll << 22;

// ---------------------------------------------------------------------------
// While a batch is being queued (kernels of earlier haystacks still running, or not yet started) no
// scratch buffer may move: hipFree waits for the device (the overlap of pick and transforms stalls) and a
// buffer whose contents a later launch still expects would be lost (round 3, gpurun_out/r03q: a peak lost
// to a flag buffer re-allocated under a running pick).  match_many / match_multi_many size everything
// before their queueing loops; with the option "debug_no_realloc" an ensure() that would still have to
// allocate inside such a loop fails the call instead (tests/test_gpu_round4.py).
extern thread_local int t_no_realloc;
struct QueueingScope {
    bool on;
    explicit QueueingScope(bool enable) : on(enable) { if (on) ++t_no_realloc; }
    ~QueueingScope() { end(); }
    void end() { if (on) { --t_no_realloc; on = false; } }
    QueueingScope(const QueueingScope&) = delete;
    QueueingScope& operator=(const QueueingScope&) = delete;
};
int realloc_refused(const char* what, size_t bytes, size_t cap);

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return AM_OK;
        if (t_no_realloc > 0) return realloc_refused("a device", bytes, cap);
        release();
        size_t want = bytes + bytes / 8;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, bytes);
            want = bytes;
            if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc(scratch)"); }
        }
        cap = want;
        return AM_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    int ensure(size_t bytes) {
        if (bytes <= cap) return AM_OK;
        if (t_no_realloc > 0) return realloc_refused("a pinned host", bytes, cap);
        release();
        hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipHostMalloc"); }
        cap = bytes;
        return AM_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
    }
};

struct Plan {
    PlanDev dev{};
    float2* tables = nullptr;  // one allocation holding the four tables
    unsigned* mf = nullptr;    // constant tables of the matrix-core row kernel (N2 = 8192 only)
};

// One set of score-side buffers: the scores, their tile summaries (level 1) and peak lists for the pick; K3's level-0
// summary and its ballots / thresholds; the work matrix the scores come from.
struct ScoreSide { DevBuf scores, stats, stats32, wflags, peaks, work; };

struct ProfRec { int name; hipEvent_t e0, e1; };
enum { KN_K1 = 0, KN_K2, KN_K3, KN_STATS, KN_PEAKS, KN_OTHER, KN_TRACE, KN_DISCOVER, KN_ENV_FRAMES, KN_ENV_PREFIX, KN_ENV_CORR, KN_EDGES, KN_MASK, KN_COUNT };

struct Ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;           // peak pick of haystack k beside the transforms of k+1 (batches)
    hipStream_t stream_tail = nullptr;       // a haystack's odd last block on the smaller plan, beside its main pass (run_tail_block)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf work_tail, tail_scores, tail_stats;   // (a batch computes the tails of up to kMaxTailBatch haystacks per launch: two alternating halves)
    DevBuf work_tail2;                           // several needles: the tail's inverse rows, one matrix per needle of a group
    std::recursive_mutex mu;
    std::map<int, Plan> plans;
    // The score-side buffers, two sets: in a batch the peak pick of haystack k runs on stream2 beside the transforms of
    // haystack k+1, which then need their own set.  The second work matrix serves the device-side redo (batches): the
    // inverse rows of haystack k are still there when its pick has found chunks whose certificate failed.  Everything
    // outside an overlapped batch works in side[0].
    ScoreSide side[2];
    DevBuf work2, segs, io_in, io_out, sum, arena_cur, wide_ctl, wide_list, wide_tiles;
    DevBuf norm_blk;   // block energies of the haystack being normalised (option score_norm; used on one stream at a time)
    // per-hit scoring, every family (the frame in am_hits.hip): the call's hit table, its partial records and their flag
    // words, the results and the spans a host form stages, each sized in bytes by the call at hand; a call holds `mu`
    // and waits for its results, so one set serves the families in turn
    DevBuf hit_tab, hit_parts, hit_flags, hit_out, hit_stage;
    HostBuf hit_io;                         // ... and the pinned host side: the table, the results behind it
    std::map<int, DevBuf> band_tabs;        // per-band hit scoring (am_bands.hip): the window and twiddle table of each frame_log2
    DevBuf warp_tab, warp_needles;          // per-hit drift scoring (am_warp.hip): the interpolator's table (kept), a call's warped needles
    // per-hit significance (am_significance.hip): the spans and score zones of one group of hits, the slice partials and
    // the per-hit state between the two passes
    DevBuf sig_span, sig_scores, sig_psum, sig_pmax, sig_mean, sig_hmax;
    std::map<std::pair<int, int>, DevBuf> rs_taps;              // sample-rate conversion: the polyphase table of each (L, M)
    DevBuf lag_parts, lag_r;   // spectral whitening (am_whiten.hip): the per-(lag, block) partial lag products and their sums
    DevBuf redo_pairs[2];   // device-side redo (batches): the per-pair "run again" flags of both sets
    // several needles: the K3s of a needle group run as ONE launch, every needle of the group with score-side
    // buffers of its own; two such sets alternate (the picks of group g beside the transforms of group g + 1)
    DevBuf grp_scores[2][kMaxNeedleGroup], grp_stats32[2][kMaxNeedleGroup], grp_wflags[2][kMaxNeedleGroup];
    DevBuf grp_stats[kMaxNeedleGroup];   // tile summaries of the group's picks (one set: picks run one group after the other)
    HostBuf failcnt;   // host-visible: one byte per chunk of a call, set when the chunk failed its certificate
    hipEvent_t ev_k3[2] = {nullptr, nullptr}, ev_pick[2] = {nullptr, nullptr};
    HostBuf pinned;
    // Per-chunk result headers live in coherent pinned host memory that the peak
    // kernel writes directly (a few KB per haystack): no device-to-host copy
    // sits between the last kernel and the host's wake-up.
    HostBuf hdr;
    HostBuf spill;   // spill arena of the single-chunk passes (same kind of memory)
    HostBuf badflag; // one word per haystack of a call: "some score was not finite"
    DevBuf ranges, range_flags;   // work area of the non-finite-sample search (rare path)
    DevBuf big;                   // lists, sort keys and bucket table of a chunk with more than AM_MAX_PEAKS_PER_CHUNK peaks (rare path)
    // the k best matches (am_best.hip): tile summaries, per-tile top keys, histograms and counters, the finite/non-finite
    // transitions, the candidate list; the score array and the down-mixed haystack of am_match_best
    DevBuf best_stats, best_lmax, best_ctl, best_trans, best_list, best_scores, best_mono;
    DevBuf trace_out, trace_parts;   // score traces (am_trace.hip): a call's records and, in the sliced form, the slices' partials
    // needle discovery (am_discover.hip): recording A down-mixed, the probe being matched, the energy parts, the slices'
    // partials and a call's records
    DevBuf disc_a, disc_probe, disc_energy, disc_parts, disc_out;
    // edge matching (am_edges.hip): both sanitised spans, their coarse scores, their energy scans with the tile totals,
    // the non-finite marks, the exact stage's partial sums, the probe records and the edge records of one haystack
    DevBuf edge_span, edge_scores, edge_scan, edge_tot, edge_ctl, edge_parts, edge_rec;
    // envelope matching (am_envelope.hip): the frame jobs of a launch, the needle bank's and the haystack's levels, the
    // bank padded to whole chunks with its per-needle sums, the haystack's prefix sums and their block sums, z and qi
    DevBuf env_jobs, env_needles, env_hay, env_bank, env_desc, env_prefix, env_blocks, env_out;
    // the chunk list currently resident in `segs` (re-uploaded only when it changes)
    std::vector<Segment> segs_resident;
    // profiling
    bool prof = false;
    std::vector<ProfRec> pending;
    std::vector<hipEvent_t> pool;
    double prof_ms[KN_COUNT] = {0};
    uint64_t prof_n[KN_COUNT] = {0};
    uint64_t prof_seq[KN_COUNT] = {0};   // launches of the class seen while profiling is on (option profile_every)
};

// Events that order the library's streams of ONE device among themselves (the pick behind K3, K3 behind the pick that
// last read its score set, the tail stream) and the events that time kernels: without the system-scope fence a default
// event performs when it is recorded (a write-back and invalidation of the caches).  Nothing here needs that fence:
// kernel boundaries order device memory by themselves, and what the host reads (result headers in pinned memory) it
// reads behind a hipStreamSynchronize.  Measured -0.7 % on the headline, near the noise: what an event costs a stream
// is its barrier packet, 4 - 8 us of a kernel boundary, fence or not (profiles/r04/event_gaps.txt).
#ifndef AM_EVENT_NO_SYSTEM_FENCE
#define AM_EVENT_NO_SYSTEM_FENCE 1
#endif
constexpr unsigned kSyncEvent = hipEventDisableTiming | (AM_EVENT_NO_SYSTEM_FENCE ? hipEventDisableSystemFence : 0u);

int get_ctx(int device, Ctx** out);
struct ProfScope {
    Ctx* c; int name; hipStream_t st; hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on;
    ProfScope(Ctx* c_, int name_, hipStream_t st_ = nullptr);   // (am_context.hip: reads the options profile_mask / profile_every)
    ~ProfScope() {
        if (on) { (void)hipEventRecord(e1, st); c->pending.push_back({name, e0, e1}); }
    }
};
hipError_t copy_on_stream(Ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

// ---- the steps the entry points share (am_context.hip, beside copy_on_stream) ----
// AM_ERR_INVALID_ARG "bad sample format" unless sample_format is AM_FMT_F32_MONO or AM_FMT_S16_STEREO; with `who` the
// message is "<who>: bad sample format <sample_format>"
int check_format(int sample_format, const char* who = nullptr);
// one f32 mono sample and one interleaved i16 stereo frame are both 4 bytes
inline size_t sample_bytes(size_t elements) { return 4 * elements; }
// A host form's input: sizes c->io_in for `bytes`, copies them up on c's stream and waits (copy_on_stream); *d is
// c->io_in.p.  The caller holds c's lock; the input stays there until the context's next upload.
int upload_input(Ctx* c, const void* host, size_t bytes, const void** d);
// `bytes` of device memory into the caller's host memory on c's stream, waited for (copy_on_stream)
int download(Ctx* c, void* host, const void* dev, size_t bytes);
// AM_ERR_INVALID_ARG unless p is device memory of `device`: hit_check_device's message behind `prefix`
// ("am_xxx_device: d_name: ", or "" for the message as it is)
int check_device_arg(const void* p, int device, const char* prefix);
// The resident form *d of a call's input p: a host form (device_io false) uploads it (upload_input); a _device form
// takes p as it is.  check_prefix says whether that _device form checks residency: nullptr = it trusts its caller,
// anything else = check_device_arg(p, c->device, check_prefix) first.
int resident_input(Ctx* c, bool device_io, const void* p, size_t bytes, const void** d, const char* check_prefix = nullptr);
// A call's list to its caller: *n_out = v.size() and the first min(v.size(), cap) elements in out; AM_ERR_CAPACITY with
// the message `too_small` when the list is longer than cap
template <class T>
int hand_back(const std::vector<T>& v, T* out, size_t cap, size_t* n_out, const char* too_small) {
    *n_out = v.size();
    for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    if (v.size() > cap) return fail(AM_ERR_CAPACITY, too_small);
    return AM_OK;
}
// force_logN1: another factorisation than the production one (am_debug_column_bench: 2^23 as 512 x 16384)
int get_plan(Ctx* c, int logN, const Plan** out, int force_logN1 = 0);

}  // namespace am

// ---------------------------------------------------------------------------
struct am_needle {
    am::Ctx* ctx = nullptr;
    float* d_needle = nullptr;
    size_t n = 0;
    float inv_autocorr = 0.f;
    double energy = 0.0;   // sum(needle^2) in f64 (launch_sumsq): the needle's half of the score_norm denominator
    std::map<int, float2*> spectra;  // logN -> conj(H)/N in pipeline layout
    std::map<int, unsigned*> spectra16;   // logN -> the same as scaled __half2 points (half_pipeline = 2)
    std::map<int, unsigned*> spectra16m;  // logN -> the same conjugated, in [a'][b'][c'] order (option k2_mfma)
    // Lowest chunk minimum of each of the last few haystacks matched with this needle (index 0:
    // unscaled scores, 1: AM_SCALE_LIB).  Bounds the raw-score write threshold from above, so that a
    // score array that drifts slowly (chunk minimum in another block pair than a tile's scores)
    // stays inside its certificate; a ring, so that one unusual haystack is forgotten again.
    static constexpr int kRecent = 8;
    float recent_min[2][kRecent];
    int recent_n[2] = {0, 0}, recent_pos[2] = {0, 0};
    void remember_min(int sm, float v) {
        recent_min[sm][recent_pos[sm]] = v;
        recent_pos[sm] = (recent_pos[sm] + 1) % kRecent;
        if (recent_n[sm] < kRecent) ++recent_n[sm];
    }
    // haystacks left for which the ring takes the LOWEST chunk minimum (after a haystack in which many chunks
    // failed their certificate: a drifting score array); otherwise, where a failed chunk is redone on the
    // device, it takes the median -- the background level -- so that a few chunks with deep dips (a hit whose
    // autocorrelation has negative lobes) do not make every later haystack write all its scores
    int conservative_left[2] = {0, 0};
    // haystacks left for which a batch queues the device-side redo (a K3 launch that looks at the pairs' flags and
    // a second pick per haystack: 1.6 % of the headline's time when nothing ever fails).  Armed by a failed
    // certificate -- of an earlier call, or of an earlier haystack of the same call as soon as its flag has
    // arrived in host memory; until then such a chunk is redone from the host, as in single calls.
    int redo_armed_left[2] = {0, 0};
    float hist_min(int sm) const {
        float m = FLT_MAX;
        for (int i = 0; i < recent_n[sm]; ++i) m = std::min(m, recent_min[sm][i]);
        return m;
    }
    // per-handle overrides of the process-wide option defaults (-1 = follow the default)
    long long opt_log_n = -1, opt_half = -1, opt_score_norm = -1;
    // Needle partitioning (needles longer than kSegmentFrom samples): sub-handles over slices of d_needle
    // (not owned), each with its own spectra; segment i starts at sample seg_off[i] of the needle.
    std::vector<am_needle*> segments;
    std::vector<long long> seg_off;
    bool owns_data = true;
    // edge matching (am_edges.hip): the needle's f64 energy scans, n prefix sums and n suffix sums behind them, made by
    // the first call that needs them
    double* d_edge_scans = nullptr;
    // masked needles (am_needle_create_masked): the gaps as given (none: an ordinary handle) and the kept spans between
    // them, as the device table the masked normalising kernel reads (am_norm.hip): [a_0, b_0, a_1, b_1, ..], ascending.
    // d_needle holds +0 in the gaps, so `energy` is the energy of the kept samples.
    // d_gap_orig (n samples) is the complement: the needle's original samples in the gaps, +0 in the kept spans
    // (am_hit_mask, am_mask.hip).
    std::vector<am_span> gaps;
    long long* d_kept = nullptr;
    int n_kept = 0;
    float* d_gap_orig = nullptr;
};

namespace am {

// The overlap-save engine: scores[j] = factor * sum_n X[j + n - lead] needle[n]
// When a ScanRequest is given and the plan supports it, K3 also writes the level-0
// (min,max) summary into the request's stats32 and ScanResult::fused becomes true.
// Where a pass works: the work matrix, K3's level-0 summary and its ballots / thresholds.  A score-side set of the
// context (scan_buffers), or -- streaming ingest -- summary and flag buffers the caller owns.
struct ScanBuffers { DevBuf* work; DevBuf* stats32; DevBuf* wflags; };
inline ScanBuffers scan_buffers(ScoreSide& sd) { return ScanBuffers{&sd.work, &sd.stats32, &sd.wflags}; }
// What the caller asks of a pass (the callee does not change it)
struct ScanRequest {
    float margin;            // a run's raw scores are written when its maximum reaches min(its K3 tile's minimum, hist_min) + margin; < 0: all
    float hist_min;          // lowest chunk minimum of the needle's recent haystacks (FLT_MAX: none)
    long long seg_c, seg_d;  // chunk geometry (scores i*seg_c .. i*seg_c + seg_d)
    ScanBuffers out;         // where the pass works (all null: set 0 of the context)
    hipEvent_t before_k3;    // K3 must not overwrite those buffers before this event (or null)
    // restrict the launch to the blocks that produce scores [range_a, range_b) (range_b = 0:
    // everything).  Used to redo single chunks with theta = -inf in place.
    long long range_a, range_b;
    // (streaming ingest): the block count the flag buffer is laid out for (0: this launch's own).  The
    // thresholds sit behind the ballots, i.e. at an offset that depends on the block count: early pairs are
    // launched under the layout of the announced length and the final pass must keep that layout even
    // when the real length gives fewer blocks.
    long long side_nblocks;
    bool skip_launch;        // (streaming ingest) launch nothing: every pair was computed while the samples arrived; only describe what is there
    bool tail_by_caller;     // the caller computes a TailPlan's scores itself (match_many, several haystacks per launch): main pass only
    bool no_scan;            // only the block restriction (range_a, range_b) applies; K3 writes plain scores
};
// What a pass reports back
struct ScanResult {
    bool fused;              // K3 produced stats32 / wflags
    SparseScores sparse;     // description of what was written
    // what a second K3 launch over the same work matrix needs (valid when redo_ok)
    bool redo_ok;
    Job redo_job; PlanDev redo_pl; float redo_scale; int redo_half; int redo_npairs; const float2* redo_work; ScanCfg redo_cfg;
};
// plain scores, every one written, no level-0 summary: the pick summarises them itself (tile_stats)
inline SparseScores plain_scores() { return SparseScores{nullptr, nullptr, nullptr, 1, 5, 5, 1.0}; }
struct Geometry {
    int logN;
    long long N, hop, nblocks, npairs;
};
// The odd last block.  Two blocks share one complex transform, so a haystack with an odd number of blocks pays a
// whole pair for its last, usually part-filled block (1 h at 44.1 kHz against a 10 s needle: 42.2 blocks of the
// 2^22 plan = 22 pairs, 2.3 % of the points for nothing).  When the scores behind the last even block boundary T fit
// into one pair of a smaller plan that has the fused scan, the main pass stops at T and those scores come from
// that plan, computed on a stream of their own beside the main pass (run_tail_block): every run written, and the
// main layout's ballots / thresholds of the block they belong to preset to "all written", so that the peak pick
// sees one score array with one geometry.  Which blocks a haystack gets depends on its own length only: its bits
// do not depend on the batch it travels in.
struct TailPlan {
    bool on;
    long long T;      // first score of the tail (a multiple of the main plan's hop, hence of kTile)
    Geometry g;       // the smaller plan's layout for scores [T, out_count): one pair
};
// Half-precision levels (option "half_pipeline"): 1 = the work matrix travels through HBM as f16,
// butterflies in f32; 2 = K2's butterflies in packed f16 as well.  The scales keep every stored
// or f16-computed value inside f16's range: level 1 normalises K2's product by the needle energy
// (times a fixed gain); level 2 scales the row by 2^-7 on the way into K2 (a full-scale tone then
// peaks at 2^15 in the forward spectrum) and the needle spectrum to an rms of 1/8 per bin.  K3
// divides the scales out in f32.
struct HalfScale {
    int level;
    float pre, hscale;
    float k3(float factor) const { return level ? factor / (hscale * pre) : factor; }
};
// What the transforms of one haystack need of the context's scratch buffers (PassPlan::need), so that a batch can
// size them once, for its largest haystack, before anything is queued (see QueueingScope).
struct Footprint {
    size_t work = 0, stats32 = 0, side = 0, work_tail = 0;
    long long npairs = 0;
    void take(const Footprint& f) {
        work = std::max(work, f.work); stats32 = std::max(stats32, f.stats32); side = std::max(side, f.side);
        work_tail = std::max(work_tail, f.work_tail);
        npairs = std::max(npairs, f.npairs);
    }
};
// Which path one haystack takes for (needle, options, score count) -- THE place that decides it (pass_plan,
// am_correlate.hip); run_correlation, the batch engine and streaming ingest all read the answer here.
enum class PassKind { Direct, Partitioned, Transform };   // direct summation (tiny needle) / one pass per needle segment / one pass
struct PassPlan {
    PassKind kind = PassKind::Direct;
    // Transform:
    Geometry g{};                      // the whole haystack's block layout
    const Plan* pl = nullptr;          // ... its plan, the needle's spectrum on it and the half-precision scales
    const float2* hc = nullptr;
    HalfScale hs{};
    bool fused = false;                // K3 carries the score scan (level-0 summary, ballots, thresholds)
    TailPlan tail{};                   // the odd last block on a smaller plan (tail.on), with its plan and spectrum
    const Plan* tail_pl = nullptr;
    const float2* tail_hc = nullptr;
    HalfScale tail_hs{};
    long long nblocks = 0, npairs = 0; // of the main pass (without the tail's block)
    long long ppg = 0;                 // block pairs per launch
    long long main_count = 0;          // scores of the main pass (tail.T, or all)
    // Partitioned: one plan per needle segment (am_needle::segments)
    std::vector<PassPlan> parts;
    Footprint need;                    // what the pass needs of the scratch buffers
    // The samples block pair q of the main pass reads, and the tail's pair.  K1 loads a full N samples per block,
    // starting at block * hop (am_fft.hip, k1_cols_fwd_*), and hop may have been rounded down to a multiple of kTile:
    // pair q reads [2q hop, (2q + 1) hop + N), or [2q hop, 2q hop + N) when its second block does not exist -- up to
    // kTile - 1 samples more than the scores it yields depend on, and a NaN there still poisons the whole pair.
    Segment pair_reads(long long q, long long len) const {
        const long long last_block = (2 * q + 1 < nblocks) ? 2 * q + 1 : 2 * q;
        return Segment{2 * q * g.hop, std::min(len, last_block * g.hop + g.N)};
    }
    Segment tail_reads(long long len) const { return Segment{tail.T, std::min(len, tail.T + (tail.g.nblocks - 1) * tail.g.hop + tail.g.N)}; }
};
// One part of a haystack that is split over several devices (am_match_part_device, am_pool_match_long*): the
// buffer holds the samples from window `first_window` on, only its first `max_windows` windows belong to
// this part (the samples behind them are the last window's overlap), and the peaks come back unmerged, in
// window order, at their positions in the whole haystack -- calc_chunks up to audio_matcher.rs:131.
struct PartSpec {
    size_t max_windows;
    uint64_t first_sample;            // position of the part's first sample in the whole haystack
    size_t chunk_base, chunk_total;   // for the per-chunk progress events: this part's first window, windows of the whole haystack
    std::vector<am_peak>* raw;        // out
};
// Streaming ingest (am_match_stream_*): the block pairs [0, pairs_done) of the one haystack were
// computed while its samples arrived, into buffers the stream object owns.
struct StreamPre {
    float* scores;
    DevBuf* stats32; DevBuf* side;
    long long pairs_done;
    long long layout_nblocks;   // the block count the early pairs laid the flag buffer out for (ScanRequest::side_nblocks)
};

inline const void* advance_src(const void* src, size_t elements) {
    return static_cast<const char*>(src) + sample_bytes(elements);
}

// ---- am_context.hip ----
Opts snapshot_opts(const am_needle* h);
// While an OptsPin lives, snapshot_opts on this thread returns the options it holds (a monitor's calls see the options
// read at am_monitor_begin, whatever am_set_option did since).
extern thread_local const Opts* t_opts_pin;
struct OptsPin {
    const Opts* prev;
    explicit OptsPin(const Opts* o) : prev(t_opts_pin) { t_opts_pin = o; }
    ~OptsPin() { t_opts_pin = prev; }
    OptsPin(const OptsPin&) = delete;
    OptsPin& operator=(const OptsPin&) = delete;
};
int check_needle(const am_needle* h);
// a handle over d_needle (n samples, owned by the handle from here on, freed if this fails) with its energy measured
int create_needle_common(Ctx* c, float* d_needle, size_t n, am_needle** out);
HalfScale half_scale(const am_needle* h, const Opts& o, const PlanDev& pl);
int needle_k2_spectrum(am_needle* h, const Opts& o, const Plan* pl, const float2** hc, HalfScale* hs);

// ---- am_norm.hip ----
// Option "score_norm" as a call sees it: on, the needle's energy and the floor (scores of windows with less energy are 0);
// for a masked handle the kept spans (device table of the handle, n_kept > 0) and the energy of the kept samples
struct NormSpec { bool on; double energy, thr; const long long* kept; int n_kept; };
NormSpec norm_spec(const am_needle* h, const Opts& o);
int norm_check(const NormSpec& ns, int scale);   // AM_ERR_INVALID_ARG unless the scale is AM_SCALE_LIB (when on)
float norm_factor(const NormSpec& ns);           // K3's factor under score_norm: 1 / sqrt(needle energy)
int norm_reserve(Ctx* c, long long max_src_len);
// scores [a, b) of the window sequence of src (window of score t = [t - lead, t - lead + s)), normalised in place on `st`
int normalise_scores(Ctx* c, hipStream_t st, const NormSpec& ns, const void* src, long long src_len, int src_kind, long long lead,
                     long long s, float* scores, long long a, long long b);
#define AM_NORM_UNSUPPORTED "score_norm: not supported by this entry point"

// ---- am_hits.hip: per-hit scoring, and the frame every per-hit family's three call forms run in ----
double hit_floor(const am_needle* h);         // the floor on E_w the NCC path applies (process option score_norm_floor_db)
double hit_floor_ratio(const am_needle* h);   // ... as a ratio to the needle's energy: 10^(-score_norm_floor_db / 10)
// Which hit of a call (for error messages): hit `hit` of pair `pair` = (haystack `hay`, needle `needle`), pair < 0: a
// single-haystack call
struct HitWhere { long long pair; size_t hay, needle, hit; };
std::string hit_pair_name(const HitWhere& w);   // "pair p (haystack k, needle j): ", or "" for a single-haystack call
std::string hit_needle_name(long long j);       // "needle j: ", or "" for j < 0 (a single-haystack call)
// AM_ERR_INVALID_ARG (message: names the pair of `where`) unless p is device memory of `device`
int hit_check_device(const void* p, int device, const HitWhere& where);
// the table entry of hit pk of haystack `hay` (its samples from element 0; `len` elements), or AM_ERR_INVALID_ARG
// (message: names `where`) when the needle does not fit behind pk.start
int hit_desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double thr,
             const HitWhere& where, HitDesc* d);

// What the host and _device forms check before they look at a hit, in this order: the needle handle, the sample format,
// n == 0 (*done: nothing to do), the pointers (`params`: the family's parameter block)
int hit_single_prelude(const am_needle* h, int sample_format, size_t n, const void* hay, const am_peak* peaks, const void* out,
                       const void* params, bool* done);
// ... and the _batch_device form: the sample format, an empty call, the pointers, *total = sum(min(n_peaks, cap)) (0:
// nothing to do); then the needle handles and that they share a device
int hit_batch_counts(size_t n_needles, size_t n_hay, int sample_format, const void* needles, const void* d_haystacks, const void* lens,
                     const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks, const void* out, const void* params, size_t* total);
int hit_batch_needles(const am_needle* const* needles, size_t n_needles);
// r[i]: the elements of the host haystack hit i reads.  Merges them (am_spans.h), copies the merged spans one after the
// other into c->hit_stage on c's stream; at[i]: where element r[i].lo lies on the device
int stage_spans(Ctx* c, const void* haystack, const HitRange* r, size_t n, const void** at);
// The table and the results of a call: sizes c->hit_tab / hit_out and the pinned hit_io (the table, the results behind
// it); rows [off, off + bytes) of the table through the pinned side to the device; the results back, waited for
int hit_io_reserve(Ctx* c, size_t tab_bytes, size_t out_bytes);
int hit_table_put(Ctx* c, const void* rows, size_t off, size_t bytes);
int hit_results_get(Ctx* c, size_t tab_bytes, size_t out_bytes, const void** res);

// A family F names its table entry (Desc; its member `win` points at the samples), its record (Rec) and
//   params()                  its parameter block, for the null check
//   recs()                    records per hit
//   check_call()              the parameters by themselves: a batch call checks them before it looks at a needle handle
//   check(h, j)               the parameters against needle h (hit_needle_name(j) for messages)
//   floor(h)                  what it reads of h's options, once per call and needle
//   desc(h, hay, len, fmt, pk, floor, where, &d)   the table entry of one hit, or its refusal
//   span(h, t, len)           the elements of the haystack a hit at t reads
//   score(c, hits, out)       the kernels: every hit of the table, out[i] the host destination of hit i's records

// the host form's staging: every hit's `win` moves from the host haystack into its span's copy on the device
template <class F>
int stage_host_spans(const F& f, Ctx* c, const am_needle* h, const void* haystack, size_t len, const am_peak* peaks,
                     std::vector<typename F::Desc>& hits) {
    const size_t n = hits.size();
    std::vector<HitRange> r(n);
    std::vector<const void*> at(n);
    for (size_t i = 0; i < n; ++i) r[i] = f.span(h, (size_t)peaks[i].start, len);
    int rc;
    if ((rc = stage_spans(c, haystack, r.data(), n, at.data()))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const size_t e = (size_t)(static_cast<const char*>(hits[i].win) - static_cast<const char*>(haystack)) / 4;
        hits[i].win = advance_src(at[i], e - r[i].lo);
    }
    return AM_OK;
}

// the host form (on_host) and the _device form
template <class F>
int hit_call(const F& f, bool on_host, const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak* peaks,
             size_t n, typename F::Rec* out) {
    bool done = false;
    int rc = hit_single_prelude(h, sample_format, n, hay, peaks, out, f.params(), &done);
    if (rc || done) return rc;
    if ((rc = f.check_call()) || (rc = f.check(h, -1))) return rc;
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!on_host && (rc = hit_check_device(hay, c->device, HitWhere{-1, 0, 0, 0}))) return rc;
    const double floor = f.floor(h);
    std::vector<typename F::Desc> hits(n);
    std::vector<typename F::Rec*> dst(n);
    for (size_t i = 0; i < n; ++i) {
        if ((rc = f.desc(h, hay, len, sample_format, peaks[i], floor, HitWhere{-1, 0, 0, i}, &hits[i]))) return rc;
        dst[i] = out + i * f.recs();
    }
    if (on_host && (rc = stage_host_spans(f, c, h, hay, len, peaks, hits))) return rc;
    return f.score(c, hits, dst.data());
}

// the _batch_device form: pair (k, j) = haystack k against needle j, its hits in slots [pair * cap, pair * cap + n_peaks[pair])
template <class F>
int hit_call_batch(const F& f, const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks, const size_t* lens,
                   size_t n_hay, int sample_format, const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                   typename F::Rec* out) {
    size_t total = 0;
    int rc = hit_batch_counts(n_needles, n_hay, sample_format, needles, d_haystacks, lens, peaks, cap_per_pair, n_peaks, out, f.params(), &total);
    if (rc || total == 0) return rc;
    if ((rc = f.check_call()) || (rc = hit_batch_needles(needles, n_needles))) return rc;
    for (size_t j = 0; j < n_needles; ++j)
        if ((rc = f.check(needles[j], (long long)j))) return rc;
    Ctx* c = needles[0]->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    std::vector<double> floor(n_needles);
    for (size_t j = 0; j < n_needles; ++j) floor[j] = f.floor(needles[j]);
    std::vector<typename F::Desc> hits;
    std::vector<typename F::Rec*> dst;
    hits.reserve(total);
    dst.reserve(total);
    for (size_t k = 0; k < n_hay; ++k) {
        bool checked = false;
        for (size_t j = 0; j < n_needles; ++j) {
            const size_t pair = k * n_needles + j, np = std::min(n_peaks[pair], cap_per_pair);
            if (np == 0) continue;
            if (!checked) {   // (once per haystack; messages are spelled out only for a refusal)
                const HitWhere w{(long long)pair, k, j, 0};
                if (!d_haystacks[k]) return fail(AM_ERR_INVALID_ARG, hit_pair_name(w) + "null haystack");
                if ((rc = hit_check_device(d_haystacks[k], c->device, w))) return rc;
                checked = true;
            }
            for (size_t i = 0; i < np; ++i) {
                typename F::Desc d{};
                const size_t slot = pair * cap_per_pair + i;
                if ((rc = f.desc(needles[j], d_haystacks[k], lens[k], sample_format, peaks[slot], floor[j], HitWhere{(long long)pair, k, j, i}, &d)))
                    return rc;
                hits.push_back(d);
                dst.push_back(out + slot * f.recs());
            }
        }
    }
    return f.score(c, hits, dst.data());
}

// The round trip of a table whose kernels write n_parts partial records of part_bytes (and one flag word each) and
// `recs` records per hit: the table up through pinned memory (no staging in the runtime, which is most of a small
// call's time), launch(table, parts, flags, results) on c's stream, the results back and out to out[i]
template <class Desc, class Rec, class Launch>
int hit_round_trip(Ctx* c, const std::vector<Desc>& hits, size_t part_bytes, size_t n_parts, size_t recs, Rec* const* out, Launch launch,
                   int prof_class = KN_OTHER) {
    const size_t n = hits.size(), tab_bytes = sizeof(Desc) * n, out_bytes = sizeof(Rec) * recs * n;
    int rc;
    if ((rc = hit_io_reserve(c, tab_bytes, out_bytes)) || (rc = c->hit_parts.ensure(part_bytes * n_parts)) ||
        (rc = c->hit_flags.ensure(sizeof(unsigned) * n_parts)) || (rc = hit_table_put(c, hits.data(), 0, tab_bytes)))
        return rc;
    {
        ProfScope ps(c, prof_class, c->stream);
        AM_HIP(launch(static_cast<const Desc*>(c->hit_tab.p), static_cast<double*>(c->hit_parts.p), static_cast<unsigned*>(c->hit_flags.p),
                      static_cast<Rec*>(c->hit_out.p)));
    }
    const void* res = nullptr;
    if ((rc = hit_results_get(c, tab_bytes, out_bytes, &res))) return rc;
    for (size_t i = 0; i < n; ++i) std::memcpy(out[i], static_cast<const Rec*>(res) + i * recs, sizeof(Rec) * recs);
    return AM_OK;
}

// ---- am_bands.hip ----
// AM_ERR_INVALID_ARG unless bp is a valid request (the table of a frame size: band_table, am_frames.h)
int band_check_params(const am_band_params* bp);

// ---- am_estimate.hip ----
// slots of the sorting network a call with n rows runs: 0 for AM_EST_MEAN (no sort), else 8, 16, 32 or 64; -1: too many rows
int estimate_slots(int method, int n);

// ---- am_correlate.hip ----
int plan_geometry(size_t s, long long out_count, const Opts& o, Geometry* g);
bool plan_fuses_scan(const PlanDev& pl, const Geometry& g);   // K3 of this plan, at this hop, carries the score scan
bool tail_plan(size_t s, long long out_count, const Opts& o, const Geometry& g, TailPlan* t);
// allow_tail: the caller's passes may leave the odd last block to a TailPlan (not streaming ingest, whose early pairs
// fix the layout; not an accumulating segment pass; not with lead != 0).  Builds the plans and the needle spectra the
// haystack will use (building one runs kernels and waits for them): call it before anything is queued.
int pass_plan(am_needle* h, const Opts& o, long long out_count, bool allow_tail, PassPlan* pp);
Job tail_job(const TailPlan& t, const void* d_src, long long src_len, long long out_count, int src_kind);
// a plan's ballot layout: column tiles per block (one threshold each), 64-bit ballot words per block
struct BallotLayout { size_t tiles, words; };
inline BallotLayout ballot_layout(int log_n1, int log_n2) {
    const size_t tiles = (size_t)1 << (log_n2 - kColsLog);
    return BallotLayout{tiles, tiles << (log_n1 - 6)};
}
size_t sparse_bytes(long long nblocks, const PlanDev& pl);
void fill_scan_cfg(ScanCfg* cfg, void* stats32, void* side, long long nblocks, const PlanDev& pl, float margin, float hist_min,
                   long long seg_c, long long seg_d);
SparseScores sparse_view(const ScanCfg& cfg, long long hop, const PlanDev& pl);
bool needle_is_segmented(const am_needle* h, const Opts& o);
float write_margin(const Opts& o, const am_match_params* p);
// plan: the haystack's pass_plan when the caller has it (a batch plans before it queues); otherwise planned here, with
// a tail allowed when a scan is requested and lead == 0
int run_correlation(am_needle* h, const Opts& o, const void* d_src, long long src_len, long long lead,
                    float* d_dst, long long out_count, float factor, const ScanRequest* scan_req = nullptr, ScanResult* res = nullptr,
                    int src_kind = 0, const PassPlan* plan = nullptr);
int nonfinite_flags(Ctx* c, const float* d_src, const Segment* ranges, int n, int* flags);
float scale_factor(const am_needle* h, int scale, size_t w);
void make_segments(size_t len, size_t s, const am_match_params* p, bool drop_tail, std::vector<Segment>& segs,
                   std::vector<size_t>* widths = nullptr, size_t max_windows = (size_t)-1);
int upload_segments(Ctx* c, const std::vector<Segment>& segs);
int prepare_results(Ctx* c, size_t nhdr, size_t arena_entries, PeakArena* arena);
// The pick's hand-over area for chunks with many candidate tiles (WideState, am_kernels.h), one entry per chunk of a
// launch; the picks of one call run in stream order, so one area serves them all.  wide_ctl holds the control words as
// five arrays of n entries, one after the other: best (8 bytes), then state, count, seg_min, ntiles (4 bytes each).
constexpr size_t kWideCtlBytes = sizeof(unsigned long long) + sizeof(int) + sizeof(unsigned) + sizeof(float) + sizeof(int);
int wide_reserve(Ctx* c, size_t n);         // sizes the area for n chunks
WideState wide_carve(Ctx* c, size_t n);     // the area as it is, laid out for n chunks
// side: the set whose tile summaries and peak lists the pick uses; bad: host-visible word the summary kernels set when a
// score is not finite, or null; res: what the pass that wrote the scores reported (null: plain scores)
int launch_pick(Ctx* c, ScoreSide& side, const float* d_scores, long long n_scores, int seg_off, int nsegs,
                float min_prom, long long min_dist, int* bad, const ScanResult* res, int hdr_off,
                const PeakArena& arena, const PeakPolicy& pol, hipStream_t st = nullptr, bool only_failed = false);
int pick_chunk_big(Ctx* c, const float* d_scores, long long n_scores, int seg_idx, const Segment& sg,
                   float min_prom, long long min_dist, const ScanResult* res, float seg_min,
                   std::vector<am_peak>& all, const PeakPolicy& pol);
// am_find_peaks on a resident score array: one chunk [0, n) (am_api.hip)
int find_peaks_host_array(Ctx* c, const float* d_scores, long long n, float min_prom, long long min_dist, std::vector<am_peak>& all);
// ---- am_best.hip ----
// The AM_MODE_VALID scores of samples x[0, w) into d_out[0, w - S + 1), as am_correlate computes them for a finite
// input: the same run_correlation with lead 0, the same half-precision redo, normalise_scores under score_norm.
int valid_scores(am_needle* h, const Opts& o0, const NormSpec& nrm, float factor, const float* d_x, long long w, float* d_out);
int best_transitions(Ctx* c, const float* d_x, long long n, std::vector<long long>& trans);
int best_select(Ctx* c, const float* d_g, long long n, float min_prom, long long min_dist, size_t k, const PeakPolicy& pol,
                std::vector<am_peak>& res);
// The score array am_match_best selects from and am_match_trace reduces: the AM_MODE_VALID scores of one resident haystack
// (len >= S) in the context's best_scores, after the bit-exact down-mix of an i16 stereo haystack; a window that holds
// a non-finite sample scores NaN, every finite stretch of at least S samples is correlated on its own.  *n = len - S + 1.
int haystack_scores(am_needle* h, const Opts& o, const void* d_hay, size_t len, int sample_format, int scale, const float** d_scores,
                    long long* n);
// ... in its two steps, for a caller that scores one haystack against many needles (am_discover.hip): the samples the
// haystack is correlated as (an i16 stereo haystack down-mixed into `mono`) with their non-finite runs, once; then the
// scores of one needle over them
struct HaySamples { const float* d_x = nullptr; size_t len = 0; std::vector<long long> trans; };
int haystack_prepare(Ctx* c, const void* d_hay, size_t len, int sample_format, DevBuf& mono, HaySamples* hs);
int prepared_scores(am_needle* h, const Opts& o, const HaySamples& hs, int scale, const float** d_scores, long long* n);
int match_best_one(am_needle* h, const void* d_hay, size_t len, int sample_format, const am_best_params* bp, am_peak* out,
                   size_t* n_out);
// ---- am_discover.hip ----
// The record of the resident scores d_g[0, n) (n >= 1) into d_out (device memory), on the context's stream: the rule of
// am_probe_scores with the excluded range [ex_lo, ex_hi) and sep >= 1
int probe_reduce(Ctx* c, const float* d_g, long long n, uint64_t ex_lo, uint64_t ex_hi, uint64_t sep, uint64_t probe, am_probe_hit* d_out);
// ---- am_trace.hip ----
int trace_check_bin(uint64_t bin);
int trace_reduce(Ctx* c, const float* d_g, long long n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out);
int match_trace_one(am_needle* h, const void* d_hay, size_t len, int sample_format, const am_trace_params* tp, am_trace_bin* out,
                    size_t cap, size_t* n_out);
int merge_peaks(std::vector<am_peak>& all, const am_match_params* p, bool from_filtered, am_peak* out, size_t cap, size_t* n_out);
// what merge_settle carries from one piece of a sorted list to the next: the element before the next one, the last one kept
struct MergeCursor { am_peak prev{}, kept{}; bool has_prev = false, has_kept = false; };
// the longest prefix of sorted[0, n) whose fates under merge_peaks are final (no element still to come starts before
// `horizon`): settles it into `cur`, appends the kept ones to *kept_out (if given), returns its length
size_t merge_settle(const am_match_params* p, bool from_filtered, MergeCursor& cur, const am_peak* sorted, size_t n,
                    uint64_t horizon, bool ended, std::vector<am_peak>* kept_out);
void append_header_peaks(const SegHeader& hd, const PeakArena& arena, std::vector<am_peak>& all);

// ---- am_engine.hip ----
int match_many(am_needle* h, const void* const* d_hays, const size_t* lens, size_t n_hay,
               const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out, int src_kind = 0,
               size_t index_base = 0, size_t index_stride = 1, bool fire_hooks = true, const StreamPre* pre = nullptr,
               const PartSpec* part = nullptr);
int match_multi_many(am_needle* const* needles, size_t nn, const void* const* d_hays, const size_t* lens, size_t n_hay,
                     int src_kind, const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out,
                     size_t index_base = 0, size_t index_stride = 1, const uint64_t* overlaps = nullptr, bool varlen = false);

}  // namespace am
