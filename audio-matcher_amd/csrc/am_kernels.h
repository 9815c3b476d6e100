// am_kernels.h -- device-side job descriptors and launcher prototypes shared by
// the HIP translation units of libaudiomatch_amd.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/audiomatch.h"

namespace am {

// One overlap-save job: a (virtually zero-padded) input signal and the score
// array it produces.  score[j] = sum_n X[j + n - lead] * needle[n], X = 0
// outside [0, src_len).  Block b reads input [b*hop - lead, b*hop - lead + N)
// and yields scores [b*hop, b*hop + hop).  Two blocks are packed into one
// complex transform (re = block 2g, im = block 2g+1).
struct Job {
    const void* src;      // device: f32 mono samples, or interleaved i16 stereo frames (src_kind 1)
    long long src_len;    // samples / frames
    long long lead;       // virtual zeros in front of src[0]
    float* dst;           // device, out_count scores
    long long out_count;
    int hop;              // new scores per block (<= N - S + 1)
    int nblocks;          // ceil(out_count / hop)
    int first_pair;       // first pair handled by this launch (slot 0 of work)
    int src_kind;         // 0 = f32 mono, 1 = i16 stereo (down-mixed in K1, mp3_reader.rs:28-37)
};

// Factorisation N = N1 * N2 of the complex transform and its twiddle tables.
struct PlanDev {
    int logN, logN1, logN2, logLo;
    const float2* tw1;    // W_N1^k, k < N1/2 (forward sign)
    const float2* tw2;    // W_N2^k, k < N2/2
    const float2* twlo;   // W_N^m,            m < 2^logLo
    const float2* twhi;   // W_N^(m << logLo), m < 2^(logN - logLo)
    // The same two tables with every entry's FOURTH power beside it, (w.x, w.y, w^4.x, w^4.y): one 16-byte
    // fetch per level yields W_N^m and W_N^(4m), the two seeds of a twiddle chain (twiddle_chain(x, base, step, step4)).
    const float4* twlo4;
    const float4* twhi4;
    // K2's twiddle seeds per lane, ready to fetch (N2 = 8192 only): k2j[2t] = (W^(2t), W^(2t+1)), k2j[2t+1] = their
    // fourth powers, t < 256; k2c[2c] = (W^(32c), W^(32c+16)), k2c[2c+1] = their fourth powers, c < 16 (W = W_8192).
    const float4* k2j;
    const float4* k2c;
    // constant tables of the matrix-core row kernel (k2_rows_m16, N2 = 8192 only; nullptr otherwise): DFT-16 and DFT-32
    // operands in the lane layout of v_mfma_f32_16x16x32_f16 and every lane's twiddles as h2 (am_fft.hip kMf*)
    const unsigned* mf;
};

constexpr int kColsLog = 5;            // B = 32 columns per K1/K3 workgroup
constexpr int kCols = 1 << kColsLog;
constexpr int kTile = 1024;            // score tile of the min/max summary
constexpr int kFftThreads = 256;

// one reference chunk's slice of a score array (audio_matcher.rs:119-126)
struct Segment {
    long long a, b;       // [a, b) in the score array
};

// half: 0 = f32 work matrix; 1 = one __half2 per point, f32 butterflies; 2 = packed f16 butterflies too
// (K2 and K1 whole; K3's first pass -- its second pass and the score scan stay f32)
// Every launcher returns hipErrorInvalidValue, and launches nothing, for a combination of plan, sample kind, half level
// and form that has no kernel (the empty rows of am_fft.hip's tables): a half level on the 1024-row plan, i16 samples or
// a half level on the 512 x 16384 plan, accumulate with a half level or on the 256-row plan.  The generic kernels
// (N below 2^21) have no half form and ignore the level.
hipError_t launch_k1(hipStream_t st, const Job& job, int npairs, float2* work, const PlanDev& pl, int half = 0);
// dst == nullptr: in place; otherwise the result goes to a second work matrix
// tail: the launch belongs to a haystack's odd last block (am_correlate.hip, run_tail_block) -- the same row kernels under
// names of their own (tail_rows_*), so that a profile's per-kernel averages stay those of the main pass
hipError_t launch_k2(hipStream_t st, int npairs, float2* work, const float2* hc, const PlanDev& pl, float2* dst = nullptr,
                     int half = 0, float hscale = 1.0f, float pre = 1.0f, bool tail = false);
// half = 2: hc points at the __half2 form of the spectrum (launch_spectrum_to_half), hscale already in it
hipError_t launch_spectrum_to_half(hipStream_t st, const float2* hc, long long n, float scale, unsigned* out);
// option "k2_mfma" (an A/B experiment for half_pipeline = 2): the row kernel's butterflies on the matrix cores;
// it takes the spectrum conjugated and in [a'][b'][c'] order (launch_spectrum_to_half_mfma)
void set_k2_mfma(int on);
bool k2_mfma_enabled();
int k2_mfma_table_dwords();
hipError_t launch_spectrum_to_half_mfma(hipStream_t st, const float2* hc, long long n, float scale, unsigned* out);
hipError_t launch_k2_spectrum(hipStream_t st, float2* work, float2* hc_out, const PlanDev& pl);
// A group of needles sharing one forward row transform (r16 rows, f32 storage only):
// needle j multiplies with hc[j] and writes its inverse rows to dst[j].
constexpr int kMaxNeedleGroup = 8;
struct K2Group {
    const float2* hc[kMaxNeedleGroup];
    float2* dst[kMaxNeedleGroup];
    int n;
};
bool plan_k2_has_group(const PlanDev& pl);
hipError_t launch_k2_group(hipStream_t st, int npairs, const float2* work, const K2Group& grp, const PlanDev& pl);
// The score scan fused into K3 (the plans of plan_has_scan).  stats32 == nullptr disables it
// (plain correlation: every score is written).
struct ScanCfg {
    float2* stats32;          // (min,max) per 32 consecutive scores, always written
    // which 32-score runs were written: one 64-bit word per (block, column tile, wavefront of the tile's
    // workgroup), bit (a << 2) | j = row a * (rows / 16) + 4 * wavefront + j of the tile
    unsigned long long* wbits;
    float* tile_theta;        // [block][column tile]: the write threshold that tile used
    float margin;             // a run's raw scores are written when its maximum >= min(the tile's minimum over its block
                              // pair, hist_min) + margin (and for runs that hold a chunk edge); margin < 0: every run
    float hist_min;           // lowest chunk minimum of the needle's recent haystacks (FLT_MAX: none)
    long long seg_c, seg_d;   // chunk geometry: runs that hold score i*seg_c or i*seg_c + seg_d are chunk edges
    double inv_c;             // 1.0 / seg_c
    // device-side redo: only the block pairs p with only_pairs[p] != 0 run (nullptr: all).  The peak pick
    // marks the pairs of the chunks whose certificate failed (SparseScores::redo_pairs), K3 then runs once
    // more for those pairs with every run written, from the work matrix it still has.
    const int* only_pairs;
    int redo_tiles;           // (set by launch_k3 for that launch: tiles in the launch, walked by a small grid)
    // Chunk edges per block pair of the launch, worked out on the host (launch_k3): for slot s of the launch the first
    // score i*seg_c and the first score i*seg_c + seg_d at or behind the start of block A (0, 1) and of block B (2, 3),
    // relative to that start, INT_MAX when out of reach.  edges_n = 0 (more pairs than kMaxEdgeSlots, or chunks
    // shorter than a block): the kernel works them out itself.
    static constexpr int kMaxEdgeSlots = 64;
    int edges_n;
    int edge_rel[kMaxEdgeSlots][4];
};
// accumulate: the scores are added to what job.dst holds (every run written; f32 work matrix only; the 512- and
// 1024-row plans and the generic ones -- the segments of a partitioned needle never run on the 256-row plan)
hipError_t launch_k3(hipStream_t st, const Job& job, int npairs, const float2* work,
                     const PlanDev& pl, float out_scale, const ScanCfg& scan, int half = 0, bool accumulate = false);
// K3 for the needles of a group in ONE launch (BASELINE configs[3]): needle z = blockIdx.y reads its own inverse rows
// and writes its own scores, summary, ballots and thresholds; block layout and chunk geometry are the group's (`job`,
// `scan`: their dst / stats32 / wbits / tile_theta / hist_min fields are replaced per needle).  f32 work matrices of the
// 512- and 256-row plans.
struct K3Group {
    int n;
    const float2* work[kMaxNeedleGroup];
    float* dst[kMaxNeedleGroup];
    float2* stats32[kMaxNeedleGroup];
    unsigned long long* wbits[kMaxNeedleGroup];
    float* tile_theta[kMaxNeedleGroup];
    float hist_min[kMaxNeedleGroup];
    float out_scale[kMaxNeedleGroup];
    // Needles of different lengths on one block layout (am_match_multi_varlen*): member z's scores end at out_count[z]
    // (scores at or beyond it are neither stored nor summarised, balloted or thresholded), its chunk edges are
    // i * seg_c and i * seg_c + seg_d[z].  The launch's own job.out_count / scan.seg_c / seg_d are those of the layout
    // (scan.seg_c = 0 when the members' edges differ: every member then works out its own edges).
    long long out_count[kMaxNeedleGroup];
    long long seg_d[kMaxNeedleGroup];
    long long seg_c;
    double inv_c;
};
bool plan_k3_has_group(const PlanDev& pl);
// The odd last blocks of several haystacks of a batch (am_engine.hip, launch_tail_batch; TailPlan in am_internal.h) as ONE launch each of K1 / K2 / K3 on the
// 256-row plan: entry z = blockIdx.y is one block pair of a job of its own (source, scores, summary), work slot z.
// Every run of raw scores is written (no ballots, no thresholds).
constexpr int kMaxTailBatch = 8;
struct TailBatch {
    int n;
    const void* src[kMaxTailBatch];      // the haystack's samples from the tail's first score on
    long long src_len[kMaxTailBatch];
    float* dst[kMaxTailBatch];           // out_count scores
    long long out_count[kMaxTailBatch];
    float2* stats32[kMaxTailBatch];      // their level-0 summary
};
// hop, src_kind: shared by the entries (one needle, one sample format)
hipError_t launch_tail_batch_k1(hipStream_t st, const TailBatch& tb, int hop, int src_kind, float2* work, const PlanDev& pl, int half);
hipError_t launch_tail_batch_k3(hipStream_t st, const TailBatch& tb, int hop, const float2* work, const PlanDev& pl, float out_scale, int half);
// A tail's scores and summary into the score-side buffers the pick reads, and the main layout's ballots / thresholds of
// the block they belong to set to "every run written" (one small launch on the pick's stream)
// several needles (K3Group): the ballots and thresholds of block `blk` of the main layout set to "every run written"
// for every needle of the group, one launch
hipError_t launch_tail_preset_group(hipStream_t st, const K3Group& grp, long long blk, int log_n1, int log_n2);
hipError_t launch_tail_commit(hipStream_t st, const float* tail_scores, float* scores, long long n, const float2* tail_stats32, float2* stats32,
                              unsigned long long* wbits, long long words, float* theta, int tiles);
hipError_t launch_k3_group(hipStream_t st, const Job& job, int npairs, const K3Group& grp, const PlanDev& pl, const ScanCfg& scan);
// needles of at most this many samples are correlated by direct summation (no transform)
constexpr int kDirectMaxNeedle = 64;
hipError_t launch_direct(hipStream_t st, const Job& job, const float* needle, int s, float out_scale);
bool plan_is_r16(const PlanDev& pl);
bool plan_is_c512(const PlanDev& pl);    // N = 2^22 = 512 x 8192, 512-thread column kernels
bool plan_is_c512w(const PlanDev& pl);   // N = 2^23 = 512 x 16384: the 512-row column kernels on longer rows (measurement only: no row kernel yet)
bool plan_is_c1024(const PlanDev& pl);   // N = 2^23 = 1024 x 8192, 1024-thread column kernels (f32 work matrix only)
bool plan_has_scan(const PlanDev& pl);   // K3 of this plan carries the fused score scan
bool plan_k2_is_r16(const PlanDev& pl);
hipError_t fft_kernels_init();

// flags[r] = 1 if x[ranges[r].a .. ranges[r].b) holds a non-finite sample (f32 sources only)
hipError_t launch_nonfinite_ranges(hipStream_t st, const float* x, const Segment* ranges, int nranges, int* flags);
// bad (optional, host-visible word): set to 1 when a score is not finite
hipError_t launch_tile_stats(hipStream_t st, const float* g, long long n, float2* stats, int* bad = nullptr);
// The picks of a needle group as one set of launches (several needles against one haystack): needle z (blockIdx.y / .z)
// works on its own score array, summaries, flags and thresholds; chunk list and geometry are shared, results are laid
// out needle after needle (n = 0: an ordinary, single pick).
struct PickGroup {
    int n;
    const float* g[kMaxNeedleGroup];
    float2* stats[kMaxNeedleGroup];
    const float2* stats32[kMaxNeedleGroup];
    const unsigned long long* wbits[kMaxNeedleGroup];
    const float* theta[kMaxNeedleGroup];
    int hdr_off[kMaxNeedleGroup];   // result headers of needle z: hdr + hdr_off[z] (relative to the pointer the launch is given)
};
hipError_t launch_stats_reduce(hipStream_t st, const float2* stats32, long long n, float2* stats, int* bad = nullptr,
                               const PickGroup* grp = nullptr);
// per-chunk result header: the count, an overflow flag and the first few peaks
// inline, so that the common case needs a single small device-to-host copy
constexpr int kInlinePeaks = 4;
struct SegHeader {
    int n;
    int overflow;      // bit 0: more than AM_MAX_PEAKS_PER_CHUNK peaks; bit 1: a write threshold was too high for this chunk;
                       // bit 2: more than kInlinePeaks peaks and no room left in the spill arena
    float seg_min;     // (lower bound of the) chunk minimum, for adapting theta
    int arena_off;     // n > kInlinePeaks: the whole list sits at arena.base[arena_off .. arena_off + n)
    am_peak first[kInlinePeaks];
};
// Spill area for the peak lists of chunks with more than kInlinePeaks peaks: a bump
// allocator shared by every chunk of a call (base may be host-mapped memory; cursor is
// device memory zeroed before the first pick of the call).  base == nullptr: no spill.
struct PeakArena {
    am_peak* base;
    unsigned* cursor;
    unsigned cap;
};
// Which raw scores exist (K3 writes them sparsely, run by run): wbits == nullptr means all.
struct SparseScores {
    const unsigned long long* wbits;   // see ScanCfg
    const float2* stats32;
    const float* tile_theta;           // thresholds K3 used (the pick's certificate reads them)
    int hop, log_n2, log_n1;           // block geometry: score n of a block = row (n >> log_n2), column (n & (2^log_n2 - 1))
    double inv_hop;
    int* redo_pairs;                   // per block pair: set by the pick when a chunk fed by the pair fails its certificate (or null)
    unsigned char* fail_flags;         // host-visible, one per chunk of the launch: set when the chunk failed its certificate (or null)
};
// Hand-over of chunks with many candidate tiles from peaks_kernel to peaks_wide /
// peaks_finish (device memory, one entry per chunk of the launch; list: AM_MAX_PEAKS_PER_CHUNK
// entries per chunk).  list == nullptr: every chunk is finished by its one workgroup.
struct WideState {
    int* state;          // 0 = finished by peaks_kernel; bit 0 = handed over, bits 1 / 2 = scan the raw head / tail piece
    unsigned* count;     // peaks appended to the chunk's list (> AM_MAX_PEAKS_PER_CHUNK: overflow)
    float* seg_min;
    unsigned long long* best;   // min_distance >= chunk length: running maximum of the peaks that pass (order-preserving key)
    am_peak* list;
    unsigned cap;        // entries per chunk in list (AM_MAX_PEAKS_PER_CHUNK on the usual path)
    int* ntiles;         // candidate tiles listed for the chunk (-1: not listed, the parts test every tile)
    int* tiles;          // kWideTileList entries per chunk: candidate tiles relative to the chunk's first full tile
};
constexpr int kWideTileList = 1024;
// The rules of find_peaks 0.1 that nothing available offline pins (crate source absent, no reference test; SURVEY.md
// 8c): the defaults are the library's documented choice (oracle/oracle.c), every alternative is implemented in the
// kernels AND in the checker, so that whoever has the crate flips an option instead of rewriting a kernel.
struct PeakPolicy {
    int order;        // 0: prominence filter, then distance filter (default); 1: distance first, then prominence (scipy's order)
    int inclusive;    // the distance filter drops a peak whose distance to a kept, higher one is  0: < min_distance (default)  1: <= min_distance
    int from_start;   // ... measured between  0: plateau middles (start + end) / 2 (default)  1: plateau starts
};
// A chunk with more than AM_MAX_PEAKS_PER_CHUNK peaks passing the prominence filter (rare: a
// min_distance shorter than the chunk and a tiny prominence bound).  launch_peaks_wide_one runs the
// list-building kernel for ONE chunk (wide.state[0] must be 1; wide.cap = 0 only counts);
// launch_peaks_big_finish orders that list by (height descending, position ascending) with a
// radix sort in global memory and applies the greedy min_distance filter through a table of
// min_distance-wide buckets (each holds at most one kept peak).  Scratch: keys 2 x n x 8 bytes,
// idx 2 x n x 4 bytes, table ((b - a) / min_distance + 3) x 8 bytes preset to 0xFF.
hipError_t launch_peaks_wide_one(hipStream_t st, const float* g, long long g_len, const float2* stats, const Segment* d_seg,
                                 float min_prom, long long min_dist, const SparseScores& sp, const WideState& wide, const PeakPolicy& pol);
hipError_t launch_peaks_big_finish(hipStream_t st, const am_peak* list, unsigned n, long long a, long long min_dist,
                                   unsigned long long* keys, unsigned* idx, long long* table, am_peak* out, unsigned* out_n,
                                   const PeakPolicy& pol);
// only_failed: pick only the chunks whose header says "certificate failed" (after the device-side redo of K3)
hipError_t launch_peaks(hipStream_t st, const float* g, long long g_len, const float2* stats,
                        const Segment* d_segs, int nsegs, float min_prom, long long min_dist,
                        am_peak* d_out, SegHeader* d_hdr, const SparseScores& sp, const PeakArena& arena,
                        const WideState& wide, bool only_failed, const PeakPolicy& pol, const PickGroup* grp = nullptr);
// writes sumsq_parts(n) partial sums (one per workgroup) to d_parts
int sumsq_parts(long long n);
hipError_t launch_sumsq(hipStream_t st, const float* x, long long n, double* d_parts);
hipError_t launch_synth(hipStream_t st, float* out, uint32_t seed, uint32_t stream, uint64_t first,
                        long long n, float amp);
hipError_t launch_axpy(hipStream_t st, float* dst, const float* src, long long n, float gain);
hipError_t launch_synth_pcm16(hipStream_t st, int16_t* out, uint32_t seed, uint32_t stream, uint64_t first, long long frames, float amp);
hipError_t launch_add_pcm16(hipStream_t st, int16_t* dst, const int16_t* src, long long frames);
hipError_t launch_pcm_downmix(hipStream_t st, const int16_t* in, long long frames, float* out);

// (l as f32 + r as f32) * 0.5 * (1 / 65535), the down-mix K1 applies (am_fft.hip, downmix_s16), bit for bit: what
// am_norm.hip and am_hits.hip read an i16 stereo frame as
__device__ __forceinline__ float norm_downmix(short2 lr) {
    return __fmul_rn((float)((int)lr.x + (int)lr.y), 0.5f * (1.0f / 65535.0f));
}
// x[u] of a hit's sample pointer (u may be negative) in either sample format, read through the global address space:
// what the per-hit kernels (am_hits.hip, am_segments.hip, am_bands.hip) load; am_resample.hip reads through the same types
typedef __attribute__((address_space(1))) const float gfloat;
typedef __attribute__((address_space(1))) const unsigned guint;   // (one i16 stereo frame)
template <int KIND>
__device__ __forceinline__ float hit_sample(const void* win, long long u) {
    return KIND ? norm_downmix(__builtin_bit_cast(short2, ((guint*)win)[u])) : ((gfloat*)win)[u];
}

// ---- am_norm.hip: window-energy normalisation (option "score_norm") ----
constexpr int kNormBlock = 1024;   // samples per block energy
constexpr int kNormTile = 2048;    // scores per workgroup of the normalising kernel
inline long long norm_blocks(long long src_len) { return (src_len + kNormBlock - 1) / kNormBlock; }
// blk[i] = sum of x^2 over samples [i kNormBlock, (i + 1) kNormBlock) in f64, non-finite samples as 0
hipError_t launch_block_energy(hipStream_t st, const void* src, long long src_len, int src_kind, double* blk);
// scores[t], t in [a, b), window [t - lead, t - lead + s) of src: multiplied by 1 / sqrt(window energy), or 0 when that
// energy is below thr; non-finite scores are left as they are
struct NormJob {
    const void* src;
    long long src_len;
    int src_kind;
    long long lead, s;
    const double* blk;   // launch_block_energy of src
    long long nblk;
    double thr;
    float* scores;
    long long a, b;
    // masked needles: the kept spans [kept[2q], kept[2q + 1]) of the needle, ascending (device memory), n_kept of them,
    // at most kNormMaxKept; the energy is then the sum over these spans only.  n_kept = 0: the whole window [0, s).
    const long long* kept;
    int n_kept;
};
constexpr int kNormMaxKept = AM_MASK_MAX_GAPS + 1;
hipError_t launch_norm_scores(hipStream_t st, const NormJob& j);          // n_kept = 0
hipError_t launch_masked_norm_scores(hipStream_t st, const NormJob& j);   // n_kept > 0

// ---- am_hits.hip: per-hit scoring (am_hit_scores*) ----
constexpr int kHitSlice = 4096;                   // needle samples per workgroup of the slice kernel
constexpr long long kHitMaxGridY = 65535;         // hits per launch of the slice kernel (grid.y)
// One hit of a call, as the kernels read it (the call's hit table, uploaded once)
struct HitDesc {
    const void* win;      // device: sample t of the haystack (f32 mono, or an i16 stereo frame for kind 1)
    const float* needle;  // device: the whole needle
    long long s;          // needle length
    int kind;             // 0 = f32 mono, 1 = i16 stereo (one kind per launch)
    int edge;             // bit 0: x[t - 1] exists, bit 1: x[t + s] exists
    long long t;          // the hit's start in the haystack
    double en, thr;       // sum(needle^2), the floor on the window's energy
    long long part0;      // first partial record of the hit
};
// parts: 4 doubles per slice (corr(t - 1), corr(t), corr(t + 1), E_w), pflags: one word per slice; d_out: n records
hipError_t launch_hit_scores(hipStream_t st, const HitDesc* d_hits, long long n, long long max_slices, int kind, double* parts,
                             unsigned* pflags, am_hit_score* d_out);

// ---- am_mask.hip: the per-hit record of a masked handle (am_hit_mask*) ----
constexpr int kMaskSums = 5;   // doubles per partial record: c_k, E_x^M, c_g, E_x,gaps, E_n,gaps
// One hit of a call, as the kernels read it (the call's hit table, uploaded once)
struct MaskDesc {
    const void* win;         // device: sample t of the haystack (f32 mono, or an i16 stereo frame for kind 1)
    const float* needle;     // device: the handle's needle (gap samples +0)
    const float* orig;       // device: the original samples in the gaps, +0 in the kept spans; null without gaps
    const long long* kept;   // device: the kept spans [kept[2q], kept[2q + 1]), n_kept of them; 0: no mask, every sample is kept
    int n_kept;
    int kind;                // 0 = f32 mono, 1 = i16 stereo (one kind per launch)
    long long s;             // needle length
    double en, thr;          // the kept samples' energy, the floor on E_x^M
    long long part0;         // first partial record of the hit
};
// parts: kMaskSums doubles per slice of kHitSlice needle samples, pflags: one word per slice (bit 0: a non-finite sample
// under a kept span, bit 1: under a gap); d_out: n records
hipError_t launch_hit_mask(hipStream_t st, const MaskDesc* d_hits, long long n, long long max_slices, int kind, double* parts,
                           unsigned* pflags, am_mask_hit* d_out);

// ---- am_segments.hip: per-segment hit scoring (am_hit_segments*) ----
// The slice kernel exists for three radii; a call runs the smallest that holds its R (kSegRadii) and reads the lags
// -R .. R of its records.  A record: c(-RT .. RT), E_w(-RT .. RT), E_n.
constexpr int kSegRadii[3] = {1, 4, 16};
inline int seg_kernel_radius(int r) { return r <= kSegRadii[0] ? kSegRadii[0] : r <= kSegRadii[1] ? kSegRadii[1] : kSegRadii[2]; }
inline int seg_record_len(int rt) { return 2 * (2 * rt + 1) + 1; }   // doubles per partial record
// One hit of a call, as the kernels read it (the call's table, uploaded once); m and R are the call's
struct SegDesc {
    const void* win;      // device: sample t of the haystack (f32 mono, or an i16 stereo frame for kind 1)
    const float* needle;  // device: the whole needle
    long long s;          // needle length
    long long ulo, uhi;   // x[t + u] exists (and is read) for ulo <= u < uhi only: [-R, s + R) clipped to the haystack
    long long part0;      // first partial record of the hit: segment j, slice k at part0 + j * nsl + k
    double floor_ratio;   // 10^(-score_norm_floor_db / 10)
    int kind;             // 0 = f32 mono, 1 = i16 stereo (one kind per launch)
    int nsl;              // slices reserved per segment: ceil(ceil(s / m) / kHitSlice)
};
// parts: seg_record_len(seg_kernel_radius(r)) doubles per slice, pflags: one word per slice; d_out: n * m records
hipError_t launch_hit_segments(hipStream_t st, const SegDesc* d_hits, long long n, int m, int r, int max_nsl, int kind,
                               double* parts, unsigned* pflags, am_hit_segment* d_out);

// the slice launches alone, over n table entries read with m = 1: what am_warp.hip runs over its (hit, rate) entries
hipError_t launch_seg_slices(hipStream_t st, const SegDesc* d_hits, long long n, int m, int r, int max_nsl, int kind, double* parts,
                             unsigned* pflags);

// ---- am_warp.hip: per-hit drift scoring (am_hit_warp*) ----
constexpr int kWarpThreads = 256;          // warped needle samples per workgroup of warp_needle
constexpr int kWarpCombineThreads = 256;   // threads of the workgroup that turns one hit's partials into its record
constexpr int kWarpMaxRates = 2 * AM_WARP_MAX_STEPS + 1;
constexpr size_t kWarpRoundBytes = (size_t)64 << 20;   // a round of hits: its partial records, and its warped needles, at most this much each (one hit at the least)
// One warped needle of a call: out[j], j < s_q, from needle[0, s) at the step inc (32.32 fixed point)
struct WarpJob {
    const float* needle;
    float* out;
    long long s, s_q;
    unsigned long long inc;
};
// The call's grid as the combine kernel reads it (a kernel argument)
struct WarpGrid {
    double centre_ppm, step_ppm;   // step_ppm = max_ppm / K (0 for K = 0)
    double d[kWarpMaxRates];       // d_q
    int k, r;
};
// table: h[phase][tap] (AM_WARP_PHASES x AM_WARP_TAPS f32)
hipError_t launch_warp_needles(hipStream_t st, const WarpJob* d_jobs, int n_jobs, long long max_len, const float* table);
// tab: 2 k + 1 entries per hit (hit i, rate q at i * (2 k + 1) + q, filled as for launch_seg_slices with m = 1); parts /
// pflags as launch_seg_slices wrote them; d_out: n records (the `length` of an AM_HIT_NONFINITE record is left to the host,
// which knows the unwarped needle)
hipError_t launch_warp_combine(hipStream_t st, const SegDesc* tab, long long n, const WarpGrid& grid, const double* parts,
                               const unsigned* pflags, am_warp_hit* d_out);

// ---- am_channel.hip: per-hit channel estimation (am_hit_channel*) ----
constexpr int kLagTile = 32;                           // lags per workgroup of the slice kernel
constexpr size_t kChanRoundBytes = (size_t)64 << 20;   // a round of items: its partial records at most this much (one item at the least)
constexpr int lag_tiles(int nlag) { return (nlag + kLagTile - 1) / kLagTile; }
constexpr int lag_record_len(int nt) { return nt * kLagTile + 2; }   // doubles per partial record: the tiles' sums, E_w, E_x
constexpr int lag_sums_len(int nlag) { return nlag + 3; }            // doubles per item's sums record: the lags' sums, E_w, E_x, the flag (0 or 1)
// One item of a call, as the kernels read it: a signal x around t against a needle, the lags lag0 .. lag0 + nlag - 1
struct LagDesc {
    const void* win;      // device: sample t of x (f32 mono, or an i16 stereo frame for kind 1)
    const float* needle;  // device: the whole needle
    long long s;          // needle length
    long long ulo, uhi;   // x[t + u] exists (and is read) for ulo <= u < uhi only
    long long part0;      // first partial record of the item: slice k at part0 + k
    int lag0, nlag;       // lag0 <= 0
    int head;             // P: E_x adds x[t - P, t) and x[t + S, t + S + P) to E_w
    int pad;
};
// items [first, first + n) of the table, all of one kind and with nt = lag_tiles(nlag) tiles; parts: lag_record_len(nt)
// doubles per slice, pflags: nt words per slice
hipError_t launch_lag_slices(hipStream_t st, const LagDesc* tab, long long first, long long n, int nt, int max_nsl, int kind, double* parts,
                             unsigned* pflags);
// one wave per item of [0, n): sums: lag_sums_len(nlag_max) doubles per item
hipError_t launch_lag_combine(hipStream_t st, const LagDesc* tab, long long n, int nt, int nlag_max, const double* parts,
                              const unsigned* pflags, double* sums);

// ---- am_stereo.hip: per-hit stereo image (am_hit_stereo*) and the stereo mix (am_pcm_s16_stereo_mix*) ----
// The slice kernel exists for the radii of kSegRadii, as seg_slices does.  A partial record: C_L(-RT .. RT), C_R(-RT .. RT)
// as doubles, then S_LL, S_RR, S_LR as 64-bit integers in the same 8-byte slots.
constexpr int stereo_record_len(int rt) { return 2 * (2 * rt + 1) + 3; }
// One hit of a call, as the kernels read it (the call's table, uploaded once); R is the call's
struct StereoDesc {
    const void* win;      // device: frame t of the haystack (i16 stereo)
    const float* needle;  // device: the whole needle
    long long s;          // needle length
    long long ulo, uhi;   // frame t + u exists (and is read) for ulo <= u < uhi only: [-R, s + R) clipped to the haystack
    long long part0;      // first partial record of the hit: slice k at part0 + k
    double en;            // sum(needle^2)
    double floor_ratio;   // 10^(-score_norm_floor_db / 10)
};
// parts: stereo_record_len(seg_kernel_radius(r)) doubles per slice, pflags: one word per slice; d_out: n records
hipError_t launch_hit_stereo(hipStream_t st, const StereoDesc* d_hits, long long n, int r, long long max_slices, double* parts,
                             unsigned* pflags, am_stereo_hit* d_out);
// out[i] = f32((f64(a) L[i] + f64(b) R[i]) k), k = (double)(1.0f / 65535.0f)
hipError_t launch_pcm_mix(hipStream_t st, const int16_t* in, long long frames, float a, float b, float* out);

// ---- am_bands.hip: per-band hit scoring (am_hit_bands*) ----
constexpr int kBandGroup = 8;   // consecutive frames per workgroup of the frame kernel, counted from the hit's first frame
inline int band_record_len(int n_bands) { return 4 * n_bands + 1; }   // doubles per partial record: (Re C, Im C, E_x, E_n) per band, E_n over every bin
// One hit of a call, as the kernels read it (the call's table, uploaded once); F and the bands are the call's
struct BandDesc {
    const void* win;      // device: sample t of the haystack (f32 mono, or an i16 stereo frame for kind 1)
    const float* needle;  // device: the whole needle
    long long nframes;    // J: frame j reads samples [j F / 2, j F / 2 + F) of both
    long long part0;      // first partial record of the hit: group g at part0 + g
    double floor_ratio;   // 10^(-score_norm_floor_db / 10)
    int kind;             // 0 = f32 mono, 1 = i16 stereo
    int ngroups;          // ceil(J / kBandGroup)
};
// tab: the table of F (window, twiddles); parts: band_record_len(B) doubles per group, pflags: one word per group; d_out: n * B records
hipError_t launch_hit_bands(hipStream_t st, const BandDesc* d_hits, long long n, const am_band_params& bp, int max_groups,
                            double empty_ratio, const double* tab, double* parts, unsigned* pflags, am_hit_band* d_out);

// ---- am_significance.hip: per-hit significance (am_hit_significance*) ----
constexpr int kSigSlice = 4096;   // scores of a hit's zone per workgroup of the slice kernels, counted from the zone's start
// One hit of a launch sequence, as the kernels read it.  The zone's scores r(lo .. hi) lie at scores[z0 .. z0 + nz).
struct SigDesc {
    long long z0;      // first score of the zone in the score buffer
    long long nz;      // hi - lo + 1
    long long c;       // t - lo: the hit's own score
    long long g;       // guard: zone index k is background when |k - c| > g
    long long part0;   // first partial record of the hit
    unsigned flags;    // AM_HIT_CLIPPED, AM_HIT_NONFINITE as the host found them
    unsigned pad;
};
// psum: one double per slice (pass 1: the sum, pass 2: the sum of squared deviations), pmax: three words per slice
// (count, largest background score, its lag), mean / hmax: the same per hit; d_out: n records
hipError_t launch_hit_significance(hipStream_t st, const SigDesc* d_hits, long long n, long long max_slices, const float* scores,
                                   double* psum, unsigned* pmax, double* mean, unsigned* hmax, am_significance* d_out);

// ---- am_resample.hip: sample-rate conversion (am_resample*) ----
constexpr int kRsThreads = 256;
constexpr int kRsJ = 8;          // outputs per work item: k, k + W, ..., k + 7 W (one phase, its taps read once)
constexpr int kRsTc = 8;         // taps per register chunk; the table's rows are padded to a multiple of it
// One launch: outputs [0, n_out) of x = src (f32 mono, or the down-mix of i16 stereo frames for kind 1).  Workgroup b
// produces the W * kRsJ outputs from k0 = b * W * kRsJ on; work item w < W (a multiple of L) the outputs k0 + w + jj W.
struct ResampleJob {
    const void* src;
    long long n_in;
    float* dst;
    long long n_out;
    const float* taps;   // device, [L][ts]: taps[p][t] = h[p + t L - H] while p + t L <= 2H, else 0
    int L, M, H, ts;
    int W;
    int xs_cap;          // floats of input staged in LDS per workgroup (0: every sample read through the cache)
    int tab_lds;         // 1: the table is staged in LDS (rows padded to ts + 1 floats)
    int vec;             // 1: src is 16-byte aligned (the staging loads read 4 samples / frames at a time)
};
hipError_t launch_resample(hipStream_t st, const ResampleJob& j, int kind);

// ---- am_whiten.hip: spectral whitening (am_lag_products*, am_fir*) ----
constexpr int kLagBlock = 8192;     // samples per block of the lag products: one f64 partial per (lag, block)
constexpr int kLagThreads = 256;
constexpr int kLagChunk = 8;        // lags accumulated at a time (8 f64 accumulators per work item)
constexpr int kLagHist = AM_WHITEN_MAX_ORDER + kLagChunk;   // samples staged in front of a block / a tile: what the aligned
                                                            // register windows of the last chunk reach back to
inline long long lag_blocks(long long n) { return (n + kLagBlock - 1) / kLagBlock; }
// parts[k * nblk + b] = sum over the samples i of block b of x~[i] x~[i - k], k <= order (x~: 0 before sample 0 and for a
// non-finite sample); r[k] = the partials of lag k added in block order.  vec: src is 16-byte aligned.
hipError_t launch_lag_products(hipStream_t st, const void* src, long long n, int kind, int vec, int order, double* parts, double* r);
constexpr int kFirThreads = 256;
constexpr int kFirPer = 4;          // consecutive outputs per work item and pass
constexpr int kFirPasses = 2;
constexpr int kFirTile = kFirThreads * kFirPer * kFirPasses;   // outputs per workgroup
constexpr int kFirChunk = 8;        // taps per register window
constexpr int kFirHist = AM_FIR_MAX_TAPS - 1 + kFirChunk;   // samples staged in front of a tile (the last window's reach)
// One launch: y[k] = sum_{j < n_taps} taps[j] x[lead + k - j], k < n_out = n_in - lead; x = src (f32 mono, or the down-mix
// of i16 stereo frames for kind 1), 0 before src[0].  The taps travel in the kernel argument.
struct FirJob {
    const void* src;
    long long n_in, lead;
    float* dst;
    long long n_out;
    int n_taps;
    int vec;             // 1: src + lead is 16-byte aligned (the staging loads read 4 samples / frames at a time)
    int vec_out;         // 1: dst is 16-byte aligned (four samples per store)
    float taps[AM_FIR_MAX_TAPS + kFirChunk - 1];   // taps[j >= n_taps] = 0, never multiplied
};
hipError_t launch_fir(hipStream_t st, const FirJob& j, int kind);

// ---- am_estimate.hip: needle estimation (am_needle_estimate_*) ----
// One row of the gather form, as the kernel reads it (the call's table, uploaded once): element n of the row is
// fl32(x[off + n] * scale), absent where off + n lies outside [0, len)
struct EstHit {
    const void* src;      // device: element 0 of the hit's haystack (f32 mono, or i16 stereo frames); readable even where len = 0
    long long len;        // its length in samples / frames
    long long off;        // start - lead (may be negative)
    float scale;
    int pad;
};
// One launch: output sample n < length from rows 0 .. n - 1, in this order
struct EstJob {
    const void* src;      // device: n x length f32, row-major (source 0), or the table of n EstHit (sources 1, 2)
    long long length;
    int n;
    int method;           // AM_EST_*
    unsigned trim_permille;
    float* est;           // device, length entries each; dev and count may be null
    float* dev;
    unsigned* count;
};
// src: 0 = rows, 1 = hit table over f32 mono haystacks, 2 = over i16 stereo haystacks.  Runs the mean kernel, or the
// smallest sorting network (8, 16, 32, 64 slots) that holds j.n rows; hipErrorInvalidValue where there is none
hipError_t launch_estimate(hipStream_t st, const EstJob& j, int src);

}  // namespace am
