/*
 * audiomatch.h -- C ABI of libaudiomatch_amd.so, the MI355X (gfx950) native
 * implementation of NilsJochem/audio-matcher's src/matcher hot path:
 * sliding-window FFT cross-correlation + prominence peak pick.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, never
 * throws or aborts across the boundary, and returns an int status
 * (AM_OK == 0).  am_last_error_string() gives a thread-local description of
 * the last failure on the calling thread.
 *
 * Each declaration cites the reference interface it replaces
 * (paths relative to the reference crate root).
 *
 * There is NO CPU fallback: with no usable HIP device every compute entry
 * point returns AM_ERR_NO_DEVICE / AM_ERR_HIP.
 */
#ifndef AUDIOMATCH_H
#define AUDIOMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AM_ABI_VERSION 3

/* status codes */
enum {
    AM_OK = 0,
    AM_ERR_INVALID_ARG = 1,   /* null pointer, zero length, unsupported size ... */
    AM_ERR_CAPACITY = 2,      /* caller buffer too small; required length was written */
    AM_ERR_HIP = 3,           /* a HIP runtime call or kernel launch failed */
    AM_ERR_NO_DEVICE = 4,     /* no gfx950-capable device / bad ordinal */
    AM_ERR_PEAK_OVERFLOW = 5, /* a chunk of 2^32 scores or more with more than AM_MAX_PEAKS_PER_CHUNK peaks */
    AM_ERR_OOM = 6            /* host or device allocation failed */
};

/* audio_matcher.rs:55-59  enum Mode { Full, Same, Valid } */
enum { AM_MODE_FULL = 0, AM_MODE_SAME = 1, AM_MODE_VALID = 2 };

/* `scale: bool` of CorrelateAlgo::correlate_with_sample (audio_matcher.rs:67-72),
 * split by implementation because the two reference algos disagree
 * (SURVEY.md F4):
 *   AM_SCALE_LIB = LibConvolve, the production algo (matcher/mod.rs:34):
 *                  corr / sum(needle^2)            audio_matcher.rs:306-308
 *   AM_SCALE_MY  = MyConvolve: corr / sum(needle^2) / within.len()
 *                                                  audio_matcher.rs:442-448 */
enum { AM_SCALE_NONE = 0, AM_SCALE_LIB = 1, AM_SCALE_MY = 2 };

/* Sample format of a haystack buffer.  The reference decodes every file to interleaved 16-bit
 * stereo (mp3_reader.rs:26 asserts two channels) and hands calc_chunks the down-mixed f32 mono
 * stream (mp3_reader.rs:28-37); both ends of that step are accepted.  One element (an f32 sample,
 * or one stereo frame of two i16) is 4 bytes in either format. */
enum { AM_FMT_F32_MONO = 0, AM_FMT_S16_STEREO = 1 };

/* Not a limit on results: any number of peaks may pass the prominence filter in a chunk and, as
 * find_peaks does, the library returns every one the distance filter keeps (the caller's `cap`
 * is the only bound).  Up to this many per chunk are ordered and filtered on chip; a chunk with
 * more (a min_distance shorter than the chunk and a tiny prominence bound) takes a slower path
 * through a list in device memory. */
#define AM_MAX_PEAKS_PER_CHUNK 1024

/* Opaque handle = the reference's `LibConvolve { sample_data, .. }` /
 * `MyConvolve` object (audio_matcher.rs:282-295, 379-403): owns a device copy
 * of the needle, its cached 1/sum(needle^2) and its cached spectra. */
typedef struct am_needle am_needle;

/* find_peaks::Peak<f32> as consumed downstream (only position and prominence
 * are read: matcher/mod.rs:110-129, archive/data.rs:87-107). */
typedef struct am_peak {
    uint64_t start;    /* position.start, absolute sample offset in the haystack */
    uint64_t end;      /* position.end (exclusive) */
    float height;      /* score at the peak */
    float prominence;  /* Option<f32>, always Some on this path */
} am_peak;

/* Parameters of calc_chunks (audio_matcher.rs:88-97) after Config::from_args
 * (audio_matcher.rs:38-52) and the duration->sample rounding of :99-100. */
typedef struct am_match_params {
    uint32_t sr;                  /* sample rate (u16 in the reference) */
    uint64_t chunk;               /* chunk_size in samples   (:100) */
    uint64_t overlap;             /* overlap_length in samples (:99) */
    float min_prominence;         /* PeakConfig.prominence = args.prominence/100 (:44) */
    uint64_t min_distance;        /* distance.as_secs() * sr, samples (:228) */
    double overshadow_distance_s; /* PeakConfig.distance in seconds (:137-138) */
    int scale;                    /* AM_SCALE_*; production passes true -> AM_SCALE_LIB (mod.rs:85) */
} am_match_params;

/* ---- library / device ------------------------------------------------- */
int am_abi_version(void);
const char* am_last_error_string(void);
int am_device_count(int* n);
/* Releases every scratch buffer, transform plan and timing event the library
 * holds on every device (needle handles stay valid and rebuild what they need
 * on their next use).  Optional: everything is also released at process exit. */
int am_shutdown(void);

/* Device pointers (every `d_` argument, and everything the `_device` entry
 * points take): the library works on a stream of its own, which is NOT ordered
 * with the caller's streams or with the null stream.  Data behind a device
 * pointer must be complete before the call (synchronise whatever produced it;
 * note that a device-to-device hipMemcpy returns before the copy has run), and
 * results written to a device pointer are complete when the call returns. */

/* ---- needle handle ----------------------------------------------------- */
/* LibConvolve::new(sample_data) audio_matcher.rs:289 / MyConvolve::new :396.
 * `needle` is host memory, copied; the handle lives on `device`. */
int am_needle_create(int device, const float* needle, size_t n, am_needle** out);
/* same, needle already resident on `device` */
int am_needle_create_device(int device, const float* d_needle, size_t n, am_needle** out);
void am_needle_destroy(am_needle* h);
int am_needle_len(const am_needle* h, size_t* n);
/* CorrelateAlgo::inverse_sample_auto_correlation (audio_matcher.rs:66, 321-329) */
int am_needle_inv_autocorr(const am_needle* h, float* out);

/* ---- masked needles: spans to ignore, NCC over the rest -------------------------------------------------------------
 * A jingle whose middle changes from one occurrence to the next (a spoken title over the theme, "the news at NINE", a
 * sponsor line): the needle carries a mask, `gaps`, the spans [begin, end) of its samples to ignore.  The kept spans are
 * what lies between them, [a_j, b_j), at most AM_MASK_MAX_GAPS + 1 of them.
 *   gaps ascend; each has begin < end <= n; gaps[i].end < gaps[i+1].begin (touching gaps are the caller's to merge, so
 *   every kept span is non-empty); the first may begin at 0, the last may end at n; at least one sample is kept;
 *   n_gaps <= AM_MASK_MAX_GAPS.  A violation is AM_ERR_INVALID_ARG, the message names the gap and the rule.  n_gaps = 0
 *   gives am_needle_create's handle in every respect.  A needle long enough to be partitioned (more than 2^22 samples)
 *   is refused: masked partitioned needles are not supported.
 * The handle's needle is the needle with its gap samples set to +0: every correlation value of every entry point is the
 * masked numerator, and am_needle_inv_autocorr is 1 / E_n^M, E_n^M = the energy of the kept samples.  With "score_norm"
 * = 0 a masked handle behaves as that zero-filled needle.  With "score_norm" = 1 every entry point that supports the
 * option returns masked NCC,
 *     mncc(t) = corr(t) / sqrt(E_n^M E_x^M(t)),   E_x^M(t) = sum_j sum_{i in [a_j, b_j)} x[t - lead + i]^2,
 * x = 0 outside the signal: what lies under the gaps, however loud, enters neither the numerator nor the denominator.
 * The score rule is that of "score_norm" with E_x^M in the window energy's place: 0 when E_x^M(t) = 0 or E_x^M(t) <
 * E_n^M 10^(-score_norm_floor_db / 10), the quotient in f64 and rounded once, a non-finite raw score left as it is.
 * E_x^M is added up span by span in ascending order, each span's energy from non-negative pieces only (never "whole
 * window minus gaps"): kept spans in digital silence score exactly 0.  A haystack's bits are the same alone and in any
 * batch.  Non-finite haystack samples cost the whole windows that hold them, gaps included (the numerator comes from a
 * transform of all samples).  Entry points that refuse "score_norm" refuse it for a masked handle too.
 * The per-hit families (am_hit_scores* and the others below) read the handle's needle and the whole window: on a
 * masked handle they score the zero-filled needle against everything under it, gaps included.  am_hit_mask* below is
 * the per-hit record of a masked handle. */
#define AM_MASK_MAX_GAPS 15
typedef struct am_span {
    uint64_t begin, end;   /* samples of the needle, [begin, end) */
} am_span;
/* `needle` is host memory, copied (gap samples may hold anything, non-finite values included) */
int am_needle_create_masked(int device, const float* needle, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out);
/* same, needle already resident on `device` (gaps is host memory) */
int am_needle_create_masked_device(int device, const float* d_needle, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out);
/* The handle's gaps: *n_gaps = their number (0 for an ordinary handle), the first min(*n_gaps, cap) in gaps (which may
 * be NULL when cap = 0); AM_ERR_CAPACITY when there are more than cap. */
int am_needle_mask(const am_needle* h, am_span* gaps, size_t cap, size_t* n_gaps);

/* The per-hit record of a masked handle: does an occurrence hold the original in its gaps, or something else, and how
 * loud is that?  For a hit at t = peak.start, the zero-filled needle n, the ORIGINAL needle samples o under the gaps and
 * the haystack's samples x (the down-mix for AM_FMT_S16_STEREO, as for am_hit_scores), in f64 by direct sums:
 *     kept samples i:  c_k = sum x[t + i] n[i],  E_x^M = sum x[t + i]^2,  E_n^M = the handle's energy
 *     gap samples i:   c_g = sum x[t + i] o[i],  E_x,gaps = sum x[t + i]^2,  E_n,gaps = sum o[i]^2
 *   ncc       c_k / sqrt(E_n^M E_x^M); 0 with AM_MASK_BELOW_FLOOR when E_x^M = 0 or E_x^M < E_n^M 10^(-score_norm_floor_db / 10)
 *             (the process option at call time, as am_hit_scores)
 *   gain      c_k / E_n^M
 *   kept_db   10 log10(E_x^M / E_n^M), -inf for E_x^M = 0
 *   ncc_gaps  c_g / sqrt(E_n,gaps E_x,gaps); 0 when either energy is 0
 *   gaps_db   10 log10(E_x,gaps / (gain^2 E_n,gaps)): what lies in the gaps against what the needle would put there at the
 *             hit's gain; -inf for E_x,gaps = 0 (flag AM_MASK_GAPS_SILENT), +inf for gain^2 E_n,gaps = 0 < E_x,gaps
 * AM_MASK_NONFINITE: a non-finite sample of the needle or the haystack under a kept span; every field is NaN.
 * AM_MASK_GAPS_NONFINITE: a non-finite sample of the original needle or the haystack under a gap; ncc_gaps and gaps_db
 * are NaN, the other fields are not affected.  AM_MASK_NO_GAPS: the handle has no mask; ncc_gaps and gaps_db are NaN.
 * The sums run over slices of the needle in a fixed order: the three forms agree bit for bit and a hit's record does not
 * depend on the other hits of the call.  The forms, their arguments and their refusals are am_hit_scores*'s (the host
 * form copies only the hits' spans; the batch form takes the pair layout of am_match_multi_batch_device). */
enum { AM_MASK_BELOW_FLOOR = 1, AM_MASK_NONFINITE = 2, AM_MASK_GAPS_SILENT = 4, AM_MASK_GAPS_NONFINITE = 8, AM_MASK_NO_GAPS = 16 };
typedef struct am_mask_hit {
    float ncc;        /* c_k / sqrt(E_n^M E_x^M(t)), exact: direct f64 sums over the kept samples */
    float gain;       /* c_k / E_n^M */
    float kept_db;    /* 10 log10(E_x^M / E_n^M) */
    float ncc_gaps;   /* the same NCC over the gap samples, against the ORIGINAL needle samples there */
    float gaps_db;    /* 10 log10(E_x,gaps / (gain^2 E_n,gaps)) */
    uint32_t flags;   /* AM_MASK_* */
} am_mask_hit;       /* 24 bytes */
int am_hit_mask_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                       const am_peak* peaks, size_t n, am_mask_hit* out);
int am_hit_mask(const am_needle* h, const void* haystack, size_t len, int sample_format,
                const am_peak* peaks, size_t n, am_mask_hit* out);
int am_hit_mask_batch_device(const am_needle* const* needles, size_t n_needles,
                             const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                             const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks, am_mask_hit* out);

/* ---- level 1: one correlation (the trait method) ------------------------ */
/* output length of a mode: audio_matcher.rs:450-456 */
int am_correlate_len(size_t w, size_t s, int mode, size_t* out_len);
/* CorrelateAlgo::correlate_with_sample(&self, within, mode, scale)
 * (audio_matcher.rs:67-72, 331-343, 471-478).  Host buffers in and out.
 * On AM_ERR_CAPACITY *out_len holds the required length. */
int am_correlate(const am_needle* h, const float* within, size_t w, int mode, int scale,
                 float* out, size_t cap, size_t* out_len);
/* same with device-resident input and output */
int am_correlate_device(const am_needle* h, const float* d_within, size_t w, int mode, int scale,
                        float* d_out, size_t cap, size_t* out_len);

/* ---- level 2: the chunked matcher --------------------------------------- */
/* calc_chunks(sr, m_samples, &algo, scale, config) (audio_matcher.rs:88-141):
 * windowing, per-chunk Valid correlation, per-chunk find_peaks
 * (:221-230), offset restore (:126), sort by start (:135) and the overshadow
 * filter (:136-139, 143-160).  Returns peaks sorted by start.
 * p->scale takes any AM_SCALE_* value, as the reference's generic calc_chunks takes any
 * CorrelateAlgo: with AM_SCALE_MY every window is scaled by its own
 * 1 / (sum(needle^2) * within.len()) (audio_matcher.rs:442-448).
 * On AM_ERR_CAPACITY *n_out holds the number of peaks found. */
int am_match(const am_needle* h, const float* haystack, size_t len,
             const am_match_params* p, am_peak* out, size_t cap, size_t* n_out);
/* haystack already resident in HBM */
int am_match_device(const am_needle* h, const float* d_haystack, size_t len,
                    const am_match_params* p, am_peak* out, size_t cap, size_t* n_out);
/* The per-file loop of matcher::run (matcher/mod.rs:42-87) over resident
 * haystacks: out holds cap_per_hay slots per haystack, n_out[k] the count
 * for haystack k (if n_out[k] > cap_per_hay the call returns AM_ERR_CAPACITY
 * after filling what fits). */
int am_match_batch_device(const am_needle* h, const float* const* d_haystacks, const size_t* lens,
                          size_t n_hay, const am_match_params* p,
                          am_peak* out, size_t cap_per_hay, size_t* n_out);

/* Several needles (equal length, same device) against one resident haystack
 * (BASELINE config 4): the haystack's forward column pass is computed once and
 * its forward row transforms once per group of needles (option "needle_group");
 * out holds cap_per_needle slots per needle, n_out[k] the count for needle k.
 * The reference has no such entry point (one snippet per run,
 * matcher/mod.rs:29-34); offsets equal those of n_needles separate
 * am_match_device calls, heights and prominences agree to f32 rounding. */
int am_match_multi_device(const am_needle* const* needles, size_t n_needles, const float* d_haystack, size_t len,
                          const am_match_params* p, am_peak* out, size_t cap_per_needle, size_t* n_out);

/* The per-file loop of matcher::run (matcher/mod.rs:42-87) around SEVERAL snippets (BASELINE
 * config 4: "32 needles vs 1000 x 1 h haystacks, haystack FFT reused"): n_needles equal-length
 * needles on one device against n_hay resident haystacks of `sample_format` (AM_FMT_*; lens in
 * samples / frames).  Per haystack the forward column pass runs once and the forward row
 * transforms once per group of needles; the peak pick of one (haystack, needle) pair runs beside the
 * transforms of the next.  out holds cap_per_pair slots per pair, pair (haystack k, needle j) at
 * index k * n_needles + j; n_out likewise.  Results equal n_hay * n_needles separate am_match_device /
 * am_match_pcm16_device calls (offsets identical, heights and prominences to f32 rounding); a
 * haystack with non-finite samples loses exactly the windows that hold them, as there. */
int am_match_multi_batch_device(const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks,
                                const size_t* lens, size_t n_hay, int sample_format, const am_match_params* p,
                                am_peak* out, size_t cap_per_pair, size_t* n_out);

/* Several needles of ANY lengths (same device) against a batch of resident haystacks: a radio archive's intro, outro,
 * stingers and station IDs in one call.  overlaps[j] is the overlap (in samples) of needle j's windows,
 * chunk + overlaps[j]; overlaps == NULL means p->overlap for every needle.  Pair (haystack k, needle j) returns what
 * am_match_device(needles[j], haystack k, p') (am_match_pcm16_device for AM_FMT_S16_STEREO) returns, p' = p with
 * overlap = overlaps[j]: offsets identical, heights and prominences to f32 rounding; non-finite samples cost exactly
 * the windows of that needle that hold them; a haystack shorter than needle j gives that pair 0 hits.  Layout of out
 * and n_out, tail_window, the peak rules, scaling (AM_SCALE_NONE / AM_SCALE_LIB) and half_pipeline as in
 * am_match_multi_batch_device; options come from needles[0].  Every haystack has one block layout, that of the
 * longest needle: its forward column pass runs once, its forward row transforms once per group of needles (grouped
 * longest first), each needle's scores end at its own last offset.  Needles of one length with every overlap equal
 * to p->overlap: am_match_multi_batch_device's results bit for bit. */
int am_match_multi_varlen_batch_device(const am_needle* const* needles, size_t n_needles, const uint64_t* overlaps,
                                       const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                                       int sample_format, const am_match_params* p,
                                       am_peak* out, size_t cap_per_pair, size_t* n_out);
/* the same for ONE haystack in host memory (AM_FMT_F32_MONO or AM_FMT_S16_STEREO; len in samples / frames):
 * out holds cap_per_needle slots per needle, n_out[j] the count for needle j */
int am_match_multi_varlen(const am_needle* const* needles, size_t n_needles, const uint64_t* overlaps,
                          const void* haystack, size_t len, int sample_format, const am_match_params* p,
                          am_peak* out, size_t cap_per_needle, size_t* n_out);

/* The same matcher on interleaved 16-bit stereo PCM, the sample format the
 * reference decodes to (mp3_reader.rs:26 asserts two channels): the down-mix
 * mono = (l as f32 + r as f32) * 0.5 * (1/65535) (mp3_reader.rs:12, 28-37) is
 * fused into the first kernel's loads, bit-exact, so PCM is read once. */
int am_needle_create_pcm16(int device, const int16_t* interleaved, size_t frames, am_needle** out);
int am_match_pcm16(const am_needle* h, const int16_t* interleaved, size_t frames,
                   const am_match_params* p, am_peak* out, size_t cap, size_t* n_out);
int am_match_pcm16_device(const am_needle* h, const int16_t* d_interleaved, size_t frames,
                          const am_match_params* p, am_peak* out, size_t cap, size_t* n_out);
int am_match_pcm16_batch_device(const am_needle* h, const int16_t* const* d_interleaved, const size_t* frames,
                                size_t n_hay, const am_match_params* p,
                                am_peak* out, size_t cap_per_hay, size_t* n_out);

/* ---- per-hit scoring ----------------------------------------------------------- */
/* A level-independent confidence and a sub-sample position for the few hits a match returned, from ANY entry point
 * (the reference reports integer offsets and the LibConvolve height only, matcher/mod.rs:110-125).  For a hit with
 * t = peak.start, needle n[0 .. S) (the handle's whole needle, partitioned handles included) and the haystack's samples
 * x (f32 mono, or for AM_FMT_S16_STEREO the down-mix (l + r) * 0.5 * (1/65535) bit for bit as above), in f64:
 *     corr(u) = sum_{i<S} x[u + i] n[i],   E_n = sum n^2 (the needle's energy),   E_w = sum_{i<S} x[t + i]^2
 *   position   t + d,  d = 0.5 (a - c) / (a - 2b + c) clamped to [-0.5, 0.5], a, b, c = corr(t - 1), corr(t), corr(t + 1)
 *              (the vertex of the parabola through the three scores).  d = 0 and flag AM_HIT_UNREFINED when t = 0,
 *              when t + S = len, when a - 2b + c >= 0 (no maximum), or when x[t - 1] or x[t + S] is not finite.
 *   ncc        corr(t) / sqrt(E_n E_w) in [-1, 1]; 0 with flag AM_HIT_BELOW_FLOOR when E_w = 0 or
 *              E_w < E_n 10^(-score_norm_floor_db / 10) -- the floor of the NCC scores, the process option at call time.
 *   gain       corr(t) / E_n: the least-squares factor of the needle in the window (0 if E_n = 0); the default
 *              (AM_SCALE_LIB) height of the hit.
 *   window_db  10 log10(E_w / E_n); -inf for a silent window.
 *   flags      AM_HIT_*.  AM_HIT_NONFINITE: a sample of x[t .. t + S) or of the needle is not finite; ncc, gain and
 *              window_db are then NaN, position = t and no other flag is set.
 * A hit's result depends on the needle, the samples it reads and the floor only -- not on the other hits of the call,
 * the batch or the entry point: the three forms below agree bit for bit.  The cost is proportional to the number of
 * hits times S (about 4 (S + 2) bytes of haystack per hit), not to the haystack's length.
 * peaks and out are host memory, out[i] scores peaks[i]; len counts samples (frames for AM_FMT_S16_STEREO).
 * AM_ERR_INVALID_ARG, naming the hit (and pair): a null pointer with n > 0, an unknown sample format,
 * peak.start + S > len, a haystack on another device than the needle.  n = 0: AM_OK, nothing launched. */
enum { AM_HIT_UNREFINED = 1, AM_HIT_BELOW_FLOOR = 2, AM_HIT_NONFINITE = 4 };
typedef struct am_hit_score {
    double position;   /* t + d, sub-sample start of the hit */
    float ncc;         /* exact normalised correlation */
    float gain;        /* least-squares gain of the needle in the window */
    float window_db;   /* window energy over needle energy, dB */
    uint32_t flags;    /* AM_HIT_* */
} am_hit_score;        /* 24 bytes, no padding */
/* the haystack resident on the needle's device */
int am_hit_scores_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_peak* peaks, size_t n, am_hit_score* out);
/* the haystack in host memory: only the spans [t - 1, t + S + 1) of the hits are copied (merged where they overlap) */
int am_hit_scores(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_peak* peaks, size_t n, am_hit_score* out);
/* The result layout of am_match_multi_batch_device (n_needles = 1: of am_match_batch_device and
 * am_match_pcm16_batch_device, unchanged): pair (haystack k, needle j) at k * n_needles + j, cap_per_pair slots per
 * pair, min(n_peaks[pair], cap_per_pair) hits scored per pair, out laid out like peaks (other slots untouched).
 * Needles may differ in length; needles and haystacks on one device.  Every hit of the call in one launch sequence.
 * Pool results: score each slot's hits with that slot's needle (am_pool_slot). */
int am_hit_scores_batch_device(const am_needle* const* needles, size_t n_needles,
                               const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                               const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks, am_hit_score* out);

/* ---- per-segment hit scoring ----------------------------------------------------- */
/* Which part of the needle a hit holds, and how its position drifts along the needle: the pass of am_hit_scores
 * resolved along the needle (the reference reports one offset and one height per hit, matcher/mod.rs:110-125).  The
 * needle n[0 .. S) is cut into m segments, segment j = needle samples [a_j, a_{j+1}) with a_j = floor(j S / m) (lengths
 * differ by at most one).  With t = peak.start and x the haystack's samples (f32 mono, or the bit-exact down-mix for
 * AM_FMT_S16_STEREO as above), x COUNTING AS 0 OUTSIDE [0, len), for every lag l in [-R, R], in f64:
 *     c_j(l) = sum_{i in seg j} x[t + l + i] n[i],   E_w,j(l) = sum_{i in seg j} x[t + l + i]^2,   E_n,j = sum_{i in seg j} n[i]^2
 *   l*         the lag with the largest c_j(l); ties go to the smaller |l|, then to the negative lag.
 *   lag        l* + d,  d = 0.5 (a - c) / (a - 2b + c) clamped to [-0.5, 0.5], a, b, c = c_j(l* - 1), c_j(l*), c_j(l* + 1).
 *              d = 0 and flag AM_HIT_UNREFINED when R = 0, when |l*| = R or when a - 2b + c >= 0.
 *   ncc        c_j(l*) / sqrt(E_n,j E_w,j(l*)); 0 with flag AM_HIT_BELOW_FLOOR when E_w,j(l*) = 0 or
 *              E_w,j(l*) < E_n,j 10^(-score_norm_floor_db / 10) -- the process option am_hit_scores reads at call time,
 *              applied per segment.
 *   gain       c_j(l*) / E_n,j.
 *   level_db   10 log10(E_w,j(l*) / E_n,j); -inf for a silent window.
 *   flags      AM_HIT_*.  AM_HIT_EMPTY_SEGMENT: E_n,j = 0 (a silent stretch of the needle); lag = 0, ncc = gain = 0,
 *              level_db = +inf for E_w,j(0) > 0 and NaN for E_w,j(0) = 0, no other flag.  AM_HIT_NONFINITE: a sample of the
 *              needle's segment, or of x[t - R + a_j .. t + R + a_{j+1}) inside [0, len), is not finite; that segment only
 *              has lag = 0 and ncc, gain, level_db NaN, no other flag.
 * A segment's result depends on the needle, the samples it reads, m, R and the floor only: the three forms below agree
 * bit for bit, whatever else the call holds.  The cost is proportional to hits x S x (2R + 1), not to the haystack.
 * out holds m records per hit, hit i at out[i m .. (i + 1) m); in the batch form hit slot q of pair p is at
 * (p cap_per_pair + q) m -- the layout of am_hit_scores_batch_device times m; other slots stay untouched.
 * AM_ERR_INVALID_ARG, naming the hit (and pair): a null pointer with n > 0, sp == NULL, segments == 0, segments > S or
 * > AM_SEG_MAX_SEGMENTS, radius > AM_SEG_MAX_RADIUS, an unknown sample format, peak.start + S > len, a haystack on
 * another device than the needle.  n = 0: AM_OK, nothing launched. */
enum { AM_HIT_EMPTY_SEGMENT = 8 };
#define AM_SEG_MAX_SEGMENTS 1024
#define AM_SEG_MAX_RADIUS   16
typedef struct am_segment_params {
    uint32_t segments;   /* m, 1 .. min(S, AM_SEG_MAX_SEGMENTS) */
    uint32_t radius;     /* R, 0 .. AM_SEG_MAX_RADIUS: lags -R .. R are examined */
} am_segment_params;
typedef struct am_hit_segment {
    double lag;        /* l* + d: where this segment fits best, in samples relative to the hit's start */
    float ncc;         /* at l* */
    float gain;        /* at l* */
    float level_db;    /* 10 log10(E_w / E_n) of the segment at l*; -inf for silence */
    uint32_t flags;    /* AM_HIT_* */
} am_hit_segment;      /* 24 bytes, no padding */
/* the haystack resident on the needle's device */
int am_hit_segments_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                           const am_peak* peaks, size_t n, const am_segment_params* sp, am_hit_segment* out);
/* the haystack in host memory: only the spans [t - R, t + S + R) of the hits are copied (clipped, merged where they overlap) */
int am_hit_segments(const am_needle* h, const void* haystack, size_t len, int sample_format,
                    const am_peak* peaks, size_t n, const am_segment_params* sp, am_hit_segment* out);
/* the pair layout of am_hit_scores_batch_device; every hit of the call in one launch sequence, needles of any lengths */
int am_hit_segments_batch_device(const am_needle* const* needles, size_t n_needles,
                                 const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                 const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                 const am_segment_params* sp, am_hit_segment* out);
/* What callers want from one hit's m records (pure host code, no device): a segment is PRESENT when its flags hold none
 * of NONFINITE | BELOW_FLOOR | EMPTY_SEGMENT and ncc >= min_ncc, USABLE when present and not UNREFINED.  The line is the
 * ordinary least-squares fit of lag_j against the segment centre (a_j + a_{j+1}) / 2 over the usable segments (sums in
 * f64, in index order); with fewer than two usable segments drift_ppm, start_lag and residual_rms are NaN.
 * AM_ERR_INVALID_ARG: a null pointer, segments == 0 or > needle_len. */
typedef struct am_segment_summary {
    double coverage;       /* needle samples in present segments / S */
    double drift_ppm;      /* 1e6 * slope of lag over needle position; NaN with fewer than 2 usable segments */
    double start_lag;      /* the fitted line at needle position 0: refined start = peak.start + start_lag */
    double residual_rms;   /* rms of lag - line over the usable segments, samples */
    int32_t first_present, last_present;   /* segment indices, -1 when none */
    uint32_t n_present, n_usable;
} am_segment_summary;
int am_hit_segments_summary(const am_hit_segment* seg, uint32_t segments, size_t needle_len, float min_ncc,
                            am_segment_summary* out);

/* ---- per-band hit scoring --------------------------------------------------------- */
/* Which frequencies of the needle a hit holds: the pass of am_hit_scores resolved along frequency (the reference reports
 * one offset and one height per hit, matcher/mod.rs:110-125).  A copy from a low-rate MP3, a telephone insert or a
 * transfer with a tilted EQ matches in some bands and not in others; one broadband NCC mixes that into one number.
 * With t = peak.start, the needle n[0 .. S) (the handle's whole needle, partitioned handles included) and x the
 * haystack's samples (f32 mono, or the bit-exact down-mix for AM_FMT_S16_STEREO as above), everything in f64:
 *   frames     F = 2^frame_log2 samples at hop H = F / 2, J = floor((S - F) / H) + 1 of them; frame j reads
 *              x[t + jH .. t + jH + F) and n[jH .. jH + F).  The fewer than H needle samples behind the last frame are
 *              not read, nor the haystack samples under them.  Window w[i] = 0.5 - 0.5 cos(2 pi i / F).
 *   spectra    X_j[k] = sum_i w[i] x[t + jH + i] e^(-2 pi i ik / F), N_j[k] likewise from the needle, k = 0 .. F / 2.
 *   sums       P_xn[k] = sum_j X_j[k] conj(N_j[k]),   P_xx[k] = sum_j |X_j[k]|^2,   P_nn[k] = sum_j |N_j[k]|^2
 *   bands      band b = the bins [edges[b], edges[b + 1]):  C_b = sum_k P_xn[k],  E_x,b = sum_k P_xx[k],
 *              E_n,b = sum_k P_nn[k];  E_n = sum_{k = 0 .. F/2} P_nn[k] over every bin, in a band or not.
 *   ncc          Re C_b / sqrt(E_x,b E_n,b): the band's NCC at lag 0, in [-1, 1].
 *   coherence    |C_b| / sqrt(E_x,b E_n,b) in [0, 1]: survives a misalignment of a few samples, where ncc falls.
 *   gain         Re C_b / E_n,b: the least-squares gain of the needle in this band (over the bands: the copy's EQ curve).
 *   level_db     10 log10(E_x,b / E_n,b); -inf for a silent band.
 *   needle_share E_n,b / E_n: how much of the needle lives in this band (0 for a needle of zeros).
 *   flags      AM_HIT_*.  AM_HIT_NONFINITE: a sample the hit reads, x[t .. t + (J - 1) H + F) or n[0 .. (J - 1) H + F), is
 *              not finite; every band of the hit then has the five floats NaN and no other flag.
 *              AM_HIT_EMPTY_BAND: needle_share < 10^(-AM_BAND_EMPTY_DB / 10) -- a computed spectrum is never exactly 0,
 *              hence a fixed relative bound; ncc = coherence = gain = 0, level_db = +inf for E_x,b > 0 and NaN
 *              otherwise, no other flag.
 *              AM_HIT_BELOW_FLOOR: E_x,b = 0 or E_x,b < E_n,b 10^(-score_norm_floor_db / 10) -- the process option
 *              am_hit_scores reads at call time, applied per band; ncc = coherence = 0, gain and level_db are given.
 * A hit's records depend on the needle, the samples it reads, the parameters and the floor only: the three forms below
 * agree bit for bit, whatever else the call holds.  The cost is proportional to hits x J transforms of F points, not to
 * the haystack: 15 us per hit for a 10 s needle at 44.1 kHz with F = 1024 and 16 bands, 14 us with F = 4096 (64 hits in one
 * call), beside 2.0 us for am_hit_segments with m = 8, R = 4 on the same hits (tools/hit_bands_bench.py, profiles/r14/).
 * out holds B = n_bands records per hit, hit i band b at out[i B + b]; in the batch form hit slot q of pair p is at
 * (p cap_per_pair + q) B -- the layout of am_hit_scores_batch_device times B; other slots stay untouched.
 * AM_ERR_INVALID_ARG, naming the hit (and pair): a null pointer with n > 0, bp == NULL, frame_log2 outside 8 .. 12,
 * n_bands == 0 or > AM_BAND_MAX_BANDS, edges not strictly ascending or edges[B] > F / 2 + 1, S < F, an unknown sample
 * format, peak.start + S > len, a haystack on another device than the needle.  n = 0: AM_OK, nothing launched. */
enum { AM_HIT_EMPTY_BAND = 128 };
#define AM_BAND_MAX_BANDS 32
#define AM_BAND_EMPTY_DB  90
typedef struct am_band_params {
    uint32_t frame_log2;                    /* 8 .. 12 */
    uint32_t n_bands;                       /* B, 1 .. AM_BAND_MAX_BANDS */
    uint32_t edges[AM_BAND_MAX_BANDS + 1];  /* B + 1 bin indices, strictly ascending, edges[B] <= F / 2 + 1 */
} am_band_params;
typedef struct am_hit_band {
    float ncc;          /* Re C_b / sqrt(E_x,b E_n,b): the band's NCC at lag 0, in [-1, 1] */
    float coherence;    /* |C_b| / sqrt(E_x,b E_n,b), in [0, 1]: survives a few samples of misalignment */
    float gain;         /* Re C_b / E_n,b: least-squares gain of the needle in this band (the copy's EQ curve) */
    float level_db;     /* 10 log10(E_x,b / E_n,b); -inf for a silent band */
    float needle_share; /* E_n,b / E_n: how much of the needle lives in this band */
    uint32_t flags;     /* AM_HIT_* */
} am_hit_band;          /* 24 bytes, no padding */
/* the haystack resident on the needle's device */
int am_hit_bands_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                        const am_peak* peaks, size_t n, const am_band_params* bp, am_hit_band* out);
/* the haystack in host memory: only the spans [t, t + (J - 1) H + F) of the hits are copied (merged where they overlap) */
int am_hit_bands(const am_needle* h, const void* haystack, size_t len, int sample_format,
                 const am_peak* peaks, size_t n, const am_band_params* bp, am_hit_band* out);
/* the pair layout of am_hit_scores_batch_device; every hit of the call in one launch sequence, needles of any lengths
 * (each at least F).  Pool results: score each slot's hits with that slot's needle (am_pool_slot). */
int am_hit_bands_batch_device(const am_needle* const* needles, size_t n_needles,
                              const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                              const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                              const am_band_params* bp, am_hit_band* out);
/* What callers want from one hit's B records (pure host code, no device): a band is COUNTABLE when its flags hold neither
 * NONFINITE nor EMPTY_BAND, PRESENT when countable, not BELOW_FLOOR and coherence >= min_coherence.  Sums run in f64, in
 * index order; coverage and weighted_coherence are NaN without a countable band.
 * AM_ERR_INVALID_ARG: a null pointer, n_bands == 0 or > AM_BAND_MAX_BANDS. */
typedef struct am_band_summary {
    double coverage;             /* sum of needle_share over present bands / sum over countable bands */
    double weighted_coherence;   /* sum of needle_share * coherence / sum of needle_share, over countable bands */
    double gain_db_spread;       /* max - min of 20 log10(gain) over present bands with gain > 0; NaN with fewer than 2 */
    int32_t first_present, last_present;   /* band indices, -1 when none */
    uint32_t n_present, n_countable;
} am_band_summary;
int am_hit_bands_summary(const am_hit_band* rec, uint32_t n_bands, float min_coherence, am_band_summary* out);
/* B log-spaced bands from lo_hz to hi_hz at sample rate sr (pure host code): edges[b] = llround(lo (hi / lo)^(b / B) F / sr),
 * b = 0 .. B, each then raised to at least its predecessor + 1; the rest of *out is zeroed.
 * AM_ERR_INVALID_ARG: out == NULL, sr == 0, frame_log2 outside 8 .. 12, n_bands == 0 or > AM_BAND_MAX_BANDS, lo_hz <= 0,
 * hi_hz <= lo_hz, hi_hz > sr / 2, or edges that do not fit below F / 2 + 1. */
int am_band_edges_log(uint32_t sr, uint32_t frame_log2, double lo_hz, double hi_hz, uint32_t n_bands, am_band_params* out);

/* ---- per-hit significance --------------------------------------------------------- */
/* How far a hit stands out from the scores around it: the peak-to-sidelobe measure of matched filtering.  NCC
 * (am_hit_scores) says how well the window matches the needle; it cannot tell a certain hit under a loud voice-over
 * (NCC 0.3, 100 sigma above its surroundings) from an ambiguous one in tonal material (NCC 0.8, 4 sigma).
 * With t = peak.start, S the needle's length, G = sp->guard, B = sp->radius, lo = max(0, t - B) and
 * hi = min(len - S, t + B):
 *   span        the samples x[lo, hi + S); for AM_FMT_S16_STEREO the bit-exact down-mix of those frames, as above.
 *   scores      r(u), u in [lo, hi]: exactly the f32 scores am_correlate returns for the span as a buffer of its own with
 *               AM_MODE_VALID and AM_SCALE_LIB under the options in force at call time -- the same transform pass with
 *               lead 0, the same half-precision redo and, under "score_norm", the same normalisation with the same
 *               floor (the scores are then NCC).
 *   background  U = { u in [lo, hi] : |u - t| > G },  n_bg = |U|.  Lags within G of the hit are its own autocorrelation
 *               lobes; G = S - 1 clears them all.
 *   reductions  in f64 over the f32 scores, in one fixed order that depends on this hit's zone only, each result
 *               rounded to f32 once, at the end:
 *                 bg_mean  = sum_U r / n_bg
 *                 bg_std   = sqrt( sum_U (r - mean)^2 / n_bg )     (two passes, not E[r^2] - mean^2)
 *                 z        = (r(t) - mean) / std
 *                 side_max = max_U r, side_lag = u - t of that score; ties go to the smaller |u - t|, then to the
 *                            negative lag.
 *   flags       AM_HIT_NONFINITE: a sample of the span, or of the needle, is not finite; the five float fields are NaN,
 *               side_lag = 0, n_bg as counted; no flag but AM_HIT_CLIPPED beside it.
 *               AM_HIT_NO_BACKGROUND: n_bg < 2; score is given, bg_mean, bg_std, z and side_max are NaN, side_lag = 0.
 *               AM_HIT_FLAT_BACKGROUND: std == 0; z is +inf, -inf or 0 by the sign of score - mean.
 *               AM_HIT_CLIPPED: lo > t - B or hi < t + B (the zone is cut by an end of the haystack); informational,
 *               combines with any other flag.
 * A hit's record depends on the needle, the samples of its span, G, B and the options only -- not on the other hits, the
 * batch or the entry point: every hit's span is correlated on its own even where spans overlap, and the three forms
 * below agree bit for bit.  A hit costs the transforms of one am_correlate_device call of its span's length plus a reduction
 * of about a quarter of their time (tools/hit_significance_bench.py, profiles/r13/).  A second occurrence of the needle inside the zone raises bg_std and side_max: by design.
 * peaks and out are host memory, out[i] scores peaks[i]; len counts samples (frames for AM_FMT_S16_STEREO).
 * AM_ERR_INVALID_ARG, naming the hit (and pair): a null pointer with n > 0, sp == NULL, guard >= radius,
 * radius > AM_SIG_MAX_RADIUS, an unknown sample format, peak.start + S > len, a haystack on another device than the
 * needle.  n = 0: AM_OK, nothing launched. */
enum { AM_HIT_NO_BACKGROUND = 16, AM_HIT_FLAT_BACKGROUND = 32, AM_HIT_CLIPPED = 64 };
#define AM_SIG_MAX_RADIUS (1u << 22)
typedef struct am_significance_params {
    uint64_t guard;    /* G: lags with |u - t| <= G are not background (the hit's own autocorrelation lobes; S - 1 clears them) */
    uint64_t radius;   /* B: lags with G < |u - t| <= B are background; G < B <= AM_SIG_MAX_RADIUS */
} am_significance_params;
typedef struct am_significance {
    float score;       /* r(t) */
    float bg_mean;     /* mean of the background scores */
    float bg_std;      /* their population standard deviation */
    float z;           /* (r(t) - mean) / std */
    float side_max;    /* largest background score */
    int32_t side_lag;  /* its lag relative to t */
    uint32_t n_bg;     /* background lags counted */
    uint32_t flags;    /* AM_HIT_* */
} am_significance;      /* 32 bytes, no padding */
/* the haystack resident on the needle's device */
int am_hit_significance_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                               const am_peak* peaks, size_t n, const am_significance_params* sp, am_significance* out);
/* the haystack in host memory: only the spans [lo, hi + S) of the hits are copied (merged where they overlap) */
int am_hit_significance(const am_needle* h, const void* haystack, size_t len, int sample_format,
                        const am_peak* peaks, size_t n, const am_significance_params* sp, am_significance* out);
/* the pair layout of am_hit_scores_batch_device (other slots stay untouched), needles of any lengths */
int am_hit_significance_batch_device(const am_needle* const* needles, size_t n_needles,
                                     const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                     const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                     const am_significance_params* sp, am_significance* out);

/* ---- streaming ingest ---------------------------------------------------------- */
/* calc_chunks consumes a lazy ExactSizeIterator<Item = f32> (audio_matcher.rs:88-97): the decoder
 * yields frames (mp3_reader.rs:13-41) and the windows are cut as they arrive (:104).  The same
 * here: begin a stream (expected_len = the iterator's size hint, mp3_duration x sample rate,
 * matcher/mod.rs:77-83; 0 = unknown), push blocks of `sample_format` samples from host memory as
 * the decoder produces them, finish.  Every push is copied on a copy stream and the transforms of
 * every block pair whose samples have arrived completely are launched at once, so copying (or
 * decoding) and matching overlap; finish runs what is left, picks the peaks and returns exactly
 * what am_match / am_match_pcm16 return for the concatenated samples, bit for bit.  After finish
 * the stream is empty again and can take the next file.  One producer per stream; streams on one
 * device share its queue.
 * A push never waits for the device when the piece is small (below 1 MB: the decoder's 1152-frame pieces,
 * mp3_reader.rs:28-37): it is a host memcpy into a two-slot pinned staging ring, and a full slot (4 MB) leaves as
 * one asynchronous copy while the other fills.  A larger piece is copied straight from the caller's buffer -- at link
 * speed when that buffer is pinned (am_host_alloc / am_host_register) -- and push returns when the copy has left it.
 * `samples` may be reused as soon as push returns, either way. */
typedef struct am_stream am_stream;
int am_match_stream_begin(const am_needle* h, int sample_format, size_t expected_len, const am_match_params* p, am_stream** out);
int am_match_stream_push(am_stream* st, const void* samples, size_t n);
int am_match_stream_finish(am_stream* st, am_peak* out, size_t cap, size_t* n_out);
void am_match_stream_destroy(am_stream* st);

/* find_peaks(y_data, sr, PeakConfig) (audio_matcher.rs:221-230) =
 * PeakFinder::new(y).with_min_prominence(p).with_min_distance(d).find_peaks()
 * on one host score array; peaks come back by descending height. */
int am_find_peaks(int device, const float* scores, size_t n, float min_prominence,
                  uint64_t min_distance, am_peak* out, size_t cap, size_t* n_out);

/* ---- the k best matches -------------------------------------------------------------------------------------
 * "Where are the k places this needle fits best?" without a prominence threshold ("The k best
 * matches").
 *
 * am_find_peaks_top(scores, n, k, p, d) returns the first min(k, count) entries of what
 * am_find_peaks(scores, n, p, d) returns: the same peaks in the same order (descending height, ties by ascending
 * start), bit for bit in start, end, height and prominence, under every value of the options "peak_filter_order" and
 * "distance_rule".  A non-finite score splits the array: every finite stretch is its own find_peaks array (no peak
 * at its ends; prominence walks and plateaus stop there); the distance rule and k apply to the union.  For an
 * all-finite array the result is exactly am_find_peaks[:k].  Selection runs on the device without computing the
 * prominence of every local maximum: a height histogram of the maxima picks a threshold that leaves a few thousand
 * candidates, whose prominences are walked and filtered; the threshold is lowered while fewer than k survive.
 * *n_out = the number of peaks written (< k when fewer exist: not an error).  out: k slots.  k == 0 or a null
 * pointer: AM_ERR_INVALID_ARG.
 *
 * am_match_best(h, haystack, len, fmt, bp) = am_find_peaks_top over the haystack's AM_MODE_VALID correlation scores
 * (one array, no chunks): on a finite f32 haystack exactly the scores am_correlate_device(h, haystack, len,
 * AM_MODE_VALID, bp->scale) writes, "score_norm" (NCC) included.  AM_FMT_S16_STEREO: the bit-exact down-mix, then as
 * for f32.  A window that holds a non-finite sample has no score (NaN, which splits the array as above): every
 * finite stretch of at least S samples is correlated on its own.  A haystack shorter than the needle: 0 hits.
 * bp->scale must be AM_SCALE_NONE or AM_SCALE_LIB (AM_SCALE_MY depends on a chunk: AM_ERR_INVALID_ARG).
 * am_match_best_batch_device: n_hay resident haystacks, k slots and one count per haystack; each result is
 * bit-identical to its single call. */
typedef struct am_best_params {
    uint64_t k;              /* hits wanted, >= 1 */
    uint64_t min_distance;   /* samples, as am_match_params.min_distance (find_peaks' with_min_distance) */
    float min_prominence;    /* 0 = every local maximum competes */
    int scale;               /* AM_SCALE_NONE or AM_SCALE_LIB */
} am_best_params;

int am_match_best(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_best_params* bp, am_peak* out, size_t* n_out);
int am_match_best_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_best_params* bp, am_peak* out, size_t* n_out);
int am_match_best_batch_device(const am_needle* h, const void* const* d_haystacks, const size_t* lens,
                               size_t n_hay, int sample_format, const am_best_params* bp,
                               am_peak* out, size_t* n_out);
int am_find_peaks_top(int device, const float* scores, size_t n, float min_prominence,
                      uint64_t min_distance, size_t k, am_peak* out, size_t* n_out);
int am_find_peaks_top_device(int device, const float* d_scores, size_t n, float min_prominence,
                             uint64_t min_distance, size_t k, am_peak* out, size_t* n_out);

/* ---- score traces ------------------------------------------------------------------------------------------------
 * "What do the scores look like where there is no hit?" ("What the scores look like between the
 * hits"): per bin of D consecutive scores the largest and the smallest score with their places, how many scores are
 * not NaN, and their sum and sum of squares -- 40 bytes per bin instead of 4 bytes per score, the score array itself
 * never leaves the device.
 *
 * Scores.  am_match_trace(h, haystack, len, fmt, tp) reduces r[0, n), n = len - S + 1: exactly the array
 * am_match_best selects from.  On a finite f32 haystack these are the scores am_correlate_device(h, haystack, len,
 * AM_MODE_VALID, tp->scale) writes under the options in force, "score_norm" (NCC) and the half-precision redo
 * included.  AM_FMT_S16_STEREO: the bit-exact down-mix, then as for f32.  A window that holds a non-finite sample has
 * score NaN; every finite stretch of at least S samples is correlated on its own.  len < S: 0 bins, AM_OK.  tp->scale
 * must be AM_SCALE_NONE or AM_SCALE_LIB (AM_SCALE_MY depends on a chunk: AM_ERR_INVALID_ARG).  Device memory: 4 bytes
 * per score, as for am_match_best.
 *
 * Bins.  Bin b holds the scores [b D, min(n, (b + 1) D)), D = tp->bin, 1 <= D <= AM_TRACE_MAX_BIN; there are
 * nb = ceil(n / D) bins, one am_trace_bin each.  NaN scores are skipped; +-inf are scores like any other; -0.0 and
 * +0.0 compare equal, so the first one wins and its bits are returned.
 *
 * The order of the f64 additions depends on D and on a score's offset in its bin only -- not on the array's address
 * or alignment, the other bins, the batch or the entry point.  A span is the whole bin when D <=
 * AM_TRACE_WAVE_BIN_MAX, otherwise the bin's scores [s AM_TRACE_SLICE, (s + 1) AM_TRACE_SLICE) for s = 0, 1, ...
 * Within a span the score at offset j of the span belongs to class j mod 256; each class adds its scores (as f64; a
 * skipped score as +0.0) in ascending j, starting from +0.0; with c[k] the sum of class k,
 *     t[l] = (c[4l] + c[4l + 1]) + (c[4l + 2] + c[4l + 3]),  l = 0 .. 63,
 * and for m = 32, 16, 8, 4, 2, 1 in turn every t[l] becomes t[l] + t[l ^ m]; the span's sum is t[0].  A bin of several
 * spans adds their sums in ascending s, starting from +0.0.  sumsq likewise over (double)r (double)r, which is
 * exact, so only the additions round.  (The debug option "trace_form", 1 or 2, forces the first or the second rule
 * for every D: every field but sum / sumsq keeps its bits.)
 *
 * All entry points fill what fits and return AM_ERR_CAPACITY with *n_out = nb when cap < nb, like am_match; `out` is
 * host memory.  am_trace_scores / am_trace_scores_device are the reduction on any score array (host memory / memory
 * of `device` at any 4-byte alignment), as am_find_peaks / am_find_peaks_top_device are for the pick.
 * am_match_trace_batch_device: n_hay resident haystacks, cap_per_hay slots and one count per haystack; each
 * haystack's records are bit-identical to its single call.  AM_ERR_INVALID_ARG: a null pointer with work to do,
 * bin == 0 or bin > AM_TRACE_MAX_BIN, reserved != 0, an unknown format, AM_SCALE_MY, a haystack that is not on the
 * needle's device.
 *
 * am_trace_summary (pure host, f64) over the records of one array: the count, the global max and min with their
 * absolute score offsets (ties to the first), mean and population standard deviation from the sums (var =
 * sumsq / count - mean^2, clamped at 0), the median and the MAD of the bin maxima over the bins with count > 0, and
 * peak_z = (max - median) / (1.4826 MAD) (+inf when MAD = 0 and max > median, otherwise 0 when MAD = 0).  No bins or
 * no counted score: count 0, offsets 0, every other field NaN, AM_OK.  Infinite scores follow IEEE arithmetic (a mean or
 * std of inf - inf is NaN) with two rules of their own: a bin maximum equal to the median deviates from it by 0, also
 * when both are infinite, and when +inf and -inf are the two middle maxima there is no median: median_max, mad_max and
 * peak_z are NaN. */
#define AM_TRACE_WAVE_BIN_MAX 2048            /* bins up to this many scores: one wavefront per bin */
#define AM_TRACE_SLICE 8192                   /* longer bins: slices of this many scores, from the bin's start */
#define AM_TRACE_MAX_BIN (1ull << 30)
typedef struct am_trace_bin {
    float    max, min;        /* bits of the score at argmax / argmin; NaN when count == 0 */
    uint32_t argmax, argmin;  /* offset in the bin of the FIRST score equal (==) to max / min; 0 when count == 0 */
    uint32_t count;           /* scores of the bin that are not NaN */
    uint32_t reserved;        /* 0 */
    double   sum, sumsq;      /* over the counted scores, each converted to f64 first; +0.0 when count == 0 */
} am_trace_bin;               /* 40 bytes, no padding */
typedef struct am_trace_params {
    uint64_t bin;             /* D: scores per bin, 1 .. AM_TRACE_MAX_BIN */
    int scale;                /* AM_SCALE_NONE or AM_SCALE_LIB */
    uint32_t reserved;        /* 0 */
} am_trace_params;
typedef struct am_trace_stats {
    uint64_t count;           /* counted scores of all bins */
    uint64_t argmax, argmin;  /* absolute score offsets of the global max / min */
    double max, min;
    double mean, std;         /* of the counted scores */
    double median_max, mad_max;   /* median of the bin maxima and their median absolute deviation from it */
    double peak_z;
} am_trace_stats;             /* 80 bytes, no padding */

int am_trace_len(size_t n_scores, uint64_t bin, size_t* n_bins);
int am_trace_scores(int device, const float* scores, size_t n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out);
int am_trace_scores_device(int device, const float* d_scores, size_t n, uint64_t bin, am_trace_bin* out, size_t cap,
                           size_t* n_out);
int am_match_trace(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_trace_params* tp,
                   am_trace_bin* out, size_t cap, size_t* n_out);
int am_match_trace_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                          const am_trace_params* tp, am_trace_bin* out, size_t cap, size_t* n_out);
int am_match_trace_batch_device(const am_needle* h, const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                                int sample_format, const am_trace_params* tp, am_trace_bin* out, size_t cap_per_hay,
                                size_t* n_out);
int am_trace_summary(const am_trace_bin* bins, size_t n_bins, uint64_t bin, am_trace_stats* out);

/* ---- needle discovery ----------------------------------------------------------------------------------------------
 * "What do these two recordings share?" when nobody has cut a needle yet ("When there is no needle
 * yet"): probes cut from recording A at a fixed hop are matched against recording B, one record per probe says where
 * in B it scores best and how far ahead of its runner-up, and am_discover_regions (pure host) chains the probes that
 * agree on one displacement into regions.  A region's samples of A are a needle.
 *
 * Recordings.  A has len_a samples, B has len_b, both in sample_format (AM_FMT_F32_MONO, or AM_FMT_S16_STEREO with the
 * bit-exact down-mix of am_pcm16_downmix, done once per recording per call).
 *
 * Probes.  L = probe_len, H = hop.  Probe i is A[p_i, p_i + L), p_i = i H, i = 0 .. P - 1, P = (len_a - L) / H + 1, and
 * P = 0 when len_a < L (AM_OK, no records, as am_match_trace for len < S).  am_discover_len returns P.
 *
 * Scores of a probe: r_i[0, n), n = len_b - L + 1 -- exactly the array am_match_trace reduces for a needle created with
 * am_needle_create_device from the probe's (down-mixed) samples, with "score_norm" = 1 and AM_SCALE_LIB.  Discovery is
 * always NCC, whatever the process default of "score_norm" is; "score_norm_floor_db", "log_n" and "half_pipeline"
 * apply as they do to such a needle, the half-precision redo included.  A window of B that holds a non-finite sample
 * scores NaN.  len_b < L: n = 0, no probe has a candidate.
 *
 * Candidates of probe i: the offsets j in [0, n) whose score is not NaN and which are not excluded.  With flag
 * AM_DISCOVER_SELF the offsets p_i - exclude < j < p_i + exclude are excluded: the probe's own place and its overlap
 * (by position; pointers are never compared).  Without the flag `exclude` must be 0.
 *
 * Record of a probe (am_probe_hit).  best: the largest candidate, ties (==, so -0.0 and +0.0 tie) to the lowest
 * offset.  second: the largest candidate with |j - best| >= separation, the same tie rule; separation = 0 means L.
 * +-inf are scores like any other.  No candidate: AM_PROBE_NO_BEST | AM_PROBE_NO_SECOND, offsets 0, NaN scores.  A best
 * but no runner-up: AM_PROBE_NO_SECOND, second 0, ncc_second NaN.  Only comparisons are involved: every field is
 * defined to the bit.
 *
 * Skipped probes are not correlated: offsets 0, NaN scores and AM_PROBE_NONFINITE (the probe holds a non-finite
 * sample) or, checked second, AM_PROBE_QUIET: with E_i the probe's f64 sum of squares and E_ref = (f64 sum of squares
 * of A's finite samples) L / len_a, the probe is quiet when E_i = 0 or E_i < E_ref 10^(-min_level_db / 10) -- the NCC
 * of silence against anything is noise.  The order of these f64 additions is not part of the contract.
 *
 * am_probe_scores / am_probe_scores_device: the record rule on any score array (host memory / memory of `device` at
 * any 4-byte alignment) with the excluded range [ex_lo, ex_hi) (empty when ex_lo >= ex_hi) and separation >= 1;
 * `probe` of the record is 0.  It is to discovery what am_trace_scores is to the traces.
 *
 * Regions (am_discover_regions; integers and f64).  A probe is good when it has no flag other than
 * AM_PROBE_NO_SECOND, ncc >= min_ncc and -- when max_second > 0 and it has a runner-up -- (double)ncc_second <=
 * (double)max_second (double)ncc.  Its displacement is d = best - probe, signed.  The records are walked in index
 * order; their `probe` fields must ascend strictly (else AM_ERR_INVALID_ARG).  A chain starts at a good probe; with g
 * the chain's last good probe a later good probe joins when |d - d_g| <= tolerance, otherwise the chain ends at g and
 * the new probe starts the next chain; probes that are not good are bridged while no more than max_gap of them lie in
 * a row behind g, one more ends the chain at g.  A chain with at least min_good good probes is a region: a_start =
 * the first good probe's p, length = the last good probe's p + L - a_start, displacement = the lower median of the
 * good d (the B-side start is a_start + displacement), first = the index of the first good probe, count = the probes
 * from the first to the last good one, good = the good ones among them, mean_ncc = (f64 sum of the good ncc in index
 * order) / good, min_ncc = the smallest good ncc, worst_second = the largest ncc_second of the good probes that have a
 * runner-up (NaN: none has).  AM_REGION_FOLD (only with AM_DISCOVER_SELF in dp->flags): a region R with negative
 * displacement is dropped when an earlier kept region K with positive displacement has |K.d + R.d| <= tolerance and
 * [K.a_start + K.d, + K.length) overlaps [R.a_start, + R.length): in a self search every repeat is seen from both of
 * its occurrences, and the fold reports it once.  A region is exact to one hop; am_hit_segments on the cut refines it.
 *
 * Outputs are host memory; cap < count: AM_ERR_CAPACITY with what fits filled and the full count in *n_out.
 * AM_ERR_INVALID_ARG (the message names the field): a null pointer, reserved != 0, probe_len = 0, hop = 0, exclude
 * without AM_DISCOVER_SELF, unknown flags, a NaN min_level_db / min_ncc / max_second, a bad format, a pointer that is
 * not on `device` (am_discover_device, am_probe_scores_device), separation = 0 (am_probe_scores*).
 * Device memory: 4 bytes per score of one probe (the context's score buffer, as for am_match_best) and a mono copy of
 * each i16 recording. */
#define AM_DISCOVER_SELF 1u                   /* am_discover_params.flags: B is A; exclude each probe's own place */
#define AM_REGION_FOLD 1u                     /* am_region_params.flags: report a repeat of a self search once */
#define AM_PROBE_NO_BEST 1u                   /* am_probe_hit.flags */
#define AM_PROBE_NO_SECOND 2u
#define AM_PROBE_NONFINITE 4u
#define AM_PROBE_QUIET 8u
#define AM_DISCOVER_SLICE 8192                /* scores one wavefront reduces; the finish kernel folds the slices */
typedef struct am_probe_hit {
    uint64_t probe;           /* p_i: the probe's first sample in A */
    uint64_t best, second;    /* score offsets (first sample of the window in B) */
    float    ncc, ncc_second; /* bits of the scores at best / second; NaN where there is none */
    uint32_t flags;           /* AM_PROBE_* */
    uint32_t reserved;        /* 0 */
} am_probe_hit;               /* 40 bytes, no padding */
typedef struct am_discover_params {
    uint64_t probe_len, hop;  /* L, H: at least 1 */
    uint64_t exclude;         /* with AM_DISCOVER_SELF: p - exclude < j < p + exclude is no candidate; else 0 */
    uint64_t separation;      /* least distance of the runner-up from the best; 0 = L */
    float    min_level_db;    /* a probe more than this many dB below A's level is AM_PROBE_QUIET */
    uint32_t flags;           /* AM_DISCOVER_SELF */
    uint32_t reserved;        /* 0 */
} am_discover_params;
typedef struct am_region_params {
    float    min_ncc;         /* a good probe scores at least this */
    float    max_second;      /* > 0: ... and its runner-up at most max_second ncc */
    uint64_t tolerance;       /* displacements of one chain differ by at most this from one good probe to the next */
    uint32_t min_good;        /* good probes a region needs */
    uint32_t max_gap;         /* probes that are not good a chain bridges in a row */
    uint32_t flags;           /* AM_REGION_FOLD */
    uint32_t reserved;        /* 0 */
} am_region_params;
typedef struct am_region {
    uint64_t a_start, length; /* samples of A */
    int64_t  displacement;    /* B-side start = a_start + displacement */
    uint64_t first;           /* index of the first good probe */
    uint32_t count, good;     /* probes from the first to the last good one; the good ones among them */
    double   mean_ncc;
    float    min_ncc, worst_second;
} am_region;                  /* 56 bytes, no padding */

int am_discover_len(size_t len_a, const am_discover_params* dp, size_t* n_probes);
int am_discover_device(int device, const void* d_a, size_t len_a, const void* d_b, size_t len_b,
                       int sample_format, const am_discover_params* dp,
                       am_probe_hit* out, size_t cap, size_t* n_out);
int am_discover(int device, const void* a, size_t len_a, const void* b, size_t len_b,
                int sample_format, const am_discover_params* dp,
                am_probe_hit* out, size_t cap, size_t* n_out);
int am_probe_scores(int device, const float* scores, size_t n, uint64_t ex_lo, uint64_t ex_hi,
                    uint64_t separation, am_probe_hit* out);
int am_probe_scores_device(int device, const float* d_scores, size_t n, uint64_t ex_lo, uint64_t ex_hi,
                           uint64_t separation, am_probe_hit* out);
int am_discover_regions(const am_probe_hit* hits, size_t n, const am_discover_params* dp,
                        const am_region_params* rp, am_region* out, size_t cap, size_t* n_out);

/* ---- edge matching: a needle cut off by a recording's start or end -------------------------------------------------
 * Every entry point above that finds a needle scores whole windows only: an occurrence that begins before the
 * recording does, or ends after it, is invisible to them ("When a recording starts or ends inside the
 * needle").  This family scores the partial overlaps at the two edges, each normalised by the energy of the part of
 * the needle that lies inside the recording.
 *
 * Needle n[0, S), the handle's whole needle.  Haystack x[0, len), f32 mono or, for AM_FMT_S16_STEREO, the bit-exact
 * down-mix of am_pcm16_downmix.  A lag u (signed) puts n[0] at x[u].
 *   Head lags  u < 0 and u + S <= len: the needle's first k = -u samples are missing, the overlap is L = S + u.  In f64
 *              c(u) = sum_{i<L} x[i] n[k+i],  E_n(u) = sum_{i>=k} n[i]^2 (a suffix sum),  E_x(u) = sum_{i<L} x[i]^2 (a prefix sum).
 *              They are u = -(S - 1) .. min(-1, len - S): min(len, S - 1) lags.
 *   Tail lags  u >= 0 and u + S > len: the overlap is L = len - u.  In f64
 *              c(u) = sum_{i<L} x[u+i] n[i],  E_n(u) = sum_{i<L} n[i]^2 (a prefix sum),  E_x(u) = sum_{i>=u} x[i]^2 (a suffix sum).
 *              They are u = max(0, len - S + 1) .. len - 1: min(len, S - 1) lags.
 *   Lags cut at BOTH ends (u < 0 and u + S > len; they exist only when len < S) are not in scope: a clip that lies
 *   inside the needle is am_match with the roles swapped -- a needle handle made from the clip, the needle as haystack.
 *   A needle of one sample has no edge lags.  am_edge_scores_len (pure host) returns an edge's lag count and first lag.
 * Every energy is a pure prefix or suffix sum of non-negative terms, never a difference of two prefix values.
 *
 * Score: ncc(u) = c(u) / sqrt(E_n(u) E_x(u)); 0 when E_x(u) = 0 or E_x(u) < E_n(u) 10^(-score_norm_floor_db / 10) (the
 * process option, as am_hit_scores reads it) -- such a lag stays a candidate with score 0 -- and 0 when E_n(u) = 0.
 * Candidates of an edge: its lags with L >= min_overlap, E_n(u) >= (double)min_share E_n (in f64; E_n the needle's
 * energy) and no non-finite haystack sample in the overlap.  Non-finite haystack samples are zeroed in the copy of the
 * span that is correlated, so they cost exactly the lags whose overlap contains them: at the head the lags with L
 * greater than the index of the first non-finite sample, at the tail the lags u at or before the last one.  A non-finite
 * needle sample: both records carry AM_EDGE_NONFINITE and NaN scores, every coarse score is NaN, nothing is launched.
 * Spans read: head x[0, min(len, S - 1)), tail x[max(0, len - S + 1), len); the host forms copy only these.
 *
 * Two stages, as in discovery.  COARSE scores (am_edge_scores*): f32, one per lag of the edge in ascending u, NaN where
 * the lag is no candidate.  c(u) comes from the f32 transforms of the overlap-save engine over the span -- always f32,
 * whatever "half_pipeline" says, "score_norm" is ignored, "log_n" applies --, the quotient is taken with the f64
 * energies and rounded once.  Coarse scores are not defined to the bit.  RECORD per edge (am_edge_hit): start is the
 * largest coarse candidate, ties to the lowest u; second is the largest coarse candidate with |u - start| >= separation
 * (separation = 0 means min_overlap), the same tie rule -- exactly the rule of am_probe_scores on the coarse array.  No
 * candidate: AM_EDGE_NO_BEST | AM_EDGE_NO_SECOND, lags 0, overlap 0, NaN scores.  No runner-up: AM_EDGE_NO_SECOND, second
 * 0, ncc_second NaN.  The two chosen lags are then scored again exactly, by direct f64 sums on the device (the order of
 * the additions is not part of the contract): ncc, ncc_second, gain = c / E_n(u) (0 when E_n(u) = 0), share = E_n(u) /
 * E_n, overlap = L, each rounded once to f32; AM_EDGE_BELOW_FLOOR when the best lag's exact score fell under the floor
 * rule.  A record depends on the needle, the span and the parameters only: the three am_match_edges* forms agree bit
 * for bit, alone and in any batch.
 *
 * The kernels (am_edges.hip): one pass per span (down-mix, zeroing, first / last non-finite index); four f64 energy
 * scans (the needle's two are kept on the handle), each in three launches of a fixed order over tiles of AM_EDGE_TILE
 * elements; the engine's transforms; one normalising launch; the record rule; one launch for the exact sums of the at
 * most four chosen lags and one that folds them.  Profile class "edges".
 *
 * Outputs are host memory.  am_edge_scores*: cap < n_lags gives AM_ERR_CAPACITY with the count in *n_out.  out of
 * am_match_edges*: [0] the head's record, [1] the tail's; the batch form writes two per haystack.
 * AM_ERR_INVALID_ARG (the message names the field): a null pointer, reserved != 0, min_overlap = 0, min_share NaN or
 * outside [0, 1], a bad format or edge, len = 0, a haystack that is not on the needle's device (_device forms). */
enum { AM_EDGE_HEAD = 0, AM_EDGE_TAIL = 1 };
#define AM_EDGE_NO_BEST 1u                    /* am_edge_hit.flags */
#define AM_EDGE_NO_SECOND 2u
#define AM_EDGE_NONFINITE 4u
#define AM_EDGE_BELOW_FLOOR 8u
#define AM_EDGE_TILE 4096                     /* elements per tile of the three-phase energy scans */
typedef struct am_edge_params {
    uint64_t min_overlap;     /* least overlap L of a candidate: at least 1 */
    uint64_t separation;      /* least distance of the runner-up from the best; 0 = min_overlap */
    float    min_share;       /* least E_n(u) / E_n of a candidate, in [0, 1] */
    uint32_t reserved;        /* 0 */
} am_edge_params;             /* 24 bytes */
typedef struct am_edge_hit {
    int64_t  start, second;   /* the lags u of the best and of the runner-up */
    uint64_t overlap;         /* L of the best */
    float    ncc, ncc_second; /* exact scores; NaN where there is none */
    float    gain, share;     /* c / E_n(u) and E_n(u) / E_n of the best */
    uint32_t edge, flags;     /* AM_EDGE_HEAD / AM_EDGE_TAIL; AM_EDGE_* */
} am_edge_hit;                /* 48 bytes, no padding */

int am_edge_scores_len(size_t len, size_t s, int edge, size_t* n_lags, int64_t* first_lag);
int am_edge_scores_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, int edge,
                          const am_edge_params* ep, float* out, size_t cap, size_t* n_out);
int am_edge_scores(const am_needle* h, const void* haystack, size_t len, int sample_format, int edge,
                   const am_edge_params* ep, float* out, size_t cap, size_t* n_out);
int am_match_edges_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                          const am_edge_params* ep, am_edge_hit* out);
int am_match_edges(const am_needle* h, const void* haystack, size_t len, int sample_format,
                   const am_edge_params* ep, am_edge_hit* out);
int am_match_edges_batch_device(const am_needle* h, const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                                int sample_format, const am_edge_params* ep, am_edge_hit* out);

/* ---- envelope matching: a needle played at another speed --------------------------------------------------------
 * Every entry point above that FINDS a needle correlates waveforms: it finds an occurrence that runs on the needle's
 * clock and keeps the needle's phases ("When a hit runs on another clock": a 10 s needle is followed to
 * about 72 ppm).  A jingle from a playout machine running 3 % fast, a tape transfer or a chain that scrambles phases is
 * never a hit.  This family matches band-level envelopes instead: a few wide frequency bands, one level per band and
 * frame of a few milliseconds, the needle's level matrix correlated against the haystack's for each speed of a coarse
 * grid.  The reference has no such stage.
 *
 * WHAT IT IS GOOD FOR.  Positions are good to a few frames, not to the sample.  The drift is good to about one or two
 * grid steps on a 10 s needle and gets worse on shorter ones: its resolution is about (width of the envelope
 * correlation peak, in frames) / J -- with a 2 s needle detection still works but the drift is crude, 1 - 2 %.  Bands
 * should be wide, a third of an octave or more, so that the pitch shift of a speed change stays inside a band.
 * Refining such a hit to the sample is deliberately not part of this family: it would be a local waveform search over
 * +-H lags and a fine drift grid around each hit (am_hit_warp measures drift only up to AM_WARP_MAX_PPM).
 *
 * 1. The envelope of a signal (am_envelope_len, am_envelope, am_envelope_device).  ep->bands is an am_band_params as for
 *    am_hit_bands (am_band_edges_log fills one); F = 2^frame_log2, H = F / 2, B = n_bands.  d = drift_ppm, |d| <=
 *    AM_ENV_MAX_PPM.
 *   frames     inc = llround(2^32 / (1 + d 1e-6)) in f64 on the host (the convention of am_hit_warp); frame j starts at
 *              a_j = (j H inc + 2^31) >> 32 (u64; exactly j H for d = 0) and reads x[a_j .. a_j + F).  J = the count of j
 *              with a_j + F <= len, 0 for len < F; am_envelope_len returns it.  Positive d: the frames sit closer
 *              together -- the signal as it sounds when the occurrence is longer than the needle.  len <= AM_ENV_MAX_LEN.
 *   band power window w[i] = 0.5 - 0.5 cos(2 pi i / F), X_j[k] the F-point spectrum of the windowed frame in f64,
 *              P_b[j] = sum of |X_j[k]|^2 over the bins [edges[b], edges[b + 1]).  x is the f32 sample or the bit-exact
 *              down-mix for AM_FMT_S16_STEREO.  Window and twiddles come from the host f64 table of am_hit_bands.
 *   level      P0 = (F / 4)^2 10^(-floor_db / 10) ((F / 4)^2: the band power of a full-scale sine), v = 10 log10((P_b[j] +
 *              P0) / P0), u_b[j] = min(llround(AM_ENV_STEPS_PER_DB v), AM_ENV_MAX_LEVEL) as uint16_t.  A frame of zeros
 *              gives exactly 0.  The order of the f64 additions is not part of the contract: an implementation may differ
 *              from another by 1 in cells whose 8 v lies within rounding of a half-integer (about 2 cells in a million).
 *   absent     a frame that reads a non-finite sample is ABSENT: every band of it holds AM_ENV_ABSENT.
 *   output     B x J levels, band-major (band b frame j at out[b J + j]), host memory.  cap counts frames: with cap < J
 *              nothing is written and the call returns AM_ERR_CAPACITY with J in *n_frames.
 *   Levels are integers on purpose: everything downstream is exact integer arithmetic, any order of additions gives
 *   the same bits.
 *
 * 2. Scores of a bank of needle envelopes against a haystack envelope (am_envelope_scores, am_envelope_scores_device).
 *   Q = n_needles matrices n_q of B x J_q levels (J_q = frames[q], 1 .. AM_ENV_MAX_FRAMES; 1 <= Q <= AM_ENV_MAX_NEEDLES;
 *   B <= AM_BAND_MAX_BANDS), one behind the other in `needles` (matrix q starts at B sum_{p < q} J_p), and one haystack
 *   matrix e of B x Jh levels (Jh <= AM_ENV_MAX_HAY_FRAMES).  A level is 0 .. AM_ENV_MAX_LEVEL or AM_ENV_ABSENT; a frame
 *   is absent when a band of it holds AM_ENV_ABSENT.
 *   T_q = Jh - J_q + 1 (0 if negative), n_out = max_q T_q.  For t < T_q, with J = J_q, all integers:
 *     xc_b = sum_j n_q,b[j] e_b[t + j],  s1_b = sum_j e_b[t + j],  s2_b = sum_j e_b[t + j]^2,
 *     N1_b = sum_j n_q,b[j],  N2_b = sum_j n_q,b[j]^2,
 *     num = sum_b (J xc_b - N1_b s1_b),   D = sum_b (J s2_b - s1_b^2),   E = sum_b (J N2_b - N1_b^2),
 *     score_q[t] = fl32((double)num / sqrt((double)E (double)D)).
 *   The three integers are below 2^53 within the limits (16384^2 32 1023^2 < 2^53): their conversion is exact, the f64
 *   multiply, sqrt and divide are rounded once each, so every score is defined to the bit.  The score is 0 where E = 0
 *   or D = 0 (exact tests: a flat needle, a flat window such as digital silence) and NaN where the window or the needle
 *   matrix holds an absent frame.
 *   z[t] = the largest non-NaN score_q[t] over the q with t < T_q (NaN if there is none), qi[t] = its q, ties to the
 *   lower q (AM_ENV_NO_Q beside a NaN).  Both have n_out entries in host memory; cap < n_out: AM_ERR_CAPACITY with what
 *   fits filled and n_out in *n_out.
 *   The kernels (am_envelope.hip): the haystack's prefix sums of e, e^2 and the absent marks (64-bit integers), then ONE
 *   correlation launch in which a workgroup owns AM_ENV_TILE consecutive t, keeps the haystack rows it needs in LDS,
 *   walks every needle in chunks of AM_ENV_CHUNK frames with packed 16-bit dot products (32-bit sums over at most 4096
 *   products, then 64-bit) and folds the best (score, q) in registers: one haystack tile is read once for all Q.
 *
 * 3. The pick rule (am_envelope_pick, pure host).  Position t is kept iff z[t] is not NaN, z[t] >= min_score, no t' with
 *   |t' - t| <= separation has z[t'] > z[t], and no such t' < t has z[t'] == z[t].  The output ascends in t.  Record:
 *   frame = t; pos = t + e, e the vertex (a - c) / (2 (a - 2 b + c)) of the parabola through a = z[t - 1], b = z[t],
 *   c = z[t + 1] in f64, clamped to +-0.5, and e = 0 at an end, beside a NaN or without a maximum (a - 2 b + c >= 0);
 *   score = z[t]; q = qi[t].
 *
 * 4. The composition (am_match_envelope, am_match_envelope_device).  The grid's Q = 2 K + 1 drifts are d_q = centre_ppm +
 *   max_ppm (q - K) / K as for am_warp_params (K = 0: the one drift centre_ppm), K <= AM_ENV_MAX_STEPS, max_ppm >= 0 and
 *   > 0 when K > 0, |centre_ppm| + max_ppm <= AM_ENV_MAX_PPM.  The needle's envelope at each d_q comes from the handle's
 *   whole needle on the device, the haystack's envelope at d = 0; then the scores, then the pick with separation = J_K
 *   (the needle's frames at the centre drift).  Record am_env_hit: start = llround(pos H) clamped into [0, len),
 *   drift_ppm = d_q, score, q, length = llround(S (1 + d_q 1e-6)).  Envelopes and scores stay on the device; only z and qi
 *   (4 + 4 bytes per frame) and the hits come up.  The result does not depend on "score_norm" or any other process option.
 *   A needle shorter than F (the first frame starts at 0 at every rate), or with more than AM_ENV_MAX_FRAMES frames at a
 *   rate of the grid (use a larger frame_log2), is AM_ERR_INVALID_ARG.
 *   len < F or fewer haystack frames than every needle envelope: AM_OK, no hits.
 *
 * AM_ERR_INVALID_ARG (the message names the field): a null pointer, reserved != 0, the rules of am_band_params, floor_db
 * outside (0, 200] or NaN, |drift_ppm| > AM_ENV_MAX_PPM or NaN, len > AM_ENV_MAX_LEN, a bad sample format, a pointer that
 * is not on the device (_device forms), n_needles = 0 or > AM_ENV_MAX_NEEDLES, n_bands = 0 or > AM_BAND_MAX_BANDS,
 * frames[q] = 0 or > AM_ENV_MAX_FRAMES, hay_frames > AM_ENV_MAX_HAY_FRAMES, a level above AM_ENV_MAX_LEVEL other than
 * AM_ENV_ABSENT, a NaN min_score, the grid's rules.
 * Measured on an MI355X: tools/envelope_bench.py, profiles/r25/. */
#define AM_ENV_STEPS_PER_DB   8
#define AM_ENV_MAX_LEVEL      1023
#define AM_ENV_ABSENT         0xFFFFu
#define AM_ENV_NO_Q           0xFFFFFFFFu
#define AM_ENV_MAX_PPM        250000
#define AM_ENV_MAX_FRAMES     16384
#define AM_ENV_MAX_NEEDLES    257
#define AM_ENV_MAX_STEPS      128
#define AM_ENV_MAX_LEN        (1ull << 31)
#define AM_ENV_MAX_HAY_FRAMES (1u << 24)
#define AM_ENV_TILE           512               /* consecutive t one workgroup of the correlation kernel owns */
#define AM_ENV_CHUNK          8                 /* needle frames per step of its inner loop */
typedef struct am_env_params {
    am_band_params bands;     /* frame_log2, B and the band edges, as for am_hit_bands */
    uint32_t reserved;        /* 0 */
    double   floor_db;        /* P0 lies this many dB below a full-scale sine; 80 is a good default */
} am_env_params;              /* 152 bytes, no padding */
typedef struct am_env_grid {
    double   centre_ppm;      /* the middle of the drift grid */
    double   max_ppm;         /* its half width */
    uint32_t steps;           /* K, 0 .. AM_ENV_MAX_STEPS: 2 K + 1 drifts */
    uint32_t reserved;        /* 0 */
} am_env_grid;                /* 24 bytes, no padding */
typedef struct am_env_pick {
    uint64_t frame;           /* t */
    double   pos;             /* t + the parabola's vertex, in frames */
    float    score;           /* z[t] */
    uint32_t q;               /* qi[t] */
} am_env_pick;                /* 24 bytes, no padding */
typedef struct am_env_hit {
    uint64_t start;           /* llround(pos H), clamped into [0, len): good to a few frames */
    uint64_t length;          /* llround(S (1 + d_q 1e-6)): the occurrence's length in haystack samples */
    double   drift_ppm;       /* d_q */
    float    score;
    uint32_t q;
} am_env_hit;                 /* 32 bytes, no padding */
int am_envelope_len(size_t len, const am_env_params* ep, double drift_ppm, size_t* n_frames);
int am_envelope(int device, const void* signal, size_t len, int sample_format, const am_env_params* ep,
                double drift_ppm, uint16_t* out, size_t cap, size_t* n_frames);
int am_envelope_device(int device, const void* d_signal, size_t len, int sample_format, const am_env_params* ep,
                       double drift_ppm, uint16_t* out, size_t cap, size_t* n_frames);
int am_envelope_scores(int device, const uint16_t* needles, const uint32_t* frames, uint32_t n_needles,
                       uint32_t n_bands, const uint16_t* hay, size_t hay_frames,
                       float* z, uint32_t* qi, size_t cap, size_t* n_out);
/* needles and hay in memory of `device` (2-byte aligned); frames, z and qi in host memory */
int am_envelope_scores_device(int device, const uint16_t* d_needles, const uint32_t* frames, uint32_t n_needles,
                              uint32_t n_bands, const uint16_t* d_hay, size_t hay_frames,
                              float* z, uint32_t* qi, size_t cap, size_t* n_out);
int am_envelope_pick(const float* z, const uint32_t* qi, size_t n, float min_score, uint64_t separation,
                     am_env_pick* out, size_t cap, size_t* n_out);
int am_match_envelope(const am_needle* h, const void* haystack, size_t len, int sample_format,
                      const am_env_params* ep, const am_env_grid* grid, float min_score,
                      am_env_hit* out, size_t cap, size_t* n_out);
int am_match_envelope_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                             const am_env_params* ep, const am_env_grid* grid, float min_score,
                             am_env_hit* out, size_t cap, size_t* n_out);


/* ---- ingest: PCM -> f32 mono -------------------------------------------- */
/* mp3_reader.rs:12, 28-37: mono = (l as f32 + r as f32) * 0.5 * (1/65535) */
int am_pcm_s16_stereo_to_mono(int device, const int16_t* interleaved, size_t frames, float* out);
int am_pcm_s16_stereo_to_mono_device(int device, const int16_t* d_interleaved, size_t frames,
                                     float* d_out);
/* A stereo mix other than the down-mix (an extension; the reference knows the down-mix only):
 *     out[i] = fl32( ((double)a L[i] + (double)b R[i]) k ),   k = (double)(1.0f / 65535.0f)
 * Both products are exact in f64 (an f32 times an i16 value): one f64 sum, one f64 product, one rounding to f32, so the
 * result is defined bit for bit.  a = b = 0.5 gives exactly the bits of am_pcm_s16_stereo_to_mono; (1, 0) is left, (0, 1)
 * right, (0.5, -0.5) side.  Matching the f32 path on the side signal finds an insert that sits polarity-inverted in the
 * two channels and cancels in the down-mix; its hit positions are frame positions, so am_hit_stereo applies to them
 * unchanged.  Arguments and refusals as am_pcm_s16_stereo_to_mono*. */
int am_pcm_s16_stereo_mix(int device, const int16_t* interleaved, size_t frames, float a, float b, float* out);
int am_pcm_s16_stereo_mix_device(int device, const int16_t* d_interleaved, size_t frames, float a, float b,
                                 float* d_out);

/* ---- sample-rate conversion ---------------------------------------------- */
/* The reference refuses a snippet and a main file of different rates (matcher/mod.rs:72-74,
 * CliError::SampleRateMismatch).  These entry points bring a signal to another rate, normally the needle to the
 * haystack's rate: offsets then stay integers in haystack samples and every match, pool, hit-scoring and streaming
 * entry point works on the result unchanged.
 *
 * Let g = gcd(src_rate, dst_rate), L = dst_rate / g, M = src_rate / g, R = max(L, M), H = 10 R, c = 1 / R.  The filter,
 * computed on the host in f64 and stored as f32:
 *     h[j] = L * w[j] / sum_i w[i],   w[j] = c * sinc(c j) * I0(5 sqrt(1 - (j/H)^2)) / I0(5),   j = -H .. H
 * (sinc(x) = sin(pi x) / (pi x)).  The output length is n_out = ceil(n_in * L / M) and the output
 *     y[k] = sum over n in [0, n_in) with |k M - n L| <= H of  x[n] * h[k M - n L]
 * which is scipy.signal.resample_poly(x, L, M) with its default window (('kaiser', 5.0), half_len = 10 max(L, M)).
 *   x          f32 mono, or for AM_FMT_S16_STEREO the down-mix (l + r) * 0.5 * (1/65535) bit for bit as above; n_in counts
 *              samples, or frames for AM_FMT_S16_STEREO.
 *   src_rate == dst_rate: y = x, the input's bits (f32) or the down-mix's bits (i16).
 *   Non-finite samples spread, by IEEE arithmetic, to the outputs whose support holds them and to no others; the
 *   matcher then drops exactly those windows, as for any haystack.
 *   Accumulation is in one fixed order that depends on (L, M) alone -- phases of up to 48 taps as one f32 chain, longer
 *   ones as f32 sums of 8 taps added up in f64 -- so every entry point gives the same bits for the same input, and
 *   max |y - y_f64| <= 1e-5 max |x| for every accepted pair.  Index arithmetic is 64-bit.
 *   AM_ERR_INVALID_ARG: a rate outside [1, 768000], R > 8192 (every pair of 8, 11.025, 12, 16, 22.05, 24, 32, 44.1, 48,
 *   64, 88.2, 96, 176.4, 192 and 384 kHz is within it; the worst, 11025 <-> 384000, has R = 5120), an unknown sample
 *   format, a null pointer.  The filter table of each (L, M) is built once per device and kept until am_shutdown. */
/* pure host function (no device), like am_correlate_len: n_out = ceil(n_in * L / M); n_in = 0 gives 0 */
int am_resample_len(size_t n_in, uint32_t src_rate, uint32_t dst_rate, size_t* n_out);
/* Host memory in and out.  *n_out receives the output length; on AM_ERR_CAPACITY (cap < n_out) nothing is written
 * but *n_out, the required length.  n_in = 0: AM_OK, *n_out = 0, nothing launched. */
int am_resample(int device, const void* in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate,
                float* out, size_t cap, size_t* n_out);
/* the same on device pointers (resident on `device`, not overlapping); complete when the call returns.  One call
 * brings a whole haystack to another rate, e.g. a batch of mixed-rate archives to one rate for am_match_batch_device. */
int am_resample_device(int device, const void* d_in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate,
                       float* d_out, size_t cap, size_t* n_out);
/* LibConvolve::new(sample_data) (audio_matcher.rs:289) on a needle brought from src_rate to dst_rate: the handle
 * am_needle_create gives on am_resample's output, bit for bit (am_needle_len reports n_out).  Everything downstream is
 * unchanged.  Pools keep their own am_pool_create*: pass them am_resample's output. */
int am_needle_create_resampled(int device, const void* needle, size_t n, int sample_format, uint32_t src_rate,
                               uint32_t dst_rate, am_needle** out);

/* ---- spectral whitening --------------------------------------------------- */
/* The reference correlates the decoded samples as they are (audio_matcher.rs:297-343) and has no such stage.  Speech and
 * music are low-pass material: a plain cross-correlation of such signals is dominated by their few loudest low
 * frequencies, its peak is wide and unrelated programme scores a large fraction of a true hit.  The remedy is to pass
 * the needle AND every haystack through one short prediction-error (whitening) filter before they are correlated.
 * These entry points prepare the signals; every match, pool, streaming, monitor and per-hit entry point then works on
 * the prepared signals unchanged.
 *
 * In all of them `in` is f32 mono, or for AM_FMT_S16_STEREO interleaved i16 stereo frames, down-mixed
 * (l + r) * 0.5 * (1/65535) bit for bit as everywhere else; n counts samples, or frames for AM_FMT_S16_STEREO.
 *
 * What a caller must know:
 *   One filter for all.  The needle and every haystack it is matched against must pass through the SAME taps.  Design
 *     the filter from the haystacks (the programme), not from the needle: add the lag products of the files.
 *   Offsets do not move: the filter is causal and applied to both sides.
 *   Needle start.  The needle's first n_taps - 1 filtered samples see zero history, where its occurrence in a haystack
 *     sees the programme before it.  That affects (n_taps - 1) / S of the needle (S = its length); at S = 4096 and
 *     order 32 no loss was measured.
 *   Scores.  Heights, NCC and per-hit records are those of the whitened signals.
 *   Pre-emphasis.  A fixed pre-emphasis is just taps = {1, -alpha}. */
#define AM_WHITEN_MAX_ORDER 64
#define AM_FIR_MAX_TAPS     (AM_WHITEN_MAX_ORDER + 1)

/* Lag products:  r[k] = sum_{i=k}^{n-1} x~[i] * x~[i-k],  k = 0 .. order;  x~ = x, with 0 for a non-finite sample.
 * r: order + 1 doubles in host memory (both forms).
 *   Every product is formed in f64, where a product of two f32 values is exact.  The sums run in one fixed order that
 *   depends on n only: blocks of 8192 samples give one partial per lag each (a block reads the samples its lags reach
 *   in front of its first one: the previous block's, nothing before index 0), and the partials are added in block order.
 *   The host and the device form give the same bits, a device pointer of any 4-byte alignment gives the same bits, and
 *   r[k] does not depend on the `order` asked for.
 *   The products are additive: a caller designs one filter for a whole archive by adding the r of its files.
 *   n = 0: all zeros, AM_OK, nothing launched.
 *   AM_ERR_INVALID_ARG: order 0 or above AM_WHITEN_MAX_ORDER, an unknown sample format, a null pointer (in: with n > 0). */
int am_lag_products(int device, const void* in, size_t n, int sample_format, uint32_t order, double* r);
/* the same on a device pointer (resident on `device`); complete when the call returns */
int am_lag_products_device(int device, const void* d_in, size_t n, int sample_format, uint32_t order, double* r);

/* Pure host function (no device): the prediction-error filter a[0 .. order], a[0] = 1, of the lag products r[0 .. order]
 * by the Levinson-Durbin recursion in f64, with r[0] replaced by r[0] * (1 + 10^(-noise_db / 10)) (the usual white-noise
 * correction; noise_db in [0, 200], 60 is a good choice).  taps: order + 1 floats, each rounded to f32 once.
 *   The recursion stops before step m when the prediction error has reached <= 0, and at step m when the reflection
 *   coefficient has |k| >= 1 (or is not a number); the taps m .. order are then 0.  r[0] <= 0 (silence): the identity
 *   {1, 0, ...}.  On white input the filter is (nearly) the identity.
 *   AM_ERR_INVALID_ARG: a null pointer, order 0 or above AM_WHITEN_MAX_ORDER, a non-finite r[k], noise_db out of range. */
int am_whiten_taps(const double* r, uint32_t order, double noise_db, float* taps);

/* FIR filter:  y[k] = sum_{j < n_taps} taps[j] * x[lead + k - j],  k in [0, n_in - lead);  x = 0 before in[0].
 * Host memory in and out.  *n_out receives the output length n_in - lead; on AM_ERR_CAPACITY (cap < n_out) nothing is
 * written but *n_out.  n_in == lead: AM_OK, *n_out = 0, nothing launched.
 *   Each output is accumulated in f32 from 0 with one fma per tap, in the order j = 0, 1, ...; every entry point gives
 *   the same bits for the same input.  Non-finite samples spread, by IEEE arithmetic, to the n_taps outputs whose support
 *   holds them and to no others; the matcher then drops exactly those windows, as for any haystack.
 *   Pieces.  For any cut a < b, am_fir on x[a - l .. b) with lead = l = min(a, n_taps - 1) equals
 *   am_fir(x, lead = 0)[a .. b) bit for bit (the launch geometry depends on n_taps and on the output index relative to
 *   `lead` only): a streaming caller keeps n_taps - 1 samples of history and pushes the filtered pieces.
 *   AM_ERR_INVALID_ARG: n_taps 0 or above AM_FIR_MAX_TAPS, a non-finite tap, lead > n_in, an unknown sample format, a
 *   null pointer. */
int am_fir(int device, const void* in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps,
           size_t lead, float* out, size_t cap, size_t* n_out);
/* the same on device pointers (resident on `device`, not overlapping; taps in host memory); complete when the call
 * returns */
int am_fir_device(int device, const void* d_in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps,
                  size_t lead, float* d_out, size_t cap, size_t* n_out);
/* LibConvolve::new(sample_data) (audio_matcher.rs:289) on a filtered needle: the handle am_needle_create gives on
 * am_fir(needle, lead = 0)'s output, bit for bit (am_needle_len reports n).  Pools keep their own am_pool_create*: pass
 * them am_fir's output. */
int am_needle_create_filtered(int device, const void* needle, size_t n, int sample_format,
                              const float* taps, uint32_t n_taps, am_needle** out);

/* ---- needle estimation: a clean needle from the hits of a rough one ---------- */
/* The reference matches with the snippet as it was cut (LibConvolve::new, audio_matcher.rs:289) and has no such stage.
 * A needle cut by hand out of one broadcast carries what lay over the jingle that day.  After a first archive run the
 * caller holds a few dozen occurrences of the same jingle, each under different material, each with a known offset
 * (am_match*) and a known gain (am_hit_scores): stacked and aligned, a robust per-sample estimate of them is the jingle
 * itself.  A median over nine occurrences removes whatever lies over fewer than half of them; a mean only dilutes it.
 *
 * Rows.  A row is `length` f32 values for one occurrence.  For a hit with `start` and `scale` and the call's `lead`, row
 *   element n (0 <= n < length) reads haystack element e = start - lead + n:  v = fl32(x[e] * scale), one f32 multiply,
 *   x the f32 sample (for AM_FMT_S16_STEREO the down-mix (l + r) * 0.5 * (1/65535), bit for bit as everywhere else).
 *   The element is ABSENT when e lies outside [0, len) or x[e] is not finite.  In a row buffer an absent element is any
 *   non-finite value (a product that overflows is therefore absent as well); NaN is what the library writes.
 *   scale = 1 / gain of am_hit_scores brings every occurrence to the needle's level.
 * For output sample n: P_n = the present values over the hits, in hit order; c_n = |P_n|.
 * Total order.  Where values are ordered, the order is that of the monotone integer key of the f32 bits:
 *   bits ^ 0x80000000 for a non-negative sign, ~bits otherwise, compared unsigned: -0 before +0, every tie pinned.
 * Methods:
 *   AM_EST_MEAN     m = the f64 sum of P_n in hit order, divided by c_n.
 *   AM_EST_MEDIAN   odd c_n: m = the middle value of the sorted P_n; even: m = ((double)a + (double)b) / 2 of the two
 *                   middle values.
 *   AM_EST_TRIMMED  d = min(floor(c_n * trim_permille / 1000), (c_n - 1) / 2) values are dropped at each end of the sorted
 *                   P_n; m = the f64 sum of the rest in ascending order, divided by c_n - 2d.  trim_permille in [0, 500].
 * Outputs (host memory, `length` entries each; dev and count may be null):
 *   est[n]   = fl32(m), rounded once.
 *   dev[n]   = fl32(sqrt(sum over P_n in hit order of (v - m)^2 / c_n)), in f64 around the unrounded m: small where the
 *              occurrences agree.  Read with a margin (lead, and length beyond the rough needle) it shows where the jingle
 *              really begins and ends: the spread collapses exactly there.
 *   count[n] = c_n.
 *   Where c_n = 0: est = 0, dev = 0, count = 0; the result is always usable as a needle.
 * Limits.  AM_EST_MAX_HITS hits for MEDIAN and TRIMMED, 65535 for MEAN; length >= 1 and n >= 1; every scale finite and
 *   not zero; lead, length < 2^62.
 * Invariant.  A result depends on the rows' values, their order and the parameters only: all entry points give the same
 *   bits.  Exactness: where more than half of the present values of a sample are the same number, the median IS that
 *   number -- occurrences g_i * c with power-of-two gains under overlays that cover fewer than half of them give c back
 *   bit for bit.
 * Other clocks.  am_hit_window aligns to whole samples on the haystack's clock.  For occurrences whose clocks differ
 *   from the needle's, am_hit_window_warped (below) cuts the row on the needle's clock from am_hit_warp's `lag` and
 *   `drift_ppm`; its rows go into am_needle_estimate_rows like any others.
 * AM_ERR_INVALID_ARG (the message names the hit where one is at fault): a null pointer, an unknown method or sample
 *   format, trim_permille > 500, n = 0 or length = 0, n above the method's limit (the message states the limit),
 *   hits[i].haystack >= n_hay, a scale that is zero or not finite, a haystack that is not memory of `device`. */
#define AM_EST_MAX_HITS 64
enum { AM_EST_MEAN = 0, AM_EST_MEDIAN = 1, AM_EST_TRIMMED = 2 };
typedef struct am_estimate_params {
    uint32_t method;          /* AM_EST_* */
    uint32_t trim_permille;   /* AM_EST_TRIMMED: share dropped at each end, in 1/1000 (0..500); checked for every method */
    uint64_t lead;            /* elements read in front of each hit's start (the margin in front of the needle) */
    uint64_t length;          /* elements per row and per output */
} am_estimate_params;         /* 24 bytes, no padding */
typedef struct am_est_hit {
    uint64_t start;           /* the hit's start in its haystack (am_peak.start) */
    uint32_t haystack;        /* index into d_haystacks */
    float scale;              /* 1 / gain */
} am_est_hit;                 /* 16 bytes */
/* Pure host function (no device): one row cut out of a host haystack, as defined above (NaN for absent).  len counts
 * samples (frames for AM_FMT_S16_STEREO); row: length floats.  A caller that holds one file at a time cuts each hit's
 * row while the file is in memory and estimates at the end. */
int am_hit_window(const void* haystack, size_t len, int sample_format, uint64_t start, float scale,
                  uint64_t lead, uint64_t length, float* row);
/* rows: n x length f32 in host memory, row-major (row i = hit i).  ep->lead is ignored. */
int am_needle_estimate_rows(int device, const float* rows, size_t n, const am_estimate_params* ep,
                            float* est, float* dev, uint32_t* count);
/* The hits in haystacks resident on `device` (an archive in device memory; one hit per file, or many): nothing but the
 * hit table travels up, the rows are gathered by the kernel.  hits, lens, est, dev, count: host memory. */
int am_needle_estimate_device(int device, const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                              int sample_format, const am_est_hit* hits, size_t n, const am_estimate_params* ep,
                              float* est, float* dev, uint32_t* count);

/* ---- per-hit drift scoring: a hit's clock drift and its corrected NCC ------------ */
/* The reference has no such stage.  Every per-hit family above assumes that an occurrence runs on the needle's clock;
 * two digitisation chains differ by tens to hundreds of ppm, a tape or a playout machine by more, and the one NCC of
 * am_hit_scores collapses long before am_hit_segments runs off its +-16 lags.  For each hit this family correlates the
 * needle, resampled to each drift of a grid, against the haystack at the lags -R .. R and reports the best cell.
 *
 * The interpolator.  One table h[p][k], p = 0 .. AM_WARP_PHASES - 1 (4096), k = 0 .. AM_WARP_TAPS - 1 (32), computed once
 *   on the host in f64 and stored as f32:  h[p][k] = v[k] / sum_k v[k],  v[k] = sinc(x) I0(8 sqrt(1 - (x / 16)^2)) / I0(8),
 *   x = k - 15 - p / 4096, sinc(x) = sin(pi x) / (pi x).  Row p = 0 is exactly the delta (h[0][15] = 1, zeros elsewhere),
 *   by definition and not by computation; where a result is taken at p = 0 it is the sample itself, no sum is formed.
 *   Measured on the CPU, for sines: the error is 1.1e-4 of the amplitude up to 0.4 of the sample rate, 3.8e-4 with the
 *   phase rounding included; above 0.45 of the sample rate it falls off.  am_warp_table returns the table (pure host
 *   function; out: AM_WARP_PHASES x AM_WARP_TAPS floats, the same bits on every call).
 * The warped needle.  For a drift d in ppm: inc = llround(2^32 / (1 + d 1e-6)) in f64 on the host, its length
 *   S_d = floor((S - 1) 2^32 / inc) + 1, and for j in [0, S_d):  u = j inc + 2^19 (u64), m = u >> 32, p = (u >> 20) & 4095,
 *     n_d[j] = fl32( sum_{k = 0 .. 31} (double)h[p][k] (double)n~[m - 15 + k] ),
 *   n~ the needle with 0 outside [0, S), the sum in f64 in the order k = 0, 1, ..., rounded to f32 once (a product of two
 *   f32 values is exact in f64: fused and unfused multiply-adds give the same bits).  d = 0 gives n_0 = n bit for bit,
 *   S_0 = S.  The sign is that of am_segment_summary.drift_ppm: positive d, the occurrence is longer than the needle and
 *   its lag grows along the needle.
 * The grid.  K = steps, Q = 2 K + 1 drifts d_q = centre_ppm + max_ppm (q - K) / K (K = 0: the one drift d_0 = centre_ppm),
 *   lags l = -R .. R.  K <= AM_WARP_MAX_STEPS, R <= AM_SEG_MAX_RADIUS, |centre_ppm| + max_ppm <= AM_WARP_MAX_PPM,
 *   max_ppm >= 0, and max_ppm > 0 when K > 0.
 * Cells.  t = peak.start, x the haystack (the bit-exact down-mix for AM_FMT_S16_STEREO), 0 outside [0, len), in f64:
 *     c(q,l) = sum_{j < S_q} x[t + l + j] n_q[j],   E_w(q,l) = sum_{j < S_q} x[t + l + j]^2,   E_n(q) = sum_j n_q[j]^2,
 *     ncc(q,l) = c / sqrt(E_n E_w),  0 when E_n(q) = 0, E_w = 0 or E_w < E_n 10^(-score_norm_floor_db / 10).
 *   The sums run in one fixed order that depends on S_q alone (slices of 4096 samples, the partials added in slice order).
 * The record of a hit:
 *   best cell  (q*, l*) = the cell with the largest ncc; ties go to the smaller |q - K|, then the smaller q, then the
 *              smaller |l|, then the negative l.
 *   drift_ppm  d_q* + e max_ppm / K, e the vertex of the parabola through ncc(q* - 1, l*), ncc(q*, l*), ncc(q* + 1, l*),
 *              clamped to +-0.5.  e = 0 and flag AM_HIT_DRIFT_UNREFINED when K = 0, when q* is 0 or 2 K (widen or move the
 *              grid) or when there is no maximum (a - 2b + c >= 0).
 *   lag        l* + the vertex through c(q*, l* - 1), c(q*, l*), c(q*, l* + 1), as am_hit_segments refines a lag;
 *              AM_HIT_UNREFINED when R = 0, |l*| = R or there is no maximum.
 *   ncc, gain, level_db   at (q*, l*): ncc(q*, l*) (AM_HIT_BELOW_FLOOR by the floor rule), c / E_n, 10 log10(E_w / E_n)
 *              (-inf for E_w = 0).
 *   ncc_centre ncc(K, 0): the value at the call's centre drift and lag 0; with centre_ppm = 0, the NCC of am_hit_scores.
 *   length     S_q*: the occurrence's length in haystack samples.
 *   flags      AM_HIT_NONFINITE: a needle sample, or a haystack sample in [t - R, t + R + max_q S_q) inside [0, len), is not
 *              finite; drift_ppm = centre_ppm, lag = 0, the four floats NaN, length = S, no other flag.
 *              AM_HIT_EMPTY_SEGMENT (the flag of am_hit_segments, reused): E_n(q*) = 0 -- a needle of zeros, every cell 0,
 *              q* = K and l* = 0 by the tie rule; drift_ppm = d_q*, lag = 0, ncc = gain = 0, level_db = +inf for
 *              E_w(q*, l*) > 0 and NaN for 0, no other flag.
 * A hit's record depends on the needle, the samples it reads, the parameters and the floor only: the three forms below
 * agree bit for bit.  Precondition: peak.start + S <= len; a warped needle longer than what is left reads zeros.  The
 * host form stages [t - R, t + R + max_q S_q) of each hit only, clipped and merged.  The cost is proportional to
 * hits x Q x (lags of the kernel) x S, not to the haystack; a large call runs its hits in rounds of bounded scratch memory.
 * Measured on an MI355X (64 hits of a 10 s needle at 44.1 kHz in a resident 1 h haystack, +-400 ppm): 35.0 us per hit with
 * K = 8, R = 4 (Q = 17) and 409 us per hit with K = 32, R = 16 (Q = 65), beside 2.03 us for am_hit_segments with m = 8, R = 4
 * on the same hits; the kernels take 0.999 and 1.002 of Q am_hit_segments calls with m = 1 at the same R
 * (tools/hit_warp_bench.py, profiles/r19/).
 * AM_ERR_INVALID_ARG, naming the hit (and pair) or the field: an unknown sample format; wp's steps > AM_WARP_MAX_STEPS,
 * radius > AM_SEG_MAX_RADIUS, max_ppm < 0 or not finite, max_ppm = 0 with steps > 0, |centre_ppm| + max_ppm >
 * AM_WARP_MAX_PPM (the parameters are checked first, whatever n is); a null pointer with n > 0; peak.start + S > len; a
 * haystack on another device.  n = 0 returns AM_OK and launches nothing. */
enum { AM_HIT_DRIFT_UNREFINED = 256 };
#define AM_WARP_PHASES    4096
#define AM_WARP_TAPS      32
#define AM_WARP_MAX_STEPS 32
#define AM_WARP_MAX_PPM   50000
typedef struct am_warp_params {
    double centre_ppm;   /* the middle of the drift grid */
    double max_ppm;      /* its half width: drifts centre_ppm - max_ppm .. centre_ppm + max_ppm */
    uint32_t steps;      /* K, 0 .. AM_WARP_MAX_STEPS: 2 K + 1 drifts */
    uint32_t radius;     /* R, 0 .. AM_SEG_MAX_RADIUS: lags -R .. R */
} am_warp_params;        /* 24 bytes, no padding */
typedef struct am_warp_hit {
    double drift_ppm;    /* the refined drift of the occurrence against the needle, ppm */
    double lag;          /* l* + vertex: where the warped needle fits best, samples relative to the hit's start */
    float ncc;           /* at the best cell */
    float gain;          /* c / E_n there */
    float level_db;      /* 10 log10(E_w / E_n) there */
    float ncc_centre;    /* ncc(K, 0): before the correction */
    uint32_t length;     /* S_q*: the occurrence's length in haystack samples */
    uint32_t flags;      /* AM_HIT_* */
} am_warp_hit;           /* 40 bytes, no padding */
int am_warp_table(float* out /* AM_WARP_PHASES x AM_WARP_TAPS */);
int am_hit_warp_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                       const am_peak* peaks, size_t n, const am_warp_params* wp, am_warp_hit* out);
int am_hit_warp(const am_needle* h, const void* haystack, size_t len, int sample_format,
                const am_peak* peaks, size_t n, const am_warp_params* wp, am_warp_hit* out);
/* pair (k, j) = haystack k against needle j, slots as in am_hit_scores_batch_device; untouched slots stay untouched */
int am_hit_warp_batch_device(const am_needle* const* needles, size_t n_needles,
                             const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                             const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                             const am_warp_params* wp, am_warp_hit* out);
/* Rows on the needle's clock (pure host function, no device): am_hit_window for an occurrence at `start` whose refined
 * lag and drift am_hit_warp reported.  Row element n (0 <= n < length) sits at needle index i = n - lead; its position in
 * the haystack is u = (start << 32) + llround(lag 2^32) + i inc' + 2^19, inc' = llround(2^32 (1 + drift_ppm 1e-6)), in
 * signed 128-bit arithmetic; m = u >> 32 (floor), p = (u >> 20) & 4095, and
 *   v = fl32( fl32( sum_k (double)h[p][k] (double)x[m - 15 + k] ) * scale ),  the sum over the taps with h[p][k] != 0 in the
 *   order k = 0, 1, ... (p = 0: the sample x[m] itself).
 * The element is ABSENT (NaN) when a tap with h[p][k] != 0 would read outside [0, len) or a non-finite sample, or when the
 * product is not finite.  lag = 0 and drift_ppm = 0 give am_hit_window's row bit for bit.  AM_ERR_INVALID_ARG: as
 * am_hit_window; lag not finite or |lag| >= 2^30; |drift_ppm| > AM_WARP_MAX_PPM or not finite; start, lead, length >= 2^62. */
int am_hit_window_warped(const void* haystack, size_t len, int sample_format, uint64_t start, float scale,
                         double lag, double drift_ppm, uint64_t lead, uint64_t length, float* row);

/* ---- per-hit channel estimation: the filter a hit went through ------------------- */
/* The reference has no such stage (it reports one offset and one height per hit, matcher/mod.rs:110-125).  A jingle played
 * through another chain -- an EQ, a codec's pre-echo, a short echo, a sub-sample delay -- scores a low broadband NCC, and
 * the families above can only say that it is low.  This family estimates, per hit, the short filter that turns the needle
 * into what the recording holds, and reports how well the filtered needle explains the span.
 *
 * For a hit with t = peak.start: n[0 .. S) the handle's whole needle, n~ the needle with 0 outside [0, S), x the haystack
 * (f32 mono, or the bit-exact down-mix for AM_FMT_S16_STEREO), 0 outside [0, len), P = cp->radius, everything in f64 (a
 * product of two f32 values is exact there):
 *     c[l] = sum_{i<S} x[t + l + i] n[i],        l = -P .. P    (the cross-correlation around the hit)
 *     r[k] = sum_{i=k}^{S-1} n[i] n[i - k],      k = 0 .. 2P    (the needle's autocorrelation)
 *     E_n = r[0],   E_w = sum_{i<S} x[t + i]^2,   E_x = sum_{u=-P}^{S+P-1} x[t + u]^2
 *   Order of the sums.  The needle is cut into slices of 4096 samples from its start.  Within a slice, work item w of 256
 *   adds the products of its 16 consecutive needle samples 16 w .. 16 w + 15 in ascending order; the 256 values are added
 *   by a butterfly over each wave of 64 (distances 32, 16, .. 1), then the four waves in order; the slices are added in
 *   slice order.  E_w adds the squares the same way.  E_x adds, per work item, behind its 16 squares of [0, S): in slice 0
 *   the square of x[t - P + w] (w < P, the head), then in the last slice the square of x[t + S + w] (w < P, the tail).
 *   r is summed like c, with the needle in the place of x; it is computed once per distinct needle of a call.
 * Taps.  h[-P .. P] is the least-squares filter with x[t + u] ~ sum_l h[l] n~[u - l] over all u (the autocorrelation
 *   method): T h = c, T[a][b] = r[|a - b|] with the diagonal multiplied by 1 + 10^(-noise_db / 10) (the white-noise
 *   correction of am_whiten_taps; noise_db in [0, 200]).  T is symmetric Toeplitz; it is solved on the host by the Levinson
 *   recursion for a general right-hand side in f64, in one fixed order (am_channel_solve).  taps[l + P] = fl32(h[l]),
 *   rounded once.  P = 0: h[0] = c[0] / (r[0] (1 + lambda)).
 * The record, from the unrounded h, with q = h^T R h, R[a][b] = r[|a - b|] (uncorrected), h.c = sum_l h[l] c[l]:
 *   ncc          c[0] / sqrt(E_n E_w); 0 with AM_HIT_BELOW_FLOOR by the floor rule of am_hit_scores.
 *   ncc_eq       (h . c) / sqrt(E_x q): the NCC of the span against the filtered needle, in [-1, 1].  0 with
 *                AM_HIT_BELOW_FLOOR when E_x = 0, when q <= 0 or when E_x < E_n 10^(-score_norm_floor_db / 10).
 *   gain_db      10 log10(q / E_n), the channel's energy gain; -inf for q <= 0.
 *   residual_db  10 log10(max(E_x - 2 h.c + q, 0) / E_x): the share of the span the filtered needle does not explain;
 *                -inf when the numerator is 0, NaN when E_x = 0.
 *   main_tap     the l with the largest |h[l]|; ties go to the smaller |l|, then to the negative l.
 *   main_share   h[main_tap]^2 / sum_l h[l]^2: 1 for a pure gain and delay; 0 if all taps are 0.
 *   flags        AM_HIT_NONFINITE: a needle sample, or a sample of x[t - P, t + S + P) inside [0, len), is not finite; the
 *                five floats and all taps are NaN, main_tap = 0, no other flag.
 *                AM_HIT_EMPTY_SEGMENT (reused): E_n = 0; the taps are 0, ncc = ncc_eq = 0, main_tap = 0, main_share = 0,
 *                gain_db NaN, residual_db 0 for E_x > 0 and NaN for E_x = 0, no other flag.
 *                AM_HIT_ILL_CONDITIONED: the recursion met a prediction error <= 0, a reflection coefficient with
 *                |k| >= 1, or a value that is not finite; the taps fall back to the plain gain, h[0] = c[0] / r[0], the
 *                rest 0, and the record is computed from that.
 * A hit's record and taps depend on the needle, the samples in [t - P, t + S + P), P, noise_db and the floor only: the three
 * forms agree bit for bit, whatever else the call holds.  The host form stages [t - P, t + S + P) of each hit only, clipped
 * and merged.  The cost is proportional to hits x (2P + 1 rounded up to 32) x S; a large call runs its hits in rounds of
 * bounded scratch memory.  out[i] and taps[i (2P+1) ..] belong to peaks[i]; taps is host memory.
 * Measured on an MI355X (64 hits of a 10 s needle at 44.1 kHz in a resident 1 h haystack): 8.9 us per hit with P = 16 and
 * 92.9 us per hit with P = 128, of which the kernels take 6.9 and 30.3 us and the host's solve the rest; the kernels at
 * P = 128 take 0.61 of the eight am_hit_segments calls (m = 1, R = 16) that cover the same 257 lags
 * (tools/hit_channel_bench.py, profiles/r20/).
 * AM_ERR_INVALID_ARG, naming the hit (and pair) or the field: cp's radius > AM_CHAN_MAX_RADIUS, reserved != 0, noise_db
 * outside [0, 200] or not finite, an unknown sample format (these are checked first, whatever n is); a null pointer with
 * n > 0 (taps included); peak.start + S > len; a haystack on another device.  n = 0 returns AM_OK and launches nothing. */
enum { AM_HIT_ILL_CONDITIONED = 512 };
#define AM_CHAN_MAX_RADIUS 128
typedef struct am_channel_params {
    uint32_t radius;     /* P, 0 .. AM_CHAN_MAX_RADIUS: taps -P .. P */
    uint32_t reserved;   /* 0 */
    double noise_db;     /* the white-noise correction, 0 .. 200 (60 is a good choice) */
} am_channel_params;     /* 16 bytes, no padding */
typedef struct am_channel_hit {
    float ncc;           /* the plain NCC of the window */
    float ncc_eq;        /* the NCC of the span against the filtered needle */
    float gain_db;       /* the channel's energy gain */
    float residual_db;   /* the unexplained share of the span */
    int32_t main_tap;    /* the lag of the largest tap */
    float main_share;    /* its share of the taps' energy */
    uint32_t flags;      /* AM_HIT_* */
    uint32_t reserved;   /* 0 */
} am_channel_hit;        /* 32 bytes, no padding */
int am_hit_channel_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                          const am_peak* peaks, size_t n, const am_channel_params* cp,
                          am_channel_hit* out, float* taps /* n x (2P+1), host */);
int am_hit_channel(const am_needle* h, const void* haystack, size_t len, int sample_format,
                   const am_peak* peaks, size_t n, const am_channel_params* cp,
                   am_channel_hit* out, float* taps /* n x (2P+1) */);
/* pair (k, j) = haystack k against needle j, slots as in am_hit_scores_batch_device; the taps of slot q of pair p at
 * (p cap_per_pair + q)(2P+1); untouched slots stay untouched */
int am_hit_channel_batch_device(const am_needle* const* needles, size_t n_needles,
                                const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                const am_channel_params* cp, am_channel_hit* out, float* taps);
/* Pure host function (no device): the solve above.  r: 2P+1 doubles r[0 .. 2P], c: 2P+1 doubles c[-P .. P] (c[l] at l + P),
 * h: 2P+1 doubles (h[l] at l + P).  The recursion, for the matrix t[0] = r[0] (1 + lambda), t[k] = r[k], in f64, every sum
 * in ascending index order: a = {1}, err = t[0], h[0] = c[0] / t[0]; for m = 1 .. 2P: k = -(t[m] + sum_{i=1}^{m-1} a[i]
 * t[m-i]) / err; a'[i] = a[i] + k a[m-i] (0 < i < m), a'[m] = k; err = err (1 - k^2); d = (c[m] - sum_{i<m} t[m-i] h[i])
 * / err; h[i] += d a'[m-i] (i <= m).  *ill != 0 when it fell back to the plain gain (h[P] = c[P] / r[0], the rest 0), as
 * AM_HIT_ILL_CONDITIONED says; with r[0] <= 0 every h is 0 and *ill != 0.
 * AM_ERR_INVALID_ARG: a null pointer, radius > AM_CHAN_MAX_RADIUS, noise_db out of range, a non-finite r[k] or c[l]. */
int am_channel_solve(const double* r, const double* c, uint32_t radius, double noise_db, double* h, int* ill);
/* Pure host function (no device): the filtered needle under a hit and what is left of the span.  For u in [0, S + 2P),
 * haystack element e = start - P + u:
 *   model[u] = fl32( sum_{l=-P..P} (double)taps[l+P] (double)n[u - P - l] ), over the l with u - P - l in [0, S), in f64,
 *              in the order l = -P .. P, rounded once;
 *   resid[u] = x[e] - model[u] (one f32 subtraction); NaN where e lies outside [0, len) or x[e] is not finite.
 * needle: S f32 samples in host memory; model or resid may be null.  What lies over the hit -- the voice-over, the start of
 * the next item -- is resid; x - gain n leaves most of an equalised jingle in place.
 * AM_ERR_INVALID_ARG: an unknown sample format, a null pointer (haystack: with len > 0), s = 0, radius >
 * AM_CHAN_MAX_RADIUS, start or s >= 2^62. */
int am_hit_residual(const void* haystack, size_t len, int sample_format, uint64_t start, const float* needle, size_t s,
                    const float* taps, uint32_t radius, float* model, float* resid);

/* ---- per-hit stereo image: channel, polarity and delay of a hit -------------------- */
/* Every entry point that takes AM_FMT_S16_STEREO first collapses a frame to (l + r) * 0.5 * (1/65535), as the reference
 * does (mp3_reader.rs:28-37), and everything behind that sees the down-mix only.  A jingle on one channel comes out at half
 * gain, an insert that sits polarity-inverted in the two channels cancels, and a hit that is found cannot be placed between
 * the channels.  This family reads the i16 frames themselves.  AM_FMT_S16_STEREO only.
 *
 * For a hit with t = peak.start, everything in f64: k = (double)(2 kappa), kappa the f32 constant 0.5f * (1.0f / 65535.0f)
 * of the down-mix; l[u] = k L[u], r[u] = k R[u] for the i16 values of frame u, 0 outside [0, len); n[0 .. S) the handle's
 * needle, E_n the handle's energy, R = sp->radius:
 *     c_L(lam) = sum_{i<S} l[t + lam + i] n[i],   c_R(lam) likewise,   lam = -R .. R
 *     E_L = sum_i l[t+i]^2,  E_R = sum_i r[t+i]^2,  E_LR = sum_i l[t+i] r[t+i]          (lag 0)
 *     E_M = (E_L + 2 E_LR + E_R) / 4,   E_D = (E_L - 2 E_LR + E_R) / 4                   (mid = (l+r)/2, side = (l-r)/2)
 *   How they are evaluated.  c_ch(lam) = k C, C = sum_i L[t + lam + i] n[i] with exact products (an i16 times an f32
 *   value), summed in the order of am_hit_channel: the needle in slices of 4096 samples, work item w of 256 its 16
 *   consecutive samples ascending, a butterfly over each wave of 64 (distances 32 .. 1), the four waves in order, the
 *   slices in order.  The energies are exact: 64-bit integer sums S_LL, S_RR, S_LR of the i16 products, E = (double)S (k k);
 *   E_M and E_D from the integers S_LL +- 2 S_LR + S_RR, times (k k), times 0.25.
 * The record:
 *   lag_left, lag_right    per channel the lag lam* with the largest |c_ch(lam)|; ties go to the smaller |lam|, then to the
 *                          negative lag; plus the vertex of the parabola through |c| at lam* - 1, lam*, lam* + 1, clamped to
 *                          +-0.5: the rule of am_hit_segments applied to |c|, so that an inverted channel gets its true
 *                          lag.  lag_left - lag_right is the inter-channel delay.
 *   ncc_left, ncc_right    c_ch(0) / sqrt(E_n E_ch); the sign is the polarity.
 *   ncc_mid, ncc_side      (c_L(0) + c_R(0)) / 2 / sqrt(E_n E_M) and (c_L(0) - c_R(0)) / 2 / sqrt(E_n E_D).  ncc_mid is
 *                          the NCC of am_hit_scores up to the down-mix's f32 rounding.
 *   ncc_best               the largest NCC any fixed mix a l + b r reaches: sqrt(max(q, 0) / E_n), q = (c_L^2 E_R - 2 c_L c_R
 *                          E_LR + c_R^2 E_L) / det, det = E_L E_R - E_LR^2, the c at lag 0.
 *   gain_left, gain_right  c_ch(0) / E_n.
 *   mix_left, mix_right    the mix that reaches ncc_best: (c_L E_R - c_R E_LR) / det and (c_R E_L - c_L E_LR) / det.
 *   flags                  AM_HIT_LEFT_SILENT, AM_HIT_RIGHT_SILENT, AM_HIT_SIDE_SILENT, and for the mid the existing
 *                          AM_HIT_BELOW_FLOOR: the energy (E_L, E_R, E_D, E_M) is 0 or below E_n 10^(-score_norm_floor_db /
 *                          10), the process option am_hit_scores reads; that NCC is then 0.
 *                          AM_HIT_LEFT_UNREFINED, AM_HIT_RIGHT_UNREFINED: under the conditions of am_hit_segments (R = 0,
 *                          |lam*| = R, or no maximum) the channel's vertex term is 0.
 *                          AM_HIT_COLLINEAR: det <= AM_STEREO_MIN_INDEPENDENCE E_L E_R, or a channel is silent.  ncc_best
 *                          and the mix then come from the channel with the larger energy alone (left wins a tie):
 *                          |c_ch(0)| / sqrt(E_n E_ch) and c_ch(0) / E_ch, the other mix weight 0; both channels silent:
 *                          ncc_best = mix = 0.
 *                          AM_HIT_NONFINITE: a needle sample is not finite; every float is NaN, both lags are 0, no other
 *                          flag.  AM_HIT_EMPTY_SEGMENT (reused): E_n = 0, a needle of zeros; every float and both lags
 *                          are 0, no other flag.
 * A hit's record depends on the needle, the frames in [t - R, t + S + R), R and the floor only: the three forms agree bit
 * for bit, whatever else the call holds.  The host form stages [t - R, t + S + R) of each hit only, clipped and merged.
 * The cost is proportional to hits x S x 2 (2R + 1), the radius rounded up to 1, 4 or 16.
 * Measured on an MI355X (64 hits of a 10 s needle at 44.1 kHz in a resident 1 h haystack, R = 8): 7.0 us per hit, of which
 * the kernels take 6.5; the two am_hit_segments_device calls (m = 1, R = 8) on de-interleaved f32 copies of L and R that
 * give the same lags take 13.3 and 12.4 (tools/hit_stereo_bench.py, profiles/r21/).
 * AM_ERR_INVALID_ARG, naming the hit (and pair) or the field: AM_FMT_F32_MONO ("am_hit_stereo: needs interleaved i16 stereo
 * frames"), radius > AM_STEREO_MAX_RADIUS, reserved != 0, a null pointer with n > 0, peak.start + S > len, a haystack on
 * another device.  n = 0 returns AM_OK and launches nothing.
 * The record type is am_stereo_hit: a typedef am_hit_stereo cannot stand beside the function of that name. */
enum {
    AM_HIT_LEFT_SILENT = 1024,
    AM_HIT_RIGHT_SILENT = 2048,
    AM_HIT_SIDE_SILENT = 4096,
    AM_HIT_COLLINEAR = 8192,
    AM_HIT_LEFT_UNREFINED = 16384,
    AM_HIT_RIGHT_UNREFINED = 32768
};
#define AM_STEREO_MAX_RADIUS 16
#define AM_STEREO_MIN_INDEPENDENCE 1e-6
typedef struct am_stereo_params {
    uint32_t radius;     /* R, 0 .. AM_STEREO_MAX_RADIUS: lags -R .. R */
    uint32_t reserved;   /* 0 */
} am_stereo_params;      /* 8 bytes */
typedef struct am_stereo_hit {
    double lag_left, lag_right;
    float ncc_left, ncc_right;
    float ncc_mid, ncc_side;
    float ncc_best;
    float gain_left, gain_right;
    float mix_left, mix_right;
    uint32_t flags;      /* AM_HIT_* */
} am_stereo_hit;         /* 56 bytes, no padding */
int am_hit_stereo_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_peak* peaks, size_t n, const am_stereo_params* sp, am_stereo_hit* out);
int am_hit_stereo(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_peak* peaks, size_t n, const am_stereo_params* sp, am_stereo_hit* out);
/* pair (k, j) = haystack k against needle j, slots as in am_hit_scores_batch_device; untouched slots stay untouched */
int am_hit_stereo_batch_device(const am_needle* const* needles, size_t n_needles,
                               const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                               const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                               const am_stereo_params* sp, am_stereo_hit* out);
/* Pure host function (no device): where one hit sits between the channels, from its record.
 *   balance_db       20 log10(|gain_left| / |gain_right|); +-inf when one gain is 0, NaN when both are.
 *   delay            lag_left - lag_right; NaN unless |ncc_left| >= min_ncc and |ncc_right| >= min_ncc.
 *   downmix_loss_db  20 log10(ncc_best / |ncc_mid|): what matching the down-mix cost; +inf when ncc_mid is 0.
 *   image, by the first rule that applies:
 *     1. ncc_best < min_ncc (or not a number)                          AM_IMAGE_ABSENT
 *     2. of |ncc_left|, |ncc_right| only the left reaches min_ncc      AM_IMAGE_LEFT; only the right: AM_IMAGE_RIGHT
 *     3. both reach it, with opposite signs                            AM_IMAGE_INVERTED
 *     4. both reach it, same sign, |balance_db| <= 3                   AM_IMAGE_CENTRE
 *     5. anything else                                                 AM_IMAGE_PANNED
 * AM_ERR_INVALID_ARG: a null pointer. */
enum { AM_IMAGE_ABSENT = 0, AM_IMAGE_CENTRE = 1, AM_IMAGE_LEFT = 2, AM_IMAGE_RIGHT = 3, AM_IMAGE_PANNED = 4, AM_IMAGE_INVERTED = 5 };
typedef struct am_stereo_summary {
    double balance_db;
    double delay;
    double downmix_loss_db;
    int32_t image;       /* AM_IMAGE_* */
    uint32_t reserved;   /* 0 */
} am_stereo_summary;     /* 32 bytes */
int am_hit_stereo_summary(const am_stereo_hit* rec, float min_ncc, am_stereo_summary* out);

/* ---- device memory plumbing (for hosts without their own HIP allocator) -- */
int am_device_malloc(int device, size_t bytes, void** out);
int am_device_free(int device, void* p);
int am_memcpy_h2d(int device, void* d_dst, const void* src, size_t bytes);
int am_memcpy_d2h(int device, void* dst, const void* d_src, size_t bytes);
int am_device_synchronize(int device);

/* Pinned host memory for the buffers handed to am_match, am_match_stream_push and am_pool_match_* (the reference
 * collects the decoder's output in ordinary Vecs, mp3_reader.rs:13-41, matcher/mod.rs:32; nothing to pin there).
 * The copy engines read pinned memory directly: no bounce buffer inside the runtime and no page faults, so the
 * copier threads of a pool feed their devices side by side ("feeding the GPUs").  Either
 * allocate the decoder's output buffer here, or register an existing allocation for the time it is in use.
 * Portable across devices. */
int am_host_alloc(size_t bytes, void** out);
int am_host_free(void* p);
int am_host_register(void* p, size_t bytes);
int am_host_unregister(void* p);

/* ---- synthetic signals for tests / benches -------- */
/* d_out[k] = uniform(seed, stream, first + k) * amp, 24-bit exact in [-amp, amp) */
int am_synth_uniform_device(int device, float* d_out, uint32_t seed, uint32_t stream,
                            uint64_t first, size_t n, float amp);
/* d_dst[i] += gain * d_src[i]  (plants a needle into a haystack) */
int am_axpy_device(int device, float* d_dst, const float* d_src, size_t n, float gain);

/* the same signal as interleaved i16 stereo frames: left = stream,
 * right = stream + 5000, each value rint(uniform * amp * 32767), saturated */
int am_synth_pcm16_stereo_device(int device, int16_t* d_out, uint32_t seed, uint32_t stream,
                                 uint64_t first, size_t frames, float amp);
/* d_dst[i] = saturate(d_dst[i] + d_src[i]) over 2 * frames interleaved i16 values (plants a needle) */
int am_add_pcm16_device(int device, int16_t* d_dst, const int16_t* d_src, size_t frames);

/* ---- the haystack batch over every GPU of a node ----------------------------- */
/* matcher::run's per-file loop (matcher/mod.rs:42-87) sharded over devices: haystacks are
 * independent given the needle (audio_matcher.rs:114-131), so haystack k goes to pool slot
 * k mod n_dev -- no exchange step, no collective; results are gathered on the host.
 * am_shard_plan is that rule as a pure function (no device needed): shard `shard` of
 * `n_shards` owns items first, first + stride, ... (count of them). */
int am_shard_plan(size_t n_items, size_t n_shards, size_t shard, size_t* first, size_t* stride, size_t* count);

/* A pool = LibConvolve::new(sample_data) (audio_matcher.rs:289) replicated on each listed
 * device (needle + its spectrum per device, built locally).  devices == NULL: every
 * visible device, in ordinal order.  A device may be listed more than once (its slots then
 * share that device's queue). */
typedef struct am_pool am_pool;
int am_pool_create(const float* needle, size_t n, const int* devices, size_t n_dev, am_pool** out);
void am_pool_destroy(am_pool* pool);
int am_pool_size(const am_pool* pool, size_t* n_dev);
/* slot's device ordinal and its needle handle (borrowed: valid until am_pool_destroy) */
int am_pool_slot(const am_pool* pool, size_t slot, int* device, const am_needle** needle);
/* The whole loop on HOST buffers: one submit thread per slot takes its haystacks in order;
 * a second thread per slot copies haystack i+1 into the other half of a two-slot HBM ring
 * while haystack i is matched, so the link and the kernels overlap.  out / n_out are laid
 * out as in am_match_batch_device (cap_per_hay slots per haystack); every submit thread
 * writes only its own haystacks' slots.  Returns the worst status over all haystacks. */
int am_pool_match_batch(am_pool* pool, const float* const* haystacks, const size_t* lens, size_t n_hay,
                        const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out);
/* Same with resident haystacks: d_haystacks[k] must live on the device of slot k mod n_dev (checked with
 * hipPointerGetAttributes: AM_ERR_INVALID_ARG names the haystack that sits on another device). */
int am_pool_match_batch_device(am_pool* pool, const float* const* d_haystacks, const size_t* lens, size_t n_hay,
                               const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out);

/* The same two loops on interleaved 16-bit stereo PCM (what the reference decodes every file
 * to, mp3_reader.rs:26-37); `frames` per haystack. */
int am_pool_match_batch_pcm16(am_pool* pool, const int16_t* const* interleaved, const size_t* frames, size_t n_hay,
                              const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out);
int am_pool_match_batch_pcm16_device(am_pool* pool, const int16_t* const* d_interleaved, const size_t* frames, size_t n_hay,
                                     const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out);
/* A pool of SEVERAL equal-length needles (BASELINE config 4 over every GPU of the node): each
 * needle = one LibConvolve::new (audio_matcher.rs:289), replicated per device.  The single-needle
 * calls above refuse such a pool; am_pool_match_multi_batch* run am_match_multi_batch_device per
 * slot on that slot's shard (haystack k on slot k mod n_dev), host buffers through the same
 * two-slot copy ring.  out / n_out: cap_per_pair slots per (haystack, needle) pair at index
 * k * n_needles + j, k the index in the caller's batch. */
int am_pool_create_multi(const float* const* needles, size_t n_needles, size_t n, const int* devices, size_t n_dev, am_pool** out);
int am_pool_needle_count(const am_pool* pool, size_t* n_needles);
int am_pool_match_multi_batch(am_pool* pool, const void* const* haystacks, const size_t* lens, size_t n_hay, int sample_format,
                              const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out);
int am_pool_match_multi_batch_device(am_pool* pool, const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                     const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out);

/* ---- ONE long haystack over several GPUs ------------------------------------------- */
/* calc_chunks fans the windows of ONE haystack out over its workers (iter.par_bridge().map(..),
 * audio_matcher.rs:104-131) and sorts and filters the union afterwards (:132-140).  The same split over
 * devices ("a single very long haystack: shard by chunk ranges with an S-1 halo"): part i of
 * n_parts owns a contiguous range of windows, its samples reach to the end of its last window (chunk +
 * overlap, which contains the S - 1 halo), its windows are matched as on one device and ONE merge runs
 * over all parts, so that a peak next to a cut meets its neighbour from the other part.  The result
 * equals am_match on the whole buffer: offsets and plateau ends identical, heights and prominences to
 * f32 rounding (the overlap-save blocks of a part start at the part, not at sample 0).
 *
 * am_long_plan is the split as a pure function (no device needed): windows [first_window, first_window +
 * n_windows) and samples [first_sample, first_sample + n_samples) of part `part`; n_windows may be 0. */
int am_long_plan(size_t len, size_t needle_len, const am_match_params* p, size_t n_parts, size_t part,
                 size_t* first_window, size_t* n_windows, size_t* first_sample, size_t* n_samples);
/* One part: calc_chunks up to audio_matcher.rs:131 (windowing, correlation, find_peaks, offset restore) on
 * the first n_windows windows of the resident samples d_part[0 .. n_samples); peaks come back UNMERGED, in
 * window order, positions shifted by first_sample.  For hosts that run one process per GPU: every rank
 * matches its part, the ranks' lists are concatenated in part order and am_merge_peaks finishes. */
int am_match_part_device(const am_needle* h, const void* d_part, size_t n_samples, int sample_format, const am_match_params* p,
                         size_t n_windows, uint64_t first_sample, am_peak* out, size_t cap, size_t* n_out);
/* sort by position.start + filter_surrounding(!is_overshadowed) (audio_matcher.rs:132-160) on a host list */
int am_merge_peaks(const am_match_params* p, const am_peak* peaks, size_t n, am_peak* out, size_t cap, size_t* n_out);
/* The three steps over the slots of a single-needle pool, one thread per slot.  Host buffer: every slot
 * copies its own sample range over its own link (the copies of n devices run side by side) and matches
 * it.  _device: d_parts[i] = the samples of part i (am_long_plan with n_parts = the pool's size), resident
 * on the device of slot i.  sample_format: AM_FMT_*; len in samples / frames.  Progress: haystack index 0,
 * chunk indices of the whole haystack. */
int am_pool_match_long(am_pool* pool, const void* haystack, size_t len, int sample_format, const am_match_params* p,
                       am_peak* out, size_t cap, size_t* n_out);
int am_pool_match_long_device(am_pool* pool, const void* const* d_parts, size_t len, int sample_format, const am_match_params* p,
                              am_peak* out, size_t cap, size_t* n_out);

/* ---- live monitoring: final hits while the audio arrives ----------------------------- */
/* The overshadow filter (is_overshadowed, audio_matcher.rs:143-160) looks at an element's two neighbours in start
 * order only, so a peak's fate is settled once its successor is known, or once no later peak can come within the
 * overshadow distance.  am_merge_ready is that rule as a pure host function.  Given the UNFILTERED peaks of a
 * recording sorted by start (stable, window order on ties) as am_merge_peaks sorts them, of which every peak with
 * start < horizon is present and none with start >= horizon is, *n_ready = the length of the longest prefix whose
 * fate under am_merge_peaks (kept or overshadowed) can no longer change, whatever peaks with start >= horizon are
 * still to come: every peak but the last, and the last too when its predecessor (option "surrounding_from" = 1: the
 * last peak kept) overshadows it or when a peak at `horizon` with +inf prominence could not.  ended != 0: nothing
 * more comes, *n_ready = n.  A list not sorted by start, or (ended == 0) a peak at or after horizon: AM_ERR_INVALID_ARG. */
int am_merge_ready(const am_match_params* p, const am_peak* sorted, size_t n, uint64_t horizon, int ended, size_t* n_ready);

/* A monitor watches an unbounded recording (a live feed) for n_needles >= 1 needles on ONE device, params[j] for
 * needle j (sr equal for all; chunk and overlap may differ), samples in sample_format (AM_FMT_F32_MONO or
 * AM_FMT_S16_STEREO).  The windows are those of calc_chunks (chunked(chunk + overlap, hop = chunk),
 * audio_matcher.rs:104; the lazy sample source of matcher/mod.rs:42-99): group g is windows [g G, g G + G),
 * G = group_windows (0 means 1), matched as one part (am_match_part_device: n_samples the group's span, first_sample
 * g G chunk) as soon as its last window's samples have arrived.  What am_monitor_poll and am_monitor_end return for
 * needle j, concatenated, equals am_merge_peaks over those parts bit for bit, for every way the samples are split
 * into pushes; offsets and plateau ends equal am_match on the whole recording, heights and prominences agree to f32
 * rounding (a part's overlap-save blocks start at the part).
 *
 * Latency: a peak is returned by the first poll after it is final under am_merge_ready with horizon g G chunk, g the
 * needle's first group not yet matched -- once the group holding its successor is matched, or the one that takes
 * the horizon the overshadow distance past it.  A returned peak is never revised.
 * Memory: the samples live in one device buffer of fixed size, 4 x (2 x the largest group span + 65536) bytes
 * (span = (G - 1) chunk + chunk + overlap); samples before the earliest horizon are dropped (a device-to-device copy
 * on the library's stream).  A push of any size is consumed in steps.
 * Options are read once, at am_monitor_begin (each needle with its handle's overrides): "half_pipeline",
 * "peak_filter_order", "distance_rule", "tail_window", "surrounding_from", "log_n", the non-finite redo path and
 * AM_SCALE_MY behave as for am_match_part_device.  "score_norm" is refused (AM_ERR_INVALID_ARG, "score_norm: not
 * supported by this entry point").  One producer per monitor; monitors of one device share its queue.
 *
 * push: n samples / frames from host memory; a piece is copied into a pinned staging slot and push returns without
 * waiting for the device unless the piece completes a group (which is then matched).  poll: the peaks that became
 * final since the last poll, of all needles, sorted by (start, needle); needle[i] (may be null) = the needle of
 * out[i].  end: end of input -- the remaining groups are matched (the windows at the end as make_segments cuts
 * them, option "tail_window") and every peak not yet returned comes back; after end, push is refused and end / poll
 * return what is left.  poll / end with cap too small: AM_ERR_CAPACITY, *n_out = the count, nothing is consumed. */
typedef struct am_monitor am_monitor;
int am_monitor_begin(const am_needle* const* needles, size_t n_needles, const am_match_params* params, int sample_format,
                     size_t group_windows, am_monitor** out);
int am_monitor_push(am_monitor* m, const void* samples, size_t n);
int am_monitor_poll(am_monitor* m, am_peak* out, uint32_t* needle, size_t cap, size_t* n_out);
int am_monitor_end(am_monitor* m, am_peak* out, uint32_t* needle, size_t cap, size_t* n_out);
typedef struct am_monitor_info {
    uint64_t received;        /* samples / frames pushed so far */
    uint64_t horizon;         /* every window before this sample has been matched (all needles) */
    uint64_t resident_bytes;  /* device bytes the monitor owns (its sample buffer); fixed at begin */
    uint64_t pending;         /* peaks found but not yet final */
} am_monitor_info;
int am_monitor_info_get(const am_monitor* m, am_monitor_info* info);
void am_monitor_destroy(am_monitor* m);

/* ---- progress hooks ---------------------------------------------------------- */
/* The two-stage progress callbacks of calc_chunks (audio_matcher.rs:102-117, 129:
 * f1 when a chunk is picked up, f2 when it is done).
 * Per haystack (aggregate): stage 0 with its chunk count when it is queued, stage 1 when
 * its peaks are back on the host.
 * Per chunk (the reference's granularity): all chunks of a haystack run in one set of
 * launches here, so stage 0 fires for chunks 0..n-1 in order when the haystack is queued
 * and stage 1 for chunks 0..n-1 in order when its results have landed; like the
 * reference's f1/f2, every chunk sees stage 0 before stage 1.
 * haystack_index is the index in the caller's batch (pool calls included; pool submit
 * threads call back concurrently).  Process-wide; a running call keeps the callbacks it
 * started with; pass NULL to clear. */
typedef void (*am_progress_fn)(void* user, size_t haystack_index, int stage, size_t n_chunks);
int am_set_progress_callback(am_progress_fn fn, void* user);
typedef void (*am_chunk_progress_fn)(void* user, size_t haystack_index, size_t chunk_index, size_t n_chunks, int stage);
int am_set_chunk_progress_callback(am_chunk_progress_fn fn, void* user);

/* ---- measurement hooks ---------------------------------------------------- */
/* When enabled every kernel launch of the pipeline on `device` is bracketed by
 * HIP events on the stream it is launched on.  am_profile_query returns the
 * summed elapsed time and launch count of kernels whose name matches `kernel`
 * exactly ("k1_cols_fwd", "k2_rows", "k3_cols_inv", "tile_stats",
 * "peaks", "other", "trace" -- the score-trace kernels --, "discover" -- the
 * kernels of needle discovery --, "envelope_frames", "envelope_prefix",
 * "envelope_correlate" -- the levels, the prefix sums and the correlation of
 * envelope matching; "envelope" adds the three --, "edges" -- the span, scan,
 * normalising and exact kernels of edge matching --, "mask" -- the kernels of
 * am_hit_mask* -- or "*" for all). */
int am_profile_enable(int device, int on);
int am_profile_reset(int device);
int am_profile_query(int device, const char* kernel, double* total_ms, uint64_t* launches);

/* Measurement hook, not part of the drop-in boundary: the two column kernels on `npairs` block pairs of synthetic
 * input, `iters` launches each, average launch time in ms.  wide = 0: the production 2^22-point plan (512 x 8192);
 * wide = 1: 2^23 points factored 512 x 16384, i.e. the same 512-row kernels on rows twice as long (no row kernel exists
 * for that factorisation yet; DESIGN.md 9.3 sizes it with this).  dense != 0: the inverse kernel writes every score. */
int am_debug_column_bench(int device, int wide, int npairs, int iters, int dense, double* k1_ms, double* k3_ms);

/* Process-wide option DEFAULTS.  A call reads them once on entry, so changing one never
 * affects a call that is already running.
 *   "log_n" (0 = auto), "pairs_per_group", "profile_mask": tuning / measurement knobs
 *   "profile_every" (n >= 1, default 1): with profiling on, bracket only every n-th launch of a kernel class with
 *       events (an event pair costs the stream about 8 us per kernel boundary; am_profile_query then reports the
 *       bracketed launches' time and count)
 *   "batch_overlap" (0/1, default 1): in am_match_batch_device pick the peaks of haystack k
 *       on a second stream beside the transforms of haystack k+1
 *   "needle_group" (1..8, default 8): how many needles of am_match_multi_device share
 *       one forward row transform of the haystack (1 = one row pass per needle)
 *   "half_pipeline" (0/1/2, BASELINE config 5; 0 = off, the default): 1 = the transform's work
 *       matrix travels through HBM in half precision, butterflies stay f32 (scores within about
 *       2e-5 on noise-like audio); 2 = the butterflies run in packed f16 as well (the row kernel and
 *       the forward column kernel whole, the first pass of the inverse column kernel; its
 *       second pass and the score scan stay f32; scores within about 1e-3).  Hit offsets are unaffected.  Meant for audio-level signals: full-scale input
 *       stays inside f16's range, inputs far above full scale may overflow it.
 *   "dense_scores" (0/1): write every raw score from the inverse pass (threshold -inf)
 *       instead of only the tiles that can matter to the peak pick; results are
 *       identical, this is the worst case of the sparse-score path for measurements.
 *   "tail_block" (0/1, default 1): two overlap-save blocks share one complex transform, so a haystack with an odd
 *       number of blocks pays a whole pair for its last, part-filled block.  1 = when the scores behind the last even
 *       block boundary fit one pair of the next smaller transform (half the points), they come from that: beside the
 *       main pass for a single haystack, several haystacks per launch in a batch.  Offsets are unaffected, scores agree
 *       to rounding (1e-6); a haystack's results do not depend on the batch it travels in.  Single-needle entry points
 *       (am_match*, am_pool_match_batch*, am_pool_match_long*, am_match_part_device) and the several-needle engine when
 *       every needle group holds at least two needles (the tail's forward pass once per haystack, its row and inverse
 *       passes once per group); not streaming ingest, not a forced "log_n".
 *   "host_pick_wait" (0/1, default 1): in a batch, the calling thread (not the stream) waits for the peak pick that
 *       last read a set of score buffers before it queues the next haystack into that set -- it runs far ahead of the
 *       GPU either way, and the main stream is spared a barrier packet per haystack (results are identical).
 *   "device_redo" (0/1, default 1): in a batch, chunks whose sparse-score certificate fails get their dense
 *       inverse pass on the device, beside the next haystack's transforms; 0 = the host path does it
 *       after the call's kernels (results are identical; for measurements).
 *   "k3_group" (0/1, default 1): in am_match_multi_*, the inverse passes (K3) of a needle group run as one launch
 *       (0: one launch per needle; results are identical, for measurements).
 *   "pick_group" (0/1, default 1): ... and so do the group's peak picks (0: four small launches per needle).
 *   "k2_mfma" (0/1, default 0, or the environment variable AM_K2_MFMA): with half_pipeline = 2, the row transform
 *       (K2) of the 8192-point rows runs on the matrix cores (v_mfma_f32_16x16x32_f16); for measurements.
 *   "pick_stream_priority" (0/1, default 0): the peak pick's stream gets the lowest stream priority, so that its
 *       workgroups fill what the transforms leave free; read when a device's context is created.
 *   The rules of the path that no source or test available offline pins (the crates find_peaks 0.1 and common are
 *   not in the reference tree).  Defaults (0) = the documented choices of oracle/oracle.c; every
 *   alternative is implemented in the kernels, on the host and in the test checker (same switches), DESIGN.md
 *   section 3 lists inputs on which they differ -- one run of the crates on those pins each rule:
 *     "peak_filter_order"  0: find_peaks filters by prominence, then by distance (audio_matcher.rs:226-229 builder order)
 *                          1: by distance first (every maximum that passes the height test competes), then by prominence:
 *                             scipy.signal.find_peaks' order
 *     "distance_rule"      bit 0: the distance filter drops a peak at a distance  0: <  1: <=  min_distance from a kept, higher one
 *                          bit 1: measured between  0: plateau middles (start + end) / 2   1: plateau starts
 *     "tail_window"        0: chunked(chunk + overlap, hop = chunk) (audio_matcher.rs:104) yields the shorter windows at the
 *                             end of the haystack   1: full-length windows only
 *     "surrounding_from"   filter_surrounding (audio_matcher.rs:136-139): 0: both neighbours from the sorted, unfiltered
 *                             sequence   1: the neighbour before = the last element kept (a sequential filter)
 *   test hooks: "debug_no_realloc" (0/1): a scratch buffer that would have to be (re)allocated while a batch
 *       is being queued fails the call with AM_ERR_HIP instead (every such buffer is sized before the queueing
 *       loop; this makes a violation visible); "debug_redo_arm_at" (k >= 0: the device-side redo of a batch is
 *       armed from haystack k of the call on; -1: never; -2, the default: when a failed certificate has been
 *       seen) -- pins the otherwise timing-dependent choice between the device and the host redo path;
 *       "trace_form" (0, the default: the bin length decides; 1: one wavefront per bin; 2: slices and a finish) -- runs
 *       either kernel form of the score traces at every bin length. */
/*
 * Window-energy normalised scores (normalised cross-correlation, NCC):
 *   "score_norm" (0/1, default 0): 1 = every score a call returns or picks from is
 *       ncc(t) = corr(t) / sqrt( sum(needle^2) * sum_{i=t}^{t+S-1} x_i^2 )      in [-1, 1]
 *     instead of the LibConvolve score corr(t) / sum(needle^2).  x is the sample sequence the call correlates (for
 *     AM_FMT_S16_STEREO the down-mix exactly as above), 0 outside [0, len): the zero padding of AM_MODE_FULL / _SAME
 *     counts as zeros.  sum(needle^2) is the needle's f64 energy (the needle against itself scores 1 within 1e-6).
 *     The score no longer grows with the level of the haystack: one prominence bound serves recordings of any level
 *     ("Normalised scores").  Requires scale == AM_SCALE_LIB (any other scale: AM_ERR_INVALID_ARG).
 *     Also per needle handle (am_needle_set_option); pools use the process default (their needles are internal).
 *     Supported by am_correlate*, am_match, am_match_device, am_match_batch_device, am_match_pcm16*,
 *     am_pool_match_batch and am_pool_match_batch_pcm16 (and their _device forms), am_match_best,
 *     am_match_best_device, am_match_best_batch_device and am_match_trace* (am_discover* is always NCC).  NOT supported -- AM_ERR_INVALID_ARG,
 *     "score_norm: not supported by this entry point" -- by am_match_multi*, am_match_multi_varlen_batch_device,
 *     am_match_multi_varlen, am_pool_match_multi*, am_match_stream_*, am_match_part_device and am_pool_match_long*.  am_find_peaks is unaffected.
 *     Non-finite samples cost exactly the windows that hold them (they count as 0 in every other window's energy); a
 *     haystack's result is the same bit pattern alone, in a batch and on any pool; chunking, "tail_window", the peak
 *     rules and the overshadow filter apply to the NCC scores unchanged; "half_pipeline" keeps its offsets and
 *     tolerances.  The needle's write-threshold history (sparse raw scores) is neither read nor fed by such calls:
 *     their transforms write every raw score.  On a masked handle (am_needle_create_masked) both energies run over
 *     the kept samples only: "masked needles" above.
 *   "score_norm_floor_db" (0..200, default 60; process-wide): a window whose energy is more than that many dB below
 *     the needle's, E_w < E_n * 10^(-floor/10), scores exactly 0.  Digital silence gives 0 (never NaN or inf).  The
 *     floor exists because the transform's absolute error scales with the energy of the whole overlap-save block,
 *     not with the energy of the window: in a near-silent window next to loud material that rounding residue,
 *     divided by the window's tiny energy, could otherwise show up as a hit.
 */
int am_set_option(const char* key, long long value);
int am_get_option(const char* key, long long* value);
/* "log_n", "half_pipeline" and "score_norm" per needle handle: -1 = follow the process default (initial
 * state), otherwise the handle's own value, which wins over the default. */
int am_needle_set_option(am_needle* h, const char* key, long long value);
int am_needle_get_option(const am_needle* h, const char* key, long long* value);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOMATCH_H */
