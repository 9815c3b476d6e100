// audiomatch.hpp -- header-only C++17 host mirror of the reference's matcher
// interface (the reference is compiled Rust; no Rust toolchain exists in the
// build image, so the host side above the C ABI is C++):
//
//   trait CorrelateAlgo<f32>          src/matcher/audio_matcher.rs:65-76
//   enum Mode                         src/matcher/audio_matcher.rs:55-59
//   struct Config / PeakConfig        src/matcher/audio_matcher.rs:25-53
//   LibConvolve::new / MyConvolve::new  :289 / :396
//   fn calc_chunks(...)               src/matcher/audio_matcher.rs:88-141
//   find_peaks::Peak<f32>             as consumed at matcher/mod.rs:110-129
//
// Same names, argument meaning and error behaviour: where the trait returns
// Err(Box<dyn Error>) these functions throw audiomatch::Error (calc_chunks in
// the reference unwraps, i.e. panics, audio_matcher.rs:122).  Everything is
// forwarded to libaudiomatch_amd.so (include/audiomatch.h); there is no CPU path.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "audiomatch.h"

namespace audiomatch {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc) {
    if (rc != AM_OK) throw Error(rc, std::string("audiomatch: ") + am_last_error_string());
}

enum class Mode : int { Full = AM_MODE_FULL, Same = AM_MODE_SAME, Valid = AM_MODE_VALID };

// find_peaks::Peak<f32>: position is the half-open range [start, end)
struct Peak {
    std::size_t start = 0, end = 0;
    float height = 0.f;
    float prominence = 0.f;   // Option<f32>; always Some on this path
};

// audio_matcher.rs:25-53, durations in seconds
struct Config {
    double chunk_size = 60.0;        // matcher/args.rs:70-72
    double overlap_length = 0.0;     // Config::from_args: the snippet duration (:41)
    double distance = 8 * 60.0;      // matcher/args.rs:73-76
    float prominence = 13.0f / 100;  // args.prominence / 100 (:44)

    am_match_params params(std::uint32_t sr, bool scale) const {
        am_match_params p{};
        p.sr = sr;
        p.chunk = static_cast<std::uint64_t>(std::llround(chunk_size * sr));       // :100
        p.overlap = static_cast<std::uint64_t>(std::llround(overlap_length * sr)); // :99
        p.min_prominence = prominence;
        p.min_distance = static_cast<std::uint64_t>(distance) * sr;                // distance.as_secs() * sr (:228)
        p.overshadow_distance_s = distance;
        p.scale = scale ? AM_SCALE_LIB : AM_SCALE_NONE;                            // production passes true (mod.rs:85)
        return p;
    }
};

// sample-rate conversion (am_resample, audiomatch.h): x (f32 mono, or interleaved i16 stereo with AM_FMT_S16_STEREO;
// n samples / frames) from src_rate to dst_rate, as scipy.signal.resample_poly computes it
inline std::vector<float> resample(const void* x, std::size_t n, int sample_format, std::uint32_t src_rate, std::uint32_t dst_rate,
                                   int device = 0) {
    std::size_t len = 0;
    check(am_resample_len(n, src_rate, dst_rate, &len));
    std::vector<float> out(len);
    check(am_resample(device, x, n, sample_format, src_rate, dst_rate, out.data(), out.size(), &len));
    return out;
}

// spectral whitening (audiomatch.h, "spectral whitening"): x is f32 mono, or interleaved i16 stereo with
// AM_FMT_S16_STEREO; n samples / frames.  The needle and every haystack it is matched against pass through the SAME taps.
// am_lag_products: r[k] = sum_i x[i] x[i - k], k = 0 .. order, in f64 (additive over the files of an archive)
inline std::vector<double> lag_products(const void* x, std::size_t n, int sample_format, std::uint32_t order, int device = 0) {
    std::vector<double> r(static_cast<std::size_t>(order) + 1);
    check(am_lag_products(device, x, n, sample_format, order, r.data()));
    return r;
}
// am_whiten_taps (pure host): the prediction-error filter a[0 .. order], a[0] = 1, of the lag products r[0 .. order]
inline std::vector<float> whiten_taps(const std::vector<double>& r, double noise_db = 60.0) {
    std::vector<float> taps(r.empty() ? 1 : r.size());
    check(am_whiten_taps(r.data(), static_cast<std::uint32_t>(taps.size() - 1), noise_db, taps.data()));
    return taps;
}
// am_fir: y[k] = sum_j taps[j] x[lead + k - j], k < n - lead; a signal filtered in pieces (lead = the history kept, up to
// taps.size() - 1 samples) gives the bits of the signal filtered whole
inline std::vector<float> fir(const void* x, std::size_t n, int sample_format, const std::vector<float>& taps, std::size_t lead = 0,
                              int device = 0) {
    std::vector<float> out(n >= lead ? n - lead : 0);
    std::size_t len = 0;
    check(am_fir(device, x, n, sample_format, taps.data(), static_cast<std::uint32_t>(taps.size()), lead, out.data(), out.size(), &len));
    return out;
}

// needle estimation (audiomatch.h, "needle estimation"): a clean needle from the hits of a rough one
struct NeedleEstimate {
    std::vector<float> est, dev;          // the estimate and the spread of the occurrences around it, per sample
    std::vector<std::uint32_t> count;     // the values each sample rests on
};
// am_hit_window (pure host): the row of one occurrence, fl32(x[start - lead + n] * scale), NaN where absent
inline std::vector<float> hit_window(const void* x, std::size_t n, int sample_format, std::uint64_t start, float scale, std::uint64_t lead,
                                     std::uint64_t length) {
    std::vector<float> row(static_cast<std::size_t>(length));
    check(am_hit_window(x, n, sample_format, start, scale, lead, length, row.data()));
    return row;
}
// am_needle_estimate_rows: rows holds n rows of `length` values, one occurrence after the other
inline NeedleEstimate estimate_needle(const std::vector<float>& rows, std::size_t n, std::uint32_t method = AM_EST_MEDIAN,
                                      std::uint32_t trim_permille = 0, int device = 0) {
    const am_estimate_params ep{method, trim_permille, 0, n ? rows.size() / n : 0};
    NeedleEstimate r{std::vector<float>(ep.length), std::vector<float>(ep.length), std::vector<std::uint32_t>(ep.length)};
    check(am_needle_estimate_rows(device, rows.data(), n, &ep, r.est.data(), r.dev.data(), r.count.data()));
    return r;
}
// am_needle_estimate_device: the hits in haystacks resident on `device`
inline NeedleEstimate estimate_needle_device(int device, const std::vector<const void*>& d_haystacks, const std::vector<std::size_t>& lens,
                                             int sample_format, const std::vector<am_est_hit>& hits, const am_estimate_params& ep) {
    NeedleEstimate r{std::vector<float>(ep.length), std::vector<float>(ep.length), std::vector<std::uint32_t>(ep.length)};
    check(am_needle_estimate_device(device, d_haystacks.data(), lens.data(), d_haystacks.size(), sample_format, hits.data(), hits.size(), &ep,
                                    r.est.data(), r.dev.data(), r.count.data()));
    return r;
}

// trait CorrelateAlgo<f32> (audio_matcher.rs:65-76)
// option keys of window-energy normalised scores (audiomatch.h): HipConvolve::set_option(kOptScoreNorm, 1) for NCC
// on one handle, am_set_option for the process default and the floor
constexpr const char* kOptScoreNorm = "score_norm";
constexpr const char* kOptScoreNormFloorDb = "score_norm_floor_db";

class CorrelateAlgo {
public:
    virtual ~CorrelateAlgo() = default;
    virtual float inverse_sample_auto_correlation() const = 0;
    virtual std::vector<float> correlate_with_sample(const float* within, std::size_t len, Mode mode,
                                                     bool scale) const = 0;
    // provided method `scale` (:73-75)
    void scale(std::vector<float>& data) const {
        const float f = inverse_sample_auto_correlation();
        for (float& v : data) v *= f;
    }
};

// The HIP-backed implementation: drop-in for LibConvolve (production, mod.rs:34).
class HipConvolve final : public CorrelateAlgo {
public:
    explicit HipConvolve(const std::vector<float>& sample_data, int device = 0) {
        check(am_needle_create(device, sample_data.data(), sample_data.size(), &h_));
    }
    // am_needle_create_resampled: the needle (f32 mono, or interleaved i16 stereo with AM_FMT_S16_STEREO; n samples /
    // frames) brought from src_rate to the haystack's dst_rate
    HipConvolve(const void* needle, std::size_t n, int sample_format, std::uint32_t src_rate, std::uint32_t dst_rate, int device = 0) {
        check(am_needle_create_resampled(device, needle, n, sample_format, src_rate, dst_rate, &h_));
    }
    // am_needle_create_filtered: the needle passed through the FIR filter `taps` (whiten_taps of the haystacks' lag
    // products, or a pre-emphasis {1, -alpha}); the haystacks pass through the same taps (fir)
    HipConvolve(const void* needle, std::size_t n, int sample_format, const std::vector<float>& taps, int device = 0) {
        check(am_needle_create_filtered(device, needle, n, sample_format, taps.data(), static_cast<std::uint32_t>(taps.size()), &h_));
    }
    // am_needle_create_masked: a masked needle, `gaps` the spans [begin, end) of its samples to ignore (under "score_norm"
    // the scores are NCC over the kept samples only); no gaps: the ordinary handle
    HipConvolve(const std::vector<float>& sample_data, const std::vector<am_span>& gaps, int device = 0) {
        check(am_needle_create_masked(device, sample_data.data(), sample_data.size(), gaps.data(), gaps.size(), &h_));
    }
    // am_needle_mask: the handle's gaps (none for an ordinary handle)
    std::vector<am_span> mask() const {
        std::vector<am_span> g(AM_MASK_MAX_GAPS);
        std::size_t n = 0;
        check(am_needle_mask(h_, g.data(), g.size(), &n));
        g.resize(n);
        return g;
    }
    HipConvolve(const HipConvolve&) = delete;
    HipConvolve& operator=(const HipConvolve&) = delete;
    HipConvolve(HipConvolve&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~HipConvolve() override { am_needle_destroy(h_); }

    float inverse_sample_auto_correlation() const override {
        float v = 0.f;
        check(am_needle_inv_autocorr(h_, &v));
        return v;
    }
    std::vector<float> correlate_with_sample(const float* within, std::size_t len, Mode mode,
                                             bool scale) const override {
        std::size_t s = 0, n = 0;
        check(am_needle_len(h_, &s));
        check(am_correlate_len(len, s, static_cast<int>(mode), &n));
        std::vector<float> out(n);
        check(am_correlate(h_, within, len, static_cast<int>(mode), scale ? AM_SCALE_LIB : AM_SCALE_NONE,
                           out.data(), out.size(), &n));
        return out;
    }
    const am_needle* handle() const { return h_; }
    // per-hit scoring (am_hit_scores): exact NCC, gain, window level and sub-sample position of each of `peaks`, found in
    // the host haystack of `sample_format` (len in samples / frames); am_hit_scores_device for a resident haystack
    std::vector<am_hit_score> hit_scores(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks) const {
        std::vector<am_hit_score> out(peaks.size());
        check(am_hit_scores(h_, haystack, len, sample_format, peaks.data(), peaks.size(), out.data()));
        return out;
    }
    std::vector<am_hit_score> hit_scores_device(const void* d_haystack, std::size_t len, int sample_format,
                                                const std::vector<am_peak>& peaks) const {
        std::vector<am_hit_score> out(peaks.size());
        check(am_hit_scores_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), out.data()));
        return out;
    }
    // the per-hit record of a masked handle (am_hit_mask): exact masked NCC, gain and level over the kept samples, and what
    // the gaps hold against the needle's original samples there; am_hit_mask_device for a resident haystack, and
    // am_hit_mask_batch_device (the C call, pair layout of am_match_multi_batch_device) for several handles and haystacks
    std::vector<am_mask_hit> hit_mask(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks) const {
        std::vector<am_mask_hit> out(peaks.size());
        check(am_hit_mask(h_, haystack, len, sample_format, peaks.data(), peaks.size(), out.data()));
        return out;
    }
    std::vector<am_mask_hit> hit_mask_device(const void* d_haystack, std::size_t len, int sample_format,
                                             const std::vector<am_peak>& peaks) const {
        std::vector<am_mask_hit> out(peaks.size());
        check(am_hit_mask_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), out.data()));
        return out;
    }
    // per-segment hit scoring (am_hit_segments): sp.segments records per peak, peak i at [i * segments, (i + 1) * segments)
    std::vector<am_hit_segment> hit_segments(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                             const am_segment_params& sp) const {
        std::vector<am_hit_segment> out(peaks.size() * sp.segments);
        check(am_hit_segments(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    std::vector<am_hit_segment> hit_segments_device(const void* d_haystack, std::size_t len, int sample_format,
                                                    const std::vector<am_peak>& peaks, const am_segment_params& sp) const {
        std::vector<am_hit_segment> out(peaks.size() * sp.segments);
        check(am_hit_segments_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    // per-hit drift scoring (am_hit_warp): each peak's clock drift, refined lag and corrected NCC over the grid wp, one
    // record per peak
    std::vector<am_warp_hit> hit_warp(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                      const am_warp_params& wp) const {
        std::vector<am_warp_hit> out(peaks.size());
        check(am_hit_warp(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &wp, out.data()));
        return out;
    }
    std::vector<am_warp_hit> hit_warp_device(const void* d_haystack, std::size_t len, int sample_format,
                                             const std::vector<am_peak>& peaks, const am_warp_params& wp) const {
        std::vector<am_warp_hit> out(peaks.size());
        check(am_hit_warp_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &wp, out.data()));
        return out;
    }
    // the interpolator's table (am_warp_table) and one occurrence's row on the needle's clock (am_hit_window_warped); no
    // device needed.  The batch form is am_hit_warp_batch_device of the C interface.
    static std::vector<float> warp_table() {
        std::vector<float> t(static_cast<std::size_t>(AM_WARP_PHASES) * AM_WARP_TAPS);
        check(am_warp_table(t.data()));
        return t;
    }
    static std::vector<float> hit_window_warped(const void* haystack, std::size_t len, int sample_format, std::uint64_t start, float scale,
                                                double lag, double drift_ppm, std::uint64_t lead, std::uint64_t length) {
        std::vector<float> row(length);
        check(am_hit_window_warped(haystack, len, sample_format, start, scale, lag, drift_ppm, lead, length, row.data()));
        return row;
    }
    // per-hit channel estimation (am_hit_channel): each peak's record, and its taps h[-P .. P] at taps[i (2P + 1) ..]
    struct ChannelHits {
        std::vector<am_channel_hit> records;
        std::vector<float> taps;
    };
    ChannelHits hit_channel(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                            const am_channel_params& cp) const {
        ChannelHits out{std::vector<am_channel_hit>(peaks.size()), std::vector<float>(peaks.size() * (2 * static_cast<std::size_t>(cp.radius) + 1))};
        check(am_hit_channel(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &cp, out.records.data(), out.taps.data()));
        return out;
    }
    ChannelHits hit_channel_device(const void* d_haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                   const am_channel_params& cp) const {
        ChannelHits out{std::vector<am_channel_hit>(peaks.size()), std::vector<float>(peaks.size() * (2 * static_cast<std::size_t>(cp.radius) + 1))};
        check(am_hit_channel_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &cp, out.records.data(), out.taps.data()));
        return out;
    }
    // the solve by itself (am_channel_solve) and the filtered needle under a hit with what is left (am_hit_residual); no
    // device needed.  The batch form is am_hit_channel_batch_device of the C interface.
    static std::vector<double> channel_solve(const std::vector<double>& r, const std::vector<double>& c, double noise_db, bool* ill = nullptr) {
        std::vector<double> h(r.size());
        int fell_back = 0;
        if (r.size() != c.size() || r.size() % 2 == 0) throw Error(AM_ERR_INVALID_ARG, "channel_solve: r and c hold 2P + 1 values each");
        check(am_channel_solve(r.data(), c.data(), static_cast<std::uint32_t>(r.size() / 2), noise_db, h.data(), &fell_back));
        if (ill) *ill = fell_back != 0;
        return h;
    }
    struct Residual {
        std::vector<float> model, resid;
    };
    static Residual hit_residual(const void* haystack, std::size_t len, int sample_format, std::uint64_t start, const std::vector<float>& needle,
                                 const std::vector<float>& taps) {
        if (taps.size() % 2 == 0) throw Error(AM_ERR_INVALID_ARG, "hit_residual: taps hold 2P + 1 values");
        Residual out{std::vector<float>(needle.size() + taps.size() - 1), std::vector<float>(needle.size() + taps.size() - 1)};
        check(am_hit_residual(haystack, len, sample_format, start, needle.data(), needle.size(), taps.data(),
                              static_cast<std::uint32_t>(taps.size() / 2), out.model.data(), out.resid.data()));
        return out;
    }
    // per-band hit scoring (am_hit_bands): bp.n_bands records per peak, peak i band b at i * n_bands + b
    std::vector<am_hit_band> hit_bands(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                       const am_band_params& bp) const {
        std::vector<am_hit_band> out(peaks.size() * bp.n_bands);
        check(am_hit_bands(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &bp, out.data()));
        return out;
    }
    std::vector<am_hit_band> hit_bands_device(const void* d_haystack, std::size_t len, int sample_format,
                                              const std::vector<am_peak>& peaks, const am_band_params& bp) const {
        std::vector<am_hit_band> out(peaks.size() * bp.n_bands);
        check(am_hit_bands_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &bp, out.data()));
        return out;
    }
    // per-hit significance (am_hit_significance): each peak's score against the scores at lags guard < |lag| <= radius
    // around it (mean, standard deviation, z and the largest background score), one record per peak
    std::vector<am_significance> hit_significance(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                                  const am_significance_params& sp) const {
        std::vector<am_significance> out(peaks.size());
        check(am_hit_significance(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    std::vector<am_significance> hit_significance_device(const void* d_haystack, std::size_t len, int sample_format,
                                                         const std::vector<am_peak>& peaks, const am_significance_params& sp) const {
        std::vector<am_significance> out(peaks.size());
        check(am_hit_significance_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    // per-hit stereo image (am_hit_stereo): where each peak sits between the channels of a haystack of i16 stereo frames
    // (AM_FMT_S16_STEREO only), one record per peak.  The batch form is am_hit_stereo_batch_device of the C interface.
    std::vector<am_stereo_hit> hit_stereo(const void* haystack, std::size_t len, int sample_format, const std::vector<am_peak>& peaks,
                                          const am_stereo_params& sp) const {
        std::vector<am_stereo_hit> out(peaks.size());
        check(am_hit_stereo(h_, haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    std::vector<am_stereo_hit> hit_stereo_device(const void* d_haystack, std::size_t len, int sample_format,
                                                 const std::vector<am_peak>& peaks, const am_stereo_params& sp) const {
        std::vector<am_stereo_hit> out(peaks.size());
        check(am_hit_stereo_device(h_, d_haystack, len, sample_format, peaks.data(), peaks.size(), &sp, out.data()));
        return out;
    }
    // image, balance, delay and what the down-mix cost, from one record (am_hit_stereo_summary; no device needed)
    static am_stereo_summary stereo_summary(const am_stereo_hit& rec, float min_ncc) {
        am_stereo_summary out{};
        check(am_hit_stereo_summary(&rec, min_ncc, &out));
        return out;
    }
    // a stereo mix other than the down-mix (am_pcm_s16_stereo_mix): f32((a L + b R) k) of `frames` interleaved i16 frames;
    // the resident form is am_pcm_s16_stereo_mix_device of the C interface
    static std::vector<float> pcm_s16_stereo_mix(int device, const std::int16_t* interleaved, std::size_t frames, float a, float b) {
        std::vector<float> out(frames);
        check(am_pcm_s16_stereo_mix(device, interleaved, frames, a, b, out.data()));
        return out;
    }
    // coverage, drift and refined start of one hit from its records (am_hit_segments_summary; no device needed)
    static am_segment_summary segment_summary(const am_hit_segment* seg, std::uint32_t segments, std::size_t needle_len, float min_ncc) {
        am_segment_summary out{};
        check(am_hit_segments_summary(seg, segments, needle_len, min_ncc, &out));
        return out;
    }
    // how much of the needle's spectrum one hit holds, from its band records (am_hit_bands_summary; no device needed)
    static am_band_summary band_summary(const am_hit_band* rec, std::uint32_t n_bands, float min_coherence) {
        am_band_summary out{};
        check(am_hit_bands_summary(rec, n_bands, min_coherence, &out));
        return out;
    }
    // n_bands log-spaced bands from lo_hz to hi_hz for frames of 2^frame_log2 samples (am_band_edges_log; no device needed)
    static am_band_params band_edges_log(std::uint32_t sr, std::uint32_t frame_log2, double lo_hz, double hi_hz, std::uint32_t n_bands) {
        am_band_params out{};
        check(am_band_edges_log(sr, frame_log2, lo_hz, hi_hz, n_bands, &out));
        return out;
    }
    // the k best matches (am_match_best): the best min(k, count) peaks of the haystack's Valid scores by descending
    // height, no prominence threshold needed; am_match_best_device / _batch_device for resident haystacks
    std::vector<am_peak> match_best(const void* haystack, std::size_t len, int sample_format, const am_best_params& bp) const {
        std::vector<am_peak> out(static_cast<std::size_t>(bp.k));
        std::size_t n = 0;
        check(am_match_best(h_, haystack, len, sample_format, &bp, out.data(), &n));
        out.resize(n);
        return out;
    }
    std::vector<am_peak> match_best_device(const void* d_haystack, std::size_t len, int sample_format, const am_best_params& bp) const {
        std::vector<am_peak> out(static_cast<std::size_t>(bp.k));
        std::size_t n = 0;
        check(am_match_best_device(h_, d_haystack, len, sample_format, &bp, out.data(), &n));
        out.resize(n);
        return out;
    }
    std::vector<std::vector<am_peak>> match_best_batch_device(const std::vector<const void*>& d_haystacks, const std::vector<std::size_t>& lens,
                                                              int sample_format, const am_best_params& bp) const {
        if (d_haystacks.size() != lens.size()) check(AM_ERR_INVALID_ARG);
        const std::size_t nh = d_haystacks.size(), k = static_cast<std::size_t>(bp.k);
        std::vector<am_peak> buf(std::max<std::size_t>(1, nh * k));
        std::vector<std::size_t> n(std::max<std::size_t>(1, nh), 0);
        check(am_match_best_batch_device(h_, d_haystacks.data(), lens.data(), nh, sample_format, &bp, buf.data(), n.data()));
        std::vector<std::vector<am_peak>> out(nh);
        for (std::size_t i = 0; i < nh; ++i) out[i].assign(buf.begin() + (std::ptrdiff_t)(i * k), buf.begin() + (std::ptrdiff_t)(i * k + n[i]));
        return out;
    }
    // score traces (am_match_trace): one am_trace_bin per tp.bin Valid scores of the haystack -- the array match_best
    // selects from; am_match_trace_device / _batch_device for resident haystacks
    std::vector<am_trace_bin> match_trace(const void* haystack, std::size_t len, int sample_format, const am_trace_params& tp) const {
        return trace_filled(len, tp, [&](am_trace_bin* out, std::size_t cap, std::size_t* n) {
            return am_match_trace(h_, haystack, len, sample_format, &tp, out, cap, n);
        });
    }
    std::vector<am_trace_bin> match_trace_device(const void* d_haystack, std::size_t len, int sample_format, const am_trace_params& tp) const {
        return trace_filled(len, tp, [&](am_trace_bin* out, std::size_t cap, std::size_t* n) {
            return am_match_trace_device(h_, d_haystack, len, sample_format, &tp, out, cap, n);
        });
    }
    std::vector<std::vector<am_trace_bin>> match_trace_batch_device(const std::vector<const void*>& d_haystacks, const std::vector<std::size_t>& lens,
                                                                    int sample_format, const am_trace_params& tp) const {
        if (d_haystacks.size() != lens.size()) check(AM_ERR_INVALID_ARG);
        const std::size_t nh = d_haystacks.size();
        std::size_t cap = 0;
        for (std::size_t len : lens) cap = std::max(cap, trace_bins_of(len, tp));
        std::vector<am_trace_bin> buf(std::max<std::size_t>(1, nh * cap));
        std::vector<std::size_t> n(std::max<std::size_t>(1, nh), 0);
        check(am_match_trace_batch_device(h_, d_haystacks.data(), lens.data(), nh, sample_format, &tp, buf.data(), cap, n.data()));
        std::vector<std::vector<am_trace_bin>> out(nh);
        for (std::size_t i = 0; i < nh; ++i) out[i].assign(buf.begin() + (std::ptrdiff_t)(i * cap), buf.begin() + (std::ptrdiff_t)(i * cap + n[i]));
        return out;
    }
    // edge matching (am_match_edges): the records of the two edges of a haystack, [0] the head's (the recording starts
    // inside the needle), [1] the tail's (it ends inside it); edge_scores: the coarse score of every lag of one edge
    std::array<am_edge_hit, 2> match_edges(const void* haystack, std::size_t len, int sample_format, const am_edge_params& ep) const {
        std::array<am_edge_hit, 2> out{};
        check(am_match_edges(h_, haystack, len, sample_format, &ep, out.data()));
        return out;
    }
    std::array<am_edge_hit, 2> match_edges_device(const void* d_haystack, std::size_t len, int sample_format, const am_edge_params& ep) const {
        std::array<am_edge_hit, 2> out{};
        check(am_match_edges_device(h_, d_haystack, len, sample_format, &ep, out.data()));
        return out;
    }
    std::vector<std::array<am_edge_hit, 2>> match_edges_batch_device(const std::vector<const void*>& d_haystacks, const std::vector<std::size_t>& lens,
                                                                     int sample_format, const am_edge_params& ep) const {
        if (d_haystacks.size() != lens.size()) check(AM_ERR_INVALID_ARG);
        std::vector<std::array<am_edge_hit, 2>> out(d_haystacks.size());
        static_assert(sizeof(std::array<am_edge_hit, 2>) == 2 * sizeof(am_edge_hit), "two records side by side");
        check(am_match_edges_batch_device(h_, d_haystacks.data(), lens.data(), d_haystacks.size(), sample_format, &ep,
                                          out.empty() ? nullptr : out[0].data()));
        return out;
    }
    std::vector<float> edge_scores(const void* haystack, std::size_t len, int sample_format, int edge, const am_edge_params& ep) const {
        return edge_scores_filled(len, edge, [&](float* out, std::size_t cap, std::size_t* n) {
            return am_edge_scores(h_, haystack, len, sample_format, edge, &ep, out, cap, n);
        });
    }
    std::vector<float> edge_scores_device(const void* d_haystack, std::size_t len, int sample_format, int edge, const am_edge_params& ep) const {
        return edge_scores_filled(len, edge, [&](float* out, std::size_t cap, std::size_t* n) {
            return am_edge_scores_device(h_, d_haystack, len, sample_format, edge, &ep, out, cap, n);
        });
    }
    template <class Call>
    std::vector<float> edge_scores_filled(std::size_t len, int edge, Call call) const {
        std::size_t s = 0, n = 0;
        std::int64_t first = 0;
        check(am_needle_len(h_, &s));
        check(am_edge_scores_len(len, s, edge, &n, &first));
        std::vector<float> out(std::max<std::size_t>(1, n));
        check(call(out.data(), n, &n));
        out.resize(n);
        return out;
    }
    // runs call(out, cap, &n) on a growing record buffer until it fits
    template <class Call>
    static std::vector<am_env_hit> env_hits_filled(Call call) {
        std::vector<am_env_hit> out(64);
        std::size_t n = 0;
        int rc = call(out.data(), out.size(), &n);
        if (rc == AM_ERR_CAPACITY) {
            out.resize(n);
            rc = call(out.data(), out.size(), &n);
        }
        check(rc);
        out.resize(std::min(n, out.size()));
        return out;
    }
    // envelope matching (am_match_envelope): this needle played at any speed of `grid`, found through its band-level
    // envelopes -- starts good to a few frames, drifts to a grid step or two; am_match_envelope_device for a resident haystack
    std::vector<am_env_hit> match_envelope(const void* haystack, std::size_t len, int sample_format, const am_env_params& ep,
                                           const am_env_grid& grid, float min_score) const {
        return env_hits_filled([&](am_env_hit* out, std::size_t cap, std::size_t* n) {
            return am_match_envelope(h_, haystack, len, sample_format, &ep, &grid, min_score, out, cap, n);
        });
    }
    std::vector<am_env_hit> match_envelope_device(const void* d_haystack, std::size_t len, int sample_format, const am_env_params& ep,
                                                  const am_env_grid& grid, float min_score) const {
        return env_hits_filled([&](am_env_hit* out, std::size_t cap, std::size_t* n) {
            return am_match_envelope_device(h_, d_haystack, len, sample_format, &ep, &grid, min_score, out, cap, n);
        });
    }
    // am_env_params over bands (band_edges_log) with the level floor in dB below a full-scale sine
    static am_env_params env_params(const am_band_params& bands, double floor_db = 80.0) {
        am_env_params ep{};
        ep.bands = bands;
        ep.floor_db = floor_db;
        return ep;
    }
    // per-handle "log_n" / "half_pipeline" / "score_norm" (-1 = follow the process default)
    void set_option(const char* key, long long value) { check(am_needle_set_option(h_, key, value)); }

private:
    // the records a haystack of len samples has under tp (am_trace_len over its Valid scores)
    std::size_t trace_bins_of(std::size_t len, const am_trace_params& tp) const {
        std::size_t s = 0, nb = 0;
        check(am_needle_len(h_, &s));
        check(am_trace_len(len >= s ? len - s + 1 : 0, tp.bin, &nb));
        return nb;
    }
    template <class Call>
    std::vector<am_trace_bin> trace_filled(std::size_t len, const am_trace_params& tp, Call call) const {
        std::vector<am_trace_bin> out(trace_bins_of(len, tp));
        std::size_t n = 0;
        check(call(out.data(), out.size(), &n));
        out.resize(std::min(n, out.size()));
        return out;
    }
    am_needle* h_ = nullptr;
};

// am_find_peaks_top: the first min(k, count) peaks find_peaks(scores) returns, by descending height, computed without
// listing them all; find_peaks_top_device for scores resident on `device`
inline std::vector<am_peak> find_peaks_top(const float* scores, std::size_t n, std::size_t k, float min_prominence = 0.0f,
                                           std::uint64_t min_distance = 0, int device = 0) {
    std::vector<am_peak> out(k);
    std::size_t got = 0;
    check(am_find_peaks_top(device, scores, n, min_prominence, min_distance, k, out.data(), &got));
    out.resize(got);
    return out;
}
inline std::vector<am_peak> find_peaks_top_device(const float* d_scores, std::size_t n, std::size_t k, float min_prominence = 0.0f,
                                                  std::uint64_t min_distance = 0, int device = 0) {
    std::vector<am_peak> out(k);
    std::size_t got = 0;
    check(am_find_peaks_top_device(device, d_scores, n, min_prominence, min_distance, k, out.data(), &got));
    out.resize(got);
    return out;
}

// am_trace_scores: one am_trace_bin per `bin` scores of any score array; trace_scores_device for scores resident on
// `device` (any 4-byte alignment); trace_summary: am_trace_summary of a trace's records (no device needed)
inline std::vector<am_trace_bin> trace_scores(const float* scores, std::size_t n, std::uint64_t bin, int device = 0) {
    std::size_t nb = 0, got = 0;
    check(am_trace_len(n, bin, &nb));
    std::vector<am_trace_bin> out(nb);
    check(am_trace_scores(device, scores, n, bin, out.data(), nb, &got));
    return out;
}
inline std::vector<am_trace_bin> trace_scores_device(const float* d_scores, std::size_t n, std::uint64_t bin, int device = 0) {
    std::size_t nb = 0, got = 0;
    check(am_trace_len(n, bin, &nb));
    std::vector<am_trace_bin> out(nb);
    check(am_trace_scores_device(device, d_scores, n, bin, out.data(), nb, &got));
    return out;
}
inline am_trace_stats trace_summary(const std::vector<am_trace_bin>& bins, std::uint64_t bin) {
    am_trace_stats out{};
    check(am_trace_summary(bins.data(), bins.size(), bin, &out));
    return out;
}

// needle discovery (am_discover*): one am_probe_hit per probe of recording A matched against recording B (host memory /
// memory of `device`); probe_scores*: the record rule on any score array; discover_regions: the regions the records
// chain into (no device needed)
inline std::size_t discover_len(std::size_t len_a, const am_discover_params& dp) {
    std::size_t n = 0;
    check(am_discover_len(len_a, &dp, &n));
    return n;
}
inline std::vector<am_probe_hit> discover(const void* a, std::size_t len_a, const void* b, std::size_t len_b, int sample_format,
                                          const am_discover_params& dp, int device = 0) {
    std::vector<am_probe_hit> out(discover_len(len_a, dp));
    std::size_t n = 0;
    check(am_discover(device, a, len_a, b, len_b, sample_format, &dp, out.data(), out.size(), &n));
    out.resize(std::min(n, out.size()));
    return out;
}
inline std::vector<am_probe_hit> discover_device(const void* d_a, std::size_t len_a, const void* d_b, std::size_t len_b, int sample_format,
                                                 const am_discover_params& dp, int device = 0) {
    std::vector<am_probe_hit> out(discover_len(len_a, dp));
    std::size_t n = 0;
    check(am_discover_device(device, d_a, len_a, d_b, len_b, sample_format, &dp, out.data(), out.size(), &n));
    out.resize(std::min(n, out.size()));
    return out;
}
inline am_probe_hit probe_scores(const float* scores, std::size_t n, std::uint64_t ex_lo, std::uint64_t ex_hi, std::uint64_t separation,
                                 int device = 0) {
    am_probe_hit out{};
    check(am_probe_scores(device, scores, n, ex_lo, ex_hi, separation, &out));
    return out;
}
inline am_probe_hit probe_scores_device(const float* d_scores, std::size_t n, std::uint64_t ex_lo, std::uint64_t ex_hi,
                                        std::uint64_t separation, int device = 0) {
    am_probe_hit out{};
    check(am_probe_scores_device(device, d_scores, n, ex_lo, ex_hi, separation, &out));
    return out;
}
inline std::vector<am_region> discover_regions(const std::vector<am_probe_hit>& hits, const am_discover_params& dp,
                                               const am_region_params& rp) {
    std::vector<am_region> out(hits.size());   // (a region holds at least one probe)
    std::size_t n = 0;
    check(am_discover_regions(hits.data(), hits.size(), &dp, &rp, out.data(), out.size(), &n));
    out.resize(std::min(n, out.size()));
    return out;
}

// envelope matching on its own (am_envelope*, am_envelope_scores*, am_envelope_pick): the band levels of a signal read at
// drift_ppm (n_bands x J uint16, band-major; host memory / memory of `device`), the scores of a bank of needle level
// matrices against a haystack's, and the pick rule on any (z, qi) (no device needed)
inline std::size_t envelope_len(std::size_t len, const am_env_params& ep, double drift_ppm = 0.0) {
    std::size_t n = 0;
    check(am_envelope_len(len, &ep, drift_ppm, &n));
    return n;
}
inline std::vector<std::uint16_t> envelope(const void* signal, std::size_t len, int sample_format, const am_env_params& ep,
                                           double drift_ppm = 0.0, int device = 0) {
    const std::size_t j = envelope_len(len, ep, drift_ppm);
    std::vector<std::uint16_t> out(std::max<std::size_t>(1, ep.bands.n_bands * j));
    std::size_t n = 0;
    check(am_envelope(device, signal, len, sample_format, &ep, drift_ppm, out.data(), j, &n));
    out.resize(ep.bands.n_bands * n);
    return out;
}
inline std::vector<std::uint16_t> envelope_device(const void* d_signal, std::size_t len, int sample_format, const am_env_params& ep,
                                                  double drift_ppm = 0.0, int device = 0) {
    const std::size_t j = envelope_len(len, ep, drift_ppm);
    std::vector<std::uint16_t> out(std::max<std::size_t>(1, ep.bands.n_bands * j));
    std::size_t n = 0;
    check(am_envelope_device(device, d_signal, len, sample_format, &ep, drift_ppm, out.data(), j, &n));
    out.resize(ep.bands.n_bands * n);
    return out;
}
struct EnvScores { std::vector<float> z; std::vector<std::uint32_t> qi; };
inline EnvScores envelope_scores(const std::uint16_t* needles, const std::vector<std::uint32_t>& frames, std::uint32_t n_bands,
                                 const std::uint16_t* hay, std::size_t hay_frames, int device = 0, bool resident = false) {
    std::size_t cap = 0;
    for (std::uint32_t j : frames)
        if (hay_frames >= j) cap = std::max(cap, hay_frames - j + 1);
    EnvScores r{std::vector<float>(std::max<std::size_t>(1, cap)), std::vector<std::uint32_t>(std::max<std::size_t>(1, cap))};
    std::size_t n = 0;
    const std::uint32_t q = (std::uint32_t)frames.size();
    check(resident ? am_envelope_scores_device(device, needles, frames.data(), q, n_bands, hay, hay_frames, r.z.data(), r.qi.data(), cap, &n)
                   : am_envelope_scores(device, needles, frames.data(), q, n_bands, hay, hay_frames, r.z.data(), r.qi.data(), cap, &n));
    r.z.resize(n);
    r.qi.resize(n);
    return r;
}
inline std::vector<am_env_pick> envelope_pick(const std::vector<float>& z, const std::vector<std::uint32_t>& qi, float min_score,
                                              std::uint64_t separation) {
    if (z.size() != qi.size()) check(AM_ERR_INVALID_ARG);
    std::vector<am_env_pick> out(z.size());
    std::size_t n = 0;
    check(am_envelope_pick(z.data(), qi.data(), z.size(), min_score, separation, out.data(), out.size(), &n));
    out.resize(std::min(n, out.size()));
    return out;
}

// calc_chunks(sr, m_samples, &algo, scale, config) (audio_matcher.rs:88-141):
// peaks sorted by position.start, overshadowed neighbours removed.
inline std::vector<Peak> calc_chunks(std::uint16_t sr, const float* m_samples, std::size_t len,
                                     const HipConvolve& algo_with_sample, bool scale, const Config& config) {
    const am_match_params p = config.params(sr, scale);
    std::vector<am_peak> buf(256);
    std::size_t n = 0;
    int rc = am_match(algo_with_sample.handle(), m_samples, len, &p, buf.data(), buf.size(), &n);
    if (rc == AM_ERR_CAPACITY) {
        buf.resize(n);
        rc = am_match(algo_with_sample.handle(), m_samples, len, &p, buf.data(), buf.size(), &n);
    }
    check(rc);
    std::vector<Peak> out(n);
    for (std::size_t i = 0; i < n; ++i)
        out[i] = Peak{static_cast<std::size_t>(buf[i].start), static_cast<std::size_t>(buf[i].end),
                      buf[i].height, buf[i].prominence};
    return out;
}

// calc_chunks for SEVERAL snippets of any lengths against one haystack (am_match_multi_varlen): result [j] = what
// calc_chunks with needles[j] and overlap overlaps[j] returns (overlaps empty: the config's overlap for every needle);
// the haystack is host memory of `sample_format` (AM_FMT_*), len in samples / frames.
inline std::vector<std::vector<Peak>> calc_chunks_multi(std::uint16_t sr, const void* m_samples, std::size_t len, int sample_format,
                                                        const std::vector<const HipConvolve*>& needles, bool scale, const Config& config,
                                                        const std::vector<std::uint64_t>& overlaps = {}, std::size_t cap_per_needle = 256) {
    const am_match_params p = config.params(sr, scale);
    const std::size_t k = needles.size();
    std::vector<const am_needle*> hs;
    for (const HipConvolve* h : needles) hs.push_back(h->handle());
    if (!overlaps.empty() && overlaps.size() != k) check(AM_ERR_INVALID_ARG);
    const std::uint64_t* ov = overlaps.empty() ? nullptr : overlaps.data();
    std::vector<am_peak> buf(k * cap_per_needle);
    std::vector<std::size_t> n(k, 0);
    int rc = am_match_multi_varlen(hs.data(), k, ov, m_samples, len, sample_format, &p, buf.data(), cap_per_needle, n.data());
    if (rc == AM_ERR_CAPACITY) {
        for (std::size_t v : n) cap_per_needle = std::max(cap_per_needle, v);
        buf.assign(k * cap_per_needle, am_peak{});
        rc = am_match_multi_varlen(hs.data(), k, ov, m_samples, len, sample_format, &p, buf.data(), cap_per_needle, n.data());
    }
    check(rc);
    std::vector<std::vector<Peak>> out(k);
    for (std::size_t j = 0; j < k; ++j)
        for (std::size_t q = 0; q < n[j]; ++q) {
            const am_peak& v = buf[j * cap_per_needle + q];
            out[j].push_back(Peak{static_cast<std::size_t>(v.start), static_cast<std::size_t>(v.end), v.height, v.prominence});
        }
    return out;
}
// ... and against a batch of resident haystacks (am_match_multi_varlen_batch_device): result [k][j]
inline std::vector<std::vector<std::vector<Peak>>> calc_chunks_multi_device(std::uint16_t sr, const std::vector<const void*>& d_haystacks,
                                                                           const std::vector<std::size_t>& lens, int sample_format,
                                                                           const std::vector<const HipConvolve*>& needles, bool scale,
                                                                           const Config& config, const std::vector<std::uint64_t>& overlaps = {},
                                                                           std::size_t cap_per_pair = 64) {
    const am_match_params p = config.params(sr, scale);
    const std::size_t k = d_haystacks.size(), nn = needles.size();
    std::vector<const am_needle*> hs;
    for (const HipConvolve* h : needles) hs.push_back(h->handle());
    if (!overlaps.empty() && overlaps.size() != nn) check(AM_ERR_INVALID_ARG);
    const std::uint64_t* ov = overlaps.empty() ? nullptr : overlaps.data();
    std::vector<am_peak> buf(k * nn * cap_per_pair);
    std::vector<std::size_t> n(k * nn, 0);
    int rc = am_match_multi_varlen_batch_device(hs.data(), nn, ov, d_haystacks.data(), lens.data(), k, sample_format, &p, buf.data(),
                                                cap_per_pair, n.data());
    if (rc == AM_ERR_CAPACITY) {
        for (std::size_t v : n) cap_per_pair = std::max(cap_per_pair, v);
        buf.assign(k * nn * cap_per_pair, am_peak{});
        rc = am_match_multi_varlen_batch_device(hs.data(), nn, ov, d_haystacks.data(), lens.data(), k, sample_format, &p, buf.data(),
                                                cap_per_pair, n.data());
    }
    check(rc);
    std::vector<std::vector<std::vector<Peak>>> out(k, std::vector<std::vector<Peak>>(nn));
    for (std::size_t i = 0; i < k; ++i)
        for (std::size_t j = 0; j < nn; ++j)
            for (std::size_t q = 0; q < n[i * nn + j]; ++q) {
                const am_peak& v = buf[(i * nn + j) * cap_per_pair + q];
                out[i][j].push_back(Peak{static_cast<std::size_t>(v.start), static_cast<std::size_t>(v.end), v.height, v.prominence});
            }
    return out;
}

// The per-file loop of matcher::run (matcher/mod.rs:42-87) over every GPU of the node: the
// needle replicated per device, haystack k matched on device k mod n (am_pool_*), one submit
// thread per device inside the library, results gathered on the host.
class HipConvolvePool {
public:
    // devices empty: every visible device
    explicit HipConvolvePool(const std::vector<float>& sample_data, const std::vector<int>& devices = {}) {
        check(am_pool_create(sample_data.data(), sample_data.size(), devices.empty() ? nullptr : devices.data(),
                             devices.size(), &p_));
    }
    HipConvolvePool(const HipConvolvePool&) = delete;
    HipConvolvePool& operator=(const HipConvolvePool&) = delete;
    ~HipConvolvePool() { am_pool_destroy(p_); }
    std::size_t size() const {
        std::size_t n = 0;
        check(am_pool_size(p_, &n));
        return n;
    }
    // calc_chunks for every haystack of the batch (host buffers); result k belongs to haystacks[k]
    std::vector<std::vector<Peak>> calc_chunks(std::uint16_t sr, const std::vector<const float*>& haystacks,
                                               const std::vector<std::size_t>& lens, bool scale, const Config& config,
                                               std::size_t cap_per_haystack = 256) {
        const am_match_params p = config.params(sr, scale);
        const std::size_t k = haystacks.size();
        std::vector<am_peak> buf(k * cap_per_haystack);
        std::vector<std::size_t> n(k, 0);
        int rc = am_pool_match_batch(p_, haystacks.data(), lens.data(), k, &p, buf.data(), cap_per_haystack, n.data());
        if (rc == AM_ERR_CAPACITY) {
            for (std::size_t v : n) cap_per_haystack = std::max(cap_per_haystack, v);
            buf.assign(k * cap_per_haystack, am_peak{});
            rc = am_pool_match_batch(p_, haystacks.data(), lens.data(), k, &p, buf.data(), cap_per_haystack, n.data());
        }
        check(rc);
        std::vector<std::vector<Peak>> out(k);
        for (std::size_t i = 0; i < k; ++i)
            for (std::size_t j = 0; j < n[i]; ++j) {
                const am_peak& q = buf[i * cap_per_haystack + j];
                out[i].push_back(Peak{static_cast<std::size_t>(q.start), static_cast<std::size_t>(q.end), q.height, q.prominence});
            }
        return out;
    }

    // the same loop on interleaved i16 stereo frames, the format the reference decodes to
    // (mp3_reader.rs:26-37); lens in frames
    std::vector<std::vector<Peak>> calc_chunks_pcm16(std::uint16_t sr, const std::vector<const std::int16_t*>& haystacks,
                                                     const std::vector<std::size_t>& frames, bool scale, const Config& config,
                                                     std::size_t cap_per_haystack = 256) {
        const am_match_params p = config.params(sr, scale);
        const std::size_t k = haystacks.size();
        std::vector<am_peak> buf(k * cap_per_haystack);
        std::vector<std::size_t> n(k, 0);
        int rc = am_pool_match_batch_pcm16(p_, haystacks.data(), frames.data(), k, &p, buf.data(), cap_per_haystack, n.data());
        if (rc == AM_ERR_CAPACITY) {
            for (std::size_t v : n) cap_per_haystack = std::max(cap_per_haystack, v);
            buf.assign(k * cap_per_haystack, am_peak{});
            rc = am_pool_match_batch_pcm16(p_, haystacks.data(), frames.data(), k, &p, buf.data(), cap_per_haystack, n.data());
        }
        check(rc);
        std::vector<std::vector<Peak>> out(k);
        for (std::size_t i = 0; i < k; ++i)
            for (std::size_t j = 0; j < n[i]; ++j) {
                const am_peak& q = buf[i * cap_per_haystack + j];
                out[i].push_back(Peak{static_cast<std::size_t>(q.start), static_cast<std::size_t>(q.end), q.height, q.prominence});
            }
        return out;
    }

    // calc_chunks on ONE long haystack, its windows split over the pool's devices (audio_matcher.rs:104-131 fans the
    // windows of one haystack out; one sort + overshadow pass over the union, :132-140)
    std::vector<Peak> calc_chunks_long(std::uint16_t sr, const float* haystack, std::size_t len, bool scale, const Config& config,
                                       std::size_t cap = 4096) {
        const am_match_params p = config.params(sr, scale);
        std::vector<am_peak> buf(cap);
        std::size_t n = 0;
        int rc = am_pool_match_long(p_, haystack, len, AM_FMT_F32_MONO, &p, buf.data(), cap, &n);
        if (rc == AM_ERR_CAPACITY) {
            buf.assign(n, am_peak{});
            rc = am_pool_match_long(p_, haystack, len, AM_FMT_F32_MONO, &p, buf.data(), buf.size(), &n);
        }
        check(rc);
        std::vector<Peak> out;
        for (std::size_t j = 0; j < n; ++j)
            out.push_back(Peak{static_cast<std::size_t>(buf[j].start), static_cast<std::size_t>(buf[j].end), buf[j].height, buf[j].prominence});
        return out;
    }

private:
    am_pool* p_ = nullptr;
};

// matcher::run's file loop around SEVERAL snippets (BASELINE config 4) over every GPU: all needles
// replicated per device, the haystack's forward transform shared by the needles of a group.
class HipConvolveMultiPool {
public:
    HipConvolveMultiPool(const std::vector<std::vector<float>>& samples, const std::vector<int>& devices = {}) {
        std::vector<const float*> ptrs;
        for (const auto& v : samples) ptrs.push_back(v.data());
        check(am_pool_create_multi(ptrs.data(), ptrs.size(), samples.empty() ? 0 : samples[0].size(),
                                   devices.empty() ? nullptr : devices.data(), devices.size(), &p_));
        nn_ = samples.size();
    }
    HipConvolveMultiPool(const HipConvolveMultiPool&) = delete;
    HipConvolveMultiPool& operator=(const HipConvolveMultiPool&) = delete;
    ~HipConvolveMultiPool() { am_pool_destroy(p_); }
    // result [k][j]: haystack k against needle j; haystacks are host buffers of `sample_format`
    std::vector<std::vector<std::vector<Peak>>> calc_chunks(std::uint16_t sr, const std::vector<const void*>& haystacks,
                                                            const std::vector<std::size_t>& lens, int sample_format, bool scale,
                                                            const Config& config, std::size_t cap_per_pair = 64) {
        const am_match_params p = config.params(sr, scale);
        const std::size_t k = haystacks.size();
        std::vector<am_peak> buf(k * nn_ * cap_per_pair);
        std::vector<std::size_t> n(k * nn_, 0);
        int rc = am_pool_match_multi_batch(p_, haystacks.data(), lens.data(), k, sample_format, &p, buf.data(), cap_per_pair, n.data());
        if (rc == AM_ERR_CAPACITY) {
            for (std::size_t v : n) cap_per_pair = std::max(cap_per_pair, v);
            buf.assign(k * nn_ * cap_per_pair, am_peak{});
            rc = am_pool_match_multi_batch(p_, haystacks.data(), lens.data(), k, sample_format, &p, buf.data(), cap_per_pair, n.data());
        }
        check(rc);
        std::vector<std::vector<std::vector<Peak>>> out(k, std::vector<std::vector<Peak>>(nn_));
        for (std::size_t i = 0; i < k; ++i)
            for (std::size_t j = 0; j < nn_; ++j)
                for (std::size_t q = 0; q < n[i * nn_ + j]; ++q) {
                    const am_peak& v = buf[(i * nn_ + j) * cap_per_pair + q];
                    out[i][j].push_back(Peak{static_cast<std::size_t>(v.start), static_cast<std::size_t>(v.end), v.height, v.prominence});
                }
        return out;
    }

private:
    am_pool* p_ = nullptr;
    std::size_t nn_ = 0;
};

// Live monitoring (am_monitor_*): the final hits of one or several needles while an unbounded recording arrives
// (calc_chunks over a lazy sample source, audio_matcher.rs:88-141 / matcher/mod.rs:42-99), in bounded device memory.
struct MonitorHit {
    std::uint32_t needle = 0;
    Peak peak;
};
class HipMonitor {
public:
    // params[j] for needles[j]; sample_format AM_FMT_*; group_windows 0 means 1
    HipMonitor(const std::vector<const HipConvolve*>& needles, const std::vector<am_match_params>& params,
               int sample_format = AM_FMT_F32_MONO, std::size_t group_windows = 1) {
        std::vector<const am_needle*> hs;
        for (const HipConvolve* n : needles) hs.push_back(n->handle());
        if (params.size() != hs.size()) throw Error(AM_ERR_INVALID_ARG, "audiomatch: one am_match_params per needle");
        check(am_monitor_begin(hs.data(), hs.size(), params.data(), sample_format, group_windows, &m_));
    }
    HipMonitor(const HipMonitor&) = delete;
    HipMonitor& operator=(const HipMonitor&) = delete;
    HipMonitor(HipMonitor&& o) noexcept : m_(std::exchange(o.m_, nullptr)) {}
    ~HipMonitor() { am_monitor_destroy(m_); }
    // n samples / frames from host memory; returns the hits that became final, by (start, needle)
    std::vector<MonitorHit> push(const void* samples, std::size_t n) {
        check(am_monitor_push(m_, samples, n));
        return take(am_monitor_poll);
    }
    std::vector<MonitorHit> poll() { return take(am_monitor_poll); }
    // end of input: every hit not yet returned
    std::vector<MonitorHit> end() { return take(am_monitor_end); }
    am_monitor_info info() const {
        am_monitor_info i{};
        check(am_monitor_info_get(m_, &i));
        return i;
    }
    // am_merge_ready: how many of `sorted` are final, whatever peaks at or after `horizon` follow
    static std::size_t merge_ready(const am_match_params& p, const std::vector<am_peak>& sorted, std::uint64_t horizon, bool ended) {
        std::size_t n = 0;
        check(am_merge_ready(&p, sorted.data(), sorted.size(), horizon, ended ? 1 : 0, &n));
        return n;
    }

private:
    std::vector<MonitorHit> take(int (*fn)(am_monitor*, am_peak*, std::uint32_t*, std::size_t, std::size_t*)) {
        std::size_t n = 0;
        int rc = fn(m_, buf_.data(), idx_.data(), buf_.size(), &n);
        if (rc == AM_ERR_CAPACITY) {
            buf_.resize(n); idx_.resize(n);
            rc = fn(m_, buf_.data(), idx_.data(), buf_.size(), &n);
        }
        check(rc);
        std::vector<MonitorHit> out;
        for (std::size_t i = 0; i < n; ++i)
            out.push_back(MonitorHit{idx_[i], Peak{static_cast<std::size_t>(buf_[i].start), static_cast<std::size_t>(buf_[i].end),
                                                   buf_[i].height, buf_[i].prominence}});
        return out;
    }
    am_monitor* m_ = nullptr;
    std::vector<am_peak> buf_ = std::vector<am_peak>(64);
    std::vector<std::uint32_t> idx_ = std::vector<std::uint32_t>(64);
};

}  // namespace audiomatch
