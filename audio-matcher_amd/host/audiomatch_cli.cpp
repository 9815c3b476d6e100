// audiomatch_cli.cpp -- `audio-matcher <haystack...> --snippet <needle>...` on the GPU library:
// the per-file loop of matcher::run (src/matcher/mod.rs:17-104) with the argument surface of
// src/matcher/args.rs:9-77.  Input files are WAV (PCM16 stereo/mono or float32 mono): MP3
// decoding (minimp3) is outside the accelerated path.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <sys/stat.h>
#include <unistd.h>

#include "am_host.hpp"

using namespace amhost;

static bool file_exists(const std::string& p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }

static std::string auto_out_file(const std::string& path) {          // mod.rs:106-108: with_extension("txt")
    const auto slash = path.find_last_of('/');
    const auto dot = path.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + ".txt";
    return path.substr(0, dot) + ".txt";
}

static bool ask_consent(const Arguments& a, const std::string& question) {   // common::args::input::Inputs
    if (a.always_answer >= 0) return a.always_answer == 1;
    std::fprintf(stderr, "%s [y/n]: ", question.c_str());
    std::string line;
    if (!std::getline(std::cin, line)) return false;
    return !line.empty() && (line[0] == 'y' || line[0] == 'Y' || line[0] == 'j' || line[0] == 'J');
}

static void progress(void*, size_t k, int stage, size_t n_chunks) {          // audio_matcher.rs:102-117, 129
    std::fprintf(stderr, "Progress: file %zu %s (%zu chunks)\n", k, stage == 0 ? "started" : "finished", n_chunks);
}

static std::string base_name(const std::string& path) {
    const auto slash = path.find_last_of('/');
    return slash == std::string::npos ? path : path.substr(slash + 1);
}

// extension: --bands B[:LOG2F].  One line per hit, to follow the hit's offset line (and its --segments line): the presence
// mask of B log-spaced bands from 50 Hz to min(sr / 2, 16 kHz) ('#' present, '.' absent, at min_coherence =
// --min-confidence if given, else 0.5), coverage, weighted coherence and gain spread (am_hit_bands + am_hit_bands_summary).
static std::vector<std::string> band_lines(const Arguments& args, const am_needle* algo, const std::vector<float>& samples,
                                           std::uint32_t sr, const am_peak* peaks, size_t n) {
    std::vector<std::string> out;
    if (n == 0) return out;
    am_band_params bp{};
    if (am_band_edges_log(sr, args.band_frame_log2, 50.0, std::min(0.5 * (double)sr, 16000.0), args.bands, &bp) != AM_OK)
        throw std::runtime_error(std::string("--bands: ") + am_last_error_string());
    const float min_coh = args.min_confidence.value_or(0.5f);
    std::vector<am_hit_band> rec(n * bp.n_bands);
    if (am_hit_bands(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, &bp, rec.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_bands: ") + am_last_error_string());
    const unsigned absent = AM_HIT_NONFINITE | AM_HIT_BELOW_FLOOR | AM_HIT_EMPTY_BAND;
    for (size_t i = 0; i < n; ++i) {
        const am_hit_band* q = rec.data() + i * bp.n_bands;
        am_band_summary sm{};
        if (am_hit_bands_summary(q, bp.n_bands, min_coh, &sm) != AM_OK)
            throw std::runtime_error(std::string("am_hit_bands_summary: ") + am_last_error_string());
        std::string mask(bp.n_bands, '.');
        for (std::uint32_t b = 0; b < bp.n_bands; ++b)
            if (!(q[b].flags & absent) && q[b].coherence >= min_coh) mask[b] = '#';
        char tail[128];
        std::snprintf(tail, sizeof tail, " coverage %.3f coherence %.3f gain_db_spread %.1f", sm.coverage, sm.weighted_coherence, sm.gain_db_spread);
        out.push_back("  bands " + mask + tail);
    }
    return out;
}

// extension: --segments M[:R].  One line per hit, to follow the hit's offset line: the presence mask of the snippet's M
// parts ('#' present, '.' absent, at min_ncc = --min-confidence if given, else 0.5), coverage, drift and start lag
// (am_hit_segments + am_hit_segments_summary).
static std::vector<std::string> segment_lines(const Arguments& args, const am_needle* algo, const std::vector<float>& samples,
                                              const am_peak* peaks, size_t n) {
    std::vector<std::string> out;
    if (n == 0) return out;
    const am_segment_params sp{args.segments, args.segment_radius};
    const float min_ncc = args.min_confidence.value_or(0.5f);
    size_t s_len = 0;
    am_needle_len(algo, &s_len);
    std::vector<am_hit_segment> seg(n * sp.segments);
    if (am_hit_segments(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, &sp, seg.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_segments: ") + am_last_error_string());
    const unsigned absent = AM_HIT_NONFINITE | AM_HIT_BELOW_FLOOR | AM_HIT_EMPTY_SEGMENT;
    for (size_t i = 0; i < n; ++i) {
        const am_hit_segment* q = seg.data() + i * sp.segments;
        am_segment_summary sm{};
        if (am_hit_segments_summary(q, sp.segments, s_len, min_ncc, &sm) != AM_OK)
            throw std::runtime_error(std::string("am_hit_segments_summary: ") + am_last_error_string());
        std::string mask(sp.segments, '.');
        for (std::uint32_t j = 0; j < sp.segments; ++j)
            if (!(q[j].flags & absent) && q[j].ncc >= min_ncc) mask[j] = '#';
        char tail[128];
        std::snprintf(tail, sizeof tail, " coverage %.3f drift_ppm %.1f start_lag %.3f", sm.coverage, sm.drift_ppm, sm.start_lag);
        out.push_back("  segments " + mask + tail);
    }
    return out;
}

// extension: --warp PPM[:STEPS[:RADIUS]].  The drift records of a file's hits (am_hit_warp over the grid -PPM .. PPM),
// computed once, right after the match; of(): the records of the hits that are left after the filters (a subset in the
// same order, told apart by their starts).
struct WarpSet {
    std::vector<std::uint64_t> starts;
    std::vector<am_warp_hit> recs;

    static WarpSet compute(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, const am_peak* peaks, size_t n) {
        WarpSet ws;
        if (!args.warp_ppm || n == 0) return ws;
        ws.recs.resize(n);
        for (size_t i = 0; i < n; ++i) ws.starts.push_back(peaks[i].start);
        const am_warp_params wp{0.0, *args.warp_ppm, args.warp_steps, args.warp_radius};
        if (am_hit_warp(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, &wp, ws.recs.data()) != AM_OK)
            throw std::runtime_error(std::string("am_hit_warp: ") + am_last_error_string());
        return ws;
    }
    std::vector<am_warp_hit> of(const am_peak* peaks, size_t n) const {
        std::vector<am_warp_hit> out;
        for (size_t i = 0, k = 0; i < n && k < starts.size(); ++k)
            if (starts[k] == peaks[i].start) { out.push_back(recs[k]); ++i; }
        return out;
    }
};

// ... one line per hit, to follow the hit's offset line: drift, refined lag, the corrected NCC and the NCC as found
static std::vector<std::string> warp_lines(const std::vector<am_warp_hit>& recs) {
    std::vector<std::string> out;
    for (const am_warp_hit& w : recs) {
        char line[192];
        std::snprintf(line, sizeof line, "  warp drift_ppm %.1f lag %.3f ncc %.6f ncc_as_found %.6f%s", w.drift_ppm, w.lag, (double)w.ncc,
                      (double)w.ncc_centre, (w.flags & AM_HIT_DRIFT_UNREFINED) ? " (drift at the grid's end or unrefined)" : "");
        out.push_back(line);
    }
    return out;
}

// ... with --min-confidence: keeps the hits whose corrected NCC is at least X, in place (ws holds the records of exactly
// these n hits); returns how many are left.  With --debug one line per hit (`prefix` in front).
static size_t warp_confidence_filter(const Arguments& args, const WarpSet& ws, am_peak* peaks, size_t n, const std::string& prefix) {
    const std::vector<am_warp_hit>& w = ws.recs;
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool keep = w[i].ncc >= *args.min_confidence;   // (a NaN ncc is dropped too)
        if (args.verbosity >= 2)
            std::printf("%shit %zu: drift_ppm %.1f lag %.3f ncc %.6f ncc_as_found %.6f gain %.6g%s\n", prefix.c_str(), i + 1, w[i].drift_ppm,
                        w[i].lag, (double)w[i].ncc, (double)w[i].ncc_centre, (double)w[i].gain, keep ? "" : " (dropped)");
        if (keep) peaks[kept++] = peaks[i];
    }
    return kept;
}

// extension: --min-significance Z [--significance-zone D].  Keeps the hits whose z against their local background
// (am_hit_significance: guard = the snippet's length - 1, radius = D at the file's rate, by default three snippet
// lengths) is at least Z, in place; returns how many are left.  With --debug one line per hit (`prefix` in front).
static size_t significance_filter(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, std::uint32_t sr,
                                  am_peak* peaks, size_t n, const std::string& prefix) {
    if (n == 0) return 0;
    size_t s_len = 0;
    am_needle_len(algo, &s_len);
    am_significance_params sp{};
    sp.guard = s_len - 1;
    sp.radius = args.significance_zone_ms ? (*args.significance_zone_ms * sr + 999) / 1000
                                          : std::min<std::uint64_t>(3 * (std::uint64_t)s_len, AM_SIG_MAX_RADIUS);
    std::vector<am_significance> sg(n);
    if (am_hit_significance(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, &sp, sg.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_significance: ") + am_last_error_string());
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool keep = sg[i].z >= *args.min_significance;   // (a NaN z -- no background, a non-finite sample -- is dropped too)
        if (args.verbosity >= 2)
            std::printf("%shit %zu: score %.6f mean %.6f std %.6f z %.2f side_max %.6f lag %d%s\n", prefix.c_str(), i + 1,
                        (double)sg[i].score, (double)sg[i].bg_mean, (double)sg[i].bg_std, (double)sg[i].z, (double)sg[i].side_max,
                        (int)sg[i].side_lag, keep ? "" : " (dropped)");
        if (keep) peaks[kept++] = peaks[i];
    }
    return kept;
}

// extension: --learn-needle OUT.wav[:METHOD] [--learn-margin D].  The reported hits of every main file, each as one row
// cut while its file is in memory (am_hit_window: scale = 1 / gain of am_hit_scores, the margin in front and behind);
// at the end of the run one am_needle_estimate_rows over the rows, the estimate written as a mono float WAV and one line
// per second of it with the mean of dev / max|est|.
struct Learner {
    struct Row { float ncc; std::vector<float> v; };
    std::vector<Row> rows;          // in the order the hits were reported; once over the cap, the best by NCC, best first
    std::uint32_t sr = 0;           // the main files' rate
    std::uint64_t length = 0;       // elements per row
    bool capped = false;

    size_t cap(const Arguments& args) const { return args.learn_method == AM_EST_MEAN ? 65535 : AM_EST_MAX_HITS; }

    // w: with --warp, the drift records of these n hits
    void take(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, std::uint32_t m_sr, const am_peak* peaks, size_t n,
              const std::vector<am_warp_hit>& w) {
        if (n == 0) return;
        size_t s_len = 0;
        am_needle_len(algo, &s_len);
        const std::uint64_t lead = round_samples_ms(args.learn_margin_ms.value_or(0), m_sr), len = s_len + 2 * lead;
        if (rows.empty() && !capped) { sr = m_sr; length = len; }
        if (m_sr != sr || len != length) throw std::runtime_error("--learn-needle: the main files must share one sample rate");
        // with --warp: gain, NCC, lag and drift of am_hit_warp, the row cut on the snippet's clock (am_hit_window_warped)
        std::vector<am_hit_score> sc(args.warp_ppm ? 0 : n);
        if (!args.warp_ppm && am_hit_scores(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, sc.data()) != AM_OK)
            throw std::runtime_error(std::string("am_hit_scores: ") + am_last_error_string());
        for (size_t i = 0; i < n; ++i) {
            const std::uint32_t flags = args.warp_ppm ? w[i].flags : sc[i].flags;
            const float gain = args.warp_ppm ? w[i].gain : sc[i].gain;
            if ((flags & (AM_HIT_NONFINITE | AM_HIT_BELOW_FLOOR | AM_HIT_EMPTY_SEGMENT)) || !(gain > 0.0f)) continue;
            const float scale = 1.0f / gain;
            if (!std::isfinite(scale)) continue;
            Row r{args.warp_ppm ? w[i].ncc : sc[i].ncc, std::vector<float>((size_t)length)};
            if (args.warp_ppm) {
                if (am_hit_window_warped(samples.data(), samples.size(), AM_FMT_F32_MONO, peaks[i].start, scale, w[i].lag, w[i].drift_ppm, lead,
                                         length, r.v.data()) != AM_OK)
                    throw std::runtime_error(std::string("am_hit_window_warped: ") + am_last_error_string());
            } else if (am_hit_window(samples.data(), samples.size(), AM_FMT_F32_MONO, peaks[i].start, scale, lead, length, r.v.data()) != AM_OK) {
                throw std::runtime_error(std::string("am_hit_window: ") + am_last_error_string());
            }
            rows.push_back(std::move(r));
        }
        if (rows.size() > cap(args)) {
            std::stable_sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.ncc > b.ncc; });
            rows.resize(cap(args));
            capped = true;
        }
    }

    int finish(const Arguments& args) const {
        if (rows.empty()) {
            std::fprintf(stderr, "--learn-needle: no usable hit, '%s' not written\n", args.learn_needle.c_str());
            return 5;
        }
        if (capped)
            std::fprintf(stderr, "--learn-needle: more than %zu usable hits, the %zu of highest NCC are used\n", cap(args), cap(args));
        std::vector<float> flat(rows.size() * (size_t)length), est((size_t)length), dev((size_t)length);
        for (size_t i = 0; i < rows.size(); ++i) std::copy(rows[i].v.begin(), rows[i].v.end(), flat.begin() + (std::ptrdiff_t)(i * (size_t)length));
        const am_estimate_params ep{args.learn_method, args.learn_trim, 0, length};
        if (am_needle_estimate_rows(args.device, flat.data(), rows.size(), &ep, est.data(), dev.data(), nullptr) != AM_OK)
            throw std::runtime_error(std::string("am_needle_estimate_rows: ") + am_last_error_string());
        write_wav_f32(args.learn_needle, est, sr);
        if (args.verbosity >= 1) {
            float peak = 0.0f;
            for (float v : est) peak = std::max(peak, std::fabs(v));
            std::printf("learned needle: %zu hits, %" PRIu64 " samples at %u Hz -> '%s'\n", rows.size(), length, sr, args.learn_needle.c_str());
            for (std::uint64_t t0 = 0, k = 0; t0 < length; t0 += sr, ++k) {
                const std::uint64_t t1 = std::min<std::uint64_t>(length, t0 + sr);
                double sum = 0.0;
                for (std::uint64_t t = t0; t < t1; ++t) sum += dev[(size_t)t];
                std::printf("  second %" PRIu64 ": spread %.4f\n", k, peak > 0.0f ? sum / (double)(t1 - t0) / (double)peak : 0.0);
            }
        }
        return 0;
    }
};

// extension: --whiten P / --preemphasis A.  The taps of the ONE filter every snippet and every main file of the run passes
// through before matching (empty: none).  --whiten: the lag products of all main files are added (am_lag_products), the
// filter is their prediction-error filter of order P with noise_db 60 (am_whiten_taps); --preemphasis: {1, -A}.
static std::vector<float> filter_taps(const Arguments& args) {
    if (args.preemphasis) return {1.0f, -*args.preemphasis};
    if (!args.whiten) return {};
    std::vector<double> r(args.whiten + 1, 0.0), part(args.whiten + 1);
    for (const std::string& main_file : args.within) {
        const std::vector<float> x = to_mono_f32(read_wav(main_file), args.device);
        if (am_lag_products(args.device, x.data(), x.size(), AM_FMT_F32_MONO, args.whiten, part.data()) != AM_OK)
            throw std::runtime_error(std::string("am_lag_products: ") + am_last_error_string());
        for (size_t k = 0; k < r.size(); ++k) r[k] += part[k];
    }
    std::vector<float> taps(args.whiten + 1);
    if (am_whiten_taps(r.data(), args.whiten, 60.0, taps.data()) != AM_OK)
        throw std::runtime_error(std::string("am_whiten_taps: ") + am_last_error_string());
    if (args.verbosity >= 2) {
        std::printf("whitening filter:");
        for (float t : taps) std::printf(" %.6g", (double)t);
        std::printf("\n");
    }
    return taps;
}

// x through the run's filter (am_fir); without one, x itself
static std::vector<float> filtered(const Arguments& args, std::vector<float> x, const std::vector<float>& taps) {
    if (taps.empty() || x.empty()) return x;
    std::vector<float> y(x.size());
    size_t n = 0;
    if (am_fir(args.device, x.data(), x.size(), AM_FMT_F32_MONO, taps.data(), (std::uint32_t)taps.size(), 0, y.data(), y.size(), &n) != AM_OK)
        throw std::runtime_error(std::string("am_fir: ") + am_last_error_string());
    return y;
}

// The handle of a snippet (rate sr) for main files of rate m_sr: resampled when the rates differ (--resample), then
// passed through the run's filter, if any.
static am_needle* make_needle(const Arguments& args, const std::vector<float>& data, std::uint32_t sr, std::uint32_t m_sr,
                              const std::vector<float>& taps) {
    am_needle* h = nullptr;
    if (taps.empty()) {
        if (sr == m_sr) {
            if (am_needle_create(args.device, data.data(), data.size(), &h) != AM_OK)
                throw std::runtime_error(std::string("am_needle_create: ") + am_last_error_string());
        } else if (am_needle_create_resampled(args.device, data.data(), data.size(), AM_FMT_F32_MONO, sr, m_sr, &h) != AM_OK) {
            throw std::runtime_error(std::string("am_needle_create_resampled: ") + am_last_error_string());
        }
        return h;
    }
    std::vector<float> at_rate;
    if (sr != m_sr) {
        size_t n = 0;
        if (am_resample_len(data.size(), sr, m_sr, &n) != AM_OK) throw std::runtime_error(std::string("am_resample_len: ") + am_last_error_string());
        at_rate.resize(n);
        if (am_resample(args.device, data.data(), data.size(), AM_FMT_F32_MONO, sr, m_sr, at_rate.data(), at_rate.size(), &n) != AM_OK)
            throw std::runtime_error(std::string("am_resample: ") + am_last_error_string());
    }
    const std::vector<float>& x = sr != m_sr ? at_rate : data;
    if (am_needle_create_filtered(args.device, x.data(), x.size(), AM_FMT_F32_MONO, taps.data(), (std::uint32_t)taps.size(), &h) != AM_OK)
        throw std::runtime_error(std::string("am_needle_create_filtered: ") + am_last_error_string());
    return h;
}

// extension: several --snippet files.  Each main file is matched by ONE am_match_multi_varlen call (the snippets may
// differ in length: each uses an overlap of its own length at the main file's rate, as make_params does for one);
// with --normalize, which that call refuses, snippet by snippet with am_match.  The label file is timelabel_from_peaks
// over the hits of all snippets, sorted by start (equal starts in --snippet order).
static int run_multi(const Arguments& args) {
    struct Snip {
        std::string name;
        std::uint32_t sr = 0;
        double duration = 0.0;
        std::vector<float> data;
        am_needle* h = nullptr;
        std::map<std::uint32_t, am_needle*> resampled;
    };
    std::vector<Snip> snips(args.snippets.size());
    auto release = [&]() {
        for (Snip& sn : snips) {
            if (sn.h) am_needle_destroy(sn.h);
            for (auto& kv : sn.resampled) am_needle_destroy(kv.second);
        }
    };
    try {
        if (args.normalize_floor_db && am_set_option("score_norm_floor_db", *args.normalize_floor_db) != AM_OK)
            throw std::runtime_error(std::string("--normalize-floor: ") + am_last_error_string());
        const std::vector<float> taps = filter_taps(args);   // extension: --whiten / --preemphasis
        for (size_t j = 0; j < snips.size(); ++j) {
            Snip& sn = snips[j];
            const Pcm pcm = read_wav(args.snippets[j]);
            sn.name = base_name(args.snippets[j]);
            sn.sr = pcm.sample_rate;
            sn.duration = (double)pcm.frames() / (double)sn.sr;
            sn.data = to_mono_f32(pcm, args.device);
            sn.h = make_needle(args, sn.data, sn.sr, sn.sr, taps);
            if (args.normalize && am_needle_set_option(sn.h, "score_norm", 1) != AM_OK)
                throw std::runtime_error(std::string("--normalize: ") + am_last_error_string());
        }
        if (args.verbosity >= 2) am_set_progress_callback(progress, nullptr);
        int rc_all = 0;
        for (const std::string& main_file : args.within) {
            std::optional<std::string> out_path = args.out_file;
            if (!out_path && !args.no_out) out_path = auto_out_file(main_file);
            if (out_path && file_exists(*out_path)) {
                if (args.skip_existing ||
                    ask_consent(args, "Ausgabe Datei \"" + *out_path + "\" existiert bereits, möchtest du skippen"))
                    continue;
                if (!ask_consent(args, "soll die existierende Datei überschrieben werden")) out_path.reset();
            }
            if (args.verbosity >= (args.within.size() == 1 ? 3 : 1))
                std::printf("preparing data of '%s'\n", main_file.c_str());
            const Pcm m = read_wav(main_file);
            const std::uint32_t m_sr = m.sample_rate;
            const size_t k = snips.size();
            std::vector<const am_needle*> handles(k);
            std::vector<std::uint64_t> overlaps(k);
            for (size_t j = 0; j < k; ++j) {
                Snip& sn = snips[j];
                if (m_sr != sn.sr && !args.resample) {
                    std::fprintf(stderr, "sample rate of snippet (%u) and main file (%u) don't match\n", sn.sr, m_sr);
                    release();
                    return 3;
                }
                am_needle* algo = sn.h;
                overlaps[j] = make_params(args, m_sr, sn.duration).overlap;
                if (m_sr != sn.sr) {
                    am_needle*& h = sn.resampled[m_sr];
                    if (!h) {
                        h = make_needle(args, sn.data, sn.sr, m_sr, taps);
                        if (args.normalize && am_needle_set_option(h, "score_norm", 1) != AM_OK)
                            throw std::runtime_error(std::string("--normalize: ") + am_last_error_string());
                    }
                    algo = h;
                    size_t s_len = 0;   // the overlap = the resampled snippet's length
                    am_needle_len(algo, &s_len);
                    overlaps[j] = s_len;
                }
                handles[j] = algo;
            }
            const std::vector<float> m_samples = filtered(args, to_mono_f32(m, args.device), taps);
            const am_match_params p = make_params(args, m_sr, snips[0].duration);
            size_t cap = 1024;
            std::vector<am_peak> peaks(cap * k);
            std::vector<size_t> n(k, 0);
            if (args.best) {   // extension: --best N, one am_match_best per snippet
                std::vector<std::vector<am_peak>> each(k);
                for (size_t j = 0; j < k; ++j) {
                    each[j] = best_hits(args, handles[j], m_samples, m_sr);
                    n[j] = each[j].size();
                    cap = std::max(cap, n[j]);
                }
                peaks.assign(cap * k, am_peak{});
                for (size_t j = 0; j < k; ++j) std::copy(each[j].begin(), each[j].end(), peaks.begin() + (std::ptrdiff_t)(j * cap));
            } else if (!args.normalize) {
                int rc = am_match_multi_varlen(handles.data(), k, overlaps.data(), m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, &p,
                                               peaks.data(), cap, n.data());
                if (rc == AM_ERR_CAPACITY) {
                    for (size_t j = 0; j < k; ++j) cap = std::max(cap, n[j]);
                    peaks.assign(cap * k, am_peak{});
                    rc = am_match_multi_varlen(handles.data(), k, overlaps.data(), m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, &p,
                                               peaks.data(), cap, n.data());
                }
                if (rc != AM_OK) throw std::runtime_error(std::string("am_match_multi_varlen: ") + am_last_error_string());
            } else {
                std::vector<std::vector<am_peak>> each(k);
                for (size_t j = 0; j < k; ++j) {
                    am_match_params pj = p;
                    pj.overlap = overlaps[j];
                    each[j].resize(1024);
                    int rc = am_match(handles[j], m_samples.data(), m_samples.size(), &pj, each[j].data(), each[j].size(), &n[j]);
                    if (rc == AM_ERR_CAPACITY) {
                        each[j].resize(n[j]);
                        rc = am_match(handles[j], m_samples.data(), m_samples.size(), &pj, each[j].data(), each[j].size(), &n[j]);
                    }
                    if (rc != AM_OK) throw std::runtime_error(std::string("am_match: ") + am_last_error_string());
                    cap = std::max(cap, n[j]);
                }
                peaks.assign(cap * k, am_peak{});
                for (size_t j = 0; j < k; ++j) std::copy(each[j].begin(), each[j].begin() + (std::ptrdiff_t)n[j], peaks.begin() + (std::ptrdiff_t)(j * cap));
            }
            for (size_t j = 0; j < k; ++j) {
                am_peak* pk = peaks.data() + j * cap;
                const WarpSet warp = WarpSet::compute(args, handles[j], m_samples, pk, n[j]);   // extension: --warp
                if (args.min_confidence && args.warp_ppm && n[j] > 0) {   // ... the corrected NCC decides
                    n[j] = warp_confidence_filter(args, warp, pk, n[j], snips[j].name + ": ");
                } else if (args.min_confidence && n[j] > 0) {   // each snippet's hits scored with that snippet's handle
                    std::vector<am_hit_score> sc(n[j]);
                    if (am_hit_scores(handles[j], m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, pk, n[j], sc.data()) != AM_OK)
                        throw std::runtime_error(std::string("am_hit_scores: ") + am_last_error_string());
                    size_t kept = 0;
                    for (size_t i = 0; i < n[j]; ++i) {
                        if (args.verbosity >= 2)
                            std::printf("%s: hit %zu: position %.3f ncc %.6f gain %.6g window %.2f dB%s\n", snips[j].name.c_str(), i + 1,
                                        sc[i].position, (double)sc[i].ncc, (double)sc[i].gain, (double)sc[i].window_db,
                                        sc[i].ncc >= *args.min_confidence ? "" : " (dropped)");
                        if (sc[i].ncc >= *args.min_confidence) pk[kept++] = pk[i];
                    }
                    n[j] = kept;
                }
                if (args.min_significance) n[j] = significance_filter(args, handles[j], m_samples, m_sr, pk, n[j], snips[j].name + ": ");
                if (args.verbosity >= 1) {
                    const std::vector<std::string> lines = offset_lines(pk, n[j], m_sr);
                    const std::vector<std::string> segs =
                        args.segments ? segment_lines(args, handles[j], m_samples, pk, n[j]) : std::vector<std::string>();
                    const std::vector<std::string> bands =
                        args.bands ? band_lines(args, handles[j], m_samples, m_sr, pk, n[j]) : std::vector<std::string>();
                    const std::vector<std::string> warps =
                        args.warp_ppm ? warp_lines(warp.of(pk, n[j])) : std::vector<std::string>();   // extension: --warp
                    for (size_t i = 0; i < lines.size(); ++i) {
                        std::printf("%s: %s\n", snips[j].name.c_str(), lines[i].c_str());
                        if (i < warps.size()) std::printf("%s: %s\n", snips[j].name.c_str(), warps[i].c_str());
                        if (i < segs.size()) std::printf("%s: %s\n", snips[j].name.c_str(), segs[i].c_str());
                        if (i < bands.size()) std::printf("%s: %s\n", snips[j].name.c_str(), bands[i].c_str());
                    }
                }
            }
            if (out_path) {
                std::vector<std::pair<std::uint64_t, size_t>> order;   // (start, slot): sorted by start, then snippet, then position
                for (size_t j = 0; j < k; ++j)
                    for (size_t i = 0; i < n[j]; ++i) order.emplace_back(peaks[j * cap + i].start, j * cap + i);
                std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
                std::vector<am_peak> merged;
                for (const auto& o : order) merged.push_back(peaks[o.second]);
                const std::string text = format_labels(timelabel_from_peaks(merged.data(), merged.size(), m_sr, 7.0, "Segment #"));
                if (args.dry_run) {
                    std::printf("would write to '%s':\n%s", out_path->c_str(), text.c_str());
                } else {
                    std::ofstream f(*out_path, std::ios::binary | std::ios::trunc);
                    if (!f) { std::fprintf(stderr, "couldn't find file '%s'\n", out_path->c_str()); rc_all = 4; continue; }
                    f << text;
                }
            }
        }
        release();
        return rc_all;
    } catch (const std::exception& e) {
        release();
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// extension: --live.  Raw PCM from stdin through one monitor (am_monitor_*, all snippets in it): every chunk of input is
// turned into the f32 mono samples the file mode would have made of the same frames (to_mono_f32), pushed, and the hits
// that became final are printed at once, numbered per snippet as the file mode numbers them.  At end of input the
// label file is written exactly as the file mode writes it for that recording (timelabel_from_peaks over the hits of
// all snippets by start, equal starts in --snippet order: the monitor's own order).
static int run_live(const Arguments& args) {
    struct Snip {
        std::string name;
        am_needle* h = nullptr;
        am_needle* resampled = nullptr;
        am_match_params p{};
        size_t hits = 0;
    };
    const std::uint32_t sr = args.rate;
    const size_t k = args.snippets.size();
    std::vector<Snip> snips(k);
    am_monitor* mon = nullptr;
    auto release = [&]() {
        if (mon) am_monitor_destroy(mon);
        for (Snip& sn : snips) {
            if (sn.h) am_needle_destroy(sn.h);
            if (sn.resampled) am_needle_destroy(sn.resampled);
        }
    };
    try {
        std::vector<const am_needle*> handles(k);
        std::vector<am_match_params> params(k);
        for (size_t j = 0; j < k; ++j) {
            Snip& sn = snips[j];
            const Pcm pcm = read_wav(args.snippets[j]);
            sn.name = base_name(args.snippets[j]);
            const double duration = (double)pcm.frames() / (double)pcm.sample_rate;
            const std::vector<float> data = to_mono_f32(pcm, args.device);
            if (am_needle_create(args.device, data.data(), data.size(), &sn.h) != AM_OK)
                throw std::runtime_error(std::string("am_needle_create: ") + am_last_error_string());
            sn.p = make_params(args, sr, duration);
            handles[j] = sn.h;
            if (pcm.sample_rate != sr) {
                if (!args.resample) {
                    std::fprintf(stderr, "sample rate of snippet (%u) and main file (%u) don't match\n", pcm.sample_rate, sr);
                    release();
                    return 3;
                }
                if (am_needle_create_resampled(args.device, data.data(), data.size(), AM_FMT_F32_MONO, pcm.sample_rate, sr, &sn.resampled) != AM_OK)
                    throw std::runtime_error(std::string("am_needle_create_resampled: ") + am_last_error_string());
                size_t s_len = 0;   // the overlap = the resampled snippet's length
                am_needle_len(sn.resampled, &s_len);
                sn.p.overlap = s_len;
                handles[j] = sn.resampled;
            }
            params[j] = sn.p;
        }
        if (am_monitor_begin(handles.data(), k, params.data(), AM_FMT_F32_MONO, 1, &mon) != AM_OK)
            throw std::runtime_error(std::string("am_monitor_begin: ") + am_last_error_string());
        std::vector<am_peak> all;            // every hit, in the monitor's order: (start, snippet)
        std::vector<am_peak> got(256);
        std::vector<std::uint32_t> which(256);
        auto report = [&](size_t n) {
            for (size_t i = 0; i < n; ++i) {
                Snip& sn = snips[which[i]];
                if (args.verbosity >= 1) {
                    const std::string line = offset_line(got[i], sn.hits, sr);
                    if (k > 1) std::printf("%s: %s\n", sn.name.c_str(), line.c_str());
                    else std::printf("%s\n", line.c_str());
                }
                ++sn.hits;
                all.push_back(got[i]);
            }
            std::fflush(stdout);
        };
        auto take = [&](int (*fn)(am_monitor*, am_peak*, std::uint32_t*, size_t, size_t*), const char* what) {
            size_t n = 0;
            int rc = fn(mon, got.data(), which.data(), got.size(), &n);
            if (rc == AM_ERR_CAPACITY) {
                got.resize(n); which.resize(n);
                rc = fn(mon, got.data(), which.data(), got.size(), &n);
            }
            if (rc != AM_OK) throw std::runtime_error(std::string(what) + ": " + am_last_error_string());
            report(n);
        };
        // stdin in pieces as they come (read(2): a pipe hands over what it holds), whole frames only
        const size_t in_frame = (args.encoding == "f32le" ? 4u : 2u) * (size_t)args.channels;
        std::vector<char> raw((size_t)1 << 16);
        size_t have = 0;
        Pcm piece;
        piece.sample_rate = sr;
        piece.channels = (std::uint16_t)args.channels;
        piece.is_float = args.encoding == "f32le";
        for (;;) {
            const ssize_t got_bytes = ::read(0, raw.data() + have, raw.size() - have);
            if (got_bytes < 0) throw std::runtime_error("reading stdin failed");
            if (got_bytes == 0) break;
            have += (size_t)got_bytes;
            const size_t frames = have / in_frame;
            if (frames == 0) continue;
            if (piece.is_float) {
                piece.f32.resize(frames);
                std::memcpy(piece.f32.data(), raw.data(), frames * 4);
            } else {
                piece.s16.resize(frames * (size_t)args.channels);
                std::memcpy(piece.s16.data(), raw.data(), frames * in_frame);
            }
            const std::vector<float> mono = to_mono_f32(piece, args.device);
            if (am_monitor_push(mon, mono.data(), mono.size()) != AM_OK)
                throw std::runtime_error(std::string("am_monitor_push: ") + am_last_error_string());
            take(am_monitor_poll, "am_monitor_poll");
            std::memmove(raw.data(), raw.data() + frames * in_frame, have - frames * in_frame);
            have -= frames * in_frame;
        }
        take(am_monitor_end, "am_monitor_end");
        if (args.verbosity >= 1)
            for (const Snip& sn : snips)
                if (sn.hits == 0) {
                    if (k > 1) std::printf("%s: no offsets found\n", sn.name.c_str());
                    else std::printf("no offsets found\n");
                }
        std::fflush(stdout);
        int rc_all = 0;
        if (args.out_file && !args.no_out) {
            const std::string text = format_labels(timelabel_from_peaks(all.data(), all.size(), sr, 7.0, "Segment #"));
            if (args.dry_run) {
                std::printf("would write to '%s':\n%s", args.out_file->c_str(), text.c_str());
            } else {
                std::ofstream f(*args.out_file, std::ios::binary | std::ios::trunc);
                if (!f) { std::fprintf(stderr, "couldn't find file '%s'\n", args.out_file->c_str()); rc_all = 4; }
                else f << text;
            }
        }
        release();
        return rc_all;
    } catch (const std::exception& e) {
        release();
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

int main(int argc, char** argv) {
    Arguments args;
    try {
        args = parse_arguments(argc, argv);
    } catch (const ArgError& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    if (args.help) {
        std::printf("%s", usage_text());
        return 0;
    }
    if (args.live) return run_live(args);
    if (args.snippets.size() > 1) return run_multi(args);
    try {
        const Pcm snippet = read_wav(args.snippet);                           // mod.rs:29
        const std::uint32_t sr = snippet.sample_rate;
        const double s_duration = (double)snippet.frames() / (double)sr;      // mod.rs:30 (mp3_duration)
        const std::vector<float> sample_data = to_mono_f32(snippet, args.device);   // mod.rs:32
        const std::vector<float> taps = filter_taps(args);                    // extension: --whiten / --preemphasis
        am_needle* snippet_algo = make_needle(args, sample_data, sr, sr, taps);   // mod.rs:34: LibConvolve::new
        if (args.normalize_floor_db && am_set_option("score_norm_floor_db", *args.normalize_floor_db) != AM_OK)
            throw std::runtime_error(std::string("--normalize-floor: ") + am_last_error_string());
        if (args.normalize && am_needle_set_option(snippet_algo, "score_norm", 1) != AM_OK)
            throw std::runtime_error(std::string("--normalize: ") + am_last_error_string());
        // extension --resample: one handle per main-file rate other than the snippet's, made on first use and kept
        std::map<std::uint32_t, am_needle*> resampled;
        if (args.verbosity >= 2) am_set_progress_callback(progress, nullptr);
        int rc_all = 0;
        Learner learner;                                                      // extension: --learn-needle
        for (const std::string& main_file : args.within) {                    // mod.rs:42
            std::optional<std::string> out_path = args.out_file;
            if (!out_path && !args.no_out) out_path = auto_out_file(main_file);
            if (out_path && file_exists(*out_path)) {                         // mod.rs:48-66
                if (args.skip_existing ||
                    ask_consent(args, "Ausgabe Datei \"" + *out_path + "\" existiert bereits, möchtest du skippen"))
                    continue;
                if (!ask_consent(args, "soll die existierende Datei überschrieben werden")) out_path.reset();
            }
            if (args.verbosity >= (args.within.size() == 1 ? 3 : 1))
                std::printf("preparing data of '%s'\n", main_file.c_str());
            const Pcm m = read_wav(main_file);                                // mod.rs:71
            am_needle* algo = snippet_algo;
            if (m.sample_rate != sr && !args.resample) {                      // mod.rs:72-74 SampleRateMismatch
                std::fprintf(stderr, "sample rate of snippet (%u) and main file (%u) don't match\n", sr, m.sample_rate);
                return 3;
            }
            if (m.sample_rate != sr) {                                        // extension: --resample
                am_needle*& h = resampled[m.sample_rate];
                if (!h) {
                    h = make_needle(args, sample_data, sr, m.sample_rate, taps);
                    if (args.normalize && am_needle_set_option(h, "score_norm", 1) != AM_OK)
                        throw std::runtime_error(std::string("--normalize: ") + am_last_error_string());
                }
                algo = h;
            }
            const std::uint32_t m_sr = m.sample_rate;
            const std::vector<float> m_samples = filtered(args, to_mono_f32(m, args.device), taps);
            am_match_params p = make_params(args, m_sr, s_duration);          // mod.rs:81-87
            if (m_sr != sr) {                                                 // the overlap = the resampled snippet's length
                size_t s_len = 0;
                am_needle_len(algo, &s_len);
                p.overlap = s_len;
            }
            std::vector<am_peak> peaks(1024);
            size_t n = 0;
            if (args.best) {                                                  // extension: --best N
                peaks = best_hits(args, algo, m_samples, m_sr);
                n = peaks.size();
            } else {
                int rc = am_match(algo, m_samples.data(), m_samples.size(), &p, peaks.data(), peaks.size(), &n);
                if (rc == AM_ERR_CAPACITY) {
                    peaks.resize(n);
                    rc = am_match(algo, m_samples.data(), m_samples.size(), &p, peaks.data(), peaks.size(), &n);
                }
                if (rc != AM_OK) throw std::runtime_error(std::string("am_match: ") + am_last_error_string());
            }
            const WarpSet warp = WarpSet::compute(args, algo, m_samples, peaks.data(), n);   // extension: --warp
            if (args.min_confidence && args.warp_ppm && n > 0) {              // ... the corrected NCC decides
                n = warp_confidence_filter(args, warp, peaks.data(), n, "");
            } else if (args.min_confidence && n > 0) {                        // extension: --min-confidence
                std::vector<am_hit_score> sc(n);
                if (am_hit_scores(algo, m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, peaks.data(), n, sc.data()) != AM_OK)
                    throw std::runtime_error(std::string("am_hit_scores: ") + am_last_error_string());
                size_t kept = 0;
                for (size_t i = 0; i < n; ++i) {
                    if (args.verbosity >= 2)
                        std::printf("hit %zu: position %.3f ncc %.6f gain %.6g window %.2f dB%s\n", i + 1, sc[i].position,
                                    (double)sc[i].ncc, (double)sc[i].gain, (double)sc[i].window_db,
                                    sc[i].ncc >= *args.min_confidence ? "" : " (dropped)");
                    if (sc[i].ncc >= *args.min_confidence) peaks[kept++] = peaks[i];   // (a NaN ncc is dropped too)
                }
                n = kept;
            }
            if (args.min_significance) n = significance_filter(args, algo, m_samples, m_sr, peaks.data(), n, "");   // extension: --min-significance
            if (!args.learn_needle.empty()) learner.take(args, algo, m_samples, m_sr, peaks.data(), n, warp.of(peaks.data(), n));           // extension: --learn-needle
            if (args.verbosity >= 1) {
                const std::vector<std::string> lines = offset_lines(peaks.data(), n, m_sr);                       // mod.rs:89
                const std::vector<std::string> segs =
                    args.segments ? segment_lines(args, algo, m_samples, peaks.data(), n) : std::vector<std::string>();   // extension: --segments
                const std::vector<std::string> bands =
                    args.bands ? band_lines(args, algo, m_samples, m_sr, peaks.data(), n) : std::vector<std::string>();   // extension: --bands
                const std::vector<std::string> warps =
                    args.warp_ppm ? warp_lines(warp.of(peaks.data(), n)) : std::vector<std::string>();   // extension: --warp
                for (size_t i = 0; i < lines.size(); ++i) {
                    std::printf("%s\n", lines[i].c_str());
                    if (i < warps.size()) std::printf("%s\n", warps[i].c_str());
                    if (i < segs.size()) std::printf("%s\n", segs[i].c_str());
                    if (i < bands.size()) std::printf("%s\n", bands[i].c_str());
                }
            }
            if (out_path) {                                                   // mod.rs:92-99
                const std::string text = format_labels(timelabel_from_peaks(peaks.data(), n, m_sr, 7.0, "Segment #"));
                if (args.dry_run) {
                    std::printf("would write to '%s':\n%s", out_path->c_str(), text.c_str());
                } else {
                    std::ofstream f(*out_path, std::ios::binary | std::ios::trunc);
                    if (!f) { std::fprintf(stderr, "couldn't find file '%s'\n", out_path->c_str()); rc_all = 4; continue; }
                    f << text;
                }
            }
        }
        if (!args.learn_needle.empty()) {
            const int rc = learner.finish(args);
            if (rc) rc_all = rc;
        }
        am_needle_destroy(snippet_algo);
        for (auto& kv : resampled) am_needle_destroy(kv.second);
        return rc_all;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
