// audiomatch_cli.cpp -- `audio-matcher <haystack...> --snippet <needle>...` on the GPU library:
// the per-file loop of matcher::run (src/matcher/mod.rs:17-104) with the argument surface of
// src/matcher/args.rs:9-77.  Input files are WAV (PCM16 stereo/mono or float32 mono): MP3
// decoding (minimp3) is outside the accelerated path.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <memory>
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

// Owners of the library's handles: however a scope is left (return, continue, exception), its handles are destroyed.
struct NeedleDeleter { void operator()(am_needle* h) const { am_needle_destroy(h); } };
struct MonitorDeleter { void operator()(am_monitor* m) const { am_monitor_destroy(m); } };
using Needle = std::unique_ptr<am_needle, NeedleDeleter>;
using Monitor = std::unique_ptr<am_monitor, MonitorDeleter>;

// exact NCC, gain and position of n hits of a main file (--min-confidence, --learn-needle)
static std::vector<am_hit_score> hit_scores(const am_needle* algo, const std::vector<float>& samples, const am_peak* peaks, size_t n) {
    std::vector<am_hit_score> sc(n);
    if (am_hit_scores(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, sc.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_scores: ") + am_last_error_string());
    return sc;
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

// extension: --ignore.  The records of the hits of a masked snippet (am_hit_mask): the exact NCC, gain and level over the
// kept part, and what the ignored spans hold against the snippet's own samples there.
static std::vector<am_mask_hit> mask_records(const am_needle* algo, const std::vector<float>& samples, const am_peak* peaks, size_t n) {
    std::vector<am_mask_hit> rec(n);
    if (n > 0 && am_hit_mask(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, rec.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_mask: ") + am_last_error_string());
    return rec;
}

// ... --mask-report: one line per hit, to follow the hit's offset line
static std::vector<std::string> mask_lines(const std::vector<am_mask_hit>& recs) {
    std::vector<std::string> out;
    for (const am_mask_hit& q : recs) {
        char line[256];
        std::snprintf(line, sizeof line, "  mask ncc %.6f gain %.6f kept_db %.2f ncc_gaps %.6f gaps_db %.2f flags %u%s%s%s%s", (double)q.ncc, (double)q.gain,
                      (double)q.kept_db, (double)q.ncc_gaps, (double)q.gaps_db, (unsigned)q.flags,
                      (q.flags & AM_MASK_BELOW_FLOOR) ? " (below the floor)" : "", (q.flags & AM_MASK_NONFINITE) ? " (non-finite samples)" : "",
                      (q.flags & AM_MASK_GAPS_SILENT) ? " (silence in the ignored spans)" : "",
                      (q.flags & AM_MASK_GAPS_NONFINITE) ? " (non-finite samples in the ignored spans)" : "");
        out.push_back(line);
    }
    return out;
}

// ... --min-confidence X with --ignore.  am_hit_scores reads the whole window, ignored spans included, and would drop
// exactly the occurrences the mask is there for: the filter takes am_hit_mask's NCC over the kept part instead (also
// with --warp).  Keeps the hits whose masked NCC is at least X, in place; returns how many are left.  With --debug one
// line per hit (`prefix` in front).
static size_t mask_confidence_filter(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, am_peak* peaks, size_t n,
                                     const std::string& prefix) {
    const std::vector<am_mask_hit> rec = mask_records(algo, samples, peaks, n);
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool keep = rec[i].ncc >= *args.min_confidence;   // (a NaN ncc is dropped too)
        if (args.verbosity >= 2)
            std::printf("%shit %zu: masked ncc %.6f gain %.6g kept %.2f dB%s\n", prefix.c_str(), i + 1, (double)rec[i].ncc, (double)rec[i].gain,
                        (double)rec[i].kept_db, keep ? "" : " (dropped)");
        if (keep) peaks[kept++] = peaks[i];
    }
    return kept;
}

// extension: --channel P[:NOISE_DB].  The records and the taps of the printed hits (am_hit_channel): what each hit went
// through on its way into the recording.
struct ChannelSet {
    std::uint32_t radius = 0;
    std::vector<am_channel_hit> recs;
    std::vector<float> taps;   // hit i at i * (2 radius + 1)
};

static ChannelSet channel_of(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, const am_peak* peaks, size_t n) {
    ChannelSet cs;
    cs.radius = *args.channel_radius;
    cs.recs.resize(n);
    cs.taps.resize(n * (2 * (size_t)cs.radius + 1));
    const am_channel_params cp{cs.radius, 0, args.channel_noise_db};
    if (n > 0 && am_hit_channel(algo, samples.data(), samples.size(), AM_FMT_F32_MONO, peaks, n, &cp, cs.recs.data(), cs.taps.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_channel: ") + am_last_error_string());
    return cs;
}

// ... one line per hit, to follow the hit's offset line
static std::vector<std::string> channel_lines(const ChannelSet& cs) {
    std::vector<std::string> out;
    for (const am_channel_hit& q : cs.recs) {
        char line[256];
        std::snprintf(line, sizeof line, "  channel ncc %.6f ncc_eq %.6f gain_db %.2f residual_db %.2f main_tap %d main_share %.4f%s%s%s%s", (double)q.ncc,
                      (double)q.ncc_eq, (double)q.gain_db, (double)q.residual_db, (int)q.main_tap, (double)q.main_share,
                      (q.flags & AM_HIT_BELOW_FLOOR) ? " (below the floor)" : "", (q.flags & AM_HIT_NONFINITE) ? " (non-finite samples)" : "",
                      (q.flags & AM_HIT_EMPTY_SEGMENT) ? " (silent snippet)" : "", (q.flags & AM_HIT_ILL_CONDITIONED) ? " (ill-conditioned: plain gain)" : "");
        out.push_back(line);
    }
    return out;
}

// extension: --residual PREFIX.  Per printed hit PREFIX<file index>_<start>.wav: the hit's span minus the snippet filtered
// by the hit's taps (am_hit_residual), samples the file does not hold (or that are not finite) as 0.  `needle`: the
// snippet's samples as the handle holds them.
static void write_residuals(const Arguments& args, const std::vector<float>& samples, std::uint32_t m_sr, const std::vector<float>& needle,
                            size_t file_index, const am_peak* peaks, size_t n, const ChannelSet& cs) {
    const size_t nt = 2 * (size_t)cs.radius + 1;
    std::vector<float> resid(needle.size() + nt - 1);
    for (size_t i = 0; i < n; ++i) {
        if (cs.recs[i].flags & AM_HIT_NONFINITE) continue;   // (no taps)
        if (am_hit_residual(samples.data(), samples.size(), AM_FMT_F32_MONO, peaks[i].start, needle.data(), needle.size(), cs.taps.data() + i * nt,
                            cs.radius, nullptr, resid.data()) != AM_OK)
            throw std::runtime_error(std::string("am_hit_residual: ") + am_last_error_string());
        for (float& v : resid)
            if (!std::isfinite(v)) v = 0.0f;
        write_wav_f32(args.residual_prefix + std::to_string(file_index) + "_" + std::to_string(peaks[i].start) + ".wav", resid, m_sr);
    }
}

// extension: --stereo R[:MIN_NCC].  One line per hit, to follow the hit's offset line: where the hit sits between the
// channels of the main file's own i16 frames (am_hit_stereo, am_hit_stereo_summary).
static std::vector<std::string> stereo_lines(const Arguments& args, const am_needle* algo, const Pcm& m, const am_peak* peaks, size_t n) {
    if (m.is_float || m.channels != 2) throw std::runtime_error("--stereo: the main file is not a 16-bit two-channel file");
    std::vector<am_stereo_hit> recs(n);
    const am_stereo_params sp{*args.stereo_radius, 0};
    if (n > 0 && am_hit_stereo(algo, m.s16.data(), m.frames(), AM_FMT_S16_STEREO, peaks, n, &sp, recs.data()) != AM_OK)
        throw std::runtime_error(std::string("am_hit_stereo: ") + am_last_error_string());
    static const char* const images[] = {"absent", "centre", "left", "right", "panned", "inverted"};
    std::vector<std::string> out;
    for (const am_stereo_hit& q : recs) {
        am_stereo_summary sm{};
        if (am_hit_stereo_summary(&q, args.stereo_min_ncc, &sm) != AM_OK)
            throw std::runtime_error(std::string("am_hit_stereo_summary: ") + am_last_error_string());
        char line[320];
        std::snprintf(line, sizeof line, "  stereo image %s ncc_left %.6f ncc_right %.6f ncc_side %.6f ncc_best %.6f balance_db %.2f delay %.3f downmix_loss_db %.2f%s%s",
                      images[sm.image], (double)q.ncc_left, (double)q.ncc_right, (double)q.ncc_side, (double)q.ncc_best, sm.balance_db, sm.delay,
                      sm.downmix_loss_db, (q.flags & AM_HIT_COLLINEAR) ? " (collinear channels)" : "", (q.flags & AM_HIT_NONFINITE) ? " (non-finite samples)" : "");
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

// extension: --min-confidence X without --warp.  Keeps the hits whose exact NCC is at least X, in place; returns how many
// are left.  With --debug one line per hit (`prefix` in front).
static size_t confidence_filter(const Arguments& args, const am_needle* algo, const std::vector<float>& samples, am_peak* peaks, size_t n,
                                const std::string& prefix) {
    const std::vector<am_hit_score> sc = hit_scores(algo, samples, peaks, n);
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool keep = sc[i].ncc >= *args.min_confidence;   // (a NaN ncc is dropped too)
        if (args.verbosity >= 2)
            std::printf("%shit %zu: position %.3f ncc %.6f gain %.6g window %.2f dB%s\n", prefix.c_str(), i + 1, sc[i].position,
                        (double)sc[i].ncc, (double)sc[i].gain, (double)sc[i].window_db, keep ? "" : " (dropped)");
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
        const std::vector<am_hit_score> sc = args.warp_ppm ? std::vector<am_hit_score>() : hit_scores(algo, samples, peaks, n);
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
        const std::vector<float> x = to_mono_f32(args, read_wav(main_file), main_file);
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
static am_needle* create_needle(const Arguments& args, const std::vector<float>& data, std::uint32_t sr, std::uint32_t m_sr,
                                const std::vector<float>& taps) {
    am_needle* h = nullptr;
    if (!args.ignore_ms.empty()) {
        // extension: --ignore (the parser admits it without --resample and a filter only): a masked handle, the spans in
        // samples of the snippet's own rate, sorted; the library names the span that breaks a rule
        std::vector<am_span> gaps;
        for (const auto& g : args.ignore_ms) gaps.push_back(am_span{round_samples_ms(g.first, sr), round_samples_ms(g.second, sr)});
        std::sort(gaps.begin(), gaps.end(), [](const am_span& a, const am_span& b) { return a.begin < b.begin; });
        if (am_needle_create_masked(args.device, data.data(), data.size(), gaps.data(), gaps.size(), &h) != AM_OK)
            throw std::runtime_error(std::string("--ignore: ") + am_last_error_string());
        return h;
    }
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

// ... owned, and with --normalize on it
static Needle make_needle(const Arguments& args, const std::vector<float>& data, std::uint32_t sr, std::uint32_t m_sr,
                          const std::vector<float>& taps) {
    Needle h(create_needle(args, data, sr, m_sr, taps));
    if (args.normalize && am_needle_set_option(h.get(), "score_norm", 1) != AM_OK)
        throw std::runtime_error(std::string("--normalize: ") + am_last_error_string());
    return h;
}

// One --snippet file of the file mode: its samples, its handle at its own rate (mod.rs:29-34) and, with --resample, one
// handle per main-file rate other than its own, made on first use and kept.
struct Snippet {
    std::string name;
    std::uint32_t sr = 0;
    double duration = 0.0;             // mod.rs:30 (mp3_duration)
    std::vector<float> data;
    Needle h;
    std::map<std::uint32_t, Needle> resampled;
};

// taps: the run's filter; where it is not designed yet, it is designed between reading the snippet and creating its handle
static Snippet load_snippet(const Arguments& args, const std::string& path, std::optional<std::vector<float>>& taps) {
    Snippet sn;
    const Pcm pcm = read_wav(path);
    sn.name = base_name(path);
    sn.sr = pcm.sample_rate;
    sn.duration = (double)pcm.frames() / (double)sn.sr;
    sn.data = to_mono_f32(args, pcm, path);
    if (!taps) taps = filter_taps(args);
    sn.h = make_needle(args, sn.data, sn.sr, sn.sr, *taps);
    return sn;
}

// The handle of sn for a main file of rate m_sr, and the overlap it is matched with: the snippet's length at that rate
// (as make_params rounds it; the resampled handle's own length where the rates differ).
static const am_needle* needle_at(const Arguments& args, Snippet& sn, std::uint32_t m_sr, const std::vector<float>& taps, std::uint64_t& overlap) {
    overlap = make_params(args, m_sr, sn.duration).overlap;
    if (m_sr == sn.sr) return sn.h.get();
    Needle& h = sn.resampled[m_sr];
    if (!h) h = make_needle(args, sn.data, sn.sr, m_sr, taps);
    size_t s_len = 0;
    am_needle_len(h.get(), &s_len);
    overlap = s_len;
    return h.get();
}

// mod.rs:44-66: where a main file's labels go (nowhere: --no-out, or an existing file that is not to be overwritten);
// false = the main file is skipped, because its output exists.
static bool output_path(const Arguments& args, const std::string& main_file, std::optional<std::string>& out_path) {
    out_path = args.out_file;
    if (!out_path && !args.no_out) out_path = auto_out_file(main_file);
    if (out_path && file_exists(*out_path)) {
        if (args.skip_existing || ask_consent(args, "Ausgabe Datei \"" + *out_path + "\" existiert bereits, möchtest du skippen"))
            return false;
        if (!ask_consent(args, "soll die existierende Datei überschrieben werden")) out_path.reset();
    }
    return true;
}

// mod.rs:92-99: the label file of a recording's hits (sorted by start), or with --dry-run its text on stdout.  Returns the
// exit status this asks for: 0, or 4 where the file cannot be written.
// `extra`: labels behind those of the hits (--edges).
static int write_labels(const Arguments& args, const std::string& out_path, const std::vector<am_peak>& hits, std::uint32_t sr,
                        const std::vector<TimeLabel>& extra = {}) {
    const std::string text = format_labels(timelabel_from_peaks(hits.data(), hits.size(), sr, 7.0, "Segment #")) + format_labels(extra);
    if (args.dry_run) {
        std::printf("would write to '%s':\n%s", out_path.c_str(), text.c_str());
        return 0;
    }
    std::ofstream f(out_path, std::ios::binary | std::ios::trunc);
    if (!f) { std::fprintf(stderr, "couldn't find file '%s'\n", out_path.c_str()); return 4; }
    f << text;
    return 0;
}

// mod.rs:81-87: the hits of one snippet in one main file
static std::vector<am_peak> match_hits(const am_needle* algo, const std::vector<float>& samples, const am_match_params& p) {
    std::vector<am_peak> peaks(1024);
    size_t n = 0;
    int rc = am_match(algo, samples.data(), samples.size(), &p, peaks.data(), peaks.size(), &n);
    if (rc == AM_ERR_CAPACITY) {
        peaks.resize(n);
        rc = am_match(algo, samples.data(), samples.size(), &p, peaks.data(), peaks.size(), &n);
    }
    if (rc != AM_OK) throw std::runtime_error(std::string("am_match: ") + am_last_error_string());
    peaks.resize(n);
    return peaks;
}

// extension: several --snippet files without --normalize and --best.  ONE am_match_multi_varlen call for a main file (the
// snippets may differ in length: each is matched with its own overlap); [j] = the hits of snippet j.
static std::vector<std::vector<am_peak>> match_hits_multi(const std::vector<const am_needle*>& handles, const std::vector<std::uint64_t>& overlaps,
                                                          const std::vector<float>& samples, const am_match_params& p) {
    const size_t k = handles.size();
    size_t cap = 1024;
    std::vector<am_peak> peaks(cap * k);
    std::vector<size_t> n(k, 0);
    int rc = am_match_multi_varlen(handles.data(), k, overlaps.data(), samples.data(), samples.size(), AM_FMT_F32_MONO, &p, peaks.data(), cap, n.data());
    if (rc == AM_ERR_CAPACITY) {
        for (size_t j = 0; j < k; ++j) cap = std::max(cap, n[j]);
        peaks.assign(cap * k, am_peak{});
        rc = am_match_multi_varlen(handles.data(), k, overlaps.data(), samples.data(), samples.size(), AM_FMT_F32_MONO, &p, peaks.data(), cap, n.data());
    }
    if (rc != AM_OK) throw std::runtime_error(std::string("am_match_multi_varlen: ") + am_last_error_string());
    std::vector<std::vector<am_peak>> each(k);
    for (size_t j = 0; j < k; ++j) each[j].assign(peaks.begin() + (std::ptrdiff_t)(j * cap), peaks.begin() + (std::ptrdiff_t)(j * cap + n[j]));
    return each;
}

// One snippet's hits in one main file, from the match to the report: the filters (--min-confidence, on the corrected NCC
// with --warp; --min-significance) drop hits from `hits`, the learner takes its rows of those that are left, and they
// are printed, every line with `prefix` in front: the offset line (mod.rs:89) and under it the hit's --warp, --segments
// and --bands lines; with --channel the hit's channel line, and with --residual its residual file (`snip`: the snippet as
// read, `file_index`: the main file's place among the FILE arguments); with --stereo the hit's stereo line (`m`: the main
// file as read, its i16 frames kept).
static void report_hits(const Arguments& args, const am_needle* algo, const std::vector<float>& m_samples, std::uint32_t m_sr,
                        std::vector<am_peak>& hits, const std::string& prefix, Learner& learner, const Snippet& snip, size_t file_index,
                        const Pcm& m) {
    am_peak* pk = hits.data();
    size_t n = hits.size();
    const WarpSet warp = WarpSet::compute(args, algo, m_samples, pk, n);
    if (args.min_confidence && n > 0 && !args.ignore_ms.empty()) n = mask_confidence_filter(args, algo, m_samples, pk, n, prefix);
    else if (args.min_confidence && n > 0)
        n = args.warp_ppm ? warp_confidence_filter(args, warp, pk, n, prefix) : confidence_filter(args, algo, m_samples, pk, n, prefix);
    if (args.min_significance) n = significance_filter(args, algo, m_samples, m_sr, pk, n, prefix);
    hits.resize(n);
    if (!args.learn_needle.empty()) learner.take(args, algo, m_samples, m_sr, pk, n, warp.of(pk, n));
    if (args.verbosity < 1) return;
    const std::vector<std::string> none;
    const std::vector<std::string> lines = offset_lines(pk, n, m_sr);
    const std::vector<std::string> segs = args.segments ? segment_lines(args, algo, m_samples, pk, n) : none;
    const std::vector<std::string> bands = args.bands ? band_lines(args, algo, m_samples, m_sr, pk, n) : none;
    const std::vector<std::string> warps = args.warp_ppm ? warp_lines(warp.of(pk, n)) : none;
    std::vector<std::string> chan_lines;
    const std::vector<std::string>& chans = chan_lines;
    if (args.channel_radius) {
        const ChannelSet cs = channel_of(args, algo, m_samples, pk, n);
        chan_lines = channel_lines(cs);
        if (!args.residual_prefix.empty()) {
            if (m_sr != snip.sr) throw std::runtime_error("--residual: the snippet was resampled for this file; its samples at the file's rate are not kept");
            write_residuals(args, m_samples, m_sr, snip.data, file_index, pk, n, cs);
        }
    }
    const std::vector<std::string> stereo = args.stereo_radius ? stereo_lines(args, algo, m, pk, n) : none;
    const std::vector<std::string> masks = args.mask_report ? mask_lines(mask_records(algo, m_samples, pk, n)) : none;
    for (size_t i = 0; i < lines.size(); ++i)
        for (const std::vector<std::string>* l : {&lines, &masks, &stereo, &warps, &chans, &segs, &bands})
            if (i < l->size()) std::printf("%s%s\n", prefix.c_str(), (*l)[i].c_str());
}

// extension: --envelope.  The places where one snippet occurs at another speed in one main file (am_match_envelope), printed
// under the snippet's offset lines; those without a hit within half a snippet of them join `hits` (height and prominence:
// the envelope score), which then stays sorted by start.
static void envelope_hits(const Arguments& args, const am_needle* algo, const std::vector<float>& m_samples, std::uint32_t m_sr,
                          std::vector<am_peak>& hits, const std::string& prefix) {
    am_env_params ep{};
    if (am_band_edges_log(m_sr, 10, 150.0, std::min(6000.0, 0.45 * (double)m_sr), 8, &ep.bands) != AM_OK)
        throw std::runtime_error(std::string("--envelope: am_band_edges_log: ") + am_last_error_string());
    ep.floor_db = 80.0;
    am_env_grid grid{};
    grid.max_ppm = *args.envelope_pct * 1e4;
    grid.steps = args.envelope_steps;
    std::vector<am_env_hit> env(256);
    size_t n = 0;
    int rc = am_match_envelope(algo, m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, &ep, &grid, args.envelope_min_score, env.data(), env.size(), &n);
    if (rc == AM_ERR_CAPACITY) {
        env.resize(n);
        rc = am_match_envelope(algo, m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, &ep, &grid, args.envelope_min_score, env.data(), env.size(), &n);
    }
    if (rc != AM_OK) throw std::runtime_error(std::string("am_match_envelope: ") + am_last_error_string());
    env.resize(n);
    size_t s_len = 0;
    am_needle_len(algo, &s_len);
    const std::vector<am_peak> found = hits;
    for (const am_env_hit& e : env) {
        if (args.verbosity >= 1) std::printf("%s%s\n", prefix.c_str(), envelope_line(e, m_sr).c_str());
        bool known = false;
        for (const am_peak& pk : found)
            known = known || (pk.start > e.start ? pk.start - e.start : e.start - pk.start) <= s_len / 2;
        if (!known) hits.push_back(am_peak{e.start, e.start + e.length, e.score, e.score});
    }
    std::stable_sort(hits.begin(), hits.end(), [](const am_peak& a, const am_peak& b) { return a.start < b.start; });
}

// extension: --edges.  One snippet cut off by the start or the end of one main file (am_match_edges): a line per edge that
// counts (edge_passes), printed behind the snippet's other lines, and its label into `labels`.
static void edge_hits(const Arguments& args, const am_needle* algo, const std::vector<float>& m_samples, std::uint32_t m_sr,
                      const std::string& prefix, std::vector<TimeLabel>& labels) {
    if (m_samples.empty()) return;
    am_edge_params ep{};
    ep.min_overlap = std::max<std::uint64_t>(1, round_samples_ms(*args.edges_ms, m_sr));
    ep.min_share = 0.05f;
    am_edge_hit recs[2];
    if (am_match_edges(algo, m_samples.data(), m_samples.size(), AM_FMT_F32_MONO, &ep, recs) != AM_OK)
        throw std::runtime_error(std::string("am_match_edges: ") + am_last_error_string());
    size_t s_len = 0;
    am_needle_len(algo, &s_len);
    for (const am_edge_hit& r : recs) {
        if (!edge_passes(r, args.edges_min_ncc, args.edges_max_second)) continue;
        if (args.verbosity >= 1) std::printf("%s%s\n", prefix.c_str(), edge_line(r, s_len, m_sr).c_str());
        labels.push_back(edge_label(r, s_len, m_samples.size(), m_sr));
    }
}

// extension: --score-trace.  The score curve of one snippet in one main file: its CSV file (`snippet_index`: set when the
// run has several snippets) and, under the offset lines, its summary line.  Returns 0, or 4 where the file cannot be
// written.
static int write_trace(const Arguments& args, const am_needle* algo, const std::vector<float>& m_samples, std::uint32_t m_sr,
                       size_t file_index, std::optional<size_t> snippet_index, const std::string& prefix) {
    std::uint64_t bin = 0;
    const std::vector<am_trace_bin> bins = trace_of(args, algo, m_samples, m_sr, &bin);
    if (args.verbosity >= 1) std::printf("%s%s\n", prefix.c_str(), trace_line(bins, bin, m_sr).c_str());
    const std::string path = args.trace_prefix + std::to_string(file_index) + (snippet_index ? "_" + std::to_string(*snippet_index) : std::string()) + ".csv";
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) { std::fprintf(stderr, "couldn't write file '%s'\n", path.c_str()); return 4; }
    f << trace_csv(bins, bin, m_sr);
    return 0;
}

// The file mode: the per-file loop of matcher::run (mod.rs:42-100) for one or several --snippet files.  One snippet is
// matched by am_match, as the reference does.  Several (an extension) are matched by ONE am_match_multi_varlen call for a
// main file; with --normalize, which that call refuses, snippet by snippet with am_match; every line of a snippet's
// report then starts with the snippet's file name, and the label file holds the hits of all snippets, sorted by start
// (equal starts in --snippet order).  --best N (an extension) takes am_match_best's hits instead, snippet by snippet.
static int run_files(const Arguments& args) {
    // (set ahead of everything else: the parser admits 0..200 only, which is the option's whole range, so the call
    // cannot fail, and the library reads the value when a call is made, not when a handle is created)
    if (args.normalize_floor_db && am_set_option("score_norm_floor_db", *args.normalize_floor_db) != AM_OK)
        throw std::runtime_error(std::string("--normalize-floor: ") + am_last_error_string());
    const size_t k = args.snippets.size();
    // extension: --whiten / --preemphasis.  Designing the filter reads the main files: with several snippets ahead of
    // the first snippet, with one after it (load_snippet) -- which of two unreadable files an error names
    std::optional<std::vector<float>> taps;
    if (k > 1) taps = filter_taps(args);
    std::vector<Snippet> snips;
    for (const std::string& path : args.snippets) snips.push_back(load_snippet(args, path, taps));
    if (args.verbosity >= 2) am_set_progress_callback(progress, nullptr);
    int rc_all = 0;
    Learner learner;                                                      // extension: --learn-needle (one snippet only)
    size_t file_index = (size_t)-1;                                       // (of --residual's file names: the main file's place among the FILE arguments)
    for (const std::string& main_file : args.within) {                    // mod.rs:42
        ++file_index;
        std::optional<std::string> out_path;
        if (!output_path(args, main_file, out_path)) continue;
        if (args.verbosity >= (args.within.size() == 1 ? 3 : 1))
            std::printf("preparing data of '%s'\n", main_file.c_str());
        const Pcm m = read_wav(main_file);                                // mod.rs:71
        const std::uint32_t m_sr = m.sample_rate;
        std::vector<const am_needle*> handles(k);
        std::vector<std::uint64_t> overlaps(k);
        for (size_t j = 0; j < k; ++j) {
            if (m_sr != snips[j].sr && !args.resample) {                  // mod.rs:72-74 SampleRateMismatch
                std::fprintf(stderr, "sample rate of snippet (%u) and main file (%u) don't match\n", snips[j].sr, m_sr);
                return 3;
            }
            handles[j] = needle_at(args, snips[j], m_sr, *taps, overlaps[j]);
        }
        const std::vector<float> m_samples = filtered(args, to_mono_f32(args, m, main_file), *taps);
        am_match_params p = make_params(args, m_sr, snips[0].duration);
        std::vector<std::vector<am_peak>> hits(k);
        if (k > 1 && !args.best && !args.normalize) {
            hits = match_hits_multi(handles, overlaps, m_samples, p);
        } else {
            for (size_t j = 0; j < k; ++j) {
                p.overlap = overlaps[j];
                hits[j] = args.best ? best_hits(args, handles[j], m_samples, m_sr) : match_hits(handles[j], m_samples, p);
            }
        }
        std::vector<TimeLabel> edge_labels;                               // extension: --edges
        for (size_t j = 0; j < k; ++j) {
            const std::string prefix = k > 1 ? snips[j].name + ": " : std::string();
            report_hits(args, handles[j], m_samples, m_sr, hits[j], prefix, learner, snips[j], file_index, m);
            if (args.envelope_pct) envelope_hits(args, handles[j], m_samples, m_sr, hits[j], prefix);
            if (args.edges_ms) edge_hits(args, handles[j], m_samples, m_sr, prefix, edge_labels);
        }
        if (!args.trace_prefix.empty())
            for (size_t j = 0; j < k; ++j)
                if (const int rc = write_trace(args, handles[j], m_samples, m_sr, file_index, k > 1 ? std::optional<size_t>(j) : std::nullopt,
                                               k > 1 ? snips[j].name + ": " : std::string()))
                    rc_all = rc;
        if (out_path) {                                                   // mod.rs:92-99
            std::vector<am_peak> all;
            for (const std::vector<am_peak>& h : hits) all.insert(all.end(), h.begin(), h.end());
            if (k > 1) std::stable_sort(all.begin(), all.end(), [](const am_peak& a, const am_peak& b) { return a.start < b.start; });
            if (const int rc = write_labels(args, *out_path, all, m_sr, edge_labels)) rc_all = rc;
        }
    }
    if (!args.learn_needle.empty())
        if (const int rc = learner.finish(args)) rc_all = rc;
    return rc_all;
}

// extension: --discover DUR[:HOP].  No snippet: the first FILE is searched against itself (AM_DISCOVER_SELF, exclude = the
// probe length, AM_REGION_FOLD) and then against every further FILE; one line per region, and with --discover-out the
// region's samples of the first FILE as a WAV file.  The region settings other than --discover-min-ncc are fixed:
// tolerance HOP / 8, at least 2 good probes, gaps of 1 bridged, probes 40 dB below the file's level skipped.
static int run_discover(const Arguments& args) {
    if (args.normalize_floor_db && am_set_option("score_norm_floor_db", *args.normalize_floor_db) != AM_OK)
        throw std::runtime_error(std::string("--normalize-floor: ") + am_last_error_string());
    const Pcm a_pcm = read_wav(args.within[0]);
    const std::uint32_t sr = a_pcm.sample_rate;
    const std::vector<float> a = to_mono_f32(args, a_pcm, args.within[0]);
    am_discover_params dp{};
    dp.probe_len = std::max<std::uint64_t>(1, round_samples_ms(*args.discover_ms, sr));
    dp.hop = std::max<std::uint64_t>(1, round_samples_ms(args.discover_hop_ms, sr));
    dp.min_level_db = 40.0f;
    am_region_params rp{};
    rp.min_ncc = args.discover_min_ncc;
    rp.tolerance = dp.hop / 8;
    rp.min_good = 2;
    rp.max_gap = 1;
    auto stamp = [&](std::uint64_t sample) {
        const std::uint64_t ms = (std::uint64_t)((double)sample * 1000.0 / (double)sr);
        char buf[64];
        std::snprintf(buf, sizeof buf, "%02" PRIu64 ":%02" PRIu64 ":%02" PRIu64 ".%03" PRIu64, ms / 3600000, (ms / 60000) % 60, (ms / 1000) % 60, ms % 1000);
        return std::string(buf);
    };
    int rc_all = 0;
    for (size_t file_index = 0; file_index < args.within.size(); ++file_index) {
        const bool self = file_index == 0;
        std::vector<float> b_own;
        if (!self) {
            const Pcm b_pcm = read_wav(args.within[file_index]);
            if (b_pcm.sample_rate != sr) {
                std::fprintf(stderr, "sample rate of '%s' (%u) and '%s' (%u) don't match\n", args.within[file_index].c_str(), b_pcm.sample_rate,
                             args.within[0].c_str(), sr);
                return 3;
            }
            b_own = to_mono_f32(args, b_pcm, args.within[file_index]);
        }
        const std::vector<float>& b = self ? a : b_own;
        dp.flags = self ? AM_DISCOVER_SELF : 0u;
        dp.exclude = self ? dp.probe_len : 0;
        rp.flags = self ? AM_REGION_FOLD : 0u;
        size_t np = 0, got = 0, nr = 0;
        if (am_discover_len(a.size(), &dp, &np) != AM_OK) throw std::runtime_error(std::string("am_discover_len: ") + am_last_error_string());
        std::vector<am_probe_hit> hits(np);
        if (am_discover(args.device, a.data(), a.size(), b.data(), b.size(), AM_FMT_F32_MONO, &dp, hits.data(), hits.size(), &got) != AM_OK)
            throw std::runtime_error(std::string("am_discover: ") + am_last_error_string());
        std::vector<am_region> regions(np);
        if (am_discover_regions(hits.data(), hits.size(), &dp, &rp, regions.data(), regions.size(), &nr) != AM_OK)
            throw std::runtime_error(std::string("am_discover_regions: ") + am_last_error_string());
        regions.resize(nr);
        for (const am_region& r : regions) {
            if (args.verbosity >= 1)
                std::printf("Region: %s +%.3fs -> %s %s, ncc mean %.3f min %.3f, %u/%u probes\n", stamp(r.a_start).c_str(),
                            (double)r.length / (double)sr, args.within[file_index].c_str(),
                            stamp((std::uint64_t)((std::int64_t)r.a_start + r.displacement)).c_str(), r.mean_ncc, (double)r.min_ncc, r.good, r.count);
            if (!args.discover_out.empty()) {
                const std::string path = args.discover_out + std::to_string(file_index) + "_" + std::to_string(r.a_start) + ".wav";
                const std::vector<float> cut(a.begin() + (std::ptrdiff_t)r.a_start, a.begin() + (std::ptrdiff_t)(r.a_start + r.length));
                try {
                    write_wav_f32(path, cut, sr);
                } catch (const std::exception& e) {
                    std::fprintf(stderr, "%s\n", e.what());
                    rc_all = 4;
                }
            }
        }
    }
    return rc_all;
}

// extension: --live.  Raw PCM from stdin through one monitor (am_monitor_*, all snippets in it): every chunk of input is
// turned into the f32 mono samples the file mode would have made of the same frames (to_mono_f32), pushed, and the hits
// that became final are printed at once, numbered per snippet as the file mode numbers them.  At end of input the
// label file is written exactly as the file mode writes it for that recording (the hits of all snippets by start, equal
// starts in --snippet order: the monitor's own order).
static int run_live(const Arguments& args) {
    struct Snip {
        std::string name;
        Needle h, resampled;
        am_match_params p{};
        size_t hits = 0;
    };
    const std::uint32_t sr = args.rate;
    const size_t k = args.snippets.size();
    std::vector<Snip> snips(k);
    std::vector<const am_needle*> handles(k);
    std::vector<am_match_params> params(k);
    for (size_t j = 0; j < k; ++j) {
        Snip& sn = snips[j];
        const Pcm pcm = read_wav(args.snippets[j]);
        sn.name = base_name(args.snippets[j]);
        const double duration = (double)pcm.frames() / (double)pcm.sample_rate;
        const std::vector<float> data = to_mono_f32(pcm, args.device);
        am_needle* h = nullptr;
        if (am_needle_create(args.device, data.data(), data.size(), &h) != AM_OK)
            throw std::runtime_error(std::string("am_needle_create: ") + am_last_error_string());
        sn.h.reset(h);
        sn.p = make_params(args, sr, duration);
        handles[j] = sn.h.get();
        if (pcm.sample_rate != sr) {
            if (!args.resample) {
                std::fprintf(stderr, "sample rate of snippet (%u) and main file (%u) don't match\n", pcm.sample_rate, sr);
                return 3;
            }
            am_needle* r = nullptr;
            if (am_needle_create_resampled(args.device, data.data(), data.size(), AM_FMT_F32_MONO, pcm.sample_rate, sr, &r) != AM_OK)
                throw std::runtime_error(std::string("am_needle_create_resampled: ") + am_last_error_string());
            sn.resampled.reset(r);
            size_t s_len = 0;   // the overlap = the resampled snippet's length
            am_needle_len(sn.resampled.get(), &s_len);
            sn.p.overlap = s_len;
            handles[j] = sn.resampled.get();
        }
        params[j] = sn.p;
    }
    am_monitor* opened = nullptr;
    if (am_monitor_begin(handles.data(), k, params.data(), AM_FMT_F32_MONO, 1, &opened) != AM_OK)
        throw std::runtime_error(std::string("am_monitor_begin: ") + am_last_error_string());
    const Monitor mon(opened);           // (declared after snips: destroyed ahead of the handles it holds)
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
        int rc = fn(mon.get(), got.data(), which.data(), got.size(), &n);
        if (rc == AM_ERR_CAPACITY) {
            got.resize(n); which.resize(n);
            rc = fn(mon.get(), got.data(), which.data(), got.size(), &n);
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
        if (am_monitor_push(mon.get(), mono.data(), mono.size()) != AM_OK)
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
    return args.out_file && !args.no_out ? write_labels(args, *args.out_file, all, sr) : 0;
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
    try {
        return args.discover_ms ? run_discover(args) : args.live ? run_live(args) : run_files(args);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
