// am_host.hpp -- host-side callers and data formats either side of the hot path
// (SURVEY.md section 8f, rows N1-N4), header-only C++17:
//
//   parse_duration            src/args.rs:80-121 (grammar "3h5m17s", "100ms", bare seconds)
//   Arguments                 src/matcher/args.rs:9-77 (flags, defaults 13 / 60 s / 8 min)
//   read_pcm (WAV)            stands in for mp3_reader::read_mp3 (src/matcher/mp3_reader.rs:13-41):
//                             MP3 decode is out of scope; the i16-stereo down-mix itself runs on
//                             the GPU (am_pcm_s16_stereo_to_mono, mp3_reader.rs:28-37)
//   print_offsets             src/matcher/mod.rs:110-125
//   timelabel_from_peaks      src/archive/data.rs:87-107
//   write_labels              audacity::data::TimeLabel::write (external crate, source absent:
//                             Audacity's label-track text format "start\tend\tname", 6 decimals;
//                             PARITY UNPINNED)
#pragma once

#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <optional>
#include <regex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/audiomatch.h"

namespace amhost {

// ---- src/args.rs:80-121 ------------------------------------------------------
// returns milliseconds; nullopt = Err(NoMatch(arg))
inline std::optional<std::uint64_t> parse_duration_ms(const std::string& arg) {
    if (arg.empty()) return std::nullopt;                                   // :84-87
    bool digits = true;
    for (char c : arg) digits = digits && c >= '0' && c <= '9';
    if (digits) {                                                           // arg.parse::<u64>() -> seconds
        errno = 0;
        const unsigned long long v = std::strtoull(arg.c_str(), nullptr, 10);
        if (errno == 0) return (std::uint64_t)v * 1000u;
    }
    static const std::regex re(
        "^(?:(?:(\\d+)h(?:ours?)?)?(?:(\\d+)m(?:in)?)?(?:(\\d+)s(?:ec)?)?)(?:(\\d+)ms(?:ec)?)?$");
    std::smatch m;
    if (!std::regex_match(arg, m, re)) return std::nullopt;
    std::uint64_t ms = 0;
    if (m[1].matched) ms += std::strtoull(m[1].str().c_str(), nullptr, 10);
    ms *= 60;
    if (m[2].matched) ms += std::strtoull(m[2].str().c_str(), nullptr, 10);
    ms *= 60;
    if (m[3].matched) ms += std::strtoull(m[3].str().c_str(), nullptr, 10);
    ms *= 1000;
    if (m[4].matched) ms += std::strtoull(m[4].str().c_str(), nullptr, 10);
    return ms;
}

// ---- src/matcher/args.rs:9-77 --------------------------------------------------
struct Arguments {
    std::vector<std::string> within;          // positional FILEs
    std::string snippet;                      // --snippet FILE (the first one given)
    std::vector<std::string> snippets;        // extension: every --snippet FILE, in order (several: one am_match_multi_varlen per file)
    float prominence = 13.0f;                 // -p/--prominence, default 13 (:19)
    std::optional<std::uint64_t> distance_ms; // --distance (default 8 min, :73-76)
    std::optional<std::uint64_t> chunk_ms;    // --chunk-size (default 60 s, :70-72)
    bool fancy_bar = false;                   // accepted, no effect here
    bool dry_run = false;
    bool skip_existing = false;
    bool no_out = false;                      // OutFile group (:54-66)
    std::optional<std::string> out_file;
    int always_answer = -1;                   // common::args::input::Inputs: -y -> 1, -n -> 0, else ask
    int verbosity = 1;                        // OutputLevel: --silent 0, default 1 (info), --debug 2, --trace 3
    int device = 0;                           // extension: GPU ordinal
    bool normalize = false;                   // extension: --normalize, window-energy normalised scores (option "score_norm")
    std::optional<int> normalize_floor_db;    // extension: --normalize-floor DB (option "score_norm_floor_db", 0..200)
    std::optional<float> min_confidence;      // extension: --min-confidence X, drop hits whose exact NCC is below X (am_hit_scores, 0..1)
    std::uint32_t segments = 0;               // extension: --segments M[:R], per-segment scoring of every printed hit (am_hit_segments), 0 = off
    std::uint32_t segment_radius = 4;         // ... the lags -R .. R examined per segment
    std::optional<double> warp_ppm;           // extension: --warp PPM[:STEPS[:RADIUS]], drift and corrected NCC of every hit (am_hit_warp)
    std::uint32_t warp_steps = 8;             // ... drifts -PPM .. PPM in 2 STEPS + 1 steps
    std::uint32_t warp_radius = 4;            // ... the lags -RADIUS .. RADIUS
    std::optional<std::uint32_t> channel_radius;   // extension: --channel P[:NOISE_DB], the filter every printed hit went through (am_hit_channel): taps -P .. P
    double channel_noise_db = 60.0;           // ... the white-noise correction of the solve
    std::string residual_prefix;              // extension: --residual PREFIX, what is left of each printed hit's span (am_hit_residual) as PREFIX<file index>_<start>.wav; empty = off
    bool mix_set = false;                     // extension: --mix left|right|mid|side|A,B, a two-channel file through am_pcm_s16_stereo_mix instead of the down-mix
    float mix_a = 0.5f, mix_b = 0.5f;         // ... out = a L + b R; mid (0.5, 0.5) is the down-mix itself
    std::optional<std::uint32_t> stereo_radius;   // extension: --stereo R[:MIN_NCC], where every printed hit sits between the channels (am_hit_stereo): lags -R .. R
    float stereo_min_ncc = 0.5f;              // ... what a channel's |NCC| must reach to count (am_hit_stereo_summary)
    std::uint32_t bands = 0;                  // extension: --bands B[:LOG2F], per-band scoring of every printed hit (am_hit_bands), 0 = off
    std::uint32_t band_frame_log2 = 11;       // ... in frames of 2^LOG2F samples
    std::optional<float> min_significance;    // extension: --min-significance Z, drop hits whose z against the local background is below Z (am_hit_significance)
    std::optional<std::uint64_t> significance_zone_ms;   // ... --significance-zone D: the background reaches D each side of a hit (default: three snippet lengths)
    bool resample = false;                    // extension: --resample, bring the snippet to each main file's rate (am_needle_create_resampled)
    std::uint32_t whiten = 0;                 // extension: --whiten P, one order-P whitening filter designed from all main files (am_lag_products, am_whiten_taps), 0 = off
    std::optional<float> preemphasis;         // extension: --preemphasis A, the fixed filter {1, -A} on snippets and main files (am_fir)
    std::string learn_needle;                 // extension: --learn-needle OUT.wav[:METHOD], a cleaner snippet estimated from the run's hits (am_needle_estimate_rows); empty = off
    std::uint32_t learn_method = AM_EST_MEDIAN;   // ... :mean | :median | :trimmed=P
    std::uint32_t learn_trim = 0;             // ... P of trimmed=P, in 1/1000 (0..500)
    std::optional<std::uint64_t> learn_margin_ms;   // ... --learn-margin D: read D in front of and behind the snippet as well (default 0)
    std::optional<std::uint64_t> best;        // extension: --best N, the N best hits per main file, no prominence threshold (am_match_best)
    std::string trace_prefix;                 // extension: --score-trace PREFIX[:BIN], the score curve of each main file (am_match_trace) as PREFIX<file index>[_<snippet index>].csv; empty = off
    std::uint64_t trace_bin_ms = 1000;        // ... one line per BIN of scores (a duration, default 1 s)
    std::optional<std::uint64_t> discover_ms; // extension: --discover DUR[:HOP], no snippet: what the first FILE shares with itself and with every further FILE (am_discover)
    std::uint64_t discover_hop_ms = 0;        // ... the hop between probes (default DUR / 2)
    float discover_min_ncc = 0.6f;            // ... --discover-min-ncc X: what a probe must score to count
    bool discover_min_ncc_set = false;
    std::string discover_out;                 // ... --discover-out PREFIX: each region's samples of the first FILE as PREFIX<file index>_<a_start>.wav; empty = off
    std::optional<double> envelope_pct;       // extension: --envelope PCT[:STEPS[:MIN_SCORE]], occurrences at another speed, found through band-level envelopes (am_match_envelope)
    std::uint32_t envelope_steps = 20;        // ... drifts -PCT % .. PCT % in 2 STEPS + 1 steps
    float envelope_min_score = 0.4f;          // ... what an envelope hit must score
    std::optional<std::uint64_t> edges_ms;    // extension: --edges DUR[:MIN_NCC[:MAX_SECOND]], a snippet cut off by the file's start or end (am_match_edges); DUR: the least overlap
    float edges_min_ncc = 0.5f;               // ... what an edge record must score
    float edges_max_second = 0.5f;            // ... and its runner-up at most this share of it
    std::vector<std::pair<std::uint64_t, std::uint64_t>> ignore_ms;   // extension: --ignore FROM-TO (repeatable), spans of the snippet to ignore, from its start (am_needle_create_masked)
    bool mask_report = false;                 // extension: --mask-report, one am_hit_mask line per hit
    bool live = false;                        // extension: --live, raw PCM from stdin through a monitor (am_monitor_*)
    std::uint32_t rate = 0;                   // --live: --rate R (samples per second of the stream)
    std::string encoding = "s16le";           // --live: --encoding s16le | f32le
    int channels = 2;                         // --live: --channels 1 | 2
    bool help = false;                        // --help

    std::uint64_t chunk_size_ms() const { return chunk_ms.value_or(60ull * 1000); }
    std::uint64_t distance_msec() const { return distance_ms.value_or(8ull * 60 * 1000); }
};

struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };

inline const char* usage_text() {
    return "usage: audiomatch <FILE>... --snippet <FILE> [--snippet <FILE>]... [options]\n"
           "  --snippet FILE         the snippet to find; give it several times to find several snippets (of any\n"
           "                         lengths) in one pass per file: each uses an overlap of its own length, the offset\n"
           "                         lines are prefixed by the snippet's file name, the label file is made from the hits\n"
           "                         of all snippets sorted by start (equal starts in --snippet order); --resample and\n"
           "                         --min-confidence apply to each snippet, --normalize matches them one by one\n"
           "  -p, --prominence P     minimal prominence of a hit, in percent (default 13)\n"
           "  --distance D           minimal distance between hits (default 8m)\n"
           "  --best N               the N best hits of each file instead of those above the prominence (whole file\n"
           "                         in one piece, hits at least --distance apart, in whole seconds)\n"
           "  --chunk-size D         length of one chunk (default 60s)\n"
           "  -o, --out FILE         label file (one input file only); --no-out: none\n"
           "  --dry-run              print the label file instead of writing it\n"
           "  --skip-existing        skip inputs whose label file exists\n"
           "  -y, --yes / -n, --no   answer questions without asking\n"
           "  --silent, --debug, --trace   output level\n"
           "  --device N             GPU ordinal (default 0)\n"
           "  --normalize            score every offset by normalised cross-correlation (NCC): the correlation divided\n"
           "                         by the energies of the snippet AND of the window it is compared with, in [-1, 1].\n"
           "                         Hits no longer depend on the recording's level; the prominence is then a fraction\n"
           "                         of a perfect match, not of the snippet's energy (default: off)\n"
           "  --normalize-floor DB   with --normalize: windows more than DB decibels below the snippet's energy score 0\n"
           "                         (0..200, default 60)\n"
           "  --ignore FROM-TO       ignore the span FROM-TO of the snippet (two durations from its start; may be given up\n"
           "                         to 15 times): the part of a jingle that changes from one occurrence to the next.  With\n"
           "                         --normalize the score is the NCC over the rest of the snippet only, whatever lies under\n"
           "                         the span; --min-confidence then filters by the exact NCC over the rest (am_hit_mask's), the\n"
           "                         other per-hit reports read the snippet with zeros in the span against everything under\n"
           "                         it.  Not with --resample, --whiten, --preemphasis, --envelope, --edges, --live or\n"
           "                         several --snippet\n"
           "  --mask-report          with --ignore: under each hit, its exact NCC over the kept part and what its ignored\n"
           "                         spans hold against the snippet's own samples there (am_hit_mask)\n"
           "  --min-confidence X     drop every hit whose normalised cross-correlation with the snippet, computed\n"
           "                         exactly for the hit's own window, is below X (0..1); with --debug, print each\n"
           "                         hit's position, ncc, gain and window level (default: keep every hit)\n"
           "  --segments M[:R]       after each hit's offset line, print which of M equal parts of the snippet the hit\n"
           "                         holds ('#' present, '.' absent: the part's NCC against --min-confidence if given,\n"
           "                         else 0.5), the covered fraction, the drift in ppm and the refined start's lag;\n"
           "                         each part is matched within R samples (0..16, default 4); M in 1..1024\n"
           "  --warp PPM[:STEPS[:RADIUS]]  for hits that run on another clock: after each hit's offset line, print its\n"
           "                         clock drift in ppm (positive: the occurrence is longer than the snippet), its refined\n"
           "                         lag in samples, the NCC with the drift taken out and the NCC as found; drifts -PPM ..\n"
           "                         PPM in 2 STEPS + 1 steps (STEPS in 1..32, default 8), lags -RADIUS .. RADIUS (0..16,\n"
           "                         default 4); PPM up to 50000.  --min-confidence then applies to the corrected NCC and\n"
           "                         --learn-needle cuts its rows on the snippet's clock.  Does not apply with --live\n"
           "  --channel P[:NOISE_DB] for hits that went through another chain (an EQ, a codec, an echo): after each hit's\n"
           "                         offset line, print the plain NCC, the NCC against the snippet filtered by the hit's own\n"
           "                         least-squares taps -P .. P (P in 0..128), the filter's gain and the unexplained share of\n"
           "                         the span in dB, the lag of the largest tap and its share of the taps' energy; NOISE_DB\n"
           "                         (0..200, default 60) steadies the solve.  Does not apply with --live\n"
           "  --residual PREFIX      with --channel: for each printed hit write PREFIX<file index>_<start>.wav, the hit's\n"
           "                         span (P samples each side) minus the filtered snippet: what lies over or under the\n"
           "                         jingle; mono 32-bit float, samples outside the file as 0.  Not with --whiten or\n"
           "                         --preemphasis, nor for a file whose rate differs from the snippet's\n"
           "  --mix M                what a 16-bit two-channel file (main file or snippet) is matched as: left, right, mid\n"
           "                         (the default: the down-mix (l + r) / 2), side ((l - r) / 2: finds an insert that sits\n"
           "                         polarity-inverted in the two channels and cancels in the down-mix), or A,B for\n"
           "                         A l + B r.  Refused for a mono or float file and with --live\n"
           "  --stereo R[:MIN_NCC]   after each hit's offset line, print where the hit sits between the channels of the\n"
           "                         16-bit two-channel main file: the image (centre, left, right, panned, inverted or\n"
           "                         absent), the NCC of the left and the right channel (the sign is the polarity), of the\n"
           "                         side signal and of the best fixed mix, the balance in dB, the delay between the\n"
           "                         channels in frames (lags -R .. R, R in 0..16) and what the down-mix cost in dB; a\n"
           "                         channel counts when its |NCC| reaches MIN_NCC (default 0.5).  Not with --live,\n"
           "                         --resample, --whiten or --preemphasis\n"
           "  --bands B[:LOG2F]      after each hit's offset line, print which of B log-spaced frequency bands of the\n"
           "                         snippet (50 Hz up to 16 kHz or half the sample rate) the hit holds ('#' present,\n"
           "                         '.' absent: the band's coherence against --min-confidence if given, else 0.5),\n"
           "                         the share of the snippet's energy in the bands held, the share-weighted coherence\n"
           "                         and the spread of the bands' gains in dB; spectra of 2^LOG2F samples (8..12,\n"
           "                         default 11); B in 1..32.  Does not apply with --live\n"
           "  --min-significance Z   drop every hit that stands less than Z standard deviations above the scores around\n"
           "                         it (its z: the hit's score minus the mean of the background scores, over their\n"
           "                         standard deviation; the background is every offset within --significance-zone of\n"
           "                         the hit and at least one snippet length away from it).  Applies to files, to\n"
           "                         several --snippet and with --best, not with --live; with --debug, print each\n"
           "                         hit's score, background mean and std, z and the largest background score with\n"
           "                         its lag (default: keep every hit)\n"
           "  --significance-zone D  how far the background reaches each side of a hit, a duration (default: three\n"
           "                         snippet lengths; at most 4194304 samples)\n"
           "  --resample             match main files of any sample rate: the snippet is resampled to each file's rate\n"
           "                         (scipy's resample_poly filter); without it, a rate mismatch stops the run\n"
           "  --whiten P             match in coloured material (speech, music): one prediction-error filter of order P\n"
           "                         (1..64) is designed from all main files of the run and applied to the snippets\n"
           "                         (after --resample) and to every main file before matching; offsets do not move,\n"
           "                         scores are those of the whitened signals.  Does not apply with --live\n"
           "  --preemphasis A        the fixed filter y[i] = x[i] - A x[i-1] (0 < A < 1) on the snippets and on every main\n"
           "                         file instead; not together with --whiten.  Does not apply with --live\n"
           "  --learn-needle OUT.wav[:mean|median|trimmed=P]\n"
           "                         after the run, write a cleaner snippet estimated from its hits: every reported hit of\n"
           "                         every main file is brought to the snippet's level (1 / gain of its exact score),\n"
           "                         the hits are stacked and each sample becomes their median (default), their mean, or\n"
           "                         their mean without the P permille (0..500) largest and smallest values; what lies over\n"
           "                         fewer than half of the hits is gone from a median.  OUT.wav is mono 32-bit float at\n"
           "                         the main files' rate (one rate for all) and can be the next run's --snippet.  Median\n"
           "                         and trimmed use the 64 hits of highest NCC.  One line per second of the result shows\n"
           "                         the spread between the hits relative to the result's peak: where they agree.  One\n"
           "                         --snippet only; not with --live, --best, --whiten or --preemphasis\n"
           "  --learn-margin D       with --learn-needle: also read D (a duration, default 0) in front of and behind the\n"
           "                         snippet; the spread shows where the jingle really begins and ends\n"
           "  --score-trace PREFIX[:BIN]  what the scores look like between the hits (am_match_trace): per main file (and\n"
           "                         per snippet, when there are several) PREFIX<file index>[_<snippet index>].csv with one\n"
           "                         line per BIN (a duration, default 1s) of scores: start_s, max, max_at_s, min, min_at_s,\n"
           "                         mean, rms, count ('nan' where a bin holds no score); and under the file's offset lines\n"
           "                         one line 'Trace: max V at hh:mm:ss.mmm, bin maxima median V mad V, peak z V'.  The\n"
           "                         scores are those that were matched: --normalize, --resample, --whiten / --preemphasis\n"
           "                         and --mix apply.  Not with --live\n"
           "  --envelope PCT[:STEPS[:MIN_SCORE]]  also find occurrences that run at another speed (a playout machine a few\n"
           "                         percent fast, a tape transfer) or whose phases are scrambled, which no waveform match\n"
           "                         sees: the snippet's band-level envelope (8 log bands from 150 Hz to 6 kHz or 0.45 of\n"
           "                         the sample rate, frames of 1024 samples) is matched against the file's at the lengths\n"
           "                         -PCT .. +PCT percent (up to 25) in 2 STEPS + 1 steps (STEPS in 1..128, default 20); under\n"
           "                         a snippet's offset lines one line per place that scores at least MIN_SCORE (-1..1,\n"
           "                         default 0.4): 'Envelope: hh:mm:ss.mmm speed +S % score V' (speed: that of the\n"
           "                         occurrence against the snippet).  The start is good to a few frames and the speed to a\n"
           "                         step or two, less for snippets of a few seconds.  Such places go into the label file\n"
           "                         unless a hit lies within half a snippet of them.  Not with --live or --discover\n"
           "  --edges DUR[:MIN_NCC[:MAX_SECOND]]  also look for the snippet cut off by the file's start or by its end\n"
           "                         (am_match_edges): the overlap must be at least DUR (a duration) and hold 5 % of the\n"
           "                         snippet's energy; an edge counts when its score over the part of the snippet inside the\n"
           "                         file is at least MIN_NCC (default 0.5) and its runner-up at most MAX_SECOND (default 0.5)\n"
           "                         of that.  After the file's offset lines one line per such edge, 'Offset head: -hh:mm:ss.mmm\n"
           "                         with ncc V overlap P %' (where the snippet would start; negative: before the file) or\n"
           "                         'Offset tail: ...', and in the label file a label 'head P %' / 'tail P %' over the part\n"
           "                         of the file the snippet covers.  Not with --live or --discover\n"
           "  --discover DUR[:HOP]   no --snippet: find what the first FILE shares with itself and with every further FILE\n"
           "                         (am_discover): probes of DUR (a duration) every HOP (default DUR/2) of the first FILE\n"
           "                         are matched under NCC, and probes that agree on one displacement (within HOP/8, at\n"
           "                         least 2 of them, gaps of 1 bridged, probes 40 dB below the file's level skipped) form\n"
           "                         a region; one line per region: 'Region: hh:mm:ss.mmm +LENGTHs -> FILE hh:mm:ss.mmm,\n"
           "                         ncc mean V min V, G/N probes'.  A repeat inside the first FILE is reported once.  No\n"
           "                         label file is written.  Not with --snippet, --live, --best, --score-trace or any\n"
           "                         per-hit option; --resample, --whiten, --preemphasis, --distance, --chunk-size, --out,\n"
           "                         --dry-run and --skip-existing do not apply (an error); --normalize is what discovery\n"
           "                         does anyway, --prominence has nothing to act on; --mix and --normalize-floor apply\n"
           "  --discover-min-ncc X   with --discover: the NCC a probe must reach to count (default 0.6)\n"
           "  --discover-out PREFIX  with --discover: write the first FILE's samples of each region as\n"
           "                         PREFIX<file index>_<start sample>.wav (file index 0: the first FILE against itself),\n"
           "                         usable as --snippet as they are\n"
           "  --live                 read raw PCM from stdin instead of files (no FILE arguments): a live feed, matched\n"
           "                         as it arrives; each hit's offset line is printed (and flushed) as soon as it is\n"
           "                         final -- a hit is final once the next hit is found, or once --distance of audio\n"
           "                         has passed behind it, so use a short --distance for monitoring.  At end of input\n"
           "                         the label file (-o FILE; none without -o) is written as for a file.  Needs --rate;\n"
           "                         --best, --normalize, --min-confidence and --segments do not apply, nor do\n"
           "                         --min-significance and --significance-zone\n"
           "  --rate R               --live: sample rate of the stream, in Hz\n"
           "  --encoding E           --live: s16le (default) or f32le (f32le: one channel only)\n"
           "  --channels C           --live: 1 or 2 (default 2)\n"
           "  --help                 this text\n";
}

inline Arguments parse_arguments(int argc, const char* const* argv) {
    Arguments a;
    auto need = [&](int& i) -> std::string {
        if (i + 1 >= argc) throw ArgError(std::string("missing value for ") + argv[i]);
        return argv[++i];
    };
    auto dur = [&](const std::string& v, const char* flag) {
        auto d = parse_duration_ms(v);
        if (!d) throw ArgError(std::string("invalid duration '") + v + "' for " + flag);
        return *d;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s == "--snippet") {
            a.snippets.push_back(need(i));
            if (a.snippets.size() == 1) a.snippet = a.snippets[0];
        }
        else if (s == "-p" || s == "--prominence") a.prominence = std::strtof(need(i).c_str(), nullptr);
        else if (s == "--distance") a.distance_ms = dur(need(i), "--distance");
        else if (s == "--chunk-size") a.chunk_ms = dur(need(i), "--chunk-size");
        else if (s == "--fancy-bar") a.fancy_bar = true;
        else if (s == "--dry-run") a.dry_run = true;
        else if (s == "--skip-existing") a.skip_existing = true;
        else if (s == "--no-out") a.no_out = true;
        else if (s == "-o" || s == "--out") a.out_file = need(i);
        else if (s == "-y" || s == "--yes") a.always_answer = 1;
        else if (s == "-n" || s == "--no") a.always_answer = 0;
        else if (s == "--silent" || s == "--quiet") a.verbosity = 0;
        else if (s == "--debug") a.verbosity = 2;
        else if (s == "--trace") a.verbosity = 3;
        else if (s == "--device") a.device = std::atoi(need(i).c_str());
        else if (s == "--normalize") a.normalize = true;
        else if (s == "--normalize-floor") {
            const std::string v = need(i);
            char* end = nullptr;
            const long db = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || db < 0 || db > 200)
                throw ArgError("invalid value '" + v + "' for --normalize-floor (whole decibels, 0..200)");
            a.normalize_floor_db = (int)db;
        }
        else if (s == "--min-confidence") {
            const std::string v = need(i);
            char* end = nullptr;
            const float x = std::strtof(v.c_str(), &end);
            if (v.empty() || *end != '\0' || !(x >= 0.0f && x <= 1.0f))
                throw ArgError("invalid value '" + v + "' for --min-confidence (a number in 0..1)");
            a.min_confidence = x;
        }
        else if (s == "--min-significance") {
            const std::string v = need(i);
            char* end = nullptr;
            const float z = std::strtof(v.c_str(), &end);
            if (v.empty() || *end != '\0' || !(z == z) || z > 3.0e38f || z < -3.0e38f)
                throw ArgError("invalid value '" + v + "' for --min-significance (a number of standard deviations)");
            a.min_significance = z;
        }
        else if (s == "--significance-zone") {
            const std::uint64_t d = dur(need(i), "--significance-zone");
            if (d == 0) throw ArgError("invalid duration '0' for --significance-zone (must be longer than 0)");
            a.significance_zone_ms = d;
        }
        else if (s == "--segments") {
            const std::string v = need(i);
            const std::size_t colon = v.find(':');
            const std::string vm = v.substr(0, colon), vr = colon == std::string::npos ? "4" : v.substr(colon + 1);
            auto whole = [](const std::string& t, unsigned long& x) {
                char* end = nullptr;
                x = std::strtoul(t.c_str(), &end, 10);
                return !t.empty() && t[0] >= '0' && t[0] <= '9' && *end == '\0';
            };
            unsigned long m = 0, r = 0;
            if (!whole(vm, m) || !whole(vr, r) || m == 0 || m > 1024 || r > 16)
                throw ArgError("invalid value '" + v + "' for --segments (M[:R], M in 1..1024 parts, R in 0..16 samples)");
            a.segments = (std::uint32_t)m;
            a.segment_radius = (std::uint32_t)r;
        }
        else if (s == "--warp") {
            const std::string v = need(i);
            const std::size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            const std::string vp = v.substr(0, c1);
            const std::string vs = c1 == std::string::npos ? "8" : v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
            const std::string vr = c2 == std::string::npos ? "4" : v.substr(c2 + 1);
            auto whole = [](const std::string& t, unsigned long& x) {
                char* end = nullptr;
                x = std::strtoul(t.c_str(), &end, 10);
                return !t.empty() && t[0] >= '0' && t[0] <= '9' && *end == '\0';
            };
            char* end = nullptr;
            const double ppm = std::strtod(vp.c_str(), &end);
            unsigned long k = 0, r = 0;
            if (vp.empty() || *end != '\0' || !(ppm > 0.0) || ppm > AM_WARP_MAX_PPM || !whole(vs, k) || !whole(vr, r) || k == 0 ||
                k > AM_WARP_MAX_STEPS || r > AM_SEG_MAX_RADIUS)
                throw ArgError("invalid value '" + v + "' for --warp (PPM[:STEPS[:RADIUS]], PPM above 0 up to 50000, STEPS in 1..32, RADIUS in 0..16)");
            a.warp_ppm = ppm;
            a.warp_steps = (std::uint32_t)k;
            a.warp_radius = (std::uint32_t)r;
        }
        else if (s == "--channel") {
            const std::string v = need(i);
            const std::size_t colon = v.find(':');
            const std::string vp = v.substr(0, colon), vn = colon == std::string::npos ? "60" : v.substr(colon + 1);
            char* end = nullptr;
            const unsigned long p = std::strtoul(vp.c_str(), &end, 10);
            const bool p_ok = !vp.empty() && vp[0] >= '0' && vp[0] <= '9' && *end == '\0' && p <= AM_CHAN_MAX_RADIUS;
            const double db = std::strtod(vn.c_str(), &end);
            if (!p_ok || vn.empty() || *end != '\0' || !(db >= 0.0 && db <= 200.0))
                throw ArgError("invalid value '" + v + "' for --channel (P[:NOISE_DB], P in 0..128 taps each side, NOISE_DB in 0..200)");
            a.channel_radius = (std::uint32_t)p;
            a.channel_noise_db = db;
        }
        else if (s == "--residual") {
            a.residual_prefix = need(i);
            if (a.residual_prefix.empty()) throw ArgError("invalid value '' for --residual (a file name prefix)");
        }
        else if (s == "--mix") {
            const std::string v = need(i);
            a.mix_set = true;
            if (v == "left") { a.mix_a = 1.0f; a.mix_b = 0.0f; }
            else if (v == "right") { a.mix_a = 0.0f; a.mix_b = 1.0f; }
            else if (v == "mid") { a.mix_a = 0.5f; a.mix_b = 0.5f; }
            else if (v == "side") { a.mix_a = 0.5f; a.mix_b = -0.5f; }
            else {
                const std::size_t comma = v.find(',');
                const std::string va = v.substr(0, comma), vb = comma == std::string::npos ? "" : v.substr(comma + 1);
                char *ea = nullptr, *eb = nullptr;
                const float fa = std::strtof(va.c_str(), &ea), fb = std::strtof(vb.c_str(), &eb);
                if (va.empty() || vb.empty() || *ea != '\0' || *eb != '\0' || !std::isfinite(fa) || !std::isfinite(fb))
                    throw ArgError("invalid value '" + v + "' for --mix (left, right, mid, side or A,B)");
                a.mix_a = fa;
                a.mix_b = fb;
            }
        }
        else if (s == "--stereo") {
            const std::string v = need(i);
            const std::size_t colon = v.find(':');
            const std::string vr = v.substr(0, colon), vm = colon == std::string::npos ? "0.5" : v.substr(colon + 1);
            char* end = nullptr;
            const unsigned long r = std::strtoul(vr.c_str(), &end, 10);
            const bool r_ok = !vr.empty() && vr[0] >= '0' && vr[0] <= '9' && *end == '\0' && r <= AM_STEREO_MAX_RADIUS;
            const float mn = std::strtof(vm.c_str(), &end);
            if (!r_ok || vm.empty() || *end != '\0' || !(mn >= 0.0f && mn <= 1.0f))
                throw ArgError("invalid value '" + v + "' for --stereo (R[:MIN_NCC], R in 0..16 lags each side, MIN_NCC in 0..1)");
            a.stereo_radius = (std::uint32_t)r;
            a.stereo_min_ncc = mn;
        }
        else if (s == "--bands") {
            const std::string v = need(i);
            const std::size_t colon = v.find(':');
            const std::string vb = v.substr(0, colon), vf = colon == std::string::npos ? "11" : v.substr(colon + 1);
            auto whole = [](const std::string& t, unsigned long& x) {
                char* end = nullptr;
                x = std::strtoul(t.c_str(), &end, 10);
                return !t.empty() && t[0] >= '0' && t[0] <= '9' && *end == '\0';
            };
            unsigned long b = 0, lf = 0;
            if (!whole(vb, b) || !whole(vf, lf) || b == 0 || b > 32 || lf < 8 || lf > 12)
                throw ArgError("invalid value '" + v + "' for --bands (B[:LOG2F], B in 1..32 bands, LOG2F in 8..12)");
            a.bands = (std::uint32_t)b;
            a.band_frame_log2 = (std::uint32_t)lf;
        }
        else if (s == "--resample") a.resample = true;
        else if (s == "--ignore") {
            const std::string v = need(i);
            const auto dash = v.find('-');
            const auto from = parse_duration_ms(v.substr(0, dash));
            const auto to = dash == std::string::npos ? std::nullopt : parse_duration_ms(v.substr(dash + 1));
            if (!from || !to || *from >= *to) throw ArgError("invalid value '" + v + "' for --ignore (FROM-TO, two durations from the snippet's start, FROM before TO)");
            a.ignore_ms.emplace_back(*from, *to);
        }
        else if (s == "--mask-report") a.mask_report = true;
        else if (s == "--whiten") {
            const std::string v = need(i);
            char* end = nullptr;
            const unsigned long p = std::strtoul(v.c_str(), &end, 10);
            if (v.empty() || v[0] < '0' || v[0] > '9' || *end != '\0' || p < 1 || p > AM_WHITEN_MAX_ORDER)
                throw ArgError("invalid value '" + v + "' for --whiten (the filter's order, 1..64)");
            a.whiten = (std::uint32_t)p;
        }
        else if (s == "--preemphasis") {
            const std::string v = need(i);
            char* end = nullptr;
            const float x = std::strtof(v.c_str(), &end);
            if (v.empty() || *end != '\0' || !(x > 0.0f && x < 1.0f))
                throw ArgError("invalid value '" + v + "' for --preemphasis (a number with 0 < A < 1)");
            a.preemphasis = x;
        }
        else if (s == "--learn-needle") {
            const std::string v = need(i);
            const std::size_t colon = v.rfind(':');
            a.learn_needle = v.substr(0, colon);
            const std::string m = colon == std::string::npos ? "median" : v.substr(colon + 1);
            bool ok = !a.learn_needle.empty();
            if (m == "median") a.learn_method = AM_EST_MEDIAN;
            else if (m == "mean") a.learn_method = AM_EST_MEAN;
            else if (m.rfind("trimmed=", 0) == 0) {
                const std::string t = m.substr(8);
                char* end = nullptr;
                const unsigned long pm = std::strtoul(t.c_str(), &end, 10);
                ok = ok && !t.empty() && t[0] >= '0' && t[0] <= '9' && *end == '\0' && pm <= 500;
                a.learn_method = AM_EST_TRIMMED;
                a.learn_trim = (std::uint32_t)pm;
            }
            else ok = false;
            if (!ok) throw ArgError("invalid value '" + v + "' for --learn-needle (OUT.wav[:mean|median|trimmed=P], P in 0..500 permille)");
        }
        else if (s == "--learn-margin") a.learn_margin_ms = dur(need(i), "--learn-margin");
        else if (s == "--best") {
            const std::string v = need(i);
            char* end = nullptr;
            const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v[0] == '-' || *end != '\0' || k == 0)
                throw ArgError("invalid value '" + v + "' for --best (a whole number of hits, at least 1)");
            a.best = (std::uint64_t)k;
        }
        else if (s == "--score-trace") {
            // PREFIX[:BIN]: what follows the last ':' is the bin when it reads as a duration (a prefix may hold ':' itself)
            const std::string v = need(i);
            a.trace_prefix = v;
            const auto colon = v.rfind(':');
            if (colon != std::string::npos) {
                if (const auto d = parse_duration_ms(v.substr(colon + 1))) {
                    a.trace_prefix = v.substr(0, colon);
                    a.trace_bin_ms = *d;
                }
            }
            if (a.trace_prefix.empty() || a.trace_bin_ms == 0)
                throw ArgError("invalid value '" + v + "' for --score-trace (PREFIX[:BIN], a file name prefix and a duration longer than 0)");
        }
        else if (s == "--envelope") {
            const std::string v = need(i);
            const std::size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            const std::string vp = v.substr(0, c1);
            const std::string vs = c1 == std::string::npos ? "20" : v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
            const std::string vm = c2 == std::string::npos ? "0.4" : v.substr(c2 + 1);
            char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
            const double pct = std::strtod(vp.c_str(), &e1);
            const unsigned long k = std::strtoul(vs.c_str(), &e2, 10);
            const float ms = std::strtof(vm.c_str(), &e3);
            if (vp.empty() || *e1 != '\0' || !(pct > 0.0) || pct > AM_ENV_MAX_PPM * 1e-4 || vs.empty() || vs[0] < '0' || vs[0] > '9' || *e2 != '\0' ||
                k == 0 || k > AM_ENV_MAX_STEPS || vm.empty() || *e3 != '\0' || !(ms >= -1.0f && ms <= 1.0f))
                throw ArgError("invalid value '" + v + "' for --envelope (PCT[:STEPS[:MIN_SCORE]], PCT above 0 up to 25, STEPS in 1..128, MIN_SCORE in -1..1)");
            a.envelope_pct = pct;
            a.envelope_steps = (std::uint32_t)k;
            a.envelope_min_score = ms;
        }
        else if (s == "--edges") {
            const std::string v = need(i);
            const std::size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            const auto d = parse_duration_ms(v.substr(0, c1));
            const std::string vn = c1 == std::string::npos ? "0.5" : v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
            const std::string vm = c2 == std::string::npos ? "0.5" : v.substr(c2 + 1);
            char *e1 = nullptr, *e2 = nullptr;
            const float mn = std::strtof(vn.c_str(), &e1), mx = std::strtof(vm.c_str(), &e2);
            if (!d || *d == 0 || vn.empty() || *e1 != '\0' || !(mn >= -1.0f && mn <= 1.0f) || vm.empty() || *e2 != '\0' || !(mx >= 0.0f && mx <= 1.0f))
                throw ArgError("invalid value '" + v + "' for --edges (DUR[:MIN_NCC[:MAX_SECOND]], a duration longer than 0, MIN_NCC in -1..1, MAX_SECOND in 0..1)");
            a.edges_ms = *d;
            a.edges_min_ncc = mn;
            a.edges_max_second = mx;
        }
        else if (s == "--discover") {
            const std::string v = need(i);
            const auto colon = v.find(':');
            const auto d = parse_duration_ms(v.substr(0, colon));
            const auto h = colon == std::string::npos ? std::optional<std::uint64_t>(d ? *d / 2 : 0) : parse_duration_ms(v.substr(colon + 1));
            if (!d || !h || *d == 0 || *h == 0)
                throw ArgError("invalid value '" + v + "' for --discover (DUR[:HOP], two durations longer than 0)");
            a.discover_ms = *d;
            a.discover_hop_ms = *h;
        }
        else if (s == "--discover-min-ncc") {
            const std::string v = need(i);
            char* end = nullptr;
            const float x = std::strtof(v.c_str(), &end);
            if (v.empty() || *end || !(x >= -1.0f && x <= 1.0f))
                throw ArgError("invalid value '" + v + "' for --discover-min-ncc (a number in -1 .. 1)");
            a.discover_min_ncc = x;
            a.discover_min_ncc_set = true;
        }
        else if (s == "--discover-out") {
            a.discover_out = need(i);
            if (a.discover_out.empty()) throw ArgError("invalid value '' for --discover-out (a file name prefix)");
        }
        else if (s == "--live") a.live = true;
        else if (s == "--rate") {
            const std::string v = need(i);
            char* end = nullptr;
            const unsigned long r = std::strtoul(v.c_str(), &end, 10);
            if (v.empty() || v[0] == '-' || *end != '\0' || r == 0 || r > 4000000)
                throw ArgError("invalid value '" + v + "' for --rate (samples per second, 1..4000000)");
            a.rate = (std::uint32_t)r;
        }
        else if (s == "--encoding") {
            a.encoding = need(i);
            if (a.encoding != "s16le" && a.encoding != "f32le") throw ArgError("invalid value '" + a.encoding + "' for --encoding (s16le or f32le)");
        }
        else if (s == "--channels") {
            const std::string v = need(i);
            if (v != "1" && v != "2") throw ArgError("invalid value '" + v + "' for --channels (1 or 2)");
            a.channels = v[0] - '0';
        }
        else if (s == "-h" || s == "--help") { a.help = true; return a; }
        else if (!s.empty() && s[0] == '-' && s != "-") throw ArgError("unknown option " + s);
        else if (!s.empty()) a.within.push_back(s);
    }
    if (a.discover_ms) {
        // (no needle in this mode: nothing that takes one, or the hits of one, applies)
        const std::pair<bool, const char*> others[] = {
            {!a.snippet.empty(), "--snippet"}, {a.live, "--live"}, {a.best.has_value(), "--best"}, {!a.trace_prefix.empty(), "--score-trace"},
            {a.min_confidence.has_value(), "--min-confidence"}, {a.segments != 0, "--segments"}, {a.bands != 0, "--bands"},
            {a.warp_ppm.has_value(), "--warp"}, {a.channel_radius.has_value(), "--channel"}, {!a.residual_prefix.empty(), "--residual"},
            {a.stereo_radius.has_value(), "--stereo"}, {a.min_significance.has_value(), "--min-significance"},
            {a.significance_zone_ms.has_value(), "--significance-zone"}, {!a.learn_needle.empty(), "--learn-needle"},
            {a.envelope_pct.has_value(), "--envelope"}, {a.edges_ms.has_value(), "--edges"}};
        for (const auto& o : others)
            if (o.first) throw ArgError(std::string("--discover and ") + o.second + " are mutually exclusive");
        // ... and what would be ignored without a word (--normalize is what discovery does anyway; --mix and
        // --normalize-floor apply)
        const std::pair<bool, const char*> ignored[] = {
            {a.resample, "--resample"}, {a.whiten != 0, "--whiten"}, {a.preemphasis.has_value(), "--preemphasis"},
            {a.learn_margin_ms.has_value(), "--learn-margin"}, {a.out_file.has_value(), "--out"}, {a.distance_ms.has_value(), "--distance"},
            {a.chunk_ms.has_value(), "--chunk-size"}, {a.dry_run, "--dry-run"}, {a.skip_existing, "--skip-existing"}};
        for (const auto& o : ignored)
            if (o.first) throw ArgError(std::string("--discover: ") + o.second + " does not apply");
        if (a.within.empty()) throw ArgError("--discover needs at least one FILE");
        return a;
    }
    if (a.discover_min_ncc_set) throw ArgError("--discover-min-ncc needs --discover");
    if (!a.discover_out.empty()) throw ArgError("--discover-out needs --discover");
    if (a.snippet.empty()) throw ArgError("--snippet <FILE> is required");
    if (a.whiten && a.preemphasis) throw ArgError("--whiten and --preemphasis are mutually exclusive");
    if (a.learn_margin_ms && a.learn_needle.empty()) throw ArgError("--learn-margin needs --learn-needle");
    if (!a.residual_prefix.empty() && !a.channel_radius) throw ArgError("--residual needs --channel");
    if (!a.residual_prefix.empty() && (a.whiten || a.preemphasis))
        throw ArgError("--residual does not apply with --whiten or --preemphasis (the span would be that of the filtered signal)");
    if (a.stereo_radius && (a.resample || a.whiten || a.preemphasis))
        throw ArgError("--stereo does not apply with --resample, --whiten or --preemphasis (the snippet would no longer be on the frames' footing)");
    if (!a.ignore_ms.empty()) {
        // (a masked handle comes from am_needle_create_masked only, and these take or build another kind of needle)
        const std::pair<bool, const char*> no_mask[] = {
            {a.resample, "--resample"}, {a.whiten != 0, "--whiten"}, {a.preemphasis.has_value(), "--preemphasis"},
            {a.envelope_pct.has_value(), "--envelope"}, {a.edges_ms.has_value(), "--edges"}, {a.live, "--live"},
            {a.snippets.size() > 1, "several --snippet"}};
        for (const auto& o : no_mask)
            if (o.first) throw ArgError(std::string("--ignore and ") + o.second + " are mutually exclusive");
        if (a.ignore_ms.size() > AM_MASK_MAX_GAPS) throw ArgError("--ignore: at most " + std::to_string(AM_MASK_MAX_GAPS) + " spans");
    }
    if (a.mask_report && a.ignore_ms.empty()) throw ArgError("--mask-report needs --ignore");
    if (a.live && a.mix_set) throw ArgError("--live: --mix does not apply");
    if (a.live && a.stereo_radius) throw ArgError("--live: --stereo does not apply");
    if (a.live && !a.trace_prefix.empty()) throw ArgError("--live: --score-trace does not apply");
    if (a.live && a.edges_ms) throw ArgError("--live: --edges does not apply");
    if (!a.learn_needle.empty()) {
        if (a.live) throw ArgError("--live: --learn-needle does not apply");
        if (a.best) throw ArgError("--learn-needle and --best are mutually exclusive");
        if (a.snippets.size() > 1) throw ArgError("--learn-needle takes one --snippet only");
        if (a.whiten || a.preemphasis) throw ArgError("--learn-needle does not apply with --whiten or --preemphasis (the hits would be those of the filtered signal)");
    }
    if (a.live) {
        if (!a.within.empty()) throw ArgError("--live reads stdin: no FILE arguments");
        if (a.rate == 0) throw ArgError("--live needs --rate");
        if (a.encoding == "f32le" && a.channels != 1) throw ArgError("--encoding f32le takes one channel only (--channels 1)");
        if (a.best || a.normalize || a.min_confidence) throw ArgError("--live: --best, --normalize and --min-confidence do not apply");
        if (a.segments) throw ArgError("--live: --segments does not apply");
        if (a.bands) throw ArgError("--live: --bands does not apply");
        if (a.warp_ppm) throw ArgError("--live: --warp does not apply");
        if (a.envelope_pct) throw ArgError("--live: --envelope does not apply");
        if (a.channel_radius) throw ArgError("--live: --channel does not apply");
        if (a.whiten || a.preemphasis) throw ArgError("--live: --whiten and --preemphasis do not apply (not supported on a live feed yet)");
        if (a.min_significance || a.significance_zone_ms) throw ArgError("--live: --min-significance and --significance-zone do not apply");
        return a;
    }
    if (a.no_out && a.out_file) throw ArgError("--no-out and --out are mutually exclusive");      // #[group(multiple = false)]
    if (a.out_file && a.within.size() != 1)
        throw ArgError("providet outfile only compatible with one main file");                     // matcher/mod.rs:20-26
    return a;
}

// ---- PCM input (WAV) -------------------------------------------------------------
struct Pcm {
    std::uint32_t sample_rate = 0;
    std::uint16_t channels = 0;
    bool is_float = false;
    std::vector<std::int16_t> s16;   // interleaved, when !is_float
    std::vector<float> f32;          // mono float, when is_float
    std::size_t frames() const { return is_float ? f32.size() : (channels ? s16.size() / channels : 0); }
};

inline Pcm read_wav(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("couldn't find file '" + path + "'");     // CliError::NoFile
    auto rd = [&](void* p, std::size_t n) { f.read(static_cast<char*>(p), (std::streamsize)n); return (std::size_t)f.gcount() == n; };
    char riff[12];
    if (!rd(riff, 12) || std::memcmp(riff, "RIFF", 4) || std::memcmp(riff + 8, "WAVE", 4))
        throw std::runtime_error("'" + path + "' is not a RIFF/WAVE file");
    Pcm pcm;
    std::uint16_t fmt = 0, bits = 0;
    bool have_fmt = false;
    for (;;) {
        char id[4]; std::uint32_t sz = 0;
        if (!rd(id, 4) || !rd(&sz, 4)) break;
        if (!std::memcmp(id, "fmt ", 4)) {
            std::vector<char> b(sz);
            if (!rd(b.data(), sz) || sz < 16) throw std::runtime_error("bad fmt chunk");
            std::memcpy(&fmt, &b[0], 2); std::memcpy(&pcm.channels, &b[2], 2);
            std::memcpy(&pcm.sample_rate, &b[4], 4); std::memcpy(&bits, &b[14], 2);
            if (fmt == 0xFFFE && sz >= 26) std::memcpy(&fmt, &b[24], 2);   // WAVE_FORMAT_EXTENSIBLE sub-format
            have_fmt = true;
        } else if (!std::memcmp(id, "data", 4)) {
            if (!have_fmt) throw std::runtime_error("data chunk before fmt chunk");
            if (fmt == 1 && bits == 16 && (pcm.channels == 1 || pcm.channels == 2)) {
                pcm.s16.resize(sz / 2);
                rd(pcm.s16.data(), (sz / 2) * 2);
            } else if (fmt == 3 && bits == 32 && pcm.channels == 1) {
                pcm.is_float = true;
                pcm.f32.resize(sz / 4);
                rd(pcm.f32.data(), (sz / 4) * 4);
            } else {
                throw std::runtime_error("unsupported WAV encoding (need PCM16 mono/stereo or float32 mono)");
            }
            return pcm;
        } else {
            f.seekg(sz + (sz & 1), std::ios::cur);
        }
    }
    throw std::runtime_error("'" + path + "' has no data chunk");
}

// mono 32-bit float WAV (format 3, with the fact chunk non-PCM formats carry): what read_wav reads back as is_float
inline void write_wav_f32(const std::string& path, const std::vector<float>& x, std::uint32_t sample_rate) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) throw std::runtime_error("couldn't write file '" + path + "'");
    const std::uint32_t data = (std::uint32_t)(x.size() * 4), n = (std::uint32_t)x.size(), riff = 4 + (8 + 16) + (8 + 4) + (8 + data);
    const std::uint32_t fmt_size = 16, fact_size = 4, byte_rate = sample_rate * 4;
    const std::uint16_t format = 3, channels = 1, block = 4, bits = 32;
    auto put = [&](const void* p, std::size_t k) { f.write(static_cast<const char*>(p), (std::streamsize)k); };
    put("RIFF", 4); put(&riff, 4); put("WAVE", 4);
    put("fmt ", 4); put(&fmt_size, 4); put(&format, 2); put(&channels, 2); put(&sample_rate, 4); put(&byte_rate, 4); put(&block, 2); put(&bits, 2);
    put("fact", 4); put(&fact_size, 4); put(&n, 4);
    put("data", 4); put(&data, 4); put(x.data(), data);
    if (!f) throw std::runtime_error("couldn't write file '" + path + "'");
}

// f32 mono samples as the matcher sees them: stereo i16 goes through the GPU
// down-mix (mp3_reader.rs:28-37); mono i16 is treated as l == r.
inline std::vector<float> to_mono_f32(const Pcm& pcm, int device) {
    if (pcm.is_float) return pcm.f32;
    std::vector<std::int16_t> stereo;
    const std::int16_t* src = pcm.s16.data();
    std::size_t frames = pcm.frames();
    if (pcm.channels == 1) {
        stereo.resize(frames * 2);
        for (std::size_t i = 0; i < frames; ++i) stereo[2 * i] = stereo[2 * i + 1] = pcm.s16[i];
        src = stereo.data();
    }
    std::vector<float> out(frames);
    if (frames) {
        const int rc = am_pcm_s16_stereo_to_mono(device, src, frames, out.data());
        if (rc != AM_OK) throw std::runtime_error(std::string("am_pcm_s16_stereo_to_mono: ") + am_last_error_string());
    }
    return out;
}

// extension: --mix.  f32 mono samples of a file under the run's mix: without --mix, and with `mid`, the down-mix above,
// byte for byte; otherwise a l + b r through am_pcm_s16_stereo_mix.  --mix is refused for a file that is not 16-bit
// two-channel (`path` names it).
inline std::vector<float> to_mono_f32(const Arguments& args, const Pcm& pcm, const std::string& path) {
    if (!args.mix_set) return to_mono_f32(pcm, args.device);
    if (pcm.is_float || pcm.channels != 2) throw std::runtime_error("--mix: '" + path + "' is not a 16-bit two-channel file");
    if (args.mix_a == 0.5f && args.mix_b == 0.5f) return to_mono_f32(pcm, args.device);
    std::vector<float> out(pcm.frames());
    if (!out.empty() && am_pcm_s16_stereo_mix(args.device, pcm.s16.data(), out.size(), args.mix_a, args.mix_b, out.data()) != AM_OK)
        throw std::runtime_error(std::string("am_pcm_s16_stereo_mix: ") + am_last_error_string());
    return out;
}

// ---- output ------------------------------------------------------------------------
// Rust's `{}` for f32: the shortest decimal that round-trips
inline std::string fmt_f32(float v) {
    char buf[64];
    for (int p = 1; p <= 9; ++p) {
        std::snprintf(buf, sizeof buf, "%.*g", p, (double)v);
        if (std::strtof(buf, nullptr) == v) break;
    }
    std::string s = buf;
    const auto e = s.find('e');
    if (e != std::string::npos) {   // Rust never prints an exponent for Display: expand it
        std::snprintf(buf, sizeof buf, "%.*f", 50, (double)v);
        s = buf;
        while (!s.empty() && s.back() == '0') s.pop_back();
        if (!s.empty() && s.back() == '.') s.pop_back();
    }
    return s;
}

// matcher/mod.rs:110-125: "Offset i: hh:mm:ss with prominence p"
inline std::string offset_line(const am_peak& peak, std::size_t i, std::uint32_t sr) {   // i counts from 0
    const double secs = (double)peak.start / (double)sr;     // start_as_duration (:127-129)
    const std::uint64_t whole = (std::uint64_t)secs;
    char buf[160];
    std::snprintf(buf, sizeof buf, "Offset %zu: %02" PRIu64 ":%02" PRIu64 ":%02" PRIu64 " with prominence %s", i + 1,
                  whole / 3600, (whole / 60) % 60, whole % 60, fmt_f32(peak.prominence).c_str());
    return buf;
}
inline std::vector<std::string> offset_lines(const am_peak* peaks, std::size_t n, std::uint32_t sr) {
    std::vector<std::string> out;
    if (n == 0) { out.push_back("no offsets found"); return out; }
    for (std::size_t i = 0; i < n; ++i) out.push_back(offset_line(peaks[i], i, sr));
    return out;
}

// extension: --envelope.  "Envelope: hh:mm:ss.mmm speed +S % score V": the speed of the occurrence against the snippet
inline std::string envelope_line(const am_env_hit& hit, std::uint32_t sr) {
    const std::uint64_t ms = (std::uint64_t)((double)hit.start * 1000.0 / (double)sr);
    char buf[160];
    std::snprintf(buf, sizeof buf, "Envelope: %02" PRIu64 ":%02" PRIu64 ":%02" PRIu64 ".%03" PRIu64 " speed %+.2f %% score %.3f", ms / 3600000,
                  (ms / 60000) % 60, (ms / 1000) % 60, ms % 1000, 100.0 * (1.0 / (1.0 + hit.drift_ppm * 1e-6) - 1.0), (double)hit.score);
    return buf;
}

struct TimeLabel { double start_s, end_s; std::string name; };

// extension: --edges.  An edge record counts when it has no flag but AM_EDGE_NO_SECOND, scores at least min_ncc and, where
// there is a runner-up, that scores at most max_second of it
inline bool edge_passes(const am_edge_hit& r, float min_ncc, float max_second) {
    if (r.flags & ~AM_EDGE_NO_SECOND) return false;
    if (!(r.ncc >= min_ncc)) return false;
    return (r.flags & AM_EDGE_NO_SECOND) || (double)r.ncc_second <= (double)max_second * (double)r.ncc;
}
inline const char* edge_tag(const am_edge_hit& r) { return r.edge == AM_EDGE_HEAD ? "head" : "tail"; }
inline int edge_percent(const am_edge_hit& r, std::size_t s_len) { return (int)std::llround(100.0 * (double)r.overlap / (double)s_len); }
// "Offset head: -hh:mm:ss.mmm with ncc V overlap P %": where the snippet would start, before the file when negative
inline std::string edge_line(const am_edge_hit& r, std::size_t s_len, std::uint32_t sr) {
    const std::uint64_t ms = (std::uint64_t)((double)(r.start < 0 ? -r.start : r.start) * 1000.0 / (double)sr);
    char buf[160];
    std::snprintf(buf, sizeof buf, "Offset %s: %s%02" PRIu64 ":%02" PRIu64 ":%02" PRIu64 ".%03" PRIu64 " with ncc %.3f overlap %d %%", edge_tag(r),
                  r.start < 0 ? "-" : "", ms / 3600000, (ms / 60000) % 60, (ms / 1000) % 60, ms % 1000, (double)r.ncc, edge_percent(r, s_len));
    return buf;
}
// the label of a counted edge: the part of the file the snippet covers, [max(0, start), min(len, start + S))
inline TimeLabel edge_label(const am_edge_hit& r, std::size_t s_len, std::size_t len, std::uint32_t sr) {
    const std::int64_t a = std::max<std::int64_t>(0, r.start), b = std::min<std::int64_t>((std::int64_t)len, r.start + (std::int64_t)s_len);
    return TimeLabel{(double)a / (double)sr, (double)b / (double)sr, std::string(edge_tag(r)) + " " + std::to_string(edge_percent(r, s_len)) + " %"};
}

// archive/data.rs:87-107: consecutive peak pairs -> [start_i + delay, start_{i+1}], name_pattern with '#' -> i (from 1)
inline std::vector<TimeLabel> timelabel_from_peaks(const am_peak* peaks, std::size_t n, std::uint32_t sr,
                                                   double delay_start_s, const std::string& name_pattern) {
    std::vector<TimeLabel> out;
    for (std::size_t i = 0; i + 1 < n; ++i) {
        TimeLabel t;
        t.start_s = (double)peaks[i].start / (double)sr + delay_start_s;
        t.end_s = (double)peaks[i + 1].start / (double)sr;
        t.name = name_pattern;
        std::string num = std::to_string(i + 1), rep;
        for (char c : t.name) { if (c == '#') rep += num; else rep += c; }
        t.name = rep;
        out.push_back(t);
    }
    return out;
}

inline std::string format_labels(const std::vector<TimeLabel>& labels) {
    std::string s;
    char buf[128];
    for (const auto& l : labels) {
        std::snprintf(buf, sizeof buf, "%.6f\t%.6f\t", l.start_s, l.end_s);
        s += buf; s += l.name; s += "\n";
    }
    return s;
}

// (secs * sr).round() as usize (audio_matcher.rs:99-100)
inline std::uint64_t round_samples_ms(std::uint64_t ms, std::uint32_t sr) {
    return (std::uint64_t)std::llround((double)ms / 1000.0 * (double)sr);
}

// Config::from_args (audio_matcher.rs:38-52) + the rounding of :99-100, :228
// --best N: the N best hits of one main file (am_match_best: no chunks, no prominence threshold; min_distance from
// --distance as the reference computes it; scale LIB), sorted by start
inline std::vector<am_peak> best_hits(const Arguments& a, const am_needle* h, const std::vector<float>& samples, std::uint32_t sr) {
    am_best_params bp{};
    bp.k = *a.best;
    bp.min_distance = (a.distance_msec() / 1000) * (std::uint64_t)sr;
    bp.min_prominence = 0.0f;
    bp.scale = AM_SCALE_LIB;
    std::vector<am_peak> out((size_t)bp.k);
    size_t n = 0;
    if (am_match_best(h, samples.data(), samples.size(), AM_FMT_F32_MONO, &bp, out.data(), &n) != AM_OK)
        throw std::runtime_error(std::string("am_match_best: ") + am_last_error_string());
    out.resize(n);
    std::stable_sort(out.begin(), out.end(), [](const am_peak& x, const am_peak& y) { return x.start < y.start; });
    return out;
}

// --score-trace: the records of one main file against one snippet (am_match_trace over the samples that were matched;
// scale LIB, BIN rounded to samples of the file's rate), *bin = the scores per record
inline std::vector<am_trace_bin> trace_of(const Arguments& a, const am_needle* h, const std::vector<float>& samples, std::uint32_t sr,
                                          std::uint64_t* bin) {
    am_trace_params tp{};
    tp.bin = std::max<std::uint64_t>(1, round_samples_ms(a.trace_bin_ms, sr));
    tp.scale = AM_SCALE_LIB;
    *bin = tp.bin;
    size_t s = 0, nb = 0, n = 0;
    if (am_needle_len(h, &s) != AM_OK || am_trace_len(samples.size() >= s ? samples.size() - s + 1 : 0, tp.bin, &nb) != AM_OK)
        throw std::runtime_error(std::string("--score-trace: ") + am_last_error_string());
    std::vector<am_trace_bin> out(nb);
    if (am_match_trace(h, samples.data(), samples.size(), AM_FMT_F32_MONO, &tp, out.data(), out.size(), &n) != AM_OK)
        throw std::runtime_error(std::string("am_match_trace: ") + am_last_error_string());
    out.resize(std::min(n, out.size()));
    return out;
}

// ... as the text of its CSV file: values with %.9g, so that an f32 reads back to its bits; a bin without a score shows nan
inline std::string trace_csv(const std::vector<am_trace_bin>& bins, std::uint64_t bin, std::uint32_t sr) {
    std::string s = "start_s,max,max_at_s,min,min_at_s,mean,rms,count\n";
    char buf[256];
    for (std::size_t b = 0; b < bins.size(); ++b) {
        const am_trace_bin& r = bins[b];
        const double t0 = (double)(b * bin), nan = std::nan(""), c = (double)r.count;
        std::snprintf(buf, sizeof buf, "%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%u\n", t0 / sr, r.count ? (double)r.max : nan,
                      r.count ? (t0 + r.argmax) / sr : nan, r.count ? (double)r.min : nan, r.count ? (t0 + r.argmin) / sr : nan,
                      r.count ? r.sum / c : nan, r.count ? std::sqrt(r.sumsq / c) : nan, r.count);
        s += buf;
    }
    return s;
}

// ... and its line under the offset lines (am_trace_summary)
inline std::string trace_line(const std::vector<am_trace_bin>& bins, std::uint64_t bin, std::uint32_t sr) {
    am_trace_stats st{};
    if (am_trace_summary(bins.data(), bins.size(), bin, &st) != AM_OK)
        throw std::runtime_error(std::string("am_trace_summary: ") + am_last_error_string());
    const std::uint64_t ms = st.count ? (std::uint64_t)((double)st.argmax * 1000.0 / (double)sr) : 0;
    char buf[256];
    std::snprintf(buf, sizeof buf, "Trace: max %.9g at %02" PRIu64 ":%02" PRIu64 ":%02" PRIu64 ".%03" PRIu64 ", bin maxima median %.9g mad %.9g, peak z %.9g",
                  st.max, ms / 3600000, (ms / 60000) % 60, (ms / 1000) % 60, ms % 1000, st.median_max, st.mad_max, st.peak_z);
    return buf;
}

inline am_match_params make_params(const Arguments& a, std::uint32_t sr, double snippet_duration_s) {
    am_match_params p{};
    p.sr = sr;
    p.chunk = round_samples_ms(a.chunk_size_ms(), sr);
    p.overlap = (std::uint64_t)std::llround(snippet_duration_s * (double)sr);
    p.min_prominence = a.prominence / 100.0f;
    p.min_distance = (a.distance_msec() / 1000) * (std::uint64_t)sr;     // distance.as_secs() as usize * sr
    p.overshadow_distance_s = (double)a.distance_msec() / 1000.0;
    p.scale = AM_SCALE_LIB;                                              // matcher/mod.rs:85 passes true
    return p;
}

}  // namespace amhost
