// am_correlate.hip -- the overlap-save pass over one haystack: plan geometry, the odd last block (TailPlan), the
// passes themselves (run_correlation), what a batch must size for them, and the peak pick's launches and merge.
// Host-side mirror of the reference's driver (paths relative to the reference):
//   calc_chunks            src/matcher/audio_matcher.rs:88-141
//   is_overshadowed        src/matcher/audio_matcher.rs:143-160
//   start_as_duration      src/matcher/mod.rs:127-129
//   Mode crop / centered   src/matcher/audio_matcher.rs:450-464
// All arithmetic on samples runs in the HIP kernels of am_fft.hip /
// am_peaks.hip; there is no CPU fallback.
#include "am_internal.h"

namespace am {

static int pick_log_n(size_t s, long long out_count, const Opts& o, int* logN_out) {
    // smallest transform that can hold the needle at all
    int min_log = kLogNMin;
    while (min_log <= kLogNMax && ((size_t)1 << min_log) < s + 1) ++min_log;
    if (min_log > kLogNMax) return fail(AM_ERR_INVALID_ARG, "needle too long for a forced transform size (2^23 at most; leave log_n at 0 for needle partitioning)");
    if (o.log_n > 0) {
        int l = (int)o.log_n;
        if (l < min_log) l = min_log;
        if (l > kLogNMax) l = kLogNMax;
        *logN_out = l;
        return AM_OK;
    }
    const long long span = out_count + (long long)s - 1;
    // The register-resident kernels exist for N = 2^21 and 2^22 only and are several times
    // faster per point than the generic ones, so every problem that is not small runs on
    // them; short needles simply get a longer hop.
    if (span > (1ll << 19)) {
        // measured crossover (tools/needle_sweep.py)
        if ((long long)s <= kWideFromSamples) { *logN_out = 21; return AM_OK; }
        if ((long long)s <= kWidestFromSamples) {
            // a short haystack (BASELINE configs[0]: one 60 s window) whose scores fit ONE pair of 2^21
            // blocks does not pay for a pair of 2^22 (half the points, same number of launches)
            long long hop21 = (1ll << 21) - (long long)s + 1;
            if (hop21 >= 8 * kTile) hop21 = (hop21 / kTile) * kTile;
            *logN_out = (hop21 > 0 && out_count <= 2 * hop21) ? 21 : 22;
            return AM_OK;
        }
        if ((long long)s <= kSegmentFrom) {
            // long needles: 2^23, unless the scores fit one pair of 2^22 blocks
            long long hop22 = (1ll << 22) - (long long)s + 1;
            if (hop22 >= 8 * kTile) hop22 = (hop22 / kTile) * kTile;
            *logN_out = (hop22 > 0 && out_count <= 2 * hop22) ? 22 : 23;
            return AM_OK;
        }
    }
    int pref = min_log;
    while (pref < kLogNMax) {
        const double n = (double)((size_t)1 << pref);
        if ((n - (double)s + 1.0) / n >= kMinEfficiency) break;
        ++pref;
    }
    // whole problem in one block if that is smaller
    int single = kLogNMin;
    while (single < kLogNMax && (long long)((size_t)1 << single) < span) ++single;
    *logN_out = std::min(pref, std::max(single, min_log));
    return AM_OK;
}

int plan_geometry(size_t s, long long out_count, const Opts& o, Geometry* g) {
    int rc = pick_log_n(s, out_count, o, &g->logN);
    if (rc) return rc;
    g->N = 1ll << g->logN;
    g->hop = g->N - (long long)s + 1;
    if (g->hop >= 8 * kTile) g->hop = (g->hop / kTile) * kTile;
    g->nblocks = (out_count + g->hop - 1) / g->hop;
    g->npairs = (g->nblocks + 1) / 2;
    return AM_OK;
}
bool tail_plan(size_t s, long long out_count, const Opts& o, const Geometry& g, TailPlan* t) {
    t->on = false;
    if (!o.tail_block || o.log_n != 0 || g.logN < 22 || !(g.nblocks & 1) || g.nblocks < 3 || (g.hop % kTile) != 0) return false;
    const long long T = (g.nblocks - 1) * g.hop, rest = out_count - T;
    for (int lt = 21; lt < g.logN; ++lt) {   // (2^21 is the smallest plan whose K3 carries the scan)
        const long long N = 1ll << lt;
        long long hop = N - (long long)s + 1;
        if (hop < 8 * kTile) continue;
        hop = (hop / kTile) * kTile;
        if (2 * hop < rest) continue;
        t->on = true; t->T = T;
        t->g.logN = lt; t->g.N = N; t->g.hop = hop; t->g.nblocks = (rest + hop - 1) / hop; t->g.npairs = 1;
        return true;
    }
    return false;
}

// Layout of a set's sparse-score side buffer: the ballots of K3's wavefronts (one 64-bit word per
// block, column tile and wavefront: which of the tile's runs were written), then the write
// thresholds K3 used, one float per (block, column tile).
static size_t sparse_word_bytes(long long nblocks, const PlanDev& pl) {
    return sizeof(unsigned long long) * (((size_t)nblocks << (pl.logN2 - kColsLog)) << (pl.logN1 - 6));
}
size_t sparse_bytes(long long nblocks, const PlanDev& pl) {
    return sparse_word_bytes(nblocks, pl) + sizeof(float) * ((size_t)nblocks << (pl.logN2 - kColsLog));
}
void fill_scan_cfg(ScanCfg* cfg, void* stats32, void* side, long long nblocks, const PlanDev& pl, float margin, float hist_min,
                          long long seg_c, long long seg_d) {
    cfg->stats32 = static_cast<float2*>(stats32);
    cfg->wbits = static_cast<unsigned long long*>(side);
    cfg->tile_theta = reinterpret_cast<float*>(static_cast<char*>(side) + sparse_word_bytes(nblocks, pl));
    cfg->margin = margin;
    cfg->hist_min = hist_min;
    cfg->seg_c = seg_c; cfg->seg_d = seg_d;
    cfg->inv_c = seg_c > 0 ? 1.0 / (double)seg_c : 0.0;
}
// what the peak pick sees of it: with every run written (margin < 0) it needs neither flags nor thresholds
SparseScores sparse_view(const ScanCfg& cfg, long long hop, const PlanDev& pl) {
    if (cfg.margin < 0.0f) return SparseScores{nullptr, cfg.stats32, nullptr, (int)hop, pl.logN2, pl.logN1, 1.0 / (double)hop};
    return SparseScores{cfg.wbits, cfg.stats32, cfg.tile_theta, (int)hop, pl.logN2, pl.logN1, 1.0 / (double)hop};
}

bool needle_is_segmented(const am_needle* h, const Opts& o) {
    return (long long)h->n > kSegmentFrom && o.log_n == 0;
}
static int needle_segments(am_needle* h) {
    if (!h->segments.empty()) return AM_OK;
    const long long n = (long long)h->n;
    const long long nseg = (n + kSegmentLen - 1) / kSegmentLen;
    for (long long i = 0; i < nseg; ++i) {
        const long long a = n * i / nseg, b = n * (i + 1) / nseg;
        am_needle* sub = new am_needle();
        sub->ctx = h->ctx; sub->d_needle = h->d_needle + a; sub->n = (size_t)(b - a);
        sub->inv_autocorr = h->inv_autocorr; sub->owns_data = false;
        h->segments.push_back(sub);
        h->seg_off.push_back(a);
    }
    return AM_OK;
}

static int run_correlation_one(am_needle* h, const Opts& o, const void* d_src, long long src_len, long long lead,
                               float* d_dst, long long out_count, float factor,
                               ScanRequest* scan_req, int src_kind, bool accumulate);

// The scores [tail.T, out_count) of a haystack on the smaller plan (TailPlan), queued on the context's tail stream:
// one block pair through K1 / K2 / K3 with every run written and the level-0 summary at its place in the main
// pass's stats32; then block `main_nblocks - 1` of the MAIN layout is marked "every run written, threshold -inf".
static int run_tail_block(am_needle* h, const Opts& o, const TailPlan& tail, const void* d_src, long long src_len,
                          float* d_dst, long long out_count, float factor, const ScanCfg& main_scan, const PlanDev& main_pl,
                          long long main_nblocks, int src_kind) {
    Ctx* c = h->ctx;
    hipStream_t st = c->stream_tail;
    int rc;
    const Plan* pl = nullptr;
    if ((rc = get_plan(c, tail.g.logN, &pl))) return rc;
    const float2* hc = nullptr;
    HalfScale hs;
    if ((rc = needle_k2_spectrum(h, o, pl, &hc, &hs))) return rc;
    if ((rc = c->work_tail.ensure((size_t)tail.g.N * sizeof(float2)))) return rc;
    Job job = tail_job(tail, d_src, src_len, out_count, src_kind);
    job.dst = d_dst + tail.T;
    ScanCfg scan{};
    scan.stats32 = main_scan.stats32 ? main_scan.stats32 + tail.T / 32 : nullptr;
    scan.margin = -1.0f; scan.hist_min = FLT_MAX;
    // (profiled as "other": the three classes' figures stay those of the main pass's launches)
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k1(st, job, 1, (float2*)c->work_tail.p, pl->dev, hs.level)); }
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k2(st, 1, (float2*)c->work_tail.p, hc, pl->dev, nullptr, hs.level, hs.hscale, hs.pre, true)); }
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k3(st, job, 1, (const float2*)c->work_tail.p, pl->dev, hs.k3(factor), scan, hs.level, false)); }
    if (main_scan.stats32 && main_scan.margin >= 0.0f && main_scan.wbits && main_scan.tile_theta) {
        const size_t tiles = (size_t)1 << (main_pl.logN2 - kColsLog), words = tiles << (main_pl.logN1 - 6);
        const size_t blk = (size_t)(main_nblocks - 1);
        AM_HIP(hipMemsetAsync(main_scan.wbits + blk * words, 0xFF, words * sizeof(unsigned long long), st));
        AM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(main_scan.tile_theta + blk * tiles), (int)0xFF7FFFFFu, tiles, st));   // -FLT_MAX
    }
    return AM_OK;
}

// The overlap-save engine for any needle length: one pass, or one pass per needle segment with the
// source shifted by the segment's offset and K3 adding up the partial sums (plain scores, every one
// written; the peak pick summarises them with tile_stats instead of the fused scan).
int run_correlation(am_needle* h, const Opts& o, const void* d_src, long long src_len, long long lead,
                           float* d_dst, long long out_count, float factor,
                           ScanRequest* scan_req, int src_kind) {
    if (!needle_is_segmented(h, o)) return run_correlation_one(h, o, d_src, src_len, lead, d_dst, out_count, factor, scan_req, src_kind, false);
    int rc = needle_segments(h);
    if (rc) return rc;
    if (scan_req && scan_req->skip_launch) return fail(AM_ERR_INVALID_ARG, "internal: streaming ingest does not run early pairs for partitioned needles");
    Opts os = o;
    os.half = 0;   // (the accumulating K3 exists for the f32 work matrix)
    const size_t nseg = h->segments.size();
    for (size_t i = 0; i < nseg; ++i) {
        // every pass writes (i = 0) or adds (i > 0) plain scores; a pass still honours the restriction to the
        // blocks of one chunk, and the first one may not touch the score buffer before the pick that last
        // read it is done
        ScanRequest plain{};
        ScanRequest* sr = nullptr;
        if (scan_req) {
            plain.margin = -1.0f; plain.range_a = scan_req->range_a; plain.range_b = scan_req->range_b;
            plain.before_k3 = i == 0 ? scan_req->before_k3 : nullptr;
            plain.no_scan = true;
            sr = &plain;
        }
        if ((rc = run_correlation_one(h->segments[i], os, d_src, src_len, lead - h->seg_off[i], d_dst, out_count, factor, sr, src_kind, i > 0)))
            return rc;
    }
    if (scan_req) {   // the sums are complete scores without a level-0 summary: the pick summarises them itself (tile_stats)
        scan_req->fused = false;
        scan_req->sparse = SparseScores{nullptr, nullptr, nullptr, 1, 5, 5, 1.0};
    }
    return AM_OK;
}

static int run_correlation_one(am_needle* h, const Opts& o, const void* d_src, long long src_len, long long lead,
                               float* d_dst, long long out_count, float factor,
                               ScanRequest* scan_req, int src_kind, bool accumulate) {
    Ctx* c = h->ctx;
    if (h->n <= (size_t)kDirectMaxNeedle && o.log_n == 0) {
        // tiny needle: direct summation, every score written, no fused scan
        if (scan_req) {
            scan_req->fused = false;
            scan_req->sparse = SparseScores{nullptr, nullptr, nullptr, 1, 5, 5, 1.0};
        }
        Job job{};
        job.src = d_src; job.src_len = src_len; job.lead = lead; job.src_kind = src_kind;
        job.dst = d_dst; job.out_count = out_count;
        ProfScope ps(c, KN_OTHER);
        AM_HIP(launch_direct(c->stream, job, h->d_needle, (int)h->n, factor));
        return AM_OK;
    }
    Geometry g{};
    int rc = plan_geometry(h->n, out_count, o, &g);
    if (rc) return rc;
    const Plan* pl = nullptr;
    if ((rc = get_plan(c, g.logN, &pl))) return rc;
    const float2* hc = nullptr;
    HalfScale hs;
    if ((rc = needle_k2_spectrum(h, o, pl, &hc, &hs))) return rc;
    const long long N = g.N, hop = g.hop, nblocks = g.nblocks;
    // (streaming ingest launches its pairs itself, under the layout of the announced length: no tail there)
    TailPlan tail{};
    if (scan_req && !scan_req->no_scan && !accumulate && lead == 0 && !scan_req->ext_stats32 && !scan_req->ext_side &&
        !scan_req->skip_launch && scan_req->side_nblocks == 0 && plan_has_scan(pl->dev) && c->stream_tail && c->ev_fork && c->ev_join)
        tail_plan(h->n, out_count, o, g, &tail);
    const long long npairs = tail.on ? g.npairs - 1 : g.npairs;   // block pairs of the main pass
    long long ppg = std::max<long long>(1, o.pairs_per_group);
    if (ppg > npairs) ppg = npairs;
    DevBuf& wk = (scan_req && scan_req->work_by_set && scan_req->set) ? c->work_b : c->work;
    if ((rc = wk.ensure((size_t)ppg * (size_t)N * sizeof(float2)))) return rc;
    if (scan_req) scan_req->redo_ok = false;
    ScanCfg scan{};
    if (scan_req && !scan_req->no_scan) {
        scan_req->fused = false;
        scan_req->sparse = SparseScores{nullptr, nullptr, nullptr, (int)hop, pl->dev.logN2, pl->dev.logN1, 1.0 / (double)hop};
        if (plan_has_scan(pl->dev) && (hop % kTile) == 0) {
            DevBuf& b32 = scan_req->ext_stats32 ? *scan_req->ext_stats32 : (scan_req->set ? c->stats32_b : c->stats32);
            DevBuf& bwf = scan_req->ext_side ? *scan_req->ext_side : (scan_req->set ? c->wflags_b : c->wflags);
            const long long side_blocks = std::max(nblocks, scan_req->side_nblocks);
            if ((rc = b32.ensure((size_t)((out_count + 31) / 32) * sizeof(float2)))) return rc;
            if ((rc = bwf.ensure(sparse_bytes(side_blocks, pl->dev)))) return rc;
            fill_scan_cfg(&scan, b32.p, bwf.p, side_blocks, pl->dev, scan_req->margin, scan_req->hist_min, scan_req->seg_c, scan_req->seg_d);
            scan_req->fused = true;
            scan_req->sparse = sparse_view(scan, hop, pl->dev);
        }
    }
    // half-precision storage of the work matrix: K2 normalises by the needle
    // energy (times a fixed gain) so that stored values sit mid-range in f16
    const float k3scale = hs.k3(factor);
    Job job{};
    job.src = d_src; job.src_len = src_len; job.lead = lead; job.src_kind = src_kind;
    job.dst = d_dst; job.out_count = tail.on ? tail.T : out_count; job.hop = (int)hop; job.nblocks = (int)(tail.on ? nblocks - 1 : nblocks);
    if (scan_req && scan_req->skip_launch) return AM_OK;
    long long pair_lo = 0, pair_hi = npairs;
    bool with_tail = tail.on;
    if (scan_req && scan_req->range_b > scan_req->range_a) {
        pair_lo = (scan_req->range_a / hop) / 2;
        pair_hi = std::min(npairs, ((scan_req->range_b - 1) / hop) / 2 + 1);
        with_tail = tail.on && scan_req->range_b > tail.T;
    }
    if (scan_req && scan_req->tail_by_caller) with_tail = false;
    if (with_tail) {
        // beside the main pass: everything this stream has been told to wait for (the pick that last read the set)
        // holds for the tail's stream too, and the main stream takes the tail back in before anything reads the scores
        AM_HIP(hipEventRecord(c->ev_fork, c->stream));
        AM_HIP(hipStreamWaitEvent(c->stream_tail, c->ev_fork, 0));
        if ((rc = run_tail_block(h, o, tail, d_src, src_len, d_dst, out_count, factor, scan, pl->dev, nblocks, src_kind))) return rc;
        AM_HIP(hipEventRecord(c->ev_join, c->stream_tail));
    }
    bool waited = false;
    for (long long first = pair_lo; first < pair_hi; first += ppg) {
        const int np = (int)std::min(ppg, pair_hi - first);
        job.first_pair = (int)first;
        { ProfScope ps(c, KN_K1); AM_HIP(launch_k1(c->stream, job, np, (float2*)wk.p, pl->dev, hs.level)); }
        { ProfScope ps(c, KN_K2); AM_HIP(launch_k2(c->stream, np, (float2*)wk.p, hc, pl->dev, nullptr, hs.level, hs.hscale, hs.pre)); }
        if (!waited && scan_req && scan_req->before_k3) AM_HIP(hipStreamWaitEvent(c->stream, scan_req->before_k3, 0));
        waited = true;
        { ProfScope ps(c, KN_K3); AM_HIP(launch_k3(c->stream, job, np, (const float2*)wk.p, pl->dev, k3scale, scan, hs.level, accumulate)); }
    }
    if (with_tail) AM_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (scan_req && scan_req->fused && !accumulate && pair_lo == 0 && pair_hi == npairs && npairs <= ppg) {
        // the whole haystack's inverse rows sit in one work matrix: K3 can run again over chosen pairs
        scan_req->redo_ok = true;
        job.first_pair = 0;
        scan_req->redo_job = job; scan_req->redo_pl = pl->dev; scan_req->redo_scale = k3scale; scan_req->redo_half = hs.level;
        scan_req->redo_npairs = (int)npairs; scan_req->redo_work = (const float2*)wk.p; scan_req->redo_cfg = scan;
    }
    return AM_OK;
}

int correlation_footprint(am_needle* h, const Opts& o, long long out_count, Footprint* f) {
    if (needle_is_segmented(h, o)) {
        int rc = needle_segments(h);
        if (rc) return rc;
        Opts os = o;
        os.half = 0;
        for (am_needle* sub : h->segments) {
            Footprint one;
            if ((rc = correlation_footprint(sub, os, out_count, &one))) return rc;
            f->work = std::max(f->work, one.work);   // (plain scores: no summary, no flags)
        }
        return AM_OK;
    }
    if (h->n <= (size_t)kDirectMaxNeedle && o.log_n == 0) return AM_OK;
    Geometry g{};
    int rc = plan_geometry(h->n, out_count, o, &g);
    if (rc) return rc;
    const Plan* pl = nullptr;
    if ((rc = get_plan(h->ctx, g.logN, &pl))) return rc;
    const float2* hc = nullptr;
    HalfScale hs;
    if ((rc = needle_k2_spectrum(h, o, pl, &hc, &hs))) return rc;
    const long long ppg = std::min(std::max<long long>(1, o.pairs_per_group), g.npairs);
    f->work = std::max(f->work, (size_t)ppg * (size_t)g.N * sizeof(float2));
    f->npairs = std::max(f->npairs, g.npairs);
    if (plan_has_scan(pl->dev) && (g.hop % kTile) == 0) {
        f->stats32 = std::max(f->stats32, (size_t)((out_count + 31) / 32) * sizeof(float2));
        f->side = std::max(f->side, sparse_bytes(g.nblocks, pl->dev));
        TailPlan tail{};
        if (tail_plan(h->n, out_count, o, g, &tail)) {   // (plan and spectrum of the odd last block's transform, see run_tail_block)
            const Plan* plt = nullptr;
            if ((rc = get_plan(h->ctx, tail.g.logN, &plt))) return rc;
            if ((rc = needle_k2_spectrum(h, o, plt, &hc, &hs))) return rc;
            f->work_tail = std::max(f->work_tail, (size_t)tail.g.N * sizeof(float2));
        }
    }
    return AM_OK;
}

float scale_factor(const am_needle* h, int scale, size_t w) {
    if (scale == AM_SCALE_LIB) return h->inv_autocorr;                 // audio_matcher.rs:306-308
    if (scale == AM_SCALE_MY) return h->inv_autocorr / (float)w;       // audio_matcher.rs:444-447
    return 1.0f;
}

// Duration::from_secs_f64(start as f64 / sr as f64) in whole nanoseconds
// (matcher/mod.rs:127-129); exact on the f64 bits, round-to-nearest-even.
static uint64_t start_nanos(uint64_t start, uint32_t sr) {
    const double t = (double)start / (double)sr;
    if (!(t > 0.0)) return 0;
    int e = 0;
    const double m = std::frexp(t, &e);
    const unsigned long long mant = (unsigned long long)std::ldexp(m, 53);
    const int sh = e - 53;
    unsigned __int128 v = (unsigned __int128)mant * 1000000000ull;
    if (sh >= 0) return (uint64_t)(v << sh);
    const int r = -sh;
    if (r >= 127) return 0;
    unsigned __int128 q = v >> r;
    const unsigned __int128 rem = v & (((unsigned __int128)1 << r) - 1);
    const unsigned __int128 half = (unsigned __int128)1 << (r - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return (uint64_t)q;
}

// audio_matcher.rs:143-160
static bool is_overshadowed(const am_peak& element, const am_peak* other, uint32_t sr, double max_distance_s) {
    if (!other) return false;
    uint64_t e = start_nanos(element.start, sr), b = start_nanos(other->start, sr);
    if (e < b) std::swap(e, b);
    const uint64_t maxd = (uint64_t)std::llround(max_distance_s * 1e9);
    return (e - b) < maxd && other->prominence > element.prominence;
}

// Makes `segs` the chunk list resident on the device.  Consecutive calls with
// the same geometry (the common case: many haystacks of one length) reuse it.
int upload_segments(Ctx* c, const std::vector<Segment>& segs) {
    const size_t bytes = sizeof(Segment) * segs.size();
    if (c->segs.p && segs.size() == c->segs_resident.size() &&
        memcmp(segs.data(), c->segs_resident.data(), bytes) == 0)
        return AM_OK;
    int rc;
    c->segs_resident.clear();
    if ((rc = c->segs.ensure(bytes))) return rc;
    if ((rc = c->pinned.ensure(bytes))) return rc;
    memcpy(c->pinned.p, segs.data(), bytes);
    AM_HIP(hipMemcpyAsync(c->segs.p, c->pinned.p, bytes, hipMemcpyHostToDevice, c->stream));
    // the staging buffer is reused by the next upload: finish this one first (rare path)
    AM_HIP(hipStreamSynchronize(c->stream));
    c->segs_resident = segs;
    return AM_OK;
}

// The result area of one call, in coherent pinned host memory that the peak kernel
// writes directly: `nhdr` per-chunk headers followed by a spill arena for the peak
// lists of chunks with more than kInlinePeaks peaks (a bump allocator in the
// kernel; its cursor lives in device memory and is zeroed per call).
int prepare_results(Ctx* c, size_t nhdr, size_t arena_entries, PeakArena* arena) {
    const size_t hdr_bytes = (sizeof(SegHeader) * nhdr + 63) / 64 * 64;
    int rc;
    if ((rc = c->hdr.ensure(hdr_bytes + sizeof(am_peak) * arena_entries))) return rc;
    if ((rc = c->arena_cur.ensure(sizeof(unsigned)))) return rc;
    AM_HIP(hipMemsetAsync(c->arena_cur.p, 0, sizeof(unsigned), c->stream));
    arena->base = reinterpret_cast<am_peak*>(static_cast<char*>(c->hdr.p) + hdr_bytes);
    arena->cursor = static_cast<unsigned*>(c->arena_cur.p);
    arena->cap = (unsigned)arena_entries;
    return AM_OK;
}

// Launches find_peaks (audio_matcher.rs:221-230) for `nsegs` segments of a
// resident score array; segment descriptors live at [seg_off, seg_off + nsegs) of the
// context's segment buffer, result headers at [hdr_off, hdr_off + nsegs).
int launch_pick(Ctx* c, const float* d_scores, long long n_scores, int seg_off, int nsegs,
                       float min_prom, long long min_dist, const ScanRequest* scan, int hdr_off,
                       const PeakArena& arena, const PeakPolicy& pol, hipStream_t st, bool only_failed) {
    if (!st) st = c->stream;
    const int set = scan ? scan->set : 0;
    DevBuf& bstats = set ? c->stats_b : c->stats;
    DevBuf& bpeaks = set ? c->peaks_b : c->peaks;
    const float2* d_stats32 = (scan && scan->fused) ? scan->sparse.stats32 : nullptr;
    const SparseScores sp = (scan && scan->fused) ? scan->sparse : SparseScores{nullptr, nullptr, nullptr, 1, 5, 5, 1.0};
    if (nsegs == 0 || n_scores <= 0) return AM_OK;
    int rc;
    const long long ntiles = (n_scores + kTile - 1) / kTile;
    if ((rc = bstats.ensure((size_t)ntiles * sizeof(float2)))) return rc;
    if (!only_failed) {   // (a second pick after a device-side redo of K3 finds the summaries it left: the scores are the same)
        ProfScope ps(c, KN_STATS, st);
        int* bad = scan ? scan->bad : nullptr;
        if (d_stats32) AM_HIP(launch_stats_reduce(st, d_stats32, n_scores, (float2*)bstats.p, bad));
        else AM_HIP(launch_tile_stats(st, d_scores, n_scores, (float2*)bstats.p, bad));
    }
    // hand-over area for chunks with many candidate tiles (per chunk of this launch; the picks
    // of one call run in stream order, so one area serves them all)
    if ((rc = c->wide_ctl.ensure((size_t)nsegs * 24))) return rc;
    if ((rc = c->wide_list.ensure((size_t)nsegs * AM_MAX_PEAKS_PER_CHUNK * sizeof(am_peak)))) return rc;
    WideState wide{};
    wide.best = static_cast<unsigned long long*>(c->wide_ctl.p);
    wide.state = reinterpret_cast<int*>(wide.best + nsegs);
    wide.count = reinterpret_cast<unsigned*>(wide.state + nsegs);
    wide.seg_min = reinterpret_cast<float*>(wide.state + 2 * nsegs);
    wide.ntiles = wide.state + 3 * nsegs;
    if ((rc = c->wide_tiles.ensure((size_t)nsegs * kWideTileList * sizeof(int)))) return rc;
    wide.tiles = static_cast<int*>(c->wide_tiles.p);
    wide.list = static_cast<am_peak*>(c->wide_list.p);
    wide.cap = AM_MAX_PEAKS_PER_CHUNK;
    {
        ProfScope ps(c, KN_PEAKS, st);
        AM_HIP(launch_peaks(st, d_scores, n_scores, (const float2*)bstats.p,
                            (const Segment*)c->segs.p + seg_off, nsegs, min_prom, min_dist,
                            (am_peak*)bpeaks.p, (SegHeader*)c->hdr.p + hdr_off, sp, arena, wide, only_failed, pol));
    }
    return AM_OK;
}

// A chunk whose pick reported more than AM_MAX_PEAKS_PER_CHUNK peaks passing the prominence filter
// (SegHeader::overflow & 1): find_peaks returns them all, so does this path.  The scores, their
// tile summary (set 0) and the resident chunk `seg_idx` are those of the pick that just failed.
// Count the qualifying peaks, build the list in global memory, sort and filter it on the device
// (am_peaks.hip, peaks_big_finish), fetch the survivors.  Synchronous; appends to `all`.
int pick_chunk_big(Ctx* c, const float* d_scores, long long n_scores, int seg_idx, const Segment& sg,
                          float min_prom, long long min_dist, const ScanRequest* scan, float seg_min,
                          std::vector<am_peak>& all, const PeakPolicy& pol) {
    const long long a = sg.a, b = std::min(sg.b, n_scores);
    if (b - a >= 0xFFFFFFFFll) return fail(AM_ERR_PEAK_OVERFLOW, "chunk of 2^32 scores or more with more than AM_MAX_PEAKS_PER_CHUNK peaks");
    const SparseScores sp = (scan && scan->fused) ? scan->sparse : SparseScores{nullptr, nullptr, nullptr, 1, 5, 5, 1.0};
    int rc;
    if ((rc = c->wide_ctl.ensure(24))) return rc;
    struct Ctl { unsigned long long best; int state; unsigned count; float seg_min; int ntiles; } ctl{0ull, 7, 0u, seg_min, -1};   // (state: handed over, head and tail pieces to be scanned)
    WideState wide{};
    wide.best = static_cast<unsigned long long*>(c->wide_ctl.p);
    wide.state = reinterpret_cast<int*>(wide.best + 1);
    wide.count = reinterpret_cast<unsigned*>(wide.state + 1);
    wide.seg_min = reinterpret_cast<float*>(wide.state + 2);
    wide.ntiles = wide.state + 3;
    wide.tiles = nullptr;
    const Segment* d_seg = (const Segment*)c->segs.p + seg_idx;
    // pass 1: count
    wide.list = nullptr; wide.cap = 0;
    AM_HIP(hipMemcpyAsync(c->wide_ctl.p, &ctl, 24, hipMemcpyHostToDevice, c->stream));
    AM_HIP(launch_peaks_wide_one(c->stream, d_scores, n_scores, (const float2*)c->stats.p, d_seg, min_prom, min_dist, sp, wide, pol));
    unsigned n = 0;
    AM_HIP(hipMemcpyAsync(&n, wide.count, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    AM_HIP(hipStreamSynchronize(c->stream));
    if (n == 0) return AM_OK;
    if (n >= 0x40000000u) return fail(AM_ERR_PEAK_OVERFLOW, "peak list build failed");
    // one allocation: list | out | keys (2n) | table | idx (2n) | out_n
    const size_t nb = min_dist > 0 ? (size_t)((b - a) / min_dist) + 3 : 1;
    const size_t off_out = sizeof(am_peak) * (size_t)n, off_keys = 2 * off_out, off_table = off_keys + 16 * (size_t)n,
                 off_idx = off_table + 8 * nb, off_n = off_idx + 8 * (size_t)n;
    if ((rc = c->big.ensure(off_n + 16))) return rc;
    char* base = static_cast<char*>(c->big.p);
    // pass 2: fill the list (in any order)
    wide.list = reinterpret_cast<am_peak*>(base); wide.cap = n;
    AM_HIP(hipMemcpyAsync(c->wide_ctl.p, &ctl, 24, hipMemcpyHostToDevice, c->stream));
    AM_HIP(launch_peaks_wide_one(c->stream, d_scores, n_scores, (const float2*)c->stats.p, d_seg, min_prom, min_dist, sp, wide, pol));
    AM_HIP(hipMemsetAsync(base + off_table, 0xFF, 8 * nb, c->stream));
    AM_HIP(launch_peaks_big_finish(c->stream, wide.list, n, a, min_dist, reinterpret_cast<unsigned long long*>(base + off_keys),
                                   reinterpret_cast<unsigned*>(base + off_idx), reinterpret_cast<long long*>(base + off_table),
                                   reinterpret_cast<am_peak*>(base + off_out), reinterpret_cast<unsigned*>(base + off_n), pol));
    unsigned kept = 0;
    AM_HIP(hipMemcpyAsync(&kept, base + off_n, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    AM_HIP(hipStreamSynchronize(c->stream));
    if (kept > n) return fail(AM_ERR_PEAK_OVERFLOW, "peak filter failed");
    const size_t old = all.size();
    all.resize(old + kept);
    if (kept) {
        AM_HIP(hipMemcpyAsync(all.data() + old, base + off_out, sizeof(am_peak) * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        AM_HIP(hipStreamSynchronize(c->stream));
    }
    return AM_OK;
}

// windows of common::chunked(chunk + overlap, hop = chunk) (audio_matcher.rs:104)
// as slices of the global score array; a window shorter than the needle has
// no valid lag and is skipped.  `widths` (optional) receives within.len() of each window.
// `drop_tail` (option "tail_window" = 1): chunked() yields full-length windows only.
void make_segments(size_t len, size_t s, const am_match_params* p, bool drop_tail, std::vector<Segment>& segs,
                          std::vector<size_t>* widths, size_t max_windows) {
    const unsigned long long window = p->chunk + p->overlap;
    size_t i = 0;
    for (unsigned long long off = 0; off < len && i < max_windows; off += p->chunk, ++i) {
        const unsigned long long w = std::min<unsigned long long>(window, len - off);
        if (w < s || (drop_tail && w < window)) continue;
        Segment sg; sg.a = (long long)off; sg.b = (long long)(off + w - s + 1);
        segs.push_back(sg);
        if (widths) widths->push_back((size_t)w);
    }
}

// sort by start (audio_matcher.rs:135) + filter_surrounding (audio_matcher.rs:136-139)
// `from_filtered` (option "surrounding_from" = 1): the neighbour before an element is the last element that was KEPT (a
// sequential filter); default: both neighbours come from the sorted, unfiltered sequence.
int merge_peaks(std::vector<am_peak>& all, const am_match_params* p, bool from_filtered, am_peak* out, size_t cap, size_t* n_out) {
    std::stable_sort(all.begin(), all.end(), [](const am_peak& x, const am_peak& y) { return x.start < y.start; });
    MergeCursor cur;
    std::vector<am_peak> kept;
    merge_settle(p, from_filtered, cur, all.data(), all.size(), 0, true, &kept);
    const size_t n = kept.size();
    for (size_t i = 0; i < n && i < cap; ++i) out[i] = kept[i];
    *n_out = n;
    if (n > cap) return fail(AM_ERR_CAPACITY, "peak output buffer too small");
    return AM_OK;
}

// The filter of merge_peaks over a list that grows at its end (am_monitor).  An element's fate depends on its two
// neighbours only (audio_matcher.rs:143-160): every element but the last has its successor in the list; the last is
// settled when its predecessor overshadows it, or when no successor can -- one at `horizon` with +inf prominence is
// the strongest and nearest any later element can be, and is_overshadowed itself decides.  `ended`: nothing comes.
size_t merge_settle(const am_match_params* p, bool from_filtered, MergeCursor& cur, const am_peak* sorted, size_t n,
                    uint64_t horizon, bool ended, std::vector<am_peak>* kept_out) {
    am_peak strongest{};
    strongest.start = horizon;
    strongest.prominence = INFINITY;
    for (size_t i = 0; i < n; ++i) {
        const am_peak& x = sorted[i];
        const am_peak* before = from_filtered ? (cur.has_kept ? &cur.kept : nullptr) : (cur.has_prev ? &cur.prev : nullptr);
        const am_peak* after = i + 1 < n ? &sorted[i + 1] : nullptr;
        const bool shadowed_before = is_overshadowed(x, before, p->sr, p->overshadow_distance_s);
        if (!after && !ended && !shadowed_before && is_overshadowed(x, &strongest, p->sr, p->overshadow_distance_s)) return i;
        if (!shadowed_before && !is_overshadowed(x, after, p->sr, p->overshadow_distance_s)) {
            cur.kept = x; cur.has_kept = true;
            if (kept_out) kept_out->push_back(x);
        }
        cur.prev = x; cur.has_prev = true;
    }
    return n;
}

// Appends the peaks of header `hd` (inline, or spilled to the arena) to `all`.
void append_header_peaks(const SegHeader& hd, const PeakArena& arena, std::vector<am_peak>& all) {
    if (hd.n <= kInlinePeaks) {
        for (int j = 0; j < hd.n; ++j) all.push_back(hd.first[j]);
    } else {
        const am_peak* src = arena.base + hd.arena_off;
        all.insert(all.end(), src, src + hd.n);
    }
}

// The write-threshold margin of a call: a run's raw scores are written when its maximum reaches its K3 tile's minimum
// plus half a prominence; every run is written (-1) under MyConvolve scaling, with "dense_scores" or without a
// positive prominence bound.
float write_margin(const Opts& o, const am_match_params* p) {
    return (p->scale != AM_SCALE_MY && !o.dense && p->min_prominence > 0.f) ? 0.5f * p->min_prominence : -1.0f;
}

// The Job of a haystack's tail pair (TailPlan): scores [T, out_count) out of the samples from T on; no destination.
Job tail_job(const TailPlan& t, const void* d_src, long long src_len, long long out_count, int src_kind) {
    Job job{};
    job.src = advance_src(d_src, (size_t)t.T);
    job.src_len = src_len - t.T; job.lead = 0; job.src_kind = src_kind;
    job.out_count = out_count - t.T; job.hop = (int)t.g.hop; job.nblocks = (int)t.g.nblocks; job.first_pair = 0;
    return job;
}

// One search kernel over `n` sample ranges of d_src: flags[i] = range i holds a non-finite value.  Synchronous.
int nonfinite_flags(Ctx* c, const float* d_src, const Segment* ranges, int n, int* flags) {
    int rc;
    if ((rc = c->ranges.ensure(sizeof(Segment) * n))) return rc;
    if ((rc = c->range_flags.ensure(sizeof(int) * n))) return rc;
    AM_HIP(hipMemcpyAsync(c->ranges.p, ranges, sizeof(Segment) * n, hipMemcpyHostToDevice, c->stream));
    AM_HIP(hipMemsetAsync(c->range_flags.p, 0, sizeof(int) * n, c->stream));
    AM_HIP(launch_nonfinite_ranges(c->stream, d_src, (const Segment*)c->ranges.p, n, (int*)c->range_flags.p));
    AM_HIP(hipMemcpyAsync(flags, c->range_flags.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}
}  // namespace am

extern "C" int am_merge_ready(const am_match_params* p, const am_peak* sorted, size_t n, uint64_t horizon, int ended, size_t* n_ready) {
    using namespace am;
    if (!p || !n_ready || (!sorted && n)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (p->sr == 0) return fail(AM_ERR_INVALID_ARG, "p->sr must be > 0");
    *n_ready = 0;
    for (size_t i = 1; i < n; ++i)
        if (sorted[i].start < sorted[i - 1].start) return fail(AM_ERR_INVALID_ARG, "sorted: peaks not sorted by start");
    if (!ended && n && sorted[n - 1].start >= horizon) return fail(AM_ERR_INVALID_ARG, "sorted: a peak starts at or after horizon");
    MergeCursor cur;
    *n_ready = merge_settle(p, snapshot_opts(nullptr).surrounding_from != 0, cur, sorted, n, horizon, ended != 0, nullptr);
    return AM_OK;
}
