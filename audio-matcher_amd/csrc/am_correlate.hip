// am_correlate.hip -- the overlap-save pass over one haystack: which path it takes (pass_plan: plan geometry, fused scan,
// the odd last block, what a batch must size), the passes themselves (run_correlation), the peak pick's launches and merge.
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
    return sizeof(unsigned long long) * (size_t)nblocks * ballot_layout(pl.logN1, pl.logN2).words;
}
size_t sparse_bytes(long long nblocks, const PlanDev& pl) {
    return sparse_word_bytes(nblocks, pl) + sizeof(float) * (size_t)nblocks * ballot_layout(pl.logN1, pl.logN2).tiles;
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
static void needle_segments(am_needle* h) {
    if (!h->segments.empty()) return;
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
}

bool plan_fuses_scan(const PlanDev& pl, const Geometry& g) { return plan_has_scan(pl) && (g.hop % kTile) == 0; }

int pass_plan(am_needle* h, const Opts& o, long long out_count, bool allow_tail, PassPlan* pp) {
    Ctx* c = h->ctx;
    *pp = PassPlan{};
    int rc;
    if (needle_is_segmented(h, o)) {
        // one pass per needle segment, K3 adding up the partial sums: plain scores, no summary, no flags, no tail
        pp->kind = PassKind::Partitioned;
        needle_segments(h);
        Opts os = o;
        os.half = 0;   // (the accumulating K3 exists for the f32 work matrix)
        pp->parts.resize(h->segments.size());
        for (size_t i = 0; i < pp->parts.size(); ++i) {
            if ((rc = pass_plan(h->segments[i], os, out_count, false, &pp->parts[i]))) return rc;
            pp->need.work = std::max(pp->need.work, pp->parts[i].need.work);
        }
        return AM_OK;
    }
    if (h->n <= (size_t)kDirectMaxNeedle && o.log_n == 0) return AM_OK;   // tiny needle: direct summation, no blocks, no scratch
    pp->kind = PassKind::Transform;
    Geometry& g = pp->g;
    if ((rc = plan_geometry(h->n, out_count, o, &g))) return rc;
    if ((rc = get_plan(c, g.logN, &pp->pl))) return rc;
    if ((rc = needle_k2_spectrum(h, o, pp->pl, &pp->hc, &pp->hs))) return rc;
    pp->fused = plan_fuses_scan(pp->pl->dev, g);
    // the tail runs on a stream of its own beside the main pass (or, in a batch, is committed in front of the pick)
    if (allow_tail && pp->fused && c->stream_tail && c->ev_fork && c->ev_join && tail_plan(h->n, out_count, o, g, &pp->tail)) {
        if ((rc = get_plan(c, pp->tail.g.logN, &pp->tail_pl))) return rc;
        if ((rc = needle_k2_spectrum(h, o, pp->tail_pl, &pp->tail_hc, &pp->tail_hs))) return rc;
        pp->need.work_tail = (size_t)pp->tail.g.N * sizeof(float2);
    }
    pp->nblocks = pp->tail.on ? g.nblocks - 1 : g.nblocks;
    pp->npairs = pp->tail.on ? g.npairs - 1 : g.npairs;
    pp->main_count = pp->tail.on ? pp->tail.T : out_count;
    pp->ppg = std::min(std::max<long long>(1, o.pairs_per_group), pp->npairs);
    pp->need.work = (size_t)pp->ppg * (size_t)g.N * sizeof(float2);
    pp->need.npairs = g.npairs;
    if (pp->fused) {
        pp->need.stats32 = (size_t)((out_count + 31) / 32) * sizeof(float2);
        pp->need.side = sparse_bytes(g.nblocks, pp->pl->dev);
    }
    return AM_OK;
}

// The scores [tail.T, out_count) of a haystack on the smaller plan (TailPlan), queued on the context's tail stream:
// one block pair through K1 / K2 / K3 with every run written and the level-0 summary at its place in the main
// pass's stats32; then the last block of the MAIN layout is marked "every run written, threshold -inf".
static int run_tail_block(Ctx* c, const PassPlan& pp, const void* d_src, long long src_len,
                          float* d_dst, long long out_count, float factor, const ScanCfg& main_scan, int src_kind) {
    hipStream_t st = c->stream_tail;
    const TailPlan& tail = pp.tail;
    const PlanDev& pl = pp.tail_pl->dev;
    const HalfScale& hs = pp.tail_hs;
    int rc;
    if ((rc = c->work_tail.ensure(pp.need.work_tail))) return rc;
    Job job = tail_job(tail, d_src, src_len, out_count, src_kind);
    job.dst = d_dst + tail.T;
    ScanCfg scan{};
    scan.stats32 = main_scan.stats32 ? main_scan.stats32 + tail.T / 32 : nullptr;
    scan.margin = -1.0f; scan.hist_min = FLT_MAX;
    // (profiled as "other": the three classes' figures stay those of the main pass's launches)
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k1(st, job, 1, (float2*)c->work_tail.p, pl, hs.level)); }
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k2(st, 1, (float2*)c->work_tail.p, pp.tail_hc, pl, nullptr, hs.level, hs.hscale, hs.pre, true)); }
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_k3(st, job, 1, (const float2*)c->work_tail.p, pl, hs.k3(factor), scan, hs.level, false)); }
    if (main_scan.stats32 && main_scan.margin >= 0.0f && main_scan.wbits && main_scan.tile_theta) {
        const BallotLayout bl = ballot_layout(pp.pl->dev.logN1, pp.pl->dev.logN2);
        const size_t blk = (size_t)(pp.g.nblocks - 1);
        AM_HIP(hipMemsetAsync(main_scan.wbits + blk * bl.words, 0xFF, bl.words * sizeof(unsigned long long), st));
        AM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(main_scan.tile_theta + blk * bl.tiles), (int)0xFF7FFFFFu, bl.tiles, st));   // -FLT_MAX
    }
    return AM_OK;
}

static int run_correlation_one(am_needle* h, const PassPlan& pp, const void* d_src, long long src_len, long long lead,
                               float* d_dst, long long out_count, float factor,
                               const ScanRequest* scan_req, ScanResult* res, int src_kind, bool accumulate);

// The overlap-save engine for any needle length: one pass, or one pass per needle segment with the
// source shifted by the segment's offset and K3 adding up the partial sums (plain scores, every one
// written; the peak pick summarises them with tile_stats instead of the fused scan).
int run_correlation(am_needle* h, const Opts& o, const void* d_src, long long src_len, long long lead,
                           float* d_dst, long long out_count, float factor,
                           const ScanRequest* scan_req, ScanResult* res, int src_kind, const PassPlan* plan) {
    int rc;
    PassPlan own;
    if (!plan) {
        if ((rc = pass_plan(h, o, out_count, scan_req && !scan_req->no_scan && lead == 0, &own))) return rc;
        plan = &own;
    }
    if (res) { res->fused = false; res->redo_ok = false; res->sparse = plain_scores(); }
    if (plan->kind != PassKind::Partitioned) return run_correlation_one(h, *plan, d_src, src_len, lead, d_dst, out_count, factor, scan_req, res, src_kind, false);
    if (scan_req && scan_req->skip_launch) return fail(AM_ERR_INVALID_ARG, "internal: streaming ingest does not run early pairs for partitioned needles");
    for (size_t i = 0; i < plan->parts.size(); ++i) {
        // every pass writes (i = 0) or adds (i > 0) plain scores; a pass still honours the restriction to the
        // blocks of one chunk, and the first one may not touch the score buffer before the pick that last
        // read it is done
        ScanRequest plain{};
        if (scan_req) {
            plain.margin = -1.0f; plain.range_a = scan_req->range_a; plain.range_b = scan_req->range_b;
            plain.before_k3 = i == 0 ? scan_req->before_k3 : nullptr;
            plain.no_scan = true;
        }
        if ((rc = run_correlation_one(h->segments[i], plan->parts[i], d_src, src_len, lead - h->seg_off[i], d_dst, out_count, factor,
                                      scan_req ? &plain : nullptr, nullptr, src_kind, i > 0)))
            return rc;
    }
    return AM_OK;
}

static int run_correlation_one(am_needle* h, const PassPlan& pp, const void* d_src, long long src_len, long long lead,
                               float* d_dst, long long out_count, float factor,
                               const ScanRequest* scan_req, ScanResult* res, int src_kind, bool accumulate) {
    Ctx* c = h->ctx;
    Job job{};
    job.src = d_src; job.src_len = src_len; job.lead = lead; job.src_kind = src_kind;
    job.dst = d_dst; job.out_count = out_count;
    if (pp.kind == PassKind::Direct) {   // every score written, no fused scan
        ProfScope ps(c, KN_OTHER);
        AM_HIP(launch_direct(c->stream, job, h->d_needle, (int)h->n, factor));
        return AM_OK;
    }
    int rc;
    const PlanDev& pl = pp.pl->dev;
    const HalfScale& hs = pp.hs;
    const TailPlan& tail = pp.tail;
    const long long N = pp.g.N, hop = pp.g.hop, npairs = pp.npairs, ppg = pp.ppg;
    const ScanBuffers out = (scan_req && scan_req->out.work) ? scan_req->out : scan_buffers(c->side[0]);
    DevBuf& wk = *out.work;
    if ((rc = wk.ensure((size_t)ppg * (size_t)N * sizeof(float2)))) return rc;
    ScanCfg scan{};
    bool fused = false;
    if (scan_req && !scan_req->no_scan) {
        if (res) res->sparse = SparseScores{nullptr, nullptr, nullptr, (int)hop, pl.logN2, pl.logN1, 1.0 / (double)hop};
        if (pp.fused) {
            const long long side_blocks = std::max(pp.g.nblocks, scan_req->side_nblocks);
            if ((rc = out.stats32->ensure((size_t)((out_count + 31) / 32) * sizeof(float2)))) return rc;
            if ((rc = out.wflags->ensure(sparse_bytes(side_blocks, pl)))) return rc;
            fill_scan_cfg(&scan, out.stats32->p, out.wflags->p, side_blocks, pl, scan_req->margin, scan_req->hist_min, scan_req->seg_c, scan_req->seg_d);
            fused = true;
            if (res) { res->fused = true; res->sparse = sparse_view(scan, hop, pl); }
        }
    }
    // half-precision storage of the work matrix: K2 normalises by the needle
    // energy (times a fixed gain) so that stored values sit mid-range in f16
    const float k3scale = hs.k3(factor);
    job.out_count = pp.main_count; job.hop = (int)hop; job.nblocks = (int)pp.nblocks;
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
        if ((rc = run_tail_block(c, pp, d_src, src_len, d_dst, out_count, factor, scan, src_kind))) return rc;
        AM_HIP(hipEventRecord(c->ev_join, c->stream_tail));
    }
    bool waited = false;
    for (long long first = pair_lo; first < pair_hi; first += ppg) {
        const int np = (int)std::min(ppg, pair_hi - first);
        job.first_pair = (int)first;
        { ProfScope ps(c, KN_K1); AM_HIP(launch_k1(c->stream, job, np, (float2*)wk.p, pl, hs.level)); }
        { ProfScope ps(c, KN_K2); AM_HIP(launch_k2(c->stream, np, (float2*)wk.p, pp.hc, pl, nullptr, hs.level, hs.hscale, hs.pre)); }
        if (!waited && scan_req && scan_req->before_k3) AM_HIP(hipStreamWaitEvent(c->stream, scan_req->before_k3, 0));
        waited = true;
        { ProfScope ps(c, KN_K3); AM_HIP(launch_k3(c->stream, job, np, (const float2*)wk.p, pl, k3scale, scan, hs.level, accumulate)); }
    }
    if (with_tail) AM_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (res && fused && !accumulate && pair_lo == 0 && pair_hi == npairs && npairs <= ppg) {
        // the whole haystack's inverse rows sit in one work matrix: K3 can run again over chosen pairs
        res->redo_ok = true;
        job.first_pair = 0;
        res->redo_job = job; res->redo_pl = pl; res->redo_scale = k3scale; res->redo_half = hs.level;
        res->redo_npairs = (int)npairs; res->redo_work = (const float2*)wk.p; res->redo_cfg = scan;
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

int wide_reserve(Ctx* c, size_t n) {
    int rc;
    if ((rc = c->wide_ctl.ensure(n * kWideCtlBytes))) return rc;
    if ((rc = c->wide_list.ensure(n * AM_MAX_PEAKS_PER_CHUNK * sizeof(am_peak)))) return rc;
    return c->wide_tiles.ensure(n * kWideTileList * sizeof(int));
}
WideState wide_carve(Ctx* c, size_t n) {
    WideState wide{};
    wide.best = static_cast<unsigned long long*>(c->wide_ctl.p);
    wide.state = reinterpret_cast<int*>(wide.best + n);
    wide.count = reinterpret_cast<unsigned*>(wide.state + n);
    wide.seg_min = reinterpret_cast<float*>(wide.state + 2 * n);
    wide.ntiles = wide.state + 3 * n;
    wide.tiles = static_cast<int*>(c->wide_tiles.p);
    wide.list = static_cast<am_peak*>(c->wide_list.p);
    wide.cap = AM_MAX_PEAKS_PER_CHUNK;
    return wide;
}

// Launches find_peaks (audio_matcher.rs:221-230) for `nsegs` segments of a
// resident score array; segment descriptors live at [seg_off, seg_off + nsegs) of the
// context's segment buffer, result headers at [hdr_off, hdr_off + nsegs).
int launch_pick(Ctx* c, ScoreSide& side, const float* d_scores, long long n_scores, int seg_off, int nsegs,
                       float min_prom, long long min_dist, int* bad, const ScanResult* res, int hdr_off,
                       const PeakArena& arena, const PeakPolicy& pol, hipStream_t st, bool only_failed) {
    if (!st) st = c->stream;
    const SparseScores sp = (res && res->fused) ? res->sparse : plain_scores();
    if (nsegs == 0 || n_scores <= 0) return AM_OK;
    int rc;
    const long long ntiles = (n_scores + kTile - 1) / kTile;
    if ((rc = side.stats.ensure((size_t)ntiles * sizeof(float2)))) return rc;
    if (!only_failed) {   // (a second pick after a device-side redo of K3 finds the summaries it left: the scores are the same)
        ProfScope ps(c, KN_STATS, st);
        if (sp.stats32) AM_HIP(launch_stats_reduce(st, sp.stats32, n_scores, (float2*)side.stats.p, bad));
        else AM_HIP(launch_tile_stats(st, d_scores, n_scores, (float2*)side.stats.p, bad));
    }
    if ((rc = wide_reserve(c, (size_t)nsegs))) return rc;
    {
        ProfScope ps(c, KN_PEAKS, st);
        AM_HIP(launch_peaks(st, d_scores, n_scores, (const float2*)side.stats.p,
                            (const Segment*)c->segs.p + seg_off, nsegs, min_prom, min_dist,
                            (am_peak*)side.peaks.p, (SegHeader*)c->hdr.p + hdr_off, sp, arena, wide_carve(c, (size_t)nsegs), only_failed, pol));
    }
    return AM_OK;
}

// A chunk whose pick reported more than AM_MAX_PEAKS_PER_CHUNK peaks passing the prominence filter
// (SegHeader::overflow & 1): find_peaks returns them all, so does this path.  The scores, their
// tile summary (set 0) and the resident chunk `seg_idx` are those of the pick that just failed.
// Count the qualifying peaks, build the list in global memory, sort and filter it on the device
// (am_peaks.hip, peaks_big_finish), fetch the survivors.  Synchronous; appends to `all`.
int pick_chunk_big(Ctx* c, const float* d_scores, long long n_scores, int seg_idx, const Segment& sg,
                          float min_prom, long long min_dist, const ScanResult* res, float seg_min,
                          std::vector<am_peak>& all, const PeakPolicy& pol) {
    const long long a = sg.a, b = std::min(sg.b, n_scores);
    if (b - a >= 0xFFFFFFFFll) return fail(AM_ERR_PEAK_OVERFLOW, "chunk of 2^32 scores or more with more than AM_MAX_PEAKS_PER_CHUNK peaks");
    const SparseScores sp = (res && res->fused) ? res->sparse : plain_scores();
    const DevBuf& stats = c->side[0].stats;
    int rc;
    if ((rc = c->wide_ctl.ensure(kWideCtlBytes))) return rc;
    struct Ctl { unsigned long long best; int state; unsigned count; float seg_min; int ntiles; } ctl{0ull, 7, 0u, seg_min, -1};   // (state: handed over, head and tail pieces to be scanned)
    static_assert(sizeof(Ctl) == kWideCtlBytes, "one chunk's control words, in wide_carve's order");
    WideState wide = wide_carve(c, 1);
    wide.tiles = nullptr;
    const Segment* d_seg = (const Segment*)c->segs.p + seg_idx;
    // pass 1: count
    wide.list = nullptr; wide.cap = 0;
    AM_HIP(hipMemcpyAsync(c->wide_ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    AM_HIP(launch_peaks_wide_one(c->stream, d_scores, n_scores, (const float2*)stats.p, d_seg, min_prom, min_dist, sp, wide, pol));
    unsigned n = 0;
    if ((rc = download(c, &n, wide.count, sizeof(unsigned)))) return rc;
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
    AM_HIP(hipMemcpyAsync(c->wide_ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    AM_HIP(launch_peaks_wide_one(c->stream, d_scores, n_scores, (const float2*)stats.p, d_seg, min_prom, min_dist, sp, wide, pol));
    AM_HIP(hipMemsetAsync(base + off_table, 0xFF, 8 * nb, c->stream));
    AM_HIP(launch_peaks_big_finish(c->stream, wide.list, n, a, min_dist, reinterpret_cast<unsigned long long*>(base + off_keys),
                                   reinterpret_cast<unsigned*>(base + off_idx), reinterpret_cast<long long*>(base + off_table),
                                   reinterpret_cast<am_peak*>(base + off_out), reinterpret_cast<unsigned*>(base + off_n), pol));
    unsigned kept = 0;
    if ((rc = download(c, &kept, base + off_n, sizeof(unsigned)))) return rc;
    if (kept > n) return fail(AM_ERR_PEAK_OVERFLOW, "peak filter failed");
    const size_t old = all.size();
    all.resize(old + kept);
    if (kept) {
        if ((rc = download(c, all.data() + old, base + off_out, sizeof(am_peak) * (size_t)kept))) return rc;
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
    return hand_back(kept, out, cap, n_out, "peak output buffer too small");
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
    if ((rc = download(c, flags, c->range_flags.p, sizeof(int) * n))) return rc;
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
