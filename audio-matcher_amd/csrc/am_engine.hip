// am_engine.hip -- the batch engines: match_many (one needle against a batch of haystacks) and match_multi_many
// (several needles, of one length or of any lengths), with what they share: the chunk plan, the two score sets, the tails of a batch.
// Host-side mirror of the reference's driver (paths relative to the reference):
//   calc_chunks            src/matcher/audio_matcher.rs:88-141
//   is_overshadowed        src/matcher/audio_matcher.rs:143-160
//   start_as_duration      src/matcher/mod.rs:127-129
//   Mode crop / centered   src/matcher/audio_matcher.rs:450-464
// All arithmetic on samples runs in the HIP kernels of am_fft.hip /
// am_peaks.hip; there is no CPU fallback.
#include "am_internal.h"

namespace am {

// The picks of a needle group (several needles against one haystack) as ONE set of launches: the level-1 summaries, the
// per-chunk pick and its two follow-up kernels each run once with the needle on a grid dimension, instead of four small
// launches per needle.  Every needle's result headers go to hdr_off[z] (absolute); scratch is laid out needle after needle.
static int launch_pick_group(Ctx* c, const K3Group& kg, long long n_scores, int seg_off, int nsegs, float min_prom, long long min_dist,
                             const SparseScores& sp_common, int* bad, const int* hdr_off, const PeakArena& arena, const PeakPolicy& pol,
                             hipStream_t st) {
    if (nsegs == 0 || n_scores <= 0 || kg.n <= 0) return AM_OK;
    int rc;
    const size_t nz = (size_t)kg.n, total = nz * (size_t)nsegs;
    const long long ntiles = (n_scores + kTile - 1) / kTile;
    PickGroup pg{};
    pg.n = kg.n;
    for (int z = 0; z < kg.n; ++z) {
        if ((rc = c->grp_stats[z].ensure((size_t)ntiles * sizeof(float2)))) return rc;
        pg.g[z] = kg.dst[z]; pg.stats[z] = static_cast<float2*>(c->grp_stats[z].p);
        pg.stats32[z] = kg.stats32[z]; pg.wbits[z] = kg.wbits[z]; pg.theta[z] = kg.tile_theta[z];
        pg.hdr_off[z] = hdr_off[z];
    }
    { ProfScope ps(c, KN_STATS, st);
      AM_HIP(launch_stats_reduce(st, pg.stats32[0], n_scores, pg.stats[0], bad, &pg)); }
    if ((rc = wide_reserve(c, total))) return rc;
    if ((rc = c->side[0].peaks.ensure(total * AM_MAX_PEAKS_PER_CHUNK * sizeof(am_peak)))) return rc;
    {
        ProfScope ps(c, KN_PEAKS, st);
        AM_HIP(launch_peaks(st, pg.g[0], n_scores, pg.stats[0], (const Segment*)c->segs.p + seg_off, nsegs, min_prom, min_dist,
                            (am_peak*)c->side[0].peaks.p, (SegHeader*)c->hdr.p, sp_common, arena, wide_carve(c, total), false, pol, &pg));
    }
    return AM_OK;
}

// ---- what both engines share --------------------------------------------------------------------------------------

// The chunks of a batch: every haystack's windows (make_segments) back to back, as slices of its score array.  With
// `split_short` (MyConvolve scaling) the shorter windows at the end of a haystack are kept apart: their factor depends
// on their length, so each is correlated on its own.
struct ChunkPlan {
    std::vector<Segment> segs, short_segs;   // main-pass chunks; the shorter windows
    std::vector<size_t> widths, short_w;     // within.len() of each
    std::vector<int> seg_off, short_off;     // haystack k: segs[seg_off[k] .. seg_off[k + 1]), the same for short_segs
    std::vector<int> n_chunks;               // windows of haystack k, of both kinds
    size_t max_scores = 0, max_segs = 1;     // the most scores and main-pass chunks of one haystack
    int ns(size_t k) const { return seg_off[k + 1] - seg_off[k]; }
    // more chunks than the pick's indices hold: per haystack, or over all result slots (nn needles per chunk)
    bool too_many(size_t nn) const { return max_segs > (size_t)1 << 18 || segs.size() * nn > (size_t)1 << 24; }
};
static void plan_chunks(size_t s, const void* const* d_hays, const size_t* lens, size_t n_hay, const am_match_params* p, const Opts& o,
                        bool split_short, size_t max_windows, ChunkPlan* cp) {
    const size_t window = (size_t)(p->chunk + p->overlap);
    cp->seg_off.assign(n_hay + 1, 0);
    cp->short_off.assign(n_hay + 1, 0);
    cp->n_chunks.assign(n_hay, 0);
    for (size_t k = 0; k < n_hay; ++k) {
        cp->seg_off[k] = (int)cp->segs.size();
        cp->short_off[k] = (int)cp->short_segs.size();
        if (!d_hays[k] || lens[k] < s) continue;
        std::vector<Segment> one;
        std::vector<size_t> w1;
        make_segments(lens[k], s, p, o.tail_window != 0, one, &w1, max_windows);
        cp->n_chunks[k] = (int)one.size();
        for (size_t i = 0; i < one.size(); ++i) {
            const bool shorter = split_short && w1[i] != window;
            (shorter ? cp->short_segs : cp->segs).push_back(one[i]);
            (shorter ? cp->short_w : cp->widths).push_back(w1[i]);
        }
        if (!one.empty()) cp->max_scores = std::max(cp->max_scores, lens[k] - s + 1);
        cp->max_segs = std::max(cp->max_segs, cp->segs.size() - (size_t)cp->seg_off[k]);
    }
    cp->seg_off[n_hay] = (int)cp->segs.size();
    cp->short_off[n_hay] = (int)cp->short_segs.size();
}

// The two alternating sets of score-side buffers of a batch.  The peak pick of one item (small, latency-bound
// kernels) runs on the second stream beside the transforms of the next item, which then need their own set; K3 waits
// for the pick that last read the set it is about to overwrite.  With one item, or option batch_overlap = 0,
// everything runs in set 0 on the main stream.
struct ScoreSets {
    Ctx* c;
    bool overlap;
    size_t seq = 0;   // items queued so far: item `seq` uses set seq & 1
    ScoreSets(Ctx* c_, const Opts& o, size_t n_items)
        : c(c_), overlap(o.batch_overlap && n_items > 1 && c_->stream2 && c_->ev_k3[0] && c_->ev_k3[1] && c_->ev_pick[0] && c_->ev_pick[1]) {}
    int count() const { return overlap ? 2 : 1; }
    int set() const { return overlap ? (int)(seq & 1) : 0; }
    ScoreSide& side() const { return c->side[set()]; }
    float* scores() const { return (float*)side().scores.p; }
    hipStream_t pick_stream() const { return overlap ? c->stream2 : c->stream; }
    // scores, tile summaries and peak lists of every set, and the pick's hand-over area, for the largest item: sized
    // before anything is queued, so that no pick has to grow them while the previous one still runs on the other stream
    int size(size_t max_scores, size_t max_segs) {
        int rc;
        for (int set = 0; set < count(); ++set) {
            ScoreSide& sd = c->side[set];
            if ((rc = sd.scores.ensure(max_scores * sizeof(float)))) return rc;
            if ((rc = sd.peaks.ensure(sizeof(am_peak) * max_segs * AM_MAX_PEAKS_PER_CHUNK))) return rc;
            if ((rc = sd.stats.ensure((max_scores + kTile - 1) / kTile * sizeof(float2)))) return rc;
        }
        return wide_reserve(c, max_segs);
    }
    // before K3 overwrites the current set: the pick that last read it is done (on_host: this thread waits for it,
    // otherwise the main stream does)
    int wait_pick(bool on_host) {
        if (!overlap || seq < 2) return AM_OK;
        if (on_host) AM_HIP(hipEventSynchronize(c->ev_pick[set()]));
        else AM_HIP(hipStreamWaitEvent(c->stream, c->ev_pick[set()], 0));
        return AM_OK;
    }
    // the item's K3 is queued: its pick (second stream) may start behind it
    int k3_done() {
        if (!overlap) return AM_OK;
        AM_HIP(hipEventRecord(c->ev_k3[set()], c->stream));
        AM_HIP(hipStreamWaitEvent(c->stream2, c->ev_k3[set()], 0));
        return AM_OK;
    }
    // the item's pick is queued: the next item takes the other set
    int pick_done() {
        if (overlap) AM_HIP(hipEventRecord(c->ev_pick[set()], c->stream2));
        ++seq;
        return AM_OK;
    }
    // everything queued has run: the result headers are in host memory
    int drain() {
        AM_HIP(hipStreamSynchronize(c->stream));
        if (overlap) AM_HIP(hipStreamSynchronize(c->stream2));
        return AM_OK;
    }
};

// One haystack through match_many on its own (no progress hooks), into result slot `slot`; AM_ERR_CAPACITY is noted
// in *worst, any other error returned.
static int match_alone(am_needle* h, const void* d_hay, size_t len, const am_match_params* p, am_peak* out, size_t cap, size_t slot,
                       size_t* n_out, int src_kind, const PartSpec* part, int* worst) {
    const int rc = match_many(h, &d_hay, &len, 1, p, out ? out + slot * cap : nullptr, cap, &n_out[slot], src_kind, 0, 1, false, nullptr, part);
    if (rc == AM_ERR_CAPACITY) *worst = rc;
    return rc == AM_ERR_CAPACITY ? AM_OK : rc;
}

// One window or chunk of match_many correlated and picked on its own, synchronously: `n_scores` scores of `src`
// into the context's set-0 score buffer, chunk `seg_idx` of the resident list (bounds `sg`) picked into the spare
// header with a spill arena of its own, its peaks appended to `all`, shifted by `shift` samples.
// With score_norm on (`nrm`), the chunk's scores are normalised before the pick, which then summarises them itself.
static int pick_alone(am_needle* h, const Opts& o, const am_match_params* p, const void* src, long long src_len, float factor,
                      const ScanRequest& req, long long n_scores, int seg_idx, const Segment& sg, int spare_hdr, uint64_t shift, int src_kind,
                      const NormSpec& nrm, std::vector<am_peak>& all) {
    Ctx* c = h->ctx;
    const PeakPolicy pol = o.peak_policy();
    int rc;
    PeakArena own{};
    if ((rc = c->spill.ensure(sizeof(am_peak) * AM_MAX_PEAKS_PER_CHUNK))) return rc;
    AM_HIP(hipMemsetAsync(c->arena_cur.p, 0, sizeof(unsigned), c->stream));
    own.base = static_cast<am_peak*>(c->spill.p); own.cursor = static_cast<unsigned*>(c->arena_cur.p);
    own.cap = AM_MAX_PEAKS_PER_CHUNK;
    ScoreSide& side = c->side[0];
    if ((rc = side.scores.ensure((size_t)n_scores * sizeof(float)))) return rc;
    float* d_scores = (float*)side.scores.p;
    ScanResult res{};
    if ((rc = run_correlation(h, o, src, src_len, 0, d_scores, n_scores, factor, &req, &res, src_kind))) return rc;
    if (nrm.on) {
        if ((rc = normalise_scores(c, c->stream, nrm, src, src_len, src_kind, 0, (long long)h->n, d_scores, sg.a, std::min(sg.b, n_scores))))
            return rc;
        res.fused = false;
    }
    if ((rc = launch_pick(c, side, d_scores, n_scores, seg_idx, 1, p->min_prominence, (long long)p->min_distance, nullptr, &res, spare_hdr, own, pol))) return rc;
    AM_HIP(hipStreamSynchronize(c->stream));
    const SegHeader& hd = static_cast<const SegHeader*>(c->hdr.p)[spare_hdr];
    const size_t old = all.size();
    if (hd.overflow & 1) {
        if ((rc = pick_chunk_big(c, d_scores, n_scores, seg_idx, sg, p->min_prominence, (long long)p->min_distance, &res, hd.seg_min, all, pol)))
            return rc;
    } else append_header_peaks(hd, own, all);
    for (size_t j = old; j < all.size(); ++j) { all[j].start += shift; all[j].end += shift; }
    return AM_OK;
}

// ---- the odd last blocks of a batch -------------------------------------------------------------------------------
// The tails of up to kMaxTailBatch haystacks of a batch (all on one smaller plan) as ONE launch each of K1 / K2 / K3 on
// the main stream: full grids instead of one under-filled launch triple per haystack beside the main pass (which costs
// about as much as the dropped pair saves, profiles/r04/tail_block_ab.txt).  The scores and their summary go to slots
// of the context's tail buffers; launch_tail_commit moves a haystack's slot into the score-side set its pick reads,
// once the pick that last read that set is done (on the pick's stream).  Same kernels' arithmetic as run_tail_block:
// a haystack's bits do not depend on whether it travels alone or in a batch.
struct TailSlots { size_t scores, stats; };   // elements per slot (floats, float2s)
// (the several-per-launch kernels exist for the 256-row plan, 2^21 points: the tail of a 2^23 main pass that needs the
// 2^22 plan is computed beside its main pass, like a single haystack's)
static bool tail_batchable(const TailPlan& t) { return t.on && t.g.logN == 21; }
static int launch_tail_batch(am_needle* h, const std::vector<PassPlan>& plans, const std::vector<size_t>& members, int half_idx,
                             const TailSlots& sl, const void* const* d_hays, const size_t* lens, float factor, int src_kind) {
    Ctx* c = h->ctx;
    const PassPlan& lead = plans[members[0]];   // (one plan, one spectrum: the members share the needle and the tail's transform size)
    const TailPlan& first = lead.tail;
    const Plan* pl = lead.tail_pl;
    const float2* hc = lead.tail_hc;
    const HalfScale& hs = lead.tail_hs;
    TailBatch tb{};
    tb.n = (int)members.size();
    for (int j = 0; j < tb.n; ++j) {
        const size_t k = members[j];
        const size_t slot = (size_t)half_idx * kMaxTailBatch + (size_t)j;
        const Job job = tail_job(plans[k].tail, d_hays[k], (long long)lens[k], (long long)(lens[k] - h->n + 1), src_kind);
        tb.src[j] = job.src;
        tb.src_len[j] = job.src_len;
        tb.out_count[j] = job.out_count;
        tb.dst[j] = static_cast<float*>(c->tail_scores.p) + slot * sl.scores;
        tb.stats32[j] = static_cast<float2*>(c->tail_stats.p) + slot * sl.stats;
    }
    float2* work = static_cast<float2*>(c->work_tail.p);
    { ProfScope ps(c, KN_OTHER); AM_HIP(launch_tail_batch_k1(c->stream, tb, (int)first.g.hop, src_kind, work, pl->dev, hs.level)); }
    { ProfScope ps(c, KN_OTHER); AM_HIP(launch_k2(c->stream, tb.n, work, hc, pl->dev, nullptr, hs.level, hs.hscale, hs.pre, true)); }
    { ProfScope ps(c, KN_OTHER); AM_HIP(launch_tail_batch_k3(c->stream, tb, (int)first.g.hop, work, pl->dev, hs.k3(factor), hs.level)); }
    return AM_OK;
}

// Which chunks of a haystack are touched by non-finite samples: drop[i] = the chunk's own window
// holds one (the reference's scores for it are NaN throughout: no peak); again[i] = its window is
// clean but some of its scores came from a block pair that holds one.  One search kernel over the
// sample ranges of all block pairs and all windows; rare path, synchronous.
static int classify_nonfinite(am_needle* h, const PassPlan& pp, const float* d_hay, size_t len,
                              const std::vector<Segment>& segs, int s0, int s1,
                              std::vector<char>* drop, std::vector<char>* again) {
    Ctx* c = h->ctx;
    const long long s = (long long)h->n;
    const int nch = s1 - s0;
    drop->assign(nch, 0); again->assign(nch, 0);
    std::vector<Segment> ranges;
    for (int i = s0; i < s1; ++i)       // the samples behind scores [a, b): a .. b + s - 2
        ranges.push_back(Segment{segs[i].a, std::min<long long>((long long)len, segs[i].b + s - 1)});
    // (direct summation spreads nothing; every segment pass of a partitioned needle has block pairs of its own: all clean windows again)
    const long long npairs = pp.kind == PassKind::Transform ? pp.npairs : 0;
    for (long long q = 0; q < npairs; ++q) ranges.push_back(pp.pair_reads(q, (long long)len));
    if (pp.tail.on) ranges.push_back(pp.tail_reads((long long)len));
    std::vector<int> flags(ranges.size(), 0);
    int rc = nonfinite_flags(c, d_hay, ranges.data(), (int)ranges.size(), flags.data());
    if (rc) return rc;
    for (int i = 0; i < nch; ++i) {
        if (flags[i]) { (*drop)[i] = 1; continue; }
        if (pp.kind == PassKind::Partitioned) { (*again)[i] = 1; continue; }
        const Segment sg = segs[s0 + i];
        for (long long q = 0; q < npairs && !(*again)[i]; ++q)
            if (flags[nch + q] && 2 * q * pp.g.hop < sg.b && (2 * q + 2) * pp.g.hop > sg.a) (*again)[i] = 1;
        if (pp.tail.on && flags[nch + npairs] && pp.tail.T < sg.b) (*again)[i] = 1;
    }
    return AM_OK;
}

// calc_chunks (audio_matcher.rs:88-141) over a batch of resident haystacks =
// the per-file loop of matcher::run (matcher/mod.rs:42-87).  Everything is
// queued on the context's stream without host synchronisation; the per-chunk
// result headers land in pinned host memory, so no copy ends the batch.
//
// scale == AM_SCALE_MY (MyConvolve's semantics, audio_matcher.rs:442-448): the factor
// 1 / (sum(needle^2) * within.len()) depends on the window, so the windows of full
// length share the main pass and every shorter window at the end of a haystack is
// correlated on its own with its own factor.
int match_many(am_needle* h, const void* const* d_hays, const size_t* lens, size_t n_hay,
               const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out, int src_kind,
               size_t index_base, size_t index_stride, bool fire_hooks, const StreamPre* pre, const PartSpec* part) {
    Ctx* c = h->ctx;
    const Opts o = snapshot_opts(h);
    const PeakPolicy pol = o.peak_policy();
    Hooks hooks = fire_hooks ? snapshot_hooks() : Hooks{};
    if (part) hooks.fn = nullptr;   // (the caller reports the whole haystack; the chunks report themselves, below)
    if (part && n_hay != 1) return fail(AM_ERR_INVALID_ARG, "internal: a part is one haystack");
    // local haystack k is item G(k) of the caller's batch: out, n_out and the progress
    // callbacks use that index (pool submit threads pass their shard: base + k * stride)
    auto G = [&](size_t k) { return index_base + k * index_stride; };
    const size_t s = h->n;
    if (p->chunk == 0) return fail(AM_ERR_INVALID_ARG, "chunk must be > 0");
    if (p->scale < AM_SCALE_NONE || p->scale > AM_SCALE_MY) return fail(AM_ERR_INVALID_ARG, "bad scale");
    // Option score_norm: K3 writes every raw score scaled by 1 / sqrt(needle energy), and each haystack's scores are
    // divided by their windows' energies on the pick's stream before its pick, which summarises them itself.  The
    // sparse-score certificate bounds raw scores only, and the needle's score history (hist_min) is neither read nor fed.
    const NormSpec nrm = norm_spec(h, o);
    if (nrm.on && (pre || part)) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    int rc = norm_check(nrm, p->scale);
    if (rc) return rc;
    const bool my = p->scale == AM_SCALE_MY;
    const float factor = nrm.on ? norm_factor(nrm) : scale_factor(h, p->scale, (size_t)(p->chunk + p->overlap));
    // Raw scores are written only for the 32-score runs whose maximum reaches their K3 tile's write
    // threshold: the tile's own minimum in the block plus half a prominence (am_fft.hip, k3_finish).
    // The peak kernel certifies per chunk that every threshold was low enough; a chunk that fails
    // (a dip deeper than half a prominence that most tiles' samples missed) is redone with every
    // run written.
    const int sm = p->scale == AM_SCALE_LIB ? 1 : 0;
    ScanRequest base{};   // what every pass of this call asks for; each pass adds its buffers and restrictions to a copy
    base.margin = nrm.on ? -1.0f : write_margin(o, p);
    const bool sparse_ok = base.margin >= 0.0f;
    base.hist_min = nrm.on ? FLT_MAX : h->hist_min(sm);   // (of the haystacks before this call: the whole batch is queued before any result is back)
    base.seg_c = (long long)p->chunk;
    base.seg_d = (long long)(p->chunk + p->overlap) - (long long)s;
    for (size_t k = 0; k < n_hay; ++k) n_out[G(k)] = 0;
    ChunkPlan cp;
    plan_chunks(s, d_hays, lens, n_hay, p, o, my, part ? part->max_windows : (size_t)-1, &cp);
    const std::vector<Segment>& segs = cp.segs;
    const std::vector<int>& seg_off = cp.seg_off;
    const size_t nsegs = segs.size();
    if (nsegs == 0 && cp.short_segs.empty()) return AM_OK;
    if (cp.too_many(1)) return fail(AM_ERR_INVALID_ARG, "chunk size too small for this haystack (more than 2^18 chunks)");
    size_t n_active = 0;
    for (size_t k = 0; k < n_hay; ++k) n_active += cp.ns(k) > 0;
    ScoreSets sets(c, o, n_active);
    if ((rc = sets.size(cp.max_scores, cp.max_segs))) return rc;
    // ... and the transforms' own buffers -- work matrix, level-0 summary, ballots and thresholds -- for the
    // haystack that needs the most of each: a ragged batch whose later haystacks are longer must not free
    // and re-allocate them under the kernels of the earlier ones (plans and needle spectra are built here too)
    // (streaming ingest launched its early pairs under the layout of the announced length: no tail there)
    std::vector<PassPlan> plans(n_hay);
    Footprint need;
    for (size_t k = 0; k < n_hay; ++k) {
        if (cp.n_chunks[k] == 0 || cp.ns(k) == 0) continue;
        if ((rc = pass_plan(h, o, (long long)(lens[k] - s + 1), pre == nullptr, &plans[k]))) return rc;
        need.take(plans[k].need);
    }
    // The odd last blocks (TailPlan).  A single haystack computes its tail beside its main pass (run_tail_block); a
    // batch that overlaps picks and transforms computes the tails of up to kMaxTailBatch haystacks per launch, into
    // slots of two alternating halves (a half is written again two batches later: every commit out of it is long done,
    // the main stream has waited for the pick of the haystack before the previous one by then).
    std::vector<int> tail_slot(n_hay, -1);
    TailSlots tslots{0, 0};
    bool batch_tails = false;
    if (need.work_tail) {
        size_t n_tails = 0;
        for (size_t k = 0; k < n_hay; ++k)
            if (tail_batchable(plans[k].tail)) {
                ++n_tails;
                tslots.scores = std::max(tslots.scores, (size_t)(2 * plans[k].tail.g.hop));
            }
        tslots.stats = tslots.scores / 32;
        batch_tails = sets.overlap && n_tails > 1;
        const size_t nslot = batch_tails ? kMaxTailBatch : 1;
        if ((rc = c->work_tail.ensure(need.work_tail * nslot))) return rc;
        if (batch_tails) {
            if ((rc = c->tail_scores.ensure(2 * kMaxTailBatch * tslots.scores * sizeof(float)))) return rc;
            if ((rc = c->tail_stats.ensure(2 * kMaxTailBatch * tslots.stats * sizeof(float2)))) return rc;
        }
    }
    int tail_batches = 0;
    for (int set = 0; set < sets.count(); ++set) {
        if (need.work && (rc = c->side[set].work.ensure(need.work))) return rc;
        if (pre) continue;   // (streaming ingest brings its own summary and flag buffers)
        if (need.stats32 && (rc = c->side[set].stats32.ensure(need.stats32))) return rc;
        if (need.side && (rc = c->side[set].wflags.ensure(need.side))) return rc;
    }
    // one spare header behind the main ones serves the single-chunk passes below; the arena
    // holds every list of one haystack in the worst case plus a few entries per chunk
    // (bounded: a chunk whose list finds no room is picked again on its own below)
    PeakArena arena{};
    if ((rc = prepare_results(c, nsegs + 1, std::min<size_t>(cp.max_segs * AM_MAX_PEAKS_PER_CHUNK, (size_t)1 << 20) + nsegs * 8, &arena))) return rc;
    // the resident chunk list: the main-pass chunks, then one local slice [0, count) per
    // second-pass window (those are correlated on their own, see below)
    std::vector<Segment> resident = segs;
    for (const Segment& sg : cp.short_segs) resident.push_back(Segment{0, sg.b - sg.a});
    // and one local slice as long as a full chunk, for chunks that are correlated again on their
    // own window (non-finite samples nearby, below); the pick clamps it to the scores there are
    const int local_seg = (int)resident.size();
    // (seg_d is the index of a full window's LAST score: chunk + overlap - s + 1 scores in all)
    resident.push_back(Segment{0, std::max<long long>(base.seg_d + 1, 1)});
    if ((rc = upload_segments(c, resident))) return rc;
    if ((rc = c->badflag.ensure(sizeof(int) * n_hay))) return rc;
    int* h_bad = static_cast<int*>(c->badflag.p);
    memset(h_bad, 0, sizeof(int) * n_hay);
    if ((rc = c->failcnt.ensure(nsegs + 1))) return rc;
    if (nrm.on) {   // (the block energies of the largest haystack, before anything is queued)
        size_t max_len = 0;
        for (size_t k = 0; k < n_hay; ++k) if (cp.ns(k) > 0) max_len = std::max(max_len, lens[k]);
        if ((rc = norm_reserve(c, (long long)max_len))) return rc;
    }
    unsigned char* h_fail = static_cast<unsigned char*>(c->failcnt.p);
    memset(h_fail, 0, nsegs + 1);
    // A chunk whose certificate fails is redone on the device when the batch overlaps picks and transforms:
    // the pick marks the block pairs that feed it, K3 runs once more for those pairs with every run written
    // (from the haystack's own work matrix: two alternate) and the chunk is picked again -- all on the
    // second stream, no host round trip.  (Single calls redo such a chunk from the host, below.)
    const bool device_redo = sets.overlap && sparse_ok && !needle_is_segmented(h, o) && o.device_redo != 0;
    if (device_redo) {   // sized once for the haystack with the most block pairs: no pick of the batch waits for an allocation
        for (int set = 0; set < 2; ++set)
            if ((rc = c->redo_pairs[set].ensure(sizeof(int) * (size_t)std::max<long long>(need.npairs, 1)))) return rc;
    }
    SegHeader* h_hdr = static_cast<SegHeader*>(c->hdr.p);
    auto chunk_events = [&](size_t k, int stage) {
        if (hooks.chunk_fn)
            for (int i = 0; i < cp.n_chunks[k]; ++i)
                hooks.chunk_fn(hooks.chunk_user, G(k), (part ? part->chunk_base : 0) + (size_t)i,
                               part ? part->chunk_total : (size_t)cp.n_chunks[k], stage);
    };
    // Which path a failed chunk takes -- redone on the device, or from the host after the call -- depends on
    // when the first failure flag becomes visible to this loop: a race between host and GPU that no test can
    // steer.  The results are identical either way; "debug_redo_arm_at" pins the switch-over to a haystack
    // index (0: armed from the start, -1: never) so that both paths and the switch are tested deterministically.
    const bool arm_forced = o.debug_redo_arm_at >= -1;
    bool redo_armed = device_redo && (arm_forced ? o.debug_redo_arm_at == 0 : h->redo_armed_left[sm] > 0);
    QueueingScope queueing(o.debug_no_realloc != 0);
    for (size_t k = 0; k < n_hay; ++k) {
        const int ns = cp.ns(k);
        if (cp.n_chunks[k] == 0) continue;
        if (device_redo && arm_forced) redo_armed = o.debug_redo_arm_at >= 0 && (long long)k >= o.debug_redo_arm_at;
        else if (device_redo && !redo_armed && (k & 3) == 0) {
            // (the flags of the haystacks queued so far: written by their picks, whenever those have run)
            const volatile unsigned char* f = h_fail;
            for (int i = 0; i < seg_off[k] && !redo_armed; ++i) redo_armed = f[i] != 0;
        }
        if (hooks.fn) hooks.fn(hooks.user, G(k), 0, (size_t)cp.n_chunks[k]);
        chunk_events(k, 0);
        if (ns == 0) continue;
        const long long out_count = (long long)(lens[k] - s + 1);
        const int set = sets.set();
        const PassPlan& pp = plans[k];
        ScoreSide& side = sets.side();
        float* d_scores = sets.scores();
        ScanRequest req = base;
        req.out = scan_buffers(side);
        // this set's work matrix, scores and summaries are overwritten: the pick (and redo) that last used them must be done
        // (On the host: this thread runs far ahead of the GPU -- it queues a haystack in 35 us, the GPU takes 700 -- so
        // waiting here for the pick of the haystack before the previous one leaves more than a haystack's work queued,
        // and the main stream is spared a barrier packet between K3 and the next K1: that boundary measured 6.5 us
        // instead of 11 - 27, profiles/r04/event_gaps.txt.  Option host_pick_wait = 0: the stream waits.)
        if ((rc = sets.wait_pick(o.host_pick_wait != 0))) return rc;
        int* d_redo = nullptr;
        if (redo_armed) {
            AM_HIP(hipMemsetAsync(c->redo_pairs[set].p, 0, sizeof(int) * (size_t)std::max<long long>(pp.g.npairs, 1), c->stream));
            d_redo = static_cast<int*>(c->redo_pairs[set].p);
        }
        // (i16 frames are always finite -- but a half-precision transform can overflow on them)
        int* bad = ((src_kind == 0 || o.half) && std::isfinite(factor)) ? &h_bad[k] : nullptr;
        if (pre) {
            // the pairs that were computed while the samples arrived are in the stream's own buffers:
            // only the rest is launched now, into the same buffers
            d_scores = pre->scores;
            req.out.stats32 = pre->stats32; req.out.wflags = pre->side;
            req.side_nblocks = pre->layout_nblocks;
            req.range_a = std::min(pre->pairs_done, pp.g.npairs) * 2 * pp.g.hop;
            req.range_b = out_count;
            req.skip_launch = req.range_a >= out_count;
        }
        if (batch_tails && tail_batchable(pp.tail)) {
            if (tail_slot[k] < 0) {   // the next batch: this haystack and the following ones with such a tail
                std::vector<size_t> members;
                for (size_t k2 = k; k2 < n_hay && members.size() < (size_t)kMaxTailBatch; ++k2)
                    if (tail_batchable(plans[k2].tail) && tail_slot[k2] < 0) {
                        tail_slot[k2] = (tail_batches & 1) * kMaxTailBatch + (int)members.size();
                        members.push_back(k2);
                    }
                if ((rc = launch_tail_batch(h, plans, members, tail_batches & 1, tslots, d_hays, lens, factor, src_kind))) return rc;
                ++tail_batches;
            }
            req.tail_by_caller = true;
        }
        ScanResult res{};
        if ((rc = run_correlation(h, o, d_hays[k], (long long)lens[k], 0, d_scores, out_count, factor, &req, &res, src_kind, &pp))) return rc;
        if ((rc = sets.k3_done())) return rc;
        if (req.tail_by_caller && res.fused) {
            // (behind the main pass in stream order, hence behind the batch that filled the slot; in front of the pick)
            const TailPlan& t = pp.tail;
            const BallotLayout bl = ballot_layout(res.sparse.log_n1, res.sparse.log_n2);
            const size_t blk = (size_t)(t.T / res.sparse.hop);
            ProfScope ps(c, KN_OTHER, c->stream2);
            AM_HIP(launch_tail_commit(c->stream2, static_cast<const float*>(c->tail_scores.p) + (size_t)tail_slot[k] * tslots.scores, d_scores + t.T,
                                      out_count - t.T, static_cast<const float2*>(c->tail_stats.p) + (size_t)tail_slot[k] * tslots.stats,
                                      const_cast<float2*>(res.sparse.stats32) + t.T / 32,
                                      res.sparse.wbits ? const_cast<unsigned long long*>(res.sparse.wbits) + blk * bl.words : nullptr, (long long)bl.words,
                                      res.sparse.tile_theta ? const_cast<float*>(res.sparse.tile_theta) + blk * bl.tiles : nullptr, (int)bl.tiles));
        }
        if (res.fused && res.sparse.wbits) {
            res.sparse.fail_flags = h_fail + seg_off[k];
            res.sparse.redo_pairs = (redo_armed && res.redo_ok) ? d_redo : nullptr;
        }
        if (nrm.on) {
            // behind K3 and the tail's commit (both ordered before the pick's stream by now), in front of the pick, which
            // then summarises the scores itself; the samples are the caller's (or io_in, which nothing overwrites before
            // this call has drained)
            if ((rc = normalise_scores(c, sets.pick_stream(), nrm, d_hays[k], (long long)lens[k], src_kind, 0, (long long)s, d_scores, 0, out_count)))
                return rc;
        }
        if ((rc = launch_pick(c, side, d_scores, out_count, seg_off[k], ns, p->min_prominence,
                              (long long)p->min_distance, bad, nrm.on ? nullptr : &res, seg_off[k], arena, pol, sets.pick_stream()))) return rc;
        if (res.fused && res.sparse.redo_pairs) {
            ScanCfg cfg = res.redo_cfg;
            cfg.margin = -1.0f;
            cfg.only_pairs = d_redo;
            { ProfScope ps(c, KN_OTHER, c->stream2);   // (not under "k3_cols_inv": an all-but-empty launch that queues behind the next haystack's kernels)
              AM_HIP(launch_k3(c->stream2, res.redo_job, res.redo_npairs, res.redo_work, res.redo_pl, res.redo_scale, cfg, res.redo_half)); }
            res.sparse.redo_pairs = nullptr; res.sparse.fail_flags = nullptr;
            if ((rc = launch_pick(c, side, d_scores, out_count, seg_off[k], ns, p->min_prominence, (long long)p->min_distance,
                                  nullptr, &res, seg_off[k], arena, pol, c->stream2, true))) return rc;
        }
        if ((rc = sets.pick_done())) return rc;
    }
    queueing.end();
    if ((rc = sets.drain())) return rc;   // the headers are in host memory once the peak kernels have finished
    int worst = AM_OK;
    std::vector<am_peak> all;
    std::vector<size_t> retry_f32;
    const int spare_hdr = (int)nsegs;
    for (size_t k = 0; k < n_hay; ++k) {
        const int s0 = seg_off[k], s1 = seg_off[k + 1];
        if (cp.n_chunks[k] == 0) continue;
        const long long out_count = (long long)(lens[k] - s + 1);
        // Non-finite scores out of a half-precision pipeline: most likely an overflow of f16's range in the
        // row transform (a strong component that needle and haystack share, e.g. a DC offset or a steady
        // tone, concentrates in a few bins).  The haystack is matched again in f32, after every other
        // result of this call has been collected (the pass reuses the call's result area).
        if (h_bad[k] && o.half) { retry_f32.push_back(k); continue; }
        if (!my && !nrm.on && !h_bad[k] && s1 > s0) {   // (a haystack with non-finite scores teaches the threshold nothing; NCC scores are no raw scores)
            std::vector<float> mins;
            int failed = 0;
            for (int i = s0; i < s1; ++i) { mins.push_back(h_hdr[i].seg_min); failed += h_fail[i] != 0; }
            std::sort(mins.begin(), mins.end());
            // many failed certificates: a score array that drifts (chunk minima in other block pairs than the tiles'
            // scores) -- the lowest minimum for a good while; a few, redone on the device: the background level
            if (failed * 8 > s1 - s0) h->conservative_left[sm] = 64;
            const bool robust = device_redo && h->conservative_left[sm] == 0;
            h->remember_min(sm, robust ? mins[mins.size() / 2] : mins.front());
            if (h->conservative_left[sm] > 0) --h->conservative_left[sm];
            if (failed) h->redo_armed_left[sm] = 64;
            else if (h->redo_armed_left[sm] > 0) --h->redo_armed_left[sm];
        }
        all.clear();
        // Non-finite samples (NaN, +-inf; f32 sources only).  The reference transforms every window
        // on its own (audio_matcher.rs:114-122): a window that holds such a sample gets NaN scores
        // throughout and yields no peak, every other window is untouched.  Here the sample has
        // poisoned the whole pair of overlap-save blocks around it, which reaches into neighbouring
        // chunks.  So, when a score kernel has reported a non-finite score for this haystack: find
        // the block pairs and the windows that hold such samples; a window that holds one yields
        // no peak; a clean window whose scores came from a poisoned pair is correlated again on its
        // own samples (as the reference does it) and picked from that.
        std::vector<char> drop, again;
        if (h_bad[k]) {
            if ((rc = classify_nonfinite(h, plans[k], (const float*)d_hays[k], lens[k], segs, s0, s1, &drop, &again))) return rc;
        }
        // collect in window order (audio_matcher.rs:132-133)
        for (int i = s0; i < s1; ++i) {
            if (!drop.empty() && drop[i - s0]) continue;
            const Segment sg = segs[i];
            if (!again.empty() && again[i - s0]) {
                ScanRequest one{};
                one.margin = -1.0f;
                if ((rc = pick_alone(h, o, p, advance_src(d_hays[k], (size_t)sg.a), (long long)cp.widths[i], factor, one, sg.b - sg.a,
                                     local_seg, Segment{0, sg.b - sg.a}, spare_hdr, (uint64_t)sg.a, src_kind, nrm, all))) return rc;
                continue;
            }
            if (!(h_hdr[i].overflow & 7)) { append_header_peaks(h_hdr[i], arena, all); continue; }
            // Rare: a write threshold was too high for this chunk (its minimum lies more than half a
            // prominence below the minimum some K3 tile sampled), its list found no room in the spill
            // arena, or more than AM_MAX_PEAKS_PER_CHUNK peaks passed the prominence filter (the
            // score buffers have moved on to later haystacks by now).  Redo the blocks that produce this
            // chunk's scores with every run written, in place in set 0 (same block layout, hence
            // bit-identical scores), and pick the chunk again with a spill arena of its own.
            ScanRequest full = base;   // (in set 0 of the context, with a tail of its own if the layout has one)
            full.margin = -1.0f;
            full.range_a = sg.a; full.range_b = sg.b;
            if ((rc = pick_alone(h, o, p, d_hays[k], (long long)lens[k], factor, full, out_count, i, sg, spare_hdr, 0, src_kind, nrm, all))) return rc;
        }
        // second pass (MyConvolve scaling only): the shorter windows at the end of the haystack, at their offsets (audio_matcher.rs:126)
        for (int i = cp.short_off[k]; i < cp.short_off[k + 1]; ++i) {
            const Segment sg = cp.short_segs[i];
            ScanRequest one{};
            one.margin = -1.0f;
            if ((rc = pick_alone(h, o, p, advance_src(d_hays[k], (size_t)sg.a), (long long)cp.short_w[i], scale_factor(h, p->scale, cp.short_w[i]),
                                 one, sg.b - sg.a, (int)nsegs + i, Segment{0, sg.b - sg.a}, spare_hdr, (uint64_t)sg.a, src_kind, nrm, all))) return rc;
        }
        if (part) {   // unmerged, in window order (audio_matcher.rs:132-133), at their positions in the whole haystack
            for (am_peak& q : all) { q.start += part->first_sample; q.end += part->first_sample; }
            part->raw->insert(part->raw->end(), all.begin(), all.end());
            n_out[G(k)] = all.size();
            rc = AM_OK;
        } else rc = merge_peaks(all, p, o.surrounding_from != 0, out ? out + G(k) * cap_per_hay : nullptr, cap_per_hay, &n_out[G(k)]);
        chunk_events(k, 1);
        if (hooks.fn) hooks.fn(hooks.user, G(k), 1, (size_t)cp.n_chunks[k]);
        if (rc == AM_ERR_CAPACITY) worst = rc;
        else if (rc) return rc;
    }
    for (size_t k : retry_f32) {
        const long long keep = h->opt_half;
        h->opt_half = 0;
        rc = match_alone(h, d_hays[k], lens[k], p, out, cap_per_hay, G(k), n_out, src_kind, part, &worst);
        h->opt_half = keep;
        chunk_events(k, 1);
        if (hooks.fn) hooks.fn(hooks.user, G(k), 1, (size_t)cp.n_chunks[k]);
        if (rc) return rc;
    }
    return worst;
}

// BASELINE config 4: several needles against a batch of resident haystacks = the per-file loop of
// matcher::run (matcher/mod.rs:42-87) around N snippets.  Per haystack the forward column pass (K1)
// runs once; needles are then taken in groups that share the forward row transforms of K2
// (k2_rows_r16_group_planes), each needle with its own inverse rows, K3 (fused scan) and peak pick.  The
// pick of (haystack, needle) runs on the second stream beside the next needle's K3 / the next
// haystack's K1 and K2; the score-side buffers alternate between two sets, as in match_many.
// Needles must share one length, unless `varlen` (am_match_multi_varlen*): then every haystack has ONE block layout,
// that of the longest needle -- hop N - S_max + 1 on the plan it would pick -- and a shorter needle's spectrum on it is
// that of the needle zero-padded to S_max (the zeros change none of its scores t <= len - S_j, nor its energy).  The
// main pass reaches the shortest needle's last score; needle j's scores end at len - S_j + 1 (K3Group::out_count: the
// partial sums behind it are neither written, summarised nor picked), and each needle has a chunk plan of its own (its
// length, overlap overlaps[j]), result headers and redo.  The needles are grouped longest first.
// Result slot of (haystack k of the caller's batch, needle j): G(k) * nn + j.
int match_multi_many(am_needle* const* needles, size_t nn, const void* const* d_hays, const size_t* lens, size_t n_hay,
                     int src_kind, const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out,
                     size_t index_base, size_t index_stride, const uint64_t* overlaps, bool varlen) {
    am_needle* h0 = needles[0];
    Ctx* c = h0->ctx;
    const Opts o = snapshot_opts(h0);
    const PeakPolicy pol = o.peak_policy();
    const Hooks hooks = snapshot_hooks();
    auto G = [&](size_t k) { return index_base + k * index_stride; };
    for (size_t j = 0; j < nn; ++j) {
        if (!needles[j] || needles[j]->ctx != c) return fail(AM_ERR_INVALID_ARG, "needles must live on one device");
        if (!varlen && needles[j]->n != h0->n) return fail(AM_ERR_INVALID_ARG, "am_match_multi: needles must have equal length");
    }
    if (o.score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    if (p->chunk == 0) return fail(AM_ERR_INVALID_ARG, "chunk must be > 0");
    if (p->scale != AM_SCALE_NONE && p->scale != AM_SCALE_LIB)
        return fail(AM_ERR_INVALID_ARG, "am_match_multi supports AM_SCALE_NONE and AM_SCALE_LIB");
    for (size_t k = 0; k < n_hay; ++k)
        for (size_t j = 0; j < nn; ++j) n_out[G(k) * nn + j] = 0;
    // needle j's parameters: the call's, with its own overlap
    std::vector<am_match_params> pj(nn, *p);
    if (overlaps)
        for (size_t j = 0; j < nn; ++j) pj[j].overlap = overlaps[j];
    int rc, worst = AM_OK;
    // partitioned needles (longer than kSegmentFrom samples) share nothing here: pair by pair; the others go in groups,
    // longest first (a stable order: needles of one length keep the caller's)
    std::vector<size_t> ord;
    bool any_segmented = false;
    for (size_t j = 0; j < nn; ++j) {
        if (needle_is_segmented(needles[j], o)) any_segmented = true;
        else ord.push_back(j);
    }
    if (any_segmented)
        for (size_t k = 0; k < n_hay; ++k)
            for (size_t j = 0; j < nn; ++j)
                if (needle_is_segmented(needles[j], o) &&
                    (rc = match_alone(needles[j], d_hays[k], lens[k], &pj[j], out, cap_per_pair, G(k) * nn + j, n_out, src_kind, nullptr, &worst)))
                    return rc;
    if (ord.empty()) return worst;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return needles[a]->n > needles[b]->n; });
    const size_t m = ord.size();                        // grouped needles; local index i is needle ord[i]
    const size_t s = needles[ord[0]]->n;                // the longest: the block layout's
    const size_t s_min = needles[ord[m - 1]]->n;        // the shortest: the layout's score count
    const int sm = p->scale == AM_SCALE_LIB ? 1 : 0;
    // one chunk plan per distinct (length, overlap); their chunk lists back to back in the resident list, needle i's
    // result headers at hdr_base[i] + (its plan's chunk index)
    std::vector<ChunkPlan> cps;
    std::vector<std::pair<size_t, uint64_t>> keys;
    std::vector<int> plan_of(m), seg_base, hdr_base(m);
    for (size_t i = 0; i < m; ++i) {
        const size_t j = ord[i];
        const std::pair<size_t, uint64_t> key(needles[j]->n, pj[j].overlap);
        const size_t u = (size_t)(std::find(keys.begin(), keys.end(), key) - keys.begin());
        if (u == keys.size()) {
            keys.push_back(key);
            cps.emplace_back();
            plan_chunks(key.first, d_hays, lens, n_hay, &pj[j], o, false, (size_t)-1, &cps.back());
        }
        plan_of[i] = (int)u;
    }
    std::vector<Segment> all_segs;
    size_t max_scores = 0, max_segs = 1, nhdr = 0;
    bool too_many = false;
    for (const ChunkPlan& cpu : cps) {
        seg_base.push_back((int)all_segs.size());
        all_segs.insert(all_segs.end(), cpu.segs.begin(), cpu.segs.end());
        max_scores = std::max(max_scores, cpu.max_scores);
        max_segs = std::max(max_segs, cpu.max_segs);
        too_many = too_many || cpu.too_many(1);
    }
    for (size_t i = 0; i < m; ++i) { hdr_base[i] = (int)nhdr; nhdr += cps[plan_of[i]].segs.size(); }
    if (nhdr == 0) return worst;
    if (too_many || nhdr > (size_t)1 << 24) return fail(AM_ERR_INVALID_ARG, "chunk size too small for this batch (too many chunks)");
    auto plan_i = [&](size_t i) -> const ChunkPlan& { return cps[plan_of[i]]; };
    auto seg_of = [&](size_t k, size_t i) { return seg_base[plan_of[i]] + plan_i(i).seg_off[k]; };
    // result headers of (haystack k, needle i): the needle's, the haystack's slice inside
    auto hdr_of = [&](size_t k, size_t i) { return hdr_base[i] + plan_i(i).seg_off[k]; };
    // chunks of haystack k for the progress callbacks: the most any needle has
    auto ns_max = [&](size_t k) { int n = 0; for (const ChunkPlan& cpu : cps) n = std::max(n, cpu.ns(k)); return n; };
    // the scores needle i has in haystack k (<= 0: the haystack is shorter than the needle)
    auto count_of = [&](size_t k, size_t i) { return (long long)lens[k] - (long long)needles[ord[i]]->n + 1; };
    // each haystack's block layout
    std::vector<Geometry> geo(n_hay);
    std::vector<TailPlan> tails(n_hay);   // the odd last block on the 2^21 plan (TailPlan), for haystacks whose needle groups all take the grouped K3
    size_t max_matrix = 0, max_wflags = 0, max_tail = 0;
    for (size_t k = 0; k < n_hay; ++k) {
        if (ns_max(k) == 0) continue;
        const long long out_count = (long long)(lens[k] - s_min + 1);
        if ((rc = plan_geometry(s, out_count, o, &geo[k]))) return rc;
        max_matrix = std::max(max_matrix, (size_t)geo[k].npairs * (size_t)geo[k].N);
        { const Plan* plk = nullptr; if ((rc = get_plan(c, geo[k].logN, &plk))) return rc; max_wflags = std::max(max_wflags, sparse_bytes(geo[k].nblocks, plk->dev)); }
        tail_plan(s, out_count, o, geo[k], &tails[k]);
    }
    // every needle's spectrum for every plan in use, before the work matrix is filled (building one uses it)
    std::map<int, std::vector<const float2*>> hcs;
    auto spectra = [&](int logN) -> int {
        if (hcs.count(logN)) return AM_OK;
        const Plan* pl = nullptr;
        int rc2 = get_plan(c, logN, &pl);
        std::vector<const float2*>& v = hcs[logN];
        v.resize(m);
        HalfScale hs;
        for (size_t i = 0; i < m && !rc2; ++i) rc2 = needle_k2_spectrum(needles[ord[i]], o, pl, &v[i], &hs);
        return rc2;
    };
    for (size_t k = 0; k < n_hay; ++k)
        if (ns_max(k) > 0 && (rc = spectra(geo[k].logN))) return rc;
    const size_t group_opt = (size_t)std::min<long long>(std::max<long long>(1, o.needle_group), kMaxNeedleGroup);
    // The tail needs every needle group of the haystack on the grouped-K3 path (the other paths keep the full layout):
    // f32, groups of at least two needles each, the 512-row plan with a 256-row tail.
    {
        const bool groups_ok = o.k3_group && group_opt > 1 && m > 1 && !o.half && (m % group_opt) != 1 && c->stream_tail != nullptr;
        for (size_t k = 0; k < n_hay; ++k) {
            if (!tails[k].on) continue;
            const Plan* plk = nullptr;
            if (ns_max(k) == 0 || !groups_ok || !tail_batchable(tails[k]) || get_plan(c, geo[k].logN, &plk) || !plan_is_c512(plk->dev)) {
                tails[k].on = false;
                continue;
            }
            max_tail = std::max(max_tail, (size_t)tails[k].g.N);
            if ((rc = spectra(tails[k].g.logN))) return rc;   // the needles' spectra on the tail's plan
        }
        if (max_tail) {
            if ((rc = c->work_tail.ensure(std::max(c->work_tail.cap, max_tail * sizeof(float2))))) return rc;
            if ((rc = c->work_tail2.ensure(std::min(group_opt, m) * max_tail * sizeof(float2)))) return rc;
        }
    }
    size_t n_pairs_active = 0;
    for (size_t k = 0; k < n_hay; ++k) n_pairs_active += ns_max(k) > 0 ? m : 0;
    ScoreSets sets(c, o, n_pairs_active);
    DevBuf& fwd = c->side[0].work;   // the haystack's forward columns (K1), shared by every needle
    if ((rc = fwd.ensure(max_matrix * sizeof(float2)))) return rc;
    if ((rc = c->work2.ensure(std::min(group_opt, m) * max_matrix * sizeof(float2)))) return rc;
    if ((rc = sets.size(max_scores, max_segs))) return rc;
    for (int set = 0; set < sets.count(); ++set) {
        if ((rc = c->side[set].stats32.ensure((max_scores + 31) / 32 * sizeof(float2)))) return rc;
        if ((rc = c->side[set].wflags.ensure(max_wflags))) return rc;
    }
    // one K3 launch per needle group: every needle of a group (two groups in flight) has its own score-side buffers
    const size_t k3_group = (o.k3_group && group_opt > 1 && m > 1 && !o.half && max_wflags > 0) ? std::min(group_opt, m) : 0;
    for (int set = 0; set < sets.count(); ++set)
        for (size_t q = 0; q < k3_group; ++q) {
            if ((rc = c->grp_scores[set][q].ensure(max_scores * sizeof(float)))) return rc;
            if ((rc = c->grp_stats32[set][q].ensure((max_scores + 31) / 32 * sizeof(float2)))) return rc;
            if ((rc = c->grp_wflags[set][q].ensure(max_wflags))) return rc;
        }
    if (k3_group && o.pick_group) {   // ... and the scratch of the group's picks, which run as one set of launches
        const size_t total = k3_group * max_segs;
        for (size_t z = 0; z < k3_group; ++z)
            if ((rc = c->grp_stats[z].ensure((max_scores + kTile - 1) / kTile * sizeof(float2)))) return rc;
        if ((rc = wide_reserve(c, total))) return rc;
        if ((rc = c->side[0].peaks.ensure(total * AM_MAX_PEAKS_PER_CHUNK * sizeof(am_peak)))) return rc;
    }
    PeakArena arena{};
    if ((rc = prepare_results(c, nhdr, nhdr * 8 + 4096, &arena))) return rc;
    if ((rc = upload_segments(c, all_segs))) return rc;
    if ((rc = c->badflag.ensure(sizeof(int) * n_hay))) return rc;
    int* h_bad = static_cast<int*>(c->badflag.p);
    memset(h_bad, 0, sizeof(int) * n_hay);
    SegHeader* h_hdr = static_cast<SegHeader*>(c->hdr.p);
    const float margin = write_margin(o, p);
    QueueingScope queueing(o.debug_no_realloc != 0);
    for (size_t k = 0; k < n_hay; ++k) {
        if (ns_max(k) == 0) continue;
        if (hooks.fn) hooks.fn(hooks.user, G(k), 0, (size_t)ns_max(k));
        const Geometry& g = geo[k];
        const Plan* pl = nullptr;
        if ((rc = get_plan(c, g.logN, &pl))) return rc;
        const std::vector<const float2*>& hc = hcs[g.logN];
        const long long out_count = (long long)(lens[k] - s_min + 1);
        const int half = (o.half && (plan_is_r16(pl->dev) || plan_is_c512(pl->dev))) ? (o.half >= 2 ? 2 : 1) : 0;
        const size_t group = (!half && plan_k2_has_group(pl->dev)) ? group_opt : 1;
        const size_t matrix = (size_t)g.npairs * (size_t)g.N;
        const bool fused = plan_fuses_scan(pl->dev, g);
        // The odd last block (TailPlan): the main pass -- K1 here, every group's K2 and K3 below -- stops at the even
        // block boundary, the scores behind it come from one pair of the 2^21 plan: K1 once, then per needle group one
        // row-kernel launch and one K3 launch (every run written) behind the group's own, and the main layout's
        // ballots / thresholds of that block preset for the group's needles.
        const TailPlan& tail = tails[k];
        const int main_pairs = (int)(tail.on ? g.npairs - 1 : g.npairs);
        const Plan* plt = nullptr;
        Job job{}, job_t{};
        job.src = d_hays[k]; job.src_len = (long long)lens[k]; job.lead = 0; job.src_kind = src_kind;
        job.out_count = tail.on ? tail.T : out_count; job.hop = (int)g.hop; job.nblocks = (int)(tail.on ? g.nblocks - 1 : g.nblocks); job.first_pair = 0;
        { ProfScope ps(c, KN_K1); AM_HIP(launch_k1(c->stream, job, main_pairs, (float2*)fwd.p, pl->dev, half)); }
        if (tail.on) {
            if ((rc = get_plan(c, tail.g.logN, &plt))) return rc;
            job_t = tail_job(tail, d_hays[k], (long long)lens[k], out_count, src_kind);
            ProfScope ps(c, KN_OTHER);
            AM_HIP(launch_k1(c->stream, job_t, 1, (float2*)c->work_tail.p, plt->dev, 0));
        }
        for (size_t i = 0; i < m; ++i) {
            am_needle* h = needles[ord[i]];
            const size_t in_group = i % group;
            const float2* inv_rows = (const float2*)c->work2.p + in_group * matrix;   // this needle's inverse rows
            const size_t gn = std::min(group, m - (i - in_group));
            if (group > 1 && in_group == 0) {
                K2Group grp{};
                grp.n = (int)gn;
                for (int q = 0; q < grp.n; ++q) { grp.hc[q] = hc[i + q]; grp.dst[q] = (float2*)c->work2.p + (size_t)q * matrix; }
                { ProfScope ps(c, KN_K2); AM_HIP(launch_k2_group(c->stream, main_pairs, (const float2*)fwd.p, grp, pl->dev)); }
                if (tail.on) {
                    K2Group gt{};
                    gt.n = (int)gn;
                    const std::vector<const float2*>& hct = hcs[tail.g.logN];
                    for (int q = 0; q < gt.n; ++q) { gt.hc[q] = hct[i + q]; gt.dst[q] = (float2*)c->work_tail2.p + (size_t)q * (size_t)tail.g.N; }
                    ProfScope ps(c, KN_OTHER);
                    AM_HIP(launch_k2_group(c->stream, 1, (const float2*)c->work_tail.p, gt, plt->dev));
                }
            }
            // The K3s of the group as one launch (needle index on blockIdx.y), the group's picks queued behind it.
            const bool grouped_k3 = k3_group && group > 1 && gn > 1 && fused && !half && plan_k3_has_group(pl->dev);
            if (grouped_k3 && in_group != 0) continue;   // (handled with the group's first needle)
            const int set = sets.set();
            if (grouped_k3) {
                K3Group kg{};
                kg.n = (int)gn;
                ScanResult scans[kMaxNeedleGroup];   // what each member's pick reads
                int* const bad = (src_kind == 0 || o.half) ? &h_bad[k] : nullptr;
                ScanCfg common{};
                bool same_plan = true, same_edges = true;
                for (size_t q = 0; q < gn; ++q) {
                    am_needle* hq = needles[ord[i + q]];
                    ScanCfg cfg{};
                    fill_scan_cfg(&cfg, c->grp_stats32[set][q].p, c->grp_wflags[set][q].p, g.nblocks, pl->dev, margin, hq->hist_min(sm),
                                  (long long)p->chunk, (long long)(p->chunk + pj[ord[i + q]].overlap) - (long long)hq->n);
                    scans[q] = ScanResult{};
                    scans[q].fused = true;
                    scans[q].sparse = sparse_view(cfg, g.hop, pl->dev);
                    if (q == 0) common = cfg;
                    same_plan = same_plan && plan_of[i + q] == plan_of[i];
                    same_edges = same_edges && cfg.seg_d == common.seg_d;
                    kg.work[q] = (const float2*)c->work2.p + q * matrix;
                    kg.dst[q] = (float*)c->grp_scores[set][q].p;
                    kg.stats32[q] = cfg.stats32; kg.wbits[q] = cfg.wbits; kg.tile_theta[q] = cfg.tile_theta;
                    kg.hist_min[q] = cfg.hist_min;
                    kg.out_scale[q] = half_scale(hq, o, pl->dev).k3(scale_factor(hq, p->scale, 1));
                    kg.out_count[q] = std::max(0ll, std::min(count_of(k, i + q), job.out_count));
                    kg.seg_d[q] = cfg.seg_d;
                }
                kg.seg_c = common.seg_c; kg.inv_c = common.inv_c;
                // members whose chunk edges differ work them out themselves: no edge table from the launch's geometry
                if (!same_edges) common.seg_c = 0;
                // K3 overwrites this set's scores and summaries: the picks that last read them must be done
                if ((rc = sets.wait_pick(false))) return rc;
                { ProfScope ps(c, KN_K3); AM_HIP(launch_k3_group(c->stream, job, main_pairs, kg, pl->dev, common)); }
                if (tail.on) {
                    K3Group kt = kg;
                    for (size_t q = 0; q < gn; ++q) {
                        kt.work[q] = (const float2*)c->work_tail2.p + q * (size_t)tail.g.N;
                        kt.dst[q] = kg.dst[q] + tail.T; kt.stats32[q] = kg.stats32[q] + tail.T / 32;
                        kt.wbits[q] = nullptr; kt.tile_theta[q] = nullptr; kt.hist_min[q] = FLT_MAX;
                        kt.out_count[q] = std::max(0ll, count_of(k, i + q) - tail.T);
                        kt.seg_d[q] = 0;
                    }
                    kt.seg_c = 0; kt.inv_c = 0.0;
                    ScanCfg dense{};
                    dense.stats32 = kt.stats32[0]; dense.margin = -1.0f; dense.hist_min = FLT_MAX;
                    ProfScope ps(c, KN_OTHER);
                    AM_HIP(launch_k3_group(c->stream, job_t, 1, kt, plt->dev, dense));
                    if (margin >= 0.0f)
                        AM_HIP(launch_tail_preset_group(c->stream, kg, (long long)(g.nblocks - 1), pl->dev.logN1, pl->dev.logN2));
                }
                if ((rc = sets.k3_done())) return rc;
                if (o.pick_group && same_plan && plan_i(i).ns(k) > 0) {   // (one chunk list for the whole group)
                    int hoff[kMaxNeedleGroup];
                    for (size_t q = 0; q < gn; ++q) hoff[q] = hdr_of(k, i + q);
                    if ((rc = launch_pick_group(c, kg, count_of(k, i), seg_of(k, i), plan_i(i).ns(k), p->min_prominence, (long long)p->min_distance,
                                                scans[0].sparse, bad, hoff, arena, pol, sets.pick_stream()))) return rc;
                } else
                for (size_t q = 0; q < gn; ++q)
                    if (plan_i(i + q).ns(k) > 0 &&
                        // (the picks of a call run one after the other: they share set 0's tile summaries and peak lists)
                        (rc = launch_pick(c, c->side[0], kg.dst[q], count_of(k, i + q), seg_of(k, i + q), plan_i(i + q).ns(k), p->min_prominence,
                                          (long long)p->min_distance, bad, &scans[q], hdr_of(k, i + q), arena, pol, sets.pick_stream()))) return rc;
                if ((rc = sets.pick_done())) return rc;
                continue;
            }
            const int ns = plan_i(i).ns(k);
            if (ns == 0) continue;   // (a haystack shorter than this needle: nothing to correlate)
            float* d_scores = sets.scores();
            Job jn = job;   // (this needle's scores end before the layout's: tails only run on the grouped path)
            jn.dst = d_scores;
            jn.out_count = std::min(count_of(k, i), job.out_count);
            ScoreSide& side = sets.side();
            int* const bad = (src_kind == 0 || o.half) ? &h_bad[k] : nullptr;   // (i16 frames are always finite; an f16 transform can overflow)
            ScanResult scan{};
            scan.fused = fused;
            scan.sparse = SparseScores{nullptr, nullptr, nullptr, (int)g.hop, pl->dev.logN2, pl->dev.logN1, 1.0 / (double)g.hop};
            ScanCfg cfg{};
            if (fused) {
                fill_scan_cfg(&cfg, side.stats32.p, side.wflags.p, g.nblocks, pl->dev, margin, h->hist_min(sm), (long long)p->chunk,
                              (long long)(p->chunk + pj[ord[i]].overlap) - (long long)h->n);
                scan.sparse = sparse_view(cfg, g.hop, pl->dev);
            }
            const float factor = scale_factor(h, p->scale, 1);
            const HalfScale hs = half_scale(h, o, pl->dev);
            if (group == 1) {
                ProfScope ps(c, KN_K2);
                AM_HIP(launch_k2(c->stream, (int)g.npairs, (float2*)fwd.p, hc[i], pl->dev, (float2*)c->work2.p, hs.level, hs.hscale, hs.pre));
            }
            // K3 overwrites this set's scores and summaries: the pick that last read them must be done
            if ((rc = sets.wait_pick(false))) return rc;
            { ProfScope ps(c, KN_K3); AM_HIP(launch_k3(c->stream, jn, (int)g.npairs, inv_rows, pl->dev, hs.k3(factor), cfg, half)); }
            if ((rc = sets.k3_done())) return rc;
            if ((rc = launch_pick(c, side, d_scores, count_of(k, i), seg_of(k, i), ns, p->min_prominence, (long long)p->min_distance,
                                  bad, &scan, hdr_of(k, i), arena, pol, sets.pick_stream()))) return rc;
            if ((rc = sets.pick_done())) return rc;
        }
    }
    queueing.end();
    if ((rc = sets.drain())) return rc;
    std::vector<am_peak> all;
    std::vector<std::pair<size_t, size_t>> redo;
    for (size_t k = 0; k < n_hay; ++k) {
        for (size_t i = 0; i < m; ++i) {
            const int ns = plan_i(i).ns(k);
            if (ns == 0) continue;
            const size_t j = ord[i];
            const SegHeader* hd = h_hdr + hdr_of(k, i);
            const size_t slot = G(k) * nn + j;
            // Non-finite samples poison whole block pairs for every needle (see match_many): such a
            // haystack goes through the single-needle path, which gives every window the reference's
            // answer.  So does a pair with a failed certificate, a lost spill or more than
            // AM_MAX_PEAKS_PER_CHUNK peaks in a chunk.
            bool again = h_bad[k] != 0;
            float lowest = FLT_MAX;
            for (int q = 0; q < ns && !again; ++q) {
                if (hd[q].overflow & 7) again = true;
                lowest = std::min(lowest, hd[q].seg_min);
            }
            if (!again) needles[j]->remember_min(sm, lowest);
            if (again) { redo.emplace_back(k, j); continue; }
            all.clear();
            for (int q = 0; q < ns; ++q) append_header_peaks(hd[q], arena, all);
            rc = merge_peaks(all, &pj[j], o.surrounding_from != 0, out ? out + slot * cap_per_pair : nullptr, cap_per_pair, &n_out[slot]);
            if (rc == AM_ERR_CAPACITY) worst = rc;
            else if (rc) return rc;
        }
    }
    // the single-needle path reuses the result area: it runs after everything else has been collected
    for (const auto& kj : redo)
        if ((rc = match_alone(needles[kj.second], d_hays[kj.first], lens[kj.first], &pj[kj.second], out, cap_per_pair, G(kj.first) * nn + kj.second,
                              n_out, src_kind, nullptr, &worst))) return rc;
    if (hooks.fn)
        for (size_t k = 0; k < n_hay; ++k)
            if (ns_max(k) > 0) hooks.fn(hooks.user, G(k), 1, (size_t)ns_max(k));
    return worst;
}

}  // namespace am
