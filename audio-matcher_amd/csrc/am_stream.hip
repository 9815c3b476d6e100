// am_stream.hip -- streaming ingest (am_match_stream_*): block pairs are transformed while the samples arrive.
#include "am_internal.h"

// ---------------------------------------------------------------------------
// Streaming ingest: calc_chunks consumes a lazy ExactSizeIterator (audio_matcher.rs:88-97; the
// windows are cut as the decoder yields frames, :104, mp3_reader.rs:13-41).  The stream object owns
// the haystack's device buffer and a set of score-side buffers; am_match_stream_push copies a block
// of samples on a copy stream and launches K1 / K2 / K3 for every block pair whose samples have
// arrived completely, so transfer (or decoding) and transforms overlap.
struct am_stream {
    am_needle* h = nullptr;
    int fmt = AM_FMT_F32_MONO;
    am_match_params p{};
    am::DevBuf hay, scores, stats32, side;
    size_t cap = 0, len = 0;          // elements (f32 samples or stereo frames, 4 bytes each); len = accepted so far
    size_t sent = 0;                  // elements whose host-to-device copy has been issued (len - sent sit in the staging ring)
    hipStream_t copy_stream = nullptr;
    hipEvent_t copied = nullptr;
    // Two-slot staging ring in pinned host memory: a push of a decoder-sized piece (minimp3 yields 1152 frames,
    // mp3_reader.rs:28-37) is a host memcpy into the current slot and returns; a full slot goes to the device as one
    // asynchronous copy while the other slot fills.  Large pushes bypass the ring (one copy straight from the caller's
    // buffer, at link speed when that buffer is pinned: am_host_alloc / am_host_register).
    static constexpr size_t kStageElems = (size_t)1 << 20;    // 4 MB per slot
    static constexpr size_t kDirectElems = (size_t)1 << 18;   // pushes of 1 MB and more are copied directly
    am::HostBuf stage[2];
    hipEvent_t staged[2] = {nullptr, nullptr};                 // the slot's last copy has left it
    bool stage_busy[2] = {false, false};
    int cur = 0;
    size_t fill = 0;                  // elements in the current slot
    bool early = false;               // block pairs may be launched before the length is known
    long long pairs_done = 0;
    am::Geometry geo{};               // the provisional block layout (from the capacity)
    float margin = 0.f;               // the write-threshold margin the early pairs were launched with (< 0: every run written)
    bool failed = false;
};

namespace am {

// (re)computes the provisional layout for the stream's capacity and sizes its score-side buffers
static int stream_layout(am_stream* st) {
    am_needle* h = st->h;
    const Opts o = snapshot_opts(h);
    st->early = false;
    st->pairs_done = 0;
    if (st->cap < h->n || st->p.scale == AM_SCALE_MY || st->p.chunk == 0) return AM_OK;
    if (o.log_n == 0 && (long long)h->n > kWidestFromSamples) return AM_OK;    // the plan depends on the final length / the needle is partitioned
    const long long out_cap = (long long)(st->cap - h->n + 1);
    PassPlan pp;   // (no tail: the early pairs fix the layout before the length is known)
    int rc = pass_plan(h, o, out_cap, false, &pp);
    if (rc) return rc;
    // direct summation has no blocks; small generic plans without the fused scan: nothing to overlap
    if (pp.kind != PassKind::Transform || !pp.fused) return AM_OK;
    st->geo = pp.g;
    if ((rc = st->scores.ensure((size_t)out_cap * sizeof(float)))) return rc;
    if ((rc = st->stats32.ensure(pp.need.stats32))) return rc;
    if ((rc = st->side.ensure(pp.need.side))) return rc;
    st->early = true;
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" {

// ---- streaming ingest -------------------------------------------------------------------
int am_match_stream_begin(const am_needle* hc, int sample_format, size_t expected_len, const am_match_params* p, am_stream** out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!p || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format))) return rc;
    if (p->chunk == 0) return fail(AM_ERR_INVALID_ARG, "chunk must be > 0");
    if (p->scale < AM_SCALE_NONE || p->scale > AM_SCALE_MY) return fail(AM_ERR_INVALID_ARG, "bad scale");
    if (snapshot_opts(h).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    am_stream* st = new am_stream();
    st->h = h; st->fmt = sample_format; st->p = *p;
    if (hipStreamCreateWithFlags(&st->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&st->copied, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&st->staged[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&st->staged[1], hipEventDisableTiming) != hipSuccess) {
        am_match_stream_destroy(st);
        return fail(AM_ERR_HIP, "hipStreamCreate(stream ingest)");
    }
    // the size hint of the reference's iterator (mp3_duration x sample rate, matcher/mod.rs:77-83) may be off
    // by a little: leave room, so that a slightly longer file does not force a new layout
    st->cap = expected_len ? expected_len + expected_len / 64 + 65536 : 0;
    if (st->cap) {
        if ((rc = st->hay.ensure(st->cap * 4)) || (rc = stream_layout(st))) { const std::string keep = t_err; am_match_stream_destroy(st); t_err = keep; return rc; }
    }
    *out = st;
    return AM_OK;
}

// the current staging slot goes to the device (asynchronously); the other slot becomes current
static int stream_flush_slot(am_stream* st) {
    if (st->fill == 0) return AM_OK;
    const int b = st->cur;
    hipError_t e = hipMemcpyAsync(static_cast<char*>(st->hay.p) + st->sent * 4, st->stage[b].p, st->fill * 4, hipMemcpyHostToDevice, st->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(st->staged[b], st->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(st->copied, st->copy_stream);
    if (e != hipSuccess) { st->failed = true; return hip_fail(e, "stream ingest: copy"); }
    st->stage_busy[b] = true;
    st->sent += st->fill;
    st->fill = 0;
    st->cur = b ^ 1;
    return AM_OK;
}

// K1 / K2 / K3 for every block pair whose samples are on their way to the device (st->sent)
static int stream_launch_ready_pairs(am_stream* st) {
    if (!st->early) return AM_OK;
    am_needle* h = st->h;
    Ctx* c = h->ctx;
    // pairs whose two blocks lie completely inside what has arrived: K1 reads [2q hop, (2q + 1) hop + N)
    const Geometry& g = st->geo;
    const long long have = (long long)st->sent;
    long long ready = have >= g.hop + g.N ? ((have - g.N) / g.hop - 1) / 2 + 1 : 0;
    ready = std::min(ready, g.npairs);
    if (ready - st->pairs_done < 1) return AM_OK;
    const Opts o = snapshot_opts(h);
    PassPlan now;
    int rc = pass_plan(h, o, (long long)(st->cap - h->n + 1), false, &now);
    if (rc) return rc;
    if (now.kind != PassKind::Transform || now.g.logN != g.logN || now.g.hop != g.hop) {   // an option changed under the stream: start over at finish
        st->early = false; st->pairs_done = 0;
        return AM_OK;
    }
    ScanRequest scan{};
    scan.margin = write_margin(o, &st->p);   // (stream_layout leaves MyConvolve scaling without early pairs)
    scan.hist_min = h->hist_min(st->p.scale == AM_SCALE_LIB ? 1 : 0);
    scan.seg_c = (long long)st->p.chunk;
    scan.seg_d = (long long)(st->p.chunk + st->p.overlap) - (long long)h->n;
    if (st->pairs_done > 0 && scan.margin != st->margin) {
        // "dense_scores" changed between two pushes: the early pairs were written under another rule than the
        // rest would be -- start over at finish
        st->early = false; st->pairs_done = 0;
        return AM_OK;
    }
    st->margin = scan.margin;
    scan.out = ScanBuffers{&c->side[0].work, &st->stats32, &st->side};
    scan.side_nblocks = g.nblocks;
    scan.range_a = st->pairs_done * 2 * g.hop;
    scan.range_b = ready * 2 * g.hop;
    AM_HIP(hipStreamWaitEvent(c->stream, st->copied, 0));   // the kernels read what has been copied so far
    rc = run_correlation(h, o, st->hay.p, (long long)st->cap, 0, (float*)st->scores.p, (long long)(st->cap - h->n + 1),
                         scale_factor(h, st->p.scale, 1), &scan, nullptr, st->fmt, &now);
    if (rc) { st->failed = true; return rc; }
    st->pairs_done = ready;
    return AM_OK;
}

int am_match_stream_push(am_stream* st, const void* samples, size_t n) {
    if (!st || !st->h || (!samples && n)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (st->failed) return fail(AM_ERR_INVALID_ARG, "stream is in a failed state: destroy it");
    if (n == 0) return AM_OK;
    am_needle* h = st->h;
    int rc = check_needle(h);
    if (rc) return rc;
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (st->len + n > st->cap) {
        // longer than announced: a larger buffer (contents moved on the device) and a new provisional layout;
        // the pairs computed so far are computed again (the layout may differ)
        const size_t want = std::max(st->len + n, st->cap * 2 + 65536);
        DevBuf bigger;
        if ((rc = bigger.ensure(want * 4))) { st->failed = true; return rc; }
        hipError_t e = hipStreamSynchronize(st->copy_stream);
        if (e == hipSuccess && st->sent) e = copy_on_stream(c, bigger.p, st->hay.p, st->sent * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { bigger.release(); st->failed = true; return hip_fail(e, "stream ingest: grow"); }
        st->hay.release();
        st->hay = bigger;
        st->cap = want;
        if ((rc = stream_layout(st))) { st->failed = true; return rc; }
    }
    if (n >= am_stream::kDirectElems) {
        // a large piece: what the ring holds goes first (order), then one copy straight from the caller's buffer;
        // the caller may reuse `samples` as soon as this returns, so that copy is waited for
        if ((rc = stream_flush_slot(st))) return rc;
        hipError_t e = hipMemcpyAsync(static_cast<char*>(st->hay.p) + st->sent * 4, samples, n * 4, hipMemcpyHostToDevice, st->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(st->copied, st->copy_stream);
        if (e != hipSuccess) { st->failed = true; return hip_fail(e, "stream ingest: copy"); }
        st->sent += n;
        st->len += n;
        rc = stream_launch_ready_pairs(st);
        AM_HIP(hipStreamSynchronize(st->copy_stream));
        return rc;
    }
    // a small piece: a host memcpy into the staging ring; full slots leave asynchronously
    const char* src = static_cast<const char*>(samples);
    size_t left = n;
    bool flushed = false;
    while (left) {
        const int b = st->cur;
        if (st->fill == 0) {
            if (!st->stage[b].p && (rc = st->stage[b].ensure(am_stream::kStageElems * 4))) { st->failed = true; return rc; }
            if (st->stage_busy[b]) {   // (the copy that last left this slot: two slots ago)
                AM_HIP(hipEventSynchronize(st->staged[b]));
                st->stage_busy[b] = false;
            }
        }
        const size_t take = std::min(left, am_stream::kStageElems - st->fill);
        memcpy(static_cast<char*>(st->stage[b].p) + st->fill * 4, src, take * 4);
        st->fill += take; st->len += take;
        src += take * 4; left -= take;
        if (st->fill == am_stream::kStageElems) {
            if ((rc = stream_flush_slot(st))) return rc;
            flushed = true;
        }
    }
    return flushed ? stream_launch_ready_pairs(st) : AM_OK;
}

int am_match_stream_finish(am_stream* st, am_peak* out, size_t cap, size_t* n_out) {
    if (!st || !st->h || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (st->failed) return fail(AM_ERR_INVALID_ARG, "stream is in a failed state: destroy it");
    am_needle* h = st->h;
    int rc = check_needle(h);
    if (rc) return rc;
    if (snapshot_opts(h).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *n_out = 0;
    const size_t len = st->len;
    rc = AM_OK;
    if (len) {
        if ((rc = stream_flush_slot(st))) return rc;          // what the staging ring still holds
        AM_HIP(hipStreamWaitEvent(c->stream, st->copied, 0));
        const void* src = st->hay.p;
        StreamPre pre{(float*)st->scores.p, &st->stats32, &st->side, st->pairs_done, st->geo.nblocks};
        bool use_pre = st->early && st->pairs_done > 0;
        if (use_pre) {
            // the layout the whole haystack gets must be the one the early pairs were computed in (the side
            // buffer keeps the offsets of the announced length: StreamPre::layout_nblocks), and so must the rule
            // by which raw scores are written: with another margin (dense_scores switched, or a prominence bound
            // that is no longer positive) the pick would read runs the early pairs never wrote
            Geometry fin{};
            const Opts o = snapshot_opts(h);
            if (len < h->n || plan_geometry(h->n, (long long)(len - h->n + 1), o, &fin) || fin.logN != st->geo.logN || fin.hop != st->geo.hop ||
                fin.nblocks > st->geo.nblocks || write_margin(o, &st->p) != st->margin)
                use_pre = false;
        }
        rc = match_many(h, &src, &len, 1, &st->p, out, cap, n_out, st->fmt, 0, 1, true, use_pre ? &pre : nullptr);
    }
    // ready for the next file of the same (announced) size; a stream that had to give up its early pairs (an
    // option changed under it) starts afresh
    st->len = 0; st->sent = 0; st->pairs_done = 0;
    if (!st->early && st->cap) (void)stream_layout(st);
    return rc;
}

void am_match_stream_destroy(am_stream* st) {
    if (!st) return;
    if (st->h && st->h->ctx) {
        std::lock_guard<std::recursive_mutex> lk(st->h->ctx->mu);
        (void)hipSetDevice(st->h->ctx->device);
        if (st->copy_stream) (void)hipStreamSynchronize(st->copy_stream);
        (void)hipStreamSynchronize(st->h->ctx->stream);
        st->hay.release(); st->scores.release(); st->stats32.release(); st->side.release();
    }
    if (st->copied) (void)hipEventDestroy(st->copied);
    for (int b = 0; b < 2; ++b) {
        if (st->staged[b]) (void)hipEventDestroy(st->staged[b]);
        st->stage[b].release();
    }
    if (st->copy_stream) (void)hipStreamDestroy(st->copy_stream);
    delete st;
}

}  // extern "C"
