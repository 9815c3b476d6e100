// am_monitor.hip -- live monitoring (am_monitor_*): final hits while the audio arrives, in bounded device memory.
//
// calc_chunks splits a recording into the windows of chunked(chunk + overlap, hop = chunk) (audio_matcher.rs:104),
// matches each and merges the union once (sort + filter_surrounding, audio_matcher.rs:132-160).  A monitor cuts the
// windows into fixed groups of G, matches a group through the part path (match_many with a PartSpec, what
// am_match_part_device runs) as soon as its last window's samples are there, and hands out the peaks whose fate
// under the merge can no longer change (merge_settle): what poll and end return for a needle, concatenated, is the
// merge of the groups' parts.  Samples before the first group not yet matched are dropped: the device buffer has a
// fixed size, two group spans plus a staging piece.
#include "am_internal.h"

struct am_monitor {
    struct Needle {
        am_needle* h = nullptr;
        am_match_params p{};
        am::Opts o{};            // the options read at begin (snapshot_opts, with this handle's overrides)
        uint64_t step = 0;       // samples between two groups: G * chunk
        uint64_t span = 0;       // samples of one group: (G - 1) * chunk + chunk + overlap
        uint64_t next = 0;       // first sample of the first group not yet matched: this needle's horizon
        std::vector<am_peak> pending;   // found, not yet final (sorted by start, window order on ties, after settle)
        am::MergeCursor cur;
    };
    std::vector<Needle> nd;
    am::Ctx* c = nullptr;
    int fmt = AM_FMT_F32_MONO;
    size_t G = 1;
    // The sample buffer: elements (f32 samples or i16 stereo frames, 4 bytes each) [base, base + cap) of the
    // recording; [base, sent) are on the device (or on their way, on the library's stream), [sent, received) sit in
    // the current staging slot.
    am::DevBuf buf;
    uint64_t cap = 0, base = 0, sent = 0, received = 0;
    // Two-slot staging ring in pinned host memory, as in am_stream: a push is a host memcpy into the current slot; a
    // full slot, or the samples that complete a group, go to the device as one asynchronous copy.
    static constexpr size_t kStageElems = (size_t)1 << 16;
    am::HostBuf stage[2];
    hipEvent_t staged[2] = {nullptr, nullptr};   // the slot's last copy has left it
    bool stage_busy[2] = {false, false};
    int cur = 0;
    size_t fill = 0;
    std::vector<std::pair<am_peak, uint32_t>> ready;   // final and kept, not yet returned: (peak, needle)
    bool ended = false, failed = false;
};

namespace am {

static int monitor_flush(am_monitor* m) {
    if (m->fill == 0) return AM_OK;
    const int b = m->cur;
    hipError_t e = hipMemcpyAsync(static_cast<char*>(m->buf.p) + (m->sent - m->base) * 4, m->stage[b].p, m->fill * 4,
                                  hipMemcpyHostToDevice, m->c->stream);
    if (e == hipSuccess) e = hipEventRecord(m->staged[b], m->c->stream);
    if (e != hipSuccess) { m->failed = true; return hip_fail(e, "monitor: copy"); }
    m->stage_busy[b] = true;
    m->sent += m->fill;
    m->fill = 0;
    m->cur = b ^ 1;
    return AM_OK;
}

// Drops the samples before the earliest horizon: [drop, sent) moves to the front of the buffer, a device-to-device copy
// on the library's stream (ordered behind the groups' kernels and the copies that brought the samples, and before
// the copies that follow).  Called with a full buffer only, where source and destination cannot overlap.
static int monitor_compact(am_monitor* m) {
    uint64_t drop = m->received;
    for (const am_monitor::Needle& n : m->nd) drop = std::min(drop, n.next);
    if (drop <= m->base) return AM_OK;
    const uint64_t keep = m->sent > drop ? m->sent - drop : 0;
    if (keep > drop - m->base) { m->failed = true; return fail(AM_ERR_HIP, "internal: monitor compaction would overlap"); }
    if (keep) {
        char* d = static_cast<char*>(m->buf.p);
        hipError_t e = hipMemcpyAsync(d, d + (drop - m->base) * 4, keep * 4, hipMemcpyDeviceToDevice, m->c->stream);
        if (e != hipSuccess) { m->failed = true; return hip_fail(e, "monitor: compaction"); }
    }
    m->base = drop;
    return AM_OK;
}

// The peaks of needle j that are final: merge_settle over the pending peaks that start before the needle's horizon
// (every later peak starts at or after it); the kept ones queue for poll.
static void monitor_settle(am_monitor* m, uint32_t j, bool ended) {
    am_monitor::Needle& n = m->nd[j];
    std::stable_sort(n.pending.begin(), n.pending.end(), [](const am_peak& x, const am_peak& y) { return x.start < y.start; });
    size_t known = n.pending.size();
    if (!ended) known = (size_t)(std::lower_bound(n.pending.begin(), n.pending.end(), n.next,
                                                  [](const am_peak& x, uint64_t t) { return x.start < t; }) - n.pending.begin());
    std::vector<am_peak> kept;
    const size_t k = merge_settle(&n.p, n.o.surrounding_from != 0, n.cur, n.pending.data(), known, n.next, ended, &kept);
    for (const am_peak& q : kept) m->ready.emplace_back(q, j);
    n.pending.erase(n.pending.begin(), n.pending.begin() + (std::ptrdiff_t)k);
}

// Group `next` of needle j as one part: its samples [next, min(received, next + span)) are on the device.
static int monitor_match_group(am_monitor* m, uint32_t j) {
    am_monitor::Needle& n = m->nd[j];
    const uint64_t first = n.next;
    size_t len = (size_t)(std::min(m->received, first + n.span) - first);
    const void* src = static_cast<const char*>(m->buf.p) + (first - m->base) * 4;
    std::vector<am_peak> raw;
    PartSpec part{m->G, first, (size_t)(first / n.p.chunk), 0, &raw};
    size_t cnt = 0;
    OptsPin pin(&n.o);
    const int rc = match_many(n.h, &src, &len, 1, &n.p, nullptr, 0, &cnt, m->fmt, 0, 1, false, nullptr, &part);
    if (rc) { m->failed = true; return rc; }
    n.pending.insert(n.pending.end(), raw.begin(), raw.end());
    n.next += n.step;
    return AM_OK;
}

// every group whose last window has arrived, needle by needle
static int monitor_run_ready(am_monitor* m) {
    int rc;
    for (uint32_t j = 0; j < (uint32_t)m->nd.size(); ++j) {
        am_monitor::Needle& n = m->nd[j];
        bool any = false;
        while (m->received >= n.next + n.span) {
            if ((rc = monitor_flush(m)) || (rc = monitor_match_group(m, j))) return rc;
            any = true;
        }
        if (any) monitor_settle(m, j, false);
    }
    return AM_OK;
}

// the earliest sample count at which some needle's next group is complete
static uint64_t monitor_next_threshold(const am_monitor* m) {
    uint64_t t = UINT64_MAX;
    for (const am_monitor::Needle& n : m->nd) t = std::min(t, n.next + n.span);
    return t;
}

// hands out the queued peaks by (start, needle), or nothing (AM_ERR_CAPACITY, *n_out = how many there are)
static int monitor_drain(am_monitor* m, am_peak* out, uint32_t* needle, size_t cap, size_t* n_out) {
    std::stable_sort(m->ready.begin(), m->ready.end(), [](const std::pair<am_peak, uint32_t>& x, const std::pair<am_peak, uint32_t>& y) {
        return x.first.start != y.first.start ? x.first.start < y.first.start : x.second < y.second;
    });
    *n_out = m->ready.size();
    if (m->ready.size() > cap) return fail(AM_ERR_CAPACITY, "out: buffer too small for the final peaks (nothing was returned)");
    for (size_t i = 0; i < m->ready.size(); ++i) {
        out[i] = m->ready[i].first;
        if (needle) needle[i] = m->ready[i].second;
    }
    m->ready.clear();
    return AM_OK;
}

static int monitor_enter(am_monitor* m) {
    if (m->failed) return fail(AM_ERR_INVALID_ARG, "monitor is in a failed state: destroy it");
    for (const am_monitor::Needle& n : m->nd) {
        const int rc = check_needle(n.h);
        if (rc) return rc;
    }
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" {

int am_monitor_begin(const am_needle* const* needles, size_t n_needles, const am_match_params* params, int sample_format,
                     size_t group_windows, am_monitor** out) {
    if (!out) return fail(AM_ERR_INVALID_ARG, "out: null pointer");
    *out = nullptr;
    if (!needles || n_needles == 0) return fail(AM_ERR_INVALID_ARG, "needles: need at least one needle handle");
    if (!params) return fail(AM_ERR_INVALID_ARG, "params: null pointer");
    if (sample_format != AM_FMT_F32_MONO && sample_format != AM_FMT_S16_STEREO)
        return fail(AM_ERR_INVALID_ARG, "sample_format: bad sample format");
    if (n_needles > UINT32_MAX) return fail(AM_ERR_INVALID_ARG, "n_needles: too many needles");
    const size_t G = group_windows ? group_windows : 1;
    if (G > ((size_t)1 << 18)) return fail(AM_ERR_INVALID_ARG, "group_windows: at most 2^18 windows per group");
    int rc;
    Ctx* c = nullptr;
    for (size_t j = 0; j < n_needles; ++j) {
        const std::string which = "needles[" + std::to_string(j) + "]: ";
        if (!needles[j]) return fail(AM_ERR_INVALID_ARG, which + "null handle");
        if ((rc = check_needle(needles[j]))) return rc;
        if (c && needles[j]->ctx != c) return fail(AM_ERR_INVALID_ARG, which + "all needles of a monitor must live on one device");
        c = needles[j]->ctx;
        const am_match_params& p = params[j];
        const std::string pw = "params[" + std::to_string(j) + "]: ";
        if (p.chunk == 0) return fail(AM_ERR_INVALID_ARG, pw + "chunk must be > 0");
        if (p.sr == 0) return fail(AM_ERR_INVALID_ARG, pw + "sr must be > 0");
        if (p.sr != params[0].sr) return fail(AM_ERR_INVALID_ARG, pw + "sr must be the same for every needle");
        if (p.scale < AM_SCALE_NONE || p.scale > AM_SCALE_MY) return fail(AM_ERR_INVALID_ARG, pw + "bad scale");
        if (snapshot_opts(needles[j]).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
        if (p.chunk > ((uint64_t)1 << 40) / G || p.overlap > ((uint64_t)1 << 40))
            return fail(AM_ERR_INVALID_ARG, pw + "chunk * group_windows + overlap is too large");
    }
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    am_monitor* m = new am_monitor();
    m->c = c; m->fmt = sample_format; m->G = G;
    m->nd.resize(n_needles);
    uint64_t max_span = 0;
    for (size_t j = 0; j < n_needles; ++j) {
        am_monitor::Needle& n = m->nd[j];
        n.h = const_cast<am_needle*>(needles[j]);
        n.p = params[j];
        n.o = snapshot_opts(n.h);
        n.step = (uint64_t)G * n.p.chunk;
        n.span = (uint64_t)(G - 1) * n.p.chunk + n.p.chunk + n.p.overlap;
        max_span = std::max(max_span, n.span);
    }
    // A group is matched as soon as it is complete, so the samples from the earliest horizon on are fewer than the
    // largest span; the buffer holds twice that and a staging piece, which keeps compaction a single forward copy.
    m->cap = 2 * max_span + am_monitor::kStageElems;
    hipError_t e = hipMalloc(&m->buf.p, m->cap * 4);
    if (e != hipSuccess) { m->buf.p = nullptr; am_monitor_destroy(m); return hip_fail(e, "hipMalloc(monitor samples)"); }
    m->buf.cap = m->cap * 4;
    for (int b = 0; b < 2; ++b) {
        if ((e = hipEventCreateWithFlags(&m->staged[b], hipEventDisableTiming)) != hipSuccess) {
            am_monitor_destroy(m);
            return hip_fail(e, "hipEventCreate(monitor)");
        }
    }
    *out = m;
    return AM_OK;
}

int am_monitor_push(am_monitor* m, const void* samples, size_t n) {
    if (!m) return fail(AM_ERR_INVALID_ARG, "m: null pointer");
    if (!samples && n) return fail(AM_ERR_INVALID_ARG, "samples: null pointer");
    int rc = monitor_enter(m);
    if (rc) return rc;
    if (m->ended) return fail(AM_ERR_INVALID_ARG, "m: the monitor has ended (am_monitor_end): no more samples");
    std::lock_guard<std::recursive_mutex> lk(m->c->mu);
    const char* src = static_cast<const char*>(samples);
    size_t left = n;
    while (left) {
        const int b = m->cur;
        if (m->fill == 0) {
            if (!m->stage[b].p && (rc = m->stage[b].ensure(am_monitor::kStageElems * 4))) { m->failed = true; return rc; }
            if (m->stage_busy[b]) {   // (the copy that last left this slot)
                AM_HIP(hipEventSynchronize(m->staged[b]));
                m->stage_busy[b] = false;
            }
        }
        if (m->received - m->base == m->cap && (rc = monitor_compact(m))) return rc;
        const uint64_t room = m->cap - (m->received - m->base);
        const uint64_t to_group = monitor_next_threshold(m) - m->received;
        const size_t take = (size_t)std::min<uint64_t>({(uint64_t)left, (uint64_t)(am_monitor::kStageElems - m->fill), room, to_group});
        if (take == 0) { m->failed = true; return fail(AM_ERR_HIP, "internal: monitor buffer full"); }
        memcpy(static_cast<char*>(m->stage[b].p) + m->fill * 4, src, take * 4);
        m->fill += take; m->received += take;
        src += take * 4; left -= take;
        if (m->fill == am_monitor::kStageElems && (rc = monitor_flush(m))) return rc;
        if (m->received == monitor_next_threshold(m) && (rc = monitor_run_ready(m))) return rc;
    }
    return AM_OK;
}

int am_monitor_poll(am_monitor* m, am_peak* out, uint32_t* needle, size_t cap, size_t* n_out) {
    if (!m) return fail(AM_ERR_INVALID_ARG, "m: null pointer");
    if (!n_out) return fail(AM_ERR_INVALID_ARG, "n_out: null pointer");
    if (!out && cap) return fail(AM_ERR_INVALID_ARG, "out: null pointer");
    *n_out = 0;
    std::lock_guard<std::recursive_mutex> lk(m->c->mu);
    return monitor_drain(m, out, needle, cap, n_out);
}

int am_monitor_end(am_monitor* m, am_peak* out, uint32_t* needle, size_t cap, size_t* n_out) {
    if (!m) return fail(AM_ERR_INVALID_ARG, "m: null pointer");
    if (!n_out) return fail(AM_ERR_INVALID_ARG, "n_out: null pointer");
    if (!out && cap) return fail(AM_ERR_INVALID_ARG, "out: null pointer");
    *n_out = 0;
    int rc = monitor_enter(m);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(m->c->mu);
    if (!m->ended) {
        // the groups that are not complete: those whose first window starts before the end (tail windows as
        // make_segments cuts them, option "tail_window")
        if ((rc = monitor_flush(m))) return rc;
        for (uint32_t j = 0; j < (uint32_t)m->nd.size(); ++j) {
            am_monitor::Needle& n = m->nd[j];
            while (n.next < m->received)
                if ((rc = monitor_match_group(m, j))) return rc;
            monitor_settle(m, j, true);
        }
        m->ended = true;
    }
    return monitor_drain(m, out, needle, cap, n_out);
}

int am_monitor_info_get(const am_monitor* m, am_monitor_info* info) {
    if (!m) return fail(AM_ERR_INVALID_ARG, "m: null pointer");
    if (!info) return fail(AM_ERR_INVALID_ARG, "info: null pointer");
    std::lock_guard<std::recursive_mutex> lk(m->c->mu);
    info->received = m->received;
    uint64_t horizon = UINT64_MAX, pending = 0;
    for (const am_monitor::Needle& n : m->nd) {
        horizon = std::min(horizon, n.next);
        pending += n.pending.size();
    }
    info->horizon = horizon;
    info->resident_bytes = m->buf.cap;
    info->pending = pending;
    return AM_OK;
}

void am_monitor_destroy(am_monitor* m) {
    if (!m) return;
    if (m->c) {
        std::lock_guard<std::recursive_mutex> lk(m->c->mu);
        (void)hipSetDevice(m->c->device);
        (void)hipStreamSynchronize(m->c->stream);
        m->buf.release();
    }
    for (int b = 0; b < 2; ++b) {
        if (m->staged[b]) (void)hipEventDestroy(m->staged[b]);
        m->stage[b].release();
    }
    delete m;
}

}  // extern "C"
