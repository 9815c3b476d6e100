// am_pool.hip -- several devices: the haystack batch sharded over a pool, and one long haystack split into parts.
#include <condition_variable>
#include <thread>

#include "am_internal.h"

using namespace am;

// ---------------------------------------------------------------------------
// The haystack batch over several devices (matcher/mod.rs:42-87 sharded).
struct am_pool {
    struct Slot {
        int device = -1;
        am_needle* needle = nullptr;           // needles[0]
        std::vector<am_needle*> needles;       // every needle of the pool, replicated on this device
        // two-slot HBM ring + copy stream of the host-buffer path
        void* ring[2] = {nullptr, nullptr};
        size_t ring_cap = 0;
        hipStream_t copy_stream = nullptr;
    };
    std::vector<Slot> slots;
    std::mutex mu;   // one batch at a time per pool
};

extern "C" {

// ---- pool ---------------------------------------------------------------------
int am_shard_plan(size_t n_items, size_t n_shards, size_t shard, size_t* first, size_t* stride, size_t* count) {
    if (!first || !stride || !count || n_shards == 0 || shard >= n_shards) return fail(AM_ERR_INVALID_ARG, "bad shard");
    *first = shard;
    *stride = n_shards;
    *count = n_items > shard ? (n_items - shard + n_shards - 1) / n_shards : 0;
    return AM_OK;
}

static int pool_create_common(const float* const* needles, size_t n_needles, size_t n, const int* devices, size_t n_dev, am_pool** out) {
    if (!needles || !out || n == 0 || n_needles == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    for (size_t j = 0; j < n_needles; ++j) if (!needles[j]) return fail(AM_ERR_INVALID_ARG, "null needle");
    std::vector<int> devs;
    if (devices) {
        if (n_dev == 0) return fail(AM_ERR_INVALID_ARG, "empty device list");
        devs.assign(devices, devices + n_dev);
    } else {
        int k = 0;
        if (hipGetDeviceCount(&k) != hipSuccess || k <= 0) return fail(AM_ERR_NO_DEVICE, "no HIP device available");
        for (int d = 0; d < k; ++d) devs.push_back(d);
    }
    am_pool* pool = new am_pool();
    pool->slots.resize(devs.size());
    for (size_t i = 0; i < devs.size(); ++i) {
        am_pool::Slot& sl = pool->slots[i];
        sl.device = devs[i];
        int rc = AM_OK;
        for (size_t j = 0; j < n_needles && rc == AM_OK; ++j) {
            am_needle* h = nullptr;
            rc = am_needle_create(devs[i], needles[j], n, &h);
            if (rc == AM_OK) sl.needles.push_back(h);
        }
        if (rc == AM_OK) sl.needle = sl.needles[0];
        if (rc == AM_OK && hipStreamCreateWithFlags(&sl.copy_stream, hipStreamNonBlocking) != hipSuccess)
            rc = fail(AM_ERR_HIP, "hipStreamCreate(pool copy stream)");
        if (rc) { const std::string keep = t_err; am_pool_destroy(pool); t_err = keep; return rc; }
    }
    *out = pool;
    return AM_OK;
}

int am_pool_create(const float* needle, size_t n, const int* devices, size_t n_dev, am_pool** out) {
    if (!needle) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    return pool_create_common(&needle, 1, n, devices, n_dev, out);
}

int am_pool_create_multi(const float* const* needles, size_t n_needles, size_t n, const int* devices, size_t n_dev, am_pool** out) {
    return pool_create_common(needles, n_needles, n, devices, n_dev, out);
}

void am_pool_destroy(am_pool* pool) {
    if (!pool) return;
    for (am_pool::Slot& sl : pool->slots) {
        if (sl.device >= 0) (void)hipSetDevice(sl.device);
        if (sl.copy_stream) { (void)hipStreamSynchronize(sl.copy_stream); (void)hipStreamDestroy(sl.copy_stream); }
        for (void* r : sl.ring) if (r) (void)hipFree(r);
        for (am_needle* h : sl.needles) am_needle_destroy(h);
    }
    delete pool;
}

int am_pool_size(const am_pool* pool, size_t* n_dev) {
    if (!pool || !n_dev) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n_dev = pool->slots.size();
    return AM_OK;
}

int am_pool_slot(const am_pool* pool, size_t slot, int* device, const am_needle** needle) {
    if (!pool || slot >= pool->slots.size()) return fail(AM_ERR_INVALID_ARG, "bad pool slot");
    if (device) *device = pool->slots[slot].device;
    if (needle) *needle = pool->slots[slot].needle;
    return AM_OK;
}

namespace {

// What a pool call runs per haystack: one needle (match_many; out holds cap slots per haystack) or
// every needle of the pool (match_multi_many; cap slots per (haystack, needle) pair, slot k * nn + j).
struct PoolJob {
    bool multi;
    int fmt;   // AM_FMT_*: one f32 mono sample and one i16 stereo frame are both 4 bytes
};

// A resident haystack must live on the device of the slot that matches it (haystack k on slot k mod n_dev):
// the kernels of that device would otherwise read it over xGMI, or fault.  Ask the runtime instead of
// trusting the caller.
int check_resident(const void* ptr, int device, size_t index) {
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, ptr);
    char buf[200];
    if (e != hipSuccess) {
        (void)hipGetLastError();
        snprintf(buf, sizeof(buf), "haystack %zu: not a device pointer the runtime knows (%s)", index, hipGetErrorString(e));
        return fail(AM_ERR_INVALID_ARG, buf);
    }
    if (attr.type == hipMemoryTypeManaged) return AM_OK;
    if (attr.type != hipMemoryTypeDevice) {
        snprintf(buf, sizeof(buf), "haystack %zu: host memory passed to a _device entry point", index);
        return fail(AM_ERR_INVALID_ARG, buf);
    }
    if (attr.device != device) {
        snprintf(buf, sizeof(buf), "haystack %zu lives on device %d but its pool slot runs on device %d (haystack k belongs on slot k mod n_dev)",
                 index, attr.device, device);
        return fail(AM_ERR_INVALID_ARG, buf);
    }
    return AM_OK;
}

int slot_match(am_pool::Slot& sl, const PoolJob& job, const void* const* ptrs, const size_t* ln, size_t count,
               const am_match_params* p, am_peak* out, size_t cap, size_t* n_out, size_t first, size_t stride) {
    am_needle* h = sl.needle;
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    if (job.multi)
        return match_multi_many(sl.needles.data(), sl.needles.size(), ptrs, ln, count, job.fmt, p, out, cap, n_out, first, stride);
    return match_many(h, ptrs, ln, count, p, out, cap, n_out, job.fmt, first, stride);
}

// The two-slot HBM ring of the host-buffer paths, at least `bytes` per slot.
int ensure_ring(am_pool::Slot& sl, size_t bytes) {
    if (bytes <= sl.ring_cap) return AM_OK;
    for (void*& r : sl.ring) { if (r) (void)hipFree(r); r = nullptr; }
    sl.ring_cap = 0;
    for (void*& r : sl.ring) {
        const hipError_t e = hipMalloc(&r, bytes);
        if (e != hipSuccess) { r = nullptr; return hip_fail(e, "hipMalloc(pool ring)"); }
    }
    sl.ring_cap = bytes;
    return AM_OK;
}

// resident haystacks: the slot's shard (items first + i * stride, i < count) goes through the matcher as one batch
int slot_run_device(am_pool::Slot& sl, const PoolJob& job, size_t first, size_t stride, size_t count, const void* const* d_hays,
                    const size_t* lens, const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    std::vector<const void*> ptrs(count);
    std::vector<size_t> ln(count);
    for (size_t i = 0; i < count; ++i) { ptrs[i] = d_hays[first + i * stride]; ln[i] = lens[first + i * stride]; }
    int rc = check_needle(sl.needle);
    if (rc) return rc;
    for (size_t i = 0; i < count; ++i)
        if (ptrs[i] && ln[i] && (rc = check_resident(ptrs[i], sl.device, first + i * stride))) return rc;
    return slot_match(sl, job, ptrs.data(), ln.data(), count, p, out, cap, n_out, first, stride);
}

// host haystacks: a copier thread fills the two-slot ring one haystack ahead of the matcher
int slot_run_host(am_pool::Slot& sl, const PoolJob& job, size_t first, size_t stride, size_t count, const void* const* hays,
                  const size_t* lens, const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    am_needle* h = sl.needle;
    int rc = check_needle(h);   // hipSetDevice for this thread
    if (rc) return rc;
    size_t max_len = 0;
    for (size_t i = 0; i < count; ++i) if (hays[first + i * stride]) max_len = std::max(max_len, lens[first + i * stride]);
    if ((rc = ensure_ring(sl, max_len * 4))) return rc;
    std::mutex m;
    std::condition_variable cv;
    bool ready[2] = {false, false};
    hipError_t copy_err = hipSuccess;
    bool stop = false;
    std::thread copier([&] {
        (void)hipSetDevice(sl.device);
        for (size_t i = 0; i < count; ++i) {
            const int b = (int)(i & 1);
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return !ready[b] || stop; });
                if (stop) return;
            }
            const size_t k = first + i * stride;
            hipError_t e = hipSuccess;
            if (hays[k] && lens[k]) {
                e = hipMemcpyAsync(sl.ring[b], hays[k], lens[k] * 4, hipMemcpyHostToDevice, sl.copy_stream);
                if (e == hipSuccess) e = hipStreamSynchronize(sl.copy_stream);
            }
            std::lock_guard<std::mutex> lk(m);
            if (e != hipSuccess) { copy_err = e; stop = true; cv.notify_all(); return; }
            ready[b] = true;
            cv.notify_all();
        }
    });
    int worst = AM_OK;
    for (size_t i = 0; i < count; ++i) {
        const int b = (int)(i & 1);
        {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return ready[b] || stop; });
            if (stop) break;
        }
        const size_t k = first + i * stride;
        const void* src = (hays[k] && lens[k]) ? sl.ring[b] : nullptr;
        rc = slot_match(sl, job, &src, &lens[k], 1, p, out, cap, n_out, k, 1);
        {
            std::lock_guard<std::mutex> lk(m);
            ready[b] = false;
            if (rc != AM_OK && rc != AM_ERR_CAPACITY) stop = true;
            cv.notify_all();
        }
        if (rc == AM_ERR_CAPACITY) worst = rc;
        else if (rc) { worst = rc; break; }
    }
    copier.join();
    if (copy_err != hipSuccess) return hip_fail(copy_err, "host-to-device copy (pool)");
    return worst;
}

int pool_run(am_pool* pool, const PoolJob& job, const void* const* hays, const size_t* lens, size_t n_hay, const am_match_params* p,
             am_peak* out, size_t cap, size_t* n_out, bool host) {
    if (!pool || !hays || !lens || !p || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_format(job.fmt)) return rc;
    if (job.multi && snapshot_opts(nullptr).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    std::lock_guard<std::mutex> lk(pool->mu);
    const size_t nslots = pool->slots.size();
    const size_t nn = pool->slots.empty() ? 0 : pool->slots[0].needles.size();
    if (!job.multi && nn != 1)
        return fail(AM_ERR_INVALID_ARG, "this pool holds several needles: use am_pool_match_multi_batch*");
    for (size_t k = 0; k < n_hay * (job.multi ? nn : 1); ++k) n_out[k] = 0;
    if (n_hay == 0) return AM_OK;
    std::vector<int> rcs(nslots, AM_OK);
    std::vector<std::string> errs(nslots);
    std::vector<std::thread> threads;
    for (size_t s = 0; s < nslots; ++s)
        threads.emplace_back([&, s] {
            size_t first, stride, count;
            am_shard_plan(n_hay, nslots, s, &first, &stride, &count);
            if (count == 0) return;
            rcs[s] = host ? slot_run_host(pool->slots[s], job, first, stride, count, hays, lens, p, out, cap, n_out)
                          : slot_run_device(pool->slots[s], job, first, stride, count, hays, lens, p, out, cap, n_out);
            if (rcs[s]) errs[s] = t_err;   // the error string is thread-local: hand it to the caller's thread
        });
    for (std::thread& th : threads) th.join();
    int worst = AM_OK;
    for (size_t s = 0; s < nslots; ++s) {
        if (rcs[s] == AM_OK) continue;
        if (worst == AM_OK || worst == AM_ERR_CAPACITY) { worst = rcs[s]; t_err = errs[s]; }
    }
    return worst;
}

}  // namespace

int am_pool_match_batch(am_pool* pool, const float* const* haystacks, const size_t* lens, size_t n_hay,
                        const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out) {
    return pool_run(pool, PoolJob{false, AM_FMT_F32_MONO}, reinterpret_cast<const void* const*>(haystacks), lens, n_hay, p, out, cap_per_hay, n_out, true);
}

int am_pool_match_batch_device(am_pool* pool, const float* const* d_haystacks, const size_t* lens, size_t n_hay,
                               const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out) {
    return pool_run(pool, PoolJob{false, AM_FMT_F32_MONO}, reinterpret_cast<const void* const*>(d_haystacks), lens, n_hay, p, out, cap_per_hay, n_out, false);
}

int am_pool_match_batch_pcm16(am_pool* pool, const int16_t* const* interleaved, const size_t* frames, size_t n_hay,
                              const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out) {
    return pool_run(pool, PoolJob{false, AM_FMT_S16_STEREO}, reinterpret_cast<const void* const*>(interleaved), frames, n_hay, p, out, cap_per_hay, n_out, true);
}

int am_pool_match_batch_pcm16_device(am_pool* pool, const int16_t* const* d_interleaved, const size_t* frames, size_t n_hay,
                                     const am_match_params* p, am_peak* out, size_t cap_per_hay, size_t* n_out) {
    return pool_run(pool, PoolJob{false, AM_FMT_S16_STEREO}, reinterpret_cast<const void* const*>(d_interleaved), frames, n_hay, p, out, cap_per_hay, n_out, false);
}

int am_pool_match_multi_batch(am_pool* pool, const void* const* haystacks, const size_t* lens, size_t n_hay, int sample_format,
                              const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out) {
    return pool_run(pool, PoolJob{true, sample_format}, haystacks, lens, n_hay, p, out, cap_per_pair, n_out, true);
}

int am_pool_match_multi_batch_device(am_pool* pool, const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                     const am_match_params* p, am_peak* out, size_t cap_per_pair, size_t* n_out) {
    return pool_run(pool, PoolJob{true, sample_format}, d_haystacks, lens, n_hay, p, out, cap_per_pair, n_out, false);
}

// ---- one long haystack over several devices ---------------------------------------------
// calc_chunks fans the windows of ONE haystack out over its workers (audio_matcher.rs:104-131) and sorts and
// filters the union afterwards (:132-140).  The same split here: contiguous window ranges per part, each part's
// buffer reaching to the end of its last window (the overlap tail = the S - 1 halo of SURVEY.md 8e and more),
// the windows of a part matched as one haystack of their own, ONE merge over all parts.
int am_long_plan(size_t len, size_t needle_len, const am_match_params* p, size_t n_parts, size_t part,
                 size_t* first_window, size_t* n_windows, size_t* first_sample, size_t* n_samples) {
    if (!p || !first_window || !n_windows || !first_sample || !n_samples || n_parts == 0 || part >= n_parts || needle_len == 0)
        return fail(AM_ERR_INVALID_ARG, "bad part");
    if (p->chunk == 0) return fail(AM_ERR_INVALID_ARG, "chunk must be > 0");
    // windows that yield scores: i * chunk < len and min(chunk + overlap, len - i * chunk) >= needle_len (make_segments)
    const unsigned long long window = p->chunk + p->overlap;
    size_t nv = 0;
    if (snapshot_opts(nullptr).tail_window) {   // option "tail_window" = 1: full-length windows only
        if (len >= window && window >= needle_len) nv = (size_t)((len - window) / p->chunk) + 1;
    } else if (len >= needle_len && window >= needle_len) {
        // the last offset whose window is long enough: off <= len - needle_len
        nv = (size_t)((len - needle_len) / p->chunk) + 1;
    }
    const size_t w0 = nv * part / n_parts, w1 = nv * (part + 1) / n_parts;
    *first_window = w0;
    *n_windows = w1 - w0;
    *first_sample = w0 * (size_t)p->chunk;
    *n_samples = 0;
    if (w1 > w0) {
        const unsigned long long end = std::min<unsigned long long>(len, (unsigned long long)(w1 - 1) * p->chunk + window);
        *n_samples = (size_t)(end - (unsigned long long)*first_sample);
    }
    return AM_OK;
}

int am_match_part_device(const am_needle* hc, const void* d_part, size_t n_samples, int sample_format, const am_match_params* p,
                         size_t n_windows, uint64_t first_sample, am_peak* out, size_t cap, size_t* n_out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!p || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format))) return rc;
    if (snapshot_opts(h).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    *n_out = 0;
    if (n_windows == 0 || n_samples == 0) return AM_OK;
    if (!d_part) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    std::vector<am_peak> raw;
    PartSpec part{n_windows, first_sample, 0, n_windows, &raw};
    size_t n = 0;
    if ((rc = match_many(h, &d_part, &n_samples, 1, p, nullptr, 0, &n, sample_format, 0, 1, true, nullptr, &part))) return rc;
    return hand_back(raw, out, cap, n_out, "peak output buffer too small");
}

int am_merge_peaks(const am_match_params* p, const am_peak* peaks, size_t n, am_peak* out, size_t cap, size_t* n_out) {
    if (!p || !n_out || (!peaks && n) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::vector<am_peak> all(peaks, peaks + n);
    return merge_peaks(all, p, snapshot_opts(nullptr).surrounding_from != 0, out, cap, n_out);
}

namespace {

int pool_long(am_pool* pool, const void* host_hay, const void* const* d_parts, size_t len, int fmt, const am_match_params* p,
              am_peak* out, size_t cap, size_t* n_out) {
    if (!pool || !p || !n_out || (!out && cap) || (!host_hay && !d_parts)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_format(fmt)) return rc;
    std::lock_guard<std::mutex> lk(pool->mu);
    *n_out = 0;
    const size_t nslots = pool->slots.size();
    if (nslots == 0) return fail(AM_ERR_INVALID_ARG, "empty pool");
    if (pool->slots[0].needles.size() != 1)
        return fail(AM_ERR_INVALID_ARG, "this pool holds several needles: am_pool_match_long takes a single-needle pool");
    if (len == 0) return AM_OK;
    const size_t s = pool->slots[0].needle->n;
    struct Part { size_t w0, nw, a, n; };
    std::vector<Part> parts(nslots);
    size_t total_windows = 0;
    for (size_t i = 0; i < nslots; ++i) {
        int rc = am_long_plan(len, s, p, nslots, i, &parts[i].w0, &parts[i].nw, &parts[i].a, &parts[i].n);
        if (rc) return rc;
        total_windows += parts[i].nw;
    }
    const Hooks hooks = snapshot_hooks();
    if (hooks.fn) hooks.fn(hooks.user, 0, 0, total_windows);
    std::vector<std::vector<am_peak>> raw(nslots);
    std::vector<int> rcs(nslots, AM_OK);
    std::vector<std::string> errs(nslots);
    std::vector<std::thread> threads;
    for (size_t i = 0; i < nslots; ++i)
        threads.emplace_back([&, i] {
            const Part& pt = parts[i];
            if (pt.nw == 0) return;
            am_pool::Slot& sl = pool->slots[i];
            int rc = check_needle(sl.needle);   // hipSetDevice for this thread
            const void* src = nullptr;
            if (rc == AM_OK && d_parts) {
                src = d_parts[i];
                if (!src) rc = fail(AM_ERR_INVALID_ARG, "null part pointer");
                else rc = check_resident(src, sl.device, i);
            } else if (rc == AM_OK) {
                rc = ensure_ring(sl, pt.n * 4);   // (the ring of the host-buffer batch path: its first slot holds the part)
                if (rc == AM_OK) {
                    hipError_t e = hipMemcpyAsync(sl.ring[0], static_cast<const char*>(host_hay) + 4 * pt.a, pt.n * 4, hipMemcpyHostToDevice,
                                                  sl.copy_stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(sl.copy_stream);
                    if (e != hipSuccess) rc = hip_fail(e, "host-to-device copy (long haystack)");
                    src = sl.ring[0];
                }
            }
            if (rc == AM_OK) {
                am_needle* h = sl.needle;
                std::lock_guard<std::recursive_mutex> lk2(h->ctx->mu);
                PartSpec spec{pt.nw, (uint64_t)pt.a, pt.w0, total_windows, &raw[i]};
                size_t n = 0;
                rc = match_many(h, &src, &pt.n, 1, p, nullptr, 0, &n, fmt, 0, 1, true, nullptr, &spec);
            }
            rcs[i] = rc;
            if (rc) errs[i] = t_err;
        });
    for (std::thread& th : threads) th.join();
    for (size_t i = 0; i < nslots; ++i)
        if (rcs[i]) { t_err = errs[i]; return rcs[i]; }
    // flatten in window order, then ONE sort + overshadow pass over the union (audio_matcher.rs:132-140): a peak
    // next to a cut sees its neighbour from the other part, exactly as in a single call
    std::vector<am_peak> all;
    for (size_t i = 0; i < nslots; ++i) all.insert(all.end(), raw[i].begin(), raw[i].end());
    const int rc = merge_peaks(all, p, snapshot_opts(nullptr).surrounding_from != 0, out, cap, n_out);
    if (hooks.fn) hooks.fn(hooks.user, 0, 1, total_windows);
    return rc;
}

}  // namespace

int am_pool_match_long(am_pool* pool, const void* haystack, size_t len, int sample_format, const am_match_params* p,
                       am_peak* out, size_t cap, size_t* n_out) {
    if (!haystack && len) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (snapshot_opts(nullptr).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    return pool_long(pool, haystack, nullptr, len, sample_format, p, out, cap, n_out);
}

int am_pool_match_long_device(am_pool* pool, const void* const* d_parts, size_t len, int sample_format, const am_match_params* p,
                              am_peak* out, size_t cap, size_t* n_out) {
    if (!d_parts) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (snapshot_opts(nullptr).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    return pool_long(pool, nullptr, d_parts, len, sample_format, p, out, cap, n_out);
}

int am_pool_needle_count(const am_pool* pool, size_t* n_needles) {
    if (!pool || !n_needles) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n_needles = pool->slots.empty() ? 0 : pool->slots[0].needles.size();
    return AM_OK;
}

}  // extern "C"
