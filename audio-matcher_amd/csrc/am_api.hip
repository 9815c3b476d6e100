// am_api.hip -- the C ABI of include/audiomatch.h that is a thin layer over the other host files: correlation, the
// single-device match entry points, find_peaks, the PCM and memory helpers and the measurement hook.  Contexts,
// needles, options and profiling are in am_context.hip, the engines in am_correlate.hip / am_engine.hip, streaming
// ingest in am_stream.hip, several devices in am_pool.hip.
//
// Host-side mirror of the reference's driver (paths relative to the reference):
//   calc_chunks            src/matcher/audio_matcher.rs:88-141
//   is_overshadowed        src/matcher/audio_matcher.rs:143-160
//   start_as_duration      src/matcher/mod.rs:127-129
//   Mode crop / centered   src/matcher/audio_matcher.rs:450-464
// All arithmetic on samples runs in the HIP kernels of am_fft.hip /
// am_peaks.hip; there is no CPU fallback.
#include "am_internal.h"

#include <climits>

using namespace am;


static size_t mode_len(size_t w, size_t s, int mode) {                // audio_matcher.rs:450-456
    if (mode == AM_MODE_FULL) return w + s - 1;
    if (mode == AM_MODE_SAME) return w;
    return (w > s ? w - s : 0) + 1;
}


// find_peaks on one host score array (am_find_peaks)
int am::find_peaks_host_array(Ctx* c, const float* d_scores, long long n, float min_prom, long long min_dist,
                              std::vector<am_peak>& all) {
    int rc;
    const PeakPolicy pol = snapshot_opts(nullptr).peak_policy();
    Segment sg; sg.a = 0; sg.b = n;
    PeakArena arena{};
    if ((rc = prepare_results(c, 1, AM_MAX_PEAKS_PER_CHUNK, &arena))) return rc;
    if ((rc = c->side[0].peaks.ensure(sizeof(am_peak) * AM_MAX_PEAKS_PER_CHUNK))) return rc;
    if ((rc = upload_segments(c, std::vector<Segment>(1, sg)))) return rc;
    if ((rc = launch_pick(c, c->side[0], d_scores, n, 0, 1, min_prom, min_dist, nullptr, nullptr, 0, arena, pol))) return rc;
    AM_HIP(hipStreamSynchronize(c->stream));
    const SegHeader hd = *static_cast<const SegHeader*>(c->hdr.p);
    all.clear();
    if (hd.overflow) return pick_chunk_big(c, d_scores, n, 0, sg, min_prom, min_dist, nullptr, hd.seg_min, all, pol);
    append_header_peaks(hd, arena, all);
    return AM_OK;
}

extern "C" {

int am_abi_version(void) { return AM_ABI_VERSION; }
const char* am_last_error_string(void) { return t_err.c_str(); }

int am_device_count(int* n) {
    if (!n) return fail(AM_ERR_INVALID_ARG, "null pointer");
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; return fail(AM_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *n = k;
    return AM_OK;
}

int am_correlate_len(size_t w, size_t s, int mode, size_t* out_len) {
    if (!out_len || w == 0 || s == 0 || mode < 0 || mode > 2) return fail(AM_ERR_INVALID_ARG, "bad argument");
    *out_len = mode_len(w, s, mode);
    return AM_OK;
}

static int correlate_impl(const am_needle* hc, const float* within, size_t w, int mode, int scale,
                          float* out, size_t cap, size_t* out_len, bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!within || !out_len || w == 0) return fail(AM_ERR_INVALID_ARG, "within must be non-empty");
    if (mode < AM_MODE_FULL || mode > AM_MODE_VALID) return fail(AM_ERR_INVALID_ARG, "bad mode");
    if (scale < AM_SCALE_NONE || scale > AM_SCALE_MY) return fail(AM_ERR_INVALID_ARG, "bad scale");
    if ((rc = norm_check(norm_spec(h, snapshot_opts(h)), scale))) return rc;
    const size_t s = h->n;
    const size_t len = mode_len(w, s, mode);
    *out_len = len;
    if (cap < len || !out) return fail(AM_ERR_CAPACITY, "output buffer too small");
    // centered(): start = (full - len) / 2 (audio_matcher.rs:460-464)
    const size_t start = (w + s - 1 - len) / 2;
    const long long lead = (long long)(s - 1) - (long long)start;
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_within = nullptr;
    if ((rc = resident_input(c, device_io, within, sample_bytes(w), &d_within))) return rc;
    const float* d_in = static_cast<const float*>(d_within);
    float* d_out = out;
    if (!device_io) {
        if ((rc = c->io_out.ensure(len * sizeof(float)))) return rc;
        d_out = (float*)c->io_out.p;
    }
    Opts o = snapshot_opts(h);
    const NormSpec nrm = norm_spec(h, o);
    const float factor = nrm.on ? norm_factor(nrm) : scale_factor(h, scale, w);
    if ((rc = run_correlation(h, o, d_in, (long long)w, lead, d_out, (long long)len, factor))) return rc;
    if (o.half) {
        // a half-precision transform can leave f16's range (see match_many): look at the result once and
        // compute it again in f32 if it holds a non-finite value (a bad input is dealt with below)
        const Segment whole{0, (long long)len};
        int flag = 0;
        if ((rc = nonfinite_flags(c, d_out, &whole, 1, &flag))) return rc;
        if (flag) {
            o.half = 0;
            if ((rc = run_correlation(h, o, d_in, (long long)w, lead, d_out, (long long)len, factor))) return rc;
        }
    }
    // score_norm: every output divided by its window's energy (the zero padding of Full / Same counts as zeros)
    if (nrm.on && (rc = normalise_scores(c, c->stream, nrm, d_in, (long long)w, 0, lead, (long long)s, d_out, 0, (long long)len))) return rc;
    // A NaN or an infinity in `within` makes every output of the reference's one transform per
    // window NaN (audio_matcher.rs:414-457); overlap-save confines it to the block pairs around
    // it.  Look at the window once and give the reference's answer.
    {
        const Segment whole{0, (long long)w};
        int flag = 0;
        if ((rc = nonfinite_flags(c, d_in, &whole, 1, &flag))) return rc;
        if (flag) AM_HIP(hipMemsetD32Async((hipDeviceptr_t)d_out, 0x7FC00000, len, c->stream));
    }
    AM_HIP(hipStreamSynchronize(c->stream));
    return device_io ? AM_OK : download(c, out, d_out, len * sizeof(float));
}

int am_correlate(const am_needle* h, const float* within, size_t w, int mode, int scale,
                 float* out, size_t cap, size_t* out_len) {
    return correlate_impl(h, within, w, mode, scale, out, cap, out_len, false);
}

int am_correlate_device(const am_needle* h, const float* d_within, size_t w, int mode, int scale,
                        float* d_out, size_t cap, size_t* out_len) {
    return correlate_impl(h, d_within, w, mode, scale, d_out, cap, out_len, true);
}

// am_match / am_match_pcm16 (src_kind 1: interleaved i16 stereo) and their _device forms
static int match_impl(const am_needle* hc, const void* haystack, size_t len, const am_match_params* p, am_peak* out, size_t cap,
                      size_t* n_out, int src_kind, bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!haystack || !p || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (len == 0) { *n_out = 0; return AM_OK; }
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = resident_input(c, device_io, haystack, sample_bytes(len), &d_in))) return rc;
    return match_many(h, &d_in, &len, 1, p, out, cap, n_out, src_kind);
}

int am_match_device(const am_needle* h, const float* d_haystack, size_t len,
                    const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    return match_impl(h, d_haystack, len, p, out, cap, n_out, 0, true);
}

int am_match(const am_needle* h, const float* haystack, size_t len,
             const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    return match_impl(h, haystack, len, p, out, cap, n_out, 0, false);
}

int am_match_batch_device(const am_needle* hc, const float* const* d_haystacks, const size_t* lens,
                          size_t n_hay, const am_match_params* p,
                          am_peak* out, size_t cap_per_hay, size_t* n_out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!d_haystacks || !lens || !p || !n_out || (!out && cap_per_hay)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    if (n_hay == 0) return AM_OK;
    return match_many(h, reinterpret_cast<const void* const*>(d_haystacks), lens, n_hay, p, out, cap_per_hay, n_out);
}

int am_match_multi_device(const am_needle* const* needles, size_t n_needles, const float* d_haystack, size_t len,
                          const am_match_params* p, am_peak* out, size_t cap_per_needle, size_t* n_out) {
    if (!needles || n_needles == 0 || !d_haystack || !p || !n_out || (!out && cap_per_needle))
        return fail(AM_ERR_INVALID_ARG, "null pointer");
    for (size_t k = 0; k < n_needles; ++k)
        if (!needles[k] || !needles[k]->ctx) return fail(AM_ERR_INVALID_ARG, "null needle handle");
    am_needle* h0 = const_cast<am_needle*>(needles[0]);
    int rc = check_needle(h0);
    if (rc) return rc;
    if (snapshot_opts(h0).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    std::lock_guard<std::recursive_mutex> lk(h0->ctx->mu);
    const void* src = d_haystack;
    return match_multi_many(const_cast<am_needle* const*>(needles), n_needles, &src, &len, 1, AM_FMT_F32_MONO, p, out, cap_per_needle, n_out);
}

int am_match_multi_batch_device(const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks,
                                const size_t* lens, size_t n_hay, int sample_format, const am_match_params* p,
                                am_peak* out, size_t cap_per_pair, size_t* n_out) {
    if (!needles || n_needles == 0 || !d_haystacks || !lens || !p || !n_out || (!out && cap_per_pair))
        return fail(AM_ERR_INVALID_ARG, "null pointer");
    int rc = check_format(sample_format);
    if (rc) return rc;
    for (size_t k = 0; k < n_needles; ++k)
        if (!needles[k] || !needles[k]->ctx) return fail(AM_ERR_INVALID_ARG, "null needle handle");
    am_needle* h0 = const_cast<am_needle*>(needles[0]);
    if ((rc = check_needle(h0))) return rc;
    if (n_hay == 0) return AM_OK;
    if (snapshot_opts(h0).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    std::lock_guard<std::recursive_mutex> lk(h0->ctx->mu);
    return match_multi_many(const_cast<am_needle* const*>(needles), n_needles, d_haystacks, lens, n_hay, sample_format, p,
                            out, cap_per_pair, n_out);
}

// ---- several needles of any lengths (match_multi_many with `varlen`) ----
static int check_multi_varlen(const am_needle* const* needles, size_t n_needles, int sample_format, const am_match_params* p, am_needle** h0) {
    if (!needles || n_needles == 0 || !p) return fail(AM_ERR_INVALID_ARG, "null pointer");
    int rc = check_format(sample_format);
    if (rc) return rc;
    for (size_t k = 0; k < n_needles; ++k)
        if (!needles[k] || !needles[k]->ctx) return fail(AM_ERR_INVALID_ARG, "null needle handle");
    for (size_t k = 1; k < n_needles; ++k)
        if (needles[k]->ctx != needles[0]->ctx) return fail(AM_ERR_INVALID_ARG, "needles must live on one device");
    *h0 = const_cast<am_needle*>(needles[0]);
    if ((rc = check_needle(*h0))) return rc;
    if (snapshot_opts(*h0).score_norm) return fail(AM_ERR_INVALID_ARG, AM_NORM_UNSUPPORTED);
    return AM_OK;
}

int am_match_multi_varlen_batch_device(const am_needle* const* needles, size_t n_needles, const uint64_t* overlaps,
                                       const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                                       int sample_format, const am_match_params* p,
                                       am_peak* out, size_t cap_per_pair, size_t* n_out) {
    if (!d_haystacks || !lens || !n_out || (!out && cap_per_pair)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    am_needle* h0 = nullptr;
    int rc = check_multi_varlen(needles, n_needles, sample_format, p, &h0);
    if (rc) return rc;
    if (n_hay == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(h0->ctx->mu);
    return match_multi_many(const_cast<am_needle* const*>(needles), n_needles, d_haystacks, lens, n_hay, sample_format, p,
                            out, cap_per_pair, n_out, 0, 1, overlaps, true);
}

int am_match_multi_varlen(const am_needle* const* needles, size_t n_needles, const uint64_t* overlaps,
                          const void* haystack, size_t len, int sample_format, const am_match_params* p,
                          am_peak* out, size_t cap_per_needle, size_t* n_out) {
    if (!haystack || !n_out || (!out && cap_per_needle)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    am_needle* h0 = nullptr;
    int rc = check_multi_varlen(needles, n_needles, sample_format, p, &h0);
    if (rc) return rc;
    if (len == 0) {
        for (size_t j = 0; j < n_needles; ++j) n_out[j] = 0;
        return AM_OK;
    }
    Ctx* c = h0->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, haystack, sample_bytes(len), &d_in))) return rc;
    return match_multi_many(const_cast<am_needle* const*>(needles), n_needles, &d_in, &len, 1, sample_format, p, out, cap_per_needle, n_out,
                            0, 1, overlaps, true);
}

// ---- the same three entry points on interleaved i16 stereo PCM: the down-mix of
// mp3_reader.rs:28-37 happens inside K1's loads, so the haystack is read once ----
int am_match_pcm16_device(const am_needle* h, const int16_t* d_interleaved, size_t frames,
                          const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    return match_impl(h, d_interleaved, frames, p, out, cap, n_out, 1, true);
}

int am_match_pcm16(const am_needle* h, const int16_t* interleaved, size_t frames,
                   const am_match_params* p, am_peak* out, size_t cap, size_t* n_out) {
    return match_impl(h, interleaved, frames, p, out, cap, n_out, 1, false);
}

int am_match_pcm16_batch_device(const am_needle* hc, const int16_t* const* d_interleaved, const size_t* frames,
                                size_t n_hay, const am_match_params* p,
                                am_peak* out, size_t cap_per_hay, size_t* n_out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!d_interleaved || !frames || !p || !n_out || (!out && cap_per_hay)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    if (n_hay == 0) return AM_OK;
    return match_many(h, reinterpret_cast<const void* const*>(d_interleaved), frames, n_hay, p, out, cap_per_hay, n_out, 1);
}


int am_find_peaks(int device, const float* scores, size_t n, float min_prominence,
                  uint64_t min_distance, am_peak* out, size_t cap, size_t* n_out) {
    if (!scores || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    *n_out = 0;
    if (n == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_scores = nullptr;
    if ((rc = upload_input(c, scores, sample_bytes(n), &d_scores))) return rc;
    std::vector<am_peak> all;
    if ((rc = find_peaks_host_array(c, (const float*)d_scores, (long long)n, min_prominence,
                                    (long long)min_distance, all))) return rc;
    return hand_back(all, out, cap, n_out, "peak output buffer too small");
}

// ---- the k best matches (am_best.hip) ----
static int best_check(const am_needle* h, int sample_format, const am_best_params* bp) {
    int rc = check_needle(h);
    if (rc) return rc;
    if (!bp) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format))) return rc;
    if (bp->k == 0) return fail(AM_ERR_INVALID_ARG, "k must be at least 1");
    if (bp->scale != AM_SCALE_NONE && bp->scale != AM_SCALE_LIB)
        return fail(AM_ERR_INVALID_ARG, "am_match_best: scale must be AM_SCALE_NONE or AM_SCALE_LIB (AM_SCALE_MY depends on a chunk)");
    return norm_check(norm_spec(h, snapshot_opts(h)), bp->scale);
}

static int match_best_impl(const am_needle* hc, const void* haystack, size_t len, int sample_format, const am_best_params* bp,
                           am_peak* out, size_t* n_out, bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = best_check(h, sample_format, bp);
    if (rc) return rc;
    if (!haystack || !out || !n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (!device_io) {   // (the host form answers a haystack shorter than the needle here, the _device form in match_best_one)
        *n_out = 0;
        if (len < h->n) return AM_OK;
    }
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_hay = nullptr;
    if ((rc = resident_input(c, device_io, haystack, sample_bytes(len), &d_hay))) return rc;
    return match_best_one(h, d_hay, len, sample_format, bp, out, n_out);
}

int am_match_best_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_best_params* bp, am_peak* out, size_t* n_out) {
    return match_best_impl(h, d_haystack, len, sample_format, bp, out, n_out, true);
}

int am_match_best(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_best_params* bp, am_peak* out, size_t* n_out) {
    return match_best_impl(h, haystack, len, sample_format, bp, out, n_out, false);
}

int am_match_best_batch_device(const am_needle* hc, const void* const* d_haystacks, const size_t* lens,
                               size_t n_hay, int sample_format, const am_best_params* bp,
                               am_peak* out, size_t* n_out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = best_check(h, sample_format, bp);
    if (rc) return rc;
    if (n_hay == 0) return AM_OK;
    if (!d_haystacks || !lens || !out || !n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    for (size_t i = 0; i < n_hay; ++i)
        if (!d_haystacks[i]) return fail(AM_ERR_INVALID_ARG, "haystack " + std::to_string(i) + ": null pointer");
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    // the score array and the down-mix sized once, for the longest haystack
    size_t longest = 0;
    for (size_t i = 0; i < n_hay; ++i) longest = std::max(longest, lens[i]);
    if (longest >= h->n) {
        if ((rc = c->best_scores.ensure(sizeof(float) * (longest - h->n + 1)))) return rc;
        if (sample_format == AM_FMT_S16_STEREO && (rc = c->best_mono.ensure(sizeof(float) * longest))) return rc;
    }
    for (size_t i = 0; i < n_hay; ++i)
        if ((rc = match_best_one(h, d_haystacks[i], lens[i], sample_format, bp, out + i * bp->k, n_out + i))) return rc;
    return AM_OK;
}

static int find_peaks_top_impl(int device, const float* scores, size_t n, float min_prominence, uint64_t min_distance,
                               size_t k, am_peak* out, size_t* n_out, bool device_io) {
    if (!scores || !out || !n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (k == 0) return fail(AM_ERR_INVALID_ARG, "k must be at least 1");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    *n_out = 0;
    if (n == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_scores = nullptr;
    if ((rc = resident_input(c, device_io, scores, sample_bytes(n), &d_scores))) return rc;
    std::vector<am_peak> res;
    if ((rc = best_select(c, (const float*)d_scores, (long long)n, min_prominence, (long long)std::min<uint64_t>(min_distance, (uint64_t)LLONG_MAX),
                          k, snapshot_opts(nullptr).peak_policy(), res))) return rc;
    for (size_t i = 0; i < res.size(); ++i) out[i] = res[i];
    *n_out = res.size();
    return AM_OK;
}

int am_find_peaks_top(int device, const float* scores, size_t n, float min_prominence,
                      uint64_t min_distance, size_t k, am_peak* out, size_t* n_out) {
    return find_peaks_top_impl(device, scores, n, min_prominence, min_distance, k, out, n_out, false);
}

int am_find_peaks_top_device(int device, const float* d_scores, size_t n, float min_prominence,
                             uint64_t min_distance, size_t k, am_peak* out, size_t* n_out) {
    return find_peaks_top_impl(device, d_scores, n, min_prominence, min_distance, k, out, n_out, true);
}

int am_pcm_s16_stereo_to_mono_device(int device, const int16_t* d_in, size_t frames, float* d_out) {
    if (!d_in || !d_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_pcm_downmix(c->stream, d_in, (long long)frames, d_out));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_pcm_s16_stereo_to_mono(int device, const int16_t* interleaved, size_t frames, float* out) {
    if (!interleaved || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, interleaved, sample_bytes(frames), &d_in)) || (rc = c->io_out.ensure(frames * sizeof(float)))) return rc;
    AM_HIP(launch_pcm_downmix(c->stream, (const int16_t*)d_in, (long long)frames, (float*)c->io_out.p));
    AM_HIP(hipStreamSynchronize(c->stream));
    return download(c, out, c->io_out.p, frames * sizeof(float));
}

int am_device_malloc(int device, size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(AM_ERR_INVALID_ARG, "bad argument");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    AM_HIP(hipMalloc(out, bytes));
    return AM_OK;
}
int am_device_free(int device, void* p) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (p) AM_HIP(hipFree(p));
    return AM_OK;
}
// Pinned host memory for the buffers a host hands to am_match / am_match_stream_push / am_pool_match_*: the
// copy engines read it directly (no bounce buffer in the runtime, no page faults), which is what lets N copier
// threads feed N devices side by side.  Portable: usable from every device's context.
int am_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(AM_ERR_INVALID_ARG, "bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(AM_ERR_NO_DEVICE, "no HIP device available");
    AM_HIP(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return AM_OK;
}
int am_host_free(void* p) {
    if (p) AM_HIP(hipHostFree(p));
    return AM_OK;
}
int am_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) return fail(AM_ERR_INVALID_ARG, "bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(AM_ERR_NO_DEVICE, "no HIP device available");
    AM_HIP(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return AM_OK;
}
int am_host_unregister(void* p) {
    if (!p) return fail(AM_ERR_INVALID_ARG, "null pointer");
    AM_HIP(hipHostUnregister(p));
    return AM_OK;
}

int am_memcpy_h2d(int device, void* d_dst, const void* src, size_t bytes) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    AM_HIP(copy_on_stream(c, d_dst, src, bytes, hipMemcpyHostToDevice));
    return AM_OK;
}
int am_memcpy_d2h(int device, void* dst, const void* d_src, size_t bytes) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    AM_HIP(copy_on_stream(c, dst, d_src, bytes, hipMemcpyDeviceToHost));
    return AM_OK;
}
int am_device_synchronize(int device) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    AM_HIP(hipDeviceSynchronize());
    return AM_OK;
}

int am_synth_uniform_device(int device, float* d_out, uint32_t seed, uint32_t stream,
                            uint64_t first, size_t n, float amp) {
    if (!d_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (n == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_synth(c->stream, d_out, seed, stream, first, (long long)n, amp));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_axpy_device(int device, float* d_dst, const float* d_src, size_t n, float gain) {
    if (!d_dst || !d_src) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (n == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_axpy(c->stream, d_dst, d_src, (long long)n, gain));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_synth_pcm16_stereo_device(int device, int16_t* d_out, uint32_t seed, uint32_t stream, uint64_t first, size_t frames, float amp) {
    if (!d_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_synth_pcm16(c->stream, d_out, seed, stream, first, (long long)frames, amp));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_add_pcm16_device(int device, int16_t* d_dst, const int16_t* d_src, size_t frames) {
    if (!d_dst || !d_src) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_add_pcm16(c->stream, d_dst, d_src, (long long)frames));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}


// Measurement hook (not part of the drop-in boundary): the column kernels K1 and K3 on `npairs` block pairs of
// synthetic input, `iters` launches each, average launch time in ms.  wide = 0: the production 2^22 plan
// (512 x 8192); wide = 1: 2^23 factored 512 x 16384 -- the same 512-row kernels on rows twice as long (no row kernel
// exists for that plan yet: this sizes what it would be worth).  dense: K3 writes every run / none.
int am_debug_column_bench(int device, int wide, int npairs, int iters, int dense, double* k1_ms, double* k3_ms) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (npairs < 1 || npairs > 64 || iters < 1 || !k1_ms || !k3_ms) return fail(AM_ERR_INVALID_ARG, "bad arguments");
    const Plan* pl = nullptr;
    if ((rc = wide ? get_plan(c, 23, &pl, 9) : get_plan(c, 22, &pl))) return rc;
    const long long N = 1ll << pl->dev.logN, s = 441000, hop = ((N - s + 1) / kTile) * kTile;
    const long long nblocks = 2ll * npairs, out_count = nblocks * hop, src_len = out_count + s - 1 + kTile;
    DevBuf src, work, scores, stats32, side;
    struct Release { DevBuf* b[5]; ~Release() { for (DevBuf* x : b) x->release(); } } release_all{{&src, &work, &scores, &stats32, &side}};
    if ((rc = src.ensure((size_t)src_len * 4)) || (rc = work.ensure((size_t)npairs * (size_t)N * sizeof(float2))) ||
        (rc = scores.ensure((size_t)out_count * 4)) || (rc = stats32.ensure((size_t)(out_count / 32) * sizeof(float2))) ||
        (rc = side.ensure(sparse_bytes(nblocks, pl->dev)))) return rc;
    AM_HIP(launch_synth(c->stream, (float*)src.p, 7, 1, 0, src_len, 0.25f));
    Job job{};
    job.src = src.p; job.src_len = src_len; job.lead = 0; job.src_kind = 0;
    job.dst = (float*)scores.p; job.out_count = out_count; job.hop = (int)hop; job.nblocks = (int)nblocks; job.first_pair = 0;
    ScanCfg scan{};
    fill_scan_cfg(&scan, stats32.p, side.p, nblocks, pl->dev, dense ? -1.0f : 1e30f, FLT_MAX, 60 * 44100, 70 * 44100 - s);
    hipEvent_t e[3];
    for (auto& x : e) AM_HIP(hipEventCreate(&x));
    double t1 = 0, t3 = 0;
    for (int it = -2; it < iters; ++it) {   // (two untimed rounds first)
        AM_HIP(hipEventRecord(e[0], c->stream));
        AM_HIP(launch_k1(c->stream, job, npairs, (float2*)work.p, pl->dev, 0));
        AM_HIP(hipEventRecord(e[1], c->stream));
        AM_HIP(launch_k3(c->stream, job, npairs, (const float2*)work.p, pl->dev, 1e-3f, scan, 0, false));
        AM_HIP(hipEventRecord(e[2], c->stream));
        AM_HIP(hipStreamSynchronize(c->stream));
        float a = 0, b = 0;
        AM_HIP(hipEventElapsedTime(&a, e[0], e[1]));
        AM_HIP(hipEventElapsedTime(&b, e[1], e[2]));
        if (it >= 0) { t1 += a; t3 += b; }
    }
    for (auto& x : e) (void)hipEventDestroy(x);
    *k1_ms = t1 / iters; *k3_ms = t3 / iters;
    return AM_OK;
}

}  // extern "C"
