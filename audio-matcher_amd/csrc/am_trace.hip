// am_trace.hip -- score traces (am_trace_*, am_match_trace*; include/audiomatch.h, "score traces"): per bin of D
// scores the largest and the smallest score with their places, the count of scores that are not NaN and their f64
// sum and sum of squares.  One read of the score array, no atomics, one fixed order of additions.
//
// Every span of scores (a whole bin in the wave form, one slice of AM_TRACE_SLICE scores of a bin in the sliced form)
// is reduced by ONE wavefront (trace_span):
//   * the score at offset j of the span belongs to class k = j mod 256; a class adds its scores in ascending j, into
//     an accumulator that starts at +0.0 (a NaN score adds +0.0: an accumulator is never -0.0, so that changes no bit);
//   * the wave reads steps of 256 scores from the 16-byte boundary at or below the span's start: lane l holds the four
//     consecutive scores at floats 4l .. 4l + 3 of the step, one 16-byte load where all four lie inside the span and
//     guarded 4-byte loads at the ragged head and tail.  With a = (address of the span's start / 4) mod 4 the lane's
//     four accumulators are the classes (4l + i - a) mod 256 in every step: the alignment decides which lane holds a
//     class, never what a class adds or in which order;
//   * at the end the accumulators rotate by a places across the lanes (two cross-lane reads per accumulator, no LDS
//     memory), so that lane l holds the classes 4l .. 4l + 3; it adds them as (c0 + c1) + (c2 + c3), and the lanes add by
//     the butterfly over lane ^ 32, 16, 8, 4, 2, 1.  max / min: the larger (smaller) score, ties to the lower offset.
// Sliced form: trace_slices writes one partial per slice (the record's own layout, offsets already in the bin),
// trace_finish folds a bin's partials in ascending slice order, one wave per bin.  Which form runs is decided by D
// alone (D <= AM_TRACE_WAVE_BIN_MAX: the wave form), or by the debug option "trace_form".
#include "am_internal.h"
#include "am_wave_steps.h"

#include <climits>

namespace am {

namespace {

constexpr int kTraceThreads = 256;            // four waves, four spans at a time
constexpr int kTraceBlocks = 2048;            // blocks of the capped grid (8 per CU); the rest is strided
constexpr unsigned kTraceNone = 0xFFFFFFFFu;  // "no score yet" in a running (value, offset) pair
static_assert(sizeof(am_trace_bin) == 40, "am_trace_bin is 40 bytes, no padding");
static_assert(AM_TRACE_SLICE % 256 == 0, "a slice is whole steps from its start");

// (vb at ob) into the running maximum (v at o): the larger score, ties (==, so -0.0 and +0.0 tie) to the lower offset
__device__ __forceinline__ void take_max(float& v, unsigned& o, float vb, unsigned ob) {
    if (ob != kTraceNone && (o == kTraceNone || vb > v || (vb == v && ob < o))) { v = vb; o = ob; }
}
__device__ __forceinline__ void take_min(float& v, unsigned& o, float vb, unsigned ob) {
    if (ob != kTraceNone && (o == kTraceNone || vb < v || (vb == v && ob < o))) { v = vb; o = ob; }
}

// One wavefront reduces the span p[0, len) (len >= 0; p at any 4-byte alignment); offsets are reported from off0 on.
// Every lane of the wave must be here.  The record is complete in every lane.
__device__ __forceinline__ am_trace_bin trace_span(const float* __restrict__ p, int len, unsigned off0) {
    const int lane = threadIdx.x & 63;
    const int a = wave_align(p);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.0f, mn = 0.0f;
    unsigned omx = kTraceNone, omn = kTraceNone, cnt = 0u;
    // the lane's four floats of a step into its accumulators, in ascending offset; the order in which a class adds its
    // scores is the order of the steps (wave_steps, am_wave_steps.h)
    wave_steps(p, len, [&](int f0, const float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = v[i];
            const bool ok = x == x;              // (a float outside the span reads as NaN)
            const double d = ok ? (double)x : 0.0;
            s[i] += d;
            q[i] += d * d;
            if (ok) {
                const unsigned o = off0 + (unsigned)(f0 + i - a);
                ++cnt;
                if (omx == kTraceNone || x > mx) { mx = x; omx = o; }   // (ascending offsets: the first of equals stays)
                if (omn == kTraceNone || x < mn) { mn = x; omn = o; }
            }
        }
    });
    // the rotation: lane l, place i takes class 4l + i, which sits a places further on
    if (a) {
        double rs[4], rq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = (i + a) & 3, src = (lane + ((i + a) >> 2)) & 63;
            const double ms = c == 0 ? s[0] : c == 1 ? s[1] : c == 2 ? s[2] : s[3];
            const double mq = c == 0 ? q[0] : c == 1 ? q[1] : c == 2 ? q[2] : q[3];
            rs[i] = __shfl(ms, src, 64);
            rq[i] = __shfl(mq, src, 64);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { s[i] = rs[i]; q[i] = rq[i]; }
    }
    double sum = (s[0] + s[1]) + (s[2] + s[3]), sq = (q[0] + q[1]) + (q[2] + q[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        sq += __shfl_xor(sq, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
        const float bx = __shfl_xor(mx, o, 64), bn = __shfl_xor(mn, o, 64);
        const unsigned box = __shfl_xor(omx, o, 64), bon = __shfl_xor(omn, o, 64);
        take_max(mx, omx, bx, box);
        take_min(mn, omn, bn, bon);
    }
    am_trace_bin r;
    r.max = cnt ? mx : __uint_as_float(0x7FC00000u);
    r.min = cnt ? mn : __uint_as_float(0x7FC00000u);
    r.argmax = cnt ? omx : 0u;
    r.argmin = cnt ? omn : 0u;
    r.count = cnt;
    r.reserved = 0u;
    r.sum = sum;
    r.sumsq = sq;
    return r;
}

// Small bins: one wave per bin, four bins per workgroup at a time, the grid strided over the bins.
__global__ void __launch_bounds__(kTraceThreads) trace_bins(const float* __restrict__ g, long long n, long long D, long long nb,
                                                            am_trace_bin* __restrict__ out) {
    const long long wave = ((long long)blockIdx.x * kTraceThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kTraceThreads) >> 6;
    for (long long b = wave; b < nb; b += nwaves) {
        const long long lo = b * D, len = std::min(D, n - lo);
        const am_trace_bin r = trace_span(g + lo, (int)len, 0u);
        if ((threadIdx.x & 63) == 0) out[b] = r;
    }
}

// Large bins: slice sl of bin b is the bin's scores [sl AM_TRACE_SLICE, (sl + 1) AM_TRACE_SLICE), one wave per slice; the
// partial of a slice behind the end of a ragged last bin is empty.
__global__ void __launch_bounds__(kTraceThreads) trace_slices(const float* __restrict__ g, long long n, long long D, long long nb,
                                                              long long per_bin, am_trace_bin* __restrict__ parts) {
    const long long wave = ((long long)blockIdx.x * kTraceThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kTraceThreads) >> 6;
    for (long long u = wave; u < nb * per_bin; u += nwaves) {
        const long long b = u / per_bin, sl = u - b * per_bin;
        const long long lo = b * D + sl * AM_TRACE_SLICE, hi = std::min(n, std::min(b * D + D, lo + AM_TRACE_SLICE));
        const am_trace_bin r = trace_span(g + std::min(lo, n), (int)std::max(0ll, hi - lo), (unsigned)(sl * AM_TRACE_SLICE));
        if ((threadIdx.x & 63) == 0) parts[u] = r;
    }
}

// ... and one wave per bin folds its partials in ascending slice order: 64 partials are loaded at a time, one per lane,
// and every lane folds them in lane order (the loads of a round are in flight together; the fold itself is serial, as
// the order of the additions says).
__global__ void __launch_bounds__(kTraceThreads) trace_finish(const am_trace_bin* __restrict__ parts, long long nb, long long per_bin,
                                                              am_trace_bin* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kTraceThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kTraceThreads) >> 6;
    for (long long b = wave; b < nb; b += nwaves) {
        const am_trace_bin* p = parts + b * per_bin;
        float mx = 0.0f, mn = 0.0f;
        unsigned omx = kTraceNone, omn = kTraceNone, cnt = 0u;
        double sum = 0.0, sq = 0.0;
        for (long long s0 = 0; s0 < per_bin; s0 += 64) {
            const int here = (int)std::min<long long>(64, per_bin - s0);
            am_trace_bin mine{};
            if (lane < here) mine = p[s0 + lane];
            for (int k = 0; k < here; ++k) {
                const unsigned c = __shfl(mine.count, k, 64);
                sum += __shfl(mine.sum, k, 64);
                sq += __shfl(mine.sumsq, k, 64);
                const float vx = __shfl(mine.max, k, 64), vn = __shfl(mine.min, k, 64);
                const unsigned ox = __shfl(mine.argmax, k, 64), on = __shfl(mine.argmin, k, 64);
                if (!c) continue;
                cnt += c;
                take_max(mx, omx, vx, ox);
                take_min(mn, omn, vn, on);
            }
        }
        am_trace_bin r;
        r.max = cnt ? mx : __uint_as_float(0x7FC00000u);
        r.min = cnt ? mn : __uint_as_float(0x7FC00000u);
        r.argmax = cnt ? omx : 0u;
        r.argmin = cnt ? omn : 0u;
        r.count = cnt;
        r.reserved = 0u;
        r.sum = sum;
        r.sumsq = sq;
        if (lane == 0) out[b] = r;
    }
}

int grid_of(long long units, long long per_block) {
    return (int)std::max<long long>(1, std::min<long long>((units + per_block - 1) / per_block, kTraceBlocks));
}

}  // namespace

int trace_check_bin(uint64_t bin) {
    if (bin == 0 || bin > AM_TRACE_MAX_BIN) return fail(AM_ERR_INVALID_ARG, "trace: bin must be 1 .. 2^30 scores");
    return AM_OK;
}

// The records of the first min(nb, cap) bins of the resident scores d_g[0, n) into the host array `out`; *n_out = nb.
// The caller holds the context's lock.  Synchronous.
int trace_reduce(Ctx* c, const float* d_g, long long n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out) {
    const long long D = (long long)bin, nb_all = (n + D - 1) / D;
    *n_out = (size_t)nb_all;
    const long long nb = (long long)std::min<uint64_t>((uint64_t)nb_all, cap);
    if (nb > 0) {
        int rc;
        if ((rc = c->trace_out.ensure(sizeof(am_trace_bin) * (size_t)nb))) return rc;
        am_trace_bin* d_out = (am_trace_bin*)c->trace_out.p;
        const long long form = snapshot_opts(nullptr).trace_form;
        const bool sliced = form == 2 || (form == 0 && D > AM_TRACE_WAVE_BIN_MAX);
        if (!sliced) {
            ProfScope ps(c, KN_TRACE, c->stream);
            hipLaunchKernelGGL(trace_bins, dim3(grid_of(nb, 4)), dim3(kTraceThreads), 0, c->stream, d_g, n, D, nb, d_out);
            AM_HIP(hipGetLastError());
        } else {
            const long long per_bin = (D + AM_TRACE_SLICE - 1) / AM_TRACE_SLICE;
            if ((rc = c->trace_parts.ensure(sizeof(am_trace_bin) * (size_t)(nb * per_bin)))) return rc;
            am_trace_bin* d_parts = (am_trace_bin*)c->trace_parts.p;
            ProfScope ps(c, KN_TRACE, c->stream);
            hipLaunchKernelGGL(trace_slices, dim3(grid_of(nb * per_bin, 4)), dim3(kTraceThreads), 0, c->stream, d_g, n, D, nb, per_bin,
                               d_parts);
            AM_HIP(hipGetLastError());
            hipLaunchKernelGGL(trace_finish, dim3(grid_of(nb, 4)), dim3(kTraceThreads), 0, c->stream,
                               (const am_trace_bin*)d_parts, nb, per_bin, d_out);
            AM_HIP(hipGetLastError());
        }
        if ((rc = download(c, out, d_out, sizeof(am_trace_bin) * (size_t)nb))) return rc;
    }
    if ((uint64_t)nb_all > cap) return fail(AM_ERR_CAPACITY, "trace output buffer too small");
    return AM_OK;
}

// am_match_trace on one resident haystack: its Valid scores (haystack_scores, am_best.hip), then the reduction.  The
// caller holds the context's lock and has checked the arguments.
int match_trace_one(am_needle* h, const void* d_hay, size_t len, int sample_format, const am_trace_params* tp, am_trace_bin* out,
                    size_t cap, size_t* n_out) {
    *n_out = 0;
    if (len < h->n) return AM_OK;
    const float* d_sc = nullptr;
    long long n = 0;
    int rc;
    if ((rc = haystack_scores(h, snapshot_opts(h), d_hay, len, sample_format, tp->scale, &d_sc, &n))) return rc;
    return trace_reduce(h->ctx, d_sc, n, tp->bin, out, cap, n_out);
}

}  // namespace am

// ---------------------------------------------------------------------------
using namespace am;

int am_trace_len(size_t n_scores, uint64_t bin, size_t* n_bins) {
    if (!n_bins) return fail(AM_ERR_INVALID_ARG, "null pointer");
    int rc = trace_check_bin(bin);
    if (rc) return rc;
    *n_bins = (size_t)(n_scores / bin + (n_scores % bin ? 1 : 0));
    return AM_OK;
}

static int trace_scores_impl(int device, const float* scores, size_t n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out,
                             bool device_io) {
    if (!n_out || (!scores && n) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    int rc = trace_check_bin(bin);
    if (rc) return rc;
    if (device_io && (reinterpret_cast<uintptr_t>(scores) & 3)) return fail(AM_ERR_INVALID_ARG, "trace: scores must be 4-byte aligned");
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    *n_out = 0;
    if (n == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_scores = nullptr;
    if ((rc = resident_input(c, device_io, scores, sample_bytes(n), &d_scores))) return rc;
    return trace_reduce(c, (const float*)d_scores, (long long)n, bin, out, cap, n_out);
}

int am_trace_scores(int device, const float* scores, size_t n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out) {
    return trace_scores_impl(device, scores, n, bin, out, cap, n_out, false);
}

int am_trace_scores_device(int device, const float* d_scores, size_t n, uint64_t bin, am_trace_bin* out, size_t cap, size_t* n_out) {
    return trace_scores_impl(device, d_scores, n, bin, out, cap, n_out, true);
}

static int trace_check(const am_needle* h, int sample_format, const am_trace_params* tp) {
    int rc = check_needle(h);
    if (rc) return rc;
    if (!tp) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format)) || (rc = trace_check_bin(tp->bin))) return rc;
    if (tp->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_trace_params: reserved must be 0");
    if (tp->scale != AM_SCALE_NONE && tp->scale != AM_SCALE_LIB)
        return fail(AM_ERR_INVALID_ARG, "am_match_trace: scale must be AM_SCALE_NONE or AM_SCALE_LIB (AM_SCALE_MY depends on a chunk)");
    return norm_check(norm_spec(h, snapshot_opts(h)), tp->scale);
}

static int match_trace_impl(const am_needle* hc, const void* haystack, size_t len, int sample_format, const am_trace_params* tp,
                            am_trace_bin* out, size_t cap, size_t* n_out, bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = trace_check(h, sample_format, tp);
    if (rc) return rc;
    if (!n_out || (!haystack && len) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n_out = 0;
    if (len < h->n) return AM_OK;
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_hay = nullptr;
    if ((rc = resident_input(c, device_io, haystack, sample_bytes(len), &d_hay, ""))) return rc;
    return match_trace_one(h, d_hay, len, sample_format, tp, out, cap, n_out);
}

int am_match_trace_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_trace_params* tp,
                          am_trace_bin* out, size_t cap, size_t* n_out) {
    return match_trace_impl(h, d_haystack, len, sample_format, tp, out, cap, n_out, true);
}

int am_match_trace(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_trace_params* tp,
                   am_trace_bin* out, size_t cap, size_t* n_out) {
    return match_trace_impl(h, haystack, len, sample_format, tp, out, cap, n_out, false);
}

int am_match_trace_batch_device(const am_needle* hc, const void* const* d_haystacks, const size_t* lens, size_t n_hay,
                                int sample_format, const am_trace_params* tp, am_trace_bin* out, size_t cap_per_hay, size_t* n_out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = trace_check(h, sample_format, tp);
    if (rc) return rc;
    if (n_hay == 0) return AM_OK;
    if (!d_haystacks || !lens || !n_out || (!out && cap_per_hay)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    for (size_t i = 0; i < n_hay; ++i)
        if (!d_haystacks[i] && lens[i]) return fail(AM_ERR_INVALID_ARG, "haystack " + std::to_string(i) + ": null pointer");
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    for (size_t i = 0; i < n_hay; ++i)
        if (lens[i] >= h->n && (rc = hit_check_device(d_haystacks[i], c->device, HitWhere{(long long)i, i, 0, 0}))) return rc;
    // every haystack is traced; the first one that does not fit decides the return value
    int first = AM_OK;
    std::string first_msg;
    for (size_t i = 0; i < n_hay; ++i) {
        rc = match_trace_one(h, d_haystacks[i], lens[i], sample_format, tp, out + i * cap_per_hay, cap_per_hay, n_out + i);
        if (rc == AM_ERR_CAPACITY) {
            if (first == AM_OK) { first = rc; first_msg = "haystack " + std::to_string(i) + ": " + t_err; }
        } else if (rc) {
            return rc;
        }
    }
    return first == AM_OK ? AM_OK : fail(first, first_msg);
}

// Pure host: what a caller usually wants of a trace, in f64.
int am_trace_summary(const am_trace_bin* bins, size_t n_bins, uint64_t bin, am_trace_stats* out) {
    if (!out || (!bins && n_bins)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    int rc = trace_check_bin(bin);
    if (rc) return rc;
    const double nan = std::nan("");
    am_trace_stats r{};
    r.count = 0;
    r.max = r.min = r.mean = r.std = r.median_max = r.mad_max = r.peak_z = nan;
    r.argmax = r.argmin = 0;
    double sum = 0.0, sumsq = 0.0;
    bool any = false;
    std::vector<double> tops;
    for (size_t b = 0; b < n_bins; ++b) {
        const am_trace_bin& x = bins[b];
        if (!x.count) continue;
        r.count += x.count;
        sum += x.sum;
        sumsq += x.sumsq;
        tops.push_back((double)x.max);
        if (!any || (double)x.max > r.max) { r.max = (double)x.max; r.argmax = (uint64_t)b * bin + x.argmax; }
        if (!any || (double)x.min < r.min) { r.min = (double)x.min; r.argmin = (uint64_t)b * bin + x.argmin; }
        any = true;
    }
    if (any) {
        const double cnt = (double)r.count;
        r.mean = sum / cnt;
        const double var = sumsq / cnt - r.mean * r.mean;
        r.std = var != var ? nan : std::sqrt(var > 0.0 ? var : 0.0);   // (infinite scores: inf - inf)
        auto median = [](std::vector<double>& v) {   // (v holds no NaN)
            std::sort(v.begin(), v.end());
            const size_t m = v.size();
            return m % 2 ? v[m / 2] : 0.5 * (v[m / 2 - 1] + v[m / 2]);
        };
        r.median_max = median(tops);
        if (r.median_max == r.median_max) {
            // a maximum equal to the median deviates by 0 from it, an infinite one included (never inf - inf)
            for (double& t : tops) t = t == r.median_max ? 0.0 : std::fabs(t - r.median_max);
            r.mad_max = median(tops);
            if (r.mad_max > 0.0) r.peak_z = (r.max - r.median_max) / (1.4826 * r.mad_max);
            else r.peak_z = r.max > r.median_max ? HUGE_VAL : 0.0;
        }   // (else +inf and -inf are the two middle maxima: no median, MAD and peak_z stay NaN)
    }
    *out = r;
    return AM_OK;
}
