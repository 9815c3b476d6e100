// am_segments.hip -- per-segment hit scoring (am_hit_segments*, include/audiomatch.h): the pass of am_hits.hip resolved
// along the needle.  For a hit at t, the needle cut into m segments [a_j, a_{j+1}), a_j = floor(j S / m), and the lags
// l = -R .. R, in f64:
//   c_j(l) = sum_{i in seg j} x[t + l + i] n[i],   E_w,j(l) = sum_{i in seg j} x[t + l + i]^2,   E_n,j = sum_{i in seg j} n[i]^2
// (x = 0 outside the haystack) and from those, per segment, the best lag with its parabola vertex and the NCC, gain and
// level there.
//
// Two kernels on the context's stream:
//   seg_slices    one workgroup per slice of kHitSlice needle samples counted from the segment's start (blockIdx.x =
//                 slice within the segment, blockIdx.y = hit * m + segment): stages x over the slice plus RT samples each
//                 side in LDS once (stage_load), keeps the thread's needle samples in registers, accumulates the
//                 2 RT + 1 pairs (c, E_w) and E_n from that one read, adds them over the workgroup (wave_sums, add_waves)
//                 and writes one partial record, one 64-bit store per lane.  RT is the smallest of kSegRadii that holds
//                 R: three instances per sample format, the accumulators in registers.
//   seg_combine   one wave per (hit, segment): adds the segment's partials (sum_slices), picks l* (pick_lag), the vertex
//                 (refine_lag) and the flags and writes the am_hit_segment.
// The kernels read x[t + u] for u in [-R, S + R) inside the haystack only (SegDesc::ulo, uhi), whatever RT is: that is
// what the host form stages, and lags beyond R never reach a result.  A segment's result depends on the needle, the
// samples it reads, m, R and the floor only (slices start at multiples of kHitSlice from a_j, every reduction runs in
// the fixed order am_hit_device.h states): the single, batch and host forms agree bit for bit.  The three forms run in the frame of am_hits.hip
// (am_internal.h: hit_call, hit_call_batch, hit_round_trip); SegFamily below is what this family adds to it.
// am_warp.hip runs seg_slices alone (launch_seg_slices, m = 1) over a table of its own and combines the records itself.
#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegPer = kHitSlice / kSegThreads;   // needle samples per thread and slice
constexpr int kSegMaxRecord = 2 * (2 * AM_SEG_MAX_RADIUS + 1) + 1;
static_assert(kHitSlice % kSegThreads == 0, "slice must split evenly over the workgroup");
static_assert(kSegRadii[2] == AM_SEG_MAX_RADIUS, "the widest kernel holds every radius");
static_assert(2 * AM_SEG_MAX_RADIUS <= kSegThreads && kSegMaxRecord < kSegThreads, "one staged tail sample and one record value per thread");

__device__ __forceinline__ long long seg_start(long long j, long long s, int m) { return j * s / m; }   // a_j (j <= 1024, s < 2^52)

template <int KIND, int RT>
__global__ __launch_bounds__(kSegThreads) void seg_slices_kernel(const SegDesc* __restrict__ hits, long long g0, int m, int r,
                                                                 double* __restrict__ parts, unsigned* __restrict__ pflags) {
    constexpr int NL = 2 * RT + 1, NV = 2 * NL + 1;
    __shared__ float xs[kHitSlice + 2 * RT];
    __shared__ double ws[NV][kSegThreads / 64];
    const long long g = g0 + blockIdx.y, h = g / m;
    const int j = (int)(g - h * m);
    const SegDesc d = hits[h];
    const long long a0 = seg_start(j, d.s, m), a1 = seg_start(j + 1, d.s, m);
    const long long i0 = (long long)blockIdx.x * kHitSlice;
    if (i0 >= a1 - a0) return;   // (a shorter segment than the launch's longest: whole workgroups leave together)
    const int tid = threadIdx.x;
    const int cnt = (int)min((long long)kHitSlice, a1 - a0 - i0);
    // every load of the slice in flight at once: xs[q] = x[t + a0 + i0 - RT + q] (stage_load, stage_store) and the
    // thread's needle samples n[a0 + i0 + q]; a staged sample counts for the segment's non-finite flag when one of the
    // lags -r .. r reads it
    gfloat* nd = (gfloat*)d.needle + (a0 + i0);
    const int qlo = RT - r, qhi = cnt + RT + r;
    float xv[kSegPer], nv[kSegPer], xt;
    stage_load<KIND, kSegThreads>(d.win, a0 + i0 - RT, cnt, 2 * RT, d.ulo, d.uhi, xv, xt, [&](int k, int q) { nv[k] = q < cnt ? nd[q] : 0.0f; });
    bool bad = false;
    // (the needle's test stands ahead of stage_store on purpose: behind it the compiler takes 84 and 180 VGPRs at RT = 4
    // and 16 instead of 82 and 178; results do not depend on the place)
#pragma unroll
    for (int k = 0; k < kSegPer; ++k) bad |= !__builtin_isfinite(nv[k]);
    stage_store<kSegThreads>(StageFlat{}, xs, 2 * RT, xv, xt, [&](int q, float x) { bad |= q >= qlo && q < qhi && !__builtin_isfinite(x); });
    __syncthreads();
    double acc[NV];   // the record: c(-RT .. RT), E_w(-RT .. RT), E_n
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kSegPer; ++k) {
        const int q = tid + k * kSegThreads;
        if (q < cnt) {
            const double dn = (double)nv[k];
            acc[2 * NL] += dn * dn;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double dx = (double)xs[q + l];
                acc[l] += dx * dn;   // (a product of two f32 values is exact in f64)
                acc[NL + l] += dx * dx;
            }
        }
    }
    wave_sums<kSegThreads>(acc, ws);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    // one 64-bit store per lane: no record leaves as one wide store (tools/check_store_hazard.py)
    const long long p = d.part0 + (long long)j * d.nsl + blockIdx.x;
    if (tid < NV) parts[NV * p + tid] = add_waves<kSegThreads>(ws[tid]);
    else if (tid == NV) pflags[p] = (unsigned)any_bad;
}

// One wave per (hit, segment): lane k adds value k (and k + 64) of the segment's partial records (sum_slices), lane 0
// turns the sums into the record.
__global__ __launch_bounds__(64) void seg_combine_kernel(const SegDesc* __restrict__ hits, int m, int r, int rt,
                                                         const double* __restrict__ parts, const unsigned* __restrict__ pflags,
                                                         am_hit_segment* __restrict__ out) {
    __shared__ double sh[kSegMaxRecord];
    const long long g = blockIdx.x, h = g / m;
    const int j = (int)(g - h * m);
    const int lane = threadIdx.x;
    const SegDesc d = hits[h];
    const long long a0 = seg_start(j, d.s, m), a1 = seg_start(j + 1, d.s, m);
    const long long ns = (a1 - a0 + kHitSlice - 1) / kHitSlice, p0 = d.part0 + (long long)j * d.nsl;
    const int nl = 2 * rt + 1, nv = 2 * nl + 1;
    for (int k = lane; k < nv; k += 64) sh[k] = sum_slices(parts, nv, p0, ns, k);
    const int bad = __syncthreads_or(or_flags(pflags, p0, ns, lane, 64) != 0 ? 1 : 0);
    if (lane != 0) return;
    const double* cc = sh + rt;        // cc[l] = c_j(l), ee[l] = E_w,j(l) for -rt <= l <= rt
    const double* ee = sh + nl + rt;
    const double en = sh[2 * nl];
    const double nan = __builtin_nan("");
    double lag = 0.0;
    float ncc, gain, ldb;
    unsigned flags = 0;
    if (bad) {
        flags = AM_HIT_NONFINITE;
        ncc = gain = ldb = (float)nan;
    } else if (en == 0.0) {
        flags = AM_HIT_EMPTY_SEGMENT;
        ncc = gain = 0.0f;
        ldb = ee[0] > 0.0 ? __builtin_inff() : (float)nan;
    } else {
        const int ls = pick_lag<false>(cc, r);
        const double bb = cc[ls], ew = ee[ls];
        bool refined, below;
        lag = refine_lag<false>(cc, r, ls, &refined);
        if (!refined) flags |= AM_HIT_UNREFINED;
        ncc = (float)ncc_or_floor(bb, en, ew, en * d.floor_ratio, &below);
        if (below) flags |= AM_HIT_BELOW_FLOOR;
        gain = (float)(bb / en);
        ldb = level_db(ew, en);
    }
    am_hit_segment* o = out + g;
    o->lag = lag;
    o->ncc = ncc;
    o->gain = gain;
    o->level_db = ldb;
    o->flags = flags;
}

template <int KIND, int RT>
void launch_seg_slices(hipStream_t st, dim3 grid, const SegDesc* d_hits, long long g0, int m, int r, double* parts, unsigned* pflags) {
    hipLaunchKernelGGL((seg_slices_kernel<KIND, RT>), grid, dim3(kSegThreads), 0, st, d_hits, g0, m, r, parts, pflags);
}

template <int KIND>
void launch_seg_slices_rt(hipStream_t st, int rt, dim3 grid, const SegDesc* d_hits, long long g0, int m, int r, double* parts,
                          unsigned* pflags) {
    if (rt == kSegRadii[0]) launch_seg_slices<KIND, kSegRadii[0]>(st, grid, d_hits, g0, m, r, parts, pflags);
    else if (rt == kSegRadii[1]) launch_seg_slices<KIND, kSegRadii[1]>(st, grid, d_hits, g0, m, r, parts, pflags);
    else launch_seg_slices<KIND, kSegRadii[2]>(st, grid, d_hits, g0, m, r, parts, pflags);
}

}  // namespace

hipError_t launch_seg_slices(hipStream_t st, const SegDesc* d_hits, long long n, int m, int r, int max_nsl, int kind, double* parts,
                             unsigned* pflags) {
    const int rt = seg_kernel_radius(r);
    return for_each_grid_y(n * m, [&](long long g0, unsigned ng) {
        const dim3 grid((unsigned)max_nsl, ng);
        if (kind) launch_seg_slices_rt<1>(st, rt, grid, d_hits, g0, m, r, parts, pflags);
        else launch_seg_slices_rt<0>(st, rt, grid, d_hits, g0, m, r, parts, pflags);
    });
}

hipError_t launch_hit_segments(hipStream_t st, const SegDesc* d_hits, long long n, int m, int r, int max_nsl, int kind,
                               double* parts, unsigned* pflags, am_hit_segment* d_out) {
    if (n <= 0) return hipSuccess;
    const hipError_t e = launch_seg_slices(st, d_hits, n, m, r, max_nsl, kind, parts, pflags);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seg_combine_kernel, dim3((unsigned)(n * m)), dim3(64), 0, st, d_hits, m, r, seg_kernel_radius(r),
                       (const double*)parts, (const unsigned*)pflags, d_out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

// scores every hit of `hits` in one launch sequence on c's stream; out[i]: host destination of hit i's sp.segments records
int score_segments(Ctx* c, std::vector<SegDesc>& hits, const am_segment_params& sp, am_hit_segment* const* out) {
    const long long m = sp.segments;
    long long total = 0;
    int max_nsl = 0;
    for (SegDesc& d : hits) {
        const long long longest = (d.s + m - 1) / m;   // (the longest segment of a needle: ceil(s / m))
        d.nsl = (int)((longest + kHitSlice - 1) / kHitSlice);
        d.part0 = total;
        total += m * d.nsl;
        max_nsl = std::max(max_nsl, d.nsl);
    }
    return hit_round_trip(c, hits, sizeof(double) * (size_t)seg_record_len(seg_kernel_radius((int)sp.radius)), (size_t)total, (size_t)m, out,
                          [&](const SegDesc* tab, double* parts, unsigned* pflags, am_hit_segment* d_out) {
                              return launch_hit_segments(c->stream, tab, (long long)hits.size(), (int)m, (int)sp.radius, max_nsl, hits[0].kind,
                                                         parts, pflags, d_out);
                          });
}

// AM_ERR_INVALID_ARG unless sp is a valid request for a needle of s samples (`who`: "" or "needle j: ")
int seg_check_params(const am_segment_params* sp, size_t s, const std::string& who) {
    if (sp->radius > AM_SEG_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(sp->radius) + " > AM_SEG_MAX_RADIUS (" + std::to_string(AM_SEG_MAX_RADIUS) + ")");
    if (sp->segments == 0) return fail(AM_ERR_INVALID_ARG, "segments = 0");
    if (sp->segments > s)
        return fail(AM_ERR_INVALID_ARG, who + "segments " + std::to_string(sp->segments) + " > needle length " + std::to_string(s));
    if (sp->segments > AM_SEG_MAX_SEGMENTS)
        return fail(AM_ERR_INVALID_ARG, "segments " + std::to_string(sp->segments) + " > AM_SEG_MAX_SEGMENTS (" + std::to_string(AM_SEG_MAX_SEGMENTS) + ")");
    return AM_OK;
}

// am_hit_segments*: a hit at t reads [t - R, t + S + R), clipped to the haystack
struct SegFamily {
    typedef SegDesc Desc;
    typedef am_hit_segment Rec;
    const am_segment_params* sp;
    const void* params() const { return sp; }
    size_t recs() const { return sp->segments; }
    int check_call() const { return AM_OK; }
    int check(const am_needle* h, long long j) const { return seg_check_params(sp, h->n, hit_needle_name(j)); }
    double floor(const am_needle* h) const { return hit_floor_ratio(h); }
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double ratio, const HitWhere& where,
             SegDesc* d) const {
        HitDesc hd{};
        const long long r = sp->radius;
        int rc;
        if ((rc = hit_desc(h, hay, len, sample_format, pk, 0.0, where, &hd))) return rc;
        *d = SegDesc{hd.win, hd.needle, hd.s, -std::min(r, hd.t), std::min(hd.s + r, (long long)len - hd.t), 0, ratio, hd.kind, 0};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const {
        const size_t r = sp->radius;
        return HitRange{t > r ? t - r : 0, std::min(len, t + h->n + r)};
    }
    int score(Ctx* c, std::vector<SegDesc>& hits, am_hit_segment* const* out) const { return score_segments(c, hits, *sp, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_segments(const am_needle* h, const void* haystack, size_t len, int sample_format,
                    const am_peak* peaks, size_t n, const am_segment_params* sp, am_hit_segment* out) {
    return hit_call(SegFamily{sp}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_segments_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                           const am_peak* peaks, size_t n, const am_segment_params* sp, am_hit_segment* out) {
    return hit_call(SegFamily{sp}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_segments_batch_device(const am_needle* const* needles, size_t n_needles,
                                 const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                 const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                 const am_segment_params* sp, am_hit_segment* out) {
    return hit_call_batch(SegFamily{sp}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

int am_hit_segments_summary(const am_hit_segment* seg, uint32_t segments, size_t needle_len, float min_ncc,
                            am_segment_summary* out) {
    if (!seg || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (segments == 0 || segments > needle_len) return fail(AM_ERR_INVALID_ARG, "segments = 0 or > needle length");
    const double nan = std::nan("");
    const uint64_t m = segments, s = needle_len;
    auto start = [&](uint64_t j) { return (double)(j * s / m); };   // a_j (exact: below 2^53)
    const unsigned absent = AM_HIT_NONFINITE | AM_HIT_BELOW_FLOOR | AM_HIT_EMPTY_SEGMENT;
    am_segment_summary r{};
    r.first_present = r.last_present = -1;
    double covered = 0.0, sx = 0.0, sy = 0.0;
    std::vector<double> xs, ys;   // centres and lags of the usable segments, in index order
    for (uint64_t j = 0; j < m; ++j) {
        const am_hit_segment& q = seg[j];
        if ((q.flags & absent) || !(q.ncc >= min_ncc)) continue;
        if (r.first_present < 0) r.first_present = (int32_t)j;
        r.last_present = (int32_t)j;
        ++r.n_present;
        covered += start(j + 1) - start(j);
        if (q.flags & AM_HIT_UNREFINED) continue;
        ++r.n_usable;
        xs.push_back(0.5 * (start(j) + start(j + 1)));
        ys.push_back(q.lag);
        sx += xs.back();
        sy += ys.back();
    }
    r.coverage = covered / (double)s;
    r.drift_ppm = r.start_lag = r.residual_rms = nan;
    if (r.n_usable >= 2) {
        const double k = (double)r.n_usable, mx = sx / k, my = sy / k;
        double sxx = 0.0, sxy = 0.0, res = 0.0;
        for (size_t i = 0; i < xs.size(); ++i) {
            sxx += (xs[i] - mx) * (xs[i] - mx);
            sxy += (xs[i] - mx) * (ys[i] - my);
        }
        const double slope = sxy / sxx;
        r.drift_ppm = 1e6 * slope;
        r.start_lag = my - slope * mx;
        for (size_t i = 0; i < xs.size(); ++i) {
            const double dv = ys[i] - (r.start_lag + slope * xs[i]);
            res += dv * dv;
        }
        r.residual_rms = std::sqrt(res / k);
    }
    *out = r;
    return AM_OK;
}

}  // extern "C"
