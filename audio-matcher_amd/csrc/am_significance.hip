// am_significance.hip -- per-hit significance (am_hit_significance*, include/audiomatch.h): a hit's score against the
// scores around it.  For a hit at t, guard G and radius B the zone is the lags lo = max(0, t - B) .. hi = min(len - S,
// t + B); its f32 scores r(u) are the AM_MODE_VALID scores of the span x[lo, hi + S) correlated as a buffer of its own
// (valid_scores, am_best.hip: what am_correlate runs), the background the zone's lags with |u - t| > G.
//
// Per group of hits (the score buffer stays bounded): every hit's span is copied (or down-mixed) to offset 0 of a
// scratch span of its own and correlated into its zone of the score buffer; then four kernels on the context's stream:
//   sig_sums      one workgroup per slice of kSigSlice zone scores of one hit (blockIdx.x = slice, blockIdx.y = hit):
//                 count, f64 sum and largest score (with its tie rule) of the slice's background lags, one partial each.
//   sig_mean      one wave per hit: walks the hit's partials in slice order; count, mean and the largest score.
//   sig_devs      the grid of sig_sums: the f64 sum of (r - mean)^2 over the slice's background lags.
//   sig_finish    one wave per hit: adds those partials in slice order and writes the am_significance record.
// No atomics: a thread adds its scores in index order, the workgroup by block_sum (am_hit_device.h), the slices in index
// order.
// Slices start at multiples of kSigSlice from the zone's first lag, so a hit's record depends on its own zone only --
// not on the group, the call or the entry point.  The three call forms run in the frame of am_hits.hip (am_internal.h:
// hit_call, hit_call_batch); SigFamily below is what this family adds to it, and score_significance uses the frame's
// table and result halves per group.
#include "am_hit_device.h"
#include "am_internal.h"

#include <climits>

namespace am {

namespace {

constexpr int kSigThreads = 256;
constexpr int kSigPer = kSigSlice / kSigThreads;   // zone scores per thread and slice
constexpr size_t kSigGroupSamples = (size_t)64 << 20;   // span samples a group of hits holds (256 MB; one hit always fits)
static_assert(kSigSlice % kSigThreads == 0, "slice must split evenly over the workgroup");

// (va at lag da) before (vb at lag db): the larger score; ties to the smaller |lag|, then to the negative lag
__device__ __forceinline__ bool sig_before(float va, int da, float vb, int db) {
    if (va != vb) return va > vb;
    const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
    return aa < ab || (aa == ab && da < db);
}
// folds the candidate (cb scores, best vb at db) into (cnt, v, d)
__device__ __forceinline__ void sig_fold(unsigned& cnt, float& v, int& d, unsigned cb, float vb, int db) {
    if (cb && (!cnt || sig_before(vb, db, v, d))) { v = vb; d = db; }
    cnt += cb;
}

// The slice's scores of one thread: zone indices k0 + tid + j kSigThreads, every load in flight at once; bg[j] says
// whether the index is a background lag.
struct SigLoad { float v[kSigPer]; bool bg[kSigPer]; int d[kSigPer]; };
__device__ __forceinline__ void sig_load(const SigDesc& d, const float* __restrict__ scores, long long k0, SigLoad& l) {
    const float* z = scores + d.z0;
#pragma unroll
    for (int j = 0; j < kSigPer; ++j) {
        const long long k = k0 + threadIdx.x + j * kSigThreads;
        const long long dd = k - d.c, ad = dd < 0 ? -dd : dd;
        l.bg[j] = k < d.nz && ad > d.g;
        l.d[j] = (int)dd;   // (|dd| <= AM_SIG_MAX_RADIUS for every index of the zone)
        l.v[j] = l.bg[j] ? z[k] : 0.0f;
    }
}

__global__ __launch_bounds__(kSigThreads) void sig_sums_kernel(const SigDesc* __restrict__ hits, long long hit0,
                                                               const float* __restrict__ scores, double* __restrict__ psum,
                                                               unsigned* __restrict__ pmax) {
    __shared__ double ws[kSigThreads / 64];
    __shared__ unsigned wc[kSigThreads / 64];
    __shared__ float wv[kSigThreads / 64];
    __shared__ int wd[kSigThreads / 64];
    const SigDesc d = hits[hit0 + blockIdx.y];
    const long long k0 = (long long)blockIdx.x * kSigSlice;
    if (k0 >= d.nz) return;   // (a shorter zone than the launch's longest: whole workgroups leave together)
    SigLoad l;
    sig_load(d, scores, k0, l);
    double sum = 0.0;
    unsigned cnt = 0;
    float bv = 0.0f;
    int bd = 0;
#pragma unroll
    for (int j = 0; j < kSigPer; ++j) {
        if (l.bg[j]) {
            sum += (double)l.v[j];
            sig_fold(cnt, bv, bd, 1u, l.v[j], l.d[j]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned cb = __shfl_xor(cnt, off, 64);
        const float vb = __shfl_xor(bv, off, 64);
        const int db = __shfl_xor(bd, off, 64);
        sig_fold(cnt, bv, bd, cb, vb, db);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { wc[w] = cnt; wv[w] = bv; wd[w] = bd; }
    const double total = block_sum<kSigThreads>(sum, ws);   // (its barrier also publishes wc, wv, wd)
    cnt = 0; bv = 0.0f; bd = 0;
    for (int i = 0; i < kSigThreads / 64; ++i) sig_fold(cnt, bv, bd, wc[i], wv[i], wd[i]);
    // one store of at most 64 bits per lane: no record leaves as one wide store (tools/check_store_hazard.py)
    const long long p = d.part0 + blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) psum[p] = total;
    else if (tid == 1) pmax[3 * p] = cnt;
    else if (tid == 2) pmax[3 * p + 1] = __float_as_uint(bv);
    else if (tid == 3) pmax[3 * p + 2] = (unsigned)bd;
}

// One wave per hit: the lanes fetch 64 partial records at a time into LDS, lane 0 folds them in slice order.
__global__ __launch_bounds__(64) void sig_mean_kernel(const SigDesc* __restrict__ hits, const double* __restrict__ psum,
                                                      const unsigned* __restrict__ pmax, double* __restrict__ mean,
                                                      unsigned* __restrict__ hmax) {
    __shared__ double ps[64];
    __shared__ unsigned pc[64], pv[64], pd[64];
    __shared__ unsigned res[3];
    const long long h = blockIdx.x;
    const int lane = threadIdx.x;
    const SigDesc d = hits[h];
    const long long ns = (d.nz + kSigSlice - 1) / kSigSlice;
    double sum = 0.0;
    unsigned cnt = 0;
    float bv = 0.0f;
    int bd = 0;
    for (long long k0 = 0; k0 < ns; k0 += 64) {
        const long long k = k0 + lane;
        if (k < ns) {
            const long long p = d.part0 + k;
            ps[lane] = psum[p];
            pc[lane] = pmax[3 * p];
            pv[lane] = pmax[3 * p + 1];
            pd[lane] = pmax[3 * p + 2];
        }
        __syncthreads();
        if (lane == 0) {
            const int m = (int)min(64ll, ns - k0);
            for (int i = 0; i < m; ++i) {
                sum += ps[i];
                sig_fold(cnt, bv, bd, pc[i], __uint_as_float(pv[i]), (int)pd[i]);
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        mean[h] = sum / (double)cnt;   // (NaN for an empty background: nothing reads it then)
        res[0] = cnt; res[1] = __float_as_uint(bv); res[2] = (unsigned)bd;
    }
    __syncthreads();
    if (lane < 3) hmax[3 * h + lane] = res[lane];
}

__global__ __launch_bounds__(kSigThreads) void sig_devs_kernel(const SigDesc* __restrict__ hits, long long hit0,
                                                               const float* __restrict__ scores, const double* __restrict__ mean,
                                                               double* __restrict__ psum) {
    __shared__ double ws[kSigThreads / 64];
    const SigDesc d = hits[hit0 + blockIdx.y];
    const long long k0 = (long long)blockIdx.x * kSigSlice;
    if (k0 >= d.nz) return;
    SigLoad l;
    sig_load(d, scores, k0, l);
    const double mu = mean[hit0 + blockIdx.y];
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < kSigPer; ++j) {
        if (l.bg[j]) {
            const double e = (double)l.v[j] - mu;
            ss += e * e;
        }
    }
    const double total = block_sum<kSigThreads>(ss, ws);
    if (threadIdx.x == 0) psum[d.part0 + blockIdx.x] = total;
}

// One wave per hit: adds the squared deviations in slice order, lane 0 turns the sums into the record, which leaves as
// one 32-bit store per lane.
__global__ __launch_bounds__(64) void sig_finish_kernel(const SigDesc* __restrict__ hits, const float* __restrict__ scores,
                                                        const double* __restrict__ psum, const double* __restrict__ mean,
                                                        const unsigned* __restrict__ hmax, am_significance* __restrict__ out) {
    __shared__ double ps[64];
    __shared__ unsigned rec[8];
    static_assert(sizeof(am_significance) == 8 * sizeof(unsigned), "the record leaves as eight words");
    const long long h = blockIdx.x;
    const int lane = threadIdx.x;
    const SigDesc d = hits[h];
    const long long ns = (d.nz + kSigSlice - 1) / kSigSlice;
    double ss = 0.0;
    for (long long k0 = 0; k0 < ns; k0 += 64) {
        const long long k = k0 + lane;
        if (k < ns) ps[lane] = psum[d.part0 + k];
        __syncthreads();
        if (lane == 0) {
            const int m = (int)min(64ll, ns - k0);
            for (int i = 0; i < m; ++i) ss += ps[i];
        }
        __syncthreads();
    }
    if (lane == 0) {
        const float fnan = __uint_as_float(0x7FC00000u);
        const unsigned n_bg = hmax[3 * h];
        float score = scores[d.z0 + d.c], fmean = fnan, fstd = fnan, z = fnan, side = fnan;
        int side_lag = 0;
        unsigned flags = d.flags;
        if (flags & AM_HIT_NONFINITE) {
            score = fnan;
        } else if (n_bg < 2) {
            flags |= AM_HIT_NO_BACKGROUND;
        } else {
            const double mu = mean[h], sd = sqrt(ss / (double)n_bg), diff = (double)score - mu;
            fmean = (float)mu;
            fstd = (float)sd;
            if (sd == 0.0) {
                flags |= AM_HIT_FLAT_BACKGROUND;
                z = diff > 0.0 ? __builtin_inff() : diff < 0.0 ? -__builtin_inff() : 0.0f;
            } else {
                z = (float)(diff / sd);
            }
            side = __uint_as_float(hmax[3 * h + 1]);
            side_lag = (int)hmax[3 * h + 2];
        }
        rec[0] = __float_as_uint(score);
        rec[1] = __float_as_uint(fmean);
        rec[2] = __float_as_uint(fstd);
        rec[3] = __float_as_uint(z);
        rec[4] = __float_as_uint(side);
        rec[5] = (unsigned)side_lag;
        rec[6] = n_bg;
        rec[7] = flags;
    }
    __syncthreads();
    if (lane < 8) reinterpret_cast<unsigned*>(out + h)[lane] = rec[lane];
}

}  // namespace

hipError_t launch_hit_significance(hipStream_t st, const SigDesc* d_hits, long long n, long long max_slices, const float* scores,
                                   double* psum, unsigned* pmax, double* mean, unsigned* hmax, am_significance* d_out) {
    if (n <= 0) return hipSuccess;
    hipError_t e = for_each_grid_y(n, [&](long long h0, unsigned nh) {
        hipLaunchKernelGGL(sig_sums_kernel, dim3((unsigned)max_slices, nh), dim3(kSigThreads), 0, st, d_hits, h0, scores, psum, pmax);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sig_mean_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, (const double*)psum, (const unsigned*)pmax, mean, hmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = for_each_grid_y(n, [&](long long h0, unsigned nh) {
        hipLaunchKernelGGL(sig_devs_kernel, dim3((unsigned)max_slices, nh), dim3(kSigThreads), 0, st, d_hits, h0, scores, (const double*)mean, psum);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sig_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, scores, (const double*)psum, (const double*)mean,
                       (const unsigned*)hmax, d_out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

// One hit of a call, as the host sees it
struct SigHit {
    am_needle* h;
    const void* win;         // device: element lo of the haystack (f32 mono, or i16 stereo frames for kind 1)
    int kind;
    long long span_len;      // hi + S - lo
    long long nz, c;         // hi - lo + 1, t - lo
    unsigned flags;          // AM_HIT_CLIPPED
};

// What a call reads of one needle, once: the options in force, the normalisation, the factor, "a sample is not finite"
struct SigNeedle { Opts o; NormSpec nrm; float factor; bool bad; };

int sig_check_params(const am_significance_params* sp) {
    if (sp->radius > AM_SIG_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(sp->radius) + " > AM_SIG_MAX_RADIUS (" + std::to_string(AM_SIG_MAX_RADIUS) + ")");
    if (sp->guard >= sp->radius)
        return fail(AM_ERR_INVALID_ARG, "guard " + std::to_string(sp->guard) + " >= radius " + std::to_string(sp->radius));
    return AM_OK;
}

// scores every hit of `hits` on c's stream, group by group; out[i]: host destination of hit i's record
int score_significance(Ctx* c, std::vector<SigHit>& hits, const am_significance_params& sp, am_significance* const* out) {
    const size_t n = hits.size();
    int rc;
    // every needle of the call once: its options as they are now, and whether it holds a non-finite sample
    std::map<am_needle*, SigNeedle> needles;
    for (const SigHit& q : hits) {
        if (needles.count(q.h)) continue;
        SigNeedle nd{};
        nd.o = snapshot_opts(q.h);
        nd.nrm = norm_spec(q.h, nd.o);
        nd.factor = nd.nrm.on ? norm_factor(nd.nrm) : scale_factor(q.h, AM_SCALE_LIB, 0);
        const Segment whole{0, (long long)q.h->n};
        int flag = 0;
        if ((rc = nonfinite_flags(c, q.h->d_needle, &whole, 1, &flag))) return rc;
        nd.bad = flag != 0;
        needles[q.h] = nd;
    }
    // the partition of every zone into slices (the zone's own), the partials of the whole call one after the other
    std::vector<SigDesc> descs(n);
    long long total = 0;
    for (size_t i = 0; i < n; ++i) {
        SigDesc& d = descs[i];
        d.z0 = 0;
        d.nz = hits[i].nz;
        d.c = hits[i].c;
        d.g = (long long)sp.guard;
        d.part0 = total;
        d.flags = hits[i].flags;
        d.pad = 0;
        total += (d.nz + kSigSlice - 1) / kSigSlice;
    }
    const size_t tab_bytes = sizeof(SigDesc) * n, out_bytes = sizeof(am_significance) * n;
    if ((rc = hit_io_reserve(c, tab_bytes, out_bytes)) || (rc = c->sig_psum.ensure(sizeof(double) * (size_t)total)) ||
        (rc = c->sig_pmax.ensure(3 * sizeof(unsigned) * (size_t)total)) || (rc = c->sig_mean.ensure(sizeof(double) * n)) ||
        (rc = c->sig_hmax.ensure(3 * sizeof(unsigned) * n)))
        return rc;
    std::vector<Segment> ranges;
    std::vector<int> bad;
    for (size_t g0 = 0; g0 < n;) {
        // the group: hits g0 .. g1, their spans and zones one after the other
        size_t g1 = g0, span_total = 0, zone_total = 0;
        long long max_slices = 0;
        ranges.clear();
        while (g1 < n && (g1 == g0 || span_total + (size_t)hits[g1].span_len <= kSigGroupSamples)) {
            ranges.push_back(Segment{(long long)span_total, (long long)span_total + hits[g1].span_len});
            descs[g1].z0 = (long long)zone_total;
            // (every span starts 256-byte aligned, like a buffer of its own: K1 loads its samples in aligned pairs)
            span_total += ((size_t)hits[g1].span_len + 63) & ~(size_t)63;
            zone_total += ((size_t)hits[g1].nz + 63) & ~(size_t)63;
            max_slices = std::max(max_slices, (hits[g1].nz + kSigSlice - 1) / kSigSlice);
            ++g1;
        }
        const size_t ng = g1 - g0;
        if ((rc = c->sig_span.ensure(sizeof(float) * span_total)) || (rc = c->sig_scores.ensure(sizeof(float) * zone_total))) return rc;
        float* d_span = static_cast<float*>(c->sig_span.p);
        float* d_scores = static_cast<float*>(c->sig_scores.p);
        for (size_t i = g0; i < g1; ++i) {
            float* dst = d_span + ranges[i - g0].a;
            if (hits[i].kind) AM_HIP(launch_pcm_downmix(c->stream, static_cast<const int16_t*>(hits[i].win), hits[i].span_len, dst));
            else AM_HIP(hipMemcpyAsync(dst, hits[i].win, sizeof(float) * (size_t)hits[i].span_len, hipMemcpyDeviceToDevice, c->stream));
        }
        bad.assign(ng, 0);
        if ((rc = nonfinite_flags(c, d_span, ranges.data(), (int)ng, bad.data()))) return rc;
        for (size_t i = g0; i < g1; ++i) {
            const SigNeedle& nd = needles[hits[i].h];
            float* zone = d_scores + descs[i].z0;
            if (nd.bad || bad[i - g0]) {
                // no score of a span that holds a non-finite sample counts: the zone reads as NaN
                descs[i].flags = (descs[i].flags & AM_HIT_CLIPPED) | AM_HIT_NONFINITE;
                AM_HIP(hipMemsetD32Async((hipDeviceptr_t)zone, 0x7FC00000, (size_t)hits[i].nz, c->stream));
            } else if ((rc = valid_scores(hits[i].h, nd.o, nd.nrm, nd.factor, d_span + ranges[i - g0].a, hits[i].span_len, zone))) {
                return rc;
            }
        }
        // (every group has its own rows of the table)
        if ((rc = hit_table_put(c, descs.data() + g0, sizeof(SigDesc) * g0, sizeof(SigDesc) * ng))) return rc;
        const SigDesc* d_tab = static_cast<const SigDesc*>(c->hit_tab.p) + g0;
        {
            ProfScope ps(c, KN_OTHER, c->stream);
            AM_HIP(launch_hit_significance(c->stream, d_tab, (long long)ng, max_slices, d_scores, static_cast<double*>(c->sig_psum.p),
                                           static_cast<unsigned*>(c->sig_pmax.p), static_cast<double*>(c->sig_mean.p) + g0,
                                           static_cast<unsigned*>(c->sig_hmax.p) + 3 * g0,
                                           static_cast<am_significance*>(c->hit_out.p) + g0));
        }
        g0 = g1;
    }
    const void* res = nullptr;
    if ((rc = hit_results_get(c, tab_bytes, out_bytes, &res))) return rc;
    for (size_t i = 0; i < n; ++i) *out[i] = static_cast<const am_significance*>(res)[i];
    return AM_OK;
}

// am_hit_significance*: a hit at t reads its zone's span [max(0, t - B), min(len - S, t + B) + S)
struct SigFamily {
    typedef SigHit Desc;
    typedef am_significance Rec;
    const am_significance_params* sp;
    const void* params() const { return sp; }
    size_t recs() const { return 1; }
    int check_call() const { return sig_check_params(sp); }
    int check(const am_needle*, long long) const { return AM_OK; }
    double floor(const am_needle*) const { return 0.0; }   // (the zone's scores are am_correlate's: nothing of its own)
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double, const HitWhere& where,
             SigHit* d) const {
        HitDesc hd{};
        int rc;
        if ((rc = hit_desc(h, hay, len, sample_format, pk, 0.0, where, &hd))) return rc;
        const long long t = hd.t, s = hd.s, b = (long long)sp->radius;
        const long long lo = std::max(0ll, t - b), hi = std::min((long long)len - s, t + b);
        *d = SigHit{const_cast<am_needle*>(h), advance_src(hay, (size_t)lo), hd.kind, hi + s - lo, hi - lo + 1, t - lo,
                    (lo > t - b || hi < t + b) ? AM_HIT_CLIPPED : 0u};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const {
        const size_t b = (size_t)sp->radius;
        return HitRange{t > b ? t - b : 0, std::min(len - h->n, t + b) + h->n};
    }
    int score(Ctx* c, std::vector<SigHit>& hits, am_significance* const* out) const { return score_significance(c, hits, *sp, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_significance(const am_needle* h, const void* haystack, size_t len, int sample_format,
                        const am_peak* peaks, size_t n, const am_significance_params* sp, am_significance* out) {
    return hit_call(SigFamily{sp}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_significance_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                               const am_peak* peaks, size_t n, const am_significance_params* sp, am_significance* out) {
    return hit_call(SigFamily{sp}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_significance_batch_device(const am_needle* const* needles, size_t n_needles,
                                     const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                     const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                     const am_significance_params* sp, am_significance* out) {
    return hit_call_batch(SigFamily{sp}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

}  // extern "C"
