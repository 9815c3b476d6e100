// am_warp.hip -- per-hit drift scoring (am_hit_warp*, am_warp_table, am_hit_window_warped; include/audiomatch.h): the
// pass of am_segments.hip with m = 1, run once per drift of a grid against the needle resampled to that drift.  For a hit
// at t, the Q = 2 K + 1 warped needles n_q (lengths S_q) and the lags l = -R .. R, in f64:
//   c(q,l) = sum_j x[t + l + j] n_q[j],   E_w(q,l) = sum_j x[t + l + j]^2,   E_n(q) = sum_j n_q[j]^2
// (x = 0 outside the haystack) and from those the best cell, its two parabola vertices and the NCC, gain and level there.
//
// Three kernels on the context's stream:
//   warp_needle    one thread per (needle, rate, j): the 32-tap f64 chain of the header over the needle, rounded to f32
//                  once, into the context's scratch (warp_needles); once per round and needle, not per hit.  The table
//                  h[phase][tap] lives in device memory, built on first use and kept until am_shutdown.
//   seg_slices     am_segments.hip's slice kernel, unchanged, over a table with one entry per (hit, rate): the entry's
//                  needle pointer and length are the warped needle's.  Its records carry E_n(q) as well, summed in the
//                  same slice order as c and E_w.
//   warp_combine   one workgroup per hit: adds each rate's partials (the loop of sum_slices), forms the Q x (2 R + 1)
//                  cells (ncc_or_floor), and one thread applies the tie rule, the two vertices (parabola_vertex,
//                  refine_lag) and the flags.  (A workgroup of four waves, not one wave: a hit has up to 65 x 67 sums of
//                  up to S / 4096 partials each, and the sums are what takes time.)
// The partial records grow with hits x Q x slices and the warped needles with needles x Q x S: a call runs its hits in
// rounds that hold at most kWarpRoundBytes of each (one hit and its needle at the least).
// A hit's record depends on the needle, the samples it reads, the parameters and the floor only; the three forms run in
// the frame of am_hits.hip (am_internal.h: hit_call, hit_call_batch) and agree bit for bit.
#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kWarpHalf = AM_WARP_TAPS / 2 - 1;   // tap k reads sample m - kWarpHalf + k
constexpr double kTwo32 = 4294967296.0;

__global__ __launch_bounds__(kWarpThreads) void warp_needle_kernel(const WarpJob* __restrict__ jobs, int job0,
                                                                   const float* __restrict__ table) {
    const WarpJob jb = jobs[job0 + blockIdx.y];
    const long long j = (long long)blockIdx.x * kWarpThreads + threadIdx.x;
    if (j >= jb.s_q) return;
    const unsigned long long u = (unsigned long long)j * jb.inc + (1ull << 19);
    const long long m = (long long)(u >> 32);
    const unsigned p = (unsigned)(u >> 20) & (AM_WARP_PHASES - 1);
    float v;
    if (p == 0) {   // the delta: the sample itself
        v = m < jb.s ? jb.needle[m] : 0.0f;
    } else {
        const float* hr = table + (size_t)p * AM_WARP_TAPS;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < AM_WARP_TAPS; ++k) {
            const long long i = m - kWarpHalf + k;
            const float x = i >= 0 && i < jb.s ? jb.needle[i] : 0.0f;
            acc += (double)hr[k] * (double)x;   // (a product of two f32 values is exact in f64)
        }
        v = (float)acc;
    }
    jb.out[j] = v;
}

// One workgroup per hit.  sh: the sums of every rate's record (nq x nv), then the cells' ncc (nq x (2 r + 1)).
__global__ __launch_bounds__(kWarpCombineThreads) void warp_combine_kernel(const SegDesc* __restrict__ tab, const WarpGrid g, int rt,
                                                                           const double* __restrict__ parts,
                                                                           const unsigned* __restrict__ pflags,
                                                                           am_warp_hit* __restrict__ out) {
    extern __shared__ double sh[];
    const int kk = g.k, r = g.r, nq = 2 * kk + 1, nl = 2 * rt + 1, nv = 2 * nl + 1, nc = 2 * r + 1;
    double* sums = sh;
    double* cell = sh + nq * nv;
    const SegDesc* hd = tab + (long long)blockIdx.x * nq;
    const int tid = threadIdx.x;
    for (int it = tid; it < nq * nv; it += kWarpCombineThreads) {
        const int q = it / nv, k = it - q * nv;
        const long long ns = (hd[q].s + kHitSlice - 1) / kHitSlice, p0 = hd[q].part0;
        double t = 0.0;   // (sum_slices<4>, written out: through the helper this kernel takes two more VGPRs)
#pragma unroll 4
        for (long long i = 0; i < ns; ++i) t += parts[nv * (p0 + i) + k];
        sums[it] = t;
    }
    unsigned b = 0;
    for (int q = 0; q < nq; ++q) b |= or_flags(pflags, hd[q].part0, (hd[q].s + kHitSlice - 1) / kHitSlice, tid, kWarpCombineThreads);
    const int bad = __syncthreads_or(b != 0 ? 1 : 0);   // (and the sums are visible)
    const double ratio = hd[0].floor_ratio;
    for (int it = tid; it < nq * nc; it += kWarpCombineThreads) {
        const int q = it / nc, l = it - q * nc - r;
        const double* s = sums + q * nv;
        const double c = s[rt + l], ew = s[nl + rt + l], en = s[2 * nl];
        bool below;   // (the cell is 0 either way; the flag is the best cell's, below)
        cell[it] = en == 0.0 ? 0.0 : ncc_or_floor(c, en, ew, en * ratio, &below);
    }
    __syncthreads();
    if (tid != 0) return;
    am_warp_hit* o = out + blockIdx.x;
    const double nan = __builtin_nan("");
    if (bad) {
        o->drift_ppm = g.centre_ppm;
        o->lag = 0.0;
        o->ncc = o->gain = o->level_db = o->ncc_centre = (float)nan;
        o->length = 0;   // (the host writes S)
        o->flags = AM_HIT_NONFINITE;
        return;
    }
    // the best cell; candidates in the order of the tie rule, replaced by a strictly larger one only
    int qs = kk, ls = 0;
    double best = cell[kk * nc + r];
    for (int dq = 0; dq <= kk; ++dq)
        for (int sq = 0; sq < (dq ? 2 : 1); ++sq) {
            const int q = sq ? kk + dq : kk - dq;
            for (int dl = 0; dl <= r; ++dl)
                for (int sl = 0; sl < (dl ? 2 : 1); ++sl) {
                    const int l = sl ? dl : -dl;
                    const double v = cell[q * nc + r + l];
                    if (v > best) { best = v; qs = q; ls = l; }
                }
        }
    const double* s = sums + qs * nv;
    const double* cc = s + rt;
    const double bb = cc[ls], ew = s[nl + rt + ls], en = s[2 * nl];
    double drift = g.d[qs], lag = (double)ls;
    unsigned flags = 0;
    float ncc, gain, ldb;
    if (en == 0.0) {
        flags = AM_HIT_EMPTY_SEGMENT;
        lag = 0.0;
        ncc = gain = 0.0f;
        ldb = ew > 0.0 ? __builtin_inff() : (float)nan;
    } else {
        bool refined = false;
        double v = 0.0;
        if (kk != 0 && qs != 0 && qs != 2 * kk) v = parabola_vertex(cell[(qs - 1) * nc + r + ls], best, cell[(qs + 1) * nc + r + ls], &refined);
        if (!refined) flags |= AM_HIT_DRIFT_UNREFINED;
        else drift += v * g.step_ppm;
        lag = refine_lag<false>(cc, r, ls, &refined);
        if (!refined) flags |= AM_HIT_UNREFINED;
        if (ew == 0.0 || ew < en * ratio) flags |= AM_HIT_BELOW_FLOOR;
        ncc = (float)best;
        gain = (float)(bb / en);
        ldb = level_db(ew, en);
    }
    o->drift_ppm = drift;
    o->lag = lag;
    o->ncc = ncc;
    o->gain = gain;
    o->level_db = ldb;
    o->ncc_centre = (float)cell[kk * nc + r];
    o->length = (unsigned)hd[qs].s;
    o->flags = flags;
}

}  // namespace

hipError_t launch_warp_needles(hipStream_t st, const WarpJob* d_jobs, int n_jobs, long long max_len, const float* table) {
    if (n_jobs <= 0 || max_len <= 0) return hipSuccess;
    const unsigned gx = (unsigned)((max_len + kWarpThreads - 1) / kWarpThreads);
    return for_each_grid_y(n_jobs, [&](long long j0, unsigned nj) {
        hipLaunchKernelGGL(warp_needle_kernel, dim3(gx, nj), dim3(kWarpThreads), 0, st, d_jobs, (int)j0, table);
    });
}

hipError_t launch_warp_combine(hipStream_t st, const SegDesc* tab, long long n, const WarpGrid& grid, const double* parts,
                               const unsigned* pflags, am_warp_hit* d_out) {
    if (n <= 0) return hipSuccess;
    const int rt = seg_kernel_radius(grid.r), nq = 2 * grid.k + 1;
    const size_t lds = sizeof(double) * (size_t)nq * (size_t)(seg_record_len(rt) + 2 * grid.r + 1);
    hipLaunchKernelGGL(warp_combine_kernel, dim3((unsigned)n), dim3(kWarpCombineThreads), lds, st, tab, grid, rt, parts, pflags, d_out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

constexpr double kPi = 3.14159265358979323846;

double bessel_i0(double z) {   // the power series: sum ((z / 2)^k / k!)^2
    const double q = 0.25 * z * z;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// the interpolator's table, computed once per process
const std::vector<float>& warp_table_host() {
    static std::vector<float> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<float> t((size_t)AM_WARP_PHASES * AM_WARP_TAPS, 0.0f);
        t[kWarpHalf] = 1.0f;   // row 0: the delta, by definition
        const double i0b = bessel_i0(8.0), half = AM_WARP_TAPS / 2;
        for (int p = 1; p < AM_WARP_PHASES; ++p) {
            double v[AM_WARP_TAPS], sum = 0.0;
            for (int k = 0; k < AM_WARP_TAPS; ++k) {
                const double x = (double)(k - kWarpHalf) - (double)p / AM_WARP_PHASES, y = x / half;
                const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
                v[k] = sinc * bessel_i0(8.0 * std::sqrt(std::max(0.0, 1.0 - y * y))) / i0b;
                sum += v[k];
            }
            for (int k = 0; k < AM_WARP_TAPS; ++k) t[(size_t)p * AM_WARP_TAPS + k] = (float)(v[k] / sum);
        }
        tab.swap(t);
    });
    return tab;
}

// ... and on c's device, built on first use and kept until am_shutdown
int warp_table_device(Ctx* c, const float** d_tab) {
    DevBuf& b = c->warp_tab;
    if (b.p) { *d_tab = static_cast<const float*>(b.p); return AM_OK; }
    const std::vector<float>& t = warp_table_host();
    int rc;
    if ((rc = b.ensure(sizeof(float) * t.size()))) return rc;
    hipError_t e = hipMemcpyAsync(b.p, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { b.release(); return hip_fail(e, "hipMemcpy(warp table)"); }
    *d_tab = static_cast<const float*>(b.p);
    return AM_OK;
}

double warp_drift(const am_warp_params& wp, int q) {   // d_q
    const int k = (int)wp.steps;
    return k == 0 ? wp.centre_ppm : wp.centre_ppm + wp.max_ppm * (double)(q - k) / (double)k;
}
unsigned long long warp_inc(double d_ppm) { return (unsigned long long)std::llround(kTwo32 / (1.0 + d_ppm * 1e-6)); }
long long warp_len(long long s, unsigned long long inc) {   // S_d
    return (long long)((((unsigned __int128)(s - 1)) << 32) / inc) + 1;
}

// AM_ERR_INVALID_ARG unless wp is a valid request
int warp_check_params(const am_warp_params* wp) {
    if (wp->steps > AM_WARP_MAX_STEPS)
        return fail(AM_ERR_INVALID_ARG, "steps " + std::to_string(wp->steps) + " > AM_WARP_MAX_STEPS (" + std::to_string(AM_WARP_MAX_STEPS) + ")");
    if (wp->radius > AM_SEG_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(wp->radius) + " > AM_SEG_MAX_RADIUS (" + std::to_string(AM_SEG_MAX_RADIUS) + ")");
    if (!std::isfinite(wp->max_ppm) || wp->max_ppm < 0.0) return fail(AM_ERR_INVALID_ARG, "max_ppm " + std::to_string(wp->max_ppm) + " < 0 or not finite");
    if (wp->steps > 0 && wp->max_ppm == 0.0) return fail(AM_ERR_INVALID_ARG, "max_ppm = 0 with steps > 0");
    if (!std::isfinite(wp->centre_ppm) || std::fabs(wp->centre_ppm) + wp->max_ppm > (double)AM_WARP_MAX_PPM)
        return fail(AM_ERR_INVALID_ARG, "|centre_ppm| + max_ppm = " + std::to_string(std::fabs(wp->centre_ppm) + wp->max_ppm) +
                                            " > AM_WARP_MAX_PPM (" + std::to_string(AM_WARP_MAX_PPM) + ")");
    return AM_OK;
}

// One hit of a call on the host; score_warp turns it into its 2 K + 1 table entries
struct WarpHit {
    const void* win;        // sample t of the haystack, on the device by the time score_warp runs
    const am_needle* h;
    long long t, left;      // the hit's start, len - t
    double floor_ratio;
    int kind;
};

int score_warp(Ctx* c, std::vector<WarpHit>& hits, const am_warp_params& wp, am_warp_hit* const* out) {
    const int kk = (int)wp.steps, nq = 2 * kk + 1, r = (int)wp.radius, nv = seg_record_len(seg_kernel_radius(r));
    WarpGrid g{};
    g.centre_ppm = wp.centre_ppm;
    g.step_ppm = kk ? wp.max_ppm / (double)kk : 0.0;
    g.k = kk;
    g.r = r;
    for (int q = 0; q < nq; ++q) g.d[q] = warp_drift(wp, q);
    // the needles of the call, in the order they first appear, and the shapes of their warped forms
    struct Shape { unsigned long long inc; long long s_q; };
    std::vector<const am_needle*> needles;
    std::vector<size_t> needle_of(hits.size());
    std::map<const am_needle*, size_t> seen;
    for (size_t i = 0; i < hits.size(); ++i) {
        auto it = seen.find(hits[i].h);
        if (it == seen.end()) {
            it = seen.emplace(hits[i].h, needles.size()).first;
            needles.push_back(hits[i].h);
        }
        needle_of[i] = it->second;
    }
    std::vector<Shape> shape(needles.size() * (size_t)nq);
    std::vector<size_t> hit_parts(needles.size(), 0), floats(needles.size(), 0);   // partial records of one hit, warped samples, per needle
    long long max_len = 0;
    for (size_t a = 0; a < needles.size(); ++a)
        for (int q = 0; q < nq; ++q) {
            Shape& sh = shape[a * nq + q];
            sh.inc = warp_inc(g.d[q]);
            sh.s_q = warp_len((long long)needles[a]->n, sh.inc);
            floats[a] += (size_t)sh.s_q;
            max_len = std::max(max_len, sh.s_q);
            hit_parts[a] += (size_t)((sh.s_q + kHitSlice - 1) / kHitSlice);
        }
    // Rounds of consecutive hits, one hit at the least: a round's partial records, and the warped forms of the needles
    // its hits use, each stay within kWarpRoundBytes (unless one hit or one needle alone is larger).  Consecutive rounds with
    // the same needles warp them once; otherwise a needle whose hits fall into several rounds is warped in each of them.
    const size_t round_parts = kWarpRoundBytes / (sizeof(double) * (size_t)nv), round_floats = kWarpRoundBytes / sizeof(float);
    std::vector<size_t> round_end;
    size_t max_hits = 0, max_parts = 0, max_floats = 0, max_needles = 0;
    {
        std::vector<char> in_round(needles.size(), 0);
        size_t first = 0, acc = 0, accf = 0, nn = 0;
        for (size_t i = 0; i < hits.size(); ++i) {
            const size_t a = needle_of[i], np = hit_parts[a], nf = in_round[a] ? 0 : floats[a];
            if (i > first && (acc + np > round_parts || (nf > 0 && accf + nf > round_floats))) {
                round_end.push_back(i);
                first = i;
                acc = accf = nn = 0;
                std::fill(in_round.begin(), in_round.end(), 0);
            }
            if (!in_round[a]) { in_round[a] = 1; accf += floats[a]; ++nn; }
            acc += np;
            max_hits = std::max(max_hits, i + 1 - first);
            max_parts = std::max(max_parts, acc);
            max_floats = std::max(max_floats, accf);
            max_needles = std::max(max_needles, nn);
        }
        round_end.push_back(hits.size());
    }
    int rc;
    const float* d_table = nullptr;
    const size_t jobs_bytes = (sizeof(WarpJob) * max_needles * (size_t)nq + 63) / 64 * 64;
    const size_t tab_bytes = jobs_bytes + sizeof(SegDesc) * (size_t)nq * max_hits;
    if ((rc = warp_table_device(c, &d_table)) || (rc = c->warp_needles.ensure(sizeof(float) * max_floats)) ||
        (rc = hit_io_reserve(c, tab_bytes, sizeof(am_warp_hit) * max_hits)) || (rc = c->hit_parts.ensure(sizeof(double) * (size_t)nv * max_parts)) ||
        (rc = c->hit_flags.ensure(sizeof(unsigned) * max_parts)))
        return rc;
    const SegDesc* d_tab = reinterpret_cast<const SegDesc*>(static_cast<const char*>(c->hit_tab.p) + jobs_bytes);
    std::vector<SegDesc> tab;
    std::vector<WarpJob> jobs;
    std::vector<size_t> job_of(needles.size());   // first job of a needle in this round
    const size_t none = (size_t)-1;
    std::vector<size_t> cur, resident;            // the needles of this round, and those whose warped forms the scratch holds
    std::vector<char> in_cur(needles.size(), 0);
    for (size_t first = 0, ri = 0; ri < round_end.size(); first = round_end[ri++]) {
        const size_t nh = round_end[ri] - first;
        // the round's needles, in the order they first appear: their jobs, the warped forms one after the other in
        // c->warp_needles.  A round with the needles of the round before it (the many hits of one needle) finds them there.
        cur.clear();
        std::fill(in_cur.begin(), in_cur.end(), 0);
        for (size_t i = 0; i < nh; ++i) {
            const size_t a = needle_of[first + i];
            if (!in_cur[a]) { in_cur[a] = 1; cur.push_back(a); }
        }
        const bool warp = cur != resident;
        if (warp) {
            std::fill(job_of.begin(), job_of.end(), none);
            jobs.clear();
            float* next = static_cast<float*>(c->warp_needles.p);
            for (size_t a : cur) {
                job_of[a] = jobs.size();
                for (int q = 0; q < nq; ++q) {
                    const Shape& sh = shape[a * nq + q];
                    jobs.push_back(WarpJob{needles[a]->d_needle, next, (long long)needles[a]->n, sh.s_q, sh.inc});
                    next += sh.s_q;
                }
            }
            resident = cur;
        }
        tab.resize(nh * (size_t)nq);
        long long total = 0;
        int max_nsl = 0;
        for (size_t i = 0; i < nh; ++i) {
            const WarpHit& w = hits[first + i];
            for (int q = 0; q < nq; ++q) {
                const WarpJob& jb = jobs[job_of[needle_of[first + i]] + q];
                const int nsl = (int)((jb.s_q + kHitSlice - 1) / kHitSlice);
                tab[i * nq + q] = SegDesc{w.win, jb.out, jb.s_q, -std::min<long long>(r, w.t), std::min(jb.s_q + r, w.left), total,
                                          w.floor_ratio, w.kind, nsl};
                total += nsl;
                max_nsl = std::max(max_nsl, nsl);
            }
        }
        if ((warp && (rc = hit_table_put(c, jobs.data(), 0, sizeof(WarpJob) * jobs.size()))) ||
            (rc = hit_table_put(c, tab.data(), jobs_bytes, sizeof(SegDesc) * tab.size())))
            return rc;
        {
            ProfScope ps(c, KN_OTHER, c->stream);
            if (warp) AM_HIP(launch_warp_needles(c->stream, static_cast<const WarpJob*>(c->hit_tab.p), (int)jobs.size(), max_len, d_table));
            AM_HIP(launch_seg_slices(c->stream, d_tab, (long long)tab.size(), 1, r, max_nsl, hits[0].kind, static_cast<double*>(c->hit_parts.p),
                                     static_cast<unsigned*>(c->hit_flags.p)));
            AM_HIP(launch_warp_combine(c->stream, d_tab, (long long)nh, g, static_cast<const double*>(c->hit_parts.p),
                                       static_cast<const unsigned*>(c->hit_flags.p), static_cast<am_warp_hit*>(c->hit_out.p)));
        }
        const void* res = nullptr;
        if ((rc = hit_results_get(c, tab_bytes, sizeof(am_warp_hit) * nh, &res))) return rc;
        for (size_t i = 0; i < nh; ++i) {
            am_warp_hit rec = static_cast<const am_warp_hit*>(res)[i];
            if (rec.flags & AM_HIT_NONFINITE) rec.length = (uint32_t)hits[first + i].h->n;
            std::memcpy(out[first + i], &rec, sizeof(rec));
        }
    }
    return AM_OK;
}

// am_hit_warp*: a hit at t reads [t - R, t + R + max_q S_q), clipped to the haystack
struct WarpFamily {
    typedef WarpHit Desc;
    typedef am_warp_hit Rec;
    const am_warp_params* wp;
    const void* params() const { return wp; }
    size_t recs() const { return 1; }
    int check_call() const { return warp_check_params(wp); }
    int check(const am_needle* h, long long j) const {
        if (h->n > ((size_t)1 << 31)) return fail(AM_ERR_INVALID_ARG, hit_needle_name(j) + "needle longer than 2^31 samples");
        return AM_OK;
    }
    double floor(const am_needle* h) const { return hit_floor_ratio(h); }
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double ratio, const HitWhere& where,
             WarpHit* d) const {
        HitDesc hd{};
        int rc;
        if ((rc = hit_desc(h, hay, len, sample_format, pk, 0.0, where, &hd))) return rc;
        *d = WarpHit{hd.win, h, hd.t, (long long)len - hd.t, ratio, hd.kind};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const {
        const size_t r = wp->radius;
        const size_t longest = (size_t)warp_len((long long)h->n, warp_inc(warp_drift(*wp, 2 * (int)wp->steps)));   // (the largest drift of the grid)
        return HitRange{t > r ? t - r : 0, std::min(len, t + longest + r)};
    }
    int score(Ctx* c, std::vector<WarpHit>& hits, am_warp_hit* const* out) const { return score_warp(c, hits, *wp, out); }
};

// the format and the parameters, before anything that needs a device
int warp_prelude(int sample_format, const am_warp_params* wp) {
    int rc;
    if ((rc = check_format(sample_format))) return rc;
    return wp ? warp_check_params(wp) : AM_OK;
}

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_warp_table(float* out) {
    if (!out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    const std::vector<float>& t = warp_table_host();
    std::memcpy(out, t.data(), sizeof(float) * t.size());
    return AM_OK;
}

int am_hit_warp(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_peak* peaks, size_t n,
                const am_warp_params* wp, am_warp_hit* out) {
    int rc;
    if ((rc = warp_prelude(sample_format, wp))) return rc;
    return hit_call(WarpFamily{wp}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_warp_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_peak* peaks, size_t n,
                       const am_warp_params* wp, am_warp_hit* out) {
    int rc;
    if ((rc = warp_prelude(sample_format, wp))) return rc;
    return hit_call(WarpFamily{wp}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_warp_batch_device(const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks, const size_t* lens,
                             size_t n_hay, int sample_format, const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                             const am_warp_params* wp, am_warp_hit* out) {
    int rc;
    if ((rc = warp_prelude(sample_format, wp))) return rc;
    return hit_call_batch(WarpFamily{wp}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

int am_hit_window_warped(const void* haystack, size_t len, int sample_format, uint64_t start, float scale, double lag, double drift_ppm,
                         uint64_t lead, uint64_t length, float* row) {
    int rc;
    if ((rc = check_format(sample_format))) return rc;
    if (!row || (!haystack && len > 0)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (length == 0) return fail(AM_ERR_INVALID_ARG, "window: length must be at least 1");
    if (!std::isfinite(scale) || scale == 0.0f) return fail(AM_ERR_INVALID_ARG, "window: scale must be finite and not zero");
    if (!std::isfinite(lag) || std::fabs(lag) >= 1073741824.0) return fail(AM_ERR_INVALID_ARG, "window: lag must be finite and below 2^30");
    if (!std::isfinite(drift_ppm) || std::fabs(drift_ppm) > (double)AM_WARP_MAX_PPM)
        return fail(AM_ERR_INVALID_ARG, "window: |drift_ppm| > AM_WARP_MAX_PPM (" + std::to_string(AM_WARP_MAX_PPM) + ") or not finite");
    const uint64_t top = (uint64_t)1 << 62;
    if (start >= top || lead >= top || length >= top) return fail(AM_ERR_INVALID_ARG, "window: start, lead and length must be below 2^62");
    const float* tab = warp_table_host().data();
    const float* f = static_cast<const float*>(haystack);
    const int16_t* s16 = static_cast<const int16_t*>(haystack);
    auto sample = [&](uint64_t e) {
        return sample_format == AM_FMT_S16_STEREO ? (float)((int)s16[2 * e] + (int)s16[2 * e + 1]) * (0.5f * (1.0f / 65535.0f)) : f[e];
    };
    const float nan = std::nanf("");
    const __int128 base = ((__int128)start << 32) + (__int128)std::llround(lag * kTwo32) + ((__int128)1 << 19);
    const __int128 inc = (__int128)std::llround(kTwo32 * (1.0 + drift_ppm * 1e-6));
    for (uint64_t n = 0; n < length; ++n) {
        const __int128 u = base + ((__int128)n - (__int128)lead) * inc;
        const __int128 m = u >> 32;   // (floor)
        const unsigned p = (unsigned)((u >> 20) & (AM_WARP_PHASES - 1));
        float v = nan;
        if (p == 0) {
            if (m >= 0 && m < (__int128)len) {
                const float x = sample((uint64_t)m);
                if (std::isfinite(x)) v = x * scale;
            }
        } else {
            const float* hr = tab + (size_t)p * AM_WARP_TAPS;
            double acc = 0.0;
            bool present = true;
            for (int k = 0; k < AM_WARP_TAPS && present; ++k) {
                if (hr[k] == 0.0f) continue;
                const __int128 e = m - kWarpHalf + k;
                if (e < 0 || e >= (__int128)len) { present = false; break; }
                const float x = sample((uint64_t)e);
                if (!std::isfinite(x)) { present = false; break; }
                acc += (double)hr[k] * (double)x;
            }
            if (present) v = (float)acc * scale;
        }
        row[n] = std::isfinite(v) ? v : nan;
    }
    return AM_OK;
}

}  // extern "C"
