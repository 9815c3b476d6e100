// am_channel.hip -- per-hit channel estimation (am_hit_channel*, am_channel_solve, am_hit_residual; include/audiomatch.h):
// for a hit at t, the needle n[0 .. S) and P = radius, in f64,
//   c[l] = sum_{i<S} x[t + l + i] n[i] (l = -P .. P),   r[k] = sum_{i>=k} n[i] n[i - k] (k = 0 .. 2P),   E_w, E_x
// (x = 0 outside the haystack), on the device; the Toeplitz solve T h = c and the record on the host.
//
// Two kernels on the context's stream:
//   lag_slices    one workgroup of 256 per (slice of kHitSlice needle samples, tile of kLagTile lags, item).  It stages x
//                 over the slice plus 31 samples in LDS once, as f32, at index pad16(q) (stage_load): work item w takes
//                 the 16 consecutive needle samples 16 w .. 16 w + 15 (in registers) and reads the 47 staged samples its 32
//                 lags reach into registers, once (lag_dot) -- 47 LDS reads for 512 products, where the strided form of
//                 seg_slices reads one sample per product.  The tile's 32 sums stay in 32 f64 accumulators; they are added
//                 over the workgroup by wave_sums and add_waves and leave as one 64-bit store per lane.
//                 The tile that holds lag 0 adds E_w and E_x from the same staged samples; the head
//                 [t - P, t) is attached to slice 0 and the tail [t + S, t + S + P) to the last slice, one sample per work
//                 item (the order is stated in the header).  Every workgroup flags a non-finite sample among what it
//                 staged; over the tiles and slices that is exactly [t - P, t + S + P) and the needle.
//                 An item is a descriptor (LagDesc).  The hits' items use the lags -P .. P; the needle's autocorrelation
//                 is the same kernel on one more item per distinct needle of the call: the needle as both signals, t = 0,
//                 len = S, lags 0 .. 2P.
//   lag_combine   one wave per item: adds the partials (sum_slices) and writes the item's sums record (the lags' sums,
//                 E_w, E_x, the flag).
// The sums go down through the frame's pinned hit_io; the host solves and fills the records and the taps.  The partial
// records grow with items x slices x tiles: a call runs its items in rounds that hold at most kChanRoundBytes of them (one
// item at the least).  A hit's record depends on the needle, the samples it reads, P, noise_db and the floor only; the
// three forms run in the frame of am_hits.hip (am_internal.h: hit_call, hit_call_batch) and agree bit for bit.
#include <cmath>

#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kChanThreads = 256;
constexpr int kLagPer = kHitSlice / kChanThreads;     // consecutive needle samples per work item
constexpr int kLagStaged = kHitSlice + kLagTile - 1;  // staged samples of a slice
constexpr int kLagNV = kLagTile + 2;                  // values a workgroup reduces: the tile's sums, E_w, E_x
static_assert(kLagPer == 16, "pad16: the LDS layout pads one word per 16 samples");
static_assert(kLagTile <= 32 && kLagNV + 1 <= kChanThreads && AM_CHAN_MAX_RADIUS <= kChanThreads,
              "one head and one tail sample, one record value per work item");

template <int KIND>
__global__ __launch_bounds__(kChanThreads, 2) void lag_slices_kernel(const LagDesc* __restrict__ items, long long g0, int nt,
                                                                    double* __restrict__ parts, unsigned* __restrict__ pflags) {
    __shared__ float xs[kLagStaged + (kLagStaged >> 4) + 1];
    __shared__ double ws[kLagNV][kChanThreads / 64];
    const LagDesc d = items[g0 + blockIdx.z];
    const long long i0 = (long long)blockIdx.x * kHitSlice;
    if (i0 >= d.s) return;   // (a shorter needle than the launch's longest: whole workgroups leave together)
    const int tid = threadIdx.x, tile = blockIdx.y;
    const int cnt = (int)min((long long)kHitSlice, d.s - i0);
    const int lag0 = d.lag0 + tile * kLagTile;
    const int ztile = -d.lag0 / kLagTile, zoff = -d.lag0 - ztile * kLagTile;   // the tile that holds lag 0, and where in it
    const bool energies = tile == ztile;
    const bool last = i0 + cnt == d.s;
    // every load of the slice in flight at once: xs[pad16(q)] = x[t + i0 + lag0 + q] (stage_load, stage_store); the work
    // item's needle samples; its head and tail sample
    float xv[kLagPer], nv[kLagPer], xt;
    stage_load<KIND, kChanThreads>(d.win, i0 + lag0, cnt, kLagTile - 1, d.ulo, d.uhi, xv, xt);
    gfloat* nd = (gfloat*)d.needle + (i0 + tid * kLagPer);
#pragma unroll
    for (int j = 0; j < kLagPer; ++j) nv[j] = tid * kLagPer + j < cnt ? nd[j] : 0.0f;
    float xh = 0.0f, xl = 0.0f;
    if (energies && tid < d.head) {
        const long long uh = (long long)tid - d.head, ul = d.s + tid;
        if (blockIdx.x == 0 && uh >= d.ulo) xh = hit_sample<KIND>(d.win, uh);
        if (last && ul < d.uhi) xl = hit_sample<KIND>(d.win, ul);
    }
    bool bad = !__builtin_isfinite(xh) || !__builtin_isfinite(xl);
    stage_store<kChanThreads>(StagePad16{}, xs, kLagTile - 1, xv, xt, [&](int, float x) { bad |= !__builtin_isfinite(x); });
#pragma unroll
    for (int k = 0; k < kLagPer; ++k) bad |= !__builtin_isfinite(nv[k]);
    __syncthreads();
    double acc[kLagNV];   // the tile's c, then E_w and E_x
#pragma unroll
    for (int k = 0; k < kLagNV; ++k) acc[k] = 0.0;
    const int q0 = tid * kLagPer;
    if (q0 < cnt) {
        lag_dot<kLagTile>(xs, nv, q0, acc);
        if (energies) {
            double e = 0.0;
#pragma unroll
            for (int j = 0; j < kLagPer; ++j) {
                const double dx = q0 + j < cnt ? (double)xs[pad16(q0 + j + zoff)] : 0.0;
                e += dx * dx;
            }
            acc[kLagTile] = e;
        }
    }
    if (energies) {
        double e = acc[kLagTile];
        e += (double)xh * (double)xh;
        e += (double)xl * (double)xl;
        acc[kLagTile + 1] = e;
    }
    wave_sums<kChanThreads>(acc, ws);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    // one 64-bit store per lane: no record leaves as one wide store (tools/check_store_hazard.py)
    const long long p = d.part0 + blockIdx.x;
    double* rec = parts + (long long)lag_record_len(nt) * p;
    if (tid < kLagTile || (energies && tid < kLagNV))
        rec[tid < kLagTile ? tile * kLagTile + tid : nt * kLagTile + (tid - kLagTile)] = add_waves<kChanThreads>(ws[tid]);
    else if (tid == kLagNV) pflags[p * nt + tile] = (unsigned)any_bad;
}

// One wave per item: lane k adds value k (and k + 64, ...) of the item's partial records (sum_slices).
__global__ __launch_bounds__(64) void lag_combine_kernel(const LagDesc* __restrict__ items, int nt, int nlag_max,
                                                         const double* __restrict__ parts, const unsigned* __restrict__ pflags,
                                                         double* __restrict__ sums) {
    const LagDesc d = items[blockIdx.x];
    const int lane = threadIdx.x, nv = lag_record_len(nt);
    const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
    double* o = sums + (long long)lag_sums_len(nlag_max) * blockIdx.x;
    for (int k = lane; k < d.nlag + 2; k += 64) {
        const int col = k < d.nlag ? k : nt * kLagTile + (k - d.nlag);
        o[k < d.nlag ? k : nlag_max + (k - d.nlag)] = sum_slices(parts, nv, d.part0, ns, col);
    }
    const int bad = __syncthreads_or(or_flags(pflags, d.part0 * nt, ns * nt, lane, 64) != 0 ? 1 : 0);
    if (lane == 0) o[nlag_max + 2] = bad ? 1.0 : 0.0;
}

}  // namespace

hipError_t launch_lag_slices(hipStream_t st, const LagDesc* tab, long long first, long long n, int nt, int max_nsl, int kind, double* parts,
                             unsigned* pflags) {
    return for_each_grid_y(n, [&](long long g0, unsigned ng) {   // (the items are grid.z here; its limit is grid.y's)
        const dim3 grid((unsigned)max_nsl, (unsigned)nt, ng);
        if (kind) hipLaunchKernelGGL(lag_slices_kernel<1>, grid, dim3(kChanThreads), 0, st, tab, first + g0, nt, parts, pflags);
        else hipLaunchKernelGGL(lag_slices_kernel<0>, grid, dim3(kChanThreads), 0, st, tab, first + g0, nt, parts, pflags);
    });
}

hipError_t launch_lag_combine(hipStream_t st, const LagDesc* tab, long long n, int nt, int nlag_max, const double* parts,
                              const unsigned* pflags, double* sums) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lag_combine_kernel, dim3((unsigned)n), dim3(64), 0, st, tab, nt, nlag_max, parts, pflags, sums);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

// The recursion of the header.  n = 2P + 1; t0 = r[0] (1 + lambda).  false: it met a prediction error <= 0, a reflection
// coefficient with |k| >= 1 or a value that is not finite.
bool levinson_solve(const double* r, double t0, const double* c, int n, double* h) {
    if (!(t0 > 0.0)) return false;
    double a[2 * AM_CHAN_MAX_RADIUS + 1], a2[2 * AM_CHAN_MAX_RADIUS + 1];
    a[0] = 1.0;
    double err = t0;
    h[0] = c[0] / t0;
    for (int m = 1; m < n; ++m) {
        double acc = r[m];
        for (int i = 1; i < m; ++i) acc += a[i] * r[m - i];
        const double k = -acc / err;
        if (!(std::fabs(k) < 1.0)) return false;
        for (int i = 1; i < m; ++i) a2[i] = a[i] + k * a[m - i];
        for (int i = 1; i < m; ++i) a[i] = a2[i];
        a[m] = k;
        err *= 1.0 - k * k;
        if (!(err > 0.0)) return false;
        double res = c[m];
        for (int i = 0; i < m; ++i) res -= r[m - i] * h[i];
        const double dlt = res / err;
        for (int i = 0; i < m; ++i) h[i] += dlt * a[m - i];
        h[m] = dlt;
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(h[i])) return false;
    return true;
}

// h (2P + 1 doubles) of r, c; *ill as am_channel_solve reports it.  The arguments are valid.
void channel_solve(const double* r, const double* c, int radius, double noise_db, double* h, int* ill) {
    const int n = 2 * radius + 1;
    const double t0 = r[0] * (1.0 + std::pow(10.0, -noise_db / 10.0));   // the white-noise correction
    *ill = 0;
    if (levinson_solve(r, t0, c, n, h)) return;
    *ill = 1;
    for (int i = 0; i < n; ++i) h[i] = 0.0;
    if (r[0] > 0.0) h[radius] = c[radius] / r[0];
}

int chan_check_noise(double noise_db) {
    if (!(noise_db >= 0.0 && noise_db <= 200.0)) return fail(AM_ERR_INVALID_ARG, "channel: noise_db must be in 0..200");
    return AM_OK;
}

// AM_ERR_INVALID_ARG unless cp is a valid request
int chan_check_params(const am_channel_params* cp) {
    if (cp->radius > AM_CHAN_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(cp->radius) + " > AM_CHAN_MAX_RADIUS (" + std::to_string(AM_CHAN_MAX_RADIUS) + ")");
    if (cp->reserved != 0) return fail(AM_ERR_INVALID_ARG, "channel: reserved must be 0");
    return chan_check_noise(cp->noise_db);
}

// One hit of a call on the host; score_channel turns it into its table entry
struct ChanHit {
    const void* win;        // sample t of the haystack, on the device by the time score_channel runs
    const am_needle* h;
    long long t, left;      // the hit's start, len - t
    double floor_ratio;
    int kind;
};

// The record and the taps of one hit from its sums (c[-P .. P], E_w, E_x, flag) and its needle's (r[0 .. 2P], .., flag)
void chan_record(const double* sc, const double* sr, int radius, double noise_db, double ratio, am_channel_hit* rec, float* taps) {
    const int n = 2 * radius + 1;
    const double* c = sc;
    const double ew = sc[n], ex = sc[n + 1], en = sr[0];
    const float nanf = std::nanf("");
    am_channel_hit o{};
    if (sc[n + 2] != 0.0 || sr[n + 2] != 0.0) {
        o.ncc = o.ncc_eq = o.gain_db = o.residual_db = o.main_share = nanf;
        o.flags = AM_HIT_NONFINITE;
        for (int i = 0; i < n; ++i) taps[i] = nanf;
        *rec = o;
        return;
    }
    if (en == 0.0) {
        o.gain_db = nanf;
        o.residual_db = ex > 0.0 ? 0.0f : nanf;
        o.flags = AM_HIT_EMPTY_SEGMENT;
        for (int i = 0; i < n; ++i) taps[i] = 0.0f;
        *rec = o;
        return;
    }
    double h[2 * AM_CHAN_MAX_RADIUS + 1];
    int ill = 0;
    channel_solve(sr, c, radius, noise_db, h, &ill);
    if (ill) o.flags |= AM_HIT_ILL_CONDITIONED;
    double hc = 0.0, q = 0.0, hh = 0.0;
    for (int a = 0; a < n; ++a) hc += h[a] * c[a];
    for (int a = 0; a < n; ++a) {
        double row = 0.0;
        for (int b = 0; b < n; ++b) row += sr[a > b ? a - b : b - a] * h[b];
        q += h[a] * row;
    }
    for (int a = 0; a < n; ++a) hh += h[a] * h[a];
    if (ew == 0.0 || ew < en * ratio) o.flags |= AM_HIT_BELOW_FLOOR;
    else o.ncc = (float)(c[radius] / std::sqrt(en * ew));
    if (ex == 0.0 || !(q > 0.0) || ex < en * ratio) o.flags |= AM_HIT_BELOW_FLOOR;
    else o.ncc_eq = (float)(hc / std::sqrt(ex * q));
    o.gain_db = q > 0.0 ? (float)(10.0 * std::log10(q / en)) : -INFINITY;
    if (ex == 0.0) {
        o.residual_db = nanf;
    } else {
        const double num = std::max(ex - 2.0 * hc + q, 0.0);
        o.residual_db = num == 0.0 ? -INFINITY : (float)(10.0 * std::log10(num / ex));
    }
    int best = 0;   // ties: the smaller |l|, then the negative l
    for (int k = 1; k <= radius; ++k) {
        if (std::fabs(h[radius - k]) > std::fabs(h[radius + best])) best = -k;
        if (std::fabs(h[radius + k]) > std::fabs(h[radius + best])) best = k;
    }
    o.main_tap = best;
    o.main_share = hh > 0.0 ? (float)(h[radius + best] * h[radius + best] / hh) : 0.0f;
    for (int i = 0; i < n; ++i) taps[i] = (float)h[i];
    *rec = o;
}

// Every hit of `hits`; out[i]: host destination of hit i's record, its taps at taps + (out[i] - out0) (2P + 1)
int score_channel(Ctx* c, std::vector<ChanHit>& hits, const am_channel_params& cp, am_channel_hit* const* out, const am_channel_hit* out0,
                  float* taps) {
    const int radius = (int)cp.radius, nlag = 2 * radius + 1, nt = lag_tiles(nlag), nv = lag_record_len(nt), ns = lag_sums_len(nlag);
    // the needles of the call, in the order they first appear: one autocorrelation item each, in front of the hits' items
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
    const size_t nn = needles.size(), n_items = nn + hits.size();
    auto needle_at = [&](size_t g) { return g < nn ? needles[g] : hits[g - nn].h; };
    auto slices = [&](size_t g) { return ((size_t)needle_at(g)->n + kHitSlice - 1) / kHitSlice; };
    // Rounds of consecutive items, one at the least: a round's partial records stay within kChanRoundBytes
    const size_t round_parts = kChanRoundBytes / (sizeof(double) * (size_t)nv);
    std::vector<size_t> round_end;
    size_t max_items = 0, max_parts = 0;
    {
        size_t first = 0, acc = 0;
        for (size_t g = 0; g < n_items; ++g) {
            const size_t np = slices(g);
            if (g > first && acc + np > round_parts) {
                round_end.push_back(g);
                first = g;
                acc = 0;
            }
            acc += np;
            max_items = std::max(max_items, g + 1 - first);
            max_parts = std::max(max_parts, acc);
        }
        round_end.push_back(n_items);
    }
    int rc;
    const size_t tab_bytes = sizeof(LagDesc) * max_items, sums_bytes = sizeof(double) * (size_t)ns;
    if ((rc = hit_io_reserve(c, tab_bytes, sums_bytes * max_items)) || (rc = c->hit_parts.ensure(sizeof(double) * (size_t)nv * max_parts)) ||
        (rc = c->hit_flags.ensure(sizeof(unsigned) * (size_t)nt * max_parts)))
        return rc;
    std::vector<double> rsums(nn * (size_t)ns);   // the needles' sums records: r[0 .. 2P], .., the flag
    std::vector<LagDesc> tab;
    for (size_t first = 0, ri = 0; ri < round_end.size(); first = round_end[ri++]) {
        const size_t ni = round_end[ri] - first;
        const size_t n_needle_items = first < nn ? std::min(nn, first + ni) - first : 0;
        tab.resize(ni);
        long long total = 0;
        int max_nsl_n = 0, max_nsl_h = 0;
        for (size_t i = 0; i < ni; ++i) {
            const size_t g = first + i;
            const am_needle* nd = needle_at(g);
            const long long s = (long long)nd->n;
            const int nsl = (int)slices(g);
            if (g < nn) {
                tab[i] = LagDesc{nd->d_needle, nd->d_needle, s, 0, s, total, 0, nlag, 0, 0};
                max_nsl_n = std::max(max_nsl_n, nsl);
            } else {
                const ChanHit& w = hits[g - nn];
                tab[i] = LagDesc{w.win, nd->d_needle, s, -std::min<long long>(radius, w.t), std::min<long long>(s + radius, w.left), total,
                                 -radius, nlag, radius, 0};
                max_nsl_h = std::max(max_nsl_h, nsl);
            }
            total += nsl;
        }
        if ((rc = hit_table_put(c, tab.data(), 0, sizeof(LagDesc) * ni))) return rc;
        {
            ProfScope ps(c, KN_OTHER, c->stream);
            const LagDesc* d_tab = static_cast<const LagDesc*>(c->hit_tab.p);
            double* parts = static_cast<double*>(c->hit_parts.p);
            unsigned* pflags = static_cast<unsigned*>(c->hit_flags.p);
            if (n_needle_items) AM_HIP(launch_lag_slices(c->stream, d_tab, 0, (long long)n_needle_items, nt, max_nsl_n, 0, parts, pflags));
            if (ni > n_needle_items)
                AM_HIP(launch_lag_slices(c->stream, d_tab, (long long)n_needle_items, (long long)(ni - n_needle_items), nt, max_nsl_h, hits[0].kind,
                                         parts, pflags));
            AM_HIP(launch_lag_combine(c->stream, d_tab, (long long)ni, nt, nlag, parts, pflags, static_cast<double*>(c->hit_out.p)));
        }
        const void* res = nullptr;
        if ((rc = hit_results_get(c, tab_bytes, sums_bytes * ni, &res))) return rc;
        const double* sums = static_cast<const double*>(res);
        for (size_t i = 0; i < ni; ++i) {
            const size_t g = first + i;
            if (g < nn) {
                std::memcpy(&rsums[g * (size_t)ns], sums + i * (size_t)ns, sums_bytes);
                continue;
            }
            const ChanHit& w = hits[g - nn];
            am_channel_hit rec;
            float tp[2 * AM_CHAN_MAX_RADIUS + 1];
            chan_record(sums + i * (size_t)ns, &rsums[needle_of[g - nn] * (size_t)ns], radius, cp.noise_db, w.floor_ratio, &rec, tp);
            std::memcpy(out[g - nn], &rec, sizeof(rec));
            std::memcpy(taps + (size_t)(out[g - nn] - out0) * (size_t)nlag, tp, sizeof(float) * (size_t)nlag);
        }
    }
    return AM_OK;
}

// am_hit_channel*: a hit at t reads [t - P, t + S + P), clipped to the haystack
struct ChanFamily {
    typedef ChanHit Desc;
    typedef am_channel_hit Rec;
    const am_channel_params* cp;
    const am_channel_hit* out0;
    float* taps;
    const void* params() const { return taps ? cp : nullptr; }   // (the null check of the frame covers the taps)
    size_t recs() const { return 1; }
    int check_call() const { return chan_check_params(cp); }
    int check(const am_needle* h, long long j) const {
        if (h->n > ((size_t)1 << 31)) return fail(AM_ERR_INVALID_ARG, hit_needle_name(j) + "needle longer than 2^31 samples");
        return AM_OK;
    }
    double floor(const am_needle* h) const { return hit_floor_ratio(h); }
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double ratio, const HitWhere& where,
             ChanHit* d) const {
        HitDesc hd{};
        int rc;
        if ((rc = hit_desc(h, hay, len, sample_format, pk, 0.0, where, &hd))) return rc;
        *d = ChanHit{hd.win, h, hd.t, (long long)len - hd.t, ratio, hd.kind};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const {
        const size_t r = cp->radius;
        return HitRange{t > r ? t - r : 0, std::min(len, t + h->n + r)};
    }
    int score(Ctx* c, std::vector<ChanHit>& hits, am_channel_hit* const* out) const { return score_channel(c, hits, *cp, out, out0, taps); }
};

// the format and the parameters, before anything that needs a device
int chan_prelude(int sample_format, const am_channel_params* cp) {
    int rc;
    if ((rc = check_format(sample_format))) return rc;
    return cp ? chan_check_params(cp) : AM_OK;
}

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_channel(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_peak* peaks, size_t n,
                   const am_channel_params* cp, am_channel_hit* out, float* taps) {
    int rc;
    if ((rc = chan_prelude(sample_format, cp))) return rc;
    return hit_call(ChanFamily{cp, out, taps}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_channel_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_peak* peaks, size_t n,
                          const am_channel_params* cp, am_channel_hit* out, float* taps) {
    int rc;
    if ((rc = chan_prelude(sample_format, cp))) return rc;
    return hit_call(ChanFamily{cp, out, taps}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_channel_batch_device(const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks, const size_t* lens,
                                size_t n_hay, int sample_format, const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                                const am_channel_params* cp, am_channel_hit* out, float* taps) {
    int rc;
    if ((rc = chan_prelude(sample_format, cp))) return rc;
    return hit_call_batch(ChanFamily{cp, out, taps}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks,
                          out);
}

int am_channel_solve(const double* r, const double* c, uint32_t radius, double noise_db, double* h, int* ill) {
    if (!r || !c || !h || !ill) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (radius > AM_CHAN_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(radius) + " > AM_CHAN_MAX_RADIUS (" + std::to_string(AM_CHAN_MAX_RADIUS) + ")");
    int rc;
    if ((rc = chan_check_noise(noise_db))) return rc;
    for (uint32_t k = 0; k <= 2 * radius; ++k) {
        if (!std::isfinite(r[k])) return fail(AM_ERR_INVALID_ARG, "channel: r[" + std::to_string(k) + "] is not finite");
        if (!std::isfinite(c[k])) return fail(AM_ERR_INVALID_ARG, "channel: c[" + std::to_string((long long)k - (long long)radius) + "] is not finite");
    }
    channel_solve(r, c, (int)radius, noise_db, h, ill);
    return AM_OK;
}

int am_hit_residual(const void* haystack, size_t len, int sample_format, uint64_t start, const float* needle, size_t s, const float* taps,
                    uint32_t radius, float* model, float* resid) {
    int rc;
    if ((rc = check_format(sample_format))) return rc;
    if (!needle || !taps || (!haystack && len > 0)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (s == 0) return fail(AM_ERR_INVALID_ARG, "residual: the needle must hold at least 1 sample");
    if (radius > AM_CHAN_MAX_RADIUS)
        return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(radius) + " > AM_CHAN_MAX_RADIUS (" + std::to_string(AM_CHAN_MAX_RADIUS) + ")");
    const uint64_t top = (uint64_t)1 << 62;
    if (start >= top || (uint64_t)s >= top) return fail(AM_ERR_INVALID_ARG, "residual: start and s must be below 2^62");
    const float* f = static_cast<const float*>(haystack);
    const int16_t* s16 = static_cast<const int16_t*>(haystack);
    const float nan = std::nanf("");
    const long long p = radius, ss = (long long)s;
    for (long long u = 0; u < ss + 2 * p; ++u) {
        double acc = 0.0;
        for (long long l = -p; l <= p; ++l) {
            const long long i = u - p - l;
            if (i >= 0 && i < ss) acc += (double)taps[l + p] * (double)needle[i];
        }
        const float m = (float)acc;
        if (model) model[u] = m;
        if (!resid) continue;
        float v = nan;
        if ((uint64_t)u + start >= (uint64_t)p && (uint64_t)u + start - (uint64_t)p < len) {
            const uint64_t e = (uint64_t)u + start - (uint64_t)p;
            const float x = sample_format == AM_FMT_S16_STEREO ? (float)((int)s16[2 * e] + (int)s16[2 * e + 1]) * (0.5f * (1.0f / 65535.0f)) : f[e];
            if (std::isfinite(x)) v = x - m;
        }
        resid[u] = v;
    }
    return AM_OK;
}

}  // extern "C"
