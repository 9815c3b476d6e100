// am_bands.hip -- per-band hit scoring (am_hit_bands*, include/audiomatch.h): the pass of am_hits.hip resolved along
// frequency.  For a hit at t, frames of F = 2^frame_log2 samples at hop H = F / 2 (J = floor((S - F) / H) + 1 of them),
// the Hann window w and the spectra X_j, N_j of the windowed haystack and needle frames, in f64:
//   P_xn[k] = sum_j X_j[k] conj(N_j[k]),   P_xx[k] = sum_j |X_j[k]|^2,   P_nn[k] = sum_j |N_j[k]|^2      (k = 0 .. F/2)
// summed over the bins of each band, and from those per band the NCC at lag 0, the coherence, the gain, the level and the
// band's share of the needle's energy.
//
// Two kernels on the context's stream:
//   band_frames   one workgroup per (hit, group of kBandGroup consecutive frames): per frame it loads F samples of x and
//                 of n, widens and windows them, packs z = x + i n, runs ONE F-point complex f64 FFT in LDS and untangles
//                 X[k] and N[k] (am_frames.h), and adds the three products to the thread's bins (registers).  After the group's frames the bins go
//                 through LDS to one sum per band and value, in a fixed order, and the workgroup writes one partial
//                 record: (Re C, Im C, E_x, E_n) per band and E_n over every bin, one 64-bit store per lane.
//   band_combine  one wave per hit: adds the hit's partials in group order, forms the B records and sets the flags.
// Window and twiddles come from a table built on the host in f64, once per (device, F): the kernels compute no
// transcendental but the final log10.  A frame whose haystack samples are all zero counts as X_j = 0 exactly (and a
// frame of needle zeros as N_j = 0): what the packed transform would leak from the other signal, 1e-32 of its power,
// never turns digital silence into a level.
// The kernels read x[t + u] for u in [0, (J - 1) H + F) and n[0 .. (J - 1) H + F) only.  A hit's records depend on the
// needle, the samples it reads, the parameters and the floor only (groups start at multiples of kBandGroup frames, every
// reduction runs in a fixed order; one kernel serves both sample formats): the single, batch and host forms agree
// bit for bit.  The three forms run in the frame of am_hits.hip (am_internal.h: hit_call, hit_call_batch,
// hit_round_trip); BandFamily below is what this family adds to it; the combine's sums are those of am_hit_device.h.
#include "am_frames.h"
#include "am_hit_device.h"

namespace am {

namespace {

constexpr int kBandThreads = kFrameThreads, kBandLds = kFrameLds, kBandBins = kFrameBins;
static_assert(AM_BAND_MAX_BANDS <= 64, "band_combine forms one record per lane");

struct BandArgs {
    am_band_params bp;
    int nrec;   // doubles per partial record: 4 B + 1
};

__global__ __launch_bounds__(kBandThreads) void band_frames_kernel(const BandDesc* __restrict__ hits, long long h0, BandArgs a,
                                                                   const double* __restrict__ tab, double* __restrict__ parts,
                                                                   unsigned* __restrict__ pflags) {
    __shared__ double sh[2 * kBandLds];
    __shared__ unsigned wbits[kBandThreads / 64];
    const BandDesc d = hits[h0 + blockIdx.y];
    if ((int)blockIdx.x >= d.ngroups) return;   // (a hit of fewer groups than the launch's largest: whole workgroups leave together)
    const int lf = (int)a.bp.frame_log2, F = 1 << lf, H = F >> 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* re = sh;
    double* im = sh + kBandLds;
    const double2* tw = reinterpret_cast<const double2*>(tab + F);   // tw[k] = (cos, -sin)(2 pi k / F), k < F / 2
    const long long j0 = (long long)blockIdx.x * kBandGroup;
    const int nfr = (int)min((long long)kBandGroup, d.nframes - j0);
    double acc[kBandBins][4];   // the thread's bins: Re P_xn, Im P_xn, P_xx, P_nn
#pragma unroll
    for (int m = 0; m < kBandBins; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0.0;
    bool bad = false;
    for (int f = 0; f < nfr; ++f) {
        const long long u0 = (j0 + f) * H;   // the frame's first sample: u0 + F <= (J - 1) H + F <= S
        unsigned nz = 0;
        for (int i = tid; i < F; i += kBandThreads) {
            const float xv = d.kind ? norm_downmix(__builtin_bit_cast(short2, ((guint*)d.win)[u0 + i])) : ((gfloat*)d.win)[u0 + i];
            const float nv = ((gfloat*)d.needle)[u0 + i];
            bad |= !__builtin_isfinite(xv) || !__builtin_isfinite(nv);
            nz |= (xv != 0.0f ? 1u : 0u) | (nv != 0.0f ? 2u : 0u);
            const double w = tab[i];
            const int p = frame_slot(i, lf);
            re[p] = (double)xv * w;
            im[p] = (double)nv * w;
        }
        const unsigned any = frame_transform(re, im, tw, lf, nz, wbits);
        const bool has_x = any & 1u, has_n = any & 2u;
#pragma unroll
        for (int m = 0; m < kBandBins; ++m) {
            const int k = tid + m * kBandThreads;
            if (k <= H) {
                const FrameBin z = frame_untangle(re, im, F, k);   // X: the haystack's spectrum, Y: the needle's
                const double xr = has_x ? z.xr : 0.0, xi = has_x ? z.xi : 0.0;
                const double nr = has_n ? z.yr : 0.0, ni = has_n ? z.yi : 0.0;
                acc[m][0] += xr * nr + xi * ni;
                acc[m][1] += xi * nr - xr * ni;
                acc[m][2] += xr * xr + xi * xi;
                acc[m][3] += nr * nr + ni * ni;
            }
        }
        __syncthreads();   // (the next frame's samples go where these were read)
    }
    // bins to bands, two values at a time through LDS: wave w sums quantity w, w + 4, ... and its lane 0 stores the sum
    const int nb = (int)a.bp.n_bands;
    double* out = parts + (d.part0 + blockIdx.x) * (long long)a.nrec;
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int m = 0; m < kBandBins; ++m) {
            const int k = tid + m * kBandThreads;
            if (k <= H) {
                re[k] = acc[m][2 * pass];
                im[k] = acc[m][2 * pass + 1];
            }
        }
        __syncthreads();
        const int nq = 2 * nb + pass;   // (the second pass also sums E_n over every bin)
        for (int q = wv; q < nq; q += kBandThreads / 64) {
            const int b = q >> 1;
            const int lo = b < nb ? (int)a.bp.edges[b] : 0, hi = b < nb ? (int)a.bp.edges[b + 1] : H + 1;
            const double* src = (q & 1) || b == nb ? im : re;
            const double v = wave_bin_sum(src, lo, hi);
            if (lane == 0) out[b < nb ? 4 * b + 2 * pass + (q & 1) : 4 * nb] = v;
        }
        __syncthreads();
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) pflags[d.part0 + blockIdx.x] = (unsigned)any_bad;
}

// One wave per hit: lane k adds value k (k + 64, ...) of the hit's partial records in group order, lane b forms band b's record.
__global__ __launch_bounds__(64) void band_combine_kernel(const BandDesc* __restrict__ hits, int nb, double empty_ratio,
                                                          const double* __restrict__ parts, const unsigned* __restrict__ pflags,
                                                          am_hit_band* __restrict__ out) {
    __shared__ double sh[4 * AM_BAND_MAX_BANDS + 1];
    const long long h = blockIdx.x;
    const int lane = threadIdx.x;
    const BandDesc d = hits[h];
    const int nrec = 4 * nb + 1;
    for (int k = lane; k < nrec; k += 64) sh[k] = sum_slices(parts, nrec, d.part0, d.ngroups, k);
    const unsigned bf = or_flags(pflags, d.part0, d.ngroups, lane, 64);
    const int bad = __syncthreads_or(bf != 0 ? 1 : 0);
    if (lane >= nb) return;
    const double cr = sh[4 * lane], ci = sh[4 * lane + 1], ex = sh[4 * lane + 2], en = sh[4 * lane + 3], ent = sh[4 * nb];
    const float nan = __builtin_nanf("");
    float ncc, coh, gain, ldb, share;
    unsigned flags = 0;
    if (bad) {
        flags = AM_HIT_NONFINITE;
        ncc = coh = gain = ldb = share = nan;
    } else {
        const double sv = ent > 0.0 ? en / ent : 0.0;   // (a silent needle: every band is empty)
        share = (float)sv;
        if (sv < empty_ratio) {
            flags = AM_HIT_EMPTY_BAND;
            ncc = coh = gain = 0.0f;
            ldb = ex > 0.0 ? __builtin_inff() : nan;
        } else {
            if (ex == 0.0 || ex < en * d.floor_ratio) {
                flags = AM_HIT_BELOW_FLOOR;
                ncc = coh = 0.0f;
            } else {
                const double den = sqrt(ex * en);
                ncc = (float)(cr / den);
                coh = (float)(sqrt(cr * cr + ci * ci) / den);
            }
            gain = (float)(cr / en);
            ldb = level_db(ex, en);
        }
    }
    // three 64-bit stores per lane (volatile: the compiler does not merge them): no record leaves as one wide store
    // (tools/check_store_hazard.py)
    volatile unsigned long long* o = reinterpret_cast<volatile unsigned long long*>(out + h * nb + lane);
    o[0] = (unsigned long long)__float_as_uint(ncc) | ((unsigned long long)__float_as_uint(coh) << 32);
    o[1] = (unsigned long long)__float_as_uint(gain) | ((unsigned long long)__float_as_uint(ldb) << 32);
    o[2] = (unsigned long long)__float_as_uint(share) | ((unsigned long long)flags << 32);
}

}  // namespace

hipError_t launch_hit_bands(hipStream_t st, const BandDesc* d_hits, long long n, const am_band_params& bp, int max_groups,
                            double empty_ratio, const double* tab, double* parts, unsigned* pflags, am_hit_band* d_out) {
    if (n <= 0) return hipSuccess;
    BandArgs a{};
    a.bp = bp;
    a.nrec = band_record_len((int)bp.n_bands);
    const hipError_t e = for_each_grid_y(n, [&](long long h0, unsigned ny) {
        hipLaunchKernelGGL(band_frames_kernel, dim3((unsigned)max_groups, ny), dim3(kBandThreads), 0, st, d_hits, h0, a, tab, parts, pflags);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(band_combine_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, (int)bp.n_bands, empty_ratio, (const double*)parts,
                       (const unsigned*)pflags, d_out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

constexpr double kPi = 3.14159265358979323846;

long long band_frames(long long s, int lf) { return (s - (1ll << lf)) / (1ll << (lf - 1)) + 1; }   // J (s >= F)
// the samples a hit reads, counted from its start: (J - 1) H + F
size_t band_span(size_t s, int lf) { return (size_t)((band_frames((long long)s, lf) - 1) * (1ll << (lf - 1)) + (1ll << lf)); }

}  // namespace

// the table of F on c's device (am_frames.h)
int band_table(Ctx* c, int lf, const double** d_tab) {
    DevBuf& b = c->band_tabs[lf];
    if (b.p) { *d_tab = static_cast<const double*>(b.p); return AM_OK; }
    const size_t f = (size_t)1 << lf;
    std::vector<double> t(2 * f);
    for (size_t i = 0; i < f; ++i) t[i] = 0.5 - 0.5 * std::cos(2.0 * kPi * (double)i / (double)f);
    for (size_t k = 0; k < f / 2; ++k) {
        t[f + 2 * k] = std::cos(2.0 * kPi * (double)k / (double)f);
        t[f + 2 * k + 1] = -std::sin(2.0 * kPi * (double)k / (double)f);
    }
    int rc;
    if ((rc = b.ensure(sizeof(double) * t.size()))) return rc;
    hipError_t e = hipMemcpyAsync(b.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (t leaves scope)
    if (e != hipSuccess) { b.release(); return hip_fail(e, "hipMemcpy(band table)"); }
    *d_tab = static_cast<const double*>(b.p);
    return AM_OK;
}

// AM_ERR_INVALID_ARG unless bp is a valid request
int band_check_params(const am_band_params* bp) {
    if (bp->frame_log2 < 8 || bp->frame_log2 > 12)
        return fail(AM_ERR_INVALID_ARG, "frame_log2 " + std::to_string(bp->frame_log2) + " outside 8 .. 12");
    if (bp->n_bands == 0) return fail(AM_ERR_INVALID_ARG, "n_bands = 0");
    if (bp->n_bands > AM_BAND_MAX_BANDS)
        return fail(AM_ERR_INVALID_ARG, "n_bands " + std::to_string(bp->n_bands) + " > AM_BAND_MAX_BANDS (" + std::to_string(AM_BAND_MAX_BANDS) + ")");
    for (uint32_t b = 0; b < bp->n_bands; ++b)
        if (bp->edges[b] >= bp->edges[b + 1])
            return fail(AM_ERR_INVALID_ARG, "edges[" + std::to_string(b + 1) + "] = " + std::to_string(bp->edges[b + 1]) + ": edges not strictly ascending");
    const uint32_t top = (1u << bp->frame_log2) / 2 + 1;
    if (bp->edges[bp->n_bands] > top)
        return fail(AM_ERR_INVALID_ARG, "edges[" + std::to_string(bp->n_bands) + "] = " + std::to_string(bp->edges[bp->n_bands]) + " > F / 2 + 1 (" +
                                            std::to_string(top) + ")");
    return AM_OK;
}

namespace {

// ... and unless a needle of s samples holds one frame (`who`: "" or "needle j: ")
int band_check_needle(const am_band_params* bp, size_t s, const std::string& who) {
    if (s < ((size_t)1 << bp->frame_log2))
        return fail(AM_ERR_INVALID_ARG, who + "needle length " + std::to_string(s) + " < frame length " + std::to_string((size_t)1 << bp->frame_log2));
    return AM_OK;
}

// scores every hit of `hits` in one launch sequence on c's stream; out[i]: host destination of hit i's bp.n_bands records
int score_bands(Ctx* c, std::vector<BandDesc>& hits, const am_band_params& bp, am_hit_band* const* out) {
    long long total = 0;
    int max_groups = 0;
    for (BandDesc& d : hits) {
        d.part0 = total;
        total += d.ngroups;
        max_groups = std::max(max_groups, d.ngroups);
    }
    const double* tab = nullptr;
    int rc;
    if ((rc = band_table(c, (int)bp.frame_log2, &tab))) return rc;
    return hit_round_trip(c, hits, sizeof(double) * (size_t)band_record_len((int)bp.n_bands), (size_t)total, (size_t)bp.n_bands, out,
                          [&](const BandDesc* d_hits, double* parts, unsigned* pflags, am_hit_band* d_out) {
                              return launch_hit_bands(c->stream, d_hits, (long long)hits.size(), bp, max_groups,
                                                      std::pow(10.0, -(double)AM_BAND_EMPTY_DB / 10.0), tab, parts, pflags, d_out);
                          });
}

// am_hit_bands*: a hit at t reads [t, t + (J - 1) H + F)
struct BandFamily {
    typedef BandDesc Desc;
    typedef am_hit_band Rec;
    const am_band_params* bp;
    const void* params() const { return bp; }
    size_t recs() const { return bp->n_bands; }
    int check_call() const { return AM_OK; }
    int check(const am_needle* h, long long j) const {
        const int rc = band_check_params(bp);
        return rc ? rc : band_check_needle(bp, h->n, hit_needle_name(j));
    }
    double floor(const am_needle* h) const { return hit_floor_ratio(h); }
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double ratio, const HitWhere& where,
             BandDesc* d) const {
        HitDesc hd{};
        int rc;
        if ((rc = hit_desc(h, hay, len, sample_format, pk, 0.0, where, &hd))) return rc;
        const long long nframes = band_frames(hd.s, (int)bp->frame_log2);
        *d = BandDesc{hd.win, hd.needle, nframes, 0, ratio, hd.kind, (int)((nframes + kBandGroup - 1) / kBandGroup)};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t) const { return HitRange{t, t + band_span(h->n, (int)bp->frame_log2)}; }
    int score(Ctx* c, std::vector<BandDesc>& hits, am_hit_band* const* out) const { return score_bands(c, hits, *bp, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_bands(const am_needle* h, const void* haystack, size_t len, int sample_format,
                 const am_peak* peaks, size_t n, const am_band_params* bp, am_hit_band* out) {
    return hit_call(BandFamily{bp}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_bands_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                        const am_peak* peaks, size_t n, const am_band_params* bp, am_hit_band* out) {
    return hit_call(BandFamily{bp}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_bands_batch_device(const am_needle* const* needles, size_t n_needles,
                              const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                              const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                              const am_band_params* bp, am_hit_band* out) {
    return hit_call_batch(BandFamily{bp}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

int am_hit_bands_summary(const am_hit_band* rec, uint32_t n_bands, float min_coherence, am_band_summary* out) {
    if (!rec || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (n_bands == 0 || n_bands > AM_BAND_MAX_BANDS) return fail(AM_ERR_INVALID_ARG, "n_bands = 0 or > AM_BAND_MAX_BANDS");
    am_band_summary r{};
    r.first_present = r.last_present = -1;
    double all = 0.0, held = 0.0, coh = 0.0, gmin = 0.0, gmax = 0.0;
    uint32_t n_gain = 0;
    for (uint32_t b = 0; b < n_bands; ++b) {
        const am_hit_band& q = rec[b];
        if (q.flags & (AM_HIT_NONFINITE | AM_HIT_EMPTY_BAND)) continue;
        ++r.n_countable;
        all += (double)q.needle_share;
        coh += (double)q.needle_share * (double)q.coherence;
        if ((q.flags & AM_HIT_BELOW_FLOOR) || !(q.coherence >= min_coherence)) continue;
        if (r.first_present < 0) r.first_present = (int32_t)b;
        r.last_present = (int32_t)b;
        ++r.n_present;
        held += (double)q.needle_share;
        if (q.gain > 0.0f) {
            const double g = 20.0 * std::log10((double)q.gain);
            gmin = n_gain ? std::min(gmin, g) : g;
            gmax = n_gain ? std::max(gmax, g) : g;
            ++n_gain;
        }
    }
    r.coverage = held / all;              // (NaN without a countable band)
    r.weighted_coherence = coh / all;
    r.gain_db_spread = n_gain >= 2 ? gmax - gmin : std::nan("");
    *out = r;
    return AM_OK;
}

int am_band_edges_log(uint32_t sr, uint32_t frame_log2, double lo_hz, double hi_hz, uint32_t n_bands, am_band_params* out) {
    if (!out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (sr == 0) return fail(AM_ERR_INVALID_ARG, "sr = 0");
    if (frame_log2 < 8 || frame_log2 > 12) return fail(AM_ERR_INVALID_ARG, "frame_log2 " + std::to_string(frame_log2) + " outside 8 .. 12");
    if (n_bands == 0 || n_bands > AM_BAND_MAX_BANDS) return fail(AM_ERR_INVALID_ARG, "n_bands = 0 or > AM_BAND_MAX_BANDS");
    if (!(lo_hz > 0.0) || !(hi_hz > lo_hz) || !(hi_hz <= 0.5 * (double)sr))
        return fail(AM_ERR_INVALID_ARG, "band edges: need 0 < lo_hz < hi_hz <= sr / 2");
    const double f = (double)(1u << frame_log2);
    am_band_params p{};
    p.frame_log2 = frame_log2;
    p.n_bands = n_bands;
    long long prev = -1;
    for (uint32_t b = 0; b <= n_bands; ++b) {
        long long e = std::llround(lo_hz * std::pow(hi_hz / lo_hz, (double)b / (double)n_bands) * f / (double)sr);
        e = std::max(e, prev + 1);
        p.edges[b] = (uint32_t)e;
        prev = e;
    }
    if (prev > (long long)(1u << frame_log2) / 2 + 1)
        return fail(AM_ERR_INVALID_ARG, "band edges: " + std::to_string(n_bands) + " bands do not fit below F / 2 + 1");
    *out = p;
    return AM_OK;
}

}  // extern "C"
