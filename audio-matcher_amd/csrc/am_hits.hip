// am_hits.hip -- per-hit scoring (am_hit_scores*, include/audiomatch.h): for a hit at t, needle n[0 .. S) and the
// haystack's samples x (the down-mix for AM_FMT_S16_STEREO), in f64:
//   corr(u) = sum_{i<S} x[u + i] n[i] at u = t - 1, t, t + 1,   E_w = sum_{i<S} x[t + i]^2
// and from those the exact NCC, the least-squares gain, the window level and a parabolic sub-sample position.
//
// Two kernels on the context's stream:
//   hit_slices    one workgroup per slice of kHitSlice needle samples of one hit (blockIdx.x = slice, blockIdx.y =
//                 hit): stages x over the slice plus one sample each side in LDS (stage_load), accumulates the four
//                 sums from that one read, adds them over the workgroup (wave_sums, add_waves) and writes one partial
//                 record (four doubles, one 64-bit store each, and a flag word).
//   hit_combine   one wave per hit: adds the hit's partials in the order of sum_slices and writes its am_hit_score.
// A hit's result depends on its needle, the samples it reads and the floor only (the slices of a hit start at
// multiples of kHitSlice of the needle, every reduction runs in the fixed order am_hit_device.h states): the single,
// batch and host forms agree bit for bit, whatever else a call holds.
//
// Below the kernels: the host side every per-hit family shares (this file, am_segments.hip, am_bands.hip,
// am_significance.hip) -- the preludes of the three call forms, span staging for the host forms and the table's trip to
// the device and back; the templates that tie them together (hit_call, hit_call_batch, hit_round_trip) are in
// am_internal.h, which also says what a family supplies.  Then am_hit_scores* itself, as the first such family.
#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kHitThreads = 256;
constexpr int kHitPer = kHitSlice / kHitThreads;   // needle samples per thread and slice
static_assert(kHitSlice % kHitThreads == 0, "slice must split evenly over the workgroup");

template <int KIND>
__global__ __launch_bounds__(kHitThreads) void hit_slices_kernel(const HitDesc* __restrict__ hits, long long hit0,
                                                                 double* __restrict__ parts, unsigned* __restrict__ pflags) {
    __shared__ float xs[kHitSlice + 2];
    __shared__ double ws[4][kHitThreads / 64];
    const HitDesc d = hits[hit0 + blockIdx.y];
    const long long i0 = (long long)blockIdx.x * kHitSlice;
    if (i0 >= d.s) return;   // (a shorter needle than the launch's longest: whole workgroups leave together)
    const int tid = threadIdx.x;
    const int m = (int)min((long long)kHitSlice, d.s - i0);
    // every load of the slice in flight at once: xs[q] = x[t + i0 - 1 + q] (stage_load, stage_store; the samples the hit
    // reads are [ulo, uhi)) and the thread's needle samples n[i0 + q]
    gfloat* nd = (gfloat*)d.needle + i0;
    float xv[kHitPer], nv[kHitPer], xt;
    stage_load<KIND, kHitThreads>(d.win, i0 - 1, m, 2, (d.edge & 1) ? -1 : 0, (d.edge & 2) ? d.s + 1 : d.s, xv, xt,
                                  [&](int r, int q) { nv[r] = q < m ? nd[q] : 0.0f; });
    stage_store<kHitThreads>(StageFlat{}, xs, 2, xv, xt);   // (the non-finite test is on what the sums read, below)
    __syncthreads();
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, ew = 0.0;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < kHitPer; ++r) {
        const int q = tid + r * kHitThreads;
        if (q < m) {
            const float n = nv[r], xm = xs[q], x = xs[q + 1], xp = xs[q + 2];
            const double dn = (double)n, dx = (double)x;
            c0 += (double)xm * dn;   // (a product of two f32 values is exact in f64)
            c1 += dx * dn;
            c2 += (double)xp * dn;
            ew += dx * dx;
            bad |= !__builtin_isfinite(x) || !__builtin_isfinite(n);
        }
    }
    const double v[4] = {c0, c1, c2, ew};
    wave_sums<kHitThreads>(v, ws);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    // one 64-bit store per lane: no record leaves as one wide store (tools/check_store_hazard.py)
    const long long p = d.part0 + blockIdx.x;
    if (tid < 4) parts[4 * p + tid] = add_waves<kHitThreads>(ws[tid]);
    else if (tid == 4) pflags[p] = (unsigned)any_bad;
}

// One wave per hit: the lanes fetch 64 partial records at a time into LDS, lane 0 adds them to 0 in slice order -- the
// order of sum_slices, not its loop: with a column per lane (four lanes, each walking its column's loads one behind the
// other) a call of few hits took 0.6 to 1.5 us longer (profiles/r23).
__global__ __launch_bounds__(64) void hit_combine_kernel(const HitDesc* __restrict__ hits, const double* __restrict__ parts,
                                                         const unsigned* __restrict__ pflags, am_hit_score* __restrict__ out) {
    __shared__ double ps[4][64];
    __shared__ unsigned fs[64];
    const long long h = blockIdx.x;
    const int lane = threadIdx.x;
    const HitDesc d = hits[h];
    const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
    double a = 0.0, b = 0.0, c = 0.0, ew = 0.0;
    unsigned bad = 0;
    for (long long k0 = 0; k0 < ns; k0 += 64) {
        const long long k = k0 + lane;
        if (k < ns) {
            const long long p = d.part0 + k;
            for (int j = 0; j < 4; ++j) ps[j][lane] = parts[4 * p + j];
            fs[lane] = pflags[p];
        }
        __syncthreads();
        if (lane == 0) {
            const int cnt = (int)min(64ll, ns - k0);
            for (int i = 0; i < cnt; ++i) {
                a += ps[0][i];
                b += ps[1][i];
                c += ps[2][i];
                ew += ps[3][i];
                bad |= fs[i];
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    const double nan = __builtin_nan("");
    double pos = (double)d.t;
    float ncc, gain, wdb;
    unsigned flags = 0;
    if (bad) {
        flags = AM_HIT_NONFINITE;
        ncc = gain = wdb = (float)nan;
    } else {
        bool refined, below;
        const double delta = parabola_vertex(a, b, c, &refined);
        if ((d.edge & 3) != 3 || !__builtin_isfinite(a) || !__builtin_isfinite(c) || !refined) flags |= AM_HIT_UNREFINED;
        else pos += delta;
        ncc = (float)ncc_or_floor(b, d.en, ew, d.thr, &below);
        if (below) flags |= AM_HIT_BELOW_FLOOR;
        gain = d.en > 0.0 ? (float)(b / d.en) : 0.0f;
        wdb = level_db(ew, d.en);
    }
    am_hit_score* o = out + h;
    o->position = pos;
    o->ncc = ncc;
    o->gain = gain;
    o->window_db = wdb;
    o->flags = flags;
}

}  // namespace

hipError_t launch_hit_scores(hipStream_t st, const HitDesc* d_hits, long long n, long long max_slices, int kind, double* parts,
                             unsigned* pflags, am_hit_score* d_out) {
    if (n <= 0) return hipSuccess;
    const hipError_t e = for_each_grid_y(n, [&](long long h0, unsigned nh) {
        const dim3 grid((unsigned)max_slices, nh);
        if (kind) hipLaunchKernelGGL(hit_slices_kernel<1>, grid, dim3(kHitThreads), 0, st, d_hits, h0, parts, pflags);
        else hipLaunchKernelGGL(hit_slices_kernel<0>, grid, dim3(kHitThreads), 0, st, d_hits, h0, parts, pflags);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hit_combine_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, (const double*)parts, (const unsigned*)pflags, d_out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

std::string hit_pair_name(const HitWhere& w) {
    if (w.pair < 0) return "";
    return "pair " + std::to_string(w.pair) + " (haystack " + std::to_string(w.hay) + ", needle " + std::to_string(w.needle) + "): ";
}

int hit_check_device(const void* p, int device, const HitWhere& where) {
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess || (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged)) {
        if (e != hipSuccess) (void)hipGetLastError();
        return fail(AM_ERR_INVALID_ARG, hit_pair_name(where) + "haystack: not device memory");
    }
    if (a.device != device)
        return fail(AM_ERR_INVALID_ARG, hit_pair_name(where) + "haystack: on device " + std::to_string(a.device) + ", the needle on device " +
                                            std::to_string(device));
    return AM_OK;
}


int hit_desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double thr,
             const HitWhere& where, HitDesc* d) {
    const size_t s = h->n;
    if (pk.start > len || s > len - pk.start)   // (the message is built only here: a call's cost does not grow with it)
        return fail(AM_ERR_INVALID_ARG, hit_pair_name(where) + "hit " + std::to_string(where.hit) + ": start + needle length > haystack length (" +
                                            std::to_string(pk.start) + " + " + std::to_string(s) + " > " + std::to_string(len) + ")");
    d->win = advance_src(hay, (size_t)pk.start);
    d->needle = h->d_needle;
    d->s = (long long)s;
    d->kind = sample_format == AM_FMT_S16_STEREO ? 1 : 0;
    d->edge = (pk.start > 0 ? 1 : 0) | (pk.start + s < len ? 2 : 0);
    d->t = (long long)pk.start;
    d->en = h->energy;
    d->thr = thr;
    d->part0 = 0;
    return AM_OK;
}

double hit_floor(const am_needle* h) {
    return norm_spec(h, snapshot_opts(h)).thr;
}

double hit_floor_ratio(const am_needle* h) {
    return std::pow(10.0, -(double)snapshot_opts(h).score_norm_floor_db / 10.0);
}

// ---- the frame of the per-hit families (am_internal.h) ---------------------------------------------------------------

std::string hit_needle_name(long long j) {
    return j < 0 ? "" : "needle " + std::to_string(j) + ": ";
}

int hit_single_prelude(const am_needle* h, int sample_format, size_t n, const void* hay, const am_peak* peaks, const void* out,
                       const void* params, bool* done) {
    int rc = check_needle(h);
    if (rc) return rc;
    if ((rc = check_format(sample_format))) return rc;
    *done = n == 0;
    if (*done) return AM_OK;
    if (!hay || !peaks || !out || !params) return fail(AM_ERR_INVALID_ARG, "null pointer");
    return AM_OK;
}

int hit_batch_counts(size_t n_needles, size_t n_hay, int sample_format, const void* needles, const void* d_haystacks, const void* lens,
                     const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks, const void* out, const void* params, size_t* total) {
    int rc;
    *total = 0;
    if ((rc = check_format(sample_format))) return rc;
    if (n_needles == 0 || n_hay == 0) return AM_OK;
    if (!needles || !d_haystacks || !lens || !n_peaks) return fail(AM_ERR_INVALID_ARG, "null pointer");
    size_t sum = 0;
    for (size_t q = 0; q < n_needles * n_hay; ++q) sum += std::min(n_peaks[q], cap_per_pair);
    if (sum && (!peaks || !out || !params)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *total = sum;
    return AM_OK;
}

int hit_batch_needles(const am_needle* const* needles, size_t n_needles) {
    int rc;
    for (size_t j = 0; j < n_needles; ++j)
        if (!needles[j] || !needles[j]->ctx) return fail(AM_ERR_INVALID_ARG, hit_needle_name((long long)j) + "null needle handle");
    if ((rc = check_needle(needles[0]))) return rc;
    const int device = needles[0]->ctx->device;
    for (size_t j = 1; j < n_needles; ++j)
        if (needles[j]->ctx->device != device)
            return fail(AM_ERR_INVALID_ARG, hit_needle_name((long long)j) + "on device " + std::to_string(needles[j]->ctx->device) +
                                                ", needle 0 on device " + std::to_string(device));
    return AM_OK;
}

int stage_spans(Ctx* c, const void* haystack, const HitRange* r, size_t n, const void** at) {
    std::vector<Span> spans;
    std::vector<size_t> span_of;
    const size_t staged = merge_spans(r, n, spans, span_of);
    int rc;
    if ((rc = c->hit_stage.ensure(4 * staged))) return rc;   // (4 bytes per f32 sample and per i16 stereo frame)
    for (const Span& sp : spans)
        AM_HIP(hipMemcpyAsync(const_cast<void*>(advance_src(c->hit_stage.p, sp.off)), advance_src(haystack, sp.lo), 4 * (sp.hi - sp.lo),
                              hipMemcpyHostToDevice, c->stream));
    for (size_t i = 0; i < n; ++i) {
        const Span& sp = spans[span_of[i]];
        at[i] = advance_src(c->hit_stage.p, sp.off + (r[i].lo - sp.lo));
    }
    return AM_OK;
}

int hit_io_reserve(Ctx* c, size_t tab_bytes, size_t out_bytes) {
    int rc;
    if ((rc = c->hit_tab.ensure(tab_bytes)) || (rc = c->hit_out.ensure(out_bytes))) return rc;
    return c->hit_io.ensure(tab_bytes + out_bytes);
}

int hit_table_put(Ctx* c, const void* rows, size_t off, size_t bytes) {
    char* pinned = static_cast<char*>(c->hit_io.p) + off;
    std::memcpy(pinned, rows, bytes);
    AM_HIP(hipMemcpyAsync(static_cast<char*>(c->hit_tab.p) + off, pinned, bytes, hipMemcpyHostToDevice, c->stream));
    return AM_OK;
}

int hit_results_get(Ctx* c, size_t tab_bytes, size_t out_bytes, const void** res) {
    void* pinned = static_cast<char*>(c->hit_io.p) + tab_bytes;
    *res = pinned;
    return download(c, pinned, c->hit_out.p, out_bytes);
}

namespace {

int score_hits(Ctx* c, std::vector<HitDesc>& hits, am_hit_score* const* out) {
    long long total = 0, max_slices = 0;
    for (HitDesc& d : hits) {
        const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
        d.part0 = total;
        total += ns;
        max_slices = std::max(max_slices, ns);
    }
    return hit_round_trip(c, hits, 4 * sizeof(double), (size_t)total, 1, out,
                          [&](const HitDesc* tab, double* parts, unsigned* pflags, am_hit_score* d_out) {
                              return launch_hit_scores(c->stream, tab, (long long)hits.size(), max_slices, hits[0].kind, parts, pflags, d_out);
                          });
}

// am_hit_scores*: no parameters; a hit at t reads [t - 1, t + S + 1), clipped to the haystack
struct ScoreFamily {
    typedef HitDesc Desc;
    typedef am_hit_score Rec;
    const void* params() const { return this; }
    size_t recs() const { return 1; }
    int check_call() const { return AM_OK; }
    int check(const am_needle*, long long) const { return AM_OK; }
    double floor(const am_needle* h) const { return hit_floor(h); }
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double thr, const HitWhere& where,
             HitDesc* d) const {
        return hit_desc(h, hay, len, sample_format, pk, thr, where, d);
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const { return HitRange{t > 0 ? t - 1 : 0, std::min(len, t + h->n + 1)}; }
    int score(Ctx* c, std::vector<HitDesc>& hits, am_hit_score* const* out) const { return score_hits(c, hits, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_scores(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_peak* peaks, size_t n, am_hit_score* out) {
    return hit_call(ScoreFamily{}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_scores_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_peak* peaks, size_t n, am_hit_score* out) {
    return hit_call(ScoreFamily{}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_scores_batch_device(const am_needle* const* needles, size_t n_needles,
                               const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                               const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks, am_hit_score* out) {
    return hit_call_batch(ScoreFamily{}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

}  // extern "C"
