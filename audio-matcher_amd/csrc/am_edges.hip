// am_edges.hip -- edge matching (am_edge_scores*, am_match_edges*; include/audiomatch.h, "edge matching"): a needle cut
// off by a recording's start or end.  Partial-overlap NCC at the head lags (the needle's first samples are missing) and
// the tail lags (its last samples are), each score normalised by the energy of the part of the needle that lies inside
// the recording.
//
// Per haystack and edge, on the context's stream:
//   edge_span        one pass over the span (head x[0, W), tail x[len - W, len), W = min(len, S - 1)): the down-mix of an
//                    i16 frame, non-finite samples zeroed, the first / last non-finite index by one atomic max per wave
//   the energy scan  x^2 in f64 as prefix (head) or suffix (tail) sums, in three launches of a fixed order: edge_tile_totals
//                    (one workgroup per tile of AM_EDGE_TILE elements), edge_scan_totals (one workgroup scans the totals),
//                    edge_tile_scan (a tile's scan plus the totals before it).  A thread walks a contiguous run of global
//                    memory (block_scan_with, am_reduce.h): no LDS tile, so no f64 bank conflicts of strided runs.  Sums
//                    of non-negative terms only, never a difference of two prefix values (see the head of am_norm.hip).
//                    The needle's prefix and suffix scans are made once per handle.
//   run_correlation  the overlap-save engine as it stands, always f32, factor 1: lead S - 1 for the head, 0 for the tail
//   edge_normalise   the coarse score of every lag from the f32 correlation and the f64 scans, NaN where the lag is no
//                    candidate; four lags per thread, 16-byte accesses
//   probe_reduce     discovery's record rule (am_discover.hip) on the coarse scores
// and once per haystack: edge_exact (the at most four chosen lags: three f64 sums each, kExactParts workgroups per lag)
// and edge_finish (folds the parts in index order and writes both records).  Every step depends on the needle, the span
// and the parameters only, so the call forms agree bit for bit.
#include "am_internal.h"
#include "am_reduce.h"

#include <climits>
#include <cmath>

namespace am {

namespace {

constexpr int kTile = AM_EDGE_TILE;
constexpr int kThreads = 256;
constexpr int kExactParts = 64;      // workgroups per chosen lag
constexpr int kPrepBlocks = 1024;    // blocks of the capped grids; the rest is strided
static_assert(sizeof(am_edge_hit) == 48, "am_edge_hit is 48 bytes, no padding");
static_assert(sizeof(am_edge_params) == 24, "am_edge_params is 24 bytes");
static_assert(kTile % kThreads == 0, "a tile splits evenly over the workgroup");

// ctl[0]: max over the non-finite samples of (W - index), ctl[1]: max of (index + 1); both 0 when there is none
template <int KIND>
__global__ void __launch_bounds__(kThreads) edge_span(const void* __restrict__ src, long long W, float* __restrict__ out,
                                                      unsigned long long* __restrict__ ctl) {
    unsigned long long m0 = 0, m1 = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < W; i += (long long)gridDim.x * kThreads) {
        const float v = hit_sample<KIND>(src, i);
        const bool fin = fabsf(v) <= __FLT_MAX__;
        out[i] = fin ? v : 0.0f;
        if (!fin) {
            m0 = max(m0, (unsigned long long)(W - i));
            m1 = max(m1, (unsigned long long)(i + 1));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        m0 = max(m0, __shfl_xor(m0, off, 64));
        m1 = max(m1, __shfl_xor(m1, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && m0) {
        atomicMax(&ctl[0], m0);
        atomicMax(&ctl[1], m1);
    }
}

// element q of the scanned sequence: x[q]^2 in f64, from the other end when rev
__device__ __forceinline__ double scan_term(const float* __restrict__ x, long long n, int rev, long long q) {
    const double d = (double)x[rev ? n - 1 - q : q];
    return d * d;
}

__global__ void __launch_bounds__(kThreads) edge_tile_totals(const float* __restrict__ x, long long n, int rev, double* __restrict__ tot) {
    __shared__ double ws[kThreads / 64];
    const long long q0 = (long long)blockIdx.x * kTile, q1 = min(q0 + kTile, n);
    double s = 0.0;
    for (long long q = q0 + threadIdx.x; q < q1; q += kThreads) s += scan_term(x, n, rev, q);
    s = block_sum<kThreads>(s, ws);
    if (threadIdx.x == 0) tot[blockIdx.x] = s;
}

// one workgroup: the totals become their inclusive scan
__global__ void __launch_bounds__(kThreads) edge_scan_totals(double* __restrict__ tot, int ntiles) {
    __shared__ double ws[kThreads / 64];
    block_scan<kThreads, false>(tot, ntiles, ws);
}

__global__ void __launch_bounds__(kThreads) edge_tile_scan(const float* __restrict__ x, long long n, int rev, const double* __restrict__ tot,
                                                           double* __restrict__ out) {
    __shared__ double ws[kThreads / 64];
    const long long q0 = (long long)blockIdx.x * kTile;
    const int cnt = (int)min((long long)kTile, n - q0);
    const double carry = blockIdx.x ? tot[blockIdx.x - 1] : 0.0;
    block_scan_with<kThreads>(
        cnt, ws, [&](int q) { return scan_term(x, n, rev, q0 + q); },
        [&](int q, double v) { out[rev ? n - 1 - (q0 + q) : q0 + q] = carry + v; });
}

struct EdgeRule {
    long long S, W;
    int edge;
    long long min_overlap;
    double share_thr;      // (double)min_share * E_n
    double floor_ratio;    // 10^(-score_norm_floor_db / 10)
};

// the score of c over the energies en, ex; *below: the floor rule made it 0
__device__ __forceinline__ float edge_score(double c, double en, double ex, double floor_ratio, bool* below) {
    *below = ex == 0.0 || ex < en * floor_ratio;
    if (*below || en == 0.0) return 0.0f;
    return (float)(c / sqrt(en * ex));
}

// lag j of the edge (its overlap L): the coarse score, NaN where it is no candidate
__device__ __forceinline__ float edge_coarse(const EdgeRule& r, long long j, float c, const double* __restrict__ nscan,
                                             const double* __restrict__ xscan, unsigned long long m0, unsigned long long m1) {
    const long long L = r.edge == AM_EDGE_HEAD ? j + 1 : r.W - j;
    const double en = r.edge == AM_EDGE_HEAD ? nscan[r.S + (r.S - L)] : nscan[L - 1];
    const bool clean = r.edge == AM_EDGE_HEAD ? (m0 == 0 || L <= r.W - (long long)m0) : j >= (long long)m1;
    if (!(L >= r.min_overlap && en >= r.share_thr && clean)) return __uint_as_float(0x7FC00000u);
    bool below;
    return edge_score((double)c, en, xscan[j], r.floor_ratio, &below);
}

// g (16-byte aligned): the f32 correlation of the edge's lags on entry, their coarse scores on return
__global__ void __launch_bounds__(kThreads) edge_normalise(float* __restrict__ g, EdgeRule r, const double* __restrict__ nscan,
                                                           const double* __restrict__ xscan, const unsigned long long* __restrict__ ctl) {
    const unsigned long long m0 = ctl[0], m1 = ctl[1];
    const long long quads = (r.W + 3) / 4;
    for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < quads; t += (long long)gridDim.x * kThreads) {
        const long long j0 = 4 * t;
        if (j0 + 4 <= r.W) {
            float4 v = reinterpret_cast<const float4*>(g)[t];
            v.x = edge_coarse(r, j0, v.x, nscan, xscan, m0, m1);
            v.y = edge_coarse(r, j0 + 1, v.y, nscan, xscan, m0, m1);
            v.z = edge_coarse(r, j0 + 2, v.z, nscan, xscan, m0, m1);
            v.w = edge_coarse(r, j0 + 3, v.w, nscan, xscan, m0, m1);
            reinterpret_cast<float4*>(g)[t] = v;
        } else {
            for (long long j = j0; j < r.W; ++j) g[j] = edge_coarse(r, j, g[j], nscan, xscan, m0, m1);
        }
    }
}

struct ExactJob {
    const float* needle;
    long long S;
    const float* span[2];
    long long W[2], first[2];
    const am_probe_hit* probe;   // [2]: the coarse records of the edges with W > 0
    double e_total, floor_ratio;
};

// Workgroup (part, q): its share of the three sums of chosen lag q (0: head best, 1: head runner-up, 2: tail best, 3:
// tail runner-up) into parts[(q kExactParts + part) 3 ..]; a lag that does not exist gives zeros.
__global__ void __launch_bounds__(kThreads) edge_exact(ExactJob job, double* __restrict__ parts) {
    __shared__ double ws[3][kThreads / 64];
    const int q = blockIdx.y, e = q >> 1, part = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    const long long W = job.W[e];
    bool have = W > 0;
    am_probe_hit rec{};
    if (have) {
        rec = job.probe[e];
        have = !(rec.flags & ((q & 1) ? AM_PROBE_NO_SECOND : AM_PROBE_NO_BEST));
    }
    if (have) {
        const long long j = (long long)((q & 1) ? rec.second : rec.best);
        const long long L = e == AM_EDGE_HEAD ? j + 1 : W - j;
        const float* __restrict__ xs = e == AM_EDGE_HEAD ? job.span[0] : job.span[1] + j;
        const float* __restrict__ ns = e == AM_EDGE_HEAD ? job.needle + (job.S - L) : job.needle;
        for (long long i = (long long)part * kThreads + threadIdx.x; i < L; i += (long long)kExactParts * kThreads) {
            const double x = (double)xs[i], n = (double)ns[i];
            v[0] += x * n;
            v[1] += n * n;
            v[2] += x * x;
        }
    }
    wave_sums<kThreads>(v, ws);
    __syncthreads();
    if (threadIdx.x < 3) parts[((size_t)q * kExactParts + part) * 3 + threadIdx.x] = add_waves<kThreads>(ws[threadIdx.x]);
}

// thread e < 2: the record of edge e from the parts, added in index order
__global__ void __launch_bounds__(64) edge_finish(ExactJob job, const double* __restrict__ parts, am_edge_hit* __restrict__ out) {
    const int e = threadIdx.x;
    if (e >= 2) return;
    const float nan = __uint_as_float(0x7FC00000u);
    am_edge_hit r;
    r.start = r.second = 0;
    r.overlap = 0;
    r.ncc = r.ncc_second = r.gain = r.share = nan;
    r.edge = (uint32_t)e;
    r.flags = AM_EDGE_NO_BEST | AM_EDGE_NO_SECOND;
    const long long W = job.W[e];
    am_probe_hit rec{};
    if (W > 0) rec = job.probe[e];
    if (W > 0 && !(rec.flags & AM_PROBE_NO_BEST)) {
        double s[2][3];
        for (int k = 0; k < 2; ++k)
            for (int m = 0; m < 3; ++m) {
                double t = 0.0;
                for (int p = 0; p < kExactParts; ++p) t += parts[((size_t)(2 * e + k) * kExactParts + p) * 3 + m];
                s[k][m] = t;
            }
        const long long j = (long long)rec.best;
        bool below;
        r.flags = 0;
        r.start = job.first[e] + j;
        r.overlap = (uint64_t)(e == AM_EDGE_HEAD ? j + 1 : W - j);
        r.ncc = edge_score(s[0][0], s[0][1], s[0][2], job.floor_ratio, &below);
        if (below) r.flags |= AM_EDGE_BELOW_FLOOR;
        r.gain = s[0][1] > 0.0 ? (float)(s[0][0] / s[0][1]) : 0.0f;
        r.share = (float)(s[0][1] / job.e_total);
        if (rec.flags & AM_PROBE_NO_SECOND) {
            r.flags |= AM_EDGE_NO_SECOND;
        } else {
            r.second = job.first[e] + (long long)rec.second;
            r.ncc_second = edge_score(s[1][0], s[1][1], s[1][2], job.floor_ratio, &below);
        }
    }
    out[e] = r;
}

// ---- host side -------------------------------------------------------------------------------------------------------

struct EdgeGeom { long long W, first; };   // the edge's lags: first .. first + W - 1
EdgeGeom edge_geom(size_t len, size_t s, int edge) {
    const long long W = (long long)std::min(len, s - 1);
    return EdgeGeom{W, edge == AM_EDGE_HEAD ? -((long long)s - 1) : (long long)len - W};
}
inline size_t pad64(long long w) { return ((size_t)w + 63) & ~(size_t)63; }

int grid_for(long long items, int per_block) {
    return (int)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, kPrepBlocks));
}

// the scan of x[0, n)^2 into out[0, n): prefix sums, or suffix sums when rev
int energy_scan(Ctx* c, const float* x, long long n, bool rev, double* out) {
    const long long ntiles = (n + kTile - 1) / kTile;
    if (ntiles > INT_MAX) return fail(AM_ERR_INVALID_ARG, "edge matching: needle too long");
    int rc;
    if ((rc = c->edge_tot.ensure(sizeof(double) * (size_t)ntiles))) return rc;
    double* tot = (double*)c->edge_tot.p;
    ProfScope ps(c, KN_EDGES, c->stream);
    hipLaunchKernelGGL(edge_tile_totals, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, x, n, (int)rev, tot);
    AM_HIP(hipGetLastError());
    hipLaunchKernelGGL(edge_scan_totals, dim3(1), dim3(kThreads), 0, c->stream, tot, (int)ntiles);
    AM_HIP(hipGetLastError());
    hipLaunchKernelGGL(edge_tile_scan, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, x, n, (int)rev, (const double*)tot, out);
    AM_HIP(hipGetLastError());
    return AM_OK;
}

int needle_scans(am_needle* h) {
    if (h->d_edge_scans) return AM_OK;
    double* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, sizeof(double) * 2 * h->n));
    int rc;
    if ((rc = energy_scan(h->ctx, h->d_needle, (long long)h->n, false, d)) ||
        (rc = energy_scan(h->ctx, h->d_needle, (long long)h->n, true, d + h->n))) {
        (void)hipStreamSynchronize(h->ctx->stream);
        (void)hipFree(d);
        return rc;
    }
    h->d_edge_scans = d;
    return AM_OK;
}

// where one haystack's edges work: everything sized for both edges of W lags
struct EdgeBufs {
    float* span[2];
    float* scores[2];
    double* xscan[2];
    unsigned long long* ctl[2];
    double* parts;
    am_probe_hit* probe;
    am_edge_hit* rec;
};
int edge_reserve(Ctx* c, long long W, EdgeBufs* b) {
    const size_t wp = std::max<size_t>(pad64(W), 64);
    int rc;
    if ((rc = c->edge_span.ensure(sizeof(float) * 2 * wp)) || (rc = c->edge_scores.ensure(sizeof(float) * 2 * wp)) ||
        (rc = c->edge_scan.ensure(sizeof(double) * 2 * wp)) || (rc = c->edge_ctl.ensure(sizeof(unsigned long long) * 4)) ||
        (rc = c->edge_parts.ensure(sizeof(double) * 4 * kExactParts * 3)) || (rc = c->edge_rec.ensure(128 + sizeof(am_edge_hit) * 2)) ||
        (rc = c->edge_tot.ensure(sizeof(double) * (size_t)((W + kTile - 1) / kTile + 1))))
        return rc;
    for (int e = 0; e < 2; ++e) {
        b->span[e] = (float*)c->edge_span.p + e * wp;
        b->scores[e] = (float*)c->edge_scores.p + e * wp;
        b->xscan[e] = (double*)c->edge_scan.p + e * wp;
        b->ctl[e] = (unsigned long long*)c->edge_ctl.p + 2 * e;
    }
    b->parts = (double*)c->edge_parts.p;
    b->probe = (am_probe_hit*)c->edge_rec.p;
    b->rec = (am_edge_hit*)((char*)c->edge_rec.p + 128);
    return AM_OK;
}

struct EdgeCall {
    am_needle* h;
    Opts o;                 // half_pipeline off: the transforms are always f32
    double floor_ratio;
    const am_edge_params* ep;
    int fmt;
};

// The coarse scores of one edge into b.scores[edge] (W >= 1 lags).  src: the span's first element.
int edge_coarse_scores(const EdgeCall& k, const void* src, long long W, int edge, const EdgeBufs& b) {
    am_needle* h = k.h;
    Ctx* c = h->ctx;
    const long long S = (long long)h->n;
    int rc;
    AM_HIP(hipMemsetAsync(b.ctl[edge], 0, sizeof(unsigned long long) * 2, c->stream));
    {
        ProfScope ps(c, KN_EDGES, c->stream);
        if (k.fmt == AM_FMT_S16_STEREO)
            hipLaunchKernelGGL(edge_span<1>, dim3(grid_for(W, kThreads)), dim3(kThreads), 0, c->stream, src, W, b.span[edge], b.ctl[edge]);
        else
            hipLaunchKernelGGL(edge_span<0>, dim3(grid_for(W, kThreads)), dim3(kThreads), 0, c->stream, src, W, b.span[edge], b.ctl[edge]);
        AM_HIP(hipGetLastError());
    }
    if ((rc = energy_scan(c, b.span[edge], W, edge == AM_EDGE_TAIL, b.xscan[edge]))) return rc;
    if ((rc = run_correlation(h, k.o, b.span[edge], W, edge == AM_EDGE_HEAD ? S - 1 : 0, b.scores[edge], W, 1.0f))) return rc;
    EdgeRule r{};
    r.S = S; r.W = W; r.edge = edge;
    r.min_overlap = (long long)std::min<uint64_t>(k.ep->min_overlap, (uint64_t)LLONG_MAX);
    r.share_thr = (double)k.ep->min_share * h->energy;
    r.floor_ratio = k.floor_ratio;
    ProfScope ps(c, KN_EDGES, c->stream);
    hipLaunchKernelGGL(edge_normalise, dim3(grid_for((W + 3) / 4, kThreads)), dim3(kThreads), 0, c->stream, b.scores[edge], r,
                       (const double*)h->d_edge_scans, (const double*)b.xscan[edge], (const unsigned long long*)b.ctl[edge]);
    AM_HIP(hipGetLastError());
    return AM_OK;
}

am_edge_hit empty_edge(int edge, uint32_t flags) {
    am_edge_hit r{};
    r.ncc = r.ncc_second = r.gain = r.share = std::nanf("");
    r.edge = (uint32_t)edge;
    r.flags = flags;
    return r;
}

bool needle_finite(const am_needle* h) { return std::isfinite(h->energy); }

// Both records of one haystack.  src[e]: the first element of edge e's span (resident).  Synchronous.
int match_edges_one(const EdgeCall& k, const void* const src[2], size_t len, am_edge_hit out[2]) {
    am_needle* h = k.h;
    Ctx* c = h->ctx;
    if (!needle_finite(h)) {
        for (int e = 0; e < 2; ++e) out[e] = empty_edge(e, AM_EDGE_NONFINITE);
        return AM_OK;
    }
    const EdgeGeom g0 = edge_geom(len, h->n, AM_EDGE_HEAD), g1 = edge_geom(len, h->n, AM_EDGE_TAIL);
    if (g0.W == 0) {   // (a needle of one sample: no edge has a lag)
        for (int e = 0; e < 2; ++e) out[e] = empty_edge(e, AM_EDGE_NO_BEST | AM_EDGE_NO_SECOND);
        return AM_OK;
    }
    int rc;
    EdgeBufs b{};
    if ((rc = needle_scans(h)) || (rc = edge_reserve(c, g0.W, &b))) return rc;
    const uint64_t sep = k.ep->separation ? k.ep->separation : k.ep->min_overlap;
    for (int e = 0; e < 2; ++e) {
        if ((rc = edge_coarse_scores(k, src[e], g0.W, e, b))) return rc;
        if ((rc = probe_reduce(c, b.scores[e], g0.W, 0, 0, sep, 0, b.probe + e))) return rc;
    }
    ExactJob job{};
    job.needle = h->d_needle; job.S = (long long)h->n;
    job.span[0] = b.span[0]; job.span[1] = b.span[1];
    job.W[0] = g0.W; job.W[1] = g1.W; job.first[0] = g0.first; job.first[1] = g1.first;
    job.probe = b.probe;
    job.e_total = h->energy; job.floor_ratio = k.floor_ratio;
    {
        ProfScope ps(c, KN_EDGES, c->stream);
        hipLaunchKernelGGL(edge_exact, dim3(kExactParts, 4), dim3(kThreads), 0, c->stream, job, b.parts);
        AM_HIP(hipGetLastError());
        hipLaunchKernelGGL(edge_finish, dim3(1), dim3(64), 0, c->stream, job, (const double*)b.parts, b.rec);
        AM_HIP(hipGetLastError());
    }
    return download(c, out, b.rec, sizeof(am_edge_hit) * 2);
}

int check_edge_params(const am_edge_params* ep) {
    if (!ep) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (ep->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_edge_params: reserved must be 0");
    if (ep->min_overlap == 0) return fail(AM_ERR_INVALID_ARG, "am_edge_params: min_overlap must be at least 1");
    if (!(ep->min_share >= 0.0f && ep->min_share <= 1.0f)) return fail(AM_ERR_INVALID_ARG, "am_edge_params: min_share must be in [0, 1]");
    return AM_OK;
}

int check_edge(int edge) {
    return edge == AM_EDGE_HEAD || edge == AM_EDGE_TAIL ? AM_OK : fail(AM_ERR_INVALID_ARG, "bad edge " + std::to_string(edge));
}

// what every form checks first: the handle, the pointers, the parameters, the format, the length
int edge_prelude(const am_needle* h, const void* hay, size_t len, int sample_format, const am_edge_params* ep, const void* out) {
    int rc = check_needle(h);
    if (rc) return rc;
    if (!hay || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_edge_params(ep)) || (rc = check_format(sample_format))) return rc;
    if (len == 0) return fail(AM_ERR_INVALID_ARG, "len must be at least 1");
    return AM_OK;
}

EdgeCall edge_call(am_needle* h, int sample_format, const am_edge_params* ep) {
    EdgeCall k{};
    k.h = h;
    k.o = snapshot_opts(h);
    k.o.half = 0;
    k.floor_ratio = hit_floor_ratio(h);
    k.ep = ep;
    k.fmt = sample_format;
    return k;
}

// The spans of a host haystack side by side in the context's input buffer (the tail's at a 256-byte boundary): only they
// are copied.  which: bit e = edge e is wanted.
int upload_spans(Ctx* c, const void* haystack, size_t len, long long W, int which, const void* src[2]) {
    const size_t bytes = sample_bytes((size_t)W), off = (bytes + 255) & ~(size_t)255;
    int rc;
    if ((rc = c->io_in.ensure(off + bytes))) return rc;
    char* base = static_cast<char*>(c->io_in.p);
    src[0] = base;
    src[1] = base + off;
    if (which & 1) AM_HIP(copy_on_stream(c, base, haystack, bytes, hipMemcpyHostToDevice));
    if (which & 2) AM_HIP(copy_on_stream(c, base + off, advance_src(haystack, len - (size_t)W), bytes, hipMemcpyHostToDevice));
    return AM_OK;
}

int match_edges_impl(const am_needle* hc, const void* hay, size_t len, int sample_format, const am_edge_params* ep, am_edge_hit* out,
                     bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = edge_prelude(h, hay, len, sample_format, ep, out);
    if (rc) return rc;
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const long long W = edge_geom(len, h->n, AM_EDGE_HEAD).W;
    const void* src[2] = {hay, advance_src(hay, len - (size_t)W)};
    if (device_io) {
        if ((rc = check_device_arg(hay, c->device, "am_match_edges_device: d_haystack: "))) return rc;
    } else if (W > 0 && needle_finite(h) && (rc = upload_spans(c, hay, len, W, 3, src))) {
        return rc;
    }
    return match_edges_one(edge_call(h, sample_format, ep), src, len, out);
}

int edge_scores_impl(const am_needle* hc, const void* hay, size_t len, int sample_format, int edge, const am_edge_params* ep, float* out,
                     size_t cap, size_t* n_out, bool device_io) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if (!hay || !n_out || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_edge_params(ep)) || (rc = check_format(sample_format)) || (rc = check_edge(edge))) return rc;
    if (len == 0) return fail(AM_ERR_INVALID_ARG, "len must be at least 1");
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (device_io && (rc = check_device_arg(hay, c->device, "am_edge_scores_device: d_haystack: "))) return rc;
    const EdgeGeom g = edge_geom(len, h->n, edge);
    *n_out = (size_t)g.W;
    if (cap < (size_t)g.W) return fail(AM_ERR_CAPACITY, "edge score output buffer too small");
    if (g.W == 0) return AM_OK;
    if (!needle_finite(h)) {
        for (long long j = 0; j < g.W; ++j) out[j] = std::nanf("");
        return AM_OK;
    }
    const void* src[2] = {hay, advance_src(hay, len - (size_t)g.W)};
    if (!device_io && (rc = upload_spans(c, hay, len, g.W, 1 << edge, src))) return rc;
    EdgeBufs b{};
    if ((rc = needle_scans(h)) || (rc = edge_reserve(c, g.W, &b))) return rc;
    if ((rc = edge_coarse_scores(edge_call(h, sample_format, ep), src[edge], g.W, edge, b))) return rc;
    return download(c, out, b.scores[edge], sizeof(float) * (size_t)g.W);
}

}  // namespace

}  // namespace am

// ---------------------------------------------------------------------------
using namespace am;

int am_edge_scores_len(size_t len, size_t s, int edge, size_t* n_lags, int64_t* first_lag) {
    if (!n_lags || !first_lag) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (len == 0 || s == 0) return fail(AM_ERR_INVALID_ARG, "len and s must be at least 1");
    int rc = check_edge(edge);
    if (rc) return rc;
    const EdgeGeom g = edge_geom(len, s, edge);
    *n_lags = (size_t)g.W;
    *first_lag = (int64_t)g.first;
    return AM_OK;
}

int am_edge_scores_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, int edge, const am_edge_params* ep,
                          float* out, size_t cap, size_t* n_out) {
    return edge_scores_impl(h, d_haystack, len, sample_format, edge, ep, out, cap, n_out, true);
}

int am_edge_scores(const am_needle* h, const void* haystack, size_t len, int sample_format, int edge, const am_edge_params* ep, float* out,
                   size_t cap, size_t* n_out) {
    return edge_scores_impl(h, haystack, len, sample_format, edge, ep, out, cap, n_out, false);
}

int am_match_edges_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_edge_params* ep,
                          am_edge_hit* out) {
    return match_edges_impl(h, d_haystack, len, sample_format, ep, out, true);
}

int am_match_edges(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_edge_params* ep, am_edge_hit* out) {
    return match_edges_impl(h, haystack, len, sample_format, ep, out, false);
}

int am_match_edges_batch_device(const am_needle* hc, const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                                const am_edge_params* ep, am_edge_hit* out) {
    am_needle* h = const_cast<am_needle*>(hc);
    int rc = check_needle(h);
    if (rc) return rc;
    if ((rc = check_edge_params(ep)) || (rc = check_format(sample_format))) return rc;
    if (n_hay == 0) return AM_OK;
    if (!d_haystacks || !lens || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    for (size_t i = 0; i < n_hay; ++i) {
        const std::string who = "am_match_edges_batch_device: haystack " + std::to_string(i) + ": ";
        if (!d_haystacks[i]) return fail(AM_ERR_INVALID_ARG, who + "null pointer");
        if (lens[i] == 0) return fail(AM_ERR_INVALID_ARG, who + "len must be at least 1");
        if ((rc = check_device_arg(d_haystacks[i], c->device, who.c_str()))) return rc;
    }
    const EdgeCall k = edge_call(h, sample_format, ep);
    for (size_t i = 0; i < n_hay; ++i) {
        const long long W = edge_geom(lens[i], h->n, AM_EDGE_HEAD).W;
        const void* src[2] = {d_haystacks[i], advance_src(d_haystacks[i], lens[i] - (size_t)W)};
        if ((rc = match_edges_one(k, src, lens[i], out + 2 * i))) return rc;
    }
    return AM_OK;
}
