// am_discover.hip -- needle discovery (am_discover*, am_probe_scores*, am_discover_regions; include/audiomatch.h,
// "needle discovery"): probes cut from recording A at a fixed hop are matched against recording B under NCC, every
// probe's score array is reduced on the device to its best candidate and an exact runner-up, and a host rule chains
// the probes that agree on one displacement into regions.
//
// Per call: A and B are down-mixed once, B's non-finite runs are listed once (haystack_prepare, am_best.hip), and ONE
// launch (probe_energy) computes every probe's energy, A's energy and the non-finite flags.  Per probe: the probe is
// copied into the context's probe buffer, an internal needle handle over that buffer computes the scores
// (prepared_scores, the step am_match_best and am_match_trace share) into the context's dense score buffer, and two
// launches reduce them:
//   * probe_slices: one wavefront per slice of AM_DISCOVER_SLICE scores (probe_span: the loads of wave_steps,
//     am_wave_steps.h, which the score traces share -- 16-byte loads, guarded 4-byte loads at the ragged head and tail,
//     four steps in flight -- and the lanes folded by a butterfly in registers) writes the slice's best candidate
//     outside the excluded range;
//   * probe_finish: one wavefront folds the partials to the best, then folds the partials of the slices that the zone
//     (best - separation, best + separation) does not touch, reads the at most two slices the zone covers partly again
//     with the zone excluded as well (slices wholly inside it hold no runner-up), and writes the record.
// So a score is read once per probe, and at most 2 AM_DISCOVER_SLICE scores a second time.  No atomics, no LDS; ties
// are decided by the offsets, so the order of the folds does not matter.  The records stay on the device until the
// call's single copy at the end.
#include "am_internal.h"
#include "am_reduce.h"
#include "am_wave_steps.h"

#include <climits>
#include <cmath>

namespace am {

namespace {

constexpr int kSlice = AM_DISCOVER_SLICE;
constexpr int kThreads = 256;        // four waves, four slices at a time
constexpr int kBlocks = 2048;        // blocks of the capped grid (8 per CU); the rest is strided
static_assert(sizeof(am_probe_hit) == 40, "am_probe_hit is 40 bytes, no padding");
static_assert(sizeof(am_region) == 56, "am_region is 56 bytes, no padding");
static_assert(kSlice % 1024 == 0, "a slice is whole steps from its start");

struct Cand { float v; long long o; };   // o < 0: none
struct SlicePart { float v; int o; };    // the best candidate of a slice, o from the slice's start (-1: none)

// b into the running best a: the larger score, ties (==, so -0.0 and +0.0 tie) to the lower offset
__device__ __forceinline__ void take_cand(Cand& a, const Cand& b) {
    if (b.o >= 0 && (a.o < 0 || b.v > a.v || (b.v == a.v && b.o < a.o))) a = b;
}
__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        Cand b;
        b.v = __shfl_xor(c.v, m, 64);
        b.o = __shfl_xor(c.o, m, 64);
        take_cand(c, b);
    }
    return c;
}

// One wavefront: the best candidate of the span p[0, len) (0 <= len <= kSlice; p at any 4-byte alignment) outside the
// two excluded ranges [x0, x1) and [y0, y1) of the span's own offsets.  Every lane of the wave must be here; the
// result (offset from p, -1: none) is complete in every lane.
__device__ __forceinline__ SlicePart probe_span(const float* __restrict__ p, int len, int x0, int x1, int y0, int y1) {
    const int a = wave_align(p);
    float v = 0.0f;
    int o = -1;
    // the lane's four floats of a step, in ascending offset (the first of equals stays)
    wave_steps(p, len, [&](int f0, const float (&w)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = w[i];
            const int j = f0 + i - a;
            const bool ok = x == x && !(j >= x0 && j < x1) && !(j >= y0 && j < y1);   // (a float outside the span reads as NaN)
            if (ok && (o < 0 || x > v)) { v = x; o = j; }
        }
    });
    const Cand c = wave_best(Cand{v, (long long)o});
    return SlicePart{c.v, (int)c.o};
}

// [lo, hi) of the array's offsets as offsets of the slice [s0, s0 + len), clamped into it
__device__ __forceinline__ void local_range(long long lo, long long hi, long long s0, int len, int* l0, int* l1) {
    *l0 = (int)std::min<long long>(std::max<long long>(lo - s0, 0), len);
    *l1 = (int)std::min<long long>(std::max<long long>(hi - s0, 0), len);
}

__global__ void __launch_bounds__(kThreads) probe_slices(const float* __restrict__ g, long long n, long long ex_lo, long long ex_hi,
                                                         long long nsl, SlicePart* __restrict__ parts) {
    const long long wave = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kThreads) >> 6;
    for (long long s = wave; s < nsl; s += nwaves) {
        const long long s0 = s * kSlice;
        const int len = (int)std::min<long long>(kSlice, n - s0);
        int x0, x1;
        local_range(ex_lo, ex_hi, s0, len, &x0, &x1);
        const SlicePart r = probe_span(g + s0, len, x0, x1, 0, 0);
        if ((threadIdx.x & 63) == 0) parts[s] = r;
    }
}

// One wavefront.  sep: 1 .. n.
__global__ void __launch_bounds__(64) probe_finish(const float* __restrict__ g, long long n, long long ex_lo, long long ex_hi, long long sep,
                                                   long long nsl, const SlicePart* __restrict__ parts, unsigned long long probe,
                                                   am_probe_hit* __restrict__ out) {
    const int lane = threadIdx.x;
    Cand best{0.0f, -1};
    for (long long s = lane; s < nsl; s += 64) {
        const SlicePart pt = parts[s];
        take_cand(best, Cand{pt.v, pt.o < 0 ? -1ll : s * kSlice + pt.o});
    }
    best = wave_best(best);
    Cand second{0.0f, -1};
    if (best.o >= 0) {
        // the zone: |j - best| < sep
        const long long z0 = std::max<long long>(best.o - sep + 1, 0), z1 = std::min<long long>(best.o + sep, n);
        for (long long s = lane; s < nsl; s += 64) {
            const long long s0 = s * kSlice, s1 = std::min<long long>(s0 + kSlice, n);
            if (s1 > z0 && s0 < z1) continue;   // touched by the zone
            const SlicePart pt = parts[s];
            take_cand(second, Cand{pt.v, pt.o < 0 ? -1ll : s0 + pt.o});
        }
        second = wave_best(second);
        // the slices the zone covers partly: the one that holds its first offset and the one that holds its last
        const long long sa = z0 / kSlice, sb = (z1 - 1) / kSlice;
        for (int k = 0; k < 2; ++k) {
            const long long s = k ? sb : sa;
            if (k && sb == sa) break;
            const long long s0 = s * kSlice, s1 = std::min<long long>(s0 + kSlice, n);
            if (s0 >= z0 && s1 <= z1) continue;   // wholly inside: no runner-up here
            const int len = (int)(s1 - s0);
            int x0, x1, y0, y1;
            local_range(ex_lo, ex_hi, s0, len, &x0, &x1);
            local_range(z0, z1, s0, len, &y0, &y1);
            const SlicePart pt = probe_span(g + s0, len, x0, x1, y0, y1);
            take_cand(second, Cand{pt.v, pt.o < 0 ? -1ll : s0 + pt.o});
        }
    }
    if (lane == 0) {
        const float nan = __uint_as_float(0x7FC00000u);
        am_probe_hit r;
        r.probe = probe;
        r.best = best.o >= 0 ? (uint64_t)best.o : 0;
        r.second = second.o >= 0 ? (uint64_t)second.o : 0;
        r.ncc = best.o >= 0 ? best.v : nan;
        r.ncc_second = second.o >= 0 ? second.v : nan;
        r.flags = (best.o >= 0 ? 0u : AM_PROBE_NO_BEST) | (second.o >= 0 ? 0u : AM_PROBE_NO_SECOND);
        r.reserved = 0u;
        *out = r;
    }
}

// Block b < n_probes * parts: part (b mod parts) of probe (b / parts), the share block_sumsq (am_reduce.h) gives that
// workgroup of sumsq_kernel (am_peaks.hip) over the probe's samples -- so the host's sum of a probe's parts in index order
// has the bits of the energy am_needle_create_device gives a needle made from the probe.  The other blocks: the same
// over all of A with `a_parts` workgroups, a non-finite sample counting as 0.  flag[b]: the block met a non-finite sample.
__global__ void __launch_bounds__(256) probe_energy(const float* __restrict__ a, long long len_a, long long L, long long H, long long n_probes,
                                                    int parts, int a_parts, double* __restrict__ sums, unsigned* __restrict__ flags) {
    __shared__ double part[4];
    __shared__ int bad[4];
    const long long b = blockIdx.x;
    const bool whole = b >= n_probes * parts;
    const long long pr = whole ? 0 : b / parts, blk = whole ? b - n_probes * parts : b - pr * parts;
    const float* __restrict__ x = whole ? a : a + pr * H;
    const long long n = whole ? len_a : L, stride = (long long)(whole ? a_parts : parts) * 256;
    const double t = block_sumsq(x, blk * 256, stride, n, whole, part, bad);
    if (threadIdx.x == 0) {
        sums[b] = t;
        flags[b] = (unsigned)(bad[0] | bad[1] | bad[2] | bad[3]);
    }
}

}  // namespace

// The record of the resident scores d_g[0, n) (n >= 1) into d_out, on the context's stream.  sep >= 1.
int probe_reduce(Ctx* c, const float* d_g, long long n, uint64_t ex_lo, uint64_t ex_hi, uint64_t sep, uint64_t probe, am_probe_hit* d_out) {
    const long long nsl = (n + kSlice - 1) / kSlice;
    int rc;
    if ((rc = c->disc_parts.ensure(sizeof(SlicePart) * (size_t)nsl))) return rc;
    const long long lo = (long long)std::min<uint64_t>(ex_lo, (uint64_t)n), hi = (long long)std::min<uint64_t>(ex_hi, (uint64_t)n);
    const long long sp = (long long)std::min<uint64_t>(sep, (uint64_t)n);   // (|j - best| < n for every pair)
    ProfScope ps(c, KN_DISCOVER, c->stream);
    const int grid = (int)std::max<long long>(1, std::min<long long>((nsl + 3) / 4, kBlocks));
    hipLaunchKernelGGL(probe_slices, dim3(grid), dim3(kThreads), 0, c->stream, d_g, n, lo, hi, nsl, (SlicePart*)c->disc_parts.p);
    AM_HIP(hipGetLastError());
    hipLaunchKernelGGL(probe_finish, dim3(1), dim3(64), 0, c->stream, d_g, n, lo, hi, sp, nsl, (const SlicePart*)c->disc_parts.p,
                       (unsigned long long)probe, d_out);
    AM_HIP(hipGetLastError());
    return AM_OK;
}

namespace {

am_probe_hit empty_record(uint64_t probe, uint32_t flags) {
    am_probe_hit r{};
    r.probe = probe;
    r.ncc = r.ncc_second = std::nanf("");
    r.flags = flags;
    return r;
}

int check_discover_params(const am_discover_params* dp) {
    if (!dp) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (dp->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_discover_params: reserved must be 0");
    if (dp->probe_len == 0) return fail(AM_ERR_INVALID_ARG, "am_discover_params: probe_len must be at least 1");
    if (dp->hop == 0) return fail(AM_ERR_INVALID_ARG, "am_discover_params: hop must be at least 1");
    if (dp->flags & ~AM_DISCOVER_SELF) return fail(AM_ERR_INVALID_ARG, "am_discover_params: unknown flags");
    if (!(dp->flags & AM_DISCOVER_SELF) && dp->exclude != 0)
        return fail(AM_ERR_INVALID_ARG, "am_discover_params: exclude needs AM_DISCOVER_SELF");
    if (dp->min_level_db != dp->min_level_db) return fail(AM_ERR_INVALID_ARG, "am_discover_params: min_level_db is NaN");
    return AM_OK;
}

size_t probes_of(size_t len_a, const am_discover_params* dp) {
    return len_a < dp->probe_len ? 0 : (size_t)((len_a - dp->probe_len) / dp->hop + 1);
}

// am_discover on resident recordings.  The caller holds the context's lock and has checked the arguments.
int discover_resident(Ctx* c, const void* d_a, size_t len_a, const void* d_b, size_t len_b, int sample_format, const am_discover_params* dp,
                      am_probe_hit* out, size_t cap, size_t* n_out) {
    const size_t P_all = probes_of(len_a, dp);
    *n_out = P_all;
    const size_t P = std::min(P_all, cap);
    const long long L = (long long)dp->probe_len, H = (long long)dp->hop;
    int rc;
    if (P > 0) {
        // recording A as f32 mono
        const float* a = static_cast<const float*>(d_a);
        if (sample_format == AM_FMT_S16_STEREO) {
            if ((rc = c->disc_a.ensure(len_a * sizeof(float)))) return rc;
            AM_HIP(launch_pcm_downmix(c->stream, static_cast<const int16_t*>(d_a), (long long)len_a, (float*)c->disc_a.p));
            a = (const float*)c->disc_a.p;
        }
        // every probe's energy, A's energy and the non-finite flags: one launch, one copy
        const int parts = sumsq_parts(L), a_parts = sumsq_parts((long long)len_a);
        const size_t blocks = P * (size_t)parts + (size_t)a_parts;
        // (one workgroup of 256 threads per part: a grid's threads must fit 32 bits)
        if (blocks > (size_t)(UINT32_MAX / 256))
            return fail(AM_ERR_INVALID_ARG, "am_discover: too many probes for one call (probe_len / 256 parts per probe, 2^24 in all): raise hop or pass A in pieces");
        if ((rc = c->disc_energy.ensure(blocks * (sizeof(double) + sizeof(unsigned))))) return rc;
        double* d_sums = (double*)c->disc_energy.p;
        unsigned* d_flags = (unsigned*)(d_sums + blocks);
        {
            ProfScope ps(c, KN_DISCOVER, c->stream);
            hipLaunchKernelGGL(probe_energy, dim3((unsigned)blocks), dim3(256), 0, c->stream, a, (long long)len_a, L, H, (long long)P, parts,
                               a_parts, d_sums, d_flags);
            AM_HIP(hipGetLastError());
        }
        std::vector<double> sums(blocks);
        std::vector<unsigned> flags(blocks);
        AM_HIP(hipMemcpyAsync(sums.data(), d_sums, blocks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if ((rc = download(c, flags.data(), d_flags, blocks * sizeof(unsigned)))) return rc;
        double e_a = 0.0;
        for (int k = 0; k < a_parts; ++k) e_a += sums[P * (size_t)parts + (size_t)k];
        const double e_ref = e_a * (double)L / (double)len_a, bound = e_ref * std::pow(10.0, -(double)dp->min_level_db / 10.0);
        // recording B: down-mixed and scanned for non-finite runs once
        HaySamples hb;
        const bool any_scores = len_b >= (size_t)L;
        if (any_scores && (rc = haystack_prepare(c, d_b, len_b, sample_format, c->best_mono, &hb))) return rc;
        const uint64_t sep = dp->separation ? dp->separation : dp->probe_len;
        if ((rc = c->disc_out.ensure(sizeof(am_probe_hit) * P))) return rc;
        if ((rc = c->disc_probe.ensure(sizeof(float) * (size_t)L))) return rc;
        am_probe_hit* d_rec = (am_probe_hit*)c->disc_out.p;
        std::vector<am_probe_hit> skipped(P);
        std::vector<char> is_skipped(P, 0);
        for (size_t i = 0; i < P; ++i) {
            const uint64_t p = (uint64_t)i * dp->hop;
            double e = 0.0;
            unsigned nf = 0;
            for (int k = 0; k < parts; ++k) { e += sums[i * (size_t)parts + (size_t)k]; nf |= flags[i * (size_t)parts + (size_t)k]; }
            uint32_t fl = 0;
            if (nf) fl = AM_PROBE_NONFINITE;
            else if (e == 0.0 || e < bound) fl = AM_PROBE_QUIET;
            else if (!any_scores) fl = AM_PROBE_NO_BEST | AM_PROBE_NO_SECOND;
            if (fl) { skipped[i] = empty_record(p, fl); is_skipped[i] = 1; continue; }
            // the probe as an internal needle handle over the probe buffer: the handle am_needle_create_device makes
            // from these samples, always NCC
            AM_HIP(hipMemcpyAsync(c->disc_probe.p, a + p, sizeof(float) * (size_t)L, hipMemcpyDeviceToDevice, c->stream));
            am_needle* h = new am_needle();
            h->ctx = c; h->d_needle = (float*)c->disc_probe.p; h->n = (size_t)L; h->owns_data = false;
            h->inv_autocorr = (float)(1.0 / e);
            h->energy = e;
            h->opt_score_norm = 1;
            const float* d_sc = nullptr;
            long long n = 0;
            rc = prepared_scores(h, snapshot_opts(h), hb, AM_SCALE_LIB, &d_sc, &n);
            if (!rc) {
                uint64_t ex_lo = 0, ex_hi = 0;
                if ((dp->flags & AM_DISCOVER_SELF) && dp->exclude) {
                    ex_lo = p >= dp->exclude ? p - dp->exclude + 1 : 0;
                    ex_hi = p + dp->exclude < p ? UINT64_MAX : p + dp->exclude;
                }
                rc = probe_reduce(c, d_sc, n, ex_lo, ex_hi, sep, p, d_rec + i);
            }
            am_needle_destroy(h);   // (waits for the stream: the probe buffer and the spectra are free for the next probe)
            if (rc) return rc;
        }
        if ((rc = download(c, out, d_rec, sizeof(am_probe_hit) * P))) return rc;
        for (size_t i = 0; i < P; ++i)
            if (is_skipped[i]) out[i] = skipped[i];
    }
    if (P_all > cap) return fail(AM_ERR_CAPACITY, "discover output buffer too small");
    return AM_OK;
}

int discover_check(const am_discover_params* dp, int sample_format, const void* a, size_t len_a, const void* b, size_t len_b,
                   am_probe_hit* out, size_t cap, size_t* n_out) {
    int rc = check_discover_params(dp);
    if (rc) return rc;
    if ((rc = check_format(sample_format))) return rc;
    if (!n_out || (!a && len_a) || (!b && len_b) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    return AM_OK;
}

int probe_scores_impl(int device, const float* scores, size_t n, uint64_t ex_lo, uint64_t ex_hi, uint64_t separation, am_probe_hit* out,
                      bool device_io) {
    if (!out || (!scores && n)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (separation == 0) return fail(AM_ERR_INVALID_ARG, "am_probe_scores: separation must be at least 1");
    if (device_io && (reinterpret_cast<uintptr_t>(scores) & 3)) return fail(AM_ERR_INVALID_ARG, "am_probe_scores: scores must be 4-byte aligned");
    Ctx* c = nullptr;
    int rc;
    if ((rc = get_ctx(device, &c))) return rc;
    if (n == 0) { *out = empty_record(0, AM_PROBE_NO_BEST | AM_PROBE_NO_SECOND); return AM_OK; }
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_scores = nullptr;
    if ((rc = resident_input(c, device_io, scores, sample_bytes(n), &d_scores, "am_probe_scores_device: d_scores: "))) return rc;
    if ((rc = c->disc_out.ensure(sizeof(am_probe_hit)))) return rc;
    if ((rc = probe_reduce(c, (const float*)d_scores, (long long)n, ex_lo, ex_hi, separation, 0, (am_probe_hit*)c->disc_out.p))) return rc;
    return download(c, out, c->disc_out.p, sizeof(am_probe_hit));
}

}  // namespace

}  // namespace am

// ---------------------------------------------------------------------------
using namespace am;

int am_discover_len(size_t len_a, const am_discover_params* dp, size_t* n_probes) {
    int rc = check_discover_params(dp);
    if (rc) return rc;
    if (!n_probes) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n_probes = probes_of(len_a, dp);
    return AM_OK;
}

static int discover_impl(int device, const void* a, size_t len_a, const void* b, size_t len_b, int sample_format,
                         const am_discover_params* dp, am_probe_hit* out, size_t cap, size_t* n_out, bool device_io) {
    int rc = discover_check(dp, sample_format, a, len_a, b, len_b, out, cap, n_out);
    if (rc) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    *n_out = 0;
    if (len_a < dp->probe_len) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (device_io) {
        if ((rc = check_device_arg(a, c->device, "am_discover_device: d_a: "))) return rc;
        if (len_b && (rc = check_device_arg(b, c->device, "am_discover_device: d_b: "))) return rc;
    } else {
        // both recordings side by side in the context's input buffer, sized once, B at a 256-byte boundary
        const size_t off_b = (sample_bytes(len_a) + 255) & ~(size_t)255;
        if ((rc = c->io_in.ensure(off_b + sample_bytes(len_b)))) return rc;
        char* base = static_cast<char*>(c->io_in.p);
        AM_HIP(copy_on_stream(c, base, a, sample_bytes(len_a), hipMemcpyHostToDevice));
        if (len_b) AM_HIP(copy_on_stream(c, base + off_b, b, sample_bytes(len_b), hipMemcpyHostToDevice));
        a = base;
        b = base + off_b;
    }
    return discover_resident(c, a, len_a, b, len_b, sample_format, dp, out, cap, n_out);
}

int am_discover_device(int device, const void* d_a, size_t len_a, const void* d_b, size_t len_b, int sample_format,
                       const am_discover_params* dp, am_probe_hit* out, size_t cap, size_t* n_out) {
    return discover_impl(device, d_a, len_a, d_b, len_b, sample_format, dp, out, cap, n_out, true);
}

int am_discover(int device, const void* a, size_t len_a, const void* b, size_t len_b, int sample_format, const am_discover_params* dp,
                am_probe_hit* out, size_t cap, size_t* n_out) {
    return discover_impl(device, a, len_a, b, len_b, sample_format, dp, out, cap, n_out, false);
}

int am_probe_scores(int device, const float* scores, size_t n, uint64_t ex_lo, uint64_t ex_hi, uint64_t separation, am_probe_hit* out) {
    return probe_scores_impl(device, scores, n, ex_lo, ex_hi, separation, out, false);
}

int am_probe_scores_device(int device, const float* d_scores, size_t n, uint64_t ex_lo, uint64_t ex_hi, uint64_t separation,
                           am_probe_hit* out) {
    return probe_scores_impl(device, d_scores, n, ex_lo, ex_hi, separation, out, true);
}

// Pure host: the region rule (include/audiomatch.h).
int am_discover_regions(const am_probe_hit* hits, size_t n, const am_discover_params* dp, const am_region_params* rp, am_region* out,
                        size_t cap, size_t* n_out) {
    int rc = check_discover_params(dp);
    if (rc) return rc;
    if (!rp || !n_out || (!hits && n) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (rp->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_region_params: reserved must be 0");
    if (rp->flags & ~AM_REGION_FOLD) return fail(AM_ERR_INVALID_ARG, "am_region_params: unknown flags");
    if ((rp->flags & AM_REGION_FOLD) && !(dp->flags & AM_DISCOVER_SELF))
        return fail(AM_ERR_INVALID_ARG, "am_region_params: AM_REGION_FOLD needs AM_DISCOVER_SELF");
    if (rp->min_ncc != rp->min_ncc || rp->max_second != rp->max_second)
        return fail(AM_ERR_INVALID_ARG, "am_region_params: min_ncc / max_second is NaN");
    *n_out = 0;
    for (size_t i = 1; i < n; ++i)
        if (!(hits[i].probe > hits[i - 1].probe)) return fail(AM_ERR_INVALID_ARG, "am_discover_regions: hits[" + std::to_string(i) + "].probe does not ascend");
    auto good = [&](const am_probe_hit& r) {
        if (r.flags & ~AM_PROBE_NO_SECOND) return false;
        if (!(r.ncc >= rp->min_ncc)) return false;
        if (rp->max_second > 0.0f && !(r.flags & AM_PROBE_NO_SECOND) && !((double)r.ncc_second <= (double)rp->max_second * (double)r.ncc)) return false;
        return true;
    };
    auto disp = [](const am_probe_hit& r) { return (int64_t)(r.best - r.probe); };
    auto absdiff = [](int64_t x, int64_t y) { return x > y ? (uint64_t)x - (uint64_t)y : (uint64_t)y - (uint64_t)x; };
    std::vector<am_region> regs;
    std::vector<size_t> chain;   // indices of the open chain's good probes
    auto close = [&]() {
        if (!chain.empty() && chain.size() >= (size_t)rp->min_good) {
            am_region g{};
            const am_probe_hit &f = hits[chain.front()], &l = hits[chain.back()];
            g.a_start = f.probe;
            g.length = l.probe + dp->probe_len - f.probe;
            std::vector<int64_t> ds;
            double sum = 0.0;
            float mn = 0.0f, ws = std::nanf("");
            for (size_t k = 0; k < chain.size(); ++k) {
                const am_probe_hit& r = hits[chain[k]];
                ds.push_back(disp(r));
                sum += (double)r.ncc;
                if (k == 0 || r.ncc < mn) mn = r.ncc;
                if (!(r.flags & AM_PROBE_NO_SECOND) && (ws != ws || r.ncc_second > ws)) ws = r.ncc_second;
            }
            std::sort(ds.begin(), ds.end());
            g.displacement = ds[(ds.size() - 1) / 2];
            g.first = (uint64_t)chain.front();
            g.count = (uint32_t)(chain.back() - chain.front() + 1);
            g.good = (uint32_t)chain.size();
            g.mean_ncc = sum / (double)chain.size();
            g.min_ncc = mn;
            g.worst_second = ws;
            regs.push_back(g);
        }
        chain.clear();
    };
    size_t gap = 0;
    for (size_t i = 0; i < n; ++i) {
        if (good(hits[i])) {
            if (!chain.empty() && absdiff(disp(hits[i]), disp(hits[chain.back()])) > rp->tolerance) close();
            chain.push_back(i);
            gap = 0;
        } else if (!chain.empty() && ++gap > (size_t)rp->max_gap) {
            close();
        }
    }
    close();
    if (rp->flags & AM_REGION_FOLD) {
        std::vector<am_region> kept;
        for (const am_region& r : regs) {
            bool drop = false;
            if (r.displacement < 0)
                for (const am_region& k : kept) {
                    if (k.displacement <= 0) continue;
                    const int64_t s = k.displacement + r.displacement;
                    if ((uint64_t)(s < 0 ? -s : s) > rp->tolerance) continue;
                    const uint64_t k0 = k.a_start + (uint64_t)k.displacement, k1 = k0 + k.length;
                    if (k0 < r.a_start + r.length && r.a_start < k1) { drop = true; break; }
                }
            if (!drop) kept.push_back(r);
        }
        regs.swap(kept);
    }
    return hand_back(regs, out, cap, n_out, "region output buffer too small");
}
