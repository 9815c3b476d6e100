// am_mask.hip -- the per-hit record of a masked handle (am_hit_mask*, include/audiomatch.h "masked needles"): for a hit
// at t, the handle's needle n (gap samples +0), the original gap samples o and the haystack's samples x, in f64:
//   over the kept samples   c_k = sum x[t + i] n[i],  E_x^M = sum x[t + i]^2
//   over the gap samples    c_g = sum x[t + i] o[i],  E_x,gaps = sum x[t + i]^2,  E_n,gaps = sum o[i]^2
// and from those the exact masked NCC, the gain, the kept level, the NCC of the gaps against the original and the level of
// what lies in the gaps against what the needle would put there.
//
// Two kernels on the context's stream, the shape of am_hits.hip's:
//   mask_slices    one workgroup per slice of kHitSlice needle samples of one hit (blockIdx.x = slice, blockIdx.y = hit):
//                  every thread adds its samples' products to the kept or the gap sums (a sample is kept when a kept
//                  span of the handle's table holds it), the workgroup adds them (wave_sums, add_waves) and writes one
//                  partial record (kMaskSums doubles, one 64-bit store each, and a flag word)
//   mask_combine   one wave per hit: lane 0 adds the hit's partials in slice order (sum_slices) and writes its am_mask_hit
// A hit's record depends on its handle, the samples under it and the floor only: slices start at multiples of kHitSlice
// of the needle and every reduction runs in the fixed order am_hit_device.h and am_reduce.h state, so the three call
// forms agree bit for bit, whatever else a call holds.
#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskPer = kHitSlice / kMaskThreads;   // needle samples per thread and slice
static_assert(kHitSlice % kMaskThreads == 0, "slice must split evenly over the workgroup");

template <int KIND>
__global__ __launch_bounds__(kMaskThreads) void mask_slices_kernel(const MaskDesc* __restrict__ hits, long long hit0,
                                                                   double* __restrict__ parts, unsigned* __restrict__ pflags) {
    __shared__ double ws[kMaskSums][kMaskThreads / 64];
    const MaskDesc d = hits[hit0 + blockIdx.y];
    const long long i0 = (long long)blockIdx.x * kHitSlice;
    if (i0 >= d.s) return;   // (a shorter needle than the launch's longest: whole workgroups leave together)
    const int tid = threadIdx.x;
    const int m = (int)min((long long)kHitSlice, d.s - i0);
    double v[kMaskSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int bad_kept = 0, bad_gap = 0;
    for (int r = 0; r < kMaskPer; ++r) {
        const int q = tid + r * kMaskThreads;
        if (q >= m) break;
        const long long i = i0 + q;   // (0 <= i < s: inside the needle, and t + i inside the haystack -- the host checks t + s <= len)
        bool kept = d.n_kept == 0;
        for (int k = 0; k < d.n_kept; ++k) kept |= i >= d.kept[2 * k] && i < d.kept[2 * k + 1];
        const float x = hit_sample<KIND>(d.win, i);
        const double dx = (double)x;
        if (kept) {
            const float n = ((gfloat*)d.needle)[i];
            v[0] += dx * (double)n;   // (a product of two f32 values is exact in f64)
            v[1] += dx * dx;
            bad_kept |= !__builtin_isfinite(x) || !__builtin_isfinite(n);
        } else {
            const float o = ((gfloat*)d.orig)[i];
            const double dn = (double)o;
            v[2] += dx * dn;
            v[3] += dx * dx;
            v[4] += dn * dn;
            bad_gap |= !__builtin_isfinite(x) || !__builtin_isfinite(o);
        }
    }
    wave_sums<kMaskThreads>(v, ws);
    const int any_kept = __syncthreads_or(bad_kept);
    const int any_gap = __syncthreads_or(bad_gap);
    // one 64-bit store per lane: no record leaves as one wide store
    const long long p = d.part0 + blockIdx.x;
    if (tid < kMaskSums) parts[kMaskSums * p + tid] = add_waves<kMaskThreads>(ws[tid]);
    else if (tid == kMaskSums) pflags[p] = (any_kept ? 1u : 0u) | (any_gap ? 2u : 0u);
}

__global__ __launch_bounds__(64) void mask_combine_kernel(const MaskDesc* __restrict__ hits, const double* __restrict__ parts,
                                                          const unsigned* __restrict__ pflags, am_mask_hit* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const long long h = blockIdx.x;
    const MaskDesc d = hits[h];
    const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
    const double ck = sum_slices(parts, kMaskSums, d.part0, ns, 0), ek = sum_slices(parts, kMaskSums, d.part0, ns, 1);
    const double cg = sum_slices(parts, kMaskSums, d.part0, ns, 2), xg = sum_slices(parts, kMaskSums, d.part0, ns, 3);
    const double ng = sum_slices(parts, kMaskSums, d.part0, ns, 4);
    const unsigned bad = or_flags(pflags, d.part0, ns, 0, 1);
    const float nan = __builtin_nanf("");
    am_mask_hit r;
    r.flags = 0;
    if (bad & 1u) {
        r.flags = AM_MASK_NONFINITE;
        r.ncc = r.gain = r.kept_db = r.ncc_gaps = r.gaps_db = nan;
    } else {
        bool below;
        r.ncc = (float)ncc_or_floor(ck, d.en, ek, d.thr, &below);
        if (below) r.flags |= AM_MASK_BELOW_FLOOR;
        const double gain = d.en > 0.0 ? ck / d.en : 0.0;
        r.gain = (float)gain;
        r.kept_db = level_db(ek, d.en);
        if (d.n_kept == 0) {
            r.flags |= AM_MASK_NO_GAPS;
            r.ncc_gaps = r.gaps_db = nan;
        } else if (bad & 2u) {
            r.flags |= AM_MASK_GAPS_NONFINITE;
            r.ncc_gaps = r.gaps_db = nan;
        } else {
            if (xg == 0.0) r.flags |= AM_MASK_GAPS_SILENT;
            r.ncc_gaps = (xg == 0.0 || ng == 0.0) ? 0.0f : (float)(cg / sqrt(ng * xg));
            r.gaps_db = level_db(xg, gain * gain * ng);
        }
    }
    am_mask_hit* o = out + h;
    o->ncc = r.ncc;
    o->gain = r.gain;
    o->kept_db = r.kept_db;
    o->ncc_gaps = r.ncc_gaps;
    o->gaps_db = r.gaps_db;
    o->flags = r.flags;
}

}  // namespace

hipError_t launch_hit_mask(hipStream_t st, const MaskDesc* d_hits, long long n, long long max_slices, int kind, double* parts,
                           unsigned* pflags, am_mask_hit* d_out) {
    if (n <= 0) return hipSuccess;
    const hipError_t e = for_each_grid_y(n, [&](long long h0, unsigned nh) {
        const dim3 grid((unsigned)max_slices, nh);
        if (kind) hipLaunchKernelGGL(mask_slices_kernel<1>, grid, dim3(kMaskThreads), 0, st, d_hits, h0, parts, pflags);
        else hipLaunchKernelGGL(mask_slices_kernel<0>, grid, dim3(kMaskThreads), 0, st, d_hits, h0, parts, pflags);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mask_combine_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, (const double*)parts, (const unsigned*)pflags, d_out);
    return hipGetLastError();
}

namespace {

int mask_hits(Ctx* c, std::vector<MaskDesc>& hits, am_mask_hit* const* out) {
    long long total = 0, max_slices = 0;
    for (MaskDesc& d : hits) {
        const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
        d.part0 = total;
        total += ns;
        max_slices = std::max(max_slices, ns);
    }
    return hit_round_trip(c, hits, kMaskSums * sizeof(double), (size_t)total, 1, out,
                          [&](const MaskDesc* tab, double* parts, unsigned* pflags, am_mask_hit* d_out) {
                              return launch_hit_mask(c->stream, tab, (long long)hits.size(), max_slices, hits[0].kind, parts, pflags, d_out);
                          },
                          KN_MASK);
}

// am_hit_mask*: no parameters; a hit at t reads [t, t + S)
struct MaskFamily {
    typedef MaskDesc Desc;
    typedef am_mask_hit Rec;
    const void* params() const { return this; }
    size_t recs() const { return 1; }
    int check_call() const { return AM_OK; }
    int check(const am_needle*, long long) const { return AM_OK; }
    double floor(const am_needle* h) const { return hit_floor(h); }
    int desc(const am_needle* h, const void* hay, size_t len, int sample_format, const am_peak& pk, double thr, const HitWhere& where,
             MaskDesc* d) const {
        HitDesc hd{};
        const int rc = hit_desc(h, hay, len, sample_format, pk, thr, where, &hd);   // (the refusal and its message are am_hit_scores')
        if (rc) return rc;
        d->win = hd.win; d->needle = hd.needle; d->s = hd.s; d->kind = hd.kind; d->en = hd.en; d->thr = hd.thr; d->part0 = 0;
        d->orig = h->d_gap_orig;
        d->kept = h->gaps.empty() ? nullptr : h->d_kept;
        d->n_kept = h->gaps.empty() ? 0 : h->n_kept;
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const { return HitRange{t, std::min(len, t + h->n)}; }
    int score(Ctx* c, std::vector<MaskDesc>& hits, am_mask_hit* const* out) const { return mask_hits(c, hits, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_mask(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_peak* peaks, size_t n, am_mask_hit* out) {
    return hit_call(MaskFamily{}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_mask_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_peak* peaks, size_t n,
                       am_mask_hit* out) {
    return hit_call(MaskFamily{}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_mask_batch_device(const am_needle* const* needles, size_t n_needles, const void* const* d_haystacks, const size_t* lens,
                             size_t n_hay, int sample_format, const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                             am_mask_hit* out) {
    return hit_call_batch(MaskFamily{}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair, n_peaks, out);
}

}  // extern "C"
