// am_hit_device.h -- the device steps the per-hit kernels share (am_hits.hip, am_segments.hip, am_channel.hip,
// am_stereo.hip, am_warp.hip, am_significance.hip, am_bands.hip, am_mask.hip), and the host loop that launches them.  The families
// promise results that are bit for bit the same across call forms, and some are checked against each other: that holds
// while every one of them adds in the same order.  The order is written down here, the workgroup sum's in am_reduce.h, and
// nowhere else (am_bands.hip: the combine's sums, level_db and the host loop).  Included by those .hip files only.
#pragma once

#include <algorithm>

#include "am_kernels.h"
#include "am_reduce.h"

namespace am {

// ---- staging a slice in LDS ----------------------------------------------------------------------------------------
// LDS index of staged sample q where a work item reads 16 consecutive samples: one word of padding per 16, so that lanes
// are 17 words apart and the reads are free of bank conflicts
__device__ __forceinline__ int pad16(int q) { return q + (q >> 4); }
struct StageFlat { __device__ __forceinline__ int operator()(int q) const { return q; } };
struct StagePad16 { __device__ __forceinline__ int operator()(int q) const { return pad16(q); } };
struct StageAlone { template <typename... A> __device__ __forceinline__ void operator()(A...) const {} };   // no callback

// xs[at(q)] = x[u0 + q] for q < cnt + extra (0 beyond, and where u0 + q is outside [ulo, uhi): the hit reads no sample
// there), for a slice of THREADS * PER samples and extra <= THREADS, in two steps so that every load of the workgroup is
// in flight before the first LDS store.  stage_load: thread tid loads q = tid + k THREADS (k < PER) into xv[k], the first
// `extra` threads q = THREADS * PER + tid into xt as well (0 for the others); with(k, q) runs beside load k, for the
// caller's own load at that index (its needle sample).  stage_store: the LDS stores, no barrier; with(q, x) runs beside
// the store of sample q, for the caller's non-finite test (the families' rules differ).  Both callbacks sit inside the
// loops because the compiler keeps the slice kernels' registers at their numbers only with the steps interleaved so.
template <int KIND, int THREADS, int PER, typename WITH = StageAlone>
__device__ __forceinline__ void stage_load(const void* win, long long u0, int cnt, int extra, long long ulo, long long uhi,
                                           float (&xv)[PER], float& xt, WITH with = WITH{}) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int q = tid + k * THREADS;
        const long long u = u0 + q;
        xv[k] = q < cnt + extra && u >= ulo && u < uhi ? hit_sample<KIND>(win, u) : 0.0f;
        with(k, q);
    }
    xt = 0.0f;
    if (tid < extra) {
        const int q = THREADS * PER + tid;
        const long long u = u0 + q;
        xt = q < cnt + extra && u >= ulo && u < uhi ? hit_sample<KIND>(win, u) : 0.0f;
    }
}
template <int THREADS, int PER, typename AT, typename WITH = StageAlone>
__device__ __forceinline__ void stage_store(AT at, float* xs, int extra, const float (&xv)[PER], float xt, WITH with = WITH{}) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        xs[at(tid + k * THREADS)] = xv[k];
        with(tid + k * THREADS, xv[k]);
    }
    if (tid < extra) {
        xs[at(THREADS * PER + tid)] = xt;
        with(THREADS * PER + tid, xt);
    }
}

// acc[l] += sum_{j < PER} xs[pad16(q0 + j + l)] nv[j] for l < NL, in f64 (a product of two f32 values is exact there): the
// PER + NL - 1 staged samples go to registers once, then j ascends, and for each j the lags ascend
template <int NL, int PER>
__device__ __forceinline__ void lag_dot(const float* xs, const float (&nv)[PER], int q0, double* acc) {
    double xd[PER + NL - 1];
#pragma unroll
    for (int j = 0; j < PER + NL - 1; ++j) xd[j] = (double)xs[pad16(q0 + j)];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const double dn = (double)nv[j];
#pragma unroll
        for (int l = 0; l < NL; ++l) acc[l] += xd[j + l] * dn;
    }
}

// ---- combining the partial records ---------------------------------------------------------------------------------
// Column k of the ns partial records (nv values each) from record p0 on: added to 0 in slice order, by one lane.
// hit_combine and warp_combine add in this order with loops of their own (their time is this loop; they say why).
template <typename T>
__device__ __forceinline__ T sum_slices(const T* __restrict__ parts, int nv, long long p0, long long ns, int k) {
    T t = 0;
    for (long long i = 0; i < ns; ++i) t += parts[nv * (p0 + i) + k];
    return t;
}
// the OR of pflags[p0 + i] over i = lane, lane + stride, .. below n: one lane's share, the caller ORs the lanes
__device__ __forceinline__ unsigned or_flags(const unsigned* __restrict__ pflags, long long p0, long long n, int lane, int stride) {
    unsigned b = 0;
    for (long long i = lane; i < n; i += stride) b |= pflags[p0 + i];
    return b;
}

// The vertex of the parabola through (-1, a), (0, b), (1, c), clamped to [-0.5, 0.5]: 0.5 (a - c) / den with
// den = a - 2 b + c, if den < 0 (*refined); 0 otherwise.
__device__ __forceinline__ double parabola_vertex(double a, double b, double c, bool* refined) {
    const double den = a - 2.0 * b + c;
    *refined = den < 0.0;
    return *refined ? fmin(fmax(0.5 * (a - c) / den, -0.5), 0.5) : 0.0;
}
// The lag of the largest cc[l] (|cc[l]| for ABS), l = -r .. r.  Candidates in the order 0, -1, 1, -2, 2, ..; a later one
// replaces an earlier one only if strictly larger: ties go to the smaller |l|, then to the negative lag.
template <bool ABS>
__device__ __forceinline__ int pick_lag(const double* cc, int r) {
    int ls = 0;
    for (int k = 1; k <= r; ++k) {
        if (ABS ? fabs(cc[-k]) > fabs(cc[ls]) : cc[-k] > cc[ls]) ls = -k;
        if (ABS ? fabs(cc[k]) > fabs(cc[ls]) : cc[k] > cc[ls]) ls = k;
    }
    return ls;
}
// ls plus the vertex through cc[ls - 1 .. ls + 1] (their magnitudes for ABS); not refined at the ends of the range
template <bool ABS>
__device__ __forceinline__ double refine_lag(const double* cc, int r, int ls, bool* refined) {
    *refined = false;
    if (r == 0 || ls == r || ls == -r) return (double)ls;
    const double a = cc[ls - 1], b = cc[ls], c = cc[ls + 1];
    return (double)ls + (ABS ? parabola_vertex(fabs(a), fabs(b), fabs(c), refined) : parabola_vertex(a, b, c, refined));
}

// b / sqrt(en ew), or 0 with *below where the window's energy ew is 0 or under the floor thr
__device__ __forceinline__ double ncc_or_floor(double b, double en, double ew, double thr, bool* below) {
    *below = ew == 0.0 || ew < thr;
    return *below ? 0.0 : b / sqrt(en * ew);
}
// 10 log10(ew / en): -inf for ew = 0, +inf for en = 0 < ew
__device__ __forceinline__ float level_db(double ew, double en) {
    return ew == 0.0 ? -__builtin_inff() : (float)(10.0 * log10(ew / en));
}

// ---- host ----------------------------------------------------------------------------------------------------------
// launch(g0, ny) for the chunks [g0, g0 + ny) of n grid rows, ny <= kHitMaxGridY (more rows than one grid column holds:
// a few launches); stops at the first launch error
template <typename F>
inline hipError_t for_each_grid_y(long long n, F launch) {
    for (long long g0 = 0; g0 < n; g0 += kHitMaxGridY) {
        launch(g0, (unsigned)std::min<long long>(kHitMaxGridY, n - g0));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace am
