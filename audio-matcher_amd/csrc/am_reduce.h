// am_reduce.h -- the sums and scans of a wave and of a workgroup, each written once.  The library's results are promised
// bit for bit (the call forms of a family agree, a probe's energy has a needle's bits): that holds while kernels that add
// the same values add them in the same order.  The orders are written down here and nowhere else; cross-lane moves of
// 64-bit values are HIP's own.  Included by am_hit_device.h, am_frames.h and the .hip files outside the per-hit families.
#pragma once

#include <hip/hip_runtime.h>

namespace am {

// the sum over the wave by an xor butterfly with the offsets 32, 16, .. 1, complete in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T t) {
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}
// The workgroup sum of NV values per thread, for a workgroup of THREADS: wave_sums adds value k over each wave and lane 0
// writes the wave's sum to ws[k][wave]; after a barrier, add_waves(ws[k]) adds the waves of one value to 0 in ascending
// order.  Two calls on one ws need a barrier between the reads and the next writes.
template <int THREADS, int NV, typename T>
__device__ __forceinline__ void wave_sums(const T (&v)[NV], T (*ws)[THREADS / 64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const T t = wave_sum(v[k]);
        if (lane == 0) ws[k][w] = t;
    }
}
template <int THREADS, typename T>
__device__ __forceinline__ T add_waves(const T (&row)[THREADS / 64]) {
    T t = 0;
    for (int i = 0; i < THREADS / 64; ++i) t += row[i];
    return t;
}
// one value per thread, barrier included: every thread gets the sum.  ws: THREADS / 64 values.
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T* ws) {
    typedef T Row[THREADS / 64];
    const T one[1] = {v};
    wave_sums<THREADS>(one, reinterpret_cast<Row*>(ws));
    __syncthreads();
    return add_waves<THREADS>(*reinterpret_cast<Row*>(ws));
}
// The second order: the four wave sums of a workgroup of 256 added as (p0 + p1) + (p2 + p3).  A needle's `energy` is
// added so (sumsq_kernel, am_peaks.hip), hence every score_norm score and every per-hit record that divides by it, and
// every discovery probe (probe_energy, am_discover.hip), whose energy must have the bits of a needle made from it.
__device__ __forceinline__ double add_waves_pairwise(const double (&p)[4]) { return (p[0] + p[1]) + (p[2] + p[3]); }
// A workgroup's (256 threads) share of sum x[i]^2 in f64 over i = first + tid, + stride, .. below n: a thread adds its
// squares in ascending i, the wave by wave_sum, the waves pairwise; every thread gets the sum.  zero_nonfinite: a
// non-finite sample counts as 0.  bad: null, or 4 words whose OR tells afterwards whether the workgroup met one.
__device__ __forceinline__ double block_sumsq(const float* __restrict__ x, long long first, long long stride, long long n, bool zero_nonfinite,
                                              double (&part)[4], int* bad) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc = 0.0;
    int nf = 0;
    for (long long i = first + threadIdx.x; i < n; i += stride) {
        const float f = x[i];
        const bool fin = fabsf(f) <= __FLT_MAX__;
        nf |= !fin;
        const double v = (zero_nonfinite && !fin) ? 0.0 : (double)f;
        acc += v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) part[w] = acc;
    if (bad) {
        for (int off = 32; off > 0; off >>= 1) nf |= __shfl_xor(nf, off, 64);
        if (lane == 0) bad[w] = nf;
    }
    __syncthreads();
    return add_waves_pairwise(part);
}
// the wave's inclusive scan: lane l gets v of the lanes 0 .. l, added over the distances d = 1, 2, .. 32 (from lane l - d)
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if ((int)(threadIdx.x & 63) >= d) v += o;
    }
    return v;
}
// The workgroup's (THREADS) inclusive scan of a sequence of n values that load(k) gives and store(k, sum) takes, k = 0
// .. n - 1.  Thread i takes a contiguous run; its start value is the wave's exclusive scan of the runs before plus the
// totals of the waves before (ws: THREADS / 64 values, free again on return).  Every value stored is a sum of the loaded
// values, no subtraction.  load(k) is called twice per k and must give the same value both times.
template <int THREADS, class Load, class Store>
__device__ __forceinline__ void block_scan_with(int n, double* ws, Load load, Store store) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (n + THREADS - 1) / THREADS;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    double s = 0.0;
    for (int q = lo; q < hi; ++q) s += load(q);
    const double incl = wave_scan_inclusive(s);
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    double run = 0.0;
    for (int i = 0; i < w; ++i) run += ws[i];
    run += excl;
    for (int q = lo; q < hi; ++q) {
        run += load(q);
        store(q, run);
    }
    __syncthreads();
}
// In-place inclusive scan of buf[0 .. n): prefix sums (REV = false) or suffix sums (REV = true)
template <int THREADS, bool REV>
__device__ __forceinline__ void block_scan(double* buf, int n, double* ws) {
    block_scan_with<THREADS>(
        n, ws, [&](int q) { return buf[REV ? n - 1 - q : q]; }, [&](int q, double v) { buf[REV ? n - 1 - q : q] = v; });
}

}  // namespace am
