// am_wave_steps.h -- how ONE wavefront reads a span of scores (am_trace.hip, am_discover.hip): the loads, their bounds
// and their order, written once.
//
// The wave reads steps of 256 scores from the 16-byte boundary at or below the span's start: with a = (address of the
// span's start / 4) mod 4, lane l holds the four consecutive floats at 4l - a .. 4l - a + 3 of the step, one 16-byte
// load where all four lie inside the span and guarded 4-byte loads at the ragged head and tail; a float outside the
// span is handed over as NaN and is never read.  The first step (its head may be ragged), then four whole steps at a
// time with their loads in flight together (one load per wave in flight leaves the kernel waiting for memory latency),
// then what is left.  take(f0, v): the lane's floats v[i] at offsets f0 + i - a of the span (wave_align(p) = a; the
// offset may be negative in the first step), called in ascending f0 per lane.  Every lane of the wave must be here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace am {

// a: how many floats the span's start lies behind a 16-byte boundary
__device__ __forceinline__ int wave_align(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

template <class Take>
__device__ __forceinline__ void wave_steps(const float* __restrict__ p, int len, Take take) {
    const int lane = threadIdx.x & 63;
    const int a = wave_align(p);
    const float* __restrict__ base = p - a;     // 16-byte aligned; floats before p are never read
    const int end = a + len;                    // floats of `base` the span ends at
    // one step with its ragged ends guarded
    auto step = [&](int f0) {
        float v[4];
        if (f0 >= a && f0 + 4 <= end) {
            const float4 w = *reinterpret_cast<const float4*>(base + f0);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (f0 + i >= a && f0 + i < end) ? base[f0 + i] : __uint_as_float(0x7FC00000u);
        }
        take(f0, v);
    };
    int f0 = 4 * lane;
    if (f0 < end) { step(f0); f0 += 256; }
    for (; f0 + 3 * 256 + 4 <= end; f0 += 4 * 256) {
        float4 w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = *reinterpret_cast<const float4*>(base + f0 + 256 * k);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v[4] = {w[k].x, w[k].y, w[k].z, w[k].w};
            take(f0 + 256 * k, v);
        }
    }
    for (; f0 < end; f0 += 256) step(f0);
}

}  // namespace am
