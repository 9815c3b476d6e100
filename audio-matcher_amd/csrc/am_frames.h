// am_frames.h -- the packed f64 frame transform of am_bands.hip and am_envelope.hip: two real frames of F = 2^lf samples
// (8 <= lf <= 12), windowed, travel as z = x + i y through ONE F-point complex FFT in LDS (radix 2, decimation in time: the
// samples are stored bit-reversed, the spectrum comes out in order; both parities of lf alike) and are untangled into
// their own spectra.  The load loops stay in the kernels: they differ on purpose (bands keeps a non-finite sample and
// flags the hit, the envelope stores 0 and marks the frame).  Everything is inlined: the kernels keep their registers
// only while their steps stay interleaved as written (am_hit_device.h).  Included by those two files only.  band_table
// (am_bands.hip) builds the table of F on c's device on first use, on the host in f64, kept until am_shutdown: the Hann
// window w[i] = 0.5 - 0.5 cos(2 pi i / F) as tab[0 .. F), then the twiddles (cos, -sin)(2 pi k / F), k < F / 2, as pairs.
#pragma once

#include "am_internal.h"
#include "am_reduce.h"

namespace am {

int band_table(Ctx* c, int lf, const double** d_tab);
constexpr int kFrameThreads = 256;
constexpr int kFrameMaxF = 1 << 12;
constexpr int kFrameLds = kFrameMaxF + (kFrameMaxF >> 5) + (kFrameMaxF >> 10);   // one padded array of F doubles
constexpr int kFrameBins = (kFrameMaxF / 2) / kFrameThreads + 1;                 // bins per thread: k = tid + m * kFrameThreads <= F / 2

// Element i of an LDS array of 8-byte values, one pad per 32 and per 1024: the bit-reversed store of a frame (stride
// F / 2, F / 4, ...) and the butterflies of the first stages (stride 2, 4, ...) then spread over the banks.
__device__ __forceinline__ int lpad(int i) { return i + (i >> 5) + (i >> 10); }
__device__ __forceinline__ int frame_slot(int i, int lf) { return lpad((int)(__brev((unsigned)i) >> (32 - lf))); }   // of sample i, in re / im
// The transform of the samples stored at frame_slot: the barrier behind their stores, then the lf stages over re / im
// with a barrier behind each; afterwards Z[k] is at lpad(k).  tw[k] = (cos, -sin)(2 pi k / F), k < F / 2: the table from
// tab + F on.  Returns the OR of every thread's `bits` (what its samples were), which crosses the waves through wbits
// (kFrameThreads / 64 words) on the first barrier.
__device__ __forceinline__ unsigned frame_transform(double* re, double* im, const double2* __restrict__ tw, int lf, unsigned bits, unsigned* wbits) {
    const int tid = threadIdx.x, H = (1 << lf) >> 1;
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if ((tid & 63) == 0) wbits[tid >> 6] = bits;
    __syncthreads();
    for (int s = 1; s <= lf; ++s) {
        const int h = 1 << (s - 1);
        for (int b = tid; b < H; b += kFrameThreads) {
            const int pos = b & (h - 1);
            const int i = lpad(((b >> (s - 1)) << s) + pos), j = lpad(((b >> (s - 1)) << s) + pos + h);
            const double2 w = tw[pos << (lf - s)];
            const double ar = re[i], ai = im[i], br = re[j], bi = im[j];
            const double tr = w.x * br - w.y * bi, ti = w.x * bi + w.y * br;
            re[i] = ar + tr;
            im[i] = ai + ti;
            re[j] = ar - tr;
            im[j] = ai - ti;
        }
        __syncthreads();
    }
    unsigned any = 0;
#pragma unroll
    for (int i = 0; i < kFrameThreads / 64; ++i) any |= wbits[i];
    return any;
}
// bin k <= F / 2 of the two spectra: X[k] = (Z[k] + conj Z[F - k]) / 2, Y[k] = (Z[k] - conj Z[F - k]) / 2i
struct FrameBin { double xr, xi, yr, yi; };
__device__ __forceinline__ FrameBin frame_untangle(const double* re, const double* im, int F, int k) {
    const int p = lpad(k), q = lpad((F - k) & (F - 1));
    const double zr = re[p], zi = im[p], mr = re[q], mi = im[q];
    return FrameBin{0.5 * (zr + mr), 0.5 * (zi - mi), 0.5 * (zi + mi), 0.5 * (mr - zr)};
}
// one wave: the sum of src[lo .. hi) (unpadded) in every lane: lane l adds the bins lo + l, lo + l + 64, .., wave_sum the lanes
__device__ __forceinline__ double wave_bin_sum(const double* src, int lo, int hi) {
    double v = 0.0;
    for (int k = lo + ((int)threadIdx.x & 63); k < hi; k += 64) v += src[k];
    return wave_sum(v);
}

}  // namespace am
