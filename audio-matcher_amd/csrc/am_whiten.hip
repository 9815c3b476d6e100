// am_whiten.hip -- spectral whitening (am_lag_products*, am_whiten_taps, am_fir*, am_needle_create_filtered;
// include/audiomatch.h): the lag products r[k] = sum_i x~[i] x~[i - k] of a signal, the prediction-error filter they
// give (Levinson-Durbin, pure host) and a short causal FIR filter y[k] = sum_j taps[j] x[lead + k - j] that the needle
// and its haystacks pass through before they are correlated.
//
// lag_products   One workgroup per block of kLagBlock samples.  The block and the kLagHist samples in front of it (the
//                previous block's; zeros in front of sample 0) are staged in LDS once, with 16-byte coalesced loads
//                when the pointer allows, i16 stereo frames down-mixed and non-finite samples zeroed on the way.  Work
//                item t takes the samples 4 (t + 256 m) .. + 3, m = 0 .. 7, of the block.  The lags run in chunks of
//                kLagChunk: for a chunk the work item reads its four samples and the aligned 12-sample window behind
//                them (three 16-byte LDS reads) and adds the 32 products to 8 f64 accumulators, so 65 accumulators
//                never live at once.  A product of two f32 values is exact in f64.  Every lag's sum runs in one order
//                (m, then the sample; a butterfly over the wave's lanes; the waves in order) that does not depend on
//                the order asked for, and one f64 partial per (block, lag) leaves in an 8-byte store.
// lag_combine    One wave per lag: the lanes fetch 64 partials at a time, lane 0 adds them in block order.
// fir            One workgroup per tile of kFirTile outputs: the tile's input span and the kFirHist samples in front
//                of it are staged in LDS as above (non-finite samples kept).  A work item produces kFirPer consecutive
//                outputs per pass from a sliding register window: per chunk of kFirChunk taps three 16-byte LDS reads
//                feed 32 f32 fmas.  Every output adds its taps in the order j = 0, 1, ... from 0 with one fma each and
//                multiplies nothing but its n_taps taps, so a non-finite sample reaches exactly the outputs whose
//                support holds it.  The taps are uniform loads from the kernel argument.  Four consecutive outputs
//                leave as one 16-byte store when the output pointer allows, consecutive lanes side by side.  Tiles are
//                counted from output 0, i.e. from input sample `lead`: the bits of an output depend on n_taps, its
//                support and nothing else, which is what lets a caller filter a signal in pieces.
#include <cmath>

#include "am_internal.h"
#include "am_reduce.h"

namespace am {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const f32x4 gf32x4;
typedef __attribute__((address_space(1))) const u32x4 gu32x4;    // (four i16 stereo frames)

static_assert(kLagBlock % (4 * kLagThreads) == 0, "a block splits evenly into runs of four samples per work item");
static_assert(kLagHist % 4 == 0 && kFirHist % 4 == 0, "the staged history keeps the 16-byte alignment of the block");
static_assert(kLagChunk == 8 && kFirChunk == 8 && kFirPer == 4, "the register windows are written for 8 lags / taps and 4 samples");

__device__ __forceinline__ float wh_mix(unsigned u) {   // one i16 stereo frame (left in the low half) as the down-mix
    return norm_downmix(make_short2((short)(u & 0xffffu), (short)(u >> 16)));
}
template <int KIND>
__device__ __forceinline__ float wh_sample(const void* src, long long n) {
    return KIND ? wh_mix(((guint*)src)[n]) : ((gfloat*)src)[n];
}
// x[g .. g + 4) of the signal, 0 outside [0, n); g is a multiple of 4 relative to a 16-byte aligned address when vec
template <int KIND>
__device__ __forceinline__ float4 wh_load4(const void* src, long long g, long long n, int vec) {
    float4 v;
    if (vec && g >= 0 && g + 4 <= n) {
        if (KIND) {
            const u32x4 f = *(gu32x4*)((guint*)src + g);
            v = make_float4(wh_mix(f.x), wh_mix(f.y), wh_mix(f.z), wh_mix(f.w));
        } else {
            const f32x4 f = *(gf32x4*)((gfloat*)src + g);
            v = make_float4(f.x, f.y, f.z, f.w);
        }
    } else {
        v.x = g >= 0 && g < n ? wh_sample<KIND>(src, g) : 0.0f;
        v.y = g + 1 >= 0 && g + 1 < n ? wh_sample<KIND>(src, g + 1) : 0.0f;
        v.z = g + 2 >= 0 && g + 2 < n ? wh_sample<KIND>(src, g + 2) : 0.0f;
        v.w = g + 3 >= 0 && g + 3 < n ? wh_sample<KIND>(src, g + 3) : 0.0f;
    }
    return v;
}
__device__ __forceinline__ float wh_finite(float v) { return __builtin_isfinite(v) ? v : 0.0f; }

template <int KIND>
__global__ __launch_bounds__(kLagThreads) void lag_products_kernel(const void* src, long long n, int vec, int order, double* __restrict__ parts,
                                                                    long long nblk, long long blk0) {
    __shared__ float4 xs4[(kLagHist + kLagBlock) / 4];
    __shared__ double ws[kLagChunk][kLagThreads / 64];
    const int tid = threadIdx.x;
    const long long b = blk0 + (long long)blockIdx.x;
    const long long g0 = b * kLagBlock - kLagHist;   // the sample xs4[0] starts at
    for (int q = tid; q < (kLagHist + kLagBlock) / 4; q += kLagThreads) {
        float4 v = wh_load4<KIND>(src, g0 + 4ll * q, n, vec);
        v.x = wh_finite(v.x); v.y = wh_finite(v.y); v.z = wh_finite(v.z); v.w = wh_finite(v.w);
        xs4[q] = v;
    }
    __syncthreads();
    for (int k0 = 0; k0 <= order; k0 += kLagChunk) {
        double acc[kLagChunk];
#pragma unroll
        for (int l = 0; l < kLagChunk; ++l) acc[l] = 0.0;
#pragma unroll 2
        for (int m = 0; m < kLagBlock / (4 * kLagThreads); ++m) {
            const int q = kLagHist / 4 + tid + kLagThreads * m;   // xs4[q] = the work item's samples i .. i + 3
            const float4 c = xs4[q];
            const int qw = q - k0 / 4;
            const float4 w0 = xs4[qw - 2], w1 = xs4[qw - 1], w2 = xs4[qw];   // x[i - k0 - 8 .. i - k0 + 3]
            const double w[12] = {(double)w0.x, (double)w0.y, (double)w0.z, (double)w0.w, (double)w1.x, (double)w1.y,
                                  (double)w1.z, (double)w1.w, (double)w2.x, (double)w2.y, (double)w2.z, (double)w2.w};
            const double x[4] = {(double)c.x, (double)c.y, (double)c.z, (double)c.w};
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int l = 0; l < kLagChunk; ++l) acc[l] += x[s] * w[8 + s - l];   // x[i + s] x[i + s - (k0 + l)]
        }
        wave_sums<kLagThreads>(acc, ws);
        __syncthreads();
        if (tid < kLagChunk && k0 + tid <= order) parts[(long long)(k0 + tid) * nblk + b] = add_waves<kLagThreads>(ws[tid]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void lag_combine_kernel(const double* __restrict__ parts, long long nblk, double* __restrict__ r) {
    __shared__ double ps[2][64];
    const int lane = threadIdx.x;
    const double* p = parts + (long long)blockIdx.x * nblk;
    double acc = 0.0;
    double nxt = lane < nblk ? p[lane] : 0.0;
    int buf = 0;
    for (long long b0 = 0; b0 < nblk; b0 += 64) {
        ps[buf][lane] = nxt;
        nxt = b0 + 64 + lane < nblk ? p[b0 + 64 + lane] : 0.0;   // (the next 64 travel while lane 0 adds these)
        __syncthreads();
        if (lane == 0) {
            const int m = (int)min(64ll, nblk - b0);
            for (int i = 0; i < m; ++i) acc += ps[buf][i];
        }
        buf ^= 1;
    }
    if (lane == 0) r[blockIdx.x] = acc;
}

// the outputs k .. k + 3 of one work item gain the taps t0 .. t0 + 7 (FULL) or t0 .. t0 + rem - 1; q4: xs4 index of x[lead + k]
template <bool FULL>
__device__ __forceinline__ void fir_chunk(const float4* xs4, int q4, const FirJob& j, int t0, int rem, float (&acc)[kFirPer]) {
    const int qw = q4 - t0 / 4;
    const float4 w0 = xs4[qw - 2], w1 = xs4[qw - 1], w2 = xs4[qw];   // x[lead + k - t0 - 8 .. lead + k - t0 + 3]
    const float w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
    for (int i = 0; i < kFirChunk; ++i) {
        if (FULL || i < rem) {
            const float t = j.taps[t0 + i];
#pragma unroll
            for (int o = 0; o < kFirPer; ++o) acc[o] = __builtin_fmaf(t, w[8 + o - i], acc[o]);   // x[lead + k + o - (t0 + i)]
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(kFirThreads) void fir_kernel(const FirJob j, long long tile0) {
    __shared__ float4 xs4[(kFirHist + kFirTile) / 4];
    const int tid = threadIdx.x;
    const long long k0 = (tile0 + (long long)blockIdx.x) * kFirTile;
    const long long g0 = j.lead + k0 - kFirHist;   // the sample xs4[0] starts at
    for (int q = tid; q < (kFirHist + kFirTile) / 4; q += kFirThreads) xs4[q] = wh_load4<KIND>(j.src, g0 + 4ll * q, j.n_in, j.vec);
    __syncthreads();
    const int nt = j.n_taps;
#pragma unroll
    for (int p = 0; p < kFirPasses; ++p) {
        const int q4 = tid + kFirThreads * p;   // the outputs k0 + 4 q4 .. + 3
        const long long k = k0 + 4ll * q4;
        if (k >= j.n_out) continue;
        float acc[kFirPer];
#pragma unroll
        for (int o = 0; o < kFirPer; ++o) acc[o] = 0.0f;
        int t0 = 0;
        for (; t0 + kFirChunk <= nt; t0 += kFirChunk) fir_chunk<true>(xs4, kFirHist / 4 + q4, j, t0, kFirChunk, acc);
        if (t0 < nt) fir_chunk<false>(xs4, kFirHist / 4 + q4, j, t0, nt - t0, acc);
        float* d = j.dst + k;
        if (j.vec_out && k + kFirPer <= j.n_out) {
            // One 16-byte store per lane, consecutive lanes 16 consecutive bytes each.  The empty-looking asm reads the
            // data registers behind the store, so nothing overwrites them before two wait states have passed (the
            // store-data hazard of DESIGN.md section 3; buf_store4 in am_fft.hip, tools/check_store_hazard.py).
            f32x4 o;
            o.x = acc[0]; o.y = acc[1]; o.z = acc[2]; o.w = acc[3];
            *(__attribute__((address_space(1))) f32x4*)d = o;
            asm volatile("s_nop 1" : : "v"(o));
        } else {
#pragma unroll
            for (int o = 0; o < kFirPer; ++o)
                if (k + o < j.n_out) d[o] = acc[o];
        }
    }
}

constexpr long long kMaxGrid = 1ll << 30;

}  // namespace

hipError_t launch_lag_products(hipStream_t st, const void* src, long long n, int kind, int vec, int order, double* parts, double* r) {
    const long long nblk = lag_blocks(n);
    if (nblk <= 0) return hipSuccess;
    for (long long b0 = 0; b0 < nblk; b0 += kMaxGrid) {
        const dim3 g((unsigned)std::min(kMaxGrid, nblk - b0)), b(kLagThreads);
        if (kind) hipLaunchKernelGGL(lag_products_kernel<1>, g, b, 0, st, src, n, vec, order, parts, nblk, b0);
        else hipLaunchKernelGGL(lag_products_kernel<0>, g, b, 0, st, src, n, vec, order, parts, nblk, b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lag_combine_kernel, dim3((unsigned)(order + 1)), dim3(64), 0, st, parts, nblk, r);
    return hipGetLastError();
}

hipError_t launch_fir(hipStream_t st, const FirJob& j, int kind) {
    if (j.n_out <= 0) return hipSuccess;
    const long long ntiles = (j.n_out + kFirTile - 1) / kFirTile;
    for (long long t0 = 0; t0 < ntiles; t0 += kMaxGrid) {
        const dim3 g((unsigned)std::min(kMaxGrid, ntiles - t0)), b(kFirThreads);
        if (kind) hipLaunchKernelGGL(fir_kernel<1>, g, b, 0, st, j, t0);
        else hipLaunchKernelGGL(fir_kernel<0>, g, b, 0, st, j, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

int wh_check_order(uint32_t order) {
    if (order < 1 || order > AM_WHITEN_MAX_ORDER)
        return fail(AM_ERR_INVALID_ARG, "whiten: order must be in 1.." + std::to_string(AM_WHITEN_MAX_ORDER) + " (got " + std::to_string(order) + ")");
    return AM_OK;
}

int wh_check_taps(const float* taps, uint32_t n_taps) {
    if (n_taps < 1 || n_taps > AM_FIR_MAX_TAPS)
        return fail(AM_ERR_INVALID_ARG, "fir: n_taps must be in 1.." + std::to_string(AM_FIR_MAX_TAPS) + " (got " + std::to_string(n_taps) + ")");
    if (!taps) return fail(AM_ERR_INVALID_ARG, "null pointer");
    for (uint32_t i = 0; i < n_taps; ++i)
        if (!std::isfinite(taps[i])) return fail(AM_ERR_INVALID_ARG, "fir: tap " + std::to_string(i) + " is not finite");
    return AM_OK;
}

// the checks am_lag_products and its device form share, in their order; *done: nothing left to do (n = 0)
int lag_args(const void* in, size_t n, int sample_format, uint32_t order, double* r, bool* done) {
    int rc;
    *done = false;
    if ((rc = wh_check_order(order)) || (rc = check_format(sample_format, "whiten"))) return rc;
    if (!r) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (n == 0) {
        for (uint32_t k = 0; k <= order; ++k) r[k] = 0.0;
        *done = true;
        return AM_OK;
    }
    if (!in) return fail(AM_ERR_INVALID_ARG, "null pointer");
    return AM_OK;
}

// the checks am_fir and its device form share, in their order; *done: nothing left to do (n_in == lead)
int fir_args(const void* in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps, size_t lead, float* out, size_t cap,
             size_t* n_out, bool* done) {
    int rc;
    *done = false;
    if (!n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format, "whiten")) || (rc = wh_check_taps(taps, n_taps))) return rc;
    if (lead > n_in) return fail(AM_ERR_INVALID_ARG, "fir: lead (" + std::to_string(lead) + ") is larger than n_in (" + std::to_string(n_in) + ")");
    *n_out = n_in - lead;
    if (*n_out > cap) return fail(AM_ERR_CAPACITY, "fir: output buffer too small (" + std::to_string(*n_out) + " samples needed)");
    if (*n_out == 0) { *done = true; return AM_OK; }
    if (!in || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    return AM_OK;
}

// r[0 .. order] of the resident signal on c's stream, into host memory; waits for the device
int lag_products_on_device(Ctx* c, const void* d_in, size_t n, int sample_format, uint32_t order, double* r) {
    int rc;
    const long long nblk = lag_blocks((long long)n);
    if ((rc = c->lag_parts.ensure(sizeof(double) * (size_t)(order + 1) * (size_t)nblk)) || (rc = c->lag_r.ensure(sizeof(double) * (order + 1))))
        return rc;
    {
        ProfScope ps(c, KN_OTHER, c->stream);
        AM_HIP(launch_lag_products(c->stream, d_in, (long long)n, sample_format == AM_FMT_S16_STEREO ? 1 : 0, ((uintptr_t)d_in & 15) == 0 ? 1 : 0,
                                   (int)order, static_cast<double*>(c->lag_parts.p), static_cast<double*>(c->lag_r.p)));
    }
    AM_HIP(copy_on_stream(c, r, c->lag_r.p, sizeof(double) * (order + 1), hipMemcpyDeviceToHost));
    return AM_OK;
}

// y = fir(in) on c's stream, both resident on c's device.  Does not wait for the device.
int fir_on_device(Ctx* c, const void* d_in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps, size_t lead, float* d_out) {
    FirJob j{};
    j.src = d_in;
    j.n_in = (long long)n_in;
    j.lead = (long long)lead;
    j.dst = d_out;
    j.n_out = (long long)(n_in - lead);
    j.n_taps = (int)n_taps;
    j.vec = (((uintptr_t)d_in + 4 * (uintptr_t)lead) & 15) == 0 ? 1 : 0;   // (4 bytes per sample or frame)
    j.vec_out = ((uintptr_t)d_out & 15) == 0 ? 1 : 0;
    for (uint32_t i = 0; i < n_taps; ++i) j.taps[i] = taps[i];
    ProfScope ps(c, KN_OTHER, c->stream);
    AM_HIP(launch_fir(c->stream, j, sample_format == AM_FMT_S16_STEREO ? 1 : 0));
    return AM_OK;
}

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

static int lag_products_impl(int device, const void* in, size_t n, int sample_format, uint32_t order, double* r, bool device_io) {
    int rc;
    bool done;
    if ((rc = lag_args(in, n, sample_format, order, r, &done)) || done) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = resident_input(c, device_io, in, sample_bytes(n), &d_in))) return rc;
    return lag_products_on_device(c, d_in, n, sample_format, order, r);
}

int am_lag_products_device(int device, const void* d_in, size_t n, int sample_format, uint32_t order, double* r) {
    return lag_products_impl(device, d_in, n, sample_format, order, r, true);
}

int am_lag_products(int device, const void* in, size_t n, int sample_format, uint32_t order, double* r) {
    return lag_products_impl(device, in, n, sample_format, order, r, false);
}

int am_whiten_taps(const double* r, uint32_t order, double noise_db, float* taps) {
    int rc;
    if ((rc = wh_check_order(order))) return rc;
    if (!r || !taps) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (!(noise_db >= 0.0 && noise_db <= 200.0)) return fail(AM_ERR_INVALID_ARG, "whiten: noise_db must be in 0..200");
    for (uint32_t k = 0; k <= order; ++k)
        if (!std::isfinite(r[k])) return fail(AM_ERR_INVALID_ARG, "whiten: r[" + std::to_string(k) + "] is not finite");
    double a[AM_FIR_MAX_TAPS] = {1.0}, t[AM_FIR_MAX_TAPS];
    if (r[0] > 0.0) {
        double err = r[0] * (1.0 + std::pow(10.0, -noise_db / 10.0));   // the white-noise correction
        for (uint32_t m = 1; m <= order && err > 0.0; ++m) {
            double acc = r[m];
            for (uint32_t i = 1; i < m; ++i) acc += a[i] * r[m - i];
            const double k = -acc / err;
            if (!(std::fabs(k) < 1.0)) break;
            for (uint32_t i = 1; i < m; ++i) t[i] = a[i] + k * a[m - i];
            for (uint32_t i = 1; i < m; ++i) a[i] = t[i];
            a[m] = k;
            err *= 1.0 - k * k;
        }
    }
    for (uint32_t i = 0; i <= order; ++i) taps[i] = (float)a[i];
    return AM_OK;
}

static int fir_impl(int device, const void* in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps, size_t lead, float* out,
                    size_t cap, size_t* n_out, bool device_io) {
    int rc;
    bool done;
    if ((rc = fir_args(in, n_in, sample_format, taps, n_taps, lead, out, cap, n_out, &done)) || done) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const size_t out_bytes = sizeof(float) * *n_out;
    const void* d_in = nullptr;
    if ((rc = resident_input(c, device_io, in, sample_bytes(n_in), &d_in))) return rc;
    if (!device_io && (rc = c->io_out.ensure(out_bytes))) return rc;
    float* d_out = device_io ? out : static_cast<float*>(c->io_out.p);
    if ((rc = fir_on_device(c, d_in, n_in, sample_format, taps, n_taps, lead, d_out))) return rc;
    if (!device_io) return download(c, out, d_out, out_bytes);
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_fir_device(int device, const void* d_in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps, size_t lead,
                  float* d_out, size_t cap, size_t* n_out) {
    return fir_impl(device, d_in, n_in, sample_format, taps, n_taps, lead, d_out, cap, n_out, true);
}

int am_fir(int device, const void* in, size_t n_in, int sample_format, const float* taps, uint32_t n_taps, size_t lead, float* out,
           size_t cap, size_t* n_out) {
    return fir_impl(device, in, n_in, sample_format, taps, n_taps, lead, out, cap, n_out, false);
}

int am_needle_create_filtered(int device, const void* needle, size_t n, int sample_format, const float* taps, uint32_t n_taps,
                              am_needle** out) {
    int rc;
    if (!needle || !out || n == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    if ((rc = check_format(sample_format, "whiten")) || (rc = wh_check_taps(taps, n_taps))) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, needle, sample_bytes(n), &d_in))) return rc;
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, n * sizeof(float)));
    rc = fir_on_device(c, d_in, n, sample_format, taps, n_taps, 0, d);
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "fir: needle");
    }
    if (rc) { (void)hipFree(d); return rc; }
    return create_needle_common(c, d, n, out);
}

}  // extern "C"
