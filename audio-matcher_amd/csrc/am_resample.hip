// am_resample.hip -- sample-rate conversion (am_resample*, am_needle_create_resampled; include/audiomatch.h): the
// polyphase form of scipy.signal.resample_poly(x, L, M) with its default Kaiser window.  For output k let
// a = k M + H, nh = floor(a / L) and p = a mod L (the phase); then
//   y[k] = sum_{t < cnt(p)} taps[p][t] x[nh - t],   cnt(p) = floor((2H - p) / L) + 1,   taps[p][t] = h[p + t L - H]
// with x = 0 outside [0, n_in).  The table is built on the host in f64 (stored f32), once per (L, M) and device.
//
// One kernel.  Workgroup b produces the outputs [k0, k0 + W kRsJ), k0 = b W kRsJ.  It stages the input span they read
// in LDS with 16-byte coalesced loads (i16 stereo frames down-mixed on the way, so PCM is read once) and, when it fits,
// the table (rows padded to an odd stride).  Work item w < W takes the outputs k0 + w + jj W, jj < kRsJ: W is a multiple
// of L, so all of them share one phase, whose taps are read once per chunk of kRsTc into registers and used kRsJ times.
// Consecutive lanes write consecutive outputs.  Every output adds its taps in the order t = 0, 1, ... with one f32 fma
// each; taps past cnt(p) are skipped (their x position lies outside the support), so a non-finite sample reaches
// exactly the outputs whose support holds it.  Rows of up to kRsSeqTaps taps are one such chain.  Longer rows are added
// chunk by chunk: the kRsTc taps of a chunk in f32 from zero, in that order, and the chunk sums into an f64 sum that is
// rounded to f32 once, at the store.  A chain of n taps is off by up to n 2^-24 sum |h x|: with sum |h| < 3 that holds
// the header's 1e-5 max |x| up to kRsSeqTaps taps and breaks it from some 50 000 taps on (8192 -> 1 Hz has 163 841),
// while the chunked form stays below (kRsTc + 2) 2^-24 sum |h x| < 2e-6 max |x| for every row length.  The launch
// geometry and the form of the sum depend on (L, M) only: every entry point gives the same bits for the same input.
#include "am_internal.h"

namespace am {

namespace {

constexpr int kRsXsMax = 8192;    // floats of staged input per workgroup (32 KB)
constexpr int kRsTabMax = 8192;   // floats of staged table per workgroup (32 KB; with the input 64 KB of LDS at most)
constexpr int kRsWMax = 2048;     // work items per workgroup (unless L alone is larger)
constexpr int kRsSeqTaps = 48;    // rows up to this long (ts) are summed as one f32 chain, longer ones through f64
constexpr uint32_t kResampleMaxRate = 768000;   // rates in 1 .. this, Hz
constexpr long long kResampleMaxR = 8192;       // R = max(L, M) up to this (11025 <-> 384000 Hz: 5120)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const f32x4 gf32x4;
typedef __attribute__((address_space(1))) const u32x4 gu32x4;    // (four i16 stereo frames)

// one i16 stereo frame (left in the low half) as the down-mix (the halves taken apart arithmetically: a bit_cast of a
// vector element to short2 took the first element for every one)
__device__ __forceinline__ float rs_mix(unsigned u) {
    return norm_downmix(make_short2((short)(u & 0xffffu), (short)(u >> 16)));
}

template <int KIND>
__device__ __forceinline__ float rs_sample(const void* src, long long n) {
    return KIND ? rs_mix(((guint*)src)[n]) : ((gfloat*)src)[n];
}

template <int KIND, bool XLDS, bool TLDS, bool WIDE>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(ResampleJob j, long long blk0) {
    extern __shared__ float4 rs_lds4[];
    float* rs_lds = reinterpret_cast<float*>(rs_lds4);
    const int tid = threadIdx.x;
    const int L = j.L, M = j.M, ts = j.ts;
    const long long bo = (long long)j.W * kRsJ;
    const long long k0 = (blk0 + (long long)blockIdx.x) * bo;
    const unsigned long long a0 = (unsigned long long)k0 * (unsigned long long)M + (unsigned long long)j.H;
    const long long q0 = (long long)(a0 / (unsigned long long)L);
    const long long r0 = (long long)(a0 % (unsigned long long)L);
    float* xs = rs_lds;
    float* tab = rs_lds + (XLDS ? j.xs_cap : 0);
    long long xb = 0;
    if (XLDS) {
        // x[xb + i] for i < 4 nq: from the lowest sample any tap of the block may address (nh(k0) - (ts - 1)) to the
        // highest one (nh of the block's last output), 0 outside [0, n_in)
        const long long lo = q0 - (ts - 1);
        xb = lo - (((lo % 4) + 4) % 4);
        const long long hi = q0 + (r0 + (bo - 1) * M) / L;
        const int nq = (int)min((hi - xb) / 4 + 1, (long long)(j.xs_cap / 4));
        for (int q = tid; q < nq; q += kRsThreads) {
            const long long n = xb + 4ll * q;
            float4 v;
            if (j.vec && n >= 0 && n + 4 <= j.n_in) {
                if (KIND) {
                    const u32x4 f = ((gu32x4*)j.src)[n >> 2];
                    v = make_float4(rs_mix(f.x), rs_mix(f.y), rs_mix(f.z), rs_mix(f.w));
                } else {
                    const f32x4 f = ((gf32x4*)j.src)[n >> 2];
                    v = make_float4(f.x, f.y, f.z, f.w);
                }
            } else {
                v.x = n >= 0 && n < j.n_in ? rs_sample<KIND>(j.src, n) : 0.0f;
                v.y = n + 1 >= 0 && n + 1 < j.n_in ? rs_sample<KIND>(j.src, n + 1) : 0.0f;
                v.z = n + 2 >= 0 && n + 2 < j.n_in ? rs_sample<KIND>(j.src, n + 2) : 0.0f;
                v.w = n + 3 >= 0 && n + 3 < j.n_in ? rs_sample<KIND>(j.src, n + 3) : 0.0f;
            }
            *(float4*)(xs + 4 * q) = v;
        }
    }
    const int tsl = TLDS ? ts + 1 : ts;   // (an odd row stride in LDS: lanes of different phases fall on different banks)
    if (TLDS) {
        const int nt = L * ts;
        for (int i = tid; i < nt; i += kRsThreads) {
            const int p = i / ts, t = i - p * ts;
            tab[p * tsl + t] = ((gfloat*)j.taps)[i];
        }
    }
    if (XLDS || TLDS) __syncthreads();
    const long long wm = (long long)(j.W / L) * M;   // input advance between the outputs k and k + W of one work item
    for (int w = tid; w < j.W; w += kRsThreads) {
        const long long k = k0 + w;
        if (k >= j.n_out) break;
        const unsigned v = (unsigned)r0 + (unsigned)w * (unsigned)M;   // (< 2^27: r0 < L, w < W, every factor <= 8192)
        const long long nh = q0 + (long long)(v / (unsigned)L);
        const int p = (int)(v % (unsigned)L);
        const int cnt = (2 * j.H - p) / L + 1;
        const float* tp = (TLDS ? (const float*)tab : j.taps) + (long long)p * tsl;
        // acc: the f32 chain of a short row, of one chunk of a long row (WIDE); accw: the f64 sum of the chunk sums
        float acc[kRsJ];
        double accw[kRsJ];
#pragma unroll
        for (int jj = 0; jj < kRsJ; ++jj) { acc[jj] = 0.0f; accw[jj] = 0.0; }
        for (int t0 = 0; t0 < cnt; t0 += kRsTc) {
            float tv[kRsTc];
#pragma unroll
            for (int i = 0; i < kRsTc; ++i) tv[i] = TLDS ? tp[t0 + i] : ((gfloat*)tp)[t0 + i];
            const int lim = cnt - t0;   // taps i < lim lie on the support
            if (XLDS) {
                const int nb = (int)(nh - xb) - t0;
#pragma unroll
                for (int jj = 0; jj < kRsJ; ++jj) {
                    const int nj = nb + jj * (int)wm;
#pragma unroll
                    for (int i = 0; i < kRsTc; ++i) {
                        const float x = i < lim ? xs[nj - i] : 0.0f;
                        acc[jj] = __builtin_fmaf(tv[i], x, acc[jj]);
                    }
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < kRsJ; ++jj) {
                    const long long nj = nh + jj * wm - t0;
#pragma unroll
                    for (int i = 0; i < kRsTc; ++i) {
                        const long long n = nj - i;
                        const float x = i < lim && n >= 0 && n < j.n_in ? rs_sample<KIND>(j.src, n) : 0.0f;
                        acc[jj] = __builtin_fmaf(tv[i], x, acc[jj]);
                    }
                }
            }
            if (WIDE) {
#pragma unroll
                for (int jj = 0; jj < kRsJ; ++jj) { accw[jj] += (double)acc[jj]; acc[jj] = 0.0f; }
            }
        }
#pragma unroll
        for (int jj = 0; jj < kRsJ; ++jj) {
            const long long kk = k + (long long)jj * j.W;
            if (kk < j.n_out) j.dst[kk] = WIDE ? (float)accw[jj] : acc[jj];
        }
    }
}

template <int KIND, bool WIDE>
hipError_t launch_kind(hipStream_t st, const ResampleJob& j, unsigned nblk, long long blk0, size_t lds) {
    const dim3 g(nblk), b(kRsThreads);
    if (j.xs_cap && j.tab_lds) hipLaunchKernelGGL((resample_kernel<KIND, true, true, WIDE>), g, b, lds, st, j, blk0);
    else if (j.xs_cap) hipLaunchKernelGGL((resample_kernel<KIND, true, false, WIDE>), g, b, lds, st, j, blk0);
    else if (j.tab_lds) hipLaunchKernelGGL((resample_kernel<KIND, false, true, WIDE>), g, b, lds, st, j, blk0);
    else hipLaunchKernelGGL((resample_kernel<KIND, false, false, WIDE>), g, b, lds, st, j, blk0);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resample(hipStream_t st, const ResampleJob& j, int kind) {
    if (j.n_out <= 0) return hipSuccess;
    const long long bo = (long long)j.W * kRsJ;
    const long long nblk = (j.n_out + bo - 1) / bo;
    const size_t lds = sizeof(float) * ((size_t)j.xs_cap + (j.tab_lds ? (size_t)j.L * (size_t)(j.ts + 1) : 0));
    constexpr long long kMaxGrid = 1ll << 30;
    const bool wide = j.ts > kRsSeqTaps;   // (a function of (L, M) alone, like the geometry)
    for (long long b0 = 0; b0 < nblk; b0 += kMaxGrid) {
        const unsigned n = (unsigned)std::min(kMaxGrid, nblk - b0);
        const hipError_t e = wide ? (kind ? launch_kind<1, true>(st, j, n, b0, lds) : launch_kind<0, true>(st, j, n, b0, lds))
                                  : (kind ? launch_kind<1, false>(st, j, n, b0, lds) : launch_kind<0, false>(st, j, n, b0, lds));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

struct Ratio { long long L, M, H; };

int rs_ratio(uint32_t src_rate, uint32_t dst_rate, Ratio* r) {
    if (src_rate < 1 || src_rate > kResampleMaxRate || dst_rate < 1 || dst_rate > kResampleMaxRate)
        return fail(AM_ERR_INVALID_ARG, "resample: rates must be in 1.." + std::to_string(kResampleMaxRate) + " (src_rate " +
                                            std::to_string(src_rate) + ", dst_rate " + std::to_string(dst_rate) + ")");
    uint32_t a = src_rate, b = dst_rate;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    r->L = dst_rate / a;
    r->M = src_rate / a;
    const long long R = std::max(r->L, r->M);
    if (R > kResampleMaxR)
        return fail(AM_ERR_INVALID_ARG, "resample: " + std::to_string(src_rate) + " -> " + std::to_string(dst_rate) + " Hz needs R = max(L, M) = " +
                                            std::to_string(R) + " > " + std::to_string(kResampleMaxR));
    r->H = 10 * R;
    return AM_OK;
}

int rs_len(size_t n_in, const Ratio& r, size_t* n_out) {
    const unsigned __int128 up = (unsigned __int128)n_in * (unsigned __int128)r.L;
    const unsigned __int128 q = (up + (unsigned __int128)(r.M - 1)) / (unsigned __int128)r.M;
    if (q > (unsigned __int128)(1ull << 62)) return fail(AM_ERR_INVALID_ARG, "resample: n_in too large");
    *n_out = (size_t)q;
    return AM_OK;
}

double bessel_i0(double x) {   // sum_k ((x/2)^k / k!)^2: for the window's x <= 5 every term is positive and it converges fast
    double s = 1.0, t = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        t *= q / ((double)k * (double)k);
        s += t;
        if (t < 1e-17 * s) break;
    }
    return s;
}

// The launch geometry of (L, M): W = L G work items, G chosen for the best share of busy lanes (ties: the larger W)
// among the W whose input span fits the LDS budget.  None fits with at least half the lanes busy (a large M / L): the
// input is read through the cache.
void rs_geometry(const Ratio& r, int ts, ResampleJob* j) {
    const long long L = r.L, M = r.M;
    auto span = [&](long long W) { return ((L - 1 + (W * kRsJ - 1) * M) / L + ts + 8 + 3) / 4 * 4; };
    const long long gmax = std::max(1ll, kRsWMax / L);
    long long best = 0, best_x = 0;
    double best_eff = -1.0, best_eff_x = -1.0;
    for (long long g = 1; g <= gmax; ++g) {
        const long long W = L * g;
        const double eff = (double)W / (double)(kRsThreads * ((W + kRsThreads - 1) / kRsThreads));
        if (eff >= best_eff) { best_eff = eff; best = W; }
        if (span(W) <= kRsXsMax && eff >= best_eff_x) { best_eff_x = eff; best_x = W; }
    }
    if (best_eff_x < 0.5) best_x = 0;   // (staging would leave most lanes idle: 384 -> 8 kHz fits 18 work items)
    j->W = (int)(best_x ? best_x : best);
    j->xs_cap = best_x ? (int)span(best_x) : 0;
    j->tab_lds = L * (ts + 1) <= kRsTabMax ? 1 : 0;
}

// the polyphase table of (L, M) on c's device, built on first use
int rs_taps(Ctx* c, const Ratio& r, const float** d_taps, int* ts_out) {
    const long long L = r.L, M = r.M, H = r.H;
    const int T = (int)(2 * H / L + 1);
    const int ts = (T + kRsTc - 1) / kRsTc * kRsTc;
    *ts_out = ts;
    DevBuf& b = c->rs_taps[std::make_pair((int)L, (int)M)];
    if (b.p) { *d_taps = static_cast<const float*>(b.p); return AM_OK; }
    // h[j + H] = L w[j] / sum w,  w[j] = c sinc(c j) I0(5 sqrt(1 - (j/H)^2)) / I0(5),  c = 1/R  (scipy's firwin with
    // window ('kaiser', 5.0), as resample_poly designs it)
    const double cc = 1.0 / (double)std::max(L, M), i05 = bessel_i0(5.0);
    std::vector<double> h((size_t)(2 * H + 1));
    double sum = 0.0;
    for (long long i = 0; i <= 2 * H; ++i) {
        const double jj = (double)(i - H), u = cc * jj;
        const double sinc = u == 0.0 ? 1.0 : std::sin(M_PI * u) / (M_PI * u);
        const double rr = jj / (double)H;
        h[(size_t)i] = cc * sinc * bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - rr * rr))) / i05;
        sum += h[(size_t)i];
    }
    std::vector<float> tab((size_t)(L * ts), 0.0f);
    for (long long p = 0; p < L; ++p)
        for (long long t = 0; p + t * L <= 2 * H; ++t) tab[(size_t)(p * ts + t)] = (float)((double)L * h[(size_t)(p + t * L)] / sum);
    int rc = b.ensure(tab.size() * sizeof(float));
    if (rc) return rc;
    const hipError_t e = copy_on_stream(c, b.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { b.release(); return hip_fail(e, "resample: table upload"); }
    *d_taps = static_cast<const float*>(b.p);
    return AM_OK;
}

}  // namespace

// y = resample(in) on c's stream, both resident on c's device; n_out = rs_len(n_in).  Equal rates copy the input (f32) or
// down-mix it (i16), so that y holds exactly those bits.  Does not wait for the device.
int resample_on_device(Ctx* c, const void* d_in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate, float* d_out,
                       size_t n_out) {
    Ratio r;
    int rc = rs_ratio(src_rate, dst_rate, &r);
    if (rc) return rc;
    if (n_out == 0) return AM_OK;
    const int kind = sample_format == AM_FMT_S16_STEREO ? 1 : 0;
    if (r.L == 1 && r.M == 1) {
        if (kind) AM_HIP(launch_pcm_downmix(c->stream, static_cast<const int16_t*>(d_in), (long long)n_in, d_out));
        else AM_HIP(hipMemcpyAsync(d_out, d_in, n_in * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        return AM_OK;
    }
    ResampleJob j{};
    if ((rc = rs_taps(c, r, &j.taps, &j.ts))) return rc;
    j.src = d_in;
    j.n_in = (long long)n_in;
    j.dst = d_out;
    j.n_out = (long long)n_out;
    j.L = (int)r.L; j.M = (int)r.M; j.H = (int)r.H;
    rs_geometry(r, j.ts, &j);
    j.vec = ((uintptr_t)d_in & 15) == 0 ? 1 : 0;
    ProfScope ps(c, KN_OTHER, c->stream);
    AM_HIP(launch_resample(c->stream, j, kind));
    return AM_OK;
}

}  // namespace am

using namespace am;

extern "C" {

int am_resample_len(size_t n_in, uint32_t src_rate, uint32_t dst_rate, size_t* n_out) {
    if (!n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ratio r;
    int rc = rs_ratio(src_rate, dst_rate, &r);
    if (rc) return rc;
    return rs_len(n_in, r, n_out);
}

static int resample_impl(int device, const void* in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate, float* out,
                         size_t cap, size_t* n_out, bool device_io) {
    int rc;
    if (!n_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format, "resample")) || (rc = am_resample_len(n_in, src_rate, dst_rate, n_out))) return rc;
    if (*n_out > cap) return fail(AM_ERR_CAPACITY, "resample: output buffer too small (" + std::to_string(*n_out) + " samples needed)");
    if (n_in == 0) return AM_OK;
    if (!in || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const size_t no = *n_out;
    const void* d_in = nullptr;
    if ((rc = resident_input(c, device_io, in, sample_bytes(n_in), &d_in))) return rc;
    if (!device_io && (rc = c->io_out.ensure(sizeof(float) * no))) return rc;
    float* d_out = device_io ? out : static_cast<float*>(c->io_out.p);
    if ((rc = resample_on_device(c, d_in, n_in, sample_format, src_rate, dst_rate, d_out, no))) return rc;
    if (!device_io) return download(c, out, d_out, sizeof(float) * no);
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_resample_device(int device, const void* d_in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate,
                       float* d_out, size_t cap, size_t* n_out) {
    return resample_impl(device, d_in, n_in, sample_format, src_rate, dst_rate, d_out, cap, n_out, true);
}

int am_resample(int device, const void* in, size_t n_in, int sample_format, uint32_t src_rate, uint32_t dst_rate,
                float* out, size_t cap, size_t* n_out) {
    return resample_impl(device, in, n_in, sample_format, src_rate, dst_rate, out, cap, n_out, false);
}

int am_needle_create_resampled(int device, const void* needle, size_t n, int sample_format, uint32_t src_rate, uint32_t dst_rate,
                               am_needle** out) {
    int rc;
    if (!needle || !out || n == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    size_t no = 0;
    if ((rc = check_format(sample_format, "resample")) || (rc = am_resample_len(n, src_rate, dst_rate, &no))) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, needle, sample_bytes(n), &d_in))) return rc;
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, no * sizeof(float)));
    rc = resample_on_device(c, d_in, n, sample_format, src_rate, dst_rate, d, no);
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "resample: needle");
    }
    if (rc) { (void)hipFree(d); return rc; }
    return create_needle_common(c, d, no, out);
}

}  // extern "C"
