// am_estimate.hip -- needle estimation (am_hit_window, am_needle_estimate_*, include/audiomatch.h): the aligned
// occurrences of one needle stacked, and a robust per-sample estimate of them.  Row i, element n is
//   rows form     rows[i * length + n]
//   gather form   fl32(x_i[off_i + n] * scale_i), off_i = start_i - lead, read from the hit's resident haystack (the
//                 down-mix fused for i16 stereo); NaN where off_i + n lies outside the haystack
// and an element is present when it is finite.
//
// One kernel template, estimate_kernel<SRC, SLOTS>, on the context's stream; one thread per output sample (grid-stride
// over `length`), so adjacent lanes read adjacent elements of one row and every load is a coalesced 4-byte load.
//   SLOTS = 0            AM_EST_MEAN: a loop over the rows with an f64 accumulator, eight loads in flight.
//   SLOTS = 8 .. 64      AM_EST_MEDIAN / AM_EST_TRIMMED: the column's values as monotone integer keys in SLOTS
//                        registers (absent: 0xFFFFFFFF, above every present key), a bitonic sorting network on them and a
//                        selection by rank, all with compile-time indices: no register array is indexed by a runtime
//                        value, nothing goes to scratch.  A call runs the smallest network that holds its rows.
// The deviation takes a second pass over the column in row order (the sort has lost that order); a workgroup re-reads
// what it has just read.
// A result depends on the rows' values, their order and the parameters only: every reduction runs in the order the
// header fixes, whatever the source.
#include "am_internal.h"

namespace am {

namespace {

constexpr int kEstThreads = 256;
constexpr int kEstMaxBlocks = 8192;   // grid-stride beyond that
constexpr int kEstBatch = 8;          // loads in flight per thread in the row loops

__host__ __device__ __forceinline__ unsigned est_key(float v) {
    const unsigned b = __builtin_bit_cast(unsigned, v);
    return (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
}
__host__ __device__ __forceinline__ float est_unkey(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? k ^ 0x80000000u : ~k);
}

// element n of row i (i < j.n); not finite: absent
template <int SRC>
__device__ __forceinline__ float est_value(const EstJob& j, int i, long long n) {
    if (SRC == 0) return ((gfloat*)j.src)[(long long)i * j.length + n];
    // The load is unconditional (outside the haystack it reads element 0, which the host guarantees to exist) and the
    // bounds decide by a select behind it: a load under a branch of its own is waited for before the next one is issued.
    const EstHit h = static_cast<const EstHit*>(j.src)[i];
    const long long e = h.off + n;
    const bool inside = e >= 0 && e < h.len;
    const float x = hit_sample<SRC == 2 ? 1 : 0>(h.src, inside ? e : 0);
    return inside ? __fmul_rn(x, h.scale) : __builtin_nanf("");
}

// ascending bitonic network on k[0 .. 2^LOG): every index is a compile-time constant once the loops are unrolled
template <int LOG>
__device__ __forceinline__ void est_sort(unsigned (&k)[1 << LOG]) {
#pragma unroll
    for (int ls = 1; ls <= LOG; ++ls) {
#pragma unroll
        for (int js = ls - 1; js >= 0; --js) {
#pragma unroll
            for (int i = 0; i < (1 << LOG); ++i) {
                const int l = i ^ (1 << js);
                if (l > i) {
                    const unsigned lo = min(k[i], k[l]), hi = max(k[i], k[l]);
                    const bool up = (i & (1 << ls)) == 0;
                    k[i] = up ? lo : hi;
                    k[l] = up ? hi : lo;
                }
            }
        }
    }
}

constexpr int est_log2(int v) { return v <= 1 ? 0 : 1 + est_log2(v >> 1); }

template <int SRC, int SLOTS>
__global__ __launch_bounds__(kEstThreads) void estimate_kernel(const EstJob j) {
    const long long step = (long long)gridDim.x * kEstThreads;
    for (long long n = (long long)blockIdx.x * kEstThreads + threadIdx.x; n < j.length; n += step) {
        double m = 0.0;
        unsigned c = 0;
        if constexpr (SLOTS == 0) {
            double s = 0.0;
            for (int i0 = 0; i0 < j.n; i0 += kEstBatch) {
                float v[kEstBatch];
#pragma unroll
                for (int u = 0; u < kEstBatch; ++u) v[u] = est_value<SRC>(j, min(i0 + u, j.n - 1), n);
#pragma unroll
                for (int u = 0; u < kEstBatch; ++u)
                    if (i0 + u < j.n && __builtin_isfinite(v[u])) {
                        s += (double)v[u];
                        ++c;
                    }
            }
            if (c) m = s / (double)c;
        } else {
            // every load of the column in flight at once (slots behind the last row read it again and stay absent)
            float v[SLOTS];
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) v[i] = est_value<SRC>(j, min(i, j.n - 1), n);
            unsigned k[SLOTS];
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                const bool present = i < j.n && __builtin_isfinite(v[i]);
                k[i] = present ? est_key(v[i]) : 0xFFFFFFFFu;
                c += present ? 1u : 0u;
            }
            est_sort<est_log2(SLOTS)>(k);
            if (c) {
                if (j.method == AM_EST_MEDIAN) {
                    const unsigned r0 = (c - 1) >> 1, r1 = c >> 1;   // the same slot for an odd count: (a + a) / 2 = a
                    unsigned a = 0, b = 0;
#pragma unroll
                    for (int i = 0; i < SLOTS; ++i) {
                        a = (unsigned)i == r0 ? k[i] : a;
                        b = (unsigned)i == r1 ? k[i] : b;
                    }
                    m = ((double)est_unkey(a) + (double)est_unkey(b)) * 0.5;
                } else {
                    const unsigned d = min(c * j.trim_permille / 1000u, (c - 1) >> 1), end = c - d;
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < SLOTS; ++i) {
                        const double x = (double)est_unkey(k[i]);
                        s = ((unsigned)i >= d && (unsigned)i < end) ? s + x : s;
                    }
                    m = s / (double)(c - 2 * d);
                }
            }
        }
        j.est[n] = (float)m;
        if (j.count) j.count[n] = c;
        if (j.dev) {
            double acc = 0.0;
            if (c)
                for (int i0 = 0; i0 < j.n; i0 += kEstBatch) {
                    float v[kEstBatch];
#pragma unroll
                    for (int u = 0; u < kEstBatch; ++u) v[u] = est_value<SRC>(j, min(i0 + u, j.n - 1), n);
#pragma unroll
                    for (int u = 0; u < kEstBatch; ++u)
                        if (i0 + u < j.n && __builtin_isfinite(v[u])) {
                            const double d = (double)v[u] - m;
                            acc += d * d;
                        }
                }
            j.dev[n] = c ? (float)sqrt(acc / (double)c) : 0.0f;
        }
    }
}

template <int SRC>
hipError_t launch_estimate_src(hipStream_t st, const EstJob& j, int slots) {
    const long long want = (j.length + kEstThreads - 1) / kEstThreads;
    const dim3 grid((unsigned)std::min<long long>(want, kEstMaxBlocks)), block(kEstThreads);
    switch (slots) {
        case 0: hipLaunchKernelGGL((estimate_kernel<SRC, 0>), grid, block, 0, st, j); break;
        case 8: hipLaunchKernelGGL((estimate_kernel<SRC, 8>), grid, block, 0, st, j); break;
        case 16: hipLaunchKernelGGL((estimate_kernel<SRC, 16>), grid, block, 0, st, j); break;
        case 32: hipLaunchKernelGGL((estimate_kernel<SRC, 32>), grid, block, 0, st, j); break;
        case 64: hipLaunchKernelGGL((estimate_kernel<SRC, 64>), grid, block, 0, st, j); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

int estimate_slots(int method, int n) {
    if (method == AM_EST_MEAN) return 0;
    for (int s = 8; s <= AM_EST_MAX_HITS; s <<= 1)
        if (n <= s) return s;
    return -1;
}

hipError_t launch_estimate(hipStream_t st, const EstJob& j, int src) {
    const int slots = estimate_slots(j.method, j.n);
    if (j.length <= 0 || j.n <= 0 || slots < 0) return hipErrorInvalidValue;
    switch (src) {
        case 0: return launch_estimate_src<0>(st, j, slots);
        case 1: return launch_estimate_src<1>(st, j, slots);
        case 2: return launch_estimate_src<2>(st, j, slots);
        default: return hipErrorInvalidValue;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

constexpr size_t kEstMeanMaxHits = 65535;
constexpr uint64_t kEstMaxIndex = (uint64_t)1 << 62;   // lead, length and a hit's start stay below it (no overflow in start - lead + n)

bool est_scale_ok(float scale) { return std::isfinite(scale) && scale != 0.0f; }

// the parameter block and the hit count of the two compute forms
int est_check_params(const am_estimate_params* ep, size_t n) {
    if (ep->method != AM_EST_MEAN && ep->method != AM_EST_MEDIAN && ep->method != AM_EST_TRIMMED)
        return fail(AM_ERR_INVALID_ARG, "estimate: unknown method " + std::to_string(ep->method));
    if (ep->trim_permille > 500)
        return fail(AM_ERR_INVALID_ARG, "estimate: trim_permille must be in 0..500 (got " + std::to_string(ep->trim_permille) + ")");
    if (n == 0) return fail(AM_ERR_INVALID_ARG, "estimate: n must be at least 1");
    if (ep->length == 0) return fail(AM_ERR_INVALID_ARG, "estimate: length must be at least 1");
    if (ep->length >= kEstMaxIndex || ep->lead >= kEstMaxIndex) return fail(AM_ERR_INVALID_ARG, "estimate: lead or length out of range");
    if (ep->method == AM_EST_MEAN) {
        if (n > kEstMeanMaxHits)
            return fail(AM_ERR_INVALID_ARG, "estimate: mean takes at most " + std::to_string(kEstMeanMaxHits) + " hits (got " + std::to_string(n) + ")");
    } else if (n > AM_EST_MAX_HITS) {
        return fail(AM_ERR_INVALID_ARG, "estimate: median and trimmed take at most " + std::to_string(AM_EST_MAX_HITS) +
                                            " hits (AM_EST_MAX_HITS; got " + std::to_string(n) + ")");
    }
    return AM_OK;
}

// the outputs a call asked for, one array behind the other
size_t est_out_bytes(const am_estimate_params* ep, const float* dev, const uint32_t* count) {
    return 4 * (size_t)ep->length * (1 + (dev ? 1 : 0) + (count ? 1 : 0));
}

// The launch and the results' trip back, after hit_io_reserve(c, tab_bytes, est_out_bytes): `src` resident (the rows, or
// the hit table already on its way to c->hit_tab, tab_bytes of it), the outputs in c->hit_out, back through the pinned side
int run_estimate(Ctx* c, const void* src, int src_kind, size_t tab_bytes, size_t n, const am_estimate_params* ep, float* est, float* dev,
                 uint32_t* count) {
    const size_t len = (size_t)ep->length, out_bytes = est_out_bytes(ep, dev, count);
    int rc;
    EstJob j{};
    j.src = src_kind ? c->hit_tab.p : src;
    j.length = (long long)len;
    j.n = (int)n;
    j.method = (int)ep->method;
    j.trim_permille = ep->trim_permille;
    float* o = static_cast<float*>(c->hit_out.p);
    j.est = o;
    j.dev = dev ? (o += len) : nullptr;
    j.count = count ? reinterpret_cast<unsigned*>(o += len) : nullptr;
    {
        ProfScope ps(c, KN_OTHER, c->stream);
        AM_HIP(launch_estimate(c->stream, j, src_kind));
    }
    const void* res = nullptr;
    if ((rc = hit_results_get(c, tab_bytes, out_bytes, &res))) return rc;
    const char* r = static_cast<const char*>(res);
    std::memcpy(est, r, 4 * len);
    if (dev) std::memcpy(dev, r += 4 * len, 4 * len);
    if (count) std::memcpy(count, r += 4 * len, 4 * len);
    return AM_OK;
}

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_window(const void* haystack, size_t len, int sample_format, uint64_t start, float scale, uint64_t lead, uint64_t length,
                  float* row) {
    int rc;
    if ((rc = check_format(sample_format, "estimate"))) return rc;
    if (!row || (!haystack && len > 0)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (length == 0) return fail(AM_ERR_INVALID_ARG, "estimate: length must be at least 1");
    if (!est_scale_ok(scale)) return fail(AM_ERR_INVALID_ARG, "estimate: scale must be finite and not zero");
    const float* f = static_cast<const float*>(haystack);
    const int16_t* s = static_cast<const int16_t*>(haystack);
    const float nan = std::nanf("");
    for (uint64_t n = 0; n < length; ++n) {
        float v = nan;
        const uint64_t pos = start + n;   // element pos - lead; absent in front of the haystack, behind it and on wrap-around
        if (pos >= start && pos >= lead && pos - lead < len) {
            const uint64_t e = pos - lead;
            const float x = sample_format == AM_FMT_S16_STEREO ? (float)((int)s[2 * e] + (int)s[2 * e + 1]) * (0.5f * (1.0f / 65535.0f)) : f[e];
            if (std::isfinite(x)) v = x * scale;
        }
        row[n] = v;
    }
    return AM_OK;
}

int am_needle_estimate_rows(int device, const float* rows, size_t n, const am_estimate_params* ep, float* est, float* dev,
                            uint32_t* count) {
    int rc;
    if (!rows || !ep || !est) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = est_check_params(ep, n))) return rc;
    if (ep->length > (SIZE_MAX / 16) / n) return fail(AM_ERR_INVALID_ARG, "estimate: n * length out of range");
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const size_t bytes = sizeof(float) * n * (size_t)ep->length;
    const void* d_rows = nullptr;
    if ((rc = upload_input(c, rows, bytes, &d_rows)) || (rc = hit_io_reserve(c, 0, est_out_bytes(ep, dev, count)))) return rc;
    return run_estimate(c, d_rows, 0, 0, n, ep, est, dev, count);
}

int am_needle_estimate_device(int device, const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                              const am_est_hit* hits, size_t n, const am_estimate_params* ep, float* est, float* dev, uint32_t* count) {
    int rc;
    if (!d_haystacks || !lens || !hits || !ep || !est) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_format(sample_format, "estimate")) || (rc = est_check_params(ep, n))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const std::string hit = "hit " + std::to_string(i) + ": ";
        if (hits[i].haystack >= n_hay)
            return fail(AM_ERR_INVALID_ARG, hit + "haystack " + std::to_string(hits[i].haystack) + " out of range (n_hay = " + std::to_string(n_hay) + ")");
        if (!d_haystacks[hits[i].haystack]) return fail(AM_ERR_INVALID_ARG, hit + "null haystack");
        if (!est_scale_ok(hits[i].scale)) return fail(AM_ERR_INVALID_ARG, hit + "scale must be finite and not zero");
    }
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const size_t tab_bytes = sizeof(EstHit) * n;
    if ((rc = hit_io_reserve(c, tab_bytes, est_out_bytes(ep, dev, count)))) return rc;
    std::vector<char> checked(n_hay, 0);
    std::vector<EstHit> tab(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t k = hits[i].haystack;
        if (!checked[k]) {   // (once per haystack, at the first hit that reads it)
            if ((rc = hit_check_device(d_haystacks[k], c->device, HitWhere{-1, k, 0, i})))
                return fail(rc, "hit " + std::to_string(i) + ": " + t_err);
            checked[k] = 1;
        }
        EstHit& h = tab[i];
        h.src = lens[k] ? d_haystacks[k] : c->hit_tab.p;   // (an empty haystack: every element absent, element 0 still readable)
        h.len = (long long)std::min<uint64_t>(lens[k], kEstMaxIndex);
        h.off = (long long)std::min<uint64_t>(hits[i].start, kEstMaxIndex) - (long long)ep->lead;
        h.scale = hits[i].scale;
        h.pad = 0;
    }
    if ((rc = hit_table_put(c, tab.data(), 0, tab_bytes))) return rc;
    return run_estimate(c, nullptr, sample_format == AM_FMT_S16_STEREO ? 2 : 1, tab_bytes, n, ep, est, dev, count);
}

}  // extern "C"
