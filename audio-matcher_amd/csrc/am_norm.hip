// am_norm.hip -- window-energy normalised scores (option "score_norm", include/audiomatch.h):
//   ncc(t) = corr(t) / sqrt(sum(needle^2) * sum_{i=t-lead}^{t-lead+S-1} x_i^2),  x = 0 outside [0, len)
// K3 writes corr(t) / sqrt(sum(needle^2)) (norm_factor); the kernels here divide by the window's own energy.
//
// Two kernels on the stream that will read the scores:
//   block_energy   one f64 sum(x^2) per block of kNormBlock samples (non-finite samples count as 0)
//   norm_scores    one workgroup per tile of kNormTile consecutive scores.  A window's energy is assembled only from
//                  non-negative pieces: the whole blocks every window of the tile covers, plus a suffix sum over the
//                  tile's head span and a prefix sum over its tail span (f64 scans in LDS).  No difference of a global
//                  prefix array: over an hour at full scale P(t+S) - P(t) cancels to about 1e-8, which is above the
//                  floor of a quiet needle, and a window of digital silence must come out as exactly 0.
//                  Needles shorter than kNormTile + 2 kNormBlock take a direct path: one local prefix scan over the
//                  tile's kNormTile + S - 1 samples.
//   masked_norm_scores   the same for a masked needle (am_needle_create_masked): the energy of the kept samples only,
//                  each kept span assembled as a needle of its own length (span_energy, shared with norm_scores), the
//                  spans added in span order.  A handle without gaps never gets here.
// Every score depends on its index, the samples and the needle only (tiles start at multiples of kNormTile of the
// score array, the reductions run in a fixed order): a haystack's bits do not depend on the batch it travels in.
#include "am_internal.h"
#include "am_reduce.h"

namespace am {

namespace {

constexpr int kNormThreads = 256;
constexpr int kNormPer = kNormTile / kNormThreads;               // scores per thread
constexpr int kNormSpan = kNormTile + (kNormTile + 2 * kNormBlock);   // LDS span of the direct path (longest)
static_assert(kNormTile % kNormThreads == 0, "tile must split evenly over the workgroup");
static_assert(kNormBlock % kNormThreads == 0, "block must split evenly over the workgroup");

// x_i^2 in f64 (exact for an f32 x); 0 outside [0, len) and for a non-finite sample
__device__ __forceinline__ double norm_sq(const void* __restrict__ src, long long i, long long len, int kind) {
    if (i < 0 || i >= len) return 0.0;
    const float v = kind ? norm_downmix(static_cast<const short2*>(src)[i]) : static_cast<const float*>(src)[i];
    if (!__builtin_isfinite(v)) return 0.0;
    const double d = (double)v;
    return d * d;
}
__device__ __forceinline__ long long floor_div(long long x, long long b) { return x >= 0 ? x / b : -((-x + b - 1) / b); }

// Sum of one value per thread, in the order of block_sum (am_reduce.h; every thread gets the result), and ws free
// again.  `ws`: kNormThreads / 64 doubles.
__device__ double norm_block_sum(double v, double* ws) {
    const double t = block_sum<kNormThreads>(v, ws);
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(kNormThreads) void block_energy_kernel(const void* __restrict__ src, long long len, int kind, double* __restrict__ blk) {
    __shared__ double ws[kNormThreads / 64];
    const long long base = (long long)blockIdx.x * kNormBlock;
    double s = 0.0;
    for (int r = 0; r < kNormBlock / kNormThreads; ++r) s += norm_sq(src, base + threadIdx.x + r * kNormThreads, len, kind);
    s = norm_block_sum(s, ws);
    if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// The energies e[r] of the kNormPer windows a thread owns, [u0 + k, u0 + k + S) for k = tid + r kNormThreads: whole
// blocks plus head suffix and tail prefix (S >= kNormTile + 2 kNormBlock), or one local scan (shorter).  Every thread of
// the workgroup calls it with the same u0 and S; a barrier must follow before buf is written again.
__device__ __forceinline__ void span_energy(const NormJob& j, long long u0, long long S, double* buf, double* ws, double (&e)[kNormPer]) {
    const int tid = threadIdx.x;
    const long long B = kNormBlock;
    if (S >= kNormTile + 2 * kNormBlock) {
        // shared whole blocks [A, Z): A at or behind every window start of the tile, Z at or before every window end
        const long long A = floor_div(u0 + kNormTile - 1 + B - 1, B) * B;
        const long long Z = floor_div(u0 + S, B) * B;
        // head pieces [u, A): suffix sums over [u0, A)
        const int nh = (int)(A - u0);
        for (int q = tid; q < nh; q += kNormThreads) buf[q] = norm_sq(j.src, u0 + q, j.src_len, j.src_kind);
        __syncthreads();
        block_scan<kNormThreads, true>(buf, nh, ws);
        for (int r = 0; r < kNormPer; ++r) {
            const int k = tid + r * kNormThreads;
            e[r] = k < nh ? buf[k] : 0.0;
        }
        __syncthreads();
        // the whole blocks
        const long long jlo = max(A / B, 0ll), jhi = min(Z / B, j.nblk);
        double m = 0.0;
        for (long long q = jlo + tid; q < jhi; q += kNormThreads) m += j.blk[q];
        m = norm_block_sum(m, ws);
        // tail pieces [Z, u + S): prefix sums over [Z, u0 + kNormTile - 1 + S)
        const int nt = (int)(u0 + kNormTile - 1 + S - Z);
        for (int q = tid; q < nt; q += kNormThreads) buf[q] = norm_sq(j.src, Z + q, j.src_len, j.src_kind);
        __syncthreads();
        block_scan<kNormThreads, false>(buf, nt, ws);
        for (int r = 0; r < kNormPer; ++r) {
            const long long k = u0 + tid + r * kNormThreads + S - Z;   // tail piece length
            e[r] = (e[r] + m) + (k > 0 ? buf[k - 1] : 0.0);
        }
    } else {
        // direct path: one prefix scan over the tile's samples [u0, u0 + kNormTile - 1 + S)
        const int n = (int)(kNormTile - 1 + S);
        for (int q = tid; q < n; q += kNormThreads) buf[q] = norm_sq(j.src, u0 + q, j.src_len, j.src_kind);
        __syncthreads();
        block_scan<kNormThreads, false>(buf, n, ws);
        for (int r = 0; r < kNormPer; ++r) {
            const int k = tid + r * kNormThreads;
            e[r] = buf[k + S - 1] - (k > 0 ? buf[k - 1] : 0.0);   // (local sums: a window of zeros gives exactly 0)
        }
    }
}

// the tile's scores [t0, t0 + kNormTile) within [a, b) divided by the root of their energies, or 0 below the floor
__device__ __forceinline__ void norm_write(const NormJob& j, long long t0, const double (&e)[kNormPer]) {
    for (int r = 0; r < kNormPer; ++r) {
        const long long t = t0 + threadIdx.x + r * kNormThreads;
        if (t < j.a || t >= j.b) continue;
        const float raw = j.scores[t];
        if (!__builtin_isfinite(raw)) continue;   // (a non-finite score stays what it is: the callers' classification reads it)
        const double E = e[r];
        j.scores[t] = (E >= j.thr && E > 0.0) ? (float)((double)raw / sqrt(E)) : 0.0f;
    }
}

__global__ __launch_bounds__(kNormThreads) void norm_scores_kernel(NormJob j, long long tile0) {
    __shared__ double buf[kNormSpan];
    __shared__ double ws[kNormThreads / 64];
    const long long t0 = (tile0 + blockIdx.x) * kNormTile;
    double e[kNormPer];
    span_energy(j, t0 - j.lead, j.s, buf, ws, e);   // (t0 - lead: first sample of the tile's first window)
    norm_write(j, t0, e);
}

// Masked needles: the same tile, the energy of each kept span [a_q, b_q) taken as above for a needle of length b_q - a_q
// whose windows start a_q samples further on, and the spans' energies added in f64 in span order.  Never the whole
// window minus the gaps: what lies under a gap is not read for the span beside it, so kept spans in digital silence
// give exactly 0 however loud the gaps are.  One buf serves the spans in turn (no more LDS than norm_scores_kernel);
// the block energies are the signal's, shared by all spans.
__global__ __launch_bounds__(kNormThreads) void masked_norm_scores_kernel(NormJob j, long long tile0) {
    __shared__ double buf[kNormSpan];
    __shared__ double ws[kNormThreads / 64];
    const long long t0 = (tile0 + blockIdx.x) * kNormTile;
    const long long u0 = t0 - j.lead;
    double E[kNormPer];
    for (int r = 0; r < kNormPer; ++r) E[r] = 0.0;
    for (int q = 0; q < j.n_kept; ++q) {
        const long long a = j.kept[2 * q], b = j.kept[2 * q + 1];
        double e[kNormPer];
        span_energy(j, u0 + a, b - a, buf, ws, e);
        for (int r = 0; r < kNormPer; ++r) E[r] += e[r];
        __syncthreads();
    }
    norm_write(j, t0, E);
}

}  // namespace

hipError_t launch_block_energy(hipStream_t st, const void* src, long long src_len, int src_kind, double* blk) {
    const long long nblk = norm_blocks(src_len);
    if (nblk <= 0) return hipSuccess;
    hipLaunchKernelGGL(block_energy_kernel, dim3((unsigned)nblk), dim3(kNormThreads), 0, st, src, src_len, src_kind, blk);
    return hipGetLastError();
}

hipError_t launch_norm_scores(hipStream_t st, const NormJob& j) {
    if (j.b <= j.a) return hipSuccess;
    const long long tile0 = j.a / kNormTile, tile1 = (j.b + kNormTile - 1) / kNormTile;
    hipLaunchKernelGGL(norm_scores_kernel, dim3((unsigned)(tile1 - tile0)), dim3(kNormThreads), 0, st, j, tile0);
    return hipGetLastError();
}

hipError_t launch_masked_norm_scores(hipStream_t st, const NormJob& j) {
    if (j.b <= j.a) return hipSuccess;
    const long long tile0 = j.a / kNormTile, tile1 = (j.b + kNormTile - 1) / kNormTile;
    hipLaunchKernelGGL(masked_norm_scores_kernel, dim3((unsigned)(tile1 - tile0)), dim3(kNormThreads), 0, st, j, tile0);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

NormSpec norm_spec(const am_needle* h, const Opts& o) {
    NormSpec ns{};
    ns.on = o.score_norm != 0;
    ns.energy = h->energy;
    ns.thr = h->energy * std::pow(10.0, -(double)o.score_norm_floor_db / 10.0);
    ns.kept = h->gaps.empty() ? nullptr : h->d_kept;
    ns.n_kept = h->gaps.empty() ? 0 : h->n_kept;
    return ns;
}

int norm_check(const NormSpec& ns, int scale) {
    if (ns.on && scale != AM_SCALE_LIB)
        return fail(AM_ERR_INVALID_ARG, "score_norm = 1 requires scale = AM_SCALE_LIB (the needle energy is divided out of the scores)");
    return AM_OK;
}

float norm_factor(const NormSpec& ns) {
    return ns.energy > 0.0 ? (float)(1.0 / std::sqrt(ns.energy)) : 0.0f;
}

int norm_reserve(Ctx* c, long long max_src_len) {
    return c->norm_blk.ensure(sizeof(double) * (size_t)std::max<long long>(norm_blocks(max_src_len), 1));
}

int normalise_scores(Ctx* c, hipStream_t st, const NormSpec& ns, const void* src, long long src_len, int src_kind, long long lead,
                     long long s, float* scores, long long a, long long b) {
    if (b <= a) return AM_OK;
    int rc;
    if ((rc = norm_reserve(c, src_len))) return rc;
    NormJob j{};
    j.src = src; j.src_len = src_len; j.src_kind = src_kind; j.lead = lead; j.s = s;
    j.blk = static_cast<const double*>(c->norm_blk.p); j.nblk = norm_blocks(src_len);
    j.thr = ns.thr; j.scores = scores; j.a = a; j.b = b;
    j.kept = ns.kept; j.n_kept = ns.n_kept;
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(launch_block_energy(st, src, src_len, src_kind, static_cast<double*>(c->norm_blk.p))); }
    { ProfScope ps(c, KN_OTHER, st); AM_HIP(j.n_kept > 0 ? launch_masked_norm_scores(st, j) : launch_norm_scores(st, j)); }
    return AM_OK;
}

}  // namespace am
