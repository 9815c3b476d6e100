// am_stereo.hip -- per-hit stereo image (am_hit_stereo*, am_hit_stereo_summary) and the stereo mix other than the
// down-mix (am_pcm_s16_stereo_mix*); include/audiomatch.h.  The first per-hit family that reads the i16 frames themselves
// instead of hit_sample<1>'s down-mix.  For a hit at t, the needle n[0 .. S), L[u] and R[u] the i16 values of frame u (0
// outside the haystack) and the lags l = -R .. R:
//   C_L(l) = sum_i L[t + l + i] n[i],   C_R(l) likewise                      (f64; an i16 times an f32 value is exact there)
//   S_LL = sum_i L[t + i]^2,   S_RR = sum_i R[t + i]^2,   S_LR = sum_i L[t + i] R[t + i]      (64-bit integers, exact)
// and from those, with k = (double)(1.0f / 65535.0f): c_ch = k C_ch, E = k^2 S, the record of the header.
//
// Three kernels on the context's stream:
//   stereo_slices   one workgroup of 256 per slice of kHitSlice needle samples of one hit (blockIdx.x = slice, blockIdx.y
//                   = hit).  It reads each frame of [t + i0 - RT, t + i0 + cnt + RT) once, as one 32-bit load, and stages
//                   both channels in LDS as f32 (an i16 value is exact there) at index pad16(q): work item w takes the
//                   16 consecutive needle samples 16 w .. 16 w + 15 (in registers) and reads the 16 + 2 RT staged samples
//                   its lags reach into registers once per channel (lag_dot).  One channel at a time: its 2 RT + 1 sums
//                   in f64 accumulators, added over each wave (wave_sums) before the other channel's begin, so that one
//                   channel's registers serve both; add_waves finishes them.  RT is the smallest of kSegRadii that holds
//                   R.  The three integer sums come from the same staged samples and take the same helpers.  One partial
//                   record per slice, one 64-bit store per lane.
//   stereo_combine  one wave per hit: adds the partials (sum_slices), picks each channel's lag on |c| (pick_lag,
//                   refine_lag) and writes the am_stereo_hit.
//   pcm_mix         grid-stride: four frames per 16-byte load and four floats per 16-byte store where the pointers allow,
//                   ragged ends scalar.
// The kernels read frame t + u for u in [-R, S + R) inside the haystack only (StereoDesc::ulo, uhi), whatever RT is: that
// is what the host form stages, and lags beyond R never reach a result.  A hit's record depends on the needle, the frames
// it reads, R and the floor only: the three forms run in the frame of am_hits.hip (am_internal.h: hit_call, hit_call_batch,
// hit_round_trip) and agree bit for bit.
#include <cmath>

#include "am_hit_device.h"
#include "am_internal.h"

namespace am {

namespace {

constexpr int kStThreads = 256;
constexpr int kStPer = kHitSlice / kStThreads;   // consecutive needle samples per work item
constexpr long long kMixMaxBlocks = 1 << 20;     // workgroups of pcm_mix
static_assert(kStPer == 16, "pad16: the LDS layout pads one word per 16 samples");
static_assert(kSegRadii[2] == AM_STEREO_MAX_RADIUS, "the widest kernel holds every radius");
static_assert(2 * AM_STEREO_MAX_RADIUS <= kStThreads && stereo_record_len(AM_STEREO_MAX_RADIUS) < kStThreads,
              "one staged tail frame and one record value per work item");

// The 2 RT + 1 sums of one channel over the work item's needle samples (lag_dot), then over each wave into ws[l][wave].
template <int RT>
__device__ __forceinline__ void st_channel(const float* xs, const float (&nv)[kStPer], int q0, bool active, double (*ws)[kStThreads / 64]) {
    constexpr int NL = 2 * RT + 1;
    double acc[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) acc[l] = 0.0;
    if (active) lag_dot<NL>(xs, nv, q0, acc);
    wave_sums<kStThreads>(acc, ws);
}

template <int RT>
__global__ __launch_bounds__(kStThreads, 2) void stereo_slices_kernel(const StereoDesc* __restrict__ hits, long long h0,
                                                                      double* __restrict__ parts, unsigned* __restrict__ pflags) {
    constexpr int NL = 2 * RT + 1, NV = stereo_record_len(RT), STAGED = kHitSlice + 2 * RT;
    __shared__ float xl[STAGED + (STAGED >> 4) + 1];
    __shared__ float xr[STAGED + (STAGED >> 4) + 1];
    __shared__ double ws[2 * NL][kStThreads / 64];
    __shared__ long long wi[3][kStThreads / 64];
    const StereoDesc d = hits[h0 + blockIdx.y];
    const long long i0 = (long long)blockIdx.x * kHitSlice;
    if (i0 >= d.s) return;   // (a shorter needle than the launch's longest: whole workgroups leave together)
    const int tid = threadIdx.x;
    const int cnt = (int)min((long long)kHitSlice, d.s - i0);
    // every load of the slice in flight at once: frame t + i0 - RT + q for q < cnt + 2 RT (0 where the hit reads no
    // frame), and the work item's needle samples.  (stage_load and stage_store written out: one 32-bit load feeds two arrays.)
    const long long u0 = i0 - RT;
    guint* fr = (guint*)d.win;
    unsigned fv[kStPer], ft = 0u;
#pragma unroll
    for (int k = 0; k < kStPer; ++k) {
        const int q = tid + k * kStThreads;
        const long long u = u0 + q;
        fv[k] = q < cnt + 2 * RT && u >= d.ulo && u < d.uhi ? fr[u] : 0u;
    }
    if (tid < 2 * RT) {
        const int q = kHitSlice + tid;
        const long long u = u0 + q;
        ft = q < cnt + 2 * RT && u >= d.ulo && u < d.uhi ? fr[u] : 0u;
    }
    const int q0 = tid * kStPer;
    gfloat* nd = (gfloat*)d.needle + (i0 + q0);
    float nv[kStPer];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) {
        nv[j] = q0 + j < cnt ? nd[j] : 0.0f;
        bad |= !__builtin_isfinite(nv[j]);
    }
#pragma unroll
    for (int k = 0; k < kStPer; ++k) {
        const int q = pad16(tid + k * kStThreads);
        xl[q] = (float)(short)(fv[k] & 0xffffu);
        xr[q] = (float)(short)(fv[k] >> 16);
    }
    if (tid < 2 * RT) {
        const int q = pad16(kHitSlice + tid);
        xl[q] = (float)(short)(ft & 0xffffu);
        xr[q] = (float)(short)(ft >> 16);
    }
    __syncthreads();
    const bool active = q0 < cnt;
    st_channel<RT>(xl, nv, q0, active, ws);
    st_channel<RT>(xr, nv, q0, active, ws + NL);
    // the energies at lag 0, in integers: the order of an integer sum does not matter
    long long si[3] = {0, 0, 0};   // S_LL, S_RR, S_LR
    if (active) {
#pragma unroll
        for (int j = 0; j < kStPer; ++j) {
            const int q = pad16(q0 + j + RT);
            const int a = q0 + j < cnt ? (int)xl[q] : 0, b = q0 + j < cnt ? (int)xr[q] : 0;
            si[0] += a * a;     // (|a|, |b| <= 2^15: a product fits an int)
            si[1] += b * b;
            si[2] += a * b;
        }
    }
    wave_sums<kStThreads>(si, wi);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    // one 64-bit store per lane: no record leaves as one wide store (tools/check_store_hazard.py)
    const long long p = d.part0 + blockIdx.x;
    if (tid < 2 * NL) parts[NV * p + tid] = add_waves<kStThreads>(ws[tid]);
    else if (tid < NV) reinterpret_cast<long long*>(parts)[NV * p + tid] = add_waves<kStThreads>(wi[tid - 2 * NL]);
    else if (tid == NV) pflags[p] = (unsigned)any_bad;
}

// the best lag of one channel over |c(l)|, l = -r .. r, with its parabola vertex
__device__ double st_lag(const double* cc, int r, bool* unrefined) {
    bool refined;
    const double lag = refine_lag<true>(cc, r, pick_lag<true>(cc, r), &refined);
    *unrefined = !refined;
    return lag;
}

// One wave per hit: lane k adds value k (and k + 64) of the hit's partial records (sum_slices), lane 0 turns the sums
// into the record.
__global__ __launch_bounds__(64) void stereo_combine_kernel(const StereoDesc* __restrict__ hits, int r, int rt,
                                                            const double* __restrict__ parts, const unsigned* __restrict__ pflags,
                                                            am_stereo_hit* __restrict__ out) {
    __shared__ double sh[2 * (2 * AM_STEREO_MAX_RADIUS + 1)];
    __shared__ long long si[3];
    const long long h = blockIdx.x;
    const int lane = threadIdx.x;
    const StereoDesc d = hits[h];
    const long long ns = (d.s + kHitSlice - 1) / kHitSlice, p0 = d.part0;
    const int nl = 2 * rt + 1, nv = stereo_record_len(rt);
    for (int k = lane; k < nv; k += 64) {
        if (k < 2 * nl) sh[k] = sum_slices(parts, nv, p0, ns, k);
        else si[k - 2 * nl] = sum_slices(reinterpret_cast<const long long*>(parts), nv, p0, ns, k);
    }
    const int bad = __syncthreads_or(or_flags(pflags, p0, ns, lane, 64) != 0 ? 1 : 0);
    if (lane != 0) return;
    const double kk = (double)(1.0f / 65535.0f), k2 = kk * kk;   // k = 2 kappa of norm_downmix
    const double* cl = sh + rt;   // cl[l] = C_L(l), cr[l] = C_R(l) for -rt <= l <= rt
    const double* cr = sh + nl + rt;
    const double en = d.en;
    const float nanf = __builtin_nanf("");
    double lag_l = 0.0, lag_r = 0.0;
    float ncc_l = 0.0f, ncc_r = 0.0f, ncc_m = 0.0f, ncc_s = 0.0f, ncc_b = 0.0f, g_l = 0.0f, g_r = 0.0f, m_l = 0.0f, m_r = 0.0f;
    unsigned flags = 0;
    if (bad) {
        flags = AM_HIT_NONFINITE;
        ncc_l = ncc_r = ncc_m = ncc_s = ncc_b = g_l = g_r = m_l = m_r = nanf;
    } else if (en == 0.0) {
        flags = AM_HIT_EMPTY_SEGMENT;
    } else {
        const long long sll = si[0], srr = si[1], slr = si[2];
        const double e_l = (double)sll * k2, e_r = (double)srr * k2, e_lr = (double)slr * k2;
        const double e_m = (double)(sll + 2 * slr + srr) * k2 * 0.25, e_d = (double)(sll - 2 * slr + srr) * k2 * 0.25;
        const double c_l = kk * cl[0], c_r = kk * cr[0];
        bool unref;
        lag_l = st_lag(cl, r, &unref);
        if (unref) flags |= AM_HIT_LEFT_UNREFINED;
        lag_r = st_lag(cr, r, &unref);
        if (unref) flags |= AM_HIT_RIGHT_UNREFINED;
        const double fl = en * d.floor_ratio;
        const bool sil_l = e_l == 0.0 || e_l < fl, sil_r = e_r == 0.0 || e_r < fl;
        const bool sil_m = e_m == 0.0 || e_m < fl, sil_d = e_d == 0.0 || e_d < fl;
        if (sil_l) flags |= AM_HIT_LEFT_SILENT;
        else ncc_l = (float)(c_l / sqrt(en * e_l));
        if (sil_r) flags |= AM_HIT_RIGHT_SILENT;
        else ncc_r = (float)(c_r / sqrt(en * e_r));
        if (sil_m) flags |= AM_HIT_BELOW_FLOOR;
        else ncc_m = (float)(0.5 * (c_l + c_r) / sqrt(en * e_m));
        if (sil_d) flags |= AM_HIT_SIDE_SILENT;
        else ncc_s = (float)(0.5 * (c_l - c_r) / sqrt(en * e_d));
        g_l = (float)(c_l / en);
        g_r = (float)(c_r / en);
        const double det = e_l * e_r - e_lr * e_lr;
        if (sil_l || sil_r || det <= AM_STEREO_MIN_INDEPENDENCE * e_l * e_r) {
            flags |= AM_HIT_COLLINEAR;
            if (!(sil_l && sil_r)) {
                if (e_l >= e_r) {   // (left wins a tie)
                    ncc_b = (float)(fabs(c_l) / sqrt(en * e_l));
                    m_l = (float)(c_l / e_l);
                } else {
                    ncc_b = (float)(fabs(c_r) / sqrt(en * e_r));
                    m_r = (float)(c_r / e_r);
                }
            }
        } else {
            const double q = (c_l * c_l * e_r - 2.0 * c_l * c_r * e_lr + c_r * c_r * e_l) / det;
            ncc_b = (float)sqrt(fmax(q, 0.0) / en);
            m_l = (float)((c_l * e_r - c_r * e_lr) / det);
            m_r = (float)((c_r * e_l - c_l * e_lr) / det);
        }
    }
    am_stereo_hit* o = out + h;
    o->lag_left = lag_l;
    o->lag_right = lag_r;
    o->ncc_left = ncc_l;
    o->ncc_right = ncc_r;
    o->ncc_mid = ncc_m;
    o->ncc_side = ncc_s;
    o->ncc_best = ncc_b;
    o->gain_left = g_l;
    o->gain_right = g_r;
    o->mix_left = m_l;
    o->mix_right = m_r;
    o->flags = flags;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 gu32x4;   // (four i16 stereo frames)

// out = f32((f64(a) L + f64(b) R) k): both products are exact, so the sum rounds once, the product once, the result once
__device__ __forceinline__ float mix_frame(unsigned f, double a, double b, double kk) {
    const double l = (double)(short)(f & 0xffffu), r = (double)(short)(f >> 16);
    return __double2float_rn(__dmul_rn(__dadd_rn(__dmul_rn(a, l), __dmul_rn(b, r)), kk));
}

// frames [0, head) and [head + 4 nq, frames) one by one, the nq quads between them as 16-byte stores (out + head is
// 16-byte aligned); WIDE_IN: in + 2 head is 16-byte aligned too, and a quad is one 16-byte load
template <bool WIDE_IN>
__global__ __launch_bounds__(256) void pcm_mix_kernel(const int16_t* __restrict__ in, long long frames, long long head, long long nq,
                                                      float a, float b, float* __restrict__ out) {
    const double da = (double)a, db = (double)b, kk = (double)(1.0f / 65535.0f);
    guint* fr = (guint*)in;
    const long long stride = (long long)gridDim.x * 256, g = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long v = g; v < nq; v += stride) {
        const long long i = head + 4 * v;
        u32x4 f;
        if (WIDE_IN) {
            f = *(gu32x4*)(fr + i);
        } else {
            f.x = fr[i]; f.y = fr[i + 1]; f.z = fr[i + 2]; f.w = fr[i + 3];
        }
        f32x4 o;
        o.x = mix_frame(f.x, da, db, kk); o.y = mix_frame(f.y, da, db, kk); o.z = mix_frame(f.z, da, db, kk); o.w = mix_frame(f.w, da, db, kk);
        // (the empty-looking asm keeps the data registers unwritten for two wait states behind the store: the store-data
        // hazard of DESIGN.md section 3, tools/check_store_hazard.py)
        *(__attribute__((address_space(1))) f32x4*)(out + i) = o;
        asm volatile("s_nop 1" : : "v"(o));
    }
    const long long tail0 = head + 4 * nq, ragged = head + (frames - tail0);
    for (long long v = g; v < ragged; v += stride) {
        const long long i = v < head ? v : tail0 + (v - head);
        out[i] = mix_frame(fr[i], da, db, kk);
    }
}

}  // namespace

hipError_t launch_hit_stereo(hipStream_t st, const StereoDesc* d_hits, long long n, int r, long long max_slices, double* parts,
                             unsigned* pflags, am_stereo_hit* d_out) {
    if (n <= 0) return hipSuccess;
    const int rt = seg_kernel_radius(r);
    const hipError_t e = for_each_grid_y(n, [&](long long h0, unsigned nh) {
        const dim3 grid((unsigned)max_slices, nh);
        if (rt == kSegRadii[0]) hipLaunchKernelGGL(stereo_slices_kernel<kSegRadii[0]>, grid, dim3(kStThreads), 0, st, d_hits, h0, parts, pflags);
        else if (rt == kSegRadii[1]) hipLaunchKernelGGL(stereo_slices_kernel<kSegRadii[1]>, grid, dim3(kStThreads), 0, st, d_hits, h0, parts, pflags);
        else hipLaunchKernelGGL(stereo_slices_kernel<kSegRadii[2]>, grid, dim3(kStThreads), 0, st, d_hits, h0, parts, pflags);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stereo_combine_kernel, dim3((unsigned)n), dim3(64), 0, st, d_hits, r, rt, (const double*)parts, (const unsigned*)pflags, d_out);
    return hipGetLastError();
}

hipError_t launch_pcm_mix(hipStream_t st, const int16_t* in, long long frames, float a, float b, float* out) {
    if (frames <= 0) return hipSuccess;
    // the frames before out reaches a 16-byte boundary (out is a float pointer: 4-byte aligned)
    const long long head = std::min<long long>(frames, (long long)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) / 4);
    const long long nq = (frames - head) / 4;
    const bool wide_in = (reinterpret_cast<uintptr_t>(in + 2 * head) & 15) == 0;
    // (one quad per work item up to 2^20 workgroups, the grid stride beyond: on a 1 h buffer a grid capped at 1024 .. 16384
    // workgroups took 0.23 .. 0.25 ms, this one 0.215 ms, pcm_downmix 0.223 ms; profiles/r21)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((nq + 255) / 256, kMixMaxBlocks));
    if (wide_in) hipLaunchKernelGGL(pcm_mix_kernel<true>, dim3(grid), dim3(256), 0, st, in, frames, head, nq, a, b, out);
    else hipLaunchKernelGGL(pcm_mix_kernel<false>, dim3(grid), dim3(256), 0, st, in, frames, head, nq, a, b, out);
    return hipGetLastError();
}

// ---- host side -------------------------------------------------------------------------------------------------------

namespace {

int score_stereo(Ctx* c, std::vector<StereoDesc>& hits, const am_stereo_params& sp, am_stereo_hit* const* out) {
    long long total = 0, max_slices = 0;
    for (StereoDesc& d : hits) {
        const long long ns = (d.s + kHitSlice - 1) / kHitSlice;
        d.part0 = total;
        total += ns;
        max_slices = std::max(max_slices, ns);
    }
    return hit_round_trip(c, hits, sizeof(double) * (size_t)stereo_record_len(seg_kernel_radius((int)sp.radius)), (size_t)total, 1, out,
                          [&](const StereoDesc* tab, double* parts, unsigned* pflags, am_stereo_hit* d_out) {
                              return launch_hit_stereo(c->stream, tab, (long long)hits.size(), (int)sp.radius, max_slices, parts, pflags, d_out);
                          });
}

// am_hit_stereo*: a hit at t reads the frames [t - R, t + S + R), clipped to the haystack
struct StereoFamily {
    typedef StereoDesc Desc;
    typedef am_stereo_hit Rec;
    const am_stereo_params* sp;
    int sample_format;
    const void* params() const { return sp; }
    size_t recs() const { return 1; }
    int check_call() const {
        if (sp->radius > AM_STEREO_MAX_RADIUS)
            return fail(AM_ERR_INVALID_ARG, "radius " + std::to_string(sp->radius) + " > AM_STEREO_MAX_RADIUS (" + std::to_string(AM_STEREO_MAX_RADIUS) + ")");
        if (sp->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_stereo_params: reserved != 0");
        if (sample_format != AM_FMT_S16_STEREO) return fail(AM_ERR_INVALID_ARG, "am_hit_stereo: needs interleaved i16 stereo frames");
        return AM_OK;
    }
    int check(const am_needle*, long long) const { return AM_OK; }
    double floor(const am_needle* h) const { return hit_floor_ratio(h); }
    // (checks as hit_desc does, same messages)
    int desc(const am_needle* h, const void* hay, size_t len, int fmt, const am_peak& pk, double ratio, const HitWhere& where,
             StereoDesc* d) const {
        HitDesc hd{};
        const long long r = sp->radius;
        int rc;
        if ((rc = hit_desc(h, hay, len, fmt, pk, 0.0, where, &hd))) return rc;
        *d = StereoDesc{hd.win, hd.needle, hd.s, -std::min(r, hd.t), std::min(hd.s + r, (long long)len - hd.t), 0, hd.en, ratio};
        return AM_OK;
    }
    HitRange span(const am_needle* h, size_t t, size_t len) const {
        const size_t r = sp->radius;
        return HitRange{t > r ? t - r : 0, std::min(len, t + h->n + r)};
    }
    int score(Ctx* c, std::vector<StereoDesc>& hits, am_stereo_hit* const* out) const { return score_stereo(c, hits, *sp, out); }
};

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_hit_stereo(const am_needle* h, const void* haystack, size_t len, int sample_format,
                  const am_peak* peaks, size_t n, const am_stereo_params* sp, am_stereo_hit* out) {
    return hit_call(StereoFamily{sp, sample_format}, true, h, haystack, len, sample_format, peaks, n, out);
}

int am_hit_stereo_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format,
                         const am_peak* peaks, size_t n, const am_stereo_params* sp, am_stereo_hit* out) {
    return hit_call(StereoFamily{sp, sample_format}, false, h, d_haystack, len, sample_format, peaks, n, out);
}

int am_hit_stereo_batch_device(const am_needle* const* needles, size_t n_needles,
                               const void* const* d_haystacks, const size_t* lens, size_t n_hay, int sample_format,
                               const am_peak* peaks, size_t cap_per_pair, const size_t* n_peaks,
                               const am_stereo_params* sp, am_stereo_hit* out) {
    return hit_call_batch(StereoFamily{sp, sample_format}, needles, n_needles, d_haystacks, lens, n_hay, sample_format, peaks, cap_per_pair,
                          n_peaks, out);
}

int am_hit_stereo_summary(const am_stereo_hit* rec, float min_ncc, am_stereo_summary* out) {
    if (!rec || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    am_stereo_summary r{};
    const double gl = std::fabs((double)rec->gain_left), gr = std::fabs((double)rec->gain_right);
    r.balance_db = 20.0 * std::log10(gl / gr);   // (+-inf for a silent side, NaN for 0 / 0)
    const bool has_l = std::fabs(rec->ncc_left) >= min_ncc, has_r = std::fabs(rec->ncc_right) >= min_ncc;
    r.delay = has_l && has_r ? rec->lag_left - rec->lag_right : std::nan("");
    r.downmix_loss_db = 20.0 * std::log10((double)rec->ncc_best / std::fabs((double)rec->ncc_mid));
    if (!(rec->ncc_best >= min_ncc)) r.image = AM_IMAGE_ABSENT;
    else if (has_l && !has_r) r.image = AM_IMAGE_LEFT;
    else if (has_r && !has_l) r.image = AM_IMAGE_RIGHT;
    else if (has_l && has_r && (rec->ncc_left < 0.0f) != (rec->ncc_right < 0.0f)) r.image = AM_IMAGE_INVERTED;
    else if (has_l && has_r && std::fabs(r.balance_db) <= 3.0) r.image = AM_IMAGE_CENTRE;
    else r.image = AM_IMAGE_PANNED;
    *out = r;
    return AM_OK;
}

int am_pcm_s16_stereo_mix_device(int device, const int16_t* d_in, size_t frames, float a, float b, float* d_out) {
    if (!d_in || !d_out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    AM_HIP(launch_pcm_mix(c->stream, d_in, (long long)frames, a, b, d_out));
    AM_HIP(hipStreamSynchronize(c->stream));
    return AM_OK;
}

int am_pcm_s16_stereo_mix(int device, const int16_t* interleaved, size_t frames, float a, float b, float* out) {
    if (!interleaved || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    if (frames == 0) return AM_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, interleaved, sample_bytes(frames), &d_in)) || (rc = c->io_out.ensure(frames * sizeof(float)))) return rc;
    AM_HIP(launch_pcm_mix(c->stream, (const int16_t*)d_in, (long long)frames, a, b, (float*)c->io_out.p));
    AM_HIP(hipStreamSynchronize(c->stream));
    return download(c, out, c->io_out.p, frames * sizeof(float));
}

}  // extern "C"
