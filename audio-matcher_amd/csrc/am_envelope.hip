// am_envelope.hip -- envelope matching (am_envelope*, am_envelope_scores*, am_envelope_pick, am_match_envelope*;
// include/audiomatch.h, "envelope matching"): a signal becomes a B x J matrix of integer band levels, one per band and
// frame; the needle's matrices, one per speed of a grid, are correlated against the haystack's matrix, and a host rule
// picks the places.  Everything behind the levels is integer arithmetic: any order of additions gives the same bits.
//
// The kernels, on the context's stream:
//   env_frames      one workgroup per (job, group of kEnvGroup consecutive frames), a job being one signal at one speed.
//                   Two frames share ONE F-point complex f64 FFT in LDS (z = x_j + i x_{j+1}; the transform of
//                   am_frames.h, window and twiddles from the host's f64 table), are untangled into |X_j[k]|^2 and |X_{j+1}[k]|^2, summed per band by one wave each and
//                   turned into levels.  A non-finite sample enters the transform as 0 and marks its frame ABSENT; a
//                   frame of zeros counts as X = 0 exactly.
//   env_needle_prep one workgroup per needle matrix: the matrix copied into the bank the correlation reads (rows padded
//                   with zeros to whole chunks, ABSENT as 0), N1_b, E and the matrix's absent / invalid flags.
//   env_block_sums, env_prefix   rows 0 .. B - 1: the haystack's levels per band, row B: the sum over the bands of their
//                   squares, row B + 1: the absent marks (an invalid level adds 2^32).  Each workgroup sums one block of
//                   kEnvBlock frames of one row; then each workgroup adds the sums of the blocks before its own and
//                   scans its block: P[row][i] = sum of the row's values before frame i, 64-bit, exact.
//   env_correlate   a workgroup owns AM_ENV_TILE consecutive t; lane l of every wave owns the 8 consecutive t from
//                   8 l on, wave w the needles q = w, w + 4, ...  The haystack rows [t0 + s, t0 + s + tile + span) of
//                   every band lie in LDS as 16-bit values (span: the longest needle, or as much as 48 KiB hold, the
//                   needles then walked in such spans); per band a lane keeps a window of 16 levels in 8 registers
//                   (one 16-byte LDS read per chunk of AM_ENV_CHUNK needle frames, conflict-free: consecutive lanes
//                   read consecutive addresses), the needle's chunk is four wave-uniform dwords, and 32 packed 16-bit
//                   dot products add 8 x 8 products to the lane's 8 sums.  Sums are 32-bit over at most 512 chunks
//                   (4096 products of at most 1023^2 < 2^32), then 64-bit.  The score of (t, q) is formed from the sum,
//                   the prefix sums and the needle's sums as the header defines it, the running best (score, q) stays
//                   in registers, and the four waves fold theirs through LDS: one haystack tile is read once for all Q.
#include "am_frames.h"
#include "am_reduce.h"

#include <climits>

namespace am {

namespace {

constexpr int kEnvThreads = kFrameThreads, kEnvLds = kFrameLds, kEnvBins = kFrameBins;
constexpr int kEnvGroup = 8;                                             // frames per workgroup: four transforms
constexpr int kEnvBlock = 4096;                                          // frames per block of the prefix sums: 16 per thread
constexpr int kTile = AM_ENV_TILE, kChunk = AM_ENV_CHUNK;
constexpr int kFlush = 512;                                              // chunks a 32-bit sum holds: 4096 products
constexpr int kEnvLdsBytes = 48 * 1024;                                  // the haystack rows of one workgroup
constexpr unsigned long long kInvalid = 1ull << 32;                      // what an invalid level adds to row B + 1
static_assert(kTile == 64 * 8 && kChunk == 8, "a lane owns 8 consecutive t and a window of 16 levels");
static_assert((unsigned long long)kFlush * kChunk * AM_ENV_MAX_LEVEL * AM_ENV_MAX_LEVEL < (1ull << 32), "a 32-bit sum holds kFlush chunks");
static_assert(sizeof(am_env_params) == 152 && sizeof(am_env_grid) == 24 && sizeof(am_env_pick) == 24 && sizeof(am_env_hit) == 32,
              "the envelope records have no padding");

// One signal at one speed: frame j < nframes starts at (j H inc + 2^31) >> 32 and goes to out[b nframes + j]
struct EnvJob {
    const void* src;
    unsigned short* out;
    unsigned long long inc;
    long long nframes;
    int kind, ngroups;
};
struct EnvArgs {
    am_band_params bp;
    double p0;   // (F / 4)^2 10^(-floor_db / 10)
};
// One needle matrix: B x J levels at off of the caller's bank, B x Jp at poff of the padded bank
struct EnvNeedle {
    long long off, poff, E;
    int J, Jp, absent, bad;
    int N1[AM_BAND_MAX_BANDS];
};

__global__ __launch_bounds__(kEnvThreads) void env_frames_kernel(const EnvJob* __restrict__ jobs, EnvArgs a, const double* __restrict__ tab) {
    __shared__ double sh[2 * kEnvLds];
    __shared__ unsigned wbits[kEnvThreads / 64];
    const EnvJob jb = jobs[blockIdx.y];
    if ((int)blockIdx.x >= jb.ngroups) return;   // (a job of fewer groups than the launch's largest: whole workgroups leave together)
    const int lf = (int)a.bp.frame_log2, F = 1 << lf, H = F >> 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* re = sh;
    double* im = sh + kEnvLds;
    const double2* tw = reinterpret_cast<const double2*>(tab + F);   // tw[k] = (cos, -sin)(2 pi k / F), k < F / 2
    const long long j0 = (long long)blockIdx.x * kEnvGroup;
    const int nfr = (int)min((long long)kEnvGroup, jb.nframes - j0);
    const int nb = (int)a.bp.n_bands;
    for (int f = 0; f < nfr; f += 2) {
        const bool two = f + 1 < nfr;
        // the frames' first samples: a + F <= len for every frame the host counted
        const unsigned long long a0 = ((unsigned long long)(j0 + f) * (unsigned long long)H * jb.inc + (1ull << 31)) >> 32;
        const unsigned long long a1 = two ? ((unsigned long long)(j0 + f + 1) * (unsigned long long)H * jb.inc + (1ull << 31)) >> 32 : a0;
        unsigned st = 0;   // bits 0, 1: the frame holds a sample that is not zero; bits 2, 3: one that is not finite
        for (int i = tid; i < F; i += kEnvThreads) {
            const float x0 = jb.kind ? norm_downmix(__builtin_bit_cast(short2, ((guint*)jb.src)[a0 + i])) : ((gfloat*)jb.src)[a0 + i];
            const float x1 = !two ? 0.0f : jb.kind ? norm_downmix(__builtin_bit_cast(short2, ((guint*)jb.src)[a1 + i])) : ((gfloat*)jb.src)[a1 + i];
            const bool f0 = __builtin_isfinite(x0), f1 = __builtin_isfinite(x1);
            st |= (x0 != 0.0f ? 1u : 0u) | (x1 != 0.0f ? 2u : 0u) | (f0 ? 0u : 4u) | (f1 ? 0u : 8u);
            const double w = tab[i];
            const int p = frame_slot(i, lf);
            re[p] = f0 ? (double)x0 * w : 0.0;
            im[p] = f1 ? (double)x1 * w : 0.0;
        }
        const unsigned any = frame_transform(re, im, tw, lf, st, wbits);
        // the two power spectra: X of frame j, Y of frame j + 1
        double pw[kEnvBins][2];
#pragma unroll
        for (int m = 0; m < kEnvBins; ++m) {
            const int k = tid + m * kEnvThreads;
            pw[m][0] = pw[m][1] = 0.0;
            if (k <= H) {
                const FrameBin z = frame_untangle(re, im, F, k);
                pw[m][0] = (any & 1u) ? z.xr * z.xr + z.xi * z.xi : 0.0;
                pw[m][1] = (any & 2u) ? z.yr * z.yr + z.yi * z.yi : 0.0;
            }
        }
        __syncthreads();   // (every spectrum value is read: the powers go where they were)
#pragma unroll
        for (int m = 0; m < kEnvBins; ++m) {
            const int k = tid + m * kEnvThreads;
            if (k <= H) {
                re[k] = pw[m][0];
                im[k] = pw[m][1];
            }
        }
        __syncthreads();
        // bins to bands: wave w forms level w, w + 4, ... of the 2 B (band, frame) pairs
        for (int q = wv; q < 2 * nb; q += kEnvThreads / 64) {
            const int b = q >> 1, which = q & 1;
            if (which && !two) continue;
            const double* src = which ? im : re;
            const double v = wave_bin_sum(src, (int)a.bp.edges[b], (int)a.bp.edges[b + 1]);
            if (lane == 0) {
                unsigned short u = (unsigned short)AM_ENV_ABSENT;
                if (!(any & (which ? 8u : 4u))) {
                    const long long l = llround((double)AM_ENV_STEPS_PER_DB * (10.0 * log10((v + a.p0) / a.p0)));
                    u = (unsigned short)min(l, (long long)AM_ENV_MAX_LEVEL);
                }
                jb.out[(long long)b * jb.nframes + j0 + f + which] = u;
            }
        }
        __syncthreads();   // (the next pair's samples go where these were read)
    }
}

// the workgroup's sum of v in every thread (integers: any order gives these bits), behind a barrier: sh (4 words) may still be read
__device__ __forceinline__ unsigned long long env_block_sum(unsigned long long v, unsigned long long* sh) {
    __syncthreads();
    return block_sum<kEnvThreads>(v, sh);
}

// frame i of row `row` of the haystack matrix e (B x n): see the file's head
__device__ __forceinline__ unsigned long long env_row_value(const unsigned short* __restrict__ e, long long n, int B, int row, long long i) {
    if (row < B) {
        const unsigned x = e[(long long)row * n + i];
        return x == AM_ENV_ABSENT ? 0ull : x;
    }
    unsigned long long sq = 0, marks = 0;
    bool absent = false;
    for (int b = 0; b < B; ++b) {
        const unsigned x = e[(long long)b * n + i];
        if (x == AM_ENV_ABSENT) absent = true;
        else if (x > AM_ENV_MAX_LEVEL) marks += kInvalid;
        else sq += (unsigned long long)(x * x);
    }
    return row == B ? sq : marks + (absent ? 1ull : 0ull);
}

// grid (blocks, B + 2): sums[row * nblk + k] = the sum of the row's values over block k
__global__ __launch_bounds__(kEnvThreads) void env_block_sums_kernel(const unsigned short* __restrict__ e, long long n, int B, long long nblk,
                                                                     unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[4];
    const int row = blockIdx.y;
    const long long i0 = (long long)blockIdx.x * kEnvBlock;
    unsigned long long v = 0;
    for (int k = threadIdx.x; k < kEnvBlock && i0 + k < n; k += kEnvThreads) v += env_row_value(e, n, B, row, i0 + k);
    v = env_block_sum(v, sh);
    if (threadIdx.x == 0) sums[(long long)row * nblk + blockIdx.x] = v;
}

// grid (blocks, B + 2): P[row * (n + 1) + i] = the sum of the row's values before frame i, i = 0 .. n
__global__ __launch_bounds__(kEnvThreads) void env_prefix_kernel(const unsigned short* __restrict__ e, long long n, int B, long long nblk,
                                                                 const unsigned long long* __restrict__ sums, unsigned long long* __restrict__ P) {
    __shared__ unsigned long long sh[4];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long carry = 0;
    for (long long k = tid; k < (long long)blockIdx.x; k += kEnvThreads) carry += sums[(long long)row * nblk + k];
    carry = env_block_sum(carry, sh);
    constexpr int kPer = kEnvBlock / kEnvThreads;
    const long long i0 = (long long)blockIdx.x * kEnvBlock + (long long)tid * kPer;
    unsigned long long v[kPer], tot = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        v[k] = i0 + k < n ? env_row_value(e, n, B, row, i0 + k) : 0ull;
        tot += v[k];
        v[k] = tot;   // inclusive within the thread
    }
    const unsigned long long inc = wave_scan_inclusive(tot);   // inclusive over the wave's threads
    __syncthreads();
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    unsigned long long base = carry + (inc - tot);
    for (int w = 0; w < wv; ++w) base += sh[w];
    volatile unsigned long long* out = P + (long long)row * (n + 1);   // (volatile: 64-bit stores, none merged into a wide one)
    if (blockIdx.x == 0 && tid == 0) out[0] = 0ull;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (i0 + k < n) out[i0 + k + 1] = base + v[k];
}

// One workgroup per needle: the padded copy and the sums
__global__ __launch_bounds__(kEnvThreads) void env_needle_prep_kernel(const unsigned short* __restrict__ raw, int B, EnvNeedle* __restrict__ nd,
                                                                      unsigned short* __restrict__ bank) {
    __shared__ unsigned long long sh[4];
    EnvNeedle& d = nd[blockIdx.x];
    const long long off = d.off, poff = d.poff;
    const int J = d.J, Jp = d.Jp;
    long long E = 0;
    unsigned long long flags = 0;   // bit 0: absent, bit 1: invalid
    for (int b = 0; b < B; ++b) {
        unsigned long long s1 = 0, s2 = 0;
        for (int j = threadIdx.x; j < Jp; j += kEnvThreads) {
            unsigned x = j < J ? raw[off + (long long)b * J + j] : 0u;
            if (x == AM_ENV_ABSENT) { flags |= 1; x = 0; }
            else if (x > AM_ENV_MAX_LEVEL) { flags |= 2; x = 0; }
            bank[poff + (long long)b * Jp + j] = (unsigned short)x;
            s1 += x;
            s2 += (unsigned long long)(x * x);
        }
        s1 = env_block_sum(s1, sh);
        s2 = env_block_sum(s2, sh);
        E += (long long)J * (long long)s2 - (long long)s1 * (long long)s1;
        if (threadIdx.x == 0) d.N1[b] = (int)s1;
    }
    const unsigned long long f1 = env_block_sum(flags & 1, sh), f2 = env_block_sum(flags >> 1, sh);
    if (threadIdx.x == 0) {
        d.E = E;
        d.absent = f1 != 0;
        d.bad = f2 != 0;
    }
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned dot2(unsigned a, unsigned b, unsigned c) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b), c, false);
}

struct CorrArgs {
    const unsigned short* hay;          // B x Jh
    const unsigned short* bank;         // the padded needle matrices
    const EnvNeedle* nd;
    const unsigned long long* P;        // (B + 2) x (Jh + 1)
    long long Jh, n_out;
    int B, Q;
    int span, lw, nspans;               // needle frames per staged span, levels per staged row (span + kTile), spans of the longest needle
};

__global__ __launch_bounds__(kEnvThreads) void env_correlate_kernel(CorrArgs a, float* __restrict__ z, unsigned* __restrict__ qi) {
    extern __shared__ __attribute__((aligned(16))) unsigned short rows[];   // B rows of a.lw levels
    __shared__ float fs[3][kTile];
    __shared__ unsigned fq[3][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long t0 = (long long)blockIdx.x * kTile;
    const int tl = lane * 8;
    const int B = a.B;
    float bs[8];
    unsigned bq[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { bs[r] = 0.0f; bq[r] = AM_ENV_NO_Q; }
    for (int g = 0; g * 4 < a.Q; ++g) {
        const int q = __builtin_amdgcn_readfirstlane(g * 4 + wv);
        const bool active = q < a.Q;
        int jp_max = 0;
        for (int k = g * 4; k < min(a.Q, g * 4 + 4); ++k) jp_max = max(jp_max, a.nd[k].Jp);
        const EnvNeedle* nq = a.nd + (active ? q : 0);
        const int J = nq->J, Jp = nq->Jp;
        const unsigned short* nbase = a.bank + nq->poff;
        long long acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0;
        for (int sp = 0; sp * a.span < jp_max; ++sp) {
            if (a.nspans > 1 || g == 0) {
                __syncthreads();   // (the rows may still be read)
                const long long s0 = t0 + (long long)sp * a.span;
                for (int idx = tid; idx < B * a.lw; idx += kEnvThreads) {
                    const int b = idx / a.lw, i = idx - b * a.lw;
                    unsigned x = s0 + i < a.Jh ? a.hay[(long long)b * a.Jh + s0 + i] : 0u;
                    if (x == AM_ENV_ABSENT) x = 0;
                    rows[idx] = (unsigned short)x;
                }
                __syncthreads();
            }
            if (!active) continue;
            const int c_lo = sp * (a.span / kChunk), c_hi = min(Jp / kChunk, (sp + 1) * (a.span / kChunk));
            for (int b = 0; b < B; ++b) {
                const unsigned short* row = rows + b * a.lw + tl - sp * a.span;    // row[j]: level t0 + tl + j of band b
                const unsigned short* nrow = nbase + (long long)b * Jp;
                for (int cb = c_lo; cb < c_hi; cb += kFlush) {
                    unsigned s32[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) s32[r] = 0;
                    const int ce = min(c_hi, cb + kFlush);
                    uint4 lo = *reinterpret_cast<const uint4*>(row + cb * kChunk);
                    uint4 hi = *reinterpret_cast<const uint4*>(row + cb * kChunk + kChunk);
                    uint4 nn = *reinterpret_cast<const uint4*>(nrow + cb * kChunk);   // wave-uniform
                    for (int c = cb; c < ce; ++c) {
                        // the next chunk's loads run beside this chunk's products (the last chunk loads itself again)
                        const int cn = min(c + 1, ce - 1);
                        const uint4 hi_next = *reinterpret_cast<const uint4*>(row + cn * kChunk + kChunk);
                        const uint4 nn_next = *reinterpret_cast<const uint4*>(nrow + cn * kChunk);
                        const unsigned E[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                        unsigned O[7];
#pragma unroll
                        for (int i = 0; i < 7; ++i) O[i] = __builtin_amdgcn_alignbit(E[i + 1], E[i], 16);
                        const unsigned N[4] = {nn.x, nn.y, nn.z, nn.w};
#pragma unroll
                        for (int r = 0; r < 8; ++r) {
#pragma unroll
                            for (int m = 0; m < 4; ++m) {
                                const int s = r + 2 * m;
                                s32[r] = dot2((s & 1) ? O[s >> 1] : E[s >> 1], N[m], s32[r]);
                            }
                        }
                        lo = hi;
                        hi = hi_next;
                        nn = nn_next;
                    }
#pragma unroll
                    for (int r = 0; r < 8; ++r) acc[r] += (long long)s32[r];
                }
            }
        }
        if (!active) continue;
        // the scores of needle q at the lane's 8 places
        const long long Tq = a.Jh >= J ? a.Jh - J + 1 : 0;
        const long long E = nq->E;
        const bool n_absent = nq->absent != 0;
        const long long stride = a.Jh + 1;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const long long t = t0 + tl + r;
            if (t >= Tq || n_absent) continue;
            if (a.P[(long long)(B + 1) * stride + t + J] != a.P[(long long)(B + 1) * stride + t]) continue;   // an absent frame: NaN
            long long num = (long long)J * acc[r];
            long long D = (long long)J * (long long)(a.P[(long long)B * stride + t + J] - a.P[(long long)B * stride + t]);
            for (int b = 0; b < B; ++b) {
                const long long s1 = (long long)(a.P[(long long)b * stride + t + J] - a.P[(long long)b * stride + t]);
                num -= (long long)nq->N1[b] * s1;
                D -= s1 * s1;
            }
            const float sc = (E == 0 || D == 0) ? 0.0f : (float)((double)num / sqrt((double)E * (double)D));
            if (bq[r] == AM_ENV_NO_Q || sc > bs[r]) { bs[r] = sc; bq[r] = (unsigned)q; }
        }
    }
    // the four waves' bests of a place into wave 0's: the larger score, ties to the lower q
    if (wv > 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) { fs[wv - 1][tl + r] = bs[r]; fq[wv - 1][tl + r] = bq[r]; }
    }
    __syncthreads();
    if (wv == 0) {
        volatile float* zo = z;      // (volatile: 32-bit stores, none merged into a wide one)
        volatile unsigned* qo = qi;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            for (int w = 0; w < 3; ++w) {
                const float s = fs[w][tl + r];
                const unsigned q = fq[w][tl + r];
                if (q != AM_ENV_NO_Q && (bq[r] == AM_ENV_NO_Q || s > bs[r] || (s == bs[r] && q < bq[r]))) { bs[r] = s; bq[r] = q; }
            }
            const long long t = t0 + tl + r;
            if (t < a.n_out) {
                zo[t] = bq[r] == AM_ENV_NO_Q ? __uint_as_float(0x7FC00000u) : bs[r];
                qo[t] = bq[r];
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

constexpr double kTwo32 = 4294967296.0;

unsigned long long env_inc(double d_ppm) { return (unsigned long long)std::llround(kTwo32 / (1.0 + d_ppm * 1e-6)); }
unsigned long long env_frame_start(unsigned long long j, int lf, unsigned long long inc) {
    return (j * (1ull << (lf - 1)) * inc + (1ull << 31)) >> 32;
}
// J: the count of j with a_j + F <= len (a_j ascends with j; len <= AM_ENV_MAX_LEN keeps j H inc inside 64 bits)
long long env_frames(size_t len, int lf, unsigned long long inc) {
    const unsigned long long F = 1ull << lf, H = F >> 1;
    if (len < F) return 0;
    unsigned long long j = (unsigned long long)((((unsigned __int128)(len - F)) << 32) / ((unsigned __int128)H * inc));   // near the last frame
    while (env_frame_start(j, lf, inc) + F > len) --j;       // (a_0 = 0: ends at j = 0 at the latest)
    while (env_frame_start(j + 1, lf, inc) + F <= len) ++j;
    return (long long)j + 1;
}

int env_check_params(const am_env_params* ep) {
    if (!ep) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (ep->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_env_params: reserved must be 0");
    int rc;
    if ((rc = band_check_params(&ep->bands))) return rc;
    if (!(ep->floor_db > 0.0) || !(ep->floor_db <= 200.0)) return fail(AM_ERR_INVALID_ARG, "am_env_params: floor_db must lie in (0, 200]");
    return AM_OK;
}
int env_check_drift(double d) {
    if (!(std::fabs(d) <= (double)AM_ENV_MAX_PPM)) return fail(AM_ERR_INVALID_ARG, "drift_ppm: |drift_ppm| > AM_ENV_MAX_PPM (" + std::to_string(AM_ENV_MAX_PPM) + ") or NaN");
    return AM_OK;
}
int env_check_len(size_t len) {
    if ((unsigned long long)len > AM_ENV_MAX_LEN) return fail(AM_ERR_INVALID_ARG, "len " + std::to_string(len) + " > AM_ENV_MAX_LEN (2^31): pass the signal in pieces");
    return AM_OK;
}
int env_check_grid(const am_env_grid* g) {
    if (!g) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (g->reserved != 0) return fail(AM_ERR_INVALID_ARG, "am_env_grid: reserved must be 0");
    if (g->steps > AM_ENV_MAX_STEPS) return fail(AM_ERR_INVALID_ARG, "am_env_grid: steps " + std::to_string(g->steps) + " > AM_ENV_MAX_STEPS (" + std::to_string(AM_ENV_MAX_STEPS) + ")");
    if (!(g->max_ppm >= 0.0) || !std::isfinite(g->max_ppm)) return fail(AM_ERR_INVALID_ARG, "am_env_grid: max_ppm must be finite and not negative");
    if (g->steps > 0 && g->max_ppm == 0.0) return fail(AM_ERR_INVALID_ARG, "am_env_grid: max_ppm = 0 with steps > 0");
    if (!(std::fabs(g->centre_ppm) + g->max_ppm <= (double)AM_ENV_MAX_PPM))
        return fail(AM_ERR_INVALID_ARG, "am_env_grid: |centre_ppm| + max_ppm > AM_ENV_MAX_PPM (" + std::to_string(AM_ENV_MAX_PPM) + ")");
    return AM_OK;
}
double env_grid_drift(const am_env_grid& g, int q) {   // d_q
    const int k = (int)g.steps;
    return k == 0 ? g.centre_ppm : g.centre_ppm + g.max_ppm * (double)(q - k) / (double)k;
}

// the levels of every job (on the host: `jobs`, the largest group count `max_groups`) in one launch
int env_launch_frames(Ctx* c, const std::vector<EnvJob>& jobs, int max_groups, const am_env_params& ep) {
    if (jobs.empty() || max_groups == 0) return AM_OK;
    const double* tab = nullptr;
    int rc;
    if ((rc = band_table(c, (int)ep.bands.frame_log2, &tab))) return rc;
    if ((rc = c->env_jobs.ensure(sizeof(EnvJob) * jobs.size()))) return rc;
    AM_HIP(copy_on_stream(c, c->env_jobs.p, jobs.data(), sizeof(EnvJob) * jobs.size(), hipMemcpyHostToDevice));
    EnvArgs a{};
    a.bp = ep.bands;
    const double f4 = (double)(1u << ep.bands.frame_log2) / 4.0;
    a.p0 = f4 * f4 * std::pow(10.0, -ep.floor_db / 10.0);
    ProfScope ps(c, KN_ENV_FRAMES, c->stream);
    hipLaunchKernelGGL(env_frames_kernel, dim3((unsigned)max_groups, (unsigned)jobs.size()), dim3(kEnvThreads), 0, c->stream,
                       (const EnvJob*)c->env_jobs.p, a, tab);
    AM_HIP(hipGetLastError());
    return AM_OK;
}
EnvJob env_job(const void* d_src, int kind, unsigned long long inc, long long nframes, unsigned short* d_out) {
    return EnvJob{d_src, d_out, inc, nframes, kind, (int)((nframes + kEnvGroup - 1) / kEnvGroup)};
}

int env_check_scores_args(const uint16_t* needles, const uint32_t* frames, uint32_t n_needles, uint32_t n_bands, const uint16_t* hay,
                          size_t hay_frames, const float* z, const uint32_t* qi, size_t cap, const size_t* n_out) {
    if (!needles || !frames || !n_out || (!hay && hay_frames) || ((!z || !qi) && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (n_needles == 0 || n_needles > AM_ENV_MAX_NEEDLES)
        return fail(AM_ERR_INVALID_ARG, "n_needles " + std::to_string(n_needles) + " outside 1 .. AM_ENV_MAX_NEEDLES (" + std::to_string(AM_ENV_MAX_NEEDLES) + ")");
    if (n_bands == 0 || n_bands > AM_BAND_MAX_BANDS)
        return fail(AM_ERR_INVALID_ARG, "n_bands " + std::to_string(n_bands) + " outside 1 .. AM_BAND_MAX_BANDS (" + std::to_string(AM_BAND_MAX_BANDS) + ")");
    for (uint32_t q = 0; q < n_needles; ++q)
        if (frames[q] == 0 || frames[q] > AM_ENV_MAX_FRAMES)
            return fail(AM_ERR_INVALID_ARG, "frames[" + std::to_string(q) + "] = " + std::to_string(frames[q]) + " outside 1 .. AM_ENV_MAX_FRAMES (" +
                                                std::to_string(AM_ENV_MAX_FRAMES) + ")");
    if (hay_frames > AM_ENV_MAX_HAY_FRAMES)
        return fail(AM_ERR_INVALID_ARG, "hay_frames " + std::to_string(hay_frames) + " > AM_ENV_MAX_HAY_FRAMES (2^24)");
    return AM_OK;
}

// z and qi (host, `cap` entries) of the resident matrices; trusted: the levels come from env_frames, nothing to validate.
// The caller holds the context's lock and has checked the arguments.
int env_scores_resident(Ctx* c, const uint16_t* d_needles, const uint32_t* frames, uint32_t Q, uint32_t B, const uint16_t* d_hay, size_t Jh,
                        bool trusted, float* z, uint32_t* qi, size_t cap, size_t* n_out) {
    std::vector<EnvNeedle> nd(Q);
    long long off = 0, poff = 0;
    int jp_max = 0;
    size_t n = 0;
    for (uint32_t q = 0; q < Q; ++q) {
        const int J = (int)frames[q], Jp = (J + kChunk - 1) / kChunk * kChunk;
        nd[q] = EnvNeedle{};
        nd[q].off = off; nd[q].poff = poff; nd[q].J = J; nd[q].Jp = Jp;
        off += (long long)B * J;
        poff += (long long)B * Jp;
        jp_max = std::max(jp_max, Jp);
        if (Jh >= (size_t)J) n = std::max(n, Jh - (size_t)J + 1);
    }
    *n_out = n;
    if (Jh == 0 || (trusted && n == 0)) return AM_OK;
    const long long nblk = ((long long)Jh + kEnvBlock - 1) / kEnvBlock;
    int rc;
    if ((rc = c->env_desc.ensure(sizeof(EnvNeedle) * Q)) || (rc = c->env_bank.ensure(sizeof(uint16_t) * (size_t)poff)) ||
        (rc = c->env_blocks.ensure(sizeof(uint64_t) * (size_t)(nblk * (B + 2)))) ||
        (rc = c->env_prefix.ensure(sizeof(uint64_t) * (size_t)(B + 2) * (Jh + 1))) || (rc = c->env_out.ensure(8 * std::max<size_t>(n, 1))))
        return rc;
    EnvNeedle* d_nd = (EnvNeedle*)c->env_desc.p;
    unsigned long long* d_sums = (unsigned long long*)c->env_blocks.p;
    unsigned long long* d_P = (unsigned long long*)c->env_prefix.p;
    AM_HIP(copy_on_stream(c, d_nd, nd.data(), sizeof(EnvNeedle) * Q, hipMemcpyHostToDevice));
    {
        ProfScope ps(c, KN_ENV_PREFIX, c->stream);
        hipLaunchKernelGGL(env_needle_prep_kernel, dim3(Q), dim3(kEnvThreads), 0, c->stream, d_needles, (int)B, d_nd, (unsigned short*)c->env_bank.p);
        AM_HIP(hipGetLastError());
        hipLaunchKernelGGL(env_block_sums_kernel, dim3((unsigned)nblk, B + 2), dim3(kEnvThreads), 0, c->stream, d_hay, (long long)Jh, (int)B, nblk, d_sums);
        AM_HIP(hipGetLastError());
        hipLaunchKernelGGL(env_prefix_kernel, dim3((unsigned)nblk, B + 2), dim3(kEnvThreads), 0, c->stream, d_hay, (long long)Jh, (int)B, nblk,
                           (const unsigned long long*)d_sums, d_P);
        AM_HIP(hipGetLastError());
    }
    if (!trusted) {   // a level above AM_ENV_MAX_LEVEL that is not AM_ENV_ABSENT: the flags the two kernels left
        std::vector<unsigned long long> marks((size_t)nblk);
        AM_HIP(hipMemcpyAsync(nd.data(), d_nd, sizeof(EnvNeedle) * Q, hipMemcpyDeviceToHost, c->stream));
        if ((rc = download(c, marks.data(), d_sums + (size_t)(B + 1) * (size_t)nblk, sizeof(uint64_t) * (size_t)nblk))) return rc;
        for (uint32_t q = 0; q < Q; ++q)
            if (nd[q].bad) return fail(AM_ERR_INVALID_ARG, "needles: matrix " + std::to_string(q) + " holds a level above AM_ENV_MAX_LEVEL that is not AM_ENV_ABSENT");
        for (unsigned long long m : marks)
            if (m >= kInvalid) return fail(AM_ERR_INVALID_ARG, "hay: a level above AM_ENV_MAX_LEVEL that is not AM_ENV_ABSENT");
    }
    if (n > 0) {
        CorrArgs a{};
        a.hay = d_hay; a.bank = (const unsigned short*)c->env_bank.p; a.nd = d_nd; a.P = d_P;
        a.Jh = (long long)Jh; a.n_out = (long long)n; a.B = (int)B; a.Q = (int)Q;
        const int lw_max = kEnvLdsBytes / 2 / (int)B / kChunk * kChunk;   // levels per row that the LDS budget holds
        a.span = std::min(jp_max, lw_max - kTile);
        a.lw = a.span + kTile;
        a.nspans = (jp_max + a.span - 1) / a.span;
        float* d_z = (float*)c->env_out.p;
        unsigned* d_qi = (unsigned*)(d_z + n);
        {
            ProfScope ps(c, KN_ENV_CORR, c->stream);
            hipLaunchKernelGGL(env_correlate_kernel, dim3((unsigned)((n + kTile - 1) / kTile)), dim3(kEnvThreads), sizeof(uint16_t) * (size_t)B * (size_t)a.lw,
                               c->stream, a, d_z, d_qi);
            AM_HIP(hipGetLastError());
        }
        const size_t m = std::min(n, cap);
        if (m) {
            AM_HIP(hipMemcpyAsync(z, d_z, sizeof(float) * m, hipMemcpyDeviceToHost, c->stream));
            AM_HIP(hipMemcpyAsync(qi, d_qi, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, c->stream));
        }
    }
    AM_HIP(hipStreamSynchronize(c->stream));
    if (n > cap) return fail(AM_ERR_CAPACITY, "envelope score buffers too small");
    return AM_OK;
}

int env_scores_impl(int device, const uint16_t* needles, const uint32_t* frames, uint32_t Q, uint32_t B, const uint16_t* hay, size_t Jh,
                    float* z, uint32_t* qi, size_t cap, size_t* n_out, bool device_io) {
    int rc = env_check_scores_args(needles, frames, Q, B, hay, Jh, z, qi, cap, n_out);
    if (rc) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    size_t total = 0;
    for (uint32_t q = 0; q < Q; ++q) total += (size_t)B * frames[q];
    const uint16_t* d_needles = needles;
    const uint16_t* d_hay = hay;
    if (device_io) {
        if ((rc = check_device_arg(needles, c->device, "am_envelope_scores_device: d_needles: "))) return rc;
        if (Jh && (rc = check_device_arg(hay, c->device, "am_envelope_scores_device: d_hay: "))) return rc;
    } else {
        if ((rc = c->env_needles.ensure(sizeof(uint16_t) * total)) || (rc = c->env_hay.ensure(sizeof(uint16_t) * std::max<size_t>((size_t)B * Jh, 1)))) return rc;
        AM_HIP(copy_on_stream(c, c->env_needles.p, needles, sizeof(uint16_t) * total, hipMemcpyHostToDevice));
        if (Jh) AM_HIP(copy_on_stream(c, c->env_hay.p, hay, sizeof(uint16_t) * (size_t)B * Jh, hipMemcpyHostToDevice));
        d_needles = (const uint16_t*)c->env_needles.p;
        d_hay = (const uint16_t*)c->env_hay.p;
    }
    return env_scores_resident(c, d_needles, frames, Q, B, d_hay, Jh, false, z, qi, cap, n_out);
}

int env_envelope_impl(int device, const void* signal, size_t len, int sample_format, const am_env_params* ep, double drift_ppm, uint16_t* out,
                      size_t cap, size_t* n_frames, bool device_io) {
    int rc;
    if ((rc = env_check_params(ep)) || (rc = env_check_drift(drift_ppm)) || (rc = check_format(sample_format)) || (rc = env_check_len(len))) return rc;
    if (!n_frames || (!signal && len) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    const unsigned long long inc = env_inc(drift_ppm);
    const long long J = env_frames(len, (int)ep->bands.frame_log2, inc);
    *n_frames = (size_t)J;
    if (J == 0) return AM_OK;
    if ((size_t)J > cap) return fail(AM_ERR_CAPACITY, "envelope output buffer too small");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_src = nullptr;
    if ((rc = resident_input(c, device_io, signal, sample_bytes(len), &d_src, "am_envelope_device: d_signal: "))) return rc;
    const size_t bytes = sizeof(uint16_t) * (size_t)ep->bands.n_bands * (size_t)J;
    if ((rc = c->env_hay.ensure(bytes))) return rc;
    const EnvJob jb = env_job(d_src, sample_format == AM_FMT_S16_STEREO ? 1 : 0, inc, J, (unsigned short*)c->env_hay.p);
    if ((rc = env_launch_frames(c, {jb}, jb.ngroups, *ep))) return rc;
    return download(c, out, c->env_hay.p, bytes);
}

// the pick rule on host arrays
void env_pick(const float* z, const uint32_t* qi, size_t n, float min_score, uint64_t sep, std::vector<am_env_pick>& out) {
    for (size_t t = 0; t < n; ++t) {
        const float v = z[t];
        if (v != v || !(v >= min_score)) continue;
        const size_t lo = (uint64_t)t > sep ? t - (size_t)sep : 0, hi = sep >= (uint64_t)(n - 1 - t) ? n - 1 : t + (size_t)sep;
        bool keep = true;
        for (size_t u = lo; u <= hi && keep; ++u) {
            if (u == t) continue;
            if (z[u] > v || (z[u] == v && u < t)) keep = false;
        }
        if (!keep) continue;
        double e = 0.0;
        if (t > 0 && t + 1 < n && z[t - 1] == z[t - 1] && z[t + 1] == z[t + 1]) {
            const double a = (double)z[t - 1], b = (double)v, c = (double)z[t + 1], den = a - 2.0 * b + c;
            if (den < 0.0) e = std::min(0.5, std::max(-0.5, (a - c) / (2.0 * den)));
        }
        out.push_back(am_env_pick{(uint64_t)t, (double)t + e, v, qi[t]});
    }
}

// am_match_envelope on a resident haystack.  The caller holds the context's lock and has checked the arguments.
int env_match_resident(const am_needle* h, const void* d_hay, size_t len, int sample_format, const am_env_params* ep, const am_env_grid* grid,
                       float min_score, am_env_hit* out, size_t cap, size_t* n_out) {
    Ctx* c = h->ctx;
    const int lf = (int)ep->bands.frame_log2, K = (int)grid->steps, Q = 2 * K + 1;
    const uint32_t B = ep->bands.n_bands;
    std::vector<uint32_t> frames((size_t)Q);
    std::vector<double> drift((size_t)Q);
    std::vector<EnvJob> jobs;
    size_t total = 0;
    int max_groups = 0;
    for (int q = 0; q < Q; ++q) {
        drift[q] = env_grid_drift(*grid, q);
        const unsigned long long inc = env_inc(drift[q]);
        const long long J = env_frames(h->n, lf, inc);
        if (J == 0)
            return fail(AM_ERR_INVALID_ARG, "needle length " + std::to_string(h->n) + " holds no frame of " + std::to_string(1u << lf) +
                                                " samples: use a smaller frame_log2");
        if (J > AM_ENV_MAX_FRAMES)
            return fail(AM_ERR_INVALID_ARG, "the needle has " + std::to_string(J) + " frames at " + std::to_string(drift[q]) + " ppm, more than AM_ENV_MAX_FRAMES (" +
                                                std::to_string(AM_ENV_MAX_FRAMES) + "): use a larger frame_log2");
        frames[q] = (uint32_t)J;
        jobs.push_back(env_job(h->d_needle, 0, inc, J, nullptr));
        max_groups = std::max(max_groups, jobs.back().ngroups);
        total += (size_t)B * (size_t)J;
    }
    *n_out = 0;
    const long long Jh = env_frames(len, lf, env_inc(0.0));
    if (Jh == 0) return AM_OK;
    int rc;
    if ((rc = c->env_needles.ensure(sizeof(uint16_t) * total)) || (rc = c->env_hay.ensure(sizeof(uint16_t) * (size_t)B * (size_t)Jh))) return rc;
    size_t at = 0;
    for (int q = 0; q < Q; ++q) {
        jobs[q].out = (unsigned short*)c->env_needles.p + at;
        at += (size_t)B * frames[q];
    }
    if ((rc = env_launch_frames(c, jobs, max_groups, *ep))) return rc;
    const EnvJob hj = env_job(d_hay, sample_format == AM_FMT_S16_STEREO ? 1 : 0, env_inc(0.0), Jh, (unsigned short*)c->env_hay.p);
    if ((rc = env_launch_frames(c, {hj}, hj.ngroups, *ep))) return rc;
    size_t n = 0;
    for (int q = 0; q < Q; ++q)
        if ((size_t)Jh >= frames[q]) n = std::max(n, (size_t)Jh - frames[q] + 1);
    std::vector<float> z(std::max<size_t>(n, 1));
    std::vector<uint32_t> qi(std::max<size_t>(n, 1));
    if ((rc = env_scores_resident(c, (const uint16_t*)c->env_needles.p, frames.data(), (uint32_t)Q, B, (const uint16_t*)c->env_hay.p, (size_t)Jh, true,
                                  z.data(), qi.data(), n, &n)))
        return rc;
    std::vector<am_env_pick> picks;
    env_pick(z.data(), qi.data(), n, min_score, (uint64_t)frames[K], picks);
    const double H = (double)(1u << (lf - 1));
    std::vector<am_env_hit> hits;
    for (const am_env_pick& p : picks) {
        const double d = drift[p.q];
        const long long s = std::llround(p.pos * H);
        am_env_hit r{};
        r.start = (uint64_t)std::min<long long>(std::max<long long>(s, 0), (long long)len - 1);
        r.length = (uint64_t)std::llround((double)h->n * (1.0 + d * 1e-6));
        r.drift_ppm = d;
        r.score = p.score;
        r.q = p.q;
        hits.push_back(r);
    }
    return hand_back(hits, out, cap, n_out, "envelope hit buffer too small");
}

int env_match_impl(const am_needle* h, const void* hay, size_t len, int sample_format, const am_env_params* ep, const am_env_grid* grid,
                   float min_score, am_env_hit* out, size_t cap, size_t* n_out, bool device_io) {
    int rc;
    if ((rc = check_needle(h)) || (rc = env_check_params(ep)) || (rc = env_check_grid(grid)) || (rc = check_format(sample_format)) ||
        (rc = env_check_len(len)) || (rc = env_check_len(h->n)))
        return rc;
    if (!n_out || (!hay && len) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (min_score != min_score) return fail(AM_ERR_INVALID_ARG, "min_score is NaN");
    Ctx* c = h->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_hay = hay;   // (an empty haystack is neither checked nor uploaded)
    if (len && (rc = resident_input(c, device_io, hay, sample_bytes(len), &d_hay, "am_match_envelope_device: d_haystack: "))) return rc;
    return env_match_resident(h, d_hay, len, sample_format, ep, grid, min_score, out, cap, n_out);
}

}  // namespace

}  // namespace am

using namespace am;

extern "C" {

int am_envelope_len(size_t len, const am_env_params* ep, double drift_ppm, size_t* n_frames) {
    int rc;
    if ((rc = env_check_params(ep)) || (rc = env_check_drift(drift_ppm)) || (rc = env_check_len(len))) return rc;
    if (!n_frames) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n_frames = (size_t)env_frames(len, (int)ep->bands.frame_log2, env_inc(drift_ppm));
    return AM_OK;
}

int am_envelope(int device, const void* signal, size_t len, int sample_format, const am_env_params* ep, double drift_ppm, uint16_t* out,
                size_t cap, size_t* n_frames) {
    return env_envelope_impl(device, signal, len, sample_format, ep, drift_ppm, out, cap, n_frames, false);
}

int am_envelope_device(int device, const void* d_signal, size_t len, int sample_format, const am_env_params* ep, double drift_ppm,
                       uint16_t* out, size_t cap, size_t* n_frames) {
    return env_envelope_impl(device, d_signal, len, sample_format, ep, drift_ppm, out, cap, n_frames, true);
}

int am_envelope_scores(int device, const uint16_t* needles, const uint32_t* frames, uint32_t n_needles, uint32_t n_bands, const uint16_t* hay,
                       size_t hay_frames, float* z, uint32_t* qi, size_t cap, size_t* n_out) {
    return env_scores_impl(device, needles, frames, n_needles, n_bands, hay, hay_frames, z, qi, cap, n_out, false);
}

int am_envelope_scores_device(int device, const uint16_t* d_needles, const uint32_t* frames, uint32_t n_needles, uint32_t n_bands,
                              const uint16_t* d_hay, size_t hay_frames, float* z, uint32_t* qi, size_t cap, size_t* n_out) {
    return env_scores_impl(device, d_needles, frames, n_needles, n_bands, d_hay, hay_frames, z, qi, cap, n_out, true);
}

int am_envelope_pick(const float* z, const uint32_t* qi, size_t n, float min_score, uint64_t separation, am_env_pick* out, size_t cap,
                     size_t* n_out) {
    if (!n_out || ((!z || !qi) && n) || (!out && cap)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (min_score != min_score) return fail(AM_ERR_INVALID_ARG, "min_score is NaN");
    std::vector<am_env_pick> picks;
    env_pick(z, qi, n, min_score, separation, picks);
    return hand_back(picks, out, cap, n_out, "envelope pick buffer too small");
}

int am_match_envelope(const am_needle* h, const void* haystack, size_t len, int sample_format, const am_env_params* ep,
                      const am_env_grid* grid, float min_score, am_env_hit* out, size_t cap, size_t* n_out) {
    return env_match_impl(h, haystack, len, sample_format, ep, grid, min_score, out, cap, n_out, false);
}

int am_match_envelope_device(const am_needle* h, const void* d_haystack, size_t len, int sample_format, const am_env_params* ep,
                             const am_env_grid* grid, float min_score, am_env_hit* out, size_t cap, size_t* n_out) {
    return env_match_impl(h, d_haystack, len, sample_format, ep, grid, min_score, out, cap, n_out, true);
}

}  // extern "C"
