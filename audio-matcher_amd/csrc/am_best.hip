// am_best.hip -- the k best matches of a needle (am_match_best*, am_find_peaks_top*; include/audiomatch.h, "the k
// best matches"): a grid-wide selection of the k best peaks of a dense score array that never computes the prominence
// of every local maximum and never sorts all of them.
//
// Why it is exact: in find_peaks' greedy distance filter (by descending height, every PeakPolicy variant) a lower
// peak never removes a higher one, and a prominence depends only on the peak and the raw scores.  So the first k
// survivors of the whole array are the first k survivors of the candidate set {local maxima of height >= tau}, for
// any tau at which that set already yields k survivors -- provided the set holds every maximum of height tau (a bin
// of the height histogram is never split, so ties at tau are all in).
//
//   1. best_scan (one read of the scores): local maxima with the plateau rule of am_peaks.hip (the tile that holds a
//      plateau's left edge resolves it), a histogram of their heights over the top 12 bits of an order-preserving
//      key, the highest key per 1024-score tile, the tile (min, max) summaries the prominence walk reads (tile_stats
//      layout) and the positions where the scores turn non-finite or finite again;
//   2. the host picks tau = the lower edge of the bin that holds the M-th largest maximum (M = max(8k, 4096)); a
//      crowded bin is split once more by best_refine (the next 12 bits, only tiles whose top key reaches the bin);
//   3. best_compact lists the maxima with tau <= key < (the previous tau) -- only tiles whose top key reaches tau;
//   4. best_prom: one wavefront per listed candidate runs the walk of am_peaks.hip (am_walk.h), bounded by the
//      candidate's finite stretch;
//   5. the host orders the list (height descending, start ascending: the order find_peaks filters in -- the list's
//      own order comes from atomics and is never used) and applies min_prominence and the distance rule in the
//      order "peak_filter_order" says, stopping at k;
//   6. fewer than k, and maxima below tau left: M grows eightfold and 2-5 run for the new candidates only.  Past
//      kBestCap candidates an all-finite array falls back to the whole-array pick (find_peaks_host_array) and
//      truncates it, which is exact by definition; an array with non-finite scores keeps descending.
#include "am_internal.h"

#include <float.h>
#include <climits>
#include <set>

namespace am {

#include "am_walk.h"

constexpr int kBestBins = 4096;                 // 12 key bits per histogram level
constexpr int kBestScanBlocks = 2048;           // blocks of the grid-stride scan (8 per CU)
constexpr unsigned kBestTransCap = 4096;        // transitions the scan lists itself (more: a second, listing pass)
constexpr long long kBestCap = 1ll << 20;       // candidates before the fallback to the whole-array pick

struct BestCand { long long ps, pe; float h, prom; };   // 24 bytes

// counters of a selection (device side, after the two histograms in best_ctl)
struct BestCounters { unsigned long long nmax; unsigned ntrans, nlist; };

// order-preserving key of a height (-0.0 and +0.0 are one height: one key); a larger key is a larger height
__device__ __forceinline__ unsigned height_key(float h) {
    const unsigned u = __float_as_uint(h + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Is i (0 < i, finite x = g[i] and xl = g[i - 1]) the left edge of a flat-topped local maximum?  Then *pe = the end
// of its plateau (exclusive).  A maximum needs finite neighbours on both sides: a non-finite score ends a stretch.
// `near` reads scores of [lo, hi) from a staged copy, everything else from g.
struct Near { const float* s; long long lo, hi; };
__device__ __forceinline__ float near_at(const float* __restrict__ g, const Near& nr, long long k) {
    return (k >= nr.lo && k < nr.hi) ? nr.s[k - nr.lo] : g[k];
}
__device__ __forceinline__ bool max_at(const float* __restrict__ g, long long n, const Near& nr, long long i, float xl, float x,
                                       long long* pe) {
    if (i < 1 || i >= n - 1 || not_finite(x) || not_finite(xl) || !(xl < x)) return false;
    long long k = i + 1;
    float xr = near_at(g, nr, k);
    while (xr == x && k < n - 1) xr = near_at(g, nr, ++k);
    if (xr == x || not_finite(xr) || !(xr < x)) return false;
    *pe = k;
    return true;
}

// ---------------------------------------------------------------------------
// Step 1.  mode 0: everything; mode 1: the transitions only (any float array: also the haystack's samples).
// A transition is an i in [0, n] with finite(x[i]) != finite(x[i - 1]), where x[-1] and x[n] count as finite: the
// non-finite runs of x are [t0, t1), [t2, t3), ...
struct BestScan {
    const float* g;
    long long n, ntiles;
    float2* stats;            // per tile (min, max), tile_stats layout
    unsigned* lmax;           // per tile the largest key of the maxima whose left edge it holds (0: none)
    unsigned* hist;           // kBestBins counts
    BestCounters* cnt;
    long long* trans;         // up to trans_cap transitions (any order)
    unsigned trans_cap;
    int mode;
};

__global__ void __launch_bounds__(256) best_scan(BestScan s) {
    __shared__ unsigned hist[kBestBins];
    __shared__ float win[kTile + 2];
    __shared__ unsigned red_key[4], red_n[4];
    __shared__ float red_mn[4], red_mx[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (s.mode == 0)
        for (int b = tid; b < kBestBins; b += 256) hist[b] = 0u;
    unsigned long long nmax = 0;
    // four consecutive scores per thread, the next tile's loaded before this one is looked at
    auto load = [&](long long t, float (&v)[4], float& halo) {
        const long long i0 = t * kTile + 4 * tid;
        if (i0 + 3 < s.n && ((reinterpret_cast<uintptr_t>(s.g + i0) & 15) == 0)) {
            const float4 q = *reinterpret_cast<const float4*>(s.g + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = i0 + j < s.n ? s.g[i0 + j] : __uint_as_float(0x7FC00000u);
        }
        // thread 0: the score before the tile; thread 1: the score after it
        const long long hi = tid == 0 ? t * kTile - 1 : t * kTile + kTile;
        halo = (tid < 2 && hi >= 0 && hi < s.n) ? s.g[hi] : __uint_as_float(0x7FC00000u);
    };
    float v[4], halo, nv[4], nhalo;
    long long t = blockIdx.x;
    if (t < s.ntiles) load(t, v, halo);
    for (; t < s.ntiles; t += gridDim.x) {
        const long long nt = t + gridDim.x;
        if (nt < s.ntiles) load(nt, nv, nhalo);
        const long long base = t * kTile;
        __syncthreads();   // (win of the previous tile no longer read)
#pragma unroll
        for (int j = 0; j < 4; ++j) win[1 + 4 * tid + j] = v[j];
        if (tid == 0) win[0] = halo;
        if (tid == 1) win[kTile + 1] = halo;
        __syncthreads();
        // transitions
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = base + 4 * tid + j;
            if (i > s.n) break;
            const bool f = i == s.n ? true : !not_finite(win[1 + 4 * tid + j]);
            const bool fp = i == 0 ? true : !not_finite(win[4 * tid + j]);
            if (f != fp) {
                const unsigned slot = atomicAdd(&s.cnt->ntrans, 1u);
                if (slot < s.trans_cap) s.trans[slot] = i;
            }
        }
        // (the end of the array when it is a multiple of kTile lies in no tile)
        if (base + kTile == s.n && tid == 0 && not_finite(win[kTile])) {
            const unsigned slot = atomicAdd(&s.cnt->ntrans, 1u);
            if (slot < s.trans_cap) s.trans[slot] = s.n;
        }
        if (s.mode == 0) {
            float mn = FLT_MAX, mx = -FLT_MAX;
            unsigned kmax = 0u, cnt = 0u;
            const Near nr{win, base - 1, base + kTile + 1};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long i = base + 4 * tid + j;
                if (i >= s.n) break;
                const float x = win[1 + 4 * tid + j];
                mn = fminf(mn, x); mx = fmaxf(mx, x);
                long long pe;
                if (max_at(s.g, s.n, nr, i, win[4 * tid + j], x, &pe)) {
                    const unsigned key = height_key(x);
                    atomicAdd(&hist[key >> 20], 1u);
                    kmax = key > kmax ? key : kmax;
                    ++cnt;
                }
            }
            mn = wave_min(mn); mx = wave_max(mx);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned ok = __shfl_xor(kmax, o);
                kmax = ok > kmax ? ok : kmax;
                cnt += __shfl_xor(cnt, o);
            }
            if (lane == 0) { red_mn[wv] = mn; red_mx[wv] = mx; red_key[wv] = kmax; red_n[wv] = cnt; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 4; ++w) {
                    mn = fminf(mn, red_mn[w]); mx = fmaxf(mx, red_mx[w]);
                    kmax = red_key[w] > kmax ? red_key[w] : kmax;
                    cnt += red_n[w];
                }
                s.stats[t] = make_float2(mn, mx);
                s.lmax[t] = kmax;
                nmax += cnt;
            }
        }
        if (nt < s.ntiles) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = nv[j];
            halo = nhalo;
        }
    }
    if (s.mode != 0) return;
    if (tid == 0 && nmax) atomicAdd(&s.cnt->nmax, nmax);
    __syncthreads();
    for (int b = tid; b < kBestBins; b += 256)
        if (hist[b]) atomicAdd(&s.hist[b], hist[b]);
}

// ---------------------------------------------------------------------------
// Steps 2 and 3 share a tile visitor: one wavefront per tile whose top key reaches `lo_key`, 16 scores per lane,
// every maximum of the tile with lo_key <= key < hi_key handed to `fn`.
template <class Fn>
__device__ __forceinline__ void visit_maxima(const float* __restrict__ g, long long n, long long ntiles, const unsigned* __restrict__ lmax,
                                             unsigned lo_key, unsigned long long hi_key, Fn fn) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const Near none{nullptr, 0, 0};
    for (long long t = wave; t < ntiles; t += nwaves) {
        if (lmax[t] < lo_key) continue;
        const long long base = t * kTile;
        for (int j = 0; j < kTile / 64; ++j) {
            const long long i = base + j * 64 + lane;
            if (i < 1 || i >= n - 1) continue;
            const float x = g[i];
            long long pe;
            if (!max_at(g, n, none, i, g[i - 1], x, &pe)) continue;
            const unsigned key = height_key(x);
            if (key >= lo_key && (unsigned long long)key < hi_key) fn(i, pe, x, key);
        }
    }
}

// the second histogram level of bin `bin`: the next 12 key bits of its maxima
__global__ void __launch_bounds__(256) best_refine(const float* __restrict__ g, long long n, long long ntiles, const unsigned* __restrict__ lmax,
                                                   unsigned bin, unsigned* hist2) {
    __shared__ unsigned hist[kBestBins];
    for (int b = threadIdx.x; b < kBestBins; b += 256) hist[b] = 0u;
    __syncthreads();
    visit_maxima(g, n, ntiles, lmax, bin << 20, ((unsigned long long)bin + 1) << 20,
                 [&](long long, long long, float, unsigned key) { atomicAdd(&hist[(key >> 8) & 0xFFFu], 1u); });
    __syncthreads();
    for (int b = threadIdx.x; b < kBestBins; b += 256)
        if (hist[b]) atomicAdd(&hist2[b], hist[b]);
}

// the maxima with lo_key <= key < hi_key, appended in any order (the host orders them)
__global__ void __launch_bounds__(256) best_compact(const float* __restrict__ g, long long n, long long ntiles, const unsigned* __restrict__ lmax,
                                                    unsigned lo_key, unsigned long long hi_key, BestCand* list, unsigned cap,
                                                    BestCounters* cnt) {
    visit_maxima(g, n, ntiles, lmax, lo_key, hi_key, [&](long long i, long long pe, float x, unsigned) {
        const unsigned slot = atomicAdd(&cnt->nlist, 1u);
        if (slot < cap) { list[slot].ps = i; list[slot].pe = pe; list[slot].h = x; list[slot].prom = 0.0f; }
    });
}

// Step 4: the prominence of candidates [from, to), one wavefront each, inside the finite stretch that holds the
// candidate (trans: the sorted transitions, ntrans of them).  A candidate below min_prom gets NaN (failed_prom of
// am_peaks.hip): it still takes part in the distance filter under peak_filter_order 1.
__global__ void __launch_bounds__(256) best_prom(const float* __restrict__ g, long long n, const float2* __restrict__ stats,
                                                 const long long* __restrict__ trans, int ntrans, BestCand* list, long long from,
                                                 long long to, float min_prom) {
    const int lane = threadIdx.x & 63;
    const long long q = from + (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (q >= to) return;
    const BestCand cd = list[q];
    // stretch: a = the last transition <= ps (or 0), b = the first one after it (or n)
    int lo = 0, hi = ntrans;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (trans[mid] <= cd.ps) lo = mid + 1; else hi = mid;
    }
    const long long a = lo > 0 ? trans[lo - 1] : 0, b = lo < ntrans ? trans[lo] : n;
    const SparseScores dense{nullptr, nullptr, nullptr, 1, 5, 5, 1.0};
    float prom = 0.0f;
    const bool keep = prominence(g, stats, dense, a, b, cd.ps, cd.pe, cd.h, min_prom, lane, prom);
    if (lane == 0) list[q].prom = keep ? prom : __uint_as_float(0x7FC00000u);
}

// ---------------------------------------------------------------------------
// host side
namespace {

struct BestBufs {
    unsigned* hist;      // kBestBins
    unsigned* hist2;     // kBestBins
    BestCounters* cnt;
};

BestBufs best_bufs(Ctx* c) {
    char* p = static_cast<char*>(c->best_ctl.p);
    return BestBufs{reinterpret_cast<unsigned*>(p), reinterpret_cast<unsigned*>(p + 4 * kBestBins),
                    reinterpret_cast<BestCounters*>(p + 8 * kBestBins)};
}
constexpr size_t kBestCtlBytes = 8 * kBestBins + sizeof(BestCounters);

int grid_for(long long waves_wanted) {
    const long long blocks = (waves_wanted + 3) / 4;
    return (int)std::max<long long>(1, std::min<long long>(blocks, kBestScanBlocks));
}

// The sorted transitions of x[0, n) (see BestScan).  `s` holds the scan to run (mode 0 or 1) and its buffers; a list
// longer than kBestTransCap is made again by a listing pass.
int scan_with_transitions(Ctx* c, BestScan s, std::vector<long long>& trans) {
    BestBufs bb = best_bufs(c);
    AM_HIP(hipMemsetAsync(c->best_ctl.p, 0, kBestCtlBytes, c->stream));
    s.cnt = bb.cnt; s.hist = bb.hist; s.trans = (long long*)c->best_trans.p; s.trans_cap = kBestTransCap;
    const int grid = (int)std::max<long long>(1, std::min<long long>(s.ntiles, kBestScanBlocks));
    {
        ProfScope ps(c, KN_STATS, c->stream);
        hipLaunchKernelGGL(best_scan, dim3(grid), dim3(256), 0, c->stream, s);
        AM_HIP(hipGetLastError());
    }
    BestCounters cnt{};
    int rc;
    if ((rc = download(c, &cnt, bb.cnt, sizeof(cnt)))) return rc;
    trans.clear();
    if (cnt.ntrans == 0) return AM_OK;
    if (cnt.ntrans > kBestTransCap) {
        if ((rc = c->best_trans.ensure(sizeof(long long) * cnt.ntrans))) return rc;
        BestScan t = s;
        t.mode = 1; t.trans = (long long*)c->best_trans.p; t.trans_cap = cnt.ntrans;
        AM_HIP(hipMemsetAsync(&bb.cnt->ntrans, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(best_scan, dim3(grid), dim3(256), 0, c->stream, t);
        AM_HIP(hipGetLastError());
    }
    trans.resize(cnt.ntrans);
    if ((rc = download(c, trans.data(), c->best_trans.p, sizeof(long long) * cnt.ntrans))) return rc;
    std::sort(trans.begin(), trans.end());
    return AM_OK;
}

}  // namespace

// The non-finite runs of x[0, n) as sorted transitions (BestScan): [t0, t1), [t2, t3), ...  Synchronous.
int best_transitions(Ctx* c, const float* d_x, long long n, std::vector<long long>& trans) {
    int rc;
    if ((rc = c->best_ctl.ensure(kBestCtlBytes))) return rc;
    if ((rc = c->best_trans.ensure(sizeof(long long) * kBestTransCap))) return rc;
    BestScan s{};
    s.g = d_x; s.n = n; s.ntiles = (n + kTile - 1) / kTile;
    s.mode = 1;
    return scan_with_transitions(c, s, trans);
}

// The k best peaks of the resident score array d_g[0, n) (include/audiomatch.h, am_find_peaks_top).  Synchronous.
int best_select(Ctx* c, const float* d_g, long long n, float min_prom, long long min_dist, size_t k, const PeakPolicy& pol,
                std::vector<am_peak>& res) {
    res.clear();
    if (n < 3 || k == 0) return AM_OK;
    int rc;
    const long long ntiles = (n + kTile - 1) / kTile;
    if ((rc = c->best_ctl.ensure(kBestCtlBytes))) return rc;
    if ((rc = c->best_trans.ensure(sizeof(long long) * kBestTransCap))) return rc;
    if ((rc = c->best_stats.ensure(sizeof(float2) * (size_t)ntiles))) return rc;
    if ((rc = c->best_lmax.ensure(sizeof(unsigned) * (size_t)ntiles))) return rc;
    const BestBufs bb = best_bufs(c);
    // 1. the scan
    BestScan s{};
    s.g = d_g; s.n = n; s.ntiles = ntiles; s.stats = (float2*)c->best_stats.p; s.lmax = (unsigned*)c->best_lmax.p; s.mode = 0;
    std::vector<long long> trans;
    if ((rc = scan_with_transitions(c, s, trans))) return rc;
    const bool finite = trans.empty();
    std::vector<unsigned> hist(kBestBins), hist2(kBestBins);
    BestCounters cnt{};
    AM_HIP(hipMemcpyAsync(hist.data(), bb.hist, 4 * kBestBins, hipMemcpyDeviceToHost, c->stream));
    if ((rc = download(c, &cnt, bb.cnt, sizeof(cnt)))) return rc;
    const long long total = (long long)cnt.nmax;
    if (total == 0) return AM_OK;
    if (!finite) {   // (sorted, for the walks' binary search)
        AM_HIP(hipMemcpyAsync(c->best_trans.p, trans.data(), sizeof(long long) * trans.size(), hipMemcpyHostToDevice, c->stream));
    }
    long long refined_bin = -1;
    // tau for M candidates: (key, count of maxima with key >= tau)
    auto pick = [&](long long M, unsigned* tau, long long* count) -> int {
        long long cum = 0;
        for (int b = kBestBins - 1; b >= 0; --b) {
            if (cum + hist[b] < M) { cum += hist[b]; continue; }
            if (cum + hist[b] > 8 * M && hist[b] > 1 && refined_bin != b) {   // a crowded bin: split it
                AM_HIP(hipMemsetAsync(bb.hist2, 0, 4 * kBestBins, c->stream));
                hipLaunchKernelGGL(best_refine, dim3(grid_for(ntiles)), dim3(256), 0, c->stream, d_g, n, ntiles,
                                   (const unsigned*)c->best_lmax.p, (unsigned)b, bb.hist2);
                AM_HIP(hipGetLastError());
                if ((rc = download(c, hist2.data(), bb.hist2, 4 * kBestBins))) return rc;
                refined_bin = b;
            }
            if (refined_bin == b) {
                for (int q = kBestBins - 1; q >= 0; --q) {
                    cum += hist2[q];
                    if (cum >= M || q == 0) { *tau = ((unsigned)b << 20) | ((unsigned)q << 8); *count = cum; return AM_OK; }
                }
            }
            *tau = (unsigned)b << 20; *count = cum + hist[b];
            return AM_OK;
        }
        *tau = 0u; *count = cum;
        return AM_OK;
    };
    // the listed candidates, in find_peaks' filter order (all of a later round lie below all of an earlier one)
    std::vector<BestCand> cands;
    unsigned long long hi_key = 1ull << 32;
    long long M = std::max<long long>(8 * (long long)std::min<size_t>(k, (size_t)1 << 40), 4096), listed = 0;
    for (;;) {
        unsigned tau = 0;
        long long count = 0;
        if ((rc = pick(M, &tau, &count))) return rc;
        if (count > kBestCap && finite) {
            // more candidates than the selection is for (k beyond what min_distance allows): the whole-array pick
            std::vector<am_peak> all;
            if ((rc = find_peaks_host_array(c, d_g, n, min_prom, min_dist, all))) return rc;
            if (all.size() > k) all.resize(k);
            res.swap(all);
            return AM_OK;
        }
        const long long fresh = count - listed;
        if (fresh > 0) {
            // 3. compact, 4. prominence
            if ((rc = c->best_list.ensure(sizeof(BestCand) * (size_t)fresh))) return rc;
            AM_HIP(hipMemsetAsync(&bb.cnt->nlist, 0, sizeof(unsigned), c->stream));
            {
                ProfScope ps(c, KN_PEAKS, c->stream);
                hipLaunchKernelGGL(best_compact, dim3(grid_for(ntiles)), dim3(256), 0, c->stream, d_g, n, ntiles,
                                   (const unsigned*)c->best_lmax.p, tau, hi_key, (BestCand*)c->best_list.p, (unsigned)fresh, bb.cnt);
                AM_HIP(hipGetLastError());
                hipLaunchKernelGGL(best_prom, dim3((unsigned)((fresh + 3) / 4)), dim3(256), 0, c->stream, d_g, n,
                                   (const float2*)c->best_stats.p, (const long long*)c->best_trans.p, (int)trans.size(),
                                   (BestCand*)c->best_list.p, 0ll, fresh, min_prom);
                AM_HIP(hipGetLastError());
            }
            unsigned got = 0;
            AM_HIP(hipMemcpyAsync(&got, &bb.cnt->nlist, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            const size_t old = cands.size();
            cands.resize(old + (size_t)fresh);
            if ((rc = download(c, cands.data() + old, c->best_list.p, sizeof(BestCand) * (size_t)fresh))) return rc;
            if ((long long)got != fresh) return fail(AM_ERR_PEAK_OVERFLOW, "k-best selection: candidate list does not match its histogram");
            std::sort(cands.begin() + old, cands.end(), [](const BestCand& x, const BestCand& y) {
                return x.h > y.h || (x.h == y.h && x.ps < y.ps);
            });
            listed = count;
        }
        // 5. filter (from the start: cheap next to the device passes)
        res.clear();
        std::set<long long> kept_pos;
        for (const BestCand& cd : cands) {
            const bool passed = cd.prom == cd.prom;   // (NaN: failed min_prominence)
            if (!passed && !pol.order) continue;
            am_peak pk{(uint64_t)cd.ps, (uint64_t)cd.pe, cd.h, cd.prom};
            const long long pos = pol.from_start ? cd.ps : (long long)(((uint64_t)cd.ps + (uint64_t)cd.pe) / 2);
            if (min_dist > 0) {
                auto it = kept_pos.lower_bound(pos);
                long long d = LLONG_MAX;
                if (it != kept_pos.end()) d = std::min(d, *it - pos);
                if (it != kept_pos.begin()) d = std::min(d, pos - *std::prev(it));
                if (pol.inclusive ? d <= min_dist : d < min_dist) continue;
                kept_pos.insert(pos);
            }
            if (!passed) continue;
            res.push_back(pk);
            if (res.size() == k) return AM_OK;
        }
        // 6. descent
        if (listed >= total || tau == 0u) return AM_OK;
        hi_key = tau;
        M = std::max(8 * M, listed + 1);
    }
}

// The AM_MODE_VALID scores of samples x[0, w) into d_out[0, w - S + 1), as correlate_impl (am_api.hip) computes them
// for a finite input: the same run_correlation, the same half-precision redo check, normalise_scores under score_norm.
int valid_scores(am_needle* h, const Opts& o0, const NormSpec& nrm, float factor, const float* d_x, long long w, float* d_out) {
    Ctx* c = h->ctx;
    const long long s = (long long)h->n, len = w - s + 1;
    Opts o = o0;
    int rc;
    if ((rc = run_correlation(h, o, d_x, w, 0, d_out, len, factor))) return rc;
    if (o.half) {
        const Segment whole{0, len};
        int flag = 0;
        if ((rc = nonfinite_flags(c, d_out, &whole, 1, &flag))) return rc;
        if (flag) {
            o.half = 0;
            if ((rc = run_correlation(h, o, d_x, w, 0, d_out, len, factor))) return rc;
        }
    }
    if (nrm.on && (rc = normalise_scores(c, c->stream, nrm, d_x, w, 0, 0, s, d_out, 0, len))) return rc;
    return AM_OK;
}

// The samples a haystack is correlated as (am_internal.h): the bit-exact down-mix of an i16 stereo haystack into `mono`,
// and the non-finite runs of the samples (one grid-wide pass: best_scan's transition mode); usually there are none.
// Synchronous.
int haystack_prepare(Ctx* c, const void* d_hay, size_t len, int sample_format, DevBuf& mono, HaySamples* hs) {
    int rc;
    const float* d_x = static_cast<const float*>(d_hay);
    if (sample_format == AM_FMT_S16_STEREO) {
        if ((rc = mono.ensure(len * sizeof(float)))) return rc;
        AM_HIP(launch_pcm_downmix(c->stream, static_cast<const int16_t*>(d_hay), (long long)len, (float*)mono.p));
        d_x = (const float*)mono.p;
    }
    hs->d_x = d_x;
    hs->len = len;
    return best_transitions(c, d_x, (long long)len, hs->trans);
}

// The Valid scores of prepared samples (len >= S) into the context's best_scores.  Synchronous.
int prepared_scores(am_needle* h, const Opts& o, const HaySamples& hs, int scale, const float** d_scores, long long* n_scores) {
    Ctx* c = h->ctx;
    const size_t s = h->n, len = hs.len;
    int rc;
    const NormSpec nrm = norm_spec(h, o);
    const float factor = nrm.on ? norm_factor(nrm) : scale_factor(h, scale, len);
    const float* d_x = hs.d_x;
    const std::vector<long long>& t = hs.trans;
    const long long n = (long long)(len - s + 1);
    if ((rc = c->best_scores.ensure(sizeof(float) * (size_t)n))) return rc;
    float* d_sc = (float*)c->best_scores.p;
    if (t.empty()) {
        if ((rc = valid_scores(h, o, nrm, factor, d_x, (long long)len, d_sc))) return rc;
    } else {
        // a window that holds a non-finite sample has no score; every finite stretch of at least S samples is
        // correlated on its own
        AM_HIP(hipMemsetD32Async((hipDeviceptr_t)d_sc, 0x7FC00000, (size_t)n, c->stream));
        long long p = 0;
        for (size_t i = 0; i <= t.size(); i += 2) {
            const long long q = i < t.size() ? t[i] : (long long)len;   // finite stretch [p, q)
            if (q - p >= (long long)s && (rc = valid_scores(h, o, nrm, factor, d_x + p, q - p, d_sc + p))) return rc;
            if (i + 1 < t.size()) p = t[i + 1];
        }
    }
    *d_scores = d_sc;
    *n_scores = n;
    return AM_OK;
}

// The score array of one resident haystack (am_internal.h): what am_match_best selects from and am_match_trace reduces.
// The caller holds the context's lock and has checked the arguments (len >= S).  Synchronous.
int haystack_scores(am_needle* h, const Opts& o, const void* d_hay, size_t len, int sample_format, int scale, const float** d_scores,
                    long long* n_scores) {
    HaySamples hs;
    int rc;
    if ((rc = haystack_prepare(h->ctx, d_hay, len, sample_format, h->ctx->best_mono, &hs))) return rc;
    return prepared_scores(h, o, hs, scale, d_scores, n_scores);
}

// am_match_best on one resident haystack (include/audiomatch.h): its Valid scores (haystack_scores), then best_select.
// The caller holds the context's lock and has checked the arguments.  Synchronous.
int match_best_one(am_needle* h, const void* d_hay, size_t len, int sample_format, const am_best_params* bp, am_peak* out,
                   size_t* n_out) {
    Ctx* c = h->ctx;
    *n_out = 0;
    if (len < h->n) return AM_OK;
    int rc;
    const Opts o = snapshot_opts(h);
    const float* d_sc = nullptr;
    long long n = 0;
    if ((rc = haystack_scores(h, o, d_hay, len, sample_format, bp->scale, &d_sc, &n))) return rc;
    std::vector<am_peak> res;
    if ((rc = best_select(c, d_sc, n, bp->min_prominence, (long long)std::min<uint64_t>(bp->min_distance, (uint64_t)LLONG_MAX),
                          (size_t)bp->k, o.peak_policy(), res))) return rc;
    for (size_t i = 0; i < res.size(); ++i) out[i] = res[i];
    *n_out = res.size();
    return AM_OK;
}

}  // namespace am
