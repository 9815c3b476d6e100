// am_walk.h -- the prominence walk of the peak pick (am_peaks.hip), shared with the k-best selection
// (am_best.hip): wave reductions, the sparse-score view and the wave-cooperative walk over tile summaries.
// Device code only; included inside namespace am.
#pragma once

constexpr int kGroup = 8;         // tiles per lane in the coarse step of a prominence walk

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= FLT_MAX); }

// K3 writes raw scores only for the 32-score runs that can matter (am_fft.hip, k3_finish);
// everywhere else only the per-32 summary exists.  The flags are the ballots of K3's wavefronts.
__device__ __forceinline__ bool run_written(const SparseScores& sp, long long idx) {
    if (sp.wbits == nullptr) return true;
    // idx / hop through one f64 multiply and a fix-up (idx < 2^50)
    long long blk = (long long)((double)idx * sp.inv_hop);
    long long rem = idx - blk * sp.hop;
    if (rem < 0) { rem += sp.hop; --blk; }
    else if (rem >= sp.hop) { rem -= sp.hop; ++blk; }
    const unsigned n = (unsigned)rem;
    const unsigned row = n >> sp.log_n2, tile = (n & ((1u << sp.log_n2) - 1u)) >> kColsLog;
    const int hb = sp.log_n1 - 4;                              // rows per register index a of a column owner
    const unsigned wave = (row >> 2) & ((1u << (hb - 2)) - 1u), bit = ((row >> hb) << 2) | (row & 3u);
    const long long word = (((blk << (sp.log_n2 - kColsLog)) + tile) << (hb - 2)) + wave;
    return (sp.wbits[word] >> bit) & 1ull;
}
// for minima: exact where written, else the run's minimum (exact whenever the
// whole run lies in the range being reduced, a lower bound otherwise)
__device__ __forceinline__ float score_for_min(const float* __restrict__ g, const SparseScores& sp, long long idx) {
    return run_written(sp, idx) ? g[idx] : sp.stats32[idx >> 5].x;
}
// for comparisons with a candidate height: an unwritten score lies below the write threshold of its
// tile, which the chunk's certificate (peaks_kernel) has shown to be below every candidate height
__device__ __forceinline__ float score_for_cmp(const float* __restrict__ g, const SparseScores& sp, long long idx) {
    return run_written(sp, idx) ? g[idx] : -FLT_MAX;
}

// One wave-cooperative step of the walk to the left of `cur` (exclusive) down
// to `a`: either skips up to 64 whole tiles through their summaries or looks at
// up to 64 raw samples.  Returns true when a strictly higher sample ended the
// walk; `cur` reaching `a` ends it at the chunk edge.
__device__ __forceinline__ bool step_left(const float* __restrict__ g, const float2* __restrict__ stats,
                                          const SparseScores& sp,
                                          long long a, long long& cur, float h, float& vmin, int lane) {
    // coarse skip: every lane summarises a group of kGroup tiles (64 groups per step)
    if ((cur % kTile) == 0 && cur - (long long)kGroup * kTile >= a) {
        const long long t1 = cur / kTile - (long long)kGroup * lane;      // group = tiles [t1 - kGroup, t1)
        const bool valid = (t1 - kGroup) * (long long)kTile >= a;
        float gmn = FLT_MAX, gmx = -FLT_MAX;
        if (valid) {
#pragma unroll
            for (int k = 1; k <= kGroup; ++k) { const float2 st = stats[t1 - k]; gmn = fminf(gmn, st.x); gmx = fmaxf(gmx, st.y); }
        }
        const unsigned long long blocked = __ballot(valid && gmx > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? gmn : FLT_MAX));
            cur -= (long long)nskip * kGroup * kTile;
            return false;
        }
    }
    if ((cur % kTile) == 0 && cur - kTile >= a) {
        const long long t = cur / kTile - 1 - lane;
        const bool valid = t >= 0 && t * (long long)kTile >= a;
        float2 st = make_float2(FLT_MAX, -FLT_MAX);
        if (valid) st = stats[t];
        const unsigned long long blocked = __ballot(valid && st.y > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? st.x : FLT_MAX));
            cur -= (long long)nskip * kTile;
            return false;
        }
    }
    const long long tile_lo = ((cur - 1) / kTile) * kTile;
    const long long lo = tile_lo > a ? tile_lo : a;
    // run-level skip through K3's exact (min,max) per 32 scores (stays inside the
    // current tile so that tile-level skipping resumes at its boundary)
    if (sp.stats32 != nullptr && (cur & 31) == 0 && cur - 32 >= lo) {
        const long long r = (cur >> 5) - 1 - lane;
        const bool valid = r * 32 >= lo;
        float2 st = make_float2(FLT_MAX, -FLT_MAX);
        if (valid) st = sp.stats32[r];
        const unsigned long long blocked = __ballot(valid && st.y > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? st.x : FLT_MAX));
            cur -= (long long)nskip * 32;
            return false;
        }
    }
    // A raw step stops at the start of the current 32-score run when run summaries
    // exist: the walk is then aligned for the run-level skip above (raw steps of 64
    // would keep the misalignment they started with all the way to the tile edge).
    const long long run_lo = (cur - 1) & ~31ll;
    const long long lo2 = (sp.stats32 != nullptr && run_lo > lo) ? run_lo : lo;
    const long long idx = cur - 1 - lane;
    const bool valid = idx >= lo2;
    const float v = valid ? score_for_min(g, sp, idx) : 0.0f;
    const unsigned long long higher = __ballot(valid && v > h);
    const int nval = __popcll(__ballot(valid));
    const int ntake = higher ? (__ffsll((long long)higher) - 1) : nval;
    vmin = fminf(vmin, wave_min(lane < ntake ? v : FLT_MAX));
    cur -= ntake;
    return higher != 0ull;
}

// Mirror image: walk to the right from `cur` (inclusive) up to `b` (exclusive).
__device__ __forceinline__ bool step_right(const float* __restrict__ g, const float2* __restrict__ stats,
                                           const SparseScores& sp,
                                           long long b, long long& cur, float h, float& vmin, int lane) {
    if ((cur % kTile) == 0 && cur + (long long)kGroup * kTile <= b) {
        const long long t0 = cur / kTile + (long long)kGroup * lane;      // group = tiles [t0, t0 + kGroup)
        const bool valid = (t0 + kGroup) * (long long)kTile <= b;
        float gmn = FLT_MAX, gmx = -FLT_MAX;
        if (valid) {
#pragma unroll
            for (int k = 0; k < kGroup; ++k) { const float2 st = stats[t0 + k]; gmn = fminf(gmn, st.x); gmx = fmaxf(gmx, st.y); }
        }
        const unsigned long long blocked = __ballot(valid && gmx > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? gmn : FLT_MAX));
            cur += (long long)nskip * kGroup * kTile;
            return false;
        }
    }
    if ((cur % kTile) == 0 && cur + kTile <= b) {
        const long long t = cur / kTile + lane;
        const bool valid = (t + 1) * (long long)kTile <= b;
        float2 st = make_float2(FLT_MAX, -FLT_MAX);
        if (valid) st = stats[t];
        const unsigned long long blocked = __ballot(valid && st.y > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? st.x : FLT_MAX));
            cur += (long long)nskip * kTile;
            return false;
        }
    }
    const long long tile_hi = (cur / kTile + 1) * kTile;
    const long long hi = tile_hi < b ? tile_hi : b;
    if (sp.stats32 != nullptr && (cur & 31) == 0 && cur + 32 <= hi) {
        const long long r = (cur >> 5) + lane;
        const bool valid = (r + 1) * 32 <= hi;
        float2 st = make_float2(FLT_MAX, -FLT_MAX);
        if (valid) st = sp.stats32[r];
        const unsigned long long blocked = __ballot(valid && st.y > h);
        const int nvalid = __popcll(__ballot(valid));
        const int nskip = blocked ? (__ffsll((long long)blocked) - 1) : nvalid;
        if (nskip > 0) {
            vmin = fminf(vmin, wave_min(lane < nskip ? st.x : FLT_MAX));
            cur += (long long)nskip * 32;
            return false;
        }
    }
    // as in step_left: end a raw step at the next run boundary when run summaries exist
    const long long run_hi = ((cur >> 5) + 1) << 5;
    const long long hi2 = (sp.stats32 != nullptr && run_hi < hi) ? run_hi : hi;
    const long long idx = cur + lane;
    const bool valid = idx < hi2;
    const float v = valid ? score_for_min(g, sp, idx) : 0.0f;
    const unsigned long long higher = __ballot(valid && v > h);
    const int nval = __popcll(__ballot(valid));
    const int ntake = higher ? (__ffsll((long long)higher) - 1) : nval;
    vmin = fminf(vmin, wave_min(lane < ntake ? v : FLT_MAX));
    cur += ntake;
    return higher != 0ull;
}

// Prominence of the flat-topped maximum [ps, pe) of height h inside chunk
// [a, b); both walks advance in lock step so that a side lobe next to a taller
// peak is rejected after a few samples (prominence <= h - min of a finished
// side).  Returns false when prominence < min_prom.
__device__ bool prominence(const float* __restrict__ g, const float2* __restrict__ stats,
                           const SparseScores& sp, long long a, long long b, long long ps, long long pe, float h,
                           float min_prom, int lane, float& prom) {
    long long cl = ps, cr = pe;
    float lmin = h, rmin = h;
    bool dl = cl <= a, dr = cr >= b;
    while (!dl || !dr) {
        if (!dl) {
            const bool stopped = step_left(g, stats, sp, a, cl, h, lmin, lane);
            dl = stopped || cl <= a;
            if (dl && !((h - lmin) >= min_prom)) return false;
        }
        if (!dr) {
            const bool stopped = step_right(g, stats, sp, b, cr, h, rmin, lane);
            dr = stopped || cr >= b;
            if (dr && !((h - rmin) >= min_prom)) return false;
        }
    }
    prom = h - fmaxf(lmin, rmin);
    return prom >= min_prom;
}
