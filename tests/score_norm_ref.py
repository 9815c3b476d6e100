"""The f64 checker of window-energy normalised scores (option "score_norm", NCC) and the designed signals of its tests.

ncc(t) = corr(t) / sqrt(sum(needle^2) * E(t)),  E(t) = sum of x_i^2 over the window [t - lead, t - lead + s), x = 0 outside.

Two designs (test_gpu_score_norm_edges.py runs them on the device, test_score_norm_design_host.py checks the designs):
  spike_case   a positive needle against zeros with integer spikes: every window energy is a small integer, exact in
               f64 on both sides, and the spikes sit on every edge am_norm.hip's index arithmetic knows of
  plant_case   planted copies of a needle with guard spikes of the copy's energy directly outside or inside the window
"""
import numpy as np

SR = 8000
MODE_FULL, MODE_SAME, MODE_VALID = 0, 1, 2   # am_mode (include/audiomatch.h)
NORM_BLOCK, NORM_TILE = 1024, 2048           # kNormBlock, kNormTile (csrc/am_kernels.h)
U = 2.0 ** -24                               # unit roundoff of f32


# ---- the checker ---------------------------------------------------------------------------------------------------
def ncc_ref(oracle, within, needle, mode, floor_db=60):
    """Level 1: NCC of every output of `mode`, zero padding as the correlation's."""
    w, s = len(within), len(needle)
    x = np.asarray(within, dtype=np.float32)
    xc = np.where(np.isfinite(x), x, 0).astype(np.float32)
    raw = oracle.correlate(xc, needle, mode, oracle.SCALE_NONE, prec=oracle.PREC_F64).astype(np.float64)
    n = len(raw)
    full = w + s - 1
    lead = (s - 1) - (full - n) // 2
    x2 = np.concatenate([np.zeros(max(lead, 0)), xc.astype(np.float64) ** 2, np.zeros(s + n)])
    c = np.concatenate([[0.0], np.cumsum(x2)])
    t = np.arange(n) + (max(lead, 0) - lead)
    ew = c[t + s] - c[t]
    en = float(np.sum(np.asarray(needle, dtype=np.float64) ** 2))
    thr = en * 10.0 ** (-floor_db / 10.0)
    ok = ew >= thr
    out = np.zeros(n)
    out[ok] = raw[ok] / np.sqrt(en * ew[ok])
    return out, ew, thr


def chunks(length, s, chunk, overlap, tail_window=0):
    window = chunk + overlap
    off = 0
    while off < length:
        w = min(window, length - off)
        if w >= s and not (tail_window and w < window):
            yield off, w
        off += chunk


def overshadow_filter(oracle, peaks, sr, dist_s):
    peaks = sorted(peaks, key=lambda q: q[0])
    out = []
    for i, q in enumerate(peaks):
        before = peaks[i - 1] if i > 0 else None
        after = peaks[i + 1] if i + 1 < len(peaks) else None
        if oracle.is_overshadowed(q, before, sr, dist_s) or oracle.is_overshadowed(q, after, sr, dist_s):
            continue
        out.append(q)
    return out


def match_ref(oracle, hay, needle, p, floor_db=60, tail_window=0, only=None):
    """Level 2: per chunk as calc_chunks, on NCC scores; chunks whose window holds a non-finite sample are dropped.
    only: restrict the check to chunks whose offset is in this set (the rest are assumed peak-free)."""
    s = len(needle)
    bad = np.flatnonzero(~np.isfinite(hay))
    peaks = []
    for off, w in chunks(len(hay), s, p.chunk, p.overlap, tail_window):
        if only is not None and off not in only:
            continue
        if np.any((bad >= off) & (bad < off + w)):
            continue
        y, _, _ = ncc_ref(oracle, hay[off:off + w], needle, oracle.MODE_VALID, floor_db)
        for a, b, h, pr in oracle.find_peaks(y.astype(np.float32), p.min_prominence, p.min_distance):
            peaks.append((a + off, b + off, h, pr))
    return overshadow_filter(oracle, peaks, p.sr, p.overshadow_distance_s)


def assert_peaks(got, exp, tol=1e-4):
    assert [(g.start, g.end) for g in got] == [(e[0], e[1]) for e in exp], (got, exp)
    for g, e in zip(got, exp):
        assert abs(g.height - e[2]) <= tol and abs(g.prominence - e[3]) <= tol, (g, e)


def bits(peaks):
    return [(q.start, q.end, np.float32(q.height).tobytes(), np.float32(q.prominence).tobytes()) for q in peaks]


# ---- window energies -----------------------------------------------------------------------------------------------
def mode_len(w, s, mode):
    """Outputs of a correlation of w samples with an s-sample needle (mode_len of csrc/am_api.hip)."""
    if mode == MODE_FULL:
        return w + s - 1
    if mode == MODE_SAME:
        return w
    return max(w - s, 0) + 1


def lead_of(w, s, mode):
    """Score t of `mode` has the window [t - lead, t - lead + s): centered() of the full correlation (correlate_impl,
    csrc/am_api.hip: start = (full - len) / 2, lead = (s - 1) - start)."""
    start = (w + s - 1 - mode_len(w, s, mode)) // 2
    return (s - 1) - start


def window_energy(x, s, lead, n):
    """E(t) = sum of x[i]^2 over [t - lead, t - lead + s) for t in [0, n), zero outside the signal: f64, from one
    cumulative sum (exact where every x[i]^2 is a small integer)."""
    w = len(x)
    c = np.concatenate([[0.0], np.cumsum(np.asarray(x, dtype=np.float64) ** 2)])
    lo = np.arange(n, dtype=np.int64) - lead
    return c[np.clip(lo + s, 0, w)] - c[np.clip(lo, 0, w)]


# ---- design 1: integer spikes on every edge ------------------------------------------------------------------------
# 4095 / 4096 / 4097 sit on the switch between the direct and the assembled path (kNormTile + 2 kNormBlock = 4096);
# 300 is not an edge: it is the one needle that takes the transform and the direct path's scan and still fits between
# two block-edge spike groups (which lie 1022 zeros apart) with room to spare, so that the scan sees windows of exact
# zeros next to windows that hold a spike.
SPIKE_S = (1, 2, 300, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5121, 8193)
SPIKE_MODES = (MODE_FULL, MODE_SAME, MODE_VALID)
MAX_ZERO_RUN = NORM_BLOCK - 2   # zeros between the spikes at 1024 k + 1 and 1024 (k + 1) - 1
# The device test's bound on the relative error of a recovered window energy (its docstring counts the roundings),
# and the smallest relative change of a window energy that a one-sample defect must cause (the design test asserts it).
ENERGY_BOUND = 16 * U
MIN_DEFECT = 1e-3


def spike_widths(s):
    """Signal lengths for needle length s: Valid-mode score counts 1, 2047, 2048, 2049, 3 * 2048, 3 * 2048 + 1 (one
    score, one tile -1 / 0 / +1, whole tiles, one score into a fourth), and one length each that is 1 and 1023 above
    a multiple of 1024 (a last block of one sample, and of all but one)."""
    ws = [s + c - 1 for c in (1, NORM_TILE - 1, NORM_TILE, NORM_TILE + 1, 3 * NORM_TILE, 3 * NORM_TILE + 1)]
    base = ((s + 3000) // NORM_BLOCK + 1) * NORM_BLOCK
    return ws + [base + 1, base + NORM_BLOCK - 1]


def spike_cases():
    return [(s, w, mode) for s in SPIKE_S for w in spike_widths(s) for mode in SPIKE_MODES]


def spike_needle(s, seed=0):
    """f32, uniform in [0.25, 1]: every product with a spike is positive."""
    return np.random.default_rng([seed, s]).uniform(0.25, 1.0, s).astype(np.float32)


def spike_signal(s, w, mode, seed=0):
    """within of spike_case: a signal that is exactly 0.0 except for spikes of amplitude 1, 2 or 3
    on the signal's ends, on every 1024-sample block edge and its two neighbours (where the whole-block range [A, Z)
    starts and ends), on the first and last sample of the first and last window of every 2048-score tile, each with
    its two neighbours, and on about w / 700 random samples."""
    lead, n = lead_of(w, s, mode), mode_len(w, s, mode)
    rng = np.random.default_rng([seed, s, w, mode])
    pos = [0, w - 1]
    for m in range(0, w + NORM_BLOCK, NORM_BLOCK):
        pos += [m - 1, m, m + 1]
    for t0 in range(0, n, NORM_TILE):
        for first in (t0 - lead, t0 + NORM_TILE - 1 - lead):
            for edge in (first, first + s - 1):
                pos += [edge - 1, edge, edge + 1]
    pos += list(rng.integers(0, w, size=max(1, round(w / 700))))
    pos = np.unique(np.array([q for q in pos if 0 <= q < w], dtype=np.int64))
    within = np.zeros(w, dtype=np.float32)
    within[pos] = rng.integers(1, 4, size=len(pos)).astype(np.float32)
    return within


def spike_case(s, w, mode, seed=0):
    """(needle, within): the positive needle of length s (one per s and seed) and spike_signal."""
    return spike_needle(s, seed), spike_signal(s, w, mode, seed)


GAP_LO, GAP_EXTRA = 1500, 2700


def gap_signal(s, mode, seed=0):
    """A spike signal with the samples [GAP_LO, GAP_LO + s + GAP_EXTRA) cleared and a spike directly in
    front of and behind them.  The block-edge spikes leave no empty window to a needle of 1023 samples or more; here
    every needle, the assembled path's included, has GAP_EXTRA + 1 windows of exact zeros in a row, over a tile edge
    of the score array, and the windows next to them hold one spike on their first or last sample."""
    w = GAP_LO + s + GAP_EXTRA + NORM_TILE + 1
    within = spike_signal(s, w, mode, seed)
    lo, hi = GAP_LO, GAP_LO + s + GAP_EXTRA
    within[lo:hi] = 0.0
    within[lo - 1] = within[hi] = 2.0
    return within


def gap_case(s, mode, seed=0):
    return spike_needle(s, seed), gap_signal(s, mode, seed)


def zero_windows_expected(s, n):
    """Whether a spike case has windows of energy exactly 0 (directly beside windows that hold a spike).  The spikes on
    the signal's ends and on every block edge leave runs of at most 1022 zeros, and a window of Full or Same mode that
    reaches over an end of the signal holds that end's spike: a window of 1023 samples or more is never empty, in any
    mode.  A shorter one is, somewhere, as soon as the scores fill a tile."""
    return s <= MAX_ZERO_RUN and n >= NORM_TILE


def sparse_corr(needle, within, lead, n):
    """corr(t) = sum_j within[t - lead + j] needle[j] in f64, summed spike by spike."""
    s = len(needle)
    nd = np.asarray(needle, dtype=np.float64)
    out = np.zeros(n)
    for q in np.flatnonzero(within):
        t = q + lead - np.arange(s)           # the scores whose window holds sample q, at needle index j
        ok = (t >= 0) & (t < n)
        out[t[ok]] += float(within[q]) * nd[ok]
    return out


def energy_variants(x, s, lead, n):
    """The window energy with one sample too few or too many: first sample dropped, last sample dropped, one more in
    front, one more behind."""
    return [window_energy(x, s - 1, lead - 1, n), window_energy(x, s - 1, lead, n),
            window_energy(x, s + 1, lead + 1, n), window_energy(x, s + 1, lead, n)]


def scale_pair(en):
    """(a, b): the f32 factors of a LIB-scaled and of a score_norm correlation for a needle of f64 energy en
    (inv_autocorr of am_needle_create, norm_factor of csrc/am_norm.hip)."""
    return np.float32(1.0 / en), np.float32(1.0 / np.sqrt(en))


def recovered_energy(lib, ncc, a, b):
    """E(t) from lib = fl(v a) and ncc = fl(fl(v b) / sqrt(E)) of the same f32 correlation value v:
    E = (lib / ncc)^2 (b / a)^2, in f64; six f32 roundings (three per factor, squared)."""
    lib, ncc = np.asarray(lib, dtype=np.float64), np.asarray(ncc, dtype=np.float64)
    return (lib / ncc) ** 2 * (float(b) / float(a)) ** 2


def simulate_pair(corr, E, en):
    """What the two correlations return for the f64 correlation values `corr` and window energies E > 0, with the
    library's roundings: v = fl(corr), lib = fl(v a), ncc = fl(fl(v b) / sqrt(E)) (the division in f64, rounded once)."""
    a, b = scale_pair(en)
    v = np.asarray(corr, dtype=np.float64).astype(np.float32)
    lib = v * a
    raw = v * b
    ncc = (raw.astype(np.float64) / np.sqrt(E)).astype(np.float32)
    return lib, ncc, a, b


# ---- design 2: plants with guard spikes ----------------------------------------------------------------------------
PLANT_S = (2000, 8000)      # the direct and the assembled path
PLANT_LEN = 90 * SR + 123
PLANT_PROMINENCE = 0.4      # between the noise's peaks (NCC about 1 / sqrt(S), prominences up to 0.25 at S = 2000)
                            # and the lowest plant (inside guards: 0.58)


def plant_offsets(S, length=PLANT_LEN, chunk=20 * SR):
    """Plants (t, kind), 9 s apart or more.  The inner ones (inner_plants) are the hits that get compared: t mod 2048
    in {0, 1, 2047}, (t + S) mod 1024 in {0, 1, 1023}, one just below a chunk start (found in the previous chunk's
    overlap).  The plants at t = 0 and t = length - S sit on the first and the last score, which are never peaks: all
    they check is that the library agrees on "no hit" there (plant_setup's sliced haystacks put hits next to an end).
    kind "out": guards at t - 1 and t + S; "in": guards at t and t + S - 1."""
    def tile(base, r):
        return base // NORM_TILE * NORM_TILE + r

    def block_end(base, r):
        return (base + S) // NORM_BLOCK * NORM_BLOCK + r - S

    return [(0, "out"), (tile(10 * SR, 1), "in"), (tile(20 * SR, 0), "out"), (tile(30 * SR, NORM_TILE - 1), "out"),
            (2 * chunk - 3, "in"), (block_end(50 * SR, 0), "out"), (block_end(60 * SR, 1), "in"),
            (block_end(70 * SR, NORM_BLOCK - 1), "out"), (length - S, "in")]


def inner_plants(S, length=PLANT_LEN):
    return [(t, kind) for t, kind in plant_offsets(S, length) if 0 < t < length - S]


def plant_case(oracle, S, length=PLANT_LEN):
    """(needle, hay, plants): a uniform needle of amplitude 0.25, `length` samples of uniform noise of amplitude 1e-3
    and the plants of plant_offsets, each with two guard spikes of the needle's energy: outside the window the correct
    NCC is about 1 (and about 0.71 from a window one sample too wide), inside it is about 0.58 (0.71 from a window one
    sample too narrow)."""
    needle = oracle.synth_uniform(11, 1, 0, S, 0.25).astype(np.float32)
    hay = oracle.synth_uniform(11, 3, 0, length, 1e-3).astype(np.float32)
    g = np.float32(np.sqrt(np.sum(needle.astype(np.float64) ** 2)))
    plants = plant_offsets(S, length)
    for t, kind in plants:
        hay[t:t + S] += needle
        for q in ((t - 1, t + S) if kind == "out" else (t, t + S - 1)):
            if 0 <= q < length:
                hay[q] += g
    return needle, hay, plants


def plant_params(am, S):
    """am: the audiomatch_amd module.  Chunks of 20 s, overlap = the needle, 5 s distance."""
    return am.Config(chunk_size_s=20.0, overlap_length_s=S / SR, distance_s=5.0, prominence=PLANT_PROMINENCE).params(SR, am.Scale.LIB)


_plant_cache = {}


def plant_setup(am, oracle, S):
    """(needle, hays, exps, plants, p): the case of needle length S, its three haystacks, the checker's peaks of each,
    the inner plants and the match parameters; computed once per session and shared, never written to.  The second
    haystack ends one sample behind a plant and the third starts one sample in front of one: hits on the last but one
    and on the second score, the nearest to an end that a peak can be."""
    if S not in _plant_cache:
        needle, hay, _ = plant_case(oracle, S)
        p = plant_params(am, S)
        assert p.chunk == 20 * SR and p.overlap == S
        cut = 2 * p.chunk - 3                     # the plant just below a chunk start
        assert (cut, "in") in inner_plants(S)
        hays = [hay, hay[:cut + S + 1], hay[cut - 1:]]
        exps = [match_ref(oracle, h, needle, p) for h in hays]
        for h in hays:
            h.setflags(write=False)
        _plant_cache[S] = (needle, hays, exps, inner_plants(S), p)
    return _plant_cache[S]


def stereo(x):
    """Interleaved i16 stereo frames of a float signal, full scale at its largest sample; the right channel at three
    quarters of the left, so that the down-mix is no copy of either."""
    k = 32000.0 / float(np.max(np.abs(x)))
    left = np.round(np.asarray(x, dtype=np.float64) * k)
    return np.ascontiguousarray(np.stack([left, np.round(0.75 * left)], axis=1).astype(np.int16))
