"""The f64 checker of masked matching (am_needle_create_masked, include/audiomatch.h "masked needles") and the designed
signals of its tests.  A module, not a test file; the tests import it.

A masked needle has gaps [begin, end) to ignore; the kept spans [a_j, b_j) are what lies between them.
    mncc(t) = corr(t) / sqrt(E_n^M E_x^M(t)),   E_x^M(t) = sum_j sum_{i in [a_j, b_j)} x[t - lead + i]^2,  x = 0 outside
corr is the correlation with the needle whose gap samples are 0, E_n^M that needle's energy.

Two designs (test_gpu_mask_energies.py and test_gpu_mask_match.py run them on the device, test_mask_host.py holds them
to their own claims without one):
  mask_signal   integer spikes against zeros, one directly inside and one directly outside every edge of every kept span
                for the first and the last window of every tile of scores, on top of score_norm_ref's block-edge spikes
  plant_case    planted needles whose gap is overwritten by noise 20 dB above the needle
"""
import numpy as np

import score_norm_ref as ref

SR = ref.SR
MAX_GAPS = 15   # AM_MASK_MAX_GAPS


# ---- the mask -------------------------------------------------------------------------------------------------------
def kept_spans(n, gaps):
    """The spans between the gaps of an n-sample needle, ascending; every one non-empty."""
    edges = [0] + [q for g in gaps for q in g] + [n]
    return [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if b > a]


def gap_violation(n, gaps):
    """None, or which rule of include/audiomatch.h the gaps of an n-sample needle break (the library refuses these)."""
    if len(gaps) > MAX_GAPS:
        return "too many"
    for i, (b, e) in enumerate(gaps):
        if b >= e:
            return "empty"
        if e > n:
            return "behind the needle"
        if i and b < gaps[i - 1][1]:
            return "not ascending"
        if i and b == gaps[i - 1][1]:
            return "touching"
    if len(gaps) == 1 and tuple(gaps[0]) == (0, n):
        return "nothing kept"
    return None


def zero_filled(needle, gaps):
    """The handle's needle: gap samples set to +0."""
    out = np.array(needle, dtype=np.float32)
    for b, e in gaps:
        out[b:e] = 0.0
    return out


def masked_energy(x, kept, lead, n):
    """E_x^M(t) for t in [0, n): per kept span the window energy of a needle of its length whose windows start a_j
    samples further on, the spans added in ascending order (exact where every x[i]^2 is a small integer)."""
    E = np.zeros(n)
    for a, b in kept:
        E = E + ref.window_energy(x, b - a, lead - a, n)
    return E


def masked_energy_direct(x, kept, lead, n):
    """The same by the definition, sample by sample (for the host test)."""
    x2 = np.asarray(x, dtype=np.float64) ** 2
    E = np.zeros(n)
    for t in range(n):
        for a, b in kept:
            lo, hi = max(t - lead + a, 0), min(t - lead + b, len(x2))
            if hi > lo:
                E[t] += float(np.sum(x2[lo:hi]))
    return E


def mncc_ref(oracle, within, needle, gaps, mode, floor_db=60):
    """Masked NCC of every output of `mode`: (scores, E_x^M, floor).  Non-finite samples count as 0 (the caller drops
    the windows that hold them, as score_norm_ref.match_ref does)."""
    s = len(needle)
    x = np.asarray(within, dtype=np.float32)
    xc = np.where(np.isfinite(x), x, 0).astype(np.float32)
    nz = zero_filled(needle, gaps)
    raw = oracle.correlate(xc, nz, mode, oracle.SCALE_NONE, prec=oracle.PREC_F64).astype(np.float64)
    n = len(raw)
    lead = ref.lead_of(len(x), s, mode)
    assert n == ref.mode_len(len(x), s, mode)
    E = masked_energy(xc, kept_spans(s, gaps), lead, n)
    en = float(np.sum(nz.astype(np.float64) ** 2))
    thr = en * 10.0 ** (-floor_db / 10.0)
    ok = (E >= thr) & (E > 0)
    out = np.zeros(n)
    out[ok] = raw[ok] / np.sqrt(en * E[ok])
    return out, E, thr


def match_ref(oracle, hay, needle, gaps, p, floor_db=60):
    """score_norm_ref.match_ref on masked scores: per chunk as calc_chunks, chunks that hold a non-finite sample dropped."""
    s = len(needle)
    bad = np.flatnonzero(~np.isfinite(hay))
    peaks = []
    for off, w in ref.chunks(len(hay), s, p.chunk, p.overlap):
        if np.any((bad >= off) & (bad < off + w)):
            continue
        y, _, _ = mncc_ref(oracle, hay[off:off + w], needle, gaps, oracle.MODE_VALID, floor_db)
        for a, b, h, pr in oracle.find_peaks(y.astype(np.float32), p.min_prominence, p.min_distance):
            peaks.append((a + off, b + off, h, pr))
    return ref.overshadow_filter(oracle, peaks, p.sr, p.overshadow_distance_s)


# ---- the per-hit record (am_hit_mask) ---------------------------------------------------------------------------------
BELOW_FLOOR, NONFINITE, GAPS_SILENT, GAPS_NONFINITE, NO_GAPS = 1, 2, 4, 8, 16


def hit_mask_ref(x, needle, gaps, t, floor_db=60):
    """(ncc, gain, kept_db, ncc_gaps, gaps_db, flags) of a hit at t by the definition of include/audiomatch.h, in f64.
    needle: the ORIGINAL samples (the handle zeroes its gaps); gaps None: an ordinary handle."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n64 = np.asarray(needle, dtype=np.float32).astype(np.float64)
    s = len(n64)
    keep = np.ones(s, dtype=bool)
    for b, e in gaps or []:
        keep[b:e] = False
    win = x64[t:t + s]
    nan = np.nan
    if not (np.all(np.isfinite(win[keep])) and np.all(np.isfinite(n64[keep]))):
        return nan, nan, nan, nan, nan, NONFINITE
    en = float(np.dot(n64[keep], n64[keep]))
    ck, ek = float(np.dot(win[keep], n64[keep])), float(np.dot(win[keep], win[keep]))
    flags = 0
    if ek == 0 or ek < en * 10.0 ** (-floor_db / 10.0):
        flags |= BELOW_FLOOR
        ncc = 0.0
    else:
        ncc = ck / np.sqrt(en * ek)
    gain = ck / en if en > 0 else 0.0
    kept_db = -np.inf if ek == 0 else 10 * np.log10(ek / en)
    if not gaps:
        return ncc, gain, kept_db, nan, nan, flags | NO_GAPS
    wg, og = win[~keep], n64[~keep]
    if not (np.all(np.isfinite(wg)) and np.all(np.isfinite(og))):
        return ncc, gain, kept_db, nan, nan, flags | GAPS_NONFINITE
    cg, xg, ng = float(np.dot(wg, og)), float(np.dot(wg, wg)), float(np.dot(og, og))
    if xg == 0:
        flags |= GAPS_SILENT
    ncc_gaps = 0.0 if xg == 0 or ng == 0 else cg / np.sqrt(ng * xg)
    den = gain * gain * ng
    gaps_db = -np.inf if xg == 0 else (np.inf if den == 0 else 10 * np.log10(xg / den))
    return ncc, gain, kept_db, ncc_gaps, gaps_db, flags


def assert_hit_mask(got, exp, tol, tol_db):
    """tol: on the three ratios; tol_db: on the two levels (hit_scores_ref.assert_ref's constants)."""
    assert got.flags == exp[5], (got, exp)
    for name, e in zip(("ncc", "gain", "kept_db", "ncc_gaps", "gaps_db"), exp[:5]):
        g = float(getattr(got, name))
        if np.isnan(e):
            assert np.isnan(g), (name, got, exp)
        elif np.isinf(e):
            assert g == e, (name, got, exp)
        else:
            assert abs(g - e) <= (tol_db if name.endswith("_db") else tol), (name, got, exp)


# ---- design 1: integer spikes on every span edge --------------------------------------------------------------------
B, T = ref.NORM_BLOCK, ref.NORM_TILE
SWITCH = T + 2 * B   # 4096: spans of this length or more are assembled from whole blocks, shorter ones scanned locally


def _gaps_of(n, kept):
    edges = [q for k in kept for q in k]
    return [(a, b) for a, b in zip([0] + edges[1::2], edges[0::2] + [n]) if b > a]


def _sixteen():
    """16 kept spans of lengths 1 .. 300, gaps of 1 .. 120 samples, the first span at 0 and the last up to the end."""
    kept, at = [], 0
    for k in range(16):
        length = (1, 2, 300, 7, 64, 129, 255, 3, 90, 256, 31, 200, 5, 128, 17, 65)[k]
        kept.append((at, at + length))
        at += length + (1, 120, 2, 63, 1, 17, 64, 5, 1, 100, 33, 2, 77, 9, 40, 0)[k]
    return kept[-1][1], kept


# name -> (needle length, kept spans).  Together: span lengths 1, 2, 4095, 4096 and 4097 (the switch between the two
# paths); span starts at 0 and at -1 / 0 / +1 around multiples of kNormBlock and kNormTile; gaps of one sample; leading
# and trailing gaps; 16 kept spans.
DESIGNS = {
    "below":   (5400, [(0, 1), (2, 4), (B - 1, B - 1 + SWITCH - 1), (5200, 5400)]),                  # 4095 from block - 1; a one-sample gap
    "at":      (5300, [(B, B + SWITCH), (B + SWITCH + 1, B + SWITCH + 3)]),                           # 4096 from a block edge; leading and trailing gap
    "above":   (5300, [(1, 2), (B + 1, B + 1 + SWITCH + 1), (5200, 5300)]),                           # 4097 from block + 1; leading gap of one sample
    "tile":    (6400, [(0, 2), (T - 1, T), (T + 1, T + 1 + 100), (T + 200, T + 200 + SWITCH)]),       # starts tile - 1, tile + 1; 4096 from tile + 200
    "tile0":   (6200, [(T, T + SWITCH + 1)]),                                                         # 4097 from a tile edge, alone: both ends gaps
    "sixteen": _sixteen(),
}
DESIGNS = {k: (n, kept, _gaps_of(n, kept)) for k, (n, kept) in DESIGNS.items()}


def design_width(s):
    """Valid-mode scores: one tile and a ragged 301 more."""
    return s + T + 300


def mask_needle(s, seed=1):
    """f32, uniform in [0.25, 1], gap samples included (the handle zeroes them)."""
    return ref.spike_needle(s, seed)


def mask_signal(s, kept, w, mode, seed=1):
    """Zeros with spikes of amplitude 1 or 2: score_norm_ref's positions thinned to amplitude 1 (the signal's ends,
    every block edge and its neighbours, the first and last window's ends of every tile), and for the first and the last
    window of every tile of scores one spike directly inside and one directly outside EVERY edge of every kept span."""
    lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
    x = np.minimum(ref.spike_signal(s, w, mode, seed), np.float32(1.0))
    rng = np.random.default_rng([seed, s, w, mode, 7])
    pos = []
    for t0 in range(0, n, T):
        for t in (t0, min(t0 + T, n) - 1):
            for a, b in kept:
                pos += [t - lead + a - 1, t - lead + a, t - lead + b - 1, t - lead + b]
    pos = np.unique(np.array([q for q in pos if 0 <= q < w], dtype=np.int64))
    # (amplitude 1 or 2 up to four spans; 1 for many spans, whose edge spikes crowd one window: energies stay below 2^8)
    x[pos] = rng.integers(1, 3 if len(kept) <= 4 else 2, size=len(pos)).astype(np.float32)
    return x


def edge_variants(x, kept, lead, n):
    """The masked energy with ONE span edge moved by one sample, every edge either way: [(span, which, by, E), ..]."""
    out = []
    for j, (a, b) in enumerate(kept):
        for which, by in ((0, -1), (0, 1), (1, -1), (1, 1)):
            k = list(kept)
            k[j] = (a + by, b) if which == 0 else (a, b + by)
            if k[j][1] <= k[j][0]:
                continue
            out.append((j, which, by, masked_energy(x, k, lead, n)))
    return out


# the silent case: one gap, loud spikes under it only
SILENT_S, SILENT_GAP = 10000, (4500, 5500)
SILENT_BURST = 100   # spikes in a row, amplitude 100


def silent_case(mode):
    """(needle, gaps, within, lo, hi): kept spans of 4500 samples on either side of a 1000-sample gap (one takes the
    block path); the signal is zero but for SILENT_BURST loud spikes, which lie inside the gap for the scores [lo, hi)."""
    s = SILENT_S
    w = design_width(s)
    lead = ref.lead_of(w, s, mode)
    p = 6700   # (Valid mode: scores [1300, 2201), over the tile edge at 2048)
    within = np.zeros(w, dtype=np.float32)
    within[p:p + SILENT_BURST] = 100.0
    lo = p + SILENT_BURST - SILENT_GAP[1] + lead   # t - lead + gap end >= p + burst
    hi = p - SILENT_GAP[0] + lead + 1              # t - lead + gap begin <= p
    return mask_needle(s), [SILENT_GAP], within, lo, hi


# ---- design 2: plants whose gap holds loud noise --------------------------------------------------------------------
PLANT_S = ref.PLANT_S
GAP_FRACTION = (0.3, 0.7)   # the 40 % gap
# The background, 14 dB under the needle: a plant scores 1 / sqrt(1 + 0.04) = 0.98 under the mask.  Not score_norm_ref's
# 1e-3: the gaps' noise is 68 dB above that, and a transform's absolute error goes with the loudest material of its block
# -- relative to a quiet window's energy it would be 2000 times the f32 rounding, which the 1e-4 of assert_peaks on the
# prominence bases cannot carry.  At 0.05 the ratio is 40.
HAY_NOISE = 0.05


def plant_gap(S):
    return (int(GAP_FRACTION[0] * S), int(GAP_FRACTION[1] * S))


def plant_case(oracle, S, length=ref.PLANT_LEN):
    """(needle, gaps, hay, plants): score_norm_ref's needle (uniform, amplitude 0.25) in a background of uniform noise of
    amplitude HAY_NOISE; a plant at every offset of score_norm_ref.plant_offsets (tile and block edges, a chunk seam, the
    first and the last window) with its gap span OVERWRITTEN by uniform noise of amplitude 2.5: 20 dB above the needle."""
    needle = oracle.synth_uniform(11, 1, 0, S, 0.25).astype(np.float32)
    hay = oracle.synth_uniform(11, 3, 0, length, HAY_NOISE).astype(np.float32)
    g0, g1 = plant_gap(S)
    plants = [t for t, _ in ref.plant_offsets(S, length)]
    for k, t in enumerate(plants):
        hay[t:t + S] += needle
        hay[t + g0:t + g1] = oracle.synth_uniform(11, 20 + k, 0, g1 - g0, 2.5).astype(np.float32)
    return needle, [(g0, g1)], hay, plants


_plant_cache = {}


def plant_setup(am, oracle, S):
    """(needle, gaps, hays, exps, inner, p): as score_norm_ref.plant_setup -- three haystacks (the whole one, one that ends
    one sample behind the seam plant, one that starts one sample in front of it), the checker's peaks of each, the
    plants that are peaks (not on the first or last score) and the match parameters; computed once, never written to."""
    if S not in _plant_cache:
        needle, gaps, hay, plants = plant_case(oracle, S)
        p = ref.plant_params(am, S)
        cut = 2 * p.chunk - 3
        assert cut in plants
        hays = [hay, hay[:cut + S + 1], hay[cut - 1:]]
        exps = [match_ref(oracle, h, needle, gaps, p) for h in hays]
        for h in hays:
            h.setflags(write=False)
        inner = [t for t in plants if 0 < t < len(hay) - S]
        _plant_cache[S] = (needle, gaps, hays, exps, inner, p)
    return _plant_cache[S]
