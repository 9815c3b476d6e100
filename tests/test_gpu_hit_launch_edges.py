"""The per-hit families where a call changes over: past one grid column (every launch site cuts a call into launches of
at most kHitMaxGridY rows and adds the launch's first row to blockIdx), past one group of am_hit_significance
(kSigGroupSamples), and at the exact edges of the 4096-sample slices of am_hit_scores, am_hit_segments and
am_hit_significance.  Large calls are held, byte for byte, to the same hits scored in small calls, and at chosen hits to
the f64 checkers of the families' own test files, at those files' tolerances."""
import ctypes as C

import numpy as np
import pytest

import hit_bands_ref as bref
import hit_channel_ref as cref
import hit_scores_ref as hsr
import hit_segments_ref as sref
import hit_significance_ref as gref
import hit_stereo_ref as stref
import hit_warp_ref as wref
from hit_launch_calls import (GRID_Y, SEG_EDGE_RADII, SEG_EDGE_SHAPES, SIG_SLICE, SLICE, checked_hits, constant, device_call,
                              in_small_calls, noise, records, seg_edge_case)
from test_gpu_hit_significance import check_hits, library_ref, make_algo

pytestmark = pytest.mark.gpu

F32, S16 = 0, 1     # AM_FMT_F32_MONO, AM_FMT_S16_STEREO
NOISE_DB = 60.0


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def test_constants():
    assert SLICE == 4096 and SIG_SLICE == 4096 and GRID_Y == 65_535


# ---- 1. more rows than one grid column ------------------------------------------------------------------------------------
# A family's case: the entry point and its record; the needle's length s and the number of hits; m, the records a hit gets;
# rows, the grid rows a hit takes in the launch that is cut, and per_record, how many of them end in one record (the three
# rates of a warp hit share one; a segment has a record of its own); the parameters; lead, the R of t_i = i + R;
# check(algo, hay, needle, t, row): the hit's bytes against the family's checker.
class Case:
    def __init__(self, symbol, record, s, hits, check, m=1, rows=1, per_record=1, params=None, lead=0, fmt=F32, taps=0, some=None):
        self.symbol, self.record, self.s, self.hits, self.check, self.m = symbol, record, s, hits, check, m
        self.rows, self.per_record, self.params, self.lead, self.fmt, self.taps = rows, per_record, params, lead, fmt, taps
        self.some = range(hits) if some is None else some     # the hits that the small calls score as well


def _scores(am):
    def check(algo, hay, needle, t, row):
        hsr.assert_ref(records(am.AmHitScore, row)[0], hsr.hit_ref(hay, needle, t))
    return Case("am_hit_scores", am.AmHitScore, SLICE + 1, 65_600, check)     # two slices, the second of one sample


def _segments(am, s, m, r, hits):
    def check(algo, hay, needle, t, row):
        sref.assert_records(records(am.HitSegment, row, m), sref.segments_ref(hay, needle, t, m, r))
    return Case("am_hit_segments", am.HitSegment, s, hits, check, m=m, rows=m, params=am.AmSegmentParams(m, r), lead=r)


def _stereo(am):
    def check(algo, hay, needle, t, row):
        stref.assert_records(records(am.HitStereo, row)[0], stref.stereo_ref(hay, needle, t, 1), t)
    return Case("am_hit_stereo", am.HitStereo, 37, 65_600, check, params=am.AmStereoParams(1, 0), lead=1, fmt=S16)


def _channel(am):
    size = C.sizeof(am.HitChannel)

    def check(algo, hay, needle, t, row):
        taps = np.frombuffer(row[size:].tobytes(), dtype=np.float32)
        cref.assert_record(records(am.HitChannel, row)[0], taps, cref.channel_ref(hay, needle, t, 1, NOISE_DB), t)
    return Case("am_hit_channel", am.HitChannel, 37, 65_600, check, params=am.channel_params(1, NOISE_DB), lead=1, taps=3)


def _warp(am):
    wp = (0.0, 1000.0, 1, 1)
    table = am.warp_table()

    def check(algo, hay, needle, t, row):
        wref.assert_records(records(am.HitWarp, row), [wref.warp_ref(hay, needle, t, wp, table)], wp)
    return Case("am_hit_warp", am.HitWarp, 37, 21_900, check, rows=3, per_record=3, params=am.warp_params(1000.0, 1, 1, 0.0), lead=1)


def _bands(am):
    edges = [1, 32, 129]

    def check(algo, hay, needle, t, row):
        bref.assert_records(records(am.HitBand, row, 2), bref.bands_ref(hay, needle, t, 8, edges))
    return Case("am_hit_bands", am.HitBand, 256, 65_600, check, m=2, params=am.band_params(8, edges))


def _significance(am):
    guard, radius = 2, 8

    def check(algo, hay, needle, t, row):
        gref.assert_record(records(am.HitSignificance, row)[0], library_ref(am, algo, hay, t, guard, radius))
    # (one copy and one correlation launch per hit: the small calls cover the hits below 600, from 65,000 on and every
    # 97th between)
    some = sorted(set(range(600)) | set(range(600, 65_000, 97)) | set(range(65_000, 65_600)))
    return Case("am_hit_significance", am.HitSignificance, 37, 65_600, check, params=am.AmSignificanceParams(guard, radius), lead=radius,
                some=some)


# name: (the case, the (hit, row of that hit) at which the second launch starts)
FAMILIES = {
    "scores": (_scores, (65_535, 0)),
    "segments-37x16": (lambda am: _segments(am, 37, 16, 4, 4_100), (4095, 15)),
    "segments-28677x7": (lambda am: _segments(am, 7 * SLICE + 5, 7, 16, 9_400), (9362, 1)),     # segments of 4096 and 4097 samples, nsl = 2
    "stereo": (_stereo, (65_535, 0)),
    "channel": (_channel, (65_535, 0)),
    "warp": (_warp, (21_845, 0)),
    "bands": (_bands, (65_535, 0)),
    "significance": (_significance, (65_535, 0)),
}


def _large_input(s, hits, lead, rows_per_hit, stereo):
    """White noise of 70,000 + S samples (frames) with the needle planted at three of the hits, among them the hit in which
    the second launch starts; the hits start at i + lead: pairwise distinct."""
    n = 70_000 + s
    ts = np.arange(hits, dtype=np.int64) + lead
    plants = [int(ts[3]), int(ts[GRID_Y // rows_per_hit]), int(ts[-1])]
    if stereo:
        needle = noise(900 + s, s, 0.2)
        hay = np.random.default_rng(901 + s).integers(-3000, 3001, size=(n, 2)).astype(np.int16)
        p = np.rint(needle.astype(np.float64) / stref.K).astype(np.int16)
        for t in plants:     # (full in the left channel, half in the right)
            hay[t:t + s, 0] += p
            hay[t:t + s, 1] += p // 2
    else:
        needle = noise(900 + s, s, 0.5)
        hay = noise(901 + s, n, 0.1)
        for t in plants:
            hay[t:t + s] += needle
    return needle, hay, ts


@pytest.mark.parametrize("family", list(FAMILIES))
def test_more_rows_than_one_grid_column(gpu, family):
    """One device-form call of more than kHitMaxGridY grid rows: (1) every hit's bytes are those of the same hit in a call
    of at most 1000 hits; (2) the f64 checker at the first hits, around the first launch's end and at the last hits;
    (3) the input tells a lost offset apart: the record of row i differs from that of row i - kHitMaxGridY."""
    am = gpu
    make, second_launch = FAMILIES[family]
    f = make(am)
    n_rows = f.hits * f.rows
    assert n_rows > GRID_Y and divmod(GRID_Y, f.rows) == second_launch
    needle, hay, ts = _large_input(f.s, f.hits, f.lead, f.rows, f.fmt == S16)
    algo = make_algo(am, needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)

    def call(some_ts):
        return device_call(am, f.symbol, f.record, f.m, algo, buf.ptr, len(hay), f.fmt, some_ts, f.params, f.taps)
    try:
        # the small calls first: the large call's scratch holds foreign records when it starts
        small, have = in_small_calls(call, ts, f.some)
        large = call(ts)
    finally:
        buf.free()
    # (3) rows as the launches count them, and the record each of them ends in: `each` of those a hit
    each = f.rows // f.per_record
    rec_small = small.reshape(f.hits * each, -1)
    row = np.arange(GRID_Y, n_rows)
    a, b = row // f.per_record, (row - GRID_Y) // f.per_record
    assert have[a // each].all() and have[b // each].all()
    same = ~(rec_small[a] != rec_small[b]).any(axis=1)
    assert not same.any(), (family, "rows whose record equals that of the row one launch earlier", row[same][:10])
    # (1) the bytes of the small calls
    differ = (large != small).any(axis=1) & have
    assert not differ.any(), (family, "hits whose bytes differ from a small call's", np.flatnonzero(differ)[:10], int(differ.sum()))
    # (2) the checker
    for i in checked_hits(f.hits, f.rows):
        f.check(algo, hay, needle, int(ts[i]), large[i])


# ---- 2. am_hit_significance: a call of two groups -------------------------------------------------------------------------
def test_significance_call_of_two_groups(gpu):
    """Eight hits whose spans exceed kSigGroupSamples: groups of 7 and 1.  Every record is the hit's record in a call of
    its own; the last hit of group 1 and the first of group 2 agree with the checker.  (2049 slices a zone: sig_mean and
    sig_finish fetch their partials in 33 rounds of 64.)"""
    am = gpu
    group = constant("am_significance.hip", r"constexpr size_t kSigGroupSamples = \(size_t\)(\d+) << 20;") << 20
    s, radius, guard = 300, am.AM_SIG_MAX_RADIUS, 299
    n = 2 * radius + s + 2000
    ts = [radius + 200 * i for i in range(8)]
    span = 2 * radius + s
    assert all(gref.zone(t, s, n, radius) == (t - radius, t + radius, False) for t in ts) and span == 8_388_908
    sizes, used = [0], 0      # the rule of score_significance: a span joins the group while the group's samples stay within it
    for _ in ts:
        if sizes[-1] and used + span > group:
            sizes.append(0)
            used = 0
        sizes[-1] += 1
        used += (span + 63) // 64 * 64
    assert sizes == [7, 1] and (2 * radius + 1 + SIG_SLICE - 1) // SIG_SLICE == 2049
    needle = noise(61, s, 0.5)
    hay = noise(62, n, 0.1)
    hay[ts[6]:ts[6] + s] += needle
    algo = make_algo(am, needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)

    def call(some_ts):
        return device_call(am, "am_hit_significance", am.HitSignificance, 1, algo, buf.ptr, n, F32, some_ts, am.AmSignificanceParams(guard, radius))
    try:
        alone = np.concatenate([call([t]) for t in ts])
        whole = call(ts)
    finally:
        buf.free()
    assert len({bytes(r) for r in alone}) == 8      # (the input tells the hits apart)
    differ = np.flatnonzero((whole != alone).any(axis=1))
    assert differ.size == 0, ("hits whose bytes differ from a call of their own", differ)
    for i in (6, 7):
        gref.assert_record(records(am.HitSignificance, whole[i])[0], library_ref(am, algo, hay, ts[i], guard, radius))
    assert records(am.HitSignificance, whole[6])[0].z > 10


# ---- 3. exact slice edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE, 2 * SLICE + 1, 64 * SLICE, 64 * SLICE + 1, 128 * SLICE + 1])
def test_scores_at_slice_edges(gpu, s):
    """Needles of exactly one slice, one sample less and more, two slices, and of 64, 65 and 129 partial records a hit
    (hit_combine fetches 64 at a time)."""
    am = gpu
    n, plant = s + 5000, 2500
    needle = noise(300 + s % 1000, s, 0.5)
    hay = noise(400 + s % 1000, n, 0.1)
    hay[plant:plant + s] += needle
    ts = [0, n - s, plant, plant + 1, 1234]
    algo = am.HipConvolve(needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        got = algo.hit_scores_device(buf.ptr, n, peaks_at(am, ts))
    finally:
        buf.free()
    for t, g in zip(ts, got):
        hsr.assert_ref(g, hsr.hit_ref(hay, needle, t))
    assert got[0].flags & hsr.UNREF and got[1].flags & hsr.UNREF
    if s >= SLICE - 1:
        assert got[2].ncc > 0.9 and not got[2].flags & (hsr.BELOW | hsr.NONFIN), got[2]


@pytest.mark.parametrize("s", [SLICE, SLICE + 1])
def test_scores_at_slice_edges_s16_stereo(gpu, s):
    am = gpu
    frames, plant = s + 5000, 2500
    needle = noise(310 + s % 1000, s, 0.2)
    lr = np.random.default_rng(410 + s % 1000).integers(-3000, 3001, size=(frames, 2)).astype(np.int16)
    lr[plant:plant + s] += np.rint(needle.astype(np.float64) / stref.K).astype(np.int16)[:, None]
    mono = am.pcm_s16_stereo_to_mono(lr)
    ts = [0, frames - s, plant, plant + 1, 1234]
    algo = am.HipConvolve(needle)
    b16, b32 = am.DeviceBuffer.from_numpy(0, lr), am.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_scores_device(b16.ptr, frames, peaks_at(am, ts), fmt=am.Fmt.S16_STEREO)
        g32 = algo.hit_scores_device(b32.ptr, frames, peaks_at(am, ts))
    finally:
        b16.free()
        b32.free()
    assert [bytes(am.AmHitScore(q.position, q.ncc, q.gain, q.window_db, q.flags)) for q in g16] == \
           [bytes(am.AmHitScore(q.position, q.ncc, q.gain, q.window_db, q.flags)) for q in g32]
    for t, g in zip(ts, g16):
        hsr.assert_ref(g, hsr.hit_ref(mono, needle, t))
    assert g16[2].ncc > 0.9


@pytest.fixture(scope="module")
def seg_edge_refs():
    """The checker's records of every slice-edge case of am_hit_segments, computed once."""
    out = {}
    for s, m in SEG_EDGE_SHAPES:
        for r in SEG_EDGE_RADII:
            needle, hay, ts = seg_edge_case(s, r)
            out[s, m, r] = [sref.segments_ref(hay, needle, t, m, r) for t in ts]
    return out


@pytest.mark.parametrize("s,m", SEG_EDGE_SHAPES)
def test_segments_at_slice_edges(gpu, seg_edge_refs, s, m):
    """Segments of 4095, 4096 and 4097 samples, at every kernel radius; at (12289, 3) two of the three segments leave the
    second slice that nsl reserves for them unwritten."""
    am = gpu
    lengths = {b - a for a, b in zip(sref.seg_bounds(s, m), sref.seg_bounds(s, m)[1:])}
    assert lengths <= {SLICE - 1, SLICE, SLICE + 1}
    if (s, m) == (3 * SLICE + 1, 3):
        assert sorted(b - a for a, b in zip(sref.seg_bounds(s, m), sref.seg_bounds(s, m)[1:])) == [SLICE, SLICE, SLICE + 1]
    for r in SEG_EDGE_RADII:
        needle, hay, ts = seg_edge_case(s, r)
        algo = am.HipConvolve(needle)
        buf = am.DeviceBuffer.from_numpy(0, hay)
        try:
            got = algo.hit_segments_device(buf.ptr, len(hay), peaks_at(am, ts), m, r)
        finally:
            buf.free()
        for t, g, exp in zip(ts, got, seg_edge_refs[s, m, r]):
            assert all(e.margin > 1e-9 for e in exp), (s, m, r, t)     # the seeds exclude no case
            sref.assert_records(g, exp)
        if r >= 4:     # the plant is found where it is, the hits beside it at their offsets
            assert all(q.ncc > 0.9 and abs(q.lag) < 0.25 for q in got[-3]), (s, m, r)
            assert all(abs(q.lag + 2) < 0.25 for q in got[-2]) and all(abs(q.lag - 2) < 0.25 for q in got[-1]), (s, m, r)


SIG_S, SIG_G = 300, 299


def _sig_case(radius):
    """White noise of 2 B + S + 1000 samples with the needle planted at B + 500, where a hit's zone is unclipped."""
    needle = noise(500 + radius % 1000, SIG_S, 0.5)
    hay = noise(600 + radius % 1000, 2 * radius + SIG_S + 1000, 0.1)
    hay[radius + 500:radius + 500 + SIG_S] += needle
    return needle, hay


@pytest.mark.parametrize("radius,clipped_too", [(2047, False), (2048, True), (4096, True), (131_072, True)])
def test_significance_zone_lengths_at_slice_edges(gpu, radius, clipped_too):
    """Zones of exactly 4095, 4097, 8193 and 262,145 scores (unclipped, 2 B + 1) and of 4096, 8192 and 262,144 (clipped on
    the left at t = B - 1, 2 B): one slice less a score, whole slices, a slice of one score; 64 and 65 partials a hit."""
    am = gpu
    needle, hay = _sig_case(radius)
    ts = [radius + 500] + ([radius - 1] if clipped_too else [])
    want = [2 * radius + 1] + ([2 * radius] if clipped_too else [])
    zones = [gref.zone(t, SIG_S, len(hay), radius) for t in ts]
    assert [hi - lo + 1 for lo, hi, _ in zones] == want and [c for _, _, c in zones] == [False, True][:len(ts)]
    assert want[0] in (SLICE - 1, SLICE + 1, 2 * SLICE + 1, 64 * SLICE + 1) and want[-1] % SLICE in (0, 1, SLICE - 1)
    algo = make_algo(am, needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        got = algo.hit_significance_device(buf.ptr, len(hay), peaks_at(am, ts), SIG_G, radius)
    finally:
        buf.free()
    check_hits(am, algo, hay, ts, SIG_G, radius, got=got)
    assert got[0].z > 10 and got[0].flags == 0


@pytest.mark.parametrize("guard,edge", [(1903, 4096), (1904, 4095), (2191, 8192), (2192, 8193)])
def test_significance_guard_on_a_slice_edge(gpu, guard, edge):
    """B = 6000, unclipped, the hit's own score at zone index 6000: the background's last left index (c - G - 1) or its
    first right index (c + G + 1) lies on a slice's last or first score."""
    am = gpu
    radius = 6000
    needle, hay = _sig_case(radius)
    t = radius + 500
    lo, hi, clipped = gref.zone(t, SIG_S, len(hay), radius)
    assert t - lo == radius and not clipped and edge in (radius - guard - 1, radius + guard + 1)
    assert edge % SIG_SLICE in (0, 1, SIG_SLICE - 1)
    algo = make_algo(am, needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        got = algo.hit_significance_device(buf.ptr, len(hay), peaks_at(am, [t]), guard, radius)
    finally:
        buf.free()
    check_hits(am, algo, hay, [t], guard, radius, got=got)
    assert got[0].n_bg == 2 * (radius - guard) and got[0].z > 10
