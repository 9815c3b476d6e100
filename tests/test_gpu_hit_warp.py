"""Per-hit drift scoring (am_hit_warp*) against the f64 numpy checker of include/audiomatch.h's definition
(tests/hit_warp_ref.py): the best cell over drifts and lags, its two parabola vertices, NCC, gain and level, with the
flags; the three forms bit for bit; the planted drifts of tests/test_hit_warp_host.py through the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hit_segments_ref as sref
import hit_warp_ref as ref
import test_gpu_hit_scores as hs
from hit_warp_ref import BELOW, DRIFT_UNREF, EMPTY, NONFIN, UNREF, bits
from test_hit_warp_host import PLANT_T, PLANTS, plant

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SLICE = int(re.search(r"constexpr int kHitSlice = (\d+);", open(os.path.join(ROOT, "audio-matcher_amd", "csrc", "am_kernels.h")).read()).group(1))


def noise(seed, n, amp=0.25):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def wp_of(am, wp):
    centre, max_ppm, steps, r = wp
    return am.warp_params(max_ppm, steps, r, centre)


@pytest.fixture(scope="module")
def table(gpu):
    return gpu.warp_table()


# ---- 1. checker agreement -----------------------------------------------------------------------------------------------
N_HAY = 60_000
SIZES = (1, 37, SLICE, SLICE + 1, 5000)
GRIDS = [(0.0, 0.0, 0), (0.0, 500.0, 1), (0.0, 4000.0, 8)]
RADII = (0, 1, 16)


def checker_case(s):
    """A white-noise haystack with the needle planted at both ends and in the middle; the hits: the plants (t = 0 and
    t + S = len: positive drifts and lags read outside the buffer), two beside a plant (best lag != 0) and one on plain
    noise.  S = 1: every cell of a one-sample needle is +-1 or 0 up to the rounding of sqrt(a^2 x^2); with both signals on
    a grid of 2^-10 that product is exact, the cells tie exactly and the tie rule decides them."""
    needle = noise(100 + s, s, 0.5)
    hay = noise(200 + s, N_HAY, 0.1)
    plants = [0, N_HAY - s, 20_011]
    for t in plants:
        hay[t:t + s] += np.float32(0.75) * needle
    if s == 1:
        needle = (np.round(needle * 1024) / 1024 + np.float32(2 ** -10)).astype(np.float32)
        hay = (np.round(hay * 1024) / 1024).astype(np.float32)
    ts = plants + [2, N_HAY - s - 3, 7777]
    return needle, hay, ts


@pytest.fixture(scope="module")
def checker_refs(table):
    """The checker's records of every case, computed once: refs[s][wp] = one WarpRef per hit."""
    out = {}
    for s in SIZES:
        needle, hay, ts = checker_case(s)
        out[s] = {(c, mx, k, r): [ref.warp_ref(hay, needle, t, (c, mx, k, r), table) for t in ts] for c, mx, k in GRIDS for r in RADII}
    return out


@pytest.mark.parametrize("s", SIZES)
def test_checker_agreement(gpu, checker_refs, s):
    needle, hay, ts = checker_case(s)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        for wp, exp in checker_refs[s].items():
            got = algo.hit_warp_device(buf.ptr, N_HAY, peaks_at(gpu, ts), wp_of(gpu, wp))
            # the seed excludes no case: the checker's best cell wins clearly wherever another cell differs from it
            assert all(e.margin > 1e-9 for e in exp), (s, wp, [e.margin for e in exp])
            ref.assert_records(got, exp, wp)
            if s >= SLICE and wp[3] == 16:   # the plants are found where they are, the hits beside them at their offsets
                assert all(q.ncc > 0.9 and abs(q.lag) < 0.25 for q in got[:3]), wp
                assert abs(got[3].lag + 2) < 0.25 and abs(got[4].lag - 3) < 0.25, wp
    finally:
        buf.free()


# ---- 2. the three forms / both sample formats ---------------------------------------------------------------------------
def test_three_forms_bit_identical(gpu, table):
    am = gpu
    n = 50_000
    needles = [noise(31, 9001, 0.5), noise(32, 3001, 0.5)]
    hays = [noise(41, n, 0.1), noise(42, n - 1234, 0.1)]
    lens = [len(h) for h in hays]
    pp = [[[0, 12_000, 12_500, 30_000], [5, 12_100]],
          [[lens[1] - 9001, 777], [lens[1] - 3001, 0, 20_000]]]
    for k in range(2):
        for j in range(2):
            hays[k][pp[k][j][1]:pp[k][j][1] + len(needles[j])] += needles[j]
    algos = [am.HipConvolve(x) for x in needles]
    bufs = [am.DeviceBuffer.from_numpy(0, h) for h in hays]
    wp = (100.0, 1200.0, 3, 2)
    w = wp_of(am, wp)
    try:
        peaks = [[peaks_at(am, pp[k][j]) for j in range(2)] for k in range(2)]
        batch = am.hit_warp_batch_device(algos, [b.ptr for b in bufs], lens, peaks, w)
        for k in range(2):
            for j in range(2):
                dev = algos[j].hit_warp_device(bufs[k].ptr, lens[k], peaks[k][j], w)
                host = algos[j].hit_warp(hays[k], peaks[k][j], w)
                assert [bits(h) for h in batch[k][j]] == [bits(h) for h in dev] == [bits(h) for h in host], (k, j)
                ref.assert_records(dev, [ref.warp_ref(hays[k], needles[j], t, wp, table) for t in pp[k][j]], wp)
        # cap_per_pair above every count: the slots behind a pair's hits stay as they were
        cap = 6
        handles = (C.c_void_p * 2)(*[a._h for a in algos])
        arr_p = (C.c_void_p * 2)(*[b.ptr for b in bufs])
        arr_l = (C.c_size_t * 2)(*lens)
        pk = (am.AmPeak * (cap * 4))()
        counts = (C.c_size_t * 4)()
        for k in range(2):
            for j in range(2):
                counts[2 * k + j] = len(pp[k][j])
                for i, t in enumerate(pp[k][j]):
                    pk[(2 * k + j) * cap + i] = am.AmPeak(t, t + 1, 0.0, 0.0)
        out = (am.HitWarp * (cap * 4))()
        C.memset(out, 0xAB, C.sizeof(out))
        assert am.lib().am_hit_warp_batch_device(handles, 2, arr_p, arr_l, 2, 0, pk, cap, counts, C.byref(w), out) == am.AM_OK
        for k in range(2):
            for j in range(2):
                q = 2 * k + j
                assert [bytes(out[q * cap + i]) for i in range(counts[q])] == [bits(h) for h in batch[k][j]]
                assert all(bytes(out[q * cap + i]) == b"\xab" * 40 for i in range(counts[q], cap))
    finally:
        for b in bufs:
            b.free()


def test_pcm16_forms(gpu, table):
    am = gpu
    rng = np.random.default_rng(55)
    frames, s = 40_000, 6000
    lr = rng.integers(-3000, 3000, size=(frames, 2)).astype(np.int16)
    mono = ((lr[:, 0].astype(np.int32) + lr[:, 1]).astype(np.float32) * (np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0)))).astype(np.float32)
    needle = mono[10_000:10_000 + s].copy()
    ts = [10_000, 9_998, 0, frames - s]
    wp = (0.0, 600.0, 2, 4)
    w = wp_of(am, wp)
    algo = am.HipConvolve(needle)
    b16, b32 = am.DeviceBuffer.from_numpy(0, lr), am.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_warp_device(b16.ptr, frames, peaks_at(am, ts), w, am.Fmt.S16_STEREO)
        g32 = algo.hit_warp_device(b32.ptr, frames, peaks_at(am, ts), w)
        both = am.hit_warp_batch_device([algo], [b16.ptr], [frames], [[peaks_at(am, ts)]], w, am.Fmt.S16_STEREO)[0][0]
    finally:
        b16.free()
        b32.free()
    host = algo.hit_warp(lr, peaks_at(am, ts), w)
    assert [bits(h) for h in g16] == [bits(h) for h in g32] == [bits(h) for h in host] == [bits(h) for h in both]
    ref.assert_records(g32, [ref.warp_ref(mono, needle, t, wp, table) for t in ts], wp)
    assert g32[0].ncc > 0.999 and abs(g32[0].drift_ppm) < 50 and abs(g32[1].lag - 2) < 0.1


# ---- 3. independence --------------------------------------------------------------------------------------------------------
def test_a_hit_does_not_depend_on_the_call(gpu):
    am = gpu
    s, n, t = 7000, 60_000, 25_000
    needle, hay = noise(81, s, 0.5), noise(82, n, 0.1)
    hay[t:t + s] += needle
    algo, other = am.HipConvolve(needle), am.HipConvolve(noise(83, 2500, 0.5))
    w = am.warp_params(800.0, 4, 3)
    alone = bits(algo.hit_warp(hay, peaks_at(am, [t]), w)[0])
    others = [int(v) for v in np.random.default_rng(9).integers(0, n - s, 30)]
    crowd = algo.hit_warp(hay, peaks_at(am, others[:15] + [t] + others[15:]), w)
    assert bits(crowd[15]) == alone
    # overlapping and touching spans in the host form
    near = [t - s // 2, t - 3, t, t + 1, t + s // 3]
    assert bits(algo.hit_warp(hay, peaks_at(am, near), w)[2]) == alone
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        assert bits(algo.hit_warp_device(buf.ptr, n, peaks_at(am, [t]), w)[0]) == alone
        batch = am.hit_warp_batch_device([other, algo], [buf.ptr], [n], [[peaks_at(am, others[:5]), peaks_at(am, others[5:9] + [t])]], w)
        assert bits(batch[0][1][4]) == alone
    finally:
        buf.free()


def test_rounds_of_a_large_call_keep_every_bit(gpu):
    """A call whose partial records, or whose warped needles, exceed one round's scratch (kWarpRoundBytes) runs in several
    rounds: every record is what the hit gives in a small call of one round."""
    am = gpu
    limit = int(re.search(r"constexpr size_t kWarpRoundBytes = \(size_t\)(\d+) << 20;", open(os.path.join(ROOT, "audio-matcher_amd", "csrc", "am_kernels.h")).read()).group(1)) << 20
    k, r = 32, 16
    w = am.warp_params(3000.0, k, r)
    record = 8 * (2 * (2 * 16 + 1) + 1)       # bytes per partial record at the widest kernel radius
    # 1. partial records: 1000 hits of a 5000-sample needle, two slices per rate
    s, n = 5000, 60_000
    needle, hay = noise(91, s, 0.5), noise(92, n, 0.1)
    hay[30_000:30_000 + s] += needle
    ts = [30_000] + [int(v) for v in np.random.default_rng(93).integers(0, n - s, 999)]
    per_hit = sum(-(-ref.warp_len(s, d) // SLICE) for d in ref.drifts(0.0, 3000.0, k)) * record
    assert len(ts) * per_hit > limit and 100 * per_hit < limit
    algo = am.HipConvolve(needle)
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        whole = algo.hit_warp_device(buf.ptr, n, peaks_at(am, ts), w)
        parts = [q for i in range(0, len(ts), 100) for q in algo.hit_warp_device(buf.ptr, n, peaks_at(am, ts[i:i + 100]), w)]
        assert [bits(q) for q in whole] == [bits(q) for q in parts]
        assert whole[0].ncc > 0.9 and abs(whole[0].drift_ppm) < 47       # (half a step of the grid)
        assert [bits(q) for q in algo.hit_warp(hay, peaks_at(am, ts), w)] == [bits(q) for q in whole]
    finally:
        buf.free()
    # 2. warped needles: two needles of 130 000 samples, 65 warped forms each, in one batch call
    s, n = 130_000, 300_000
    needles = [noise(94, s, 0.5), noise(95, s, 0.5)]
    assert 4 * 65 * s < limit < 2 * 4 * 65 * s
    hay = noise(96, n, 0.1)
    hay[10_000:10_000 + s] += needles[0]
    hay[150_000:150_000 + s] += needles[1]       # (apart: each plant lies in noise alone)
    algos = [am.HipConvolve(x) for x in needles]
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        pk = [peaks_at(am, [10_000, 150_000]), peaks_at(am, [150_000, 3])]
        batch = am.hit_warp_batch_device(algos, [buf.ptr], [n], [pk], w)[0]
        for j in range(2):
            assert [bits(q) for q in batch[j]] == [bits(q) for q in algos[j].hit_warp_device(buf.ptr, n, pk[j], w)], j
        assert batch[0][0].ncc > 0.9 and batch[1][0].ncc > 0.9 and abs(batch[0][1].ncc) < 0.1
    finally:
        buf.free()


# ---- 4. non-finite samples -----------------------------------------------------------------------------------------------
def test_nonfinite_samples(gpu, table):
    am = gpu
    s, n, t = 5000, 30_000, 8000
    needle, hay = noise(51, s, 0.5), noise(52, n, 0.1)
    hay[t:t + s] += needle
    wp = (0.0, 2000.0, 2, 3)
    w = wp_of(am, wp)
    r = wp[3]
    longest = ref.warp_len(s, 2000.0)
    assert longest > s
    algo = am.HipConvolve(needle)
    clean = algo.hit_warp(hay, peaks_at(am, [t]), w)[0]
    assert clean.flags == 0
    for u, flagged in ((t + r + longest - 1, True), (t + r + longest, False), (t - r, True), (t - r - 1, False), (t + 100, True)):
        bad = hay.copy()
        bad[u] = np.nan
        got = algo.hit_warp(bad, peaks_at(am, [t]), w)[0]
        if flagged:
            assert got.flags == NONFIN and got.drift_ppm == 0.0 and got.lag == 0.0 and got.length == s, (u - t, got)
            assert all(np.isnan(v) for v in (got.ncc, got.gain, got.level_db, got.ncc_centre)), (u - t, got)
        else:
            assert bits(got) == bits(clean), (u - t, got)
        ref.assert_records([got], [ref.warp_ref(bad, needle, t, wp, table)], wp)
    # K = 0 with max_ppm > 0: the one drift is centre_ppm, the widest cell is its own
    one = (300.0, 1500.0, 0, 3)
    own = ref.warp_len(s, 300.0)
    assert s < own < ref.warp_len(s, 1800.0)
    clean = algo.hit_warp(hay, peaks_at(am, [t]), wp_of(am, one))[0]
    for u, flagged in ((t + r + own - 1, True), (t + r + own, False)):
        bad = hay.copy()
        bad[u] = np.nan
        got = algo.hit_warp(bad, peaks_at(am, [t]), wp_of(am, one))[0]
        assert (got.flags == NONFIN) == flagged and (flagged or bits(got) == bits(clean)), (u - t, got)
        ref.assert_records([got], [ref.warp_ref(bad, needle, t, one, table)], one)
    nd = needle.copy()
    nd[1234] = np.inf
    got = am.HipConvolve(nd).hit_warp(hay, peaks_at(am, [t]), am.warp_params(2000.0, 2, 3, 150.0))[0]
    assert got.flags == NONFIN and got.drift_ppm == 150.0 and got.length == s


# ---- 5. consistency with the family ---------------------------------------------------------------------------------------
def test_no_drift_agrees_with_hit_scores_and_segments(gpu):
    am = gpu
    s, n = 5000, 40_000
    needle, hay = noise(1, s, 0.5), noise(2, n, 0.1)
    ts = [0, 9000, 22_222, n - s]
    for t in ts:
        hay[t:t + s] += needle
    algo = am.HipConvolve(needle)
    pk = peaks_at(am, ts + [15_000])
    scores = algo.hit_scores(hay, pk)
    for sc, wr in zip(scores, algo.hit_warp(hay, pk, am.warp_params(0.0, 0, 0))):
        assert wr.flags == UNREF | DRIFT_UNREF and wr.drift_ppm == 0.0 and wr.lag == 0.0 and wr.length == s
        for a, b in ((wr.ncc, sc.ncc), (wr.ncc_centre, sc.ncc), (wr.gain, sc.gain), (wr.level_db, sc.window_db)):
            assert sref.f32_ulps(a, b) <= 2, (sc, wr)
    segs = algo.hit_segments(hay, pk[:4], 1, 2)
    for sg, wr in zip(segs, algo.hit_warp(hay, pk[:4], am.warp_params(0.0, 0, 2))):
        assert abs(wr.lag - sg[0].lag) <= 1e-9 and wr.flags == DRIFT_UNREF | sg[0].flags, (sg, wr)
        assert sref.f32_ulps(wr.ncc, sg[0].ncc) <= 2 and sref.f32_ulps(wr.gain, sg[0].gain) <= 2


# ---- 6. the drift plants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s,n,ppm,wp,cell,tol", PLANTS, ids=[p[0] for p in PLANTS])
def test_planted_drifts(gpu, table, name, s, n, ppm, wp, cell, tol):
    am = gpu
    needle, hay = plant(21, s, n, PLANT_T, ppm)
    exp = ref.warp_ref(hay, needle, PLANT_T, wp, table)
    got = am.HipConvolve(needle).hit_warp(hay, peaks_at(am, [PLANT_T]), wp_of(am, wp))[0]
    print(name, got)
    ref.assert_records([got], [exp], wp)
    assert exp.qstar == cell and exp.margin > 1e-3
    assert got.ncc >= 0.95 and got.ncc_centre <= 0.6 and abs(got.drift_ppm - ppm) <= tol and got.flags == 0
    assert got.length == ref.warp_len(s, ref.drifts(*wp[:3])[cell])


def test_plant_at_the_grid_end_then_recentred(gpu, table):
    am = gpu
    needle, hay = plant(21, 40_000, 50_000, PLANT_T, 200.0)
    algo = am.HipConvolve(needle)
    first = (0.0, 200.0, 4, 4)
    got = algo.hit_warp(hay, peaks_at(am, [PLANT_T]), wp_of(am, first))[0]
    ref.assert_records([got], [ref.warp_ref(hay, needle, PLANT_T, first, table)], first)
    assert got.flags & DRIFT_UNREF and got.drift_ppm == 200.0
    second = (got.drift_ppm, 200.0, 4, 4)
    got = algo.hit_warp(hay, peaks_at(am, [PLANT_T]), wp_of(am, second))[0]
    ref.assert_records([got], [ref.warp_ref(hay, needle, PLANT_T, second, table)], second)
    assert got.flags == 0 and abs(got.drift_ppm - 200.0) <= 2.0 and got.ncc >= 0.95


# ---- 7. flags -------------------------------------------------------------------------------------------------------------
def test_flags(gpu, table):
    am = gpu
    s, n, t = 6000, 30_000, 10_000
    needle = noise(61, s, 0.5)
    wp = (0.0, 800.0, 2, 2)
    w = wp_of(am, wp)
    algo = am.HipConvolve(needle)
    # a plant 80 dB down in digital silence, the floor at 60
    hay = np.zeros(n, dtype=np.float32)
    hay[t:t + s] = needle * np.float32(1e-4)
    got = algo.hit_warp(hay, peaks_at(am, [t]), w)[0]
    ref.assert_records([got], [ref.warp_ref(hay, needle, t, wp, table)], wp)
    assert got.flags & BELOW and got.ncc == 0.0 and got.ncc_centre == 0.0 and abs(got.level_db + 80) < 0.01
    keep = am.get_option(am.OPT_SCORE_NORM_FLOOR_DB)
    am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, 90)
    try:
        low = algo.hit_warp(hay, peaks_at(am, [t]), w)[0]
    finally:
        am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, keep)
    ref.assert_records([low], [ref.warp_ref(hay, needle, t, wp, table, floor_db=90)], wp)
    assert not low.flags & BELOW and low.ncc > 0.999
    # a needle of zeros
    live = noise(62, n, 0.1)
    zero = am.HipConvolve(np.zeros(s, dtype=np.float32))
    got = zero.hit_warp(live, peaks_at(am, [t]), w)[0]
    assert got.flags == EMPTY and got.drift_ppm == 0.0 and got.lag == 0.0 and got.ncc == 0.0 and got.gain == 0.0
    assert got.level_db == np.inf and got.ncc_centre == 0.0 and got.length == s
    ref.assert_records([got], [ref.warp_ref(live, np.zeros(s, dtype=np.float32), t, wp, table)], wp)
    assert np.isnan(zero.hit_warp(np.zeros(n, dtype=np.float32), peaks_at(am, [t]), w)[0].level_db)
    # R = 0
    live[t:t + s] += needle
    got = algo.hit_warp(live, peaks_at(am, [t]), am.warp_params(800.0, 2, 0))[0]
    assert got.flags == UNREF and got.lag == 0.0 and got.ncc > 0.9
    # nothing to do
    assert algo.hit_warp(live, [], w) == []


# ---- 8. interleaved with the other families on one context ---------------------------------------------------------------
def test_interleaved_with_segments_and_scores(gpu):
    am = gpu
    s, n = 9001, 50_000
    hits = [0, 12_000, 12_500, n - s]
    needle, hay = noise(71, s, 0.5), noise(72, n, 0.1)
    for t in hits:
        hay[t:t + s] += needle
    algo = am.HipConvolve(needle)
    pk = peaks_at(am, hits)
    small, large = am.warp_params(300.0, 1, 1), am.warp_params(3000.0, 12, 16)
    want = {"scores": hs.bits(algo.hit_scores(hay, pk)), "segments": [sref.bits(q) for q in algo.hit_segments(hay, pk, 5, 3)],
            "small": [bits(q) for q in algo.hit_warp(hay, pk, small)], "large": [bits(q) for q in algo.hit_warp(hay, pk, large)]}
    assert am.lib().am_shutdown() == am.AM_OK   # every shared buffer, and the interpolator's table, start empty again
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        assert [bits(q) for q in algo.hit_warp(hay, pk[:1], small)] == want["small"][:1]
        assert hs.bits(algo.hit_scores_device(buf.ptr, n, pk)) == want["scores"]
        assert [bits(q) for q in algo.hit_warp_device(buf.ptr, n, pk, large)] == want["large"]
        assert [sref.bits(q) for q in algo.hit_segments(hay, pk, 5, 3)] == want["segments"]
        assert [bits(q) for q in algo.hit_warp(hay, pk, small)] == want["small"]
        assert [sref.bits(q) for q in algo.hit_segments_device(buf.ptr, n, pk, 5, 3)] == want["segments"]
        assert hs.bits(algo.hit_scores(hay, pk)) == want["scores"]
        assert [bits(q) for q in algo.hit_warp(hay, pk, large)] == want["large"]
    finally:
        buf.free()
