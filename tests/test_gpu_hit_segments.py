"""Per-segment hit scoring (am_hit_segments*) against the f64 numpy checker of include/audiomatch.h's definition
(tests/hit_segments_ref.py): per segment the best lag within R samples, its parabola vertex, NCC, gain and level, with
the flags; the summary (coverage, drift) on a truncated and on a time-scaled plant."""
import ctypes as C

import numpy as np
import pytest

import hit_segments_ref as ref
from hit_segments_ref import BELOW, EMPTY, NONFIN, UNREF, bits

pytestmark = pytest.mark.gpu


def noise(seed, n, amp=0.25):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


# ---- 1. checker agreement -----------------------------------------------------------------------------------------------
N_HAY = 60_000
CHECK_M, CHECK_R = (1, 3, 7, 16), (0, 1, 4, 16)


def checker_case(s):
    """A white-noise haystack with the needle planted at gain 0.7 at both ends and in the middle; the hits: the plants
    (t = 0 and t + S = len read outside the buffer), two beside a plant (best lag != 0) and one on plain noise."""
    needle = noise(100 + s, s, 0.5)
    hay = noise(200 + s, N_HAY, 0.1)
    plants = [0, N_HAY - s] + ([20_011] if s <= 5000 else [])
    for t in plants:
        hay[t:t + s] += np.float32(0.7) * needle
    ts = plants + [2, N_HAY - s - 3, 7777]
    return needle, hay, ts


@pytest.fixture(scope="module")
def checker_refs():
    """The checker's records of every case, computed once: refs[s][(m, r)] = one list of SegRef per hit."""
    out = {}
    for s in (1, 37, 5000, 30_000):
        needle, hay, ts = checker_case(s)
        out[s] = {(m, r): [ref.segments_ref(hay, needle, t, m, r) for t in ts] for m in CHECK_M if m <= s for r in CHECK_R}
    return out


@pytest.mark.parametrize("s", [1, 37, 5000, 30_000])
def test_checker_agreement(gpu, checker_refs, s):
    needle, hay, ts = checker_case(s)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        for (m, r), exp in checker_refs[s].items():
            got = algo.hit_segments_device(buf.ptr, N_HAY, peaks_at(gpu, ts), m, r)
            for i, t in enumerate(ts):
                # the seed excludes no case: wherever two lags are examined the checker's best wins clearly
                assert all(e.margin > 1e-9 for e in exp[i]), (s, m, r, t)
                ref.assert_records(got[i], exp[i])
            if s >= 5000 and r >= 4:   # the plants are found where they are, the hits beside them at their offsets
                # (segments of 312 samples and more: the planted lag's score is 17 sigma above the others, the vertex
                # moves it by 0.02 samples rms)
                assert all(q.ncc > 0.9 and abs(q.lag) < 0.25 for q in got[0] + got[1]), (m, r)
                assert all(abs(q.lag + 2) < 0.25 for q in got[-3]) and all(abs(q.lag - 3) < 0.25 for q in got[-2]), (m, r)
    finally:
        buf.free()


# ---- 2. m = 1 agrees with am_hit_scores ---------------------------------------------------------------------------------
def test_one_segment_agrees_with_hit_scores(gpu):
    s, n = 5000, 40_000
    needle = noise(1, s, 0.5)
    hay = noise(2, n, 0.1)
    ts = [0, 9000, 22_222, n - s]
    for t in ts:
        hay[t:t + s] += needle
    ts.append(15_000)   # (plain noise: only R = 0 is compared there)
    algo = gpu.HipConvolve(needle)
    scores = algo.hit_scores(hay, peaks_at(gpu, ts))
    for r in (0, 2):
        segs = algo.hit_segments(hay, peaks_at(gpu, ts), 1, r)
        for sc, sg in list(zip(scores, segs))[:len(ts) if r == 0 else 4]:
            assert len(sg) == 1 and round(sg[0].lag) == 0
            assert ref.f32_ulps(sg[0].ncc, sc.ncc) <= 2 and ref.f32_ulps(sg[0].gain, sc.gain) <= 2, (r, sc, sg)
            assert ref.f32_ulps(sg[0].level_db, sc.window_db) <= 2, (r, sc, sg)


# ---- 3. a truncated plant -------------------------------------------------------------------------------------------------
def test_truncated_plant(gpu):
    s, m, r, t, n = 40_000, 16, 2, 5000, 50_000
    rng = np.random.default_rng(11)
    needle = rng.normal(0, 0.1, s).astype(np.float32)
    hay = rng.normal(0, 0.01, n).astype(np.float32)            # white noise 20 dB below the needle's level
    hay[t:t + s // 2] += needle[:s // 2]
    exp = ref.segments_ref(hay, needle, t, m, r)
    assert all(e.ncc >= 0.9 for e in exp[:8]) and all(abs(e.ncc) <= 0.1 for e in exp[8:]), exp   # the input meets the bounds
    algo = gpu.HipConvolve(needle)
    got = algo.hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    ref.assert_records(got, exp)
    assert all(q.ncc >= 0.9 for q in got[:8]), got[:8]
    assert all(abs(q.ncc) <= 0.1 for q in got[8:]), got[8:]   # 5 sigma of 1 / sqrt(2500) for uncorrelated noise
    sm = gpu.hit_segments_summary(got, s, 0.5)
    assert (sm.coverage, sm.first_present, sm.last_present, sm.n_present) == (0.5, 0, 7, 8)
    whole = gpu.HipConvolve(needle).hit_scores(hay, peaks_at(gpu, [t]))[0]
    assert whole.ncc < 0.75   # the one number of am_hit_scores, for comparison: half the needle is missing


# ---- 4. drift ---------------------------------------------------------------------------------------------------------------
def test_drift(gpu):
    s, m, r, t, n = 40_000, 16, 8, 3000, 50_000
    eps = 200e-6
    rng = np.random.default_rng(21)
    needle = np.convolve(rng.normal(0, 0.3, s + 7), np.ones(8) / 8, mode="valid").astype(np.float32)   # smoothed noise
    hay = rng.normal(0, 0.001, n).astype(np.float32)
    k = np.arange(int(s * (1 + eps)) + 1)
    hay[t:t + len(k)] += np.interp(k / (1 + eps), np.arange(s), needle.astype(np.float64), right=0.0).astype(np.float32)
    exp = ref.segments_ref(hay, needle, t, m, r)
    want = ref.summary_ref(exp, s, 0.5)
    assert abs(want["drift_ppm"] - 200) <= 20 and want["n_usable"] >= 12, want   # the input carries the planted drift
    got = gpu.HipConvolve(needle).hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    ref.assert_records(got, exp, lag_tol=1e-6)
    sm = gpu.hit_segments_summary(got, s, 0.5)
    assert abs(sm.drift_ppm - want["drift_ppm"]) <= 1e-3 and abs(sm.start_lag - want["start_lag"]) <= 1e-6
    assert sm.n_usable == want["n_usable"] and sm.coverage == want["coverage"]
    print("drift_ppm", sm.drift_ppm, "start_lag", sm.start_lag, "residual_rms", sm.residual_rms, "usable", sm.n_usable)


# ---- 5. the three forms / 6. pcm16 ----------------------------------------------------------------------------------------
def test_three_forms_bit_identical(gpu):
    n = 50_000
    needles = [noise(31, 9001, 0.5), noise(32, 3001, 0.5)]
    hays = [noise(41, n, 0.1), noise(42, n - 1234, 0.1)]
    lens = [len(h) for h in hays]
    pp = [[[0, 12_000, 12_500, 30_000], [5, 12_100]],            # hits of (haystack 0, needle 0), (haystack 0, needle 1)
          [[lens[1] - 9001, 777], [lens[1] - 3001, 0, 20_000]]]
    for k in range(2):
        for j in range(2):
            hays[k][pp[k][j][1]:pp[k][j][1] + len(needles[j])] += needles[j]
    algos = [gpu.HipConvolve(x) for x in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    m, r = 5, 3
    try:
        peaks = [[peaks_at(gpu, pp[k][j]) for j in range(2)] for k in range(2)]
        batch = gpu.hit_segments_batch_device(algos, [b.ptr for b in bufs], lens, peaks, m, r)
        for k in range(2):
            for j in range(2):
                dev = algos[j].hit_segments_device(bufs[k].ptr, lens[k], peaks[k][j], m, r)
                host = algos[j].hit_segments(hays[k], peaks[k][j], m, r)
                assert [bits(h) for h in batch[k][j]] == [bits(h) for h in dev] == [bits(h) for h in host], (k, j)
                for t, h in zip(pp[k][j], dev):
                    ref.assert_records(h, ref.segments_ref(hays[k], needles[j], t, m, r))
                    alone = algos[j].hit_segments(hays[k], peaks_at(gpu, [t]), m, r)[0]   # independent of the call's other hits
                    assert bits(alone) == bits(h)
        # the raw call: cap_per_pair larger than every count, the slots beyond the counts stay as they were
        cap = 6
        pk = (gpu.AmPeak * (4 * cap))()
        counts = (C.c_size_t * 4)()
        for k in range(2):
            for j in range(2):
                counts[2 * k + j] = len(pp[k][j])
                for i, t in enumerate(pp[k][j]):
                    pk[(2 * k + j) * cap + i] = gpu.AmPeak(t, t + 1, 0, 0)
        out = (gpu.HitSegment * (4 * cap * m))()
        C.memset(out, 0xA5, C.sizeof(out))
        sp = gpu.AmSegmentParams(m, r)
        gpu._check(gpu.lib().am_hit_segments_batch_device((C.c_void_p * 2)(*[a._h for a in algos]), 2, (C.c_void_p * 2)(*[b.ptr for b in bufs]),
                                                          (C.c_size_t * 2)(*lens), 2, 0, pk, cap, counts, C.byref(sp), out))
        raw = bytes(out)
        rec = C.sizeof(gpu.HitSegment)
        for q in range(4):
            for i in range(cap):
                got = raw[(q * cap + i) * m * rec:(q * cap + i + 1) * m * rec]
                if i < counts[q]:
                    assert got == b"".join(bits(batch[q // 2][q % 2][i])), (q, i)
                else:
                    assert got == b"\xA5" * (m * rec), (q, i)
    finally:
        for b in bufs:
            b.free()


def test_pcm16_equals_f32_downmix(gpu):
    rng = np.random.default_rng(9)
    s, frames = 4000, 30_000
    needle = noise(9, s, 0.3)
    lr = rng.integers(-9000, 9000, size=(frames, 2)).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(lr)
    ts = [0, 100, 2500, 17_000, frames - s]
    algo = gpu.HipConvolve(needle)
    b16 = gpu.DeviceBuffer.from_numpy(0, lr)
    b32 = gpu.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_segments_device(b16.ptr, frames, peaks_at(gpu, ts), 6, 4, fmt=gpu.Fmt.S16_STEREO)
        g32 = algo.hit_segments_device(b32.ptr, frames, peaks_at(gpu, ts), 6, 4)
    finally:
        b16.free()
        b32.free()
    assert [bits(h) for h in g16] == [bits(h) for h in g32]
    assert [bits(h) for h in algo.hit_segments(lr, peaks_at(gpu, ts), 6, 4)] == [bits(h) for h in g32]
    for t, h in zip(ts, g32):
        ref.assert_records(h, ref.segments_ref(mono, needle, t, 6, 4))


# ---- 7. non-finite samples / 8. floor and silence -----------------------------------------------------------------------
def test_nonfinite_flags_its_segments_only(gpu):
    s, n, t, m, r = 10_000, 30_000, 8000, 8, 3
    needle = noise(51, s, 0.5)
    hay = noise(52, n, 0.1)
    hay[t:t + s] += needle
    a = ref.seg_bounds(s, m)
    algo = gpu.HipConvolve(needle)
    clean = algo.hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    # (sample, the segments whose read span [t - R + a_j, t + R + a_{j+1}) holds it)
    for u, hit in ((t + a[3] + 100, [3]), (t + a[5] + r - 1, [4, 5]), (t + a[5] - r, [4, 5]), (t + a[5] + r, [5]),
                   (t + a[5] - r - 1, [4]), (t - r, [0]), (t - r - 1, []), (t + s + r - 1, [7]), (t + s + r, [])):
        bad = hay.copy()
        bad[u] = np.nan
        got = algo.hit_segments(bad, peaks_at(gpu, [t]), m, r)[0]
        assert [j for j in range(m) if got[j].flags & NONFIN] == hit, (u - t, hit)
        for j in range(m):
            if j in hit:
                assert got[j].flags == NONFIN and got[j].lag == 0.0 and np.isnan(got[j].ncc) and np.isnan(got[j].gain) \
                    and np.isnan(got[j].level_db)
            else:
                assert bits([got[j]]) == bits([clean[j]]), (u - t, j)
        ref.assert_records(got, ref.segments_ref(bad, needle, t, m, r))
    nd = needle.copy()
    nd[a[2] + 5] = np.inf
    got = gpu.HipConvolve(nd).hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    assert [q.flags & NONFIN for q in got] == [0, 0, NONFIN, 0, 0, 0, 0, 0]
    assert bits(got[:2] + got[3:]) == bits(clean[:2] + clean[3:])


def test_floor_and_silence(gpu):
    s, n, t, m, r = 8000, 30_000, 10_000, 8, 2
    needle = noise(61, s, 0.5)
    a = ref.seg_bounds(s, m)
    hay = noise(62, n, 0.1)
    hay[t:t + s] += needle
    hay[t + a[2] - r:t + a[3] + r] = 0.0                                             # segment 2 reads digital silence
    hay[t + a[5]:t + a[6]] = needle[a[5]:a[6]] * np.float32(10 ** (-70 / 20))        # segment 5: 70 dB below the needle
    hay[t + a[5] - r:t + a[5]] = 0.0
    hay[t + a[6]:t + a[6] + r] = 0.0
    algo = gpu.HipConvolve(needle)
    got = algo.hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    ref.assert_records(got, ref.segments_ref(hay, needle, t, m, r))
    assert got[2].flags == BELOW | UNREF and got[2].ncc == 0.0 and got[2].level_db == -np.inf and got[2].lag == 0.0 and got[2].gain == 0.0
    assert got[5].flags & BELOW and got[5].ncc == 0.0 and abs(got[5].level_db + 70) < 0.01
    assert all(q.flags == 0 and q.ncc > 0.9 for j, q in enumerate(got) if j not in (2, 5))
    keep = gpu.get_option(gpu.OPT_SCORE_NORM_FLOOR_DB)
    gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, 80)
    try:
        low = algo.hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    finally:
        gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, keep)
    ref.assert_records(low, ref.segments_ref(hay, needle, t, m, r, floor_db=80))
    assert not low[5].flags & BELOW and low[5].ncc > 0.999 and low[2].flags & BELOW
    # a silent stretch of the needle covering segment 3 (and reaching into its neighbours)
    nd = needle.copy()
    nd[a[3] - 10:a[4] + 10] = 0.0
    got = gpu.HipConvolve(nd).hit_segments(hay, peaks_at(gpu, [t]), m, r)[0]
    ref.assert_records(got, ref.segments_ref(hay, nd, t, m, r))
    assert [q.flags & EMPTY for q in got] == [0, 0, 0, EMPTY, 0, 0, 0, 0]
    assert got[3].flags == EMPTY and got[3].lag == 0.0 and got[3].ncc == 0.0 and got[3].gain == 0.0 and got[3].level_db == np.inf
    silent = np.zeros(n, dtype=np.float32)
    got = gpu.HipConvolve(nd).hit_segments(silent, peaks_at(gpu, [t]), m, r)[0]
    assert got[3].flags == EMPTY and np.isnan(got[3].level_db) and got[0].flags == BELOW | UNREF


# ---- 9. errors ----------------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_errors(gpu):
    L = gpu.lib()
    s, n = 5000, 30_000
    needle, hay = noise(71, s, 0.5), noise(72, n, 0.1)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    m = 4
    out = (gpu.HitSegment * (2 * m))()
    sp = gpu.AmSegmentParams(m, 2)
    spp = C.byref(sp)
    INV = gpu.AM_ERR_INVALID_ARG
    try:
        assert _rc(gpu, L.am_hit_segments_device, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK     # n = 0
        assert _rc(gpu, L.am_hit_segments, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK
        cnt = (C.c_size_t * 1)(0)
        assert _rc(gpu, L.am_hit_segments_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                   (C.c_size_t * 1)(n), 1, 0, None, 4, cnt, None, None)[0] == gpu.AM_OK
        for fn, src in ((L.am_hit_segments_device, buf.ptr), (L.am_hit_segments, hay.ctypes.data)):
            for args in ((algo._h, None, n, 0, pk, 1, spp, out), (algo._h, src, n, 0, None, 1, spp, out),
                         (algo._h, src, n, 0, pk, 1, spp, None), (algo._h, src, n, 0, pk, 1, None, out)):     # the last: sp == NULL
                rc, msg = _rc(gpu, fn, *args)
                assert rc == INV and "null" in msg, msg
            assert _rc(gpu, fn, None, src, n, 0, pk, 1, spp, out)[0] == INV
            for bad, text in ((gpu.AmSegmentParams(0, 2), "segments = 0"), (gpu.AmSegmentParams(s + 1, 2), "needle length"),
                              (gpu.AmSegmentParams(1025, 2), "AM_SEG_MAX_SEGMENTS"), (gpu.AmSegmentParams(m, 17), "AM_SEG_MAX_RADIUS")):
                big = (gpu.HitSegment * 8192)()
                rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 1, C.byref(bad), big)
                assert rc == INV and text in msg, msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 2, pk, 1, spp, out)
            assert rc == INV and "format" in msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 2, spp, out)
            assert rc == INV and "hit 1" in msg and "haystack length" in msg
        rc, msg = _rc(gpu, L.am_hit_segments_device, algo._h, hay.ctypes.data, n, 0, pk, 1, spp, out)   # host memory
        assert rc == INV and "device" in msg
        # batch: the message names the pair and the hit; the parameters are checked against every needle
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        outs = (gpu.HitSegment * (4 * m))()
        one = (C.c_void_p * 1)(algo._h)
        rc, msg = _rc(gpu, L.am_hit_segments_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 2), spp, outs)
        assert rc == INV and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_segments_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, hay.ctypes.data),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), spp, outs)
        assert rc == INV and "pair 1" in msg and "device" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_segments_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), None, outs)
        assert rc == INV and "null" in msg
        short = gpu.HipConvolve(needle[:3])
        rc, msg = _rc(gpu, L.am_hit_segments_batch_device, (C.c_void_p * 2)(algo._h, short._h), 2, (C.c_void_p * 1)(buf.ptr),
                      (C.c_size_t * 1)(n), 1, 0, pairs, 2, (C.c_size_t * 2)(1, 1), spp, outs)
        assert rc == INV and "needle 1" in msg and "needle length" in msg, msg
        # A haystack on another device than the needle needs a second GPU; on a one-GPU machine only the host-memory
        # refusal above runs.
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, hay)
            try:
                rc, msg = _rc(gpu, L.am_hit_segments_device, algo._h, other.ptr, n, 0, pk, 1, spp, out)
                assert rc == INV and "device" in msg
            finally:
                other.free()
        # a good call still works after the refusals, and after am_shutdown (the scratch buffers come back), same bits
        before = algo.hit_segments_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)], m, 2)[0]
        ref.assert_records(before, ref.segments_ref(hay, needle, 10, m, 2))
    finally:
        buf.free()
    host = algo.hit_segments(hay, [gpu.Peak(10, 11, 0, 0)], m, 2)[0]
    assert bits(host) == bits(before)
    assert L.am_shutdown() == gpu.AM_OK
    assert bits(algo.hit_segments(hay, [gpu.Peak(10, 11, 0, 0)], m, 2)[0]) == bits(before)
