"""Per-band hit scoring (am_hit_bands*) against the f64 numpy checker of include/audiomatch.h's definition
(tests/hit_bands_ref.py): per band the NCC at lag 0, the coherence, the gain, the level and the needle's share, with the
flags.  Every float field within 2 f32 ulps of the checker's value rounded to f32, plus 1e-9 absolute: the device
computes in f64 from host-built f64 tables, so only the final rounding to f32 and the order of f64 sums differ.
sr = 8000 throughout; the shapes are the smallest at which the kernels can still go wrong."""
import ctypes as C

import numpy as np
import pytest

import hit_bands_ref as ref
from hit_bands_ref import BELOW, EMPTY, NONFIN, bits

pytestmark = pytest.mark.gpu


def noise(seed, n, amp=0.25):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def four_bands(lf):
    f = 1 << lf
    return [0, f // 16, f // 8, f // 4, f // 2 + 1]


def planted(needle, n, t, seed, gain=0.5, amp=0.25):
    hay = noise(seed, n, amp)
    hay[t:t + len(needle)] += np.float32(gain) * needle
    return hay


# ---- 1. every transform size --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lf", [8, 9, 10, 11, 12])
def test_every_transform_size(gpu, lf):
    f = 1 << lf
    s, t = 3 * f + 17, 2 * f + 5
    needle = noise(100 + lf, s, 0.5)
    hay = planted(needle, t + s + f + 3, t, 200 + lf)
    edges = four_bands(lf)
    exp = ref.bands_ref(hay, needle, t, lf, edges)
    assert all(e.flags == 0 and e.ncc > 0.5 for e in exp), exp   # (gain 0.5 over noise of a quarter of the power)
    got = gpu.HipConvolve(needle).hit_bands(hay, peaks_at(gpu, [t]), gpu.band_params(lf, edges))[0]
    ref.assert_records(got, exp)


# ---- 2. frame counts and group seams ------------------------------------------------------------------------------------
SEAM_EDGES = [1, 2, 4, 8, 16, 32, 64, 129]


@pytest.mark.parametrize("r", [0, 127])
def test_frame_counts_and_group_seams(gpu, r):
    base = noise(7, 256 + 128 * 39 + 127, 0.5)
    bp = gpu.band_params(8, SEAM_EDGES)
    for j in range(1, 41):
        s = 256 + 128 * (j - 1) + r
        assert ref.frame_count(s, 8) == j
        needle = base[:s]
        t = 131
        hay = planted(needle, t + s + 64, t, 300 + j)
        got = gpu.HipConvolve(needle).hit_bands(hay, peaks_at(gpu, [t]), bp)[0]
        ref.assert_records(got, ref.bands_ref(hay, needle, t, 8, SEAM_EDGES))


# ---- 3. a pure copy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lf", [8, 11])
def test_pure_copy(gpu, lf):
    f = 1 << lf
    s, t = 5 * f + 100, 77
    needle = noise(31, s, 0.5)
    hay = noise(32, t + s + 50, 0.25)
    hay[t:t + s] = np.float32(0.5) * needle   # (exact in f32)
    edges = four_bands(lf)
    got = gpu.HipConvolve(needle).hit_bands(hay, peaks_at(gpu, [t]), gpu.band_params(lf, edges))[0]
    ref.assert_records(got, ref.bands_ref(hay, needle, t, lf, edges))
    for q in got:
        assert q.flags == 0
        assert abs(q.ncc - 1) <= 1e-6 and abs(q.coherence - 1) <= 1e-6, q
        assert ref.f32_ulps(q.gain, 0.5) <= 2 and abs(q.level_db - 20 * np.log10(0.5)) <= 1e-5, q
    assert abs(sum(q.needle_share for q in got) - 1) <= 1e-6   # (the four bands cover every bin)


# ---- 4. a band-limited needle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lf", [8, 9, 10, 11, 12])
def test_band_limited_needle(gpu, lf):
    f = 1 << lf
    s, t = 3 * f + 17, f + 9
    i = np.arange(s, dtype=np.float64)
    needle = (0.2 * sum(np.cos(2 * np.pi * k * i / f) for k in (3, f // 32, f // 16 - 1))).astype(np.float32)
    hay = planted(needle, t + s + 40, t, 400 + lf)
    edges = four_bands(lf)
    exp = ref.bands_ref(hay, needle, t, lf, edges)
    assert all(not 1e-10 <= e.needle_share <= 1e-8 for e in exp), exp   # no band sits on the EMPTY_BAND threshold
    assert abs(exp[0].needle_share - 0.944) < 2e-3 and abs(exp[1].needle_share - 0.056) < 2e-3
    assert exp[2].needle_share < 1e-12 and exp[3].needle_share < 1e-12
    got = gpu.HipConvolve(needle).hit_bands(hay, peaks_at(gpu, [t]), gpu.band_params(lf, edges))[0]
    ref.assert_records(got, exp)
    assert got[0].flags == 0 and got[1].flags == 0 and got[0].ncc > 0.9
    for q in got[2:]:
        assert q.flags == EMPTY and q.ncc == 0 and q.coherence == 0 and q.gain == 0 and q.level_db == np.inf, q


# ---- 5. the case the feature is for / 6. misalignment -----------------------------------------------------------------
LP_EDGES = [0, 32, 64, 128, 256, 513]
LP_S, LP_T = 16_000, 3000


@pytest.fixture(scope="module")
def lowpassed():
    """A white needle, its copy low-passed at fs / 8 (81-tap windowed sinc) planted at gain 0.5 under +-0.25 noise."""
    needle = noise(51, LP_S, 1.0)
    k = np.arange(81) - 40
    h = 0.25 * np.sinc(0.25 * k) * np.hamming(81)
    copy = np.convolve(needle.astype(np.float64), h, mode="same")
    hay = noise(52, LP_T + LP_S + 2000, 0.25)
    hay[LP_T:LP_T + LP_S] += (0.5 * copy).astype(np.float32)
    return needle, hay


def test_lowpassed_copy(gpu, lowpassed):
    needle, hay = lowpassed
    exp = ref.bands_ref(hay, needle, LP_T, 10, LP_EDGES)
    algo = gpu.HipConvolve(needle)
    got = algo.hit_bands(hay, peaks_at(gpu, [LP_T]), gpu.band_params(10, LP_EDGES))[0]
    print("bands", [(round(q.ncc, 3), round(q.gain, 3)) for q in got])
    ref.assert_records(got, exp)
    whole = algo.hit_scores(hay, peaks_at(gpu, [LP_T]))[0]
    print("broadband ncc", whole.ncc)
    assert all(q.ncc > 0.8 for q in got[:3]), got[:3]
    assert got[4].ncc < 0.1 and whole.ncc < 0.5
    sm = gpu.hit_bands_summary(got, 0.5)
    assert (sm.first_present, sm.last_present, sm.n_present, sm.n_countable) == (0, 2, 3, 5)


def test_misalignment(gpu, lowpassed):
    needle, hay = lowpassed
    bp = gpu.band_params(10, LP_EDGES)
    algo = gpu.HipConvolve(needle)
    on, off = algo.hit_bands(hay, peaks_at(gpu, [LP_T, LP_T + 3]), bp)
    ref.assert_records(off, ref.bands_ref(hay, needle, LP_T + 3, 10, LP_EDGES))
    print("3 samples off", [(round(q.ncc, 3), round(q.coherence, 3)) for q in off])
    assert off[0].coherence > 0.8 and off[0].ncc < on[0].ncc
    assert off[2].coherence > 0.7 and off[2].ncc < 0.2   # (3 samples are more than a quarter period from bin 86 on)


# ---- 7. non-finite samples ----------------------------------------------------------------------------------------------
def test_nonfinite(gpu):
    lf, r = 8, 100
    s = 256 + 128 * 9 + r
    read = ref.span(s, lf)
    assert read == s - r
    needle = noise(61, s, 0.5)
    ts = [50, 4000, 8000]
    hay = noise(62, 8000 + s + 10, 0.25)
    for t in ts:
        hay[t:t + s] += np.float32(0.5) * needle
    bp = gpu.band_params(lf, SEAM_EDGES)
    algo = gpu.HipConvolve(needle)
    clean = algo.hit_bands(hay, peaks_at(gpu, ts), bp)
    for u in (4000, 4000 + 700, 4000 + read - 1):          # first, inner and last sample read
        bad = hay.copy()
        bad[u] = np.nan if u != 4000 + 700 else np.inf
        got = algo.hit_bands(bad, peaks_at(gpu, ts), bp)
        assert bits(got[0]) == bits(clean[0]) and bits(got[2]) == bits(clean[2]), u
        for q in got[1]:
            assert q.flags == NONFIN and all(np.isnan(getattr(q, k)) for k in ref.FIELDS), q
        ref.assert_records(got[1], ref.bands_ref(bad, needle, 4000, lf, SEAM_EDGES))
    for u in (4000 + read, 4000 - 1):                       # the first unread sample behind and the one before the hit
        bad = hay.copy()
        bad[u] = np.nan
        got = algo.hit_bands(bad, peaks_at(gpu, ts), bp)
        assert [bits(h) for h in got] == [bits(h) for h in clean], u
    nd = needle.copy()
    nd[read] = np.nan                                       # the needle's first unread sample
    assert [bits(h) for h in gpu.HipConvolve(nd).hit_bands(hay, peaks_at(gpu, ts), bp)] == [bits(h) for h in clean]
    nd = needle.copy()
    nd[300] = np.nan
    got = gpu.HipConvolve(nd).hit_bands(hay, peaks_at(gpu, ts), bp)
    assert all(q.flags == NONFIN and np.isnan(q.ncc) and np.isnan(q.needle_share) for h in got for q in h)


# ---- 8. floor -------------------------------------------------------------------------------------------------------------
def test_floor(gpu):
    lf, s, t = 9, 512 * 4 + 33, 700
    edges = four_bands(lf)
    needle = noise(71, s, 0.5)
    bp = gpu.band_params(lf, edges)
    algo = gpu.HipConvolve(needle)
    hay = noise(72, t + s + 500, 0.25)
    hay[t:t + s] = 0.0
    got = algo.hit_bands(hay, peaks_at(gpu, [t]), bp)[0]
    ref.assert_records(got, ref.bands_ref(hay, needle, t, lf, edges))
    for q in got:
        assert q.flags == BELOW and q.ncc == 0 and q.coherence == 0 and q.gain == 0 and q.level_db == -np.inf, q
    hay[t:t + s] = needle * np.float32(10 ** (-70 / 20))
    got = algo.hit_bands(hay, peaks_at(gpu, [t]), bp)[0]
    ref.assert_records(got, ref.bands_ref(hay, needle, t, lf, edges))
    assert all(q.flags == BELOW and q.ncc == 0 and q.coherence == 0 and abs(q.level_db + 70) < 0.01 for q in got), got
    keep = gpu.get_option(gpu.OPT_SCORE_NORM_FLOOR_DB)
    gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, 80)
    try:
        low = algo.hit_bands(hay, peaks_at(gpu, [t]), bp)[0]
    finally:
        gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, keep)
    ref.assert_records(low, ref.bands_ref(hay, needle, t, lf, edges, floor_db=80))
    assert all(q.flags == 0 and q.ncc > 0.999 for q in low), low
    # a needle of zeros: every band is empty, whatever the window holds
    zeros = np.zeros(s, dtype=np.float32)
    got = gpu.HipConvolve(zeros).hit_bands(hay, peaks_at(gpu, [t, 0]), bp)
    ref.assert_records(got[0], ref.bands_ref(hay, zeros, t, lf, edges))
    assert all(q.flags == EMPTY and q.needle_share == 0 and q.level_db == np.inf for q in got[0] + got[1])


# ---- 9. ends and overlap ------------------------------------------------------------------------------------------------
def test_ends_and_overlap(gpu):
    lf, s, n = 8, 256 * 5 + 77, 6000
    needle = noise(81, s, 0.5)
    hay = noise(82, n, 0.25)
    for t in (0, 2000, n - s):
        hay[t:t + s] += np.float32(0.5) * needle
    ts = [n - s, 2000, 0, 2300, 1900, 2000]   # both ends; three overlapping spans (and one hit twice), unsorted
    bp = gpu.band_params(lf, SEAM_EDGES)
    algo = gpu.HipConvolve(needle)
    got = algo.hit_bands(hay, peaks_at(gpu, ts), bp)
    for t, h in zip(ts, got):
        ref.assert_records(h, ref.bands_ref(hay, needle, t, lf, SEAM_EDGES))
        assert bits(algo.hit_bands(hay, peaks_at(gpu, [t]), bp)[0]) == bits(h), t   # independent of the call's other hits
    assert bits(got[1]) == bits(got[5])
    assert all(q.ncc > 0.5 for q in got[0] + got[2]), (got[0], got[2])   # (0.5 / sqrt(0.25 + 0.25) = 0.71 for these levels)


# ---- 10. one result, three forms ----------------------------------------------------------------------------------------
def test_three_forms_bit_identical(gpu):
    n = 20_000
    lf = 9
    edges = four_bands(lf)
    bp = gpu.band_params(lf, edges)
    nb = len(edges) - 1
    needles = [noise(31, 5001, 0.5), noise(32, 1777, 0.5)]
    hays = [noise(41, n, 0.1), noise(42, n - 1234, 0.1)]
    lens = [len(h) for h in hays]
    pp = [[[0, 6000, 6500, 12_000], [5, 6100]],            # hits of (haystack 0, needle 0), (haystack 0, needle 1)
          [[lens[1] - 5001, 777], [lens[1] - 1777, 0, 9000]]]
    for k in range(2):
        for j in range(2):
            hays[k][pp[k][j][1]:pp[k][j][1] + len(needles[j])] += needles[j]
    algos = [gpu.HipConvolve(x) for x in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        peaks = [[peaks_at(gpu, pp[k][j]) for j in range(2)] for k in range(2)]
        batch = gpu.hit_bands_batch_device(algos, [b.ptr for b in bufs], lens, peaks, bp)
        for k in range(2):
            for j in range(2):
                dev = algos[j].hit_bands_device(bufs[k].ptr, lens[k], peaks[k][j], bp)
                host = algos[j].hit_bands(hays[k], peaks[k][j], bp)
                assert [bits(h) for h in batch[k][j]] == [bits(h) for h in dev] == [bits(h) for h in host], (k, j)
                for t, h in zip(pp[k][j], dev):
                    ref.assert_records(h, ref.bands_ref(hays[k], needles[j], t, lf, edges))
        # the raw call: cap_per_pair larger than every count, the slots beyond the counts stay as they were
        cap = 6
        pk = (gpu.AmPeak * (4 * cap))()
        counts = (C.c_size_t * 4)()
        for k in range(2):
            for j in range(2):
                counts[2 * k + j] = len(pp[k][j])
                for i, t in enumerate(pp[k][j]):
                    pk[(2 * k + j) * cap + i] = gpu.AmPeak(t, t + 1, 0, 0)
        out = (gpu.HitBand * (4 * cap * nb))()
        C.memset(out, 0xA5, C.sizeof(out))
        gpu._check(gpu.lib().am_hit_bands_batch_device((C.c_void_p * 2)(*[a._h for a in algos]), 2, (C.c_void_p * 2)(*[b.ptr for b in bufs]),
                                                       (C.c_size_t * 2)(*lens), 2, 0, pk, cap, counts, C.byref(bp), out))
        raw = bytes(out)
        rec = C.sizeof(gpu.HitBand)
        assert rec == 24
        for q in range(4):
            for i in range(cap):
                got = raw[(q * cap + i) * nb * rec:(q * cap + i + 1) * nb * rec]
                if i < counts[q]:
                    assert got == b"".join(bits(batch[q // 2][q % 2][i])), (q, i)
                else:
                    assert got == b"\xA5" * (nb * rec), (q, i)
    finally:
        for b in bufs:
            b.free()


def test_pcm16_equals_f32_downmix(gpu):
    rng = np.random.default_rng(9)
    lf, s, frames = 10, 4000, 12_000
    edges = four_bands(lf)
    bp = gpu.band_params(lf, edges)
    needle = noise(9, s, 0.3)
    lr = rng.integers(-9000, 9000, size=(frames, 2)).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(lr)
    ts = [0, 100, 2500, frames - s]
    algo = gpu.HipConvolve(needle)
    b16 = gpu.DeviceBuffer.from_numpy(0, lr)
    b32 = gpu.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_bands_device(b16.ptr, frames, peaks_at(gpu, ts), bp, fmt=gpu.Fmt.S16_STEREO)
        g32 = algo.hit_bands_device(b32.ptr, frames, peaks_at(gpu, ts), bp)
    finally:
        b16.free()
        b32.free()
    assert [bits(h) for h in g16] == [bits(h) for h in g32]
    assert [bits(h) for h in algo.hit_bands(lr, peaks_at(gpu, ts), bp)] == [bits(h) for h in g32]
    for t, h in zip(ts, g32):
        ref.assert_records(h, ref.bands_ref(mono, needle, t, lf, edges))


# ---- 11. errors -----------------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_errors(gpu):
    L = gpu.lib()
    s, n, lf = 2000, 9000, 8
    needle, hay = noise(71, s, 0.5), noise(72, n, 0.1)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    bp = gpu.band_params(lf, SEAM_EDGES)
    nb = bp.n_bands
    out = (gpu.HitBand * (2 * 32))()
    bpp = C.byref(bp)
    INV = gpu.AM_ERR_INVALID_ARG

    def params(lf_, edges):
        return gpu.band_params(lf_, edges)

    many = gpu.AmBandParams(8, 33)
    for b in range(33):
        many.edges[b] = b
    refusals = ((params(7, [0, 10]), "frame_log2"), (params(13, [0, 10]), "frame_log2"), (gpu.AmBandParams(8, 0), "n_bands"),
                (many, "AM_BAND_MAX_BANDS"), (params(8, [0, 10, 10, 20]), "ascending"), (params(8, [5, 3]), "ascending"),
                (params(8, [0, 64, 130]), "F / 2 + 1"), (params(11, [0, 100]), "needle length"))
    try:
        assert _rc(gpu, L.am_hit_bands_device, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK     # n = 0
        assert _rc(gpu, L.am_hit_bands, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK
        cnt = (C.c_size_t * 1)(0)
        assert _rc(gpu, L.am_hit_bands_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                   (C.c_size_t * 1)(n), 1, 0, None, 4, cnt, None, None)[0] == gpu.AM_OK
        for fn, src in ((L.am_hit_bands_device, buf.ptr), (L.am_hit_bands, hay.ctypes.data)):
            for args in ((algo._h, None, n, 0, pk, 1, bpp, out), (algo._h, src, n, 0, None, 1, bpp, out),
                         (algo._h, src, n, 0, pk, 1, bpp, None), (algo._h, src, n, 0, pk, 1, None, out)):     # the last: bp == NULL
                rc, msg = _rc(gpu, fn, *args)
                assert rc == INV and "null" in msg, msg
            assert _rc(gpu, fn, None, src, n, 0, pk, 1, bpp, out)[0] == INV
            for bad, text in refusals:
                rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 1, C.byref(bad), out)
                assert rc == INV and text in msg, (text, msg)
            rc, msg = _rc(gpu, fn, algo._h, src, n, 2, pk, 1, bpp, out)
            assert rc == INV and "format" in msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 2, bpp, out)
            assert rc == INV and "hit 1" in msg and "haystack length" in msg
        rc, msg = _rc(gpu, L.am_hit_bands_device, algo._h, hay.ctypes.data, n, 0, pk, 1, bpp, out)   # host memory
        assert rc == INV and "device" in msg
        # batch: the message names the pair and the hit; the parameters are checked against every needle
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        outs = (gpu.HitBand * (4 * 32))()
        one = (C.c_void_p * 1)(algo._h)
        rc, msg = _rc(gpu, L.am_hit_bands_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 2), bpp, outs)
        assert rc == INV and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_bands_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, hay.ctypes.data),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), bpp, outs)
        assert rc == INV and "pair 1" in msg and "device" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_bands_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), None, outs)
        assert rc == INV and "null" in msg
        for bad, text in refusals[:-1]:
            rc, msg = _rc(gpu, L.am_hit_bands_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                          (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), C.byref(bad), outs)
            assert rc == INV and text in msg, (text, msg)
        short = gpu.HipConvolve(needle[:255])
        rc, msg = _rc(gpu, L.am_hit_bands_batch_device, (C.c_void_p * 2)(algo._h, short._h), 2, (C.c_void_p * 1)(buf.ptr),
                      (C.c_size_t * 1)(n), 1, 0, pairs, 2, (C.c_size_t * 2)(1, 1), bpp, outs)
        assert rc == INV and "needle 1" in msg and "needle length" in msg, msg
        # A haystack on another device than the needle needs a second GPU; on a one-GPU machine only the host-memory
        # refusal above runs.
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, hay)
            try:
                rc, msg = _rc(gpu, L.am_hit_bands_device, algo._h, other.ptr, n, 0, pk, 1, bpp, out)
                assert rc == INV and "device" in msg
            finally:
                other.free()
        # a good call still works after the refusals, and after am_shutdown (the tables and scratch buffers come back), same bits
        before = algo.hit_bands_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)], bp)[0]
        assert len(before) == nb
        ref.assert_records(before, ref.bands_ref(hay, needle, 10, lf, SEAM_EDGES))
    finally:
        buf.free()
    host = algo.hit_bands(hay, [gpu.Peak(10, 11, 0, 0)], bp)[0]
    assert bits(host) == bits(before)
    assert L.am_shutdown() == gpu.AM_OK
    assert bits(algo.hit_bands(hay, [gpu.Peak(10, 11, 0, 0)], bp)[0]) == bits(before)
