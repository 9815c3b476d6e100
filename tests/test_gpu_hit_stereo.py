"""The per-hit stereo image (am_hit_stereo*) and the stereo mix (am_pcm_s16_stereo_mix*) against the f64 numpy checker of
include/audiomatch.h's definition (tests/hit_stereo_ref.py): the records at every boundary of the slice kernel and at every
radius the kernel is built for, the exact cases, ncc_mid against am_hit_scores, the three forms bit for bit, the refusals,
the mix bit for bit, and the case the down-mix cannot see, end to end."""
import ctypes as C

import numpy as np
import pytest

import hit_stereo_ref as ref
from hit_stereo_ref import BELOW, COLLINEAR, NONFIN, RIGHT_SILENT, SIDE_SILENT, bits
from test_hit_stereo_host import FRAMES, RADII, SIZES, designed, designed_refs, needle_of

pytestmark = pytest.mark.gpu

S16 = 1     # AM_FMT_S16_STEREO


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def noise(seed, frames, amp=3000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, size=(frames, 2)).astype(np.int16)


def i16_of(needle, gain=1.0):
    """The needle at `gain` in i16 steps (l = k L)."""
    return np.rint(gain * needle.astype(np.float64) / ref.K).astype(np.int16)


# ---- 1. checker agreement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SIZES)
def test_checker_agreement(gpu, s):
    am = gpu
    needle, lr, hits = designed(s)
    for r in RADII:      # first: the checker's margins exclude no case
        assert all(q.margin_left > 1e-9 and q.margin_right > 1e-9 for q in designed_refs(s, r)), (s, r)
    algo = am.HipConvolve(needle)
    buf = am.DeviceBuffer.from_numpy(0, lr)
    try:
        for r in RADII:
            got = algo.hit_stereo_device(buf.ptr, FRAMES, peaks_at(am, hits), r)
            for t, q, exp in zip(hits, got, designed_refs(s, r)):
                ref.assert_records(q, exp, (s, r, t))
    finally:
        buf.free()


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------
def test_exact_cases(gpu):
    am = gpu
    s, r, t, n = 4097, 4, 1000, 8000
    needle = needle_of(s)
    algo = am.HipConvolve(needle)
    p = i16_of(needle)
    lr = np.zeros((n, 2), dtype=np.int16)
    # L == R
    lr[t:t + s, 0] = lr[t:t + s, 1] = p
    q = algo.hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, needle, t, r), "L == R")
    assert q.flags == COLLINEAR | SIDE_SILENT and q.ncc_side == 0.0 and q.ncc_best == abs(q.ncc_left) and q.mix_right == 0.0
    exp = ref.stereo_ref(lr, needle, t, r)
    assert abs(q.mix_left - exp.mix_left) <= 2 * ref.ulp32(exp.mix_left) and abs(exp.mix_left - 1.0) < 1e-4      # mix = (c / E, 0)
    assert am.hit_stereo_summary(q, 0.5).image == am.AM_IMAGE_CENTRE
    # R == 0
    lr[:, 1] = 0
    q = algo.hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, needle, t, r), "R == 0")
    assert q.flags & RIGHT_SILENT and q.flags & COLLINEAR and q.ncc_right == 0.0 and q.ncc_left > 0.9999
    assert am.hit_stereo_summary(q, 0.5).image == am.AM_IMAGE_LEFT
    # R == -L, no noise
    lr[:, 1] = -lr[:, 0]
    q = algo.hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, needle, t, r), "R == -L")
    assert q.flags & BELOW and q.ncc_mid == 0.0 and abs(q.ncc_side - q.ncc_left) <= 2 * ref.ulp32(q.ncc_left) and q.ncc_right < -0.9999
    sm = am.hit_stereo_summary(q, 0.5)
    assert sm.image == am.AM_IMAGE_INVERTED and sm.downmix_loss_db == np.inf and sm.delay == 0.0
    # a needle containing a NaN
    bad = needle.copy()
    bad[s - 3] = np.nan
    q = am.HipConvolve(bad).hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, bad, t, r), "NaN")
    assert q.flags == NONFIN and np.isnan(q.ncc_best) and np.isnan(q.mix_left) and q.lag_left == 0.0 == q.lag_right
    # silence in both channels; a needle of zeros
    q = algo.hit_stereo(np.zeros((n, 2), dtype=np.int16), peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(np.zeros((n, 2), dtype=np.int16), needle, t, r), "silence")
    assert q.ncc_best == 0.0 and q.mix_left == 0.0 == q.mix_right and q.flags & COLLINEAR
    q = am.HipConvolve(np.zeros(s, dtype=np.float32)).hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, np.zeros(s, dtype=np.float32), t, r), "zeros")
    assert q.flags == ref.EMPTY


def test_the_floor_is_the_option_of_hit_scores(gpu):
    am = gpu
    s, r, t, n = 5000, 1, 100, 6000
    needle = needle_of(s)
    lr = np.zeros((n, 2), dtype=np.int16)
    lr[t:t + s, 0] = i16_of(needle, 10 ** -3.5)        # 70 dB under the needle: silent at the floor of 60, present at 90
    lr[t:t + s, 1] = i16_of(needle)
    algo = am.HipConvolve(needle)
    q = algo.hit_stereo(lr, peaks_at(am, [t]), r)[0]
    ref.assert_records(q, ref.stereo_ref(lr, needle, t, r), "floor 60")
    assert q.flags & ref.LEFT_SILENT and q.ncc_left == 0.0
    keep = am.get_option(am.OPT_SCORE_NORM_FLOOR_DB)
    am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, 90)
    try:
        low = algo.hit_stereo(lr, peaks_at(am, [t]), r)[0]
    finally:
        am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, keep)
    ref.assert_records(low, ref.stereo_ref(lr, needle, t, r, floor_db=90), "floor 90")
    assert not low.flags & ref.LEFT_SILENT and low.ncc_left > 0.9


# ---- 3. consistency with am_hit_scores ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (4097, 30_000))
def test_ncc_mid_is_the_ncc_of_hit_scores(gpu, s):
    """ncc_mid against am_hit_scores(...).ncc on the same i16 frames.  am_hit_scores works on the down-mix rounded to f32,
    am_hit_stereo on the exact mid.  What that rounding allows is measured by the checker itself: the f64 NCC of the
    rounded down-mix, d, against the checker's exact ncc_mid, m.  Both library values are f64 results rounded once to f32
    (the checker's own tolerance: 2 ulp or 1e-9), so |got_mid - got_scores| <= |d - m| + 2 (2 ulp + 1e-9)."""
    am = gpu
    needle, lr, hits = designed(s)
    algo = am.HipConvolve(needle)
    mid = algo.hit_stereo(lr, peaks_at(am, hits), 1)
    sc = algo.hit_scores(lr, peaks_at(am, hits))
    x = ref.downmix(lr).astype(np.float64)
    n64 = needle.astype(np.float64)
    en = float(np.dot(n64, n64))
    for t, q, h, exp in zip(hits, mid, sc, designed_refs(s, 1)):
        w = x[t:t + s]
        d = float(np.dot(w, n64) / np.sqrt(en * np.dot(w, w)))
        allowed = abs(d - exp.ncc_mid) + 2 * (2 * ref.ulp32(d) + 1e-9)
        print(s, t, "ncc_mid", q.ncc_mid, "hit_scores", h.ncc, "rounding allows", abs(d - exp.ncc_mid), "difference", abs(q.ncc_mid - h.ncc))
        assert abs(d - exp.ncc_mid) <= 2.0 ** -23, (s, t)        # (the rounding is one of 2^-24 per sample: it cannot move an NCC by more)
        assert abs(q.ncc_mid - h.ncc) <= allowed, (s, t, q.ncc_mid, h.ncc, allowed)


# ---- 4. the three forms ------------------------------------------------------------------------------------------------
def test_three_forms_bit_identical(gpu):
    am = gpu
    r = 4
    needles = [needle_of(2 * 4096 + 37), needle_of(3001)]
    hays = [noise(41, 30_000), noise(42, 30_000 - 1234)]
    lens = [len(h) for h in hays]
    pp = [[[0, 12_000, 12_500, 20_000], []],
          [[lens[1] - len(needles[0]), 777], [lens[1] - 3001, 0, 20_000]]]
    for k in range(2):
        for j in range(2):
            for t in pp[k][j][:2]:
                hays[k][t:t + len(needles[j]), 0] += i16_of(needles[j], 0.7)
                hays[k][t:t + len(needles[j]), 1] -= i16_of(needles[j], 0.35)
    algos = [am.HipConvolve(x) for x in needles]
    bufs = [am.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        peaks = [[peaks_at(am, pp[k][j]) for j in range(2)] for k in range(2)]
        batch = am.hit_stereo_batch_device(algos, [b.ptr for b in bufs], lens, peaks, r)
        for k in range(2):
            for j in range(2):
                if not pp[k][j]:
                    assert batch[k][j] == []
                    continue
                dev = algos[j].hit_stereo_device(bufs[k].ptr, lens[k], peaks[k][j], r)
                host = algos[j].hit_stereo(hays[k], peaks[k][j], r)          # (12 000 and 12 500: overlapping spans)
                assert [bits(q) for q in batch[k][j]] == [bits(q) for q in dev] == [bits(q) for q in host], (k, j)
                for t, q in zip(pp[k][j], dev):
                    ref.assert_records(q, ref.stereo_ref(hays[k], needles[j], t, r), (k, j, t))
                # a hit's record does not depend on the call: each hit alone
                for t, q in zip(pp[k][j], dev):
                    assert bits(algos[j].hit_stereo(hays[k], peaks_at(am, [t]), r)[0]) == bits(q), (k, j, t)
        # a cap_per_pair that cuts pair (0, 0) short, an empty pair; the slots behind a pair's hits keep the sentinel
        cap = 3
        handles = (C.c_void_p * 2)(*[a._h for a in algos])
        arr_p = (C.c_void_p * 2)(*[b.ptr for b in bufs])
        arr_l = (C.c_size_t * 2)(*lens)
        pk = (am.AmPeak * (cap * 4))()
        counts = (C.c_size_t * 4)()
        for k in range(2):
            for j in range(2):
                counts[2 * k + j] = len(pp[k][j])          # (4 for pair 0: above cap)
                for i, t in enumerate(pp[k][j][:cap]):
                    pk[(2 * k + j) * cap + i] = am.AmPeak(t, t + 1, 0.0, 0.0)
        out = (am.HitStereo * (cap * 4))()
        C.memset(out, 0xA5, C.sizeof(out))
        sp = am.AmStereoParams(r, 0)
        assert am.lib().am_hit_stereo_batch_device(handles, 2, arr_p, arr_l, 2, S16, pk, cap, counts, C.byref(sp), out) == am.AM_OK
        for k in range(2):
            for j in range(2):
                q = 2 * k + j
                used = min(counts[q], cap)
                assert [bytes(out[q * cap + i]) for i in range(used)] == [bits(h) for h in batch[k][j][:used]]
                assert all(bytes(out[q * cap + i]) == b"\xa5" * 56 for i in range(used, cap))
    finally:
        for b in bufs:
            b.free()


def test_host_form_reads_its_spans_only(gpu):
    """The host form stages [t - R, t + S + R) of each hit, clipped: frames outside it change no bit."""
    am = gpu
    s, r, n = 4097, 16, 20_000
    needle = needle_of(s)
    lr = noise(61, n)
    algo = am.HipConvolve(needle)
    ts = [0, 5, n - s, n - s - 7, 9000]
    whole = algo.hit_stereo(lr, peaks_at(am, ts), r)
    for t, q in zip(ts, whole):
        masked = np.full((n, 2), 32767, dtype=np.int16)
        lo, hi = max(t - r, 0), min(t + s + r, n)
        masked[lo:hi] = lr[lo:hi]
        assert bits(algo.hit_stereo(masked, peaks_at(am, [t]), r)[0]) == bits(q), t
        ref.assert_records(q, ref.stereo_ref(lr, needle, t, r), t)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_errors(gpu):
    L = gpu.lib()
    s, n, r = 5000, 30_000, 4
    needle, lr = needle_of(s), noise(72, n)
    mono = ref.downmix(lr)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, lr)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    out = (gpu.HitStereo * 4)()
    sp = gpu.AmStereoParams(r, 0)
    spp = C.byref(sp)
    INV = gpu.AM_ERR_INVALID_ARG
    try:
        # n = 0: AM_OK, nothing launched
        gpu.set_option("profile_mask", -1)
        with gpu.Profile(0) as prof:
            assert _rc(gpu, L.am_hit_stereo_device, algo._h, None, n, S16, None, 0, None, None)[0] == gpu.AM_OK
            assert _rc(gpu, L.am_hit_stereo, algo._h, None, n, S16, None, 0, spp, None)[0] == gpu.AM_OK
            cnt = (C.c_size_t * 1)(0)
            assert _rc(gpu, L.am_hit_stereo_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                       (C.c_size_t * 1)(n), 1, S16, None, 4, cnt, None, None)[0] == gpu.AM_OK
            assert prof.query("*")[1] == 0
        for fn, src in ((L.am_hit_stereo_device, buf.ptr), (L.am_hit_stereo, lr.ctypes.data)):
            # the f32 format
            rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 1, spp, out)
            assert rc == INV and "am_hit_stereo: needs interleaved i16 stereo frames" in msg, msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 2, pk, 1, spp, out)
            assert rc == INV and "format" in msg
            for bad, text in ((gpu.AmStereoParams(17, 0), "AM_STEREO_MAX_RADIUS"), (gpu.AmStereoParams(r, 1), "reserved")):
                rc, msg = _rc(gpu, fn, algo._h, src, n, S16, pk, 1, C.byref(bad), out)
                assert rc == INV and text in msg, msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, S16, pk, 2, spp, out)          # start + S > len
            assert rc == INV and "hit 1" in msg and "haystack length" in msg, msg
            for args in ((algo._h, None, n, S16, pk, 1, spp, out), (algo._h, src, n, S16, None, 1, spp, out),
                         (algo._h, src, n, S16, pk, 1, None, out), (algo._h, src, n, S16, pk, 1, spp, None)):
                rc, msg = _rc(gpu, fn, *args)
                assert rc == INV and "null" in msg, msg
            assert _rc(gpu, fn, None, src, n, S16, pk, 1, spp, out)[0] == INV
        rc, msg = _rc(gpu, L.am_hit_stereo_device, algo._h, lr.ctypes.data, n, S16, pk, 1, spp, out)      # host memory
        assert rc == INV and "device" in msg
        # batch: the message names the pair and the hit
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        one = (C.c_void_p * 1)(algo._h)
        two = (C.c_void_p * 2)(buf.ptr, buf.ptr)
        rc, msg = _rc(gpu, L.am_hit_stereo_batch_device, one, 1, two, (C.c_size_t * 2)(n, n), 2, S16, pairs, 2, (C.c_size_t * 2)(1, 2), spp, out)
        assert rc == INV and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_stereo_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, lr.ctypes.data), (C.c_size_t * 2)(n, n), 2, S16,
                      pairs, 2, (C.c_size_t * 2)(1, 1), spp, out)
        assert rc == INV and "pair 1" in msg and "device" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_stereo_batch_device, one, 1, two, (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), spp, out)
        assert rc == INV and "needs interleaved i16 stereo frames" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_stereo_batch_device, one, 1, two, (C.c_size_t * 2)(n, n), 2, S16, pairs, 2, (C.c_size_t * 2)(1, 1), spp, None)
        assert rc == INV and "null" in msg
        # a haystack on another device than the needle needs a second GPU
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, lr)
            try:
                rc, msg = _rc(gpu, L.am_hit_stereo_device, algo._h, other.ptr, n, S16, pk, 1, spp, out)
                assert rc == INV and "device" in msg
            finally:
                other.free()
        # the Python forms refuse an f32 haystack the same way
        with pytest.raises(gpu.AudioMatchError, match="needs interleaved i16 stereo frames"):
            algo.hit_stereo(mono, [gpu.Peak(10, 11, 0, 0)], r)
        # a good call still works after the refusals
        q = algo.hit_stereo_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)], r)[0]
        ref.assert_records(q, ref.stereo_ref(lr, needle, 10, r))
    finally:
        buf.free()
    assert algo.hit_stereo(lr, [], r) == []


# ---- 6. the mix --------------------------------------------------------------------------------------------------------
MIXES = ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.5, -0.5), (0.3, -1.7))


@pytest.mark.parametrize("frames", (0, 1, 3, 4, 5, 4099))
def test_pcm_mix_bit_for_bit(gpu, frames):
    am = gpu
    rng = np.random.default_rng(80 + frames)
    lr = rng.integers(-32768, 32768, size=(frames + 1, 2)).astype(np.int16)
    if frames:
        lr[:min(frames, 3)] = [[32767, 32767], [-32768, -32768], [32767, -32768]][:min(frames, 3)]
    src = am.DeviceBuffer.from_numpy(0, lr)
    dst = am.DeviceBuffer(0, 4 * (frames + 2))
    try:
        for a, b in MIXES:
            want = ref.mix_ref(a, b, lr[:frames])
            assert am.pcm_s16_stereo_mix(lr[:frames], a, b).tobytes() == want.tobytes(), (a, b)
            # the device form, also at a source offset by one frame (unaligned for 16-byte loads) and at a destination
            # offset by one float
            for so, do in ((0, 0), (1, 0), (0, 1), (1, 1)):
                am.pcm_s16_stereo_mix_device(0, src.ptr + 4 * so, frames, a, b, dst.ptr + 4 * do)
                got = dst.to_numpy(np.float32, frames + 2)[do:do + frames]
                assert got.tobytes() == ref.mix_ref(a, b, lr[so:so + frames]).tobytes(), (a, b, so, do)
        assert am.pcm_s16_stereo_mix(lr[:frames], 0.5, 0.5).tobytes() == am.pcm_s16_stereo_to_mono(lr[:frames]).tobytes()
    finally:
        src.free()
        dst.free()


def test_pcm_mix_refusals(gpu):
    L = gpu.lib()
    x = np.zeros(8, dtype=np.int16)
    y = np.zeros(4, dtype=np.float32)
    assert L.am_pcm_s16_stereo_mix(0, None, 4, 1.0, 0.0, y.ctypes.data) == gpu.AM_ERR_INVALID_ARG
    assert L.am_pcm_s16_stereo_mix(0, x.ctypes.data, 4, 1.0, 0.0, None) == gpu.AM_ERR_INVALID_ARG
    assert L.am_pcm_s16_stereo_mix_device(0, None, 4, 1.0, 0.0, None) == gpu.AM_ERR_INVALID_ARG


# ---- 7. end to end: the case the down-mix cannot see -------------------------------------------------------------------
def test_inverted_plant_end_to_end(gpu):
    am = gpu
    s, n, t, sr = 20_000, 200_000, 123_457, 10_000
    needle = np.random.default_rng(91).normal(0, 0.1, s).astype(np.float32)
    lr = noise(92, n).astype(np.int64)
    lr[t:t + s, 0] += i16_of(needle, 0.5)
    lr[t:t + s, 1] -= i16_of(needle, 0.5)
    assert np.abs(lr).max() <= 32767
    lr = lr.astype(np.int16)
    # the input meets the bounds, by the checker
    exp = ref.stereo_ref(lr, needle, t, 4)
    sm = ref.summary_ref(exp, 0.5)
    assert sm[0] == ref.INVERTED and exp.ncc_side > 0.9 and abs(exp.ncc_mid) < 0.1 and sm[3] > 18, (exp, sm)
    algo = am.HipConvolve(needle)
    p = am.Config(chunk_size_s=10.0, overlap_length_s=s / sr, distance_s=5.0, prominence=0.13).params(sr, am.Scale.LIB)
    assert algo.match_pcm16(lr, p) == []                                   # the down-mix: never a hit
    side = am.pcm_s16_stereo_mix(lr, 0.5, -0.5)
    assert side.tobytes() == ref.mix_ref(0.5, -0.5, lr).tobytes()
    hits = algo.match(side, p)                                             # the f32 path on the side signal
    assert [h.start for h in hits] == [t], hits
    q = algo.hit_stereo(lr, hits, 4)[0]
    ref.assert_records(q, exp)
    got = am.hit_stereo_summary(q, 0.5)
    print(q, got)
    assert got.image == am.AM_IMAGE_INVERTED and q.ncc_side > 0.9 and abs(q.ncc_mid) < 0.1 and got.downmix_loss_db > 18
    assert got.delay == q.lag_left - q.lag_right and abs(got.delay) < 0.05
