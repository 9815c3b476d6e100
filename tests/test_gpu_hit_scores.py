"""Per-hit scoring (am_hit_scores*) against an f64 numpy checker of include/audiomatch.h's definitions
(tests/hit_scores_ref.py): exact NCC, least-squares gain, window level and parabolic sub-sample position of each hit,
with the flags."""
import ctypes as C
import struct

import numpy as np
import pytest

from hit_scores_ref import BELOW, NONFIN, UNREF, assert_ref, hit_ref

pytestmark = pytest.mark.gpu


def bits(scores):
    return [struct.pack("<dfffI", q.position, q.ncc, q.gain, q.window_db, q.flags) for q in scores]


def peaks_at(am, ts, s):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def noise(seed, n, amp=0.25):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def case(seed=1, s=5000, n=120_000, plants=(20_000, 61_111, 90_003)):
    needle = noise(seed, s, 0.5)
    hay = noise(seed + 100, n, 0.1)
    for t in plants:
        hay[t:t + s] += needle
    return needle, hay


# ---- 1. checker agreement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1.0, 1 / 64, 4.0])
def test_checker_agreement(gpu, level):
    needle, hay = case()
    hay = (hay * np.float32(level)).astype(np.float32)
    s, n = len(needle), len(hay)
    rng = np.random.default_rng(7)
    ts = [0, n - s, 20_000, 61_111, 90_003, 90_004, 1, n - s - 1] + list(rng.integers(0, n - s, 24))
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        got = algo.hit_scores_device(buf.ptr, n, peaks_at(gpu, ts, s))
    finally:
        buf.free()
    for t, g in zip(ts, got):
        assert_ref(g, hit_ref(hay, needle, t))
    assert got[0].flags & UNREF and got[1].flags & UNREF and got[0].position == 0.0
    assert all(g.ncc > 0.9 for g in got[2:5]), got[2:5]


# ---- 2. gain invariance -------------------------------------------------------------------------------------------------
def test_gain_invariance(gpu):
    needle, hay = case(seed=2)
    s, n = len(needle), len(hay)
    ts = [3, 20_000, 61_111, 61_112, 77_777, n - s]
    algo = gpu.HipConvolve(needle)
    base = algo.hit_scores(hay, peaks_at(gpu, ts, s))
    for k in (-6, 7):
        got = algo.hit_scores((hay * np.float32(2.0 ** k)).astype(np.float32), peaks_at(gpu, ts, s))
        for b, g in zip(base, got):
            assert g.flags == b.flags == (b.flags & UNREF), (b, g)
            assert struct.pack("<f", g.ncc) == struct.pack("<f", b.ncc)
            assert g.gain == np.float32(b.gain * 2.0 ** k) and g.position == b.position


# ---- 3. agreement with the matchers -------------------------------------------------------------------------------------
def test_agreement_with_matchers(gpu):
    sr = 8000
    needle, hay = case(seed=3, s=sr, n=40 * sr, plants=(3 * sr + 5, 17 * sr + 1, 30 * sr + 77))
    hay[14 * sr:22 * sr] *= np.float32(0.05)     # one hit's region recorded quieter
    cfg = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=0.13)
    p = cfg.params(sr, gpu.Scale.LIB)
    ncc_algo = gpu.HipConvolve(needle, score_norm=True)
    hits = ncc_algo.match(hay, p)
    assert hits, "no NCC hits"
    for q, g in zip(hits, ncc_algo.hit_scores(hay, hits)):
        assert abs(q.height - g.ncc) <= 1e-4, (q, g)
    lib_algo = gpu.HipConvolve(needle)
    hits = lib_algo.match(hay, p)
    assert hits, "no LIB hits"
    for q, g in zip(hits, lib_algo.hit_scores(hay, hits)):
        assert abs(q.height - g.gain) <= 1e-4, (q, g)


def test_batch_equals_single_and_checker(gpu):
    sr = 8000
    s, n = sr, 30 * sr
    needles = [noise(40 + j, s, 0.5) for j in range(4)]
    hays = []
    for k in range(3):
        h = noise(50 + k, n, 0.1)
        for j in range(4):
            t = (2 + 6 * j + k) * sr + 13 * j + k
            h[t:t + s] += needles[j]
        hays.append(h)
    algos = [gpu.HipConvolve(x) for x in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=0.13).params(sr, gpu.Scale.LIB)
        res = gpu.match_multi_batch_device(algos, [b.ptr for b in bufs], [n] * 3, p)
        assert sum(len(res[k][j]) for k in range(3) for j in range(4)) >= 12
        batch = gpu.hit_scores_batch_device(algos, [b.ptr for b in bufs], [n] * 3, res)
        for k in range(3):
            for j in range(4):
                single = algos[j].hit_scores_device(bufs[k].ptr, n, res[k][j])
                assert bits(batch[k][j]) == bits(single)
                for q, g in zip(res[k][j], single):
                    assert_ref(g, hit_ref(hays[k], needles[j], q.start))
        # one call with needles of two lengths (hits planted by hand, one overlapping another's window)
        short = needles[0][:3001].copy()
        mixed = [gpu.HipConvolve(needles[1]), gpu.HipConvolve(short)]
        pp = [[peaks_at(gpu, [6 * sr + 13, 9 * sr, 0], s), peaks_at(gpu, [2 * sr, 2 * sr + 500, n - 3001], 3001)]]
        got = gpu.hit_scores_batch_device(mixed, [bufs[0].ptr], [n], pp)
        assert bits(got[0][0]) == bits(mixed[0].hit_scores_device(bufs[0].ptr, n, pp[0][0]))
        assert bits(got[0][1]) == bits(mixed[1].hit_scores_device(bufs[0].ptr, n, pp[0][1]))
        for j, nd in enumerate((needles[1], short)):
            for q, g in zip(pp[0][j], got[0][j]):
                assert_ref(g, hit_ref(hays[0], nd, q.start))
    finally:
        for b in bufs:
            b.free()


# ---- 4. pcm16 / 5. host form ------------------------------------------------------------------------------------------
def test_pcm16_equals_f32_downmix(gpu):
    rng = np.random.default_rng(9)
    s, frames = 4000, 60_000
    needle = noise(9, s, 0.3)
    lr = rng.integers(-9000, 9000, size=(frames, 2)).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(lr)
    ts = [0, 100, 2500, 31_000, frames - s]
    algo = gpu.HipConvolve(needle)
    b16 = gpu.DeviceBuffer.from_numpy(0, lr)
    b32 = gpu.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_scores_device(b16.ptr, frames, peaks_at(gpu, ts, s), fmt=gpu.Fmt.S16_STEREO)
        g32 = algo.hit_scores_device(b32.ptr, frames, peaks_at(gpu, ts, s))
    finally:
        b16.free()
        b32.free()
    assert bits(g16) == bits(g32)
    assert bits(algo.hit_scores(lr, peaks_at(gpu, ts, s))) == bits(g32)
    for t, g in zip(ts, g32):
        assert_ref(g, hit_ref(mono, needle, t))


def test_host_form_equals_device_form(gpu):
    needle, hay = case(seed=5)
    s, n = len(needle), len(hay)
    ts = [61_111, 0, 20_000, 20_001, 20_000 + s - 1, 20_000 + s + 1, 90_003, n - s, n - s - 2]   # overlapping windows
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        dev = algo.hit_scores_device(buf.ptr, n, peaks_at(gpu, ts, s))
    finally:
        buf.free()
    assert bits(algo.hit_scores(hay, peaks_at(gpu, ts, s))) == bits(dev)
    one = [algo.hit_scores(hay, peaks_at(gpu, [t], s))[0] for t in ts]   # independent of the other hits of the call
    assert bits(one) == bits(dev)


# ---- 6. sub-sample position ---------------------------------------------------------------------------------------------
def band_limited(s, seed=3):
    """A Gaussian-windowed sum of sinusoids below 0.12 fs, as a function of (fractional) time."""
    rng = np.random.default_rng(seed)
    f, ph, amp = rng.uniform(0.01, 0.12, 24), rng.uniform(0, 2 * np.pi, 24), rng.uniform(0.5, 1.0, 24)

    def g(tt):
        w = np.exp(-0.5 * ((tt - s / 2) / (s / 6)) ** 2)
        return 0.05 * w * np.sum(amp[:, None] * np.cos(2 * np.pi * f[:, None] * tt[None, :] + ph[:, None]), axis=0)
    return g


def test_sub_sample_position(gpu):
    s, n, t0 = 4000, 20_000, 8000
    g = band_limited(s)
    needle = g(np.arange(s)).astype(np.float32)
    algo = gpu.HipConvolve(needle)
    errs = []
    for d in (0.0, 0.25, -0.4):
        hay = np.zeros(n, dtype=np.float32)
        hay[t0 - 200:t0 + s + 200] = g(np.arange(-200, s + 200) - d)
        got = algo.hit_scores(hay, peaks_at(gpu, [t0], s))[0]
        assert got.flags == 0 and got.ncc > 0.9, got
        errs.append(got.position - (t0 + d))
        assert_ref(got, hit_ref(hay, needle, t0))
    print("sub-sample position error (samples) at delays 0, 0.25, -0.4:", errs)
    assert max(abs(e) for e in errs) <= 0.1, errs


# ---- 7. floor and silence / 8. non-finite -------------------------------------------------------------------------------
def test_floor_and_silence(gpu):
    s, n = 3000, 40_000
    needle = noise(11, s, 0.5)
    hay = noise(12, n)
    hay[5000:5000 + s + 50] = 0.0                                          # a window of exact zeros
    quiet = (needle * np.float32(10 ** (-70 / 20))).astype(np.float32)     # 70 dB below the needle
    hay[20_000 - 10:20_000 + s + 10] = 0.0
    hay[20_000:20_000 + s] = quiet
    algo = gpu.HipConvolve(needle)
    got = algo.hit_scores(hay, peaks_at(gpu, [5001, 20_000], s))
    assert got[0].ncc == 0.0 and got[0].flags & BELOW and got[0].window_db == -np.inf and got[0].gain == 0.0
    assert got[1].ncc == 0.0 and got[1].flags & BELOW
    assert_ref(got[1], hit_ref(hay, needle, 20_000))
    keep = gpu.get_option(gpu.OPT_SCORE_NORM_FLOOR_DB)
    gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, 80)
    try:
        got = algo.hit_scores(hay, peaks_at(gpu, [20_000], s))[0]
    finally:
        gpu.set_option(gpu.OPT_SCORE_NORM_FLOOR_DB, keep)
    assert not got.flags & BELOW and got.ncc > 0.999
    assert_ref(got, hit_ref(hay, needle, 20_000, floor_db=80))


def test_nonfinite_flags_its_hit_only(gpu):
    needle, hay = case(seed=13)
    s = len(needle)
    hay[61_111 + 700] = np.nan            # inside the second hit's window
    hay[90_003 - 1] = np.inf              # the sample before the third hit: that hit is only unrefined
    ts = [20_000, 61_111, 90_003]
    got = gpu.HipConvolve(needle).hit_scores(hay, peaks_at(gpu, ts, s))
    assert got[1].flags == NONFIN and np.isnan(got[1].ncc) and np.isnan(got[1].gain) and got[1].position == 61_111
    assert got[2].flags == UNREF and got[2].position == 90_003 and got[2].ncc > 0.9
    for t, g in zip(ts, got):
        assert_ref(g, hit_ref(hay, needle, t))


# ---- 9. long needle / 10. full size -------------------------------------------------------------------------------------
def test_long_needle(gpu):
    s = (1 << 22) + 12_345                # a partitioned handle
    needle = noise(21, s, 0.5)
    hay = noise(22, s + 300_000, 0.1)
    hay[100_000:100_000 + s] += needle
    algo = gpu.HipConvolve(needle)
    ts = [0, 100_000, 100_001, 250_000, len(hay) - s]
    got = algo.hit_scores(hay, peaks_at(gpu, ts, s))
    for t, g in zip(ts, got):
        assert_ref(g, hit_ref(hay, needle, t))
    assert got[1].ncc > 0.9


def test_full_size_hour(gpu):
    sr = 44100
    n, s = 3600 * sr, 10 * sr
    needle = noise(31, s, 0.5)
    d_needle = gpu.DeviceBuffer.from_numpy(0, needle)
    hay = gpu.synth_uniform_device(0, n, seed=31, stream=1)
    try:
        plants = [(k * 7 * 60 + 30) * sr + 17 * k for k in range(8)]
        for off in plants:
            gpu.axpy_device(0, hay, off, d_needle.ptr, s, 1.0)
        algo = gpu.HipConvolve(needle)
        p = gpu.Config(overlap_length_s=10.0, distance_s=60.0).params(sr, gpu.Scale.LIB)
        hits = algo.match_batch_device([hay.ptr], [n], p)
        assert [q.start for q in hits[0]] == plants
        got = gpu.hit_scores_batch_device([algo], [hay.ptr], [n], [[hits[0]]])[0][0]
        assert bits(got) == bits(algo.hit_scores_device(hay.ptr, n, hits[0]))
        for q, g in zip(hits[0], got):
            assert g.ncc > 0.5, g
            seg = np.empty(s + 2, dtype=np.float32)
            gpu._check(gpu.lib().am_memcpy_d2h(0, seg.ctypes.data, C.c_void_p(hay.ptr + 4 * (q.start - 1)), 4 * (s + 2)))
            pos, ncc, gain, wdb, flags = hit_ref(seg, needle, 1)
            assert_ref(g, (pos - 1 + q.start, ncc, gain, wdb, flags))
    finally:
        hay.free()
        d_needle.free()


# ---- 11. errors ---------------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_errors(gpu):
    L = gpu.lib()
    needle, hay = case(seed=41, n=30_000, plants=())
    s, n = len(needle), len(hay)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    out = (gpu.AmHitScore * 2)()
    try:
        assert _rc(gpu, L.am_hit_scores_device, algo._h, None, n, 0, None, 0, None)[0] == gpu.AM_OK     # n = 0
        assert _rc(gpu, L.am_hit_scores, algo._h, None, n, 0, None, 0, None)[0] == gpu.AM_OK
        cnt = (C.c_size_t * 1)(0)
        assert _rc(gpu, L.am_hit_scores_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                   (C.c_size_t * 1)(n), 1, 0, None, 4, cnt, None)[0] == gpu.AM_OK
        for args in ((algo._h, None, n, 0, pk, 1, out), (algo._h, buf.ptr, n, 0, None, 1, out), (algo._h, buf.ptr, n, 0, pk, 1, None)):
            assert _rc(gpu, L.am_hit_scores_device, *args)[0] == gpu.AM_ERR_INVALID_ARG
        assert _rc(gpu, L.am_hit_scores_device, None, buf.ptr, n, 0, pk, 1, out)[0] == gpu.AM_ERR_INVALID_ARG
        rc, msg = _rc(gpu, L.am_hit_scores_device, algo._h, buf.ptr, n, 2, pk, 1, out)
        assert rc == gpu.AM_ERR_INVALID_ARG and "format" in msg
        rc, msg = _rc(gpu, L.am_hit_scores_device, algo._h, buf.ptr, n, 0, pk, 2, out)
        assert rc == gpu.AM_ERR_INVALID_ARG and "hit 1" in msg
        rc, msg = _rc(gpu, L.am_hit_scores, algo._h, hay.ctypes.data, n, 0, pk, 2, out)
        assert rc == gpu.AM_ERR_INVALID_ARG and "hit 1" in msg
        rc, msg = _rc(gpu, L.am_hit_scores_device, algo._h, hay.ctypes.data, n, 0, pk, 1, out)   # host memory
        assert rc == gpu.AM_ERR_INVALID_ARG and "device" in msg
        # batch: the message names the pair and the hit
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        outs = (gpu.AmHitScore * 4)()
        rc, msg = _rc(gpu, L.am_hit_scores_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 2), outs)
        assert rc == gpu.AM_ERR_INVALID_ARG and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_scores_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 2)(buf.ptr, hay.ctypes.data),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), outs)
        assert rc == gpu.AM_ERR_INVALID_ARG and "pair 1" in msg and "device" in msg, msg
        # A haystack on another device than the needle.  This needs a second GPU: on a one-GPU machine only the
        # host-memory refusal above runs, and the device-mismatch branch of hit_check_device (am_hits.hip) is not
        # exercised.
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, hay)
            try:
                rc, msg = _rc(gpu, L.am_hit_scores_device, algo._h, other.ptr, n, 0, pk, 1, out)
                assert rc == gpu.AM_ERR_INVALID_ARG and "device" in msg
            finally:
                other.free()
        # a good call still works after the refusals
        assert algo.hit_scores_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)])[0].flags in (0, UNREF, BELOW, UNREF | BELOW)
    finally:
        buf.free()


def test_after_shutdown(gpu):
    """am_shutdown releases the hit-scoring buffers with the others; the next call allocates them again, same bits."""
    needle, hay = case(seed=51)
    s, n = len(needle), len(hay)
    ts = [0, 20_000, 61_111, n - s]
    algo = gpu.HipConvolve(needle)
    before = bits(algo.hit_scores(hay, peaks_at(gpu, ts, s)))
    assert gpu.lib().am_shutdown() == gpu.AM_OK
    assert bits(algo.hit_scores(hay, peaks_at(gpu, ts, s))) == before
