"""Per-hit channel estimation (am_hit_channel*) against the f64 numpy checker of include/audiomatch.h's definition
(tests/hit_channel_ref.py): the taps and the record at every boundary of the slice kernel (slices of 4096 needle samples,
tiles of 32 lags), a known channel recovered, the haystack's edges, the three forms bit for bit, the flags and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hit_channel_ref as ref
from hit_channel_ref import BELOW, EMPTY, NONFIN, bits
from test_hit_channel_host import G, ar1, downmix, white

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNELS_H = open(os.path.join(ROOT, "audio-matcher_amd", "csrc", "am_kernels.h")).read()
SLICE = int(re.search(r"constexpr int kHitSlice = (\d+);", KERNELS_H).group(1))
TILE = int(re.search(r"constexpr int kLagTile = (\d+);", KERNELS_H).group(1))
SIZES = (37, SLICE, SLICE + 1, 2 * SLICE + 37)     # under one slice, exactly one, one over, two and a ragged third
RADII = (0, 1, 15, 16, 17, 128)                    # 31, 33 and 35 lags straddle the 32-lag tile; 257 spans nine tiles
NOISE_DB = 60.0


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def unit_noise(seed, n):
    return np.random.default_rng(seed).normal(0, 1.0, n).astype(np.float32)


def needle_of(kind, s):
    return white(300 + s, s) if kind == "white" else ar1(400 + s, s)


def planted(kind, s, p):
    """The needle at gain 0.7 in unit noise, in a haystack of about 3 S + 4 P samples; (needle, hay, t)."""
    needle = needle_of(kind, s)
    t = s + 2 * p + 3
    hay = unit_noise(500 + s + p, 3 * s + 4 * p + 11)
    hay[t:t + s] += np.float32(0.7) * needle
    return needle, hay, t


def through(needle, n, t):
    """A silent haystack of n samples that holds the needle through G at t, and nothing else."""
    hay = np.zeros(n, dtype=np.float64)
    for l, g in G.items():
        hay[t + l:t + l + len(needle)] += g * needle.astype(np.float64)
    return hay.astype(np.float32)


def packed(recs, taps):
    return [bits(q) for q in recs], taps.tobytes()


# ---- 1. sums and records against the checker ----------------------------------------------------------------------------
def test_constants():
    assert SLICE == 4096 and TILE == 32 and SIZES[3] == 8229


@pytest.mark.parametrize("s", SIZES)
def test_checker_agreement(gpu, s):
    am = gpu
    for kind in ("white", "ar1"):
        algo = am.HipConvolve(needle_of(kind, s))
        for p in RADII:
            needle, hay, t = planted(kind, s, p)
            ts = [t, t + 2, 5]                     # the plant, beside it, plain noise
            buf = am.DeviceBuffer.from_numpy(0, hay)
            try:
                recs, taps = algo.hit_channel_device(buf.ptr, len(hay), peaks_at(am, ts), am.channel_params(p, NOISE_DB))
            finally:
                buf.free()
            assert taps.shape == (3, 2 * p + 1)
            for i, u in enumerate(ts):
                exp = ref.channel_ref(hay, needle, u, p, NOISE_DB)
                assert exp.cond <= 1e5, (kind, s, p, exp.cond)
                ref.assert_record(recs[i], taps[i], exp, (kind, s, p, u))
            # the plant is found where it is: a tap's standard error in unit noise is 1 / (0.3 sqrt(S)) for the white needle
            if s >= SLICE and kind == "white":
                assert recs[0].main_tap == 0 and abs(taps[0][p] - 0.7) < 5 / (0.3 * np.sqrt(s)) and recs[0].flags == 0, (kind, s, p, recs[0])
                if p >= 2:
                    assert recs[1].main_tap == -2, (kind, s, p, recs[1])


# ---- 2. recovery: the test a user reads ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (SLICE + 1, 2 * SLICE + 37))
def test_a_known_channel_is_recovered(gpu, s):
    """A needle that went through g = {0: 1, 3: 0.5, -2: -0.25} and lies alone in its span: the plain NCC is low, the taps
    are g, the filtered needle explains the span."""
    am = gpu
    p, t = 8, 100
    needle = white(600 + s, s)
    hay = through(needle, s + 300, t)
    recs, taps = am.HipConvolve(needle).hit_channel(hay, peaks_at(am, [t]), am.channel_params(p, 200.0))
    want = np.zeros(2 * p + 1)
    for l, g in G.items():
        want[l + p] = g
    q = recs[0]
    print(q, "taps error", np.abs(taps[0] - want).max())
    # (the haystack's samples are the f32 roundings of g * n: the taps carry that rounding, 6e-8 relative, and no more)
    assert np.abs(taps[0] - want).max() <= 1e-6
    assert q.ncc_eq >= 1 - 1e-6 and q.residual_db <= -100 and q.ncc < 0.9 and q.flags == 0
    assert q.main_tap == 0 and abs(q.main_share - 1 / (1 + 0.25 + 0.0625)) < 1e-5
    assert abs(q.gain_db - 10 * np.log10(1 + 0.25 + 0.0625)) < 0.5      # (a white needle: q / E_n is close to |g|^2)
    ref.assert_record(q, taps[0], ref.channel_ref(hay, needle, t, p, 200.0))


# ---- 3. edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (17, 128))
def test_edges_of_the_haystack(gpu, p):
    am = gpu
    s = SLICE + 1
    needle = white(700, s)
    n = 3 * s + 4 * p
    hay = unit_noise(701 + p, n)
    ts = [0, p - 3, n - s, n - s - p + 2, s + p]
    for t in ts:
        hay[t:t + s] += np.float32(0.7) * needle
    algo = am.HipConvolve(needle)
    cp = am.channel_params(p, NOISE_DB)
    recs, taps = algo.hit_channel(hay, peaks_at(am, ts), cp)
    for i, t in enumerate(ts):
        ref.assert_record(recs[i], taps[i], ref.channel_ref(hay, needle, t, p, NOISE_DB), (p, t))
    # the host form reads nothing outside [t - P, t + S + P) clipped: NaN everywhere else changes no bit
    for i, t in enumerate(ts):
        masked = np.full(n, np.nan, dtype=np.float32)
        lo, hi = max(t - p, 0), min(t + s + p, n)
        masked[lo:hi] = hay[lo:hi]
        one, tp = algo.hit_channel(masked, peaks_at(am, [t]), cp)
        assert bits(one[0]) == bits(recs[i]) and tp[0].tobytes() == taps[i].tobytes(), (p, t)


# ---- 4. the three forms / both sample formats ---------------------------------------------------------------------------
def test_three_forms_bit_identical(gpu):
    am = gpu
    p = 17
    needles = [white(31, 2 * SLICE + 37), white(32, 3001)]
    hays = [unit_noise(41, 30_000), unit_noise(42, 30_000 - 1234)]
    lens = [len(h) for h in hays]
    pp = [[[0, 12_000, 12_500, 20_000], []],
          [[lens[1] - len(needles[0]), 777], [lens[1] - 3001, 0, 20_000]]]
    for k in range(2):
        for j in range(2):
            for t in pp[k][j][:2]:
                hays[k][t:t + len(needles[j])] += np.float32(0.7) * needles[j]
    algos = [am.HipConvolve(x) for x in needles]
    bufs = [am.DeviceBuffer.from_numpy(0, h) for h in hays]
    cp = am.channel_params(p, NOISE_DB)
    try:
        peaks = [[peaks_at(am, pp[k][j]) for j in range(2)] for k in range(2)]
        batch = am.hit_channel_batch_device(algos, [b.ptr for b in bufs], lens, peaks, cp)
        for k in range(2):
            for j in range(2):
                if not pp[k][j]:
                    assert batch[k][j][0] == [] and batch[k][j][1].shape == (0, 2 * p + 1)
                    continue
                dev = algos[j].hit_channel_device(bufs[k].ptr, lens[k], peaks[k][j], cp)
                host = algos[j].hit_channel(hays[k], peaks[k][j], cp)
                assert packed(*batch[k][j]) == packed(*dev) == packed(*host), (k, j)
                for i, t in enumerate(pp[k][j]):
                    ref.assert_record(dev[0][i], dev[1][i], ref.channel_ref(hays[k], needles[j], t, p, NOISE_DB), (k, j, t))
        # cap_per_pair above every count: the slots behind a pair's hits stay as they were, records and taps
        cap, nt = 6, 2 * p + 1
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
        out = (am.HitChannel * (cap * 4))()
        C.memset(out, 0xA5, C.sizeof(out))
        tp = np.frombuffer(b"\xa5" * (4 * cap * 4 * nt), dtype=np.float32).copy().reshape(cap * 4, nt)
        assert am.lib().am_hit_channel_batch_device(handles, 2, arr_p, arr_l, 2, 0, pk, cap, counts, C.byref(cp), out, tp.ctypes.data) == am.AM_OK
        for k in range(2):
            for j in range(2):
                q = 2 * k + j
                assert [bytes(out[q * cap + i]) for i in range(counts[q])] == [bits(h) for h in batch[k][j][0]]
                assert tp[q * cap:q * cap + counts[q]].tobytes() == batch[k][j][1].tobytes()
                assert all(bytes(out[q * cap + i]) == b"\xa5" * 32 for i in range(counts[q], cap))
                assert tp[q * cap + counts[q]:(q + 1) * cap].tobytes() == b"\xa5" * (4 * nt * (cap - counts[q]))
    finally:
        for b in bufs:
            b.free()


def test_a_hit_does_not_depend_on_the_call(gpu):
    am = gpu
    s, n, t, p = SLICE + 1, 30_000, 9000, 16
    needle, hay = white(81, s), unit_noise(82, n)
    hay[t:t + s] += np.float32(0.7) * needle
    algo, other = am.HipConvolve(needle), am.HipConvolve(white(83, 2500))
    cp = am.channel_params(p, NOISE_DB)
    alone = packed(*algo.hit_channel(hay, peaks_at(am, [t]), cp))
    others = [int(v) for v in np.random.default_rng(9).integers(0, n - s, 12)]
    recs, taps = algo.hit_channel(hay, peaks_at(am, others[:6] + [t] + others[6:]), cp)
    assert ([bits(recs[6])], taps[6].tobytes()) == alone
    near = [t - s // 2, t - 3, t, t + 1, t + s // 3]          # overlapping and touching spans in the host form
    recs, taps = algo.hit_channel(hay, peaks_at(am, near), cp)
    assert ([bits(recs[2])], taps[2].tobytes()) == alone
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        recs, taps = am.hit_channel_batch_device([other, algo], [buf.ptr], [n], [[peaks_at(am, others[:5]), peaks_at(am, others[5:9] + [t])]], cp)[0][1]
        assert ([bits(recs[4])], taps[4].tobytes()) == alone
    finally:
        buf.free()


def test_pcm16_equals_f32_on_the_downmix(gpu):
    am = gpu
    rng = np.random.default_rng(55)
    frames, s, p = 20_000, SLICE + 1, 17
    lr = rng.integers(-3000, 3000, size=(frames, 2)).astype(np.int16)
    mono = downmix(lr)
    needle = mono[6000:6000 + s].copy()
    ts = [6000, 5998, 0, frames - s]
    cp = am.channel_params(p, NOISE_DB)
    algo = am.HipConvolve(needle)
    b16, b32 = am.DeviceBuffer.from_numpy(0, lr), am.DeviceBuffer.from_numpy(0, mono)
    try:
        g16 = algo.hit_channel_device(b16.ptr, frames, peaks_at(am, ts), cp, am.Fmt.S16_STEREO)
        g32 = algo.hit_channel_device(b32.ptr, frames, peaks_at(am, ts), cp)
        both = am.hit_channel_batch_device([algo], [b16.ptr], [frames], [[peaks_at(am, ts)]], cp, am.Fmt.S16_STEREO)[0][0]
    finally:
        b16.free()
        b32.free()
    host = algo.hit_channel(lr, peaks_at(am, ts), cp)
    assert packed(*g16) == packed(*g32) == packed(*host) == packed(*both)
    for i, t in enumerate(ts):
        ref.assert_record(g32[0][i], g32[1][i], ref.channel_ref(mono, needle, t, p, NOISE_DB), t)
    assert g32[0][0].ncc > 0.999 and g32[0][0].main_tap == 0 and g32[0][1].main_tap == 2


def test_rounds_of_a_large_call_keep_every_bit(gpu):
    """A call whose partial records exceed one round's scratch (kChanRoundBytes) runs in several rounds: every record is
    what the hit gives in a small call of one round."""
    am = gpu
    limit = int(re.search(r"constexpr size_t kChanRoundBytes = \(size_t\)(\d+) << 20;", KERNELS_H).group(1)) << 20
    s, n, p = 2 * SLICE + 37, 40_000, 128
    per_hit = 3 * 8 * (9 * TILE + 2)
    needle, hay = white(91, s), unit_noise(92, n)
    hay[20_000:20_000 + s] += np.float32(0.7) * needle
    count = limit // per_hit + 50
    ts = [20_000] + [int(v) for v in np.random.default_rng(93).integers(0, n - s, count - 1)]
    assert len(ts) * per_hit > limit and 100 * per_hit < limit
    algo = am.HipConvolve(needle)
    cp = am.channel_params(p, NOISE_DB)
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        whole = algo.hit_channel_device(buf.ptr, n, peaks_at(am, ts), cp)
        some = list(range(0, 40)) + list(range(len(ts) - 40, len(ts)))
        small = algo.hit_channel_device(buf.ptr, n, peaks_at(am, [ts[i] for i in some]), cp)
        assert [bits(whole[0][i]) for i in some] == [bits(q) for q in small[0]]
        assert whole[1][some].tobytes() == small[1].tobytes()
        assert whole[0][0].main_tap == 0 and abs(whole[1][0][p] - 0.7) < 0.2      # (5 standard errors of 1 / (0.3 sqrt(S)))
    finally:
        buf.free()


# ---- 5. flags -----------------------------------------------------------------------------------------------------------
def test_nonfinite_samples(gpu):
    am = gpu
    s, n, t, p = SLICE + 1, 14_000, 5000, 17
    needle, hay = white(51, s), unit_noise(52, n)
    hay[t:t + s] += np.float32(0.7) * needle
    cp = am.channel_params(p, NOISE_DB)
    algo = am.HipConvolve(needle)
    clean = algo.hit_channel(hay, peaks_at(am, [t]), cp)
    assert clean[0][0].flags == 0
    for u, flagged in ((t - p, True), (t - p - 1, False), (t + s + p - 1, True), (t + s + p, False), (t + 100, True)):
        bad = hay.copy()
        bad[u] = np.nan
        recs, taps = algo.hit_channel(bad, peaks_at(am, [t]), cp)
        if flagged:
            assert recs[0].flags == NONFIN and recs[0].main_tap == 0 and np.isnan(taps).all(), (u - t, recs[0])
        else:
            assert packed(recs, taps) == packed(*clean), (u - t, recs[0])
        ref.assert_record(recs[0], taps[0], ref.channel_ref(bad, needle, t, p, NOISE_DB), u - t)
    nd = needle.copy()
    nd[1234] = np.nan
    recs, taps = am.HipConvolve(nd).hit_channel(hay, peaks_at(am, [t]), cp)
    assert recs[0].flags == NONFIN and np.isnan(taps).all() and np.isnan(recs[0].ncc_eq)


def test_flags(gpu):
    am = gpu
    s, n, t, p = SLICE + 1, 14_000, 5000, 16
    needle = white(61, s)
    cp = am.channel_params(p, NOISE_DB)
    algo = am.HipConvolve(needle)
    live = unit_noise(62, n)
    # a needle of zeros
    zero = am.HipConvolve(np.zeros(s, dtype=np.float32))
    recs, taps = zero.hit_channel(live, peaks_at(am, [t]), cp)
    q = recs[0]
    assert q.flags == EMPTY and (taps == 0).all() and q.ncc == 0.0 and q.ncc_eq == 0.0 and np.isnan(q.gain_db) and q.residual_db == 0.0
    assert q.main_tap == 0 and q.main_share == 0.0
    ref.assert_record(q, taps[0], ref.channel_ref(live, np.zeros(s, dtype=np.float32), t, p, NOISE_DB))
    assert np.isnan(zero.hit_channel(np.zeros(n, dtype=np.float32), peaks_at(am, [t]), cp)[0][0].residual_db)
    # a silent span
    recs, taps = algo.hit_channel(np.zeros(n, dtype=np.float32), peaks_at(am, [t]), cp)
    q = recs[0]
    assert q.flags == BELOW and q.ncc == 0.0 and q.ncc_eq == 0.0 and (taps == 0).all() and np.isnan(q.residual_db) and q.gain_db == -np.inf
    ref.assert_record(q, taps[0], ref.channel_ref(np.zeros(n, dtype=np.float32), needle, t, p, NOISE_DB))
    # a span 70 dB under the needle, the floor at 60; then the floor at 90
    hay = np.zeros(n, dtype=np.float32)
    hay[t:t + s] = needle * np.float32(10 ** -3.5)
    recs, taps = algo.hit_channel(hay, peaks_at(am, [t]), cp)
    q = recs[0]
    assert q.flags == BELOW and q.ncc == 0.0 and q.ncc_eq == 0.0 and abs(q.gain_db + 70) < 0.01 and q.main_tap == 0
    ref.assert_record(q, taps[0], ref.channel_ref(hay, needle, t, p, NOISE_DB))
    keep = am.get_option(am.OPT_SCORE_NORM_FLOOR_DB)
    am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, 90)
    try:
        low, ltaps = algo.hit_channel(hay, peaks_at(am, [t]), cp)
    finally:
        am.set_option(am.OPT_SCORE_NORM_FLOOR_DB, keep)
    ref.assert_record(low[0], ltaps[0], ref.channel_ref(hay, needle, t, p, NOISE_DB, floor_db=90))
    assert low[0].flags == 0 and low[0].ncc > 0.999 and low[0].ncc_eq > 0.999 and ltaps.tobytes() == taps.tobytes()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_errors(gpu):
    L = gpu.lib()
    s, n, p = 5000, 30_000, 4
    needle, hay = white(71, s), unit_noise(72, n)
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    out = (gpu.HitChannel * 4)()
    taps = (C.c_float * (4 * (2 * p + 1)))()
    cp = gpu.channel_params(p)
    cpp = C.byref(cp)
    INV = gpu.AM_ERR_INVALID_ARG
    try:
        # n = 0: AM_OK, nothing launched
        gpu.set_option("profile_mask", -1)
        with gpu.Profile(0) as prof:
            assert _rc(gpu, L.am_hit_channel_device, algo._h, None, n, 0, None, 0, None, None, None)[0] == gpu.AM_OK
            assert _rc(gpu, L.am_hit_channel, algo._h, None, n, 0, None, 0, cpp, None, None)[0] == gpu.AM_OK
            cnt = (C.c_size_t * 1)(0)
            assert _rc(gpu, L.am_hit_channel_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                       (C.c_size_t * 1)(n), 1, 0, None, 4, cnt, None, None, None)[0] == gpu.AM_OK
            assert prof.query("*")[1] == 0
        # ... but the parameters are checked first, whatever n is
        for bad, text in ((gpu.AmChannelParams(129, 0, 60.0), "AM_CHAN_MAX_RADIUS"), (gpu.AmChannelParams(p, 1, 60.0), "reserved"),
                          (gpu.AmChannelParams(p, 0, -1.0), "noise_db"), (gpu.AmChannelParams(p, 0, 201.0), "noise_db"),
                          (gpu.AmChannelParams(p, 0, float("nan")), "noise_db")):
            for count in (0, 1):
                rc, msg = _rc(gpu, L.am_hit_channel_device, algo._h, buf.ptr, n, 0, pk, count, C.byref(bad), out, taps)
                assert rc == INV and text in msg, msg
            rc, msg = _rc(gpu, L.am_hit_channel, algo._h, hay.ctypes.data, n, 0, pk, 1, C.byref(bad), out, taps)
            assert rc == INV and text in msg, msg
        for fn, src in ((L.am_hit_channel_device, buf.ptr), (L.am_hit_channel, hay.ctypes.data)):
            for args in ((algo._h, None, n, 0, pk, 1, cpp, out, taps), (algo._h, src, n, 0, None, 1, cpp, out, taps),
                         (algo._h, src, n, 0, pk, 1, cpp, None, taps), (algo._h, src, n, 0, pk, 1, None, out, taps),
                         (algo._h, src, n, 0, pk, 1, cpp, out, None)):
                rc, msg = _rc(gpu, fn, *args)
                assert rc == INV and "null" in msg, msg
            assert _rc(gpu, fn, None, src, n, 0, pk, 1, cpp, out, taps)[0] == INV
            rc, msg = _rc(gpu, fn, algo._h, src, n, 2, pk, 1, cpp, out, taps)
            assert rc == INV and "format" in msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 2, cpp, out, taps)
            assert rc == INV and "hit 1" in msg and "haystack length" in msg
        rc, msg = _rc(gpu, L.am_hit_channel_device, algo._h, hay.ctypes.data, n, 0, pk, 1, cpp, out, taps)   # host memory
        assert rc == INV and "device" in msg
        # batch: the message names the pair and the hit
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        one = (C.c_void_p * 1)(algo._h)
        rc, msg = _rc(gpu, L.am_hit_channel_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 2), cpp, out, taps)
        assert rc == INV and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_channel_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, hay.ctypes.data),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), cpp, out, taps)
        assert rc == INV and "pair 1" in msg and "device" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_channel_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), cpp, out, None)
        assert rc == INV and "null" in msg
        # A haystack on another device than the needle needs a second GPU; on a one-GPU machine only the host-memory
        # refusal above runs.
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, hay)
            try:
                rc, msg = _rc(gpu, L.am_hit_channel_device, algo._h, other.ptr, n, 0, pk, 1, cpp, out, taps)
                assert rc == INV and "device" in msg
            finally:
                other.free()
        # a good call still works after the refusals, and after am_shutdown (the scratch buffers come back), same bits
        before = algo.hit_channel_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)], cp)
        ref.assert_record(before[0][0], before[1][0], ref.channel_ref(hay, needle, 10, p, 60.0))
    finally:
        buf.free()
    assert packed(*algo.hit_channel(hay, [gpu.Peak(10, 11, 0, 0)], cp)) == packed(*before)
    assert L.am_shutdown() == gpu.AM_OK
    assert packed(*algo.hit_channel(hay, [gpu.Peak(10, 11, 0, 0)], cp)) == packed(*before)
    recs, taps = algo.hit_channel(hay, [], cp)
    assert recs == [] and taps.shape == (0, 2 * p + 1)
