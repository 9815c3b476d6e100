"""Window-energy normalised scores (option "score_norm", NCC) against an f64 numpy checker:
ncc(t) = corr(t) / sqrt(sum(needle^2) * sum(window^2)), 0 for windows more than the floor below the needle."""
import ctypes as C

import numpy as np
import pytest

from score_norm_ref import assert_peaks, bits, chunks, match_ref, ncc_ref, overshadow_filter  # noqa: F401

pytestmark = pytest.mark.gpu

SR = 8000
UNSUPPORTED = "score_norm: not supported by this entry point"


@pytest.fixture
def opts(gpu):
    """Process options set by a test, restored afterwards."""
    keep = {}

    def set_(key, value):
        keep.setdefault(key, gpu.get_option(key))
        gpu.set_option(key, value)
    yield set_
    for k, v in keep.items():
        gpu.set_option(k, v)


def noise(oracle, stream, n, amp=0.25):
    return oracle.synth_uniform(11, stream, 0, n, amp)


def level_hay(oracle, n, regions, plants, needle, stream=3):
    """Noise whose regions [a, b) are scaled by g (a recording at another level), plants (offset, gain)."""
    hay = noise(oracle, stream, n).astype(np.float32)
    for a, b, g in regions:
        hay[a:b] *= np.float32(g)
    for off, g in plants:
        hay[off:off + len(needle)] += np.float32(g) * needle
    return hay


def params(gpu, chunk_s=20.0, overlap_s=1.0, dist_s=5.0, prom=0.13):
    return gpu.Config(chunk_size_s=chunk_s, overlap_length_s=overlap_s, distance_s=dist_s, prominence=prom).params(SR, gpu.Scale.LIB)


# ---- 1. level 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [3, 64, 1000, 40000])
def test_level1_against_checker(gpu, oracle, s):
    rng = np.random.default_rng(s)
    needle = rng.uniform(-1, 1, s).astype(np.float32)
    w = 3 * s + 20000
    within = rng.uniform(-1, 1, w).astype(np.float32)
    within[w // 3:w // 3 + 2 * s + 5000] = 0.0          # a stretch of exact zeros, longer than a window
    within[-s // 2 - 100:] *= np.float32(1e-4)          # and a quiet end (-80 dB)
    algo = gpu.HipConvolve(needle, score_norm=True)
    got_self = algo.correlate_with_sample(needle, gpu.Mode.Valid, True)
    assert abs(float(got_self[0]) - 1.0) <= 1e-6
    for mode in (gpu.Mode.Full, gpu.Mode.Same, gpu.Mode.Valid):
        got = algo.correlate_with_sample(within, mode, True).astype(np.float64)
        exp, ew, thr = ncc_ref(oracle, within, needle, int(mode))
        assert got.shape == exp.shape and np.all(np.isfinite(got))
        above, below = ew >= thr * (1 + 1e-9), ew < thr * (1 - 1e-9)
        assert np.max(np.abs(got[above] - exp[above])) <= 2e-5, (mode, np.max(np.abs(got[above] - exp[above])))
        assert np.all(got[below] == 0.0), mode
        assert below.any() and above.any()


# ---- 2. gain invariance --------------------------------------------------------------------------------------------
def test_gain_invariance(gpu, oracle):
    needle = noise(oracle, 1, SR)
    base = level_hay(oracle, 30 * SR, [], [(12 * SR + 77, 1.0)], needle)   # one recording: noise and a plant ...
    gains = (0.05, 1.0, 4.0)
    hay = np.concatenate([np.float32(g) * base for g in gains])           # ... at three levels
    plants = [(k * 30 * SR + 12 * SR + 77, g) for k, g in enumerate(gains)]
    p = params(gpu, chunk_s=30.0, dist_s=5.0)
    got = gpu.HipConvolve(needle, score_norm=True).match(hay, p)
    assert [g.start for g in got] == [o for o, _ in plants]
    hs = [g.height for g in got]
    assert max(hs) - min(hs) <= 1e-4, hs
    lib = gpu.HipConvolve(needle).match(hay, p)
    assert plants[0][0] not in [g.start for g in lib]     # LIB scores the quiet plant by the level: missed


# ---- 3. level 2 ----------------------------------------------------------------------------------------------------
def level2_case(oracle, needle):
    n = 600 * SR + 17 * SR + 123                       # a short last window
    regions = [(100 * SR, 200 * SR, 0.05), (380 * SR, 420 * SR, 4.0), (300 * SR, 320 * SR, 0.0)]
    plants = [(30 * SR + 11, 1.0), (150 * SR + 4000, 0.05), (400 * SR + 17, 4.0), (500 * SR, 0.3), (610 * SR + 3, 1.0)]
    hay = level_hay(oracle, n, regions, plants, needle)
    hay[250 * SR:260 * SR] = noise(oracle, 9, 10 * SR, amp=1.0)   # a loud, uncorrelated burst
    return hay


@pytest.mark.parametrize("tail_block,tail_window", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_level2_against_checker(gpu, oracle, opts, tail_block, tail_window):
    needle = noise(oracle, 1, SR)
    hay = level2_case(oracle, needle)
    opts("tail_block", tail_block)
    opts("tail_window", tail_window)
    p = params(gpu, chunk_s=60.0)
    exp = match_ref(oracle, hay, needle, p, tail_window=tail_window)
    got = gpu.HipConvolve(needle, score_norm=True).match(hay, p)
    assert_peaks(got, exp)
    assert 610 * SR + 3 in [g.start for g in got] or tail_window   # (the plant in the short last window)


# ---- 4. floor ------------------------------------------------------------------------------------------------------
def test_floor(gpu, oracle, opts):
    needle = noise(oracle, 1, SR)
    g = 10.0 ** (-70 / 20)
    n = 60 * SR
    hay = level_hay(oracle, n, [(8 * SR, 52 * SR, g)], [(30 * SR + 9, g)], needle)   # 44 s quiet: longer than a block
    p = params(gpu, chunk_s=20.0)
    algo = gpu.HipConvolve(needle, score_norm=True)
    algo.set_option("log_n", 16)   # (blocks of 2^16 points: the quiet region spans several)
    assert 30 * SR + 9 not in [q.start for q in algo.match(hay, p)]
    y = algo.correlate_with_sample(hay[25 * SR:36 * SR], gpu.Mode.Valid, True)
    assert np.all(y[: 20 * SR] == 0.0)
    opts("score_norm_floor_db", 80)
    got = algo.match(hay, p)
    assert 30 * SR + 9 in [q.start for q in got]
    assert_peaks(got, match_ref(oracle, hay, needle, p, floor_db=80), tol=1e-3)


# ---- 5. NaN --------------------------------------------------------------------------------------------------------
def test_nan_costs_its_windows(gpu, oracle):
    needle = noise(oracle, 1, SR)
    n = 120 * SR
    hay = level_hay(oracle, n, [(60 * SR, n, 0.1)], [(15 * SR, 1.0), (45 * SR, 1.0), (75 * SR, 0.1), (105 * SR, 0.1)], needle)
    hay[44 * SR + 5] = np.nan
    p = params(gpu, chunk_s=20.0)
    got = gpu.HipConvolve(needle, score_norm=True).match(hay, p)
    exp = match_ref(oracle, hay, needle, p)
    assert_peaks(got, exp)
    assert 45 * SR not in [q.start for q in got] and 15 * SR in [q.start for q in got]


# ---- 6. consistency ------------------------------------------------------------------------------------------------
def test_batch_pcm16_pool_bit_identical(gpu, oracle, opts):
    needle = noise(oracle, 1, SR)
    p = params(gpu, chunk_s=20.0)
    hays = [level_hay(oracle, (40 + 13 * k) * SR + 31 * k, [(5 * SR, 30 * SR, 0.05 * (k + 1))], [(10 * SR + k, 0.05 * (k + 1)), (33 * SR, 1.0)],
                      needle, stream=20 + k) for k in range(5)]
    algo = gpu.HipConvolve(needle, score_norm=True)
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        batch = algo.match_batch_device([b.ptr for b in bufs], [h.size for h in hays], p)
        single = [algo.match_device(b.ptr, h.size, p) for b, h in zip(bufs, hays)]
        assert [bits(x) for x in batch] == [bits(x) for x in single]
        assert all(len(x) >= 2 for x in batch)
        opts("score_norm", 1)   # (pool needles follow the process default)
        pool = gpu.Pool(needle, devices=[0, 0])
        try:
            pooled = pool.match_batch(hays, p)
        finally:
            pool.close()
        assert [bits(x) for x in pooled] == [bits(x) for x in batch]
    finally:
        for b in bufs:
            b.free()
    rng = np.random.default_rng(4)
    lr = np.clip(rng.normal(0, 3000, size=2 * 50 * SR), -32768, 32767).astype(np.int16)
    lr[2 * 20 * SR:2 * 60 * SR:] //= 16
    mono = gpu.pcm_s16_stereo_to_mono(lr)
    got16 = algo.match_pcm16(lr, p)
    got32 = algo.match(mono, p)
    assert bits(got16) == bits(got32)


# ---- 7. no state leak ----------------------------------------------------------------------------------------------
def test_no_state_leak(gpu, oracle):
    needle = noise(oracle, 1, SR)
    hay = level2_case(oracle, needle)[: 200 * SR]
    p = params(gpu, chunk_s=60.0)
    algo = gpu.HipConvolve(needle)
    lib1 = algo.match(hay, p)
    algo.set_option("score_norm", 1)
    ncc = algo.match(hay, p)
    algo.set_option("score_norm", -1)
    lib2 = algo.match(hay, p)
    fresh = gpu.HipConvolve(needle).match(hay, p)
    assert bits(lib1) == bits(lib2) == bits(fresh)
    assert bits(ncc) != bits(lib1)
    assert gpu.get_option("score_norm") == 0 and algo.get_option("score_norm") == -1
    assert gpu.calc_chunks(SR, hay, algo, True, gpu.Config(chunk_size_s=60.0, overlap_length_s=1.0, distance_s=5.0), ncc=True)
    assert algo.get_option("score_norm") == -1


# ---- 8. errors -----------------------------------------------------------------------------------------------------
def _code(fn):
    import audiomatch_amd as am
    with pytest.raises(am.AudioMatchError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_errors(gpu, oracle, opts):
    INV = 1
    needle = noise(oracle, 1, SR)
    hay = noise(oracle, 2, 30 * SR)
    algo = gpu.HipConvolve(needle, score_norm=True)
    for sc in (gpu.Scale.NONE, gpu.Scale.MY):
        assert _code(lambda: algo.correlate_with_sample(hay, gpu.Mode.Valid, sc))[0] == INV
        assert _code(lambda: algo.match(hay, gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0).params(SR, sc)))[0] == INV
    p = params(gpu, chunk_s=10.0)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        calls = [
            lambda: gpu.match_multi_device([algo, algo], buf.ptr, hay.size, p),
            lambda: gpu.match_multi_batch_device([algo, algo], [buf.ptr], [hay.size], p),
            lambda: gpu.MatchStream(algo, p),
            lambda: gpu.match_part_device(algo, buf.ptr, hay.size, p, 1, 0),
        ]
        for fn in calls:
            code, msg = _code(fn)
            assert code == INV and UNSUPPORTED in msg, msg
        opts("score_norm", 1)
        pool = gpu.Pool(needle, devices=[0])
        try:
            code, msg = _code(lambda: pool.match_long(hay, p))
            assert code == INV and UNSUPPORTED in msg
            code, msg = _code(lambda: pool.match_long_device([buf.ptr], hay.size, p))
            assert code == INV and UNSUPPORTED in msg
        finally:
            pool.close()
        mp = gpu.MultiPool([needle, needle], devices=[0])
        try:
            code, msg = _code(lambda: mp.match_batch([hay], p))
            assert code == INV and UNSUPPORTED in msg
        finally:
            mp.close()
    finally:
        buf.free()
    for key, v in (("score_norm", 2), ("score_norm", -1), ("score_norm_floor_db", -1), ("score_norm_floor_db", 201)):
        assert _code(lambda: gpu.set_option(key, v))[0] == INV
    assert _code(lambda: algo.set_option("score_norm", 2))[0] == INV
    assert gpu.get_option("score_norm_floor_db") == 60


# ---- 9. half pipeline ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [1, 2])
def test_half_pipeline_offsets(gpu, oracle, half):
    needle = noise(oracle, 1, SR)
    hay = level2_case(oracle, needle)
    p = params(gpu, chunk_s=60.0)
    f32 = gpu.HipConvolve(needle, score_norm=True).match(hay, p)
    algo = gpu.HipConvolve(needle, score_norm=True)
    algo.set_option("half_pipeline", half)
    got = algo.match(hay, p)
    assert [(q.start, q.end) for q in got] == [(q.start, q.end) for q in f32]
    tol = 2e-4 if half == 1 else 3e-3
    assert all(abs(a.height - b.height) <= tol for a, b in zip(got, f32))


# ---- 10. full size -------------------------------------------------------------------------------------------------
def test_full_size_levels(gpu, oracle):
    sr = 44100
    n = 3600 * sr
    s = 10 * sr
    needle = oracle.synth_uniform(5, 0, 0, s)
    d_needle = gpu.DeviceBuffer.from_numpy(0, needle)
    hay = gpu.synth_uniform_device(0, n, seed=5, stream=1)
    try:
        regions = [(5 * 60 * sr, 15 * 60 * sr, 10 ** (-26 / 20)), (40 * 60 * sr, 50 * 60 * sr, 10 ** (6 / 20))]
        plants = [(10 * 60 * sr + 20 * sr + 7, regions[0][2]), (30 * 60 * sr + 25 * sr + 1, 1.0), (45 * 60 * sr + 15 * sr + 3, regions[1][2])]
        for a, b, g in regions:   # the region as recorded at another level: noise scaled in place
            gpu.axpy_device(0, hay, a, hay.ptr + 4 * a, b - a, g - 1.0)
        for off, g in plants:
            gpu.axpy_device(0, hay, off, d_needle.ptr, s, g)
        cfg = gpu.Config(overlap_length_s=10.0)
        p = cfg.params(sr, gpu.Scale.LIB)
        got = gpu.HipConvolve(needle, score_norm=True).match_device(hay.ptr, n, p)
        assert [q.start for q in got] == [o for o, _ in plants]
        # the checker on the chunks that hold the plants and two others
        win = p.chunk + p.overlap
        for q in got:
            off = (q.start // p.chunk) * p.chunk
            seg = np.empty(win, dtype=np.float32)
            gpu._check(gpu.lib().am_memcpy_d2h(0, seg.ctypes.data, C.c_void_p(hay.ptr + 4 * off), 4 * win))
            y, _, _ = ncc_ref(oracle, seg, needle, oracle.MODE_VALID)
            pk = oracle.find_peaks(y.astype(np.float32), p.min_prominence, p.min_distance)
            assert [a + off for a, _, _, _ in pk] == [q.start]
            assert abs(pk[0][2] - q.height) <= 1e-3
        for off in (0, 20 * p.chunk):
            seg = np.empty(win, dtype=np.float32)
            gpu._check(gpu.lib().am_memcpy_d2h(0, seg.ctypes.data, C.c_void_p(hay.ptr + 4 * off), 4 * win))
            y, _, _ = ncc_ref(oracle, seg, needle, oracle.MODE_VALID)
            assert oracle.find_peaks(y.astype(np.float32), p.min_prominence, p.min_distance) == []
    finally:
        hay.free()
        d_needle.free()
