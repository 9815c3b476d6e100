"""GPU tests of the k best matches (include/audiomatch.h, "the k best matches"): am_find_peaks_top equals the first k
peaks of am_find_peaks bit for bit under every peak policy, and am_match_best equals am_find_peaks_top over the
am_correlate_device scores (raw and NCC, f32 and i16 stereo, single and batch, with non-finite samples)."""
import ctypes as C

import numpy as np
import pytest

import policy_cases as pc

pytestmark = pytest.mark.gpu

SR = 8000


def key(r):
    return [(int(q.start), int(q.end), np.float32(q.height).tobytes(), np.float32(q.prominence).tobytes()) for q in r]


class policy_set:
    def __init__(self, gpu, **kw):
        self.gpu, self.kw = gpu, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        for k in ("peak_filter_order", "distance_rule", "score_norm"):
            self.gpu.set_option(k, 0)


def head_of_find_peaks(gpu, y, prom, dist, k):
    """The first k peaks am_find_peaks returns (its full list can be millions long: read only k of them)."""
    a = np.ascontiguousarray(y, dtype=np.float32)
    buf = (gpu.AmPeak * k)()
    n = C.c_size_t(0)
    rc = gpu.lib().am_find_peaks(0, a.ctypes.data, a.size, float(prom), int(dist), buf, k, C.byref(n))
    assert rc in (0, 2), rc          # AM_ERR_CAPACITY: more than k exist, the first k are written
    return [gpu.Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:min(k, n.value)]]


@pytest.mark.parametrize("case", sorted(pc.PEAK_CASES))
def test_top_equals_find_peaks_under_every_policy(gpu, case):
    make, prom, dist = pc.PEAK_CASES[case]
    x = make()
    for order, rule in pc.PEAK_POLICIES:
        with policy_set(gpu, peak_filter_order=order, distance_rule=rule):
            for p, d in ((prom, dist), (0.0, dist), (prom, 0)):
                full = gpu.find_peaks(x, p, d, cap=x.size)
                for k in (1, 3, 17, max(1, len(full))):
                    got = gpu.find_peaks_top(x, k, p, d)
                    assert key(got) == key(full[:k]), (case, order, rule, p, d, k)


def test_white_noise_descent_and_fallback(gpu):
    y = np.random.default_rng(11).standard_normal(1 << 24).astype(np.float32)
    # every maximum survives: one round
    assert key(gpu.find_peaks_top(y, 1000, 0.0, 0)) == key(head_of_find_peaks(gpu, y, 0.0, 0, 1000))
    # a prominence bound and a distance that few maxima pass: the threshold descends
    for prom, dist, k in ((2.5, 0, 1000), (0.0, 16000, 1000)):
        assert key(gpu.find_peaks_top(y, k, prom, dist)) == key(head_of_find_peaks(gpu, y, prom, dist, k)), (prom, dist)
    # k beyond what min_distance allows: the whole-array pick, truncated
    full = gpu.find_peaks(y, 0.0, 10 ** 6, cap=64)
    assert len(full) < 50
    assert key(gpu.find_peaks_top(y, 50, 0.0, 10 ** 6)) == key(full)


def test_plateaus_across_tile_edges(gpu):
    rng = np.random.default_rng(3)
    y = (0.1 * rng.standard_normal(1 << 14)).astype(np.float32)
    for lo, hi, v in ((1020, 1030, 2.0), (2047, 2049, 3.0), (4095, 4096, 1.5), (8190, 8200, 2.5), (3000, 3003, 2.0)):
        y[lo:hi] = v
    y[-5:] = 4.0                        # a plateau that runs to the end: no peak
    for order, rule in pc.PEAK_POLICIES:
        with policy_set(gpu, peak_filter_order=order, distance_rule=rule):
            for d in (0, 5, 1000):
                full = gpu.find_peaks(y, 0.0, d, cap=y.size)
                for k in (1, 4, 50, len(full)):
                    assert key(gpu.find_peaks_top(y, k, 0.0, d)) == key(full[:k]), (order, rule, d, k)


def stretches_of(y):
    fin = np.isfinite(y)
    out, i, n = [], 0, y.size
    while i < n:
        if not fin[i]:
            i += 1
            continue
        j = i
        while j < n and fin[j]:
            j += 1
        out.append((i, j))
        i = j
    return out


def union_top(gpu, y, prom, dist, k, stretches=None):
    """Per finite stretch find_peaks, shifted, ordered by (height desc, start asc), truncated (stretches further apart
    than dist: the distance rule between them is moot)."""
    allp = []
    for a, b in (stretches or stretches_of(y)):
        if b - a >= 3:
            for q in gpu.find_peaks(y[a:b], prom, dist, cap=b - a):
                allp.append(gpu.Peak(q.start + a, q.end + a, q.height, q.prominence))
    allp.sort(key=lambda q: (-np.float32(q.height), q.start))
    return allp[:k]


def test_nonfinite_scores_split_the_array(gpu):
    rng = np.random.default_rng(4)
    y = rng.standard_normal(200000).astype(np.float32)
    y[5000:7000] = np.nan
    y[50000:52000] = np.inf
    y[120000:121500] = -np.inf
    y[7000] = 9.0                       # first score of a stretch: no peak
    y[4999] = 9.0                       # last score of a stretch: no peak
    for k in (1, 10, 300):
        assert key(gpu.find_peaks_top(y, k, 0.0, 1000)) == key(union_top(gpu, y, 0.0, 1000, k))
        assert key(gpu.find_peaks_top(y, k, 1.0, 0)) == key(union_top(gpu, y, 1.0, 0, k))


# ---------------------------------------------------------------------------
def planted(seed, seconds, S, gains, level=None):
    rng = np.random.default_rng(seed)
    n = seconds * SR
    needle = rng.uniform(-0.5, 0.5, S).astype(np.float32)
    hay = rng.uniform(-0.25, 0.25, n).astype(np.float32)
    # one plant per slot of 4 S (its region [t - S, t + 2 S) inside the slot)
    offs = sorted(rng.choice(np.arange(n // (4 * S)), size=len(gains), replace=False) * 4 * S + S + rng.integers(0, S, len(gains)))
    for t, g in zip(offs, gains):
        hay[t:t + S] += np.float32(g) * needle
    if level is not None:               # the same SNR everywhere, the level of each region scaled
        for t, lv in zip(offs, level):
            hay[max(0, t - S):t + 2 * S] *= np.float32(lv)
    return needle, hay, [int(t) for t in offs]


def test_match_best_equals_top_of_correlate_and_checker(gpu, oracle):
    S = SR // 2
    for seed, secs in ((1, 60), (2, 120)):
        gains = [0.9, 0.5, 1.3, 0.7, 1.1]
        needle, hay, offs = planted(seed, secs, S, gains)
        algo = gpu.HipConvolve(needle)
        got = algo.match_best(hay, 3, min_distance=S)
        scores = algo.correlate_with_sample(hay, gpu.Mode.Valid, scale=True)
        assert key(got) == key(gpu.find_peaks_top(scores, 3, 0.0, S))
        loud = sorted(offs[i] for i in np.argsort(gains)[::-1][:3])
        assert sorted(q.start for q in got) == loud
        ref = oracle.find_peaks(oracle.correlate(hay, needle, oracle.MODE_VALID, oracle.SCALE_LIB), 0.0, S)[:3]
        assert [q.start for q in got] == [r[0] for r in ref]
        assert np.allclose([q.height for q in got], [r[2] for r in ref], atol=1e-4)
        algo.close()


def test_match_best_ncc_ranks_every_plant_on_top(gpu):
    S = SR // 2
    needle, hay, offs = planted(5, 90, S, [0.5] * 5, level=[1.0, 0.1, 3.0, 0.3, 0.03])
    raw = gpu.HipConvolve(needle, score_norm=False)
    ncc = gpu.HipConvolve(needle, score_norm=True)
    got = ncc.match_best(hay, 5, min_distance=S)
    assert sorted(q.start for q in got) == offs
    scores = ncc.correlate_with_sample(hay, gpu.Mode.Valid, scale=True)
    assert key(got) == key(gpu.find_peaks_top(scores, 5, 0.0, S))
    assert sorted(q.start for q in raw.match_best(hay, 5, min_distance=S)) != offs   # raw scores follow the level
    raw.close(); ncc.close()


def test_pcm16_equals_f32_on_the_downmix(gpu):
    S = SR // 2
    rng = np.random.default_rng(8)
    needle, hay, offs = planted(8, 60, S, [0.9, 0.6, 1.2])
    st = np.stack([hay * 20000, hay * 20000 + rng.normal(0, 300, hay.size)], axis=1).clip(-32768, 32767).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(st)
    for norm in (False, True):
        algo = gpu.HipConvolve(needle, score_norm=norm)
        assert key(algo.match_best(st, 3, S)) == key(algo.match_best(mono, 3, S))
        algo.close()


def test_batch_equals_singles(gpu):
    S = SR // 2
    needle, _, _ = planted(9, 10, S, [1.0])
    hays = [planted(20 + i, secs, S, [0.8, 1.1, 0.6])[1] for i, secs in enumerate((60, 7, 95, 12))]
    hays[3] = hays[3][:S - 10]          # shorter than the needle: no hit
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    for norm in (False, True):
        algo = gpu.HipConvolve(needle, score_norm=norm)
        bp = gpu.best_params(4, S)
        batch = algo.match_best_batch_device([b.ptr for b in bufs], [h.size for h in hays], bp)
        singles = [algo.match_best_device(b.ptr, h.size, bp) for b, h in zip(bufs, hays)]
        assert [key(r) for r in batch] == [key(r) for r in singles]
        assert singles[3] == [] and len(singles[0]) == 4
        algo.close()


def test_nonfinite_samples_cost_their_windows(gpu):
    S = SR // 2
    needle, hay, offs = planted(12, 60, S, [0.9, 0.6, 1.2, 0.8, 1.0])
    hay[100000:100010] = np.nan
    hay[300000] = np.inf
    algo = gpu.HipConvolve(needle)
    got = algo.match_best(hay, 20, min_distance=S // 2)
    sample_stretches = stretches_of(hay)
    score_stretches = [(a, b - S + 1) for a, b in sample_stretches if b - a >= S]
    n = hay.size - S + 1
    scores = np.full(n, np.nan, dtype=np.float32)
    for a, b in sample_stretches:
        if b - a >= S:
            scores[a:b - S + 1] = algo.correlate_with_sample(hay[a:b], gpu.Mode.Valid, scale=True)
    assert key(got) == key(union_top(gpu, scores, 0.0, S // 2, 20, score_stretches))
    for q in got:
        assert np.all(np.isfinite(hay[q.start:q.start + S]))
    algo.close()


def test_edges_and_errors(gpu):
    S = SR // 2
    needle, hay, _ = planted(13, 5, S, [1.0])
    algo = gpu.HipConvolve(needle)
    few = algo.match_best(hay[:S + 3], 10)
    assert 0 < len(few) < 10                               # k beyond the peaks that exist: not an error
    assert algo.match_best(hay[:S - 1], 3) == []           # shorter than the needle
    for bad in (dict(k=0), dict(k=3, scale=gpu.Scale.MY)):
        with pytest.raises(gpu.AudioMatchError) as e:
            algo.match_best(hay, **bad)
        assert e.value.code == 1
    bp = gpu.best_params(3)
    n = C.c_size_t(0)
    out = (gpu.AmPeak * 3)()
    assert gpu.lib().am_match_best(algo._h, None, hay.size, 0, C.byref(bp), out, C.byref(n)) == 1
    assert gpu.lib().am_match_best(algo._h, hay.ctypes.data, hay.size, 0, None, out, C.byref(n)) == 1
    assert gpu.lib().am_match_best(algo._h, hay.ctypes.data, hay.size, 0, C.byref(bp), None, C.byref(n)) == 1
    assert gpu.lib().am_find_peaks_top(0, hay.ctypes.data, hay.size, 0.0, 0, 0, out, C.byref(n)) == 1
    assert gpu.lib().am_find_peaks_top(0, None, hay.size, 0.0, 0, 3, out, C.byref(n)) == 1
    with pytest.raises(gpu.AudioMatchError):
        gpu.HipConvolve(needle, score_norm=True).match_best(hay, 3, scale=gpu.Scale.NONE)
    algo.close()


def test_full_size_hour(gpu):
    """1 h at 44.1 kHz, a 10 s needle, 8 plants, k = 8, min_distance = S: the offsets are the plants."""
    sr, S = 44100, 441000
    H = 3600 * sr
    needle = gpu.synth_uniform_device(0, S, seed=7, stream=0)
    hay = gpu.synth_uniform_device(0, H, seed=7, stream=1)
    plants = [int(t) for t in np.linspace(3 * S, H - 3 * S, 8).astype(np.int64) + np.arange(8) * 977]
    for t in plants:
        gpu.axpy_device(0, hay, t, needle.ptr, S, 1.0)
    algo = gpu.HipConvolve.from_device(0, needle.ptr, S)
    got = algo.match_best_device(hay.ptr, H, gpu.best_params(8, S))
    assert sorted(q.start for q in got) == plants
    algo.close()
