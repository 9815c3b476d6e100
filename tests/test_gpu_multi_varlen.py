"""Several needles of different lengths in one call (am_match_multi_varlen_batch_device, am_match_multi_varlen): every
(haystack, needle) pair equals one am_match_device / am_match_pcm16_device call with that needle's own overlap, and the
checker; needles of one length give am_match_multi_batch_device's results bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
PROM = 0.3


def params_with(gpu, p, overlap):
    q = gpu.AmMatchParams.from_buffer_copy(p)
    q.overlap = int(overlap)
    return q


def peaks(r):
    return [(g.start, g.end) for g in r]


def assert_close(got, one, tol=TOL):
    assert peaks(got) == peaks(one)
    for g, o in zip(got, one):
        assert abs(g.height - o.height) < tol and abs(g.prominence - o.prominence) < tol


def singles(gpu, algos, bufs, lens, p, overlaps=None, pcm=False):
    """[k][j]: one single-needle call per pair, with needle j's overlap"""
    out = []
    for b, n in zip(bufs, lens):
        row = []
        for j, a in enumerate(algos):
            q = p if overlaps is None else params_with(gpu, p, overlaps[j])
            row.append(a.match_pcm16_device(b.ptr, n, q) if pcm else a.match_device(b.ptr, n, q))
        out.append(row)
    return out


SR8 = 8000
# 0.5 / 1.3 / 2 / 3.7 s and a length one sample past 1 s
LENS8 = [4000, 10400, 16000, 29600, 8001]


def small_set(oracle):
    """Five needles of different lengths at 8 kHz against three haystacks: 100 s and 70 s (the 2^21 plan: grouped K3),
    3 s (shorter than the longest needle).  Every needle is planted once in the middle and once within S_max of the
    haystack's end, where zero-padding every needle to the longest would lose it."""
    needles = [oracle.synth_uniform(41, 100 + j, 0, s) for j, s in enumerate(LENS8)]
    smax = max(LENS8)
    hays, plants = [], []
    for k, n in enumerate((100 * SR8 + 123, 70 * SR8 + 5, 3 * SR8)):
        h = oracle.synth_uniform(41, 1 + k, 0, n)
        pk = []
        for j, nd in enumerate(needles):
            offs = []
            if n >= 20 * SR8:
                # (the first well inside a window for every overlap used below, the second within S_max of the end)
                offs = [(1 + j) * 10 * SR8 + 2 * SR8 + 17 * k, n - len(nd) - 300 * (j + 1)]
                assert offs[1] + len(nd) > n - smax
            elif len(nd) <= n // 2:
                offs = [n - len(nd) - 50]
            for o in offs:
                h[o:o + len(nd)] += nd
            pk.append(sorted(offs))
        hays.append(h)
        plants.append(pk)
    return needles, hays, plants


def test_varlen_equals_single_calls_and_checker(gpu, oracle):
    needles, hays, plants = small_set(oracle)
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=PROM).params(SR8, gpu.Scale.LIB)
    algos = [gpu.HipConvolve(n) for n in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    lens = [h.size for h in hays]
    try:
        for overlaps in (None, [s // 3 for s in LENS8], [2 * s + 7 for s in LENS8]):
            one = singles(gpu, algos, bufs, lens, p, overlaps)
            for k in range(3):
                for j in range(len(needles)):
                    ov = p.overlap if overlaps is None else overlaps[j]
                    exp = oracle.calc_chunks(SR8, hays[k], needles[j], p.chunk, ov, PROM, p.min_distance, 5.0)
                    # (a hit found by two overlapping windows with equal prominence is reported twice, as the reference does)
                    assert sorted(set(e[0] for e in exp)) == plants[k][j], (k, j)
                    assert [g.start for g in one[k][j]] == [e[0] for e in exp]
            for _ in range(2):   # (the second round on the sparse-score path)
                res = gpu.match_multi_varlen_batch_device(algos, [b.ptr for b in bufs], lens, p, overlaps=overlaps)
                for k in range(3):
                    for j in range(len(needles)):
                        assert_close(res[k][j], one[k][j])
            # the host form, haystack by haystack
            for k in range(3):
                res = gpu.match_multi_varlen(algos, hays[k], p, overlaps=overlaps)
                for j in range(len(needles)):
                    assert_close(res[j], one[k][j])
        # groupings, grouped K3 and grouped picks on and off: the same offsets
        one = singles(gpu, algos, bufs, lens, p)
        for group, k3g, pickg in ((1, 1, 1), (3, 1, 1), (3, 1, 0), (3, 0, 1), (8, 1, 0), (8, 0, 0), (8, 1, 1)):
            gpu.set_option("needle_group", group)
            gpu.set_option("k3_group", k3g)
            gpu.set_option("pick_group", pickg)
            res = gpu.match_multi_varlen_batch_device(algos, [b.ptr for b in bufs], lens, p)
            for k in range(3):
                for j in range(len(needles)):
                    assert_close(res[k][j], one[k][j])
    finally:
        gpu.set_option("needle_group", 8)
        gpu.set_option("k3_group", 1)
        gpu.set_option("pick_group", 1)


def test_varlen_pcm16_and_half_pipeline(gpu, oracle):
    needles, hays, plants = small_set(oracle)
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=PROM).params(SR8, gpu.Scale.LIB)
    rng = np.random.default_rng(5)
    # i16 stereo: needles and haystacks as frames; the checker is am_match_pcm16_device
    n_lr = [rng.integers(-9000, 9000, size=2 * s).astype(np.int16) for s in LENS8]
    h_lr = []
    for k, h in enumerate(hays):
        x = rng.integers(-9000, 9000, size=2 * h.size).astype(np.int32)
        for j, offs in enumerate(plants[k]):
            for o in offs:
                x[2 * o:2 * (o + LENS8[j])] += n_lr[j]
        h_lr.append(np.clip(x, -32768, 32767).astype(np.int16))
    algos = [gpu.HipConvolve.from_pcm16(x) for x in n_lr]
    bufs = [gpu.DeviceBuffer.from_numpy(0, x) for x in h_lr]
    lens = [x.size // 2 for x in h_lr]
    one = singles(gpu, algos, bufs, lens, p, pcm=True)
    for k in range(3):
        for j in range(len(algos)):
            assert [g.start for g in one[k][j]] == plants[k][j]
    res = gpu.match_multi_varlen_batch_device(algos, [b.ptr for b in bufs], lens, p, fmt=gpu.Fmt.S16_STEREO)
    for k in range(3):
        for j in range(len(algos)):
            assert_close(res[k][j], one[k][j])
    res = gpu.match_multi_varlen(algos, h_lr[0], p)
    for j in range(len(algos)):
        assert_close(res[j], one[0][j])
    # half_pipeline 1 and 2: the offsets of the f32 path
    f_algos = [gpu.HipConvolve(n) for n in needles]
    f_bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    f_lens = [h.size for h in hays]
    ref = gpu.match_multi_varlen_batch_device(f_algos, [b.ptr for b in f_bufs], f_lens, p)
    try:
        for level in (1, 2):
            gpu.set_option("half_pipeline", level)
            res = gpu.match_multi_varlen_batch_device(f_algos, [b.ptr for b in f_bufs], f_lens, p)
            for k in range(3):
                for j in range(len(f_algos)):
                    assert peaks(res[k][j]) == peaks(ref[k][j]), (level, k, j)
    finally:
        gpu.set_option("half_pipeline", 0)


def test_varlen_nonfinite_costs_only_that_needles_windows(gpu, oracle):
    """A NaN inside the first window of the long needle but outside the first window of the short one (overlap = each
    needle's own length, as the CLI sets it; window i of needle j = samples [i chunk, i chunk + chunk + S_j)): each pair
    loses only its own windows -- the long needle its hit at 2 s, the short one keeps its hit at 4 s."""
    sr = SR8
    s_short, s_long = 4000, 29600
    needles = [oracle.synth_uniform(43, 200, 0, s_short), oracle.synth_uniform(43, 201, 0, s_long)]
    hay = oracle.synth_uniform(43, 1, 0, 100 * sr)
    for o in (4 * sr, 14 * sr, 55 * sr):
        hay[o:o + s_short] += needles[0]
    for o in (2 * sr, 16 * sr, 61 * sr):
        hay[o:o + s_long] += needles[1]
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=PROM).params(sr, gpu.Scale.LIB)
    overlaps = [s_short, s_long]
    nan_at = 95000
    assert p.chunk + s_short <= nan_at < p.chunk + s_long
    bad = hay.copy()
    bad[nan_at] = np.nan
    algos = [gpu.HipConvolve(n) for n in needles]
    b = gpu.DeviceBuffer.from_numpy(0, bad)
    one = singles(gpu, algos, [b], [bad.size], p, overlaps)
    for _ in range(2):
        res = gpu.match_multi_varlen_batch_device(algos, [b.ptr], [bad.size], p, overlaps=overlaps)
        for j in range(2):
            exp = oracle.calc_chunks(sr, bad, needles[j], p.chunk, overlaps[j], PROM, p.min_distance, 5.0)
            assert [g.start for g in res[0][j]] == [e[0] for e in exp] == [g.start for g in one[0][j]]
            assert_close(res[0][j], one[0][j])
    assert [g.start for g in res[0][0]] == [4 * sr, 55 * sr]    # the short needle keeps its first window's hit
    assert [g.start for g in res[0][1]] == [61 * sr]             # the long needle's first two windows hold the NaN


def test_varlen_odd_last_block_and_full_size(gpu, oracle):
    """44.1 kHz: 32 needles of 3-12 s (seeded lengths) against a 1 h haystack, and a shorter haystack whose main
    layout has an odd last block (the tail block on the 2^21 plan) -- every pair equals its single call."""
    sr = 44100
    rng = np.random.default_rng(808)
    lens_n = [int(x) for x in rng.integers(3 * sr, 12 * sr + 1, size=32)]
    lens_n[0] = 12 * sr
    needles = [oracle.synth_uniform(47, 300 + j, 0, s) for j, s in enumerate(lens_n)]
    s_min, s_max = min(lens_n), max(lens_n)
    hop = ((1 << 22) - s_max + 1) // 1024 * 1024
    hays = [oracle.synth_uniform(47, 1, 0, 3600 * sr), oracle.synth_uniform(47, 2, 0, 2 * hop + 1500000 + s_min - 1)]
    plants = []
    for k, h in enumerate(hays):
        pk = []
        for j, nd in enumerate(needles):
            offs = [((20 + 97 * j + 13 * k) * sr + 12345) % (h.size - 2 * s_max), h.size - len(nd) - 1000 * (j + 1)]
            for o in offs:
                h[o:o + len(nd)] += nd
            pk.append(sorted(offs))
        plants.append(pk)
    p = gpu.Config(chunk_size_s=60.0, overlap_length_s=10.0, distance_s=2.0, prominence=0.3).params(sr, gpu.Scale.LIB)
    algos = [gpu.HipConvolve(n) for n in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    lens = [h.size for h in hays]
    overlaps = lens_n   # (each needle's own length, as the CLI sets it: no gaps between windows)
    try:
        one = singles(gpu, algos, bufs, lens, p, overlaps)
        for k in range(2):
            for j in range(len(needles)):
                assert [g.start for g in one[k][j]] == plants[k][j], (k, j)
        for on in (1, 0):
            gpu.set_option("tail_block", on)
            res = gpu.match_multi_varlen_batch_device(algos, [b.ptr for b in bufs], lens, p, overlaps=overlaps)
            for k in range(2):
                for j in range(len(needles)):
                    assert_close(res[k][j], one[k][j])
    finally:
        gpu.set_option("tail_block", 1)
        for a in algos:
            a.close()


def test_varlen_equal_lengths_bit_identical(gpu, oracle):
    sr = SR8
    s = 12000
    needles = [oracle.synth_uniform(49, 400 + j, 0, s) for j in range(5)]
    hays = [oracle.synth_uniform(49, 1 + k, 0, n) for k, n in enumerate((90 * sr, 41 * sr + 7))]
    for k, h in enumerate(hays):
        for j, nd in enumerate(needles):
            o = (3 + 7 * j + k) * sr + sr // 2
            h[o:o + s] += nd
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=5.0, prominence=PROM).params(sr, gpu.Scale.LIB)
    algos = [gpu.HipConvolve(n) for n in needles]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    lens = [h.size for h in hays]
    key = lambda r: [[[(g.start, g.end, g.height, g.prominence) for g in r[k][j]] for j in range(5)] for k in range(2)]
    for fmt_overlaps in (None, [p.overlap] * 5):
        a = gpu.match_multi_batch_device(algos, [b.ptr for b in bufs], lens, p)
        b_ = gpu.match_multi_varlen_batch_device(algos, [b.ptr for b in bufs], lens, p, overlaps=fmt_overlaps)
        assert key(a) == key(b_)
        assert sum(len(x) for row in a for x in row) == 10


def test_varlen_errors(gpu, oracle):
    sr = SR8
    needles = [oracle.synth_uniform(51, 500 + j, 0, s) for j, s in enumerate((4000, 9000))]
    hay = oracle.synth_uniform(51, 1, 0, 40 * sr)
    for o in range(2 * sr, 38 * sr, 3 * sr):
        hay[o:o + 4000] += needles[0]
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=1.0, distance_s=0.1, prominence=PROM).params(sr, gpu.Scale.LIB)
    algos = [gpu.HipConvolve(n) for n in needles]
    b = gpu.DeviceBuffer.from_numpy(0, hay)
    L = gpu.lib()
    handles = (C.c_void_p * 2)(*[a._h for a in algos])
    ptrs = (C.c_void_p * 1)(b.ptr)
    lens = (C.c_size_t * 1)(hay.size)
    counts = (C.c_size_t * 2)()
    buf = (gpu.AmPeak * 8)()
    # capacity: AM_ERR_CAPACITY with the counts filled in (12 hits of needle 0, 4 slots per pair)
    rc = L.am_match_multi_varlen_batch_device(handles, 2, None, ptrs, lens, 1, 0, C.byref(p), buf, 4, counts)
    assert rc == gpu.AM_ERR_CAPACITY and counts[0] == 12 and counts[1] == 0
    # null pointers
    assert L.am_match_multi_varlen_batch_device(None, 2, None, ptrs, lens, 1, 0, C.byref(p), buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    assert L.am_match_multi_varlen_batch_device(handles, 2, None, None, lens, 1, 0, C.byref(p), buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    assert L.am_match_multi_varlen_batch_device(handles, 2, None, ptrs, lens, 1, 0, None, buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    assert L.am_match_multi_varlen(handles, 2, None, None, hay.size, 0, C.byref(p), buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    nulls = (C.c_void_p * 2)(algos[0]._h, None)
    assert L.am_match_multi_varlen_batch_device(nulls, 2, None, ptrs, lens, 1, 0, C.byref(p), buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    assert L.am_match_multi_varlen_batch_device(handles, 2, None, ptrs, lens, 1, 7, C.byref(p), buf, 4, counts) == gpu.AM_ERR_INVALID_ARG
    # AM_SCALE_MY is refused
    q = gpu.AmMatchParams.from_buffer_copy(p)
    q.scale = int(gpu.Scale.MY)
    with pytest.raises(gpu.AudioMatchError):
        gpu.match_multi_varlen_batch_device(algos, [b.ptr], [hay.size], q)
    # score_norm is refused with the shared message
    algos[0].set_option("score_norm", 1)
    try:
        with pytest.raises(gpu.AudioMatchError, match="score_norm: not supported by this entry point"):
            gpu.match_multi_varlen_batch_device(algos, [b.ptr], [hay.size], p)
        with pytest.raises(gpu.AudioMatchError, match="score_norm: not supported by this entry point"):
            gpu.match_multi_varlen(algos, hay, p)
    finally:
        algos[0].set_option("score_norm", -1)
    # the overlap list must match the needles (binding)
    with pytest.raises(ValueError):
        gpu.match_multi_varlen(algos, hay, p, overlaps=[1])
    # needles on two devices
    if gpu.device_count() > 1:
        other = gpu.HipConvolve(needles[1], device=1)
        with pytest.raises(gpu.AudioMatchError, match="one device"):
            gpu.match_multi_varlen_batch_device([algos[0], other], [b.ptr], [hay.size], p)
