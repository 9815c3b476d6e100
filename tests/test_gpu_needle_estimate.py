"""Needle estimation on the device (am_needle_estimate_rows, am_needle_estimate_device) against the checker of
tests/needle_estimate_ref.py: est and count bit for bit, dev within 2 f32 ulps (its f64 sum of squares may be contracted
to fma on the device, which can move the last f64 bit and so flip one f32 rounding; est adds exactly representable terms
and its divisions are correctly rounded).  Every case is one or a few launches on a few thousand samples, apart from the
end-to-end match."""
import ctypes as C

import numpy as np
import pytest

import needle_estimate_ref as ref

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64)          # the edges of the 8-, 16-, 32- and 64-slot networks
LENGTHS = (1, 63, 64, 65, 255, 257, 4097)             # lane, wave and workgroup edges, more than one workgroup
TRIMS = (0, 100, 334, 500)
DEV_ULPS = 2.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, rows, method, trim=0, what=""):
    est, dev, cnt = got
    w_est, w_dev, w_cnt = ref.estimate(rows, method, trim)
    assert np.array_equal(cnt, w_cnt), what
    assert np.array_equal(bits(est), bits(w_est)), (what, np.flatnonzero(bits(est) != bits(w_est))[:5])
    u = ref.ulps_f32(dev, w_dev)
    print(f"{what}: dev max {u.max():.2f} ulp")
    assert np.isfinite(dev).all() and u.max() <= DEV_ULPS, (what, u.max())


def random_rows(rng, n, length):
    """about 10 % absent elements; -0, +0, equal values and denormals among the rest; one all-absent column"""
    r = rng.standard_normal((n, length)).astype(np.float32)
    kind = rng.random((n, length))
    r = np.where(kind < 0.10, np.round(r * 2) / 2, r)                  # equal values: multiples of 0.5
    r = np.where((kind >= 0.10) & (kind < 0.15), np.float32(-0.0), r)
    r = np.where((kind >= 0.15) & (kind < 0.20), np.float32(0.0), r)
    r = np.where((kind >= 0.20) & (kind < 0.25), (r * np.float32(1e-41)).astype(np.float32), r)   # denormals of both signs
    r = np.where((kind >= 0.25) & (kind < 0.33), np.float32(np.nan), r)
    r = np.where((kind >= 0.33) & (kind < 0.34), np.float32(np.inf), r)
    r = np.where((kind >= 0.34) & (kind < 0.35), np.float32(-np.inf), r)
    r = r.astype(np.float32)
    if length >= 2:
        r[:, length // 2] = np.nan
    return r


@pytest.mark.parametrize("n", NS)
def test_rows_against_the_checker(gpu, n):
    rng = np.random.default_rng(1000 + n)
    for length in LENGTHS:
        rows = random_rows(rng, n, length)
        check(gpu.estimate_needle(rows, gpu.Est.MEAN), rows, ref.MEAN, what=f"mean n={n} length={length}")
        got = gpu.estimate_needle(rows, gpu.Est.MEDIAN)
        check(got, rows, ref.MEDIAN, what=f"median n={n} length={length}")
        if length >= 2:
            col = length // 2
            assert (got[0][col], got[1][col], got[2][col]) == (0.0, 0.0, 0)
        for trim in TRIMS:
            check(gpu.estimate_needle(rows, gpu.Est.TRIMMED, trim), rows, ref.TRIMMED, trim, what=f"trimmed {trim} n={n} length={length}")


def test_total_order_is_pinned(gpu):
    """columns of -0 / +0 / equal values only: the sign of a zero estimate says which one the rank picked"""
    z, nz, nan = np.float32(0.0), np.float32(-0.0), np.float32(np.nan)
    cols = [[nz, z, z], [nz, nz, z], [z, nz, nan], [nz, nan, nan], [z, z, z], [nz, nz, nz], [nan, nan, nan], [1.0, 1.0, -1.0]]
    rows = np.array(cols, dtype=np.float32).T.copy()
    est, dev, cnt = gpu.estimate_needle(rows, gpu.Est.MEDIAN)
    assert np.signbit(est).tolist() == [False, True, False, True, False, True, False, False]
    assert cnt.tolist() == [3, 3, 2, 1, 3, 3, 0, 3] and est[7] == 1.0 and (dev[:7] == 0).all()
    check((est, dev, cnt), rows, ref.MEDIAN, what="zeros")
    for method, trim in ((ref.MEAN, 0), (ref.TRIMMED, 0), (ref.TRIMMED, 334)):
        check(gpu.estimate_needle(rows, method, trim), rows, method, trim, what=f"zeros method {method} trim {trim}")
    # dev and count are optional
    L = gpu.lib()
    ep = gpu.AmEstimateParams(ref.MEDIAN, 0, 0, rows.shape[1])
    only = np.full(rows.shape[1], 7.0, np.float32)
    assert L.am_needle_estimate_rows(0, rows.ctypes.data, 3, C.byref(ep), only.ctypes.data, None, None) == 0
    assert np.array_equal(bits(only), bits(est))


def test_mean_takes_many_rows_and_median_states_its_limit(gpu):
    rng = np.random.default_rng(5)
    rows = random_rows(rng, 1000, 300)
    check(gpu.estimate_needle(rows, gpu.Est.MEAN), rows, ref.MEAN, what="mean n=1000")
    for method in (gpu.Est.MEDIAN, gpu.Est.TRIMMED):
        with pytest.raises(gpu.AudioMatchError) as e:
            gpu.estimate_needle(rows[:65], method)
        assert e.value.code == gpu.AM_ERR_INVALID_ARG and "at most 64 hits" in str(e.value)


LEAD, LENGTH, HAY = 200, 2500, 20000
# (haystack, start, scale): start < lead, odd starts, one that reaches past its haystack's end, one window with a NaN
HITS = [(0, 50, 1.0), (1, 19001, 0.5), (2, 6001, -2.0), (0, 7777, 0.125), (1, 333, 3.0), (2, 12345, 0.7), (0, 15001, 1.5),
        (1, 9000, -0.3), (2, 201, 4.0)]


@pytest.mark.parametrize("kind", ["f32", "s16"])
def test_device_form_equals_rows_form(gpu, kind):
    rng = np.random.default_rng(77)
    if kind == "f32":
        hays = [rng.uniform(-1, 1, HAY).astype(np.float32) for _ in range(3)]
        hays[2][7000] = np.nan
        hays[1][19500] = np.inf
        fmt = gpu.Fmt.F32_MONO
    else:
        hays = [rng.integers(-32768, 32768, 2 * HAY, dtype=np.int16) for _ in range(3)]
        fmt = gpu.Fmt.S16_STEREO
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        for order in (list(range(9)), [4, 8, 0, 2, 6, 1, 7, 3, 5]):
            hits = [HITS[i] for i in order]
            rows = np.stack([gpu.hit_window(hays[k], start, scale, LEAD, LENGTH) for k, start, scale in hits])
            want_rows = np.stack([ref.hit_window(hays[k], start, scale, LEAD, LENGTH) for k, start, scale in hits])
            assert np.array_equal(np.isnan(rows), np.isnan(want_rows)) and np.array_equal(bits(np.nan_to_num(rows)), bits(np.nan_to_num(want_rows)))
            assert np.isnan(rows[order.index(0), :150]).all() and np.isnan(rows[order.index(1), 1199:]).all()
            results = {}
            for method, trim in ((ref.MEAN, 0), (ref.MEDIAN, 0), (ref.TRIMMED, 100)):
                a = gpu.estimate_needle_device(0, [b.ptr for b in bufs], [HAY] * 3, hits, LEAD, LENGTH, method, trim, fmt)
                b = gpu.estimate_needle(rows, method, trim)
                for x, y in zip(a, b):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (kind, method)
                check(a, rows, method, trim, what=f"{kind} device form method {method}")
                results[method] = a
            if order == list(range(9)):
                first = results
            else:
                assert np.array_equal(bits(results[ref.MEDIAN][0]), bits(first[ref.MEDIAN][0]))   # the median ignores the order
                assert np.array_equal(results[ref.MEAN][2], first[ref.MEAN][2])
    finally:
        for b in bufs:
            b.free()


def test_device_form_refuses_host_memory(gpu):
    x = np.zeros(100, np.float32)
    with pytest.raises(gpu.AudioMatchError) as e:
        gpu.estimate_needle_device(0, [x.ctypes.data], [100], [(0, 0, 1.0)], 0, 10)
    assert e.value.code == gpu.AM_ERR_INVALID_ARG and str(e.value).count("hit 0: ") == 1 and "not device memory" in str(e.value)


MARGIN = 256


def test_designed_exactness(gpu):
    """nine occurrences g_i * c under overlays that cover a third each: the median and the 334 permille trimmed mean give c
    back bit for bit, the mean does not; on the margins (a background of exact zeros) est = 0 and dev = 0"""
    c, occ, scales, dirty = ref.designed_case()
    length = ref.CLEAN_LEN + 2 * MARGIN
    hays, hits = [], []
    for i in range(9):
        h = np.zeros(8192, np.float32)
        start = 1001 + 37 * i
        h[start:start + ref.CLEAN_LEN] = occ[i]
        hays.append(h)
        hits.append((i, start, float(scales[i])))
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        rows = np.stack([gpu.hit_window(hays[k], start, scale, MARGIN, length) for k, start, scale in hits])
        inner = slice(MARGIN, MARGIN + ref.CLEAN_LEN)
        for form in ("rows", "device"):
            def run(method, trim=0):
                if form == "rows":
                    return gpu.estimate_needle(rows, method, trim)
                return gpu.estimate_needle_device(0, [b.ptr for b in bufs], [8192] * 9, hits, MARGIN, length, method, trim)
            for method, trim in ((ref.MEDIAN, 0), (ref.TRIMMED, 334)):
                est, dev, cnt = run(method, trim)
                assert (cnt == 9).all()
                assert np.array_equal(bits(est[inner]), bits(c)), (form, method)
                for edge in (slice(0, MARGIN), slice(MARGIN + ref.CLEAN_LEN, length)):
                    assert (est[edge] == 0).all() and (dev[edge] == 0).all(), (form, method)
                assert (dev[inner] > 0).all()
            est, dev, cnt = run(ref.MEAN)
            bound = 0.01 * np.abs(c).max()
            for t in range(3):
                third = slice(t * ref.THIRD, min((t + 1) * ref.THIRD, ref.CLEAN_LEN))
                assert np.abs(est[inner] - c)[third].max() > bound, (form, t)
            assert (est[:MARGIN] == 0).all() and (dev[:MARGIN] == 0).all()
    finally:
        for b in bufs:
            b.free()


def ncc(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def test_end_to_end_rough_needle_to_better_needle(gpu):
    """match with the rough needle (occurrence 0, overlay included), scale = 1 / gain of am_hit_scores, estimate: the bits
    of the checker on the same hits and scales, and a median estimate closer to the clean needle than the rough one was.
    (The gain measured against the rough needle is no power of two: exact recovery of c is not claimed here.)"""
    c, occ, scales, dirty = ref.designed_case()
    sr = 8192
    rough = occ[0]
    algo = gpu.HipConvolve(rough)
    p = gpu.Config(chunk_size_s=4.0, overlap_length_s=ref.CLEAN_LEN / sr, distance_s=1.0, prominence=0.05).params(sr, gpu.Scale.LIB)
    rows, want_rows = [], []
    try:
        for i in range(9):
            hay = np.zeros(65536, np.float32)
            start = 5003 + 4099 * i
            hay[start:start + ref.CLEAN_LEN] = occ[i]
            peaks = algo.match(hay, p)
            at = [pk for pk in peaks if pk.start == start]
            assert len(at) == 1, (i, start, [pk.start for pk in peaks])
            score = algo.hit_scores(hay, at)[0]
            assert score.flags & 6 == 0 and score.gain > 0, (i, score)
            scale = np.float32(1.0) / np.float32(score.gain)
            rows.append(gpu.hit_window(hay, start, scale, 0, ref.CLEAN_LEN))
            want_rows.append(ref.hit_window(hay, start, scale, 0, ref.CLEAN_LEN))
    finally:
        algo.close()
    rows, want_rows = np.stack(rows), np.stack(want_rows)
    assert np.array_equal(bits(rows), bits(want_rows))
    est, dev, cnt = gpu.estimate_needle(rows, gpu.Est.MEDIAN)
    check((est, dev, cnt), want_rows, ref.MEDIAN, what="end to end")
    before, after = ncc(rough, c), ncc(est, c)
    print(f"ncc(rough, c) = {before:.4f}, ncc(median estimate, c) = {after:.4f}")
    assert after > before


def test_empty_haystack_is_all_absent(gpu):
    buf = gpu.DeviceBuffer.from_numpy(0, np.ones(4, np.float32))
    try:
        est, dev, cnt = gpu.estimate_needle_device(0, [buf.ptr, buf.ptr], [0, 4], [(0, 0, 1.0), (1, 0, 2.0)], 1, 6, ref.MEDIAN)
        assert est.tolist() == [0.0, 2.0, 2.0, 2.0, 2.0, 0.0] and cnt.tolist() == [0, 1, 1, 1, 1, 0] and (dev == 0).all()
    finally:
        buf.free()
