"""Per-hit significance (am_hit_significance*): each hit's score against its local background, checked against the
library's own am_correlate scores of the hit's span (bit for bit where the definition allows), against f64 truth, and
for the independence of a hit's record from everything but its own zone."""
import ctypes as C

import numpy as np
import pytest

import hit_significance_ref as ref

pytestmark = pytest.mark.gpu

S, N, PLANTS = 5000, 120_000, (20_000, 61_111, 90_003)
G, B = S - 1, 3 * S


def noise(seed, n, amp):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def case(seed=1, s=S, n=N, plants=PLANTS):
    needle = noise(seed, s, 0.5)
    hay = noise(seed + 100, n, 0.1)
    for t in plants:
        hay[t:t + s] += needle
    return needle, hay


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def bits(recs):
    return [ref.pack(q) for q in recs]


def library_ref(am, algo, hay, t, guard, radius):
    """The checker's record of a hit at t, fed with the host am_correlate scores of the hit's span."""
    s = len(algo._needle_for_tests)
    lo, hi, clipped = ref.zone(t, s, len(hay), radius)
    scores = algo.correlate_with_sample(hay[lo:hi + s], am.Mode.Valid, scale=True)
    assert len(scores) == hi - lo + 1
    return ref.significance_ref(scores, t - lo, guard, clipped)


def make_algo(am, needle, **kw):
    algo = am.HipConvolve(needle, **kw)
    algo._needle_for_tests = needle
    return algo


def check_hits(am, algo, hay, ts, guard, radius, got=None):
    got = got if got is not None else algo.hit_significance(hay, peaks_at(am, ts), guard, radius)
    for t, g in zip(ts, got):
        ref.assert_record(g, library_ref(am, algo, hay, int(t), guard, radius))
    return got


@pytest.fixture(scope="module")
def base():
    return case()


@pytest.fixture(scope="module")
def truth(base):
    """Every LIB score of the base case from f64 dot products (computed once, shared, never changed)."""
    needle, hay = base
    n64 = needle.astype(np.float64)
    r = np.correlate(hay.astype(np.float64), n64, mode="valid") / np.dot(n64, n64)
    r.setflags(write=False)
    return r


# ---- 1. the contract against the library's own scores ----------------------------------------------------------------
def test_contract_against_library_scores(gpu, base):
    needle, hay = base
    ts = list(PLANTS) + [0, N - S, 1] + [int(t) for t in np.random.default_rng(7).integers(0, N - S + 1, 16)]
    algo = make_algo(gpu, needle)
    got = check_hits(gpu, algo, hay, ts, G, B)
    for g in got[:3]:
        assert g.flags == 0 and g.n_bg == 2 * (B - G), g
    assert got[3].flags == ref.CLIPPED and got[4].flags == ref.CLIPPED and got[5].flags == ref.CLIPPED


# ---- 2. against f64 truth --------------------------------------------------------------------------------------------
def test_against_f64_truth(gpu, base, truth):
    needle, hay = base
    algo = make_algo(gpu, needle)
    got = algo.hit_significance(hay, peaks_at(gpu, PLANTS), G, B)
    for t, g in zip(PLANTS, got):
        lo, hi, clipped = ref.zone(t, S, N, B)
        exp = ref.significance_ref(truth[lo:hi + 1], t - lo, G, clipped)
        print("plant", t, "z", g.z, "truth z", exp["_z64"], "score", g.score, exp["score"], "side", g.side_max, exp["side_max"])
        assert abs(g.score - exp["score"]) <= 1e-4 and abs(g.side_max - exp["side_max"]) <= 1e-4, (g, exp)
        assert abs(g.z - exp["_z64"]) <= 0.01 * abs(exp["_z64"]), (g, exp)
        assert g.z > 100, g


def test_background_positions_are_insignificant(gpu):
    needle, hay = case(seed=5, n=400_000, plants=(20_000,))
    ts = [int(t) for t in np.random.default_rng(11).integers(50_000, 400_000 - S + 1, 64)]
    algo = make_algo(gpu, needle)
    got = algo.hit_significance(hay, peaks_at(gpu, ts), G, B)
    zs = [abs(g.z) for g in got]
    print("largest |z| over 64 background positions:", max(zs))
    assert all(g.flags in (0, ref.CLIPPED) for g in got)
    assert max(zs) < 6, max(zs)


# ---- 3. the three forms agree bit for bit ----------------------------------------------------------------------------
def test_three_forms_agree(gpu):
    am, L = gpu, gpu.lib()
    lens = (40_000, 52_345, 33_333)
    needles = [noise(21, 3000, 0.5), noise(22, 4321, 0.5)]
    hays = []
    for k, n in enumerate(lens):
        h = noise(30 + k, n, 0.1)
        for j, nd in enumerate(needles):
            t = 5000 + 9000 * j + 1000 * k
            h[t:t + len(nd)] += nd
        hays.append(h)
    guard, radius = 4320, 9000
    algos = [make_algo(am, nd) for nd in needles]
    bufs = [am.DeviceBuffer.from_numpy(0, h) for h in hays]
    nn, nh, cap, count = 2, 3, 3, 5        # each pair announces 5 hits, the layout holds 3: 3 are scored
    rng = np.random.default_rng(3)
    peaks = (am.AmPeak * (cap * nn * nh))()
    counts = (C.c_size_t * (nn * nh))()
    ts = {}
    for k in range(nh):
        for j in range(nn):
            q = k * nn + j
            counts[q] = count if q != 4 else 2   # one pair with fewer hits than slots: its last slot stays untouched
            ts[q] = [5000 + 9000 * j + 1000 * k, 0] + [int(rng.integers(0, lens[k] - len(needles[j]) + 1))]
            for i, t in enumerate(ts[q]):
                peaks[q * cap + i] = am.AmPeak(t, t + 1, 0, 0)
    sentinel = am.HitSignificance(-7.0, -7.0, -7.0, -7.0, -7.0, -77, 777, 0xABCD)
    out = (am.HitSignificance * (cap * nn * nh))(*[sentinel] * (cap * nn * nh))
    sp = am.AmSignificanceParams(guard, radius)
    try:
        rc = L.am_hit_significance_batch_device((C.c_void_p * nn)(*[a._h for a in algos]), nn, (C.c_void_p * nh)(*[b.ptr for b in bufs]),
                                                (C.c_size_t * nh)(*lens), nh, 0, peaks, cap, counts, C.byref(sp), out)
        assert rc == am.AM_OK, L.am_last_error_string()
        for k in range(nh):
            for j in range(nn):
                q = k * nn + j
                scored = min(int(counts[q]), cap)
                pk = peaks_at(am, ts[q][:scored])
                host = algos[j].hit_significance(hays[k], pk, guard, radius)
                dev = algos[j].hit_significance_device(bufs[k].ptr, lens[k], pk, guard, radius)
                batch = [out[q * cap + i] for i in range(scored)]
                assert bits(host) == bits(dev) == bits(batch), (k, j)
                check_hits(am, algos[j], hays[k], ts[q][:scored], guard, radius, got=host)
                for i in range(scored, cap):
                    assert ref.pack(out[q * cap + i]) == ref.pack(sentinel), (k, j, i)
        assert host[0].z > 50
    finally:
        for b in bufs:
            b.free()


# ---- 4. independence -------------------------------------------------------------------------------------------------
def test_independence_of_other_hits(gpu, base):
    needle, hay = base
    algo = make_algo(gpu, needle)
    t0 = 61_111
    alone = algo.hit_significance(hay, peaks_at(gpu, [t0]), G, B)[0]
    others = [int(t) for t in np.random.default_rng(13).integers(t0 - 2 * B, t0 + 2 * B, 40)]   # overlapping zones
    ts = others[:17] + [t0] + others[17:]
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        among = algo.hit_significance_device(buf.ptr, N, peaks_at(gpu, ts), G, B)
        rev = algo.hit_significance_device(buf.ptr, N, peaks_at(gpu, ts[::-1]), G, B)
    finally:
        buf.free()
    assert ref.pack(among[17]) == ref.pack(alone) == ref.pack(rev[len(ts) - 1 - 17])
    assert bits(among) == bits(rev[::-1])
    assert bits(algo.hit_significance(hay, peaks_at(gpu, ts), G, B)) == bits(among)


# ---- 5. zone edges ---------------------------------------------------------------------------------------------------
def test_zone_edges(gpu, base):
    needle, hay = base
    algo = make_algo(gpu, needle)
    ts = [0, 7, 20_000, N - S - 3, N - S]
    check_hits(gpu, algo, hay, ts, 0, B)                       # G = 0
    got = check_hits(gpu, algo, hay, ts, 10, 11)               # B = G + 1
    assert got[2].n_bg == 2 and got[2].flags == 0, got[2]
    assert got[0].n_bg == 1 and got[0].flags == ref.NO_BG | ref.CLIPPED
    # the CLIPPED flag exactly where the checker sets it
    edge = [B - 1, B, B + 1, N - S - B - 1, N - S - B, N - S - B + 1]
    got = check_hits(gpu, algo, hay, edge, G, B)
    assert [bool(g.flags & ref.CLIPPED) for g in got] == [True, False, False, False, False, True]
    # a haystack of exactly S samples: no background, the score is am_correlate's
    only = hay[20_000:20_000 + S].copy()
    g = check_hits(gpu, algo, only, [0], G, B)[0]
    assert g.n_bg == 0 and g.flags == ref.NO_BG | ref.CLIPPED and np.isnan(g.z) and g.side_lag == 0
    assert ref.f32_bits(g.score) == ref.f32_bits(algo.correlate_with_sample(only, gpu.Mode.Valid, scale=True)[0])
    # len = S + 1, G = 0, B = 1: one background lag
    for t in (0, 1):
        g = check_hits(gpu, algo, hay[30_000:30_000 + S + 1].copy(), [t], 0, 1)[0]
        assert g.n_bg == 1 and g.flags == ref.NO_BG | ref.CLIPPED and np.isnan(g.bg_mean) and np.isnan(g.side_max)


def test_flat_background(gpu):
    s, n, guard = 1000, 20_000, 99
    needle = noise(41, s, 0.5)
    zeros = np.zeros(n, dtype=np.float32)
    algo = make_algo(gpu, needle)
    got = check_hits(gpu, algo, zeros, [8000, 0, n - s], guard, 3000)
    for g, lag, clip in zip(got, (-(guard + 1), guard + 1, -(guard + 1)), (0, ref.CLIPPED, ref.CLIPPED)):
        assert g.flags == ref.FLAT | clip and g.z == 0.0 and g.side_lag == lag, g
        assert g.bg_std == 0.0 and g.bg_mean == 0.0 and g.side_max == 0.0 and g.score == 0.0


# ---- 6. plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,n,t,guard,radius", [(300, 5000, 2222, 299, 400), (100_000, 1_400_000, 640_001, 99_999, 550_000),
                                                ((1 << 22) + 1001, (1 << 22) + 120_001, 60_000, 1000, 50_000)],
                         ids=["generic", "register", "partitioned"])
def test_plans(gpu, s, n, t, guard, radius):
    """A single plant through every size class.  (A partitioned needle is longer than AM_SIG_MAX_RADIUS: its guard
    cannot be S - 1; white noise has no lobes to clear, so a short guard serves.)"""
    needle, hay = case(seed=9, s=s, n=n, plants=(t,))
    algo = make_algo(gpu, needle)
    g = check_hits(gpu, algo, hay, [t], guard, radius)[0]
    print("s", s, "span", min(n - s, t + radius) + s - max(0, t - radius), "z", g.z, "n_bg", g.n_bg)
    assert g.z > 5 and not g.flags & (ref.NONFIN | ref.NO_BG | ref.FLAT), g


# ---- 7. formats and options ------------------------------------------------------------------------------------------
def test_s16_stereo_equals_f32_of_the_downmix(gpu):
    s, frames = 2000, 50_000
    rng = np.random.default_rng(17)
    lr = rng.integers(-3000, 3000, size=(frames, 2)).astype(np.int16)
    nd = rng.integers(-12000, 12000, size=(s, 2)).astype(np.int16)
    lr[31_000:31_000 + s] += nd
    needle = gpu.pcm_s16_stereo_to_mono(nd)
    mono = gpu.pcm_s16_stereo_to_mono(lr)
    ts = [31_000, 0, 100, 12_345, frames - s]
    algo = make_algo(gpu, needle)
    b16, b32 = gpu.DeviceBuffer.from_numpy(0, lr), gpu.DeviceBuffer.from_numpy(0, mono)
    try:
        d16 = algo.hit_significance_device(b16.ptr, frames, peaks_at(gpu, ts), s - 1, 3 * s, fmt=gpu.Fmt.S16_STEREO)
        d32 = algo.hit_significance_device(b32.ptr, frames, peaks_at(gpu, ts), s - 1, 3 * s)
    finally:
        b16.free()
        b32.free()
    assert bits(d16) == bits(d32) == bits(algo.hit_significance(lr, peaks_at(gpu, ts), s - 1, 3 * s))
    check_hits(gpu, algo, mono, ts, s - 1, 3 * s, got=d16)
    assert d16[0].z > 50


def test_score_norm_gives_ncc_records(gpu, base):
    needle, hay = base
    ts = list(PLANTS) + [0, 33_333, N - S]
    algo = make_algo(gpu, needle, score_norm=True)
    got = check_hits(gpu, algo, hay, ts, G, B)     # (correlate_with_sample under this handle returns NCC)
    plain = make_algo(gpu, needle).hit_significance(hay, peaks_at(gpu, ts), G, B)
    # white noise: the NCC of an unrelated window has a standard deviation of 1 / sqrt(S), so z is about score * sqrt(S) = 69
    for g, p in zip(got[:3], plain[:3]):
        assert 0.9 < g.score <= 1.0 and abs(g.z - g.score * np.sqrt(S)) < 0.1 * g.z and p.score > g.score, (g, p)


def test_half_pipeline_keeps_offsets_and_flags(gpu, base):
    needle, hay = base
    ts = list(PLANTS) + [0, 33_333, N - S]
    f32 = make_algo(gpu, needle).hit_significance(hay, peaks_at(gpu, ts), G, B)
    algo = make_algo(gpu, needle)
    algo.set_option("half_pipeline", 2)
    half = check_hits(gpu, algo, hay, ts, G, B)
    for a, b in zip(f32, half):
        assert (a.flags, a.n_bg) == (b.flags, b.n_bg), (a, b)
    for a, b in zip(f32[:3], half[:3]):
        assert a.side_lag == b.side_lag and abs(a.z - b.z) <= 0.01 * abs(a.z), (a, b)


# ---- 8. non-finite samples -------------------------------------------------------------------------------------------
def test_nonfinite(gpu, base):
    needle, hay = base
    algo = make_algo(gpu, needle)
    ts = [61_111, 20_000]
    clean = algo.hit_significance(hay, peaks_at(gpu, ts), G, B)
    bad = hay.copy()
    bad[61_111 + S + 4000] = np.nan            # inside the first hit's span, outside its window; the second misses it
    got = algo.hit_significance(bad, peaks_at(gpu, ts), G, B)
    lo, hi, clipped = ref.zone(61_111, S, N, B)
    ref.assert_record(got[0], ref.significance_ref(np.zeros(hi - lo + 1, np.float32), 61_111 - lo, G, clipped, nonfinite=True))
    assert got[0].flags == ref.NONFIN and got[0].n_bg == clean[0].n_bg and got[0].side_lag == 0
    assert all(np.isnan(v) for v in (got[0].score, got[0].bg_mean, got[0].bg_std, got[0].z, got[0].side_max))
    assert ref.pack(got[1]) == ref.pack(clean[1])
    # an inf in the needle: every hit, CLIPPED the only flag beside it
    nd = needle.copy()
    nd[123] = np.inf
    got = make_algo(gpu, nd).hit_significance(hay, peaks_at(gpu, [61_111, 0]), G, B)
    assert [g.flags for g in got] == [ref.NONFIN, ref.NONFIN | ref.CLIPPED] and all(np.isnan(g.score) and np.isnan(g.z) for g in got)
    assert got[0].n_bg == 2 * (B - G)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def _rc(gpu, fn, *args):
    rc = fn(*args)
    msg = gpu.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_refusals(gpu):
    L = gpu.lib()
    s, n = 5000, 30_000
    needle, hay = noise(71, s, 0.5), noise(72, n, 0.1)
    algo = make_algo(gpu, needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    pk = (gpu.AmPeak * 2)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(n - s + 1, n - s + 2, 0, 0))
    out = (gpu.HitSignificance * 4)()
    sp = gpu.AmSignificanceParams(s - 1, 3 * s)
    spp = C.byref(sp)
    INV = gpu.AM_ERR_INVALID_ARG
    try:
        assert _rc(gpu, L.am_hit_significance_device, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK     # n = 0
        assert _rc(gpu, L.am_hit_significance, algo._h, None, n, 0, None, 0, None, None)[0] == gpu.AM_OK
        cnt = (C.c_size_t * 1)(0)
        assert _rc(gpu, L.am_hit_significance_batch_device, (C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr),
                   (C.c_size_t * 1)(n), 1, 0, None, 4, cnt, None, None)[0] == gpu.AM_OK
        for fn, src in ((L.am_hit_significance_device, buf.ptr), (L.am_hit_significance, hay.ctypes.data)):
            for args in ((algo._h, None, n, 0, pk, 1, spp, out), (algo._h, src, n, 0, None, 1, spp, out),
                         (algo._h, src, n, 0, pk, 1, spp, None), (algo._h, src, n, 0, pk, 1, None, out)):     # the last: sp == NULL
                rc, msg = _rc(gpu, fn, *args)
                assert rc == INV and "null" in msg, msg
            assert _rc(gpu, fn, None, src, n, 0, pk, 1, spp, out)[0] == INV
            for bad, text in ((gpu.AmSignificanceParams(5, 5), "guard 5 >= radius 5"), (gpu.AmSignificanceParams(9, 3), "guard 9 >= radius 3"),
                              (gpu.AmSignificanceParams(0, 0), "guard 0 >= radius 0"),
                              (gpu.AmSignificanceParams(0, (1 << 22) + 1), "AM_SIG_MAX_RADIUS")):
                rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 1, C.byref(bad), out)
                assert rc == INV and text in msg, msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 2, pk, 1, spp, out)
            assert rc == INV and "format" in msg
            rc, msg = _rc(gpu, fn, algo._h, src, n, 0, pk, 2, spp, out)
            assert rc == INV and "hit 1" in msg and "haystack length" in msg
        rc, msg = _rc(gpu, L.am_hit_significance_device, algo._h, hay.ctypes.data, n, 0, pk, 1, spp, out)   # host memory
        assert rc == INV and "device" in msg
        # batch: the message names the pair and the hit
        pairs = (gpu.AmPeak * 4)(gpu.AmPeak(10, 11, 0, 0), gpu.AmPeak(0, 0, 0, 0), gpu.AmPeak(20, 21, 0, 0), gpu.AmPeak(n, n + 1, 0, 0))
        one = (C.c_void_p * 1)(algo._h)
        rc, msg = _rc(gpu, L.am_hit_significance_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 2), spp, out)
        assert rc == INV and "pair 1" in msg and "hit 1" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_significance_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, hay.ctypes.data),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), spp, out)
        assert rc == INV and "pair 1" in msg and "device" in msg, msg
        rc, msg = _rc(gpu, L.am_hit_significance_batch_device, one, 1, (C.c_void_p * 2)(buf.ptr, buf.ptr),
                      (C.c_size_t * 2)(n, n), 2, 0, pairs, 2, (C.c_size_t * 2)(1, 1), None, out)
        assert rc == INV and "null" in msg
        # A haystack on another device than the needle needs a second GPU; on a one-GPU machine only the host-memory
        # refusal above runs.
        if gpu.device_count() >= 2:
            other = gpu.DeviceBuffer.from_numpy(1, hay)
            try:
                rc, msg = _rc(gpu, L.am_hit_significance_device, algo._h, other.ptr, n, 0, pk, 1, spp, out)
                assert rc == INV and "device" in msg
            finally:
                other.free()
        # a good call still works after the refusals, and after am_shutdown (the scratch buffers come back), same bits
        before = algo.hit_significance_device(buf.ptr, n, [gpu.Peak(10, 11, 0, 0)], s - 1, 3 * s)[0]
    finally:
        buf.free()
    check_hits(gpu, algo, hay, [10], s - 1, 3 * s, got=[before])
    assert ref.pack(algo.hit_significance(hay, [gpu.Peak(10, 11, 0, 0)], s - 1, 3 * s)[0]) == ref.pack(before)
    assert L.am_shutdown() == gpu.AM_OK
    assert ref.pack(algo.hit_significance(hay, [gpu.Peak(10, 11, 0, 0)], s - 1, 3 * s)[0]) == ref.pack(before)
