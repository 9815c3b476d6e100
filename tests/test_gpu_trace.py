"""GPU tests of the score traces (include/audiomatch.h, "score traces").

Array forms: am_trace_scores / am_trace_scores_device against trace_ref on the designed arrays of trace_cases.py, at every
bin length around the two kernel forms' sizes, at every 4-byte alignment of the device array and under every value of
the option "trace_form" -- all fields and, the values being integers, the sums bit for bit; on white noise the fields bit
for bit and the sums within the bound of two orders of the same additions (trace_ref.sum_bound), and on scores whose sums
round every record bit for bit against a numpy model of the order the header documents (trace_ref.trace_ordered).

Match forms: am_match_trace* against trace_ref over the scores am_correlate_device writes."""
import ctypes as C
import functools

import numpy as np
import pytest

import trace_cases as tc
import trace_ref as tr

pytestmark = pytest.mark.gpu

SR = 8000
S = 4000


class forced_form:
    def __init__(self, gpu, form):
        self.gpu, self.form = gpu, form

    def __enter__(self):
        self.gpu.set_option("trace_form", self.form)

    def __exit__(self, *exc):
        self.gpu.set_option("trace_form", 0)


def upload_at_every_alignment(gpu, buf, x):
    """x four times in buf, copy k starting k floats behind a 16-byte boundary; the device address of each copy."""
    n = x.size
    stride = (n + 3 + 3) // 4 * 4
    packed = np.zeros(4 * stride, dtype=np.float32)
    for k in range(4):
        packed[k * stride + k:k * stride + k + n] = x
    assert packed.nbytes <= buf.nbytes
    assert gpu.lib().am_memcpy_h2d(0, buf.ptr, packed.ctypes.data, packed.nbytes) == 0
    return [buf.ptr + 4 * (k * stride + k) for k in range(4)]


# ---- array forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_designed_arrays_every_form_and_alignment(gpu, case):
    W, SL = gpu.AM_TRACE_WAVE_BIN_MAX, gpu.AM_TRACE_SLICE
    lengths = tc.bin_lengths(W, SL)
    buf = gpu.DeviceBuffer(0, 4 * 4 * (3 * max(lengths) + 8))
    for D in lengths:
        for n in tc.score_counts(D):
            x, claims = tc.build(case, D, n, SL)
            ref = tr.trace(x, D)
            ptrs = upload_at_every_alignment(gpu, buf, x)
            assert ptrs[0] % 16 == 0
            for form in (0, 1, 2):
                with forced_form(gpu, form):
                    host = gpu.trace_scores(x, D)
                    assert tc.check_claims(host, claims) == [], (case, D, n, form)
                    assert tr.same_bits(host, ref), (case, D, n, form, "host form")
                    for k, p in enumerate(ptrs):
                        assert tr.same_bits(gpu.trace_scores_device(0, p, n, D), ref), (case, D, n, form, "device, base + %d floats" % k)
    buf.free()


@functools.lru_cache(maxsize=None)
def noise():
    return np.random.default_rng(22).standard_normal((1 << 24) + 5, dtype=np.float32)


@pytest.fixture(scope="module")
def noise_on_device(gpu):
    buf = gpu.DeviceBuffer.from_numpy(0, noise())
    yield buf
    buf.free()


@pytest.mark.parametrize("D", [4410, 1 << 20])
def test_white_noise_fields_exact_sums_within_the_bound(gpu, noise_on_device, D):
    x = noise()
    ref = tr.trace(x, D)
    bs, bq = tr.sum_bound(x, D)
    buf = noise_on_device
    natural = None
    for form in (0, 1, 2):
        with forced_form(gpu, form):
            got = gpu.trace_scores_device(0, buf.ptr, x.size, D)
        assert tr.same_fields(got, ref), (D, form)
        es, eq = np.abs(got["sum"] - ref["sum"]), np.abs(got["sumsq"] - ref["sumsq"])
        print("D %d form %d: max |sum - ref| / bound %.3g, max |sumsq - ref| / bound %.3g" % (D, form, (es / bs).max(), (eq / bq).max()))
        assert np.all(es <= bs) and np.all(eq <= bq), (D, form)
        if form == 0:
            natural = got
    # the natural form is one of the two: its records are that form's, bit for bit
    with forced_form(gpu, 1 if D <= gpu.AM_TRACE_WAVE_BIN_MAX else 2):
        assert tr.same_bits(gpu.trace_scores_device(0, buf.ptr, x.size, D), natural)
    # ... and the host form equals the device form
    assert tr.same_bits(gpu.trace_scores(x[:3 * D + 17], D), gpu.trace_scores_device(0, buf.ptr, 3 * D + 17, D))


def test_sums_are_added_in_the_order_the_header_documents(gpu):
    """Rounding sums (white noise, scaled so that the f64 sums do round): every record equals, bit for bit, the numpy
    model of the header's order (trace_ref.trace_ordered) -- one span per bin up to AM_TRACE_WAVE_BIN_MAX and under
    trace_form 1, slices from the bin's start beyond it and under trace_form 2."""
    W, SL = gpu.AM_TRACE_WAVE_BIN_MAX, gpu.AM_TRACE_SLICE
    x = (noise()[:150001].astype(np.float64) * np.exp(noise()[150001:300002].astype(np.float64) * 4)).astype(np.float32)
    x[::1013] = np.nan
    buf = gpu.DeviceBuffer(0, 4 * 4 * (x.size + 8))
    ptrs = upload_at_every_alignment(gpu, buf, x)
    rounds = False
    for D in (1, 3, 255, 256, 257, 1000, W, W + 1, 4410, SL, SL + 1, 2 * SL + 1, 5 * SL + 7, x.size):
        n = min(x.size, 2000 * D + 17)                     # (a few thousand bins say as much as all of them)
        for form in (0, 1, 2):
            sliced = form == 2 or (form == 0 and D > W)
            want = tr.trace_ordered(x[:n], D, sliced, SL)
            rounds = rounds or not tr.same_bits(want, tr.trace(x[:n], D))
            with forced_form(gpu, form):
                for k in (0, 3):
                    assert tr.same_bits(gpu.trace_scores_device(0, ptrs[k], n, D), want), (D, form, k)
    assert rounds                                          # (the data does make the order matter)
    buf.free()


def test_sums_do_not_depend_on_the_alignment_or_the_other_bins(gpu):
    """Rounding sums (white noise): the same scores at another address, at another alignment and with other bins around
    them give the same bits, under every form."""
    x = noise()[:200000]
    buf = gpu.DeviceBuffer(0, 4 * 4 * (x.size + 8))
    ptrs = upload_at_every_alignment(gpu, buf, x)
    for D in (100, 2048, 4410, 8192, 30000):
        for form in (0, 1, 2):
            with forced_form(gpu, form):
                base = gpu.trace_scores_device(0, ptrs[0], x.size, D)
                for p in ptrs[1:]:
                    assert tr.same_bits(gpu.trace_scores_device(0, p, x.size, D), base), (D, form)
                # bins 2 .. 4 traced as an array of their own
                part = gpu.trace_scores_device(0, ptrs[0] + 4 * 2 * D, 3 * D, D)
                assert tr.same_bits(part, base[2:5]), (D, form)
    buf.free()


def test_capacity(gpu):
    x = noise()[:1000]
    ref = tr.trace(x, 64)
    out = np.zeros(8, dtype=gpu.TRACE_BIN_DTYPE)
    n = C.c_size_t(0)
    buf = gpu.DeviceBuffer.from_numpy(0, x)
    for call in (lambda: gpu.lib().am_trace_scores(0, x.ctypes.data, x.size, 64, out.ctypes.data, 5, C.byref(n)),
                 lambda: gpu.lib().am_trace_scores_device(0, buf.ptr, x.size, 64, out.ctypes.data, 5, C.byref(n))):
        out[:] = 0
        n.value = 0
        assert call() == gpu.AM_ERR_CAPACITY
        assert n.value == 16 == ref.size
        assert tr.same_fields(out[:5], ref[:5]) and not out[5:].tobytes().strip(b"\0")
    n.value = 7
    assert gpu.lib().am_trace_scores(0, x.ctypes.data, x.size, 64, None, 0, C.byref(n)) == gpu.AM_ERR_CAPACITY and n.value == 16
    assert gpu.lib().am_trace_scores(0, None, 0, 64, None, 0, C.byref(n)) == 0 and n.value == 0          # no scores: no bins
    for rc in (gpu.lib().am_trace_scores(0, None, 10, 64, out.ctypes.data, 8, C.byref(n)),
               gpu.lib().am_trace_scores(0, x.ctypes.data, 10, 64, None, 8, C.byref(n)),
               gpu.lib().am_trace_scores(0, x.ctypes.data, 10, 64, out.ctypes.data, 8, None),
               gpu.lib().am_trace_scores(0, x.ctypes.data, 10, 0, out.ctypes.data, 8, C.byref(n)),
               gpu.lib().am_trace_scores_device(0, buf.ptr, 10, (1 << 30) + 1, out.ctypes.data, 8, C.byref(n))):
        assert rc == gpu.AM_ERR_INVALID_ARG
    buf.free()


# ---- match forms -----------------------------------------------------------------------------------------------------
def planted(seed, n, gains):
    rng = np.random.default_rng(seed)
    needle = rng.uniform(-0.5, 0.5, S).astype(np.float32)
    hay = rng.uniform(-0.25, 0.25, n).astype(np.float32)
    offs = sorted(int(t) for t in rng.choice(np.arange(1, n // (4 * S)), size=len(gains), replace=False) * 4 * S + rng.integers(0, S, len(gains)))
    for t, g in zip(offs, gains):
        hay[t:t + S] += np.float32(g) * needle
    return needle, hay, offs


def correlate_device(gpu, algo, ptr, length, scale):
    """The AM_MODE_VALID scores am_correlate_device writes for the resident f32 samples."""
    n = length - S + 1
    out = gpu.DeviceBuffer(0, 4 * n)
    got = C.c_size_t(0)
    rc = gpu.lib().am_correlate_device(algo._h, ptr, length, int(gpu.Mode.Valid), int(scale), out.ptr, n, C.byref(got))
    assert rc == 0 and got.value == n, gpu.lib().am_last_error_string()
    y = out.to_numpy(np.float32, n)
    out.free()
    return y


def check_against_scores(got, scores, D, what):
    ref = tr.trace(scores, D)
    assert tr.same_fields(got, ref), what
    bs, bq = tr.sum_bound(scores, D)
    assert np.all(np.abs(got["sum"] - ref["sum"]) <= bs) and np.all(np.abs(got["sumsq"] - ref["sumsq"]) <= bq), what


BINS = (1000, SR, 50000)       # the wave form, one slice per bin, several slices per bin


@pytest.mark.parametrize("norm", [False, True])
def test_match_trace_equals_trace_of_correlate(gpu, norm):
    needle, hay, offs = planted(31, 230000, [0.9, 1.3, 0.6])
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    algo = gpu.HipConvolve(needle, score_norm=norm)
    for scale in ((gpu.Scale.LIB,) if norm else (gpu.Scale.LIB, gpu.Scale.NONE)):
        scores = correlate_device(gpu, algo, buf.ptr, hay.size, scale)
        for D in BINS:
            dev = algo.match_trace_device(buf.ptr, hay.size, gpu.trace_params(D, scale))
            check_against_scores(dev, scores, D, (norm, int(scale), D))
            assert tr.same_bits(algo.match_trace(hay, D, scale), dev), (norm, int(scale), D)      # host form = device form
    # the trace's global maximum is where am_match_best puts its best hit
    scores = correlate_device(gpu, algo, buf.ptr, hay.size, gpu.Scale.LIB)
    best = algo.match_best_device(buf.ptr, hay.size, gpu.best_params(1, 0, 0.0))
    for D in BINS:
        st = gpu.trace_summary(algo.match_trace_device(buf.ptr, hay.size, gpu.trace_params(D)), D)
        assert st.argmax == best[0].start == offs[1], (D, st.argmax, best[0].start, offs)
        assert np.float32(st.max) == np.float32(best[0].height) == scores[offs[1]]
    if norm:
        assert abs(scores[offs[1]]) <= 1.0 + 1e-5
    algo.close(); buf.free()


def test_pcm16_stereo_takes_the_downmix(gpu):
    rng = np.random.default_rng(8)
    needle, hay, _ = planted(32, 150000, [0.9, 1.2])
    st = np.stack([hay * 20000, hay * 20000 + rng.normal(0, 300, hay.size)], axis=1).clip(-32768, 32767).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(st)
    b16, b32 = gpu.DeviceBuffer.from_numpy(0, st), gpu.DeviceBuffer.from_numpy(0, mono)
    for norm in (False, True):
        algo = gpu.HipConvolve(needle, score_norm=norm)
        scores = correlate_device(gpu, algo, b32.ptr, mono.size, gpu.Scale.LIB)
        for D in BINS:
            dev = algo.match_trace_device(b16.ptr, mono.size, gpu.trace_params(D), fmt=gpu.Fmt.S16_STEREO)
            check_against_scores(dev, scores, D, (norm, D))
            assert tr.same_bits(dev, algo.match_trace_device(b32.ptr, mono.size, gpu.trace_params(D))), (norm, D)
            assert tr.same_bits(dev, algo.match_trace(st, D)), (norm, D)
        algo.close()
    b16.free(); b32.free()


def test_several_blocks_and_a_tail_block(gpu):
    """log_n = 13 (hop 4193): a haystack of 300 000 samples spans 71 blocks, the last one part-filled."""
    needle, hay, _ = planted(33, 300000, [1.0, 0.7, 1.2])
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    for log_n in (13, 14):
        algo = gpu.HipConvolve(needle)
        algo.set_option("log_n", log_n)
        scores = correlate_device(gpu, algo, buf.ptr, hay.size, gpu.Scale.LIB)
        for D in BINS:
            check_against_scores(algo.match_trace_device(buf.ptr, hay.size, gpu.trace_params(D)), scores, D, (log_n, D))
        algo.close()
    buf.free()


def test_a_nan_stretch_costs_its_windows(gpu):
    needle, hay, _ = planted(34, 200000, [0.9, 1.1])
    hay[100000:100010] = np.nan
    hay[150000] = np.inf
    hay[150000 + S - 5] = np.nan                      # a finite stretch shorter than the needle between them: no score
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    algo = gpu.HipConvolve(needle)
    scores = np.full(hay.size - S + 1, np.nan, dtype=np.float32)
    fin = np.isfinite(hay)
    edges = np.flatnonzero(np.diff(np.concatenate(([False], fin, [False])).astype(np.int8)))
    for a, b in zip(edges[::2], edges[1::2]):         # one am_correlate_device call per finite stretch
        if b - a >= S:
            scores[a:b - S + 1] = correlate_device(gpu, algo, buf.ptr + 4 * int(a), int(b - a), gpu.Scale.LIB)
    assert np.isnan(scores).sum() == (S + 9) + (2 * S - 5)
    for D in BINS:
        dev = algo.match_trace_device(buf.ptr, hay.size, gpu.trace_params(D))
        check_against_scores(dev, scores, D, D)
        assert int(dev["count"].sum()) == int((~np.isnan(scores)).sum())
        assert tr.same_bits(dev, algo.match_trace(hay, D)), D
    algo.close(); buf.free()


def test_shortest_haystacks(gpu):
    needle, hay, _ = planted(35, 100000, [1.0])
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    for D in (1, SR, 1 << 30):
        one = algo.match_trace_device(buf.ptr, S, gpu.trace_params(D))
        score = correlate_device(gpu, algo, buf.ptr, S, gpu.Scale.LIB)
        assert one.size == 1 and int(one["count"][0]) == 1 and one["max"][0] == one["min"][0] == score[0]
        assert tr.same_bits(one, algo.match_trace(hay[:S], D))
        assert algo.match_trace_device(buf.ptr, S - 1, gpu.trace_params(D)).size == 0       # shorter than the needle: 0 bins
        assert algo.match_trace(hay[:S - 1], D).size == 0
    n = C.c_size_t(5)
    tp = gpu.trace_params(SR)
    assert gpu.lib().am_match_trace_device(algo._h, buf.ptr, S - 1, 0, C.byref(tp), None, 0, C.byref(n)) == 0 and n.value == 0
    algo.close(); buf.free()


def test_batch_equals_singles(gpu):
    needle, _, _ = planted(36, 100000, [1.0])
    hays = [planted(40 + i, n, [0.8, 1.1])[1] for i, n in enumerate((120000, 100000, 260000, 100000))]
    hays[1] = hays[1][:S - 10]                         # shorter than the needle: no bins
    hays[3] = hays[3][:S]                              # one score
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    for norm in (False, True):
        algo = gpu.HipConvolve(needle, score_norm=norm)
        for D in BINS:
            tp = gpu.trace_params(D)
            batch = algo.match_trace_batch_device([b.ptr for b in bufs], [h.size for h in hays], tp)
            singles = [algo.match_trace_device(b.ptr, h.size, tp) for b, h in zip(bufs, hays)]
            assert [r.size for r in batch] == [tr.n_bins(max(0, h.size - S + 1), D) for h in hays]
            assert all(tr.same_bits(x, y) for x, y in zip(batch, singles)), (norm, D)
        # too few slots per haystack: what fits, every count, AM_ERR_CAPACITY
        tp = gpu.trace_params(1000)
        out = np.zeros(4 * 3, dtype=gpu.TRACE_BIN_DTYPE)
        counts = (C.c_size_t * 4)()
        rc = gpu.lib().am_match_trace_batch_device(algo._h, (C.c_void_p * 4)(*[b.ptr for b in bufs]), (C.c_size_t * 4)(*[h.size for h in hays]),
                                                   4, 0, C.byref(tp), out.ctypes.data, 3, counts)
        assert rc == gpu.AM_ERR_CAPACITY and list(counts) == [117, 0, 257, 1]
        singles = [algo.match_trace_device(b.ptr, h.size, tp) for b, h in zip(bufs, hays)]
        assert tr.same_bits(out[0:3], singles[0][:3]) and tr.same_bits(out[6:9], singles[2][:3]) and tr.same_bits(out[9:10], singles[3])
        algo.close()
    for b in bufs:
        b.free()


def test_errors(gpu):
    needle, hay, _ = planted(37, 100000, [1.0])
    algo = gpu.HipConvolve(needle)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    L, h, bad = gpu.lib(), algo._h, gpu.AM_ERR_INVALID_ARG
    out = np.zeros(200, dtype=gpu.TRACE_BIN_DTYPE)
    n = C.c_size_t(0)
    ok = gpu.trace_params(SR)

    def both(tp, fmt=0, hay_host=hay.ctypes.data, hay_dev=buf.ptr, o=out.ctypes.data, np_=C.byref(n)):
        tpp = C.byref(tp) if tp is not None else None
        return (L.am_match_trace(h, hay_host, hay.size, fmt, tpp, o, out.size, np_),
                L.am_match_trace_device(h, hay_dev, hay.size, fmt, tpp, o, out.size, np_))

    assert both(ok) == (0, 0) and n.value == tr.n_bins(hay.size - S + 1, SR)
    assert both(None) == (bad, bad)                                           # null pointers with work to do
    assert both(ok, hay_host=None, hay_dev=None) == (bad, bad)
    assert both(ok, o=None) == (bad, bad)
    assert both(ok, np_=None) == (bad, bad)
    assert both(gpu.trace_params(0)) == (bad, bad)                            # the bin
    assert both(gpu.trace_params((1 << 30) + 1)) == (bad, bad)
    assert b"bin" in L.am_last_error_string()
    assert both(gpu.AmTraceParams(bin=SR, scale=int(gpu.Scale.LIB), reserved=1)) == (bad, bad)
    assert b"reserved" in L.am_last_error_string()
    assert both(ok, fmt=7) == (bad, bad)                                      # an unknown format
    assert both(gpu.trace_params(SR, gpu.Scale.MY)) == (bad, bad)
    assert b"AM_SCALE_MY" in L.am_last_error_string()
    assert L.am_match_trace_device(h, hay.ctypes.data, hay.size, 0, C.byref(ok), out.ctypes.data, out.size, C.byref(n)) == bad   # not on the needle's device
    assert b"device" in L.am_last_error_string()
    ptrs, lens, counts = (C.c_void_p * 2)(buf.ptr, None), (C.c_size_t * 2)(hay.size, hay.size), (C.c_size_t * 2)()
    assert L.am_match_trace_batch_device(h, ptrs, lens, 2, 0, C.byref(ok), out.ctypes.data, 100, counts) == bad
    assert b"haystack 1" in L.am_last_error_string()
    assert L.am_match_trace_batch_device(h, None, lens, 2, 0, C.byref(ok), out.ctypes.data, 100, counts) == bad
    assert L.am_match_trace_batch_device(h, ptrs, lens, 0, 0, C.byref(ok), None, 0, None) == 0          # no haystacks: nothing to do
    ncc = gpu.HipConvolve(needle, score_norm=True)
    with pytest.raises(gpu.AudioMatchError) as e:                             # NCC scores need AM_SCALE_LIB
        ncc.match_trace(hay, SR, scale=gpu.Scale.NONE)
    assert e.value.code == bad
    with pytest.raises(gpu.AudioMatchError):
        gpu.set_option("trace_form", 3)
    assert gpu.get_option("trace_form") == 0
    ncc.close(); algo.close(); buf.free()
