"""Host form == _device form, bit for bit, for every entry-point pair that shares the upload / residency steps.

The host form uploads the caller's bytes into the context's input buffer and runs the code the _device form runs, so
the two must agree in every byte.  What would break that: a wrong byte count (the f32 / i16-stereo sizes), a missing
wait behind the upload, a stale input buffer.  Hence, per pair and within one test: haystacks of 4099, then 12289, then
1031 elements (the input buffer grows, then is larger than the input, where a short upload leaves the previous call's
samples behind), both sample formats where the call takes one, a needle planted at the very end of the haystack, and
host arrays that are fresh allocations released as soon as the call returns.
"""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 257
LENS = (4099, 12289, 1031)
F32, S16 = 0, 1
SR = 8000


def needle():
    return np.random.default_rng(1).uniform(-1, 1, S).astype(np.float32)


def signal(n, fmt, seed=0):
    """A fresh array: noise with the needle at a fifth of it and over its last samples; f32, or (n, 2) i16 whose down-mix holds it"""
    rng = np.random.default_rng(1000 * seed + n)
    x = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    for t in (n // 5, n - S - 5):
        x[t:t + S] += 0.5 * needle()
    if fmt == F32:
        return x
    left = np.round(x * 40000.0)
    return np.stack([left + rng.integers(-300, 300, n), left - rng.integers(-300, 300, n)], axis=1).astype(np.int16)


def scores(n, seed=0):
    rng = np.random.default_rng(77 * seed + n)
    y = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    y[[n // 7, n // 2, n - 1]] += (1.0, 0.8, 0.9)
    return y


def bits(v):
    """The bytes of a result: numpy arrays, Peak lists and tuples / lists of those"""
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, (list, tuple)):
        return b"|".join(bits(e) for e in v)
    if hasattr(v, "prominence"):
        return struct.pack("<QQff", v.start, v.end, v.height, v.prominence)
    return bytes(v)


def both(gpu, make, host_call, device_call, what):
    """host_call(a fresh host array, released right behind the call) == device_call(its resident copy); the host result"""
    got = host_call(make())
    buf = gpu.DeviceBuffer.from_numpy(0, make())
    try:
        want = device_call(buf.ptr)
    finally:
        buf.free()
    assert len(bits(want)) > 0 and bits(got) == bits(want), what
    return got


def params(gpu):
    return gpu.AmMatchParams(sr=SR, chunk=2000, overlap=S, min_prominence=0.13, min_distance=300, overshadow_distance_s=300 / SR,
                             scale=int(gpu.Scale.LIB))


@pytest.mark.parametrize("mode", ["Valid", "Same"])
def test_correlate(gpu, mode):
    algo, L, m = gpu.HipConvolve(needle()), gpu.lib(), int(gpu.Mode[mode])
    for n in LENS:
        def device(ptr):
            cnt = C.c_size_t(0)
            gpu._check(L.am_correlate_len(n, S, m, C.byref(cnt)))
            out = gpu.DeviceBuffer(0, 4 * cnt.value)
            gpu._check(L.am_correlate_device(algo._h, ptr, n, m, 1, out.ptr, cnt.value, C.byref(cnt)))
            return out.to_numpy(np.float32, cnt.value)
        both(gpu, lambda: signal(n, F32), lambda x: algo.correlate_with_sample(x, gpu.Mode[mode], True), device, (mode, n))


def test_match_and_match_pcm16(gpu):
    algo, p = gpu.HipConvolve(needle()), params(gpu)
    for n in LENS:
        got = both(gpu, lambda: signal(n, F32), lambda x: algo.match(x, p), lambda ptr: algo.match_device(ptr, n, p), n)
        assert any(pk.start > n - 2 * S for pk in got), (n, got)   # (the plant at the end: a short upload loses it)
        got = both(gpu, lambda: signal(n, S16), lambda x: algo.match_pcm16(x, p), lambda ptr: algo.match_pcm16_device(ptr, n, p), n)
        assert any(pk.start > n - 2 * S for pk in got), (n, got)


@pytest.mark.parametrize("fmt", [F32, S16])
def test_multi_varlen_against_its_batch_form(gpu, fmt):
    algos, p = [gpu.HipConvolve(needle()), gpu.HipConvolve(needle()[:131])], params(gpu)
    for n in LENS:
        both(gpu, lambda: signal(n, fmt), lambda x: gpu.match_multi_varlen(algos, x, p),
             lambda ptr: gpu.match_multi_varlen_batch_device(algos, [ptr], [n], p, fmt)[0], n)


def test_find_peaks_top_trace_scores_probe_scores(gpu):
    for n in LENS:
        both(gpu, lambda: scores(n), lambda y: gpu.find_peaks_top(y, 5, 0.1, 10), lambda ptr: gpu.find_peaks_top_device(0, ptr, n, 5, 0.1, 10), n)
        both(gpu, lambda: scores(n), lambda y: gpu.trace_scores(y, 500), lambda ptr: gpu.trace_scores_device(0, ptr, n, 500), n)
        both(gpu, lambda: scores(n), lambda y: np.array([gpu.probe_scores(y, 3, 40, 25)]),
             lambda ptr: np.array([gpu.probe_scores_device(0, ptr, n, 3, 40, 25)]), n)


@pytest.mark.parametrize("fmt", [F32, S16])
def test_match_best_and_match_trace(gpu, fmt):
    algo = gpu.HipConvolve(needle())
    bp, tp = gpu.best_params(4, 100), gpu.trace_params(500)
    for n in LENS:
        both(gpu, lambda: signal(n, fmt), lambda x: algo.match_best(x, 4, 100), lambda ptr: algo.match_best_device(ptr, n, bp, fmt), n)
        both(gpu, lambda: signal(n, fmt), lambda x: algo.match_trace(x, 500), lambda ptr: algo.match_trace_device(ptr, n, tp, fmt), n)


@pytest.mark.parametrize("fmt", [F32, S16])
def test_discover(gpu, fmt):
    """len_a 4099, len_b 6007: recording B starts at a 256-byte boundary of the input buffer that is not 4 * len_a"""
    dp = gpu.discover_params(512, 256)
    la, lb = 4099, 6007

    def make_b():
        b = signal(lb, fmt, seed=3)
        b[2500:4000] = signal(la, fmt)[1000:2500]
        return b
    got = bits(gpu.discover(signal(la, fmt), make_b(), dp))
    da, db = gpu.DeviceBuffer.from_numpy(0, signal(la, fmt)), gpu.DeviceBuffer.from_numpy(0, make_b())
    want = bits(gpu.discover_device(0, da.ptr, la, db.ptr, lb, dp, fmt))
    assert got == want and len(want) == 15 * gpu.PROBE_HIT_DTYPE.itemsize


@pytest.mark.parametrize("fmt", [F32, S16])
def test_envelope_and_match_envelope(gpu, fmt):
    ep = gpu.env_params(gpu.band_edges_log(SR, 8, 150.0, 3000.0, 4))
    grid = gpu.env_grid(0.0, 0)   # (one speed: a needle of 257 samples holds one frame of 256)
    algo = gpu.HipConvolve(needle())
    for n in LENS:
        both(gpu, lambda: signal(n, fmt), lambda x: gpu.envelope(x, ep, 1500.0), lambda ptr: gpu.envelope_device(0, ptr, n, ep, 1500.0, fmt), n)
        both(gpu, lambda: signal(n, fmt), lambda x: algo.match_envelope(x, ep, grid, -1.0),
             lambda ptr: algo.match_envelope_device(ptr, n, ep, grid, -1.0, fmt), n)


def test_envelope_scores(gpu):
    rng = np.random.default_rng(5)
    mats = [rng.integers(0, 1000, (4, j)).astype(np.uint16) for j in (6, 9)]
    bank = np.concatenate([m.reshape(-1) for m in mats])
    for n in LENS:
        jh = n // 64
        hay = np.random.default_rng(n).integers(0, 1000, (4, jh)).astype(np.uint16)
        got = gpu.envelope_scores(mats, hay.copy())
        db, dh = gpu.DeviceBuffer.from_numpy(0, bank), gpu.DeviceBuffer.from_numpy(0, hay)
        want = gpu.envelope_scores_device(0, db.ptr, [6, 9], 4, dh.ptr, jh)
        assert bits(got) == bits(want) and want[0].size == want[1].size == jh - 5, n


@pytest.mark.parametrize("fmt", [F32, S16])
def test_lag_products_fir_resample(gpu, fmt):
    taps = np.array([1.0, -0.6, 0.3, -0.1, 0.05], np.float32)
    for n in LENS:
        both(gpu, lambda: signal(n, fmt), lambda x: gpu.lag_products(x, 8), lambda ptr: gpu.lag_products_device(0, ptr, n, 8, fmt), n)

        def fir_device(ptr):
            out = gpu.DeviceBuffer(0, 4 * n)
            return out.to_numpy(np.float32, gpu.fir_device(0, ptr, n, taps, out.ptr, n, 3, fmt))
        assert both(gpu, lambda: signal(n, fmt), lambda x: gpu.fir(x, taps, 3), fir_device, n).size == n - 3
        for src, dst in ((44100, 48000), (44100, 44100)):
            def resample_device(ptr):
                cap = gpu.resample_len(n, src, dst)
                out = gpu.DeviceBuffer(0, 4 * cap)
                return out.to_numpy(np.float32, gpu.resample_device(0, ptr, n, src, dst, out.ptr, cap, fmt))
            both(gpu, lambda: signal(n, fmt), lambda x: gpu.resample(x, src, dst), resample_device, (n, src, dst))


def test_stereo_down_mix(gpu):
    L = gpu.lib()
    for n in LENS:
        def mono_device(ptr):
            out = gpu.DeviceBuffer(0, 4 * n)
            gpu._check(L.am_pcm_s16_stereo_to_mono_device(0, ptr, n, out.ptr))
            return out.to_numpy(np.float32, n)

        def mix_device(ptr):
            out = gpu.DeviceBuffer(0, 4 * n)
            gpu.pcm_s16_stereo_mix_device(0, ptr, n, 0.75, -0.25, out.ptr)
            return out.to_numpy(np.float32, n)
        both(gpu, lambda: signal(n, S16), gpu.pcm_s16_stereo_to_mono, mono_device, n)
        both(gpu, lambda: signal(n, S16), lambda x: gpu.pcm_s16_stereo_mix(x, 0.75, -0.25), mix_device, n)
