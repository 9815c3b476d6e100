"""Masked matching through every entry point that takes score_norm, against the f64 checker of mask_ref.py.

The needles of score_norm_ref (S = 2000: every kept span on the local-scan path; S = 8000: the 40 % gap leaves spans of
2400 samples, so both sizes scan locally and differ in plan and chunk geometry) on a 90 s haystack; every plant's gap is
overwritten by noise 20 dB above the needle.  Plants sit on tile and block edges, on a chunk seam and on the first and
last window (mask_ref.plant_case).  With the mask every plant is found; the zero-filled needle without a mask finds none."""
import ctypes as C

import numpy as np
import pytest

import mask_ref as mr
import score_norm_ref as ref
from score_norm_ref import assert_peaks, bits

pytestmark = pytest.mark.gpu


def report(name, got, exp):
    d = max([abs(g.height - e[2]) for g, e in zip(got, exp)] + [abs(g.prominence - e[3]) for g, e in zip(got, exp)] + [0.0])
    print("%s: %d hits, worst height / prominence error %.3g" % (name, len(got), d))


@pytest.fixture
def bufs(gpu):
    made = []

    def up(arrays):
        made.extend(gpu.DeviceBuffer.from_numpy(0, a) for a in arrays)
        return made[-len(arrays):]
    yield up
    for b in made:
        b.free()


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_checker_finds_every_plant(gpu, oracle, S):
    needle, gaps, hays, exps, inner, p = mr.plant_setup(gpu, oracle, S)
    assert [e[0] for e in exps[0]] == inner and len(inner) == 7
    assert all(e[2] > 0.97 for e in exps[0])
    assert len(exps[1]) >= 1 and len(exps[2]) >= 1


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_match_forms(gpu, oracle, bufs, S):
    """am_match, am_match_device and am_match_batch_device (a batch of 3): the checker's peaks within assert_peaks'
    tolerance, and one set of bits."""
    needle, gaps, hays, exps, inner, p = mr.plant_setup(gpu, oracle, S)
    algo = gpu.HipConvolve(needle, gaps=gaps, score_norm=True)
    host = [algo.match(h, p) for h in hays]
    for k, (got, exp) in enumerate(zip(host, exps)):
        report("match %d" % k, got, exp)
        assert_peaks(got, exp)
    assert [q.start for q in host[0]] == inner
    d = bufs(hays)
    single = [algo.match_device(b.ptr, h.size, p) for b, h in zip(d, hays)]
    batch = algo.match_batch_device([b.ptr for b in d], [h.size for h in hays], p)
    assert [bits(x) for x in single] == [bits(x) for x in host] == [bits(x) for x in batch]


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_without_the_mask_no_plant_is_found(gpu, oracle, S):
    """The caller's old way: the needle zero-filled by hand, no mask, score_norm.  The denominator is the whole window's
    energy, a plant scores about 0.12 and none reaches the prominence bound.  (Fails without masked matching: the
    masked handle of the other tests does not exist.)"""
    needle, gaps, hays, exps, inner, p = mr.plant_setup(gpu, oracle, S)
    plain = gpu.HipConvolve(mr.zero_filled(needle, gaps), score_norm=True).match(hays[0], p)
    assert not set(q.start for q in plain) & set(inner), plain
    masked = gpu.HipConvolve(needle, gaps=gaps, score_norm=True).match(hays[0], p)
    assert [q.start for q in masked] == inner


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_pcm16(gpu, oracle, bufs, S):
    """The i16 stereo forms against the checker run on the library's own down-mix of the frames."""
    needle, gaps, hays, _, inner, p = mr.plant_setup(gpu, oracle, S)
    frames = [ref.stereo(h) for h in hays]
    monos = [gpu.pcm_s16_stereo_to_mono(f) for f in frames]
    exps = [mr.match_ref(oracle, m, needle, gaps, p) for m in monos]
    assert [e[0] for e in exps[0]] == inner
    algo = gpu.HipConvolve(needle, gaps=gaps, score_norm=True)
    got = algo.match_pcm16(frames[0], p)
    report("pcm16", got, exps[0])
    assert_peaks(got, exps[0])
    d = bufs(frames)
    dev = algo.match_pcm16_device(d[0].ptr, len(frames[0]), p)
    batch = algo.match_pcm16_batch_device([b.ptr for b in d], [len(f) for f in frames], p)
    single = [algo.match_pcm16_device(b.ptr, len(f), p) for b, f in zip(d, frames)]
    assert bits(dev) == bits(got)
    for g, e in zip(batch, exps):
        assert_peaks(g, e)
    assert [bits(x) for x in batch] == [bits(x) for x in single]


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_match_best(gpu, oracle, bufs, S):
    """am_match_best alone and in a batch of 3: the inner plants, the best first, heights as the checker's."""
    needle, gaps, hays, _, inner, p = mr.plant_setup(gpu, oracle, S)
    y, _, _ = mr.mncc_ref(oracle, hays[0], needle, gaps, oracle.MODE_VALID)
    k = len(inner) + 2
    algo = gpu.HipConvolve(needle, gaps=gaps, score_norm=True)
    got = algo.match_best(hays[0], k, min_distance=p.min_distance, min_prominence=ref.PLANT_PROMINENCE)
    assert sorted(q.start for q in got) == inner
    assert [q.height for q in got] == sorted((q.height for q in got), reverse=True)
    worst = max(abs(q.height - y[q.start]) for q in got)
    print("match_best: worst height error %.3g" % worst)
    assert worst <= 1e-4
    bp = gpu.best_params(k, p.min_distance, ref.PLANT_PROMINENCE)
    d = bufs(hays)
    single = [algo.match_best_device(b.ptr, h.size, bp) for b, h in zip(d, hays)]
    batch = algo.match_best_batch_device([b.ptr for b in d], [h.size for h in hays], bp)
    assert bits(single[0]) == bits(got)
    assert [bits(x) for x in batch] == [bits(x) for x in single]
    assert all(len(x) >= 1 for x in batch)


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_trace_and_correlate_device_agree_with_host(gpu, oracle, bufs, S):
    """am_match_trace and am_correlate_device on resident samples: the bits of their host forms; the correlation's
    scores are the checker's."""
    needle, gaps, hays, _, inner, p = mr.plant_setup(gpu, oracle, S)
    hay = hays[1]
    algo = gpu.HipConvolve(needle, gaps=gaps, score_norm=True)
    n = hay.size - S + 1
    host = algo.correlate_with_sample(hay, gpu.Mode.Valid, True)
    y, E, thr = mr.mncc_ref(oracle, hay, needle, gaps, oracle.MODE_VALID)
    clear = (E >= thr * (1 + 1e-9))
    assert clear.all() and np.max(np.abs(host - y)) <= 1e-4
    src, = bufs([hay])
    dst = gpu.DeviceBuffer(0, 4 * n)
    try:
        got_n = C.c_size_t(0)
        gpu._check(gpu.lib().am_correlate_device(algo._h, C.c_void_p(src.ptr), hay.size, int(gpu.Mode.Valid), int(gpu.Scale.LIB),
                                                 C.c_void_p(dst.ptr), n, C.byref(got_n)))
        assert got_n.value == n
        assert dst.to_numpy(np.float32, n).tobytes() == host.tobytes()
    finally:
        dst.free()
    bin_ = 4000
    t_host = algo.match_trace(hay, bin_)
    t_dev = algo.match_trace_device(src.ptr, hay.size, gpu.trace_params(bin_))
    assert t_host.tobytes() == t_dev.tobytes() and len(t_host) == gpu.trace_len(n, bin_)
    assert float(np.max(t_host["max"])) > 0.97


@pytest.mark.parametrize("S", mr.PLANT_S)
def test_no_gaps_is_the_ordinary_handle(gpu, oracle, bufs, S):
    """A handle made with n_gaps = 0 gives the bits of am_needle_create on every one of these calls."""
    needle, _, hays, _, _, p = mr.plant_setup(gpu, oracle, S)
    hay = hays[1]
    a, b = gpu.HipConvolve(needle, score_norm=True), gpu.HipConvolve(needle, gaps=[], score_norm=True)
    assert b.mask() == []
    d = bufs(hays)
    bp = gpu.best_params(5, p.min_distance, 0.05)
    frames = ref.stereo(hay)
    calls = [
        lambda h: h.correlate_with_sample(hay[:3 * S + 5000], gpu.Mode.Same, True).tobytes(),
        lambda h: bits(h.match(hay, p)),
        lambda h: bits(h.match_device(d[1].ptr, hay.size, p)),
        lambda h: [bits(x) for x in h.match_batch_device([x.ptr for x in d], [x.size for x in hays], p)],
        lambda h: bits(h.match_pcm16(frames, p)),
        lambda h: bits(h.match_best(hay, 5, min_distance=p.min_distance, min_prominence=0.05)),
        lambda h: [bits(x) for x in h.match_best_batch_device([x.ptr for x in d], [x.size for x in hays], bp)],
        lambda h: h.match_trace(hay, 4000).tobytes(),
    ]
    for k, fn in enumerate(calls):
        assert fn(a) == fn(b), k
    assert np.float32(a.inverse_sample_auto_correlation()).tobytes() == np.float32(b.inverse_sample_auto_correlation()).tobytes()
