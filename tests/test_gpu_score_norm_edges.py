"""Window energies of score_norm (csrc/am_norm.hip), exact at every tile, block and path edge.

a. The energy of every window, recovered from two score arrays of the same correlation (designed spike signals,
   score_norm_ref.spike_case), against an exact f64 window sum.
b. Planted needles with guard spikes directly outside or inside the window (score_norm_ref.plant_case) through every
   match entry point, against the f64 checker.
test_score_norm_design_host.py checks both designs without a device."""
import ctypes as C

import numpy as np
import pytest

import score_norm_ref as ref
from score_norm_ref import assert_peaks, bits, match_ref, ncc_ref

pytestmark = pytest.mark.gpu

SR = ref.SR


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


# ---- a. energy recovered from two score arrays ---------------------------------------------------------------------
@pytest.mark.parametrize("s", ref.SPIKE_S)
def test_window_energy_from_two_arrays(gpu, s):
    """Two handles on one needle correlate the same signal:
        plain, LIB scale:   lib = fl(v a),                 a = f32(1 / en)        (inverse_sample_auto_correlation)
        score_norm:         ncc = fl(fl(v b) / sqrt(E)),   b = f32(1 / sqrt(en))  (norm_factor), the division in f64
    v is the same f32 value in both: the plan, the needle's bits and the kernels are the same, and the factor enters as
    ONE f32 multiply of the finished value on every path these lengths take -- correlate_direct (needles of at most 64
    samples: acc * out_scale) and the generic column kernel k3_cols_inv_gen (v * out_scale + 0, whole problems under 2^19
    samples never reach the register-kernel plans, which fold the factor into a twiddle); f32 pipeline, so hs.k3(factor)
    is the factor; no partitioned needles.  Hence
        E = (lib / ncc)^2 (b / a)^2
    up to three f32 roundings per factor, squared: 6 u.  The bound is 16 u = 9.5e-7 (score_norm_ref.ENERGY_BOUND); a
    window one sample too short or too long is off by 3.9e-3 or more (the design test asserts 1e-3, 1000 bounds).
    The signal's window energies are integers below 2^8 on both sides, so E itself carries no error; en is summed in
    another order on the device, which moves b by an ulp at the most (2 u more).
    Every score is compared: where E > 0 the correlation is at least 0.25 (positive needle), where E = 0 the score
    must be exactly 0.  The spike cases leave empty windows to short needles only; the gap cases (score_norm_ref.gap_signal)
    have a run of them for every length, bounded by windows with one spike on their first or last sample."""
    needle = ref.spike_needle(s)
    plain, normed = gpu.HipConvolve(needle), gpu.HipConvolve(needle, score_norm=True)
    a = np.float32(plain.inverse_sample_auto_correlation())
    a_host, b = ref.scale_pair(float(np.sum(needle.astype(np.float64) ** 2)))
    assert abs(float(a) / float(a_host) - 1.0) <= 2 * ref.U
    worst, zeros, gap_zeros = 0.0, 0, 0
    cases = [(False, mode, ref.spike_signal(s, w, mode)) for w in ref.spike_widths(s) for mode in ref.SPIKE_MODES]
    cases += [(True, mode, ref.gap_signal(s, mode)) for mode in ref.SPIKE_MODES]
    for gap, mode, within in cases:
        w = len(within)
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        E = ref.window_energy(within, s, lead, n)
        lib = plain.correlate_with_sample(within, gpu.Mode(mode), True)
        ncc = normed.correlate_with_sample(within, gpu.Mode(mode), True)
        assert lib.shape == ncc.shape == E.shape
        assert np.all(np.isfinite(lib)) and np.all(np.isfinite(ncc))
        pos = E > 0
        assert pos.any() and np.all(lib[pos] != 0) and np.all(ncc[pos] != 0), (w, mode)
        assert np.all(ncc[~pos] == 0.0), (w, mode, np.flatnonzero(ncc[~pos] != 0)[:8])
        if gap:
            assert np.count_nonzero(~pos) >= ref.GAP_EXTRA + 1
            gap_zeros += int(np.count_nonzero(~pos))
        else:
            assert (~pos).any() or not ref.zero_windows_expected(s, n)
            zeros += int(np.count_nonzero(~pos))
        err = np.abs(ref.recovered_energy(lib[pos], ncc[pos], a, b) / E[pos] - 1.0)
        k = int(np.argmax(err))
        print("s = %d, w = %d%s, mode %d: %d scores, %d of energy 0, worst energy error %.3g = %.2f bounds (score %d)"
              % (s, w, " (gap)" if gap else "", mode, n, np.count_nonzero(~pos), err[k], err[k] / ref.ENERGY_BOUND, np.flatnonzero(pos)[k]))
        assert err[k] <= ref.ENERGY_BOUND, (w, mode, int(np.flatnonzero(pos)[k]), float(E[pos][k]), float(err[k]))
        worst = max(worst, float(err[k]))
    print("s = %d: worst energy error %.3g = %.2f of the bound, %d + %d windows of energy 0" % (s, worst, worst / ref.ENERGY_BOUND, zeros, gap_zeros))
    assert (zeros > 0) == (s <= ref.MAX_ZERO_RUN) and gap_zeros >= 3 * (ref.GAP_EXTRA + 1)


@pytest.mark.parametrize("s,mode", [(300, ref.MODE_SAME), (4097, ref.MODE_FULL), (8193, ref.MODE_VALID)])
def test_correlate_device_bits(gpu, s, mode):
    """am_correlate_device on resident samples: the bits of am_correlate."""
    w = ref.spike_widths(s)[-1]
    needle, within = ref.spike_case(s, w, mode)
    n = ref.mode_len(w, s, mode)
    algo = gpu.HipConvolve(needle, score_norm=True)
    host = algo.correlate_with_sample(within, gpu.Mode(mode), True)
    src, dst = gpu.DeviceBuffer.from_numpy(0, within), gpu.DeviceBuffer(0, 4 * n)
    try:
        got_n = C.c_size_t(0)
        gpu._check(gpu.lib().am_correlate_device(algo._h, C.c_void_p(src.ptr), w, mode, int(gpu.Scale.LIB), C.c_void_p(dst.ptr), n, C.byref(got_n)))
        assert got_n.value == n == host.size
        dev = dst.to_numpy(np.float32, n)
    finally:
        src.free()
        dst.free()
    assert dev.tobytes() == host.tobytes()
    assert np.count_nonzero(dev) > 0


# ---- b. plants with guard spikes through every match path ----------------------------------------------------------
plant_setup = ref.plant_setup


def report(name, got, exp):
    d = max([abs(g.height - e[2]) for g, e in zip(got, exp)] + [abs(g.prominence - e[3]) for g, e in zip(got, exp)] + [0.0])
    print("%s: %d hits, worst height / prominence error %.3g" % (name, len(got), d))


@pytest.mark.parametrize("S", ref.PLANT_S)
def test_plants_match_and_device(gpu, oracle, S):
    needle, hays, exps, plants, p = plant_setup(gpu, oracle, S)
    algo = gpu.HipConvolve(needle, score_norm=True)
    got = algo.match(hays[0], p)
    report("match", got, exps[0])
    assert_peaks(got, exps[0])
    buf = gpu.DeviceBuffer.from_numpy(0, hays[0])
    try:
        dev = algo.match_device(buf.ptr, hays[0].size, p)
    finally:
        buf.free()
    assert_peaks(dev, exps[0])
    assert bits(dev) == bits(got)


@pytest.mark.parametrize("S", ref.PLANT_S)
def test_plants_batch_and_pool(gpu, oracle, opts, S):
    needle, hays, exps, plants, p = plant_setup(gpu, oracle, S)
    algo = gpu.HipConvolve(needle, score_norm=True)
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
    try:
        batch = algo.match_batch_device([b.ptr for b in bufs], [h.size for h in hays], p)
        single = [algo.match_device(b.ptr, h.size, p) for b, h in zip(bufs, hays)]
    finally:
        for b in bufs:
            b.free()
    for k, (got, exp) in enumerate(zip(batch, exps)):
        report("batch %d" % k, got, exp)
        assert_peaks(got, exp)
    assert [bits(x) for x in batch] == [bits(x) for x in single]
    opts("score_norm", 1)   # (pool needles follow the process default)
    pool = gpu.Pool(needle, devices=[0, 0])
    try:
        pooled = pool.match_batch(hays, p)
    finally:
        pool.close()
    for got, exp in zip(pooled, exps):
        assert_peaks(got, exp)
    assert [bits(x) for x in pooled] == [bits(x) for x in batch]


@pytest.mark.parametrize("S", ref.PLANT_S)
def test_plants_pcm16(gpu, oracle, S):
    """The i16 form of the window sum (short2 loads, down-mix in the load) against the checker run on the library's
    down-mix of the same frames: its first absolute check."""
    needle, hays, _, plants, p = plant_setup(gpu, oracle, S)
    frames = [ref.stereo(h) for h in hays]
    monos = [gpu.pcm_s16_stereo_to_mono(f) for f in frames]
    assert all(m.size == h.size for m, h in zip(monos, hays))
    exps = [match_ref(oracle, m, needle, p) for m in monos]
    assert [e[0] for e in exps[0]] == [t for t, _ in plants]
    algo = gpu.HipConvolve(needle, score_norm=True)
    got = algo.match_pcm16(frames[0], p)
    report("pcm16", got, exps[0])
    assert_peaks(got, exps[0])
    bufs = [gpu.DeviceBuffer.from_numpy(0, f) for f in frames]
    try:
        dev = algo.match_pcm16_device(bufs[0].ptr, len(frames[0]), p)
        batch = algo.match_pcm16_batch_device([b.ptr for b in bufs], [len(f) for f in frames], p)
        single = [algo.match_pcm16_device(b.ptr, len(f), p) for b, f in zip(bufs, frames)]
    finally:
        for b in bufs:
            b.free()
    assert bits(dev) == bits(got)
    for k, (g, e) in enumerate(zip(batch, exps)):
        report("pcm16 batch %d" % k, g, e)
        assert_peaks(g, e)
    assert [bits(x) for x in batch] == [bits(x) for x in single]


@pytest.mark.parametrize("S", ref.PLANT_S)
def test_plants_match_best(gpu, oracle, S):
    """The k best of the whole haystack's scores (one array, no chunks), k = the number of plants: the two on the
    array's ends are no peaks, the others come back, the best first."""
    needle, hays, _, plants, p = plant_setup(gpu, oracle, S)
    y, _, _ = ncc_ref(oracle, hays[0], needle, oracle.MODE_VALID)
    k = len(ref.plant_offsets(S))
    assert k == len(plants) + 2
    got = gpu.HipConvolve(needle, score_norm=True).match_best(hays[0], k, min_distance=p.min_distance, min_prominence=ref.PLANT_PROMINENCE)
    assert sorted(q.start for q in got) == [t for t, _ in plants]
    assert [q.height for q in got] == sorted((q.height for q in got), reverse=True)
    d = max(abs(q.height - y[q.start]) for q in got)
    print("match_best: worst height error %.3g" % d)
    assert d <= 1e-4
    pk = oracle.find_peaks(y.astype(np.float32), ref.PLANT_PROMINENCE, p.min_distance)
    assert sorted(e[0] for e in pk) == [t for t, _ in plants]
