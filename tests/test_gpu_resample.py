"""Sample-rate conversion on the GPU (am_resample*, am_needle_create_resampled) against the f64 checker of
tests/resample_ref.py, bit identity across entry points, non-finite samples, a full-size hour and matching across
rates end to end."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as ref

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (48000, 44100), (44100, 22050), (22050, 44100), (8000, 11025), (11025, 32000), (96000, 44100),
         (384000, 8000)]


def tol_ok(y, x64, src, dst, **kw):
    want = ref.resample(x64, src, dst, **kw)
    assert y.shape == want.shape
    scale = max(np.abs(x64).max(), 1e-30)
    err = np.abs(y.astype(np.float64) - want).max() if y.size else 0.0
    assert err <= 1e-5 * scale, (src, dst, err / scale)


@pytest.mark.parametrize("src,dst", PAIRS)
def test_against_checker(gpu, src, dst):
    rng = np.random.default_rng(src ^ dst)
    L, M, H = ref.ratio(src, dst)
    short = max(1, (2 * H) // max(L, M) // 2)            # shorter than the filter's span of input samples
    for n in (1, short, 3001, 10 * src):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        y = gpu.resample(x, src, dst)
        assert y.size == ref.out_len(n, src, dst)
        tol_ok(y, x, src, dst)
    for n in (3001, 10 * src):                           # i16 stereo: down-mixed on load
        lr = rng.integers(-32768, 32767, size=2 * n).astype(np.int16)
        y = gpu.resample(lr.reshape(-1, 2), src, dst)
        tol_ok(y, ref.downmix(lr), src, dst)
        assert np.array_equal(y.view(np.uint32), gpu.resample(gpu.pcm_s16_stereo_to_mono(lr), src, dst).view(np.uint32))


def test_large_ratio_r1280(gpu):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(20001).astype(np.float32)
    tol_ok(gpu.resample(x, 11025, 32000), x, 11025, 32000)
    tol_ok(gpu.resample(x, 32000, 11025), x, 32000, 11025)


def test_equal_rates_are_the_input_bits(gpu):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(5001).astype(np.float32)
    x[17] = np.nan
    assert np.array_equal(gpu.resample(x, 48000, 48000).view(np.uint32), x.view(np.uint32))
    lr = rng.integers(-32768, 32767, size=2 * 5001).astype(np.int16)
    assert np.array_equal(gpu.resample(lr, 44100, 44100).view(np.uint32), gpu.pcm_s16_stereo_to_mono(lr).view(np.uint32))


def test_host_and_device_forms_agree(gpu):
    rng = np.random.default_rng(2)
    n = 100003
    x = rng.standard_normal(n + 1).astype(np.float32)
    for src, dst in ((44100, 48000), (48000, 44100), (96000, 44100)):
        m = ref.out_len(n, src, dst)
        din = gpu.DeviceBuffer.from_numpy(0, x)
        dout = gpu.DeviceBuffer(0, 4 * m)
        assert gpu.resample_device(0, din.ptr, n, src, dst, dout.ptr, m) == m
        host = gpu.resample(x[:n], src, dst)
        assert np.array_equal(dout.to_numpy(np.float32, m).view(np.uint32), host.view(np.uint32))
        # a source that is not 16-byte aligned takes the scalar staging loads: same bits
        assert gpu.resample_device(0, din.ptr + 4, n, src, dst, dout.ptr, m) == m
        assert np.array_equal(dout.to_numpy(np.float32, m).view(np.uint32), gpu.resample(x[1:], src, dst).view(np.uint32))
        lr = rng.integers(-32768, 32767, size=2 * n).astype(np.int16)
        dl = gpu.DeviceBuffer.from_numpy(0, lr)
        assert gpu.resample_device(0, dl.ptr, n, src, dst, dout.ptr, m, fmt=gpu.Fmt.S16_STEREO) == m
        assert np.array_equal(dout.to_numpy(np.float32, m).view(np.uint32), gpu.resample(lr, src, dst).view(np.uint32))
        # capacity: nothing written, the required length reported
        got = C.c_size_t(0)
        rc = gpu.lib().am_resample_device(0, din.ptr, n, 0, src, dst, dout.ptr, m - 1, C.byref(got))
        assert rc == gpu.AM_ERR_CAPACITY and got.value == m
        for b in (din, dout, dl):
            b.free()


def test_nonfinite_reaches_exactly_its_support(gpu):
    rng = np.random.default_rng(3)
    n = 40000
    x = rng.standard_normal(n).astype(np.float32)
    x[1234], x[20000], x[n - 1] = np.nan, np.inf, -np.inf
    for src, dst in ((48000, 44100), (44100, 48000), (22050, 44100)):
        y = gpu.resample(x, src, dst)
        want = ref.resample(x, src, dst)
        assert np.array_equal(np.isfinite(y), np.isfinite(want)), (src, dst)
        assert (~np.isfinite(y)).sum() > 0
        ok = np.isfinite(want)
        xf = np.where(np.isfinite(x), x, 0).astype(np.float64)
        assert np.abs(y[ok] - want[ok]).max() <= 1e-5 * np.abs(xf).max()


def test_resampled_needle_equals_needle_of_resampled(gpu):
    rng = np.random.default_rng(4)
    src, dst = 44100, 48000
    needle = rng.uniform(-0.5, 0.5, 2 * src).astype(np.float32)
    a = gpu.HipConvolve.resampled(needle, src, dst)
    b = gpu.HipConvolve(gpu.resample(needle, src, dst))
    assert a.sample_len == b.sample_len == ref.out_len(needle.size, src, dst)
    hay = rng.uniform(-0.05, 0.05, 70 * dst).astype(np.float32)
    for off in (5 * dst + 3, 31 * dst, 55 * dst + 101):
        hay[off:off + b.sample_len] += gpu.resample(needle, src, dst)
    p = gpu.Config(chunk_size_s=20.0, overlap_length_s=2.0, distance_s=10.0, prominence=0.13).params(dst, gpu.Scale.LIB)
    pa, pb = a.match(hay, p), b.match(hay, p)
    assert [(q.start, q.height) for q in pa] == [(q.start, q.height) for q in pb] and len(pa) == 3
    d = gpu.DeviceBuffer.from_numpy(0, hay)
    assert a.match_batch_device([d.ptr, d.ptr], [hay.size] * 2, p) == b.match_batch_device([d.ptr, d.ptr], [hay.size] * 2, p)
    sa, sb = a.hit_scores(hay, pa), b.hit_scores(hay, pb)
    assert [(s.position, s.ncc, s.gain) for s in sa] == [(s.position, s.ncc, s.gain) for s in sb]
    lr = np.clip(np.repeat(hay[:, None], 2, axis=1) * 65535, -32768, 32767).astype(np.int16)
    for h in (a, b):
        h.set_option("half_pipeline", 2)
    assert [(q.start, q.height) for q in a.match_pcm16(lr, p)] == [(q.start, q.height) for q in b.match_pcm16(lr, p)]
    for h in (a, b):
        h.set_option("half_pipeline", -1)
        h.set_option("score_norm", 1)
    na, nb = a.match(hay, p), b.match(hay, p)
    assert [(q.start, q.height) for q in na] == [(q.start, q.height) for q in nb] and len(na) == 3
    c = gpu.HipConvolve.resampled(needle, src, dst, score_norm=True)
    assert [(q.start, q.height) for q in c.match(hay, p)] == [(q.start, q.height) for q in na]
    # i16 needle: the handle of the down-mix, resampled
    nlr = rng.integers(-20000, 20000, size=2 * 3000).astype(np.int16)
    e = gpu.HipConvolve.resampled(nlr, src, dst)
    f = gpu.HipConvolve(gpu.resample(gpu.pcm_s16_stereo_to_mono(nlr), src, dst))
    assert e.sample_len == f.sample_len and e.inverse_sample_auto_correlation() == f.inverse_sample_auto_correlation()
    d.free()


def tones(rate, n, freqs, phases, amps, t0=0.0):
    t = t0 + np.arange(n, dtype=np.float64) / rate
    return (amps[None, :] * np.sin(2 * np.pi * freqs[None, :] * t[:, None] + phases[None, :])).sum(axis=1)


@pytest.mark.parametrize("src,dst", [(44100, 48000), (48000, 44100)])
def test_end_to_end_across_rates(gpu, src, dst):
    """A band-limited needle rendered at src is found in a dst haystack holding the same tones rendered at dst."""
    rng = np.random.default_rng(src)
    k = 150
    freqs = rng.uniform(100.0, 8000.0, k)
    phases = rng.uniform(0, 2 * np.pi, k)
    amps = rng.uniform(0.2, 1.0, k)
    dur = 2.0
    needle = tones(src, int(dur * src), freqs, phases, amps)
    needle = (needle / np.abs(needle).max() * 0.5).astype(np.float32)
    level = np.sqrt(np.mean(needle.astype(np.float64) ** 2))
    planted = tones(dst, int(dur * dst), freqs, phases, amps)
    planted = planted / np.abs(tones(src, int(dur * src), freqs, phases, amps)).max() * 0.5
    hay_len = 95 * dst + 12345
    hay = rng.standard_normal(hay_len) * level * 0.1           # 20 dB below the needle
    plants = [7 * dst + 11, 41 * dst + 3, hay_len - planted.size - 2 * dst - 7]   # the last one in the haystack's tail
    for off in plants:
        hay[off:off + planted.size] += planted
    hay = hay.astype(np.float32)
    p = gpu.Config(chunk_size_s=20.0, overlap_length_s=dur, distance_s=10.0, prominence=0.13).params(dst, gpu.Scale.LIB)
    a = gpu.HipConvolve.resampled(needle, src, dst)
    p.overlap = a.sample_len
    hits = a.match(hay, p)
    assert [q.start for q in hits] == plants, [q.start for q in hits]
    for s, off in zip(a.hit_scores(hay, hits), plants):
        assert s.ncc >= 0.99 and abs(s.position - off) <= 0.1, (s, off)
    plain = gpu.HipConvolve(needle)                              # the needle at the wrong rate
    p.overlap = plain.sample_len
    got = plain.match(hay, p)
    assert not ({q.start for q in got} & set(plants)), [q.start for q in got]
    if got:
        assert max(s.ncc for s in plain.hit_scores(hay, got)) < 0.5


def test_full_size_hour_i16(gpu):
    """One hour of 48 kHz i16 stereo -> 44.1 kHz through am_resample_device, 16 spans against the checker (the last one
    and one past k M = 2^32 among them)."""
    src, dst = 48000, 44100
    L, M, H = ref.ratio(src, dst)
    frames = 3600 * src
    n_out = ref.out_len(frames, src, dst)
    din = gpu.synth_pcm16_stereo_device(0, frames, 11, 3, amp=0.5)
    dout = gpu.DeviceBuffer(0, 4 * n_out)
    assert gpu.resample_device(0, din.ptr, frames, src, dst, dout.ptr, n_out, fmt=gpu.Fmt.S16_STEREO) == n_out
    rng = np.random.default_rng(5)
    span = 4096
    starts = sorted(set([0, n_out - span, (1 << 32) // M + 17] + list(rng.integers(0, n_out - span, 13))))
    assert any(s * M >= 1 << 32 for s in starts) and len(starts) == 16
    for k0 in starts:
        k0 = int(k0)
        y = np.empty(span, np.float32)
        gpu.lib().am_memcpy_d2h(0, y.ctypes.data, dout.ptr + 4 * k0, 4 * span)
        n0 = max(0, (k0 * M - H) // L - 1)
        n1 = min(frames, ((k0 + span) * M + H) // L + 2)
        lr = np.empty(2 * (n1 - n0), np.int16)
        gpu.lib().am_memcpy_d2h(0, lr.ctypes.data, din.ptr + 4 * n0, 4 * (n1 - n0))
        x = ref.downmix(lr)
        want = ref.resample(x, src, dst, k0, k0 + span, n0=n0, n_in=frames)
        assert np.abs(y - want).max() <= 1e-5 * max(1e-30, np.abs(x).max()), k0
    din.free()
    dout.free()


def test_after_shutdown_and_errors(gpu):
    x = np.random.default_rng(6).standard_normal(9000).astype(np.float32)
    first = gpu.resample(x, 44100, 48000)
    assert gpu.lib().am_shutdown() == 0
    assert np.array_equal(gpu.resample(x, 44100, 48000).view(np.uint32), first.view(np.uint32))
    h = gpu.HipConvolve.resampled(x, 44100, 48000)
    assert h.sample_len == first.size
    with pytest.raises(gpu.AudioMatchError) as e:
        gpu.resample(x, 44100, 0)
    assert e.value.code == gpu.AM_ERR_INVALID_ARG and "rates must be in 1..768000" in str(e.value)
    with pytest.raises(gpu.AudioMatchError) as e:
        gpu.HipConvolve.resampled(x, 8193, 1)
    assert e.value.code == gpu.AM_ERR_INVALID_ARG and "8193 > 8192" in str(e.value)
    with pytest.raises(gpu.AudioMatchError) as e:
        gpu.resample(x, 44100, 48000, device=999)
    assert e.value.code in (gpu.AM_ERR_NO_DEVICE, gpu.AM_ERR_INVALID_ARG, gpu.AM_ERR_HIP)
