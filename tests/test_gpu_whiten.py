"""Spectral whitening on the GPU (am_lag_products*, am_fir*, am_needle_create_filtered) against the f64 checker of
tests/whiten_ref.py: tolerances, bit identities across entry points, alignments and sample formats, non-finite samples,
filtering in pieces, and matching in coloured noise end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import whiten_ref as ref

pytestmark = pytest.mark.gpu

ORDERS = (1, 7, 64)
TAP_COUNTS = (1, 2, 5, 33, 65)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def lag_signal(n):
    return np.random.default_rng(1000 + n).uniform(-1, 1, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lag_reference(n):
    """(r, mag) at order 64 of lag_signal(n): computed once, shared by the tests"""
    return ref.lag_products(lag_signal(n), 64)


def lag_sizes(gpu, order):
    B = gpu.LAG_BLOCK
    return sorted({1, order, order + 1, B - 1, B, B + 1, 3 * B + 17})


@pytest.mark.parametrize("order", ORDERS)
def test_lag_products_against_fsum(gpu, order):
    for n in lag_sizes(gpu, order):
        x = lag_signal(n)
        want, mag = lag_reference(n)
        got = gpu.lag_products(x, order)
        assert got.shape == (order + 1,)
        err = np.abs(got - want[:order + 1])
        bound = ref.lag_bound(n, mag[:order + 1])
        print(f"order {order} n {n}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all(), (order, n, err, bound)
        if n <= order:
            assert (got[n:] == 0.0).all()          # lags that reach in front of the signal


def test_lag_products_bit_identities(gpu):
    B = gpu.LAG_BLOCK
    rng = np.random.default_rng(11)
    for n in (1, 65, B + 1, 3 * B + 17):
        x = lag_signal(n)
        full = gpu.lag_products(x, 64)
        for order in (1, 7, 8, 32):                   # r[k] does not depend on the order asked for
            assert np.array_equal(bits(gpu.lag_products(x, order)), bits(full[:order + 1])), (n, order)
        d = gpu.DeviceBuffer.from_numpy(0, np.concatenate([np.zeros(1, np.float32), x]))
        # a device pointer that is not 16-byte aligned takes the scalar staging loads: same bits
        assert np.array_equal(bits(gpu.lag_products_device(0, d.ptr + 4, n, 64)), bits(full)), n
        d.free()
        d = gpu.DeviceBuffer.from_numpy(0, x)
        assert np.array_equal(bits(gpu.lag_products_device(0, d.ptr, n, 64)), bits(full)), n
        d.free()
        lr = rng.integers(-32768, 32767, size=2 * n).astype(np.int16)
        mono = ref.downmix(lr)
        assert np.array_equal(bits(mono), bits(gpu.pcm_s16_stereo_to_mono(lr)))
        want = gpu.lag_products(mono, 64)
        assert np.array_equal(bits(gpu.lag_products(lr.reshape(-1, 2), 64)), bits(want)), n
        dl = gpu.DeviceBuffer.from_numpy(0, lr)
        assert np.array_equal(bits(gpu.lag_products_device(0, dl.ptr, n, 64, fmt=gpu.Fmt.S16_STEREO)), bits(want)), n
        dl.free()


def test_lag_products_nonfinite_count_as_zero_and_add_up(gpu):
    B = gpu.LAG_BLOCK
    n = 2 * B + 301
    x = lag_signal(n).copy()
    z = x.copy()
    for i, v in ((0, np.nan), (B - 1, np.inf), (B, -np.inf), (B + 70, np.nan), (n - 1, np.inf)):
        x[i], z[i] = v, 0.0
    got = gpu.lag_products(x, 64)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(gpu.lag_products(z, 64)))
    want, mag = ref.lag_products(x, 64)
    assert (np.abs(got - want) <= ref.lag_bound(n, mag)).all()
    # additivity: the r of a file with at least `order` zeros behind it and the r of the next add up to the r of both
    a, b = lag_signal(3000), lag_signal(B + 1)
    both = np.concatenate([a, np.zeros(64, np.float32), b])
    ra, rb, rab = gpu.lag_products(a, 64), gpu.lag_products(b, 64), gpu.lag_products(both, 64)
    _, mag = ref.lag_products(both, 64)
    assert (np.abs(ra + rb - rab) <= 2 * ref.lag_bound(both.size, mag)).all()


@functools.lru_cache(maxsize=None)
def fir_case(n_taps):
    """(x, taps): the longest signal of the size list and random taps, shared by the FIR tests"""
    rng = np.random.default_rng(77 + n_taps)
    return rng.uniform(-1, 1, 3 * 2048 + 5 + 64).astype(np.float32), rng.uniform(-1, 1, n_taps).astype(np.float32)


def fir_bound(taps, x):
    """n_taps products and n_taps additions, each rounded once in f32 (u = 2^-24): (n_taps + 1) u sum|taps| max|x|"""
    return (len(taps) + 1) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * float(np.abs(x).max() if x.size else 0.0)


@pytest.mark.parametrize("n_taps", TAP_COUNTS)
def test_fir_against_checker(gpu, n_taps):
    W = gpu.FIR_TILE
    assert 3 * W + 5 <= fir_case(n_taps)[0].size
    xs, taps = fir_case(n_taps)
    for n in sorted({1, n_taps - 1, n_taps, W - 1, W, W + 1, 3 * W + 5}):
        x = xs[:n]
        y = gpu.fir(x, taps)
        assert y.shape == (n,) and y.dtype == np.float32
        if n == 0:
            continue
        err = np.abs(y.astype(np.float64) - ref.fir(x, taps)).max()
        print(f"n_taps {n_taps} n {n}: error {err:.3g}, bound {fir_bound(taps, x):.3g}")
        assert err <= fir_bound(taps, x), (n_taps, n, err)


@pytest.mark.parametrize("n_taps", TAP_COUNTS)
def test_fir_pieces_are_the_bits_of_the_whole(gpu, n_taps):
    W = gpu.FIR_TILE
    x, taps = fir_case(n_taps)
    n = 3 * W + 5
    x = x[:n]
    full = gpu.fir(x, taps)
    for a in sorted({1, n_taps - 2, n_taps - 1, W - 1, W, W + 1} - {-1, 0}):
        l = min(a, n_taps - 1)
        for b in (a + 1, a + W + 3, n):
            piece = gpu.fir(x[a - l:b], taps, lead=l)
            assert piece.size == b - a and np.array_equal(bits(piece), bits(full[a:b])), (n_taps, a, b)


def test_fir_same_bits_across_entry_points(gpu):
    W = gpu.FIR_TILE
    rng = np.random.default_rng(21)
    n = 3 * W + 5
    for n_taps in (2, 33, 65):
        x, taps = fir_case(n_taps)
        x = x[:n + 1]
        host = gpu.fir(x[:n], taps)
        din = gpu.DeviceBuffer.from_numpy(0, x)
        dout = gpu.DeviceBuffer(0, 4 * (n + 1))
        assert gpu.fir_device(0, din.ptr, n, taps, dout.ptr, n) == n
        assert np.array_equal(bits(dout.to_numpy(np.float32, n)), bits(host))
        # neither pointer 16-byte aligned: the scalar staging loads and stores, same bits
        assert gpu.fir_device(0, din.ptr + 4, n, taps, dout.ptr + 4, n) == n
        assert np.array_equal(bits(dout.to_numpy(np.float32, n + 1)[1:]), bits(gpu.fir(x[1:], taps)))
        # lead on the device form
        assert gpu.fir_device(0, din.ptr, n, taps, dout.ptr, n, lead=7) == n - 7
        assert np.array_equal(bits(dout.to_numpy(np.float32, n - 7)), bits(gpu.fir(x[:n], taps, lead=7)))
        # capacity: the length reported, nothing written
        before = dout.to_numpy(np.float32, n + 1)
        got = C.c_size_t(0)
        t = np.ascontiguousarray(taps)
        rc = gpu.lib().am_fir_device(0, din.ptr, n, 0, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, 3, dout.ptr, n - 4, C.byref(got))
        assert rc == gpu.AM_ERR_CAPACITY and got.value == n - 3
        assert np.array_equal(bits(dout.to_numpy(np.float32, n + 1)), bits(before))
        out = np.full(8, 3.0, np.float32)
        rc = gpu.lib().am_fir(0, x.ctypes.data, 100, 0, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, 0, out.ctypes.data, 8, C.byref(got))
        assert rc == gpu.AM_ERR_CAPACITY and got.value == 100 and (out == 3.0).all()
        # i16 stereo: the bits of the f32 down-mix
        lr = rng.integers(-32768, 32767, size=2 * n).astype(np.int16)
        want = gpu.fir(gpu.pcm_s16_stereo_to_mono(lr), taps)
        assert np.array_equal(bits(gpu.fir(lr.reshape(-1, 2), taps)), bits(want))
        dl = gpu.DeviceBuffer.from_numpy(0, lr)
        assert gpu.fir_device(0, dl.ptr, n, taps, dout.ptr, n, fmt=gpu.Fmt.S16_STEREO) == n
        assert np.array_equal(bits(dout.to_numpy(np.float32, n)), bits(want))
        assert np.abs(want.astype(np.float64) - ref.fir(ref.downmix(lr), taps)).max() <= fir_bound(taps, ref.downmix(lr))
        for b in (din, dout, dl):
            b.free()


@pytest.mark.parametrize("n_taps", TAP_COUNTS)
def test_fir_one_nan_reaches_exactly_n_taps_outputs(gpu, n_taps):
    W = gpu.FIR_TILE
    x, taps = fir_case(n_taps)
    n = 3 * W + 5
    clean = gpu.fir(x[:n], taps)
    for at in (0, W - 3, W, 2 * W + 100, n - 1):
        for v in (np.nan, np.inf):
            z = x[:n].copy()
            z[at] = v
            y = gpu.fir(z, taps)
            hit = np.zeros(n, bool)
            hit[at:at + n_taps] = True
            assert not np.isfinite(y[hit]).any(), (n_taps, at)
            assert hit.sum() == min(n_taps, n - at)
            assert np.array_equal(bits(y[~hit]), bits(clean[~hit])), (n_taps, at)


def test_fir_identity_and_preemphasis(gpu):
    x = fir_case(1)[0].copy()
    x[5], x[6] = 0.0, -0.0
    y = gpu.fir(x, [1.0])
    assert (y == x).all()                    # (== and not the bits: -0 comes back as +0 from 0 + 1 * x)
    alpha = np.float32(0.95)
    y = gpu.fir(x, [1.0, -alpha])
    want = x.astype(np.float64)
    want[1:] -= float(alpha) * x[:-1].astype(np.float64)
    assert np.abs(y - want).max() <= fir_bound(np.array([1.0, alpha], np.float32), x)


def test_needle_create_filtered(gpu):
    rng = np.random.default_rng(31)
    needle = rng.uniform(-0.5, 0.5, 4099).astype(np.float32)
    taps = fir_case(33)[1]
    a = gpu.HipConvolve.filtered(needle, taps)
    b = gpu.HipConvolve(gpu.fir(needle, taps))
    n = C.c_size_t(0)
    assert gpu.lib().am_needle_len(a._h, C.byref(n)) == 0 and n.value == needle.size == a.sample_len == b.sample_len
    assert a.inverse_sample_auto_correlation() == b.inverse_sample_auto_correlation()
    window = rng.uniform(-1, 1, 20011).astype(np.float32)
    for scale in (False, True):
        assert np.array_equal(bits(a.correlate_with_sample(window, gpu.Mode.Valid, scale)),
                              bits(b.correlate_with_sample(window, gpu.Mode.Valid, scale)))
    lr = rng.integers(-20000, 20000, size=2 * 3000).astype(np.int16)
    e = gpu.HipConvolve.filtered(lr, taps)
    f = gpu.HipConvolve(gpu.fir(gpu.pcm_s16_stereo_to_mono(lr), taps))
    assert e.sample_len == f.sample_len == 3000
    assert np.array_equal(bits(e.correlate_with_sample(window)), bits(f.correlate_with_sample(window)))
    with pytest.raises(gpu.AudioMatchError) as err:
        gpu.HipConvolve.filtered(needle, np.zeros(66, np.float32))
    assert err.value.code == gpu.AM_ERR_INVALID_ARG


def correlate_device(gpu, algo, d_hay, n):
    m = n - algo.sample_len + 1
    dout = gpu.DeviceBuffer(0, 4 * m)
    got = C.c_size_t(0)
    rc = gpu.lib().am_correlate_device(algo._h, d_hay.ptr, n, int(gpu.Mode.Valid), int(gpu.Scale.LIB), dout.ptr, m, C.byref(got))
    assert rc == 0 and got.value == m
    out = dout.to_numpy(np.float32, m)
    dout.free()
    return out


def test_end_to_end_coloured_noise(gpu):
    """AR(1) noise with rho = 0.98 (8 kHz, 60 000 samples), a 4096-sample needle of the same process planted at 30011 with
    gain 0.5.  In f64 on the CPU this seed gives (largest score at least S away from the hit) / (score at the hit) =
    0.747 raw and 0.129 whitened (order 8, noise_db 60): whitening must at least halve the ratio."""
    S, N, T, sr = 4096, 60000, 30011, 8000
    rng = np.random.default_rng(5)
    hay = ref.ar1(rng, N, 0.98)
    needle = ref.ar1(rng, S, 0.98)
    hay[T:T + S] += 0.5 * needle
    hay, needle = hay.astype(np.float32), needle.astype(np.float32)
    d_hay = gpu.DeviceBuffer.from_numpy(0, hay)
    d_white = gpu.DeviceBuffer(0, 4 * N)
    r = gpu.lag_products_device(0, d_hay.ptr, N, 8)
    taps = gpu.whiten_taps(r, 60.0)
    assert taps[0] == 1.0 and abs(taps[1] + 0.98) < 0.02       # AR(1): the filter is close to {1, -rho}
    assert gpu.fir_device(0, d_hay.ptr, N, taps, d_white.ptr, N) == N
    raw_algo, white_algo = gpu.HipConvolve(needle), gpu.HipConvolve.filtered(needle, taps)
    u = np.arange(N - S + 1)
    far = np.abs(u - T) >= S
    ratios = []
    for algo, d in ((raw_algo, d_hay), (white_algo, d_white)):
        c = correlate_device(gpu, algo, d, N).astype(np.float64)
        assert int(np.argmax(c)) == T
        ratios.append(c[far].max() / c[T])
    print(f"side ratio raw {ratios[0]:.3f}, whitened {ratios[1]:.3f}")
    assert ratios[1] <= 0.5 * ratios[0], ratios
    p = gpu.Config(chunk_size_s=4.0, overlap_length_s=S / sr, distance_s=1.0, prominence=0.25).params(sr, gpu.Scale.LIB)
    hits = white_algo.match_device(d_white.ptr, N, p)
    assert [q.start for q in hits] == [T], hits
    assert [q.start for q in white_algo.match(gpu.fir(hay, taps), p)] == [T]
    d_hay.free()
    d_white.free()
