"""The resampling kernel (am_resample.hip) on designed inputs: every kernel form (input span staged in LDS or not,
table staged or not, f32 or i16 source) and geometry regime (L above the work-item cap, both factors near 8192, a staged
span next to its cap, an odd W, table rows without padding) across two workgroup edges and a partial last workgroup.

  impulses     one tap per output: exact zeros outside every support, a h[idx] to one f32 rounding inside, the same bits
               wherever the same tap meets the same amplitude, and from every entry point
  non-finite   NaN and +-Inf on the first and last sample each edge output reads, just outside them, on the staged
               span's first and last quad and at both signal ends reach exactly their supports
  random       noise of the four lengths mod 4 against the f64 checker, i16 bit-identical to its down-mix
  long filters tens of thousands of taps per output within the header's 1e-5 max |x|

resample_ref.geometry places the inputs and words the failures; every expected value is the f64 checker's."""
import functools

import numpy as np
import pytest

import resample_ref as ref

pytestmark = pytest.mark.gpu

KINDS = ("f32", "i16")
BOUND = 1e-5            # include/audiomatch.h: max |y - y_f64| <= 1e-5 max |x|


@functools.lru_cache(maxsize=None)
def taps(src, dst):
    h = ref.taps(src, dst)
    h.setflags(write=False)
    return h


def bits(y):
    return np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)


def device_forms(gpu, x, src, dst, n_out):
    """am_resample_device on x (f32, or (frames, 2) i16): from a 16-byte aligned source and from one offset by a sample
    (the scalar staging loads)."""
    fmt = gpu.Fmt.S16_STEREO if x.dtype == np.int16 else gpu.Fmt.F32_MONO
    n_in = x.shape[0]
    flat = np.ascontiguousarray(x).reshape(-1)
    per = flat.size // max(n_in, 1)                                  # elements per sample or frame (4 bytes either way)
    lead = np.full(per, 12345, flat.dtype)
    din = gpu.DeviceBuffer.from_numpy(0, np.concatenate([lead, flat]))
    dout = gpu.DeviceBuffer(0, 4 * n_out)
    try:
        assert gpu.resample_device(0, din.ptr + 4, n_in, src, dst, dout.ptr, n_out, fmt=fmt) == n_out
        off = dout.to_numpy(np.float32, n_out)
        gpu.lib().am_memcpy_h2d(0, din.ptr, flat.ctypes.data, flat.nbytes)
        assert gpu.resample_device(0, din.ptr, n_in, src, dst, dout.ptr, n_out, fmt=fmt) == n_out
        return dout.to_numpy(np.float32, n_out), off
    finally:
        din.free()
        dout.free()


def tail_checked(x64, src, dst, n_base, h):
    """The checker's outputs for the prefixes x64[:n_base + e], e = 0 .. 3: one full run for the longest and, for each
    shorter one, a fresh run over the outputs whose support reaches past its end (the others read the same samples)."""
    g = ref.geometry(src, dst)
    full = ref.resample(x64[:n_base + 3], src, dst, h=h)
    kt = max(0, -((g["H"] - n_base * g["L"]) // g["M"]) - 1)        # below it no output reads a sample >= n_base
    out = []
    for e in range(4):
        n = n_base + e
        n_out = ref.out_len(n, src, dst)
        k0 = min(kt, n_out)
        out.append(np.concatenate([full[:k0], ref.resample(x64[:n], src, dst, k0, n_out, h=h)]))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_impulses(gpu, src, dst, kind):
    g = ref.geometry(src, dst)
    h = taps(src, dst)
    n_in = ref.design_len(g)
    n_out = ref.out_len(n_in, src, dst)
    seen = []
    for d in ref.impulse_designs(g, n_in, i16=kind == "i16"):
        pos, amp, x = d[:3]
        feed = d[3] if kind == "i16" else x
        y = gpu.resample(feed, src, dst)
        assert y.shape == (n_out,)
        k, idx, a, want = ref.impulse_expectation(g, n_out, pos, amp, h)
        outside = np.ones(n_out, bool)
        outside[k] = False
        bad = np.flatnonzero(outside & (y != 0.0))
        assert bad.size == 0, "%s: %g outside every support (%d such outputs)" % (ref.where(g, int(bad[0])), y[bad[0]], bad.size)
        err = np.abs(y[k].astype(np.float64) - want)
        tol = 2.0 ** -23 * np.abs(want) + 1e-12 * np.abs(a)
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, "%s tap %d: %r, want %r x %r (%d such outputs)" % (
            ref.where(g, int(k[bad[0]])), idx[bad[0]], y[k[bad[0]]], a[bad[0]], h[idx[bad[0]]], bad.size)
        seen.append((k, idx, a, bits(y)[k]))
        # the other entry points: the same bits
        dev, off = device_forms(gpu, feed, src, dst, n_out)
        for name, other in (("device", dev), ("device, source offset by a sample", off)):
            diff = np.flatnonzero(bits(other) != bits(y))
            assert diff.size == 0, "%s: %s form gives %r, host form %r" % (ref.where(g, int(diff[0])), name, other[diff[0]], y[diff[0]])
        if len(seen) <= 2:      # (a needle's samples cannot be read back: its energy, a fixed-order f64 sum of them, stands in)
            a_h = gpu.HipConvolve.resampled(feed, src, dst)
            b_h = gpu.HipConvolve(y)
            assert a_h.sample_len == n_out
            assert a_h.inverse_sample_auto_correlation() == b_h.inverse_sample_auto_correlation(), (src, dst, "needle form")
    # the same tap on the same amplitude: the same bits, in whichever block, lane, pass and input it falls
    k, idx, a, b = (np.concatenate(c) for c in zip(*seen))
    order = np.lexsort((b, a, idx))
    k, idx, a, b = k[order], idx[order], a[order], b[order]
    same = (idx[1:] == idx[:-1]) & (a[1:] == a[:-1])
    bad = np.flatnonzero(same & (b[1:] != b[:-1]))
    assert bad.size == 0, "tap %d x %r: %s gives bits %08x, %s gives %08x" % (
        idx[bad[0]], a[bad[0]], ref.where(g, int(k[bad[0]])), b[bad[0]], ref.where(g, int(k[bad[0] + 1])), b[bad[0] + 1])
    assert same.any()


@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_nonfinite_at_the_edges_f32(gpu, src, dst):
    g = ref.geometry(src, dst)
    h = taps(src, dst)
    L, M, H = g["L"], g["M"], g["H"]
    n_in = ref.design_len(g)
    n_out = ref.out_len(n_in, src, dst)
    rng = np.random.default_rng(src * 7 + dst)
    bg = rng.uniform(-1, 1, n_in).astype(np.float32)
    base = ref.resample(bg, src, dst, h=h)
    scale = float(np.abs(bg).max())
    interior = [g["bo"] * M // L // 2 + 1]
    specials = (np.nan, np.inf, -np.inf)
    c = 0
    for grp in ref.far_apart(g, ref.edge_samples(g, n_in), interior):
        x = bg.copy()
        for n in grp:
            x[n] = specials[c % 3]
            c += 1
        y = gpu.resample(x, src, dst)
        want = base.copy()                          # the checker, run afresh wherever a support holds a changed sample
        x64 = x.astype(np.float64)
        for n in grp:
            k0, k1 = max(0, -((H - n * L) // M) - 2), min(n_out, (n * L + H) // M + 3)
            if k1 > k0:
                want[k0:k1] = ref.resample(x64, src, dst, k0, k1, h=h)
        fy, fw = np.isfinite(y), np.isfinite(want)
        bad = np.flatnonzero(fy != fw)
        assert bad.size == 0, "%s: finite %s, the checker %s (%d such outputs; samples %s)" % (
            ref.where(g, int(bad[0])), fy[bad[0]], fw[bad[0]], bad.size, grp)
        assert (~fy).any()
        if fw.any():
            err = np.abs(y[fw].astype(np.float64) - want[fw])
            assert err.max() <= BOUND * scale, "%s: off by %g max |x|" % (ref.where(g, int(np.flatnonzero(fw)[err.argmax()])), err.max() / scale)


@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_full_scale_at_the_edges_i16(gpu, src, dst):
    """i16 holds no NaN: full-scale frames on silence at the same positions, and the outputs that are not zero."""
    g = ref.geometry(src, dst)
    h = taps(src, dst)
    n_in = ref.design_len(g)
    n_out = ref.out_len(n_in, src, dst)
    c = 0
    for grp in ref.far_apart(g, ref.edge_samples(g, n_in), [g["bo"] * g["M"] // g["L"] // 2 + 1]):
        pos = np.asarray(grp, np.int64)
        lr = np.zeros((n_in, 2), np.int16)
        lr[pos, 0] = lr[pos, 1] = [(32767, -32768)[(c + i) % 2] for i in range(pos.size)]
        c += pos.size
        x = ref.downmix(lr)
        y = gpu.resample(lr, src, dst)
        k, idx, a, want = ref.impulse_expectation(g, n_out, pos, x[pos], h)
        dense = np.zeros(n_out)
        dense[k] = want
        bad = np.flatnonzero((y != 0.0) != (dense != 0.0))
        assert bad.size == 0, "%s: %r, the checker %r (%d such outputs)" % (ref.where(g, int(bad[0])), y[bad[0]], dense[bad[0]], bad.size)
        assert np.abs(y - dense).max() <= BOUND * np.abs(x).max()


@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_random_against_checker(gpu, src, dst):
    g = ref.geometry(src, dst)
    h = taps(src, dst)
    n_base = ref.design_len(g)
    rng = np.random.default_rng(src * 11 + dst)
    x = rng.uniform(-1, 1, n_base + 3).astype(np.float32)
    lr = rng.integers(-32768, 32768, size=(n_base + 3, 2)).astype(np.int16)
    mono = ref.downmix(lr)
    for name, sig, feed in (("f32", x, x), ("i16", mono, lr)):
        wants = tail_checked(sig.astype(np.float64), src, dst, n_base, h)
        scale = float(np.abs(sig).max())
        for e, want in enumerate(wants):
            n = n_base + e
            y = gpu.resample(feed[:n], src, dst)
            assert y.shape == want.shape
            err = np.abs(y.astype(np.float64) - want)
            assert err.max() <= BOUND * scale, "%s %s n_in %d: off by %g max |x|" % (ref.where(g, int(err.argmax())), name, n, err.max() / scale)
            if name == "i16":
                diff = np.flatnonzero(bits(y) != bits(gpu.resample(mono[:n], src, dst)))
                assert diff.size == 0, "%s n_in %d: i16 and its down-mix differ (%d outputs)" % (ref.where(g, int(diff[0])), n, diff.size)


@pytest.mark.parametrize("src,dst", ref.LONG_PAIRS)
def test_long_filters(gpu, src, dst):
    """x = 1, the sign of one output's taps and a sine of 5 periods over the filter, 12 full-support outputs and both
    ends, against the per-output f64 dot product.  Worst |y - y_f64| / max |x| on an MI355X: 4.1e-8 to 5.6e-8 for the four
    long pairs, 7.1e-8 for the control.  One f32 chain per output, the kernel's form before these tests, gave 5.9e-5
    (8192 -> 1), 3.3e-5 (8191 -> 2), 8.0e-5 (768000 -> 100), 2.8e-5 (3000 -> 1) and 1.5e-6 (the control)."""
    g = ref.geometry(src, dst)
    h = taps(src, dst)
    n_in, inputs = ref.long_inputs(g)
    worst = {}
    for name, x in inputs.items():
        y = gpu.resample(x, src, dst)
        want = ref.resample_dot(x, src, dst, h=h)
        assert y.shape == want.shape
        worst[name] = float(np.abs(y.astype(np.float64) - want).max() / (BOUND * np.abs(x).max()))
    print("resample long filter %d->%d (%d taps): worst error / bound %s" % (
        src, dst, g["T"], ", ".join("%s %.4f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, "%d->%d (%d taps): worst error over 1e-5 max |x|: %s" % (src, dst, g["T"], worst)
