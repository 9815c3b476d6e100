"""Host-side checks of per-hit channel estimation (no device): the header, the exports and the record sizes;
am_channel_solve against the explicit solve of tests/hit_channel_ref.py, on exact recovery and at its fallback; its
refusals; am_hit_residual against a numpy restatement bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hit_channel_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_channel", "am_hit_channel_device", "am_hit_channel_batch_device", "am_channel_solve", "am_hit_residual")
G = {0: 1.0, 3: 0.5, -2: -0.25}   # the channel of the recovery tests


def white(seed, s):
    return np.random.default_rng(seed).normal(0, 0.3, s).astype(np.float32)


def ar1(seed, s, a=0.9):
    e = np.random.default_rng(seed).normal(0, 0.1, s)
    y = np.empty(s)
    acc = 0.0
    for i in range(s):
        acc = a * acc + e[i]
        y[i] = acc
    return y.astype(np.float32)


def autocorr(n, p):
    n = n.astype(np.float64)
    return np.array([np.dot(n[k:], n[:len(n) - k]) for k in range(2 * p + 1)])


def through_g(needle, p):
    """(c, r) in f64 of the span that holds the needle through G and nothing else: c[l] = sum_m g[m] r[|l - m|]."""
    r_long = autocorr(needle, p + 3)
    c = np.array([sum(g * r_long[abs(l - m)] for m, g in G.items()) for l in range(-p, p + 1)])
    return c, r_long[:2 * p + 1]


def test_header_declares_channel_and_library_exports_it(amlib):
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h
    assert re.search(r"#define AM_CHAN_MAX_RADIUS\s+128\b", h) and amlib.AM_CHAN_MAX_RADIUS == 128 == ref.MAX_RADIUS
    assert "AM_HIT_ILL_CONDITIONED = 512" in h and amlib.AM_HIT_ILL_CONDITIONED == 512 == ref.ILL
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(FUNCS) <= exported and set(FUNCS) <= set(amlib.declared_symbols())
    assert amlib.lib().am_abi_version() == 3
    assert C.sizeof(amlib.HitChannel) == 32 and C.sizeof(amlib.AmChannelParams) == 16
    for name in FUNCS:
        assert name in open(os.path.join(ROOT, "include", "audiomatch.hpp")).read(), name
        assert "pub fn " + name + "(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read(), name


def test_struct_sizes_in_c(tmp_path):
    """sizeof(am_channel_hit) == 32 and sizeof(am_channel_params) == 16, as a C compiler sees the header."""
    src = tmp_path / "sizes.c"
    src.write_text('#include "audiomatch.h"\n_Static_assert(sizeof(am_channel_hit) == 32, "record");\n'
                   '_Static_assert(sizeof(am_channel_params) == 16, "params");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "sizes.o")])


@pytest.mark.parametrize("kind", ["white", "ar1"])
@pytest.mark.parametrize("p", [0, 1, 16, 128])
def test_solve_against_the_checker(amlib, kind, p):
    s = 4096
    needle = white(11, s) if kind == "white" else ar1(12, s)
    r = autocorr(needle, p)
    c = np.random.default_rng(13 + p).normal(0, 1.0, 2 * p + 1) * r[0]
    for noise_db in (60.0, 200.0):
        want, cond = ref.solve_ref(r, c, noise_db)
        got, ill = amlib.channel_solve(r, c, noise_db)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(kind, p, noise_db, "cond", cond, "err", err)
        assert cond <= 1e4, (kind, p, cond)
        assert not ill and err <= 1e-9, (kind, p, noise_db, err)
    if p == 0:
        assert got[0] == c[0] / (r[0] * (1.0 + 1e-20))


@pytest.mark.parametrize("kind", ["white", "ar1"])
def test_exact_recovery(amlib, kind):
    p = 8
    needle = white(21, 4096) if kind == "white" else ar1(22, 4096)
    c, r = through_g(needle, p)
    want = np.zeros(2 * p + 1)
    for l, g in G.items():
        want[l + p] = g
    h, ill = amlib.channel_solve(r, c, 200.0)
    print(kind, "noise 200:", np.abs(h - want).max())
    assert not ill and np.abs(h - want).max() <= 1e-6
    # noise_db = 60: (T + lambda r0 I) h = T g, so h - g = -lambda r0 (T + lambda r0 I)^-1 g and |h - g| <= lambda (r0 /
    # lambda_min(T)) |g|.  A white needle has r0 / lambda_min close to 1: the bias is at most lambda |g| = 1.15e-6, inside
    # 2e-6.  The AR(1) needle is held to the bound of its own matrix.
    h, ill = amlib.channel_solve(r, c, 60.0)
    spread = r[0] / np.linalg.eigvalsh(ref.toeplitz(r)).min()
    bound = 1e-6 * spread * np.linalg.norm(list(G.values()))
    print(kind, "noise 60:", np.abs(h - want).max(), "r0 / lambda_min", spread, "bound", bound)
    assert not ill and np.abs(h - want).max() <= (2e-6 if kind == "white" else bound)
    assert kind != "white" or bound <= 2e-6


def test_fallback_is_the_plain_gain_or_a_solution(amlib):
    p = 8
    n = np.full(64, 0.25, dtype=np.float32)
    r = autocorr(n, p)
    c = 0.5 * r[np.abs(np.arange(-p, p + 1))]
    h, ill = amlib.channel_solve(r, c, 200.0)
    if ill:
        want = np.zeros(2 * p + 1)
        want[p] = c[p] / r[0]
        assert (h == want).all()
    else:
        assert np.isfinite(h).all() and np.abs(ref.toeplitz(r, 1e-20) @ h - c).max() <= 1e-6 * np.abs(c).max()
    h2, ill2 = amlib.channel_solve(r, c, 200.0)
    assert ill2 == ill and h2.tobytes() == h.tobytes()
    # a matrix that is not positive definite: the recursion stops, the taps are the plain gain
    bad = np.array([1.0, 2.0, 0.0])
    h, ill = amlib.channel_solve(bad, np.array([1.0, 3.0, 1.0]), 200.0)
    assert ill and (h == np.array([0.0, 3.0, 0.0])).all()
    h, ill = amlib.channel_solve(np.zeros(3), np.array([1.0, 3.0, 1.0]), 60.0)
    assert ill and (h == 0.0).all()


def test_solve_refusals(amlib):
    L = amlib.lib()
    INV = amlib.AM_ERR_INVALID_ARG
    r = np.array([2.0, 0.5, 0.1])
    c = np.array([0.3, 1.0, 0.2])
    h = np.zeros(3)
    ill = C.c_int(0)

    def call(rp, cp, radius, noise, hp, ip):
        rc = L.am_channel_solve(rp, cp, radius, noise, hp, ip)
        msg = L.am_last_error_string()
        return rc, (msg.decode() if msg else "")

    ok = (r.ctypes.data, c.ctypes.data, 1, 60.0, h.ctypes.data, C.byref(ill))
    assert call(*ok)[0] == amlib.AM_OK
    for k in (0, 1, 4):
        args = list(ok)
        args[k] = None
        rc, msg = call(*args)
        assert rc == INV and "null" in msg, msg
    rc, msg = call(r.ctypes.data, c.ctypes.data, 1, 60.0, h.ctypes.data, None)
    assert rc == INV and "null" in msg
    big = np.zeros(2 * 129 + 1)
    rc, msg = call(big.ctypes.data, big.ctypes.data, 129, 60.0, big.ctypes.data, C.byref(ill))
    assert rc == INV and "AM_CHAN_MAX_RADIUS" in msg, msg
    for noise in (-1.0, 201.0, float("nan")):
        rc, msg = call(r.ctypes.data, c.ctypes.data, 1, noise, h.ctypes.data, C.byref(ill))
        assert rc == INV and "noise_db" in msg, msg
    for v in (np.nan, np.inf):
        rb = r.copy()
        rb[2] = v
        rc, msg = call(rb.ctypes.data, c.ctypes.data, 1, 60.0, h.ctypes.data, C.byref(ill))
        assert rc == INV and "r[2]" in msg, msg
    with pytest.raises(ValueError):
        amlib.channel_solve(r, c[:2])


def downmix(lr):
    return ((lr[:, 0].astype(np.int32) + lr[:, 1]).astype(np.float32) * (np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0)))).astype(np.float32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_hit_residual_bit_for_bit(amlib):
    rng = np.random.default_rng(31)
    s, p, n = 300, 5, 1000
    needle = white(32, s)
    taps = rng.normal(0, 0.3, 2 * p + 1).astype(np.float32)
    hay = rng.normal(0, 0.2, n).astype(np.float32)
    hay[417] = np.nan
    lr = rng.integers(-3000, 3000, size=(n, 2)).astype(np.int16)
    for start in (400, 2, 0, n - s, n - s - 2):      # inside (a NaN in the span), absent head, absent tail
        model, resid = amlib.hit_residual(hay, start, needle, taps)
        wm, wr = ref.residual_ref(hay, start, needle, taps)
        assert same_bits(model, wm) and same_bits(resid, wr), start
        absent = np.array([not (0 <= start - p + u < n) for u in range(s + 2 * p)])
        assert np.isnan(resid[absent]).all() and absent.sum() == max(p - start, 0) + max(start + s + p - n, 0)
        if start == 400:
            assert np.isnan(resid[417 - (start - p)]) and np.isnan(resid).sum() == 1
        model, resid = amlib.hit_residual(lr, start, needle, taps)
        wm, wr = ref.residual_ref(downmix(lr), start, needle, taps)
        assert same_bits(model, wm) and same_bits(resid, wr), start
    # taps = the delta: the model is the needle, embedded; the residual is x - n there and x elsewhere
    delta = np.zeros(2 * p + 1, dtype=np.float32)
    delta[p] = 1.0
    clean = rng.normal(0, 0.2, n).astype(np.float32)
    start = 350
    model, resid = amlib.hit_residual(clean, start, needle, delta)
    want = np.zeros(s + 2 * p, dtype=np.float32)
    want[p:p + s] = needle
    assert same_bits(model, want)
    span = clean[start - p:start + s + p].copy()
    span[p:p + s] -= needle
    assert same_bits(resid, span)
    # P = 0 and either output alone
    m0, r0 = amlib.hit_residual(clean, start, needle, np.array([0.5], dtype=np.float32))
    assert same_bits(m0, (needle.astype(np.float64) * 0.5).astype(np.float32)) and same_bits(r0, clean[start:start + s] - m0)
    L = amlib.lib()
    only = np.empty(s + 2 * p, dtype=np.float32)
    assert L.am_hit_residual(clean.ctypes.data, n, 0, start, needle.ctypes.data, s, delta.ctypes.data, p, None, only.ctypes.data) == amlib.AM_OK
    assert same_bits(only, span)
    assert L.am_hit_residual(clean.ctypes.data, n, 0, start, needle.ctypes.data, s, delta.ctypes.data, p, only.ctypes.data, None) == amlib.AM_OK
    assert same_bits(only, want)


def test_hit_residual_refusals(amlib):
    L = amlib.lib()
    INV = amlib.AM_ERR_INVALID_ARG
    x = np.zeros(100, dtype=np.float32)
    nd = np.ones(10, dtype=np.float32)
    tp = np.ones(3, dtype=np.float32)
    out = np.zeros(12, dtype=np.float32)
    ok = [x.ctypes.data, 100, 0, 5, nd.ctypes.data, 10, tp.ctypes.data, 1, out.ctypes.data, out.ctypes.data]
    assert L.am_hit_residual(*ok) == amlib.AM_OK
    for k, v, text in ((0, None, "null"), (4, None, "null"), (6, None, "null"), (2, 2, "format"), (5, 0, "at least 1"),
                       (7, 129, "AM_CHAN_MAX_RADIUS"), (3, 1 << 62, "2^62")):
        args = list(ok)
        args[k] = v
        assert L.am_hit_residual(*args) == INV
        assert text in L.am_last_error_string().decode(), (k, L.am_last_error_string())
