"""Host-side checks of needle estimation (no device): am_hit_window against the checker of tests/needle_estimate_ref.py
bit for bit, the checker against its own claims on the designed case, the header and the exports, the argument checks
of the two compute forms and what they answer without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import needle_estimate_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_window", "am_needle_estimate_rows", "am_needle_estimate_device")


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def haystacks():
    rng = np.random.default_rng(41)
    f = rng.uniform(-1.0, 1.0, 1000).astype(np.float32)
    f[500] = np.nan
    f[517] = np.inf
    f[530] = np.float32(1e-41)      # a denormal
    f[531] = np.float32(-0.0)
    s = rng.integers(-32768, 32768, 2000, dtype=np.int16)
    return {"f32": f, "s16": s}


@pytest.mark.parametrize("kind", ["f32", "s16"])
def test_hit_window_equals_the_checker(amlib, kind):
    x = haystacks()[kind]
    n = x.size if kind == "f32" else x.size // 2
    cases = [  # (start, scale, lead, length)
        (100, 1.0, 0, 64),
        (101, 0.37, 16, 300),             # odd start
        (5, 2.0, 32, 100),                # start < lead: the head is absent
        (0, -1.5, 7, 20),
        (n - 50, 0.5, 10, 200),           # start - lead + length > len: the tail is absent
        (n - 1, 3.0, 0, 1),               # length = 1, the last element
        (n, 1.0, 0, 1),                   # ... and the first one behind the haystack
        (490, 0.25, 8, 80),               # f32: a NaN, an inf, a denormal and -0 inside
        (517, 1e30, 0, 1),
        (n + 1000, 1.0, 3, 9),            # wholly outside
        (3, 1.0, 2 * n, 40),              # lead beyond everything
    ]
    for start, scale, lead, length in cases:
        got = amlib.hit_window(x, start, scale, lead, length)
        want = ref.hit_window(x, start, scale, lead, length)
        assert got.dtype == np.float32 and same_bits(got, want), (kind, start, scale, lead, length)
    head = amlib.hit_window(x, 5, 2.0, 32, 100)
    assert np.isnan(head[:27]).all() and np.isfinite(head[27:]).all()
    tail = amlib.hit_window(x, n - 50, 0.5, 10, 200)
    assert np.isfinite(tail[:60]).all() and np.isnan(tail[60:]).all()
    if kind == "f32":
        w = amlib.hit_window(x, 490, 0.25, 8, 80)   # element n reads x[482 + n]
        assert np.isnan(w[18]) and np.isnan(w[35]) and np.isfinite(np.delete(w, [18, 35])).all()
        assert w[48] == np.float32(1e-41) * np.float32(0.25) and w[48] != 0.0
        assert w[49] == 0.0 and np.signbit(w[49])


def test_hit_window_arguments(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    x = np.zeros(16, np.float32)
    row = np.full(8, 5.0, np.float32)
    assert L.am_hit_window(x.ctypes.data, 16, 7, 0, 1.0, 0, 8, row.ctypes.data) == bad and b"bad sample format 7" in L.am_last_error_string()
    assert L.am_hit_window(x.ctypes.data, 16, 0, 0, 1.0, 0, 8, None) == bad and L.am_last_error_string() == b"null pointer"
    assert L.am_hit_window(None, 16, 0, 0, 1.0, 0, 8, row.ctypes.data) == bad
    assert L.am_hit_window(x.ctypes.data, 16, 0, 0, 1.0, 0, 0, row.ctypes.data) == bad and b"length must be at least 1" in L.am_last_error_string()
    for s in (0.0, float("nan"), float("inf"), float("-inf")):
        assert L.am_hit_window(x.ctypes.data, 16, 0, 0, s, 0, 8, row.ctypes.data) == bad
        assert b"scale must be finite and not zero" in L.am_last_error_string()
    assert (row == 5.0).all()
    assert L.am_hit_window(None, 0, 0, 0, 1.0, 0, 8, row.ctypes.data) == 0 and np.isnan(row).all()   # an empty haystack: all absent


def test_checker_holds_its_claims_on_the_designed_case():
    c, occ, scales, dirty = ref.designed_case()
    assert dirty.sum(axis=0).max() == 3 and set(np.unique(np.log2(1.0 / scales))) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    rows = np.stack([ref.hit_window(occ[i], 0, scales[i], 0, ref.CLEAN_LEN) for i in range(9)])
    assert np.array_equal(rows[~dirty].view(np.uint32), np.broadcast_to(c, rows.shape)[~dirty].view(np.uint32))
    med, dev_med, cnt = ref.estimate(rows, ref.MEDIAN)
    trm, _, _ = ref.estimate(rows, ref.TRIMMED, 334)
    mean, _, _ = ref.estimate(rows, ref.MEAN)
    assert (cnt == 9).all()
    assert np.array_equal(med.view(np.uint32), c.view(np.uint32))
    assert np.array_equal(trm.view(np.uint32), c.view(np.uint32))
    bound = 0.01 * np.abs(c).max()
    for t in range(3):
        assert np.abs(mean - c)[t * ref.THIRD:min((t + 1) * ref.THIRD, ref.CLEAN_LEN)].max() > bound
    assert (dev_med > 0).all()      # some row is contaminated at every sample of the needle


def test_checker_orders_and_trims():
    v = np.array([[0.0], [-0.0], [np.nan], [1.0], [-1.0], [np.float32(1e-45)]], dtype=np.float32)
    k = ref.keys(v[:, 0])
    order = np.argsort(np.where(np.isfinite(v[:, 0]), k, ref.ABSENT_KEY), kind="stable")
    assert order.tolist() == [4, 1, 0, 5, 3, 2]                     # -1 < -0 < +0 < denormal < 1, absent last
    assert np.array_equal(ref.unkeys(k).view(np.uint32), v[:, 0].view(np.uint32))
    est, dev, cnt = ref.estimate(v, ref.MEDIAN)
    assert cnt[0] == 5 and est[0] == 0.0 and not np.signbit(est[0])  # the middle of five: +0
    est, _, _ = ref.estimate(v[[1, 0, 2]], ref.MEDIAN)               # even count: (-0 + +0) / 2 = +0
    assert est[0] == 0.0 and not np.signbit(est[0])
    est, _, _ = ref.estimate(v[[1, 2]], ref.MEDIAN)                  # one value: itself, sign and all
    assert est[0] == 0.0 and np.signbit(est[0])
    r = np.arange(10, dtype=np.float32).reshape(10, 1)
    assert ref.estimate(r, ref.TRIMMED, 0)[0][0] == 4.5 and ref.estimate(r, ref.TRIMMED, 100)[0][0] == 4.5
    assert ref.estimate(r[:9], ref.TRIMMED, 500)[0][0] == 4.0       # d capped at (c - 1) / 2: the median of an odd count
    assert ref.estimate(r, ref.TRIMMED, 500)[0][0] == 4.5           # ... and the two middle values of an even one
    r2 = r.copy(); r2[9] = 1000.0
    assert ref.estimate(r2, ref.TRIMMED, 100)[0][0] == 4.5 and ref.estimate(r2, ref.MEAN)[0][0] > 100
    est, dev, cnt = ref.estimate(np.full((3, 2), np.nan, np.float32), ref.MEAN)
    assert est.tolist() == [0.0, 0.0] and dev.tolist() == [0.0, 0.0] and cnt.tolist() == [0, 0]


def test_header_declares_estimation_and_library_exports_it(amlib):
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h and "#define AM_EST_MAX_HITS 64" in h
    assert re.search(r"enum \{ AM_EST_MEAN = 0, AM_EST_MEDIAN = 1, AM_EST_TRIMMED = 2 \};", h)
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(FUNCS) <= exported and set(FUNCS) <= set(amlib.declared_symbols())
    assert (amlib.EST_MAX_HITS, int(amlib.Est.MEAN), int(amlib.Est.MEDIAN), int(amlib.Est.TRIMMED)) == (ref.MAX_HITS, ref.MEAN, ref.MEDIAN, ref.TRIMMED)
    assert C.sizeof(amlib.AmEstimateParams) == 24 and C.sizeof(amlib.AmEstHit) == 16
    for name in FUNCS:   # the other bindings mirror them
        assert name in open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
        assert "pub fn " + name + "(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def no_device(amlib, rc):
    """what a valid call gives on a machine without a device (with one, it simply succeeds)"""
    return rc in (amlib.AM_ERR_NO_DEVICE, amlib.AM_ERR_HIP) or (rc == 0 and amlib.device_count() > 0)


def params(amlib, method, trim, lead, length):
    return amlib.AmEstimateParams(method, trim, lead, length)


def test_estimate_rows_arguments_before_any_device(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    rows = np.zeros((4, 8), np.float32)
    est, dev, cnt = np.full(8, 5.0, np.float32), np.full(8, 5.0, np.float32), np.full(8, 5, np.uint32)

    def call(n, ep, rows_p=rows.ctypes.data, est_p=est.ctypes.data, device=999):
        return L.am_needle_estimate_rows(device, rows_p, n, C.byref(ep) if ep is not None else None, est_p, dev.ctypes.data, cnt.ctypes.data)

    ok = params(amlib, 1, 0, 0, 8)
    assert call(4, ok, rows_p=None) == bad and L.am_last_error_string() == b"null pointer"
    assert call(4, None) == bad and call(4, ok, est_p=None) == bad
    assert call(4, params(amlib, 3, 0, 0, 8)) == bad and b"unknown method 3" in L.am_last_error_string()
    assert call(4, params(amlib, 2, 501, 0, 8)) == bad and b"trim_permille must be in 0..500 (got 501)" in L.am_last_error_string()
    assert call(4, params(amlib, 0, 501, 0, 8)) == bad
    assert call(0, ok) == bad and b"n must be at least 1" in L.am_last_error_string()
    assert call(4, params(amlib, 1, 0, 0, 0)) == bad and b"length must be at least 1" in L.am_last_error_string()
    for method in (1, 2):
        assert call(65, params(amlib, method, 0, 0, 8)) == bad
        assert b"at most 64 hits" in L.am_last_error_string() and b"got 65" in L.am_last_error_string()
    assert call(65536, params(amlib, 0, 0, 0, 8)) == bad and b"mean takes at most 65535 hits" in L.am_last_error_string()
    assert (est == 5.0).all() and (dev == 5.0).all() and (cnt == 5).all()
    # valid calls reach the device: without one they fail loudly (a bad ordinal is refused in any case)
    assert call(4, ok) != 0
    assert no_device(amlib, call(4, ok, device=0))
    assert no_device(amlib, call(4, params(amlib, 2, 500, 12345, 8), device=0))   # (lead is ignored)


def test_estimate_device_arguments_before_any_device(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    est, dev, cnt = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint32)
    ptrs = (C.c_void_p * 2)(0x1000, 0x2000)     # never dereferenced: every call below is refused before a device is asked
    lens = (C.c_size_t * 2)(100, 100)
    ok = params(amlib, 1, 0, 4, 8)

    def call(hits, ep=ok, fmt=0, pp=ptrs, ll=lens, n_hay=2, n=None, est_p=est.ctypes.data):
        hh = (amlib.AmEstHit * max(len(hits), 1))(*[amlib.AmEstHit(*h) for h in hits]) if hits is not None else None
        return L.am_needle_estimate_device(999, pp, ll, n_hay, fmt, hh, len(hits) if n is None else n, C.byref(ep), est_p,
                                           dev.ctypes.data, cnt.ctypes.data)

    good = [(10, 0, 1.0), (20, 1, 0.5)]
    assert call(good, pp=None) == bad and L.am_last_error_string() == b"null pointer"
    assert call(good, ll=None) == bad and call(None, n=2) == bad and call(good, est_p=None) == bad
    assert call(good, fmt=5) == bad and b"bad sample format 5" in L.am_last_error_string()
    assert call(good, ep=params(amlib, 9, 0, 0, 8)) == bad and b"unknown method 9" in L.am_last_error_string()
    assert call(good, ep=params(amlib, 2, 600, 0, 8)) == bad and b"trim_permille" in L.am_last_error_string()
    assert call([], ep=ok) == bad and b"n must be at least 1" in L.am_last_error_string()
    assert call(good, ep=params(amlib, 1, 0, 0, 0)) == bad
    assert call([(0, 0, 1.0)] * 65) == bad and b"at most 64 hits" in L.am_last_error_string()
    assert call(good + [(5, 2, 1.0)]) == bad and L.am_last_error_string() == b"hit 2: haystack 2 out of range (n_hay = 2)"
    for s in (0.0, float("nan"), float("inf")):
        assert call(good + [(5, 1, s)]) == bad and L.am_last_error_string() == b"hit 2: scale must be finite and not zero"
    null1 = (C.c_void_p * 2)(0x1000, None)
    assert call(good, pp=null1) == bad and L.am_last_error_string() == b"hit 1: null haystack"
    assert call([(10, 0, 1.0)], pp=null1) != 0       # (haystack 1 is not read) a valid call: refused for its device only
    assert call(good) in (amlib.AM_ERR_NO_DEVICE, amlib.AM_ERR_HIP, bad)   # device 999
    with pytest.raises(amlib.AudioMatchError):
        amlib.estimate_needle(np.zeros((65, 4), np.float32), amlib.Est.MEDIAN)
    with pytest.raises(ValueError):
        amlib.estimate_needle(np.zeros(4, np.float32))


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("learn=%s method=%u trim=%u margin_ms=%lld\n", a.learn_needle.c_str(), a.learn_method, a.learn_trim,
                    a.learn_margin_ms ? (long long)*a.learn_margin_ms : -1ll);
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_learn_needle(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    base = ("a.wav", "b.wav", "--snippet", "s.wav")
    assert run(*base) == (0, "learn= method=1 trim=0 margin_ms=-1\n")
    assert run(*base, "--learn-needle", "out.wav") == (0, "learn=out.wav method=1 trim=0 margin_ms=-1\n")
    assert run(*base, "--learn-needle", "out.wav:median", "--learn-margin", "0") == (0, "learn=out.wav method=1 trim=0 margin_ms=0\n")
    assert run(*base, "--learn-needle", "out.wav:mean", "--learn-margin", "1500ms") == (0, "learn=out.wav method=0 trim=0 margin_ms=1500\n")
    assert run(*base, "--learn-needle", "d/out.wav:trimmed=334") == (0, "learn=d/out.wav method=2 trim=334 margin_ms=-1\n")
    assert run(*base, "--learn-needle", "out.wav:trimmed=0")[0] == 0 and run(*base, "--learn-needle", "out.wav:trimmed=500")[0] == 0
    for v in ("out.wav:trimmed=501", "out.wav:trimmed=", "out.wav:trimmed=-1", "out.wav:mode", ":median", "out.wav:"):
        code, out = run(*base, "--learn-needle", v)
        assert code == 2 and "for --learn-needle (OUT.wav[:mean|median|trimmed=P], P in 0..500 permille)" in out, (v, out)
    code, out = run(*base, "--learn-needle")
    assert code == 2 and "missing value for --learn-needle" in out
    code, out = run(*base, "--learn-margin", "2s")
    assert code == 2 and "--learn-margin needs --learn-needle" in out
    code, out = run(*base, "--learn-needle", "o.wav", "--learn-margin", "soon")
    assert code == 2 and "invalid duration 'soon' for --learn-margin" in out
    code, out = run(*base, "--learn-needle", "o.wav", "--best", "3")
    assert code == 2 and "--learn-needle and --best are mutually exclusive" in out
    code, out = run(*base, "--snippet", "t.wav", "--learn-needle", "o.wav")
    assert code == 2 and "--learn-needle takes one --snippet only" in out
    for extra in (("--whiten", "8"), ("--preemphasis", "0.9")):
        code, out = run(*base, "--learn-needle", "o.wav", *extra)
        assert code == 2 and "--learn-needle does not apply with --whiten or --preemphasis" in out
    code, out = run("--live", "--rate", "8000", "--snippet", "s.wav", "--learn-needle", "o.wav")
    assert code == 2 and "--live: --learn-needle does not apply" in out
    code, out = run("--help")
    assert code == 0 and re.search(r"^  --learn-needle OUT\.wav\[:mean\|median\|trimmed=P\]$", out, re.M) and re.search(r"^  --learn-margin D {2,}\S", out, re.M)
    assert all(len(ln) <= 120 for ln in out.splitlines())
