"""Host-side checks of sample-rate conversion (no device): am_resample_len, the rate checks, the tests' f64 checker
against scipy.signal.resample_poly, and the CLI's --resample flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000, 384000)


def test_header_declares_resampling():
    h = open(HEADER).read()
    for fn in ("am_resample_len", "am_resample", "am_resample_device", "am_needle_create_resampled"):
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h


def _len(amlib, n, src, dst):
    out = C.c_size_t(12345)
    rc = amlib.lib().am_resample_len(n, src, dst, C.byref(out))
    return rc, out.value


def test_resample_len(amlib):
    assert _len(amlib, 44100, 44100, 48000) == (0, 48000)          # exact
    assert _len(amlib, 48000, 48000, 44100) == (0, 44100)
    assert _len(amlib, 1, 44100, 48000) == (0, 2)                  # ceil(160 / 147)
    assert _len(amlib, 1, 48000, 44100) == (0, 1)
    assert _len(amlib, 147, 48000, 44100) == (0, 136)              # ceil(147 * 147 / 160) = ceil(135.06)
    assert _len(amlib, 3, 2, 1) == (0, 2)                          # ceil(3 / 2)
    assert _len(amlib, 0, 44100, 48000) == (0, 0)
    assert _len(amlib, 0, 48000, 48000) == (0, 0)
    assert _len(amlib, 12345, 48000, 48000) == (0, 12345)          # equal rates
    hour = 3600 * 48000
    assert _len(amlib, hour, 48000, 44100) == (0, 3600 * 44100)
    for n in (1, 2, 17, 441, 1000003):
        for s, d in ((44100, 48000), (11025, 384000), (384000, 8000), (8000, 11025)):
            assert _len(amlib, n, s, d) == (0, ref.out_len(n, s, d)), (n, s, d)
    assert amlib.resample_len(10, 44100, 22050) == 5


def test_resample_len_errors(amlib):
    L = amlib.lib()
    assert _len(amlib, 10, 0, 48000)[0] == amlib.AM_ERR_INVALID_ARG
    assert b"rates must be in 1..768000" in L.am_last_error_string()
    assert _len(amlib, 10, 48000, 0)[0] == amlib.AM_ERR_INVALID_ARG
    assert _len(amlib, 10, 768001, 48000)[0] == amlib.AM_ERR_INVALID_ARG
    assert _len(amlib, 10, 48000, 768001)[0] == amlib.AM_ERR_INVALID_ARG
    assert _len(amlib, 10, 768000, 1)[0] == amlib.AM_ERR_INVALID_ARG     # R = 768000
    assert b"R = max(L, M) = 768000 > 8192" in L.am_last_error_string()
    assert _len(amlib, 10, 8193, 1)[0] == amlib.AM_ERR_INVALID_ARG       # R = 8193
    assert _len(amlib, 10, 8192, 1) == (0, 1)                          # R = 8192: the limit itself
    assert _len(amlib, 10, 768000, 768000) == (0, 10)
    assert L.am_resample_len(10, 44100, 48000, None) == amlib.AM_ERR_INVALID_ARG
    with pytest.raises(amlib.AudioMatchError):
        amlib.resample_len(10, 0, 1)


def test_every_common_pair_is_accepted(amlib):
    worst = 0
    for s in RATES:
        for d in RATES:
            rc, n = _len(amlib, 1000, s, d)
            assert rc == 0 and n == ref.out_len(1000, s, d), (s, d)
            L, M, _ = ref.ratio(s, d)
            worst = max(worst, L, M)
    assert worst == 5120                                               # 11025 <-> 384000


def test_argument_errors_before_any_device(amlib):
    """Rate, format, capacity and null-pointer checks run before a device is touched."""
    L = amlib.lib()
    x = np.zeros(16, np.float32)
    out = np.zeros(32, np.float32)
    n = C.c_size_t(0)
    assert L.am_resample(0, x.ctypes.data, 16, 0, 0, 48000, out.ctypes.data, 32, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_resample(0, x.ctypes.data, 16, 7, 44100, 48000, out.ctypes.data, 32, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    assert b"bad sample format" in L.am_last_error_string()
    assert L.am_resample(0, x.ctypes.data, 16, 0, 44100, 48000, out.ctypes.data, 17, C.byref(n)) == amlib.AM_ERR_CAPACITY
    assert n.value == 18 and b"18 samples needed" in L.am_last_error_string()
    assert L.am_resample_device(0, x.ctypes.data, 16, 0, 44100, 48000, out.ctypes.data, 0, C.byref(n)) == amlib.AM_ERR_CAPACITY
    assert n.value == 18
    assert L.am_resample(0, x.ctypes.data, 16, 0, 44100, 48000, out.ctypes.data, 32, None) == amlib.AM_ERR_INVALID_ARG
    assert L.am_resample(0, None, 16, 0, 44100, 48000, out.ctypes.data, 32, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_resample(0, None, 0, 0, 44100, 48000, None, 0, C.byref(n)) == 0 and n.value == 0   # n_in = 0
    h = C.c_void_p()
    assert L.am_needle_create_resampled(0, x.ctypes.data, 0, 0, 44100, 48000, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_needle_create_resampled(0, x.ctypes.data, 16, 0, 44100, 9000000, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
    assert {"am_resample_len", "am_resample", "am_resample_device", "am_needle_create_resampled"} <= set(amlib.declared_symbols())


@pytest.mark.parametrize("src,dst", [(44100, 48000), (48000, 44100), (44100, 22050), (22050, 44100), (8000, 11025),
                                     (11025, 32000), (96000, 44100), (384000, 8000), (11025, 384000)])
def test_checker_matches_scipy(src, dst):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(src + dst)
    L, M, _ = ref.ratio(src, dst)
    for n in (1, 7, 2001):
        x = rng.standard_normal(n)
        want = signal.resample_poly(x, L, M)
        got = ref.resample(x, src, dst)
        assert got.shape == want.shape == (ref.out_len(n, src, dst),)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(x).max()), (src, dst, n)


def test_checker_spans_and_nonfinite():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(5000)
    full = ref.resample(x, 48000, 44100)
    assert np.array_equal(ref.resample(x, 48000, 44100, 100, 300), full[100:300])
    x[2500] = np.nan
    y = ref.resample(x, 48000, 44100)
    L, M, H = ref.ratio(48000, 44100)
    k = np.arange(y.size)
    hit = np.abs(k * M - 2500 * L) <= H
    assert hit.any() and np.isnan(y[hit]).all() and np.isfinite(y[~hit]).all()
    # a window of the signal gives the same outputs as the whole signal
    assert np.array_equal(ref.resample(x[2000:3500], 48000, 44100, 2000, 2600, n0=2000, n_in=5000), y[2000:2600], equal_nan=True)


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("resample=%d files=%zu\n", a.resample ? 1 : 0, a.within.size());
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_resample(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "resample=0 files=1\n")
    assert run("a.wav", "--snippet", "s.wav", "--resample") == (0, "resample=1 files=1\n")
    assert run("--resample", "a.wav", "b.wav", "--snippet", "s.wav") == (0, "resample=1 files=2\n")
    code, out = run("a.wav", "--snippet", "s.wav", "--resample=1")
    assert code == 2 and "unknown option --resample=1" in out
    code, out = run("--help")
    assert code == 0 and re.search(r"^  --resample {2,}\S", out, re.M), out
