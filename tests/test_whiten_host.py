"""Host-side checks of spectral whitening (no device): the header and the exports, am_whiten_taps against the f64
checker of tests/whiten_ref.py, the checker against scipy.linalg.solve_toeplitz, the argument checks of the device
entry points and the CLI's --whiten / --preemphasis flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import whiten_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
KERNELS_H = os.path.join(ROOT, "audio-matcher_amd", "csrc", "am_kernels.h")
FUNCS = ("am_lag_products", "am_lag_products_device", "am_whiten_taps", "am_fir", "am_fir_device", "am_needle_create_filtered")
ORDERS = (1, 8, 32, 64)
DP = C.POINTER(C.c_double)
FP = C.POINTER(C.c_float)


def signals():
    """The four signals of the design tests, 20 000 samples each, rounded to f32 as the library sees them."""
    rng = np.random.default_rng(2024)
    n = 20000
    t = np.arange(n)
    out = {
        "white": rng.standard_normal(n),
        "ar1_0.98": ref.ar1(rng, n, 0.98),
        "ar2_resonant": ref.ar2(rng, n, 1.8, -0.9),
        "sine_in_-60dB_noise": np.sin(2 * np.pi * 0.0371 * t) + 1e-3 * rng.standard_normal(n),
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


def test_header_declares_whitening_and_library_exports_it(amlib):
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h
    assert "#define AM_WHITEN_MAX_ORDER 64" in h and re.search(r"#define AM_FIR_MAX_TAPS\s+\(AM_WHITEN_MAX_ORDER \+ 1\)", h)
    assert "audio_matcher.rs:297-343" in h
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(FUNCS) <= exported
    assert set(FUNCS) <= set(amlib.declared_symbols())
    assert amlib.lib().am_abi_version() == 3
    assert (amlib.WHITEN_MAX_ORDER, amlib.FIR_MAX_TAPS) == (ref.MAX_ORDER, ref.MAX_TAPS) == (64, 65)


def test_python_constants_are_the_kernels():
    k = open(KERNELS_H).read()
    import audiomatch_amd as am
    assert re.search(r"constexpr int kLagBlock = (\d+);", k).group(1) == str(am.LAG_BLOCK)
    threads, per, passes = (int(re.search(r"constexpr int %s = (\d+);" % name, k).group(1)) for name in ("kFirThreads", "kFirPer", "kFirPasses"))
    assert re.search(r"constexpr int kFirTile = kFirThreads \* kFirPer \* kFirPasses;", k)
    assert threads * per * passes == am.FIR_TILE


@pytest.mark.parametrize("name", ["white", "ar1_0.98", "ar2_resonant", "sine_in_-60dB_noise"])
def test_whiten_taps_against_checker_and_scipy(amlib, name):
    linalg = pytest.importorskip("scipy.linalg")
    x = signals()[name]
    r_all, _ = ref.lag_products(x, 64)
    for order in ORDERS:
        r = r_all[:order + 1]
        want = ref.whiten_taps(r, 60.0)
        # the checker is the solution of the normal equations: T a[1:] = -r[1:], T = toeplitz(corrected r[0 .. order - 1])
        c = r[:order].copy()
        c[0] *= 1.0 + 1e-6
        sol = linalg.solve_toeplitz(c, -r[1:order + 1])
        err = np.abs(want[1:] - sol).max()
        print(f"{name} order {order}: checker against solve_toeplitz {err:.3g}")
        assert want[0] == 1.0 and err <= 1e-9, (name, order, err)
        got = amlib.whiten_taps(r, 60.0)
        assert got.dtype == np.float32 and got.shape == (order + 1,) and got[0] == 1.0
        ulp = np.spacing(np.maximum(1.0, np.abs(want)).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= ulp).all(), (name, order)
    if name == "white":   # on white input the filter changes (nearly) nothing
        assert np.abs(amlib.whiten_taps(r_all[:33])[1:]).max() < 0.05


def test_whiten_taps_special_inputs(amlib):
    L = amlib.lib()
    assert amlib.whiten_taps([1.0, 0.0, 0.0]).tolist() == [1.0, 0.0, 0.0]
    assert amlib.whiten_taps([0.0, 0.5, 0.25]).tolist() == [1.0, 0.0, 0.0]          # r[0] = 0: silence
    assert amlib.whiten_taps([-1.0, 0.5]).tolist() == [1.0, 0.0]
    # |k| >= 1 at the first step: the recursion stops there, the remaining taps are 0
    assert amlib.whiten_taps([1.0, 2.0, 0.5], 200.0).tolist() == ref.whiten_taps([1.0, 2.0, 0.5], 200.0).tolist() == [1.0, 0.0, 0.0]
    # ... and at the second: the first tap stays
    got, want = amlib.whiten_taps([1.0, 0.5, -2.0], 200.0), ref.whiten_taps([1.0, 0.5, -2.0], 200.0)
    assert want[2] == 0.0 and want[1] != 0.0 and got.tolist() == want.astype(np.float32).tolist()
    r = (C.c_double * 66)(*([1.0] + [0.0] * 65))
    taps = (C.c_float * 66)()
    bad = amlib.AM_ERR_INVALID_ARG
    assert L.am_whiten_taps(r, 0, 60.0, taps) == bad and b"order must be in 1..64" in L.am_last_error_string()
    assert L.am_whiten_taps(r, 65, 60.0, taps) == bad
    assert L.am_whiten_taps(None, 2, 60.0, taps) == bad
    assert L.am_whiten_taps(r, 2, 60.0, None) == bad
    assert L.am_whiten_taps(r, 2, -0.5, taps) == bad and b"noise_db" in L.am_last_error_string()
    assert L.am_whiten_taps(r, 2, 200.5, taps) == bad
    assert L.am_whiten_taps(r, 2, float("nan"), taps) == bad
    assert L.am_whiten_taps(r, 64, 0.0, taps) == 0 and L.am_whiten_taps(r, 64, 200.0, taps) == 0
    for v in (float("nan"), float("inf"), float("-inf")):
        r2 = (C.c_double * 3)(1.0, 0.5, v)
        assert L.am_whiten_taps(r2, 2, 60.0, taps) == bad
        assert L.am_whiten_taps(r2, 1, 60.0, taps) == 0          # (r[2] is not read at order 1)
    with pytest.raises(amlib.AudioMatchError):
        amlib.whiten_taps([1.0])


def no_device(amlib, rc):
    """what a valid call gives on a machine without a device (with one, it simply succeeds)"""
    return rc in (amlib.AM_ERR_NO_DEVICE, amlib.AM_ERR_HIP) or (rc == 0 and amlib.device_count() > 0)


def test_lag_products_arguments_before_any_device(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    x = np.zeros(16, np.float32)
    r = (C.c_double * 66)(*([7.0] * 66))
    for fn in (L.am_lag_products, L.am_lag_products_device):
        assert fn(0, x.ctypes.data, 16, 0, 0, r) == bad and b"order must be in 1..64" in L.am_last_error_string()
        assert fn(0, x.ctypes.data, 16, 0, 65, r) == bad
        assert fn(0, x.ctypes.data, 16, 7, 4, r) == bad and b"bad sample format" in L.am_last_error_string()
        assert fn(0, x.ctypes.data, 16, 0, 4, None) == bad
        assert fn(0, None, 16, 0, 4, r) == bad
        assert fn(999, None, 16, 0, 4, r) == bad                 # argument errors come before the device
        assert list(r)[:6] == [7.0] * 6
        assert fn(0, None, 0, 0, 4, r) == 0 and list(r)[:6] == [0.0] * 5 + [7.0]   # n = 0: zeros, nothing launched
        for i in range(5):
            r[i] = 7.0
        assert fn(999, None, 0, 1, 4, r) == 0                    # ... on any device ordinal
        for i in range(5):
            r[i] = 7.0
    assert no_device(amlib, L.am_lag_products(0, x.ctypes.data, 16, 0, 4, r))
    assert amlib.lag_products(np.zeros(0, np.float32), 3).tolist() == [0.0] * 4


def test_fir_arguments_before_any_device(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    x = np.zeros(16, np.float32)
    out = np.full(32, 5.0, np.float32)
    n = C.c_size_t(77)
    taps = (C.c_float * 66)(*([0.5] * 66))
    for fn in (L.am_fir, L.am_fir_device):
        assert fn(0, x.ctypes.data, 16, 0, taps, 0, 0, out.ctypes.data, 32, C.byref(n)) == bad
        assert b"n_taps must be in 1..65" in L.am_last_error_string()
        assert fn(0, x.ctypes.data, 16, 0, taps, 66, 0, out.ctypes.data, 32, C.byref(n)) == bad
        assert fn(0, x.ctypes.data, 16, 0, None, 2, 0, out.ctypes.data, 32, C.byref(n)) == bad
        assert fn(0, x.ctypes.data, 16, 7, taps, 2, 0, out.ctypes.data, 32, C.byref(n)) == bad
        assert fn(0, x.ctypes.data, 16, 0, taps, 2, 17, out.ctypes.data, 32, C.byref(n)) == bad and b"lead" in L.am_last_error_string()
        assert fn(0, x.ctypes.data, 16, 0, taps, 2, 0, out.ctypes.data, 32, None) == bad
        assert fn(0, None, 16, 0, taps, 2, 0, out.ctypes.data, 32, C.byref(n)) == bad
        assert fn(0, x.ctypes.data, 16, 0, taps, 2, 0, None, 32, C.byref(n)) == bad
        for v in (float("nan"), float("inf")):
            t2 = (C.c_float * 3)(1.0, v, 0.5)
            assert fn(0, x.ctypes.data, 16, 0, t2, 3, 0, out.ctypes.data, 32, C.byref(n)) == bad and b"tap 1 is not finite" in L.am_last_error_string()
            assert fn(0, None, 0, 0, t2, 1, 0, None, 0, C.byref(n)) == 0          # (tap 1 is not read with one tap)
        n.value = 77
        assert fn(999, x.ctypes.data, 16, 0, taps, 2, 3, out.ctypes.data, 12, C.byref(n)) == amlib.AM_ERR_CAPACITY
        assert n.value == 13 and b"13 samples needed" in L.am_last_error_string()
        assert fn(999, x.ctypes.data, 16, 0, taps, 65, 16, out.ctypes.data, 0, C.byref(n)) == 0 and n.value == 0   # n_in == lead
        assert fn(999, None, 0, 1, taps, 1, 0, None, 0, C.byref(n)) == 0 and n.value == 0                        # n_in = 0
        assert (out == 5.0).all()
    assert no_device(amlib, L.am_fir(0, x.ctypes.data, 16, 0, taps, 2, 0, out.ctypes.data, 32, C.byref(n)))
    assert amlib.fir(np.zeros(3, np.float32), [1.0, -0.5], lead=3).size == 0


def test_needle_create_filtered_arguments_before_any_device(amlib):
    L = amlib.lib()
    bad = amlib.AM_ERR_INVALID_ARG
    x = np.ones(16, np.float32)
    taps = (C.c_float * 66)(*([0.5] * 66))
    h = C.c_void_p()
    assert L.am_needle_create_filtered(999, x.ctypes.data, 0, 0, taps, 2, C.byref(h)) == bad
    assert L.am_needle_create_filtered(999, None, 16, 0, taps, 2, C.byref(h)) == bad
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 0, taps, 2, None) == bad
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 3, taps, 2, C.byref(h)) == bad
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 0, taps, 0, C.byref(h)) == bad
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 0, taps, 66, C.byref(h)) == bad
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 0, None, 2, C.byref(h)) == bad
    t2 = (C.c_float * 2)(1.0, float("nan"))
    assert L.am_needle_create_filtered(999, x.ctypes.data, 16, 0, t2, 2, C.byref(h)) == bad
    assert not h.value
    rc = L.am_needle_create_filtered(0, x.ctypes.data, 16, 0, taps, 2, C.byref(h))
    assert no_device(amlib, rc)
    if rc == 0:
        L.am_needle_destroy(h)


def test_checker_fir_pieces_and_nonfinite():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(300)
    taps = rng.standard_normal(9)
    full = ref.fir(x, taps)
    assert np.allclose(full, np.convolve(x, taps)[:x.size], rtol=0, atol=1e-12)
    for a in (1, 7, 8, 9, 100):
        l = min(a, taps.size - 1)
        assert np.array_equal(ref.fir(x[a - l:250], taps, lead=l), full[a:250])
    x[120] = np.nan
    y = ref.fir(x, taps)
    assert np.isnan(y[120:129]).all() and np.isfinite(np.delete(y, range(120, 129))).all()
    r, mag = ref.lag_products(x, 4)
    x[120] = 0.0
    assert np.array_equal(r, ref.lag_products(x, 4)[0]) and (mag >= np.abs(r)).all()


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("whiten=%u preemphasis=%g files=%zu\n", a.whiten, a.preemphasis ? (double)*a.preemphasis : -1.0, a.within.size());
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_whiten(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    base = ("a.wav", "--snippet", "s.wav")
    assert run(*base) == (0, "whiten=0 preemphasis=-1 files=1\n")
    assert run(*base, "--whiten", "8") == (0, "whiten=8 preemphasis=-1 files=1\n")
    assert run("--whiten", "64", "a.wav", "b.wav", "--snippet", "s.wav") == (0, "whiten=64 preemphasis=-1 files=2\n")
    assert run(*base, "--whiten", "1")[0] == 0
    assert run(*base, "--preemphasis", "0.95") == (0, "whiten=0 preemphasis=0.95 files=1\n")
    for v in ("0", "65", "-3", "8.5", "x", ""):
        code, out = run(*base, "--whiten", v)
        assert code == 2 and "for --whiten (the filter's order, 1..64)" in out, (v, out)
    for v in ("0", "1", "1.5", "-0.5", "nan", "a", ""):
        code, out = run(*base, "--preemphasis", v)
        assert code == 2 and "for --preemphasis (a number with 0 < A < 1)" in out, (v, out)
    code, out = run(*base, "--whiten")
    assert code == 2 and "missing value for --whiten" in out
    code, out = run(*base, "--whiten", "8", "--preemphasis", "0.9")
    assert code == 2 and "--whiten and --preemphasis are mutually exclusive" in out
    live = ("--live", "--rate", "8000", "--snippet", "s.wav")
    assert run(*live)[0] == 0
    for extra in (("--whiten", "8"), ("--preemphasis", "0.95")):
        code, out = run(*live, *extra)
        assert code == 2 and "--live: --whiten and --preemphasis do not apply" in out, out
    code, out = run("--help")
    assert code == 0 and re.search(r"^  --whiten P {2,}\S", out, re.M) and re.search(r"^  --preemphasis A {2,}\S", out, re.M), out
    assert all(len(ln) <= 120 for ln in out.splitlines())
