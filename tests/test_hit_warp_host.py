"""Host-side checks of per-hit drift scoring (no device): the header, the exports and the record sizes, am_warp_table
against the numpy formula, the checker of tests/hit_warp_ref.py by itself (warped lengths, the designs on planted drifts,
the estimation rows), am_hit_window_warped against the checker bit for bit and the argument checks of every entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hit_warp_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_warp_table", "am_hit_warp", "am_hit_warp_device", "am_hit_warp_batch_device", "am_hit_window_warped")


@pytest.fixture(scope="module")
def table(amlib):
    return amlib.warp_table()


def plant(seed, s, n, t, ppm, noise=0.001):
    """The generator of test_gpu_hit_segments.test_drift: a smoothed-noise needle of s samples, planted at t by linear
    interpolation at `ppm` in noise."""
    eps = ppm * 1e-6
    rng = np.random.default_rng(seed)
    needle = np.convolve(rng.normal(0, 0.3, s + 7), np.ones(8) / 8, mode="valid").astype(np.float32)
    hay = rng.normal(0, noise, n).astype(np.float32)
    k = np.arange(int(s * (1 + eps)) + 1)
    hay[t:t + len(k)] += np.interp(k / (1 + eps), np.arange(s), needle.astype(np.float64), right=0.0).astype(np.float32)
    return needle, hay


# (name, needle length, haystack length, planted ppm, (centre, max_ppm, K, R), planted cell, drift tolerance in ppm)
PLANTS = [
    ("+200", 40_000, 50_000, 200.0, (0.0, 400.0, 8, 4), 12, 2.0),
    ("-1000", 40_000, 50_000, -1000.0, (0.0, 2000.0, 8, 4), 4, 2.0),
    ("+2000", 5_000, 12_000, 2000.0, (0.0, 8000.0, 8, 4), 10, 10.0),    # 1 % of the 1000 ppm step
]
PLANT_T = 3000


def test_header_declares_warp_and_library_exports_it(amlib):
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h
    for name, val in (("AM_WARP_PHASES", 4096), ("AM_WARP_TAPS", 32), ("AM_WARP_MAX_STEPS", 32), ("AM_WARP_MAX_PPM", 50000)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), h), name
        assert getattr(amlib, name) == val
    assert "AM_HIT_DRIFT_UNREFINED = 256" in h and amlib.AM_HIT_DRIFT_UNREFINED == 256 == ref.DRIFT_UNREF
    assert "the rows are not resampled here" not in h and "am_hit_window_warped" in h
    assert "the rows are not resampled here" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(FUNCS) <= exported and set(FUNCS) <= set(amlib.declared_symbols())
    assert amlib.lib().am_abi_version() == 3
    assert C.sizeof(amlib.HitWarp) == 40 and C.sizeof(amlib.AmWarpParams) == 24
    for name in FUNCS:
        assert name in open(os.path.join(ROOT, "include", "audiomatch.hpp")).read(), name
        assert "pub fn " + name + "(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read(), name


def test_warp_table(amlib, table):
    want = ref.table_formula()
    assert table.shape == (ref.PHASES, ref.TAPS) and table.dtype == np.float32
    err = np.abs(table.astype(np.float64) - want).max()
    print("table against the formula:", err)
    assert err <= 1e-7
    delta = np.zeros(ref.TAPS, dtype=np.float32)
    delta[15] = 1.0
    assert table[0].tobytes() == delta.tobytes()
    assert np.abs(table.astype(np.float64).sum(axis=1) - 1.0).max() <= 2e-7
    assert amlib.warp_table().tobytes() == table.tobytes()
    assert amlib.lib().am_warp_table(None) == amlib.AM_ERR_INVALID_ARG


def test_checker_warp_identity_and_lengths(table):
    rng = np.random.default_rng(5)
    n = rng.normal(0, 1, 5000).astype(np.float32)
    assert ref.warp(n, 0.0, table).tobytes() == n.tobytes()
    for d in (-50_000, -1, 1, 50_000):
        inc = ref.llround(2.0 ** 32 / (1 + d * 1e-6))
        for s in (1, 2, 37, 5000):
            want = ((s - 1) * 2 ** 32) // inc + 1
            assert len(ref.warp(n[:s], float(d), table)) == want == ref.warp_len(s, float(d)), (d, s)
            assert (want >= s) == (d > 0) or want == s, (d, s, want)


def _f32_of(x):
    a = np.asarray(x)
    if a.dtype == np.int16:
        k = np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0))
        f = a.reshape(-1, 2).astype(np.int32)
        return ((f[:, 0] + f[:, 1]).astype(np.float32) * k).astype(np.float32)
    return a.astype(np.float32)


def _check_row(amlib, table, x, **kw):
    got = amlib.hit_window_warped(x, **kw)
    want = ref.window_warped(_f32_of(x), h=table, **kw)
    assert np.array_equal(ref.row_bits(got), ref.row_bits(want)), kw
    return got


def test_window_warped_against_checker(amlib, table):
    rng = np.random.default_rng(77)
    n = 3000
    xf = rng.normal(0, 0.3, n).astype(np.float32)
    xi = rng.integers(-20000, 20000, size=(n, 2)).astype(np.int16)
    for x in (xf, xi):
        for drift in (300.0, -300.0, 0.0):
            # in the middle, with a lag and a lead
            row = _check_row(amlib, table, x, start=700, scale=1.25, lag=0.37, drift_ppm=drift, lead=40, length=1500)
            assert np.isfinite(row).all()
            # at the start: the elements in front of the haystack, and those whose taps reach in front of it, are absent
            row = _check_row(amlib, table, x, start=0, scale=0.5, lag=0.37, drift_ppm=drift, lead=25, length=400)
            assert np.isnan(row[:25]).all() and np.isfinite(row[60:]).all() and np.isnan(row).sum() >= 25 + 14
            # at the end
            row = _check_row(amlib, table, x, start=n - 300, scale=2.0, lag=-0.37, drift_ppm=drift, lead=0, length=400)
            assert np.isnan(row[300:]).all() and np.isfinite(row[:250]).all() and np.isnan(row).sum() >= 100 + 14
        # lag 0 and drift 0: am_hit_window's row, bit for bit (absent elements included)
        for start, lead, length in ((700, 40, 1500), (0, 25, 400), (n - 300, 0, 400)):
            a = amlib.hit_window_warped(x, start=start, scale=1.25, lag=0.0, drift_ppm=0.0, lead=lead, length=length)
            b = amlib.hit_window(x, start, 1.25, lead, length)
            assert np.array_equal(ref.row_bits(a), ref.row_bits(b))
            _check_row(amlib, table, x, start=start, scale=1.25, lag=0.0, drift_ppm=0.0, lead=lead, length=length)


def test_window_warped_nan_sample(amlib, table):
    rng = np.random.default_rng(78)
    x = rng.normal(0, 0.3, 2000).astype(np.float32)
    x[1000] = np.nan
    kw = dict(start=600, scale=1.0, lag=0.37, drift_ppm=300.0, lead=0, length=800)
    row = _check_row(amlib, table, x, **kw)
    # exactly the elements whose non-zero taps read sample 1000: the checker's m and p say which
    inc = ref.llround(2.0 ** 32 * (1 + 300e-6))
    base = (600 << 32) + ref.llround(0.37 * 2.0 ** 32) + (1 << 19)
    want = []
    for i in range(800):
        u = base + i * inc
        m, p = u >> 32, (u >> 20) & 4095
        k = 1000 - (m - 15)
        want.append(0 <= k < 32 and table[p, k] != 0)
    assert np.array_equal(np.isnan(row), np.array(want)) and 30 <= sum(want) <= 33
    # a phase-0 element beside the NaN reads its one sample only
    row = _check_row(amlib, table, x, start=600, scale=1.0, lag=0.0, drift_ppm=0.0, lead=0, length=800)
    assert np.isnan(row).sum() == 1 and np.isnan(row[400])


def test_window_warped_errors(amlib):
    L = amlib.lib()
    x = np.zeros(100, dtype=np.float32)
    row = np.zeros(10, dtype=np.float32)
    ok = dict(hay=x.ctypes.data, n=100, fmt=0, start=0, scale=1.0, lag=0.0, drift=0.0, lead=0, length=10, row=row.ctypes.data)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.am_hit_window_warped(a["hay"], a["n"], a["fmt"], a["start"], a["scale"], a["lag"], a["drift"], a["lead"], a["length"], a["row"])
        return rc, (L.am_last_error_string() or b"").decode()
    assert call()[0] == amlib.AM_OK
    for kw, word in ((dict(row=None), "null"), (dict(hay=None), "null"), (dict(fmt=7), "format"), (dict(length=0), "length"),
                     (dict(scale=0.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(lag=float("nan")), "lag"),
                     (dict(lag=2.0 ** 30), "lag"), (dict(drift=50_001.0), "drift_ppm"), (dict(drift=float("nan")), "drift_ppm"),
                     (dict(start=1 << 62), "start")):
        rc, msg = call(**kw)
        assert rc == amlib.AM_ERR_INVALID_ARG and word in msg, (kw, msg)


@pytest.fixture(scope="module")
def plant_records(table):
    """The checker's record of each plant (shared: a record takes a few hundred milliseconds)."""
    out = {}
    for name, s, n, ppm, wp, cell, tol in PLANTS:
        needle, hay = plant(21, s, n, PLANT_T, ppm)
        out[name] = ref.warp_ref(hay, needle, PLANT_T, wp, table)
    return out


@pytest.mark.parametrize("name,s,n,ppm,wp,cell,tol", PLANTS, ids=[p[0] for p in PLANTS])
def test_design_on_planted_drifts(plant_records, name, s, n, ppm, wp, cell, tol):
    e = plant_records[name]
    print(f"{name} ppm: cell {e.qstar} lag {e.lstar} margin {e.margin:.4g} ncc {e.ncc:.4f} ncc_centre {e.ncc_centre:.4f} "
          f"drift {e.drift_ppm:.3f} flags {e.flags}")
    assert e.qstar == cell and e.margin > 1e-3
    assert e.ncc >= 0.95 and e.ncc_centre <= 0.6
    assert abs(e.drift_ppm - ppm) <= tol and not e.flags & ref.DRIFT_UNREF


def test_design_off_grid_plant(table):
    needle, hay = plant(21, 40_000, 50_000, PLANT_T, 230.0)
    e = ref.warp_ref(hay, needle, PLANT_T, (0.0, 400.0, 8, 4), table)
    print(f"+230 ppm on the 50 ppm grid: cell {e.qstar} ncc {e.ncc:.4f} drift {e.drift_ppm:.2f}")
    assert e.qstar in (12, 13) and abs(e.drift_ppm - 230.0) <= 10.0 and not e.flags & ref.DRIFT_UNREF


def test_design_estimation_rows(table):
    """Nine occurrences at drifts -300 .. +300 ppm, three of them under an overlay: the median of rows cut on the needle's
    clock against the median of plain rows.  The background's own share of a median of nine is 1.25 / 3 of its rms."""
    s, t, n = 40_000, 100, 40_400
    rng = np.random.default_rng(21)
    needle = np.convolve(rng.normal(0, 0.3, s + 7), np.ones(8) / 8, mode="valid").astype(np.float32)
    rms = float(np.sqrt(np.mean(needle.astype(np.float64) ** 2)))
    ratio = 0.33
    warped, plain = [], []
    for i, ppm in enumerate(np.linspace(-300.0, 300.0, 9)):
        eps = ppm * 1e-6
        hay = rng.normal(0, ratio * rms, n).astype(np.float32)
        k = np.arange(int(s * (1 + eps)) + 1)
        hay[t:t + len(k)] += np.interp(k / (1 + eps), np.arange(s), needle.astype(np.float64), right=0.0).astype(np.float32)
        if i % 3 == 1:
            # the overlay: other programme at the needle's own level.  Three of nine rows with sqrt(1 + 1 / ratio^2) = 3.2
            # times the background's spread raise the spread of the median by 1.28 (order statistics of the mixture), an
            # overlay of any level by at most 1.49: the 1.5 below
            hay += rng.normal(0, rms, n).astype(np.float32)
        warped.append(ref.window_warped(hay, t, 1.0, 0.0, float(ppm), 0, s, table))
        plain.append(ref.window_warped(hay, t, 1.0, 0.0, 0.0, 0, s, table))
    inner = slice(16, s - 16)       # (the first and last taps of a warped row reach outside the planted occurrence)
    err = {}
    for name, rows in (("warped", warped), ("plain", plain)):
        med = np.nanmedian(np.stack(rows).astype(np.float64), axis=0)
        err[name] = float(np.sqrt(np.mean((med[inner] - needle[inner].astype(np.float64)) ** 2))) / rms
    share = ratio * 1.25 / 3
    print(f"median of nine: warped rows miss the needle by {err['warped']:.3f} of its rms, plain rows by {err['plain']:.3f}; "
          f"the background's share {share:.3f}")
    assert err["warped"] < err["plain"] and err["warped"] <= 1.5 * share


def test_entry_points_check_arguments_without_a_device(amlib):
    L = amlib.lib()
    peaks = (amlib.AmPeak * 1)(amlib.AmPeak(0, 1, 1.0, 1.0))
    out = (amlib.HitWarp * 1)()
    x = np.zeros(64, dtype=np.float32)
    good = amlib.AmWarpParams(0.0, 400.0, 8, 4)
    bad = [(amlib.AmWarpParams(0.0, 400.0, 33, 4), "steps"), (amlib.AmWarpParams(0.0, 400.0, 8, 17), "radius"),
           (amlib.AmWarpParams(0.0, -1.0, 8, 4), "max_ppm"), (amlib.AmWarpParams(0.0, 0.0, 8, 4), "max_ppm"),
           (amlib.AmWarpParams(-49_900.0, 200.0, 8, 4), "centre_ppm"), (amlib.AmWarpParams(0.0, 50_001.0, 0, 4), "centre_ppm")]
    one = (C.c_size_t * 1)(64)
    counts = (C.c_size_t * 1)(1)
    hays = (C.c_void_p * 1)(x.ctypes.data)
    handles = (C.c_void_p * 1)(None)

    def forms(wp, fmt=0):
        w = C.byref(wp) if wp is not None else None
        yield "am_hit_warp", L.am_hit_warp(None, x.ctypes.data, 64, fmt, peaks, 1, w, out)
        yield "am_hit_warp_device", L.am_hit_warp_device(None, x.ctypes.data, 64, fmt, peaks, 1, w, out)
        yield "am_hit_warp_batch_device", L.am_hit_warp_batch_device(handles, 1, hays, one, 1, fmt, peaks, 1, counts, w, out)

    for wp, word in bad:
        for name, rc in forms(wp):
            msg = (L.am_last_error_string() or b"").decode()
            assert rc == amlib.AM_ERR_INVALID_ARG and word in msg, (name, word, msg)
    for name, rc in forms(good, fmt=9):
        assert rc == amlib.AM_ERR_INVALID_ARG and "format" in (L.am_last_error_string() or b"").decode(), name
    for name, rc in forms(good):          # a null needle handle
        assert rc == amlib.AM_ERR_INVALID_ARG and "null" in (L.am_last_error_string() or b"").decode(), name
    for name, rc in forms(None):          # no parameter block
        assert rc == amlib.AM_ERR_INVALID_ARG and "null" in (L.am_last_error_string() or b"").decode(), name
    assert L.am_hit_warp_batch_device(None, 1, hays, one, 1, 0, peaks, 1, counts, C.byref(good), out) == amlib.AM_ERR_INVALID_ARG
    assert "null pointer" in L.am_last_error_string().decode()
    assert L.am_hit_warp_batch_device(handles, 1, hays, one, 1, 0, None, 1, counts, C.byref(good), out) == amlib.AM_ERR_INVALID_ARG
    assert "null pointer" in L.am_last_error_string().decode()
    # nothing to do: AM_OK, whatever the pointers
    assert L.am_hit_warp_batch_device(handles, 0, hays, one, 1, 0, None, 1, None, C.byref(good), None) == amlib.AM_OK
