"""CPU tests of the score traces (include/audiomatch.h, "score traces"): the numpy reference against a plain loop, the
designed cases against their claims, the pure-host entry points am_trace_len and am_trace_summary against the
reference, that header, C++ mirror and Rust binding name every new symbol, and the CLI's argument errors."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import trace_cases as tc
import trace_ref as tr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["am_trace_len", "am_trace_scores", "am_trace_scores_device", "am_match_trace", "am_match_trace_device",
       "am_match_trace_batch_device", "am_trace_summary"]


def header_constants():
    txt = open(os.path.join(ROOT, "include", "audiomatch.h")).read()
    w = int(re.search(r"#define AM_TRACE_WAVE_BIN_MAX (\d+)", txt).group(1))
    sl = int(re.search(r"#define AM_TRACE_SLICE (\d+)", txt).group(1))
    return w, sl


def test_reference_equals_plain_loop():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 130):
        x = rng.integers(-50, 51, size=n).astype(np.float32)
        x[rng.random(n) < 0.2] = np.nan
        if n > 4:
            x[1], x[3] = np.float32(0.0), np.float32(-0.0)
        for D in (1, 2, 3, 5, 64, 65, 200):
            assert tr.same_bits(tr.trace(x, D), tr.trace_loop(x, D)), (n, D)
    x = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 3, 3, np.nan], dtype=np.float32)
    for D in (1, 2, 4, 8, 9):
        a, b = tr.trace(x, D), tr.trace_loop(x, D)
        assert tr.same_fields(a, b) and tr.n_bins(x.size, D) == a.size, D
        for f in ("sum", "sumsq"):             # (inf - inf: NaN on both sides)
            assert np.array_equal(a[f], b[f], equal_nan=True), (D, f)
    assert tr.trace(np.zeros(0, np.float32), 4).size == 0


@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_cases_hold_their_claims_under_the_reference(case):
    W, SL = header_constants()
    pinned = 0
    for D in tc.bin_lengths(W, SL):
        for n in tc.score_counts(D):
            x, claims = tc.build(case, D, n, SL)
            assert x.size == n and n <= 1 << 22
            fin = x[np.isfinite(x)]
            assert np.all(fin == np.rint(fin)) and np.all(np.abs(fin) <= 2 ** 12)
            assert tc.check_claims(tr.trace(x, D), claims) == [], (case, D, n)
            pinned += sum(len(c) for c in claims)
    assert pinned > 0


def test_tie_cases_reach_two_lanes_two_steps_and_two_slices():
    """The same extreme twice: every distance occurs, and in every bin longer than a slice the two lie in two slices, so
    only the fold of the partials can decide between them -- for the maximum and for the minimum."""
    W, SL = header_constants()
    for kind in ("max", "min"):
        for which in tc.TWICE:
            want = {"slice": SL, "slice+1": SL + 1}.get(which) or int(which)
            dists, cross, same_place = set(), 0, 0
            for D in tc.bin_lengths(W, SL):
                for n in tc.score_counts(D):
                    x, claims = tc.build("twice_%s_%s" % (kind, which), D, n, SL)
                    for b, c in enumerate(claims):
                        if "_pair" not in c:
                            continue
                        p, q = c["_pair"]
                        L = min(D, n - b * D)
                        assert 0 <= p < q < L and x[b * D + p] == x[b * D + q] == (tc.TOP if kind == "max" else -tc.TOP)
                        assert c["arg" + kind] == p
                        dists.add(q - p)
                        if L > SL:
                            assert p // SL != q // SL, (kind, which, D, n, b)
                            cross += 1
                        same_place += (q - p) % 256 == 0
            assert want in dists, (kind, which, dists)
            assert cross >= 6, (kind, which)
            if which == "256":
                assert same_place > 0


def test_slice_cases_make_every_slice_the_deciding_one():
    """At D = 5 SL + 7 the six slices (the last one of 7 scores) each hold the maximum at their first offset in one case
    and at their last offset in another; the mirrored minimum does the same from the other end."""
    W, SL = header_constants()
    D = 5 * SL + 7
    for kind in ("first", "last"):
        seen = set()
        for k in range(6):
            x, claims = tc.build("slice_%s_%d" % (kind, k), D, 3 * D + 1, SL)
            for b, c in enumerate(claims[:3]):
                s = c["_slice"]
                want = s * SL if kind == "first" else min(D, (s + 1) * SL) - 1
                assert c["argmax"] == want and x[b * D + want] == tc.TOP
                seen.add(s)
        assert seen == set(range(6)), (kind, seen)


def test_header_order_model_is_a_reordering_of_the_same_sums():
    """trace_ordered (the order the header documents) against the plain sums: equal bits on integers, within sum_bound on
    noise; and it is not numpy's order (so a test against it pins the header's)."""
    W, SL = header_constants()
    rng = np.random.default_rng(3)
    ints = rng.integers(-4096, 4097, size=3 * SL + 100).astype(np.float32)
    ints[::97] = np.nan
    noise = rng.standard_normal(3 * SL + 100).astype(np.float32) * np.float32(1e3)
    differs = False
    for D in (1, 3, 255, 256, 257, 1000, SL, SL + 1, 2 * SL + 1):
        for sliced in (False, True):
            assert tr.same_bits(tr.trace_ordered(ints, D, sliced, SL), tr.trace(ints, D)), (D, sliced)
            got, ref = tr.trace_ordered(noise, D, sliced, SL), tr.trace(noise, D)
            bs, bq = tr.sum_bound(noise, D)
            assert tr.same_fields(got, ref)
            assert np.all(np.abs(got["sum"] - ref["sum"]) <= bs) and np.all(np.abs(got["sumsq"] - ref["sumsq"]) <= bq), (D, sliced)
            differs = differs or not tr.same_bits(got, ref)
    assert differs


def test_header_names_the_constants_and_the_binding_agrees(amlib):
    W, SL = header_constants()
    assert 64 <= W <= SL and SL % 256 == 0
    assert (amlib.AM_TRACE_WAVE_BIN_MAX, amlib.AM_TRACE_SLICE) == (W, SL)
    assert amlib.TRACE_BIN_DTYPE == tr.BIN_DTYPE and amlib.TRACE_BIN_DTYPE.itemsize == 40
    assert C.sizeof(amlib.AmTraceParams) == 16 and C.sizeof(amlib.AmTraceStats) == 80


def test_trace_len(amlib):
    n = C.c_size_t(99)
    L = amlib.lib()
    for ns, D in ((0, 1), (1, 1), (10, 3), (9, 3), (1, 1 << 30), ((1 << 40) + 1, 1 << 30)):
        assert L.am_trace_len(ns, D, C.byref(n)) == 0 and n.value == tr.n_bins(ns, D) == amlib.trace_len(ns, D)
    for D in (0, (1 << 30) + 1):
        assert L.am_trace_len(10, D, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
        assert b"bin" in L.am_last_error_string()
    assert L.am_trace_len(10, 4, None) == amlib.AM_ERR_INVALID_ARG


def summary_of(amlib, bins, D):
    st = amlib.trace_summary(bins, D)
    return {f: getattr(st, f) for f in tr.SUMMARY_FIELDS}


def same_summary(a, b):
    for f in tr.SUMMARY_FIELDS:
        x, y = a[f], b[f]
        if isinstance(y, float) and math.isnan(y):
            if not math.isnan(x):
                return False
        elif x != y:
            return False
    return True


def test_trace_summary_equals_reference(amlib):
    rng = np.random.default_rng(9)
    x = rng.standard_normal(5000).astype(np.float32)
    x[700:1300] = np.nan                                  # bins without a score in between
    x[4000] = 7.5
    x[4100] = 7.5                                         # the same maximum twice: the first one's offset
    x[10], x[2000] = -9.0, -9.0
    for D in (1, 7, 100, 256, 5000, 6000):
        bins = tr.trace(x, D)
        want = tr.summary(bins, D)
        assert same_summary(want, tr.summary_loop(bins, D)), D
        assert same_summary(summary_of(amlib, bins, D), want), (D, summary_of(amlib, bins, D), want)
        assert want["argmax"] == 4000 and want["argmin"] == 10 and want["count"] == 4400
    # no bins, and bins without a counted score: NaN fields, count 0
    for bins in (np.zeros(0, tr.BIN_DTYPE), tr.trace(np.full(10, np.nan, np.float32), 4)):
        got = summary_of(amlib, bins, 4)
        assert same_summary(got, tr.summary(bins, 4)) and got["count"] == 0 and math.isnan(got["peak_z"]) and math.isnan(got["max"])
    # MAD = 0: peak_z is +inf when the maximum stands above the median, otherwise 0
    flat = np.full(40, 2.0, np.float32)
    got = summary_of(amlib, tr.trace(flat, 4), 4)
    assert got["mad_max"] == 0 and got["peak_z"] == 0 and got["std"] == 0 and same_summary(got, tr.summary(tr.trace(flat, 4), 4))
    flat[17] = 5.0
    got = summary_of(amlib, tr.trace(flat, 4), 4)
    assert got["mad_max"] == 0 and got["peak_z"] == math.inf and got["argmax"] == 17
    assert same_summary(got, tr.summary(tr.trace(flat, 4), 4))
    # infinite maxima: a maximum equal to an infinite median deviates by 0; +inf and -inf in the middle: no median
    for vals in ((np.inf, np.inf, 1.0), (np.inf, 2.0, 1.0, -np.inf), (np.inf, -np.inf), (np.inf, np.inf, np.inf, 1.0, 2.0),
                 (-np.inf, -np.inf, 3.0)):
        y = np.repeat(np.array(vals, dtype=np.float32), 4)
        y[1::4] -= 1                                       # (each bin's maximum is its first score)
        bins = tr.trace(y, 4)
        want = tr.summary(bins, 4)
        assert same_summary(want, tr.summary_loop(bins, 4)), vals
        assert same_summary(summary_of(amlib, bins, 4), want), (vals, summary_of(amlib, bins, 4), want)
    assert tr.summary(tr.trace(np.repeat(np.float32([np.inf, np.inf, 1.0]), 4), 4), 4)["mad_max"] == 0
    assert math.isnan(tr.summary(tr.trace(np.repeat(np.float32([np.inf, -np.inf]), 4), 4), 4)["median_max"])
    # a single bin
    got = summary_of(amlib, tr.trace(x[:50], 64), 64)
    assert same_summary(got, tr.summary(tr.trace(x[:50], 64), 64)) and got["peak_z"] == 0
    st = amlib.AmTraceStats()
    assert amlib.lib().am_trace_summary(None, 3, 4, C.byref(st)) == amlib.AM_ERR_INVALID_ARG
    assert amlib.lib().am_trace_summary(None, 0, 0, C.byref(st)) == amlib.AM_ERR_INVALID_ARG
    assert amlib.lib().am_trace_summary(None, 0, 4, None) == amlib.AM_ERR_INVALID_ARG


def test_header_mirror_and_rust_name_every_symbol(amlib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "audiomatch.h")).read(), flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in amlib.declared_symbols() and name in exported, name
        assert name + "(" in hpp, name
        assert "pub fn " + name + "(" in rust, name
    for struct in ("am_trace_bin", "am_trace_params", "am_trace_stats"):
        assert "typedef struct " + struct in code
    assert "pub struct AmTraceBin" in rust and "pub struct AmTraceParams" in rust
    for fn in ("trace_len", "trace_scores", "trace_scores_device", "trace_summary", "trace_params"):
        assert callable(getattr(amlib, fn))
    for fn in ("match_trace", "match_trace_device", "match_trace_batch_device"):
        assert callable(getattr(amlib.HipConvolve, fn))
    assert amlib.lib().am_abi_version() == 3


def test_cli_argument_errors():
    import build as am_build
    cli = am_build.build_cli()
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--score-trace PREFIX[:BIN]" in out.stdout
    base = [cli, "hay.wav", "--snippet", "a.wav"]
    for bad in (["--score-trace"], ["--score-trace", ""], ["--score-trace", ":1s"], ["--score-trace", "curve:0s"],
                ["--score-trace", "curve:0"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and "--score-trace" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "--live", "--rate", "8000", "--snippet", "a.wav", "--score-trace", "curve"], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--live: --score-trace does not apply" in r.stderr
