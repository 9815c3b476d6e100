"""Host-side checks of per-segment hit scoring (no device): the header's declarations, the ctypes record's layout, the
CLI's --segments flag and am_hit_segments_summary against the checker (tests/hit_segments_ref.py) and numpy.polyfit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hit_segments_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_segments_device", "am_hit_segments", "am_hit_segments_batch_device", "am_hit_segments_summary")


def test_header_declares_segment_scoring():
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    for struct in ("am_segment_params", "am_hit_segment", "am_segment_summary"):
        assert "typedef struct %s {" % struct in h and "} %s;" % struct in h, struct
    assert "AM_HIT_EMPTY_SEGMENT = 8" in h
    assert re.search(r"#define AM_SEG_MAX_SEGMENTS\s+1024\b", h) and re.search(r"#define AM_SEG_MAX_RADIUS\s+16\b", h)
    assert h.index("per-hit scoring") < h.index("per-segment hit scoring") < h.index("streaming ingest")
    assert "#define AM_ABI_VERSION 3" in h


LAYOUT_PROBE = r'''
#include <cstddef>
#include <cstdio>
#include "audiomatch.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(am_hit_segment), offsetof(am_hit_segment, lag),
                offsetof(am_hit_segment, ncc), offsetof(am_hit_segment, gain), offsetof(am_hit_segment, level_db),
                offsetof(am_hit_segment, flags), AM_HIT_EMPTY_SEGMENT, AM_SEG_MAX_SEGMENTS, AM_SEG_MAX_RADIUS);
    std::printf("%zu %zu %zu\n", sizeof(am_segment_params), offsetof(am_segment_params, segments), offsetof(am_segment_params, radius));
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(am_segment_summary), offsetof(am_segment_summary, coverage),
                offsetof(am_segment_summary, drift_ppm), offsetof(am_segment_summary, start_lag),
                offsetof(am_segment_summary, residual_rms), offsetof(am_segment_summary, first_present),
                offsetof(am_segment_summary, last_present), offsetof(am_segment_summary, n_present),
                offsetof(am_segment_summary, n_usable));
    return 0;
}
'''


def test_ctypes_records_match_header(tmp_path):
    import audiomatch_amd as am
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROBE)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    R, P, S = am.HitSegment, am.AmSegmentParams, am.AmSegmentSummary
    assert C.sizeof(R) == 24
    assert rows[0] == [C.sizeof(R), R.lag.offset, R.ncc.offset, R.gain.offset, R.level_db.offset, R.flags.offset,
                       am.AM_HIT_EMPTY_SEGMENT, am.AM_SEG_MAX_SEGMENTS, am.AM_SEG_MAX_RADIUS]
    assert rows[1] == [C.sizeof(P), P.segments.offset, P.radius.offset]
    assert rows[2] == [C.sizeof(S), S.coverage.offset, S.drift_ppm.offset, S.start_lag.offset, S.residual_rms.offset,
                       S.first_present.offset, S.last_present.offset, S.n_present.offset, S.n_usable.offset]
    assert set(FUNCS) <= set(am.declared_symbols())


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("segments=%u radius=%u\n", a.segments, a.segment_radius);
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_segments(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "segments=0 radius=4\n")
    assert run("a.wav", "--snippet", "s.wav", "--segments", "8") == (0, "segments=8 radius=4\n")
    assert run("a.wav", "--snippet", "s.wav", "--segments", "8:2") == (0, "segments=8 radius=2\n")
    assert run("a.wav", "--snippet", "s.wav", "--segments", "1024:0") == (0, "segments=1024 radius=0\n")
    for bad in ("0", "8:17", "1025", "8:", ":2", "-3", "8:-1", "x", "", "8:2:1", "8.5"):
        code, out = run("a.wav", "--snippet", "s.wav", "--segments", bad)
        assert code == 2 and "--segments" in out, (bad, out)
    code, out = run("a.wav", "--snippet", "s.wav", "--segments")
    assert code == 2 and "--segments" in out
    code, out = run("--snippet", "s.wav", "--live", "--rate", "8000", "--segments", "8")
    assert code == 2 and "--live" in out and "--segments" in out
    code, out = run("--help")
    assert code == 0 and "--segments M[:R]" in out


# ---- am_hit_segments_summary ------------------------------------------------------------------------------------------
def records(am, rows):
    return [am.HitSegment(lag, ncc, 0.7, -3.0, flags) for lag, ncc, flags in rows]


def check_summary(am, rows, s, min_ncc=0.5):
    recs = records(am, rows)
    got = am.hit_segments_summary(recs, s, min_ncc)
    exp = ref.summary_ref(recs, s, min_ncc)
    for k in ("first_present", "last_present", "n_present", "n_usable"):
        assert getattr(got, k) == exp[k], (k, got, exp)
    assert got.coverage == exp["coverage"]
    for k in ("drift_ppm", "start_lag", "residual_rms"):
        g, e = getattr(got, k), exp[k]
        assert (np.isnan(g) and np.isnan(e)) or abs(g - e) <= 1e-9 * max(1.0, abs(e)), (k, got, exp)
    return got


def test_summary_all_present(amlib):
    m, s = 16, 40_000
    rng = np.random.default_rng(3)
    centres = np.array([(j * s // m + (j + 1) * s // m) / 2 for j in range(m)])
    lags = 0.3 + 150e-6 * centres + rng.normal(0, 0.02, m)
    got = check_summary(amlib, [(float(l), 0.9, 0) for l in lags], s)
    assert (got.coverage, got.first_present, got.last_present, got.n_present, got.n_usable) == (1.0, 0, m - 1, m, m)
    slope, icpt = np.polyfit(centres, lags, 1)
    assert abs(got.drift_ppm - 1e6 * slope) <= 1e-6 and abs(got.start_lag - icpt) <= 1e-9
    assert abs(got.residual_rms - np.sqrt(np.mean((lags - (icpt + slope * centres)) ** 2))) <= 1e-9


def test_summary_none_present(amlib):
    got = check_summary(amlib, [(0.0, 0.1, 0)] * 8, 8000)
    assert (got.coverage, got.first_present, got.last_present, got.n_present, got.n_usable) == (0.0, -1, -1, 0, 0)
    assert np.isnan(got.drift_ppm) and np.isnan(got.start_lag) and np.isnan(got.residual_rms)


def test_summary_one_usable_segment(amlib):
    rows = [(0.0, 0.2, 0), (1.25, 0.9, 0), (2.0, 0.9, ref.UNREF), (0.0, 0.3, 0)]
    got = check_summary(amlib, rows, 1000)
    assert (got.n_present, got.n_usable, got.first_present, got.last_present, got.coverage) == (2, 1, 1, 2, 0.5)
    assert np.isnan(got.drift_ppm)


def test_summary_skips_flagged_segments(amlib):
    nan = float("nan")
    rows = [(0.1, 0.9, 0), (5.0, nan, ref.NONFIN), (0.3, 0.9, 0), (7.0, 0.0, ref.BELOW), (0.0, 0.0, ref.EMPTY),
            (0.6, 0.95, 0), (3.0, 0.9, ref.UNREF), (0.8, 0.49, 0)]
    got = check_summary(amlib, rows, 8 * 512)
    assert (got.n_present, got.n_usable, got.first_present, got.last_present, got.coverage) == (4, 3, 0, 6, 0.5)
    centres = np.array([256.0, 2 * 512 + 256.0, 5 * 512 + 256.0])
    slope, icpt = np.polyfit(centres, np.array([0.1, 0.3, 0.6]), 1)
    assert abs(got.drift_ppm - 1e6 * slope) <= 1e-6 and abs(got.start_lag - icpt) <= 1e-9
    # a NaN ncc without a flag is absent too; min_ncc moves the line
    assert amlib.hit_segments_summary(records(amlib, [(0.0, nan, 0), (0.0, 0.4, 0)]), 100, 0.5).n_present == 0
    assert amlib.hit_segments_summary(records(amlib, [(0.0, nan, 0), (0.0, 0.4, 0)]), 100, 0.25).n_present == 1


def test_summary_needle_not_divisible(amlib):
    s, m = 37, 7
    a = ref.seg_bounds(s, m)
    assert a == [0, 5, 10, 15, 21, 26, 31, 37]
    rows = [(0.5 + 0.01 * j, 0.9 if j not in (2, 3) else 0.1, 0) for j in range(m)]
    got = check_summary(amlib, rows, s)
    assert got.coverage == (37 - 5 - 6) / 37 and got.n_present == 5
    centres = np.array([(a[j] + a[j + 1]) / 2 for j in (0, 1, 4, 5, 6)])
    slope, icpt = np.polyfit(centres, np.array([rows[j][0] for j in (0, 1, 4, 5, 6)]), 1)
    assert abs(got.drift_ppm - 1e6 * slope) <= 1e-4 and abs(got.start_lag - icpt) <= 1e-9


def test_summary_errors(amlib):
    L = amlib.lib()
    out = amlib.AmSegmentSummary()
    buf = (amlib.HitSegment * 4)()
    for args in ((None, 4, 100, 0.5, C.byref(out)), (buf, 4, 100, 0.5, None), (buf, 0, 100, 0.5, C.byref(out)),
                 (buf, 4, 3, 0.5, C.byref(out))):
        assert L.am_hit_segments_summary(*args) == amlib.AM_ERR_INVALID_ARG
    with pytest.raises(amlib.AudioMatchError):
        amlib.hit_segments_summary([], 100)
