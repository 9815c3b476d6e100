"""Host-side checks of per-band hit scoring (no device): the checker (tests/hit_bands_ref.py) against a direct O(F^2)
DFT, the header's declarations, the ctypes records' layout, the CLI's --bands flag, and am_hit_bands_summary and
am_band_edges_log -- pure host code, called through the built library -- against their Python twins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hit_bands_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_bands_device", "am_hit_bands", "am_hit_bands_batch_device", "am_hit_bands_summary", "am_band_edges_log")


# ---- the checker itself -------------------------------------------------------------------------------------------------
def test_checker_against_direct_dft():
    rng = np.random.default_rng(5)
    s, t, lf = 256 + 128 * 4 + 60, 33, 8
    needle = rng.uniform(-0.5, 0.5, s).astype(np.float32)
    hay = rng.uniform(-0.25, 0.25, t + s + 20).astype(np.float32)
    hay[t:t + s] += np.float32(0.5) * needle
    x = rng.normal(size=256)
    a, b = np.fft.rfft(x), ref.dft_direct(x)
    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    for edges in ([1, 2, 4, 8, 16, 32, 64, 129], [0, 16, 32, 64, 129], [0, 129]):
        fast = ref.bands_ref(hay, needle, t, lf, edges)
        slow = ref.bands_ref(hay, needle, t, lf, edges, transform=ref.dft_direct)
        for q, e in zip(fast, slow):
            assert q.flags == e.flags == 0
            for name in ref.FIELDS:
                assert abs(getattr(q, name) - getattr(e, name)) <= 1e-12 * max(1.0, abs(getattr(e, name))), (name, q, e)
    whole = ref.bands_ref(hay, needle, t, lf, [0, 129])[0]
    assert whole.needle_share == 1.0 and 0.6 < whole.ncc <= whole.coherence <= 1.0 and abs(whole.gain - 0.5) < 0.1


def test_checker_flags():
    rng = np.random.default_rng(6)
    s, lf, edges = 256 + 128 * 2 + 100, 8, [0, 16, 129]
    needle = rng.uniform(-0.5, 0.5, s).astype(np.float32)
    hay = rng.uniform(-0.25, 0.25, s + 50).astype(np.float32)
    assert ref.frame_count(s, lf) == 3 and ref.span(s, lf) == 512
    bad = hay.copy()
    bad[10 + 511] = np.nan
    assert all(q.flags == ref.NONFIN and np.isnan(q.ncc) for q in ref.bands_ref(bad, needle, 10, lf, edges))
    bad = hay.copy()
    bad[10 + 512] = np.nan                                    # the first unread sample
    assert all(q.flags == 0 for q in ref.bands_ref(bad, needle, 10, lf, edges))
    silent = np.zeros_like(hay)
    assert all(q.flags == ref.BELOW and q.level_db == -np.inf and q.gain == 0 for q in ref.bands_ref(silent, needle, 0, lf, edges))
    tone = np.cos(2 * np.pi * 4 * np.arange(s) / 256).astype(np.float32)
    got = ref.bands_ref(hay, tone, 0, lf, edges)
    assert got[0].flags == 0 and got[1].flags == ref.EMPTY and got[1].level_db == np.inf and got[1].needle_share < 1e-12


# ---- header and binding -------------------------------------------------------------------------------------------------
def test_header_declares_band_scoring():
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    for struct in ("am_band_params", "am_hit_band", "am_band_summary"):
        assert "typedef struct %s {" % struct in h and "} %s;" % struct in h, struct
    assert "AM_HIT_EMPTY_BAND = 128" in h
    assert re.search(r"#define AM_BAND_MAX_BANDS\s+32\b", h) and re.search(r"#define AM_BAND_EMPTY_DB\s+90\b", h)
    assert h.index("per-segment hit scoring") < h.index("per-band hit scoring") < h.index("streaming ingest")
    doc = h[h.index("per-band hit scoring"):h.index("enum { AM_HIT_EMPTY_BAND")]
    for word in ("AM_HIT_EMPTY_BAND", "AM_HIT_NONFINITE", "AM_HIT_BELOW_FLOOR", "coherence", "needle_share", "bit for bit",
                 "tools/hit_bands_bench.py"):
        assert word in doc, word
    assert "#define AM_ABI_VERSION 3" in h
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for fn in FUNCS:
        assert fn in hpp or fn.endswith("_batch_device"), fn   # (the C++ mirror wraps the per-needle forms, as for segments)
        assert "pub fn " + fn + "(" in rs, fn


LAYOUT_PROBE = r'''
#include <cstddef>
#include <cstdio>
#include "audiomatch.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(am_hit_band), offsetof(am_hit_band, ncc),
                offsetof(am_hit_band, coherence), offsetof(am_hit_band, gain), offsetof(am_hit_band, level_db),
                offsetof(am_hit_band, needle_share), offsetof(am_hit_band, flags), AM_HIT_EMPTY_BAND, AM_BAND_MAX_BANDS, AM_BAND_EMPTY_DB);
    std::printf("%zu %zu %zu %zu\n", sizeof(am_band_params), offsetof(am_band_params, frame_log2), offsetof(am_band_params, n_bands),
                offsetof(am_band_params, edges));
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(am_band_summary), offsetof(am_band_summary, coverage),
                offsetof(am_band_summary, weighted_coherence), offsetof(am_band_summary, gain_db_spread),
                offsetof(am_band_summary, first_present), offsetof(am_band_summary, last_present),
                offsetof(am_band_summary, n_present), offsetof(am_band_summary, n_countable));
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
    R, P, S = am.HitBand, am.AmBandParams, am.AmBandSummary
    assert C.sizeof(R) == 24
    assert rows[0] == [C.sizeof(R), R.ncc.offset, R.coherence.offset, R.gain.offset, R.level_db.offset, R.needle_share.offset,
                       R.flags.offset, am.AM_HIT_EMPTY_BAND, am.AM_BAND_MAX_BANDS, am.AM_BAND_EMPTY_DB]
    assert rows[1] == [C.sizeof(P), P.frame_log2.offset, P.n_bands.offset, P.edges.offset]
    assert rows[2] == [C.sizeof(S), S.coverage.offset, S.weighted_coherence.offset, S.gain_db_spread.offset,
                       S.first_present.offset, S.last_present.offset, S.n_present.offset, S.n_countable.offset]
    assert set(FUNCS) <= set(am.declared_symbols())
    assert (ref.BELOW, ref.NONFIN, ref.EMPTY) == (am.AM_HIT_BELOW_FLOOR, am.AM_HIT_NONFINITE, am.AM_HIT_EMPTY_BAND)


# ---- the CLI's parser ---------------------------------------------------------------------------------------------------
PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("bands=%u log2f=%u\n", a.bands, a.band_frame_log2);
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_bands(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "bands=0 log2f=11\n")
    assert run("a.wav", "--snippet", "s.wav", "--bands", "8") == (0, "bands=8 log2f=11\n")
    assert run("a.wav", "--snippet", "s.wav", "--bands", "8:10") == (0, "bands=8 log2f=10\n")
    assert run("a.wav", "--snippet", "s.wav", "--bands", "32:12") == (0, "bands=32 log2f=12\n")
    assert run("a.wav", "--snippet", "s.wav", "--bands", "1:8", "--segments", "4") == (0, "bands=1 log2f=8\n")
    for bad in ("0", "33", "8:7", "8:13", "8:", ":10", "-3", "x", "", "8:10:1", "8.5"):
        code, out = run("a.wav", "--snippet", "s.wav", "--bands", bad)
        assert code == 2 and "--bands" in out, (bad, out)
    code, out = run("a.wav", "--snippet", "s.wav", "--bands")
    assert code == 2 and "--bands" in out
    code, out = run("--snippet", "s.wav", "--live", "--rate", "8000", "--bands", "8")
    assert code == 2 and "--live" in out and "--bands" in out
    code, out = run("--help")
    assert code == 0 and "--bands B[:LOG2F]" in out and "--segments M[:R]" in out


# ---- am_hit_bands_summary -----------------------------------------------------------------------------------------------
def records(am, rows):
    return [am.HitBand(0.8 * coh, coh, gain, -6.0, share, flags) for coh, gain, share, flags in rows]


def check_summary(am, rows, min_coherence=0.5):
    recs = records(am, rows)
    got = am.hit_bands_summary(recs, min_coherence)
    exp = ref.summary_ref(recs, min_coherence)
    for k in ("first_present", "last_present", "n_present", "n_countable"):
        assert getattr(got, k) == exp[k], (k, got, exp)
    for k in ("coverage", "weighted_coherence", "gain_db_spread"):
        g, e = getattr(got, k), exp[k]
        assert (np.isnan(g) and np.isnan(e)) or abs(g - e) <= 1e-12 * max(1.0, abs(e)), (k, got, exp)
    return got


def test_summary_all_present(amlib):
    rows = [(0.9, 0.5, 0.125, 0)] * 8
    got = check_summary(amlib, rows)
    assert (got.coverage, got.first_present, got.last_present, got.n_present, got.n_countable) == (1.0, 0, 7, 8, 8)
    assert abs(got.weighted_coherence - np.float32(0.9)) < 1e-12 and got.gain_db_spread == 0.0


def test_summary_low_passed_copy(amlib):
    rows = [(0.9, 0.5, 0.25, 0), (0.89, 0.25, 0.25, 0), (0.88, 0.48, 0.25, 0), (0.06, 0.01, 0.125, 0), (0.01, 0.0, 0.125, 0)]
    got = check_summary(amlib, rows)
    assert (got.first_present, got.last_present, got.n_present, got.n_countable) == (0, 2, 3, 5)
    assert abs(got.coverage - 0.75) < 1e-12 and abs(got.gain_db_spread - 20 * np.log10(2.0)) < 1e-9
    assert check_summary(amlib, rows, 0.05).n_present == 4


def test_summary_skips_flagged_bands(amlib):
    nan = float("nan")
    rows = [(nan, nan, nan, ref.NONFIN), (0.0, 0.0, 1e-12, ref.EMPTY), (0.9, 0.7, 0.5, 0), (0.0, 0.3, 0.25, ref.BELOW),
            (0.95, -0.2, 0.125, 0), (0.4, 0.6, 0.125, 0)]
    got = check_summary(amlib, rows)
    assert (got.n_countable, got.n_present, got.first_present, got.last_present) == (4, 2, 2, 4)
    assert abs(got.coverage - 0.625) < 1e-12
    assert np.isnan(got.gain_db_spread)                      # one present band with a positive gain only
    # a NaN coherence without a flag is not present; no countable band: NaN
    assert amlib.hit_bands_summary(records(amlib, [(nan, 0.5, 0.5, 0), (0.6, 0.5, 0.5, 0)]), 0.5).n_present == 1
    none = check_summary(amlib, [(0.0, 0.0, 0.0, ref.EMPTY)] * 3)
    assert (none.n_countable, none.n_present, none.first_present, none.last_present) == (0, 0, -1, -1)
    assert np.isnan(none.coverage) and np.isnan(none.weighted_coherence)


def test_summary_errors(amlib):
    L = amlib.lib()
    out = amlib.AmBandSummary()
    buf = (amlib.HitBand * 40)()
    for args in ((None, 4, 0.5, C.byref(out)), (buf, 4, 0.5, None), (buf, 0, 0.5, C.byref(out)), (buf, 33, 0.5, C.byref(out))):
        assert L.am_hit_bands_summary(*args) == amlib.AM_ERR_INVALID_ARG
    with pytest.raises(amlib.AudioMatchError):
        amlib.hit_bands_summary([])


# ---- am_band_edges_log --------------------------------------------------------------------------------------------------
def test_edges_log(amlib):
    cases = [(8000, 11, 50.0, 4000.0, 8), (44100, 11, 50.0, 16000.0, 16), (44100, 12, 50.0, 16000.0, 32), (8000, 8, 50.0, 4000.0, 8),
             (8000, 8, 10.0, 4000.0, 32), (48000, 10, 20.0, 24000.0, 1), (8000, 8, 3000.0, 4000.0, 32), (8000, 8, 1.0, 2.0, 5),
             (8000, 9, 62.5, 4000.0, 6)]
    for sr, lf, lo, hi, nb in cases:
        exp = ref.edges_log_ref(sr, lf, lo, hi, nb)
        assert exp is not None, (sr, lf, lo, hi, nb)
        bp = amlib.band_edges_log(sr, lf, lo, hi, nb)
        assert (bp.frame_log2, bp.n_bands) == (lf, nb)
        assert list(bp.edges[:nb + 1]) == exp, (sr, lf, lo, hi, nb)
        assert all(e == 0 for e in bp.edges[nb + 1:])
        assert all(exp[b] < exp[b + 1] for b in range(nb)) and exp[nb] <= (1 << lf) // 2 + 1
    assert list(amlib.band_edges_log(8000, 11, 50.0, 4000.0, 8).edges[:9]) == [13, 22, 38, 66, 114, 198, 342, 592, 1024]
    assert list(amlib.band_edges_log(8000, 8, 1.0, 2.0, 5).edges[:6]) == [0, 1, 2, 3, 4, 5]   # raised to the predecessor + 1


def test_edges_log_errors(amlib):
    L = amlib.lib()
    out = amlib.AmBandParams()
    bad = [(8000, 11, 0.0, 4000.0, 8), (8000, 11, -1.0, 4000.0, 8), (8000, 11, 500.0, 500.0, 8), (8000, 11, 500.0, 100.0, 8),
           (8000, 11, 50.0, 4000.5, 8), (8000, 7, 50.0, 4000.0, 8), (8000, 13, 50.0, 4000.0, 8), (8000, 11, 50.0, 4000.0, 0),
           (8000, 11, 50.0, 4000.0, 33), (0, 11, 50.0, 4000.0, 8), (8000, 8, 3900.0, 4000.0, 32), (8000, 11, float("nan"), 4000.0, 8)]
    for sr, lf, lo, hi, nb in bad:
        assert ref.edges_log_ref(sr, lf, lo, hi, nb) is None, (sr, lf, lo, hi, nb)
        assert L.am_band_edges_log(sr, lf, lo, hi, nb, C.byref(out)) == amlib.AM_ERR_INVALID_ARG, (sr, lf, lo, hi, nb)
    assert L.am_band_edges_log(8000, 11, 50.0, 4000.0, 8, None) == amlib.AM_ERR_INVALID_ARG
    with pytest.raises(amlib.AudioMatchError):
        amlib.band_edges_log(8000, 11, 50.0, 5000.0, 8)
