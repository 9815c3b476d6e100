"""Host-side checks of per-hit significance (no device): the header's declarations and their place, the ctypes records'
layout, the CLI's --min-significance / --significance-zone flags, the refusals that need no device, and the checker
(tests/hit_significance_ref.py) on hand-made score arrays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import hit_significance_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_significance_device", "am_hit_significance", "am_hit_significance_batch_device")


def test_header_declares_significance():
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    for struct in ("am_significance_params", "am_significance"):
        assert "typedef struct %s {" % struct in h and "} %s;" % struct in h, struct
    assert "AM_HIT_NO_BACKGROUND = 16, AM_HIT_FLAT_BACKGROUND = 32, AM_HIT_CLIPPED = 64" in h
    assert re.search(r"#define AM_SIG_MAX_RADIUS\s+\(1u << 22\)", h)
    first = h.index("int am_hit_significance_device(")
    assert h.index("---- per-segment hit scoring") < h.index("---- per-hit significance") < first < h.index("---- streaming ingest")
    assert h.index("int am_hit_segments_summary(") < first
    assert "#define AM_ABI_VERSION 3" in h
    # the definition is the contract: the header spells out the tie rule, the two-pass deviation and every flag's result
    doc = h[h.index("---- per-hit significance"):first]
    for text in ("AM_MODE_VALID", "AM_SCALE_LIB", "|u - t| > G", "two passes", "smaller |u - t|", "negative lag", "AM_HIT_NONFINITE",
                 "AM_HIT_NO_BACKGROUND", "AM_HIT_FLAT_BACKGROUND", "AM_HIT_CLIPPED", "bit for bit", "guard >= radius"):
        assert text in doc, text
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    assert "hit_significance(" in hpp and "hit_significance_device(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for fn in FUNCS:
        assert "pub fn %s(" % fn in rs, fn


LAYOUT_PROBE = r'''
#include <cstddef>
#include <cstdio>
#include "audiomatch.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(am_significance), offsetof(am_significance, score),
                offsetof(am_significance, bg_mean), offsetof(am_significance, bg_std), offsetof(am_significance, z),
                offsetof(am_significance, side_max), offsetof(am_significance, side_lag), offsetof(am_significance, n_bg),
                offsetof(am_significance, flags));
    std::printf("%zu %zu %zu\n", sizeof(am_significance_params), offsetof(am_significance_params, guard),
                offsetof(am_significance_params, radius));
    std::printf("%d %d %d %u\n", AM_HIT_NO_BACKGROUND, AM_HIT_FLAT_BACKGROUND, AM_HIT_CLIPPED, AM_SIG_MAX_RADIUS);
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
    R, P = am.HitSignificance, am.AmSignificanceParams
    assert C.sizeof(R) == 32 and C.sizeof(P) == 16
    assert rows[0] == [C.sizeof(R), R.score.offset, R.bg_mean.offset, R.bg_std.offset, R.z.offset, R.side_max.offset,
                       R.side_lag.offset, R.n_bg.offset, R.flags.offset] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert rows[1] == [C.sizeof(P), P.guard.offset, P.radius.offset] == [16, 0, 8]
    assert rows[2] == [am.AM_HIT_NO_BACKGROUND, am.AM_HIT_FLAT_BACKGROUND, am.AM_HIT_CLIPPED, am.AM_SIG_MAX_RADIUS] == [16, 32, 64, 1 << 22]
    assert (ref.NO_BG, ref.FLAT, ref.CLIPPED, ref.NONFIN) == (16, 32, 64, am.AM_HIT_NONFINITE)
    assert set(FUNCS) <= set(am.declared_symbols())
    q = R(1.0, 2.0, 3.0, 4.0, 5.0, -6, 7, 8)
    assert q.pack() == ref.pack(q) and len(q.pack()) == 32


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("z=%g zone=%lld\n", a.min_significance ? (double)*a.min_significance : -1.0,
                    a.significance_zone_ms ? (long long)*a.significance_zone_ms : -1ll);
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_significance(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "z=-1 zone=-1\n")
    assert run("a.wav", "--snippet", "s.wav", "--min-significance", "50") == (0, "z=50 zone=-1\n")
    assert run("a.wav", "--snippet", "s.wav", "--min-significance", "7.5", "--significance-zone", "30s") == (0, "z=7.5 zone=30000\n")
    assert run("a.wav", "--snippet", "s.wav", "--snippet", "t.wav", "--best", "3", "--min-significance", "0") == (0, "z=0 zone=-1\n")
    for bad in ("abc", "", "5x", "nan", "inf"):
        code, out = run("a.wav", "--snippet", "s.wav", "--min-significance", bad)
        assert code == 2 and "--min-significance" in out, (bad, out)
    for bad in ("0", "0s", "x", ""):
        code, out = run("a.wav", "--snippet", "s.wav", "--significance-zone", bad)
        assert code == 2 and "--significance-zone" in out, (bad, out)
    code, out = run("a.wav", "--snippet", "s.wav", "--min-significance")
    assert code == 2 and "--min-significance" in out
    code, out = run("--snippet", "s.wav", "--live", "--rate", "8000", "--min-significance", "5")
    assert code == 2 and "--live" in out and "--min-significance" in out
    code, out = run("--help")
    assert code == 0 and "--min-significance Z" in out and "--significance-zone D" in out
    live = out[out.index("  --live "):out.index("  --rate R")]
    assert "--min-significance" in live


def _rc(am, fn, *args):
    rc = fn(*args)
    msg = am.lib().am_last_error_string()
    return rc, (msg.decode() if msg else "")


def test_refusals_without_a_device(amlib):
    am, L = amlib, amlib.lib()
    INV = am.AM_ERR_INVALID_ARG
    pk = (am.AmPeak * 1)(am.AmPeak(0, 1, 0, 0))
    out = (am.HitSignificance * 1)()
    sp = am.AmSignificanceParams(4, 9)
    x = np.zeros(16, dtype=np.float32)
    for fn in (L.am_hit_significance, L.am_hit_significance_device):
        rc, msg = _rc(am, fn, None, x.ctypes.data, 16, 0, pk, 1, C.byref(sp), out)
        assert rc == INV and "null needle handle" in msg, msg
    none1, lens, cnt = (C.c_void_p * 1)(None), (C.c_size_t * 1)(16), (C.c_size_t * 1)(1)

    def batch(fmt, peaks, counts, spp, dst, n_needles=1, n_hay=1):
        return _rc(am, L.am_hit_significance_batch_device, none1, n_needles, none1, lens, n_hay, fmt, peaks, 1, counts, spp, dst)

    rc, msg = batch(5, pk, cnt, C.byref(sp), out)
    assert rc == INV and "format" in msg, msg
    assert batch(0, pk, cnt, C.byref(sp), out, n_needles=0)[0] == am.AM_OK           # nothing to do
    assert batch(0, pk, cnt, C.byref(sp), out, n_hay=0)[0] == am.AM_OK
    assert batch(0, None, (C.c_size_t * 1)(0), None, None)[0] == am.AM_OK            # no hits: nothing is read
    for args in ((None, cnt, C.byref(sp), out), (pk, cnt, None, out), (pk, cnt, C.byref(sp), None), (pk, None, C.byref(sp), out)):
        rc, msg = batch(0, *args)
        assert rc == INV and "null pointer" in msg, msg
    for bad, text in ((am.AmSignificanceParams(9, 9), "guard 9 >= radius 9"), (am.AmSignificanceParams(10, 2), "guard 10 >= radius 2"),
                      (am.AmSignificanceParams(0, (1 << 22) + 1), "AM_SIG_MAX_RADIUS")):
        rc, msg = batch(0, pk, cnt, C.byref(bad), out)
        assert rc == INV and text in msg, msg
    rc, msg = batch(0, pk, cnt, C.byref(sp), out)
    assert rc == INV and "needle 0: null needle handle" in msg, msg
    assert ref.pack(out[0]) == bytes(32)      # no refusal wrote a record


# ---- the checker on hand-made score arrays --------------------------------------------------------------------------
def test_checker_statistics():
    r = np.array([1, 2, 3, 100, 50, 9, 5, 6, 7], dtype=np.float32)
    q = ref.significance_ref(r, 4, 1)                    # background: indices 0 1 2 and 6 7 8
    assert (q["score"], q["n_bg"], q["flags"]) == (50.0, 6, 0)
    assert q["bg_mean"] == 4.0 and q["side_max"] == 7.0 and q["side_lag"] == 4
    assert abs(q["bg_std"] - np.sqrt(28 / 6)) < 1e-6 and abs(q["z"] - 46 / np.sqrt(28 / 6)) < 1e-5
    q = ref.significance_ref(r, 4, 0)                    # G = 0: the neighbours count, 100 at lag -1 is the largest
    assert (q["n_bg"], q["side_max"], q["side_lag"]) == (8, 100.0, -1)
    # two passes, not E[r^2] - mean^2: a large common offset leaves the deviation exact
    big = (np.array([0, 1, 0, 9, 0, 1, 0], dtype=np.float32) + np.float32(4096)).astype(np.float32)
    q = ref.significance_ref(big, 3, 0)
    assert abs(q["_mean64"] - (4096 + 1 / 3)) < 1e-9 and abs(q["_std64"] - np.sqrt(2 / 9)) < 1e-9


def test_checker_tie_rule():
    r = np.zeros(21, dtype=np.float32)
    q = ref.significance_ref(r, 10, 3)                   # all equal: the smallest |lag| beyond the guard, negative first
    assert (q["side_lag"], q["flags"], q["z"], q["bg_std"]) == (-4, ref.FLAT, 0.0, 0.0)
    q = ref.significance_ref(r, 0, 3, clipped=True)      # nothing on the negative side
    assert (q["side_lag"], q["flags"]) == (4, ref.FLAT | ref.CLIPPED)
    r[[2, 16, 18]] = 5.0                                 # lags -8, +6, +8: the smaller |lag| wins over the sign
    assert ref.significance_ref(r, 10, 3)["side_lag"] == 6
    r[4] = 5.0                                           # lag -6 ties with +6: the negative lag
    assert ref.significance_ref(r, 10, 3)["side_lag"] == -6
    r[11] = 9.0                                          # inside the guard: not background
    q = ref.significance_ref(r, 10, 3)
    assert (q["side_max"], q["side_lag"]) == (5.0, -6)
    r[14] = 9.0                                          # at lag +4 it is
    q = ref.significance_ref(r, 10, 3)
    assert (q["side_max"], q["side_lag"]) == (9.0, 4)


def test_checker_flags():
    r = np.arange(9, dtype=np.float32)
    q = ref.significance_ref(r, 4, 3)                    # n_bg = 2: enough
    assert (q["n_bg"], q["flags"], q["bg_mean"], q["bg_std"]) == (2, 0, 4.0, 4.0)
    q = ref.significance_ref(r[:8], 4, 3, clipped=True)  # n_bg = 1
    assert (q["n_bg"], q["flags"], q["side_lag"], q["score"]) == (1, ref.NO_BG | ref.CLIPPED, 0, 4.0)
    assert all(np.isnan(q[k]) for k in ("bg_mean", "bg_std", "z", "side_max"))
    q = ref.significance_ref(r[4:5], 0, 0, clipped=True)
    assert (q["n_bg"], q["flags"], q["score"]) == (0, ref.NO_BG | ref.CLIPPED, 4.0)
    flat = np.array([2, 2, 7, 2, 2], dtype=np.float32)
    assert (ref.significance_ref(flat, 2, 0)["z"], ref.significance_ref(flat, 2, 0)["flags"]) == (float("inf"), ref.FLAT)
    flat[2] = -1
    assert ref.significance_ref(flat, 2, 0)["z"] == float("-inf")
    q = ref.significance_ref(r, 4, 1, clipped=True, nonfinite=True)
    assert (q["flags"], q["n_bg"], q["side_lag"]) == (ref.NONFIN | ref.CLIPPED, 6, 0)
    assert all(np.isnan(q[k]) for k in ("score", "bg_mean", "bg_std", "z", "side_max"))


def test_checker_zone():
    assert ref.zone(100, 10, 1000, 50) == (50, 150, False)
    assert ref.zone(50, 10, 1000, 50) == (0, 100, False)
    assert ref.zone(49, 10, 1000, 50) == (0, 99, True)
    assert ref.zone(940, 10, 1000, 50) == (890, 990, False)
    assert ref.zone(941, 10, 1000, 50) == (891, 990, True)
    assert ref.zone(0, 10, 10, 50) == (0, 0, True)
