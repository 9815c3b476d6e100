"""Host-side checks of per-hit scoring (no device): the header's declarations, the ctypes record's layout and the
CLI's --min-confidence flag."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")


def test_header_declares_hit_scoring():
    h = open(HEADER).read()
    for fn in ("am_hit_scores_device", "am_hit_scores", "am_hit_scores_batch_device"):
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "typedef struct am_hit_score {" in h and "} am_hit_score;" in h
    for flag in ("AM_HIT_UNREFINED", "AM_HIT_BELOW_FLOOR", "AM_HIT_NONFINITE"):
        assert flag in h, flag
    assert "#define AM_ABI_VERSION 3" in h


LAYOUT_PROBE = r'''
#include <cstddef>
#include <cstdio>
#include "audiomatch.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(am_hit_score), offsetof(am_hit_score, position),
                offsetof(am_hit_score, ncc), offsetof(am_hit_score, gain), offsetof(am_hit_score, window_db),
                offsetof(am_hit_score, flags), AM_HIT_UNREFINED, AM_HIT_BELOW_FLOOR, AM_HIT_NONFINITE);
    return 0;
}
'''


def test_ctypes_record_matches_header(tmp_path):
    import audiomatch_amd as am
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROBE)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    R = am.AmHitScore
    assert C.sizeof(R) == 24
    assert got == [C.sizeof(R), R.position.offset, R.ncc.offset, R.gain.offset, R.window_db.offset, R.flags.offset,
                   am.AM_HIT_UNREFINED, am.AM_HIT_BELOW_FLOOR, am.AM_HIT_NONFINITE]
    assert {"am_hit_scores", "am_hit_scores_device", "am_hit_scores_batch_device"} <= set(am.declared_symbols())


PARSER_PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        if (a.min_confidence) std::printf("min_confidence=%g\n", (double)*a.min_confidence);
        else std::printf("min_confidence=none\n");
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_min_confidence(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "min_confidence=none\n")
    assert run("a.wav", "--snippet", "s.wav", "--min-confidence", "0.5") == (0, "min_confidence=0.5\n")
    assert run("a.wav", "--snippet", "s.wav", "--min-confidence", "0") == (0, "min_confidence=0\n")
    assert run("a.wav", "--snippet", "s.wav", "--min-confidence", "1") == (0, "min_confidence=1\n")
    for bad in ("-0.1", "1.5", "abc", "", "nan", "0.5x"):
        code, out = run("a.wav", "--snippet", "s.wav", "--min-confidence", bad)
        assert code == 2 and "--min-confidence" in out, (bad, out)
    code, out = run("a.wav", "--snippet", "s.wav", "--min-confidence")
    assert code == 2 and "--min-confidence" in out
    code, out = run("--help")
    assert code == 0 and "--min-confidence X" in out
