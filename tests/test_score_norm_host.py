"""Host-side checks of the score_norm option (no device): the header's contract and the CLI's flags."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_header_documents_score_norm():
    h = open(os.path.join(ROOT, "include", "audiomatch.h")).read()
    assert '"score_norm"' in h and '"score_norm_floor_db"' in h
    assert "score_norm: not supported by this entry point" in h
    for ep in ("am_match_multi*", "am_pool_match_multi*", "am_match_stream_*", "am_match_part_device", "am_pool_match_long*"):
        assert ep in h, ep
    assert "AM_SCALE_LIB" in h and "#define AM_ABI_VERSION 3" in h
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    assert 'kOptScoreNorm = "score_norm"' in hpp and 'kOptScoreNormFloorDb = "score_norm_floor_db"' in hpp


def test_binding_exposes_option_keys():
    import audiomatch_amd as am
    assert am.OPT_SCORE_NORM == "score_norm" and am.OPT_SCORE_NORM_FLOOR_DB == "score_norm_floor_db"


PROBE = r'''
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", usage_text()); return 0; }
        std::printf("normalize=%d floor=%d\n", a.normalize ? 1 : 0, a.normalize_floor_db ? *a.normalize_floor_db : -1);
        return 0;
    } catch (const ArgError& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_normalize_flags(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "normalize=0 floor=-1\n")
    assert run("a.wav", "--snippet", "s.wav", "--normalize") == (0, "normalize=1 floor=-1\n")
    assert run("a.wav", "--snippet", "s.wav", "--normalize", "--normalize-floor", "80") == (0, "normalize=1 floor=80\n")
    for bad in ("abc", "-1", "201", "12dB", ""):
        code, out = run("a.wav", "--snippet", "s.wav", "--normalize-floor", bad)
        assert code == 2 and "--normalize-floor" in out, (bad, out)
    code, out = run("--help")
    assert code == 0 and "--normalize " in out and "--normalize-floor DB" in out
