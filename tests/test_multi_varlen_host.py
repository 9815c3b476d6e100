"""Host-side checks of the several-needles-of-any-length entry points (no device): the header declares and documents
them, the binding exposes them, the library exports them, and the CLI parser takes --snippet several times."""
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("am_match_multi_varlen_batch_device", "am_match_multi_varlen")


def test_header_declares_and_documents_varlen():
    h = open(os.path.join(ROOT, "include", "audiomatch.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", h), name
    assert "const uint64_t* overlaps" in h and "overlaps == NULL means p->overlap" in h
    # the list of entry points that refuse score_norm names them
    refusal = h[h.index('"score_norm: not supported by this entry point" -- by'):]
    refusal = refusal[:refusal.index(".")]
    for name in NAMES:
        assert name in refusal
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    assert "am_match_multi_varlen_batch_device(" in hpp and "am_match_multi_varlen(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn am_match_multi_varlen_batch_device(" in rs and "pub fn am_match_multi_varlen(" in rs
    assert "pub fn calc_chunks_multi(" in rs


def test_binding_and_library_expose_varlen(amlib):
    for name in NAMES:
        assert name in amlib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(NAMES) <= exported
    assert callable(amlib.match_multi_varlen_batch_device) and callable(amlib.match_multi_varlen)


PARSER_PROBE = r'''
#include "am_host.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    try {
        const amhost::Arguments a = amhost::parse_arguments(argc, argv);
        if (a.help) { std::printf("%s", amhost::usage_text()); return 0; }
        std::printf("snippet=%s n=%zu", a.snippet.c_str(), a.snippets.size());
        for (const auto& s : a.snippets) std::printf(" %s", s.c_str());
        std::printf("\n");
        return 0;
    } catch (const amhost::ArgError& e) {
        std::printf("%s\n", e.what());
        return 2;
    }
}
'''


def test_cli_parser_repeated_snippet(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PARSER_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(src)])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run("a.wav", "--snippet", "s.wav") == (0, "snippet=s.wav n=1 s.wav\n")
    assert run("a.wav", "--snippet", "s.wav", "--snippet", "t.wav", "--snippet", "u.wav") == (0, "snippet=s.wav n=3 s.wav t.wav u.wav\n")
    code, out = run("a.wav")
    assert code == 2 and "--snippet <FILE> is required" in out
    code, out = run("--help")
    assert code == 0 and "[--snippet <FILE>]..." in out and re.search(r"^  --snippet FILE {2,}\S", out, re.M), out
