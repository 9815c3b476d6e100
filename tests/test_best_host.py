"""CPU tests of the k best matches (include/audiomatch.h, "the k best matches"): the header declares and documents the
five calls and am_best_params, the binding declares and the library exports them, the ABI version stays 3, the C++
mirror and the CLI know them.  No device is needed."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
CALLS = ["am_match_best", "am_match_best_device", "am_match_best_batch_device", "am_find_peaks_top",
         "am_find_peaks_top_device"]


def header_text():
    return open(HEADER).read()


def test_header_declares_and_documents_the_calls():
    txt = header_text()
    sec = txt[txt.index("---- the k best matches"):]
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, sec), name
    m = re.search(r"typedef struct am_best_params \{(.*?)\} am_best_params;", sec, re.S)
    assert m, "am_best_params"
    fields = re.findall(r"\b(uint64_t|float|int)\s+(\w+);", m.group(1))
    assert fields == [("uint64_t", "k"), ("uint64_t", "min_distance"), ("float", "min_prominence"), ("int", "scale")]
    for word in ("am_find_peaks[:k]", "bit for bit", "peak_filter_order", "distance_rule", "AM_SCALE_MY", "k == 0",
                 "AM_MODE_VALID", "AM_FMT_S16_STEREO", "non-finite"):
        assert word in sec, word
    assert "AM_ABI_VERSION 3" in re.sub(r"\s+", " ", txt)


def test_score_norm_paragraph_names_the_new_entry_points():
    txt = re.sub(r"\s+", " ", re.sub(r"\n\s*\* ?", " ", header_text()))
    sup = txt[txt.index("Supported by am_correlate*"):txt.index("NOT supported")]
    for name in ("am_match_best,", "am_match_best_device", "am_match_best_batch_device"):
        assert name in sup, name


def test_binding_declares_and_library_exports(amlib):
    assert set(CALLS) <= set(amlib.declared_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(CALLS) <= exported
    assert amlib.lib().am_abi_version() == 3
    assert C.sizeof(amlib.AmBestParams) == 24
    bp = amlib.best_params(3, 100, 0.25, amlib.Scale.NONE)
    assert (bp.k, bp.min_distance, bp.min_prominence, bp.scale) == (3, 100, 0.25, 0)


def test_refusals_need_no_device(amlib):
    """k == 0 and null pointers are refused before any device is touched."""
    n = C.c_size_t(7)
    out = (amlib.AmPeak * 1)()
    assert amlib.lib().am_find_peaks_top(0, None, 10, 0.0, 0, 1, out, C.byref(n)) == 1
    x = (C.c_float * 10)()
    assert amlib.lib().am_find_peaks_top(0, x, 10, 0.0, 0, 0, out, C.byref(n)) == 1
    assert amlib.lib().am_find_peaks_top_device(0, x, 10, 0.0, 0, 1, None, C.byref(n)) == 1
    assert amlib.lib().am_match_best(None, x, 10, 0, None, out, C.byref(n)) == 1


def test_cpp_mirror_and_cli_know_best():
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    for name in ("am_match_best(", "am_match_best_device(", "am_match_best_batch_device(", "am_find_peaks_top(",
                 "am_find_peaks_top_device("):
        assert name in hpp, name
    host = open(os.path.join(ROOT, "audio-matcher_amd", "host", "am_host.hpp")).read()
    assert '"--best"' in host and "am_match_best" in host


def test_cli_parses_best(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
    import build as am_build
    cli = am_build.build_cli()
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--best N" in out.stdout + out.stderr
    for bad in ("0", "-2", "x"):
        out = subprocess.run([cli, "a.wav", "--snippet", "b.wav", "--best", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "--best" in out.stderr, bad
