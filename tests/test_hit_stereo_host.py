"""Host-side checks of the per-hit stereo image (no device): the header, the exports, the mirrors and the record sizes;
am_hit_stereo_summary on hand-made records, one per image class and per boundary of its rules; the checker
(tests/hit_stereo_ref.py) held to its own claims on the designed inputs of the GPU tests; mix_ref against the down-mix;
the CLI's parsing of --mix and --stereo."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hit_stereo_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "audiomatch.h")
FUNCS = ("am_hit_stereo", "am_hit_stereo_device", "am_hit_stereo_batch_device", "am_hit_stereo_summary", "am_pcm_s16_stereo_mix",
         "am_pcm_s16_stereo_mix_device")
SIZES = (1, 37, 4096, 4097, 5000, 30_000)      # 4096 and 4097: the slice edge and one past it
RADII = (0, 1, 4, 16)
FRAMES = 60_000
GAIN = 0.7


# ---- the designed inputs of tests/test_gpu_hit_stereo.py ---------------------------------------------------------------
def needle_of(s):
    return np.random.default_rng(900 + s).normal(0, 0.06, s).astype(np.float32)


def plant(lr, t, needle, left, right, delay=0):
    """Adds the needle at gain `left` to L at t and at gain `right` to R at t + delay, in i16 steps (l = k L)."""
    p = np.rint(needle.astype(np.float64) / ref.K).astype(np.int64)
    s = len(needle)
    lr[t:t + s, 0] += np.rint(left * p).astype(np.int64)
    hi = min(t + delay + s, len(lr))
    lr[t + delay:hi, 1] += np.rint(right * p[:hi - t - delay]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def designed(s):
    """(needle, frames [FRAMES, 2] i16, hits) for a needle of s samples: independent i16 noise of amplitude 3000 per channel
    and four plants at gain 0.7 -- both channels, left only, inverted in right, right delayed by 3 frames (they overlap for
    the longest needle).  Hits: t = 0 and t + S = len (their lags read outside the haystack, that is zeros), the four
    plants, one hit between plants, two beside the first plant (the best lag is not 0)."""
    rng = np.random.default_rng(1000 + s)
    needle = needle_of(s)
    lr = rng.integers(-3000, 3001, size=(FRAMES, 2)).astype(np.int64)
    at = [4 + j * ((FRAMES - s - 8) // 4) for j in range(1, 5)]
    plant(lr, at[0], needle, GAIN, GAIN)
    plant(lr, at[1], needle, GAIN, 0.0)
    plant(lr, at[2], needle, GAIN, -GAIN)
    plant(lr, at[3], needle, GAIN, GAIN, delay=3)
    assert np.abs(lr).max() <= 32767
    hits = [0, FRAMES - s] + at + [(at[0] + at[1]) // 2, at[0] + 2, at[0] - 1]
    lr = lr.astype(np.int16)
    lr.setflags(write=False)
    needle.setflags(write=False)
    return needle, lr, hits


@functools.lru_cache(maxsize=None)
def designed_refs(s, r):
    """The checker's records of designed(s) at radius r, computed once and shared."""
    needle, lr, hits = designed(s)
    return [ref.stereo_ref(lr, needle, t, r) for t in hits]


# ---- header, exports, mirrors ------------------------------------------------------------------------------------------
def test_header_declares_stereo_and_library_exports_it(amlib):
    h = open(HEADER).read()
    for fn in FUNCS:
        assert re.search(r"\bint " + fn + r"\(", h), fn
    assert "#define AM_ABI_VERSION 3" in h and amlib.lib().am_abi_version() == 3
    assert re.search(r"#define AM_STEREO_MAX_RADIUS\s+16\b", h) and amlib.AM_STEREO_MAX_RADIUS == 16 == ref.MAX_RADIUS
    assert re.search(r"#define AM_STEREO_MIN_INDEPENDENCE\s+1e-6\b", h) and amlib.AM_STEREO_MIN_INDEPENDENCE == ref.MIN_INDEPENDENCE
    for name, value in (("LEFT_SILENT", 1024), ("RIGHT_SILENT", 2048), ("SIDE_SILENT", 4096), ("COLLINEAR", 8192),
                        ("LEFT_UNREFINED", 16384), ("RIGHT_UNREFINED", 32768)):
        assert re.search(r"AM_HIT_%s = %d\b" % (name, value), h), name
        assert getattr(amlib, "AM_HIT_" + name) == value == getattr(ref, name)
    for i, name in enumerate(("ABSENT", "CENTRE", "LEFT", "RIGHT", "PANNED", "INVERTED")):
        assert re.search(r"AM_IMAGE_%s = %d\b" % (name, i), h) and getattr(amlib, "AM_IMAGE_" + name) == i == getattr(ref, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    assert set(FUNCS) <= exported and set(FUNCS) <= set(amlib.declared_symbols())
    assert C.sizeof(amlib.HitStereo) == 56 and C.sizeof(amlib.AmStereoParams) == 8 and C.sizeof(amlib.AmStereoSummary) == 32
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in FUNCS:
        assert "pub fn " + name + "(" in rs, name
    for name in ("am_hit_stereo", "am_hit_stereo_device", "am_hit_stereo_summary", "am_pcm_s16_stereo_mix"):
        assert name + "(" in hpp, name
    for field, _ in amlib.HitStereo._fields_:
        assert re.search(r"pub %s: (f64|f32|u32)," % field, rs), field


def test_struct_sizes_in_c(tmp_path):
    """sizeof(am_stereo_hit) == 56 and sizeof(am_stereo_params) == 8, as a C compiler sees the header."""
    src = tmp_path / "sizes.c"
    src.write_text('#include "audiomatch.h"\n_Static_assert(sizeof(am_stereo_hit) == 56, "record");\n'
                   '_Static_assert(sizeof(am_stereo_params) == 8, "params");\n'
                   '_Static_assert(sizeof(am_stereo_summary) == 32, "summary");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "sizes.o")])


# ---- am_hit_stereo_summary ---------------------------------------------------------------------------------------------
def record(amlib, ncc_left, ncc_right, ncc_mid, ncc_best, gain_left, gain_right, lag_left=0.0, lag_right=0.0):
    return amlib.HitStereo(lag_left, lag_right, float(ncc_left), float(ncc_right), float(ncc_mid), 0.0, float(ncc_best), float(gain_left),
                           float(gain_right), 0.0, 0.0, 0)


G3 = 10.0 ** (3.0 / 20.0)      # a gain ratio of 3 dB


@pytest.mark.parametrize("name,args,image", [
    ("absent", (0.3, 0.3, 0.4, 0.45, 1.0, 1.0), ref.ABSENT),
    ("best exactly at min_ncc is not absent", (0.5, 0.5, 0.5, 0.5, 1.0, 1.0), ref.CENTRE),
    ("best just under", (0.5, 0.5, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 1.0), ref.ABSENT),
    ("centre", (0.8, 0.8, 0.9, 0.9, 1.0, 1.0), ref.CENTRE),
    ("centre, both negative", (-0.8, -0.8, -0.9, 0.9, -1.0, -1.0), ref.CENTRE),
    ("left", (0.9, 0.1, 0.6, 0.9, 1.0, 0.1), ref.LEFT),
    ("left at exactly min_ncc, right just under", (0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.6, 0.9, 1.0, 1.0), ref.LEFT),
    ("left, negative", (-0.9, 0.1, 0.6, 0.9, -1.0, 0.1), ref.LEFT),
    ("right", (0.1, 0.9, 0.6, 0.9, 0.1, 1.0), ref.RIGHT),
    ("right, negative", (0.1, -0.9, -0.6, 0.9, 0.1, -1.0), ref.RIGHT),
    ("inverted, right negative", (0.8, -0.8, 0.0, 0.9, 1.0, -1.0), ref.INVERTED),
    ("inverted, left negative", (-0.8, 0.8, 0.0, 0.9, -1.0, 1.0), ref.INVERTED),
    ("inverted wins over the balance", (0.8, -0.6, 0.1, 0.9, 4.0, -1.0), ref.INVERTED),
    ("balance just inside 3 dB", (0.8, 0.8, 0.9, 0.9, 1.4125, 1.0), ref.CENTRE),
    ("balance just outside 3 dB", (0.8, 0.8, 0.9, 0.9, 1.4126, 1.0), ref.PANNED),
    ("balance just inside -3 dB", (0.8, 0.8, 0.9, 0.9, 1.0, 1.4125), ref.CENTRE),
    ("balance just outside -3 dB", (0.8, 0.8, 0.9, 0.9, 1.0, 1.4126), ref.PANNED),
    ("panned", (0.9, 0.6, 0.9, 0.95, 2.0, 1.0), ref.PANNED),
    ("neither channel alone, the mix does", (0.45, 0.45, 0.6, 0.6, 1.0, 1.0), ref.PANNED),
])
def test_summary_rules(amlib, name, args, image):
    q = record(amlib, *args, lag_left=1.25, lag_right=-0.5)
    got = amlib.hit_stereo_summary(q, 0.5)
    want = ref.summary_ref(q, 0.5)
    assert got.image == image == want[0], (name, got, want)
    # (two log10 implementations differ by an ulp or so: 1e-12 dB, or both the same infinity or both NaN)
    for g, w in ((got.balance_db, want[1]), (got.downmix_loss_db, want[3])):
        assert g == w or abs(g - w) <= 1e-12 or (np.isnan(g) and np.isnan(w)), (name, got, want)
    if abs(q.ncc_left) >= 0.5 and abs(q.ncc_right) >= 0.5:
        assert got.delay == 1.75, (name, got)
    else:
        assert np.isnan(got.delay), (name, got)


def test_summary_balance_at_exactly_3_db_and_the_infinities(amlib):
    """|balance_db| <= 3 includes 3: gains whose f32 ratio gives 20 log10 = 3 to the last bit or just under stay CENTRE;
    the rule is applied to the balance_db the summary returns."""
    for gl, gr in ((G3, 1.0), (1.0, G3), (-G3, -1.0)):
        q = record(amlib, 0.8 if gl > 0 else -0.8, 0.8 if gr > 0 else -0.8, 0.9, 0.9, gl, gr)
        got = amlib.hit_stereo_summary(q, 0.5)
        print(gl, gr, got)
        assert abs(abs(got.balance_db) - 3.0) < 1e-6
        assert got.image == (ref.CENTRE if abs(got.balance_db) <= 3.0 else ref.PANNED) == ref.summary_ref(q, 0.5)[0]
    # a balance_db of exactly 3.0 cannot be made from f32 gains for certain; the comparison itself is checked on the
    # two neighbours of 3 dB above (1.4125 and 1.4126) and here on the sign symmetry
    q = record(amlib, 0.9, 0.0, 0.6, 0.9, 1.0, 0.0)
    got = amlib.hit_stereo_summary(q, 0.5)
    assert got.balance_db == np.inf and got.image == ref.LEFT and np.isnan(got.delay)
    q = record(amlib, 0.0, 0.9, 0.6, 0.9, 0.0, 1.0)
    assert amlib.hit_stereo_summary(q, 0.5).balance_db == -np.inf
    q = record(amlib, 0.8, -0.8, 0.0, 0.9, 1.0, -1.0)
    got = amlib.hit_stereo_summary(q, 0.5)
    assert got.downmix_loss_db == np.inf and got.image == ref.INVERTED and got.delay == 0.0
    q = record(amlib, 0.8, 0.8, 0.45, 0.9, 1.0, 1.0)
    assert abs(amlib.hit_stereo_summary(q, 0.5).downmix_loss_db - 20 * np.log10(np.float64(np.float32(0.9)) / np.float64(np.float32(0.45)))) < 1e-12
    L = amlib.lib()
    out = amlib.AmStereoSummary()
    assert L.am_hit_stereo_summary(None, 0.5, C.byref(out)) == amlib.AM_ERR_INVALID_ARG and b"null" in L.am_last_error_string()
    assert L.am_hit_stereo_summary(C.byref(q), 0.5, None) == amlib.AM_ERR_INVALID_ARG


# ---- the checker against its own claims --------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SIZES)
def test_checker_on_the_designed_inputs(s):
    needle, lr, hits = designed(s)
    assert len(hits) == 9 and hits[0] == 0 and hits[1] + s == FRAMES and min(hits) >= 0 and max(hits) + s <= FRAMES
    for r in RADII:
        recs = designed_refs(s, r)
        for t, q in zip(hits, recs):
            who = (s, r, t)
            # the margins exclude no case: every hit's best lag is decided
            assert q.margin_left > 1e-9 and q.margin_right > 1e-9, who
            assert not q.flags & (ref.NONFIN | ref.EMPTY), who
            # the best mix is at least as good as any of the four fixed ones
            assert q.ncc_best >= max(abs(q.ncc_left), abs(q.ncc_right), abs(q.ncc_mid), abs(q.ncc_side)) - 1e-12, (who, q)
            # never within a factor 1000 of the collinear threshold unless exactly collinear (one sample: rank 1)
            if s == 1:
                assert q.flags & ref.COLLINEAR and abs(q.det_ratio) < 1e-12, (who, q)
            else:
                assert q.det_ratio > 1000 * ref.MIN_INDEPENDENCE and not q.flags & ref.COLLINEAR, (who, q)
            # which flags fire: a channel is unrefined at R = 0 and at the ends of the lag range, else its vertex lies within 0.5
            for lag, best, bit in ((q.lag_left, q.best_left, ref.LEFT_UNREFINED), (q.lag_right, q.best_right, ref.RIGHT_UNREFINED)):
                if r == 0 or abs(best) == r:
                    assert q.flags & bit and lag == best, (who, q)
                assert abs(lag - best) <= 0.5 and (lag == best or not q.flags & bit), (who, q)
        if s >= 4096:
            both, left, inv, delayed, noise, beside2, before1 = recs[2:]
            if s < 30_000:      # (the longest needle's plants overlap: the figures below are those of separate ones)
                assert both.ncc_left > 0.8 and both.ncc_right > 0.8 and both.ncc_mid > 0.85, both
                assert (both.flags & ~(ref.LEFT_UNREFINED | ref.RIGHT_UNREFINED)) == 0, both
                assert inv.ncc_left > 0.8 and inv.ncc_right < -0.8, inv
                assert left.ncc_left > 0.8 and abs(left.ncc_right) < 0.1 and abs(noise.ncc_best) < 0.1
                assert abs(inv.ncc_mid) < 0.1 and inv.ncc_side > 0.85 and inv.ncc_best >= inv.ncc_side
            if r >= 4:
                assert both.best_left == 0 == both.best_right and abs(both.lag_left) < 0.05
                assert delayed.best_left == 0 and delayed.best_right == 3 and abs(delayed.lag_left - delayed.lag_right + 3) < 0.1
                assert beside2.best_left == -2 == beside2.best_right and before1.best_left == 1 == before1.best_right


def test_checker_special_cases():
    """The flags of the header on exact inputs, by the checker alone (the GPU tests hold the library to the same)."""
    s, r = 300, 4
    needle = needle_of(s)
    p = np.rint(needle.astype(np.float64) / ref.K).astype(np.int16)
    lr = np.zeros((1000, 2), dtype=np.int16)
    lr[100:100 + s, 0] = p
    lr[100:100 + s, 1] = p
    q = ref.stereo_ref(lr, needle, 100, r)
    assert q.flags == ref.COLLINEAR | ref.SIDE_SILENT and q.ncc_side == 0.0 and q.ncc_best == abs(q.ncc_left) and q.mix_right == 0.0
    assert q.ncc_left > 0.9999 and q.ncc_mid > 0.9999
    lr[:, 1] = 0
    q = ref.stereo_ref(lr, needle, 100, r)
    assert q.flags & ref.RIGHT_SILENT and q.flags & ref.COLLINEAR and q.ncc_right == 0.0 and q.gain_right == 0.0
    lr[:, 1] = -lr[:, 0]
    q = ref.stereo_ref(lr, needle, 100, r)
    assert q.flags & ref.BELOW and q.flags & ref.COLLINEAR and q.ncc_mid == 0.0 and abs(q.ncc_side - q.ncc_left) < 1e-15
    assert ref.summary_ref(q, 0.5)[0] == ref.INVERTED
    bad = needle.copy()
    bad[7] = np.nan
    q = ref.stereo_ref(lr, bad, 100, r)
    assert q.flags == ref.NONFIN and np.isnan(q.ncc_best) and q.lag_left == 0.0
    lr[:, :] = 0
    q = ref.stereo_ref(lr, needle, 100, r)
    assert q.flags & ref.LEFT_SILENT and q.flags & ref.RIGHT_SILENT and q.ncc_best == 0.0 and q.mix_left == 0.0 == q.mix_right


def test_mix_ref_is_the_downmix_at_a_half():
    rng = np.random.default_rng(5)
    lr = rng.integers(-32768, 32768, size=(5000, 2)).astype(np.int16)
    lr[:4] = [[32767, 32767], [-32768, -32768], [32767, -32768], [0, 1]]
    assert ref.mix_ref(0.5, 0.5, lr).tobytes() == ref.downmix(lr).tobytes()
    assert ref.mix_ref(1.0, 0.0, lr).tobytes() == (lr[:, 0].astype(np.float64) * ref.K).astype(np.float32).tobytes()
    side = ref.mix_ref(0.5, -0.5, lr)
    assert side[2] == np.float32(0.5 * 65535 * ref.K) and side[0] == 0.0


# ---- the CLI's parsing of --mix and --stereo ---------------------------------------------------------------------------
PARSE_CPP = r"""
#include <cstdio>
#include "am_host.hpp"
using namespace amhost;
int main(int argc, char** argv) {
    try {
        const Arguments a = parse_arguments(argc, argv);
        std::printf("ok mix_set %d a %.9g b %.9g stereo %d radius %u min_ncc %.9g\n", (int)a.mix_set, (double)a.mix_a, (double)a.mix_b,
                    (int)a.stereo_radius.has_value(), a.stereo_radius ? *a.stereo_radius : 0u, (double)a.stereo_min_ncc);
    } catch (const ArgError& e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """parse_arguments of the CLI's host header (the code host/selftest.cpp checks), as a small program: g++ only, no
    device."""
    d = tmp_path_factory.mktemp("parse")
    (d / "parse.cpp").write_text(PARSE_CPP)
    exe = str(d / "parse")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "audio-matcher_amd", "host"), "-o", exe, str(d / "parse.cpp")])

    def run(*opts, live=False):
        tail = ["--live", "--rate", "8000"] if live else ["main.wav"]
        return subprocess.run([exe, "--snippet", "s.wav", *opts, *tail], capture_output=True, text=True, check=True).stdout.strip()

    return run


def test_cli_parses_mix_and_stereo(parse):
    assert parse() == "ok mix_set 0 a 0.5 b 0.5 stereo 0 radius 0 min_ncc 0.5"
    for word, a, b in (("left", 1, 0), ("right", 0, 1), ("mid", 0.5, 0.5), ("side", 0.5, -0.5), ("0.3,-1.7", np.float32(0.3), np.float32(-1.7)),
                       ("1e-3,2", np.float32(1e-3), 2)):
        assert parse("--mix", word) == "ok mix_set 1 a %.9g b %.9g stereo 0 radius 0 min_ncc 0.5" % (a, b), word
    for bad in ("", "centre", "0.5", "0.5,", ",0.5", "0.5,x", "1,2,3", "nan,1", "1,inf"):
        out = parse("--mix", bad)
        assert out.startswith("refused") and "--mix" in out, (bad, out)
    assert parse("--stereo", "4") == "ok mix_set 0 a 0.5 b 0.5 stereo 1 radius 4 min_ncc 0.5"
    assert parse("--stereo", "0:0.25") == "ok mix_set 0 a 0.5 b 0.5 stereo 1 radius 0 min_ncc 0.25"
    assert parse("--stereo", "16:1") == "ok mix_set 0 a 0.5 b 0.5 stereo 1 radius 16 min_ncc 1"
    assert parse("--mix", "side", "--stereo", "8") == "ok mix_set 1 a 0.5 b -0.5 stereo 1 radius 8 min_ncc 0.5"
    for bad in ("", "17", "-1", "x", "4:", "4:x", "4:1.5", "4:-0.1", "4:nan", "4.5"):
        out = parse("--stereo", bad)
        assert out.startswith("refused") and "--stereo" in out, (bad, out)
    for other in (["--resample"], ["--whiten", "8"], ["--preemphasis", "0.9"]):
        out = parse("--stereo", "4", *other)
        assert out.startswith("refused") and "--stereo does not apply with" in out, (other, out)
    assert parse("--mix", "side", live=True) == "refused --live: --mix does not apply"
    assert parse("--stereo", "4", live=True) == "refused --live: --stereo does not apply"
    assert parse("--mix", "side", "--whiten", "8").startswith("ok")
