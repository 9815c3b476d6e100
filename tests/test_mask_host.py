"""CPU tests of masked matching: gap validation through the library (it needs no device), the mirrors, and the designs
of mask_ref.py held to their own claims."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mask_ref as mr
import score_norm_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FUNCS = ("am_needle_create_masked", "am_needle_create_masked_device", "am_needle_mask",
         "am_hit_mask", "am_hit_mask_device", "am_hit_mask_batch_device")


# ---- the interface ---------------------------------------------------------------------------------------------------
def test_header_mirrors_and_exports(amlib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "audiomatch.h")).read(), flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in amlib.declared_symbols() and name in exported, name
        assert "pub fn " + name + "(" in rust, name
    for name in ("am_needle_create_masked", "am_needle_mask", "am_hit_mask", "am_hit_mask_device", "am_hit_mask_batch_device"):
        assert name in hpp, name
    assert re.search(r"#define\s+AM_MASK_MAX_GAPS\s+15\b", code) and amlib.AM_MASK_MAX_GAPS == mr.MAX_GAPS == 15
    assert "typedef struct am_span" in code and "pub struct AmSpan" in rust
    assert "typedef struct am_mask_hit" in code and "pub struct AmMaskHit" in rust
    assert C.sizeof(amlib.AmSpan) == 16 and C.sizeof(amlib.HitMask) == 24
    flags = dict(re.findall(r"(AM_MASK_[A-Z_]+) = (\d+)", code))
    assert {k: int(v) for k, v in flags.items()} == {
        "AM_MASK_BELOW_FLOOR": mr.BELOW_FLOOR, "AM_MASK_NONFINITE": mr.NONFINITE, "AM_MASK_GAPS_SILENT": mr.GAPS_SILENT,
        "AM_MASK_GAPS_NONFINITE": mr.GAPS_NONFINITE, "AM_MASK_NO_GAPS": mr.NO_GAPS}
    assert (amlib.AM_MASK_BELOW_FLOOR, amlib.AM_MASK_NONFINITE, amlib.AM_MASK_GAPS_SILENT, amlib.AM_MASK_GAPS_NONFINITE,
            amlib.AM_MASK_NO_GAPS) == (1, 2, 4, 8, 16)
    for fn in ("hit_mask", "hit_mask_device", "mask"):
        assert callable(getattr(amlib.HipConvolve, fn))
    assert callable(amlib.hit_mask_batch_device)
    assert amlib.lib().am_abi_version() == 3


def test_header_compiles_as_c(tmp_path):
    """The record and the function that fills it have different names (a typedef and a function cannot share one in C)."""
    src = tmp_path / "t.c"
    src.write_text('#include "audiomatch.h"\n_Static_assert(sizeof(am_mask_hit) == 24, "record");\n'
                   '_Static_assert(sizeof(am_span) == 16, "span");\nint main(void) { return AM_MASK_MAX_GAPS == 15 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_hit_mask_ref_cases():
    """The checker on cases with known answers."""
    rng = np.random.default_rng(2)
    needle = rng.uniform(-1, 1, 64).astype(np.float32)
    gaps = [(10, 20), (50, 64)]
    x = np.zeros(200, dtype=np.float32)
    x[30:94] = 2 * needle
    ncc, gain, kept_db, ncc_gaps, gaps_db, flags = mr.hit_mask_ref(x, needle, gaps, 30)
    assert flags == 0 and abs(ncc - 1) < 1e-12 and abs(gain - 2) < 1e-12 and abs(ncc_gaps - 1) < 1e-12 and abs(gaps_db) < 1e-9
    assert abs(kept_db - 20 * np.log10(2)) < 1e-9
    y = x.copy()
    y[80:94] = 0
    y[40:50] = 0
    r = mr.hit_mask_ref(y, needle, gaps, 30)
    assert r[5] == mr.GAPS_SILENT and r[3] == 0.0 and r[4] == -np.inf and abs(r[0] - 1) < 1e-12
    y[45] = np.nan
    r = mr.hit_mask_ref(y, needle, gaps, 30)
    assert r[5] == mr.GAPS_NONFINITE and np.isnan(r[3]) and abs(r[0] - 1) < 1e-12
    y[60] = np.nan
    assert mr.hit_mask_ref(y, needle, gaps, 30)[5] == mr.NONFINITE
    r = mr.hit_mask_ref(x, needle, None, 30)
    assert r[5] == mr.NO_GAPS and np.isnan(r[3]) and np.isnan(r[4])
    assert mr.hit_mask_ref(np.zeros(200, dtype=np.float32), needle, gaps, 0)[5] == mr.BELOW_FLOOR | mr.GAPS_SILENT


REFUSED = [
    # (n, gaps, what the message must name)
    (100, [(5, 5)], ("gap 0", "begin < end")),
    (100, [(7, 5)], ("gap 0", "begin < end")),
    (100, [(2, 4), (90, 101)], ("gap 1", "end <= n")),
    (100, [(10, 20), (15, 30)], ("gap 1", "ascend")),
    (100, [(40, 50), (10, 20)], ("gap 1", "ascend")),
    (100, [(10, 20), (20, 30)], ("gap 1", "touch")),
    (100, [(0, 100)], ("gap 0", "at least one sample")),
    (100, [(2 * k, 2 * k + 1) for k in range(16)], ("16 gaps", "AM_MASK_MAX_GAPS")),
    ((1 << 22) + 1, [(3, 4)], ("partitioned",)),
]


@pytest.mark.parametrize("n,gaps,words", REFUSED)
def test_gap_rules_refused(amlib, n, gaps, words):
    """Every rule of the header, refused before a device is looked for: AM_ERR_INVALID_ARG, the message names the gap and
    the rule.  mask_ref.gap_violation agrees on which masks are refused."""
    assert mr.gap_violation(n, gaps) is not None or "partitioned" in words
    a = np.ones(8, dtype=np.float32)   # (never read: the gaps are checked first)
    arr, k = amlib._spans(gaps)
    h = C.c_void_p()
    for fn in (amlib.lib().am_needle_create_masked, amlib.lib().am_needle_create_masked_device):
        assert fn(0, a.ctypes.data, n, arr, k, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
        msg = amlib.lib().am_last_error_string().decode()
        assert all(w in msg for w in words), msg
        assert not h.value


def test_null_arguments(amlib):
    L = amlib.lib()
    h = C.c_void_p()
    a = np.ones(8, dtype=np.float32)
    assert L.am_needle_create_masked(0, None, 8, None, 0, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_needle_create_masked(0, a.ctypes.data, 0, None, 0, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_needle_create_masked(0, a.ctypes.data, 8, None, 0, None) == amlib.AM_ERR_INVALID_ARG
    assert L.am_needle_create_masked(0, a.ctypes.data, 8, None, 2, C.byref(h)) == amlib.AM_ERR_INVALID_ARG
    assert "null gaps" in L.am_last_error_string().decode()
    n = C.c_size_t(7)
    arr = (amlib.AmSpan * 2)()
    assert L.am_needle_mask(None, arr, 2, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    assert "null needle handle" in L.am_last_error_string().decode()


def test_valid_masks_pass_the_rules():
    for name, (n, kept, gaps) in mr.DESIGNS.items():
        assert mr.gap_violation(n, gaps) is None, name
        assert mr.kept_spans(n, gaps) == kept, name
        assert len(kept) <= mr.MAX_GAPS + 1
    assert len(mr.DESIGNS["sixteen"][1]) == 16 and len(mr.DESIGNS["sixteen"][2]) == 15
    assert mr.gap_violation(10, [(0, 3), (9, 10)]) is None and mr.kept_spans(10, [(0, 3), (9, 10)]) == [(3, 9)]
    assert mr.gap_violation(10, []) is None and mr.kept_spans(10, []) == [(0, 10)]


# ---- the reference against the definition ----------------------------------------------------------------------------
def test_masked_energy_against_the_definition():
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, size=300).astype(np.float32)
    kept = [(0, 1), (4, 30), (31, 33), (60, 97)]
    for mode in ref.SPIKE_MODES:
        lead, n = ref.lead_of(len(x), 100, mode), ref.mode_len(len(x), 100, mode)
        assert np.array_equal(mr.masked_energy(x, kept, lead, n), mr.masked_energy_direct(x, kept, lead, n))
    # no gaps: the window energy
    assert np.array_equal(mr.masked_energy(x, [(0, 100)], 0, 201), ref.window_energy(x, 100, 0, 201))


def test_mncc_ref_without_gaps_is_ncc_ref(oracle):
    rng = np.random.default_rng(5)
    needle, x = rng.uniform(-1, 1, 50).astype(np.float32), rng.uniform(-1, 1, 400).astype(np.float32)
    for mode in ref.SPIKE_MODES:
        a, _, _ = mr.mncc_ref(oracle, x, needle, [], mode)
        b, _, _ = ref.ncc_ref(oracle, x, needle, mode)
        assert np.allclose(a, b, rtol=0, atol=1e-15)
    # a perfect occurrence with anything in the gap scores 1
    gaps = [(20, 40)]
    x[100:150] = needle
    x[120:140] = 50.0
    y, _, _ = mr.mncc_ref(oracle, x, needle, gaps, oracle.MODE_VALID)
    assert abs(y[100] - 1.0) <= 1e-6   # (the oracle's correlation is a transform: about 1e-8 with a sample of 50 beside)
    plain, _, _ = ref.ncc_ref(oracle, x, mr.zero_filled(needle, gaps), oracle.MODE_VALID)
    assert plain[100] < 0.05


# ---- design 1 held to its claims -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mr.DESIGNS))
def test_design_energies_and_edge_sensitivity(name):
    """Every designed masked energy is an integer below 2^8 (exact in f64 whatever the order of the additions), and
    moving ANY edge of any kept span by one sample, either way, changes some window's energy by at least MIN_DEFECT
    (relative): an index error of one sample at any edge cannot hide under the device test's bound."""
    s, kept, gaps = mr.DESIGNS[name]
    w = mr.design_width(s)
    assert 2 * w + s < 1 << 19
    for mode in ref.SPIKE_MODES:
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        assert n > ref.NORM_TILE and n % ref.NORM_TILE != 0
        x = mr.mask_signal(s, kept, w, mode)
        assert np.all(x == np.round(x)) and x.min() >= 0 and x.max() <= 2
        E = mr.masked_energy(x, kept, lead, n)
        assert np.all(E == np.round(E)) and E.max() < 2 ** 8, (name, mode, E.max())
        assert np.count_nonzero(E > 0) > n // 2
        for j, which, by, Ev in mr.edge_variants(x, kept, lead, n):
            pos = E > 0
            d = np.max(np.abs(Ev[pos] - E[pos]) / E[pos])
            assert d >= ref.MIN_DEFECT, (name, mode, j, which, by, d)


def test_silent_case_design():
    for mode in ref.SPIKE_MODES:
        needle, gaps, within, lo, hi = mr.silent_case(mode)
        s, w = len(needle), len(within)
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        kept = mr.kept_spans(s, gaps)
        assert [b - a for a, b in kept] == [4500, 4500] and 4500 >= mr.SWITCH
        E = mr.masked_energy(within, kept, lead, n)
        whole = ref.window_energy(within, s, lead, n)
        assert 0 <= lo < hi <= n and hi - lo == 1000 - mr.SILENT_BURST + 1
        assert np.all(E[lo:hi] == 0) and np.all(whole[lo:hi] == mr.SILENT_BURST * 100.0 ** 2)
        assert E[lo - 1] > 0 and E[hi] > 0


# ---- design 2 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", mr.PLANT_S)
def test_plant_design(oracle, S):
    """The gap's noise is 20 dB above the needle; a plant scores about 1 under the mask and about 0.12 as the zero-filled
    needle under the whole window's energy: far below the prominence bound."""
    needle, gaps, hay, plants = mr.plant_case(oracle, S)
    (g0, g1), = gaps
    assert g1 - g0 == round(0.4 * S)
    t = plants[1]
    db = 10 * np.log10(np.mean(hay[t + g0:t + g1].astype(np.float64) ** 2) / np.mean(needle.astype(np.float64) ** 2))
    assert abs(db - 20.0) < 0.5, db
    seg = hay[t - 50:t + S + 50]
    y, _, _ = mr.mncc_ref(oracle, seg, needle, gaps, oracle.MODE_VALID)
    plain, _, _ = ref.ncc_ref(oracle, seg, mr.zero_filled(needle, gaps), oracle.MODE_VALID)
    assert y[50] > 0.97 and int(np.argmax(y)) == 50   # (1 / sqrt(1 + 0.04): the background under the kept spans)
    assert plain.max() < 0.2 < ref.PLANT_PROMINENCE
