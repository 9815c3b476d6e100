"""CPU tests of edge matching: the numpy reference (edges_ref.py) and the designs of the GPU tests held to their claims,
am_edge_scores_len and every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest

import edges_ref as er

P = er.PLANT


# ---- the reference against the definitions as plain loops ----------------------------------------------------------------
@pytest.mark.parametrize("s,length", [(1, 5), (2, 1), (2, 5), (7, 3), (7, 6), (7, 7), (7, 8), (7, 12), (7, 19), (12, 5)])
def test_reference_follows_the_definitions(s, length):
    needle, x = er.white(s, 10 * s + length), er.white(length, 7 * s + length)
    for edge in (er.HEAD, er.TAIL):
        naive = er.naive_terms(needle, x, edge)
        t = er.edge_terms(needle, x, edge)
        n_lags, first = er.geometry(length, s, edge)
        assert n_lags == len(naive) == t["L"].size == min(length, s - 1)
        if n_lags:
            assert [u for u, *_ in naive] == list(range(first, first + n_lags))
            assert [L for _, L, *_ in naive] == list(t["L"])
            for k, key in ((2, "c"), (3, "en"), (4, "ex")):
                np.testing.assert_allclose([row[k] for row in naive], t[key], rtol=1e-12, atol=1e-12)
        # the spans are the ones the header names
        sp = er.span_of(x, s, edge)
        assert sp.size == n_lags
        assert np.array_equal(sp, x[:n_lags] if edge == er.HEAD else x[length - n_lags:])


def test_lags_cut_at_both_ends_are_no_lags():
    s, length = 10, 4
    for edge in (er.HEAD, er.TAIL):
        n, first = er.geometry(length, s, edge)
        for u in range(first, first + n):
            assert not (u < 0 and u + s > length)
    assert er.geometry(length, s, er.HEAD) == (4, -9) and er.geometry(length, s, er.TAIL) == (4, 0)


def test_nonfinite_samples_cost_exactly_the_lags_that_hold_them():
    s, length = 9, 30
    needle, x = er.white(s, 1), er.white(length, 2)
    x[3] = np.nan
    x[length - 5] = np.inf
    sc, t, mask = er.coarse(needle, x, er.HEAD, 1, 0.0)
    assert list(mask) == [L <= 3 for L in t["L"]]          # x[0, L) holds x[3] iff L > 3
    sc, t, mask = er.coarse(needle, x, er.TAIL, 1, 0.0)
    lags = t["first"] + np.arange(mask.size)
    assert list(mask) == [u > length - 5 for u in lags]    # x[u, len) holds x[len - 5] iff u <= len - 5
    assert np.all(np.isfinite(sc[mask]))


def test_record_rule_and_flags():
    needle, x = er.white(50, 3), er.white(200, 4)
    assert int(er.record(needle, x, er.HEAD, 60, 0, 0.0)["flags"]) == er.NO_BEST | er.NO_SECOND   # no lag overlaps that much
    r = er.record(needle, x, er.TAIL, 1, 1000, 0.0)
    assert int(r["flags"]) == er.NO_SECOND and np.isnan(r["ncc_second"]) and int(r["second"]) == 0
    bad = needle.copy()
    bad[7] = np.inf
    r = er.record(bad, x, er.HEAD, 1, 0, 0.0)
    assert int(r["flags"]) == er.NONFINITE and np.isnan(r["ncc"])
    r = er.record(needle, np.zeros(200, np.float32), er.HEAD, 1, 0, 0.0)
    assert int(r["flags"]) & er.BELOW_FLOOR and float(r["ncc"]) == 0.0
    assert er.pick(np.array([np.nan, 1.0, 1.0, 0.5, 1.0]), 2) == (1, 4)


# ---- the planted designs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", er.PLANT_SEEDS)
def test_planted_lags_are_the_reference_best(seed):
    needle, x, u_head, u_tail = er.planted(seed)
    for edge, want in ((er.HEAD, u_head), (er.TAIL, u_tail)):
        r = er.record(needle, x, edge, P["min_overlap"], 0, P["min_share"])
        assert int(r["start"]) == want and int(r["flags"]) == 0
        assert 0.83 <= float(r["ncc"]) <= 0.87, float(r["ncc"])
        assert float(r["ncc_second"]) <= 0.5 * float(r["ncc"]) and float(r["ncc_second"]) <= 0.16
        assert abs(float(r["gain"]) - P["gain"]) < 0.05
        L = P["S"] - P["head_missing"] if edge == er.HEAD else P["tail_kept"]
        assert int(r["overlap"]) == L and abs(float(r["share"]) - L / P["S"]) < 0.03


@pytest.mark.parametrize("seed", er.PLANT_SEEDS[:2])
def test_clip_and_noise(seed):
    needle, x, u = er.clip_inside(seed)
    r = er.record(needle, x, er.HEAD, P["min_overlap"], 0, P["min_share"])
    assert int(r["start"]) == u and float(r["ncc"]) >= 0.95 and int(r["overlap"]) == x.size
    assert int(r["flags"]) == er.NO_SECOND or float(r["ncc_second"]) <= 0.5 * float(r["ncc"])
    needle, x = er.noise_only(seed)
    for edge in (er.HEAD, er.TAIL):
        r = er.record(needle, x, edge, P["min_overlap"], 0, P["min_share"])
        assert float(r["ncc"]) <= 0.16


def test_candidate_counts_are_as_designed():
    needle, x, _, _ = er.planted(1)
    s = P["S"]
    for edge in (er.HEAD, er.TAIL):
        sc, t, mask = er.coarse(needle, x, edge, P["min_overlap"], P["min_share"])
        assert mask.size == s - 1
        # a white needle: E_n(u) / E_n is close to L / S, so min_share = 0.05 cuts near L = 300, below min_overlap = 512
        assert int(mask.sum()) == s - 1 - (P["min_overlap"] - 1)
        sc0, _, mask0 = er.coarse(needle, x, edge, 1, 0.0)
        assert int(mask0.sum()) == s - 1
    # silent tenths: at the head E_n(u) is a suffix sum, 0 over the silent last tenth
    n2 = er.silent_tenths(1000, 5)
    xs = er.white(3000, 6)
    for edge in (er.HEAD, er.TAIL):
        _, t, mask = er.coarse(n2, xs, edge, 1, 0.05)
        assert not mask[t["L"] <= 100].any() and mask[t["L"] >= 200].all()
        _, _, mask0 = er.coarse(n2, xs, edge, 1, 0.0)
        assert mask0.all()


def test_one_reference_serves_both_formats():
    needle, pcm = er.case_signals(65, 135, 3)
    x = er.downmix(pcm)
    assert x.dtype == np.float32 and x.size == 135 and pcm.shape == (135, 2) and np.any(pcm[:, 0] != pcm[:, 1])
    r = er.record(needle, x, er.HEAD, 1, 0, 0.0)
    assert int(r["start"]) == -(65 - 33)


# ---- the library without a device ----------------------------------------------------------------------------------------
def test_edge_scores_len(amlib):
    for s in (1, 2, 3, 64, 4097, 40000):
        for length in (1, 2, s - 1, s, s + 1, 2 * s - 2, 3 * s):
            if length < 1:
                continue
            for edge in (er.HEAD, er.TAIL):
                n, first = amlib.edge_scores_len(length, s, edge)
                want_n, want_first = er.geometry(length, s, edge)
                assert n == want_n == min(length, s - 1)
                if n:
                    assert first == want_first, (s, length, edge)
    L = amlib.lib()
    n, f = C.c_size_t(0), C.c_int64(0)
    assert L.am_edge_scores_len(0, 5, 0, C.byref(n), C.byref(f)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores_len(5, 0, 0, C.byref(n), C.byref(f)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores_len(5, 5, 2, C.byref(n), C.byref(f)) == amlib.AM_ERR_INVALID_ARG
    assert b"edge" in L.am_last_error_string()
    assert L.am_edge_scores_len(5, 5, -1, C.byref(n), C.byref(f)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores_len(5, 5, 0, None, C.byref(f)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores_len(5, 5, 0, C.byref(n), None) == amlib.AM_ERR_INVALID_ARG
    assert L.am_last_error_string() == b"null pointer"


def test_refusals_without_a_device(amlib):
    L = amlib.lib()
    ep = amlib.edge_params(16)
    x = np.zeros(64, np.float32)
    out = np.zeros(2, amlib.EDGE_HIT_DTYPE)
    sc = np.zeros(64, np.float32)
    n = C.c_size_t(0)
    # a null needle handle is refused before anything else
    assert L.am_match_edges(None, x.ctypes.data, 64, 0, C.byref(ep), out.ctypes.data) == amlib.AM_ERR_INVALID_ARG
    assert b"needle" in L.am_last_error_string()
    assert L.am_match_edges_device(None, x.ctypes.data, 64, 0, C.byref(ep), out.ctypes.data) == amlib.AM_ERR_INVALID_ARG
    assert L.am_match_edges_batch_device(None, None, None, 0, 0, C.byref(ep), out.ctypes.data) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores(None, x.ctypes.data, 64, 0, 0, C.byref(ep), sc.ctypes.data, 64, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    assert L.am_edge_scores_device(None, x.ctypes.data, 64, 0, 0, C.byref(ep), sc.ctypes.data, 64, C.byref(n)) == amlib.AM_ERR_INVALID_ARG
    # the structs have the header's sizes
    assert C.sizeof(amlib.AmEdgeParams) == 24 and amlib.EDGE_HIT_DTYPE.itemsize == 48
    assert (amlib.AM_EDGE_HEAD, amlib.AM_EDGE_TAIL) == (er.HEAD, er.TAIL)
    assert (amlib.AM_EDGE_NO_BEST, amlib.AM_EDGE_NO_SECOND, amlib.AM_EDGE_NONFINITE, amlib.AM_EDGE_BELOW_FLOOR) == (1, 2, 4, 8)
