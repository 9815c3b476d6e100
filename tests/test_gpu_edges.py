"""GPU tests of edge matching (include/audiomatch.h, "edge matching") against the f64 reference of edges_ref.py.

Coarse scores.  The NaN mask equals the reference's exactly.  The error bound of a candidate is measured, not assumed:
eps = max_j |a[j] - c_ref[j]| with a = am_correlate(h, span, Full, AM_SCALE_NONE) on the sanitised span -- the engine
as it was before this family existed -- and then |coarse(u) - ref(u)| <= 2 eps / sqrt(E_n(u) E_x(u)) + 2^-22: the factor 2
covers a scale applied before the f32 rounding, the additive term the rounding of a quotient of magnitude at most 1.

Records.  The lags and flags are, bit for bit, what am_probe_scores gives on the array am_edge_scores returned; the exact
fields lie within one f32 ulp of the reference's f64 values at those lags.

Every case ran on unpartitioned handles only: a needle is cut into segments from 2^22 samples on, whatever "log_n" says.
"""
import ctypes as C

import numpy as np
import pytest

import edges_ref as er

pytestmark = pytest.mark.gpu

T = 4096   # AM_EDGE_TILE (asserted below)
SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 40000)
MAX_SAMPLES = 200000


def lengths_of(s):
    out = []
    for length in (1, s - 1, s, s + 1, 2 * s - 2, 2 * s + 5, 3 * s):
        if length >= 1 and s + length <= MAX_SAMPLES and length not in out:
            out.append(length)
    return out


def check_coarse(gpu, h, needle, x, t, edge, got, min_overlap, min_share, eps, what):
    """got against the reference: the mask exactly, every candidate within the measured bound; the largest error ratio."""
    ncc, _ = er.scores_of(t)
    mask = er.candidates(t, needle, min_overlap, min_share)
    assert got.size == mask.size, what
    assert np.array_equal(~np.isnan(got), mask), (what, np.flatnonzero(np.isnan(got) == mask)[:8])
    if not mask.any():
        return 0.0
    den = np.sqrt(t["en"] * t["ex"])[mask]
    with np.errstate(divide="ignore"):
        bound = 2.0 * eps / den + 2.0 ** -22
    err = np.abs(got[mask].astype(np.float64) - ncc[mask])
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), (what, "lag index", int(np.flatnonzero(mask)[worst]), "error", err[worst], "bound", bound[worst], "eps", eps)
    return float(np.max(err / bound))


def measured_eps(gpu, h, needle, x, edge):
    """max |am_correlate(Full, unscaled) - f64 correlation| over the sanitised span, and the f64 terms of the edge."""
    t = er.edge_terms(needle, x, edge)
    span, _ = er.sanitise(np.asarray(er.span_of(x, needle.size, edge), dtype=np.float32))
    a = h.correlate_with_sample(span.astype(np.float32), gpu.Mode.Full, False)
    full = t["full"]
    return float(np.max(np.abs(a.astype(np.float64) - full))), t


# ---- 1. every coarse score -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,length", [(s, length) for s in SIZES for length in lengths_of(s)])
def test_every_coarse_score(gpu, s, length):
    assert gpu.AM_EDGE_TILE == T
    ratios = []
    needle, pcm = er.case_signals(s, length, 100 * s + length)
    x = er.downmix(pcm)
    h = gpu.HipConvolve(needle)
    big = max(2, s // 3)
    for edge in (er.HEAD, er.TAIL):
        n_lags, first = gpu.edge_scores_len(length, s, edge)
        assert n_lags == er.geometry(length, s, edge)[0]
        if n_lags == 0:
            assert h.edge_scores(x, edge, gpu.edge_params(1, 0, 0.0)).size == 0
            assert h.edge_scores(pcm, edge, gpu.edge_params(1, 0, 0.0)).size == 0
            continue
        assert first == er.geometry(length, s, edge)[1]
        eps, t = measured_eps(gpu, h, needle, x, edge)
        for min_overlap in (1, big):
            for min_share in (0.0, 0.05):
                ep = gpu.edge_params(min_overlap, 0, min_share)
                what = dict(S=s, len=length, edge=edge, min_overlap=min_overlap, min_share=min_share)
                got32 = h.edge_scores(x, edge, ep)
                got16 = h.edge_scores(pcm, edge, ep)
                assert np.array_equal(got32.view(np.uint32), got16.view(np.uint32)), what
                ratios.append(check_coarse(gpu, h, needle, x, t, edge, got32, min_overlap, min_share, eps, what))
    h.close()
    print("S = %d, len = %d: largest coarse error / bound = %.3f" % (s, length, max(ratios, default=0.0)))


# ---- 2. records ------------------------------------------------------------------------------------------------------
def check_record(gpu, h, needle, x, edge, ep, rec, what):
    """rec against am_probe_scores on the coarse array (bit level) and against the reference's f64 values (one ulp)."""
    sep = int(ep.separation) if ep.separation else int(ep.min_overlap)
    assert int(rec["edge"]) == edge, what
    n_lags, first = er.geometry(x.size, needle.size, edge)
    if n_lags == 0:
        assert int(rec["flags"]) == er.NO_BEST | er.NO_SECOND and int(rec["start"]) == 0 and np.isnan(rec["ncc"]), (what, rec)
        return
    arr = h.edge_scores(x, edge, ep)
    pr = gpu.probe_scores(arr, 0, 0, sep)
    if int(pr["flags"]) & 1:
        assert int(rec["flags"]) == er.NO_BEST | er.NO_SECOND, (what, rec)
        assert int(rec["start"]) == 0 and int(rec["second"]) == 0 and int(rec["overlap"]) == 0, (what, rec)
        assert all(np.isnan(rec[k]) for k in ("ncc", "ncc_second", "gain", "share")), (what, rec)
        return
    assert int(rec["start"]) == first + int(pr["best"]), (what, rec, pr)
    assert (int(rec["flags"]) & 3) == int(pr["flags"]), (what, rec, pr)
    assert int(rec["second"]) == (0 if int(pr["flags"]) & 2 else first + int(pr["second"])), (what, rec, pr)
    ref = er.record(needle, x, edge, ep.min_overlap, ep.separation, ep.min_share, on=arr)
    assert int(ref["start"]) == int(rec["start"]) and int(ref["second"]) == int(rec["second"]), (what, rec, ref)
    assert int(rec["flags"]) == int(ref["flags"]) and int(rec["overlap"]) == int(ref["overlap"]), (what, rec, ref)
    for k in ("ncc", "ncc_second", "gain", "share"):
        if np.isnan(ref[k]):
            assert np.isnan(rec[k]), (what, k, rec, ref)
        else:
            assert abs(float(rec[k]) - float(ref[k])) <= er.ulp32(float(ref[k])), (what, k, float(rec[k]), float(ref[k]))


@pytest.mark.parametrize("s", (2, 65, T + 1, 2 * T + 1))
def test_records_against_probe_scores_and_reference(gpu, s):
    for length in lengths_of(s):
        needle, pcm = er.case_signals(s, length, 7 * s + length)
        x = er.downmix(pcm)
        h = gpu.HipConvolve(needle)
        for ep in (gpu.edge_params(1, 0, 0.0), gpu.edge_params(max(2, s // 3), max(1, s // 8), 0.05)):
            recs = h.match_edges(x, ep)
            for edge in (er.HEAD, er.TAIL):
                check_record(gpu, h, needle, x, edge, ep, recs[edge], dict(S=s, len=length, edge=edge, min_overlap=int(ep.min_overlap)))
        h.close()


@pytest.mark.parametrize("seed", er.PLANT_SEEDS)
def test_planted_cases_are_found(gpu, seed):
    p = er.PLANT
    needle, x, u_head, u_tail = er.planted(seed)
    h = gpu.HipConvolve(needle)
    ep = gpu.edge_params(p["min_overlap"], 0, p["min_share"])
    recs = h.match_edges(x, ep)
    for edge, want in ((er.HEAD, u_head), (er.TAIL, u_tail)):
        r = recs[edge]
        assert int(r["start"]) == want and int(r["flags"]) == 0, (edge, r)
        assert float(r["ncc"]) >= 0.8 and float(r["ncc_second"]) <= 0.5 * float(r["ncc"]), (edge, r)
        check_record(gpu, h, needle, x, edge, ep, r, dict(seed=seed, edge=edge))
    h.close()
    needle, x, u = er.clip_inside(seed)
    h = gpu.HipConvolve(needle)
    recs = h.match_edges(x, ep)
    assert int(recs[0]["start"]) == u and float(recs[0]["ncc"]) >= 0.9 and int(recs[0]["overlap"]) == x.size, recs[0]
    check_record(gpu, h, needle, x, er.HEAD, ep, recs[0], dict(seed=seed, clip=True))
    h.close()


# ---- 3. forms --------------------------------------------------------------------------------------------------------
def test_forms_agree_bit_for_bit(gpu):
    s = T + 77
    needle, _ = er.case_signals(s, 3 * s, 11)
    h = gpu.HipConvolve(needle)
    ep = gpu.edge_params(200, 0, 0.05)
    pcms = [er.case_signals(s, length, 20 + i)[1] for i, length in enumerate((3 * s + 1, s - 300, 2 * s - 2))]
    # every haystack carries the needle's own cut ends (case_signals draws its own needle: plant this one)
    for pcm in pcms:
        length = pcm.shape[0]
        kh, kt = min(length, (s + 1) // 2), min(length, s // 2)
        pcm[:kh, 0] = np.clip(pcm[:kh, 0].astype(np.int32) + np.round(7000 * needle[s - kh:]).astype(np.int32), -32768, 32767)
        pcm[length - kt:, 1] = np.clip(pcm[length - kt:, 1].astype(np.int32) + np.round(7000 * needle[:kt]).astype(np.int32), -32768, 32767)
    for as_pcm in (False, True):
        hays = [pcm if as_pcm else er.downmix(pcm) for pcm in pcms]
        fmt = gpu.Fmt.S16_STEREO if as_pcm else gpu.Fmt.F32_MONO
        bufs = [gpu.DeviceBuffer.from_numpy(0, a) for a in hays]
        lens = [a.shape[0] for a in hays]
        host = [h.match_edges(a, ep) for a in hays]
        dev = [h.match_edges_device(b.ptr, n, ep, fmt=fmt) for b, n in zip(bufs, lens)]
        batch = h.match_edges_batch_device([b.ptr for b in bufs], lens, ep, fmt=fmt)
        rev = h.match_edges_batch_device([b.ptr for b in bufs][::-1], lens[::-1], ep, fmt=fmt)[::-1]
        for i in range(3):
            assert host[i].tobytes() == dev[i].tobytes() == batch[i].tobytes() == rev[i].tobytes(), (as_pcm, i, host[i], dev[i], batch[i])
            assert int(host[i][0]["flags"]) & 1 == 0 and int(host[i][0]["edge"]) == 0 and int(host[i][1]["edge"]) == 1
            sd = [h.edge_scores_device(bufs[i].ptr, lens[i], e, ep, fmt=fmt) for e in (0, 1)]
            sh = [h.edge_scores(hays[i], e, ep) for e in (0, 1)]
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(sd, sh))
        if as_pcm:
            for i in range(3):
                assert host[i].tobytes() == f32_host[i].tobytes(), (i, host[i], f32_host[i])   # i16 stereo = f32 of its down-mix
        else:
            f32_host = host
        for b in bufs:
            b.free()
    assert h.match_edges_batch_device([], [], ep).shape == (0, 2)
    h.close()


# ---- 4. rules --------------------------------------------------------------------------------------------------------
def test_nonfinite_haystack_samples_cost_exactly_their_lags(gpu):
    s, length = T + 301, 3 * T
    needle, pcm = er.case_signals(s, length, 31)
    x = er.downmix(pcm)
    h = gpu.HipConvolve(needle)
    for places in ((700,), (s - 2,), (0,), (5, 3000)):
        for edge in (er.HEAD, er.TAIL):
            y = x.copy()
            for k, p in enumerate(places):
                y[p if edge == er.HEAD else length - 1 - p] = (np.nan, np.inf)[k % 2]
            eps, t = measured_eps(gpu, h, needle, y, edge)
            got = h.edge_scores(y, edge, gpu.edge_params(1, 0, 0.0))
            lost = int(np.isnan(got).sum())
            assert lost == (s - 1) - min(places), (places, edge, lost)   # head: L > first index; tail mirrored
            check_coarse(gpu, h, needle, y, t, edge, got, 1, 0.0, eps, dict(places=places, edge=edge))
            rec = h.match_edges(y, gpu.edge_params(1, 0, 0.0))[edge]
            check_record(gpu, h, needle, y, edge, gpu.edge_params(1, 0, 0.0), rec, dict(places=places, edge=edge))
    h.close()


def test_min_share_on_a_needle_with_silent_ends(gpu):
    s, length = 5000, 9000
    needle = er.silent_tenths(s, 41)
    x = er.white(length, 42, 0.5)
    x[:3000] += np.float32(0.8) * needle[s - 3000:]
    x[length - 3000:] += np.float32(0.8) * needle[:3000]
    h = gpu.HipConvolve(needle)
    for edge in (er.HEAD, er.TAIL):
        eps, t = measured_eps(gpu, h, needle, x, edge)
        for min_share in (0.0, 0.05, 0.5):
            got = h.edge_scores(x, edge, gpu.edge_params(1, 0, min_share))
            check_coarse(gpu, h, needle, x, t, edge, got, 1, min_share, eps, dict(edge=edge, min_share=min_share))
            if min_share == 0.0:
                assert not np.isnan(got).any() and np.all(got[t["L"] <= s // 10] == 0.0)   # E_n(u) = 0: score 0, still a candidate
            else:
                assert np.isnan(got[t["L"] <= s // 10]).all()
    h.close()


def test_silence_nonfinite_needle_and_separation(gpu):
    s, length = 3000, 7000
    needle = er.white(s, 51)
    h = gpu.HipConvolve(needle)
    ep = gpu.edge_params(64, 0, 0.05)
    # a digitally silent haystack: every candidate scores 0, the best is flagged
    z = np.zeros(length, np.float32)
    for edge in (er.HEAD, er.TAIL):
        got = h.edge_scores(z, edge, ep)
        assert np.all(got[~np.isnan(got)] == 0.0) and (~np.isnan(got)).sum() > 0
    for r in h.match_edges(z, ep):
        assert int(r["flags"]) & er.BELOW_FLOOR and float(r["ncc"]) == 0.0 and not int(r["flags"]) & er.NO_BEST, r
    assert h.match_edges(np.zeros((length, 2), np.int16), ep).tobytes() == h.match_edges(z, ep).tobytes()
    # a separation larger than the lag range: no runner-up
    x = er.white(length, 52)
    for r in h.match_edges(x, gpu.edge_params(64, 10 * s, 0.05)):
        assert int(r["flags"]) == er.NO_SECOND and int(r["second"]) == 0 and np.isnan(r["ncc_second"]) and not np.isnan(r["ncc"]), r
    # min_overlap beyond every overlap: no candidate
    for r in h.match_edges(x, gpu.edge_params(s, 0, 0.0)):
        assert int(r["flags"]) == er.NO_BEST | er.NO_SECOND and np.isnan(r["ncc"]) and int(r["overlap"]) == 0, r
    assert np.isnan(h.edge_scores(x, 0, gpu.edge_params(s, 0, 0.0))).all()
    h.close()
    # a needle of one sample has no lags
    h1 = gpu.HipConvolve(np.ones(1, np.float32))
    for r in h1.match_edges(x, gpu.edge_params(1, 0, 0.0)):
        assert int(r["flags"]) == er.NO_BEST | er.NO_SECOND, r
    h1.close()
    # a non-finite needle sample
    bad = needle.copy()
    bad[100] = np.nan
    hb = gpu.HipConvolve(bad)
    recs = hb.match_edges(x, ep)
    for e, r in enumerate(recs):
        assert int(r["flags"]) == er.NONFINITE and int(r["edge"]) == e and np.isnan(r["ncc"]) and np.isnan(r["ncc_second"]), r
    assert np.isnan(hb.edge_scores(x, 1, ep)).all() and hb.edge_scores(x, 1, ep).size == s - 1
    d = gpu.DeviceBuffer.from_numpy(0, x)
    assert hb.match_edges_device(d.ptr, length, ep).tobytes() == recs.tobytes()
    assert hb.match_edges_batch_device([d.ptr], [length], ep)[0].tobytes() == recs.tobytes()
    d.free()
    hb.close()


def test_log_n_applies_and_half_pipeline_does_not(gpu):
    s, length = 3000, 9000
    needle, pcm = er.case_signals(s, length, 61)
    x = er.downmix(pcm)
    h = gpu.HipConvolve(needle)
    ep = gpu.edge_params(64, 0, 0.05)
    base = [h.edge_scores(x, e, ep) for e in (0, 1)]
    recs = h.match_edges(x, ep)
    h.set_option("half_pipeline", 2)
    assert all(np.array_equal(a.view(np.uint32), h.edge_scores(x, e, ep).view(np.uint32)) for e, a in enumerate(base))
    h.set_option("half_pipeline", 0)
    before = gpu.get_option("score_norm")
    gpu.set_option("score_norm", 1)
    try:
        assert all(np.array_equal(a.view(np.uint32), h.edge_scores(x, e, ep).view(np.uint32)) for e, a in enumerate(base))
    finally:
        gpu.set_option("score_norm", before)
    h.set_option("log_n", 14)
    for edge in (er.HEAD, er.TAIL):
        eps, t = measured_eps(gpu, h, needle, x, edge)
        check_coarse(gpu, h, needle, x, t, edge, h.edge_scores(x, edge, ep), 64, 0.05, eps, dict(log_n=14, edge=edge))
    got = h.match_edges(x, ep)
    assert [int(r["start"]) for r in got] == [int(r["start"]) for r in recs]
    h.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    L = gpu.lib()
    needle = er.white(100, 71)
    x = er.white(400, 72)
    h = gpu.HipConvolve(needle)
    out = np.zeros(2, gpu.EDGE_HIT_DTYPE)
    sc = np.zeros(99, np.float32)
    n = C.c_size_t(0)
    ok = gpu.edge_params(8)
    inv = gpu.AM_ERR_INVALID_ARG

    def match(ep, hay=x.ctypes.data, length=400, fmt=0, o=out.ctypes.data):
        return L.am_match_edges(h._h, hay, length, fmt, C.byref(ep) if ep is not None else None, o)

    assert match(ok) == 0
    for ep, word in ((gpu.AmEdgeParams(8, 0, 0.05, 1), b"reserved"), (gpu.edge_params(0), b"min_overlap"),
                     (gpu.edge_params(8, 0, float("nan")), b"min_share"), (gpu.edge_params(8, 0, -0.01), b"min_share"),
                     (gpu.edge_params(8, 0, 1.5), b"min_share")):
        assert match(ep) == inv and word in L.am_last_error_string(), word
        assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 0, C.byref(ep), sc.ctypes.data, 99, C.byref(n)) == inv
        assert word in L.am_last_error_string(), word
    assert match(None) == inv and match(ok, hay=None) == inv and match(ok, o=None) == inv
    assert L.am_last_error_string() == b"null pointer"
    assert match(ok, fmt=7) == inv and b"format" in L.am_last_error_string()
    assert match(ok, length=0) == inv and b"len" in L.am_last_error_string()
    assert match(gpu.edge_params(8, 0, 0.0)) == 0 and match(gpu.edge_params(8, 0, 1.0)) == 0
    # am_edge_scores: the edge, the capacity, the pointers
    assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 2, C.byref(ok), sc.ctypes.data, 99, C.byref(n)) == inv
    assert b"edge" in L.am_last_error_string()
    assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 1, C.byref(ok), sc.ctypes.data, 98, C.byref(n)) == gpu.AM_ERR_CAPACITY
    assert n.value == 99
    assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 1, C.byref(ok), sc.ctypes.data, 99, None) == inv
    assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 1, C.byref(ok), None, 99, C.byref(n)) == inv
    assert L.am_edge_scores(h._h, x.ctypes.data, 0, 0, 1, C.byref(ok), sc.ctypes.data, 99, C.byref(n)) == inv
    assert L.am_edge_scores(h._h, x.ctypes.data, 400, 0, 1, C.byref(ok), sc.ctypes.data, 99, C.byref(n)) == 0 and n.value == 99
    # host memory where device memory is expected
    assert L.am_match_edges_device(h._h, x.ctypes.data, 400, 0, C.byref(ok), out.ctypes.data) == inv
    assert b"d_haystack" in L.am_last_error_string()
    assert L.am_edge_scores_device(h._h, x.ctypes.data, 400, 0, 0, C.byref(ok), sc.ctypes.data, 99, C.byref(n)) == inv
    assert b"d_haystack" in L.am_last_error_string()
    d = gpu.DeviceBuffer.from_numpy(0, x)
    ptrs = (C.c_void_p * 2)(d.ptr, x.ctypes.data)
    lens = (C.c_size_t * 2)(400, 400)
    out4 = np.zeros(4, gpu.EDGE_HIT_DTYPE)
    assert L.am_match_edges_batch_device(h._h, ptrs, lens, 2, 0, C.byref(ok), out4.ctypes.data) == inv
    assert b"haystack 1" in L.am_last_error_string()
    lens0 = (C.c_size_t * 2)(400, 0)
    ptrs2 = (C.c_void_p * 2)(d.ptr, d.ptr)
    assert L.am_match_edges_batch_device(h._h, ptrs2, lens0, 2, 0, C.byref(ok), out4.ctypes.data) == inv
    assert L.am_match_edges_batch_device(h._h, None, lens, 2, 0, C.byref(ok), out4.ctypes.data) == inv
    assert L.am_match_edges_batch_device(h._h, ptrs2, lens, 2, 0, C.byref(ok), None) == inv
    assert L.am_match_edges_batch_device(h._h, ptrs2, lens, 2, 0, C.byref(ok), out4.ctypes.data) == 0
    assert match(ok) == 0
    assert out4[:2].tobytes() == out4[2:].tobytes() == out.tobytes()
    d.free()
    h.close()
