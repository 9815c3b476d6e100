"""GPU tests of envelope matching (include/audiomatch.h, "envelope matching") against tests/envelope_ref.py.

Levels: a level may differ from the checker's only where the checker's 8 v lies within 1e-6 of a half-integer, and then
by 1 (the two transforms add in different orders); such cells are counted and may be at most 0.1 % of all cells.  Absent
frames equal exactly; the host and _device forms agree bit for bit.

Scores: z and qi bit for bit on designed uint16 matrices, at the correlation kernel's tile (AM_ENV_TILE places per
workgroup) and chunk (AM_ENV_CHUNK needle frames per step) edges, through its staged spans (B = 32: 256 frames per span)
and at the 32-bit sums' limit (512 chunks, then 64-bit).

Composition: the hit list equals the checker's pipeline on the checker's levels (on the device's levels where an exempt
cell exists), holds the plant, does not depend on score_norm and is profiled under `envelope`."""
import ctypes as C

import numpy as np
import pytest

import envelope_ref as er

pytestmark = pytest.mark.gpu

TILE, CHUNK = 512, 8


def test_exported_constants(gpu):
    assert (gpu.AM_ENV_TILE, gpu.AM_ENV_CHUNK) == (TILE, CHUNK)
    assert (gpu.AM_ENV_MAX_LEVEL, gpu.AM_ENV_ABSENT, gpu.AM_ENV_NO_Q, gpu.AM_ENV_STEPS_PER_DB) == (er.MAX_LEVEL, er.ABSENT, er.NO_Q, er.STEPS_PER_DB)
    assert (gpu.AM_ENV_MAX_PPM, gpu.AM_ENV_MAX_FRAMES, gpu.AM_ENV_MAX_NEEDLES, gpu.AM_ENV_MAX_STEPS) == (er.MAX_PPM, er.MAX_FRAMES, er.MAX_NEEDLES, er.MAX_STEPS)
    assert gpu.ENV_PICK_DTYPE == er.PICK_DTYPE and gpu.ENV_HIT_DTYPE == er.HIT_DTYPE


# ---- levels ----------------------------------------------------------------------------------------------------------
def band_edges(frame_log2, nb):
    top = (1 << frame_log2) // 2 + 1
    if nb == 1:
        return [0, top]                      # every bin
    if nb == 4:
        return [2, 5, 17, 18, top - 3]       # a band of one bin among wide ones
    return [1 + 3 * k for k in range(nb + 1)]


def signal(seed, n=40000):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.3 * np.sin(2 * np.pi * 0.031 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 7000.0)) + 0.05 * rng.standard_normal(n)
    x[12000:14000] = 0.0                     # digital silence: whole frames of zeros
    x[30000:30500] *= 1e-4
    return x.astype(np.float32)


def check_levels(got, ref_u, ref_ev, what):
    """got against the checker: (cells, exempt cells)."""
    assert got.shape == ref_u.shape and got.dtype == np.uint16, what
    assert np.array_equal(got == er.ABSENT, ref_u == er.ABSENT), what
    diff = got != ref_u
    if diff.any():
        assert np.all(er.near_half(ref_ev[diff])), (what, got[diff], ref_u[diff], ref_ev[diff])
        assert np.all(np.abs(got[diff].astype(np.int64) - ref_u[diff].astype(np.int64)) == 1), what
    return got.size, int(diff.sum())


def test_levels_against_checker(gpu):
    x = signal(31)
    xn = x.copy()
    xn[[5000, 5001, 26000]] = [np.inf, np.nan, -np.inf]           # absent frames
    s16 = er.to_s16_stereo(signal(32))
    s16[20000:20400] = 0
    cells = exempt = 0
    for name, sig in (("f32", x), ("f32 with non-finite samples", xn), ("s16 stereo", s16)):
        a, fmt, length = gpu._samples(sig)
        buf = gpu.DeviceBuffer.from_numpy(0, a)
        for lf in (8, 12):
            for nb in (1, 4, 32):
                edges = band_edges(lf, nb)
                ep = gpu.env_params(gpu.band_params(lf, edges), 80.0 if nb != 4 else 55.5)
                for d in (0.0, 40000.0, -250000.0):
                    what = (name, lf, nb, d)
                    ref_u, ref_ev = er.levels(sig, lf, edges, ep.floor_db, d)
                    host = gpu.envelope(sig, ep, d)
                    c, e = check_levels(host, ref_u, ref_ev, what)
                    cells, exempt = cells + c, exempt + e
                    dev = gpu.envelope_device(0, buf.ptr, length, ep, d, fmt)
                    assert er.same_bits(host, dev), what
        buf.free()
    print("levels: %d cells, %d within 1e-6 of a half-integer step and 1 off" % (cells, exempt))
    assert exempt <= cells // 1000
    assert np.any(gpu.envelope(xn, gpu.env_params(gpu.band_params(8, [1, 9, 60])), 0.0) == er.ABSENT)


def test_levels_of_short_signals(gpu):
    ep = gpu.env_params(gpu.band_params(8, [1, 9, 60, 129]))
    x = signal(33, 1000)
    assert gpu.envelope(x[:255], ep).shape == (3, 0) and gpu.envelope(x[:0], ep).shape == (3, 0)
    for n in (256, 383):
        got = gpu.envelope(x[:n], ep)
        assert got.shape == (3, 1) and np.array_equal(got, er.levels(x[:n], 8, [1, 9, 60, 129])[0])
    assert gpu.envelope(x[:384], ep).shape == (3, 2)
    assert gpu.envelope(x[:300], ep, -250000.0).shape == (3, 1)      # frames 171 apart: the second would end at 427
    assert gpu.envelope(np.zeros(2000, dtype=np.float32), ep).tolist() == np.zeros((3, 14), dtype=np.uint16).tolist()
    # capacity: nothing written, the count reported
    out = np.full(3 * 2, 7, dtype=np.uint16)
    n = C.c_size_t(0)
    assert gpu.lib().am_envelope(0, x.ctypes.data, 1000, 0, C.byref(ep), 0.0, out.ctypes.data, 2, C.byref(n)) == gpu.AM_ERR_CAPACITY
    assert n.value == 6 and np.all(out == 7)


# ---- scores ----------------------------------------------------------------------------------------------------------
def rand_levels(rng, nb, j):
    return rng.integers(0, er.MAX_LEVEL + 1, size=(nb, j)).astype(np.uint16)


def score_cases():
    rng = np.random.default_rng(41)
    cases = []
    hay = rand_levels(rng, 4, 311)
    cases.append(("Q = 1, J = 14", [rand_levels(rng, 4, 14)], hay))
    cases.append(("Q = 1, J = 45", [rand_levels(rng, 4, 45)], hay))
    five = [rand_levels(rng, 4, j) for j in (14, 45, 23, 31, 40)]
    five[2] = hay[:, 100:123].copy()                                  # a score of exactly 1
    cases.append(("Q = 5, different J", five, hay))
    for n_out in (TILE - 1, TILE, TILE + 1):
        cases.append(("n_out = %d" % n_out, [rand_levels(rng, 4, 14), rand_levels(rng, 4, 20)], rand_levels(rng, 4, n_out + 13)))
    cases.append(("J at the chunk size", [rand_levels(rng, 4, j) for j in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)], hay))
    cases.append(("J = 1: every score 0", [rand_levels(rng, 4, 1), rand_levels(rng, 4, 1)], hay))
    cases.append(("a constant haystack", [rand_levels(rng, 4, 14)], np.full((4, 100), 517, dtype=np.uint16)))
    cases.append(("a haystack of zeros and a flat needle", [np.full((4, 9), 3, dtype=np.uint16), rand_levels(rng, 4, 9)], np.zeros((4, 64), dtype=np.uint16)))
    e = hay.copy()
    e[:, 50] = er.ABSENT
    e[2, 200] = er.ABSENT                                             # one band of a frame marks the frame
    e[:, 310] = er.ABSENT
    cases.append(("absent frames at a window's first and last frame", [rand_levels(rng, 4, 14), rand_levels(rng, 4, 45)], e))
    n_abs = rand_levels(rng, 4, 14)
    n_abs[1, 13] = er.ABSENT
    cases.append(("an absent frame in one needle", [n_abs, rand_levels(rng, 4, 14)], hay))
    cases.append(("an absent frame in the only needle", [n_abs], hay))
    twin = rand_levels(rng, 4, 17)
    cases.append(("exact ties between two q", [rand_levels(rng, 4, 17), twin, rand_levels(rng, 4, 30), twin.copy()], hay))
    cases.append(("more needles than waves, ties across waves", [twin] * 9 + [hay[:, 7:24].copy()] * 2, hay))
    cases.append(("J > Jh for some q", [rand_levels(rng, 4, 400), rand_levels(rng, 4, 300), rand_levels(rng, 4, 312)], hay))
    cases.append(("J > Jh for every q", [rand_levels(rng, 4, 312)], hay))
    cases.append(("J = Jh", [rand_levels(rng, 4, 311)], hay))
    cases.append(("B = 1", [rand_levels(rng, 1, 33)], rand_levels(rng, 1, 700)))
    # B = 32: the staged rows hold 256 needle frames, longer needles are walked in spans
    h32 = rand_levels(rng, 32, 900)
    cases.append(("B = 32, spans", [rand_levels(rng, 32, j) for j in (255, 256, 257, 300, 513)] + [h32[:, 300:813].copy()], h32))
    return cases


def overflow_cases():
    """Every level 1023 but one per band: sums that an int32 or f32 accumulator loses."""
    out = []
    for nb, extra in ((32, 300), (1, 100)):                           # (B = 1: one span of 2048 chunks, four 32-bit rounds)
        j = er.MAX_FRAMES
        n = np.full((nb, j), er.MAX_LEVEL, dtype=np.uint16)
        e = np.full((nb, j + extra), er.MAX_LEVEL, dtype=np.uint16)
        for b in range(nb):
            n[b, (b * 509 + 3) % j] = 0
            e[b, 11 + 7 * b] = 1
        out.append(("the overflow edge, B = %d" % nb, [n], e))
    return out


def run_scores(gpu, name, needles, hay):
    z_ref, qi_ref = er.scores(needles, hay)
    z, qi = gpu.envelope_scores(needles, hay)
    assert er.same_bits(z, z_ref) and np.array_equal(qi, qi_ref), (name, "host form", z[:8], z_ref[:8], qi[:8], qi_ref[:8])
    _, frames, bank = gpu._env_bank(needles)
    dn, dh = gpu.DeviceBuffer.from_numpy(0, bank), gpu.DeviceBuffer.from_numpy(0, np.ascontiguousarray(hay))
    zd, qd = gpu.envelope_scores_device(0, dn.ptr, frames, hay.shape[0], dh.ptr, hay.shape[1])
    dn.free()
    dh.free()
    assert er.same_bits(zd, z_ref) and np.array_equal(qd, qi_ref), (name, "device form")
    return z_ref, qi_ref


def test_scores_bit_for_bit(gpu):
    for name, needles, hay in score_cases():
        z, qi = run_scores(gpu, name, needles, hay)
        if name.startswith("J = 1") or name.startswith("a constant") or name.startswith("a haystack of zeros"):
            assert z.size and not z.any() and not qi.any(), name
        if name == "exact ties between two q":
            assert np.any(qi == 1) and not np.any(qi == 3), name
        if name.startswith("more needles"):
            assert set(qi.tolist()) <= {0, 9} and qi[7] == 9 and z[7] == 1.0, name
        if name.startswith("J > Jh for some"):
            assert z.size == 12 and set(qi.tolist()) == {1}, name
        if name.startswith("J > Jh for every"):
            assert z.size == 0, name
        if name == "an absent frame in the only needle":
            assert np.all(np.isnan(z)) and np.all(qi == er.NO_Q), name
        if name.startswith("absent frames at"):
            assert np.isnan(z[50]) and np.isnan(z[37]) and not np.isnan(z[36]) and not np.isnan(z[51]) and np.isnan(z[297]), name
            assert qi[6] == 0 and qi[266] == 0 and np.any(qi == 1)   # there the long needle's windows reach an absent frame, the short one's do not


def test_scores_at_the_overflow_edge(gpu):
    for name, needles, hay in overflow_cases():
        z, _ = run_scores(gpu, name, needles, hay)
        assert np.all(np.isfinite(z)) and np.ptp(z) > 0, name


def test_scores_capacity_and_arguments(gpu):
    rng = np.random.default_rng(42)
    L = gpu.lib()
    hay = rand_levels(rng, 4, 100)
    needles = [rand_levels(rng, 4, 14), rand_levels(rng, 4, 20)]
    z_ref, qi_ref = er.scores(needles, hay)
    _, frames, bank = gpu._env_bank(needles)
    zz, qq, n = np.zeros(87, np.float32), np.zeros(87, np.uint32), C.c_size_t(0)

    def call(bank=bank, frames=frames, nq=2, nb=4, hay=hay, jh=100, cap=87, z=zz, qi=qq):
        return L.am_envelope_scores(0, bank.ctypes.data if bank is not None else None, frames.ctypes.data, nq, nb,
                                    hay.ctypes.data if hay is not None else None, jh, z.ctypes.data if z is not None else None,
                                    qi.ctypes.data, cap, C.byref(n))
    assert call(cap=10) == gpu.AM_ERR_CAPACITY and n.value == 87                    # what fits is filled, the count reported
    assert er.same_bits(zz[:10], z_ref[:10]) and np.array_equal(qq[:10], qi_ref[:10]) and not zz[10:].any()
    assert call() == 0 and n.value == 87 and er.same_bits(zz, z_ref)
    for kw, word in ((dict(nq=0), b"n_needles"), (dict(nq=258), b"n_needles"), (dict(nb=0), b"n_bands"), (dict(nb=33), b"n_bands"),
                     (dict(frames=np.array([14, 0], np.uint32)), b"frames[1]"), (dict(frames=np.array([16385, 20], np.uint32)), b"frames[0]"),
                     (dict(jh=(1 << 24) + 1), b"hay_frames"), (dict(bank=None), b"null"), (dict(hay=None), b"null"), (dict(z=None), b"null")):
        assert call(**kw) == gpu.AM_ERR_INVALID_ARG and word in L.am_last_error_string(), (kw, L.am_last_error_string())
    bad = bank.copy()
    bad[4 * 14 + 5] = 1024
    assert call(bank=bad) == gpu.AM_ERR_INVALID_ARG and b"matrix 1" in L.am_last_error_string()
    bad_hay = hay.copy()
    bad_hay[3, 99] = 0xFFFE
    assert call(hay=bad_hay) == gpu.AM_ERR_INVALID_ARG and b"hay" in L.am_last_error_string()
    assert L.am_envelope_scores_device(0, bank.ctypes.data, frames.ctypes.data, 2, 4, hay.ctypes.data, 100, zz.ctypes.data, qq.ctypes.data, 87,
                                       C.byref(n)) == gpu.AM_ERR_INVALID_ARG and b"d_needles" in L.am_last_error_string()


# ---- composition -----------------------------------------------------------------------------------------------------
SR, LF, NB, K, MAX_PPM, MIN_SCORE = 16000, 9, 6, 8, 40000.0, 0.3


@pytest.fixture(scope="module")
def design(gpu):
    needle, hay, at = er.composition_design(SR)
    edges = er.edges_log(SR, LF, 150.0, 6000.0, NB)
    ep = gpu.env_params(gpu.band_edges_log(SR, LF, 150.0, 6000.0, NB))
    assert list(ep.bands.edges[:NB + 1]) == edges
    grid = gpu.env_grid(MAX_PPM, K)
    drifts = er.grid_drifts(0.0, MAX_PPM, K)
    assert np.array_equal(gpu.env_grid_drifts(grid), np.array(drifts))
    algo = gpu.HipConvolve(needle)
    yield dict(needle=needle, hay=hay, at=at, edges=edges, ep=ep, grid=grid, drifts=drifts, algo=algo)
    algo.close()


def reference_hits(gpu, d, hay):
    """The checker's pipeline on the checker's levels -- on the device's where they differ in exempt cells (counted)."""
    needle, edges, ep = d["needle"], d["edges"], d["ep"]
    exempt, nl = 0, []
    for dq in d["drifts"]:
        ref_u, ref_ev = er.levels(needle, LF, edges, 80.0, dq)
        got = gpu.envelope(needle, ep, dq)
        exempt += check_levels(got, ref_u, ref_ev, ("needle", dq))[1]
        nl.append(got)
    ref_u, ref_ev = er.levels(hay, LF, edges, 80.0, 0.0)
    hl = gpu.envelope(hay, ep, 0.0)
    exempt += check_levels(hl, ref_u, ref_ev, "haystack")[1]
    n_hay = hay.size // 2 if hay.dtype == np.int16 else hay.size
    return er.hits_from(nl, hl, d["drifts"], needle.size, n_hay, LF, MIN_SCORE)[0], exempt


def test_composition_equals_the_checker_and_holds_the_plant(gpu, design):
    d = design
    ref, exempt = reference_hits(gpu, d, d["hay"])
    print("composition: %d exempt level cells; hits %s" % (exempt, [(int(h["start"]), float(h["drift_ppm"]), float(h["score"])) for h in ref]))
    got = d["algo"].match_envelope(d["hay"], d["ep"], d["grid"], MIN_SCORE)
    assert er.same_bits(got, ref), (got, ref)
    buf = gpu.DeviceBuffer.from_numpy(0, d["hay"])
    with gpu.Profile(0) as prof:
        dev = d["algo"].match_envelope_device(buf.ptr, d["hay"].size, d["ep"], d["grid"], MIN_SCORE)
    assert er.same_bits(dev, ref)
    ms, launches = prof.query("envelope")
    parts = [prof.query("envelope_" + k) for k in ("frames", "prefix", "correlate")]
    # (counted per bracketed group of launches: the needle's and the haystack's levels; bank, block sums and prefix; the correlation)
    assert launches == 4 and [p[1] for p in parts] == [2, 1, 1] and ms > 0 and abs(ms - sum(p[0] for p in parts)) < 1e-9
    assert prof.query("k1_cols_fwd")[1] == 0 and prof.query("other")[1] == 0       # no waveform pass
    # the plant: +3 % at d["at"], found within 4 frames; the drift of a 3 s needle is good to a grid step or two
    H = 1 << (LF - 1)
    best = max(got, key=lambda h: float(h["score"]))
    assert abs(int(best["start"]) - d["at"]) <= 4 * H and abs(float(best["drift_ppm"]) - 30000.0) <= 2 * MAX_PPM / K
    assert int(best["length"]) == er.llround(d["needle"].size * (1.0 + float(best["drift_ppm"]) * 1e-6))
    # the waveform matcher does not see it
    ncc = gpu.HipConvolve(d["needle"], score_norm=True)
    assert max((p.height for p in ncc.match_best(d["hay"], 1)), default=0.0) < 0.3
    ncc.close()
    # capacity
    out, n = np.zeros(1, gpu.ENV_HIT_DTYPE), C.c_size_t(0)
    assert gpu.lib().am_match_envelope_device(d["algo"]._h, buf.ptr, d["hay"].size, 0, C.byref(d["ep"]), C.byref(d["grid"]), MIN_SCORE,
                                              out.ctypes.data, 1, C.byref(n)) == gpu.AM_ERR_CAPACITY
    assert n.value == ref.size >= 2 and er.same_bits(out, ref[:1])
    buf.free()


def test_composition_s16_stereo_and_options(gpu, design):
    d = design
    f32 = d["algo"].match_envelope(d["hay"], d["ep"], d["grid"], MIN_SCORE)
    s16 = er.to_s16_stereo(d["hay"])
    ref, _ = reference_hits(gpu, d, s16)
    got = d["algo"].match_envelope(s16, d["ep"], d["grid"], MIN_SCORE)
    assert er.same_bits(got, ref)
    H = 1 << (LF - 1)
    assert got.size == f32.size and np.all(np.abs(got["start"].astype(np.int64) - f32["start"].astype(np.int64)) <= H // 2)
    assert np.array_equal(got["q"], f32["q"])
    try:
        gpu.set_option("score_norm", 1)
        gpu.set_option("half_pipeline", 1)
        assert er.same_bits(d["algo"].match_envelope(d["hay"], d["ep"], d["grid"], MIN_SCORE), f32)
    finally:
        gpu.set_option("score_norm", 0)
        gpu.set_option("half_pipeline", 0)
    # a haystack shorter than a frame, and one with fewer frames than the needle's envelopes: no hits
    assert d["algo"].match_envelope(d["hay"][:100], d["ep"], d["grid"], MIN_SCORE).size == 0
    assert d["algo"].match_envelope(d["hay"][:20000], d["ep"], d["grid"], MIN_SCORE).size == 0
    # K = 0: the one drift of the centre
    one = d["algo"].match_envelope(d["hay"], d["ep"], gpu.env_grid(0.0, 0, 30000.0), MIN_SCORE)
    ref1 = er.match(d["needle"], d["hay"], LF, d["edges"], 80.0, 30000.0, 0.0, 0, MIN_SCORE)[0]
    assert er.same_bits(one, ref1) and one.size >= 1 and np.all(one["q"] == 0)


def test_invalid_arguments(gpu, design):
    d = design
    L = gpu.lib()
    out, n = np.zeros(8, gpu.ENV_HIT_DTYPE), C.c_size_t(0)
    hay = d["hay"]

    def call(h=d["algo"]._h, ptr=hay.ctypes.data, length=hay.size, fmt=0, ep=d["ep"], grid=d["grid"], ms=MIN_SCORE, o=out.ctypes.data, cap=8, np_=C.byref(n)):
        return L.am_match_envelope(h, ptr, length, fmt, C.byref(ep) if ep is not None else None, C.byref(grid) if grid is not None else None,
                                   ms, o, cap, np_)

    def ep_with(**kw):
        ep = gpu.env_params(gpu.band_edges_log(SR, LF, 150.0, 6000.0, NB))
        for k, v in kw.items():
            if k in ("frame_log2", "n_bands"):
                setattr(ep.bands, k, v)
            else:
                setattr(ep, k, v)
        return ep
    cases = [(dict(h=None), b"needle"), (dict(ptr=None), b"null"), (dict(ep=None), b"null"), (dict(grid=None), b"null"), (dict(o=None), b"null"),
             (dict(np_=None), b"null"), (dict(fmt=7), b"format"), (dict(ms=float("nan")), b"min_score"), (dict(length=(1 << 31) + 1), b"AM_ENV_MAX_LEN"),
             (dict(ep=ep_with(reserved=5)), b"reserved"), (dict(ep=ep_with(floor_db=float("nan"))), b"floor_db"), (dict(ep=ep_with(floor_db=201.0)), b"floor_db"),
             (dict(ep=ep_with(frame_log2=7)), b"frame_log2"), (dict(ep=ep_with(n_bands=0)), b"n_bands"), (dict(ep=ep_with(n_bands=33)), b"n_bands"),
             (dict(grid=gpu.AmEnvGrid(0.0, 1000.0, 129, 0)), b"steps"), (dict(grid=gpu.AmEnvGrid(0.0, 1000.0, 2, 1)), b"reserved"),
             (dict(grid=gpu.AmEnvGrid(0.0, -1.0, 2, 0)), b"max_ppm"), (dict(grid=gpu.AmEnvGrid(0.0, 0.0, 2, 0)), b"max_ppm"),
             (dict(grid=gpu.AmEnvGrid(-200000.0, 50001.0, 2, 0)), b"AM_ENV_MAX_PPM"), (dict(grid=gpu.AmEnvGrid(float("nan"), 10.0, 2, 0)), b"AM_ENV_MAX_PPM")]
    for kw, word in cases:
        assert call(**kw) == gpu.AM_ERR_INVALID_ARG and word in L.am_last_error_string(), (kw, L.am_last_error_string())
    bad_edges = gpu.env_params(gpu.band_params(LF, [5, 9, 9, 30]))
    assert call(ep=bad_edges) == gpu.AM_ERR_INVALID_ARG and b"edges" in L.am_last_error_string()
    short = gpu.HipConvolve(d["needle"][:511])      # shorter than a frame (the first frame starts at 0 at every rate)
    assert call(h=short._h) == gpu.AM_ERR_INVALID_ARG and b"holds no frame" in L.am_last_error_string() and b"frame_log2" in L.am_last_error_string()
    short.close()


def test_needle_frame_limits(gpu):
    L = gpu.lib()
    rng = np.random.default_rng(43)
    out, n = np.zeros(8, gpu.ENV_HIT_DTYPE), C.c_size_t(0)
    hay = rng.standard_normal(5000).astype(np.float32)
    ep = gpu.env_params(gpu.band_params(8, [1, 9, 60]))
    grid = gpu.env_grid(250000.0, 1)

    def call(algo, ep=ep, grid=grid):
        return L.am_match_envelope(algo._h, hay.ctypes.data, hay.size, 0, C.byref(ep), C.byref(grid), 0.5, out.ctypes.data, 8, C.byref(n))
    tiny = gpu.HipConvolve(rng.standard_normal(255).astype(np.float32))
    assert call(tiny) == gpu.AM_ERR_INVALID_ARG and b"holds no frame" in L.am_last_error_string() and b"frame_log2" in L.am_last_error_string()
    tiny.close()
    one = gpu.HipConvolve(hay[1000:1256].copy())                                       # exactly one frame at every rate: J = 1, every score 0
    assert call(one) == 0 and n.value == 0
    one.close()
    # more than AM_ENV_MAX_FRAMES frames: 16385 frames of hop 128 need 128 * 16384 + 256 samples at 0 ppm
    long_needle = gpu.HipConvolve(np.zeros(128 * 16384 + 256, dtype=np.float32) + 0.25)
    assert call(long_needle, grid=gpu.env_grid(0.0, 0)) == gpu.AM_ERR_INVALID_ARG
    assert b"AM_ENV_MAX_FRAMES" in L.am_last_error_string() and b"larger frame_log2" in L.am_last_error_string()
    long_needle.close()
    fits = gpu.HipConvolve(np.zeros(128 * 16384 + 255, dtype=np.float32) + 0.25)
    assert call(fits, grid=gpu.env_grid(0.0, 0)) == 0 and n.value == 0                 # 16384 frames: allowed; the haystack is shorter
    fits.close()
