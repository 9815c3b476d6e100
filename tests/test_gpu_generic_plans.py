"""Every score of the generic plans (N = 2^10 .. 2^20) against the CPU oracle.  These are the transform sizes of every
problem whose span is at most 2^19 samples and of every forced log_n below 21, and they run other kernels than the
register plans of test_gpu_plan_geometry.py: the in-LDS radix-4 column kernels (k1_cols_fwd_gen, k3_cols_inv_gen) with
32 rows up to 2^18, 64 on 2^19 (the only even column transform, no radix-2 stage) and 128 on 2^20; the in-LDS row
kernel (k2_rows_gen) with rows of 2^5 .. 2^12 points up to 2^17; and from 2^18 up the generic columns around the
8192-point register row kernel.

The cases are those of the block layout: a raw hop of 2 and of 3, raw hops up to 8191, the hop floored to the score
tile from 8192 on, a block that reads more than it emits, a ragged last block, a last pair with an empty second block,
launches whose first pair is not pair 0, the virtual zeros of Full and Same, forced tiny needles -- and combs, whose
tones sit on chosen rows of the work matrix, so that a wrong twiddle shows at 1e-4 on 2^20 as it does on 2^10 (white
noise spreads over all N bins: one wrong bin moves a score by about 1 / sqrt(s * N), 1e-6 on 2^20).

The layout is computed here (plan_geometry_ref.py) only to choose lengths and to word failures; every expectation is
the oracle's, whose own scores at these shapes test_plan_geometry_host.py holds to plain f64 dot products."""
import time

import numpy as np
import pytest

import plan_geometry_ref as R
from plan_geometry_ref import TOL

pytestmark = pytest.mark.gpu

FULL, SAME, VALID = R.MODES
PLANS = range(10, 21)

# more than 64 pairs of a hop of 2 or 3: the default pairs_per_group of 64 splits the call into two launches
MANY_PAIRS = 2 * 64
MANY_STRIDE = 16        # ... with a plant on every 16th seam (the last one on the first block of the second launch)

_REF = {}


def reference(oracle, log_n, s, count, n_blocks=6, stride=1):
    """(needle, within, {mode: scores}) of the case whose Valid output has `count` scores; never written to.  One
    needle's references are kept at a time (its cases follow each other)."""
    key = (log_n, s, count, n_blocks, stride)
    if key not in _REF:
        for k in [k for k in _REF if k[:2] != key[:2]]:
            del _REF[k]
        needle, within = R.signals(oracle, log_n, s, count + s - 1, R.hop_of(log_n, s), n_blocks, stride)
        exp = R.all_modes(oracle, within, needle)
        for a in (needle, within, *exp.values()):
            a.flags.writeable = False
        _REF[key] = (needle, within, exp)
    return _REF[key]


def forced(gpu, needle, log_n):
    algo = gpu.HipConvolve(needle)
    algo.set_option("log_n", log_n)      # per handle: gone with the handle
    assert algo.get_option("log_n") == log_n
    return algo


def single_block_needle(log_n):
    """A raw hop of N / 8 up to 2^15, a floored one from 2^16 up."""
    n = 1 << log_n
    return n - n // 8 + 1


# ---------------------------------------------------------------------------
# a. every score of level 1
# ---------------------------------------------------------------------------
def level1_cases():
    """(log_n, s, count, mode, ref_count, n_blocks, stride): `count` Valid scores, i.e. a `within` of count + s - 1
    samples, in `mode`; the reference is that of the needle's `within` of ref_count Valid scores with the
    plants(hop, n_blocks, stride)."""
    cases = []
    for log_n in PLANS:
        for s in R.generic_needle_lengths(log_n):
            hop = R.hop_of(log_n, s)
            counts = sorted(set(R.score_counts(hop)))        # (with a hop of 2, 3 * hop + 1 is 4 * hop - 1)
            longest = max(counts)
            cases += [(log_n, s, c, VALID, longest, 6, 1) for c in counts]
            cases += [(log_n, s, c, m, c, 6, 1) for c in (5 * hop + 2, 4 * hop + 1) for m in (SAME, FULL)]
            if hop in (2, 3):
                many = MANY_PAIRS * hop + 3
                cases += [(log_n, s, many, VALID, many, MANY_PAIRS + 2, MANY_STRIDE)]
        # fewer than `hop` scores: a single block, so the second half of pair 0 is empty
        s = single_block_needle(log_n)
        few = R.hop_of(log_n, s) - 7
        cases += [(log_n, s, few, VALID, few, 6, 1)]
    return cases


def case_id(case):
    log_n, s, count, mode = case[:4]
    hop = R.hop_of(log_n, s)
    q, r = divmod(count + hop // 2, hop)
    r -= hop // 2
    return "2^%d-s=N-%d-hop%d-n=%dhop%+d-%s" % (log_n, (1 << log_n) - s, hop, q, r, R.MODE_NAMES[mode])


def test_the_cases_cover_every_plan_and_regime():
    """What the parametrisation promises: every log_n from 10 to 20; on each a hop of 2 and of 3 with more than 64
    pairs, a single block; from 2^14 up the raw hop 8191, the floored hops 8192 (raw 8192 and raw 9001)."""
    cases = level1_cases()
    assert len({case_id(c) for c in cases}) == len(cases)
    for log_n in PLANS:
        mine = [c for c in cases if c[0] == log_n]
        hops = {R.hop_of(log_n, c[1]) for c in mine}
        assert {2, 3} <= hops and all(any(R.hop_of(log_n, c[1]) == h and -(-c[2] // h) > 2 * 64 for c in mine) for h in (2, 3))
        assert any(c[2] < R.hop_of(log_n, c[1]) for c in mine)
        assert {m for c in mine for m in c[3:4]} == set(R.MODES)
        if (1 << log_n) > 5000:
            assert 5000 in hops
        if log_n >= 14:
            n = 1 << log_n
            assert {8191, 8192} <= hops and R.hop_of(log_n, n - 9000) == 8192 and n - 9000 in {c[1] for c in mine}
        if log_n in (14, 20):
            assert max(hops) == 3 * (1 << log_n) // 4


@pytest.mark.parametrize("case", level1_cases(), ids=case_id)
def test_every_score_of_a_generic_plan(gpu, oracle, case):
    log_n, s, count, mode, ref_count, n_blocks, stride = case
    t0 = time.perf_counter()
    hop = R.hop_of(log_n, s)
    needle, within, exp = reference(oracle, log_n, s, ref_count, n_blocks, stride)
    expect = exp[VALID][:count] if mode == VALID else exp[mode]
    assert mode == VALID or count == ref_count
    if count >= 2 * hop:
        assert float(exp[VALID].max()) > 0.5     # the plants: scores of order 1 on the seams
    t1 = time.perf_counter()
    algo = forced(gpu, needle, log_n)
    try:
        got = algo.correlate_with_sample(within[:count + s - 1], gpu.Mode(mode), True)
    finally:
        algo.close()
    t2 = time.perf_counter()
    worst = R.check_scores(got, expect, hop, case_id(case))
    print("%s: %d scores, %d blocks, max error %.3g; reference %.2f s, library %.2f s" % (
        case_id(case), got.size, -(-got.size // hop), worst, t1 - t0, t2 - t1))


# ---------------------------------------------------------------------------
# b. combs: a tone on every row of the work matrix
# ---------------------------------------------------------------------------
def comb_cases():
    """(log_n, which, s, blocks): every comb of every plan with the needle of the first floored hop (8192; a raw
    hop below 2^14), five blocks; from 2^14 up also with the large-hop needle of N / 4 + 1 samples, one pair.  A block
    of 8192 scores is at most two of the 32 rows K3's column transform puts out on 2^17 and only row 0 from 2^18 up,
    and row 0 is the plain sum of its inputs: no twiddle of that transform can show in it.  A hop of three quarters
    of N keeps three quarters of the rows."""
    cases = []
    for log_n in PLANS:
        for which in range(R.comb_count(log_n)):
            cases.append((log_n, which, R.comb_needle_length(log_n), 5))
            if log_n >= 14:
                cases.append((log_n, which, (1 << log_n) // 4 + 1, 2))
    return cases


def comb_id(case):
    log_n, which, s, blocks = case
    return "2^%d-comb%d-hop%d-%dblocks" % (log_n, which, R.hop_of(log_n, s), blocks)


@pytest.mark.parametrize("case", comb_cases(), ids=comb_id)
def test_comb_on_every_row(gpu, oracle, case):
    """Valid scores of 16 tones of amplitude 1/16 on the bins k1 + N1 * k2 of rows k1 = 16 * which .. + 15."""
    log_n, which, s, blocks = case
    t0 = time.perf_counter()
    hop = R.hop_of(log_n, s)
    count = blocks * hop
    needle, within = R.comb_signals(log_n, s, count + s - 1, which)
    expect = oracle.correlate(within, needle, oracle.MODE_VALID, oracle.SCALE_LIB)
    assert expect.size == count and abs(float(expect[0]) - 1.0) < 1e-6     # the needle on itself
    t1 = time.perf_counter()
    algo = forced(gpu, needle, log_n)
    try:
        got = algo.correlate_with_sample(within, gpu.Mode.Valid, True)
    finally:
        algo.close()
    t2 = time.perf_counter()
    what = "2^%d comb %d (rows %d..%d of %d), hop %d" % (log_n, which, 16 * which, 16 * which + 15, R.n1_of(log_n), hop)
    worst = R.check_scores(got, expect, hop, what)
    print("%s: %d scores, max error %.3g; reference %.2f s, library %.2f s" % (what, got.size, worst, t1 - t0, t2 - t1))


# ---------------------------------------------------------------------------
# c. forced tiny needles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
@pytest.mark.parametrize("s", [1, 2, 65])
@pytest.mark.parametrize("log_n", [10, 14])
def test_forced_tiny_needle(gpu, oracle, log_n, s, mode):
    """A forced log_n bypasses direct summation: hop = N - s + 1, so N itself for one sample (no score of a block is
    discarded), floored on 2^14.  Three blocks and five scores; the tolerance is relative to the largest score, as in
    test_gpu_correlate.py's test_modes_and_scales, because LIB scaling by the energy of a sample or two is not of
    order 1."""
    hop = R.hop_of(log_n, s)
    assert hop == {10: (1 << 10) - s + 1, 14: ((1 << 14) - s + 1) // 1024 * 1024}[log_n]
    count = 3 * hop + 5
    needle, within = R.signals(oracle, log_n, s, count + s - 1, hop)
    expect = oracle.correlate(within, needle, mode, oracle.SCALE_LIB)
    ref = max(1.0, float(np.abs(expect).max()))
    algo = forced(gpu, needle, log_n)
    try:
        got = algo.correlate_with_sample(within, gpu.Mode(mode), True)
    finally:
        algo.close()
    assert got.dtype == np.float32 and got.shape == expect.shape
    err = np.abs(got.astype(np.float64) - expect.astype(np.float64))
    err[~np.isfinite(err)] = np.inf
    i = int(np.argmax(err))
    print("2^%d s=%d %s: hop %d, %d scores, largest %.3g, max error %.3g of it" % (
        log_n, s, R.MODE_NAMES[mode], hop, got.size, ref, err[i] / ref))
    assert err[i] / ref < TOL, "max error %.3g (of a largest score of %.3g) at %s: got %r, expected %r" % (
        err[i], ref, R.place(i, hop), float(got[i]), float(expect[i]))


# ---------------------------------------------------------------------------
# d. one haystack over several launches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,back", [(12, 1000), (19, 4999), (20, 4999)], ids=["2^12", "2^19", "2^20"])
def test_one_haystack_over_several_launches(gpu, oracle, log_n, back):
    """pairs_per_group caps the pairs of a launch, so 1 and 2 run the later pairs with first_pair != 0: the same
    scores bit for bit as one launch, and as many K1 launches as the layout computed here needs."""
    s = (1 << log_n) - back
    hop = R.hop_of(log_n, s)
    count = 9 * hop + 3
    npairs = (-(-count // hop) + 1) // 2
    assert npairs == 5 and hop == back + 1
    needle, within, exp = reference(oracle, log_n, s, count, 10, 1)
    default = gpu.get_option("pairs_per_group")
    mask, every = gpu.get_option("profile_mask"), gpu.get_option("profile_every")
    assert default == 64
    algo = forced(gpu, needle, log_n)
    got, launches = {}, {}
    try:
        gpu.set_option("profile_mask", -1)
        gpu.set_option("profile_every", 1)
        for ppg in (default, 1, 2):
            gpu.set_option("pairs_per_group", ppg)
            with gpu.Profile(0) as prof:
                got[ppg] = algo.correlate_with_sample(within, gpu.Mode.Valid, True)
                launches[ppg] = prof.query("k1_cols_fwd")[1]
    finally:
        gpu.set_option("pairs_per_group", default)
        gpu.set_option("profile_mask", mask)
        gpu.set_option("profile_every", every)
        algo.close()
    print("2^%d, hop %d, %d scores, %d pairs: K1 launches %r" % (log_n, hop, count, npairs, launches))
    R.check_scores(got[default], exp[VALID], hop, "2^%d, pairs_per_group %d" % (log_n, default))
    for ppg in (1, 2):
        differ = np.flatnonzero(got[ppg].view(np.uint32) != got[default].view(np.uint32))
        assert np.array_equal(got[ppg], got[default]) and differ.size == 0, "pairs_per_group %d: %d scores differ, the first at %s" % (
            ppg, differ.size, R.place(int(differ[0]), hop))
    assert launches == {default: 1, 1: npairs, 2: -(-npairs // 2)}


# ---------------------------------------------------------------------------
# e. the half pipeline is inert on these plans
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [13, 19])
def test_half_pipeline_is_inert(gpu, oracle, log_n):
    """half_scale() gives level 0 on every plan that is not 256- or 512-row: "half_pipeline" 1 and 2 on the handle
    give the bits of 0.  On 2^19 this pins that the register row kernel of a mixed plan is never handed a
    half-precision matrix that the generic K1 did not write."""
    s = (1 << log_n) - 4999
    hop = R.hop_of(log_n, s)
    count = 4 * hop + 1
    needle, within, exp = reference(oracle, log_n, s, count)
    algo = forced(gpu, needle, log_n)
    got = {}
    try:
        for level in (0, 1, 2, 0):
            algo.set_option("half_pipeline", level)
            assert algo.get_option("half_pipeline") == level
            out = algo.correlate_with_sample(within, gpu.Mode.Valid, True)
            assert level not in got or np.array_equal(out.view(np.uint32), got[level].view(np.uint32))
            got[level] = out
    finally:
        algo.close()
    worst = R.check_scores(got[0], exp[VALID], hop, "2^%d, half_pipeline 0" % log_n)
    print("2^%d, hop %d: max error %.3g" % (log_n, hop, worst))
    for level in (1, 2):
        differ = np.flatnonzero(got[level].view(np.uint32) != got[0].view(np.uint32))
        assert differ.size == 0, "half_pipeline %d: %d scores differ from level 0, the first at %s" % (
            level, differ.size, R.place(int(differ[0]), hop))


# ---------------------------------------------------------------------------
# f. level 2 on the same geometry, both sample formats
# ---------------------------------------------------------------------------
def check_peaks(got, exp, tol, what):
    assert [(g.start, g.end) for g in got] == [(e[0], e[1]) for e in exp], what
    worst = 0.0
    for g, e in zip(got, exp):
        worst = max(worst, abs(g.height - e[2]), abs(g.prominence - e[3]))
        assert abs(g.height - e[2]) < tol and abs(g.prominence - e[3]) < tol, (what, g, e)
    return worst


@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("log_n", [17, 19, 20], ids=["2^17", "2^19", "2^20"])
def test_hits_on_the_seams_level2(gpu, oracle, log_n, d):
    """One plan of each column length (32, 64 and 128 rows), forced on the handle: a needle of 20 000 samples in a
    haystack of five blocks and 3000 samples.  Hits at hop + d, 2 * hop + d and at the last offset len - s, f32 and
    i16 stereo, twice each.  The chunks (10 s at 8 kHz) are no multiple of the hop, so chunk edges fall inside
    blocks."""
    sr, s = 8000, 20000
    hop = R.hop_of(log_n, s)
    length = 5 * hop + 3000
    needle = oracle.synth_uniform(4200 + 8 * log_n + d, 0, 0, s)
    hay = oracle.synth_uniform(4200 + 8 * log_n + d, 1, 0, length)
    for p, gain in [(hop + d, 1.0), (2 * hop + d, 0.9), (length - s, 0.8)]:
        hay[p:p + s] += np.float32(gain) * needle
    cfg = gpu.Config(chunk_size_s=10.0, overlap_length_s=s / sr, distance_s=5.0, prominence=0.13)
    p = cfg.params(sr, gpu.Scale.LIB)
    assert p.overlap == s
    edges = range(p.chunk, length, p.chunk)
    assert len(edges) >= 4 and all(e % hop for e in edges)
    lr = np.clip(np.round(np.repeat(hay, 2) * 20000.0), -32768, 32767).astype(np.int16)
    nlr = np.clip(np.round(np.repeat(needle, 2) * 20000.0), -32768, 32767).astype(np.int16)
    m_needle, m_hay = oracle.pcm_s16_stereo_to_mono(nlr), oracle.pcm_s16_stereo_to_mono(lr)
    exp = oracle.calc_chunks(sr, hay, needle, p.chunk, p.overlap, 0.13, p.min_distance, 5.0)
    exp16 = oracle.calc_chunks(sr, m_hay, m_needle, p.chunk, p.overlap, 0.13, p.min_distance, 5.0)
    assert {hop + d, 2 * hop + d} <= {e[0] for e in exp} and [e[0] for e in exp] == [e[0] for e in exp16]
    algo, a16 = gpu.HipConvolve(needle), gpu.HipConvolve.from_pcm16(nlr)
    worst = [0.0, 0.0]
    try:
        for a in (algo, a16):
            a.set_option("log_n", log_n)
            assert a.get_option("log_n") == log_n
        for call in range(2):
            got, got16 = algo.match(hay, p), a16.match_pcm16(lr, p)
            worst[0] = max(worst[0], check_peaks(got, exp, TOL, ("f32", log_n, d, call)))
            worst[1] = max(worst[1], check_peaks(got16, exp16, 3 * TOL, ("pcm16", log_n, d, call)))
    finally:
        algo.close()
        a16.close()
    print("2^%d d=%+d: hop %d, %d samples, hits at %r; max error f32 %.3g, pcm16 %.3g" % (
        log_n, d, hop, length, [e[0] for e in exp], worst[0], worst[1]))
