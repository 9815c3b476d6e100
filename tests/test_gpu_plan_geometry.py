"""Every score of the register-kernel plans (N = 2^21, 2^22, 2^23) against the CPU oracle where their block geometry
has its special cases: two blocks packed into one complex transform, virtual zeros in front of the source (Full, Same)
and behind it, a raw (odd or even) hop below 8192 scores and a hop floored to the score tile from there on, the 8-byte
and the scalar score stores, a ragged last block, a last pair with an empty second block, launches whose first pair is
not pair 0 -- and level 2 (f32 and i16 stereo ingest) with hits on the seams of the same layout.

The layout is computed here (plan_geometry_ref.py) only to choose lengths and to word failures; every expectation is
the oracle's, whose own scores at these shapes test_plan_geometry_host.py holds to plain f64 dot products."""
import time

import numpy as np
import pytest

import plan_geometry_ref as R
from plan_geometry_ref import TOL

pytestmark = pytest.mark.gpu

FULL, SAME, VALID = R.MODES


# One reference per needle: the oracle's scores of all three modes (one f64 transform) for the longest `within` of
# the needle's cases.  Valid scores of a shorter `within` -- a prefix of the longest -- are a prefix of its Valid
# scores: score j reads within[j, j + s) only.  The cases of one needle follow each other, so only that needle's
# references are kept.
_REF = {}


def reference(oracle, log_n, s, count):
    """(needle, within, {mode: scores}) of the case whose Valid output has `count` scores; never written to."""
    key = (log_n, s, count)
    if key not in _REF:
        for k in [k for k in _REF if k[:2] != key[:2]]:
            del _REF[k]
        needle, within = R.signals(oracle, log_n, s, count + s - 1, R.hop_of(log_n, s))
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


# ---------------------------------------------------------------------------
# 1. every score of level 1
# ---------------------------------------------------------------------------
def level1_cases():
    """(log_n, s, count, mode, ref_count): `count` Valid scores, i.e. a `within` of count + s - 1 samples, in `mode`;
    the reference is that of the needle's `within` of ref_count Valid scores."""
    cases = []
    for log_n in (21, 22):
        for s in R.needle_lengths(log_n):
            hop = R.hop_of(log_n, s)
            longest = max(R.score_counts(hop))
            cases += [(log_n, s, c, VALID, longest) for c in R.score_counts(hop)]
            cases += [(log_n, s, c, m, c) for c in (5 * hop + 2, 4 * hop + 1) for m in (SAME, FULL)]
    # 2^23: the oracle's transform has 2^25 points here, so only an even block count ending in a block of 2 scores
    # (raw odd hop; Valid and Full) and an odd one whose last pair has an empty second block (hop 8192)
    n = 1 << 23
    cases += [(23, n - 5000, 5 * 5001 + 2, m, 5 * 5001 + 2) for m in (VALID, FULL)]
    cases += [(23, n - 8191, 4 * 8192 + 1, VALID, 4 * 8192 + 1)]
    # 2^21, the rounded regime with real pair packing: three pairs of large blocks, 7 scores in the sixth block
    hop = R.hop_of(21, R.LARGE_HOP_S)
    cases += [(21, R.LARGE_HOP_S, 5 * hop + 7, VALID, 5 * hop + 7)]
    return cases


def case_id(case):
    log_n, s, count, mode, _ = case
    hop = R.hop_of(log_n, s)
    q, r = divmod(count + hop // 2, hop)
    r -= hop // 2
    return "2^%d-s=N-%d-hop%d-n=%dhop%+d-%s" % (log_n, (1 << log_n) - s, hop, q, r, R.MODE_NAMES[mode])


@pytest.mark.parametrize("case", level1_cases(), ids=case_id)
def test_every_score_of_a_register_plan(gpu, oracle, case):
    log_n, s, count, mode, ref_count = case
    t0 = time.perf_counter()
    hop = R.hop_of(log_n, s)
    needle, within, exp = reference(oracle, log_n, s, ref_count)
    expect = exp[VALID][:count] if mode == VALID else exp[mode]
    assert mode == VALID or count == ref_count
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
# 2. a loud block beside a silent one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["noise", "needle"])
@pytest.mark.parametrize("log_n", [21, 22])
def test_loud_block_beside_a_silent_one(gpu, oracle, log_n, content):
    """Four blocks of hop 8192; `within` is zero wherever block 1 or block 3 reads, and of amplitude 1.0 (four times
    the needle's) in what is left.  With a hop this far below N the blocks' inputs overlap almost wholly: what only
    blocks 0 and 2 read is [0, hop), so block 0 is loud and its partner in the pair, block 1, is silent -- exactly 0
    in the oracle.  A leak between the real and the imaginary half of a pair, or halves that swapped, puts block 0's
    scores into block 1.  `noise`: the loud samples are noise (scores of about TOL only: LIB scaling divides by the
    energy of 2^21 needle samples); `needle`: they are the needle's first samples at that amplitude, which makes
    score 0 about 4 * hop / s, 78 to 157 TOL."""
    n = 1 << log_n
    s = n - 8191
    hop = R.hop_of(log_n, s)
    count = 4 * hop
    needle, within = R.signals(oracle, log_n, s, count + s - 1)
    within = within * np.float32(4.0) if content == "noise" else np.resize(needle * np.float32(4.0), within.size)
    for b in (1, 3):
        within[b * hop:b * hop + n] = 0.0
    assert np.count_nonzero(within) > 0 and 0.9 < float(np.abs(within).max()) <= 1.0
    expect = oracle.correlate(within, needle, oracle.MODE_VALID, oracle.SCALE_LIB)
    if content == "needle":
        assert expect[0] > 50 * TOL
    algo = forced(gpu, needle, log_n)
    try:
        got = algo.correlate_with_sample(within, gpu.Mode.Valid, True)
    finally:
        algo.close()
    R.check_scores(got, expect, hop, "2^%d loud/silent (%s)" % (log_n, content))


# ---------------------------------------------------------------------------
# 3. one haystack over several launches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("s,blocks,extra", [(R.LARGE_HOP_S, 5, 7), ((1 << 21) - 5000, 9, 3)], ids=["large-hop", "raw-hop"])
def test_one_haystack_over_several_launches(gpu, oracle, s, blocks, extra):
    """pairs_per_group caps the pairs of a launch, so 1 and 2 (the smallest values am_context.hip's opt_pairs takes)
    run the later pairs with first_pair != 0: the same scores bit for bit as one launch, and as many K1 launches as
    the layout computed here needs."""
    log_n = 21
    hop = R.hop_of(log_n, s)
    count = blocks * hop + extra
    npairs = (-(-count // hop) + 1) // 2
    assert npairs >= 3
    needle, within, exp = reference(oracle, log_n, s, count)
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
    print("hop %d, %d scores, %d pairs: K1 launches %r" % (hop, count, npairs, launches))
    R.check_scores(got[default], exp[VALID], hop, "pairs_per_group %d" % default)
    for ppg in (1, 2):
        differ = np.flatnonzero(got[ppg].view(np.uint32) != got[default].view(np.uint32))
        assert np.array_equal(got[ppg], got[default]) and differ.size == 0, "pairs_per_group %d: %d scores differ, the first at %s" % (
            ppg, differ.size, R.place(int(differ[0]), hop))
    assert launches == {default: 1, 1: npairs, 2: -(-npairs // 2)}


# ---------------------------------------------------------------------------
# 4. level 2 on the same geometry, both sample formats
# ---------------------------------------------------------------------------
def peak_key(peaks):
    return [(q.start, q.end, q.height, q.prominence) for q in peaks]


def check_peaks(got, exp, tol, what):
    assert [(g.start, g.end) for g in got] == [(e[0], e[1]) for e in exp], what
    for g, e in zip(got, exp):
        assert abs(g.height - e[2]) < tol and abs(g.prominence - e[3]) < tol, (what, g, e)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_hits_on_the_seams_level2(gpu, oracle, d):
    """A needle of 20 000 samples in a haystack of 4.3 M: the 2^21 plan by the library's own choice, hop 2 076 672,
    three blocks.  Hits at hop + d, 2 * hop + d and at the last offset len - s (the very last score, which is no
    peak: the first and last score of a window never are), f32 and i16 stereo, twice each (the second call takes
    the sparse score path), and the same bit for bit with tail_block = 0."""
    sr, s, length = 8000, 20000, 4_300_000
    hop = R.hop_of(21, s)
    needle = oracle.synth_uniform(4100 + d, 0, 0, s)
    hay = oracle.synth_uniform(4100 + d, 1, 0, length)
    plants = [(hop + d, 1.0), (2 * hop + d, 0.9), (length - s, 0.8)]
    for p, gain in plants:
        hay[p:p + s] += np.float32(gain) * needle
    cfg = gpu.Config(chunk_size_s=60.0, overlap_length_s=s / sr, distance_s=5.0, prominence=0.13)
    p = cfg.params(sr, gpu.Scale.LIB)
    assert p.overlap == s
    lr = np.clip(np.round(np.repeat(hay, 2) * 20000.0), -32768, 32767).astype(np.int16)
    nlr = np.clip(np.round(np.repeat(needle, 2) * 20000.0), -32768, 32767).astype(np.int16)
    m_needle, m_hay = oracle.pcm_s16_stereo_to_mono(nlr), oracle.pcm_s16_stereo_to_mono(lr)
    exp = oracle.calc_chunks(sr, hay, needle, p.chunk, p.overlap, 0.13, p.min_distance, 5.0)
    exp16 = oracle.calc_chunks(sr, m_hay, m_needle, p.chunk, p.overlap, 0.13, p.min_distance, 5.0)
    assert [e[0] for e in exp] == [e[0] for e in exp16] == [hop + d, 2 * hop + d]
    algo, a16 = gpu.HipConvolve(needle), gpu.HipConvolve.from_pcm16(nlr)
    tail = gpu.get_option("tail_block")
    assert tail == 1
    try:
        runs = {}
        for setting in (tail, 0):
            gpu.set_option("tail_block", setting)
            for call in range(2):
                got, got16 = algo.match(hay, p), a16.match_pcm16(lr, p)
                check_peaks(got, exp, TOL, ("f32", setting, call))
                check_peaks(got16, exp16, 3 * TOL, ("pcm16", setting, call))
                runs[setting, call] = (peak_key(got), peak_key(got16))
    finally:
        gpu.set_option("tail_block", tail)
        algo.close()
        a16.close()
    assert runs[0, 0] == runs[tail, 0] and runs[0, 1] == runs[tail, 1]
