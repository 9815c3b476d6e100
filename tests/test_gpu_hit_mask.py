"""The per-hit record of a masked handle (am_hit_mask*, csrc/am_mask.hip) against the f64 definition of
mask_ref.hit_mask_ref: what the gaps of an occurrence hold (the original, loud noise, silence, a NaN), the flags, the three
call forms bit for bit, hits on both ends of the haystack and more hits than one grid column of the slice launch."""
import inspect

import numpy as np
import pytest

import hit_scores_ref as hs
import mask_ref as mr

pytestmark = pytest.mark.gpu

# the bound test_gpu_hit_scores.py holds am_hit_scores to (hit_scores_ref.assert_ref): an f32 rounding of an f64 result, 1e-6
# on the ratios; its level bound
TOL = inspect.signature(hs.assert_ref).parameters["tol"].default
TOL_DB = 1e-3
assert TOL == 1e-6

S = 10000                                            # three slices of 4096: 4096 + 4096 + 1808
GAPS = [(0, 100), (4000, 4200), (8190, 8200)]        # a leading gap, one over the first slice edge, one beside the second
N_HAY = 90_000
T_ORIGINAL, T_NOISE, T_SILENT, T_NAN_GAP, T_NAN_KEPT = 12_345, 25_000, 37_001, 49_152, 62_000


def peaks_at(am, ts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in ts]


def pack(recs):
    return b"".join(bytes(r) for r in recs)


@pytest.fixture(scope="module")
def case():
    """(needle, hay): a needle of amplitude 0.25 in a background of amplitude 0.01, planted whole (original in the gaps) at
    T_ORIGINAL and on both ends of the haystack, with noise 20 dB above it in the gaps at T_NOISE, with silent gaps at
    T_SILENT, with a NaN under a gap at T_NAN_GAP and under a kept span at T_NAN_KEPT."""
    rng = np.random.default_rng(17)
    needle = rng.uniform(-0.25, 0.25, S).astype(np.float32)
    hay = rng.uniform(-0.01, 0.01, N_HAY).astype(np.float32)
    for t in (0, T_ORIGINAL, T_NOISE, T_SILENT, T_NAN_GAP, T_NAN_KEPT, N_HAY - S):
        hay[t:t + S] += needle
    for b, e in GAPS:
        hay[T_NOISE + b:T_NOISE + e] = rng.uniform(-2.5, 2.5, e - b).astype(np.float32)
        hay[T_SILENT + b:T_SILENT + e] = 0.0
    hay[T_NAN_GAP + 4100] = np.nan
    hay[T_NAN_KEPT + 5000] = np.inf
    hay.setflags(write=False)
    return needle, hay


ALL_T = (0, T_ORIGINAL, T_NOISE, T_SILENT, T_NAN_GAP, T_NAN_KEPT, N_HAY - S, 70_000)


def test_records_against_the_definition(gpu, case):
    needle, hay = case
    algo = gpu.HipConvolve(needle, gaps=GAPS)
    got = algo.hit_mask(hay, peaks_at(gpu, ALL_T))
    exp = [mr.hit_mask_ref(hay, needle, GAPS, t) for t in ALL_T]
    for t, g, e in zip(ALL_T, got, exp):
        print(t, g, e)
        mr.assert_hit_mask(g, e, TOL, TOL_DB)
    by_t = dict(zip(ALL_T, got))
    for t in (0, T_ORIGINAL, N_HAY - S):                      # the original in the gaps
        assert by_t[t].flags == 0 and by_t[t].ncc_gaps > 0.99 and by_t[t].ncc > 0.99 and abs(by_t[t].gaps_db) < 0.1
    assert by_t[T_NOISE].flags == 0 and by_t[T_NOISE].ncc > 0.99 and abs(by_t[T_NOISE].ncc_gaps) < 0.3
    assert abs(by_t[T_NOISE].gaps_db - 20.0) < 1.0            # the gaps' noise against what the needle would put there
    assert by_t[T_SILENT].flags == mr.GAPS_SILENT and by_t[T_SILENT].gaps_db == -np.inf and by_t[T_SILENT].ncc_gaps == 0.0
    assert by_t[T_NAN_GAP].flags == mr.GAPS_NONFINITE and by_t[T_NAN_GAP].ncc > 0.99 and np.isnan(by_t[T_NAN_GAP].ncc_gaps)
    assert by_t[T_NAN_KEPT].flags == mr.NONFINITE and np.isnan(by_t[T_NAN_KEPT].ncc) and np.isnan(by_t[T_NAN_KEPT].gaps_db)
    assert by_t[70_000].ncc < 0.1                             # no occurrence


def test_ordinary_handle_and_floor(gpu, case):
    """A handle without gaps: AM_MASK_NO_GAPS, NaN gap fields, the kept fields are am_hit_scores' over the whole window.
    A hit over digital silence: below the floor."""
    needle, hay = case
    ts = (T_ORIGINAL, T_NOISE)
    got = gpu.HipConvolve(needle).hit_mask(hay, peaks_at(gpu, ts))
    scores = gpu.HipConvolve(needle).hit_scores(hay, peaks_at(gpu, ts))
    for t, g, sc in zip(ts, got, scores):
        mr.assert_hit_mask(g, mr.hit_mask_ref(hay, needle, None, t), TOL, TOL_DB)
        assert g.flags == mr.NO_GAPS and np.isnan(g.ncc_gaps) and np.isnan(g.gaps_db)
        assert abs(g.ncc - sc.ncc) <= TOL and abs(g.gain - sc.gain) <= TOL
    quiet = np.zeros(S + 10, dtype=np.float32)
    quiet[GAPS[1][0] + 3] = 1.0   # loud under a gap, silence under every kept span
    g, = gpu.HipConvolve(needle, gaps=GAPS).hit_mask(quiet, peaks_at(gpu, [0]))
    mr.assert_hit_mask(g, mr.hit_mask_ref(quiet, needle, GAPS, 0), TOL, TOL_DB)
    assert g.flags == mr.BELOW_FLOOR and g.ncc == 0.0 and g.kept_db == -np.inf and g.gaps_db == np.inf


def test_three_forms_agree_in_bits(gpu, case):
    """Host, _device and _batch_device (two handles, one of them ordinary, against two haystacks): one set of bits, and
    a hit's record does not depend on the other hits of the call."""
    needle, hay = case
    masked, plain = gpu.HipConvolve(needle, gaps=GAPS), gpu.HipConvolve(needle)
    hay2 = np.ascontiguousarray(hay[5000:80_000])
    peaks = [peaks_at(gpu, ALL_T), peaks_at(gpu, [T_ORIGINAL - 5000, T_NOISE - 5000, 0, hay2.size - S])]
    bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in (hay, hay2)]
    try:
        host = [[a.hit_mask(h, p) for a in (masked, plain)] for h, p in zip((hay, hay2), peaks)]
        dev = [[a.hit_mask_device(b.ptr, h.size, p) for a in (masked, plain)] for b, h, p in zip(bufs, (hay, hay2), peaks)]
        batch = gpu.hit_mask_batch_device([masked, plain], [b.ptr for b in bufs], [hay.size, hay2.size], [[p, p] for p in peaks])
        alone = [masked.hit_mask_device(bufs[0].ptr, hay.size, peaks_at(gpu, [t]))[0] for t in ALL_T]
    finally:
        for b in bufs:
            b.free()
    for k in range(2):
        for j in range(2):
            assert pack(host[k][j]) == pack(dev[k][j]) == pack(batch[k][j]), (k, j)
    assert pack(alone) == pack(host[0][0])
    # the same samples at another offset of another haystack: the same record
    assert bytes(host[1][0][0]) == bytes(host[0][0][1])


def test_pcm16_forms(gpu, case):
    """Interleaved i16 stereo: the record of the library's own down-mix of the frames, host and device forms alike."""
    import score_norm_ref as ref
    needle, hay = case
    clean = np.where(np.isfinite(hay), hay, 0).astype(np.float32)
    frames = ref.stereo(clean)
    mono = gpu.pcm_s16_stereo_to_mono(frames)
    ts = (0, T_ORIGINAL, T_NOISE, T_SILENT, N_HAY - S)
    algo = gpu.HipConvolve(needle, gaps=GAPS)
    got = algo.hit_mask(frames, peaks_at(gpu, ts))
    for t, g in zip(ts, got):
        mr.assert_hit_mask(g, mr.hit_mask_ref(mono, needle, GAPS, t), TOL, TOL_DB)
    buf = gpu.DeviceBuffer.from_numpy(0, frames)
    try:
        dev = algo.hit_mask_device(buf.ptr, len(frames), peaks_at(gpu, ts), fmt=gpu.Fmt.S16_STEREO)
    finally:
        buf.free()
    assert pack(dev) == pack(got)
    assert pack(algo.hit_mask(mono, peaks_at(gpu, ts))) == pack(got)


def test_more_hits_than_one_grid_column(gpu):
    """65 535 hits fill one grid column of the slice launch (kHitMaxGridY): 65 536 + 3 hits take a second launch.  A short
    needle with two gaps, a hit on every offset; every record against the definition, computed for all offsets at once."""
    s, gaps = 48, [(5, 9), (40, 48)]
    n_hits = 65_535 + 4
    rng = np.random.default_rng(23)
    needle = rng.uniform(-1, 1, s).astype(np.float32)
    hay = rng.uniform(-1, 1, n_hits + s - 1).astype(np.float32)   # the last hit ends on the haystack's last sample
    algo = gpu.HipConvolve(needle, gaps=gaps)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    try:
        got = algo.hit_mask_device(buf.ptr, hay.size, peaks_at(gpu, range(n_hits)))
    finally:
        buf.free()
    keep = np.ones(s, dtype=bool)
    for b, e in gaps:
        keep[b:e] = False
    x, n64 = hay.astype(np.float64), needle.astype(np.float64)
    nk, og = np.where(keep, n64, 0), np.where(keep, 0, n64)
    ck, cg = np.correlate(x, nk, "valid"), np.correlate(x, og, "valid")
    ek, xg = np.correlate(x * x, keep.astype(np.float64), "valid"), np.correlate(x * x, (~keep).astype(np.float64), "valid")
    en, ng = float(nk @ nk), float(og @ og)
    ncc, gain, ncc_gaps = ck / np.sqrt(en * ek), ck / en, cg / np.sqrt(ng * xg)
    gaps_db = 10 * np.log10(xg / (gain * gain * ng))
    g = np.array([(q.ncc, q.gain, q.ncc_gaps, q.gaps_db, q.flags) for q in got], dtype=np.float64)
    assert np.all(g[:, 4] == 0)
    assert np.max(np.abs(g[:, 0] - ncc)) <= TOL and np.max(np.abs(g[:, 2] - ncc_gaps)) <= TOL
    assert np.max(np.abs(g[:, 1] - gain)) <= TOL
    assert np.max(np.abs(g[:, 3] - gaps_db)) <= TOL_DB
    for t in (0, 65_534, 65_535, n_hits - 1):                      # the launches' first and last rows, by the scalar definition
        mr.assert_hit_mask(got[t], mr.hit_mask_ref(hay, needle, gaps, t), TOL, TOL_DB)


def test_refusals_are_hit_scores(gpu, case):
    """The refusals of am_hit_scores: a hit whose window leaves the haystack (message as there), a host pointer given to
    the _device form, an empty call."""
    needle, hay = case
    algo = gpu.HipConvolve(needle, gaps=GAPS)
    with pytest.raises(gpu.AudioMatchError) as ei:
        algo.hit_mask(hay, peaks_at(gpu, [N_HAY - S + 1]))
    assert ei.value.code == gpu.AM_ERR_INVALID_ARG and "start + needle length > haystack length" in str(ei.value)
    with pytest.raises(gpu.AudioMatchError) as ei:
        algo.hit_mask_device(hay.ctypes.data, hay.size, peaks_at(gpu, [0]))
    assert ei.value.code == gpu.AM_ERR_INVALID_ARG and "not device memory" in str(ei.value)
    assert algo.hit_mask(hay, []) == []
