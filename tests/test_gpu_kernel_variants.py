"""Every row of the transform kernels' tables (am_fft.hip: kK1, kTailK1, kK2, kK2h, kK2Mfma, kK2Group, kK2Spectrum,
kK2Gen, kK3, kK3Gen, kK3Group, kTailK3) reached once through public entry points and checked against the CPU oracle:
a launcher that picked another row than the one its arguments name -- another sample kind, half level, form or plan --
reads or writes the work matrix in another format, and the scores are garbage.

How a row is reached:
  * plan: the per-handle option log_n (21: 256-row, 22: 512-row, 23: 1024-row kernels; 16: the generic ones);
  * half level: the per-handle option half_pipeline (0, 1, 2; the 1024-row and generic plans have level 0 only);
  * sample kind: am_match* on f32 samples, am_match_pcm16* on i16 stereo frames;
  * the spectrum kernel: by creating the handle's spectrum on a plan with 8192-point rows (every case);
  * redo rows: a chunk that fails its certificate (a dip deeper than half a prominence) in a batch with
    debug_redo_arm_at = 0, as test_gpu_round4.py::test_redo_paths_chosen_deterministically does, and with that test's
    proof that the path ran: the profile's launch counts (K3 fuses its scan, and so can be redone, only with a hop
    that is a multiple of 1024: hence the needle N - 8191);
  * accumulate rows: a needle longer than 2^22 samples, as test_gpu_round4.py::test_accumulating_k3_takes_any_score_pointer
    (its segments' scores fit one pair of 2^22 blocks: the 512-row plan) and test_gpu_round3.py::test_long_needles (more
    scores than that: the 1024-row plan) do;
  * group rows: am_match_multi_device with two needles of one length (one K3 launch fewer than with k3_group = 0);
  * tail rows: a haystack with an odd, part-filled last block on the library's own choice of plan (2^22, the tail on
    2^21; log_n must be 0 for that), alone (launch_k1 / launch_k2(tail) / launch_k3) and in a batch (launch_tail_batch_*),
    as test_gpu_round4.py::test_odd_last_block_on_the_smaller_plan does;
  * k2_mfma: on for one half-level-2 case;
  * the 512 x 16384 rows: am_debug_column_bench(wide = 1), the only caller of that plan.  It has no row kernel, hence
    no scores: these two rows are only launched, what they compute is not checked.

Shapes: two block pairs, the second block of the last pair ragged (3 hops + 7 scores), needle N - 8191 (hop 8192, the
smallest that is floored to the score tile) and signals of plan_geometry_ref.py.  Bounds: f32 correlation to plan_geometry_ref.TOL through check_scores; hits
with offsets identical to calc_chunks' and heights to TOL (f32, level 0) or to the 1e-3 of
test_gpu_round2.py::test_half_pipeline_levels_on_both_plans_and_several_needles (half levels 1 and 2, i16 stereo).

A combination without a kernel is an empty row: the launcher answers hipErrorInvalidValue and launches nothing.  No
public entry point asks for one (half_scale() gives level 0 where no half form exists), so that is checked twice: on the
host, by calling the launchers themselves with such a combination and no block pairs (an empty row answers before
anything else; a row that is not empty would be refused its empty grid, so nothing can start either way and the test
needs no device), and on the device by half_pipeline on a 2^23 plan staying inert."""
import ctypes as C

import numpy as np
import pytest

import plan_geometry_ref as R
from plan_geometry_ref import TOL

HALF_TOL = 1e-3
SR = 8000
PROMINENCE = 0.13


# ---------------------------------------------------------------------------
# host only: an empty row is an invalid argument and launches nothing
# ---------------------------------------------------------------------------
class Job(C.Structure):       # am_kernels.h
    _fields_ = [("src", C.c_void_p), ("src_len", C.c_longlong), ("lead", C.c_longlong), ("dst", C.c_void_p),
                ("out_count", C.c_longlong), ("hop", C.c_int), ("nblocks", C.c_int), ("first_pair", C.c_int), ("src_kind", C.c_int)]


class PlanDev(C.Structure):   # am_kernels.h
    _fields_ = [("logN", C.c_int), ("logN1", C.c_int), ("logN2", C.c_int), ("logLo", C.c_int)] + [
        (n, C.c_void_p) for n in ("tw1", "tw2", "twlo", "twhi", "twlo4", "twhi4", "k2j", "k2c", "mf")]


HIP_ERROR_INVALID_VALUE = 1
LAUNCH_K1 = "_ZN2am9launch_k1EP12ihipStream_tRKNS_3JobEiP15HIP_vector_typeIfLj2EERKNS_7PlanDevEi"
LAUNCH_K3 = "_ZN2am9launch_k3EP12ihipStream_tRKNS_3JobEiPK15HIP_vector_typeIfLj2EERKNS_7PlanDevEfRKNS_7ScanCfgEib"
PLANS = {"r16": (8, 13), "c512": (9, 13), "c1024": (10, 13), "c512w": (9, 14)}


def plan(name):
    n1, n2 = PLANS[name]
    return PlanDev(logN=n1 + n2, logN1=n1, logN2=n2, logLo=12)


@pytest.mark.parametrize("name,kind,half", [("c1024", 0, 1), ("c1024", 1, 2), ("c512w", 0, 1), ("c512w", 1, 0)])
def test_k1_without_a_kernel_is_an_invalid_argument(amlib, name, kind, half):
    fn = getattr(amlib.lib(), LAUNCH_K1)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(Job), C.c_int, C.c_void_p, C.POINTER(PlanDev), C.c_int]
    job = Job(src_kind=kind, hop=5000, nblocks=2, out_count=10000)
    assert fn(None, C.byref(job), 0, None, C.byref(plan(name)), half) == HIP_ERROR_INVALID_VALUE   # (npairs = 0: see the module's docstring)


@pytest.mark.parametrize("name,half,accumulate,only_pairs", [
    ("c1024", 1, False, False), ("c1024", 2, False, True), ("c512", 1, True, False), ("r16", 0, True, False), ("r16", 2, True, False),
    ("c512w", 1, False, False), ("c512w", 0, True, False), ("c512w", 0, False, True)])
def test_k3_without_a_kernel_is_an_invalid_argument(amlib, name, half, accumulate, only_pairs):
    fn = getattr(amlib.lib(), LAUNCH_K3)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(Job), C.c_int, C.c_void_p, C.POINTER(PlanDev), C.c_float, C.c_void_p, C.c_int, C.c_bool]
    job = Job(hop=5000, nblocks=2, out_count=10000)
    # ScanCfg (am_kernels.h): stats32, wbits, tile_theta, margin, hist_min, seg_c, seg_d, inv_c, only_pairs at byte 56;
    # all zero = no scan, no redo
    scan = (C.c_ulonglong * 256)()
    flags = (C.c_int * 4)()
    if only_pairs:
        scan[7] = C.addressof(flags)
    assert fn(None, C.byref(job), 0, None, C.byref(plan(name)), C.c_float(1.0), scan, half, accumulate) == HIP_ERROR_INVALID_VALUE


# ---------------------------------------------------------------------------
# the cases of a forced plan: one needle, one haystack, one reference per sample kind
# ---------------------------------------------------------------------------
_CASE = {}


def stereo(x):
    """The signal as interleaved i16 stereo frames, left = right (the down-mix gives it back, scaled and rounded)."""
    return np.clip(np.round(np.repeat(x, 2) * 12000.0), -32768, 32767).astype(np.int16)


def params(gpu, s):
    """One window: a chunk of 4 s (more than the 24 583 scores of a case) with the needle's length as overlap
    (Config::from_args, audio_matcher.rs:41)."""
    return gpu.AmMatchParams(sr=SR, chunk=4 * SR, overlap=s, min_prominence=PROMINENCE, min_distance=SR // 10,
                             overshadow_distance_s=0.1, scale=int(gpu.Scale.LIB))


def forced_case(gpu, oracle, log_n):
    """Needle N - 8191 (hop 8192), 3 hops + 7 scores; the plants of plan_geometry_ref.signals on the seams, a second needle's hit
    for the group call, and an inverted copy of the needle (a score of -0.5: the chunk fails its certificate).  The
    signals of one plan are shared by its cases and never written to; so is each reference, computed by the first
    case that needs it (reference())."""
    if log_n not in _CASE:
        _CASE.clear()
        n = 1 << log_n
        s = R.needle_lengths(log_n)[2] if log_n >= 21 else R.generic_needle_lengths(log_n)[4]
        assert s == n - 8191 and R.hop_of(log_n, s) == 8192
        hop = R.hop_of(log_n, s)
        count = 3 * hop + 7
        needle, hay = R.signals(oracle, log_n, s, count + s - 1, hop)
        hay = hay.copy()
        other = oracle.synth_uniform(log_n, 7, 0, s)
        hay[hop + 2000:hop + 2000 + s] += np.float32(0.9) * other
        hay[700:700 + s] -= np.float32(0.5) * needle
        hits = [off for off, _ in R.plants(hop) if off < count]   # one on either side of a seam and one on it
        assert len(hits) == 3
        c = {"s": s, "hop": hop, "count": count, "needle": needle, "other": other, "hay": hay, "p": params(gpu, s), "hits": hits,
             "needle16": stereo(needle), "hay16": stereo(hay)}
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _CASE[log_n] = c
    return _CASE[log_n]


def reference(c, oracle, which):
    """The oracle's answer for a case: "f32" / "i16" / "other": calc_chunks of the needle on the f32 samples, on the
    down-mixed frames, of the second needle; "scores": every Valid score."""
    which = "reference " + which
    if which not in c:
        p = c["p"]
        chunks = lambda hay, needle: oracle.calc_chunks(SR, hay, needle, p.chunk, p.overlap, PROMINENCE, p.min_distance, 0.1)
        if which == "reference scores":
            c[which] = oracle.correlate(c["hay"], c["needle"], oracle.MODE_VALID, oracle.SCALE_LIB)
        elif which == "reference i16":
            c[which] = chunks(oracle.pcm_s16_stereo_to_mono(c["hay16"]), oracle.pcm_s16_stereo_to_mono(c["needle16"]))
        else:
            c[which] = chunks(c["hay"], c["other"] if which == "reference other" else c["needle"])
        if which != "reference scores":
            assert [e[0] for e in c[which]] == ([c["hop"] + 2000] if which == "reference other" else c["hits"])
    return c[which]


def check_hits(got, exp, tol, what):
    assert [(g.start, g.end) for g in got] == [(e[0], e[1]) for e in exp], what
    for g, e in zip(got, exp):
        print("%s: hit %d height %.6f (oracle %.6f)" % (what, g.start, g.height, e[2]))
        assert abs(g.height - e[2]) < tol, (what, g, e)


def key(peaks):
    return [(q.start, q.end, q.height, q.prominence) for q in peaks]


def handle(gpu, needle, pcm, log_n, half):
    algo = gpu.HipConvolve.from_pcm16(needle) if pcm else gpu.HipConvolve(needle)
    algo.set_option("log_n", log_n)
    algo.set_option("half_pipeline", half)
    return algo


FORCED = [(log_n, pcm, half) for log_n in (21, 22) for pcm in (False, True) for half in (0, 1, 2)] + [
    (23, False, 0), (23, True, 0), (16, False, 0), (16, True, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,pcm,half", FORCED, ids=["2^%d-%s-half%d" % (l, "i16" if k else "f32", h) for l, k, h in FORCED])
def test_k1_k2_k3_rows_of_a_forced_plan(gpu, oracle, log_n, pcm, half):
    """One call alone (K1, K2 and plain K3 of the plan, sample kind and half level; the host redoes the failed chunk
    with the plain K3 row), then a batch of two on fresh handles (no history of failures) with the device-side redo
    off and on.  On: one launch more per haystack outside the profile's kernel classes (the redo row), and one K3
    launch per haystack; off: the host launches K3 again for the failed chunks."""
    c = forced_case(gpu, oracle, log_n)
    tol = TOL if half == 0 and not pcm else HALF_TOL
    exp = reference(c, oracle, "i16" if pcm else "f32")
    what = "2^%d %s half %d" % (log_n, "i16" if pcm else "f32", half)
    needle, hay = (c["needle16"], c["hay16"]) if pcm else (c["needle"], c["hay"])
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    n = c["hay"].size
    mask = gpu.get_option("profile_mask")
    counts = {}
    try:
        algo = handle(gpu, needle, pcm, log_n, half)
        alone = algo.match_pcm16(hay, c["p"]) if pcm else algo.match(hay, c["p"])
        algo.close()
        check_hits(alone, exp, tol, what)
        gpu.set_option("profile_mask", -1)
        for arm in (-1, 0):
            gpu.set_option("debug_redo_arm_at", arm)
            algo = handle(gpu, needle, pcm, log_n, half)
            with gpu.Profile(0) as prof:
                both = (algo.match_pcm16_batch_device if pcm else algo.match_batch_device)([buf.ptr, buf.ptr], [n, n], c["p"])
                counts[arm] = (prof.query("k3_cols_inv")[1], prof.query("other")[1])
            algo.close()
            for got in both:
                check_hits(got, exp, tol, what + ", batch, debug_redo_arm_at %d" % arm)
    finally:
        gpu.set_option("debug_redo_arm_at", -2)
        gpu.set_option("profile_mask", mask)
    print("%s: (K3, other) launches by debug_redo_arm_at: %r" % (what, counts))
    if log_n >= 21:      # (the generic kernels have no fused scan, hence no redo)
        assert counts[0][1] - counts[-1][1] == 2, counts
        assert counts[0][0] == 2 and counts[-1][0] > 2, counts
    else:
        assert counts[0] == counts[-1], counts


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [21, 22, 23, 16])
def test_f32_scores_of_a_forced_plan(gpu, oracle, log_n):
    """Every score of the f32 rows, and half_pipeline inert where the plan has no half form (2^23, generic)."""
    c = forced_case(gpu, oracle, log_n)
    exp = reference(c, oracle, "scores")
    algo = handle(gpu, c["needle"], False, log_n, 0)
    try:
        got = algo.correlate_with_sample(c["hay"], gpu.Mode.Valid, True)
        worst = R.check_scores(got, exp, c["hop"], "2^%d" % log_n)
        print("2^%d: %d scores, max error %.3g" % (log_n, got.size, worst))
        if log_n in (23, 16):
            for level in (1, 2):
                algo.set_option("half_pipeline", level)
                again = algo.correlate_with_sample(c["hay"], gpu.Mode.Valid, True)
                assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "half_pipeline %d is not inert on 2^%d" % (level, log_n)
    finally:
        algo.close()


@pytest.mark.gpu
def test_matrix_core_row(gpu, oracle):
    """k2_mfma with half level 2 on the 256-row plan: the kK2Mfma row (and the packed-f16 K1 / K3 rows around it)."""
    c = forced_case(gpu, oracle, 21)
    assert gpu.get_option("k2_mfma") == 0
    gpu.set_option("k2_mfma", 1)
    algo = handle(gpu, c["needle"], False, 21, 2)
    try:
        check_hits(algo.match(c["hay"], c["p"]), reference(c, oracle, "f32"), HALF_TOL, "2^21 f32 half 2, k2_mfma")
    finally:
        gpu.set_option("k2_mfma", 0)
        algo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [21, 22])
def test_needle_group_rows(gpu, oracle, log_n):
    """Two needles of one length against one haystack: the group row of K2 and the plan's group row of K3 -- one K3
    launch for both needles, where k3_group = 0 launches one each (fresh handles per setting: no history)."""
    c = forced_case(gpu, oracle, log_n)
    p = c["p"]
    buf = gpu.DeviceBuffer.from_numpy(0, c["hay"])
    mask = gpu.get_option("profile_mask")
    assert gpu.get_option("k3_group") == 1
    launches = {}
    try:
        gpu.set_option("profile_mask", -1)
        for grouped in (1, 0):
            gpu.set_option("k3_group", grouped)
            algos = [handle(gpu, x, False, log_n, 0) for x in (c["needle"], c["other"])]
            with gpu.Profile(0) as prof:
                res = gpu.match_multi_device(algos, buf.ptr, c["hay"].size, p)
                launches[grouped] = prof.query("k3_cols_inv")[1]
            for a in algos:
                a.close()
            check_hits(res[0], reference(c, oracle, "f32"), TOL, "2^%d k3_group %d, needle 0" % (log_n, grouped))
            check_hits(res[1], reference(c, oracle, "other"), TOL, "2^%d k3_group %d, needle 1" % (log_n, grouped))
    finally:
        gpu.set_option("k3_group", 1)
        gpu.set_option("profile_mask", mask)
    print("2^%d: K3 launches by k3_group: %r" % (log_n, launches))
    assert launches[0] - launches[1] == 1, launches


@pytest.mark.gpu
@pytest.mark.parametrize("count", ["one-pair-of-2^22", "more"])
def test_accumulate_rows(gpu, oracle, count):
    """A needle of 2^22 + 12 345 samples is two segments of 2.1 M; K3 adds the second one's scores to the first one's.
    70 002 scores fit one pair of 2^22 blocks (the 512-row plan), two hops and 5000 more do not (the 1024-row plan)."""
    s = (1 << 22) + 12345
    seg = s - s // 2
    hop22 = R.hop_of(22, seg)
    n_out = 70002 if count == "one-pair-of-2^22" else 2 * hop22 + 5000
    needle = oracle.synth_uniform(83, 0, 0, s)
    within = oracle.synth_uniform(83, 1, 0, n_out + s - 1)
    for off, gain in ((1234, 1.0), (n_out - 3, 0.8)):
        within[off:off + s] += np.float32(gain) * needle
    exp = oracle.correlate(within, needle, oracle.MODE_VALID, oracle.SCALE_LIB)
    algo = gpu.HipConvolve(needle)
    try:
        got = algo.correlate_with_sample(within, gpu.Mode.Valid, True)
    finally:
        algo.close()
    worst = R.check_scores(got, exp, hop22 if count == "one-pair-of-2^22" else R.hop_of(23, seg), "partitioned needle, " + count)
    print("partitioned needle, %s: %d scores, max error %.3g" % (count, got.size, worst))


_TAIL = {}


def tail_case(gpu, oracle, pcm):
    """10 s of 44.1 kHz (the 2^22 plan by the library's choice): two blocks of that plan and one hop of the 2^21 plan
    + 200 000 scores more, which are two blocks of that plan, the second ragged.  Hits in the main pass, on the tail's
    first score, on the last score of the tail's first block and near the end.  (needle, haystack, expected) of a kind."""
    sr, s = 44100, 441000
    if not _TAIL:
        hop, hop_t = R.hop_of(22, s), R.hop_of(21, s)
        T, rest = 2 * hop, hop_t + 200000
        needle = oracle.synth_uniform(231, 0, 0, s)
        hay = oracle.synth_uniform(231, 1, 0, T + rest + s - 1)
        offs = [20 * sr, T, T + hop_t - 1, T + rest - sr]
        for off in offs:
            hay[off:off + s] += needle
        p = gpu.Config(chunk_size_s=60.0, overlap_length_s=10.0, distance_s=2.0, prominence=0.3).params(sr, gpu.Scale.LIB)
        _TAIL.update({"p": p, "offs": offs, False: [needle, hay], True: [stereo(needle), stereo(hay)]})
    t, p = _TAIL[pcm], _TAIL["p"]
    if len(t) == 2:
        needle, hay = (oracle.pcm_s16_stereo_to_mono(x) for x in t) if pcm else t
        t.append(oracle.calc_chunks(sr, hay, needle, p.chunk, p.overlap, 0.3, p.min_distance, 2.0))
        assert [e[0] for e in t[2]] == _TAIL["offs"]
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("half", [0, 1, 2])
def test_tail_rows(gpu, oracle, half, pcm):
    """The odd last block alone (the 256-row K1 / K3 rows and the tail row of K2) and the tails of two haystacks in one
    launch each (the rows of kTailK1 and kTailK3)."""
    needle, hay, exp = tail_case(gpu, oracle, pcm)
    p = _TAIL["p"]
    assert gpu.get_option("tail_block") == 1
    tol = TOL if half == 0 and not pcm else HALF_TOL
    what = "tail, %s half %d" % ("i16" if pcm else "f32", half)
    algo = handle(gpu, needle, pcm, 0, half)
    buf = gpu.DeviceBuffer.from_numpy(0, hay)
    n = hay.size // 2 if pcm else hay.size
    try:
        alone = algo.match_pcm16(hay, p) if pcm else algo.match(hay, p)
        check_hits(alone, exp, tol, what)
        both = (algo.match_pcm16_batch_device if pcm else algo.match_batch_device)([buf.ptr, buf.ptr], [n, n], p)
        assert key(both[0]) == key(both[1])
        check_hits(both[0], exp, tol, what + ", batch")
    finally:
        algo.close()


@pytest.mark.gpu
def test_wide_column_rows(gpu):
    """The 512 x 16384 plan has column kernels only and one caller, the measurement hook: its two rows launch and
    the hook returns.  Nothing more can be said here: without a row kernel the plan yields no scores to compare."""
    k1, k3 = C.c_double(0.0), C.c_double(0.0)
    gpu._check(gpu.lib().am_debug_column_bench(0, 1, 2, 1, 1, C.byref(k1), C.byref(k3)))
    assert k1.value > 0.0 and k3.value > 0.0
