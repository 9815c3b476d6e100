"""The fixed list of small cases whose raw output bytes pin the library's kernels between two builds (a refactor of the
kernels must not move a bit).  tools/hit_records_dump.py dumps them to a file and compares two files;
tests/test_gpu_kernel_bytes.py compares their SHA-256 digests with tests/golden/kernel_bytes.json, which was recorded
from the parent of the commit that added it.

A family is a function f(am, record): it calls record(name, fn, *inputs) once per case; fn() returns the list of the
case's output arrays, `inputs` are the arrays the case was computed from (their digest tells a changed random stream
from a changed library).  A call the library refuses is recorded as its error code.  The inputs are seeded numpy arrays.

The per-hit families (scores, segments, warp, channel, stereo): needle lengths 1, 255, 4095, 4096, 4097 and 8200 (one
thread, under one wave stride, the slice edge and its neighbours, three slices with a ragged last) in a haystack of
S + 64 samples with the needle planted at 17; hits at 0, 17 and len - S (the first and last clip the head and the tail);
f32 mono and i16 stereo.  Scores on all of those; segments with m = 1, 3 and R = 0, 1, 2, 4, 5, 16 (both sides of every
kernel radius); warp with K = 2, R = 2 on the two longest needles; channel with P = 0, 15, 16, 40 (one lag tile, a tile
edge and its neighbour, three tiles); stereo with R = 0, 1, 4, 5, 16; for each family one case with a NaN sample inside
the window and one with an all-zero window.  The cases go through the host form of each family; the _device and
_batch_device forms are called as well, on the 4097-sample needle with one setting per family.
significance: 3 * 4096 + 5 scores with guard 3 and radius 64 (and radius 5000: zones of three slices), hits at both ends
and in the middle.
score_norm: the NCC scores of correlate for a short needle (norm_scores' direct path, one workgroup of the needle's sum
of squares) and one of 4097 samples (whole block energies; 17 workgroups of the sum of squares) on a haystack that
crosses a tile edge; needle_energy: 1 / energy as the handle reports it at one workgroup (255, 256), two (257), and at
and past 2048 workgroups of 256 threads (524288, 524289, 600001: a thread adds more than one square); the scores of
windows that are the needle itself (window_db shows the energy's last bits).
bands: F = 2^8 (one bin per thread) and 2^12 (nine; bin 2048 is thread 0's last); 1, 8, 9 and 17 frames (one group, a
full group, the seam, a ragged third); B = 1 and 32 (the combine's 129 values pass the 64-lane stride twice); f32 and
i16 stereo, a NaN in the window, an all-zero window, the three call forms on one case; a 17-frame window whose group
partials cancel (bands_cancelling: the order of the combine's additions shows in the f32 records).
envelope: the same two frame sizes; 1, 2, 8, 9 frames (one frame is the unpaired half of a packed transform); drift 0
and +-1000 ppm, i16 stereo, a NaN, digital silence.
envelope_scores: 1, 4095, 4096, 4097, 8200 haystack frames (the prefix blocks of 4096); needles of 1, 8, 9 frames;
Q = 1, 4, 5 (wave groups of four); B = 1 and 32; with B = 32 a needle of 257 frames (two LDS spans); an absent and an
invalid level in the haystack and in a needle.
lag_products: lengths 1, 8191, 8192, 8193, 16400 (blocks of 8192); orders 0 (refused), 7, 8 and 64; f32 and i16; a NaN.
discover: probes of one part (200 samples) and of four (1000), hop 300, a NaN in A; probe_scores on 8191, 8192, 8193
and 3 * 8192 + 5 scores with the best in the first, a middle and the last slice, resident scores at a start that is
not 16-byte aligned.
trace: am_match_trace with bins of 101 and 2048 (one wave per bin), 2049, 8191, 8192 and 8193 scores (slices of 8192);
am_trace_scores_device at a start that is not 16-byte aligned (the rotation)."""
import ctypes as C
import hashlib

import numpy as np

LENGTHS = (1, 255, 4095, 4096, 4097, 8200)
PAD = 64
PLANT = 17
SEG_RADII = (0, 1, 2, 4, 5, 16)
CHAN_RADII = (0, 15, 16, 40)
STEREO_RADII = (0, 1, 4, 5, 16)
ENV_ABSENT = 0xFFFF


def needle_of(s, seed=0):
    return np.random.default_rng([seed, s]).standard_normal(s).astype(np.float32)


def haystack_of(needle, fmt, kind="planted", length=None):
    """A seeded haystack of len(needle) + PAD samples (or `length`) with the needle at PLANT.  kind: "planted", "nan"
    (f32 only: one NaN in the middle of the planted window) or "zero" (the planted window is all zero)."""
    s = needle.size
    n = s + PAD if length is None else length
    rng = np.random.default_rng([1, s, 0 if fmt == "f32" else 1])
    if fmt == "f32":
        hay = (0.25 * rng.standard_normal(n)).astype(np.float32)
        hay[PLANT:PLANT + s] += needle
        if kind == "nan":
            hay[PLANT + s // 2] = np.nan
        if kind == "zero":
            hay[max(0, PLANT - 20):PLANT + s + 20] = 0.0
        return hay
    hay = rng.integers(-2000, 2000, size=(n, 2)).astype(np.int32)
    hay[PLANT:PLANT + s, 0] += np.rint(6000.0 * needle).astype(np.int32)
    hay[PLANT + 1:PLANT + s, 1] -= np.rint(3000.0 * needle[:-1]).astype(np.int32)   # (right: inverted, one frame late)
    if kind == "zero":
        hay[max(0, PLANT - 20):PLANT + s + 20] = 0
    return np.clip(hay, -32768, 32767).astype(np.int16)


def raw(a):
    return a.tobytes() if hasattr(a, "tobytes") else bytes(a)


def _peaks_of(am, starts):
    return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in starts]


def _lead_of(am, form, algo, hay, starts):
    """the arguments ahead of the parameters for one call form ("" host, "_device", "_batch_device": one needle, one
    haystack), and what must stay alive during the call"""
    a, fmt, length = am._samples(hay)
    k = len(starts)
    pk = am._peak_array(_peaks_of(am, starts))
    if form == "":
        return (algo._h, a.ctypes.data, length, int(fmt), pk, k), a
    buf = am.DeviceBuffer.from_numpy(0, a)
    if form == "_device":
        return (algo._h, buf.ptr, length, int(fmt), pk, k), buf
    return ((C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(length), 1, int(fmt), pk, k,
            (C.c_size_t * 1)(k)), buf


def _family(am, fam, algo, hay, starts, args, form=""):
    lead, keep = _lead_of(am, form, algo, hay, starts)
    rec, _ = am._hit_call(fam, form, lead, len(starts), args)
    return [rec]


def _channel(am, algo, hay, starts, cp, form=""):
    lead, keep = _lead_of(am, form, algo, hay, starts)
    rec, taps = am._channel_call(form, lead, len(starts), cp)
    return [rec, taps]


def hits(am, record):
    def all_families(tag, algo, needle, hay, fmt, s, starts, every, form=""):
        """every: the whole parameter lists; otherwise one setting per family (the flag cases and the other call forms)"""
        record("scores/" + tag, lambda: _family(am, am._SCORES, algo, hay, starts, (), form), needle, hay)
        for m in (1, 3):
            for r in SEG_RADII if every else (4,):
                if m <= s:
                    record("segments/%s/m%d/r%d" % (tag, m, r), lambda: _family(am, am._SEGMENTS, algo, hay, starts, (m, r), form), needle, hay)
        if s >= 4096:
            record("warp/" + tag, lambda: _family(am, am._WARP, algo, hay, starts, (am.warp_params(200.0, 2, 2),), form), needle, hay)
        for p in CHAN_RADII if every else (16,):
            record("channel/%s/p%d" % (tag, p), lambda: _channel(am, algo, hay, starts, am.channel_params(p), form), needle, hay)
        if fmt == "i16":
            for r in STEREO_RADII if every else (4,):
                record("stereo/%s/r%d" % (tag, r), lambda: _family(am, am._STEREO, algo, hay, starts, (r,), form), needle, hay)

    for s in LENGTHS:
        needle = needle_of(s)
        algo = am.HipConvolve(needle)
        for fmt in ("f32", "i16"):
            all_families("s%d/%s" % (s, fmt), algo, needle, haystack_of(needle, fmt), fmt, s, (0, PLANT, PAD), True)
            if s == 4097:   # the other two call forms of every family: the same kernels behind another front
                for form in ("_device", "_batch_device"):
                    all_families("s%d/%s%s" % (s, fmt, form), algo, needle, haystack_of(needle, fmt), fmt, s, (0, PLANT, PAD), False, form)
    # the flag branches: a NaN sample inside the window, an all-zero window
    s = 4097
    needle = needle_of(s)
    algo = am.HipConvolve(needle)
    for fmt, kind in (("f32", "nan"), ("f32", "zero"), ("i16", "zero")):
        all_families("%s/s%d/%s" % (kind, s, fmt), algo, needle, haystack_of(needle, fmt, kind), fmt, s, (0, PLANT, PAD), False)


def significance(am, record):
    s = 255
    n_scores = 3 * 4096 + 5
    needle = needle_of(s)
    algo = am.HipConvolve(needle)
    starts = (0, PLANT, n_scores // 2, n_scores - 1)
    for fmt, kind in (("f32", "planted"), ("i16", "planted"), ("f32", "nan"), ("f32", "zero")):
        hay = haystack_of(needle, fmt, kind, length=s + n_scores - 1)
        for guard, radius in ((3, 64), (3, 5000)):
            for form in ("", "_device", "_batch_device") if kind == "planted" else ("",):
                record("significance/%s/%s/g%d/b%d%s" % (kind, fmt, guard, radius, form),
                       lambda: _family(am, am._SIGNIFICANCE, algo, hay, starts, (guard, radius), form), needle, hay)


def score_norm(am, record):
    # a short needle (norm_scores' direct path) and one of 4097 samples (>= 2048 + 2 * 1024, the bound in am_norm.hip from
    # which a window is assembled from whole block energies: the path with the workgroup sum), on a haystack whose 2148
    # scores cross a tile edge (tiles of 2048 scores)
    for s in (255, 4097):
        needle = needle_of(s)
        algo = am.HipConvolve(needle, score_norm=True)
        for kind in ("planted", "zero", "nan"):
            hay = haystack_of(needle, "f32", kind, length=s + 2048 + 100)
            record("score_norm/%s/s%d" % (kind, s), lambda: [algo.correlate_with_sample(hay, am.Mode.Valid, scale=True)], needle, hay)


def needle_energy(am, record):
    for s in (255, 256, 257, 4097, 524288, 524289, 600001):
        needle = needle_of(s)
        record("needle_energy/s%d" % s,
               lambda: [np.array([am.HipConvolve(needle).inverse_sample_auto_correlation()], dtype=np.float32)], needle)
    # the energy's last bits: a window that is the needle itself has window_db = 10 log10(E_w / E_n) with E_w / E_n = 1 to a
    # few ulp, so the record's f32 shows the ulps of E_n that 1 / E_n as f32 hides
    for s in (257, 1000, 4097, 8200, 20000, 600001):
        needle = needle_of(s, seed=9)
        hay = np.concatenate([np.zeros(PLANT, dtype=np.float32), needle, np.zeros(PAD - PLANT, dtype=np.float32)])
        record("needle_energy/window_db/s%d" % s, lambda: _family(am, am._SCORES, am.HipConvolve(needle), hay, (PLANT,), ()), needle, hay)


def _band_edges(lf, nb):
    top = (1 << lf) // 2 + 1
    return [0, top] if nb == 1 else [int(e) for e in np.rint(np.linspace(1, top, nb + 1))]


def bands(am, record):
    for lf in (8, 12):
        f = 1 << lf
        for frames in (1, 8, 9, 17):
            s = f + (frames - 1) * (f // 2)
            needle = needle_of(s, seed=2)
            algo = am.HipConvolve(needle)
            for nb in (1, 32):
                bp = am.band_params(lf, _band_edges(lf, nb))
                for fmt in ("f32", "i16"):
                    hay = haystack_of(needle, fmt)
                    tag = "bands/f%d/j%d/b%d/%s" % (lf, frames, nb, fmt)
                    record(tag, lambda: _family(am, am._BANDS, algo, hay, (0, PLANT, PAD), (bp,)), needle, hay)
                    if frames == 17 and nb == 32:
                        for form in ("_device", "_batch_device"):
                            record(tag + form, lambda: _family(am, am._BANDS, algo, hay, (0, PLANT, PAD), (bp,), form), needle, hay)
                if frames in (9, 17):
                    for fmt, kind in (("f32", "nan"), ("f32", "zero"), ("i16", "zero")):
                        hay = haystack_of(needle, fmt, kind)
                        record("bands/%s/f%d/j%d/b%d/%s" % (kind, lf, frames, nb, fmt),
                               lambda: _family(am, am._BANDS, algo, hay, (0, PLANT, PAD), (bp,)), needle, hay)
    bands_cancelling(am, record)


def bands_cancelling(am, record):
    """17 frames whose group partials cancel: the needle has the period of a group (8 hops), the window is +needle under
    group 0's frames and -needle under group 1's (0 where a frame of one group overlaps the other's), so the two groups'
    partial records are each other's negatives exactly, and 1e-10 needle under the last half of frame 16: P_xn of a band
    is group 2's small value exactly when the groups are added in ascending order, and carries the rounding of the large
    partials, some 1e-6 of it, in any other order."""
    lf = 8
    h = (1 << lf) // 2
    base = needle_of(8 * h, seed=10)
    needle = np.concatenate([base, base, base[:2 * h]])
    x = np.zeros(18 * h, dtype=np.float32)
    x[h:8 * h] = needle[h:8 * h]
    x[9 * h:16 * h] = -needle[9 * h:16 * h]
    x[17 * h:] = np.float32(1e-10) * needle[17 * h:]
    hay = np.concatenate([np.zeros(PLANT, dtype=np.float32), x, np.zeros(PAD - PLANT, dtype=np.float32)])
    algo = am.HipConvolve(needle)
    for nb in (1, 32):
        bp = am.band_params(lf, _band_edges(lf, nb))
        record("bands/cancel/b%d" % nb, lambda: _family(am, am._BANDS, algo, hay, (PLANT,), (bp,)), needle, hay)


def envelope(am, record):
    slack = 40   # (under half a frame: no further frame at drift 0; the frames of +-1000 ppm reach at most 17 samples further)
    for lf in (8, 12):
        f = 1 << lf
        for nb in (4, 32):
            ep = am.env_params(am.band_params(lf, _band_edges(lf, nb)), 80.0)
            for frames in (1, 2, 8, 9):
                n = f + (frames - 1) * (f // 2) + slack
                rng = np.random.default_rng([3, lf, frames])
                x = (0.3 * rng.standard_normal(n)).astype(np.float32)
                pcm = rng.integers(-9000, 9000, size=(n, 2)).astype(np.int16)
                tag = "envelope/f%d/b%d/j%d" % (lf, nb, frames)
                for ppm in (0.0, 1000.0, -1000.0) if nb == 4 else (0.0,):
                    record("%s/f32/ppm%d" % (tag, int(ppm)), lambda: [am.envelope(x, ep, ppm)], x)
                    record("%s/i16/ppm%d" % (tag, int(ppm)), lambda: [am.envelope(pcm, ep, ppm)], pcm)
                if nb == 4:
                    bad = x.copy()
                    bad[n // 2] = np.nan
                    record(tag + "/nan", lambda: [am.envelope(bad, ep, 0.0)], bad)
                    quiet = x.copy()
                    quiet[:min(n, f + f // 2)] = 0.0   # (the first frame, or the first two, silent)
                    record(tag + "/head_silent", lambda: [am.envelope(quiet, ep, 0.0)], quiet)
                    zeros = np.zeros(n, dtype=np.float32)
                    record(tag + "/silence", lambda: [am.envelope(zeros, ep, 0.0)], zeros)
                    zpcm = np.zeros((n, 2), dtype=np.int16)
                    record(tag + "/silence_i16", lambda: [am.envelope(zpcm, ep, 0.0)], zpcm)


def envelope_scores(am, record):
    def levels(rng, nb, j):
        return rng.integers(0, 1024, size=(nb, j)).astype(np.uint16)

    def scores(needles, hay):
        z, qi = am.envelope_scores(needles, hay)
        return [z, qi]

    needle_frames = (1, 8, 9, 8, 1)
    for jh in (1, 4095, 4096, 4097, 8200):
        for nb in (1, 32):
            for q in (1, 4, 5):
                rng = np.random.default_rng([4, jh, nb, q])
                hay = levels(rng, nb, jh)
                needles = [levels(rng, nb, j) for j in needle_frames[:q]]
                if jh > 100:   # a needle cut from the haystack: a score of 1 among the others
                    needles[-1] = hay[:, 50:50 + needles[-1].shape[1]].copy()
                record("envelope_scores/h%d/b%d/q%d" % (jh, nb, q), lambda: scores(needles, hay), hay, *needles)
    rng = np.random.default_rng([4, 257])
    hay = levels(rng, 32, 4097)
    long_needles = [hay[:, 1000:1257].copy(), levels(rng, 32, 9), levels(rng, 32, 257)]
    record("envelope_scores/two_spans", lambda: scores(long_needles, hay), hay, *long_needles)
    hay1 = levels(rng, 4, 4097)
    needles = [levels(rng, 4, 8), levels(rng, 4, 9)]
    for tag, where, value in (("absent", "hay", ENV_ABSENT), ("invalid", "hay", 2000), ("absent", "needle", ENV_ABSENT), ("invalid", "needle", 2000)):
        h2, n2 = hay1.copy(), [m.copy() for m in needles]
        if where == "hay":
            h2[1, 4095] = value   # (the last frame of the first prefix block)
        else:
            n2[1][2, 3] = value
        record("envelope_scores/%s_%s" % (tag, where), lambda: scores(n2, h2), h2, *n2)


def lag_products(am, record):
    for n in (1, 8191, 8192, 8193, 16400):
        rng = np.random.default_rng([5, n])
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        pcm = rng.integers(-9000, 9000, size=(n, 2)).astype(np.int16)
        for order in (0, 7, 8, 64):
            record("lag_products/n%d/o%d/f32" % (n, order), lambda: [am.lag_products(x, order)], x)
            record("lag_products/n%d/o%d/i16" % (n, order), lambda: [am.lag_products(pcm, order)], pcm)
    bad = x.copy()
    bad[8200] = np.nan
    record("lag_products/nan", lambda: [am.lag_products(bad, 64)], bad)


def discover(am, record):
    rng = np.random.default_rng([6])
    a = (0.3 * rng.standard_normal(5000)).astype(np.float32)
    b = (0.3 * rng.standard_normal(3 * 8192 + 5 + 999)).astype(np.float32)
    b[20000:23000] += a[1000:4000]
    bad = a.copy()
    bad[1234] = np.nan
    for probe_len in (200, 1000):   # sumsq_parts: 1 and 4
        dp = am.discover_params(probe_len, 300)
        record("discover/l%d" % probe_len, lambda: [am.discover(a, b, dp)], a, b)
        record("discover/l%d/nan" % probe_len, lambda: [am.discover(bad, b, dp)], bad, b)
    dps = am.discover_params(1000, 300, exclude=500, flags=1)   # AM_DISCOVER_SELF
    record("discover/self", lambda: [am.discover(a, a, dps)], a)
    for n in (8191, 8192, 8193, 3 * 8192 + 5):
        for where, pos in (("first", 100), ("middle", n // 2), ("last", n - 3)):
            y = (0.1 * np.random.default_rng([7, n]).standard_normal(n)).astype(np.float32)
            y[pos] = 0.9
            y[(pos + n // 3) % n] = 0.8
            y[15] = 0.95   # (inside the excluded range)
            record("probe_scores/n%d/%s" % (n, where), lambda: [am.probe_scores(y, 10, 20, 100)], y)
    y = np.concatenate([np.zeros(1, dtype=np.float32), y])
    buf = am.DeviceBuffer.from_numpy(0, y)
    record("probe_scores/unaligned", lambda: [am.probe_scores_device(0, buf.ptr + 4, y.size - 1, 10, 20, 100)], y)


def trace(am, record):
    s = 255
    n_scores = 3 * 8192 + 5
    needle = needle_of(s)
    algo = am.HipConvolve(needle)
    for fmt in ("f32", "i16"):
        hay = haystack_of(needle, fmt, length=s + n_scores - 1)
        for bin_ in (101, 2048, 2049, 8191, 8192, 8193):
            record("trace/match/%s/d%d" % (fmt, bin_), lambda: [algo.match_trace(hay, bin_)], needle, hay)
    y = (0.1 * np.random.default_rng([8]).standard_normal(n_scores + 1)).astype(np.float32)
    y[777] = np.nan
    buf = am.DeviceBuffer.from_numpy(0, y)
    for bin_ in (101, 2048, 8192, 8193):
        record("trace/scores/d%d" % bin_, lambda: [am.trace_scores(y[1:], bin_)], y)
        record("trace/scores_unaligned/d%d" % bin_, lambda: [am.trace_scores_device(0, buf.ptr + 4, n_scores, bin_)], y)


FAMILIES = {"hits": hits, "significance": significance, "score_norm": score_norm, "needle_energy": needle_energy, "bands": bands,
            "envelope": envelope, "envelope_scores": envelope_scores, "lag_products": lag_products, "discover": discover, "trace": trace}


def run_family(am, name):
    """{case: (SHA-256 of the input bytes, the output bytes)} of one family; a case of several arrays is case/0, case/1, .."""
    out = {}

    def record(case, fn, *inputs):
        h = hashlib.sha256()
        for a in inputs:
            h.update(raw(a))
        try:
            arrs = fn()
        except am.AudioMatchError as e:
            arrs = [("error %s" % e.code).encode()]
        for i, a in enumerate(arrs):
            key = case if len(arrs) == 1 else "%s/%d" % (case, i)
            assert key not in out, key
            out[key] = (h.hexdigest(), raw(a))

    FAMILIES[name](am, record)
    return out


def digests(am, name):
    """{case: {"in": .., "out": ..}}: what tests/golden/kernel_bytes.json holds per family"""
    return {k: {"in": i, "out": hashlib.sha256(o).hexdigest()} for k, (i, o) in run_family(am, name).items()}
