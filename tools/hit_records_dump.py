#!/usr/bin/env python3
"""The raw record bytes of the per-hit families and of score_norm on a fixed list of small cases, for comparing two
builds of the library byte for byte (a refactor of the kernels must not move a bit).

  python tools/hit_records_dump.py OUT.npz        every case's records, as uint8 arrays keyed by the case's name
  python tools/hit_records_dump.py --compare A.npz B.npz
                                                  one JSON line: the case count, equal or not, the differing cases

The inputs are seeded numpy arrays; the tool reads nothing but the library of the tree it stands in.  Run it once in
each tree, each in a process of its own, then compare the files.

The cases: needle lengths 1, 255, 4095, 4096, 4097 and 8200 (one thread, under one wave stride, the slice edge and its
neighbours, three slices with a ragged last) in a haystack of S + 64 samples with the needle planted at 17; hits at 0,
17 and len - S (the first and last clip the head and the tail); f32 mono and i16 stereo.  Scores on all of those;
segments with m = 1, 3 and R = 0, 1, 2, 4, 5, 16 (both sides of every kernel radius); warp with K = 2, R = 2 on the two
longest needles; channel with P = 0, 15, 16, 40 (one lag tile, a tile edge and its neighbour, three tiles); stereo with
R = 0, 1, 4, 5, 16; significance on 3 * 4096 + 5 scores with guard 3 and radius 64 (and radius 5000: zones of three
slices), hits at both ends and in the middle; the NCC scores of correlate for a short and a long needle on a haystack
that crosses a tile edge.  For each family one case with a NaN sample inside the window and one with an all-zero window.
The cases go through the host form of each family (am_hit_scores, ...): the three forms share their kernels and their
launch sequence.  The _device and _batch_device forms are called as well, on the 4097-sample needle with one setting per
family, so that every entry point is in the file.  A call the library refuses is recorded as its error code."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))

LENGTHS = (1, 255, 4095, 4096, 4097, 8200)
PAD = 64
PLANT = 17
SEG_RADII = (0, 1, 2, 4, 5, 16)
CHAN_RADII = (0, 15, 16, 40)
STEREO_RADII = (0, 1, 4, 5, 16)


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


def dump(path):
    import audiomatch_amd as am
    out = {}

    def peaks_of(starts):
        return [am.Peak(int(t), int(t) + 1, 0.0, 0.0) for t in starts]

    def record(name, fn):
        try:
            arrs = fn()
        except am.AudioMatchError as e:
            arrs = [np.frombuffer(("error %s" % e.code).encode(), dtype=np.uint8)]
        for i, a in enumerate(arrs):
            out[name if len(arrs) == 1 else "%s/%d" % (name, i)] = np.frombuffer(bytes(a), dtype=np.uint8).copy()

    def lead_of(form, algo, hay, starts):
        """the arguments ahead of the parameters for one call form ("" host, "_device", "_batch_device": one needle, one
        haystack), and what must stay alive during the call"""
        a, fmt, length = am._samples(hay)
        k = len(starts)
        pk = am._peak_array(peaks_of(starts))
        if form == "":
            return (algo._h, a.ctypes.data, length, int(fmt), pk, k), a
        buf = am.DeviceBuffer.from_numpy(0, a)
        if form == "_device":
            return (algo._h, buf.ptr, length, int(fmt), pk, k), buf
        return ((C.c_void_p * 1)(algo._h), 1, (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(length), 1, int(fmt), pk, k,
                (C.c_size_t * 1)(k)), buf

    def family(fam, algo, hay, starts, args, form=""):
        lead, keep = lead_of(form, algo, hay, starts)
        rec, _ = am._hit_call(fam, form, lead, len(starts), args)
        return [rec]

    def channel(algo, hay, starts, cp, form=""):
        lead, keep = lead_of(form, algo, hay, starts)
        rec, taps = am._channel_call(form, lead, len(starts), cp)
        return [rec, taps]

    def all_families(tag, algo, hay, fmt, s, starts, every, form=""):
        """every: the whole parameter lists; otherwise one setting per family (the flag cases and the other call forms)"""
        record("scores/" + tag, lambda: family(am._SCORES, algo, hay, starts, (), form))
        for m in (1, 3):
            for r in SEG_RADII if every else (4,):
                if m <= s:
                    record("segments/%s/m%d/r%d" % (tag, m, r), lambda: family(am._SEGMENTS, algo, hay, starts, (m, r), form))
        if s >= 4096:
            record("warp/" + tag, lambda: family(am._WARP, algo, hay, starts, (am.warp_params(200.0, 2, 2),), form))
        for p in CHAN_RADII if every else (16,):
            record("channel/%s/p%d" % (tag, p), lambda: channel(algo, hay, starts, am.channel_params(p), form))
        if fmt == "i16":
            for r in STEREO_RADII if every else (4,):
                record("stereo/%s/r%d" % (tag, r), lambda: family(am._STEREO, algo, hay, starts, (r,), form))

    for s in LENGTHS:
        needle = needle_of(s)
        algo = am.HipConvolve(needle)
        for fmt in ("f32", "i16"):
            all_families("s%d/%s" % (s, fmt), algo, haystack_of(needle, fmt), fmt, s, (0, PLANT, PAD), True)
            if s == 4097:   # the other two call forms of every family: the same kernels behind another front
                for form in ("_device", "_batch_device"):
                    all_families("s%d/%s%s" % (s, fmt, form), algo, haystack_of(needle, fmt), fmt, s, (0, PLANT, PAD), False, form)

    # the flag branches: a NaN sample inside the window, an all-zero window
    s = 4097
    needle = needle_of(s)
    algo = am.HipConvolve(needle)
    for fmt, kind in (("f32", "nan"), ("f32", "zero"), ("i16", "zero")):
        all_families("%s/s%d/%s" % (kind, s, fmt), algo, haystack_of(needle, fmt, kind), fmt, s, (0, PLANT, PAD), False)

    # significance: 3 * 4096 + 5 scores, hits at both ends and in the middle
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
                       lambda: family(am._SIGNIFICANCE, algo, hay, starts, (guard, radius), form))

    # score_norm: the NCC scores of correlate; a short needle (norm_scores' direct path) and one of 4097 samples (>= 2048
    # + 2 * 1024, the bound in am_norm.hip from which a window is assembled from whole block energies: the path with the
    # workgroup sum), on a haystack whose 2148 scores cross a tile edge (tiles of 2048 scores)
    for s in (255, 4097):
        needle = needle_of(s)
        algo = am.HipConvolve(needle, score_norm=True)
        for kind in ("planted", "zero", "nan"):
            hay = haystack_of(needle, "f32", kind, length=s + 2048 + 100)
            record("score_norm/%s/s%d" % (kind, s), lambda: [algo.correlate_with_sample(hay, am.Mode.Valid, scale=True)])

    np.savez(path, **out)
    print(json.dumps({"cases": len(out), "bytes": int(sum(a.size for a in out.values())), "file": path}))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    differing = [n for n in names if n not in a.files or n not in b.files or a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]
    errors = [n for n in a.files if bytes(a[n][:5]) == b"error"]
    print(json.dumps({"cases": len(names), "equal": not differing, "differing": differing, "refused_calls": errors}))
    return 0 if not differing else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("paths", nargs="+")
    a = ap.parse_args()
    if a.compare:
        if len(a.paths) != 2:
            ap.error("--compare takes two files")
        sys.exit(compare(*a.paths))
    if len(a.paths) != 1:
        ap.error("one output file")
    dump(a.paths[0])


if __name__ == "__main__":
    main()
