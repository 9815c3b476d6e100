#!/usr/bin/env python3
"""Per-band hit scoring (am_hit_bands_device) beside per-segment hit scoring (am_hit_segments_device) on the workload of
tools/hit_scores_bench.py: the 10 s needle at 44.1 kHz, a seeded resident 1 h haystack and 64 hits (the planted ones
first, the rest at seeded random offsets).

Per F in (1024, 4096), 16 log-spaced bands from 50 Hz to 16 kHz: the call's time (host clock around the C entry point on
prebuilt arguments, median and min of --reps) and the kernels' time (device events around the launch sequence,
am_profile_*), both per hit; and in the same run am_hit_segments_device with m = 8, R = 4 on the same hits, for scale.
The planted hits are checked (every band's ncc > 0.5).  Prints one JSON line.

  python tools/hit_bands_bench.py [--reps R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_scores_bench as hsb  # noqa: E402
from hit_scores_bench import H, S, SR, am  # noqa: E402

HITS, BANDS = 64, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = 0
    rng = np.random.default_rng(1)
    needle = am.synth_uniform_device(dev, S, 7, 0, amp=0.5)
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    hay = am.synth_uniform_device(dev, H, 7, 1, amp=0.1)
    planted = [600 * SR * m + 30 * SR for m in range(6)]
    for t in planted:
        am.axpy_device(dev, hay, t, needle.ptr, S, 1.0)
    starts = planted + [int(rng.integers(0, H - S)) for _ in range(HITS - len(planted))]
    n = len(starts)
    L = am.lib()
    pk = (am.AmPeak * n)(*[am.AmPeak(t, t + 1, 0.0, 0.0) for t in starts])
    sp = am.AmSegmentParams(8, 4)
    seg = (am.HitSegment * (n * 8))()
    _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_segments_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(sp), seg)),
                                a.reps, a.warmup, dev)
    base = {"segments": 8, "radius": 4, "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n,
            "kernel_us_per_hit_median": 1e3 * kms / n}
    rows = []
    for lf in (10, 12):
        bp = am.band_edges_log(SR, lf, 50.0, 16000.0, BANDS)
        out = (am.HitBand * (n * BANDS))()
        _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_bands_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(bp), out)),
                                    a.reps, a.warmup, dev)
        for i in range(len(planted)):
            assert all(out[i * BANDS + b].flags == 0 and out[i * BANDS + b].ncc > 0.5 for b in range(BANDS)), (lf, i)
        frames = (S - (1 << lf)) // (1 << (lf - 1)) + 1
        rows.append({"frame": 1 << lf, "frames_per_hit": frames, "edges": list(bp.edges[:BANDS + 1]),
                     "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n, "kernel_us_per_hit_median": 1e3 * kms / n,
                     "kernel_us_per_frame": 1e3 * kms / n / frames,
                     "call_ratio_to_hit_segments": (1e3 * med / n) / base["call_us_per_hit_median"],
                     "kernel_ratio_to_hit_segments": (1e3 * kms / n) / base["kernel_us_per_hit_median"] if base["kernel_us_per_hit_median"] > 0 else None})
    hay.free()
    print(json.dumps({"shape": f"needle {S} samples (10 s at 44.1 kHz), one resident 1 h f32 haystack, {n} hits, {BANDS} bands",
                      "reps": a.reps, "hit_segments": base, "hit_bands": rows}))


if __name__ == "__main__":
    main()
