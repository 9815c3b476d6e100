#!/usr/bin/env python3
"""Per-hit channel estimation (am_hit_channel_device) on the workload of tools/hit_scores_bench.py: the 10 s needle at
44.1 kHz, a seeded resident 1 h haystack and 64 hits (the planted ones first, the rest at seeded random offsets).

Per radius (P = 16 and P = 128): the call's time (host clock around the C entry point on prebuilt arguments, median and
min of --reps; it holds the host's solve) and the kernels' time (device events around the launch sequences, am_profile_*),
both per hit; and in the same run the obvious alternative for the same lags: ceil((2 P + 1) / 33) calls of
am_hit_segments_device with m = 1, R = 16 at starts shifted by 33, which cover the lags -P .. P and compute E_w beside
every c (kernel_ratio_to_segments_calls; above 1 the tile kernel would be mis-shaped).  The shifted starts are clamped to
the haystack; the work per call does not depend on the start.
The planted hits are checked (main tap 0, taps close to the delta, ncc_eq > 0.95).  Prints one JSON line.

  python tools/hit_channel_bench.py [--reps R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_scores_bench as hsb  # noqa: E402
from hit_scores_bench import H, S, SR, am  # noqa: E402

HITS = 64
SEG_R = 16


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
    rows = []
    for p in (16, 128):
        cp = am.channel_params(p, 60.0)
        out = (am.HitChannel * n)()
        taps = np.zeros((n, 2 * p + 1), dtype=np.float32)
        _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_channel_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(cp), out, taps.ctypes.data)),
                                    a.reps, a.warmup, dev)
        for i in range(len(planted)):
            assert out[i].flags == 0 and out[i].main_tap == 0 and abs(taps[i][p] - 1.0) < 0.01 and out[i].ncc_eq > 0.95, (p, i, out[i])
        # the same lags by the segment kernel: calls of 33 lags each, centred at -P + 16, -P + 49, ...
        ncalls = -(-(2 * p + 1) // (2 * SEG_R + 1))
        sp = am.AmSegmentParams(1, SEG_R)
        seg = (am.HitSegment * n)()
        shifted = []
        for q in range(ncalls):
            off = -p + SEG_R + q * (2 * SEG_R + 1)
            shifted.append((am.AmPeak * n)(*[am.AmPeak(min(max(t + off, 0), H - S), min(max(t + off, 0), H - S) + 1, 0.0, 0.0) for t in starts]))

        def all_calls():
            for arr in shifted:
                am._check(L.am_hit_segments_device(algo._h, hay.ptr, H, 0, arr, n, C.byref(sp), seg))

        _, smed, smn, skms = hsb.timed(all_calls, a.reps, a.warmup, dev)
        rows.append({"radius": p, "lags": 2 * p + 1, "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n,
                     "kernel_us_per_hit_median": 1e3 * kms / n,
                     "segments_calls": {"calls": ncalls, "segments": 1, "radius": SEG_R, "call_us_per_hit_median": 1e3 * smed / n,
                                        "call_us_per_hit_min": 1e3 * smn / n, "kernel_us_per_hit_median": 1e3 * skms / n},
                     "kernel_ratio_to_segments_calls": kms / skms if skms > 0 else None,
                     "call_ratio_to_segments_calls": med / smed})
    hay.free()
    print(json.dumps({"shape": f"needle {S} samples (10 s at 44.1 kHz), one resident 1 h f32 haystack, {n} hits, noise_db 60",
                      "reps": a.reps, "hit_channel": rows}))


if __name__ == "__main__":
    main()
