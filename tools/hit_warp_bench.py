#!/usr/bin/env python3
"""Per-hit drift scoring (am_hit_warp_device) beside per-segment hit scoring (am_hit_segments_device) on the workload of
tools/hit_scores_bench.py: the 10 s needle at 44.1 kHz, a seeded resident 1 h haystack and 64 hits (the planted ones
first, the rest at seeded random offsets).

Per grid (K = 8, R = 4 and K = 32, R = 16, +-400 ppm): the call's time (host clock around the C entry point on prebuilt
arguments, median and min of --reps) and the kernels' time (device events around the launch sequences, am_profile_*),
both per hit; and in the same run am_hit_segments_device on the same hits with m = 8, R = 4 (the family's usual call) and
with m = 1 at the grid's R: per (hit, rate) the correlation does the work of one such call, so a hit should cost about
Q = 2 K + 1 times that plus the warp pass (ratio_to_q_segments_m1; above 1.5 is worth an explanation).
The planted hits are checked (drift within 5 ppm of 0, ncc > 0.9).  Prints one JSON line.

  python tools/hit_warp_bench.py [--reps R] [--warmup W]"""
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

    def segments(m, r):
        sp = am.AmSegmentParams(m, r)
        seg = (am.HitSegment * (n * m))()
        _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_segments_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(sp), seg)),
                                    a.reps, a.warmup, dev)
        return {"segments": m, "radius": r, "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n,
                "kernel_us_per_hit_median": 1e3 * kms / n}

    base = segments(8, 4)
    rows = []
    for k, r in ((8, 4), (32, 16)):
        one = segments(1, r)
        wp = am.warp_params(400.0, k, r)
        out = (am.HitWarp * n)()
        _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_warp_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(wp), out)),
                                    a.reps, a.warmup, dev)
        for i in range(len(planted)):
            assert not out[i].flags & ~1 and abs(out[i].drift_ppm) < 5.0 and out[i].ncc > 0.9, (k, r, i, out[i])
        q = 2 * k + 1
        rows.append({"steps": k, "radius": r, "rates": q, "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n,
                     "kernel_us_per_hit_median": 1e3 * kms / n, "kernel_us_per_hit_and_rate": 1e3 * kms / n / q,
                     "hit_segments_m1": one,
                     "call_ratio_to_hit_segments_m8_r4": (1e3 * med / n) / base["call_us_per_hit_median"],
                     "kernel_ratio_to_q_segments_m1": (1e3 * kms / n) / (q * one["kernel_us_per_hit_median"]) if one["kernel_us_per_hit_median"] > 0 else None,
                     "call_ratio_to_q_segments_m1": (1e3 * med / n) / (q * one["call_us_per_hit_median"])})
    hay.free()
    print(json.dumps({"shape": f"needle {S} samples (10 s at 44.1 kHz), one resident 1 h f32 haystack, {n} hits, drifts +-400 ppm",
                      "reps": a.reps, "hit_segments": base, "hit_warp": rows}))


if __name__ == "__main__":
    main()
