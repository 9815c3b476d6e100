#!/usr/bin/env python3
"""Per-segment hit scoring (am_hit_segments_device) beside per-hit scoring (am_hit_scores_device) on the workload of
tools/hit_scores_bench.py: the 10 s needle at 44.1 kHz, the same seeded resident 1 h haystacks and the same hits (those
of haystack 0 in each of that tool's batch rows: 1, 32, 500 and 5000 hits, the planted ones first).

Per row and per (m, R) in (16, 1), (16, 4), (64, 16): the call's time (host clock around the C entry point on prebuilt
arguments, median and min of --reps), the kernels' time (device events around the launch sequence, am_profile_*), both per
hit, and their ratios to am_hit_scores_device on the same hits in the same run.  The planted hits are checked (every
segment's ncc > 0.5, lag within half a sample of 0).  Prints one JSON line.

  python tools/hit_segments_bench.py [--reps R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_scores_bench as hsb  # noqa: E402
from hit_scores_bench import H, NH, S, SR, am  # noqa: E402

CONFIGS = ((16, 1), (16, 4), (64, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = 0
    rng = np.random.default_rng(1)
    needle = am.synth_uniform_device(dev, S, 7, 0, amp=0.5)
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    hay = am.synth_uniform_device(dev, H, 7, 1, amp=0.1)          # haystack 0 of hit_scores_bench.py
    planted = [[600 * SR * m + 30 * SR + 17 * k for m in range(6)] for k in range(NH)]
    for t in planted[0]:
        am.axpy_device(dev, hay, t, needle.ptr, S, 1.0)
    L = am.lib()
    rows = []
    for nhits in (1, 64, 1000, 10000):
        starts = []
        for i in range(nhits):   # that tool's hit list (the random offsets of both haystacks are drawn, haystack 0's kept)
            k, j = i % NH, i // NH
            t = planted[k][j] if j < len(planted[k]) else int(rng.integers(0, H - S))
            if k == 0:
                starts.append(t)
        n = len(starts)
        pk = (am.AmPeak * n)(*[am.AmPeak(t, t + 1, 0.0, 0.0) for t in starts])
        sc = (am.AmHitScore * n)()
        _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_scores_device(algo._h, hay.ptr, H, 0, pk, n, sc)), a.reps, a.warmup, dev)
        base = {"call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n, "kernel_us_per_hit_median": 1e3 * kms / n}
        row = {"hits": n, "hit_scores": base, "hit_segments": []}
        for m, r in CONFIGS:
            sp = am.AmSegmentParams(m, r)
            out = (am.HitSegment * (n * m))()
            _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_segments_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(sp), out)),
                                        a.reps, a.warmup, dev)
            for i, t in enumerate(starts):
                if t in planted[0]:
                    assert all(out[i * m + j].ncc > 0.5 and abs(out[i * m + j].lag) < 0.5 for j in range(m)), (t, m, r)
            row["hit_segments"].append({
                "segments": m, "radius": r,
                "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n, "kernel_us_per_hit_median": 1e3 * kms / n,
                "call_ratio_to_hit_scores": (1e3 * med / n) / base["call_us_per_hit_median"],
                "kernel_ratio_to_hit_scores": (1e3 * kms / n) / base["kernel_us_per_hit_median"] if base["kernel_us_per_hit_median"] > 0 else None})
        rows.append(row)
    hay.free()
    print(json.dumps({"shape": f"needle {S} samples (10 s at 44.1 kHz), one resident 1 h f32 haystack", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
