#!/usr/bin/env python3
"""The per-hit stereo image (am_hit_stereo_device) on the workload of tools/hit_scores_bench.py in i16 stereo: a 10 s
needle at 44.1 kHz (the down-mix of a synthetic stereo snippet), a seeded resident 1 h haystack of i16 stereo frames and
64 hits (the planted ones first, the rest at seeded random offsets), R = 8.

  hit_stereo   the call's time (host clock around the C entry point on prebuilt arguments, median and min of --reps) and
               the kernels' time (device events around the launch sequence, am_profile_*), both per hit
  baseline     what gives the same lags without this family: two am_hit_segments_device calls (m = 1, R = 8) on
               de-interleaved f32 copies of L and R, plus the two passes over the PCM that make those copies (here
               am_pcm_s16_stereo_mix_device with (1, 0) and (0, 1); host clock, they end in a device synchronise).  The
               copies are made once per haystack, so the passes are reported beside the calls, not per hit.
  pcm          am_pcm_s16_stereo_mix_device against am_pcm_s16_stereo_to_mono_device on the same 1 h buffer: they move
               the same bytes (median, min and max of --reps each)
The planted hits are checked (ncc_mid > 0.5, image centre).  Prints one JSON line.

  python tools/hit_stereo_bench.py [--reps R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_scores_bench as hsb  # noqa: E402
from hit_scores_bench import H, S, SR, am  # noqa: E402

HITS = 64
RADIUS = 8


def clocked(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = 0
    rng = np.random.default_rng(1)
    L = am.lib()
    snippet = am.synth_pcm16_stereo_device(dev, S, 7, 0, amp=0.5)
    needle = am.DeviceBuffer(dev, 4 * S)
    am._check(L.am_pcm_s16_stereo_to_mono_device(dev, snippet.ptr, S, needle.ptr))
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    hay = am.synth_pcm16_stereo_device(dev, H, 7, 1, amp=0.1)
    planted = [600 * SR * m + 30 * SR for m in range(6)]
    for t in planted:
        am.add_pcm16_device(dev, hay, t, snippet.ptr, S)
    starts = planted + [int(rng.integers(0, H - S)) for _ in range(HITS - len(planted))]
    n = len(starts)
    pk = (am.AmPeak * n)(*[am.AmPeak(t, t + 1, 0.0, 0.0) for t in starts])
    sp = am.AmStereoParams(RADIUS, 0)
    out = (am.HitStereo * n)()
    _, med, mn, kms = hsb.timed(lambda: am._check(L.am_hit_stereo_device(algo._h, hay.ptr, H, 1, pk, n, C.byref(sp), out)), a.reps, a.warmup, dev)
    for i in range(len(planted)):
        assert out[i].ncc_mid > 0.5 and am.hit_stereo_summary(out[i], 0.5).image == am.AM_IMAGE_CENTRE, (i, out[i])
    stereo = {"radius": RADIUS, "call_us_per_hit_median": 1e3 * med / n, "call_us_per_hit_min": 1e3 * mn / n, "kernel_us_per_hit_median": 1e3 * kms / n}

    # the baseline: f32 copies of L and R, one am_hit_segments_device call (m = 1) on each
    left, right = am.DeviceBuffer(dev, 4 * H), am.DeviceBuffer(dev, 4 * H)
    passes = clocked(lambda: (am.pcm_s16_stereo_mix_device(dev, hay.ptr, H, 1.0, 0.0, left.ptr),
                              am.pcm_s16_stereo_mix_device(dev, hay.ptr, H, 0.0, 1.0, right.ptr)), a.reps, a.warmup)
    sg = am.AmSegmentParams(1, RADIUS)
    seg = (am.HitSegment * n)()

    def two_calls():
        am._check(L.am_hit_segments_device(algo._h, left.ptr, H, 0, pk, n, C.byref(sg), seg))
        am._check(L.am_hit_segments_device(algo._h, right.ptr, H, 0, pk, n, C.byref(sg), seg))

    _, smed, smn, skms = hsb.timed(two_calls, a.reps, a.warmup, dev)
    baseline = {"calls": 2, "segments": 1, "radius": RADIUS, "call_us_per_hit_median": 1e3 * smed / n, "call_us_per_hit_min": 1e3 * smn / n,
                "kernel_us_per_hit_median": 1e3 * skms / n, "two_pcm_passes": passes}
    right.free()

    # the mix against the down-mix on the same buffer
    mix = clocked(lambda: am.pcm_s16_stereo_mix_device(dev, hay.ptr, H, 0.5, -0.5, left.ptr), a.reps, a.warmup)
    mono = clocked(lambda: am._check(L.am_pcm_s16_stereo_to_mono_device(dev, hay.ptr, H, left.ptr)), a.reps, a.warmup)
    left.free()
    hay.free()
    print(json.dumps({"shape": f"needle {S} samples (10 s at 44.1 kHz), one resident 1 h i16 stereo haystack, {n} hits, radius {RADIUS}",
                      "reps": a.reps, "hit_stereo": stereo, "baseline_two_segments_calls": baseline,
                      "kernel_ratio_to_baseline": kms / skms if skms > 0 else None, "call_ratio_to_baseline": med / smed,
                      "pcm_1h": {"stereo_mix_device": mix, "stereo_to_mono_device": mono, "frames": H}}))


if __name__ == "__main__":
    main()
