#!/usr/bin/env python3
"""Per-hit significance (am_hit_significance_device) on the headline needle: a 10 s needle at 44.1 kHz, guard S - 1,
radius 30 s, 64 hits in one resident 1 h f32 haystack (six planted, the rest at seeded random offsets, none clipped),
beside am_correlate_device (AM_MODE_VALID, AM_SCALE_LIB) on ONE span of the same length -- what the definition says a
hit's scores are.

Reported: the call's time per hit (host clock around the C entry point on prebuilt arguments, median and min of
--reps), the device time of the transform kernels and of the reduction kernels per hit (device events, am_profile_*:
classes k1_cols_fwd + k2_rows + k3_cols_inv, and "other" = the four sig_* kernels of a call with these options), the
reduction's share of the call, the one-span am_correlate_device call, and the ratio of the two.  The planted hits are
checked (z > 100).  Prints one JSON line.

  python tools/hit_significance_bench.py [--reps R] [--warmup W] [--hits N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

SR = 44100
S = 10 * SR
H = 3600 * SR
B = 30 * SR
KERNELS = ("k1_cols_fwd", "k2_rows", "k3_cols_inv", "other")


def timed(fn, reps, warmup, dev):
    """(median ms, min ms, {kernel class: median device ms}) of fn; the events are in calls of their own."""
    for _ in range(warmup):
        fn()
    ts, ks = [], {k: [] for k in KERNELS}
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    for _ in range(reps):
        with am.Profile(dev) as prof:
            fn()
        for k in KERNELS:
            ks[k].append(prof.query(k)[0])
    ts.sort()
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, {k: sorted(v)[len(v) // 2] for k, v in ks.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hits", type=int, default=64)
    a = ap.parse_args()
    dev = 0
    rng = np.random.default_rng(1)
    needle = am.synth_uniform_device(dev, S, 7, 0, amp=0.5)
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    hay = am.synth_uniform_device(dev, H, 7, 1, amp=0.1)
    planted = [600 * SR * m + 45 * SR for m in range(6)]
    for t in planted:
        am.axpy_device(dev, hay, t, needle.ptr, S, 1.0)
    starts = (planted + [int(t) for t in rng.integers(B, H - S - B, max(0, a.hits - len(planted)))])[:a.hits]
    n = len(starts)
    L = am.lib()
    pk = (am.AmPeak * n)(*[am.AmPeak(t, t + 1, 0.0, 0.0) for t in starts])
    out = (am.HitSignificance * n)()
    sp = am.AmSignificanceParams(S - 1, B)
    med, mn, ks = timed(lambda: am._check(L.am_hit_significance_device(algo._h, hay.ptr, H, 0, pk, n, C.byref(sp), out)),
                        a.reps, a.warmup, dev)
    for i, t in enumerate(starts):
        assert out[i].flags == 0 and out[i].n_bg == 2 * (B - S + 1), (t, out[i])
        if t in planted:
            assert out[i].z > 100, (t, out[i])
    zs = [out[i].z for i in range(n)]
    transforms = ks["k1_cols_fwd"] + ks["k2_rows"] + ks["k3_cols_inv"]
    # one equal span through am_correlate_device
    span = 2 * B + S
    scores = am.DeviceBuffer(dev, 4 * (2 * B + 1))
    got = C.c_size_t(0)
    lo = planted[1] - B
    cmed, cmn, cks = timed(lambda: am._check(L.am_correlate_device(algo._h, hay.ptr + 4 * lo, span, int(am.Mode.Valid), int(am.Scale.LIB),
                                                                   scores.ptr, 2 * B + 1, C.byref(got))), a.reps, a.warmup, dev)
    assert got.value == 2 * B + 1
    scores.free()
    hay.free()
    print(json.dumps({
        "shape": f"needle {S} samples (10 s at 44.1 kHz), guard {S - 1}, radius {B} (30 s), {n} hits in one resident 1 h f32 haystack; "
                 f"span {span} samples, zone {2 * B + 1} scores per hit",
        "reps": a.reps,
        "hit_significance": {
            "call_ms_median": med, "call_ms_min": mn, "call_ms_per_hit_median": med / n, "call_ms_per_hit_min": mn / n,
            "transform_kernels_ms_per_hit": transforms / n, "reduction_kernels_ms_per_hit": ks["other"] / n,
            "reduction_share_of_call": ks["other"] / med, "reduction_share_of_kernels": ks["other"] / (transforms + ks["other"]),
            "z_planted_min": min(z for z, t in zip(zs, starts) if t in planted),
            "abs_z_elsewhere_max": max([abs(z) for z, t in zip(zs, starts) if t not in planted] or [0.0])},
        "correlate_one_span": {"call_ms_median": cmed, "call_ms_min": cmn,
                               "transform_kernels_ms": cks["k1_cols_fwd"] + cks["k2_rows"] + cks["k3_cols_inv"]},
        "hit_over_correlate": (med / n) / cmed}))


if __name__ == "__main__":
    main()
