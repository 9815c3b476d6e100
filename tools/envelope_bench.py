#!/usr/bin/env python3
"""Envelope matching (am_match_envelope_device) on a resident hour: 1 h of f32 at 44.1 kHz, a 10 s needle of noise
bursts planted 3 % long, F = 1024, 8 log bands 150 - 6000 Hz, +-5 % in 101 speeds.

Whole calls are timed by the host clock around calls that end in a device synchronise (median, min and max of --reps
after --warmup); one profiled call gives the kernel time of the three profile classes (envelope_frames: the levels of
the needle at every speed and of the haystack; envelope_prefix: the needle bank's sums and the haystack's prefix sums;
envelope_correlate: the one correlation launch).  One plain am_match_device of the same haystack with the same needle
stands beside it for scale.  Prints one JSON line.

  python tools/envelope_bench.py [--reps R] [--warmup W] [--seconds S] [--out FILE]"""
import argparse
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


def clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def spread(ts, name):
    return {name + "_ms": round(float(np.median(ts)), 3), name + "_min_ms": round(float(np.min(ts)), 3),
            name + "_max_ms": round(float(np.max(ts)), 3)}


def burst_noise(rng, n):
    """Noise switched on and off every 50 - 250 ms: a needle whose envelope has something to hold on to."""
    x = rng.standard_normal(n) * 0.3
    at, on = 0, True
    while at < n:
        ln = int(rng.uniform(0.05, 0.25) * SR)
        if not on:
            x[at:at + ln] *= 0.02
        at, on = at + ln, not on
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(25)
    length = a.seconds * SR
    needle = burst_noise(rng, 10 * SR)
    drift, at = 30000.0, (a.seconds // 3) * SR + 321
    r = 1.0 + drift * 1e-6
    m = int((needle.size - 1) * r) + 1
    plant = np.interp(np.arange(m) / r, np.arange(needle.size), needle).astype(np.float32)
    hay = am.synth_uniform_device(0, length, seed=25, stream=1, amp=0.02)
    dplant = am.DeviceBuffer.from_numpy(0, plant)
    am.axpy_device(0, hay, at, dplant.ptr, plant.size, 1.0)
    algo = am.HipConvolve(needle)
    ep = am.env_params(am.band_edges_log(SR, 10, 150.0, 6000.0, 8))
    grid = am.env_grid(50000.0, 50)
    hits = []

    def envelope():
        hits[:] = [algo.match_envelope_device(hay.ptr, length, ep, grid, 0.4)]

    params = am.Config().params(SR, am.Scale.LIB)
    t_env = clock(envelope, a.reps, a.warmup)
    t_match = clock(lambda: algo.match_device(hay.ptr, length, params), a.reps, a.warmup)
    with am.Profile(0) as p:
        envelope()
        parts = {k: p.query("envelope_" + k) for k in ("frames", "prefix", "correlate")}
        total_ms, launches = p.query("envelope")
    got = hits[0]
    j_needle = am.envelope_len(needle.size, ep, 0.0)
    j_hay = am.envelope_len(length, ep, 0.0)
    frames_all = sum(am.envelope_len(needle.size, ep, float(d)) for d in am.env_grid_drifts(grid))
    found = [h for h in got if abs(int(h["start"]) - at) <= 4 * 512]
    res = dict(shape=dict(sr=SR, hay_seconds=a.seconds, needle_seconds=10, frame=1024, bands=8, speeds=101, max_ppm=50000,
                          hay_frames=j_hay, needle_frames=j_needle),
               unit="ms per call",
               **spread(t_env, "match_envelope_device"), **spread(t_match, "match_device"),
               kernels_ms=round(total_ms, 3), kernel_launches=int(launches),
               frames_ms=round(parts["frames"][0], 3), prefix_ms=round(parts["prefix"][0], 3), correlate_ms=round(parts["correlate"][0], 3),
               frame_transforms=int(frames_all + j_hay), multiply_adds=int(8 * frames_all * max(j_hay - j_needle + 1, 0)),
               hits=int(got.size), planted_found=bool(found),
               planted=dict(start_off_samples=int(found[0]["start"]) - at, drift_ppm=float(found[0]["drift_ppm"]),
                            score=round(float(found[0]["score"]), 4)) if found else None)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
