#!/usr/bin/env python3
"""Window-energy normalised scores (option "score_norm", NCC) against the default LIB scores on the headline
shape: a 10 s needle and 8 x 1 h 44.1 kHz f32 haystacks through am_match_batch_device.  Host clocks around calls that
end in a device synchronise; the planted offsets are checked in every timed call.  Prints one JSON line.

  python tools/score_norm_bench.py [--reps R] [--warmup W] [--only ncc|lib]
(--only ncc with few reps is the run to put under a kernel trace.)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

SR = 44100
S = 10 * SR
H = 3600 * SR
NH = 8


def plants(k):
    return [600 * SR * m + 30 * SR + 17 * k + 1234 for m in range(6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("ncc", "lib"), default=None)
    a = ap.parse_args()
    dev = 0
    needle = am.synth_uniform_device(dev, S, 1, 0)
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    p = am.Config(chunk_size_s=60, overlap_length_s=10, distance_s=480.0, prominence=0.13).params(SR, am.Scale.LIB)
    hays = []
    for k in range(NH):
        b = am.synth_uniform_device(dev, H, 1, k + 1)
        for t in plants(k):
            am.axpy_device(dev, b, t, needle.ptr, S, 1.0)
        hays.append(b)
    ptrs, lens = [b.ptr for b in hays], [H] * NH
    out = {"shape": f"needle {S} samples, {NH} x {H} samples (1 h at 44.1 kHz), am_match_batch_device", "reps": a.reps}
    for name, norm in (("lib", 0), ("ncc", 1)):
        if a.only and a.only != name:
            continue
        algo.set_option("score_norm", norm)
        for _ in range(a.warmup):
            algo.match_batch_device(ptrs, lens, p)
        ts = []
        heights = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = algo.match_batch_device(ptrs, lens, p)
            ts.append(time.perf_counter() - t0)
            assert all([q.start for q in r] == plants(k) for k, r in enumerate(res)), name
            heights = [q.height for r in res for q in r]
        ts.sort()
        med = ts[len(ts) // 2]
        out[name] = {"ms_per_hour_median": med / NH * 1e3, "ms_per_hour_min": ts[0] / NH * 1e3,
                     "height_min": min(heights), "height_max": max(heights)}
    if "lib" in out and "ncc" in out:
        out["ncc_over_lib"] = out["ncc"]["ms_per_hour_median"] / out["lib"]["ms_per_hour_median"]
    algo.set_option("score_norm", -1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
