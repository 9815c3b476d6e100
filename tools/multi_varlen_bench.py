#!/usr/bin/env python3
"""Several needles of different lengths (am_match_multi_varlen_batch_device) on one GPU: 32 needles of seeded lengths
3-12 s at 44.1 kHz against 8 distinct 1 h haystacks, in ms per needle-hour, against
  (b) am_match_multi_batch_device with 32 needles of 12 s (the equal-length engine at the longest length),
  (c) 32 am_match_batch_device calls, one per needle (no sharing).
Prints one JSON object with the three rates, the ratios the issue asks about and the per-kernel breakdown (HIP events)
of (a) and (b).  --lean: one timed call per case (for a kernel trace under rocprofv3)."""
import json
import sys
import time

sys.path.insert(0, "audio-matcher_amd/python"); sys.path.insert(0, "audio-matcher_amd")
import numpy as np
import audiomatch_amd as am

dev = 0
SR = 44100
H = 3600 * SR
NN, NH = 32, 8
lean = "--lean" in sys.argv
rng = np.random.default_rng(2024)
lens_n = [int(x) for x in rng.integers(3 * SR, 12 * SR + 1, size=NN)]
p = am.Config(chunk_size_s=60, overlap_length_s=10, distance_s=480.0, prominence=0.13).params(SR, am.Scale.LIB)
needles = [am.synth_uniform_device(dev, s, 1, 3001 + j) for j, s in enumerate(lens_n)]
algos = [am.HipConvolve.from_device(dev, n.ptr, s) for n, s in zip(needles, lens_n)]
needles12 = [am.synth_uniform_device(dev, 12 * SR, 1, 4001 + j) for j in range(NN)]
algos12 = [am.HipConvolve.from_device(dev, n.ptr, 12 * SR) for n in needles12]
hays = [am.synth_uniform_device(dev, H, 1, 10 + k) for k in range(NH)]
plants = {}
for k, hay in enumerate(hays):
    for j in range(NN):
        t = (97 * j + 311 * k) % 3400 * SR + 1000 * j + 777   # (off the chunk edges, where a hit is no peak)
        am.axpy_device(dev, hay, t, needles[j].ptr, lens_n[j], 1.0)
        am.axpy_device(dev, hay, t + 7 * SR, needles12[j].ptr, 12 * SR, 1.0)
        plants[(k, j)] = t
ptrs, lens = [h.ptr for h in hays], [H] * NH

# every needle with an overlap of its own length, as the CLI sets it (windows without gaps between them)
p12 = am.AmMatchParams.from_buffer_copy(p)
p12.overlap = 12 * SR
p_own = []
for s in lens_n:
    q = am.AmMatchParams.from_buffer_copy(p)
    q.overlap = s
    p_own.append(q)
cases = {
    "a_varlen": lambda: am.match_multi_varlen_batch_device(algos, ptrs, lens, p, overlaps=lens_n),
    "b_multi_12s": lambda: am.match_multi_batch_device(algos12, ptrs, lens, p12),
    "c_single_calls": lambda: [a.match_batch_device(ptrs, lens, q) for a, q in zip(algos, p_own)],
}
res = cases["a_varlen"]()
assert all(plants[(k, j)] in [q.start for q in res[k][j]] for k in range(NH) for j in range(NN))
KN = ("k1_cols_fwd", "k2_rows", "k3_cols_inv", "tile_stats", "peaks")
out = {"needles": NN, "haystacks": NH, "needle_lengths_s": [round(s / SR, 3) for s in lens_n]}
for name, fn in cases.items():
    for _ in range(1 if lean else 3):
        fn()                                            # clock ramp + sparse-score state
    reps = 1 if lean else 5
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = (time.perf_counter() - t0) / reps
    entry = {"ms_per_call": dt * 1e3, "ms_per_needle_hour": dt * 1e3 / (NN * NH)}
    if name != "c_single_calls" and not lean:
        with am.Profile(dev) as prof:
            fn()
            entry["kernel_ms_per_call"] = {n: round(prof.query(n)[0], 3) for n in KN}
    out[name] = entry
a, b, c = (out[k]["ms_per_needle_hour"] for k in ("a_varlen", "b_multi_12s", "c_single_calls"))
out["a_over_b"] = a / b
out["a_over_c"] = a / c
print(json.dumps(out, indent=1))
