#!/usr/bin/env python3
"""Live monitoring (am_monitor_*) on one GPU: catch-up throughput and per-group latency.

One hour of 44.1 kHz audio with a 10 s needle planted every few minutes, pushed in 1 s pieces through a monitor with
G = 1 and G = 8 windows per group, against am_match on the same hour (host buffer).  Catch-up: hour of audio per wall
second (the real-time factor).  Latency: wall time of the push that completes a group (it matches the group) plus the
poll that hands out what became final.  Writes profiles/r10/monitor_bench.json (or the path given)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

SR = 44100
S = 10 * SR
H = 3600 * SR
PLANT = [int((37 + 311 * k) * SR) for k in range(11)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10", "monitor_bench.json")
    rng = np.random.default_rng(5)
    needle = (rng.random(S, dtype=np.float32) - 0.5) * 0.5
    hay = (rng.random(H, dtype=np.float32) - 0.5) * 0.5
    for t in PLANT:
        hay[t:t + S] += needle
    # the reference's defaults (60 s chunks, overlap = the snippet) with a monitoring distance of 30 s
    p = am.Config(chunk_size_s=60.0, overlap_length_s=10.0, distance_s=30.0, prominence=0.13).params(SR, am.Scale.LIB)
    algo = am.HipConvolve(needle)
    res = {"audio_s": H / SR, "needle_s": S / SR, "push_s": 1.0, "params": {"chunk": p.chunk, "overlap": p.overlap,
                                                                          "distance_s": p.overshadow_distance_s}}
    for _ in range(3):
        whole = algo.match(hay, p)
    assert [q.start for q in whole] == PLANT, [q.start for q in whole]
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        algo.match(hay, p)
    dt = (time.perf_counter() - t0) / reps
    res["am_match"] = {"s_per_hour": dt, "realtime_x": (H / SR) / dt}
    for G in (1, 8):
        for attempt in range(2):      # the first pass warms plans and buffers for this group length
            m = am.HipMonitor([algo], p, group_windows=G)
            got, lat = [], []
            t0 = time.perf_counter()
            for a in range(0, H, SR):
                h0 = m.info().horizon
                t1 = time.perf_counter()
                got += m.push(hay[a:a + SR])
                t2 = time.perf_counter()
                if m.info().horizon != h0:
                    lat.append(t2 - t1)
            got += m.end()
            dt = time.perf_counter() - t0
            info = m.info()
            m.close()
        assert [q.start for _, q in got] == PLANT, [q.start for _, q in got]
        lat_ms = np.array(lat) * 1e3
        res[f"monitor_G{G}"] = {
            "s_per_hour": dt, "realtime_x": (H / SR) / dt, "vs_am_match": dt / res["am_match"]["s_per_hour"],
            "groups": len(lat), "group_latency_ms": {"median": float(np.median(lat_ms)), "p95": float(np.percentile(lat_ms, 95)),
                                                     "max": float(lat_ms.max())},
            "resident_bytes": info.resident_bytes}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
