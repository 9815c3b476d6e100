#!/usr/bin/env python3
"""Sample-rate conversion (am_resample_device, am_needle_create_resampled) at the sizes users run.

  hay48    1 h of 48 kHz i16 stereo -> 44.1 kHz f32 mono (a broadcast archive brought to the needle's rate)
  hay44    1 h of 44.1 kHz f32 -> 48 kHz f32
  needle   creating a 10 s 44.1 kHz needle for 48 kHz haystacks (am_needle_create_resampled) against a plain
           am_needle_create of the same samples

Per haystack row: the kernel time of every call (device events around the launch: am_profile_*, the "other" class;
median and min of --reps calls after --warmup), the call's time (host clock around the C entry point, which ends in a
device synchronise), bytes in + out (4 per frame / sample in, 4 per sample out) and those bytes over the kernel time
against 8 TB/s.  Prints one JSON line.

  python tools/resample_bench.py [--reps R] [--warmup W]"""
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

PEAK_BW = 8.0e12
DEV = 0


def median_min(v):
    v = sorted(v)
    return v[len(v) // 2], v[0]


def hay_row(name, src, dst, fmt, din, n_in, reps, warmup):
    lib = am.lib()
    n_out = am.resample_len(n_in, src, dst)
    dout = am.DeviceBuffer(DEV, 4 * n_out)
    got = C.c_size_t(0)

    def call():
        rc = lib.am_resample_device(DEV, din.ptr, n_in, int(fmt), src, dst, dout.ptr, n_out, C.byref(got))
        assert rc == 0 and got.value == n_out, (rc, got.value)

    for _ in range(warmup):
        call()
    ks, ts = [], []
    for _ in range(reps):
        with am.Profile(DEV) as prof:
            call()
        ks.append(prof.query("other")[0])
    for _ in range(reps):   # (host-clock calls without the profiling events)
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    k_med, k_min = median_min(ks)
    c_med, c_min = median_min(ts)
    nbytes = 4.0 * n_in + 4.0 * n_out
    dout.free()
    return {"case": name, "src_rate": src, "dst_rate": dst, "format": "i16_stereo" if fmt else "f32", "n_in": n_in,
            "n_out": n_out, "kernel_ms_median": k_med, "kernel_ms_min": k_min, "call_ms_median": c_med, "call_ms_min": c_min,
            "bytes": nbytes, "floor_ms_8TBps": nbytes / PEAK_BW * 1e3,
            "bytes_per_s_kernel": nbytes / (k_med * 1e-3), "fraction_of_8TBps_kernel": nbytes / (k_med * 1e-3) / PEAK_BW}


def needle_row(reps, warmup):
    src, dst = 44100, 48000
    x = np.random.default_rng(1).uniform(-0.5, 0.5, 10 * src).astype(np.float32)
    lib = am.lib()

    def make(resampled):
        h = C.c_void_p()
        if resampled:
            rc = lib.am_needle_create_resampled(DEV, x.ctypes.data, x.size, 0, src, dst, C.byref(h))
        else:
            rc = lib.am_needle_create(DEV, x.ctypes.data, x.size, C.byref(h))
        assert rc == 0
        lib.am_needle_destroy(h)

    out = {"case": "needle", "needle_s": 10, "src_rate": src, "dst_rate": dst}
    for key, flag in (("plain", False), ("resampled", True)):
        for _ in range(warmup):
            make(flag)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            make(flag)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[key + "_ms_median"], out[key + "_ms_min"] = median_min(ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if am.device_count() < 1:
        raise SystemExit("resample_bench needs a HIP device")
    rows = []
    frames = 3600 * 48000
    din = am.synth_pcm16_stereo_device(DEV, frames, 7, 1, amp=0.5)
    rows.append(hay_row("hay48", 48000, 44100, am.Fmt.S16_STEREO, din, frames, a.reps, a.warmup))
    din.free()
    n = 3600 * 44100
    din = am.synth_uniform_device(DEV, n, 7, 2, amp=0.5)
    rows.append(hay_row("hay44", 44100, 48000, am.Fmt.F32_MONO, din, n, a.reps, a.warmup))
    din.free()
    rows.append(needle_row(a.reps, a.warmup))
    print(json.dumps({"bench": "resample", "reps": a.reps, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
