"""Raw device-form calls of the per-hit families, for tests/test_gpu_hit_launch_edges.py: the peaks go in as one numpy
table and the records come back as bytes, one row per hit, so that a call of 65,600 hits costs no Python object per
record and two calls compare with one array comparison.  A module, not a test file."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "audio-matcher_amd", "csrc")
PEAK = np.dtype([("start", "<u8"), ("end", "<u8"), ("height", "<f4"), ("prominence", "<f4")])   # am_peak


def constant(source, pattern):
    """The integer that `pattern` (one group) finds in a file of the library's sources."""
    return int(re.search(pattern, open(os.path.join(CSRC, source)).read()).group(1))


SLICE = constant("am_kernels.h", r"constexpr int kHitSlice = (\d+);")
SIG_SLICE = constant("am_kernels.h", r"constexpr int kSigSlice = (\d+);")
GRID_Y = constant("am_kernels.h", r"constexpr long long kHitMaxGridY = (\d+);")          # rows of one launch


def noise(seed, n, amp=0.25):
    return (np.random.default_rng(seed).uniform(-amp, amp, n)).astype(np.float32)


def device_call(am, symbol, record, m, algo, ptr, length, fmt, ts, params=None, taps=0):
    """symbol + "_device" for the hits that start at ts: uint8 [len(ts), m * sizeof(record) + 4 * taps], row i the m
    records of hit i (for am_hit_channel, taps = 2 P + 1: its f32 taps behind its record)."""
    n = len(ts)
    pk = np.zeros(n, dtype=PEAK)
    pk["start"] = ts
    pk["end"] = pk["start"] + 1
    out = np.zeros((n, m * C.sizeof(record)), dtype=np.uint8)
    args = [algo._h, ptr, length, int(fmt), pk.ctypes.data_as(C.POINTER(am.AmPeak)), n]
    if params is not None:
        args.append(C.byref(params))
    args.append(out.ctypes.data_as(C.POINTER(record)))
    tp = np.zeros((n, taps), dtype=np.float32)
    if taps:
        args.append(tp.ctypes.data)
    am._check(getattr(am.lib(), symbol + "_device")(*args))
    return np.concatenate([out, tp.view(np.uint8)], axis=1) if taps else out


def in_small_calls(call, ts, which, step=1000):
    """call(ts of at most `step` hits) for the hits `which` (ascending indices into ts), call after call: (rows, have) --
    rows[i] the bytes of hit i, have[i] whether hit i was among them."""
    ts = np.asarray(ts)
    which = np.asarray(which)
    rows, have = None, np.zeros(len(ts), dtype=bool)
    for k in range(0, len(which), step):
        idx = which[k:k + step]
        got = call(ts[idx])
        if rows is None:
            rows = np.zeros((len(ts), got.shape[1]), dtype=np.uint8)
        rows[idx] = got
        have[idx] = True
    return rows, have


def records(record, row, m=1):
    """The m records a row of device_call holds, as copies."""
    size = C.sizeof(record)
    return [record.from_buffer_copy(row[j * size:(j + 1) * size].tobytes()) for j in range(m)]


def checked_hits(n_hits, rows_per_hit):
    """The hits a large call is checked at: the first eight, those that own the rows around the first launch's end
    (GRID_Y - 15 .. GRID_Y + 15) and the last eight."""
    seam = range((GRID_Y - 15) // rows_per_hit, (GRID_Y + 15) // rows_per_hit + 1)
    return sorted(set(range(8)) | set(seam) | set(range(n_hits - 8, n_hits)))


# ---- the slice-edge cases of am_hit_segments (settled on the CPU: every margin of the checker exceeds 1e-9) ---------------
SEG_EDGE_SHAPES = ((SLICE, 1), (SLICE + 1, 1), (2 * SLICE + 1, 2), (3 * SLICE - 1, 3), (3 * SLICE, 3), (3 * SLICE + 1, 3))
SEG_EDGE_RADII = (0, 1, 4, 16)
SEG_EDGE_TAIL, SEG_EDGE_PLANT = 6000, 3000


def seg_edge_case(s, r):
    """(needle, hay, ts): a haystack of S + 6000 samples of white noise, the needle planted at 3000; the hits: t = 0,
    t = R - 1 (the left lags clipped in part), t = len - S, the plant, two samples before and behind it."""
    needle = noise(700 + s, s, 0.5)
    hay = noise(800 + s, s + SEG_EDGE_TAIL, 0.1)
    hay[SEG_EDGE_PLANT:SEG_EDGE_PLANT + s] += np.float32(0.7) * needle
    ts = [0] + ([r - 1] if r > 1 else []) + [SEG_EDGE_TAIL, SEG_EDGE_PLANT, SEG_EDGE_PLANT + 2, SEG_EDGE_PLANT - 2]
    return needle, hay, ts
