"""The checker of per-band hit scoring (am_hit_bands*, am_hit_bands_summary, am_band_edges_log): a plain numpy f64
implementation of the definition in include/audiomatch.h (np.fft.rfft per frame), flags included.  A module, not a test
file; the tests import it."""
import ctypes
import math
import struct
from dataclasses import dataclass

import numpy as np

BELOW, NONFIN, EMPTY = 2, 4, 128
EMPTY_DB = 90
MAX_BANDS = 32


@dataclass
class BandRef:
    ncc: float
    coherence: float
    gain: float
    level_db: float
    needle_share: float
    flags: int


FIELDS = ("ncc", "coherence", "gain", "level_db", "needle_share")


def frame_count(s, frame_log2):
    f = 1 << frame_log2
    return (s - f) // (f // 2) + 1


def span(s, frame_log2):
    """The samples a hit reads, counted from its start: (J - 1) H + F."""
    f = 1 << frame_log2
    return (frame_count(s, frame_log2) - 1) * (f // 2) + f


def window(f):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(f, dtype=np.float64) / f)


def cross_spectra(x, needle, t, frame_log2, transform=np.fft.rfft):
    """P_xn, P_xx, P_nn over the bins 0 .. F / 2 of a hit at t, frames added in order."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n64 = np.asarray(needle, dtype=np.float32).astype(np.float64)
    f = 1 << frame_log2
    h = f // 2
    w = window(f)
    pxn = np.zeros(h + 1, dtype=np.complex128)
    pxx = np.zeros(h + 1)
    pnn = np.zeros(h + 1)
    for j in range(frame_count(len(n64), frame_log2)):
        xs = transform(w * x64[t + j * h:t + j * h + f])
        ns = transform(w * n64[j * h:j * h + f])
        pxn += xs * np.conj(ns)
        pxx += xs.real ** 2 + xs.imag ** 2
        pnn += ns.real ** 2 + ns.imag ** 2
    return pxn, pxx, pnn


def dft_direct(v):
    """The O(F^2) transform of the definition, bins 0 .. F / 2."""
    f = len(v)
    k = np.arange(f // 2 + 1, dtype=np.float64)[:, None]
    i = np.arange(f, dtype=np.float64)[None, :]
    return np.exp(-2j * np.pi * ((k * i) % f) / f) @ np.asarray(v, dtype=np.float64)


def bands_ref(x, needle, t, frame_log2, edges, floor_db=60, transform=np.fft.rfft):
    """The B BandRef records of a hit at t in f32 samples x against the f32 needle."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n64 = np.asarray(needle, dtype=np.float32).astype(np.float64)
    s, f, nb = len(n64), 1 << frame_log2, len(edges) - 1
    assert s >= f and t + s <= len(x64) and 1 <= nb <= MAX_BANDS
    assert all(edges[b] < edges[b + 1] for b in range(nb)) and edges[nb] <= f // 2 + 1
    read = span(s, frame_log2)
    if not (np.all(np.isfinite(x64[t:t + read])) and np.all(np.isfinite(n64[:read]))):
        return [BandRef(np.nan, np.nan, np.nan, np.nan, np.nan, NONFIN) for _ in range(nb)]
    pxn, pxx, pnn = cross_spectra(x64, n64, t, frame_log2, transform)
    en_all = float(pnn.sum())
    ratio = 10.0 ** (-floor_db / 10.0)
    out = []
    for b in range(nb):
        lo, hi = edges[b], edges[b + 1]
        c, ex, en = complex(pxn[lo:hi].sum()), float(pxx[lo:hi].sum()), float(pnn[lo:hi].sum())
        share = en / en_all if en_all > 0 else 0.0
        if share < 10.0 ** (-EMPTY_DB / 10.0):
            out.append(BandRef(0.0, 0.0, 0.0, np.inf if ex > 0 else np.nan, share, EMPTY))
            continue
        gain = c.real / en
        level = -np.inf if ex == 0 else 10.0 * math.log10(ex / en)
        if ex == 0 or ex < en * ratio:
            out.append(BandRef(0.0, 0.0, gain, level, share, BELOW))
        else:
            den = math.sqrt(ex * en)
            out.append(BandRef(c.real / den, abs(c) / den, gain, level, share, 0))
    return out


def summary_ref(recs, min_coherence):
    """am_hit_bands_summary of one hit's records (anything with the fields of am_hit_band): a dict."""
    countable = [b for b, q in enumerate(recs) if not q.flags & (NONFIN | EMPTY)]
    present = [b for b in countable if not recs[b].flags & BELOW and recs[b].coherence >= min_coherence]
    total = sum(float(recs[b].needle_share) for b in countable)
    held = sum(float(recs[b].needle_share) for b in present)
    coh = sum(float(recs[b].needle_share) * float(recs[b].coherence) for b in countable)
    gains = [20.0 * math.log10(float(recs[b].gain)) for b in present if recs[b].gain > 0]
    return dict(coverage=held / total if total != 0 else np.nan, weighted_coherence=coh / total if total != 0 else np.nan,
                gain_db_spread=max(gains) - min(gains) if len(gains) >= 2 else np.nan,
                first_present=present[0] if present else -1, last_present=present[-1] if present else -1,
                n_present=len(present), n_countable=len(countable))


def edges_log_ref(sr, frame_log2, lo_hz, hi_hz, n_bands):
    """am_band_edges_log: the B + 1 edges, or None where the library refuses."""
    if not (sr > 0 and 8 <= frame_log2 <= 12 and 1 <= n_bands <= MAX_BANDS and lo_hz > 0 and hi_hz > lo_hz and hi_hz <= sr / 2):
        return None
    f = 1 << frame_log2
    edges, prev = [], -1
    for b in range(n_bands + 1):
        e = max(int(math.floor(lo_hz * (hi_hz / lo_hz) ** (b / n_bands) * f / sr + 0.5)), prev + 1)   # (llround of a positive value)
        edges.append(e)
        prev = e
    return edges if prev <= f // 2 + 1 else None


def f32_ulps(a, b):
    """How many f32 values lie between a and b (both taken as f32); 0 for equal infinities or two NaNs."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 31
    if a == b:
        return 0
    if np.isinf(a) or np.isinf(b):
        return 1 << 31

    def key(v):
        i = struct.unpack("<i", struct.pack("<f", v))[0]
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def close(got, want, ulps=2, abs_tol=1e-9):
    """A float field against the checker's f64 value: within `ulps` f32 ulps of it rounded to f32, plus abs_tol."""
    if f32_ulps(got, want) <= ulps:
        return True
    got, want = float(np.float32(got)), float(np.float32(want))
    if not (math.isfinite(got) and math.isfinite(want)):
        return False
    lo, hi = np.float32(want), np.float32(want)
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    return float(lo) - abs_tol <= got <= float(hi) + abs_tol


def assert_records(got, ref):
    """got: the library's records of one hit, ref: bands_ref's.  Flags equal, every float field close()."""
    assert len(got) == len(ref)
    for b, (g, e) in enumerate(zip(got, ref)):
        assert g.flags == e.flags, (b, g, e)
        for name in FIELDS:
            assert close(getattr(g, name), getattr(e, name)), (b, name, g, e)


def bits(hit_records):
    """The records of one hit, byte for byte."""
    return [bytes(q) if isinstance(q, ctypes.Structure) else
            struct.pack("<fffffI", q.ncc, q.coherence, q.gain, q.level_db, q.needle_share, q.flags) for q in hit_records]
