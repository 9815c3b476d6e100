"""ctypes host binding of libaudiomatch_amd.so (MI355X / gfx950).

Mirrors the reference's matcher interface (src/matcher/audio_matcher.rs):

    LibConvolve::new(sample)                 -> HipConvolve(sample)
    algo.inverse_sample_auto_correlation()   -> HipConvolve.inverse_sample_auto_correlation()
    algo.correlate_with_sample(w, mode, sc)  -> HipConvolve.correlate_with_sample(w, mode, scale)
    calc_chunks(sr, samples, &algo, scale, config)
                                             -> calc_chunks(sr, samples, algo, scale, config)

Every call goes through the C ABI of include/audiomatch.h; there is no Python
or CPU implementation behind it.  Importing this module fails loudly when the
HIP library is missing or cannot be loaded.
"""
from __future__ import annotations

import ctypes as C
import struct
import enum
import os
from dataclasses import dataclass

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.abspath(os.path.join(_PKG, "..", ".."))
LIB_PATH = os.path.join(_ROOT, "libaudiomatch_amd.so")

AM_OK, AM_ERR_INVALID_ARG, AM_ERR_CAPACITY, AM_ERR_HIP, AM_ERR_NO_DEVICE, \
    AM_ERR_PEAK_OVERFLOW, AM_ERR_OOM = range(7)
AM_MAX_PEAKS_PER_CHUNK = 1024


class Fmt(enum.IntEnum):           # sample format of a haystack buffer (AM_FMT_*)
    F32_MONO = 0
    S16_STEREO = 1                 # interleaved i16 stereo frames (mp3_reader.rs:26-37)


class Mode(enum.IntEnum):          # audio_matcher.rs:55-59
    Full = 0
    Same = 1
    Valid = 2


class Scale(enum.IntEnum):
    NONE = 0
    LIB = 1                        # LibConvolve, production (audio_matcher.rs:306-308)
    MY = 2                         # MyConvolve (audio_matcher.rs:442-448)


class AmPeak(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64),
                ("height", C.c_float), ("prominence", C.c_float)]


class AmHitScore(C.Structure):     # am_hit_score (include/audiomatch.h, per-hit scoring)
    _fields_ = [("position", C.c_double), ("ncc", C.c_float), ("gain", C.c_float),
                ("window_db", C.c_float), ("flags", C.c_uint32)]


AM_HIT_UNREFINED, AM_HIT_BELOW_FLOOR, AM_HIT_NONFINITE = 1, 2, 4


class AmSegmentParams(C.Structure):   # am_segment_params (include/audiomatch.h, per-segment hit scoring)
    _fields_ = [("segments", C.c_uint32), ("radius", C.c_uint32)]


class HitSegment(C.Structure):        # am_hit_segment: one segment of one hit
    _fields_ = [("lag", C.c_double), ("ncc", C.c_float), ("gain", C.c_float),
                ("level_db", C.c_float), ("flags", C.c_uint32)]

    def __repr__(self):
        return f"HitSegment(lag={self.lag!r}, ncc={self.ncc!r}, gain={self.gain!r}, level_db={self.level_db!r}, flags={self.flags})"


class AmSegmentSummary(C.Structure):  # am_segment_summary
    _fields_ = [("coverage", C.c_double), ("drift_ppm", C.c_double), ("start_lag", C.c_double),
                ("residual_rms", C.c_double), ("first_present", C.c_int32), ("last_present", C.c_int32),
                ("n_present", C.c_uint32), ("n_usable", C.c_uint32)]


AM_HIT_EMPTY_SEGMENT = 8
AM_SEG_MAX_SEGMENTS, AM_SEG_MAX_RADIUS = 1024, 16


class AmWarpParams(C.Structure):      # am_warp_params (include/audiomatch.h, per-hit drift scoring)
    _fields_ = [("centre_ppm", C.c_double), ("max_ppm", C.c_double), ("steps", C.c_uint32), ("radius", C.c_uint32)]


class HitWarp(C.Structure):           # am_warp_hit: one hit's drift, lag and corrected NCC
    _fields_ = [("drift_ppm", C.c_double), ("lag", C.c_double), ("ncc", C.c_float), ("gain", C.c_float),
                ("level_db", C.c_float), ("ncc_centre", C.c_float), ("length", C.c_uint32), ("flags", C.c_uint32)]

    def __repr__(self):
        return (f"HitWarp(drift_ppm={self.drift_ppm!r}, lag={self.lag!r}, ncc={self.ncc!r}, gain={self.gain!r}, "
                f"level_db={self.level_db!r}, ncc_centre={self.ncc_centre!r}, length={self.length}, flags={self.flags})")

    def pack(self) -> bytes:
        """The record's 40 bytes (for bit-for-bit comparisons)."""
        return bytes(self)


AM_HIT_DRIFT_UNREFINED = 256
AM_WARP_PHASES, AM_WARP_TAPS, AM_WARP_MAX_STEPS, AM_WARP_MAX_PPM = 4096, 32, 32, 50000


class AmChannelParams(C.Structure):   # am_channel_params (include/audiomatch.h, per-hit channel estimation)
    _fields_ = [("radius", C.c_uint32), ("reserved", C.c_uint32), ("noise_db", C.c_double)]


class HitChannel(C.Structure):        # am_channel_hit: how well the needle, filtered by the hit's own taps, explains the span
    _fields_ = [("ncc", C.c_float), ("ncc_eq", C.c_float), ("gain_db", C.c_float), ("residual_db", C.c_float),
                ("main_tap", C.c_int32), ("main_share", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __repr__(self):
        return (f"HitChannel(ncc={self.ncc!r}, ncc_eq={self.ncc_eq!r}, gain_db={self.gain_db!r}, residual_db={self.residual_db!r}, "
                f"main_tap={self.main_tap}, main_share={self.main_share!r}, flags={self.flags})")

    def pack(self) -> bytes:
        """The record's 32 bytes (for bit-for-bit comparisons)."""
        return bytes(self)


AM_HIT_ILL_CONDITIONED = 512
AM_CHAN_MAX_RADIUS = 128


class AmStereoParams(C.Structure):    # am_stereo_params (include/audiomatch.h, per-hit stereo image)
    _fields_ = [("radius", C.c_uint32), ("reserved", C.c_uint32)]


class HitStereo(C.Structure):         # am_stereo_hit: where a hit sits between the channels
    _fields_ = [("lag_left", C.c_double), ("lag_right", C.c_double), ("ncc_left", C.c_float), ("ncc_right", C.c_float),
                ("ncc_mid", C.c_float), ("ncc_side", C.c_float), ("ncc_best", C.c_float), ("gain_left", C.c_float),
                ("gain_right", C.c_float), ("mix_left", C.c_float), ("mix_right", C.c_float), ("flags", C.c_uint32)]

    def __repr__(self):
        return "HitStereo(" + ", ".join(f"{n}={getattr(self, n)!r}" for n, _ in self._fields_) + ")"

    def pack(self) -> bytes:
        """The record's 56 bytes (for bit-for-bit comparisons)."""
        return bytes(self)


class AmStereoSummary(C.Structure):   # am_stereo_summary
    _fields_ = [("balance_db", C.c_double), ("delay", C.c_double), ("downmix_loss_db", C.c_double), ("image", C.c_int32),
                ("reserved", C.c_uint32)]


AM_HIT_LEFT_SILENT, AM_HIT_RIGHT_SILENT, AM_HIT_SIDE_SILENT, AM_HIT_COLLINEAR = 1024, 2048, 4096, 8192
AM_HIT_LEFT_UNREFINED, AM_HIT_RIGHT_UNREFINED = 16384, 32768
AM_STEREO_MAX_RADIUS, AM_STEREO_MIN_INDEPENDENCE = 16, 1e-6
AM_IMAGE_ABSENT, AM_IMAGE_CENTRE, AM_IMAGE_LEFT, AM_IMAGE_RIGHT, AM_IMAGE_PANNED, AM_IMAGE_INVERTED = range(6)


class AmBandParams(C.Structure):      # am_band_params (include/audiomatch.h, per-band hit scoring)
    _fields_ = [("frame_log2", C.c_uint32), ("n_bands", C.c_uint32), ("edges", C.c_uint32 * 33)]


class HitBand(C.Structure):           # am_hit_band: one band of one hit
    _fields_ = [("ncc", C.c_float), ("coherence", C.c_float), ("gain", C.c_float), ("level_db", C.c_float),
                ("needle_share", C.c_float), ("flags", C.c_uint32)]

    def __repr__(self):
        return (f"HitBand(ncc={self.ncc!r}, coherence={self.coherence!r}, gain={self.gain!r}, level_db={self.level_db!r}, "
                f"needle_share={self.needle_share!r}, flags={self.flags})")

    def pack(self) -> bytes:
        """The record's 24 bytes (for bit-for-bit comparisons)."""
        return bytes(self)


class AmBandSummary(C.Structure):     # am_band_summary
    _fields_ = [("coverage", C.c_double), ("weighted_coherence", C.c_double), ("gain_db_spread", C.c_double),
                ("first_present", C.c_int32), ("last_present", C.c_int32), ("n_present", C.c_uint32),
                ("n_countable", C.c_uint32)]


AM_HIT_EMPTY_BAND = 128
AM_BAND_MAX_BANDS, AM_BAND_EMPTY_DB = 32, 90


class AmSignificanceParams(C.Structure):   # am_significance_params (include/audiomatch.h, per-hit significance)
    _fields_ = [("guard", C.c_uint64), ("radius", C.c_uint64)]


class HitSignificance(C.Structure):        # am_significance: one hit against its local background
    _fields_ = [("score", C.c_float), ("bg_mean", C.c_float), ("bg_std", C.c_float), ("z", C.c_float),
                ("side_max", C.c_float), ("side_lag", C.c_int32), ("n_bg", C.c_uint32), ("flags", C.c_uint32)]

    def __repr__(self):
        return (f"HitSignificance(score={self.score!r}, bg_mean={self.bg_mean!r}, bg_std={self.bg_std!r}, z={self.z!r}, "
                f"side_max={self.side_max!r}, side_lag={self.side_lag}, n_bg={self.n_bg}, flags={self.flags})")

    def pack(self) -> bytes:
        """The record's 32 bytes (for bit-for-bit comparisons)."""
        return bytes(self)


AM_HIT_NO_BACKGROUND, AM_HIT_FLAT_BACKGROUND, AM_HIT_CLIPPED = 16, 32, 64
AM_SIG_MAX_RADIUS = 1 << 22


class AmEstimateParams(C.Structure):   # am_estimate_params (include/audiomatch.h, needle estimation)
    _fields_ = [("method", C.c_uint32), ("trim_permille", C.c_uint32), ("lead", C.c_uint64), ("length", C.c_uint64)]


class AmEstHit(C.Structure):           # am_est_hit: one occurrence in a resident haystack
    _fields_ = [("start", C.c_uint64), ("haystack", C.c_uint32), ("scale", C.c_float)]


class Est(enum.IntEnum):               # AM_EST_*
    MEAN = 0
    MEDIAN = 1
    TRIMMED = 2


EST_MAX_HITS = 64                      # AM_EST_MAX_HITS


class AmMatchParams(C.Structure):
    _fields_ = [("sr", C.c_uint32), ("chunk", C.c_uint64), ("overlap", C.c_uint64),
                ("min_prominence", C.c_float), ("min_distance", C.c_uint64),
                ("overshadow_distance_s", C.c_double), ("scale", C.c_int)]


class AmBestParams(C.Structure):     # am_best_params (include/audiomatch.h, the k best matches)
    _fields_ = [("k", C.c_uint64), ("min_distance", C.c_uint64), ("min_prominence", C.c_float), ("scale", C.c_int)]


class AmTraceParams(C.Structure):    # am_trace_params (include/audiomatch.h, score traces)
    _fields_ = [("bin", C.c_uint64), ("scale", C.c_int), ("reserved", C.c_uint32)]


class AmTraceStats(C.Structure):     # am_trace_stats: what am_trace_summary returns
    _fields_ = [("count", C.c_uint64), ("argmax", C.c_uint64), ("argmin", C.c_uint64), ("max", C.c_double), ("min", C.c_double),
                ("mean", C.c_double), ("std", C.c_double), ("median_max", C.c_double), ("mad_max", C.c_double),
                ("peak_z", C.c_double)]


# am_trace_bin as a numpy structured dtype (40 bytes, no padding): what the trace calls return arrays of
TRACE_BIN_DTYPE = np.dtype([("max", "<f4"), ("min", "<f4"), ("argmax", "<u4"), ("argmin", "<u4"), ("count", "<u4"),
                            ("reserved", "<u4"), ("sum", "<f8"), ("sumsq", "<f8")])
AM_TRACE_WAVE_BIN_MAX, AM_TRACE_SLICE, AM_TRACE_MAX_BIN = 2048, 8192, 1 << 30


class AmDiscoverParams(C.Structure):   # am_discover_params (include/audiomatch.h, needle discovery)
    _fields_ = [("probe_len", C.c_uint64), ("hop", C.c_uint64), ("exclude", C.c_uint64), ("separation", C.c_uint64),
                ("min_level_db", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AmRegionParams(C.Structure):     # am_region_params
    _fields_ = [("min_ncc", C.c_float), ("max_second", C.c_float), ("tolerance", C.c_uint64), ("min_good", C.c_uint32),
                ("max_gap", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# am_probe_hit (40 bytes) and am_region (56 bytes) as numpy structured dtypes: what the discovery calls return arrays of
PROBE_HIT_DTYPE = np.dtype([("probe", "<u8"), ("best", "<u8"), ("second", "<u8"), ("ncc", "<f4"), ("ncc_second", "<f4"),
                            ("flags", "<u4"), ("reserved", "<u4")])
REGION_DTYPE = np.dtype([("a_start", "<u8"), ("length", "<u8"), ("displacement", "<i8"), ("first", "<u8"), ("count", "<u4"),
                         ("good", "<u4"), ("mean_ncc", "<f8"), ("min_ncc", "<f4"), ("worst_second", "<f4")])
AM_DISCOVER_SELF, AM_REGION_FOLD, AM_DISCOVER_SLICE = 1, 1, 8192
AM_PROBE_NO_BEST, AM_PROBE_NO_SECOND, AM_PROBE_NONFINITE, AM_PROBE_QUIET = 1, 2, 4, 8


class AmEdgeParams(C.Structure):       # am_edge_params (include/audiomatch.h, edge matching), 24 bytes
    _fields_ = [("min_overlap", C.c_uint64), ("separation", C.c_uint64), ("min_share", C.c_float), ("reserved", C.c_uint32)]


# am_edge_hit (48 bytes, no padding) as a numpy structured dtype: what the edge calls return two of per haystack
EDGE_HIT_DTYPE = np.dtype([("start", "<i8"), ("second", "<i8"), ("overlap", "<u8"), ("ncc", "<f4"), ("ncc_second", "<f4"),
                           ("gain", "<f4"), ("share", "<f4"), ("edge", "<u4"), ("flags", "<u4")])
AM_EDGE_HEAD, AM_EDGE_TAIL, AM_EDGE_TILE = 0, 1, 4096
AM_EDGE_NO_BEST, AM_EDGE_NO_SECOND, AM_EDGE_NONFINITE, AM_EDGE_BELOW_FLOOR = 1, 2, 4, 8


class AmEnvParams(C.Structure):        # am_env_params (include/audiomatch.h, envelope matching)
    _fields_ = [("bands", AmBandParams), ("reserved", C.c_uint32), ("floor_db", C.c_double)]


class AmEnvGrid(C.Structure):          # am_env_grid: 2 K + 1 drifts centre_ppm + max_ppm (q - K) / K
    _fields_ = [("centre_ppm", C.c_double), ("max_ppm", C.c_double), ("steps", C.c_uint32), ("reserved", C.c_uint32)]


# am_env_pick (24 bytes) and am_env_hit (32 bytes) as numpy structured dtypes
ENV_PICK_DTYPE = np.dtype([("frame", "<u8"), ("pos", "<f8"), ("score", "<f4"), ("q", "<u4")])
ENV_HIT_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("drift_ppm", "<f8"), ("score", "<f4"), ("q", "<u4")])
AM_ENV_STEPS_PER_DB, AM_ENV_MAX_LEVEL, AM_ENV_ABSENT, AM_ENV_NO_Q = 8, 1023, 0xFFFF, 0xFFFFFFFF
AM_ENV_MAX_PPM, AM_ENV_MAX_FRAMES, AM_ENV_MAX_NEEDLES, AM_ENV_MAX_STEPS = 250000, 16384, 257, 128
AM_ENV_MAX_LEN, AM_ENV_MAX_HAY_FRAMES, AM_ENV_TILE, AM_ENV_CHUNK = 1 << 31, 1 << 24, 512, 8


class AmMonitorInfo(C.Structure):  # am_monitor_info (include/audiomatch.h, live monitoring)
    _fields_ = [("received", C.c_uint64), ("horizon", C.c_uint64), ("resident_bytes", C.c_uint64), ("pending", C.c_uint64)]


class AudioMatchError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"audiomatch error {code}: {msg}")
        self.code = code


AM_MASK_MAX_GAPS = 15


class AmSpan(C.Structure):
    """am_span: samples [begin, end) of a needle (a gap of a masked needle)."""
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64)]


AM_MASK_BELOW_FLOOR, AM_MASK_NONFINITE, AM_MASK_GAPS_SILENT, AM_MASK_GAPS_NONFINITE, AM_MASK_NO_GAPS = 1, 2, 4, 8, 16


class HitMask(C.Structure):           # am_mask_hit: the per-hit record of a masked handle (am_hit_mask*)
    _fields_ = [("ncc", C.c_float), ("gain", C.c_float), ("kept_db", C.c_float), ("ncc_gaps", C.c_float), ("gaps_db", C.c_float),
                ("flags", C.c_uint32)]

    def __repr__(self):
        return "HitMask(" + ", ".join(f"{n}={getattr(self, n)!r}" for n, _ in self._fields_) + ")"


def _spans(gaps):
    """A list of (begin, end) as an am_span array and its length."""
    gaps = [] if gaps is None else list(gaps)
    arr = (AmSpan * max(len(gaps), 1))()
    for i, (b, e) in enumerate(gaps):
        arr[i].begin, arr[i].end = int(b), int(e)
    return arr, len(gaps)


# every symbol include/audiomatch.h declares: (name, restype, argtypes)
_f32p = C.POINTER(C.c_float)
_SIGNATURES = {
    "am_needle_create_masked": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(AmSpan), C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_needle_create_masked_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(AmSpan), C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_needle_mask": (C.c_int, [C.c_void_p, C.POINTER(AmSpan), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_hit_mask_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(HitMask)]),
    "am_hit_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(HitMask)]),
    "am_hit_mask_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                           C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(HitMask)]),
    "am_abi_version": (C.c_int, []),
    "am_last_error_string": (C.c_char_p, []),
    "am_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "am_shutdown": (C.c_int, []),
    "am_needle_create": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_needle_create_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_needle_destroy": (None, [C.c_void_p]),
    "am_needle_len": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "am_needle_inv_autocorr": (C.c_int, [C.c_void_p, _f32p]),
    "am_correlate_len": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]),
    "am_correlate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                               C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_correlate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AmMatchParams),
                           C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AmMatchParams),
                                  C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                        C.c_size_t, C.POINTER(AmMatchParams), C.POINTER(AmPeak),
                                        C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_multi_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "am_needle_create_pcm16": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_match_pcm16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AmMatchParams),
                                 C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_pcm16_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AmMatchParams),
                                        C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_pcm16_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.c_size_t, C.POINTER(AmMatchParams), C.POINTER(AmPeak),
                                              C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_find_peaks": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_uint64,
                                C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_pcm_s16_stereo_to_mono": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "am_pcm_s16_stereo_to_mono_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "am_device_malloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "am_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_host_free": (C.c_int, [C.c_void_p]),
    "am_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "am_host_unregister": (C.c_int, [C.c_void_p]),
    "am_memcpy_h2d": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "am_memcpy_d2h": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "am_device_synchronize": (C.c_int, [C.c_int]),
    "am_synth_uniform_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                          C.c_size_t, C.c_float]),
    "am_axpy_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "am_synth_pcm16_stereo_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                               C.c_size_t, C.c_float]),
    "am_add_pcm16_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "am_set_progress_callback": (C.c_int, [C.c_void_p, C.c_void_p]),
    "am_set_chunk_progress_callback": (C.c_int, [C.c_void_p, C.c_void_p]),
    "am_needle_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_longlong]),
    "am_needle_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong)]),
    "am_shard_plan": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                                C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "am_pool_create": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_void_p)]),
    "am_pool_destroy": (None, [C.c_void_p]),
    "am_pool_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "am_pool_slot": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "am_pool_match_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t,
                                      C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "am_pool_match_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t,
                                             C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "am_match_multi_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.c_size_t, C.c_int, C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                              C.POINTER(C.c_size_t)]),
    "am_pool_match_batch_pcm16": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t,
                                            C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "am_pool_match_batch_pcm16_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                   C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                                   C.POINTER(C.c_size_t)]),
    "am_match_multi_varlen_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.POINTER(AmMatchParams),
                                                     C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_multi_varlen": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t,
                                        C.c_int, C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "am_pool_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                       C.POINTER(C.c_void_p)]),
    "am_pool_needle_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "am_pool_match_multi_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                            C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "am_pool_match_multi_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                                   C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t,
                                                   C.POINTER(C.c_size_t)]),
    "am_long_plan": (C.c_int, [C.c_size_t, C.c_size_t, C.POINTER(AmMatchParams), C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                               C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "am_match_part_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmMatchParams), C.c_size_t,
                                       C.c_uint64, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_merge_peaks": (C.c_int, [C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t, C.POINTER(AmPeak), C.c_size_t,
                                 C.POINTER(C.c_size_t)]),
    "am_pool_match_long": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmMatchParams), C.POINTER(AmPeak),
                                     C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_pool_match_long_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.POINTER(AmMatchParams),
                                            C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_merge_ready": (C.c_int, [C.POINTER(AmMatchParams), C.POINTER(AmPeak), C.c_size_t, C.c_uint64, C.c_int,
                                 C.POINTER(C.c_size_t)]),
    "am_monitor_begin": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(AmMatchParams), C.c_int, C.c_size_t,
                                   C.POINTER(C.c_void_p)]),
    "am_monitor_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "am_monitor_poll": (C.c_int, [C.c_void_p, C.POINTER(AmPeak), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_monitor_end": (C.c_int, [C.c_void_p, C.POINTER(AmPeak), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_monitor_info_get": (C.c_int, [C.c_void_p, C.POINTER(AmMonitorInfo)]),
    "am_monitor_destroy": (None, [C.c_void_p]),
    "am_match_stream_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(AmMatchParams), C.POINTER(C.c_void_p)]),
    "am_match_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "am_match_stream_finish": (C.c_int, [C.c_void_p, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_stream_destroy": (None, [C.c_void_p]),
    "am_debug_column_bench": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "am_profile_enable": (C.c_int, [C.c_int, C.c_int]),
    "am_profile_reset": (C.c_int, [C.c_int]),
    "am_profile_query": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "am_hit_scores_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                       C.POINTER(AmHitScore)]),
    "am_hit_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                C.POINTER(AmHitScore)]),
    "am_hit_scores_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                             C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(AmHitScore)]),
    "am_hit_segments_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                         C.POINTER(AmSegmentParams), C.POINTER(HitSegment)]),
    "am_hit_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                  C.POINTER(AmSegmentParams), C.POINTER(HitSegment)]),
    "am_hit_segments_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                               C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(AmSegmentParams), C.POINTER(HitSegment)]),
    "am_hit_segments_summary": (C.c_int, [C.POINTER(HitSegment), C.c_uint32, C.c_size_t, C.c_float,
                                          C.POINTER(AmSegmentSummary)]),
    "am_hit_bands_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                      C.POINTER(AmBandParams), C.POINTER(HitBand)]),
    "am_hit_bands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                               C.POINTER(AmBandParams), C.POINTER(HitBand)]),
    "am_hit_bands_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                            C.POINTER(AmBandParams), C.POINTER(HitBand)]),
    "am_hit_bands_summary": (C.c_int, [C.POINTER(HitBand), C.c_uint32, C.c_float, C.POINTER(AmBandSummary)]),
    "am_band_edges_log": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.POINTER(AmBandParams)]),
    "am_hit_significance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                             C.POINTER(AmSignificanceParams), C.POINTER(HitSignificance)]),
    "am_hit_significance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                      C.POINTER(AmSignificanceParams), C.POINTER(HitSignificance)]),
    "am_hit_significance_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                   C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                                   C.POINTER(AmSignificanceParams), C.POINTER(HitSignificance)]),
    "am_resample_len": (C.c_int, [C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]),
    "am_resample": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                              C.POINTER(C.c_size_t)]),
    "am_resample_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
                                     C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_needle_create_resampled": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32,
                                             C.POINTER(C.c_void_p)]),
    "am_lag_products": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_double)]),
    "am_lag_products_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_double)]),
    "am_whiten_taps": (C.c_int, [C.POINTER(C.c_double), C.c_uint32, C.c_double, C.POINTER(C.c_float)]),
    "am_fir": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.c_uint32, C.c_size_t, C.c_void_p,
                         C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_fir_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.c_uint32, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_needle_create_filtered": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.c_uint32,
                                            C.POINTER(C.c_void_p)]),
    "am_hit_window": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p]),
    "am_warp_table": (C.c_int, [C.c_void_p]),
    "am_hit_warp_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                     C.POINTER(AmWarpParams), C.POINTER(HitWarp)]),
    "am_hit_warp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                              C.POINTER(AmWarpParams), C.POINTER(HitWarp)]),
    "am_hit_warp_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                           C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(AmWarpParams), C.POINTER(HitWarp)]),
    "am_hit_window_warped": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_float, C.c_double, C.c_double,
                                       C.c_uint64, C.c_uint64, C.c_void_p]),
    "am_hit_channel_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                        C.POINTER(AmChannelParams), C.POINTER(HitChannel), C.c_void_p]),
    "am_hit_channel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                 C.POINTER(AmChannelParams), C.POINTER(HitChannel), C.c_void_p]),
    "am_hit_channel_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                              C.POINTER(AmChannelParams), C.POINTER(HitChannel), C.c_void_p]),
    "am_channel_solve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_int)]),
    "am_hit_residual": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_void_p]),
    "am_hit_stereo_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                       C.POINTER(AmStereoParams), C.POINTER(HitStereo)]),
    "am_hit_stereo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t,
                                C.POINTER(AmStereoParams), C.POINTER(HitStereo)]),
    "am_hit_stereo_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                             C.c_size_t, C.c_int, C.POINTER(AmPeak), C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(AmStereoParams), C.POINTER(HitStereo)]),
    "am_hit_stereo_summary": (C.c_int, [C.POINTER(HitStereo), C.c_float, C.POINTER(AmStereoSummary)]),
    "am_pcm_s16_stereo_mix": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p]),
    "am_pcm_s16_stereo_mix_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p]),
    "am_needle_estimate_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(AmEstimateParams), C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "am_needle_estimate_device": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                            C.POINTER(AmEstHit), C.c_size_t, C.POINTER(AmEstimateParams), C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "am_set_option": (C.c_int, [C.c_char_p, C.c_longlong]),
    "am_match_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmBestParams), C.POINTER(AmPeak),
                                C.POINTER(C.c_size_t)]),
    "am_match_best_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmBestParams),
                                       C.POINTER(AmPeak), C.POINTER(C.c_size_t)]),
    "am_match_best_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                             C.POINTER(AmBestParams), C.POINTER(AmPeak), C.POINTER(C.c_size_t)]),
    "am_find_peaks_top": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_uint64, C.c_size_t,
                                    C.POINTER(AmPeak), C.POINTER(C.c_size_t)]),
    "am_trace_len": (C.c_int, [C.c_size_t, C.c_uint64, C.POINTER(C.c_size_t)]),
    "am_trace_scores": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_trace_scores_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "am_match_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmTraceParams), C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_size_t)]),
    "am_match_trace_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmTraceParams), C.c_void_p,
                                        C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_trace_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                              C.POINTER(AmTraceParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_trace_summary": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(AmTraceStats)]),
    "am_find_peaks_top_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_uint64, C.c_size_t,
                                           C.POINTER(AmPeak), C.POINTER(C.c_size_t)]),
    "am_discover_len": (C.c_int, [C.c_size_t, C.POINTER(AmDiscoverParams), C.POINTER(C.c_size_t)]),
    "am_discover": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmDiscoverParams),
                              C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_discover_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                     C.POINTER(AmDiscoverParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_probe_scores": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "am_probe_scores_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "am_edge_scores_len": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "am_edge_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(AmEdgeParams), C.c_void_p,
                                 C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_edge_scores_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(AmEdgeParams), C.c_void_p,
                                        C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEdgeParams), C.c_void_p]),
    "am_match_edges_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEdgeParams), C.c_void_p]),
    "am_match_edges_batch_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                                              C.POINTER(AmEdgeParams), C.c_void_p]),
    "am_discover_regions": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(AmDiscoverParams), C.POINTER(AmRegionParams),
                                      C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_envelope_len": (C.c_int, [C.c_size_t, C.POINTER(AmEnvParams), C.c_double, C.POINTER(C.c_size_t)]),
    "am_envelope": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEnvParams), C.c_double, C.c_void_p, C.c_size_t,
                              C.POINTER(C.c_size_t)]),
    "am_envelope_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEnvParams), C.c_double, C.c_void_p,
                                     C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_envelope_scores": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_envelope_scores_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_envelope_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint64, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]),
    "am_match_envelope": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEnvParams), C.POINTER(AmEnvGrid),
                                    C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_match_envelope_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(AmEnvParams), C.POINTER(AmEnvGrid),
                                           C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "am_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_longlong)]),
}


def declared_symbols():
    return sorted(_SIGNATURES)


_lib = None


def lib():
    """Load the HIP library (no fallback: raises if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python audio-matcher_amd/build.py` "
                "(__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)      # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int):
    if rc != AM_OK:
        msg = lib().am_last_error_string()
        raise AudioMatchError(rc, msg.decode() if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().am_device_count(C.byref(n))
    return n.value if rc == AM_OK else 0


def set_option(key: str, value: int):
    _check(lib().am_set_option(key.encode(), int(value)))


def get_option(key: str) -> int:
    v = C.c_longlong(0)
    _check(lib().am_get_option(key.encode(), C.byref(v)))
    return v.value


# ---------------------------------------------------------------------------
class DeviceBuffer:
    """A raw HBM allocation owned through the C ABI (am_device_malloc)."""

    def __init__(self, device: int, nbytes: int):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        _check(lib().am_device_malloc(device, max(self.nbytes, 4), C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, device: int, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(device, a.nbytes)
        if a.nbytes:
            _check(lib().am_memcpy_h2d(device, buf.ptr, a.ctypes.data, a.nbytes))
        return buf

    def to_numpy(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            _check(lib().am_memcpy_d2h(self.device, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().am_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """A numpy array in pinned host memory (am_host_alloc): what a decoder would write its output into."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _check(lib().am_host_alloc(max(self.nbytes, 4), C.byref(p)))
        self.ptr = p.value
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(self.ptr), dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().am_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class registered:
    """with registered(array): the array's memory is pinned for the duration (am_host_register)."""

    def __init__(self, a: np.ndarray):
        self.a = a

    def __enter__(self):
        _check(lib().am_host_register(self.a.ctypes.data, self.a.nbytes))
        return self.a

    def __exit__(self, *exc):
        _check(lib().am_host_unregister(self.a.ctypes.data))


def synth_uniform_device(device: int, n: int, seed: int, stream: int, first: int = 0,
                         amp: float = 0.25) -> DeviceBuffer:
    buf = DeviceBuffer(device, n * 4)
    _check(lib().am_synth_uniform_device(device, buf.ptr, seed, stream, first, n, amp))
    return buf


def synth_pcm16_stereo_device(device: int, frames: int, seed: int, stream: int, first: int = 0,
                              amp: float = 0.25) -> DeviceBuffer:
    """Interleaved i16 stereo frames of the synthetic signal (left = stream, right = stream + 5000)."""
    buf = DeviceBuffer(device, frames * 4)
    _check(lib().am_synth_pcm16_stereo_device(device, buf.ptr, seed, stream, first, frames, amp))
    return buf


def add_pcm16_device(device: int, dst: DeviceBuffer, dst_frame: int, src_ptr: int, frames: int):
    _check(lib().am_add_pcm16_device(device, dst.ptr + 4 * dst_frame, src_ptr, frames))


def axpy_device(device: int, dst: DeviceBuffer, dst_offset: int, src_ptr: int, n: int, gain: float = 1.0):
    _check(lib().am_axpy_device(device, dst.ptr + 4 * dst_offset, src_ptr, n, gain))


def pcm_s16_stereo_to_mono(interleaved: np.ndarray, device: int = 0) -> np.ndarray:
    """mp3_reader.rs:28-37 down-mix on the GPU."""
    a = np.ascontiguousarray(interleaved, dtype=np.int16)
    frames = a.size // 2
    out = np.empty(frames, dtype=np.float32)
    _check(lib().am_pcm_s16_stereo_to_mono(device, a.ctypes.data, frames, out.ctypes.data))
    return out


def pcm_s16_stereo_mix(interleaved: np.ndarray, a: float, b: float, device: int = 0) -> np.ndarray:
    """am_pcm_s16_stereo_mix: f32((f64(a) L + f64(b) R) k) of interleaved i16 stereo frames; (0.5, 0.5) is the down-mix,
    (1, 0) left, (0, 1) right, (0.5, -0.5) side."""
    x = np.ascontiguousarray(interleaved, dtype=np.int16)
    frames = x.size // 2
    out = np.empty(frames, dtype=np.float32)
    _check(lib().am_pcm_s16_stereo_mix(device, x.ctypes.data, frames, float(a), float(b), out.ctypes.data))
    return out


def pcm_s16_stereo_mix_device(device: int, src_ptr: int, frames: int, a: float, b: float, dst_ptr: int):
    """am_pcm_s16_stereo_mix_device: the same between two buffers resident on `device`."""
    _check(lib().am_pcm_s16_stereo_mix_device(device, src_ptr, int(frames), float(a), float(b), dst_ptr))


def _samples(x):
    """(array, format, length) of a host signal: f32 mono, or int16 interleaved stereo (flat or (frames, 2))."""
    a = np.asarray(x)
    if a.dtype == np.int16:
        a = np.ascontiguousarray(a)
        return a, Fmt.S16_STEREO, a.size // 2
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, Fmt.F32_MONO, a.size


def resample_len(n_in: int, src_rate: int, dst_rate: int) -> int:
    """am_resample_len: ceil(n_in * L / M), L / M = dst_rate / src_rate in lowest terms (pure host function)."""
    n = C.c_size_t(0)
    _check(lib().am_resample_len(int(n_in), int(src_rate), int(dst_rate), C.byref(n)))
    return n.value


def resample(x, src_rate: int, dst_rate: int, device: int = 0) -> np.ndarray:
    """am_resample: x (f32 mono, or int16 interleaved stereo, flat or (frames, 2)) from src_rate to dst_rate, as
    scipy.signal.resample_poly(x, L, M) computes it (include/audiomatch.h); f32 mono out."""
    a, fmt, length = _samples(x)
    n = resample_len(length, src_rate, dst_rate)
    out = np.empty(n, dtype=np.float32)
    got = C.c_size_t(0)
    _check(lib().am_resample(device, a.ctypes.data, length, int(fmt), int(src_rate), int(dst_rate), out.ctypes.data, n,
                             C.byref(got)))
    return out


def resample_device(device: int, src_ptr: int, n_in: int, src_rate: int, dst_rate: int, dst_ptr: int, cap: int,
                    fmt: int = Fmt.F32_MONO) -> int:
    """am_resample_device on resident buffers; returns the output length."""
    got = C.c_size_t(0)
    _check(lib().am_resample_device(device, src_ptr, int(n_in), int(fmt), int(src_rate), int(dst_rate), dst_ptr, int(cap),
                                    C.byref(got)))
    return got.value


WHITEN_MAX_ORDER = 64                 # AM_WHITEN_MAX_ORDER
FIR_MAX_TAPS = WHITEN_MAX_ORDER + 1   # AM_FIR_MAX_TAPS
LAG_BLOCK = 8192                      # samples per block of the lag products (kLagBlock, csrc/am_kernels.h)
FIR_TILE = 2048                       # outputs per workgroup of the FIR kernel (kFirTile, csrc/am_kernels.h)


def lag_products(x, order: int, device: int = 0) -> np.ndarray:
    """am_lag_products: r[k] = sum_i x~[i] x~[i - k], k = 0 .. order, in f64 (x: f32 mono, or int16 interleaved stereo;
    non-finite samples count as 0).  Additive over files: add the r of an archive's files to design one filter."""
    a, fmt, length = _samples(x)
    r = np.zeros(int(order) + 1, dtype=np.float64)
    _check(lib().am_lag_products(device, a.ctypes.data, length, int(fmt), int(order), r.ctypes.data_as(C.POINTER(C.c_double))))
    return r


def lag_products_device(device: int, src_ptr: int, n: int, order: int, fmt: int = Fmt.F32_MONO) -> np.ndarray:
    """am_lag_products_device on a resident buffer; r comes back in host memory."""
    r = np.zeros(int(order) + 1, dtype=np.float64)
    _check(lib().am_lag_products_device(device, src_ptr, int(n), int(fmt), int(order), r.ctypes.data_as(C.POINTER(C.c_double))))
    return r


def whiten_taps(r, noise_db: float = 60.0) -> np.ndarray:
    """am_whiten_taps (pure host function): the prediction-error filter a[0 .. order], a[0] = 1, of the lag products
    r[0 .. order] (Levinson-Durbin in f64, r[0] raised by -noise_db of white noise), rounded to f32."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    taps = np.zeros(max(r.size, 1), dtype=np.float32)
    _check(lib().am_whiten_taps(r.ctypes.data_as(C.POINTER(C.c_double)), r.size - 1, float(noise_db),
                                taps.ctypes.data_as(C.POINTER(C.c_float))))
    return taps


def _taps(taps):
    t = np.ascontiguousarray(taps, dtype=np.float32)
    return t, t.ctypes.data_as(C.POINTER(C.c_float))


def fir(x, taps, lead: int = 0, device: int = 0) -> np.ndarray:
    """am_fir: y[k] = sum_j taps[j] x[lead + k - j], k < len(x) - lead (x: f32 mono, or int16 interleaved stereo; x = 0
    before its first sample); f32 mono out.  Filtering x[a - l:b] with lead = l = min(a, len(taps) - 1) gives
    fir(x, taps)[a:b] bit for bit."""
    a, fmt, length = _samples(x)
    t, tp = _taps(taps)
    out = np.empty(max(length - int(lead), 0), dtype=np.float32)
    got = C.c_size_t(0)
    _check(lib().am_fir(device, a.ctypes.data, length, int(fmt), tp, t.size, int(lead), out.ctypes.data, out.size, C.byref(got)))
    return out


def fir_device(device: int, src_ptr: int, n_in: int, taps, dst_ptr: int, cap: int, lead: int = 0,
               fmt: int = Fmt.F32_MONO) -> int:
    """am_fir_device on resident buffers; returns the output length."""
    t, tp = _taps(taps)
    got = C.c_size_t(0)
    _check(lib().am_fir_device(device, src_ptr, int(n_in), int(fmt), tp, t.size, int(lead), dst_ptr, int(cap), C.byref(got)))
    return got.value


def hit_window(haystack, start: int, scale: float, lead: int, length: int) -> np.ndarray:
    """am_hit_window (pure host function): the row of one occurrence, element n = fl32(x[start - lead + n] * scale) of the
    host haystack x (f32 mono, or int16 interleaved stereo); NaN where that element lies outside x or is not finite."""
    a, fmt, n = _samples(haystack)
    row = np.empty(int(length), dtype=np.float32)
    _check(lib().am_hit_window(a.ctypes.data, n, int(fmt), int(start), float(scale), int(lead), int(length), row.ctypes.data))
    return row


def hit_window_warped(haystack, start: int, scale: float, lag: float, drift_ppm: float, lead: int, length: int) -> np.ndarray:
    """am_hit_window_warped (pure host function): hit_window's row on the needle's clock, for an occurrence whose `lag`
    and `drift_ppm` hit_warp reported.  NaN where an element is absent."""
    a, fmt, n = _samples(haystack)
    row = np.empty(int(length), dtype=np.float32)
    _check(lib().am_hit_window_warped(a.ctypes.data, n, int(fmt), int(start), float(scale), float(lag), float(drift_ppm),
                                      int(lead), int(length), row.ctypes.data))
    return row


def warp_table() -> np.ndarray:
    """am_warp_table (pure host function): the interpolator's table, (AM_WARP_PHASES, AM_WARP_TAPS) f32."""
    t = np.empty((AM_WARP_PHASES, AM_WARP_TAPS), dtype=np.float32)
    _check(lib().am_warp_table(t.ctypes.data))
    return t


def warp_params(max_ppm: float, steps: int = 8, radius: int = 4, centre_ppm: float = 0.0) -> AmWarpParams:
    return AmWarpParams(float(centre_ppm), float(max_ppm), int(steps), int(radius))


def channel_params(radius: int, noise_db: float = 60.0) -> AmChannelParams:
    return AmChannelParams(int(radius), 0, float(noise_db))


def channel_solve(r, c, noise_db: float = 60.0):
    """am_channel_solve (pure host function): (h, ill) -- the taps h[-P .. P] (f64, h[l] at l + P) of the needle's
    autocorrelation r[0 .. 2P] and the cross-correlation c[-P .. P], by the Levinson recursion for a general right-hand
    side; ill: it fell back to the plain gain."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if r.size != c.size or r.size % 2 == 0:
        raise ValueError("channel_solve: r and c hold 2P + 1 values each")
    h = np.empty(r.size, dtype=np.float64)
    ill = C.c_int(0)
    _check(lib().am_channel_solve(r.ctypes.data, c.ctypes.data, r.size // 2, float(noise_db), h.ctypes.data, C.byref(ill)))
    return h, bool(ill.value)


def hit_residual(haystack, start: int, needle, taps):
    """am_hit_residual (pure host function): (model, resid) over the S + 2P elements from start - P on -- the needle
    filtered by the hit's taps (hit_channel), and the host haystack minus that; resid is NaN where the haystack has no
    finite sample."""
    a, fmt, n = _samples(haystack)
    nd = np.ascontiguousarray(needle, dtype=np.float32)
    t = np.ascontiguousarray(taps, dtype=np.float32)
    if t.size % 2 == 0:
        raise ValueError("hit_residual: taps hold 2P + 1 values")
    model = np.empty(nd.size + t.size - 1, dtype=np.float32)
    resid = np.empty_like(model)
    _check(lib().am_hit_residual(a.ctypes.data, n, int(fmt), int(start), nd.ctypes.data, nd.size, t.ctypes.data, t.size // 2,
                                 model.ctypes.data, resid.ctypes.data))
    return model, resid


def _estimate_out(length: int):
    return np.empty(length, dtype=np.float32), np.empty(length, dtype=np.float32), np.empty(length, dtype=np.uint32)


def estimate_needle(rows, method: int = Est.MEDIAN, trim_permille: int = 0, device: int = 0):
    """am_needle_estimate_rows: (est, dev, count) of the stacked occurrences rows[i] (n x length f32, a non-finite element
    is absent): the per-sample mean, median or trimmed mean, the spread around it and the number of values it rests on."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim != 2:
        raise ValueError("rows must be a 2-d array (n x length)")
    ep = AmEstimateParams(int(method), int(trim_permille), 0, r.shape[1])
    est, dev, count = _estimate_out(r.shape[1])
    _check(lib().am_needle_estimate_rows(device, r.ctypes.data, r.shape[0], C.byref(ep), est.ctypes.data, dev.ctypes.data,
                                         count.ctypes.data))
    return est, dev, count


def estimate_needle_device(device: int, ptrs, lengths, hits, lead: int, length: int, method: int = Est.MEDIAN,
                           trim_permille: int = 0, fmt: int = Fmt.F32_MONO):
    """am_needle_estimate_device: the same from hits = [(haystack index, start, scale), ...] in the resident haystacks
    ptrs[k] (lengths[k] samples / frames); element n of a hit's row reads haystack element start - lead + n."""
    n_hay = len(ptrs)
    pp = (C.c_void_p * max(n_hay, 1))(*ptrs)
    ll = (C.c_size_t * max(n_hay, 1))(*[int(v) for v in lengths])
    hh = (AmEstHit * max(len(hits), 1))(*[AmEstHit(int(start), int(k), float(scale)) for k, start, scale in hits])
    ep = AmEstimateParams(int(method), int(trim_permille), int(lead), int(length))
    est, dev, count = _estimate_out(int(length))
    _check(lib().am_needle_estimate_device(device, pp, ll, n_hay, int(fmt), hh, len(hits), C.byref(ep), est.ctypes.data,
                                           dev.ctypes.data, count.ctypes.data))
    return est, dev, count


def find_peaks(y_data, min_prominence: float, min_distance: int = 0, device: int = 0, cap: int = 65536):
    """audio_matcher.rs:221-230 on the GPU; peaks by descending height."""
    a = np.ascontiguousarray(y_data, dtype=np.float32)
    buf = (AmPeak * cap)()
    n = C.c_size_t(0)
    _check(lib().am_find_peaks(device, a.ctypes.data, a.size, float(min_prominence), int(min_distance),
                               buf, cap, C.byref(n)))
    return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]


def find_peaks_top(y_data, k: int, min_prominence: float = 0.0, min_distance: int = 0, device: int = 0):
    """am_find_peaks_top: the first min(k, count) peaks find_peaks(y_data, min_prominence, min_distance) returns, by
    descending height, without computing all of them.  A non-finite score splits the array."""
    a = np.ascontiguousarray(y_data, dtype=np.float32)
    buf = (AmPeak * max(1, int(k)))()
    n = C.c_size_t(0)
    _check(lib().am_find_peaks_top(device, a.ctypes.data, a.size, float(min_prominence), int(min_distance), int(k),
                                   buf, C.byref(n)))
    return _peaks(buf, n.value)


def find_peaks_top_device(device: int, ptr: int, n: int, k: int, min_prominence: float = 0.0, min_distance: int = 0):
    """am_find_peaks_top_device: the same on n f32 scores resident on `device`."""
    buf = (AmPeak * max(1, int(k)))()
    got = C.c_size_t(0)
    _check(lib().am_find_peaks_top_device(device, ptr, int(n), float(min_prominence), int(min_distance), int(k),
                                          buf, C.byref(got)))
    return _peaks(buf, got.value)


def trace_len(n_scores: int, bin: int) -> int:
    """am_trace_len: ceil(n_scores / bin), the records a trace of n_scores scores has (pure host)."""
    n = C.c_size_t(0)
    _check(lib().am_trace_len(int(n_scores), int(bin), C.byref(n)))
    return n.value


def trace_params(bin: int, scale=Scale.LIB) -> AmTraceParams:
    """am_trace_params (scale: Scale.NONE or Scale.LIB, or a bool as in correlate_with_sample)."""
    sc = int(Scale.LIB if scale is True else Scale.NONE if scale is False else scale)
    return AmTraceParams(bin=int(bin), scale=sc, reserved=0)


def _records_call(fn, dtype, cap):
    """Runs fn(out_ptr, cap, byref(n)) on an array of `cap` records of `dtype`; the records written."""
    cap = int(cap)
    out = np.zeros(max(1, cap), dtype=dtype)
    n = C.c_size_t(0)
    _check(fn(out.ctypes.data, cap, C.byref(n)))
    return out[:min(n.value, cap)]


def _trace_call(fn, n_scores: int, bin: int, cap):
    """_records_call on `cap` trace records (default: all bins)."""
    nb = trace_len(n_scores, bin)
    return _records_call(fn, TRACE_BIN_DTYPE, nb if cap is None else cap)


def trace_scores(y_data, bin: int, device: int = 0, cap=None):
    """am_trace_scores: per bin of `bin` scores of the host array y_data one record (TRACE_BIN_DTYPE): max, min, their
    offsets in the bin, the count of scores that are not NaN, their f64 sum and sum of squares."""
    a = np.ascontiguousarray(y_data, dtype=np.float32)
    return _trace_call(lambda o, c, n: lib().am_trace_scores(device, a.ctypes.data, a.size, int(bin), o, c, n), a.size, bin, cap)


def trace_scores_device(device: int, ptr: int, n: int, bin: int, cap=None):
    """am_trace_scores_device: the same on n f32 scores resident on `device` (any 4-byte alignment)."""
    return _trace_call(lambda o, c, m: lib().am_trace_scores_device(device, ptr, int(n), int(bin), o, c, m), n, bin, cap)


def trace_summary(bins, bin: int) -> AmTraceStats:
    """am_trace_summary: count, global max / min with their score offsets, mean, std, the median and MAD of the bin
    maxima and peak_z of a trace's records (pure host)."""
    a = np.ascontiguousarray(bins, dtype=TRACE_BIN_DTYPE)
    st = AmTraceStats()
    _check(lib().am_trace_summary(a.ctypes.data if a.size else None, a.size, int(bin), C.byref(st)))
    return st


def discover_params(probe_len: int, hop: int, exclude: int = 0, separation: int = 0, min_level_db: float = 40.0,
                    flags: int = 0) -> AmDiscoverParams:
    """am_discover_params (flags: AM_DISCOVER_SELF; separation 0 = probe_len)."""
    return AmDiscoverParams(probe_len=int(probe_len), hop=int(hop), exclude=int(exclude), separation=int(separation),
                            min_level_db=float(min_level_db), flags=int(flags), reserved=0)


def region_params(min_ncc: float, tolerance: int, min_good: int = 2, max_gap: int = 1, max_second: float = 0.0,
                  flags: int = 0) -> AmRegionParams:
    """am_region_params (flags: AM_REGION_FOLD, only for records of an AM_DISCOVER_SELF search)."""
    return AmRegionParams(min_ncc=float(min_ncc), max_second=float(max_second), tolerance=int(tolerance),
                          min_good=int(min_good), max_gap=int(max_gap), flags=int(flags), reserved=0)


def discover_len(len_a: int, params: AmDiscoverParams) -> int:
    """am_discover_len: the probes a recording of len_a samples has (pure host)."""
    n = C.c_size_t(0)
    _check(lib().am_discover_len(int(len_a), C.byref(params), C.byref(n)))
    return n.value


def _discover_call(fn, len_a: int, params: AmDiscoverParams, cap):
    return _records_call(fn, PROBE_HIT_DTYPE, discover_len(len_a, params) if cap is None else cap)


def discover(a, b, params: AmDiscoverParams, device: int = 0, cap=None):
    """am_discover: one PROBE_HIT_DTYPE record per probe of recording `a` matched against recording `b` (both f32
    arrays, or both i16 (frames, 2) arrays of interleaved stereo); pass b = a with AM_DISCOVER_SELF for a self search."""
    xa, fa, la = _samples(a)
    xb, fb, lb = _samples(b)
    if fa != fb:
        raise ValueError("discover: both recordings must have one sample format")
    return _discover_call(lambda o, c, n: lib().am_discover(device, xa.ctypes.data, la, xb.ctypes.data, lb, int(fa), C.byref(params),
                                                            o, c, n), la, params, cap)


def discover_device(device: int, ptr_a: int, len_a: int, ptr_b: int, len_b: int, params: AmDiscoverParams,
                    fmt: int = Fmt.F32_MONO, cap=None):
    """am_discover_device: the same on recordings resident on `device`."""
    return _discover_call(lambda o, c, n: lib().am_discover_device(device, ptr_a, int(len_a), ptr_b, int(len_b), int(fmt),
                                                                   C.byref(params), o, c, n), len_a, params, cap)


def probe_scores(y_data, ex_lo: int, ex_hi: int, separation: int, device: int = 0):
    """am_probe_scores: the record rule of discovery on the host score array y_data -- the best candidate outside
    [ex_lo, ex_hi) and the largest one at least `separation` away from it (one PROBE_HIT_DTYPE record)."""
    a = np.ascontiguousarray(y_data, dtype=np.float32)
    out = np.zeros(1, dtype=PROBE_HIT_DTYPE)
    _check(lib().am_probe_scores(device, a.ctypes.data if a.size else None, a.size, int(ex_lo), int(ex_hi), int(separation),
                                 out.ctypes.data))
    return out[0]


def probe_scores_device(device: int, ptr: int, n: int, ex_lo: int, ex_hi: int, separation: int):
    """am_probe_scores_device: the same on n f32 scores resident on `device` (any 4-byte alignment)."""
    out = np.zeros(1, dtype=PROBE_HIT_DTYPE)
    _check(lib().am_probe_scores_device(device, ptr, int(n), int(ex_lo), int(ex_hi), int(separation), out.ctypes.data))
    return out[0]


def discover_regions(hits, params: AmDiscoverParams, rparams: AmRegionParams, cap=None):
    """am_discover_regions: the regions (REGION_DTYPE) the probes' records chain into (pure host)."""
    h = np.ascontiguousarray(hits, dtype=PROBE_HIT_DTYPE)
    return _records_call(lambda o, c, n: lib().am_discover_regions(h.ctypes.data if h.size else None, h.size, C.byref(params),
                                                                   C.byref(rparams), o, c, n),
                         REGION_DTYPE, h.size if cap is None else cap)


def edge_params(min_overlap: int, separation: int = 0, min_share: float = 0.05) -> AmEdgeParams:
    """am_edge_params (separation 0 = min_overlap; min_share: least E_n(u) / E_n of a candidate lag)."""
    return AmEdgeParams(min_overlap=int(min_overlap), separation=int(separation), min_share=float(min_share), reserved=0)


def edge_scores_len(length: int, s: int, edge: int):
    """am_edge_scores_len: (n_lags, first_lag) of an edge for a haystack of `length` and a needle of `s` samples (pure host)."""
    n, first = C.c_size_t(0), C.c_int64(0)
    _check(lib().am_edge_scores_len(int(length), int(s), int(edge), C.byref(n), C.byref(first)))
    return n.value, first.value


def env_params(bands: AmBandParams, floor_db: float = 80.0) -> AmEnvParams:
    """am_env_params: the bands (band_params or band_edges_log) and the level floor in dB below a full-scale sine."""
    ep = AmEnvParams()
    ep.bands = bands
    ep.reserved = 0
    ep.floor_db = float(floor_db)
    return ep


def env_grid(max_ppm: float, steps: int, centre_ppm: float = 0.0) -> AmEnvGrid:
    """am_env_grid: the 2 * steps + 1 drifts centre_ppm - max_ppm .. centre_ppm + max_ppm."""
    return AmEnvGrid(centre_ppm=float(centre_ppm), max_ppm=float(max_ppm), steps=int(steps), reserved=0)


def env_grid_drifts(grid: AmEnvGrid):
    """The drifts d_q of a grid, in ppm (the rule of include/audiomatch.h in f64)."""
    k = int(grid.steps)
    if k == 0:
        return np.array([grid.centre_ppm], dtype=np.float64)
    return np.array([grid.centre_ppm + grid.max_ppm * float(q - k) / float(k) for q in range(2 * k + 1)], dtype=np.float64)


def envelope_len(length: int, ep: AmEnvParams, drift_ppm: float = 0.0) -> int:
    """am_envelope_len: the frames J of a signal of `length` samples at drift_ppm (pure host)."""
    n = C.c_size_t(0)
    _check(lib().am_envelope_len(int(length), C.byref(ep), float(drift_ppm), C.byref(n)))
    return n.value


def _envelope_call(fn, length: int, ep: AmEnvParams, drift_ppm: float, cap):
    j = envelope_len(length, ep, drift_ppm)
    cap = j if cap is None else int(cap)
    nb = int(ep.bands.n_bands)
    out = np.zeros(max(1, nb * cap), dtype=np.uint16)
    n = C.c_size_t(0)
    _check(fn(out.ctypes.data, cap, C.byref(n)))
    return out[:nb * n.value].reshape(nb, n.value)   # (band-major with J frames per band, whatever cap was)


def envelope(signal, ep: AmEnvParams, drift_ppm: float = 0.0, device: int = 0, cap=None):
    """am_envelope: the (B, J) uint16 band levels of a host signal (f32, or i16 (frames, 2) interleaved stereo) read at
    drift_ppm; AM_ENV_ABSENT marks a frame with a non-finite sample."""
    a, fmt, length = _samples(signal)
    return _envelope_call(lambda o, c, n: lib().am_envelope(device, a.ctypes.data, length, int(fmt), C.byref(ep), float(drift_ppm), o, c, n),
                          length, ep, drift_ppm, cap)


def envelope_device(device: int, ptr: int, length: int, ep: AmEnvParams, drift_ppm: float = 0.0, fmt: int = Fmt.F32_MONO, cap=None):
    """am_envelope_device: the same of a signal resident on `device`."""
    return _envelope_call(lambda o, c, n: lib().am_envelope_device(device, ptr, int(length), int(fmt), C.byref(ep), float(drift_ppm), o, c, n),
                          length, ep, drift_ppm, cap)


def _env_bank(needles):
    mats = [np.ascontiguousarray(m, dtype=np.uint16) for m in needles]
    frames = np.array([m.shape[1] for m in mats], dtype=np.uint32)
    bank = np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0, dtype=np.uint16)
    return mats, frames, bank


def _env_scores_call(fn, frames, hay_frames: int, cap):
    n_all = max([hay_frames - int(j) + 1 for j in frames if hay_frames >= int(j)], default=0)
    cap = n_all if cap is None else int(cap)
    z = np.zeros(max(1, cap), dtype=np.float32)
    qi = np.zeros(max(1, cap), dtype=np.uint32)
    n = C.c_size_t(0)
    _check(fn(z.ctypes.data, qi.ctypes.data, cap, C.byref(n)))
    m = min(n.value, cap)
    return z[:m], qi[:m]


def envelope_scores(needles, hay, device: int = 0, cap=None):
    """am_envelope_scores: (z, qi) of a list of (B, J_q) uint16 needle matrices against the (B, Jh) haystack matrix --
    per place t the largest score over the needles and its needle (AM_ENV_NO_Q beside a NaN)."""
    mats, frames, bank = _env_bank(needles)
    e = np.ascontiguousarray(hay, dtype=np.uint16)
    nb = e.shape[0]
    return _env_scores_call(lambda z, q, c, n: lib().am_envelope_scores(device, bank.ctypes.data, frames.ctypes.data, len(mats), nb,
                                                                        e.ctypes.data if e.size else None, e.shape[1], z, q, c, n),
                            frames, e.shape[1], cap)


def envelope_scores_device(device: int, ptr_needles: int, frames, n_bands: int, ptr_hay: int, hay_frames: int, cap=None):
    """am_envelope_scores_device: the same on matrices resident on `device` (the needle matrices one behind the other)."""
    fr = np.ascontiguousarray(frames, dtype=np.uint32)
    return _env_scores_call(lambda z, q, c, n: lib().am_envelope_scores_device(device, ptr_needles, fr.ctypes.data, fr.size, int(n_bands),
                                                                               ptr_hay, int(hay_frames), z, q, c, n),
                            fr, int(hay_frames), cap)


def envelope_pick(z, qi, min_score: float, separation: int, cap=None):
    """am_envelope_pick: the places (ENV_PICK_DTYPE) of a score array that are its largest within +-separation (pure host)."""
    zz = np.ascontiguousarray(z, dtype=np.float32)
    qq = np.ascontiguousarray(qi, dtype=np.uint32)
    return _records_call(lambda o, c, n: lib().am_envelope_pick(zz.ctypes.data if zz.size else None, qq.ctypes.data if qq.size else None,
                                                                zz.size, float(min_score), int(separation), o, c, n),
                         ENV_PICK_DTYPE, zz.size if cap is None else cap)


def _env_match_call(fn, cap):
    return _records_call(fn, ENV_HIT_DTYPE, 1024 if cap is None else cap)


def best_params(k: int, min_distance: int = 0, min_prominence: float = 0.0, scale=Scale.LIB) -> AmBestParams:
    """am_best_params of the k best matches (scale: Scale.NONE or Scale.LIB, or a bool as in correlate_with_sample)."""
    sc = int(Scale.LIB if scale is True else Scale.NONE if scale is False else scale)
    return AmBestParams(k=int(k), min_distance=int(min_distance), min_prominence=float(min_prominence), scale=sc)


@dataclass
class HitScore:
    """am_hit_score: exact NCC, least-squares gain, window level and sub-sample position of one hit."""
    position: float
    ncc: float
    gain: float
    window_db: float
    flags: int


def _am_peak(q) -> AmPeak:
    return AmPeak(int(q.start), int(q.end), float(q.height), float(q.prominence))


def _peak_array(peaks):
    k = len(peaks)
    return (AmPeak * max(1, k))(*[_am_peak(q) for q in peaks])


@dataclass
class SegmentSummary:
    """am_segment_summary: coverage, drift and refined start of one hit, from its segment records."""
    coverage: float
    drift_ppm: float
    start_lag: float
    residual_rms: float
    first_present: int
    last_present: int
    n_present: int
    n_usable: int


def hit_segments_summary(segments, needle_len: int, min_ncc: float = 0.5) -> SegmentSummary:
    """am_hit_segments_summary (pure host code): `segments` = one hit's HitSegment records."""
    m = len(segments)
    buf = (HitSegment * max(1, m))(*[HitSegment(q.lag, q.ncc, q.gain, q.level_db, q.flags) for q in segments])
    out = AmSegmentSummary()
    _check(lib().am_hit_segments_summary(buf, m, int(needle_len), float(min_ncc), C.byref(out)))
    return SegmentSummary(out.coverage, out.drift_ppm, out.start_lag, out.residual_rms, out.first_present,
                          out.last_present, out.n_present, out.n_usable)


@dataclass
class StereoSummary:
    """am_stereo_summary: where one hit sits between the channels, from its HitStereo record."""
    image: int
    balance_db: float
    delay: float
    downmix_loss_db: float


def hit_stereo_summary(rec, min_ncc: float = 0.5) -> StereoSummary:
    """am_hit_stereo_summary (pure host code): `rec` = one hit's HitStereo record."""
    out = AmStereoSummary()
    _check(lib().am_hit_stereo_summary(C.byref(HitStereo.from_buffer_copy(bytes(rec))), float(min_ncc), C.byref(out)))
    return StereoSummary(int(out.image), out.balance_db, out.delay, out.downmix_loss_db)


def band_params(frame_log2: int, edges) -> AmBandParams:
    """am_band_params for F = 2^frame_log2 and the bands [edges[b], edges[b + 1]) (bin indices)."""
    edges = [int(e) for e in edges]
    bp = AmBandParams(int(frame_log2), max(len(edges) - 1, 0))
    for b, e in enumerate(edges[:AM_BAND_MAX_BANDS + 1]):
        bp.edges[b] = e
    return bp


def band_edges_log(sr: int, frame_log2: int, lo_hz: float, hi_hz: float, n_bands: int) -> AmBandParams:
    """am_band_edges_log (pure host code): n_bands log-spaced bands from lo_hz to hi_hz at sample rate sr."""
    out = AmBandParams()
    _check(lib().am_band_edges_log(int(sr), int(frame_log2), float(lo_hz), float(hi_hz), int(n_bands), C.byref(out)))
    return out


@dataclass
class BandSummary:
    """am_band_summary: how much of the needle's spectrum one hit holds, from its band records."""
    coverage: float
    weighted_coherence: float
    gain_db_spread: float
    first_present: int
    last_present: int
    n_present: int
    n_countable: int


def hit_bands_summary(bands, min_coherence: float = 0.5) -> BandSummary:
    """am_hit_bands_summary (pure host code): `bands` = one hit's HitBand records."""
    nb = len(bands)
    buf = (HitBand * max(1, nb))(*[HitBand(q.ncc, q.coherence, q.gain, q.level_db, q.needle_share, q.flags) for q in bands])
    out = AmBandSummary()
    _check(lib().am_hit_bands_summary(buf, nb, float(min_coherence), C.byref(out)))
    return BandSummary(out.coverage, out.weighted_coherence, out.gain_db_spread, out.first_present, out.last_present,
                       out.n_present, out.n_countable)


# ---------------------------------------------------------------------------
# Per-hit records.  A family is one kind of record: `symbol` names its host entry point (symbol + "_device" and symbol +
# "_batch_device" are the other two), `record` is its ctypes type, params(*public arguments after the peaks) gives the
# parameter struct (None: the family has none) and m, the records per hit, and unpack(out, i, m) is what the caller gets
# for hit i of the call -- one object, or the list of its m records.  Every unpacked record is a copy: it outlives `out`.
class _HitFamily:
    def __init__(self, symbol, record, params, unpack):
        self.symbol, self.record, self.params, self.unpack = symbol, record, params, unpack


_SCORES = _HitFamily(
    "am_hit_scores", AmHitScore, lambda: (None, 1),
    lambda out, i, m: HitScore(out[i].position, out[i].ncc, out[i].gain, out[i].window_db, int(out[i].flags)))
_SEGMENTS = _HitFamily(
    "am_hit_segments", HitSegment, lambda segments, radius: (AmSegmentParams(int(segments), int(radius)), int(segments)),
    lambda out, i, m: [HitSegment(q.lag, q.ncc, q.gain, q.level_db, q.flags) for q in (out[i * m + j] for j in range(m))])
_WARP = _HitFamily(
    "am_hit_warp", HitWarp, lambda wp: (wp, 1), lambda out, i, m: HitWarp.from_buffer_copy(bytes(out[i])))
_BANDS = _HitFamily(
    "am_hit_bands", HitBand, lambda bp: (bp, int(bp.n_bands)),
    lambda out, i, m: [HitBand.from_buffer_copy(out[i * m + b]) for b in range(m)])
_STEREO = _HitFamily(
    "am_hit_stereo", HitStereo, lambda radius: (AmStereoParams(int(radius), 0), 1),
    lambda out, i, m: HitStereo.from_buffer_copy(out[i]))
_MASK = _HitFamily("am_hit_mask", HitMask, lambda: (None, 1), lambda out, i, m: HitMask.from_buffer_copy(out[i]))
_SIGNIFICANCE = _HitFamily(
    "am_hit_significance", HitSignificance, lambda guard, radius: (AmSignificanceParams(int(guard), int(radius)), 1),
    lambda out, i, m: HitSignificance.from_buffer_copy(out[i]))


def _hit_call(fam, form, lead, n_hits, args):
    """One form's call: `lead`, then the parameter struct if the family has one, then `out`, sized for n_hits hits (a
    negative m sizes it as 0 and goes to the library, which refuses it).  Returns (out, m)."""
    params, m = fam.params(*args)
    out = (fam.record * max(1, n_hits * max(m, 0)))()
    tail = (out,) if params is None else (C.byref(params), out)
    _check(getattr(lib(), fam.symbol + form)(*lead, *tail))
    return out, m


def _hit_device(fam, algo, ptr, length, peaks, fmt, args, form="_device"):
    """[i] = the records of peaks[i] in a haystack resident on the needle's device."""
    k = len(peaks)
    out, m = _hit_call(fam, form, (algo._h, ptr, length, int(fmt), _peak_array(peaks), k), k, args)
    return [fam.unpack(out, i, m) for i in range(k)]


def _hit_host(fam, algo, haystack, peaks, args):
    """The same for a host haystack: an f32 array, or an i16 (frames, 2) array of interleaved stereo."""
    a, fmt, length = _samples(haystack)
    return _hit_device(fam, algo, a.ctypes.data, length, peaks, fmt, args, form="")


def _hit_batch(fam, algos, ptrs, lengths, peaks_per_pair, fmt, args):
    """[h][j][i] = the records of hit i of peaks_per_pair[h][j] (resident haystack h against needle j): the pair's hits
    stand in slot h * nn + j of a table of `cap` rows a slot, its records in the same rows of `out`."""
    nn, k = len(algos), len(ptrs)
    pairs = [peaks_per_pair[h][j] for h in range(k) for j in range(nn)]
    cap = max([1] + [len(hits) for hits in pairs])
    handles = (C.c_void_p * max(1, nn))(*[a._h for a in algos])
    arr_p = (C.c_void_p * max(1, k))(*ptrs)
    arr_l = (C.c_size_t * max(1, k))(*lengths)
    buf = (AmPeak * max(1, cap * k * nn))()
    counts = (C.c_size_t * max(1, k * nn))(*[len(hits) for hits in pairs])
    for q, hits in enumerate(pairs):
        for i, p in enumerate(hits):
            buf[q * cap + i] = _am_peak(p)
    out, m = _hit_call(fam, "_batch_device", (handles, nn, arr_p, arr_l, k, int(fmt), buf, cap, counts), cap * k * nn, args)
    return [[[fam.unpack(out, (h * nn + j) * cap + i, m) for i in range(counts[h * nn + j])] for j in range(nn)]
            for h in range(k)]


def _channel_call(form, lead, n_hits, cp):
    """One form of am_hit_channel: `lead`, the parameters, then the records and the taps, sized for n_hits hits.  Returns
    (records, taps [n_hits, 2P + 1])."""
    out = (HitChannel * max(1, n_hits))()
    taps = np.zeros((max(1, n_hits), 2 * int(cp.radius) + 1), dtype=np.float32)
    _check(getattr(lib(), "am_hit_channel" + form)(*lead, C.byref(cp), out, taps.ctypes.data))
    return out, taps


def _channel_device(algo, ptr, length, peaks, fmt, cp, form="_device"):
    k = len(peaks)
    out, taps = _channel_call(form, (algo._h, ptr, length, int(fmt), _peak_array(peaks), k), k, cp)
    return [HitChannel.from_buffer_copy(out[i]) for i in range(k)], taps[:k].copy()


# ---------------------------------------------------------------------------
@dataclass
class Peak:
    """find_peaks::Peak<f32> as used downstream (position, height, prominence)."""
    start: int
    end: int
    height: float
    prominence: float

    @property
    def position(self):
        return range(self.start, self.end)


@dataclass
class Config:
    """audio_matcher.rs:25-53 (Config + PeakConfig), durations in seconds."""
    chunk_size_s: float = 60.0          # matcher/args.rs:70-72
    overlap_length_s: float = 0.0       # Config::from_args sets it to the snippet duration (:41)
    distance_s: float = 8 * 60.0        # matcher/args.rs:73-76
    prominence: float = 13.0 / 100.0    # args.prominence / 100 (:44), default 13 (args.rs:19)

    def params(self, sr: int, scale: int) -> AmMatchParams:
        def rnd(x):                     # f64::round: half away from zero (audio_matcher.rs:99-100)
            return int(np.floor(x + 0.5))
        return AmMatchParams(
            sr=sr, chunk=rnd(self.chunk_size_s * sr), overlap=rnd(self.overlap_length_s * sr),
            min_prominence=self.prominence,
            min_distance=int(self.distance_s) * sr,          # distance.as_secs() as usize * sr (:228)
            overshadow_distance_s=self.distance_s, scale=int(scale))


# Option keys of window-energy normalised scores (NCC, include/audiomatch.h): "score_norm" 0 = off, 1 = NCC (process
# default, or per handle: HipConvolve(score_norm=...)); "score_norm_floor_db": windows more than that many dB below the
# needle score 0.
OPT_SCORE_NORM = "score_norm"
OPT_SCORE_NORM_FLOOR_DB = "score_norm_floor_db"


class HipConvolve:
    """CorrelateAlgo<f32> (audio_matcher.rs:65-76) backed by the HIP library.

    score_norm: None follows the process default; True / False fixes this handle's "score_norm" (NCC scores,
    which need the LIB scale).
    gaps: None, or [(begin, end), ..]: spans of the needle to ignore (am_needle_create_masked: a masked needle; with
    score_norm the scores are NCC over the kept samples only).  An empty list gives the ordinary handle."""

    def __init__(self, sample_data, device: int = 0, score_norm=None, gaps=None):
        a = np.ascontiguousarray(sample_data, dtype=np.float32)
        self.device = device
        self._h = C.c_void_p()
        if gaps is None:
            _check(lib().am_needle_create(device, a.ctypes.data, a.size, C.byref(self._h)))
        else:
            arr, n = _spans(gaps)
            _check(lib().am_needle_create_masked(device, a.ctypes.data, a.size, arr, n, C.byref(self._h)))
        self.sample_len = int(a.size)
        if score_norm is not None:
            self.set_option(OPT_SCORE_NORM, int(bool(score_norm)))

    @classmethod
    def from_device(cls, device: int, ptr: int, n: int, gaps=None) -> "HipConvolve":
        self = cls.__new__(cls)
        self.device = device
        self._h = C.c_void_p()
        if gaps is None:
            _check(lib().am_needle_create_device(device, ptr, n, C.byref(self._h)))
        else:
            arr, k = _spans(gaps)
            _check(lib().am_needle_create_masked_device(device, ptr, n, arr, k, C.byref(self._h)))
        self.sample_len = int(n)
        return self

    def mask(self):
        """am_needle_mask: the handle's gaps as [(begin, end), ..]; [] for an ordinary handle."""
        arr = (AmSpan * AM_MASK_MAX_GAPS)()
        n = C.c_size_t(0)
        _check(lib().am_needle_mask(self._h, arr, AM_MASK_MAX_GAPS, C.byref(n)))
        return [(int(g.begin), int(g.end)) for g in arr[:n.value]]

    @classmethod
    def from_pcm16(cls, interleaved, device: int = 0) -> "HipConvolve":
        """Needle given as interleaved i16 stereo frames (down-mixed on the GPU)."""
        a = np.ascontiguousarray(interleaved, dtype=np.int16)
        self = cls.__new__(cls)
        self.device = device
        self._h = C.c_void_p()
        _check(lib().am_needle_create_pcm16(device, a.ctypes.data, a.size // 2, C.byref(self._h)))
        self.sample_len = int(a.size // 2)
        return self

    @classmethod
    def resampled(cls, needle, src_rate: int, dst_rate: int, device: int = 0, score_norm=None) -> "HipConvolve":
        """am_needle_create_resampled: the needle (f32, or int16 interleaved stereo) brought from src_rate to the
        haystack's dst_rate; the same handle as HipConvolve(resample(needle, src_rate, dst_rate))."""
        a, fmt, length = _samples(needle)
        self = cls.__new__(cls)
        self.device = device
        self._h = C.c_void_p()
        _check(lib().am_needle_create_resampled(device, a.ctypes.data, length, int(fmt), int(src_rate), int(dst_rate),
                                                C.byref(self._h)))
        n = C.c_size_t(0)
        _check(lib().am_needle_len(self._h, C.byref(n)))
        self.sample_len = int(n.value)
        if score_norm is not None:
            self.set_option(OPT_SCORE_NORM, int(bool(score_norm)))
        return self

    @classmethod
    def filtered(cls, needle, taps, device: int = 0, score_norm=None) -> "HipConvolve":
        """am_needle_create_filtered: the needle (f32, or int16 interleaved stereo) passed through the FIR filter `taps`
        (whiten_taps of the haystacks' lag_products, or a pre-emphasis [1, -alpha]); the same handle as
        HipConvolve(fir(needle, taps)).  Every haystack it is matched against must pass through the same taps."""
        a, fmt, length = _samples(needle)
        t, tp = _taps(taps)
        self = cls.__new__(cls)
        self.device = device
        self._h = C.c_void_p()
        _check(lib().am_needle_create_filtered(device, a.ctypes.data, length, int(fmt), tp, t.size, C.byref(self._h)))
        self.sample_len = int(length)
        if score_norm is not None:
            self.set_option(OPT_SCORE_NORM, int(bool(score_norm)))
        return self

    def match_pcm16(self, interleaved, params: AmMatchParams, cap: int = 4096):
        a = np.ascontiguousarray(interleaved, dtype=np.int16)
        buf = (AmPeak * cap)()
        n = C.c_size_t(0)
        _check(lib().am_match_pcm16(self._h, a.ctypes.data, a.size // 2, C.byref(params), buf, cap, C.byref(n)))
        return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]

    def set_option(self, key: str, value: int):
        """Per-handle "log_n" / "half_pipeline" / "score_norm" (-1 = follow the process default)."""
        _check(lib().am_needle_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_longlong(0)
        _check(lib().am_needle_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def match_pcm16_batch_device(self, ptrs, frames, params: AmMatchParams, cap_per_hay: int = 256):
        k = len(ptrs)
        arr_p = (C.c_void_p * k)(*ptrs)
        arr_l = (C.c_size_t * k)(*frames)
        buf = (AmPeak * (cap_per_hay * k))()
        counts = (C.c_size_t * k)()
        _check(lib().am_match_pcm16_batch_device(self._h, arr_p, arr_l, k, C.byref(params), buf,
                                                 cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)

    def match_pcm16_device(self, ptr: int, frames: int, params: AmMatchParams, cap: int = 4096):
        buf = (AmPeak * cap)()
        n = C.c_size_t(0)
        _check(lib().am_match_pcm16_device(self._h, ptr, frames, C.byref(params), buf, cap, C.byref(n)))
        return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]

    def close(self):
        if getattr(self, "_h", None):
            lib().am_needle_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def inverse_sample_auto_correlation(self) -> float:
        v = C.c_float(0)
        _check(lib().am_needle_inv_autocorr(self._h, C.byref(v)))
        return v.value

    def correlate_with_sample(self, within, mode: Mode = Mode.Valid, scale=False) -> np.ndarray:
        """scale: bool as in the reference (True = production/LibConvolve) or a Scale value."""
        w = np.ascontiguousarray(within, dtype=np.float32)
        sc = int(Scale.LIB if scale is True else Scale.NONE if scale is False else scale)
        n = C.c_size_t(0)
        _check(lib().am_correlate_len(w.size, self.sample_len, int(mode), C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        _check(lib().am_correlate(self._h, w.ctypes.data, w.size, int(mode), sc,
                                  out.ctypes.data, out.size, C.byref(n)))
        return out

    # -- level 2 --
    def match(self, haystack, params: AmMatchParams, cap: int = 4096):
        h = np.ascontiguousarray(haystack, dtype=np.float32)
        buf = (AmPeak * cap)()
        n = C.c_size_t(0)
        _check(lib().am_match(self._h, h.ctypes.data, h.size, C.byref(params), buf, cap, C.byref(n)))
        return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]

    def match_device(self, ptr: int, length: int, params: AmMatchParams, cap: int = 4096):
        buf = (AmPeak * cap)()
        n = C.c_size_t(0)
        _check(lib().am_match_device(self._h, ptr, length, C.byref(params), buf, cap, C.byref(n)))
        return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]

    def match_batch_device(self, ptrs, lengths, params: AmMatchParams, cap_per_hay: int = 256):
        k = len(ptrs)
        arr_p = (C.c_void_p * k)(*ptrs)
        arr_l = (C.c_size_t * k)(*lengths)
        buf = (AmPeak * (cap_per_hay * k))()
        counts = (C.c_size_t * k)()
        _check(lib().am_match_batch_device(self._h, arr_p, arr_l, k, C.byref(params), buf,
                                           cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)


    # -- the k best matches --
    def match_best(self, haystack, k: int, min_distance: int = 0, min_prominence: float = 0.0, scale=Scale.LIB):
        """am_match_best: the k best peaks of the haystack's Valid scores (one array, no chunks), by descending height.
        haystack: an f32 array, or an i16 (frames, 2) array of interleaved stereo."""
        a, fmt, length = _samples(haystack)
        bp = best_params(k, min_distance, min_prominence, scale)
        buf = (AmPeak * max(1, int(k)))()
        n = C.c_size_t(0)
        _check(lib().am_match_best(self._h, a.ctypes.data, length, int(fmt), C.byref(bp), buf, C.byref(n)))
        return _peaks(buf, n.value)

    def match_best_device(self, ptr: int, length: int, params: AmBestParams, fmt: int = Fmt.F32_MONO):
        """am_match_best_device on a haystack resident on this needle's device."""
        buf = (AmPeak * max(1, int(params.k)))()
        n = C.c_size_t(0)
        _check(lib().am_match_best_device(self._h, ptr, length, int(fmt), C.byref(params), buf, C.byref(n)))
        return _peaks(buf, n.value)

    def match_best_batch_device(self, ptrs, lengths, params: AmBestParams, fmt: int = Fmt.F32_MONO):
        """am_match_best_batch_device: one list of the k best peaks per resident haystack."""
        nh = len(ptrs)
        k = int(params.k)
        arr_p = (C.c_void_p * max(1, nh))(*ptrs)
        arr_l = (C.c_size_t * max(1, nh))(*lengths)
        buf = (AmPeak * max(1, k * nh))()
        counts = (C.c_size_t * max(1, nh))()
        _check(lib().am_match_best_batch_device(self._h, arr_p, arr_l, nh, int(fmt), C.byref(params), buf, counts))
        return _split_batch(buf, counts, nh, k)

    # -- score traces --
    def match_trace(self, haystack, bin: int, scale=Scale.LIB, cap=None):
        """am_match_trace: one TRACE_BIN_DTYPE record per `bin` Valid scores of the haystack (the array match_best
        selects from).  haystack: an f32 array, or an i16 (frames, 2) array of interleaved stereo."""
        a, fmt, length = _samples(haystack)
        tp = trace_params(bin, scale)
        return _trace_call(lambda o, c, n: lib().am_match_trace(self._h, a.ctypes.data, length, int(fmt), C.byref(tp), o, c, n),
                           max(0, length - self.sample_len + 1), bin, cap)

    def match_trace_device(self, ptr: int, length: int, params: AmTraceParams, fmt: int = Fmt.F32_MONO, cap=None):
        """am_match_trace_device on a haystack resident on this needle's device."""
        return _trace_call(lambda o, c, n: lib().am_match_trace_device(self._h, ptr, length, int(fmt), C.byref(params), o, c, n),
                           max(0, length - self.sample_len + 1), params.bin, cap)

    def match_trace_batch_device(self, ptrs, lengths, params: AmTraceParams, fmt: int = Fmt.F32_MONO, cap_per_hay=None):
        """am_match_trace_batch_device: one record array per resident haystack."""
        nh = len(ptrs)
        nbs = [trace_len(max(0, int(l) - self.sample_len + 1), params.bin) for l in lengths]
        cap = max(nbs, default=0) if cap_per_hay is None else int(cap_per_hay)
        arr_p = (C.c_void_p * max(1, nh))(*ptrs)
        arr_l = (C.c_size_t * max(1, nh))(*lengths)
        out = np.zeros(max(1, cap * nh), dtype=TRACE_BIN_DTYPE)
        counts = (C.c_size_t * max(1, nh))()
        _check(lib().am_match_trace_batch_device(self._h, arr_p, arr_l, nh, int(fmt), C.byref(params), out.ctypes.data, cap, counts))
        return [out[i * cap:i * cap + min(counts[i], cap)].copy() for i in range(nh)]

    # -- edge matching --
    def _edge_scores_call(self, fn, length: int, edge: int, cap):
        cap = edge_scores_len(length, self.sample_len, edge)[0] if cap is None else int(cap)
        out = np.zeros(max(1, cap), dtype=np.float32)
        n = C.c_size_t(0)
        _check(fn(out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)]

    def edge_scores(self, haystack, edge: int, params: AmEdgeParams, cap=None):
        """am_edge_scores: the coarse partial-overlap NCC of every lag of one edge (AM_EDGE_HEAD / AM_EDGE_TAIL) of a host
        haystack (f32, or i16 (frames, 2) interleaved stereo) in ascending lag, NaN where the lag is no candidate."""
        a, fmt, length = _samples(haystack)
        return self._edge_scores_call(lambda o, c, n: lib().am_edge_scores(self._h, a.ctypes.data, length, int(fmt), int(edge),
                                                                           C.byref(params), o, c, n), length, edge, cap)

    def edge_scores_device(self, ptr: int, length: int, edge: int, params: AmEdgeParams, fmt: int = Fmt.F32_MONO, cap=None):
        """am_edge_scores_device on a haystack resident on this needle's device."""
        return self._edge_scores_call(lambda o, c, n: lib().am_edge_scores_device(self._h, ptr, int(length), int(fmt), int(edge),
                                                                                  C.byref(params), o, c, n), length, edge, cap)

    def match_edges(self, haystack, params: AmEdgeParams):
        """am_match_edges: the two EDGE_HIT_DTYPE records of a host haystack, [0] the head's (the recording starts inside
        the needle), [1] the tail's (it ends inside it)."""
        a, fmt, length = _samples(haystack)
        out = np.zeros(2, dtype=EDGE_HIT_DTYPE)
        _check(lib().am_match_edges(self._h, a.ctypes.data, length, int(fmt), C.byref(params), out.ctypes.data))
        return out

    def match_edges_device(self, ptr: int, length: int, params: AmEdgeParams, fmt: int = Fmt.F32_MONO):
        """am_match_edges_device on a haystack resident on this needle's device."""
        out = np.zeros(2, dtype=EDGE_HIT_DTYPE)
        _check(lib().am_match_edges_device(self._h, ptr, int(length), int(fmt), C.byref(params), out.ctypes.data))
        return out

    def match_edges_batch_device(self, ptrs, lengths, params: AmEdgeParams, fmt: int = Fmt.F32_MONO):
        """am_match_edges_batch_device: a (n_hay, 2) array of records, one pair per resident haystack."""
        nh = len(ptrs)
        arr_p = (C.c_void_p * max(1, nh))(*ptrs)
        arr_l = (C.c_size_t * max(1, nh))(*lengths)
        out = np.zeros((max(1, nh), 2), dtype=EDGE_HIT_DTYPE)
        _check(lib().am_match_edges_batch_device(self._h, arr_p, arr_l, nh, int(fmt), C.byref(params), out.ctypes.data))
        return out[:nh]

    # -- envelope matching --
    def match_envelope(self, haystack, ep: AmEnvParams, grid: AmEnvGrid, min_score: float, cap=None):
        """am_match_envelope: the occurrences (ENV_HIT_DTYPE) of this needle played at any speed of `grid` in a host
        haystack (f32, or i16 (frames, 2) interleaved stereo): start good to a few frames, drift to a grid step or two."""
        a, fmt, length = _samples(haystack)
        return _env_match_call(lambda o, c, n: lib().am_match_envelope(self._h, a.ctypes.data, length, int(fmt), C.byref(ep), C.byref(grid),
                                                                       float(min_score), o, c, n), cap)

    def match_envelope_device(self, ptr: int, length: int, ep: AmEnvParams, grid: AmEnvGrid, min_score: float,
                              fmt: int = Fmt.F32_MONO, cap=None):
        """am_match_envelope_device on a haystack resident on this needle's device."""
        return _env_match_call(lambda o, c, n: lib().am_match_envelope_device(self._h, ptr, int(length), int(fmt), C.byref(ep), C.byref(grid),
                                                                              float(min_score), o, c, n), cap)

    # -- per-hit scoring --
    def hit_scores(self, haystack, peaks):
        """am_hit_scores: score `peaks` (Peak / AmPeak) of a host haystack -- an f32 array, or an i16 (frames, 2) array
        of interleaved stereo.  Only the hits' spans are copied to the device."""
        return _hit_host(_SCORES, self, haystack, peaks, ())

    def hit_scores_device(self, ptr: int, length: int, peaks, fmt: int = Fmt.F32_MONO):
        """am_hit_scores_device: score `peaks` of a haystack resident on this needle's device."""
        return _hit_device(_SCORES, self, ptr, length, peaks, fmt, ())

    # -- the per-hit record of a masked handle --
    def hit_mask(self, haystack, peaks):
        """am_hit_mask: one HitMask per hit of a host haystack (as in hit_scores): exact masked NCC, gain and level over
        the kept samples, and what the gaps hold against the needle's original samples there."""
        return _hit_host(_MASK, self, haystack, peaks, ())

    def hit_mask_device(self, ptr: int, length: int, peaks, fmt: int = Fmt.F32_MONO):
        """am_hit_mask_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_MASK, self, ptr, length, peaks, fmt, ())

    # -- per-segment hit scoring --
    def hit_segments(self, haystack, peaks, segments: int, radius: int = 4):
        """am_hit_segments: for each of `peaks` of a host haystack (as in hit_scores) the list of its `segments`
        HitSegment records, lags -radius .. radius examined."""
        return _hit_host(_SEGMENTS, self, haystack, peaks, (segments, radius))

    def hit_segments_device(self, ptr: int, length: int, peaks, segments: int, radius: int = 4, fmt: int = Fmt.F32_MONO):
        """am_hit_segments_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_SEGMENTS, self, ptr, length, peaks, fmt, (segments, radius))

    # -- per-hit drift scoring --
    def hit_warp(self, haystack, peaks, wp: AmWarpParams):
        """am_hit_warp: for each of `peaks` of a host haystack (as in hit_scores) its HitWarp record over the grid `wp`
        (warp_params)."""
        return _hit_host(_WARP, self, haystack, peaks, (wp,))

    def hit_channel(self, haystack, peaks, cp: AmChannelParams):
        """am_hit_channel: for each of `peaks` of a host haystack (as in hit_scores) its HitChannel record and its taps
        h[-P .. P] under `cp` (channel_params): (records, taps ndarray [n, 2P + 1])."""
        a, fmt, length = _samples(haystack)
        return _channel_device(self, a.ctypes.data, length, peaks, fmt, cp, form="")

    def hit_channel_device(self, ptr: int, length: int, peaks, cp: AmChannelParams, fmt: int = Fmt.F32_MONO):
        """am_hit_channel_device: the same for a haystack resident on this needle's device."""
        return _channel_device(self, ptr, length, peaks, fmt, cp)

    def hit_stereo(self, haystack, peaks, radius: int = 4):
        """am_hit_stereo: for each of `peaks` of a host haystack of i16 stereo frames ((frames, 2) or flat) its HitStereo
        record: per channel the best of the lags -radius .. radius, the polarity and the NCC, and the NCC of the mid, the
        side and the best fixed mix."""
        return _hit_host(_STEREO, self, haystack, peaks, (radius,))

    def hit_stereo_device(self, ptr: int, length: int, peaks, radius: int = 4, fmt: int = Fmt.S16_STEREO):
        """am_hit_stereo_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_STEREO, self, ptr, length, peaks, fmt, (radius,))

    def hit_warp_device(self, ptr: int, length: int, peaks, wp: AmWarpParams, fmt: int = Fmt.F32_MONO):
        """am_hit_warp_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_WARP, self, ptr, length, peaks, fmt, (wp,))

    # -- per-band hit scoring --
    def hit_bands(self, haystack, peaks, bp: AmBandParams):
        """am_hit_bands: for each of `peaks` of a host haystack (as in hit_scores) the list of its bp.n_bands HitBand
        records (bp: band_params or band_edges_log)."""
        return _hit_host(_BANDS, self, haystack, peaks, (bp,))

    def hit_bands_device(self, ptr: int, length: int, peaks, bp: AmBandParams, fmt: int = Fmt.F32_MONO):
        """am_hit_bands_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_BANDS, self, ptr, length, peaks, fmt, (bp,))

    # -- per-hit significance --
    def hit_significance(self, haystack, peaks, guard: int, radius: int):
        """am_hit_significance: for each of `peaks` of a host haystack (as in hit_scores) its HitSignificance -- the
        hit's score against the scores at lags guard < |lag| <= radius around it."""
        return _hit_host(_SIGNIFICANCE, self, haystack, peaks, (guard, radius))

    def hit_significance_device(self, ptr: int, length: int, peaks, guard: int, radius: int, fmt: int = Fmt.F32_MONO):
        """am_hit_significance_device: the same for a haystack resident on this needle's device."""
        return _hit_device(_SIGNIFICANCE, self, ptr, length, peaks, fmt, (guard, radius))


class MatchStream:
    """calc_chunks on a haystack that arrives in pieces (am_match_stream_*): the reference's lazy
    sample iterator (audio_matcher.rs:88-97, mp3_reader.rs:13-41)."""

    def __init__(self, algo: "HipConvolve", params: AmMatchParams, expected_len: int = 0, fmt: int = Fmt.F32_MONO):
        self._algo = algo                      # keeps the needle handle alive
        self.fmt = int(fmt)
        self._s = C.c_void_p()
        _check(lib().am_match_stream_begin(algo._h, self.fmt, int(expected_len), C.byref(params), C.byref(self._s)))

    def push(self, samples):
        a = np.ascontiguousarray(samples, dtype=np.float32 if self.fmt == Fmt.F32_MONO else np.int16)
        n = a.size if self.fmt == Fmt.F32_MONO else a.size // 2
        _check(lib().am_match_stream_push(self._s, a.ctypes.data, n))

    def finish(self, cap: int = 4096):
        buf = (AmPeak * cap)()
        n = C.c_size_t(0)
        _check(lib().am_match_stream_finish(self._s, buf, cap, C.byref(n)))
        return [Peak(int(b.start), int(b.end), float(b.height), float(b.prominence)) for b in buf[:n.value]]

    def close(self):
        if getattr(self, "_s", None):
            lib().am_match_stream_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# am_peak records straight out of the result buffer's bytes (struct.iter_unpack): a third of the time of reading the
# four fields of every ctypes structure one by one -- this runs once per call, in the caller's timed loop
_PEAK_REC = struct.Struct("<QQff")
assert _PEAK_REC.size == C.sizeof(AmPeak)


def _peaks_at(buf, first: int, n: int):
    mv = memoryview(buf).cast("B")
    return [Peak(*t) for t in _PEAK_REC.iter_unpack(mv[first * _PEAK_REC.size:(first + n) * _PEAK_REC.size])]


def _split_batch(buf, counts, k: int, cap: int):
    return [_peaks_at(buf, i * cap, counts[i]) for i in range(k)]


def _peaks(buf, n):
    return _peaks_at(buf, 0, n)


def long_plan(length: int, needle_len: int, params: AmMatchParams, n_parts: int, part: int):
    """am_long_plan: (first_window, n_windows, first_sample, n_samples) of part `part` of one long haystack."""
    v = [C.c_size_t(0) for _ in range(4)]
    _check(lib().am_long_plan(length, needle_len, C.byref(params), n_parts, part, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def match_part_device(algo: "HipConvolve", ptr: int, n_samples: int, params: AmMatchParams, n_windows: int, first_sample: int,
                      fmt: int = Fmt.F32_MONO, cap: int = 4096):
    """am_match_part_device: the unmerged peaks of one part (window order, positions in the whole haystack)."""
    buf = (AmPeak * cap)()
    n = C.c_size_t(0)
    _check(lib().am_match_part_device(algo._h, ptr, n_samples, int(fmt), C.byref(params), n_windows, first_sample, buf, cap, C.byref(n)))
    return _peaks(buf, n.value)


def merge_peaks(params: AmMatchParams, peaks, cap: int = 4096):
    """am_merge_peaks: sort by start + the overshadow filter (audio_matcher.rs:132-160)."""
    k = len(peaks)
    src = (AmPeak * max(1, k))(*[AmPeak(q.start, q.end, q.height, q.prominence) for q in peaks])
    buf = (AmPeak * cap)()
    n = C.c_size_t(0)
    _check(lib().am_merge_peaks(C.byref(params), src, k, buf, cap, C.byref(n)))
    return _peaks(buf, n.value)


def merge_ready(params: AmMatchParams, peaks, horizon: int, ended: bool = False) -> int:
    """am_merge_ready: how many of `peaks` (unfiltered, sorted by start; none at or after `horizon`) have a fate under
    merge_peaks that no later peak can change (audio_matcher.rs:143-160)."""
    n = C.c_size_t(0)
    _check(lib().am_merge_ready(C.byref(params), _peak_array(peaks), len(peaks), int(horizon), int(bool(ended)), C.byref(n)))
    return n.value


@dataclass
class MonitorInfo:
    received: int        # samples / frames pushed so far
    horizon: int         # every window before this sample has been matched
    resident_bytes: int  # device bytes of the monitor's sample buffer (fixed at begin)
    pending: int         # peaks found but not yet final


class HipMonitor:
    """Live monitoring (am_monitor_*): the final hits of one or several needles while the recording arrives, in
    bounded device memory.  params: one AmMatchParams for all needles, or one per needle.  push() returns the hits
    that became final, as (needle index, Peak) sorted by (start, needle); end() returns the rest."""

    def __init__(self, algos, params, fmt: int = Fmt.F32_MONO, group_windows: int = 1):
        algos = list(algos) if isinstance(algos, (list, tuple)) else [algos]
        self._algos = algos                    # keeps the needle handles alive
        self.fmt = int(fmt)
        ps = list(params) if isinstance(params, (list, tuple)) else [params] * len(algos)
        hs = (C.c_void_p * len(algos))(*[a._h.value for a in algos])
        pa = (AmMatchParams * len(ps))(*ps)
        self._m = C.c_void_p()
        self._cap = 256
        _check(lib().am_monitor_begin(hs, len(algos), pa, self.fmt, int(group_windows), C.byref(self._m)))

    def _take(self, fn):
        while True:
            buf = (AmPeak * self._cap)()
            idx = (C.c_uint32 * self._cap)()
            n = C.c_size_t(0)
            rc = fn(self._m, buf, idx, self._cap, C.byref(n))
            if rc == AM_ERR_CAPACITY:
                self._cap = max(2 * self._cap, n.value)
                continue
            _check(rc)
            return list(zip(idx[:n.value], _peaks(buf, n.value)))

    def push(self, samples):
        a = np.ascontiguousarray(samples, dtype=np.float32 if self.fmt == Fmt.F32_MONO else np.int16)
        n = a.size if self.fmt == Fmt.F32_MONO else a.size // 2
        _check(lib().am_monitor_push(self._m, a.ctypes.data, n))
        return self.poll()

    def poll(self):
        return self._take(lib().am_monitor_poll)

    def end(self):
        return self._take(lib().am_monitor_end)

    def info(self) -> MonitorInfo:
        i = AmMonitorInfo()
        _check(lib().am_monitor_info_get(self._m, C.byref(i)))
        return MonitorInfo(i.received, i.horizon, i.resident_bytes, i.pending)

    def close(self):
        if getattr(self, "_m", None):
            lib().am_monitor_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_plan(n_items: int, n_shards: int, shard: int):
    """am_shard_plan: (first, stride, count) of the items shard `shard` owns (k mod n_shards)."""
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _check(lib().am_shard_plan(n_items, n_shards, shard, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


class Pool:
    """The haystack loop of matcher::run (matcher/mod.rs:42-87) over several GPUs: the needle
    replicated per device, haystack k matched on slot k mod n (am_pool_*)."""

    def __init__(self, sample_data, devices=None, score_norm=None):
        """score_norm: None follows the process default ("score_norm"); True / False fixes it on every slot's
        needle handle (NCC scores, which need the LIB scale)."""
        a = np.ascontiguousarray(sample_data, dtype=np.float32)
        self._p = C.c_void_p()
        if devices is None:
            _check(lib().am_pool_create(a.ctypes.data, a.size, None, 0, C.byref(self._p)))
        else:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().am_pool_create(a.ctypes.data, a.size, arr, len(devices), C.byref(self._p)))
        n = C.c_size_t(0)
        _check(lib().am_pool_size(self._p, C.byref(n)))
        self.size = n.value
        if score_norm is not None:
            for slot in range(self.size):
                h = C.c_void_p()
                _check(lib().am_pool_slot(self._p, slot, None, C.byref(h)))
                _check(lib().am_needle_set_option(h, OPT_SCORE_NORM.encode(), int(bool(score_norm))))

    def device_of(self, slot: int) -> int:
        d = C.c_int(0)
        _check(lib().am_pool_slot(self._p, slot, C.byref(d), None))
        return d.value

    def match_batch(self, haystacks, params: AmMatchParams, cap_per_hay: int = 256):
        """Host haystacks (numpy f32 arrays; None = skipped)."""
        hs = [None if h is None else np.ascontiguousarray(h, dtype=np.float32) for h in haystacks]
        k = len(hs)
        arr_p = (C.c_void_p * k)(*[None if h is None else h.ctypes.data for h in hs])
        arr_l = (C.c_size_t * k)(*[0 if h is None else h.size for h in hs])
        buf = (AmPeak * max(1, cap_per_hay * k))()
        counts = (C.c_size_t * max(1, k))()
        _check(lib().am_pool_match_batch(self._p, arr_p, arr_l, k, C.byref(params), buf, cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)

    def match_batch_device(self, ptrs, lengths, params: AmMatchParams, cap_per_hay: int = 256):
        """Resident haystacks: ptrs[k] must live on the device of slot k mod size."""
        k = len(ptrs)
        arr_p = (C.c_void_p * k)(*ptrs)
        arr_l = (C.c_size_t * k)(*lengths)
        buf = (AmPeak * max(1, cap_per_hay * k))()
        counts = (C.c_size_t * max(1, k))()
        _check(lib().am_pool_match_batch_device(self._p, arr_p, arr_l, k, C.byref(params), buf, cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)

    def match_long(self, haystack, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap: int = 4096):
        """ONE long host haystack split over the pool's slots by window ranges (am_pool_match_long)."""
        a = np.ascontiguousarray(haystack, dtype=np.float32 if int(fmt) == Fmt.F32_MONO else np.int16)
        n = a.size if int(fmt) == Fmt.F32_MONO else a.size // 2
        buf = (AmPeak * cap)()
        cnt = C.c_size_t(0)
        _check(lib().am_pool_match_long(self._p, a.ctypes.data, n, int(fmt), C.byref(params), buf, cap, C.byref(cnt)))
        return _peaks(buf, cnt.value)

    def match_long_device(self, part_ptrs, length: int, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap: int = 4096):
        """The same with resident parts: part_ptrs[i] = the samples of part i (long_plan) on slot i's device."""
        arr = (C.c_void_p * len(part_ptrs))(*part_ptrs)
        buf = (AmPeak * cap)()
        cnt = C.c_size_t(0)
        _check(lib().am_pool_match_long_device(self._p, arr, length, int(fmt), C.byref(params), buf, cap, C.byref(cnt)))
        return _peaks(buf, cnt.value)

    def match_batch_pcm16(self, haystacks, params: AmMatchParams, cap_per_hay: int = 256):
        """Host haystacks as interleaved i16 stereo arrays (2 * frames values; None = skipped)."""
        hs = [None if h is None else np.ascontiguousarray(h, dtype=np.int16) for h in haystacks]
        k = len(hs)
        arr_p = (C.c_void_p * k)(*[None if h is None else h.ctypes.data for h in hs])
        arr_l = (C.c_size_t * k)(*[0 if h is None else h.size // 2 for h in hs])
        buf = (AmPeak * max(1, cap_per_hay * k))()
        counts = (C.c_size_t * max(1, k))()
        _check(lib().am_pool_match_batch_pcm16(self._p, arr_p, arr_l, k, C.byref(params), buf, cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)

    def match_batch_pcm16_device(self, ptrs, frames, params: AmMatchParams, cap_per_hay: int = 256):
        k = len(ptrs)
        arr_p = (C.c_void_p * k)(*ptrs)
        arr_l = (C.c_size_t * k)(*frames)
        buf = (AmPeak * max(1, cap_per_hay * k))()
        counts = (C.c_size_t * max(1, k))()
        _check(lib().am_pool_match_batch_pcm16_device(self._p, arr_p, arr_l, k, C.byref(params), buf, cap_per_hay, counts))
        return _split_batch(buf, counts, k, cap_per_hay)

    def close(self):
        if getattr(self, "_p", None):
            lib().am_pool_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _split_pairs(buf, counts, n_hay: int, nn: int, cap: int):
    """[k][j] = peaks of haystack k against needle j (slot k * nn + j)."""
    return [[_peaks_at(buf, (k * nn + j) * cap, counts[k * nn + j]) for j in range(nn)] for k in range(n_hay)]


def match_multi_batch_device(algos, ptrs, lengths, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap_per_pair: int = 64):
    """Several equal-length needles against a batch of resident haystacks (am_match_multi_batch_device):
    result [k][j] = haystack k against needle j."""
    nn, k = len(algos), len(ptrs)
    handles = (C.c_void_p * nn)(*[a._h for a in algos])
    arr_p = (C.c_void_p * k)(*ptrs)
    arr_l = (C.c_size_t * k)(*lengths)
    buf = (AmPeak * max(1, cap_per_pair * k * nn))()
    counts = (C.c_size_t * max(1, k * nn))()
    _check(lib().am_match_multi_batch_device(handles, nn, arr_p, arr_l, k, int(fmt), C.byref(params), buf, cap_per_pair, counts))
    return _split_pairs(buf, counts, k, nn, cap_per_pair)


def _overlaps(overlaps, nn: int):
    if overlaps is None:
        return None
    if len(overlaps) != nn:
        raise ValueError(f"{len(overlaps)} overlaps for {nn} needles")
    return (C.c_uint64 * max(1, nn))(*[int(v) for v in overlaps])


def match_multi_varlen_batch_device(algos, ptrs, lengths, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap_per_pair: int = 64,
                                    overlaps=None):
    """Several needles of any lengths against a batch of resident haystacks (am_match_multi_varlen_batch_device):
    result [k][j] = haystack k against needle j, as am_match_device with overlap overlaps[j] (None: params.overlap)."""
    nn, k = len(algos), len(ptrs)
    handles = (C.c_void_p * max(1, nn))(*[a._h for a in algos])
    arr_p = (C.c_void_p * max(1, k))(*ptrs)
    arr_l = (C.c_size_t * max(1, k))(*lengths)
    buf = (AmPeak * max(1, cap_per_pair * k * nn))()
    counts = (C.c_size_t * max(1, k * nn))()
    _check(lib().am_match_multi_varlen_batch_device(handles, nn, _overlaps(overlaps, nn), arr_p, arr_l, k, int(fmt), C.byref(params),
                                                    buf, cap_per_pair, counts))
    return _split_pairs(buf, counts, k, nn, cap_per_pair)


def match_multi_varlen(algos, haystack, params: AmMatchParams, overlaps=None, cap_per_needle: int = 256):
    """Several needles of any lengths against ONE haystack in host memory (am_match_multi_varlen): a numpy f32 mono
    array, or an interleaved i16 stereo array (int16 dtype, frames x 2 or flat).  Result [j] = the hits of needle j."""
    h, fmt, length = _samples(haystack)
    nn = len(algos)
    handles = (C.c_void_p * max(1, nn))(*[a._h for a in algos])
    buf = (AmPeak * max(1, cap_per_needle * nn))()
    counts = (C.c_size_t * max(1, nn))()
    _check(lib().am_match_multi_varlen(handles, nn, _overlaps(overlaps, nn), h.ctypes.data, length, int(fmt), C.byref(params),
                                       buf, cap_per_needle, counts))
    return [_peaks_at(buf, j * cap_per_needle, counts[j]) for j in range(nn)]


def hit_scores_batch_device(algos, ptrs, lengths, peaks_per_pair, fmt: int = Fmt.F32_MONO):
    """am_hit_scores_batch_device: peaks_per_pair[k][j] = the hits of haystack k against needle j (the shape
    match_multi_batch_device returns; needles may differ in length); result [k][j] = their HitScores."""
    return _hit_batch(_SCORES, algos, ptrs, lengths, peaks_per_pair, fmt, ())


def hit_mask_batch_device(algos, ptrs, lengths, peaks_per_pair, fmt: int = Fmt.F32_MONO):
    """am_hit_mask_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j] = their HitMask records."""
    return _hit_batch(_MASK, algos, ptrs, lengths, peaks_per_pair, fmt, ())


def hit_segments_batch_device(algos, ptrs, lengths, peaks_per_pair, segments: int, radius: int = 4, fmt: int = Fmt.F32_MONO):
    """am_hit_segments_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j][i] = the
    `segments` HitSegment records of hit i of haystack k against needle j."""
    return _hit_batch(_SEGMENTS, algos, ptrs, lengths, peaks_per_pair, fmt, (segments, radius))


def hit_stereo_batch_device(algos, ptrs, lengths, peaks_per_pair, radius: int = 4, fmt: int = Fmt.S16_STEREO):
    """am_hit_stereo_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j] = the HitStereo records
    of haystack k (i16 stereo frames) against needle j."""
    return _hit_batch(_STEREO, algos, ptrs, lengths, peaks_per_pair, fmt, (radius,))


def hit_channel_batch_device(algos, ptrs, lengths, peaks_per_pair, cp: AmChannelParams, fmt: int = Fmt.F32_MONO):
    """am_hit_channel_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j] = (records, taps
    [n, 2P + 1]) of that pair's hits."""
    nn, k = len(algos), len(ptrs)
    pairs = [peaks_per_pair[h][j] for h in range(k) for j in range(nn)]
    cap = max([1] + [len(hits) for hits in pairs])
    handles = (C.c_void_p * max(1, nn))(*[a._h for a in algos])
    arr_p = (C.c_void_p * max(1, k))(*ptrs)
    arr_l = (C.c_size_t * max(1, k))(*lengths)
    buf = (AmPeak * max(1, cap * k * nn))()
    counts = (C.c_size_t * max(1, k * nn))(*[len(hits) for hits in pairs])
    for q, hits in enumerate(pairs):
        for i, p in enumerate(hits):
            buf[q * cap + i] = _am_peak(p)
    out, taps = _channel_call("_batch_device", (handles, nn, arr_p, arr_l, k, int(fmt), buf, cap, counts), cap * k * nn, cp)
    return [[([HitChannel.from_buffer_copy(out[(h * nn + j) * cap + i]) for i in range(counts[h * nn + j])],
              taps[(h * nn + j) * cap:(h * nn + j) * cap + counts[h * nn + j]].copy()) for j in range(nn)] for h in range(k)]


def hit_warp_batch_device(algos, ptrs, lengths, peaks_per_pair, wp: AmWarpParams, fmt: int = Fmt.F32_MONO):
    """am_hit_warp_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j] = the HitWarp records
    of haystack k against needle j."""
    return _hit_batch(_WARP, algos, ptrs, lengths, peaks_per_pair, fmt, (wp,))


def hit_bands_batch_device(algos, ptrs, lengths, peaks_per_pair, bp: AmBandParams, fmt: int = Fmt.F32_MONO):
    """am_hit_bands_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j][i] = the bp.n_bands
    HitBand records of hit i of haystack k against needle j."""
    return _hit_batch(_BANDS, algos, ptrs, lengths, peaks_per_pair, fmt, (bp,))


def hit_significance_batch_device(algos, ptrs, lengths, peaks_per_pair, guard: int, radius: int, fmt: int = Fmt.F32_MONO):
    """am_hit_significance_batch_device: peaks_per_pair[k][j] as in hit_scores_batch_device; result [k][j][i] = the
    HitSignificance of hit i of haystack k against needle j."""
    return _hit_batch(_SIGNIFICANCE, algos, ptrs, lengths, peaks_per_pair, fmt, (guard, radius))


class MultiPool:
    """Several equal-length needles replicated on every listed device (am_pool_create_multi): the file
    loop of matcher::run around N snippets, haystack k on slot k mod n."""

    def __init__(self, samples, devices=None):
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in samples]
        assert arrs and all(a.size == arrs[0].size for a in arrs)
        self._keep = arrs
        self.n_needles = len(arrs)
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        self._p = C.c_void_p()
        if devices is None:
            _check(lib().am_pool_create_multi(ptrs, len(arrs), arrs[0].size, None, 0, C.byref(self._p)))
        else:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().am_pool_create_multi(ptrs, len(arrs), arrs[0].size, arr, len(devices), C.byref(self._p)))
        n = C.c_size_t(0)
        _check(lib().am_pool_size(self._p, C.byref(n)))
        self.size = n.value

    def _run(self, fn, ptrs, lens, fmt, params, cap_per_pair):
        k, nn = len(ptrs), self.n_needles
        arr_p = (C.c_void_p * max(1, k))(*ptrs)
        arr_l = (C.c_size_t * max(1, k))(*lens)
        buf = (AmPeak * max(1, cap_per_pair * k * nn))()
        counts = (C.c_size_t * max(1, k * nn))()
        _check(fn(self._p, arr_p, arr_l, k, int(fmt), C.byref(params), buf, cap_per_pair, counts))
        return _split_pairs(buf, counts, k, nn, cap_per_pair)

    def match_batch(self, haystacks, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap_per_pair: int = 64):
        """Host haystacks: f32 arrays, or interleaved i16 stereo arrays with fmt = Fmt.S16_STEREO."""
        dt = np.float32 if int(fmt) == Fmt.F32_MONO else np.int16
        per = 1 if int(fmt) == Fmt.F32_MONO else 2
        hs = [None if h is None else np.ascontiguousarray(h, dtype=dt) for h in haystacks]
        return self._run(lib().am_pool_match_multi_batch, [None if h is None else h.ctypes.data for h in hs],
                         [0 if h is None else h.size // per for h in hs], fmt, params, cap_per_pair)

    def match_batch_device(self, ptrs, lengths, params: AmMatchParams, fmt: int = Fmt.F32_MONO, cap_per_pair: int = 64):
        return self._run(lib().am_pool_match_multi_batch_device, ptrs, lengths, fmt, params, cap_per_pair)

    def close(self):
        if getattr(self, "_p", None):
            lib().am_pool_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_multi_device(algos, ptr: int, length: int, params: AmMatchParams, cap_per_needle: int = 256):
    """Several equal-length needles against one resident haystack (shared forward pass)."""
    k = len(algos)
    handles = (C.c_void_p * k)(*[a._h for a in algos])
    buf = (AmPeak * (cap_per_needle * k))()
    counts = (C.c_size_t * k)()
    _check(lib().am_match_multi_device(handles, k, ptr, length, C.byref(params), buf, cap_per_needle, counts))
    return [[Peak(int(b.start), int(b.end), float(b.height), float(b.prominence))
             for b in buf[i * cap_per_needle: i * cap_per_needle + counts[i]]] for i in range(k)]


def calc_chunks(sr: int, m_samples, algo_with_sample: HipConvolve, scale: bool, config: Config, ncc: bool = False):
    """audio_matcher.rs:88-141 on the GPU: returns peaks sorted by position.start.

    ncc: window-energy normalised scores for this call (option "score_norm" on the handle, restored afterwards);
    needs scale = True."""
    params = config.params(sr, Scale.LIB if scale else Scale.NONE)
    if not ncc:
        return algo_with_sample.match(m_samples, params)
    keep = algo_with_sample.get_option(OPT_SCORE_NORM)
    algo_with_sample.set_option(OPT_SCORE_NORM, 1)
    try:
        return algo_with_sample.match(m_samples, params)
    finally:
        algo_with_sample.set_option(OPT_SCORE_NORM, keep)


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t)
_progress_keepalive = None


def set_progress_callback(fn):
    """fn(haystack_index, stage, n_chunks): stage 0 = queued, 1 = finished
    (the f1/f2 callbacks of audio_matcher.rs:102-117, 129); None clears it."""
    global _progress_keepalive
    if fn is None:
        _progress_keepalive = None
        _check(lib().am_set_progress_callback(None, None))
        return
    cb = PROGRESS_FN(lambda user, k, stage, n: fn(int(k), int(stage), int(n)))
    _progress_keepalive = cb
    _check(lib().am_set_progress_callback(C.cast(cb, C.c_void_p), None))


CHUNK_PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int)
_chunk_progress_keepalive = None


def set_chunk_progress_callback(fn):
    """fn(haystack_index, chunk_index, n_chunks, stage): the per-chunk f1/f2 callbacks of
    audio_matcher.rs:116-117, 129 (stage 0 = picked up, 1 = done); None clears it."""
    global _chunk_progress_keepalive
    if fn is None:
        _check(lib().am_set_chunk_progress_callback(None, None))
        _chunk_progress_keepalive = None
        return
    cb = CHUNK_PROGRESS_FN(lambda user, k, i, n, stage: fn(int(k), int(i), int(n), int(stage)))
    _check(lib().am_set_chunk_progress_callback(C.cast(cb, C.c_void_p), None))
    _chunk_progress_keepalive = cb


class Profile:
    """HIP-event timing of the pipeline kernels (am_profile_*)."""

    def __init__(self, device: int = 0):
        self.device = device

    def __enter__(self):
        _check(lib().am_profile_reset(self.device))
        _check(lib().am_profile_enable(self.device, 1))
        return self

    def __exit__(self, *exc):
        _check(lib().am_profile_enable(self.device, 0))

    def query(self, kernel: str):
        ms, n = C.c_double(0), C.c_uint64(0)
        _check(lib().am_profile_query(self.device, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
