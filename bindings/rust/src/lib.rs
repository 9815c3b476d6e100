//! Rust binding of the C ABI in `include/audiomatch.h` and the adapter that makes it a
//! third implementor of the reference's `CorrelateAlgo<f32>` (src/matcher/audio_matcher.rs:65-76)
//! next to `LibConvolve` and `MyConvolve`, plus the fast replacement of `calc_chunks`
//! (src/matcher/audio_matcher.rs:88-141).
//!
//! Source only: the build image has no Rust toolchain.

use std::os::raw::{c_char, c_int};
use std::time::Duration;

#[repr(C)]
pub struct AmNeedle {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmPeak {
    pub start: u64,
    pub end: u64,
    pub height: f32,
    pub prominence: f32,
}

#[repr(C)]
pub struct AmMatchParams {
    pub sr: u32,
    pub chunk: u64,
    pub overlap: u64,
    pub min_prominence: f32,
    pub min_distance: u64,
    pub overshadow_distance_s: f64,
    pub scale: c_int,
}

/// am_hit_score: the result of per-hit scoring (24 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmHitScore {
    pub position: f64,
    pub ncc: f32,
    pub gain: f32,
    pub window_db: f32,
    pub flags: u32,
}
/// am_segment_params: per-segment hit scoring (am_hit_segments*)
/// am_estimate_params (needle estimation, 24 bytes): method AM_EST_*, trim_permille 0..500, the margin read in front of
/// each hit and the row length
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEstimateParams {
    pub method: u32,
    pub trim_permille: u32,
    pub lead: u64,
    pub length: u64,
}
/// am_est_hit: one occurrence in a resident haystack (16 bytes); scale = 1 / gain of am_hit_scores
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEstHit {
    pub start: u64,
    pub haystack: u32,
    pub scale: f32,
}
pub const AM_EST_MEAN: u32 = 0;
pub const AM_EST_MEDIAN: u32 = 1;
pub const AM_EST_TRIMMED: u32 = 2;
pub const AM_EST_MAX_HITS: usize = 64;

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmSegmentParams {
    pub segments: u32,
    pub radius: u32,
}
/// am_hit_segment: one segment of one hit (24 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmHitSegment {
    pub lag: f64,
    pub ncc: f32,
    pub gain: f32,
    pub level_db: f32,
    pub flags: u32,
}
/// am_warp_params: per-hit drift scoring (am_hit_warp*), 24 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmWarpParams {
    pub centre_ppm: f64,
    pub max_ppm: f64,
    pub steps: u32,
    pub radius: u32,
}
/// am_warp_hit: one hit's drift, refined lag and corrected NCC (40 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmWarpHit {
    pub drift_ppm: f64,
    pub lag: f64,
    pub ncc: f32,
    pub gain: f32,
    pub level_db: f32,
    pub ncc_centre: f32,
    pub length: u32,
    pub flags: u32,
}
pub const AM_HIT_DRIFT_UNREFINED: u32 = 256;
pub const AM_WARP_PHASES: usize = 4096;
pub const AM_WARP_TAPS: usize = 32;
pub const AM_WARP_MAX_STEPS: u32 = 32;
pub const AM_WARP_MAX_PPM: f64 = 50000.0;
/// am_channel_params: per-hit channel estimation (am_hit_channel*), 16 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmChannelParams {
    pub radius: u32,
    pub reserved: u32,
    pub noise_db: f64,
}
/// am_channel_hit: how well the needle, filtered by the hit's own taps, explains the span (32 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmChannelHit {
    pub ncc: f32,
    pub ncc_eq: f32,
    pub gain_db: f32,
    pub residual_db: f32,
    pub main_tap: i32,
    pub main_share: f32,
    pub flags: u32,
    pub reserved: u32,
}
pub const AM_HIT_ILL_CONDITIONED: u32 = 512;
pub const AM_CHAN_MAX_RADIUS: u32 = 128;
/// am_stereo_params: per-hit stereo image (am_hit_stereo*), 8 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmStereoParams {
    pub radius: u32,
    pub reserved: u32,
}
/// am_stereo_hit: where a hit sits between the channels of a haystack of i16 stereo frames (56 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmStereoHit {
    pub lag_left: f64,
    pub lag_right: f64,
    pub ncc_left: f32,
    pub ncc_right: f32,
    pub ncc_mid: f32,
    pub ncc_side: f32,
    pub ncc_best: f32,
    pub gain_left: f32,
    pub gain_right: f32,
    pub mix_left: f32,
    pub mix_right: f32,
    pub flags: u32,
}
/// am_stereo_summary: image (AM_IMAGE_*), balance, inter-channel delay and what the down-mix cost (32 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmStereoSummary {
    pub balance_db: f64,
    pub delay: f64,
    pub downmix_loss_db: f64,
    pub image: i32,
    pub reserved: u32,
}
pub const AM_HIT_LEFT_SILENT: u32 = 1024;
pub const AM_HIT_RIGHT_SILENT: u32 = 2048;
pub const AM_HIT_SIDE_SILENT: u32 = 4096;
pub const AM_HIT_COLLINEAR: u32 = 8192;
pub const AM_HIT_LEFT_UNREFINED: u32 = 16384;
pub const AM_HIT_RIGHT_UNREFINED: u32 = 32768;
pub const AM_STEREO_MAX_RADIUS: u32 = 16;
pub const AM_STEREO_MIN_INDEPENDENCE: f64 = 1e-6;
pub const AM_IMAGE_ABSENT: i32 = 0;
pub const AM_IMAGE_CENTRE: i32 = 1;
pub const AM_IMAGE_LEFT: i32 = 2;
pub const AM_IMAGE_RIGHT: i32 = 3;
pub const AM_IMAGE_PANNED: i32 = 4;
pub const AM_IMAGE_INVERTED: i32 = 5;
/// am_band_params: per-band hit scoring (am_hit_bands*)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct AmBandParams {
    pub frame_log2: u32,
    pub n_bands: u32,
    pub edges: [u32; AM_BAND_MAX_BANDS + 1],
}
impl Default for AmBandParams {
    fn default() -> Self { AmBandParams { frame_log2: 0, n_bands: 0, edges: [0; AM_BAND_MAX_BANDS + 1] } }
}
/// am_hit_band: one band of one hit (24 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmHitBand {
    pub ncc: f32,
    pub coherence: f32,
    pub gain: f32,
    pub level_db: f32,
    pub needle_share: f32,
    pub flags: u32,
}
/// am_band_summary: how much of the needle's spectrum one hit holds
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmBandSummary {
    pub coverage: f64,
    pub weighted_coherence: f64,
    pub gain_db_spread: f64,
    pub first_present: i32,
    pub last_present: i32,
    pub n_present: u32,
    pub n_countable: u32,
}
pub const AM_HIT_EMPTY_BAND: u32 = 128;
pub const AM_BAND_MAX_BANDS: usize = 32;
pub const AM_BAND_EMPTY_DB: u32 = 90;
/// am_significance_params: per-hit significance (am_hit_significance*)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmSignificanceParams {
    pub guard: u64,
    pub radius: u64,
}
/// am_significance: one hit against its local background (32 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmSignificance {
    pub score: f32,
    pub bg_mean: f32,
    pub bg_std: f32,
    pub z: f32,
    pub side_max: f32,
    pub side_lag: i32,
    pub n_bg: u32,
    pub flags: u32,
}
pub const AM_HIT_NO_BACKGROUND: u32 = 16;
pub const AM_HIT_FLAT_BACKGROUND: u32 = 32;
pub const AM_HIT_CLIPPED: u32 = 64;
pub const AM_SIG_MAX_RADIUS: u64 = 1 << 22;
/// am_segment_summary: coverage, drift and refined start of one hit
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmSegmentSummary {
    pub coverage: f64,
    pub drift_ppm: f64,
    pub start_lag: f64,
    pub residual_rms: f64,
    pub first_present: i32,
    pub last_present: i32,
    pub n_present: u32,
    pub n_usable: u32,
}
/// am_best_params: the k best matches (am_match_best*)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmBestParams {
    pub k: u64,
    pub min_distance: u64,
    pub min_prominence: f32,
    pub scale: c_int,
}
/// am_trace_bin: one bin of a score trace (am_trace_*, am_match_trace*), 40 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmTraceBin {
    pub max: f32,
    pub min: f32,
    pub argmax: u32,
    pub argmin: u32,
    pub count: u32,
    pub reserved: u32,
    pub sum: f64,
    pub sumsq: f64,
}
/// am_trace_params: scores per bin (1 ..= 2^30) and the scale (AM_SCALE_NONE or AM_SCALE_LIB); reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmTraceParams {
    pub bin: u64,
    pub scale: c_int,
    pub reserved: u32,
}
/// am_trace_stats: what am_trace_summary returns
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmTraceStats {
    pub count: u64,
    pub argmax: u64,
    pub argmin: u64,
    pub max: f64,
    pub min: f64,
    pub mean: f64,
    pub std: f64,
    pub median_max: f64,
    pub mad_max: f64,
    pub peak_z: f64,
}
/// am_probe_hit: one probe of a discovery (am_discover*, am_probe_scores*), 40 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmProbeHit {
    pub probe: u64,
    pub best: u64,
    pub second: u64,
    pub ncc: f32,
    pub ncc_second: f32,
    pub flags: u32,
    pub reserved: u32,
}
/// am_edge_params: least overlap (at least 1), the runner-up's least distance (0 = min_overlap), the least share of the
/// needle's energy a candidate lag holds (in [0, 1]); reserved = 0.  24 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEdgeParams {
    pub min_overlap: u64,
    pub separation: u64,
    pub min_share: f32,
    pub reserved: u32,
}
/// am_edge_hit: the record of one edge of a haystack (am_match_edges*), 48 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEdgeHit {
    pub start: i64,
    pub second: i64,
    pub overlap: u64,
    pub ncc: f32,
    pub ncc_second: f32,
    pub gain: f32,
    pub share: f32,
    pub edge: u32,
    pub flags: u32,
}
/// am_discover_params: probe length and hop (at least 1), the exclusion of a self search, the runner-up's least
/// distance (0 = probe_len), the level rule, AM_DISCOVER_SELF; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmDiscoverParams {
    pub probe_len: u64,
    pub hop: u64,
    pub exclude: u64,
    pub separation: u64,
    pub min_level_db: f32,
    pub flags: u32,
    pub reserved: u32,
}
/// am_region_params: the region rule of am_discover_regions; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmRegionParams {
    pub min_ncc: f32,
    pub max_second: f32,
    pub tolerance: u64,
    pub min_good: u32,
    pub max_gap: u32,
    pub flags: u32,
    pub reserved: u32,
}
/// am_region: one region two recordings share, 56 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmRegion {
    pub a_start: u64,
    pub length: u64,
    pub displacement: i64,
    pub first: u64,
    pub count: u32,
    pub good: u32,
    pub mean_ncc: f64,
    pub min_ncc: f32,
    pub worst_second: f32,
}
/// am_env_params: the bands (as for am_hit_bands) and the level floor of envelope matching, 152 bytes; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct AmEnvParams {
    pub bands: AmBandParams,
    pub reserved: u32,
    pub floor_db: f64,
}
/// am_env_grid: the 2 * steps + 1 drifts centre_ppm + max_ppm (q - steps) / steps; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEnvGrid {
    pub centre_ppm: f64,
    pub max_ppm: f64,
    pub steps: u32,
    pub reserved: u32,
}
/// am_env_pick: one place the pick rule keeps, 24 bytes
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEnvPick {
    pub frame: u64,
    pub pos: f64,
    pub score: f32,
    pub q: u32,
}
/// am_env_hit: one occurrence found through its envelope, 32 bytes: start good to a few frames, drift to a grid step or two
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmEnvHit {
    pub start: u64,
    pub length: u64,
    pub drift_ppm: f64,
    pub score: f32,
    pub q: u32,
}
pub const AM_ENV_STEPS_PER_DB: u32 = 8;
pub const AM_ENV_MAX_LEVEL: u16 = 1023;
pub const AM_ENV_ABSENT: u16 = 0xFFFF;
pub const AM_ENV_NO_Q: u32 = 0xFFFF_FFFF;
pub const AM_ENV_MAX_PPM: f64 = 250000.0;
pub const AM_ENV_MAX_FRAMES: u32 = 16384;
pub const AM_ENV_MAX_NEEDLES: u32 = 257;
pub const AM_ENV_MAX_STEPS: u32 = 128;
pub const AM_DISCOVER_SELF: u32 = 1;
pub const AM_REGION_FOLD: u32 = 1;
pub const AM_PROBE_NO_BEST: u32 = 1;
pub const AM_PROBE_NO_SECOND: u32 = 2;
pub const AM_PROBE_NONFINITE: u32 = 4;
pub const AM_PROBE_QUIET: u32 = 8;
pub const AM_DISCOVER_SLICE: u64 = 8192;
pub const AM_EDGE_HEAD: c_int = 0;
pub const AM_EDGE_TAIL: c_int = 1;
pub const AM_EDGE_NO_BEST: u32 = 1;
pub const AM_EDGE_NO_SECOND: u32 = 2;
pub const AM_EDGE_NONFINITE: u32 = 4;
pub const AM_EDGE_BELOW_FLOOR: u32 = 8;
pub const AM_EDGE_TILE: u64 = 4096;
pub const AM_TRACE_WAVE_BIN_MAX: u64 = 2048;
pub const AM_TRACE_SLICE: u64 = 8192;
pub const AM_TRACE_MAX_BIN: u64 = 1 << 30;

pub const AM_HIT_UNREFINED: u32 = 1;
pub const AM_HIT_BELOW_FLOOR: u32 = 2;
pub const AM_HIT_NONFINITE: u32 = 4;

/// am_span: samples [begin, end) of a needle (a gap of a masked needle, am_needle_create_masked)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct AmSpan {
    pub begin: u64,
    pub end: u64,
}
pub const AM_MASK_MAX_GAPS: usize = 15;
/// am_mask_hit: the per-hit record of a masked handle (24 bytes)
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmMaskHit {
    pub ncc: f32,
    pub gain: f32,
    pub kept_db: f32,
    pub ncc_gaps: f32,
    pub gaps_db: f32,
    pub flags: u32,
}
pub const AM_MASK_BELOW_FLOOR: u32 = 1;
pub const AM_MASK_NONFINITE: u32 = 2;
pub const AM_MASK_GAPS_SILENT: u32 = 4;
pub const AM_MASK_GAPS_NONFINITE: u32 = 8;
pub const AM_MASK_NO_GAPS: u32 = 16;

pub const AM_OK: c_int = 0;
pub const AM_ERR_INVALID_ARG: c_int = 1;
pub const AM_ERR_CAPACITY: c_int = 2;

extern "C" {
    pub fn am_last_error_string() -> *const c_char;
    pub fn am_needle_create(device: c_int, needle: *const f32, n: usize, out: *mut *mut AmNeedle) -> c_int;
    pub fn am_needle_create_masked(device: c_int, needle: *const f32, n: usize, gaps: *const AmSpan, n_gaps: usize, out: *mut *mut AmNeedle) -> c_int;
    pub fn am_needle_create_masked_device(device: c_int, d_needle: *const f32, n: usize, gaps: *const AmSpan, n_gaps: usize, out: *mut *mut AmNeedle) -> c_int;
    pub fn am_needle_mask(h: *const AmNeedle, gaps: *mut AmSpan, cap: usize, n_gaps: *mut usize) -> c_int;
    pub fn am_needle_destroy(h: *mut AmNeedle);
    pub fn am_needle_len(h: *const AmNeedle, n: *mut usize) -> c_int;
    pub fn am_needle_inv_autocorr(h: *const AmNeedle, out: *mut f32) -> c_int;
    pub fn am_correlate_len(w: usize, s: usize, mode: c_int, out_len: *mut usize) -> c_int;
    pub fn am_correlate(
        h: *const AmNeedle, within: *const f32, w: usize, mode: c_int, scale: c_int,
        out: *mut f32, cap: usize, out_len: *mut usize,
    ) -> c_int;
    pub fn am_match(
        h: *const AmNeedle, haystack: *const f32, len: usize, p: *const AmMatchParams,
        out: *mut AmPeak, cap: usize, n_out: *mut usize,
    ) -> c_int;
    /// interleaved i16 stereo frames, i.e. what minimp3 yields before the down-mix of
    /// mp3_reader.rs:28-37 (the down-mix then happens inside the first kernel, bit-exact)
    pub fn am_needle_create_pcm16(device: c_int, interleaved: *const i16, frames: usize, out: *mut *mut AmNeedle) -> c_int;
    pub fn am_match_pcm16(
        h: *const AmNeedle, interleaved: *const i16, frames: usize, p: *const AmMatchParams,
        out: *mut AmPeak, cap: usize, n_out: *mut usize,
    ) -> c_int;
    /// haystack k -> shard k mod n_shards (no device needed)
    pub fn am_shard_plan(n_items: usize, n_shards: usize, shard: usize, first: *mut usize, stride: *mut usize, count: *mut usize) -> c_int;
    /// the file loop of matcher::run (matcher/mod.rs:42-87) over every GPU of the node
    pub fn am_pool_create(needle: *const f32, n: usize, devices: *const c_int, n_dev: usize, out: *mut *mut AmPool) -> c_int;
    pub fn am_pool_destroy(pool: *mut AmPool);
    pub fn am_pool_match_batch(
        pool: *mut AmPool, haystacks: *const *const f32, lens: *const usize, n_hay: usize,
        p: *const AmMatchParams, out: *mut AmPeak, cap_per_hay: usize, n_out: *mut usize,
    ) -> c_int;
    /// the same loop on the decoder's interleaved i16 stereo frames (mp3_reader.rs:26-37)
    pub fn am_pool_match_batch_pcm16(
        pool: *mut AmPool, interleaved: *const *const i16, frames: *const usize, n_hay: usize,
        p: *const AmMatchParams, out: *mut AmPeak, cap_per_hay: usize, n_out: *mut usize,
    ) -> c_int;
    /// ONE long haystack over the pool's devices (the window fan-out of audio_matcher.rs:104-131 across GPUs,
    /// one sort + overshadow pass over the union, :132-140); sample_format 0 = f32 mono, 1 = i16 stereo frames
    pub fn am_pool_match_long(
        pool: *mut AmPool, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int,
        p: *const AmMatchParams, out: *mut AmPeak, cap: usize, n_out: *mut usize,
    ) -> c_int;
    /// the pieces of that, for one process per GPU: the split as a pure function, one part (peaks unmerged), the merge
    pub fn am_long_plan(
        len: usize, needle_len: usize, p: *const AmMatchParams, n_parts: usize, part: usize,
        first_window: *mut usize, n_windows: *mut usize, first_sample: *mut usize, n_samples: *mut usize,
    ) -> c_int;
    pub fn am_match_part_device(
        h: *const AmNeedle, d_part: *const std::ffi::c_void, n_samples: usize, sample_format: c_int, p: *const AmMatchParams,
        n_windows: usize, first_sample: u64, out: *mut AmPeak, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_merge_peaks(p: *const AmMatchParams, peaks: *const AmPeak, n: usize, out: *mut AmPeak, cap: usize, n_out: *mut usize) -> c_int;
    /// pinned host memory for the decoder's output (read by the copy engines without a bounce buffer)
    pub fn am_host_alloc(bytes: usize, out: *mut *mut std::ffi::c_void) -> c_int;
    pub fn am_host_free(p: *mut std::ffi::c_void) -> c_int;
    pub fn am_host_register(p: *mut std::ffi::c_void, bytes: usize) -> c_int;
    pub fn am_host_unregister(p: *mut std::ffi::c_void) -> c_int;
    /// several snippets of one length: the haystack's forward transform is shared by a group of needles
    pub fn am_match_multi_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void,
        lens: *const usize, n_hay: usize, sample_format: c_int, p: *const AmMatchParams,
        out: *mut AmPeak, cap_per_pair: usize, n_out: *mut usize,
    ) -> c_int;
    /// several snippets of ANY lengths: one block layout per haystack from the longest, overlaps[j] per needle (null: p.overlap)
    pub fn am_match_multi_varlen_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, overlaps: *const u64, d_haystacks: *const *const std::ffi::c_void,
        lens: *const usize, n_hay: usize, sample_format: c_int, p: *const AmMatchParams,
        out: *mut AmPeak, cap_per_pair: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_multi_varlen(
        needles: *const *const AmNeedle, n_needles: usize, overlaps: *const u64, haystack: *const std::ffi::c_void, len: usize,
        sample_format: c_int, p: *const AmMatchParams, out: *mut AmPeak, cap_per_needle: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_pool_create_multi(
        needles: *const *const f32, n_needles: usize, n: usize, devices: *const c_int, n_dev: usize, out: *mut *mut AmPool,
    ) -> c_int;
    pub fn am_pool_match_multi_batch(
        pool: *mut AmPool, haystacks: *const *const std::ffi::c_void, lens: *const usize, n_hay: usize, sample_format: c_int,
        p: *const AmMatchParams, out: *mut AmPeak, cap_per_pair: usize, n_out: *mut usize,
    ) -> c_int;
    /// sample-rate conversion: scipy.signal.resample_poly(x, L, M) with its default window (audiomatch.h)
    pub fn am_resample_len(n_in: usize, src_rate: u32, dst_rate: u32, n_out: *mut usize) -> c_int;
    pub fn am_resample(
        device: c_int, input: *const std::ffi::c_void, n_in: usize, sample_format: c_int, src_rate: u32, dst_rate: u32,
        out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_resample_device(
        device: c_int, d_in: *const std::ffi::c_void, n_in: usize, sample_format: c_int, src_rate: u32, dst_rate: u32,
        d_out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_needle_create_resampled(
        device: c_int, needle: *const std::ffi::c_void, n: usize, sample_format: c_int, src_rate: u32, dst_rate: u32,
        out: *mut *mut AmNeedle,
    ) -> c_int;
    /// spectral whitening (audiomatch.h): lag products, the prediction-error filter they give, a short FIR filter for
    /// the needle and every haystack it is matched against (the reference has no such stage, audio_matcher.rs:297-343)
    pub fn am_lag_products(
        device: c_int, input: *const std::ffi::c_void, n: usize, sample_format: c_int, order: u32, r: *mut f64,
    ) -> c_int;
    pub fn am_lag_products_device(
        device: c_int, d_in: *const std::ffi::c_void, n: usize, sample_format: c_int, order: u32, r: *mut f64,
    ) -> c_int;
    pub fn am_whiten_taps(r: *const f64, order: u32, noise_db: f64, taps: *mut f32) -> c_int;
    pub fn am_fir(
        device: c_int, input: *const std::ffi::c_void, n_in: usize, sample_format: c_int, taps: *const f32, n_taps: u32,
        lead: usize, out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_fir_device(
        device: c_int, d_in: *const std::ffi::c_void, n_in: usize, sample_format: c_int, taps: *const f32, n_taps: u32,
        lead: usize, d_out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_needle_create_filtered(
        device: c_int, needle: *const std::ffi::c_void, n: usize, sample_format: c_int, taps: *const f32, n_taps: u32,
        out: *mut *mut AmNeedle,
    ) -> c_int;
    /// needle estimation (audiomatch.h): a clean needle from the hits of a rough one -- rows of aligned occurrences, their
    /// per-sample mean, median or trimmed mean, the spread around it (the reference has no such stage, audio_matcher.rs:289)
    pub fn am_hit_window(
        haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, start: u64, scale: f32, lead: u64, length: u64,
        row: *mut f32,
    ) -> c_int;
    pub fn am_needle_estimate_rows(
        device: c_int, rows: *const f32, n: usize, ep: *const AmEstimateParams, est: *mut f32, dev: *mut f32, count: *mut u32,
    ) -> c_int;
    pub fn am_needle_estimate_device(
        device: c_int, d_haystacks: *const *const std::ffi::c_void, lens: *const usize, n_hay: usize, sample_format: c_int,
        hits: *const AmEstHit, n: usize, ep: *const AmEstimateParams, est: *mut f32, dev: *mut f32, count: *mut u32,
    ) -> c_int;
    /// per-hit scoring: exact NCC, gain, window level and sub-sample position of each hit (audiomatch.h)
    pub fn am_hit_scores(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        out: *mut AmHitScore,
    ) -> c_int;
    pub fn am_hit_scores_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        out: *mut AmHitScore,
    ) -> c_int;
    pub fn am_hit_scores_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize, out: *mut AmHitScore,
    ) -> c_int;
    /// the per-hit record of a masked handle (audiomatch.h, "masked needles")
    pub fn am_hit_mask(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        out: *mut AmMaskHit,
    ) -> c_int;
    pub fn am_hit_mask_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        out: *mut AmMaskHit,
    ) -> c_int;
    pub fn am_hit_mask_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize, out: *mut AmMaskHit,
    ) -> c_int;
    /// per-segment hit scoring: which part of the needle a hit holds, and its drift (audiomatch.h)
    pub fn am_hit_segments(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmSegmentParams, out: *mut AmHitSegment,
    ) -> c_int;
    pub fn am_hit_segments_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmSegmentParams, out: *mut AmHitSegment,
    ) -> c_int;
    pub fn am_hit_segments_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        sp: *const AmSegmentParams, out: *mut AmHitSegment,
    ) -> c_int;
    pub fn am_hit_segments_summary(
        seg: *const AmHitSegment, segments: u32, needle_len: usize, min_ncc: f32, out: *mut AmSegmentSummary,
    ) -> c_int;
    /// per-hit drift scoring: a hit's clock drift and its corrected NCC; rows on the needle's clock (audiomatch.h)
    pub fn am_warp_table(out: *mut f32) -> c_int;
    pub fn am_hit_warp(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        wp: *const AmWarpParams, out: *mut AmWarpHit,
    ) -> c_int;
    pub fn am_hit_warp_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        wp: *const AmWarpParams, out: *mut AmWarpHit,
    ) -> c_int;
    pub fn am_hit_warp_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        wp: *const AmWarpParams, out: *mut AmWarpHit,
    ) -> c_int;
    pub fn am_hit_window_warped(
        haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, start: u64, scale: f32, lag: f64, drift_ppm: f64,
        lead: u64, length: u64, row: *mut f32,
    ) -> c_int;
    /// per-hit channel estimation: the filter a hit went through, and what is left of its span (audiomatch.h);
    /// taps: n x (2 radius + 1) f32 in host memory
    pub fn am_hit_channel(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        cp: *const AmChannelParams, out: *mut AmChannelHit, taps: *mut f32,
    ) -> c_int;
    pub fn am_hit_channel_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        cp: *const AmChannelParams, out: *mut AmChannelHit, taps: *mut f32,
    ) -> c_int;
    pub fn am_hit_channel_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        cp: *const AmChannelParams, out: *mut AmChannelHit, taps: *mut f32,
    ) -> c_int;
    /// per-hit stereo image: channel, polarity and delay of a hit (audiomatch.h); AM_FMT_S16_STEREO only
    pub fn am_hit_stereo(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmStereoParams, out: *mut AmStereoHit,
    ) -> c_int;
    pub fn am_hit_stereo_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmStereoParams, out: *mut AmStereoHit,
    ) -> c_int;
    pub fn am_hit_stereo_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        sp: *const AmStereoParams, out: *mut AmStereoHit,
    ) -> c_int;
    pub fn am_hit_stereo_summary(rec: *const AmStereoHit, min_ncc: f32, out: *mut AmStereoSummary) -> c_int;
    /// a stereo mix other than the down-mix: f32((a L + b R) k) of interleaved i16 frames (audiomatch.h)
    pub fn am_pcm_s16_stereo_mix(device: c_int, interleaved: *const i16, frames: usize, a: f32, b: f32, out: *mut f32) -> c_int;
    pub fn am_pcm_s16_stereo_mix_device(device: c_int, d_interleaved: *const i16, frames: usize, a: f32, b: f32, d_out: *mut f32) -> c_int;
    pub fn am_channel_solve(r: *const f64, c: *const f64, radius: u32, noise_db: f64, h: *mut f64, ill: *mut c_int) -> c_int;
    pub fn am_hit_residual(
        haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, start: u64, needle: *const f32, s: usize,
        taps: *const f32, radius: u32, model: *mut f32, resid: *mut f32,
    ) -> c_int;
    /// per-band hit scoring: which frequencies of the needle a hit holds (audiomatch.h)
    pub fn am_hit_bands(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        bp: *const AmBandParams, out: *mut AmHitBand,
    ) -> c_int;
    pub fn am_hit_bands_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        bp: *const AmBandParams, out: *mut AmHitBand,
    ) -> c_int;
    pub fn am_hit_bands_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        bp: *const AmBandParams, out: *mut AmHitBand,
    ) -> c_int;
    pub fn am_hit_bands_summary(rec: *const AmHitBand, n_bands: u32, min_coherence: f32, out: *mut AmBandSummary) -> c_int;
    pub fn am_band_edges_log(sr: u32, frame_log2: u32, lo_hz: f64, hi_hz: f64, n_bands: u32, out: *mut AmBandParams) -> c_int;
    /// per-hit significance: each hit's score against its local background (audiomatch.h)
    pub fn am_hit_significance(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmSignificanceParams, out: *mut AmSignificance,
    ) -> c_int;
    pub fn am_hit_significance_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, peaks: *const AmPeak, n: usize,
        sp: *const AmSignificanceParams, out: *mut AmSignificance,
    ) -> c_int;
    pub fn am_hit_significance_batch_device(
        needles: *const *const AmNeedle, n_needles: usize, d_haystacks: *const *const std::ffi::c_void, lens: *const usize,
        n_hay: usize, sample_format: c_int, peaks: *const AmPeak, cap_per_pair: usize, n_peaks: *const usize,
        sp: *const AmSignificanceParams, out: *mut AmSignificance,
    ) -> c_int;
    /// the k best matches: the first k peaks of find_peaks over the Valid scores, no prominence threshold (audiomatch.h)
    pub fn am_match_best(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, bp: *const AmBestParams,
        out: *mut AmPeak, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_best_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, bp: *const AmBestParams,
        out: *mut AmPeak, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_best_batch_device(
        h: *const AmNeedle, d_haystacks: *const *const std::ffi::c_void, lens: *const usize, n_hay: usize, sample_format: c_int,
        bp: *const AmBestParams, out: *mut AmPeak, n_out: *mut usize,
    ) -> c_int;
    pub fn am_find_peaks_top(
        device: c_int, scores: *const f32, n: usize, min_prominence: f32, min_distance: u64, k: usize, out: *mut AmPeak,
        n_out: *mut usize,
    ) -> c_int;
    pub fn am_find_peaks_top_device(
        device: c_int, d_scores: *const f32, n: usize, min_prominence: f32, min_distance: u64, k: usize, out: *mut AmPeak,
        n_out: *mut usize,
    ) -> c_int;
    /// score traces: per bin of `bin` scores the max, min, their offsets, the count and the f64 sums (audiomatch.h)
    pub fn am_trace_len(n_scores: usize, bin: u64, n_bins: *mut usize) -> c_int;
    pub fn am_trace_scores(
        device: c_int, scores: *const f32, n: usize, bin: u64, out: *mut AmTraceBin, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_trace_scores_device(
        device: c_int, d_scores: *const f32, n: usize, bin: u64, out: *mut AmTraceBin, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_trace(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, tp: *const AmTraceParams,
        out: *mut AmTraceBin, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_trace_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, tp: *const AmTraceParams,
        out: *mut AmTraceBin, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_trace_batch_device(
        h: *const AmNeedle, d_haystacks: *const *const std::ffi::c_void, lens: *const usize, n_hay: usize, sample_format: c_int,
        tp: *const AmTraceParams, out: *mut AmTraceBin, cap_per_hay: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_trace_summary(bins: *const AmTraceBin, n_bins: usize, bin: u64, out: *mut AmTraceStats) -> c_int;
    /// needle discovery: probes of recording A matched against recording B, one record per probe (audiomatch.h)
    pub fn am_discover_len(len_a: usize, dp: *const AmDiscoverParams, n_probes: *mut usize) -> c_int;
    pub fn am_discover_device(
        device: c_int, d_a: *const std::ffi::c_void, len_a: usize, d_b: *const std::ffi::c_void, len_b: usize, sample_format: c_int,
        dp: *const AmDiscoverParams, out: *mut AmProbeHit, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_discover(
        device: c_int, a: *const std::ffi::c_void, len_a: usize, b: *const std::ffi::c_void, len_b: usize, sample_format: c_int,
        dp: *const AmDiscoverParams, out: *mut AmProbeHit, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_probe_scores(
        device: c_int, scores: *const f32, n: usize, ex_lo: u64, ex_hi: u64, separation: u64, out: *mut AmProbeHit,
    ) -> c_int;
    pub fn am_probe_scores_device(
        device: c_int, d_scores: *const f32, n: usize, ex_lo: u64, ex_hi: u64, separation: u64, out: *mut AmProbeHit,
    ) -> c_int;
    pub fn am_discover_regions(
        hits: *const AmProbeHit, n: usize, dp: *const AmDiscoverParams, rp: *const AmRegionParams, out: *mut AmRegion, cap: usize,
        n_out: *mut usize,
    ) -> c_int;
    /// edge matching: a needle cut off by a recording's start or end (audiomatch.h)
    pub fn am_edge_scores_len(len: usize, s: usize, edge: c_int, n_lags: *mut usize, first_lag: *mut i64) -> c_int;
    pub fn am_edge_scores_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, edge: c_int, ep: *const AmEdgeParams,
        out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_edge_scores(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, edge: c_int, ep: *const AmEdgeParams,
        out: *mut f32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_edges_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEdgeParams,
        out: *mut AmEdgeHit,
    ) -> c_int;
    pub fn am_match_edges(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEdgeParams,
        out: *mut AmEdgeHit,
    ) -> c_int;
    pub fn am_match_edges_batch_device(
        h: *const AmNeedle, d_haystacks: *const *const std::ffi::c_void, lens: *const usize, n_hay: usize, sample_format: c_int,
        ep: *const AmEdgeParams, out: *mut AmEdgeHit,
    ) -> c_int;
    /// envelope matching: a needle played at another speed, found through band-level envelopes (audiomatch.h)
    pub fn am_envelope_len(len: usize, ep: *const AmEnvParams, drift_ppm: f64, n_frames: *mut usize) -> c_int;
    pub fn am_envelope(
        device: c_int, signal: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEnvParams, drift_ppm: f64,
        out: *mut u16, cap: usize, n_frames: *mut usize,
    ) -> c_int;
    pub fn am_envelope_device(
        device: c_int, d_signal: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEnvParams, drift_ppm: f64,
        out: *mut u16, cap: usize, n_frames: *mut usize,
    ) -> c_int;
    pub fn am_envelope_scores(
        device: c_int, needles: *const u16, frames: *const u32, n_needles: u32, n_bands: u32, hay: *const u16, hay_frames: usize,
        z: *mut f32, qi: *mut u32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_envelope_scores_device(
        device: c_int, d_needles: *const u16, frames: *const u32, n_needles: u32, n_bands: u32, d_hay: *const u16, hay_frames: usize,
        z: *mut f32, qi: *mut u32, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_envelope_pick(
        z: *const f32, qi: *const u32, n: usize, min_score: f32, separation: u64, out: *mut AmEnvPick, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_envelope(
        h: *const AmNeedle, haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEnvParams,
        grid: *const AmEnvGrid, min_score: f32, out: *mut AmEnvHit, cap: usize, n_out: *mut usize,
    ) -> c_int;
    pub fn am_match_envelope_device(
        h: *const AmNeedle, d_haystack: *const std::ffi::c_void, len: usize, sample_format: c_int, ep: *const AmEnvParams,
        grid: *const AmEnvGrid, min_score: f32, out: *mut AmEnvHit, cap: usize, n_out: *mut usize,
    ) -> c_int;
    /// calc_chunks on the lazy sample iterator (audio_matcher.rs:88-104, mp3_reader.rs:13-41)
    pub fn am_match_stream_begin(
        h: *const AmNeedle, sample_format: c_int, expected_len: usize, p: *const AmMatchParams, out: *mut *mut AmStream,
    ) -> c_int;
    pub fn am_match_stream_push(st: *mut AmStream, samples: *const std::ffi::c_void, n: usize) -> c_int;
    pub fn am_match_stream_finish(st: *mut AmStream, out: *mut AmPeak, cap: usize, n_out: *mut usize) -> c_int;
    pub fn am_match_stream_destroy(st: *mut AmStream);
    /// live monitoring: the finality rule of the overshadow filter (audio_matcher.rs:143-160) and the monitor over an
    /// unbounded sample source (matcher/mod.rs:42-99)
    pub fn am_merge_ready(p: *const AmMatchParams, sorted: *const AmPeak, n: usize, horizon: u64, ended: c_int, n_ready: *mut usize) -> c_int;
    pub fn am_monitor_begin(
        needles: *const *const AmNeedle, n_needles: usize, params: *const AmMatchParams, sample_format: c_int, group_windows: usize,
        out: *mut *mut AmMonitor,
    ) -> c_int;
    pub fn am_monitor_push(m: *mut AmMonitor, samples: *const std::ffi::c_void, n: usize) -> c_int;
    pub fn am_monitor_poll(m: *mut AmMonitor, out: *mut AmPeak, needle: *mut u32, cap: usize, n_out: *mut usize) -> c_int;
    pub fn am_monitor_end(m: *mut AmMonitor, out: *mut AmPeak, needle: *mut u32, cap: usize, n_out: *mut usize) -> c_int;
    pub fn am_monitor_info_get(m: *const AmMonitor, info: *mut AmMonitorInfo) -> c_int;
    pub fn am_monitor_destroy(m: *mut AmMonitor);
}

pub const AM_FMT_F32_MONO: c_int = 0;
pub const AM_FMT_S16_STEREO: c_int = 1;

/// Option keys of window-energy normalised scores (audiomatch.h): "score_norm" (0 = off, 1 = NCC; process default
/// through am_set_option, per handle through am_needle_set_option) and "score_norm_floor_db" (0..200, default 60).
pub const AM_OPT_SCORE_NORM: &str = "score_norm";
pub const AM_OPT_SCORE_NORM_FLOOR_DB: &str = "score_norm_floor_db";

#[repr(C)]
pub struct AmStream {
    _private: [u8; 0],
}

#[repr(C)]
pub struct AmMonitor {
    _private: [u8; 0],
}

/// am_monitor_info
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct AmMonitorInfo {
    pub received: u64,
    pub horizon: u64,
    pub resident_bytes: u64,
    pub pending: u64,
}

#[repr(C)]
pub struct AmPool {
    _private: [u8; 0],
}

/// audio_matcher.rs:55-59
#[derive(Debug, Clone, Copy)]
pub enum Mode {
    Full,
    Same,
    Valid,
}

fn am_err(rc: c_int) -> Box<dyn std::error::Error> {
    let msg = unsafe { std::ffi::CStr::from_ptr(am_last_error_string()) }.to_string_lossy().into_owned();
    format!("audiomatch error {rc}: {msg}").into()
}

/// Drop-in for `LibConvolve` (matcher/mod.rs:34).  In the reference crate this type gets
/// `impl CorrelateAlgo<SampleType> for HipConvolve` with exactly these two methods.
pub struct HipConvolve {
    h: *mut AmNeedle,
    len: usize,
}
unsafe impl Send for HipConvolve {}
unsafe impl Sync for HipConvolve {}

/// How much of the needle's spectrum one hit holds, from its band records (am_hit_bands_summary; no device needed).
pub fn band_summary(rec: &[AmHitBand], min_coherence: f32) -> Result<AmBandSummary, Box<dyn std::error::Error>> {
    let mut out = AmBandSummary::default();
    let rc = unsafe { am_hit_bands_summary(rec.as_ptr(), rec.len() as u32, min_coherence, &mut out) };
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok(out)
}

/// `n_bands` log-spaced bands from `lo_hz` to `hi_hz` for frames of 2^`frame_log2` samples (am_band_edges_log; no device needed).
pub fn band_edges_log(sr: u32, frame_log2: u32, lo_hz: f64, hi_hz: f64, n_bands: u32) -> Result<AmBandParams, Box<dyn std::error::Error>> {
    let mut out = AmBandParams::default();
    let rc = unsafe { am_band_edges_log(sr, frame_log2, lo_hz, hi_hz, n_bands, &mut out) };
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok(out)
}

/// Coverage, drift and refined start of one hit from its segment records (am_hit_segments_summary; no device needed).
pub fn segment_summary(seg: &[AmHitSegment], needle_len: usize, min_ncc: f32) -> Result<AmSegmentSummary, Box<dyn std::error::Error>> {
    let mut out = AmSegmentSummary::default();
    let rc = unsafe { am_hit_segments_summary(seg.as_ptr(), seg.len() as u32, needle_len, min_ncc, &mut out) };
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok(out)
}

/// Image, balance, inter-channel delay and what the down-mix cost, from one hit's record (am_hit_stereo_summary; no device needed).
pub fn stereo_summary(rec: &AmStereoHit, min_ncc: f32) -> Result<AmStereoSummary, Box<dyn std::error::Error>> {
    let mut out = AmStereoSummary::default();
    let rc = unsafe { am_hit_stereo_summary(rec, min_ncc, &mut out) };
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok(out)
}

/// A stereo mix other than the down-mix (am_pcm_s16_stereo_mix): f32((a L + b R) k) of interleaved i16 stereo frames on device 0;
/// (0.5, 0.5) is the down-mix bit for bit, (0.5, -0.5) the side signal.
pub fn pcm_s16_stereo_mix(interleaved: &[i16], a: f32, b: f32) -> Result<Vec<f32>, Box<dyn std::error::Error>> {
    let frames = interleaved.len() / 2;
    let mut out = vec![0f32; frames];
    let rc = unsafe { am_pcm_s16_stereo_mix(0, interleaved.as_ptr(), frames, a, b, out.as_mut_ptr()) };
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok(out)
}

impl HipConvolve {
    /// Per-hit stereo image (am_hit_stereo): where each of `peaks` sits between the channels of a haystack of interleaved
    /// i16 stereo frames -- per channel the best of the lags -radius .. radius, the polarity and the NCC, and the NCC of
    /// the mid, the side and the best fixed mix.
    pub fn hit_stereo(&self, interleaved: &[i16], peaks: &[AmPeak], radius: u32) -> Result<Vec<AmStereoHit>, Box<dyn std::error::Error>> {
        let sp = AmStereoParams { radius, reserved: 0 };
        let mut out = vec![AmStereoHit::default(); peaks.len()];
        let rc = unsafe {
            am_hit_stereo(self.h, interleaved.as_ptr() as *const std::ffi::c_void, interleaved.len() / 2, AM_FMT_S16_STEREO, peaks.as_ptr(),
                          peaks.len(), &sp, out.as_mut_ptr())
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    pub fn new(sample_data: Box<[f32]>) -> Result<Self, Box<dyn std::error::Error>> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe { am_needle_create(0, sample_data.as_ptr(), sample_data.len(), &mut h) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(Self { h, len: sample_data.len() })
    }

    /// `LibConvolve::new` on a snippet with spans to ignore (am_needle_create_masked): with the option "score_norm" the
    /// scores are NCC over the kept samples only.  No gaps: the handle of `new`.
    pub fn new_masked(sample_data: &[f32], gaps: &[AmSpan]) -> Result<Self, Box<dyn std::error::Error>> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe { am_needle_create_masked(0, sample_data.as_ptr(), sample_data.len(), gaps.as_ptr(), gaps.len(), &mut h) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(Self { h, len: sample_data.len() })
    }

    /// The handle's gaps (am_needle_mask); empty for an ordinary handle.
    pub fn mask(&self) -> Result<Vec<AmSpan>, Box<dyn std::error::Error>> {
        let mut gaps = vec![AmSpan::default(); AM_MASK_MAX_GAPS];
        let mut n = 0usize;
        let rc = unsafe { am_needle_mask(self.h, gaps.as_mut_ptr(), gaps.len(), &mut n) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        gaps.truncate(n);
        Ok(gaps)
    }

    /// `LibConvolve::new` on a snippet recorded at `src_rate`, brought to the haystack's `dst_rate` on the GPU
    /// (am_needle_create_resampled): matching then runs on haystacks of that rate, offsets in their samples.  The
    /// reference stops with CliError::SampleRateMismatch instead (matcher/mod.rs:72-74).
    pub fn new_resampled(sample_data: &[f32], src_rate: u32, dst_rate: u32) -> Result<Self, Box<dyn std::error::Error>> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe {
            am_needle_create_resampled(0, sample_data.as_ptr() as *const std::ffi::c_void, sample_data.len(), AM_FMT_F32_MONO,
                                       src_rate, dst_rate, &mut h)
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        let mut len = 0usize;
        let rc = unsafe { am_needle_len(h, &mut len) };
        if rc != AM_OK {
            unsafe { am_needle_destroy(h) };
            return Err(am_err(rc));
        }
        Ok(Self { h, len })
    }

    /// `LibConvolve::new` on a snippet passed through the FIR filter `taps` (am_needle_create_filtered): the whitening
    /// filter designed from the haystacks (am_lag_products, am_whiten_taps) or a pre-emphasis `[1, -alpha]`.  Every
    /// haystack it is matched against must pass through the same taps (am_fir); offsets do not move.
    pub fn new_filtered(sample_data: &[f32], taps: &[f32]) -> Result<Self, Box<dyn std::error::Error>> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe {
            am_needle_create_filtered(0, sample_data.as_ptr() as *const std::ffi::c_void, sample_data.len(), AM_FMT_F32_MONO,
                                      taps.as_ptr(), taps.len() as u32, &mut h)
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(Self { h, len: sample_data.len() })
    }

    /// The same from decoded stereo PCM (`frame.data`, mp3_reader.rs:28): no CPU down-mix pass.
    pub fn from_pcm16(interleaved: &[i16]) -> Result<Self, Box<dyn std::error::Error>> {
        let mut h = std::ptr::null_mut();
        let frames = interleaved.len() / 2;
        let rc = unsafe { am_needle_create_pcm16(0, interleaved.as_ptr(), frames, &mut h) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(Self { h, len: frames })
    }

    /// CorrelateAlgo::inverse_sample_auto_correlation (audio_matcher.rs:66)
    pub fn inverse_sample_auto_correlation(&self) -> f32 {
        let mut v = 0f32;
        unsafe { am_needle_inv_autocorr(self.h, &mut v) };
        v
    }

    /// CorrelateAlgo::correlate_with_sample (audio_matcher.rs:67-72)
    pub fn correlate_with_sample(&self, within: &[f32], mode: Mode, scale: bool) -> Result<Vec<f32>, Box<dyn std::error::Error>> {
        let m = match mode {
            Mode::Full => 0,
            Mode::Same => 1,
            Mode::Valid => 2,
        };
        let mut n = 0usize;
        let rc = unsafe { am_correlate_len(within.len(), self.len, m, &mut n) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        let mut out = vec![0f32; n];
        let rc = unsafe { am_correlate(self.h, within.as_ptr(), within.len(), m, scale as c_int, out.as_mut_ptr(), out.len(), &mut n) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    /// calc_chunks (audio_matcher.rs:88-141) on the GPU: peaks sorted by start, overshadowed ones removed.
    pub fn calc_chunks(&self, sr: u16, m_samples: &[f32], scale: bool, chunk_size: Duration, overlap_length: Duration,
                       distance: Duration, prominence: f32) -> Result<Vec<AmPeak>, Box<dyn std::error::Error>> {
        let p = AmMatchParams {
            sr: sr as u32,
            chunk: (chunk_size.as_secs_f64() * sr as f64).round() as u64,       // :100
            overlap: (overlap_length.as_secs_f64() * sr as f64).round() as u64, // :99
            min_prominence: prominence,                                         // :227
            min_distance: distance.as_secs() * sr as u64,                       // :228
            overshadow_distance_s: distance.as_secs_f64(),                      // :137-138
            scale: scale as c_int,
        };
        let mut buf = vec![AmPeak::default(); 256];
        let mut n = 0usize;
        let mut rc = unsafe { am_match(self.h, m_samples.as_ptr(), m_samples.len(), &p, buf.as_mut_ptr(), buf.len(), &mut n) };
        if rc == AM_ERR_CAPACITY {
            buf.resize(n, AmPeak::default());
            rc = unsafe { am_match(self.h, m_samples.as_ptr(), m_samples.len(), &p, buf.as_mut_ptr(), buf.len(), &mut n) };
        }
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        buf.truncate(n);
        Ok(buf)
    }

    /// The per-hit record of a masked handle (am_hit_mask) for `peaks` found in the host haystack `m_samples`: exact
    /// masked NCC, gain and level over the kept samples, and what the gaps hold against the original needle there.
    pub fn hit_mask(&self, m_samples: &[f32], peaks: &[AmPeak]) -> Result<Vec<AmMaskHit>, Box<dyn std::error::Error>> {
        let mut out = vec![AmMaskHit::default(); peaks.len()];
        let rc = unsafe {
            am_hit_mask(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, peaks.as_ptr(),
                        peaks.len(), out.as_mut_ptr())
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    /// Per-hit scoring (am_hit_scores) of `peaks` found in the host haystack `m_samples`: exact NCC, gain, window
    /// level and sub-sample position, one record per peak.  Only the hits' spans are copied to the device.
    pub fn hit_scores(&self, m_samples: &[f32], peaks: &[AmPeak]) -> Result<Vec<AmHitScore>, Box<dyn std::error::Error>> {
        let mut out = vec![AmHitScore::default(); peaks.len()];
        let rc = unsafe {
            am_hit_scores(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, peaks.as_ptr(),
                          peaks.len(), out.as_mut_ptr())
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    /// Per-segment hit scoring (am_hit_segments) of `peaks` found in the host haystack `m_samples`: `segments` records
    /// per peak (peak i at [i * segments, (i + 1) * segments)), lags -radius ..= radius examined per segment.
    pub fn hit_segments(&self, m_samples: &[f32], peaks: &[AmPeak], segments: u32, radius: u32)
                        -> Result<Vec<AmHitSegment>, Box<dyn std::error::Error>> {
        let sp = AmSegmentParams { segments, radius };
        let mut out = vec![AmHitSegment::default(); peaks.len() * segments as usize];
        let rc = unsafe {
            am_hit_segments(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, peaks.as_ptr(),
                            peaks.len(), &sp, out.as_mut_ptr())
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    /// Per-band hit scoring (am_hit_bands) of `peaks` found in the host haystack `m_samples`: `bp.n_bands` records per
    /// peak (peak i, band b at i * n_bands + b).
    pub fn hit_bands(&self, m_samples: &[f32], peaks: &[AmPeak], bp: &AmBandParams) -> Result<Vec<AmHitBand>, Box<dyn std::error::Error>> {
        let mut out = vec![AmHitBand::default(); peaks.len() * bp.n_bands as usize];
        let rc = unsafe {
            am_hit_bands(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, peaks.as_ptr(),
                         peaks.len(), bp, out.as_mut_ptr())
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(out)
    }

    /// Envelope matching (am_match_envelope): the occurrences of this needle in the host haystack `m_samples` at any speed of
    /// `grid`, found through the band-level envelopes of `bands` (floor 80 dB).  Starts are good to a few frames, drifts to a
    /// grid step or two; a waveform search around a hit refines it.
    pub fn match_envelope(&self, m_samples: &[f32], bands: &AmBandParams, grid: &AmEnvGrid, min_score: f32)
                          -> Result<Vec<AmEnvHit>, Box<dyn std::error::Error>> {
        let ep = AmEnvParams { bands: *bands, reserved: 0, floor_db: 80.0 };
        let mut out = vec![AmEnvHit::default(); 64];
        let mut n = 0usize;
        let call = |out: &mut Vec<AmEnvHit>, n: &mut usize| unsafe {
            am_match_envelope(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, &ep, grid,
                              min_score, out.as_mut_ptr(), out.len(), n)
        };
        let mut rc = call(&mut out, &mut n);
        if rc == AM_ERR_CAPACITY {
            out.resize(n, AmEnvHit::default());
            rc = call(&mut out, &mut n);
        }
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        out.truncate(n);
        Ok(out)
    }

    /// The `k` best matches in the host haystack `m_samples` (am_match_best): the best peaks of its Valid scores by
    /// descending height, at least `min_distance` samples apart, no prominence threshold; LIB scale (NCC when the
    /// handle's "score_norm" is on).  Fewer than `k` when fewer peaks exist.
    pub fn best_matches(&self, m_samples: &[f32], k: usize, min_distance: u64) -> Result<Vec<AmPeak>, Box<dyn std::error::Error>> {
        let bp = AmBestParams { k: k as u64, min_distance, min_prominence: 0.0, scale: 1 };
        let mut out = vec![AmPeak::default(); k.max(1)];
        let mut n = 0usize;
        let rc = unsafe {
            am_match_best(self.h, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, &bp,
                          out.as_mut_ptr(), &mut n)
        };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        out.truncate(n);
        Ok(out)
    }

    /// `calc_chunks` on decoded stereo PCM frames (interleaved i16, as minimp3 delivers them):
    /// same result as down-mixing on the CPU first, one pass less over the haystack.
    pub fn calc_chunks_pcm16(&self, p: &AmMatchParams, interleaved: &[i16]) -> Result<Vec<AmPeak>, Box<dyn std::error::Error>> {
        let frames = interleaved.len() / 2;
        let mut buf = vec![AmPeak::default(); 256];
        let mut n = 0usize;
        let mut rc = unsafe { am_match_pcm16(self.h, interleaved.as_ptr(), frames, p, buf.as_mut_ptr(), buf.len(), &mut n) };
        if rc == AM_ERR_CAPACITY {
            buf.resize(n, AmPeak::default());
            rc = unsafe { am_match_pcm16(self.h, interleaved.as_ptr(), frames, p, buf.as_mut_ptr(), buf.len(), &mut n) };
        }
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        buf.truncate(n);
        Ok(buf)
    }
}

/// `calc_chunks` for SEVERAL snippets of any lengths against one haystack in one pass (am_match_multi_varlen): result
/// [j] is what `needles[j].calc_chunks` returns with overlap `overlaps[j]` (None: `p.overlap` for every snippet).
pub fn calc_chunks_multi(needles: &[&HipConvolve], p: &AmMatchParams, overlaps: Option<&[u64]>, m_samples: &[f32])
                         -> Result<Vec<Vec<AmPeak>>, Box<dyn std::error::Error>> {
    let k = needles.len();
    if let Some(o) = overlaps {
        if o.len() != k {
            return Err(am_err(AM_ERR_INVALID_ARG));
        }
    }
    let hs: Vec<*const AmNeedle> = needles.iter().map(|n| n.h as *const AmNeedle).collect();
    let ov = overlaps.map_or(std::ptr::null(), |o| o.as_ptr());
    let mut cap = 256usize;
    let mut buf = vec![AmPeak::default(); k * cap];
    let mut n = vec![0usize; k];
    let run = |buf: &mut Vec<AmPeak>, n: &mut Vec<usize>, cap: usize| unsafe {
        am_match_multi_varlen(hs.as_ptr(), k, ov, m_samples.as_ptr() as *const std::ffi::c_void, m_samples.len(), AM_FMT_F32_MONO, p,
                              buf.as_mut_ptr(), cap, n.as_mut_ptr())
    };
    let mut rc = run(&mut buf, &mut n, cap);
    if rc == AM_ERR_CAPACITY {
        cap = n.iter().copied().max().unwrap_or(cap).max(cap);
        buf = vec![AmPeak::default(); k * cap];
        rc = run(&mut buf, &mut n, cap);
    }
    if rc != AM_OK {
        return Err(am_err(rc));
    }
    Ok((0..k).map(|j| buf[j * cap..j * cap + n[j]].to_vec()).collect())
}

impl Drop for HipConvolve {
    fn drop(&mut self) {
        unsafe { am_needle_destroy(self.h) }
    }
}

/// The file loop of `matcher::run` (matcher/mod.rs:42-87) over every GPU of the node: the needle
/// replicated per device, haystack `k` matched on device `k mod n` (no exchange step), one submit
/// thread per device inside the library, every result in the slot of its haystack.
pub struct HipConvolvePool {
    p: *mut AmPool,
}
unsafe impl Send for HipConvolvePool {}

impl HipConvolvePool {
    /// `devices = None`: every visible device
    pub fn new(sample_data: &[f32], devices: Option<&[c_int]>) -> Result<Self, Box<dyn std::error::Error>> {
        let mut p = std::ptr::null_mut();
        let (dp, dn) = match devices {
            Some(d) => (d.as_ptr(), d.len()),
            None => (std::ptr::null(), 0),
        };
        let rc = unsafe { am_pool_create(sample_data.as_ptr(), sample_data.len(), dp, dn, &mut p) };
        if rc != AM_OK {
            return Err(am_err(rc));
        }
        Ok(Self { p })
    }

    /// `calc_chunks` for every haystack of the batch; result `k` belongs to `haystacks[k]`
    pub fn calc_chunks(&mut self, p: &AmMatchParams, haystacks: &[&[f32]]) -> Result<Vec<Vec<AmPeak>>, Box<dyn std::error::Error>> {
        let ptrs: Vec<*const f32> = haystacks.iter().map(|h| h.as_ptr()).collect();
        let lens: Vec<usize> = haystacks.iter().map(|h| h.len()).collect();
        let mut cap = 64usize;
        loop {
            let mut buf = vec![AmPeak::default(); cap * haystacks.len().max(1)];
            let mut n = vec![0usize; haystacks.len()];
            let rc = unsafe {
                am_pool_match_batch(self.p, ptrs.as_ptr(), lens.as_ptr(), haystacks.len(), p, buf.as_mut_ptr(), cap, n.as_mut_ptr())
            };
            if rc == AM_ERR_CAPACITY {
                cap = n.iter().copied().max().unwrap_or(cap).max(cap + 1);
                continue;
            }
            if rc != AM_OK {
                return Err(am_err(rc));
            }
            return Ok((0..haystacks.len()).map(|k| buf[k * cap..k * cap + n[k]].to_vec()).collect());
        }
    }

    /// calc_chunks on ONE long recording, its windows split over the pool's devices
    pub fn match_long(&self, haystack: &[f32], p: &AmMatchParams) -> Result<Vec<AmPeak>, Box<dyn std::error::Error>> {
        let mut cap = 4096usize;
        loop {
            let mut buf = vec![AmPeak::default(); cap];
            let mut n = 0usize;
            let rc = unsafe { am_pool_match_long(self.p, haystack.as_ptr().cast(), haystack.len(), 0, p, buf.as_mut_ptr(), cap, &mut n) };
            if rc == AM_ERR_CAPACITY {
                cap = n;
                continue;
            }
            if rc != AM_OK {
                return Err(am_err(rc));
            }
            buf.truncate(n);
            return Ok(buf);
        }
    }
}

impl Drop for HipConvolvePool {
    fn drop(&mut self) {
        unsafe { am_pool_destroy(self.p) }
    }
}

impl HipConvolve {
    /// `calc_chunks` on the reference's own argument shape: a lazy `ExactSizeIterator` of samples
    /// (audio_matcher.rs:88-97).  Blocks of samples are pushed as the iterator yields them; the
    /// transforms of every block pair that has arrived run while the decoder is still producing.
    pub fn calc_chunks_iter<I: ExactSizeIterator<Item = f32>>(&self, p: &AmMatchParams, m_samples: I)
        -> Result<Vec<AmPeak>, Box<dyn std::error::Error>> {
        let mut st = std::ptr::null_mut();
        let rc = unsafe { am_match_stream_begin(self.h, AM_FMT_F32_MONO, m_samples.len(), p, &mut st) };
        if rc != AM_OK { return Err(am_err(rc)); }
        let mut block: Vec<f32> = Vec::with_capacity(1 << 20);
        let mut push = |b: &mut Vec<f32>| -> c_int {
            let rc = unsafe { am_match_stream_push(st, b.as_ptr().cast(), b.len()) };
            b.clear();
            rc
        };
        let mut rc = AM_OK;
        for x in m_samples {
            block.push(x);
            if block.len() == block.capacity() { rc = push(&mut block); if rc != AM_OK { break; } }
        }
        if rc == AM_OK { rc = push(&mut block); }
        let mut buf = vec![AmPeak::default(); 256];
        let mut n = 0usize;
        if rc == AM_OK { rc = unsafe { am_match_stream_finish(st, buf.as_mut_ptr(), buf.len(), &mut n) }; }
        unsafe { am_match_stream_destroy(st) };
        if rc != AM_OK { return Err(am_err(rc)); }
        buf.truncate(n);
        Ok(buf)
    }
}

/// Live monitoring over a sample source that may never end: `LiveHits` pulls samples from `I` in blocks of `block`,
/// pushes them through one monitor and yields `(needle, peak)` as soon as each hit is final (by start, then needle);
/// at the end of `I` it yields the rest.  Each needle's hits, concatenated, equal calc_chunks on the whole recording
/// (offsets exactly, values to f32 rounding), merged as the reference merges (audio_matcher.rs:132-160).
pub struct LiveHits<'a, I: Iterator<Item = f32>> {
    m: *mut AmMonitor,
    src: I,
    block: Vec<f32>,
    ready: std::collections::VecDeque<(u32, AmPeak)>,
    done: bool,
    _needles: std::marker::PhantomData<&'a HipConvolve>,
}

impl<'a, I: Iterator<Item = f32>> LiveHits<'a, I> {
    pub fn new(needles: &[&'a HipConvolve], params: &[AmMatchParams], group_windows: usize, block: usize, src: I)
        -> Result<Self, Box<dyn std::error::Error>> {
        if needles.len() != params.len() { return Err("one AmMatchParams per needle".into()); }
        let hs: Vec<*const AmNeedle> = needles.iter().map(|n| n.h as *const AmNeedle).collect();
        let mut m = std::ptr::null_mut();
        let rc = unsafe { am_monitor_begin(hs.as_ptr(), hs.len(), params.as_ptr(), AM_FMT_F32_MONO, group_windows, &mut m) };
        if rc != AM_OK { return Err(am_err(rc)); }
        Ok(Self { m, src, block: Vec::with_capacity(block.max(1)), ready: Default::default(), done: false,
                  _needles: std::marker::PhantomData })
    }

    pub fn info(&self) -> Result<AmMonitorInfo, Box<dyn std::error::Error>> {
        let mut i = AmMonitorInfo::default();
        let rc = unsafe { am_monitor_info_get(self.m, &mut i) };
        if rc != AM_OK { return Err(am_err(rc)); }
        Ok(i)
    }

    fn take(&mut self, end: bool) -> c_int {
        let mut cap = 64usize;
        loop {
            let mut buf = vec![AmPeak::default(); cap];
            let mut idx = vec![0u32; cap];
            let mut n = 0usize;
            let rc = unsafe {
                if end { am_monitor_end(self.m, buf.as_mut_ptr(), idx.as_mut_ptr(), cap, &mut n) }
                else { am_monitor_poll(self.m, buf.as_mut_ptr(), idx.as_mut_ptr(), cap, &mut n) }
            };
            if rc == AM_ERR_CAPACITY { cap = n; continue; }
            if rc == AM_OK { self.ready.extend(idx[..n].iter().copied().zip(buf[..n].iter().copied())); }
            return rc;
        }
    }
}

impl<'a, I: Iterator<Item = f32>> Iterator for LiveHits<'a, I> {
    type Item = Result<(u32, AmPeak), Box<dyn std::error::Error>>;
    fn next(&mut self) -> Option<Self::Item> {
        loop {
            if let Some(h) = self.ready.pop_front() { return Some(Ok(h)); }
            if self.done { return None; }
            self.block.clear();
            while self.block.len() < self.block.capacity() {
                match self.src.next() { Some(x) => self.block.push(x), None => break }
            }
            let end = self.block.len() < self.block.capacity();
            let mut rc = AM_OK;
            if !self.block.is_empty() { rc = unsafe { am_monitor_push(self.m, self.block.as_ptr().cast(), self.block.len()) }; }
            if rc == AM_OK { rc = self.take(end); }
            if end { self.done = true; }
            if rc != AM_OK { self.done = true; return Some(Err(am_err(rc))); }
        }
    }
}

impl<'a, I: Iterator<Item = f32>> Drop for LiveHits<'a, I> {
    fn drop(&mut self) {
        unsafe { am_monitor_destroy(self.m) }
    }
}
