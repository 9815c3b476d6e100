// am_context.hip -- errors, progress hooks and options; device contexts, transform plans and needle spectra;
// the needle handle's life cycle, profiling and am_shutdown.
// Host-side mirror of the reference's driver (paths relative to the reference):
//   calc_chunks            src/matcher/audio_matcher.rs:88-141
//   is_overshadowed        src/matcher/audio_matcher.rs:143-160
//   start_as_duration      src/matcher/mod.rs:127-129
//   Mode crop / centered   src/matcher/audio_matcher.rs:450-464
// All arithmetic on samples runs in the HIP kernels of am_fft.hip /
// am_peaks.hip; there is no CPU fallback.
#include "am_internal.h"

namespace am {

// ---------------------------------------------------------------------------
thread_local std::string t_err;

int fail(int code, const std::string& msg) {
    t_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    t_err = buf;
    return e == hipErrorOutOfMemory ? AM_ERR_OOM : AM_ERR_HIP;
}

// progress hooks (audio_matcher.rs:102-117, 129); a call works on the snapshot it takes on entry
static std::mutex g_hooks_mu;
static Hooks g_hooks;
Hooks snapshot_hooks() {
    std::lock_guard<std::mutex> lk(g_hooks_mu);
    return g_hooks;
}

// ---- options (am_set_option / am_get_option) -------------------------------------------------------------------------
// One row per process-wide option: its name, its value (initially the default), the rule a new value passes (it
// normalises the value, or returns what is wrong with it) and the Opts member snapshot_opts fills from it.  "k2_mfma"
// keeps its switch beside its kernels (am_fft.hip).
using OptRule = const char* (*)(long long& v);
static const char* opt_any(long long&) { return nullptr; }
static const char* opt_bool(long long& v) { v = v ? 1 : 0; return nullptr; }
static const char* opt_log_n(long long& v) { return v != 0 && (v < kLogNMin || v > kLogNMax) ? "log_n out of range" : nullptr; }
static const char* opt_half(long long& v) { v = v <= 0 ? 0 : (v >= 2 ? 2 : 1); return nullptr; }
static const char* opt_every(long long& v) { v = v < 1 ? 1 : v; return nullptr; }
static const char* opt_arm_at(long long& v) { v = v < -1 ? -2 : v; return nullptr; }
static const char* opt_needle_group(long long& v) { return v < 1 || v > kMaxNeedleGroup ? "needle_group out of range" : nullptr; }
static const char* opt_pairs(long long& v) { return v < 1 || v > 64 ? "pairs_per_group out of range" : nullptr; }
static const char* opt_score_norm(long long& v) { return v < 0 || v > 1 ? "score_norm out of range (0 = off, 1 = NCC)" : nullptr; }
static const char* opt_floor_db(long long& v) { return v < 0 || v > 200 ? "score_norm_floor_db out of range (0..200)" : nullptr; }
static const char* opt_trace_form(long long& v) { return v < 0 || v > 2 ? "trace_form out of range (0 = by bin length, 1 = wave form, 2 = sliced form)" : nullptr; }
static const char* opt_distance(long long& v) {
    return v < 0 || v > 3 ? "distance_rule out of range (bit 0: inclusive, bit 1: between plateau starts)" : nullptr;
}
struct Option {
    const char* name;
    std::atomic<long long> value;
    OptRule rule;
    long long Opts::*field;
};
static Option g_options[] = {
    {"log_n", {0}, opt_log_n, &Opts::log_n},                          // 0 = auto
    {"pairs_per_group", {64}, opt_pairs, &Opts::pairs_per_group},
    {"profile_mask", {-1}, opt_any, &Opts::profile_mask},             // bit i = bracket kernel class i with events while profiling is on
    {"profile_every", {1}, opt_every, &Opts::profile_every},          // ... every n-th launch of the class only (an event pair costs the stream about 8 us per kernel boundary)
    {"half_pipeline", {0}, opt_half, &Opts::half},                    // 1 = half-precision storage of the work matrix (config 5)
    {"batch_overlap", {1}, opt_bool, &Opts::batch_overlap},           // 1 = in a batch, pick the peaks of haystack k beside the transforms of k+1
    {"needle_group", {8}, opt_needle_group, &Opts::needle_group},     // needles sharing one forward row transform in am_match_multi_device
    {"pick_stream_priority", {0}, opt_bool, &Opts::pick_priority},    // 1 = the pick's stream is created with the lowest priority (read at context creation)
    {"pick_group", {1}, opt_bool, &Opts::pick_group},                 // 1 = ... and so do the group's picks (0: four small launches per needle, for A/B)
    {"k3_group", {1}, opt_bool, &Opts::k3_group},                     // 1 = the K3s of a needle group run as one launch (0: one launch per needle, for A/B)
    {"host_pick_wait", {1}, opt_bool, &Opts::host_pick_wait},         // 1 = a batch's host thread waits for the pick that last read a score set before it queues the next haystack into it (0: the stream waits)
    {"device_redo", {1}, opt_bool, &Opts::device_redo},               // 0 = failed certificates are redone by the host path only (experiments)
    {"tail_block", {1}, opt_bool, &Opts::tail_block},                 // 1 = a haystack's last, odd block goes through the next smaller plan (TailPlan); 0 = as half of a full pair
    {"dense_scores", {0}, opt_bool, &Opts::dense},                    // 1 = K3 writes every raw score (theta = -inf): the worst case of the sparse-score path
    {"score_norm", {0}, opt_score_norm, &Opts::score_norm},           // 1 = scores normalised by the window energy as well (NCC, am_norm.hip)
    {"score_norm_floor_db", {60}, opt_floor_db, &Opts::score_norm_floor_db},   // ... a window more than this many dB below the needle scores 0
    // test hooks (defaults = production behaviour)
    {"debug_no_realloc", {0}, opt_bool, &Opts::debug_no_realloc},     // 1 = a scratch buffer that would be (re)allocated while a call is queueing fails the call
    {"debug_redo_arm_at", {-2}, opt_arm_at, &Opts::debug_redo_arm_at},   // >= 0: the device-side redo of a batch arms at that haystack; -1: never; -2: when a failure is seen
    {"trace_form", {0}, opt_trace_form, &Opts::trace_form},           // score traces (am_trace.hip): 0 = the form the bin length decides, 1 = one wave per bin, 2 = slices and a finish
    // The semantics nothing available offline pins (the crates find_peaks 0.1 and common are absent, no
    // reference test covers these rules).  Defaults = the documented choices of oracle/oracle.c; every alternative exists
    // in the kernels, on the host AND in the checker, so that one run by someone who has the crates settles each with an
    // option instead of a rewrite (DESIGN.md section 3 lists inputs on which the variants differ).
    {"peak_filter_order", {0}, opt_bool, &Opts::peak_filter_order},   // 0 = prominence, then distance; 1 = distance, then prominence (scipy's order)
    {"distance_rule", {0}, opt_distance, &Opts::distance_rule},       // bit 0: drop at distance <= min_distance (default <); bit 1: between plateau starts (default middles)
    {"tail_window", {0}, opt_bool, &Opts::tail_window},               // 0 = chunked() emits the shorter windows at the end; 1 = only full-length windows
    {"surrounding_from", {0}, opt_bool, &Opts::surrounding_from},     // filter_surrounding's neighbours: 0 = of the sorted, unfiltered sequence; 1 = the neighbour before is the last element kept
};
static Option* find_option(const char* key) {
    for (Option& r : g_options)
        if (!strcmp(key, r.name)) return &r;
    return nullptr;
}

// every option's value now, with the handle's own "log_n" / "half_pipeline" / "score_norm" (>= 0) over the defaults
thread_local const Opts* t_opts_pin = nullptr;
Opts snapshot_opts(const am_needle* h) {
    if (t_opts_pin) return *t_opts_pin;
    Opts o;
    for (const Option& r : g_options) o.*r.field = r.value.load(std::memory_order_relaxed);
    if (h && h->opt_log_n >= 0) o.log_n = h->opt_log_n;
    if (h && h->opt_half >= 0) o.half = h->opt_half;
    if (h && h->opt_score_norm >= 0) o.score_norm = h->opt_score_norm;
    return o;
}

thread_local int t_no_realloc = 0;
int realloc_refused(const char* what, size_t bytes, size_t cap) {
    char buf[160];
    snprintf(buf, sizeof(buf), "debug_no_realloc: %s buffer would grow from %zu to %zu bytes while a call is queueing", what, cap, bytes);
    return fail(AM_ERR_HIP, buf);
}

static const char* kKernelNames[] = {"k1_cols_fwd", "k2_rows", "k3_cols_inv", "tile_stats", "peaks", "other", "trace", "discover",
                                     "envelope_frames", "envelope_prefix", "envelope_correlate", "edges", "mask"};
static std::mutex g_ctx_mu;
static std::map<int, Ctx*> g_ctx;

int get_ctx(int device, Ctx** out) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(AM_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= n) return fail(AM_ERR_NO_DEVICE, "device ordinal out of range");
    auto it = g_ctx.find(device);
    if (it != g_ctx.end()) { *out = it->second; AM_HIP(hipSetDevice(device)); return AM_OK; }
    AM_HIP(hipSetDevice(device));
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);   // may fail if the primary context is already active: harmless
    (void)hipGetLastError();
    AM_HIP(fft_kernels_init());   // function attributes are per device
    Ctx* c = new Ctx();
    c->device = device;
    c->hdr.flags = hipHostMallocMapped | hipHostMallocCoherent;
    c->failcnt.flags = hipHostMallocMapped | hipHostMallocCoherent;
    c->spill.flags = hipHostMallocMapped | hipHostMallocCoherent;
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return hip_fail(se, "hipStreamCreate"); }
    // the pick's stream: small, latency-bound kernels that run beside the next haystack's transforms; at the lowest
    // priority their workgroups fill what the transform kernels leave free instead of competing for dispatch slots
    // (option "pick_stream_priority", read when the context is created: 0 = same priority as the transforms)
    {
        int least = 0, greatest = 0;
        if (snapshot_opts(nullptr).pick_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
            (void)hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, least);
        else
            (void)hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
        (void)hipGetLastError();
    }
    (void)hipStreamCreateWithFlags(&c->stream_tail, hipStreamNonBlocking);
    (void)hipEventCreateWithFlags(&c->ev_fork, kSyncEvent);
    (void)hipEventCreateWithFlags(&c->ev_join, kSyncEvent);
    (void)hipGetLastError();
    for (int i = 0; i < 2; ++i) {
        (void)hipEventCreateWithFlags(&c->ev_k3[i], kSyncEvent);
        (void)hipEventCreateWithFlags(&c->ev_pick[i], kSyncEvent);
    }
    g_ctx[device] = c;
    *out = c;
    return AM_OK;
}

// ---- profiling helpers ------------------------------------------------------
static hipEvent_t prof_event(Ctx* c) {
    if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, AM_EVENT_NO_SYSTEM_FENCE ? hipEventDisableSystemFence : hipEventDefault);   // (timing only: see kSyncEvent)
    return e;
}
ProfScope::ProfScope(Ctx* c_, int name_, hipStream_t st_) : c(c_), name(name_), st(st_ ? st_ : c_->stream) {
    on = c->prof;
    if (on) {
        const Opts o = snapshot_opts(nullptr);
        on = ((o.profile_mask >> name) & 1) && (c->prof_seq[name]++ % (uint64_t)std::max<long long>(1, o.profile_every)) == 0;
    }
    if (on) { e0 = prof_event(c); e1 = prof_event(c); (void)hipEventRecord(e0, st); }
}
static void prof_harvest(Ctx* c) {
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->stream_tail) (void)hipStreamSynchronize(c->stream_tail);
    for (auto& r : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { c->prof_ms[r.name] += ms; c->prof_n[r.name] += 1; }
        c->pool.push_back(r.e0); c->pool.push_back(r.e1);
    }
    c->pending.clear();
}

// ---- copies ------------------------------------------------------------------
// Every copy of the library runs on the context's stream and is waited for there.
// That stream is non-blocking, i.e. not ordered with the null stream a plain
// hipMemcpy uses; a device-to-device hipMemcpy returns before the copy has run and
// a copy from pageable host memory may return once the data is staged, so kernels
// queued on the context's stream right afterwards could otherwise read data that has
// not arrived yet.
hipError_t copy_on_stream(Ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

// ---- the steps the entry points share (contracts: am_internal.h) ----------------
int check_format(int sample_format, const char* who) {
    if (sample_format == AM_FMT_F32_MONO || sample_format == AM_FMT_S16_STEREO) return AM_OK;
    const std::string text = "bad sample format";
    return fail(AM_ERR_INVALID_ARG, who ? std::string(who) + ": " + text + " " + std::to_string(sample_format) : text);
}

int upload_input(Ctx* c, const void* host, size_t bytes, const void** d) {
    int rc = c->io_in.ensure(bytes);
    if (rc) return rc;
    AM_HIP(copy_on_stream(c, c->io_in.p, host, bytes, hipMemcpyHostToDevice));
    *d = c->io_in.p;
    return AM_OK;
}

int download(Ctx* c, void* host, const void* dev, size_t bytes) {
    AM_HIP(copy_on_stream(c, host, dev, bytes, hipMemcpyDeviceToHost));
    return AM_OK;
}

int check_device_arg(const void* p, int device, const char* prefix) {
    const int rc = hit_check_device(p, device, HitWhere{-1, 0, 0, 0});
    return rc ? fail(rc, prefix + t_err) : AM_OK;
}

int resident_input(Ctx* c, bool device_io, const void* p, size_t bytes, const void** d, const char* check_prefix) {
    if (!device_io) return upload_input(c, p, bytes, d);
    *d = p;
    return check_prefix ? check_device_arg(p, c->device, check_prefix) : AM_OK;
}

// ---- plans --------------------------------------------------------------------
static void fill_twiddles(std::vector<float2>& v, size_t off, size_t count, double denom, double mult) {
    for (size_t k = 0; k < count; ++k) {
        const double ang = -2.0 * M_PI * (double)k * mult / denom;
        v[off + k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
}

// Constant tables of k2_rows_m16 (am_fft.hip): the DFT-16 and DFT-32 matrices as operands of
// v_mfma_f32_16x16x32_f16 -- lane (i = lane & 15, g = lane >> 4) holds row i, k = 8g .. 8g+7 with k = 2 p' + {re, im}
// of input point p = 4g + p' (+ 16 ks): [Re F | -Im F] rows give the outputs' real parts, [Im F | Re F] the imaginary
// parts, F[m][p] = W^(m p) -- and every thread's twiddles as h2: T1[gl][e][r] = W_8192^((32 (4w + gl) + 2n + e)(4g + r)),
// T2[ch][r] = W_512^((16 ch + n)(4g + r)) for thread t = 64 w + 16 g + n.  Values are computed in f64 and rounded once.
static void build_mfma_tables(std::vector<unsigned>& tab) {
    tab.assign((size_t)k2_mfma_table_dwords(), 0u);
    auto pack = [](double re, double im) {
        const _Float16 a = (_Float16)re, b = (_Float16)im;
        unsigned short ua, ub;
        memcpy(&ua, &a, 2); memcpy(&ub, &b, 2);
        return (unsigned)ua | ((unsigned)ub << 16);
    };
    // operand element pair (k = 2p', 2p'+1) of row m for input point p: real-part rows (cos, sin), imaginary-part rows (-sin, cos)
    // with F = cos - i sin:  re_out = sum cos x_re + sin x_im,  im_out = sum -sin x_re + cos x_im
    auto operand = [&](size_t base, int m_off, int p_off, double denom) {
        for (int ri = 0; ri < 2; ++ri)
            for (int lane = 0; lane < 64; ++lane)
                for (int pp = 0; pp < 4; ++pp) {
                    const int m = m_off + (lane & 15), pt = p_off + 4 * (lane >> 4) + pp;
                    const double ang = 2.0 * M_PI * (double)((m * pt) % (int)denom) / denom;
                    tab[base + (size_t)ri * 256 + (size_t)lane * 4 + pp] = ri == 0 ? pack(std::cos(ang), std::sin(ang)) : pack(-std::sin(ang), std::cos(ang));
                }
    };
    operand(0, 0, 0, 16.0);                                                   // A16: re rows, im rows
    for (int mb = 0; mb < 2; ++mb)
        for (int ks = 0; ks < 2; ++ks) operand(512 + (size_t)(mb * 2 + ks) * 512, 16 * mb, 16 * ks, 32.0);   // A32[mb][ks][re, im]
    const size_t t1 = 512 + 2048, t2 = t1 + 256 * 32;
    for (int t = 0; t < 256; ++t) {
        const int w = t >> 6, g = (t >> 4) & 3, n = t & 15;
        for (int gl = 0; gl < 4; ++gl)
            for (int e = 0; e < 2; ++e)
                for (int r = 0; r < 4; ++r) {
                    const long long m = ((long long)(32 * (4 * w + gl) + 2 * n + e) * (4 * g + r)) % 8192;
                    const double ang = -2.0 * M_PI * (double)m / 8192.0;
                    tab[t1 + (size_t)t * 32 + gl * 8 + e * 4 + r] = pack(std::cos(ang), std::sin(ang));
                }
        for (int ch = 0; ch < 2; ++ch)
            for (int r = 0; r < 4; ++r) {
                const int m = ((16 * ch + n) * (4 * g + r)) % 512;
                const double ang = -2.0 * M_PI * (double)m / 512.0;
                tab[t2 + (size_t)t * 8 + ch * 4 + r] = pack(std::cos(ang), std::sin(ang));
            }
    }
}

// force_logN1: another factorisation than the production one (am_debug_column_bench: 2^23 as 512 x 16384)
int get_plan(Ctx* c, int logN, const Plan** out, int force_logN1) {
    const int key = force_logN1 ? 1000 * force_logN1 + logN : logN;
    auto it = c->plans.find(key);
    if (it != c->plans.end()) { *out = &it->second; return AM_OK; }
    if (logN < kLogNMin || logN > kLogNMax) return fail(AM_ERR_INVALID_ARG, "unsupported transform size");
    Plan p;
    int logN1 = logN - 13;
    if (logN1 < kColsLog) logN1 = kColsLog;
    if (logN1 > 10) logN1 = 10;
    if (force_logN1) logN1 = force_logN1;
    int logN2 = logN - logN1;
    // N = 2^21 -> 256 x 8192, N = 2^22 -> 512 x 8192, N = 2^23 -> 1024 x 8192: the register kernels
    const int logLo = (logN + 1) / 2;
    const size_t n1h = (size_t)1 << (logN1 - 1), n2h = (size_t)1 << (logN2 - 1);
    const size_t nlo = (size_t)1 << logLo, nhi = (size_t)1 << (logN - logLo);
    // float2 tables, then the float4 ones (see PlanDev): offsets in float2 units, the float4 part 16-byte aligned
    const size_t f2count = (n1h + n2h + nlo + nhi + 1) & ~(size_t)1;
    const size_t nk2j = logN2 == 13 ? 2 * 256 : 0, nk2c = logN2 == 13 ? 2 * 16 : 0;
    std::vector<float2> host(f2count + 2 * (nlo + nhi + nk2j + nk2c));
    fill_twiddles(host, 0, n1h, (double)(1u << logN1), 1.0);
    fill_twiddles(host, n1h, n2h, (double)(1u << logN2), 1.0);
    fill_twiddles(host, n1h + n2h, nlo, (double)((size_t)1 << logN), 1.0);
    fill_twiddles(host, n1h + n2h + nlo, nhi, (double)((size_t)1 << logN), (double)nlo);
    auto tw = [](double num, double denom) {
        const double ang = -2.0 * M_PI * std::fmod(num, denom) / denom;
        return make_float2((float)std::cos(ang), (float)std::sin(ang));
    };
    const double dN = (double)((size_t)1 << logN);
    size_t o = f2count;
    const size_t o_lo4 = o;
    for (size_t k = 0; k < nlo; ++k) { host[o++] = tw((double)k, dN); host[o++] = tw(4.0 * (double)k, dN); }
    const size_t o_hi4 = o;
    for (size_t k = 0; k < nhi; ++k) { host[o++] = tw((double)k * (double)nlo, dN); host[o++] = tw(4.0 * (double)k * (double)nlo, dN); }
    const size_t o_k2j = o;
    for (size_t t = 0; t < nk2j / 2; ++t) {
        host[o++] = tw(2.0 * t, 8192.0); host[o++] = tw(2.0 * t + 1.0, 8192.0);
        host[o++] = tw(8.0 * t, 8192.0); host[o++] = tw(8.0 * t + 4.0, 8192.0);
    }
    const size_t o_k2c = o;
    for (size_t cidx = 0; cidx < nk2c / 2; ++cidx) {
        host[o++] = tw(32.0 * cidx, 8192.0); host[o++] = tw(32.0 * cidx + 16.0, 8192.0);
        host[o++] = tw(128.0 * cidx, 8192.0); host[o++] = tw(128.0 * cidx + 64.0, 8192.0);
    }
    AM_HIP(hipMalloc((void**)&p.tables, host.size() * sizeof(float2)));
    AM_HIP(copy_on_stream(c, p.tables, host.data(), host.size() * sizeof(float2), hipMemcpyHostToDevice));
    p.dev.logN = logN; p.dev.logN1 = logN1; p.dev.logN2 = logN2; p.dev.logLo = logLo;
    p.dev.tw1 = p.tables;
    p.dev.tw2 = p.tables + n1h;
    p.dev.twlo = p.tables + n1h + n2h;
    p.dev.twhi = p.tables + n1h + n2h + nlo;
    p.dev.twlo4 = reinterpret_cast<const float4*>(p.tables + o_lo4);
    p.dev.twhi4 = reinterpret_cast<const float4*>(p.tables + o_hi4);
    p.dev.k2j = nk2j ? reinterpret_cast<const float4*>(p.tables + o_k2j) : nullptr;
    p.dev.k2c = nk2c ? reinterpret_cast<const float4*>(p.tables + o_k2c) : nullptr;
    p.dev.mf = nullptr;
    if (logN2 == 13) {
        std::vector<unsigned> tab;
        build_mfma_tables(tab);
        AM_HIP(hipMalloc((void**)&p.mf, tab.size() * sizeof(unsigned)));
        AM_HIP(copy_on_stream(c, p.mf, tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        p.dev.mf = p.mf;
    }
    auto ins = c->plans.emplace(key, p);
    *out = &ins.first->second;
    return AM_OK;
}

static int needle_spectrum(am_needle* h, const Plan* pl, const float2** out) {
    Ctx* c = h->ctx;
    const int key = pl->dev.logN;
    auto it = h->spectra.find(key);
    if (it != h->spectra.end()) { *out = it->second; return AM_OK; }
    const size_t N = (size_t)1 << pl->dev.logN;
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);   // (a device-side redo may still read the work matrix)
    DevBuf& work = c->side[0].work;
    int rc = work.ensure(std::max<size_t>(N * sizeof(float2), work.cap));
    if (rc) return rc;
    float2* hc = nullptr;
    AM_HIP(hipMalloc((void**)&hc, N * sizeof(float2)));
    Job job{};
    job.src = h->d_needle; job.src_len = (long long)h->n; job.lead = 0;
    job.dst = nullptr; job.out_count = 0; job.hop = 1; job.nblocks = 1; job.first_pair = 0;
    hipError_t e;
    {
        ProfScope ps(c, KN_OTHER);
        e = launch_k1(c->stream, job, 1, (float2*)work.p, pl->dev);
        if (e == hipSuccess) e = launch_k2_spectrum(c->stream, (float2*)work.p, hc, pl->dev);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(hc); return hip_fail(e, "needle spectrum"); }
    h->spectra[key] = hc;
    *out = hc;
    return AM_OK;
}

// half_pipeline = 2: the spectrum as __half2 points times `hscale` (fixed per needle and plan)
static int needle_spectrum16(am_needle* h, const Plan* pl, float hscale, const float2** out) {
    const int key = pl->dev.logN;
    const bool mfma = k2_mfma_enabled() && pl->dev.mf != nullptr && plan_k2_is_r16(pl->dev);   // (the matrix-core row kernel's layout)
    std::map<int, unsigned*>& cache = mfma ? h->spectra16m : h->spectra16;
    auto it = cache.find(key);
    if (it != cache.end()) { *out = reinterpret_cast<const float2*>(it->second); return AM_OK; }
    const float2* hc = nullptr;
    int rc = needle_spectrum(h, pl, &hc);
    if (rc) return rc;
    Ctx* c = h->ctx;
    const size_t N = (size_t)1 << pl->dev.logN;
    unsigned* h16 = nullptr;
    AM_HIP(hipMalloc((void**)&h16, N * sizeof(unsigned)));
    hipError_t e;
    { ProfScope ps(c, KN_OTHER);
      e = mfma ? launch_spectrum_to_half_mfma(c->stream, hc, (long long)N, hscale, h16) : launch_spectrum_to_half(c->stream, hc, (long long)N, hscale, h16); }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(h16); return hip_fail(e, "needle spectrum (f16)"); }
    cache[key] = h16;
    *out = reinterpret_cast<const float2*>(h16);
    return AM_OK;
}
HalfScale half_scale(const am_needle* h, const Opts& o, const PlanDev& pl) {
    HalfScale s{0, 1.0f, 1.0f};
    if (!o.half || !(plan_is_r16(pl) || plan_is_c512(pl))) return s;
    s.level = o.half >= 2 ? 2 : 1;
    if (s.level == 1) s.hscale = kHalfGain * h->inv_autocorr;
    else {
        s.pre = 1.0f / 128.0f;
        s.hscale = (float)((double)(1ull << pl.logN) * std::sqrt((double)h->inv_autocorr) / 8.0);
    }
    return s;
}

// The needle spectrum K2 reads on plan `pl` -- with half_pipeline = 2 the scaled f16 one -- and the plan's HalfScale.
int needle_k2_spectrum(am_needle* h, const Opts& o, const Plan* pl, const float2** hc, HalfScale* hs) {
    int rc = needle_spectrum(h, pl, hc);
    if (rc) return rc;
    *hs = half_scale(h, o, pl->dev);
    return hs->level == 2 ? needle_spectrum16(h, pl, hs->hscale, hc) : AM_OK;
}

int check_needle(const am_needle* h) {
    if (!h || !h->ctx) return fail(AM_ERR_INVALID_ARG, "null needle handle");
    AM_HIP(hipSetDevice(h->ctx->device));
    return AM_OK;
}

int create_needle_common(Ctx* c, float* d_needle, size_t n, am_needle** out) {
    am_needle* h = new am_needle();
    h->ctx = c; h->d_needle = d_needle; h->n = n;
    const int parts = sumsq_parts((long long)n);
    int rc = c->sum.ensure(sizeof(double) * (size_t)parts);
    if (rc) { (void)hipFree(d_needle); delete h; return rc; }
    hipError_t e = launch_sumsq(c->stream, d_needle, (long long)n, (double*)c->sum.p);
    std::vector<double> part((size_t)parts, 0.0);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = copy_on_stream(c, part.data(), c->sum.p, sizeof(double) * (size_t)parts, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { (void)hipFree(d_needle); delete h; return hip_fail(e, "needle energy"); }
    double ss = 0.0;
    for (double v : part) ss += v;
    h->inv_autocorr = (float)(1.0 / ss);   // audio_matcher.rs:321-329
    h->energy = ss;
    *out = h;
    return AM_OK;
}

// ---- masked needles ---------------------------------------------------------------
// the rules of include/audiomatch.h ("masked needles") for the gaps of an n-sample needle; needs no device
static int check_gaps(size_t n, const am_span* gaps, size_t n_gaps) {
    if (n_gaps > 0 && !gaps) return fail(AM_ERR_INVALID_ARG, "null gaps");
    if (n_gaps > AM_MASK_MAX_GAPS)
        return fail(AM_ERR_INVALID_ARG, "masked needle: " + std::to_string(n_gaps) + " gaps, at most " + std::to_string(AM_MASK_MAX_GAPS) + " (AM_MASK_MAX_GAPS)");
    for (size_t i = 0; i < n_gaps; ++i) {
        const std::string who = "masked needle: gap " + std::to_string(i) + " [" + std::to_string(gaps[i].begin) + ", " + std::to_string(gaps[i].end) + "): ";
        if (gaps[i].begin >= gaps[i].end) return fail(AM_ERR_INVALID_ARG, who + "empty or reversed (begin < end required)");
        if (gaps[i].end > n) return fail(AM_ERR_INVALID_ARG, who + "ends behind the needle's " + std::to_string(n) + " samples (end <= n required)");
        if (i > 0 && gaps[i].begin < gaps[i - 1].end) return fail(AM_ERR_INVALID_ARG, who + "begins before gap " + std::to_string(i - 1) + " ends (gaps must ascend)");
        if (i > 0 && gaps[i].begin == gaps[i - 1].end)
            return fail(AM_ERR_INVALID_ARG, who + "touches gap " + std::to_string(i - 1) + " (merge touching gaps: every kept span must be non-empty)");
    }
    if (n_gaps == 1 && gaps[0].begin == 0 && gaps[0].end == n) return fail(AM_ERR_INVALID_ARG, "masked needle: gap 0 covers the whole needle (at least one sample must be kept)");
    if (n_gaps > 0 && (long long)n > kSegmentFrom)
        return fail(AM_ERR_INVALID_ARG, "masked needle: " + std::to_string(n) + " samples is long enough to be partitioned (more than " +
                                            std::to_string(kSegmentFrom) + "); masked partitioned needles are not supported");
    return AM_OK;
}

// The handle over d (n samples, owned from here on, freed if this fails) with the gaps' samples set to +0, the gaps and
// the kept spans' device table.  No gaps: create_needle_common's handle.
static int create_needle_masked(Ctx* c, float* d, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out) {
    std::vector<long long> kept;
    for (size_t i = 0; i <= n_gaps && n_gaps > 0; ++i) {
        const long long a = i == 0 ? 0 : (long long)gaps[i - 1].end, b = i == n_gaps ? (long long)n : (long long)gaps[i].begin;
        if (b > a) { kept.push_back(a); kept.push_back(b); }   // (only the first and the last can be empty: a leading / trailing gap)
    }
    long long* d_kept = nullptr;
    float* d_orig = nullptr;
    hipError_t e = hipSuccess;
    if (n_gaps > 0) e = hipMalloc((void**)&d_orig, sizeof(float) * n);
    if (e == hipSuccess && n_gaps > 0) e = hipMemcpyAsync(d_orig, d, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream);
    for (size_t q = 0; q + 1 < kept.size() && e == hipSuccess; q += 2)
        e = hipMemsetAsync(d_orig + kept[q], 0, sizeof(float) * (size_t)(kept[q + 1] - kept[q]), c->stream);
    for (size_t i = 0; i < n_gaps && e == hipSuccess; ++i)
        e = hipMemsetAsync(d + gaps[i].begin, 0, sizeof(float) * (size_t)(gaps[i].end - gaps[i].begin), c->stream);
    if (e == hipSuccess && n_gaps > 0) e = hipMalloc((void**)&d_kept, sizeof(long long) * kept.size());
    if (e == hipSuccess && n_gaps > 0) e = copy_on_stream(c, d_kept, kept.data(), sizeof(long long) * kept.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        if (d_kept) (void)hipFree(d_kept);
        if (d_orig) (void)hipFree(d_orig);
        return hip_fail(e, "masked needle");
    }
    am_needle* h = nullptr;
    const int rc = create_needle_common(c, d, n, &h);
    if (rc) { if (d_kept) (void)hipFree(d_kept); if (d_orig) (void)hipFree(d_orig); return rc; }
    h->gaps.assign(gaps, gaps + n_gaps);
    h->d_kept = d_kept;
    h->d_gap_orig = d_orig;
    h->n_kept = (int)(kept.size() / 2);
    *out = h;
    return AM_OK;
}

static int needle_create_masked(bool device_io, int device, const float* needle, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out) {
    if (!needle || !out || n == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    int rc = check_gaps(n, gaps, n_gaps);
    if (rc) return rc;
    Ctx* c = nullptr;
    if ((rc = get_ctx(device, &c))) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, n * sizeof(float)));
    const hipError_t e = copy_on_stream(c, d, needle, n * sizeof(float), device_io ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, device_io ? "copy_on_stream(c, needle d2d)" : "copy_on_stream(c, needle)"); }
    return create_needle_masked(c, d, n, gaps, n_gaps, out);
}

}  // namespace am

using namespace am;

extern "C" {

int am_needle_create_masked(int device, const float* needle, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out) {
    return needle_create_masked(false, device, needle, n, gaps, n_gaps, out);
}

int am_needle_create_masked_device(int device, const float* d_needle, size_t n, const am_span* gaps, size_t n_gaps, am_needle** out) {
    return needle_create_masked(true, device, d_needle, n, gaps, n_gaps, out);
}

int am_needle_mask(const am_needle* h, am_span* gaps, size_t cap, size_t* n_gaps) {
    if (!h || !h->ctx) return fail(AM_ERR_INVALID_ARG, "null needle handle");
    if (!n_gaps || (cap > 0 && !gaps)) return fail(AM_ERR_INVALID_ARG, "null pointer");
    return hand_back(h->gaps, gaps, cap, n_gaps, "am_needle_mask: more gaps than cap");
}

int am_needle_create(int device, const float* needle, size_t n, am_needle** out) {
    if (!needle || !out || n == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, n * sizeof(float)));
    hipError_t e = copy_on_stream(c, d, needle, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "copy_on_stream(c, needle)"); }
    return create_needle_common(c, d, n, out);
}

int am_needle_create_device(int device, const float* d_needle, size_t n, am_needle** out) {
    if (!d_needle || !out || n == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, n * sizeof(float)));
    hipError_t e = copy_on_stream(c, d, d_needle, n * sizeof(float), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "copy_on_stream(c, needle d2d)"); }
    return create_needle_common(c, d, n, out);
}

void am_needle_destroy(am_needle* h) {
    if (!h) return;
    if (h->ctx) {
        std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        auto free_spectra = [](am_needle* x) {
            for (auto& kv : x->spectra) (void)hipFree(kv.second);
            for (auto* m : {&x->spectra16, &x->spectra16m})
                for (auto& kv : *m) (void)hipFree(kv.second);
        };
        for (am_needle* sub : h->segments) { free_spectra(sub); delete sub; }
        free_spectra(h);
        if (h->d_edge_scans) (void)hipFree(h->d_edge_scans);
        if (h->d_kept) (void)hipFree(h->d_kept);
        if (h->d_gap_orig) (void)hipFree(h->d_gap_orig);
        if (h->d_needle && h->owns_data) (void)hipFree(h->d_needle);
    }
    delete h;
}

int am_needle_len(const am_needle* h, size_t* n) {
    if (!h || !n) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *n = h->n;
    return AM_OK;
}

int am_needle_inv_autocorr(const am_needle* h, float* out) {
    if (!h || !out) return fail(AM_ERR_INVALID_ARG, "null pointer");
    *out = h->inv_autocorr;
    return AM_OK;
}

int am_needle_create_pcm16(int device, const int16_t* interleaved, size_t frames, am_needle** out) {
    if (!interleaved || !out || frames == 0) return fail(AM_ERR_INVALID_ARG, "needle must be non-empty");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const void* d_in = nullptr;
    if ((rc = upload_input(c, interleaved, sample_bytes(frames), &d_in))) return rc;
    float* d = nullptr;
    AM_HIP(hipMalloc((void**)&d, frames * sizeof(float)));
    hipError_t e = launch_pcm_downmix(c->stream, (const int16_t*)d_in, (long long)frames, d);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "needle down-mix"); }
    return create_needle_common(c, d, frames, out);
}

int am_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (auto& kv : g_ctx) {
        Ctx* c = kv.second;
        std::lock_guard<std::recursive_mutex> lk2(c->mu);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->stream2) (void)hipStreamSynchronize(c->stream2);
        if (c->stream_tail) (void)hipStreamSynchronize(c->stream_tail);
        for (ScoreSide& sd : c->side)
            for (DevBuf* b : {&sd.scores, &sd.stats, &sd.stats32, &sd.wflags, &sd.peaks, &sd.work}) b->release();
        for (DevBuf* b : {&c->work2, &c->segs, &c->redo_pairs[0], &c->redo_pairs[1],
                          &c->io_in, &c->io_out, &c->sum, &c->arena_cur, &c->wide_ctl, &c->wide_list, &c->wide_tiles})
            b->release();
        for (HostBuf* b : {&c->pinned, &c->hdr, &c->spill, &c->badflag, &c->failcnt}) b->release();
        c->ranges.release(); c->range_flags.release(); c->big.release(); c->norm_blk.release();
        for (DevBuf* b : {&c->hit_tab, &c->hit_parts, &c->hit_flags, &c->hit_out, &c->hit_stage}) b->release();
        c->hit_io.release();
        for (DevBuf* b : {&c->sig_span, &c->sig_scores, &c->sig_psum, &c->sig_pmax, &c->sig_mean, &c->sig_hmax}) b->release();
        for (DevBuf* b : {&c->best_stats, &c->best_lmax, &c->best_ctl, &c->best_trans, &c->best_list, &c->best_scores, &c->best_mono, &c->trace_out, &c->trace_parts}) b->release();
        for (DevBuf* b : {&c->disc_a, &c->disc_probe, &c->disc_energy, &c->disc_parts, &c->disc_out}) b->release();
        for (DevBuf* b : {&c->env_jobs, &c->env_needles, &c->env_hay, &c->env_bank, &c->env_desc, &c->env_prefix, &c->env_blocks, &c->env_out}) b->release();
        for (auto& kv : c->rs_taps) kv.second.release();
        c->rs_taps.clear();
        c->lag_parts.release(); c->lag_r.release();
        for (auto& kv : c->band_tabs) kv.second.release();
        c->band_tabs.clear();
        c->warp_tab.release(); c->warp_needles.release();
        c->work_tail.release(); c->tail_scores.release(); c->tail_stats.release(); c->work_tail2.release();
        for (int set = 0; set < 2; ++set)
            for (int i = 0; i < kMaxNeedleGroup; ++i) { c->grp_scores[set][i].release(); c->grp_stats32[set][i].release(); c->grp_wflags[set][i].release(); }
        for (int i = 0; i < kMaxNeedleGroup; ++i) c->grp_stats[i].release();
        c->segs_resident.clear();
        for (auto& pk : c->plans) { if (pk.second.tables) (void)hipFree(pk.second.tables); if (pk.second.mf) (void)hipFree(pk.second.mf); }
        c->plans.clear();
        for (auto& r : c->pending) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        c->pending.clear();
        for (hipEvent_t e : c->pool) (void)hipEventDestroy(e);
        c->pool.clear();
    }
    return AM_OK;
}

int am_set_progress_callback(am_progress_fn fn, void* user) {
    std::lock_guard<std::mutex> lk(g_hooks_mu);
    g_hooks.fn = fn;
    g_hooks.user = user;
    return AM_OK;
}

int am_set_chunk_progress_callback(am_chunk_progress_fn fn, void* user) {
    std::lock_guard<std::mutex> lk(g_hooks_mu);
    g_hooks.chunk_fn = fn;
    g_hooks.chunk_user = user;
    return AM_OK;
}

int am_profile_enable(int device, int on) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    prof_harvest(c);
    c->prof = on != 0;
    return AM_OK;
}
int am_profile_reset(int device) {
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    prof_harvest(c);
    for (int i = 0; i < KN_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
    return AM_OK;
}
int am_profile_query(int device, const char* kernel, double* total_ms, uint64_t* launches) {
    if (!kernel || !total_ms || !launches) return fail(AM_ERR_INVALID_ARG, "null pointer");
    Ctx* c = nullptr;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    prof_harvest(c);
    double ms = 0; uint64_t n = 0; bool found = false;
    for (int i = 0; i < KN_COUNT; ++i) {
        // ("envelope": the three classes of envelope matching together)
        const bool family = !strcmp(kernel, "envelope") && !strncmp(kKernelNames[i], "envelope_", 9);
        if (!strcmp(kernel, "*") || !strcmp(kernel, kKernelNames[i]) || family) { ms += c->prof_ms[i]; n += c->prof_n[i]; found = true; }
    }
    if (!found) return fail(AM_ERR_INVALID_ARG, "unknown kernel name");
    *total_ms = ms; *launches = n;
    return AM_OK;
}

int am_set_option(const char* key, long long value) {
    if (!key) return fail(AM_ERR_INVALID_ARG, "null key");
    if (!strcmp(key, "k2_mfma")) { set_k2_mfma(value != 0); return AM_OK; }
    Option* r = find_option(key);
    if (!r) return fail(AM_ERR_INVALID_ARG, "unknown option");
    if (const char* err = r->rule(value)) return fail(AM_ERR_INVALID_ARG, err);
    r->value = value;
    return AM_OK;
}
int am_get_option(const char* key, long long* value) {
    if (!key || !value) return fail(AM_ERR_INVALID_ARG, "null pointer");
    if (!strcmp(key, "k2_mfma")) { *value = k2_mfma_enabled() ? 1 : 0; return AM_OK; }
    const Option* r = find_option(key);
    if (!r) return fail(AM_ERR_INVALID_ARG, "unknown option");
    *value = r->value.load();
    return AM_OK;
}

int am_needle_set_option(am_needle* h, const char* key, long long value) {
    if (!h || !h->ctx || !key) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    if (!strcmp(key, "log_n")) {
        if (value > 0 && (value < kLogNMin || value > kLogNMax)) return fail(AM_ERR_INVALID_ARG, "log_n out of range");
        h->opt_log_n = value < 0 ? -1 : value; return AM_OK;
    }
    if (!strcmp(key, "half_pipeline")) { h->opt_half = value < 0 ? -1 : (value >= 2 ? 2 : (value ? 1 : 0)); return AM_OK; }
    if (!strcmp(key, "score_norm")) {
        if (value > 1) return fail(AM_ERR_INVALID_ARG, "score_norm out of range (-1 = default, 0 = off, 1 = NCC)");
        h->opt_score_norm = value < 0 ? -1 : value; return AM_OK;
    }
    return fail(AM_ERR_INVALID_ARG, "unknown per-handle option (log_n, half_pipeline, score_norm)");
}
int am_needle_get_option(const am_needle* h, const char* key, long long* value) {
    if (!h || !h->ctx || !key || !value) return fail(AM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::recursive_mutex> lk(h->ctx->mu);
    if (!strcmp(key, "log_n")) { *value = h->opt_log_n; return AM_OK; }
    if (!strcmp(key, "half_pipeline")) { *value = h->opt_half; return AM_OK; }
    if (!strcmp(key, "score_norm")) { *value = h->opt_score_norm; return AM_OK; }
    return fail(AM_ERR_INVALID_ARG, "unknown per-handle option (log_n, half_pipeline, score_norm)");
}

}  // extern "C"
