// libtinyvc_hip.so - the stream stage entries: SOLA, the window push, the gate, the loudness match, the limiter, the suppressor and the
// resampling door.  Each validates on the host and calls its driver; none takes workspace.
#include <cmath>

#include "tvc_common.h"

using namespace tvc;

extern "C" {

int tvc_sola_f32(tvc_ctx* ctx, void* stream, const float* y, float* sola_buf, const float* fade_in, float* out,
                 int32_t* shift_out, int S, int64_t Ly, int block, int use_phase_vocoder) {
    if (!ctx) return TVC_ERR_ARG;
    if (!y || !sola_buf || !fade_in || !out || S <= 0 || block <= 0 || block > kSolaMaxBlock || Ly < (int64_t)block + kSolaCross + kSolaSearch + kSolaDelay)
        return fail(ctx, TVC_ERR_ARG, "tvc_sola_f32: bad argument (Ly must cover block+1920+1920+3840)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_sola(ctx, (hipStream_t)stream, y, sola_buf, fade_in, out, shift_out, S, Ly, block, kSolaCross, kSolaSearch, kSolaDelay, use_phase_vocoder);
}

int tvc_sola_geometry(int block, int cross, int search, int delay, int64_t* min_ly, int* latency_min, int* latency_max) {
    return sola_geometry(block, cross, search, delay, min_ly, latency_min, latency_max, nullptr, 0);
}

const char* tvc_sola_geometry_message(int block, int cross, int search, int delay) {
    static thread_local char why[96];
    sola_geometry(block, cross, search, delay, nullptr, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_sola_geom_f32(tvc_ctx* ctx, void* stream, const float* y, float* sola_buf, const float* fade_in, float* out, int32_t* shift_out, int S,
                      int64_t Ly, int block, int cross, int search, int delay, int use_phase_vocoder) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    int64_t min_ly = 0;
    if (sola_geometry(block, cross, search, delay, &min_ly, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_sola_geom_f32: %s", why);
    if (!y || !sola_buf || !fade_in || !out || S <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_sola_geom_f32: bad argument (a NULL pointer or S <= 0)");
    if (Ly < min_ly)
        return fail(ctx, TVC_ERR_ARG, "tvc_sola_geom_f32: Ly = %ld is shorter than block + cross + search + delay = %ld", (long)Ly, (long)min_ly);
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_sola(ctx, (hipStream_t)stream, y, sola_buf, fade_in, out, shift_out, S, Ly, block, cross, search, delay, use_phase_vocoder);
}

int tvc_stream_push_f32(tvc_ctx* ctx, void* stream, float* buf, const float* blocks, int S, int64_t n, int block) {
    if (!ctx) return TVC_ERR_ARG;
    // (the kernel indexes a row with 32-bit ints and rounds n up to whole 32 768-sample tiles)
    if (!buf || !blocks || S <= 0 || block <= 0 || n < block || n > INT32_MAX - 32768)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_push_f32: bad argument (block <= n <= 2^31 - 32769)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_stream_push(ctx, (hipStream_t)stream, buf, blocks, S, (int)n, block);
}

int tvc_stream_gate_geometry(int block, int sub, int look, int hold, int attack, int release, int* nsub, int* look_samples) {
    return stream_gate_geometry(block, sub, look, hold, attack, release, nsub, look_samples, nullptr, 0);
}

const char* tvc_stream_gate_geometry_message(int block, int sub, int look, int hold, int attack, int release) {
    static thread_local char why[96];
    stream_gate_geometry(block, sub, look, hold, attack, release, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_stream_gate_f32(tvc_ctx* ctx, void* stream, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                        int block, int sub, int look, int hold, int attack, int release, float hysteresis_db, float range_db,
                        const float* threshold_db, int32_t* open, int32_t* hold_state, float* gain, float* level_db) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (stream_gate_geometry(block, sub, look, hold, attack, release, nullptr, nullptr, why, sizeof(why)) != 0)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_gate_f32: %s", why);
    if (!x || !y || !out || !threshold_db || !open || !hold_state || !gain || S <= 0)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_gate_f32: bad argument (a NULL pointer or S <= 0)");
    constexpr int64_t kSpan = (int64_t)1 << 40;      // a + i stays far inside 64 bits for any int32 shift
    if (n < 1 || n > kSpan || base < -kSpan || base > kSpan)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_gate_f32: n = %ld is outside 1 .. 2^40 or |base| = |%ld| is above 2^40", (long)n, (long)base);
    if (!(hysteresis_db >= 0.f) || std::isinf(hysteresis_db))
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_gate_f32: hysteresis_db = %g is not a finite number >= 0", (double)hysteresis_db);
    if (!(range_db <= 0.f)) return fail(ctx, TVC_ERR_ARG, "tvc_stream_gate_f32: range_db = %g is not <= 0 (-inf: a closed gate emits zeros)", (double)range_db);
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    StreamGate g;
    g.block = block; g.sub = sub; g.look = look; g.hold = hold; g.attack = attack; g.release = release;
    g.hysteresis_db = hysteresis_db; g.range_db = range_db;
    g.threshold_db = threshold_db; g.open = open; g.hold_state = hold_state; g.gain = gain; g.level_db = level_db;
    return run_stream_gate(ctx, (hipStream_t)stream, x, n, base, shift, y, out, S, g);
}

int tvc_loudness_geometry(int64_t length, int sub, int smooth, int64_t* nsub, int* window, int* tile) {
    return loudness_geometry(length, sub, smooth, false, nsub, window, tile, nullptr, 0);
}

const char* tvc_loudness_geometry_message(int64_t length, int sub, int smooth) {
    static thread_local char why[96];
    loudness_geometry(length, sub, smooth, false, nullptr, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_stream_loudness_geometry(int block, int sub, int smooth, int* nsub, int* window) {
    int64_t n = 0;
    const int rc = loudness_geometry(block, sub, smooth, true, &n, window, nullptr, nullptr, 0);
    if (rc == 0 && nsub) *nsub = (int)n;
    return rc;
}

const char* tvc_stream_loudness_geometry_message(int block, int sub, int smooth) {
    static thread_local char why[96];
    loudness_geometry(block, sub, smooth, true, nullptr, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_loudness_match_f32(tvc_ctx* ctx, void* stream, const float* x, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* share,
                           int sub, int smooth, float floor_db, float boost_db, float cut_db, float* gains) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (loudness_geometry(L, sub, smooth, false, nullptr, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: %s", why);
    if (!x || !y || !out || !share || B <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: bad argument (a NULL pointer or B <= 0)");
    LoudnessConst c;
    if (loudness_constants(floor_db, boost_db, cut_db, &c, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: %s", why);
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15)
        return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: x, y and out must be 16-byte aligned (the rows are read and written 16 bytes at a time)");
    const int64_t tiles = (L / sub + kLoudnessTile - 1) / kLoudnessTile;
    if (tiles * std::min(B, kLoudnessLenRows) > INT32_MAX) return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: %d rows of %ld tiles are more than 2^31 - 1 workgroups", std::min(B, kLoudnessLenRows), (long)tiles);
    // out is y, or lies apart from it: a workgroup reads its neighbours' sub-frames of y, which a partly overlapping out would be changing.  x likewise
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float), o = (uintptr_t)out;
    auto overlaps = [&](const float* p) { return o < (uintptr_t)p + bytes && (uintptr_t)p < o + bytes; };
    if ((out != y && overlaps(y)) || overlaps(x))
        return fail(ctx, TVC_ERR_ARG, "tvc_loudness_match_f32: out overlaps x, or y without being y");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_loudness_match(ctx, (hipStream_t)stream, x, y, out, B, L, lengths, share, sub, smooth, c, gains);
}

int tvc_stream_loudness_f32(tvc_ctx* ctx, void* stream, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                            int block, int sub, int smooth, float floor_db, float boost_db, float cut_db, const float* share, double* src_ring,
                            double* out_ring, int64_t* frames, float* gain, float* gain_db, float* gains) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (loudness_geometry(block, sub, smooth, true, nullptr, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: %s", why);
    if (!x || !y || !out || !share || !src_ring || !out_ring || !frames || !gain || S <= 0)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: bad argument (a NULL pointer or S <= 0)");
    constexpr int64_t kSpan = (int64_t)1 << 40;      // a + i stays far inside 64 bits for any int32 shift
    if (n < 1 || n > kSpan || base < -kSpan || base > kSpan)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: n = %ld is outside 1 .. 2^40 or |base| = |%ld| is above 2^40", (long)n, (long)base);
    LoudnessConst c;
    if (loudness_constants(floor_db, boost_db, cut_db, &c, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: %s", why);
    if (((uintptr_t)y | (uintptr_t)out) & 15)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: y and out must be 16-byte aligned (the blocks are read and written 16 bytes at a time)");
    // out is y, or lies apart from it; and apart from the windows, which the next block's conversion reads
    const uintptr_t obytes = (uintptr_t)S * (uintptr_t)block * sizeof(float), xbytes = (uintptr_t)S * (uintptr_t)n * sizeof(float), o = (uintptr_t)out;
    if ((out != y && o < (uintptr_t)y + obytes && (uintptr_t)y < o + obytes) || (o < (uintptr_t)x + xbytes && (uintptr_t)x < o + obytes))
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_loudness_f32: out overlaps x, or y without being y");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    StreamLoudness g;
    g.block = block; g.sub = sub; g.smooth = smooth;
    g.share = share; g.src_ring = src_ring; g.out_ring = out_ring; g.frames = frames; g.gain = gain; g.gain_db = gain_db;
    return run_stream_loudness(ctx, (hipStream_t)stream, x, n, base, shift, y, out, S, g, c, gains);
}

int tvc_limiter_geometry(int64_t length, int sub, int release, int64_t* nsub, int* delay, int* tile) {
    return limiter_geometry(length, sub, release, false, nsub, delay, tile, nullptr, 0);
}

const char* tvc_limiter_geometry_message(int64_t length, int sub, int release) {
    static thread_local char why[96];
    limiter_geometry(length, sub, release, false, nullptr, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_stream_limiter_geometry(int block, int sub, int release, int* nsub, int* delay, int* chunk) {
    int64_t n = 0;
    const int rc = limiter_geometry(block, sub, release, true, &n, delay, chunk, nullptr, 0);
    if (rc == 0 && nsub) *nsub = (int)n;
    return rc;
}

const char* tvc_stream_limiter_geometry_message(int block, int sub, int release) {
    static thread_local char why[96];
    limiter_geometry(block, sub, release, true, nullptr, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_limit_f32(tvc_ctx* ctx, void* stream, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* ceiling, int sub, int release,
                  float drive_db, float* gains) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (limiter_geometry(L, sub, release, false, nullptr, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: %s", why);
    if (!y || !out || !ceiling || B <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: bad argument (a NULL pointer or B <= 0)");
    float drive = 1.f;
    if (limiter_drive(drive_db, &drive, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: %s", why);
    if (((uintptr_t)y | (uintptr_t)out) & 15)
        return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: y and out must be 16-byte aligned (the rows are read and written 16 bytes at a time)");
    const int64_t tiles = (L / sub + kLimiterTile - 1) / kLimiterTile;
    if (tiles * std::min(B, kLoudnessLenRows) > INT32_MAX)
        return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: %d rows of %ld tiles are more than 2^31 - 1 workgroups", std::min(B, kLoudnessLenRows), (long)tiles);
    // a workgroup reads the sub-frames of y in its neighbours' tiles, which an overlapping out would be changing: in place is refused too
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float), o = (uintptr_t)out;
    if (o < (uintptr_t)y + bytes && (uintptr_t)y < o + bytes) return fail(ctx, TVC_ERR_ARG, "tvc_limit_f32: out overlaps y (another tile's halo would be read while it is being scaled)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_limit(ctx, (hipStream_t)stream, y, out, B, L, lengths, ceiling, sub, release, drive, gains);
}

int tvc_stream_limit_f32(tvc_ctx* ctx, void* stream, const float* y, float* out, int S, int block, int sub, int release, float drive_db, const float* ceiling,
                         float* tail, float* peak, float* gain, float* reduction_db, float* gains) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (limiter_geometry(block, sub, release, true, nullptr, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_limit_f32: %s", why);
    if (!y || !out || !ceiling || !tail || !peak || !gain || S <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_limit_f32: bad argument (a NULL pointer or S <= 0)");
    float drive = 1.f;
    if (limiter_drive(drive_db, &drive, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_limit_f32: %s", why);
    if (((uintptr_t)y | (uintptr_t)out | (uintptr_t)tail) & 15)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_limit_f32: y, out and tail must be 16-byte aligned (they are read and written 16 bytes at a time)");
    // an output sub-frame is the input sub-frame before it: an overlapping out would change samples that are still to be read
    const uintptr_t bytes = (uintptr_t)S * (uintptr_t)block * sizeof(float), o = (uintptr_t)out;
    if (o < (uintptr_t)y + bytes && (uintptr_t)y < o + bytes) return fail(ctx, TVC_ERR_ARG, "tvc_stream_limit_f32: out overlaps y");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    StreamLimiter g;
    g.block = block; g.sub = sub;
    g.ceiling = ceiling; g.tail = tail; g.peak = peak; g.gain = gain; g.reduction_db = reduction_db;
    return run_stream_limit(ctx, (hipStream_t)stream, y, out, S, g, release, drive, gains);
}

int tvc_stream_denoise_geometry(int block, int hop, int* frames, int* delay) { return stream_denoise_geometry(block, hop, frames, delay, nullptr, 0); }

const char* tvc_stream_denoise_geometry_message(int block, int hop) {
    static thread_local char why[96];
    stream_denoise_geometry(block, hop, nullptr, nullptr, why, sizeof(why));
    return why;
}

int tvc_stream_denoise_f32(tvc_ctx* ctx, void* stream, const float* x, float* out, int S, int block, int hop, float a_s, float a_n, float clamp,
                           float beta, int warm, const float* reduction_db, float* hist, float* ola, float* smooth, float* noise, int32_t* frames,
                           float* noise_db) {
    if (!ctx) return TVC_ERR_ARG;
    char why[96];
    if (stream_denoise_geometry(block, hop, nullptr, nullptr, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: %s", why);
    if (!x || !out || !reduction_db || !hist || !ola || !smooth || !noise || !frames || S <= 0)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: bad argument (a NULL pointer or S <= 0)");
    if (!std::isfinite(a_s) || !std::isfinite(a_n) || !std::isfinite(clamp) || !std::isfinite(beta))
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: a_s = %g, a_n = %g, clamp = %g, beta = %g: not all finite", (double)a_s, (double)a_n, (double)clamp,
                    (double)beta);
    if (a_s < 0.f || a_s >= 1.f || a_n < 0.f || a_n >= 1.f)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: a_s = %g or a_n = %g is outside [0, 1)", (double)a_s, (double)a_n);
    if (clamp < 1.f) return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: clamp = %g is below 1", (double)clamp);
    if (beta < 0.f) return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: beta = %g is negative", (double)beta);
    if (warm < 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_denoise_f32: warm = %d is negative", warm);
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    StreamDenoise d;
    d.block = block; d.hop = hop; d.a_s = a_s; d.a_n = a_n; d.clamp = clamp; d.beta = beta; d.warm = warm;
    d.reduction_db = reduction_db; d.hist = hist; d.ola = ola; d.smooth = smooth; d.noise = noise; d.frames = frames; d.noise_db = noise_db;
    return run_stream_denoise(ctx, (hipStream_t)stream, x, out, S, d);
}

int tvc_stream_resample_geometry(int in_freq, int out_freq, int64_t n_in, int64_t* n_out, int* hist, int* delay) {
    if (!n_out || !hist || !delay) return TVC_ERR_ARG;
    return stream_resample_geometry(in_freq, out_freq, n_in, n_out, hist, delay);
}

int tvc_stream_resample_prepare(tvc_ctx* ctx, int in_freq, int out_freq) {
    if (!ctx) return TVC_ERR_ARG;
    if (in_freq <= 0 || out_freq <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_stream_resample_prepare: rates must be positive");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return stream_resample_prepare(ctx, in_freq, out_freq);
}

int tvc_stream_resample(tvc_ctx* ctx, void* stream, const void* in, int in_is_pcm16, void* out, int out_is_pcm16, float* state, int S, int64_t n_in,
                        int in_freq, int out_freq, float gain_db) {
    if (!ctx) return TVC_ERR_ARG;
    if (!in || !out || S <= 0 || n_in <= 0 || in_freq <= 0 || out_freq <= 0 || (!state && in_freq != out_freq))
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_resample: bad argument (state may be NULL only at equal rates)");
    if (in_is_pcm16 && out_is_pcm16) return fail(ctx, TVC_ERR_ARG, "tvc_stream_resample: one side is fp32 (a door stands between int16 and the model)");
    if (!in_is_pcm16 && !out_is_pcm16 && gain_db != 0.f)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_resample: gain_db belongs to the int16 conversion; fp32 to fp32 takes 0");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_stream_resample(ctx, (hipStream_t)stream, in, in_is_pcm16 != 0, out, out_is_pcm16 != 0, state, S, n_in, in_freq, out_freq, gain_db);
}

}  // extern "C"
