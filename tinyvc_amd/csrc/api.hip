// libtinyvc_hip.so — the extern "C" surface: context, prepared-blob registry, weights, the single-stage entries, the ragged plan and encode,
// index compaction and the profiler.  An entry validates, describes its call and hands it to run_walks (api.h).  The conversion entries:
// api_convert.hip; the stream stages: api_stream.hip.  No kernel lives here - checkpoint packing: pack.hip, the ragged batch planner and its
// loops: ragged.hip.
#include <atomic>
#include <cmath>
#include <mutex>

#include <cstdlib>

#include "api.h"
#include "knn_blob.h"

using namespace tvc;

// Prepared kNN blobs of this process: device pointer -> N it was prepared for.  The kernels take the blob's geometry (offsets of the
// inverse norms and the fp16 image) from the caller's N, so a call whose N differs from the one the blob was prepared with would read
// out of bounds: such a call is refused.  (A blob this process did not prepare - e.g. a copy - is unknown here and trusted.)
// The record is made only after the prepare launches succeeded; tvc_knn_forget drops it when the memory is handed to something else
// (a device address is recycled: a blob copied to where a blob of another size once lived must not inherit that record), and the
// registry is bounded: past kMaxBlobRecords it starts over (a forgotten record only loses this check).
static std::mutex g_blob_mu;
static std::map<const void*, int64_t> g_blobs;
constexpr size_t kMaxBlobRecords = 4096;
static void blob_record(const void* p, int64_t N) {
    std::lock_guard<std::mutex> lk(g_blob_mu);
    if (g_blobs.size() >= kMaxBlobRecords && !g_blobs.count(p)) g_blobs.clear();
    g_blobs[p] = N;
}
static void blob_forget(const void* p) {
    std::lock_guard<std::mutex> lk(g_blob_mu);
    g_blobs.erase(p);
}
// A blob this process did not prepare (a copy, a blob loaded from a file) is read ONCE - its 24-byte header, after the caller's stream has drained -
// and must carry this build's magic, format version and the caller's N; then it is recorded like a prepared one.  Inside a stream capture nothing
// may synchronise: an unknown blob is trusted there (capture after one eager call, as the module path does).
int tvc::blob_check(tvc_ctx* ctx, hipStream_t s, const void* p, int64_t N, const char* what) {
    {
        std::lock_guard<std::mutex> lk(g_blob_mu);
        auto it = g_blobs.find(p);
        if (it != g_blobs.end()) {
            if (it->second != N)
                return fail(ctx, TVC_ERR_ARG, "%s: this blob was prepared for N = %lld index vectors, the call says N = %lld", what, (long long)it->second, (long long)N);
            return 0;
        }
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return 0;
    int h[BLOB_WORDS] = {};
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h, p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ctx, TVC_ERR_HIP, "%s: cannot read the prepared index's header", what);
    const int64_t n = ((int64_t)(unsigned)h[BLOB_W_N_HI] << 32) | (unsigned)h[BLOB_W_N_LO];
    if (h[BLOB_W_MAGIC] != BLOB_MAGIC || (h[BLOB_W_KIND] != KIND_F32 && h[BLOB_W_KIND] != KIND_F16))
        return fail(ctx, TVC_ERR_ARG, "%s: `prepared` is not a blob of tvc_knn_prepare_index_f32 / _f16", what);
    if (h[BLOB_W_VERSION] != tvc::kBlobVersion)
        return fail(ctx, TVC_ERR_ARG, "%s: the prepared index has format version %d, this library writes and reads version %d: prepare it again", what, h[BLOB_W_VERSION], tvc::kBlobVersion);
    if (n != N) return fail(ctx, TVC_ERR_ARG, "%s: this blob was prepared for N = %lld index vectors, the call says N = %lld", what, (long long)n, (long long)N);
    blob_record(p, N);
    return 0;
}

// noise_angle = NULL makes the library draw the phases from `seed` - a kernel ARGUMENT, which a stream capture bakes into the graph: every replay
// would synthesise the same noise.  A capturing caller must pass the phases (a buffer it refills between replays, as the module path does).
int tvc::draw_under_capture(tvc_ctx* ctx, hipStream_t s, const float* noise_angle, const char* what) {
    if (noise_angle) return 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(ctx, TVC_ERR_STATE, "%s: noise_angle = NULL inside a stream capture would replay ONE seed's phases on every graph launch; pass noise_angle", what);
    return 0;
}

extern "C" {

int tvc_version(void) { return TVC_ABI_VERSION; }

int tvc_ctx_create(int hip_device, tvc_ctx** out) {
    if (!out) return TVC_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count) return TVC_ERR_HIP;
    tvc_ctx* c = new tvc_ctx();
    c->device = hip_device;
    {   // constant tables (FFT twiddles, Hann window): independent of any checkpoint
        ArenaBuilder ab;
        pack_constants(c, &ab);
        if (hipSetDevice(hip_device) != hipSuccess ||
            hipMalloc((void**)&c->const_arena, ab.buf.size() * sizeof(float)) != hipSuccess ||
            hipMemcpy(c->const_arena, ab.buf.data(), ab.buf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            if (c->const_arena) (void)hipFree(c->const_arena);
            delete c;
            return TVC_ERR_HIP;
        }
        ab.resolve(c->const_arena);
    }
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess) {
        tvc_ctx_destroy(c);
        return TVC_ERR_HIP;
    }
    // the side stream carries the pitch estimator beside the SSL trunk (encoder.hip): lowest priority, so that its workgroups take the
    // slots the trunk's launches leave free instead of competing with them (the pitch chain has ~150 us of slack)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_least) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_amps, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_src, hipEventDisableTiming) != hipSuccess) {
        tvc_ctx_destroy(c);
        return TVC_ERR_HIP;
    }
    *out = c;
    return TVC_OK;
}

void tvc_ctx_destroy(tvc_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto& r : ctx->regions) {
        if (r.a) (void)hipEventDestroy(r.a);
        if (r.b) (void)hipEventDestroy(r.b);
    }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_fork2) (void)hipEventDestroy(ctx->ev_fork2);
    if (ctx->ev_join2) (void)hipEventDestroy(ctx->ev_join2);
    if (ctx->ev_amps) (void)hipEventDestroy(ctx->ev_amps);
    if (ctx->ev_src) (void)hipEventDestroy(ctx->ev_src);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    frontdoor_release(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->const_arena) (void)hipFree(ctx->const_arena);
    delete ctx;
}

const char* tvc_last_error(const tvc_ctx* ctx) { return ctx ? ctx->err : "null ctx"; }

int tvc_load_tensor(tvc_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim) {
    if (!ctx || !key || !host_data || !shape || ndim < 1 || ndim > 4) return fail(ctx, TVC_ERR_ARG, "tvc_load_tensor: bad argument");
    size_t n = 1;
    HostTensor t;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_load_tensor(%s): bad shape", key);
        n *= (size_t)shape[i];
        t.shape.push_back(shape[i]);
    }
    t.data.assign(host_data, host_data + n);
    ctx->host[key] = std::move(t);
    ctx->enc_ready = ctx->dec_ready = false;
    return TVC_OK;
}

int tvc_set_pitch_table(tvc_ctx* ctx, const float* host_freqs, int n) {
    if (!ctx || !host_freqs || n != kPitchClasses) return fail(ctx, TVC_ERR_ARG, "pitch table must have %d entries", kPitchClasses);
    ctx->pitch_table.assign(host_freqs, host_freqs + n);
    ctx->enc_ready = ctx->dec_ready = false;
    return TVC_OK;
}

int tvc_finalize_weights(tvc_ctx* ctx) {
    if (!ctx) return TVC_ERR_ARG;
    ctx->enc_ready = ctx->dec_ready = false;
    ArenaBuilder ab;
    std::string missing_enc, missing_dec;
    pack_checkpoint(ctx, &ab, &missing_enc, &missing_dec);
    snprintf(ctx->enc_missing, sizeof(ctx->enc_missing), "%s", missing_enc.c_str());
    snprintf(ctx->dec_missing, sizeof(ctx->dec_missing), "%s", missing_dec.c_str());
    if (!missing_enc.empty() && !missing_dec.empty())
        return fail(ctx, TVC_ERR_STATE, "no complete checkpoint: encoder lacks %s; decoder lacks %s", missing_enc.c_str(), missing_dec.c_str());

    TVC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->arena) {
        TVC_HIP(ctx, hipFree(ctx->arena));
        ctx->arena = nullptr;
    }
    ctx->arena_floats = ab.buf.size();
    TVC_HIP(ctx, hipMalloc((void**)&ctx->arena, ctx->arena_floats * sizeof(float)));
    TVC_HIP(ctx, hipMemcpy(ctx->arena, ab.buf.data(), ctx->arena_floats * sizeof(float), hipMemcpyHostToDevice));
    ab.resolve(ctx->arena);
    ctx->enc_ready = missing_enc.empty();
    ctx->dec_ready = missing_dec.empty();
    ctx->host.clear();   // staged copies are no longer needed
    return TVC_OK;
}

}  // extern "C"

int tvc::need_ready(tvc_ctx* ctx, int need) {
    if (!ctx) return TVC_ERR_ARG;
    if ((need & NEED_ENC) && !ctx->enc_ready)
        return fail(ctx, TVC_ERR_STATE, "encoder weights not loaded (%s)", ctx->enc_missing[0] ? ctx->enc_missing : "tvc_finalize_weights not called");
    if ((need & NEED_DEC) && !ctx->dec_ready)
        return fail(ctx, TVC_ERR_STATE, "decoder weights not loaded (%s)", ctx->dec_missing[0] ? ctx->dec_missing : "tvc_finalize_weights not called");
    return 0;
}

extern "C" {

int tvc_stft_mag_f32(tvc_ctx* ctx, void* stream, const float* wav, float* spec, int B, int64_t L, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!wav || !spec || B <= 0 || L <= 0 || L % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_stft_mag_f32: bad argument (L must be a multiple of 480)");
    if (L < kNfft / 2 + 1) return fail(ctx, TVC_ERR_ARG, "tvc_stft_mag_f32: L must exceed 960 (reflect padding)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_stft(ctx, s, ws, wav, spec, B, L); });
}

int64_t tvc_resample_out_len(int64_t n, int orig_freq, int new_freq) { return resample_out_len(n, orig_freq, new_freq); }

int tvc_resample_f32(tvc_ctx* ctx, void* stream, const float* x, float* y, int rows, int64_t n, int orig_freq, int new_freq) {
    if (!ctx) return TVC_ERR_ARG;
    if (!x || !y || rows <= 0 || n <= 0 || orig_freq <= 0 || new_freq <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_resample_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_resample(ctx, (hipStream_t)stream, x, y, rows, n, orig_freq, new_freq);
}

int tvc_pcm16_to_f32(tvc_ctx* ctx, void* stream, const int16_t* pcm, float* y, int64_t n, float gain_db) {
    if (!ctx) return TVC_ERR_ARG;
    if (!pcm || !y || n <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_pcm16_to_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pcm16_to_f32(ctx, (hipStream_t)stream, pcm, y, n, gain_db);
}

int tvc_f32_to_pcm16(tvc_ctx* ctx, void* stream, const float* x, int16_t* pcm, int64_t n, float gain_db) {
    if (!ctx) return TVC_ERR_ARG;
    if (!x || !pcm || n <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_f32_to_pcm16: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_f32_to_pcm16(ctx, (hipStream_t)stream, x, pcm, n, gain_db);
}

int tvc_energy_f32(tvc_ctx* ctx, void* stream, const float* wav, float* energy, int B, int64_t L, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!wav || !energy || B <= 0 || L < 128) return fail(ctx, TVC_ERR_ARG, "tvc_energy_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_energy(ctx, s, ws, wav, energy, B, L); });
}

int tvc_encoder_f32(tvc_ctx* ctx, void* stream, const float* spec, float* ssl, float* f0, float* logits, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC));
    if (!spec || !ssl || !f0 || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_encoder_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_encoder(ctx, s, ws, spec, ssl, f0, logits, B, T); });
}

int tvc_pitch_decode_f32(tvc_ctx* ctx, void* stream, const float* logits, float* f0, int B, int T) {
    TVC_CHECK(need_ready(ctx, NEED_ENC));
    if (!logits || !f0 || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_decode_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_decode(ctx, (hipStream_t)stream, logits, f0, B, T);
}

int64_t tvc_knn_prepared_elems(int64_t N) {
    return N <= 0 ? 0 : blob_elems(KIND_F32, N);
}

int64_t tvc_knn_prepared_elems_f16(int64_t N) {
    return N <= 0 ? 0 : blob_elems(KIND_F16, N);
}

int tvc_knn_prepare_index_f32(tvc_ctx* ctx, void* stream, const float* index, float* prepared, int64_t N) {
    if (!ctx) return TVC_ERR_ARG;
    if (!index || !prepared || N <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_prepare_index_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    blob_forget(prepared);
    TVC_CHECK(run_prepare_index(ctx, (hipStream_t)stream, index, prepared, N));
    blob_record(prepared, N);
    return TVC_OK;
}

int tvc_knn_forget(tvc_ctx* ctx, const float* prepared) {
    if (!ctx) return TVC_ERR_ARG;
    blob_forget(prepared);
    return TVC_OK;
}

int tvc_knn_prepare_index_f16(tvc_ctx* ctx, void* stream, const void* rows_f16, float* prepared, int64_t N) {
    if (!ctx) return TVC_ERR_ARG;
    if (!rows_f16 || !prepared || N <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_prepare_index_f16: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    blob_forget(prepared);
    TVC_CHECK(run_prepare_index_f16(ctx, (hipStream_t)stream, rows_f16, prepared, N));
    blob_record(prepared, N);
    return TVC_OK;
}

static int prepare_cols_check(tvc_ctx* ctx, const float* feats, int64_t S, const int64_t* cols, int64_t N, const float* prepared, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    if (!feats || !cols || !prepared || S <= 0 || N <= 0) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    if (N > 0x7fffffff - 128) return fail(ctx, TVC_ERR_ARG, "%s: N beyond 32-bit indexing", what);
    return 0;
}

int tvc_knn_prepare_index_cols_f32(tvc_ctx* ctx, void* stream, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared,
                                   float* index_out) {
    TVC_CHECK(prepare_cols_check(ctx, feats, S, cols, N, prepared, "tvc_knn_prepare_index_cols_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    blob_forget(prepared);
    TVC_CHECK(run_prepare_index_cols(ctx, (hipStream_t)stream, feats, S, cols, N, prepared, index_out));
    blob_record(prepared, N);
    return TVC_OK;
}

int tvc_knn_prepare_index_cols_f16(tvc_ctx* ctx, void* stream, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared,
                                   void* index_out_f16) {
    TVC_CHECK(prepare_cols_check(ctx, feats, S, cols, N, prepared, "tvc_knn_prepare_index_cols_f16"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    blob_forget(prepared);
    TVC_CHECK(run_prepare_index_cols_f16(ctx, (hipStream_t)stream, feats, S, cols, N, prepared, index_out_f16));
    blob_record(prepared, N);
    return TVC_OK;
}

int tvc_knn_match_f32(tvc_ctx* ctx, void* stream, const float* src, const float* prepared, int64_t N, float* out,
                      int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !prepared || !out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_f32: bad argument");
    if (N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_f32: index needs at least k=4 vectors (torch.topk raises too)");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_knn_match_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_knn(ctx, s, ws, src, prepared, N, out, idx_out, B, T); });
}

int tvc_knn_match_general_f32(tvc_ctx* ctx, void* stream, const float* src, const float* index, int64_t N, int k, int metric, float* out,
                              int64_t* idx_out, float* sim_out, int B, int T, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !index || !out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_general_f32: bad argument");
    if (k < 1 || k > 8) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_general_f32: k must be 1 ... 8");
    if (metric < 0 || metric > 2) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_general_f32: metric is 0 ('cos'), 1 ('IP') or 2 ('L2')");
    if (N < k) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_general_f32: selected index k out of range (the index has fewer than k vectors; torch.topk raises too)");
    if (N > 0x7ffffffe || (long)B * T > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_general_f32: sizes beyond 32-bit indexing");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_knn_general(ctx, s, ws, src, index, N, k, metric, out, idx_out, sim_out, B, T); });
}

int tvc_knn_topk_f32(tvc_ctx* ctx, void* stream, const float* src, const float* prepared, int64_t N, float* sims_out,
                     int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !prepared || !sims_out || !idx_out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_topk_f32: bad argument");
    if (N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_knn_topk_f32: an index shard needs at least k=4 vectors");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_knn_topk_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_knn_topk(ctx, s, ws, src, prepared, N, sims_out, idx_out, B, T); });
}

int tvc_knn_gather_slots_f32(tvc_ctx* ctx, void* stream, const float* prepared, int64_t N, const int64_t* idx, float* slots,
                             int64_t nslots) {
    if (!ctx) return TVC_ERR_ARG;
    if (!prepared || !idx || !slots || N <= 0 || nslots <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_gather_slots_f32: bad argument");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_knn_gather_slots_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_knn_slots(ctx, (hipStream_t)stream, prepared, N, idx, slots, nslots);
}

int tvc_knn_finish_f32(tvc_ctx* ctx, void* stream, const float* slots, float* out, int B, int T) {
    if (!ctx) return TVC_ERR_ARG;
    if (!slots || !out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_finish_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_knn_finish(ctx, (hipStream_t)stream, slots, out, B, T);
}

int tvc_shift_frequency_f32(tvc_ctx* ctx, void* stream, const float* f0, float* out, int64_t n, float semitones) {
    if (!ctx) return TVC_ERR_ARG;
    if (!f0 || !out || n <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_shift_frequency_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_shift(ctx, (hipStream_t)stream, f0, out, n, semitones);
}

int tvc_noise_angle_from_uniform_f32(tvc_ctx* ctx, void* stream, float* u, int64_t n) {
    if (!ctx) return TVC_ERR_ARG;
    if (!u || n <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_noise_angle_from_uniform_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_uniform_to_angle(ctx, (hipStream_t)stream, u, n);
}

int tvc_decoder_stages_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0, const float* energy,
                           const float* noise_angle, uint64_t seed, float* wave, float* amps, float* kernel,
                           float* source, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_DEC));
    if (!content || !f0 || !energy || B <= 0 || T <= 0 || (!wave && !amps && !kernel && !source)) return fail(ctx, TVC_ERR_ARG, "tvc_decoder_f32: bad argument");
    if (wave || source) TVC_CHECK(draw_under_capture(ctx, (hipStream_t)stream, noise_angle, "tvc_decoder_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_decoder(ctx, s, ws, content, f0, energy, noise_angle, seed, wave, amps, kernel, source, B, T); });
}

int tvc_filter_net_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0, const float* energy, const float* source,
                       float* wave, float* const* skips, float* const* ups, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_DEC));
    if (!content || !f0 || !energy || !source || !wave || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_filter_net_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    FilterTaps taps;
    for (int i = 0; i < 5 && skips; ++i) taps.skips[i] = skips[i];
    for (int i = 0; i < 4 && ups; ++i) taps.ups[i] = ups[i];
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_filter(ctx, s, ws, content, f0, energy, source, wave, B, T, &taps); });
}

int tvc_dsp_f32(tvc_ctx* ctx, void* stream, const float* f0, const float* amps, const float* kernel, const float* noise_angle,
                uint64_t seed, float* source, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!f0 || !amps || !kernel || !source || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_dsp_f32: bad argument");
    TVC_CHECK(draw_under_capture(ctx, (hipStream_t)stream, noise_angle, "tvc_dsp_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_dsp(ctx, s, ws, f0, amps, kernel, noise_angle, seed, source, B, T); });
}

int tvc_decoder_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0, const float* energy,
                    const float* noise_angle, uint64_t seed, float* wave, int B, int T, void* wsp, size_t ws_bytes) {
    return tvc_decoder_stages_f32(ctx, stream, content, f0, energy, noise_angle, seed, wave, nullptr, nullptr, nullptr, B, T, wsp, ws_bytes);
}

// ---- ragged batches: the plan (ragged.hip) as callers see it, and the ragged encode ----------------------------------------------------
int tvc_ctx_set_ragged_batch_frames(tvc_ctx* ctx, int max_frames) {
    if (!ctx) return TVC_ERR_ARG;
    if (max_frames < 0) return fail(ctx, TVC_ERR_ARG, "tvc_ctx_set_ragged_batch_frames: the cap is a frame count (0 = the default)");
    ctx->rag_batch_frames = max_frames;
    return TVC_OK;
}
int tvc_ragged_plan(int B, int64_t Lmax, const int64_t* lens, int max_frames, int32_t* batch_of_row, int* n_batches) {
    if (!lens || !batch_of_row || !n_batches || B <= 0 || Lmax <= 0 || Lmax % kHop != 0 || max_frames < 0) return TVC_ERR_ARG;
    std::vector<RagBatchPlan> batches;
    const int rc = ragged_split(nullptr, max_frames, B, Lmax, lens, &batches);
    if (rc) return rc;
    for (size_t i = 0; i < batches.size(); ++i)
        for (int b : batches[i].rows) batch_of_row[b] = (int32_t)i;
    *n_batches = (int)batches.size();
    return TVC_OK;
}

int tvc_workspace_bytes_encode_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || !lens || B <= 0 || Lmax <= 0 || Lmax % kHop != 0) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_encode_ragged: need B>0, Lmax%%480==0, lens[B]");
    std::vector<RagBatchPlan> batches;
    std::vector<int> gpre;
    int64_t S = 0;
    TVC_CHECK(encode_ragged_plan(ctx, B, Lmax, lens, &batches, &gpre, &S));
    return measure(kRagGranule, out_bytes, [&](Ws& ws) { return encode_ragged_batches(ctx, nullptr, ws, batches, gpre, kDryPtr, Lmax, kDryPtr, kDryPtr, S); });
}

int tvc_encode_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, float* ssl, float* f0, int B, void* wsp,
                          size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC));
    if (!wav || !lens || !ssl || !f0 || B <= 0 || Lmax <= 0 || Lmax % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_encode_ragged_f32: bad argument (Lmax must be a positive multiple of 480)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<RagBatchPlan> batches;
    std::vector<int> gpre;
    int64_t S = 0;
    TVC_CHECK(encode_ragged_plan(ctx, B, Lmax, lens, &batches, &gpre, &S));
    return run_walks(ctx, __func__, wsp, ws_bytes, kRagGranule, [&](Ws& ws) { return encode_ragged_batches(ctx, s, ws, batches, gpre, wav, Lmax, ssl, f0, S); });
}

// ---- compacting an index: k-means over a prepared blob (index_compact.hip) -------------------------------------------------------
static int compact_check(tvc_ctx* ctx, int64_t N, int64_t K, const char* what) {
    if (K < 4 || K > N) return fail(ctx, TVC_ERR_ARG, "%s: need 4 <= K <= N (K = %lld, N = %lld)", what, (long long)K, (long long)N);
    if (K > kIndexCompactMaxK) return fail(ctx, TVC_ERR_ARG, "%s: K = %lld is above the limit of %lld centroids", what, (long long)K, (long long)kIndexCompactMaxK);
    if (N > 0x7fffff00L) return fail(ctx, TVC_ERR_ARG, "%s: N beyond 32-bit indexing", what);
    return 0;
}

int tvc_ctx_set_index_assign_chunk(tvc_ctx* ctx, int max_queries) {
    if (!ctx) return TVC_ERR_ARG;
    if (max_queries < 0) return fail(ctx, TVC_ERR_ARG, "tvc_ctx_set_index_assign_chunk: the chunk is a count of query columns (0 = the default)");
    ctx->index_assign_chunk = max_queries;
    return TVC_OK;
}

int tvc_workspace_bytes_index_compact(tvc_ctx* ctx, int64_t N, int64_t K, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!out_bytes) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_index_compact: out_bytes is NULL");
    TVC_CHECK(compact_check(ctx, N, K, "tvc_workspace_bytes_index_compact"));
    return measure(1, out_bytes, [&](Ws& ws) { return run_index_compact(ctx, nullptr, ws, kDryPtr, N, nullptr, K, 1, kDryPtr, kDryPtr, nullptr, nullptr, nullptr); });
}

int tvc_index_assign_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const float* centroids_prepared, int64_t K,
                         int64_t* assign_inout, float* sim_out, int32_t* moved_out, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!points_prepared || !centroids_prepared || !assign_inout) return fail(ctx, TVC_ERR_ARG, "tvc_index_assign_f32: bad argument");
    TVC_CHECK(compact_check(ctx, N, K, "tvc_index_assign_f32"));
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(blob_check(ctx, s, points_prepared, N, "tvc_index_assign_f32 (points)"));
    TVC_CHECK(blob_check(ctx, s, centroids_prepared, K, "tvc_index_assign_f32 (centroids)"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_index_assign(ctx, s, ws, points_prepared, N, centroids_prepared, K, assign_inout, sim_out, moved_out); });
}

int tvc_index_update_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const int64_t* assign, int64_t K, float* centroids_inout,
                         int32_t* counts_out, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!points_prepared || !assign || !centroids_inout) return fail(ctx, TVC_ERR_ARG, "tvc_index_update_f32: bad argument");
    TVC_CHECK(compact_check(ctx, N, K, "tvc_index_update_f32"));
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(blob_check(ctx, s, points_prepared, N, "tvc_index_update_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) { return run_index_update(ctx, s, ws, points_prepared, N, assign, K, centroids_inout, counts_out); });
}

int tvc_index_compact_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const int64_t* init_cols, int64_t K, int iters,
                          float* centroids_out, float* prepared_out, int64_t* assign_out, int32_t* counts_out, int32_t* moved_out, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!points_prepared || !init_cols || !centroids_out || !prepared_out || iters < 1) return fail(ctx, TVC_ERR_ARG, "tvc_index_compact_f32: bad argument (iters >= 1)");
    TVC_CHECK(compact_check(ctx, N, K, "tvc_index_compact_f32"));
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(blob_check(ctx, s, points_prepared, N, "tvc_index_compact_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    blob_forget(prepared_out);
    TVC_CHECK(run_walks(ctx, __func__, wsp, ws_bytes, 1, [&](Ws& ws) {
        return run_index_compact(ctx, s, ws, points_prepared, N, init_cols, K, iters, centroids_out, prepared_out, assign_out, counts_out, moved_out);
    }));
    blob_record(prepared_out, K);
    return TVC_OK;
}

int tvc_profile_enable(tvc_ctx* ctx, int on) {
    if (!ctx) return TVC_ERR_ARG;
    ctx->profiling = on < 0 ? 0 : (on > 2 ? 1 : on);
    return TVC_OK;
}

// Synchronises the recorded events and writes "name=ms;name=ms;..." (durations summed per region
// name since the last read) into buf.
int tvc_profile_read(tvc_ctx* ctx, char* buf, size_t buf_bytes) {
    if (!ctx || !buf || buf_bytes < 2) return TVC_ERR_ARG;
    std::vector<std::pair<std::string, double>> agg;
    for (auto& r : ctx->regions) {
        float ms = 0.f;
        if (r.a && r.b && hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            bool found = false;
            for (auto& a : agg)
                if (a.first == r.name) {
                    a.second += ms;
                    found = true;
                }
            if (!found) agg.push_back({r.name, ms});
        }
        if (r.a) ctx->event_pool.push_back(r.a);
        if (r.b) ctx->event_pool.push_back(r.b);
    }
    ctx->regions.clear();
    std::string out;
    for (auto& a : agg) {
        char tmp[160];
        snprintf(tmp, sizeof(tmp), "%s=%.6f;", a.first.c_str(), a.second);
        out += tmp;
    }
    snprintf(buf, buf_bytes, "%s", out.c_str());
    return TVC_OK;
}

}  // extern "C"
