// libtinyvc_hip.so — context, workspace sizing and the extern "C" surface (checkpoint packing: pack.hip).
#include <atomic>
#include <cmath>
#include <functional>
#include <mutex>

#include <cstdlib>

#include "tvc_common.h"

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
static int blob_check(tvc_ctx* ctx, hipStream_t s, const void* p, int64_t N, const char* what) {
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
    int h[6] = {0, 0, 0, 0, 0, 0};
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h, p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ctx, TVC_ERR_HIP, "%s: cannot read the prepared index's header", what);
    const int64_t n = ((int64_t)(unsigned)h[3] << 32) | (unsigned)h[2];
    if (h[0] != tvc::kBlobMagic || (h[1] != 0 && h[1] != 1))
        return fail(ctx, TVC_ERR_ARG, "%s: `prepared` is not a blob of tvc_knn_prepare_index_f32 / _f16", what);
    if (h[5] != tvc::kBlobVersion)
        return fail(ctx, TVC_ERR_ARG, "%s: the prepared index has format version %d, this library writes and reads version %d: prepare it again", what, h[5], tvc::kBlobVersion);
    if (n != N) return fail(ctx, TVC_ERR_ARG, "%s: this blob was prepared for N = %lld index vectors, the call says N = %lld", what, (long long)n, (long long)N);
    blob_record(p, N);
    return 0;
}

// noise_angle = NULL makes the library draw the phases from `seed` - a kernel ARGUMENT, which a stream capture bakes into the graph: every replay
// would synthesise the same noise.  A capturing caller must pass the phases (a buffer it refills between replays, as the module path does).
static int draw_under_capture(tvc_ctx* ctx, hipStream_t s, const float* noise_angle, const char* what) {
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
        hipEventCreateWithFlags(&c->ev_amps, hipEventDisableTiming) != hipSuccess) {
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

enum { NEED_NONE = 0, NEED_ENC = 1, NEED_DEC = 2 };
static int need_ready(tvc_ctx* ctx, int need) {
    if (!ctx) return TVC_ERR_ARG;
    if ((need & NEED_ENC) && !ctx->enc_ready)
        return fail(ctx, TVC_ERR_STATE, "encoder weights not loaded (%s)", ctx->enc_missing[0] ? ctx->enc_missing : "tvc_finalize_weights not called");
    if ((need & NEED_DEC) && !ctx->dec_ready)
        return fail(ctx, TVC_ERR_STATE, "decoder weights not loaded (%s)", ctx->dec_missing[0] ? ctx->dec_missing : "tvc_finalize_weights not called");
    return 0;
}

// One prepared index (and optionally one pitch shift) per row of a call (tvc_*_multi): host arrays indexed by the caller's row.
struct RowIndex {
    const float* const* blob;
    const int64_t* N;
    const float* shifts;       // nullptr: every row takes the call's pitch_shift
};

static int convert_impl(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* wav, const float* prepared,
                        int64_t N, float pitch_shift, const float* angle,
                        uint64_t seed, float* wave, int B, int64_t L, const RowIndex* rows = nullptr) {
    const int T = (int)(L / kHop);
    float* spec = ws.get<float>((size_t)B * kBins * T);
    float* energy = ws.get<float>((size_t)B * L);
    float* ssl = ws.get<float>((size_t)B * kSslDim * T);
    float* matched = ws.get<float>((size_t)B * kSslDim * T);
    float* f0 = ws.get<float>((size_t)B * T);
    float* f0s = ws.get<float>((size_t)B * T);
    // |max| slots the path can bound without a pass over the tensors (block-floating-point guard of the fp16 split, split_fp16.h; equal-length
    // batches): emax = max |wav| per utterance (the energy stage's pooled maxima, 1 500 values each) bounds the energy envelope - a linear
    // interpolation of them - and, times the Hann window's sum (960), every |STFT| bin; `matched` is a mean of index rows.
    // A ragged batch (the driver passed B = 1, T = all frames: ragged.h) derives them per utterance in the same way - an utterance's scales,
    // and with them its bits, are those of its own B = 1 call at every input amplitude (test_gpu_ragged.py scales the input by 1e4 and 1e-7).
    const int NB = ctx->rag ? ctx->rag->B : B;
    float* emax = ws.get<float>((size_t)5 * NB);
    float* spec_bound = emax + NB;
    float* enc_slots = spec_bound + NB;      // the encoder's three atomicMax slots: zeroed by the energy stage's pooled-maximum launch
    const bool bounds = true;
    // one index per row: every utterance's matched-content bound is its own index's |max| (so its fp16-split scales, and its bits, are those
    // of its own B = 1 call), and its runs of query columns go to the search as segments; per-row pitch shifts travel like the lengths
    float* rowmax = rows ? ws.get<float>((size_t)NB) : nullptr;
    float* rshift = rows && rows->shifts ? ws.get<float>((size_t)NB) : nullptr;
    std::vector<KnnSegIn> segs;
    if (rows) {
        for (int i = 0; i < NB; ++i) {
            const int r = ctx->rag ? ctx->rag->row[i] : i;
            const int c0 = ctx->rag ? ctx->rag->pre[i] : i * T, nc = ctx->rag ? ctx->rag->tb[i] : T;
            segs.push_back(KnnSegIn{rows->blob[r], rows->N[r], c0, nc});
        }
    } else {
        segs.push_back(KnnSegIn{prepared, N, 0, B * T});
    }
    if (rows && !ws.dry) {
        std::vector<const float*> bl(NB);
        std::vector<int> sh(NB);
        for (int i = 0; i < NB; ++i) {
            const int r = ctx->rag ? ctx->rag->row[i] : i;
            bl[i] = rows->blob[r];
            if (rshift) std::memcpy(&sh[i], &rows->shifts[r], sizeof(int));
        }
        TVC_CHECK(run_knn_amax_rows(ctx, s, bl, rowmax));
        if (rshift) TVC_CHECK(upload_ints(ctx, s, sh, reinterpret_cast<int*>(rshift)));
    }
    size_t m = ws.mark();
    {
        ProfScope ps(ctx, s, ws, "stft");
        TVC_CHECK(run_stft(ctx, s, ws, wav, spec, B, L));
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "energy");
        TVC_CHECK(run_energy(ctx, s, ws, wav, energy, B, L, bounds ? emax : nullptr, bounds ? spec_bound : nullptr, bounds ? enc_slots : nullptr, 3 * NB));
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "encoder");
        TVC_CHECK(run_encoder(ctx, s, ws, spec, ssl, f0, nullptr, B, T, bounds ? spec_bound : nullptr, bounds ? enc_slots : nullptr, f0s, pitch_shift, rshift));
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "knn");
        TVC_CHECK(run_knn_segs(ctx, s, ws, ssl, segs.data(), (int)segs.size(), matched, nullptr, B, T));
    }
    ws.release(m);
    TVC_CHECK(run_decoder(ctx, s, ws, matched, f0s, energy, angle, seed, wave, nullptr, nullptr, nullptr, B, T, ws.dry ? nullptr : (rows ? rowmax : knn_index_amax(prepared)),
                          bounds ? emax : nullptr, rows ? 1 : 0));
    ws.release(m);
    return 0;
}

// stands for a caller's buffer in a walk that only sizes the workspace (ws.dry: no pointer is dereferenced)
static float* const kDryPtr = (float*)(uintptr_t)256;

// behind the launching walk of an entry: it took no more workspace than its measuring walk (ws.dry) found
static int walks_agree(tvc_ctx* ctx, const char* entry, size_t real_peak, size_t measured) {
    return real_peak <= measured ? TVC_OK : fail(ctx, TVC_ERR_WORKSPACE, "%s: the launching walk took %zu workspace bytes, the measuring walk %zu", entry, real_peak, measured);
}

int tvc_workspace_bytes(tvc_ctx* ctx, int B, int64_t L, int64_t N, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || B <= 0 || L <= 0 || L % kHop != 0 || N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes: need B>0, L%%480==0, N>=4");
    Ws ws(nullptr, 0, true);
    TVC_CHECK(convert_impl(ctx, nullptr, ws, kDryPtr, kDryPtr, N, 0.f, nullptr, 0, kDryPtr, B, L));
    *out_bytes = ws.peak + 4096;
    return TVC_OK;
}

// Workspace is validated *before* launching: every entry walks `call` twice, first with a Ws that only measures (ws.dry), then with the
// caller's workspace.  Both walks take the same allocations (tvc_common.h Ws); the host check behind the second one states it.
#define TVC_RUN(call)                                                                                                           \
    {                                                                                                                           \
        Ws need(nullptr, 0, true);                                                                                              \
        {                                                                                                                       \
            Ws& ws = need;                                                                                                      \
            TVC_CHECK(call);                                                                                                    \
        }                                                                                                                       \
        if (need.peak > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need.peak, ws_bytes); \
        Ws ws(wsp, ws_bytes, false);                                                                                            \
        TVC_CHECK(call);                                                                                                        \
        return walks_agree(ctx, __func__, ws.peak, need.peak);                                                                  \
    }

int tvc_stft_mag_f32(tvc_ctx* ctx, void* stream, const float* wav, float* spec, int B, int64_t L, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!wav || !spec || B <= 0 || L <= 0 || L % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_stft_mag_f32: bad argument (L must be a multiple of 480)");
    if (L < kNfft / 2 + 1) return fail(ctx, TVC_ERR_ARG, "tvc_stft_mag_f32: L must exceed 960 (reflect padding)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    TVC_RUN(run_stft(ctx, s, ws, wav, spec, B, L));
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
    TVC_RUN(run_energy(ctx, s, ws, wav, energy, B, L));
}

int tvc_encoder_f32(tvc_ctx* ctx, void* stream, const float* spec, float* ssl, float* f0, float* logits, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC));
    if (!spec || !ssl || !f0 || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_encoder_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    TVC_RUN(run_encoder(ctx, s, ws, spec, ssl, f0, logits, B, T));
}

int tvc_pitch_decode_f32(tvc_ctx* ctx, void* stream, const float* logits, float* f0, int B, int T) {
    TVC_CHECK(need_ready(ctx, NEED_ENC));
    if (!logits || !f0 || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_decode_f32: bad argument");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_decode(ctx, (hipStream_t)stream, logits, f0, B, T);
}

int64_t tvc_knn_prepared_elems(int64_t N) {
    if (N <= 0) return 0;
    int64_t npad = (N + 127) / 128 * 128;
    // header + raw rows [N][768] + split image of the normalised vectors (3 bf16 per value = 1.5 floats)
    // + inverse norms [Npad] + fp16 image of the normalised vectors (the coarse pass's operand, half a float per value)
    return 64 + N * (int64_t)kSslDim + (int64_t)kSslDim * npad * 3 / 2 + npad + (int64_t)kSslDim * npad / 2;
}

int64_t tvc_knn_prepared_elems_f16(int64_t N) {
    if (N <= 0) return 0;
    int64_t npad = (N + 127) / 128 * 128;
    // header + inverse norms [Npad] + fp16 image (half a float per value) + the largest inverse norm of every 128-vector tile
    return 64 + npad + (int64_t)kSslDim * npad / 2 + npad / 128;
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
    TVC_RUN(run_knn(ctx, s, ws, src, prepared, N, out, idx_out, B, T));
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
    TVC_RUN(run_knn_general(ctx, s, ws, src, index, N, k, metric, out, idx_out, sim_out, B, T));
}

int tvc_knn_topk_f32(tvc_ctx* ctx, void* stream, const float* src, const float* prepared, int64_t N, float* sims_out,
                     int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !prepared || !sims_out || !idx_out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_knn_topk_f32: bad argument");
    if (N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_knn_topk_f32: an index shard needs at least k=4 vectors");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_knn_topk_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    TVC_RUN(run_knn_topk(ctx, s, ws, src, prepared, N, sims_out, idx_out, B, T));
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
    TVC_RUN(run_decoder(ctx, s, ws, content, f0, energy, noise_angle, seed, wave, amps, kernel, source, B, T));
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
    TVC_RUN(run_filter(ctx, s, ws, content, f0, energy, source, wave, B, T, &taps));
}

int tvc_dsp_f32(tvc_ctx* ctx, void* stream, const float* f0, const float* amps, const float* kernel, const float* noise_angle,
                uint64_t seed, float* source, int B, int T, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!f0 || !amps || !kernel || !source || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "tvc_dsp_f32: bad argument");
    TVC_CHECK(draw_under_capture(ctx, (hipStream_t)stream, noise_angle, "tvc_dsp_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    TVC_RUN(run_dsp(ctx, s, ws, f0, amps, kernel, noise_angle, seed, source, B, T));
}

int tvc_decoder_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0, const float* energy,
                    const float* noise_angle, uint64_t seed, float* wave, int B, int T, void* wsp, size_t ws_bytes) {
    return tvc_decoder_stages_f32(ctx, stream, content, f0, energy, noise_angle, seed, wave, nullptr, nullptr, nullptr, B, T, wsp, ws_bytes);
}

int tvc_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* prepared, int64_t N,
                    float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L,
                    void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC | NEED_DEC));
    if (!wav || !prepared || !wave || B <= 0 || L <= 0 || L % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_convert_f32: bad argument (L must be a positive multiple of 480)");
    if (L < kNfft / 2 + 1) return fail(ctx, TVC_ERR_ARG, "tvc_convert_f32: L must exceed 960 samples (STFT reflect padding, as torch.stft requires)");
    if (N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_convert_f32: index needs at least k=4 vectors");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_convert_f32"));
    TVC_CHECK(draw_under_capture(ctx, (hipStream_t)stream, noise_angle, "tvc_convert_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    TVC_RUN(convert_impl(ctx, s, ws, wav, prepared, N, pitch_shift, noise_angle, seed, wave, B, L));
}

// ---- ragged batches ---------------------------------------------------------------------------------------------------------
namespace {
// Every utterance of a ragged call is converted inside the kernels (ragged.h), in batches of utterances that select the SAME kernels: which
// FiLM kernel a FilterNet level runs depends on the utterance's own length there (film_s2 / the pre-split hand-over need one 256-column tile:
// 2 T, 6 T, 24 T >= 256, decoder.hip film_conv), so the frame counts split into four classes at 11, 43 and 128 frames; inside a class every
// utterance takes exactly the path its own B = 1 call takes and the result is bit-identical to it.
constexpr int kRagClassBounds[3] = {11, 43, 128};
constexpr int kRagMaxFrames = 80000;       // frames per in-kernel batch: 24 rows x 480 x 4 B x frames stays below the 32-bit byte offsets of the 24-channel kernels
struct RagBatchPlan {
    std::vector<int> rows, frames;
    int Ttot = 0;
};
int ragged_split(tvc_ctx* ctx, int cap, int B, int64_t Lmax, const int64_t* lens, std::vector<RagBatchPlan>* batches, bool classes = true) {
    std::vector<RagBatchPlan> open(4);          // the batch being filled, per class (cap: tvc_ctx_set_ragged_batch_frames / tvc_ragged_plan's argument, 0 = the default)
    const int max_frames = cap > 0 && cap < kRagMaxFrames ? cap : kRagMaxFrames;
    for (int b = 0; b < B; ++b) {
        if (lens[b] <= 0 || lens[b] % kHop || lens[b] > Lmax || lens[b] < kNfft / 2 + 1)
            return fail(ctx, TVC_ERR_ARG, "ragged batch: lens[%d] = %lld must be a multiple of 480 in (960, Lmax]", b, (long long)lens[b]);
        const int T = (int)(lens[b] / kHop);
        if (T > kRagMaxFrames) return fail(ctx, TVC_ERR_ARG, "ragged batch: lens[%d] = %lld is longer than a batch may be; convert it with tvc_convert_f32", b, (long long)lens[b]);
        const int cls = classes ? (T >= kRagClassBounds[0]) + (T >= kRagClassBounds[1]) + (T >= kRagClassBounds[2]) : 0;      // (the encoder's kernels make no length-dependent choice: one class)
        RagBatchPlan& p = open[cls];
        if (p.Ttot + T > max_frames && !p.rows.empty()) {
            batches->push_back(p);
            p = RagBatchPlan();
        }
        p.rows.push_back(b);
        p.frames.push_back(T);
        p.Ttot += T;
    }
    for (int c = 3; c >= 0; --c)
        if (!open[c].rows.empty()) batches->push_back(open[c]);
    return 0;
}
// the batches of a call, one after the other on the caller's stream, each from the start of the same workspace region: [tables][convert
// workspace].  The drivers run a batch as ONE utterance of Ttot frames (B = 1) with ctx->rag set.
int ragged_batches(tvc_ctx* ctx, hipStream_t s, Ws& ws, const std::vector<RagBatchPlan>& batches, const float* wav, int64_t Lmax, const float* prepared,
                   int64_t N, float pitch_shift, const float* angle, uint64_t seed, float* wave, const RowIndex* rows = nullptr) {
    for (auto& p : batches) {
        ws.release(0);
        RagHost h;
        TVC_CHECK(rag_setup(ctx, s, ws, h, p.frames, p.rows, (int)(Lmax / kHop)));
        ctx->rag = &h;
        const int rc = convert_impl(ctx, s, ws, wav, prepared, N, pitch_shift, angle, seed, wave, 1, (int64_t)p.Ttot * kHop, rows);
        ctx->rag = nullptr;
        TVC_CHECK(rc);
    }
    return 0;
}
}  // namespace

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

int tvc_workspace_bytes_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, int64_t N, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || !lens || B <= 0 || Lmax <= 0 || Lmax % kHop != 0 || N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_ragged: need B>0, Lmax%%480==0, N>=4");
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, &batches));
    Ws ws(nullptr, 0, true);      // (no allocation depends on whether the call brings its own noise phases)
    TVC_CHECK(ragged_batches(ctx, nullptr, ws, batches, kDryPtr, Lmax, kDryPtr, N, 0.f, nullptr, 0, kDryPtr));
    *out_bytes = ((ws.peak + 4095) & ~size_t(4095)) + 4096;
    return TVC_OK;
}

int tvc_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* prepared, int64_t N,
                           float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC | NEED_DEC));
    if (!wav || !lens || !prepared || !wave || B <= 0 || Lmax <= 0 || Lmax % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_convert_ragged_f32: bad argument (Lmax must be a positive multiple of 480)");
    if (N < 4) return fail(ctx, TVC_ERR_ARG, "tvc_convert_ragged_f32: index needs at least k=4 vectors");
    TVC_CHECK(blob_check(ctx, (hipStream_t)stream, prepared, N, "tvc_convert_ragged_f32"));
    TVC_CHECK(draw_under_capture(ctx, (hipStream_t)stream, noise_angle, "tvc_convert_ragged_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, &batches));
    Ws need(nullptr, 0, true);
    TVC_CHECK(ragged_batches(ctx, s, need, batches, wav, Lmax, prepared, N, pitch_shift, noise_angle, seed, wave));      // host time on the launch path
    const size_t bytes = (need.peak + 4095) & ~size_t(4095);      // (whole 4 KiB pages, as tvc_workspace_bytes_ragged promises)
    if (bytes > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", bytes, ws_bytes);
    // the whole padded output is cleared once: every kernel writes its utterance's own samples only
    TVC_HIP(ctx, hipMemsetAsync(wave, 0, (size_t)B * Lmax * sizeof(float), s));
    Ws ws(wsp, bytes, false);
    TVC_CHECK(ragged_batches(ctx, s, ws, batches, wav, Lmax, prepared, N, pitch_shift, noise_angle, seed, wave));
    return walks_agree(ctx, __func__, ws.peak, need.peak);
}

// ---- ragged encode ----------------------------------------------------------------------------------------------------------------
// Generator.encode (generator.py:19-23) over utterances of different lengths, as extract_index.py:47-52 needs it for a folder of clips:
// rag_setup, |STFT|, encoder with ctx->rag set - the first half of convert_impl, no index, no decoder.  The spectrogram's |max| slot is
// the measured per-utterance maximum (run_encoder without a bound: run_amax_rows), as in the stage calls tvc_stft_mag_f32 + tvc_encoder_f32
// that Generator.encode makes for one utterance: utterance b's columns are bit-identical to those calls at B = 1.  The length classes of
// ragged_split exist for FilterNet's FiLM kernels; the encoder's kernels choose nothing by an utterance's length, so a call is cut by the
// frame cap alone and its batches are runs of consecutive rows.
namespace {
// packed[c][gpre[row of b] + t'] = batch[c][pre[b] + t'] (c = 768: the f0 row): a later batch's columns into the call's packed outputs
__global__ __launch_bounds__(256) void pack_batch_kernel(const float* __restrict__ ssl_b, const float* __restrict__ f0_b, float* __restrict__ ssl,
                                                         float* __restrict__ f0, RagDev rg, const int* __restrict__ gpre, int Ttot, long S) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Ttot) return;
    const int b = rg.col2b[t];
    const long dst = (long)gpre[rg.row[b]] + (t - rg.pre[b]);
    const int c = blockIdx.y;
    if (c < kSslDim) ssl[(long)c * S + dst] = ssl_b[(long)c * Ttot + t];
    else f0[dst] = f0_b[t];
}
int encode_ragged_batches(tvc_ctx* ctx, hipStream_t s, Ws& ws, const std::vector<RagBatchPlan>& batches, const std::vector<int>& gpre, const float* wav,
                          int64_t Lmax, float* ssl, float* f0, int64_t S) {
    ws.release(0);
    const bool direct = batches.size() == 1;      // one batch holds every row in the caller's order: its layout IS the packed one (row stride S)
    int* d_gpre = nullptr;
    if (!direct) {
        d_gpre = ws.get<int>(gpre.size());
        if (!ws.dry) TVC_CHECK(upload_ints(ctx, s, gpre, d_gpre));
    }
    const size_t m0 = ws.mark();
    for (auto& p : batches) {
        ws.release(m0);
        RagHost h;
        TVC_CHECK(rag_setup(ctx, s, ws, h, p.frames, p.rows, (int)(Lmax / kHop)));
        float* spec = ws.get<float>((size_t)kBins * p.Ttot);
        float* ssl_b = direct ? ssl : ws.get<float>((size_t)kSslDim * p.Ttot);
        float* f0_b = direct ? f0 : ws.get<float>((size_t)p.Ttot);
        ctx->rag = &h;
        int rc = run_stft(ctx, s, ws, wav, spec, 1, (int64_t)p.Ttot * kHop);
        if (!rc) rc = run_encoder(ctx, s, ws, spec, ssl_b, f0_b, nullptr, 1, p.Ttot);
        if (!rc && !direct && !ws.dry) {
            RagDev rg;
            rc = rag_view(ctx, s, 1, 0, &rg, nullptr);
            if (!rc) {
                hipLaunchKernelGGL(pack_batch_kernel, dim3((unsigned)((p.Ttot + 255) / 256), kSslDim + 1), dim3(256), 0, s, ssl_b, f0_b, ssl, f0, rg, d_gpre, p.Ttot, (long)S);
                rc = launch_check(ctx, "encode_ragged pack");
            }
        }
        ctx->rag = nullptr;
        TVC_CHECK(rc);
    }
    return 0;
}
// the call's plan: its batches, the packed column of every row's first frame, S
int encode_ragged_plan(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, std::vector<RagBatchPlan>* batches, std::vector<int>* gpre, int64_t* S) {
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, batches, false));
    gpre->assign((size_t)B, 0);
    int64_t tot = 0;
    for (int b = 0; b < B; ++b) {
        (*gpre)[b] = (int)tot;
        tot += lens[b] / kHop;
        if (tot > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "ragged encode: more than 2^31 - 1 frames in one call");
    }
    *S = tot;
    return 0;
}
}  // namespace

int tvc_workspace_bytes_encode_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || !lens || B <= 0 || Lmax <= 0 || Lmax % kHop != 0) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_encode_ragged: need B>0, Lmax%%480==0, lens[B]");
    std::vector<RagBatchPlan> batches;
    std::vector<int> gpre;
    int64_t S = 0;
    TVC_CHECK(encode_ragged_plan(ctx, B, Lmax, lens, &batches, &gpre, &S));
    Ws ws(nullptr, 0, true);
    TVC_CHECK(encode_ragged_batches(ctx, nullptr, ws, batches, gpre, kDryPtr, Lmax, kDryPtr, kDryPtr, S));
    *out_bytes = ((ws.peak + 4095) & ~size_t(4095)) + 4096;
    return TVC_OK;
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
    Ws need(nullptr, 0, true);
    TVC_CHECK(encode_ragged_batches(ctx, s, need, batches, gpre, wav, Lmax, ssl, f0, S));
    const size_t bytes = (need.peak + 4095) & ~size_t(4095);
    if (bytes > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", bytes, ws_bytes);
    Ws ws(wsp, bytes, false);
    TVC_CHECK(encode_ragged_batches(ctx, s, ws, batches, gpre, wav, Lmax, ssl, f0, S));
    return walks_agree(ctx, __func__, ws.peak, need.peak);
}

// ---- one prepared index per row ------------------------------------------------------------------------------------------------
// The table is checked whole before anything is enqueued: every entry non-null, N >= 4, and the blob_check of the single-index calls.
static int rows_check(tvc_ctx* ctx, hipStream_t s, int B, const float* const* prepared, const int64_t* N, const char* what) {
    if (!prepared || !N) return fail(ctx, TVC_ERR_ARG, "%s: prepared and N are host arrays of B entries", what);
    for (int b = 0; b < B; ++b) {
        if (!prepared[b]) return fail(ctx, TVC_ERR_ARG, "%s: prepared[%d] is NULL", what, b);
        if (N[b] < 4) return fail(ctx, TVC_ERR_ARG, "%s: N[%d] = %lld: an index needs at least k=4 vectors", what, b, (long long)N[b]);
    }
    for (int b = 0; b < B; ++b) TVC_CHECK(blob_check(ctx, s, prepared[b], N[b], what));
    return 0;
}
// the workspace queries plan every row as a segment of its own (distinct stand-in blobs): a call whose rows share blobs needs less
static std::vector<const float*> dry_blobs(int B) {
    std::vector<const float*> v((size_t)B);
    for (int b = 0; b < B; ++b) v[b] = kDryPtr + 64 * (size_t)b;
    return v;
}

int tvc_knn_match_multi_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, float* out,
                            int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !out || B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "tvc_knn_match_multi_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B, prepared, N, "tvc_knn_match_multi_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KnnSegIn> in((size_t)B);
    for (int b = 0; b < B; ++b) in[b] = KnnSegIn{prepared[b], N[b], b * T, T};
    TVC_RUN(run_knn_segs(ctx, s, ws, src, in.data(), B, out, idx_out, B, T));
}

int tvc_workspace_bytes_multi(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || !N || B <= 0 || L <= 0 || L % kHop != 0) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_multi: need B>0, L%%480==0, N[B]");
    for (int b = 0; b < B; ++b)
        if (N[b] < 4) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_multi: N[%d] < 4", b);
    const std::vector<const float*> blobs = dry_blobs(B);
    const float shift = 0.f;
    const RowIndex rows{blobs.data(), N, &shift};      // (a shift table takes workspace: counted; never read in this walk)
    Ws ws(nullptr, 0, true);
    TVC_CHECK(convert_impl(ctx, nullptr, ws, kDryPtr, kDryPtr, N[0], 0.f, nullptr, 0, kDryPtr, B, L, &rows));
    *out_bytes = ws.peak + 4096;
    return TVC_OK;
}

int tvc_convert_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, float pitch_shift,
                          const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC | NEED_DEC));
    if (!wav || !wave || B <= 0 || L <= 0 || L % kHop) return fail(ctx, TVC_ERR_ARG, "tvc_convert_multi_f32: bad argument (L must be a positive multiple of 480)");
    if (L < kNfft / 2 + 1) return fail(ctx, TVC_ERR_ARG, "tvc_convert_multi_f32: L must exceed 960 samples (STFT reflect padding, as torch.stft requires)");
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B, prepared, N, "tvc_convert_multi_f32"));
    TVC_CHECK(draw_under_capture(ctx, s, noise_angle, "tvc_convert_multi_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    const RowIndex rows{prepared, N, pitch_shifts};
    TVC_RUN(convert_impl(ctx, s, ws, wav, prepared[0], N[0], pitch_shift, noise_angle, seed, wave, B, L, &rows));
}

int tvc_workspace_bytes_ragged_multi(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, size_t* out_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || !lens || !N || B <= 0 || Lmax <= 0 || Lmax % kHop != 0)
        return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_ragged_multi: need B>0, Lmax%%480==0, lens[B], N[B]");
    for (int b = 0; b < B; ++b)
        if (N[b] < 4) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_ragged_multi: N[%d] < 4", b);
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, &batches));
    const std::vector<const float*> blobs = dry_blobs(B);
    const float shift = 0.f;
    const RowIndex rows{blobs.data(), N, &shift};
    Ws ws(nullptr, 0, true);
    TVC_CHECK(ragged_batches(ctx, nullptr, ws, batches, kDryPtr, Lmax, kDryPtr, N[0], 0.f, nullptr, 0, kDryPtr, &rows));
    *out_bytes = ((ws.peak + 4095) & ~size_t(4095)) + 4096;
    return TVC_OK;
}

int tvc_convert_ragged_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave,
                                 int B, void* wsp, size_t ws_bytes) {
    TVC_CHECK(need_ready(ctx, NEED_ENC | NEED_DEC));
    if (!wav || !lens || !wave || B <= 0 || Lmax <= 0 || Lmax % kHop)
        return fail(ctx, TVC_ERR_ARG, "tvc_convert_ragged_multi_f32: bad argument (Lmax must be a positive multiple of 480)");
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B, prepared, N, "tvc_convert_ragged_multi_f32"));
    TVC_CHECK(draw_under_capture(ctx, s, noise_angle, "tvc_convert_ragged_multi_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, &batches));
    const RowIndex rows{prepared, N, pitch_shifts};
    Ws need(nullptr, 0, true);
    TVC_CHECK(ragged_batches(ctx, s, need, batches, wav, Lmax, prepared[0], N[0], pitch_shift, noise_angle, seed, wave, &rows));
    const size_t bytes = (need.peak + 4095) & ~size_t(4095);
    if (bytes > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", bytes, ws_bytes);
    TVC_HIP(ctx, hipMemsetAsync(wave, 0, (size_t)B * Lmax * sizeof(float), s));
    Ws ws(wsp, bytes, false);
    TVC_CHECK(ragged_batches(ctx, s, ws, batches, wav, Lmax, prepared[0], N[0], pitch_shift, noise_angle, seed, wave, &rows));
    return walks_agree(ctx, __func__, ws.peak, need.peak);
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
    Ws ws(nullptr, 0, true);
    TVC_CHECK(run_index_compact(ctx, nullptr, ws, kDryPtr, N, nullptr, K, 1, kDryPtr, kDryPtr, nullptr, nullptr, nullptr));
    *out_bytes = ws.peak + 4096;
    return TVC_OK;
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
    TVC_RUN(run_index_assign(ctx, s, ws, points_prepared, N, centroids_prepared, K, assign_inout, sim_out, moved_out));
}

int tvc_index_update_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const int64_t* assign, int64_t K, float* centroids_inout,
                         int32_t* counts_out, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    if (!points_prepared || !assign || !centroids_inout) return fail(ctx, TVC_ERR_ARG, "tvc_index_update_f32: bad argument");
    TVC_CHECK(compact_check(ctx, N, K, "tvc_index_update_f32"));
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(blob_check(ctx, s, points_prepared, N, "tvc_index_update_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    TVC_RUN(run_index_update(ctx, s, ws, points_prepared, N, assign, K, centroids_inout, counts_out));
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
    {
        Ws need(nullptr, 0, true);
        TVC_CHECK(run_index_compact(ctx, s, need, points_prepared, N, init_cols, K, iters, centroids_out, prepared_out, assign_out, counts_out, moved_out));
        if (need.peak > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need.peak, ws_bytes);
        Ws ws(wsp, ws_bytes, false);
        TVC_CHECK(run_index_compact(ctx, s, ws, points_prepared, N, init_cols, K, iters, centroids_out, prepared_out, assign_out, counts_out, moved_out));
        TVC_CHECK(walks_agree(ctx, __func__, ws.peak, need.peak));
    }
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

int tvc_sola_f32(tvc_ctx* ctx, void* stream, const float* y, float* sola_buf, const float* fade_in, float* out,
                 int32_t* shift_out, int S, int64_t Ly, int block, int use_phase_vocoder) {
    if (!ctx) return TVC_ERR_ARG;
    if (!y || !sola_buf || !fade_in || !out || S <= 0 || block <= 0 || Ly < block + kSolaCross + kSolaSearch + kSolaDelay)
        return fail(ctx, TVC_ERR_ARG, "tvc_sola_f32: bad argument (Ly must cover block+1920+1920+3840)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_sola(ctx, (hipStream_t)stream, y, sola_buf, fade_in, out, shift_out, S, Ly, block, use_phase_vocoder);
}

int tvc_stream_push_f32(tvc_ctx* ctx, void* stream, float* buf, const float* blocks, int S, int64_t n, int block) {
    if (!ctx) return TVC_ERR_ARG;
    // (the kernel indexes a row with 32-bit ints and rounds n up to whole 32 768-sample tiles)
    if (!buf || !blocks || S <= 0 || block <= 0 || n < block || n > INT32_MAX - 32768)
        return fail(ctx, TVC_ERR_ARG, "tvc_stream_push_f32: bad argument (block <= n <= 2^31 - 32769)");
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_stream_push(ctx, (hipStream_t)stream, buf, blocks, S, (int)n, block);
}

}  // extern "C"
