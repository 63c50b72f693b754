// libtinyvc_hip.so — the extern "C" surface: context, prepared-blob registry, argument checks, and the two workspace walks every entry
// makes (run_walks; measure for the tvc_workspace_bytes* queries).  An entry validates, describes its call and hands it to run_walks.
// The one driver that lives here is convert_impl (the stage drivers chained); no kernel does - checkpoint packing: pack.hip, the
// ragged batch planner and its loops: ragged.hip.
#include <atomic>
#include <cmath>
#include <mutex>

#include <cstdlib>

#include "knn_blob.h"
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

enum { NEED_NONE = 0, NEED_ENC = 1, NEED_DEC = 2 };
static int need_ready(tvc_ctx* ctx, int need) {
    if (!ctx) return TVC_ERR_ARG;
    if ((need & NEED_ENC) && !ctx->enc_ready)
        return fail(ctx, TVC_ERR_STATE, "encoder weights not loaded (%s)", ctx->enc_missing[0] ? ctx->enc_missing : "tvc_finalize_weights not called");
    if ((need & NEED_DEC) && !ctx->dec_ready)
        return fail(ctx, TVC_ERR_STATE, "decoder weights not loaded (%s)", ctx->dec_missing[0] ? ctx->dec_missing : "tvc_finalize_weights not called");
    return 0;
}

}  // extern "C": convert_impl is declared in tvc_common.h, the walk runners are templates

// Generator.convert: c.B rows of c.L samples each (tvc_common.h ConvertCall; a ragged batch comes as ONE row with ctx->rag set, ragged.hip)
int tvc::convert_impl(tvc_ctx* ctx, hipStream_t s, Ws& ws, const ConvertCall& c) {
    const int B = c.B;
    const int64_t L = c.L;
    const ConvertIndex& ix = c.index;
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
    // An alpha call (c.alpha) mixes the share a of ssl into `matched`: its bound takes the measured |max| of the utterance's own ssl - one more
    // atomicMax slot per utterance behind the encoder's, zeroed with them - and becomes |1 - a| * (the index's bound) + |a| * that maximum.
    // A protect call (c.protect; c.alpha may be null = 0) is an alpha call whose share is per frame: share[column] = a + (1 - a) * (p * w) from the
    // f0 decoded here (run_frame_share behind the encoder), and its bound takes the larger factors of a and a + (1 - a) * p.
    const bool mixed = c.alpha || c.protect;
    const int nslots = mixed ? 4 : 3;
    float* emax = ws.get<float>((size_t)(2 + nslots) * NB);
    float* spec_bound = emax + NB;
    float* enc_slots = spec_bound + NB;      // the encoder's three atomicMax slots: zeroed by the energy stage's pooled-maximum launch
    float* srcmax = mixed ? enc_slots + 3 * NB : nullptr;
    float* abound = mixed ? ws.get<float>((size_t)NB) : nullptr;
    float* share = c.protect ? ws.get<float>((size_t)B * T) : nullptr;
    // one index per row: every utterance's matched-content bound is its own index's |max| (so its fp16-split scales, and its bits, are those
    // of its own B = 1 call), and its runs of query columns go to the search as segments; per-row pitch shifts travel like the lengths.
    // A blend (ix.M terms per row): the (term, row) runs over ix.M x the columns, term-major, and the bound is sum_m |w_m| * |max|_m.
    const int M = ix.M > 0 ? ix.M : 1;
    float* rowmax = ix.per_row ? ws.get<float>((size_t)NB) : nullptr;
    const bool auto_pitch = c.target_f0 != nullptr;      // the shifts come from the f0 this call decodes (run_pitch_match behind the encoder)
    float* rshift = ix.per_row && c.shifts && !auto_pitch ? ws.get<float>((size_t)NB) : nullptr;
    std::vector<KnnSegIn> segs;
    if (ix.per_row) {
        for (int m = 0; m < M; ++m)
            for (int i = 0; i < NB; ++i) {
                const int r = ctx->rag ? ctx->rag->row[i] : i;
                const int c0 = ctx->rag ? ctx->rag->pre[i] : i * T, nc = ctx->rag ? ctx->rag->tb[i] : T;
                segs.push_back(KnnSegIn{ix.blobs[(size_t)r * M + m], ix.Ns[(size_t)r * M + m], m * B * T + c0, nc});
            }
    } else {
        segs.push_back(KnnSegIn{ix.blob, ix.N, 0, B * T});
    }
    if (ix.per_row && !ws.dry) {
        std::vector<const float*> bl((size_t)NB * M);
        std::vector<int> sh(NB), rows(NB);
        for (int i = 0; i < NB; ++i) {
            const int r = ctx->rag ? ctx->rag->row[i] : i;
            rows[i] = r;
            for (int m = 0; m < M; ++m) bl[(size_t)i * M + m] = ix.blobs[(size_t)r * M + m];
            if (rshift) std::memcpy(&sh[i], &c.shifts[r], sizeof(int));
        }
        if (ix.M > 0) TVC_CHECK(run_knn_blend_bound(ctx, s, bl, rows, M, ix.weights, rowmax));
        else TVC_CHECK(run_knn_amax_rows(ctx, s, bl, rowmax));
        if (rshift) TVC_CHECK(upload_ints(ctx, s, sh, reinterpret_cast<int*>(rshift)));
    }
    size_t m = ws.mark();
    {
        ProfScope ps(ctx, s, ws, "stft");
        TVC_CHECK(run_stft(ctx, s, ws, c.wav, spec, B, L));
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "energy");
        TVC_CHECK(run_energy(ctx, s, ws, c.wav, energy, B, L, emax, spec_bound, enc_slots, nslots * NB));
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "encoder");
        // A path call (c.path) keeps the logits and decodes them again over each utterance as a whole (run_pitch_path: one workgroup per
        // utterance, its back-pointers in workspace that goes back with the encoder's): f0, and f0s unless a register decides the shift, are
        // the path's from here on - the tracker, the register, protect's voicing weight and the decoder read nothing else.
        float* lgt = c.path ? ws.get<float>((size_t)B * kPitchClasses * T) : nullptr;
        uint16_t* bp = c.path ? ws.get<uint16_t>((size_t)B * T * kPitchClasses) : nullptr;
        TVC_CHECK(run_encoder(ctx, s, ws, spec, ssl, f0, lgt, B, T, spec_bound, enc_slots, auto_pitch || c.path ? nullptr : f0s, c.shift, rshift));
        if (c.path && !ws.dry) {
            std::vector<PitchPathRow> rows((size_t)NB);
            for (int i = 0; i < NB; ++i) {
                const int r = ctx->rag ? ctx->rag->row[i] : i;
                rows[i] = PitchPathRow{ctx->rag ? ctx->rag->pre[i] : i * T, ctx->rag ? ctx->rag->tb[i] : T, ix.per_row && c.shifts ? c.shifts[r] : c.shift};
            }
            TVC_CHECK(run_pitch_path(ctx, s, lgt, T, rows, *c.path, bp, f0, auto_pitch ? nullptr : f0s, nullptr, nullptr, c.carry_frame, c.carry, c.carry));
        }
        if (c.track && !ws.dry) {      // one workgroup per stream: its history's register, the slew-limited shift, its shifted f0 (no workspace)
            TVC_CHECK(run_pitch_track(ctx, s, f0, B, T, *c.track, c.target_f0, c.shift, c.shifts, nullptr, nullptr, c.shift_out, f0s));
        } else if (auto_pitch && !ws.dry) {      // one workgroup per utterance: its register, its shift (offset = the host value), its shifted f0
            std::vector<PitchRow> rows((size_t)NB);
            for (int i = 0; i < NB; ++i) {
                const int r = ctx->rag ? ctx->rag->row[i] : i;
                rows[i] = PitchRow{ctx->rag ? ctx->rag->pre[i] : i * T, ctx->rag ? ctx->rag->tb[i] : T, r, c.shifts ? c.shifts[r] : c.shift};
            }
            TVC_CHECK(run_pitch_match(ctx, s, f0, rows, c.target_f0, nullptr, nullptr, c.shift_out, f0s));
        }
        if (c.protect && !ws.dry) TVC_CHECK(run_frame_share(ctx, s, f0, c.alpha, c.protect, share, B, T));      // from f0 itself, before any shift
    }
    ws.release(m);
    {
        ProfScope ps(ctx, s, ws, "knn");
        if (ix.M > 0) TVC_CHECK(run_knn_blend(ctx, s, ws, ssl, segs.data(), (int)segs.size(), ix.M, ix.weights, matched, nullptr, B, T, c.alpha, share));
        else TVC_CHECK(run_knn_segs(ctx, s, ws, ssl, segs.data(), (int)segs.size(), matched, nullptr, B, T, c.alpha, share));
    }
    ws.release(m);
    const float* idx_bound = ws.dry ? nullptr : (ix.per_row ? rowmax : blob_amax(ix.blob));
    if (mixed && !ws.dry) {
        TVC_CHECK(run_ssl_amax(ctx, s, ssl, B, T, srcmax));
        TVC_CHECK(run_knn_alpha_bound(ctx, s, c.alpha, idx_bound, ix.per_row ? 1 : 0, srcmax, abound, NB, c.protect));
    }
    TVC_CHECK(run_decoder(ctx, s, ws, matched, f0s, energy, c.angle, c.seed, c.wave, nullptr, nullptr, nullptr, B, T, mixed && !ws.dry ? abound : idx_bound, emax,
                          mixed || ix.per_row ? 1 : 0));
    ws.release(m);
    return 0;
}

// stands for a caller's buffer in a walk that only sizes the workspace (ws.dry: no pointer is dereferenced)
static float* const kDryPtr = (float*)(uintptr_t)256;

// behind the launching walk of an entry: it took no more workspace than its measuring walk (ws.dry) found
static int walks_agree(tvc_ctx* ctx, const char* entry, size_t real_peak, size_t measured) {
    return real_peak <= measured ? TVC_OK : fail(ctx, TVC_ERR_WORKSPACE, "%s: the launching walk took %zu workspace bytes, the measuring walk %zu", entry, real_peak, measured);
}

// Workspace is validated *before* launching: every entry walks its drivers twice, first with a Ws that only measures (ws.dry), then with the
// caller's workspace.  Both walks take the same allocations (tvc_common.h Ws); the host check behind the second one states it.
//   walk(Ws&) -> int        the entry's driver calls; called twice, so it must not change what it captures
//   granule                 the measured peak counts in whole granules: 1, or 4 KiB pages for the ragged entries (kRagGranule)
//   before_launch() -> int  (optional) runs once the workspace is known to suffice, in front of the launching walk
// A refused call has launched nothing: the measuring walk launches nothing, and before_launch runs behind the size check.
// (Function templates over the callables, no std::function: this is the host time of a B = 1 call.)
static size_t whole_granules(size_t bytes, size_t granule) { return (bytes + granule - 1) / granule * granule; }
template <class Walk, class Step>
static int run_walks(tvc_ctx* ctx, const char* entry, void* wsp, size_t ws_bytes, size_t granule, Walk&& walk, Step&& before_launch) {
    Ws need(nullptr, 0, true);
    TVC_CHECK(walk(need));
    const size_t bytes = whole_granules(need.peak, granule);
    if (bytes > ws_bytes) return fail(ctx, TVC_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", bytes, ws_bytes);
    TVC_CHECK(before_launch());
    Ws ws(wsp, bytes, false);
    TVC_CHECK(walk(ws));
    return walks_agree(ctx, entry, ws.peak, need.peak);
}
template <class Walk>
static int run_walks(tvc_ctx* ctx, const char* entry, void* wsp, size_t ws_bytes, size_t granule, Walk&& walk) {
    return run_walks(ctx, entry, wsp, ws_bytes, granule, walk, [] { return 0; });
}
// the measuring walk alone, for the tvc_workspace_bytes* queries: the same granules, and 4096 bytes on top of the peak
template <class Walk>
static int measure(size_t granule, size_t* out_bytes, Walk&& walk) {
    Ws ws(nullptr, 0, true);
    TVC_CHECK(walk(ws));
    *out_bytes = whole_granules(ws.peak, granule) + 4096;
    return TVC_OK;
}
constexpr size_t kRagGranule = 4096;

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

// ---- conversion: one index or one per row, rows of equal length or ragged --------------------------------------------------------------
// A table of indices is checked whole before anything is enqueued: every entry non-null, N >= 4, and the blob_check of the single-index calls.
static int rows_check(tvc_ctx* ctx, hipStream_t s, int B, const float* const* prepared, const int64_t* N, const char* what) {
    if (!prepared || !N) return fail(ctx, TVC_ERR_ARG, "%s: prepared and N are host arrays of B entries", what);
    for (int b = 0; b < B; ++b) {
        if (!prepared[b]) return fail(ctx, TVC_ERR_ARG, "%s: prepared[%d] is NULL", what, b);
        if (N[b] < 4) return fail(ctx, TVC_ERR_ARG, "%s: N[%d] = %lld: an index needs at least k=4 vectors", what, b, (long long)N[b]);
    }
    for (int b = 0; b < B; ++b) TVC_CHECK(blob_check(ctx, s, prepared[b], N[b], what));
    return 0;
}

// a blend's own arguments: 1 .. TVC_BLEND_MAX terms per row, the device weights, tables that 32-bit column numbers can address
static int blend_check(tvc_ctx* ctx, int B, int M, const float* weights, const char* what) {
    if (M < 1 || M > TVC_BLEND_MAX) return fail(ctx, TVC_ERR_ARG, "%s: M = %d terms per row; a blend takes 1 ... %d", what, M, TVC_BLEND_MAX);
    if (!weights) return fail(ctx, TVC_ERR_ARG, "%s: weights is NULL (a device array of B * M floats)", what);
    if (B <= 0 || (int64_t)B * M > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    return 0;
}

// The tvc_convert*_f32 entries: the checks under the entry's own name `what`, then the two walks.  ragged: c.lens holds every row's
// own length and c.L is Lmax; the call runs as the batches of ragged_split and the padded output is cleared once in front of them.
static int convert_entry(tvc_ctx* ctx, void* stream, const ConvertCall& c, bool ragged, void* wsp, size_t ws_bytes, const char* what) {
    TVC_CHECK(need_ready(ctx, NEED_ENC | NEED_DEC));
    hipStream_t s = (hipStream_t)stream;
    const ConvertIndex& ix = c.index;
    if (!c.wav || !c.wave || (ragged && !c.lens) || (!ix.per_row && !ix.blob) || c.B <= 0 || c.L <= 0 || c.L % kHop)
        return fail(ctx, TVC_ERR_ARG, "%s: bad argument (%s must be a positive multiple of 480)", what, ragged ? "Lmax" : "L");
    if (!ragged && c.L < kNfft / 2 + 1) return fail(ctx, TVC_ERR_ARG, "%s: L must exceed 960 samples (STFT reflect padding, as torch.stft requires)", what);
    if (ix.weights || ix.M) TVC_CHECK(blend_check(ctx, c.B, ix.M, ix.weights, what));
    if (ix.per_row) {
        TVC_CHECK(rows_check(ctx, s, c.B * (ix.M > 0 ? ix.M : 1), ix.blobs, ix.Ns, what));
    } else {
        if (ix.N < 4) return fail(ctx, TVC_ERR_ARG, "%s: index needs at least k=4 vectors", what);
        TVC_CHECK(blob_check(ctx, s, ix.blob, ix.N, what));
    }
    if (ix.M > 0 && (int64_t)c.B * ix.M * (c.L / kHop) > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: more than 2^31 - 1 query columns", what);
    TVC_CHECK(draw_under_capture(ctx, s, c.angle, what));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    if (!ragged) return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) { return convert_impl(ctx, s, ws, c); });
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, c.B, c.L, c.lens, &batches));
    return run_walks(
        ctx, what, wsp, ws_bytes, kRagGranule, [&](Ws& ws) { return convert_ragged_batches(ctx, s, ws, batches, c); },      // (the measuring walk is host time on the launch path)
        [&] {      // the whole padded output is cleared once: every kernel writes its utterance's own samples only
            TVC_HIP(ctx, hipMemsetAsync(c.wave, 0, (size_t)c.B * c.L * sizeof(float), s));
            return 0;
        });
}

// The tvc_workspace_bytes* query that goes with each of them: the same description with stand-in buffers, the measuring walk alone.  A
// per-row index (ix.Ns; ix.blobs is not looked at) is planned with every row a segment of its own (distinct stand-in blobs) and a shift
// table (it takes workspace; never read in this walk): a call whose rows share blobs, or without per-row shifts, needs less.
// (No allocation depends on whether the call brings its own noise phases.)
static int convert_query(tvc_ctx* ctx, int B, int64_t L, const int64_t* lens, bool ragged, const ConvertIndex& ix, size_t* out_bytes, const char* what,
                         bool auto_pitch = false, bool alpha = false, bool protect = false, bool path = false) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    if (!out_bytes || (ragged && !lens) || (ix.per_row ? !ix.Ns : ix.N < 4) || B <= 0 || L <= 0 || L % kHop != 0)
        return fail(ctx, TVC_ERR_ARG, "%s: need B>0, %s%%480==0, %s%s", what, ragged ? "Lmax" : "L", ragged && ix.per_row ? "lens[B], " : "", ix.per_row ? "N[B]" : "N>=4");
    if (ix.M) TVC_CHECK(blend_check(ctx, B, ix.M, kDryPtr, what));
    const int M = ix.M > 0 ? ix.M : 1;
    if (!ragged && (int64_t)B * M * (L / kHop) > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: more than 2^31 - 1 query columns", what);
    for (int b = 0; ix.per_row && b < B * M; ++b)
        if (ix.Ns[b] < 4) return fail(ctx, TVC_ERR_ARG, "%s: N[%d] < 4", what, b);
    std::vector<const float*> blobs(ix.per_row ? (size_t)B * M : 0);
    for (size_t b = 0; b < blobs.size(); ++b) blobs[b] = kDryPtr + 64 * b;
    const float shift = 0.f;
    ConvertCall c;
    c.wav = c.wave = kDryPtr;
    c.B = B;
    c.L = L;
    c.lens = lens;
    c.index = ix.M ? ConvertIndex::blend(blobs.data(), ix.Ns, ix.M, kDryPtr) : ix.per_row ? ConvertIndex::table(blobs.data(), ix.Ns) : ConvertIndex::one(kDryPtr, ix.N);
    c.shifts = ix.per_row ? &shift : nullptr;
    c.target_f0 = auto_pitch ? kDryPtr : nullptr;
    c.alpha = alpha ? kDryPtr : nullptr;
    c.protect = protect ? kDryPtr : nullptr;
    const tvc_pitch_path any_path = TVC_PITCH_PATH_DEFAULT;      // the settings take no part in the sizes
    c.path = path ? &any_path : nullptr;
    if (!ragged) return measure(1, out_bytes, [&](Ws& ws) { return convert_impl(ctx, nullptr, ws, c); });
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, L, lens, &batches));
    return measure(kRagGranule, out_bytes, [&](Ws& ws) { return convert_ragged_batches(ctx, nullptr, ws, batches, c); });
}

int tvc_workspace_bytes(tvc_ctx* ctx, int B, int64_t L, int64_t N, size_t* out_bytes) {
    return convert_query(ctx, B, L, nullptr, false, ConvertIndex::one(nullptr, N), out_bytes, "tvc_workspace_bytes");
}
int tvc_workspace_bytes_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, int64_t N, size_t* out_bytes) {
    return convert_query(ctx, B, Lmax, lens, true, ConvertIndex::one(nullptr, N), out_bytes, "tvc_workspace_bytes_ragged");
}
int tvc_workspace_bytes_multi(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, size_t* out_bytes) {
    return convert_query(ctx, B, L, nullptr, false, ConvertIndex::table(nullptr, N), out_bytes, "tvc_workspace_bytes_multi");
}
int tvc_workspace_bytes_ragged_multi(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, size_t* out_bytes) {
    return convert_query(ctx, B, Lmax, lens, true, ConvertIndex::table(nullptr, N), out_bytes, "tvc_workspace_bytes_ragged_multi");
}

int tvc_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* prepared, int64_t N,
                    float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L,
                    void* wsp, size_t ws_bytes) {
    const ConvertCall c{wav, wave, B, L, nullptr, ConvertIndex::one(prepared, N), pitch_shift, nullptr, noise_angle, seed};
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, "tvc_convert_f32");
}
int tvc_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* prepared, int64_t N,
                           float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    const ConvertCall c{wav, wave, B, Lmax, lens, ConvertIndex::one(prepared, N), pitch_shift, nullptr, noise_angle, seed};
    return convert_entry(ctx, stream, c, true, wsp, ws_bytes, "tvc_convert_ragged_f32");
}
int tvc_convert_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, float pitch_shift,
                          const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    const ConvertCall c{wav, wave, B, L, nullptr, ConvertIndex::table(prepared, N), pitch_shift, pitch_shifts, noise_angle, seed};
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, "tvc_convert_multi_f32");
}
int tvc_convert_ragged_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave,
                                 int B, void* wsp, size_t ws_bytes) {
    const ConvertCall c{wav, wave, B, Lmax, lens, ConvertIndex::table(prepared, N), pitch_shift, pitch_shifts, noise_angle, seed};
    return convert_entry(ctx, stream, c, true, wsp, ws_bytes, "tvc_convert_ragged_multi_f32");
}

// the stage calls' share per column: with protect set, B * T floats of workspace (both walks) filled from the caller's f0 [B][T] in front of the search
static int match_share(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* f0, const float* alpha, const float* protect, int B, int T, float** share) {
    *share = protect ? ws.get<float>((size_t)B * T) : nullptr;
    if (protect && !ws.dry) TVC_CHECK(run_frame_share(ctx, s, f0, alpha, protect, *share, B, T));
    return 0;
}
// the match against one index per row, under the entry's own name `what`; alpha (nullable): the alpha form of the same call; protect
// (nullable, with f0): its protect form
static int match_table(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, const float* alpha, float* out,
                       int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes, const char* what, const float* f0 = nullptr, const float* protect = nullptr) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !out || B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B, prepared, N, what));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KnnSegIn> in((size_t)B);
    for (int b = 0; b < B; ++b) in[b] = KnnSegIn{prepared[b], N[b], b * T, T};
    return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) {
        float* share;
        TVC_CHECK(match_share(ctx, s, ws, f0, alpha, protect, B, T, &share));
        return run_knn_segs(ctx, s, ws, src, in.data(), B, out, idx_out, B, T, alpha, share);
    });
}
int tvc_knn_match_multi_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, float* out,
                            int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    return match_table(ctx, stream, src, prepared, N, nullptr, out, idx_out, B, T, wsp, ws_bytes, "tvc_knn_match_multi_f32");
}

// ---- a weighted blend of several indices per row ------------------------------------------------------------------------------------------
int tvc_workspace_bytes_blend(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, "tvc_workspace_bytes_blend"));
    return convert_query(ctx, B, L, nullptr, false, ConvertIndex::blend(nullptr, N, M, nullptr), out_bytes, "tvc_workspace_bytes_blend");
}
int tvc_workspace_bytes_ragged_blend(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, "tvc_workspace_bytes_ragged_blend"));
    return convert_query(ctx, B, Lmax, lens, true, ConvertIndex::blend(nullptr, N, M, nullptr), out_bytes, "tvc_workspace_bytes_ragged_blend");
}
int tvc_convert_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp,
                          size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, weights, "tvc_convert_blend_f32"));
    const ConvertCall c{wav, wave, B, L, nullptr, ConvertIndex::blend(prepared, N, M, weights), pitch_shift, pitch_shifts, noise_angle, seed};
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, "tvc_convert_blend_f32");
}
int tvc_convert_ragged_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, int M, const float* weights, float pitch_shift, const float* pitch_shifts, const float* noise_angle,
                                 uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, weights, "tvc_convert_ragged_blend_f32"));
    const ConvertCall c{wav, wave, B, Lmax, lens, ConvertIndex::blend(prepared, N, M, weights), pitch_shift, pitch_shifts, noise_angle, seed};
    return convert_entry(ctx, stream, c, true, wsp, ws_bytes, "tvc_convert_ragged_blend_f32");
}

// ---- automatic pitch: the shift that moves a row's register onto its target's, found on the device ------------------------------------------
int tvc_pitch_match_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, int rows, const float* target_f0, float pitch_shift,
                        const float* pitch_shifts, float* median_out, int32_t* voiced_out, float* shift_out, float* f0_shifted) {
    if (!ctx) return TVC_ERR_ARG;
    if (!f0 || !row_start || rows <= 0 || (!median_out && !voiced_out && !shift_out && !f0_shifted)) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_match_f32: bad argument");
    if (row_start[0] < 0 || row_start[rows] > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_match_f32: row_start beyond 32-bit indexing");
    std::vector<PitchRow> pr((size_t)rows);
    for (int b = 0; b < rows; ++b) {
        if (row_start[b + 1] < row_start[b]) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_match_f32: row_start[%d] > row_start[%d] (rows + 1 ascending column numbers)", b, b + 1);
        pr[b] = PitchRow{(int)row_start[b], (int)(row_start[b + 1] - row_start[b]), b, pitch_shifts ? pitch_shifts[b] : pitch_shift};
    }
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_match(ctx, (hipStream_t)stream, f0, pr, target_f0, median_out, voiced_out, shift_out, f0_shifted);
}

// the table form of the blend entries: weights == NULL is the multi-index call and takes M = 1
static int auto_index(tvc_ctx* ctx, int B, const float* const* prepared, const int64_t* N, int M, const float* weights, ConvertIndex* ix, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    if (!weights) {
        if (M != 1) return fail(ctx, TVC_ERR_ARG, "%s: weights = NULL is one index per row: M must be 1, got %d", what, M);
        *ix = ConvertIndex::table(prepared, N);
        return 0;
    }
    TVC_CHECK(blend_check(ctx, B, M, weights, what));
    *ix = ConvertIndex::blend(prepared, N, M, weights);
    return 0;
}
// M = 1 may come with weights (a one-term blend) or without (the multi-index call): the query covers both
static int auto_query(tvc_ctx* ctx, int B, int64_t L, const int64_t* lens, bool ragged, const int64_t* N, int M, size_t* out_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, what));
    TVC_CHECK(convert_query(ctx, B, L, lens, ragged, ConvertIndex::blend(nullptr, N, M, nullptr), out_bytes, what, true));
    if (M == 1) {
        size_t table = 0;
        TVC_CHECK(convert_query(ctx, B, L, lens, ragged, ConvertIndex::table(nullptr, N), &table, what, true));
        if (table > *out_bytes) *out_bytes = table;
    }
    return TVC_OK;
}
int tvc_workspace_bytes_auto(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    return auto_query(ctx, B, L, nullptr, false, N, M, out_bytes, "tvc_workspace_bytes_auto");
}
int tvc_workspace_bytes_ragged_auto(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    return auto_query(ctx, B, Lmax, lens, true, N, M, out_bytes, "tvc_workspace_bytes_ragged_auto");
}
int tvc_convert_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                         const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                         float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertIndex ix;
    TVC_CHECK(auto_index(ctx, B, prepared, N, M, weights, &ix, "tvc_convert_auto_f32"));
    if (!target_f0) return fail(ctx, TVC_ERR_ARG, "tvc_convert_auto_f32: target_f0 is NULL (a device array of B registers in Hz)");
    const ConvertCall c{wav, wave, B, L, nullptr, ix, pitch_shift, pitch_shifts, noise_angle, seed, target_f0, shift_out};
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, "tvc_convert_auto_f32");
}
int tvc_convert_ragged_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                const int64_t* N, int M, const float* weights, const float* target_f0, float pitch_shift, const float* pitch_shifts,
                                float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertIndex ix;
    TVC_CHECK(auto_index(ctx, B, prepared, N, M, weights, &ix, "tvc_convert_ragged_auto_f32"));
    if (!target_f0) return fail(ctx, TVC_ERR_ARG, "tvc_convert_ragged_auto_f32: target_f0 is NULL (a device array of B registers in Hz)");
    const ConvertCall c{wav, wave, B, Lmax, lens, ix, pitch_shift, pitch_shifts, noise_angle, seed, target_f0, shift_out};
    return convert_entry(ctx, stream, c, true, wsp, ws_bytes, "tvc_convert_ragged_auto_f32");
}

// ---- automatic pitch in streams: the register is the stream's history (a ring per stream on the device) ---------------------------------------
// every host value of a tracker call, checked under the entry's own name before any device work
static int track_check(tvc_ctx* ctx, int S, int T, const PitchTrackState& t, const float* target_f0, const char* what) {
    if (S <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "%s: S = %d streams of T = %d frames", what, S, T);
    if (!target_f0) return fail(ctx, TVC_ERR_ARG, "%s: target_f0 is NULL (a device array of S registers in Hz)", what);
    if (!t.ring || !t.count || !t.autos) return fail(ctx, TVC_ERR_ARG, "%s: the tracker state (ring [S][W], count [S], auto [S]) has a NULL pointer", what);
    if (t.W < 1 || t.W > TVC_PITCH_TRACK_MAX_WINDOW) return fail(ctx, TVC_ERR_ARG, "%s: W = %d; a ring holds 1 ... %d frames", what, t.W, TVC_PITCH_TRACK_MAX_WINDOW);
    if (t.n < 0 || t.n > 256) return fail(ctx, TVC_ERR_ARG, "%s: n = %d new frames; a block brings 0 ... 256", what, t.n);
    if (t.start < 0 || (int64_t)t.start + t.n > T) return fail(ctx, TVC_ERR_ARG, "%s: columns [%d, %d + %d) do not lie within T = %d", what, t.start, t.start, t.n, T);
    if (t.min_voiced < 1) return fail(ctx, TVC_ERR_ARG, "%s: min_voiced = %d; at least 1", what, t.min_voiced);
    if (!(t.slew >= 0.f)) return fail(ctx, TVC_ERR_ARG, "%s: slew must be >= 0 semitones per call (+inf: no limit)", what);
    return 0;
}
int tvc_pitch_track_f32(tvc_ctx* ctx, void* stream, const float* f0, int S, int T, int start, int n, const float* target_f0, float pitch_shift,
                        const float* pitch_shifts, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float* median_out,
                        int64_t* count_out, float* shift_out, float* f0_shifted) {
    if (!ctx) return TVC_ERR_ARG;
    if (!f0) return fail(ctx, TVC_ERR_ARG, "tvc_pitch_track_f32: f0 is NULL");
    const PitchTrackState t{start, n, W, min_voiced, slew, ring, count, auto_shift};
    TVC_CHECK(track_check(ctx, S, T, t, target_f0, "tvc_pitch_track_f32"));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_track(ctx, (hipStream_t)stream, f0, S, T, t, target_f0, pitch_shift, pitch_shifts, median_out, count_out, shift_out, f0_shifted);
}
int tvc_convert_track_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift,
                          float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B,
                          int64_t L, void* wsp, size_t ws_bytes) {
    ConvertIndex ix;
    TVC_CHECK(auto_index(ctx, B, prepared, N, M, weights, &ix, "tvc_convert_track_f32"));
    const PitchTrackState t{start, n, W, min_voiced, slew, ring, count, auto_shift};
    if (L <= 0 || L / kHop > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "tvc_convert_track_f32: bad argument (L must be a positive multiple of 480)");
    TVC_CHECK(track_check(ctx, B, (int)(L / kHop), t, target_f0, "tvc_convert_track_f32"));
    ConvertCall c{wav, wave, B, L, nullptr, ix, pitch_shift, pitch_shifts, noise_angle, seed, target_f0, shift_out};
    c.track = &t;
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, "tvc_convert_track_f32");
}

// the match against a blend, under the entry's own name `what`; alpha (nullable): the alpha form of the same call; protect (nullable, with f0): its protect form
static int match_blend(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M, const float* weights,
                       const float* alpha, float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes, const char* what, const float* f0 = nullptr,
                       const float* protect = nullptr) {
    if (!ctx) return TVC_ERR_ARG;
    if (!src || !out || B <= 0 || T <= 0) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    TVC_CHECK(blend_check(ctx, B, M, weights, what));
    if ((int64_t)B * M * T > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: more than 2^31 - 1 query columns", what);
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B * M, prepared, N, what));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KnnSegIn> in;
    for (int m = 0; m < M; ++m)
        for (int b = 0; b < B; ++b) in.push_back(KnnSegIn{prepared[(size_t)b * M + m], N[(size_t)b * M + m], (m * B + b) * T, T});
    return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) {
        float* share;
        TVC_CHECK(match_share(ctx, s, ws, f0, alpha, protect, B, T, &share));
        return run_knn_blend(ctx, s, ws, src, in.data(), (int)in.size(), M, weights, out, idx_out, B, T, alpha, share);
    });
}
int tvc_knn_match_blend_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    return match_blend(ctx, stream, src, prepared, N, M, weights, nullptr, out, idx_out, B, T, wsp, ws_bytes, "tvc_knn_match_blend_f32");
}

// ---- alpha: a share of the source's own content features kept in the match (the reference's match_features(..., alpha)) ---------------------
// The table form of the auto entries plus `alpha` (device, one fp32 per row); alpha == NULL is the sibling call.  One ConvertCall field and one
// argument of the kNN drivers: no second path.
static int alpha_query(tvc_ctx* ctx, int B, int64_t L, const int64_t* lens, bool ragged, const int64_t* N, int M, size_t* out_bytes, const char* what,
                       bool protect = false, bool path = false) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, what));
    size_t most = 0;
    for (int auto_pitch = 0; auto_pitch < 2; ++auto_pitch)      // with and without target registers, as a blend and (M = 1) as a table: the largest
        for (int table = 0; table < (M == 1 ? 2 : 1); ++table) {
            size_t bytes = 0;
            TVC_CHECK(convert_query(ctx, B, L, lens, ragged, table ? ConvertIndex::table(nullptr, N) : ConvertIndex::blend(nullptr, N, M, nullptr), &bytes, what,
                                    auto_pitch != 0, true, protect, path));
            if (bytes > most) most = bytes;
        }
    *out_bytes = most;
    return TVC_OK;
}
int tvc_workspace_bytes_alpha(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, L, nullptr, false, N, M, out_bytes, "tvc_workspace_bytes_alpha");
}
int tvc_workspace_bytes_ragged_alpha(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, Lmax, lens, true, N, M, out_bytes, "tvc_workspace_bytes_ragged_alpha");
}
// a call's path settings (nullable: no path), refused under the entry's own name `what` before any device work
static int path_check(tvc_ctx* ctx, const tvc_pitch_path* path, const char* what) {
    char why[96];
    if (path && pitch_path_check(*path, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "%s: path: %s", what, why);
    return 0;
}
// the alpha, the protect and the path entries share their bodies: protect == nullptr is the alpha call, path == nullptr the protect call, under
// the entry's own name `what`
static int convert_alpha(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                         const float* alpha, const float* protect, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring,
                         int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                         uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes, const char* what, const tvc_pitch_path* path = nullptr,
                         int carry_frame = 0, float* carry = nullptr) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(path_check(ctx, path, what));
    if (carry) {      // the path's state from block to block: refused here, before any device work
        if (!path) return fail(ctx, TVC_ERR_ARG, "%s: carry needs path (the state is the pitch path's)", what);
        if (carry_frame < 1 || L / kHop <= carry_frame)
            return fail(ctx, TVC_ERR_ARG, "%s: carry_frame = %d must be >= 1 and below the window's %lld frames", what, carry_frame, (long long)(L / kHop));
    }
    ConvertIndex ix;
    TVC_CHECK(auto_index(ctx, B, prepared, N, M, weights, &ix, what));
    ConvertCall c{wav, wave, B, L, nullptr, ix, pitch_shift, pitch_shifts, noise_angle, seed, target_f0, target_f0 ? shift_out : nullptr};
    c.alpha = alpha;
    c.protect = protect;
    c.path = path;
    c.carry_frame = carry ? carry_frame : 0;
    c.carry = carry;
    const PitchTrackState t{start, n, W, min_voiced, slew, ring, count, auto_shift};
    if (ring) {      // a tracker: tvc_convert_track_f32's checks
        if (L <= 0 || L / kHop > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: bad argument (L must be a positive multiple of 480)", what);
        TVC_CHECK(track_check(ctx, B, (int)(L / kHop), t, target_f0, what));
        c.track = &t;
    }
    return convert_entry(ctx, stream, c, false, wsp, ws_bytes, what);
}
static int convert_ragged_alpha(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const float* target_f0,
                                float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B,
                                void* wsp, size_t ws_bytes, const char* what, const tvc_pitch_path* path = nullptr) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(path_check(ctx, path, what));
    ConvertIndex ix;
    TVC_CHECK(auto_index(ctx, B, prepared, N, M, weights, &ix, what));
    ConvertCall c{wav, wave, B, Lmax, lens, ix, pitch_shift, pitch_shifts, noise_angle, seed, target_f0, target_f0 ? shift_out : nullptr};
    c.alpha = alpha;
    c.protect = protect;
    c.path = path;
    return convert_entry(ctx, stream, c, true, wsp, ws_bytes, what);
}
static int match_alpha(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N, int M,
                       const float* weights, const float* alpha, const float* protect, float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes,
                       const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    if ((alpha || protect) && src && src == out)
        return fail(ctx, TVC_ERR_ARG, "%s: out must be another buffer than src (the source's share is read while out is written)", what);
    if (protect && !f0) return fail(ctx, TVC_ERR_ARG, "%s: protect needs f0 (device, [B][T]: the voicing comes from it)", what);
    if (weights) return match_blend(ctx, stream, src, prepared, N, M, weights, alpha, out, idx_out, B, T, wsp, ws_bytes, what, f0, protect);
    if (M != 1) return fail(ctx, TVC_ERR_ARG, "%s: weights = NULL is one index per row: M must be 1, got %d", what, M);
    return match_table(ctx, stream, src, prepared, N, alpha, out, idx_out, B, T, wsp, ws_bytes, what, f0, protect);
}
int tvc_convert_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* alpha, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count,
                          float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                          float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    return convert_alpha(ctx, stream, wav, prepared, N, M, weights, alpha, nullptr, target_f0, start, n, W, min_voiced, slew, ring, count, auto_shift, pitch_shift,
                         pitch_shifts, shift_out, noise_angle, seed, wave, B, L, wsp, ws_bytes, "tvc_convert_alpha_f32");
}
int tvc_convert_ragged_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, int M, const float* weights, const float* alpha, const float* target_f0, float pitch_shift,
                                 const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp,
                                 size_t ws_bytes) {
    return convert_ragged_alpha(ctx, stream, wav, Lmax, lens, prepared, N, M, weights, alpha, nullptr, target_f0, pitch_shift, pitch_shifts, shift_out, noise_angle,
                                seed, wave, B, wsp, ws_bytes, "tvc_convert_ragged_alpha_f32");
}
int tvc_knn_match_alpha_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            const float* alpha, float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    return match_alpha(ctx, stream, src, nullptr, prepared, N, M, weights, alpha, nullptr, out, idx_out, B, T, wsp, ws_bytes, "tvc_knn_match_alpha_f32");
}

// ---- protect: the alpha entries with a per-frame share - more of the source on the unvoiced frames of the f0 the call decodes --------------
// `protect` (device, one fp32 per row) behind alpha; protect == NULL is the alpha call, launch for launch; alpha == NULL with protect set: a = 0.
int tvc_workspace_bytes_protect(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, L, nullptr, false, N, M, out_bytes, "tvc_workspace_bytes_protect", true);
}
int tvc_workspace_bytes_ragged_protect(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, Lmax, lens, true, N, M, out_bytes, "tvc_workspace_bytes_ragged_protect", true);
}
int tvc_convert_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            const float* alpha, const float* protect, const float* target_f0, int start, int n, int W, int min_voiced, float slew,
                            float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                            const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    return convert_alpha(ctx, stream, wav, prepared, N, M, weights, alpha, protect, target_f0, start, n, W, min_voiced, slew, ring, count, auto_shift, pitch_shift,
                         pitch_shifts, shift_out, noise_angle, seed, wave, B, L, wsp, ws_bytes, "tvc_convert_protect_f32");
}
int tvc_convert_ragged_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                   const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const float* target_f0,
                                   float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave,
                                   int B, void* wsp, size_t ws_bytes) {
    return convert_ragged_alpha(ctx, stream, wav, Lmax, lens, prepared, N, M, weights, alpha, protect, target_f0, pitch_shift, pitch_shifts, shift_out, noise_angle,
                                seed, wave, B, wsp, ws_bytes, "tvc_convert_ragged_protect_f32");
}
int tvc_knn_match_protect_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N, int M,
                              const float* weights, const float* alpha, const float* protect, float* out, int64_t* idx_out, int B, int T, void* wsp,
                              size_t ws_bytes) {
    return match_alpha(ctx, stream, src, f0, prepared, N, M, weights, alpha, protect, out, idx_out, B, T, wsp, ws_bytes, "tvc_knn_match_protect_f32");
}

// ---- the pitch path: the protect entries with the Viterbi decode of the call's own logits in the per-frame decode's place ------------------
// `path` (host settings) behind protect; path == NULL is the protect call, launch for launch.
int tvc_workspace_bytes_path(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, L, nullptr, false, N, M, out_bytes, "tvc_workspace_bytes_path", true, true);
}
int tvc_workspace_bytes_ragged_path(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    return alpha_query(ctx, B, Lmax, lens, true, N, M, out_bytes, "tvc_workspace_bytes_ragged_path", true, true);
}
int tvc_convert_path_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                         const float* alpha, const float* protect, const tvc_pitch_path* path, const float* target_f0, int start, int n, int W,
                         int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts,
                         float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    return convert_alpha(ctx, stream, wav, prepared, N, M, weights, alpha, protect, target_f0, start, n, W, min_voiced, slew, ring, count, auto_shift, pitch_shift,
                         pitch_shifts, shift_out, noise_angle, seed, wave, B, L, wsp, ws_bytes, "tvc_convert_path_f32", path);
}
int tvc_convert_ragged_path_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path,
                                const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                                uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    return convert_ragged_alpha(ctx, stream, wav, Lmax, lens, prepared, N, M, weights, alpha, protect, target_f0, pitch_shift, pitch_shifts, shift_out, noise_angle,
                                seed, wave, B, wsp, ws_bytes, "tvc_convert_ragged_path_f32", path);
}
// the carry: the path entry with the path's state [B][512] on the device, read at frame 0 and written at frame carry_frame, in place.  Equal
// lengths only (streams advance in lock step); carry == NULL is the path call, launch for launch.  Workspace: tvc_workspace_bytes_path.
int tvc_convert_carry_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* alpha, const float* protect, const tvc_pitch_path* path, int carry_frame, float* carry, const float* target_f0,
                          int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift,
                          const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp,
                          size_t ws_bytes) {
    return convert_alpha(ctx, stream, wav, prepared, N, M, weights, alpha, protect, target_f0, start, n, W, min_voiced, slew, ring, count, auto_shift, pitch_shift,
                         pitch_shifts, shift_out, noise_angle, seed, wave, B, L, wsp, ws_bytes, "tvc_convert_carry_f32", path, carry_frame, carry);
}
// the stage call's rows, checked on the host: ascending, apart, inside 32-bit indexing and inside one run of class_stride columns each
static int path_rows(tvc_ctx* ctx, const int64_t* row_start, const int64_t* row_count, int rows, int64_t S, int64_t* span, const char* what) {
    if (!row_start || !row_count || rows <= 0) return fail(ctx, TVC_ERR_ARG, "%s: bad argument (row_start, row_count and rows > 0)", what);
    int64_t end = 0;
    for (int b = 0; b < rows; ++b) {
        if (row_start[b] < end || row_count[b] < 0 || row_start[b] + row_count[b] > 0x7fffffff)
            return fail(ctx, TVC_ERR_ARG, "%s: row %d = [%lld, +%lld) must begin at or behind the row before it and end below 2^31", what, b, (long long)row_start[b],
                        (long long)row_count[b]);
        if (S > 0 && row_count[b] > 0 && row_start[b] / S != (row_start[b] + row_count[b] - 1) / S)
            return fail(ctx, TVC_ERR_ARG, "%s: row %d = [%lld, +%lld) straddles a multiple of class_stride = %lld", what, b, (long long)row_start[b],
                        (long long)row_count[b], (long long)S);
        end = row_start[b] + row_count[b];
    }
    *span = end;
    return 0;
}
int tvc_workspace_bytes_pitch_path(tvc_ctx* ctx, const int64_t* row_start, const int64_t* row_count, int rows, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    int64_t span = 0;
    if (!out_bytes) return fail(ctx, TVC_ERR_ARG, "tvc_workspace_bytes_pitch_path: bad argument");
    TVC_CHECK(path_rows(ctx, row_start, row_count, rows, 0, &span, "tvc_workspace_bytes_pitch_path"));
    return measure(1, out_bytes, [&](Ws& ws) { ws.get<uint16_t>(pitch_path_ws_bytes(span) / sizeof(uint16_t)); return 0; });
}
// the stage call and its carried form share their body: prior == carry_out == nullptr is the call as it was, under the entry's own name `what`
static int pitch_path_entry(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows, int64_t class_stride,
                            const tvc_pitch_path* path, int carry_frame, const float* prior, float* carry_out, float pitch_shift, const float* pitch_shifts,
                            float* f0, float* f0_shifted, int32_t* path_out, float* score_out, void* wsp, size_t ws_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    if (!logits || !path || class_stride <= 0 || class_stride > 0x7fffffff || (!f0 && !f0_shifted && !path_out && !score_out && !carry_out))
        return fail(ctx, TVC_ERR_ARG, "%s: bad argument (logits, path, 0 < class_stride < 2^31 and at least one output)", what);
    TVC_CHECK(path_check(ctx, path, what));
    int64_t span = 0;
    TVC_CHECK(path_rows(ctx, row_start, row_count, rows, class_stride, &span, what));
    if (carry_out) {      // frame h must exist in every row that runs
        if (carry_frame < 1) return fail(ctx, TVC_ERR_ARG, "%s: carry_frame = %d must be >= 1", what, carry_frame);
        for (int b = 0; b < rows; ++b)
            if (row_count[b] > 0 && row_count[b] <= carry_frame)
                return fail(ctx, TVC_ERR_ARG, "%s: row %d has %lld frames: carry_out takes frame carry_frame = %d, so every non-empty row needs more", what, b,
                            (long long)row_count[b], carry_frame);
    }
    std::vector<PitchPathRow> rw((size_t)rows);
    for (int b = 0; b < rows; ++b) rw[b] = PitchPathRow{(int)row_start[b], (int)row_count[b], pitch_shifts ? pitch_shifts[b] : pitch_shift};
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) {
        uint16_t* bp = ws.get<uint16_t>(pitch_path_ws_bytes(span) / sizeof(uint16_t));
        if (ws.dry) return 0;
        return run_pitch_path(ctx, (hipStream_t)stream, logits, (long)class_stride, rw, *path, bp, f0, f0_shifted, path_out, score_out, carry_frame, prior,
                              carry_out);
    });
}
int tvc_pitch_path_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows, int64_t class_stride,
                       const tvc_pitch_path* path, float pitch_shift, const float* pitch_shifts, float* f0, float* f0_shifted, int32_t* path_out,
                       float* score_out, void* wsp, size_t ws_bytes) {
    return pitch_path_entry(ctx, stream, logits, row_start, row_count, rows, class_stride, path, 0, nullptr, nullptr, pitch_shift, pitch_shifts, f0, f0_shifted,
                            path_out, score_out, wsp, ws_bytes, "tvc_pitch_path_f32");
}
int tvc_pitch_path_carry_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows,
                             int64_t class_stride, const tvc_pitch_path* path, int carry_frame, const float* prior, float* carry_out, float pitch_shift,
                             const float* pitch_shifts, float* f0, float* f0_shifted, int32_t* path_out, float* score_out, void* wsp, size_t ws_bytes) {
    return pitch_path_entry(ctx, stream, logits, row_start, row_count, rows, class_stride, path, carry_frame, prior, carry_out, pitch_shift, pitch_shifts, f0,
                            f0_shifted, path_out, score_out, wsp, ws_bytes, "tvc_pitch_path_carry_f32");
}
int tvc_frame_share_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, const int64_t* row_count, int rows, const float* alpha,
                        const float* protect, float* share_out) {
    const char* what = "tvc_frame_share_f32";
    if (!ctx) return TVC_ERR_ARG;
    if (!f0 || !row_start || !row_count || rows <= 0 || !protect || !share_out || f0 == share_out) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    std::vector<int> start((size_t)rows), len((size_t)rows);
    for (int b = 0; b < rows; ++b) {
        if (row_start[b] < 0 || row_count[b] < 0 || row_start[b] + row_count[b] > 0x7fffffff)
            return fail(ctx, TVC_ERR_ARG, "%s: row %d = [%lld, +%lld) beyond 32-bit indexing", what, b, (long long)row_start[b], (long long)row_count[b]);
        start[b] = (int)row_start[b];
        len[b] = (int)row_count[b];
    }
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_frame_share_rows(ctx, (hipStream_t)stream, f0, start, len, alpha, protect, share_out);
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
