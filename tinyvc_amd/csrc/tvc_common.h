// Internal declarations shared by the translation units of libtinyvc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/tinyvc_hip.h"
#include "ragged.h"

namespace tvc {

constexpr int kSampleRate = 24000;
constexpr int kNfft = 1920;
constexpr int kHop = 480;
constexpr int kBins = 961;
constexpr int kSslDim = 768;
constexpr int kSslCh = 384;
constexpr int kPitchCh = 128;
constexpr int kPitchClasses = 512;
constexpr int kSrcCh = 128;
constexpr int kHarm = 15;  // num_harmonics + 1 sinusoids
constexpr int kSolaCross = 1920, kSolaSearch = 1920, kSolaDelay = 3840;   // the reference's SOLA geometry (stream.py:48-50): the default, and the caps of cross and search
constexpr int kSolaMaxBlock = 1 << 30;
constexpr int kSolaGroups = 8, kSolaPartFloats = 16384;   // lag groups (workgroups) per stream of the correlation search; its scratch in the context's constant arena

// A conv / 1x1 weight packed for the split-precision MFMA kernels (conv3s.h): the two-part fp16 image A6 (K16 steps x MT6 = Mpad / 32
// m-tiles x 2 parts, 1 KiB pieces in MFMA lane order; every m-tile normalised by a power of two, wscale[MT6] = what the epilogue
// multiplies back) plus the bias row [Mpad].  M / K = real rows / k = cin * taps.
struct PackedW {
    const float* bias = nullptr;
    const float* A6 = nullptr;
    const float* wscale = nullptr;   // [MT6] power-of-two scale of every m-tile: W = image * wscale
    const float* wjoint = nullptr;   // the A6 of the image this one shares its m-tile scales with (two convs accumulated into one tile), else nullptr
    int M = 0, K = 0, Mpad = 0, Kpad = 0, cin = 0, taps = 1, MT6 = 0, S6 = 0;   // S6 = 16-channel slabs in A6 (zero-padded to a multiple of 6)
};

struct ConvNeXtW {
    const float* dw_w = nullptr;  // [C][7]
    const float* dw_b = nullptr;  // [C]
    const float* ln_g = nullptr;
    const float* ln_b = nullptr;
    PackedW c2, c3;
    const float* grn_g = nullptr;  // [2C]
    const float* grn_b = nullptr;
    const float* c3_bias_grn = nullptr;  // c3.bias + c3.weight . grn.beta  [Mpad] (GRN's beta folded through the 1x1)
    float ln_bound = 0.f;                // sqrt(C) max|gamma| + max|beta| >= |LayerNorm output|: the first 1x1's input needs no |max| slot while this is < 2^15
    int C = 0, dilation = 1;
};

// Weight blobs of the 24-channel split-precision kernels (filter_up24s.hip), written by pack.hip: 1 KiB pieces of fp16 pairs in
// v_mfma_f32_32x32x16_f16 A-lane order (a k3 conv's m-tile takes K24_PIECES: 5 K16 steps x 2 parts), then FLOATS floats at the offsets below.
constexpr int K24_PIECES = 10;
struct Up24sBlob {        // one half of the fused ups.4 block (Packer::up24s_half)
    static constexpr int PIECES = 28;
    static constexpr int BA = 0, BB = 32, BSC = 64, BSH = 96;     // biases of conv a, conv b, to_scale, to_shift [32 each]
    static constexpr int W75 = 128, B75 = 296;                    // the folded output conv c5 . output_layer: taps [24][7], bias
    static constexpr int SA = 297, SB = 298, SSC = 299, SSH = 300; // power-of-two scales of conv a, conv b, to_scale, to_shift
    static constexpr int L1A = 301, BMA = 302;                    // max_m sum_k |w_a[m][k]|, max |b_a|: the bound of conv a's output
    static constexpr int FLOATS = 304;
};
struct Down0sBlob {       // the 17 -> 24 k3 conv of downs.0 (Packer::down0s)
    static constexpr int PIECES = K24_PIECES;
    static constexpr int BIAS = 0;                                // [24]
    static constexpr int BW = 29, BB = 30;                        // |out| <= BW |x|max + BB
    static constexpr int SCALE = 31;                              // the image's power-of-two scale
    static constexpr int FLOATS = 32;
};
struct Conv24sBlob {      // one 24-input-channel k3 conv of down24f_kernel, M = 24 or 48 rows: K24_PIECES per m-tile (Packer::conv24s)
    static constexpr int BIAS = 0;                                // [M]
    static constexpr int SCALE = 62;                              // + m-tile: power-of-two scales
    static constexpr int FLOATS = 64;
};

struct DownW {
    PackedW res, c1, c2, c3;             // c3 and res share their per-m-tile scales (accumulated into one tile); cin == 24 packs c3 and res only
    const float* c3res_bias = nullptr;   // c3.bias + down_res.bias [c3.Mpad]: c3 launches that fold the residual 1x1 in as a second K phase
    const float* s24c1 = nullptr;   // cin == 24: weight blobs of down24f_kernel (filter_up24s.hip)
    const float* s24c2 = nullptr;
    const float* s24c3r = nullptr;   // c3's blob with c3.bias + down_res.bias and the joint scales (the launch folds the residual 1x1 in)
    float b1_w = 0.f, b1_b = 0.f, b2_w = 0.f, b2_b = 0.f;   // cin == 24: |c1 out| <= b1_w |xi|max + b1_b, |c2 out| <= b2_w |c1 out| + b2_b (down24f_kernel's on-chip intermediates)
    int cin = 0, cout = 0, factor = 1;
};
// conv + FiLM packed for film_s2.h (cin >= 96): one weight image whose 30 KiB units hold everything a (96-row block, 16-channel slab)
// step multiplies - the conv's three taps and the to_scale / to_shift columns of the same 16 channels - and one table of per-row
// constants [6][C]: conv bias, conv row scale, b_scale, b_shift, to_scale row scale, to_shift row scale.
struct FilmU {
    static constexpr int TAB_BIAS = 0, TAB_SCALE = 1, TAB_BSC = 2, TAB_BSH = 3, TAB_SSC = 4, TAB_SSH = 5;      // rows of `tab`
    const float* img = nullptr;
    const float* tab = nullptr;
    int C = 0;
    float hb_w = 0.f, hb_b = 0.f;      // bound of the half's FIRST conv (the producer of this kernel's h): |c(x) + b| <= hb_w |x|max + hb_b
};
struct UpW {
    PackedW c1, c2, c3, c4, c5, film1, film2;  // film = [to_scale ; to_shift] stacked on M (2C); film.bias = [b_scale (C) ; b_shift (C)]; cin == 24 packs none
    FilmU fu1, fu2;                            // (c2, film1) and (c4, film2) for the single-accumulator pipelined kernel
    const float* s24a = nullptr;               // cin == 24: weight blobs of the two halves of the split-precision fused block (filter_up24s.hip)
    const float* s24b = nullptr;
    float c5_bw = 0.f, c5_bb = 0.f;            // |c5 output| <= c5_bw |its input|max + c5_bb (max_m sum_k |w|, max |b|): the level output's |max| slot without a pass over it
    int cin = 0, cout = 0, factor = 1;
};

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

// Host image of one device arena (pack.hip): the floats to upload and the context slots that point into them.
struct ArenaBuilder {
    std::vector<float> buf;
    std::vector<std::pair<const float**, size_t>> fix;      // (slot, offset): *slot = arena + offset once uploaded
    size_t put(const float** slot, const float* v, size_t n);      // a copy of v[0 .. n) at a 256-byte aligned offset, which `slot` will point at
    size_t put(const float** slot, const std::vector<float>& v) { return put(slot, v.data(), v.size()); }
    void resolve(const float* arena) const {
        for (auto& f : fix) *f.first = arena + f.second;
    }
};

}  // namespace tvc

struct tvc_prof_region {
    std::string name;
    hipEvent_t a = nullptr, b = nullptr;
};

struct tvc_ctx {
    int device = 0;
    int ncu = 0;                              // compute units of the device (tvc_ctx_create): persistent launches size their grids by it
    int profiling = 0;                        // tvc_profile_enable: 0 = off, 1 = hipEvent pairs around every named region, 2 = around `filter_net` only
    std::vector<tvc_prof_region> regions;
    std::vector<hipEvent_t> event_pool;       // recycled hipEvents: no hipEventCreate on the hot path
    hipStream_t side = nullptr;               // fork/join stream: the pitch estimator runs beside the SSL chain
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr, ev_amps = nullptr;      // the decoder's fork: the oscillator beside SourceNet / dsp, FilterNet's content-only front beside SourceNet and the noise branch's tail (decoder.hip run_decoder)
    hipEvent_t ev_src = nullptr;              // ... its first join: the harmonic rows of `source` are written (the launch stream waits for it in front of FilterNet)
    tvc::RagHost* rag = nullptr;              // the ragged batch the drivers are currently running for (ragged.h); nullptr = equal lengths
    int rag_batch_frames = 0;                 // tvc_ctx_set_ragged_batch_frames: frames per in-kernel batch of THIS context's ragged calls (0 = the default)
    int index_assign_chunk = 0;               // tvc_ctx_set_index_assign_chunk: query columns per search call of THIS context's index assignment (0 = the default)
    bool enc_ready = false, dec_ready = false;  // which checkpoint groups tvc_finalize_weights packed
    char enc_missing[160] = {0}, dec_missing[160] = {0};
    std::map<std::string, tvc::HostTensor> host;  // staged checkpoint tensors
    std::vector<float> pitch_table;
    float* arena = nullptr;        // packed checkpoint weights, one allocation per finalize
    float* const_arena = nullptr;  // FFT tables, built at ctx_create
    size_t arena_floats = 0;
    char err[512] = {0};

    // constant tables
    const float* fft_tw960 = nullptr;    // fft.hip tables: (cos, sin)(2 pi j / 960) [960], (cos, sin)(2 pi k / 1920) [961], periodic Hann [1920]
    const float* fft_tw1920 = nullptr;
    const float* fft_hann = nullptr;
    const float* pitch_freq = nullptr;  // [512]
    const float* sola_part = nullptr;   // scratch of the split SOLA search: (best value, best lag) per (stream, lag group); kSolaPartFloats floats
    const float* dn_win = nullptr;      // denoise.hip tables: sqrt-Hann window [640], (cos, sin)(2 pi j / 320) [320], (cos, sin)(2 pi k / 640) [321]
    const float* dn_tw320 = nullptr;
    const float* dn_tw640 = nullptr;

    // encoder
    tvc::PackedW enc_in;  // ssl(384) and pitch(128) input 1x1 stacked: M = 512
    const float* ssl_ln_g = nullptr;
    const float* ssl_ln_b = nullptr;
    const float* pit_ln_g = nullptr;
    const float* pit_ln_b = nullptr;
    tvc::ConvNeXtW ssl_mid[6], pit_mid[4], src_mid[3];
    tvc::PackedW ssl_out, pit_out;
    // source net
    tvc::PackedW src_content_in, src_to_amps, src_to_kernel;
    const float* src_e_w = nullptr;
    const float* src_e_b = nullptr;
    const float* src_f_w = nullptr;
    const float* src_f_b = nullptr;
    // filter net
    tvc::PackedW flt_content_in;
    const float* flt_down0s = nullptr;   // downs.0 weight blob of the split-precision kernel (filter_up24s.hip)
    float down0_bw = 0.f, down0_bb = 0.f; // |downs.0 output| <= down0_bw |input|max + down0_bb: the scale skips[0] is written / read with
    float flt_in_bw = 0.f, flt_in_bb = 0.f;   // |content_in(content) + f0_in(log f0)| <= flt_in_bw |content|max + flt_in_bb: FilterNet's x0 slot without a pass over x0
    const float* flt_f_w = nullptr;
    const float* flt_f_b = nullptr;
    tvc::DownW downs[4];
    tvc::UpW ups[5];
};

namespace tvc {

inline int fail(tvc_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define TVC_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return tvc::fail(ctx, TVC_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                                \
    } while (0)

#define TVC_CHECK(expr)        \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != 0) return rc_; \
    } while (0)

// Bump allocator over the caller's workspace; in dry mode it only measures (api.h run_walks: every entry walks its driver dry, then for
// real).  The drivers make the same get() calls in both walks - only launches, memsets, events and uploads look at `dry` -: equal peaks.
struct Ws {
    char* base;
    size_t cap, off = 0, peak = 0;
    bool dry;
    Ws(void* p, size_t c, bool d) : base((char*)p), cap(c), dry(d) {}
    template <class T>
    T* get(size_t n) {
        size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
        size_t o = off;
        off += bytes;
        if (off > peak) peak = off;
        if (dry) return (T*)(uintptr_t)256;  // never dereferenced
        return (T*)(base + o);
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};

// RAII region timer: records a hipEvent pair on the launch stream when ctx->profiling is on (never while ws.dry).
struct ProfScope {
    tvc_ctx* ctx;
    hipStream_t s;
    int idx = -1;
    ProfScope(tvc_ctx* c, hipStream_t st, const Ws& ws, const char* name) : ctx(c), s(st) {
        if (!c || !c->profiling || ws.dry) return;
        if (c->profiling == 2 && std::strncmp(name, "filter_net", 10) != 0) return;     // the roofline's regions alone (filter_net, and filter_net.input@side when the input contraction is forked): 2-4 event records per step instead of 38
        tvc_prof_region r;
        r.name = name;
        auto take = [&](hipEvent_t* e) {
            if (!c->event_pool.empty()) {
                *e = c->event_pool.back();
                c->event_pool.pop_back();
                return true;
            }
            return hipEventCreate(e) == hipSuccess;
        };
        if (!take(&r.a) || !take(&r.b)) return;
        (void)hipEventRecord(r.a, s);
        c->regions.push_back(r);
        idx = (int)c->regions.size() - 1;
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(ctx->regions[idx].b, s);
    }
};

// A branch on the context's side stream (run_encoder's pitch chain, run_decoder's oscillator and FilterNet's content-only front).  fork() forks
// only when the side stream and both events exist, ws.dry is false and `s` is not being captured; `side` = the branch's
// stream (`s` unforked).  join_so_far(ev) puts `s` behind the side launches made so far and leaves the branch open.  end() records `ev_join`
// behind the branch; join() makes `s` wait for it (recording it first if end() has not run), and so does the destructor if join() has not
// run: an error return leaves `s` behind every side launch (they write into the workspace), whichever of the joins it came before.
struct SideFork {
    tvc_ctx* ctx;
    hipStream_t s, side;
    hipEvent_t ev_join = nullptr;      // non-null while forked
    bool ended = false;
    SideFork(tvc_ctx* c, hipStream_t st) : ctx(c), s(st), side(st) {}
    bool forked() const { return ev_join != nullptr; }
    int fork(const Ws& ws, hipEvent_t ev_fork, hipEvent_t join) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (ws.dry || !ctx->side || !ev_fork || !join || hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return 0;
        TVC_HIP(ctx, hipEventRecord(ev_fork, s));
        TVC_HIP(ctx, hipStreamWaitEvent(ctx->side, ev_fork, 0));
        side = ctx->side;
        ev_join = join;
        return 0;
    }
    int join_so_far(hipEvent_t ev) {
        if (!forked()) return 0;
        TVC_HIP(ctx, hipEventRecord(ev, side));
        TVC_HIP(ctx, hipStreamWaitEvent(s, ev, 0));
        return 0;
    }
    int end() {
        if (forked() && !ended) TVC_HIP(ctx, hipEventRecord(ev_join, side));
        ended = true;
        return 0;
    }
    hipError_t record_and_wait() {
        hipEvent_t e = ev_join;
        ev_join = nullptr;
        const hipError_t r = e && !ended ? hipEventRecord(e, side) : hipSuccess;
        return e && r == hipSuccess ? hipStreamWaitEvent(s, e, 0) : r;
    }
    int join() { TVC_HIP(ctx, record_and_wait()); return 0; }
    ~SideFork() { (void)record_and_wait(); }      // (an error return between fork and join keeps its own message)
};

inline int launch_check(tvc_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, TVC_ERR_HIP, "launch %s: %s", what, hipGetErrorString(e));
    return 0;
}

// Opts the kernels K... into `bytes` of dynamic LDS on the first call per device.  The attribute is per (function, device), so the flag is
// process-wide and not the context's: a second context whose first call is being captured must not set the attribute inside the capture.
template <auto... K>
int lds_optin(tvc_ctx* ctx, int bytes, const char* what) {
    static std::atomic<bool> ready_dev[64];
    std::atomic<bool>& ready = ready_dev[ctx->device & 63];
    if (ready.load(std::memory_order_acquire)) return 0;
    for (const void* k : {(const void*)K...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return fail(ctx, TVC_ERR_HIP, "%s setup: %s", what, hipGetErrorString(e));
    }
    ready.store(true, std::memory_order_release);
    return 0;
}

// ---- checkpoint packing (pack.hip: host only, no HIP call) ---------------------------------------
// the constant arena: FFT tables and the SOLA search's scratch, independent of any checkpoint
void pack_constants(tvc_ctx*, ArenaBuilder*);
// the weight arena from ctx->host and ctx->pitch_table; it also sets the images' geometry and the analytic bounds in ctx.
// missing_enc / missing_dec: the first missing or misshapen key of the encoder's / the decoder's tensors (empty: complete).
void pack_checkpoint(tvc_ctx*, ArenaBuilder*, std::string* missing_enc, std::string* missing_dec);

// ---- stage drivers (each enqueues kernels on `s`; ws.dry = measure the workspace only) ----------
int run_stft(tvc_ctx*, hipStream_t, Ws&, const float* wav, float* spec, int B, int64_t L);
int run_stft_fft(tvc_ctx*, hipStream_t, const float* wav, float* spec, int B, int64_t L);
int run_noise_ifft(tvc_ctx*, hipStream_t, const float* kern, const float* angle, uint64_t seed, float* frames, int B, int T, bool angle_padded = false);      // angle == nullptr: phases drawn in the kernel from `seed`
// emax (optional, equal-length batches only): per-utterance max of the pooled |x| = max |wav| of the utterance, written (not accumulated)
int run_energy(tvc_ctx*, hipStream_t, Ws&, const float* wav, float* energy, int B, int64_t L, float* emax = nullptr, float* spec_bound = nullptr,
               float* zero = nullptr, int nz = 0);      // (emax given: the pooled-maximum launch also zeroes zero[0 .. nz))
int run_knn_amax_rows(tvc_ctx*, hipStream_t, const std::vector<const float*>& blobs, float* out);      // out[i] = *blob_amax(blobs[i]) (knn_gather.hip)
// out[b] = a * in[b * in_stride] + c for b < n: a |max| slot from the slot of the tensor it is a bounded function of (frontend.hip)
int run_slot_affine(tvc_ctx*, hipStream_t, float* out, const float* in, int in_stride, float a, float c, int n);
int run_slot_prep(tvc_ctx*, hipStream_t, float* zero, int nz, float* o1, const float* in1, int s1, float a1, float c1, float* o2, const float* in2, int s2, float a2,
                  float c2, float* o3, float a3, float c3, int n);
// prepared kNN blob (knn_blob.h; written by knn_prepare.hip): header word 0 = magic, word 5 = format version.  Version 2 (round 5): word 4 holds the raw vectors' |max| (a float), which
// the decoder takes as the bound of `matched` - a blob of another version has 0 there (= "no scaling": the fp16 range guard silently off) and is refused.
constexpr int kBlobMagic = 0x54564B4E, kBlobVersion = 2;
constexpr int kFilterSlotX = 2;       // ... and the one of its input contraction's output (S_X)
constexpr int kFilterSlots = 41;      // run_filter's |max| slots per utterance (decoder.hip S_COUNT)
// spec_bound (optional): per-utterance upper bounds of |spec| (the slot of the input contraction); nullptr = one pass over spec measures it
int run_encoder(tvc_ctx*, hipStream_t, Ws&, const float* spec, float* ssl, float* f0,
                float* logits, int B, int T, const float* spec_bound = nullptr, float* zeroed_slots = nullptr,      // zeroed_slots: 3 x utterances floats already zeroed on this stream
                float* f0_shifted = nullptr, float shift = 0.f,      // f0_shifted: also shift_frequency(f0, shift)
                const float* shifts = nullptr);                      // ... with shifts[utterance] (device, one per utterance) instead of `shift`
int run_pitch_decode(tvc_ctx*, hipStream_t, const float* logits, float* f0, int B, int T);
int run_knn(tvc_ctx*, hipStream_t, Ws&, const float* src, const float* prepared, int64_t N,
            float* out, int64_t* idx_out, int B, int T);
// several prepared indices in one call (knn_gather.hip; knn_search.h segments): in[] = runs of query columns [col0, col0 + ncols) of the [B][768][T] queries
// that search `blob` (prepared for N vectors), in column order, covering all B * T columns; adjacent runs of one blob are one segment
struct KnnSegIn {
    const float* blob;
    int64_t N;
    int col0, ncols;
};
// alpha (optional, both drivers): the caller's DEVICE array [rows] of the source's own share - out = mu * (1 - a) + src * a with mu the alpha-less
// result (knn_gather.hip); nullptr launches exactly what the call without it launches.  share (optional, both drivers; takes alpha's place): a
// DEVICE array of one share per query COLUMN (run_frame_share's, which has alpha in it) - the protect form of the same store
// wt (optional, both drivers; with or without alpha / share): the weighted form of the same launch - the mean over the neighbours[row] nearest
// of the four rows, weighted by their similarities under width[row] (DEVICE arrays of one value per caller's row, either nullable = 4 / +inf;
// a ragged batch finds the row through its tables, as alpha), sims_out (nullable) [M][B][T][4] the merged lists' similarities beside idx_out
struct KnnWeight {
    const int* neighbours = nullptr;
    const float* width = nullptr;
    float* sims_out = nullptr;
};
// jn (optional, both drivers; with or without wt, alpha / share): the joined form - the weights form around the neighbour a path over the
// utterance chose (knn_gather.hip: merge + affinity, the path, the joined gather).  join: a DEVICE array of one continuity weight per caller's
// row; anchor_out (nullable) [M][B][T] int32, affinity_out (nullable) [M][B][T][4][4].  Takes workspace (both walks): 101 bytes per virtual column.
struct KnnJoin {
    const float* join = nullptr;
    int* anchor_out = nullptr;
    float* affinity_out = nullptr;
};
int run_knn_segs(tvc_ctx*, hipStream_t, Ws&, const float* src, const KnnSegIn* in, int nin, float* out, int64_t* idx_out, int B, int T,
                 const float* alpha = nullptr, const float* share = nullptr, const KnnWeight* wt = nullptr, const KnnJoin* jn = nullptr);
// a weighted blend of M indices per row (knn_gather.hip): in[] = the (term, row) runs over M * B * T VIRTUAL query columns, term-major - term m's
// search of real column n is column m * B * T + n -, weights = the caller's device array [rows][M] (read by the kernels, never by the host),
// out [B][768][T] = w_0 * mu_0 + ... in term order, idx_out (nullable) [M][B][T][4]
int run_knn_blend(tvc_ctx*, hipStream_t, Ws&, const float* src, const KnnSegIn* in, int nin, int M, const float* weights, float* out, int64_t* idx_out,
                  int B, int T, const float* alpha = nullptr, const float* share = nullptr, const KnnWeight* wt = nullptr, const KnnJoin* jn = nullptr);
// out[i] = sum_m |weights[rows[i]][m]| * *blob_amax(blobs[i * M + m]): the bound of row i's blended content
int run_knn_blend_bound(tvc_ctx*, hipStream_t, const std::vector<const float*>& blobs, const std::vector<int>& rows, int M, const float* weights, float* out);
// the content bound of an alpha call: out[i] = |1 - a| * idx_bound[i * stride] + |a| * srcmax[i] for utterance i < n, a = alpha[its row]
// protect (optional; alpha then nullable = 0): with a_u = a + (1 - a) * protect[row], max(|1 - a|, |1 - a_u|) and max(|a|, |a_u|) take the factors' places
int run_knn_alpha_bound(tvc_ctx*, hipStream_t, const float* alpha, const float* idx_bound, int stride, const float* srcmax, float* out, int n,
                        const float* protect = nullptr);
// share[n] = the source's share of query column n of a conversion of B rows of T frames (a ragged batch: ctx->rag, B = 1) from its f0 [B][T]:
// a + (1 - a) * (p * w[n]), a = alpha[row] (nullptr: 0), p = protect[row], w the unvoiced weight of the frame within its own utterance
// (knn_gather.hip frame_share_kernel; include/tinyvc_hip.h has the definition)
int run_frame_share(tvc_ctx*, hipStream_t, const float* f0, const float* alpha, const float* protect, float* share, int B, int T);
// the same over caller's rows i = columns [start[i], start[i] + len[i]) of f0 and share, alpha / protect one per row
int run_frame_share_rows(tvc_ctx*, hipStream_t, const float* f0, const std::vector<int>& start, const std::vector<int>& len, const float* alpha,
                         const float* protect, float* share);
// slot[utterance] = max |ssl| of that utterance (slot already zeroed on this stream; encoder.hip)
int run_ssl_amax(tvc_ctx*, hipStream_t, const float* ssl, int B, int T, float* slot);

// ---- one conversion, as the entries describe it to convert_impl (api_convert.hip) and to the ragged batch loop (ragged.hip) -----------
// What the rows of a call search: ONE prepared index, or host tables of one per row of the caller's batch (tvc_*_multi) - never both.
// The blend form (tvc_*_blend) is a per-row table with M terms per row: blobs / Ns are [rows][M] row-major, `weights` the device array
// [rows][M] in the caller's row order.
struct ConvertIndex {
    const float* blob = nullptr;               // one index for every row ...
    int64_t N = 0;
    const float* const* blobs = nullptr;       // ... or, per_row, blobs[r] / Ns[r] for the caller's row r (blob and N stay unset)
    const int64_t* Ns = nullptr;
    bool per_row = false;
    int M = 0;                                 // blend: terms per row (0: no blend, one blob per row)
    const float* weights = nullptr;            // blend: device, [rows][M]
    static ConvertIndex one(const float* blob, int64_t N) { return {blob, N, nullptr, nullptr, false, 0, nullptr}; }
    static ConvertIndex table(const float* const* blobs, const int64_t* Ns) { return {nullptr, 0, blobs, Ns, true, 0, nullptr}; }
    static ConvertIndex blend(const float* const* blobs, const int64_t* Ns, int M, const float* weights) { return {nullptr, 0, blobs, Ns, true, M, weights}; }
};
// A stream set's pitch tracker (frontend.hip pitch_track_kernel): the device state - ring [S][W] fp32, count [S] int64, autos [S] fp32 - and
// the host values of one block: the new frames are columns [start, start + n) of every row, n <= 256; 1 <= W <= 8192; min_voiced >= 1;
// slew >= 0 semitones per call (+inf: none)
struct PitchTrackState {
    int start = 0, n = 0, W = 0, min_voiced = 1;
    float slew = 0.f;
    float* ring = nullptr;
    int64_t* count = nullptr;
    float* autos = nullptr;
};
struct ConvertCall {
    const float* wav = nullptr;                // [B][L] in, row b zero-padded behind lens[b] samples
    float* wave = nullptr;                     // [B][L] out
    int B = 0;
    int64_t L = 0;                             // samples per row (the Lmax of a ragged call)
    const int64_t* lens = nullptr;             // host, one per row; nullptr: every row is L samples long
    ConvertIndex index;
    float shift = 0.f;                         // semitones of every row ...
    const float* shifts = nullptr;             // ... or (host, with a per-row index only) one per row
    const float* angle = nullptr;              // noise phases; nullptr: drawn from `seed`
    uint64_t seed = 0;
    // automatic pitch (tvc_convert_auto_f32): target_f0 (device, one register in Hz per caller's row) makes shift / shifts the OFFSET on top
    // of 12 log2(target_f0[r] / the row's own register), found on the device between the encoder and the decoder (run_pitch_match);
    // shift_out (device, nullable) receives the applied shifts, one per caller's row
    const float* target_f0 = nullptr;
    float* shift_out = nullptr;
    // tvc_convert_track_f32 (equal lengths only): the register is the stream's history, not the call's own rows - run_pitch_track takes
    // run_pitch_match's place
    const PitchTrackState* track = nullptr;
    // tvc_convert_*alpha_f32: alpha (device, one fp32 per caller's row, read when the kernels run) keeps that share of the row's own content
    // features - matched = mu * (1 - a) + ssl * a - and the decoder's content bound becomes |1 - a| * (the index's) + |a| * max |ssl|
    const float* alpha = nullptr;
    // tvc_convert_*protect_f32: protect (device, one fp32 per caller's row; alpha may then be nullptr = 0) raises the share on unvoiced frames of
    // the f0 this call decodes - a_t = a + (1 - a) * (p * w[t]), one per query column (run_frame_share) in the place of the row's alpha
    const float* protect = nullptr;
    // tvc_weighted_convert*_f32: neighbours (device, one int32 per caller's row) and width (device, one fp32 per caller's row), either nullable:
    // the match is the mean over the row's k nearest of the four rows, weighted by their similarities (knn_gather.hip WeightIn) - the mu of alpha's
    // and protect's definitions, every term's mu_m of a blend.  A convex combination of index rows: the content bounds stay as they are.
    const int* neighbours = nullptr;
    const float* width = nullptr;
    // tvc_joined_convert*_f32: join (device, one fp32 per caller's row) - the continuity weight of the match along a path (knn_gather.hip KnnJoin):
    // the weights above form around the neighbour the path chose.  Still a convex combination of index rows.
    const float* join = nullptr;
    // tvc_convert_*path_f32: path (host settings) puts the Viterbi decode of the call's own logits (run_pitch_path, directly behind the encoder) in
    // the place of the per-frame decode: protect's voicing weight, the automatic shift, a tracker, the shift and the decoder read its f0
    const tvc_pitch_path* path = nullptr;
    // tvc_convert_carry_f32 (equal lengths only, with path): carry (device, [B][512], read and written in place) is the path's state from one
    // stream block to the next - row b starts from carry[b] and leaves the best-predecessor values of frame carry_frame there
    int carry_frame = 0;
    float* carry = nullptr;
    // tvc_tuned_convert*_f32: snap (host settings) puts the pitch correction (run_pitch_snap, directly in front of the decoder, in place) on the
    // shifted f0 - notes (device, [128]) and strength (device, one fp32 per caller's row, nullable = 1) are read when the kernel runs; the
    // state snap_note / snap_ratio (device, one per row, both or neither, equal lengths only) is read at frame 0 and written behind frame
    // snap_carry_frame - 1
    const tvc_pitch_snap* snap = nullptr;
    const float *notes = nullptr, *strength = nullptr;
    int snap_carry_frame = 0;
    int32_t* snap_note = nullptr;
    float* snap_ratio = nullptr;
};
// Generator.convert over c.B rows of c.L samples (c.lens is not looked at: a ragged call reaches this through convert_ragged_batches,
// one batch at a time as ONE row with ctx->rag set, ragged.h)
int convert_impl(tvc_ctx*, hipStream_t, Ws&, const ConvertCall& c);
int run_knn_topk(tvc_ctx*, hipStream_t, Ws&, const float* src, const float* prepared, int64_t N,
                 float* sims_out, int64_t* idx_out, int B, int T);
// match_features for any k <= 8 and metric (0 cos, 1 IP, 2 L2) on the RAW index [768][N] in plain fp32 (knn_general.hip)
int run_knn_general(tvc_ctx*, hipStream_t, Ws&, const float* src, const float* index, int64_t N, int k, int metric, float* out, int64_t* idx_out,
                    float* val_out, int B, int T);
int run_knn_slots(tvc_ctx*, hipStream_t, const float* prepared, int64_t N, const int64_t* idx, float* slots, int64_t nslots);
int run_knn_finish(tvc_ctx*, hipStream_t, const float* slots, float* out, int B, int T);
int run_shift(tvc_ctx*, hipStream_t, const float* f0, float* out, int64_t n, float semitones);
// The pitch register of rows of f0 and the shift that moves it onto a target's (frontend.hip pitch_match_kernel): row i = columns
// [start, start + len) of f0, its slot `idx` in target / median_out / voiced_out / shift_out, its host offset in semitones.
//   median = the lower median of the row's values > 0 (0 without one), voiced = their count,
//   shift  = offset + 12 log2(target[idx] / median)   (offset alone: no voiced frame, target[idx] <= 0 or NaN, target == nullptr),
//   f0s[start + t] = shift_frequency(f0[start + t], shift).   Every output is optional.  One launch per 256 rows, no workspace.
struct PitchRow {
    int start, len, idx;
    float offset;
};
int run_pitch_match(tvc_ctx*, hipStream_t, const float* f0, const std::vector<PitchRow>& rows, const float* target, float* median_out, int* voiced_out,
                    float* shift_out, float* f0s);
// One block of S streams in lock step, f0 [S][T] (frontend.hip pitch_track_kernel): append the voiced frames among columns [t.start,
// t.start + t.n) to each stream's ring, take the lower median of the ring, move t.autos toward 12 log2(target / median) by at most t.slew,
// shift = offset (offsets[s] when given, host values) + autos, f0s = shift_frequency(f0, shift) over all T columns.  median_out, count_out,
// shift_out and f0s are optional.  One launch (one per 512 streams with per-stream offsets), no workspace.
int run_pitch_track(tvc_ctx*, hipStream_t, const float* f0, int S, int T, const PitchTrackState& t, const float* target, float offset,
                    const float* offsets, float* median_out, int64_t* count_out, float* shift_out, float* f0s);
// The pitch path (pitch_path.hip; include/tinyvc_hip.h has the definition): a Viterbi decode of rows of logits.  Row i = columns [start, start +
// len) with `shift` the semitones of its f0s; class k of column n lies at logits[(n / S) * 512 * S + k * S + n % S] and no row straddles a
// multiple of S; bp = 512 uint16 per column up to the last row's end (pitch_path_ws_bytes); f0, f0s, path_out, score_out [rows][512] optional.
// One launch per 256 rows.  The caller has checked the settings (pitch_path_check: 0, or TVC_ERR_ARG with the reason in `why`).
// The carry: prior / carry_out (device, [rows][512], nullable, may be one array) and carry_frame = h - row i starts from the sanitised
// prior[i] and leaves best_h in carry_out[i]; the caller has checked that every non-empty row has more than h >= 1 frames (a row without
// frame h stores nothing).  Both nullptr is the call as it was, and launches the kernel it launched.
constexpr int kPitchPathMaxBand = TVC_PITCH_PATH_MAX_BAND, kPitchPathMaxRefine = TVC_PITCH_PATH_MAX_REFINE;
struct PitchPathRow {
    int start, len;
    float shift;
};
size_t pitch_path_ws_bytes(int64_t columns);
int pitch_path_check(const tvc_pitch_path& p, char* why, size_t why_bytes);
int run_pitch_path(tvc_ctx*, hipStream_t, const float* logits, long S, const std::vector<PitchPathRow>& rows, const tvc_pitch_path& p, uint16_t* bp, float* f0,
                   float* f0s, int* path_out, float* score_out, int carry_frame = 0, const float* prior = nullptr, float* carry_out = nullptr);
// Pitch correction (pitch_snap.hip; include/tinyvc_hip.h has the definition): row i = columns [start, start + len) of f0 and of out (which
// may be f0), idx = its slot in strength (nullable) and in the state note / ratio (both or neither; stored behind frame carry_frame - 1, which
// the caller has checked every non-empty row to have).  note_out optional.  One launch for equal rows back to back, else one per 256
// rows; no workspace.  The caller has checked the settings (pitch_snap_check: 0, or TVC_ERR_ARG with the reason in `why`).
constexpr int SNAP_ROWS = 256;
constexpr float kSnapMaxHysteresis = 1.0594631f;      // (float)2^(1/12)
struct SnapRow {
    int start, len, idx;
};
int pitch_snap_check(const tvc_pitch_snap& p, char* why, size_t why_bytes);
int run_pitch_snap(tvc_ctx*, hipStream_t, const float* f0, const std::vector<SnapRow>& rows, const tvc_pitch_snap& p, const float* notes, const float* strength,
                   int carry_frame, int32_t* note, float* ratio, float* out, int32_t* note_out);
int run_uniform_to_angle(tvc_ctx*, hipStream_t, float* u, int64_t n);
// content_bound (optional): an upper bound of |content| (the prepared index's |max| when content came out of the kNN match): ONE float, or
// with content_bound_stride = 1 one per utterance (a match against one index per utterance);
// energy_bound (optional): per-utterance upper bounds of |energy|.  nullptr = measured by a pass over the tensor.
int run_decoder(tvc_ctx*, hipStream_t, Ws&, const float* content, const float* f0,
                const float* energy, const float* angle, uint64_t seed, float* wave, float* amps_out,
                float* kernel_out, float* source_out, int B, int T, const float* content_bound = nullptr, const float* energy_bound = nullptr,
                int content_bound_stride = 0);
struct FilterTaps {   // optional copies of FilterNet's block outputs (tvc_filter_net_f32)
    float* skips[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* ups[4] = {nullptr, nullptr, nullptr, nullptr};
};
// cmax / smax / the trailing float* of run_dsp: per-utterance |max| slots of content / cat[source, energy] (block-floating-point
// guard of the fp16 split, split_fp16.h); nullptr = the stage computes (or keeps) its own
// FilterNet's content-only front - the input contraction x0 and Upsample 0's c1 output h0, which read content, f0 and cmax only - as
// run_decoder hands it to run_filter: the two buffers (live for the whole call, outside the region run_filter allocates from), and the
// caller's fork.  With the fork open, the caller has launched the contraction on fk->side; run_filter launches c1 behind it there, beside
// its own first launches, and joins fk in front of Upsample 0's FiLM launch, the first that reads h0; an earlier return leaves the join to fk's
// destructor.  Unforked, run_filter runs both on `s`, in the chain's order.
struct FilterFront {
    SideFork* fk;         // the caller's fork
    float *x0, *h0;       // [B][384][T], [B][384][2 T]
};
int run_filter(tvc_ctx*, hipStream_t, Ws&, const float* content, const float* f0, const float* energy,
               const float* source, float* wave, int B, int T, const FilterTaps* taps = nullptr, const float* cmax = nullptr, const float* smax = nullptr,
               float* zeroed_slots = nullptr, bool x_slot_set = false, const FilterFront* front = nullptr);      // zeroed_slots: kFilterSlots x utterances floats the caller has already zeroed on this
                                                                             // stream; x_slot_set: ... and has set slot kFilterSlotX to flt_in_bw |content|max + flt_in_bb (a forked front needs both)
// run_decoder's fork (decoder.hip): the harmonic synthesis on `side` beside SourceNet's to_kernel GEMM and the noise branch; csum's frame sums
// are already scanned there, amps_ready is recorded on the launch stream behind the amplitudes' GEMM.  The caller joins `side` itself.
struct DspFork {
    hipStream_t side;
    hipEvent_t amps_ready;
};
// csum: the oscillator's frame sums [B][15][T] (doubles); nullptr = run_dsp takes its own from ws
int run_dsp(tvc_ctx*, hipStream_t, Ws&, const float* f0, const float* amps, const float* kern, const float* angle, uint64_t seed, float* source, int B, int T,
            float* smax = nullptr, double* csum = nullptr, const DspFork* fk = nullptr);
// the legal SOLA geometries, in one place (sola.hip): 0, or TVC_ERR_ARG with the reason in `why`; every out pointer is nullable
int sola_geometry(int block, int cross, int search, int delay, int64_t* min_ly, int* latency_min, int* latency_max, char* why, size_t why_bytes);
int run_sola(tvc_ctx*, hipStream_t, const float* y, float* sola_buf, const float* fade_in, float* out, int32_t* shift_out,
             int S, int64_t Ly, int block, int cross, int search, int delay, int use_pv);
int run_stream_push(tvc_ctx* ctx, hipStream_t s, float* buf, const float* blocks, int S, int n, int m);
// the noise gate behind the tail (gate.hip).  kGateMaxSub: the sub-frame powers of a block and its look-ahead that a workgroup keeps in LDS
constexpr int kGateMaxSub = 4096, kGateMaxSubFrame = 1 << 16, kGateMaxCount = 1 << 20;
struct StreamGate {
    int block, sub, look, hold, attack, release;      // samples, samples, and counts of sub-frames
    float hysteresis_db, range_db;
    const float* threshold_db;      // [S] device, read when the kernel runs
    int32_t* open;                  // [S] device state, read and advanced in place: open, hold, gain
    int32_t* hold_state;
    float* gain;
    float* level_db;                // [S] device, optional: the block's input level
};
// the legal gate geometries, in one place (gate.hip): 0, or TVC_ERR_ARG with the reason in `why`; every out pointer is nullable
int stream_gate_geometry(int block, int sub, int look, int hold, int attack, int release, int* nsub, int* look_samples, char* why, size_t why_bytes);
// (the caller has checked the geometry; x [S][n], y and out [S][block], out may be y; shift [S] optional)
int run_stream_gate(tvc_ctx*, hipStream_t, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S, const StreamGate& g);
// the loudness envelope match (loudness.hip).  kLoudnessTile: the sub-frames one workgroup of the offline form owns (tvc_loudness_geometry
// reports it); kLoudnessChunk: the sub-frames of a stream block whose powers a workgroup keeps in LDS at a time
constexpr int kLoudnessTile = 64, kLoudnessChunk = 512, kLoudnessMaxSmooth = 32, kLoudnessMaxSubFrame = 1 << 16;
// the cap on a stream block's sub-frames is the gate's, kept so that the two stages take the same blocks: the kernel walks a block in chunks
// of kLoudnessChunk sub-frames, so nothing of it is sized by this number
constexpr int kLoudnessMaxBlockSub = 4096;
constexpr int64_t kLoudnessMaxLength = (int64_t)1 << 40;
// a ragged batch's row lengths as kernel arguments: the rows of one launch of the offline form (3 KiB of the 4 KiB a launch may pass)
constexpr int kLoudnessLenRows = 384;
struct LoudnessLens {
    int64_t v[kLoudnessLenRows];
};
struct LoudnessConst {
    double floor, lo, hi;      // 10^(floor_db / 10), 10^(-cut_db / 20), 10^(boost_db / 20)
};
struct StreamLoudness {
    int block, sub, smooth;         // samples, samples, sub-frames each side (the window trails: 2 * smooth + 1 sub-frames)
    const float* share;             // [S] device, read when the kernel runs
    double* src_ring;               // [S][2 * smooth + 1] device state, read and advanced in place: the last powers of the input and of the output,
    double* out_ring;               //   slot = sub-frame index % window
    int64_t* frames;                // [S] sub-frames seen
    float* gain;                    // [S] the last edge gain
    float* gain_db;                 // [S] device, optional: the same in dB
};
// the legal geometries, in one place (loudness.hip): 0, or TVC_ERR_ARG with the reason in `why`; every out pointer is nullable.  stream_block:
// `length` is a stream's block
int loudness_geometry(int64_t length, int sub, int smooth, bool stream_block, int64_t* nsub, int* window, int* tile, char* why, size_t why_bytes);
// the three dB settings as the kernels take them: 0, or TVC_ERR_ARG with the reason in `why`
int loudness_constants(float floor_db, float boost_db, float cut_db, LoudnessConst* c, char* why, size_t why_bytes);
// (the caller has checked the geometry, the alignment and that out is y or does not overlap it; lengths [B] HOST, optional; gains optional)
int run_loudness_match(tvc_ctx*, hipStream_t, const float* x, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* share, int sub,
                       int smooth, const LoudnessConst& c, float* gains);
int run_stream_loudness(tvc_ctx*, hipStream_t, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                        const StreamLoudness& g, const LoudnessConst& c, float* gains);
// the look-ahead peak limiter (limiter.hip).  kLimiterTile: the sub-frames one workgroup of the offline form owns (tvc_limiter_geometry reports
// it); kLimiterEdges: the consecutive edges of a tile one of its 256 threads owns; kLimiterChunk: the sub-frames of a stream block whose
// peaks and gains a workgroup keeps in LDS at a time (tvc_stream_limiter_geometry reports it)
constexpr int kLimiterTile = 512, kLimiterEdges = (kLimiterTile + 1 + 255) / 256, kLimiterChunk = 512, kLimiterMaxRelease = 4096, kLimiterMaxSubFrame = 1 << 16;
constexpr int kLimiterMaxBlock = 1 << 30;
constexpr int64_t kLimiterMaxLength = (int64_t)1 << 40;
struct StreamLimiter {
    int block, sub;                 // samples, samples
    const float* ceiling;           // [S] device, read when the kernel runs: linear; NaN, <= 0 and +inf are off
    float* tail;                    // [S][sub] device state, read and advanced in place: the driven samples of the sub-frame not yet emitted,
    float* peak;                    // [S] that sub-frame's peak,
    float* gain;                    // [S] e at that sub-frame's start
    float* reduction_db;            // [S] device, optional: 20 log10 of the block's smallest edge gain
};
// the legal geometries, in one place (limiter.hip): 0, or TVC_ERR_ARG with the reason in `why`; every out pointer is nullable.  stream_block:
// `length` is a stream's block, and `tile` the chunk
int limiter_geometry(int64_t length, int sub, int release, bool stream_block, int64_t* nsub, int* delay, int* tile, char* why, size_t why_bytes);
// drive_db as the factor the kernels take: 0, or TVC_ERR_ARG with the reason in `why`
int limiter_drive(float drive_db, float* drive, char* why, size_t why_bytes);
// (the caller has checked the geometry, the alignment and that out lies apart from y; lengths [B] HOST, optional; gains optional)
int run_limit(tvc_ctx*, hipStream_t, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* ceiling, int sub, int release, float drive,
              float* gains);
int run_stream_limit(tvc_ctx*, hipStream_t, const float* y, float* out, int S, const StreamLimiter& g, int release, float drive, float* gains);
// the spectral suppressor in front of the window (denoise.hip).  Frames of kDenoiseFrame samples at a hop of 160 or 320
constexpr int kDenoiseFrame = 640, kDenoiseBins = kDenoiseFrame / 2 + 1, kDenoiseMaxFrames = 4096;
struct StreamDenoise {
    int block, hop;                        // samples
    float a_s, a_n, clamp, beta;           // smoothing of the power, adaptation and clamp of the noise estimate, over-subtraction
    int warm;                              // frames the noise estimate is a running mean over
    const float* reduction_db;             // [S] device, read when the kernel runs
    float* hist;                           // [S][640 - hop] device state, read and advanced in place: raw input tail, overlap-add tail,
    float* ola;                            //   smoothed power and noise power per bin [S][321], frames counted
    float* smooth;
    float* noise;
    int32_t* frames;
    float* noise_db;                       // [S] device, optional: the noise estimate in dB re full scale per sample
};
// the legal suppressor geometries, in one place (denoise.hip): 0, or TVC_ERR_ARG with the reason in `why`; every out pointer is nullable
int stream_denoise_geometry(int block, int hop, int* frames, int* delay, char* why, size_t why_bytes);
// (the caller has checked the geometry and the scalars; x and out [S][block], out may be x)
int run_stream_denoise(tvc_ctx*, hipStream_t, const float* x, float* out, int S, const StreamDenoise& d);
int64_t resample_out_len(int64_t n, int orig_freq, int new_freq);
int run_resample(tvc_ctx*, hipStream_t, const float* x, float* y, int rows, int64_t n, int orig_freq, int new_freq);
int stream_resample_geometry(int in_freq, int out_freq, int64_t n_in, int64_t* n_out, int* hist, int* delay);
int stream_resample_prepare(tvc_ctx*, int in_freq, int out_freq);
int run_stream_resample(tvc_ctx*, hipStream_t, const void* in, bool in16, void* out, bool out16, float* state, int S, int64_t n_in, int in_freq,
                        int out_freq, float gain_db);
int run_pcm16_to_f32(tvc_ctx*, hipStream_t, const int16_t* pcm, float* y, int64_t n, float gain_db);
int run_f32_to_pcm16(tvc_ctx*, hipStream_t, const float* x, int16_t* pcm, int64_t n, float gain_db);
void frontdoor_release(tvc_ctx*);
int run_prepare_index(tvc_ctx*, hipStream_t, const float* index, float* prepared, int64_t N);
int run_prepare_index_f16(tvc_ctx*, hipStream_t, const void* rows_f16, float* prepared, int64_t N);
// the blobs run_prepare_index / _f16 make of feats[:, cols] (feats [768][S], cols a DEVICE array of N columns), gathered in one launch;
// index_out (optional): feats[:, cols] itself, [768][N] fp32 / half
int run_prepare_index_cols(tvc_ctx*, hipStream_t, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared, float* index_out);
int run_prepare_index_cols_f16(tvc_ctx*, hipStream_t, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared, void* index_out_f16);

// k-means over the raw vectors of a prepared blob (index_compact.hip): assignment = column 0 of run_knn_topk with the points as queries, in
// chunks of kIndexAssignChunk (or the context's) query columns; update = segmented fp64 mean without floating-point atomics
constexpr int kIndexAssignChunk = 32768;
constexpr int64_t kIndexCompactMaxK = 1 << 20;
int run_index_assign(tvc_ctx*, hipStream_t, Ws&, const float* points, int64_t N, const float* cent_blob, int64_t K, int64_t* assign, float* sim_out, int32_t* moved);
int run_index_update(tvc_ctx*, hipStream_t, Ws&, const float* points, int64_t N, const int64_t* assign, int64_t K, float* centroids, int32_t* counts_out);
int run_index_compact(tvc_ctx*, hipStream_t, Ws&, const float* points, int64_t N, const int64_t* init_cols, int64_t K, int iters, float* centroids, float* prepared_out,
                      int64_t* assign_out, int32_t* counts_out, int32_t* moved_out);

// fused FilterNet kernels (filter_up24s.hip, conv48s.hip)
// (the amax_* arguments are the per-utterance |max| slots of the block-floating-point guard, split_fp16.h)
// skips[0] travels as the FiLM 1x1s' ready operand (two fp16 planes, scaled by the bound cbw |max of downs.0's input| + cbb): run_down0_split writes
// it (out_fp32: optional fp32 copy for the parity taps), run_up24_split reads it (amax_c = the slot of downs.0's INPUT)
int run_up24_split(tvc_ctx*, hipStream_t, const UpW& u, const float* x, const float* cond_planes, float cbw, float cbb, float* x1, float* out, int B, int len,
                   const float* amax_x, const float* amax_c, float* amax_x1);
int run_down0_split(tvc_ctx*, hipStream_t, const float* blob, const float* source, const float* energy, float* planes, float* out_fp32, float* y2, int B, int len,
                    const float* amax_x, float* amax_y);
int run_down24_fused(tvc_ctx*, hipStream_t, const DownW& d, const float* xi, float* out, float* y2, int B, int len, const float* amax_xi, float* amax_out);
int run_conv48s(tvc_ctx*, hipStream_t, const PackedW& w, const float* x, const PackedW* film, const float* bsc, const float* bsh, const float* cond,
                const float* res, float* out, int B, int len, int dil, const float* amax_x, const float* amax_c, float* amax_y,
                const PackedW* c5 = nullptr, float* out5 = nullptr);

int run_conv48_pair(tvc_ctx*, hipStream_t, const PackedW& wa, const PackedW& wb, const float* x, int lin, float lscale, const PackedW* film, const float* bsc,
                    const float* bsh, const float* cond, float* out, int B, int len, int da, int db, const float* amax_x, const float* amax_c,
                    float* amax_y);

// ConvNeXt-v2 layer on x [B, C, T] in place (convnext.py:49-58); tmp buffers from ws.
int run_convnext(tvc_ctx*, hipStream_t, Ws&, const ConvNeXtW& w, float* x, int B, int T, float* amax_out = nullptr);

}  // namespace tvc
