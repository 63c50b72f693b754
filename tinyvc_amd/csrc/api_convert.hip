// libtinyvc_hip.so - the conversion entries: convert_impl (the stage drivers chained), the tvc_convert*_f32 ladder with its workspace queries,
// the matches against per-row indices and the pitch stage calls.  Every entry validates, describes its call and hands it to run_walks (api.h).
#include "api.h"
#include "knn_blob.h"

using namespace tvc;

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
        // a weighted call (c.neighbours / c.width): the same search, the weighted instantiation of the merge + gather.  Its mu is a convex
        // combination of the same index rows, so every content bound below stays what it is without it.
        const KnnWeight weight{c.neighbours, c.width, nullptr};
        const KnnWeight* wt = c.neighbours || c.width ? &weight : nullptr;
        // a joined call (c.join): the weights form around the neighbour a path over each utterance chose - two launches and workspace of their
        // own in front of the gather (both walks), the same convex combination behind it
        const KnnJoin join{c.join, nullptr, nullptr};
        const KnnJoin* jn = c.join ? &join : nullptr;
        if (ix.M > 0) TVC_CHECK(run_knn_blend(ctx, s, ws, ssl, segs.data(), (int)segs.size(), ix.M, ix.weights, matched, nullptr, B, T, c.alpha, share, wt, jn));
        else TVC_CHECK(run_knn_segs(ctx, s, ws, ssl, segs.data(), (int)segs.size(), matched, nullptr, B, T, c.alpha, share, wt, jn));
    }
    ws.release(m);
    const float* idx_bound = ws.dry ? nullptr : (ix.per_row ? rowmax : blob_amax(ix.blob));
    if (mixed && !ws.dry) {
        TVC_CHECK(run_ssl_amax(ctx, s, ssl, B, T, srcmax));
        TVC_CHECK(run_knn_alpha_bound(ctx, s, c.alpha, idx_bound, ix.per_row ? 1 : 0, srcmax, abound, NB, c.protect));
    }
    if (c.snap && !ws.dry) {      // pitch correction: one wavefront per utterance over the f0 the decoder is about to read, in place (no workspace)
        std::vector<SnapRow> rows((size_t)NB);
        for (int i = 0; i < NB; ++i) rows[i] = SnapRow{ctx->rag ? ctx->rag->pre[i] : i * T, ctx->rag ? ctx->rag->tb[i] : T, ctx->rag ? ctx->rag->row[i] : i};
        TVC_CHECK(run_pitch_snap(ctx, s, f0s, rows, *c.snap, c.notes, c.strength, c.snap_carry_frame, c.snap_note, c.snap_ratio, f0s, nullptr));
    }
    TVC_CHECK(run_decoder(ctx, s, ws, matched, f0s, energy, c.angle, c.seed, c.wave, nullptr, nullptr, nullptr, B, T, mixed && !ws.dry ? abound : idx_bound, emax,
                          mixed || ix.per_row ? 1 : 0));
    ws.release(m);
    return 0;
}

extern "C" {

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

// A tvc_workspace_bytes* query by field name: the sizes of the call it plans, and which of the ladder's features the call has.
struct ConvertQuery {
    int B = 0;
    int64_t L = 0;                             // samples per row (the Lmax of a ragged query)
    const int64_t* lens = nullptr;
    bool ragged = false;
    ConvertIndex index;                        // N, or Ns and M: the blobs and weights are not looked at
    bool auto_pitch = false, alpha = false, protect = false, path = false, join = false;
};
// The tvc_workspace_bytes* query that goes with each entry: the same description with stand-in buffers, the measuring walk alone.  A
// per-row index (ix.Ns; ix.blobs is not looked at) is planned with every row a segment of its own (distinct stand-in blobs) and a shift
// table (it takes workspace; never read in this walk): a call whose rows share blobs, or without per-row shifts, needs less.
// (No allocation depends on whether the call brings its own noise phases.)
static int convert_query(tvc_ctx* ctx, const ConvertQuery& q, size_t* out_bytes, const char* what) {
    TVC_CHECK(need_ready(ctx, NEED_NONE));
    const ConvertIndex& ix = q.index;
    if (!out_bytes || (q.ragged && !q.lens) || (ix.per_row ? !ix.Ns : ix.N < 4) || q.B <= 0 || q.L <= 0 || q.L % kHop != 0)
        return fail(ctx, TVC_ERR_ARG, "%s: need B>0, %s%%480==0, %s%s", what, q.ragged ? "Lmax" : "L", q.ragged && ix.per_row ? "lens[B], " : "", ix.per_row ? "N[B]" : "N>=4");
    if (ix.M) TVC_CHECK(blend_check(ctx, q.B, ix.M, kDryPtr, what));
    const int M = ix.M > 0 ? ix.M : 1;
    if (!q.ragged && (int64_t)q.B * M * (q.L / kHop) > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: more than 2^31 - 1 query columns", what);
    for (int b = 0; ix.per_row && b < q.B * M; ++b)
        if (ix.Ns[b] < 4) return fail(ctx, TVC_ERR_ARG, "%s: N[%d] < 4", what, b);
    std::vector<const float*> blobs(ix.per_row ? (size_t)q.B * M : 0);
    for (size_t b = 0; b < blobs.size(); ++b) blobs[b] = kDryPtr + 64 * b;
    const float shift = 0.f;
    ConvertCall c;
    c.wav = c.wave = kDryPtr;
    c.B = q.B;
    c.L = q.L;
    c.lens = q.lens;
    c.index = ix.M ? ConvertIndex::blend(blobs.data(), ix.Ns, ix.M, kDryPtr) : ix.per_row ? ConvertIndex::table(blobs.data(), ix.Ns) : ConvertIndex::one(kDryPtr, ix.N);
    c.shifts = ix.per_row ? &shift : nullptr;
    c.target_f0 = q.auto_pitch ? kDryPtr : nullptr;
    c.alpha = q.alpha ? kDryPtr : nullptr;
    c.protect = q.protect ? kDryPtr : nullptr;
    c.join = q.join ? kDryPtr : nullptr;
    const tvc_pitch_path any_path = TVC_PITCH_PATH_DEFAULT;      // the settings take no part in the sizes
    c.path = q.path ? &any_path : nullptr;
    if (!q.ragged) return measure(1, out_bytes, [&](Ws& ws) { return convert_impl(ctx, nullptr, ws, c); });
    std::vector<RagBatchPlan> batches;
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, q.B, q.L, q.lens, &batches));
    return measure(kRagGranule, out_bytes, [&](Ws& ws) { return convert_ragged_batches(ctx, nullptr, ws, batches, c); });
}
// The queries of the entries that take (N, M, weights): q.index is the blend form.  M = 1 may come with weights (a one-term blend) or
// without (the multi-index call), and behind the auto entries the target registers are optional (target_optional): the largest of the
// forms the entry takes.
static int ladder_query(tvc_ctx* ctx, ConvertQuery q, bool target_optional, size_t* out_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    const ConvertIndex blend = q.index;
    TVC_CHECK(blend_check(ctx, q.B, blend.M, kDryPtr, what));
    size_t most = 0, bytes = 0;
    for (int with_target = target_optional ? 0 : 1; with_target < 2; ++with_target)
        for (int table = 0; table < (blend.M == 1 ? 2 : 1); ++table) {
            q.auto_pitch = with_target != 0;
            q.index = table ? ConvertIndex::table(nullptr, blend.Ns) : blend;
            TVC_CHECK(convert_query(ctx, q, out_bytes ? &bytes : nullptr, what));
            if (bytes > most) most = bytes;
        }
    *out_bytes = most;
    return TVC_OK;
}

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
// a call's path settings (nullable: no path), refused under the entry's own name `what` before any device work
static int path_check(tvc_ctx* ctx, const tvc_pitch_path* path, const char* what) {
    char why[96];
    if (path && pitch_path_check(*path, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "%s: path: %s", what, why);
    return 0;
}

// a call's correction settings (nullable: none), likewise
static int snap_check(tvc_ctx* ctx, const tvc_pitch_snap* snap, const char* what) {
    char why[128];
    if (snap && pitch_snap_check(*snap, why, sizeof(why)) != 0) return fail(ctx, TVC_ERR_ARG, "%s: snap: %s", what, why);
    return 0;
}

// The per-row index as a caller gives it - host tables of B * M blobs and sizes, the device weights - and what the entry asks of it
struct IndexAsGiven {
    const float* const* prepared = nullptr;
    const int64_t* N = nullptr;
    int M = 1;
    const float* weights = nullptr;            // nullptr: the multi-index call, M must be 1 - or, weights_required, refused
    bool weights_required = false;             // the blend entries
    bool target_required = false;              // the auto entries: target_f0 = NULL is refused
};
// Every conversion entry's checks, once and in one order, under the entry's own name `what`: the null context, the path settings, the
// carry, the index as given (nullptr: c.index is the entry's one shared index), the target registers where the entry requires them, the
// tracker (nullptr: none) - then convert_entry's.  Nothing is enqueued before the last of them.
static int convert_checked(tvc_ctx* ctx, void* stream, ConvertCall c, const IndexAsGiven* given, const PitchTrackState* track, bool ragged, void* wsp,
                           size_t ws_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(path_check(ctx, c.path, what));
    if (c.carry) {      // the path's state from block to block
        if (!c.path) return fail(ctx, TVC_ERR_ARG, "%s: carry needs path (the state is the pitch path's)", what);
        if (c.carry_frame < 1 || c.L / kHop <= c.carry_frame)
            return fail(ctx, TVC_ERR_ARG, "%s: carry_frame = %d must be >= 1 and below the window's %lld frames", what, c.carry_frame, (long long)(c.L / kHop));
    } else {
        c.carry_frame = 0;
    }
    TVC_CHECK(snap_check(ctx, c.snap, what));
    if (c.snap) {      // the correction: its table, and its state from block to block
        if (!c.notes) return fail(ctx, TVC_ERR_ARG, "%s: snap needs notes (a device array of %d fp32)", what, TVC_PITCH_SNAP_NOTES);
        if (!c.snap_note != !c.snap_ratio) return fail(ctx, TVC_ERR_ARG, "%s: snap_note and snap_ratio are both NULL or both given", what);
        if (c.snap_note && (c.snap_carry_frame < 1 || c.L / kHop < c.snap_carry_frame))
            return fail(ctx, TVC_ERR_ARG, "%s: snap_carry_frame = %d must be >= 1 and at most the window's %lld frames", what, c.snap_carry_frame,
                        (long long)(c.L / kHop));
    } else {
        c.notes = c.strength = nullptr;
        c.snap_note = nullptr;
        c.snap_ratio = nullptr;
    }
    if (!c.snap_note) c.snap_carry_frame = 0;
    if (given && (given->weights || given->weights_required)) {
        TVC_CHECK(blend_check(ctx, c.B, given->M, given->weights, what));
        c.index = ConvertIndex::blend(given->prepared, given->N, given->M, given->weights);
    } else if (given) {
        if (given->M != 1) return fail(ctx, TVC_ERR_ARG, "%s: weights = NULL is one index per row: M must be 1, got %d", what, given->M);
        c.index = ConvertIndex::table(given->prepared, given->N);
    }
    if (given && given->target_required && !c.target_f0) return fail(ctx, TVC_ERR_ARG, "%s: target_f0 is NULL (a device array of B registers in Hz)", what);
    if (track) {
        if (c.L <= 0 || c.L / kHop > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: bad argument (L must be a positive multiple of 480)", what);
        TVC_CHECK(track_check(ctx, c.B, (int)(c.L / kHop), *track, c.target_f0, what));
        c.track = track;
    }
    return convert_entry(ctx, stream, c, ragged, wsp, ws_bytes, what);
}

// ---- one shared index, or one per row ---------------------------------------------------------------------------------------------------
int tvc_workspace_bytes(tvc_ctx* ctx, int B, int64_t L, int64_t N, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::one(nullptr, N);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes");
}
int tvc_workspace_bytes_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, int64_t N, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::one(nullptr, N);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes_ragged");
}
int tvc_workspace_bytes_multi(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::table(nullptr, N);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes_multi");
}
int tvc_workspace_bytes_ragged_multi(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::table(nullptr, N);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes_ragged_multi");
}

int tvc_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* prepared, int64_t N,
                    float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L,
                    void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.angle = noise_angle; c.seed = seed;
    c.index = ConvertIndex::one(prepared, N);
    return convert_checked(ctx, stream, c, nullptr, nullptr, false, wsp, ws_bytes, "tvc_convert_f32");
}
int tvc_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* prepared, int64_t N,
                           float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.angle = noise_angle; c.seed = seed;
    c.index = ConvertIndex::one(prepared, N);
    return convert_checked(ctx, stream, c, nullptr, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_f32");
}
int tvc_convert_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, float pitch_shift,
                          const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    IndexAsGiven g; g.prepared = prepared; g.N = N;
    return convert_checked(ctx, stream, c, &g, nullptr, false, wsp, ws_bytes, "tvc_convert_multi_f32");
}
int tvc_convert_ragged_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave,
                                 int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    IndexAsGiven g; g.prepared = prepared; g.N = N;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_multi_f32");
}

// ---- a weighted blend of several indices per row ------------------------------------------------------------------------------------------
int tvc_workspace_bytes_blend(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, "tvc_workspace_bytes_blend"));
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes_blend");
}
int tvc_workspace_bytes_ragged_blend(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, "tvc_workspace_bytes_ragged_blend"));
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr);
    return convert_query(ctx, q, out_bytes, "tvc_workspace_bytes_ragged_blend");
}
int tvc_convert_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp,
                          size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights; g.weights_required = true;
    return convert_checked(ctx, stream, c, &g, nullptr, false, wsp, ws_bytes, "tvc_convert_blend_f32");
}
int tvc_convert_ragged_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, int M, const float* weights, float pitch_shift, const float* pitch_shifts, const float* noise_angle,
                                 uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights; g.weights_required = true;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_blend_f32");
}

// ---- automatic pitch: the shift that moves a row's register onto its target's, found on the device ------------------------------------------
// the table form of the blend entries: weights == NULL is the multi-index call and takes M = 1
int tvc_workspace_bytes_auto(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr);
    return ladder_query(ctx, q, false, out_bytes, "tvc_workspace_bytes_auto");
}
int tvc_workspace_bytes_ragged_auto(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr);
    return ladder_query(ctx, q, false, out_bytes, "tvc_workspace_bytes_ragged_auto");
}
int tvc_convert_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                         const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                         float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.target_f0 = target_f0; c.shift_out = shift_out;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights; g.target_required = true;
    return convert_checked(ctx, stream, c, &g, nullptr, false, wsp, ws_bytes, "tvc_convert_auto_f32");
}
int tvc_convert_ragged_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                const int64_t* N, int M, const float* weights, const float* target_f0, float pitch_shift, const float* pitch_shifts,
                                float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.target_f0 = target_f0; c.shift_out = shift_out;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights; g.target_required = true;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_auto_f32");
}

// ---- automatic pitch in streams: the register is the stream's history (a ring per stream on the device) ---------------------------------------
int tvc_convert_track_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift,
                          float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B,
                          int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.target_f0 = target_f0; c.shift_out = shift_out;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, &t, false, wsp, ws_bytes, "tvc_convert_track_f32");
}

// ---- alpha: a share of the source's own content features kept in the match (the reference's match_features(..., alpha)) ---------------------
// The table form of the auto entries plus `alpha` (device, one fp32 per row); alpha == NULL is the sibling call.  One ConvertCall field and one
// argument of the kNN drivers: no second path.  The target registers are optional here (shift_out goes with them), and so is the tracker
// (ring == NULL: none).
int tvc_workspace_bytes_alpha(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_alpha");
}
int tvc_workspace_bytes_ragged_alpha(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_ragged_alpha");
}
int tvc_convert_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* alpha, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count,
                          float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                          float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_convert_alpha_f32");
}
int tvc_convert_ragged_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, int M, const float* weights, const float* alpha, const float* target_f0, float pitch_shift,
                                 const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp,
                                 size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_alpha_f32");
}

// ---- protect: the alpha entries with a per-frame share - more of the source on the unvoiced frames of the f0 the call decodes --------------
// `protect` (device, one fp32 per row) behind alpha; protect == NULL is the alpha call, launch for launch; alpha == NULL with protect set: a = 0.
int tvc_workspace_bytes_protect(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_protect");
}
int tvc_workspace_bytes_ragged_protect(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_ragged_protect");
}
int tvc_convert_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            const float* alpha, const float* protect, const float* target_f0, int start, int n, int W, int min_voiced, float slew,
                            float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                            const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_convert_protect_f32");
}
int tvc_convert_ragged_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                   const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const float* target_f0,
                                   float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave,
                                   int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_protect_f32");
}

// ---- the pitch path: the protect entries with the Viterbi decode of the call's own logits in the per-frame decode's place ------------------
// `path` (host settings) behind protect; path == NULL is the protect call, launch for launch.
int tvc_workspace_bytes_path(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = q.path = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_path");
}
int tvc_workspace_bytes_ragged_path(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = q.path = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_ragged_path");
}
int tvc_convert_path_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                         const float* alpha, const float* protect, const tvc_pitch_path* path, const float* target_f0, int start, int n, int W,
                         int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts,
                         float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_convert_path_f32");
}
int tvc_convert_ragged_path_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path,
                                const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                                uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_convert_ragged_path_f32");
}
// the carry: the path entry with the path's state [B][512] on the device, read at frame 0 and written at frame carry_frame, in place.  Equal
// lengths only (streams advance in lock step); carry == NULL is the path call, launch for launch.  Workspace: tvc_workspace_bytes_path.
int tvc_convert_carry_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* alpha, const float* protect, const tvc_pitch_path* path, int carry_frame, float* carry, const float* target_f0,
                          int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift,
                          const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp,
                          size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.carry_frame = carry_frame; c.carry = carry; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_convert_carry_f32");
}

// ---- pitch correction: the carry entry and the ragged path entry with the snap stage in front of the decoder ---------------------------------
// snap (host settings), notes, strength and - equal lengths only - the state behind carry / path; snap == NULL is the sibling call, launch
// for launch.  Workspace: tvc_workspace_bytes_path / _ragged_path.
int tvc_tuned_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                          const float* alpha, const float* protect, const tvc_pitch_path* path, int carry_frame, float* carry, const tvc_pitch_snap* snap,
                          const float* notes, const float* strength, int snap_carry_frame, int32_t* snap_note, float* snap_ratio, const float* target_f0,
                          int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift,
                          const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp,
                          size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.carry_frame = carry_frame; c.carry = carry; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength; c.snap_carry_frame = snap_carry_frame; c.snap_note = snap_note; c.snap_ratio = snap_ratio;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_tuned_convert_f32");
}
int tvc_tuned_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                 const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path,
                                 const tvc_pitch_snap* snap, const float* notes, const float* strength, const float* target_f0, float pitch_shift,
                                 const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp,
                                 size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_tuned_convert_ragged_f32");
}

// ---- weighted neighbours: the tuned entries with a k of 1 .. 4 and a similarity width per row in the match ----------------------------------
// `neighbours` (device, one int32 per row) and `width` (device, one fp32 per row) behind protect, either nullable (4, +inf); both NULL is the
// tuned call, launch for launch.  One more instantiation of the merge + gather: no workspace of its own (tvc_workspace_bytes_path / _ragged_path).
int tvc_weighted_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                             const float* alpha, const float* protect, const int32_t* neighbours, const float* width, const tvc_pitch_path* path,
                             int carry_frame, float* carry, const tvc_pitch_snap* snap, const float* notes, const float* strength, int snap_carry_frame,
                             int32_t* snap_note, float* snap_ratio, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring,
                             int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                             uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.carry_frame = carry_frame; c.carry = carry; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength; c.snap_carry_frame = snap_carry_frame; c.snap_note = snap_note; c.snap_ratio = snap_ratio;
    c.neighbours = neighbours; c.width = width;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_weighted_convert_f32");
}
int tvc_weighted_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                    const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const int32_t* neighbours,
                                    const float* width, const tvc_pitch_path* path, const tvc_pitch_snap* snap, const float* notes, const float* strength,
                                    const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                                    uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength;
    c.neighbours = neighbours; c.width = width;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_weighted_convert_ragged_f32");
}

// ---- match along a path: the weighted entries with a continuity weight per row ------------------------------------------------------------------
// `join` (device, one fp32 per row) behind width; join == NULL is the weighted call, launch for launch.  The path takes workspace of its own:
// tvc_workspace_bytes_joined / _ragged_joined (the path queries with it).
int tvc_workspace_bytes_joined(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = L; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = q.path = q.join = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_joined");
}
int tvc_workspace_bytes_ragged_joined(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes) {
    ConvertQuery q; q.B = B; q.L = Lmax; q.lens = lens; q.ragged = true; q.index = ConvertIndex::blend(nullptr, N, M, nullptr); q.alpha = q.protect = q.path = q.join = true;
    return ladder_query(ctx, q, true, out_bytes, "tvc_workspace_bytes_ragged_joined");
}
int tvc_joined_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M, const float* weights,
                           const float* alpha, const float* protect, const int32_t* neighbours, const float* width, const float* join,
                           const tvc_pitch_path* path, int carry_frame, float* carry, const tvc_pitch_snap* snap, const float* notes, const float* strength,
                           int snap_carry_frame, int32_t* snap_note, float* snap_ratio, const float* target_f0, int start, int n, int W, int min_voiced,
                           float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                           const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = L; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.carry_frame = carry_frame; c.carry = carry; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength; c.snap_carry_frame = snap_carry_frame; c.snap_note = snap_note; c.snap_ratio = snap_ratio;
    c.neighbours = neighbours; c.width = width; c.join = join;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    PitchTrackState t; t.start = start; t.n = n; t.W = W; t.min_voiced = min_voiced; t.slew = slew; t.ring = ring; t.count = count; t.autos = auto_shift;
    return convert_checked(ctx, stream, c, &g, ring ? &t : nullptr, false, wsp, ws_bytes, "tvc_joined_convert_f32");
}
int tvc_joined_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* const* prepared,
                                  const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, const int32_t* neighbours,
                                  const float* width, const float* join, const tvc_pitch_path* path, const tvc_pitch_snap* snap, const float* notes,
                                  const float* strength, const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out,
                                  const float* noise_angle, uint64_t seed, float* wave, int B, void* wsp, size_t ws_bytes) {
    ConvertCall c; c.wav = wav; c.wave = wave; c.B = B; c.L = Lmax; c.lens = lens; c.shift = pitch_shift; c.shifts = pitch_shifts; c.angle = noise_angle; c.seed = seed;
    c.alpha = alpha; c.protect = protect; c.path = path; c.target_f0 = target_f0; c.shift_out = target_f0 ? shift_out : nullptr;
    c.snap = snap; c.notes = notes; c.strength = strength;
    c.neighbours = neighbours; c.width = width; c.join = join;
    IndexAsGiven g; g.prepared = prepared; g.N = N; g.M = M; g.weights = weights;
    return convert_checked(ctx, stream, c, &g, nullptr, true, wsp, ws_bytes, "tvc_joined_convert_ragged_f32");
}

// ---- the matches against one index per row or a blend: the kNN stage of the entries above on the caller's own features ---------------------
// One match by field name.  alpha (nullable): the alpha form of the same call; protect (nullable, with f0): its protect form.
struct MatchCall {
    const float* src = nullptr;                // [B][768][T]
    const float* f0 = nullptr;                 // [B][T], the protect form's voicing
    IndexAsGiven index;
    const float *alpha = nullptr, *protect = nullptr;
    KnnWeight weight;                          // the weighted form: neighbours, width, sims_out - all nullable, all null: not weighted
    KnnJoin join;                              // the joined form: join (null: not joined), anchor_out, affinity_out
    float* out = nullptr;
    int64_t* idx_out = nullptr;      // nullable
    int B = 0, T = 0;
};
// the (term, row) runs of M * B * T virtual query columns, term-major: term m of row b searches its own blob over columns [(m * B + b) * T, + T)
static std::vector<KnnSegIn> term_row_segments(const IndexAsGiven& ix, int B, int T) {
    std::vector<KnnSegIn> in;
    for (int m = 0; m < ix.M; ++m)
        for (int b = 0; b < B; ++b) in.push_back(KnnSegIn{ix.prepared[(size_t)b * ix.M + m], ix.N[(size_t)b * ix.M + m], (m * B + b) * T, T});
    return in;
}
// the stage calls' share per column: with protect set, B * T floats of workspace (both walks) filled from the caller's f0 [B][T] in front of the search
static int match_share(tvc_ctx* ctx, hipStream_t s, Ws& ws, const MatchCall& c, float** share) {
    *share = c.protect ? ws.get<float>((size_t)c.B * c.T) : nullptr;
    if (c.protect && !ws.dry) TVC_CHECK(run_frame_share(ctx, s, c.f0, c.alpha, c.protect, *share, c.B, c.T));
    return 0;
}
// one walk of a match: the share, then the search and its gather
static int match_walk(tvc_ctx* ctx, hipStream_t s, Ws& ws, const MatchCall& c, const std::vector<KnnSegIn>& in, bool blend) {
    const KnnWeight* wt = c.weight.neighbours || c.weight.width || c.weight.sims_out ? &c.weight : nullptr;
    const KnnJoin* jn = c.join.join ? &c.join : nullptr;
    float* share;
    TVC_CHECK(match_share(ctx, s, ws, c, &share));
    if (blend) return run_knn_blend(ctx, s, ws, c.src, in.data(), (int)in.size(), c.index.M, c.index.weights, c.out, c.idx_out, c.B, c.T, c.alpha, share, wt, jn);
    return run_knn_segs(ctx, s, ws, c.src, in.data(), c.B, c.out, c.idx_out, c.B, c.T, c.alpha, share, wt, jn);
}
// every match entry's checks and its two walks, under the entry's own name `what`
static int match_checked(tvc_ctx* ctx, void* stream, const MatchCall& c, void* wsp, size_t ws_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    const IndexAsGiven& ix = c.index;
    const int B = c.B, T = c.T;
    if ((c.alpha || c.protect) && c.src && c.src == c.out)
        return fail(ctx, TVC_ERR_ARG, "%s: out must be another buffer than src (the source's share is read while out is written)", what);
    if (c.protect && !c.f0) return fail(ctx, TVC_ERR_ARG, "%s: protect needs f0 (device, [B][T]: the voicing comes from it)", what);
    if (!c.join.join && (c.join.anchor_out || c.join.affinity_out))
        return fail(ctx, TVC_ERR_ARG, "%s: anchor_out and affinity_out are the path's: they need join (device, one fp32 per row)", what);
    const bool blend = ix.weights || ix.weights_required;
    if (!blend && ix.M != 1) return fail(ctx, TVC_ERR_ARG, "%s: weights = NULL is one index per row: M must be 1, got %d", what, ix.M);
    if (!c.src || !c.out || B <= 0 || T <= 0 || (!blend && (int64_t)B * T > 0x7fffffff)) return fail(ctx, TVC_ERR_ARG, "%s: bad argument", what);
    if (blend) {
        TVC_CHECK(blend_check(ctx, B, ix.M, ix.weights, what));
        if ((int64_t)B * ix.M * T > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "%s: more than 2^31 - 1 query columns", what);
    }
    hipStream_t s = (hipStream_t)stream;
    TVC_CHECK(rows_check(ctx, s, B * ix.M, ix.prepared, ix.N, what));
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    const std::vector<KnnSegIn> in = term_row_segments(ix, B, T);
    return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) { return match_walk(ctx, s, ws, c, in, blend); });
}
int tvc_knn_match_multi_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, float* out,
                            int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    MatchCall c; c.src = src; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.index.prepared = prepared; c.index.N = N;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_multi_f32");
}
int tvc_knn_match_blend_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    MatchCall c; c.src = src; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.index.prepared = prepared; c.index.N = N; c.index.M = M; c.index.weights = weights; c.index.weights_required = true;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_blend_f32");
}
int tvc_knn_match_alpha_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M, const float* weights,
                            const float* alpha, float* out, int64_t* idx_out, int B, int T, void* wsp, size_t ws_bytes) {
    MatchCall c; c.src = src; c.alpha = alpha; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.index.prepared = prepared; c.index.N = N; c.index.M = M; c.index.weights = weights;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_alpha_f32");
}
int tvc_knn_match_protect_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N, int M,
                              const float* weights, const float* alpha, const float* protect, float* out, int64_t* idx_out, int B, int T, void* wsp,
                              size_t ws_bytes) {
    MatchCall c; c.src = src; c.f0 = f0; c.alpha = alpha; c.protect = protect; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.index.prepared = prepared; c.index.N = N; c.index.M = M; c.index.weights = weights;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_protect_f32");
}
int tvc_knn_match_weighted_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N, int M,
                               const float* weights, const float* alpha, const float* protect, const int32_t* neighbours, const float* width, float* out,
                               int64_t* idx_out, float* sims_out, int B, int T, void* wsp, size_t ws_bytes) {
    MatchCall c; c.src = src; c.f0 = f0; c.alpha = alpha; c.protect = protect; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.weight.neighbours = neighbours; c.weight.width = width; c.weight.sims_out = sims_out;
    c.index.prepared = prepared; c.index.N = N; c.index.M = M; c.index.weights = weights;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_weighted_f32");
}
// the joined stage call: the weighted match with `join` behind width, and the path's own outputs behind sims_out - anchor_out (nullable,
// int32 [M][B][T]) and affinity_out (nullable, fp32 [M][B][T][4][4], frame 0's sixteen are zeros).  join == NULL is the weighted call.
// Workspace: tvc_workspace_bytes_match_joined, the largest of the forms the entry takes (B rows of L / 480 columns).
int tvc_workspace_bytes_match_joined(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes) {
    if (!ctx) return TVC_ERR_ARG;
    const char* what = "tvc_workspace_bytes_match_joined";
    TVC_CHECK(blend_check(ctx, B, M, kDryPtr, what));
    if (!out_bytes || !N || L <= 0 || L % kHop != 0 || (int64_t)B * M * (L / kHop) > 0x7fffffff)
        return fail(ctx, TVC_ERR_ARG, "%s: need B>0, L%%480==0, N[B * M], at most 2^31 - 1 query columns", what);
    for (int b = 0; b < B * M; ++b)
        if (N[b] < 4) return fail(ctx, TVC_ERR_ARG, "%s: N[%d] < 4", what, b);
    std::vector<const float*> blobs((size_t)B * M);
    for (size_t b = 0; b < blobs.size(); ++b) blobs[b] = kDryPtr + 64 * b;      // every (row, term) a segment of its own: the most a call can need
    MatchCall c; c.src = c.f0 = c.alpha = c.protect = kDryPtr; c.out = kDryPtr; c.B = B; c.T = (int)(L / kHop);
    c.join.join = kDryPtr;
    c.index.prepared = blobs.data(); c.index.N = N; c.index.M = M; c.index.weights = kDryPtr;
    const std::vector<KnnSegIn> in = term_row_segments(c.index, B, c.T);
    size_t most = 0;
    for (int blend = M == 1 ? 0 : 1; blend < 2; ++blend) {
        size_t bytes = 0;
        TVC_CHECK(measure(1, &bytes, [&](Ws& ws) { return match_walk(ctx, nullptr, ws, c, in, blend != 0); }));
        if (bytes > most) most = bytes;
    }
    *out_bytes = most;
    return TVC_OK;
}
int tvc_knn_match_joined_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N, int M,
                             const float* weights, const float* alpha, const float* protect, const int32_t* neighbours, const float* width,
                             const float* join, float* out, int64_t* idx_out, float* sims_out, int32_t* anchor_out, float* affinity_out, int B, int T,
                             void* wsp, size_t ws_bytes) {
    MatchCall c; c.src = src; c.f0 = f0; c.alpha = alpha; c.protect = protect; c.out = out; c.idx_out = idx_out; c.B = B; c.T = T;
    c.weight.neighbours = neighbours; c.weight.width = width; c.weight.sims_out = sims_out;
    c.join.join = join; c.join.anchor_out = anchor_out; c.join.affinity_out = affinity_out;
    c.index.prepared = prepared; c.index.N = N; c.index.M = M; c.index.weights = weights;
    return match_checked(ctx, stream, c, wsp, ws_bytes, "tvc_knn_match_joined_f32");
}

// ---- the pitch stage calls: the register match, the tracker, the path and the per-frame share on the caller's own f0 / logits -------------
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
// The stage call by field name; its carried form adds carry_frame, prior and carry_out (prior == carry_out == nullptr: the call as it was).
struct PitchPathCall {
    const float* logits = nullptr;
    const int64_t *row_start = nullptr, *row_count = nullptr;
    int rows = 0, carry_frame = 0;
    int64_t class_stride = 0;
    const tvc_pitch_path* path = nullptr;
    const float *prior = nullptr, *pitch_shifts = nullptr;
    float pitch_shift = 0.f;
    float *carry_out = nullptr, *f0 = nullptr, *f0_shifted = nullptr, *score_out = nullptr;
    int32_t* path_out = nullptr;
};
// both forms' checks and walks, under the entry's own name `what`
static int pitch_path_entry(tvc_ctx* ctx, void* stream, const PitchPathCall& c, void* wsp, size_t ws_bytes, const char* what) {
    if (!ctx) return TVC_ERR_ARG;
    if (!c.logits || !c.path || c.class_stride <= 0 || c.class_stride > 0x7fffffff || (!c.f0 && !c.f0_shifted && !c.path_out && !c.score_out && !c.carry_out))
        return fail(ctx, TVC_ERR_ARG, "%s: bad argument (logits, path, 0 < class_stride < 2^31 and at least one output)", what);
    TVC_CHECK(path_check(ctx, c.path, what));
    int64_t span = 0;
    TVC_CHECK(path_rows(ctx, c.row_start, c.row_count, c.rows, c.class_stride, &span, what));
    if (c.carry_out) {      // frame h must exist in every row that runs
        if (c.carry_frame < 1) return fail(ctx, TVC_ERR_ARG, "%s: carry_frame = %d must be >= 1", what, c.carry_frame);
        for (int b = 0; b < c.rows; ++b)
            if (c.row_count[b] > 0 && c.row_count[b] <= c.carry_frame)
                return fail(ctx, TVC_ERR_ARG, "%s: row %d has %lld frames: carry_out takes frame carry_frame = %d, so every non-empty row needs more", what, b,
                            (long long)c.row_count[b], c.carry_frame);
    }
    std::vector<PitchPathRow> rw((size_t)c.rows);
    for (int b = 0; b < c.rows; ++b) rw[b] = PitchPathRow{(int)c.row_start[b], (int)c.row_count[b], c.pitch_shifts ? c.pitch_shifts[b] : c.pitch_shift};
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_walks(ctx, what, wsp, ws_bytes, 1, [&](Ws& ws) {
        uint16_t* bp = ws.get<uint16_t>(pitch_path_ws_bytes(span) / sizeof(uint16_t));
        if (ws.dry) return 0;
        return run_pitch_path(ctx, (hipStream_t)stream, c.logits, (long)c.class_stride, rw, *c.path, bp, c.f0, c.f0_shifted, c.path_out, c.score_out, c.carry_frame,
                              c.prior, c.carry_out);
    });
}
int tvc_pitch_path_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows, int64_t class_stride,
                       const tvc_pitch_path* path, float pitch_shift, const float* pitch_shifts, float* f0, float* f0_shifted, int32_t* path_out,
                       float* score_out, void* wsp, size_t ws_bytes) {
    PitchPathCall c; c.logits = logits; c.row_start = row_start; c.row_count = row_count; c.rows = rows; c.class_stride = class_stride; c.path = path;
    c.pitch_shift = pitch_shift; c.pitch_shifts = pitch_shifts; c.f0 = f0; c.f0_shifted = f0_shifted; c.path_out = path_out; c.score_out = score_out;
    return pitch_path_entry(ctx, stream, c, wsp, ws_bytes, "tvc_pitch_path_f32");
}
int tvc_pitch_path_carry_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows,
                             int64_t class_stride, const tvc_pitch_path* path, int carry_frame, const float* prior, float* carry_out, float pitch_shift,
                             const float* pitch_shifts, float* f0, float* f0_shifted, int32_t* path_out, float* score_out, void* wsp, size_t ws_bytes) {
    PitchPathCall c; c.logits = logits; c.row_start = row_start; c.row_count = row_count; c.rows = rows; c.class_stride = class_stride; c.path = path;
    c.carry_frame = carry_frame; c.prior = prior; c.carry_out = carry_out;
    c.pitch_shift = pitch_shift; c.pitch_shifts = pitch_shifts; c.f0 = f0; c.f0_shifted = f0_shifted; c.path_out = path_out; c.score_out = score_out;
    return pitch_path_entry(ctx, stream, c, wsp, ws_bytes, "tvc_pitch_path_carry_f32");
}
int tvc_pitch_snap_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, const int64_t* row_count, int rows, const tvc_pitch_snap* snap,
                       const float* notes, const float* strength, int carry_frame, int32_t* note, float* ratio, float* out, int32_t* note_out) {
    const char* what = "tvc_pitch_snap_f32";
    if (!ctx) return TVC_ERR_ARG;
    if (!f0 || !snap || !notes || !out) return fail(ctx, TVC_ERR_ARG, "%s: bad argument (f0, snap, notes and out)", what);
    if (!note != !ratio) return fail(ctx, TVC_ERR_ARG, "%s: note and ratio are both NULL or both given", what);
    TVC_CHECK(snap_check(ctx, snap, what));
    int64_t span = 0;
    TVC_CHECK(path_rows(ctx, row_start, row_count, rows, 0, &span, what));
    if (note) {      // frame h - 1 must exist in every row that runs
        if (carry_frame < 1) return fail(ctx, TVC_ERR_ARG, "%s: carry_frame = %d must be >= 1", what, carry_frame);
        for (int b = 0; b < rows; ++b)
            if (row_count[b] > 0 && row_count[b] < carry_frame)
                return fail(ctx, TVC_ERR_ARG, "%s: row %d has %lld frames: the state is stored behind frame carry_frame - 1 = %d, so every non-empty row needs "
                            "at least carry_frame", what, b, (long long)row_count[b], carry_frame - 1);
    }
    std::vector<SnapRow> rw((size_t)rows);
    for (int b = 0; b < rows; ++b) rw[b] = SnapRow{(int)row_start[b], (int)row_count[b], b};
    TVC_HIP(ctx, hipSetDevice(ctx->device));
    return run_pitch_snap(ctx, (hipStream_t)stream, f0, rw, *snap, notes, strength, note ? carry_frame : 0, note, ratio, out, note_out);
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

}  // extern "C"
