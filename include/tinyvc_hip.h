/* tinyvc_hip.h — C ABI of libtinyvc_hip.so: the MI355X (gfx950) implementation of the tinyvc
 * voice-conversion inference path (encoder -> kNN match -> source-filter decoder -> SOLA).
 *
 * The reference (uthree/tinyvc) has no FFI: its boundary is the Python module surface.  Each entry
 * point below names the reference function it stands in for; the Python host package
 * (`tinyvc_amd.module.*`) re-exposes those functions with the reference's names and binds them to
 * these symbols through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every `const float*` / `float*` tensor argument is a DEVICE pointer owned by the caller
 *     (a torch tensor's data_ptr), fp32, contiguous, channels-first [B, C, T] like the reference;
 *     16-byte aligned;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all
 *     work is enqueued asynchronously on it; nothing here synchronises the device (one exception: the first use of a prepared
 *     index this process did not prepare itself reads its 24-byte header, see tvc_knn_prepare_index_f32).  Outside a stream
 *     capture the encoder forks its pitch estimator, and the decoder its harmonic oscillator and FilterNet's content-only front
 *     (the input contraction and Upsample 0's first conv), onto a context-owned side stream and joins them back onto `stream`
 *     with events before the call returns - an error return included -, so `stream` order is all a caller ever sees; equal and
 *     ragged batches alike.  The decoder's branch is joined twice: the harmonic rows in front of FilterNet's first launch, the
 *     front - which may still run beside FilterNet's first launches - in front of Upsample 0's FiLM launch.  While `stream` is being captured
 *     everything stays on `stream` (one chain replays faster than a fork inside a graph: DESIGN.md section 4).  Results do not
 *     depend on it;
 *   - stream capture: every call may be captured into a HIP graph, with two rules.  Kernel arguments are baked into the graph,
 *     so a call that draws its own noise phases (noise_angle = NULL: the seed is an argument) is refused with TVC_ERR_STATE while
 *     capturing - pass noise_angle and refill that buffer between replays.  And a prepared index must have been used (or
 *     prepared) by this process once before the capture, so that its header check does not have to synchronise;
 *   - `ws` is a caller-allocated device scratch buffer of at least tvc_workspace_bytes() bytes;
 *     the library never allocates device memory after tvc_finalize_weights();
 *   - arithmetic: fp32 in, fp32 out.  Channel contractions run on the fp16 matrix pipe with every fp32 operand split into two
 *     fp16 parts (22 significand bits, fp32-GEMM-level error); a per-utterance power-of-two scale keeps the parts inside fp16's
 *     range, so results do not depend on the loudness of the input, and one utterance's range never affects another utterance of
 *     the batch.  The scale comes from an UPPER BOUND of the tensor's largest magnitude: measured by the producing kernel's epilogue
 *     where that is free, analytic elsewhere (max |wav| bounds the energy envelope and, times the Hann window's sum, every |STFT|
 *     bin; the index's |max|, stored in the prepared blob, bounds the matched content; an l1 norm of the weights times the input's
 *     bound + the largest bias bounds a 1x1's output); inside [2^-10, 2^15) nothing is scaled, so a bound and the exact maximum give
 *     the same bits.  The whole-path calls (tvc_convert_*) and the stage calls derive them per utterance in the same way for equal
 *     and ragged batches;
 *   - return value: 0 = ok, negative = tvc_status; tvc_last_error() has the message;
 *   - one ctx per device, one host thread per ctx at a time.
 */
#ifndef TINYVC_HIP_H
#define TINYVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tvc_ctx tvc_ctx;

enum tvc_status {
    TVC_OK = 0,
    TVC_ERR_ARG = -1,        /* bad shape / null pointer / unsupported size */
    TVC_ERR_HIP = -2,        /* a HIP runtime call failed (message has the hipError string) */
    TVC_ERR_STATE = -3,      /* weights missing / not finalised */
    TVC_ERR_WORKSPACE = -4   /* workspace too small */
};

#define TVC_ABI_VERSION 1
int tvc_version(void);

/* lifecycle ------------------------------------------------------------------------------- */
int tvc_ctx_create(int hip_device, tvc_ctx** out);
void tvc_ctx_destroy(tvc_ctx* ctx);
const char* tvc_last_error(const tvc_ctx* ctx);

/* Checkpoint loading: one call per state_dict entry of encoder.pt / decoder.pt
 * (reference infer.py:34-37 `load_state_dict`; key names and shapes: SURVEY.md §2.4).
 * `host_data` is a HOST pointer to contiguous fp32; the library copies it.  After the last tensor,
 * tvc_finalize_weights() packs everything into the kernels' layouts and uploads once. */
int tvc_load_tensor(tvc_ctx* ctx, const char* state_dict_key, const float* host_data,
                    const int64_t* shape, int ndim);
/* 512-entry class->Hz table of PitchEstimator.id2freq (reference encoder.py:48-54), host fp32. */
int tvc_set_pitch_table(tvc_ctx* ctx, const float* host_freqs, int n);
int tvc_finalize_weights(tvc_ctx* ctx);

/* Scratch needed by any entry point below for a batch of B utterances of L samples (L % 480 == 0)
 * matched against an index of N vectors. */
int tvc_workspace_bytes(tvc_ctx* ctx, int B, int64_t L, int64_t N, size_t* out_bytes);

/* front end ------------------------------------------------------------------------------- */
/* module.utils.spectrogram (reference module/utils/spectrogram.py:8-15):
 * wav [B, L] -> spec [B, 961, T], T = L/480. */
int tvc_stft_mag_f32(tvc_ctx* ctx, void* stream, const float* wav, float* spec, int B, int64_t L,
                     void* ws, size_t ws_bytes);
/* module.utils.estimate_energy (reference module/utils/energy_estimation.py:9-14):
 * wav [B, L] -> energy [B, 1, L]. */
int tvc_energy_f32(tvc_ctx* ctx, void* stream, const float* wav, float* energy, int B, int64_t L,
                   void* ws, size_t ws_bytes);

/* front door ------------------------------------------------------------------------------- */
/* torchaudio.functional.resample(waveform, orig_freq, new_freq) as the entry scripts call it (reference infer.py:46,63;
 * infer_streaming.py:70): x [rows, n] -> y [rows, tvc_resample_out_len(n, ...)] with torchaudio's default Hann-windowed
 * sinc polyphase filter (lowpass_filter_width 6, rolloff 0.99).  torchaudio itself is not available to pin this against
 * (SURVEY.md 8c): the parity reference is this repository's host restatement tinyvc_amd/resample.py. */
int64_t tvc_resample_out_len(int64_t n, int orig_freq, int new_freq);
int tvc_resample_f32(tvc_ctx* ctx, void* stream, const float* x, float* y, int rows, int64_t n, int orig_freq,
                     int new_freq);
/* The streaming loop's sample conversions (reference infer_streaming.py:85-94): int16 PCM -> float / 32768 ->
 * torchaudio.functional.gain(gain_db) on the way in; gain(gain_db) -> * 32768 -> numpy's float32 -> int16 cast
 * (truncation toward zero, wrap-around outside int16) on the way out.  gain_db == 0 skips the gain multiply, as
 * torchaudio does. */
int tvc_pcm16_to_f32(tvc_ctx* ctx, void* stream, const int16_t* pcm, float* y, int64_t n, float gain_db);
int tvc_f32_to_pcm16(tvc_ctx* ctx, void* stream, const float* x, int16_t* pcm, int64_t n, float gain_db);

/* encoder --------------------------------------------------------------------------------- */
/* Encoder.infer (reference module/tinyvc/encoder.py:113-116): spec [B,961,T] ->
 * ssl [B,768,T], f0 [B,1,T]; `logits` [B,512,T] is optional (NULL to skip): Encoder.forward's
 * second output (encoder.py:108-111). */
int tvc_encoder_f32(tvc_ctx* ctx, void* stream, const float* spec, float* ssl, float* f0,
                    float* logits, int B, int T, void* ws, size_t ws_bytes);

/* PitchEstimator.decode (reference module/tinyvc/encoder.py:61-67, with id2freq :48-54 as the uploaded table):
 * logits [B,512,T] -> f0 [B,1,T] (top-4 classes, softmax over their logits, expectation of the class frequencies,
 * <= 20 Hz -> 0).  tvc_encoder_f32 runs the same kernel on its own logits. */
int tvc_pitch_decode_f32(tvc_ctx* ctx, void* stream, const float* logits, float* f0, int B, int T);

/* kNN match ------------------------------------------------------------------------------- */
/* Prepare an index for matching, once per index: index [768, N] (the [1,768,N] tensor of index.pt,
 * reference extract_index.py:58 / infer.py:49, or Generator.encode's output) -> `prepared`, a blob of
 * tvc_knn_prepared_elems(N) floats: a 256-byte header, the raw vectors row-major (the final gather) and the vectors
 * scaled by 1/(||r||+1e-6) (feature_retrieval.py:25 recomputes that on every call) split into three bf16 parts per
 * value in MFMA lane order (the similarity GEMM's operand), plus the same vectors in fp16 and their inverse norms (the
 * coarse pass of the two-stage search): 12 bytes per index element.  The layout is private to the
 * library; the blob is self-describing (magic, kind, N, the raw vectors' |max| - the decoder's bound of the matched content -,
 * format version), so every entry point below takes either kind of blob.  A blob at an address this process did not prepare
 * (a copy, a blob read back from a file) has its header read once, on its first use outside a stream capture - the one place the
 * library waits for `stream` -, and is refused (TVC_ERR_ARG) if the magic, the format version or N do not match: blobs of an
 * earlier format must be prepared again. */
int64_t tvc_knn_prepared_elems(int64_t N);
int tvc_knn_prepare_index_f32(tvc_ctx* ctx, void* stream, const float* index, float* prepared,
                              int64_t N);
/* fp16 index storage for very large indices (BASELINE.json configs[4]: 1 M vectors): `rows_f16` =
 * [N, 768] IEEE binary16, one vector per row (index.pt's tensor transposed and cast to half) -> a blob of
 * tvc_knn_prepared_elems_f16(N) floats holding the fp16 vectors in MFMA lane order and one fp32 inverse norm per
 * vector: 2 bytes per index element (1.5 GB at N = 1 M).  Matching against it computes cos = dot(q_hat, r) / (||r||+1e-6)
 * with r the fp16 values (exactly two bf16 parts each), fp32 accumulation; the k = 4 rows averaged are the fp16 values.
 * Results equal the fp32-storage path run on the same (fp16-rounded) vectors up to fp32 rounding of the similarities. */
int64_t tvc_knn_prepared_elems_f16(int64_t N);
int tvc_knn_prepare_index_f16(tvc_ctx* ctx, void* stream, const void* rows_f16, float* prepared,
                              int64_t N);
/* An index selected out of packed encoder features, prepared in one launch (reference extract_index.py:43-58: every stride-th frame of
 * each clip, concatenated, permuted, truncated - here a column list): feats [768, S] fp32 (tvc_encode_ragged_f32's ssl, or any [768, S]
 * tensor), cols a DEVICE array of N columns, each in [0, S) (a column outside is clamped into the tensor; the host's column plan refuses
 * it first) -> `prepared`, byte for byte the blob tvc_knn_prepare_index_f32 makes of feats[:, cols] (tvc_knn_prepared_elems(N) floats), and
 * optionally index_out [768, N] = feats[:, cols] itself (the tensor of index.pt; NULL = not wanted).  The _f16 form writes the blob
 * tvc_knn_prepare_index_f16 makes of feats[:, cols] transposed and cast to half (tvc_knn_prepared_elems_f16(N) floats) and
 * index_out_f16 [768, N] IEEE binary16.  The selected vectors never exist as a tensor of their own unless index_out asks for it.
 * Asynchronous on `stream`, capturable; the blob is recorded like the other prepare calls'. */
int tvc_knn_prepare_index_cols_f32(tvc_ctx* ctx, void* stream, const float* feats, int64_t S, const int64_t* cols, int64_t N,
                                   float* prepared, float* index_out);
int tvc_knn_prepare_index_cols_f16(tvc_ctx* ctx, void* stream, const float* feats, int64_t S, const int64_t* cols, int64_t N,
                                   float* prepared, void* index_out_f16);

/* The library remembers the N every blob was prepared with (by device address) and refuses calls that pass another N.  Call this
 * before the memory of a prepared blob is reused for anything else than a fresh tvc_knn_prepare_index_* (for instance a COPY of
 * another blob): an address that is recycled must not inherit the record.  (No reference counterpart: feature_retrieval.py:25-27
 * re-normalises the index on every call and keeps no prepared state.) */
int tvc_knn_forget(tvc_ctx* ctx, const float* prepared);
/* match_features(source, reference, k=4, alpha=0, metrics='cos')
 * (reference module/tinyvc/feature_retrieval.py:15-33): src [B,768,T] against one shared prepared
 * index -> out [B,768,T]; idx_out [B,T,4] int64 (nullable) = topk indices, ties -> lowest index. */
int tvc_knn_match_f32(tvc_ctx* ctx, void* stream, const float* src, const float* prepared, int64_t N,
                      float* out, int64_t* idx_out, int B, int T, void* ws, size_t ws_bytes);

/* match_features with the reference's full signature (module/tinyvc/feature_retrieval.py:15-33): the k = 1 ... 8 nearest index vectors of
 * every source frame under metric 0 = 'cos', 1 = 'IP' (inner product), 2 = 'L2' (negative Euclidean distance), out = the mean of the k RAW
 * vectors (alpha blending is the caller's one-liner here; the inference path has it inside the call: tvc_*_alpha_f32).  src [B,768,T]; index [768,N] = the raw [1,768,N] tensor of index.pt (no prepared
 * blob: this is not the inference path - that asks for k = 4, 'cos' and runs tvc_knn_match_f32 - but every other argument the reference
 * accepts, in plain fp32 on the raw vectors); out [B,768,T]; idx_out [B,T,k] int64 and sim_out [B,T,k] (nullable) = torch.topk's indices
 * and values in rank order, equal similarities by lower index.  N >= k.  Workspace: B * T * k * 8 bytes + 4096 when idx_out is NULL. */
int tvc_knn_match_general_f32(tvc_ctx* ctx, void* stream, const float* src, const float* index, int64_t N, int k, int metric,
                              float* out, int64_t* idx_out, float* sim_out, int B, int T, void* ws, size_t ws_bytes);

/* compacting an index -------------------------------------------------------------------------- */
/* A smaller index by k-means instead of truncation.  The reference has no counterpart: its recipe (extract_index.py:43-58) permutes the
 * strided frames and keeps the first `size` - a random subsample -; these calls complement it by keeping K centroids of ALL the vectors
 * (what RVC's index training and so-vits-svc's cluster model do on the host).  Points are the N raw vectors of a prepared blob of either
 * kind (for the fp16 kind: the fp16 values); centroids are an fp32 tensor [768, K], index.pt's layout.  4 <= K <= N, K <= 1 048 576.
 *   - tvc_index_assign_f32 stands in for `argmax(cosine(points, centroids))`: assign[n] (and sim_out[n], nullable) = column 0 of what
 *     tvc_knn_topk_f32 returns for src = the points as [1, 768, N] against `centroids_prepared` (an fp32-kind blob of the centroids) - the
 *     same similarity, the same tie rule (lower index), bit for bit.  The points go through that search in chunks of at most
 *     tvc_ctx_set_index_assign_chunk query columns (default 32 768; 0 restores it; a property of the context - no environment variable, no
 *     process-wide state; results do not depend on it).  moved_out (nullable, [1]) += the entries of assign_inout that changed: start
 *     assign at -1 and moved at 0 and the first call counts N.
 *   - tvc_index_update_f32 stands in for `centroids[:, k] = points[assign == k].mean(0)`: sums in fp64 in ascending point index (a
 *     cluster longer than 256 members in runs of 256, the runs' partial sums added in run order), mean = sum / count in fp64, rounded once
 *     to fp32.  A cluster without members keeps its previous centroid bit for bit (counts_out[k] = 0; counts_out [K] nullable); an assign
 *     value outside [0, K) belongs to no cluster.  No floating-point atomics: bit-identical from run to run.
 *   - tvc_index_compact_f32 is the loop: centroids[:, k] = point init_cols[k] (a DEVICE int64 [K]; a column outside [0, N) is clamped),
 *     then `iters` times (prepare the centroids, assign, update) - a fixed count, no convergence test, no host synchronisation - and one
 *     last prepare into prepared_out (tvc_knn_prepared_elems(K) floats, recorded like the prepare calls' blobs; it also serves as the
 *     loop's own centroid blob).  Outputs: centroids_out [768, K], prepared_out, and nullable assign_out [N] / counts_out [K] (what the last
 *     update used) and moved_out [iters] (points that changed cluster in each iteration; moved_out[0] = N).
 * Cosine assignment with a raw-mean update is the pair the match itself computes (a mean of raw vectors selected by cosine); it does not
 * minimise one objective monotonically: moved_out is what reports convergence.
 * Asynchronous on `stream`; not meant for stream capture.  Workspace for any of the three: tvc_workspace_bytes_index_compact. */
int tvc_ctx_set_index_assign_chunk(tvc_ctx* ctx, int max_queries);
int tvc_workspace_bytes_index_compact(tvc_ctx* ctx, int64_t N, int64_t K, size_t* out_bytes);
int tvc_index_assign_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const float* centroids_prepared, int64_t K,
                         int64_t* assign_inout, float* sim_out, int32_t* moved_out, void* ws, size_t ws_bytes);
int tvc_index_update_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const int64_t* assign, int64_t K,
                         float* centroids_inout, int32_t* counts_out, void* ws, size_t ws_bytes);
int tvc_index_compact_f32(tvc_ctx* ctx, void* stream, const float* points_prepared, int64_t N, const int64_t* init_cols, int64_t K, int iters,
                          float* centroids_out, float* prepared_out, int64_t* assign_out, int32_t* counts_out, int32_t* moved_out, void* ws,
                          size_t ws_bytes);

/* pitch shift ----------------------------------------------------------------------------- */
/* Index-sharded variant of the match (a very large speaker index split over the GPUs of a node):
 * every rank holds a prepared shard and
 *   1. tvc_knn_topk_f32: this shard's top-4 per query: sims_out [B,T,4] (cosine similarity, descending, ties ->
 *      lower index first) and idx_out [B,T,4] (LOCAL indices into the shard);
 *   2. the host all-gathers (sim, global index) and keeps the global top-4 per query (tinyvc_amd/parallel.py);
 *   3. tvc_knn_gather_slots_f32: slots [nslots,768] <- this shard's raw rows for idx[nslots] (local index, or a
 *      negative value where the row lives on another rank -> zeros); summed over ranks every slot has exactly one
 *      contributor, so the all-reduce is exact;
 *   4. tvc_knn_finish_f32: out [B,768,T] = mean of the 4 slots of each query in the single-GPU order. */
int tvc_knn_topk_f32(tvc_ctx* ctx, void* stream, const float* src, const float* prepared, int64_t N,
                     float* sims_out, int64_t* idx_out, int B, int T, void* ws, size_t ws_bytes);
int tvc_knn_gather_slots_f32(tvc_ctx* ctx, void* stream, const float* prepared, int64_t N,
                             const int64_t* idx, float* slots, int64_t nslots);
int tvc_knn_finish_f32(tvc_ctx* ctx, void* stream, const float* slots, float* out, int B, int T);

/* module.utils.shift_frequency (reference module/utils/pitch_shift.py:5-15), n elements. */
int tvc_shift_frequency_f32(tvc_ctx* ctx, void* stream, const float* f0, float* out, int64_t n,
                            float semitones);

/* The affine map of the noise phases (reference module/tinyvc/decoder.py:78: `torch.rand(N, fft_bin, Lf) * 2 * math.pi - math.pi`,
 * three tensor ops): u [n] uniform draws in [0, 1) -> u * 2 * pi - pi with the same three fp32 roundings, in place, one launch.
 * The draw itself stays the caller's (torch's generator on the device, as in the reference). */
int tvc_noise_angle_from_uniform_f32(tvc_ctx* ctx, void* stream, float* u, int64_t n);

/* decoder --------------------------------------------------------------------------------- */
/* Decoder.infer (reference module/tinyvc/decoder.py:253-257): content [B,768,T], f0 [B,1,T],
 * energy [B,1,L], noise_angle [B,961,T] = the uniform phases of decoder.py:78 in [-pi,pi)
 * (NULL -> drawn on device from `seed`; not bit-comparable with torch's CPU generator)
 * -> wave [B, L]. */
int tvc_decoder_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0,
                    const float* energy, const float* noise_angle, uint64_t seed, float* wave,
                    int B, int T, void* ws, size_t ws_bytes);
/* Stage outputs of the decoder for parity tests (any pointer may be NULL):
 * amps [B,15,T], kernel [B,961,T] (SourceNet.forward, decoder.py:126-134),
 * source [B,16,L] (Decoder.dsp, decoder.py:259-266). Same arguments as tvc_decoder_f32.
 * `wave` may be NULL too: the call then stops behind the last stage asked for - amps / kernel only = SourceNet.forward
 * alone (no DSP, no FilterNet pass), + source = up to Decoder.dsp. */
int tvc_decoder_stages_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0,
                           const float* energy, const float* noise_angle, uint64_t seed,
                           float* wave, float* amps, float* kernel, float* source, int B, int T,
                           void* ws, size_t ws_bytes);

/* FilterNet.forward (reference module/tinyvc/decoder.py:222-233): content [B,768,T], f0 [B,1,T], energy [B,1,L],
 * source [B,16,L] (Decoder.dsp's output) -> wave [B, L].  For parity tests the block outputs can be copied out:
 * skips[i] (i = 0..4, any entry or the array itself may be NULL) = the outputs of `downs[i]` (decoder.py:227-229):
 * [B,24,L], [B,48,L/5], [B,96,L/20], [B,192,L/80], [B,384,L/240]; ups[i] (i = 0..3) = the outputs of `ups[i]`
 * (decoder.py:231-232): [B,192,2T], [B,96,6T], [B,48,24T], [B,24,96T].  ups[4] does not exist in this implementation:
 * its 1x1 (c5) is folded into output_layer's k7 conv when the weights are packed, and `wave` is what checks it. */
int tvc_filter_net_f32(tvc_ctx* ctx, void* stream, const float* content, const float* f0, const float* energy,
                       const float* source, float* wave, float* const* skips, float* const* ups, int B, int T,
                       void* ws, size_t ws_bytes);

/* Decoder.dsp (reference module/tinyvc/decoder.py:259-266): f0 [B,1,T], amps [B,15,T],
 * kernel [B,961,T], noise_angle as above -> source [B,16,L] (15 harmonics + filtered noise). */
int tvc_dsp_f32(tvc_ctx* ctx, void* stream, const float* f0, const float* amps, const float* kernel,
                const float* noise_angle, uint64_t seed, float* source, int B, int T, void* ws,
                size_t ws_bytes);

/* whole path ------------------------------------------------------------------------------ */
/* Generator.convert (reference module/infer/generator.py:26-34): wav [B, L] (already padded to
 * L % 480 == 0, autopad_waveform is a host-side zero pad) -> wave [B, L]. */
int tvc_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* prepared_index,
                    int64_t N, float pitch_shift, const float* noise_angle, uint64_t seed,
                    float* wave, int B, int64_t L, void* ws, size_t ws_bytes);

/* Generator.convert over a RAGGED batch (the reference converts the files of a directory one by one: infer.py:60-66; padding
 * them to a common length would change results - GRN and the phase scan run over the whole time axis, convnext.py:31-34).
 * wav / wave [B, Lmax] row-major, utterance b occupies its first lens[b] samples (lens[b] % 480 == 0, 960 < lens[b] <= Lmax; the
 * tail of a wave row is zero-filled); noise_angle [B, 961, Lmax/480] (utterance b uses its first lens[b]/480 frames) or NULL.
 * `lens` is a HOST array (lengths are launch geometry; they travel to the device as kernel arguments, asynchronously on `stream`).
 * The utterances share every kernel launch - the kernels take per-utterance lengths (csrc/ragged.h) -, in at most four batches per
 * call by length class (frames < 11, < 43, < 128, the rest: the kernels a FilterNet level runs depend on the utterance's length there),
 * one after the other on `stream`.  Every utterance gets exactly the samples a B = 1 tvc_convert_f32 call gives it for the same noise
 * phases.  With noise_angle = NULL the library draws them itself: the phase of (row b, bin, frame) is a hash of `seed` and of those three
 * numbers alone - independent of the other utterances, of their lengths and of the split into batches -, so row b of a ragged call equals row
 * b of an equal-length call with the same seed over its own frames, and row 0 the B = 1 call.  A single
 * utterance may be up to 80 000 frames.  Workspace: tvc_workspace_bytes_ragged. */
int tvc_workspace_bytes_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, int64_t N, size_t* out_bytes);
/* Which utterances of a ragged call share their kernel launches: batch_of_row[b] = the in-kernel batch (0 .. *n_batches - 1, the order they
 * run in) that utterance b is converted in.  Pure host logic, no context, no device: the split tvc_convert_ragged_f32 makes (length classes
 * at 11 / 43 / 128 frames, at most `max_frames` frames per batch; 0 or anything above 80 000 = the default, 80 000 - pass what the context
 * that will convert was given by tvc_ctx_set_ragged_batch_frames).  Returns TVC_ERR_ARG for a length the ragged call would refuse. */
int tvc_ragged_plan(int B, int64_t Lmax, const int64_t* lens, int max_frames, int32_t* batch_of_row, int* n_batches);
/* Frames per in-kernel batch of THIS context's ragged calls (0 or anything above 80 000 = the default, 80 000): a smaller cap cuts a length
 * class into several batches, one after the other.  Results do not depend on it (every utterance equals its B = 1 conversion);
 * tvc_workspace_bytes_ragged and tvc_convert_ragged_f32 of the context follow it, so set it between calls (one host thread per ctx at a time).
 * (The tests use it to reach the several-batches-per-class path with small inputs; there is no environment variable and no process-wide state behind it.) */
int tvc_ctx_set_ragged_batch_frames(tvc_ctx* ctx, int max_frames);
int tvc_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, const float* prepared_index,
                           int64_t N, float pitch_shift, const float* noise_angle, uint64_t seed, float* wave, int B, void* ws,
                           size_t ws_bytes);

/* Generator.encode (reference module/infer/generator.py:19-23) over a RAGGED batch - the clips of a target speaker, which
 * extract_index.py:47-52 encodes one by one: wav [B, Lmax] as in tvc_convert_ragged_f32 (lens a HOST array, lens[b] % 480 == 0,
 * 960 < lens[b] <= Lmax) -> ssl [768, S] and f0 [S] with S = sum(lens[b] / 480), packed as ONE long utterance (csrc/ragged.h): utterance b
 * occupies columns pre[b] .. pre[b] + lens[b] / 480 (pre = the exclusive prefix of the frame counts in the caller's row order), row stride S,
 * however the call is cut into in-kernel batches (at most 80 000 frames, or tvc_ctx_set_ragged_batch_frames; no length classes: the
 * encoder's kernels choose nothing by an utterance's length).  Utterance b's columns are bit-identical to tvc_stft_mag_f32 +
 * tvc_encoder_f32 on it alone (B = 1): the spectrogram's |max| slot is the measured per-utterance maximum, as in those calls.
 * Asynchronous on `stream`, capturable.  Workspace: tvc_workspace_bytes_encode_ragged. */
int tvc_workspace_bytes_encode_ragged(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, size_t* out_bytes);
int tvc_encode_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens, float* ssl, float* f0,
                          int B, void* ws, size_t ws_bytes);

/* one speaker index per utterance ----------------------------------------------------------- */
/* The calls above with a TABLE of prepared indices instead of one: prepared[b] (a device blob) and N[b] are HOST arrays of B entries,
 * row b of the batch searches prepared[b] (the reference's form: match_features(source [B,768,T], reference [B,768,N]) is a bmm over the
 * batch, feature_retrieval.py:15-33).  Blobs may differ in size and storage (fp32 / fp16), rows may share a blob.
 *   - segments: a maximal run of consecutive query columns that search one blob is a segment (an equal-length batch: rows b..b' with one
 *     blob; a ragged batch: the utterances of an in-kernel batch in its order).  Every pass of the search is ONE launch over all segments'
 *     work units, a query tile never crosses a segment, and each segment has its own candidate-overflow flag: a segment takes exactly the
 *     path its own B = 1 call takes.  A table whose rows all share one blob is one segment and launches what tvc_convert_f32 launches.
 *   - per-row contract: row b is bit-identical to the single-index call (tvc_knn_match_f32 / tvc_convert_f32 / tvc_convert_ragged_f32)
 *     with B = 1, prepared[b], the row's noise phases and its pitch shift - including the decoder's fp16-split scales, which take row b's
 *     bound from prepared[b]'s own |max|.
 *   - pitch_shifts: a HOST array of B semitone shifts (or NULL: every row takes pitch_shift).  The shift belongs to the (source, target)
 *     pair, so a batch of different targets takes one per row.
 *   - every entry is checked like the single-index calls' blob (non-null, N[b] >= 4, the N it was prepared for; a blob this process did not
 *     prepare has its header read once, outside a capture only); nothing is launched when any entry fails (TVC_ERR_ARG).
 *   - capture: the segment table, the per-row bounds' sources and the shifts travel as kernel ARGUMENTS (no host synchronisation), so a
 *     captured graph replays the table of the call it recorded - re-capture when the table changes.  The seeded-draw rule still holds.
 * Workspace: tvc_workspace_bytes_multi / _ragged_multi (they assume every row has a blob of its own: enough for any sharing). */
int tvc_knn_match_multi_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N,
                            float* out, int64_t* idx_out, int B, int T, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_multi(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, size_t* out_bytes);
int tvc_convert_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N,
                          float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave,
                          int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_ragged_multi(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, size_t* out_bytes);
int tvc_convert_ragged_multi_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                 const float* const* prepared, const int64_t* N, float pitch_shift, const float* pitch_shifts,
                                 const float* noise_angle, uint64_t seed, float* wave, int B, void* ws, size_t ws_bytes);

/* a weighted blend of several speaker indices ------------------------------------------------ */
/* The multi-index calls above with M prepared indices ("terms") per row and a weight for each: the usual voice morph of kNN-based conversion
 * (an interpolation slider between two targets, a blend of several enrolments of one speaker, extrapolation away from a speaker with a
 * negative weight).  The reference has no counterpart: its match_features(source, reference) takes one index per row
 * (feature_retrieval.py:15-33); staged, a blend is one match per term and a tensor sum.  1 <= M <= TVC_BLEND_MAX.
 *   - prepared / N: HOST arrays of B * M entries, row-major [B][M]: term m of row b is prepared[b * M + m], a blob of either kind with
 *     N[b * M + m] >= 4 vectors.  Rows and terms may share blobs.
 *   - weights: a DEVICE array of B * M floats, row-major [B][M], in the caller's row order.  The kernels read it when they run; the host
 *     never does.  Weights may be negative or zero and are not normalised by the library; a zero-weight term is still searched (the host
 *     cannot see the weights) and contributes +0; a non-finite weight gives non-finite output.
 *   - every query column:  mu_m = (((r0 + r1) + r2) + r3) * 0.25f   (term m's four nearest raw rows: exactly what tvc_knn_match_f32 writes
 *                                                                     for that blob)
 *                          out  = w_0 * mu_0;  out = out + w_m * mu_m  for m = 1 .. M - 1
 *     products and sums rounded separately (no fused multiply-add), in term order.  Each term's four rows are what the single-index search
 *     returns for that (row, blob) - the two-stage search or the exact kernel by that blob's own size, with its own overflow fallback: the
 *     segments of the multi-index calls are here the (term, row) runs, every pass of the search still ONE launch for the whole call (the
 *     search cost grows about M-fold: M * B * T query columns).  The per-term matched tensors never exist in memory.
 *   - the decoder's content bound of row b is sum_m |w[b][m]| * (|max| of term m's blob), computed on the device in term order.  With M = 1
 *     and w = 1 a call is bit-identical to its multi-index sibling; with weights (1, 0) to the call against the first terms alone.
 *   - idx_out (tvc_knn_match_blend_f32, nullable): [M][B][T][4] int64, term m's indices of row b.
 *   - pitch_shift / pitch_shifts, noise_angle / seed, lens: as in the multi-index calls.
 *   - every table entry is checked like theirs (non-null, N >= 4, the N it was prepared for), 1 <= M <= TVC_BLEND_MAX and weights non-null;
 *     nothing is launched when any check fails (TVC_ERR_ARG).
 *   - capture: the tables travel as kernel ARGUMENTS, the weights are read from the caller's device array at replay time - changing the
 *     weights in place needs NO re-capture, changing the tables does.  The seeded-draw rule still holds.
 * Workspace: tvc_workspace_bytes_blend / _ragged_blend (N: the host table of B * M sizes; they assume every entry is a blob of its own). */
#define TVC_BLEND_MAX 4
int tvc_knn_match_blend_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M,
                            const float* weights, float* out, int64_t* idx_out, int B, int T, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_blend(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                          const float* weights, float pitch_shift, const float* pitch_shifts, const float* noise_angle, uint64_t seed,
                          float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_ragged_blend(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_ragged_blend_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                 const float* const* prepared, const int64_t* N, int M, const float* weights, float pitch_shift,
                                 const float* pitch_shifts, const float* noise_angle, uint64_t seed, float* wave, int B, void* ws,
                                 size_t ws_bytes);

/* automatic pitch: the target speaker's register, matched on the device ------------------------ */
/* The kNN match replaces timbre only: every frame of the source's f0 reaches the decoder as it is, shifted by a number of semitones the
 * caller has to guess.  "Auto pitch" moves the source's median f0 onto the target's.  The source's f0 exists only inside the fused call,
 * behind the encoder, so the shift is found there, by one launch, without a host synchronisation (capturable).
 *   - register of a row of f0: the LOWER median of its voiced frames, torch.median(row[row > 0]) - the element of rank (n_voiced - 1) / 2
 *     among the values > 0; zeros, negatives and NaN are unvoiced.  An order statistic of fp32 values (a radix select over the bit
 *     pattern, one workgroup per row): exact and bit-defined, no floating-point sum, independent of grid and order.  A row without a voiced
 *     frame reports median 0 and voiced 0.
 *   - shift[b] = offset[b] + 12 * log2(target_f0[b] / median[b]), evaluated in fp64 and rounded once to fp32; offset[b] = pitch_shifts[b],
 *     or pitch_shift when pitch_shifts is NULL (HOST values: they travel as kernel arguments).  shift[b] = offset[b] exactly when the row has
 *     no voiced frame, target_f0[b] <= 0 or NaN, or target_f0 is NULL.
 *   - f0_shifted[n] = tvc_shift_frequency_f32(f0[n], shift[b]) for every column n of row b, same arithmetic, same launch.
 * tvc_pitch_match_f32, the stage call: f0 (device) holds the rows as runs of columns, row b = [row_start[b], row_start[b + 1]) with row_start
 * a HOST array of rows + 1 ascending column numbers below 2^31 (an equal batch [B][T]: b * T; a packed ragged encode: its prefix; one long row:
 * {0, S}; an empty row is unvoiced).  target_f0 (device, rows floats in Hz) may be NULL: the call then only measures.  Outputs (device, each
 * may be NULL, not all): median_out [rows], voiced_out [rows] int32, shift_out [rows], f0_shifted (f0's layout; columns outside every row
 * are not written).  Rows of 28 frames and of millions go through the same kernel; no workspace.
 * tvc_convert_auto_f32 / tvc_convert_ragged_auto_f32: the table form of the blend entries - prepared / N are HOST arrays [B][M], weights the
 * DEVICE array [B][M], or NULL with M = 1: the multi-index call - with target_f0 (device, B registers in Hz, read when the kernels run: a
 * captured graph follows in-place changes) and shift_out (device, B floats, nullable: the shifts applied).  pitch_shift / pitch_shifts become
 * the offset on top of the automatic shift.  Row b is bit-identical to the multi-index / blend call given shift_out[b] as its host shift.
 * Everything else - checks, lens, noise_angle / seed, capture - as in those calls.  Workspace: tvc_workspace_bytes_auto / _ragged_auto
 * (N: the host table of B * M sizes). */
int tvc_pitch_match_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, int rows, const float* target_f0,
                        float pitch_shift, const float* pitch_shifts, float* median_out, int32_t* voiced_out, float* shift_out,
                        float* f0_shifted);
int tvc_workspace_bytes_auto(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                         const float* weights, const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out,
                         const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_ragged_auto(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_ragged_auto_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                const float* const* prepared, const int64_t* N, int M, const float* weights, const float* target_f0,
                                float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                                float* wave, int B, void* ws, size_t ws_bytes);

/* automatic pitch in streams: a per-stream pitch tracker on the device -------------------------- */
/* A streaming block's window is 28 frames, so its own median jumps from block to block: a stream's register is a statistic over its
 * HISTORY, kept on the device (thousands of streams in one call, one captured graph per block, no host synchronisation).
 * State, device tensors owned by the caller, one set per set of S streams that advance in lock step:
 *   ring [S][W] fp32  - the last W voiced f0 values of each stream, as a ring; unwritten slots are 0.0, so a row's live entries are
 *                       exactly its entries > 0.  1 <= W <= TVC_PITCH_TRACK_MAX_WINDOW (a row fits LDS: one code path).
 *   count [S] int64   - voiced frames appended since the last reset: the write cursor is count % W, the fill min(count, W)
 *   auto_shift [S] fp32 - the automatic part of the shift applied in the latest block
 * All zero = a fresh stream.  One block, one launch of one 256-thread workgroup per stream, no workspace, no floating-point atomics; the
 * host values T, start, n (0 <= n <= 256, start + n <= T), W, min_voiced >= 1, slew >= 0 (+inf allowed) and the offsets travel as kernel
 * arguments (baked into a capture); f0, target_f0 and the state are read when the kernel runs.  For every stream s:
 *   1. x_k = f0[s][start + k], k = 0 .. n - 1; a frame is voiced iff x_k > 0 (zero, negatives and NaN are not: tvc_pitch_match_f32's rule)
 *   2. the voiced x_k go into the ring in ascending k at ring[s][(count + j) % W], j = 0, 1, ..; then count += nv.  The result equals
 *      appending them one at a time: with nv > W only the last W survive.
 *   3. fill = min(count, W); median = the lower median of the fill live entries (rank (fill - 1) / 2; torch.median bit for bit; 0 when empty)
 *   4. wanted = (fill >= min_voiced && target_f0[s] > 0) ? (float)(12 * log2((double)target_f0[s] / (double)median)) : 0.f
 *   5. a = auto_shift[s], d = wanted - a (fp32): if !(|d| > slew) a = wanted (it lands exactly) else a = a + copysignf(slew, d);
 *      auto_shift[s] = a.  slew is in semitones per call; +inf never limits, 0 never moves.
 *   6. shift[s] = offset[s] + a, one fp32 add; offset[s] = pitch_shifts[s], or pitch_shift when pitch_shifts is NULL (HOST values)
 *   7. f0_shifted[s][t] = tvc_shift_frequency_f32(f0[s][t], shift[s]) for all T columns, in the same launch.
 * tvc_pitch_track_f32, the stage call over a caller's f0 [S][T] (device).  Outputs (device, each may be NULL): median_out [S], count_out [S]
 * int64 (= count), shift_out [S], f0_shifted [S][T].  Every argument is checked before any device work.
 * tvc_convert_track_f32: tvc_convert_auto_f32 (equal lengths; one index per row, or a blend with weights) with the tracker in the place of
 * the per-call register: B = S streams, T = L / 480, and row b's shift is step 6's.  target_f0, shift_out, noise and capture rules as in
 * tvc_convert_auto_f32; row b is bit-identical to the multi-index / blend call given shift_out[b] as its host shift.  Workspace:
 * tvc_workspace_bytes_auto (the tracker takes none).  There is no ragged form: streams advance in lock step. */
#define TVC_PITCH_TRACK_MAX_WINDOW 8192
int tvc_pitch_track_f32(tvc_ctx* ctx, void* stream, const float* f0, int S, int T, int start, int n, const float* target_f0,
                        float pitch_shift, const float* pitch_shifts, int W, int min_voiced, float slew, float* ring, int64_t* count,
                        float* auto_shift, float* median_out, int64_t* count_out, float* shift_out, float* f0_shifted);
int tvc_convert_track_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                          const float* weights, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring,
                          int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                          const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* ws, size_t ws_bytes);

/* alpha: a share of the source's own content features ------------------------------------------- */
/* The reference's match_features(source, reference, k=4, alpha=0.0) ends in `result * (1 - alpha) + input_data * alpha`
 * (feature_retrieval.py:33): the share of the source's own features that survives the match (RVC's "index rate" is its complement).  In the
 * fused conversion the encoder's output and the matched tensor exist only inside the call, so the blend happens there, per row:
 *   - alpha: a DEVICE array of B floats in the caller's row order, read when the kernels run (the host never reads it): a captured graph
 *     follows an in-place change without a new capture.  Neither clamped nor normalised: any finite value is legal, values below 0 or above 1
 *     extrapolate, a non-finite value gives non-finite output.  alpha == NULL is legal and IS the sibling call: the same launches, the same
 *     bits (tvc_knn_match_multi_f32 / _blend_f32; tvc_convert_multi / _blend / _auto / _track_f32 and their ragged forms).
 *   - every element of a query column of row b, with a = alpha[b], mu = what the alpha-less call writes there (the mean of the four rows, or
 *     the accumulated blend) and src = the same element of the tensor that was searched:
 *         keep = 1 - a;   out = mu * keep + src * a
 *     three separate fp32 roundings after the subtraction, no fused multiply-add: the bits of torch's eager `mu * (1 - a_t) + src * a_t`.
 *     The indices found do not depend on alpha.  One launch: the alpha forms of the merge + gather kernels read src where they store.
 *   - the decoder's content bound of row b becomes |keep| * (the alpha-less call's bound: the blob's |max|, or the blend bound) + |a| * (the
 *     measured |max| of utterance b's own encoder output; per utterance in a ragged batch), products and sum rounded separately.  At a = 0
 *     it is the alpha-less bound exactly: such a row has the scales, and the bits, of the alpha-less call.
 *   - per-row contract: row b is bit-identical to its own B = 1 call with alpha[b].
 * tvc_knn_match_alpha_f32, the stage call: the table form - prepared / N HOST arrays [B][M], weights the DEVICE array [B][M], or NULL with
 * M = 1 (one index per row) -, out [B,768,T] (another buffer than src), idx_out (nullable) [M][B][T][4] as the blend call's.
 * tvc_convert_alpha_f32: tvc_convert_track_f32's arguments plus alpha (behind weights).  ring == NULL: no tracker (start, n, W, min_voiced,
 * slew, count, auto_shift are not looked at) - tvc_convert_auto_f32's behaviour; target_f0 == NULL as well: plain host shifts (shift_out is
 * not written) - tvc_convert_multi_f32's / _blend_f32's.  tvc_convert_ragged_alpha_f32: tvc_convert_ragged_auto_f32's arguments plus alpha,
 * target_f0 nullable in the same way.  Every host check runs before any device work, as in the siblings; all three are capturable under
 * their rules.  Workspace: tvc_workspace_bytes_alpha / _ragged_alpha (N: the host table of B * M sizes; enough with or without target_f0,
 * a tracker or alpha). */
int tvc_knn_match_alpha_f32(tvc_ctx* ctx, void* stream, const float* src, const float* const* prepared, const int64_t* N, int M,
                            const float* weights, const float* alpha, float* out, int64_t* idx_out, int B, int T, void* ws,
                            size_t ws_bytes);
int tvc_workspace_bytes_alpha(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                          const float* weights, const float* alpha, const float* target_f0, int start, int n, int W, int min_voiced,
                          float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts,
                          float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* ws,
                          size_t ws_bytes);
int tvc_workspace_bytes_ragged_alpha(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_ragged_alpha_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                 const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                 const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out,
                                 const float* noise_angle, uint64_t seed, float* wave, int B, void* ws, size_t ws_bytes);

/* protect: a per-frame share of the source from the call's own f0 -------------------------------- */
/* A per-row alpha keeps the source's features on every frame alike.  RVC's `protect` keeps more of them on UNVOICED frames only - consonants,
 * breaths, silence, where the kNN match has least to offer - and leaves voiced frames fully converted.  Here it is a second per-row value
 * beside alpha.  Definition, over ONE utterance of T frames (a ragged batch: the utterance's own T_b frames; a stream: the window's frames):
 *   - voicing flag u[t] = f0[t] > 0 ? 1 : 0, f0 the f0 this call's encoder decodes, before any shift (the stage calls: the caller's f0); NaN
 *     and negative values count as unvoiced.
 *   - voicing weight v[t] = (u[t-1] + 2 u[t] + u[t+1]) / 4 with u[-1] = u[0] and u[T] = u[T-1]: neighbours never cross into another
 *     utterance, row or stream.  w[t] = 1 - v[t] takes only the values {0, .25, .5, .75, 1}, all exact in fp32.
 *   - with a = alpha[row] (alpha == NULL: 0) and p = protect[row], the frame's share is a_t = a + (1 - a) * (p * w[t]) - torch's eager
 *     expression on fp32 tensors, every operation rounded separately (one subtraction, two products, one sum; no fused multiply-add).
 *   - every element of the frame's query column is then stored as out = mu * (1 - a_t) + src * a_t, rounded exactly as the alpha form rounds.
 * So: on a fully unvoiced frame (w = 1) the match keeps the share (1 - a)(1 - p) - RVC's composition of index rate and protect with
 * p = 1 - (RVC's protect value), as a = 1 - (RVC's index rate); p = 0 is the alpha call bit for bit (and with alpha NULL or 0 the plain
 * call's bits); a fully voiced neighbourhood (w = 0) is untouched by p; a = 0, p = 1, w = 1 stores the source's bits; the indices do not
 * depend on p.  protect is meant for [0, 1]; like alpha it is neither clamped nor normalised and any finite value is computed as defined.
 * The 3-tap weight is a guess at a useful smoothing, not a tuned one: nobody has listened to any setting.
 * The decoder's content bound stays per utterance: with a_u = a + (1 - a) * p (the same roundings; every a_t lies between a and a_u because
 * rounding is monotonic) it is max(|1 - a|, |1 - a_u|) * (the index's bound) + max(|a|, |a_u|) * (the measured |max| of the utterance's own
 * encoder output), products and sum rounded separately - at p = 0 the alpha call's bound exactly, so such rows keep its scales and bits.
 * alpha and protect are DEVICE arrays of one fp32 per caller's row, read when the kernels run (a captured graph follows in-place changes).
 * tvc_convert_protect_f32 / tvc_convert_ragged_protect_f32: the alpha entries' arguments plus `protect` behind alpha.  protect == NULL is the
 * alpha call, launch for launch (and with alpha NULL too its sibling); alpha == NULL with protect set means a = 0.  Table and blend forms,
 * target_f0 and the tracker as there.  One more launch (one thread per query column writes a_t into B * T floats of workspace) in front of
 * the search, and the per-column instantiation of the merge + gather kernels.  Workspace: tvc_workspace_bytes_protect / _ragged_protect
 * (enough with or without alpha, protect, target_f0 and a tracker).  Per-row contract: row b is bit-identical to its own B = 1 call.
 * tvc_knn_match_protect_f32, the stage call: tvc_knn_match_alpha_f32 with f0 [B][T] (device, behind src; needed when protect is set) and
 * protect behind alpha.
 * tvc_frame_share_f32: the a_t kernel alone over packed rows, row i = columns [row_start[i], row_start[i] + row_count[i]) of f0 and of
 * share_out (HOST arrays of `rows` entries, below 2^31; an empty row writes nothing; columns outside every row are not written); alpha
 * (nullable = 0) and protect are device arrays of `rows` floats.  No workspace. */
int tvc_workspace_bytes_protect(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                            const float* weights, const float* alpha, const float* protect, const float* target_f0, int start, int n, int W,
                            int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift, float pitch_shift,
                            const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B,
                            int64_t L, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_ragged_protect(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_ragged_protect_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                   const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                   const float* protect, const float* target_f0, float pitch_shift, const float* pitch_shifts,
                                   float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* ws,
                                   size_t ws_bytes);
int tvc_knn_match_protect_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared,
                              const int64_t* N, int M, const float* weights, const float* alpha, const float* protect, float* out,
                              int64_t* idx_out, int B, int T, void* ws, size_t ws_bytes);
int tvc_frame_share_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, const int64_t* row_count, int rows,
                        const float* alpha, const float* protect, float* share_out);

/* the pitch path: a Viterbi decode of the pitch logits ------------------------------------------------------------------------ */
/* tvc_pitch_decode_f32 decodes every frame on its own: the four largest logits need not be neighbours (mass split between a class and the
 * class an octave above leaves at 1.5 times the pitch), class 0 (unvoiced, 0 Hz) in the four drags a frame down, and nothing ties frame t to
 * frame t - 1.  The pitch path is the decode every neural pitch tracker offers for this (CREPE's viterbi): the best sequence of classes under
 * a cost for moving.  It takes the per-frame decode's place when a call asks for it; without it every call is what it was.
 * It runs over ONE utterance of T frames (a ragged batch: the utterance's own T_b frames; a stream: the window's frames) and never crosses
 * rows.  Settings, a HOST struct (the values travel as kernel arguments and are baked into a capture):
 *   step >= 0, finite        cost per class of distance inside the band
 *   band W, 0 .. 32          classes a voiced frame may move at `step` each (48 classes are one octave)
 *   jump >= W * step         cost of any longer move between voiced classes; +inf is allowed
 *   voicing >= 0             cost of a move between class 0 and a voiced class; +inf is allowed
 *   refine r, 0 .. 4         the frequency is a local expectation over the classes within r of the path's
 * Everything is fp32 and every operation is rounded on its own (no fused multiply-add).  x = the logit of class j at frame t:
 *   - emission e_t[j] = x clamped to [-1e30, 1e30], NaN -> -1e30: everything stays finite.
 *   - cost(i, j) = 0 for i = j = 0; voicing when exactly one of i, j is 0; (float)|i - j| * step when both are >= 1 and |i - j| <= W; jump when
 *     both are >= 1 and further apart.
 *   - u_0[j] = e_0[j].  For every t: m_t = max_j u_t[j], s_t[j] = u_t[j] - m_t (the normalisation keeps a five-minute row at full precision).
 *   - t >= 1: cand(i -> j) = s_{t-1}[i] - cost(i, j); best_t[j] = max_i cand; bp_t[j] = the LOWEST i that attains it; u_t[j] = best_t[j] + e_t[j].
 *   - path[T-1] = the lowest argmax of s_{T-1}; path[t-1] = bp_t[path[t]].
 *   - frequency, c = path[t]: c = 0 gives f0[t] = 0.  Otherwise, over the window j in [max(1, c - r), min(511, c + r)]: d_j = e_t[j] - (the
 *     window's maximum) - the clamped emission, so the frequency is finite too -, w_j = (float)exp((double)d_j) (tvc_pitch_decode_f32's exp),
 *     den = the sum of w_j in ascending j, f0[t] = sum_j (w_j / den) * freq[j] in ascending j - quotient, product and sum rounded separately -,
 *     then tvc_pitch_decode_f32's `<= 20 -> 0` gate.  r = 0 gives freq[c] exactly.
 *   - step = jump = voicing = 0 is the per-frame argmax, lowest class on equal logits.
 * jump >= W * step is what lets the kernel take the far candidates from ONE per-frame reduction - the maximum, and its lowest class, of
 * s[i] - jump over the voiced classes: rounding is monotone, so a class inside the band never does better by the jump route, and the
 * lowest-class rule survives when the two results are combined as `min` on equal values (tests/helpers_pitch_path.py holds both forms equal).
 * TVC_PITCH_PATH_DEFAULT: step 0.5, band 12, jump 12, voicing 3, refine 2 - 48 classes per octave and 20 ms frames make the band 3 semitones
 * per frame.  THESE ARE GUESSES: nobody has listened to any setting.
 * Kernel: one workgroup of 512 threads per utterance, two barriers per frame, uint16 back-pointers [columns][512] in workspace, the walk back
 * and the frequencies in the same launch; no floating-point atomics, no host synchronisation; rows of 1 frame and of 15 000 take one path.
 * tvc_pitch_path_f32, the stage call: row i = columns [row_start[i], row_start[i] + row_count[i]) (HOST arrays of `rows` entries, ascending
 * and apart, ends below 2^31; an empty row writes nothing; columns outside every row are not written).  class_stride S: class j of column n
 * lies at logits[(n / S) * 512 * S + j * S + n % S] - an equal batch [B][512][T] has S = T, a packed ragged [512][Ttot] has S = Ttot - and no
 * row straddles a multiple of S.  pitch_shift, or pitch_shifts (HOST, one per row), is the shift of f0_shifted.  Outputs (device, each may
 * be NULL, not all): f0 and f0_shifted (one per column), path_out (int32, one per column), score_out [rows][512] = s_{T-1} (an empty row's is
 * not written).  Workspace: tvc_workspace_bytes_pitch_path (1 KiB per column up to the last row's end).
 * tvc_convert_path_f32 / tvc_convert_ragged_path_f32: the protect entries' arguments plus `path` behind protect.  path == NULL is the protect
 * call, launch for launch and bit for bit.  With it the call keeps the encoder's logits, runs the path kernel directly behind the encoder (one
 * launch per 256 utterances) and everything that reads f0 - the voicing weight of protect, the automatic shift, a tracker, the shift, the
 * decoder - reads the path's.  Workspace: tvc_workspace_bytes_path / _ragged_path (enough with or without any of the optional arguments).
 * THE CARRY: the path's state from one stream block to the next.  Two optional per-row device arrays of 512 fp32, `prior` (read) and
 * `carry_out` (written), and a host integer carry_frame = h >= 1.
 *   - prior: p_j = prior[j] where prior[j] <= 0 (-inf included); every other value - NaN, a positive value, +inf - counts as 0; if after that
 *     every p_j is -inf, all p_j are 0 (a reset).  u_0[j] = p_j + e_0[j], one rounded fp32 add; everything else of the definition is unchanged.
 *     prior == NULL is u_0 = e_0, the call as it was; a prior of zeros gives the same classes, back-pointers and f0, and scores equal by value.
 *   - carry: carry_out[j] = best_h[j], the best-predecessor value of frame h before e_h[j] is added.  It is computed from s_{h-1}, so its
 *     maximum is exactly 0.0; it is never NaN or positive, and -inf only under infinite costs.  Every non-empty row must have more than h
 *     frames (TVC_ERR_ARG with the reason otherwise).  prior and carry_out may be the same array: thread j reads its element at frame 0 and
 *     writes it at frame h.
 *   - in a stream whose window advances by h = block_size / 480 frames, each window's best_h is the next window's prior at its frame 0, the
 *     same instant: the exact forward recursion of an online Viterbi.  Decoded window by window over slices of ONE logits tensor, scores,
 *     back-pointers and path equal the decode of the whole prefix (tests/helpers_pitch_carry.py).  In a stream every window has logits of its
 *     own, so the chain accumulates the emissions of each window's oldest h frames; the state is a prior, not the decode of any one tensor.
 *   - MEMORY SAFETY, the one rule: no state, whatever a caller wrote into it, may leave a frame of the kernel without a class whose s == 0.
 *     The sanitised prior holds a finite value <= 0 and the emissions are finite, so m_0 is finite and the rule holds from frame 0 on as it
 *     does without a prior; no score is NaN, and every back-pointer is a class.  Independently of it the walk back never starts from the
 *     "none" value 512: it falls back to class 0.
 * tvc_pitch_path_carry_f32: tvc_pitch_path_f32's arguments with carry_frame, prior, carry_out behind path; the arrays are [rows][512], either
 * may be NULL, carry_frame is ignored when carry_out is NULL, and carry_out counts as an output.  Both NULL is tvc_pitch_path_f32.
 * tvc_convert_carry_f32: tvc_convert_path_f32's arguments with carry_frame, carry behind path; carry is [B][512] on the device, read and written
 * in place (needs path; L / 480 must be more than carry_frame).  carry == NULL is the path call, launch for launch and bit for bit.  There is
 * no ragged form: streams advance in lock step.  Both workspace queries are the path's.  The carried calls launch a variant of the kernel
 * that adds one barrier at frame 0 and one 4-byte store per thread at frame h; no new workspace, no atomics, capturable. */
typedef struct tvc_pitch_path {
    float step;
    int32_t band;
    float jump;
    float voicing;
    int32_t refine;
} tvc_pitch_path;
#define TVC_PITCH_PATH_DEFAULT {0.5f, 12, 12.0f, 3.0f, 2}
#define TVC_PITCH_PATH_MAX_BAND 32
#define TVC_PITCH_PATH_MAX_REFINE 4
int tvc_workspace_bytes_pitch_path(tvc_ctx* ctx, const int64_t* row_start, const int64_t* row_count, int rows, size_t* out_bytes);
int tvc_pitch_path_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows,
                       int64_t class_stride, const tvc_pitch_path* path, float pitch_shift, const float* pitch_shifts, float* f0,
                       float* f0_shifted, int32_t* path_out, float* score_out, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_path(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_path_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                         const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path, const float* target_f0,
                         int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift,
                         float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                         float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_pitch_path_carry_f32(tvc_ctx* ctx, void* stream, const float* logits, const int64_t* row_start, const int64_t* row_count, int rows,
                             int64_t class_stride, const tvc_pitch_path* path, int carry_frame, const float* prior, float* carry_out,
                             float pitch_shift, const float* pitch_shifts, float* f0, float* f0_shifted, int32_t* path_out, float* score_out,
                             void* ws, size_t ws_bytes);
int tvc_convert_carry_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                          const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path, int carry_frame,
                          float* carry, const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring,
                          int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                          const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_workspace_bytes_ragged_path(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_convert_ragged_path_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                const float* protect, const tvc_pitch_path* path, const float* target_f0, float pitch_shift,
                                const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B,
                                void* ws, size_t ws_bytes);

/* pitch correction: snap f0 to a table of allowed notes ------------------------------------------------------------------------ */
/* The f0 the decoder's oscillator reads exists only inside the fused call, so this is where it can be put in tune.  A note is chosen with
 * hysteresis (a pitch hovering between two notes does not flutter), the correction is smoothed by a retune coefficient (vibrato passes
 * while the note's centre moves), and a strength says how much of it is applied.  Off unless a call asks for it.
 * Everything is fp32 and every operation is rounded on its own: mul, add, sub and div below are single correctly rounded operations, sqrt
 * is correctly rounded, compares, min and max are exact.  No transcendentals: tests/helpers_pitch_snap.py holds the definition bit for bit.
 * It runs over ONE row of T frames (an utterance; an utterance's own frames in a ragged batch; a stream's window) and never crosses rows.
 * Its input x[t] is the f0 the decoder would have read - behind the path, the register, the tracker and every shift; protect's voicing
 * weight and the tracker keep reading the unshifted f0.
 * Inputs:
 *   notes     fp32 [TVC_PITCH_SNAP_NOTES = 128] on the device, read when the kernel runs: the allowed frequencies in Hz, ascending, padded
 *             with +inf
 *   strength  fp32 on the device, one per row, or NULL = 1; the kernel clamps it to [0, 1], NaN counts as 0; read when the kernel runs
 *   tvc_pitch_snap, a HOST struct: hysteresis = h, a frequency ratio in [1, 2^(1/12)]; retune = g in (0, 1], the per-frame coefficient of
 *             a one-pole smoother; 32 <= f_min <= f_max, both finite.  Anything else: TVC_ERR_ARG with the reason.
 *   state (streams; optional): note int32 and ratio fp32, one per row, and a host integer carry_frame = hop >= 1
 * Table: K is the largest k <= 128 such that notes[0 .. k-1] are finite, notes[0] > 0 and the entries are strictly ascending.  The kernel
 *   finds K itself: a table a caller scribbled into can give wrong pitches, never an index outside 0 .. K-1.  K = 0 makes every frame "out".
 *   b[i] = sqrt(mul(notes[i], notes[i+1])) for i < K-1;  near(x) = the number of i with b[i] <= x;
 *   lo[0] = 0, lo[i] = div(b[i-1], h);  hi[i] = mul(b[i], h), hi[K-1] = +inf.
 * State (q, c): (-1, anything) without a prior.  A prior (note, ratio) counts only if 0 <= note < K and 2/3f <= ratio <= 1.5f (2/3f is fp32
 *   0x3F2AAAAB; a NaN fails the compare); otherwise q = -1.
 * Frame t, x = x[t]:
 *   out:      if f_min <= x && x <= f_max is false - 0 = unvoiced, negatives, NaN, values out of range - out[t] = x with the same bits,
 *             q = -1, note_out[t] = -1.
 *   in range: n = q if q >= 0 && lo[q] < x && x < hi[q], else n = near(x);  r = div(notes[n], x);
 *             c = r if q < 0 (a note starts in tune), otherwise c = add(c, mul(g, sub(r, c)));  then c = min(max(c, 2/3f), 1.5f);  q = n;
 *             out[t] = mul(x, add(1, mul(s, sub(c, 1))));  note_out[t] = n.
 *   safety:   with f_min >= 32 and the clamp, out >= 32 * 2/3 > 20: correction never pushes a voiced frame under the decoder's 20 Hz
 *             voicing gate, whatever the table holds.
 * Carry: behind frame carry_frame - 1 the row's (q, c) is stored to the state, c as 1.0 where q = -1; every non-empty row needs at least
 *   carry_frame frames; prior and carry may be (and in these entries are) the same arrays.  Windows advanced by hop frames over slices of
 *   ONE f0 tensor equal the run over the whole prefix, by construction.  In a real stream every window decodes an f0 of its own, so the
 *   state is a prior, as with the pitch carry.
 * Identities: s = 0 returns the input bits; a table of one note maps every in-range frame toward it; g = 1, h = 1 is the memoryless
 *   nearest-note snap.
 * Kernel: one wavefront per row, four rows per workgroup, the table in LDS; no workspace, no atomics, no host synchronisation; capturable;
 *   out may be f0.  Equal rows back to back take one launch, any other row table one per 256 rows.
 * tvc_pitch_snap_f32, the stage call: rows as tvc_pitch_path_f32's (HOST arrays, ascending and apart, ends below 2^31; an empty row writes
 *   nothing; columns outside every row are not written).  note and ratio are both NULL or both given (carry_frame is ignored when NULL);
 *   note_out (int32 per column) may be NULL.
 * tvc_tuned_convert_f32: tvc_convert_carry_f32's arguments plus snap, notes, strength [B], snap_carry_frame, snap_note [B], snap_ratio [B]
 *   behind carry.  tvc_tuned_convert_ragged_f32: tvc_convert_ragged_path_f32's plus snap, notes, strength behind path (no state: streams
 *   advance in lock step).  snap == NULL is the carry call / the ragged path call, launch for launch and bit for bit; path, alpha, protect
 *   and the registers all stay optional.  The one new launch sits directly in front of the decoder, in place on the shifted f0.
 *   Workspace: tvc_workspace_bytes_path / _ragged_path (the stage needs none).
 * The Python defaults built on this (feature_retrieval.PitchSnap) are guesses: nobody has listened. */
typedef struct tvc_pitch_snap {
    float hysteresis;
    float retune;
    float f_min;
    float f_max;
} tvc_pitch_snap;
#define TVC_PITCH_SNAP_NOTES 128
int tvc_pitch_snap_f32(tvc_ctx* ctx, void* stream, const float* f0, const int64_t* row_start, const int64_t* row_count, int rows,
                       const tvc_pitch_snap* snap, const float* notes, const float* strength, int carry_frame, int32_t* note, float* ratio,
                       float* out, int32_t* note_out);
int tvc_tuned_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                          const float* weights, const float* alpha, const float* protect, const tvc_pitch_path* path, int carry_frame,
                          float* carry, const tvc_pitch_snap* snap, const float* notes, const float* strength, int snap_carry_frame,
                          int32_t* snap_note, float* snap_ratio, const float* target_f0, int start, int n, int W, int min_voiced, float slew,
                          float* ring, int64_t* count, float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out,
                          const float* noise_angle, uint64_t seed, float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_tuned_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                 const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                 const float* protect, const tvc_pitch_path* path, const tvc_pitch_snap* snap, const float* notes,
                                 const float* strength, const float* target_f0, float pitch_shift, const float* pitch_shifts,
                                 float* shift_out, const float* noise_angle, uint64_t seed, float* wave, int B, void* ws, size_t ws_bytes);

/* ---- weighted neighbours: a k of 1 .. 4 and a similarity width per row (the reference's match_features(..., k), and a weight it lacks) ----
 * Every other conversion entry averages the four nearest index rows with equal weight.  These entries average the k nearest, each weighted by
 * how close its similarity lies to the nearest row's.  Per query column of caller's row r:
 *   s_0 >= s_1 >= s_2 >= s_3 and i_0 .. i_3: the column's merged top-4, exactly what every entry selects (NaN counted as +inf, a sentinel
 *     mapped to row 0) - the indices depend on neither array: the top-k under the lists' strict order is a prefix of the top-4;
 *   k = min(max(neighbours[r], 1), 4), neighbours a DEVICE array of one int32 per caller's row; width[r] a DEVICE array of one fp32 per
 *     caller's row, in cosine units.  Both are read when the kernel runs: a captured graph replays with whatever they hold then.
 * Weights: w_0 = 1;  for 1 <= e < k:  g = s_0 - s_e (one fp32 subtraction), t = g / width (__fdiv_rn), w_e = (t > 0) ? fmaxf(0, 1 - t) : 1;
 *   for e >= k: w_e = 0.  The rule is total: NaN or inf similarities, inf / inf, 0 / 0 (a tie under width 0), a NaN or negative width all give
 *   w_e = 1; width = +inf gives 1 for every e < k; width = 0 keeps the nearest row and its exact ties.  Every w_e lies in [0, 1] and W >= 1:
 *   whatever a caller writes into the two arrays gives features, never a fault and never a division by zero.
 * Matched value of every element of the column, r_e the element of row i_e:  acc = r_0;  for e = 1 .. k - 1 in order, where w_e != 0:
 *   acc = acc + w_e * r_e (product and sum rounded separately, no FMA; a neighbour of weight 0 takes no part);  W = ((w_0 + w_1) + w_2) + w_3;
 *   mu = acc / W (__fdiv_rn).  tests/helpers_match_weight.py restates it in numpy, operation by operation.
 * Consequences: k = 4 with width = +inf is every other entry's mean bit for bit (x / 4 == x * 0.25f); k = 1, and width = 0 without ties,
 *   store the nearest row's own bits; k = 2 with width = +inf is (r_0 + r_1) * 0.5f.
 * neighbours == NULL means 4, width == NULL means +inf; both NULL is the call as it was, launch for launch.
 * alpha / protect: mu above is the mu of their definitions.  A blend: every term's mu_m is formed this way, with the row's k and width and
 *   the term's own similarities, before w_m * mu_m is accumulated.  A ragged batch finds the row as alpha does.  An index still needs N >= 4:
 *   the search keeps four.
 * Range guard: mu is a convex combination of index rows, so the decoder's content bound (the blob's |max|, the blend's sum, alpha's and
 *   protect's formulas) stays as it is; the guard scales by powers of two with three orders of magnitude of headroom, so the few ulps of
 *   rounding in acc / W do not matter.
 * tvc_knn_match_weighted_f32, the stage call: tvc_knn_match_protect_f32's arguments plus neighbours and width behind protect, and sims_out
 *   (nullable, [M][B][T][4] fp32, beside idx_out): the similarities exactly as the lists held them when the weights were formed - cosines of
 *   the query and the selected rows, accurate to the fp32 accumulation of a 768-term product of unit vectors (770 * 2^-24), and the one
 *   measure of how well an index covers a speaker that the library can give.  With neighbours, width and sims_out all NULL it is the protect call.
 * tvc_weighted_convert_f32 / tvc_weighted_convert_ragged_f32: the tuned entries' arguments plus neighbours and width behind protect.  No
 *   workspace of their own: tvc_workspace_bytes_path / _ragged_path.  Capturable under the siblings' rules; every host check runs before
 *   any device work; the one kernel that changes is the merge + gather, in its weighted instantiation - no new pass, no host synchronisation.
 * Per row: row b equals its own B = 1 call bit for bit whenever its segment of the search takes the path its own call takes.  A (query, row)
 *   similarity's bits do not depend on splits, tiles or the segments' order - the rescore is one fixed-order fp32 chain per pair, the exact
 *   kernel one fixed-order accumulator per pair - but the two kernels round differently, and rows that share ONE blob in adjacent columns
 *   are one segment with one overflow flag: a dense neighbourhood in one row (more than the candidate cap) then sends its neighbours' rows
 *   to the exact kernel too.  The indices are the same either way; the similarities, and so the weights, then agree to 770 * 2^-24 only.
 *   Rows with blobs of their own are segments of their own and keep the bit-for-bit contract.
 * No default width is suggested: nobody has listened. */
int tvc_knn_match_weighted_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared,
                               const int64_t* N, int M, const float* weights, const float* alpha, const float* protect,
                               const int32_t* neighbours, const float* width, float* out, int64_t* idx_out, float* sims_out, int B, int T,
                               void* ws, size_t ws_bytes);
int tvc_weighted_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                             const float* weights, const float* alpha, const float* protect, const int32_t* neighbours, const float* width,
                             const tvc_pitch_path* path, int carry_frame, float* carry, const tvc_pitch_snap* snap, const float* notes,
                             const float* strength, int snap_carry_frame, int32_t* snap_note, float* snap_ratio, const float* target_f0,
                             int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count, float* auto_shift,
                             float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                             float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_weighted_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                    const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                    const float* protect, const int32_t* neighbours, const float* width, const tvc_pitch_path* path,
                                    const tvc_pitch_snap* snap, const float* notes, const float* strength, const float* target_f0,
                                    float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle, uint64_t seed,
                                    float* wave, int B, void* ws, size_t ws_bytes);

/* ---- match along a path: a continuity weight between neighbouring frames (unit selection's join cost; no reference counterpart) ----
 * The weighted entries choose per frame: the weights form around neighbour 0, whatever the frame before chose.  Where two index rows are
 * almost equally near a stretch of frames, the anchor of a sharp match (k = 1, a small width) alternates between them every 20 ms.  These
 * entries choose the anchor as a SEQUENCE: a neighbour gains by its similarity to the query (s, which the search holds) and by its
 * similarity to the neighbour chosen for the frame before (the affinity a).  Per utterance - a row's T frames, or in a ragged batch the
 * frames [pre[u], pre[u] + tb[u]) of utterance u - and, in a blend, per term: a path never leaves its utterance, its row, its term or its
 * stream.  Frames t = 0 .. len - 1; k = the row's clamped neighbours (NULL: 4); s_t[e], i_t[e] the column's merged top-4, exactly what every
 * entry selects; c = join[r], a DEVICE fp32 per caller's row, read when the kernels run.  Every step below is one fp32 rounding, no FMA.
 * THE TOTAL RULE (the kernels' memory safety rests on it): a similarity or an affinity that is not finite counts as 0; a c that is NaN or
 *   negative counts as 0, a c of +inf as the largest finite float (FLT_MAX); and sat(x) = fminf(fmaxf(x, -FLT_MAX), FLT_MAX) - NaN gives
 *   -FLT_MAX - is applied where the rules below say so (it changes nothing while |values| stay below FLT_MAX).  Then every state of every
 *   frame has a finite score <= 0 with a maximum of exactly 0, and - independently of that - a back-pointer is the d < k of a comparison
 *   chain that starts at d = 0 and the last anchor the e < k of one that starts at e = 0: whatever the arrays hold, every anchor lies in
 *   0 .. k - 1.
 * Affinity, t >= 1 and d, e < 4:  a_t[d][e] = (dot(row i_{t-1}[d], row i_t[e]) * inv[i_{t-1}[d]]) * inv[i_t[e]] over the segment's own blob,
 *   inv = 1 / (|v| + 1e-6) as every prepared blob holds it.  The dot in ONE order: with p_k the rounded product of channel k, partial sum
 *   P_l = ((p_l + p_{l+64}) + ..) + p_{l+704} for l = 0 .. 63 (ascending), then six rounds Q_l <- Q_l + Q_{l xor m} for m = 32, 16, 8, 4, 2, 1;
 *   dot = Q_0.  Its bits depend on no tile, split, batch size or k.  The dot carries 18 roundings (a product, 11 + 6 sums) where one chain of 768 carries
 *   768; with the two inv factors a is held to the 770 * 2^-24 of sims_out against dot / ((|u| + 1e-6) (|v| + 1e-6)) in fp64.  Frame 0 of an utterance has none (affinity_out: zeros).
 * Scores:  D_0[e] = s_0[e];  for t >= 1, e < k:  D_t[e] = sat(s_t[e] + max_{d<k} (D_{t-1}[d] + sat(c * a_t[d][e]))) - the max is exact, ties
 *   go to the lowest d, and the back-pointer records it.  After every frame, 0 included: D_t[e] = sat(D_t[e] - max_{e<k} D_t[e]), one
 *   subtraction - scores stay near 0 at 15 000 frames, where accumulated sums would lose the 1e-3 differences between similarities.
 * Anchor:  p(len - 1) = argmax_{e<k} D, the lowest e on ties;  p(t - 1) = the back-pointer of state p(t) of frame t.
 * Weights around the anchor p:  w_p = 1;  for e < k, e != p:  g = |s_p - s_e|, t = g / width (__fdiv_rn), w_e = (t > 0) ? fmaxf(0, 1 - t) : 1
 *   (the RAW similarities, as the weighted entries');  w_e = 0 from k on.
 * Mean:  the terms w_e * r_e with w_e != 0 are added in ascending e, the first of them starting the sum (product and sum rounded on their
 *   own; a weight of exactly 1 contributes r_e's own bits);  W = ((w_0 + w_1) + w_2) + w_3 >= 1;  mu = acc / W (__fdiv_rn).
 *   tests/helpers_match_join.py restates all of it in numpy fp32, operation by operation.
 * Consequences: c = 0 on finite similarities gives anchor 0 on every frame and the weighted call bit for bit; width = +inf makes the path
 *   irrelevant (the same bits for any c); width = 0 without ties stores the path's row's own bits - unit selection; k = 1 has no choice to
 *   make; mu stays a convex combination of index rows, so the decoder's range guard and every content bound stay as they are;
 *   join == NULL is the weighted call, launch for launch.
 * Kernels: no search kernel changes and the indices depend on nothing new.  Three launches take the weighted gather's place: merge +
 *   affinity (the merged lists, idx_out and sims_out; the 16 affinities per column), the path (one wavefront per (term, utterance), the walk
 *   back in the same launch) and the joined form of the merge + gather, which reads the anchor where it forms the weights.  No host
 *   synchronisation: capturable.  Workspace of their own (101 bytes per query column and term), from the call's one walk.
 * tvc_knn_match_joined_f32: tvc_knn_match_weighted_f32's arguments plus join behind width and, behind sims_out, anchor_out (nullable, int32
 *   [M][B][T]) and affinity_out (nullable, fp32 [M][B][T][4][4], [d][e]; frame 0's sixteen are zeros).  anchor_out / affinity_out without
 *   join are refused.  Workspace: tvc_workspace_bytes_match_joined (B rows of L = 480 T samples).
 * tvc_joined_convert_f32 / tvc_joined_convert_ragged_f32: the weighted entries' arguments plus join behind width.  Workspace:
 *   tvc_workspace_bytes_joined / _ragged_joined.  Every host check runs before any device work.
 * A stream decodes a path per window; carrying the scores from window to window is out of scope, as are the sharded route and a default:
 *   nobody has listened. */
int tvc_workspace_bytes_joined(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_workspace_bytes_ragged_joined(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, const int64_t* N, int M, size_t* out_bytes);
int tvc_workspace_bytes_match_joined(tvc_ctx* ctx, int B, int64_t L, const int64_t* N, int M, size_t* out_bytes);
int tvc_knn_match_joined_f32(tvc_ctx* ctx, void* stream, const float* src, const float* f0, const float* const* prepared, const int64_t* N,
                             int M, const float* weights, const float* alpha, const float* protect, const int32_t* neighbours,
                             const float* width, const float* join, float* out, int64_t* idx_out, float* sims_out, int32_t* anchor_out,
                             float* affinity_out, int B, int T, void* ws, size_t ws_bytes);
int tvc_joined_convert_f32(tvc_ctx* ctx, void* stream, const float* wav, const float* const* prepared, const int64_t* N, int M,
                           const float* weights, const float* alpha, const float* protect, const int32_t* neighbours, const float* width,
                           const float* join, const tvc_pitch_path* path, int carry_frame, float* carry, const tvc_pitch_snap* snap,
                           const float* notes, const float* strength, int snap_carry_frame, int32_t* snap_note, float* snap_ratio,
                           const float* target_f0, int start, int n, int W, int min_voiced, float slew, float* ring, int64_t* count,
                           float* auto_shift, float pitch_shift, const float* pitch_shifts, float* shift_out, const float* noise_angle,
                           uint64_t seed, float* wave, int B, int64_t L, void* ws, size_t ws_bytes);
int tvc_joined_convert_ragged_f32(tvc_ctx* ctx, void* stream, const float* wav, int64_t Lmax, const int64_t* lens,
                                  const float* const* prepared, const int64_t* N, int M, const float* weights, const float* alpha,
                                  const float* protect, const int32_t* neighbours, const float* width, const float* join,
                                  const tvc_pitch_path* path, const tvc_pitch_snap* snap, const float* notes, const float* strength,
                                  const float* target_f0, float pitch_shift, const float* pitch_shifts, float* shift_out,
                                  const float* noise_angle, uint64_t seed, float* wave, int B, void* ws, size_t ws_bytes);

/* streaming tail-------------------------------------------------------------------------- */
/* StreamInfer.audio_callback after convert (reference module/infer/stream.py:74-95), batched over
 * S streams: y [S, Ly] converted buffers; sola_buf [S,1920] in/out; fade_in [1920] = the sin^2
 * window init_buffer builds (stream.py:61; fade_out = 1 - fade_in); out [S, block];
 * shift_out [S] int32 (nullable) = chosen SOLA lag.  block = 1920 in the reference;
 * crossfade = search = 1920, delay = 3840 (stream.py:48-50).  use_phase_vocoder selects
 * phase_vocoder() (stream.py:9-26) instead of the sin^2 cross-fade. */
int tvc_sola_f32(tvc_ctx* ctx, void* stream, const float* y, float* sola_buf, const float* fade_in,
                 float* out, int32_t* shift_out, int S, int64_t Ly, int block,
                 int use_phase_vocoder);

/* The same tail with the geometry chosen by the caller: sola_buf [S][cross], fade_in [cross], temp = y[Ly - (block + cross + search + delay) :
 * Ly - delay], the lag is searched over 0 .. search.  tvc_sola_f32 is the (1920, 1920, 3840) call of it.  The first sample of the block a
 * stream emits lags the first sample of its newest input block by cross + search + delay - shift samples, shift in [0, search].
 *
 * tvc_sola_geometry (host only: no context, no device) holds the limits: 4 <= cross <= 1920 and cross % 4 == 0; 0 <= search <= 1920
 * (0 = one lag: a plain cross-fade); delay >= 0; 1 <= block <= 2^30.  Anything else returns TVC_ERR_ARG; otherwise min_ly = block + cross +
 * search + delay (the shortest y), latency_min = cross + delay and latency_max = cross + search + delay, in samples (out pointers are
 * nullable).  tvc_sola_geometry_message gives the reason of a refusal ("" for a legal geometry), valid until the thread's next call.
 * tvc_sola_geom_f32 refuses the same geometries and Ly < min_ly with that reason in tvc_last_error (a short Ly names the minimum).
 * Capturable like tvc_sola_f32: the geometry is baked into a capture, the samples and the buffer are read when the kernel runs. */
int tvc_sola_geometry(int block, int cross, int search, int delay, int64_t* min_ly, int* latency_min, int* latency_max);
const char* tvc_sola_geometry_message(int block, int cross, int search, int delay);
int tvc_sola_geom_f32(tvc_ctx* ctx, void* stream, const float* y, float* sola_buf, const float* fade_in, float* out, int32_t* shift_out, int S,
                      int64_t Ly, int block, int cross, int search, int delay, int use_phase_vocoder);

/* StreamInfer.audio_callback before convert (reference module/infer/stream.py:69-70: `input_wav = torch.roll(input_wav, -block)`,
 * `input_wav[-block:] = block`), batched over S streams, in place and in one launch: buf [S, n] rolling input buffers,
 * blocks [S, block] the new blocks; afterwards buf[s] = (old buf[s][block:], blocks[s]).  Any block <= n < 2^31 - 32 768; a row longer
 * than 32 768 samples is shifted in 32 768-sample tiles inside the same launch (capturable like every other call). */
int tvc_stream_push_f32(tvc_ctx* ctx, void* stream, float* buf, const float* blocks, int S, int64_t n, int block);

/* The streaming door (extension): tvc_resample_f32 block by block, for S streams whose clients run at another rate than the model's
 * 24 kHz, fused with the int16 conversions and gain above.  Each stream carries `hist` fp32 input samples of filter history on the
 * device (state [S][hist], zeros at the start of a stream; zero a row to restart that stream).
 *
 * Definition: for every prefix of a stream, the blocks emitted so far are the first samples of tvc_resample_f32 applied to
 * (G * orig zeros ++ the prefix), bit for bit - the same filter table, the same ascending fmaf chain per output.
 *
 * Geometry (host only: no context, no device; g = gcd(in_freq, out_freq), orig = in_freq / g, new = out_freq / g, width and
 * taps = 2 * width + orig as tvc_resample_f32's table has them):
 *   a block is n_in input samples with n_in % orig == 0 and gives exactly n_out = n_in / orig * new outputs;
 *   G = ceil(width / orig) whole output groups of look-ahead;  hist = G * orig + width;  delay = G * new output samples of latency,
 *   the least for which every emitted output has all its `taps` inputs (48000 -> 24000: hist 27, delay 7; 44100 -> 24000: orig 147,
 *   new 80, G 1, hist 159, delay 80 = 3.3 ms - one whole 147:80 group, and the same again on the way back out).
 * tvc_stream_resample_geometry returns TVC_ERR_ARG for a non-positive rate or n_in, for n_in % orig != 0, and for a block whose
 * hist + n_in floats exceed TVC_STREAM_RESAMPLE_LDS_FLOATS: the kernel stages a stream's history and block in LDS, one workgroup per
 * stream, and 64 KiB is what a workgroup gets.  Equal rates are legal: hist = delay = 0, n_out = n_in.
 *
 * tvc_stream_resample: in [S][n_in] (int16 when in_is_pcm16, else fp32) -> out [S][n_out] (int16 when out_is_pcm16, else fp32); state is
 * read and advanced in place (NULL allowed at equal rates).  One side at most is int16; gain_db is that side's gain (tvc_pcm16_to_f32's
 * arithmetic before the filter, tvc_f32_to_pcm16's after it - wrap-around included) and must be 0 between fp32 and fp32.  Equal rates
 * run the plain conversions (a device copy for fp32 to fp32).  The rates, n_in and the gain are kernel arguments, baked into a stream
 * capture; the samples and the state are read when the kernel runs, so a captured block replays as the streams advance or restart.
 * No workspace.  The first use of a rate pair by a context builds its filter table synchronously: tvc_stream_resample_prepare does that
 * ahead of time, and tvc_stream_resample refuses with TVC_ERR_STATE inside a capture when it has not been done. */
#define TVC_STREAM_RESAMPLE_LDS_FLOATS 16384
int tvc_stream_resample_geometry(int in_freq, int out_freq, int64_t n_in, int64_t* n_out, int* hist, int* delay);
int tvc_stream_resample_prepare(tvc_ctx* ctx, int in_freq, int out_freq);
int tvc_stream_resample(tvc_ctx* ctx, void* stream, const void* in, int in_is_pcm16, void* out, int out_is_pcm16, float* state, int S,
                        int64_t n_in, int in_freq, int out_freq, float gain_db);

/* The streams' noise gate (extension): one launch behind the tail, one workgroup per stream.  For stream s: x = its input window
 * [n] (x [S][n]), y = the block the tail emitted ([S][block]), a = base + shift[s] (shift: the tail's shift_out, NULL = 0), so that
 * x[a + j] is the input sample y[j] was converted from (for a stream: base = Ly - block - cross - search - delay); an index outside
 * [0, n) reads as 0.  With nsub = block / sub sub-frames and `look` sub-frames of look-ahead:
 *   p[i] = mean(x[a + i*sub .. a + (i+1)*sub)^2), i < nsub + look (fp32);  T_open = 10^(threshold_db[s] / 10), T_close = T_open *
 *   10^(-hysteresis_db / 10) (-inf dB -> 0: always open);  for i = 0 .. nsub - 1 in order, carrying (open, hold, g) from block to block:
 *     d = max(p[i] .. p[i + look])                       (a NaN d is below both thresholds)
 *     d >= T_open: open = 1, hold = H;  else open and d >= T_close: hold = H;  else open: hold > 0 ? hold -= 1 : open = 0
 *     tgt = open ? 1 : floor (= 10^(range_db / 20), -inf -> 0);  g_prev = g;
 *     g = tgt > g ? min(tgt, g + 1.0f / attack) : max(tgt, g - 1.0f / release)      (fp32: one add, one clamp)
 *     out[i*sub + j] = y[i*sub + j] * (g_prev + (g - g_prev) * ((j + 1) / (float)sub)),  j < sub
 *   level_db[s] = 10 log10(max(mean(p[0 .. nsub)), 1e-20))      (nullable)
 * Where g_prev == g the multiplier is exactly g: an open gate changes no bit, a closed one at range_db = -inf emits zeros.  H (`hold`),
 * attack and release count sub-frames.  threshold_db [S] and the state - open [S] int32, hold_state [S] int32, gain [S] fp32; a stream
 * starts at (1, 0, 1.0) - live on the device and are read when the kernel runs (the state is advanced in place), so a captured launch
 * replays as they move; everything else is baked in.  out may be y.  No workspace.
 *
 * tvc_stream_gate_geometry (host only: no context, no device) holds the limits: 4 <= sub <= 65536, sub % 4 == 0, block >= 1 a multiple
 * of sub; look >= 0 and block / sub + look <= 4096 (the powers sit in LDS); 0 <= hold <= 2^20; 1 <= attack, release <= 2^20.  Anything
 * else returns TVC_ERR_ARG; otherwise nsub = block / sub and look_samples = look * sub (out pointers are nullable).
 * tvc_stream_gate_geometry_message gives the reason of a refusal ("" for a legal geometry), valid until the thread's next call.
 * tvc_stream_gate_f32 refuses the same geometries with that reason in tvc_last_error, and: a NULL x, y, out, threshold_db or state
 * pointer, S <= 0, n outside 1 .. 2^40, |base| > 2^40, a hysteresis_db that is negative or not finite, a range_db that is positive or
 * NaN - all with TVC_ERR_ARG before anything is launched. */
int tvc_stream_gate_geometry(int block, int sub, int look, int hold, int attack, int release, int* nsub, int* look_samples);
const char* tvc_stream_gate_geometry_message(int block, int sub, int look, int hold, int attack, int release);
int tvc_stream_gate_f32(tvc_ctx* ctx, void* stream, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                        int block, int sub, int look, int hold, int attack, int release, float hysteresis_db, float range_db,
                        const float* threshold_db, int32_t* open, int32_t* hold_state, float* gain, float* level_db);

/* The streams' spectral suppressor (extension): one launch in front of tvc_stream_push_f32, one workgroup per stream, a stateful short-time
 * spectral gain on the 24 kHz block x [S][block] before it enters the rolling window.  Frames of NF = 640 samples at a hop of `hop` (160 or
 * 320), analysis and synthesis window w[n] = sqrt(0.5 - 0.5 cos(2 pi n / 640)) (tabulated in fp64, rounded once), synthesis scale
 * 2 hop / 640 (the overlap-add of w^2 is then exactly 1); block % hop == 0; the output is the processed input delayed by D = 640 - hop.
 * State per stream, on the device, advanced in place; a stream starts with all of it zero:
 *   hist [S][D] raw input tail, ola [S][D] overlap-add tail, smooth [S][321] smoothed power per bin, noise [S][321] noise power per bin,
 *   frames [S] int32 frames counted so far (saturating at 2^30).
 * reduction_db [S] fp32 on the device is read when the kernel runs: floor = 10^(-max(reduction_db, 0) / 20).  a_s, a_n, clamp, beta (fp32)
 * and warm (int) are baked in; NMIN = TVC_STREAM_DENOISE_NMIN, tiny = 1e-30f.  For frame m of the stream, in order, with
 * f = (hist ++ x)[m hop .. m hop + 640):
 *   1. all 640 samples of f are +-0: the frame adds nothing to the overlap-add and leaves smooth, noise and frames as they are (a muted
 *      microphone neither counts as warm-up nor drags the estimate to zero);
 *   2. otherwise X = rfft(w f) (321 bins), P = re^2 + im^2, and per bin
 *        smooth = a_s smooth + (1 - a_s) P
 *        frames < warm:  noise = noise + (P - noise) / (frames + 1)           (a running mean)
 *        otherwise:      noise = a_n noise + (1 - a_n) min(P, max(clamp noise, NMIN))
 *        G = max(floor, 1 - beta noise / max(smooth, tiny));  Y = G X;   then frames += 1;
 *   3. irfft(Y) w (2 hop / 640) is added into the overlap-add accumulator in ascending frame order: an output sample is the carried ola
 *      plus at most 640 / hop contributions, added in that order;
 *   4. hop finished samples leave.
 * noise_db [S] (nullable) = 10 log10(max(sum_k m_k noise[k] / (640 * 320), 1e-20)) after the block, m_k = 1 for k = 0 and 320, else 2: the
 * estimate in dB re full scale per sample.  Every rule is continuous in the data (the branches are min / max and two integer tests).
 * Output and state do not depend, bit for bit, on how a stream is cut into blocks, on S or on the other streams; reduction_db == 0 gives
 * G == 1 (the delayed input within the transforms' rounding; the state still advances); a stream of zeros emits zeros and keeps its state.
 * out may be x.  No workspace.
 *
 * tvc_stream_denoise_geometry (host only: no context, no device) holds the limits: hop is 160 or 320, block >= hop a multiple of hop,
 * block / hop <= 4096.  Anything else returns TVC_ERR_ARG; otherwise frames = block / hop and delay = 640 - hop (out pointers are nullable).
 * tvc_stream_denoise_geometry_message gives the reason of a refusal ("" for a legal geometry), valid until the thread's next call.
 * tvc_stream_denoise_f32 refuses the same geometries with that reason in tvc_last_error, and: a NULL pointer (noise_db is exempt), S <= 0,
 * a_s or a_n outside [0, 1), clamp < 1, beta < 0, warm < 0, any scalar that is not finite - all with TVC_ERR_ARG before anything is launched. */
#define TVC_STREAM_DENOISE_NMIN 1e-12f
int tvc_stream_denoise_geometry(int block, int hop, int* frames, int* delay);
const char* tvc_stream_denoise_geometry_message(int block, int hop);
int tvc_stream_denoise_f32(tvc_ctx* ctx, void* stream, const float* x, float* out, int S, int block, int hop, float a_s, float a_n, float clamp,
                           float beta, int warm, const float* reduction_db, float* hist, float* ola, float* smooth, float* noise, int32_t* frames,
                           float* noise_db);

/* The loudness envelope match (extension; RVC's rms_mix_rate, as 1 - its value): the converted signal follows the loudness envelope of
 * the signal it was converted from, by a share e in [0, 1].  x is the input at the model's rate on the output's time axis, y the converted
 * output; both are cut into sub-frames of `sub` samples (a multiple of 4; 240 = 10 ms).
 *   Powers     Ps[i], Po[i] = the mean power of sub-frame i of x and of y, accumulated in fp64 (an fp32 square is exact in fp64, so the
 *              order of the reduction does not matter at fp32 precision).
 *   Envelope   Es[i] = the mean of Ps over a window of sub-frames, summed in ascending index order in fp64 and divided by the number of
 *              sub-frames actually present; Eo[i] likewise from Po.
 *   Gain       q = max(Es, floor) / max(Eo, floor), floor = 10^(floor_db / 10);  r = exp2(0.5 * e * log2(q)), all in fp64;  r is clamped
 *              to [10^(-cut_db / 20), 10^(boost_db / 20)] and rounded to fp32 once: the gain g[i] of sub-frame i.
 *   Special    a window that holds a NaN or infinite power gives g[i] = 1 exactly.  e is read from device memory when the kernel runs:
 *              values outside [0, 1] are clamped, NaN is 0, and e == 0 gives g[i] = 1.0f exactly - the samples keep their bits.
 *   Ramp       the gate's: with g0 the gain at the previous sub-frame edge and g1 = g[i], sample j of sub-frame i is multiplied by
 *              g0 + (g1 - g0) * ((j + 1) / (float)sub), every operation rounded on its own in fp32.  The very first sub-frame of an
 *              utterance or a stream is flat at its own gain (g0 = g1).
 * Defaults (guesses: nobody has listened): floor_db = -60, boost_db = 12, cut_db = 40, smooth = 2 sub-frames each side.
 *
 * tvc_loudness_match_f32 (offline): x, y, out [B][L], share [B] fp32 on the device.  The window is centred - sub-frames i - smooth ..
 * i + smooth, truncated to the row's own sub-frames.  lengths (nullable): int64 [B] on the HOST, as in the ragged conversions; they travel
 * as kernel arguments (no copy, no workspace: asynchronous, and baked into a capture) - row b owns its first lengths[b] samples (clamped
 * to 0 .. L, whole sub-frames of them); the window never crosses that length and the samples behind it are copied unchanged.  gains (nullable): [B][L / sub + 1] fp32, the gain at every sub-frame edge - edge 0 and edge 1 hold g[0], edge
 * i + 1 holds g[i], edges behind a row's length hold 1.  One launch (one per 384 rows of a larger batch), no workspace, 64-bit indices: the grid is rows x tiles of `tile`
 * sub-frames (tvc_loudness_geometry reports the constant), and each workgroup recomputes the powers of its halo of 2 * smooth + 1
 * sub-frames.  out may be y: the call is then one workgroup per row, which walks the row's tiles in order (another workgroup's halo would
 * be read while this one scales it), with the same bits.  Any other overlap of out with x or y is refused; x, y and out are 16-byte aligned.
 *
 * tvc_stream_loudness_f32 (streams): one launch behind the tail, one workgroup per stream, with the gate's addressing - x [S][n] the input
 * windows, y [S][block] the emitted blocks, x[base + shift[s] + j] is the input sample y[j] was converted from (shift NULL = 0; an index
 * outside [0, n) reads 0).  The window trails: the last W = 2 * smooth + 1 sub-frames up to and including the current one, fewer at the
 * start of a stream.  State per stream, on the device, advanced in place: src_ring, out_ring [S][W] fp64 (the last powers, slot = sub-frame
 * index % W, summed oldest to newest), frames [S] int64 (sub-frames seen), gain [S] fp32 (the last edge gain); a stream starts at zeros,
 * 0 and 1.0.  A stream is therefore the offline gain sequence `smooth` sub-frames late - in the interior the two agree bit for bit - and
 * its result does not depend, bit for bit, on how it is cut into blocks, on S or on the other streams.  The state advances when e == 0
 * too.  gain_db [S] (nullable): the last edge gain in dB.  gains (nullable): [S][block / sub + 1], the block's edge gains (edge 0: the
 * carried gain).  out may be y (any other overlap of out with x or y is refused); y and out are 16-byte aligned.  No workspace.
 *
 * tvc_loudness_geometry (host only: no context, no device) holds the limits: 4 <= sub <= 65536, sub % 4 == 0, 1 <= length <= 2^40 a
 * multiple of sub, 0 <= smooth <= 32; tvc_stream_loudness_geometry the same for a stream's block, and at most 4096 sub-frames per block
 * (the gate's cap, so that both stages take the same blocks; no resource of the kernel depends on it).
 * Anything else returns TVC_ERR_ARG; otherwise nsub = length / sub, window = 2 * smooth + 1 and tile (out pointers are nullable).  The
 * _message entries give the reason of a refusal ("" for a legal geometry), valid until the thread's next call.  The two device entries
 * refuse the same geometries with that reason in tvc_last_error, and: a NULL pointer (lengths, shift, gain_db and gains are exempt), B or
 * S <= 0, a floor_db that is not finite (or whose 10^(floor_db / 10) is not a positive double), a boost_db or cut_db that is negative or
 * not finite (or whose gain is not a positive finite fp32 number), n outside 1 .. 2^40, |base| > 2^40 - all with TVC_ERR_ARG before
 * anything is launched. */
int tvc_loudness_geometry(int64_t length, int sub, int smooth, int64_t* nsub, int* window, int* tile);
const char* tvc_loudness_geometry_message(int64_t length, int sub, int smooth);
int tvc_stream_loudness_geometry(int block, int sub, int smooth, int* nsub, int* window);
const char* tvc_stream_loudness_geometry_message(int block, int sub, int smooth);
int tvc_loudness_match_f32(tvc_ctx* ctx, void* stream, const float* x, const float* y, float* out, int B, int64_t L, const int64_t* lengths,
                           const float* share, int sub, int smooth, float floor_db, float boost_db, float cut_db, float* gains);
int tvc_stream_loudness_f32(tvc_ctx* ctx, void* stream, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                            int block, int sub, int smooth, float floor_db, float boost_db, float cut_db, const float* share, double* src_ring,
                            double* out_ring, int64_t* frames, float* gain, float* gain_db, float* gains);

/* The look-ahead peak limiter (extension; the stage every real-time voice chain ends in): nothing it emits lies above a ceiling, exactly.
 * y is the signal to limit, cut into sub-frames of `sub` samples (a multiple of 4; 24 = 1 ms, which is the look-ahead and the attack).
 *   c          = ceiling[row or stream], a linear fp32 amplitude read from device memory when the kernel runs; NaN, <= 0 and +inf mean off
 *              and are treated as +inf.
 *   drive      an fp32 factor baked in: (float)10^(drive_db / 20), computed in double on the host and rounded once.
 *   R          = release, in sub-frames, 1 <= R <= 4096;  d = 1.0f / (float)R, one fp32 division.
 * Every operation below is a separate fp32 rounding (__fmul_rn, __fadd_rn, __fdiv_rn, ...), as in the loudness match's ramp.
 *   v[n]  = y[n] * drive
 *   p[k]  = max over sub-frame k of |v|        (NaN samples ignored; p[-1] = 0; p[K] = 0 behind the last sub-frame of a row)
 *   m[k]  = max(p[k-1], p[k])                  for edge k = the start of sub-frame k, k = 0 .. K
 *   r[k]  = m[k] > c ? c / m[k] : 1.0f         (m = inf -> 0)
 *   e[k]  = min(r[k], min(1.0f, e[k-1] + d))   e[-1] = 1          (instant fall, linear rise: the gate's rule)
 *   out[k*sub + j] = clampc( v[k*sub + j] * (e[k] + (e[k+1] - e[k]) * ((j + 1) / (float)sub)) )      the gate's ramp
 *   clampc(t) = t > c ? c : (t < -c ? -c : t)                      (NaN passes; with c = inf nothing happens)
 * Both edge gains of sub-frame k are at most c / p[k] and the ramp stays between them up to rounding, so |out| <= c up to a few ulp; clampc
 * makes the bound exact and only ever moves a sample by that rounding.  Wherever e[k] == e[k+1] == 1 and drive == 1 the samples keep their
 * bits.  A NaN sample comes out NaN and moves no gain; an infinite one drives its two edges to 0 and comes out NaN.
 * f(e) = min(1, e + d) is monotone and f^(R+1)(0) == 1.0f exactly for every legal R, so e[k] depends on r[k - R .. k] only: a recurrence
 * restarted from e = 1 at R + 1 edges back gives the same bits.  The offline kernel's tile grid rests on this.
 * Defaults (guesses: nobody has listened): sub = 24, release = 100 sub-frames (100 ms), ceiling -1 dBFS, drive 0 dB.
 *
 * tvc_limit_f32 (offline): y, out [B][L], ceiling [B] fp32 on the device.  lengths (nullable): int64 [B] on the HOST, travelling as kernel
 * arguments as in tvc_loudness_match_f32 - row b owns its first lengths[b] samples (clamped to 0 .. L, whole sub-frames of them), p is 0
 * behind those sub-frames and the samples behind them are copied unchanged.  gains (nullable): [B][L / sub + 1] fp32, the edge gains
 * e[0 .. K]; edges behind a row's last one hold 1.  One launch (one per 384 rows of a larger batch) on a grid of rows x tiles of `tile`
 * sub-frames, no workspace, no host synchronisation, 64-bit indices.  Per tile a workgroup takes the peaks of its sub-frames, of the R + 2
 * before them and of the one after, runs the recurrence with every thread owning a few edges behind a warm-up of R + 1, and applies the
 * ramp; only peaks and gains sit in LDS (tile + R + 3 floats).  out must not overlap y - an in-place call is refused: another tile's halo
 * would be read while it is being scaled.  y and out are 16-byte aligned.
 *
 * tvc_stream_limit_f32 (streams): y, out [S][block], one launch, one workgroup per stream, which walks the block in chunks of `chunk`
 * sub-frames, so no resource depends on the block.  Sub-frame k can only leave once p[k+1] is known: the stage delays by exactly `sub`
 * samples.  State per stream, on the device, advanced in place: tail [S][sub] fp32 (the driven samples of the sub-frame not yet emitted),
 * peak [S] (its peak), gain [S] (e at its start); a stream starts at zeros, 0 and 1.0.  A stream's blocks, concatenated, are `sub` zeros
 * followed by the offline result of the whole signal, bit for bit, however the stream is cut into blocks, whatever S is and whatever the
 * neighbours do.  reduction_db [S] (nullable): 20 log10 of the smallest edge gain of the block, the carried one included (a meter).
 * gains (nullable): [S][block / sub + 1], the block's edge gains (edge 0: the carried gain).  out must not overlap y; y, out and tail are
 * 16-byte aligned.  Everything but ceiling and the state is baked into a capture.  No workspace.
 *
 * tvc_limiter_geometry (host only: no context, no device) holds the limits: 4 <= sub <= 65536, sub % 4 == 0, 1 <= length <= 2^40 a multiple
 * of sub, 1 <= release <= 4096; tvc_stream_limiter_geometry the same for a stream's block of one sub-frame .. 2^30 samples.  Anything else
 * returns TVC_ERR_ARG; otherwise nsub = length / sub, delay = sub and tile / chunk (out pointers are nullable).  The _message entries give
 * the reason of a refusal ("" for a legal geometry), valid until the thread's next call.  The two device entries refuse the same
 * geometries with that reason in tvc_last_error, and: a NULL pointer (lengths, reduction_db and gains are exempt), B or S <= 0, a drive_db
 * that is not finite or whose factor is not a positive finite fp32 number - all with TVC_ERR_ARG before anything is launched.
 *
 * Two limits of the guarantee: the door's int16 conversion still wraps a sample above 32767 / 32768, so a ceiling above that bounds
 * nothing there; and a resampling door interpolates between samples and may overshoot the ceiling: -1 dB is margin, not proof. */
int tvc_limiter_geometry(int64_t length, int sub, int release, int64_t* nsub, int* delay, int* tile);
const char* tvc_limiter_geometry_message(int64_t length, int sub, int release);
int tvc_stream_limiter_geometry(int block, int sub, int release, int* nsub, int* delay, int* chunk);
const char* tvc_stream_limiter_geometry_message(int block, int sub, int release);
int tvc_limit_f32(tvc_ctx* ctx, void* stream, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* ceiling, int sub, int release,
                  float drive_db, float* gains);
int tvc_stream_limit_f32(tvc_ctx* ctx, void* stream, const float* y, float* out, int S, int block, int sub, int release, float drive_db, const float* ceiling,
                         float* tail, float* peak, float* gain, float* reduction_db, float* gains);

/* measurement ----------------------------------------------------------------------------- */
/* on = 1: every stage (and every FilterNet block) is bracketed by a hipEvent pair on the launch stream (19 pairs per
 * convert, ~0.1 ms of a 8.4 ms step); on = 2: only the `filter_net` region (the roofline's kernel group); on = 0: off.
 * tvc_profile_read() synchronises those events and writes "region=milliseconds;..." (summed per region name since the
 * previous read) into buf. */
int tvc_profile_enable(tvc_ctx* ctx, int on);
int tvc_profile_read(tvc_ctx* ctx, char* buf, size_t buf_bytes);

#ifdef __cplusplus
}
#endif
#endif /* TINYVC_HIP_H */
