// The pitch path (extension; tvc_pitch_path_f32 and the *_path_f32 conversions): a Viterbi decode of the pitch logits over one utterance,
// in the place of the per-frame top-4 expectation of pitch_decode_kernel.  The definition is in tinyvc_hip.h; tests/helpers_pitch_path.py
// restates it in numpy, and every score, back-pointer and class here equals that restatement bit for bit.
//
// One workgroup of 512 threads per utterance, thread j = class j.  A frame is
//   u_t[j] -> the maximum of u_t over the voiced classes (wave shuffles, one barrier), which with u_t[0] gives m_t and the VALUES of the two
//   far candidates (the best s - jump and s - voicing over the voiced classes: rounding is monotone) -> s_t[j] = u_t[j] - m_t into LDS, and
//   the lowest CLASS that attains each value by a ballot per wave (one barrier) -> the band's 2W + 1 candidates of the thread's class from
//   LDS, the far candidate and the class-0 candidate -> bp_{t+1}[j] (uint16, workspace) and u_{t+1}[j].
// Two barriers and one shuffle reduction per frame: 2.6 us per frame measured on one long row (the first version reduced three (value,
// class) pairs by shuffles and read the band one class at a time: 3.5 us).
// One score buffer is enough: s_t is read between the second barrier of frame t and the first of frame t + 1 and written behind that
// one; the partial results likewise.  The emissions of the next four frames are in registers (a thread's loads are
// T floats apart, so every sixteenth frame is a miss for all 512 threads at once).
// Then the same workgroup walks back: 32 frames of back-pointers at a time return to LDS with 16-byte loads, thread 0 follows them there
// (a dependent LDS read per frame, where the walk through memory was a dependent miss per frame), and one thread per frame writes the
// class, f0 and the shifted f0.  No atomics on floats, no host synchronisation: the launch is capturable.
// The carry (tvc_pitch_path_carry_f32, tvc_convert_carry_f32) is a compile-time variant, pitch_path_kernel<true>: thread j adds the sanitised
// prior[row][j] to its first emission (one __syncthreads_or for the all -inf rule) and stores best_h[j], the best-predecessor value of frame h
// before e_h[j] is added, into carry_out[row][j] - the same thread reads and writes its element, so the two may be one array.  The calls
// without a carry launch pitch_path_kernel<false>, whose code is what it was.
// MEMORY SAFETY (the rule of tinyvc_hip.h): every frame leaves with a class whose s == 0.  The emissions are finite; a prior enters only
// through pp_prior below, which lets nothing but values <= 0 through and resets a state without a finite one - so m_t is finite, no score is
// NaN or positive, every ballot has a lane and every back-pointer is a class below 512.
#include <cmath>
#include <cstdint>

#include "small_kernels.h"
#include "tvc_common.h"

namespace tvc {

constexpr int kPpPad = kPitchPathMaxBand;      // -inf on both sides of the scores: the band needs no bounds
constexpr int kPpWaves = kPitchClasses / 64;
constexpr int kPpChunk = 32;                   // frames of back-pointers in LDS during the walk back
constexpr int PP_ROWS = 256;                   // utterances per launch: their tables travel as kernel arguments
constexpr float kPpClamp = 1e30f;
static_assert(kPitchClasses == 512, "one thread per class, uint16 back-pointers, 64 16-byte vectors per frame");

struct PitchPathRows {
    int start[PP_ROWS], len[PP_ROWS];
    float shift[PP_ROWS];
};
struct PitchPathOut {
    float* f0;
    float* f0s;
    int* path;
    float* score;
};
// the carried variant's share: prior / out [rows][512] (either may be nullptr, both may be one array), frame = h >= 1 (looked at with out only)
struct PitchPathCarryArgs {
    const float* prior;
    float* out;
    int frame;
};

__device__ __forceinline__ float pp_emission(float x) { return x != x ? -kPpClamp : fminf(fmaxf(x, -kPpClamp), kPpClamp); }
// a carried state as the recursion takes it, whatever a caller wrote there: values <= 0 (-inf included) as they are, everything else - NaN,
// positive values, +inf - counts as 0.  The caller (all 512 threads) turns a state that is -inf throughout into zeros.
__device__ __forceinline__ float pp_prior(float p) { return p <= 0.f ? p : 0.f; }

// f0 of class c at a frame whose logits are p[class * S]: freq[c] weighted over the classes within r of c (definition: tinyvc_hip.h)
__device__ __forceinline__ float pp_frequency(const float* __restrict__ p, long S, const float* __restrict__ freq, int c, int r) {
    if (c == 0) return 0.f;
    const int lo = c - r < 1 ? 1 : c - r, hi = c + r > kPitchClasses - 1 ? kPitchClasses - 1 : c + r;
    constexpr int NW = 2 * kPitchPathMaxRefine + 1;
    float x[NW], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        x[k] = lo + k <= hi ? pp_emission(p[(long)(lo + k) * S]) : -INFINITY;
        mx = fmaxf(mx, x[k]);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        x[k] = lo + k <= hi ? (float)exp((double)__fsub_rn(x[k], mx)) : 0.f;      // pitch_decode_kernel's exp: fp64, rounded once
        if (lo + k <= hi) den = k == 0 ? x[k] : __fadd_rn(den, x[k]);
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k)
        if (lo + k <= hi) {
            const float term = __fmul_rn(__fdiv_rn(x[k], den), freq[lo + k]);
            acc = k == 0 ? term : __fadd_rn(acc, term);
        }
    return acc <= 20.f ? 0.f : acc;
}

template <bool CARRY>
static __global__ __launch_bounds__(kPitchClasses) void pitch_path_kernel(PitchPathRows rows, int row0, const float* __restrict__ logits, long S,
                                                                          const float* __restrict__ freq, float step, int W, float jump, float voicing,
                                                                          int refine, uint16_t* __restrict__ bp, PitchPathOut out, PitchPathCarryArgs carry) {
    __shared__ float sc[kPpPad + kPitchClasses + kPpPad];      // s_t of the voiced classes; class 0's slot and the pads hold -inf
    __shared__ float s0;                                       // s_t[0]
    __shared__ float pm[kPpWaves];                             // the waves' maxima of u_t over the voiced classes,
    __shared__ float uz;                                       // and u_t[0]
    __shared__ int pi[2][kPpWaves];                            // the waves' lowest classes that attain the best s - jump [0] and s - voicing [1] (512: none)
    __shared__ int last;                                       // the lowest class with s_{T-1} == 0
    __shared__ __align__(16) uint16_t cb[kPpChunk][kPitchClasses];
    __shared__ int cpath[kPpChunk];
    const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const int T = rows.len[blockIdx.x];
    if (T <= 0) return;
    const long c0 = rows.start[blockIdx.x];
    // class k of column n lies at logits[(n / S) * 512 * S + k * S + n % S]; a row stays inside one run of S columns (checked by the host)
    const float* lg = logits + (c0 / S) * (long)kPitchClasses * S + c0 % S;
    const float* mine = lg + (long)j * S;
    uint16_t* bpr = bp + c0 * kPitchClasses;

    if (j < kPpPad) { sc[j] = -INFINITY; sc[kPpPad + kPitchClasses + j] = -INFINITY; }
    if (j == 0) { sc[kPpPad] = -INFINITY; last = kPitchClasses; }
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = 1 + k < T ? pp_emission(mine[1 + k]) : 0.f;
    float u = pp_emission(mine[0]), s = 0.f;
    if constexpr (CARRY) {
        if (carry.prior) {      // uniform over the workgroup: every thread meets the barrier
            float p = pp_prior(carry.prior[(long)(row0 + blockIdx.x) * kPitchClasses + j]);
            if (!__syncthreads_or(p != -INFINITY)) p = 0.f;      // -inf throughout: a reset
            u = __fadd_rn(p, u);
        }
    }
    for (int tb = 0; tb < T; tb += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = tb + k;      // u = u_t
            if (t >= T) break;
            // ONE reduction of values per frame: the maximum of u over the voiced classes (class 0's travels by itself).  m follows from it, and
            // so do the two far candidates' VALUES: rounding is monotone, so max_i (s[i] - jump) == (max_i s[i]) - jump, and the class that
            // holds the maximum computes the same s.  Their lowest CLASSES are then two ballots - which lanes attain the value - and no shuffle.
            float mv = j == 0 ? -INFINITY : u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mv = fmaxf(mv, __shfl_xor(mv, o));
            if (lane == 0) pm[wave] = mv;
            if (j == 0) uz = u;
            __syncthreads();
            mv = pm[0];
#pragma unroll
            for (int w = 1; w < kPpWaves; ++w) mv = fmaxf(mv, pm[w]);
            const float m = fmaxf(mv, uz);
            s = __fsub_rn(u, m);
            if (t == T - 1) break;
            const float sv = __fsub_rn(mv, m);                   // the best voiced score: some voiced class holds exactly this s
            const float fvj = __fsub_rn(sv, jump), fvv = __fsub_rn(sv, voicing);
            if (j == 0) s0 = s;
            else sc[kPpPad + j] = s;
            const unsigned long long bj = __ballot(j != 0 && __fsub_rn(s, jump) == fvj), bv = __ballot(j != 0 && __fsub_rn(s, voicing) == fvv);
            if (lane == 0) {
                pi[0][wave] = bj ? j + __ffsll((long long)bj) - 1 : kPitchClasses;
                pi[1][wave] = bv ? j + __ffsll((long long)bv) - 1 : kPitchClasses;
            }
            __syncthreads();
            // frame t + 1: the best predecessor of class j, the lowest on equal values
            const int sel = j == 0 ? 1 : 0;
            const float fv = sel ? fvv : fvj;
            int fi = pi[sel][0];
#pragma unroll
            for (int w = 1; w < kPpWaves; ++w) fi = min(fi, pi[sel][w]);
            float best;
            int from = 0;
            if (j == 0) {
                best = s0;                                       // 0 -> 0 costs nothing
                if (fv > best) { best = fv; from = fi; }
            } else {
                best = __fsub_rn(s0, voicing);                   // 0 -> j
                for (int d0 = -W; d0 <= W; d0 += 8) {            // the band, ascending: `>` keeps the lowest class; eight reads in flight at a time
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = sc[kPpPad + j + (d0 + q < W ? d0 + q : W)];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int d = d0 + q;
                        const float cand = __fsub_rn(v[q], __fmul_rn((float)(d < 0 ? -d : d), step));
                        if (d <= W && cand > best) { best = cand; from = j + d; }
                    }
                }
                // every voiced class by the jump route: never better than the band for a class inside it (jump >= W * step and rounding is
                // monotone), so the maximum over ALL voiced classes stands for the far ones; equal values go to the lower class
                if (fv > best || (fv == best && fi < from)) { best = fv; from = fi; }
            }
            bpr[(long)(t + 1) * kPitchClasses + j] = (uint16_t)from;
            if constexpr (CARRY) {
                if (carry.out && t + 1 == carry.frame) carry.out[(long)(row0 + blockIdx.x) * kPitchClasses + j] = best;
            }
            u = __fadd_rn(best, e[k]);
            if (t + 5 < T) e[k] = pp_emission(mine[t + 5]);
        }
    }
    // s = s_{T-1}[j]; its maximum is exactly 0, at every class whose u equals m
    if (out.score) out.score[(long)(row0 + blockIdx.x) * kPitchClasses + j] = s;
    if (s == 0.f) atomicMin(&last, j);
    __threadfence();      // the back-pointers of the other threads are read below
    __syncthreads();
    const float shift = rows.shift[blockIdx.x];
    auto emit = [&](int t, int c) {
        const float fv = pp_frequency(lg + t, S, freq, c, refine);
        if (out.path) out.path[c0 + t] = c;
        if (out.f0) out.f0[c0 + t] = fv;
        if (out.f0s) out.f0s[c0 + t] = shift_frequency_one(fv, shift);
    };
    int c = last;      // thread 0 keeps path[hi]
    if constexpr (CARRY) {
        if (c >= kPitchClasses) c = 0;      // never reached under the rule above; the walk back indexes LDS by c, so it does not rest on it
    }
    if (j == 0) emit(T - 1, c);
    for (int hi = T - 1; hi > 0;) {
        const int n = hi < kPpChunk ? hi : kPpChunk;      // back-pointers of frames hi - n + 1 .. hi give the classes of frames hi - n .. hi - 1
        const uint4* src = reinterpret_cast<const uint4*>(bpr + (long)(hi - n + 1) * kPitchClasses);
        uint4* dst = reinterpret_cast<uint4*>(&cb[0][0]);
        for (int v = j; v < n * (kPitchClasses / 8); v += kPitchClasses) dst[v] = src[v];
        __syncthreads();
        if (j == 0)
            for (int k = n - 1; k >= 0; --k) {
                c = cb[k][c];
                cpath[k] = c;
            }
        __syncthreads();
        if (j < n) emit(hi - n + j, cpath[j]);
        hi -= n;
    }
}

size_t pitch_path_ws_bytes(int64_t columns) { return (size_t)columns * kPitchClasses * sizeof(uint16_t); }

int pitch_path_check(const tvc_pitch_path& p, char* why, size_t why_bytes) {
    auto refuse = [&](const char* msg) {
        if (why && why_bytes) snprintf(why, why_bytes, "%s", msg);
        return (int)TVC_ERR_ARG;
    };
    if (!(p.step >= 0.f) || std::isinf(p.step)) return refuse("step must be finite and >= 0");
    if (p.band < 0 || p.band > kPitchPathMaxBand) return refuse("band must lie in 0 .. 32");
    if (!(p.jump >= (float)p.band * p.step)) return refuse("jump must be >= band * step (+inf is allowed)");
    if (!(p.voicing >= 0.f)) return refuse("voicing must be >= 0 (+inf is allowed)");
    if (p.refine < 0 || p.refine > kPitchPathMaxRefine) return refuse("refine must lie in 0 .. 4");
    if (why && why_bytes) why[0] = 0;
    return 0;
}

int run_pitch_path(tvc_ctx* ctx, hipStream_t s, const float* logits, long S, const std::vector<PitchPathRow>& rows, const tvc_pitch_path& p, uint16_t* bp,
                   float* f0, float* f0s, int* path_out, float* score_out, int carry_frame, const float* prior, float* carry_out) {
    if (!ctx->pitch_freq) return fail(ctx, TVC_ERR_STATE, "pitch table not uploaded (tvc_set_pitch_table + tvc_finalize_weights)");
    const PitchPathOut out{f0, f0s, path_out, score_out};
    const PitchPathCarryArgs carry{prior, carry_out, carry_out ? carry_frame : 0};
    const auto kernel = prior || carry_out ? pitch_path_kernel<true> : pitch_path_kernel<false>;
    for (size_t o = 0; o < rows.size(); o += PP_ROWS) {
        PitchPathRows r;
        const int n = (int)(rows.size() - o < PP_ROWS ? rows.size() - o : PP_ROWS);
        for (int i = 0; i < n; ++i) {
            r.start[i] = rows[o + i].start;
            r.len[i] = rows[o + i].len;
            r.shift[i] = rows[o + i].shift;
        }
        hipLaunchKernelGGL(kernel, dim3(n), dim3(kPitchClasses), 0, s, r, (int)o, logits, S, ctx->pitch_freq, p.step, p.band, p.jump, p.voicing, p.refine, bp,
                           out, carry);
    }
    return launch_check(ctx, "pitch_path");
}

}  // namespace tvc
