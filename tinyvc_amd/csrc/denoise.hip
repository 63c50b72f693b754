// The spectral suppressor of a set of streams (extension; tvc_stream_denoise_f32): one launch in front of the rolling window (stream_push),
// one workgroup per stream.  The 24 kHz block goes through a short-time spectral gain - 640-sample frames under a square-root Hann window at
// a hop of 160 or 320, a noise estimate per bin, the gain G = max(floor, 1 - beta * noise / smooth), weighted overlap-add - and comes out
// delayed by 640 - hop samples.  The definition (tinyvc_hip.h) is a recurrence over a stream's frames with two 321-bin arrays, two sample
// tails and a frame count of state per stream; the reduction and the state are read from device memory when the kernel runs, so a captured
// block replays as the reduction moves and the streams advance and restart.
// A frame is 640 real samples = one complex FFT of 320 points on z[m] = x[2m] + i x[2m+1] plus the even/odd untangling; 320 = 64 x 5:
// fft320_wave (fft_wave.h) is fft.hip's wave-level plan with the 5-point DFT in registers.  Tables (pack.hip pack_constants, fp64-made):
// win[n] = sqrt(0.5 - 0.5 cos(2 pi n / 640)), tw320[j] = (cos, sin)(2 pi j / 320), tw640[k] = (cos, sin)(2 pi k / 640).
#include "fft_wave.h"
#include "tvc_common.h"

namespace tvc {

// The one place that says which suppressor geometries the kernel takes (tvc_stream_denoise_geometry and through it tvc_stream_denoise_f32).
// 0, or TVC_ERR_ARG with the reason in `why` (nullable):
//   hop is 160 or 320                                   the synthesis scale 2 hop / 640 makes the overlap-add of the squared window 1
//   block >= hop, block % hop == 0                      whole frames per block
//   block / hop <= 4096
int stream_denoise_geometry(int block, int hop, int* frames, int* delay, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, int v, int w) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v, w);
        return (int)TVC_ERR_ARG;
    };
    if (hop != 160 && hop != 320) return refuse("hop = %d is neither 160 nor 320", hop, 0);
    if (block < hop) return refuse("block = %d is shorter than one hop of %d samples", block, hop);
    if (block % hop) return refuse("block = %d is not a whole number of %d-sample hops", block, hop);
    if (block / hop > kDenoiseMaxFrames) return refuse("block / hop = %d frames is above %d", block / hop, kDenoiseMaxFrames);
    if (why && why_bytes) why[0] = 0;
    if (frames) *frames = block / hop;
    if (delay) *delay = kDenoiseFrame - hop;
    return 0;
}

namespace {

constexpr int kNF = kDenoiseFrame;      // 640 samples per frame
constexpr int kM = kNF / 2;             // complex FFT size
constexpr int kNB = kDenoiseBins;       // 321 bins
constexpr int kW = 8;                   // frames (waves) per group
constexpr int kRow = kNB + 1;           // float2 row stride of a frame's bins / samples in LDS
constexpr int kMaxHop = 320, kMaxD = kNF - 160;
constexpr int kXin = kMaxD + kW * kMaxHop;      // >= D + kW * hop for both hops: a group's input samples

// x / out [S][block] (out may be x: a group's input is in LDS before its output is written, and later groups read behind it).
// Frames go in groups of kW, a wave per frame:  1. the group's input (the carried tail ++ the block's next samples) into LDS;
// 2. forward transforms, a wave per frame, bins into the wave's LDS row (a frame of +-0 only is flagged and skipped everywhere);
// 3. the per-bin recurrence across the group's frames in order, a thread per bin, smooth / noise in registers from group to group,
//    Y = G X in place;  4. inverse transforms, a wave per frame, samples into the wave's row;  5. a thread per output position adds the
//    frames' windowed samples in ascending frame order onto the carried overlap-add tail; finished samples leave, the rest is the new tail.
__global__ __launch_bounds__(kW * 64) void stream_denoise_kernel(const float* x, float* out, StreamDenoise d, float oma_s, float oma_n, const float* __restrict__ win_g,
                                                                 const float2* __restrict__ tw320, const float2* __restrict__ tw640) {
    __shared__ __attribute__((aligned(16))) float2 rows[kW * kRow];
    __shared__ float xin[kXin];
    __shared__ float ola[2][kMaxD];
    __shared__ float win[kNF];
    __shared__ float red[kNB + 7];
    __shared__ int nz[kW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long st = blockIdx.x;
    const int hop = d.hop, D = kNF - hop, F = d.block / hop;
    const float* xs = x + st * d.block;
    float* os = out + st * d.block;
    const float scale = hop == 160 ? 0.5f : 1.0f;      // 2 hop / 640
    const float isc = 1.f / (float)kNF;

    for (int i = tid; i < kNF; i += kW * 64) win[i] = win_g[i];
    for (int i = tid; i < D; i += kW * 64) {
        xin[i] = d.hist[st * D + i];
        ola[0][i] = d.ola[st * D + i];
    }
    float smooth = 0.f, noise = 0.f;
    if (tid < kNB) {
        smooth = d.smooth[st * kNB + tid];
        noise = d.noise[st * kNB + tid];
    }
    int count = d.frames[st];
    const float red_db = fmaxf(d.reduction_db[st], 0.f);
    const float floor_g = red_db == 0.f ? 1.f : exp10f(-red_db / 20.f);      // (10^-0 is 1: the branch only spares the call)
    int cur = 0;

    for (int m0 = 0; m0 < F; m0 += kW) {
        const int nf = F - m0 < kW ? F - m0 : kW;
        // 1. the samples behind the carried tail
        for (int i = tid; i < nf * hop; i += kW * 64) xin[D + i] = xs[(long)m0 * hop + i];
        __syncthreads();
        // 2. forward: z[m] = w x[2m] + i w x[2m+1], m = 64 n2 + lane
        bool live = false;
        if (wave < nf) {
            const float* f = xin + wave * hop;
            float2 v[5];
            unsigned any = 0;
#pragma unroll
            for (int n2 = 0; n2 < 5; ++n2) {
                const int n = 2 * (64 * n2 + lane);
                const float a = f[n], b = f[n + 1];
                any |= (__float_as_uint(a) | __float_as_uint(b)) & 0x7fffffffu;
                v[n2] = make_float2(__fmul_rn(a, win[n]), __fmul_rn(b, win[n + 1]));
            }
            live = __any(any != 0);
            if (lane == 0) nz[wave] = live ? 1 : 0;
            if (live) {
                fft320_wave<-1>(v, lane, tw320);
                const int k1 = bitrev6(lane);
                float2* Z = rows + wave * kRow;
#pragma unroll
                for (int k2 = 0; k2 < 5; ++k2) Z[5 * k1 + k2] = v[k2];
            }
        }
        __syncthreads();
        constexpr int NK = (kM + 64) / 64;      // bins per lane: k = lane + 64 i <= 320
        float2 X[NK];
        if (live) {
            // X[k] = (Z[k] + conj Z[M-k]) / 2 - i W_640^k (Z[k] - conj Z[M-k]) / 2
            const float2* Z = rows + wave * kRow;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const int k = lane + 64 * i;
                X[i] = make_float2(0.f, 0.f);
                if (k <= kM) {
                    const float2 a = Z[k == kM ? 0 : k], c = Z[k == 0 ? 0 : kM - k];
                    const float2 e = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
                    const float2 o = make_float2(0.5f * (a.x - c.x), 0.5f * (a.y + c.y));
                    const float2 w = tw640[k];                                 // (cos, sin): W = cos - i sin
                    X[i].x = e.x + fmaf(w.x, o.y, -w.y * o.x);
                    X[i].y = (k == 0 || k == kM) ? 0.f : e.y - fmaf(w.x, o.x, w.y * o.y);      // DC and Nyquist of a real signal are real
                }
            }
        }
        __syncthreads();                        // every wave has read its Z before the row takes X
        if (live) {
            float2* Xr = rows + wave * kRow;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const int k = lane + 64 * i;
                if (k <= kM) Xr[k] = X[i];
            }
        }
        __syncthreads();
        // 3. the recurrence, frame after frame; `count` is the same number in every thread
        for (int f = 0; f < nf; ++f) {
            if (!nz[f]) continue;
            if (tid < kNB) {
                float2* Xr = rows + f * kRow;
                const float2 v = Xr[tid];
                const float P = fmaf(v.x, v.x, v.y * v.y);
                smooth = fmaf(d.a_s, smooth, oma_s * P);
                if (count < d.warm) {
                    noise = noise + (P - noise) / (float)(count + 1);
                } else {
                    const float cap = fmaxf(d.clamp * noise, TVC_STREAM_DENOISE_NMIN);
                    noise = fmaf(d.a_n, noise, oma_n * fminf(P, cap));
                }
                const float G = fmaxf(floor_g, 1.f - d.beta * noise / fmaxf(smooth, 1e-30f));
                Xr[tid] = make_float2(G * v.x, G * v.y);
            }
            count = count < (1 << 30) ? count + 1 : count;
        }
        __syncthreads();
        // 4. inverse: Z[k] = E[k] + i O[k],  E = Y[k] + conj Y[M-k],  O = (Y[k] - conj Y[M-k]) e^(+2 pi i k / 640),  k = 0..319
        float2 v[5];
        if (live) {
            const float2* Y = rows + wave * kRow;
#pragma unroll
            for (int n2 = 0; n2 < 5; ++n2) {
                const int k = 64 * n2 + lane;
                const float2 a = Y[k], c = Y[kM - k];
                const float2 e = make_float2(a.x + c.x, a.y - c.y), dd = make_float2(a.x - c.x, a.y + c.y);
                const float2 w = tw640[k];
                const float2 o = make_float2(fmaf(dd.x, w.x, -dd.y * w.y), fmaf(dd.x, w.y, dd.y * w.x));
                v[n2] = make_float2(e.x - o.y, e.y + o.x);
            }
        }
        __syncthreads();                        // every wave has read its Y before the row takes the samples
        if (live) {
            fft320_wave<+1>(v, lane, tw320);
            const int k1 = bitrev6(lane);
            float2* Y = rows + wave * kRow;
#pragma unroll
            for (int k2 = 0; k2 < 5; ++k2) Y[5 * k1 + k2] = make_float2(v[k2].x * isc, v[k2].y * isc);      // (y[2m], y[2m+1]), m = 5 k1 + k2
        }
        // the tail of the input the next group starts from: D <= 480 < the workgroup's threads, one value each
        const float keep = tid < D ? xin[nf * hop + tid] : 0.f;
        __syncthreads();
        if (tid < D) xin[tid] = keep;
        // 5. overlap-add in ascending frame order onto the carried tail
        const float* ys = reinterpret_cast<const float*>(rows);
        for (int q = tid; q < nf * hop + D; q += kW * 64) {
            float a = q < D ? ola[cur][q] : 0.f;
            for (int f = 0; f < nf; ++f) {
                const int n = q - f * hop;
                if (n >= 0 && n < kNF && nz[f]) a = __fadd_rn(a, __fmul_rn(__fmul_rn(ys[f * (2 * kRow) + n], win[n]), scale));
            }
            if (q < nf * hop) os[(long)m0 * hop + q] = a;
            else ola[cur ^ 1][q - nf * hop] = a;
        }
        cur ^= 1;
        __syncthreads();
    }

    for (int i = tid; i < D; i += kW * 64) {
        d.hist[st * D + i] = xin[i];
        d.ola[st * D + i] = ola[cur][i];
    }
    if (tid < kNB) {
        d.smooth[st * kNB + tid] = smooth;
        d.noise[st * kNB + tid] = noise;
        red[tid] = (tid == 0 || tid == kM) ? noise : 2.f * noise;
    }
    if (tid == 0) d.frames[st] = count;
    if (d.noise_db) {
        __syncthreads();
        if (wave == 0) {
            float acc = 0.f;
            for (int k = lane; k < kNB; k += 64) acc += red[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) d.noise_db[st] = 10.f * log10f(fmaxf(acc / (float)(kNF * kM), 1e-20f));
        }
    }
}

}  // namespace

int run_stream_denoise(tvc_ctx* ctx, hipStream_t s, const float* x, float* out, int S, const StreamDenoise& d) {
    if (!ctx->dn_win || !ctx->dn_tw320 || !ctx->dn_tw640) return fail(ctx, TVC_ERR_STATE, "the suppressor's tables are missing");
    static_assert(kMaxD + kW * 160 <= kXin && 160 + kW * kMaxHop <= kXin, "a group's input fits for both hops");
    static_assert(kMaxD < kW * 64, "one carried input sample per thread");
    hipLaunchKernelGGL(stream_denoise_kernel, dim3((unsigned)S), dim3(kW * 64), 0, s, x, out, d, 1.0f - d.a_s, 1.0f - d.a_n, ctx->dn_win,
                       reinterpret_cast<const float2*>(ctx->dn_tw320), reinterpret_cast<const float2*>(ctx->dn_tw640));
    return launch_check(ctx, "stream_denoise");
}

}  // namespace tvc
