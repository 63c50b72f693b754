// Front door of the entry scripts, on the device: sample-rate conversion to the model's 24 kHz
// (reference infer.py:46,63 / infer_streaming.py:70 call torchaudio.functional.resample), int16 PCM <-> fp32 and dB gain
// (infer_streaming.py:85-94).  torchaudio is third-party arithmetic that is absent from the build image, so the resampler
// restates its documented default algorithm (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and its parity is
// pinned only against this repository's own host restatement (tinyvc_amd/resample.py).
#include <cmath>
#include <map>
#include <utility>

#include "small_kernels.h"
#include <mutex>

#include "tvc_common.h"

namespace tvc {

// y[r][t] = sum_k kern[t % new][k] * x[r][(t / new) * orig + k - width]   (zero outside [0, n))
// = torchaudio's conv1d(pad(x, (width, width + orig)), kern, stride = orig), output interleaved over the `new` phases.
static __global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, long n, long n_out,
                                                              const float* __restrict__ kern, int orig, int newf, int width, int taps) {
    const long total = (long)rows * n_out;
    for (long o = blockIdx.x * (long)blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const long r = o / n_out, t = o - r * n_out;
        const long j = t / newf;
        const int i = (int)(t - j * newf);
        const float* kr = kern + (long)i * taps;
        const float* xr = x + r * n;
        const long base = j * orig - width;
        float acc = 0.f;
        for (int k = 0; k < taps; ++k) {
            const long p = base + k;
            const float v = (p >= 0 && p < n) ? xr[p] : 0.f;
            acc = fmaf(kr[k], v, acc);
        }
        y[o] = acc;
    }
}

// chunk = int16 / 32768, then torchaudio.functional.gain (x * 10^(dB/20); skipped for 0 dB)   (infer_streaming.py:85-89)
static __global__ void pcm16_to_f32_kernel(const int16_t* __restrict__ pcm, float* __restrict__ y, long n, float ratio, int apply) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = (float)pcm[i] / 32768.f;
        if (apply) v = v * ratio;
        y[i] = v;
    }
}
// gain, * 32768, numpy's float32 -> int16 cast: truncation toward zero, out-of-range values wrap through int32
// (infer_streaming.py:91-94)
static __global__ void f32_to_pcm16_kernel(const float* __restrict__ x, int16_t* __restrict__ pcm, long n, float ratio, int apply) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = x[i];
        if (apply) v = v * ratio;
        v = v * 32768.f;
        const int q = (v != v || fabsf(v) >= 2147483648.f) ? (int)0x80000000 : (int)v;   // x86 cvttss2si's "indefinite" outside int32
        pcm[i] = (int16_t)(unsigned short)(q & 0xffff);
    }
}

static long gcd_l(long a, long b) { return b ? gcd_l(b, a % b) : a; }

// A rate pair reduced to lowest terms and the filter torchaudio's defaults give it: `width` input samples on either side of an output
// group, taps = 2 * width + orig per phase.  The one place these are computed: the table and the streaming door's geometry both start here.
constexpr double kLowpassWidth = 6.0, kRolloff = 0.99;
struct RateGeometry {
    int orig, newf, width, taps;
    double base;
};
static RateGeometry rate_geometry(int orig_freq, int new_freq) {
    const long g = gcd_l(orig_freq, new_freq);
    RateGeometry r;
    r.orig = (int)(orig_freq / g);
    r.newf = (int)(new_freq / g);
    r.base = (double)(r.orig < r.newf ? r.orig : r.newf) * kRolloff;
    r.width = (int)std::ceil(kLowpassWidth * r.orig / r.base);
    r.taps = 2 * r.width + r.orig;
    return r;
}

struct ResampleTable {
    float* kern = nullptr;
    int orig = 0, newf = 0, width = 0, taps = 0;
};
static std::map<std::pair<tvc_ctx*, std::pair<int, int>>, ResampleTable>& tables() {
    static std::map<std::pair<tvc_ctx*, std::pair<int, int>>, ResampleTable> t;
    return t;
}
static std::mutex& tables_mu() {      // one host thread per ctx is the contract, but the map is shared by the ctxs of a process
    static std::mutex m;
    return m;
}

// Hann-windowed sinc filter bank, computed in fp64 and rounded once (the formula of tinyvc_amd/resample.py:_kernel)
// (the first use of a rate pair allocates and uploads its table synchronously: not inside a stream capture)
static int get_table(tvc_ctx* ctx, int orig_freq, int new_freq, ResampleTable* out) {
    std::lock_guard<std::mutex> lk(tables_mu());
    auto key = std::make_pair(ctx, std::make_pair(orig_freq, new_freq));
    auto it = tables().find(key);
    if (it != tables().end()) {
        *out = it->second;
        return 0;
    }
    const RateGeometry rg = rate_geometry(orig_freq, new_freq);
    const int orig = rg.orig, newf = rg.newf, width = rg.width, taps = rg.taps;
    const double lpw = kLowpassWidth, pi = 3.14159265358979323846, base = rg.base;
    std::vector<float> k((size_t)newf * taps);
    for (int i = 0; i < newf; ++i)
        for (int c = 0; c < taps; ++c) {
            double t = ((double)(-i) / newf + (double)(c - width) / orig) * base;
            t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
            const double w = std::cos(t * pi / lpw / 2.0);
            t *= pi;
            const double sinc = t == 0.0 ? 1.0 : std::sin(t) / t;
            k[(size_t)i * taps + c] = (float)(sinc * (w * w) * (base / orig));
        }
    ResampleTable tb;
    tb.orig = orig;
    tb.newf = newf;
    tb.width = width;
    tb.taps = taps;
    TVC_HIP(ctx, hipMalloc((void**)&tb.kern, k.size() * sizeof(float)));      // one-off per (ctx, rate pair), outside any hot path
    TVC_HIP(ctx, hipMemcpy(tb.kern, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice));
    tables()[key] = tb;
    *out = tb;
    return 0;
}

void frontdoor_release(tvc_ctx* ctx) {
    std::lock_guard<std::mutex> lk(tables_mu());
    for (auto it = tables().begin(); it != tables().end();) {
        if (it->first.first == ctx) {
            if (it->second.kern) (void)hipFree(it->second.kern);
            it = tables().erase(it);
        } else {
            ++it;
        }
    }
}

int64_t resample_out_len(int64_t n, int orig_freq, int new_freq) {
    if (n <= 0 || orig_freq <= 0 || new_freq <= 0) return 0;
    const long g = gcd_l(orig_freq, new_freq);
    const long orig = orig_freq / g, newf = new_freq / g;
    return (newf * n + orig - 1) / orig;          // ceil(new * n / orig), torchaudio's target length
}

int run_resample(tvc_ctx* ctx, hipStream_t s, const float* x, float* y, int rows, int64_t n, int orig_freq, int new_freq) {
    ResampleTable tb;
    TVC_CHECK(get_table(ctx, orig_freq, new_freq, &tb));
    const long n_out = resample_out_len(n, orig_freq, new_freq);
    hipLaunchKernelGGL(resample_kernel, dim3(grid_for((long)rows * n_out)), dim3(256), 0, s, x, y, rows, (long)n, n_out, tb.kern, tb.orig, tb.newf,
                       tb.width, tb.taps);
    return launch_check(ctx, "resample");
}

static float db_ratio(float gain_db) { return (float)std::pow(10.0, (double)gain_db / 20.0); }

int run_pcm16_to_f32(tvc_ctx* ctx, hipStream_t s, const int16_t* pcm, float* y, int64_t n, float gain_db) {
    hipLaunchKernelGGL(pcm16_to_f32_kernel, dim3(grid_for(n)), dim3(256), 0, s, pcm, y, (long)n, db_ratio(gain_db), gain_db != 0.f);
    return launch_check(ctx, "pcm16_to_f32");
}
int run_f32_to_pcm16(tvc_ctx* ctx, hipStream_t s, const float* x, int16_t* pcm, int64_t n, float gain_db) {
    hipLaunchKernelGGL(f32_to_pcm16_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, pcm, (long)n, db_ratio(gain_db), gain_db != 0.f);
    return launch_check(ctx, "f32_to_pcm16");
}

// ---- the streaming door: resample_kernel's sums block by block, one workgroup per stream -------------------------------------------------
// A stream's history is its last hist = G * orig + width input samples (G = ceil(width / orig) whole groups of look-ahead), fp32, zeros
// at the start.  With buf = state ++ block (hist + n_in samples, staged in LDS) local output u = jl * new + i is
//     y[u] = sum_k kern[i][k] * buf[jl * orig + k],   k = 0 .. taps - 1 ascending, one fmaf chain from 0.f
// - the chain resample_kernel runs for output G * new + u of (G * orig zeros ++ the stream so far): every block of every stream equals the
// offline result on that input, bit for bit, G * new outputs late.  The highest index read is n_in + 2 * width - 1 < hist + n_in.
// IN16 / OUT16: pcm16_to_f32_kernel's arithmetic on the way into LDS, f32_to_pcm16_kernel's on the way out.  The state is read before the
// one barrier and written after it, and LDS is not written after it, so the hand-over needs no second one (also when n_in < hist: the new
// state is buf[n_in .. n_in + hist), part old state, part block).
constexpr int kDoorThreads = 1024;
constexpr int kDoorLdsFloats = TVC_STREAM_RESAMPLE_LDS_FLOATS;

template <bool IN16, bool OUT16>
static __global__ __launch_bounds__(kDoorThreads) void stream_resample_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                                              float* __restrict__ state, int n_in, int n_out,
                                                                              const float* __restrict__ kern, int orig, int newf, int taps,
                                                                              int hist, float ratio, int apply) {
    extern __shared__ __attribute__((aligned(16))) float buf[];
    const int tid = threadIdx.x;
    float* srow = state + (long)blockIdx.x * hist;
    for (int i = tid; i < hist; i += kDoorThreads) buf[i] = srow[i];
    float* blk = buf + hist;
    if (IN16) {
        const int16_t* p = (const int16_t*)in + (long)blockIdx.x * n_in;
        const auto cvt = [&](int16_t s) {
            float v = (float)s / 32768.f;
            if (apply) v = v * ratio;
            return v;
        };
        // four samples per 8-byte load between the row's first 8-byte boundary and its last (rows start wherever S * n_in puts them)
        int head = (int)((0 - (uintptr_t)p) & 7) >> 1;
        if (head > n_in) head = n_in;
        const int quads = (n_in - head) >> 2;
        const short4* p4 = (const short4*)(p + head);
        for (int q = tid; q < quads; q += kDoorThreads) {
            const short4 s4 = p4[q];
            float* d = blk + head + 4 * q;
            d[0] = cvt(s4.x);
            d[1] = cvt(s4.y);
            d[2] = cvt(s4.z);
            d[3] = cvt(s4.w);
        }
        const int tail0 = head + 4 * quads;
        for (int i = tid; i < head + (n_in - tail0); i += kDoorThreads) {
            const int j = i < head ? i : tail0 + (i - head);
            blk[j] = cvt(p[j]);
        }
    } else {
        const float* p = (const float*)in + (long)blockIdx.x * n_in;
        for (int i = tid; i < n_in; i += kDoorThreads) blk[i] = p[i];
    }
    __syncthreads();
    const auto put = [&](int u, float acc) {
        if (OUT16) {
            float v = acc;
            if (apply) v = v * ratio;
            v = v * 32768.f;
            const int q = (v != v || fabsf(v) >= 2147483648.f) ? (int)0x80000000 : (int)v;
            ((int16_t*)out)[(long)blockIdx.x * n_out + u] = (int16_t)(unsigned short)(q & 0xffff);
        } else {
            ((float*)out)[(long)blockIdx.x * n_out + u] = acc;
        }
    };
    if (newf == 1) {      // one phase: kern[k] is the same address for the whole workgroup, so the row comes through the scalar cache
        for (int u = tid; u < n_out; u += kDoorThreads) {
            const float* x = buf + u * orig;
            float acc = 0.f;
            for (int k = 0; k < taps; ++k) acc = fmaf(kern[k], x[k], acc);
            put(u, acc);
        }
    } else {
        for (int u = tid; u < n_out; u += kDoorThreads) {
            const int jl = u / newf, i = u - jl * newf;
            const float* kr = kern + (long)i * taps;
            const float* x = buf + jl * orig;
            float acc = 0.f;
            for (int k = 0; k < taps; ++k) acc = fmaf(kr[k], x[k], acc);
            put(u, acc);
        }
    }
    for (int i = tid; i < hist; i += kDoorThreads) srow[i] = buf[n_in + i];
}

int stream_resample_geometry(int in_freq, int out_freq, int64_t n_in, int64_t* n_out, int* hist, int* delay) {
    if (in_freq <= 0 || out_freq <= 0 || n_in <= 0) return TVC_ERR_ARG;
    if (in_freq == out_freq) {
        *n_out = n_in;
        *hist = *delay = 0;
        return 0;
    }
    const RateGeometry rg = rate_geometry(in_freq, out_freq);
    if (n_in % rg.orig != 0) return TVC_ERR_ARG;
    const int G = (rg.width + rg.orig - 1) / rg.orig;
    const long h = (long)G * rg.orig + rg.width;
    if (h + n_in > kDoorLdsFloats) return TVC_ERR_ARG;
    *n_out = n_in / rg.orig * rg.newf;
    *hist = (int)h;
    *delay = G * rg.newf;
    return 0;
}

int stream_resample_prepare(tvc_ctx* ctx, int in_freq, int out_freq) {
    ResampleTable tb;
    return in_freq == out_freq ? 0 : get_table(ctx, in_freq, out_freq, &tb);
}

int run_stream_resample(tvc_ctx* ctx, hipStream_t s, const void* in, bool in16, void* out, bool out16, float* state, int S, int64_t n_in,
                        int in_freq, int out_freq, float gain_db) {
    int64_t n_out = 0;
    int hist = 0, delay = 0;
    if (stream_resample_geometry(in_freq, out_freq, n_in, &n_out, &hist, &delay) != 0)
        return fail(ctx, TVC_ERR_ARG,
                    "tvc_stream_resample: %d -> %d Hz takes blocks of whole input groups whose history + block fit %d floats of LDS; got n_in = %ld",
                    in_freq, out_freq, kDoorLdsFloats, (long)n_in);
    if (in_freq == out_freq) {      // no filter, no history: the plain conversions
        if (in16) return run_pcm16_to_f32(ctx, s, (const int16_t*)in, (float*)out, (int64_t)S * n_in, gain_db);
        if (out16) return run_f32_to_pcm16(ctx, s, (const float*)in, (int16_t*)out, (int64_t)S * n_in, gain_db);
        TVC_HIP(ctx, hipMemcpyAsync(out, in, (size_t)S * n_in * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    {      // the table's first use allocates and copies synchronously, which a capture cannot record
        std::lock_guard<std::mutex> lk(tables_mu());
        const bool known = tables().count(std::make_pair(ctx, std::make_pair(in_freq, out_freq))) != 0;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (!known && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
            return fail(ctx, TVC_ERR_STATE, "tvc_stream_resample: the %d -> %d Hz table is not built yet; call tvc_stream_resample_prepare before the capture",
                        in_freq, out_freq);
    }
    ResampleTable tb;
    TVC_CHECK(get_table(ctx, in_freq, out_freq, &tb));
    const size_t lds = (size_t)(hist + n_in) * sizeof(float);
    const float ratio = db_ratio(gain_db);
    const int apply = gain_db != 0.f;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(kDoorThreads), lds, s, in, out, state, (int)n_in, (int)n_out, tb.kern, tb.orig, tb.newf,
                           tb.taps, hist, ratio, apply);
    };
    if (in16) launch(stream_resample_kernel<true, false>);
    else if (out16) launch(stream_resample_kernel<false, true>);
    else launch(stream_resample_kernel<false, false>);
    return launch_check(ctx, "stream_resample");
}

}  // namespace tvc
