// The noise gate of a set of streams (extension; tvc_stream_gate_f32): one launch behind the streaming tail (sola.hip), one workgroup per
// stream.  The emitted block y [block] is multiplied by a gain that follows the power of the INPUT samples the block was converted from -
// x[a + j] for y[j], a = base + the lag SOLA chose on the device - and of the `look` sub-frames of input behind them, which the rolling
// window already holds: look-ahead without latency.  The definition (tinyvc_hip.h) is a serial scan over the block's sub-frames with three
// words of state per stream; everything a client may move between blocks (threshold, state) is read from device memory when the kernel
// runs, so a captured block replays as the thresholds move and the streams open, close and restart.
#include "tvc_common.h"

namespace tvc {

// The one place that says which gate geometries the kernel takes (tvc_stream_gate_geometry and through it tvc_stream_gate_f32).  0, or
// TVC_ERR_ARG with the reason in `why` (nullable):
//   4 <= sub <= 65536, sub % 4 == 0, block >= 1, block % sub == 0      whole sub-frames; the per-sample ramp is (j + 1) / sub
//   look >= 0, block / sub + look <= 4096                              the powers of a block and its look-ahead sit in LDS
//   0 <= hold <= 2^20, 1 <= attack, release <= 2^20                    counts of sub-frames (and 1 / attack stays a normal fp32 step)
int stream_gate_geometry(int block, int sub, int look, int hold, int attack, int release, int* nsub, int* look_samples, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, int v, int w) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v, w);
        return (int)TVC_ERR_ARG;
    };
    if (sub < 4 || sub > kGateMaxSubFrame) return refuse("sub = %d is outside 4 .. %d", sub, kGateMaxSubFrame);
    if (sub % 4) return refuse("sub = %d is not a multiple of 4", sub, 0);
    if (block < 1) return refuse("block = %d is not positive", block, 0);
    if (block % sub) return refuse("block = %d is not a whole number of %d-sample sub-frames", block, sub);
    if (look < 0) return refuse("look = %d is negative", look, 0);
    if ((int64_t)block / sub + look > kGateMaxSub)
        return refuse("block / sub + look = %d sub-frames is above %d", (int)std::min<int64_t>((int64_t)block / sub + look, INT32_MAX), kGateMaxSub);
    if (hold < 0 || hold > kGateMaxCount) return refuse("hold = %d is outside 0 .. %d", hold, kGateMaxCount);
    if (attack < 1 || attack > kGateMaxCount) return refuse("attack = %d is outside 1 .. %d", attack, kGateMaxCount);
    if (release < 1 || release > kGateMaxCount) return refuse("release = %d is outside 1 .. %d", release, kGateMaxCount);
    if (why && why_bytes) why[0] = 0;
    if (nsub) *nsub = block / sub;
    if (look_samples) *look_samples = look * sub;      // <= 4096 * 65536 = 2^28
    return 0;
}

// the host's share of the definition, as fp32 kernel arguments
struct GateConst {
    float close_ratio;      // 10^(-hysteresis_db / 10): T_close = T_open * close_ratio
    float floor;            // 10^(range_db / 20), 0 at -inf
    float up, down;         // 1.0f / attack, 1.0f / release
};

// x [S][n] input windows, y / out [S][block] (out may be y: a thread reads y[i] before it writes out[i], and nobody else touches i).
// 1. p[i], i < nsub + look: one wave per sub-frame, lanes strided over its samples (the start a = base + shift has any alignment: plain
//    4-byte loads), an index outside [0, n) reads 0;  2. d[i] = max(p[i .. i + look]), NaN if one of them is;  3. lane 0 scans the nsub
//    sub-frames in order and leaves the gain at every sub-frame edge in gs[0 .. nsub], another wave's lane 0 takes the level;
// 4. all lanes apply the per-sample ramp.
static __global__ __launch_bounds__(256) void stream_gate_kernel(const float* __restrict__ x, long n, long base, const int32_t* __restrict__ shift,
                                                                 const float* y, float* out, StreamGate g, GateConst c) {
    __shared__ float p[kGateMaxSub];
    __shared__ float d[kGateMaxSub];
    __shared__ float gs[kGateMaxSub + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long st = blockIdx.x;
    const int sub = g.sub, nsub = g.block / sub, np = nsub + g.look;
    const float* xs = x + st * n;
    const long a = base + (shift ? (long)shift[st] : 0L);

    for (int i = wave; i < np; i += 4) {
        const long a0 = a + (long)i * sub;
        float acc = 0.f;
        for (int j = lane; j < sub; j += 64) {
            const long idx = a0 + j;
            const float v = idx >= 0 && idx < n ? xs[idx] : 0.f;
            acc = fmaf(v, v, acc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) p[i] = acc / (float)sub;
    }
    __syncthreads();
    for (int i = tid; i < nsub; i += 256) {
        float m = p[i];
        bool nan = m != m;
        for (int k = 1; k <= g.look; ++k) {
            const float v = p[i + k];
            nan |= v != v;
            m = fmaxf(m, v);
        }
        d[i] = nan ? __int_as_float(0x7fc00000) : m;
    }
    __syncthreads();
    if (tid == 0) {
        int open = g.open[st] != 0, hold = g.hold_state[st];
        float gain = g.gain[st];
        const float t_open = exp10f(g.threshold_db[st] / 10.f);      // -inf dB -> 0: every d that is a number opens; a NaN threshold: none does
        const float t_close = __fmul_rn(t_open, c.close_ratio);
        gs[0] = gain;
        for (int i = 0; i < nsub; ++i) {
            const float di = d[i];
            if (di >= t_open) {
                open = 1;
                hold = g.hold;
            } else if (open && di >= t_close) {
                hold = g.hold;
            } else if (open) {
                if (hold > 0) --hold;
                else open = 0;
            }
            const float tgt = open ? 1.f : c.floor;
            gain = tgt > gain ? fminf(tgt, __fadd_rn(gain, c.up)) : fmaxf(tgt, __fsub_rn(gain, c.down));
            gs[i + 1] = gain;
        }
        g.open[st] = open;
        g.hold_state[st] = hold;
        g.gain[st] = gain;
    } else if (tid == 64 && g.level_db) {
        double acc = 0.;
        for (int i = 0; i < nsub; ++i) acc += (double)p[i];
        g.level_db[st] = 10.f * log10f(fmaxf((float)(acc / (double)nsub), 1e-20f));
    }
    __syncthreads();
    const float* ys = y + st * g.block;
    float* os = out + st * g.block;
    const float fsub = (float)sub;
    for (int i = tid; i < g.block; i += 256) {
        const int f = i / sub, j = i - f * sub;
        const float g0 = gs[f], g1 = gs[f + 1];
        // g0 == g1: (g1 - g0) * t is +-0 and the multiplier is g0 exactly - an open gate changes no bit, a closed one at floor 0 emits zeros
        const float m = __fadd_rn(g0, __fmul_rn(__fsub_rn(g1, g0), __fdiv_rn((float)(j + 1), fsub)));
        os[i] = __fmul_rn(ys[i], m);
    }
}

int run_stream_gate(tvc_ctx* ctx, hipStream_t s, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                    const StreamGate& g) {
    GateConst c;
    c.close_ratio = (float)std::pow(10.0, -(double)g.hysteresis_db / 10.0);
    c.floor = (float)std::pow(10.0, (double)g.range_db / 20.0);      // pow(10, -inf) = 0
    c.up = 1.0f / (float)g.attack;
    c.down = 1.0f / (float)g.release;
    hipLaunchKernelGGL(stream_gate_kernel, dim3((unsigned)S), dim3(256), 0, s, x, (long)n, (long)base, shift, y, out, g, c);
    return launch_check(ctx, "stream_gate");
}

}  // namespace tvc
