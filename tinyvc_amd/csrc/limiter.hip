// The look-ahead peak limiter (extension; tvc_limit_f32 and tvc_stream_limit_f32): the last stage of a chain, which holds every sample at or
// below a ceiling c exactly.  The definition is in tinyvc_hip.h.  Both forms are built from the same device functions - the peak of a
// sub-frame (a max, so any reduction shape gives the same bits), the edge ratio r, one step of the recurrence e, and the gate's per-sample
// ramp followed by the clamp (fp32, every operation rounded on its own) - so a stream is the offline result delayed by one sub-frame, bit
// for bit.  The samples are streamed; only peaks and edge gains sit in LDS.
#include <algorithm>
#include <cmath>

#include "tvc_common.h"

namespace tvc {

// The one place that says which geometries the two kernels take (tvc_limiter_geometry / tvc_stream_limiter_geometry and through them the
// two device entries).  0, or TVC_ERR_ARG with the reason in `why` (nullable):
//   4 <= sub <= 65536, sub % 4 == 0                        whole quads of samples: a 16-byte access never straddles a sub-frame
//   offline: 1 <= length <= 2^40, length % sub == 0        whole sub-frames
//   stream_block: sub <= length <= 2^30, length % sub == 0 a stream's block, at least one sub-frame
//   1 <= release <= 4096                                   sub-frames a gain of 0 takes back to 1
int limiter_geometry(int64_t length, int sub, int release, bool stream_block, int64_t* nsub, int* delay, int* tile, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, long v, long w) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v, w);
        return (int)TVC_ERR_ARG;
    };
    if (sub < 4 || sub > kLimiterMaxSubFrame) return refuse("sub = %ld is outside 4 .. %ld", sub, kLimiterMaxSubFrame);
    if (sub % 4) return refuse("sub = %ld is not a multiple of 4", sub, 0);
    if (stream_block) {
        if (length < sub || length > kLimiterMaxBlock) return refuse("block = %ld is outside one sub-frame .. %ld", (long)length, kLimiterMaxBlock);
        if (length % sub) return refuse("block = %ld is not a whole number of %ld-sample sub-frames", (long)length, sub);
    } else {
        if (length < 1 || length > kLimiterMaxLength) return refuse("length = %ld is outside 1 .. %ld", (long)length, (long)kLimiterMaxLength);
        if (length % sub) return refuse("length = %ld is not a whole number of %ld-sample sub-frames", (long)length, sub);
    }
    if (release < 1 || release > kLimiterMaxRelease) return refuse("release = %ld is outside 1 .. %ld sub-frames", release, kLimiterMaxRelease);
    if (why && why_bytes) why[0] = 0;
    if (nsub) *nsub = length / sub;
    if (delay) *delay = sub;
    if (tile) *tile = stream_block ? kLimiterChunk : kLimiterTile;
    return 0;
}

// The host's share of the definition: drive = (float)10^(drive_db / 20), made in double and rounded once.  0, or TVC_ERR_ARG with the reason.
int limiter_drive(float drive_db, float* drive, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, double v) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v);
        return (int)TVC_ERR_ARG;
    };
    if (!std::isfinite(drive_db)) return refuse("drive_db = %g is not finite", (double)drive_db);
    const float f = (float)std::pow(10.0, (double)drive_db / 20.0);
    if (!(f > 0.f) || !std::isfinite(f)) return refuse("drive_db = %g: 10^(drive_db / 20) is not a positive finite fp32 number", (double)drive_db);
    if (why && why_bytes) why[0] = 0;
    *drive = f;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- shared device functions

// the ceiling a row or a stream asks for, as the kernel reads it: NaN, <= 0 and +inf are off (+inf)
static __device__ __forceinline__ float limiter_ceiling(const float* ceiling, long i) {
    const float c = ceiling[i];
    return c > 0.f ? c : INFINITY;
}

// max |v| of four driven samples; a NaN sample is ignored (fmaxf returns the other operand).  The result is >= +0, so its bit pattern
// orders like the value and an integer max in LDS reduces a sub-frame whatever the lanes that hold its quads.
static __device__ __forceinline__ unsigned quad_peak(float4 v) {
    float m = fmaxf(0.f, fabsf(v.x));
    m = fmaxf(m, fabsf(v.y));
    m = fmaxf(m, fabsf(v.z));
    m = fmaxf(m, fabsf(v.w));
    return __float_as_uint(m);
}

static __device__ __forceinline__ float4 limiter_drive4(float4 v, float drive) {
    v.x = __fmul_rn(v.x, drive);
    v.y = __fmul_rn(v.y, drive);
    v.z = __fmul_rn(v.z, drive);
    v.w = __fmul_rn(v.w, drive);
    return v;
}

// r at an edge between sub-frames of peaks p0 and p1
static __device__ __forceinline__ float limiter_ratio(float p0, float p1, float c) {
    const float m = fmaxf(p0, p1);
    return m > c ? __fdiv_rn(c, m) : 1.f;
}

// one step of the recurrence: instant fall, linear rise
static __device__ __forceinline__ float limiter_step(float e, float r, float d) { return fminf(r, fminf(1.f, __fadd_rn(e, d))); }

static __device__ __forceinline__ float limiter_clamp(float t, float c) { return t > c ? c : (t < -c ? -c : t); }

// the gate's ramp on four driven samples j .. j + 3 of a sub-frame between the edge gains e0 and e1, then the clamp
static __device__ __forceinline__ float4 limiter_ramp(float4 v, float e0, float e1, int j, float fsub, float c) {
    const float d = __fsub_rn(e1, e0);
    v.x = limiter_clamp(__fmul_rn(v.x, __fadd_rn(e0, __fmul_rn(d, __fdiv_rn((float)(j + 1), fsub)))), c);
    v.y = limiter_clamp(__fmul_rn(v.y, __fadd_rn(e0, __fmul_rn(d, __fdiv_rn((float)(j + 2), fsub)))), c);
    v.z = limiter_clamp(__fmul_rn(v.z, __fadd_rn(e0, __fmul_rn(d, __fdiv_rn((float)(j + 3), fsub)))), c);
    v.w = limiter_clamp(__fmul_rn(v.w, __fadd_rn(e0, __fmul_rn(d, __fdiv_rn((float)(j + 4), fsub)))), c);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------- offline

// y, out [B][L], apart.  Workgroup (row b, tile t) owns sub-frames [k0, k0 + T), k0 = t * T, and so the edges k0 .. k0 + T.  Dynamic LDS:
// one array of T + R + 3 words.
//   1. peaks: pk[i] = p[k0 - R - 2 + i]: the tile's sub-frames, the R + 2 before and the one after; 0 outside the row's own sub-frames.  A
//      thread takes a quad and folds it in with an integer max.
//   2. ratios, in place: pk[i] <- r[k0 - R - 1 + i] from pk[i] and pk[i + 1], i < T + R + 2 (read, barrier, write).
//   3. the recurrence: thread `tid` owns kLimiterEdges consecutive edges of the tile and starts from e = 1 at R + 1 edges before them (or at
//      edge 0): after R + 1 steps the recurrence has forgotten where it started, so these are the row's exact gains.  They wait in registers
//      until every thread has read its ratios, then go to pk[0 .. T].
//   4. the ramp and the clamp on the tile's samples; samples behind the row's length are copied.
static __global__ __launch_bounds__(256) void limit_kernel(const float* __restrict__ y, float* __restrict__ out, long L, long tiles, long row0, LoudnessLens lens,
                                                           int has_lens, const float* __restrict__ ceiling, int sub, int R, float d, float drive,
                                                           float* __restrict__ gains) {
    extern __shared__ float pk[];
    unsigned* pku = reinterpret_cast<unsigned*>(pk);
    constexpr int T = kLimiterTile;
    const int tid = threadIdx.x;
    const long r = (long)blockIdx.x / tiles, b = row0 + r, t = (long)blockIdx.x - r * tiles;
    const long nsub_l = L / sub;
    long len = has_lens ? (long)lens.v[r] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    const long nsub = len / sub;                    // the row's own sub-frames; samples behind nsub * sub are copied
    const long k0 = t * T, kn = min(k0 + (long)T, nsub_l);
    const float c = limiter_ceiling(ceiling, b);
    const float fsub = (float)sub;
    const int qsub = sub / 4, np = T + R + 3;
    const float4* yq = reinterpret_cast<const float4*>(y + b * L);
    float4* oq = reinterpret_cast<float4*>(out + b * L);

    if (k0 <= nsub) {      // (uniform over the workgroup) a tile behind the row's last edge only copies
        for (int i = tid; i < np; i += 256) pku[i] = 0u;
        __syncthreads();
        const long ka = max(k0 - R - 2, 0L), kb = min(k0 + (long)T + 1, nsub);      // the sub-frames whose peaks are not 0
        for (long q = ka * qsub + tid; q < kb * qsub; q += 256) {
            const long k = q / qsub;
            atomicMax(&pku[(int)(k - (k0 - R - 2))], quad_peak(limiter_drive4(yq[q], drive)));
        }
        __syncthreads();
        constexpr int kPer = (T + 4099 + 2 + 255) / 256;      // ratios a thread holds between the two barriers
        float rr[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int i = tid + u * 256;
            rr[u] = i < np - 1 ? limiter_ratio(pk[i], pk[i + 1], c) : 1.f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int i = tid + u * 256;
            if (i < np - 1) pk[i] = rr[u];
        }
        __syncthreads();
        // pk[i] = r at edge k0 - R - 1 + i; edge k0 + w sits at R + 1 + w
        float ev[kLimiterEdges];
        const int w0 = tid * kLimiterEdges;
        if (w0 <= T) {
            float e = 1.f;
            const int first = (int)max((long)w0, (long)(R + 1) - k0);      // R + 1 edges back, or edge 0
            for (int i = first; i < R + 1 + w0; ++i) e = limiter_step(e, pk[i], d);
#pragma unroll
            for (int u = 0; u < kLimiterEdges; ++u) {
                if (w0 + u <= T) e = limiter_step(e, pk[R + 1 + w0 + u], d);
                ev[u] = e;
            }
        }
        __syncthreads();
        if (w0 <= T) {
#pragma unroll
            for (int u = 0; u < kLimiterEdges; ++u)
                if (w0 + u <= T) pk[w0 + u] = k0 + w0 + u <= nsub ? ev[u] : 1.f;      // behind the row's length the gain is 1
        }
        __syncthreads();
    }
    if (gains) {      // edge k0 + w, w < T, belongs to this tile; the row's last edge to its last tile
        float* gr = gains + b * (nsub_l + 1);
        for (int w = tid; w <= T; w += 256)
            if (k0 + w <= nsub_l && (w < T || k0 + T == nsub_l)) gr[k0 + w] = k0 <= nsub ? pk[w] : 1.f;
    }
    const long q0 = k0 * qsub, q1 = kn * qsub;
    for (long q = q0 + tid; q < q1; q += 256) {
        const int f = (int)((q - q0) / qsub), j = (int)((q - q0) - (long)f * qsub) * 4;
        float4 v = yq[q];
        if (k0 + f < nsub) v = limiter_ramp(limiter_drive4(v, drive), pk[f], pk[f + 1], j, fsub, c);
        oq[q] = v;
    }
    // the samples behind the last whole sub-frame of L do not exist: L is whole sub-frames
}

// lengths: HOST, nullable.  One launch for up to kLoudnessLenRows rows, one more for every further kLoudnessLenRows of a larger batch.
int run_limit(tvc_ctx* ctx, hipStream_t s, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* ceiling, int sub, int release,
              float drive, float* gains) {
    const int64_t tiles = (L / sub + kLimiterTile - 1) / kLimiterTile;
    const float d = 1.0f / (float)release;
    const size_t lds = (size_t)(kLimiterTile + release + 3) * sizeof(float);
    LoudnessLens lens = {};
    for (int row0 = 0; row0 < B; row0 += kLoudnessLenRows) {
        const int rows = std::min(B - row0, kLoudnessLenRows);
        if (lengths) std::memcpy(lens.v, lengths + row0, (size_t)rows * sizeof(int64_t));
        hipLaunchKernelGGL(limit_kernel, dim3((unsigned)(tiles * rows)), dim3(256), lds, s, y, out, (long)L, (long)tiles, (long)row0, lens, lengths ? 1 : 0, ceiling,
                           sub, release, d, drive, gains);
    }
    return launch_check(ctx, "limit");
}

// ---------------------------------------------------------------------------------------------------------------------------- streams

// y, out [S][block], apart.  One workgroup per stream walks the block in chunks of kLimiterChunk sub-frames; a chunk is a block of its own.
// The stream carries the one sub-frame it could not emit yet: its driven samples (tail), its peak and e at its start.  Per chunk of m
// sub-frames: 1. pk[0] = the carried peak, pk[1 + i] = the peak of the chunk's sub-frame i;  2. eg[1 + i] = r at the edge in front of
// sub-frame i;  3. lane 0 runs the recurrence from eg[0] = the carried gain;  4. output sub-frame i is the sub-frame before the chunk's
// sub-frame i - the tail, or y - between eg[i] and eg[i + 1].  Then the block's last sub-frame becomes the tail.
static __global__ __launch_bounds__(256) void stream_limit_kernel(const float* __restrict__ y, float* __restrict__ out, StreamLimiter g, float d, float drive,
                                                                  float* __restrict__ gains) {
    __shared__ float pk[kLimiterChunk + 1];
    __shared__ float eg[kLimiterChunk + 1];
    unsigned* pku = reinterpret_cast<unsigned*>(pk);
    const int tid = threadIdx.x;
    const long st = blockIdx.x;
    const int sub = g.sub, nsub = g.block / sub, qsub = sub / 4;
    const float4* yq = reinterpret_cast<const float4*>(y + st * g.block);
    float4* oq = reinterpret_cast<float4*>(out + st * g.block);
    float4* tq = reinterpret_cast<float4*>(g.tail + st * sub);
    const float c = limiter_ceiling(g.ceiling, st);
    const float fsub = (float)sub;
    float peak = g.peak[st], gain = g.gain[st];      // every lane reads the carried state here; lane 0 writes it behind the last chunk's barriers
    float least = gain;

    for (int c0 = 0; c0 < nsub; c0 += kLimiterChunk) {
        const int m = min(kLimiterChunk, nsub - c0);
        for (int i = tid; i <= m; i += 256) pku[i] = i == 0 ? __float_as_uint(fmaxf(0.f, peak)) : 0u;
        __syncthreads();
        for (int q = tid; q < m * qsub; q += 256) atomicMax(&pku[1 + q / qsub], quad_peak(limiter_drive4(yq[(long)c0 * qsub + q], drive)));
        __syncthreads();
        for (int i = tid; i < m; i += 256) eg[1 + i] = limiter_ratio(pk[i], pk[i + 1], c);
        __syncthreads();
        if (tid == 0) {
            float e = gain;
            eg[0] = e;
            for (int i = 1; i <= m; ++i) {
                e = limiter_step(e, eg[i], d);
                eg[i] = e;
                least = fminf(least, e);
            }
        }
        __syncthreads();
        for (int q = tid; q < m * qsub; q += 256) {
            const int f = q / qsub, j = (q - f * qsub) * 4;
            const long src = (long)(c0 + f - 1) * qsub + (q - f * qsub);      // the sub-frame before, in y; the tail in front of the block
            const float4 v = src < 0 ? tq[q] : limiter_drive4(yq[src], drive);
            oq[(long)c0 * qsub + q] = limiter_ramp(v, eg[f], eg[f + 1], j, fsub, c);
        }
        if (gains) {
            float* gr = gains + st * (nsub + 1);
            for (int i = tid; i <= m; i += 256)
                if (i > 0 || c0 == 0) gr[c0 + i] = eg[i];
        }
        peak = pk[m];
        gain = eg[m];
        __syncthreads();      // pk and eg are free for the next chunk; the tail has been read
    }
    for (int q = tid; q < qsub; q += 256) tq[q] = limiter_drive4(yq[(long)(nsub - 1) * qsub + q], drive);
    if (tid == 0) {
        g.peak[st] = peak;
        g.gain[st] = gain;
        if (g.reduction_db) g.reduction_db[st] = 20.f * log10f(least);
    }
}

int run_stream_limit(tvc_ctx* ctx, hipStream_t s, const float* y, float* out, int S, const StreamLimiter& g, int release, float drive, float* gains) {
    hipLaunchKernelGGL(stream_limit_kernel, dim3((unsigned)S), dim3(256), 0, s, y, out, g, 1.0f / (float)release, drive, gains);
    return launch_check(ctx, "stream_limit");
}

}  // namespace tvc
