// The loudness envelope match (extension; tvc_loudness_match_f32 and tvc_stream_loudness_f32): the converted signal y is multiplied by a
// gain that moves the envelope of its power toward that of the input x it was converted from, by the share e a row or a stream asks for.
// The definition is in tinyvc_hip.h.  Both forms are built from the three device functions below - the power of a sub-frame (one wavefront
// per sub-frame, fp64), the gain from two window sums (fp64, one lane per sub-frame edge) and the gate's per-sample ramp (fp32, every
// operation rounded on its own) - so wherever the two forms see the same window they give the same bits.  The samples are streamed (two
// reads, one write); only the powers and the edge gains sit in LDS.
#include <algorithm>
#include <cmath>

#include "tvc_common.h"

namespace tvc {

// The one place that says which geometries the two kernels take (tvc_loudness_geometry / tvc_stream_loudness_geometry and through them
// the two device entries).  0, or TVC_ERR_ARG with the reason in `why` (nullable):
//   4 <= sub <= 65536, sub % 4 == 0                        whole quads of samples: a 16-byte access never straddles a sub-frame
//   1 <= length <= 2^40, length % sub == 0                 whole sub-frames
//   0 <= smooth <= 32                                      window = 2 * smooth + 1 sub-frames
//   stream_block: length / sub <= 4096                     a stream block
int loudness_geometry(int64_t length, int sub, int smooth, bool stream_block, int64_t* nsub, int* window, int* tile, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, long v, long w) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v, w);
        return (int)TVC_ERR_ARG;
    };
    if (sub < 4 || sub > kLoudnessMaxSubFrame) return refuse("sub = %ld is outside 4 .. %ld", sub, kLoudnessMaxSubFrame);
    if (sub % 4) return refuse("sub = %ld is not a multiple of 4", sub, 0);
    if (length < 1 || length > kLoudnessMaxLength) return refuse("length = %ld is outside 1 .. %ld", (long)length, (long)kLoudnessMaxLength);
    if (length % sub) return refuse("length = %ld is not a whole number of %ld-sample sub-frames", (long)length, sub);
    if (smooth < 0 || smooth > kLoudnessMaxSmooth) return refuse("smooth = %ld is outside 0 .. %ld", smooth, kLoudnessMaxSmooth);
    if (stream_block && length / sub > kLoudnessMaxBlockSub)
        return refuse("block / sub = %ld sub-frames is above %ld", (long)(length / sub), kLoudnessMaxBlockSub);
    if (why && why_bytes) why[0] = 0;
    if (nsub) *nsub = length / sub;
    if (window) *window = 2 * smooth + 1;
    if (tile) *tile = kLoudnessTile;
    return 0;
}

// The host's share of the definition, as fp64 kernel arguments.  0, or TVC_ERR_ARG with the reason in `why`.
int loudness_constants(float floor_db, float boost_db, float cut_db, LoudnessConst* c, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, double v) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v);
        return (int)TVC_ERR_ARG;
    };
    if (!std::isfinite(floor_db)) return refuse("floor_db = %g is not finite", (double)floor_db);
    if (!(boost_db >= 0.f) || std::isinf(boost_db)) return refuse("boost_db = %g is not a finite number >= 0", (double)boost_db);
    if (!(cut_db >= 0.f) || std::isinf(cut_db)) return refuse("cut_db = %g is not a finite number >= 0", (double)cut_db);
    LoudnessConst k;
    k.floor = std::pow(10.0, (double)floor_db / 10.0);
    k.hi = std::pow(10.0, (double)boost_db / 20.0);
    k.lo = std::pow(10.0, -(double)cut_db / 20.0);
    if (!(k.floor > 0.0) || !std::isfinite(k.floor)) return refuse("floor_db = %g: 10^(floor_db / 10) is not a positive finite double", (double)floor_db);
    if (!std::isfinite((float)k.hi)) return refuse("boost_db = %g: 10^(boost_db / 20) is not a finite fp32 number", (double)boost_db);
    if (!((float)k.lo > 0.f)) return refuse("cut_db = %g: 10^(-cut_db / 20) is not a positive fp32 number", (double)cut_db);
    if (why && why_bytes) why[0] = 0;
    *c = k;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- shared device functions

// The mean power of one sub-frame, by one wavefront: quad(q) gives samples 4q .. 4q + 3 of the sub-frame.  Lane l squares quads l, l + 64,
// ... in order (an fp32 square is exact in fp64), then a butterfly: every lane returns the same bits, and both forms the same bits for the
// same samples.
template <class Quad>
static __device__ __forceinline__ double subframe_power(Quad quad, int sub, int lane) {
    double acc = 0.;
    for (int q = lane; q < sub / 4; q += 64) {
        const float4 v = quad(q);
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc / (double)sub;
}

// the share a row or a stream asks for, as the kernel reads it: clamped to [0, 1], NaN is 0
static __device__ __forceinline__ double loudness_share(const float* share, long i) {
    const float e = share[i];
    return e > 0.f ? (e < 1.f ? (double)e : 1.) : 0.;
}

// The gain of a sub-frame from the two sums over its window of `cnt` sub-frame powers: one lane per sub-frame edge.  A NaN or infinite
// power in either window makes its sum NaN or infinite (powers are >= 0: nothing cancels) and the gain exactly 1.
static __device__ __forceinline__ float loudness_gain(double sum_s, double sum_o, int cnt, double e, const LoudnessConst& c) {
    if (e == 0. || !isfinite(sum_s) || !isfinite(sum_o)) return 1.f;
    const double es = sum_s / (double)cnt, eo = sum_o / (double)cnt;
    const double q = fmax(es, c.floor) / fmax(eo, c.floor);
    const double r = exp2(0.5 * e * log2(q));
    return (float)fmin(fmax(r, c.lo), c.hi);
}

// gate.hip's ramp on four samples j .. j + 3 of a sub-frame between the edge gains g0 and g1; g0 == g1: the multiplier is g0 exactly
static __device__ __forceinline__ float4 loudness_ramp(float4 v, float g0, float g1, int j, float fsub) {
    const float d = __fsub_rn(g1, g0);
    v.x = __fmul_rn(v.x, __fadd_rn(g0, __fmul_rn(d, __fdiv_rn((float)(j + 1), fsub))));
    v.y = __fmul_rn(v.y, __fadd_rn(g0, __fmul_rn(d, __fdiv_rn((float)(j + 2), fsub))));
    v.z = __fmul_rn(v.z, __fadd_rn(g0, __fmul_rn(d, __fdiv_rn((float)(j + 3), fsub))));
    v.w = __fmul_rn(v.w, __fadd_rn(g0, __fmul_rn(d, __fdiv_rn((float)(j + 4), fsub))));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------- offline

// x, y, out [B][L].  Workgroup (row b, group g) walks tiles [g * span, (g + 1) * span) of the row in order; tile t owns sub-frames
// [t * tile, (t + 1) * tile).  Per tile: 1. ps / po [i], i < tile + 1 + 2 * smooth: the powers of sub-frames t * tile - 1 - smooth + i inside
// the row (one wave per sub-frame);  2. lane i <= tile: the gain of sub-frame max(t * tile - 1 + i, 0) into gs[i] - gs[0] is the gain at the
// tile's first edge, and the row's first sub-frame is flat at its own gain;  3. all lanes apply the ramp.
// out != y: span = 1, the grid is rows x tiles and every workgroup recomputes its halo.  out == y: a tile's halo lies in its neighbours'
// tiles, which another workgroup would be scaling in place while this one reads them - so one workgroup walks the whole row (span = tiles)
// and carries the 2 * smooth + 1 powers the next tile shares with this one in LDS, taken before the ramp reached them: the powers, and with
// them every bit of the result, are those of the out != y call.
// A launch takes rows [row0, row0 + gridDim.x / groups); a ragged batch's lengths travel as kernel arguments (`lens`, this launch's rows:
// ragged.h's upload_ints scheme without the table in memory), so a call with lengths stays asynchronous and capturable.
static __global__ __launch_bounds__(256) void loudness_match_kernel(const float* x, const float* y, float* out, long L, long tiles, long span, long row0,
                                                                    LoudnessLens lens, int has_lens, const float* __restrict__ share, int sub, int smooth,
                                                                    LoudnessConst c, float* gains) {
    __shared__ double ps[kLoudnessTile + 1 + 2 * kLoudnessMaxSmooth];
    __shared__ double po[kLoudnessTile + 1 + 2 * kLoudnessMaxSmooth];
    __shared__ float gs[kLoudnessTile + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long groups = (tiles + span - 1) / span;
    const long r = (long)blockIdx.x / groups, b = row0 + r, t0 = ((long)blockIdx.x - r * groups) * span, t1 = min(t0 + span, tiles);
    const long nsub_l = L / sub;
    long len = has_lens ? (long)lens.v[r] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    const long nsub = len / sub;                    // the row's own sub-frames; samples behind nsub * sub are copied
    const float* xs = x + b * L;
    const float* ys = y + b * L;
    float* os = out + b * L;
    const double e = loudness_share(share, b);
    const float fsub = (float)sub;
    const int qsub = sub / 4, np = kLoudnessTile + 1 + 2 * smooth;
    const float4* yq = reinterpret_cast<const float4*>(ys);
    float4* oq = reinterpret_cast<float4*>(os);

    for (long t = t0; t < t1; ++t) {
        const long k0 = t * kLoudnessTile;              // the tile's first sub-frame
        const long kn = min(k0 + (long)kLoudnessTile, nsub_l);
        int carry = 0;
        if (t > t0) {      // the last 2 * smooth + 1 powers of the tile before are the first of this one (the ranges may overlap: read, then write)
            carry = 2 * smooth + 1;
            double a = 0., o = 0.;
            if (tid < carry) {
                a = ps[kLoudnessTile + tid];
                o = po[kLoudnessTile + tid];
            }
            __syncthreads();
            if (tid < carry) {
                ps[tid] = a;
                po[tid] = o;
            }
        }
        for (int i = carry + wave; i < np; i += 4) {
            const long k = k0 - 1 - smooth + i;
            double a = 0., o = 0.;
            if (k >= 0 && k < nsub) {      // (uniform over the wave)
                const float4* xk = reinterpret_cast<const float4*>(xs + k * sub);
                const float4* yk = reinterpret_cast<const float4*>(ys + k * sub);
                a = subframe_power([&](int q) { return xk[q]; }, sub, lane);
                o = subframe_power([&](int q) { return yk[q]; }, sub, lane);
            }
            if (lane == 0) {
                ps[i] = a;
                po[i] = o;
            }
        }
        __syncthreads();
        if (tid <= kLoudnessTile) {
            const long k = max(k0 - 1 + (long)tid, 0L);
            float g = 1.f;
            if (k < nsub) {
                const long lo = max(k - smooth, 0L), hi = min(k + smooth, nsub - 1);
                double ss = 0., so = 0.;
                for (long w = lo; w <= hi; ++w) {
                    const int i = (int)(w - (k0 - 1 - smooth));
                    ss += ps[i];
                    so += po[i];
                }
                g = loudness_gain(ss, so, (int)(hi - lo + 1), e, c);
            }
            gs[tid] = g;
            if (gains) {      // edge k + 1 belongs to sub-frame k's tile, edge 0 to the row's first; behind the row's length the gain is 1
                float* gr = gains + b * (nsub_l + 1);
                if (tid == 0 && t == 0) gr[0] = g;
                if (tid >= 1 && k0 + tid - 1 < kn) gr[k0 + tid] = g;
            }
        }
        __syncthreads();
        const long kw = os == ys ? min(kn, max(nsub, k0)) : kn;      // in place, the samples behind the row's length stay where they are
        const long q0 = k0 * qsub, q1 = kw * qsub;
        for (long q = q0 + tid; q < q1; q += 256) {
            const int f = (int)((q - q0) / qsub), j = (int)((q - q0) - (long)f * qsub) * 4;
            float4 v = yq[q];
            if (k0 + f < nsub) v = loudness_ramp(v, gs[f], gs[f + 1], j, fsub);
            oq[q] = v;
        }
        __syncthreads();      // gs, ps and po are free for the next tile
    }
}

// lengths: HOST, nullable.  One launch for up to kLoudnessLenRows rows, one more for every further kLoudnessLenRows of a larger batch.
int run_loudness_match(tvc_ctx* ctx, hipStream_t s, const float* x, const float* y, float* out, int B, int64_t L, const int64_t* lengths, const float* share,
                       int sub, int smooth, const LoudnessConst& c, float* gains) {
    const int64_t tiles = (L / sub + kLoudnessTile - 1) / kLoudnessTile;
    const int64_t span = out == y ? tiles : 1;      // (the caller has refused a partial overlap)
    const int64_t groups = (tiles + span - 1) / span;
    LoudnessLens lens = {};
    for (int row0 = 0; row0 < B; row0 += kLoudnessLenRows) {
        const int rows = std::min(B - row0, kLoudnessLenRows);
        if (lengths) std::memcpy(lens.v, lengths + row0, (size_t)rows * sizeof(int64_t));
        hipLaunchKernelGGL(loudness_match_kernel, dim3((unsigned)(groups * rows)), dim3(256), 0, s, x, y, out, (long)L, (long)tiles, (long)span, (long)row0, lens,
                           lengths ? 1 : 0, share, sub, smooth, c, gains);
    }
    return launch_check(ctx, "loudness_match");
}

// ---------------------------------------------------------------------------------------------------------------------------- streams

// x [S][n] input windows, y / out [S][block] (out may be y: a thread reads quad i of y before it writes quad i of out, and the powers of a
// chunk are taken before the barrier in front of its ramp).  One workgroup per stream walks the block in chunks of kLoudnessChunk
// sub-frames; a chunk is a block of its own - the result does not depend on how a stream is cut -, so the rings in device memory carry
// the window from chunk to chunk as they do from block to block.  Per chunk: 1. ps / po [i]: one wave per sub-frame (x at base + shift +
// ..., any alignment: four 4-byte loads, an index outside [0, n) reads 0);  2. lane i: the sums over the last min(seen + i + 1, W)
// sub-frames, oldest first - ring entries for the ones before the chunk - and the gain into gs[i + 1]; gs[0] is the carried edge gain, or
// the first sub-frame's own at the start of a stream;  3. the ramp, the readout and the chunk's last W powers into the rings.
static __global__ __launch_bounds__(256) void stream_loudness_kernel(const float* __restrict__ x, long n, long base, const int32_t* __restrict__ shift,
                                                                     const float* y, float* out, StreamLoudness g, LoudnessConst c, float* gains) {
    __shared__ double ps[kLoudnessChunk];
    __shared__ double po[kLoudnessChunk];
    __shared__ float gs[kLoudnessChunk + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long st = blockIdx.x;
    const int sub = g.sub, nsub = g.block / sub, W = 2 * g.smooth + 1, qsub = sub / 4;
    const float* xs = x + st * n;
    const float* ys = y + st * g.block;
    float* os = out + st * g.block;
    double* rs = g.src_ring + st * W;
    double* ro = g.out_ring + st * W;
    const long a = base + (shift ? (long)shift[st] : 0L);
    const double e = loudness_share(g.share, st);
    const float fsub = (float)sub;
    long seen = g.frames[st];      // every lane reads the carried state here; lane 0 writes it behind the last chunk's barriers
    seen = seen < 0 ? 0 : seen;
    float prev = g.gain[st];

    for (int c0 = 0; c0 < nsub; c0 += kLoudnessChunk) {
        const int m = min(kLoudnessChunk, nsub - c0);
        for (int i = wave; i < m; i += 4) {
            const long a0 = a + (long)(c0 + i) * sub;
            const float4* yq = reinterpret_cast<const float4*>(ys + (long)(c0 + i) * sub);
            auto xq = [&](int q) {
                const long i0 = a0 + 4 * (long)q;
                float4 v;
                v.x = i0 >= 0 && i0 < n ? xs[i0] : 0.f;
                v.y = i0 + 1 >= 0 && i0 + 1 < n ? xs[i0 + 1] : 0.f;
                v.z = i0 + 2 >= 0 && i0 + 2 < n ? xs[i0 + 2] : 0.f;
                v.w = i0 + 3 >= 0 && i0 + 3 < n ? xs[i0 + 3] : 0.f;
                return v;
            };
            const double p = subframe_power(xq, sub, lane);
            const double o = subframe_power([&](int q) { return yq[q]; }, sub, lane);
            if (lane == 0) {
                ps[i] = p;
                po[i] = o;
            }
        }
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const long have = seen + i + 1;      // sub-frames of the stream up to and including this one
            const int cnt = (int)min(have, (long)W);
            double ss = 0., so = 0.;
            for (int k = i - cnt + 1; k <= i; ++k) {      // k < 0: before the chunk, in the rings (seen + k >= 0 as cnt <= seen + i + 1)
                const int r = (int)((seen + k) % W);
                ss += k >= 0 ? ps[k] : rs[r];
                so += k >= 0 ? po[k] : ro[r];
            }
            const float gi = loudness_gain(ss, so, cnt, e, c);
            gs[i + 1] = gi;
            if (i == 0) gs[0] = seen == 0 ? gi : prev;
        }
        __syncthreads();      // the rings' old entries have been read: the chunk may overwrite them
        const float4* yq = reinterpret_cast<const float4*>(ys + (long)c0 * sub);
        float4* oq = reinterpret_cast<float4*>(os + (long)c0 * sub);
        for (int q = tid; q < m * qsub; q += 256) {
            const int f = q / qsub, j = (q - f * qsub) * 4;
            oq[q] = loudness_ramp(yq[q], gs[f], gs[f + 1], j, fsub);
        }
        for (int i = tid; i < m; i += 256) {
            if (i >= m - W) {
                const int r = (int)((seen + i) % W);
                rs[r] = ps[i];
                ro[r] = po[i];
            }
            if (gains) {
                float* gr = gains + st * (nsub + 1);
                gr[c0 + i + 1] = gs[i + 1];
                if (c0 + i == 0) gr[0] = gs[0];
            }
        }
        prev = gs[m];
        seen += m;
        __syncthreads();      // gs, ps and po are free for the next chunk, and its lanes see this chunk's ring entries
    }
    if (tid == 0) {
        g.frames[st] = seen;
        g.gain[st] = prev;
        if (g.gain_db) g.gain_db[st] = 20.f * log10f(prev);
    }
}

int run_stream_loudness(tvc_ctx* ctx, hipStream_t s, const float* x, int64_t n, int64_t base, const int32_t* shift, const float* y, float* out, int S,
                        const StreamLoudness& g, const LoudnessConst& c, float* gains) {
    hipLaunchKernelGGL(stream_loudness_kernel, dim3((unsigned)S), dim3(256), 0, s, x, (long)n, (long)base, shift, y, out, g, c, gains);
    return launch_check(ctx, "stream_loudness");
}

}  // namespace tvc
