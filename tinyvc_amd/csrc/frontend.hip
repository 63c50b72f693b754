// Front end: |STFT| (spectrogram.py:8-15), energy envelope (energy_estimation.py:9-14),
// semitone shift (pitch_shift.py:5-15), the row-wise pitch register and the automatic shift onto a target's (no reference counterpart).
#include "small_kernels.h"
#include "tvc_common.h"

namespace tvc {

// |STFT| (spectrogram.py:8-15): one wavefront per 1920-sample frame, a 960-point complex FFT on the packed real frame
// (fft.hip).  Needs no scratch.
int run_stft(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* wav, float* spec, int B, int64_t L) {
    return ws.dry ? 0 : run_stft_fft(ctx, s, wav, spec, B, L);
}

// ---- energy -------------------------------------------------------------------------------------
// e[j] = max |x[64 j - 32 .. 64 j + 95]| (max_pool1d(|x|, 128, 64, 32): out-of-range = -inf)
static __global__ void energy_pool_kernel(const float* __restrict__ wav, float* __restrict__ e, int B, int L, int ne) {
    long total = (long)B * ne;
    const int lane = threadIdx.x & 63;
    long wave = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long i = wave; i < total; i += nwaves) {
        int b = (int)(i / ne), j = (int)(i - (long)b * ne);
        const float* x = wav + (long)b * L;
        int lo = 64 * j - 32;
        float m = -INFINITY;
        for (int k = lane; k < 128; k += 64) {
            int p = lo + k;
            if (p >= 0 && p < L) m = fmaxf(m, fabsf(x[p]));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) e[i] = m;
    }
}

// ragged batch (ragged.h): utterance b = blockIdx.y pools its own row of the caller's padded tensor over its own length into
// e[eoff(b) ...] (eoff(b) = floor(7.5 pre[b]): the pooled lengths floor(7.5 tb) of the utterances before it fit in front), then
// F.interpolate(e_b, L_b) lands at samples pre[b] * 480 ... of the batch-wide energy row
static __global__ __launch_bounds__(256) void energy_rag_kernel(const float* __restrict__ wav, float* __restrict__ e, float* __restrict__ energy, RagDev rg, int phase) {
    const int b = blockIdx.y;
    const int T = rg.tb[b], L = T * kHop, ne = (L + 2 * 32 - 128) / 64 + 1;
    float* eb = e + (15L * rg.pre[b]) / 2;
    if (phase == 0) {
        const float* x = wav + (long)rg.row[b] * rg.Tmax * kHop;
        const int lane = threadIdx.x & 63;
        const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
        for (int j = wave; j < ne; j += nwaves) {
            const int lo = 64 * j - 32;
            float m = -INFINITY;
            for (int k = lane; k < 128; k += 64) {
                const int p = lo + k;
                if (p >= 0 && p < L) m = fmaxf(m, fabsf(x[p]));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0) eb[j] = m;
        }
    } else {
        const float scale = __fdiv_rn((float)ne, (float)L);      // F.interpolate(e, L): `size` given -> scale = float(in) / float(out)
        float* y = energy + (long)rg.pre[b] * kHop;
        for (int d = blockIdx.x * blockDim.x + threadIdx.x; d < L; d += gridDim.x * blockDim.x) {
            const Lerp c = lerp_coord(d, scale, ne);
            y[d] = lerp_eval(c, eb[c.i0], eb[c.i1]);
        }
    }
}

// out[b] = a * in[b * in_stride] + c: the |max| slot of a tensor from the slot of the tensor it is a bounded function of (in_stride = 0:
// one value for every utterance).  One 64-thread workgroup; NaN / Inf carry through (bfp_from_amax ignores them).
static __global__ void slot_affine_kernel(float* __restrict__ out, const float* __restrict__ in, int in_stride, float a, float c, int n) {
    for (int b = threadIdx.x; b < n; b += blockDim.x) out[b] = fmaf(a, in[(long)b * in_stride], c);
}
int run_slot_affine(tvc_ctx* ctx, hipStream_t s, float* out, const float* in, int in_stride, float a, float c, int n) {
    hipLaunchKernelGGL(slot_affine_kernel, dim3(1), dim3(64), 0, s, out, in, in_stride, a, c, n);
    return launch_check(ctx, "slot_affine");
}
// The decoder's slots in one launch: zero[0 .. nz) = 0 (the slots its kernels raise with atomicMax), then the two bounds it is handed:
// o1[b] = a1 in1[b * s1] + c1, o2[b] = a2 in2[b * s2] + c2 (either pair may be null), and o3[b] = a3 o1[b] + c3 (a bound of a bounded function
// of the first tensor; null without o1).  One workgroup.
static __global__ void slot_prep_kernel(float* __restrict__ zero, int nz, float* __restrict__ o1, const float* __restrict__ in1, int s1, float a1, float c1,
                                        float* __restrict__ o2, const float* __restrict__ in2, int s2, float a2, float c2, float* __restrict__ o3, float a3,
                                        float c3, int n) {
    for (int i = threadIdx.x; i < nz; i += blockDim.x) zero[i] = 0.f;
    __syncthreads();      // (the bounds' slots lie inside the zeroed block)
    for (int b = threadIdx.x; b < n; b += blockDim.x) {
        if (o1) {
            const float v1 = fmaf(a1, in1[(long)b * s1], c1);
            o1[b] = v1;
            if (o3) o3[b] = fmaf(a3, v1, c3);
        }
        if (o2) o2[b] = fmaf(a2, in2[(long)b * s2], c2);
    }
}
int run_slot_prep(tvc_ctx* ctx, hipStream_t s, float* zero, int nz, float* o1, const float* in1, int s1, float a1, float c1, float* o2, const float* in2, int s2,
                  float a2, float c2, float* o3, float a3, float c3, int n) {
    hipLaunchKernelGGL(slot_prep_kernel, dim3(1), dim3(256), 0, s, zero, nz, o1, in1, s1, a1, c1, o2, in2, s2, a2, c2, o3, a3, c3, n);
    return launch_check(ctx, "slot_prep");
}
// emax[b] = max_j e[b][j] (one workgroup per utterance: 1 500 values); spec_bound[b] = 960.5 emax[b] >= every |STFT| bin (the Hann window's sum)
// zero[0 .. nz) = 0: the encoder's atomicMax slots, zeroed here instead of by a memset of their own
static __global__ __launch_bounds__(256) void pooled_max_kernel(const float* __restrict__ e, int ne, float* __restrict__ emax, float* __restrict__ spec_bound, float* __restrict__ zero, int nz) {
    __shared__ float red[4];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nz; i += gridDim.x * 256) zero[i] = 0.f;
    const float* p = e + (long)blockIdx.x * ne;
    float m = 0.f;
    for (int j = threadIdx.x; j < ne; j += 256) m = fmaxf(m, p[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        emax[blockIdx.x] = m;
        if (spec_bound) spec_bound[blockIdx.x] = fmaf(960.5f, m, 0.f);
    }
}

// the same for a ragged batch: utterance b = blockIdx.x pools ITS floor(7.5 tb) + 1 values (energy_rag_kernel's layout) - the bound its own B = 1 call computes
static __global__ __launch_bounds__(256) void pooled_max_rag_kernel(const float* __restrict__ e, RagDev rg, float* __restrict__ emax, float* __restrict__ spec_bound, float* __restrict__ zero, int nz) {
    __shared__ float red[4];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nz; i += gridDim.x * 256) zero[i] = 0.f;
    const int b = blockIdx.x;
    const int L = rg.tb[b] * kHop, ne = (L + 2 * 32 - 128) / 64 + 1;
    const float* p = e + (15L * rg.pre[b]) / 2;
    float m = 0.f;
    for (int j = threadIdx.x; j < ne; j += 256) m = fmaxf(m, p[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        emax[b] = m;
        if (spec_bound) spec_bound[b] = fmaf(960.5f, m, 0.f);
    }
}

int run_energy(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* wav, float* energy, int B, int64_t L, float* emax, float* spec_bound, float* zero, int nz) {
    const int ne = (int)((L + 2 * 32 - 128) / 64 + 1);
    float* e = ws.get<float>((size_t)B * ne + 8);
    if (ws.dry) return 0;
    if (ctx->rag) {
        RagDev rg;
        TVC_CHECK(rag_view(ctx, s, kHop, 0, &rg, nullptr));
        const int gx = ctx->rag->B >= 32 ? 8 : 64;
        hipLaunchKernelGGL(energy_rag_kernel, dim3(gx, ctx->rag->B), dim3(256), 0, s, wav, e, energy, rg, 0);
        if (emax) hipLaunchKernelGGL(pooled_max_rag_kernel, dim3(ctx->rag->B), dim3(256), 0, s, e, rg, emax, spec_bound, zero, nz);
        hipLaunchKernelGGL(energy_rag_kernel, dim3(gx * 4, ctx->rag->B), dim3(256), 0, s, wav, e, energy, rg, 1);
        return launch_check(ctx, "energy (ragged)");
    }
    hipLaunchKernelGGL(energy_pool_kernel, dim3(grid_for((long)B * ne * 64)), dim3(256), 0, s, wav, e, B, (int)L, ne);
    if (emax) hipLaunchKernelGGL(pooled_max_kernel, dim3(B), dim3(256), 0, s, e, ne, emax, spec_bound, zero, nz);
    // F.interpolate(e, L): `size` given -> scale = float(in) / float(out)
    float scale = (float)ne / (float)L;
    {
        const LerpLaunch ll = lerp_launch((long)B, (int)L);
        hipLaunchKernelGGL(lerp_resize_kernel, ll.grid, dim3(256), 0, s, e, energy, (long)B, ne, (int)L, scale, ll.tx);
    }
    return launch_check(ctx, "energy");
}

// ---- shift_frequency ----------------------------------------------------------------------------
// midi = log2(relu(f/440) + 1e-6) * 12 + 69 + shift;  f' = 440 * 2^((midi - 69) / 12)
// Every step is the fp32 op ATen runs, in ATen's order.  The two transcendentals are evaluated in fp64 and rounded
// once: ATen's CPU log2 / pow (Sleef u10) return the correctly rounded fp32 value on ~99 % of inputs and differ by one
// ulp otherwise, whereas two different <= 1 ulp approximations disagree on a large fraction - and one ulp of `midi`
// is 2.2e-7 of f0, which the harmonic oscillator integrates over the whole utterance (measured: 4.5e-5 of the 7.1e-5
// end-to-end rms difference at 4 s came from this function alone before the change).
static __global__ void shift_kernel(const float* __restrict__ f0, float* __restrict__ out, long n, float shift) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = shift_frequency_one(f0[i], shift);
}

// u in [0, 1) -> u * 2 * pi - pi with the reference expression's three fp32 roundings (decoder.py:78: `torch.rand(...) * 2 * math.pi - math.pi`
// is three tensor ops; u * 2 is exact), in place, four values per thread
static __global__ __launch_bounds__(256) void uniform_to_angle_kernel(float* __restrict__ u, int64_t n) {
    const int64_t i = 4 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
    const float pi = 3.1415927410125732f;          // float(math.pi)
    if (i + 3 < n && (reinterpret_cast<uintptr_t>(u) & 15) == 0) {
        float4 v = *reinterpret_cast<float4*>(u + i);
        v.x = __fsub_rn(__fmul_rn(__fmul_rn(v.x, 2.f), pi), pi);
        v.y = __fsub_rn(__fmul_rn(__fmul_rn(v.y, 2.f), pi), pi);
        v.z = __fsub_rn(__fmul_rn(__fmul_rn(v.z, 2.f), pi), pi);
        v.w = __fsub_rn(__fmul_rn(__fmul_rn(v.w, 2.f), pi), pi);
        *reinterpret_cast<float4*>(u + i) = v;
    } else {
        for (int64_t k = i; k < n && k < i + 4; ++k) u[k] = __fsub_rn(__fmul_rn(__fmul_rn(u[k], 2.f), pi), pi);
    }
}
int run_uniform_to_angle(tvc_ctx* ctx, hipStream_t s, float* u, int64_t n) {
    const int64_t groups = (n + 3) / 4;
    hipLaunchKernelGGL(uniform_to_angle_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, u, n);
    return launch_check(ctx, "uniform_to_angle");
}

int run_shift(tvc_ctx* ctx, hipStream_t s, const float* f0, float* out, int64_t n, float semitones) {
    hipLaunchKernelGGL(shift_kernel, dim3(grid_for(n)), dim3(256), 0, s, f0, out, (long)n, semitones);
    return launch_check(ctx, "shift_frequency");
}

// ---- pitch register and automatic shift ------------------------------------------------------------
// The register of a row of f0 = the LOWER median of its voiced frames, torch.median(row[row > 0]): the element of rank (nv - 1) / 2 among
// the nv values > 0 (zeros, negatives and NaN are unvoiced).  An order statistic: exact, no floating-point sum, independent of the grid.
// Positive floats order like their bit patterns, so it is a radix select over bits 30 .. 0 (the sign of a voiced value is 0): four passes
// over the digits [30:23] (the exponent), [22:15], [14:7], [6:0], each a histogram of the values that share the digits selected so far,
// then a scan that finds the digit holding the wanted rank.  One 256-thread workgroup per row; rows come as runs of columns (start,
// length) in the kernel's ARGUMENTS, like the offsets (host values of the call: asynchronous, capturable).
// f0 lives in 20 Hz .. a few kHz: a row's values share their top bits, the exponent pass meets 2 - 4 distinct digits and a pass over equal
// values one.  So every wave keeps its own histogram and first peels the two most advanced digits of its 64 values with a ballot (one add of
// the population count by the first lane that holds the digit); only what is left goes to the LDS atomics one by one.  Integer atomics
// on LDS only.
//   shift[b] = offset[b] + 12 log2(target[b] / median[b])   evaluated in fp64, rounded once (like shift_frequency_one's transcendentals);
//   shift[b] = offset[b] exactly when the row has no voiced frame, target[b] <= 0 or NaN, or there is no target (measuring only).
// The same workgroup then walks its row again: f0s[n] = shift_frequency_one(f0[n], shift[b]).  The median of a row without a voiced
// frame is reported as 0.
constexpr int kPmRows = 256;      // rows per launch: their descriptions are kernel arguments (3 KiB of the 4 KiB a launch may carry)
struct PitchRowChunk {
    int start[kPmRows], len[kPmRows], idx[kPmRows];      // columns [start, start + len) of f0; idx = the row's slot in target / the outputs
    float offset[kPmRows];
};

// The select itself, shared by pitch_match_kernel (a row in global memory) and pitch_track_kernel (a ring staged in LDS): the bit pattern of
// the lower median of the values > 0 among p[0 .. n), and their number in *nv_out (0: no voiced value, the result is 0).  Called by all
// 256 threads of the workgroup; the result is uniform over it.
struct PitchSelectLds {
    unsigned hist[4][256];
    unsigned wsum[4];
    unsigned sel_digit, sel_rank;
};
static __device__ __forceinline__ unsigned pitch_select(const float* __restrict__ p, long n, PitchSelectLds& lds, unsigned* nv_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0, rank = 0, nv = 0;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int lo = pass == 3 ? 0 : 23 - 8 * pass;            // 23, 15, 7, 0
        const int width = pass == 3 ? 7 : 8;
        for (int w = 0; w < 4; ++w) lds.hist[w][tid] = 0;
        __syncthreads();
        for (long base = 0; base < n; base += 256 * 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = base + u * 256 + tid;
                v[u] = i < n ? p[i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned bits = __float_as_uint(v[u]);
                bool live = v[u] > 0.f && (pass == 0 || (bits >> (lo + width)) == prefix);
                const unsigned digit = (bits >> lo) & ((1u << width) - 1u);
#pragma unroll
                for (int round = 0; round < 2; ++round) {
                    const unsigned long long act = __ballot(live);
                    if (!act) break;
                    const int first = __ffsll((long long)act) - 1;
                    const unsigned d0 = (unsigned)__shfl((int)digit, first);
                    const unsigned long long same = __ballot(live && digit == d0);
                    if (lane == first) atomicAdd(&lds.hist[wave][d0], (unsigned)__popcll(same));
                    if (digit == d0) live = false;
                }
                if (live) atomicAdd(&lds.hist[wave][digit], 1u);
            }
        }
        __syncthreads();
        // exclusive scan of the 256 bins (thread = bin): the bin that holds `rank`
        const unsigned c = lds.hist[0][tid] + lds.hist[1][tid] + lds.hist[2][tid] + lds.hist[3][tid];
        unsigned inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = (unsigned)__shfl_up((int)inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) lds.wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += lds.wsum[w];
            total += lds.wsum[w];
        }
        if (pass == 0) {
            nv = total;
            rank = nv ? (nv - 1) / 2 : 0;
        }
        if (total == 0) break;      // (pass 0 only: no voiced frame; uniform over the workgroup)
        const unsigned excl = before + inc - c;
        if (c && excl <= rank && rank < excl + c) {
            lds.sel_digit = (unsigned)tid;
            lds.sel_rank = rank - excl;
        }
        __syncthreads();
        prefix = (prefix << width) | lds.sel_digit;
        rank = lds.sel_rank;
    }
    *nv_out = nv;
    return nv ? prefix : 0u;
}

static __global__ __launch_bounds__(256) void pitch_match_kernel(const float* __restrict__ f0, PitchRowChunk rows, const float* __restrict__ target,
                                                                 float* __restrict__ median_out, int* __restrict__ voiced_out, float* __restrict__ shift_out,
                                                                 float* __restrict__ f0s) {
    __shared__ PitchSelectLds sel;
    __shared__ float sh_shift;
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const long n = rows.len[r];
    const float* p = f0 + rows.start[r];
    unsigned nv;
    const unsigned prefix = pitch_select(p, n, sel, &nv);
    if (tid == 0) {
        const float med = nv ? __uint_as_float(prefix) : 0.f;
        const int slot = rows.idx[r];
        const float off = rows.offset[r];
        float sh = off;
        if (target && nv) {
            const float tg = target[slot];
            if (tg > 0.f) sh = (float)((double)off + 12.0 * log2((double)tg / (double)med));
        }
        if (median_out) median_out[slot] = med;
        if (voiced_out) voiced_out[slot] = (int)nv;
        if (shift_out) shift_out[slot] = sh;
        sh_shift = sh;
    }
    if (!f0s) return;
    __syncthreads();
    const float sh = sh_shift;
    float* q = f0s + rows.start[r];
    for (long i = tid; i < n; i += 256) q[i] = shift_frequency_one(p[i], sh);
}

int run_pitch_match(tvc_ctx* ctx, hipStream_t s, const float* f0, const std::vector<PitchRow>& rows, const float* target, float* median_out, int* voiced_out,
                    float* shift_out, float* f0s) {
    for (size_t o = 0; o < rows.size(); o += kPmRows) {
        PitchRowChunk c{};
        const int n = (int)(rows.size() - o < (size_t)kPmRows ? rows.size() - o : (size_t)kPmRows);
        for (int i = 0; i < n; ++i) {
            c.start[i] = rows[o + i].start;
            c.len[i] = rows[o + i].len;
            c.idx[i] = rows[o + i].idx;
            c.offset[i] = rows[o + i].offset;
        }
        hipLaunchKernelGGL(pitch_match_kernel, dim3(n), dim3(256), 0, s, f0, c, target, median_out, voiced_out, shift_out, f0s);
    }
    return launch_check(ctx, "pitch_match");
}

// ---- the pitch register of a STREAM: a ring of its last W voiced f0 values, and a slew-limited shift onto the target's ---------------------
// A block's window is 28 frames: its own median jumps from block to block.  A stream's register is the lower median over its history, kept on
// the device (thousands of streams, one captured graph per block, no host synchronisation): per stream a ring [W] of the last W voiced
// values (unwritten slots 0.0, so the live entries are the entries > 0), count = the voiced frames appended since the last reset (write
// cursor count % W, fill min(count, W)) and `auto` = the automatic part of the latest shift.  One 256-thread workgroup per stream:
//   1. x_k = f0[s][start + k], k < n <= 256 (one per thread); voiced iff x_k > 0, pitch_match's rule
//   2. the voiced x_k in ascending k go to ring[(count + j) % W], j their rank among the voiced: a ballot prefix per wave plus the wave
//      offsets.  Equal to appending one at a time: of nv > W values only the last W are written (so no slot is written twice); count += nv.
//      The row is staged in LDS once, the append goes to LDS and to global memory, the select reads LDS: one global read of the row.
//   3. median = pitch_select over the staged row (rank (fill - 1) / 2 of its fill live entries)
//   4. wanted = fill >= min_voiced && target > 0 ? (float)(12 log2((double)target / (double)median)) : 0
//   5. d = wanted - auto;  |d| > slew ? auto += copysign(slew, d) : auto = wanted (it lands exactly; slew = +inf always lands, 0 never moves)
//   6. shift = offset + auto (one fp32 add), 7. f0s[s][:] = shift_frequency_one(f0[s][:], shift) over all T columns.
// W <= 8192: a row is at most 32 KiB of (dynamic) LDS, one code path.  Host values (T, start, n, W, min_voiced, slew, the offsets) are kernel
// arguments, baked into a capture like pitch_match's row descriptions; target, the ring, count and auto are read when the kernel runs.
// Integer arithmetic and order statistics only up to step 3: no floating-point sum, no floating-point atomic.
constexpr int kPtRows = 512;      // streams per launch when every stream has its own offset (2 KiB of kernel arguments); one launch otherwise
struct PitchTrackOffsets {
    float v[kPtRows];
};

static __global__ __launch_bounds__(256) void pitch_track_kernel(const float* __restrict__ f0, int T, int start, int n, int W, int min_voiced, float slew,
                                                                 float offset, PitchTrackOffsets offsets, int per_row, int s0, const float* __restrict__ target,
                                                                 float* __restrict__ ring, long long* __restrict__ count, float* __restrict__ autos,
                                                                 float* __restrict__ median_out, long long* __restrict__ count_out,
                                                                 float* __restrict__ shift_out, float* __restrict__ f0s) {
    extern __shared__ float row[];      // [W]
    __shared__ PitchSelectLds sel;
    __shared__ unsigned wave_voiced[4];
    __shared__ float sh_shift;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long s = s0 + (long)blockIdx.x;
    const float* p = f0 + s * T;
    float* rg = ring + s * W;
    const long long cnt = count[s];
    const int cursor = (int)(((cnt % W) + W) % W);      // (within the row even for a count the caller corrupted)
    for (int i = tid; i < W; i += 256) row[i] = rg[i];
    const float x = tid < n ? p[start + tid] : 0.f;
    const bool voiced = x > 0.f;
    const unsigned long long vb = __ballot(voiced);
    if (lane == 0) wave_voiced[wave] = (unsigned)__popcll(vb);
    __syncthreads();      // the staged row and the waves' counts
    int j = __popcll(vb & ((1ull << lane) - 1ull)), nv = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) j += (int)wave_voiced[w];
        nv += (int)wave_voiced[w];
    }
    if (voiced && nv - j <= W) {      // one of the last W: slot (cursor + j) % W, distinct over the writers
        const int slot = (cursor + j) % W;
        row[slot] = x;
        rg[slot] = x;
    }
    const long long now = cnt + nv;
    const int fill = now < (long long)W ? (int)now : W;
    __syncthreads();
    unsigned live;
    const unsigned bits = pitch_select(row, W, sel, &live);
    if (tid == 0) {
        const float med = __uint_as_float(bits);
        const float tg = target[s];
        float wanted = 0.f;
        if (live && fill >= min_voiced && tg > 0.f) wanted = (float)(12.0 * log2((double)tg / (double)med));
        float a = autos[s];
        const float d = __fsub_rn(wanted, a);
        a = fabsf(d) > slew ? __fadd_rn(a, copysignf(slew, d)) : wanted;
        const float sh = __fadd_rn(per_row ? offsets.v[blockIdx.x] : offset, a);
        count[s] = now;
        autos[s] = a;
        if (median_out) median_out[s] = med;
        if (count_out) count_out[s] = now;
        if (shift_out) shift_out[s] = sh;
        sh_shift = sh;
    }
    if (!f0s) return;
    __syncthreads();
    const float sh = sh_shift;
    float* q = f0s + s * T;
    for (int i = tid; i < T; i += 256) q[i] = shift_frequency_one(p[i], sh);
}

int run_pitch_track(tvc_ctx* ctx, hipStream_t s, const float* f0, int S, int T, const PitchTrackState& t, const float* target, float offset,
                    const float* offsets, float* median_out, int64_t* count_out, float* shift_out, float* f0s) {
    const size_t lds = (size_t)t.W * sizeof(float);
    PitchTrackOffsets o{};
    for (int s0 = 0; s0 < S; s0 += offsets ? kPtRows : S) {
        const int rows = offsets ? (S - s0 < kPtRows ? S - s0 : kPtRows) : S;
        if (offsets) std::memcpy(o.v, offsets + s0, (size_t)rows * sizeof(float));
        hipLaunchKernelGGL(pitch_track_kernel, dim3(rows), dim3(256), lds, s, f0, T, t.start, t.n, t.W, t.min_voiced, t.slew, offset, o, offsets ? 1 : 0, s0,
                           target, t.ring, reinterpret_cast<long long*>(t.count), t.autos, median_out, reinterpret_cast<long long*>(count_out), shift_out, f0s);
    }
    return launch_check(ctx, "pitch_track");
}

}  // namespace tvc
