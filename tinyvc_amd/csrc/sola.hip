// Streaming tail: SOLA alignment + cross-fade (stream.py:74-95) and the optional phase-vocoder
// cross-fade (stream.py:9-26), batched over streams, with the arg-max kept on the device (the
// reference's `.item()` host sync at stream.py:79 is what serialises concurrent streams).
//
// The geometry - cross-fade length `cross`, lag range `search`, look-ahead `delay` (stream.py:48-50 hard-codes 1920, 1920, 3840) - is a
// run-time argument of every kernel here, within sola_geometry's limits: the reference's values are the caps, so the static LDS arrays
// and the dynamic LDS budget are the reference geometry's.  The first sample a block emits lags the first sample of the newest input
// block by cross + search + delay - shift samples, shift in [0, search]: cross + delay .. cross + search + delay.  Every kernel is
// instantiated twice: FIXED = the reference's geometry as compile-time constants (the code the default streams have always run), and the
// run-time one; the sums, their order and the arg-max order are one text, so the lag search and the sin^2 tail give the same bits either
// way (the vocoder differs: the run-time one evaluates the formula in fp64, see there).
#include "tvc_common.h"

namespace tvc {

struct SolaGeom {
    int cross, search, delay;
};
// the geometry a kernel instantiation works with: compile-time constants when FIXED
#define TVC_SOLA_GEOM(g)                                 \
    const int CROSS = FIXED ? kSolaCross : (g).cross;    \
    const int SEARCH = FIXED ? kSolaSearch : (g).search; \
    const int DELAY = FIXED ? kSolaDelay : (g).delay

// phase_vocoder(a = sola buffer, b = new head, fade_out, fade_in) for n = 1920, written into `res`.
// Direct DFT of the two windowed segments (961 bins x 1920 samples each), then the 961-term cosine
// bank per output sample — O(n^2) like the reference's [1920, 961] broadcast.
static __device__ void phase_vocoder_block(const float* a, const float* b, const float* fin, float* res,
                                           float* re_a, float* im_a, float* re_b, float* im_b) {
    const int n = kSolaCross, nb = n / 2 + 1;
    const float two_pi = 6.283185307179586f;
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        float ra = 0.f, ia = 0.f, rb = 0.f, ib = 0.f;
        for (int j = 0; j < n; ++j) {
            float w = sqrtf((1.f - fin[j]) * fin[j]);
            float sn, cs;
            int r = (int)(((long)k * j) % n);
            sincosf(two_pi * (float)r / (float)n, &sn, &cs);
            float av = a[j] * w, bv = b[j] * w;
            ra = fmaf(av, cs, ra);
            ia = fmaf(-av, sn, ia);
            rb = fmaf(bv, cs, rb);
            ib = fmaf(-bv, sn, ib);
        }
        re_a[k] = ra; im_a[k] = ia; re_b[k] = rb; im_b[k] = ib;
    }
    __syncthreads();
    // per-bin magnitude sum, phase of a, wrapped phase advance
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        float mag = hypotf(re_a[k], im_a[k]) + hypotf(re_b[k], im_b[k]);
        if (k >= 1 && k < nb - 1) mag *= 2.f;
        float pa = atan2f(im_a[k], re_a[k]);
        float pb = atan2f(im_b[k], re_b[k]);
        float dp = pb - pa;
        dp = dp - two_pi * floorf(dp / 2.f / 3.14159265358979f + 0.5f);
        re_a[k] = mag;                       // reuse: magnitude
        im_a[k] = pa;                        // phase of a
        re_b[k] = two_pi * (float)k + dp;    // w
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        float t = (float)j / (float)n;
        float acc = 0.f;
        for (int k = 0; k < nb; ++k) acc += re_a[k] * cosf(re_b[k] * t + im_a[k]);
        float fi = fin[j], fo = 1.f - fi;
        float w = sqrtf(fo * fi);
        res[j] = a[j] * (fo * fo) + b[j] * (fi * fi) + acc * w / (float)n;
    }
    __syncthreads();
}

// The same formula for a run-time even n, evaluated in fp64 and rounded to fp32 once per output sample.  A short head has no sum to hide
// behind: at n = 4 three samples carry all of it, and every fp32 rounding on the way (a twiddle that misses cos = 0 by 4e-8, hypotf,
// atan2f, cosf) shows in the last place of the result.  Rounded once, a sample is the fp32 value nearest the exact one, so no fp32
// evaluation of the formula - the reference's included - is nearer.  The twiddle of the rational angle 2 pi r / n comes from sincospi's
// exact reduction.  Each thread keeps its bins from the DFT through the phase step in registers; mag, pha, dph: nb doubles each.
static __device__ void phase_vocoder_block_rt(const float* a, const float* b, const float* fin, float* res,
                                              double* mag, double* pha, double* dph, int n) {
    const int nb = n / 2 + 1;
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        double ra = 0., ia = 0., rb = 0., ib = 0.;
        for (int j = 0; j < n; ++j) {
            const double fi = (double)fin[j];
            const double w = sqrt((1. - fi) * fi);
            double sn, cs;
            const int r = (int)(((long)k * j) % n);
            sincospi((double)(2 * r) / (double)n, &sn, &cs);
            const double av = (double)a[j] * w, bv = (double)b[j] * w;
            ra = fma(av, cs, ra);
            ia = fma(-av, sn, ia);
            rb = fma(bv, cs, rb);
            ib = fma(-bv, sn, ib);
        }
        double m = hypot(ra, ia) + hypot(rb, ib);
        if (k >= 1 && k < nb - 1) m *= 2.;
        const double pa = atan2(ia, ra);
        double dp = atan2(ib, rb) - pa;
        dp = dp - two_pi * floor(dp / 2. / pi + 0.5);
        mag[k] = m; pha[k] = pa; dph[k] = dp;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const double t = (double)j / (double)n;
        double acc = 0.;
        for (int k = 0; k < nb; ++k) acc += mag[k] * cos((two_pi * (double)k + dph[k]) * t + pha[k]);
        const double fi = (double)fin[j], fo = 1. - fi;
        res[j] = (float)((double)a[j] * (fo * fo) + (double)b[j] * (fi * fi) + acc * sqrt(fo * fi) / (double)n);
    }
    __syncthreads();
}

// The order of the lag arg-max, shared by every step of it (per thread, across lanes, across waves, across lag groups): is candidate
// (ov, oi) ahead of (bv, bi)?  torch.argmax's rule - a NaN correlation is ahead of any number, among equals (two NaNs included) the
// lower lag is - which is a total order, so the result does not depend on how the lags were split, and a thread that starts from
// (-inf, kNoLag) ends with a lag in [0, SEARCH] as soon as it has seen one.
constexpr int kNoLag = 0x7fffffff;
static __device__ __forceinline__ bool lag_ahead(float ov, int oi, float bv, int bi) {
    if (ov != ov) return bv == bv || oi < bi;
    return bv == bv && (ov > bv || (ov == bv && oi < bi));
}

// Normalised cross-correlation over the SEARCH + 1 lags (the two F.conv1d of stream.py:77-78), split over kSolaGroups workgroups
// per stream: one lag per thread, the same sums in the same order as the one-workgroup kernel below (bit-identical values), so
// the search of 32 streams fills the chip instead of 32 CUs (173 us -> see DESIGN.md).  part[(st * G + g) * 2] = best value of
// the group, [.. + 1] = its lag (as bits); the order is lag_ahead's.  A group takes LPG = ceil((SEARCH + 1) / kSolaGroups) consecutive lags
// (241 at the reference's search, the most there is); at a short search the last groups are short or empty (search + 1 < 8 * LPG).
template <bool FIXED>
static __global__ __launch_bounds__(256) void sola_corr_kernel(const float* __restrict__ y, const float* __restrict__ sola_buf,
                                                               float* __restrict__ part, long Ly, int block, SolaGeom geom) {
    TVC_SOLA_GEOM(geom);
    constexpr int kMaxLPG = (kSolaSearch + 1 + kSolaGroups - 1) / kSolaGroups;     // 241 lags per group at the largest search
    const int LPG = (SEARCH + 1 + kSolaGroups - 1) / kSolaGroups;                  // <= 241 <= the 256 threads: one lag per thread
    __shared__ float ci[kMaxLPG + kSolaCross];
    __shared__ __attribute__((aligned(16))) float sb[kSolaCross];
    __shared__ float bestv[4];
    __shared__ int besti[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int st = blockIdx.x / kSolaGroups, g = blockIdx.x - st * kSolaGroups;
    const int lag0 = g * LPG;
    if constexpr (!FIXED) {
        // a group that starts past the last lag (search + 1 < 8 * LPG) has nothing to look at: it reports "no lag", which is behind every lag
        if (lag0 > SEARCH) {
            if (tid == 0) {
                part[(long)blockIdx.x * 2] = -INFINITY;
                part[(long)blockIdx.x * 2 + 1] = __int_as_float(kNoLag);
            }
            return;
        }
    }
    const int tw_len = block + CROSS + SEARCH;
    const float* tw = y + (long)st * Ly + (Ly - tw_len - DELAY) + lag0;
    const int nload = (lag0 + LPG + CROSS <= CROSS + SEARCH ? LPG + CROSS : CROSS + SEARCH - lag0);
    for (int i = tid; i < LPG + CROSS; i += 256) {
        ci[i] = i < nload ? tw[i] : 0.f;
    }
    for (int i = tid; i < CROSS; i += 256) sb[i] = sola_buf[(long)st * CROSS + i];
    __syncthreads();
    float bv = -INFINITY;
    int bi = kNoLag;
    const int lag = lag0 + tid;
    if (tid < LPG && lag <= SEARCH) {
        float nom = 0.f, den = 0.f;
        // (the loop is LDS-bound - three 4-byte reads per term for four waves -: the buffer's four values come as one 16-byte broadcast read
        // and the square is taken in a register; same products and sums in the same order)
        const float* c = ci + tid;
        static_assert(kSolaCross % 4 == 0, "four terms per broadcast read");      // (sola_geometry: cross % 4 == 0)
#pragma unroll 2
        for (int j = 0; j < CROSS; j += 4) {
            const float4 b4 = *reinterpret_cast<const float4*>(sb + j);
            const float c0 = c[j], c1 = c[j + 1], c2 = c[j + 2], c3 = c[j + 3];
            nom = fmaf(c0, b4.x, nom);
            den = __fadd_rn(den, __fmul_rn(c0, c0));
            nom = fmaf(c1, b4.y, nom);
            den = __fadd_rn(den, __fmul_rn(c1, c1));
            nom = fmaf(c2, b4.z, nom);
            den = __fadd_rn(den, __fmul_rn(c2, c2));
            nom = fmaf(c3, b4.w, nom);
            den = __fadd_rn(den, __fmul_rn(c3, c3));
        }
        bv = nom / sqrtf(den + 1e-8f);
        bi = lag;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(bv, o);
        int oi = __shfl_xor(bi, o);
        if (lag_ahead(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { bestv[wave] = bv; besti[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = bestv[0];
        int i = besti[0];
        for (int w = 1; w < 4; ++w)
            if (lag_ahead(bestv[w], besti[w], v, i)) { v = bestv[w]; i = besti[w]; }
        part[(long)blockIdx.x * 2] = v;
        part[(long)blockIdx.x * 2 + 1] = __int_as_float(i);
    }
}

// one workgroup per stream; `part` != nullptr: the lag search was done by sola_corr_kernel, only its kSolaGroups candidates are compared here
// (run_sola: while the scratch holds them, S <= kSolaPartFloats / 16 = 1024 streams); `part` == nullptr: the search runs here, lags strided by 256
// over the threads - the same sums, and through lag_ahead the same lag (tests/test_gpu_sola.py compares the two row by row)
template <bool FIXED>
static __global__ __launch_bounds__(256) void sola_kernel(const float* __restrict__ y, float* __restrict__ sola_buf,
                                                          const float* __restrict__ fade_in, float* __restrict__ out,
                                                          int32_t* __restrict__ shift_out, long Ly, int block, int use_pv,
                                                          const float* __restrict__ part, SolaGeom geom) {
    TVC_SOLA_GEOM(geom);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* ci = sm;                       // [CROSS + SEARCH] head of temp_wav
    float* sb = sm + CROSS + SEARCH;      // [CROSS] sola buffer
    float* sq = sb + CROSS;               // [CROSS + SEARCH] squares of ci
    __shared__ float bestv[4];
    __shared__ int besti[4];
    __shared__ int s_shift;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int st = blockIdx.x;
    const int tw_len = block + CROSS + SEARCH;  // temp_wav = y[-tw_len-DELAY : -DELAY]
    const float* tw = y + (long)st * Ly + (Ly - tw_len - DELAY);
    float* sbuf = sola_buf + (long)st * CROSS;

    if (!part) {
        for (int i = tid; i < CROSS + SEARCH; i += 256) {
            float v = tw[i];
            ci[i] = v;
            sq[i] = v * v;
        }
    }
    for (int i = tid; i < CROSS; i += 256) sb[i] = sbuf[i];
    __syncthreads();

    // normalised cross-correlation over SEARCH+1 lags (two F.conv1d in stream.py:77-78)
    float bv = -INFINITY;
    int bi = kNoLag;
    if (part) {
        if (tid < kSolaGroups) {
            bv = part[((long)st * kSolaGroups + tid) * 2];
            bi = __float_as_int(part[((long)st * kSolaGroups + tid) * 2 + 1]);
        }
    } else {
        for (int lag = tid; lag <= SEARCH; lag += 256) {
            float nom = 0.f, den = 0.f;
            for (int j = 0; j < CROSS; ++j) {
                nom = fmaf(ci[lag + j], sb[j], nom);
                den += sq[lag + j];
            }
            float v = nom / sqrtf(den + 1e-8f);
            if (lag_ahead(v, lag, bv, bi)) { bv = v; bi = lag; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(bv, o);
        int oi = __shfl_xor(bi, o);
        if (lag_ahead(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { bestv[wave] = bv; besti[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = bestv[0];
        int i = besti[0];
        for (int w = 1; w < 4; ++w)
            if (lag_ahead(bestv[w], besti[w], v, i)) { v = bestv[w]; i = besti[w]; }
        s_shift = i;
        if (shift_out) shift_out[st] = i;
    }
    __syncthreads();
    const int shift = s_shift;
    const float* seg = tw + shift;  // temp_wav[shift : shift + block + CROSS]

    // cross-faded head (first CROSS samples) into ci[0:CROSS]
    if (use_pv) {
        float* head = sq;            // b = seg[:CROSS]
        for (int i = tid; i < CROSS; i += 256) head[i] = seg[i];
        __syncthreads();
        float* scratch = sm + 2 * (CROSS + SEARCH) + CROSS + 8;
        const int nbp = (CROSS / 2 + 1 + 7) & ~7;      // a spectrum's bins, rounded up to 8: 968 at 1920
        if constexpr (FIXED) {
            phase_vocoder_block(sb, head, fade_in, ci, scratch, scratch + nbp, scratch + 2 * nbp, scratch + 3 * nbp);
        } else {      // (scratch starts an even number of floats into the 16-byte aligned sm: doubles sit on 8 bytes)
            double* sc = reinterpret_cast<double*>(scratch);
            phase_vocoder_block_rt(sb, head, fade_in, ci, sc, sc + nbp, sc + 2 * nbp, CROSS);
        }
    } else {
        for (int i = tid; i < CROSS; i += 256) {
            float fi = fade_in[i];
            ci[i] = __fadd_rn(__fmul_rn(seg[i], fi), __fmul_rn(sb[i], 1.f - fi));
        }
        __syncthreads();
    }
    // temp = [head (CROSS) | seg[CROSS : block + CROSS]];  out = temp[:block]; sola = temp[block:]
    float* o = out + (long)st * block;
    for (int i = tid; i < block; i += 256) o[i] = i < CROSS ? ci[i] : seg[i];
    for (int i = tid; i < CROSS; i += 256) {
        int src = block + i;
        sbuf[i] = src < CROSS ? ci[src] : seg[src];
    }
}

// The one place that says which geometries the kernels take (tvc_sola_geometry, tvc_sola_geom_f32 and through it tvc_sola_f32).  0, or
// TVC_ERR_ARG with the reason in `why` (nullable):
//   4 <= cross <= 1920, cross % 4 == 0   the split search reads the buffer 16 bytes at a time; an even n keeps the vocoder on the reference's even-n branch
//   0 <= search <= 1920                  0 = one lag: a plain cross-fade
//   delay >= 0, 1 <= block <= 2^30
int sola_geometry(int block, int cross, int search, int delay, int64_t* min_ly, int* latency_min, int* latency_max, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, int v) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v);
        return (int)TVC_ERR_ARG;
    };
    if (cross < 4 || cross > kSolaCross) return refuse("cross = %d is outside 4 .. 1920", cross);
    if (cross % 4) return refuse("cross = %d is not a multiple of 4", cross);
    if (search < 0 || search > kSolaSearch) return refuse("search = %d is outside 0 .. 1920", search);
    if (delay < 0) return refuse("delay = %d is negative", delay);
    if (block < 1) return refuse("block = %d is not positive", block);
    if (block > kSolaMaxBlock) return refuse("block = %d is above 2^30", block);      // block + cross + search stays an int in the kernels
    if (why && why_bytes) why[0] = 0;
    if (min_ly) *min_ly = (int64_t)block + cross + search + delay;
    if (latency_min) *latency_min = (int)std::min<int64_t>((int64_t)cross + delay, INT32_MAX);
    if (latency_max) *latency_max = (int)std::min<int64_t>((int64_t)cross + search + delay, INT32_MAX);
    return 0;
}

template <bool FIXED>
static void launch_sola(hipStream_t s, const float* y, float* sola_buf, const float* fade_in, float* out, int32_t* shift_out, int S, int64_t Ly,
                        int block, int use_pv, float* part, SolaGeom g) {
    // ci, sb, sq, 8 floats of slack, the vocoder's four spectra (cross / 2 + 1 bins each, rounded up to 8); the run-time vocoder keeps
    // three fp64 arrays there instead, half as much again: 61 728 bytes at the caps, inside the 64 KiB a workgroup gets without asking
    const int nbp = (g.cross / 2 + 1 + 7) & ~7;
    const size_t lds = (size_t)(2 * (g.cross + g.search) + g.cross + 8 + (!FIXED && use_pv ? 6 : 4) * nbp) * sizeof(float) + 64;
    if (part) hipLaunchKernelGGL(sola_corr_kernel<FIXED>, dim3(S * kSolaGroups), dim3(256), 0, s, y, sola_buf, part, (long)Ly, block, g);
    hipLaunchKernelGGL(sola_kernel<FIXED>, dim3(S), dim3(256), lds, s, y, sola_buf, fade_in, out, shift_out, (long)Ly, block, use_pv, part, g);
}

// (the caller has checked the geometry and Ly against sola_geometry)
int run_sola(tvc_ctx* ctx, hipStream_t s, const float* y, float* sola_buf, const float* fade_in, float* out,
             int32_t* shift_out, int S, int64_t Ly, int block, int cross, int search, int delay, int use_pv) {
    // the lag search on S * kSolaGroups workgroups when its scratch (context-owned, one call at a time like every other scratch of the
    // context) holds their candidates; the arg-max, cross-fade and buffer update stay one workgroup per stream
    float* part = nullptr;
    if (ctx->sola_part && (long)S * kSolaGroups * 2 <= kSolaPartFloats) part = const_cast<float*>(ctx->sola_part);
    const SolaGeom g{cross, search, delay};
    if (cross == kSolaCross && search == kSolaSearch && delay == kSolaDelay)
        launch_sola<true>(s, y, sola_buf, fade_in, out, shift_out, S, Ly, block, use_pv, part, g);
    else
        launch_sola<false>(s, y, sola_buf, fade_in, out, shift_out, S, Ly, block, use_pv, part, g);
    return launch_check(ctx, "sola");
}

// The rolling input buffer of a stream (stream.py:69-70: `input_wav = roll(input_wav, -block)`, `input_wav[-block:] = block`), in place and in
// ONE launch instead of three ATen kernels: buf[st][i] = buf[st][i + m] for i < n - m, buf[st][n - m + j] = blocks[st][j].  One workgroup per
// stream reads the whole row into registers (PER x 1024 >= n), meets at a barrier, writes it back shifted.
// TILED: a row longer than PER x 1024 samples is walked in tiles of that size in ascending order, each tile read into registers, a barrier,
// written back.  The shift goes left, so tile k reads only indices >= its own start + m: no earlier tile wrote them, and a later tile writes
// only behind a later barrier, after every thread has read tile k.
template <int PER, bool TILED = false>
static __global__ __launch_bounds__(1024) void stream_push_kernel(float* __restrict__ buf, const float* __restrict__ blocks, int n, int m) {
    float* b = buf + (long)blockIdx.x * n;
    const float* nb = blocks + (long)blockIdx.x * m;
    const int tiles = TILED ? (n + PER * 1024 - 1) / (PER * 1024) : 1;
    for (int k = 0; k < tiles; ++k) {
        const int i0 = k * (PER * 1024) + threadIdx.x;
        float v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = i0 + j * 1024;
            v[j] = i < n - m ? b[i + m] : (i < n ? nb[i - (n - m)] : 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = i0 + j * 1024;
            if (i < n) b[i] = v[j];
        }
    }
}
int run_stream_push(tvc_ctx* ctx, hipStream_t s, float* buf, const float* blocks, int S, int n, int m) {
    const int per = (n + 1023) / 1024;
    if (per <= 16) hipLaunchKernelGGL(stream_push_kernel<16>, dim3((unsigned)S), dim3(1024), 0, s, buf, blocks, n, m);
    else if (per <= 32) hipLaunchKernelGGL(stream_push_kernel<32>, dim3((unsigned)S), dim3(1024), 0, s, buf, blocks, n, m);
    else hipLaunchKernelGGL((stream_push_kernel<32, true>), dim3((unsigned)S), dim3(1024), 0, s, buf, blocks, n, m);
    return launch_check(ctx, "stream_push");
}

}  // namespace tvc
