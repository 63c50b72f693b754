// kNN feature match (feature_retrieval.py:15-33, metrics='cos', k=4, alpha=0).
//
// The reference materialises sims[T][N] and calls torch.topk; here the index streams through the matrix pipe in
// 128-vector tiles and every lane keeps a running top-4 for the query column it owns in the MFMA accumulator layout
// (index vectors are the M axis, queries the N axis, so the 16 accumulator registers of a lane are 16 index vectors
// against ONE query: the reduction is lane-local).  The index is split across workgroups for occupancy; a second kernel
// merges the per-split candidates, emits int64 indices and gathers + averages the 4 raw index vectors.
// This file is the search: query normalisation, the exact top-4 kernel, the two-stage coarse + rescore search and the host plan
// (knn_search.h).  Prepared blobs are written by knn_prepare.hip (layout: knn_blob.h); the lists become results in knn_gather.hip.
//
// Similarities run on the split-precision path (conv3s.h): bf16 part-products, fp32 accumulation, error below an fp32
// FMA chain's.  Two index storages share the kernels (the prepared blob is self-describing, so every entry point - and a
// captured HIP graph - works with either):
//   kind 0, fp32 storage: raw rows [N][768] fp32 (the final gather) + the cosine-normalised vectors as three bf16 parts
//           per value in MFMA lane order (10 B per element); six part-products per product; bit-exact indices on the
//           gap-checked fixtures.
//   kind 1, fp16 storage (BASELINE configs[4]: a 1 M-vector index): the raw vectors as fp16 in MFMA lane
//           order + one fp32 inverse norm per vector (2 B per element: 1.5 GB at N = 1 M).  An fp16 value is exactly two
//           bf16 parts, split while a tile is staged into LDS; five part-products per product; the similarity is
//           dot(q_hat, r) * inv_norm; the gather reads the same image.
// Tie-break: equal similarities -> lower index first (torch.topk leaves it unspecified).
#include "knn_blob.h"
#include "knn_search.h"
#include "split_fp16.h"
#include "tvc_common.h"

namespace tvc {

constexpr int KNN_BLOCKS = 1024;   // target workgroup count (query tiles x index splits)

// qn[b][k][t] = src[b][k][t] / (||src[b][:][t]|| + 1e-6).  One workgroup = 64 consecutive columns;
// its 4 waves each sum a quarter of the 768 channels (lanes along time, coalesced), partial sums of
// squares meet in LDS in a fixed order, then every wave rescales its quarter.
// qh (optional) = the same values in fp16, in the coarse pass's B-fragment order [256-query tile][K16 step][8-channel half][query][8]
// (a segment's tiles are consecutive, its columns beyond its own count in its last tile are zero: the grid then runs over whole tiles);
// cnt / flag (optional) = the two-stage search's per-query candidate counters and the segments' overflow flags, zeroed here;
// col2seg (optional, several segments) = the segment of every column.
// Bsrc = rows of src: row b of qn holds the queries of src row b % Bsrc (a blend call searches every source row once per term: B = terms x
// Bsrc virtual rows; every other call has Bsrc == B).
constexpr int QN_WAVES = 16;     // waves per 64-column group: each squares / scales KD / 16 = 48 channels (strided rows: the loop is a latency chain)
static __global__ __launch_bounds__(QN_WAVES * 64) void query_normalize_kernel(const float* __restrict__ src, float* __restrict__ qn, int B, int Bsrc, int T,
                                                                     uint4* __restrict__ qh, int* __restrict__ cnt, int* __restrict__ flag,
                                                                     const KnnSegs segs, int* __restrict__ col2seg) {
    __shared__ float part[QN_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long ncols = (long)B * T;
    long n, nn;
    bool ok;
    int sg;
    if (qh) {      // tile-aligned: the group's four 64-column quarters of one query tile belong to one segment
        const int tile = blockIdx.x >> 2;
        sg = seg_find<3>(segs, tile);
        const KnnSeg g = seg_get(segs, sg);
        const long loc = (long)(tile - g.u[3]) * 256 + (blockIdx.x & 3) * 64 + lane;
        ok = loc < g.ncols;
        n = g.col0 + loc;
        nn = ok ? n : g.col0 + g.ncols - 1;
    } else {
        n = blockIdx.x * 64L + lane;
        ok = n < ncols;
        nn = ok ? n : ncols - 1;
        sg = col2seg ? seg_find<4>(segs, (int)nn) : 0;
    }
    // bookkeeping first: nothing of it stays live across the 48-channel loads (this kernel runs at 128 registers)
    if (blockIdx.x == 0 && flag)
        for (int i = threadIdx.x; i < segs.n; i += QN_WAVES * 64) flag[i] = 0;
    if (wave == 0 && ok && cnt) cnt[n] = 0;
    if (wave == 0 && ok && col2seg) col2seg[n] = sg;
    const int b = (int)(nn / T), t = (int)(nn - (long)b * T);
    const float* p = src + (long)(b % Bsrc) * KD * T + t;
    float* q = qn + (long)b * KD * T + t;
    constexpr int KW = KD / QN_WAVES;
    const int k0 = wave * KW;
    float x[KW];       // the wave's 48 channels stay in registers: requested together (the summing loop was a chain of load latencies), read once
#pragma unroll
    for (int i = 0; i < KW; ++i) x[i] = p[(long)(k0 + i) * T];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < KW; ++i) s = fmaf(x[i], x[i], s);
    part[wave][lane] = s;
    __syncthreads();
    float ss = part[0][lane];
#pragma unroll
    for (int w = 1; w < QN_WAVES; ++w) ss += part[w][lane];      // fixed order
    const float den = sqrtf(ss) + 1e-6f;
    uint4* qhp = qh ? qh + (blockIdx.x >> 2) * (long)(STEPS * 2 * 256) + (blockIdx.x & 3) * 64 + lane : nullptr;
#pragma unroll
    for (int i = 0; i < KW; i += 8) {
        const int k = k0 + i;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ok ? x[i + j] / den : 0.f;
        if (ok) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[(long)(k + j) * T] = v[j];
        }
        if (qh) {
            unsigned o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const __half2 h = __floats2half2_rn(v[2 * j], v[2 * j + 1]);
                o[j] = (unsigned)__half_as_ushort(__low2half(h)) | ((unsigned)__half_as_ushort(__high2half(h)) << 16);
            }
            qhp[(long)(k >> 3) * 256] = make_uint4(o[0], o[1], o[2], o[3]);     // (K16 step, half) = k / 8
        }
    }
}

// The exact kernel's own split: three bf16 parts per fp32 operand (x = x1 + x2 + x3, residuals exact), six part-products per
// product on v_mfma_f32_32x32x16_bf16.  (The conv / GEMM kernels moved to the two-term fp16 split of conv3s.h; this kernel only runs
// for N < 4096 and as the in-call fallback of the two-stage search, whose coarse passes are single fp16 products.)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split8_bf3(const float (&v)[8], uint4& p1, uint4& p2, uint4& p3) {
    unsigned o1[4], o2[4], o3[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2 a = {v[2 * j], v[2 * j + 1]};
        bf16x2 h1 = __builtin_convertvector(a, bf16x2);
        f32x2 r = a - __builtin_convertvector(h1, f32x2);
        bf16x2 h2 = __builtin_convertvector(r, bf16x2);
        f32x2 r2 = r - __builtin_convertvector(h2, f32x2);
        bf16x2 h3 = __builtin_convertvector(r2, bf16x2);
        o1[j] = __builtin_bit_cast(unsigned, h1);
        o2[j] = __builtin_bit_cast(unsigned, h2);
        o3[j] = __builtin_bit_cast(unsigned, h3);
    }
    p1 = make_uint4(o1[0], o1[1], o1[2], o1[3]);
    p2 = make_uint4(o2[0], o2[1], o2[2], o2[3]);
    p3 = make_uint4(o3[0], o3[1], o3[2], o3[3]);
}
// two bf16 parts of 8 fp16 values (exact: 11 significant bits fit in 8 + 8), packed for one 16-byte LDS row each
__device__ __forceinline__ void split8_half(const u32x4 h8, uint4& p1, uint4& p2) {
    const f16x8 hv = __builtin_bit_cast(f16x8, h8);
    unsigned o1[4], o2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2 a = {(float)hv[2 * j], (float)hv[2 * j + 1]};
        bf16x2 h1 = __builtin_convertvector(a, bf16x2);
        f32x2 r = a - __builtin_convertvector(h1, f32x2);
        bf16x2 h2 = __builtin_convertvector(r, bf16x2);
        o1[j] = __builtin_bit_cast(unsigned, h1);
        o2[j] = __builtin_bit_cast(unsigned, h2);
    }
    p1 = make_uint4(o1[0], o1[1], o1[2], o1[3]);
    p2 = make_uint4(o2[0], o2[1], o2[2], o2[3]);
}

// grid = qtiles * nsplit; workgroup = KNN_QT queries x (tiles_per_split index tiles of 128).
// 8 waves as 2 (index halves) x 4 (query quarters); a wave owns 64 index vectors x 64 queries = 2 x 2 MFMA tiles, so every
// A and B fragment read from LDS feeds two MFMAs (0.5 KiB of LDS reads per MFMA; the 64 x 32 wave tile of round 1 read
// 0.75) and a (tile, step) carries 24 MFMAs per wave between barriers.  The (tile, step) sequence is one flat pipeline:
// registers hold step g+1, LDS is double-buffered, one raw barrier per step.
// NP = bf16 parts per index value in LDS (3: fp32 storage, 2: fp16 storage).
constexpr int KNN_QT = 256;                                      // queries per workgroup
constexpr int KNN_A_U4 = 12 * 64, KNN_X_U4 = 3 * 2 * KNN_QT;    // one LDS buffer each: 12 KiB + 24 KiB
// (unit = this workgroup's work unit inside its segment; the segment's ncols queries start at column col0 of the call, the candidate
// lists are [split][cstride][4] over all columns of the call)
template <bool F16>
__device__ __forceinline__ void knn_topk_body(const float* __restrict__ blob, long Npad, int N, const float* __restrict__ qn, int ncols, int col0, int cstride,
                                              int T, int unit, int nsplit, int tiles_per_split, float* __restrict__ cand_v, int* __restrict__ cand_i,
                                              uint4* smem) {
    constexpr int NP = F16 ? 2 : 3;                    // parts per index value in LDS
    constexpr int GP = F16 ? 4 : 12;                   // 1 KiB pieces per (tile, step) in the global image
    uint4* As = smem;
    uint4* Xs = smem + 2 * KNN_A_U4;
    const uint4* img = F16 ? blob_img16(blob, KIND_F16, N, Npad) : blob_img3(blob, N);
    const float* inv = blob_inv(blob, KIND_F16, N, Npad);      // fp16 storage only

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int l31 = lane & 31, lh = lane >> 5;
    const int split = unit % nsplit;
    const int qtile = unit / nsplit;
    const int n0 = qtile * KNN_QT;
    const int mtiles = (int)(Npad >> 7);
    const int mt_lo = split * tiles_per_split;
    const int mt_hi = min(mtiles, mt_lo + tiles_per_split);
    const int G = (mt_hi - mt_lo) * STEPS;               // flat (tile, step) sequence

    // staging roles: every thread owns one query item (8 channels of one column: 2 halves x 256 columns); the index pieces of
    // a (tile, step) go to waves p % 8 (fp32 storage: 12 pieces, waves 0..3 take two) or to waves 0..3 (fp16 storage: one
    // fp16 piece each, split into its two bf16 parts on the way into LDS)
    const float* qp;
    int xdst;
    {
        const int g = tid >> 8, pos = tid & 255;
        int n = n0 + pos;
        n = col0 + (n < ncols ? n : ncols - 1);
        const int b = n / T, t = n - b * T;
        qp = qn + ((long)b * KD + 8 * g) * T + t;
        xdst = g * KNN_QT + pos;
    }
    const bool a2 = !F16 && wave < 4;                  // this wave stages a second piece (wave + 8)
    const bool a1 = !F16 || wave < 4;
    float xr[8];
    u32x4 ar[2];
    auto gload = [&](int g) __attribute__((always_inline)) {
        const int mt = mt_lo + g / STEPS, st = g - (g / STEPS) * STEPS;
        const uint4* src = img + ((long)mt * STEPS + st) * (GP * 64) + lane;
        if (a1) ar[0] = *reinterpret_cast<const u32x4*>(src + wave * 64);
        if (a2) ar[1] = *reinterpret_cast<const u32x4*>(src + (wave + 8) * 64);
#pragma unroll
        for (int j = 0; j < 8; ++j) xr[j] = qp[(long)(st * 16 + j) * T];
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        uint4* ab = As + buf * KNN_A_U4;
        if (F16) {
            if (a1) {
                uint4 p1, p2;
                split8_half(ar[0], p1, p2);
                ab[(wave * 2) * 64 + lane] = p1;
                ab[(wave * 2 + 1) * 64 + lane] = p2;
            }
        } else {
            *reinterpret_cast<u32x4*>(ab + wave * 64 + lane) = ar[0];
            if (a2) *reinterpret_cast<u32x4*>(ab + (wave + 8) * 64 + lane) = ar[1];
        }
        uint4 p1, p2, p3;
        split8_bf3(xr, p1, p2, p3);
        uint4* xb = Xs + buf * KNN_X_U4;
        xb[xdst] = p1;
        xb[2 * KNN_QT + xdst] = p2;
        xb[4 * KNN_QT + xdst] = p3;
    };

    Top4 top[2];
    top[0].init();
    top[1].init();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (G > 0) {
        gload(0);
        lstore(0);
        if (G > 1) gload(1);
        slab_barrier();
    }
    for (int g = 0; g < G; ++g) {
        const int cur = g & 1;
        if (g + 1 < G) {
            lstore(cur ^ 1);                        // step g+1 (its buffer was last read in step g-1, behind the barrier)
            if (g + 2 < G) gload(g + 2);            // flies across this step's MFMAs and the next barrier
        }
        const uint4* as = As + cur * KNN_A_U4 + wm * (2 * NP * 64) + lane;
        const uint4* xs = Xs + cur * KNN_X_U4 + lh * KNN_QT + wn * 64 + l31;
        bf16x8 af[2][NP], bf[2][3];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < 3; ++p) bf[j][p] = __builtin_bit_cast(bf16x8, xs[p * 2 * KNN_QT + j * 32]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int p = 0; p < NP; ++p) af[i][p] = __builtin_bit_cast(bf16x8, as[(i * NP + p) * 64]);
        // part-products, least significant first: (index part, query part)
        constexpr int NQ = F16 ? 5 : 6;
        constexpr int PA3[6] = {2, 1, 0, 1, 0, 0}, PB3[6] = {0, 1, 2, 0, 1, 0};
        constexpr int PA2[5] = {1, 0, 1, 0, 0}, PB2[5] = {1, 2, 0, 1, 0};
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][F16 ? PA2[q < 5 ? q : 0] : PA3[q]], bf[j][F16 ? PB2[q < 5 ? q : 0] : PB3[q]],
                                                                        acc[i][j], 0, 0, 0);
        const int st = g - (g / STEPS) * STEPS;
        if (st == STEPS - 1) {
            // running top-4: a lane's 16 registers of one MFMA tile are 16 index vectors against ONE of its two queries
            const int m0 = (mt_lo + g / STEPS) * 128;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (row < N) {
                        const float sc = F16 ? inv[row] : 1.f;
#pragma unroll
                        for (int j = 0; j < 2; ++j) top[j].insert(nan_max(F16 ? acc[i][j][r] * sc : acc[i][j][r]), row);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j][r] = 0.f;
                }
        }
        slab_barrier();
    }

    // merge the 4 partial lists (wm in {0,1} x lh in {0,1}) of every query through LDS (the staging buffers are free now:
    // the loop's last barrier is behind every wave's last fragment read)
    float (*mv)[16] = reinterpret_cast<float (*)[16]>(smem);
    int (*mi)[16] = reinterpret_cast<int (*)[16]>(reinterpret_cast<float*>(smem) + KNN_QT * 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wn * 64 + j * 32 + l31;
        const int slot = (wm * 2 + lh) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mv[q][slot + e] = top[j].v[e];
            mi[q][slot + e] = top[j].i[e];
        }
    }
    __syncthreads();
    if (tid < KNN_QT) {
        Top4 t4;
        t4.init();
        for (int e = 0; e < 16; ++e) t4.insert(mv[tid][e], mi[tid][e]);
        int n = n0 + tid;
        if (n < ncols) {
            long o = ((long)split * cstride + col0 + n) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cand_v[o + e] = t4.v[e];
                cand_i[o + e] = t4.i[e];
            }
        }
    }
}

// grid = the exact plan's units of every segment; flags = the segments' overflow flags (nullptr: no segment searches in two stages)
static __global__ __launch_bounds__(512) void knn_topk_split_kernel(const KnnSegs segs, const float* __restrict__ qn, int cstride, int T,
                                                                    float* __restrict__ cand_v, int* __restrict__ cand_i,
                                                                    const int* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint4 smem[2 * (KNN_A_U4 + KNN_X_U4)];      // 72 KiB; the final merge reuses 32 KiB of it
    const int si = seg_find<2>(segs, blockIdx.x);
    const KnnSeg g = seg_get(segs, si);
    if (g.two && flags[si] == 0) return;                         // the segment's two-stage search succeeded: nothing to do (uniform)
    const int kind = blob_kind(g.blob);                          // uniform: which storage this prepared index uses
    const int unit = blockIdx.x - g.u[2];
    if (kind == KIND_F16) knn_topk_body<true>(g.blob, blob_npad(g.N), g.N, qn, g.ncols, g.col0, cstride, T, unit, g.nsE, g.tpsE, cand_v, cand_i, smem);
    else knn_topk_body<false>(g.blob, blob_npad(g.N), g.N, qn, g.ncols, g.col0, cstride, T, unit, g.nsE, g.tpsE, cand_v, cand_i, smem);
}

// =================================================================================================
// Two-stage search (N >= KNN_COARSE_MIN).  The exact kernel above spends six bf16 part-products per similarity on every
// (query, index vector) pair although only a handful of index vectors per query can be in the top 4.  Stage 1 computes a
// COARSE similarity c with ONE fp16 product per element (fp16 has 11 significant bits: |c - s| <= eps for unit vectors, see
// C_EPS) and keeps, per query, every index vector that could still be in the exact top 4:
//   pass A  coarse top-4 values over a sample of the index (any subset's 4th best is a lower bound of the global 4th
//           best) -> theta = c4 - 2 eps;
//   pass B  coarse similarities of the whole index; rows with c >= theta are appended to the query's candidate list
//           (C_CAP entries; a handful for random data);
//   rescore exact fp32 similarity of every candidate (fp32 FMA chain over the raw vectors, x 1 / norm), top-4 with the
//           library's order (similarity descending, lower index first).
// Why this is exact: let R be the final top-4 (by the rescored similarity s') and T4 the coarse top-4 of the sample.
// For r in R: s'_r >= 4th largest s' overall >= min_{t in T4} s'_t >= c4 - eps, hence c_r >= s'_r - eps >= c4 - 2 eps = theta,
// so r is a candidate.  If any query collects more than C_CAP candidates (dense neighbourhoods), a flag makes the exact
// kernel run instead (it is always launched and exits at once when the flag is clear), so results never depend on the
// data distribution - only the speed does.
// =================================================================================================
constexpr int C_QT = 256, C_MT = 256, C_K = 64, C_STEPS = KD / C_K;            // 256 queries x 256 index vectors x K = 64 per step
constexpr int C_A_U4 = 4 * 8 * 64, C_X_U4 = 4 * 2 * C_QT;                      // one LDS buffer each: 32 KiB + 32 KiB
constexpr int C_LDS = 2 * (C_A_U4 + C_X_U4) * 16;                              // 128 KiB, double-buffered
constexpr int C_CAP = 256;                                                     // candidates per query before the exact fallback (theta comes from a sample, so lists run to a few dozen)
// |coarse - exact| for unit vectors: both operands rounded to fp16 (2^-11 relative each, 2^-25 absolute below the normal
// range), fp32 accumulation of 768 exact products (<= 768 * 2^-24), the rescoring's own rounding (< 1e-6):
// 2^-10 * 1.01 + 768 * 2^-25 + 768 * 2^-24 + 1e-6 < 1.06e-3; C_EPS leaves a margin.
constexpr float C_EPS = 1.25e-3f;
constexpr int KNN_COARSE_MIN = 4096;   // index size from which the two-stage search runs

struct Top4V {   // four largest values
    float v[4];
    __device__ __forceinline__ void init() { v[0] = v[1] = v[2] = v[3] = -INFINITY; }
    __device__ __forceinline__ void insert(float x) {
        if (!(x > v[3])) return;
        if (x > v[0]) { v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = x; }
        else if (x > v[1]) { v[3] = v[2]; v[2] = v[1]; v[1] = x; }
        else if (x > v[2]) { v[3] = v[2]; v[2] = x; }
        else v[3] = x;
    }
};

// grid = qtiles * nsplit; a workgroup owns 256 queries and walks `tiles_per_split` 256-vector index tiles (of the first
// `t2_cover` tiles).  8 waves as 2 (index halves) x 4 (query quarters), a wave owns 128 index vectors x 64 queries = 4 x 2
// MFMA tiles (v_mfma_f32_32x32x16_f16); both operands arrive as ready 16-byte fragments rows (the index's fp16 image,
// the queries' fp16 image), so staging is copies only: 8 loads + 8 ds_write_b128 per thread and K = 64 step, 32 MFMAs per
// wave and step.  MODE 0: coarse top-4 values per (split, query) -> c4v.  MODE 1: rows with c >= theta -> candidate lists.
// (per segment: qh / c4v / cnt / cand / candv / overflow come offset to the segment's first tile / column / flag, the segment's ncols
// queries are its own, c4v rows are cstride columns apart, unit = the workgroup's unit inside the segment)
template <bool F16, int MODE>
static __device__ __forceinline__ void knn_coarse_body(const float* __restrict__ blob, long Npad, int N, const uint4* __restrict__ qh,
                                                       int ncols, int cstride, int unit, int nsplit, int tiles_per_split, int t2_cover,
                                                       float* __restrict__ c4v, int ns_sample,
                                                       int* __restrict__ cnt, int* __restrict__ cand, float* __restrict__ candv,
                                                       int* __restrict__ overflow) {
    extern __shared__ __attribute__((aligned(16))) uint4 csmem[];
    uint4* As = csmem;
    uint4* Xs = csmem + 2 * C_A_U4;
    const int kind = F16 ? KIND_F16 : KIND_F32;
    const uint4* img = blob_img16(blob, kind, N, Npad);
    const float* inv = blob_inv(blob, kind, N, Npad);          // fp16 storage: the image holds the raw vectors

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int l31 = lane & 31, lh = lane >> 5;
    const int split = unit % nsplit;
    const int qtile = unit / nsplit;
    const int n0 = qtile * C_QT;
    const int mtiles = (int)(Npad >> 7);                         // 128-vector tiles of the image
    const int t_lo = split * tiles_per_split;
    const int t_hi = min(t2_cover, t_lo + tiles_per_split);
    const int G = (t_hi - t_lo) * C_STEPS;

    // staging: thread tid copies uint4 number tid + 512 i (i < 4) of the step's A block [k16][m-tile (8)][lane] and of its
    // X block [k16][8-channel half][query] - the LDS images are linear in exactly that order
    const uint4* xsrc = qh + (long)qtile * (STEPS * 2 * 256) + (tid & 511);
    u32x4 ar[4], xr[4];
    auto gload = [&](int g) __attribute__((always_inline)) {
        const int t2 = t_lo + g / C_STEPS, st = g - (g / C_STEPS) * C_STEPS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = wave + 8 * i, k16 = piece >> 3, mt8 = piece & 7;
            int t128 = 2 * t2 + (mt8 >> 2);
            t128 = t128 < mtiles ? t128 : mtiles - 1;                 // odd tile count: the missing half re-reads the last tile (its rows are >= N: ignored)
            ar[i] = *reinterpret_cast<const u32x4*>(img + (((long)t128 * STEPS + 4 * st + k16) * 4 + (mt8 & 3)) * 64 + lane);
            xr[i] = *reinterpret_cast<const u32x4*>(xsrc + (long)(4 * st + i) * 512);
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<u32x4*>(As + buf * C_A_U4 + tid + 512 * i) = ar[i];
            *reinterpret_cast<u32x4*>(Xs + buf * C_X_U4 + tid + 512 * i) = xr[i];
        }
    };

    Top4V top[2];
    top[0].init();
    top[1].init();
    float th[2] = {INFINITY, INFINITY};
    if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // theta = (fourth largest coarse similarity of pass A's sample: its splits' top-4 lists, c4v) - 2 eps
            const int n = n0 + wn * 64 + j * 32 + l31;
            if (n < ncols) {
                Top4V t4;
                t4.init();
                for (int sp = 0; sp < ns_sample; ++sp) {
                    const float4 v4 = *reinterpret_cast<const float4*>(c4v + ((long)sp * cstride + n) * 4);
                    t4.insert(v4.x);
                    t4.insert(v4.y);
                    t4.insert(v4.z);
                    t4.insert(v4.w);
                }
                th[j] = t4.v[3] - 2.f * C_EPS;
            }
        }
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (G > 0) {
        gload(0);
        lstore(0);
        gload(G > 1 ? 1 : 0);
        slab_barrier();
    }
    for (int g = 0; g < G; ++g) {
        const int cur = g & 1;
        // no branch around the staging: past the end it re-stages the last step into the idle buffer (harmless), and the
        // compiler is free to thread the stores and loads between this step's MFMAs
        lstore(cur ^ 1);
        gload(g + 2 < G ? g + 2 : G - 1);
        const uint4* as = As + cur * C_A_U4 + wm * (4 * 64) + lane;
        const uint4* xs = Xs + cur * C_X_U4 + lh * C_QT + wn * 64 + l31;
#pragma unroll
        for (int k16 = 0; k16 < 4; ++k16) {
            f16x8 af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = __builtin_bit_cast(f16x8, as[(k16 * 8 + i) * 64]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = __builtin_bit_cast(f16x8, xs[k16 * 2 * C_QT + j * 32]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        const int st = g - (g / C_STEPS) * C_STEPS;
        if (st == C_STEPS - 1) {
            const int t2 = t_lo + g / C_STEPS;
            const int m0 = t2 * C_MT;
            // fp16 storage: c = acc * inv[row].  max(acc, 0) * (largest inv of the tile) bounds c from above, so the
            // per-row inverse norm is only fetched for the few values that survive that bound.
            float imx = 1.f;
            if (F16) {
                const float* im = blob_invmax(blob, Npad);
                const int ta = 2 * t2 < mtiles ? 2 * t2 : mtiles - 1, tb = 2 * t2 + 1 < mtiles ? 2 * t2 + 1 : mtiles - 1;
                imx = fmaxf(im[ta], im[tb]);
            }
            // Per 32 x 32 accumulator tile: the largest of a lane's 16 values decides, for the whole wave at once (ballot), whether
            // any of them can matter; only then are the 16 walked one by one.  (The element-wise walk with its per-element
            // branches cost 11 000 cycles per 256 x 256 tile - 18 % of the pass - although a lane sees a hit every few dozen tiles.)
            const bool whole = m0 + C_MT <= N;                      // uniform: no row of this tile lies beyond the index
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float mx = acc[i][j][0];
                    bool anynan = false;
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[i][j][r]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) anynan |= acc[i][j][r] != acc[i][j][r];      // NaN orders as the maximum (nan_max, torch.topk): never skipped, in either pass
                    bool maybe;
                    if (MODE == 0) maybe = anynan || !((F16 ? fmaxf(mx, 0.f) * imx : mx) <= top[j].v[3]);
                    else maybe = anynan || (F16 ? fmaxf(mx, 0.f) * imx : mx) >= th[j];
                    if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = m0 + (wm * 4 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                            if (whole || row < N) {
                                const float a = acc[i][j][r];
                                if (MODE == 0) {
                                    if (!F16) {
                                        top[j].insert(nan_max(a));
                                    } else if (!(fmaxf(a, 0.f) * imx <= top[j].v[3])) {      // could enter the list (NaN passes)
                                        top[j].insert(nan_max(a * inv[row]));
                                    }
                                } else {
                                    bool hit;                                                  // a NaN similarity is a candidate (the exact kernel ranks it first)
                                    float cv = a;                                              // the coarse similarity the list keeps beside the row (rescore's second threshold)
                                    if (!F16) hit = !(a < th[j]);
                                    else {
                                        hit = a != a || (fmaxf(a, 0.f) * imx >= th[j]);
                                        if (hit) {
                                            cv = a * inv[row];
                                            hit = a != a || cv >= th[j];
                                        }
                                    }
                                    hit = hit && th[j] != INFINITY;                            // a padding column of the 256-query tile has no list (its threshold is +inf)
                                    if (hit) {
                                        const int n = n0 + wn * 64 + j * 32 + l31;
                                        const int pos = atomicAdd(&cnt[n], 1);
                                        if (pos < C_CAP) {
                                            cand[(long)n * C_CAP + pos] = row;
                                            candv[(long)n * C_CAP + pos] = cv;
                                        } else *overflow = 1;
                                    }
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        slab_barrier();
    }
    if (MODE == 1) return;

    // merge the 4 partial lists (wm x lh) of every query through LDS, write this split's four largest coarse values
    float (*mv)[16] = reinterpret_cast<float (*)[16]>(csmem);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wn * 64 + j * 32 + l31;
        const int slot = (wm * 2 + lh) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) mv[q][slot + e] = top[j].v[e];
    }
    __syncthreads();
    if (tid < C_QT) {
        Top4V t4;
        t4.init();
        for (int e = 0; e < 16; ++e) t4.insert(mv[tid][e]);
        const int n = n0 + tid;
        if (n < ncols) {
            const long o = ((long)split * cstride + n) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) c4v[o + e] = t4.v[e];
        }
    }
}

// The blob's kind lives in device memory (its header): one launch, the workgroup branches to the storage's instantiation of the body
// (both fit the 256 registers a wave has at one 128 KiB workgroup per CU; two launches cost an empty 4.6 us one per pass).
// grid = the pass's units of every two-stage segment (MODE 0: pass A, 1: pass B); flags = the segments' overflow flags
template <int MODE>
static __global__ __launch_bounds__(512) void knn_coarse_kernel(const KnnSegs segs, const uint4* __restrict__ qh, int cstride,
                                                                float* __restrict__ c4v, int* __restrict__ cnt, int* __restrict__ cand,
                                                                float* __restrict__ candv, int* __restrict__ flags) {
    const int si = seg_find<MODE>(segs, blockIdx.x);
    const KnnSeg g = seg_get(segs, si);
    const int unit = blockIdx.x - g.u[MODE];
    const int nsplit = MODE ? g.nsB : g.nsA, tps = MODE ? g.tpsB : g.tpsA, cover = MODE ? g.t2 : g.sample;
    const uint4* q = qh + (long)g.u[3] * (STEPS * 2 * 256);
    float* c4 = c4v + (long)g.col0 * 4;
    int* ct = cnt + g.col0;
    int* cd = cand + (long)g.col0 * C_CAP;
    float* cdv = candv + (long)g.col0 * C_CAP;
    if (blob_kind(g.blob) == KIND_F16)
        knn_coarse_body<true, MODE>(g.blob, blob_npad(g.N), g.N, q, g.ncols, cstride, unit, nsplit, tps, cover, c4, g.nsA, ct, cd, cdv, flags + si);
    else
        knn_coarse_body<false, MODE>(g.blob, blob_npad(g.N), g.N, q, g.ncols, cstride, unit, nsplit, tps, cover, c4, g.nsA, ct, cd, cdv, flags + si);
}

// One wavefront per query: exact similarity of every candidate = (fp32 FMA chain of q_hat against the raw vector, lanes
// along k, fixed-order shuffle reduction) * (1 / norm); top-4 in the library's order -> rv / ri [ncols][4].
// A query with fewer than four candidates had non-finite coarse similarities (NaN / Inf samples upstream): rows 0..3 with
// similarity +inf, what the exact kernel's NaN-as-maximum rule selects.
// (the query's blob: its segment's, col2seg; a query of a segment that searches with the exact kernel only has no list: the wave leaves)
static __global__ __launch_bounds__(256) void knn_rescore_kernel(const KnnSegs segs, const int* __restrict__ col2seg, const float* __restrict__ qn,
                                                                 int ncols, int T, const int* __restrict__ cnt, const int* __restrict__ cand,
                                                                 const float* __restrict__ candv, float* __restrict__ rv, int* __restrict__ ri) {
    constexpr int RG = 4;                           // candidates scored together
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= ncols) return;
    const KnnSeg g = seg_get(segs, col2seg ? __builtin_amdgcn_readfirstlane(col2seg[n]) : 0);
    if (!g.two) return;
    const float* __restrict__ blob = g.blob;
    const int N = g.N;
    const long Npad = blob_npad(g.N);
    const int kind = blob_kind(blob);
    const float* inv = blob_inv(blob, kind, N, Npad);
    const int b = n / T, t = n - b * T;
    const float* qp = qn + (long)b * KD * T + t;
    // the list's rows and coarse values are requested together with its length (all C_CAP entries exist; those past the end are masked
    // below): one round trip instead of three in a kernel that is a chain of them (WAIT 0.64, ACTIVE 0.09)
    int rowl[C_CAP / 64];
    float cvl[C_CAP / 64];
#pragma unroll
    for (int c = 0; c < C_CAP / 64; ++c) {
        rowl[c] = cand[(long)n * C_CAP + 64 * c + lane];
        cvl[c] = candv[(long)n * C_CAP + 64 * c + lane];
    }
    const int nc = min(cnt[n], C_CAP);
    Top4 t4;
    t4.init();
    // Second threshold.  Pass B's was cut from a SAMPLE of the index, so a list holds the few dozen rows above the sample's fourth best.
    // The list itself knows better: it contains every row with coarse >= theta, hence the four largest coarse values of the WHOLE index;
    // with c4 the fourth of them, four rows have exact >= c4 - eps, so a row of the exact top four has exact >= c4 - eps and coarse
    // >= c4 - 2 eps.  Only those are scored (a handful): the 3 KB gather per candidate was the kernel's whole cost.  NaN coarse values are
    // left out of the ranking (a lower c4: more rows kept) and always scored.
    float th2;
    {
        float rk[C_CAP / 64];
#pragma unroll
        for (int c = 0; c < C_CAP / 64; ++c) {
            if (!(64 * c + lane < nc)) {
                cvl[c] = -INFINITY;
                rowl[c] = 0;
            }
            rk[c] = cvl[c] == cvl[c] ? cvl[c] : -INFINITY;
        }
        float wm = -INFINITY;
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            float lm = rk[0];
#pragma unroll
            for (int c = 1; c < C_CAP / 64; ++c) lm = fmaxf(lm, rk[c]);
            wm = lm;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
            const unsigned long long who = __builtin_amdgcn_ballot_w64(lm == wm);
            if (lane == __builtin_ctzll(who)) {       // one instance leaves the ranking (equal values count once each)
                bool done = false;
#pragma unroll
                for (int c = 0; c < C_CAP / 64; ++c)
                    if (!done && rk[c] == wm) {
                        rk[c] = -INFINITY;
                        done = true;
                    }
            }
        }
        th2 = wm - 2.f * C_EPS;                       // (fewer than four finite values: -inf, everything is scored)
    }
    static_assert(C_CAP == 256, "four 64-entry chunks");
    if (kind == KIND_F16) {
        // the fp16 image keeps a vector as 96 16-byte segments (8 consecutive channels each, 4 KiB apart): lane l reads
        // segments l and 64 + l (l < 32) with one 16-byte load each instead of twelve 2-byte loads
        const uint4* img = blob_img16(blob, kind, N, Npad);
        float qs[2][8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int seg = lane + 64 * h;
                qs[h][j] = seg < 96 ? qp[(long)(8 * seg + j) * T] : 0.f;
            }
        // The candidate list is read 64 entries at a time (one coalesced load, the row numbers then come out of a register by lane
        // broadcast) and the candidates are scored four at a time: their loads are in flight together instead of one list entry -> one
        // vector -> one reduction after the other (the chain was 2 - 3 us per candidate with nothing else to issue: ACTIVE 0.06).
        for (int base = 0, ch = 0; base < nc; base += 64, ++ch) {
            const int mine = ch == 0 ? rowl[0] : (ch == 1 ? rowl[1] : (ch == 2 ? rowl[2] : rowl[3]));
            const float cvv = ch == 0 ? cvl[0] : (ch == 1 ? cvl[1] : (ch == 2 ? cvl[2] : cvl[3]));
            unsigned long long mask = __builtin_amdgcn_ballot_w64(base + lane < nc && !(cvv < th2));      // the entries that pass (NaN does)
            while (mask) {
                int row[RG];
                bool live[RG];
                float d[RG], iv[RG];
                u32x4 w[RG][2];
                int pos = 0;
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    live[g] = mask != 0ull;
                    if (live[g]) {
                        pos = __builtin_ctzll(mask);
                        mask &= mask - 1;
                    }
                    row[g] = __shfl(mine, pos);      // (past the end: the last one again, not inserted)
                    const long rbase = ((long)(row[g] >> 7) * STEPS * 4 + ((row[g] & 127) >> 5)) * 64 + (row[g] & 31);     // + (step * 4) * 64 + half * 32
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int seg = lane + 64 * h < 96 ? lane + 64 * h : 0;
                        w[g][h] = *reinterpret_cast<const u32x4*>(img + rbase + (long)(seg >> 1) * 256 + (seg & 1) * 32);
                    }
                    iv[g] = inv[row[g]];
                }
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    d[g] = 0.f;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if (lane + 64 * h < 96) {
                            const f16x8 hv = __builtin_bit_cast(f16x8, w[g][h]);
#pragma unroll
                            for (int j = 0; j < 8; ++j) d[g] = fmaf(qs[h][j], (float)hv[j], d[g]);
                        }
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                    for (int g = 0; g < RG; ++g) d[g] += __shfl_xor(d[g], o);
#pragma unroll
                for (int g = 0; g < RG; ++g)
                    if (live[g]) t4.insert(nan_max(d[g] * iv[g]), row[g]);
            }
        }
    } else {
        float qv[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) qv[u] = qp[(long)(lane + 64 * u) * T];
        const float* rows = blob_rows(blob);
        for (int base = 0, ch = 0; base < nc; base += 64, ++ch) {
            const int mine = ch == 0 ? rowl[0] : (ch == 1 ? rowl[1] : (ch == 2 ? rowl[2] : rowl[3]));
            const float cvv = ch == 0 ? cvl[0] : (ch == 1 ? cvl[1] : (ch == 2 ? cvl[2] : cvl[3]));
            unsigned long long mask = __builtin_amdgcn_ballot_w64(base + lane < nc && !(cvv < th2));      // the entries that pass (NaN does)
            while (mask) {
                int row[RG];
                bool live[RG];
                float d[RG], iv[RG], xv[RG][12];
                int pos = 0;
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    live[g] = mask != 0ull;
                    if (live[g]) {
                        pos = __builtin_ctzll(mask);
                        mask &= mask - 1;
                    }
                    row[g] = __shfl(mine, pos);      // (past the end: the last one again, not inserted)
                    const float* rp = rows + (long)row[g] * KD + lane;
#pragma unroll
                    for (int u = 0; u < 12; ++u) xv[g][u] = rp[64 * u];
                    iv[g] = inv[row[g]];
                }
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    d[g] = 0.f;
#pragma unroll
                    for (int u = 0; u < 12; ++u) d[g] = fmaf(qv[u], xv[g][u], d[g]);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                    for (int g = 0; g < RG; ++g) d[g] += __shfl_xor(d[g], o);
#pragma unroll
                for (int g = 0; g < RG; ++g)
                    if (live[g]) t4.insert(nan_max(d[g] * iv[g]), row[g]);
            }
        }
    }
    if (nc < 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t4.v[e] = INFINITY;
            t4.i[e] = e;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            rv[(long)n * 4 + e] = t4.v[e];
            ri[(long)n * 4 + e] = t4.i[e];
        }
    }
}

// ---- host plan ------------------------------------------------------------------------------------------------------------
// splits of one pass over `cover` index tiles: about `blocks` workgroups over the call's `qtiles` query tiles
static void split_plan(int blocks, int qtiles, int cover, int* ns, int* tps) {
    int n = (blocks + qtiles - 1) / qtiles;
    if (n > cover) n = cover;
    if (n < 1) n = 1;
    *tps = (cover + n - 1) / n;
    *ns = (cover + *tps - 1) / *tps;
}

// Segments from the callers' runs (in column order): adjacent runs of the same blob merge.  Every split count follows from the call's
// total query tiles, so a one-segment call plans exactly what the single-index search always planned.
int knn_call_plan(tvc_ctx* ctx, const KnnSegIn* in, int nin, int ncols, KnnCall* c) {
    static_assert(KNN_QT == C_QT, "one query tiling for both searches");
    c->ncols = ncols;
    for (int i = 0; i < nin; ++i) {
        if (in[i].N > 0x7fffff00L) return fail(ctx, TVC_ERR_ARG, "index too large");
        if (in[i].ncols <= 0) continue;
        if (!c->seg.empty() && c->seg.back().blob == in[i].blob && c->seg.back().col0 + c->seg.back().ncols == in[i].col0) {
            c->seg.back().ncols += in[i].ncols;
            continue;
        }
        KnnSeg g{};
        g.blob = in[i].blob;
        g.N = (int)in[i].N;
        g.col0 = in[i].col0;
        g.ncols = in[i].ncols;
        c->seg.push_back(g);
    }
    if (c->seg.empty()) return fail(ctx, TVC_ERR_ARG, "knn: no query columns");
    for (auto& g : c->seg) c->cq += (g.ncols + C_QT - 1) / C_QT;
    int mt_max = 1;
    int tile = 0;
    for (auto& g : c->seg) {
        const long Npad = blob_npad(g.N);
        const int mtiles = (int)(Npad / 128);
        const int qt = (g.ncols + C_QT - 1) / C_QT;
        mt_max = mtiles > mt_max ? mtiles : mt_max;
        g.two = g.N >= KNN_COARSE_MIN;
        g.t2 = (int)((Npad + C_MT - 1) / C_MT);          // 256-vector tiles
        // pass A: an eighth of the index, at least 1280 vectors.  (A smaller sample lowers the threshold: longer lists - whose rows the
        // rescoring wave's own threshold then drops unscored - and, past C_CAP entries, the exact fallback: a sixteenth sends the
        // 100 000-vector index there.  Five tiles x 50 query tiles of the bench batch are one round of the chip.)
        g.sample = g.t2 / 8 < 5 ? 5 : g.t2 / 8;
        if (g.sample > g.t2) g.sample = g.t2;
        // coarse passes: ~3 workgroups per CU's worth of work units (one resident workgroup per CU: 128 KiB of LDS)
        split_plan(768, c->cq, g.sample, &g.nsA, &g.tpsA);
        split_plan(768, c->cq, g.t2, &g.nsB, &g.tpsB);
        split_plan(KNN_BLOCKS, c->cq, mtiles, &g.nsE, &g.tpsE);
        g.u[0] = c->units[0];
        g.u[1] = c->units[1];
        g.u[2] = c->units[2];
        g.u[3] = tile;
        if (g.two) {
            c->units[0] += qt * g.nsA;
            c->units[1] += qt * g.nsB;
            c->two = true;
        }
        c->units[2] += qt * g.nsE;
        tile += qt;
    }
    // several segments: a bound that no split of the columns into segments exceeds (the workspace query of the multi-index calls plans
    // every row as its own segment, a call whose rows share blobs has fewer)
    if (c->seg.size() == 1) c->ns_cv = c->seg[0].nsE;
    else {
        const int cq_min = (ncols + C_QT - 1) / C_QT;
        c->ns_cv = (KNN_BLOCKS + cq_min - 1) / cq_min;
        c->ns_cv = c->ns_cv < mt_max ? c->ns_cv : mt_max;
    }
    return 0;
}

template <int MODE>
static int coarse_launch(tvc_ctx* ctx, hipStream_t s, const KnnCall& c, const KnnLists& L, const uint4* qh, float* c4v, int* cnt, int* cand, float* candv) {
    TVC_CHECK(lds_optin<knn_coarse_kernel<MODE>>(ctx, C_LDS, "knn coarse"));
    hipLaunchKernelGGL((knn_coarse_kernel<MODE>), dim3((unsigned)c.units[MODE]), dim3(512), C_LDS, s, L.segs, qh, c.ncols, c4v, cnt, cand, candv, L.flag);
    return 0;
}

// workspace of the two-stage search for `qtiles` 256-query tiles (also the worst case over index sizes)
static int coarse_max_nsplit(int qtiles) { return (768 + qtiles - 1) / qtiles; }

// query normalisation + the per-query top-4 lists; shared by the whole-index match and the index-sharded variant.
// (The blob's kind lives in device memory - its header -, so the host cannot pick an instantiation: the kernels branch on it.)
// The segment table of a several-segment call is uploaded as kernel arguments (ragged.h upload_ints): asynchronous, capturable.
// (Bsrc: rows of src behind the B rows of queries - query_normalize_kernel; 0 = B)
int knn_candidates(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const KnnCall& c, int B, int T, KnnLists* L, int Bsrc) {
    const int nseg = (int)c.seg.size();
    float* qn = ws.get<float>((size_t)B * KD * T);
    L->cv = ws.get<float>((size_t)c.ns_cv * c.ncols * 4);
    L->ci = ws.get<int>((size_t)c.ns_cv * c.ncols * 4);
    int* dtab = nseg > 1 ? ws.get<int>((size_t)nseg * sizeof(KnnSeg) / sizeof(int)) : nullptr;
    L->col2seg = nseg > 1 ? ws.get<int>((size_t)c.ncols) : nullptr;
    uint4* qh = nullptr;
    float* c4v = nullptr;
    int *cnt = nullptr, *cand = nullptr;
    float* candv = nullptr;
    if (c.two) {
        qh = ws.get<uint4>((size_t)c.cq * STEPS * 2 * 256);
        c4v = ws.get<float>((size_t)coarse_max_nsplit((c.ncols + C_QT - 1) / C_QT) * c.ncols * 4);
        cnt = ws.get<int>((size_t)c.ncols);
        cand = ws.get<int>((size_t)c.ncols * C_CAP);
        candv = ws.get<float>((size_t)c.ncols * C_CAP);
        L->rv = ws.get<float>((size_t)c.ncols * 4);
        L->ri = ws.get<int>((size_t)c.ncols * 4);
        L->flag = ws.get<int>((size_t)(nseg > 64 ? nseg : 64));
    }
    if (ws.dry) return 0;
    L->segs.n = nseg;
    L->segs.one = c.seg[0];
    L->segs.d = reinterpret_cast<const KnnSeg*>(dtab);
    if (dtab) {
        std::vector<int> words((size_t)nseg * sizeof(KnnSeg) / sizeof(int));
        std::memcpy(words.data(), c.seg.data(), words.size() * sizeof(int));
        TVC_CHECK(upload_ints(ctx, s, words, dtab));
    }
    const int nblk = c.two ? c.cq * 4 : (c.ncols + 63) / 64;      // the fp16 query image is written for whole 256-query tiles
    hipLaunchKernelGGL(query_normalize_kernel, dim3(nblk), dim3(QN_WAVES * 64), 0, s, src, qn, B, Bsrc > 0 ? Bsrc : B, T, qh, cnt, L->flag, L->segs, L->col2seg);
    if (c.two) {
        ProfScope ps(ctx, s, ws, "knn.coarse+rescore");
        TVC_CHECK((coarse_launch<0>(ctx, s, c, *L, qh, c4v, cnt, cand, candv)));
        TVC_CHECK((coarse_launch<1>(ctx, s, c, *L, qh, c4v, cnt, cand, candv)));
        hipLaunchKernelGGL(knn_rescore_kernel, dim3((c.ncols + 3) / 4), dim3(256), 0, s, L->segs, (const int*)L->col2seg, qn, c.ncols, T, cnt, cand, candv, L->rv, L->ri);
    }
    ProfScope ps(ctx, s, ws, "knn.exact");       // ~0 when the two-stage search succeeded (the kernel exits on the flag)
    hipLaunchKernelGGL(knn_topk_split_kernel, dim3((unsigned)c.units[2]), dim3(512), 0, s, L->segs, qn, c.ncols, T, L->cv, L->ci, (const int*)L->flag);
    return 0;
}

}  // namespace tvc
