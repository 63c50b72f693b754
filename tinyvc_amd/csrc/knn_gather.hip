// From the search's top-4 lists (knn.hip, knn_search.h) to results: the merge + gather of the whole-index match (one index, one per
// row, a weighted blend; each also in its alpha form, which keeps a share of the source), the index-sharded route's three steps (merge, slot
// gather, finish) and the |max| bounds of `matched`.
// Every route averages the four rows with mean4 and stores through store_tile_along_t: equal lists give equal bits on all of them.  The
// weighted forms of the two merge + gather kernels (WeightIn) put weighted_mean4 - the k nearest, weighted by their similarities - in its place;
// their joined forms (JoinIn) form those weights around the neighbour a path over the utterance chose (the merge + affinity and path kernels).
#include <type_traits>

#include "knn_blob.h"
#include "knn_search.h"
#include "tvc_common.h"

namespace tvc {

// ---- what the kernels below share ----------------------------------------------------------------------------------------------
// the `nsplit` x 4 list entries of query column `col` of a search over `stride` columns -> one top-4 (sentinels as they are)
__device__ __forceinline__ Top4 merge_lists(const float* __restrict__ cv, const int* __restrict__ ci, int nsplit, long stride, long col) {
    Top4 t4;
    t4.init();
    for (int s = 0; s < nsplit; ++s) {
        const long o = (s * stride + col) * 4;
        for (int e = 0; e < 4; ++e) t4.insert(cv[o + e], ci[o + e]);
    }
    return t4;
}
// sel[4] = the rows column `col` of segment g (number si) gathers: its rescored lists (one "split") where the segment's two-stage search
// succeeded, else the exact kernel's g.nsE splits, merged; never a sentinel; also written to idx_out[col] (nullable).  A column that is not
// live (past the end of the call) reads nothing and selects row 0.  sims (nullable, the weighted forms): the four similarities as the merged
// list holds them (NaN arrived as +inf, a sentinel's is -inf; a column that is not live: zeros), also written to sims_out[col] (nullable).
__device__ __forceinline__ void merged_top4(const KnnSeg& g, int si, const int* __restrict__ flags, const float* __restrict__ cand_v,
                                            const int* __restrict__ cand_i, const float* __restrict__ rv, const int* __restrict__ ri, long stride,
                                            long col, bool live, int64_t* __restrict__ idx_out, int* sel, float* sims = nullptr,
                                            float* __restrict__ sims_out = nullptr) {
    const bool rescored = g.two && flags[si] == 0;
    Top4 t4;
    t4.init();
    if (live) {
        t4 = merge_lists(rescored ? rv : cand_v, rescored ? ri : cand_i, rescored ? 1 : g.nsE, stride, col);
        for (int e = 0; e < 4; ++e) t4.i[e] = (unsigned)t4.i[e] < (unsigned)g.N ? t4.i[e] : 0;   // never gather through a sentinel
        if (idx_out)
            for (int e = 0; e < 4; ++e) idx_out[col * 4 + e] = (int64_t)t4.i[e];
        if (sims_out)
            for (int e = 0; e < 4; ++e) sims_out[col * 4 + e] = t4.v[e];
    }
    for (int e = 0; e < 4; ++e) sel[e] = live ? t4.i[e] : 0;
    if (sims)
        for (int e = 0; e < 4; ++e) sims[e] = live ? t4.v[e] : 0.f;
}
// r[qq][u][e] = channel k + 64 u of row sel[q][e] of query q = q0 + 4 qq's blob (src(q)): four queries' 48 loads in flight per lane (one
// query at a time was eight serial round trips per wave and chunk - 48 us per launch whatever the batch, a chain of latencies)
struct RowSrc { const float* blob; int kind, N; };
template <class Src>
__device__ __forceinline__ void gather4x3(float (&r)[4][3][4], int q0, Src src, const int (*sel)[4], int k) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        const int q = q0 + 4 * qq;
        const RowSrc b = src(q);
        const long Npad = blob_npad(b.N);
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) r[qq][u][e] = blob_row_value(b.blob, b.kind, b.N, Npad, sel[q][e], k + 64 * u);
    }
}
// the mean of the four rows, in the one order every route keeps: (((r0 + r1) + r2) + r3) * 0.25
__device__ __forceinline__ float mean4(float r0, float r1, float r2, float r3) {
    return __fadd_rn(__fadd_rn(__fadd_rn(r0, r1), r2), r3) * 0.25f;
}
// tile[q][kk] = channel kc + kk of column n0 + q -> out[b][kc + kk][t]: lanes run along the 32 queries (time), 8 k-rows per pass
__device__ __forceinline__ void store_tile_along_t(const float (&tile)[32][193], float* __restrict__ out, int n0, int ncols, int T, int kc) {
    for (int kk = threadIdx.x >> 5; kk < 192; kk += 8) {
        const int q = threadIdx.x & 31;
        const int n = n0 + q;
        if (n < ncols) {
            const int b = n / T, t = n - b * T;
            out[((long)b * KD + kc + kk) * T + t] = tile[q][kk];
        }
    }
}

// The alpha forms (tvc_*_alpha_f32) keep a share of the source's own features: a = alpha[row of the column] (the caller's DEVICE array, read
// here: a captured graph replays with whatever it holds then), and every element leaves as
//   out = mu * (1 - a) + src * a      (__fsub_rn, two __fmul_rn, __fadd_rn: torch's eager mu * (1 - a_t) + src * a_t on fp32 tensors)
// with mu what the alpha-less kernel stores there.  src has out's layout, so it is read in the store phase at the address of the store (lanes
// along t); a tile's 32 columns may straddle rows with different alpha.  The row of a column: its batch row, or rowmap[col2b[column]] in a
// ragged batch (ragged.h) - the blend kernel's weight row.
struct AlphaIn {
    const float* alpha;      // [rows]
    const float* src;        // [B][768][T]: the queries that were searched (another buffer than `out`)
    const int* col2b;        // ragged batch: column -> utterance, utterance -> caller's row; else nullptr
    const int* rowmap;
};
__device__ __forceinline__ float alpha_of_column(const AlphaIn& al, int nc, int T) { return al.alpha[al.col2b ? al.rowmap[al.col2b[nc]] : nc / T]; }
// The protect forms (tvc_*_protect_f32) give every query COLUMN its own share: a = share[column], the a_t that frame_share_kernel below wrote
// from the call's f0 in front of the search.  The same store phase, and no col2b / rowmap lookup: one more instantiation of the two kernels.
struct ShareIn {
    const float* share;      // [ncols]
    const float* src;        // [B][768][T], as AlphaIn's
};
__device__ __forceinline__ float alpha_of_column(const ShareIn& sh, int nc, int) { return sh.share[nc]; }
// The weighted forms (tvc_*weighted*_f32; the definition is in include/tinyvc_hip.h) take the mean over the k nearest of the four rows, each
// weighted by how close its similarity lies to the nearest's: k = neighbours[row] clamped to 1 .. 4, the width = width[row] in cosine units,
// both the caller's DEVICE arrays, read here (a captured graph replays with whatever they hold then).  Either may be null: 4, +inf.  The row
// of a column is alpha's.  sims_out (nullable): the merged lists' similarities, beside idx_out.
struct WeightIn {
    const int* neighbours;   // [rows]
    const float* width;      // [rows]
    const int* col2b;        // ragged batch: column -> utterance, utterance -> caller's row; else nullptr
    const int* rowmap;
    float* sims_out;         // [M][B][T][4]
};
// a weighted instantiation's one more argument: the weights' inputs and, behind them, the store form's (Mix: AlphaIn, ShareIn or NoMix)
struct NoMix {};
template <class Mix>
struct Weighted {
    WeightIn w;
    Mix mix;
};
// The joined forms (tvc_*joined*_f32; the definition is in include/tinyvc_hip.h) are the weighted forms with the weights formed around an ANCHOR
// per column instead of around neighbour 0: the path kernel below chose it, over the utterance as a whole.  The merge + affinity kernel left
// the merged lists in workspace, so the merge threads read them there instead of merging again.
struct JoinIn {
    const int* sel;          // [M * ncols][4] the merged rows (never a sentinel)
    const float* sims;       // [M * ncols][4] their similarities, as sims_out
    const int* anchor;       // [M * ncols] the path's neighbour, 0 .. k - 1
};
template <class Mix>
struct Joined {
    WeightIn w;
    JoinIn j;
    Mix mix;
};
template <class... A> struct Forms { static constexpr bool weighted = false, joined = false, mixed = sizeof...(A) > 0; };
template <class Mix> struct Forms<Weighted<Mix>> { static constexpr bool weighted = true, joined = false, mixed = !std::is_same<Mix, NoMix>::value; };
template <class Mix> struct Forms<Joined<Mix>> { static constexpr bool weighted = true, joined = true, mixed = !std::is_same<Mix, NoMix>::value; };
template <class AI> __device__ __forceinline__ const AI& mix_of(const AI& al) { return al; }
template <class Mix> __device__ __forceinline__ const Mix& mix_of(const Weighted<Mix>& x) { return x.mix; }
template <class Mix> __device__ __forceinline__ const Mix& mix_of(const Joined<Mix>& x) { return x.mix; }
// w[0 .. 3] = the four weights of a column and w[4] = their sum W from its merged similarities s[0] >= ... >= s[3]: w_0 = 1, w_e = 1 - (s_0 - s_e) /
// width clamped to [0, 1] for e < k - and 1 wherever that quotient is not a positive number (NaN, a tie under width 0, a negative width) -, 0 from
// k on.  Every operation is rounded on its own; W >= 1 whatever the two arrays hold.
__device__ __forceinline__ void match_weights(const WeightIn& wi, int row, const float* s, float* w) {
    int k = wi.neighbours ? wi.neighbours[row] : 4;
    k = k < 1 ? 1 : (k > 4 ? 4 : k);
    const float width = wi.width ? wi.width[row] : INFINITY;
    w[0] = 1.f;
    for (int e = 1; e < 4; ++e) {
        const float t = __fdiv_rn(__fsub_rn(s[0], s[e]), width);
        w[e] = e < k ? (t > 0.f ? fmaxf(0.f, __fsub_rn(1.f, t)) : 1.f) : 0.f;
    }
    w[4] = __fadd_rn(__fadd_rn(__fadd_rn(w[0], w[1]), w[2]), w[3]);
}
// the weighted mean of the four rows: r0, then + w_e * r_e in order where w_e != 0 (a neighbour of weight 0 takes no part, whatever it holds),
// product and sum rounded separately, over W.  w = {1, 1, 1, 1, 4} is mean4 bit for bit (x / 4 == x * 0.25f), {1, 0, 0, 0, 1} r0's own bits.
__device__ __forceinline__ float weighted_mean4(float r0, float r1, float r2, float r3, const float* w) {
    float acc = r0;
    acc = w[1] != 0.f ? __fadd_rn(acc, __fmul_rn(w[1], r1)) : acc;
    acc = w[2] != 0.f ? __fadd_rn(acc, __fmul_rn(w[2], r2)) : acc;
    acc = w[3] != 0.f ? __fadd_rn(acc, __fmul_rn(w[3], r3)) : acc;
    return __fdiv_rn(acc, w[4]);
}
// the joined forms' merge: column `col`'s merged rows and similarities as the merge + affinity kernel stored them -> sel[4], s[4]; returns the
// path's anchor.  `& 3`: whatever the workspace held, the anchor indexes the four.  A column that is not live: row 0, zeros, anchor 0.
__device__ __forceinline__ int joined_top4(const JoinIn& ji, long col, bool live, int* sel, float* s) {
    for (int e = 0; e < 4; ++e) {
        sel[e] = live ? ji.sel[col * 4 + e] : 0;
        s[e] = live ? ji.sims[col * 4 + e] : 0.f;
    }
    return live ? ji.anchor[col] & 3 : 0;
}
// match_weights around the anchor p: w_p = 1, w_e = 1 - |s_p - s_e| / width clamped to [0, 1] for e < k, e != p - and 1 wherever the quotient is
// not a positive number -, 0 from k on; w[4] = W >= 1.  p = 0 is match_weights bit for bit (s_0 - s_e >= 0 in a sorted list).
__device__ __forceinline__ void join_weights(const WeightIn& wi, int row, const float* s, int p, float* w) {
    int k = wi.neighbours ? wi.neighbours[row] : 4;
    k = k < 1 ? 1 : (k > 4 ? 4 : k);
    const float width = wi.width ? wi.width[row] : INFINITY;
    const float sp = p == 0 ? s[0] : (p == 1 ? s[1] : (p == 2 ? s[2] : s[3]));
    for (int e = 0; e < 4; ++e) {
        const float t = __fdiv_rn(fabsf(__fsub_rn(sp, s[e])), width);
        w[e] = e == p ? 1.f : (e < k ? (t > 0.f ? fmaxf(0.f, __fsub_rn(1.f, t)) : 1.f) : 0.f);
    }
    w[4] = __fadd_rn(__fadd_rn(__fadd_rn(w[0], w[1]), w[2]), w[3]);
}
// the mean around an anchor: the terms w_e * r_e with w_e != 0 in ascending e, the first of them starting the sum (neighbour 0 may weigh
// nothing here), product and sum rounded separately, over W.  w[0] == 1 is weighted_mean4 bit for bit (1 * r0 == r0).
__device__ __forceinline__ float joined_mean4(float r0, float r1, float r2, float r3, const float* w) {
    const float r[4] = {r0, r1, r2, r3};
    float acc = 0.f;
    bool started = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float term = __fmul_rn(w[e], r[e]);
        acc = w[e] != 0.f ? (started ? __fadd_rn(acc, term) : term) : acc;
        started = started || w[e] != 0.f;
    }
    return __fdiv_rn(acc, w[4]);
}
// store_tile_along_t with the source's share a of this thread's column mixed in (AI: AlphaIn or ShareIn)
template <class AI>
__device__ __forceinline__ void store_tile_along_t_alpha(const float (&tile)[32][193], float* __restrict__ out, const AI& al, float a, int n0,
                                                         int ncols, int T, int kc) {
    const float* __restrict__ src = al.src;
    const float keep = __fsub_rn(1.f, a);
    for (int kk = threadIdx.x >> 5; kk < 192; kk += 8) {
        const int q = threadIdx.x & 31;
        const int n = n0 + q;
        if (n < ncols) {
            const int b = n / T, t = n - b * T;
            const long o = ((long)b * KD + kc + kk) * T + t;
            out[o] = __fadd_rn(__fmul_rn(tile[q][kk], keep), __fmul_rn(src[o], a));
        }
    }
}

// One workgroup = 32 consecutive query columns: merge split candidates -> top-4, write indices,
// gather the 4 raw rows per query (coalesced along the feature axis), average, and write
// out[b][k][t] through an LDS transpose so stores run along t.  Every query takes its segment's blob and lists (col2seg: several
// segments; the 32 columns may straddle a segment boundary).  MULTI = false: one segment, whose blob the gather reads as a uniform value.
// A... = AlphaIn: the alpha form (an instantiation with one more argument), ShareIn: the protect form; empty: the kernel as it has always been,
// argument for argument.  Weighted<Mix>: the weighted form of any of the three - the merge threads leave each column's weights in LDS beside
// sel, and the gather, its loads as they are, divides the weighted sum by theirs.
template <bool MULTI, class... A>
static __global__ __launch_bounds__(256) void knn_merge_gather_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                                      const KnnSegs segs, const int* __restrict__ col2seg, int ncols, int T,
                                                                      float* __restrict__ out, int64_t* __restrict__ idx_out,
                                                                      const float* __restrict__ rv, const int* __restrict__ ri,
                                                                      const int* __restrict__ flags, const A... al) {
    constexpr bool ALPHA = Forms<A...>::mixed, WEIGHTED = Forms<A...>::weighted, JOINED = Forms<A...>::joined;
    __shared__ int sel[32][4];
    __shared__ float tile[32][193];
    __shared__ const float* sblob[32];
    __shared__ int skind[32], sN[32];
    __shared__ float sw[WEIGHTED ? 32 : 1][5];      // the weighted forms: a column's four weights and their sum
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * 32;
    float a = 0.f;
    if constexpr (ALPHA) {      // this thread's column in the store phase (a column past the end reads the last column's row: never stored)
        const int n = n0 + (tid & 31);
        a = alpha_of_column(mix_of(al...), n < ncols ? n : ncols - 1, T);
    }
    if (tid < 32) {
        const int n = n0 + tid;
        const int nc = n < ncols ? n : ncols - 1;      // (a column past the end gathers row 0 of the last column's blob: never stored)
        const int si = MULTI ? col2seg[nc] : 0;
        const KnnSeg g = seg_get(segs, si);
        if constexpr (JOINED) {      // the lists were merged (and idx_out / sims_out written) by the merge + affinity kernel; the weights form around the path's anchor
            const WeightIn& wi = (al.w, ...);
            float sims[4];
            const int p = joined_top4((al.j, ...), n, n < ncols, sel[tid], sims);
            join_weights(wi, wi.col2b ? wi.rowmap[wi.col2b[nc]] : nc / T, sims, p, sw[tid]);
        } else if constexpr (WEIGHTED) {
            const WeightIn& wi = (al.w, ...);
            float sims[4];
            merged_top4(g, si, flags, cand_v, cand_i, rv, ri, ncols, n, n < ncols, idx_out, sel[tid], sims, wi.sims_out);
            match_weights(wi, wi.col2b ? wi.rowmap[wi.col2b[nc]] : nc / T, sims, sw[tid]);
        } else {
            merged_top4(g, si, flags, cand_v, cand_i, rv, ri, ncols, n, n < ncols, idx_out, sel[tid]);
        }
        if (MULTI) {
            sblob[tid] = g.blob;
            skind[tid] = blob_kind(g.blob);
            sN[tid] = g.N;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const RowSrc one{segs.one.blob, MULTI ? 0 : blob_kind(segs.one.blob), segs.one.N};      // MULTI = false: uniform values, no table read
    for (int kc = 0; kc < KD; kc += 192) {
        // gather: wave handles queries wave, wave+4, ...; lanes run along k (3 x 64 = 192)
        for (int q0 = wave; q0 < 32; q0 += 16) {
            float r[4][3][4];
            if (MULTI) gather4x3(r, q0, [&](int q) { return RowSrc{sblob[q], skind[q], sN[q]}; }, sel, kc + lane);
            else gather4x3(r, q0, [&](int) { return one; }, sel, kc + lane);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    if constexpr (JOINED) tile[q0 + 4 * qq][lane + 64 * u] = joined_mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3], sw[q0 + 4 * qq]);
                    else if constexpr (WEIGHTED) tile[q0 + 4 * qq][lane + 64 * u] = weighted_mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3], sw[q0 + 4 * qq]);
                    else tile[q0 + 4 * qq][lane + 64 * u] = mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3]);
                }
        }
        __syncthreads();
        if constexpr (ALPHA) store_tile_along_t_alpha(tile, out, mix_of(al...), a, n0, ncols, T, kc);
        else store_tile_along_t(tile, out, n0, ncols, T, kc);
        __syncthreads();
    }
}

// ---- a weighted blend of several indices (tvc_*_blend_f32) -------------------------------------------------------------------
// Every source row is searched once per term: term m of the call's ncols real columns is the virtual columns [m * ncols, (m + 1) * ncols)
// of ONE search (virtual row m * B + b holds the queries of source row b: query_normalize_kernel's Bsrc), whose segments are the
// (term, row) runs - each with its own path and overflow flag, exactly the single-index search of that (row, blob).  This kernel is the
// blend's knn_merge_gather_kernel<true>: one workgroup = 32 REAL columns; threads (m, q) merge term m's lists of column q and write its
// indices; the gather then walks the terms per query, four queries in flight per wave as there, and keeps
//   out = w_0 * mu_0;  out = out + w_m * mu_m  (m = 1 .. M - 1),   mu_m = (((r0 + r1) + r2) + r3) * 0.25f
// in registers - products and sums rounded separately (__fmul_rn / __fadd_rn), in term order - so the per-term matched tensors never exist
// in memory.  One LDS transpose, stores along t.  weights [rows][M] is the caller's DEVICE array, read here: a captured graph replays with
// whatever it holds then.  The weight row of a column is its batch row, or rowmap[col2b[column]] in a ragged batch (ragged.h).
// A... = AlphaIn: the alpha form, as above - the accumulated blend is the mu of its definition, alpha's row the weights'; ShareIn: the protect form.
constexpr int BLEND_MAX = TVC_BLEND_MAX;
template <class... A>
static __global__ __launch_bounds__(256) void knn_merge_blend_gather_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                                            const KnnSegs segs, const int* __restrict__ col2seg, int ncols, int T,
                                                                            int M, const float* __restrict__ weights, const int* __restrict__ col2b,
                                                                            const int* __restrict__ rowmap, float* __restrict__ out,
                                                                            int64_t* __restrict__ idx_out, const float* __restrict__ rv,
                                                                            const int* __restrict__ ri, const int* __restrict__ flags, const A... al) {
    constexpr bool ALPHA = Forms<A...>::mixed, WEIGHTED = Forms<A...>::weighted, JOINED = Forms<A...>::joined;
    __shared__ int sel[BLEND_MAX][32][4];
    __shared__ float tile[32][193];
    __shared__ const float* sblob[BLEND_MAX][32];
    __shared__ int skind[BLEND_MAX][32], sN[BLEND_MAX][32];
    __shared__ float sw[BLEND_MAX][32];
    __shared__ float snw[WEIGHTED ? BLEND_MAX : 1][WEIGHTED ? 32 : 1][5];      // the weighted forms: a (term, column)'s four weights and their sum
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * 32;
    float a = 0.f;
    if constexpr (ALPHA) {      // this thread's column in the store phase
        const int n = n0 + (tid & 31);
        a = alpha_of_column(mix_of(al...), n < ncols ? n : ncols - 1, T);
    }
    if (tid < 32 * M) {
        const int m = tid >> 5, q = tid & 31;
        const int n = n0 + q;
        const bool live = n < ncols;
        const int nc = live ? n : ncols - 1;            // (a column past the end gathers row 0 of the last column's blobs: never stored)
        const long vcols = (long)M * ncols;             // the search's columns: the lists' stride
        const long vc = (long)m * ncols + nc;           // this term's virtual column
        const int si = col2seg ? col2seg[vc] : 0;
        const KnnSeg g = seg_get(segs, si);
        [[maybe_unused]] float sims[4];
        [[maybe_unused]] int anchor = 0;
        if constexpr (JOINED) anchor = joined_top4((al.j, ...), vc, live, sel[m][q], sims);      // this term's own lists and path
        else if constexpr (WEIGHTED) merged_top4(g, si, flags, cand_v, cand_i, rv, ri, vcols, vc, live, idx_out, sel[m][q], sims, (al.w, ...).sims_out);
        else merged_top4(g, si, flags, cand_v, cand_i, rv, ri, vcols, vc, live, idx_out, sel[m][q]);
        sblob[m][q] = g.blob;
        skind[m][q] = blob_kind(g.blob);
        sN[m][q] = g.N;
        const int row = col2b ? rowmap[col2b[nc]] : nc / T;
        sw[m][q] = weights[(long)row * M + m];
        if constexpr (JOINED) join_weights((al.w, ...), row, sims, anchor, snw[m][q]);
        else if constexpr (WEIGHTED) match_weights((al.w, ...), row, sims, snw[m][q]);      // every term's mu_m: the row's k and width, the term's own similarities
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int kc = 0; kc < KD; kc += 192) {
        for (int q0 = wave; q0 < 32; q0 += 16) {
            float acc[4][3];
#pragma unroll 1
            for (int m = 0; m < M; ++m) {
                float r[4][3][4];
                gather4x3(r, q0, [&](int q) { return RowSrc{sblob[m][q], skind[m][q], sN[m][q]}; }, sel[m], kc + lane);
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    const float w = sw[m][q0 + 4 * qq];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        float mu;
                        if constexpr (JOINED) mu = joined_mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3], snw[m][q0 + 4 * qq]);
                        else if constexpr (WEIGHTED) mu = weighted_mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3], snw[m][q0 + 4 * qq]);
                        else mu = mean4(r[qq][u][0], r[qq][u][1], r[qq][u][2], r[qq][u][3]);
                        const float term = __fmul_rn(w, mu);
                        acc[qq][u] = m == 0 ? term : __fadd_rn(acc[qq][u], term);
                    }
                }
            }
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                for (int u = 0; u < 3; ++u) tile[q0 + 4 * qq][lane + 64 * u] = acc[qq][u];
        }
        __syncthreads();
        if constexpr (ALPHA) store_tile_along_t_alpha(tile, out, mix_of(al...), a, n0, ncols, T, kc);
        else store_tile_along_t(tile, out, n0, ncols, T, kc);
        __syncthreads();
    }
}

// out[i] = |1 - a| * idx_bound[i * stride] + |a| * srcmax[i], a = alpha[row[i]] (row == nullptr: i), products and sum rounded separately: the
// bound of utterance i's content in an alpha call (|mu| <= the alpha-less call's bound, |src| <= the measured |max| of its own ssl), the
// decoder's content bound there.  At a = 0 it is idx_bound exactly: such a row keeps the alpha-less call's scales.
static __global__ __launch_bounds__(256) void alpha_bound_kernel(const float* __restrict__ alpha, const int* __restrict__ row,
                                                                 const float* __restrict__ idx_bound, int stride, const float* __restrict__ srcmax,
                                                                 float* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = alpha[row ? row[i] : i];
    out[i] = __fadd_rn(__fmul_rn(fabsf(__fsub_rn(1.f, a)), idx_bound[(long)i * stride]), __fmul_rn(fabsf(a), srcmax[i]));
}
// a + (1 - a) * (p * w), every operation rounded on its own: the share of a frame of unvoiced weight w under alpha a and protect p
__device__ __forceinline__ float share_of_frame(float a, float p, float w) { return __fadd_rn(a, __fmul_rn(__fsub_rn(1.f, a), __fmul_rn(p, w))); }
// The protect form (alpha nullable: a = 0): a frame's share a_t lies between a (w = 0) and a_u = a + (1 - a) * p (w = 1) - rounding is monotonic -,
// so out[i] = max(|1 - a|, |1 - a_u|) * idx_bound + max(|a|, |a_u|) * srcmax; at p = 0, a_u == a and it is the kernel above's value exactly.
static __global__ __launch_bounds__(256) void protect_bound_kernel(const float* __restrict__ alpha, const float* __restrict__ protect,
                                                                   const int* __restrict__ row, const float* __restrict__ idx_bound, int stride,
                                                                   const float* __restrict__ srcmax, float* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = row ? row[i] : i;
    const float a = alpha ? alpha[r] : 0.f;
    const float au = share_of_frame(a, protect[r], 1.f);
    out[i] = __fadd_rn(__fmul_rn(fmaxf(fabsf(__fsub_rn(1.f, a)), fabsf(__fsub_rn(1.f, au))), idx_bound[(long)i * stride]),
                       __fmul_rn(fmaxf(fabsf(a), fabsf(au)), srcmax[i]));
}
int run_knn_alpha_bound(tvc_ctx* ctx, hipStream_t s, const float* alpha, const float* idx_bound, int stride, const float* srcmax, float* out, int n,
                        const float* protect) {
    const RagHost* h = ctx->rag;
    const int* row = h ? (const int*)h->d_row : (const int*)nullptr;
    if (protect) {
        hipLaunchKernelGGL(protect_bound_kernel, dim3((n + 255) / 256), dim3(256), 0, s, alpha, protect, row, idx_bound, stride, srcmax, out, n);
        return launch_check(ctx, "knn_protect_bound");
    }
    hipLaunchKernelGGL(alpha_bound_kernel, dim3((n + 255) / 256), dim3(256), 0, s, alpha, row, idx_bound, stride, srcmax, out, n);
    return launch_check(ctx, "knn_alpha_bound");
}

// ---- protect: a per-frame source share from the call's own f0 (tvc_*_protect_f32, tvc_frame_share_f32) -----------------------------------
// Frame t of an utterance of len frames at f0[0 .. len): u[t] = f0[t] > 0 (NaN and negatives: unvoiced), the voicing weight
// v[t] = (u[t-1] + 2 u[t] + u[t+1]) / 4 with u[-1] = u[0], u[len] = u[len-1] - neighbours never leave the utterance -, w = 1 - v one of
// {0, .25, .5, .75, 1} (exact), and the frame keeps a_t = a + (1 - a) * (p * w) of the source: torch's eager expression on fp32 tensors, every
// operation rounded on its own.  p = 0: a_t == a, bit for bit (a + 0 or a + (-0)).
__device__ __forceinline__ float frame_share_one(const float* __restrict__ f0, int len, int t, float a, float p) {
    const int tl = t > 0 ? t - 1 : 0, tr = t + 1 < len ? t + 1 : len - 1;
    const int voiced = (f0[tl] > 0.f ? 1 : 0) + (f0[t] > 0.f ? 2 : 0) + (f0[tr] > 0.f ? 1 : 0);
    return share_of_frame(a, p, (float)(4 - voiced) * 0.25f);
}
// one thread per query column n of a conversion: share[n] = a_t of its frame.  Its utterance: row n / T, columns [row * T, row * T + T) - or,
// in a ragged batch (col2b set: ragged.h's tables), utterance u = col2b[n], columns [pre[u], pre[u] + tb[u]), the caller's row rowmap[u].
static __global__ __launch_bounds__(256) void frame_share_kernel(const float* __restrict__ f0, const float* __restrict__ alpha,
                                                                 const float* __restrict__ protect, const int* __restrict__ col2b,
                                                                 const int* __restrict__ pre, const int* __restrict__ tb, const int* __restrict__ rowmap,
                                                                 int ncols, int T, float* __restrict__ share) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= ncols) return;
    int row = n / T, start = row * T, len = T;
    if (col2b) {
        const int u = col2b[n];
        row = rowmap[u];
        start = pre[u];
        len = tb[u];
    }
    share[n] = frame_share_one(f0 + start, len, n - start, alpha ? alpha[row] : 0.f, protect[row]);
}
int run_frame_share(tvc_ctx* ctx, hipStream_t s, const float* f0, const float* alpha, const float* protect, float* share, int B, int T) {
    const RagHost* h = ctx->rag;
    const int ncols = B * T;
    hipLaunchKernelGGL(frame_share_kernel, dim3((ncols + 255) / 256), dim3(256), 0, s, f0, alpha, protect, h ? (const int*)h->d_col2b : (const int*)nullptr,
                       h ? (const int*)h->d_pre : (const int*)nullptr, h ? (const int*)h->d_tb : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr,
                       ncols, T, share);
    return launch_check(ctx, "frame_share");
}
// the same over caller's rows: row i = columns [start[i], start[i] + len[i]) of f0 and share, the rows travel as kernel arguments (blockIdx.y)
constexpr int FS_ROWS = 256;
struct FrameShareRows {
    int start[FS_ROWS], len[FS_ROWS];
};
static __global__ __launch_bounds__(256) void frame_share_rows_kernel(FrameShareRows r, int row0, const float* __restrict__ f0, const float* __restrict__ alpha,
                                                                      const float* __restrict__ protect, float* __restrict__ share) {
    const int i = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= r.len[i]) return;
    const long start = r.start[i];
    share[start + t] = frame_share_one(f0 + start, r.len[i], t, alpha ? alpha[row0 + i] : 0.f, protect[row0 + i]);
}
int run_frame_share_rows(tvc_ctx* ctx, hipStream_t s, const float* f0, const std::vector<int>& start, const std::vector<int>& len, const float* alpha,
                         const float* protect, float* share) {
    for (size_t o = 0; o < start.size(); o += FS_ROWS) {
        FrameShareRows r;
        const int n = (int)(start.size() - o < FS_ROWS ? start.size() - o : FS_ROWS);
        int longest = 0;
        for (int i = 0; i < n; ++i) {
            r.start[i] = start[o + i];
            r.len[i] = len[o + i];
            if (len[o + i] > longest) longest = len[o + i];
        }
        if (longest == 0) continue;
        hipLaunchKernelGGL(frame_share_rows_kernel, dim3((longest + 255) / 256, n), dim3(256), 0, s, r, (int)o, f0, alpha, protect, share);
    }
    return launch_check(ctx, "frame_share_rows");
}

// out[i] = sum_m |w[row[i]][m]| * (the |max| of blob (i, m)), in term order, products and sums rounded separately: the bound of row i's blended
// content (|mu_m| <= its blob's |max|), the decoder's content bound of a blend call.  One workgroup; the blobs and the weight rows travel as
// kernel arguments (like index_amax_rows_kernel), the weights are read from the caller's device array.
constexpr int BB_ROWS = 64;
struct BlendBoundChunk {
    const float* p[BB_ROWS * BLEND_MAX];
    int row[BB_ROWS];
};
static __global__ __launch_bounds__(BB_ROWS) void blend_bound_kernel(BlendBoundChunk c, const float* __restrict__ weights, int M, float* __restrict__ out, int n) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const float* w = weights + (long)c.row[i] * M;
    float b = __fmul_rn(fabsf(w[0]), *blob_amax(c.p[i * M]));
    for (int m = 1; m < M; ++m) b = __fadd_rn(b, __fmul_rn(fabsf(w[m]), *blob_amax(c.p[i * M + m])));
    out[i] = b;
}
int run_knn_blend_bound(tvc_ctx* ctx, hipStream_t s, const std::vector<const float*>& blobs, const std::vector<int>& rows, int M, const float* weights, float* out) {
    for (size_t o = 0; o < rows.size(); o += BB_ROWS) {
        BlendBoundChunk c;
        const int n = (int)(rows.size() - o < BB_ROWS ? rows.size() - o : BB_ROWS);
        for (int i = 0; i < n; ++i) {
            c.row[i] = rows[o + i];
            for (int m = 0; m < M; ++m) c.p[i * M + m] = blobs[(o + i) * M + m];
        }
        hipLaunchKernelGGL(blend_bound_kernel, dim3(1), dim3(BB_ROWS), 0, s, c, weights, M, out + o, n);
    }
    return launch_check(ctx, "knn_blend_bound");
}

// out[i] = the |max| of blob i (one index per utterance: each utterance's content bound is its own index's): the pointers travel as kernel
// arguments, like ragged.h's upload_ints
struct BlobChunk {
    const float* p[480];
};
static __global__ void index_amax_rows_kernel(BlobChunk c, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = *blob_amax(c.p[i]);
}
int run_knn_amax_rows(tvc_ctx* ctx, hipStream_t s, const std::vector<const float*>& blobs, float* out) {
    for (size_t o = 0; o < blobs.size(); o += 480) {
        BlobChunk c;
        const int n = (int)(blobs.size() - o < 480 ? blobs.size() - o : 480);
        for (int i = 0; i < n; ++i) c.p[i] = blobs[o + i];
        hipLaunchKernelGGL(index_amax_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c, out + o, n);
    }
    return launch_check(ctx, "knn_amax_rows");
}

// ---- index-sharded search (one index shard per GPU): local top-4 with similarities, slot gather, finish ----
// merge the split candidates of every query -> this shard's top-4 (similarity, local index)
static __global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i, int nsplit, int ncols,
                                                               float* __restrict__ sims_out, int64_t* __restrict__ idx_out,
                                                               const float* __restrict__ rv, const int* __restrict__ ri, const int* __restrict__ flag) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= ncols) return;
    if (flag && *flag == 0) {
        cand_v = rv;
        cand_i = ri;
        nsplit = 1;
    }
    const Top4 t4 = merge_lists(cand_v, cand_i, nsplit, ncols, n);      // sentinels as they are: the caller merges across shards
    for (int e = 0; e < 4; ++e) {
        sims_out[(long)n * 4 + e] = t4.v[e];
        idx_out[(long)n * 4 + e] = (int64_t)t4.i[e];
    }
}
// slots[n][e][:] = raw row idx[n][e] of this shard, or zeros where idx < 0 (the row lives on another rank)
static __global__ __launch_bounds__(192) void knn_slot_gather_kernel(const float* __restrict__ blob, const int64_t* __restrict__ idx, long nslots,
                                                                     long N, long Npad, float* __restrict__ slots) {
    const long sl = blockIdx.x;
    if (sl >= nslots) return;
    const int kind = blob_kind(blob);
    const int64_t i = idx[sl];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i >= 0 && i < N) {
        const int k = 4 * threadIdx.x;
        v = make_float4(blob_row_value(blob, kind, N, Npad, i, k), blob_row_value(blob, kind, N, Npad, i, k + 1),
                        blob_row_value(blob, kind, N, Npad, i, k + 2), blob_row_value(blob, kind, N, Npad, i, k + 3));
    }
    reinterpret_cast<float4*>(slots + sl * KD)[threadIdx.x] = v;
}
// out[b][k][t] = (((s0 + s1) + s2) + s3) * 0.25 from slots [B*T][4][768] (the same order as the single-GPU gather),
// transposed through LDS so reads run along k and stores along t
static __global__ __launch_bounds__(256) void knn_finish_kernel(const float* __restrict__ slots, int ncols, int T, float* __restrict__ out) {
    __shared__ float tile[32][193];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 32;
    for (int kc = 0; kc < KD; kc += 192) {
        for (int q = wave; q < 32; q += 4) {
            const int n = n0 + q < ncols ? n0 + q : ncols - 1;
            const float* r0 = slots + ((long)n * 4) * KD + kc;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int k = lane + 64 * u;
                tile[q][k] = mean4(r0[k], r0[KD + k], r0[2 * KD + k], r0[3 * KD + k]);
            }
        }
        __syncthreads();
        store_tile_along_t(tile, out, n0, ncols, T, kc);
        __syncthreads();
    }
}

int run_knn_topk(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const float* prepared, int64_t N,
                 float* sims_out, int64_t* idx_out, int B, int T) {
    const KnnSegIn one{prepared, N, 0, B * T};
    KnnCall c;
    TVC_CHECK(knn_call_plan(ctx, &one, 1, B * T, &c));
    KnnLists L;
    TVC_CHECK(knn_candidates(ctx, s, ws, src, c, B, T, &L));
    if (ws.dry) return 0;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((c.ncols + 255) / 256), dim3(256), 0, s, L.cv, L.ci, c.seg[0].nsE, c.ncols, sims_out, idx_out, L.rv, L.ri, L.flag);
    return launch_check(ctx, "knn_topk");
}

int run_knn_slots(tvc_ctx* ctx, hipStream_t s, const float* prepared, int64_t N, const int64_t* idx, float* slots, int64_t nslots) {
    hipLaunchKernelGGL(knn_slot_gather_kernel, dim3((unsigned)nslots), dim3(192), 0, s, prepared, idx, (long)nslots, (long)N, blob_npad(N), slots);
    return launch_check(ctx, "knn_slots");
}

int run_knn_finish(tvc_ctx* ctx, hipStream_t s, const float* slots, float* out, int B, int T) {
    const int ncols = B * T;
    hipLaunchKernelGGL(knn_finish_kernel, dim3((ncols + 31) / 32), dim3(256), 0, s, slots, ncols, T, out);
    return launch_check(ctx, "knn_finish");
}

// ---- match along a path (tvc_*joined*_f32): merge + affinity, the path, then the joined form of the merge + gather above -------------------
// 1. knn_join_affinity_kernel: one workgroup = 32 consecutive VIRTUAL columns (a blend's terms are columns m * ncols + n of the one search)
//    and the column in front of them.  Threads 0 .. 32 merge their column's lists (merged_top4: idx_out and sims_out are written here) and
//    leave rows and similarities in workspace for the other two kernels.  Then every wave walks 8 columns in order, the rows of the column
//    before in registers and the next column's 48 loads in flight: lanes along the 768 channels as gather4x3 has them, the 16 dots
//      dot[d][e] = sum_k row i_{t-1}[d][k] * row i_t[e][k]
//    each in ONE order - lane l adds its channels l, l + 64, .., l + 704 in ascending order (product and sum rounded on their own), then the 64
//    partial sums meet in a butterfly over lane distances 32, 16, 8, 4, 2, 1 (every lane adds its partner's value to its own: fp32 addition
//    commutes, so all lanes hold the same bits) - and a = (dot * inv[i_{t-1}[d]]) * inv[i_t[e]].  The order knows nothing of tiles, splits,
//    the batch or k.  The first frame of an utterance gets zeros.
// 2. knn_join_path_kernel: one wavefront per (term, utterance), four to a workgroup; the definition's recursion on wave-uniform values, a
//    chunk of 64 frames' similarities and affinities in the lanes' registers (lane j holds frame j's twenty floats, the next chunk's loads in
//    flight), one byte of back-pointers per frame (2 bits per state) to workspace, and the walk back in the same launch.
// MEMORY SAFETY: a back-pointer is the d < k of a comparison chain that starts at d = 0 and the last anchor the e < k of one that starts at
// e = 0, so every anchor lies in 0 .. k - 1 whatever the scores are; the scores themselves stay finite by the definition's saturations.
constexpr float JOIN_BIG = 3.402823466e38f;      // FLT_MAX
__device__ __forceinline__ float join_sat(float x) { return fminf(fmaxf(x, -JOIN_BIG), JOIN_BIG); }      // (NaN: -FLT_MAX)
__device__ __forceinline__ float join_finite(float x) { return fabsf(x) <= JOIN_BIG ? x : 0.f; }        // NaN and +-inf count as 0
struct JoinWs {           // workspace of one joined call, [vcols] = M * B * T entries each
    int* sel;             // [vcols][4]
    float* sims;          // [vcols][4]
    float* aff;           // [vcols][16], [d][e]
    unsigned char* bp;    // [vcols]
    int* anchor;          // [vcols]
};
static __global__ __launch_bounds__(256) void knn_join_affinity_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i, const KnnSegs segs,
                                                                       const int* __restrict__ col2seg, int vcols, int ncols, int T,
                                                                       const int* __restrict__ col2b, const int* __restrict__ pre,
                                                                       int64_t* __restrict__ idx_out, float* __restrict__ sims_out,
                                                                       const float* __restrict__ rv, const int* __restrict__ ri,
                                                                       const int* __restrict__ flags, JoinWs jw, float* __restrict__ aff_out) {
    __shared__ int sel[33][4];
    __shared__ const float* sblob[33];
    __shared__ int skind[33], sN[33], sfirst[33];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * 32;
    if (tid < 33) {      // slot 0: the column in front of the tile
        const int vc = n0 - 1 + tid;
        const bool live = vc >= 0 && vc < vcols;
        const int vcc = vc < 0 ? 0 : (vc < vcols ? vc : vcols - 1);
        const int si = col2seg ? col2seg[vcc] : 0;
        const KnnSeg g = seg_get(segs, si);
        const bool own = tid > 0;
        float sims[4];
        merged_top4(g, si, flags, cand_v, cand_i, rv, ri, vcols, vc, live, own ? idx_out : nullptr, sel[tid], sims, own ? sims_out : nullptr);
        if (own && live)
            for (int e = 0; e < 4; ++e) {
                jw.sel[(long)vc * 4 + e] = sel[tid][e];
                jw.sims[(long)vc * 4 + e] = sims[e];
            }
        sblob[tid] = g.blob;
        skind[tid] = blob_kind(g.blob);
        sN[tid] = g.N;
        const int n = vcc % ncols;      // the real column: a path never leaves its term, its row or its utterance
        sfirst[tid] = col2b ? n == pre[col2b[n]] : n % T == 0;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    float prev[4][12], cur[4][12], nxt[4][12];
    const auto load = [&](float (&r)[4][12], int slot) {
        const float* blob = sblob[slot];
        const int kind = skind[slot], N = sN[slot];
        const long Npad = blob_npad(N);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int u = 0; u < 12; ++u) r[e][u] = blob_row_value(blob, kind, N, Npad, sel[slot][e], lane + 64 * u);
    };
    load(prev, wave * 8);
    load(cur, wave * 8 + 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int slot = wave * 8 + 1 + j;
        const int vc = n0 + wave * 8 + j;
        if (j < 7) load(nxt, slot + 1);
        if (vc < vcols) {      // wave-uniform
            float a = 0.f;
            if (!sfirst[slot]) {
                float mine = 0.f;
#pragma unroll
                for (int d = 0; d < 4; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float acc = __fmul_rn(prev[d][0], cur[e][0]);
#pragma unroll
                        for (int u = 1; u < 12; ++u) acc = __fadd_rn(acc, __fmul_rn(prev[d][u], cur[e][u]));
#pragma unroll
                        for (int m = 32; m; m >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, m));
                        mine = lane == d * 4 + e ? acc : mine;
                    }
                if (lane < 16) {
                    const int d = lane >> 2, e = lane & 3;
                    const float* ip = blob_inv(sblob[slot - 1], skind[slot - 1], sN[slot - 1], blob_npad(sN[slot - 1]));
                    const float* ic = blob_inv(sblob[slot], skind[slot], sN[slot], blob_npad(sN[slot]));
                    a = __fmul_rn(__fmul_rn(mine, ip[sel[slot - 1][d]]), ic[sel[slot][e]]);
                }
            }
            if (lane < 16) {
                jw.aff[(long)vc * 16 + lane] = a;
                if (aff_out) aff_out[(long)vc * 16 + lane] = a;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int u = 0; u < 12; ++u) {
                prev[e][u] = cur[e][u];
                cur[e][u] = nxt[e][u];
            }
    }
}

// the (term, utterance) paths of one launch by value: virtual columns [start, start + len), row = the caller's row (k and the continuity weight)
constexpr int JOIN_ROWS = 256;
struct JoinRows {
    int start[JOIN_ROWS], len[JOIN_ROWS], row[JOIN_ROWS];
};
// uniform_len >= 0: path i = columns [i * uniform_len, + uniform_len), row i % rowmod - any number of paths in one launch
static __global__ __launch_bounds__(256) void knn_join_path_kernel(JoinRows rows, int nrows, int uniform_len, int rowmod, const int* __restrict__ neighbours,
                                                                   const float* __restrict__ join, JoinWs jw, int* __restrict__ anchor_out) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= nrows) return;
    const int len = uniform_len >= 0 ? uniform_len : rows.len[u];
    if (len <= 0) return;
    const long start = uniform_len >= 0 ? (long)u * uniform_len : (long)rows.start[u];
    const int row = uniform_len >= 0 ? u % rowmod : rows.row[u];
    int k = neighbours ? neighbours[row] : 4;
    k = k < 1 ? 1 : (k > 4 ? 4 : k);
    float c = join[row];
    c = c > 0.f ? fminf(c, JOIN_BIG) : 0.f;      // NaN and negatives: 0; +inf: the largest finite float
    const float4* __restrict__ sims4 = reinterpret_cast<const float4*>(jw.sims) + start;
    const float4* __restrict__ aff4 = reinterpret_cast<const float4*>(jw.aff) + start * 4;
    const auto bcast = [](float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ns = lane < len ? sims4[lane] : zero, na[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) na[d] = lane < len ? aff4[lane * 4 + d] : zero;
    float D[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int m = min(64, len - t0);
        const float4 cs = ns;
        float4 ca[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) ca[d] = na[d];
        if (t0 + 64 < len) {      // the next chunk's twenty floats per frame, in flight while this one is walked
            const int t = t0 + 64 + lane;
            ns = t < len ? sims4[t] : zero;
#pragma unroll
            for (int d = 0; d < 4; ++d) na[d] = t < len ? aff4[(long)t * 4 + d] : zero;
        }
        int mybp = 0;
        for (int j = 0; j < m; ++j) {
            const float s[4] = {join_finite(bcast(cs.x, j)), join_finite(bcast(cs.y, j)), join_finite(bcast(cs.z, j)), join_finite(bcast(cs.w, j))};
            float x[4];
            int bpj = 0;
            if (t0 + j == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = s[e];
            } else {
                float jc[4][4];      // c * a_t[d][e], saturated
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    jc[d][0] = join_sat(__fmul_rn(c, join_finite(bcast(ca[d].x, j))));
                    jc[d][1] = join_sat(__fmul_rn(c, join_finite(bcast(ca[d].y, j))));
                    jc[d][2] = join_sat(__fmul_rn(c, join_finite(bcast(ca[d].z, j))));
                    jc[d][3] = join_sat(__fmul_rn(c, join_finite(bcast(ca[d].w, j))));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float best = __fadd_rn(D[0], jc[0][e]);
                    int bd = 0;
#pragma unroll
                    for (int d = 1; d < 4; ++d) {
                        const float cand = __fadd_rn(D[d], jc[d][e]);
                        const bool take = d < k && cand > best;      // ties keep the lowest d
                        best = take ? cand : best;
                        bd = take ? d : bd;
                    }
                    x[e] = join_sat(__fadd_rn(s[e], best));
                    bpj |= bd << (2 * e);
                }
            }
            float mx = x[0];
#pragma unroll
            for (int e = 1; e < 4; ++e) mx = e < k ? fmaxf(mx, x[e]) : mx;
#pragma unroll
            for (int e = 0; e < 4; ++e) D[e] = join_sat(__fsub_rn(x[e], mx));
            mybp = lane == j ? bpj : mybp;
        }
        if (lane < m) jw.bp[start + t0 + lane] = (unsigned char)mybp;
    }
    int p = 0;
    {
        float best = D[0];
#pragma unroll
        for (int e = 1; e < 4; ++e) {
            const bool take = e < k && D[e] > best;
            best = take ? D[e] : best;
            p = take ? e : p;
        }
    }
    __threadfence();      // the back-pointers the other lanes stored are read below
    for (int t0 = (len - 1) / 64 * 64; t0 >= 0; t0 -= 64) {
        const int m = min(64, len - t0);
        const int mybp = lane < m ? (int)jw.bp[start + t0 + lane] : 0;
        int mine = 0;
        for (int j = m - 1; j >= 0; --j) {
            mine = lane == j ? p : mine;
            p = (__builtin_amdgcn_readlane(mybp, j) >> (2 * p)) & 3;      // frame t0 + j's back-pointer of state p: the anchor of the frame before
        }
        if (lane < m) {
            jw.anchor[start + t0 + lane] = mine;
            if (anchor_out) anchor_out[start + t0 + lane] = mine;
        }
    }
}

// what a joined call takes from the workspace, in both walks: the merged lists, the affinities, the back-pointers and the anchors
static JoinWs join_workspace(Ws& ws, size_t vcols) {
    JoinWs jw;
    jw.sel = ws.get<int>(vcols * 4);
    jw.sims = ws.get<float>(vcols * 4);
    jw.aff = ws.get<float>(vcols * 16);
    jw.bp = ws.get<unsigned char>(vcols);
    jw.anchor = ws.get<int>(vcols);
    return jw;
}
// the two launches in front of the joined gather: M terms of `ncols` real columns each (B rows of T, or the current ragged batch's utterances)
// (under tvc_profile_enable each of the two is a region of its own, "knn.join_affinity" and "knn.join_path": tools/match_join_probe.py)
static int run_knn_join(tvc_ctx* ctx, hipStream_t s, const Ws& ws, const KnnLists& L, int M, int B, int T, const KnnWeight& wt, const KnnJoin& jn,
                        const JoinWs& jw, int64_t* idx_out) {
    const RagHost* h = ctx->rag;
    const int ncols = B * T, vcols = M * ncols;
    {
        ProfScope ps(ctx, s, ws, "knn.join_affinity");
        hipLaunchKernelGGL(knn_join_affinity_kernel, dim3((vcols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, vcols, ncols, T,
                           h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_pre : (const int*)nullptr, idx_out, wt.sims_out, L.rv, L.ri,
                           (const int*)L.flag, jw, jn.affinity_out);
    }
    TVC_CHECK(launch_check(ctx, "knn_join_affinity"));
    ProfScope ps(ctx, s, ws, "knn.join_path");
    JoinRows r = {};
    if (!h) {      // equal rows: one launch however many
        hipLaunchKernelGGL(knn_join_path_kernel, dim3((M * B + 3) / 4), dim3(256), 0, s, r, M * B, T, B, wt.neighbours, jn.join, jw, jn.anchor_out);
        return launch_check(ctx, "knn_join_path");
    }
    const size_t n = (size_t)M * h->B;
    for (size_t o = 0; o < n; o += JOIN_ROWS) {
        const int cnt = (int)(n - o < JOIN_ROWS ? n - o : JOIN_ROWS);
        for (int i = 0; i < cnt; ++i) {
            const int m = (int)((o + i) / h->B), ui = (int)((o + i) % h->B);
            r.start[i] = m * ncols + h->pre[ui];
            r.len[i] = h->tb[ui];
            r.row[i] = h->row[ui];
        }
        hipLaunchKernelGGL(knn_join_path_kernel, dim3((cnt + 3) / 4), dim3(256), 0, s, r, cnt, -1, 1, wt.neighbours, jn.join, jw, jn.anchor_out);
    }
    return launch_check(ctx, "knn_join_path");
}

// the weighted forms' launch: the same grid and lists with Weighted<Mix> as the one more argument (Mix: the store form's AlphaIn / ShareIn / NoMix)
static WeightIn weight_in(const tvc_ctx* ctx, const KnnWeight& wt) {
    const RagHost* h = ctx->rag;
    return WeightIn{wt.neighbours, wt.width, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr, wt.sims_out};
}
template <class Mix>
static int launch_weighted(tvc_ctx* ctx, hipStream_t s, const KnnCall& c, const KnnLists& L, int T, float* out, int64_t* idx_out, const KnnWeight& wt, const Mix& mix) {
    const Weighted<Mix> x{weight_in(ctx, wt), mix};
    const auto kernel = L.col2seg ? knn_merge_gather_kernel<true, Weighted<Mix>> : knn_merge_gather_kernel<false, Weighted<Mix>>;
    hipLaunchKernelGGL(kernel, dim3((c.ncols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, c.ncols, T, out, idx_out, L.rv, L.ri,
                       (const int*)L.flag, x);
    return launch_check(ctx, "knn_match_weighted");
}
template <class Mix>
static int launch_weighted_blend(tvc_ctx* ctx, hipStream_t s, const KnnLists& L, int B, int T, int M, const float* weights, float* out, int64_t* idx_out,
                                 const KnnWeight& wt, const Mix& mix) {
    const Weighted<Mix> x{weight_in(ctx, wt), mix};
    hipLaunchKernelGGL(knn_merge_blend_gather_kernel<Weighted<Mix>>, dim3((B * T + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, B * T, T, M,
                       weights, x.w.col2b, x.w.rowmap, out, idx_out, L.rv, L.ri, (const int*)L.flag, x);
    return launch_check(ctx, "knn_match_blend_weighted");
}

// the joined forms' launch: Joined<Mix> in Weighted<Mix>'s place - the lists, the indices and the similarities are in workspace already
template <class Mix>
static int launch_joined(tvc_ctx* ctx, hipStream_t s, const KnnCall& c, const KnnLists& L, int T, float* out, const KnnWeight& wt, const JoinWs& jw, const Mix& mix) {
    const Joined<Mix> x{weight_in(ctx, wt), JoinIn{jw.sel, jw.sims, jw.anchor}, mix};
    const auto kernel = L.col2seg ? knn_merge_gather_kernel<true, Joined<Mix>> : knn_merge_gather_kernel<false, Joined<Mix>>;
    hipLaunchKernelGGL(kernel, dim3((c.ncols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, c.ncols, T, out, (int64_t*)nullptr, L.rv, L.ri,
                       (const int*)L.flag, x);
    return launch_check(ctx, "knn_match_joined");
}
template <class Mix>
static int launch_joined_blend(tvc_ctx* ctx, hipStream_t s, const KnnLists& L, int B, int T, int M, const float* weights, float* out, const KnnWeight& wt,
                               const JoinWs& jw, const Mix& mix) {
    const Joined<Mix> x{weight_in(ctx, wt), JoinIn{jw.sel, jw.sims, jw.anchor}, mix};
    hipLaunchKernelGGL(knn_merge_blend_gather_kernel<Joined<Mix>>, dim3((B * T + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, B * T, T, M,
                       weights, x.w.col2b, x.w.rowmap, out, (int64_t*)nullptr, L.rv, L.ri, (const int*)L.flag, x);
    return launch_check(ctx, "knn_match_blend_joined");
}

int run_knn_segs(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const KnnSegIn* in, int nin, float* out, int64_t* idx_out, int B, int T,
                 const float* alpha, const float* share, const KnnWeight* wt, const KnnJoin* jn) {
    KnnCall c;
    TVC_CHECK(knn_call_plan(ctx, in, nin, B * T, &c));
    KnnLists L;
    TVC_CHECK(knn_candidates(ctx, s, ws, src, c, B, T, &L));
    JoinWs jw{};
    if (jn) jw = join_workspace(ws, (size_t)B * T);
    if (ws.dry) return 0;
    if (jn) {      // the joined forms: merge + affinity, the path, then the weights around the path's anchor; the store form as below
        const KnnWeight none{};
        const KnnWeight& w = wt ? *wt : none;
        const RagHost* h = ctx->rag;
        TVC_CHECK(run_knn_join(ctx, s, ws, L, 1, B, T, w, *jn, jw, idx_out));
        if (share) return launch_joined(ctx, s, c, L, T, out, w, jw, ShareIn{share, src});
        if (alpha) return launch_joined(ctx, s, c, L, T, out, w, jw, AlphaIn{alpha, src, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr});
        return launch_joined(ctx, s, c, L, T, out, w, jw, NoMix{});
    }
    if (wt) {      // the weighted forms: the same lists, the four rows weighted by their similarities; the store form as below
        const RagHost* h = ctx->rag;
        if (share) return launch_weighted(ctx, s, c, L, T, out, idx_out, *wt, ShareIn{share, src});
        if (alpha) return launch_weighted(ctx, s, c, L, T, out, idx_out, *wt, AlphaIn{alpha, src, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr});
        return launch_weighted(ctx, s, c, L, T, out, idx_out, *wt, NoMix{});
    }
    if (share) {      // the protect form: a share per column (run_frame_share), which has alpha in it
        const ShareIn sh{share, src};
        const auto skernel = L.col2seg ? knn_merge_gather_kernel<true, ShareIn> : knn_merge_gather_kernel<false, ShareIn>;
        hipLaunchKernelGGL(skernel, dim3((c.ncols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, c.ncols, T, out, idx_out, L.rv, L.ri,
                           (const int*)L.flag, sh);
        return launch_check(ctx, "knn_match_protect");
    }
    if (alpha) {      // the alpha form: the same lists, the source's share mixed in at the store (a ragged batch finds alpha's row through its tables)
        const RagHost* h = ctx->rag;
        const AlphaIn al{alpha, src, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr};
        const auto akernel = L.col2seg ? knn_merge_gather_kernel<true, AlphaIn> : knn_merge_gather_kernel<false, AlphaIn>;
        hipLaunchKernelGGL(akernel, dim3((c.ncols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, c.ncols, T, out, idx_out, L.rv, L.ri,
                           (const int*)L.flag, al);
        return launch_check(ctx, "knn_match_alpha");
    }
    const auto kernel = L.col2seg ? knn_merge_gather_kernel<true> : knn_merge_gather_kernel<false>;      // several segments : one (no table read)
    hipLaunchKernelGGL(kernel, dim3((c.ncols + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, c.ncols, T, out, idx_out, L.rv, L.ri,
                       (const int*)L.flag);
    return launch_check(ctx, "knn_match");
}

// in[]: the (term, row) runs over the M * B * T virtual columns, term-major (term m's copy of real column n is column m * B * T + n); one
// knn_candidates walk - every pass one launch, as run_knn_segs -, then the blend gather.  idx_out (nullable): [M][B][T][4].  A ragged batch
// (ctx->rag: B = 1, T = all its frames) finds a column's weight row through the batch's tables.
int run_knn_blend(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const KnnSegIn* in, int nin, int M, const float* weights, float* out,
                  int64_t* idx_out, int B, int T, const float* alpha, const float* share, const KnnWeight* wt, const KnnJoin* jn) {
    KnnCall c;
    TVC_CHECK(knn_call_plan(ctx, in, nin, M * B * T, &c));
    KnnLists L;
    TVC_CHECK(knn_candidates(ctx, s, ws, src, c, M * B, T, &L, B));
    JoinWs jw{};
    if (jn) jw = join_workspace(ws, (size_t)M * B * T);
    if (ws.dry) return 0;
    const RagHost* h = ctx->rag;
    if (jn) {      // every term a path of its own
        const KnnWeight none{};
        const KnnWeight& w = wt ? *wt : none;
        TVC_CHECK(run_knn_join(ctx, s, ws, L, M, B, T, w, *jn, jw, idx_out));
        if (share) return launch_joined_blend(ctx, s, L, B, T, M, weights, out, w, jw, ShareIn{share, src});
        if (alpha) return launch_joined_blend(ctx, s, L, B, T, M, weights, out, w, jw, AlphaIn{alpha, src, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr});
        return launch_joined_blend(ctx, s, L, B, T, M, weights, out, w, jw, NoMix{});
    }
    if (wt) {
        if (share) return launch_weighted_blend(ctx, s, L, B, T, M, weights, out, idx_out, *wt, ShareIn{share, src});
        if (alpha) return launch_weighted_blend(ctx, s, L, B, T, M, weights, out, idx_out, *wt, AlphaIn{alpha, src, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr});
        return launch_weighted_blend(ctx, s, L, B, T, M, weights, out, idx_out, *wt, NoMix{});
    }
    if (share) {
        const ShareIn sh{share, src};
        hipLaunchKernelGGL(knn_merge_blend_gather_kernel<ShareIn>, dim3((B * T + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, B * T, T, M,
                           weights, h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr, out, idx_out, L.rv, L.ri,
                           (const int*)L.flag, sh);
        return launch_check(ctx, "knn_match_blend_protect");
    }
    if (alpha) {
        const int* col2b = h ? (const int*)h->d_col2b : nullptr;
        const int* rowmap = h ? (const int*)h->d_row : nullptr;
        const AlphaIn al{alpha, src, col2b, rowmap};
        hipLaunchKernelGGL(knn_merge_blend_gather_kernel<AlphaIn>, dim3((B * T + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, B * T, T, M,
                           weights, col2b, rowmap, out, idx_out, L.rv, L.ri, (const int*)L.flag, al);
        return launch_check(ctx, "knn_match_blend_alpha");
    }
    hipLaunchKernelGGL(knn_merge_blend_gather_kernel<>, dim3((B * T + 31) / 32), dim3(256), 0, s, L.cv, L.ci, L.segs, (const int*)L.col2seg, B * T, T, M, weights,
                       h ? (const int*)h->d_col2b : (const int*)nullptr, h ? (const int*)h->d_row : (const int*)nullptr, out, idx_out, L.rv, L.ri,
                       (const int*)L.flag);
    return launch_check(ctx, "knn_match_blend");
}

int run_knn(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const float* prepared, int64_t N,
            float* out, int64_t* idx_out, int B, int T) {
    const KnnSegIn one{prepared, N, 0, B * T};
    return run_knn_segs(ctx, s, ws, src, &one, 1, out, idx_out, B, T);
}

}  // namespace tvc
