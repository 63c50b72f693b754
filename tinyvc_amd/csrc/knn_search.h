// What the search (knn.hip) hands to the kernels that turn its lists into results (knn_gather.hip): the segment table, the top-4 list
// type and the host plan of one call.  Internal to those two files.
#pragma once
#include "tvc_common.h"

namespace tvc {

// ---- segments: one call, several prepared indices -------------------------------------------------------------------------
// A segment is a maximal run of consecutive query columns that search the same blob (tvc_*_multi: one speaker index per row; a
// ragged sub-batch's rows in its own order).  Query tiles (KNN_QT = C_QT = 256) never cross a segment; every pass is ONE launch
// over the concatenated (segment, query tile, split) work units of the segments that take it, a workgroup finds its segment in the
// unit prefix u[], and the per-query kernels (rescore, merge + gather) look it up in col2seg[].  Each segment has its own overflow
// flag, so it takes exactly the path its own B = 1 call takes.  A call with one blob is one segment - the table then travels by
// value in the kernel arguments (KnnSegs::one) and nothing is uploaded: the single-index launch sequence is the degenerate case.
struct KnnSeg {
    const float* blob;
    int N, col0, ncols;        // query columns [col0, col0 + ncols) of the call
    int two;                   // two-stage search (N >= KNN_COARSE_MIN); else the exact kernel only
    int sample, t2;            // 256-vector tiles covered by coarse pass A / pass B
    int nsA, tpsA, nsB, tpsB;  // coarse splits
    int nsE, tpsE;             // exact kernel splits
    int u[4];                  // first work unit of pass A, pass B and the exact kernel; [3]: first 256-query tile
};
static_assert(sizeof(KnnSeg) % sizeof(int) == 0, "uploaded as ints");
struct KnnSegs {               // kernel argument
    const KnnSeg* d;           // device table (n > 1)
    int n;
    KnnSeg one;                // the table when n == 1
};
// last segment whose key (u[F]; F == 4: col0) is <= v - segments without units of a launch share their successor's prefix and are skipped
template <int F>
__device__ __forceinline__ int seg_find(const KnnSegs& S, int v) {
    if (S.n == 1) return 0;
    int lo = 0, hi = S.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int key = F == 4 ? S.d[mid].col0 : S.d[mid].u[F];
        if (key <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// field by field: a select between the kernel-argument copy and the device table (selecting the whole struct put it on the stack)
__device__ __forceinline__ KnnSeg seg_get(const KnnSegs& S, int i) {
    KnnSeg g;
    const bool one = S.n == 1;
    const KnnSeg* __restrict__ d = S.d + (one ? 0 : i);
#define TVC_SEG_FIELD(f) g.f = one ? S.one.f : d->f
    TVC_SEG_FIELD(blob);
    TVC_SEG_FIELD(N);
    TVC_SEG_FIELD(col0);
    TVC_SEG_FIELD(ncols);
    TVC_SEG_FIELD(two);
    TVC_SEG_FIELD(sample);
    TVC_SEG_FIELD(t2);
    TVC_SEG_FIELD(nsA);
    TVC_SEG_FIELD(tpsA);
    TVC_SEG_FIELD(nsB);
    TVC_SEG_FIELD(tpsB);
    TVC_SEG_FIELD(nsE);
    TVC_SEG_FIELD(tpsE);
    TVC_SEG_FIELD(u[0]);
    TVC_SEG_FIELD(u[1]);
    TVC_SEG_FIELD(u[2]);
    TVC_SEG_FIELD(u[3]);
#undef TVC_SEG_FIELD
    return g;
}

// torch.topk orders NaN above every number; a query column with NaN / Inf samples upstream makes every similarity NaN.
// Mapping NaN to +inf keeps that order (ties -> lowest index, so such a column selects rows 0..3 like any all-equal
// column) and, more to the point, keeps the 0x7fffffff list sentinel from ever reaching the row gather.
__device__ __forceinline__ float nan_max(float x) { return x != x ? INFINITY : x; }

struct Top4 {
    float v[4];
    int i[4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = -INFINITY;
            i[j] = 0x7fffffff;
        }
    }
    // strict ordering: higher value first, then lower index
    __device__ __forceinline__ static bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
    __device__ __forceinline__ void insert(float x, int ix) {
        if (!better(x, ix, v[3], i[3])) return;
        if (better(x, ix, v[0], i[0])) { v[3] = v[2]; i[3] = i[2]; v[2] = v[1]; i[2] = i[1]; v[1] = v[0]; i[1] = i[0]; v[0] = x; i[0] = ix; }
        else if (better(x, ix, v[1], i[1])) { v[3] = v[2]; i[3] = i[2]; v[2] = v[1]; i[2] = i[1]; v[1] = x; i[1] = ix; }
        else if (better(x, ix, v[2], i[2])) { v[3] = v[2]; i[3] = i[2]; v[2] = x; i[2] = ix; }
        else { v[3] = x; i[3] = ix; }
    }
};

struct KnnCall {                 // one call's segments and launch geometry
    std::vector<KnnSeg> seg;
    int ncols = 0, cq = 0;       // query columns; 256-query tiles (each segment's own)
    int units[3] = {0, 0, 0};    // workgroups of pass A, pass B, the exact kernel
    int ns_cv = 1;               // splits the exact kernel's lists are sized for
    bool two = false;            // some segment searches in two stages
};

struct KnnLists {        // where the merge kernels find the per-query top-4 lists
    float* cv = nullptr;    // exact kernel: [nsplit][ncols][4]
    int* ci = nullptr;
    float* rv = nullptr;    // two-stage search: [ncols][4]
    int* ri = nullptr;
    int* flag = nullptr;    // per segment: 0 = its two-stage lists are valid; nullptr = no segment searches in two stages
    int* col2seg = nullptr; // [ncols] (several segments)
    KnnSegs segs{};
};

// Segments from the callers' runs (in column order): adjacent runs of the same blob merge.  (knn.hip)
int knn_call_plan(tvc_ctx* ctx, const KnnSegIn* in, int nin, int ncols, KnnCall* c);
// query normalisation + the per-query top-4 lists of every segment (knn.hip; Bsrc: rows of src behind the B rows of queries, 0 = B)
int knn_candidates(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* src, const KnnCall& c, int B, int T, KnnLists* L, int Bsrc = 0);

}  // namespace tvc
