// Compacting a speaker index on the device: k-means over the raw vectors of a prepared blob (tvc_index_assign_f32 / _update_f32 /
// _compact_f32).  The reference has no counterpart: its extract_index.py:43-58 makes an index smaller by truncating a random
// permutation; this keeps K centroids instead (what RVC's index training and so-vits-svc's cluster model do on the host).
//
//   assign  the existing top-4 search (run_knn_topk, nothing of it changed) with the POINTS as queries against the prepared centroids,
//           in chunks of at most Q points: a chunk of raw rows is transposed into a [768][q] query tensor (ic_stage_kernel, either blob
//           kind, through an LDS tile), searched with B = 1, T = q, and column 0 of its lists becomes assign / sim (ic_take_kernel).
//   update  centroid k <- the mean of the raw vectors assigned to it, store-then-sum without floating-point atomics: a stable counting
//           sort of the point ids by cluster (per-chunk histograms, a plain three-launch exclusive scan in (cluster major, chunk minor)
//           order, a placement in which ONE wave walks its chunk in point order), then a wave per (cluster, run of IC_RUN members) sums its
//           members' rows in fp64 in rank order, and the partial sums of a cluster longer than one run are added in run order.  The order
//           of a cluster's sum is therefore a function of its members' ranks (ascending point index) alone: bit-identical from run to run,
//           whatever the grid, the scheduling or the number of histogram chunks.  No workgroup waits for another: every dependence is a
//           kernel boundary.
//
// Cosine assignment with a raw-mean update is the pair the match itself uses (a mean of raw vectors selected by cosine); it does not
// minimise one objective monotonically - moved[] (points that changed cluster per iteration) is what reports convergence.
#include <hip/hip_fp16.h>

#include "knn_blob.h"
#include "tvc_common.h"

namespace tvc {

namespace {

constexpr int IC_RUN = 256;            // members per (cluster, run) work unit of the mean kernel: a constant, so the summation order is a function of the rank alone
constexpr int IC_SCAN_PER = 16;        // elements per thread of the scan kernels
constexpr int IC_SCAN_TILE = 256 * IC_SCAN_PER;
constexpr long IC_HIST_MAX = 1L << 24; // histogram entries (clusters x chunks) the chunk count is chosen to stay under

// ---- staging: raw rows -> columns ------------------------------------------------------------------------------------------------
// dst[c * dstride + q] = row(n0 + q)[c] for q < ncols: rows of a blob of either kind (rows == nullptr), or plain fp32 rows [.][768].
// A 64-row x 64-channel tile meets in LDS as [c][r] (rows padded by one float): fp32 rows are read with lanes along c (256-byte runs),
// the fp16 image as whole 16-byte pieces with lanes along r (32 consecutive vectors of one (step, half) are 512 contiguous bytes), and
// the stores leave with lanes along q.  keep (optional): a column q with keep[q] == 0 is not written.
__global__ __launch_bounds__(256) void ic_stage_kernel(const float* __restrict__ blob, const float* __restrict__ rows, long N, long n0, int ncols,
                                                       float* __restrict__ dst, long dstride, const int* __restrict__ keep) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const int q0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int kind = rows ? KIND_F32 : blob_kind(blob);
    if (kind == KIND_F16) {
        const uint4* __restrict__ img = blob_img16(blob, KIND_F16, N, blob_npad(N));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pt = i * 256 + t, r = pt & 63, pc = pt >> 6;          // 8 pieces of 8 channels per row of the tile
            const long n = n0 + q0 + r;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (q0 + r < ncols) v = img[img_elem(n, c0 + pc * 8, 1) >> 3];
            const __half2* h = reinterpret_cast<const __half2*>(&v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 f = __half22float2(h[j]);
                tile[pc * 8 + 2 * j][r] = f.x;
                tile[pc * 8 + 2 * j + 1][r] = f.y;
            }
        }
    } else {
        const float* own = blob_rows(blob);      // (taken unconditionally: the choice below stays a select)
        const float* __restrict__ base = rows ? rows : own;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = i * 256 + t, r = e >> 6, c = e & 63;
            tile[c][r] = q0 + r < ncols ? base[(n0 + q0 + r) * KD + c0 + c] : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = i * 256 + t, c = e >> 6, r = e & 63;
        const int q = q0 + r;
        if (q < ncols && (!keep || keep[q] != 0)) dst[(long)(c0 + c) * dstride + q] = tile[c][r];
    }
}

// centroids[c][k] = point cols[k], channel c (a column outside [0, N) is clamped into the index, as the gather of the index build does)
__global__ __launch_bounds__(256) void ic_init_kernel(const float* __restrict__ blob, long N, const int64_t* __restrict__ cols, int K, float* __restrict__ cent) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    long n = cols[k];
    n = n < 0 ? 0 : (n >= N ? N - 1 : n);
    const int kind = blob_kind(blob);
    const int c = blockIdx.y;
    cent[(long)c * K + k] = blob_row_value(blob, kind, N, blob_npad(N), n, c);
}

// column 0 of a chunk's top-4 lists -> assign / sim; the entries that changed are counted with one integer atomic per wave
__global__ __launch_bounds__(256) void ic_take_kernel(const float* __restrict__ sims, const int64_t* __restrict__ idx, int ncols, int64_t* __restrict__ assign,
                                                      float* __restrict__ sim_out, int* __restrict__ moved) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if (q < ncols) {
        const int64_t a = idx[(long)q * 4];
        changed = assign[q] != a;
        assign[q] = a;
        if (sim_out) sim_out[q] = sims[(long)q * 4];
    }
    const unsigned long long m = __ballot(changed);
    if (moved && (threadIdx.x & 63) == 0 && m) atomicAdd(moved, __popcll(m));
}

// ---- counting sort of the point ids by cluster -----------------------------------------------------------------------------------
// hist[k * G + g] = points of chunk g (points [g * chunk, (g + 1) * chunk)) assigned to cluster k; an assignment outside [0, K) counts
// nowhere.  Integer atomics, each workgroup into entries no other workgroup touches.
__global__ __launch_bounds__(256) void ic_hist_kernel(const int64_t* __restrict__ assign, long N, int K, int G, long chunk, int* __restrict__ hist) {
    const int g = blockIdx.x;
    const long n1 = (g + 1) * chunk < N ? (g + 1) * chunk : N;
    for (long n = g * chunk + threadIdx.x; n < n1; n += 256) {
        const int64_t k = assign[n];
        if (k >= 0 && k < K) atomicAdd(&hist[k * G + g], 1);
    }
}

// exclusive scan of a[0 .. n) in place, three launches: tile sums, the scan of the tile sums (one workgroup), the tiles
__global__ __launch_bounds__(256) void ic_scan_sums_kernel(const int* __restrict__ a, long n, int* __restrict__ sums) {
    __shared__ int red[4];
    const long base = (long)blockIdx.x * IC_SCAN_TILE + threadIdx.x * IC_SCAN_PER;
    int s = 0;
#pragma unroll
    for (int i = 0; i < IC_SCAN_PER; ++i) s += base + i < n ? a[base + i] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// the exclusive prefix of v over the 256 threads of the workgroup
__device__ __forceinline__ int ic_block_exclusive(int v, int* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += red[i];
    __syncthreads();
    return off + inc - v;
}
__global__ __launch_bounds__(256) void ic_scan_top_kernel(int* __restrict__ sums, int nb) {
    __shared__ int red[4];
    const int per = (nb + 255) / 256;
    const int b0 = threadIdx.x * per;
    int s = 0;
    for (int i = 0; i < per; ++i) s += b0 + i < nb ? sums[b0 + i] : 0;
    int run = ic_block_exclusive(s, red);
    for (int i = 0; i < per && b0 + i < nb; ++i) {
        const int v = sums[b0 + i];
        sums[b0 + i] = run;
        run += v;
    }
}
__global__ __launch_bounds__(256) void ic_scan_tiles_kernel(int* __restrict__ a, long n, const int* __restrict__ sums) {
    __shared__ int red[4];
    const long base = (long)blockIdx.x * IC_SCAN_TILE + threadIdx.x * IC_SCAN_PER;
    int v[IC_SCAN_PER];
    int s = 0;
#pragma unroll
    for (int i = 0; i < IC_SCAN_PER; ++i) {
        v[i] = base + i < n ? a[base + i] : 0;
        s += v[i];
    }
    int run = sums[blockIdx.x] + ic_block_exclusive(s, red);
#pragma unroll
    for (int i = 0; i < IC_SCAN_PER; ++i) {
        if (base + i < n) a[base + i] = run;
        run += v[i];
    }
}

// Stable placement: ONE wave per chunk walks it in point order, 64 points at a time; a point's slot is its cluster's cursor for this
// chunk (the scanned histogram entry, advanced by an integer atomic of the wave that owns it) plus its rank among the lanes below it
// with the same cluster.  The cursors ARE the scanned histogram, advanced in place: afterwards entry (k, g) holds its END, so the
// cluster bounds are taken before this kernel (ic_runs_kernel).
__global__ __launch_bounds__(64) void ic_place_kernel(const int64_t* __restrict__ assign, long N, int K, int G, long chunk, int* __restrict__ cur, int* __restrict__ order) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const long n1 = (g + 1) * chunk < N ? (g + 1) * chunk : N;
    for (long nb = g * chunk; nb < n1; nb += 64) {
        const long n = nb + lane;
        const int64_t k = n < n1 ? assign[n] : -1;
        const bool valid = k >= 0 && k < K;
        unsigned long long rem = __ballot(valid);
        int rank = 0, cnt = 0, lead = lane;
        while (rem) {
            const int src = __ffsll((long long)rem) - 1;
            const int k0 = __shfl((int)k, src);
            const bool same = valid && (int)k == k0;
            const unsigned long long m = __ballot(same);
            if (same) {
                rank = __popcll(m & ((1ull << lane) - 1));
                cnt = __popcll(m);
                lead = src;
            }
            rem &= ~m;
        }
        int base = 0;
        if (valid && lead == lane) base = atomicAdd(&cur[k * G + g], cnt);
        base = __shfl(base, lead);
        if (valid) order[base + rank] = (int)n;
    }
}

// per cluster, from the scanned histogram (before the placement advances it): its first sorted position, its size, its runs and - for a
// cluster longer than one run - the partial-sum slots it takes; entry K of runs / slots is the scans' total
__global__ __launch_bounds__(256) void ic_runs_kernel(const int* __restrict__ start, int K, int G, int* __restrict__ first, int* __restrict__ counts, int* __restrict__ runs,
                                                      int* __restrict__ slots, int* __restrict__ counts_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    if (k == K) {
        runs[K] = 0;
        slots[K] = 0;
        return;
    }
    const int s = start[(long)k * G], c = start[(long)(k + 1) * G] - s;      // (the scanned array has K * G + 1 entries: the last is the total)
    const int r = (c + IC_RUN - 1) / IC_RUN;
    first[k] = s;
    counts[k] = c;
    if (counts_out) counts_out[k] = c;
    runs[k] = r;
    slots[k] = r > 1 ? r : 0;
}

// ---- the mean: one wave per (cluster, run) ---------------------------------------------------------------------------------------
// The wave reads a member's whole row as 16-byte pieces - fp32 rows: 64 lanes x 3 float4; the fp16 image: its 96 pieces of 8 channels,
// lanes 0 .. 31 two each -, four rows in flight, and adds them into fp64 accumulators in rank order.  A cluster of one run leaves as
// mean = (float)(sum / count) into mrows[k][768]; a longer one leaves fp64 partial sums [slot][768] for ic_combine_kernel.
__device__ __forceinline__ void ic_add4(double* acc, const float4 v) {
    acc[0] += (double)v.x;
    acc[1] += (double)v.y;
    acc[2] += (double)v.z;
    acc[3] += (double)v.w;
}
__device__ __forceinline__ void ic_add8h(double* acc, const uint4 v) {
    const __half2* h = reinterpret_cast<const __half2*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float2 f = __half22float2(h[j]);
        acc[2 * j] += (double)f.x;
        acc[2 * j + 1] += (double)f.y;
    }
}
__device__ __forceinline__ long ic_piece(long n, int p) {      // 16-byte piece p (channels 8 p .. 8 p + 7) of vector n in the fp16 image
    return img_elem(n, p * 8, 1) >> 3;
}

__global__ __launch_bounds__(256) void ic_mean_kernel(const float* __restrict__ blob, long N, const int* __restrict__ first, const int* __restrict__ counts,
                                                      const int* __restrict__ runs, const int* __restrict__ slots, const int* __restrict__ order, int K,
                                                      double* __restrict__ part, float* __restrict__ mrows) {
    const int lane = threadIdx.x & 63;
    const int u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (u >= runs[K]) return;
    int lo = 0, hi = K - 1;                       // the cluster whose runs [runs[k], runs[k + 1]) hold unit u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (runs[mid + 1] > u) hi = mid;
        else lo = mid + 1;
    }
    const int k = lo, r = u - runs[k];
    const int cnt = counts[k];
    const int m0 = first[k] + r * IC_RUN;
    const int m1 = first[k] + (cnt < (r + 1) * IC_RUN ? cnt : (r + 1) * IC_RUN);
    const bool single = cnt <= IC_RUN;
    const double dn = (double)cnt;
    const int kind = blob_kind(blob);
    if (kind == KIND_F16) {
        const uint4* __restrict__ img = blob_img16(blob, KIND_F16, N, blob_npad(N));
        const bool two = lane < 32;
        double acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0;
        for (int mb = m0; mb < m1; mb += 64) {
            const int nb = m1 - mb < 64 ? m1 - mb : 64;
            const int mine = lane < nb ? order[mb + lane] : 0;
            for (int j = 0; j < nb; j += 4) {
                uint4 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long n = __shfl(mine, (j + i) & 63);
                    a[i] = b[i] = make_uint4(0, 0, 0, 0);
                    if (j + i < nb) {
                        a[i] = img[ic_piece(n, lane)];
                        if (two) b[i] = img[ic_piece(n, lane + 64)];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j + i < nb) {
                        ic_add8h(acc, a[i]);
                        ic_add8h(acc + 8, b[i]);
                    }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ch = 8 * (lane + 64 * h);
            if (h == 1 && !two) {
            } else if (single) {
                float4 o0, o1;
                o0.x = (float)(acc[8 * h + 0] / dn);
                o0.y = (float)(acc[8 * h + 1] / dn);
                o0.z = (float)(acc[8 * h + 2] / dn);
                o0.w = (float)(acc[8 * h + 3] / dn);
                o1.x = (float)(acc[8 * h + 4] / dn);
                o1.y = (float)(acc[8 * h + 5] / dn);
                o1.z = (float)(acc[8 * h + 6] / dn);
                o1.w = (float)(acc[8 * h + 7] / dn);
                float4* o = reinterpret_cast<float4*>(mrows + (long)k * KD + ch);
                o[0] = o0;
                o[1] = o1;
            } else {
                double2* o = reinterpret_cast<double2*>(part + (long)(slots[k] + r) * KD + ch);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = make_double2(acc[8 * h + 2 * i], acc[8 * h + 2 * i + 1]);
            }
        }
    } else {
        const float4* __restrict__ rows = reinterpret_cast<const float4*>(blob_rows(blob));
        double acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
        for (int mb = m0; mb < m1; mb += 64) {
            const int nb = m1 - mb < 64 ? m1 - mb : 64;
            const int mine = lane < nb ? order[mb + lane] : 0;
            for (int j = 0; j < nb; j += 4) {
                float4 v[4][3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long n = __shfl(mine, (j + i) & 63);
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        v[i][p] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (j + i < nb) v[i][p] = rows[n * (KD / 4) + lane + 64 * p];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j + i < nb) {
#pragma unroll
                        for (int p = 0; p < 3; ++p) ic_add4(acc + 4 * p, v[i][p]);
                    }
            }
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int ch = 4 * (lane + 64 * p);
            if (single) {
                float4 o;
                o.x = (float)(acc[4 * p + 0] / dn);
                o.y = (float)(acc[4 * p + 1] / dn);
                o.z = (float)(acc[4 * p + 2] / dn);
                o.w = (float)(acc[4 * p + 3] / dn);
                *reinterpret_cast<float4*>(mrows + (long)k * KD + ch) = o;
            } else {
                double2* o = reinterpret_cast<double2*>(part + (long)(slots[k] + r) * KD + ch);
                o[0] = make_double2(acc[4 * p + 0], acc[4 * p + 1]);
                o[1] = make_double2(acc[4 * p + 2], acc[4 * p + 3]);
            }
        }
    }
}

// a cluster longer than one run: its partial sums added in run order, divided by its size in fp64, rounded once
__global__ __launch_bounds__(256) void ic_combine_kernel(const int* __restrict__ counts, const int* __restrict__ slots, const double* __restrict__ part,
                                                         float* __restrict__ mrows) {
    const int k = blockIdx.x;
    const int cnt = counts[k];
    if (cnt <= IC_RUN) return;
    const int nr = (cnt + IC_RUN - 1) / IC_RUN;
    const double* __restrict__ p = part + (long)slots[k] * KD;
    for (int c = threadIdx.x; c < KD; c += 256) {
        double s = p[c];
        for (int r = 1; r < nr; ++r) s += p[(long)r * KD + c];
        mrows[(long)k * KD + c] = (float)(s / (double)cnt);
    }
}

int ic_scan(tvc_ctx* ctx, hipStream_t s, int* a, long n, int* sums) {
    const int nb = (int)((n + IC_SCAN_TILE - 1) / IC_SCAN_TILE);
    hipLaunchKernelGGL(ic_scan_sums_kernel, dim3(nb), dim3(256), 0, s, (const int*)a, n, sums);
    hipLaunchKernelGGL(ic_scan_top_kernel, dim3(1), dim3(256), 0, s, sums, nb);
    hipLaunchKernelGGL(ic_scan_tiles_kernel, dim3(nb), dim3(256), 0, s, a, n, (const int*)sums);
    return launch_check(ctx, "index_update scan");
}
size_t ic_scan_tiles(long n) { return (size_t)((n + IC_SCAN_TILE - 1) / IC_SCAN_TILE); }

// histogram chunks: about 1024 points each, at most 256, fewer while clusters x chunks would pass IC_HIST_MAX; whole 64-point tiles.
// (The sort is stable for every chunk count: the result does not depend on this choice.)
void ic_chunks(int64_t N, int64_t K, int* G, long* chunk) {
    long g = (N + 1023) / 1024;
    g = g > 256 ? 256 : g;
    while (g > 1 && g * K > IC_HIST_MAX) g /= 2;
    long c = (N + g - 1) / g;
    c = (c + 63) / 64 * 64;
    *chunk = c;
    *G = (int)((N + c - 1) / c);
}

}  // namespace

int run_index_assign(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* points, int64_t N, const float* cent_blob, int64_t K, int64_t* assign, float* sim_out,
                     int32_t* moved) {
    const int64_t Q = ctx->index_assign_chunk > 0 ? ctx->index_assign_chunk : kIndexAssignChunk;
    const size_t m0 = ws.mark();
    for (int64_t n0 = 0; n0 < N; n0 += Q) {
        ws.release(m0);
        const int q = (int)(N - n0 < Q ? N - n0 : Q);
        float* stage = ws.get<float>((size_t)KD * q);
        float* sims = ws.get<float>((size_t)q * 4);
        int64_t* idx = ws.get<int64_t>((size_t)q * 4);
        if (!ws.dry) hipLaunchKernelGGL(ic_stage_kernel, dim3((q + 63) / 64, KD / 64), dim3(256), 0, s, points, (const float*)nullptr, (long)N, (long)n0, q, stage, (long)q, (const int*)nullptr);
        TVC_CHECK(run_knn_topk(ctx, s, ws, stage, cent_blob, K, sims, idx, 1, q));
        if (ws.dry) continue;
        hipLaunchKernelGGL(ic_take_kernel, dim3((q + 255) / 256), dim3(256), 0, s, (const float*)sims, (const int64_t*)idx, q, assign + n0, sim_out ? sim_out + n0 : nullptr, (int*)moved);
        TVC_CHECK(launch_check(ctx, "index_assign"));
    }
    ws.release(m0);
    return 0;
}

int run_index_update(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* points, int64_t N, const int64_t* assign, int64_t K, float* centroids, int32_t* counts_out) {
    int G;
    long chunk;
    ic_chunks(N, K, &G, &chunk);
    const long nh = (long)K * G + 1;
    const size_t m0 = ws.mark();
    int* hist = ws.get<int>((size_t)nh);
    int* sums = ws.get<int>(ic_scan_tiles(nh));
    int* order = ws.get<int>((size_t)N);
    int* first = ws.get<int>((size_t)K);
    int* counts = ws.get<int>((size_t)K);
    int* runs = ws.get<int>((size_t)K + 1);
    int* slots = ws.get<int>((size_t)K + 1);
    int* sums2 = ws.get<int>(ic_scan_tiles(K + 1));
    const size_t nslots = (size_t)(2 * N / IC_RUN) + 2;      // clusters longer than one run take ceil(c / IC_RUN) < 2 c / IC_RUN slots each
    double* part = ws.get<double>(nslots * KD);
    float* mrows = ws.get<float>((size_t)K * KD);
    ws.release(m0);
    if (ws.dry) return 0;
    TVC_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)nh * sizeof(int), s));
    hipLaunchKernelGGL(ic_hist_kernel, dim3(G), dim3(256), 0, s, assign, (long)N, (int)K, G, chunk, hist);
    TVC_CHECK(ic_scan(ctx, s, hist, nh, sums));
    hipLaunchKernelGGL(ic_runs_kernel, dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, s, (const int*)hist, (int)K, G, first, counts, runs, slots, (int*)counts_out);
    hipLaunchKernelGGL(ic_place_kernel, dim3(G), dim3(64), 0, s, assign, (long)N, (int)K, G, chunk, hist, order);
    TVC_CHECK(ic_scan(ctx, s, runs, K + 1, sums2));
    TVC_CHECK(ic_scan(ctx, s, slots, K + 1, sums2));
    const long units = (K < N ? K : N) + N / IC_RUN + 1;      // >= the sum of ceil(c / IC_RUN) over the non-empty clusters
    hipLaunchKernelGGL(ic_mean_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, points, (long)N, (const int*)first, (const int*)counts, (const int*)runs,
                       (const int*)slots, (const int*)order, (int)K, part, mrows);
    hipLaunchKernelGGL(ic_combine_kernel, dim3((unsigned)K), dim3(256), 0, s, (const int*)counts, (const int*)slots, (const double*)part, mrows);
    // rows -> the [768][K] layout of index.pt; an empty cluster's column is not written: it keeps its previous centroid bit for bit
    hipLaunchKernelGGL(ic_stage_kernel, dim3((unsigned)((K + 63) / 64), KD / 64), dim3(256), 0, s, (const float*)nullptr, (const float*)mrows, (long)K, 0L, (int)K, centroids,
                       (long)K, (const int*)counts);
    return launch_check(ctx, "index_update");
}

int run_index_compact(tvc_ctx* ctx, hipStream_t s, Ws& ws, const float* points, int64_t N, const int64_t* init_cols, int64_t K, int iters, float* centroids,
                      float* prepared_out, int64_t* assign_out, int32_t* counts_out, int32_t* moved_out) {
    int64_t* assign = assign_out ? assign_out : ws.get<int64_t>((size_t)N);
    if (!ws.dry) {
        hipLaunchKernelGGL(ic_init_kernel, dim3((unsigned)((K + 255) / 256), KD), dim3(256), 0, s, points, (long)N, init_cols, (int)K, centroids);
        TVC_CHECK(launch_check(ctx, "index_compact init"));
        TVC_HIP(ctx, hipMemsetAsync(assign, 0xff, (size_t)N * sizeof(int64_t), s));      // -1: every point moves in the first iteration
        if (moved_out) TVC_HIP(ctx, hipMemsetAsync(moved_out, 0, (size_t)iters * sizeof(int32_t), s));
    }
    for (int it = 0; it < iters; ++it) {
        if (!ws.dry) TVC_CHECK(run_prepare_index(ctx, s, centroids, prepared_out, K));
        TVC_CHECK(run_index_assign(ctx, s, ws, points, N, prepared_out, K, assign, nullptr, moved_out ? moved_out + it : nullptr));
        TVC_CHECK(run_index_update(ctx, s, ws, points, N, assign, K, centroids, counts_out));
        if (ws.dry) break;      // (every iteration takes the same workspace)
    }
    if (!ws.dry) TVC_CHECK(run_prepare_index(ctx, s, centroids, prepared_out, K));
    return 0;
}

}  // namespace tvc
