// Everything that writes a prepared kNN blob (layout: knn_blob.h): from an index tensor (fp32 or fp16 storage) and from a column
// selection of packed features, gathered straight into the blob.  The search that reads the blobs is knn.hip.
#include "knn_blob.h"
#include "tvc_common.h"

namespace tvc {

template <class T>
static T* writable(const T* p) { return const_cast<T*>(p); }      // knn_blob.h's accessors are the readers'; this file is the writer

static __global__ void blob_header_kernel(float* blob, int kind, long N) {
    int* h = reinterpret_cast<int*>(blob);
    if (threadIdx.x < HDR) h[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        h[BLOB_W_MAGIC] = BLOB_MAGIC;
        h[BLOB_W_KIND] = kind;
        h[BLOB_W_N_LO] = (int)(N & 0xffffffffL);
        h[BLOB_W_N_HI] = (int)(N >> 32);
        h[BLOB_W_VERSION] = kBlobVersion;
    }
}

// the three-term bf16 split of one value (v = h1 + h2 + h3, residuals exact), as bit patterns
__device__ __forceinline__ void split_bf3(float v, unsigned short& h1, unsigned short& h2, unsigned short& h3) {
    const __bf16 b1 = (__bf16)v;
    const float r = v - (float)b1;
    const __bf16 b2 = (__bf16)r;
    const float r2 = r - (float)b2;
    const __bf16 b3 = (__bf16)r2;
    h1 = __builtin_bit_cast(unsigned short, b1);
    h2 = __builtin_bit_cast(unsigned short, b2);
    h3 = __builtin_bit_cast(unsigned short, b3);
}

// fp32 storage.  index [768][N] (the [1,768,N] tensor of index.pt) -> raw rows + the bf16x3 image of v / (||v|| + 1e-6)
// (feature_retrieval.py:25 recomputes that normalisation on every call).  One thread per vector; reads run along n.
static __global__ void index_prepare_kernel(const float* __restrict__ index, float* __restrict__ rows,
                                            unsigned short* __restrict__ img, float* __restrict__ inv, __half* __restrict__ img16,
                                            long N, long Npad) {
    long n = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (n >= Npad) return;
    float den = 1.f;
    if (n < N) {
        float s = 0.f;
        for (int k = 0; k < KD; ++k) {
            float v = index[(long)k * N + n];
            s = fmaf(v, v, s);
        }
        den = sqrtf(s) + 1e-6f;
    }
    inv[n] = n < N ? 1.f / den : 0.f;
    for (int k = 0; k < KD; ++k) {
        float raw = n < N ? index[(long)k * N + n] : 0.f;
        if (n < N) rows[n * KD + k] = raw;
        float v = raw / den;
        img16[img_elem(n, k, 1)] = __float2half(v);      // the coarse pass's operand (knn_coarse_kernel)
        const long base = img_elem(n, k, 3);
        split_bf3(v, img[base], img[base + 512], img[base + 1024]);
    }
}

// fp16 storage.  rows16 [N][768] IEEE half (row-major: one vector per row) -> inverse norms + the fp16 image.
// One wavefront per vector: lanes run along k (coalesced 128-byte reads), the norm is a fixed-order wave reduction.
static __global__ __launch_bounds__(256) void index_prepare_f16_kernel(const __half* __restrict__ rows16, float* __restrict__ inv,
                                                                       __half* __restrict__ img, long N, long Npad) {
    const int lane = threadIdx.x & 63;
    const long n = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 6;
    if (n >= Npad) return;
    float s = 0.f;
    for (int k = lane; k < KD; k += 64) {
        const __half h = n < N ? rows16[n * KD + k] : __float2half(0.f);
        const float v = __half2float(h);
        s = fmaf(v, v, s);
        img[img_elem(n, k, 1)] = h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) inv[n] = n < N ? 1.f / (sqrtf(s) + 1e-6f) : 0.f;
}

// a workgroup's (4 waves) largest |value| -> the blob's |max| word (blob_amax)
__device__ __forceinline__ void amax_flush(float mx, float* red, float* __restrict__ slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(slot), __builtin_bit_cast(unsigned, m));      // non-negative floats order like their bits; NaN never enters
    }
}
// the largest |value| of the index
template <class T>
static __global__ __launch_bounds__(256) void index_amax_kernel(const T* __restrict__ p, long n, float* __restrict__ slot) {
    __shared__ float red[4];
    float mx = 0.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) mx = fmaxf(mx, fabsf((float)p[i]));
    amax_flush(mx, red, slot);
}

int run_prepare_index(tvc_ctx* ctx, hipStream_t s, const float* index, float* prepared, int64_t N) {
    const long Npad = blob_npad(N);
    hipLaunchKernelGGL(blob_header_kernel, dim3(1), dim3(64), 0, s, prepared, KIND_F32, (long)N);
    float* rows = writable(blob_rows(prepared));
    unsigned short* img = reinterpret_cast<unsigned short*>(writable(blob_img3(prepared, N)));
    float* inv = writable(blob_inv(prepared, KIND_F32, N, Npad));
    __half* img16 = reinterpret_cast<__half*>(writable(blob_img16(prepared, KIND_F32, N, Npad)));
    hipLaunchKernelGGL(index_prepare_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, index, rows, img, inv, img16, (long)N, Npad);
    hipLaunchKernelGGL(index_amax_kernel<float>, dim3(64), dim3(256), 0, s, index, (long)N * KD, writable(blob_amax(prepared)));
    return launch_check(ctx, "knn_prepare_index");
}

static __global__ void index_invmax_kernel(const float* __restrict__ inv, float* __restrict__ invmax, long ntiles) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    float m = 0.f;
    for (int i = 0; i < 128; ++i) m = fmaxf(m, inv[t * 128 + i]);
    invmax[t] = m;
}

int run_prepare_index_f16(tvc_ctx* ctx, hipStream_t s, const void* rows16, float* prepared, int64_t N) {
    const long Npad = blob_npad(N);
    hipLaunchKernelGGL(blob_header_kernel, dim3(1), dim3(64), 0, s, prepared, KIND_F16, (long)N);
    float* inv = writable(blob_inv(prepared, KIND_F16, N, Npad));
    __half* img = reinterpret_cast<__half*>(writable(blob_img16(prepared, KIND_F16, N, Npad)));
    hipLaunchKernelGGL(index_prepare_f16_kernel, dim3((unsigned)((Npad * 64 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const __half*>(rows16), inv, img, (long)N, Npad);
    hipLaunchKernelGGL(index_invmax_kernel, dim3((unsigned)((Npad / 128 + 255) / 256)), dim3(256), 0, s, inv, writable(blob_invmax(prepared, Npad)), Npad / 128);
    hipLaunchKernelGGL(index_amax_kernel<__half>, dim3(64), dim3(256), 0, s, reinterpret_cast<const __half*>(rows16), (long)N * KD, writable(blob_amax(prepared)));
    return launch_check(ctx, "knn_prepare_index_f16");
}

// ---- an index gathered straight into a blob ---------------------------------------------------------------------------------
// extract_index.py:43-58 selects index vectors out of the clips' features (every stride-th frame, permuted, truncated); here the
// selection is a column list into packed features [768][S] and the selected vectors go straight into a prepared blob, byte for byte
// the blob run_prepare_index / run_prepare_index_f16 make of feats[:, cols].  One workgroup per 128-vector image tile:
//   * the column gather is element-granular (lanes along n read feats[k][cols[n]]: every lane its own cache line, served by L2 / the
//     Infinity Cache - all tiles walk the channels in the same order), 32 independent loads per thread in flight;
//   * a 64-channel chunk of the tile meets in LDS ([k][n], rows padded by one float: lanes along n and lanes along k are both
//     conflict-free), and every store leaves with its lanes along the fast axis of its destination: raw rows in 256-byte runs,
//     index_out along n, the images as whole 16-byte pieces (img_elem keeps the 8 j of one (n, step, lh) adjacent: 1 KiB per wave).
// What byte identity pins: the norm's summation order (fp32 kind: ONE fmaf chain over k ascending per vector; fp16 kind: 64 lane-strided
// chains, k = lane + 64 c, then the xor butterfly), raw / den as a division - restated below as they stand in index_prepare_kernel /
// index_prepare_f16_kernel - and the three-term bf16 split, which both fp32 kernels take from split_bf3.
constexpr int GP_KC = 64;             // channels per chunk: 4 K16 steps, one raw-row run of 256 bytes
constexpr int GP_LD = 128 + 1;        // LDS row stride in floats
static_assert(KD % GP_KC == 0 && GP_KC == 64, "the fp16 kind's lane-strided chains take one term per chunk");

// a column outside [0, S) never leaves the tensor (the host's column plan refuses it first: feature_retrieval.py index_columns)
__device__ __forceinline__ long gp_column(const int64_t* __restrict__ cols, long n, long N, long S) {
    const long c = n < N ? (long)cols[n] : 0;
    return c < 0 ? 0 : (c >= S ? S - 1 : c);
}
__device__ __forceinline__ unsigned gp_pack(unsigned short lo, unsigned short hi) { return (unsigned)lo | ((unsigned)hi << 16); }

// fp32 storage.  Pass 1: gather, norm chain, raw rows, index_out, |max|.  Pass 2: the tile's own rows (just written: L2-hot, contiguous)
// come back through LDS and leave as the bf16x3 and fp16 images of v / den.
static __global__ __launch_bounds__(256) void index_gather_prepare_kernel(const float* __restrict__ feats, long S, const int64_t* __restrict__ cols,
                                                                          float* rows, uint4* __restrict__ img, float* __restrict__ inv,
                                                                          uint4* __restrict__ img16, float* __restrict__ index_out,
                                                                          float* __restrict__ slot, long N) {
    __shared__ float tile[GP_KC * GP_LD];
    __shared__ float den_s[128];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n0 = blockIdx.x * 128L;
    const int gn = tid & 127, gh = tid >> 7;      // the gather: vector gn of the tile, channels 32 gh ... of the chunk
    const long n = n0 + gn;
    const bool live = n < N;
    const float* src = feats + gp_column(cols, n, N, S);
    float s = 0.f, mx = 0.f;
    for (int k0 = 0; k0 < KD; k0 += GP_KC) {
        float x[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) x[i] = src[(long)(k0 + gh * 32 + i) * S];      // (a vector beyond N reads column 0 and drops it)
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float v = live ? x[i] : 0.f;
            tile[(gh * 32 + i) * GP_LD + gn] = v;
            mx = fmaxf(mx, fabsf(v));
            if (index_out && live) index_out[(long)(k0 + gh * 32 + i) * N + n] = v;
        }
        __syncthreads();
        if (tid < 128) {      // thread t owns vector t's chain (gn == tid): k ascending, one accumulator
#pragma unroll 16
            for (int k = 0; k < GP_KC; ++k) {
                const float v = tile[k * GP_LD + tid];
                s = fmaf(v, v, s);
            }
        }
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {      // raw rows: a wave writes channels k0 ... k0 + 63 of one vector
            const int r = wave * 32 + j;
            if (n0 + r < N) rows[(n0 + r) * KD + k0 + lane] = tile[lane * GP_LD + r];
        }
        __syncthreads();
    }
    amax_flush(mx, red, slot);
    if (tid < 128) {
        const float den = live ? sqrtf(s) + 1e-6f : 1.f;
        den_s[tid] = den;
        inv[n] = live ? 1.f / den : 0.f;
    }
    __syncthreads();
    const int nl = wave * 32 + (lane & 31), lh = lane >> 5;      // pass 2: wave = m-tile, lane = (lh, vector & 31) - the MFMA lane of the piece
    const float den = den_s[nl];
    for (int k0 = 0; k0 < KD; k0 += GP_KC) {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
            const int r = wave * 32 + j;
            tile[lane * GP_LD + r] = n0 + r < N ? rows[(n0 + r) * KD + k0 + lane] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < GP_KC / 16; ++st) {
            unsigned short b1[8], b2[8], b3[8], hf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float raw = tile[(st * 16 + lh * 8 + j) * GP_LD + nl];
                float v = raw / den;
                hf[j] = __half_as_ushort(__float2half(v));
                split_bf3(v, b1[j], b2[j], b3[j]);
            }
            const long piece = ((long)blockIdx.x * STEPS + (k0 >> 4) + st) * 4 + wave;      // img_elem / 8 = (piece * parts + part) * 64 + lane
            img[(piece * 3 + 0) * 64 + lane] = make_uint4(gp_pack(b1[0], b1[1]), gp_pack(b1[2], b1[3]), gp_pack(b1[4], b1[5]), gp_pack(b1[6], b1[7]));
            img[(piece * 3 + 1) * 64 + lane] = make_uint4(gp_pack(b2[0], b2[1]), gp_pack(b2[2], b2[3]), gp_pack(b2[4], b2[5]), gp_pack(b2[6], b2[7]));
            img[(piece * 3 + 2) * 64 + lane] = make_uint4(gp_pack(b3[0], b3[1]), gp_pack(b3[2], b3[3]), gp_pack(b3[4], b3[5]), gp_pack(b3[6], b3[7]));
            img16[piece * 64 + lane] = make_uint4(gp_pack(hf[0], hf[1]), gp_pack(hf[2], hf[3]), gp_pack(hf[4], hf[5]), gp_pack(hf[6], hf[7]));
        }
        __syncthreads();
    }
}

// fp16 storage: no raw rows, one pass.  The chunk holds the fp16-rounded values (as floats); wave w keeps the 64 lane-strided chains of its
// 32 vectors in registers (chunk c is term c of every chain) and folds them with the butterfly behind the last chunk.
static __global__ __launch_bounds__(256) void index_gather_prepare_f16_kernel(const float* __restrict__ feats, long S, const int64_t* __restrict__ cols,
                                                                              float* __restrict__ inv, uint4* __restrict__ img, float* __restrict__ invmax,
                                                                              __half* __restrict__ index_out, float* __restrict__ slot, long N) {
    __shared__ float tile[GP_KC * GP_LD];
    __shared__ float red[4];
    __shared__ float imx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n0 = blockIdx.x * 128L;
    const int gn = tid & 127, gh = tid >> 7;
    const long n = n0 + gn;
    const bool live = n < N;
    const float* src = feats + gp_column(cols, n, N, S);
    const int nl = wave * 32 + (lane & 31), lh = lane >> 5;
    float p[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) p[j] = 0.f;
    float mx = 0.f;
    for (int k0 = 0; k0 < KD; k0 += GP_KC) {
        float x[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) x[i] = src[(long)(k0 + gh * 32 + i) * S];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const __half h = __float2half(live ? x[i] : 0.f);
            const float v = __half2float(h);
            tile[(gh * 32 + i) * GP_LD + gn] = v;
            mx = fmaxf(mx, fabsf(v));
            if (index_out && live) index_out[(long)(k0 + gh * 32 + i) * N + n] = h;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float v = tile[lane * GP_LD + wave * 32 + j];
            p[j] = fmaf(v, v, p[j]);
        }
#pragma unroll
        for (int st = 0; st < GP_KC / 16; ++st) {
            unsigned short hf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) hf[j] = __half_as_ushort(__float2half(tile[(st * 16 + lh * 8 + j) * GP_LD + nl]));      // exact: the values are halves
            const long piece = ((long)blockIdx.x * STEPS + (k0 >> 4) + st) * 4 + wave;
            img[piece * 64 + lane] = make_uint4(gp_pack(hf[0], hf[1]), gp_pack(hf[2], hf[3]), gp_pack(hf[4], hf[5]), gp_pack(hf[6], hf[7]));
        }
        __syncthreads();
    }
    amax_flush(mx, red, slot);
    float wmax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        float s = p[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const long r = n0 + wave * 32 + j;
        const float iv = r < N ? 1.f / (sqrtf(s) + 1e-6f) : 0.f;
        if (lane == 0) inv[r] = iv;
        wmax = fmaxf(wmax, iv);
    }
    if (lane == 0) imx[wave] = wmax;
    __syncthreads();
    if (tid == 0) invmax[blockIdx.x] = fmaxf(fmaxf(fmaxf(fmaxf(0.f, imx[0]), imx[1]), imx[2]), imx[3]);      // the tile's largest inverse norm (index_invmax_kernel)
}

int run_prepare_index_cols(tvc_ctx* ctx, hipStream_t s, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared, float* index_out) {
    const long Npad = blob_npad(N);
    hipLaunchKernelGGL(blob_header_kernel, dim3(1), dim3(64), 0, s, prepared, KIND_F32, (long)N);
    float* rows = writable(blob_rows(prepared));
    uint4* img = writable(blob_img3(prepared, N));
    float* inv = writable(blob_inv(prepared, KIND_F32, N, Npad));
    uint4* img16 = writable(blob_img16(prepared, KIND_F32, N, Npad));
    hipLaunchKernelGGL(index_gather_prepare_kernel, dim3((unsigned)(Npad / 128)), dim3(256), 0, s, feats, (long)S, cols, rows, img, inv, img16, index_out,
                       writable(blob_amax(prepared)), (long)N);
    return launch_check(ctx, "knn_prepare_index_cols");
}

int run_prepare_index_cols_f16(tvc_ctx* ctx, hipStream_t s, const float* feats, int64_t S, const int64_t* cols, int64_t N, float* prepared, void* index_out_f16) {
    const long Npad = blob_npad(N);
    hipLaunchKernelGGL(blob_header_kernel, dim3(1), dim3(64), 0, s, prepared, KIND_F16, (long)N);
    float* inv = writable(blob_inv(prepared, KIND_F16, N, Npad));
    uint4* img = writable(blob_img16(prepared, KIND_F16, N, Npad));
    hipLaunchKernelGGL(index_gather_prepare_f16_kernel, dim3((unsigned)(Npad / 128)), dim3(256), 0, s, feats, (long)S, cols, inv, img,
                       writable(blob_invmax(prepared, Npad)), reinterpret_cast<__half*>(index_out_f16), writable(blob_amax(prepared)), (long)N);
    return launch_check(ctx, "knn_prepare_index_cols_f16");
}

}  // namespace tvc
