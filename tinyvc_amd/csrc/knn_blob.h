// Layout of a prepared kNN blob (knn_prepare.hip writes it; knn.hip, knn_gather.hip and index_compact.hip read it; api.hip sizes and checks it).
// Every offset, header word and size of a blob is stated here and nowhere else.
#pragma once
#include <hip/hip_fp16.h>

#include "tvc_common.h"

namespace tvc {

constexpr int KD = kSslDim;        // 768
constexpr int STEPS = KD / 16;     // 48 K16 steps per index tile
constexpr int HDR = 64;            // blob header, floats (the words below; the rest is zero)
constexpr int KIND_F32 = 0, KIND_F16 = 1;
constexpr int BLOB_MAGIC = kBlobMagic;
// header words (32 bits each; kBlobMagic, kBlobVersion: tvc_common.h; AMAX: |max| of the raw vectors, a float; WORDS: what a reader fetches)
constexpr int BLOB_W_MAGIC = 0, BLOB_W_KIND = 1, BLOB_W_N_LO = 2, BLOB_W_N_HI = 3, BLOB_W_AMAX = 4, BLOB_W_VERSION = 5, BLOB_WORDS = 6;
// fp32 kind:  header | rows fp32 [N][768] | bf16x3 image of v / den [Npad*768*3 bf16] | inv = 1 / den [Npad] | fp16 image of v / den [Npad*768]
// fp16 kind:  header | inv [Npad] | fp16 image of the raw vectors [Npad*768] | largest inv of every 128-vector tile [Npad/128]
// (both fp16 images in the 128-vector-tiled MFMA lane order, one part; Npad = N rounded up to whole 128-vector tiles)
__host__ __device__ inline long blob_npad(long N) { return (N + 127) / 128 * 128; }
// floats of a blob of N vectors (tvc_knn_prepared_elems / _f16)
inline int64_t blob_elems(int kind, int64_t N) {
    const int64_t Npad = blob_npad(N);
    if (kind == KIND_F16) return HDR + Npad + (int64_t)KD * Npad / 2 + Npad / 128;
    return HDR + N * (int64_t)KD + (int64_t)KD * Npad * 3 / 2 + Npad + (int64_t)KD * Npad / 2;
}
__device__ __forceinline__ int blob_kind(const float* blob) { return reinterpret_cast<const int*>(blob)[BLOB_W_KIND]; }
// the |max| word: `matched` (a mean of four raw rows) is bounded by it, so the conversion takes the |max| slot of the decoder's content
// input from here instead of a pass over the tensor (block-floating-point guard, split_fp16.h)
__host__ __device__ inline const float* blob_amax(const float* blob) { return blob + BLOB_W_AMAX; }
__host__ __device__ inline const float* blob_rows(const float* blob) { return blob + HDR; }      // fp32 kind only
__host__ __device__ inline const uint4* blob_img3(const float* blob, long N) { return reinterpret_cast<const uint4*>(blob + HDR + (size_t)N * KD); }      // fp32 kind only
__host__ __device__ inline const float* blob_inv(const float* blob, int kind, long N, long Npad) {
    return kind == KIND_F16 ? blob + HDR : blob + HDR + (size_t)N * KD + (size_t)Npad * KD * 3 / 2;
}
__host__ __device__ inline const uint4* blob_img16(const float* blob, int kind, long N, long Npad) {
    return reinterpret_cast<const uint4*>(blob_inv(blob, kind, N, Npad) + Npad);
}
__host__ __device__ inline const float* blob_invmax(const float* blob, long Npad) {      // fp16 kind only
    return blob + HDR + Npad + (size_t)Npad * KD / 2;
}
// element (vector n, channel k) of a 128-vector-tiled MFMA-ordered image with P parts per (m-tile, step): the index of
// part 0's 8-value piece row; row = lane & 31, k = 16 step + 8 (lane >> 5) + j
__device__ __forceinline__ long img_elem(long n, int k, int parts) {
    const long tile = n >> 7;
    const int mt = (int)(n & 127) >> 5, l31 = (int)(n & 31);
    const int step = k >> 4, lh = (k >> 3) & 1, j = k & 7;
    return ((((tile * STEPS + step) * 4 + mt) * parts) * 64 + (lh * 32 + l31)) * 8 + j;
}

// raw vector value (n, k) of either blob kind (the gathers)
__device__ __forceinline__ float blob_row_value(const float* __restrict__ blob, int kind, long N, long Npad, long n, int k) {
    if (kind == KIND_F16) return __half2float(reinterpret_cast<const __half*>(blob + HDR + Npad)[img_elem(n, k, 1)]);      // blob_img16, as halves
    return blob[HDR + n * KD + k];                                                                                         // blob_rows(blob)[n][k]
}

}  // namespace tvc
