// Split-fp16 arithmetic: the scheme every MFMA kernel of the library follows for fp32-equivalent accuracy on the fp16 matrix
// pipe, and the helpers that carry it out.  Every fp32 operand is split into TWO fp16 parts, x = h1 + 2^-11 h2 with
// h1 = fp16(x), h2 = fp16((x - h1) * 2^11) (the residual is exact in fp32; the 2^11 keeps it out of fp16's subnormal range),
// 22 significand bits in all, and a product is accumulated in fp32 from THREE part-products: h1 w1 into one accumulator,
// h1 w2 + h2 w1 (the 2^-11-order terms, in units of 2^-11) into a second one; out = acc_hi + 2^-11 acc_lo.  The dropped
// h2 w2 term is <= 2^-24 relative.  Measured against fp64 on the part (tools/micro/f16split.hip, K = 768): 1.9e-7 rel rms,
// vs 4.9e-7 for the fp32 MFMA and 4.2e-7 for the bf16 x 3 / six-product split this replaces (which spent twice the
// matrix-pipe cycles, 1.5x the LDS bytes and 1.5x the split arithmetic).  v_mfma_f32_32x32x16_f16 keeps fp16 subnormals
// (measured), so the absolute error floor of an operand is 2^-36 of its scale unit.
//
// Range guard (block floating point).  fp16 tops out at 65504, so every operand travels with a power-of-two scale:
//   weights      normalised per 32-row m-tile at pack time (largest |w| of the tile in [1, 2)), the exponent comes back
//                in the epilogue (PackedW::wscale);
//   activations  every tensor that is read as a B operand has a per-utterance |max| slot, written by the kernel that
//                produces it (running max of the values it stores, one atomicMax per wave when it grows); the consuming
//                kernel multiplies by 2^-e while staging and by 2^e in its epilogue, e = floor(log2 amax), whenever amax
//                is outside [2^-10, 2^15) - inside that window e = 0 and nothing is scaled.  Intermediates that never leave
//                the CU (fused blocks) use the bound sum|w| * amax_in + max|b| instead of a measured maximum.
#pragma once
#include "tvc_common.h"

namespace tvc {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));   // one 32 x 32 MFMA accumulator per lane
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // register-friendly 16-byte value (HIP's uint4 struct defeats SROA in arrays)

constexpr int kParts = 2;                 // fp16 parts per fp32 operand
constexpr int kPU4 = kParts * 64;         // uint4 per (K16 step, m-tile) of a weight image
constexpr float kLoScale = 2048.f;        // h2 = fp16((x - h1) * 2^11)
constexpr float kLoInv = 1.f / 2048.f;

// power-of-two input scale from a tensor's per-utterance |max|: identity while amax is inside [2^-10, 2^15), else 2^-floor(log2 amax)
struct Bfp {
    float s, inv;
};
__device__ __forceinline__ Bfp bfp_from_amax(float amax) {
    const unsigned u = __builtin_bit_cast(unsigned, amax);
    int e = (int)(u >> 23) - 127;
    Bfp r{1.f, 1.f};
    if (u != 0u && u < 0x7f800000u && (e >= 15 || e < -10)) {     // zero, Inf and NaN carry no information: no scaling
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        r.s = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
        r.inv = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    }
    return r;
}
__device__ __forceinline__ Bfp bfp_load(const float* amax, int b) { return amax ? bfp_from_amax(amax[b]) : Bfp{1.f, 1.f}; }
// A slot read through the SCALAR cache (the address must be wave-uniform).  The persistent fused kernels read their utterance's slots at
// the top of every tile; as a vector load (the compiler cannot prove a global store does not alias them) each read was followed by
// `s_waitcnt vmcnt(0)` - i.e. every tile began by waiting for ALL of the previous tile's stores to be acknowledged (cycle stamps
// of the fused ups.4 kernels, round 5: 2-3 k of a 13 k-cycle tile).  Slots are written by EARLIER launches (caches are invalidated at launch boundaries),
// so the scalar path is coherent; it counts on lgkmcnt and leaves the store queue alone.
__device__ __forceinline__ float sload_f32(const float* p) {
    float v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
__device__ __forceinline__ Bfp bfp_load_u(const float* amax, int b) { return amax ? bfp_from_amax(sload_f32(amax + b)) : Bfp{1.f, 1.f}; }
// the smaller of two scales (two tensors accumulated into one tile share it)
__device__ __forceinline__ Bfp bfp_min(const Bfp& a, const Bfp& b) { return a.s < b.s ? a : b; }
// Publishing a |max| slot.  Same-address device-scope atomics complete at ~3 per microsecond on this part (measured: one
// atomicMax per wave and tile - 200 k per launch on 64 slots - added 1 ms to a 0.3 ms kernel), so they are kept to a handful per
// slot and launch: persistent kernels walk CONTIGUOUS tile ranges (a workgroup meets one or two utterances), every wave keeps a
// running maximum in a register, and when the workgroup moves on to another utterance (and at its end) the waves' maxima meet in
// LDS and ONE thread issues ONE atomic, fire-and-forget (reading the slot first to skip it made the wave wait for that load and,
// with it, for the next tile's prefetch).  Non-negative floats order like their bit patterns; NaNs never enter a maximum (fmaxf).
__device__ __forceinline__ float wave_max(float mx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    return mx;
}
// every thread of the workgroup calls it (it contains a barrier); red = LDS scratch of >= (workgroup waves) floats
__device__ __forceinline__ void amax_flush_wg(float* slot, float mx, float* red) {
    mx = wave_max(mx);
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));      // (the LDS address below is not worth a register held - or spilled - across the caller's tile loop)
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (tid == 0) {
        float m = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
        if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(slot), __builtin_bit_cast(unsigned, m));
    }
    // (red is rewritten at this workgroup's next flush, at least one tile - several barriers - later)
}
// contiguous tile range of persistent workgroup w of g: [first, last)
__device__ __forceinline__ void tile_range(int ntiles, int& first, int& last) {
    first = (int)((long)ntiles * blockIdx.x / gridDim.x);
    last = (int)((long)ntiles * (blockIdx.x + 1) / gridDim.x);
}

// Global accesses as uniform base (SGPR pair) + 32-bit byte offset per lane (the global_load saddr form): the row bases are
// pinned into SGPRs through an empty asm, otherwise the compiler re-associates base + row stride into chains of 64-bit
// vector adds (one v_lshl_add_u64 per load).
typedef const __attribute__((address_space(1))) float* gcf32;
typedef __attribute__((address_space(1))) float* gf32;
__device__ __forceinline__ float ldg_so(const float* base, unsigned byte_off) {
    gcf32 p = (gcf32)base;
    asm("" : "+s"(p));
    return *reinterpret_cast<gcf32>(reinterpret_cast<const __attribute__((address_space(1))) char*>(p) + byte_off);
}
__device__ __forceinline__ void stg_so(float* base, unsigned byte_off, float v) {
    gf32 p = (gf32)base;
    asm("" : "+s"(p));
    *reinterpret_cast<gf32>(reinterpret_cast<__attribute__((address_space(1))) char*>(p) + byte_off) = v;
}
__device__ __forceinline__ void stg_so4(float* base, unsigned byte_off, const float (&v)[4]) {
    typedef float f32x4g __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) f32x4g* gf4;
    gf32 p = (gf32)base;
    asm("" : "+s"(p));
    *reinterpret_cast<gf4>(reinterpret_cast<__attribute__((address_space(1))) char*>(p) + byte_off) = f32x4g{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ u32x4 ldg_so4(const uint4* base, unsigned byte_off) {
    typedef const __attribute__((address_space(1))) u32x4* gcu4;
    gcu4 p = (gcu4)base;
    asm("" : "+s"(p));
    return *reinterpret_cast<gcu4>(reinterpret_cast<const __attribute__((address_space(1))) char*>(p) + byte_off);
}

// The two parts of a pair of fp32 values: h1 = fp16(v) (packed), h2 = fp16((v - h1) * S), S = kLoScale (or 1: film_s2.h).
// The second part is ONE v_fma_mix per value - fp16(fma(h1, -S, v * S)), the fp16 operand read straight from h1's register half -
// instead of convert-back, subtract, scale, convert: four vector instructions per pair instead of six, on the path every staged
// activation takes.  The product h1 * S and the difference are exact in fp32, so the single rounding equals the four-step result bit for
// bit (tools/micro/split_mix.hip: 2 M pairs over the whole exponent range, none different).
template <bool SCALED = true>
__device__ __forceinline__ void split2(float v0, float v1, unsigned& p1, unsigned& p2) {
    const f32x2 a = {v0, v1};
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(a, f16x2v));
    const f32x2 b = SCALED ? a * kLoScale : a;
    const float ns = SCALED ? -kLoScale : -1.f;
    unsigned r;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(p1), "s"(ns), "v"(b[0]));
    asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r) : "v"(p1), "s"(ns), "v"(b[1]));
    p2 = r;
}
// two fp16 parts of 8 fp32 values (v = h1 + 2^-11 h2), packed for one 16-byte LDS row each
__device__ __forceinline__ void split8(const float (&v)[8], uint4& p1, uint4& p2) {
    unsigned o1[4], o2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split2(v[2 * j], v[2 * j + 1], o1[j], o2[j]);
    p1 = make_uint4(o1[0], o1[1], o1[2], o1[3]);
    p2 = make_uint4(o2[0], o2[1], o2[2], o2[3]);
}
// acc_hi += w1 x1;  acc_lo += w2 x1 + w1 x2   (one K16 step of one 32 x 32 tile)
#define TVC_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
// out = acc_hi * c + acc_lo * (c / 2048)
__device__ __forceinline__ float comb(float hi, float lo, float c, float clo) { return fmaf(lo, clo, hi * c); }

// workgroup barrier that drains this wave's LDS traffic but not its global loads
__device__ __forceinline__ void slab_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// per-utterance |max| slots of a launch's tensors (block-floating-point guard, see the top of this file): x / cond are read
// (nullptr = the tensor is known to sit inside the fp16 window: no scaling), y is written (nullptr = nobody needs it)
struct BfpSlots {
    const float* x = nullptr;
    const float* c = nullptr;
    float* y = nullptr;
};

// Per-utterance |max| of a [B][C][len] tensor into slot[b] (zeroed first): the block-floating-point slot of a tensor whose
// producer does not track it (tensors that enter a stage through the C ABI, epilogue-functor outputs).  One pass over the tensor.
static __global__ __launch_bounds__(256) void amax_rows_kernel(const float* __restrict__ x, long n, float* __restrict__ slot) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const float* p = x + (long)b * n;
    float mx = 0.f;
    if ((n & 3) == 0) {                      // rows are whole float4s (and 16-byte aligned: workspace tensors are 256-byte aligned)
        for (long i = blockIdx.x * 256L + threadIdx.x; i < (n >> 2); i += (long)gridDim.x * 256) {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) mx = fmaxf(mx, fabsf(p[i]));
    }
    amax_flush_wg(slot + b, mx, red);
}
// ragged batch (ragged.h): x is [C][rs] over the whole batch; utterance blockIdx.y owns columns [pre * mult, (pre + tb) * mult) of every row
static __global__ __launch_bounds__(256) void amax_rag_kernel(const float* __restrict__ x, int C, int rs, RagDev rg, float* __restrict__ slot) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const int n = rg.tb[b] * rg.mult;
    const float* p = x + (long)rg.pre[b] * rg.mult;
    float mx = 0.f;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        const float* r = p + (long)c * rs;
        for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, fabsf(r[i]));
    }
    amax_flush_wg(slot + b, mx, red);
}
// slot must have been zeroed (one memset per stage covers all of a stage's slots); rows of C * len floats must be 16-byte aligned
inline int run_amax_rows(tvc_ctx* ctx, hipStream_t s, const float* x, int B, int C, long len, float* slot) {
    if (ctx->rag) {     // (the driver passed B = 1 and len = the batch's columns at this tensor's rate)
        RagDev rg;
        TVC_CHECK(rag_tiles(ctx, s, B, len, 0, &rg, nullptr, "amax_rows"));
        const int gx = C < 8 ? C : (ctx->rag->B >= 64 ? 8 : 16);
        hipLaunchKernelGGL(amax_rag_kernel, dim3((unsigned)gx, (unsigned)ctx->rag->B), dim3(256), 0, s, x, C, (int)len, rg, slot);
        return launch_check(ctx, "amax_rows (ragged)");
    }
    const long n = (long)C * len;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return fail(ctx, TVC_ERR_ARG, "amax_rows: the tensor must be 16-byte aligned");
    // one atomic per workgroup: a few per utterance while the launch still fills the chip
    long gx = (n / 4 + 255) / 256 / 8;                     // >= 8 float4 per thread
    const long cap = B >= 64 ? 8 : 512 / (B > 0 ? B : 1);
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(amax_rows_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, s, x, n, slot);
    return launch_check(ctx, "amax_rows");
}

}  // namespace tvc
