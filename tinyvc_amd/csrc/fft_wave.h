// The wave-level FFT building blocks shared by fft.hip (the 1920-point transforms of the path) and denoise.hip (the 640-point frames of
// the streams' suppressor): complex helpers, the 3- and 5-point DFTs in registers, and the complex FFTs of 960 = 64 x 15 and 320 = 64 x 5
// points held by one wavefront - a small DFT over the registers of a lane, a twiddle, and a 64-point radix-2 DIF across the lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace tvc {

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * (c + i SIGN s)
template <int SIGN>
__device__ __forceinline__ float2 cmul_tw(float2 a, float2 w) {
    const float s = SIGN < 0 ? -w.y : w.y;
    return make_float2(fmaf(a.x, w.x, -a.y * s), fmaf(a.x, s, a.y * w.x));
}
// multiply by SIGN * i
template <int SIGN>
__device__ __forceinline__ float2 mul_i(float2 a) { return SIGN < 0 ? make_float2(a.y, -a.x) : make_float2(-a.y, a.x); }

// 3-point DFT in place: y[k] = sum_n x[n] e^(SIGN 2 pi i n k / 3)
template <int SIGN>
__device__ __forceinline__ void dft3(float2& a, float2& b, float2& c) {
    const float s = 0.86602540378443864676f;
    const float2 t = cadd(b, c), d = csub(b, c);
    const float2 m = make_float2(fmaf(-0.5f, t.x, a.x), fmaf(-0.5f, t.y, a.y));
    const float2 js = mul_i<SIGN>(make_float2(s * d.x, s * d.y));     // SIGN i s (b - c)
    a = cadd(a, t);
    b = cadd(m, js);
    c = csub(m, js);
}
// 5-point DFT in place
template <int SIGN>
__device__ __forceinline__ void dft5(float2& x0, float2& x1, float2& x2, float2& x3, float2& x4) {
    const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;    // cos(2 pi / 5), cos(4 pi / 5)
    const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;     // sin(2 pi / 5), sin(4 pi / 5)
    const float2 t1 = cadd(x1, x4), t2 = cadd(x2, x3), t3 = csub(x1, x4), t4 = csub(x2, x3);
    const float2 m1 = make_float2(fmaf(c1, t1.x, fmaf(c2, t2.x, x0.x)), fmaf(c1, t1.y, fmaf(c2, t2.y, x0.y)));
    const float2 m2 = make_float2(fmaf(c2, t1.x, fmaf(c1, t2.x, x0.x)), fmaf(c2, t1.y, fmaf(c1, t2.y, x0.y)));
    const float2 u1 = mul_i<SIGN>(make_float2(fmaf(s1, t3.x, s2 * t4.x), fmaf(s1, t3.y, s2 * t4.y)));   // SIGN i (s1 t3 + s2 t4)
    const float2 u2 = mul_i<SIGN>(make_float2(fmaf(s2, t3.x, -s1 * t4.x), fmaf(s2, t3.y, -s1 * t4.y)));  // SIGN i (s2 t3 - s1 t4)
    x0 = cadd(x0, cadd(t1, t2));
    x1 = cadd(m1, u1);
    x4 = csub(m1, u1);
    x2 = cadd(m2, u2);
    x3 = csub(m2, u2);
}

// register slot of output index k2 of the 15-point DFT below
__device__ __forceinline__ constexpr int slot15(int k2) { return 5 * (k2 % 3) + k2 / 3; }

// Complex FFT of 960 points held by one wavefront.  In: v[n2] = z[64 n2 + lane].  Out: v[slot15(k2)] = Z[15 bitrev6(lane) + k2]
// with Z[k] = sum_m z[m] e^(SIGN 2 pi i m k / 960) (unnormalised).
template <int SIGN>
__device__ __forceinline__ void fft960_wave(float2 (&v)[15], int lane, const float2* __restrict__ tw960) {
    // 15-point DFT over n2 = 5 na + nb -> k2 = ka + 3 kb
#pragma unroll
    for (int nb = 0; nb < 5; ++nb) dft3<SIGN>(v[nb], v[5 + nb], v[10 + nb]);          // v[5 ka + nb]
#pragma unroll
    for (int ka = 1; ka < 3; ++ka)
#pragma unroll
        for (int nb = 1; nb < 5; ++nb) v[5 * ka + nb] = cmul_tw<SIGN>(v[5 * ka + nb], tw960[64 * nb * ka]);   // W_15^(nb ka)
#pragma unroll
    for (int ka = 0; ka < 3; ++ka) dft5<SIGN>(v[5 * ka], v[5 * ka + 1], v[5 * ka + 2], v[5 * ka + 3], v[5 * ka + 4]);   // v[5 ka + kb]
    // twiddle W_960^(n1 k2), n1 = lane
#pragma unroll
    for (int k2 = 1; k2 < 15; ++k2) v[slot15(k2)] = cmul_tw<SIGN>(v[slot15(k2)], tw960[lane * k2]);
    // 64-point DIF FFT across the lanes
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const bool lower = (lane & h) != 0;
        const float2 w = tw960[(480 / h) * (lane & (h - 1))];                          // W_(2h)^(lane mod h)
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            const float2 p = make_float2(__shfl_xor(v[i].x, h), __shfl_xor(v[i].y, h));
            const float2 sum = cadd(v[i], p), dif = csub(p, v[i]);                      // lower lanes: partner is the upper element
            v[i] = lower ? (h > 1 ? cmul_tw<SIGN>(dif, w) : dif) : sum;
        }
    }
}

__device__ __forceinline__ int bitrev6(int l) { return (int)(__brev((unsigned)l) >> 26); }

// Complex FFT of 320 points held by one wavefront: fft960_wave's plan with the 5-point DFT in place of the 15-point stage.
// In: v[n2] = z[64 n2 + lane].  Out: v[k2] = Z[5 bitrev6(lane) + k2], Z[k] = sum_m z[m] e^(SIGN 2 pi i m k / 320) (unnormalised).
// tw320[j] = (cos, sin)(2 pi j / 320).
template <int SIGN>
__device__ __forceinline__ void fft320_wave(float2 (&v)[5], int lane, const float2* __restrict__ tw320) {
    dft5<SIGN>(v[0], v[1], v[2], v[3], v[4]);
    // twiddle W_320^(n1 k2), n1 = lane
#pragma unroll
    for (int k2 = 1; k2 < 5; ++k2) v[k2] = cmul_tw<SIGN>(v[k2], tw320[lane * k2]);
    // 64-point DIF FFT across the lanes
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const bool lower = (lane & h) != 0;
        const float2 w = tw320[(160 / h) * (lane & (h - 1))];                          // W_(2h)^(lane mod h)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float2 p = make_float2(__shfl_xor(v[i].x, h), __shfl_xor(v[i].y, h));
            const float2 sum = cadd(v[i], p), dif = csub(p, v[i]);                      // lower lanes: partner is the upper element
            v[i] = lower ? (h > 1 ? cmul_tw<SIGN>(dif, w) : dif) : sum;
        }
    }
}

}  // namespace tvc
