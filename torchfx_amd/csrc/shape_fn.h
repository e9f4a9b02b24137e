// shape_fn.h -- the transfer functions of the waveshaper (waveshaper.hip), host and device from one text: only + - * /,
// comparisons and explicit fma, no fast-math flag and no approximate intrinsic, every product-sum spelled out (the library is
// built with -ffp-contract=on).  A host program that includes this header (tools/shape_sweep.cpp) therefore runs the arithmetic
// the device runs; the float64 tanh alone calls the math library's.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SF_HD __host__ __device__ inline
#else
#define SF_HD inline
#endif

namespace shape_fn {

enum { HARD = 0, CUBIC = 1, TANH = 2, CURVE = 3 };          // tfx_shape

// one rounding each, never contracted
#if defined(__HIP_DEVICE_COMPILE__)
SF_HD float mul(float a, float b) { return __fmul_rn(a, b); }
SF_HD float add(float a, float b) { return __fadd_rn(a, b); }
SF_HD double mul(double a, double b) { return __dmul_rn(a, b); }
SF_HD double add(double a, double b) { return __dadd_rn(a, b); }
#else
SF_HD float mul(float a, float b) { volatile float p = a * b; return p; }
SF_HD float add(float a, float b) { volatile float s = a + b; return s; }
SF_HD double mul(double a, double b) { volatile double p = a * b; return p; }
SF_HD double add(double a, double b) { volatile double s = a + b; return s; }
#endif
SF_HD float fmad(float a, float b, float c) { return fmaf(a, b, c); }
SF_HD double fmad(double a, double b, double c) { return fma(a, b, c); }

template <typename T> SF_HD T clamp1(T v) { return v < (T)-1 ? (T)-1 : (v > (T)1 ? (T)1 : v); }

// min(max(v, -1), 1)
template <typename T> SF_HD T hard(T v) { return clamp1(v); }

// 1.5 v - 0.5 v^3 inside [-1, 1], sign(v) outside: v * (1.5 - 0.5 v^2), three roundings
template <typename T> SF_HD T cubic(T v)
{
    if (v >= (T)1) return (T)1;
    if (v <= (T)-1) return (T)-1;
    return mul(v, fmad((T)-0.5, mul(v, v), (T)1.5));
}

// float32 tanh: the odd 13th-degree over even 6th-degree rational minimax form used by Eigen and XLA, on the argument clamped
// to [-9, 9] (tanh(9) rounds to 1), Horner chains of explicit fmas, one division, the quotient clamped to [-1, 1]
SF_HD float tanh_f32(float v)
{
    const float x = v < -9.0f ? -9.0f : (v > 9.0f ? 9.0f : v);
    if (x > -0x1p-13f && x < 0x1p-13f) return x;                // tanh x = x (1 - x^2 / 3 + ...): within 2^-28 of x, relatively
    const float x2 = mul(x, x);
    float p = -2.76076847742355e-16f;
    p = fmad(x2, p, 2.00018790482477e-13f);
    p = fmad(x2, p, -8.60467152213735e-11f);
    p = fmad(x2, p, 5.12229709037114e-08f);
    p = fmad(x2, p, 1.48572235717979e-05f);
    p = fmad(x2, p, 6.37261928875436e-04f);
    p = fmad(x2, p, 4.89352455891786e-03f);
    p = mul(x, p);
    float q = 1.19825839466702e-06f;
    q = fmad(x2, q, 1.18534705686654e-04f);
    q = fmad(x2, q, 2.26843463243900e-03f);
    q = fmad(x2, q, 4.89352518554385e-03f);
    return clamp1(p / q);
}

SF_HD float tanh_of(float v) { return tanh_f32(v); }
SF_HD double tanh_of(double v) { return tanh(v); }

// WebAudio's WaveShaperNode rule for a table c of n >= 2 points over [-1, 1]
template <typename T, typename C> SF_HD T curve(T v, const C *c, int n)
{
    const T top = (T)(n - 1);
    T pos = mul(add(v, (T)1), mul(top, (T)0.5));
    pos = !(pos > (T)0) ? (T)0 : (pos > top ? top : pos);       // a NaN reads c[0]; the caller poisons non-finite values
    int i = (int)pos;
    i = i > n - 2 ? n - 2 : i;
    const T c0 = c[i], c1 = c[i + 1];
    return add(c0, mul(add(pos, -(T)i), add(c1, -c0)));
}

template <typename T, typename C> SF_HD T apply(int shape, T v, const C *c, int n)
{
    switch (shape) {
    case HARD: return hard(v);
    case CUBIC: return cubic(v);
    case TANH: return tanh_of(v);
    default: return curve(v, c, n);
    }
}

}  // namespace shape_fn
