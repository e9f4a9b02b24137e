// lfo.h -- the low-frequency oscillator the modulation effects share (modulation.hip: the delay of Chorus, Flanger and Vibrato;
// phaser.hip: the all-pass coefficient).  One definition, so a sweep means the same thing in every effect:
//   t = double(n) * inc   -- one IEEE multiplication, never contracted into an FMA (a fused n * inc - floor(t) moves the phase at
//                            n = 2^40 by far more than the last bit)
//   a = (t - floor(t)) + off                                  in [0, 2) for off in [0, 1)
//   l = sinpi(2 a)  (sine)   or   1 - 4 |frac(a + 0.25) - 0.5|  (triangle)
// Contraction is off inside, so every expression rounds exactly as written, on the device and in the host paths.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tfx {

template <bool TRI> __device__ __forceinline__ double lfo_at(int64_t n, double inc, double off)
{
#pragma clang fp contract(off)
    const double t = __dmul_rn((double)n, inc);
    const double a = (t - floor(t)) + off;
    if (TRI) {
        const double z = a + 0.25;
        return 1.0 - 4.0 * fabs((z - floor(z)) - 0.5);
    }
    return sinpi(2.0 * a);
}

}  // namespace tfx
