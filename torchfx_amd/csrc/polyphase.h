// polyphase.h -- what resample.hip and limiter.hip share: scipy.signal.resample_poly's geometry, the cached polyphase tap
// table and the device helpers of the `up`x interpolator chain (true_peak_kernel, limiter_kernel).
#pragma once
#include "common.h"
#include "plan_cache.h"

#include <memory>

namespace tfx {

// scipy.signal.resample_poly's arithmetic for a filter of nh taps (up, down already reduced)
struct ResampleGeom {
    int64_t n_out, pre_pad, post_pad, pre_remove, padded, Lp;
};

inline int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

inline ResampleGeom resample_geometry(int64_t T, int64_t up, int64_t down, int64_t nh)
{
    ResampleGeom g{};
    g.n_out = ceil_div(T * up, down);
    const int64_t half_len = (nh - 1) / 2;
    g.pre_pad = down - half_len % down;
    g.pre_remove = (half_len + g.pre_pad) / down;
    // SciPy increments n_post_pad while _output_len(len, T, up, down) = ((T-1)*up + len - 1) // down + 1 < n_out + pre_remove;
    // the least such pad in closed form (floor division: T = 0 gives a negative numerator)
    const int64_t len0 = nh + g.pre_pad, need = g.n_out + g.pre_remove;
    const int64_t have = floor_div((T - 1) * up + len0 - 1, down) + 1;
    g.post_pad = have >= need ? 0 : down * (need - 1) - (T - 1) * up - len0 + 1;
    g.padded = len0 + g.post_pad;
    g.Lp = ceil_div(g.padded, up);
    return g;
}

// register-tap buckets: each is one instantiation of a kernel
inline int64_t reg_bucket(int64_t Lp)
{
    for (int64_t b : {8, 16, 24, 32, 48, 64})
        if (Lp <= b) return b;
    return 0;
}

// The polyphase table hp[p][j] = h_padded[p + j*up] (Lp taps per phase, zeros past the filter) on the device, cached by the
// taps' bytes plus (up, down, dtype, n_pre_pad, Lp); `keep` holds it until the caller's launches are enqueued (resample.hip).
template <typename T>
const T *resample_table(const void *taps_host, int64_t nh, int64_t up, int64_t down, int64_t pre_pad, int64_t Lp,
                        hipStream_t stream, std::shared_ptr<DeviceBuffer> *keep);

constexpr int RS_STAGE_BATCH = 8;                         // staging loads in flight per thread

// ---- the interpolator chain: TP_R consecutive input positions per thread, a phase's taps the same for every lane -------------
constexpr int TP_THREADS = 256;
constexpr int TP_R = 16;                                  // consecutive input positions per thread
constexpr int64_t TP_TILE = (int64_t)TP_THREADS * TP_R;   // positions per workgroup (limiter_kernel: per detector pass)
constexpr int64_t TP_LP_MAX = 72;                         // nh <= 64 * up gives Lp <= 65

template <typename T> using tp_const_ptr = const T __attribute__((address_space(4))) *;

// acc = fma(tap, x, acc); tp_fma0 starts a chain from +0.  The f32 forms are single instructions by hand: left to itself the
// compiler packs neighbouring chains into v_pk_fma_f32 and pays a register copy for every odd-aligned pair of inputs (238
// v_mov per 384 fma and 234 VGPRs).  The tap is asked for in a vector register: one v_mov per tap and phase, and the fma
// measured 18 % faster than with the tap as its scalar operand.
__device__ __forceinline__ float tp_fma(float tap, float x, float acc)
{
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(tap), "v"(x));
    return acc;
}
__device__ __forceinline__ float tp_fma0(float tap, float x)
{
    float acc;
    asm("v_fma_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(tap), "v"(x));
    return acc;
}
__device__ __forceinline__ double tp_fma(double tap, double x, double acc) { return fma(tap, x, acc); }
__device__ __forceinline__ double tp_fma0(double tap, double x) { return fma(tap, x, 0.0); }

template <typename T> __device__ __forceinline__ T tp_max(T m, T a) { return (a > m || a != a) ? a : m; }

// window line stride: 256 columns + up to ceil(71 / 16) = 5 of halo; f32 S = 2 (mod 32), f64 S = 1 (mod 16)
template <typename T> constexpr int tp_stride() { return sizeof(T) == 4 ? 290 : 273; }

inline int64_t tp_bucket(int64_t Lp) { return reg_bucket(Lp) ? reg_bucket(Lp) : TP_LP_MAX; }

}  // namespace tfx
