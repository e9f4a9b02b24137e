// polyphase.h -- what resample.hip, limiter.hip and waveshaper.hip share: scipy.signal.resample_poly's geometry, the cached
// polyphase tap table, and the `up`x interpolator chain of true_peak_kernel and waveshaper_kernel, written once:
//   device   tp_stage (window into LDS, transposed), tp_window / tp_win_at (a thread's inputs), tp_phase (one phase's R sums
//            from registers), tp_phase_at (one sum from LDS), StreamRow and stream_hist_copy (a row as [hist | x])
//   host     interp_plan (the taps' refusals, bucket and first position), tp_dispatch (bucket -> instantiation),
//            launch_dynamic_lds, StreamArgs / stream_enter (what the entries that hold outputs back do before they launch)
// limiter_kernel takes everything but tp_stage, tp_window, tp_phase and tp_phase_at: its detector keeps those four loops
// written out over tp_win_at and tp_fma (limiter.hip says why).  DESIGN.md 4.11d says what a kernel that uses the chain
// supplies itself.
#pragma once
#include "common.h"
#include "plan_cache.h"

#include <algorithm>
#include <memory>
#include <type_traits>

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

// The polyphase table hp[p][j] = h_padded[p + j*up] (Lp taps per phase, zeros past the filter) on the device, cached by the
// taps' bytes plus (up, down, dtype, n_pre_pad, Lp); `keep` holds it until the caller's launches are enqueued (resample.hip).
template <typename T>
const T *resample_table(const void *taps_host, int64_t nh, int64_t up, int64_t down, int64_t pre_pad, int64_t Lp,
                        hipStream_t stream, std::shared_ptr<DeviceBuffer> *keep);

constexpr int RS_STAGE_BATCH = 8;                         // staging loads in flight per thread

// ---- the interpolator chain: R consecutive input positions per thread, a phase's taps the same for every lane ----------------
constexpr int TP_THREADS = 256;
constexpr int TP_R = 16;                                  // consecutive input positions per thread
constexpr int64_t TP_TILE = (int64_t)TP_THREADS * TP_R;   // positions per workgroup (limiter_kernel: per detector pass)
constexpr int64_t TP_LP_MAX = 72;                         // nh <= 64 * up gives Lp <= 65

// register-tap buckets: each is one instantiation of a kernel
inline int64_t reg_bucket(int64_t Lp)
{
    for (int64_t b : {8, 16, 24, 32, 48, 64})
        if (Lp <= b) return b;
    return 0;
}
inline int64_t tp_bucket(int64_t Lp) { return reg_bucket(Lp) ? reg_bucket(Lp) : TP_LP_MAX; }

// f(std::integral_constant<int, LP>) for the chain's bucket LP = tp_bucket(Lp)
template <typename F> void tp_dispatch(int64_t LP, F &&f)
{
    switch (LP) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 24: return f(std::integral_constant<int, 24>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 48: return f(std::integral_constant<int, 48>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return f(std::integral_constant<int, (int)TP_LP_MAX>{});
    }
}

// What an `up`x interpolator of nh taps is to the chain: resample_forward(x, up, 1)'s geometry, the bucket LP that holds its
// Lp taps per phase and i_lo, the input position of the row's first output.  Refuses what the chain cannot hold, in this order.
struct InterpPlan {
    ResampleGeom g;
    int64_t LP, i_lo;
};

inline InterpPlan interp_plan(const char *who, int64_t up, int64_t nh, int64_t T)
{
    TFX_CHECK(nh >= 1, "%s: no taps", who);
    TFX_CHECK(nh <= 64 * up, "%s: %lld taps, at most 64 * up = %lld are held in registers", who, (long long)nh, (long long)(64 * up));
    TFX_CHECK(T <= (INT64_MAX / 64) / up, "%s: T * up overflows", who);
    InterpPlan ip{};
    ip.g = resample_geometry(T, up, 1, nh);
    TFX_CHECK(ip.g.Lp <= TP_LP_MAX, "%s: %lld taps per phase", who, (long long)ip.g.Lp);
    ip.LP = tp_bucket(ip.g.Lp);
    ip.i_lo = ip.g.pre_remove / up;
    TFX_CHECK(ip.i_lo <= ip.LP - 1, "%s: the filter's delay exceeds its taps per phase", who);
    return ip;
}

template <typename T> using tp_const_ptr = const T __attribute__((address_space(4))) *;

// acc = fma(tap, x, acc); tp_fma0 starts a chain from +0.  The f32 forms are single instructions by hand: left to itself the
// compiler packs neighbouring chains into v_pk_fma_f32 and pays a register copy for every odd-aligned pair of inputs (238
// v_mov per 384 fma and 234 VGPRs).  The tap is asked for in a vector register: one v_mov per tap and phase, and the fma
// measured 18 % faster than with the tap as its scalar operand.  tp_fma<true> asks for the scalar operand all the same:
// limiter_kernel's written-out chain takes it for its long filters (LP >= 64), which have no vector registers left for taps.
template <bool SCALAR = false> __device__ __forceinline__ float tp_fma(float tap, float x, float acc)
{
    if constexpr (SCALAR) asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "s"(tap), "v"(x));
    else asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(tap), "v"(x));
    return acc;
}
__device__ __forceinline__ float tp_fma0(float tap, float x)
{
    float acc;
    asm("v_fma_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(tap), "v"(x));
    return acc;
}
template <bool SCALAR = false> __device__ __forceinline__ double tp_fma(double tap, double x, double acc) { return fma(tap, x, acc); }
__device__ __forceinline__ double tp_fma0(double tap, double x) { return fma(tap, x, 0.0); }

template <typename T> __device__ __forceinline__ T tp_max(T m, T a) { return (a > m || a != a) ? a : m; }

// window line stride: 256 columns + up to ceil(71 / 16) = 5 of halo; f32 S = 2 (mod 32), f64 S = 1 (mod 16)
template <typename T> constexpr int tp_stride() { return sizeof(T) == 4 ? 290 : 273; }

// The window of a tile in LDS, transposed: index w lies at column w / R of line w % R (S words per line).  Thread t owns the
// positions t*R .. t*R + R - 1 and reads its k-th input at column t + k / R of line k % R: the lanes of one read are
// consecutive words, and S is chosen so that the consecutive w of a staging store fall into distinct banks too.
template <int R, int S, typename T> __device__ __forceinline__ T &tp_win_at(T *win, int t, int k) { return win[(k % R) * S + t + k / R]; }

// the R + LP - 1 inputs of thread t's positions into registers
template <int R, int S, typename T, int NW> __device__ __forceinline__ void tp_window(T (&xw)[NW], T *win, int t)
{
#pragma unroll
    for (int k = 0; k < NW; ++k) xw[k] = tp_win_at<R, S>(win, t, k);
}

// Stages row.at(s0 + j), j < span, as window index j, RS_STAGE_BATCH loads in flight per thread; true when this thread met a
// NaN or an Inf.  The caller's barrier follows.  R = 1 is a plain window (resample_kernel).
template <int R, int S, int THREADS, typename T, typename Row>
__device__ __forceinline__ bool tp_stage(T *win, const Row &row, int64_t s0, int span, int t)
{
    bool bad = false;
    for (int j0 = 0; j0 < span; j0 += THREADS * RS_STAGE_BATCH) {
        T v[RS_STAGE_BATCH];
#pragma unroll
        for (int u = 0; u < RS_STAGE_BATCH; ++u) {
            const int j = j0 + u * THREADS + t;
            v[u] = j < span ? row.at(s0 + j) : (T)0;
        }
#pragma unroll
        for (int u = 0; u < RS_STAGE_BATCH; ++u) {
            const int j = j0 + u * THREADS + t;
            if (j < span) tp_win_at<R, S>(win, 0, j) = v[u];
            bad |= !isfinite(v[u]);
        }
    }
    return bad;
}

// One phase for a thread's R positions: acc[r] = the descending-j fma chain from +0 over taps[j] * xw[r + LP - 1 - j], which
// is resample_forward's sum.  The table is read-only for the whole launch: through the constant address space its taps, the
// same for every lane, are scalar loads (a global load per lane and tap otherwise).
template <int LP, typename T, int R>
__device__ __forceinline__ void tp_phase(T (&acc)[R], const T *taps, const T (&xw)[R + LP - 1])
{
    const tp_const_ptr<T> h = (tp_const_ptr<T>)taps;
    T tap[LP];
#pragma unroll
    for (int j = 0; j < LP; ++j) tap[j] = h[j];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = tp_fma0(tap[LP - 1], xw[r]);
#pragma unroll
    for (int j = LP - 2; j >= 0; --j)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = tp_fma(tap[j], xw[r + LP - 1 - j], acc[r]);
}

// The same sum for position r of thread t alone, from LDS, over the first n_taps taps of a phase (LP: the window's halo + 1).
// Edge threads, whose phases are not all outputs, and tiles with a non-finite window take this one.
template <int R, int S, typename T> __device__ __forceinline__ T tp_phase_at(const T *h, int n_taps, int LP, T *win, int t, int r)
{
    T acc = (T)0;
    for (int j = n_taps - 1; j >= 0; --j) acc = fma(h[j], tp_win_at<R, S>(win, t, r + LP - 1 - j), acc);
    return acc;
}

// A row by sample position.  One-shot: x[row] over [0, end).  Stream: positions [N - Hs, N) come from hist (zeros when null),
// [N, end) from x; nothing exists before 0 or from `end` on.
template <typename T, bool STREAM> struct StreamRow {
    const T *xr, *hr;
    int64_t N, h0, end;
    __device__ __forceinline__ StreamRow(const T *x, int64_t pitch, const T *hist, int64_t Hs, int64_t N_, int64_t end_, int64_t row)
        : xr(x + row * pitch), hr(nullptr), N(0), h0(0), end(end_)
    {
        if constexpr (STREAM) {
            hr = hist ? hist + row * Hs : nullptr;
            N = N_;
            h0 = N_ - Hs;
        }
    }
    __device__ __forceinline__ T at(int64_t i) const
    {
        if constexpr (STREAM) {
            if (i < 0 || i >= end) return (T)0;
            if (i >= N) return xr[i - N];
            return (hr && i >= h0) ? hr[i - h0] : (T)0;
        } else {
            return (i >= 0 && i < end) ? xr[i] : (T)0;
        }
    }
};

// the next chunk's history of one row, the newest Hs samples of [hist | x[:n_in]]: entries first, first + step, ...
template <typename T>
__device__ __forceinline__ void stream_hist_copy(T *hist_out, const T *x, int64_t pitch, const T *hist, int64_t n_in, int64_t Hs,
                                                 int64_t row, int64_t first, int64_t step)
{
    const T *hr = hist ? hist + row * Hs : nullptr;
    for (int64_t j = first; j < Hs; j += step) hist_out[row * Hs + j] = stream_hist_at(x + row * pitch, hr, n_in, Hs, j);
}

// ---- host: launches and stream entries ---------------------------------------------------------------------------------------
// Launches Kernel with `lds` bytes of dynamic LDS, raising the kernel's limit first where this device has not seen as much.
template <auto Kernel, typename Args>
void launch_dynamic_lds(const char *name, int64_t grid, int threads, size_t lds, hipStream_t stream, const Args &p)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if (lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        have = lds;
    }
    ProfScope ps(name, stream);
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds, stream, p);
    TFX_HIP(hipGetLastError());
}

// what a stream entry that holds outputs back hands to its launch; N is `consumed` after the clamp
struct StreamArgs {
    const void *hist_in;
    void *hist_out;
    int64_t n_in, N, D, Hs;
};

// The chunk's refusals (x, y: [rows, T], of which n_in samples per row are real; the histories: [rows, Hs]) and the chunks
// that launch nothing: no rows, or T == 0, where the history moves on unchanged.  True when there is a launch to make.
inline bool stream_enter(StreamArgs *st, const char *who, size_t esz, const void *x, const void *y, int64_t rows, int64_t T,
                         int64_t n_in, int64_t consumed, int64_t D, int64_t Hs, const void *hist_in, void *hist_out,
                         hipStream_t stream)
{
    TFX_CHECK(n_in >= 0 && n_in <= T, "%s: n_in = %lld is not in [0, T = %lld]", who, (long long)n_in, (long long)T);
    TFX_CHECK(consumed >= 0, "%s: negative stream position %lld", who, (long long)consumed);
    TFX_CHECK(rows * T == 0 || y, "%s: null pointer", who);
    TFX_CHECK(rows * n_in == 0 || x, "%s: null pointer", who);
    check_stream_buffers(who, esz, x, rows * T, y, rows * T, hist_in, hist_out, rows * Hs);
    if (rows == 0) return false;
    if (T == 0) {
        const size_t bytes = (size_t)(rows * Hs) * esz;
        if (hist_out && bytes) {
            if (hist_in) TFX_HIP(hipMemcpyAsync(hist_out, hist_in, bytes, hipMemcpyDeviceToDevice, stream));
            else TFX_HIP(hipMemsetAsync(hist_out, 0, bytes, stream));
        }
        return false;
    }
    // positions before N - Hs are never read and position 0 matters only while it lies in [N - Hs, N + T): past Hs + D every N
    // gives the same chunk
    *st = StreamArgs{hist_in, hist_out, n_in, std::min(consumed, Hs + D), D, Hs};
    return true;
}

}  // namespace tfx
