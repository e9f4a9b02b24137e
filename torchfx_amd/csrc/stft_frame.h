// stft_frame.h -- what stft.hip (forward) and istft.hip (inverse) share: the M-point complex transform of one frame in LDS by
// M / 16 threads, and the twiddle tables [W_M^j | W_n^k] of the plan cache.  One text: a frame's bits are the same in both files.
//
// Stage (radix r, stride s; s is the product of the earlier radices, m = M / (r s)): butterfly b = q + s p (q < s, p < m) takes
// a_j = x[b + (M / r) j], forms the r-point DFT A_k and stores y[q + s (r p + k)] = A_k W_M^(s p k).  A thread holds the sixteen
// values t + TPF e (e < 16) of its frame: those are the inputs of its 16 / r butterflies in EVERY stage, and the outputs of the
// last one, so each exchange is "store scattered, barrier, load own".
#pragma once
#include "ldsfft.h"
#include "plan_cache.h"

#include <cmath>
#include <memory>
#include <vector>

namespace tfx {

// [W_M^j | W_n^k] in double, rounded once; keyed by n_fft and the element size (no coefficient bytes).  Defined in stft.hip.
extern PlanCache<DeviceBuffer, 2> g_stft_tables;

namespace {

using ldsfft::cadd;
using ldsfft::cmul;
using ldsfft::csub;
using ldsfft::cx;
using ldsfft::mk;

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }

// r-point DFT, inputs and outputs in natural order
template <typename R, int RADIX> __device__ __forceinline__ void dft_natural(cx<R> (&a)[RADIX])
{
    if constexpr (RADIX == 16) {
        ldsfft::dft16<R, false>(a);
        cx<R> o[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = a[LDS_DFT16_AT(k)];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = o[k];
    } else if constexpr (RADIX == 8) {
        constexpr R R2 = (R)0.70710678118654752440L;
        ldsfft::dft4<R, false>(a[0], a[2], a[4], a[6]);
        ldsfft::dft4<R, false>(a[1], a[3], a[5], a[7]);
        const cx<R> e[4] = {a[0], a[2], a[4], a[6]};
        const cx<R> o[4] = {a[1], mk<R>((a[3].x + a[3].y) * R2, (a[3].y - a[3].x) * R2), mk<R>(a[5].y, -a[5].x),
                            mk<R>((a[7].y - a[7].x) * R2, -(a[7].x + a[7].y) * R2)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[k] = cadd(e[k], o[k]);
            a[k + 4] = csub(e[k], o[k]);
        }
    } else if constexpr (RADIX == 4) {
        ldsfft::dft4<R, false>(a[0], a[1], a[2], a[3]);
    } else {
        static_assert(RADIX == 2, "radix");
        const cx<R> s = cadd(a[0], a[1]);
        a[1] = csub(a[0], a[1]);
        a[0] = s;
    }
}

__device__ __forceinline__ int stft_at(int p) { return p + (p >> 4); }      // position of element p in a frame's exchange buffer

template <typename R, int M, int RADIX, int S, bool LAST>
__device__ __forceinline__ void stft_stage(cx<R> (&v)[16], cx<R> *wk, const cx<R> *tw, int t)
{
    constexpr int TPF = M / 16, NB = 16 / RADIX;
    static_assert(!LAST || S * RADIX == M, "the last stage ends the transform");
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        cx<R> a[RADIX];
#pragma unroll
        for (int j = 0; j < RADIX; ++j) a[j] = v[i + NB * j];
        dft_natural<R, RADIX>(a);
        const int b = t + TPF * i, q = b & (S - 1), ps = b - q;         // ps = s p
        const int o0 = q + RADIX * ps;
#pragma unroll
        for (int k = 0; k < RADIX; ++k) {
            cx<R> y = a[k];
            if (!LAST && k > 0) y = cmul(y, tw[ps * k]);                // s p k <= s (m - 1) (r - 1) < M
            wk[stft_at(o0 + S * k)] = y;
        }
    }
}

template <typename R, int M> __device__ __forceinline__ void stft_reload(cx<R> (&v)[16], const cx<R> *wk, int t)
{
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = wk[stft_at(t + (M / 16) * e)];
    __syncthreads();
}

// the M-point complex transform of one frame: v in, Z in wk (natural order, at stft_at).  The last stage multiplies by no
// twiddle, so W_M is dead once the exchange in front of it is through: `before_last` runs there (the forward kernel puts W_n in
// its place)
template <typename R, int M, typename F>
__device__ __forceinline__ void stft_transform(cx<R> (&v)[16], cx<R> *wk, const cx<R> *tw, int t, F &&before_last)
{
    if constexpr (M == 128) {
        stft_stage<R, M, 8, 1, false>(v, wk, tw, t);
        stft_reload<R, M>(v, wk, t);
        before_last();
        stft_stage<R, M, 16, 8, true>(v, wk, tw, t);
    } else if constexpr (M == 256) {
        stft_stage<R, M, 16, 1, false>(v, wk, tw, t);
        stft_reload<R, M>(v, wk, t);
        before_last();
        stft_stage<R, M, 16, 16, true>(v, wk, tw, t);
    } else {
        constexpr int R0 = M / 256;                                     // 2, 4 or 8
        stft_stage<R, M, R0, 1, false>(v, wk, tw, t);
        stft_reload<R, M>(v, wk, t);
        stft_stage<R, M, 16, R0, false>(v, wk, tw, t);
        stft_reload<R, M>(v, wk, t);
        before_last();
        stft_stage<R, M, 16, 16 * R0, true>(v, wk, tw, t);
    }
}

template <typename R> std::shared_ptr<DeviceBuffer> stft_tables(int64_t n_fft, hipStream_t stream)
{
    static const char none = 0;
    const int64_t tail[2] = {n_fft, (int64_t)sizeof(R)};
    return g_stft_tables.get(&none, 0, tail, stream, [&] {
        const int64_t M = n_fft / 2;
        const double tau = 6.283185307179586476925286766559;
        std::vector<cx<R>> h((size_t)(2 * M));
        for (int64_t j = 0; j < M; ++j) {
            // the exact octants: W^0 = 1, W^(M/4) = -i, W^(M/2) = -1 and W_n^(M/2) = -i carry no rounding of pi
            const double a = tau * (double)j / (double)M, b = tau * (double)j / (double)n_fft;
            h[(size_t)j].x = (R)(4 * j == M || 4 * j == 3 * M ? 0.0 : std::cos(a));
            h[(size_t)j].y = (R)(2 * j == M || j == 0 ? 0.0 : -std::sin(a));
            h[(size_t)(M + j)].x = (R)(2 * j == M ? 0.0 : std::cos(b));
            h[(size_t)(M + j)].y = (R)(j == 0 ? 0.0 : -std::sin(b));
        }
        return std::make_shared<DeviceBuffer>(h);
    });
}

}  // namespace
}  // namespace tfx
