// stft_frame.h -- what stft.hip (forward), istft.hip (inverse) and mel.hip (mel spectrogram) share: the M-point complex transform
// of one frame in LDS by M / 16 threads, and the twiddle tables [W_M^j | W_n^k] of the plan cache.  One text: a frame's bits are
// the same in all files.  The two forward kernels share their whole front, bin and power expressions and plan as well (below).
//
// Stage (radix r, stride s; s is the product of the earlier radices, m = M / (r s)): butterfly b = q + s p (q < s, p < m) takes
// a_j = x[b + (M / r) j], forms the r-point DFT A_k and stores y[q + s (r p + k)] = A_k W_M^(s p k).  A thread holds the sixteen
// values t + TPF e (e < 16) of its frame: those are the inputs of its 16 / r butterflies in EVERY stage, and the outputs of the
// last one, so each exchange is "store scattered, barrier, load own".
#pragma once
#include "ldsfft.h"
#include "plan_cache.h"
#include "../../include/torchfx_hip.h"

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

// ---- the forward kernels' front: stft.hip and mel.hip (the inverse has a front of its own) ----

constexpr int STFT_POWER_COMPLEX = 0, STFT_POWER_MAGNITUDE = 1, STFT_POWER_SQUARE = 2;

template <typename R> struct StftArgs {
    const R *x;             // [rows, T]
    const R *win;           // [win_len] or null (ones)
    const cx<R> *tab;       // [W_M^j, j < M | W_n^k, k < M]
    void *out;              // [rows, frames, M + 1] complex or real (mel.hip: [rows, frames, n_filters] real)
    int64_t T, frames, groups_per_row, hop, pad;
    int hop_lds;            // min(hop, n_fft): distance of two frames in the staged image
    int win_len, win_left, reflect, power, normalized;
    R scale;                // n_fft^-1/2
};

template <int M> constexpr int stft_log2n() { return M == 128 ? 8 : M == 256 ? 9 : M == 512 ? 10 : M == 1024 ? 11 : 12; }

// What a workgroup of THREADS threads does before its output loop, for the G = THREADS / (M / 16) frames f0 ... of `row`: every
// global load up front, the staged span, the window product and the transform.  LDS at smem: [W_M: M complex | window: n_fft
// reals | staged samples, then -- behind a barrier -- the G frames' exchange buffers of M + M / 16 complex each].  On return
// (behind a barrier) frame g's Z is in its exchange buffer (natural order, at stft_at) and W_n^k has taken W_M's place.
// `more_loads` issues the caller's own global loads among the others, `more_stores` puts them into LDS with the tables.
template <typename R, int M, int THREADS, typename FL, typename FS_>
__device__ __forceinline__ void stft_frames(const StftArgs<R> &p, unsigned char *smem, int64_t row, int64_t f0, FL &&more_loads,
                                            FS_ &&more_stores)
{
    constexpr int N = 2 * M, TPF = M / 16, G = THREADS / TPF, FS = M + M / 16, LOGN = stft_log2n<M>(), BATCH = 8;
    constexpr int NP = (M + THREADS - 1) / THREADS, NW = (N + THREADS - 1) / THREADS;
    cx<R> *tw = (cx<R> *)smem;
    R *win = (R *)(tw + M);
    R *stage = win + N;
    cx<R> *work = (cx<R> *)stage;                                       // reuses the staged samples' bytes, behind a barrier
    const int tid = (int)threadIdx.x;

    // Every global load of the workgroup is issued here, before the first one is used: both tables, the window and the samples
    // (in batches).  A workgroup has two or three neighbours on its CU and a few microseconds to live; a load it waits for in the
    // middle -- one per loop iteration, or the post-twiddles in the output loop -- costs it a full memory latency each time.
    R tvx[NP], tvy[NP], pvx[NP], pvy[NP], wv[NW];                        // scalars: arrays of cx<double> end up in scratch
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int i = u * THREADS + tid;
        tvx[u] = tvy[u] = pvx[u] = pvy[u] = (R)0;
        if (M % THREADS == 0 || i < M) {
            const cx<R> a = p.tab[i], b = p.tab[M + i];
            tvx[u] = a.x; tvy[u] = a.y; pvx[u] = b.x; pvy[u] = b.y;
        }
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const int j = u * THREADS + tid - p.win_left;
        wv[u] = (R)0;
        if (j >= 0 && j < p.win_len) wv[u] = p.win ? p.win[j] : (R)1;
    }
    more_loads();
    {
        const R *xr = p.x + row * p.T;
        const int64_t base = f0 * p.hop - p.pad;
        const bool apart = p.hop > N;                                   // frames that do not touch are staged one by one
        const int span = (G - 1) * p.hop_lds + N;
        for (int e0 = tid; e0 < span; e0 += BATCH * THREADS) {
            R val[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = e0 + u * THREADS;
                int64_t i = apart ? base + (int64_t)(e >> LOGN) * p.hop + (e & (N - 1)) : base + e;
                if (p.reflect) i = i < 0 ? -i : (i >= p.T ? 2 * (p.T - 1) - i : i);
                val[u] = (e < span && i >= 0 && i < p.T) ? xr[i] : (R)0;     // beyond one reflection: frames past the last one only
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (e0 + u * THREADS < span) stage[e0 + u * THREADS] = val[u];
        }
    }
#pragma unroll
    for (int u = 0; u < NP; ++u)
        if (M % THREADS == 0 || u * THREADS + tid < M) tw[u * THREADS + tid] = mk<R>(tvx[u], tvy[u]);
#pragma unroll
    for (int u = 0; u < NW; ++u)
        if (N % THREADS == 0 || u * THREADS + tid < N) win[u * THREADS + tid] = wv[u];
    more_stores();
    __syncthreads();

    const int g = tid / TPF, t = tid - g * TPF;
    cx<R> v[16];
    {
        const R *s = stage + g * p.hop_lds;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = 2 * (t + TPF * e);
            v[e] = mk<R>(mul_rn(s[n], win[n]), mul_rn(s[n + 1], win[n + 1]));
        }
    }
    __syncthreads();
    stft_transform<R, M>(v, work + g * FS, tw, t, [&] {
#pragma unroll
        for (int u = 0; u < NP; ++u)
            if (M % THREADS == 0 || u * THREADS + tid < M) tw[u * THREADS + tid] = mk<R>(pvx[u], pvy[u]);
    });
    __syncthreads();
}

// bin k <= M of the real input's spectrum from a frame's Z (wk) and W_n^k (post), scaled when `normalized`
template <typename R, int M> __device__ __forceinline__ cx<R> stft_bin(const cx<R> *wk, const cx<R> *post, int k, const StftArgs<R> &p)
{
    cx<R> X;
    if (k == 0 || k == M) {
        const cx<R> z = wk[0];
        X = mk<R>(k == 0 ? z.x + z.y : z.x - z.y, (R)0);
    } else {
        const cx<R> a = wk[stft_at(k)], bz = wk[stft_at(M - k)];
        const cx<R> ev = mk<R>((a.x + bz.x) * (R)0.5, (a.y - bz.y) * (R)0.5);          // (A + conj B) / 2
        const cx<R> od = mk<R>((a.y + bz.y) * (R)0.5, (bz.x - a.x) * (R)0.5);          // -i (A - conj B) / 2
        X = cadd(ev, cmul(post[k], od));
    }
    if (p.normalized) X = mk<R>(X.x * p.scale, X.y * p.scale);
    return X;
}

// |X| (STFT_POWER_MAGNITUDE) or |X|^2
template <typename R> __device__ __forceinline__ R stft_power(const cx<R> X, int power)
{
    const R pw = X.x * X.x + X.y * X.y;
    return power == STFT_POWER_MAGNITUDE ? (R)sqrt(pw) : pw;
}

struct StftPlan {
    int route = 0;          // 1: the LDS kernels, 0: torch.stft (the caller's business)
    int threads = 0;
    int64_t frames = 0, G = 0, tpf = 0, lds = 0, groups_per_row = 0, workgroups = 0;
};

// every check on the sizes, and the geometry; pad is the samples added at each end (n_fft / 2 when centred)
inline StftPlan stft_plan(const char *what, int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int64_t pad,
                          int pad_mode, int onesided)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: dtype must be TFX_F32 or TFX_F64", what);
    TFX_CHECK(n_fft >= 1 && n_fft <= (int64_t)1 << 30, "%s: n_fft %lld out of range", what, (long long)n_fft);
    TFX_CHECK(hop >= 1, "%s: hop %lld must be at least 1", what, (long long)hop);
    TFX_CHECK(win_length >= 1 && win_length <= n_fft, "%s: win_length %lld must be in [1, n_fft]", what, (long long)win_length);
    TFX_CHECK(rows >= 0 && T >= 1 && T <= (int64_t)1 << 40, "%s: bad shape (rows %lld, T %lld)", what, (long long)rows, (long long)T);
    TFX_CHECK(pad >= 0 && pad <= n_fft, "%s: pad %lld must be in [0, n_fft]", what, (long long)pad);
    TFX_CHECK(pad_mode >= TFX_STFT_PAD_CONSTANT && pad_mode <= TFX_STFT_PAD_CIRCULAR, "%s: unknown pad_mode %d", what, pad_mode);
    TFX_CHECK(pad == 0 || pad_mode == TFX_STFT_PAD_CONSTANT || pad_mode == TFX_STFT_PAD_REPLICATE || pad < T || (pad_mode == TFX_STFT_PAD_CIRCULAR && pad <= T),
              "%s: padding %lld does not fit a row of %lld samples", what, (long long)pad, (long long)T);
    TFX_CHECK(T + 2 * pad >= n_fft, "%s: %lld samples (with padding) are fewer than n_fft %lld", what, (long long)(T + 2 * pad),
              (long long)n_fft);
    StftPlan pl;
    pl.frames = 1 + (T + 2 * pad - n_fft) / hop;
    const bool size_ok = n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096;
    if (!size_ok || !onesided || (pad > 0 && pad_mode != TFX_STFT_PAD_CONSTANT && pad_mode != TFX_STFT_PAD_REFLECT)) return pl;
    const int64_t esz = dtype == TFX_F32 ? 4 : 8;
    pl.route = 1;
    pl.threads = dtype == TFX_F32 ? 256 : 128;
    pl.tpf = n_fft / 32;
    pl.G = pl.threads / pl.tpf;
    pl.groups_per_row = ceil_div(pl.frames, pl.G);
    pl.workgroups = rows * pl.groups_per_row;
    TFX_CHECK(pl.workgroups <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid", what, (long long)pl.workgroups);
    const int64_t M = n_fft / 2, span = (pl.G - 1) * (hop < n_fft ? hop : n_fft) + n_fft, work = pl.G * (M + M / 16) * 2;
    pl.lds = esz * (2 * M + n_fft + (span > work ? span : work));
    return pl;
}

// the kernel arguments of one launch, from the plan and the geometry
template <typename R>
StftArgs<R> stft_args(const void *x, const void *window, const cx<R> *tab, void *out, int64_t T, int64_t n_fft, int64_t hop,
                      int64_t win_length, int64_t pad, int pad_mode, int power, int normalized, const StftPlan &pl)
{
    StftArgs<R> p{};
    p.x = (const R *)x; p.win = (const R *)window; p.tab = tab; p.out = out;
    p.T = T; p.frames = pl.frames; p.groups_per_row = pl.groups_per_row; p.hop = hop; p.pad = pad;
    p.hop_lds = (int)(hop < n_fft ? hop : n_fft);
    p.win_len = (int)win_length; p.win_left = (int)((n_fft - win_length) / 2);
    p.reflect = pad > 0 && pad_mode == TFX_STFT_PAD_REFLECT; p.power = power; p.normalized = normalized;
    p.scale = (R)(1.0 / std::sqrt((double)n_fft));
    return p;
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
