// waveshaper.hip -- an oversampled memoryless nonlinearity (Waveshaper, Distortion) in ONE launch.  With L = oversample,
// h_up / h_dn the taps of resample_forward(x, L, 1) / (w, 1, L) and f a transfer function of shape_fn.h:
//   u = resample(x, L, 1);  v = drive * u + bias;  w = f(v) - c0;  z = resample(w, 1, L);  y = dry * x + wet * z
// (include/torchfx_hip.h has the definition).  Both FIR stages are recursion-free, so a tile with halos is exact: a workgroup
// owns WS_THREADS * R input positions of one row, N = WS_THREADS * R - Ku of them outputs and Ku of them the halo the decimator
// needs, reads each sample once, keeps the oversampled signal in LDS only and writes each output once.
//   stage   the positions' window (LP - 1 inputs of halo in front, zeros outside [0, T)) goes to LDS as true_peak_kernel's:
//           win[(k % R) * S + k / R], so a thread reads its R + LP - 1 consecutive inputs at consecutive addresses across lanes
//   up      thread t owns R consecutive positions and runs phase after phase over the inputs it holds in registers: the
//           per-output sum is resample_forward's (a descending-j fma chain from +0 over hp[phase][j]; the taps of a phase are
//           wave-uniform scalar loads through the constant address space)
//   shape   drive, bias, f, - c0 in registers; an up-sampled value that is not finite shapes to NaN; values outside [0, T*L)
//           are zeros.  The shaped sample n goes to wbuf[n mod L][n div L]: one line per phase of the decimator.  A thread's R
//           columns are consecutive, so a line's columns are spread with one pad per 32 (ws_col): the R-strided stores of a
//           wave then fall into distinct banks, and the decimator's reads stay consecutive.
//   down    thread t owns the outputs t + WS_THREADS * e (e < R): per tap j one uniform (line, column offset), R LDS reads at
//           consecutive addresses across lanes (no bank conflict at stride L: the stride is inside the line index) and R
//           independent fma chains, descending j from +0 over the zero-padded h_dn -- resample_forward(w, 1, L)'s sum
//   mix     y = dry * x + wet * z, coalesced stores
// Non-finite input.  A tile whose window is finite holds the up-sampler's taps in registers, LP >= Lp of them with zeros past
// Lp: the extra terms add +-0.  A tile whose window holds a NaN or an Inf sums exactly the Lp terms of the definition from LDS,
// so the sample poisons exactly the outputs whose windows cover it; the decimator always sums exactly its Lp_dn terms.  Either
// way an output's bits do not depend on where the tiles fall.  The tiling is fixed: it does not depend on the row count.
#include "common.h"
#include "plan_cache.h"
#include "polyphase.h"
#include "shape_fn.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <vector>

namespace tfx {

constexpr int WS_THREADS = 256;
constexpr int WS_PAD = 72;                                  // columns a masked output may read past the tile's last one
constexpr int64_t WS_CURVE_MAX = 4096;

template <typename T> constexpr int ws_r() { return sizeof(T) == 4 ? 8 : 4; }                  // positions per thread
template <typename T> constexpr int ws_positions() { return WS_THREADS * ws_r<T>(); }           // per workgroup
// window line stride: 256 columns + up to ceil(71 / R) of halo; f32 S = 4 (mod 32), f64 S = 4 (mod 16): the consecutive
// window indices of a staging store fall into distinct banks
template <typename T> constexpr int ws_stride() { return sizeof(T) == 4 ? 292 : 276; }
template <typename T> constexpr int ws_wstride() { return ws_positions<T>() + ws_positions<T>() / 32 + WS_PAD; }
__host__ __device__ inline int ws_col(int c) { return c + (c >> 5); }

template <typename T> struct WsArgs {
    const T *x;                 // [rows, T_]
    T *y;                       // [rows, T_]
    const T *hup;               // [L, LP]: resample_table's layout, zeros past Lp_up
    const T *hdn;               // [Lp_dn]: the zero-padded decimator
    const T *curve;             // [curve_n] or null
    int64_t T_, tiles;
    int L, logL, shape, curve_n;
    int N;                      // outputs per tile
    int I0;                     // the tile's first position, counted from its first output
    int Lp_up, Lp_dn;
    int D;                      // wbuf index (column * L + line) of position 0, phase 0
    int Q0;                     // column of the sample tap 0 of the tile's first output reads
    int CA;                     // absolute column of wbuf's column 0, counted from the tile's first output
    int ncols;                  // columns the decimator reads: N + Q0
    T drive, bias, c0, dry, wet;
};

template <typename T> __device__ __forceinline__ T ws_shape(int shape, T u, const WsArgs<T> &p, const T *curve)
{
    const T v = shape_fn::add(shape_fn::mul(p.drive, u), p.bias);
    const T w = shape_fn::add(shape_fn::apply(shape, v, curve, p.curve_n), -p.c0);
    return isfinite(u) ? w : (T)NAN;
}

// the R shaped outputs of one phase into their line of wbuf; SHAPE is a constant so that the loop holds no switch
template <typename T, int SHAPE>
__device__ __forceinline__ void ws_store(const T (&acc)[ws_r<T>()], const WsArgs<T> &p, const T *curve, T *wline, int col0, int line,
                                         int rel_lo, int rel_hi)
{
    constexpr int R = ws_r<T>();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int col = col0 + r, rel = col * p.L + line;
        const T w = ws_shape<T>(SHAPE, acc[r], p, curve);
        if (col >= 0 && col < p.ncols) wline[ws_col(col)] = (rel >= rel_lo && rel < rel_hi) ? w : (T)0;
    }
}

template <typename T, int LP>
__global__ void __launch_bounds__(WS_THREADS) waveshaper_kernel(const WsArgs<T> p)
{
    constexpr int R = ws_r<T>(), S = ws_stride<T>(), WS = ws_wstride<T>(), PT = ws_positions<T>();
    constexpr int NW = R + LP - 1, SPAN = PT + LP - 1;
    static_assert(WS_THREADS + (LP - 2) / R + 1 <= S, "the halo columns must fit the line");
    extern __shared__ __align__(16) unsigned char ws_lds_raw[];
    T *win = (T *)ws_lds_raw;                                   // [R][S]
    T *wbuf = win + R * S;                                      // [L][WS]
    T *curve = wbuf + p.L * WS;                                 // [curve_n]
    const int64_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const T *xr = p.x + row * p.T_;
    T *yr = p.y + row * p.T_;
    const int64_t m0 = tile * p.N;
    const int64_t s0 = m0 + p.I0 - (LP - 1);                    // first input of the window
    const int t = (int)threadIdx.x;
    bool bad = false;
    for (int j0 = 0; j0 < SPAN; j0 += WS_THREADS * RS_STAGE_BATCH) {
        T v[RS_STAGE_BATCH];
#pragma unroll
        for (int u = 0; u < RS_STAGE_BATCH; ++u) {
            const int j = j0 + u * WS_THREADS + t;
            const int64_t i = s0 + j;
            v[u] = (j < SPAN && i >= 0 && i < p.T_) ? xr[i] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < RS_STAGE_BATCH; ++u) {
            const int j = j0 + u * WS_THREADS + t;
            if (j < SPAN) win[(j % R) * S + j / R] = v[u];
            bad |= !isfinite(v[u]);
        }
    }
    if (p.shape == shape_fn::CURVE)
        for (int k = t; k < p.curve_n; k += WS_THREADS) curve[k] = p.curve[k];
    const bool finite = !__syncthreads_or(bad);

    // wbuf index `rel` = (n - (m0 + CA) * L) of the up-sampled sample n; the samples of [0, T * L) are the row's
    const int64_t colA = m0 + p.CA;
    const int64_t lo64 = -colA * p.L, hi64 = (p.T_ - colA) * p.L, cap = (int64_t)p.ncols * p.L;
    const int rel_lo = (int)(lo64 < 0 ? 0 : (lo64 > cap ? cap : lo64)), rel_hi = (int)(hi64 < 0 ? 0 : (hi64 > cap ? cap : hi64));

    T xw[NW];
    if (finite) {
#pragma unroll
        for (int k = 0; k < NW; ++k) xw[k] = win[(k % R) * S + t + k / R];
    }
#pragma unroll 1
    for (int ph = 0; ph < p.L; ++ph) {
        T acc[R];
        if (finite) {
            const tp_const_ptr<T> h = (tp_const_ptr<T>)(p.hup + ph * LP);
            T tap[LP];
#pragma unroll
            for (int j = 0; j < LP; ++j) tap[j] = h[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = tp_fma0(tap[LP - 1], xw[r]);
#pragma unroll
            for (int j = LP - 2; j >= 0; --j)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = tp_fma(tap[j], xw[r + LP - 1 - j], acc[r]);
        } else {
            const T *h = p.hup + ph * LP;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                T a = (T)0;
                for (int j = p.Lp_up - 1; j >= 0; --j) {
                    const int k = r + LP - 1 - j;
                    a = fma(h[j], win[(k % R) * S + t + k / R], a);
                }
                acc[r] = a;
            }
        }
        const int sh = ph + p.D, line = sh & (p.L - 1), col0 = t * R + (sh >> p.logL);
        T *wline = wbuf + line * WS;
        switch (p.shape) {
        case shape_fn::HARD: ws_store<T, shape_fn::HARD>(acc, p, curve, wline, col0, line, rel_lo, rel_hi); break;
        case shape_fn::CUBIC: ws_store<T, shape_fn::CUBIC>(acc, p, curve, wline, col0, line, rel_lo, rel_hi); break;
        case shape_fn::TANH: ws_store<T, shape_fn::TANH>(acc, p, curve, wline, col0, line, rel_lo, rel_hi); break;
        default: ws_store<T, shape_fn::CURVE>(acc, p, curve, wline, col0, line, rel_lo, rel_hi); break;
        }
    }
    __syncthreads();

    // the decimator: output m0 + t + 256 e reads, for tap j = b L + a, line (L - a) mod L at column t + 256 e + Q0 - b - (a > 0)
    const int64_t left = p.T_ - m0;
    const int mend = (int)(left < p.N ? left : p.N);
    T xv[R], acc[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const int m = t + WS_THREADS * e;
        xv[e] = m < mend ? xr[m0 + m] : (T)0;
        acc[e] = (T)0;
    }
    const tp_const_ptr<T> hd = (tp_const_ptr<T>)p.hdn;
    const int tq = t + p.Q0;
    constexpr int ESTEP = WS_THREADS + WS_THREADS / 32;         // ws_col(c + 256 e) - ws_col(c)
    auto term = [&](int j) {
        const int a = j & (p.L - 1), b = j >> p.logL;
        const int c = tq - b - (a != 0);
        const T *w = wbuf + ((p.L - a) & (p.L - 1)) * WS + ws_col(c);
        const T tap = hd[j];
#pragma unroll
        for (int e = 0; e < R; ++e) acc[e] = tp_fma(tap, w[e * ESTEP], acc[e]);
    };
    int j = p.Lp_dn - 1;
    for (; j >= 7; j -= 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) term(j - k);
    }
    for (; j >= 0; --j) term(j);
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const int m = t + WS_THREADS * e;
        if (m < mend) yr[m0 + m] = shape_fn::add(shape_fn::mul(p.dry, xv[e]), shape_fn::mul(p.wet, acc[e]));
    }
}

// L = 1: no filters, y = dry x + wet (f(drive x + bias) - c0)
template <typename T> __global__ void __launch_bounds__(WS_THREADS) waveshaper_plain_kernel(const WsArgs<T> p, int64_t n)
{
    extern __shared__ __align__(16) unsigned char ws_lds_raw[];
    T *curve = (T *)ws_lds_raw;
    if (p.shape == shape_fn::CURVE) {
        for (int k = (int)threadIdx.x; k < p.curve_n; k += WS_THREADS) curve[k] = p.curve[k];
        __syncthreads();
    }
    constexpr int E = 4;
    const int64_t base = (int64_t)blockIdx.x * (WS_THREADS * E) + threadIdx.x;
    T v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int64_t i = base + (int64_t)e * WS_THREADS;
        v[e] = i < n ? p.x[i] : (T)0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int64_t i = base + (int64_t)e * WS_THREADS;
        if (i < n) p.y[i] = shape_fn::add(shape_fn::mul(p.dry, v[e]), shape_fn::mul(p.wet, ws_shape<T>(p.shape, v[e], p, curve)));
    }
}

struct WsPlan {
    int64_t L, logL, Lp_up, Lp_dn, LP, N, tiles, I0, D, Q0, CA, ncols, reach_before, reach_after, lds;
    ResampleGeom gu, gd;
};

// everything but the pointers (host-only)
static WsPlan waveshaper_plan(const char *who, int dtype, int64_t rows, int64_t T, int64_t L, int64_t nh_up, int64_t nh_dn,
                              int shape, int64_t curve_n)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", who, dtype);
    TFX_CHECK(L == 1 || L == 2 || L == 4 || L == 8, "%s: oversample must be 1, 2, 4 or 8, got %lld", who, (long long)L);
    TFX_CHECK(rows >= 0 && T >= 0, "%s: negative size", who);
    TFX_CHECK(shape >= TFX_SHAPE_HARD && shape <= TFX_SHAPE_CURVE, "%s: bad shape %d", who, shape);
    if (shape == TFX_SHAPE_CURVE)
        TFX_CHECK(curve_n >= 2 && curve_n <= WS_CURVE_MAX, "%s: a curve must have 2 to %lld points, got %lld", who,
                  (long long)WS_CURVE_MAX, (long long)curve_n);
    else
        TFX_CHECK(curve_n == 0, "%s: %lld curve points with a shape that is no curve", who, (long long)curve_n);
    TFX_CHECK(T <= (INT64_MAX / 64) / L, "%s: T * oversample overflows", who);
    TFX_CHECK(rows == 0 || T <= INT64_MAX / 16 / rows, "%s: size overflows", who);
    const int esz = dtype == TFX_F32 ? 4 : 8;
    const int64_t curve_bytes = shape == TFX_SHAPE_CURVE ? curve_n * esz : 0;
    WsPlan pl{};
    pl.L = L;
    if (L == 1) {
        pl.N = WS_THREADS * 4;
        pl.tiles = ceil_div(T, pl.N);
        pl.lds = curve_bytes;
        TFX_CHECK(ceil_div(rows * T, pl.N) < (1ll << 31), "%s: grid too large", who);
        return pl;
    }
    TFX_CHECK(nh_up >= 1 && nh_dn >= 1, "%s: no taps", who);
    TFX_CHECK(nh_up <= 64 * L && nh_dn <= 64 * L, "%s: %lld and %lld taps, each stage takes at most 64 * oversample = %lld", who,
              (long long)nh_up, (long long)nh_dn, (long long)(64 * L));
    pl.logL = L == 2 ? 1 : (L == 4 ? 2 : 3);
    pl.gu = resample_geometry(T, L, 1, nh_up);
    pl.gd = resample_geometry(T * L, 1, L, nh_dn);
    pl.Lp_up = pl.gu.Lp;
    pl.Lp_dn = pl.gd.Lp;
    TFX_CHECK(pl.Lp_up <= TP_LP_MAX, "%s: %lld taps per phase", who, (long long)pl.Lp_up);
    pl.LP = tp_bucket(pl.Lp_up);
    const int64_t PT = dtype == TFX_F32 ? ws_positions<float>() : ws_positions<double>();
    const int64_t WS = dtype == TFX_F32 ? ws_wstride<float>() : ws_wstride<double>();
    const int64_t RS = dtype == TFX_F32 ? ws_r<float>() * ws_stride<float>() : ws_r<double>() * ws_stride<double>();
    const int64_t pre_up = pl.gu.pre_remove, pre_dn = pl.gd.pre_remove;
    // the decimator's output m reads the up-sampled samples (m + pre_dn) L - j, j < Lp_dn; sample n reads the inputs
    // (n + pre_up) / L - j, j < Lp_up
    const int64_t first = pre_dn * L - pl.Lp_dn + 1;            // the first sample output 0 reads
    pl.CA = floor_div(first, L);
    pl.Q0 = pre_dn - pl.CA;
    pl.I0 = floor_div(first + pre_up, L);
    const int64_t Ku = pre_dn + pre_up / L - pl.I0;             // positions of a tile that are halo
    pl.N = PT - Ku;
    pl.ncols = pl.N + pl.Q0;
    pl.D = pl.I0 * L - pre_up - pl.CA * L;
    pl.reach_before = pre_dn + pre_up / L;
    pl.reach_after = pl.Lp_up - 1 - pl.I0;
    TFX_CHECK(pl.N >= PT / 2 && pl.Q0 >= 0 && pl.Q0 * L - pl.Lp_dn + 1 >= 0 && pl.Q0 <= WS_PAD - 3 && pl.D <= L - 1 && pl.D > -(1 << 20) &&
                  ws_col((int)(PT - 1 + pl.Q0)) < WS,
              "%s: the filters' geometry does not fit the tile", who);
    pl.tiles = ceil_div(T, pl.N);
    pl.lds = (RS + L * WS) * esz + curve_bytes;
    TFX_CHECK(rows == 0 || pl.tiles < (1ll << 31) / rows, "%s: grid too large", who);
    return pl;
}

void waveshaper_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n, int dtype,
                          int64_t *tile, int64_t *tiles, int64_t *reach_before, int64_t *reach_after, int64_t *lds_bytes,
                          int64_t *taps_up, int64_t *taps_dn)
{
    const WsPlan pl = waveshaper_plan("waveshaper_plan_info", dtype, rows, T, oversample, nh_up, nh_dn,
                                      curve_n ? TFX_SHAPE_CURVE : TFX_SHAPE_HARD, curve_n);
    *tile = pl.N;
    *tiles = pl.tiles;
    *reach_before = pl.reach_before;
    *reach_after = pl.reach_after;
    *lds_bytes = pl.lds;
    *taps_up = pl.Lp_up;
    *taps_dn = pl.Lp_dn;
}

// curve tables by content (the bytes plus the element size)
static PlanCache<DeviceBuffer, 1> g_curves(32, "waveshaper_forward");

template <typename T, int LP> static void waveshaper_launch_lp(const WsArgs<T> &p, int64_t rows, size_t lds, hipStream_t stream)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if (lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)waveshaper_kernel<T, LP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        have = lds;
    }
    ProfScope ps("waveshaper_kernel", stream);
    hipLaunchKernelGGL((waveshaper_kernel<T, LP>), dim3((unsigned)(rows * p.tiles)), dim3(WS_THREADS), lds, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename T>
static void waveshaper_launch(const void *x, void *y, int64_t rows, int64_t T_, int shape, const void *curve_host, int64_t curve_n,
                              double drive, double bias, double dry, double wet, const void *taps_up_host, int64_t nh_up,
                              const void *taps_dn_host, int64_t nh_dn, const WsPlan &pl, hipStream_t stream)
{
    std::shared_ptr<DeviceBuffer> tup, tdn, tcurve;
    WsArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.T_ = T_; p.tiles = pl.tiles; p.L = (int)pl.L; p.logL = (int)pl.logL; p.shape = shape;
    p.curve_n = (int)curve_n; p.N = (int)pl.N; p.I0 = (int)pl.I0; p.Lp_up = (int)pl.Lp_up; p.Lp_dn = (int)pl.Lp_dn; p.D = (int)pl.D;
    p.Q0 = (int)pl.Q0; p.CA = (int)pl.CA; p.ncols = (int)pl.ncols;
    p.drive = (T)drive; p.bias = (T)bias; p.dry = (T)dry; p.wet = (T)wet;
    // c0 = f(bias) in float64 (bias and the curve as the signal's dtype holds them), rounded once
    std::vector<double> cd;
    if (shape == TFX_SHAPE_CURVE) {
        const T *c = (const T *)curve_host;
        cd.assign(c, c + curve_n);
        const int64_t tail[1] = {(int64_t)sizeof(T)};
        tcurve = g_curves.get(curve_host, (size_t)curve_n * sizeof(T), tail, stream,
                              [&] { return std::make_shared<DeviceBuffer>(curve_host, (size_t)curve_n * sizeof(T)); });
        p.curve = (const T *)tcurve->p;
    }
    p.c0 = (T)shape_fn::apply<double, double>(shape, (double)p.bias, cd.data(), (int)curve_n);
    if (pl.L == 1) {
        const int64_t n = rows * T_;
        ProfScope ps("waveshaper_plain_kernel", stream);
        hipLaunchKernelGGL((waveshaper_plain_kernel<T>), dim3((unsigned)ceil_div(n, pl.N)), dim3(WS_THREADS), (size_t)pl.lds, stream, p, n);
        TFX_HIP(hipGetLastError());
        return;
    }
    p.hup = resample_table<T>(taps_up_host, nh_up, pl.L, 1, pl.gu.pre_pad, pl.LP, stream, &tup);
    p.hdn = resample_table<T>(taps_dn_host, nh_dn, 1, pl.L, pl.gd.pre_pad, pl.Lp_dn, stream, &tdn);
    switch (pl.LP) {
    case 8: waveshaper_launch_lp<T, 8>(p, rows, (size_t)pl.lds, stream); break;
    case 16: waveshaper_launch_lp<T, 16>(p, rows, (size_t)pl.lds, stream); break;
    case 24: waveshaper_launch_lp<T, 24>(p, rows, (size_t)pl.lds, stream); break;
    case 32: waveshaper_launch_lp<T, 32>(p, rows, (size_t)pl.lds, stream); break;
    case 48: waveshaper_launch_lp<T, 48>(p, rows, (size_t)pl.lds, stream); break;
    case 64: waveshaper_launch_lp<T, 64>(p, rows, (size_t)pl.lds, stream); break;
    default: waveshaper_launch_lp<T, (int)TP_LP_MAX>(p, rows, (size_t)pl.lds, stream); break;
    }
}

void waveshaper_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t oversample, int shape,
                        const void *curve_host, int64_t curve_n, double drive, double bias, double dry, double wet,
                        const void *taps_up_host, int64_t nh_up, const void *taps_dn_host, int64_t nh_dn, hipStream_t stream)
{
    const char *who = "waveshaper_forward";
    const WsPlan pl = waveshaper_plan(who, dtype, rows, T, oversample, nh_up, nh_dn, shape, curve_n);
    TFX_CHECK(std::isfinite(drive) && std::isfinite(bias) && std::isfinite(dry) && std::isfinite(wet),
              "%s: drive, bias, dry and wet must be finite", who);
    TFX_CHECK(shape != TFX_SHAPE_CURVE || curve_host, "%s: no curve", who);
    TFX_CHECK(oversample == 1 || (taps_up_host && taps_dn_host), "%s: no taps", who);
    TFX_CHECK(rows * T == 0 || (x && y), "%s: null pointer", who);
    const int64_t esz = dtype == TFX_F32 ? 4 : 8;
    const char *xb = (const char *)x, *yb = (const char *)y;
    TFX_CHECK(rows * T == 0 || xb + rows * T * esz <= yb || yb + rows * T * esz <= xb, "%s: y may not overlap x", who);
    if (rows * T == 0) return;
    if (dtype == TFX_F32)
        waveshaper_launch<float>(x, y, rows, T, shape, curve_host, curve_n, drive, bias, dry, wet, taps_up_host, nh_up, taps_dn_host,
                                 nh_dn, pl, stream);
    else
        waveshaper_launch<double>(x, y, rows, T, shape, curve_host, curve_n, drive, bias, dry, wet, taps_up_host, nh_up, taps_dn_host,
                                  nh_dn, pl, stream);
}

void waveshaper_clear() { g_curves.clear(); }

}  // namespace tfx
