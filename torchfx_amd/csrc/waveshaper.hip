// waveshaper.hip -- an oversampled memoryless nonlinearity (Waveshaper, Distortion) in ONE launch.  With L = oversample,
// h_up / h_dn the taps of resample_forward(x, L, 1) / (w, 1, L) and f a transfer function of shape_fn.h:
//   u = resample(x, L, 1);  v = drive * u + bias;  w = f(v) - c0;  z = resample(w, 1, L);  y = dry * x + wet * z
// (include/torchfx_hip.h has the definition).  Both FIR stages are recursion-free, so a tile with halos is exact: a workgroup
// owns WS_THREADS * R input positions of one row, N = WS_THREADS * R - Ku of them outputs and Ku of them the halo the decimator
// needs, reads each sample once, keeps the oversampled signal in LDS only and writes each output once.
//   stage   the positions' window (LP - 1 inputs of halo in front, zeros outside [0, T)) goes to LDS transposed (tp_stage,
//           polyphase.h), so a thread reads its R + LP - 1 consecutive inputs at consecutive addresses across lanes
//   up      thread t owns R consecutive positions and runs phase after phase over the inputs it holds in registers (tp_phase):
//           the per-output sum is resample_forward's (a descending-j fma chain from +0 over hp[phase][j]; the taps of a phase
//           are wave-uniform scalar loads through the constant address space)
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
//
// Stream form (tfx_waveshaper_stream_forward, waveshaper_kernel<T, LP, true>): the same kernel on [hist | x], a row's carried
// history and its chunk in their two buffers.  A chunk's outputs trail its inputs by the latency D = reach_before; the masks of
// the shaped signal are the stream's start and its end (or none), not the row's; the dry term comes from the staged window;
// whole waves whose positions no output of the chunk reads skip `up` and `shape`, and a chunk of at most 512 samples runs two
// of the decimator's R chains per thread.  Every sum, the transfer function and the mix are the one-shot form's source, so the
// bits agree.  The launch also writes the next chunk's history (WsStreamPlan below has the geometry).
#include "common.h"
#include "plan_cache.h"
#include "polyphase.h"
#include "shape_fn.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>
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
    // stream form only (tfx_waveshaper_stream_forward): a row is [hist | x], T_ = Nc + n_in is where its inputs end so far
    const T *hist;              // [rows, Hs] or null (silence)
    T *hist_out;                // [rows, Hs] or null
    int64_t Tc, Nc, Hs, n_in;   // chunk length (pitch of x and y), inputs before the chunk (clamped), history, real inputs
    int lat;                    // latency: output t of the chunk is stream position Nc - lat + t
    int KX;                     // a tile of n outputs reads the up-sampled samples of its positions 0 .. n + KX
    int ends;                   // n_in < Tc: the stream ends at T_, the shaped signal is cut there
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

// the decimator's sum for the outputs t + WS_THREADS * e, e < NE, of a thread: per tap one uniform (line, column offset) and NE
// independent fma chains, descending j from +0
template <typename T, int NE>
__device__ __forceinline__ void ws_decimate(T (&acc)[ws_r<T>()], const WsArgs<T> &p, const T *wbuf, int tq)
{
    constexpr int WS = ws_wstride<T>();
    constexpr int ESTEP = WS_THREADS + WS_THREADS / 32;         // ws_col(c + 256 e) - ws_col(c)
    const tp_const_ptr<T> hd = (tp_const_ptr<T>)p.hdn;
    auto term = [&](int j) {
        const int a = j & (p.L - 1), b = j >> p.logL;
        const int c = tq - b - (a != 0);
        const T *w = wbuf + ((p.L - a) & (p.L - 1)) * WS + ws_col(c);
        const T tap = hd[j];
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = tp_fma(tap, w[e * ESTEP], acc[e]);
    };
    int j = p.Lp_dn - 1;
    for (; j >= 7; j -= 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) term(j - k);
    }
    for (; j >= 0; --j) term(j);
}

// STREAM: one chunk of a stream.  Output o of tile k is chunk sample k * N + o at stream position Nc - lat + k * N + o (0 is
// written where that is negative).
template <typename T, int LP, bool STREAM>
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
    const int64_t pitch = STREAM ? p.Tc : p.T_, y0 = tile * p.N;  // rows of x and y, the tile's first sample in them
    const StreamRow<T, STREAM> xr(p.x, pitch, p.hist, p.Hs, p.Nc, p.T_, row);
    T *yr = p.y + row * pitch + y0;
    const int64_t m0 = y0 - (STREAM ? p.lat - p.Nc : 0);        // position of the tile's first output
    const int64_t left = pitch - y0;
    const int mend = (int)(left < p.N ? left : p.N);            // the tile's outputs
    // the positions whose up-sampled samples they read, in whole waves
    constexpr int WV = 64 * R;
    const int npos = STREAM ? min(PT, ((mend + p.KX) / WV + 1) * WV) : PT;
    const int span = STREAM ? npos + LP - 1 : SPAN;
    const int64_t s0 = m0 + p.I0 - (LP - 1);                    // first input of the window
    const int t = (int)threadIdx.x;
    if constexpr (STREAM) {
        if (p.hist_out)
            stream_hist_copy(p.hist_out, p.x, p.Tc, p.hist, p.n_in, p.Hs, row, tile * WS_THREADS + t, p.tiles * WS_THREADS);
    }
    const bool bad = tp_stage<R, S, WS_THREADS>(win, xr, s0, span, t);
    if (p.shape == shape_fn::CURVE)
        for (int k = t; k < p.curve_n; k += WS_THREADS) curve[k] = p.curve[k];
    const bool finite = !__syncthreads_or(bad);

    // wbuf index `rel` = (n - (m0 + CA) * L) of the up-sampled sample n; the samples of [0, T * L) are the row's (stream: from
    // the stream's start to its end, if the chunk says that it ends)
    const int64_t colA = m0 + p.CA;
    const int64_t lo64 = -colA * p.L, hi64 = (p.T_ - colA) * p.L, cap = (int64_t)p.ncols * p.L;
    const int rel_lo = (int)(lo64 < 0 ? 0 : (lo64 > cap ? cap : lo64));
    const int rel_hi = (STREAM && !p.ends) ? (int)cap : (int)(hi64 < 0 ? 0 : (hi64 > cap ? cap : hi64));

    // stream: a wave none of whose positions is read skips `up` and `shape` (wave-uniform)
    const bool active = !STREAM || __builtin_amdgcn_readfirstlane(t >> 6) * WV < npos;
    T xw[NW];
    if (finite && active) tp_window<R, S>(xw, win, t);
#pragma unroll 1
    for (int ph = 0; active && ph < p.L; ++ph) {
        T acc[R];
        if (finite) {
            tp_phase<LP>(acc, p.hup + ph * LP, xw);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = tp_phase_at<R, S>(p.hup + ph * LP, p.Lp_up, LP, win, t, r);
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
    T xv[R], acc[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const int m = t + WS_THREADS * e;
        if constexpr (STREAM) {                                 // position m0 + m is window index m - I0 + LP - 1
            xv[e] = m < mend ? tp_win_at<R, S>(win, 0, m - p.I0 + LP - 1) : (T)0;
        } else {
            xv[e] = m < mend ? xr.xr[m0 + m] : (T)0;
        }
        acc[e] = (T)0;
    }
    if (STREAM && mend <= 2 * WS_THREADS) ws_decimate<T, 2>(acc, p, wbuf, t + p.Q0);
    else ws_decimate<T, R>(acc, p, wbuf, t + p.Q0);
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const int m = t + WS_THREADS * e;
        if (m < mend) {
            const T y = shape_fn::add(shape_fn::mul(p.dry, xv[e]), shape_fn::mul(p.wet, acc[e]));
            yr[m] = (STREAM && m0 + m < 0) ? (T)0 : y;
        }
    }
}

// L = 1: no filters, y = dry x + wet (f(drive x + bias) - c0)
// ENDS (a stream's chunk with n_in < Tc real inputs per row): x[., n_in:] is not read and the outputs there are zeros
template <typename T, bool ENDS> __global__ void __launch_bounds__(WS_THREADS) waveshaper_plain_kernel(const WsArgs<T> p, int64_t n)
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
    bool real[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int64_t i = base + (int64_t)e * WS_THREADS;
        real[e] = i < n && (!ENDS || i % p.Tc < p.n_in);
        v[e] = real[e] ? p.x[i] : (T)0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int64_t i = base + (int64_t)e * WS_THREADS;
        const T y = shape_fn::add(shape_fn::mul(p.dry, v[e]), shape_fn::mul(p.wet, ws_shape<T>(p.shape, v[e], p, curve)));
        if (i < n) p.y[i] = (ENDS && !real[e]) ? (T)0 : y;
    }
}

struct WsPlan {
    int64_t L, logL, Lp_up, Lp_dn, LP, N, tiles, I0, D, Q0, CA, ncols, reach_before, reach_after, lds;
    int64_t KX;                 // a stream's (waveshaper_stream_plan), else 0
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
    // none of interp_plan's refusals can fire here: nh_up and T are checked above, nh_up <= 64 L gives Lp <= 65, and with
    // down = 1 i_lo = ((nh_up - 1) / 2 + 1) / L <= Lp - 1
    const InterpPlan ip = interp_plan(who, L, nh_up, T);
    pl.gu = ip.g;
    pl.gd = resample_geometry(T * L, 1, L, nh_dn);
    pl.Lp_up = pl.gu.Lp;
    pl.Lp_dn = pl.gd.Lp;
    pl.LP = ip.LP;
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

template <typename T>
static void waveshaper_launch(const void *x, void *y, int64_t rows, int64_t T_, int shape, const void *curve_host, int64_t curve_n,
                              double drive, double bias, double dry, double wet, const void *taps_up_host, int64_t nh_up,
                              const void *taps_dn_host, int64_t nh_dn, const WsPlan &pl, hipStream_t stream,
                              const StreamArgs *st = nullptr)
{
    std::shared_ptr<DeviceBuffer> tup, tdn, tcurve;
    WsArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.T_ = T_; p.tiles = pl.tiles; p.L = (int)pl.L; p.logL = (int)pl.logL; p.shape = shape;
    p.curve_n = (int)curve_n; p.N = (int)pl.N; p.I0 = (int)pl.I0; p.Lp_up = (int)pl.Lp_up; p.Lp_dn = (int)pl.Lp_dn; p.D = (int)pl.D;
    p.Q0 = (int)pl.Q0; p.CA = (int)pl.CA; p.ncols = (int)pl.ncols;
    p.drive = (T)drive; p.bias = (T)bias; p.dry = (T)dry; p.wet = (T)wet;
    if (st) {                                   // T_ is the chunk's length; the kernel's T_ is where the stream's inputs end so far
        p.hist = (const T *)st->hist_in; p.hist_out = (T *)st->hist_out;
        p.Tc = T_; p.Nc = st->N; p.Hs = st->Hs; p.n_in = st->n_in; p.lat = (int)st->D; p.KX = (int)pl.KX; p.ends = st->n_in < T_;
        p.T_ = st->N + st->n_in;
    }
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
        const dim3 grid((unsigned)ceil_div(n, pl.N));
        ProfScope ps(st ? "waveshaper_stream_kernel" : "waveshaper_plain_kernel", stream);
        if (st && p.ends) hipLaunchKernelGGL((waveshaper_plain_kernel<T, true>), grid, dim3(WS_THREADS), (size_t)pl.lds, stream, p, n);
        else hipLaunchKernelGGL((waveshaper_plain_kernel<T, false>), grid, dim3(WS_THREADS), (size_t)pl.lds, stream, p, n);
        TFX_HIP(hipGetLastError());
        return;
    }
    p.hup = resample_table<T>(taps_up_host, nh_up, pl.L, 1, pl.gu.pre_pad, pl.LP, stream, &tup);
    p.hdn = resample_table<T>(taps_dn_host, nh_dn, 1, pl.L, pl.gd.pre_pad, pl.Lp_dn, stream, &tdn);
    tp_dispatch(pl.LP, [&](auto lp) {
        const int64_t grid = rows * p.tiles;
        const size_t lds = (size_t)pl.lds;
        if (st) launch_dynamic_lds<waveshaper_kernel<T, lp(), true>>("waveshaper_stream_kernel", grid, WS_THREADS, lds, stream, p);
        else launch_dynamic_lds<waveshaper_kernel<T, lp(), false>>("waveshaper_kernel", grid, WS_THREADS, lds, stream, p);
    });
}

// what both entries refuse about the values (host-only)
static void waveshaper_check_values(const char *who, int dtype, int64_t oversample, int shape, const void *curve_host, double drive,
                                    double bias, double dry, double wet, const void *taps_up_host, const void *taps_dn_host)
{
    // as the kernel holds them: a double beyond float32's range rounds to Inf, and silence would shape to 0 * Inf = NaN
    auto finite = [dtype](double v) { return dtype == TFX_F32 ? std::isfinite((float)v) : std::isfinite(v); };
    TFX_CHECK(finite(drive) && finite(bias) && finite(dry) && finite(wet), "%s: drive, bias, dry and wet must be finite in %s", who,
              dtype == TFX_F32 ? "float32" : "float64");
    TFX_CHECK(shape != TFX_SHAPE_CURVE || curve_host, "%s: no curve", who);
    TFX_CHECK(oversample == 1 || (taps_up_host && taps_dn_host), "%s: no taps", who);
}

void waveshaper_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t oversample, int shape,
                        const void *curve_host, int64_t curve_n, double drive, double bias, double dry, double wet,
                        const void *taps_up_host, int64_t nh_up, const void *taps_dn_host, int64_t nh_dn, hipStream_t stream)
{
    const char *who = "waveshaper_forward";
    const WsPlan pl = waveshaper_plan(who, dtype, rows, T, oversample, nh_up, nh_dn, shape, curve_n);
    waveshaper_check_values(who, dtype, oversample, shape, curve_host, drive, bias, dry, wet, taps_up_host, taps_dn_host);
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

// ---- the stream form ------------------------------------------------------------------------------------------------------
// Geometry of a stream (oversample, nh_up, nh_dn alone: resample_geometry's pre_remove and Lp do not depend on T, whose terms
// cancel in both stages).  Output n reads the inputs n - reach_after .. n + reach_before, so it is final once input n + D is
// in, D = reach_before, and the chunk that starts with output N - D reads back to N - D - reach_after = N - Hs.  Position k of
// a tile makes the columns k + floor(D_w / L) and, when L does not divide pre_up, the next one of wbuf (D_w: WsPlan::D); the
// last column the tile's n outputs read is n - 1 + Q0, and only line 0 of it, which the earlier of its two positions makes: they
// read the positions up to n + KX, KX = Q0 - ceil(D_w / L) - 1 = reach_before - 1 - I0 (a whole tile: all PT of them).
struct WsStreamPlan {
    WsPlan pl;
    int64_t D, Hs, positions;
};

static WsStreamPlan waveshaper_stream_plan(const char *who, int dtype, int64_t rows, int64_t T, int64_t L, int64_t nh_up,
                                           int64_t nh_dn, int shape, int64_t curve_n)
{
    WsStreamPlan sp{};
    sp.pl = waveshaper_plan(who, dtype, rows, T, L, nh_up, nh_dn, shape, curve_n);
    if (L == 1) {
        sp.positions = std::min(T, sp.pl.N);
        return sp;
    }
    WsPlan &pl = sp.pl;
    const int64_t PT = dtype == TFX_F32 ? ws_positions<float>() : ws_positions<double>(), WV = PT / (WS_THREADS / 64);
    sp.D = pl.reach_before;
    sp.Hs = pl.reach_before + pl.reach_after;
    pl.KX = pl.Q0 - ceil_div(pl.D + (1 << 20) * L, L) + (1 << 20) - 1;          // ceil of a D_w that may be negative
    // the dry sample of output o is position o - I0 of the tile: staged with the positions 0 .. o + KX, at a window index >= 0
    TFX_CHECK(pl.reach_before >= 1 && pl.reach_after >= 0 && pl.I0 <= pl.LP - 1 && pl.KX == pl.reach_before - 1 - pl.I0 &&
                  pl.N + pl.KX == PT - 1,
              "%s: the filters' geometry does not fit the stream", who);
    sp.positions = T == 0 ? 0 : std::min(PT, ((std::min(T, pl.N) + pl.KX) / WV + 1) * WV);
    return sp;
}

void waveshaper_stream_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n, int dtype,
                                 int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles, int64_t *positions,
                                 int64_t *lds_bytes)
{
    const WsStreamPlan sp = waveshaper_stream_plan("waveshaper_stream_plan_info", dtype, rows, T, oversample, nh_up, nh_dn,
                                                   curve_n ? TFX_SHAPE_CURVE : TFX_SHAPE_HARD, curve_n);
    *latency = sp.D;
    *history = sp.Hs;
    *tile = sp.pl.N;
    *tiles = sp.pl.tiles;
    *positions = sp.positions;
    *lds_bytes = sp.pl.lds;
}

void waveshaper_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t n_in, int64_t consumed,
                               int64_t oversample, int shape, const void *curve_host, int64_t curve_n, double drive, double bias,
                               double dry, double wet, const void *taps_up_host, int64_t nh_up, const void *taps_dn_host,
                               int64_t nh_dn, const void *hist_in, void *hist_out, hipStream_t stream)
{
    const char *who = "waveshaper_stream_forward";
    const WsStreamPlan sp = waveshaper_stream_plan(who, dtype, rows, T, oversample, nh_up, nh_dn, shape, curve_n);
    waveshaper_check_values(who, dtype, oversample, shape, curve_host, drive, bias, dry, wet, taps_up_host, taps_dn_host);
    StreamArgs st;
    const size_t esz = dtype == TFX_F32 ? 4 : 8;
    if (!stream_enter(&st, who, esz, x, y, rows, T, n_in, consumed, sp.D, sp.Hs, hist_in, hist_out, stream)) return;
    if (dtype == TFX_F32)
        waveshaper_launch<float>(x, y, rows, T, shape, curve_host, curve_n, drive, bias, dry, wet, taps_up_host, nh_up, taps_dn_host,
                                 nh_dn, sp.pl, stream, &st);
    else
        waveshaper_launch<double>(x, y, rows, T, shape, curve_host, curve_n, drive, bias, dry, wet, taps_up_host, nh_up, taps_dn_host,
                                  nh_dn, sp.pl, stream, &st);
}

void waveshaper_clear() { g_curves.clear(); }

}  // namespace tfx

