// limiter.hip -- look-ahead true-peak limiter in ONE launch (tfx_limiter_forward).  For a group of `channels` rows that share
// one gain curve, in the signal's dtype (include/torchfx_hip.h has the full contract):
//   q[ch,i] = max_ph |v[ch, i*up + ph]|, v = resample_forward(x[ch], up, 1)         (up = 1: no q)
//   p[i]    = max_ch max(|x[ch,i]|, q[ch,i], q[ch,i-1])                              (up = 1: max_ch |x[ch,i]|)
//   r[i]    = p[i] > c ? c / p[i] : 1,  1 outside [0, T)
//   m[k]    = min r[k-H+1 .. k+A-1]
//   s[n]    = fma chain from +0 over j = A-1 .. 0 of w[j] * (1 - m[n-j])
//   g[n]    = min(max(1 - s[n], 0), r[n]);   y[ch,n] = g[n] * x[ch,n]
// No recursion: an output depends on inputs A+H-2 (+ the interpolator's reach) behind and A-1 ahead, so tiles with halos are
// exact and a group's bits do not depend on the batch.
//
// Work unit.  A workgroup of 256 threads is one tile of `tile` = LM_NR + 1 - 2A - H consecutive outputs of one group, and owns
// LM_NR = 8192 consecutive positions of p / r: the tile, A+H-2 behind, A-1 ahead and one spare at either end.
//   detect   channel by channel, in two passes of TP_TILE = 4096 positions: the pass's input window is staged transposed in
//            LDS and every thread runs the interpolator chain of polyphase.h on 16 consecutive positions (taps of a phase as
//            scalar loads, v_fmac_f32 by hand; written out below, not through tp_stage / tp_window / tp_phase).  Table phase ph' of position i is output
//            m = i*up + ph' - rem (rem = n_pre_remove mod up): phases below rem belong to sample i-1 (lo), the others to i
//            (hi).  p[i] = max(|x_i|, hi[i], lo[i+1], hi[i-1], lo[i]) is accumulated in LDS over the channels; the two terms
//            from a neighbouring thread's positions are added in a second, barrier-separated step, each LDS word written by
//            one thread per step.  No atomics.
//   r        one correctly rounded division per position
//   m        exact sliding minimum by log-step doubling in LDS (min over 2^k, then two overlapping windows), staged through
//            registers so it runs in place
//   s, g     1 - m is stored transposed like the input window; a thread takes 16 consecutive outputs and, per block of 16
//            weights (scalar loads), reads 31 values and issues 256 fma, j descending
//   apply    a second loop over the channels multiplies and stores (coalesced; the tile's re-read comes from cache)
// p / r live at index a + a/16 (a thread's 16 consecutive words and a wave's strided sweep both spread over the banks).
// LDS: (8704 + 8736) elements = 69 760 B float32 (two workgroups per CU), 139 520 B float64 (one).
// Non-finite: a tile whose staged windows hold a NaN or an Inf in any channel writes NaN to all its outputs of the group.
//
// Stream form (tfx_limiter_stream_forward, limiter_kernel<T, LP, true>): the same kernel on [hist | x], a row's carried history
// and its chunk in their two buffers.  A chunk's outputs trail its inputs by the latency D, a tile sweeps only the positions its
// outputs depend on, and the launch also writes the next chunk's history (LimiterStreamPlan below has the geometry).
#include "common.h"
#include "plan_cache.h"
#include "polyphase.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace tfx {

constexpr int LM_THREADS = TP_THREADS;
constexpr int LM_NR = 2 * (int)TP_TILE;                   // positions of p / r per workgroup
constexpr int LM_PAD = LM_NR + LM_NR / 16;                // ... stored at a + a/16
constexpr int LM_SD = 546;                                // line stride of the transposed 1 - m: 2 (mod 32), >= 8736 / 16
constexpr int LM_REGION = TP_R * LM_SD;                   // input window, then m, then 1 - m
constexpr int LM_EPT = LM_NR / LM_THREADS;                // 32 positions per thread in a strided sweep
constexpr int LM_DE = LM_EPT + 1;                         // 1 - m has up to tile + roundup(A, 16) - 1 <= 33 * 256 entries
constexpr int64_t LM_A_MAX = 512, LM_H_MAX = 4096;

template <typename T> struct LimiterArgs {
    const T *x;                 // [groups, channels, T_]
    T *y;                       // [groups, channels, T_]
    T *gain;                    // [groups, T_] or null
    const T *hp;                // [up, LP]: resample_table's layout with LP >= Lp taps per phase; unused for up = 1
    const T *w;                 // [Apad]: the smoothing weights, zeros past A
    int64_t T_, tiles, up;
    int64_t i_lo, n_lo, n_hi;   // interp_plan's i_lo; n = i*up + phase is an output for n in [n_lo, n_hi)
    int channels, A, Apad, H, tile;
    int rem;                    // n_pre_remove mod up
    int xoff;                   // LP - 1 - i_lo: window offset of a position's own sample
    T c;
    // stream form only (tfx_limiter_stream_forward): a row is [hist | x], T_ = N + n_in is where the stream ends so far
    const T *hist;              // [groups, channels, Hs] or null (silence)
    T *hist_out;                // [groups, channels, Hs] or null
    int64_t Tc, N, Hs, n_in;    // chunk length (pitch of x, y and gain), inputs before the chunk (clamped), history, real inputs
    int D;                      // latency: output t of the chunk is stream position N - D + t
};

// a row by sample position: x[row] over [0, T_), or the stream's [hist | x]
template <typename T, bool STREAM> __device__ __forceinline__ StreamRow<T, STREAM> lm_row(const LimiterArgs<T> &p, int64_t row)
{
    return StreamRow<T, STREAM>(p.x, STREAM ? p.Tc : p.T_, p.hist, p.Hs, p.N, p.T_, row);
}

__device__ __forceinline__ int lm_idx(int a) { return a + (a >> 4); }
template <typename T> __device__ __forceinline__ T lm_max(T a, T b) { return b > a ? b : a; }
template <typename T> __device__ __forceinline__ T lm_min(T a, T b) { return b < a ? b : a; }
__device__ __forceinline__ float lm_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double lm_div(double a, double b) { return a / b; }

// LP > 0: `up`x interpolator with LP taps per phase in registers;  LP == 0: up = 1, the sample peak.
// STREAM: one chunk of a stream.  Output o of tile k is chunk sample t = k * tile + o at stream position N - D + t (0 is written
// where that is negative); the tile's `nout` outputs depend on positions a < np = nout + 2A + H - 2 of p / r only, and every
// phase below sweeps those alone (a 512-sample block: about 1100 of the 8192).  The arithmetic per output is the one-shot
// form's, so the bits agree.  The blocks of a group also copy the newest Hs samples of [hist | x[:n_in]] to hist_out.
template <typename T, int LP, bool STREAM>
__global__ void __launch_bounds__(LM_THREADS) limiter_kernel(const LimiterArgs<T> p)
{
    constexpr int S = tp_stride<T>(), NW = TP_R + (LP > 0 ? LP : 1) - 1, SPAN = (int)TP_TILE + (LP > 0 ? LP : 1) - 1;
    static_assert(TP_R * S <= LM_REGION, "the input window must fit the shared region");
    extern __shared__ unsigned char lm_lds_raw[];
    T *rr = (T *)lm_lds_raw;                                     // p, then r, then g at lm_idx(a)
    T *reg = rr + LM_PAD;                                        // LM_REGION
    const int t = (int)threadIdx.x;
    const int64_t grp = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int64_t n0 = tile * p.tile - (STREAM ? p.D - p.N : 0);  // position of the tile's first output
    const int64_t rb = n0 - (p.A + p.H - 1);                     // sample of position a = 0
    const int64_t left = (STREAM ? p.Tc : p.T_) - tile * p.tile;
    const int nout = left < p.tile ? (int)left : p.tile;         // the tile's outputs
    const int np = STREAM ? nout + 2 * p.A + p.H - 2 : LM_NR;    // positions of p / r they depend on (a = 0 is spare)
    if constexpr (STREAM) {
        if (p.hist_out)
            for (int ch = 0; ch < p.channels; ++ch)
                stream_hist_copy(p.hist_out, p.x, p.Tc, p.hist, p.n_in, p.Hs, grp * p.channels + ch, tile * LM_THREADS + t,
                                 p.tiles * LM_THREADS);
    }
    {
        const int nz = (STREAM && np + 2 * TP_R < LM_NR) ? np + 2 * TP_R : LM_NR;
        for (int a = t; a < nz; a += LM_THREADS) rr[lm_idx(a)] = (T)0;
    }
    bool bad = false;
    if constexpr (LP == 0) {
        for (int ch = 0; ch < p.channels; ++ch) {
            const auto xr = lm_row<T, STREAM>(p, grp * p.channels + ch);
            for (int a = t; a < np; a += LM_THREADS) {           // a thread's own words only: no barrier
                const T v = xr.at(rb + a);
                bad |= !isfinite(v);
                rr[lm_idx(a)] = lm_max(rr[lm_idx(a)], (T)fabs(v));
            }
        }
    } else {
        const int up = (int)p.up;
        // positions 0 .. np feed p[a], a < np (p[a] takes a term from a + 1): the passes and the threads of a pass that hold one
        const int passes = (STREAM && np < (int)TP_TILE) ? 1 : LM_NR / (int)TP_TILE;
        for (int ch = 0; ch < p.channels; ++ch) {
            const auto xr = lm_row<T, STREAM>(p, grp * p.channels + ch);
            for (int ps = 0; ps < passes; ++ps) {
                const int a0 = ps * (int)TP_TILE + t * TP_R;     // the thread's first position
                const bool live = !STREAM || a0 <= np;
                const int span = STREAM ? min(SPAN, (np - ps * (int)TP_TILE) / TP_R * TP_R + NW) : SPAN;
                const int64_t s0 = p.i_lo + rb + ps * TP_TILE - (LP - 1);       // first input of the window
                // What follows is polyphase.h's tp_stage, tp_window, tp_phase (scalar-operand fma for LP >= 64) and tp_phase_at,
                // written out over tp_win_at and tp_fma.  Through the four helpers this kernel's registers are allocated
                // differently and a single workgroup's full sweep measured 0.4 to 0.8 % slower; written out, every kernel
                // has the instruction count it had before polyphase.h held the chain (profiles/interp_chain_refactor.txt).
                for (int j0 = 0; j0 < span; j0 += LM_THREADS * RS_STAGE_BATCH) {
                    T v[RS_STAGE_BATCH];
#pragma unroll
                    for (int u = 0; u < RS_STAGE_BATCH; ++u) {
                        const int j = j0 + u * LM_THREADS + t;
                        v[u] = j < span ? xr.at(s0 + j) : (T)0;
                    }
#pragma unroll
                    for (int u = 0; u < RS_STAGE_BATCH; ++u) {
                        const int j = j0 + u * LM_THREADS + t;
                        if (j < span) tp_win_at<TP_R, S>(reg, 0, j) = v[u];
                        bad |= !isfinite(v[u]);
                    }
                }
                __syncthreads();                                 // window staged; the last pass's neighbour terms are in
                T hi[TP_R], lo[TP_R];
#pragma unroll
                for (int r = 0; r < TP_R; ++r) hi[r] = lo[r] = (T)0;
                const int64_t nf = (p.i_lo + rb + a0) * p.up;    // n of the thread's first position, phase 0
                if (!live) {
                    // nothing of this thread's 16 positions is needed
                } else if (nf >= p.n_lo && nf + (int64_t)TP_R * up <= p.n_hi) {
                    T xw[NW];
#pragma unroll
                    for (int k = 0; k < NW; ++k) xw[k] = tp_win_at<TP_R, S>(reg, t, k);
#pragma unroll 1
                    for (int ph = 0; ph < up; ++ph) {
                        const tp_const_ptr<T> h = (tp_const_ptr<T>)(p.hp + ph * LP);
                        T tap[LP > 0 ? LP : 1];
#pragma unroll
                        for (int j = 0; j < LP; ++j) tap[j] = h[j];
                        T acc[TP_R];                             // LP >= 64: no vector registers left for taps, scalar operands
#pragma unroll
                        for (int r = 0; r < TP_R; ++r) acc[r] = LP >= 64 ? tp_fma<true>(tap[LP - 1], xw[r], (T)0) : tp_fma0(tap[LP - 1], xw[r]);
#pragma unroll
                        for (int j = LP - 2; j >= 0; --j)
#pragma unroll
                            for (int r = 0; r < TP_R; ++r) acc[r] = tp_fma<(LP >= 64)>(tap[j], xw[r + LP - 1 - j], acc[r]);
                        if (ph < p.rem) {
#pragma unroll
                            for (int r = 0; r < TP_R; ++r) lo[r] = lm_max(lo[r], (T)fabs(acc[r]));
                        } else {
#pragma unroll
                            for (int r = 0; r < TP_R; ++r) hi[r] = lm_max(hi[r], (T)fabs(acc[r]));
                        }
                    }
                } else if (nf < p.n_hi && nf + (int64_t)TP_R * up > p.n_lo) {
#pragma unroll 1
                    for (int r = 0; r < TP_R; ++r) {
                        T h_ = (T)0, l_ = (T)0;
                        for (int ph = 0; ph < up; ++ph) {
                            const int64_t n = nf + (int64_t)r * up + ph;
                            if (n < p.n_lo || n >= p.n_hi) continue;
                            const T *h = p.hp + ph * LP;
                            T acc = (T)0;
                            for (int j = LP - 1; j >= 0; --j) acc = fma(h[j], tp_win_at<TP_R, S>(reg, t, r + LP - 1 - j), acc);
                            if (ph < p.rem) l_ = lm_max(l_, (T)fabs(acc));
                            else h_ = lm_max(h_, (T)fabs(acc));
                        }
#pragma unroll
                        for (int rr_ = 0; rr_ < TP_R; ++rr_)
                            if (rr_ == r) hi[rr_] = h_, lo[rr_] = l_;
                    }
                }
                // step 1: a thread's own 16 positions
#pragma unroll
                for (int r = 0; r < TP_R && live; ++r) {
                    T v = lm_max(lm_max(hi[r], lo[r]), (T)fabs(tp_win_at<TP_R, S>(reg, t, r + p.xoff)));
                    if (r + 1 < TP_R) v = lm_max(v, lo[r + 1 < TP_R ? r + 1 : r]);
                    if (r > 0) v = lm_max(v, hi[r > 0 ? r - 1 : 0]);
                    const int ix = lm_idx(a0 + r);
                    rr[ix] = lm_max(rr[ix], v);
                }
                __syncthreads();                                 // also: every read of the window is done
                // step 2: the two terms that belong to a neighbour's position
                if (live && a0 > 0) rr[lm_idx(a0 - 1)] = lm_max(rr[lm_idx(a0 - 1)], lo[0]);
                if (live && a0 + TP_R < LM_NR) rr[lm_idx(a0 + TP_R)] = lm_max(rr[lm_idx(a0 + TP_R)], hi[TP_R - 1]);
            }
        }
    }
    const int64_t pitch = STREAM ? p.Tc : p.T_, y0 = tile * p.tile;    // rows of y / gain, the tile's first sample in them
    if (__syncthreads_or(bad)) {
        const T nan = (T)NAN;
        for (int ch = 0; ch < p.channels; ++ch) {
            T *yr = p.y + (grp * p.channels + ch) * pitch + y0;
            for (int o = t; o < nout; o += LM_THREADS) yr[o] = (STREAM && n0 + o < 0) ? (T)0 : nan;
        }
        if (p.gain)
            for (int o = t; o < nout; o += LM_THREADS) p.gain[grp * pitch + y0 + o] = (STREAM && n0 + o < 0) ? (T)1 : nan;
        return;
    }
    // r, and its copy the sliding minimum starts from
    for (int a = t; a < np; a += LM_THREADS) {
        const int64_t i = rb + a;
        const T pv = rr[lm_idx(a)];
        const T rv = (i >= 0 && i < p.T_ && pv > p.c) ? lm_div(p.c, pv) : (T)1;
        rr[lm_idx(a)] = rv;
        reg[a] = rv;
    }
    __syncthreads();
    // reg[a] = min r[a .. a + w - 1], w doubling while 2w <= W = A + H - 1
    const int W = p.A + p.H - 1;
    int w = 1;
    while (2 * w <= W) {
        T v[LM_EPT];
#pragma unroll
        for (int e = 0; e < LM_EPT; ++e) {
            if (STREAM && e * LM_THREADS >= np) break;
            const int a = e * LM_THREADS + t, b = a + w < np ? a + w : a;
            v[e] = (!STREAM || a < np) ? lm_min(reg[a], reg[b]) : (T)1;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < LM_EPT; ++e) {
            if (STREAM && e * LM_THREADS >= np) break;
            reg[e * LM_THREADS + t] = v[e];
        }
        __syncthreads();
        w *= 2;
    }
    // d[delta] = 1 - m[k], k = n0 - Apad + 1 + delta: m[k] = min r[a .. a + W - 1] at a = delta + 1 - (Apad - A), two windows
    // of w; transposed in place through registers.  Entries in front of n0 - A + 1 meet zero weights only: 0.
    {
        const int shift = p.Apad - p.A;
        const int nd = STREAM ? (nout + TP_R - 1) / TP_R * TP_R + p.Apad : LM_DE * LM_THREADS;    // entries the sweeps read
        T d[LM_DE];
#pragma unroll
        for (int e = 0; e < LM_DE; ++e) {
            if (STREAM && e * LM_THREADS >= nd) break;
            const int a = e * LM_THREADS + t + 1 - shift;
            d[e] = (a >= 1 && a + W - 1 < np) ? (T)1 - lm_min(reg[a], reg[a + W - w]) : (T)0;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < LM_DE; ++e) {
            if (STREAM && e * LM_THREADS >= nd) break;
            const int dl = e * LM_THREADS + t;
            tp_win_at<TP_R, LM_SD>(reg, 0, dl) = d[e];
        }
        __syncthreads();
    }
    // s and g: 16 consecutive outputs per thread and sweep
    for (int sw = 0; sw * (int)TP_TILE < nout; ++sw) {
        const int o0 = sw * (int)TP_TILE + t * TP_R;
        T acc[TP_R];
#pragma unroll
        for (int e = 0; e < TP_R; ++e) acc[e] = (T)0;
        if (o0 < nout) {
#pragma unroll 1
            for (int jb = p.Apad - TP_R; jb >= 0; jb -= TP_R) {
                // weights j = jb + jj; output e reads d at o0 + cb + e + 15 - jj, cb = Apad - 16 - jb
                const int col = t + sw * LM_THREADS + (p.Apad - TP_R - jb) / TP_R;
                T dv[2 * TP_R - 1], wt[TP_R];
                tp_window<TP_R, LM_SD>(dv, reg, col);
                const tp_const_ptr<T> wp = (tp_const_ptr<T>)(p.w + jb);
#pragma unroll
                for (int jj = 0; jj < TP_R; ++jj) wt[jj] = wp[jj];
#pragma unroll
                for (int jj = TP_R - 1; jj >= 0; --jj)
#pragma unroll
                    for (int e = 0; e < TP_R; ++e) acc[e] = tp_fma(wt[jj], dv[e + TP_R - 1 - jj], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < TP_R; ++e) {
                if (o0 + e < nout) {
                    const int ix = lm_idx(o0 + e + p.A + p.H - 1);
                    T g = (T)1 - acc[e];
                    g = g > (T)0 ? g : (T)0;
                    rr[ix] = lm_min(g, rr[ix]);                  // only this thread reads or writes the word
                }
            }
        }
    }
    __syncthreads();
    for (int ch = 0; ch < p.channels; ++ch) {
        const auto xr = lm_row<T, STREAM>(p, grp * p.channels + ch);
        T *yr = p.y + (grp * p.channels + ch) * pitch + y0;
        for (int o = t; o < nout; o += LM_THREADS) {
            if constexpr (STREAM) yr[o] = n0 + o < 0 ? (T)0 : rr[lm_idx(o + p.A + p.H - 1)] * xr.at(n0 + o);
            else yr[o] = rr[lm_idx(o + p.A + p.H - 1)] * xr.xr[n0 + o];
        }
    }
    if (p.gain)
        for (int o = t; o < nout; o += LM_THREADS)
            p.gain[grp * pitch + y0 + o] = (STREAM && n0 + o < 0) ? (T)1 : rr[lm_idx(o + p.A + p.H - 1)];
}

struct LimiterPlan : InterpPlan {                 // zeros for up = 1
    int64_t tile, tiles, halo_left, halo_right, lds;
};

// everything but the pointers and the values of c and the window (host-only)
static LimiterPlan limiter_plan(const char *what, int dtype, int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    TFX_CHECK(up == 1 || up == 2 || up == 4 || up == 8, "%s: up must be 1, 2, 4 or 8, got %lld", what, (long long)up);
    TFX_CHECK(groups >= 0 && T >= 0, "%s: negative size", what);
    TFX_CHECK(channels >= 1 && channels <= (1 << 20), "%s: channels must be in [1, 2^20], got %lld", what, (long long)channels);
    TFX_CHECK(A >= 1 && A <= LM_A_MAX, "%s: look-ahead of %lld samples, the limit is 1 ... %lld", what, (long long)A,
              (long long)LM_A_MAX);
    TFX_CHECK(H >= 1 && H <= LM_H_MAX, "%s: hold of %lld samples, the limit is 1 ... %lld", what, (long long)H,
              (long long)LM_H_MAX);
    TFX_CHECK(T <= (INT64_MAX / 64) / up, "%s: T * up overflows", what);
    LimiterPlan pl{};
    if (up > 1) static_cast<InterpPlan &>(pl) = interp_plan(what, up, nh, T);
    pl.tile = LM_NR + 1 - 2 * A - H;
    pl.tiles = ceil_div(T, pl.tile);
    pl.halo_left = A + H - 1 + (up > 1 ? pl.LP - 1 - pl.i_lo : 0);
    pl.halo_right = A + pl.i_lo;
    pl.lds = (int64_t)(LM_PAD + LM_REGION) * (dtype == TFX_F32 ? 4 : 8);
    TFX_CHECK(groups == 0 || (T <= INT64_MAX / 16 / groups / channels && pl.tiles < (1ll << 31) / groups),
              "%s: size overflows", what);
    return pl;
}

static void limiter_check_values(const char *what, int dtype, double c, int64_t A, const void *window_host, int64_t up,
                                 const void *taps_host)
{
    TFX_CHECK(std::isfinite(c) && c > 0.0, "%s: the ceiling must be a finite linear value > 0, got %g", what, c);
    TFX_CHECK(window_host, "%s: no window", what);
    TFX_CHECK(up == 1 || taps_host, "%s: no taps", what);
    for (int64_t j = 0; j < A; ++j) {
        const double v = dtype == TFX_F32 ? (double)((const float *)window_host)[j] : ((const double *)window_host)[j];
        TFX_CHECK(std::isfinite(v) && v >= 0.0, "%s: window[%lld] = %g is negative or not finite", what, (long long)j, v);
    }
}

// every refusal of limiter_forward (host-only); hands back the plan it built on the way
static LimiterPlan limiter_check(const void *x, const void *y, int dtype, int64_t groups, int64_t channels, int64_t T, double c,
                                 int64_t A, int64_t H, const void *window_host, int64_t up, const void *taps_host, int64_t nh)
{
    const char *what = "limiter_forward";
    const LimiterPlan pl = limiter_plan(what, dtype, groups, channels, T, A, H, up, nh);
    limiter_check_values(what, dtype, c, A, window_host, up, taps_host);
    TFX_CHECK(groups * T == 0 || (x && y), "%s: null pointer", what);
    return pl;
}

void limiter_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh, int dtype,
                       int64_t *tile, int64_t *tiles, int64_t *halo_left, int64_t *halo_right, int64_t *Lp, int64_t *lds_bytes)
{
    const LimiterPlan pl = limiter_plan("limiter_forward", dtype, groups, channels, T, A, H, up, nh);
    *tile = pl.tile;
    *tiles = pl.tiles;
    *halo_left = pl.halo_left;
    *halo_right = pl.halo_right;
    *Lp = pl.g.Lp;
    *lds_bytes = pl.lds;
}

// the smoothing weights zero padded to a multiple of 16, by content
static PlanCache<DeviceBuffer, 2> g_windows(32, "limiter_forward");

template <typename T>
static void limiter_launch(const void *x, void *y, void *gain, int64_t groups, int64_t channels, int64_t T_, double c, int64_t A,
                           int64_t H, const void *window_host, int64_t up, const void *taps_host, int64_t nh,
                           const LimiterPlan &pl, hipStream_t stream, const StreamArgs *st = nullptr)
{
    std::shared_ptr<DeviceBuffer> table, window;
    LimiterArgs<T> p{};
    const int64_t Apad = ceil_div(A, TP_R) * TP_R;
    const int64_t tail[2] = {Apad, (int64_t)sizeof(T)};
    window = g_windows.get(window_host, (size_t)A * sizeof(T), tail, stream, [&] {
        std::vector<T> wv((size_t)Apad, (T)0);
        for (int64_t j = 0; j < A; ++j) wv[(size_t)j] = ((const T *)window_host)[j];
        return std::make_shared<DeviceBuffer>(wv);
    });
    p.x = (const T *)x; p.y = (T *)y; p.gain = (T *)gain; p.w = (const T *)window->p;
    p.T_ = T_; p.tiles = pl.tiles; p.up = up; p.channels = (int)channels; p.A = (int)A; p.Apad = (int)Apad; p.H = (int)H;
    p.tile = (int)pl.tile; p.c = (T)c;
    if (st) {                                   // T_ is the chunk's length; the kernel's T_ is where the stream ends so far
        p.hist = (const T *)st->hist_in; p.hist_out = (T *)st->hist_out;
        p.Tc = T_; p.N = st->N; p.Hs = st->Hs; p.n_in = st->n_in; p.D = (int)st->D;
        T_ = p.T_ = st->N + st->n_in;
    }
    if (up > 1) {
        p.hp = resample_table<T>(taps_host, nh, up, 1, pl.g.pre_pad, pl.LP, stream, &table);
        p.i_lo = pl.i_lo; p.n_lo = pl.g.pre_remove; p.n_hi = pl.g.pre_remove + T_ * up;
        p.rem = (int)(pl.g.pre_remove % up); p.xoff = (int)(pl.LP - 1 - pl.i_lo);
    }
    const auto launch = [&](auto lp) {
        const int64_t grid = groups * p.tiles;
        const size_t lds = (size_t)pl.lds;
        if (st) launch_dynamic_lds<limiter_kernel<T, lp(), true>>("limiter_stream_kernel", grid, LM_THREADS, lds, stream, p);
        else launch_dynamic_lds<limiter_kernel<T, lp(), false>>("limiter_kernel", grid, LM_THREADS, lds, stream, p);
    };
    if (up > 1) tp_dispatch(pl.LP, launch);
    else launch(std::integral_constant<int, 0>{});         // the sample peak
}

void limiter_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, double c,
                     int64_t A, int64_t H, const void *window_host, int64_t up, const void *taps_host, int64_t nh,
                     hipStream_t stream)
{
    const LimiterPlan pl = limiter_check(x, y, dtype, groups, channels, T, c, A, H, window_host, up, taps_host, nh);
    if (groups * T == 0) return;
    if (dtype == TFX_F32) limiter_launch<float>(x, y, gain, groups, channels, T, c, A, H, window_host, up, taps_host, nh, pl, stream);
    else limiter_launch<double>(x, y, gain, groups, channels, T, c, A, H, window_host, up, taps_host, nh, pl, stream);
}

// ---- the stream form ------------------------------------------------------------------------------------------------------
// Geometry of a stream (A, H, up, nh alone).  p[i] takes the interpolator's outputs of positions i - 1, i and i + 1's phases
// below rem: the newest input any of them reads is i + i_lo -- i + i_lo + 1 when rem >= 2 (with rem == 1 the one tap that
// meets it is the zero SciPy pads in front; with an odd-length design rem is 1) -- and the oldest i - 1 + i_lo - (Lp - 1).
// g[n] reads r over [n - A - H + 2, n + A - 1].  So output n is final once input n + D is in, D = A - 1 + forward reach, and
// the chunk that starts with output N - D reads back to N - D - (A + H - 2) - (Lp - i_lo).
struct LimiterStreamPlan {
    LimiterPlan pl;
    int64_t D, Hs, positions;
};

static LimiterStreamPlan limiter_stream_plan(int dtype, int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H,
                                             int64_t up, int64_t nh)
{
    LimiterStreamPlan sp{};
    sp.pl = limiter_plan("limiter_stream_forward", dtype, groups, channels, T, A, H, up, nh);
    const int64_t rem = up > 1 ? sp.pl.g.pre_remove % up : 0;
    const int64_t back = up > 1 ? std::max<int64_t>(1, sp.pl.g.Lp - sp.pl.i_lo) : 0;
    sp.D = A - 1 + sp.pl.i_lo + (rem >= 2 ? 1 : 0);
    sp.Hs = sp.D + A + H - 2 + back;
    sp.positions = std::min(T, sp.pl.tile) + 2 * A + H - 2;
    return sp;
}

void limiter_stream_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh, int dtype,
                              int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles, int64_t *positions,
                              int64_t *lds_bytes)
{
    const LimiterStreamPlan sp = limiter_stream_plan(dtype, groups, channels, T, A, H, up, nh);
    *latency = sp.D;
    *history = sp.Hs;
    *tile = sp.pl.tile;
    *tiles = sp.pl.tiles;
    *positions = sp.positions;
    *lds_bytes = sp.pl.lds;
}

void limiter_stream_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, int64_t n_in,
                            int64_t consumed, double c, int64_t A, int64_t H, const void *window_host, int64_t up,
                            const void *taps_host, int64_t nh, const void *hist_in, void *hist_out, hipStream_t stream)
{
    const char *what = "limiter_stream_forward";
    const LimiterStreamPlan sp = limiter_stream_plan(dtype, groups, channels, T, A, H, up, nh);
    limiter_check_values(what, dtype, c, A, window_host, up, taps_host);
    const int64_t rows = groups * channels;
    const size_t esz = dtype == TFX_F32 ? 4 : 8;
    StreamArgs st;
    if (!stream_enter(&st, what, esz, x, y, rows, T, n_in, consumed, sp.D, sp.Hs, hist_in, hist_out, stream)) return;
    // the gain track against the other buffers (an empty chunk has none)
    check_stream_buffers(what, esz, x, rows * T, gain, groups * T, hist_in, hist_out, rows * sp.Hs);
    check_stream_buffers(what, esz, y, rows * T, gain, groups * T, nullptr, nullptr, 0);
    if (dtype == TFX_F32)
        limiter_launch<float>(x, y, gain, groups, channels, T, c, A, H, window_host, up, taps_host, nh, sp.pl, stream, &st);
    else
        limiter_launch<double>(x, y, gain, groups, channels, T, c, A, H, window_host, up, taps_host, nh, sp.pl, stream, &st);
}

void limiter_clear() { g_windows.clear(); }

}  // namespace tfx
