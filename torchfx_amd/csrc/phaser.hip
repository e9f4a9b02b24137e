// phaser.hip -- the phaser: N first-order all-pass sections in series whose one coefficient an LFO sweeps every sample
// (tfx_phaser_forward; include/torchfx_hip.h has the definition step by step).  For the absolute sample n, every intermediate in
// float64 for both signal dtypes:
//   a[n]   = (g - 1) / (g + 1),  g = tan(w fc),  fc = min_freq exp(Lg (0.5 + 0.5 lfo(n)))         (lfo.h: the modulation effects' LFO)
//   x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1],  k = 1..N;      y[n] = dtype(dry x_0[n] + wet x_N[n])
// A stage is the affine recursion y -> c[n] y + b[n] with c[n] = -a[n] and b[n] = a[n] u[n] + u[n-1] (u the stage's input), so a run
// of samples acts on the incoming y as y -> C y + B with C the product of its c's: a scan.  Every stage has the same c[n], so the
// products the scan strides need are computed once per tile and serve all N stages.
//
// Work unit: scan_tile.h's, a unit being a row.  The N + 1 carries x_k[tile start - 1] are
// the values the last thread of the previous tile computed; they sit in 2 x 13 doubles of LDS (read as broadcasts), because a
// register array indexed by the stage counter would live in scratch memory.  A tile: x_0 through LDS with coalesced loads; a[n]
// once; the lane products of c and their Kogge-Stone prefix products over the wave; then per stage: b from the input and the sample
// in front (shuffle, the wave in front through LDS, the carry), a lane-local run over the 8 samples from nothing, the Kogge-Stone
// scan of B over the wave, the 4 wave totals through LDS, a second run from the true start.  Combines are ordered by position
// alone and read only what lies in front, so a sample's bits do not depend on values after it.
//
// segments == 1: one launch (pass C).  Otherwise two:
//   A  every segment but the last: the segment acts on the incoming (x_1[-1] .. x_N[-1]) as s -> M s + v.  M depends on the
//      coefficients alone and is lower-triangular Toeplitz (every stage is the same operator, and a state enters stage k exactly as
//      it enters stage 1).  The pass runs the segment twice in lockstep on one coefficient track: the real signal from a zero state
//      gives v, the zero signal from x_1[-1] = 1 gives the N distinct entries of M.  x_0[-1] is read from the signal itself.
//   C  every segment: composes the summaries in front of it (a short loop of triangular products), runs the stages, writes y.
// Both passes compute a[n] with the same code, so the numbers they compose are the same numbers.
#include "common.h"
#include "lfo.h"
#include "scan_tile.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)                            // the coefficient track rounds exactly as written; the recursion says fma()

namespace tfx {

constexpr int PH_MAXN = 12;
constexpr int64_t PH_AUTO_BLOCKS = 512, PH_AUTO_ROWS = 256;   // two workgroups per CU; the rows alone fill the chip

template <typename T> struct PhaserArgs {
    const T *x;                 // [rows, T_]
    T *y;                       // [rows, T_]
    double *coef;               // [coef_rows, T_] or null
    const double *state_in;     // [rows, N + 1] (x_0[-1] .. x_N[-1]) or null (silence)
    double *state_out;          // [rows, N + 1] or null
    double *scratch;            // [rows, segments, 2 N] (v, then M's first column); unused for segments == 1
    const int64_t *pos_in;      // DEVICE position of sample 0, null = pos
    int64_t *pos_out;           // receives the position + T_, or null
    int64_t pos;
    int channels, coef_rows, N;
    ScanCut cut;                // behind the ints: in front of them the float64 pass C reserves a stack slot for a scalar spill
    double inc, phase, spread, fmin, lg, w, dry, wet;
};

// steps 2 to 5 of the definition: (n, channel offset) -> a[n]
template <bool TRI> __device__ __forceinline__ double ph_coef(int64_t n, double off, double inc, double fmin, double lg, double w)
{
    const double l = lfo_at<TRI>(n, inc, off);
    const double fc = fmin * exp(lg * (0.5 + 0.5 * l));
    const double g = tan(w * fc);
    return (g - 1.0) / (g + 1.0);
}

// PASS 0 = A (two runs in lockstep: r = 0 the real signal from a zero state, r = 1 the zero signal from x_1[-1] = 1), 1 = C
template <typename T, bool TRI, int PASS>
__global__ void __launch_bounds__(ST_THREADS) phaser_kernel(const PhaserArgs<T> p)
{
    constexpr int R = PASS == 0 ? 2 : 1;
    __shared__ double slot[ST_PAD];
    __shared__ double wC[ST_WAVES], wB[R][ST_WAVES], wU[R][ST_WAVES];
    __shared__ double sC[2][R][PH_MAXN + 1];                         // the carries x_k[tile start - 1], by tile parity
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = p.N;
    const ScanSeg sg = scan_segment(p.cut, PASS == 1 ? p.cut.segments : p.cut.segments - 1);
    const int64_t row = sg.unit, tile0 = sg.tile0, ntile = sg.ntile, T_ = p.cut.T_;
    const int seg = sg.seg;
    const int64_t pos = p.pos_in ? *p.pos_in : p.pos;
    const T *xr = p.x + row * T_;
    const double z = p.phase + (double)(row % p.channels) * p.spread;
    const double off = z - floor(z);
    if (PASS == 1 && blockIdx.x == 0 && t == 0 && p.pos_out) *p.pos_out = pos + T_;

    // the carries at the segment's start
    {
        double s[PH_MAXN + 1];
        s[0] = tile0 == 0 ? (p.state_in ? p.state_in[row * (N + 1)] : 0.0) : (double)xr[tile0 * ST_TILE - 1];
#pragma unroll
        for (int k = 1; k <= PH_MAXN; ++k) s[k] = (PASS == 1 && p.state_in && k <= N) ? p.state_in[row * (N + 1) + k] : 0.0;
        if constexpr (PASS == 1) {
            // the state through the summaries of the segments in front: s <- M s + v, M[k][j] = m[k - j]
            const double *sc = p.scratch + row * p.cut.segments * 2 * N;
            for (int g = 0; g < seg; ++g) {
                const double *sv = sc + (int64_t)g * 2 * N, *sm = sv + N;
                double m[PH_MAXN];
#pragma unroll
                for (int i = 0; i < PH_MAXN; ++i) m[i] = i < N ? sm[i] : 0.0;
#pragma unroll
                for (int k = PH_MAXN; k >= 1; --k) {
                    if (k <= N) {
                        double acc = sv[k - 1];
#pragma unroll
                        for (int j = 1; j <= k; ++j) acc = fma(m[k - j], s[j], acc);
                        s[k] = acc;
                    }
                }
            }
        }
        if (t == 0) {
#pragma unroll
            for (int k = 0; k <= PH_MAXN; ++k) {
                sC[0][0][k] = s[k];
                if (R == 2) sC[0][R - 1][k] = k == 1 ? 1.0 : 0.0;
            }
        }
    }

    for (int64_t it = 0; it < ntile; ++it) {
        const int cur = (int)(it & 1), nxt = cur ^ 1;
        const int64_t n0 = (tile0 + it) * ST_TILE;
        // x_0, coalesced, into the slots
#pragma unroll
        for (int k = 0; k < ST_E; ++k) {
            const int a = k * ST_THREADS + t;
            const int64_t n = n0 + a;
            slot[st_sweep(a)] = n < T_ ? (double)xr[n] : 0.0;
        }
        // the coefficient of the lane's 8 samples, and what the scan of every stage needs of it: P[j] = the product of c = -a over
        // the 2^j lanes that end at this one, Pinc over the lanes 0 .. this one, Pex over the lanes in front
        const int64_t nl = n0 + (int64_t)t * ST_E;                   // the lane's first sample
        double a[ST_E];
#pragma unroll
        for (int e = 0; e < ST_E; ++e) a[e] = ph_coef<TRI>(pos + nl + e, off, p.inc, p.fmin, p.lg, p.w);
        if constexpr (PASS == 1) {
            if (p.coef && row < p.coef_rows) {
#pragma unroll
                for (int e = 0; e < ST_E; ++e)
                    if (nl + e < T_) p.coef[row * T_ + nl + e] = a[e];
            }
        }
        double P[6], Pinc = -a[0];
#pragma unroll
        for (int e = 1; e < ST_E; ++e) Pinc = Pinc * -a[e];
        scan_wave(Pinc, lane, [&](double up, double Pc, int j) {
            P[j] = Pc;
            return Pc * up;
        });
        const double Pex = scan_shfl_up(Pinc, 1);                    // lane 0: unused
        __syncthreads();                                             // the slots are full; the last tile's reads of wC, wU are over

        double u[R][ST_E];
#pragma unroll
        for (int e = 0; e < ST_E; ++e) {
            u[0][e] = slot[st_own(t, e)];
            if (R == 2) u[R - 1][e] = 0.0;
        }
        const bool last = PASS == 1 && p.state_out && n0 + ST_TILE >= T_;      // this tile holds the row's last sample
        if (last) {
#pragma unroll
            for (int e = 0; e < ST_E; ++e)
                if (nl + e == T_ - 1) p.state_out[row * (N + 1)] = u[0][e];
        }
        if (lane == 63) {
            wC[wave] = Pinc;
#pragma unroll
            for (int r = 0; r < R; ++r) wU[r][wave] = u[r][ST_E - 1];
        }
        if (t == ST_THREADS - 1) {
#pragma unroll
            for (int r = 0; r < R; ++r) sC[nxt][r][0] = u[r][ST_E - 1];
        }

        for (int k = 1; k <= N; ++k) {
            __syncthreads();                                         // wU and the carries of stage k - 1 are in place; wB is free
            double Bex[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                // b[n] = a[n] u[n] + u[n-1], in place of u from the back
                double up = __shfl_up(u[r][ST_E - 1], 1);
                if (lane == 0) up = wave == 0 ? sC[cur][r][k - 1] : wU[r][wave - 1];
#pragma unroll
                for (int e = ST_E - 1; e >= 1; --e) u[r][e] = fma(a[e], u[r][e], u[r][e - 1]);
                u[r][0] = fma(a[0], u[r][0], up);
                // the lane's 8 samples from nothing, then the lanes in front by strides
                double B = u[r][0];
#pragma unroll
                for (int e = 1; e < ST_E; ++e) B = fma(-a[e], B, u[r][e]);
                scan_wave(B, lane, [&](double Bp, double Bc, int j) { return fma(P[j], Bp, Bc); });
                Bex[r] = scan_shfl_up(B, 1);
                if (lane == 63) wB[r][wave] = B;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                // second run from the true start
                double yv = sC[cur][r][k];
#pragma unroll
                for (int w = 0; w < ST_WAVES - 1; ++w)
                    if (w < wave) yv = fma(wC[w], yv, wB[r][w]);
                if (lane > 0) yv = fma(Pex, yv, Bex[r]);
#pragma unroll
                for (int e = 0; e < ST_E; ++e) {
                    yv = fma(-a[e], yv, u[r][e]);
                    u[r][e] = yv;
                }
                if (lane == 63) wU[r][wave] = yv;
                if (t == ST_THREADS - 1) sC[nxt][r][k] = yv;
            }
            if (last) {
#pragma unroll
                for (int e = 0; e < ST_E; ++e)
                    if (nl + e == T_ - 1) p.state_out[row * (N + 1) + k] = u[0][e];
            }
        }

        if constexpr (PASS == 1) {
#pragma unroll
            for (int e = 0; e < ST_E; ++e) {
                const int i = st_own(t, e);
                slot[i] = p.dry * slot[i] + p.wet * u[0][e];
            }
            __syncthreads();
            T *yr = p.y + row * T_;
#pragma unroll
            for (int k = 0; k < ST_E; ++k) {
                const int i = k * ST_THREADS + t;
                const int64_t n = n0 + i;
                if (n < T_) yr[n] = (T)slot[st_sweep(i)];
            }
            __syncthreads();                                         // the slots are free again
        }
    }

    if constexpr (PASS == 0) {
        __syncthreads();
        const int fin = (int)(ntile & 1);
        double *sc = p.scratch + (row * p.cut.segments + seg) * 2 * N;
        if (t < N) sc[t] = sC[fin][0][t + 1];
        else if (t < 2 * N) sc[t] = sC[fin][1][t - N + 1];
    }
}

// an empty chunk still hands its position on
__global__ void phaser_position_kernel(const int64_t *pos_in, int64_t pos, int64_t *pos_out) { *pos_out = pos_in ? *pos_in : pos; }

// sizes alone (host-only); the two checks that are the phaser's own sit where callers have always met them, after the size checks
static ScanPlan phaser_plan(const char *what, int64_t rows, int64_t channels, int64_t T, int64_t stages, int64_t segments)
{
    scan_check_sizes(what, rows, channels, T);
    TFX_CHECK(rows % channels == 0, "%s: %lld rows do not split into items of %lld channels", what, (long long)rows, (long long)channels);
    TFX_CHECK(stages >= 1 && stages <= PH_MAXN, "%s: stages must be in [1, %d], got %lld", what, PH_MAXN, (long long)stages);
    return scan_plan(what, rows, 1, T, segments, PH_AUTO_BLOCKS, PH_AUTO_ROWS, 2 * stages * (int64_t)sizeof(double));
}

void phaser_plan_info(int64_t rows, int64_t channels, int64_t T, int64_t stages, int64_t segments, int64_t *tile, int64_t *tiles,
                      int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes)
{
    scan_plan_info(phaser_plan("phaser_plan_info", rows, channels, T, stages, segments), tile, tiles, segments_out, seg_tiles,
                   scratch_bytes);
}

void phaser_forward(const void *x, void *y, double *coef, int dtype, int64_t rows, int64_t channels, int64_t T, int64_t stages, double fs,
                    double rate, double min_freq, double max_freq, double phase, double spread, double dry, double wet, int shape,
                    int64_t position, const int64_t *pos_in, int64_t *pos_out, const double *state_in, double *state_out,
                    int64_t segments, void *scratch, hipStream_t stream)
{
    const char *what = "phaser_forward";
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    const ScanPlan pl = phaser_plan(what, rows, channels, T, stages, segments);
    TFX_CHECK(shape == TFX_LFO_SINE || shape == TFX_LFO_TRIANGLE, "%s: bad LFO shape %d", what, shape);
    TFX_CHECK(std::isfinite(fs) && fs > 0.0, "%s: the sample rate must be finite and > 0, got %g", what, fs);
    TFX_CHECK(min_freq >= 10.0 && min_freq <= max_freq && max_freq <= 0.45 * fs,
              "%s: need 10 Hz <= min_freq <= max_freq <= 0.45 fs = %g Hz, got %g and %g", what, 0.45 * fs, min_freq, max_freq);
    TFX_CHECK(rate > 0.0 && rate < 0.5 * fs, "%s: the rate must be in (0, fs / 2) = (0, %g) Hz, got %g", what, 0.5 * fs, rate);
    TFX_CHECK(std::isfinite(phase), "%s: the phase must be finite, got %g", what, phase);
    TFX_CHECK(std::isfinite(spread), "%s: spread must be finite, got %g", what, spread);
    TFX_CHECK(std::isfinite(dry), "%s: dry must be finite, got %g", what, dry);
    TFX_CHECK(std::isfinite(wet), "%s: wet must be finite, got %g", what, wet);
    TFX_CHECK(position >= 0 && position <= (1ll << 52), "%s: the position must be in [0, 2^52], got %lld", what, (long long)position);
    scan_check_buffers(what, pl, T, x, y, scratch, state_in, state_out);
    TFX_CHECK(!pos_out || pos_out != pos_in, "%s: the new position needs its own buffer", what);
    check_stream_buffers(what, dtype == TFX_F32 ? 4 : 8, x, rows * T, y, rows * T, nullptr, nullptr, 0);
    if (rows * T == 0) {                         // nothing in, nothing out: the state and the position move on unchanged
        scan_empty_chunk(rows, stages + 1, state_in, state_out, stream);
        if (pos_out) {
            hipLaunchKernelGGL(phaser_position_kernel, dim3(1), dim3(1), 0, stream, pos_in, position, pos_out);
            TFX_HIP(hipGetLastError());
        }
        return;
    }
    // the reduced parameters, as doubles on the host: inc = rate / fs, Lg = ln(max_freq / min_freq), w = pi / fs
    const double par[8] = {rate / fs, phase, spread, min_freq, std::log(max_freq / min_freq), M_PI / fs, dry, wet};
    auto run = [&](auto tag, auto tri) {
        using E = decltype(tag);
        PhaserArgs<E> p{};
        p.x = (const E *)x; p.y = (E *)y; p.coef = coef; p.state_in = state_in; p.state_out = state_out; p.scratch = (double *)scratch;
        p.pos_in = pos_in; p.pos_out = pos_out; p.pos = position;
        p.cut = scan_cut(pl, T);
        p.channels = (int)channels; p.coef_rows = (int)((spread == 0.0 || channels == 1) ? 1 : channels); p.N = (int)stages;
        p.inc = par[0]; p.phase = par[1]; p.spread = par[2]; p.fmin = par[3]; p.lg = par[4]; p.w = par[5]; p.dry = par[6]; p.wet = par[7];
        const ScanPass<PhaserArgs<E>> ladder[] = {{phaser_kernel<E, tri(), 0>, "phaser_pass_a"}, {phaser_kernel<E, tri(), 1>, "phaser_pass_c"}};
        scan_launch(ladder, p, pl, stream);
    };
    const bool tri = shape == TFX_LFO_TRIANGLE;
    if (dtype == TFX_F32) tri ? run(float{}, std::true_type{}) : run(float{}, std::false_type{});
    else tri ? run(double{}, std::true_type{}) : run(double{}, std::false_type{});
}

}  // namespace tfx
