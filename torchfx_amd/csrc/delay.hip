// delay.hip -- the BPM-synced multi-tap Delay (src/torchfx/effect.py:934-1538) as ONE launch per call:
//   wet[n] = sum_{i=1..taps} a_i * src[n - i*D]       (a_1 = 1, a_i = feedback^(i-1); taps whose position falls
//                                                      outside [0, T) are not added, as in the reference's slices)
//   dry[n] = n < T ? x[n] : 0
//   y[n]   = lerp(dry[n], wet[n], mix)                 n in [0, L), L = T + taps*D
// Mono: src = the row itself.  Ping-pong (consecutive row pairs): output row 1 sums the odd taps of row 0, output row 0 the
// even taps of row 1.  The composition the reference runs (`taps` multiplies, `taps` adds, a zero-pad copy and torch.lerp)
// reads each row ~2*taps+3 times; here every output sample is stored once and every input sample is read from HBM about
// once, so the floor is e*(T + L) bytes per row.
//
// Arithmetic = the composition's, in the signal dtype, so results are bit-identical to it on the device:
//   * the wet sum starts at +0.0 and adds fl(x * (T)a_i) in tap order; the product and the sum are rounded separately
//     (two kernels in the composition), so contraction is switched off in this file's tap loops (contract(off) below);
//   * the mix is ATen's lerp (ATen/native/Lerp.h, `|w| < 0.5 ? self + w*(end - self) : end - (end - self)*(1 - w)`) as
//     PyTorch's ROCm build compiles it: hipcc's default -ffp-contract=fast-honor-pragmas fuses each branch into one fma,
//     so lerp_mix spells those two fmas out.
// Three regimes (delay_regime): LATTICE for long delays (D >= 256, taps <= 8): a workgroup walks a block of residues
// n mod D down the row, one coalesced read per input sample, the last `taps` inputs in a register ring; SPAN for short
// spans (taps*D + tile in 64 KiB of LDS): a tile stages its window once and sums the taps from LDS; GATHER for anything
// else (correct, not fast): every tap is a global load.  The tile kernels walk each row in order on one XCD (bijective
// blockIdx remap), so the halo a tile re-reads was just read by its neighbour through the same L2.
#include "common.h"
#include "epilogue.h"
#include "plan_cache.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#pragma clang fp contract(off)

namespace tfx {

constexpr int DLY_THREADS = 256;
constexpr int DLY_E = 4;                                   // outputs per thread in the tile kernels
constexpr int64_t DLY_TILE = (int64_t)DLY_THREADS * DLY_E;
constexpr int DLY_ARG_AMPS = 64;                           // amplitudes passed by value; more go through a device buffer
constexpr int DLY_RING = 8;                                // LATTICE: taps held in registers
constexpr int64_t DLY_LAT_MIN_D = 256;
constexpr int64_t DLY_SPAN_LDS = 65536;
enum { DLY_SPAN = 0, DLY_LATTICE = 1, DLY_GATHER = 2 };

template <typename T> struct DelayArgs {
    const T *x;
    T *y;
    int64_t T_, L, D;
    int taps;
    T w;                        // mix, in the signal dtype (ATen's lerp takes the scalar weight as opmath = T)
    T gain;
    int scale, clamp, stat_mode, per_row;
    double *partial;            // [units * RU * groups] (per row) or [units * groups] (global)
    int64_t groups;             // workgroups per unit (row, or row pair)
    int64_t units, nwg;         // rows / pairs; workgroups in the grid
    int64_t tiles;              // SPAN / GATHER: tiles per row;  LATTICE: residue blocks per row
    int64_t kc, nchunks;        // LATTICE: k steps per chunk, chunks per residue block
    const double *a_dev;        // taps > DLY_ARG_AMPS: device [taps]; else null
    double a[DLY_ARG_AMPS];
};

template <typename T> __device__ __forceinline__ T amp(const DelayArgs<T> &p, int i)     // i = 1 .. taps
{
    return (T)(p.a_dev ? p.a_dev[i - 1] : p.a[i - 1]);
}

// (T)a is what torch multiplies by: a Python float scalar is converted to the tensor's opmath type
template <typename T> __device__ __forceinline__ T lerp_mix(T dry, T wet, T w)
{
    const T diff = wet - dry;
    return fabs(w) < (T)0.5 ? fma(w, diff, dry) : fma(-diff, (T)1 - w, wet);
}

template <typename T> __device__ __forceinline__ T epilogue_apply(const DelayArgs<T> &p, T v)
{
    if (p.scale) v = v * p.gain;
    if (p.clamp) v = clamp_unit(v);
    return v;
}

// first level of the statistic: one partial per workgroup and output row of the unit (RU rows)
template <typename T, int RU> __device__ void store_partials(const DelayArgs<T> &p, const double (&acc)[RU], int64_t unit, int64_t g)
{
    __shared__ double red[RU][DLY_THREADS / 64];
    const int mode = p.stat_mode;
#pragma unroll
    for (int c = 0; c < RU; ++c) {
        double v = acc[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = red_comb_rt(mode, v, __shfl_xor(v, off));
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
#pragma unroll
        for (int c = 0; c < RU; ++c) {
            const double s = red_comb_rt(mode, red_comb_rt(mode, red[c][0], red[c][1]), red_comb_rt(mode, red[c][2], red[c][3]));
            if (p.per_row) p.partial[(unit * RU + c) * p.groups + g] = s;
            else tot = c == 0 ? s : red_comb_rt(mode, tot, s);
        }
        if (!p.per_row) p.partial[unit * p.groups + g] = tot;
    }
}

// blockIdx -> logical workgroup: the workgroups that share an XCD (blockIdx % 8) take one contiguous range of tiles
__device__ __forceinline__ int64_t xcd_contiguous(int64_t id, int64_t n)
{
    const int64_t q = n / 8, r = n % 8, x = id % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + id / 8;
}

// ---- SPAN: the tile's window x[n0 - taps*D, n0 + TILE) of the unit's RU rows staged in LDS -----------------------------
template <typename T, bool PP>
__global__ void __launch_bounds__(DLY_THREADS) delay_span_kernel(const DelayArgs<T> p)
{
    constexpr int RU = PP ? 2 : 1;
    extern __shared__ unsigned char dly_lds_raw[];
    T *lds = (T *)dly_lds_raw;
    const int64_t lid = xcd_contiguous(blockIdx.x, p.nwg);
    const int64_t unit = lid / p.tiles, tile = lid % p.tiles;
    const int64_t S = (int64_t)p.taps * p.D, W = S + DLY_TILE;
    const int64_t n0 = tile * DLY_TILE, w0 = n0 - S;
#pragma unroll
    for (int c = 0; c < RU; ++c) {
        const T *xr = p.x + (unit * RU + c) * p.T_;
        for (int64_t j = threadIdx.x; j < W; j += DLY_THREADS) {
            const int64_t m = w0 + j;
            lds[c * W + j] = (m >= 0 && m < p.T_) ? xr[m] : (T)0;
        }
    }
    __syncthreads();
    double acc[RU];
#pragma unroll
    for (int c = 0; c < RU; ++c) acc[c] = 0.0;
#pragma unroll
    for (int c = 0; c < RU; ++c) {
        const T *src = lds + (PP ? (1 - c) : c) * W;       // ping-pong: the partner row feeds this one
        T wet[DLY_E];
#pragma unroll
        for (int e = 0; e < DLY_E; ++e) wet[e] = (T)0;
        for (int i = 1; i <= p.taps; ++i) {
            if (PP && ((i & 1) != c)) continue;              // odd taps -> row 1, even taps -> row 0
            const T a = amp(p, i);
            const int64_t back = (int64_t)i * p.D;
#pragma unroll
            for (int e = 0; e < DLY_E; ++e) {
                const int64_t n = n0 + e * DLY_THREADS + threadIdx.x, m = n - back;
                if (m >= 0 && m < p.T_) wet[e] = wet[e] + src[S + (n - n0) - back] * a;
            }
        }
        T *yr = p.y + (unit * RU + c) * p.L;
#pragma unroll
        for (int e = 0; e < DLY_E; ++e) {
            const int64_t n = n0 + e * DLY_THREADS + threadIdx.x;
            if (n < p.L) {
                const T dry = n < p.T_ ? lds[c * W + S + (n - n0)] : (T)0;
                const T v = epilogue_apply(p, lerp_mix(dry, wet[e], p.w));
                yr[n] = v;
                if (p.stat_mode >= 0) acc[c] = red_comb_rt(p.stat_mode, acc[c], red_elem_rt(p.stat_mode, (double)v));
            }
        }
    }
    if (p.stat_mode >= 0) store_partials<T, RU>(p, acc, unit, tile);
}

// ---- GATHER: every tap a global load (any D, any taps) -------------------------------------------------------------------
template <typename T, bool PP>
__global__ void __launch_bounds__(DLY_THREADS) delay_gather_kernel(const DelayArgs<T> p)
{
    const int64_t lid = xcd_contiguous(blockIdx.x, p.nwg);
    const int64_t row = lid / p.tiles, tile = lid % p.tiles;         // one output row per workgroup
    const int c = PP ? (int)(row & 1) : 0;
    const T *xr = p.x + row * p.T_;
    const T *src = PP ? p.x + (row ^ 1) * p.T_ : xr;
    T *yr = p.y + row * p.L;
    double acc[1] = {0.0};
#pragma unroll
    for (int e = 0; e < DLY_E; ++e) {
        const int64_t n = tile * DLY_TILE + e * DLY_THREADS + threadIdx.x;
        if (n >= p.L) continue;
        // taps that land inside [0, T): i in [i_lo, i_hi], walked in tap order
        int64_t i_lo = 1, i_hi = p.taps;
        if (p.D > 0) {
            i_hi = n / p.D < i_hi ? n / p.D : i_hi;
            const int64_t over = n - p.T_ + 1;                       // i*D >= over
            if (over > 0) i_lo = (over + p.D - 1) / p.D > 1 ? (over + p.D - 1) / p.D : 1;
        } else if (n >= p.T_) {
            // unreachable from delay_forward: D = 0 gives taps*D = 0, which delay_regime always sends to SPAN.  Kept so that
            // the kernel stays correct for any D on its own, and so that its instructions are the ones already measured.
            i_hi = 0;
        }
        T wet = (T)0;
        for (int64_t i = i_lo; i <= i_hi; ++i) {
            if (PP && ((int)(i & 1) != c)) continue;
            wet = wet + src[n - i * p.D] * amp(p, (int)i);
        }
        const T dry = n < p.T_ ? xr[n] : (T)0;
        const T v = epilogue_apply(p, lerp_mix(dry, wet, p.w));
        yr[n] = v;
        if (p.stat_mode >= 0) acc[0] = red_comb_rt(p.stat_mode, acc[0], red_elem_rt(p.stat_mode, (double)v));
    }
    if (p.stat_mode >= 0) store_partials<T, 1>(p, acc, row, tile);
}

// ---- LATTICE: residue classes n mod D, the last DLY_RING inputs of each lane in registers -----------------------------
// Workgroup = (unit, residue block rb, chunk): lanes r = rb*256 + lane (< D), k = chunk*kc ... (chunk+1)*kc - 1, n = k*D + r.
// Before its first step a chunk reads the `taps` inputs behind it (k - taps ... k - 1): that is the only input read twice.
template <typename T, bool PP>
__global__ void __launch_bounds__(DLY_THREADS) delay_lattice_kernel(const DelayArgs<T> p)
{
    constexpr int RU = PP ? 2 : 1;
    const int64_t lid = blockIdx.x;                  // consecutive blocks: neighbouring residues of the same chunk
    const int64_t per_unit = p.tiles * p.nchunks;
    const int64_t unit = lid / per_unit, g = lid % per_unit;
    const int64_t chunk = g / p.tiles, rb = g % p.tiles;
    const int64_t r = rb * DLY_THREADS + threadIdx.x;
    const bool lane_on = r < p.D;
    const T *xr[RU];
    T *yr[RU];
#pragma unroll
    for (int c = 0; c < RU; ++c) {
        xr[c] = p.x + (unit * RU + c) * p.T_;
        yr[c] = p.y + (unit * RU + c) * p.L;
    }
    T a[DLY_RING];
#pragma unroll
    for (int i = 1; i <= DLY_RING; ++i) a[i - 1] = i <= p.taps ? amp(p, i) : (T)0;
    const int64_t k0 = chunk * p.kc;
    // ring[c][j] = input of row c at step k - 1 - j (0 outside the row; such taps are also masked by position)
    T ring[RU][DLY_RING];
#pragma unroll
    for (int c = 0; c < RU; ++c)
#pragma unroll
        for (int j = 0; j < DLY_RING; ++j) {
            const int64_t m = (k0 - 1 - j) * p.D + r;
            ring[c][j] = (lane_on && j < p.taps && m >= 0 && m < p.T_) ? xr[c][m] : (T)0;
        }
    double acc[RU];
#pragma unroll
    for (int c = 0; c < RU; ++c) acc[c] = 0.0;
    const int64_t k1 = k0 + p.kc;
#pragma unroll 2
    for (int64_t k = k0; k < k1; ++k) {
        const int64_t n = k * p.D + r;
        if (k * p.D >= p.L) break;                   // uniform: no lane of this step is inside the output
        const bool out_on = lane_on && n < p.L;
        T cur[RU];
#pragma unroll
        for (int c = 0; c < RU; ++c) cur[c] = (out_on && n < p.T_) ? xr[c][n] : (T)0;
#pragma unroll
        for (int c = 0; c < RU; ++c) {
            T wet = (T)0;
#pragma unroll
            for (int i = 1; i <= DLY_RING; ++i) {
                if (PP && ((i & 1) != c)) continue;
                const int64_t m = n - (int64_t)i * p.D;
                if (i <= p.taps && m >= 0 && m < p.T_) wet = wet + ring[PP ? 1 - c : c][i - 1] * a[i - 1];
            }
            if (out_on) {
                const T v = epilogue_apply(p, lerp_mix(cur[c], wet, p.w));
                yr[c][n] = v;
                if (p.stat_mode >= 0) acc[c] = red_comb_rt(p.stat_mode, acc[c], red_elem_rt(p.stat_mode, (double)v));
            }
        }
#pragma unroll
        for (int c = 0; c < RU; ++c) {
#pragma unroll
            for (int j = DLY_RING - 1; j > 0; --j) ring[c][j] = ring[c][j - 1];
            ring[c][0] = cur[c];
        }
    }
    if (p.stat_mode >= 0) store_partials<T, RU>(p, acc, unit, g);
}

// ---- host ------------------------------------------------------------------------------------------------------------
int delay_regime(int64_t D, int64_t taps, int esz, int pingpong)
{
    const int64_t ru = pingpong ? 2 : 1, S = taps * D;
    const bool fits = S <= DLY_SPAN_LDS && ru * (S + DLY_TILE) * esz <= DLY_SPAN_LDS;
    const bool lattice = D >= DLY_LAT_MIN_D && taps <= DLY_RING;
    if (fits && S <= 4 * DLY_TILE) return DLY_SPAN;          // halo of at most four tiles
    if (lattice) return DLY_LATTICE;
    return fits ? DLY_SPAN : DLY_GATHER;
}

// the checks that need no pointer: delay_forward and the host-only delay_tiling_info share them
static void delay_check_sizes(const char *who, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps, int pingpong)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", who, dtype);
    TFX_CHECK(taps >= 1, "%s: taps must be at least 1, got %lld", who, (long long)taps);
    TFX_CHECK(delay >= 0, "%s: negative delay %lld", who, (long long)delay);
    TFX_CHECK(rows >= 0 && T >= 0, "%s: negative size", who);
    TFX_CHECK(!pingpong || rows % 2 == 0, "%s: ping-pong needs an even number of rows, got %lld", who, (long long)rows);
    TFX_CHECK(delay == 0 || taps <= (INT64_MAX / 2 - T) / delay, "%s: T + taps*delay overflows", who);
}

static void delay_check(const void *x, const void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                        const double *amps_host, double mix, int pingpong, const Epilogue *ep)
{
    delay_check_sizes("delay_forward", dtype, rows, T, delay, taps, pingpong);
    TFX_CHECK(amps_host, "delay_forward: null amplitudes");
    TFX_CHECK(mix == mix, "delay_forward: NaN mix");
    const int64_t L = T + taps * delay;
    TFX_CHECK((x || rows * T == 0) && (y || rows * L == 0), "delay_forward: null pointer");
    TFX_CHECK(!ep || ep->stat_mode < 0 || ep->stat_out, "delay_forward: statistic requested without an output buffer");
}

// The geometry of one launch.  LATTICE: `tiles` residue blocks of 256 lanes, the ceil(L / D) steps of a row cut into chunks of
// kc = 128 steps, halved down to 16 while the grid has fewer than 4096 workgroups.  SPAN / GATHER: tiles of DLY_TILE outputs.
DelayPlan delay_plan(int64_t rows, int64_t T, int64_t D, int64_t taps, int esz, int pingpong)
{
    DelayPlan q{};
    const int64_t ru = pingpong ? 2 : 1, L = T + taps * D;
    q.regime = delay_regime(D, taps, esz, pingpong);
    if (q.regime == DLY_LATTICE) {
        q.units = rows / ru;
        q.tiles = ceil_div(D, (int64_t)DLY_THREADS);
        const int64_t ksteps = ceil_div(L, D);
        q.kc = 128;
        while (q.kc > 16 && q.units * q.tiles * ceil_div(ksteps, q.kc) < 4096) q.kc /= 2;
        q.nchunks = ceil_div(ksteps, q.kc);
        q.groups = q.tiles * q.nchunks;
    } else {
        q.units = q.regime == DLY_SPAN ? rows / ru : rows;
        q.tiles = ceil_div(L, DLY_TILE);
        q.groups = q.tiles;
        if (q.regime == DLY_SPAN) q.lds_bytes = ru * (taps * D + DLY_TILE) * esz;
    }
    q.nwg = q.units * q.groups;
    return q;
}

void delay_tiling_info(int64_t rows, int64_t T, int64_t delay, int64_t taps, int dtype, int pingpong, int *regime, int64_t *units,
                       int64_t *tiles, int64_t *kc, int64_t *nchunks, int64_t *groups, int64_t *nwg, int64_t *lds_bytes)
{
    delay_check_sizes("delay_tiling_info", dtype, rows, T, delay, taps, pingpong);
    const DelayPlan q = delay_plan(rows, T, delay, taps, dtype == TFX_F32 ? 4 : 8, pingpong != 0);
    *regime = q.regime; *units = q.units; *tiles = q.tiles; *kc = q.kc; *nchunks = q.nchunks; *groups = q.groups; *nwg = q.nwg;
    *lds_bytes = q.lds_bytes;
}

// amplitude tables beyond the kernel arguments, by content
static PlanCache<DeviceBuffer, 1> g_amps(64, "delay_forward (more than 64 taps)");

template <typename T>
static void delay_launch(const void *x, void *y, int64_t rows, int64_t T_, int64_t D, int64_t taps, const double *amps_host,
                         double mix, int pingpong, const Epilogue &ep, hipStream_t stream)
{
    DelayArgs<T> p{};
    const int esz = sizeof(T), ru = pingpong ? 2 : 1;
    p.x = (const T *)x; p.y = (T *)y; p.T_ = T_; p.D = D; p.taps = (int)taps; p.L = T_ + taps * D;
    p.w = (T)mix; p.gain = (T)ep.gain; p.scale = ep.scale; p.clamp = ep.clamp; p.stat_mode = ep.stat_mode; p.per_row = ep.per_row;
    std::shared_ptr<DeviceBuffer> amps_dev;
    if (taps > DLY_ARG_AMPS) {
        const int64_t tail[1] = {taps};
        amps_dev = g_amps.get(amps_host, (size_t)taps * sizeof(double), tail, stream,
                              [&] { return std::make_shared<DeviceBuffer>(amps_host, (size_t)taps * sizeof(double)); });
        p.a_dev = (const double *)amps_dev->p;
    } else {
        for (int64_t i = 0; i < taps; ++i) p.a[i] = amps_host[i];
    }
    const DelayPlan q = delay_plan(rows, T_, D, taps, esz, pingpong);
    const int regime = q.regime;
    const size_t lds = (size_t)q.lds_bytes;
    p.units = q.units; p.tiles = q.tiles; p.kc = q.kc; p.nchunks = q.nchunks; p.groups = q.groups; p.nwg = q.nwg;
    TFX_CHECK(p.nwg < (1ll << 31), "delay_forward: grid too large");
    if (ep.stat_mode >= 0)
        p.partial = (double *)scratch("delay_partial", (size_t)(p.nwg * (ep.per_row ? ru : 1)) * sizeof(double), stream);
    const dim3 grid((unsigned)p.nwg), block(DLY_THREADS);
    {
        ProfScope ps(regime == DLY_LATTICE ? "delay_lattice_kernel" : regime == DLY_SPAN ? "delay_span_kernel" : "delay_gather_kernel",
                     stream);
        if (regime == DLY_LATTICE) {
            if (pingpong) hipLaunchKernelGGL((delay_lattice_kernel<T, true>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((delay_lattice_kernel<T, false>), grid, block, 0, stream, p);
        } else if (regime == DLY_SPAN) {
            if (pingpong) hipLaunchKernelGGL((delay_span_kernel<T, true>), grid, block, lds, stream, p);
            else hipLaunchKernelGGL((delay_span_kernel<T, false>), grid, block, lds, stream, p);
        } else {
            if (pingpong) hipLaunchKernelGGL((delay_gather_kernel<T, true>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((delay_gather_kernel<T, false>), grid, block, 0, stream, p);
        }
        TFX_HIP(hipGetLastError());
    }
    if (ep.stat_mode >= 0) {
        // per row: RU rows per unit, each with `groups` partials; global: every workgroup's partial
        if (ep.per_row) stat_finish(p.partial, rows, p.groups, ep.stat_mode, ep.stat_out, stream);
        else stat_finish(p.partial, 1, p.nwg, ep.stat_mode, ep.stat_out, stream);
    }
}

void delay_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                   const double *amps_host, double mix, int pingpong, const Epilogue *ep, hipStream_t stream)
{
    delay_check(x, y, dtype, rows, T, delay, taps, amps_host, mix, pingpong, ep);
    Epilogue none;
    const Epilogue &e = ep ? *ep : none;
    const int64_t L = T + taps * delay;
    if (rows == 0 || L == 0) {
        if (e.stat_mode >= 0 && (e.per_row ? rows : 1) > 0)
            TFX_HIP(hipMemsetAsync(e.stat_out, 0, (size_t)(e.per_row ? rows : 1) * 8, stream));
        return;
    }
    if (dtype == TFX_F32) delay_launch<float>(x, y, rows, T, delay, taps, amps_host, mix, pingpong, e, stream);
    else delay_launch<double>(x, y, rows, T, delay, taps, amps_host, mix, pingpong, e, stream);
}

// ---- streaming (StatefulDelay) ----------------------------------------------------------------------------------------
// One chunk of a continuous stream.  The chunk's rows sit behind the last H = taps*D input samples of each row (hist_in,
// null = silence); on that virtual row v = [hist_in | x] the chunk's outputs are the one-shot kernels' outputs at the
// chunk's positions, and flushing H zero samples gives the tail:
//   wet[n] = sum_{i=1..taps} a_i * src(n - i*D),  src(m) = m >= 0 ? x[m] : hist_in[H + m]   (n in [0, T), tap order)
//   y[n]   = lerp(x[n], wet[n], w);   hist_out = the newest H samples of v
// Exactness against the one-shot call on the whole signal: the wet sum starts at +0.0, and a history sample that stands for
// "before the signal" (silence at the start of the stream, or the zero chunk of a flush) adds fl(+0.0 * a_i) = +0.0 (a_i >= 0);
// a sum that starts at +0.0 is never -0.0 under round-to-nearest, and v + (+0.0) = v for every other v (NaN and Inf
// included), so those terms leave the bits of the sum where the one-shot kernel, which skips them, leaves them.  Every
// other term, the product rounding (contract(off) above) and lerp_mix are the one-shot kernels'.
// Regime: one coalesced gather kernel for every chunk size.  In the real-time regime (T <= D) each tap's sources are one
// contiguous run of the history, so reading taps*T samples and writing T is the floor; for T >> D the re-reads of a
// tap (taps*D samples behind) are served by L2, because the tiles of a row run in order on one XCD (xcd_contiguous, applied
// to the output tiles alone so that all eight XCDs share them however large the history is).
// The launch carries a second role: the workgroups past the output tiles write hist_out (no second launch).
constexpr int DLY_STR_E = 4;                               // history elements per thread
constexpr int64_t DLY_STR_OTILE = DLY_THREADS, DLY_STR_HTILE = (int64_t)DLY_THREADS * DLY_STR_E;

template <typename T> struct DelayStreamArgs {
    const T *x, *hist_in;       // [rows, T], [rows, H] or null
    T *y, *hist_out;            // [rows, T], [rows, H]
    int64_t T_, H, D;
    int taps;
    T w;
    int64_t otiles, htiles;     // output / history tiles per row
    int64_t rows, nwg;
    const double *a_dev;
    double a[DLY_ARG_AMPS];
};

template <typename T> __device__ __forceinline__ T amp(const DelayStreamArgs<T> &p, int i)
{
    return (T)(p.a_dev ? p.a_dev[i - 1] : p.a[i - 1]);
}

template <typename T, bool PP>
__global__ void __launch_bounds__(DLY_THREADS) delay_stream_kernel(const DelayStreamArgs<T> p)
{
    const int64_t n_out = p.rows * p.otiles;
    if ((int64_t)blockIdx.x < n_out) {
        // the output tiles are the first n_out blocks, remapped among themselves: every XCD gets a contiguous run of them
        const int64_t lid = xcd_contiguous(blockIdx.x, n_out);
        const int64_t row = lid / p.otiles, tile = lid % p.otiles;
        const int c = PP ? (int)(row & 1) : 0;
        const int64_t srow = PP ? (row ^ 1) : row;             // ping-pong: the partner row feeds this one
        const T *src = p.x + srow * p.T_;
        const T *hsrc = p.hist_in ? p.hist_in + srow * p.H + p.H : nullptr;     // hsrc[m], m in [-H, 0)
        const int64_t n = tile * DLY_STR_OTILE + threadIdx.x;
        if (n >= p.T_) return;
        T wet = (T)0;
        for (int i = 1; i <= p.taps; ++i) {
            if (PP && ((i & 1) != c)) continue;                  // odd taps -> row 1, even taps -> row 0
            const int64_t m = n - (int64_t)i * p.D;
            if (m >= 0) wet = wet + src[m] * amp(p, i);
            else if (hsrc) wet = wet + hsrc[m] * amp(p, i);
        }
        p.y[row * p.T_ + n] = lerp_mix(p.x[row * p.T_ + n], wet, p.w);
        return;
    }
    // second role: hist_out[row, j] = v[T + j], v = [hist_in | x] of the row
    const int64_t g = (int64_t)blockIdx.x - n_out, row = g / p.htiles, tile = g % p.htiles;
    const T *xr = p.x + row * p.T_;
    const T *hr = p.hist_in ? p.hist_in + row * p.H : nullptr;
    T *ho = p.hist_out + row * p.H;
#pragma unroll
    for (int e = 0; e < DLY_STR_E; ++e) {
        const int64_t j = tile * DLY_STR_HTILE + e * DLY_THREADS + threadIdx.x;
        if (j >= p.H) break;
        ho[j] = stream_hist_at(xr, hr, p.T_, p.H, j);
    }
}

static void delay_stream_check(const void *x, const void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                               const double *amps_host, double mix, int pingpong, const void *hist_in, const void *hist_out)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "delay_stream_forward: bad dtype %d", dtype);
    TFX_CHECK(taps >= 1, "delay_stream_forward: taps must be at least 1, got %lld", (long long)taps);
    TFX_CHECK(delay >= 0, "delay_stream_forward: negative delay %lld", (long long)delay);
    TFX_CHECK(rows >= 0 && T >= 0, "delay_stream_forward: negative size");
    TFX_CHECK(!pingpong || rows % 2 == 0, "delay_stream_forward: ping-pong needs an even number of rows, got %lld", (long long)rows);
    TFX_CHECK(amps_host, "delay_stream_forward: null amplitudes");
    TFX_CHECK(delay == 0 || taps <= (INT64_MAX / 4) / delay, "delay_stream_forward: taps*delay overflows");
    TFX_CHECK(mix == mix, "delay_stream_forward: NaN mix");
    const int64_t H = taps * delay;
    TFX_CHECK(rows == 0 || (T <= INT64_MAX / 4 / rows && H <= INT64_MAX / 4 / rows), "delay_stream_forward: size overflows");
    TFX_CHECK((x || rows * T == 0) && (y || rows * T == 0) && (hist_out || rows * H == 0), "delay_stream_forward: null pointer");
    check_stream_buffers("delay_stream_forward", dtype == TFX_F32 ? 4 : 8, x, rows * T, y, rows * T, hist_in, hist_out, rows * H);
}

template <typename T>
static void delay_stream_launch(const void *x, void *y, int64_t rows, int64_t T_, int64_t D, int64_t taps, const double *amps_host,
                                double mix, int pingpong, const void *hist_in, void *hist_out, hipStream_t stream)
{
    DelayStreamArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.hist_in = (const T *)hist_in; p.hist_out = (T *)hist_out;
    p.T_ = T_; p.D = D; p.taps = (int)taps; p.H = taps * D; p.w = (T)mix; p.rows = rows;
    std::shared_ptr<DeviceBuffer> amps_dev;
    if (taps > DLY_ARG_AMPS) {
        const int64_t tail[1] = {taps};
        amps_dev = g_amps.get(amps_host, (size_t)taps * sizeof(double), tail, stream,
                              [&] { return std::make_shared<DeviceBuffer>(amps_host, (size_t)taps * sizeof(double)); });
        p.a_dev = (const double *)amps_dev->p;
    } else {
        for (int64_t i = 0; i < taps; ++i) p.a[i] = amps_host[i];
    }
    p.otiles = ceil_div(T_, DLY_STR_OTILE);
    p.htiles = ceil_div(p.H, DLY_STR_HTILE);
    p.nwg = rows * (p.otiles + p.htiles);
    if (p.nwg == 0) return;
    TFX_CHECK(p.nwg < (1ll << 31), "delay_stream_forward: grid too large");
    ProfScope ps("delay_stream_kernel", stream);
    if (pingpong) hipLaunchKernelGGL((delay_stream_kernel<T, true>), dim3((unsigned)p.nwg), dim3(DLY_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((delay_stream_kernel<T, false>), dim3((unsigned)p.nwg), dim3(DLY_THREADS), 0, stream, p);
    TFX_HIP(hipGetLastError());
}

void delay_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                          const double *amps_host, double mix, int pingpong, const void *hist_in, void *hist_out, hipStream_t stream)
{
    delay_stream_check(x, y, dtype, rows, T, delay, taps, amps_host, mix, pingpong, hist_in, hist_out);
    if (dtype == TFX_F32) delay_stream_launch<float>(x, y, rows, T, delay, taps, amps_host, mix, pingpong, hist_in, hist_out, stream);
    else delay_stream_launch<double>(x, y, rows, T, delay, taps, amps_host, mix, pingpong, hist_in, hist_out, stream);
}

void delay_clear() { g_amps.clear(); }

}  // namespace tfx
