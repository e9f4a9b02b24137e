// modulation.hip -- the modulated delay line behind Chorus, Flanger and Vibrato, ONE launch per call (or per chunk of a stream):
//   y[n] = dtype(dry * x[n] + sum_v g_v * xd_v[n]),   xd_v[n] = x(n - d_v[n]) read by linear or 4-point Lagrange interpolation,
//   d_v[n] = base_v + depth_v * lfo(frac(n * inc_v) + off_{v,c}),   off_{v,c} = frac(phase_v + c * spread),  c = row mod channels
// with every intermediate in float64 for both signal dtypes (include/torchfx_hip.h, tfx_modulated_delay_forward, has the
// definition step by step).  The effect is feed-forward: an output sample reads at most H = max_v floor(base_v + depth_v) + 2
// samples back and none ahead, so tiles and chunks are exact and a row's bits depend on neither.
//
// Work unit: a workgroup of 256 threads owns (tile of 1024 samples, channel index c, up to MD_BATCH batch items).  Lanes own
// neighbouring samples (thread t: tile_base + e * 256 + t), so a wave's reads for one voice cover 64 + 3 consecutive elements
// (the delay moves by depth * 2 pi * inc << 1 sample per sample) and coalesce straight from global memory; the other voices'
// re-reads of the same lines come from cache.  No LDS.  The delay (i, f) and the interpolation weights depend on (n, v, c) alone,
// not on the batch item: they are computed once and applied to the workgroup's batch items in turn -- the float64 sinpi is the
// expensive part.  That reuse is bit-neutral: every batch item runs the same expressions on the same (i, f).
//
// mod_delay_at is the one place (n, voice, channel) becomes (i, f); mod_tile is the one place outputs are computed.  The one-shot
// kernel and the stream kernel both call mod_tile, so a stream cannot drift from the one-shot call.  Contraction is off in this
// file: t = double(n) * inc must stay one IEEE multiplication (a fused n * inc - floor(t) moves the LFO phase by up to 2e-5
// samples of delay at n = 2^40), and with it off every expression below rounds exactly as written, on the device and the host.
// Plain vector stores only; nothing crosses between workgroups.
#include "common.h"
#include "lfo.h"
#include "plan_cache.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>

#pragma clang fp contract(off)

namespace tfx {

constexpr int MD_THREADS = 256;
constexpr int MD_E = 4;                                    // samples per thread and tile
constexpr int64_t MD_TILE = (int64_t)MD_THREADS * MD_E;
constexpr int MD_BATCH = 4;                                // batch items a workgroup applies one (i, f) to
constexpr int MD_MAXV = 8;
constexpr int64_t MD_MAX_REACH = 1ll << 24;

struct ModVoice {
    double base, depth, inc, gain;
};

template <typename T> struct ModArgs {
    const T *x, *hist_in;       // [rows, T]; [rows, H] or null (one-shot, or silence)
    T *y, *hist_out;            // [rows, T]; [rows, H] (stream only)
    const int64_t *pos_in;      // stream: DEVICE position of the chunk's first sample, null = 0
    int64_t *pos_out;           // stream: receives pos_in + T
    int64_t pos;                // one-shot: the position as a host scalar
    int64_t T_, H;
    int64_t batch, channels, rows;
    int64_t tiles, n_out;       // output tiles per row; output workgroups = tiles * channels * batch groups
    int64_t htiles;             // stream: history tiles per row
    int V;
    double dry;
    const ModVoice *voice;      // DEVICE [V]
    const double *off;          // DEVICE [channels, V]: off[c * V + v] = frac(phase_v + c * spread), computed on the host
};

// (n, voice, channel offset) -> the delay d = i + f, i = floor(d), f in [0, 1)
template <bool TRI>
__device__ __forceinline__ void mod_delay_at(int64_t n, const ModVoice &vc, double off, int64_t &i, double &f)
{
    const double l = lfo_at<TRI>(n, vc.inc, off);           // lfo.h: shared with the phaser
    const double d = vc.base + vc.depth * l;
    const double fl = floor(d);
    i = (int64_t)fl;
    f = d - fl;
}

// sample m of a row's [hr (H samples) | xr (T_ samples)] as float64; 0 outside it (before the stream's first sample, and --
// unreachable for a delay within the argument rules -- at or past T_)
template <typename T>
__device__ __forceinline__ double mod_read(const T *xr, const T *hr, int64_t T_, int64_t H, int64_t m)
{
    if (m >= 0) return m < T_ ? (double)xr[m] : 0.0;
    return (hr && m >= -H) ? (double)hr[H + m] : 0.0;
}

// the interpolation weights for x[m+1], x[m], x[m-1], x[m-2] (m = n - i) at f; linear uses w[1], w[2] as (unused, f)
template <bool CUBIC> __device__ __forceinline__ void mod_weights(double f, double (&w)[4])
{
    if (CUBIC) {
        const double fp = f + 1.0, fm = f - 1.0, f2 = f - 2.0;
        w[0] = -f * fm * f2 * (1.0 / 6.0);
        w[1] = fp * fm * f2 * 0.5;
        w[2] = -fp * f * f2 * 0.5;
        w[3] = fp * f * fm * (1.0 / 6.0);
    } else {
        w[0] = w[1] = w[3] = 0.0;
        w[2] = f;
    }
}

template <typename T, bool CUBIC>
__device__ __forceinline__ double mod_tap(const T *xr, const T *hr, int64_t T_, int64_t H, int64_t m, const double (&w)[4])
{
    const double x0 = mod_read(xr, hr, T_, H, m), x1 = mod_read(xr, hr, T_, H, m - 1);
    if (!CUBIC) return x0 + w[2] * (x1 - x0);
    const double xm = mod_read(xr, hr, T_, H, m + 1), x2 = mod_read(xr, hr, T_, H, m - 2);
    return w[0] * xm + w[1] * x0 + w[2] * x1 + w[3] * x2;
}

// output workgroup `lid` of the launch: (tile, channel index, batch group), pos = the absolute position of sample 0
template <typename T, bool CUBIC, bool TRI>
__device__ __forceinline__ void mod_tile(const ModArgs<T> &p, int64_t lid, int64_t pos)
{
    const int64_t tile = lid % p.tiles, rest = lid / p.tiles;
    const int64_t c = rest % p.channels, b0 = (rest / p.channels) * MD_BATCH;
    const int nb = (int)(p.batch - b0 < MD_BATCH ? p.batch - b0 : MD_BATCH);
    const double *off = p.off + c * p.V;
    const int64_t row0 = b0 * p.channels + c;                // batch item b of the group: row0 + b * channels
    for (int e = 0; e < MD_E; ++e) {
        const int64_t j = tile * MD_TILE + (int64_t)e * MD_THREADS + threadIdx.x;
        if (j >= p.T_) break;
        double acc[MD_BATCH];
#pragma unroll
        for (int b = 0; b < MD_BATCH; ++b)
            acc[b] = b < nb ? p.dry * (double)p.x[(row0 + b * p.channels) * p.T_ + j] : 0.0;
        for (int v = 0; v < p.V; ++v) {
            int64_t i;
            double f, w[4];
            const ModVoice vc = p.voice[v];
            mod_delay_at<TRI>(pos + j, vc, off[v], i, f);
            mod_weights<CUBIC>(f, w);
            const double g = vc.gain;
#pragma unroll
            for (int b = 0; b < MD_BATCH; ++b) {
                if (b < nb) {
                    const int64_t row = row0 + b * p.channels;
                    const T *hr = p.hist_in ? p.hist_in + row * p.H : nullptr;
                    acc[b] = acc[b] + g * mod_tap<T, CUBIC>(p.x + row * p.T_, hr, p.T_, p.H, j - i, w);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < MD_BATCH; ++b)
            if (b < nb) p.y[(row0 + b * p.channels) * p.T_ + j] = (T)acc[b];
    }
}

template <typename T, bool CUBIC, bool TRI>
__global__ void __launch_bounds__(MD_THREADS) modulated_delay_kernel(const ModArgs<T> p)
{
    mod_tile<T, CUBIC, TRI>(p, blockIdx.x, p.pos);
}

// One chunk of a stream.  The first n_out workgroups are the output tiles; the ones past them write hist_out, the newest H
// samples of [hist_in | x] (which also covers chunks shorter than H), and one lane of the first of them stores the new position.
template <typename T, bool CUBIC, bool TRI>
__global__ void __launch_bounds__(MD_THREADS) modulated_delay_stream_kernel(const ModArgs<T> p)
{
    const int64_t pos = p.pos_in ? *p.pos_in : 0;
    if ((int64_t)blockIdx.x < p.n_out) {
        mod_tile<T, CUBIC, TRI>(p, blockIdx.x, pos);
        return;
    }
    const int64_t g = (int64_t)blockIdx.x - p.n_out;
    if (g == 0 && threadIdx.x == 0 && p.pos_out) *p.pos_out = pos + p.T_;
    const int64_t row = g / p.htiles, tile = g % p.htiles;
    if (row >= p.rows) return;
    const T *xr = p.x + row * p.T_;
    const T *hr = p.hist_in ? p.hist_in + row * p.H : nullptr;
    T *ho = p.hist_out + row * p.H;
    for (int e = 0; e < MD_E; ++e) {
        const int64_t j = tile * MD_TILE + (int64_t)e * MD_THREADS + threadIdx.x;
        if (j >= p.H) break;
        ho[j] = stream_hist_at(xr, hr, p.T_, p.H, j);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
struct ModPlan {
    int64_t rows, tiles, bgroups, n_out, H;
};

// sizes and the voice table (host-only): every argument error of both entries that does not need a pointer
static ModPlan mod_plan(const char *what, int dtype, int64_t batch, int64_t channels, int64_t T, const double *voices, int64_t V,
                        double spread, double dry, int shape, int interp)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    TFX_CHECK(V >= 1 && V <= MD_MAXV, "%s: the number of voices must be in [1, %d], got %lld", what, MD_MAXV, (long long)V);
    TFX_CHECK(shape == TFX_LFO_SINE || shape == TFX_LFO_TRIANGLE, "%s: bad LFO shape %d", what, shape);
    TFX_CHECK(interp == TFX_INTERP_LINEAR || interp == TFX_INTERP_CUBIC, "%s: bad interpolation %d", what, interp);
    TFX_CHECK(batch >= 0 && T >= 0, "%s: negative size", what);
    TFX_CHECK(channels >= 1 && channels <= (1 << 20), "%s: channels must be in [1, 2^20], got %lld", what, (long long)channels);
    TFX_CHECK(batch == 0 || T <= INT64_MAX / 16 / batch / channels, "%s: size overflows", what);
    TFX_CHECK(voices, "%s: null voice table", what);
    TFX_CHECK(std::isfinite(spread), "%s: spread must be finite, got %g", what, spread);
    TFX_CHECK(std::isfinite(dry), "%s: dry must be finite, got %g", what, dry);
    const double lowest = interp == TFX_INTERP_CUBIC ? 1.0 : 0.0;
    ModPlan pl{};
    for (int64_t v = 0; v < V; ++v) {
        const double base = voices[5 * v], depth = voices[5 * v + 1], inc = voices[5 * v + 2], phase = voices[5 * v + 3],
                     gain = voices[5 * v + 4];
        TFX_CHECK(std::isfinite(base) && base >= 0.0, "%s: voice %lld: the delay must be finite and >= 0 samples, got %g", what,
                  (long long)v, base);
        TFX_CHECK(std::isfinite(depth) && depth >= 0.0, "%s: voice %lld: the depth must be finite and >= 0 samples, got %g", what,
                  (long long)v, depth);
        TFX_CHECK(base - depth >= lowest, "%s: voice %lld: delay - depth must be >= %g samples for %s interpolation, got %g - %g", what,
                  (long long)v, lowest, interp == TFX_INTERP_CUBIC ? "cubic" : "linear", base, depth);
        TFX_CHECK(std::floor(base + depth) + 3.0 <= (double)MD_MAX_REACH,
                  "%s: voice %lld: delay + depth must stay below 2^24 - 3 samples, got %g", what, (long long)v, base + depth);
        TFX_CHECK(inc > 0.0 && inc < 0.5, "%s: voice %lld: rate / fs must be in (0, 0.5), got %g", what, (long long)v, inc);
        TFX_CHECK(std::isfinite(phase), "%s: voice %lld: the phase must be finite, got %g", what, (long long)v, phase);
        TFX_CHECK(std::isfinite(gain), "%s: voice %lld: the gain must be finite, got %g", what, (long long)v, gain);
        pl.H = std::max(pl.H, (int64_t)std::floor(base + depth) + 2);
    }
    pl.rows = batch * channels;
    pl.tiles = ceil_div(T, MD_TILE);
    pl.bgroups = ceil_div(batch, MD_BATCH);
    TFX_CHECK(pl.tiles == 0 || pl.bgroups * channels < (1ll << 30) / pl.tiles, "%s: grid too large", what);
    pl.n_out = pl.tiles * channels * pl.bgroups;
    return pl;
}

void modulated_delay_plan_info(int64_t batch, int64_t channels, int64_t T, const double *voices_host, int64_t V, int interp,
                               int64_t *tile, int64_t *tiles, int64_t *history, int64_t *batch_items, int64_t *batch_groups)
{
    const ModPlan pl = mod_plan("modulated_delay_plan_info", TFX_F32, batch, channels, T, voices_host, V, 0.0, 0.0, TFX_LFO_SINE, interp);
    *tile = MD_TILE;
    *tiles = pl.tiles;
    *history = pl.H;
    *batch_items = MD_BATCH;
    *batch_groups = pl.bgroups;
}

// The launch's table, built on the host in float64 and cached on the device by its bytes: the V voices, then
// off[c, v] = frac(phase_v + c * spread).  A first use uploads it with a blocking copy, so it cannot happen inside a capture.
static PlanCache<DeviceBuffer, 2> g_tables(64, "modulated_delay_forward");

// the launch's arguments but for its signal pointers
template <typename T>
static std::shared_ptr<DeviceBuffer> mod_fill(ModArgs<T> &p, const ModPlan &pl, int64_t batch, int64_t channels, int64_t T_,
                                              const double *voices, int64_t V, double spread, double dry, hipStream_t stream)
{
    p.T_ = T_; p.H = pl.H; p.batch = batch; p.channels = channels; p.rows = pl.rows; p.tiles = pl.tiles; p.n_out = pl.n_out;
    p.V = (int)V; p.dry = dry;
    std::vector<double> tab((size_t)(4 * V + channels * V));
    for (int64_t v = 0; v < V; ++v) {
        tab[4 * v] = voices[5 * v]; tab[4 * v + 1] = voices[5 * v + 1]; tab[4 * v + 2] = voices[5 * v + 2]; tab[4 * v + 3] = voices[5 * v + 4];
    }
    for (int64_t c = 0; c < channels; ++c)
        for (int64_t v = 0; v < V; ++v) {
            const double z = voices[5 * v + 3] + (double)c * spread;
            tab[(size_t)(4 * V + c * V + v)] = z - std::floor(z);
        }
    const int64_t tail[2] = {V, channels};
    std::shared_ptr<DeviceBuffer> keep =
        g_tables.get(tab.data(), tab.size() * sizeof(double), tail, stream, [&] { return std::make_shared<DeviceBuffer>(tab); });
    p.voice = (const ModVoice *)keep->p;
    p.off = (const double *)keep->p + 4 * V;
    return keep;
}

template <typename T, bool STREAM>
static void mod_launch(const ModArgs<T> &p, int64_t nwg, int shape, int interp, hipStream_t stream)
{
    ProfScope ps(STREAM ? "modulated_delay_stream_kernel" : "modulated_delay_kernel", stream);
    const dim3 grid((unsigned)nwg), block(MD_THREADS);
#define MD_GO(CUBIC, TRI)                                                                                              \
    do {                                                                                                               \
        if (STREAM) hipLaunchKernelGGL((modulated_delay_stream_kernel<T, CUBIC, TRI>), grid, block, 0, stream, p);     \
        else hipLaunchKernelGGL((modulated_delay_kernel<T, CUBIC, TRI>), grid, block, 0, stream, p);                   \
    } while (0)
    const bool cubic = interp == TFX_INTERP_CUBIC, tri = shape == TFX_LFO_TRIANGLE;
    if (cubic && tri) MD_GO(true, true);
    else if (cubic) MD_GO(true, false);
    else if (tri) MD_GO(false, true);
    else MD_GO(false, false);
#undef MD_GO
    TFX_HIP(hipGetLastError());
}

template <typename T>
static void mod_forward(const void *x, void *y, const ModPlan &pl, int64_t batch, int64_t channels, int64_t T_, const double *voices,
                        int64_t V, double spread, double dry, int shape, int interp, int64_t position, hipStream_t stream)
{
    ModArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.pos = position;
    const std::shared_ptr<DeviceBuffer> keep = mod_fill(p, pl, batch, channels, T_, voices, V, spread, dry, stream);
    p.H = 0;                                                  // no history: reads before sample 0 give 0
    mod_launch<T, false>(p, pl.n_out, shape, interp, stream);
}

void modulated_delay_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T, const double *voices_host,
                             int64_t V, double spread, double dry, int shape, int interp, int64_t position, hipStream_t stream)
{
    const char *what = "modulated_delay_forward";
    const ModPlan pl = mod_plan(what, dtype, batch, channels, T, voices_host, V, spread, dry, shape, interp);
    TFX_CHECK(position >= 0 && position <= (1ll << 52), "%s: the position must be in [0, 2^52], got %lld", what, (long long)position);
    TFX_CHECK(pl.rows * T == 0 || (x && y), "%s: null pointer", what);
    check_stream_buffers(what, dtype == TFX_F32 ? 4 : 8, x, pl.rows * T, y, pl.rows * T, nullptr, nullptr, 0);
    if (pl.n_out == 0) return;
    if (dtype == TFX_F32) mod_forward<float>(x, y, pl, batch, channels, T, voices_host, V, spread, dry, shape, interp, position, stream);
    else mod_forward<double>(x, y, pl, batch, channels, T, voices_host, V, spread, dry, shape, interp, position, stream);
}

template <typename T>
static void mod_stream(const void *x, void *y, const ModPlan &pl, int64_t batch, int64_t channels, int64_t T_, const double *voices,
                       int64_t V, double spread, double dry, int shape, int interp, const void *hist_in, void *hist_out,
                       const int64_t *pos_in, int64_t *pos_out, hipStream_t stream)
{
    ModArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.hist_in = (const T *)hist_in; p.hist_out = (T *)hist_out;
    p.pos_in = pos_in; p.pos_out = pos_out;
    p.htiles = ceil_div(pl.H, MD_TILE);
    const int64_t hwg = std::max<int64_t>(pl.rows * p.htiles, pos_out ? 1 : 0);       // an empty chunk still moves the position
    if (pl.n_out + hwg == 0) return;
    TFX_CHECK(pl.n_out + hwg < (1ll << 31), "modulated_delay_stream_forward: grid too large");
    const std::shared_ptr<DeviceBuffer> keep = mod_fill(p, pl, batch, channels, T_, voices, V, spread, dry, stream);
    mod_launch<T, true>(p, pl.n_out + hwg, shape, interp, stream);
}

void modulated_delay_stream_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T,
                                    const double *voices_host, int64_t V, double spread, double dry, int shape, int interp,
                                    const void *hist_in, void *hist_out, const int64_t *pos_in, int64_t *pos_out, hipStream_t stream)
{
    const char *what = "modulated_delay_stream_forward";
    const ModPlan pl = mod_plan(what, dtype, batch, channels, T, voices_host, V, spread, dry, shape, interp);
    TFX_CHECK(pl.rows == 0 || pl.H <= INT64_MAX / 16 / pl.rows, "%s: size overflows", what);
    TFX_CHECK((pl.rows * T == 0 || (x && y)) && (pl.rows == 0 || hist_out), "%s: null pointer", what);
    TFX_CHECK(!pos_out || pos_out != pos_in, "%s: the new position needs its own buffer", what);
    check_stream_buffers(what, dtype == TFX_F32 ? 4 : 8, x, pl.rows * T, y, pl.rows * T, hist_in, hist_out, pl.rows * pl.H);
    if (dtype == TFX_F32)
        mod_stream<float>(x, y, pl, batch, channels, T, voices_host, V, spread, dry, shape, interp, hist_in, hist_out, pos_in, pos_out,
                          stream);
    else
        mod_stream<double>(x, y, pl, batch, channels, T, voices_host, V, spread, dry, shape, interp, hist_in, hist_out, pos_in, pos_out,
                           stream);
}

void modulation_clear() { g_tables.clear(); }

}  // namespace tfx
